"""The restatement of g4c_weighted_integrals_adjoint (tests/integrals_adjoint_ref.py) against the restatement of the forward
(tests/integrals_ref.py: `terms`), on the host: `adjoint64` before its cast equals the central difference of

    F(x) = Σ_i Σ_e g[q_i, e] · terms(x)[i, e]          (summed with math.fsum)

in every column of every row.  F is quadratic in x, so the central difference IS the derivative — any step, no truncation — up to the
rounding of the two evaluations: each addend g · (w · (z_a · z_b)) carries three roundings and fsum one more, so an evaluation is
within 4 · 2⁻⁵³ Σ|addends of F| of its exact value, and the quotient within 4 · 2⁻⁵³ (Σ|F₊| + Σ|F₋|) / (2 h); the adjoint itself within
the second part of its own `bound`.  The samples sit on a grid of 2⁻⁸ and h = 1/2, so x ± h are float32 exactly (`terms` reads
float32) and so is x − sub in fp64."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import integrals_adjoint_ref as A          # noqa: E402
import integrals_ref as R                  # noqa: E402

H = 0.5
N, LD = 11, 6


def inputs(nz, sub, strided, groups, t, seed):
    rng = np.random.default_rng(seed)
    steps = t + 1
    x_step = nz + 1 if strided else 0
    grid = lambda shape: (rng.integers(-1024, 1025, shape) / 256.0).astype(np.float32)          # noqa: E731
    x = grid((N, x_step * steps + 2 if strided else LD))
    s = grid((N, LD + 1)) if sub else None
    w = rng.random(N)
    w[3] = 0.0
    G = max(groups, 1)
    group = rng.integers(0, G, N).astype(np.int32) if groups else None
    return x, s, w, group, G, x_step


def forward(x, s, w, entries, g, group, x_step, t):
    """(F, Σ|addends|)."""
    T, keep = R.terms(x, w, entries, s, x_step, 0, t)
    q = np.zeros(N, dtype=np.int64) if group is None else group.astype(np.int64)
    add = (g[q] * T)[keep].ravel().tolist()
    return math.fsum(add), math.fsum(abs(v) for v in add)


@pytest.mark.parametrize("nz,entries", [
    (3, [(0, 1), (2, 2), (1, -1), (-1, -1), (-1, 2), (0, 0), (1, 0), (2, 0)]),          # every form, column 0 named by several
    (4, [(0, 0)]),                                                                      # a == b alone: two adds; columns named by none
    (4, [(1, 3), (3, 1), (-1, 3)]),
    (1, [(0, 0), (0, -1), (-1, 0), (-1, -1)]),
])
@pytest.mark.parametrize("sub", [False, True])
@pytest.mark.parametrize("groups", [0, 3])
@pytest.mark.parametrize("strided,t", [(False, 0), (True, 2)])
def test_the_adjoint_is_the_derivative_of_the_forward(nz, entries, sub, groups, strided, t):
    x, s, w, group, G, x_step = inputs(nz, sub, strided, groups, t, seed=7 * nz + len(entries) + 100 * groups + t)
    ne = len(entries)
    g = np.random.default_rng(5).standard_normal((G, ne))
    acc, addends = A.adjoint64(x, w, entries, g, s, x_step, 0, t, group, nz)
    assert acc.shape == (N, nz)
    worst = 0.0
    for i in range(N):
        for c in range(nz):
            col = x_step * t + c
            xp, xm = x.copy(), x.copy()
            xp[i, col] += np.float32(H)
            xm[i, col] -= np.float32(H)
            assert float(xp[i, col]) - float(x[i, col]) == H and float(x[i, col]) - float(xm[i, col]) == H
            fp, ap = forward(xp, s, w, entries, g, group, x_step, t)
            fm, am = forward(xm, s, w, entries, g, group, x_step, t)
            want = (fp - fm) / (2 * H)
            tol = 4 * 2.0 ** -53 * (ap + am) / (2 * H) + 2.0 * (2 * ne + 4) * 2.0 ** -53 * addends[i, c]
            err = abs(acc[i, c] - want)
            worst = max(worst, err / tol if tol > 0 else (0.0 if err == 0 else math.inf))
            assert err <= tol, (i, c, acc[i, c], want, tol)
    print(f"largest |adjoint64 − central difference| / tolerance = {worst:.3e}")
    assert not acc[3].any() and not np.signbit(acc[3]).any()          # the row of zero weight: +0
    named = {c for e in entries for c in e if c >= 0}
    for c in set(range(nz)) - named:
        assert not acc[:, c].any()          # a column named by no entry: +0


def test_the_two_adds_of_a_square_are_kept_apart():
    """a == b == c: two addends gw · z, added one after the other — not one addend 2 gw z (the same value here, but the order is the
    promise) — and a column of −1 reads 1.0."""
    x = np.array([[3.0, 5.0]], np.float32)
    acc, addends = A.adjoint64(x, [2.0], [(0, 0), (1, -1), (-1, 1)], [[7.0, 11.0, 13.0]])
    assert acc.tolist() == [[2 * 7.0 * 2.0 * 3.0, 11.0 * 2.0 + 13.0 * 2.0]]
    assert addends.tolist() == [[84.0, 48.0]]


def test_rows_outside_the_groups_and_of_zero_weight_are_plus_zero():
    x = np.full((4, 2), np.nan, np.float32)
    x[0] = 1.0
    acc, _ = A.adjoint64(x, [1.0, 0.0, 1.0, 1.0], [(0, 1)], np.ones((2, 1)), group=np.array([1, 0, 2, -1], np.int32))
    assert acc[0].tolist() == [1.0, 1.0]
    assert not acc[1:].any() and not np.signbit(acc[1:]).any() and not np.isnan(acc).any()


def test_cast_and_bound():
    assert A.cast(np.array([1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, 1e300, -1e300])).tolist() == [1.0, 1.0 + 2.0 ** -22, math.inf, -math.inf]
    b = A.bound(np.array([2.0]), np.array([4.0]), 3)
    assert b[0] == 2.0 ** -23 + 2 * 10 * 2.0 ** -53 * 4.0


def test_cases_cover_what_the_device_test_promises():
    cs = dict(A.cases())
    assert {c["x"].shape[0] for c in cs.values()} >= {1, 255, 256, 257} and max(c["x"].shape[0] for c in cs.values()) > A.MAX_ROWS_A_PASS
    assert {len(c["entries"]) for c in cs.values()} == set(range(1, 9))
    assert {c["nz"] for c in cs.values()} == {1, 3, 4, 5, 9}
    assert any(c["x_step"] and c["t"] > 0 for c in cs.values()) and any(c["sub_step"] and c["t"] > 0 for c in cs.values())
    assert any(c["group"] is None for c in cs.values())
    assert any(c["group"] is not None and (c["group"] >= 3).any() and (c["group"] < 0).any() for c in cs.values())
    assert all(np.isnan(c["x"][c["w"] == 0.0]).any() for c in cs.values() if c["x"].shape[0] > 200)
    forms = set()
    for c in cs.values():
        forms |= {("one", "one") if a < 0 and b < 0 else ("col", "one") if b < 0 else ("one", "col") if a < 0 else ("sq",) if a == b else ("ab",)
                  for a, b in c["entries"]}
    assert len(forms) == 5
