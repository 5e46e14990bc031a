"""What every case of tests/periodic_cases.py claims, proved on the CPU with the reference alone (tests/periodic_ref.py), and the
negative controls of the check the GPU tests use.  Nothing here passes emptily: in every case at least 10 % of the self rows AND at
least 10 % of the query rows have a neighbour across the seam — but for the one case that says it exists for its queries only, where
the floor holds for the query rows — and the non-periodic table fails the check against the wrapped matrix.

The accuracy claim of the periodic `MeshJet` is at the end, on the fp64 restatement of tests/jet_ref.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import jet_ref as J                      # noqa: E402
import periodic_ref as P                 # noqa: E402
from periodic_cases import CASES, IDS    # noqa: E402
from oracle import knn_ref as K          # noqa: E402

SLACK = K.NONPERIODIC


def tables(case):
    pos, k, per = case["pos"], case["k"], case["period"]
    D_self, D_q = P.distances(pos, per), P.distances(pos, per, case["queries"])
    return D_self, P.brute_force_table(D_self, k), D_q, P.brute_force_table(D_q, k)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_is_dyadic_tie_free_and_crosses_the_seam(case):
    pos, k, per, q = case["pos"], case["k"], case["period"], case["queries"]
    assert (pos.astype(np.float64) * 2 ** 16 % 1 == 0).all() and (q.astype(np.float64) * 2 ** 16 % 1 == 0).all()
    assert pos.shape[0] <= 3000 and len({tuple(r) for r in pos.tolist()}) == pos.shape[0]
    D_self, T_self, D_q, T_q = tables(case)
    # no exact tie among the k + 2 nearest: the table is unique, order included
    assert K.tie_free(D_self, k + 1, **SLACK) and K.tie_free(D_q, k + 1, **SLACK), case["name"]
    o, L = P.frame(pos, per)
    cross_self = P.crosses(pos, pos, T_self.numpy(), L)
    cross_q = P.crosses(pos, P.wrap32(q, o, L), T_q.numpy(), L)
    print(f"{case['name']}: {100 * cross_self.mean():.1f} % of the self rows and {100 * cross_q.mean():.1f} % of the query rows cross the seam")
    # the tables differ from the non-periodic ones
    t = torch.from_numpy(pos)
    plain, plain_q = K.brute_force_table(t, t, k + 1)[:, 1:], K.brute_force_table(t, torch.from_numpy(P.wrap32(q, o, L)), k)
    differ_self, differ_q = float((T_self != plain).any(1).float().mean()), float((T_q != plain_q).any(1).float().mean())
    assert cross_q.mean() >= 0.10 and differ_q >= 0.10 and cross_self.any(), (case["name"], cross_q.mean(), differ_q)
    if not case.get("queries_only"):          # (the floor on each table of its own)
        assert cross_self.mean() >= 0.10 and differ_self >= 0.10, (case["name"], cross_self.mean(), differ_self)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_case_reaches_the_grid_and_the_rings_it_claims(case):
    pos, k, per, q = case["pos"], case["k"], case["period"], case["queries"]
    o, L, cells, nc = P.grid(pos, k, per)
    if "nc" in case:
        assert tuple(int(v) for v in nc) == tuple(case["nc"]), nc
    for a in range(pos.shape[1]):
        if L[a] > 0:
            assert abs(nc[a] * cells[a] - float(L[a])) <= 1e-15 * float(L[a]) and float(L[a]) >= float(pos[:, a].max() - pos[:, a].min())
    Rs, ws, ss = P.rings_needed(pos, k, per)
    Rq, wq, sq = P.rings_needed(pos, k, per, q)
    print(f"{case['name']}: cells {nc.tolist()}, rings self {int(Rs.max())} query {int(Rq.max())}, whole {int(ws.sum() + wq.sum())}, "
          f"split {int(ss.sum() + sq.sum())}")
    assert max(int(Rs.max()), int(Rq.max())) >= case.get("rings", 1)
    if case.get("whole"):
        assert ws.any() or wq.any()
    if case.get("split"):
        assert ss.any() and sq.any()
    if case.get("rings", 1) >= 2:          # the second ring is needed ACROSS the seam
        o, L = P.frame(pos, per)
        T_q = P.brute_force_table(P.distances(pos, per, q), k)
        assert (P.crosses(pos, P.wrap32(q, o, L), T_q.numpy(), L) & (Rq >= 2)).any()


def test_the_cases_cover_the_small_grids_and_the_axis_combinations():
    counts, combos = set(), set()
    for case in CASES:
        o, L, cells, nc = P.grid(case["pos"], case["k"], case["period"])
        counts |= {int(nc[a]) for a in range(len(nc)) if L[a] > 0}
        combos.add((len(nc), tuple(bool(v > 0) for v in L)))
    assert {1, 2, 3, 4} <= counts, counts
    assert {(2, (True, False)), (2, (False, True)), (2, (True, True)), (3, (True, True, True))} <= combos
    assert any(d == 3 and sum(p) == 1 for d, p in combos)
    assert any(c["far"] for c in CASES) and any(isinstance(d, float) and d > float(np.ptp(c["pos"][:, a])) + 0.1
                                                for c in CASES for a, d in enumerate(c["period"]))


def test_far_queries_wrap_onto_their_originals_bit_for_bit():
    for case in CASES:
        if not case["far"]:
            continue
        o, L = P.frame(case["pos"], case["period"])
        w = P.wrap32(case["queries"], o, L)
        n = case["far"]
        assert (w[-n:] == w[:n]).all() and (case["queries"][-n:] != case["queries"][:n]).any()
        lo = o.astype(np.float64)
        for a in range(len(L)):
            if L[a] > 0:
                assert (w[:, a] >= lo[a]).all() and (w[:, a] < lo[a] + float(L[a])).all()


def test_wrap_loop_on_awkward_values():
    """Not dyadic: whatever the rounding, the result is within one period's ulp of [o, o + L) and a fixed function of the input."""
    rng = np.random.default_rng(0)
    o, L = np.array([0.1, -3.3], np.float32), np.array([0.7, 2.9], np.float32)
    q = (rng.standard_normal((4000, 2)) * 40).astype(np.float32)
    q[:8, 0] = [0.1, 0.8, np.nextafter(np.float32(0.8), np.float32(0)), np.nextafter(np.float32(0.1), np.float32(0)), -0.6, 1.5, 0.0999999, 0.45]
    w = P.wrap32(q, o, L)
    top = (o + L).astype(np.float32)
    for a in range(2):
        assert (w[:, a] >= np.nextafter(o[a], np.float32(-np.inf))).all() and (w[:, a] <= top[a]).all()
        shift = (w[:, a].astype(np.float64) - q[:, a].astype(np.float64)) / float(L[a])
        assert np.abs(shift - np.round(shift)).max() < 1e-4
    assert (P.wrap32(w, o, L) == w).mean() > 0.999


def test_the_wrap_is_always_finite_and_says_when_it_stood_in():
    """The rule the kernels rely on for their addresses (include/g4c.h): wherever the sequence overflows or meets a value that is not
    finite the result is the origin, and `wraps_finite` — the tracers' test — is False exactly there."""
    o, L = np.array([0.25, -1.0], np.float32), np.array([0.5, 3.0], np.float32)
    big = np.float32(np.finfo(np.float32).max)
    q = np.array([[2e38, 0.0], [-2e38, 0.0], [big, 0.0], [np.inf, 0.0], [-np.inf, 0.0], [np.nan, 0.0], [0.0, np.inf], [0.0, -np.inf], [0.0, np.nan],
                  [1.8e38, 0.0], [0.3, 1.0], [1e30, 1e30], [-7.75, 100.5]], np.float32)
    w, ok = P.wrap32(q, o, L), P.wraps_finite(q, o, L)
    assert np.isfinite(w).all()
    assert ok.tolist() == [False] * 10 + [True] * 3          # (1.8e38 / 0.5 overflows although 1.8e38 is finite; 1e30 wraps, inexactly)
    assert (w[:6, 0] == o[0]).all() and (w[6:9, 1] == o[1]).all() and w[9, 0] == o[0]
    assert (w[10] == q[10]).all() and o[0] <= w[12, 0] < o[0] + L[0] and o[1] <= w[12, 1] < o[1] + L[1]
    # a period of 1 or more does not overflow the quotient of a finite q − o
    assert P.wraps_finite(np.array([[0.0, 3e38]], np.float32), o, L)[0]


# ---------------------------------------------------------------------- negative controls
@pytest.mark.parametrize("case", [CASES[0], CASES[6], CASES[8]], ids=[IDS[0], IDS[6], IDS[8]])
def test_negative_controls(case):
    pos, k, per, q = case["pos"], case["k"], case["period"], case["queries"]
    D_self, T_self, D_q, T_q = tables(case)
    K.assert_knn(D_self, T_self, k, **SLACK)
    K.assert_knn(D_q, T_q, k, **SLACK, self_mode=False)
    # the non-periodic brute-force tables are no k-nearest tables of the wrapped matrix
    t = torch.from_numpy(pos)
    assert K.violations(D_self, K.brute_force_table(t, t, k + 1)[:, 1:].contiguous(), k, **SLACK)
    o, L = P.frame(pos, per)
    plain_q = K.brute_force_table(t, torch.from_numpy(P.wrap32(q, o, L)), k)
    assert K.violations(D_q, plain_q, k, **SLACK, self_mode=False)
    # a perturbed correct table fails as well
    assert "ascending" in K.violations(D_self, K.swap_two_tiers(D_self, T_self, k, **SLACK), k, **SLACK)
    assert K.violations(D_self, K.replace_kth_by_farther(D_self, T_self, k, **SLACK), k, **SLACK) >= {"near"}
    assert "range" in K.violations(D_self, K.repeat_index(T_self), k, **SLACK)
    assert K.violations(D_q, K.replace_kth_by_farther(D_q, T_q, k, **SLACK), k, **SLACK, self_mode=False)


# ---------------------------------------------------------------------- the accuracy claim, on the fp64 restatement
SEAM_RATIO_THRESHOLD = 1.066         # halfway between the two ratios measured below (tests/PERIODIC_MEASURED.md records them)


def _laplacian_errors(period):
    """(relative rms error of the Laplacian at the nodes within two spacings of a periodic face, the same in the interior, the
    stencil table) on 2 000 random nodes of [0, 1) x [0, 0.5), k = 12, power 2, f = sin(2 pi x) cos(4 pi y): the fp64 restatement of
    tests/jet_ref.py on the brute-force tables, one-sided (`period` None) or wrapped with periods (1, 0.5)."""
    rng = np.random.default_rng(0)
    pos = (rng.random((2000, 2)) * np.array([1.0, 0.5])).astype(np.float32)
    n, k = pos.shape[0], 12
    t = torch.from_numpy(pos)
    if period is None:
        T, L = K.brute_force_table(t, t, k + 1)[:, 1:].numpy(), np.zeros(2, np.float32)
    else:
        T, L = P.brute_force_table(P.distances(pos, period), k).numpy(), np.array(period, np.float32)
    off = np.arange(0, n * k + 1, k, dtype=np.int32)
    src = T.reshape(-1).astype(np.int32)
    c64 = J.weights(off, None, src, P.rel32(pos, T, L), 2, 2)[0]
    p64 = pos.astype(np.float64)
    f = np.sin(2 * np.pi * p64[:, 0]) * np.cos(4 * np.pi * p64[:, 1])
    jets = J.jets64(f[:, None], off, c64, src)[:, 0, :]
    lap = jets[:, 2] + jets[:, 4]
    exact = -(4 + 16) * np.pi ** 2 * f
    spacing = np.sqrt(0.5 / n)
    band = (p64[:, 0] < 2 * spacing) | (p64[:, 0] > 1 - 2 * spacing) | (p64[:, 1] < 2 * spacing) | (p64[:, 1] > 0.5 - 2 * spacing)
    scale = np.sqrt((exact ** 2).mean())
    err = lap - exact
    return np.sqrt((err[band] ** 2).mean()) / scale, np.sqrt((err[~band] ** 2).mean()) / scale, T


def test_the_wrapped_stencil_keeps_the_seam_as_accurate_as_the_interior():
    seam_1, interior_1, T_1 = _laplacian_errors(None)
    seam_p, interior_p, T_p = _laplacian_errors((1.0, 0.5))
    changed = int((T_1 != T_p).any(1).sum())
    print(f"one-sided: seam {seam_1:.4f} interior {interior_1:.4f} ratio {seam_1 / interior_1:.4f}; wrapped: seam {seam_p:.4f} interior "
          f"{interior_p:.4f} ratio {seam_p / interior_p:.4f}; {changed} of 2000 stencils change")
    assert changed >= 200
    assert seam_p / interior_p < SEAM_RATIO_THRESHOLD < seam_1 / interior_1
