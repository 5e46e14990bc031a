"""The numpy restatement of the point sampler (tests/sampler_ref.py) against itself and against the mathematics, on the host: the fp32
loop within its bound of the fp64 apply, the identities of the fp64 coefficients (partition of unity, linear exactness inside and
outside the hull, exact hits, Shepard's weights where the neighbours cannot span the space), and the precondition of the GPU weight
test — no point of its clouds sits near the degeneracy threshold, so the device's flags must equal the restatement's.

Bounds.  The apply: (k + 3) 2^-24 Σ_j |c_j x_j| — k product roundings and k − 1 additions, with a margin of 4.  The identities hold in
exact arithmetic; in fp64 the coefficients carry the roundings of some tens of operations per neighbour (2^-53 each), amplified by the
conditioning of the normal matrix, which 1 / ratio bounds (ratio = det M / (tr M / dim)^dim <= 1): allowed = 256 k 2^-53 Σ|terms| / ratio
per point."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sampler_ref as R          # noqa: E402

RATIOS = {}


def note(name, r):
    RATIOS[name] = max(RATIOS.get(name, 0.0), float(r))


def cases(ks=R.WEIGHT_K, clouds=R.WEIGHT_CLOUDS):
    for dim in (2, 3):
        for n in clouds:
            for k in ks[dim]:
                yield dim, n, k


def identity_bound(k, ratio, mag):
    with np.errstate(all="ignore"):
        return 256.0 * k * 2.0 ** -53 * mag / ratio[:, None]


def test_fp32_apply_stays_within_its_bound_of_the_fp64_apply():
    rng = np.random.default_rng(5)
    for dim, n, k in cases():
        pos, q = R.cloud(n, dim), R.queries(257, dim)
        idx = R.nearest(pos, q, k)
        for power in R.POWERS:
            c32 = R.coefficients(pos, q, idx, power)[1]
            for nf in (1, 3, 37):
                x = rng.standard_normal((n, nf)).astype(np.float32)
                val, mag = R.apply64(x, idx, c32)
                note("host: |apply32 - apply64| / ((k + 3) 2^-24 sum|c x|)", R.within(R.apply32(x, idx, c32), val, R.bound32(mag, k), f"dim {dim} n {n} k {k}"))
    # negative control: one coefficient off by an ulp of the largest is seen
    c_bad = c32.copy()
    c_bad[:, 0] += np.float32(2.0 ** -10)
    assert R.rejects(R.within, R.apply32(x, idx, c_bad), val, R.bound32(mag, k))


IDENTITY_K = {2: (3, 6, 8, 16), 3: (4, 8, 10, 16)}          # k = dim + 1 belongs here only: its fits are exact and badly conditioned


def test_the_coefficients_sum_to_one_and_reproduce_linear_fields():
    rng = np.random.default_rng(6)
    outside = 0
    for dim, n, k in cases(IDENTITY_K, (65, 257, 1000)):
        pos, q = R.cloud(n, dim), R.queries(257, dim)
        idx = R.nearest(pos, q, k)
        slope, const = rng.standard_normal((dim, 3)), rng.standard_normal(3)
        x = pos.astype(np.float64) @ slope + const                      # fp64 values of three linear fields at the nodes
        want = q.astype(np.float64) @ slope + const
        outside += int(((q < 0) | (q > 1)).any(1).sum())
        for power in R.POWERS:
            c64, c32, dist, degen, ratio = R.coefficients(pos, q, idx, power)
            assert not degen.any() and (ratio > 0).all(), (dim, n, k, power)
            what = f"dim {dim} n {n} k {k} power {power}"
            note("host: |sum c - 1| / (256 k 2^-53 sum|c| / ratio)",
                 R.within(c64.sum(1, keepdims=True), np.ones((257, 1)), identity_bound(k, ratio, np.abs(c64).sum(1, keepdims=True)), what))
            val, mag = R.apply64(x, idx, c64)
            note("host: |linear field - sample| / (256 k 2^-53 sum|c x| / ratio)", R.within(val, want, identity_bound(k, ratio, mag), what))
            # the nearest node's distance, from the same differences
            d0 = np.sqrt(((pos.astype(np.float64)[idx[:, 0]] - q.astype(np.float64)) ** 2).sum(1))
            assert R.ulps32(dist, d0.astype(np.float32)) <= 1
    assert outside > 100          # points outside the hull were among them
    # negative control: a quadratic field is not reproduced
    val, mag = R.apply64((pos.astype(np.float64) ** 2).sum(1, keepdims=True), idx, c64)
    assert R.rejects(R.within, val, (q.astype(np.float64) ** 2).sum(1, keepdims=True), identity_bound(k, ratio, mag))


def test_an_exact_hit_returns_the_nodes_row_bit_for_bit():
    rng = np.random.default_rng(7)
    for dim, n, k in cases():
        pos = R.cloud(n, dim)
        rows = rng.integers(0, n, 33)
        q = pos[rows].copy()
        idx = R.nearest(pos, q, k)
        assert (idx[:, 0] == rows).all()
        x = rng.standard_normal((n, 5)).astype(np.float32)
        for power in R.POWERS:
            c64, c32, dist, degen, ratio = R.coefficients(pos, q, idx, power)
            assert (c32[:, 0] == 1).all() and (c32[:, 1:] == 0).all() and not degen.any() and (dist == 0).all() and np.isnan(ratio).all()
            R.same(R.apply32(x, idx, c32), x[rows], f"dim {dim} n {n} k {k}")


def test_too_few_neighbours_give_shepards_weights():
    for dim in (2, 3):
        pos, q = R.cloud(65, dim), R.queries(257, dim)
        for k in range(1, dim + 1):
            idx = R.nearest(pos, q, k)
            for power in R.POWERS:
                c64, c32, dist, degen, ratio = R.coefficients(pos, q, idx, power)
                assert degen.all()
                d = pos.astype(np.float64)[idx] - q.astype(np.float64)[:, None, :]
                r2 = (d ** 2).sum(2)
                w = np.ones_like(r2) if power == 0 else r2 ** (-0.5 * power)
                assert np.allclose(c64, w / w.sum(1, keepdims=True), rtol=1e-14, atol=0) and np.allclose(c64.sum(1), 1.0, rtol=1e-14)
    # collinear neighbours in 2-D: the threshold, not the count, decides
    line = np.stack([np.linspace(0, 1, 9), np.zeros(9)], axis=1).astype(np.float32)
    q = np.array([[0.3, 0.2]], np.float32)
    c64, c32, dist, degen, ratio = R.coefficients(line, q, R.nearest(line, q, 6), 2)
    assert degen.all() and ratio[0] <= 1e-14 and abs(c64.sum() - 1) < 1e-14 and (c64 > 0).all()


def test_no_point_of_the_weight_clouds_sits_near_the_degeneracy_threshold():
    """The precondition of the GPU weight test: with k > dim every point's ratio is >= 1e-3 (the flag 0) or <= 1e-14 (the flag 1) — nine
    orders of magnitude either side of the threshold 1e-12, far beyond what the device's square root and division can move; with
    k <= dim the flag is 1 by the count, whatever the ratio."""
    lowest = np.inf
    for dim, n, k in cases():
        pos, q = R.cloud(n, dim), R.queries(257, dim)
        idx = R.nearest(pos, q, k)
        for power in R.POWERS:
            degen, ratio = R.coefficients(pos, q, idx, power)[3:]
            if k <= dim:
                assert degen.all()
                continue
            assert (ratio[degen == 0] >= 1e-3).all() and (ratio[degen == 1] <= 1e-14).all(), (dim, n, k, power, ratio.min())
            lowest = min(lowest, ratio[degen == 0].min())
    print(f"MEASURED host: the smallest ratio of the weight clouds: {lowest:.3e}")


def test_zz_print_the_measured_ratios():
    """Not a check: the measured / allowed ratio of every bound above, for tests/SAMPLER_MEASURED.md (pytest -s)."""
    for k, v in sorted(RATIOS.items()):
        print(f"MEASURED {k}: {v:.3f}")
        assert v <= 1.0
