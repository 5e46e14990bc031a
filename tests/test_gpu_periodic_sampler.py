"""`gfd.PointSampler(period=)` and `SampleLoss(period=)` (g4c_sample_weights_periodic, csrc/point_sample.hip) against the fp64
restatement of tests/sampler_ref.py fed the wrapped offsets, on the dyadic clouds of tests/periodic_cases.py: there a wrapped offset
is exact in fp32, so the restatement takes the offsets as a cloud of their own seen from the origin.  The allowances are those of
tests/test_gpu_point_sampler.py: 2^-23 max_j |c_ref,j| per point for the coefficients, one ulp for the distance, the flags exact."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

import periodic_ref as P                       # noqa: E402
import sampler_ref as R                        # noqa: E402
from periodic_cases import CASES, IDS          # noqa: E402
import graphs4cfd_amd as gfd                   # noqa: E402
from graphs4cfd_amd import synthetic as S      # noqa: E402

DEV = torch.device("cuda", 0)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def restated(pos, q, idx, period, power):
    """sampler_ref.coefficients on the wrapped offsets of the table `idx` [P, k]: the offsets (exact fp32 on a dyadic cloud) are the
    cloud, the origin is the one query."""
    o, L = P.frame(pos, period)
    d = P.stencil_offsets(pos, P.wrap32(q, o, L), idx, L)
    m, k, dim = d.shape
    d32 = d.astype(np.float32)
    assert (d32.astype(np.float64) == d).all()
    return R.coefficients(d32.reshape(m * k, dim), np.zeros((m, dim), np.float32), np.arange(m * k).reshape(m, k), power)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_tables_match_the_restatement_on_wrapped_offsets(case):
    pos, k, per, q = case["pos"], case["k"], case["period"], case["queries"]
    g = gfd.Graph(pos=dev(pos))
    for power in R.POWERS:
        s = gfd.PointSampler(g, torch.from_numpy(q), k=k, power=power, period=per)
        idx = s.idx.cpu().numpy()
        assert torch.equal(s.idx.long(), S.knn_query_device(dev(pos), dev(q), k, period=per))
        c64, c32, dist, degen, ratio = restated(pos, q, idx, per, power)
        R.within(s.coef, c64, R.coefficient_bound(c64), f"{case['name']} power {power}: coef")
        assert R.ulps32(s.distance, dist) <= 1
        R.same(s.degenerate.to(torch.uint8), degen, "degenerate")
        D = P.distances(pos, per, q)
        assert R.ulps32(s.distance, D.min(1).values.numpy().astype(np.float32)) <= 1          # the wrapped distance
        if case["far"]:
            n = case["far"]
            assert torch.equal(s.coef[-n:], s.coef[:n]) and torch.equal(s.idx[-n:], s.idx[:n])


def test_a_field_linear_in_the_wrapped_offset_is_reproduced_next_to_the_seam():
    case = CASES[0]
    pos, k, per = case["pos"], case["k"], case["period"]
    o, L = P.frame(pos, per)
    q = case["queries"][:96]
    s = gfd.PointSampler(gfd.Graph(pos=dev(pos)), dev(q), k=k, period=per)
    idx, coef = s.idx.cpu().numpy(), s.coef.cpu().numpy().astype(np.float64)
    d = P.stencil_offsets(pos, P.wrap32(q, o, L), idx, L)
    assert P.crosses(pos, P.wrap32(q, o, L), idx, L).mean() > 0.3
    c64, _, _, degen, ratio = restated(pos, q, idx, per, 2)
    assert not degen.any()
    slope, const = np.array([0.75, -1.25]), 2.0
    value = (coef * (d @ slope + const)).sum(1)          # Σ_j c_j f(d_j), f linear in the wrapped offset: f(0) at the point
    mag = np.abs(coef * (d @ slope + const)).sum(1)
    # the coefficients' rounding to fp32 (2^-23 max|c| per neighbour, the sampler tests' allowance) and the restatement's fp64 identity error
    allowed = 2.0 ** -23 * np.abs(c64).max(1) * np.abs(d @ slope + const).sum(1) + 256 * k * 2.0 ** -53 * mag / ratio
    R.within(value, np.full(96, const), allowed, "linear in the wrapped offset")
    # the plain offsets do not reproduce it: the check sees the seam
    plain = pos.astype(np.float64)[idx] - P.wrap32(q, o, L).astype(np.float64)[:, None, :]
    assert R.rejects(R.within, (coef * (plain @ slope + const)).sum(1), np.full(96, const), allowed)


@pytest.mark.parametrize("shift", [(0.25, 0.0), (0.40625, 0.15625)])
def test_seam_invariance_under_a_cyclic_dyadic_shift(shift):
    """Nodes and points shifted cyclically by a dyadic amount (periods 1 and 0.5, powers of two): the same table — idx as node labels,
    coef, distance — bit for bit.  (The cloud's minimum, the origin of the wrap and of the grid, moves with the shift: the table does
    not depend on it, since every wrapped offset is an exact dyadic number whatever the frame.)"""
    per, k = (1.0, 0.5), 12
    pos_a = CASES[1]["pos"]          # (tie-free with these queries, and a shift keeps every distance)
    q = CASES[1]["queries"]
    sh = np.array(shift)

    def shifted(x):
        y = x.astype(np.float64) + sh
        return (y - np.floor(y / np.array(per)) * np.array(per)).astype(np.float32)
    pos_b = shifted(pos_a)
    a = gfd.PointSampler(gfd.Graph(pos=dev(pos_a)), dev(q), k=k, period=per)
    b = gfd.PointSampler(gfd.Graph(pos=dev(pos_b)), dev(shifted(q)), k=k, period=per)
    assert (pos_b != pos_a).any() and (pos_b[:, 0] < pos_a[:, 0]).any()          # some nodes went round the seam
    assert P.crosses(pos_a, P.wrap32(q, *P.frame(pos_a, per)), a.idx.cpu().numpy(), np.array(per, np.float32)).any()
    assert torch.equal(a.idx, b.idx) and torch.equal(a.coef, b.coef) and torch.equal(a.distance, b.distance)
    assert torch.equal(a.degenerate, b.degenerate)


def test_period_none_is_todays_sampler():
    pos, q = CASES[1]["pos"], CASES[1]["queries"]
    g = gfd.Graph(pos=dev(pos))
    a, b = gfd.PointSampler(g, dev(q), k=6), gfd.PointSampler(g, dev(q), k=6, period=(None, None))
    assert a.period is None and b.period is None
    assert torch.equal(a.idx, b.idx) and torch.equal(a.coef, b.coef) and torch.equal(a.distance, b.distance)
    line = gfd.PointSampler.line(g, (0.0, 0.0), (1.0, 0.5), 9, period=(1.0, 0.5))
    grid = gfd.PointSampler.grid(g, (4, 3), period=(1.0, "auto"))
    assert line.period is not None and grid.period is not None and grid.shape == (4, 3)


def test_sample_loss_backward_is_the_adjoint_of_the_periodic_tables():
    case = CASES[1]
    pos, per, q = case["pos"], case["period"], case["queries"]
    g = gfd.Graph(pos=dev(pos))
    from graphs4cfd_amd.nn.losses import SampleLoss
    loss = SampleLoss(torch.from_numpy(q), weight=1.0, node_weight=0.0, k=12, period=per)
    gen = torch.Generator().manual_seed(0)
    pred = torch.randn(pos.shape[0], 3, generator=gen).to(DEV).requires_grad_(True)
    target = torch.randn(pos.shape[0], 3, generator=gen).to(DEV)
    value = loss(g, pred, target)
    value.backward()
    s = gfd.PointSampler(g, torch.from_numpy(q), k=12, period=per)
    kept = loss.sampler(g)[0]
    assert torch.equal(kept.idx, s.idx) and torch.equal(kept.coef, s.coef)
    with torch.no_grad():
        diff = s.sample(pred.detach()) - s.sample(target)
        gy = (2.0 / diff.numel()) * diff
        want = s.adjoint(gy)
        assert torch.allclose(value, (diff ** 2).mean(), rtol=1e-6)
        # the backward is adjoint(gy') with gy' = 2 diff / count as autograd forms it in fp32: at most three roundings (2^-24 each)
        # away from gy per entry.  Both sides are fp32 sums over a node's list of m <= M entries, each within (m + 3) 2^-24 Σ|c||gy| of
        # its exact sum (the apply's bound, tests/sampler_ref.py), and the exact sums differ by 3 · 2^-24 Σ|c||gy|.
        mag = gfd.PointSampler.from_tables(s._idx, s._coef.abs(), pos.shape[0]).adjoint(gy.abs())
        M = int(s._node_side()[0].diff().max())
    assert bool(((pred.grad - want).abs() <= (2 * (M + 3) + 3) * 2.0 ** -24 * mag).all()), float((pred.grad - want).abs().max())
    assert float(want.abs().max()) > 0
    plain = gfd.PointSampler(g, torch.from_numpy(q), k=12)
    assert not torch.equal(plain.idx, s.idx)


def test_points_that_are_not_finite_form_no_address():
    """Along a periodic axis a point that does not wrap is fitted from the origin; along another axis a point that is not finite has
    no neighbours: its row names node 0 (never −1) and its coefficients are NaN."""
    pos = CASES[2]["pos"]                                   # axis 0 periodic, axis 1 not
    g = gfd.Graph(pos=dev(pos))
    wild = np.array([[np.inf, 0.2], [np.nan, 0.2], [float(pos[:, 0].min()), 0.2], [0.3, np.nan], [0.3, np.inf], [0.3, 1e30]], np.float32)
    s = gfd.PointSampler(g, dev(wild), k=12, period=(1.0, None))
    assert int(s.idx.min()) >= 0 and int(s.idx.max()) < pos.shape[0]
    assert torch.equal(s.idx[0], s.idx[2]) and torch.equal(s.idx[1], s.idx[2]) and torch.equal(s.coef[:2], s.coef[2:3].expand(2, 12))
    assert bool(torch.isfinite(s.coef[:3]).all()) and bool(torch.isnan(s.coef[3:5]).all()) and bool((s.idx[3:5] == 0).all())
    x = torch.ones(pos.shape[0], 2, device=DEV)
    out = s.sample(x)
    assert bool(torch.isnan(out[3:5]).all()) and bool(torch.isfinite(out[:3]).all())
