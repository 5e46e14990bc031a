"""g4c_tracer_advance_periodic (csrc/tracer.hip) through `ops.tracer_advance` on a periodic grid, `gfd.Tracers(period=)` and
`GNN.trace(period=)`: one launch equals, bit for bit, the composition wrap loop → periodic query → periodic weights → fp32 sum →
update → wrap loop (each pinned by its own tests); a particle under a uniform velocity crosses the seam again and again, stays
moving and ends at the position of the numpy.float32 loop; the paths of a rollout are those of a replay of `Tracers.advance`."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

import periodic_ref as P                                 # noqa: E402
from periodic_cases import CASES                         # noqa: E402
import graphs4cfd_amd as gfd                             # noqa: E402
from graphs4cfd_amd import _lib, ops, synthetic as S     # noqa: E402

DEV = torch.device("cuda", 0)
F32, I32, U8 = torch.float32, torch.int32, torch.uint8
STEP_CASES = [CASES[1], CASES[6], CASES[8]]          # both axes of two, one axis with a period above the extent, three of three


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def stage_ref(pos_d, frame, per, r, x, cfg, k, power):
    """The velocity at r by the pinned launches: periodic query, periodic weights, fp32 sum, scale and shift."""
    o, L = frame
    idx = S.knn_query_device(pos_d, r, k, period=per).t().to(I32).contiguous()
    coef, dist, _ = ops.sample_weights(pos_d, r, idx, power, origin=[float(v) for v in o], period=[float(v) for v in L])
    u = ops.sample_points(x[:, cfg["vcol"]].contiguous(), idx, coef)
    v = torch.mul(u, torch.tensor(cfg["scale"], dtype=F32, device=DEV))
    return torch.add(v, torch.tensor(cfg["shift"], dtype=F32, device=DEV)), dist


def step_ref(pos_d, frame, per, q, x0, x1, cfg, k, power, scheme):
    dt = torch.tensor(cfg["dt"], dtype=F32, device=DEV)
    v0, dist = stage_ref(pos_d, frame, per, q, x0, cfg, k, power)
    qn = torch.add(q, torch.mul(v0, dt))
    if scheme == _lib.TRACER_HEUN:
        v1, _ = stage_ref(pos_d, frame, per, qn, x1, cfg, k, power)
        qn = torch.add(q, torch.mul(torch.add(v0, v1), torch.mul(dt, 0.5)))
    return dev(P.wrap32(qn.cpu().numpy(), *frame)), v0, dist


@pytest.mark.parametrize("case", STEP_CASES, ids=[c["name"] for c in STEP_CASES])
@pytest.mark.parametrize("scheme", [_lib.TRACER_EULER, _lib.TRACER_HEUN])
def test_a_step_equals_the_composition(case, scheme):
    pos, k, per = case["pos"], case["k"], case["period"]
    n, dim = pos.shape
    pos_d, frame = dev(pos), P.frame(pos, per)
    grid = S._bin_cloud_periodic(pos_d, k, S.check_period(per, dim))
    assert [np.float32(v) for v in grid["periods"][:dim]] == list(frame[1]) and [np.float32(v) for v in grid["origin"][:dim]] == list(frame[0])
    gen = torch.Generator().manual_seed(n + scheme)
    w0, w1 = torch.randn(n, 9, generator=gen).to(DEV), torch.randn(n, 9, generator=gen).to(DEV)
    x0, x1 = w0[:, 2:7], w1[:, 3:8]
    cfg = dict(vcol=[2, 0, 3][:dim], scale=[1.5, -0.75, 0.5][:dim], shift=[0.25, -0.125, 0.0625][:dim], dt=0.1)
    q0 = dev(case["queries"])                                   # next to the seams, on cell faces, some three periods away
    p = int(q0.size(0))
    for power in (0, 2):
        q = q0.clone()
        status, stopped = torch.zeros(p, dtype=U8, device=DEV), torch.full((p,), -1, dtype=I32, device=DEV)
        release, vel = torch.zeros(p, dtype=I32, device=DEV), torch.zeros(p, dim, device=DEV)
        series = torch.full((1, p, dim), -7.0, device=DEV)
        want_q, want_v, _ = step_ref(pos_d, frame, per, q0, x0, x1, cfg, k, power, scheme)
        ops.tracer_advance(grid, x0, x1 if scheme == _lib.TRACER_HEUN else None, q, status, stopped, release, dt=cfg["dt"], k=k, power=power,
                           scheme=scheme, vcol=cfg["vcol"], scale=cfg["scale"], shift=cfg["shift"], t=0, max_steps=4, every=1, series=series, vel=vel)
        what = f"{case['name']} scheme {scheme} power {power}"
        assert torch.equal(q, want_q), what + ": q'"
        assert torch.equal(vel, want_v), what + ": vel"
        assert torch.equal(series[0], want_q), what + ": the slot holds the wrapped positions"
        assert bool((status == _lib.TRACER_MOVING).all()) and bool((stopped == -1).all()), what
        # the step is no trivial one: some particles went through a periodic face
        L = frame[1].astype(np.float64)
        inside0 = P.wrap32(q0.cpu().numpy(), *frame).astype(np.float64)
        assert ((np.abs(want_q.cpu().numpy() - inside0) > 0.5 * np.where(L > 0, L, np.inf)).any()), what + ": nobody crossed"


@pytest.mark.parametrize("limit", [None, 0.2])
@pytest.mark.parametrize("scheme", ["euler", "heun"])
def test_a_uniform_velocity_carries_particles_round_and_round(scheme, limit):
    case = CASES[1]
    pos, per = case["pos"], case["period"]
    n = pos.shape[0]
    frame = P.frame(pos, per)
    g = gfd.Graph(pos=dev(pos))
    U, dt, steps = (0.8125, -0.4375), 0.25, 24           # 4.9 periods along x, 5.25 along y: every particle crosses many times
    seeds = torch.from_numpy(case["queries"][:40])
    tr = gfd.Tracers(g, seeds, dt, scheme=scheme, k=12, shift=U, max_distance=limit, period=per)
    zero = torch.zeros(n, 3, device=DEV)                  # the field is 0: v = scale · 0 + shift = U exactly, at every stage
    want = seeds.numpy().copy()                           # (the seeds are taken as given; every later position is wrapped)
    crossings = 0
    for t in range(steps):
        tr.advance(zero, zero, t)
        step = (np.float32(dt) * np.array(U, np.float32)).astype(np.float32)
        if scheme == "heun":                              # q + (0.5 dt) (U + U), every operation in fp32
            step = (np.float32(np.float32(0.5) * np.float32(dt)) * (np.array(U, np.float32) + np.array(U, np.float32)).astype(np.float32)).astype(np.float32)
        moved = (want + step).astype(np.float32)
        new = P.wrap32(moved, *frame)
        crossings += int((new != moved).any(1).sum())
        want = new
        assert torch.equal(tr.positions.cpu(), torch.from_numpy(want)), (scheme, t)
        assert bool((tr.status == gfd.tracers.MOVING).all()), (scheme, t, tr.status.unique().tolist())
    assert crossings >= 4 * 40 and bool((tr.stopped == -1).all())
    lo, L = frame[0].astype(np.float64), frame[1].astype(np.float64)
    assert (want >= lo).all() and (want < lo + L).all()
    # without the period the same particles leave the cloud
    plain = gfd.Tracers(g, seeds, dt, scheme=scheme, k=12, shift=U, max_distance=0.2)
    for t in range(steps):
        plain.advance(zero, zero, t)
    assert bool((plain.status == gfd.tracers.FAR).all())


@pytest.fixture(scope="module")
def rollout():
    g = S.mus_graph(600, levels=1, seed=3).to(DEV)
    g.batch = torch.zeros(g.num_nodes, dtype=torch.long, device=DEV)
    torch.manual_seed(4)
    model = gfd.nn.NsOneScaleGNN(arch=S.mus_arch("NsOneScaleGNN", 64), device=DEV)
    model.eval()
    return g, model, model.solve(g.clone(), 5)


@pytest.mark.parametrize("capture", [True, False])
def test_trace_with_a_period_equals_a_replay_of_advance(rollout, capture):
    g, model, full = rollout
    n_out, nf = 5, 3
    lo, hi = g.pos.min(0).values.cpu(), g.pos.max(0).values.cpu()
    seeds = lo + (hi - lo) * torch.rand(64, 2, generator=torch.Generator().manual_seed(6))
    seeds[:16, 0] = lo[0] + 1e-3 * (hi[0] - lo[0])         # next to both periodic faces: either sign of u carries some across
    seeds[16:32, 0] = hi[0] - 1e-3 * (hi[0] - lo[0])
    per = ("auto", None)
    vmax = max(float(full.abs().max()), 1e-6)
    dt = 0.4 * float(hi[0] - lo[0]) / vmax                # a fastest particle covers 0.4 of the period a step: many cross the seam
    rt = model.trace(g.clone(), n_out, seeds, dt, every=1, capture=capture, period=per)
    ref = gfd.Tracers(g, seeds, dt, period=per)
    kept, x0 = [], g.field[:, -nf:].float()
    for s in range(n_out):
        x1 = full[:, nf * s:nf * (s + 1)]
        ref.advance(x0, x1, s)
        x0 = x1
        kept.append(ref.positions.clone())
    want = torch.cat(kept, dim=1)
    assert torch.equal(rt.paths, want) and torch.equal(rt.status, ref.status) and torch.equal(rt.positions, ref.positions)
    assert bool((rt.status == gfd.tracers.MOVING).all())
    L = float(P.frame(g.pos.cpu().numpy(), per)[1][0])
    x = torch.cat([seeds[:, :1].to(DEV), rt.paths[:, 0::2]], dim=1)
    assert bool(((x[:, 1:] - x[:, :-1]).abs() > 0.5 * L).any()), "no particle crossed the seam"
    assert bool((rt.paths[:, 0::2] >= float(lo[0])).all()) and bool((rt.paths[:, 0::2] < float(lo[0]) + L).all())
    plain = model.trace(g.clone(), n_out, seeds, dt, every=1, capture=capture)
    assert not torch.equal(plain.paths, rt.paths)


@pytest.mark.parametrize("scheme", ["euler", "heun"])
def test_a_position_that_does_not_wrap_stops_the_particle_before_any_stage(scheme):
    """Finite positions so large that the wrap overflows (period 0.5: above 1.7e38) — a seed taken as given, Heun's predictor, the new
    position — are positions that are not finite: status 4, stopped = t, q unchanged, no search from a made-up position."""
    case = CASES[1]
    pos, per = case["pos"], case["period"]                  # periods (1, 0.5)
    n = pos.shape[0]
    g = gfd.Graph(pos=dev(pos))
    seeds = torch.tensor([[0.3, 2e38], [0.3, -3e38], [0.4, 0.2], [3e38, 0.1]], dtype=F32)
    assert P.wraps_finite(seeds.numpy(), *P.frame(pos, per)).tolist() == [False, False, True, True]          # (3e38 / 1 does not overflow)
    zero = torch.zeros(n, 3, device=DEV)
    tr = gfd.Tracers(g, seeds, 1.0, scheme=scheme, k=12, period=per)
    tr.advance(zero, zero, 7)
    assert tr.status.tolist() == [4, 4, 1, 1] and tr.stopped.tolist() == [7, 7, -1, -1]
    assert torch.equal(tr.positions[:2].cpu(), seeds[:2]) and bool(torch.isfinite(tr.positions).all())
    # the update itself leaves the range: v = shift = (0, 2e38), dt = 1 — Heun's predictor and Euler's new position do not wrap
    tr = gfd.Tracers(g, seeds[2:3], 1.0, scheme=scheme, k=12, shift=(0.0, 2e38), period=per)
    tr.advance(zero, zero, 3)
    assert tr.status.tolist() == [4] and tr.stopped.tolist() == [3] and torch.equal(tr.positions.cpu(), seeds[2:3])
