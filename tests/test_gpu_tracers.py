"""g4c_tracer_advance (csrc/tracer.hip) through ops.tracer_advance against the composition of the launches that are already pinned:
for the same positions and node tensors, `knn_query_device` (the search), `ops.sample_weights` (the fit), `ops.sample_points` on the
velocity columns (the sum) and the advance as separate torch fp32 multiplies and adds — twice for a Heun step.  The new positions, the
velocity, the status and the stopping step must be EQUAL.  Clouds and particles are uniformly random, so no two candidate distances
tie and the neighbour order is unambiguous.  Every output lives in a guard arena (tests/footprint.py), every input is frozen.

One Euler step is also compared with the fp64 form of tests/tracer_ref.py (from the device's own neighbour table) within
  dt |scale_a| [(k + 3) 2^-24 Σ_j |c_j x_j| + 2^-23 max_j |c_j| Σ_j |x_j|] + 2^-23 (|q_a| + dt |v_a|):
the fp32 sum; the one-ulp freedom of the fp64 library sqrt and division in the coefficients (the sampler's own bound); the two
roundings of the advance.  tests/TRACERS_MEASURED.md records measured / allowed."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

import sampler_ref as R                                        # noqa: E402
import tracer_ref as T                                         # noqa: E402
from footprint import PATTERN, assert_footprint, flat_arena, frozen     # noqa: E402
from graphs4cfd_amd import _lib, ops, synthetic as S           # noqa: E402

DEV = torch.device("cuda", 0)
F32, F64, I32, U8 = torch.float32, torch.float64, torch.int32, torch.uint8
INF = float("inf")
MAX_STEPS, EVERY, T_STEP = 7, 3, 2          # step 2 fills slot 0 of the two slots
RATIOS = {}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def config(dim, limits):
    """Velocity columns (2, 0[, 3]) of a window of 5 columns, a scale and a shift that are no 1 and 0, and — with `limits` — a box that
    some particles leave and a largest distance that the far particle exceeds."""
    return dict(vcol=[2, 0, 3][:dim], scale=[1.5, -0.75, 0.5][:dim], shift=[0.25, -0.125, 0.0625][:dim], dt=0.01,
                box_lo=[-0.05] * dim if limits else None, box_hi=[1.05] * dim if limits else None, max_distance=0.5 if limits else INF)


def particles(pos, p, dim, h):
    """The first p of the fixed random set in [-0.1, 1.1]^dim; from nine particles on, seven sit exactly on nodes and one lies 50 cell
    sizes off the cloud, where the ring search grows to the whole grid."""
    q = R.queries(p, dim).copy()
    if p >= 9:
        q[1:8] = pos[[0, 3, 5, 8, 11, 13, 16]]
        q[8] = pos.min(0)
        q[8, 0] -= np.float32(50.0 * h)
    return q


def fields(n, seed):
    """x0 and x1: windows of 5 columns of tensors of 9 (a leading dimension above the width)."""
    g = torch.Generator().manual_seed(seed)
    w0, w1 = torch.randn(n, 9, generator=g).to(DEV), torch.randn(n, 9, generator=g).to(DEV)
    return w0, w1, w0[:, 2:7], w1[:, 3:8]


def stage_ref(pos_d, r, x, cfg, k, power):
    nearest = S.knn_query_device(pos_d, r, k)
    idx = nearest.t().to(I32).contiguous()
    coef, dist, _ = ops.sample_weights(pos_d, r, idx, power)
    u = ops.sample_points(x[:, cfg["vcol"]].contiguous(), idx, coef)
    v = torch.mul(u, torch.tensor(cfg["scale"], dtype=F32, device=DEV))
    return torch.add(v, torch.tensor(cfg["shift"], dtype=F32, device=DEV)), dist


def step_ref(pos_d, q, status, stopped, release, x0, x1, t, cfg, k, power, scheme):
    """(q', status', stopped', vel, the rows whose vel is written) by the composition; every particle's position must be finite."""
    p, dim = int(q.size(0)), int(q.size(1))
    if p == 0 or not 0 <= t < MAX_STEPS:
        return q.clone(), status.clone(), stopped.clone(), torch.zeros_like(q), torch.zeros(p, dtype=torch.bool, device=DEV)
    dt = torch.tensor(cfg["dt"], dtype=F32, device=DEV)
    act = (release <= t) & (status < 2)
    v0, dist = stage_ref(pos_d, q, x0, cfg, k, power)
    far = act & (dist > cfg["max_distance"])
    go = act & ~far
    qn = torch.add(q, torch.mul(v0, dt))
    if scheme == _lib.TRACER_HEUN:
        assert bool(torch.isfinite(qn).all())
        v1, _ = stage_ref(pos_d, qn, x1, cfg, k, power)
        s = torch.add(v0, v1)
        qn = torch.add(q, torch.mul(s, torch.mul(dt, 0.5)))
    lo = torch.tensor(cfg["box_lo"] or [-INF] * dim, dtype=F32, device=DEV)
    hi = torch.tensor(cfg["box_hi"] or [INF] * dim, dtype=F32, device=DEV)
    left = go & ~((qn >= lo) & (qn <= hi)).all(1)
    st = torch.where(act, torch.ones_like(status), status)
    st = torch.where(far, torch.full_like(status, 3), st)
    st = torch.where(left, torch.full_like(status, 2), st)
    return (torch.where(go[:, None], qn, q), st, torch.where(far | left, torch.full_like(stopped, t), stopped), v0, go)


class Launch:
    """One guarded launch: every output in an arena of its own, filled from the initial state."""

    def __init__(self, grid, q, status, stopped, release, slots=MAX_STEPS // EVERY):
        self.grid, self.p, self.dim, self.release = grid, int(q.size(0)), int(q.size(1)), release
        n = max(self.p * self.dim, 1)
        self.q, self.q_all = flat_arena(n, F32, device=DEV)
        self.vel, self.vel_all = flat_arena(n, F32, device=DEV)
        self.stopped, self.stopped_all = flat_arena(max(self.p, 1), I32, device=DEV)
        self.series, self.series_all = flat_arena(max(slots * self.p * self.dim, 1), F32, device=DEV)
        # status is uint8 and the arenas' patterns start at two bytes: its bytes are those of an int32 arena, four to a word
        self.words = -(-self.p // 4)
        self.status_words, self.status_all = flat_arena(max(self.words, 1), I32, device=DEV)
        self.status_bytes = self.status_words.view(U8)
        self.slots = slots
        self.q[:self.p * self.dim].copy_(q.reshape(-1))
        self.stopped[:self.p].copy_(stopped)
        self.status_bytes[:self.p].copy_(status)

    def views(self):
        p, d = self.p, self.dim
        return (self.q[:p * d].view(p, d), self.status_bytes[:p], self.stopped[:p], self.vel[:p * d].view(p, d),
                self.series[:self.slots * p * d].view(self.slots, p, d))

    def run(self, x0, x1, cfg, k, power, scheme, t, device_step, frozen_too=()):
        q, status, stopped, vel, series = self.views()
        step = torch.tensor([t, 12345], dtype=I32, device=DEV) if device_step else None
        g = self.grid
        with frozen(g["pos_sorted"], g["order"], g["cell_start"], self.release, step, *frozen_too, what="tracer_advance"):
            ops.tracer_advance(g, x0, x1 if scheme == _lib.TRACER_HEUN else None, q, status, stopped, self.release, dt=cfg["dt"], k=k,
                               power=power, scheme=scheme, vcol=cfg["vcol"], scale=cfg["scale"], shift=cfg["shift"], box_lo=cfg["box_lo"],
                               box_hi=cfg["box_hi"], max_distance=cfg["max_distance"], step=step, t=0 if device_step else t,
                               max_steps=MAX_STEPS, every=EVERY, series=series, vel=vel)
            torch.cuda.synchronize(DEV)
        return q, status, stopped, vel, series

    def check_footprint(self, vel_rows, slot, what):
        p, d = self.p, self.dim
        assert_footprint(self.q_all, self.q[:p * d], what=what + ": q", inside=p > 0)
        assert_footprint(self.stopped_all, self.stopped[:p], what=what + ": stopped", inside=p > 0)
        assert_footprint(self.status_all, self.status_words[:self.words], what=what + ": status", inside=p > 0)
        tail = torch.arange(p, 4 * self.words, device=DEV)          # the bytes of the last word behind the last particle keep the pattern's
        assert torch.equal(self.status_bytes[p:4 * self.words], ((torch.full_like(tail, PATTERN[4][1]) >> (8 * (tail % 4))) & 0xFF).to(U8)), what + ": status"
        mask = torch.zeros((1, max(p * d, 1)), dtype=torch.bool)
        mask[0, :p * d] = vel_rows.cpu()[:, None].expand(p, d).reshape(-1)
        assert_footprint(self.vel_all, self.vel, mask, what=what + ": vel")
        mask = torch.zeros((1, max(self.slots * p * d, 1)), dtype=torch.bool)
        if slot is not None:
            mask[0, slot * p * d:(slot + 1) * p * d] = True
        assert_footprint(self.series_all, self.series, mask, what=what + ": series")


def initial(q_np):
    p = q_np.shape[0]
    rows = torch.arange(p)
    status = torch.where(rows % 11 == 5, 2, 0).to(U8).to(DEV)                 # some are frozen already
    stopped = torch.where(rows % 11 == 5, 0, -1).to(I32).to(DEV)
    release = torch.where(rows % 7 == 3, 5, 0).to(I32).to(DEV)                # some are released after T_STEP
    return dev(q_np), status, stopped, release


def equal_to_the_composition(pos, k, power, scheme, p, limits, seed, what):
    n, dim = pos.shape
    pos_d = dev(pos)
    grid = S._bin_cloud(pos_d, k)
    cfg = config(dim, limits)
    w0, w1, x0, x1 = fields(n, seed)
    q, status, stopped, release = initial(particles(pos, p, dim, grid["h"]))
    want_q, want_st, want_sp, want_v, go = step_ref(pos_d, q, status, stopped, release, x0, x1, T_STEP, cfg, k, power, scheme)
    runs = []
    for device_step in (True, False):
        la = Launch(grid, q, status, stopped, release)
        got = la.run(x0, x1, cfg, k, power, scheme, T_STEP, device_step, frozen_too=(w0, w1))
        la.check_footprint(go, 0, what)
        assert torch.equal(got[0], want_q), what + ": q'"
        assert torch.equal(got[1], want_st) and torch.equal(got[2], want_sp), what + ": status, stopped"
        assert torch.equal(got[3][go], want_v[go]), what + ": vel"
        assert torch.equal(got[4][0], want_q), what + ": the slot holds every particle's position"
        runs.append(got)
    for a, b in zip(*runs):                                      # two runs, the same bits — the step index on the device or by value
        assert torch.equal(a.view(torch.int32) if a.dtype == F32 else a, b.view(torch.int32) if b.dtype == F32 else b), what + ": two runs"
    return want_st


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("n", [17, 65, 1000])
def test_a_launch_equals_the_composition_of_the_pinned_launches(n, dim):
    pos = R.cloud(n, dim)
    seen = set()
    for k in (1, dim, 6, 10, 16):
        for power in R.POWERS:
            for scheme in (_lib.TRACER_EULER, _lib.TRACER_HEUN):
                for p in (0, 1, 63, 64, 65, 257):
                    what = f"n {n} dim {dim} k {k} power {power} scheme {scheme} P {p}"
                    st = equal_to_the_composition(pos, k, power, scheme, p, limits=p % 2 == 1, seed=n + 10 * k + p, what=what)
                    seen |= set(st.tolist())
    assert seen == {0, 1, 2, 3}, seen          # waiting, moving, left the box, too far: every branch was compared


def test_more_particles_than_one_pass_of_the_grid():
    pos, p = R.cloud(1000, 2), 262_444                              # 1024 workgroups of 256 hold 262 144
    pos_d = dev(pos)
    grid = S._bin_cloud(pos_d, 6)
    cfg = config(2, True)
    w0, w1, x0, x1 = fields(1000, 9)
    q_np = (np.random.default_rng(11).random((p, 2)) * 1.2 - 0.1).astype(np.float32)
    q, status, stopped, release = initial(q_np)
    want_q, want_st, want_sp, want_v, go = step_ref(pos_d, q, status, stopped, release, x0, x1, T_STEP, cfg, 6, 2, _lib.TRACER_HEUN)
    la = Launch(grid, q, status, stopped, release)
    got = la.run(x0, x1, cfg, 6, 2, _lib.TRACER_HEUN, T_STEP, True)
    la.check_footprint(go, 0, "262 444 particles")
    assert torch.equal(got[0], want_q) and torch.equal(got[1], want_st) and torch.equal(got[2], want_sp)
    assert torch.equal(got[3][go], want_v[go]) and torch.equal(got[4][0], want_q)
    assert int(go[262_144:].sum()) > 100 and not torch.equal(got[0][262_144:], q[262_144:])


@pytest.mark.parametrize("dim", [2, 3])
def test_steps_off_the_slots_out_of_range_and_before_the_release_write_what_they_own(dim):
    pos = R.cloud(65, dim)
    pos_d = dev(pos)
    k = 6
    grid = S._bin_cloud(pos_d, k)
    cfg = config(dim, True)
    w0, w1, x0, x1 = fields(65, 5)
    q, status, stopped, release = initial(particles(pos, 65, dim, grid["h"]))
    none = torch.zeros(65, dtype=torch.bool, device=DEV)
    for scheme in (_lib.TRACER_EULER, _lib.TRACER_HEUN):
        # an off-slot step moves the particles and writes no slot; step 5 fills slot 1 and moves the late releases too
        for t, slot in ((1, None), (3, None), (5, 1)):
            want = step_ref(pos_d, q, status, stopped, release, x0, x1, t, cfg, k, 2, scheme)
            la = Launch(grid, q, status, stopped, release)
            got = la.run(x0, x1, cfg, k, 2, scheme, t, t % 2 == 1)
            la.check_footprint(want[4], slot, f"step {t}")
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2]), t
            assert (t < 5) == bool(((got[1] == 0) & (release == 5)).any())
            if slot is not None:
                assert torch.equal(got[4][slot], want[0])
        # a step index out of range writes nothing at all, on the device or by value
        for t, device_step in ((MAX_STEPS, True), (MAX_STEPS, False), (-1, True), (-1, False), (2 ** 31 - 1, True)):
            la = Launch(grid, q, status, stopped, release)
            got = la.run(x0, x1, cfg, k, 2, scheme, t, device_step)
            la.check_footprint(none, None, f"step {t}")
            assert torch.equal(got[0], q) and torch.equal(got[1], status) and torch.equal(got[2], stopped)
    # nobody released, nobody moving: the slot step still writes every position, and nothing else
    late = torch.full_like(release, 6)
    la = Launch(grid, q, status, stopped, late)
    got = la.run(x0, x1, cfg, k, 2, _lib.TRACER_HEUN, T_STEP, True)
    la.check_footprint(none, 0, "unreleased")
    assert torch.equal(got[0], q) and torch.equal(got[1], status) and torch.equal(got[2], stopped) and torch.equal(got[4][0], q)


def test_positions_that_are_not_finite_stop_before_any_search():
    pos = R.cloud(65, 2)
    pos_d = dev(pos)
    grid = S._bin_cloud(pos_d, 6)
    cfg = config(2, False)
    w0, w1, x0, x1 = fields(65, 6)
    q_np = R.queries(65, 2).copy()
    q_np[3], q_np[10], q_np[20], q_np[33] = (np.nan, 0.5), (0.5, np.inf), (-np.inf, np.nan), (3e38, -3e38)          # the last is finite, and wild
    p = 65
    q, release = dev(q_np), torch.zeros(p, dtype=I32, device=DEV)
    status, stopped = torch.zeros(p, dtype=U8, device=DEV), torch.full((p,), -1, dtype=I32, device=DEV)
    for scheme in (_lib.TRACER_EULER, _lib.TRACER_HEUN):
        la = Launch(grid, q, status, stopped, release)
        got_q, got_st, got_sp, got_v, _ = la.run(x0, x1, cfg, 6, 2, scheme, T_STEP, True)
        bad = [3, 10, 20]
        assert got_st[bad].tolist() == [4, 4, 4] and got_sp[bad].tolist() == [T_STEP] * 3
        assert torch.equal(got_q[bad].view(torch.int32), q[bad].view(torch.int32))          # left as they were, bit for bit
        # the wild particle is finite: it is searched (every node is as far, the fit falls back to Shepard's weights) and moved, by a
        # dt v far below half an ulp of 3e38 — status 1 under both schemes (Heun's q* is as finite), the position bit for bit what it was
        assert int(got_st[33]) == 1 and int(got_sp[33]) == -1 and torch.equal(got_q[33], q[33]) and bool(torch.isfinite(got_v[33]).all())
        rest = torch.ones(p, dtype=torch.bool, device=DEV)
        rest[bad + [33]] = False
        assert bool((got_st[rest] == 1).all()) and bool((got_sp[rest] == -1).all()) and bool(torch.isfinite(got_q[rest]).all())
        ref = T.advance(pos, q_np, np.zeros(p, np.uint8), np.full(p, -1, np.int32), np.zeros(p, np.int32), x0.cpu().numpy(),
                        x1.cpu().numpy(), T_STEP, T.params(2, cfg["dt"], 6, 2, scheme, cfg["vcol"], cfg["scale"], cfg["shift"], max_steps=MAX_STEPS))
        R.same(got_st, ref[1], "status against the restatement")
        R.same(got_sp, ref[2], "stopped against the restatement")
    # a velocity that throws Heun's predictor out of the finite range freezes the particle where it was
    big = torch.full((65, 5), 3e38, dtype=F32, device=DEV)
    la = Launch(grid, dev(R.queries(65, 2)), status, stopped, release)
    got_q, got_st, got_sp, got_v, _ = la.run(big, big, dict(cfg, dt=10.0, scale=[1.0, 1.0], shift=[0.0, 0.0]), 6, 2, _lib.TRACER_HEUN, T_STEP, False)
    assert bool((got_st == 4).all()) and bool((got_sp == T_STEP).all()) and torch.equal(got_q, dev(R.queries(65, 2)))


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("n", R.WEIGHT_CLOUDS)
def test_an_euler_step_is_within_its_bound_of_the_fp64_form(n, dim):
    """Measured / allowed at the sizes below: tests/TRACERS_MEASURED.md."""
    pos, q = R.cloud(n, dim), R.queries(257, dim)
    pos_d, q_d = dev(pos), dev(q)
    w0, w1, x0, x1 = fields(n, 7)
    cfg = config(dim, False)
    dt, scale, shift = float(np.float32(cfg["dt"])), np.asarray(cfg["scale"], np.float64), np.asarray(cfg["shift"], np.float64)
    xv = x0.cpu().numpy()[:, cfg["vcol"]].astype(np.float64)
    p = 257
    release = torch.zeros(p, dtype=I32, device=DEV)
    status, stopped = torch.zeros(p, dtype=U8, device=DEV), torch.full((p,), -1, dtype=I32, device=DEV)
    worst = 0.0
    for k in R.WEIGHT_K[dim]:
        idx = S.knn_query_device(pos_d, q_d, k).cpu().numpy().astype(np.int32)
        grid = S._bin_cloud(pos_d, k)
        for power in R.POWERS:
            what = f"n {n} dim {dim} k {k} power {power}"
            la = Launch(grid, q_d, status, stopped, release)
            got_q, got_st, _, got_v, _ = la.run(x0, None, cfg, k, power, _lib.TRACER_EULER, T_STEP, True)
            assert bool((got_st == 1).all()), what
            c64 = R.coefficients(pos, q, idx, power)[0]
            val, mag = R.apply64(xv, idx, c64)
            v = scale * val + shift
            want = q.astype(np.float64) + dt * v
            sum_x = np.abs(xv)[idx].sum(1)                                                 # [P, dim]: Σ_j |x_j|
            allowed = (dt * np.abs(scale) * (R.bound32(mag, k) + 2.0 ** -23 * np.abs(c64).max(1, keepdims=True) * sum_x)
                       + 2.0 ** -23 * (np.abs(q.astype(np.float64)) + dt * np.abs(v)))
            ratio = R.within(got_q, want, allowed, what)
            print(f"{what}: measured / allowed {ratio:.3f}")
            worst = max(worst, ratio)
            # and bit for bit the restatement's fp32 loop over the device's coefficients' neighbours
            ref = T.advance(pos, q, np.zeros(p, np.uint8), np.full(p, -1, np.int32), np.zeros(p, np.int32), x0.cpu().numpy(), None, T_STEP,
                            T.params(dim, cfg["dt"], k, power, T.EULER, cfg["vcol"], cfg["scale"], cfg["shift"], max_steps=MAX_STEPS), idx0=idx)
            R.within(got_q, ref[0], allowed, what + ", against the fp32 restatement")
    RATIOS[(n, dim)] = worst
    print(f"n {n} dim {dim}: the largest measured / allowed {worst:.3f}")
    # negative control: a position off by a part in 2^19 of a step is outside
    assert R.rejects(R.within, got_q.cpu().numpy() + np.float32(2.0 ** -19) * np.abs(got_q.cpu().numpy()) + np.float32(1e-6), want, allowed)


def test_the_entry_point_refuses_what_the_wrapper_cannot_see():
    pos_d = dev(R.cloud(65, 2))
    grid = S._bin_cloud(pos_d, 6)
    w0, w1, x0, x1 = fields(65, 1)
    q = dev(R.queries(5, 2))
    args = dict(q=q, status=torch.zeros(5, dtype=U8, device=DEV), stopped=torch.zeros(5, dtype=I32, device=DEV),
                release=torch.zeros(5, dtype=I32, device=DEV), dt=0.01, k=6)
    for patch in (dict(h=0.0), dict(n_cells=[0, 1, 1]), dict(n_cells=[2, 2, 2]), dict(h=math.nan)):
        with pytest.raises(ValueError, match="tracer_advance"):
            ops.tracer_advance(dict(grid, **patch), x0, x1, **args)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.tracer_advance(grid, x0, x1, **dict(args, q=q.cpu()))
    with pytest.raises(ValueError, match="x1"):
        ops.tracer_advance(grid, x0, x1.cpu(), **args)
    # no particles: nothing is launched, whatever the grid
    empty = dict(q=q[:0], status=args["status"][:0], stopped=args["stopped"][:0], release=args["release"][:0], dt=0.01, k=6)
    assert ops.tracer_advance(grid, x0, x1, **empty).numel() == 0
