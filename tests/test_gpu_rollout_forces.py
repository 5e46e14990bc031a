"""`Rollout(forces=, force_*=, wall_moments=, target_forces=)`, `GNN.forces` and `GNN.evaluate(forces=)` against a replay of
`gfd.BodyForces` (which tests/test_gpu_body_forces.py pins to the restatement) over what the same rollout returns: the per-step sums
bit for bit `BodyForces.forces` of every step of `result()` — with and without capture, with and without the Morton renumbering (the
gradient's tables are re-indexed, every node keeps its in-edges in the caller's order) —, the time statistics and Fourier modes bit
for bit tests/moments_ref.py and tests/spectrum_ref.py run over the per-step `cur` / `wall` of the replay."""
import math
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

import forces_ref as R                                   # noqa: E402
import moments_ref as M                                  # noqa: E402
import spectrum_ref as SP                                # noqa: E402
import graphs4cfd_amd as gfd                             # noqa: E402
from graphs4cfd_amd import ops, synthetic as S           # noqa: E402
from graphs4cfd_amd.nn.model import Rollout              # noqa: E402

DEV = torch.device("cuda", 0)
N_OUT, NF = 6, 3
SCALE, SHIFT, MU = [2.0, 0.5, 1.25], [0.5, 0.0, -0.25], 0.0125
WALLS = (((0.35, 0.5), 0.15, 64), ((0.75, 0.5), 0.1, 40))          # (centre, radius, wall nodes) of the two bodies


@pytest.fixture(scope="module")
def mesh():
    g = S.mus_graph(1500, levels=2, seed=11).to(DEV)
    g.batch = torch.zeros(g.num_nodes, dtype=torch.long, device=DEV)
    pos = g.pos.cpu().double()
    bound = torch.zeros(g.num_nodes, dtype=torch.long, device=DEV)          # (kept off the shared graph: a Graph with attributes the
    labels = torch.zeros(g.num_nodes, dtype=torch.long)
    for b, ((cx, cy), r, m) in enumerate(WALLS):                  # the m nodes nearest to each circle: a ring, star-shaped about its mean
        ring = torch.argsort(((pos[:, 0] - cx).hypot(pos[:, 1] - cy) - r).abs())[:m]
        bound[ring.to(DEV)] = 4                                   #  Morton renumbering does not know runs as it is numbered)
        labels[ring] = 10 * (b + 1)
    nodes = torch.nonzero(bound == 4).flatten()
    assert int(nodes.numel()) == 104
    torch.manual_seed(12)
    model = gfd.nn.NsTwoScaleGNN(arch=S.mus_arch("NsTwoScaleGNN", 128), device=DEV)
    model.eval()
    full = model.solve(g.clone(), N_OUT)
    op = gfd.BodyForces(g, nodes, labels[nodes.cpu()], mu=MU, scale=SCALE, shift=SHIFT)
    assert op.n_bodies == 2 and op.body_offsets.tolist() == [0, 64, 104]
    return dict(g=g, model=model, full=full, op=op, labels=labels[nodes.cpu()], nodes=nodes, bound=bound, runs={})


def steps_of(cols, nf=NF):
    return [cols[:, nf * t:nf * (t + 1)] for t in range(int(cols.size(1)) // nf)]


def replay(op, cols):
    """Per step of the columns: (sums [B, 6] fp64, cur [B, 3] fp32, wall [W, 2] fp32) by the operator's own launch."""
    out = []
    for x in steps_of(cols):
        sums = op.forces(x).cpu().numpy()
        out.append((sums, R.cur32(sums), op.wall(x).cpu().numpy()))
    return out


def moments_equal_over(mo, samples, steps, start, stride, what, first=0):
    st = M.run(samples, steps, start, stride, None, first=first)
    assert mo.count == M.count(st, stride) > 0 and mo.origin == int(st["window"][0]) and mo.stride == stride, (what, mo)
    for k, got in zip(M.NAMES, (mo.pivot, mo.sum, mo.sum2, mo.min, mo.max)):
        M.same(got, np.ascontiguousarray(st[k].T), f"{what}, {k}")


def spectrum_equal_over(sp, samples, steps, start, stride, what, first=0):
    st = SP.run(samples, steps, sp.tw.numpy(), start, stride, first=first)
    assert sp.count == SP.count(st, stride) > 0 and sp.origin == int(st["window"][0]), (what, sp)
    for k, got in zip(SP.NAMES, (sp.pivot, sp.sum, sp.re.flatten(1), sp.im.flatten(1))):
        SP.same(got, np.ascontiguousarray(st[k].T), f"{what}, {k}")


def forces_equal_the_replay(rf, rep, what, first=0, moments=(1, 2), wall=(0, 1), spectrum=(0, 1)):
    R.same(rf.sums, np.stack([s for s, _, _ in rep]), what + ": sums")
    assert torch.equal(rf.pressure[..., 2], rf.sums[..., 4]) and torch.equal(rf.total, rf.pressure + rf.viscous) and bool(rf.viscous.abs().sum() > 0)
    run = rep[first:]
    if rf.moments is not None:
        moments_equal_over(rf.moments, [c for _, c, _ in run], N_OUT, *moments, what + ": force_moments", first=first)
    if rf.wall_moments is not None:
        moments_equal_over(rf.wall_moments, [w for _, _, w in run], N_OUT, *wall, what + ": wall_moments", first=first)
    if rf.spectrum is not None:
        spectrum_equal_over(rf.spectrum, [c for _, c, _ in run], N_OUT, *spectrum, what + ": force_spectrum", first=first)


@pytest.mark.parametrize("capture", [True, False])
@pytest.mark.parametrize("reorder", [False, True])
def test_rollout_forces_equal_the_replay_over_the_result(mesh, reorder, capture):
    spec = gfd.Spectrum([0, 1, 2], start=0, stride=1)
    with Rollout(mesh["model"], mesh["g"], N_OUT, capture=capture, reorder=reorder, every=1, forces=mesh["op"], force_moments=(1, 2),
                 wall_moments=True, force_spectrum=spec) as ro:
        ro.run(N_OUT)
        assert (ro._perm is not None) == reorder
        res, rf = ro.result(), ro.forces()
    what = f"reorder {reorder} capture {capture}"
    if not reorder:
        assert torch.equal(res, mesh["full"])
    assert type(rf) is gfd.nn.RolloutForces and rf.steps == N_OUT and tuple(rf.pressure.shape) == (N_OUT, 2, 3) and rf.target is None
    assert torch.equal(rf.angle, mesh["op"].angle) and rf.body_offsets.tolist() == [0, 64, 104]
    forces_equal_the_replay(rf, replay(mesh["op"], res), what)
    assert rf.moments.count == 3 and rf.wall_moments.count == N_OUT and rf.spectrum.complete and tuple(rf.wall_moments.pivot.shape) == (104, 2)
    mesh["runs"][(reorder, capture)] = rf
    other = mesh["runs"].get((reorder, not capture))
    if other is not None:                                      # captured and eager: the same bits
        assert torch.equal(rf.sums, other.sums) and torch.equal(rf.moments.sum2, other.moments.sum2)
        assert torch.equal(rf.wall_moments.sum2, other.wall_moments.sum2) and torch.equal(rf.spectrum.re, other.spectrum.re)


def test_a_rollout_without_forces_is_what_it_was(mesh, monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a rollout without forces launched body_forces")
    calls, plain = [], ops.rollout_advance
    for name in ("body_forces", "mesh_gradient_weights", "rollout_moments", "rollout_spectrum", "mesh_derived", "sample_points", "rollout_advance_record"):
        monkeypatch.setattr(ops, name, refuse)
    monkeypatch.setattr(ops, "rollout_advance", lambda *a, **k: (calls.append(1), plain(*a, **k))[1])
    with Rollout(mesh["model"], mesh["g"], N_OUT, reorder=False, capture=False) as ro:
        ro.run(N_OUT)
        assert ro._forces is None and len(calls) == N_OUT and torch.equal(ro.result(), mesh["full"])
        with pytest.raises(RuntimeError, match="forces"):
            ro.forces()
    assert torch.equal(mesh["model"].solve(mesh["g"].clone(), N_OUT), mesh["full"])
    with pytest.raises(AssertionError, match="without forces"):
        with Rollout(mesh["model"], mesh["g"], N_OUT, reorder=False, forces=mesh["op"]) as ro:
            ro.run(1)


def test_rewind_leaves_the_forces_of_the_steps_since(mesh):
    g, f0, op = mesh["g"], mesh["g"].field, mesh["op"]
    try:
        with Rollout(mesh["model"], g, N_OUT, reorder=False, every=1, forces=op, force_moments=(0, 2), wall_moments=1,
                     force_spectrum=gfd.Spectrum([0, 1], start=0, stride=2)) as ro:
            ro.run(3)
            before = ro.forces()
            forces_equal_the_replay(before, replay(op, ro.result())[:3], "before rewind", moments=(0, 2), wall=(1, 1), spectrum=(0, 2))
            ro.rewind()                                   # the device step index is 1 again: rows 1, 2, ... are written next
            assert ro.forces().moments.count == 0 and ro.forces().spectrum.count == 0 and ro.forces().wall_moments.count == 0
            ro.run(4)
            res, rf = ro.result(), ro.forces()
        assert rf.steps == 5 and torch.equal(res[:, 3:12], mesh["full"][:, 9:18])          # steps 3 .. 5 of the rollout sit in slots 1 .. 3
        assert torch.equal(rf.sums[0], before.sums[0]) and not torch.equal(rf.sums[1], before.sums[1])
        forces_equal_the_replay(rf, replay(op, res)[:5], "after rewind", first=1, moments=(0, 2), wall=(1, 1), spectrum=(0, 2))
        assert rf.moments.origin == 2 and rf.moments.count == 2
    finally:
        g.field = f0


def test_a_clipped_rollout_leaves_the_forces_of_its_recomputation(mesh):
    """Inputs of 1e5 leave the fp16 range: the steps are computed again in bf16x6 and the forces are those of the second pass."""
    g, f0, op = mesh["g"], mesh["g"].field, mesh["op"]

    def run(precision=None):
        old = ops.set_mlp_precision(precision) if precision else None
        try:
            g.field = f0 * 1e5
            with Rollout(mesh["model"], g, N_OUT, reorder=False, every=1, forces=op, force_moments=(1, 2), wall_moments=True) as ro:
                ro.run(N_OUT)
                return ro.result().clone(), ro.forces(), ro
        finally:
            g.field = f0
            if old:
                ops.set_mlp_precision(old)

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res, rf, ro = run()
        res_x, rf_x, ro_x = run("bf16x6")
    assert ro.exact_range and not ro_x.exact_range and torch.equal(res, res_x)
    assert torch.equal(rf.sums, rf_x.sums) and torch.equal(rf.moments.sum2, rf_x.moments.sum2) and torch.equal(rf.wall_moments.sum, rf_x.wall_moments.sum)
    forces_equal_the_replay(rf, replay(op, res), "clipped", wall=(0, 1))


def test_forces_and_evaluate_agree_with_the_rollout(mesh):
    g, model, op = mesh["g"].clone(), mesh["model"], mesh["op"]
    rep = replay(op, mesh["full"])
    rf = model.forces(g.clone(), N_OUT, op, discard=1, stride=2, wall=True, spectrum=gfd.Spectrum([0, 1], start=1, stride=2), capture=False)
    forces_equal_the_replay(rf, rep, "forces()", wall=(1, 2), spectrum=(1, 2))
    # built from keyword arguments: the graph's own bound == 4 and the labels
    built = model.forces(g.clone(), N_OUT, mesh["labels"], nodes=mesh["nodes"], mu=MU, scale=SCALE, shift=SHIFT)
    assert torch.equal(built.sums, rf.sums) and built.moments is None and built.spectrum is None
    walled = g.clone()
    walled.bound = mesh["bound"]
    one = model.forces(walled, N_OUT, mu=MU, scale=SCALE, shift=SHIFT, centre=op.centre[:1].tolist())          # bound == 4: one body of 104 items
    assert tuple(one.sums.shape) == (N_OUT, 1, 6)
    both = model.forces(walled, N_OUT, mesh["labels"], mu=MU, scale=SCALE, shift=SHIFT)
    assert torch.equal(both.sums, rf.sums)
    with pytest.raises(ValueError, match="carries its own"):
        model.forces(g.clone(), N_OUT, op, mu=1.0)
    # evaluate: the same forces, and the target's by one more launch per step
    g.target = torch.randn(g.num_nodes, NF * N_OUT + 2, generator=torch.Generator().manual_seed(5)).to(DEV)
    plain = model.evaluate(g.clone(), N_OUT)
    assert plain.forces is None
    errs = model.evaluate(g.clone(), N_OUT, forces=op, force_moments=(1, 2))
    assert torch.equal(errs.sums, plain.sums) and torch.equal(errs.forces.sums, rf.sums) and torch.equal(errs.forces.moments.sum2, rf.moments.sum2)
    want = op.history(g.target, N_OUT, nf=NF)
    assert tuple(errs.forces.target.shape) == (N_OUT, 2, 6) and torch.equal(errs.forces.target, want.cpu())
    R.same(want[3], op.forces(g.target[:, 3 * NF:4 * NF]).cpu().numpy(), "history against forces")
    for reorder in (False, True):                              # the target's rows follow the renumbering
        with Rollout(model, g, N_OUT, reorder=reorder, every=0, forces=op, target=g.target, target_forces=True) as ro:
            ro.run(N_OUT)
            assert torch.equal(ro.forces().target, want.cpu())
    with pytest.raises(ValueError, match="^forces"):
        model.evaluate([g.clone(), g.clone()], N_OUT, forces=op)
    with pytest.raises(ValueError, match="^target_forces"):
        Rollout(model, mesh["g"], N_OUT, forces=op, target_forces=True)


def test_coefficients_and_strouhal_of_a_synthetic_lift(mesh):
    """A hand-made target whose pressure is −(A cos ωt / area) y + 1: the lift is A cos ωt, the drag 0; fed through `history`."""
    g = mesh["g"]
    n, b, amp, dt, D, U, rho = 32, 4, 0.75, 0.05, 0.3, 2.0, 1.2
    ring = torch.nonzero(mesh["labels"] == 10).flatten()
    op = gfd.BodyForces(g, mesh["nodes"][ring.to(DEV)])
    area = R.shoelace(g.pos.cpu().double().numpy()[op.items.cpu().numpy()])
    t = torch.arange(n, dtype=torch.float64)
    lift = amp * torch.cos(2 * math.pi * b * t / n)
    target = torch.zeros(g.num_nodes, NF * n, dtype=torch.float64)
    target[:, 2::NF] = 1.0 - g.pos[:, 1:2].cpu().double() * (lift / area)[None, :]
    hist = op.history(target.float().to(DEV), n, nf=NF)
    # the spectrum of the per-step total, by the restatement over the table a rollout would use
    tw, w, freqs = ops.spectrum_table(bins=[0, 2, 4, 8], samples=n, dt=dt)
    st = SP.run([c for c in R.cur32(hist.cpu().numpy().reshape(n, 6)).reshape(n, 1, 3)], n, tw.numpy())
    sp = gfd.nn.RolloutSpectrum(n, 0, 1, dt, "rect", freqs, tw, w, *(torch.from_numpy(np.ascontiguousarray(st[k].T)) for k in ("pivot", "sum")),
                                torch.from_numpy(np.ascontiguousarray(st["re"].T)).unflatten(1, (3, 4)), torch.from_numpy(np.ascontiguousarray(st["im"].T)).unflatten(1, (3, 4)))
    rf = gfd.nn.RolloutForces(hist.cpu(), spectrum=sp)
    cd, cl, cm = rf.coefficients(rho, U, D)
    q = 0.5 * rho * U * U * D
    # the pressure was rounded to fp32 once: 2⁻²⁴ |p| on every item, times the item's area
    tol = 2.0 ** -23 * float((1.0 + amp / area) * op.area.abs().sum())
    assert float((cl[:, 0] * q - lift).abs().max()) <= tol and float((cd[:, 0] * q).abs().max()) <= tol
    assert rf.strouhal(D, U) == float(freqs[2]) * D / U == pytest.approx((b / (n * dt)) * D / U, rel=1e-12)
    assert abs(float(sp.amplitude[0, 1, 2]) - amp) <= tol * 2
    with pytest.raises(ValueError, match="^body"):
        rf.strouhal(D, U, body=1)
