"""`Rollout(tracers=, tracer_every=)`, `GNN.trace` and `GNN.evaluate(tracers=)` against a replay of `Tracers.advance` — one launch a
step, outside any rollout, which tests/test_gpu_tracers.py pins — over the input field and what the same rollout returns: the paths
are EQUAL, with and without capture, with and without the Morton renumbering, whose bits they do not depend on; `rewind()` continues
from the current positions, a recomputation starts again from the saved ones; a rollout without tracers is what it was."""
import os
import sys
import warnings

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

import graphs4cfd_amd as gfd                             # noqa: E402
from graphs4cfd_amd import ops, synthetic as S           # noqa: E402
from graphs4cfd_amd.nn.model import Rollout              # noqa: E402

DEV = torch.device("cuda", 0)
N_OUT, NF, N_SEEDS = 7, 3, 101


def seeds_in(g, n, seed):
    lo, hi = g.pos.min(0).values.cpu(), g.pos.max(0).values.cpu()
    return lo + (hi - lo) * (torch.rand(n, int(g.pos.size(1)), generator=torch.Generator().manual_seed(seed)) * 0.9 + 0.05)


@pytest.fixture(scope="module")
def mesh():
    g = S.mus_graph(3000, levels=3, seed=3).to(DEV)
    g.batch = torch.zeros(g.num_nodes, dtype=torch.long, device=DEV)
    torch.manual_seed(4)
    model = gfd.nn.NsThreeScaleGNN(arch=S.mus_arch("NsThreeScaleGNN", 128), device=DEV)
    model.eval()
    full = model.solve(g.clone(), N_OUT)
    # the largest |v| dt of the run is about one mean node spacing
    lo, hi = g.pos.min(0).values, g.pos.max(0).values
    spacing = float(((hi - lo).prod() / g.num_nodes).sqrt())
    vmax = max(float(full.view(-1, N_OUT, NF)[:, :, :2].abs().max()), float(g.field[:, -NF:-1].abs().max()))
    dt = spacing / vmax
    seeds = seeds_in(g, N_SEEDS, 5)
    seeds[:3] = g.pos[[0, 1500, 2999]].cpu()                                       # three seeds on nodes
    release = (torch.arange(N_SEEDS) % 4 == 1).int() * 3 + (torch.arange(N_SEEDS) % 9 == 2).int() * 20      # some late, some never
    box = ((float(lo[0]) + 0.1 * float(hi[0] - lo[0]), float("-inf")), (float("inf"), float(hi[1])))
    kw = dict(release=release, box=box, max_distance=3 * spacing)
    return dict(g=g, model=model, full=full, dt=dt, seeds=seeds, kw=kw, tracers=gfd.Tracers(g, seeds, dt, **kw), runs={}, spacing=spacing)


def step_columns(res, t):
    return res[:, NF * t:NF * (t + 1)]


def replay(tr, x_first, res, steps, every, t0=0):
    """Slots of `tr`'s positions after steps t0 .. t0 + steps − 1: x0 of the first step is `x_first`, then column block after column
    block of `res` (whose block s is the prediction of step t0 + s)."""
    kept, x0 = [], x_first
    for s in range(steps):
        x1 = step_columns(res, s)
        tr.advance(x0, x1, t0 + s)
        x0 = x1
        if (t0 + s + 1) % every == 0:
            kept.append(tr.positions.clone())
    return torch.cat(kept, dim=1) if kept else None


def fresh(mesh, **kw):
    return gfd.Tracers(mesh["g"], mesh["seeds"], mesh["dt"], **dict(mesh["kw"], **kw))


@pytest.mark.parametrize("capture", [True, False])
@pytest.mark.parametrize("reorder", [False, True])
def test_rollout_paths_equal_a_replay_over_the_result(mesh, reorder, capture):
    g, tr = mesh["g"], mesh["tracers"]
    with Rollout(mesh["model"], g, N_OUT, capture=capture, reorder=reorder, every=1, tracers=tr, tracer_every=2) as ro:
        ro.run(N_OUT)
        assert (ro._perm is not None) == reorder
        res, rt = ro.result(), ro.tracers()
    what = f"reorder {reorder} capture {capture}"
    if not reorder:
        assert torch.equal(res, mesh["full"]), what
    assert type(rt) is gfd.nn.RolloutTracers and rt.slots == 3 and tuple(rt.paths.shape) == (N_SEEDS, 2 * 3) and rt.target_paths is None
    # the caller's object is a description: the rollout moved a copy
    assert torch.equal(tr.positions, mesh["seeds"].to(DEV)) and int(tr.status.sum()) == 0
    ref = fresh(mesh)
    want = replay(ref, g.field[:, -NF:].float(), res, N_OUT, 2)
    assert torch.equal(rt.paths, want), what
    assert torch.equal(rt.positions, ref.positions) and torch.equal(rt.status, ref.status) and torch.equal(rt.stopped, ref.stopped), what
    assert torch.equal(rt.release, ref.release) and torch.equal(rt.seeds, ref.seeds)
    # the run is no trivial one: particles moved about a spacing a step, some wait for ever, some were released late, some left the box
    moved = (rt.positions - rt.seeds).norm(dim=1)
    assert float(moved.max()) > mesh["spacing"] and set(rt.status.tolist()) >= {0, 1, 2}, (float(moved.max()), set(rt.status.tolist()))
    late = rt.release == 3
    assert torch.equal(rt.paths[late][:, :2], rt.seeds[late]) and not torch.equal(rt.paths[late][:, 2:4], rt.seeds[late])
    assert torch.equal(rt.residence()[rt.status < 2], torch.full_like(rt.stopped[rt.status < 2], -1))
    # The same bits whatever the capture and the numbering.  The renumbered mesh adds its neighbours in another order, so its PREDICTIONS
    # differ in their last bits from the caller's numbering (tests/test_gpu_rollout_moments.py pins both) and particles carried by other
    # velocities go elsewhere: two runs are compared when their predictions are equal — the two captures of one numbering always are.
    # That the tracers themselves do not depend on the numbering is the replay above: `ref` searches the caller's cloud, the rollout
    # its renumbered one, over the same predictions.
    for (other_reorder, _), (other_res, other) in mesh["runs"].items():
        if other_reorder == reorder:
            assert torch.equal(res, other_res), what          # (captured and eager steps of one numbering predict the same)
        if torch.equal(res, other_res):
            assert torch.equal(rt.paths, other.paths) and torch.equal(rt.status, other.status) and torch.equal(rt.stopped, other.stopped), what
            assert torch.equal(rt.positions, other.positions), what
    mesh["runs"][(reorder, capture)] = (res, rt)


def test_a_rollout_without_tracers_is_what_it_was(mesh, monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a rollout without tracers launched tracer_advance")
    calls, plain = [], ops.rollout_advance
    for name in ("tracer_advance", "sample_points", "sample_weights", "rollout_moments", "rollout_spectrum", "mesh_derived", "rollout_advance_record"):
        monkeypatch.setattr(ops, name, refuse)
    monkeypatch.setattr(S, "knn_query_device", refuse)
    monkeypatch.setattr(S, "_bin_cloud", refuse)
    monkeypatch.setattr(ops, "rollout_advance", lambda *a, **k: (calls.append(1), plain(*a, **k))[1])
    with Rollout(mesh["model"], mesh["g"], N_OUT, reorder=False, capture=False) as ro:
        ro.run(N_OUT)
        assert ro._tracers is None and len(calls) == N_OUT and torch.equal(ro.result(), mesh["full"])
        with pytest.raises(RuntimeError, match="tracers"):
            ro.tracers()
    assert torch.equal(mesh["model"].solve(mesh["g"].clone(), N_OUT), mesh["full"])
    monkeypatch.undo()
    monkeypatch.setattr(ops, "tracer_advance", refuse)
    with pytest.raises(AssertionError, match="without tracers"):          # the guard itself fires when tracers are on
        with Rollout(mesh["model"], mesh["g"], N_OUT, reorder=False, tracers=mesh["tracers"]) as ro:
            ro.run(1)


def test_rewind_continues_from_the_current_positions(mesh):
    g, f0 = mesh["g"], mesh["g"].field
    try:
        with Rollout(mesh["model"], g, N_OUT, reorder=False, every=1, tracers=(mesh["seeds"], mesh["dt"], mesh["kw"]), tracer_every=1) as ro:
            ro.run(3)
            before, res_before = ro.tracers(), ro.result().clone()
            ref = fresh(mesh)
            assert torch.equal(before.paths[:, :6], replay(ref, f0[:, -NF:].float(), res_before, 3, 1))
            ro.rewind()                                   # the device step index is 1 again: slots 1, 2, ... are written next
            ro.run(4)
            res, rt = ro.result(), ro.tracers()
        assert torch.equal(res[:, 3:15], mesh["full"][:, 9:21])          # steps 3 .. 6 of the rollout sit in slots 1 .. 4
        # the replay goes on from where the particles were: steps 1 .. 4 by the index, from the prediction of step 2 through slots 1 .. 4
        want = replay(ref, step_columns(res_before, 2), res[:, 3:15], 4, 1, t0=1)
        assert torch.equal(rt.paths[:, 2:10], want) and torch.equal(rt.paths[:, :2], before.paths[:, :2])
        assert torch.equal(rt.positions, ref.positions) and torch.equal(rt.status, ref.status) and torch.equal(rt.stopped, ref.stopped)
        assert not torch.equal(rt.paths[:, 2:4], before.paths[:, 2:4])
    finally:
        g.field = f0


def test_a_clipped_rollout_leaves_the_tracers_of_its_recomputation(mesh):
    g, f0 = mesh["g"], mesh["g"].field
    kw = dict(mesh["kw"], max_distance=None, box=None)

    def run(precision=None):
        old = ops.set_mlp_precision(precision) if precision else None
        try:
            g.field = f0 * 1e5
            with Rollout(mesh["model"], g, N_OUT, reorder=False, every=1, tracers=(mesh["seeds"], mesh["dt"] * 1e-5, kw)) as ro:
                ro.run(N_OUT)
                return ro.result().clone(), ro.tracers(), ro
        finally:
            g.field = f0
            if old:
                ops.set_mlp_precision(old)

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res, rt, ro = run()
        res_x, rt_x, ro_x = run("bf16x6")
    assert ro.exact_range and not ro_x.exact_range and torch.equal(res, res_x)
    # the particles restarted from their seeds: the paths are those of a run made in "bf16x6" from the start
    assert torch.equal(rt.paths, rt_x.paths) and torch.equal(rt.status, rt_x.status) and torch.equal(rt.stopped, rt_x.stopped)
    ref = gfd.Tracers(g, mesh["seeds"], mesh["dt"] * 1e-5, **kw)
    assert torch.equal(rt.paths, replay(ref, (f0 * 1e5)[:, -NF:].float(), res, N_OUT, 1))
    assert not torch.equal(rt.positions, rt.seeds)


def test_trace_and_evaluate_agree_with_the_rollout(mesh):
    g, model = mesh["g"].clone(), mesh["model"]
    by_rollout = mesh["runs"].get((False, True), (None, None))[1]
    rt = model.trace(g.clone(), N_OUT, mesh["seeds"], mesh["dt"], every=2, **mesh["kw"])
    want = replay(fresh(mesh), g.field[:, -NF:].float(), mesh["full"], N_OUT, 2)
    assert rt.slots == 3 and torch.equal(rt.paths, want)
    if by_rollout is not None:
        assert torch.equal(rt.paths, by_rollout.paths) and torch.equal(rt.status, by_rollout.status)
    by_object = model.trace(g.clone(), N_OUT, mesh["tracers"], every=2, capture=False)
    assert torch.equal(by_object.paths, rt.paths) and torch.equal(by_object.stopped, rt.stopped)
    euler = model.trace(g.clone(), N_OUT, mesh["seeds"], mesh["dt"], every=0, scheme="euler", velocity=(1, 0))
    ref = gfd.Tracers(g, mesh["seeds"], mesh["dt"], scheme="euler", velocity=(1, 0))
    replay(ref, g.field[:, -NF:].float(), mesh["full"], N_OUT, 1)
    assert euler.paths is None and euler.slots == 0 and torch.equal(euler.positions, ref.positions) and not torch.equal(euler.positions, rt.positions)
    # evaluate: the same tracers, and the same particles carried by the target
    g.target = (0.5 * torch.randn(g.num_nodes, NF * N_OUT + 2, generator=torch.Generator().manual_seed(5))).to(DEV)
    plain = model.evaluate(g.clone(), N_OUT)
    assert plain.tracers is None
    errs = model.evaluate(g.clone(), N_OUT, tracers=mesh["tracers"], tracer_every=2)
    assert torch.equal(errs.sums, plain.sums) and torch.equal(errs.tracers.paths, rt.paths)
    want = replay(fresh(mesh), g.field[:, -NF:].float(), g.target[:, :NF * N_OUT], N_OUT, 2)
    assert tuple(errs.tracers.target_paths.shape) == (N_SEEDS, 2 * 3) and torch.equal(errs.tracers.target_paths, want)
    assert not torch.equal(errs.tracers.target_paths, errs.tracers.paths)
    with pytest.raises(ValueError, match="^tracers"):
        model.trace([g.clone(), g.clone()], N_OUT, mesh["seeds"], mesh["dt"])
    with pytest.raises(ValueError, match="^tracers"):
        model.evaluate([g.clone(), g.clone()], N_OUT, tracers=(mesh["seeds"], mesh["dt"]))


def test_a_streak_has_its_shape_and_keeps_the_unreleased_at_their_seeds(mesh):
    g, model = mesh["g"], mesh["model"]
    seeds = mesh["seeds"][3:8]
    streak = gfd.Tracers.streak(g, seeds, mesh["dt"], release_every=2, releases=4)          # released at steps 0, 2, 4, 6
    assert streak.groups == (4, 5) and streak.n_particles == 20
    rt = model.trace(g.clone(), N_OUT, streak, every=1)
    assert rt.groups == (4, 5) and rt.slots == N_OUT
    for slot in (0, 3, N_OUT - 1):
        line, released = rt.streakline(slot)
        assert tuple(line.shape) == (5, 4, 2) and tuple(released.shape) == (5, 4)
        assert released[0].tolist() == [slot >= r for r in (0, 2, 4, 6)]
        waiting = ~released
        assert torch.equal(line[waiting], seeds.to(DEV)[:, None, :].expand(5, 4, 2)[waiting])
        assert not bool((line[released] == seeds.to(DEV)[:, None, :].expand(5, 4, 2)[released]).all(-1).any())
    # the oldest particle of a streak is the pathline of a single release
    single = model.trace(g.clone(), N_OUT, seeds, mesh["dt"], every=1)
    assert torch.equal(rt.paths[:5], single.paths)
    assert torch.equal(rt.streakline(-1)[0], rt.paths[:, -2:].reshape(4, 5, 2).permute(1, 0, 2))


def test_remus():
    g = S.remus_graph(1500, k=5, seed=4).to(DEV)
    torch.manual_seed(6)
    model = gfd.nn.NsRotEquiTreeScaleGNN(arch=S.remus_arch(64), device=DEV)
    full = model.solve(g.clone(), N_OUT)
    lo, hi = g.pos.min(0).values, g.pos.max(0).values
    dt = float(((hi - lo).prod() / g.num_nodes).sqrt()) / float(full.abs().max())
    seeds = seeds_in(g, 33, 7)
    rt = model.trace(g.clone(), N_OUT, seeds, dt, every=3)
    assert rt.slots == 2 and rt.dim == 2
    ref, kept, x0 = gfd.Tracers(g, seeds, dt), [], g.field[:, -2:].float()
    for t in range(N_OUT):
        x1 = full[:, 2 * t:2 * t + 2]
        ref.advance(x0, x1, t)
        x0 = x1
        if (t + 1) % 3 == 0:
            kept.append(ref.positions.clone())
    assert torch.equal(rt.paths, torch.cat(kept, dim=1)) and torch.equal(rt.positions, ref.positions)
