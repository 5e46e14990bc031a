"""g4c_rollout_advance_record (csrc/rollout_record.hip) through ops.rollout_advance_record against the fp64 restatement of
tests/record_ref.py, and the records of `Rollout` / `GNN.solve(every=)` / `GNN.evaluate` against the full result of `solve`.

Kernel level: eight consecutive launches with max_steps = 7 (the eighth is past the record: it moves the field and the step and
writes nothing else).  Every record buffer starts as a sentinel and is compared WHOLE with the restatement after every launch, so
every element a launch does not own — other steps' slots, other snapshot slots, rows of `stats` of steps not run — must still hold
what it held.  Bit for bit: field, step, snapshots, probes on any data; all six statistics on small integers; max |d| on floats.  On
float data the five sums are held to 2 (n + 4) 2^-53 sum|terms| (record_ref.stats_close prints measured / allowed)."""
import os
import sys
import warnings

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

import record_ref as R                                   # noqa: E402
import graphs4cfd_amd as gfd                             # noqa: E402
from graphs4cfd_amd import _lib, ops, synthetic as S     # noqa: E402
from graphs4cfd_amd.nn.model import Rollout              # noqa: E402

DEV = torch.device("cuda", 0)
F32, F64, I32 = torch.float32, torch.float64, torch.int32
SENT = -7777.0
STEPS = 7
U64 = 2.0 ** -53


def _draw(kind, gen, offset):
    if kind == "int":
        return lambda *s: torch.randint(-8, 9, s, generator=gen).to(F32)
    return lambda *s: (torch.randn(*s, generator=gen, dtype=F64) + offset).to(F32)


def run_launches(n, nf, cols, every, n_probe, mask_kind, kind, with_target=True, offset=0.0, launches=STEPS + 1, check=True):
    """`launches` consecutive launches on one stream, each compared with the restatement; returns the final device buffers."""
    gen = torch.Generator().manual_seed(1000 * n + 10 * nf + every)
    draw = _draw(kind, gen, offset)
    field0, preds = draw(n, cols), [draw(n, nf) for _ in range(launches)]
    wide = draw(n, nf * STEPS + 5)                                  # the target is the column window 2 .. 2 + nf * STEPS + 1 of it
    mask = {None: None, "zero": torch.zeros(n, dtype=torch.bool), "mixed": torch.rand(n, generator=gen) < 0.3}[mask_kind]
    rows = {0: None, 1: torch.tensor([n // 2], dtype=I32), 5: torch.tensor([0, 3 % n, 3 % n, n // 2, n - 1], dtype=I32)}[n_probe]
    n_snap = STEPS // every if every else 0

    def sentinel(shape, dtype=F32):
        return torch.full(shape, SENT, dtype=dtype, device=DEV)

    dev = dict(snap=sentinel((n_snap, n, nf)) if every else None, probe_rows=None if rows is None else rows.to(DEV),
               probe_out=None if rows is None else sentinel((STEPS, n_probe, nf)))
    tgt = None
    if with_target:
        tgt = wide.to(DEV)[:, 2:2 + nf * STEPS + 1]
        assert not tgt.is_contiguous() or n <= 1
        dev.update(target=tgt, mask=None if mask is None else mask.to(DEV), stats=sentinel((STEPS, nf, R.NSTAT), F64),
                   scratch=ops.rollout_record_scratch(n, nf, DEV))
    field, step = field0.to(DEV).clone(), torch.zeros(2, dtype=I32, device=DEV)
    ref = dict(snap=None if every == 0 else torch.full((n_snap, n, nf), SENT, dtype=F64),
               probe_out=None if rows is None else torch.full((STEPS, n_probe, nf), SENT, dtype=F64),
               stats=torch.full((STEPS, nf, R.NSTAT), SENT, dtype=F64) if with_target else None)
    ref_field = field0.double()
    worst = 0.0
    for t in range(launches):
        ops.rollout_advance_record(field, preds[t].to(DEV), step, nf, STEPS, every=every, **dev)
        if not check:
            continue
        o = R.advance_record(ref_field, preds[t], t, STEPS, every=every, probe_rows=rows, target=None if tgt is None else tgt.cpu(),
                             mask=mask, **ref)
        ref_field, ref = o["field"], dict(snap=o["snap"], probe_out=o["probe_out"], stats=o["stats"])
        what = f"n {n} nf {nf} cols {cols} every {every} probes {n_probe} mask {mask_kind} {kind} launch {t}"
        assert step.tolist() == [t + 1, 0] and o["step"] == t + 1, what
        R.same(field, ref_field, what + ", field")
        for k in ("snap", "probe_out"):
            if ref[k] is not None:
                R.same(dev[k], ref[k], f"{what}, {k}")
        if with_target:
            got = dev["stats"].cpu()
            if kind == "int":
                R.same(got, ref["stats"], what + ", stats")
            else:
                done = min(t + 1, STEPS)
                R.same(got[done:], ref["stats"][done:], what + ", stats of steps not run")
                for s in range(done):
                    absref = R.step_stats(preds[s], tgt.cpu(), s, mask)[1]
                    worst = max(worst, R.stats_close(got[s], ref["stats"][s], absref, n, f"{what}, stats[{s}]"))
    return dev, field, step, worst


# every (n_nodes, nf) of the issue's grid, the other parameters dealt round so that each value meets several shapes
NODES, FIELDS = (1, 255, 256, 257, 1000), (1, 3, 4)
EVERY, PROBES, MASKS = (0, 1, 2, 3, 9), (0, 1, 5), (None, "zero", "mixed")
GRID = [(n, nf, (nf, 2 * nf, 3 * nf + 1)[(i + j) % 3], EVERY[(i + 2 * j) % 5], PROBES[(i + j + 1) % 3], MASKS[(2 * i + j) % 3])
        for i, n in enumerate(NODES) for j, nf in enumerate(FIELDS)]


@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("n,nf,cols,every,n_probe,mask_kind", GRID)
def test_records_match_the_restatement(n, nf, cols, every, n_probe, mask_kind, kind):
    run_launches(n, nf, cols, every, n_probe, mask_kind, kind)


@pytest.mark.parametrize("every", EVERY)
@pytest.mark.parametrize("n_probe", PROBES)
def test_records_without_a_target(every, n_probe):
    """The launch without statistics (any nf: 3, and 9, which the statistics refuse)."""
    run_launches(257, 3, 7, every, n_probe, None, "float", with_target=False)
    run_launches(1000, 9, 19, every, n_probe, None, "int", with_target=False)


@pytest.mark.parametrize("kind", ["int", "float"])
def test_eight_fields_and_every_mask(kind):
    for mask_kind in MASKS:
        run_launches(257, 8, 17, 3, 5, mask_kind, kind)


@pytest.mark.parametrize("kind", ["int", "float"])
def test_large_mesh_takes_several_rows_per_thread(kind):
    """300 001 rows on at most 1024 workgroups of 256: 37 857 threads take a second row."""
    run_launches(300_001, 3, 7, 2, 5, "mixed", kind, launches=3)


def test_sums_of_data_with_a_common_offset():
    """pred and target = 1e4 + N(0, 1): the sums of y and y^2 carry 1e4 n and 1e8 n, the error sums stay O(n)."""
    worst = run_launches(1000, 3, 6, 1, 1, "mixed", "float", offset=1e4)[3]
    assert worst <= 1.0


def test_nine_fields_with_a_target_are_refused():
    n, nf = 50, 9
    field, pred, step = torch.full((n, nf), SENT, device=DEV), torch.zeros(n, nf, device=DEV), torch.zeros(2, dtype=I32, device=DEV)
    stats = torch.full((STEPS, nf, R.NSTAT), SENT, dtype=F64, device=DEV)
    with pytest.raises(NotImplementedError):
        ops.rollout_record_scratch(n, nf, DEV)
    with pytest.raises(NotImplementedError):
        ops.rollout_advance_record(field, pred, step, nf, STEPS, target=torch.zeros(n, nf * STEPS, device=DEV), stats=stats,
                                   scratch=torch.zeros(4096, dtype=F64, device=DEV))
    assert step.tolist() == [0, 0] and bool((field == SENT).all()) and bool((stats == SENT).all())


def test_no_nodes_advance_the_step():
    step = torch.zeros(2, dtype=I32, device=DEV)
    stats = torch.full((STEPS, 3, R.NSTAT), SENT, dtype=F64, device=DEV)
    for t in range(3):
        ops.rollout_advance_record(torch.zeros(0, 6, device=DEV), torch.zeros(0, 3, device=DEV), step, 3, STEPS,
                                   snap=torch.zeros(STEPS, 0, 3, device=DEV), every=1, probe_rows=torch.zeros(0, dtype=I32, device=DEV),
                                   probe_out=torch.zeros(STEPS, 0, 3, device=DEV), target=torch.zeros(0, 3 * STEPS, device=DEV),
                                   stats=stats, scratch=ops.rollout_record_scratch(0, 3, DEV))
        assert step.tolist() == [t + 1, 0]
    assert bool((stats == SENT).all())


def test_a_recomputed_step_replaces_its_record():
    """The step index decides the slot: set back to 2, the launch overwrites stats[2], probe_out[2] and nothing else."""
    n, nf = 257, 3
    dev, field, step, _ = run_launches(n, nf, 7, 1, 5, "mixed", "int", launches=5)
    before = {k: dev[k].clone() for k in ("snap", "probe_out", "stats")}
    step.copy_(torch.tensor([2, 0], dtype=I32))
    pred = torch.randint(-8, 9, (n, nf), generator=torch.Generator().manual_seed(5)).to(F32)
    field_before = field.cpu().clone()
    ops.rollout_advance_record(field, pred.to(DEV), step, nf, STEPS, every=1, **dev)
    assert step.tolist() == [3, 0]
    want = R.advance_record(field_before, pred, 2, STEPS, every=1, probe_rows=dev["probe_rows"].cpu(), target=dev["target"].cpu(),
                            mask=dev["mask"].cpu(), **{k: v.cpu() for k, v in before.items()})
    R.same(field, want["field"], "field")
    for k in before:
        R.same(dev[k], want[k], k)
        assert not torch.equal(dev[k][2], before[k][2]), k
        assert torch.equal(dev[k][:2], before[k][:2]) and torch.equal(dev[k][3:], before[k][3:]), k


def test_statistics_are_reproducible():
    a = run_launches(1000, 3, 7, 2, 5, "mixed", "float", check=False)[0]["stats"].clone()
    b = run_launches(1000, 3, 7, 2, 5, "mixed", "float", check=False)[0]["stats"]
    assert torch.equal(a, b) and bool((a != SENT).all())


def test_negative_controls_on_the_launch():
    """The launch's own records fail the checkers against a restatement with one mistake (tests/test_rollout_record_ref.py runs the
    same controls on the host)."""
    n, nf = 257, 3
    dev, _, _, _ = run_launches(n, nf, 7, 2, 5, "mixed", "float", launches=3)
    gen = torch.Generator().manual_seed(1000 * n + 10 * nf + 2)
    draw = _draw("float", gen, 0.0)
    field0, preds, wide = draw(n, 7), [draw(n, nf) for _ in range(3)], draw(n, nf * STEPS + 5)
    mask = torch.rand(n, generator=gen) < 0.3
    rows, tgt = dev["probe_rows"].cpu(), wide[:, 2:2 + nf * STEPS + 1]
    for wrong in (None,) + R.WRONG:
        ref = dict(snap=torch.full((3, n, nf), SENT, dtype=F64), probe_out=torch.full((STEPS, 5, nf), SENT, dtype=F64),
                   stats=torch.full((STEPS, nf, R.NSTAT), SENT, dtype=F64))
        f = field0
        for t in range(3):
            o = R.advance_record(f, preds[t], t, STEPS, every=2, probe_rows=rows, target=tgt, mask=mask, wrong=wrong, **ref)
            f, ref = o["field"], dict(snap=o["snap"], probe_out=o["probe_out"], stats=o["stats"])

        def check():
            R.same(dev["snap"], ref["snap"], "snap")
            R.same(dev["probe_out"], ref["probe_out"], "probe_out")
            for s in range(3):
                R.stats_close(dev["stats"][s], ref["stats"][s], R.step_stats(preds[s], tgt, s, mask)[1], n, f"stats[{s}]")

        assert R.rejects(check) == (wrong is not None), wrong


# ====================================================================== Rollout / solve / evaluate
N_OUT = 6


@pytest.fixture(scope="module")
def mesh():
    g = S.mus_graph(2000, levels=2, seed=3).to(DEV)
    g.batch = torch.zeros(g.num_nodes, dtype=torch.long, device=DEV)
    torch.manual_seed(4)
    model = gfd.nn.NsTwoScaleGNN(arch=S.mus_arch("NsTwoScaleGNN", 128), device=DEV)
    model.eval()
    gen = torch.Generator().manual_seed(5)
    target = torch.randn(g.num_nodes, 3 * N_OUT + 2, generator=gen)
    probes = torch.tensor([0, 17, 17, 1234, g.num_nodes - 1])
    mask = (g.omega[:, 0] == 1)
    full = {}
    for reorder in (False, True):
        with Rollout(model, g, N_OUT, capture=True, reorder=reorder) as ro:
            ro.run(N_OUT)
            full[reorder] = ro.result().clone()
            assert (ro._perm is not None) == reorder
    return dict(g=g, model=model, target=target, probes=probes, mask=mask, full=full)


def steps_of(full, steps, nf=3):
    return full.reshape(full.size(0), -1, nf)[:, steps].reshape(full.size(0), -1)


def recorded(m, reorder=False, capture=True, every=2, field_scale=1.0, precision=None):
    """One recording rollout of N_OUT steps: (snapshots, probes, sums, the Rollout)."""
    g, f0 = m["g"], m["g"].field
    old = ops.set_mlp_precision(precision) if precision else None
    try:
        g.field = f0 * field_scale
        with Rollout(m["model"], g, N_OUT, capture=capture, reorder=reorder, every=every, probes=m["probes"], target=m["target"].to(DEV),
                     mask=m["mask"]) as ro:
            ro.run(N_OUT)
            e = ro.errors()
            return (ro.result().clone() if every else None), ro.probes().clone(), e, ro
    finally:
        g.field = f0
        if old:
            ops.set_mlp_precision(old)


def test_solve_every(mesh):
    g, model, full = mesh["g"], mesh["model"], mesh["full"][False]
    assert torch.equal(model.solve(g.clone(), N_OUT), full)
    assert torch.equal(model.solve(g.clone(), N_OUT, every=1), full)
    assert torch.equal(model.solve(g.clone(), N_OUT, every=2), steps_of(full, [1, 3, 5]))
    assert torch.equal(model.solve(g.clone(), N_OUT, every=4), steps_of(full, [3]))
    with pytest.raises(ValueError, match="every"):
        model.solve(g.clone(), N_OUT, every=0)


@pytest.mark.parametrize("reorder", [False, True])
def test_rollout_records_equal_the_full_result(mesh, reorder):
    full = mesh["full"][reorder]
    snaps, probes, errs, ro = recorded(mesh, reorder=reorder)
    assert tuple(ro._out_steps.shape) == (N_OUT // 2, mesh["g"].num_nodes, 3)
    assert torch.equal(snaps, steps_of(full, [1, 3, 5]))
    assert torch.equal(probes, full[mesh["probes"].to(DEV)])
    assert torch.equal(errs.snapshots, snaps) and torch.equal(errs.probes, probes)
    # eager steps leave the same records as replayed ones, bit for bit
    snaps_e, probes_e, errs_e, _ = recorded(mesh, reorder=reorder, capture=False)
    assert torch.equal(snaps_e, snaps) and torch.equal(probes_e, probes) and torch.equal(errs_e.sums, errs.sums)
    _errors_against_the_host(errs, full, mesh, f"reorder {reorder}")


def _errors_against_the_host(errs, full, m, what, nf=3):
    """errors() and graph_loss(0.5) against the same quantities in fp64 on the host, from the full result and the target.  The sums
    within B sum|terms|, B = 2 (n + 4) 2^-53; a quotient of sums within the propagated bound (+ 4 ulp of its own roundings)."""
    n = int(full.size(0))
    B = 2.0 * (n + 4) * U64
    mask = None if m["mask"] is None else m["mask"].cpu()
    assert errs.steps == N_OUT and tuple(errs.sums.shape) == (N_OUT, nf, R.NSTAT) and errs.sums.dtype == F64 and not errs.sums.is_cuda
    pred, tgt = full.cpu(), m["target"].cpu()
    loss = gfd.nn.GraphLoss(0.5)
    omega = None if mask is None else mask.double()[:, None]
    for t in range(N_OUT):
        p = pred[:, nf * t:nf * (t + 1)]
        ref, absref = R.step_stats(p, tgt, t, mask)
        R.stats_close(errs.sums[t], ref, absref, n, f"{what}, step {t}")
        y, d = tgt[:, nf * t:nf * (t + 1)].double(), p.double() - tgt[:, nf * t:nf * (t + 1)].double()

        def close(got, want, allow, name):
            assert bool(((got - want).abs() <= allow + 4 * U64 * want.abs()).all()), f"{what}, step {t}, {name}: {got} vs {want}"

        close(errs.mse[t], (d * d).mean(0), B * (d * d).mean(0), "mse")
        close(errs.mae[t], d.abs().mean(0), B * d.abs().mean(0), "mae")
        assert torch.equal(errs.max_abs[t], d.abs().max(0).values)
        den = (y * y).sum(0) - y.sum(0) ** 2 / n
        dden = B * ((y * y).sum(0) + 2 * y.sum(0).abs() * y.abs().sum(0) / n)
        sq = (d * d).sum(0)
        close(errs.r2[t], 1.0 - sq / den, B * sq / den + sq * dden / den ** 2, "r2")
        if mask is not None:
            k = int(mask.sum())
            close(errs.mae_masked[t], d[mask].abs().sum(0) / k, B * d.abs().sum(0) / k, "mae_masked")
            want = loss(gfd.Graph(omega=omega), p.double(), y)
            close(errs.graph_loss(0.5)[t], want, B * want.abs(), "graph_loss(0.5)")
        else:
            assert errs.mae_masked is None
        close(errs.graph_loss(0.0)[t], (d * d).mean(), B * (d * d).mean(), "graph_loss(0)")


def test_every_zero_keeps_no_prediction_buffer(mesh):
    snaps, probes, errs, ro = recorded(mesh, every=0)
    assert snaps is None and ro._out_steps is None and errs.snapshots is None
    assert not any(torch.is_tensor(v) and v.dim() == 3 and tuple(v.shape) == (N_OUT, mesh["g"].num_nodes, 3)
                   for v in list(vars(ro).values()) + list(vars(ro._rec).values()))
    with pytest.raises(RuntimeError, match="every=0"):
        ro.result()
    assert torch.equal(probes, mesh["full"][False][mesh["probes"].to(DEV)])
    assert torch.equal(errs.sums, recorded(mesh, every=2)[2].sums)


def test_a_clipped_rollout_leaves_the_records_of_its_recomputation(mesh):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        snaps, probes, errs, ro = recorded(mesh, field_scale=1e5)
        snaps_x, probes_x, errs_x, ro_x = recorded(mesh, field_scale=1e5, precision="bf16x6")
    assert ro.exact_range and not ro_x.exact_range
    assert torch.isfinite(snaps).all()
    assert torch.equal(snaps, snaps_x) and torch.equal(probes, probes_x) and torch.equal(errs.sums, errs_x.sums)


def test_a_plain_rollout_still_ends_in_rollout_advance(mesh, monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a rollout without records went through rollout_advance_record")
    monkeypatch.setattr(ops, "rollout_advance_record", refuse)
    g, model = mesh["g"], mesh["model"]
    with Rollout(model, g, N_OUT, reorder=False) as ro:
        ro.run(N_OUT)
        assert ro._rec is None and torch.equal(ro.result(), mesh["full"][False])
    assert torch.equal(model.solve(g.clone(), N_OUT), mesh["full"][False])
    with pytest.raises(AssertionError, match="rollout_advance_record"):
        with Rollout(model, g, N_OUT, reorder=False, every=2) as ro:
            ro.run(1)


def test_rewind_keeps_the_slots_a_function_of_the_step_index(mesh):
    """After rewind() the device step index is 1: the next steps overwrite slots 1, 2, ... of every record."""
    g, f0 = mesh["g"], mesh["g"].field
    try:
        with Rollout(mesh["model"], g, N_OUT, reorder=False, every=1, probes=mesh["probes"], target=mesh["target"].to(DEV)) as ro:
            ro.run(3)
            first = ro.errors().sums.clone()
            ro.rewind()
            ro.run(2)
            e = ro.errors()
            assert e.steps == 3 and torch.equal(e.sums[0], first[0]) and not torch.equal(e.sums[1:], first[1:])
            assert e.mae_masked is None
            full = mesh["full"][False]
            # steps 3 and 4 of the rollout now sit in slots 1 and 2, scored against the target's steps 1 and 2
            assert torch.equal(ro.result()[:, 3:9], steps_of(full, [3, 4]))
            assert torch.equal(ro.probes()[:, 3:9], steps_of(full, [3, 4])[mesh["probes"].to(DEV)])
    finally:
        g.field = f0


def test_evaluate(mesh):
    g, model = mesh["g"].clone(), mesh["model"]
    g.target = mesh["target"][:, :3 * N_OUT].to(DEV)
    errs = model.evaluate(g.clone())
    assert errs.steps == N_OUT and errs.snapshots is None and errs.probes is None and errs.n_masked == int(mesh["mask"].sum())
    assert torch.equal(errs.sums, recorded(mesh, every=2)[2].sums)
    some = model.evaluate(g.clone(), 4, every=2, probes=mesh["probes"])
    assert some.steps == 4 and torch.equal(some.sums, errs.sums[:4])
    assert torch.equal(some.snapshots, steps_of(mesh["full"][False], [1, 3]))
    assert torch.equal(some.probes, mesh["full"][False][mesh["probes"].to(DEV)][:, :12])
    assert gfd.nn.RolloutErrors is type(errs)
    import graphs4cfd
    assert graphs4cfd.nn.RolloutErrors is gfd.nn.RolloutErrors and graphs4cfd.nn.Rollout is Rollout


def test_evaluate_list_of_graphs():
    """A list of graphs is collated as in solve: one rollout of the batch, scored against the concatenated targets."""
    gen = torch.Generator().manual_seed(8)
    graphs = [S.mus_graph(n, levels=1, seed=20 + n).to(DEV) for n in (300, 500)]
    for gr in graphs:
        gr.target = torch.randn(gr.num_nodes, 3 * N_OUT, generator=gen).to(DEV)
    torch.manual_seed(9)
    model = gfd.nn.NsOneScaleGNN(arch=S.mus_arch("NsOneScaleGNN", 64), device=DEV)
    full = model.solve([gr.clone() for gr in graphs], N_OUT)
    errs = model.evaluate([gr.clone() for gr in graphs])
    assert errs.n_nodes == 800 and tuple(full.shape) == (800, 3 * N_OUT)
    m = dict(mask=torch.cat([gr.omega[:, 0] == 1 for gr in graphs]), target=torch.cat([gr.target for gr in graphs]))
    assert errs.n_masked == int(m["mask"].sum())
    _errors_against_the_host(errs, full, m, "two graphs")


def test_evaluate_remus():
    g = S.remus_graph(1500, k=5, seed=4).to(DEV)
    torch.manual_seed(6)
    model = gfd.nn.NsRotEquiTreeScaleGNN(arch=S.remus_arch(64), device=DEV)
    g.target = torch.randn(g.num_nodes, 2 * N_OUT, generator=torch.Generator().manual_seed(7)).to(DEV)
    full = model.solve(g.clone(), N_OUT)
    errs = model.evaluate(g.clone(), every=1, probes=torch.tensor([5, 1499]))
    assert torch.equal(errs.snapshots, full) and torch.equal(errs.probes, full[[5, 1499]])
    m = dict(mask=(g.omega[:, 0] == 1), target=g.target)
    _errors_against_the_host(errs, full, m, "REMuS", nf=2)
