"""The partitioned step on the HIP back-ends (HipImpl, RemusHipImpl, the overlapped interior / boundary launches, the real
HaloExchanger with its pack launch), every rank a thread on the one GPU (tests/partition_harness.py), pinned stage by stage to the
fp64 whole-mesh references of oracle/partition_ref.py.  Eager only: a hipGraph capture cannot span the thread barriers, and
captured == eager is held by test_gpu_parity.py.

Cases (MuS: NsThreeScaleGNN, width 128 — the heads path needs it —, 3000 nodes, 3 levels; REMuS: 6000 nodes, k = 5, width 128: the
smallest sizes at which every level / channel has halo rows on every rank at every world size run here, which is asserted):

  MuS    world 2, 3, 4   f16x3    HOIST_MIN_ROWS 0 (every MP layer hoists: first-layer products in the halo)   overlap on
  MuS    world 3         f16x3    0                                                                              overlap off
  MuS    world 3         f16x3    default (nobody hoists: latents in the halo)                                   overlap on
  MuS    world 3         f16x3    a value between the ranks' level-1 edge counts, decisions on uniform_edge_counts
  MuS    world 2         bf16x6   0                                                                              overlap on
  MuS    world 3         f16x3    0, two separated clouds: rank 0 has an empty halo on every level and still enters every exchange
  REMuS  world 2, 3      f16x3

Checks, in every case and for every rank:
 (a) after each exchange the halo rows are torch.equal to the owner's rows of the same tensor at that moment; under the NaN poison
     (fresh buffers are NaN; REMuS: halo rows are NaN again after every launch that writes own rows) every recorded output is finite;
     a MuS layer that takes products leaves the latents' halo rows NaN (HipImpl.mp's promise that they are not read); the kinds
     exchanged ("v" / "prod") are the same on every rank and are the ones the program implies — a node launch asked for products
     must deliver them (HipImpl._node_launch falls back silently when MLP.run_with_heads declines);
 (b) every recorded output, assembled over the ranks, is as accurate against the fp64 reference of ITS stage as the plain fp32
     evaluation of the same formula (fwd_ref.assert_as_accurate_as_fp32, its factors), separately for the rows that have a halo
     sender and those that do not;
 (c) the assembled prediction against O.mus_forward / O.remus_forward in float64: mean and 99.9th-percentile error within 1.15 x the
     single-rank HIP forward's own (the form and factor of test_distributed_remus_two_ranks_in_process_bf16);
 (d) overlap on == overlap off, bit for bit (e' of every layer, prediction);
 (e) negative controls, each REJECTED: a halo of the coarsest level one exchange old and two peers' slices swapped fail (a); a stage
     reference in which one boundary edge takes the next boundary edge's sender fails (b) for e'; a reference whose pooled coarse e
     is in the unsorted coarse edge order fails (b).  They perturb the transport or a reference, never a launch.

With G4C_PARTITION_REF_REPORT=<path> the worst ratios of (b) per case / output / row class and the figures of (c) are written there
as tables (tests/PARTITION_REF_MEASURED.md)."""
import contextlib
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

import graphs4cfd_amd as gfd                                                   # noqa: E402
import partition_harness as H                                                  # noqa: E402
from graphs4cfd_amd import ops, partition as P, partition_remus as PR, synthetic as S   # noqa: E402
from graphs4cfd_amd.graph import Graph                                         # noqa: E402
from graphs4cfd_amd.nn import blocks as B                                      # noqa: E402
from oracle import fwd_ref as R, g4c_oracle as O, partition_ref as PRf         # noqa: E402

DEV = torch.device("cuda", 0)
F64, F32 = torch.float64, torch.float32
MUS, WIDTH, NF = "NsThreeScaleGNN", 128, 3
END_TO_END = []          # (case, partitioned (mean, p99.9, max), single-rank (mean, p99.9, max))


@pytest.fixture(autouse=True)
def _inference():
    with torch.no_grad():
        yield


@pytest.fixture(scope="module", autouse=True)
def _report():
    del R.STATS[:]
    del END_TO_END[:]
    yield
    path = os.environ.get("G4C_PARTITION_REF_REPORT")
    if not path:
        return
    worst = {}
    for what, cls, mx, mean, rmax, rmean in R.STATS:
        if what.endswith("CONTROL"):          # (the negative controls: rejected on purpose)
            continue
        case, out = what.split(" | ")
        key = (case, out.split(" ", 2)[2], cls)          # "<position> <module> <stage>.<name>" -> "<stage>.<name>"
        w = worst.setdefault(key, [0.0, 0.0, 0.0, 0.0, 0])
        worst[key] = [max(w[0], mx), max(w[1], mean), max(w[2], rmax), max(w[3], rmean), w[4] + 1]
    with open(path, "w") as f:
        f.write("(b) stage accuracy: per case, output and row class, the worst over the stages of that kind\n\n")
        f.write("| case | output | row class | stages | max err | mean err | max / allowed | mean / allowed |\n|---|---|---|---|---|---|---|---|\n")
        for (case, out, cls), (mx, mean, rmax, rmean, n) in worst.items():
            f.write(f"| {case} | {out} | {cls} | {n} | {mx:.2e} | {mean:.2e} | {rmax:.3f} | {rmean:.3f} |\n")
        f.write("\n(c) end to end against the fp64 oracle forward: partitioned / single-rank HIP forward (allowed: 1.15 for mean and p99.9)\n\n")
        f.write("| case | mean | p99.9 | max | single mean | single p99.9 | single max | mean ratio | p99.9 ratio |\n|---|---|---|---|---|---|---|---|---|\n")
        for case, p, s in END_TO_END:
            f.write(f"| {case} | {p[0]:.3e} | {p[1]:.3e} | {p[2]:.3e} | {s[0]:.3e} | {s[1]:.3e} | {s[2]:.3e} | {p[0] / s[0]:.3f} | {p[1] / s[1]:.3f} |\n")


@contextlib.contextmanager
def settings(prec="f16x3", hoist=None, overlap="1"):
    old_p, old_h, old_o = ops.set_mlp_precision(prec), B.HOIST_MIN_ROWS, os.environ.get("G4C_DIST_OVERLAP")
    if hoist is not None:
        B.HOIST_MIN_ROWS = hoist
    os.environ["G4C_DIST_OVERLAP"] = overlap
    try:
        yield
    finally:
        ops.set_mlp_precision(old_p)
        B.HOIST_MIN_ROWS = old_h
        if old_o is None:
            del os.environ["G4C_DIST_OVERLAP"]
        else:
            os.environ["G4C_DIST_OVERLAP"] = old_o


def two_clouds(n: int, seed: int) -> Graph:
    """S.mus_graph's recipe on two well-separated clouds, one third of the points in x < 0.3 and two thirds in x > 0.7 (y in
    [0, 0.5]: x is the longer axis): neither a kNN edge nor a grid cell spans the gap, and the first bisection of a 3-rank partition
    (weights 1 : 2) cuts through it."""
    gen = torch.Generator().manual_seed(seed)
    pos = torch.rand(n, 2, generator=gen) * torch.tensor([0.3, 0.5])
    pos[n // 3:, 0] += 0.7
    g = Graph(pos=pos)
    g.edge_index, ea = S.connect_knn(pos, 6)
    g.edge_attr = S.true_divide_by(ea, 4.0 * float(n) ** -0.5)
    S.add_grid_levels(g, S.default_cells(n, 2, 3))
    g.field = torch.randn(n, NF, generator=gen)
    g.glob = torch.rand(n, 1, generator=gen)
    g.omega = (torch.rand(n, 1, generator=gen) > 0.9).float()
    return g


def _mus_bundle(g, model):
    w = {k: v.detach() for k, v in model.state_dict().items()}
    edges = {l + 1: torch.from_numpy(e).to(DEV) for l, e in enumerate(P.coarse_topology(g, 3))}
    gd = g.to_dict()
    b = SimpleNamespace(g=g, model=model, edges=edges, g64=PRf.cast(gd, F64, DEV), g32=PRf.cast(gd, F32, DEV),
                        w64=PRf.cast(w, F64, DEV), w32=PRf.cast(w, F32, DEV), single={}, runs={})
    b.oracle = O.mus_forward(MUS, b.g64, b.w64, NF)
    return b


@pytest.fixture(scope="module")
def mus_model():
    torch.manual_seed(32)
    return getattr(gfd.nn, MUS)(arch=S.mus_arch(MUS, WIDTH), device=DEV)


@pytest.fixture(scope="module")
def mus(mus_model):
    return _mus_bundle(S.mus_graph(3000, levels=3, seed=31), mus_model)


@pytest.fixture(scope="module")
def clouds(mus_model):
    return _mus_bundle(two_clouds(3000, 33), mus_model)


@pytest.fixture(scope="module")
def remus():
    g = S.remus_graph(6000, k=5, seed=51)
    torch.manual_seed(52)
    model = gfd.nn.NsRotEquiTreeScaleGNN(arch=S.remus_arch(WIDTH), device=DEV)
    w = {k: v.detach() for k, v in model.state_dict().items()}
    gd = g.to_dict()
    b = SimpleNamespace(g=g, model=model, g64=PRf.cast(gd, F64, DEV), g32=PRf.cast(gd, F32, DEV), w64=PRf.cast(w, F64, DEV),
                        w32=PRf.cast(w, F32, DEV), runs={})
    b.oracle = O.remus_forward(b.g64, b.w64)
    with settings():
        b.single = model.forward(g.clone().to(DEV))
    return b


# ------------------------------------------------------------------------------------- running a case
def mus_run(b, world, prec="f16x3", hoist=0, overlap="1", **controls):
    """One partitioned forward of every rank; cached per case (the negative controls on the transport are not)."""
    key = (world, prec, hoist, overlap)
    if not controls and key in b.runs:
        return b.runs[key]
    parts = P.build_partition(b.g, 3, world)
    hoist_rows = H.straddling_threshold(parts) if hoist == "straddle" else hoist
    maps = H.MusMaps(parts)
    tr = H.Transport(world, maps, **controls)
    with settings(prec, hoist_rows, overlap):
        make = H.mus_factory(b.g, b.model._PROGRAM, parts, DEV, lambda r, mesh: H.RecordingHipImpl(b.model), WIDTH, NF)
        fwds, preds = H.run_ranks(world, make, tr, DEV)
        torch.cuda.synchronize()
        if (prec, hoist_rows) not in b.single:
            b.single[(prec, hoist_rows)] = b.model.forward(b.g.clone().to(DEV))
    impls = [f.impl for f in fwds]
    prog = b.model._PROGRAM
    had = {k: impls[0].rec[(k, "mp")]["had_products"] for k, n in enumerate(prog) if n.startswith("mp")}
    res = SimpleNamespace(case=f"MuS world {world} {prec} hoist {hoist} overlap {overlap}", world=world, parts=parts, maps=maps, tr=tr, fwds=fwds,
                          impls=impls, preds=preds, had=had, hoists=hoist_rows is not None and hoist_rows <= min(P.uniform_edge_counts(parts)),
                          overlap=overlap == "1", single=b.single[(prec, hoist_rows)], hoist_rows=hoist_rows)
    if not controls:
        b.runs[key] = res
    return res


def expected_mus_kinds(prog, hoists_at):
    """(level, kind) of every exchange the program implies: one before every MP layer; products when the stage before it is a node
    launch on the same level (encode, MP, up) and the layer hoists."""
    out, level = [], 1
    for k, name in enumerate(prog):
        if name.startswith("down_mp"):
            level += 1
        elif name.startswith("up_mp"):
            level -= 1
        else:
            node_launch_before = k == 0 or not prog[k - 1].startswith("down_mp")
            out.append((level, "prod" if (node_launch_before and hoists_at(level)) else "v"))
    return out


def finite_outputs(impls):
    bad = []
    for r, im in enumerate(impls):
        for key, ent in im.rec.items():
            for name, t in ent.items():
                if torch.is_tensor(t) and t.is_floating_point() and name not in ("v_in_halo", "prod_r_halo") and not bool(torch.isfinite(t).all()):
                    bad.append((r, key, name))
    return bad


def check_a_mus(b, res, need_halo=True):
    tr, prog = res.tr, b.model._PROGRAM
    if need_halo:
        assert all(min(f.mesh.n_halo) > 0 for f in res.fwds), [f.mesh.n_halo for f in res.fwds]
    bad = tr.halo_mismatches()
    assert not bad, f"halo rows that are not their owner's rows after (rank, exchange, level) {bad[:6]}"
    assert finite_outputs(res.impls) == []
    uni = P.uniform_edge_counts(res.parts)
    threshold = B.HOIST_MIN_ROWS if res.hoist_rows is None else res.hoist_rows
    expect = expected_mus_kinds(prog, lambda lvl: uni[lvl - 1] >= threshold)
    for r in range(res.world):
        assert tr.kinds(r) == expect, f"rank {r} exchanged {tr.kinds(r)}, the program implies {expect}"
        im = res.impls[r]
        for key, ent in im.rec.items():
            if ent.get("asked_prod"):
                assert "prod_r" in ent, f"rank {r}, {key}: the node launch was asked for the next layer's products and fell back"
        for k, h in res.had.items():
            ent = im.rec[(k, "mp")]
            assert ent["had_products"] == h
            if h:        # the latents' halo rows were never exchanged and never read: still the poison
                assert bool(torch.isnan(ent["v_in_halo"]).all()), f"rank {r}, layer {prog[k]}: latents' halo rows were written"
                assert ent["overlapped"] == res.overlap
    side = {e["on_side_stream"] for e in tr.log if e["kind"] == "prod"}
    assert side <= {res.overlap}, "product exchanges run on the side stream exactly when the overlap is on"


def halo_classes(mask: np.ndarray):
    m = torch.from_numpy(mask).to(DEV)
    return {"halo sender": m, "no halo sender": ~m}


def mus_classes(maps, prog, pos, stage, level, name):
    if stage == "mp":
        return halo_classes(maps.boundary("edge" if name == "e" else "node", level))
    if stage == "down" and name == "e_pool":
        return halo_classes(maps.boundary("edge", level))
    return None


def check_b_mus(b, res):
    prog = b.model._PROGRAM
    rec = H.assemble_mus(res.maps, prog, res.impls)
    ref = PRf.mus_stages(MUS, b.g64, b.w64, PRf.cast_rec(rec, F64, DEV), NF, b.edges, res.had)
    cmp = PRf.mus_stages(MUS, b.g32, b.w32, PRf.cast_rec(rec, F32, DEV), NF, b.edges, res.had)
    assert set(ref) == set(rec)
    failures = []
    levels = H.mus_level_of(prog)
    for pos, stage in rec:
        level = levels[pos][1]
        assert set(ref[(pos, stage)]) == set(rec[(pos, stage)]), (pos, stage)
        module = prog[pos] if 0 <= pos < len(prog) else stage
        for name, got in rec[(pos, stage)].items():
            try:
                R.assert_as_accurate_as_fp32(got, ref[(pos, stage)][name], cmp[(pos, stage)][name],
                                             mus_classes(res.maps, prog, pos, stage, level, name), f"{res.case} | {pos} {module} {stage}.{name}")
            except AssertionError as exc:
                failures.append(str(exc))
    assert not failures, "\n".join(failures)
    return rec


def check_c(case, pred, oracle, single):
    p, s = PRf.error_triple(pred, oracle), PRf.error_triple(single, oracle)
    END_TO_END.append((case, p, s))
    print(f"{case}: partitioned mean {p[0]:.3e} ({p[0] / s[0]:.3f}x) p99.9 {p[1]:.3e} ({p[1] / s[1]:.3f}x) max {p[2]:.3e} | "
          f"single rank mean {s[0]:.3e} p99.9 {s[1]:.3e} max {s[2]:.3e}")
    assert p[0] <= 1.15 * s[0] and p[1] <= 1.15 * s[1], (case, p, s)


MUS_CASES = [(2, "f16x3", 0, "1"), (3, "f16x3", 0, "1"), (4, "f16x3", 0, "1"), (3, "f16x3", 0, "0"), (3, "f16x3", None, "1"),
             (3, "f16x3", "straddle", "1"), (2, "bf16x6", 0, "1")]


@pytest.mark.parametrize("world,prec,hoist,overlap", MUS_CASES, ids=lambda v: str(v))
def test_mus_partitioned_step(mus, world, prec, hoist, overlap):
    res = mus_run(mus, world, prec, hoist, overlap)
    if hoist == "straddle":
        counts = [int(p[0].edge_index.shape[1]) for p in res.parts]
        assert min(counts) < res.hoist_rows <= max(counts) and not res.hoists
        assert all(f.mesh.decision_edges == P.uniform_edge_counts(res.parts) for f in res.fwds)
    assert res.hoists == (hoist == 0) and any(res.had.values()) == res.hoists
    check_a_mus(mus, res)
    rec = check_b_mus(mus, res)
    check_c(res.case, rec[(len(mus.model._PROGRAM), "decode")]["pred"], mus.oracle, res.single)


def test_mus_rank_with_an_empty_halo_enters_every_exchange(clouds):
    res = mus_run(clouds, 3, "f16x3", 0, "1")
    res.case = "MuS two clouds world 3 f16x3 hoist 0 overlap 1"
    assert res.fwds[0].mesh.n_halo == [0, 0, 0] and all(sum(c) == 0 for c in res.fwds[0].mesh.send_counts)
    assert all(min(f.mesh.n_halo) > 0 for f in res.fwds[1:])
    mine = res.tr.of_rank(0)
    assert len(mine) == len(res.tr.of_rank(1)) == 16 and all(e["rows"] == 0 for e in mine)          # zero-length splits, every exchange
    assert all(e["rows"] > 0 for e in res.tr.of_rank(1))
    check_a_mus(clouds, res, need_halo=False)
    rec = check_b_mus(clouds, res)
    check_c(res.case, rec[(len(clouds.model._PROGRAM), "decode")]["pred"], clouds.oracle, res.single)


def test_mus_overlap_on_equals_overlap_off(mus):
    """(d): every edge row is independent and out_idx32 only places it."""
    on, off = mus_run(mus, 3, "f16x3", 0, "1"), mus_run(mus, 3, "f16x3", 0, "0")
    n = 0
    for r in range(3):
        assert torch.equal(on.preds[r], off.preds[r])
        for k, h in on.had.items():
            a, c = on.impls[r].rec[(k, "mp")], off.impls[r].rec[(k, "mp")]
            assert torch.equal(a["e"], c["e"]) and torch.equal(a["v"], c["v"]), (r, k)
            n += a["overlapped"] and not c["overlapped"]
    assert n > 0


# ------------------------------------------------------------------------------------- (e) negative controls
def test_control_stale_halo_on_the_coarsest_level_is_rejected(mus):
    res = mus_run(mus, 3, "f16x3", 0, "1", stale=(3, 1))
    assert res.tr.stale_served > 0 and finite_outputs(res.impls) == []       # plausible values: nothing else would notice
    with pytest.raises(AssertionError, match="not their owner's rows"):
        check_a_mus(mus, res)
    assert {lvl for _, _, lvl in res.tr.halo_mismatches()} == {3}


def test_control_swapped_peers_are_rejected(mus):
    res = mus_run(mus, 3, "f16x3", 0, "1", swap_peers=1)
    assert res.tr.swapped and min(n for *_, n in res.tr.swapped) > 0, "a world-3 case in which a rank has two peers at level 1"
    with pytest.raises(AssertionError, match="not their owner's rows"):
        check_a_mus(mus, res)
    assert {r for r, *_ in res.tr.swapped} <= {r for r, _, _ in res.tr.halo_mismatches()}


@pytest.mark.parametrize("hoist", [0, None], ids=["products", "latents"])
def test_control_wrong_boundary_sender_is_rejected(mus, hoist):
    """The reference (and its fp32 comparator) of ONE MP layer in which one boundary edge takes the next boundary edge's sender."""
    res = mus_run(mus, 3, "f16x3", hoist, "1")
    prog = mus.model._PROGRAM
    rec = H.assemble_mus(res.maps, prog, res.impls)
    k = 1          # mp112: level 1, behind an MP layer
    assert res.had[k] == (hoist == 0)
    bnd = torch.from_numpy(np.nonzero(res.maps.boundary("edge", 1))[0]).to(DEV)
    classes = halo_classes(res.maps.boundary("edge", 1))
    got = rec[(k, "mp")]["e"]
    for wrong in (False, True):
        edges = dict(mus.edges)
        if wrong:
            edges[1], eid = PRf.wrong_boundary_sender(mus.edges[1], bnd)
            assert int(edges[1].max()) < 3000 and int((edges[1] != mus.edges[1]).sum()) == 1
        ref = PRf.mus_stages(MUS, mus.g64, mus.w64, PRf.cast_rec(rec, F64, DEV), NF, edges, res.had, only=[k], check_topology=False)[(k, "mp")]["e"]
        cmp = PRf.mus_stages(MUS, mus.g32, mus.w32, PRf.cast_rec(rec, F32, DEV), NF, edges, res.had, only=[k], check_topology=False)[(k, "mp")]["e"]
        assert R.rejects(R.assert_as_accurate_as_fp32, got, ref, cmp, classes, f"{res.case} | {k} {prog[k]} mp.e CONTROL") == wrong


def test_control_unsorted_coarse_edge_order_is_rejected(mus):
    """The reference (and its comparator) of the pooled coarse e with every rank's rows in the partition table's order instead of the
    target-sorted order LocalMesh stores them in."""
    res = mus_run(mus, 3, "f16x3", 0, "1")
    prog = mus.model._PROGRAM
    rec = H.assemble_mus(res.maps, prog, res.impls)
    k = prog.index("down_mp12")
    got = rec[(k, "down")]["e_pool"]
    ids = lambda s: [torch.from_numpy(res.maps.ids("edge", 2, r, sorted_coarse=s)) for r in range(3)]      # noqa: E731
    assert any(not torch.equal(a, c) for a, c in zip(ids(True), ids(False))), "the sort moves something"
    ref = PRf.mus_stages(MUS, mus.g64, mus.w64, PRf.cast_rec(rec, F64, DEV), NF, mus.edges, res.had, only=[k])[(k, "down")]["e_pool"]
    cmp = PRf.mus_stages(MUS, mus.g32, mus.w32, PRf.cast_rec(rec, F32, DEV), NF, mus.edges, res.had, only=[k])[(k, "down")]["e_pool"]
    classes = halo_classes(res.maps.boundary("edge", 2))
    what = f"{res.case} | {k} down_mp12 down.e_pool CONTROL"
    assert not R.rejects(R.assert_as_accurate_as_fp32, got, ref, cmp, classes, what)
    assert R.rejects(R.assert_as_accurate_as_fp32, got, PRf.rows_moved(ref, ids(True), ids(False)), PRf.rows_moved(cmp, ids(True), ids(False)), classes, what)


# ------------------------------------------------------------------------------------- REMuS-GNN
def remus_run(b, world):
    if world in b.runs:
        return b.runs[world]
    parts = PR.build_remus_partition(b.g, world)
    maps = H.RemusMaps(parts)
    tr = H.Transport(world, maps)
    with settings():
        fwds, preds = H.run_ranks(world, H.remus_factory(b.g, b.model._PROGRAM, parts, DEV, lambda r, mesh: H.RecordingRemusHipImpl(b.model, mesh)), tr, DEV)
        torch.cuda.synchronize()
    b.runs[world] = SimpleNamespace(case=f"REMuS world {world} f16x3", world=world, parts=parts, maps=maps, tr=tr, fwds=fwds,
                                    impls=[f.impl for f in fwds], preds=preds)
    return b.runs[world]


def remus_classes(maps, op, lvl, stage, name):
    if stage == "mp":
        return halo_classes(maps.boundary("angle" if name == "a" else "edge", lvl))
    if stage == "down":
        return halo_classes(maps.boundary("down_edge", lvl))
    if stage == "up":
        return halo_classes(maps.boundary("up_edge", lvl - 1))
    return None


@pytest.mark.parametrize("world", [2, 3])
def test_remus_partitioned_step(remus, world):
    res = remus_run(remus, world)
    prog = remus.model._PROGRAM
    # (a)
    assert all(min(f.mesh.n_halo) > 0 for f in res.fwds), [f.mesh.n_halo for f in res.fwds]
    bad = res.tr.halo_mismatches()
    assert not bad, f"halo rows that are not their owner's rows after (rank, exchange, channel) {bad[:6]}"
    assert finite_outputs(res.impls) == [], "a stage read a halo row that was not exchanged since its buffer was written"
    expect = []
    for op, _, lvl in prog:
        expect.append((lvl if op != "up" else PR.CH_NODE[lvl], "v"))
    for r in range(world):
        # every EdgeMP / DownEdgeMP exchanges its level's edge latents (the launch before it wrote them), every UpEdgeMP the node vectors
        assert res.tr.kinds(r) == expect and len(expect) == 16 + 2 + 2, res.tr.kinds(r)
    # (b)
    rec = H.assemble_remus(res.maps, prog, res.impls)
    assert all(t.dtype == F32 for ent in rec.values() for t in ent.values())
    ref = PRf.remus_stages(remus.g64, remus.w64, PRf.cast_rec(rec, F64, DEV), prog)
    cmp = PRf.remus_stages(remus.g32, remus.w32, PRf.cast_rec(rec, F32, DEV), prog)
    assert set(ref) == set(rec)
    failures = []
    for (pos, stage), ent in rec.items():
        assert set(ref[(pos, stage)]) == set(ent), (pos, stage)
        op, module, lvl = prog[pos] if 0 <= pos < len(prog) else (stage, stage, 1)
        for name, got in ent.items():
            try:
                R.assert_as_accurate_as_fp32(got, ref[(pos, stage)][name], cmp[(pos, stage)][name], remus_classes(res.maps, op, lvl, stage, name),
                                             f"{res.case} | {pos} {module} {stage}.{name}")
            except AssertionError as exc:
                failures.append(str(exc))
    assert not failures, "\n".join(failures)
    # (c)
    check_c(res.case, rec[(len(prog), "decode")]["pred"], remus.oracle, remus.single[:, :2])
