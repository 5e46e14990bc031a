"""tests/partition_harness.py and oracle/partition_ref.py without a GPU: the in-process runner, the lock-step collective under the
real HaloExchanger, the recording mix-ins and the local-to-global maps, run over the oracle back-ends of tests/test_partition.py on
CPU tensors in float64.  Every assembled stage tensor equals the whole-mesh restatement of its stage to 1e-10 (relative to the
tensor's largest magnitude) at world 2, 3 and 4, with latents and with first-layer products in the halo; after every exchange the halo
rows are their owners' rows bit for bit; both transport controls (a halo one exchange old, two peers' slices swapped) break exactly
that; and the decisions on WHAT an exchange carries are the same on every rank when they are taken on `uniform_edge_counts` — the
counts DistributedRollout installs — for a mesh whose ranks' own counts lie on opposite sides of the hoisting threshold."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import graphs4cfd_amd as gfd                                                   # noqa: E402
import partition_harness as H                                                  # noqa: E402
from graphs4cfd_amd import partition as P, partition_remus as PR, synthetic as S   # noqa: E402
from graphs4cfd_amd.graph import Graph                                         # noqa: E402
from graphs4cfd_amd.nn import blocks as B                                      # noqa: E402
from oracle import g4c_oracle as O, partition_ref as PRf                       # noqa: E402
from test_partition import OracleImpl, RemusOracleImpl                         # noqa: E402

F64 = torch.float64
CPU = torch.device("cpu")
MUS = "NsThreeScaleGNN"


class RecOracle(H.MusRecorder, OracleImpl):
    pass


class RecRemusOracle(H.RemusRecorder, RemusOracleImpl):
    pass


class RecOracleDecidingLikeHip(H.MusRecorder, OracleImpl):
    """The oracle back-end with HipImpl's own decision on hoisting (edge count against blocks.HOIST_MIN_ROWS)."""

    def __init__(self, w, **kw):
        super().__init__(w, True, **kw)

    def hoists(self, n_edges):
        return P.HipImpl.hoists(self, n_edges)


@pytest.fixture(autouse=True)
def _float64_default():
    """The oracle back-ends allocate with the default dtype."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(F64)
    yield
    torch.set_default_dtype(old)


def f64(g: Graph) -> Graph:
    return Graph(**{k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in g.to_dict().items()})


def close(got, ref, what):
    assert tuple(got.shape) == tuple(ref.shape), (what, tuple(got.shape), tuple(ref.shape))
    err = float((got - ref).abs().max()) if got.numel() else 0.0
    assert torch.isfinite(got).all() and err <= 1e-10 * max(1.0, float(ref.abs().max())), f"{what}: {err:.3e}"


@pytest.fixture(scope="module")
def mus():
    g = f64(S.mus_graph(1500, levels=3, seed=5))
    torch.manual_seed(11)
    model = getattr(gfd.nn, MUS)(arch=S.mus_arch(MUS, 32))          # CPU: parameters only, never run
    w = {k: v.detach().double() for k, v in model.state_dict().items()}
    edges = {l + 1: torch.from_numpy(e) for l, e in enumerate(P.coarse_topology(g, 3))}
    return g, model, w, edges


@pytest.fixture(scope="module")
def remus():
    torch.manual_seed(0)
    g = f64(S.remus_graph(1200, k=5, seed=7))
    model = gfd.nn.NsRotEquiTreeScaleGNN(arch=S.remus_arch(32))
    return g, model, {k: v.detach().double() for k, v in model.state_dict().items()}


def run_mus(mus, world, use_products, **controls):
    g, model, w, edges = mus
    parts = P.build_partition(g, 3, world)
    maps = H.MusMaps(parts)
    tr = H.Transport(world, maps, **controls)
    make = H.mus_factory(g, model._PROGRAM, parts, CPU, lambda r, mesh: RecOracle(w, use_products, rec_dtype=F64), 32, 3)
    fwds, preds = H.run_ranks(world, make, tr)
    return parts, maps, tr, fwds, preds


@pytest.mark.parametrize("use_products", [False, True], ids=["latents", "products"])
@pytest.mark.parametrize("world", [2, 3, 4])
def test_mus_harness_equals_the_whole_mesh_oracle(mus, world, use_products):
    g, model, w, edges = mus
    parts, maps, tr, fwds, preds = run_mus(mus, world, use_products)
    impls = [f.impl for f in fwds]
    assert all(min(f.mesh.n_halo) > 0 for f in fwds)
    # after every exchange the halo rows are the owners' rows; every rank exchanged the same kinds at the same levels
    assert tr.halo_mismatches() == [] and len(tr.log) == world * len(tr.of_rank(0)) > 0
    assert all(tr.kinds(r) == tr.kinds(0) for r in range(world))
    assert ("prod" in {k for _, k in tr.kinds(0)}) == use_products and "?" not in {k for _, k in tr.kinds(0)}
    had = {k: impls[0].rec[(k, "mp")]["had_products"] for k, n in enumerate(model._PROGRAM) if n.startswith("mp")}
    assert all(im.rec[(k, "mp")]["had_products"] == h for im in impls for k, h in had.items()) and any(had.values()) == use_products
    for im in impls:        # a layer that took products never read the latents' halo rows: they still hold the poison
        for k, h in had.items():
            assert not h or bool(torch.isnan(im.rec[(k, "mp")]["v_in_halo"]).all())
    rec = H.assemble_mus(maps, model._PROGRAM, impls)
    ref = PRf.mus_stages(MUS, g.to_dict(), w, rec, 3, edges, had)
    assert set(ref) == set(rec)
    n = 0
    for key in rec:
        assert set(ref[key]) == set(rec[key]), key
        for name in rec[key]:
            close(rec[key][name], ref[key][name], (key, name))
            n += 1
    assert n >= 2 * len(model._PROGRAM)
    with torch.no_grad():
        close(rec[(len(model._PROGRAM), "decode")]["pred"], O.mus_forward(MUS, g.to_dict(), w, 3), "prediction, end to end")


@pytest.mark.parametrize("world", [2, 3, 4])
def test_remus_harness_equals_the_whole_mesh_oracle(remus, world):
    g, model, w = remus
    parts = PR.build_remus_partition(g, world)
    maps = H.RemusMaps(parts)
    tr = H.Transport(world, maps)
    fwds, preds = H.run_ranks(world, H.remus_factory(g, model._PROGRAM, parts, CPU, lambda r, mesh: RecRemusOracle(w, mesh)), tr)
    assert all(max(f.mesh.n_halo[c] for f in fwds) > 0 for c in range(5)) and (world > 3 or all(min(f.mesh.n_halo) > 0 for f in fwds))
    assert tr.halo_mismatches() == [] and len(tr.of_rank(0)) == 16 + 2 + 2 and {e["level"] for e in tr.log} == {1, 2, 3, 4, 5}
    rec = H.assemble_remus(maps, model._PROGRAM, [f.impl for f in fwds])
    ref = PRf.remus_stages(g.to_dict(), w, rec, model._PROGRAM, raw_angles=False)
    assert set(ref) == set(rec)
    for key in rec:
        assert set(ref[key]) == set(rec[key]), key
        for name in rec[key]:
            close(rec[key][name], ref[key][name], (key, name))
    with torch.no_grad():
        close(rec[(len(model._PROGRAM), "decode")]["pred"], O.remus_forward(g.to_dict(), w), "prediction, end to end")


def test_maps_reject_rows_written_twice(mus):
    g = mus[0]
    parts = P.build_partition(g, 3, 2)
    maps = H.MusMaps(parts)
    rows = [torch.zeros(p[0].n_own, 2) for p in parts]
    maps.assemble("node", 1, rows)
    with pytest.raises(AssertionError, match="exactly once"):
        twice = np.resize(parts[0][0].owned, parts[1][0].n_own)         # rank 1's rows under rank 0's global ids
        H._assemble([parts[0][0].owned, twice], int(g.pos.size(0)), rows)


@pytest.mark.parametrize("use_products", [False, True], ids=["latents", "products"])
def test_transport_controls_break_the_halo_equality(mus, use_products):
    """A halo of the coarsest level one exchange old, and two peers' slices delivered in each other's place (world 3)."""
    *_, tr, _, _ = run_mus(mus, 3, use_products, stale=(3, 1))
    bad = tr.halo_mismatches()
    assert tr.stale_served > 0 and bad and {lvl for _, _, lvl in bad} == {3}
    *_, tr, _, _ = run_mus(mus, 3, use_products, swap_peers=1)
    bad = tr.halo_mismatches()
    assert tr.swapped and min(n for *_, n in tr.swapped) > 0, "a world-3 case in which a rank has two peers at level 1"
    assert {r for r, *_ in tr.swapped} <= {r for r, _, _ in bad} and {lvl for _, _, lvl in bad} == {1}


def test_remus_transport_stale_control_breaks_the_halo_equality(remus):
    g, model, w = remus
    parts = PR.build_remus_partition(g, 3)
    tr = H.Transport(3, H.RemusMaps(parts), stale=(3, 1))
    H.run_ranks(3, H.remus_factory(g, model._PROGRAM, parts, CPU, lambda r, mesh: RecRemusOracle(w, mesh)), tr)
    assert tr.stale_served > 0 and {lvl for _, _, lvl in tr.halo_mismatches()} == {3}


def test_a_failing_rank_is_reported_and_a_missed_rendezvous_times_out(mus):
    g, model, w, edges = mus
    parts = P.build_partition(g, 3, 2)

    class Failing(RecOracle):
        def down(self, *a, **k):
            raise RuntimeError("rank-local failure")

    def make_impl(r, mesh):
        return (Failing if r == 1 else RecOracle)(w, False, rec_dtype=F64)
    with pytest.raises(AssertionError, match="rank 1 failed: RuntimeError: rank-local failure"):
        H.run_ranks(2, H.mus_factory(g, model._PROGRAM, parts, CPU, make_impl, 32, 3), H.Transport(2, H.MusMaps(parts)))

    class Absent(RecOracle):          # rank 1 leaves before its second exchange: rank 0 must not wait for ever
        def mp(self, name, *a, **k):
            if name == "mp112":
                raise SystemExit
            return super().mp(name, *a, **k)

    tr = H.Transport(2, H.MusMaps(parts), timeout=0.2)
    tr.barrier.abort = lambda: None        # (the leaving rank tells nobody)
    with pytest.raises(AssertionError, match="failed"):
        H.run_ranks(2, H.mus_factory(g, model._PROGRAM, parts, CPU, lambda r, mesh: (Absent if r == 1 else RecOracle)(w, False, rec_dtype=F64), 32, 3), tr)


def test_exchange_kinds_are_rank_uniform_across_the_hoisting_threshold(mus, monkeypatch):
    """Ranks whose level-1 edge counts lie on opposite sides of HOIST_MIN_ROWS: decided on the local counts, one rank sends
    first-layer products where its peer expects latents; decided on uniform_edge_counts — what DistributedRollout installs — every
    rank exchanges the same kind at every exchange."""
    g, model, w, edges = mus
    world = 3
    parts = P.build_partition(g, 3, world)
    counts = [int(p[0].edge_index.shape[1]) for p in parts]
    thr = H.straddling_threshold(parts)
    assert min(counts) < thr <= max(counts)
    monkeypatch.setattr(B, "HOIST_MIN_ROWS", thr)
    seq = {}
    for uniform in (True, False):
        tr = H.Transport(world, H.MusMaps(parts))
        make = H.mus_factory(g, model._PROGRAM, parts, CPU, lambda r, mesh: RecOracleDecidingLikeHip(w, rec_dtype=F64), 32, 3, uniform=uniform)
        fwds, _ = H.run_ranks(world, make, tr)
        seq[uniform] = [tr.kinds(r) for r in range(world)]
        assert all("?" not in {k for _, k in s} for s in seq[uniform])
        if uniform:
            assert all(f.mesh.decision_edges == P.uniform_edge_counts(parts) for f in fwds)
    assert all(s == seq[True][0] for s in seq[True]), "uniform counts: one sequence of kinds"
    assert any(s != seq[False][0] for s in seq[False]), "local counts: the ranks disagree (the hazard uniform_edge_counts exists for)"
    # below the threshold with everybody, above with everybody: products appear exactly when the smallest rank hoists
    assert {k for _, k in seq[True][0]} == {"v"}
    monkeypatch.setattr(B, "HOIST_MIN_ROWS", min(counts))
    tr = H.Transport(world, H.MusMaps(parts))
    H.run_ranks(world, H.mus_factory(g, model._PROGRAM, parts, CPU, lambda r, mesh: RecOracleDecidingLikeHip(w, rec_dtype=F64), 32, 3), tr)
    assert all(tr.kinds(r) == tr.kinds(0) for r in range(world)) and (1, "prod") in tr.kinds(0) and tr.halo_mismatches() == []


def test_distributed_rollout_installs_the_uniform_counts(monkeypatch):
    """Constructing only (world 3, CPU device): the mesh of every rank decides on uniform_edge_counts of the whole table."""
    g = S.mus_graph(1500, levels=3, seed=5)
    torch.manual_seed(11)
    model = getattr(gfd.nn, MUS)(arch=S.mus_arch(MUS, 32))
    parts = P.build_partition(g, 3, 3)
    uni = P.uniform_edge_counts(parts)
    for r in range(3):
        dr = P.DistributedRollout(model, g, 2, r, 3, CPU, capture=False)
        local = [int(p.edge_index.shape[1]) for p in parts[r]]
        assert dr.mesh.decision_edges == uni and dr.fwd.mesh is dr.mesh and all(u <= n for u, n in zip(uni, local))
    assert any(uni != [int(p.edge_index.shape[1]) for p in parts[r]] for r in range(3))
