"""Host-side logic that needs no GPU: the C-ABI library loads and exports every symbol the header declares,
the static-plan builders (host C++) agree with the oracle's topology, the gfd-compatible module surface
(state_dict keys, checkpoint format, Graph container, error behaviour)."""
import os
import re

import numpy as np
import pytest
import torch

import graphs4cfd_amd as gfd
from graphs4cfd_amd import _lib, plan, synthetic as S
from oracle import g4c_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    header = open(os.path.join(ROOT, "include", "g4c.h")).read()
    declared = set(re.findall(r"\b(g4c_[a-z0-9_]+)\s*\(", header))
    assert declared, "no declarations parsed"
    lib = _lib.load()
    for name in sorted(declared):
        assert hasattr(lib, name), f"libg4c.so does not export {name}"
    assert declared == set(_lib.EXPORTED_SYMBOLS), (declared ^ set(_lib.EXPORTED_SYMBOLS))
    assert lib.g4c_version() >= 1


def test_mlp_run_validates_its_descriptor_before_any_hip_call():
    """g4c_mlp_run checks g4c_mlp_io_t.size first (a binding out of step with g4c.h gets G4C_EINVAL, not garbage reads) and the
    launch arguments before it touches the device: both errors come back on a machine without a GPU."""
    import ctypes as C
    lib = _lib.load()
    mlp = _lib.g4c_mlp_t(n_layers=1)
    src = (_lib.g4c_src_t * 1)()
    io = _lib.g4c_mlp_io_t(row_count=64)
    io.size -= 8
    assert lib.g4c_mlp_run(C.byref(mlp), src, 1, 64, C.byref(io), None) == _lib.EINVAL
    assert "size" in lib.g4c_last_error().decode()
    io = _lib.g4c_mlp_io_t(row_count=64, act=7)
    assert lib.g4c_mlp_run(C.byref(mlp), src, 1, 64, C.byref(io), None) == _lib.EINVAL
    assert "bad activation 7" in lib.g4c_last_error().decode()
    # the fp16 range flags a launch writes are named by the launch (io.range_flag), the word by the MLP (range_slot): both checked
    flags = (C.c_int32 * 8)()
    f16 = _lib.g4c_mlp_t(n_layers=1, w_format=_lib.WFMT_F16X2, range_slot=-1)
    io = _lib.g4c_mlp_io_t(row_count=64, range_flag=C.addressof(flags))
    assert lib.g4c_mlp_run(C.byref(f16), src, 1, 64, C.byref(io), None) == _lib.EINVAL
    assert "negative range_slot" in lib.g4c_last_error().decode()
    upd = _lib.g4c_mlp_t(n_layers=1, w_format=_lib.WFMT_F16X2, range_slot=-1)
    f16.range_slot = 0
    io = _lib.g4c_mlp_io_t(row_count=64, range_flag=C.addressof(flags), upd=C.pointer(upd))
    assert lib.g4c_mlp_run(C.byref(f16), src, 1, 64, C.byref(io), None) == _lib.EINVAL
    assert "negative range_slot" in lib.g4c_last_error().decode()
    assert list(flags) == [0] * 8
    assert lib.g4c_version() == 3


def test_plan_csr_matches_stable_argsort():
    rng = np.random.default_rng(0)
    keys = torch.from_numpy(rng.integers(0, 37, size=500))
    p = plan.build_csr(keys, 40, torch.device("cpu"))
    order = torch.sort(keys, stable=True)[1].to(torch.int32)
    assert torch.equal(p.perm, order)
    assert torch.equal(p.off.long(), torch.cat([torch.zeros(1, dtype=torch.long), torch.bincount(keys, minlength=40).cumsum(0)]))
    assert p.max_deg == int(torch.bincount(keys).max())
    # already grouped in order -> no permutation at all
    sorted_keys = torch.arange(50).repeat_interleave(6)
    assert plan.build_csr(sorted_keys, 50, torch.device("cpu")).perm is None
    with pytest.raises(ValueError):
        plan.build_csr(torch.tensor([0, 7]), 5, torch.device("cpu"))


def test_pool_edge_plan_topology_matches_oracle(golden):
    import ctypes as C
    lib = _lib.load()
    for tag in ("mean", "empty"):
        c = golden("blocks.pt")[f"pool_edge_{tag}"]
        idx = np.ascontiguousarray(c["idx"].numpy())
        ei = np.ascontiguousarray(c["edge_index"].numpy())
        n_edges = ei.shape[1]
        coarse = np.empty((2, n_edges), dtype=np.int64)
        perm = np.empty(n_edges, dtype=np.int32)
        off = np.empty(n_edges + 1, dtype=np.int32)
        kept = C.c_int64(0)
        nc = lib.g4c_plan_pool_edge(idx.ctypes.data, idx.shape[0], ei.ctypes.data, n_edges, coarse.ctypes.data,
                                    perm.ctypes.data, off.ctypes.data, C.byref(kept))
        got = torch.from_numpy(coarse.reshape(-1)[: 2 * nc].reshape(2, nc).copy())
        assert torch.equal(got, c["edge_index_out"])
        # the segmented permutation reproduces the reference's mean of duplicate edges
        ea = c["edge_attr"]
        if nc:
            seg = torch.repeat_interleave(torch.arange(nc), torch.from_numpy(np.diff(off[: nc + 1])).long())
            pooled = O.scatter(ea[torch.from_numpy(perm[: kept.value].copy()).long()], seg, nc, "mean")
            torch.testing.assert_close(pooled, c["edge_attr_out"], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("cls", sorted(S.MUS_LAYERS))
def test_state_dict_keys_and_shapes_match_reference(golden, cls):
    c = golden("models_mus.pt")[cls]
    model = getattr(gfd.nn, cls)(arch=c["arch"])
    sd = model.state_dict()
    assert list(sd.keys()) == list(c["weights"].keys())
    assert all(sd[k].shape == v.shape for k, v in c["weights"].items())
    model.load_state_dict(c["weights"])
    assert model.num_params == c["num_params"] and model.num_fields == c["arch"]["decoder"][1][-1]


def test_remus_state_dict_and_seeded_init_match_reference(golden):
    c = golden("model_remus.pt")
    torch.manual_seed(400)           # the seed make_golden.py used: same construction order -> same init
    model = gfd.nn.NsRotEquiTreeScaleGNN(arch=c["arch"])
    assert list(model.state_dict().keys()) == list(c["weights"].keys())
    for k, v in c["weights"].items():
        assert torch.equal(model.state_dict()[k], v), k


def test_checkpoint_round_trip_in_reference_format(golden, tmp_path):
    path = os.path.join(os.path.dirname(__file__), "golden", "reference_saved.chk")
    model = gfd.nn.NsOneScaleGNN(checkpoint=path)      # a file written by the reference's save_checkpoint
    assert list(model.state_dict().keys()) == golden("checkpoint_io.pt")["keys"]
    out = str(tmp_path / "mine.chk")
    model.save_checkpoint(out, n_out=2, epoch=5)
    chk = torch.load(out, weights_only=False)
    assert set(chk) >= {"arch", "weights", "n_out", "epoch"} and chk["arch"] == model.arch
    again = gfd.nn.NsOneScaleGNN(checkpoint=out)
    assert all(torch.equal(a, b) for a, b in zip(again.state_dict().values(), model.state_dict().values()))
    w = str(tmp_path / "weights.pt")
    torch.save(model.state_dict(), w)
    third = gfd.nn.NsOneScaleGNN(arch=model.arch, weights=w)
    assert all(torch.equal(a, b) for a, b in zip(third.state_dict().values(), model.state_dict().values()))


def test_graph_container_and_collate():
    g = gfd.Graph(pos=torch.zeros(5, 2), field=torch.ones(5, 3), edge_index=torch.tensor([[0, 1], [1, 2]]))
    assert g.num_nodes == 5 and g.num_edges == 2 and hasattr(g, "field") and not hasattr(g, "loc")
    g.idx1_to_idx2 = torch.arange(5)
    assert getattr(g, "idx1_to_idx2").numel() == 5 and "idx1_to_idx2" in g.keys()
    assert g.to("cpu") is g
    b = gfd.nn.collate([g.clone(), g.clone()])
    assert b.num_nodes == 10 and b.edge_index.tolist() == [[0, 1, 5, 6], [1, 2, 6, 7]]
    assert b.batch.tolist() == [0] * 5 + [1] * 5


def test_product_path_has_no_cpu_fallback_and_validates():
    mlp = gfd.nn.blocks.MLP(8, (16, 16), True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        mlp(torch.randn(4, 8))
    model = gfd.nn.NsOneScaleGNN(arch=S.mus_arch("NsOneScaleGNN", 32))
    with pytest.raises(AssertionError):
        model.solve(S.mus_graph(50), 0)
    with pytest.raises(ValueError, match="not recognized"):
        gfd.nn.NsTwoScaleGNN(model="nope")
    with pytest.raises(ValueError):
        gfd.nn.blocks.MLP(4, (8,))
    src = open(os.path.join(ROOT, "graphs4cfd_amd", "ops.py")).read() + open(os.path.join(ROOT, "graphs4cfd_amd", "nn", "blocks.py")).read()
    assert "oracle" not in src, "the product path must not import the oracle"


def test_pool_edge_plan_rejects_unassigned_fine_nodes():
    """A -1 entry (the 'empty' value of the reference's mask2idx tables) must be an argument error, not a heap overrun."""
    import ctypes as C
    lib = _lib.load()
    idx = np.array([0, 1, -1, 1], dtype=np.int64)
    ei = np.array([[0, 1, 2], [1, 2, 3]], dtype=np.int64)
    coarse, perm, off = np.empty((2, 3), dtype=np.int64), np.empty(3, dtype=np.int32), np.empty(4, dtype=np.int32)
    kept = C.c_int64(0)
    nc = lib.g4c_plan_pool_edge(idx.ctypes.data, 4, ei.ctypes.data, 3, coarse.ctypes.data, perm.ctypes.data, off.ctypes.data, C.byref(kept))
    assert nc < 0 and b"negative" in lib.g4c_last_error()


def test_plan_caches_are_bounded_by_bytes():
    c = plan._Cache(capacity=100, max_bytes=10_000)
    keep = []
    for i in range(20):
        k = torch.zeros(250, dtype=torch.int32)      # 1000 bytes pinned by the key + 1000 by the value
        keep.append(k)
        c.put(plan._Cache.key(k), (k,), (torch.zeros(250, dtype=torch.int32), 7))
        assert c.bytes <= 10_000 and c.bytes == sum(e[2] for e in c.data.values())
    assert len(c.data) == 5 and c.get(plan._Cache.key(keep[-1])) is not None and c.get(plan._Cache.key(keep[0])) is None
    big = torch.zeros(100_000, dtype=torch.int32)    # larger than the bound: still cached (alone) for the rollout that needs it
    c.put(plan._Cache.key(big), (big,), None)
    assert len(c.data) == 1 and c.get(plan._Cache.key(big)) is None and plan._Cache.key(big) in c.data
    c.clear()
    assert c.bytes == 0 and not c.data
    assert isinstance(plan.snapshot(), list)


def test_connect_knn_keeps_in_degree_k_with_coincident_points():
    torch.manual_seed(0)
    pos = torch.rand(60, 2)
    pos[10:15] = pos[10]            # five coincident points: a k + 1 query need not return the centre itself
    ei, ea = S.connect_knn(pos, 3)
    assert (np.bincount(ei[1].numpy(), minlength=60) == 3).all() and bool((ei[0] != ei[1]).all())
    torch.testing.assert_close(ea, pos[ei[1]] - pos[ei[0]])


def test_reference_package_name_is_an_alias():
    """`import graphs4cfd as gfd` (the examples' import) binds to the same module objects as graphs4cfd_amd."""
    import graphs4cfd as ref_name
    import graphs4cfd.nn.mus_gnn as mus
    from graphs4cfd.transforms import Compose, ConnectKNN, GridClustering, ScaleEdgeAttr
    assert ref_name.nn is gfd.nn and ref_name.Graph is gfd.Graph and ref_name.DataLoader is gfd.DataLoader
    assert mus.NsThreeScaleGNN is gfd.nn.NsThreeScaleGNN and ConnectKNN is gfd.transforms.ConnectKNN
    g = Compose([ConnectKNN(4), ScaleEdgeAttr(0.1), GridClustering([0.2])])(gfd.Graph(pos=torch.rand(200, 2)))
    assert g.edge_index.shape == (2, 800) and hasattr(g, "cluster_2")
    with pytest.raises(ImportError, match="plot"):
        ref_name.plot


def test_invalidate_packed_bumps_the_weights_epoch():
    from graphs4cfd_amd import ops
    model = gfd.nn.NsOneScaleGNN(arch=S.mus_arch("NsOneScaleGNN", 32))
    e0 = ops.weights_epoch()
    model.invalidate_packed()
    e1 = ops.weights_epoch()
    model.load_state_dict(model.state_dict())
    e2 = ops.weights_epoch()
    model.float()
    assert e0 < e1 < e2 < ops.weights_epoch()
    assert not hasattr(model, "_require_inference")


def test_locality_renumbering_keeps_the_mesh():
    """reorder.reorder_nodes: a permutation of the level-1 nodes along a Morton curve; same edges, grouped by the new target with the
    per-target order kept; level-2 maps carried along; layouts it does not know are left alone."""
    from graphs4cfd_amd.reorder import reorder_nodes
    g = S.mus_graph(3000, levels=3, seed=5)
    g2, perm = reorder_nodes(g)
    n = 3000
    assert sorted(perm.tolist()) == list(range(n))
    assert torch.equal(g2.pos, g.pos[perm]) and torch.equal(g2.field, g.field[perm]) and torch.equal(g2.idx1_to_idx2, g.idx1_to_idx2[perm])
    assert torch.equal(g2.e_12, g.e_12[perm]) and g2.pos_2 is g.pos_2 and g2.idx2_to_idx3 is g.idx2_to_idx3
    col = g2.edge_index[1]
    assert bool((col[1:] >= col[:-1]).all()), "edges grouped by the new target"
    old_edges = set(map(tuple, g.edge_index.t().tolist()))
    new_edges = set((int(perm[r]), int(perm[c])) for r, c in g2.edge_index.t().tolist())
    assert old_edges == new_edges
    # per target: the same senders in the same order, with the same attributes
    for tgt_new in (0, 17, n - 1):
        tgt_old = int(perm[tgt_new])
        a = g.edge_index[0][g.edge_index[1] == tgt_old]
        b = perm[g2.edge_index[0][g2.edge_index[1] == tgt_new]]
        assert torch.equal(a, b)
        torch.testing.assert_close(g2.edge_attr[g2.edge_index[1] == tgt_new], g.edge_attr[g.edge_index[1] == tgt_old])
    # neighbours get nearby numbers: mean |row - col| far below a random numbering's n / 3
    assert float((g2.edge_index[0] - g2.edge_index[1]).abs().float().mean()) < 0.1 * float((g.edge_index[0] - g.edge_index[1]).abs().float().mean())
    assert reorder_nodes(S.remus_graph(300, k=5, seed=1)) is None
    g.extra = torch.zeros(7)
    assert reorder_nodes(g) is None


def test_mlp_precision_names_and_f16_range_warning():
    """The arithmetic modes the host accepts, and the input-magnitude hint of the default one: solve() warns when an
    input tensor is large enough for a hidden activation to reach fp16's range (the f16x3 kernels clip there), and only then."""
    import warnings
    from graphs4cfd_amd import ops
    from graphs4cfd_amd.nn import model as M
    assert ops.PRECISIONS == ("fp32", "bf16", "bf16x6", "f16x3") and ops.mlp_precision() in ops.PRECISIONS
    with pytest.raises(ValueError):
        ops.set_mlp_precision("fp16")
    g = S.mus_graph(300, levels=1, seed=3)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        M._warn_f16_range(g)
    g.field = g.field * (2.0 * M.F16_INPUT_WARN / float(g.field.abs().max()))
    with pytest.warns(RuntimeWarning, match="f16x3"):
        M._warn_f16_range(g)


def test_bench_starts_its_own_ranks_when_not_under_torchrun(monkeypatch):
    """`python bench.py --gpus N` (the driver's command shape) must not die in argument checking: outside a
    torch.distributed.run job it launches the N ranks itself, inside one it is a rank."""
    import importlib.util
    import sys
    spec = importlib.util.spec_from_file_location("g4c_bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    assert bench.launcher_needed(2, {}) and bench.launcher_needed(8, {"PATH": "/bin"})
    assert not bench.launcher_needed(1, {})
    assert not bench.launcher_needed(2, {"WORLD_SIZE": "2", "RANK": "0"})
    cmd = bench.launcher_command(4, ["--gpus", "4", "--steps", "3"], 29511)
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nproc-per-node=4" in cmd and "--nnodes=1" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and cmd[cmd.index("--master-port") + 1] == "29511"
    assert cmd[-5:] == [os.path.join(ROOT, "bench.py"), "--gpus", "4", "--steps", "3"]
    # main() takes the launcher branch (and returns the job's return code) before it touches a GPU
    seen = {}

    def fake_launch(gpus, argv):
        seen["gpus"], seen["argv"] = gpus, list(argv)
        return 7
    monkeypatch.setattr(bench, "launch_ranks", fake_launch)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2", "--steps", "2", "--warmup", "1"])
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    with pytest.raises(SystemExit) as exc:
        bench.main()
    assert exc.value.code == 7 and seen == {"gpus": 2, "argv": ["--gpus", "2", "--steps", "2", "--warmup", "1"]}


def test_bench_plain_run_options_and_output_dump(monkeypatch, tmp_path):
    """A plain `bench.py` run leaves the extra measurements to --full; --dump-outputs writes the last timed step's block of the
    caller's [N, nf * steps] result (float32), and a fixed, seeded sample of its rows when the whole block is over the limit."""
    import importlib.util
    import sys
    spec = importlib.util.spec_from_file_location("g4c_bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", str(tmp_path)])
    a = bench.parse()
    assert a.full and a.dump_outputs == str(tmp_path)

    class FakeRollout:
        nf, steps_done = 3, 4

        def __init__(self, n):
            self.res = torch.arange(n * self.nf * 5, dtype=torch.float32).reshape(n, self.nf * 5)

        def result(self):
            return self.res
    ro = FakeRollout(50)
    bench.dump_outputs(str(tmp_path / "all"), ro, 1, 0)
    got = np.load(tmp_path / "all" / "last_step_prediction.npy")
    assert got.dtype == np.float32 and np.array_equal(got, ro.res[:, 9:12].numpy())
    assert not (tmp_path / "all" / "last_step_prediction_rows.npy").exists()
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 20 * (4 * 3 + 8))
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), ro, 1, 0)
    rows = np.load(tmp_path / "s1" / "last_step_prediction_rows.npy")
    assert rows.dtype == np.float64 and len(rows) == 20 and np.all(np.diff(rows) > 0)
    assert np.array_equal(rows, np.load(tmp_path / "s2" / "last_step_prediction_rows.npy"))
    assert np.array_equal(np.load(tmp_path / "s1" / "last_step_prediction.npy"), ro.res[rows.astype(np.int64), 9:12].numpy())


def test_range_flags_belong_to_the_consumer_that_issued_the_launch(monkeypatch):
    """ops.RangeFlags / ops._run (host logic: the flag buffers stand on the CPU, and a stand-in for g4c_mlp_run writes 1 into
    io.range_flag[range_slot] — and [upd.range_slot] — as a clipping f16x3 kernel does): a launch issued inside a consumer's scope
    reports into that consumer's buffer (the innermost scope on the launch's device wins), one outside any scope into the device's
    default buffer.  take() answers once, also after the consumer has left its scope; f16_range_report / check_f16_range read the
    default buffer only, and a consumer never sees what was launched outside it."""
    import ctypes as C
    import types
    import warnings
    from graphs4cfd_amd import ops
    dev = torch.device("cpu")

    class ClippingLib:                                        # every launch clips
        def g4c_mlp_run(self, mlp, srcs, n_src, n_rows, io, stream):
            mlp, io = mlp._obj, io._obj
            if io.range_flag is not None:
                for slot in (mlp.range_slot,) + ((io.upd.contents.range_slot,) if io.upd else ()):
                    C.c_int32.from_address(io.range_flag + 4 * slot).value = 1
            return _lib.OK
    monkeypatch.setattr(_lib, "load", lambda: ClippingLib())
    monkeypatch.setattr(_lib, "stream_handle", lambda d: None)
    monkeypatch.setattr(ops, "_range_bufs", {})
    monkeypatch.setattr(ops.RangeFlags, "active", None)
    reads = []
    read_flags = ops._read_flags
    monkeypatch.setattr(ops, "_read_flags", lambda buf: (reads.append(1), read_flags(buf))[1])
    sa, su, sb, so = "T.model_a.mlp", "T.model_a.upd", "T.model_b.mlp", "T.outside.mlp"

    def packed(site, split="f16x2"):
        return types.SimpleNamespace(split=split, precision="bf16x6", desc=_lib.g4c_mlp_t(range_slot=ops._range_slot(site)))

    def launch(p, upd=None):
        io = _lib.g4c_mlp_io_t(upd=C.pointer(upd.desc) if upd is not None else None)
        ops._run(p, None, 1, 64, io, dev, 0.0, 0.0)
        return io

    def set_sites(buf):
        return sorted(n for s in torch.nonzero(buf).flatten().tolist() for n in ops._range_sites[s])
    pa, pu, pb, po = packed(sa), packed(su), packed(sb), packed(so)
    default = ops._range_buffer(dev)
    a, b = ops.RangeFlags(dev), ops.RangeFlags(dev)
    elsewhere = ops.RangeFlags(torch.device("meta"))          # a consumer on another device
    with a:
        launch(pa, upd=pu)                                    # the fused MP layer: both slots, one buffer
        with b:
            launch(pb)                                        # nested scopes: the innermost consumer's
        assert ops.RangeFlags.active is a
        with elsewhere:
            launch(po)                                        # the innermost consumer is not on the launch's device: the default
    assert ops.RangeFlags.active is None
    assert launch(packed(so, split="bf16x3")).range_flag is None          # only f16x3 launches carry a buffer
    assert set_sites(a.buf) == [sa, su] and set_sites(b.buf) == [sb] and set_sites(default) == [so]
    # the report and the check read the default buffer only; a consumer reads its own, once, after it has left its scope
    assert ops.f16_range_report(dev, clear=False) == [so]
    del reads[:]
    assert a.take() == [sa, su] and len(reads) == 1 and int(a.buf.sum()) == 0
    assert a.take() == [] and b.take() == [sb] and b.take() == []
    launch(pa)                                                # model A's MLP launched outside A: never A's
    assert a.take() == [] and set_sites(default) == [sa, so]
    with a:
        launch(pa)
    assert ops.f16_range_report(dev, clear=False) == [sa, so]          # (clear=False: read, kept)
    assert ops.f16_range_report(dev, sites=[sa, sb]) == [sa]           # sites=: only these are looked at and cleared
    assert ops.f16_range_report(dev, clear=False) == [so]
    with pytest.warns(RuntimeWarning, match="T.outside.mlp"):
        assert ops.check_f16_range(dev, "test") == [so]
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        assert ops.check_f16_range(dev) == [] and ops.f16_range_report(dev) == []
    assert a.take() == [sa]


def test_csr_plan_knows_a_uniform_in_degree():
    """CsrPlan.uniform_deg (what G4C_AGG_UNIFORM is fed with): k when EVERY segment has exactly k rows, else 0 (one shorter or
    one empty segment is enough)."""
    dev = torch.device("cpu")
    assert plan.build_csr(torch.arange(50).repeat_interleave(6), 50, dev).uniform_deg == 6
    assert plan.build_csr(torch.arange(7).repeat_interleave(5), 7, dev).uniform_deg == 5
    ragged = torch.cat([torch.arange(49).repeat_interleave(6), torch.full((5,), 49)])
    assert plan.build_csr(ragged, 50, dev).uniform_deg == 0
    assert plan.build_csr(torch.arange(49).repeat_interleave(6), 50, dev).uniform_deg == 0          # the last target is empty
    assert plan.build_csr(torch.arange(3).repeat_interleave(40), 3, dev).uniform_deg == 0           # beyond 32 rows: not offered


def test_row_split_column_order_is_the_mfma_lane_order():
    """ops._rs_k_order (include/g4c.h "row-split order"): position 32 j + 8 g + 4 h + e holds feature 32 j + 16 h + 4 g + e — the eight
    values lane (n, g) of a 16x16x32 MFMA holds of 32-feature step j are 16 contiguous bytes; rs_rows_to_natural undoes it; the tag
    survives row slices and is refused for anything but bf16 [n, 128] rows."""
    import torch
    from graphs4cfd_amd import ops
    order = ops._rs_k_order(torch.device("cpu")).tolist()
    assert sorted(order) == list(range(128))
    for j in range(4):
        for g in range(4):
            got = order[32 * j + 8 * g: 32 * j + 8 * g + 8]
            # a C-layout lane holds features 16 b + 4 g + e of feature blocks b = 2 j and 2 j + 1
            assert got == [16 * (2 * j) + 4 * g + e for e in range(4)] + [16 * (2 * j + 1) + 4 * g + e for e in range(4)]
    rows = torch.arange(3 * 128, dtype=torch.float32).reshape(3, 128).to(torch.bfloat16)
    tagged = ops.RsOrderedRows.tag(rows[:, order].contiguous())
    assert isinstance(tagged[1:], ops.RsOrderedRows)
    back = ops.rs_rows_to_natural(tagged)
    assert type(back) is torch.Tensor and torch.equal(back, rows)
    with pytest.raises(ValueError):
        ops.RsOrderedRows.tag(rows.float())


def test_row_split_tag_is_dropped_by_anything_that_moves_columns():
    """ops.RsOrderedRows tells a reader to put the columns back in feature order.  An operation that changes columns, their type or their
    values must therefore return a plain Tensor — otherwise rows a caller already reordered by hand (t.index_select(1, inv)) would be
    reordered a second time by mlp_forward, silently.  Row selections, views, contiguous, clone, detach and device moves keep it."""
    import torch
    from graphs4cfd_amd import ops
    R = ops.RsOrderedRows
    order = ops._rs_k_order(torch.device("cpu"))
    inv = torch.argsort(order)
    t = R.tag(torch.randn(12, 128).to(torch.bfloat16)[:, order].contiguous())
    plain = {"column slice": t[:, :64], "column gather": t[:, inv], "float": t.float(), "cat dim 1": torch.cat([t, t], 1),
             "cat dim 0": torch.cat([t, t], 0), "index_select dim 1": t.index_select(1, inv), "add": t + 1, "mul": t * 2, "neg": -t,
             "sub tagged": t - t, "transpose": t.t(), "one row": t[3], "as_subclass": t.as_subclass(torch.Tensor), "split": torch.split(t, 5)[0]}
    for name, x in plain.items():
        assert type(x) is torch.Tensor, (name, type(x))
    kept = {"row slice": t[2:7], "row slice, all columns": t[2:7, :], "row gather": t[torch.tensor([0, 5, 5])],
            "index_select dim 0": t.index_select(0, torch.tensor([1, 2])), "narrow dim 0": t.narrow(0, 1, 4), "view": t.view(12, 128),
            "reshape": t.reshape(-1, 128), "contiguous": t.contiguous(), "clone": t.clone(), "detach": t.detach(), "to device": t.to("cpu"),
            "cpu": t.cpu(), "to same dtype": t.to(torch.bfloat16)}
    for name, x in kept.items():
        assert type(x) is R, (name, type(x))
    assert torch.equal(kept["row slice"].as_subclass(torch.Tensor), t.as_subclass(torch.Tensor)[2:7])
    # the reader's guard sees what the caller did: a hand-made natural copy is no longer tagged, rs_rows_to_natural's result is not either
    by_hand = t.index_select(1, inv)
    assert type(by_hand) is torch.Tensor and torch.equal(by_hand, ops.rs_rows_to_natural(t))
    if torch.cuda.is_available():
        assert type(t.to("cuda")) is R and type(t.cuda().cpu()) is R


def test_remus_program_knows_which_run_outputs_only_mlps_read():
    """remus_gnn._mlp_readers_only: the edge latents a run of EdgeMPs leaves behind may be stored as the bf16 rows their readers round
    them to (rounded-bf16 mode) exactly where no UpEdgeMP projects them with fp32 arithmetic (edgeScalarToNodeVector, nn/blocks.py:420-430)
    before the level's next run replaces them."""
    from graphs4cfd_amd.nn.remus_gnn import NsRotEquiTreeScaleGNN as M
    prog = M._PROGRAM
    at = {name: k for k, (_, name, _) in enumerate(prog)}
    lvl = {name: l for _, name, l in prog}
    got = {name: M._mlp_readers_only(prog, at[name], lvl[name]) for name in ("mp114", "mp212", "mp34", "mp222", "mp124")}
    # mp114 -> down_mp12 (products) and up_mp21 (skip input); mp212 -> down_mp23, up_mp32 (skip); mp124 -> decoder: MLP operands only.
    # mp34 -> up_mp32 and mp222 -> up_mp21 project the latents of the coarse side: fp32 readers.
    assert got == {"mp114": True, "mp212": True, "mp34": False, "mp222": False, "mp124": True}, got


# ------------------------------------------------------------------ MLP.PackSpec: the key of an MLP's packed weight images
@pytest.fixture
def specs_only(monkeypatch):
    """MLP's packing entry points return the description they would ask MLP._image for; loading the library is an error."""
    from graphs4cfd_amd import ops
    from graphs4cfd_amd.nn import blocks as B

    def no_library():
        raise AssertionError("deriving a PackSpec loaded the library")
    monkeypatch.setattr(_lib, "load", no_library)
    monkeypatch.setattr(B.MLP, "_image", lambda self, spec: spec)
    prev = ops.set_mlp_precision("bf16")          # (the rounded-bf16 mode: the one with row-split streams and orders)
    yield B
    ops.set_mlp_precision(prev)


def _named_requests(B):
    """What the call sites of nn/blocks.py ask for, under the names they used when every call site spelled its own key."""
    H = 128
    msg, upd = B.MLP(3 * H, (H, H, H), layer_norm=True), B.MLP(2 * H, (H, H), layer_norm=True)
    two = ([H, H], [False, False])
    return {
        "hoist": lambda: msg._packed_cols(0, H, [H], [False], False),
        "hoist1": lambda: msg._packed_cols(H, 2 * H, [H], [False], True),
        "hoist_rs": lambda: msg._packed_cols(0, H, [H], [False], False, rs_order=True),
        "hoist1_rs": lambda: msg._packed_cols(H, 2 * H, [H], [False], True, rs_rows=True),
        "hoist1_rs/rs_in": lambda: msg._packed_cols(H, 2 * H, [H], [False], True, rs_rows=True, rs_in=True),
        "hoist1, next block": lambda: msg._packed_cols(2 * H, 3 * H, [H], [False], True),
        "packed": lambda: msg.packed([H, H, H], [False, False, False]),
        "packed, a block negated": lambda: msg.packed([H, H, H], [True, False, False]),
        "packed, a block in the row-split order": lambda: upd.packed(*two, None, [True, False]),
        "update": lambda: upd.packed(*two),
        "heads": lambda: upd._heads_spec(two, msg, H, [H, H]),
        "heads, rs_rows": lambda: upd._heads_spec(two, msg, H, [H, H], rs_rows=True),
        "heads, one": lambda: upd._heads_spec(two, msg, H, [H]),
        "rs2 format 4": lambda: upd._image(upd._spec(*two, stream=_lib.WFMT_BF16_RS2)),
        "rs2 format 5": lambda: upd._image(upd._spec(*two, stream=_lib.WFMT_BF16_RS2N)),
        "rs2 format 4, heads": lambda: upd._heads_spec(two, msg, H, [H, H], stream=_lib.WFMT_BF16_RS2),
        "rs2 format 5, heads": lambda: upd._heads_spec(two, msg, H, [H, H], stream=_lib.WFMT_BF16_RS2N),
    }


def test_pack_specs_of_different_images_are_different_keys(specs_only):
    """One cache per MLP, keyed by the image's description alone: every request the blocks make for a different weight stream is a
    different dictionary key — among them the pairs that once shared a hand-written tag — and the same request twice is the same key."""
    requests = _named_requests(specs_only)
    specs = {name: ask() for name, ask in requests.items()}
    assert all(isinstance(s, specs_only.PackSpec) for s in specs.values()), specs
    assert len({s: name for name, s in specs.items()}) == len(specs), "two different images share a key"
    names = sorted(specs)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            assert specs[a] != specs[b] and hash(specs[a]) is not None, (a, b)
    # (a name in front of MLP._packed_cols' arguments, as call sites once passed to tell their images apart, reaches no key)
    H, msg = 128, specs_only.MLP(384, (128, 128, 128), layer_norm=True)
    for name in ("hoist1", "anything else"):
        assert msg._packed_cols(name, H, 2 * H, [H], [False], True) == msg._packed_cols(H, 2 * H, [H], [False], True)
        assert msg._packed_cols(name, H, 2 * H, [H], [False], True, rs_rows=True) != msg._packed_cols(name, H, 2 * H, [H], [False], True)
    again = {name: ask() for name, ask in requests.items()}
    assert again == specs and all(hash(again[n]) == hash(specs[n]) for n in names)
    # the stream's arithmetic is part of the key: the same request in another mode is another image
    from graphs4cfd_amd import ops
    prev = ops.set_mlp_precision("f16x3")
    try:
        assert requests["hoist"]() != specs["hoist"] and requests["packed"]() != specs["packed"]
    finally:
        ops.set_mlp_precision(prev)


def test_every_field_of_a_pack_spec_is_part_of_the_key(specs_only):
    import dataclasses
    requests = _named_requests(specs_only)

    def other(v):
        if isinstance(v, bool):
            return not v
        if isinstance(v, int):
            return v + 1
        if isinstance(v, str):
            return v + "'"
        if isinstance(v, tuple):
            return v + v[:1] if v else (0,)
        if v is None:
            return ()
        raise TypeError(f"no other value known for a field of type {type(v)}")

    for name in ("hoist1_rs/rs_in", "heads, rs_rows", "rs2 format 5"):
        spec = requests[name]()
        fields = dataclasses.fields(spec)
        assert len(fields) >= 13
        for f in fields:
            changed = dataclasses.replace(spec, **{f.name: other(getattr(spec, f.name))})
            assert changed != spec and len({spec: 0, changed: 1}) == 2, (name, f.name)
            assert dataclasses.replace(changed, **{f.name: getattr(spec, f.name)}) == spec, (name, f.name)
    with pytest.raises(dataclasses.FrozenInstanceError):
        spec.rs_rows = True


def test_requests_no_launch_can_carry_are_refused_before_anything_is_built(specs_only):
    """No heads from a consumer whose first layer is not 128 wide, for widths other than 128, for more heads than a launch has, or from an MLP
    that is a chain of launches: None, decided from shapes — the row-split update format included.  Blocks that do not add up to the
    image's columns are an error at the same point."""
    B, H = specs_only, 128
    msg, upd = B.MLP(3 * H, (H, H, H), layer_norm=True), B.MLP(2 * H, (H, H), layer_norm=True)
    narrow_consumer, chain = B.MLP(3 * H, (64, H), layer_norm=True), B.MLP(2 * H, (256, H), layer_norm=True)
    two = ([H, H], [False, False])
    for stream in (0, _lib.WFMT_BF16_RS2):
        assert upd._heads_spec(two, narrow_consumer, H, [H, H], stream=stream) is None
        assert upd._heads_spec(two, msg, H, [64, 64], stream=stream) is None
        assert upd._heads_spec(two, msg, H, [H] * (_lib.MAX_HEADS + 1), stream=stream) is None
        assert upd._heads_spec(two, msg, H, [], stream=stream) is None
        assert chain._heads_spec(two, msg, H, [H, H], stream=stream) is None
    assert B.MLP(2 * H, (H, 64), layer_norm=True)._heads_spec(two, msg, H, [H, H]) is None          # (heads read a 128-wide output)
    from graphs4cfd_amd.ops import Source
    x = [Source(torch.randn(8, H)), Source(torch.randn(8, H))]
    with torch.no_grad():
        assert upd.run_with_heads(x, 8, _lib.ACT_SELU, narrow_consumer, H, [H, H]) is None
        assert upd.run_with_heads(x, 8, _lib.ACT_SELU, msg, H, [64, 64], rs_rows=True) is None
        assert chain.run_with_heads(x, 8, _lib.ACT_SELU, msg, H, [H, H]) is None
    assert upd.run_with_heads(x, 8, _lib.ACT_SELU, msg, H, [H, H]) is None          # (recorded for autograd: the plain launches)
    with pytest.raises(ValueError, match="expects 384 input columns"):
        msg.packed([H, H], [False, False])
    with pytest.raises(ValueError, match="row-split order"):
        msg._packed_cols(0, H, [H], [False], False, rs_rows=True)


def test_a_cut_stage_recorded_for_autograd_is_an_image_of_its_own(specs_only):
    """A launch of a chain of launches (an MLP outside the one-launch envelope) that takes part of a layer's weight keeps a view of the
    parameter only while the call is recorded for autograd: the image packed for inference holds no path back to the parameter, so the
    recorded call must not be handed it.  Whole layers are passed as the parameters themselves: one image serves both."""
    from graphs4cfd_amd.ops import Source
    chain = specs_only.MLP(128, (256, 128), layer_norm=True)
    x, halves = [Source(torch.randn(8, 128))], [Source(torch.randn(8, 128)), Source(torch.randn(8, 128))]
    with torch.no_grad():
        cut, whole = chain._stage(x, layers=(0, 1), rows=(0, 128)), chain._stage(halves, layers=(1, 2))
    with torch.enable_grad():
        cut_g, whole_g = chain._stage(x, layers=(0, 1), rows=(0, 128)), chain._stage(halves, layers=(1, 2))
    assert cut != cut_g and cut_g.grad and not cut.grad
    assert whole == whole_g and not whole.grad and whole.layer_norm and not cut.layer_norm
