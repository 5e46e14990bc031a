"""The caller's fp16 range certificate (g4c_mlp_t.range_certified) on the device: a certified launch runs the kernel instantiation
without the range tracker and gives bit for bit what the tracked one gives; a launch without a complete proof keeps its tracker and
flags a clip exactly as before; in a model's forward every launch that reads only LayerNorm'd latents is certified."""
import warnings

import pytest
import torch

import graphs4cfd_amd as gfd
from graphs4cfd_amd import _lib, ops, plan
from graphs4cfd_amd import synthetic as S
from graphs4cfd_amd.nn.blocks import MLP
from graphs4cfd_amd.ops import Source

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SELU, NONE = _lib.ACT_SELU, _lib.ACT_NONE
WS, WS_CERT, BX6, BX6_CERT = _lib.KERNEL_MLP_WS, _lib.KERNEL_MLP_WS_CERT, _lib.KERNEL_MLP_BX6, _lib.KERNEL_MLP_BX6_CERT


def last_kernel() -> int:
    return int(_lib.load().g4c_mlp_last_kernel())


@pytest.fixture()
def f16x3():
    old = ops.set_mlp_precision("f16x3")
    try:
        with torch.no_grad():          # (the inference forms of the launches: heads, fused aggregation, one launch per MP layer)
            yield
    finally:
        ops.set_mlp_precision(old)


def knn_like_edges(n: int, k: int, seed: int):
    """[2, n k] edges grouped by receiver, k per receiver (the level-1 layout of a kNN mesh)."""
    gen = torch.Generator().manual_seed(seed)
    col = torch.arange(n).repeat_interleave(k)
    row = torch.randint(0, n, (n * k,), generator=gen)
    return torch.stack([row, col]).to(DEV)


def test_level1_message_launch_certified_equals_tracked(f16x3):
    """600k x 128 rows, dense k = 6, SELU on load, two gathered additive blocks, fused mean: mlp_ws_kernel<.., DENSE> with and without
    the tracker."""
    n, k, H = 100_000, 6, 128
    torch.manual_seed(0)
    mlp = MLP(3 * H, (H, H, H), True).to(DEV)
    ei = knn_like_edges(n, k, 1)
    ep, csr = plan.edge_csr(ei, n)
    assert csr.uniform_deg == k and ops.can_fuse_aggregation(csr, H)
    e = torch.randn(n * k, H, device=DEV).clamp_(-4, 4)
    prods = [torch.randn(n, H, device=DEV).clamp_(-4, 4) for _ in range(2)]
    pk = mlp._packed_cols(0, H, [H], [False], False)

    def launch(bound):
        srcs = [Source(e, pre_act=SELU, bound=bound), Source(prods[0], index=ep.row, additive=True, bound=bound),
                Source(prods[1], index=ep.col, additive=True, bound=bound)]
        agg = torch.empty(n, H, device=DEV)
        y = ops.mlp_forward(pk, srcs, n * k, NONE, agg=(csr, agg, True))
        return y, agg, last_kernel(), ops.take_bounds()
    y0, a0, k0, lb0 = launch(None)
    y1, a1, k1, lb1 = launch(4.0)
    assert (k0, k1) == (WS, WS_CERT), (k0, k1)
    assert lb0.converted is None and ops.certifies(lb1.converted) and lb1.out == lb0.out
    assert torch.equal(y0, y1) and torch.equal(a0, a1)
    assert float(y1.abs().max()) <= lb1.out          # (the LayerNorm bound of the rows the launch wrote)
    # a bound that is too large for the proof: tracked again
    assert launch(3.0e4)[2] == WS


def test_level1_node_launch_certified_equals_tracked(f16x3):
    """[aggregate | v] -> three layers -> LayerNorm -> SELU, + the next layer's two product heads: mlp_bx6_kernel with and without the
    tracker, at the level-1 size and at a small launch (the deep-ring instantiation)."""
    H = 128
    torch.manual_seed(1)
    upd, nxt = MLP(2 * H, (H, H, H), True).to(DEV), MLP(3 * H, (H, H, H), True).to(DEV)
    for n in (100_000, 3_000):
        agg, v = torch.randn(n, H, device=DEV).clamp_(-4, 4), torch.randn(n, H, device=DEV).clamp_(-4, 4)

        def launch(bound):
            got = upd.run_with_heads([Source(agg, bound=bound), Source(v, bound=bound)], n, SELU, nxt, H, [H, H])
            return got[0], got[1], last_kernel(), ops.take_bounds()
        y0, h0, k0, lb0 = launch(None)
        y1, h1, k1, lb1 = launch(4.0)
        assert (k0, k1) == (BX6, BX6_CERT), (n, k0, k1)
        assert lb0.converted is None and ops.certifies(lb1.converted) and lb1.heads is not None
        assert torch.equal(y0, y1) and all(torch.equal(a, b) for a, b in zip(h0, h1))
        assert float(y1.abs().max()) <= lb1.out and all(float(h.abs().max()) <= b for h, b in zip(h1, lb1.heads))


def test_fused_layer_certified_equals_tracked(f16x3):
    """One launch per MP layer (mlp_ws_kernel<.., NODE>): message loop and node phase with and without their trackers."""
    n, k, H = 10_000, 6, 128
    torch.manual_seed(2)
    msg, upd, nxt = MLP(3 * H, (H, H, H), True).to(DEV), MLP(2 * H, (H, H, H), True).to(DEV), MLP(3 * H, (H, H, H), True).to(DEV)
    ei = knn_like_edges(n, k, 3)
    ep, csr = plan.edge_csr(ei, n)
    e, v = torch.randn(n * k, H, device=DEV).clamp_(-4, 4), torch.randn(n, H, device=DEV).clamp_(-4, 4)
    prods = [torch.randn(n, H, device=DEV).clamp_(-4, 4) for _ in range(2)]
    pk_msg = msg._packed_cols(0, H, [H], [False], False)
    pk_upd = upd._image(upd._heads_spec(([H, H], [False, False]), nxt, H, [H, H]))

    def launch(bound):
        srcs = [Source(e, pre_act=SELU, bound=bound), Source(prods[0], index=ep.row, additive=True, bound=bound),
                Source(prods[1], index=ep.col, additive=True, bound=bound)]
        heads = [torch.empty(n, H, device=DEV) for _ in range(2)]
        e_new, v_new, _ = ops.mp_layer_forward(pk_msg, srcs, n * k, csr, True, pk_upd, v, SELU, head_outs=heads, v_bound=bound)
        return e_new, v_new, heads, last_kernel(), ops.take_bounds()
    e0, v0, h0, k0, _ = launch(None)
    e1, v1, h1, k1, lb = launch(4.0)
    assert (k0, k1) == (WS, WS_CERT), (k0, k1)
    assert torch.equal(e0, e1) and torch.equal(v0, v1) and all(torch.equal(a, b) for a, b in zip(h0, h1))
    assert float(e1.abs().max()) <= lb.e and float(v1.abs().max()) <= lb.out


def test_a_certified_launch_never_writes_its_flag_and_a_tracked_one_still_does(f16x3):
    """The certificate is the caller's promise: a launch that carries it writes nothing into its flag word even when the promise is
    false (which is why only a proof may set it); the same launch without it flags the clip."""
    n, H = 5_000, 128
    torch.manual_seed(3)
    mlp = MLP(H, (H, H, H), True).to(DEV)
    x = torch.full((n, H), 3.0e5, device=DEV)
    flags = ops.RangeFlags(DEV)
    with flags:
        mlp.run([Source(x, bound=1.0)], n)          # (a false bound, set by hand)
        assert last_kernel() in (BX6_CERT, WS_CERT)
    assert flags.take() == []
    with flags:
        mlp.run([Source(x)], n)
        assert last_kernel() in (BX6, WS)
    assert len(flags.take()) == 1


def test_user_tensors_are_still_flagged(f16x3):
    """MLP.forward(x) and GNBlock.forward(v, e, ...) on tensors scaled to 3e4 (SELU / the first layer push them past 65504): a
    user's tensor carries no bound, the launches are tracked and the clip is reported."""
    H = 128
    torch.manual_seed(4)
    mlp = MLP(H, (H, H, H), True).to(DEV)
    mlp._site = "T.user.mlp"
    ops.f16_range_clear(DEV)
    with torch.no_grad():
        mlp(torch.randn(5000, H, device=DEV) * 3e4)
    assert last_kernel() in (BX6, WS)
    assert ops.f16_range_report(DEV) == ["T.user.mlp"]
    block = gfd.nn.blocks.GNBlock((3 * H, (H, H, H), True), (2 * H, (H, H, H), True)).to(DEV)
    block.edge_mlp._site, block.node_mlp._site = "T.user.edge_mlp", "T.user.node_mlp"
    n, k = 5000, 6
    ei = knn_like_edges(n, k, 5)
    with torch.no_grad():
        block(torch.randn(n, H, device=DEV) * 3e4, torch.randn(n * k, H, device=DEV) * 3e4, ei)
    assert "T.user.edge_mlp" in ops.f16_range_report(DEV)


class Recorder:
    """Every fused-MLP launch of a scope: (site of the MLP, with a fused node MLP, rows, kernel that ran, proven bound of the values
    the launch converts to fp16 or None — of a fused layer: the larger of its two MLPs')."""

    def __init__(self, monkeypatch):
        self.launches = []
        run, certify = ops._run, ops._certify
        proofs = []

        def certifying(packed, sources, act, residual, tracked):
            lb = certify(packed, sources, act, residual, tracked)
            proofs.append(lb.converted)
            return lb

        def recording(packed, arr, n_src, n_rows, io, dev, flops, nbytes):
            run(packed, arr, n_src, n_rows, io, dev, flops, nbytes)
            conv = None if any(c is None for c in proofs) else max(proofs)
            del proofs[:]
            self.launches.append((packed.site, bool(io.upd), int(n_rows), last_kernel(), conv))
        monkeypatch.setattr(ops, "_certify", certifying)
        monkeypatch.setattr(ops, "_run", recording)


def headline_model():
    g = S.mus_graph(100_000, levels=3, seed=0, device=DEV)
    torch.manual_seed(0)
    model = gfd.nn.NsThreeScaleGNN(arch=S.mus_arch("NsThreeScaleGNN", 128), device=DEV)
    model.eval()
    return g, model


def test_headline_step_certifies_every_launch_behind_the_first_mp_layer(f16x3, monkeypatch):
    """NsThreeScaleGNN, 100 000 nodes, one eager validated forward.  The encoders have no LayerNorm: v0 depends on data, so the encoder
    launches and the first MP layer's message and node launches stay tracked (they read v0 or its products).  Every later launch reads
    LayerNorm outputs only (the Down / Up MLPs have LayerNorm, pool_edge averages certified rows): a condition, not a measurement —
    at least 7 of the 8 level-1 message launches, 7 of the 8 level-1 node launches and all 8 fused coarse layers run certified."""
    g, model = headline_model()
    rec = Recorder(monkeypatch)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        with torch.no_grad():
            model(g)
    L = rec.launches
    lvl1 = [f"NsThreeScaleGNN.mp1{a}{b}" for a in (1, 2) for b in (1, 2, 3, 4)]
    msg = [x for x in L if not x[1] and any(x[0] == f"{m}.edge_mlp" for m in lvl1) and x[2] == 600_000]
    node = [x for x in L if any(x[0] == f"{m}.node_mlp" for m in lvl1)]
    fused = [x for x in L if x[1]]
    print(f"{len(L)} fused-MLP launches; level-1 message {[x[3] for x in msg]}, node {[x[3] for x in node]}, fused layers {[x[3] for x in fused]}")
    assert len(msg) == 8 and len(node) == 8 and len(fused) == 8, (len(msg), len(node), len(fused))
    assert all(x[3] in (WS, WS_CERT) for x in msg + fused) and all(x[3] in (BX6, BX6_CERT) for x in node)
    assert sum(x[3] == WS_CERT for x in msg) >= 7 and msg[0][3] == WS
    assert sum(x[3] == BX6_CERT for x in node) >= 7 and node[0][3] == BX6
    assert all(x[3] == WS_CERT for x in fused)
    assert sum(x[3] in (WS_CERT, BX6_CERT) for x in L) >= 22
    # the margin of the proof with default-initialised weights: above 10x for every certified launch of the MP layers
    certified = [x for x in msg + node + fused if x[3] in (WS_CERT, BX6_CERT)]
    print("proven bounds of the converted values:", [(x[0].split(".", 1)[1], round(x[4], 1)) for x in certified])
    assert all(65504.0 / x[4] > 10.0 for x in certified), [(x[0], x[4]) for x in certified]


def test_a_model_whose_bound_fails_runs_tracked_and_recomputes(f16x3, monkeypatch):
    """mp111.edge_mlp's LayerNorm gain x 3e4: the launches that READ its latents — the next message launch, the node update through
    the aggregate — lose their proof (the producer's bound travels with the Source; the image and its norms were rebuilt), run the
    tracked kernels, flag the clip, and solve() recomputes in bf16x6 as before; launches that read other producers keep theirs."""
    g = S.mus_graph(3000, levels=2, seed=3)
    torch.manual_seed(4)
    model = gfd.nn.NsTwoScaleGNN(arch=S.mus_arch("NsTwoScaleGNN", 128), device=DEV)
    rec = Recorder(monkeypatch)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        model.solve(g.clone(), 1, capture=False)
    # (first launch per MLP; at 18 000 edges an MP layer is ONE launch under its message MLP's name, the node update fused behind it)
    def first_kernels():
        seen = {}
        for s, _, _, k, _ in rec.launches:
            seen.setdefault(s.split(".", 1)[1], k)          # (the first pass: f16x3)
        return seen
    CERT, TRACKED = (WS_CERT, BX6_CERT), (WS, BX6)
    before = first_kernels()
    print("before:", before)
    assert before["mp111.edge_mlp"] in TRACKED          # reads v0 and its products: tracked
    assert before["mp112.edge_mlp"] in CERT and before["mp113.edge_mlp"] in CERT
    with torch.no_grad():
        model.mp111.edge_mlp.MLP.layer_norm.weight.mul_(3e4)
    model.invalidate_packed()
    del rec.launches[:]
    with pytest.warns(RuntimeWarning, match="recomputed in 'bf16x6'") as w:
        out = model.solve(g.clone(), 2, capture=False)
    assert any("NsTwoScaleGNN.mp11" in str(r.message) for r in w)
    after = first_kernels()
    print("after:", after)
    # the readers of mp111's message latents: the next layer (message rows; in a fused layer also the node update through the
    # aggregate, one certificate for both), and — through pool_edge's mean of mp114's rows — nothing: mp114 has its own LayerNorm
    assert after["mp111.edge_mlp"] in TRACKED and after["mp112.edge_mlp"] in TRACKED, after
    assert after["mp113.edge_mlp"] in CERT, after
    old = ops.set_mlp_precision("bf16x6")
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)
            ref = model.solve(g.clone(), 2, capture=False)
    finally:
        ops.set_mlp_precision(old)
    assert torch.equal(out, ref)
