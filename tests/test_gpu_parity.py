"""Parity of the HIP path (through the C-ABI of libg4c.so) with the oracle and with the golden
vectors produced by the reference's own source.  Every test needs a real MI355X.

Tolerances (fp32): per block max|d| <= 1e-4 on O(1) LayerNorm-scale outputs;
full forward <= 5e-4; rollouts stated per length (error compounds autoregressively)."""
import pytest
import torch

import graphs4cfd_amd as gfd
from graphs4cfd_amd import _lib, ops, plan, synthetic as S
from graphs4cfd_amd.nn import blocks as B
from oracle import g4c_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


@pytest.fixture(autouse=True)
def _inference():
    """This file covers the inference path (every launch form, including the inference-only ones: out=, heads, fused
    aggregation, explicit kernel variants).  The training path has its own file (test_gpu_train.py)."""
    with torch.no_grad():
        yield
BLOCK = dict(rtol=1e-4, atol=1e-4)
FWD = dict(rtol=5e-4, atol=5e-4)


def cu(x):
    if torch.is_tensor(x):
        return x.to(DEV)
    if isinstance(x, dict):
        return {k: cu(v) for k, v in x.items()}
    return x


def load_weights(module, weights):
    module.load_state_dict(weights)
    return module.to(DEV)


# ------------------------------------------------------------------ segment reduce (the scatter)
@pytest.mark.parametrize("width", [128, 64, 32, 16, 6, 1])
@pytest.mark.parametrize("reduce", ["sum", "mean"])
def test_segment_reduce_random_index(width, reduce):
    torch.manual_seed(width)
    n_seg, m = 500, 4000
    idx = torch.randint(0, n_seg - 20, (m,))      # last 20 segments empty
    idx[:300] = 7                                  # hub
    src = torch.randn(m, width)
    ref = O.scatter(src, idx, n_seg, reduce)
    csr = plan.build_csr(idx, n_seg, DEV)
    out = ops.segment_reduce(src.to(DEV), csr, reduce == "mean")
    # plan order == index order within a segment -> same summation order as a sequential scatter_add_
    torch.testing.assert_close(out.cpu(), ref, rtol=1e-6, atol=1e-6)
    assert torch.all(out[-20:] == 0)


def test_segment_reduce_sorted_bit_exact_and_activations():
    torch.manual_seed(0)
    k, n = 6, 3000
    idx = torch.arange(n).repeat_interleave(k)
    src = torch.randn(n * k, 128)
    csr = plan.build_csr(idx, n, DEV)
    assert csr.perm is None
    out = ops.segment_reduce(src.to(DEV), csr, False)
    ref = torch.zeros(n, 128).index_add_(0, idx, src)
    assert torch.equal(out.cpu(), ref)
    out = ops.segment_reduce(src.to(DEV), csr, True, act=_lib.ACT_TANH, src_act=_lib.ACT_SELU)
    ref = torch.tanh(O.scatter(torch.nn.functional.selu(src), idx, n, "mean"))
    torch.testing.assert_close(out.cpu(), ref, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("permuted", [False, True])
def test_segment_reduce_large_ragged_bit_exact(permuted):
    """40k ragged segments: bit-identical to a sequential index_add_ in plan order — empty segments at both ends and in long runs,
    segments longer than one batch of rows (8), with and without the plan's permutation; a tensor without any row."""
    torch.manual_seed(5)
    n_seg = 40_003
    deg = torch.randint(0, 12, (n_seg,))
    deg[:40] = 0; deg[-23:] = 0; deg[1000:1100] = 0; deg[5000] = 77; deg[5001] = 9; deg[5002] = 8
    idx = torch.arange(n_seg).repeat_interleave(deg)
    m = int(idx.numel())
    if permuted:
        idx = idx[torch.randperm(m)]
    src = torch.randn(m, 128)
    csr = plan.build_csr(idx, n_seg, DEV)
    assert (csr.perm is not None) == permuted
    out = ops.segment_reduce(src.to(DEV), csr, False)
    ref = torch.zeros(n_seg, 128).index_add_(0, idx, src)
    if not permuted:
        assert torch.equal(out.cpu(), ref)
    else:           # (index_add_ adds in index order = the stable plan's order per segment)
        assert torch.equal(out.cpu(), ref)
    mean = ops.segment_reduce(src.to(DEV), csr, True, act=_lib.ACT_TANH, src_act=_lib.ACT_SELU)
    cnt = torch.bincount(idx, minlength=n_seg).clamp(min=1).float()[:, None]
    ref_m = torch.tanh(torch.zeros(n_seg, 128).index_add_(0, idx, torch.nn.functional.selu(src)) / cnt)
    torch.testing.assert_close(mean.cpu(), ref_m, rtol=1e-5, atol=1e-6)
    # no rows at all
    empty = plan.build_csr(torch.zeros(0, dtype=torch.long), 20_000, DEV)
    z = ops.segment_reduce(torch.zeros(0, 128, device=DEV), empty, True)
    assert z.shape == (20_000, 128) and torch.all(z == 0)


def test_scatter_dropin(golden):
    c = golden("blocks.pt")["scatter"]
    src, idx = c["src"].to(DEV), c["index"].to(DEV)
    torch.testing.assert_close(B.scatter(src, idx, 0, 7, "sum").cpu(), c["sum_7"], rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(B.scatter(src, idx, 0, 7, "mean").cpu(), c["mean_7"], rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(B.scatter(src, idx, 0, None, "mean").cpu(), c["mean_none"], rtol=1e-6, atol=1e-6)


# ------------------------------------------------------------------ blocks vs golden
@pytest.mark.parametrize("i", range(8))
def test_mlp(golden, i):
    c = golden("blocks.pt")[f"mlp_{i}"]
    mlp = load_weights(B.MLP(*c["args"]), c["weights"])
    y = mlp(c["x"].to(DEV))
    torch.testing.assert_close(y.cpu(), c["y"], **BLOCK)


def test_mlp_row_tails_and_leading_dims(golden):
    c = golden("blocks.pt")["mlp_1"]
    mlp = load_weights(B.MLP(*c["args"]), c["weights"])
    w = {f"m.{k}": v for k, v in c["weights"].items()}
    for m in (1, 63, 64, 65, 200):
        x = torch.randn(m, 384)
        torch.testing.assert_close(mlp(x.to(DEV)).cpu(), O.mlp(x, w, "m"), **BLOCK)
    x = torch.randn(3, 5, 384)
    assert mlp(x.to(DEV)).shape == (3, 5, 128)


@pytest.mark.parametrize("rows", [1, 33, 1000, 20000])
def test_mlp_kernel_row_range_launches_agree(rows, monkeypatch):
    """The fp32-MFMA kernel (G4C_WFMT_FP32), whole and split over two row-range launches (g4c_mlp_io_t.row_begin / row_count):
    hoisted edge form (gathered additive terms + SELU-on-load) and the two-block node form, against the oracle MLP on the
    concatenated input.  A row range that does not start at a multiple of 32 is an argument error."""
    H, n = 128, max(rows // 6, 1)
    torch.manual_seed(rows)
    monkeypatch.setattr(ops, "_PRECISION", "fp32")      # the tile variants are the fp32-MFMA kernels
    blk = B.GNBlock((3 * H, (H, H, H), True), (2 * H, (H, H, H), True)).to(DEV)
    e, v, agg = torch.randn(rows, H, device=DEV), torch.randn(n, H, device=DEV), torch.randn(n, H, device=DEV)
    row = torch.randint(0, n, (rows,), device=DEV, dtype=torch.int32)
    col = torch.randint(0, n, (rows,), device=DEV, dtype=torch.int32)
    w = {f"m.{k}": t.cpu() for k, t in blk.edge_mlp.state_dict().items()}
    x = torch.cat([torch.selu(e), v[row.long()], v[col.long()]], 1).cpu()
    ref_e = O.mlp(x, w, "m")
    # first-layer products of the node-side blocks, as _mp_step's hoisting computes them
    W1 = blk.edge_mlp.state_dict()["MLP.linear_1.weight"]
    pr, pc = v @ W1[:, H:2 * H].T, v @ W1[:, 2 * H:].T
    pk_e = blk.edge_mlp._packed_cols(0, H, [H], [False], False)
    src_e = [ops.Source(e, pre_act=_lib.ACT_SELU), ops.Source(pr, index=row, additive=True), ops.Source(pc, index=col, additive=True)]
    pk_v = blk.node_mlp.packed([H, H], [False, False])
    idx = torch.randint(0, n, (n,), device=DEV, dtype=torch.int32)
    src_v = [ops.Source(agg), ops.Source(v, index=idx)]
    wn = {f"m.{k}": t.cpu() for k, t in blk.node_mlp.state_dict().items()}
    ref_v = O.mlp(torch.cat([agg, v[idx.long()]], 1).cpu(), wn, "m")
    with pytest.raises(ValueError, match="row_begin"):
        ops.mlp_forward(pk_e, src_e, rows, rows=(16, rows - 16))

    def launches(pk, src, m, act):
        """The whole range in one launch, and in two launches split at a multiple of 32 into one output."""
        whole = ops.mlp_forward(pk, src, m, act)
        cut = min(((m + 1) // 2 + 31) // 32 * 32, m // 32 * 32)
        split = torch.full_like(whole, float("nan"))
        for r in ((0, cut), (cut, m - cut)):
            ops.mlp_forward(pk, src, m, act, out=split, rows=r)
        return {"whole": whole, "split": split}
    for mode, y in launches(pk_e, src_e, rows, _lib.ACT_NONE).items():
        torch.testing.assert_close(y.cpu(), ref_e, rtol=2e-4, atol=2e-4, msg=lambda m: f"edge {mode}: {m}")
    for mode, y in launches(pk_v, src_v, n, _lib.ACT_SELU).items():
        torch.testing.assert_close(y.cpu(), torch.selu(ref_v), rtol=2e-4, atol=2e-4, msg=lambda m: f"node {mode}: {m}")


@pytest.mark.parametrize("rows", [1, 200, 40000])
def test_mlp_bf16_variant(rows):
    """Opt-in bf16-MFMA MLPs (BASELINE config 3): against the SAME computation with operands rounded to bf16 where
    the kernel rounds them (tight), and against the fp32 oracle at the stated bf16 tolerance (1e-2 scale)."""
    H, n = 128, max(rows // 6, 1)
    torch.manual_seed(rows + 7)
    blk = B.GNBlock((3 * H, (H, H, H), True), (2 * H + 3, (H, H, H), True)).to(DEV)
    e, v = torch.randn(rows, H, device=DEV), torch.randn(n, H, device=DEV)
    row = torch.randint(0, n, (rows,), device=DEV, dtype=torch.int32)
    col = torch.randint(0, n, (rows,), device=DEV, dtype=torch.int32)
    x3 = torch.randn(rows, 3, device=DEV)

    def emulate(mlp, x, exact_from=None):       # bf16-rounded operands, fp32 accumulation (fp64 here), fp32 epilogue
        """`exact_from`: first-layer input columns from there on form a NARROW block, which the kernel multiplies in fp32
        on the vector ALUs (not rounded)."""
        lin = mlp._linears()
        r = lambda t: t.to(torch.bfloat16).double()
        y = x.double()
        for li, l in enumerate(lin):
            W = l.weight.detach()
            if li == 0 and exact_from is not None:
                y = (r(y[:, :exact_from].float()) @ r(W[:, :exact_from]).T + y[:, exact_from:] @ W[:, exact_from:].double().T
                     + l.bias.detach().double())
            else:
                y = r(y.float()) @ r(W).T + l.bias.detach().double()
            if li < len(lin) - 1:
                y = torch.selu(y)
        ln = getattr(mlp.MLP, "layer_norm", None)
        if ln is not None:
            y = torch.nn.functional.layer_norm(y.float(), (y.size(-1),), ln.weight, ln.bias, ln.eps).double()
        return y.float()

    def close_bf16(got, want):
        # an activation that lands on a bf16 rounding tie may round the other way in the kernel's fp32 epilogue than in
        # this fp64 emulation: isolated elements move by one bf16 ulp of an operand, everything else agrees to fp32 noise
        d = (got - want).abs()
        assert d.mean().item() < 2e-4 and d.max().item() < 2e-2, (d.mean().item(), d.max().item())

    old = ops.set_mlp_precision("bf16")
    try:
        # edge MLP, plain 3-block form with SELU-on-load and gathers
        y = blk.edge_mlp.run_coded([ops.Source(e, pre_act=_lib.ACT_SELU), ops.Source(v, index=row), ops.Source(v, index=col)], rows)
        xin = torch.cat([torch.selu(e), v[row.long()], v[col.long()]], 1)
        close_bf16(y, emulate(blk.edge_mlp, xin))
        # node-like MLP with a narrow, unaligned third block and a fused activation
        y2 = blk.node_mlp.run_coded([ops.Source(e), ops.Source(e), ops.Source(x3)], rows, _lib.ACT_TANH)
        close_bf16(y2, torch.tanh(emulate(blk.node_mlp, torch.cat([e, e, x3], 1), exact_from=2 * H)))
    finally:
        ops.set_mlp_precision(old)
    w = {f"m.{k}": t.cpu() for k, t in blk.edge_mlp.state_dict().items()}
    ref = O.mlp(xin.cpu(), w, "m")
    err = (y.cpu() - ref).abs().max().item()
    assert err < 6e-2, err                          # LayerNorm-scale outputs, three bf16 GEMMs deep
    assert (y.cpu() - ref).abs().mean().item() < 6e-3


@pytest.mark.parametrize("prec", ["fp32", "bf16x6", "f16x3"])
@pytest.mark.parametrize("rows", [33, 5000, 40000])
def test_mlp_heads(rows, prec, monkeypatch):
    """Heads (g4c_mlp_io_t.n_heads): the node MLP launch also emits W1[:, H:2H] y and W1[:, 2H:] y of the next edge MLP
    == separate products of the stored output."""
    H = 128
    torch.manual_seed(rows)
    monkeypatch.setattr(ops, "_PRECISION", prec)
    blk = B.GNBlock((3 * H, (H, H, H), True), (2 * H, (H, H, H), True)).to(DEV)
    nxt = B.GNBlock((3 * H, (H, H, H), True), (2 * H, (H, H, H), True)).to(DEV)
    agg, v = torch.randn(rows, H, device=DEV), torch.randn(rows, H, device=DEV)
    res = blk.node_mlp.run_with_heads([ops.Source(agg), ops.Source(v)], rows, _lib.ACT_SELU, nxt.edge_mlp, H, [H, H])
    assert res is not None
    y, (pr, pc) = res
    wn = {f"m.{k}": t.cpu() for k, t in blk.node_mlp.state_dict().items()}
    ref = torch.selu(O.mlp(torch.cat([agg, v], 1).cpu(), wn, "m"))
    torch.testing.assert_close(y.cpu(), ref, rtol=2e-4, atol=2e-4)
    W1 = nxt.edge_mlp.state_dict()["MLP.linear_1.weight"].cpu().double()
    torch.testing.assert_close(pr.cpu(), (y.cpu().double() @ W1[:, H:2 * H].T).float(), rtol=2e-4, atol=2e-4)
    torch.testing.assert_close(pc.cpu(), (y.cpu().double() @ W1[:, 2 * H:].T).float(), rtol=2e-4, atol=2e-4)
    # a launch that cannot carry heads says so instead of computing something else
    assert blk.node_mlp.run_with_heads([ops.Source(agg), ops.Source(v)], rows, _lib.ACT_SELU, nxt.edge_mlp, H, [H, H, H]) is None


@pytest.mark.parametrize("prec", ["f16x3", "bf16x6", "bf16"])
@pytest.mark.parametrize("case", ["knn6", "ragged", "unsorted", "long_segment"])
def test_edge_mlp_with_fused_aggregation(case, prec, monkeypatch):
    """ops.mlp_forward(agg=...): the edge launch also reduces its output rows per target (g4c_mlp_io_t.agg on tiles
    of whole segments) == the plain launch followed by g4c_segment_reduce, bit for bit; inputs the fused kernel cannot
    take (rows not in segment order, a segment longer than a tile) go through the separate reduction transparently."""
    H, n = 128, 700
    torch.manual_seed(21)
    monkeypatch.setattr(ops, "FUSE_AGG", True)
    monkeypatch.setattr(ops, "_PRECISION", prec)       # ("bf16": G4C_WFMT_BF16, the rounded-operand mode of config 3)
    if case == "knn6":
        col = torch.arange(n).repeat_interleave(6)
    elif case == "ragged":                          # degrees 0..9 incl. empty targets at both ends
        deg = torch.randint(0, 10, (n,)); deg[0] = 0; deg[-1] = 0; deg[5:9] = 0
        col = torch.arange(n).repeat_interleave(deg)
    elif case == "unsorted":
        col = torch.randint(0, n, (4000,))
    else:
        deg = torch.full((n,), 3); deg[17] = 40
        col = torch.arange(n).repeat_interleave(deg)
    E = int(col.numel())
    row = torch.randint(0, n, (E,))
    edge_index = torch.stack([row, col]).to(DEV)
    blk = B.GNBlock((3 * H, (H, H, H), True), (2 * H, (H, H, H), True)).to(DEV)
    v, e = torch.randn(n, H, device=DEV), torch.randn(E, H, device=DEV)
    ep, csr = plan.edge_csr(edge_index, n)
    assert (csr.tiles() is not None) == (case in ("knn6", "ragged"))
    srcs = [ops.Source(e), ops.Source(v, index=ep.row), ops.Source(v, index=ep.col)]
    pk = blk.edge_mlp.packed([H, H, H], [False] * 3)
    for mean in (True, False):
        agg = torch.full((n, H), float("nan"), device=DEV)
        y = ops.mlp_forward(pk, srcs, E, agg=(csr, agg, mean))
        y_ref = ops.mlp_forward(pk, srcs, E)
        agg_ref = ops.segment_reduce(y_ref, csr, mean)
        assert torch.equal(y, y_ref) and torch.equal(agg, agg_ref)
        if prec == "bf16" and csr.tiles() is not None:
            # message rows stored as bf16 (rows_dtype): the rounded rows, the same fp32 aggregate; as an input block they read
            # exactly like their fp32 widening
            agg16 = torch.full((n, H), float("nan"), device=DEV)
            y16 = ops.mlp_forward(pk, srcs, E, agg=(csr, agg16, mean), rows_dtype=torch.bfloat16)
            assert y16.dtype == torch.bfloat16 and torch.equal(y16, y_ref.to(torch.bfloat16)) and torch.equal(agg16, agg_ref)
            nxt16 = ops.mlp_forward(pk, [ops.Source(y16, pre_act=_lib.ACT_SELU)] + srcs[1:], E)
            nxt32 = ops.mlp_forward(pk, [ops.Source(y16.float(), pre_act=_lib.ACT_SELU)] + srcs[1:], E)
            assert torch.equal(nxt16, nxt32)
        # and against an independent dense reduction
        dense = torch.zeros(n, H, device=DEV).index_add_(0, col.to(DEV), y_ref)
        if mean:
            dense /= torch.bincount(col, minlength=n).clamp(min=1).to(DEV)[:, None]
        torch.testing.assert_close(agg, dense, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("rows", [1, 77, 5000])
def test_mlp_narrow_input_blocks(rows):
    """Narrow input blocks (g4c_src_t.additive == 2: the 2..5-wide encoder / DownMP / UpMP inputs) are multiplied in fp32
    on the vector ALUs instead of being padded to 128-k matrix blocks: all-narrow first layers (edge encoder), narrow +
    wide mixes with a folded sign (UpMP), strided views, vs the oracle MLP on the concatenated input."""
    H = 128
    torch.manual_seed(rows + 3)
    enc = B.MLP(2, (H, H, H), False).to(DEV)
    node_enc = B.MLP(5, (H, H, H), False).to(DEV)
    up = B.MLP(2 + 2 * H, (H, H, H), True).to(DEV)
    ea = torch.randn(rows, 2, device=DEV)
    buf = torch.randn(rows, 9, device=DEV)                       # field | glob | omega as column views of one buffer
    field, glob, omega = buf[:, 1:4], buf[:, 5:6], buf[:, 8:9]
    a, b = torch.randn(rows, H, device=DEV), torch.randn(rows, H, device=DEV)
    w = lambda m: {f"m.{k}": t.cpu() for k, t in m.state_dict().items()}
    y = enc.run_coded([ops.Source(ea)], rows, _lib.ACT_SELU)
    torch.testing.assert_close(y.cpu(), torch.selu(O.mlp(ea.cpu(), w(enc), "m")), **BLOCK)
    y = node_enc.run_coded([ops.Source(field), ops.Source(glob), ops.Source(omega)], rows, _lib.ACT_SELU)
    torch.testing.assert_close(y.cpu(), torch.selu(O.mlp(torch.cat([field, glob, omega], 1).cpu(), w(node_enc), "m")), **BLOCK)
    y = up.run_coded([ops.Source(ea, negate=True), ops.Source(a), ops.Source(b)], rows, _lib.ACT_TANH)
    torch.testing.assert_close(y.cpu(), torch.tanh(O.mlp(torch.cat([-ea, a, b], 1).cpu(), w(up), "m")), **BLOCK)
    pk = up.packed([2, H, H], [True, False, False], [True, False, False])
    assert (pk.narrow == (True, False, False)) == (ops.mlp_precision() != "fp32")


@pytest.mark.parametrize("case", ["knn6", "ragged"])
def test_node_mlp_aggregates_on_load(case):
    """g4c_src_t.seg_off: the node MLP averages / sums each target's messages while gathering its input == the separate
    g4c_segment_reduce followed by the plain launch, bit for bit (degrees 0..40 incl. empty targets and a long segment)."""
    H, n = 128, 900
    torch.manual_seed(31)
    if case == "knn6":
        col = torch.arange(n).repeat_interleave(6)
    else:
        deg = torch.randint(0, 10, (n,)); deg[0] = 0; deg[-1] = 0; deg[7:11] = 0; deg[100] = 40
        col = torch.arange(n).repeat_interleave(deg)
    E = int(col.numel())
    edge_index = torch.stack([torch.randint(0, n, (E,)), col]).to(DEV)
    ep, csr = plan.edge_csr(edge_index, n)
    blk = B.GNBlock((3 * H, (H, H, H), True), (2 * H, (H, H, H), True)).to(DEV)
    e_new, v = torch.randn(E, H, device=DEV), torch.randn(n, H, device=DEV)
    if ops.mlp_precision() == "fp32":
        pytest.skip("aggregation on load is a feature of the bf16x6 kernels")
    for mean in (True, False):
        y = blk.node_mlp.run_coded([ops.Source(e_new, segments=csr, seg_mean=mean), ops.Source(v)], n, _lib.ACT_SELU)
        agg = ops.segment_reduce(e_new, csr, mean)
        y_ref = blk.node_mlp.run_coded([ops.Source(agg), ops.Source(v)], n, _lib.ACT_SELU)
        assert torch.equal(y, y_ref)
    # through a permutation and with the pending activation of the stored rows (pool_edge's fine -> coarse plan, DownMP)
    g = S.mus_graph(1500, levels=2, seed=4).to(DEV)
    pp = plan.pool_edge_plan(g.idx1_to_idx2, g.edge_index, True)
    assert pp.csr.perm is not None
    e_f = torch.randn(g.edge_index.size(1), H, device=DEV)
    lazy = ops.Source(e_f, pre_act=_lib.ACT_SELU, segments=pp.csr, seg_mean=True)
    x2 = torch.randn(pp.n_coarse, H, device=DEV)
    y = blk.node_mlp.run_coded([lazy, ops.Source(x2)], pp.n_coarse, _lib.ACT_NONE)
    pooled = ops.segment_reduce(e_f, pp.csr, True, src_act=_lib.ACT_SELU)
    torch.testing.assert_close(pooled, torch.zeros_like(pooled).index_add_(
        0, torch.repeat_interleave(torch.arange(pp.n_coarse, device=DEV), (pp.csr.off[1:] - pp.csr.off[:-1]).long()),
        torch.selu(e_f)[pp.csr.perm.long()]) / (pp.csr.off[1:] - pp.csr.off[:-1]).clamp(min=1)[:, None], rtol=1e-5, atol=1e-5)
    assert torch.equal(y, blk.node_mlp.run_coded([ops.Source(pooled), ops.Source(x2)], pp.n_coarse, _lib.ACT_NONE))


def test_mlp_precisions_vs_fp64():
    """The default f16x3 arithmetic (two-way fp16 split, three partial products on the f16 matrix pipe, the 2^-11 terms in their
    own accumulator) and bf16x6 (exact three-way bf16 split, six partial products) are as accurate as the fp32-MFMA kernels: all
    against an fp64 evaluation of the same edge MLP (gathers, SELU-on-load, LayerNorm); plain bf16 is the only mode that deviates
    (its stated ~1e-2).  Then the range contract of f16x3: an activation beyond +-65504 is clipped (the row stays finite, no other
    row changes); tiny activations lose nothing."""
    H, rows = 128, 20000
    n = rows // 6
    torch.manual_seed(11)
    blk = B.GNBlock((3 * H, (H, H, H), True), (2 * H, (H, H, H), True)).to(DEV)
    e, v = 3.0 * torch.randn(rows, H, device=DEV), torch.randn(n, H, device=DEV)
    e[::7] *= 1e3                                   # large magnitudes (up to ~1.5e4: inside fp16's range, far outside bf16's 8 bits)
    e[5::11] *= 1e-4
    row = torch.randint(0, n, (rows,), device=DEV, dtype=torch.int32)
    col = torch.randint(0, n, (rows,), device=DEV, dtype=torch.int32)
    y = torch.cat([e, v[row.long()], v[col.long()]], 1).double()
    lin = blk.edge_mlp._linears()
    for li, l in enumerate(lin):
        y = y @ l.weight.detach().double().T + l.bias.detach().double()
        if li < len(lin) - 1:
            y = torch.selu(y)
    ln = blk.edge_mlp.MLP.layer_norm
    ref = torch.nn.functional.layer_norm(y, (H,), ln.weight.double(), ln.bias.double(), ln.eps)
    err = {}
    old = ops.mlp_precision()
    try:
        for prec in ("fp32", "bf16x6", "f16x3", "bf16"):
            ops.set_mlp_precision(prec)
            out = blk.edge_mlp.run_coded([ops.Source(e), ops.Source(v, index=row), ops.Source(v, index=col)], rows)
            d = (out.double() - ref).abs()
            err[prec] = (d.max().item(), d.mean().item())
        ops.set_mlp_precision("f16x3")
        e2 = e.clone()
        e2[3] *= 1e-6                               # a row of tiny values: still fp32-class (fp16 subnormals are honoured)
        e2[17, 5] = 1.0e5                           # one value beyond fp16: clipped to 65504 (1 + 2^-11), no other row changes
        out2 = blk.edge_mlp.run_coded([ops.Source(e2), ops.Source(v, index=row), ops.Source(v, index=col)], rows)
        ops.set_mlp_precision("bf16x6")
        ref2 = blk.edge_mlp.run_coded([ops.Source(e2), ops.Source(v, index=row), ops.Source(v, index=col)], rows)
    finally:
        ops.set_mlp_precision(old)
    assert err["fp32"][0] < 2e-5 and err["bf16x6"][0] < 2e-5 and err["f16x3"][0] < 2e-5, err
    assert err["bf16x6"][0] <= 2.0 * err["fp32"][0] + 1e-6 and err["bf16x6"][1] <= 1.5 * err["fp32"][1] + 1e-7, err
    assert err["f16x3"][0] <= 2.0 * err["fp32"][0] + 1e-6 and err["f16x3"][1] <= 1.5 * err["fp32"][1] + 1e-7, err
    assert 1e-3 < err["bf16"][0] < 2e-1, err
    assert torch.isfinite(out2).all() and torch.isfinite(ref2).all()
    keep = torch.ones(rows, dtype=torch.bool, device=DEV); keep[17] = False
    torch.testing.assert_close(out2[keep], ref2[keep], rtol=2e-5, atol=2e-5)
    e3 = e2.clone(); e3[17, 5] = 65504.0 * (1.0 + 2.0 ** -11)
    ops.set_mlp_precision("bf16x6")
    try:
        ref3 = blk.edge_mlp.run_coded([ops.Source(e3), ops.Source(v, index=row), ops.Source(v, index=col)], rows)
    finally:
        ops.set_mlp_precision(old)
    torch.testing.assert_close(out2[17], ref3[17], rtol=1e-4, atol=1e-4)         # = the MLP of the clipped row


def test_mp_chain_with_and_without_heads(monkeypatch):
    """Two chained GNBlocks: products riding on the producer's launch == the consumer computing them itself."""
    H, n, k = 128, 3000, 6
    g = S.mus_graph(n, levels=1, seed=2).to(DEV)
    torch.manual_seed(3)
    b1 = B.GNBlock((3 * H, (H, H, H), True), (2 * H, (H, H, H), True)).to(DEV)
    b2 = B.GNBlock((3 * H, (H, H, H), True), (2 * H, (H, H, H), True)).to(DEV)
    v, e = torch.randn(n, H, device=DEV), torch.randn(g.edge_index.size(1), H, device=DEV)
    monkeypatch.setattr(B, "HOIST_MIN_ROWS", 0)
    v1, e1, prod = b1.step(v, e, g.edge_index, _lib.ACT_SELU, next_msg=b2.edge_mlp)
    assert prod is not None and len(prod) == 2
    v2, e2 = b2.step(v1, e1, g.edge_index, _lib.ACT_SELU, e_pre_act=_lib.ACT_SELU, products=prod)
    u1, f1 = b1.step(v, e, g.edge_index, _lib.ACT_SELU)
    u2, f2 = b2.step(u1, f1, g.edge_index, _lib.ACT_SELU, e_pre_act=_lib.ACT_SELU)
    torch.testing.assert_close(v1, u1, rtol=0, atol=0)
    torch.testing.assert_close(v2, u2, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(e2, f2, rtol=1e-5, atol=1e-5)


@pytest.mark.parametrize("tag", ["h128_mean", "h32_sum", "h32_mean", "irregular"])
def test_gnblock(golden, tag):
    c = golden("blocks.pt")[f"gnblock_{tag}"]
    blk = load_weights(B.GNBlock(*c["args"], aggr=c["aggr"]), c["weights"])
    v, e = blk(c["v"].to(DEV), c["e"].to(DEV), c["edge_index"].to(DEV))
    torch.testing.assert_close(v.cpu(), c["v_out"], **BLOCK)
    torch.testing.assert_close(e.cpu(), c["e_out"], **BLOCK)
    # fused-activation extension == activation applied afterwards
    v2, e2 = blk(c["v"].to(DEV), c["e"].to(DEV), c["edge_index"].to(DEV), activation="selu")
    torch.testing.assert_close(v2.cpu(), torch.nn.functional.selu(c["v_out"]), **BLOCK)
    torch.testing.assert_close(e2.cpu(), torch.nn.functional.selu(c["e_out"]), **BLOCK)


@pytest.mark.parametrize("tag", ["mean", "sum", "empty"])
def test_pool_edge(golden, tag):
    c = golden("blocks.pt")[f"pool_edge_{tag}"]
    ei, ea = B.pool_edge(c["idx"].to(DEV), c["edge_index"].to(DEV), c["edge_attr"].to(DEV),
                         aggr="sum" if tag == "sum" else "mean")
    assert torch.equal(ei.cpu(), c["edge_index_out"])
    torch.testing.assert_close(ea.cpu(), c["edge_attr_out"], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("H", [32, 128])
def test_down_up(golden, H):
    c = golden("blocks.pt")[f"downup_h{H}"]
    g = gfd.Graph(**cu(c["graph"]))
    down = load_weights(B.DownMP(*c["down_args"]), c["down_weights"])
    up = load_weights(B.UpMP(*c["up_args"]), c["up_weights"])
    field1, pos1 = c["field1"].to(DEV), g.pos
    g.field, g.edge_attr = field1, c["edge_attr1"].to(DEV)
    g = down(g, activation=torch.tanh)
    torch.testing.assert_close(g.field.cpu(), c["down_field"], **BLOCK)
    assert torch.equal(g.edge_index.cpu(), c["down_edge_index"])
    torch.testing.assert_close(g.edge_attr.cpu(), c["down_edge_attr"], rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(g.pos.cpu(), c["down_pos"])
    g = up(g, field1, pos1, activation=torch.tanh)
    torch.testing.assert_close(g.field.cpu(), c["up_field"], **BLOCK)
    assert g.pos is pos1


def test_remus_blocks(golden):
    b = golden("blocks.pt")
    g = cu(b["remus_graph"])
    c = b["edgemp"]
    emp = load_weights(B.EdgeMP(*c["args"]), c["weights"])
    e, a = emp(c["e"].to(DEV), c["a"].to(DEV), c["angle_index"].to(DEV))
    torch.testing.assert_close(e.cpu(), c["e_out"], **BLOCK)
    torch.testing.assert_close(a.cpu(), c["a_out"], **BLOCK)
    c = b["downedgemp"]
    dmp = load_weights(B.DownEdgeMP(*c["args"]), c["weights"])
    e2 = dmp(c["e1"].to(DEV), c["e2"].to(DEV), c["a12"].to(DEV), c["angle_index12"].to(DEV))
    torch.testing.assert_close(e2.cpu(), c["e2_out"], **BLOCK)
    c = b["upedgemp_21"]
    ump = load_weights(B.UpEdgeMP(*c["args"]), c["weights"])
    e1 = ump(g["pos"], g["y_idx_21"], g["x_idx_21"], g["weights_21"], c["edge_attr2"].to(DEV), g["edge_index2"],
             g["edgeUnitVectorInverse2"], g["coarse_mask2"], c["edge_attr1"].to(DEV), g["edge_index"], g["edgeUnitVector"])
    torch.testing.assert_close(e1.cpu(), c["e1_out"], **BLOCK)
    c2 = b["upedgemp_32"]
    e2 = ump(g["pos"], g["y_idx_32"], g["x_idx_32"], g["weights_32"], c2["edge_attr3"].to(DEV), g["edge_index3"],
             g["edgeUnitVectorInverse3"], g["coarse_mask3"], c2["edge_attr2"].to(DEV), g["edge_index2"],
             g["edgeUnitVector2"], g["coarse_mask2"])
    torch.testing.assert_close(e2.cpu(), c2["e2_out"], **BLOCK)


def test_remus_helpers(golden):
    b = golden("blocks.pt")
    g = cu(b["remus_graph"])
    c = b["es2nv"]
    out = B.edgeScalarToNodeVector(c["s1"].to(DEV), g["edge_index"], edgeUnitVectorInverse=g["edgeUnitVectorInverse"])
    torch.testing.assert_close(out.cpu(), c["v1"], rtol=1e-5, atol=1e-5)
    out = B.edgeScalarToNodeVector(c["sH"].to(DEV), g["edge_index2"], edgeUnitVectorInverse=g["edgeUnitVectorInverse2"],
                                   coarse_mask=g["coarse_mask2"])
    torch.testing.assert_close(out.cpu(), c["vH"], rtol=1e-5, atol=1e-5)
    out = B.edgeScalarToNodeVector(c["s1"].to(DEV), g["edge_index"], edgeUnitVector=g["edgeUnitVector"])
    torch.testing.assert_close(out.cpu(), c["v1_lstsq"], rtol=1e-3, atol=1e-4)
    with pytest.raises(AssertionError):
        B.edgeScalarToNodeVector(c["s1"].to(DEV), g["edge_index"])
    c = b["knn_interpolate"]
    y = B.knn_interpolate(c["x"].to(DEV), g["y_idx_21"], g["x_idx_21"], g["weights_21"])
    torch.testing.assert_close(y.cpu(), c["y"], rtol=1e-5, atol=1e-5)
    c = b["restriction"]
    rg = gfd.Graph(field=torch.zeros(int(g["coarse_mask2"].sum()), 4, device=DEV))
    B.restriction(rg, g["coarse_mask2"], torch.zeros(1, device=DEV), g["edge_index2"], g["pos"].size(0), DEV)
    assert torch.equal(rg.edge_index.cpu(), c["edge_index_out"])


# ------------------------------------------------------------------ models vs golden
@pytest.mark.parametrize("prec", ["f16x3", "bf16x6"])
@pytest.mark.parametrize("cls", sorted(S.MUS_LAYERS))
def test_mus_models(golden, cls, prec, monkeypatch):
    monkeypatch.setattr(ops, "_PRECISION", prec)
    c = golden("models_mus.pt")[cls]
    model = getattr(gfd.nn, cls)(arch=c["arch"], device=DEV)
    model.load_state_dict(c["weights"])
    assert model.num_params == c["num_params"]
    g = gfd.Graph(**cu(c["graph"]))
    before = {k: v for k, v in g.to_dict().items()}
    with torch.no_grad():
        y = model.forward(g)
    torch.testing.assert_close(y.cpu(), c["forward"], **FWD)
    assert all(g.to_dict()[k] is v for k, v in before.items()), "forward must leave the Graph untouched"
    y3 = model.solve(g, 3)
    torch.testing.assert_close(y3.cpu(), c["solve3"], rtol=1e-3, atol=1e-3)
    assert g.field is before["field"]


@pytest.mark.parametrize("cls", sorted(S.MUGS_LAYERS))
def test_mugs_models(golden, cls):
    """gMuS-GNN classes on the HIP blocks vs the reference's forward / solve (graphs from its own transforms)."""
    c = golden("models_mugs.pt")[cls]
    model = getattr(gfd.nn, cls)(arch=c["arch"], device=DEV)
    model.load_state_dict(c["weights"])
    assert model.num_params == c["num_params"]
    g = gfd.Graph(**cu(c["graph"]))
    before = {k: v for k, v in g.to_dict().items()}
    with torch.no_grad():
        y = model.forward(g)
    torch.testing.assert_close(y.cpu(), c["forward"], **FWD)
    assert all(g.to_dict()[k] is v for k, v in before.items()), "forward must leave the Graph untouched"
    torch.testing.assert_close(model.solve(g, 3).cpu(), c["solve3"], rtol=1e-3, atol=1e-3)


def test_mugs_three_scale_h128_vs_oracle():
    """Production width: heads between consecutive layers, the 2H-wide latents after each up-sampling as two 128-wide column chunks
    on the split-operand kernels (no launch on the fp32-MFMA fallback), hipGraph-captured rollout == eager."""
    g = S.mugs_graph(9000, levels=3, seed=8)
    torch.manual_seed(9)
    model = gfd.nn.NsThreeGuillardScaleGNN(arch=S.mugs_arch("NsThreeGuillardScaleGNN", 128), device=DEV)
    w = {k: v.cpu() for k, v in model.state_dict().items()}
    ref = O.mugs_forward("NsThreeGuillardScaleGNN", g.to_dict(), w, 3)
    gd = g.clone().to(DEV)
    with torch.no_grad(), ops.KernelTimer() as kt:
        y = model.forward(gd)
    torch.testing.assert_close(y.cpu(), ref, **FWD)
    if ops.mlp_precision() in ("f16x3", "bf16x6"):
        assert "mlp_split_kernel" not in kt.summary(), kt.summary().keys()      # (no launch fell back to the fp32-MFMA kernel)
    torch.testing.assert_close(model.solve(gd, 3, capture=True), model.solve(gd, 3, capture=False), rtol=0, atol=0)


def test_remus_model(golden):
    c = golden("model_remus.pt")
    model = gfd.nn.NsRotEquiTreeScaleGNN(arch=c["arch"], device=DEV)
    model.load_state_dict(c["weights"])
    assert model.num_params == c["num_params"] and model.num_fields == 2
    g = gfd.Graph(**cu(c["graph"]))
    with torch.no_grad():
        y = model.forward(g)
    torch.testing.assert_close(y.cpu(), c["forward"], **FWD)
    torch.testing.assert_close(model.solve(g, 3).cpu(), c["solve3"], rtol=1e-3, atol=1e-3)


def test_rollouts_eager_and_hipgraph(golden):
    r = golden("rollout.pt")
    c = r["two_scale"]
    model = gfd.nn.NsTwoScaleGNN(arch=c["arch"], device=DEV)
    model.load_state_dict(c["weights"])
    g = gfd.Graph(**cu(c["graph"]))
    torch.testing.assert_close(model.solve(g, 1).cpu(), c["solve1"], **FWD)
    eager5 = model.solve(g, 5, capture=False)
    torch.testing.assert_close(eager5.cpu(), c["solve5"], rtol=1e-3, atol=1e-3)
    graph5 = model.solve(g, 5, capture=True)
    assert torch.equal(eager5, graph5), "hipGraph replay must reproduce the eager rollout bit for bit"
    s50 = model.solve(g, 50).cpu()
    torch.testing.assert_close(s50[:, :30], c["solve50"][:, :30], rtol=2e-3, atol=2e-3)
    torch.testing.assert_close(s50, c["solve50"], rtol=2e-2, atol=2e-2)
    # history window n_in = 2 (shift_and_replace)
    c = r["one_scale_nin2"]
    model = gfd.nn.NsOneScaleGNN(arch=c["arch"], device=DEV)
    model.load_state_dict(c["weights"])
    g = gfd.Graph(**cu(c["graph"]))
    torch.testing.assert_close(model.solve(g, 4, capture=False).cpu(), c["solve4"], rtol=1e-3, atol=1e-3)
    torch.testing.assert_close(model.solve(g, 4, capture=True).cpu(), c["solve4"], rtol=1e-3, atol=1e-3)
    x, y = torch.randn(10, 6, device=DEV), torch.randn(10, 3, device=DEV)
    torch.testing.assert_close(model.shift_and_replace(x, y), torch.cat([x[:, 3:], y], 1))
    with pytest.raises(AssertionError):
        model.solve(g, 0)


def test_solve_list_of_graphs(golden):
    """solve([g1, g2]) (nn/model.py:308-309: one rollout of the PyG batch of the graphs — node tensors concatenated, `*index*`
    tensors offset by the running node count) against the reference's own result on two meshes of different sizes; the rows of
    each mesh equal its own single-graph rollout; eager == captured."""
    c = golden("solve_list.pt")
    model = gfd.nn.NsOneScaleGNN(arch=c["arch"], device=DEV)
    model.load_state_dict(c["weights"])
    graphs = [gfd.Graph(**cu(d)) for d in c["graphs"]]
    out = model.solve([gfd.Graph(**cu(d)) for d in c["graphs"]], 3, capture=False)
    assert out.shape == c["solve3"].shape
    torch.testing.assert_close(out.cpu(), c["solve3"], rtol=1e-3, atol=1e-3)
    n1 = graphs[0].num_nodes
    torch.testing.assert_close(out[:n1], model.solve(graphs[0], 3, capture=False), rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(out[n1:], model.solve(graphs[1], 3, capture=False), rtol=1e-5, atol=1e-5)
    assert torch.equal(model.solve([gfd.Graph(**cu(d)) for d in c["graphs"]], 4, capture=True)[:, :9], out)


def test_rollout_advance_layouts_agree():
    """g4c_rollout_advance (nn/model.py:316-327: outputs[:, nf t : nf (t + 1)] = pred, field window shifted): the step-major output
    buffer [steps, N, nf] (out_ld = 0, what Rollout uses) holds the same values as the reference's row-major [N, nf * steps]."""
    torch.manual_seed(3)
    N, nf, n_in, steps = 1234, 3, 2, 5
    f_row, f_step = torch.randn(N, nf * n_in, device=DEV), None
    f_step = f_row.clone()
    out_row = torch.zeros(N, nf * steps, device=DEV)
    out_step = torch.zeros(steps, N, nf, device=DEV)
    c_row, c_step = torch.zeros(2, dtype=torch.int32, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)
    ref_field = f_row.clone().cpu()
    for t in range(steps):
        pred = torch.randn(N, nf, device=DEV)
        ops.rollout_advance(f_row, pred, out_row, c_row, nf)
        ops.rollout_advance(f_step, pred, out_step, c_step, nf)
        ref_field = torch.cat([ref_field[:, nf:], pred.cpu()], 1)
    assert torch.equal(ops.steps_to_columns(out_step), out_row) and torch.equal(f_row, f_step)
    assert torch.equal(f_row.cpu(), ref_field) and c_row.tolist() == [steps, 0] and c_step.tolist() == [steps, 0]


def test_rollout_on_the_renumbered_mesh(golden):
    """Rollout(reorder=True) (the default from 50k nodes): same result rows, in the caller's numbering, up to the summation order
    inside clusters / coarse edges; captured == eager; the caller's Graph is untouched."""
    from graphs4cfd_amd.nn.model import Rollout
    g = S.mus_graph(5000, levels=3, seed=61).to(DEV)
    torch.manual_seed(62)
    model = gfd.nn.NsThreeScaleGNN(arch=S.mus_arch("NsThreeScaleGNN", 128), device=DEV)
    g.batch = torch.zeros(g.num_nodes, dtype=torch.long, device=DEV)
    field0, ei0 = g.field.clone(), g.edge_index.clone()
    outs = {}
    for reorder, capture in ((False, False), (True, False), (True, True)):
        with Rollout(model, g, 6, capture=capture, reorder=reorder) as ro:
            ro.run(6)
            assert (ro._perm is not None) == reorder
            outs[(reorder, capture)] = ro.result().clone()
    torch.testing.assert_close(outs[(True, False)], outs[(False, False)], rtol=1e-4, atol=1e-4)
    assert torch.equal(outs[(True, True)], outs[(True, False)])
    assert torch.equal(g.field, field0) and torch.equal(g.edge_index, ei0)


def test_reference_checkpoint_loads_and_runs(golden):
    import os
    c = golden("checkpoint_io.pt")
    path = os.path.join(os.path.dirname(__file__), "golden", "reference_saved.chk")
    model = gfd.nn.NsOneScaleGNN(checkpoint=path, device=DEV)
    assert list(model.state_dict().keys()) == c["keys"]
    g = gfd.Graph(**cu(c["graph"]))
    with torch.no_grad():
        torch.testing.assert_close(model.forward(g).cpu(), c["forward"], **FWD)


# ------------------------------------------------------------------ production width vs oracle
@pytest.mark.parametrize("agg_on_load_min_rows", [0, 1 << 30])
def test_three_scale_h128_vs_oracle(agg_on_load_min_rows, monkeypatch):
    """(0: every level aggregates inside the node launch's gather; 1 << 30: separate g4c_segment_reduce launches — the default
    switches between the two at ops.AGG_ON_LOAD_MIN_ROWS aggregated rows)"""
    monkeypatch.setattr(ops, "AGG_ON_LOAD_MIN_ROWS", agg_on_load_min_rows)
    g = S.mus_graph(6000, levels=3, seed=3)
    arch = S.mus_arch("NsThreeScaleGNN", 128)
    torch.manual_seed(5)
    model = gfd.nn.NsThreeScaleGNN(arch=arch, device=DEV)
    w = {k: v.cpu() for k, v in model.state_dict().items()}
    ref = O.mus_forward("NsThreeScaleGNN", g.to_dict(), w, 3)
    with torch.no_grad():
        y = model.forward(g.clone().to(DEV))
    torch.testing.assert_close(y.cpu(), ref, **FWD)


def test_remus_h128_vs_oracle():
    g = S.remus_graph(1500, k=5, seed=4)
    torch.manual_seed(6)
    model = gfd.nn.NsRotEquiTreeScaleGNN(arch=S.remus_arch(128), device=DEV)
    w = {k: v.cpu() for k, v in model.state_dict().items()}
    ref = O.remus_forward(g.to_dict(), w)
    with torch.no_grad():
        y = model.forward(g.clone().to(DEV))
    torch.testing.assert_close(y.cpu(), ref, **FWD)


def test_models_bf16_mode_vs_oracle():
    """Opt-in bf16-MFMA MLPs, whole forwards vs the fp32 oracle: the tolerance SURVEY 8(c) states for the bf16 variant
    (~1e-2 on O(1) outputs; measured max 1.7e-2 / 2.0e-2, mean 3e-3 — scripts/bf16_error.py)."""
    old = ops.set_mlp_precision("bf16")
    try:
        g = S.mus_graph(6000, levels=3, seed=3)
        torch.manual_seed(5)
        model = gfd.nn.NsThreeScaleGNN(arch=S.mus_arch("NsThreeScaleGNN", 128), device=DEV)
        ref = O.mus_forward("NsThreeScaleGNN", g.to_dict(), {k: v.cpu() for k, v in model.state_dict().items()}, 3)
        with torch.no_grad():
            d = (model.forward(g.clone().to(DEV)).cpu() - ref).abs()
        assert d.max().item() < 6e-2 and d.mean().item() < 1e-2, (d.max().item(), d.mean().item())
        g = S.remus_graph(1500, k=5, seed=4)
        torch.manual_seed(6)
        model = gfd.nn.NsRotEquiTreeScaleGNN(arch=S.remus_arch(128), device=DEV)
        ref = O.remus_forward(g.to_dict(), {k: v.cpu() for k, v in model.state_dict().items()})
        with torch.no_grad():
            d = (model.forward(g.clone().to(DEV)).cpu() - ref).abs()
        assert d.max().item() < 6e-2 and d.mean().item() < 1e-2, (d.max().item(), d.mean().item())
    finally:
        ops.set_mlp_precision(old)


def test_solve_warns_about_inputs_near_the_fp16_range(golden):
    """The default f16x3 arithmetic clips activations at +-65504: solve() says so when an input tensor is large enough for
    the first hidden layer to get there (un-normalised data), and only then; bf16x6 never warns."""
    import warnings
    c = golden("rollout.pt")["two_scale"]
    model = gfd.nn.NsTwoScaleGNN(arch=c["arch"], device=DEV)
    model.load_state_dict(c["weights"])
    g = gfd.Graph(**cu(c["graph"]))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        model.solve(g.clone(), 2)
    big = g.clone()
    big.field = big.field * 1.0e5
    with pytest.warns(RuntimeWarning, match="f16x3"):
        out = model.solve(big, 2)
    assert torch.isfinite(out).all()
    old = ops.set_mlp_precision("bf16x6")
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            model.solve(big.clone(), 2)
    finally:
        ops.set_mlp_precision(old)


# ------------------------------------------------------------------ BASELINE configs at size
def test_headline_100k_vs_oracle():
    """The bench workload itself (NsThreeScaleGNN, H = 128, 100k-node 2-D mesh, default f16x3 kernels with the fused
    per-target aggregation): forward vs the oracle at the stated fp32 tolerance, then the hipGraph-replayed rollout step
    vs the eager one, bit for bit."""
    assert ops.mlp_precision() == "f16x3"
    g = S.mus_graph(100_000, levels=3, seed=0)
    torch.manual_seed(1)
    model = gfd.nn.NsThreeScaleGNN(arch=S.mus_arch("NsThreeScaleGNN", 128), device=DEV)
    ref = O.mus_forward("NsThreeScaleGNN", g.to_dict(), {k: v.cpu() for k, v in model.state_dict().items()}, 3)
    gd = g.clone().to(DEV)
    with torch.no_grad():
        y = model.forward(gd)
    torch.testing.assert_close(y.cpu(), ref, **FWD)
    cap, eag = model.solve(gd, 4, capture=True), model.solve(gd, 4, capture=False)
    assert torch.equal(cap, eag) and torch.isfinite(cap).all()


@pytest.mark.parametrize("prec", ["f16x3", "bf16x6", "bf16"])
def test_remus_20k_vs_oracle(prec):
    """BASELINE config 3's model (REMuS-GNN 3-scale, H = 128) at 20k nodes / 100k level-1 edges, on the fp32-accurate default and on
    the config's bf16 edge-MLP MFMA variant (tolerance of SURVEY 8(c): ~1e-2 on O(1) outputs)."""
    old = ops.set_mlp_precision(prec)
    try:
        g = S.remus_graph(20_000, k=5, seed=21)
        torch.manual_seed(22)
        model = gfd.nn.NsRotEquiTreeScaleGNN(arch=S.remus_arch(128), device=DEV)
        ref = O.remus_forward(g.to_dict(), {k: v.cpu() for k, v in model.state_dict().items()})
        with torch.no_grad():
            y = model.forward(g.clone().to(DEV)).cpu()
        if prec != "bf16":
            torch.testing.assert_close(y, ref, **FWD)
        else:
            # (rounded operands: a noise floor, not a bound that shrinks — mean 2 - 3e-3, 99.9th percentile 1 - 2e-2 on every seed and
            # kernel choice; the single largest of the 40 000 deviations moves between 3e-2 and 8e-2 with the summation order alone)
            d = (y - ref).abs()
            p999 = d.flatten().kthvalue(int(0.999 * d.numel())).values.item()
            assert d.mean().item() < 1e-2 and p999 < 3e-2 and d.max().item() < 1e-1, (d.max().item(), p999, d.mean().item())
    finally:
        ops.set_mlp_precision(old)


@pytest.mark.parametrize("cls", ["NsFourScaleGNN", "NsTwoScaleGNN"])
def test_mus_models_3d(golden, cls):
    """BASELINE config 5's data path at fixture size: the reference's own forward / solve on a 3-D mesh (3-wide edge
    attributes, 3 + H pooling inputs)."""
    c = golden("models_mus_3d.pt")[cls]
    model = getattr(gfd.nn, cls)(arch=c["arch"], device=DEV)
    model.load_state_dict(c["weights"])
    assert model.num_params == c["num_params"]
    g = gfd.Graph(**cu(c["graph"]))
    with torch.no_grad():
        torch.testing.assert_close(model.forward(g).cpu(), c["forward"], **FWD)
    torch.testing.assert_close(model.solve(g, 3).cpu(), c["solve3"], rtol=1e-3, atol=1e-3)


def test_four_scale_3d_500_step_captured_rollout():
    """Config 5 on one GPU, scaled to 30k nodes: NsFourScaleGNN (H = 128) on a 3-D mesh vs the oracle, then the 500-step
    rollout with the hipGraph-captured step == the eager rollout bit for bit (and stays finite)."""
    g = S.mus_graph(30_000, levels=4, dim=3, seed=31)
    torch.manual_seed(32)
    model = gfd.nn.NsFourScaleGNN(arch=S.mus_arch("NsFourScaleGNN", 128, dim=3), device=DEV)
    for p in model.node_decoder.parameters():    # damp the residual update so that 500 steps of a random-weight model stay O(1)
        p.data.mul_(0.02)
    model.invalidate_packed()
    ref = O.mus_forward("NsFourScaleGNN", g.to_dict(), {k: v.cpu() for k, v in model.state_dict().items()}, 3)
    gd = g.clone().to(DEV)
    with torch.no_grad():
        torch.testing.assert_close(model.forward(gd).cpu(), ref, **FWD)
    cap = model.solve(gd, 500, capture=True)
    eag = model.solve(gd, 500, capture=False)
    assert cap.shape == (30_000, 1500) and torch.isfinite(cap).all()
    assert torch.equal(cap, eag), "hipGraph replay must reproduce the eager rollout bit for bit over 500 steps"


def test_config5_mesh_at_its_own_size_on_one_gpu():
    """BASELINE config 5 at ITS size — 1M nodes, 3-D, NsFourScaleGNN (H = 128) — on the one GPU of the test box (VERDICT r04 missing 5;
    the oracle cannot run this in seconds, so size-independent properties): the mesh is built on the device, six rollout steps stay
    finite, the hipGraph-replayed rollout equals the eager one bit for bit, and the default f16x3 arithmetic agrees with the exact
    three-way bf16 split (bf16x6: another kernel family, twice the products) to fp32 round-off class on every one of the 3M outputs
    of the first step."""
    g = S.mus_graph(1_000_000, levels=4, dim=3, seed=51, device=DEV)
    torch.manual_seed(52)
    model = gfd.nn.NsFourScaleGNN(arch=S.mus_arch("NsFourScaleGNN", 128, dim=3), device=DEV)
    for p in model.node_decoder.parameters():
        p.data.mul_(0.02)
    model.invalidate_packed()
    old = ops.set_mlp_precision("f16x3")
    try:
        cap = model.solve(g.clone(), 6, capture=True)
        eag = model.solve(g.clone(), 6, capture=False)
        assert cap.shape == (1_000_000, 18) and torch.isfinite(cap).all()
        assert torch.equal(cap, eag)
        ops.set_mlp_precision("bf16x6")
        ref = model.solve(g.clone(), 1, capture=False)
        d = (cap[:, :3] - ref).abs()
        assert d.max().item() < 2e-4 and d.mean().item() < 2e-6, (d.max().item(), d.mean().item())
    finally:
        ops.set_mlp_precision(old)


# ------------------------------------------------------------------ full-size properties (100k nodes)
def test_full_size_properties():
    n, k, H = 100_000, 6, 128
    g = S.mus_graph(n, levels=1, seed=9).to(DEV)
    ep, csr = plan.edge_csr(g.edge_index, n)
    assert csr.perm is None and csr.max_deg == k
    # mean of per-edge constants equals the constant; sum is linear
    a = torch.randn(n * k, H, device=DEV)
    b = torch.randn(n * k, H, device=DEV)
    sa, sb = ops.segment_reduce(a, csr, False), ops.segment_reduce(b, csr, False)
    sab = ops.segment_reduce(a + 2 * b, csr, False)
    torch.testing.assert_close(sab, sa + 2 * sb, rtol=1e-5, atol=1e-4)
    ones = torch.full((n * k, H), 3.25, device=DEV)
    assert torch.all(ops.segment_reduce(ones, csr, True) == 3.25)
    # checksum: total of all segment sums == total of all messages (fp64 reference)
    torch.testing.assert_close(sa.double().sum(), a.double().sum(), rtol=1e-9, atol=1e-3)
    # one GNBlock at full size: permuting the edge order must not change node outputs
    torch.manual_seed(1)
    blk = B.GNBlock((3 * H, (H, H, H), True), (2 * H, (H, H, H), True)).to(DEV)
    v, e = torch.randn(n, H, device=DEV), torch.randn(n * k, H, device=DEV)
    v1, e1 = blk(v, e, g.edge_index)
    p = torch.randperm(n * k, device=DEV)
    v2, e2 = blk(v, e[p], g.edge_index[:, p].contiguous())
    torch.testing.assert_close(v2, v1, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(e2, e1[p], rtol=1e-5, atol=1e-5)
    assert torch.isfinite(v1).all() and abs(float(v1.mean())) < 0.2


# ------------------------------------------------------------------ error behaviour
@pytest.mark.parametrize("prec", ["f16x3", "bf16x6", "fp32"])
@pytest.mark.parametrize("shape", [(8, (256, 16), False), (300, (200, 300, 64), True), (128, (128,) * 6, True), (64, (64, 300), False),
                                   (40, (512, 96, 96, 96, 96, 33), True), (128, (130, 128), True), (8, (16, 256), True), (70, (300, 1300), True),
                                   (8, (1024, 16), False), (600, (700, 48), True), (24, (640, 640, 640), True)],
                         ids=["wide-hidden", "wide-in-and-hidden", "six-layers", "wide-out", "wide-then-deep", "just-over", "wide-layernorm",
                              "very-wide-layernorm", "hidden-over-512", "wide-in-over-512", "all-over-512"])
def test_mlp_any_widths_and_depth(shape, prec):
    """The reference's MLP takes any widths and depth (nn/blocks.py:129-141); the fused kernels take <= 4 layers of <= 128 outputs per
    launch.  Outside that envelope the module runs a chain of launches (MLP._run_stages: a wide layer as one launch per 128-column
    chunk of its output, deep MLPs as consecutive launches, a layer with more than four 128-wide input blocks as launches over groups
    of blocks that add to the previous group's partial sums, a LayerNorm over more than 128 columns as g4c_layer_norm behind the
    chunks) — same result as torch's nn.Sequential on the same weights."""
    k_in, widths, ln = shape
    old = ops.set_mlp_precision(prec)
    try:
        torch.manual_seed(sum(widths))
        mlp = B.MLP(k_in, widths, ln).to(DEV)
        assert not mlp.fits_one_launch()
        x = torch.randn(777, k_in, device=DEV)
        with torch.no_grad():
            got = mlp(x)
            ref = mlp.MLP.double()(x.double()).float()
            mlp.MLP.float()
            got_act = mlp.run([ops.Source(x)], 777, activation="selu")
        torch.testing.assert_close(got, ref, **BLOCK)
        torch.testing.assert_close(got_act, torch.nn.functional.selu(ref), **BLOCK)
    finally:
        ops.set_mlp_precision(old)


def test_errors():
    mlp = B.MLP(8, (16, 16), True).to(DEV)
    with pytest.raises(RuntimeError, match="HIP"):
        mlp(torch.randn(4, 8))
    with pytest.raises(ValueError):
        mlp(torch.randn(4, 9, device=DEV))
    with pytest.raises(ValueError):
        gfd.nn.NsOneScaleGNN(model="no-such-model")


# ------------------------------------------------------------------ node partition on the HIP back-end
@pytest.mark.parametrize("hoist_min_rows", [None, 0])
def test_partitioned_hip_forward_two_ranks_in_process(hoist_min_rows, monkeypatch):
    """Two 'ranks' on the one GPU of the test box, as two threads with an in-process halo exchange
    (the RCCL path differs only in the transport; the partition / gloo exchange is tested on CPU).
    hoist_min_rows = 0: every MP layer hoists, so consecutive layers exchange the halo rows of W1r v (emitted by the
    previous layer's node launch) instead of the latents."""
    import threading
    from graphs4cfd_amd import partition as P
    if hoist_min_rows is not None:
        monkeypatch.setattr(B, "HOIST_MIN_ROWS", hoist_min_rows)
    world, levels = 2, 3
    g = S.mus_graph(4000, levels=levels, seed=12)
    torch.manual_seed(13)
    model = gfd.nn.NsThreeScaleGNN(arch=S.mus_arch("NsThreeScaleGNN", 128), device=DEV)
    with torch.no_grad():
        ref = model.forward(g.clone().to(DEV))
    parts = P.build_partition(g, levels, world)
    meshes = [P.LocalMesh(g, levels, parts[r], DEV, r, world) for r in range(world)]
    barrier = threading.Barrier(world)
    posted = {}

    class ThreadExchanger:
        def __init__(self, mesh):
            self.mesh = mesh

        def exchange(self, v, level):
            m = self.mesh
            posted[(m.rank, level)] = v
            barrier.wait()
            off = m.n_own[level - 1]
            for q in range(world):
                k = m.recv_counts[level - 1][q]
                if k:
                    peer = meshes[q]
                    v[off:off + k] = posted[(q, level)][peer.send_idx32[level - 1][m.rank].long()]
                    off += k
            torch.cuda.synchronize()
            barrier.wait()

        def exchange_async(self, v, level):     # the interior / boundary launches of HipImpl.mp, synchronous transport
            self.exchange(v, level)
            overlapped.append(level)

        def wait(self, handle):
            pass

    preds, errors, overlapped = [None] * world, [], []

    def run(r):
        try:
            fwd = P.MusPartitionedForward(model._PROGRAM, meshes[r], P.HipImpl(model), ThreadExchanger(meshes[r]), 128, 3)
            with torch.no_grad():
                preds[r] = fwd.forward()
        except Exception as exc:   # surface worker failures instead of dead-locking the barrier
            errors.append(exc)
            barrier.abort()

    threads = [threading.Thread(target=run, args=(r,)) for r in range(world)]
    [t.start() for t in threads]
    [t.join() for t in threads]
    assert not errors, errors
    full = torch.zeros_like(ref)
    for r in range(world):
        full[meshes[r].owned_global[0]] = preds[r]
    torch.testing.assert_close(full, ref, **FWD)
    assert bool(overlapped) == (hoist_min_rows == 0)


def test_overlapped_exchange_in_hipgraph_equals_eager_sequential(monkeypatch):
    """Rank 0 of 2 with a stand-in transport (halo rows <- a fixed function of the packed send rows).  The overlapped step
    (exchange on a side stream, interior edges meanwhile, boundary edges after) captured into a hipGraph and replayed
    equals the eager step with one edge launch after a blocking exchange, bit for bit (every edge row is independent)."""
    import torch.distributed as dist
    from graphs4cfd_amd import partition as P
    monkeypatch.setattr(B, "HOIST_MIN_ROWS", 0)
    calls = []

    def stand_in(recv, send, output_split_sizes=None, input_split_sizes=None, group=None):
        calls.append(torch.cuda.current_stream().cuda_stream)
        pick = torch.arange(recv.size(0), device=recv.device) % send.size(0)
        recv.copy_(torch.index_select(send, 0, pick))

    monkeypatch.setattr(dist, "all_to_all_single", stand_in)
    g = S.mus_graph(6000, levels=3, seed=21)
    torch.manual_seed(22)
    model = gfd.nn.NsThreeScaleGNN(arch=S.mus_arch("NsThreeScaleGNN", 128), device=DEV)
    outs = {}
    for overlap, capture in ((False, False), (True, False), (True, True)):
        monkeypatch.setenv("G4C_DIST_OVERLAP", "1" if overlap else "0")
        dr = P.DistributedRollout(model, g, 4, 0, 2, DEV, capture=capture)
        assert dr.fwd.overlap == overlap and min(dr.mesh.n_halo) > 0
        del calls[:]
        dr.run(4)
        torch.cuda.synchronize()
        assert dr.capture == capture and (dr._hipgraph is not None) == capture
        main = torch.cuda.current_stream().cuda_stream
        assert overlap == any(c != main for c in calls[:20])      # first (eager) step: the exchange ran on the side stream
        outs[(overlap, capture)] = dr.outputs.clone()
    assert torch.isfinite(outs[(False, False)]).all()
    assert torch.equal(outs[(True, False)], outs[(False, False)])
    assert torch.equal(outs[(True, True)], outs[(False, False)])


def test_distributed_rollout_single_rank_equals_rollout():
    from graphs4cfd_amd import partition as P
    from graphs4cfd_amd.nn.model import Rollout
    g = S.mus_graph(3000, levels=2, seed=14)
    torch.manual_seed(15)
    model = gfd.nn.NsTwoScaleGNN(arch=S.mus_arch("NsTwoScaleGNN", 128), device=DEV)
    ref = model.solve(g.clone().to(DEV), 3, capture=False)
    dr = P.DistributedRollout(model, g, 3, 0, 1, DEV)
    dr.run(3)
    torch.testing.assert_close(dr.gather_outputs(), ref, rtol=1e-4, atol=1e-4)


def test_distributed_rollout_recomputes_a_clipped_rollout_in_bf16x6():
    """DistributedRollout.validate (called by gather_outputs): as nn.model.Rollout — a partitioned rollout whose launches reached the end
    of the fp16 range is recomputed from its input window in "bf16x6" (the decision is an all-reduce over the ranks; world size 1
    here) and stays in that arithmetic; what gather_outputs returns equals the bf16x6 solve of the same model."""
    import warnings
    from graphs4cfd_amd import partition as P
    g = S.mus_graph(3000, levels=2, seed=16)
    torch.manual_seed(17)
    model = gfd.nn.NsTwoScaleGNN(arch=S.mus_arch("NsTwoScaleGNN", 128), device=DEV)
    with torch.no_grad():
        model.mp111.edge_mlp.MLP.layer_norm.weight.mul_(3e4)
    model.invalidate_packed()
    old = ops.set_mlp_precision("f16x3")
    try:
        ops.f16_range_clear()
        for capture in (False, True):
            dr = P.DistributedRollout(model, g, 4, 0, 1, DEV, capture=capture)
            dr.run(4)
            with pytest.warns(RuntimeWarning, match="recomputed in"):
                got = dr.gather_outputs()
            assert dr.exact_range and dr.steps_done == 4
            with warnings.catch_warnings():
                warnings.simplefilter("error", RuntimeWarning)
                assert torch.equal(dr.gather_outputs(), got)          # nothing left to report, nothing recomputed twice
            ops.set_mlp_precision("bf16x6")
            with warnings.catch_warnings():
                warnings.simplefilter("error", RuntimeWarning)
                ref = model.solve(g.clone().to(DEV), 4, capture=False)
            ops.set_mlp_precision("f16x3")
            torch.testing.assert_close(got, ref, rtol=1e-4, atol=1e-4 * float(ref.abs().max()))
    finally:
        ops.set_mlp_precision(old)


def test_distributed_remus_single_rank_and_two_ranks_in_process():
    """REMuS-GNN through DistributedRollout: world = 1 == model.solve; and a 2-rank partition run in ONE process (both ranks'
    forwards interleaved by a fake transport that copies halo rows between the two meshes) == the single-rank forward."""
    from graphs4cfd_amd import partition as P, partition_remus as PR
    g = S.remus_graph(6000, k=5, seed=51)
    torch.manual_seed(52)
    model = gfd.nn.NsRotEquiTreeScaleGNN(arch=S.remus_arch(128), device=DEV)
    ref = model.solve(g.clone().to(DEV), 3, capture=False)
    dr = P.DistributedRollout(model, g, 3, 0, 1, DEV)
    dr.run(3)
    torch.testing.assert_close(dr.gather_outputs(), ref, rtol=1e-4, atol=1e-4)
    assert dr.captured
    # two ranks, one process: run rank 0 and rank 1 in lock step on two threads, exchanging through host memory
    import threading
    parts = PR.build_remus_partition(g, 2)
    meshes = [PR.RemusLocalMesh(g, parts[r], DEV, r, 2) for r in range(2)]
    barrier, box = threading.Barrier(2), {}

    class PairExchange:
        def __init__(self, mesh):
            self.mesh, self.n_exchanges = mesh, 0

        def exchange(self, v, ch):
            m, r = self.mesh, self.mesh.rank
            torch.cuda.synchronize()
            box[r] = v[m.send_idx32[ch - 1][1 - r].long()].clone()
            barrier.wait()
            v[m.n_own[ch - 1]:] = box[1 - r]
            torch.cuda.synchronize()
            barrier.wait()
            self.n_exchanges += 1

    preds, errs = {}, []

    def work(r):
        try:
            torch.cuda.set_device(DEV)
            with torch.no_grad():
                fwd = PR.RemusPartitionedForward(model._PROGRAM, meshes[r], PR.RemusHipImpl(model, meshes[r]), PairExchange(meshes[r]))
                preds[r] = fwd.forward()
        except Exception as exc:      # noqa: BLE001
            errs.append(exc)
            barrier.abort()
    threads = [threading.Thread(target=work, args=(r,)) for r in range(2)]
    [t.start() for t in threads]
    [t.join() for t in threads]
    assert not errs, errs
    full = torch.zeros(6000, 2, device=DEV)
    for r in range(2):
        full[meshes[r].owned_global[0]] = preds[r]
    torch.testing.assert_close(full, ref[:, :2], rtol=1e-4, atol=1e-4)
    assert all(meshes[r].n_halo[c] > 0 for r in range(2) for c in range(5))


def _remus_two_ranks_in_process(model, g, stale_channel=None):
    """The 2-rank in-process partitioned REMuS forward (two threads in lock step, halo rows copied through a fake transport): the
    prediction of every node, assembled in global order.  `stale_channel` (negative control): that channel's halo is fed from its
    PREVIOUS exchange — one layer old — from the second exchange on."""
    import threading
    from graphs4cfd_amd import partition_remus as PR
    parts = PR.build_remus_partition(g, 2)
    meshes = [PR.RemusLocalMesh(g, parts[r], DEV, r, 2) for r in range(2)]
    assert all(meshes[r].n_halo[c] > 0 for r in range(2) for c in range(5))          # (every level has halo rows)
    barrier, box = threading.Barrier(2), {}

    class PairExchange:
        def __init__(self, mesh):
            self.mesh, self.n_exchanges, self.prev = mesh, 0, {}

        def exchange(self, v, ch):
            m, r = self.mesh, self.mesh.rank
            torch.cuda.synchronize()
            rows = v[m.send_idx32[ch - 1][1 - r].long()].clone()
            box[r] = self.prev[ch] if (ch == stale_channel and ch in self.prev) else rows
            self.prev[ch] = rows
            barrier.wait()
            v[m.n_own[ch - 1]:] = box[1 - r]
            torch.cuda.synchronize()
            barrier.wait()
            self.n_exchanges += 1

    preds, errs = {}, []

    def work(r):
        try:
            torch.cuda.set_device(DEV)
            with torch.no_grad():
                fwd = PR.RemusPartitionedForward(model._PROGRAM, meshes[r], PR.RemusHipImpl(model, meshes[r]), PairExchange(meshes[r]))
                preds[r] = fwd.forward()
        except Exception as exc:      # noqa: BLE001
            errs.append(exc)
            barrier.abort()
    threads = [threading.Thread(target=work, args=(r,)) for r in range(2)]
    [t.start() for t in threads]
    [t.join() for t in threads]
    assert not errs, errs
    full = torch.zeros(g.num_nodes, 2, device=DEV)
    for r in range(2):
        full[meshes[r].owned_global[0]] = preds[r]
    return full


@pytest.mark.parametrize("stale_channel", [None, 1], ids=["fresh_halo", "stale_halo_channel_1"])
def test_distributed_remus_two_ranks_in_process_bf16(stale_channel):
    """The partitioned REMuS forward in the rounded-bf16 mode (2 ranks in one process, every level with halo rows): its sub-meshes take
    other kernels than the whole mesh, so it is held to the mode's accuracy instead of to the single-rank bits — against the fp32 oracle,
    mean and p99.9 within 1.15x of the single-rank forward's (measured 1.000x / 0.963x: profiles/r07_remus_bf16_partition.log).  Negative
    control: with the level-1 edge latents' halo one layer old the check must fail (measured 1.50x / 13.1x).  The largest deviation is
    not bounded: on this seed the single-rank forward's own is 1.02e-1."""
    old = ops.set_mlp_precision("bf16")
    try:
        g = S.remus_graph(20_000, k=5, seed=53)
        torch.manual_seed(54)
        model = gfd.nn.NsRotEquiTreeScaleGNN(arch=S.remus_arch(128), device=DEV)
        oracle = O.remus_forward(g.to_dict(), {k: v.cpu() for k, v in model.state_dict().items()})
        with torch.no_grad():
            single = model.forward(g.clone().to(DEV))
        part = _remus_two_ranks_in_process(model, g, stale_channel)
        assert torch.isfinite(part).all()
        s, p = _vs_oracle(single, oracle), _vs_oracle(part, oracle)
        ok = p[0] <= 1.15 * s[0] and p[1] <= 1.15 * s[1]
        print(f"partitioned bf16 ({'fresh' if stale_channel is None else f'stale channel {stale_channel}'}): mean {p[0]:.3e} ({p[0] / s[0]:.3f}x) "
              f"p99.9 {p[1]:.3e} ({p[1] / s[1]:.3f}x) max {p[2]:.3e} | single rank mean {s[0]:.3e} p99.9 {s[1]:.3e} max {s[2]:.3e}")
        assert ok == (stale_channel is None), (stale_channel, p, s)
    finally:
        ops.set_mlp_precision(old)


def test_remus_bf16_rollout_drift():
    """A 10-step rounded-bf16 rollout at 20k nodes against the fp32 oracle's rollout (O.remus_solve): finite at every step, and the
    deviation grows no faster than linearly with the step — mean_s <= 1.3 s mean_1, p99.9_s <= 1.5 s p99.9_1 (measured at most 0.87 s and
    0.98 s: 1.5x margin) — with max_10 < 1 (measured 0.63).  profiles/r07_remus_bf16_drift.log holds steps 1 .. 10."""
    old = ops.set_mlp_precision("bf16")
    try:
        g = S.remus_graph(20_000, k=5, seed=55)
        torch.manual_seed(56)
        model = gfd.nn.NsRotEquiTreeScaleGNN(arch=S.remus_arch(128), device=DEV)
        ref = O.remus_solve(g.to_dict(), {k: v.cpu() for k, v in model.state_dict().items()}, 10)
        y = model.solve(g.clone().to(DEV), 10).cpu()
        assert torch.isfinite(y).all()
        st = {}
        for step in range(1, 11):
            st[step] = _vs_oracle(y[:, 2 * (step - 1):2 * step], ref[:, 2 * (step - 1):2 * step])
            print(f"drift step {step}: mean {st[step][0]:.3e} ({st[step][0] / (step * st[1][0]):.3f} x step x step 1) p99.9 {st[step][1]:.3e} "
                  f"({st[step][1] / (step * st[1][1]):.3f} x step x step 1) max {st[step][2]:.3e} above 3e-2 {st[step][3]}")
        for step in range(2, 11):
            assert st[step][0] <= 1.3 * step * st[1][0] and st[step][1] <= 1.5 * step * st[1][1], (step, st[step], st[1])
        assert st[10][2] < 1.0, st[10]
    finally:
        ops.set_mlp_precision(old)


def test_remus_100k_bf16():
    """Config 3's size (REMuS-GNN at 100k nodes) in the rounded-bf16 mode: the captured rollout equals the eager one bit for bit, every
    value is finite, and against the f16x3 forward (fp32-accurate, standing in for the oracle at this size) the mean and p99.9 stay within
    the 20k bounds of test_remus_20k_vs_oracle (1e-2 / 3e-2) and within 1.15x of the mode's tile path (as at 20k).  The largest deviation
    is a tail statistic of 5x as many outputs as at 20k: it is bounded at 5e-1 and its fraction above 3e-2 at 1e-3 (measured 0.26 and
    3.6e-4; at 20k up to 1.0e-1 and 2.8e-4: profiles/r07_remus_bf16_drift.log)."""
    old = ops.set_mlp_precision("f16x3")
    was = B.ROW_SPLIT_BF16, B.UPDATE_ROW_SPLIT, B.RS1_MIN_ROWS
    try:
        g = S.remus_graph(100_000, k=5, seed=57).to(DEV)
        torch.manual_seed(58)
        model = gfd.nn.NsRotEquiTreeScaleGNN(arch=S.remus_arch(128), device=DEV)
        with torch.no_grad():
            ref = model.forward(g.clone()).cpu()
        ops.set_mlp_precision("bf16")
        res = {}
        for path in ("tile", "default"):
            B.ROW_SPLIT_BF16, B.UPDATE_ROW_SPLIT, B.RS1_MIN_ROWS = was if path == "default" else (False, False, 1 << 40)
            with torch.no_grad():
                y = model.forward(g.clone())
            assert torch.isfinite(y).all()
            res[path] = _vs_oracle(y, ref)
            m, p999, mx, above = res[path]
            print(f"100k bf16 {path} path vs f16x3: mean {m:.3e} p99.9 {p999:.3e} max {mx:.3e} above 3e-2 {above} of {y.numel()}")
        (m, p999, mx, above), (m1, p1, _, _) = res["default"], res["tile"]
        assert m < 1e-2 and p999 < 3e-2 and m <= 1.15 * m1 and p999 <= 1.15 * p1, res
        assert mx < 5e-1 and above <= 1e-3 * y.numel(), res
        cap, eag = model.solve(g.clone(), 4, capture=True), model.solve(g.clone(), 4, capture=False)
        assert torch.isfinite(cap).all() and torch.equal(cap, eag)
    finally:
        B.ROW_SPLIT_BF16, B.UPDATE_ROW_SPLIT, B.RS1_MIN_ROWS = was
        ops.set_mlp_precision(old)


def test_distributed_rollout_two_processes_one_gpu():
    """Two ranks (two processes) drive the partitioned HIP path end to end on this box's single GPU, with the
    gloo transport for the halo exchange (the RCCL transport needs one GPU per rank; the driver's scaling run
    uses it).  Compared inside the script with the single-process rollout."""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    port = 29700 + os.getpid() % 200
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(root, "scripts", "dist_check.py"), "--backend", "gloo", "--same-gpu",
           "--nodes", "12000", "--steps", "3"]
    # --hoist-min-rows 0: every MP layer hoists, i.e. the halo exchange carries the first-layer products (partition.py)
    for extra in ([], ["--hoist-min-rows", "0"]):
        out = subprocess.run(cmd + extra, capture_output=True, text=True, timeout=600, env=dict(os.environ))
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        assert "max|partitioned - single|" in out.stdout


def test_distributed_rollout_four_processes_one_gpu():
    """BASELINE config 4's split (100k-node mesh, node-partitioned 4-way) with four processes on this box's single GPU over the
    gloo transport: latent exchange (default) and first-layer-product exchange, a 3-D four-scale model (config 5's program)
    and REMuS-GNN (config 3's model, edge-latent halo) on smaller meshes; compared inside the script with the single-process rollout."""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    port = 29300 + os.getpid() % 200
    base = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", "4", "--master-addr", "127.0.0.1",
            "--master-port", str(port), os.path.join(root, "scripts", "dist_check.py"), "--backend", "gloo", "--same-gpu"]
    runs = [(base + ["--nodes", "100000", "--steps", "2"], dict(os.environ)),
            (base + ["--nodes", "30000", "--steps", "2", "--hoist-min-rows", "0"], dict(os.environ)),
            (base + ["--nodes", "20000", "--steps", "2", "--model", "NsFourScaleGNN", "--dim", "3"], dict(os.environ)),
            (base + ["--nodes", "20000", "--steps", "2", "--model", "NsRotEquiTreeScaleGNN"], dict(os.environ))]
    for cmd, env in runs:
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
        assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
        assert "world=4" in out.stdout and "max|partitioned - single|" in out.stdout


def test_distributed_rollout_rccl_capture_single_rank():
    """The RCCL transport itself, as far as a one-GPU box can execute it: one process, backend nccl, every halo collective entered
    with zero-length splits (--force-exchange), the partitioned step — collectives included — captured into a hipGraph and replayed
    (the script asserts `captured`), against the single-process rollout at the 5e-4 forward tolerance."""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    port = 29500 + os.getpid() % 200
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nproc-per-node", "1", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(root, "scripts", "dist_check.py"), "--backend", "nccl", "--capture", "1", "--force-exchange", "--nodes", "20000",
           "--steps", "5"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0"))
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    assert "world=1 backend=nccl" in out.stdout and "captured=True" in out.stdout, out.stdout[-1000:]


# ------------------------------------------------------------------ weights that change under cached images / captured steps
def test_invalidate_packed_and_rollout_recapture():
    """An update that bypasses autograd's version counters (`p.data` arithmetic, EMA, a broadcast) is picked up after
    model.invalidate_packed(); a live Rollout drops its captured hipGraph and re-captures on the new images."""
    from graphs4cfd_amd.nn.model import Rollout
    g = S.mus_graph(4000, levels=2, seed=41).to(DEV)
    torch.manual_seed(42)
    model = gfd.nn.NsTwoScaleGNN(arch=S.mus_arch("NsTwoScaleGNN", 128), device=DEV)
    g.batch = torch.zeros(g.num_nodes, dtype=torch.long, device=DEV)
    with torch.no_grad():
        y0 = model.forward(g).clone()
        ro = Rollout(model, g, 12, capture=True)
        ro.run(4)
        assert ro._hipgraph is not None
        w_old = {k: v.clone() for k, v in model.state_dict().items()}
        for p in model.node_decoder.parameters():
            p.data.mul_(0.5)                       # does not advance p._version
        model.invalidate_packed()
        ro.run(4)                                  # eager on the new weights, re-captured, replayed
        assert ro._hipgraph is not None
        got = ro.outputs[:, : 3 * 8].clone()
        ro.close()
        y1 = model.forward(g)
        assert (y1 - y0).abs().max().item() > 1e-3, "the forward must see the new weights"
        # the same 4 + 4 steps with eager launches only
        new = {k: v.clone() for k, v in model.state_dict().items()}
        model.load_state_dict(w_old)
        ro = Rollout(model, g, 12, capture=False)
        ro.run(4)
        model.load_state_dict(new)
        ro.run(4)
        assert torch.equal(ro.outputs[:, : 3 * 8], got)
        ro.close()


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two visible GPUs: the gpurun boxes and the driver's GPU-test tier expose "
                    "one, and HIP_VISIBLE_DEVICES cannot make one device appear twice — g4c::DeviceGuard's device switch has run on "
                    "device 0 only (a no-op there); run this test on a multi-GPU node")
def test_model_on_a_non_current_device():
    """`device=cuda:1` while the process's current device stays 0 (the reference API's usage): the C entry points switch to
    the device that owns their buffers."""
    assert torch.cuda.current_device() == 0
    d1 = torch.device("cuda", 1)
    g = S.mus_graph(3000, levels=2, seed=43)
    torch.manual_seed(44)
    m0 = gfd.nn.NsTwoScaleGNN(arch=S.mus_arch("NsTwoScaleGNN", 128), device=DEV)
    m1 = gfd.nn.NsTwoScaleGNN(arch=S.mus_arch("NsTwoScaleGNN", 128), device=d1)
    m1.load_state_dict(m0.state_dict())
    y0 = m0.solve(g.clone().to(DEV), 5)
    y1 = m1.solve(g.clone().to(d1), 5)
    assert y1.device == d1 and torch.cuda.current_device() == 0
    assert torch.equal(y0.cpu(), y1.cpu())


# ------------------------------------------------------------------ the dual-tile kernel of the large message launches (mlp_bx6i.hip)
@pytest.mark.parametrize("kernel", ["bx6i"])
@pytest.mark.parametrize("prec", ["f16x3", "bf16x6"])
@pytest.mark.parametrize("rows", [1, 33, 64, 6001, 90000])
def test_bx6i_dual_tile_kernel_equals_tile_kernel(rows, kernel, prec, monkeypatch):
    """g4c_mlp_bx6i_enable(2) (every eligible launch; the default mode takes launches of >= 400k rows, exercised by the at-size
    tests): the dual-tile software-pipelined kernel against the 32-row-tile kernel on the hoisted message form, a plain one-block
    form with SELU output, and the fused per-target aggregation (bit-exact reduction of the rows it stores, ragged segments)."""
    lib = _lib.load()
    monkeypatch.setattr(ops, "_PRECISION", prec)
    H, n = 128, max(rows // 6, 2)
    torch.manual_seed(rows)
    blk = B.GNBlock((3 * H, (H, H, H), True), (2 * H, (H, H, H), True)).to(DEV)
    deg = torch.randint(0, 10, (n,)) if rows > 64 else torch.full((n,), max(rows // n, 1))
    col = torch.arange(n).repeat_interleave(deg)
    E = max(int(col.numel()), 1)
    if int(col.numel()) == 0:
        col = torch.zeros(1, dtype=torch.long)
    edge_index = torch.stack([torch.randint(0, n, (E,)), col]).to(DEV)
    ep, csr = plan.edge_csr(edge_index, n)
    v, e = torch.randn(n, H, device=DEV), torch.randn(E, H, device=DEV)
    W1 = blk.edge_mlp.state_dict()["MLP.linear_1.weight"]
    pr, pc = (v @ W1[:, H:2 * H].T).contiguous(), (v @ W1[:, 2 * H:].T).contiguous()
    pk = blk.edge_mlp._packed_cols(0, H, [H], [False], False)
    src = [ops.Source(e, pre_act=_lib.ACT_SELU), ops.Source(pr, index=ep.row, additive=True), ops.Source(pc, index=ep.col, additive=True)]

    ids = torch.randperm(E, device=DEV)[: max(E // 2, 1)].to(torch.int32)
    sub = [ops.Source(e, index=ids, pre_act=_lib.ACT_SELU), ops.Source(pr, index=ep.row[ids.long()].contiguous(), additive=True),
           ops.Source(pc, index=ep.col[ids.long()].contiguous(), additive=True)]

    def run():
        out = {"edge": ops.mlp_forward(pk, src, E), "plain_selu": ops.mlp_forward(pk, [ops.Source(e, index=ep.row)], E, _lib.ACT_SELU)}
        # a subset of the rows gathered through an index and scattered back through out_idx (the interior / boundary launches of the
        # partitioned forward, partition.py)
        buf = torch.zeros(E, H, device=DEV)
        ops.mlp_forward(pk, sub, int(ids.numel()), out=buf, out_idx32=ids)
        out["subset_scattered"] = buf
        if csr.tiles() is not None:
            for mean in (True, False):
                a = torch.full((n, H), float("nan"), device=DEV)
                out[f"rows_agg_{mean}"] = ops.mlp_forward(pk, src, E, agg=(csr, a, mean))
                out[f"agg_{mean}"] = a
                a2 = torch.full((n, H), float("nan"), device=DEV)
                assert ops.mlp_forward(pk, src, E, agg=(csr, a2, mean), store_rows=False) is None
                out[f"agg_only_{mean}"] = a2
        return out
    enable = getattr(lib, f"g4c_mlp_{kernel}_enable")
    olds = (lib.g4c_mlp_bx6i_enable(0),)
    try:
        ref = run()
        enable(2)
        got = run()
    finally:
        lib.g4c_mlp_bx6i_enable(olds[0])
    for k in ref:
        torch.testing.assert_close(got[k], ref[k], rtol=2e-5, atol=2e-5, msg=lambda m: f"{k}: {m}")
    for mean in (True, False):
        if f"agg_{mean}" in got:
            assert torch.equal(got[f"agg_{mean}"], ops.segment_reduce(got[f"rows_agg_{mean}"], csr, mean))
            assert torch.equal(got[f"agg_only_{mean}"], got[f"agg_{mean}"])


# ------------------------------------------------------------------ the tile kernel's small-launch instantiation (deep weight ring)
@pytest.mark.parametrize("prec", ["f16x3", "bf16x6", "bf16"])
@pytest.mark.parametrize("rows", [1, 33, 700, 5000])
def test_small_launch_deep_ring_is_bit_identical(rows, prec):
    """g4c_mlp_small_launch_tiles: launches of few tiles run mlp_bx6_kernel with a whole 128-k block of weights in flight per wave
    instead of the two-step ring.  Only the order of the weight LOADS changes — every result must be bit for bit the ring-of-two
    kernel's: node launch with heads (two direct blocks), message launch with additive rows / an index / the fused aggregation,
    an encoder with a narrow input, in the three split arithmetics."""
    if ops.mlp_precision() != "f16x3":
        pytest.skip("runs under the default arithmetic only (it sets the mode itself)")
    lib = _lib.load()
    H, n = 128, max(rows // 6, 2)
    old_prec = ops.set_mlp_precision(prec)
    old_ws, old_i = lib.g4c_mlp_ws_enable(0), lib.g4c_mlp_bx6i_enable(0)
    old_lim = lib.g4c_mlp_small_launch_tiles(-1)
    try:
        torch.manual_seed(rows + 7)
        blk = B.GNBlock((3 * H, (H, H, H), True), (2 * H, (H, H, H), True)).to(DEV)
        enc = B.MLP(5, (H, H, H), True).to(DEV)
        v, aggr = torch.randn(n, H, device=DEV), torch.randn(n, H, device=DEV)
        col = torch.arange(n).repeat_interleave(6)
        E = int(col.numel())
        edge_index = torch.stack([torch.randint(0, n, (E,)), col]).to(DEV)
        e, ea = torch.randn(E, H, device=DEV), torch.randn(E, 5, device=DEV)
        ep, csr = plan.edge_csr(edge_index, n)
        W1 = blk.edge_mlp.state_dict()["MLP.linear_1.weight"]
        pr, pc = (v @ W1[:, H:2 * H].T).contiguous(), (v @ W1[:, 2 * H:].T).contiguous()
        pk = blk.edge_mlp._packed_cols(0, H, [H], [False], False)
        adds = [ops.Source(pr, index=ep.row, additive=True), ops.Source(pc, index=ep.col, additive=True)]
        idx = torch.randint(0, E, (E,), device=DEV, dtype=torch.int32)

        def run():
            out = {}
            y, heads = blk.node_mlp.run_with_heads([ops.Source(aggr), ops.Source(v)], n, _lib.ACT_SELU, blk.edge_mlp, H, [H, H])
            out["node"], out["head0"], out["head1"] = y, heads[0].float(), heads[1].float()
            out["edge"] = ops.mlp_forward(pk, [ops.Source(e, pre_act=_lib.ACT_SELU)] + adds, E)
            out["indexed"] = ops.mlp_forward(pk, [ops.Source(e, index=idx)] + adds, E, _lib.ACT_SELU)
            out["encoder"] = enc(ea)
            if csr.tiles() is not None:
                a = torch.full((n, H), float("nan"), device=DEV)
                out["rows"] = ops.mlp_forward(pk, [ops.Source(e)] + adds, E, agg=(csr, a, True))
                out["agg"] = a
            return {k: t.clone() for k, t in out.items()}
        lib.g4c_mlp_small_launch_tiles(0)
        ref = run()
        lib.g4c_mlp_small_launch_tiles(1 << 30)
        got = run()
    finally:
        lib.g4c_mlp_small_launch_tiles(old_lim)
        lib.g4c_mlp_ws_enable(old_ws); lib.g4c_mlp_bx6i_enable(old_i)
        ops.set_mlp_precision(old_prec)
    for k in ref:
        assert torch.isfinite(got[k]).all() and torch.equal(got[k], ref[k]), k


# ------------------------------------------------------------------ the weight-stationary persistent kernel (mlp_ws.hip)
@pytest.mark.parametrize("variant", [("f16x3", 3), ("f16x3", 2), ("bf16", 2), ("bf16", 3)], ids=lambda v: f"{v[0]}-{v[1]}layers")
@pytest.mark.parametrize("rows", [1, 33, 6000, 70000])
def test_ws_persistent_kernel_equals_tile_kernel(rows, variant):
    """g4c_mlp_ws_enable(2): the weight-stationary persistent kernel against the 32-row-tile kernel on the message form (first
    layer hoisted, rows direct / through an index / scattered through an output index), with the fused per-target aggregation on
    regular and ragged segments (bit-exact reduction of the rows it stores, same aggregate when the rows are not stored) — in the
    f16x3 stream and in the rounded-bf16 mode, for three-layer (MuS-GNN) and two-layer (REMuS-GNN) MLPs; in the rounded-bf16 mode
    also with bf16 rows in and bf16 / bf16(SELU) rows out (g4c_mlp_io_t.out_dtype: REMuS-GNN's angle launches).
    Rounded-bf16 tolerance: the kernels add a row's products in different orders, and a last-bit difference of a hidden
    pre-activation can flip its rounding to bf16 (single elements differ by ~1e-3, the mean difference is round-off)."""
    prec, layers = variant
    if ops.mlp_precision() != "f16x3":
        pytest.skip("runs under the default arithmetic only (it sets the mode itself)")
    lib = _lib.load()
    H, n = 128, max(rows // 6, 2)
    old_prec = ops.set_mlp_precision(prec)
    old_ws, old_i = lib.g4c_mlp_ws_enable(0), lib.g4c_mlp_bx6i_enable(0)
    try:
        torch.manual_seed(rows)
        hid = (H,) * layers
        blk = B.GNBlock((3 * H, hid, True), (2 * H, hid, True)).to(DEV)
        v = torch.randn(n, H, device=DEV)
        deg = torch.full((n,), 6, dtype=torch.long) if rows != 6000 else torch.randint(0, 10, (n,))
        col = torch.arange(n).repeat_interleave(deg)
        E = int(col.numel())
        edge_index = torch.stack([torch.randint(0, n, (E,)), col]).to(DEV)
        e = torch.randn(E, H, device=DEV)
        ep, csr = plan.edge_csr(edge_index, n)
        W1 = blk.edge_mlp.state_dict()["MLP.linear_1.weight"]
        pr, pc = (v @ W1[:, H:2 * H].T).contiguous(), (v @ W1[:, 2 * H:].T).contiguous()
        pk = blk.edge_mlp._packed_cols(0, H, [H], [False], False)
        adds = [ops.Source(pr, index=ep.row, additive=True), ops.Source(pc, index=ep.col, additive=True)]
        src = [ops.Source(e, pre_act=_lib.ACT_SELU)] + adds
        idx = torch.randint(0, E, (E,), device=DEV, dtype=torch.int32)
        oidx = torch.randperm(E, device=DEV).to(torch.int32)
        e16 = torch.nn.functional.selu(e).to(torch.bfloat16)

        def run():
            out = {"edge": ops.mlp_forward(pk, src, E), "indexed": ops.mlp_forward(pk, [ops.Source(e, index=idx)] + adds, E, _lib.ACT_SELU),
                   "indexed_no_adds": ops.mlp_forward(pk, [ops.Source(e, index=idx)], E, _lib.ACT_SELU),
                   "scattered": ops.mlp_forward(pk, src, E, out=torch.zeros(E, H, device=DEV), out_idx32=oidx)}
            if csr.tiles() is not None:
                for mean in (True, False):
                    a = torch.full((n, H), float("nan"), device=DEV)
                    out[f"rows_{mean}"] = ops.mlp_forward(pk, src, E, agg=(csr, a, mean))
                    out[f"agg_{mean}"] = a
                    a2 = torch.full((n, H), float("nan"), device=DEV)
                    ops.mlp_forward(pk, src, E, agg=(csr, a2, mean), store_rows=False)
                    out[f"agg_only_{mean}"] = a2
                if prec == "bf16":
                    for name, act in (("selu", _lib.ACT_SELU), ("plain", _lib.ACT_NONE)):
                        a = torch.full((n, H), float("nan"), device=DEV)
                        y = ops.mlp_forward(pk, [ops.Source(e16)] + adds, E, agg=(csr, a, True), rows_dtype=torch.bfloat16, rows_act=act)
                        assert y.dtype == torch.bfloat16
                        out[f"rows16_{name}"], out[f"agg16_{name}"] = y.float(), a
            return out
        ref = run()
        lib.g4c_mlp_ws_enable(2)
        got = run()
    finally:
        lib.g4c_mlp_ws_enable(old_ws); lib.g4c_mlp_bx6i_enable(old_i)
        ops.set_mlp_precision(old_prec)
    for k in ref:
        if prec != "bf16":
            torch.testing.assert_close(got[k], ref[k], rtol=2e-5, atol=2e-5, msg=lambda m: f"{k}: {m}")
        else:
            d = (got[k] - ref[k]).abs()
            lim, mlim = (6e-2, 2e-4) if k.startswith("rows16") else (3e-2, 5e-5)        # (rows16: one bf16 ulp of an O(1) value is 8e-3)
            assert torch.isfinite(got[k]).all() and d.max().item() <= lim and d.mean().item() <= mlim, (k, d.max().item(), d.mean().item())
    for mean in (True, False):
        if f"agg_{mean}" in got:
            assert torch.equal(got[f"agg_{mean}"], ops.segment_reduce(got[f"rows_{mean}"], csr, mean))
            assert torch.equal(got[f"agg_only_{mean}"], got[f"agg_{mean}"])


@pytest.mark.parametrize("prec", ["f16x3", "bf16"])
@pytest.mark.parametrize("deg", [4, 5, 6, 7, 8])
def test_ws_dense_pairs_of_uniform_segments(deg, prec):
    """G4C_AGG_UNIFORM(k): on a mesh whose every target has k incoming edges the weight-stationary kernel cuts each workgroup's rows
    into pairs of 64 consecutive rows — segments straddle tiles and pairs, the partial sum of a segment cut by a pair's end is carried
    to the next pair — and aggregates with static addressing.  The rows are those of the tile kernel (2e-5), the aggregate is the
    segment reduction of the rows the launch stored, bit for bit, at sizes that put every remainder at the pair boundaries (one
    workgroup with a single short pair, ranges that end inside a tile, more workgroups than pairs)."""
    if ops.mlp_precision() != "f16x3":
        pytest.skip("runs under the default arithmetic only (it sets the mode itself)")
    lib = _lib.load()
    H = 128
    old_prec = ops.set_mlp_precision(prec)
    old_ws, old_i = lib.g4c_mlp_ws_enable(0), lib.g4c_mlp_bx6i_enable(0)
    try:
        for n in (1, 9, 11, 173, 2999, 20011):
            torch.manual_seed(100 * deg + n)
            layers = 3 if prec == "f16x3" else 2
            blk = B.GNBlock((3 * H, (H,) * layers, True), (2 * H, (H,) * layers, True)).to(DEV)
            E = n * deg
            col = torch.arange(n).repeat_interleave(deg)
            edge_index = torch.stack([torch.randint(0, n, (E,)), col]).to(DEV)
            ep, csr = plan.edge_csr(edge_index, n)
            assert csr.uniform_deg == deg and csr.tiles() is not None
            e, pr, pc = torch.randn(E, H, device=DEV), torch.randn(n, H, device=DEV), torch.randn(n, H, device=DEV)
            pk = blk.edge_mlp._packed_cols(0, H, [H], [False], False)
            src = [ops.Source(e, pre_act=_lib.ACT_SELU), ops.Source(pr, index=ep.row, additive=True), ops.Source(pc, index=ep.col, additive=True)]
            lib.g4c_mlp_ws_enable(0)
            ref = ops.mlp_forward(pk, src, E)
            lib.g4c_mlp_ws_enable(2)
            for mean in (True, False):
                a = torch.full((n, H), float("nan"), device=DEV)
                y = ops.mlp_forward(pk, src, E, agg=(csr, a, mean))
                assert int(lib.g4c_mlp_last_kernel()) == 4
                if prec == "f16x3":
                    torch.testing.assert_close(y, ref, rtol=2e-5, atol=2e-5, msg=lambda m: f"rows {(deg, n, mean)}: {m}")
                else:
                    assert (y - ref).abs().mean().item() < 2e-4 and (y - ref).abs().max().item() < 0.1
                assert torch.equal(a, ops.segment_reduce(y, csr, mean)), (deg, n, mean)
                a2 = torch.full((n, H), float("nan"), device=DEV)
                ops.mlp_forward(pk, src, E, agg=(csr, a2, mean), store_rows=False)
                assert torch.equal(a2, a), (deg, n, mean)
    finally:
        lib.g4c_mlp_ws_enable(old_ws); lib.g4c_mlp_bx6i_enable(old_i)
        ops.set_mlp_precision(old_prec)


@pytest.mark.parametrize("variant", [("f16x3", 3, "ws"), ("f16x3", 2, "ws"), ("bf16", 2, "ws"), ("bf16x6", 3, "bx6i")],
                         ids=lambda v: f"{v[2]}-{v[0]}-{v[1]}layers")
def test_ws_persistent_kernel_repeated_launches_are_identical(variant):
    """The persistent kernel hands tiles from wave to wave through LDS; a missing barrier shows up as a rare difference between two
    launches on the same inputs (round 3: the tail of a launch WITHOUT the fused aggregation lacked the one between the next pair's
    parked rows and their first use — seen as one mismatch in a 600k-row launch).  60 launches of each large shape must be
    bit-identical to the first.  (Also the dual-tile kernel of the bf16x6 stream, which pipelines pairs of tiles the same way.)"""
    prec, layers, kernel = variant
    if ops.mlp_precision() != "f16x3":
        pytest.skip("runs under the default arithmetic only (it sets the mode itself)")
    lib = _lib.load()
    H, rows = 128, 300_000
    n = rows // 6
    old_prec = ops.set_mlp_precision(prec)
    old_ws, old_i = lib.g4c_mlp_ws_enable(2 if kernel == "ws" else 0), lib.g4c_mlp_bx6i_enable(2 if kernel == "bx6i" else 0)
    try:
        torch.manual_seed(7)
        hid = (H,) * layers
        blk = B.GNBlock((3 * H, hid, True), (2 * H, hid, True)).to(DEV)
        e, v = torch.randn(rows, H, device=DEV), torch.randn(n, H, device=DEV)
        W1 = blk.edge_mlp.state_dict()["MLP.linear_1.weight"]
        pr, pc = (v @ W1[:, H:2 * H].T).contiguous(), (v @ W1[:, 2 * H:].T).contiguous()
        pk = blk.edge_mlp._packed_cols(0, H, [H], [False], False)
        idx = torch.randint(0, rows, (rows,), device=DEV, dtype=torch.int32)
        col = torch.arange(rows, device=DEV) // 6
        ep, csr = plan.edge_csr(torch.stack([torch.randint(0, n, (rows,), device=DEV), col]), n)
        adds = [ops.Source(pr, index=ep.row, additive=True), ops.Source(pc, index=ep.col, additive=True)]
        agg = torch.empty(n, H, device=DEV)
        cases = {"indexed + adds": lambda: ops.mlp_forward(pk, [ops.Source(e, index=idx)] + adds, rows, _lib.ACT_SELU),
                 "direct + adds": lambda: ops.mlp_forward(pk, [ops.Source(e, pre_act=_lib.ACT_SELU)] + adds, rows),
                 "direct + adds + aggregation": lambda: ops.mlp_forward(pk, [ops.Source(e, pre_act=_lib.ACT_SELU)] + adds, rows, agg=(csr, agg, True))}
        if prec != "bf16":
            cases["indexed, no adds"] = lambda: ops.mlp_forward(pk, [ops.Source(e, index=idx)], rows, _lib.ACT_SELU)
        for name, fn in cases.items():
            first = fn().clone()
            for _ in range(60):
                assert torch.equal(fn(), first), name
    finally:
        lib.g4c_mlp_ws_enable(old_ws); lib.g4c_mlp_bx6i_enable(old_i)
        ops.set_mlp_precision(old_prec)


# ------------------------------------------------------------------ the fp16 range of the default arithmetic is observable
def test_f16_range_clip_recomputes_in_bf16x6_and_matches_the_oracle():
    """Adversarial WEIGHTS, normal inputs: the LayerNorm gain of the first MP layer's message MLP x 3e4 puts its output latents
    (|e'| up to ~1e5) beyond the fp16 range.  The reference computes in fp32 (nn/model.py:303-321).  The default "f16x3" arithmetic
    runs optimistically: the launches that convert those latents flag the clip, and solve() then recomputes the rollout in "bf16x6"
    (fp32 exponent range) before it returns — with a RuntimeWarning naming the MLPs, nothing silent — so its result IS the bf16x6
    result, bit for bit, and matches the oracle.  Nothing may be reported or recomputed for an ordinary model."""
    import warnings
    from graphs4cfd_amd.nn.model import Rollout
    g = S.mus_graph(3000, levels=2, seed=3)
    torch.manual_seed(4)
    model = gfd.nn.NsTwoScaleGNN(arch=S.mus_arch("NsTwoScaleGNN", 128), device=DEV)
    old = ops.set_mlp_precision("f16x3")
    try:
        ops.f16_range_report()                                  # (clear what earlier tests may have left)
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)      # an ordinary model: no clip, no warning, no second pass
            model.solve(g.clone(), 2)
        assert ops.f16_range_report() == []
        with torch.no_grad():
            model.mp111.edge_mlp.MLP.layer_norm.weight.mul_(3e4)
        model.invalidate_packed()
        w = {k: v.cpu() for k, v in model.state_dict().items()}
        ref = O.mus_solve("NsTwoScaleGNN", g.to_dict(), w, 5, model.num_fields)
        for capture in (False, True):                           # (5 steps: eager, captured, three replays)
            with pytest.warns(RuntimeWarning, match="recomputed in 'bf16x6'") as rec:
                out16 = model.solve(g.clone(), 5, capture=capture)
            assert any("NsTwoScaleGNN.mp11" in str(r.message) for r in rec), [str(r.message) for r in rec]
            assert ops.f16_range_report() == []                 # read once, then cleared
            torch.testing.assert_close(out16.cpu(), ref, rtol=2e-3, atol=2e-3)
            ops.set_mlp_precision("bf16x6")
            with warnings.catch_warnings():
                warnings.simplefilter("error", RuntimeWarning)
                out = model.solve(g.clone(), 5, capture=capture)
            ops.set_mlp_precision("f16x3")
            assert torch.equal(out16, out), (out16 - out).abs().max().item()
        # a rollout object that clipped stays in the exact-range arithmetic: later steps need no second pass
        gd = g.clone().to(DEV)
        gd.batch = torch.zeros(gd.num_nodes, dtype=torch.long, device=DEV)
        with Rollout(model, gd, 6, capture=True, reorder=False) as ro:
            ro.run(3)
            with pytest.warns(RuntimeWarning, match="recomputed in 'bf16x6'"):
                assert ro.validate() and ro.exact_range
            ro.run(3)
            with warnings.catch_warnings():
                warnings.simplefilter("error", RuntimeWarning)
                got = ro.result().clone()
        ops.set_mlp_precision("bf16x6")
        ref6 = model.solve(g.clone(), 6, capture=True)
        assert torch.equal(got, ref6)
    finally:
        ops.set_mlp_precision(old)


def test_bare_forward_is_range_validated_and_rollouts_keep_their_own_evidence():
    """VERDICT r05 item 6 / ADVICE r05: (a) a bare `model.forward(graph)` in the default arithmetic (the reference's other public
    entry, nn/mus_gnn.py:173-218) returns — with a RuntimeWarning — the "bf16x6" forward bit for bit when a value left the fp16 range,
    and an ordinary forward costs exactly one read of a flag buffer (ops._read_flags), no warning, nothing recomputed; (b) a second
    Rollout on the same model, a bare forward or a check_f16_range() call between the steps of a live rollout do not erase the clip
    that rollout still has to act on (it reads its own flag buffer)."""
    import warnings
    from graphs4cfd_amd.nn.model import Rollout
    torch.manual_seed(8)
    model = gfd.nn.NsOneScaleGNN(arch=S.mus_arch("NsOneScaleGNN", 128), device=DEV)
    old = ops.set_mlp_precision("f16x3")
    reads = []
    real_read = ops._read_flags
    try:
        g = S.mus_graph(2000, levels=1, seed=9).to(DEV)
        big = g.clone(); big.field = big.field * 1e5
        ops.f16_range_report()
        ops._read_flags = lambda buf: (reads.append(1), real_read(buf))[1]
        with torch.no_grad(), warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)
            y = model.forward(g).clone()
        assert len(reads) == 1, "an ordinary bare forward reads the range flags once"
        ops._read_flags = real_read
        with torch.no_grad(), pytest.warns(RuntimeWarning, match="computed again in 'bf16x6'"):
            y_big = model.forward(big).clone()
        ops.set_mlp_precision("bf16x6")
        with torch.no_grad():
            ref, ref_big = model.forward(g).clone(), model.forward(big).clone()
        ops.set_mlp_precision("f16x3")
        assert torch.equal(y_big, ref_big) and torch.isfinite(y_big).all()
        torch.testing.assert_close(y, ref, rtol=2e-5, atol=2e-5)
        assert ops.f16_range_report() == []
        # validation off: the clipped forward is delivered as computed, and says so when asked
        was = gfd.set_forward_validation(False)
        try:
            with torch.no_grad(), warnings.catch_warnings():
                warnings.simplefilter("error", RuntimeWarning)
                model.forward(big)
            assert any("NsOneScaleGNN" in n for n in ops.f16_range_report())
        finally:
            gfd.set_forward_validation(was)
        # (b) rollout A clips; then rollout B (ordinary input) is built on the same model, a bare forward and a report run in between
        big.batch = torch.zeros(big.num_nodes, dtype=torch.long, device=DEV)
        g.batch = big.batch
        ro_a = Rollout(model, big, 4, capture=False, reorder=False, label="A")
        ro_a.run(2)
        ro_b = Rollout(model, g, 4, capture=False, reorder=False, label="B")
        with torch.no_grad():
            model.forward(g)
        ops.check_f16_range()
        ro_b.run(2)
        with pytest.warns(RuntimeWarning, match="recomputed in 'bf16x6'"):
            out_a = ro_a.result().clone()
        assert ro_a.exact_range
        ro_a.close(); ro_b.close()
        ops.set_mlp_precision("bf16x6")
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ref_a = model.solve(big.clone(), 4, capture=False)
        assert torch.equal(out_a[:, :6], ref_a[:, :6])
    finally:
        ops._read_flags = real_read
        ops.set_mlp_precision(old)


def test_f16x3_is_range_safe_for_huge_and_tiny_input_rows():
    """inputs far outside the fp16 range.  A field scaled by 1e5 makes the first hidden activations of the node
    encoder ~1e5; scaled by 1e30 everything downstream is astronomically large.  The reference computes in fp32.  solve() in the
    default arithmetic must return what "bf16x6" returns (it recomputes in it: bit-equal), finite, with a warning; a field scaled by
    1e-6 (tiny rows) must NOT need the second pass and must agree with "bf16x6" to fp32 round-off."""
    import warnings
    torch.manual_seed(5)
    model = gfd.nn.NsOneScaleGNN(arch=S.mus_arch("NsOneScaleGNN", 128), device=DEV)
    old = ops.set_mlp_precision("f16x3")
    try:
        for scale, second_pass in ((1e5, True), (1e30, True), (1e-6, False)):
            g = S.mus_graph(2000, levels=1, seed=6)
            g.field = g.field * scale
            ops.f16_range_report()
            ops.set_mlp_precision("f16x3")
            with warnings.catch_warnings(record=True) as rec:
                warnings.simplefilter("always")
                out = model.solve(g.clone(), 3)
            redone = any("recomputed in 'bf16x6'" in str(r.message) for r in rec)
            assert redone == second_pass, (scale, [str(r.message) for r in rec])
            ops.set_mlp_precision("bf16x6")
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")          # (solve() notes inputs beyond 4096 in either arithmetic)
                ref = model.solve(g.clone(), 3)
            assert torch.isfinite(ref).all() and torch.isfinite(out).all(), scale
            if second_pass:
                assert torch.equal(out, ref), scale
            else:
                torch.testing.assert_close(out, ref, rtol=2e-5, atol=2e-5 * float(ref.abs().max()))
    finally:
        ops.set_mlp_precision(old)


def test_remus_bf16_compact_messages_are_bit_identical():
    """Rounded-bf16 mode (BASELINE config 3): the angle messages stored as bf16(SELU(row)) by the launch that fuses the aggregation
    (G4C_DTYPE_BF16_SELU, half the bytes) give bit for bit the forward of fp32 message rows — the reader forms the same operand (one
    rounding, after the activation), the aggregate is taken from the fp32 rows either way."""
    old = ops.set_mlp_precision("bf16")
    was = B.COMPACT_MESSAGES
    try:
        g = S.remus_graph(20_000, k=5, seed=23).to(DEV)
        torch.manual_seed(24)
        model = gfd.nn.NsRotEquiTreeScaleGNN(arch=S.remus_arch(128), device=DEV)
        outs = []
        for on in (False, True):
            B.COMPACT_MESSAGES = on
            with torch.no_grad():
                outs.append(model.forward(g).clone())
        assert torch.equal(outs[0], outs[1]), (outs[0] - outs[1]).abs().max().item()
    finally:
        B.COMPACT_MESSAGES = was
        ops.set_mlp_precision(old)


@pytest.mark.parametrize("layers", [2, 3])
def test_row_split_kernel_matches_the_weight_stationary_path(layers):
    """Rounded-bf16 mode, round 6 (blocks.ROW_SPLIT_BF16; csrc/mlp_rs.hip): message launches over receivers of one uniform in-degree
    4 .. 8 run on the row-split kernel — a wave owns 16 rows through all layers, bf16 rows in its own column order
    (ops.RsOrderedRows), the aggregation a segmented scan.  Against the weight-stationary / tile path of the same mode on the same
    inputs: rows and aggregates agree to the mode's rounding (a hidden activation that rounds to the neighbouring bf16 under the other
    summation order moves an output by ~1e-3: mean difference < 2e-5); the aggregate is the fixed-order sum of the kernel's OWN fp32
    rows to 1e-6; compact rows come back tagged, and a reader outside the kernel sees them in feature order."""
    lib = _lib.load()
    old = ops.set_mlp_precision("bf16")
    was = B.ROW_SPLIT_BF16
    H = 128
    try:
        for n, K in ((5001, 5), (6200, 4), (3100, 8), (3601, 7), (4200, 6)):
            torch.manual_seed(1000 * layers + K)
            E = n * K
            assert E >= max(B.RS1_MIN_ROWS, B.HOIST_MIN_ROWS)          # (both paths hoist the first layer: bf16 products either way)
            blk = B.GNBlock((3 * H, (H,) * layers, True), (2 * H, (H,) * layers, True)).to(DEV)
            a32, e_send, e_recv = torch.randn(E, H, device=DEV), torch.randn(n, H, device=DEV), torch.randn(n, H, device=DEV)
            ei = torch.stack([torch.randint(0, n, (E,)), torch.arange(n).repeat_interleave(K)]).to(DEV)
            ep, csr = plan.edge_csr(ei, n)
            assert csr.uniform_deg == K

            def launch(x_src, **kw):
                agg = torch.full((n, H), float("nan"), device=DEV)
                with torch.no_grad():
                    y = blk.edge_mlp.run_hoisted([x_src], [(e_send, ep.row), (e_recv, ep.col)], E, agg=(csr, agg, True), **kw)
                return y, agg, int(lib.g4c_mlp_last_kernel())

            compact = dict(rows_dtype=torch.bfloat16, rows_act=_lib.ACT_SELU)
            res = {}
            for on in (False, True):
                B.ROW_SPLIT_BF16 = on
                res[on, "fp32"] = launch(ops.Source(a32, pre_act=_lib.ACT_SELU))
                res[on, "compact"] = launch(ops.Source(a32, pre_act=_lib.ACT_SELU), **compact)
                # compact rows as the next launch's input (already activated; the same rows for both paths, in each one's column order)
                x16 = res[False, "compact"][0]
                res[on, "chained"] = launch(ops.Source(ops.RsOrderedRows.tag(x16[:, ops._rs_k_order(DEV)].contiguous()) if on else x16), **compact)
                res[on, "no rows"] = launch(ops.Source(a32, pre_act=_lib.ACT_SELU), store_rows=False)
            for form in ("fp32", "compact", "chained", "no rows"):
                (y0, g0, k0), (y1, g1, k1) = res[False, form], res[True, form]
                assert k1 == _lib.KERNEL_MLP_RS and k0 != _lib.KERNEL_MLP_RS, (form, k0, k1)
                assert torch.isfinite(g1).all()
                d = (g1 - g0).abs()
                assert d.mean().item() < 2e-5 and d.max().item() < 2e-2, (form, K, d.mean().item(), d.max().item())
                if form == "no rows":
                    assert y0 is None and y1 is None
                    continue
                if y1.dtype == torch.bfloat16:
                    assert isinstance(y1, ops.RsOrderedRows) and not isinstance(y0, ops.RsOrderedRows)
                    y1 = ops.rs_rows_to_natural(y1)
                d = (y1.float() - y0.float()).abs()
                assert d.mean().item() < 2e-5 and d.max().item() < 4e-2, (form, K, d.mean().item(), d.max().item())
            # the scan: the aggregate is the mean of the kernel's own fp32 rows
            y1, g1, _ = res[True, "fp32"]
            torch.testing.assert_close(g1, ops.segment_reduce(y1, csr, True), rtol=0, atol=1e-6)
            # "no rows" and "compact" aggregate the same fp32 rows
            assert torch.equal(res[True, "no rows"][1], res[True, "compact"][1])
            # a reader outside the kernel (here: the tile kernel, forced) sees tagged rows in feature order
            tagged = res[True, "compact"][0]
            pk = blk.edge_mlp._packed_cols(0, H, [H], [False], False)
            with torch.no_grad():
                pr = ops.mlp_forward(blk.edge_mlp._packed_cols(H, 2 * H, [H], [False], True), [ops.Source(e_send)], n)
                pc = ops.mlp_forward(blk.edge_mlp._packed_cols(2 * H, 3 * H, [H], [False], True), [ops.Source(e_recv)], n)
                adds = [ops.Source(pr, index=ep.row, additive=True), ops.Source(pc, index=ep.col, additive=True)]
                via_guard = ops.mlp_forward(pk, [ops.Source(tagged)] + adds, E)
                by_hand = ops.mlp_forward(pk, [ops.Source(ops.rs_rows_to_natural(tagged))] + adds, E)
            assert torch.equal(via_guard, by_hand)
    finally:
        B.ROW_SPLIT_BF16 = was
        ops.set_mlp_precision(old)


def test_bf16_aggregate_of_the_row_split_kernel_is_the_operand_its_reader_forms():
    """Rounded-bf16 mode (blocks.AGGREGATE_BF16, G4C_AGG_OUT_BF16): the row-split kernel stores the per-receiver mean as bf16 rows in its
    column order when the layer's update MLP reads it — (a) bit for bit the round-to-nearest bf16 of the fp32 aggregate it stores
    otherwise; (b) the update MLP, packed with that block's weight columns in the same order, gives the result of the fp32 aggregate
    up to the summation order of its first layer (1e-5), with and without the next layer's product heads."""
    lib = _lib.load()
    old = ops.set_mlp_precision("bf16")
    was = B.AGGREGATE_BF16
    H = 128
    try:
        torch.manual_seed(77)
        n, K = 6000, 5
        E = n * K
        blk = B.GNBlock((3 * H, (H, H), True), (2 * H, (H, H), True)).to(DEV)
        nxt = B.GNBlock((3 * H, (H, H), True), (2 * H, (H, H), True)).to(DEV)
        a, v = torch.randn(E, H, device=DEV), torch.randn(n, H, device=DEV)
        ei = torch.stack([torch.randint(0, n, (E,)), torch.arange(n).repeat_interleave(K)]).to(DEV)
        ep, csr = plan.edge_csr(ei, n)
        order = ops._rs_k_order(DEV)
        # (a) the launch alone
        aggs = {}
        for dt in (torch.float32, torch.bfloat16):
            g = torch.empty(n, H, dtype=dt, device=DEV)
            with torch.no_grad():
                blk.edge_mlp.run_hoisted([ops.Source(a, pre_act=_lib.ACT_SELU)], [(v, ep.row), (v, ep.col)], E, agg=(csr, g, True), store_rows=False)
            assert int(lib.g4c_mlp_last_kernel()) == _lib.KERNEL_MLP_RS
            aggs[dt] = g
        assert torch.equal(aggs[torch.bfloat16], aggs[torch.float32].to(torch.bfloat16)[:, order])
        # (b) the whole layer
        res = {}
        for on in (False, True):
            B.AGGREGATE_BF16 = on
            with torch.no_grad():
                res[on, "heads"] = B._mp_step(blk.edge_mlp, blk.node_mlp, v, a, ei, "mean", _lib.ACT_SELU, e_pre_act=_lib.ACT_SELU,
                                              next_msg=nxt.edge_mlp, compact_messages=True)
                res[on, "plain"] = B._mp_step(blk.edge_mlp, blk.node_mlp, v, a, ei, "mean", _lib.ACT_SELU, e_pre_act=_lib.ACT_SELU, compact_messages=True)
        for form in ("heads", "plain"):
            (v0, e0, *p0), (v1, e1, *p1) = res[False, form], res[True, form]
            assert torch.equal(e0, e1)                                    # (the message rows do not depend on how the aggregate is stored)
            torch.testing.assert_close(v1, v0, rtol=0, atol=1e-5)
            if form == "heads":
                assert p0[0] is not None and p1[0] is not None
                for h0, h1 in zip(p0[0], p1[0]):
                    d = (h1.float() - h0.float()).abs()
                    assert d.mean().item() < 1e-5 and d.max().item() < 4e-2          # (bf16 rows: a rare one-ulp flip)
    finally:
        B.AGGREGATE_BF16 = was
        ops.set_mlp_precision(old)


def test_row_split_update_kernel_matches_the_tile_kernel():
    """Rounded-bf16 mode, round 6 (blocks.UPDATE_ROW_SPLIT; csrc/mlp_rs.hip mlp_rs2_kernel): the update MLP of an EdgeMP — [bf16 aggregate
    | bf16 e] -> 256 -> 128 -> 128 -> LayerNorm -> SELU -> e' (+ the next layer's two product heads) — on the row-split update kernel
    (all five weight blocks in LDS, bias / LayerNorm vectors in registers), against the tile kernel on the same inputs: with fp32 output
    rows and both blocks in the row-split order the two sum in the same order (1e-5); bf16 rows agree to a rare one-ulp flip."""
    lib = _lib.load()
    old = ops.set_mlp_precision("bf16")
    was = B.UPDATE_ROW_SPLIT
    H = 128
    order = ops._rs_k_order(DEV)
    rs = lambda t: ops.RsOrderedRows.tag(t[:, order].contiguous())
    nat = lambda t: ops.rs_rows_to_natural(t) if isinstance(t, ops.RsOrderedRows) else t
    try:
        for n in (20001, 47000):
            torch.manual_seed(n)
            blk = B.GNBlock((3 * H, (H, H), True), (2 * H, (H, H), True)).to(DEV)
            nxt = B.GNBlock((3 * H, (H, H), True), (2 * H, (H, H), True)).to(DEV)
            agg = torch.randn(n, H, device=DEV).to(torch.bfloat16)
            e = torch.nn.functional.selu(torch.randn(n, H, device=DEV)).to(torch.bfloat16)
            for e_tagged in (True, False):
                for heads in (True, False):
                    for out16 in (True, False):
                        res = {}
                        for on in (False, True):
                            B.UPDATE_ROW_SPLIT = on
                            src = [ops.Source(rs(agg)), ops.Source(rs(e) if e_tagged else e)]
                            out = torch.empty(n, H, device=DEV, dtype=torch.bfloat16 if out16 else torch.float32)
                            with torch.no_grad():
                                if heads:
                                    y, hs = blk.node_mlp.run_with_heads(src, n, _lib.ACT_SELU, nxt.edge_mlp, H, [H, H], out=out, rs_rows=True)
                                else:
                                    y, hs = blk.node_mlp.run_coded(src, n, _lib.ACT_SELU, out=out), []
                            k = int(lib.g4c_mlp_last_kernel())
                            assert (k == _lib.KERNEL_MLP_RS2) == on, (k, on)
                            if on:
                                assert isinstance(y, ops.RsOrderedRows) == out16 and all(isinstance(h, ops.RsOrderedRows) for h in hs)
                            res[on] = (nat(y).float().clone(), [nat(h).float().clone() for h in hs])
                        (y0, h0), (y1, h1) = res[False], res[True]
                        d = (y1 - y0).abs()
                        form = (n, e_tagged, heads, out16)
                        if not out16 and e_tagged:
                            assert d.max().item() < 1e-5, (form, d.max().item())
                        assert d.mean().item() < 2e-6 and d.max().item() < 4e-2, (form, d.mean().item(), d.max().item())
                        for a, b in zip(h0, h1):
                            dh = (b - a).abs()
                            assert dh.mean().item() < 2e-6 and dh.max().item() < 4e-2, (form, dh.mean().item(), dh.max().item())
    finally:
        B.UPDATE_ROW_SPLIT = was
        ops.set_mlp_precision(old)


def test_row_split_path_in_the_remus_model():
    """BASELINE config 3's model at 20k nodes in the rounded-bf16 mode with and without the row-split kernel: the level-1 and level-2
    angle launches take it (k = 5 angles per edge), products and compact messages travel in its column order between consecutive
    EdgeMPs, and the forward agrees with the weight-stationary path to the mode's rounding; a captured rollout replays it."""
    lib = _lib.load()
    old = ops.set_mlp_precision("bf16")
    was = B.ROW_SPLIT_BF16
    try:
        g = S.remus_graph(20_000, k=5, seed=31).to(DEV)
        torch.manual_seed(32)
        model = gfd.nn.NsRotEquiTreeScaleGNN(arch=S.remus_arch(128), device=DEV)
        outs, used = {}, {}
        for on in (False, True):
            B.ROW_SPLIT_BF16 = on
            seen = set()
            orig = ops.mlp_forward

            def spy(*a, **kw):
                r = orig(*a, **kw)
                seen.add(int(lib.g4c_mlp_last_kernel()))
                return r
            ops.mlp_forward = spy
            try:
                with torch.no_grad():
                    outs[on] = model.forward(g.clone()).clone()
            finally:
                ops.mlp_forward = orig
            used[on] = seen
        assert _lib.KERNEL_MLP_RS in used[True] and _lib.KERNEL_MLP_RS not in used[False], used
        d = (outs[True] - outs[False]).abs()
        assert torch.isfinite(outs[True]).all() and d.max().item() < 6e-2 and d.mean().item() < 2e-3, (d.max().item(), d.mean().item())      # (the mode's own tolerance against the fp32 oracle: 6e-2 / 1e-2)
        B.ROW_SPLIT_BF16 = True
        cap, eag = model.solve(g.clone(), 3, capture=True), model.solve(g.clone(), 3, capture=False)
        assert torch.equal(cap, eag) and torch.isfinite(cap).all()
        # inside a rollout the static angle latents are cached as the bf16 rows the kernel would form from them: the same step, bit for bit
        assert torch.equal(cap[:, :outs[True].size(1)], outs[True])
    finally:
        B.ROW_SPLIT_BF16 = was
        ops.set_mlp_precision(old)


@pytest.mark.parametrize("prec", ["f16x3", "bf16"])
def test_remus_entry_products_come_from_the_producer_launch(prec):
    """remus_gnn.ENTRY_PRODUCTS (round 6): the hoisted first-layer products of the first EdgeMP of a run on a level are two heads of the
    launch that produces its edge latents (edge encoder, DownEdgeMP, UpEdgeMP) instead of two product launches — the same products
    (same operand rounding, same weights, same summation order): the forward is bit-identical."""
    from graphs4cfd_amd.nn import remus_gnn as R
    old = ops.set_mlp_precision(prec)
    was, was_u = R.ENTRY_PRODUCTS, B.UPDATE_ROW_SPLIT
    B.UPDATE_ROW_SPLIT = False          # (kernel for kernel: with compact entry latents the first update would move to mlp_rs2_kernel)
    try:
        g = S.remus_graph(20_000, k=5, seed=41).to(DEV)
        torch.manual_seed(42)
        model = gfd.nn.NsRotEquiTreeScaleGNN(arch=S.remus_arch(128), device=DEV)
        outs = {}
        for on in (False, True):
            R.ENTRY_PRODUCTS = on
            with torch.no_grad():
                outs[on] = model.forward(g.clone()).clone()
        assert torch.equal(outs[True], outs[False]), (outs[True] - outs[False]).abs().max().item()
    finally:
        R.ENTRY_PRODUCTS, B.UPDATE_ROW_SPLIT = was, was_u
        ops.set_mlp_precision(old)


def test_remus_compact_edge_latents_are_the_same_operand():
    """blocks.COMPACT_LATENTS (round 6, rounded-bf16 mode): the edge latents between consecutive EdgeMPs of a level are stored as bf16
    rows by the update launch (out_dtype G4C_DTYPE_BF16 beside bf16 heads) — their only reader, the next update MLP, rounds them to bf16 on load:
    the forward is bit-identical."""
    old = ops.set_mlp_precision("bf16")
    was, was_u = B.COMPACT_LATENTS, B.UPDATE_ROW_SPLIT
    B.UPDATE_ROW_SPLIT = False          # (kernel for kernel: compact latents are what makes an update eligible for mlp_rs2_kernel)
    try:
        g = S.remus_graph(20_000, k=5, seed=51).to(DEV)
        torch.manual_seed(52)
        model = gfd.nn.NsRotEquiTreeScaleGNN(arch=S.remus_arch(128), device=DEV)
        outs = {}
        for on in (False, True):
            B.COMPACT_LATENTS = on
            with torch.no_grad():
                outs[on] = model.forward(g.clone()).clone()
        assert torch.equal(outs[True], outs[False]), (outs[True] - outs[False]).abs().max().item()
    finally:
        B.COMPACT_LATENTS, B.UPDATE_ROW_SPLIT = was, was_u
        ops.set_mlp_precision(old)


def test_remus_down_angles_grouped_by_receiver():
    """remus_gnn.GROUP_DOWN_ANGLES (round 6, rounded-bf16 mode): the static inter-level angle latents and their index regrouped by
    receiver, so that DownEdgeMP's angle launch runs on the row-split kernel (aggregation fused, no rows stored) instead of
    mlp_ws_kernel + segment_reduce over rows in no receiver order: the same sums in another order — the forward agrees to the mode's
    rounding; plan.grouped_by_target is a stable grouping with an identity of its own."""
    from graphs4cfd_amd.nn import remus_gnn as R
    old = ops.set_mlp_precision("bf16")
    was = R.GROUP_DOWN_ANGLES
    try:
        g = S.remus_graph(20_000, k=5, seed=61).to(DEV)
        n2 = int(g.edge_index2.size(1))
        grouped, perm = plan.grouped_by_target(g.angle_index12, n2)
        assert perm is not None and torch.equal(grouped, g.angle_index12[:, perm]) and bool((grouped[1][1:] >= grouped[1][:-1]).all())
        assert plan.grouped_by_target(g.angle_index12, n2)[0] is grouped and plan.edge_csr(grouped, n2)[1].perm is None
        torch.manual_seed(62)
        model = gfd.nn.NsRotEquiTreeScaleGNN(arch=S.remus_arch(128), device=DEV)
        outs = {}
        for on in (False, True):
            R.GROUP_DOWN_ANGLES = on
            with torch.no_grad():
                outs[on] = model.forward(g.clone()).clone()
        d = (outs[True] - outs[False]).abs()
        assert torch.isfinite(outs[True]).all() and d.mean().item() < 1e-2 and d.max().item() < 1e-1, (d.mean().item(), d.max().item())      # (two results of the mode: its noise floor)
    finally:
        R.GROUP_DOWN_ANGLES = was
        ops.set_mlp_precision(old)


def _vs_oracle(y, ref):
    """(mean, p99.9, max, elements above 3e-2) of |y - ref|."""
    d = (y.cpu().double() - ref.double()).abs().flatten()
    return d.mean().item(), d.kthvalue(int(0.999 * d.numel())).values.item(), d.max().item(), int((d > 3e-2).sum())


def test_remus_bf16_mode_switches_one_at_a_time():
    """Every switch of the rounded-bf16 mode's REMuS path turned off alone (the combinations a user can reach through the module
    attributes / G4C_* environment variables): the forward runs, and agrees with the default path to the mode's noise floor.  The
    switches that change a summation order or add / remove a rounding (the others are bit-identical: next test) must moreover leave the
    forward as accurate as the default against the fp32 oracle — mean and p99.9 within 1.15x of the default's — and differ from the
    default by no more than two results of the mode differ (measured: mean <= 2.2e-3, p99.9 <= 1.4e-2, max <= 5.9e-2;
    profiles/r07_remus_bf16_switches.log)."""
    from graphs4cfd_amd.nn import remus_gnn as R
    old = ops.set_mlp_precision("bf16")
    switches = [(B, "COMPACT_MESSAGES"), (B, "HOIST_BF16"), (B, "PRODUCTS_BF16"), (B, "ROW_SPLIT_BF16"), (B, "AGGREGATE_BF16"),
                (B, "COMPACT_LATENTS"), (B, "UPDATE_ROW_SPLIT"), (R, "ENTRY_PRODUCTS"), (R, "GROUP_DOWN_ANGLES"), (R, "LAST_COMPACT")]
    reordering = {"HOIST_BF16", "PRODUCTS_BF16", "ROW_SPLIT_BF16", "AGGREGATE_BF16", "UPDATE_ROW_SPLIT", "GROUP_DOWN_ANGLES"}
    try:
        g = S.remus_graph(20_000, k=5, seed=81).to(DEV)
        torch.manual_seed(82)
        model = gfd.nn.NsRotEquiTreeScaleGNN(arch=S.remus_arch(128), device=DEV)
        oracle = O.remus_forward(S.remus_graph(20_000, k=5, seed=81).to_dict(), {k: v.cpu() for k, v in model.state_dict().items()})
        with torch.no_grad():
            ref = model.forward(g.clone()).clone()
        base = _vs_oracle(ref, oracle)
        print(f"default vs oracle: mean {base[0]:.3e} p99.9 {base[1]:.3e} max {base[2]:.3e} above 3e-2 {base[3]}")
        for mod, name in switches:
            was = getattr(mod, name)
            setattr(mod, name, False)
            try:
                with torch.no_grad():
                    y = model.forward(g.clone())
                d = (y - ref).abs()
                assert torch.isfinite(y).all() and d.mean().item() < 1e-2 and d.max().item() < 1e-1, (name, d.mean().item(), d.max().item())
                if name in reordering:
                    p999 = d.flatten().kthvalue(int(0.999 * d.numel())).values.item()
                    off = _vs_oracle(y, oracle)
                    print(f"{name} off: vs default mean {d.mean().item():.3e} p99.9 {p999:.3e} max {d.max().item():.3e}; vs oracle mean {off[0]:.3e} "
                          f"({off[0] / base[0]:.3f}x) p99.9 {off[1]:.3e} ({off[1] / base[1]:.3f}x) max {off[2]:.3e} above 3e-2 {off[3]}")
                    assert d.mean().item() < 3e-3 and p999 < 2e-2 and d.max().item() < 8e-2, (name, d.mean().item(), p999, d.max().item())
                    assert off[0] <= 1.15 * base[0] and off[1] <= 1.15 * base[1], (name, off, base)
            finally:
                setattr(mod, name, was)
    finally:
        ops.set_mlp_precision(old)


@pytest.mark.parametrize("name", ["LAST_COMPACT"])
def test_remus_bf16_bit_identical_switches(name):
    """The representation-only switches give the forward bit for bit.  COMPACT_MESSAGES, ENTRY_PRODUCTS and COMPACT_LATENTS have tests
    of their own (test_remus_bf16_compact_messages_are_bit_identical, test_remus_entry_products_come_from_the_producer_launch,
    test_remus_compact_edge_latents_are_the_same_operand); this one covers the compact latents a run leaves behind (remus_gnn.LAST_COMPACT).
    Compact latents decide whether an update MLP becomes eligible for mlp_rs2_kernel (another summation order), so blocks.UPDATE_ROW_SPLIT
    is pinned off, kernel for kernel, as those tests do (DESIGN states the condition)."""
    from graphs4cfd_amd.nn import remus_gnn as R
    mod = R if name in ("ENTRY_PRODUCTS", "LAST_COMPACT") else B
    pin = name != "COMPACT_MESSAGES"
    old = ops.set_mlp_precision("bf16")
    was, was_u = getattr(mod, name), B.UPDATE_ROW_SPLIT
    try:
        if pin:
            B.UPDATE_ROW_SPLIT = False
        g = S.remus_graph(20_000, k=5, seed=83).to(DEV)
        torch.manual_seed(84)
        model = gfd.nn.NsRotEquiTreeScaleGNN(arch=S.remus_arch(128), device=DEV)
        outs = {}
        for on in (True, False):
            setattr(mod, name, on)
            with torch.no_grad():
                outs[on] = model.forward(g.clone()).clone()
        assert torch.isfinite(outs[True]).all()
        assert torch.equal(outs[True], outs[False]), (name, (outs[True] - outs[False]).abs().max().item())
    finally:
        setattr(mod, name, was)
        B.UPDATE_ROW_SPLIT = was_u
        ops.set_mlp_precision(old)


@pytest.mark.parametrize("seed", [21, 23, 25])
def test_remus_20k_bf16_default_path_as_accurate_as_the_tile_path(seed):
    """Config 3's model at 20k nodes in the rounded-bf16 mode: the default path (row-split kernels, compact rows, bf16 aggregates) is as
    accurate against the fp32 oracle as the tile path of the same mode (blocks.ROW_SPLIT_BF16 = UPDATE_ROW_SPLIT = False, RS1_MIN_ROWS out
    of reach): mean and p99.9 within 1.15x of the tile path's; at most 16 of the default path's 40 000 outputs above 3e-2 (measured: 1 - 8 on
    the default path, 1 - 11 on the tile path, over these seeds: profiles/r07_remus_bf16_switches.log).  The largest deviation is not
    bounded tighter than test_remus_20k_vs_oracle's 1e-1: on seed 21 it is 6.5e-2 on the default path (same log)."""
    old = ops.set_mlp_precision("bf16")
    was = B.ROW_SPLIT_BF16, B.UPDATE_ROW_SPLIT, B.RS1_MIN_ROWS
    try:
        g = S.remus_graph(20_000, k=5, seed=seed)
        torch.manual_seed(seed + 1)
        model = gfd.nn.NsRotEquiTreeScaleGNN(arch=S.remus_arch(128), device=DEV)
        ref = O.remus_forward(g.to_dict(), {k: v.cpu() for k, v in model.state_dict().items()})
        res = {}
        for path in ("default", "tile"):
            B.ROW_SPLIT_BF16, B.UPDATE_ROW_SPLIT, B.RS1_MIN_ROWS = was if path == "default" else (False, False, 1 << 40)
            with torch.no_grad():
                y = model.forward(g.clone().to(DEV))
            assert torch.isfinite(y).all()
            res[path] = _vs_oracle(y, ref)
        (m0, p0, x0, c0), (m1, p1, x1, c1) = res["default"], res["tile"]
        print(f"seed {seed}: default mean {m0:.3e} p99.9 {p0:.3e} max {x0:.3e} above 3e-2 {c0} | tile mean {m1:.3e} p99.9 {p1:.3e} max {x1:.3e} "
              f"above 3e-2 {c1} | ratios {m0 / m1:.3f} {p0 / p1:.3f}")
        assert m0 <= 1.15 * m1 and p0 <= 1.15 * p1, res
        assert c0 <= 16, res
    finally:
        B.ROW_SPLIT_BF16, B.UPDATE_ROW_SPLIT, B.RS1_MIN_ROWS = was
        ops.set_mlp_precision(old)


def test_bf16_product_rows_are_exact_copies():
    """Rounded-bf16 mode, round 5 (blocks.PRODUCTS_BF16): the hoisted first-layer products are stored as bf16.  The kernels only
    change representation — (a) head rows / plain output rows stored as bf16 are the round-to-nearest bf16 of the fp32 rows the same
    launch stores otherwise; (b) a message launch that gathers bf16 additive rows gives bit for bit what it gives for their fp32
    widening, on the weight-stationary kernel (large launch, fused aggregation) and on the tile kernel (small launch)."""
    lib = _lib.load()
    old = ops.set_mlp_precision("bf16")
    try:
        torch.manual_seed(91)
        H = 128
        blk = B.GNBlock((3 * H, (H, H), True), (2 * H, (H, H), True)).to(DEV)
        nxt = B.GNBlock((3 * H, (H, H), True), (2 * H, (H, H), True)).to(DEV)
        n = 12000                      # (>= the 10 000 targets of the larger message launch below)
        v, agg = torch.randn(n, H, device=DEV), torch.randn(n, H, device=DEV)
        with torch.no_grad():
            was = B.PRODUCTS_BF16
            try:
                B.PRODUCTS_BF16 = False
                y32, h32 = blk.node_mlp.run_with_heads([ops.Source(agg), ops.Source(v)], n, _lib.ACT_SELU, nxt.edge_mlp, H, [H, H])
                B.PRODUCTS_BF16 = True
                y16, h16 = blk.node_mlp.run_with_heads([ops.Source(agg), ops.Source(v)], n, _lib.ACT_SELU, nxt.edge_mlp, H, [H, H])
            finally:
                B.PRODUCTS_BF16 = was
            assert h16[0].dtype == torch.bfloat16 and h32[0].dtype == torch.float32 and torch.equal(y32, y16)
            for a, b in zip(h32, h16):
                assert torch.equal(a.to(torch.bfloat16), b)
            # plain launch: the first layer's block alone (MLP.run_hoisted's "hoist1" launch)
            pk1 = nxt.edge_mlp._packed_cols(H, 2 * H, [H], [False], True)
            p32 = ops.mlp_forward(pk1, [ops.Source(v)], n)
            p16 = ops.mlp_forward(pk1, [ops.Source(v)], n, out=torch.empty(n, H, dtype=torch.bfloat16, device=DEV))
            assert torch.equal(p32.to(torch.bfloat16), p16)
            # the consumer: bf16 additive rows == their fp32 widening
            pk = nxt.edge_mlp._packed_cols(0, H, [H], [False], False)
            for rows, deg in ((60000, 6), (900, 6)):
                nn_ = rows // deg
                e = torch.randn(rows, H, device=DEV)
                colh = torch.arange(nn_).repeat_interleave(deg)
                ei = torch.stack([torch.randint(0, nn_, (rows,)), colh]).to(DEV)
                ep, csr = plan.edge_csr(ei, nn_)
                pr16, pc16 = h16[0][:nn_].contiguous(), h16[1][:nn_].contiguous()
                outs = []
                for pr, pc in ((pr16, pc16), (pr16.float(), pc16.float())):
                    src = [ops.Source(e, pre_act=_lib.ACT_SELU), ops.Source(pr, index=ep.row, additive=True), ops.Source(pc, index=ep.col, additive=True)]
                    ag = torch.empty(nn_, H, device=DEV)
                    y = ops.mlp_forward(pk, src, rows, agg=(csr, ag, True))
                    outs.append((y.clone(), ag.clone(), int(lib.g4c_mlp_last_kernel())))
                assert outs[0][2] == outs[1][2]
                assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), rows
            # fp32 additive rows in another arithmetic are refused loudly
        ops.set_mlp_precision("f16x3")
        pkf = nxt.edge_mlp._packed_cols(0, H, [H], [False], False)
        with pytest.raises(NotImplementedError, match="rounded-bf16 mode"):
            ops.mlp_forward(pkf, [ops.Source(e), ops.Source(pr16, index=ep.row, additive=True), ops.Source(pc16, index=ep.col, additive=True)], rows)
    finally:
        ops.set_mlp_precision(old)


def test_product_image_in_row_split_order_is_an_image_of_its_own():
    """Rounded-bf16 mode: one MLP asked for the first-layer product image of the same columns with and without the row-split output order
    (MLP._packed_cols rs_rows) packs two images — the order is part of the cache key (blocks.PackSpec) — and the second one's product is
    the first one's with its columns taken in ops._rs_k_order, bit for bit: the weight's rows are permuted, every output column is the
    same sum."""
    old = ops.set_mlp_precision("bf16")
    try:
        torch.manual_seed(93)
        H, n = 128, 3000
        m = B.MLP(3 * H, (H, H, H), True).to(DEV)
        v = torch.randn(n, H, device=DEV)
        pk_nat = m._packed_cols(H, 2 * H, [H], [False], True)
        pk_rs = m._packed_cols(H, 2 * H, [H], [False], True, rs_rows=True)
        assert pk_nat is not pk_rs
        assert m._packed_cols(H, 2 * H, [H], [False], True) is pk_nat and m._packed_cols(H, 2 * H, [H], [False], True, rs_rows=True) is pk_rs
        order = ops._rs_k_order(DEV)
        for dtype in (torch.bfloat16, torch.float32):
            nat = ops.mlp_forward(pk_nat, [ops.Source(v)], n, out=torch.empty(n, H, dtype=dtype, device=DEV))
            rs = ops.mlp_forward(pk_rs, [ops.Source(v)], n, out=torch.empty(n, H, dtype=dtype, device=DEV))
            assert nat.abs().max().item() > 0 and not torch.equal(rs, nat)
            assert torch.equal(rs, nat[:, order]), dtype
    finally:
        ops.set_mlp_precision(old)


@pytest.mark.parametrize("family", ["mus", "remus"])
def test_a_warm_forward_packs_no_weights(family, monkeypatch):
    """Every packed weight image of a model is cached by its MLP: the second forward constructs no ops.PackedMLP, and after
    model.invalidate_packed() the next forward constructs exactly the images the first one did.  A MuS-GNN in the default arithmetic
    (hoisted first layers, products from the producer's launch, one launch per MP layer) and REMuS-GNN in the rounded-bf16 mode (the
    row-split kernels' streams and orders)."""
    built = []
    init = ops.PackedMLP.__init__

    def counting(self, *a, **kw):
        built.append(1)
        init(self, *a, **kw)
    monkeypatch.setattr(ops.PackedMLP, "__init__", counting)
    old = ops.set_mlp_precision("f16x3" if family == "mus" else "bf16")
    try:
        torch.manual_seed(94)
        if family == "mus":
            g = S.mus_graph(8000, levels=2, seed=3).to(DEV)
            model = gfd.nn.NsTwoScaleGNN(arch=S.mus_arch("NsTwoScaleGNN", 128), device=DEV)
        else:
            g = S.remus_graph(20_000, k=5, seed=31).to(DEV)
            model = gfd.nn.NsRotEquiTreeScaleGNN(arch=S.remus_arch(128), device=DEV)
        first = model.forward(g.clone()).clone()
        n_first = len(built)
        assert n_first > 0
        again = model.forward(g.clone()).clone()
        assert len(built) == n_first, f"a warm forward packed {len(built) - n_first} images"
        model.invalidate_packed()
        third = model.forward(g.clone())
        assert len(built) == 2 * n_first, (n_first, len(built))
        assert torch.equal(first, again) and torch.equal(first, third)
    finally:
        ops.set_mlp_precision(old)


# ------------------------------------------------------------------ one launch per MP layer (round 5)
@pytest.mark.parametrize("layers", [3, 2])
def test_fused_mp_layer_matches_the_separate_launches(layers):
    """ops.mp_layer_forward / g4c_mlp_io_t.upd (message MLP + aggregation + node MLP + the next layer's products in one
    launch; reference nn/blocks.py:175-186) against the separate launches of the same GNBlock, at sizes from less than one tile to
    several tile pairs per workgroup, constant and ragged in-degrees (empty segments, trailing targets without edges: node tiles of
    1 .. 64 rows per workgroup), with and without heads, with and without stored messages.  Same arithmetic per element; sums over k
    are associated as in the weight-stationary kernel (the node update otherwise runs on the 32x32x16 tile kernel): 2e-5."""
    H = 128
    old = ops.set_mlp_precision("f16x3")
    was = (B.FUSE_LAYER, B.FUSE_LAYER_MIN_ROWS)
    try:
        torch.manual_seed(100 + layers)
        hid = (H,) * layers
        blk = B.GNBlock((3 * H, hid, True), (2 * H, hid, True)).to(DEV)
        nxt = B.GNBlock((3 * H, hid, True), (2 * H, hid, True)).to(DEV)
        W1 = nxt.edge_mlp._linears()[0].weight
        B.FUSE_LAYER_MIN_ROWS = 1
        for n, deg, ragged in ((6, 6, False), (37, 6, True), (1500, 6, True), (12500, 6, False), (20000, 4, True)):
            gen = torch.Generator().manual_seed(n)
            if ragged:
                d = torch.randint(0, 2 * deg + 1, (n,), generator=gen); d[0] = 0; d[-3:] = 0
            else:
                d = torch.full((n,), deg)
            col = torch.arange(n).repeat_interleave(d)
            ei = torch.stack([torch.randint(0, n, (int(col.numel()),), generator=gen), col]).to(DEV)
            E = int(ei.size(1))
            v, e = torch.randn(n, H, device=DEV), torch.randn(E, H, device=DEV)
            for heads, keep in ((True, True), (False, True), (True, False), (False, False)):
                res = []
                with torch.no_grad():
                    for fuse in (False, True):
                        B.FUSE_LAYER = fuse
                        res.append(blk.step(v, e, ei, _lib.ACT_SELU, e_pre_act=_lib.ACT_SELU, next_msg=nxt.edge_mlp if heads else None, keep_e=keep))
                tag = (layers, n, E, heads, keep)
                torch.testing.assert_close(res[1][0], res[0][0], rtol=0, atol=2e-5, msg=lambda m: f"v' {tag}: {m}")
                if keep:
                    torch.testing.assert_close(res[1][1], res[0][1], rtol=0, atol=2e-5, msg=lambda m: f"e' {tag}: {m}")
                else:
                    assert res[1][1] is None
                if heads:      # (the separate form makes products from HOIST_MIN_ROWS edges on only: otherwise compare with W1 v')
                    assert res[1][2] is not None
                    for j in range(2):
                        want = res[0][2][j] if res[0][2] is not None else res[0][0] @ W1[:, H * (1 + j):H * (2 + j)].T
                        torch.testing.assert_close(res[1][2][j], want, rtol=0, atol=2e-5 if res[0][2] is not None else 1e-4)
        # a whole model: every MP layer of the levels inside the size window runs fused; eager == hipGraph-replayed, bit for bit
        B.FUSE_LAYER_MIN_ROWS = was[1]
        g = S.mus_graph(4000, levels=3, seed=12)
        torch.manual_seed(13)
        model = gfd.nn.NsThreeScaleGNN(arch=S.mus_arch("NsThreeScaleGNN", 128), device=DEV)
        w = {k: v.cpu() for k, v in model.state_dict().items()}
        ref = O.mus_solve("NsThreeScaleGNN", g.to_dict(), w, 4, model.num_fields)
        outs = {}
        for fuse in (False, True):
            B.FUSE_LAYER = fuse
            for capture in (False, True):
                outs[(fuse, capture)] = model.solve(g.clone(), 4, capture=capture)
        assert torch.equal(outs[(True, False)], outs[(True, True)])
        torch.testing.assert_close(outs[(True, True)], outs[(False, True)], rtol=0, atol=1e-4)
        torch.testing.assert_close(outs[(True, True)].cpu(), ref, rtol=1e-3, atol=1e-3)
    finally:
        B.FUSE_LAYER, B.FUSE_LAYER_MIN_ROWS = was
        ops.set_mlp_precision(old)


# ------------------------------------------------------------------ per-mesh constants are cached across rollout steps (round 4)
def _manual_rollout(model, g, field, n_out):
    """solve() spelled out with bare forward() calls (which never use the cache); n_in = 1: the next input is the prediction.
    Returns ([N, nf * n_out], last prediction)."""
    outs = []
    with torch.no_grad():
        for _ in range(n_out):
            g.field = field
            field = model.forward(g).clone()
            outs.append(field)
    return torch.cat(outs, dim=1), field


@pytest.mark.parametrize("family", ["mus", "remus"])
def test_static_encoder_cache_is_bit_identical_and_invalidates(family):
    """Rollout computes selu(edge_encoder(edge_attr)) (MuS-GNN; reference nn/mus_gnn.py:73,178) / the five angle encoders (REMuS-GNN;
    nn/remus_gnn.py:136-140) ONCE: nn/model.py:316-320 replaces graph.field only.  Same bits as launching them every step; an
    in-place edit of the static input or new weights recompute; a bare forward() never touches the cache."""
    from graphs4cfd_amd.nn.model import Rollout
    if family == "mus":
        g = S.mus_graph(4000, levels=2, seed=71).to(DEV)
        torch.manual_seed(72)
        model = gfd.nn.NsTwoScaleGNN(arch=S.mus_arch("NsTwoScaleGNN", 128), device=DEV)
        static_attr, n_static = "edge_attr", 1
    else:
        g = S.remus_graph(3000, k=5, seed=73).to(DEV)
        torch.manual_seed(74)
        model = gfd.nn.NsRotEquiTreeScaleGNN(arch=S.remus_arch(128), device=DEV)
        static_attr, n_static = "angle_attr", 5
    g.batch = torch.zeros(g.num_nodes, dtype=torch.long, device=DEV)
    f0 = g.field.clone()
    assert f0.size(1) == model.num_fields
    ref, _ = _manual_rollout(model, g, f0.clone(), 4)
    for capture in (False, True):
        g.field = f0.clone()
        with Rollout(model, g, 4, capture=capture, reorder=False) as ro:
            ro.run(4)
            assert ro.static.misses == n_static and ro.static.hits == n_static * (1 if capture else 3), (ro.static.misses, ro.static.hits)
            assert torch.equal(ro.result(), ref), (ro.result() - ref).abs().max().item()
    assert ops.StaticCache.active is None
    # an in-place edit of the static input between two steps of ONE rollout is seen (version counter), as are new weights
    att = getattr(g, static_attr)
    att0 = att.clone()
    g.field = f0.clone()
    with Rollout(model, g, 4, capture=False, reorder=False) as ro:
        ro.run(2)
        att.mul_(1.5)
        ro.run(1)
        assert ro.static.misses == n_static + 1
        model.invalidate_packed()
        ro.run(1)
        assert ro.static.misses == 2 * n_static + 1
        got = ro.result().clone()
    # (the same edit at the same step with every launch executed)
    att.copy_(att0)
    a, last = _manual_rollout(model, g, f0.clone(), 2)
    att.mul_(1.5)
    b, _ = _manual_rollout(model, g, last, 2)
    assert torch.equal(got, torch.cat([a, b], dim=1))
    # ... and by a CAPTURED rollout: the replayed step contains neither the encoder launches nor a look-up, so the
    # rollout checks its cache before every replay, runs one eager step when an entry is stale and captures again
    att.copy_(att0)
    g.field = f0.clone()
    with Rollout(model, g, 6, capture=True, reorder=False) as ro:
        ro.run(3)                                # eager, captured, replayed
        assert ro._hipgraph is not None
        att.mul_(1.5)
        ro.run(1)                                # stale: eager again
        assert ro.static.misses == n_static + 1
        ro.run(2)                                # captured again, replayed
        assert ro._hipgraph is not None
        got = ro.result().clone()
    att.copy_(att0)
    a, last = _manual_rollout(model, g, f0.clone(), 3)
    att.mul_(1.5)
    b, _ = _manual_rollout(model, g, last, 3)
    assert torch.equal(got, torch.cat([a, b], dim=1))
    att.copy_(att0)


def test_f16_range_report_is_scoped_to_the_model_that_clipped():
    """A clip in model A's launches must not be reported by model B's solve() (a rollout reads the flags of its own launches only:
    ops.RangeFlags; launches outside any consumer go to the device's default flags, which f16_range_report reads), and it must still
    be reported when A is asked."""
    import warnings
    old = ops.set_mlp_precision("f16x3")
    try:
        ops.f16_range_clear()                               # (whatever earlier tests left behind)
        g = S.mus_graph(2500, levels=2, seed=81)
        torch.manual_seed(82)
        a = gfd.nn.NsTwoScaleGNN(arch=S.mus_arch("NsTwoScaleGNN", 128), device=DEV)
        b = gfd.nn.NsOneScaleGNN(arch=S.mus_arch("NsOneScaleGNN", 128), device=DEV)
        g1 = S.mus_graph(2500, levels=1, seed=83)
        with torch.no_grad():
            a.mp111.edge_mlp.MLP.layer_norm.weight.mul_(3e4)
        a.invalidate_packed()
        ga = g.clone().to(DEV)
        ga.batch = torch.zeros(ga.num_nodes, dtype=torch.long, device=DEV)
        was = gfd.set_forward_validation(False)             # (a validated bare forward would deal with its clip itself)
        try:
            with torch.no_grad():
                a.forward(ga)                               # bare forward: sets A's flags, nobody asked yet
        finally:
            gfd.set_forward_validation(was)
        # a clip of an MLP that belongs to no model at all (the stale flag GPUTEST_r03 showed in an unrelated test's warnings)
        mlp = B.MLP(128, (128, 128), True).to(DEV)
        mlp(torch.full((64, 128), 1e5, device=DEV))
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)
            b.solve(g1.clone(), 2)                          # B did not clip: silent
        hit = ops.f16_range_report(DEV, clear=False)
        assert any(h.startswith("NsTwoScaleGNN.mp11") for h in hit) and any("outside a model" in h for h in hit), hit
        with pytest.warns(RuntimeWarning, match="NsTwoScaleGNN.mp11"):
            gfd.check_f16_range(torch.device("cuda"), sites=a._range_sites)        # (un-indexed device = the current one)
        # A's own solve(): the flags of its earlier forward are not its own, its own clip is reported, nothing else
        with pytest.warns(RuntimeWarning) as rec:
            a.solve(g.clone(), 2)
        msgs = [str(r.message) for r in rec if "fp16 range" in str(r.message)]
        assert msgs and all("outside a model" not in m and "NsOneScaleGNN" not in m for m in msgs), msgs
        assert ops.f16_range_report(DEV) == ["an MLP created outside a model"]
    finally:
        ops.set_mlp_precision(old)


def test_f16_range_flags_belong_to_the_consumer_that_launched():
    """The flags a launch writes belong to whoever issued it (ops.RangeFlags).  (a) `with Rollout(...) as ro: ro.run(n)`, then
    `ro.result()` outside the block: the clip of its steps is still its own — warned and recomputed, the result is the bf16x6 solve
    bit for bit, and the caller's graph keeps its field.  (b) Live, unclosed rollouts of the same model (a Rollout and a world-1
    DistributedRollout) neither hide the clip of a bare forward with validation off from f16_range_report() nor are blamed for it.
    (c) The clip of a forward recorded for autograd is not blamed on the next validated bare forward (no warning, no second pass),
    and check_f16_range() still reports it."""
    import warnings
    from graphs4cfd_amd import partition as P
    from graphs4cfd_amd.nn.model import Rollout
    g = S.mus_graph(3000, levels=2, seed=18)
    torch.manual_seed(19)
    model = gfd.nn.NsTwoScaleGNN(arch=S.mus_arch("NsTwoScaleGNN", 128), device=DEV)
    old = ops.set_mlp_precision("f16x3")
    try:
        ops.f16_range_clear()                               # (whatever earlier tests left behind)
        gd = g.clone().to(DEV)
        gd.batch = torch.zeros(gd.num_nodes, dtype=torch.long, device=DEV)
        big = gd.clone(); big.field = big.field * 1e5
        f_big = big.field
        # (a)
        with Rollout(model, big, 5, capture=True, reorder=False) as ro:
            ro.run(5)
        with pytest.warns(RuntimeWarning, match="recomputed in 'bf16x6'"):
            got = ro.result().clone()
        assert ro.exact_range and big.field is f_big
        assert ops.f16_range_report() == []                 # (the rollout's clip never reached the default flags)
        ops.set_mlp_precision("bf16x6")
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                 # (solve() notes inputs beyond 4096 in either arithmetic)
            ref = model.solve(big.clone(), 5, capture=True)
        ops.set_mlp_precision("f16x3")
        assert torch.equal(got, ref), (got - ref).abs().max().item()
        # (b)
        ro = Rollout(model, gd, 4, capture=True, reorder=False)
        ro.run(2)
        dr = P.DistributedRollout(model, g, 4, 0, 1, DEV)
        dr.run(2)
        was = gfd.set_forward_validation(False)
        try:
            with torch.no_grad(), warnings.catch_warnings():
                warnings.simplefilter("error", RuntimeWarning)
                model.forward(big)
        finally:
            gfd.set_forward_validation(was)
        hit = ops.f16_range_report()
        assert any(h.startswith("NsTwoScaleGNN.") for h in hit), hit
        with warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)
            assert not ro.validate() and not dr.validate()
        ro.close()
        # (c)
        with torch.enable_grad():
            y = model.forward(big)
        assert y.requires_grad
        del y
        with torch.no_grad(), warnings.catch_warnings():
            warnings.simplefilter("error", RuntimeWarning)
            model.forward(gd)
        with pytest.warns(RuntimeWarning, match="NsTwoScaleGNN"):
            assert ops.check_f16_range()
        assert ops.f16_range_report() == []
    finally:
        ops.set_mlp_precision(old)


def test_mean_div_is_the_ieee_quotient():
    """g4c::mean_div4 (the quotient of the fused aggregation's mean in mlp_ws_kernel: shared reciprocal + one FMA correction per value,
    the division itself for everything unusual) against torch's fp32 division, bit for bit: every count up to 4200 (past the routine's
    own limit) with random numerators of several magnitudes; the whole binade [1, 2) of numerators for small counts; zeros, subnormal
    quotients, infinities, NaNs."""
    lib = _lib.load()

    def run(a, cnt):
        a = a.contiguous(); cnt = cnt.to(torch.int32).contiguous(); out = torch.empty_like(a)
        rc = lib.g4c_debug_mean_div(a.data_ptr(), cnt.data_ptr(), out.data_ptr(), a.numel() // 4, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, _lib.last_error()
        return out

    def check(a, cnt, what):
        got, ref = run(a, cnt), a / cnt.float().repeat_interleave(4)
        same = (got.view(torch.int32) == ref.view(torch.int32)) | (torch.isnan(got) & torch.isnan(ref))
        assert bool(same.all()), (what, a[~same][:4], cnt.repeat_interleave(4)[~same][:4], got[~same][:4], ref[~same][:4])

    g = torch.Generator(device=DEV).manual_seed(0)
    counts = torch.arange(1, 4201, device=DEV)
    for scale in (1.0, 1e-3, 37.0, 1e30, 1e-30):
        cnt = counts.repeat_interleave(256)
        a = torch.randn(cnt.numel() * 4, device=DEV, generator=g) * scale
        check(a, cnt, f"random numerators x {scale}")
    binade = (torch.arange(1 << 23, device=DEV, dtype=torch.int32) + 0x3F800000).view(torch.float32)       # every float in [1, 2)
    for c in (3, 5, 6, 7, 9, 11, 13, 127, 4095):
        check(binade, torch.full((binade.numel() // 4,), c, device=DEV), f"binade, count {c}")
    special = torch.tensor([0.0, -0.0, 1e-45, -3e-39, 1e-38, 2e-38, float("inf"), -float("inf"), float("nan"), 3.4e38, 1.0, -1.0], device=DEV)
    for c in (1, 3, 6, 4096, 4097, 100000):
        a = special.repeat_interleave(4)[: special.numel() * 4].reshape(-1, 4).repeat(1, 1).reshape(-1)
        check(a, torch.full((a.numel() // 4,), c, device=DEV), f"special values, count {c}")


@pytest.mark.parametrize("width", [1, 33, 128, 200, 1024, 1500])
def test_layer_norm_rows(width):
    """g4c_layer_norm against torch.nn.functional.layer_norm (fp64) on rows of any width, strided views, in place, with an activation."""
    torch.manual_seed(width)
    x = torch.randn(301, width + 5, device=DEV)[:, 2:2 + width] * 3.0 + 0.7
    g, b = torch.randn(width, device=DEV), torch.randn(width, device=DEV)
    ref = torch.nn.functional.layer_norm(x.double(), (width,), g.double(), b.double(), 1e-5).float()
    torch.testing.assert_close(ops.layer_norm(x, g, b, 1e-5), ref, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(ops.layer_norm(x, None, None, 1e-5, _lib.ACT_SELU),
                               torch.nn.functional.selu(torch.nn.functional.layer_norm(x.double(), (width,), None, None, 1e-5)).float(), rtol=1e-5, atol=1e-5)
    y = x.clone()
    assert ops.layer_norm(y, g, b, 1e-5, out=y) is y
    torch.testing.assert_close(y, ref, rtol=1e-5, atol=1e-5)
