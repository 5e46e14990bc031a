"""Every launch form of the rounded-bf16 mode (`set_mlp_precision("bf16")`, BASELINE config 3) against an fp64 restatement of its own
arithmetic (oracle/bf16_ref.py): the tile / small-launch kernel, mlp_ws_kernel<SP = 1>, mlp_rs1_kernel, mlp_rs2_kernel and the hoisted
product launches.  Each test asserts which kernel ran (g4c_mlp_last_kernel), so it cannot quietly test another one.  The bounds are
oracle/bf16_ref.py NOISE (derived on CPU: scripts/bf16_noise_bounds.py, profiles/r07_bf16_noise_bounds.log); the negative controls
perturb only the reference and assert that the checker then rejects the kernel's output."""
import contextlib

import pytest
import torch

from graphs4cfd_amd import _lib, ops, plan
from graphs4cfd_amd.nn import blocks as B
from oracle import bf16_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
H = 128
TILE, WS, RS1, RS2 = 2, 4, _lib.KERNEL_MLP_RS, _lib.KERNEL_MLP_RS2
SELU = _lib.ACT_SELU


@contextlib.contextmanager
def bf16_mode(ws: int = 0):
    """The rounded-bf16 mode, the weight-stationary kernel off (0) or taking every launch it can (2), the dual-tile kernel off."""
    lib = _lib.load()
    old = ops.set_mlp_precision("bf16")
    old_ws, old_i = lib.g4c_mlp_ws_enable(ws), lib.g4c_mlp_bx6i_enable(0)
    try:
        with torch.no_grad():
            yield lib
    finally:
        lib.g4c_mlp_ws_enable(old_ws)
        lib.g4c_mlp_bx6i_enable(old_i)
        ops.set_mlp_precision(old)


def last_kernel() -> int:
    return int(_lib.load().g4c_mlp_last_kernel())


def make_mlp(k_in: int, layers: int, ln: bool, seed: int) -> B.MLP:
    torch.manual_seed(seed)
    m = B.MLP(k_in, (H,) * layers, ln)
    if ln:          # (a LayerNorm with a gain / shift of its own: the kernels must apply both)
        with torch.no_grad():
            m.MLP.layer_norm.weight.copy_(1.0 + 0.1 * torch.randn(H))
            m.MLP.layer_norm.bias.copy_(0.1 * torch.randn(H))
    return m.to(DEV)


def sd(m) -> dict:
    return {k: t.detach().cpu() for k, t in m.state_dict().items()}


def nat(t):
    return ops.rs_rows_to_natural(t) if isinstance(t, ops.RsOrderedRows) else t


def to_rs(t):
    """bf16 rows [n, 128] in feature order -> the same rows in the row-split kernel's column order, tagged."""
    return ops.RsOrderedRows.tag(t[:, ops._rs_k_order(t.device)].contiguous())


def check(got, ref, kind, what):
    s = R.assert_bf16_order_noise(nat(got).float(), ref, kind, what)
    print(f"[bf16-noise] {what} {kind}: mean {s['mean']:.3e} frac {s['frac']:.3e} max {s['max']:.3e} row_count {s['row_count']}")
    return s


def uniform_edges(n: int, K: int, seed: int):
    g = torch.Generator().manual_seed(seed)
    E = n * K
    ei = torch.stack([torch.randint(0, n, (E,), generator=g), torch.arange(n).repeat_interleave(K)]).to(DEV)
    ep, csr = plan.edge_csr(ei, n)
    assert csr.uniform_deg == K and csr.perm is None and csr.tiles() is not None
    return E, ep, csr


# ------------------------------------------------------------------ tile / small-launch kernel
@pytest.mark.parametrize("layers,ln", [(2, True), (3, True), (2, False), (3, False)], ids=lambda x: str(x))
@pytest.mark.parametrize("rows", [1, 33, 700, 5000])
def test_tile_kernel_vs_reference(rows, layers, ln):
    """Plain launches: [SELU(e) | v[row] | v[col]] with gathers; the same with bf16 source rows; a node MLP with a narrow 3-wide block and
    tanh; the hoisted form with fp32 and with bf16 additive product rows."""
    n = max(rows // 6, 1)
    g = torch.Generator().manual_seed(rows + 10 * layers + ln)
    e, v = torch.randn(rows, H, generator=g).to(DEV), torch.randn(n, H, generator=g).to(DEV)
    row, col = (torch.randint(0, n, (rows,), generator=g).to(DEV, torch.int32) for _ in range(2))
    x3 = torch.randn(rows, 3, generator=g).to(DEV)
    m = make_mlp(3 * H, layers, ln, rows + layers)
    node = make_mlp(2 * H + 3, layers, ln, rows + layers + 1)
    w, wn = sd(m), sd(node)
    with bf16_mode():
        y = m.run_coded([ops.Source(e, pre_act=SELU), ops.Source(v, index=row), ops.Source(v, index=col)], rows)
        assert last_kernel() == TILE
        check(y, R.mlp(w, [R.Block(e, pre_act="selu"), R.Block(v, index=row), R.Block(v, index=col)], rows), "rows32", "gathers")
        e16 = torch.nn.functional.selu(e).to(torch.bfloat16)
        y = m.run_coded([ops.Source(e16), ops.Source(v, index=row), ops.Source(v, index=col)], rows)
        assert last_kernel() == TILE
        check(y, R.mlp(w, [R.Block(e16), R.Block(v, index=row), R.Block(v, index=col)], rows), "rows32", "bf16 source rows")
        y = node.run_coded([ops.Source(e), ops.Source(e), ops.Source(x3)], rows, _lib.ACT_TANH)
        assert last_kernel() == TILE
        check(y, R.mlp(wn, [R.Block(e), R.Block(e), R.Block(x3, narrow=True)], rows, act="tanh"), "rows32", "narrow block")
        pk = m._packed_cols(0, H, [H], [False], False)
        W1 = w["MLP.linear_1.weight"]
        for bf16_adds in (False, True):
            pr, pc = (R.products(W1[:, a:a + H], v, bf16_out=bf16_adds) for a in (H, 2 * H))
            dt = torch.bfloat16 if bf16_adds else torch.float32
            src = [ops.Source(e, pre_act=SELU), ops.Source(pr.to(DEV, dt), index=row, additive=True),
                   ops.Source(pc.to(DEV, dt), index=col, additive=True)]
            y = ops.mlp_forward(pk, src, rows)
            assert last_kernel() == TILE
            ref = R.mlp(w, [R.Block(e, pre_act="selu")], rows, additive=[R.Additive(pr, row), R.Additive(pc, col)], first_cols=(0, H))
            check(y, ref, "rows32", f"hoisted, {dt} additive rows")


@pytest.mark.parametrize("rows", [33, 5000])
def test_tile_kernel_heads_and_products_vs_reference(rows):
    """run_with_heads in the rounded-bf16 mode (bf16 head rows: the next message MLP's products of this launch's own output) and the
    hoisted product launches ("hoist1", bf16 rows in feature order; "hoist1_rs", bf16 rows in the row-split order) against
    bf16_rne(bf16(W) . bf16(v))."""
    g = torch.Generator().manual_seed(rows)
    agg, v = torch.randn(rows, H, generator=g).to(DEV), torch.randn(rows, H, generator=g).to(DEV)
    node, nxt = make_mlp(2 * H, 2, True, rows), make_mlp(3 * H, 2, True, rows + 1)
    wn, W1 = sd(node), sd(nxt)["MLP.linear_1.weight"]
    with bf16_mode():
        y, heads = node.run_with_heads([ops.Source(agg), ops.Source(v)], rows, SELU, nxt, H, [H, H])
        assert last_kernel() == TILE and all(h.dtype == torch.bfloat16 for h in heads)
        y_ref = R.mlp(wn, [R.Block(agg), R.Block(v)], rows, act="selu")
        check(y, y_ref, "rows32", "heads launch rows")
        for j, h in enumerate(heads):
            check(h, R.products(W1[:, H * (j + 1):H * (j + 2)], y_ref), "prod16", f"head {j}")
        for tag, kw in (("hoist1", {}), ("hoist1_rs", dict(rs_rows=True))):
            pk1 = nxt._packed_cols(H, 2 * H, [H], [False], True, **kw)
            out = torch.empty(rows, H, dtype=torch.bfloat16, device=DEV)
            ops.mlp_forward(pk1, [ops.Source(v)], rows, out=out)
            assert last_kernel() == TILE
            got = ops.rs_rows_to_natural(out) if kw else out
            check(got, R.products(W1[:, H:2 * H], v), "prod16", tag)


# ------------------------------------------------------------------ mlp_ws_kernel<SP = 1>
@pytest.mark.parametrize("layers", [2, 3])
@pytest.mark.parametrize("deg", [4, 5, 6, 7, 8])
def test_ws_kernel_vs_reference(deg, layers):
    """Dense pairs of uniform segments (G4C_AGG_UNIFORM) at in-degree 4 .. 8, row counts that are not multiples of 64, the aggregation
    fused, with fp32, bf16 and bf16(SELU) rows."""
    m = make_mlp(3 * H, layers, True, 100 * deg + layers)
    w = sd(m)
    W1 = w["MLP.linear_1.weight"]
    for n in (11, 2999):
        E, ep, csr = uniform_edges(n, deg, n + deg)
        assert E % 64
        g = torch.Generator().manual_seed(E)
        e, v = torch.randn(E, H, generator=g).to(DEV), torch.randn(n, H, generator=g).to(DEV)
        pr, pc = (R.products(W1[:, a:a + H], v) for a in (H, 2 * H))
        src = [ops.Source(e, pre_act=SELU), ops.Source(pr.to(DEV, torch.bfloat16), index=ep.row, additive=True),
               ops.Source(pc.to(DEV, torch.bfloat16), index=ep.col, additive=True)]
        ref = R.mlp(w, [R.Block(e, pre_act="selu")], E, additive=[R.Additive(pr, ep.row), R.Additive(pc, ep.col)], first_cols=(0, H))
        agg_ref = R.segment_mean(ref, csr.off)
        with bf16_mode(ws=2):
            pk = m._packed_cols(0, H, [H], [False], False)
            for fmt, kw in (("fp32", {}), ("bf16", dict(rows_dtype=torch.bfloat16)),
                            ("bf16_selu", dict(rows_dtype=torch.bfloat16, rows_act=SELU))):
                a = torch.full((n, H), float("nan"), device=DEV)
                y = ops.mlp_forward(pk, src, E, agg=(csr, a, True), **kw)
                assert last_kernel() == WS
                what = f"ws K{deg} n{n} {fmt} rows"
                check(y, R.stored_rows(ref, fmt), "rows32" if fmt == "fp32" else "rows16", what)
                check(a, agg_ref, "agg32", what + " aggregate")


# ------------------------------------------------------------------ mlp_rs1_kernel
def _rs1_case(n, K, layers):
    blk = B.GNBlock((3 * H, (H,) * layers, True), (2 * H, (H,) * layers, True)).to(DEV)
    m = blk.edge_mlp
    with torch.no_grad():
        m.MLP.layer_norm.weight.copy_(1.0 + 0.1 * torch.randn(H, device=DEV))
        m.MLP.layer_norm.bias.copy_(0.1 * torch.randn(H, device=DEV))
    E, ep, csr = uniform_edges(n, K, 7 * n + K)
    g = torch.Generator().manual_seed(n * K)
    a32, s, r = torch.randn(E, H, generator=g).to(DEV), torch.randn(n, H, generator=g).to(DEV), torch.randn(n, H, generator=g).to(DEV)
    w = sd(m)
    W1 = w["MLP.linear_1.weight"]
    adds = [R.Additive(R.products(W1[:, H:2 * H], s), ep.row), R.Additive(R.products(W1[:, 2 * H:], r), ep.col)]
    ref = lambda x, ar=R.FP64, **kw: R.mlp(w, [x], E, additive=adds, first_cols=(0, H), ar=ar, **kw)
    launch = lambda x, agg, **kw: m.run_hoisted([x], [(s, ep.row), (r, ep.col)], E, agg=(csr, agg, True), **kw)
    return m, E, csr, a32, ref, launch


@pytest.mark.parametrize("layers", [2, 3])
@pytest.mark.parametrize("n,K", [(7, 5), (3, 8), (4001, 5), (2503, 8), (5001, 4), (2859, 7), (3337, 6)])
def test_rs1_kernel_vs_reference(n, K, layers, monkeypatch):
    """The row-split message kernel: fp32 rows, compact bf16(SELU) rows, tagged compact rows as the next launch's input, no rows, the bf16
    aggregate in the row-split order — at in-degree 4 .. 8, row counts just above RS1_MIN_ROWS and far below it (the threshold lowered),
    none a multiple of 16 rows per wave where the shape allows."""
    if n * K < B.RS1_MIN_ROWS:
        monkeypatch.setattr(B, "RS1_MIN_ROWS", 1)
    torch.manual_seed(n + layers)
    with bf16_mode():
        assert B.ROW_SPLIT_BF16
        m, E, csr, a32, ref, launch = _rs1_case(n, K, layers)
        x = R.Block(a32, pre_act="selu")
        y_ref = ref(x)
        agg_ref = R.segment_mean(y_ref, csr.off)
        a = torch.full((n, H), float("nan"), device=DEV)
        y = launch(ops.Source(a32, pre_act=SELU), a)
        assert last_kernel() == RS1 and y.dtype == torch.float32
        check(y, y_ref, "rows32", f"rs1 n{n} K{K} L{layers} fp32 rows")
        check(a, agg_ref, "agg32", f"rs1 n{n} K{K} L{layers} aggregate")
        a = torch.full((n, H), float("nan"), device=DEV)
        y16 = launch(ops.Source(a32, pre_act=SELU), a, rows_dtype=torch.bfloat16, rows_act=SELU)
        assert last_kernel() == RS1 and isinstance(y16, ops.RsOrderedRows)
        check(y16, R.stored_rows(y_ref, "bf16_selu"), "rows16", f"rs1 n{n} K{K} L{layers} compact rows")
        check(a, agg_ref, "agg32", f"rs1 n{n} K{K} L{layers} compact rows' aggregate")
        # chained: the compact rows as the next launch's input (already activated: read as they are)
        x16 = ops.rs_rows_to_natural(y16)
        y_ref2 = ref(R.Block(x16))
        a = torch.full((n, H), float("nan"), device=DEV)
        y2 = launch(ops.Source(y16), a, rows_dtype=torch.bfloat16, rows_act=SELU)
        assert last_kernel() == RS1
        check(y2, R.stored_rows(y_ref2, "bf16_selu"), "rows16", f"rs1 n{n} K{K} L{layers} chained")
        check(a, R.segment_mean(y_ref2, csr.off), "agg32", f"rs1 n{n} K{K} L{layers} chained aggregate")
        # no rows, fp32 and bf16 aggregate (the latter in the row-split order)
        a = torch.full((n, H), float("nan"), device=DEV)
        assert launch(ops.Source(a32, pre_act=SELU), a, store_rows=False) is None and last_kernel() == RS1
        check(a, agg_ref, "agg32", f"rs1 n{n} K{K} L{layers} no rows")
        a16 = torch.empty((n, H), dtype=torch.bfloat16, device=DEV)
        assert launch(ops.Source(a32, pre_act=SELU), a16, store_rows=False) is None and last_kernel() == RS1
        check(ops.rs_rows_to_natural(a16), R.segment_mean(y_ref, csr.off, bf16_out=True), "agg16", f"rs1 n{n} K{K} L{layers} bf16 aggregate")


# ------------------------------------------------------------------ mlp_rs2_kernel
@pytest.mark.parametrize("n", [33, 4097, 20001])
def test_rs2_kernel_vs_reference(n, monkeypatch):
    """The row-split update kernel: [bf16 aggregate (row-split order) | bf16 e] -> 256 -> 128 -> 128 -> LayerNorm -> SELU, e in the row-split
    order (format 4) or in feature order (5), with and without the next layer's two bf16 product heads, fp32 and bf16 output rows."""
    if n < B.RS1_MIN_ROWS:
        monkeypatch.setattr(B, "RS1_MIN_ROWS", 1)
    node, nxt = make_mlp(2 * H, 2, True, n), make_mlp(3 * H, 2, True, n + 1)
    wn, W1 = sd(node), sd(nxt)["MLP.linear_1.weight"]
    g = torch.Generator().manual_seed(n)
    agg = torch.randn(n, H, generator=g).to(DEV).to(torch.bfloat16)
    e = torch.nn.functional.selu(torch.randn(n, H, generator=g)).to(DEV).to(torch.bfloat16)
    y_ref = R.mlp(wn, [R.Block(agg), R.Block(e)], n, act="selu")
    h_ref = [R.products(W1[:, H * (j + 1):H * (j + 2)], y_ref) for j in range(2)]
    with bf16_mode():
        assert B.UPDATE_ROW_SPLIT
        for e_tagged in (True, False):
            for heads in (True, False):
                for out16 in (True, False):
                    src = [ops.Source(to_rs(agg)), ops.Source(to_rs(e) if e_tagged else e)]
                    out = torch.empty(n, H, device=DEV, dtype=torch.bfloat16 if out16 else torch.float32)
                    if heads:
                        y, hs = node.run_with_heads(src, n, SELU, nxt, H, [H, H], out=out, rs_rows=True)
                    else:
                        y, hs = node.run_coded(src, n, SELU, out=out), []
                    assert last_kernel() == RS2
                    what = f"rs2 n{n} format {4 if e_tagged else 5} heads {heads} {'bf16' if out16 else 'fp32'} rows"
                    check(y, R.stored_rows(y_ref, "bf16" if out16 else "fp32"), "rows16" if out16 else "rows32", what)
                    for j, h in enumerate(hs):
                        assert isinstance(h, ops.RsOrderedRows)
                        check(h, h_ref[j], "prod16", what + f" head {j}")


# ------------------------------------------------------------------ negative controls
@pytest.mark.parametrize("perturbation", ["round_toward_zero", "swap_adjacent_columns", "row_in_next_segment"])
def test_checker_rejects_the_kernel_against_a_perturbed_reference(perturbation):
    """The checker can fail: against a reference with weights rounded toward zero, with two adjacent input columns of one 32-feature step
    exchanged, or with one row counted in the next segment, the row-split kernel's (correct) output is rejected — while it passes the
    unperturbed reference.  Only the reference is touched."""
    n, K = 4001, 5
    torch.manual_seed(99)
    with bf16_mode():
        m, E, csr, a32, ref, launch = _rs1_case(n, K, 2)
        a = torch.full((n, H), float("nan"), device=DEV)
        y = launch(ops.Source(a32, pre_act=SELU), a)
        assert last_kernel() == RS1
    x = R.Block(a32, pre_act="selu")
    y_ref = ref(x)
    check(y, y_ref, "rows32", "control")
    check(a, R.segment_mean(y_ref, csr.off), "agg32", "control")
    if perturbation == "round_toward_zero":
        ok, s, lim = R.check_bf16_order_noise(y.float(), ref(x, R.Arith(weight_round="rtz")), "rows32")
    elif perturbation == "swap_adjacent_columns":
        ok, s, lim = R.check_bf16_order_noise(y.float(), ref(x, perturb=R.swap_adjacent_columns), "rows32")
    else:
        ok, s, lim = R.check_bf16_order_noise(a, R.segment_mean(y_ref, R.move_row_to_next_segment(csr.off, n // 2)), "agg32")
    print(f"[bf16-noise] negative control {perturbation}: {s} (limits {lim})")
    assert not ok, (perturbation, s, lim)


# ------------------------------------------------------------------ the tag and the C-ABI
def test_rows_put_back_in_feature_order_by_hand_are_read_as_such():
    """ops.RsOrderedRows: a tagged tensor whose columns the caller restored by hand (index_select along dim 1) is a plain Tensor now,
    so mlp_forward reads it as feature order — the same result as rs_rows_to_natural(t); before, the reader restored it a second time."""
    rows = 700
    m = make_mlp(3 * H, 2, True, 5)
    g = torch.Generator().manual_seed(5)
    x16 = torch.randn(rows, H, generator=g).to(DEV).to(torch.bfloat16)
    v = torch.randn(rows, H, generator=g).to(DEV)
    t = to_rs(x16)
    by_hand = t.index_select(1, torch.argsort(ops._rs_k_order(DEV)))
    assert type(by_hand) is torch.Tensor and torch.equal(by_hand, x16)
    with bf16_mode():
        outs = [m.run_coded([ops.Source(x), ops.Source(v), ops.Source(v)], rows) for x in (by_hand, ops.rs_rows_to_natural(t))]
    assert torch.equal(outs[0], outs[1])


def test_mlp_run_refuses_a_uniform_row_count_it_cannot_split():
    """G4C_AGG_UNIFORM(k) through the C-ABI (ctypes): a launch whose row count is not a multiple of k is refused with G4C_EINVAL before
    anything runs (the `row_count % k` check of g4c_mlp_run's output stage, csrc/mlp_run.hip); the same launch with whole segments runs on mlp_ws_kernel's dense mode.
    (The launcher's refusal of a sub-range in dense mode is a guard only: g4c_mlp_run refuses a row sub-range of any launch with an
    aggregation before that.)"""
    import ctypes as C
    n, K = 301, 5
    m = make_mlp(3 * H, 2, True, 3)
    E, ep, csr = uniform_edges(n, K, 3)
    g = torch.Generator().manual_seed(3)
    e, p = torch.randn(E, H, generator=g).to(DEV), torch.randn(n, H, generator=g).to(DEV)
    src = [ops.Source(e, pre_act=SELU), ops.Source(p, index=ep.row, additive=True), ops.Source(p, index=ep.col, additive=True)]
    with bf16_mode(ws=2) as lib:
        pk = m._packed_cols(0, H, [H], [False], False)
        arr = ops._src_array(src)
        out, agg = torch.empty(E, H, device=DEV), torch.full((n, H), float("nan"), device=DEV)
        t_rows, t_seg, nt = csr.tiles()

        def call(rows):
            io = _lib.g4c_mlp_io_t(row_count=rows, out=_lib.ptr(out), out_ld=H, tile_rows=_lib.ptr(t_rows), tile_seg=_lib.ptr(t_seg),
                                   seg_off=_lib.ptr(csr.off), n_tiles=nt, agg=_lib.ptr(agg), agg_ld=H, agg_mode=1 | (K << 8))
            return lib.g4c_mlp_run(C.byref(pk.desc), arr, len(src), rows, C.byref(io), _lib.stream_handle(DEV))
        assert call(E - 1) == _lib.EINVAL and last_kernel() == 0
        assert torch.isnan(agg).all()
        assert call(E) == _lib.OK and last_kernel() == WS
        torch.cuda.synchronize()
        assert torch.equal(agg, ops.segment_reduce(out, csr, True))
