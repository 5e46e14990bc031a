"""Where every family of g4c_mlp_run writes (tests/footprint.py): one launch per case under its switches (arithmetic,
g4c_mlp_ws_enable, g4c_mlp_bx6i_enable, g4c_mlp_small_launch_tiles, g4c_mlp_shapes_enable; all restored), the asserted kernel code and
tile shape, and then

- every tensor the launch writes — output rows, heads, the fused aggregate, v', every save[l], the bf16 forms of the rounded-bf16 mode —
  sits in a guard arena: 64 pattern rows above and below, pattern columns left and right (a leading dimension larger than the width).
  Outside what the launch owns the pattern must still be there, inside every element must be gone and finite.  With an output index
  the rows no index names are not owned, with a row sub-range the rows outside it, with store_rows=False there is no row tensor at all;
- every tensor the launch reads — source rows, gathered tables, `first`, v, the residual, `mul` rows, index vectors, the CSR offsets,
  permutation and tile tables, the packed weight stream and bias block, the LayerNorm parameters — is bit for bit what it was.

Values are tests/test_gpu_fwd_ref.py's and tests/test_gpu_bf16.py's business; the case builders are the former's.

Row counts.  A kernel whose row block is B runs n in {1, B - 1, B, B + 1, 2B - 1, 2B + 1} and one count of several blocks plus a remainder:
B = 32 for mlp_split_kernel and the tile kernel (ROWS = 32 in csrc/mlp_fused.hip), B = 64 — a pair of 32-row tiles per workgroup step — for
mlp_ws_kernel and mlp_bx6i_kernel, B = 16 — the chunk a wave owns — and 16 RS_WAVES = 128 — what one more workgroup is launched for
(rs_grid) — for the row-split kernels, read from csrc/mlp_rs.hip (`rs_blocks`).  The aggregating forms run on tiles of whole segments: ragged plans with
empty runs, a last tile that is a single one-row segment, a last segment of exactly 32 rows; the dense uniform mode (K = 4, 6, 8) with
segment counts one segment short of, at and past a pair.

Every test states the matrix lines it must hit — (kernel code, case label, arithmetic) — and `_matrix_lines` compares them with what
its launches asserted, as in tests/test_gpu_fwd_ref.py.  The negative control of the helpers is tests/test_footprint_host.py."""
import contextlib
import ctypes as C
import dataclasses
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

import footprint as FP                               # noqa: E402
import test_gpu_fwd_ref as F                         # noqa: E402  (its case builders: node_blocks, message_blocks, net, csr_of, ragged_degrees)
from graphs4cfd_amd import _lib, ops                 # noqa: E402

DEV = F.DEV
F32, BF16 = torch.float32, torch.bfloat16
H = 128
ACT = F.ACT
K_SPLIT, K_BX6, K_BX6I, K_WS, K_BX6_CERT, K_WS_CERT = F.K_SPLIT, F.K_BX6, F.K_BX6I, F.K_WS, F.K_BX6_CERT, F.K_WS_CERT
K_RS1, K_RS2, K_WS_PRE = _lib.KERNEL_MLP_RS, _lib.KERNEL_MLP_RS2, _lib.KERNEL_MLP_WS_PRE
GENERIC, NODE = _lib.TILE_SHAPE_GENERIC, _lib.TILE_SHAPE_NODE
RING, DEEP = F.RING, F.DEEP
FORMS, PRECS = F.FORMS, F.PRECS


def counts(B, several):
    return (1, B - 1, B, B + 1, 2 * B - 1, 2 * B + 1, several)


N32 = counts(32, 5 * 32 + 7)           # split and tile kernels
N64 = counts(64, 4 * 64 + 9)           # mlp_ws_kernel, mlp_bx6i_kernel: pairs of tiles


def rs_blocks():
    """(rows of a wave's chunk, rows one more workgroup is launched for) of the row-split kernels, from their source."""
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "graphs4cfd_amd", "csrc", "mlp_rs.hip")).read()
    waves = int(re.search(r"constexpr int RS_WAVES = (\d+);", src).group(1))
    assert "chunks = (p.M + 15) / 16, want = (chunks + RS_WAVES - 1) / RS_WAVES" in src          # (rs_grid: 16-row chunks, RS_WAVES per workgroup)
    return 16, 16 * waves


RS_B, RS_WG = rs_blocks()
N_RS = (1, RS_B - 1, RS_B, RS_B + 1, 2 * RS_B - 1, 2 * RS_B + 1, RS_WG - 1, RS_WG, RS_WG + 1, 3 * RS_WG + RS_B + 5)

HIT = set()
LINES = {}


def lines(fn):
    def deco(test):
        LINES[test.__name__] = fn
        return test
    return deco


@pytest.fixture(autouse=True)
def _matrix_lines(request):
    """Every test hits exactly the matrix lines it states."""
    before = set(HIT)
    HIT.clear()
    yield
    got = set(HIT)
    HIT.clear(); HIT.update(before | got)
    want = LINES[request.node.originalname](**getattr(getattr(request.node, "callspec", None), "params", {}))
    assert got == want, f"matrix lines missing {sorted(want - got)}, unexpected {sorted(got - want)}"


@pytest.fixture(autouse=True)
def _inference():
    with torch.no_grad():
        yield


@contextlib.contextmanager
def switches(prec, ws=0, bx6i=0, small=None, shapes=1):
    with F.switches(prec, ws, bx6i, small) as lib:
        old = lib.g4c_mlp_shapes_enable(shapes)
        try:
            yield lib
        finally:
            lib.g4c_mlp_shapes_enable(old)


class Outs:
    """The arenas of one launch."""

    def __init__(self):
        self.items = []

    def add(self, name, rows, cols=H, dtype=F32, written=None, **kw):
        view, whole = FP.arena(rows, cols, dtype, device=DEV, **kw)
        assert kw or view.data_ptr() % 16 == 0          # (the default window is on every kernel's vector path)
        self.items.append((name, view, whole, written))
        return view

    def check(self, what):
        torch.cuda.synchronize()
        for name, view, whole, written in self.items:
            FP.assert_footprint(whole, view, written_rows=written, what=f"{what}: {name}")
            if isinstance(written, range):
                written = torch.arange(written.start, written.stop)
            got = view if written is None else view[torch.as_tensor(written).to(DEV)]
            assert bool(torch.isfinite(got.float()).all()), f"{what}: {name} holds a non-finite value in a row the launch owns"


def plan_tensors(csr):
    if csr is None:
        return []
    t = csr.tiles()
    return [csr.off, csr.perm] + ([t[0], t[1]] if t is not None else [])


def inputs_of(sources, packs, *more):
    ts = []
    for s in sources:
        ts += [s.tensor, s.index] + plan_tensors(s.segments)
    for pk in packs:
        ts += list(pk._keep)
    return ts + [t for t in more if t is not None]


def ran(lib, what, expect, shape=GENERIC):
    k, s = int(lib.g4c_mlp_last_kernel()), int(lib.g4c_mlp_last_shape())
    assert k == expect, f"{what}: kernel {_lib.KERNEL_NAMES.get(k)} ({k}) ran, expected code {expect}"
    assert s == shape, f"{what}: tile shape {s}, expected {shape}"


def launch(what, prec, nt, blks, n_rows, expect, *, act=None, heads=False, agg=None, store_rows=True, out_idx=None, out_rows=None,
           resid=None, resid_col0=0, rows=None, certify=False, ws=0, bx6i=0, small=None, shape=GENERIC, shapes=1, out_dtype=F32,
           head_dtype=F32, agg_dtype=F32, window=None):
    """One ops.mlp_forward launch: every output in an arena, every input frozen, kernel and shape asserted.  `agg` = (csr, mean);
    `rows` = (begin, count); `window`: col0 / pad_cols of the output arena (default: the aligned window)."""
    n_out = int(nt.W[-1].size(0))
    outs = Outs()
    with switches(prec, ws, bx6i, small, shapes) as lib:
        pk = nt.pack(blks, prec, heads)
        srcs = [b.source(certify) for b in blks]
        oi32 = None if out_idx is None else out_idx.to(torch.int32)
        written = None
        if out_idx is not None:
            written = out_idx
        elif rows is not None:
            written = range(rows[0], rows[0] + rows[1])
        out = outs.add("out", out_rows or n_rows, n_out, out_dtype, written, **(window or {})) if store_rows else None
        head_outs = [outs.add(f"head{j}", n_rows, H, head_dtype) for j in range(len(nt.heads))] if heads else None
        agg_out = outs.add("agg", agg[0].n_seg, H, agg_dtype) if agg else None
        frozen = inputs_of(srcs, [pk], resid, oi32, *plan_tensors(agg[0] if agg else None))
        with FP.frozen(*frozen, what=what), ops.RangeFlags(DEV):
            y = ops.mlp_forward(pk, srcs, n_rows, ACT[act], out=out, out_idx32=oi32, resid=resid, resid_col0=resid_col0, rows=rows,
                                head_outs=head_outs, agg=None if agg is None else (agg[0], agg_out, agg[1]), store_rows=store_rows)
            ran(lib, what, expect, shape)
            assert (y is None) == (not store_rows) and (y is None or y.data_ptr() == out.data_ptr())
            outs.check(what)
    HIT.add((expect, what.split(" ")[0], prec))


def raw_launch(what, prec, pk, srcs, n_rows, expect, csr, mean, *, out_dtype=None, io_out_dtype=0, agg_dtype=F32, ws=0):
    """g4c_mlp_run through ctypes, for the row formats ops.mlp_forward only produces into tensors of its own (bf16(SELU(row)) rows:
    G4C_DTYPE_BF16_SELU)."""
    outs = Outs()
    with switches(prec, ws) as lib:
        out = outs.add("out", n_rows, H, out_dtype) if out_dtype is not None else None
        agg_out = outs.add("agg", csr.n_seg, H, agg_dtype)
        arr = ops._src_array(srcs)
        io = _lib.g4c_mlp_io_t(row_count=n_rows, out=_lib.ptr(out), out_ld=H if out is None else int(out.stride(0)), out_dtype=io_out_dtype)
        ops._set_agg(io, csr, agg_out, mean)
        if agg_dtype == BF16:
            io.agg_mode |= 1 << 16
        with FP.frozen(*inputs_of(srcs, [pk], *plan_tensors(csr)), what=what):
            rc = lib.g4c_mlp_run(C.byref(pk.desc), arr, len(srcs), n_rows, C.byref(io), _lib.stream_handle(DEV))
            assert rc == _lib.OK, f"{what}: {lib.g4c_last_error().decode()}"
            ran(lib, what, expect)
            outs.check(what)
    HIT.add((expect, what.split(" ")[0], prec))


# ---- tile plans of whole segments ---------------------------------------------------------------------------------------------------
def seg_cases():
    """(name, degrees): ragged plans whose LAST tile is what the name says; the property is asserted on the plan (tile_plan)."""
    r = F.ragged_degrees(47, 300)
    return [("one-segment", torch.tensor([1])), ("tiny", torch.tensor([5, 0, 3])), ("ragged", r),
            ("last-tile-one-row", torch.cat([r, torch.tensor([32, 1])])), ("last-segment-32", torch.cat([r, torch.tensor([7, 32])])),
            ("ragged-long", F.ragged_degrees(160, 301, 12))]


def tile_plan(name, deg):
    csr = F.csr_of(deg)
    t_rows, _, nt = csr.tiles()
    t_rows = t_rows.cpu()
    assert int(t_rows[nt]) == csr.n
    if name == "last-tile-one-row":
        assert int(t_rows[nt] - t_rows[nt - 1]) == 1
    if name == "last-segment-32":
        assert int(t_rows[nt] - t_rows[nt - 1]) == 32 and int(csr.off[-1] - csr.off[-2]) == 32
    if name.startswith("ragged"):
        assert int((deg == 0).sum()) >= 10 and int(deg[0]) == 0
    return csr


def permuted_plan(deg, seed):
    """F.csr_of's plan over rows that arrive in random order — with the permutation spelled out where the shuffle of a few rows left
    them in segment order (one segment, say): the launch must take the seg_perm path either way."""
    keys = torch.arange(int(deg.numel())).repeat_interleave(deg)
    keys = keys[torch.randperm(int(keys.numel()), generator=F._gen(seed))]
    c = F.plan.build_csr(keys, int(deg.numel()), DEV)
    if c.perm is None:
        c = dataclasses.replace(c, perm=torch.arange(c.n, dtype=torch.int32, device=DEV), _tiles=False)
    return c


def dense_cases():
    """Uniform segments of K rows: n_seg K one segment short of, at (where K divides a pair of 64 rows; else at the first common multiple)
    and past a pair, one lone segment, and several pairs with a remainder."""
    out = []
    for K in (4, 6, 8):
        at = 64 // K if 64 % K == 0 else 192 // K
        for n_seg in sorted({1, 64 // K - (64 % K == 0), 64 // K + (64 % K != 0), at, at + 1, 5 * 64 // K + 3}):
            out.append((K, n_seg))
    return out


# ====================================================================== MLP_SPLIT (fp32)
@lines(lambda path: {(K_SPLIT, f"split:{path}:{x}", "fp32") for x in ("n_out=3", "n_out=37", "n_out=128", "heads")})
@pytest.mark.parametrize("path", ["vec", "unaligned"])
def test_split_kernel(path):
    for n in N32:
        blks = F.node_blocks(n, "C", 10 + n, path)
        k_in = sum(b.w() for b in blks)
        for n_out in (3, 37, 128):          # out_ld = n_out + 16: an odd leading dimension for 3 and 37
            launch(f"split:{path}:n_out={n_out} n={n}", "fp32", F.net(k_in, (H, H, n_out), 11), blks, n, K_SPLIT, act="selu")
        launch(f"split:{path}:heads n={n}", "fp32", F.net(k_in, (H, H, H), 12, n_heads=2), blks, n, K_SPLIT, act="selu", heads=True)


# ====================================================================== MLP_BX6: the tile kernel, ring and deep ring
@lines(lambda prec, form: {(K_BX6, f"bx6:{form[0]}:{x}", prec) for x in ("full", "vec", "unaligned", "heads", "out_idx", "resid", "n_out=3",
                                                                           "n_out=64", "rows")})
@pytest.mark.parametrize("form", FORMS, ids=lambda f: f[0])
@pytest.mark.parametrize("prec", PRECS)
def test_tile_kernel_rows(prec, form):
    """The three source paths, heads, an output index, a residual, n_out < 128 into a column window, a row sub-range."""
    tag, kw = f"bx6:{form[0]}", dict(small=form[1])
    for n in N32:
        for path in ("full", "vec", "unaligned"):
            blks = F.node_blocks(n, "C", 20 + n, path)
            launch(f"{tag}:{path} n={n}", prec, F.net(sum(b.w() for b in blks), (H, H, H), 21), blks, n, K_BX6, **kw)
        blks = F.node_blocks(n, "C", 22 + n, "full")
        nt = F.net(2 * H, (H, H, H), 23, n_heads=2)
        launch(f"{tag}:heads n={n}", prec, nt, blks, n, K_BX6, act="selu", heads=True, **kw)
        oi = torch.randperm(2 * n + 3, generator=F._gen(24 + n))[:n].to(DEV)
        launch(f"{tag}:out_idx n={n}", prec, nt, blks, n, K_BX6, act="tanh", out_idx=oi, out_rows=2 * n + 3, **kw)
        launch(f"{tag}:resid n={n}", prec, nt, blks, n, K_BX6, act="selu", resid=F.table(n, 140, 25 + n), resid_col0=4, **kw)
        for n_out, window in ((3, dict(col0=5, pad_cols=3)), (64, dict(col0=8, pad_cols=8))):
            launch(f"{tag}:n_out={n_out} n={n}", prec, F.net(2 * H, (H, n_out), 26, ln=(n_out == 64)), blks, n, K_BX6, act="tanh",
                   window=window, **kw)
    # a row sub-range: only [begin, begin + count) is written (begin a multiple of 32; a range that ends inside a tile, at a tile, at the end)
    n = 167
    blks = F.node_blocks(n, "C", 27, "full")
    nt = F.net(2 * H, (H, H, H), 28)
    for begin, count in ((0, 33), (32, 45), (64, 64), (96, 71), (160, 7), (32, 1)):
        launch(f"{tag}:rows [{begin}, +{count})", prec, nt, blks, n, K_BX6, rows=(begin, count), **kw)


@lines(lambda prec, form: {(K_BX6, f"bx6:{form[0]}:{x}", prec) for x in ("agg:stored", "agg:not-stored", "agg_on_load:ordered",
                                                                           "agg_on_load:seg_perm", "narrow-only", "narrow+wide")})
@pytest.mark.parametrize("form", FORMS, ids=lambda f: f[0])
@pytest.mark.parametrize("prec", PRECS)
def test_tile_kernel_aggregation_and_narrow_blocks(prec, form):
    tag, kw = f"bx6:{form[0]}", dict(small=form[1])
    nt = F.net(H, (H, H, H), 30)
    for i, (name, deg) in enumerate(seg_cases() + [(f"k={k}", torch.full((m,), k)) for k, m in ((6, 11), (5, 13), (32, 3))]):
        csr = tile_plan(name, deg)
        blks, _ = F.message_blocks(csr.n, csr.n_seg, "C", 31 + i)
        for store in (True, False):
            launch(f"{tag}:agg:{'stored' if store else 'not-stored'} {name}", prec, nt, blks, csr.n, K_BX6, agg=(csr, bool(i % 2)),
                   store_rows=store, **kw)
    # aggregation on load: the node launch reads each target's rows through the plan (n = targets: the tile counts of N32)
    nn = F.net(2 * H, (H, H, H), 40)
    for i, n in enumerate(N32):
        deg = F.ragged_degrees(n, 41 + n, 6) if n >= 40 else torch.randint(0, 5, (n,), generator=F._gen(41 + n))
        deg[-1] = 3
        for order, shuffle in (("ordered", None), ("seg_perm", 42 + n)):
            csr = F.csr_of(deg) if shuffle is None else permuted_plan(deg, shuffle)
            blks = [F.Blk(F.rows_of(csr.n, H, "C", 43 + n), csr=csr, mean=bool(i % 2), pre_act="selu" if i % 2 else None), F.Blk(F.table(n, H, 44 + n))]
            launch(f"{tag}:agg_on_load:{order} n={n}", prec, nn, blks, n, K_BX6, act="selu", **kw)
    for n in N32:
        buf = F.rows_of(n, 24, "C", 50 + n)
        nb = [F.Blk(buf, col0=1, width=2, narrow=True), F.Blk(buf, col0=4, width=3, narrow=True), F.Blk(buf, col0=8, width=5, narrow=True)]
        launch(f"{tag}:narrow-only n={n}", prec, F.net(10, (H, H, H), 51, False), nb, n, K_BX6, act="selu", **kw)
        mb = [F.Blk(buf, col0=16, width=8, narrow=True, negate=True), F.Blk(F.rows_of(n, H, "C", 52 + n)), F.Blk(buf, col0=2, width=2, narrow=True)]
        launch(f"{tag}:narrow+wide n={n}", prec, F.net(8 + H + 2, (H, H, H), 53), mb, n, K_BX6, act="tanh", **kw)


@lines(lambda form: {(K_BX6_CERT, f"bx6_cert:{form[0]}", "f16x3")} | ({(K_BX6, f"bx6:ring:shape:{s}", "f16x3") for s in ("NODE", "GENERIC")}
                                                                     | {(K_BX6_CERT, "bx6_cert:ring:shape:NODE", "f16x3")} if form[0] == "ring" else set()))
@pytest.mark.parametrize("form", FORMS, ids=lambda f: f[0])
def test_tile_kernel_certified_and_compile_time_shapes(form):
    """The tracker-free instantiation (sources with a true bound), and — the two-step ring only — the node-update launch on its
    compile-time shape and, the shapes switched off, on the all-runtime kernel; heads on both."""
    for n in N32:
        blks = F.node_blocks(n, "C", 60 + n, "full")
        nt = F.net(2 * H, (H, H, H), 61, True, "ln", n_heads=2)
        launch(f"bx6_cert:{form[0]} n={n}", "f16x3", nt, blks, n, K_BX6_CERT, act="selu", heads=True, certify=True, small=form[1])
        if form[0] != "ring":
            continue
        direct = [F.Blk(F.rows_of(n, H, "C", 62 + n)), F.Blk(F.table(n, 3 * H + 8, 63 + n), col0=H + 4, width=H)]
        for heads in (False, True):
            launch(f"bx6:ring:shape:NODE n={n} heads={heads}", "f16x3", nt, direct, n, K_BX6, act="selu", heads=heads, small=RING, shape=NODE)
            launch(f"bx6:ring:shape:GENERIC n={n} heads={heads}", "f16x3", nt, direct, n, K_BX6, act="selu", heads=heads, small=RING, shapes=0)
        launch(f"bx6_cert:ring:shape:NODE n={n}", "f16x3", nt, direct, n, K_BX6_CERT, act="selu", heads=True, certify=True, small=RING, shape=NODE)


@lines(lambda form: {(K_BX6, f"bx6:{form[0]}:bf16:{x}", "bf16") for x in ("fp32-rows", "bf16-rows", "bf16-heads", "bf16-rows+heads", "agg:bf16-rows")})
@pytest.mark.parametrize("form", FORMS, ids=lambda f: f[0])
def test_tile_kernel_rounded_bf16_outputs(form):
    """The rounded-bf16 mode on the tile kernel: fp32 and bf16 output rows, bf16 head rows (the next message MLP's products), bf16 rows
    under a fused fp32 aggregate."""
    tag, kw = f"bx6:{form[0]}:bf16", dict(small=form[1])
    nt = F.net(2 * H, (H, H), 170, n_heads=2)
    for n in N32:
        blks = F.node_blocks(n, "C", 171 + n, "full")
        launch(f"{tag}:fp32-rows n={n}", "bf16", nt, blks, n, K_BX6, act="selu", **kw)
        launch(f"{tag}:bf16-rows n={n}", "bf16", nt, blks, n, K_BX6, act="selu", out_dtype=BF16, **kw)
        launch(f"{tag}:bf16-heads n={n}", "bf16", nt, blks, n, K_BX6, act="selu", heads=True, head_dtype=BF16, **kw)
        launch(f"{tag}:bf16-rows+heads n={n}", "bf16", nt, blks, n, K_BX6, act="selu", heads=True, head_dtype=BF16, out_dtype=BF16, **kw)
    mt = F.net(H, (H, H, H), 172)
    for i, (name, deg) in enumerate(seg_cases()):
        csr = tile_plan(name, deg)
        blks, _ = F.message_blocks(csr.n, csr.n_seg, "C", 173 + i)
        launch(f"{tag}:agg:bf16-rows {name}", "bf16", mt, blks, csr.n, K_BX6, agg=(csr, bool(i % 2)), out_dtype=BF16, **kw)


# ====================================================================== the training forms: save / mul
SAVE_FORMS = (("f16x3", F32), ("bf16x6", F32), ("bf16", F32), ("bf16", BF16))


@lines(lambda form: {(K_BX6, f"{x}:{'bf16' if form[1] == BF16 else 'fp32'}-rows", form[0]) for x in ("save", "save:no-ln", "mul")})
@pytest.mark.parametrize("form", SAVE_FORMS, ids=lambda f: f"{f[0]}-{str(f[1]).replace('torch.', '')}")
def test_save_and_mul_forms(form):
    """The recording forward (every layer's rows kept: save[l] in an arena with save_ld = 144; without a LayerNorm the last entry is
    None) and the backward chain's form (save of every hidden layer, `mul` rows whose slope multiplies it: frozen)."""
    prec, dt = form
    tag = "bf16-rows" if dt == BF16 else "fp32-rows"
    for n in N32:
        for ln in (True, False):
            nt = F.net(2 * H, (H, H, H), 70 + ln, ln)
            blks = [F.Blk(F.rows_of(n, H, "C", 71 + n), pre_act="selu"), F.Blk(F.table(max(n // 5, 1), H, 72 + n), index=F.index(n, max(n // 5, 1), 73 + n))]
            what = f"{'save' if ln else 'save:no-ln'}:{tag} n={n}"
            outs = Outs()
            with switches(prec) as lib:
                pk, srcs = nt.pack(blks, prec), [b.source(False) for b in blks]
                out = outs.add("out", n)
                save = [outs.add(f"save[{l}]", n, H, dt) for l in range(2)] + [outs.add("save[2]", n, H, dt) if ln else None]
                with FP.frozen(*inputs_of(srcs, [pk]), what=what), ops.RangeFlags(DEV):
                    ops.mlp_forward(pk, srcs, n, ACT["tanh"], out=out, save=save)
                    ran(lib, what, K_BX6)
                    outs.check(what)
            HIT.add((K_BX6, what.split(" ")[0], prec))
        # the backward chain: g -> W3^T -> (x slope of a2) -> W2^T -> (x slope of a1) -> W_dense^T, no biases, no LayerNorm
        what = f"mul:{tag} n={n}"
        Ws = [F.table(H, H, 74 + l) / 11 for l in range(3)]
        acts = [torch.nn.functional.selu(F.table(n, H + 8, 77 + l)).to(dt) for l in range(2)]          # (mul_ld = 136)
        outs = Outs()
        with switches(prec) as lib:
            pk = ops.PackedMLP(Ws, [None] * 3, None, [H], [False], precision=prec, site="footprint")
            srcs = [ops.Source(F.table(n, H, 79 + n))]
            out = outs.add("out", n)
            save = [outs.add(f"save[{l}]", n) for l in range(2)] + [None]
            mul = [a[:, :H] for a in acts] + [None]
            with FP.frozen(*inputs_of(srcs, [pk], *acts), what=what), ops.RangeFlags(DEV):
                ops.mlp_forward(pk, srcs, n, ACT[None], out=out, save=save, mul=mul)
                ran(lib, what, K_BX6)
                outs.check(what)
        HIT.add((K_BX6, what.split(" ")[0], prec))


# ====================================================================== MLP_BX6I (bf16x6, every size: mode 2)
@lines(lambda: {(K_BX6I, f"bx6i:{x}", "bf16x6") for x in ("direct", "indexed", "direct:agg", "indexed:agg", "direct:agg-only", "indexed:agg-only",
                                                            "indexed+out_idx")})
def test_bx6i_kernel():
    nt = F.net(H, (H, H, H), 80)
    for n in N64:
        for src, indexed in (("direct", False), ("indexed", True)):
            blks, _ = F.message_blocks(n, max(n // 6, 1), "C", 81 + n, indexed=indexed, pre_act=None if indexed else "selu")
            launch(f"bx6i:{src} n={n}", "bf16x6", nt, blks, n, K_BX6I, bx6i=2)
        oi = torch.randperm(n + 50, generator=F._gen(82 + n))[:n].to(DEV)
        launch(f"bx6i:indexed+out_idx n={n}", "bf16x6", nt, blks, n, K_BX6I, act="selu", out_idx=oi, out_rows=n + 50, bx6i=2)
    for i, (name, deg) in enumerate(seg_cases() + [("k=6", torch.full((11,), 6)), ("k=32 x 3", torch.full((3,), 32)), ("k=32 x 4", torch.full((4,), 32))]):
        csr = tile_plan(name, deg)
        for src, indexed in (("direct", False), ("indexed", True)):
            blks, _ = F.message_blocks(csr.n, csr.n_seg, "C", 83 + i, indexed=indexed, pre_act=None if indexed else "selu")
            launch(f"bx6i:{src}:agg {name}", "bf16x6", nt, blks, csr.n, K_BX6I, agg=(csr, bool(i % 2)), bx6i=2)
            launch(f"bx6i:{src}:agg-only {name}", "bf16x6", nt, blks, csr.n, K_BX6I, agg=(csr, bool(i % 2)), store_rows=False, bx6i=2)


# ====================================================================== MLP_WS / MLP_WS_CERT (f16x3)
def ws_net(layers, cert, seed):
    return F.net(H, (H,) * layers, seed, True, "ln" if cert else "default")


@lines(lambda layers, cert: {(K_WS_CERT if cert else K_WS, f"ws:{x}:L{layers}", "f16x3") for x in ("plain", "indexed", "out_idx")})
@pytest.mark.parametrize("cert", [False, True], ids=["tracked", "certified"])
@pytest.mark.parametrize("layers", [2, 3])
def test_ws_plain_indexed_scattered(layers, cert):
    code, nt = K_WS_CERT if cert else K_WS, ws_net(layers, cert, 90)
    for n in N64:
        blks, _ = F.message_blocks(n, max(n // 6, 1), "C", 91 + n)
        launch(f"ws:plain:L{layers} n={n}", "f16x3", nt, blks, n, code, ws=2, certify=cert)
        ib, _ = F.message_blocks(n, max(n // 6, 1), "C", 92 + n, indexed=True, pre_act=None)
        launch(f"ws:indexed:L{layers} n={n}", "f16x3", nt, ib, n, code, ws=2, act="selu", certify=cert)
        oi = torch.randperm(n + 40, generator=F._gen(93 + n))[:n].to(DEV)
        launch(f"ws:out_idx:L{layers} n={n}", "f16x3", nt, blks, n, code, ws=2, out_idx=oi, out_rows=n + 40, certify=cert)


@lines(lambda layers, cert: {(K_WS_CERT if cert else K_WS, f"ws:{x}:{f}:L{layers}", "f16x3") for x in ("agg", "agg-only") for f in ("ragged", "dense")})
@pytest.mark.parametrize("cert", [False, True], ids=["tracked", "certified"])
@pytest.mark.parametrize("layers", [2, 3])
def test_ws_fused_aggregation(layers, cert):
    """Tiles of whole ragged segments, and the dense mode of uniform segments of 4, 6 and 8 rows, which cuts its rows at segment
    boundaries: rows stored and not stored.  The aggregate is owned in full, the zero rows of empty segments included."""
    code, nt = K_WS_CERT if cert else K_WS, ws_net(layers, cert, 100)
    plans = [("ragged", name, tile_plan(name, deg)) for name, deg in seg_cases()]
    plans += [("dense", f"k={K} n_seg={m}", F.csr_of(torch.full((m,), K))) for K, m in dense_cases()]
    for i, (form, name, csr) in enumerate(plans):
        assert (4 <= csr.uniform_deg <= 8) == (form == "dense"), name
        blks, _ = F.message_blocks(csr.n, csr.n_seg, "C", 101 + i)
        launch(f"ws:agg:{form}:L{layers} {name}", "f16x3", nt, blks, csr.n, code, ws=2, agg=(csr, bool(i % 2)), certify=cert)
        launch(f"ws:agg-only:{form}:L{layers} {name}", "f16x3", nt, blks, csr.n, code, ws=2, agg=(csr, bool(i % 2)), store_rows=False, certify=cert)


@lines(lambda layers: {(K_WS, f"ws:bf16:{x}:{f}:L{layers}", "bf16") for x in ("fp32-rows", "bf16-rows", "bf16-selu-rows", "no-rows") for f in ("ragged", "dense")})
@pytest.mark.parametrize("layers", [2, 3])
def test_ws_rounded_bf16_rows(layers):
    """The rounded-bf16 mode on mlp_ws_kernel: fp32 rows, bf16 rows (`rows_dtype`), bf16(SELU(row)) rows (`rows_act`), no rows; the
    aggregate stays fp32.  bf16 product tables, as the mode's models launch it."""
    nt = ws_net(layers, False, 110)
    plans = [("ragged", name, tile_plan(name, deg)) for name, deg in seg_cases()[2:5]]
    plans += [("dense", f"k={K} n_seg={m}", F.csr_of(torch.full((m,), K))) for K, m in dense_cases()]
    for i, (form, name, csr) in enumerate(plans):
        blks, _ = F.message_blocks(csr.n, csr.n_seg, "C", 111 + i)
        for b in blks[1:]:
            b.x = b.x.to(BF16)
        tag = f":{form}:L{layers} {name}"
        launch(f"ws:bf16:fp32-rows{tag}", "bf16", nt, blks, csr.n, K_WS, ws=2, agg=(csr, True))
        launch(f"ws:bf16:bf16-rows{tag}", "bf16", nt, blks, csr.n, K_WS, ws=2, agg=(csr, False), out_dtype=BF16)
        launch(f"ws:bf16:no-rows{tag}", "bf16", nt, blks, csr.n, K_WS, ws=2, agg=(csr, True), store_rows=False)
        with switches("bf16", 2):
            pk, srcs = nt.pack(blks, "bf16"), [b.source(False) for b in blks]
        raw_launch(f"ws:bf16:bf16-selu-rows{tag}", "bf16", pk, srcs, csr.n, K_WS, csr, True, out_dtype=BF16, io_out_dtype=2, ws=2)


# ====================================================================== the fused MP layer and the precomputed first layer
@lines(lambda layers, cert: {(K_WS_CERT if cert else K_WS, f"mp_layer:L{layers}:{x}", "f16x3") for x in ("stored", "not-stored", "stored:heads", "not-stored:heads")})
@pytest.mark.parametrize("cert", [False, True], ids=["tracked", "certified"])
@pytest.mark.parametrize("layers", [2, 3])
def test_ws_fused_mp_layer(layers, cert):
    """ops.mp_layer_forward: e' (stored / not stored), the aggregate the launch writes and re-reads, v' and both heads — the node-side
    tensors own n_seg rows."""
    code = K_WS_CERT if cert else K_WS
    msg = F.net(H, (H,) * layers, 120, True, "ln" if cert else "default")
    upd = F.net(2 * H, (H,) * layers, 121, True, "ln" if cert else "default", n_heads=2)
    plans = [(name, tile_plan(name, deg)) for name, deg in seg_cases()] + [(f"k={K} n_seg={m}", F.csr_of(torch.full((m,), K))) for K, m in dense_cases()[::2]]
    for i, (name, csr) in enumerate(plans):
        n, E = csr.n_seg, csr.n
        blks, _ = F.message_blocks(E, n, "C", 122 + i)
        v = F.table(n, H, 123 + i)
        for store in (True, False):
            for heads in (False, True):
                what = f"mp_layer:L{layers}:{'stored' if store else 'not-stored'}{':heads' if heads else ''} {name}"
                outs = Outs()
                with switches("f16x3", 2) as lib:
                    pm, pu = msg.pack(blks, "f16x3"), upd.pack([F.Blk(v), F.Blk(v)], "f16x3", heads=True)
                    srcs = [b.source(cert) for b in blks]
                    e_out = outs.add("e'", E) if store else None
                    agg_out, v_out = outs.add("agg", n), outs.add("v'", n)
                    head_outs = [outs.add(f"head{j}", n) for j in range(2)] if heads else None
                    with FP.frozen(*inputs_of(srcs, [pm, pu], v, *plan_tensors(csr)), what=what), ops.RangeFlags(DEV):
                        e, vo, _ = ops.mp_layer_forward(pm, srcs, E, csr, bool(i % 2), pu, v, ACT["selu"], store_rows=store, head_outs=head_outs,
                                                        v_out=v_out, v_bound=float(v.abs().max()) if cert else None, e_out=e_out, agg_out=agg_out)
                        ran(lib, what, code)
                        assert (e is None) == (not store) and (e is None or e.data_ptr() == e_out.data_ptr()) and vo.data_ptr() == v_out.data_ptr()
                        outs.check(what)
                HIT.add((code, what.split(" ")[0], "f16x3"))


@lines(lambda: {(K_WS_PRE, f"ws_pre:{x}:{m}", "f16x3") for x in ("stored", "not-stored") for m in ("mean", "sum")})
def test_ws_precomputed_first_layer():
    """ops.mlp_forward_precomputed: rows stored (in the caller's arena) and not stored, mean and sum."""
    nt = F.net(H, (H, H, H), 130)
    plans = [(name, tile_plan(name, deg)) for name, deg in seg_cases()] + [(f"k={K} n_seg={m}", F.csr_of(torch.full((m,), K))) for K, m in dense_cases()]
    for i, (name, csr) in enumerate(plans):
        n, E = csr.n_seg, csr.n
        first = F.table(E, H, 131 + i)
        prods = [ops.Source(F.table(n, H, 132 + i + j), index=F.index(E, n, 134 + i + j).to(torch.int32), additive=True) for j in range(2)]
        for store in (True, False):
            for mean in (True, False):
                what = f"ws_pre:{'stored' if store else 'not-stored'}:{'mean' if mean else 'sum'} {name}"
                outs = Outs()
                with switches("f16x3") as lib:
                    pk = nt.pack([F.Blk(first)], "f16x3")
                    out = outs.add("out", E) if store else None
                    agg_out = outs.add("agg", n)
                    with FP.frozen(*inputs_of(prods, [pk], first, *plan_tensors(csr)), what=what), ops.RangeFlags(DEV):
                        y = ops.mlp_forward_precomputed(pk, first, prods, E, (csr, agg_out, mean), store_rows=store, out=out)
                        ran(lib, what, K_WS_PRE)
                        assert (y is None) == (not store) and (y is None or y.data_ptr() == out.data_ptr())
                        outs.check(what)
                HIT.add((K_WS_PRE, what.split(" ")[0], "f16x3"))


# ====================================================================== the row-split kernels (rounded-bf16 mode)
def tagged(n, seed):
    """bf16 [n, 128] rows tagged as being in the row-split column order (the values are N(0, 1) either way)."""
    return ops.RsOrderedRows.tag(F.table(n, H, seed).to(BF16))


@lines(lambda layers: {(K_RS1, f"rs1:L{layers}:K{K}:{x}", "bf16") for K in (4, 8)
                       for x in ("fp32-rows", "fp32-rows:fp32-adds", "bf16-selu-rows", "no-rows", "no-rows:bf16-agg", "bf16-selu-rows:bf16-agg")})
@pytest.mark.parametrize("layers", [2, 3])
def test_rs1_kernel(layers):
    """mlp_rs1_kernel at uniform in-degree 4 and 8: fp32 rows, compact bf16(SELU) rows, no rows; the fp32 and the bf16 aggregate.  Row
    counts n_seg K around a wave's 16-row chunk and a workgroup's 128 rows."""
    nt = F.net(H, (H,) * layers, 140, True, "ln")
    for K in (4, 8):
        for n_seg in sorted({1, RS_B // K - 1, RS_B // K, RS_B // K + 1, RS_WG // K - 1, RS_WG // K, RS_WG // K + 1, 5 * RS_WG // K + 3} - {0}):
            csr = F.csr_of(torch.full((n_seg,), K))
            E = csr.n
            x = ops.Source(F.rows_of(E, H, "C", 141 + E), pre_act=_lib.ACT_SELU)
            idx = [F.index(E, n_seg, 142 + E + j).to(torch.int32) for j in range(2)]
            adds16 = [ops.Source(tagged(n_seg, 144 + j), index=idx[j], additive=True) for j in range(2)]
            adds32 = [ops.Source(F.table(n_seg, H, 146 + j), index=idx[j], additive=True) for j in range(2)]
            with switches("bf16"):
                pk = ops.PackedMLP(nt.W, nt.b, (nt.ln[0], nt.ln[1], F.R.LN_EPS), [H], [False], precision="bf16", rs_order=True, site="footprint")
            tag = f"rs1:L{layers}:K{K}"
            for label, adds in (("fp32-rows", adds16), ("fp32-rows:fp32-adds", adds32)):
                what = f"{tag}:{label} n_seg={n_seg}"
                outs = Outs()
                with switches("bf16") as lib:
                    out, agg_out = outs.add("out", E), outs.add("agg", n_seg)
                    with FP.frozen(*inputs_of([x] + adds, [pk], *plan_tensors(csr)), what=what):
                        ops.mlp_forward(pk, [x] + adds, E, agg=(csr, agg_out, True), out=out)
                        ran(lib, what, K_RS1)
                        outs.check(what)
                HIT.add((K_RS1, what.split(" ")[0], "bf16"))
            raw_launch(f"{tag}:bf16-selu-rows n_seg={n_seg}", "bf16", pk, [x] + adds16, E, K_RS1, csr, True, out_dtype=BF16, io_out_dtype=2)
            raw_launch(f"{tag}:bf16-selu-rows:bf16-agg n_seg={n_seg}", "bf16", pk, [x] + adds16, E, K_RS1, csr, False, out_dtype=BF16, io_out_dtype=2,
                       agg_dtype=BF16)
            raw_launch(f"{tag}:no-rows n_seg={n_seg}", "bf16", pk, [x] + adds16, E, K_RS1, csr, False)
            raw_launch(f"{tag}:no-rows:bf16-agg n_seg={n_seg}", "bf16", pk, [x] + adds16, E, K_RS1, csr, True, agg_dtype=BF16)


@lines(lambda fmt: {(K_RS2, f"rs2:{fmt}:{r}-rows{h}", "bf16") for r in ("fp32", "bf16") for h in ("", ":heads")})
@pytest.mark.parametrize("fmt", ["rs2", "rs2n"])
def test_rs2_kernel(fmt):
    """mlp_rs2_kernel: [bf16 aggregate | bf16 e] with e in the row-split order (rs2) or in feature order (rs2n), fp32 and bf16 output
    rows, with and without the two bf16 heads."""
    nt = F.net(2 * H, (H, H), 150, True, "ln", n_heads=2)
    ln = (nt.ln[0], nt.ln[1], F.R.LN_EPS)
    with switches("bf16"):
        packs = {h: ops.PackedMLP(nt.W, nt.b, ln, [H, H], [False, False], nt.heads if h else (), precision="bf16", rs2=4 if fmt == "rs2" else 5,
                                  site="footprint") for h in (False, True)}
    for n in N_RS:
        e = tagged(n, 151 + n) if fmt == "rs2" else F.table(n, H, 151 + n).to(BF16)
        srcs = [ops.Source(tagged(n, 152 + n)), ops.Source(e)]
        for dt in (F32, BF16):
            for heads in (False, True):
                what = f"rs2:{fmt}:{'bf16' if dt == BF16 else 'fp32'}-rows{':heads' if heads else ''} n={n}"
                outs = Outs()
                with switches("bf16") as lib:
                    out = outs.add("out", n, H, dt)
                    head_outs = [outs.add(f"head{j}", n, H, BF16) for j in range(2)] if heads else None
                    with FP.frozen(*inputs_of(srcs, [packs[heads]]), what=what):
                        ops.mlp_forward(packs[heads], srcs, n, ACT["selu"], out=out, head_outs=head_outs)
                        ran(lib, what, K_RS2)
                        outs.check(what)
                HIT.add((K_RS2, what.split(" ")[0], "bf16"))


# ====================================================================== the check itself, on real launches
@lines(lambda: {(K_BX6, "control:rows", "f16x3"), (K_BX6, "control:out_idx", "f16x3"), (K_WS, "control:agg", "f16x3")})
def test_the_check_rejects_a_correct_launch_against_a_smaller_claim():
    """Nothing perturbs a launch: the launches are the ones above and pass as they are.  The CHECK is then told that the launch owns
    less than it does — one row fewer, one column fewer, one index fewer, an aggregate one segment shorter — and must name the row or
    column the launch (rightly) wrote as the first stray element."""
    import re
    n = 33
    blks = F.node_blocks(n, "C", 160, "full")
    nt = F.net(2 * H, (H, H, H), 161)
    with switches("f16x3") as lib, ops.RangeFlags(DEV):
        pk, srcs = nt.pack(blks, "f16x3"), [b.source(False) for b in blks]
        view, whole = FP.arena(n, H, F32, device=DEV)
        ops.mlp_forward(pk, srcs, n, out=view)
        ran(lib, "control:rows", K_BX6)
        torch.cuda.synchronize()
    HIT.add((K_BX6, "control:rows", "f16x3"))
    FP.assert_footprint(whole, view, what="control")
    with pytest.raises(AssertionError, match=re.escape(f"{H} element(s) written outside what the launch owns, the first at (row {n - 1}, column 0)") + ".*below"):
        FP.assert_footprint(whole, view[:n - 1], what="control")
    with pytest.raises(AssertionError, match=re.escape(f"{H} element(s) written outside what the launch owns, the first at (row -1, column 0)") + ".*above"):
        FP.assert_footprint(whole, view[1:], what="control")
    with pytest.raises(AssertionError, match=re.escape(f"{n} element(s) written outside what the launch owns, the first at (row 0, column {H - 1})") + ".*right of"):
        FP.assert_footprint(whole, view[:, :H - 1], what="control")
    with pytest.raises(AssertionError, match=re.escape(f"{n} element(s) written outside what the launch owns, the first at (row 0, column -1)") + ".*left of"):
        FP.assert_footprint(whole, view[:, 1:], what="control")
    # an output index: the check is told one index fewer
    oi = torch.randperm(2 * n, generator=F._gen(162))[:n].to(DEV)
    with switches("f16x3") as lib, ops.RangeFlags(DEV):
        view, whole = FP.arena(2 * n, H, F32, device=DEV)
        ops.mlp_forward(pk, srcs, n, out=view, out_idx32=oi.to(torch.int32))
        ran(lib, "control:out_idx", K_BX6)
        torch.cuda.synchronize()
    HIT.add((K_BX6, "control:out_idx", "f16x3"))
    FP.assert_footprint(whole, view, written_rows=oi, what="control")
    with pytest.raises(AssertionError, match=re.escape(f"(row {int(oi[-1])}, column 0)") + ".*in a row nobody owns"):
        FP.assert_footprint(whole, view, written_rows=oi[:-1], what="control")
    with pytest.raises(AssertionError, match=re.escape(f"{n * H} owned element(s) left unwritten")):
        FP.assert_footprint(whole, view, what="control")
    # the fused aggregate of mlp_ws_kernel: the check is told one segment fewer
    csr = tile_plan("ragged", F.ragged_degrees(47, 300))
    mb, _ = F.message_blocks(csr.n, csr.n_seg, "C", 163)
    mt = ws_net(3, False, 164)
    with switches("f16x3", 2) as lib, ops.RangeFlags(DEV):
        agg, a_whole = FP.arena(csr.n_seg, H, F32, device=DEV)
        assert ops.mlp_forward(mt.pack(mb, "f16x3"), [b.source(False) for b in mb], csr.n, agg=(csr, agg, True), store_rows=False) is None
        ran(lib, "control:agg", K_WS)
        torch.cuda.synchronize()
    HIT.add((K_WS, "control:agg", "f16x3"))
    FP.assert_footprint(a_whole, agg, what="control")
    with pytest.raises(AssertionError, match=re.escape(f"(row {csr.n_seg - 1}, column 0)") + ".*below"):          # (an empty segment's zero row)
        FP.assert_footprint(a_whole, agg[:-1], what="control")
