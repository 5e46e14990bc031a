"""Row addressing of the launches past the 32-bit offset boundaries: operands of M_TALL = 2^24 + 4096 + 37 rows at the production leading
dimension (tests/tall_cases.py: row 2^22 of an fp32 [M, 128] operand lies 2^31 bytes from its base, row 2^23 lies 2^32 bytes, row 2^24
is element 2^31), reached through the ops wrappers the models use.  Every launch gets two checks:

(a) windows — the first 256 rows, 256 rows on either side of every boundary row, the last 256 + tail rows — against the plain reference
    the launch already has (oracle/mem_ref.py, fwd_ref.py, grad_ref.py, bf16_ref.py; tests/moments_ref.py, spectrum_ref.py,
    modes_ref.py), under that suite's own criterion: bit equality for integer data and the exact helpers, `assert_fp32_class` /
    `assert_as_accurate_as_fp32` / `assert_bf16_order_noise` for the bounded ones.  No tolerance is introduced here;
(b) the whole tall output, bit for bit, against the same launch issued as row slabs of fewer than 2^30 bytes (slab edges multiples of
    64 rows and of the segment length; the slab shapes are those the small suites pin), with the same kernel code on both sides.

An operand is tall only where it has to be: a gathered source or a scattered output is tall on its own and its launch has a few
thousand rows whose index names rows inside the windows; only the direct cases run M_TALL rows.  Tall outputs sit between guard rows
(footprint.arena at the production leading dimension), inputs are `frozen` — a tall one is compared with its generating function
instead of a copy where three tall tensors are live —, rows that no index names keep their bits.  A test holds at most 40 GiB.
Outputs whose bits legitimately depend on position (sums over all rows, the row-split kernel's aggregate) are listed with the line
of code that causes it in tests/TALL_MEASURED.md and held to their fp64 reference instead of (b).
tests/test_tall_host.py is the negative control.  With G4C_TALL_REPORT=<path> the kernel, wall time and peak memory of every test are
written there (tests/TALL_MEASURED.md)."""
import gc
import os
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

import footprint as FP                                  # noqa: E402
import mem_cases as K                                   # noqa: E402
import tall_cases as T                                  # noqa: E402
import test_gpu_fwd_ref as FR                           # noqa: E402
from graphs4cfd_amd import _lib, ops, plan              # noqa: E402
from oracle import fwd_ref as R                         # noqa: E402
from oracle import mem_ref as M                         # noqa: E402

DEV = torch.device("cuda", 0)
F32, F64, I32, I64 = torch.float32, torch.float64, torch.int32, torch.int64
H = T.H
ACT = {None: _lib.ACT_NONE, "selu": _lib.ACT_SELU, "tanh": _lib.ACT_TANH}
M_TALL = T.M_TALL
SLAB = 6 * 64 * 5450          # rows of a slab: a multiple of 64 and of the degree 6, 1 071 513 600 bytes of fp32 rows < 2^30
MEM_LIMIT = 40 * 2 ** 30
REPORT = []                   # (test, kernel, seconds, peak bytes)
RAN = []                      # kernels the current test asserted


@pytest.fixture(autouse=True)
def _measured(request):
    """Inference mode; wall time and peak memory of the test; nothing of it stays allocated."""
    torch.cuda.init()
    gc.collect(); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats(DEV)
    del RAN[:]
    t0 = time.perf_counter()
    with torch.no_grad():
        yield
    torch.cuda.synchronize()
    dt, peak = time.perf_counter() - t0, torch.cuda.max_memory_allocated(DEV)
    gc.collect(); torch.cuda.empty_cache()
    REPORT.append((request.node.name, ", ".join(dict.fromkeys(RAN)) or "-", dt, peak))
    print(f"  {request.node.name}: {dt:.1f} s, peak {peak / 2 ** 30:.1f} GiB")
    assert peak <= MEM_LIMIT, f"{peak / 2 ** 30:.1f} GiB live"


@pytest.fixture(scope="module", autouse=True)
def _report():
    del REPORT[:]
    yield
    path = os.environ.get("G4C_TALL_REPORT")
    if path:
        with open(path, "w") as f:
            f.write("| test | kernel | wall time (s) | peak memory (GiB) |\n|---|---|---|---|\n")
            for name, kern, dt, peak in REPORT:
                f.write(f"| {name} | {kern} | {dt:.1f} | {peak / 2 ** 30:.1f} |\n")


# ====================================================================== operands, windows, comparisons
def tall(rows, cols, seed, kind="float", dtype=F32):
    return T.fill_(torch.empty((rows, cols), dtype=dtype, device=DEV), seed, kind)


def rows_of(seed, rows, cols=H, kind="float", dtype=F32, col0=0):
    """The rows `rows` (any int64 tensor) of operand `seed`, on the device, without the operand."""
    return T.value(seed, rows.to(DEV), cols, kind, dtype, col0)


def out_arena(rows, cols=H, dtype=F32):
    """(view, whole): a tall output at its production leading dimension between 64 guard rows of the pattern."""
    return FP.arena(rows, cols, dtype, col0=0, pad_cols=0, device=DEV)


def same_bits(a, b, what):
    at = FP.equal_bits_chunked(a, b)
    assert at is None, f"{what}: the tall launch and its slabs differ, first in row {at}"


def still_holds(t, seed, kind="float", what="", chunk=1 << 18):
    """`frozen` for a tall input without a copy of it: the operand still equals its generating function, bit for bit, chunk by chunk."""
    for lo in range(0, int(t.size(0)), chunk):          # (the int64 temporaries of `value` stay at 256 MB for 128 columns)
        hi = min(lo + chunk, int(t.size(0)))
        want = T.value(seed, torch.arange(lo, hi, dtype=I64, device=t.device), int(t.size(1)), kind, t.dtype)
        assert FP.equal_bits_chunked(t[lo:hi], want) is None, f"{what}: a tall input changed in rows {lo} .. {hi}"


def slabs(n, step=SLAB):
    return [(lo, min(lo + step, n)) for lo in range(0, n, step)]


def windows(n=M_TALL, row_bytes=4 * H, cols=H, tail=0, elements=True):
    wins = T.tall_windows(n, row_bytes, cols, tail, elements)
    assert len(wins) >= 3, wins          # the operand reaches a boundary
    return wins, T.window_rows(wins, DEV)


def window_index(n, rows, seed):
    """int64 [n] on the device: entries drawn from `rows` (the window rows of a tall operand), every window row named at least once when
    n allows, in random order."""
    g = torch.Generator().manual_seed(seed)
    pick = torch.cat([torch.randperm(int(rows.numel()), generator=g), torch.randint(0, int(rows.numel()), (max(n - int(rows.numel()), 0),), generator=g)])[:n]
    return rows[pick[torch.randperm(n, generator=g)].to(DEV)]


def uniform_csr(n_seg, k, first=0):
    off = (torch.arange(n_seg + 1, dtype=I64) * k).to(I32)
    c = plan.CsrPlan(perm=None, off=off.to(DEV), n=n_seg * k, n_seg=n_seg, max_deg=k, uniform_deg=k)
    plan.remember_host(c.off, off)
    return c


# ====================================================================== segment_reduce
SEG_PATTERN = (0, 1, 2, 3, 4, 5, 7, 8, 9, 12)          # 51 rows per ten segments: the batch of 8 and its half-batch switch at 4


def seg_offsets(n_rows):
    """int64 offsets on the host: SEG_PATTERN repeated over n_rows rows, what is left (< 51 rows) in one last segment."""
    blocks = n_rows // sum(SEG_PATTERN)
    lens = torch.tensor(SEG_PATTERN, dtype=I64).repeat(blocks)
    lens = torch.cat([lens, torch.tensor([n_rows - blocks * sum(SEG_PATTERN)], dtype=I64)])
    off = torch.zeros(int(lens.numel()) + 1, dtype=I64)
    off[1:] = torch.cumsum(lens, 0)
    return off


def csr_from(off, perm=None):
    o32 = off.to(I32)
    lens = off[1:] - off[:-1]
    c = plan.CsrPlan(perm=perm, off=o32.to(DEV), n=int(off[-1]), n_seg=int(off.numel()) - 1, max_deg=int(lens.max()))
    plan.remember_host(c.off, o32)
    return c


@pytest.mark.parametrize("kernel", ["vector", "scalar"])
def test_segment_reduce_direct_tall_source(kernel):
    """Rows in plan order, no permutation: the source is tall (M_TALL rows), the output has a fifth as many rows.  `scalar`: the same
    rows through a [:, 1:128] view — a base 4 bytes off 16-byte alignment, the leading dimension still 128."""
    whole = tall(M_TALL, H, 11, "int")
    src = whole if kernel == "vector" else whole[:, 1:]
    c0, width = (0, H) if kernel == "vector" else (1, H - 1)
    assert (src.data_ptr() % 16 == 0) == (kernel == "vector") and src.stride(0) == H
    RAN.append(f"segment_reduce_{kernel}_kernel")
    off = seg_offsets(M_TALL)
    csr = csr_from(off)
    wins, _ = windows()
    with FP.frozen(whole, csr.off, what="segment_reduce"):
        outs = {}
        for mean in (False, True):
            view, arena = out_arena(csr.n_seg, width)
            ops.segment_reduce(src, csr, mean, out=view)
            FP.assert_footprint_chunked(arena, view, what=f"segment_reduce mean={mean}")
            outs[mean] = view
    # (a) the segments that touch a window of the SOURCE, against the fp64 reference on those rows alone
    for lo, hi in wins:
        s0 = int(torch.searchsorted(off, torch.tensor(lo), right=True)) - 1
        s1 = min(int(torch.searchsorted(off, torch.tensor(hi - 1), right=True)), csr.n_seg)
        local = off[s0:s1 + 1] - off[s0]
        rows = T.value(11, torch.arange(int(off[s0]), int(off[s1])), width, "int", col0=c0)
        ref, absref = M.segment_reduce(rows, local, None, False)
        M.check_int_bound(absref)
        M.assert_exact(outs[False][s0:s1].cpu(), ref, f"sum, source rows {lo} .. {hi}")
        M.assert_exact(outs[True][s0:s1].cpu(), M.segment_mean_fp32(rows, local, None), f"mean, source rows {lo} .. {hi}")
    # (b) slabs of whole segments: 640 segments are 51 x 64 rows
    per = 640 * (SLAB // (51 * 64))
    for s0, s1 in slabs(csr.n_seg, per):
        r0, r1 = int(off[s0]), int(off[s1])
        assert (r1 - r0) * 4 * H < 2 ** 30 and r0 % 64 == 0
        part = csr_from(off[s0:s1 + 1] - off[s0])
        for mean in (False, True):
            same_bits(outs[mean][s0:s1], ops.segment_reduce(src[r0:r1], part, mean), f"segment_reduce {kernel} mean={mean} segments {s0} ..")


@pytest.mark.parametrize("kernel", ["vector", "scalar"])
def test_segment_reduce_tall_source_through_perm_and_tall_output(kernel):
    """(1) 1031 segments of the small suite's lengths whose permutation names window rows of a tall source; (2) M_TALL segments of one row
    each, gathered from a small table: the OUTPUT is tall."""
    whole = tall(M_TALL, H, 12, "int")
    src = whole if kernel == "vector" else whole[:, 1:]
    c0, width = (0, H) if kernel == "vector" else (1, H - 1)
    RAN.append(f"segment_reduce_{kernel}_kernel")
    _, wrows = windows()
    off = K.offsets(K.seg_lengths(1031)).long()
    perm = window_index(int(off[-1]), wrows, 13)
    csr = csr_from(off, perm.to(I32))
    compact = rows_of(12, perm, width, "int", col0=c0)
    with FP.frozen(whole, what="segment_reduce perm"):
        for mean in (False, True):
            got = ops.segment_reduce(src, csr, mean)
            ref = M.segment_reduce(compact.cpu(), off, None, False)[0] if not mean else M.segment_mean_fp32(compact.cpu(), off, None)
            M.assert_exact(got.cpu(), ref, f"perm, mean={mean}")
            same_bits(got, ops.segment_reduce(compact, csr_from(off), mean), f"perm {kernel} mean={mean} against the compact source")
    del whole, src
    # (2) out[s] = table[perm[s]]
    table = tall(4099, H, 14, "int")
    tsrc = table if kernel == "vector" else table[:, 1:]
    idx = torch.randint(0, 4099, (M_TALL,), generator=torch.Generator().manual_seed(15)).to(DEV)
    one = csr_from(torch.arange(M_TALL + 1, dtype=I64), idx.to(I32))
    view, arena = out_arena(M_TALL, width)
    ops.segment_reduce(tsrc, one, True, out=view)
    FP.assert_footprint_chunked(arena, view, what="segment_reduce tall out")
    wins, wrows = windows()
    assert torch.equal(view[wrows], rows_of(14, idx[wrows], width, "int", col0=c0))
    for lo, hi in slabs(M_TALL):
        part = csr_from(torch.arange(hi - lo + 1, dtype=I64), idx[lo:hi].to(I32))
        same_bits(view[lo:hi], ops.segment_reduce(tsrc, part, True), f"segment_reduce {kernel} tall out rows {lo} ..")


# ====================================================================== weighted_segment_mean
def test_weighted_segment_mean_tall_x_and_tall_out():
    """257 segments of 5 neighbours: x is tall and read through x_idx (window rows), out is tall and written through out_idx (window
    rows); every other row of out keeps its bits."""
    RAN.append("weighted_segment_mean_kernel")
    c = K.wm_case(5, 128, 257, "int", True)
    _, wrows = windows()
    x = tall(M_TALL, H, 21, "int")
    x_idx = window_index(c["n"], wrows, 22)
    out_idx = wrows[torch.randperm(int(wrows.numel()), generator=torch.Generator().manual_seed(23))[:257].to(DEV)]
    csr = plan.CsrPlan(perm=None, off=c["off"].to(DEV), n=c["n"], n_seg=257, max_deg=5, uniform_deg=5)
    view, arena = out_arena(M_TALL)
    w = c["w"].to(DEV)
    with FP.frozen(x, w, what="weighted_segment_mean"):
        ops.weighted_segment_mean(x, x_idx.to(I32), w, csr, view, out_idx.to(I32))
    written = torch.zeros(M_TALL, dtype=torch.bool, device=DEV)
    written[out_idx] = True
    FP.assert_footprint_chunked(arena, view, written, what="weighted_segment_mean")
    # the compact launch: the same rows from a compact x into a compact out
    xc = rows_of(21, x_idx, H, "int")
    ref, _ = M.weighted_segment_mean(xc.cpu(), torch.arange(c["n"]), c["w"], c["off"])
    M.assert_exact(view[out_idx].cpu(), ref, "weighted_segment_mean, tall x and out")
    small = ops.weighted_segment_mean(xc, torch.arange(c["n"], dtype=I32, device=DEV), w, csr)
    same_bits(view[out_idx], small, "weighted_segment_mean against the compact launch")


# ====================================================================== layer_norm, activation_, copy_cols, add_cols
def test_layer_norm_tall():
    RAN.append("layer_norm_rows_kernel")
    x = tall(M_TALL, H, 31)
    g = torch.Generator().manual_seed(32)
    gamma, beta = (1 + 0.3 * torch.randn(H, generator=g)), 0.2 * torch.randn(H, generator=g)
    view, arena = out_arena(M_TALL)
    with FP.frozen(x, what="layer_norm"):
        ops.layer_norm(x, gamma.to(DEV), beta.to(DEV), K.LN_EPS, ACT["selu"], out=view)
    FP.assert_footprint_chunked(arena, view, what="layer_norm")
    _, wrows = windows(tail=M_TALL % 4)
    M.assert_fp32_class(view[wrows].cpu(), *M.layer_norm(rows_of(31, wrows).cpu(), gamma, beta, K.LN_EPS, "selu"), M.n_eff_layer_norm(H, "selu"),
                        "layer_norm, windows")
    for lo, hi in slabs(M_TALL):
        same_bits(view[lo:hi], ops.layer_norm(x[lo:hi], gamma.to(DEV), beta.to(DEV), K.LN_EPS, ACT["selu"]), f"layer_norm rows {lo} ..")
    # in place, the way the models call it: the same bits
    ops.layer_norm(x, gamma.to(DEV), beta.to(DEV), K.LN_EPS, ACT["selu"], out=x)
    same_bits(x, view, "layer_norm in place")


def test_activation_inplace_tall():
    """2^31 + ... elements of one contiguous tensor: the element index itself passes 2^31."""
    RAN.append("activation_kernel")
    view, arena = out_arena(M_TALL)
    T.fill_(view, 41)
    keep = view[: SLAB].clone()
    ops.activation_(view, ACT["tanh"])
    FP.assert_footprint_chunked(arena, view, what="activation_")
    _, wrows = windows()
    M.assert_fp32_class(view[wrows].cpu(), *M.activation(rows_of(41, wrows).cpu(), "tanh"), M.N_EFF_ACT, "activation_, windows")
    for lo, hi in slabs(M_TALL):
        part = keep[: hi - lo] if lo == 0 else T.value(41, torch.arange(lo, hi, device=DEV), H)
        same_bits(view[lo:hi], ops.activation_(part.contiguous(), ACT["tanh"]), f"activation_ rows {lo} ..")


def test_copy_cols_tall():
    """Direct: M_TALL rows of a 128-wide window copied between tall tensors; gathered: a tall source through an index of window rows."""
    RAN.append("copy_cols_kernel")
    src = tall(M_TALL, H, 51)
    view, arena = out_arena(M_TALL)
    with FP.frozen(src, what="copy_cols"):
        ops.copy_cols(src, view, 0)
    FP.assert_footprint_chunked(arena, view, what="copy_cols")
    wins, wrows = windows()
    assert torch.equal(view[wrows], rows_of(51, wrows)), "copy_cols, windows"
    same_bits(view, src, "copy_cols")          # (the copy itself is the slab reference: every slab of a copy is the source's slab)
    # a 3-wide window at an odd column, rows through an index
    idx = window_index(4099, wrows, 52)
    dst = FP.fill(torch.empty((4099 + 40, 7), device=DEV))
    ops.copy_cols(src, dst, 2, scol0=5, width=3, idx32=idx.to(I32), n_rows=4099)
    want = FP.fill(torch.empty((4099 + 40, 7), device=DEV))
    want[:4099, 2:5] = rows_of(51, idx, 3, col0=5)
    same_bits(dst, want, "copy_cols gathered")


def test_add_cols_tall():
    RAN.append("add_cols_kernel")
    a, b = tall(M_TALL, H, 61, "int"), tall(M_TALL, H, 62, "int")
    view, arena = out_arena(M_TALL)
    ops.add_cols(a, 0, b, view)
    still_holds(a, 61, "int", "add_cols a"); still_holds(b, 62, "int", "add_cols b")          # (three tall tensors, no copies)
    FP.assert_footprint_chunked(arena, view, what="add_cols")
    _, wrows = windows()
    assert torch.equal(view[wrows].cpu(), M.add_cols(rows_of(61, wrows, kind="int"), 0, rows_of(62, wrows, kind="int"))), "add_cols, windows"
    for lo, hi in slabs(M_TALL):
        tmp = torch.empty((hi - lo, H), device=DEV)
        same_bits(view[lo:hi], ops.add_cols(a[lo:hi], 0, b[lo:hi], tmp), f"add_cols rows {lo} ..")


# ====================================================================== project_to_edges, edge_scalar_to_node_vector
def test_project_to_edges_tall():
    """n_feat 64: v rows are 128 wide.  Direct: M_TALL edges read row e; gathered: 4099 edges read window rows."""
    RAN.append("project_to_edges_kernel")
    v = tall(M_TALL, H, 71, "int")
    unit = tall(M_TALL, 2, 72, "int")
    wins, wrows = windows()
    with FP.frozen(v, unit, what="project_to_edges"):
        out = ops.project_to_edges(v, None, unit, M_TALL, 64)
        idx = window_index(4099, wrows, 73)
        got = ops.project_to_edges(v, idx.to(I32), unit[:4099].contiguous(), 4099, 64)
    ref, absref = M.project_to_edges(rows_of(71, wrows, kind="int").cpu(), None, rows_of(72, wrows, 2, "int").cpu(), 64)
    M.check_int_bound(absref)
    M.assert_exact(out[wrows].cpu(), ref, "project_to_edges, windows")
    for lo, hi in slabs(M_TALL):
        same_bits(out[lo:hi], ops.project_to_edges(v[lo:hi], None, unit[lo:hi], hi - lo, 64), f"project_to_edges rows {lo} ..")
    M.assert_exact(got.cpu(), M.project_to_edges(rows_of(71, idx, kind="int").cpu(), None, unit[:4099].cpu(), 64)[0], "project_to_edges gathered")
    same_bits(got, ops.project_to_edges(rows_of(71, idx, kind="int"), None, unit[:4099].contiguous(), 4099, 64), "project_to_edges gathered, compact")


def test_edge_scalar_to_node_vector_tall():
    """k = 4 incoming edges per node, 128 features: e is tall (M_TALL rounded down to whole nodes), out [n_nodes, 256] has a quarter of
    the rows at twice the width — 2^32 bytes at node 2^22."""
    RAN.append("edge_scalar_to_node_vector_kernel")
    k = 4
    n_nodes = M_TALL // k
    e = tall(n_nodes * k, H, 81, "int")
    ui = tall(n_nodes, 2 * k, 82, "int")
    view, arena = out_arena(n_nodes, 2 * H)
    with FP.frozen(e, ui, what="edge_scalar_to_node_vector"):
        ops.edge_scalar_to_node_vector(e, ui.view(n_nodes, 2, k), n_nodes, k, out=view)
    FP.assert_footprint_chunked(arena, view, what="edge_scalar_to_node_vector")
    # windows of the OUTPUT's nodes; they cover the windows of e's rows (node n reads rows 4 n ..)
    wins = T.windows(n_nodes, sorted({b // k for b in T.boundary_rows(4 * H, H, n_nodes * k)} | set(T.boundary_rows(8 * H, 2 * H, n_nodes))))
    nodes = T.window_rows(wins, DEV)
    erows = (nodes[:, None] * k + torch.arange(k, device=DEV)[None, :]).reshape(-1)
    ref, absref = M.edge_scalar_to_node_vector(rows_of(81, erows, kind="int").cpu(), rows_of(82, nodes, 2 * k, "int").cpu().view(-1, 2, k), k)
    M.check_int_bound(absref)
    M.assert_exact(view[nodes].cpu(), ref, "edge_scalar_to_node_vector, windows")
    for lo, hi in slabs(n_nodes, SLAB // k):
        part = ops.edge_scalar_to_node_vector(e[lo * k:hi * k], ui[lo:hi].view(-1, 2, k), hi - lo, k)
        same_bits(view[lo:hi], part, f"edge_scalar_to_node_vector nodes {lo} ..")


# ====================================================================== rollout_advance
RA_NODES, RA_NF = 2 ** 20, 3


def _advance(layout, steps, at):
    """One launch with the step index preset to each of `at`: the step's slice equals pred, every other slice keeps the pattern."""
    RAN.append("rollout_advance_record_kernel<0>" if layout == "snap" else "rollout_advance_kernel")
    n, nf = RA_NODES, RA_NF
    shape = (n, nf * steps) if layout == "rows" else (steps, n, nf)          # ("snap": the snapshot slots of rollout_advance_record)
    outputs = FP.fill(torch.empty(shape, device=DEV))
    idt, pat = FP.PATTERN[4]
    field0 = tall(n, 5 * nf, 91)
    done = []
    for j, t in enumerate(at):
        pred = tall(n, nf, 92 + j)
        field = field0.clone()
        step = torch.tensor([t, 0], dtype=I32, device=DEV)
        with FP.frozen(pred, what="rollout_advance"):
            if layout == "snap":
                ops.rollout_advance_record(field, pred, step, nf, steps, snap=outputs, every=1)
            else:
                ops.rollout_advance(field, pred, outputs, step, nf)
        assert step.tolist() == [t + 1, 0]
        assert torch.equal(field, torch.cat((field0[:, nf:], pred), 1)), f"field after step {t}"
        done.append((t, pred))
        # every slice: pred where a launch wrote it, the pattern everywhere else
        if layout != "rows":
            for lo in range(0, steps, 64):
                blk = outputs[lo:lo + 64].view(idt).clone()
                for tt, pp in done:
                    if lo <= tt < lo + 64:
                        assert torch.equal(outputs[tt], pp), f"slice {tt} is not pred ({layout})"
                        blk[tt - lo] = pat
                assert bool((blk == pat).all()), f"a slice in {lo} .. {lo + 64} that no launch owns changed (step {t}, {layout})"
        else:
            for lo in range(0, n, 2 ** 16):
                blk = outputs[lo:lo + 2 ** 16].view(idt).clone()
                for tt, pp in done:
                    assert torch.equal(outputs[lo:lo + 2 ** 16, nf * tt:nf * (tt + 1)], pp[lo:lo + 2 ** 16]), f"slice {tt} is not pred ({layout})"
                    blk[:, nf * tt:nf * (tt + 1)] = pat
                assert bool((blk == pat).all()), f"a slot of rows {lo} .. that no launch owns changed (step {t}, {layout})"


def test_rollout_advance_step_major_tall():
    """[steps, 2^20, 3] outputs: a step's slice is 12 MiB, slice 171 starts below 2^31 bytes and ends above, 342 likewise for 2^32
    bytes, 683 for 2^31 elements.  The slices just below, across and just above each boundary."""
    plane = RA_NODES * RA_NF
    cross = [2 ** 31 // (4 * plane), 2 ** 32 // (4 * plane), 2 ** 31 // plane]
    assert cross == [170, 341, 682] and all((c * plane * 4 < b <= (c + 1) * plane * 4) for c, b in zip(cross[:2], (2 ** 31, 2 ** 32)))
    at = [c + d for c in cross for d in (-1, 0, 1)]
    _advance("steps", 700, at)


def test_rollout_advance_record_snapshot_slots_tall():
    """g4c_rollout_advance_record with every = 1: step t goes into snapshot slot t of [700, 2^20, 3] — the slots just below, across and
    just above each boundary, as the step-major outputs of rollout_advance."""
    plane = RA_NODES * RA_NF
    cross = [2 ** 31 // (4 * plane), 2 ** 32 // (4 * plane), 2 ** 31 // plane]
    _advance("snap", 700, [c + d for c in cross for d in (-1, 0, 1)])


def test_rollout_advance_record_probes_and_statistics_tall():
    """g4c_rollout_advance_record with a tall row-major target [2^20, 3 x 700] (every launch reads one 3-column slot of every row: the
    row offsets cross all three boundaries), a tall probe buffer [700, 2^20, 3] (slot t starts below / across / above each boundary)
    and the error statistics.  Integer predictions and targets: every sum is exact in fp64 in any order, so stats[t] equals plain
    fp64 torch sums on the device bit for bit; the probe slot equals pred[probe_rows]; every other slot and row of stats keeps its
    pattern."""
    RAN.append("rollout_advance_record_kernel<3>, g4c::partials_kernel (3 fields)")
    n, nf, steps = RA_NODES, RA_NF, 700
    plane = n * nf
    cross = [2 ** 31 // (4 * plane), 2 ** 32 // (4 * plane), 2 ** 31 // plane]
    target = T.fill_(torch.empty((n, nf * steps), device=DEV), 301, "int", chunk=1 << 14)
    probe_rows = torch.randperm(n, generator=torch.Generator().manual_seed(302)).to(DEV, I32)
    probe_out = FP.fill(torch.empty((steps, n, nf), device=DEV))
    stats = FP.fill(torch.empty((steps, nf, _lib.REC_NSTAT), dtype=F64, device=DEV))
    mask = (torch.arange(n, device=DEV) % 3 == 0).to(torch.uint8)
    scratch = ops.rollout_record_scratch(n, nf, DEV)
    field0 = tall(n, 5 * nf, 303, "int")
    i32, p32 = FP.PATTERN[4]
    i64, p64 = FP.PATTERN[8]
    done = []
    for j, t in enumerate([c + d for c in cross for d in (-1, 0, 1)] + [0, steps - 1]):
        pred = tall(n, nf, 304 + j, "int")
        field, step = field0.clone(), torch.tensor([t, 0], dtype=I32, device=DEV)
        with FP.frozen(pred, probe_rows, mask, what="rollout_advance_record"):
            ops.rollout_advance_record(field, pred, step, nf, steps, probe_rows=probe_rows, probe_out=probe_out, target=target, mask=mask,
                                       stats=stats, scratch=scratch)
        assert step.tolist() == [t + 1, 0] and torch.equal(field, torch.cat((field0[:, nf:], pred), 1))
        assert torch.equal(probe_out[t], pred[probe_rows.long()]), f"probe slot {t}"
        yt = target[:, nf * t:nf * (t + 1)].double()
        d = pred.double() - yt
        want = torch.empty((nf, _lib.REC_NSTAT), dtype=F64, device=DEV)
        want[:, _lib.REC_SQ_ERR], want[:, _lib.REC_ABS_ERR], want[:, _lib.REC_MAX_ABS_ERR] = (d * d).sum(0), d.abs().sum(0), d.abs().amax(0)
        want[:, _lib.REC_TGT_SUM], want[:, _lib.REC_TGT_SQ_SUM] = yt.sum(0), (yt * yt).sum(0)
        want[:, _lib.REC_ABS_ERR_MASK] = (d.abs() * mask[:, None].double()).sum(0)
        assert torch.equal(stats[t], want), f"statistics of step {t}: {stats[t].tolist()} vs {want.tolist()}"
        done.append(t)
    still_holds(target, 301, "int", "rollout_advance_record target", chunk=1 << 14)
    kept = torch.ones(steps, dtype=torch.bool, device=DEV)
    kept[done] = False
    assert bool((stats.view(i64)[kept] == p64).all()), "a statistics row of a step that was not taken changed"
    for lo in range(0, steps, 64):
        blk = probe_out[lo:lo + 64].view(i32)
        assert bool((blk[kept[lo:lo + 64]] == p32).all()), f"a probe slot in {lo} .. that no launch owns changed"


def test_rollout_advance_row_major_tall():
    """[2^20, 3 x 700] outputs: every launch writes one 3-column slot of EVERY row, rows 8400 bytes apart — the row offsets of one launch
    cross all three boundaries.  The first slot, one in the middle, the last."""
    assert RA_NODES * RA_NF * 700 > 2 ** 31 + 4096 * RA_NF * 700
    _advance("rows", 700, [0, 350, 699])


# ====================================================================== g4c_mlp_run
def _net(k_in, layers, seed, n_heads=0):
    return FR.net(k_in, (H,) * layers, seed, True, "ln", n_heads=n_heads)


def _launch(lib, pk, sources, n, act, expect, what, **kw):
    y = ops.mlp_forward(pk, sources, n, ACT[act], **kw)
    ran = int(lib.g4c_mlp_last_kernel())
    assert ran == expect, f"{what}: kernel {_lib.KERNEL_NAMES.get(ran)} ({ran}) ran, expected code {expect}"
    return y


def _reference(nt, blocks, adds, act, heads=False):
    """(fp64 rows, fp32 comparator rows[, heads of both]) of the launch on compact blocks."""
    L = R.Launch([R.Src(b) for b in blocks], nt.W, nt.b, nt.ln, act, [R.Add(a) for a in adds])
    return R.ref64(L)["y"], R.evaluate(L, F32)["y"]


def _node_form(prec, expect, certified, what, shapes=0, heads=False, small=None):
    """[tall direct rows | a small table through an index] -> three layers -> LayerNorm -> SELU (+ two heads), M_TALL rows into a tall
    output: (a) windows against fp64, (b) slabs bit for bit, the guard rows, the frozen inputs."""
    RAN.append(_lib.KERNEL_NAMES[expect] + (" (certified)" if certified else ""))
    nt = _net(2 * H, 3, 101, n_heads=2 if heads else 0)
    a = tall(M_TALL, H, 102)
    tab = tall(4099, H, 103)
    idx = torch.randint(0, 4099, (M_TALL,), generator=torch.Generator().manual_seed(104)).to(DEV, I32)
    bound = 3.0 if certified else None          # (tall_cases.value, kind "float": |v| < 3)
    view, arena = out_arena(M_TALL)
    hv = [out_arena(M_TALL) for _ in range(2)] if heads else []
    with FR.switches(prec, 0, 0, small) as lib:
        old_shapes = lib.g4c_mlp_shapes_enable(shapes)
        try:
            pk = nt.pack([FR.Blk(a), FR.Blk(tab)], prec, heads)
            srcs = lambda rows, lo, hi: [ops.Source(rows, bound=bound), ops.Source(tab, idx[lo:hi], bound=bound)]          # noqa: E731
            with ops.RangeFlags(DEV) as flags, FP.frozen(tab, idx, what=what):
                _launch(lib, pk, srcs(a, 0, M_TALL), M_TALL, "selu", expect, what, out=view, head_outs=[h[0] for h in hv] or None)
                shape = int(lib.g4c_mlp_last_shape())
            still_holds(a, 102, what=what)          # (no copy of the tall source: with both heads the test would hold five tall tensors)
            assert prec != "f16x3" or flags.take() == []
            for v_, w_ in [(view, arena)] + hv:
                FP.assert_footprint_chunked(w_, v_, what=what)
            # (a)
            _, wrows = windows(tail=M_TALL % 64)
            ref, c32 = _reference(nt, [rows_of(102, wrows), tab[idx[wrows].long()]], [], "selu")
            R.assert_as_accurate_as_fp32(view[wrows], ref, c32, None, what + ", windows")
            for j, (h, _) in enumerate(hv):
                y = view[wrows]
                R.assert_as_accurate_as_fp32(h[wrows], R.heads(y, nt.heads)[j], R.heads(y, nt.heads, F32)[j], None, f"{what} head{j}, windows")
            # (b) — the slabs of the source from its generating function (it was just compared with it): with both heads the tall
            # source and a slab's three outputs would not fit under the memory limit together
            del a
            for lo, hi in slabs(M_TALL):
                tmp = [torch.empty((hi - lo, H), device=DEV) for _ in range(1 + len(hv))]
                part = T.fill_(torch.empty((hi - lo, H), device=DEV), 102, row0=lo)
                _launch(lib, pk, srcs(part, lo, hi), hi - lo, "selu", expect, f"{what} rows {lo} ..", out=tmp[0], head_outs=tmp[1:] or None)
                for got, (full, _) in zip(tmp, [(view, arena)] + hv):
                    same_bits(full[lo:hi], got, f"{what} rows {lo} ..")
        finally:
            lib.g4c_mlp_shapes_enable(old_shapes)
    return shape


def test_mlp_split_kernel_tall():
    _node_form("fp32", FR.K_SPLIT, False, "split")


@pytest.mark.parametrize("certified", [False, True], ids=["tracked", "certified"])
def test_mlp_tile_kernel_tall(certified):
    """The all-runtime tile kernel (shapes off on both sides: the same kernel code), two-step ring, with both heads."""
    _node_form("f16x3", FR.K_BX6_CERT if certified else FR.K_BX6, certified, "tile", heads=True)


def test_mlp_tile_kernel_bf16x6_tall():
    _node_form("bf16x6", FR.K_BX6, False, "tile bf16x6")


def test_a_tall_output_runs_the_generic_tile_kernel():
    """The shaped tile kernels decline on tall operands (tile_shape_of: a direct source's and the output's byte extent stay below
    2^31): with the shapes ON, two direct 128-wide sources -> three layers -> LayerNorm -> SELU is the node-update shape at 97 rows —
    into an output of its own and into the last 97 rows of the tall output — and the all-runtime kernel at M_TALL rows, whose bits
    equal those of the slabs, which DO take the shape.  (test_gpu_tile_shapes.py has the output guard alone, sources compact.)"""
    lib = _lib.load()
    RAN.append("mlp_bx6_kernel (shapes on)")
    nt = _net(2 * H, 3, 111)
    a, b = tall(M_TALL, H, 112), tall(97, H, 113)
    view, arena = out_arena(M_TALL)
    with FR.switches("f16x3", 0, 0, 0):
        old = lib.g4c_mlp_shapes_enable(1)
        try:
            pk = nt.pack([FR.Blk(a), FR.Blk(b)], "f16x3")
            # two direct 128-wide sources, three layers, LayerNorm: the node-update shape — at 97 rows
            small = _launch(lib, pk, [ops.Source(a[:97]), ops.Source(b)], 97, "selu", FR.K_BX6, "compact")
            assert int(lib.g4c_mlp_last_shape()) == _lib.TILE_SHAPE_NODE
            # the same 97 rows stored into the LAST rows of the tall output: the launch sees out + (M_TALL - 97) rows, an output of 97
            # rows — still the shape; a launch of M_TALL rows into it: generic
            tail = view[M_TALL - 97:]
            _launch(lib, pk, [ops.Source(a[:97]), ops.Source(b)], 97, "selu", FR.K_BX6, "compact into the tail", out=tail)
            assert int(lib.g4c_mlp_last_shape()) == _lib.TILE_SHAPE_NODE and torch.equal(tail, small)
            b_tall = tall(M_TALL, H, 113)
            assert torch.equal(b_tall[:97], b)
            _launch(lib, pk, [ops.Source(a), ops.Source(b_tall)], M_TALL, "selu", FR.K_BX6, "tall", out=view)
            assert int(lib.g4c_mlp_last_shape()) == _lib.TILE_SHAPE_GENERIC
            FP.assert_footprint_chunked(arena, view, what="tall output, shapes on")
            assert torch.equal(view[:97], small), "the generic kernel on the tall output and the node shape on the compact one differ"
            for lo, hi in slabs(M_TALL):
                got = _launch(lib, pk, [ops.Source(a[lo:hi]), ops.Source(b_tall[lo:hi])], hi - lo, "selu", FR.K_BX6, f"slab {lo}")
                assert int(lib.g4c_mlp_last_shape()) == _lib.TILE_SHAPE_NODE
                same_bits(view[lo:hi], got, f"tall output (generic) against its slabs (node shape), rows {lo} ..")
        finally:
            lib.g4c_mlp_shapes_enable(old)


def _message_form(prec, expect, what, ws=0, bx6i=0, certified=False, agg=None):
    """The hoisted message launch: [tall direct e, SELU on load] + two product tables through indices -> three layers -> LayerNorm,
    M rows (a multiple of the degree 6, a partial last tile) into a tall output, with the fused aggregate (`agg`: None / "mean" /
    "sum") of degree 6."""
    RAN.append(_lib.KERNEL_NAMES[expect] + (" (certified)" if certified else ""))
    k = 6
    m = M_TALL - M_TALL % k
    assert m % 32 and m % 64
    nt = _net(H, 3, 121)
    e = tall(m, H, 122)
    tabs = [tall(4099, H, 123), tall(4099, H, 124)]
    idx = [torch.randint(0, 4099, (m,), generator=torch.Generator().manual_seed(125 + j)).to(DEV, I32) for j in range(2)]
    bound = 3.0 if certified else None
    view, arena = out_arena(m)
    csr = uniform_csr(m // k, k) if agg else None
    av, aarena = out_arena(m // k) if agg else (None, None)
    with FR.switches(prec, ws, bx6i) as lib:
        blks = [FR.Blk(e, pre_act="selu"), FR.Blk(tabs[0], additive=True), FR.Blk(tabs[1], additive=True)]
        pk = nt.pack(blks, prec)

        def srcs(lo, hi):
            return [ops.Source(e[lo:hi], pre_act=ACT["selu"], bound=bound)] + [ops.Source(t, i[lo:hi], additive=True, bound=bound) for t, i in zip(tabs, idx)]
        with ops.RangeFlags(DEV) as flags, FP.frozen(e, *tabs, *idx, what=what):
            _launch(lib, pk, srcs(0, m), m, None, expect, what, out=view, agg=(csr, av, agg == "mean") if agg else None)
        assert prec != "f16x3" or flags.take() == []
        FP.assert_footprint_chunked(arena, view, what=what)
        if agg:
            FP.assert_footprint_chunked(aarena, av, what=what + " aggregate")
        # (a) windows of whole segments
        wins = [(lo - lo % k, min(hi + (-hi) % k, m)) for lo, hi in T.tall_windows(m, tail=m % 64)]
        wrows = T.window_rows(wins, DEV)
        L = R.Launch([R.Src(rows_of(122, wrows), pre_act="selu")], nt.W, nt.b, nt.ln, None, [R.Add(t[i[wrows].long()]) for t, i in zip(tabs, idx)])
        R.assert_as_accurate_as_fp32(view[wrows], R.ref64(L)["y"], R.evaluate(L, F32)["y"], None, what + ", windows")
        if agg:          # the header's promise: the fp32 segment reduction of the stored rows, bit for bit
            for lo, hi in wins:
                want = R.segment_reduce_fp32(view[lo:hi].cpu(), torch.arange(0, hi - lo + 1, k), agg == "mean")
                assert torch.equal(av[lo // k:hi // k].cpu(), want), f"{what}: aggregate of rows {lo} .. {hi}"
        # (b)
        for lo, hi in slabs(m):
            tmp = torch.empty((hi - lo, H), device=DEV)
            part = uniform_csr((hi - lo) // k, k) if agg else None
            atmp = torch.empty(((hi - lo) // k, H), device=DEV) if agg else None
            _launch(lib, pk, srcs(lo, hi), hi - lo, None, expect, f"{what} rows {lo} ..", out=tmp, agg=(part, atmp, agg == "mean") if agg else None)
            same_bits(view[lo:hi], tmp, f"{what} rows {lo} ..")
            if agg:
                same_bits(av[lo // k:hi // k], atmp, f"{what} aggregate of rows {lo} ..")


@pytest.mark.parametrize("certified,agg", [(False, None), (False, "mean"), (False, "sum"), (True, None), (True, "mean")],
                         ids=["tracked", "tracked-mean", "tracked-sum", "certified", "certified-mean"])
def test_mlp_ws_kernel_tall(certified, agg):
    _message_form("f16x3", FR.K_WS_CERT if certified else FR.K_WS, "ws", ws=2, certified=certified, agg=agg)


@pytest.mark.parametrize("prec", ["f16x3", "bf16x6"])
@pytest.mark.parametrize("agg", ["mean", "sum"])
def test_mlp_tile_kernel_fused_aggregate_tall(agg, prec):
    """The all-runtime tile kernel on the message form with its fused aggregate (tiles of whole segments: 30 of 32 rows at degree 6)."""
    _message_form(prec, FR.K_BX6, "tile message form", agg=agg)


@pytest.mark.parametrize("agg", [None, "mean"])
def test_mlp_bx6i_kernel_tall(agg):
    _message_form("bf16x6", FR.K_BX6I, "bx6i", bx6i=2, agg=agg)


@pytest.mark.parametrize("kernel", ["split", "tile", "ws", "bx6i"])
def test_mlp_tall_gathered_source_and_scattered_output(kernel):
    """A launch of 4099 rows whose weighted block is gathered from window rows of a tall tensor, whose additive tables are tall and read
    through indices of window rows, and whose rows are scattered through out_idx into window rows of a tall output: against fp64,
    against the same launch on compact operands, and every row of the output that no index names keeps its bits."""
    prec, expect, ws, bx6i = {"split": ("fp32", FR.K_SPLIT, 0, 0), "tile": ("f16x3", FR.K_BX6, 0, 0), "ws": ("f16x3", FR.K_WS, 2, 0), "bx6i": ("bf16x6", FR.K_BX6I, 0, 2)}[kernel]
    RAN.append(_lib.KERNEL_NAMES[expect])
    n = 4099
    nt = _net(H, 3, 131)
    _, wrows = windows()
    e = tall(M_TALL, H, 132)
    tab = tall(M_TALL, H, 133)
    ie, i0, i1 = (window_index(n, wrows, 134 + j) for j in range(3))
    oi = wrows[torch.randperm(int(wrows.numel()), generator=torch.Generator().manual_seed(137))[:n].to(DEV)] if n <= int(wrows.numel()) else None
    assert oi is None or int(oi.unique().numel()) == n
    if oi is None:          # (more launch rows than window rows: every window row, and rows next to the windows)
        oi = torch.cat([wrows, wrows[-1] - 300 - torch.arange(n - int(wrows.numel()), device=DEV)])
        oi = oi[torch.randperm(n, generator=torch.Generator().manual_seed(137)).to(DEV)]
        assert int(oi.unique().numel()) == n and int(oi.min()) >= 0
    view, arena = out_arena(M_TALL)
    with FR.switches(prec, ws, bx6i) as lib:
        pk = nt.pack([FR.Blk(e), FR.Blk(tab, additive=True), FR.Blk(tab, additive=True)], prec)
        srcs = [ops.Source(e, ie.to(I32)), ops.Source(tab, i0.to(I32), additive=True), ops.Source(tab, i1.to(I32), additive=True)]
        with ops.RangeFlags(DEV) as flags:
            _launch(lib, pk, srcs, n, "selu", expect, kernel, out=view, out_idx32=oi.to(I32))
        still_holds(e, 132, what=kernel + " e"); still_holds(tab, 133, what=kernel + " table")          # (three tall tensors, no copies)
        assert prec != "f16x3" or flags.take() == []
        written = torch.zeros(M_TALL, dtype=torch.bool, device=DEV)
        written[oi] = True
        FP.assert_footprint_chunked(arena, view, written, what=kernel)
        ec, t0, t1 = rows_of(132, ie), rows_of(133, i0), rows_of(133, i1)
        L = R.Launch([R.Src(ec)], nt.W, nt.b, nt.ln, "selu", [R.Add(t0), R.Add(t1)])
        R.assert_as_accurate_as_fp32(view[oi], R.ref64(L)["y"], R.evaluate(L, F32)["y"], None, kernel + ", gathered and scattered")
        ar = torch.arange(n, dtype=I32, device=DEV)
        compact = _launch(lib, pk, [ops.Source(ec, ar), ops.Source(t0, ar, additive=True), ops.Source(t1, ar, additive=True)], n, "selu", expect,
                          kernel + " compact", out=torch.empty((n, H), device=DEV), out_idx32=ar)
        same_bits(view[oi], compact, kernel + " against the compact launch")


def test_row_counts_from_2_31_are_refused():
    """The launchers refuse n_rows >= 2^31 (no tensor of that size is touched: the check precedes every access)."""
    nt = _net(H, 3, 141)
    x = torch.zeros((64, H), device=DEV)
    with FR.switches("f16x3"):
        pk = nt.pack([FR.Blk(x)], "f16x3")
        with pytest.raises(Exception, match="n_rows"):
            ops.mlp_forward(pk, [ops.Source(x)], 2 ** 31, out=x)


# ====================================================================== the fused MP layer: mlp_ws_kernel with its node phase
@pytest.mark.parametrize("certified", [False, True], ids=["tracked", "certified"])
def test_mlp_ws_node_phase_tall(certified):
    """ops.mp_layer_forward: the message launch of `_message_form` (degree 6, mean) with the node update in the same workgroups — e'
    tall, v / v' / both heads [M / 6, 128].  (a) e' and v' windows against fp64 (v' from the launch's own e' rows, as
    test_gpu_fwd_ref.mp_layer); (b) slabs of whole segments: a segment's six rows and its node are in one slab."""
    from test_gpu_fwd_ref import Blk
    expect = FR.K_WS_CERT if certified else FR.K_WS
    RAN.append(_lib.KERNEL_NAMES[expect] + " + node phase" + (" (certified)" if certified else ""))
    k = 6
    m = M_TALL - M_TALL % k
    n = m // k
    msg, upd = _net(H, 3, 151), _net(2 * H, 3, 152, n_heads=2)
    e = tall(m, H, 153)
    v = tall(n, H, 154)
    tabs = [tall(4099, H, 155), tall(4099, H, 156)]
    idx = [torch.randint(0, 4099, (m,), generator=torch.Generator().manual_seed(157 + j)).to(DEV, I32) for j in range(2)]
    bound = 3.0 if certified else None
    csr = uniform_csr(n, k)
    e_out, e_arena = out_arena(m)
    v_out, v_arena = out_arena(n)
    heads = [out_arena(n) for _ in range(2)]
    with FR.switches("f16x3", 2, 0) as lib:
        blks = [Blk(e, pre_act="selu"), Blk(tabs[0], additive=True), Blk(tabs[1], additive=True)]
        pm, pu = msg.pack(blks, "f16x3"), upd.pack([Blk(v), Blk(v)], "f16x3", heads=True)

        def srcs(lo, hi):
            return [ops.Source(e[lo:hi], pre_act=ACT["selu"], bound=bound)] + [ops.Source(t, i[lo:hi], additive=True, bound=bound) for t, i in zip(tabs, idx)]
        with ops.RangeFlags(DEV) as flags, FP.frozen(v, *tabs, *idx, what="mp_layer"):
            ops.mp_layer_forward(pm, srcs(0, m), m, csr, True, pu, v, ACT["selu"], head_outs=[h[0] for h in heads], v_out=v_out,
                                 v_bound=bound, e_out=e_out)
            assert int(lib.g4c_mlp_last_kernel()) == expect
        assert flags.take() == []
        still_holds(e, 153, what="mp_layer e")
        for view, arena in [(e_out, e_arena), (v_out, v_arena)] + heads:
            FP.assert_footprint_chunked(arena, view, what="mp_layer")
        # (a) windows of nodes: those whose rows touch a window of e, and the windows of the node tensors themselves
        nwins = T.windows(n, sorted({b // k for b in T.boundary_rows(4 * H, H, m)} | set(T.boundary_rows(4 * H, H, n))), tail=64)
        nodes = T.window_rows(nwins, DEV)
        erows = (nodes[:, None] * k + torch.arange(k, device=DEV)[None, :]).reshape(-1)
        L = R.Launch([R.Src(rows_of(153, erows), pre_act="selu")], msg.W, msg.b, msg.ln, None, [R.Add(t[i[erows].long()]) for t, i in zip(tabs, idx)])
        R.assert_as_accurate_as_fp32(e_out[erows], R.ref64(L)["y"], R.evaluate(L, F32)["y"], None, "mp_layer e', windows")
        off = torch.arange(0, int(erows.numel()) + 1, k, device=DEV)
        vw = rows_of(154, nodes)
        r64 = R.mp_layer(L, off, True, upd.W, upd.b, upd.ln, vw, "selu", F64, e_rows=e_out[erows])
        r32 = R.mp_layer(L, off, True, upd.W, upd.b, upd.ln, vw, "selu", F32, e_rows=e_out[erows])
        R.assert_as_accurate_as_fp32(v_out[nodes], r64["v"], r32["v"], None, "mp_layer v', windows")
        for j, (h, _) in enumerate(heads):
            y = v_out[nodes]
            R.assert_as_accurate_as_fp32(h[nodes], R.heads(y, upd.heads)[j], R.heads(y, upd.heads, F32)[j], None, f"mp_layer head{j}, windows")
        # (b)
        for lo, hi in slabs(m):
            a, b = lo // k, hi // k
            he = [torch.empty((b - a, H), device=DEV) for _ in range(2)]
            eo, vo, _ = ops.mp_layer_forward(pm, srcs(lo, hi), hi - lo, uniform_csr(b - a, k), True, pu, v[a:b], ACT["selu"], head_outs=he, v_bound=bound)
            assert int(lib.g4c_mlp_last_kernel()) == expect
            same_bits(e_out[lo:hi], eo, f"mp_layer e' rows {lo} ..")
            same_bits(v_out[a:b], vo, f"mp_layer v' nodes {a} ..")
            for (h, _), got in zip(heads, he):
                same_bits(h[a:b], got, f"mp_layer heads nodes {a} ..")


# ====================================================================== training helpers (csrc/train_ops.hip)
from graphs4cfd_amd import autograd as AG               # noqa: E402
from oracle import grad_ref as G                         # noqa: E402


@pytest.mark.parametrize("v4", [True, False], ids=["v4", "v1"])
def test_train_gather_tall(v4):
    """dst = -a (negated, written), then dst += b (accumulated): both vector widths — 128 aligned columns, or 127 columns from column 1
    (the V = 1 kernel) — direct over M_TALL rows; then 4099 rows gathered from window rows of the tall source."""
    RAN.append(f"train_gather_kernel<{4 if v4 else 1}>")
    c0, width = (0, H) if v4 else (1, H - 1)
    a, b = tall(M_TALL, H, 161, "int"), tall(M_TALL, H, 162, "int")
    whole_view, arena = out_arena(M_TALL)
    view = whole_view[:, c0:c0 + width]
    AG.train_gather(a, whole_view, c0, c0, width, None, _lib.ACT_NONE, True, M_TALL, False)
    FP.assert_footprint_chunked(arena, view, what="train_gather")
    _, wrows = windows()
    aw, bw = rows_of(161, wrows, kind="int"), rows_of(162, wrows, kind="int")
    G.assert_exact(view[wrows], G.gather(aw, None, c0, width, None, True), "train_gather written, windows")
    for lo, hi in slabs(M_TALL):
        tmp = torch.zeros((hi - lo, H), device=DEV)
        AG.train_gather(a[lo:hi], tmp, c0, c0, width, None, _lib.ACT_NONE, True, hi - lo, False)
        same_bits(view[lo:hi], tmp[:, c0:c0 + width], f"train_gather rows {lo} ..")
    AG.train_gather(b, whole_view, c0, c0, width, None, _lib.ACT_NONE, False, M_TALL, True)
    FP.assert_footprint_chunked(arena, view, what="train_gather accumulated")
    G.assert_exact(view[wrows], G.gather(bw, None, c0, width, None, False, -aw[:, c0:c0 + width], 0, True), "train_gather accumulated, windows")
    for lo, hi in slabs(M_TALL):
        tmp = torch.zeros((hi - lo, H), device=DEV)
        AG.train_gather(a[lo:hi], tmp, c0, c0, width, None, _lib.ACT_NONE, True, hi - lo, False)
        AG.train_gather(b[lo:hi], tmp, c0, c0, width, None, _lib.ACT_NONE, False, hi - lo, True)
        same_bits(view[lo:hi], tmp[:, c0:c0 + width], f"train_gather accumulated rows {lo} ..")
    still_holds(a, 161, "int", "train_gather a"); still_holds(b, 162, "int", "train_gather b")
    idx = window_index(4099, wrows, 163)
    dst = torch.zeros((4099, H), device=DEV)
    AG.train_gather(a, dst, c0, c0, width, idx.to(I32), _lib.ACT_NONE, False, 4099, False)
    G.assert_exact(dst[:, c0:c0 + width], G.gather(rows_of(161, idx, kind="int"), None, c0, width), "train_gather gathered")


@pytest.mark.parametrize("ref16", [False, True], ids=["ref32", "ref16"])
def test_act_grad_tall(ref16):
    RAN.append("act_grad_kernel<4, %s>" % ("bf16" if ref16 else "float"))
    dt = torch.bfloat16 if ref16 else F32
    dy, ref = tall(M_TALL, H, 171), tall(M_TALL, H, 172, dtype=dt)
    view, arena = out_arena(M_TALL)
    AG.act_grad(dy, ref, ACT["selu"], False, out=view)
    FP.assert_footprint_chunked(arena, view, what="act_grad")
    still_holds(dy, 171, what="act_grad dy"); still_holds(ref, 172, what="act_grad ref")
    _, wrows = windows()
    want, absw = G.act_grad(rows_of(171, wrows), rows_of(172, wrows, dtype=dt).float(), "selu", False)
    G.assert_fp32_class(view[wrows], want, absw, G.N_EFF_ACT, "act_grad, windows")
    for lo, hi in slabs(M_TALL):
        same_bits(view[lo:hi], AG.act_grad(dy[lo:hi], ref[lo:hi], ACT["selu"], False), f"act_grad rows {lo} ..")


def _fp64_chunks(n, fn):
    """Sum over row chunks of fn(lo, hi) (fp64 tensors on the device)."""
    total = None
    for lo in range(0, n, 1 << 20):
        part = fn(lo, min(lo + (1 << 20), n))
        total = part if total is None else total + part
    return total


@pytest.mark.parametrize("z16", [False, True], ids=["z32", "z16"])
def test_layernorm_grad_tall(z16):
    """dz row by row (windows against fp64, slabs bit for bit); dgamma / dbeta are sums over all rows whose association depends on
    where a row falls in the grid-stride loop (train_ops.hip:121, `r += gridDim.x * 4`), so instead of (b) they are held to the fp64
    sums over row chunks under the small suite's bound — and dbeta, the sum of an integer-valued dy, bit for bit."""
    RAN.append("layernorm_grad_kernel<%s>" % ("bf16" if z16 else "float"))
    dt = torch.bfloat16 if z16 else F32
    z, dy = tall(M_TALL, H, 181, dtype=dt), tall(M_TALL, H, 182, "int")
    gamma = (1 + 0.3 * torch.randn(H, generator=torch.Generator().manual_seed(183))).to(DEV)
    dz, dg, db = AG.layernorm_grad(z, gamma, dy, G.LN_EPS)
    still_holds(z, 181, what="layernorm_grad z"); still_holds(dy, 182, "int", "layernorm_grad dy")
    _, wrows = windows()
    (rz, _, _), (az, _, _) = G.layernorm_grad(rows_of(181, wrows, dtype=dt).float(), gamma, rows_of(182, wrows, kind="int"))
    G.assert_fp32_class(dz[wrows], rz, az, G.N_EFF_LN_ROW, "LN dz, windows")
    for lo, hi in slabs(M_TALL):
        same_bits(dz[lo:hi], AG.layernorm_grad(z[lo:hi], gamma, dy[lo:hi], G.LN_EPS)[0], f"LN dz rows {lo} ..")
    del dz

    def sums(lo, hi):
        (_, g, b), (_, ga, ba) = G.layernorm_grad(z[lo:hi].float(), gamma, dy[lo:hi])
        return torch.stack([g, b, ga, ba])
    rg, rb, ag, ab = _fp64_chunks(M_TALL, sums)
    nwg = int(_lib.load().g4c_layernorm_grad_partials(M_TALL))
    n_col = -(-M_TALL // (4 * nwg)) + 2 + G.n_eff_colsum(nwg, 2 * H) + G.N_EFF_LN_ROW          # (test_gpu_train_ref.test_layernorm_grad_bounded)
    G.assert_fp32_class(dg, rg, ag, n_col, "LN dgamma, all rows")
    G.assert_fp32_class(db, rb, ab, n_col, "LN dbeta, all rows")
    # At 1.7e7 rows that bound exceeds the sums themselves.  What has teeth: dy is integer-valued (|v| <= 8), so dbeta = sum of dy is exact
    # in fp32 in any association — one misread row of dy changes it — and dz, checked above, pins the loads of z; dgamma is accumulated
    # from the same two loads of the row (train_ops.hip:126-127, 151-152).
    G.assert_exact(db, rb, "LN dbeta is the exact sum of the integer dy")


def test_colsum_tall():
    """Integer rows: every partial sum the kernel forms is an integer far below 2^24 (at most 2^24 terms of magnitude <= 8 with random
    signs: a random walk of some 2e4), so the fp32 sums are exact in any order — bit equality with the fp64 sums over row chunks, and
    the sum of the slabs' column sums equals the tall launch's."""
    RAN.append("colsum_stage_kernel")
    x = tall(M_TALL, H, 191, "int")
    got = AG.colsum(x)
    still_holds(x, 191, "int", "colsum")
    G.assert_exact(got, _fp64_chunks(M_TALL, lambda lo, hi: x[lo:hi].double().sum(0)), "colsum, all rows")
    parts = sum(AG.colsum(x[lo:hi]).double() for lo, hi in slabs(M_TALL))
    G.assert_exact(got, parts, "colsum against its slabs")
    # sensitivity: rows a wrapped offset would read instead change the sums
    assert not torch.equal(got.double(), _fp64_chunks(M_TALL - 2 ** 22, lambda lo, hi: x[lo:hi].double().sum(0)))


@pytest.mark.parametrize("form", ["fp32", "bf16", "bf16_a16"])
def test_weight_grad_tall(form):
    """dW = g^T a and db over M_TALL rows, the three launches (g4c_weight_grad, _bf16, _bf16_a16) on integer rows (exact in bf16 too;
    exact sums by the argument of test_colsum_tall, |g a| <= 64): bit equality with the fp64 sums over row chunks on the device."""
    RAN.append({"fp32": "weight_grad_kernel", "bf16": "weight_grad_bf16_kernel<float>", "bf16_a16": "weight_grad_bf16_kernel<bf16>"}[form])
    g, a = tall(M_TALL, H, 201, "int"), tall(M_TALL, H, 202, "int", torch.bfloat16 if form == "bf16_a16" else F32)
    old, old_saved = ops.train_precision(), ops.saved_precision()
    ops.set_train_precision("bf16x6" if form == "fp32" else "bf16")
    try:
        dW, db = AG.weight_bias_grad(g, a, True)
        parts = [AG.weight_bias_grad(g[lo:hi], a[lo:hi], True) for lo, hi in slabs(M_TALL)]
    finally:
        ops.set_train_precision(old, old_saved)
    still_holds(g, 201, "int", "weight_grad g"); still_holds(a, 202, "int", "weight_grad a")
    G.assert_exact(dW, _fp64_chunks(M_TALL, lambda lo, hi: g[lo:hi].double().t() @ a[lo:hi].double()), f"dW {form}, all rows")
    G.assert_exact(db, _fp64_chunks(M_TALL, lambda lo, hi: g[lo:hi].double().sum(0)), f"db {form}, all rows")
    G.assert_exact(dW, sum(p[0].double() for p in parts), f"dW {form} against its slabs")
    G.assert_exact(db, sum(p[1].double() for p in parts), f"db {form} against its slabs")


def test_segment_broadcast_tall():
    """The adjoint of segment_reduce: (1) rows in plan order — dsrc is tall (M_TALL rows), dout has a fifth as many rows; (2) 150
    segments whose permutation names distinct window rows of a tall dsrc: every other row stays zero."""
    RAN.append("segment_broadcast_kernel")
    off = seg_offsets(M_TALL)
    csr = csr_from(off)
    dout = tall(csr.n_seg, H, 211)
    with FP.frozen(dout, what="segment_broadcast"):
        dsrc = {mean: AG.segment_broadcast(dout, csr, mean, M_TALL) for mean in (False, True)}
    wins, _ = windows()
    for lo, hi in wins:
        s0 = int(torch.searchsorted(off, torch.tensor(lo), right=True)) - 1
        s1 = min(int(torch.searchsorted(off, torch.tensor(hi - 1), right=True)), csr.n_seg)
        local = (off[s0:s1 + 1] - off[s0]).to(DEV)
        r0, r1 = int(off[s0]), int(off[s1])
        for mean in (False, True):
            want = G.segment_broadcast(dout[s0:s1], local, None, r1 - r0, mean)
            G.assert_exact(dsrc[mean][r0:r1], want, f"segment_broadcast mean={mean}, rows {r0} .. {r1}")
    per = 640 * (SLAB // (51 * 64))
    for s0, s1 in slabs(csr.n_seg, per):
        r0, r1 = int(off[s0]), int(off[s1])
        part = csr_from(off[s0:s1 + 1] - off[s0])
        for mean in (False, True):
            same_bits(dsrc[mean][r0:r1], AG.segment_broadcast(dout[s0:s1], part, mean, r1 - r0), f"segment_broadcast mean={mean} segments {s0} ..")
    del dsrc
    _, wrows = windows()
    soff = K.offsets(K.seg_lengths(150)).long()
    perm = wrows[torch.randperm(int(wrows.numel()), generator=torch.Generator().manual_seed(212))[: int(soff[-1])].to(DEV)]
    assert int(perm.numel()) == int(soff[-1])          # (distinct rows: the segments of a plan are disjoint)
    small = tall(150, H, 213)
    got = AG.segment_broadcast(small, csr_from(soff, perm.to(I32)), True, M_TALL)
    compact = G.segment_broadcast(small, soff.to(DEV), None, int(soff[-1]), True)
    G.assert_exact(got[perm], compact, "segment_broadcast through perm")
    touched = torch.zeros(M_TALL, dtype=torch.bool, device=DEV)
    touched[perm] = True
    for lo in range(0, M_TALL, 1 << 20):
        blk = got[lo:lo + (1 << 20)]
        assert bool((blk[~touched[lo:lo + (1 << 20)]].view(I32) == 0).all()), f"segment_broadcast: a row no segment owns is not +0, rows {lo} .."


# ====================================================================== plane-major accumulators: g4c_rollout_moments
import moments_ref as MR                                 # noqa: E402


def test_rollout_moments_tall_planes():
    """Eight fields on 2^24 + 37 nodes: sum2 has 36 planes of 134 MB — element 2^28 (2^31 bytes) lies in plane 15, element 2^29 (2^32
    bytes) in plane 31.  Two steps (the first initialises, the second accumulates): (a) every plane on the node windows — the first
    256 nodes, the last 293, 256 nodes on either side of the two boundary elements' nodes — bit for bit against moments_ref; (b) the
    whole state bit for bit against the launch on node slabs (the planes of a slab are compact: at most 2^21 nodes each)."""
    RAN.append("rollout_moments_kernel<8>")
    nf, n, steps = 8, 2 ** 24 + 37, 4
    npair = ops.moment_pairs(nf)
    assert 15 * n < 2 ** 28 < 16 * n and 31 * n < 2 ** 29 < 32 * n and npair * n * 8 > 2 ** 32 + 4096 * 8
    names, planes = MR.NAMES, (nf, nf, npair, nf, nf)
    state = [FP.fill(torch.empty((p, n), dtype=F64, device=DEV)) for p in planes]
    window = torch.tensor([0, -1], dtype=I32, device=DEV)
    preds = [tall(n, nf, 221 + t) for t in range(2)]
    for t in range(2):
        step = torch.tensor([t, 0], dtype=I32, device=DEV)
        with FP.frozen(preds[t], step, what="rollout_moments"):
            ops.rollout_moments(preds[t], step, nf, steps, window, *state)
    assert window.tolist() == [0, 1]
    nodes = T.window_rows(T.windows(n, [2 ** 28 % n, 2 ** 29 % n], tail=37), DEV)
    ref = MR.new_state(int(nodes.numel()), nf)
    for t in range(2):
        ref = MR.accumulate(ref, rows_of(221 + t, nodes, nf).cpu().numpy(), t, steps)
    for name, got in zip(names, state):
        MR.same(got[:, nodes], ref[name], f"rollout_moments {name}, node windows")
    for lo, hi in slabs(n, 2 ** 21):
        part = [torch.empty((p, hi - lo), dtype=F64, device=DEV) for p in planes]
        w2 = torch.tensor([0, -1], dtype=I32, device=DEV)
        for t in range(2):
            ops.rollout_moments(preds[t][lo:hi], torch.tensor([t, 0], dtype=I32, device=DEV), nf, steps, w2, *part)
        for name, got, sl in zip(names, state, part):
            for p in range(int(got.size(0))):
                assert FP.equal_bits_chunked(got[p, lo:hi], sl[p]) is None, f"rollout_moments {name} plane {p}, nodes {lo} .. {hi}"


# ====================================================================== plane-major accumulators: g4c_rollout_spectrum
import spectrum_ref as SR                                # noqa: E402


def test_rollout_spectrum_tall_planes():
    """Eight fields x 64 bins (the most the launch takes) on 2^20 + 37 nodes: re and im have 512 planes of 8 MB each — element 2^28 (2^31
    bytes) lies in plane 255, element 2^29 (2^32 bytes) in plane 511, the last.  Two samples (the first initialises, the second accumulates): (a) every plane on the node
    windows bit for bit against spectrum_ref; (b) the whole state bit for bit against the launch on node slabs of 2^18 nodes."""
    RAN.append("rollout_spectrum_kernel")
    nf, K, n, steps, samples = 8, 64, 2 ** 20 + 37, 4, 128
    assert 255 * n < 2 ** 28 < 256 * n and 511 * n < 2 ** 29 < 512 * n and nf * K * n * 8 > 2 ** 32 + 4096 * 8
    tw_host, _, _ = ops.spectrum_table(bins=list(range(K)), samples=samples)
    tw = tw_host.to(DEV)
    names, planes = SR.NAMES, (nf, nf, nf * K, nf * K)
    state = [FP.fill(torch.empty((p, n), dtype=F64, device=DEV)) for p in planes]
    window = torch.tensor([0, -1], dtype=I32, device=DEV)
    xs = [tall(n, nf, 231 + t) for t in range(2)]
    for t in range(2):
        step = torch.tensor([t, 0], dtype=I32, device=DEV)
        with FP.frozen(xs[t], step, tw, what="rollout_spectrum"):
            ops.rollout_spectrum(xs[t], step, nf, steps, window, tw, *state)
    assert window.tolist() == [0, 1]
    nodes = T.window_rows(T.windows(n, [2 ** 28 % n, 2 ** 29 % n], tail=37), DEV)
    ref = SR.new_state(int(nodes.numel()), nf, K)
    for t in range(2):
        ref = SR.accumulate(ref, rows_of(231 + t, nodes, nf).cpu().numpy(), t, steps, tw_host.numpy())
    for name, got in zip(names, state):
        SR.same(got[:, nodes], ref[name], f"rollout_spectrum {name}, node windows")
    for lo, hi in slabs(n, 2 ** 18):
        part = [torch.empty((p, hi - lo), dtype=F64, device=DEV) for p in planes]
        w2 = torch.tensor([0, -1], dtype=I32, device=DEV)
        for t in range(2):
            ops.rollout_spectrum(xs[t][lo:hi], torch.tensor([t, 0], dtype=I32, device=DEV), nf, steps, w2, tw, *part)
        for name, got, sl in zip(names, state, part):
            assert FP.equal_bits_chunked(got[:, lo:hi], sl) is None, f"rollout_spectrum {name}, nodes {lo} .. {hi}"


# ====================================================================== snapshot launches (csrc/snapshot_modes.hip)
import modes_ref as MO                                   # noqa: E402


def test_snapshot_mean_gram_combine_tall():
    """A snapshot matrix [700, 2^20, 3] (8.8 GB): snapshot 170 crosses 2^31 bytes, 341 crosses 2^32 bytes, 682 crosses 2^31 elements.
    Integer snapshots and integer coefficients: every sum is exact in fp64 in any order, so each launch is compared bit for bit with
    plain fp64 torch sums over column chunks on the device (all columns), with modes_ref on the column windows around each boundary
    (mean, combine), and with the launch on compact column slabs.  snapshot_combine with 700 combinations also WRITES a tall tensor."""
    RAN.append("snapshot_mean_kernel, snapshot_gram kernels, snapshot_combine_kernel")
    m, n, nf = 700, 2 ** 20, 3
    L = n * nf
    x = torch.empty((m, n, nf), device=DEV)
    T.fill_(x.view(m * L // H, H), 241, "int")
    flat = x.view(m, L)
    coef = T.value(242, torch.arange(m), m, "int").double().to(DEV)
    mean, G, comb = ops.snapshot_mean(x), ops.snapshot_gram(x), ops.snapshot_combine(x, coef)
    still_holds(x.view(m * L // H, H), 241, "int", "snapshots")
    assert torch.equal(G, G.t())
    # every column, fp64 sums over column chunks (exact)
    g_ref = torch.zeros((m, m), dtype=F64, device=DEV)
    step = 2 ** 17
    for c0 in range(0, L, step):
        xc = flat[:, c0:c0 + step].double()
        g_ref += xc @ xc.t()
        # (a tensor divisor: torch divides by a Python scalar on the device as a product with its reciprocal)
        assert torch.equal(mean[c0:c0 + step], xc.sum(0) / torch.full((1,), float(m), dtype=F64, device=DEV)), f"snapshot_mean, columns {c0} .."
        assert torch.equal(comb[:, c0:c0 + step], (coef.t() @ xc).float()), f"snapshot_combine, columns {c0} .."
    assert torch.equal(G, g_ref), "snapshot_gram"
    # modes_ref on the windows: the columns around the element where each boundary falls, the first and the last
    cols = T.window_rows(T.windows(L, sorted({2 ** 29 % L, 2 ** 30 % L, 2 ** 31 % L}), margin=64), DEV)
    xw = T.value_at(241, torch.arange(m, device=DEV)[:, None] * L + cols[None, :], H, "int").cpu().numpy()
    MO.same_bits(mean[cols], MO.mean(xw), "snapshot_mean, column windows")
    MO.same_bits(comb[:8][:, cols], MO.combine(xw, coef[:, :8].cpu().numpy()), "snapshot_combine, column windows")
    del comb
    # compact column slabs (under 2^30 bytes each)
    per = 2 ** 30 // (4 * m) // 64 * 64
    g_sum = torch.zeros((m, m), dtype=F64, device=DEV)
    for c0, c1 in slabs(L, per):
        part = flat[:, c0:c1].contiguous()
        assert torch.equal(mean[c0:c1], ops.snapshot_mean(part)), f"snapshot_mean slab {c0}"
        g_sum += ops.snapshot_gram(part)
    assert torch.equal(G, g_sum), "snapshot_gram against the sum of its column slabs"


# ====================================================================== the row-split kernels of the rounded-bf16 mode (csrc/mlp_rs.hip)
import test_gpu_bf16 as BF                               # noqa: E402
from graphs4cfd_amd.nn import blocks as B                # noqa: E402
from oracle import bf16_ref as RB                        # noqa: E402


def bf16_noise_on_device(got, ref, kind, what):
    """oracle.bf16_ref.check_bf16_order_noise — the same statistics against the same limits — evaluated where the tensors are (the
    aggregate of 2.8 million segments, slab by slab, without a trip to the host)."""
    m, thr, f, mx, _, rc = RB.NOISE[kind]
    assert tuple(got.shape) == tuple(ref.shape) and bool(torch.isfinite(got).all()), what
    d = (got.double() - ref.double()).abs()
    stats = {"mean": float(d.mean()), "frac": float((d > thr).double().mean()), "max": float(d.max()),
             "row_count": int((d > RB.row_threshold(kind)).sum(1).max())}
    lim = {"mean": RB.MEAN_X * m + RB.FLIP_ROWS * mx / int(got.size(0)), "frac": RB.FRAC_X * f + RB.FRAC_FLOOR + 2.0 / d.numel(),
           "max": RB.MAX_X * mx, "row_count": rc}
    assert all(stats[key] <= lim[key] for key in lim), f"{what} [{kind}]: {stats} against limits {lim}"


def test_mlp_rs1_kernel_tall():
    """mlp_rs1_kernel through MLP.run_hoisted, degree 6: tall fp32 e rows (halved: |v| < 1.5, near the N(0, 1) rows the noise bounds
    of oracle/bf16_ref.py were derived on), products of two node tensors through indices, fp32 rows and — a second launch — compact
    bf16(SELU) rows (tall bf16: boundaries at rows 2^23 and 2^24), the fused mean.  (a) windows of whole segments under
    `assert_bf16_order_noise`; (b) the rows bit for bit against slabs.  The aggregate's bits depend on where a wave's 16-row chunks cut
    a segment (mlp_rs.hip:337, `y = fmaf(carry, mc, y)`: the partial sum carried from the previous chunk), so the tall
    launch's aggregate is held, slab by slab, to the fp64 mean of the launch's own rows under the "agg32" bound instead."""
    RAN.append("mlp_rs1_kernel")
    k = 6
    E = M_TALL - M_TALL % k
    n = E // k
    torch.manual_seed(251)
    with BF.bf16_mode():
        assert B.ROW_SPLIT_BF16
        m = B.GNBlock((3 * H, (H, H, H), True), (2 * H, (H, H, H), True)).to(DEV).edge_mlp
        with torch.no_grad():
            m.MLP.layer_norm.weight.copy_(1.0 + 0.1 * torch.randn(H, device=DEV))
            m.MLP.layer_norm.bias.copy_(0.1 * torch.randn(H, device=DEV))
        w = BF.sd(m)
        W1 = w["MLP.linear_1.weight"]
        a32 = tall(E, H, 252).mul_(0.5)
        s, r = tall(n, H, 253).mul_(0.5), tall(n, H, 254).mul_(0.5)
        row, col = (torch.randint(0, n, (E,), generator=torch.Generator().manual_seed(255 + j)).to(DEV, I32) for j in range(2))
        csr = uniform_csr(n, k)

        def launch(lo, hi, **kw):
            part = csr if (lo, hi) == (0, E) else uniform_csr((hi - lo) // k, k)
            agg = torch.full((part.n_seg, H), float("nan"), device=DEV)
            y = m.run_hoisted([ops.Source(a32[lo:hi], pre_act=BF.SELU)], [(s, row[lo:hi]), (r, col[lo:hi])], hi - lo, agg=(part, agg, True), **kw)
            assert BF.last_kernel() == BF.RS1
            return y, agg
        wins = [(lo - lo % k, min(hi + (-hi) % k, E)) for lo, hi in T.tall_windows(E, tail=E % 64)]
        wrows = T.window_rows(wins, DEV)
        nw, ar = int(wrows.numel()), torch.arange(int(wrows.numel()))
        adds = [RB.Additive(RB.products(W1[:, H:2 * H], s[row[wrows].long()]), ar), RB.Additive(RB.products(W1[:, 2 * H:], r[col[wrows].long()]), ar)]
        ref = RB.mlp(w, [RB.Block(rows_of(252, wrows) * 0.5, pre_act="selu")], nw, additive=adds, first_cols=(0, H))
        woff = torch.arange(0, nw + 1, k)
        segs = torch.cat([torch.arange(lo // k, hi // k) for lo, hi in wins]).to(DEV)
        for fmt, kw in (("fp32", {}), ("bf16_selu", dict(rows_dtype=torch.bfloat16, rows_act=BF.SELU))):
            y, agg = launch(0, E, **kw)
            assert y.dtype == (F32 if fmt == "fp32" else torch.bfloat16) and isinstance(y, ops.RsOrderedRows) == (fmt != "fp32")
            yw = y.as_subclass(torch.Tensor)[wrows]
            if fmt != "fp32":          # (compact rows are in the row-split column order)
                yw = yw[:, torch.argsort(ops._rs_k_order(DEV))]
            BF.check(yw, RB.stored_rows(ref, fmt), "rows32" if fmt == "fp32" else "rows16", f"rs1 tall {fmt} rows, windows")
            BF.check(agg[segs], RB.segment_mean(ref, woff), "agg32", f"rs1 tall {fmt} aggregate, windows")
            for lo, hi in slabs(E):
                ys, aggs = launch(lo, hi, **kw)
                same_bits(y[lo:hi], ys, f"rs1 {fmt} rows {lo} ..")
                if fmt == "fp32":
                    own = ys.double().view(-1, k, H).sum(1) / k
                    bf16_noise_on_device(agg[lo // k:hi // k], own, "agg32", f"rs1 tall aggregate of rows {lo} .. against the launch's own rows")
            del y, agg
        still_holds(a32.mul_(2.0), 252, what="rs1 e")


def test_mlp_rs2_kernel_tall():
    """mlp_rs2_kernel: [bf16 aggregate in the row-split order | bf16 e in feature order] -> 256 -> 128 -> 128 -> LayerNorm -> SELU over
    M_TALL rows, fp32 output rows and both bf16 product heads (row-split order): windows under `assert_bf16_order_noise`, slabs bit
    for bit.  (bf16 rows: 2^31 bytes at row 2^23, 2^32 bytes at row 2^24.)"""
    RAN.append("mlp_rs2_kernel")
    n = M_TALL
    node, nxt = BF.make_mlp(2 * H, 2, True, 261), BF.make_mlp(3 * H, 2, True, 262)
    wn, W1 = BF.sd(node), BF.sd(nxt)["MLP.linear_1.weight"]
    order = ops._rs_k_order(DEV)
    agg = ops.RsOrderedRows.tag(tall(n, H, 263, dtype=torch.bfloat16))          # (these ARE the rows in the row-split order)
    e = tall(n, H, 264, dtype=torch.bfloat16)
    out = torch.empty((n, H), device=DEV)
    with BF.bf16_mode():
        assert B.UPDATE_ROW_SPLIT
        y, hs = node.run_with_heads([ops.Source(agg), ops.Source(e)], n, BF.SELU, nxt, H, [H, H], out=out, rs_rows=True)
        assert BF.last_kernel() == BF.RS2 and all(isinstance(h, ops.RsOrderedRows) and h.dtype == torch.bfloat16 for h in hs)
        _, wrows = windows(tail=n % 16)
        natural = torch.empty_like(order)
        natural[order] = torch.arange(H, device=DEV)          # feature f sits in column natural[f] of a row-split row
        agg_w = rows_of(263, wrows, dtype=torch.bfloat16)[:, natural]
        y_ref = RB.mlp(wn, [RB.Block(agg_w), RB.Block(rows_of(264, wrows, dtype=torch.bfloat16))], int(wrows.numel()), act="selu")
        BF.check(y[wrows], y_ref, "rows32", "rs2 tall rows, windows")
        for j, h in enumerate(hs):
            got = h.as_subclass(torch.Tensor)[wrows][:, natural]
            BF.check(got, RB.products(W1[:, H * (j + 1):H * (j + 2)], y_ref), "prod16", f"rs2 tall head {j}, windows")
        for lo, hi in slabs(n):
            ys, hss = node.run_with_heads([ops.Source(ops.RsOrderedRows.tag(agg.as_subclass(torch.Tensor)[lo:hi])), ops.Source(e[lo:hi])], hi - lo,
                                          BF.SELU, nxt, H, [H, H], rs_rows=True)
            assert BF.last_kernel() == BF.RS2
            same_bits(y[lo:hi], ys, f"rs2 rows {lo} ..")
            for h, h2 in zip(hs, hss):
                same_bits(h.as_subclass(torch.Tensor)[lo:hi], h2.as_subclass(torch.Tensor), f"rs2 heads rows {lo} ..")
    still_holds(agg.as_subclass(torch.Tensor), 263, what="rs2 aggregate"); still_holds(e, 264, what="rs2 e")


# ====================================================================== bf16 rows on the tile and weight-stationary kernels (rounded-bf16 mode)
BF16 = torch.bfloat16


def _state_dict_of(nt):
    """A test_gpu_fwd_ref.Net as the state dict oracle/bf16_ref.py reads."""
    w = {}
    for i, (W, b) in enumerate(zip(nt.W, nt.b), 1):
        w[f"MLP.linear_{i}.weight"], w[f"MLP.linear_{i}.bias"] = W.cpu(), b.cpu()
    w["MLP.layer_norm.weight"], w["MLP.layer_norm.bias"] = nt.ln[0].cpu(), nt.ln[1].cpu()
    return w


def test_mlp_tile_kernel_bf16_rows_tall():
    """mlp_bx6_kernel in the rounded-bf16 mode: a tall bf16 source read directly (2^31 bytes at row 2^23, 2^32 bytes at row 2^24) next
    to a gathered fp32 table -> two layers -> LayerNorm -> SELU; first launch: fp32 rows and both heads as tall bf16 rows; second
    launch: the rows themselves stored as bf16.  Windows under `assert_bf16_order_noise`, slabs bit for bit, guard rows."""
    RAN.append("mlp_bx6_kernel (rounded bf16, bf16 rows)")
    n = M_TALL
    nt = _net(2 * H, 2, 311, n_heads=2)
    w = _state_dict_of(nt)
    a16 = tall(n, H, 312, dtype=BF16).mul_(0.5)
    tab = tall(4099, H, 313).mul_(0.5)
    idx = torch.randint(0, 4099, (n,), generator=torch.Generator().manual_seed(314)).to(DEV, I32)
    _, wrows = windows(tail=n % 64)
    with BF.bf16_mode() as lib:
        pk = nt.pack([FR.Blk(a16), FR.Blk(tab)], "bf16", True)
        srcs = lambda lo, hi: [ops.Source(a16[lo:hi]), ops.Source(tab, idx[lo:hi])]          # noqa: E731
        y_ref = RB.mlp(w, [RB.Block(rows_of(312, wrows, dtype=BF16) * 0.5), RB.Block(tab[idx[wrows].long()])], int(wrows.numel()), act="selu")
        view, arena = out_arena(n)
        hv = [out_arena(n, H, BF16) for _ in range(2)]
        _launch(lib, pk, srcs(0, n), n, "selu", FR.K_BX6, "tile bf16 rows", out=view, head_outs=[h[0] for h in hv])
        for v_, w_ in [(view, arena)] + hv:
            FP.assert_footprint_chunked(w_, v_, what="tile bf16 rows")
        BF.check(view[wrows], y_ref, "rows32", "tile tall rows from a bf16 source, windows")
        for j, (h, _) in enumerate(hv):
            BF.check(h[wrows], RB.products(nt.heads[j], y_ref), "prod16", f"tile tall bf16 head {j}, windows")
        for lo, hi in slabs(n):
            tmp = [torch.empty((hi - lo, H), device=DEV)] + [torch.empty((hi - lo, H), dtype=BF16, device=DEV) for _ in range(2)]
            _launch(lib, pk, srcs(lo, hi), hi - lo, "selu", FR.K_BX6, f"tile bf16 rows {lo} ..", out=tmp[0], head_outs=tmp[1:])
            for got, (full, _) in zip(tmp, [(view, arena)] + hv):
                same_bits(full[lo:hi], got, f"tile bf16 rows {lo} ..")
        del view, arena, hv, tmp, got, full, h
        view, arena = out_arena(n, H, BF16)
        _launch(lib, pk, srcs(0, n), n, "selu", FR.K_BX6, "tile bf16 output rows", out=view)
        FP.assert_footprint_chunked(arena, view, what="tile bf16 output rows")
        BF.check(view[wrows], RB.stored_rows(y_ref, "bf16"), "rows16", "tile tall bf16 output rows, windows")
        for lo, hi in slabs(n):
            got = torch.empty((hi - lo, H), dtype=BF16, device=DEV)
            _launch(lib, pk, srcs(lo, hi), hi - lo, "selu", FR.K_BX6, f"tile bf16 output rows {lo} ..", out=got)
            same_bits(view[lo:hi], got, f"tile bf16 output rows {lo} ..")
    still_holds(a16.mul_(2.0), 312, what="tile bf16 source")


def test_mlp_ws_kernel_bf16_rows_tall():
    """mlp_ws_kernel in the rounded-bf16 mode (SP = 1): a tall bf16 source read directly, two bf16 product tables through indices, the
    fused mean of degree 6, the rows stored as tall bf16 rows.  Windows of whole segments under `assert_bf16_order_noise`; rows and
    aggregate bit for bit against slabs of whole segments."""
    RAN.append("mlp_ws_kernel (rounded bf16, bf16 rows)")
    k = 6
    m = M_TALL - M_TALL % k
    nt = _net(H, 3, 321)
    w = _state_dict_of(nt)
    e16 = tall(m, H, 322, dtype=BF16).mul_(0.5)
    tabs = [tall(4099, H, 323 + j, dtype=BF16).mul_(0.5) for j in range(2)]
    idx = [torch.randint(0, 4099, (m,), generator=torch.Generator().manual_seed(325 + j)).to(DEV, I32) for j in range(2)]
    av, aarena = out_arena(m // k)
    with BF.bf16_mode(ws=2) as lib:
        pk = nt.pack([FR.Blk(e16), FR.Blk(tabs[0], additive=True), FR.Blk(tabs[1], additive=True)], "bf16")

        def run(lo, hi, agg_out):
            srcs = [ops.Source(e16[lo:hi])] + [ops.Source(t, i[lo:hi], additive=True) for t, i in zip(tabs, idx)]
            y = _launch(lib, pk, srcs, hi - lo, None, FR.K_WS, f"ws bf16 rows {lo} ..", agg=(uniform_csr((hi - lo) // k, k), agg_out, True),
                        rows_dtype=BF16)
            assert y.dtype == BF16
            return y
        y = run(0, m, av)
        FP.assert_footprint_chunked(aarena, av, what="ws bf16 aggregate")
        wins = [(lo - lo % k, min(hi + (-hi) % k, m)) for lo, hi in T.tall_windows(m, tail=m % 64)]
        wrows = T.window_rows(wins, DEV)
        nw = int(wrows.numel())
        ref = RB.mlp(w, [RB.Block(rows_of(322, wrows, dtype=BF16) * 0.5)], nw,
                     additive=[RB.Additive(t[i[wrows].long()].float()) for t, i in zip(tabs, idx)])
        BF.check(y[wrows], RB.stored_rows(ref, "bf16"), "rows16", "ws tall bf16 rows, windows")
        segs = torch.cat([torch.arange(lo // k, hi // k) for lo, hi in wins]).to(DEV)
        BF.check(av[segs], RB.segment_mean(ref, torch.arange(0, nw + 1, k)), "agg32", "ws tall aggregate of bf16 rows, windows")
        for lo, hi in slabs(m):
            part = torch.empty(((hi - lo) // k, H), device=DEV)
            same_bits(y[lo:hi], run(lo, hi, part), f"ws bf16 rows {lo} ..")
            same_bits(av[lo // k:hi // k], part, f"ws aggregate of bf16 rows {lo} ..")
    still_holds(e16.mul_(2.0), 322, what="ws bf16 source")


# ====================================================================== one whole model: plans, int32 index tensors between the launches
import graphs4cfd_amd as gfd                             # noqa: E402
from graphs4cfd_amd import synthetic as S                # noqa: E402
from oracle import g4c_oracle as O                       # noqa: E402
from test_gpu_parity import FWD                          # noqa: E402  (the full-forward tolerance of this model class against the oracle)


def _block_diagonal(g0, fields):
    """B copies of the four-level graph g0 as ONE graph — the same topology, copy c's nodes, clusters and coarse nodes behind copy
    c - 1's on every level, `field` from `fields[c]`: node tensors concatenated, `edge_index` offset by the node count, the
    fine-to-coarse maps by the coarse node count, the voxel ids of `cluster_l` / `mask_l` by a stride above the largest id."""
    B, out = int(fields.size(0)), {}
    n = {1: g0.num_nodes, **{lvl: int(getattr(g0, f"mask_{lvl}").numel()) for lvl in (2, 3, 4)}}
    for key, v in g0.__dict__.items():
        if not torch.is_tensor(v):
            out[key] = v
        elif key == "field":
            out[key] = fields.reshape(-1, int(fields.size(-1)))
        elif key == "edge_index":
            out[key] = torch.cat([v + c * n[1] for c in range(B)], 1)
        elif key.startswith("idx"):          # idx{h}_to_idx{l}
            lvl = int(key[-1])
            out[key] = torch.cat([v + c * n[lvl] for c in range(B)])
        elif key.startswith("cluster_") or key.startswith("mask_"):
            stride = int(getattr(g0, "cluster_" + key[-1]).max()) + 1
            out[key] = torch.cat([v + c * stride for c in range(B)])
        else:
            out[key] = torch.cat([v] * B, 0)
    return gfd.Graph(**out)


def test_whole_model_forward_on_a_tall_batch():
    """NsFourScaleGNN.forward under f16x3 on 342 block-diagonal copies of a four-level 3-D graph of 4096 nodes (k = 6): 8 404 992
    level-1 edge rows — past 2^23 + 4096, what c5-1gpu reaches and a little more.  The copies differ in `field` alone.  The first
    copy, the copy whose edge rows straddle row 2^22 (170) and the last one, which straddles row 2^23 (341), must agree in the batch
    with their runs as single small graphs, within the tolerance test_gpu_parity.py holds this model class to against the oracle; copy
    170 is also compared with oracle/g4c_oracle.py; and consecutive copies differ, so a wrap onto the neighbouring copy cannot pass."""
    RAN.append("NsFourScaleGNN.forward")
    n, k, B = 4096, 6, 342
    assert B * n * k > 2 ** 23 + 4096 and 170 * n * k < 2 ** 22 < 171 * n * k and 341 * n * k < 2 ** 23 < 342 * n * k
    assert ops.mlp_precision() == "f16x3"
    g0 = S.mus_graph(n, levels=4, k=k, dim=3, seed=331).to(DEV)
    assert int(g0.edge_index.size(1)) == n * k
    fields = torch.randn(B, n, 3, generator=torch.Generator().manual_seed(332)).to(DEV)
    torch.manual_seed(333)
    model = gfd.nn.NsFourScaleGNN(arch=S.mus_arch("NsFourScaleGNN", 128, dim=3), device=DEV)
    batch = _block_diagonal(g0, fields)
    assert batch.num_nodes == B * n and int(batch.edge_index.size(1)) == B * n * k and batch.edge_index.dtype == torch.int64
    y = model.forward(batch).view(B, n, 3)
    assert bool(torch.isfinite(y).all())
    del batch
    for c in (0, 170, B - 1):
        g = g0.clone()
        g.field = fields[c].clone()
        alone = model.forward(g)
        torch.testing.assert_close(y[c], alone, msg=lambda m, c=c: f"copy {c} in the batch against its own run: {m}", **FWD)
        if c == 170:
            gc = g0.clone().to("cpu")
            gc.field = fields[c].cpu()
            ref = O.mus_forward("NsFourScaleGNN", gc.to_dict(), {key: v.cpu() for key, v in model.state_dict().items()}, 3)
            torch.testing.assert_close(y[c].cpu(), ref, **FWD)
            torch.testing.assert_close(alone.cpu(), ref, **FWD)
    gap = (y[1:] - y[:-1]).abs().amax((1, 2))
    assert float(gap.min()) > 100 * FWD["atol"], f"two consecutive copies are {float(gap.min()):.2e} apart: a wrap onto a neighbour would pass"
