"""The memory-bound helper launches (csrc/segment_reduce.hip, csrc/remus_ops.hip) against the plain fp64 references of
oracle/mem_ref.py, called through ops.*, at the shapes and data of tests/mem_cases.py (the smallest that reach each code path).

Exact (`assert_exact`, integer operands, or fp32 data against the kernel's stated rounding): segment sums, the mean as one correctly
rounded fp32 division of the exact sum, the weighted mean with power-of-two weights, project_to_edges (bit-equal to its two-rounding
form on floats), edge_scalar_to_node_vector, copy_cols, add_cols, rollout_advance, the vector and scalar segment kernels on the same
floats.  Bounded (`assert_fp32_class`, C = 2, n_eff derived per kernel in mem_ref.py; the measured / allowed ratio of each is
printed): activations, segment_reduce with activations, the weighted mean with weights spanning 1e16, edge_scalar_to_node_vector,
layer_norm.  Every output buffer is pre-filled with a sentinel: pad columns, rows no index names, columns outside a window and
other steps' slots must still hold it.  One negative control per kernel family: the kernel's own result fails its checker against a
perturbed reference.  The last test hands each wrapper a malformed call: it raises in Python and nothing is written."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

import mem_cases as K                                    # noqa: E402
from graphs4cfd_amd import _lib, ops, plan               # noqa: E402
from oracle import mem_ref as M                          # noqa: E402

DEV = torch.device("cuda", 0)
F32, F64, I32 = torch.float32, torch.float64, torch.int32
ACT = {None: _lib.ACT_NONE, "selu": _lib.ACT_SELU, "tanh": _lib.ACT_TANH}


def dev(t):
    return None if t is None else t.to(DEV)


def sentinel(*shape):
    return torch.full(shape, K.SENT, dtype=F32, device=DEV)


def holds_sentinel(t, what):
    assert bool((t == K.SENT).all()), f"{what}: {int((t != K.SENT).sum())} elements the launch does not own were written"


def window(data, col0, pad):
    """`data` as the columns col0 .. of a wider sentinel-filled device tensor: (the view, the wide tensor)."""
    wide = sentinel(data.size(0), col0 + data.size(1) + pad)
    view = wide[:, col0:col0 + data.size(1)]
    view.copy_(data)
    return view, wide


def pads_untouched(wide, col0, width, what):
    holds_sentinel(wide[:, :col0], what + " (columns left of the window)")
    holds_sentinel(wide[:, col0 + width:], what + " (columns right of the window)")


def csr_of(c):
    return plan.CsrPlan(perm=dev(c["perm"]), off=dev(c["off"]), n=c["n"], n_seg=c["n_seg"], max_deg=c["max_deg"])


# ====================================================================== segment_reduce
def _seg_launch(c, mean, sa=None, a=None, strided=False):
    """The launch's output on the host.  strided: src is a column window of a wider tensor and out= one of a wider sentinel buffer,
    both placed so that a vector width stays on the vector path (16-byte aligned window, leading dimensions multiples of 4)."""
    width = c["src"].size(1)
    vec = width % 4 == 0
    if not strided:
        return ops.segment_reduce(dev(c["src"]), csr_of(c), mean, ACT[a], src_act=ACT[sa]).cpu()
    src, _ = window(c["src"], 4 if vec else 1, 4 if vec else 2)
    out_wide = sentinel(c["n_seg"], width + (4 if vec else 1))
    res = ops.segment_reduce(src, csr_of(c), mean, ACT[a], out=out_wide[:, :width], src_act=ACT[sa])
    assert res.data_ptr() == out_wide.data_ptr()
    pads_untouched(out_wide, 0, width, f"segment_reduce out= w{width}")
    return res.cpu()


@pytest.mark.parametrize("width", K.VEC_WIDTHS + K.SCALAR_WIDTHS)
@pytest.mark.parametrize("n_seg", K.N_SEGS)
def test_segment_reduce_sum_and_mean_are_exact(n_seg, width):
    for perm in K.PERMS:
        c = K.seg_case(n_seg, width, perm, "int")
        ref_sum, absref = M.segment_reduce(c["src"], c["off"], c["perm"], False)
        M.check_int_bound(absref)
        ref_mean = M.segment_mean_fp32(c["src"], c["off"], c["perm"])
        for strided in (False, True):
            what = f"n_seg {n_seg} w{width} perm {perm} strided {strided}"
            M.assert_exact(_seg_launch(c, False, strided=strided), ref_sum, "sum, " + what)
            M.assert_exact(_seg_launch(c, True, strided=strided), ref_mean, "mean, " + what)


def test_segment_reduce_built_plan_equals_hand_built():
    """plan.build_csr (a full permutation) against the same keys grouped by hand."""
    g = K.gen("built", 1)
    keys = torch.randint(0, 33, (700,), generator=g)
    src = M.int_operand((700, 68), 8, g)
    csr = plan.build_csr(keys.to(DEV), 33, DEV)
    perm = torch.argsort(keys, stable=True)
    off = torch.zeros(34, dtype=torch.int64)
    off[1:] = torch.cumsum(torch.bincount(keys, minlength=33), 0)
    assert torch.equal(csr.off.cpu().long(), off) and torch.equal(csr.perm.cpu().long(), perm)
    M.assert_exact(ops.segment_reduce(dev(src), csr, False).cpu(), M.segment_reduce(src, off, perm, False)[0], "built plan")


@pytest.mark.parametrize("width", (128, 6, 260))
def test_segment_reduce_activations_are_bounded(width):
    c = K.seg_case(33, width, "subset", "float")
    for mean in (False, True):
        for sa in K.ACTS:
            for a in K.ACTS:
                got = _seg_launch(c, mean, sa, a, strided=(sa is None) != (a is None))
                ref = M.segment_reduce(c["src"], c["off"], c["perm"], mean, sa, a)
                M.assert_fp32_class(got, *ref, M.n_eff_segment_reduce(c["off"], mean, sa, a), f"segment_reduce w{width} mean={mean} {sa}/{a}")


@pytest.mark.parametrize("n_seg", (33, 1031))
def test_segment_reduce_vector_and_scalar_paths_are_bit_equal(n_seg):
    """Width 128 on the vector path (aligned, contiguous) and on the scalar fallback — a base pointer 4 bytes off 16-byte alignment
    (a [:, 1:129] view) and a leading dimension of 130: the same additions in the same order, the same bits on float inputs."""
    for perm in ("full", "subset"):
        c = K.seg_case(n_seg, 128, perm, "float")
        csr = csr_of(c)
        src = dev(c["src"])
        off4, wide132 = window(c["src"], 1, 3)
        ld130, wide130 = window(c["src"], 0, 2)
        assert src.data_ptr() % 16 == 0 and off4.data_ptr() % 16 == 4 and off4.stride(0) == 132 and ld130.stride(0) == 130
        for mean, sa, a in ((False, None, None), (True, None, None), (True, "selu", "tanh"), (False, "tanh", "selu")):
            vec = ops.segment_reduce(src, csr, mean, ACT[a], src_act=ACT[sa])
            for name, view in (("misaligned base", off4), ("leading dimension 130", ld130)):
                sc = ops.segment_reduce(view, csr, mean, ACT[a], src_act=ACT[sa])
                assert torch.equal(vec, sc), f"{name}: {int((vec != sc).sum())} elements differ (mean={mean} {sa}/{a})"
            ref = M.segment_reduce(c["src"], c["off"], c["perm"], mean, sa, a)
            M.assert_fp32_class(vec.cpu(), *ref, M.n_eff_segment_reduce(c["off"], mean, sa, a), f"vector path n_seg {n_seg} {perm} mean={mean} {sa}/{a}")
        # the scalar fallback into an out= whose own leading dimension is odd
        out_wide = sentinel(n_seg, 131)
        ops.segment_reduce(src, csr, True, out=out_wide[:, 2:130])
        assert torch.equal(out_wide[:, 2:130], ops.segment_reduce(src, csr, True))
        pads_untouched(out_wide, 2, 128, "segment_reduce out= ld 131")


def test_segment_reduce_negative_controls():
    c = K.seg_case(33, 128, "subset", "int")
    src, off, p = c["src"], c["off"], c["perm"]
    s = int(torch.nonzero(M.counts(off) > 1)[-1])
    got_sum, got_mean = _seg_launch(c, False), _seg_launch(c, True)
    for what, src_b, off_b in (("row moved into the next segment", src, M.move_boundary(off, s + 1)),
                               ("last row dropped", M.drop_last_row(src, off, p, s), off)):
        assert M.rejects(M.assert_exact, got_sum, M.segment_reduce(src_b, off_b, p, False)[0], what), what
        assert M.rejects(M.assert_exact, got_mean, M.segment_mean_fp32(src_b, off_b, p), what), what
    c = K.seg_case(33, 128, "subset", "float")
    src, off, p = c["src"], c["off"], c["perm"]
    s = int(torch.nonzero(M.counts(off) == 40)[0])
    got = _seg_launch(c, True, "selu", "tanh")
    n_eff = M.n_eff_segment_reduce(off, True, "selu", "tanh")
    M.assert_fp32_class(got, *M.segment_reduce(src, off, p, True, "selu", "tanh"), n_eff, "segment_reduce, control's own reference")
    assert M.rejects(M.assert_fp32_class, got, *M.segment_reduce(src, M.move_boundary(off, s), p, True, "selu", "tanh"), n_eff, "moved boundary")
    assert M.rejects(M.assert_fp32_class, got, *M.segment_reduce(M.drop_last_row(src, off, p, s - 1), off, p, True, "selu", "tanh"), n_eff, "dropped row")


# ====================================================================== weighted_segment_mean
def _wm_launch(c, strided):
    """(result on the host as the whole [n_out, width] output, reference initial contents)."""
    width = c["x"].size(1)
    csr = plan.CsrPlan(perm=None, off=dev(c["off"]), n=c["n"], n_seg=c["n_seg"], max_deg=c["k"], uniform_deg=c["k"])
    x = window(c["x"], 2, 1)[0] if strided else dev(c["x"])
    init = torch.full((c["n_out"], width), K.SENT)
    if c["out_idx"] is None and not strided:
        out = ops.weighted_segment_mean(x, dev(c["x_idx"]), dev(c["w"]), csr)
        assert tuple(out.shape) == (c["n_seg"], width)
        return out.cpu(), init
    out_wide = sentinel(c["n_out"], width + (3 if strided else 0))
    out = out_wide[:, 1:1 + width] if strided else out_wide
    res = ops.weighted_segment_mean(x, dev(c["x_idx"]), dev(c["w"]), csr, out, dev(c["out_idx"]))
    assert res.data_ptr() == out.data_ptr()
    if strided:
        pads_untouched(out_wide, 1, width, f"weighted_segment_mean out= w{width}")
    return out.cpu(), init


@pytest.mark.parametrize("width", K.WM_WIDTHS)
@pytest.mark.parametrize("k", K.WM_K)
def test_weighted_segment_mean(k, width):
    for n_seg in K.WM_NSEG:
        for scattered in (False, True):
            for strided in (False, True):
                what = f"k{k} w{width} n_seg {n_seg} scattered {scattered} strided {strided}"
                c = K.wm_case(k, width, n_seg, "int", scattered)
                got, init = _wm_launch(c, strided)
                ref, _ = M.weighted_segment_mean(c["x"], c["x_idx"], c["w"], c["off"], c["out_idx"], init)
                M.assert_exact(got, ref, "exact, " + what)
                c = K.wm_case(k, width, n_seg, "float", scattered)
                got, init = _wm_launch(c, strided)
                M.assert_fp32_class(got, *M.weighted_segment_mean(c["x"], c["x_idx"], c["w"], c["off"], c["out_idx"], init),
                                    M.n_eff_weighted_mean(c["off"]), "weighted mean " + what)


def test_weighted_segment_mean_negative_controls():
    c = K.wm_case(5, 65, 257, "float", True)
    got, init = _wm_launch(c, True)
    n_eff = M.n_eff_weighted_mean(c["off"])
    args = (c["x"], c["x_idx"])
    M.assert_fp32_class(got, *M.weighted_segment_mean(*args, c["w"], c["off"], c["out_idx"], init), n_eff, "weighted mean, control's own reference")
    bad = M.weighted_segment_mean(*args, M.drop_last_weight(c["w"], c["off"], 7), c["off"], c["out_idx"], init)
    assert M.rejects(M.assert_fp32_class, got, *bad, n_eff, "dropped neighbour")
    bad = M.weighted_segment_mean(*args, c["w"], M.move_boundary(c["off"], 8), c["out_idx"], init)
    assert M.rejects(M.assert_fp32_class, got, *bad, n_eff, "moved boundary")
    wrong = c["out_idx"].clone()
    wrong[[3, 4]] = wrong[[4, 3]]
    assert M.rejects(M.assert_fp32_class, got, *M.weighted_segment_mean(*args, c["w"], c["off"], wrong, init), n_eff, "output rows exchanged")


# ====================================================================== project_to_edges, edge_scalar_to_node_vector
@pytest.mark.parametrize("n_feat", K.RM_FEATS)
@pytest.mark.parametrize("n_edges", K.RM_N)
def test_project_to_edges(n_edges, n_feat):
    for indexed in (False, True):
        what = f"E {n_edges} f{n_feat} indexed {indexed}"
        c = K.proj_case(n_edges, n_feat, indexed, "int")
        assert c["v"].size(1) > 2 * n_feat                                         # (v_ld > 2 n_feat)
        got = ops.project_to_edges(dev(c["v"]), dev(c["node"]), dev(c["unit"]), n_edges, n_feat).cpu()
        ref, absref = M.project_to_edges(c["v"], c["node"], c["unit"], n_feat)
        M.check_int_bound(absref)
        M.assert_exact(got, ref, "integers, " + what)
        c = K.proj_case(n_edges, n_feat, indexed, "float")
        got = ops.project_to_edges(dev(c["v"]), dev(c["node"]), dev(c["unit"]), n_edges, n_feat).cpu()
        two = M.project_to_edges_fp32(c["v"], c["node"], c["unit"], n_feat)
        assert tuple(got.shape) == (n_edges, n_feat) and torch.equal(got, two), \
            f"{what}: {int((got != two).sum())} elements differ from the two-rounding form"


@pytest.mark.parametrize("n_feat", K.RM_FEATS)
@pytest.mark.parametrize("n_nodes", K.RM_N)
def test_edge_scalar_to_node_vector(n_nodes, n_feat):
    for k in K.RM_K:
        for strided_out in (False, True):
            what = f"N {n_nodes} f{n_feat} k{k} out= {strided_out}"
            for kind in ("int", "float"):
                c = K.e2n_case(n_nodes, n_feat, k, kind)
                e = dev(c["e"])[:, :n_feat]                                       # (e_ld = n_feat + 3)
                if strided_out:
                    out_wide = sentinel(n_nodes, 2 * n_feat + 2)
                    got = ops.edge_scalar_to_node_vector(e, dev(c["unit_inv"]), n_nodes, k, out=out_wide[:, :2 * n_feat]).cpu()
                    pads_untouched(out_wide, 0, 2 * n_feat, "edge_scalar_to_node_vector out=")
                else:
                    got = ops.edge_scalar_to_node_vector(e, dev(c["unit_inv"]), n_nodes, k).cpu()
                ref, absref = M.edge_scalar_to_node_vector(c["e"][:, :n_feat], c["unit_inv"], k)
                if kind == "int":
                    M.check_int_bound(absref)
                    M.assert_exact(got, ref, "integers, " + what)
                else:
                    M.assert_fp32_class(got, ref, absref, k, "edge_scalar_to_node_vector " + what)


def test_remus_helpers_negative_controls():
    c = K.proj_case(257, 64, True, "float")
    got = ops.project_to_edges(dev(c["v"]), dev(c["node"]), dev(c["unit"]), 257, 64).cpu()
    assert torch.equal(got, M.project_to_edges_fp32(c["v"], c["node"], c["unit"], 64))
    assert not torch.equal(got, M.project_to_edges_fp32(c["v"], c["node"], M.swap_unit(c["unit"]), 64)), "unit components swapped"
    assert not torch.equal(got, M.project_to_edges_fp32(c["v"], c["other"], c["unit"], 64)), "the other endpoint's index"
    c = K.proj_case(257, 64, True, "int")
    got = ops.project_to_edges(dev(c["v"]), dev(c["node"]), dev(c["unit"]), 257, 64).cpu()
    assert M.rejects(M.assert_exact, got, M.project_to_edges(c["v"], c["node"], M.swap_unit(c["unit"]), 64)[0], "unit components swapped")
    assert M.rejects(M.assert_exact, got, M.project_to_edges(c["v"], c["other"], c["unit"], 64)[0], "the other endpoint's index")
    c = K.e2n_case(257, 64, 5, "float")
    e = c["e"][:, :64]
    got = ops.edge_scalar_to_node_vector(dev(c["e"])[:, :64], dev(c["unit_inv"]), 257, 5).cpu()
    M.assert_fp32_class(got, *M.edge_scalar_to_node_vector(e, c["unit_inv"], 5), 5, "edge_scalar_to_node_vector, control's own reference")
    assert M.rejects(M.assert_fp32_class, got, *M.edge_scalar_to_node_vector(e, M.swap_unit(c["unit_inv"]), 5), 5, "components swapped")


# ====================================================================== copy_cols, add_cols, activation_
@pytest.mark.parametrize("width", K.CC_WIDTHS)
def test_copy_cols_and_add_cols(width):
    for indexed in (False, True):
        c = K.cc_case(width, indexed)
        dst = sentinel(*c["dst_shape"])
        ops.copy_cols(dev(c["src"]), dst, c["dcol0"], scol0=c["scol0"], width=width, idx32=dev(c["idx"]), n_rows=c["n_rows"])
        ref = M.copy_cols(c["src"], torch.full(c["dst_shape"], K.SENT), c["dcol0"], c["scol0"], width, c["idx"], c["n_rows"])
        assert torch.equal(dst.cpu().double(), ref), f"copy_cols w{width} indexed {indexed}"
        holds_sentinel(dst[c["n_rows"]:], "copy_cols rows past n_rows")
        pads_untouched(dst, c["dcol0"], width, "copy_cols")
        if indexed:       # negative control: the kernel's result against the reference of a shifted index / window
            assert not torch.equal(dst.cpu().double(), M.copy_cols(c["src"], torch.full(c["dst_shape"], K.SENT), c["dcol0"], c["scol0"], width,
                                                                   c["idx"].roll(1), c["n_rows"]))
    # the defaults: the whole width from scol0 on, every row of dst
    c = K.cc_case(width, False)
    dst = sentinel(29, width + 5)
    ops.copy_cols(dev(c["src"]), dst, 2, scol0=3)
    assert torch.equal(dst[:, 2:4 + width].cpu(), c["src"][:29, 3:])
    pads_untouched(dst, 2, width + 2, "copy_cols defaults")
    a = K.ac_case(width)
    b, _ = window(a["b_wide"][:, :width], 0, 3)
    out_wide = sentinel(33, width + 2)
    a_dev = window(a["a"], 1, 0)[0]                                              # (a strided too)
    res = ops.add_cols(a_dev, a["a_col0"], b, out_wide[:, 1:1 + width])
    want = M.add_cols(a["a"], a["a_col0"], a["b_wide"][:, :width])
    assert torch.equal(res.cpu(), want), f"add_cols w{width}"
    pads_untouched(out_wide, 1, width, "add_cols")
    assert not torch.equal(res.cpu(), M.add_cols(a["a"], a["a_col0"] + 1, a["b_wide"][:, :width])), "a_col0 + 1"


def _activate(x, act):
    """ops.activation_ on a 16-byte aligned prefix of a sentinel buffer: (result on the host, the untouched tail checked)."""
    buf = sentinel(x.numel() + 8)
    view = buf[: x.numel()]
    view.copy_(x)
    assert ops.activation_(view, ACT[act]) is view
    holds_sentinel(buf[x.numel():], f"activation_ n {x.numel()}")
    return view.cpu()


@pytest.mark.parametrize("n", K.ACT_N)
def test_activation_inplace(n):
    x = K.act_case(n)
    for act in ("selu", "tanh"):
        M.assert_fp32_class(_activate(x, act), *M.activation(x, act), M.N_EFF_ACT, f"activation_ {act} n {n}")
    assert torch.equal(_activate(x, None), x)                                    # ACT_NONE leaves the buffer untouched
    if n == 1025:                                                                # a 2-D contiguous tensor, the way the models call it
        t = dev(x[:1024].reshape(8, 128).clone())
        ops.activation_(t, ACT["selu"])
        assert torch.equal(t.cpu().reshape(-1), _activate(x[:1024], "selu"))
        assert M.rejects(M.assert_fp32_class, _activate(x, "selu"), *M.activation(x, "tanh"), M.N_EFF_ACT, "the other activation")


def test_activation_special_values():
    x = torch.tensor(K.SPECIAL, dtype=F32)
    finite = torch.isfinite(x)
    sa32 = torch.tensor(M.SELU_SCALE, dtype=F32) * torch.tensor(M.SELU_ALPHA, dtype=F32)
    selu, tanh = _activate(x, "selu"), _activate(x, "tanh")
    M.assert_fp32_class(selu[finite], *M.activation(x[finite], "selu"), M.N_EFF_ACT, "SELU, special values")
    M.assert_fp32_class(tanh[finite], *M.activation(x[finite], "tanh"), M.N_EFF_ACT, "tanh, special values")
    at = {v: i for i, v in enumerate(K.SPECIAL) if v not in (0.0,)}
    assert float(selu[at[float("inf")]]) == float("inf")
    assert float(selu[at[float("-inf")]]) == -float(sa32)                         # SELU(-inf) = -scale * alpha
    assert float(tanh[at[float("inf")]]) == 1.0 and float(tanh[at[float("-inf")]]) == -1.0
    assert float(tanh[at[20.0]]) == 1.0 and float(tanh[at[-20.0]]) == -1.0 and float(tanh[at[1e30]]) == 1.0
    assert float(selu[at[-1e30]]) == -float(sa32) and float(selu[at[-88.0]]) == -float(sa32)
    # the sign of zero is preserved by tanh (K.SPECIAL[0] = +0, [1] = -0); tanh of a subnormal keeps its sign too
    assert float(tanh[0]) == 0.0 and not bool(torch.signbit(tanh[0])) and float(tanh[1]) == 0.0 and bool(torch.signbit(tanh[1]))
    assert bool(torch.signbit(tanh[at[-1e-40]])) and not bool(torch.signbit(tanh[at[1e-40]]))
    assert float(selu[0]) == 0.0 and float(selu[1]) == 0.0


def test_activation_nan_is_not_propagated():
    """Documented difference from F.selu / torch.tanh (include/g4c.h G4C_ACT_*), as measured on gfx950: the branch-free
    activations do not propagate NaN.  selu_f: fmaxf(NaN, 0) = 0 and the [0, 1] clamp of exp2(NaN) gives 0, so SELU(NaN) =
    -scale * alpha = -1.7580993 (0xbfe10966), SELU's limit at -inf, for either sign of the NaN; tanh_f: fminf(|NaN|, 20) = 20, so
    tanh(NaN) = +1 / -1 by the NaN's sign bit."""
    bits = torch.tensor([0x7FC00000, 0xFFC00000 - 2 ** 32], dtype=torch.int64).to(I32)     # quiet NaN, sign clear / set
    x = bits.view(F32)
    assert bool(torch.isnan(x).all()) and not bool(torch.signbit(x[0])) and bool(torch.signbit(x[1]))
    sa32 = float(torch.tensor(M.SELU_SCALE, dtype=F32) * torch.tensor(M.SELU_ALPHA, dtype=F32))
    selu, tanh = _activate(x, "selu"), _activate(x, "tanh")
    print(f"  SELU(+NaN, -NaN) = {selu.tolist()}, tanh(+NaN, -NaN) = {tanh.tolist()}")
    assert selu.tolist() == [-sa32, -sa32]
    assert tanh.tolist() == [1.0, -1.0]
    # the same through a fused epilogue that shares the device functions: segment_reduce's src_act / act
    c = K.seg_case(7, 4, "none", "float")
    src = c["src"].clone()
    src[:] = x[0]
    got = ops.segment_reduce(dev(src), csr_of(c), False, ACT["tanh"], src_act=ACT["selu"]).cpu()
    cnt = M.counts(c["off"]).double()[:, None].expand(-1, 4)
    M.assert_fp32_class(got, *M.through_act(-sa32 * cnt, sa32 * cnt * (1 + M.U), "tanh"), 40 + M.N_EFF_ACT, "tanh(sum SELU(NaN))")


# ====================================================================== layer_norm
@pytest.mark.parametrize("width", K.LN_WIDTHS)
def test_layer_norm(width):
    c = K.ln_case(width)
    gamma_d, beta_d = dev(c["gamma"]), dev(c["beta"])
    rows_seen = set()
    for rows, affine, act, inplace, strided in K.LN_CONFIGS:
        rows_seen.add(rows)
        x = c["x"][:rows]
        g, b = (c["gamma"], c["beta"]) if affine else (None, None)
        gd, bd = (gamma_d, beta_d) if affine else (None, None)
        what = f"layer_norm w{width} rows {rows} affine {affine} {act} inplace {inplace} strided {strided}"
        x_dev, x_wide = window(x, 1, 2) if strided else (dev(x).clone(), None)
        if inplace:
            res = ops.layer_norm(x_dev, gd, bd, K.LN_EPS, ACT[act], out=x_dev)
            assert res is x_dev
        elif strided:
            out_wide = sentinel(rows, width + 5)
            res = ops.layer_norm(x_dev, gd, bd, K.LN_EPS, ACT[act], out=out_wide[:, 2:2 + width])
            pads_untouched(out_wide, 2, width, what)
        else:
            res = ops.layer_norm(x_dev, gd, bd, K.LN_EPS, ACT[act])
            assert tuple(res.shape) == (rows, width)
        if x_wide is not None:
            pads_untouched(x_wide, 1, width, what + ", input")
        if not inplace:
            assert torch.equal(x_dev.cpu(), x), what + ": the input was modified"
        M.assert_fp32_class(res.cpu(), *M.layer_norm(x, g, b, K.LN_EPS, act), M.n_eff_layer_norm(width, act), what)
    assert rows_seen == set(K.LN_ROWS)


def test_layer_norm_negative_controls():
    for width in (65, 1100):
        c = K.ln_case(width)
        x, fam = c["x"], c["family"]
        got = ops.layer_norm(dev(x), dev(c["gamma"]), dev(c["beta"]), K.LN_EPS).cpu()
        n_eff = M.n_eff_layer_norm(width)
        for f_id, name in enumerate(K.LN_FAMILIES):
            sel = fam == f_id
            ref = M.layer_norm(x[sel], c["gamma"], c["beta"], K.LN_EPS)
            M.assert_fp32_class(got[sel], *ref, n_eff, f"layer_norm w{width}, {name} rows")
            bad = M.layer_norm(x[sel], c["gamma"], c["beta"], K.LN_EPS, denom=width + 1)
            assert M.rejects(M.assert_fp32_class, got[sel], *bad, n_eff, name) == (name != "tiny"), name
        # what the bound is worth: a one-pass variance in fp32 fails it on the rows with a common offset of 1e4
        off_rows = x[fam == 1]
        one = M.layer_norm_one_pass_fp32(off_rows, c["gamma"], c["beta"], K.LN_EPS)
        assert M.rejects(M.assert_fp32_class, one, *M.layer_norm(off_rows, c["gamma"], c["beta"], K.LN_EPS), n_eff, "one-pass variance")


# ====================================================================== rollout_advance
@pytest.mark.parametrize("nf,cols", K.RA_SHAPES)
@pytest.mark.parametrize("n_nodes", K.RA_NODES)
def test_rollout_advance(n_nodes, nf, cols):
    c = K.ra_case(n_nodes, nf, cols)
    for layout, shape in (("rows", (n_nodes, nf * K.RA_SLOTS)), ("steps", (K.RA_SLOTS, n_nodes, nf))):
        field, outputs, step = dev(c["field"]).clone(), sentinel(*shape), torch.zeros(2, dtype=I32, device=DEV)
        ref_f, ref_o, ref_t = c["field"].double(), torch.full(shape, K.SENT, dtype=F64), 0
        for t, pred in enumerate(c["preds"]):                    # six consecutive launches on one stream
            ops.rollout_advance(field, dev(pred), outputs, step, nf)
            ref_f, ref_o, ref_t = M.rollout_advance(ref_f, pred, ref_o, t, layout)
            what = f"rollout_advance n {n_nodes} nf {nf} cols {cols} {layout} step {t}"
            assert step.tolist() == [t + 1, 0] and ref_t == t + 1, what
            M.assert_exact(field.cpu(), ref_f, what + ", field")
            assert torch.equal(outputs.cpu().double(), ref_o), what + ", outputs"
            later = outputs[:, nf * (t + 1):] if layout == "rows" else outputs[t + 1:]
            holds_sentinel(later, what + ", slots of steps not yet taken")
        if layout == "steps" and n_nodes:
            assert torch.equal(ops.steps_to_columns(outputs[:K.RA_STEPS]).cpu().double(), torch.cat([p.double() for p in c["preds"]], 1))


def test_rollout_advance_negative_controls():
    c = K.ra_case(257, 3, 15)
    pred = c["preds"][0]
    for layout, shape in (("rows", (257, 3 * K.RA_SLOTS)), ("steps", (K.RA_SLOTS, 257, 3))):
        field, outputs = dev(c["field"]).clone(), sentinel(*shape)
        step = torch.tensor([2, 0], dtype=I32, device=DEV)
        ops.rollout_advance(field, dev(pred), outputs, step, 3)
        assert step.tolist() == [3, 0]
        init = torch.full(shape, K.SENT)
        good = M.rollout_advance(c["field"], pred, init, 2, layout)
        M.assert_exact(field.cpu(), good[0], "field")
        assert torch.equal(outputs.cpu().double(), good[1])
        for d in (1, -1):
            assert M.rejects(M.assert_exact, field.cpu(), M.roll_shifted(c["field"], pred, d), f"roll by nf {d:+d}")
        assert not torch.equal(outputs.cpu().double(), M.rollout_advance(c["field"], pred, init, 3, layout)[1]), "slot t + 1"


# ====================================================================== malformed calls are stopped in Python
def test_malformed_calls_raise_and_write_nothing():
    c = K.seg_case(9, 128, "full", "int")
    csr, src = csr_of(c), dev(c["src"])
    out = sentinel(9, 128)
    w = K.wm_case(4, 64, 257, "float", False)
    wcsr = plan.CsrPlan(perm=None, off=dev(w["off"]), n=w["n"], n_seg=257, max_deg=4)
    wout = sentinel(257, 64)
    x, gamma = dev(K.ln_case(65)["x"]), dev(K.ln_case(65)["gamma"])
    ln_out = sentinel(301, 65)
    field, outputs, step = sentinel(50, 6), sentinel(50, 12), torch.zeros(2, dtype=I32, device=DEV)
    dst, e_out = sentinel(20, 8), sentinel(10, 6)
    idx64 = torch.zeros(20, dtype=torch.int64, device=DEV)
    buf = sentinel(64)
    calls = [
        (ValueError, lambda: ops.segment_reduce(src[:-1], plan.CsrPlan(None, csr.off, csr.n, 9, 40), False, out=out)),
        (ValueError, lambda: ops.segment_reduce(src, csr, False, out=out[:8])),
        (TypeError, lambda: ops.segment_reduce(src, plan.CsrPlan(csr.perm.long(), csr.off, csr.n, 9, 40), False, out=out)),
        (TypeError, lambda: ops.weighted_segment_mean(dev(w["x"]), dev(w["x_idx"]).long(), dev(w["w"]), wcsr, wout)),
        (ValueError, lambda: ops.weighted_segment_mean(dev(w["x"]), dev(w["x_idx"])[:-1], dev(w["w"]), wcsr, wout)),
        (ValueError, lambda: ops.layer_norm(x, gamma[:-1], None, 1e-5, out=ln_out)),
        (ValueError, lambda: ops.layer_norm(x, None, None, 1e-5, out=ln_out[:300])),
        (ValueError, lambda: ops.rollout_advance(field, sentinel(49, 3), outputs, step, 3)),
        (TypeError, lambda: ops.rollout_advance(field, sentinel(50, 3).double(), outputs, step, 3)),
        (TypeError, lambda: ops.copy_cols(field, dst, 0, idx32=idx64, n_rows=20)),
        (ValueError, lambda: ops.copy_cols(field, dst, 4)),
        (ValueError, lambda: ops.add_cols(field[:19], 0, sentinel(20, 6), dst[:, :6])),
        (TypeError, lambda: ops.project_to_edges(field, idx64, sentinel(20, 2), 20, 3)),
        (ValueError, lambda: ops.edge_scalar_to_node_vector(field, sentinel(10, 2, 5), 10, 5, out=e_out)),
        (ValueError, lambda: ops.activation_(buf.view(8, 8)[:, :4], ACT["selu"])),
        (TypeError, lambda: ops.activation_(idx64, ACT["selu"])),
    ]
    for exc, call in calls:
        with pytest.raises(exc):
            call()
    torch.cuda.synchronize()
    for name, t in (("segment_reduce out", out), ("weighted_segment_mean out", wout), ("layer_norm out", ln_out), ("field", field),
                    ("outputs", outputs), ("copy_cols / add_cols dst", dst), ("edge_scalar_to_node_vector out", e_out), ("activation_ x", buf)):
        holds_sentinel(t, name + " after a malformed call")
    assert step.tolist() == [0, 0] and int(idx64.sum()) == 0
