"""The fp64 references of the memory-bound helper launches (oracle/mem_ref.py) and their checkers, on CPU, at the shapes and data
tests/test_gpu_mem_ref.py launches (tests/mem_cases.py): each reference equals the plain torch formulation of the operation
(index_add_, F.layer_norm in float64, torch.roll + a slice assignment ...), each integer generator keeps every sum below 2^24, a
plain fp32 evaluation in the kernel's summation order passes every exact and bounded check (the bounds are attainable: the
measured / allowed ratios are printed) and every perturbation is rejected by the same checkers on that fp32 result."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mem_cases as K                        # noqa: E402
from oracle import mem_ref as M              # noqa: E402

F64, F32 = torch.float64, torch.float32
TORCH_ACT = {None: lambda t: t, "selu": F.selu, "tanh": torch.tanh}


# ================================================================== fp32 restatements in the kernels' order
def seg_reduce_fp32(src, off, perm, mean, src_act=None, act=None):
    """One fp32 accumulator per (segment, column), rows added in plan order; mean: one division by (float)max(count, 1)."""
    s = TORCH_ACT[src_act](src.to(F32))
    cnt, beg = M.counts(off), off.long()[:-1]
    acc = torch.zeros(cnt.numel(), src.size(1), dtype=F32)
    for j in range(int(cnt.max()) if cnt.numel() else 0):
        on = cnt > j
        p = beg[on] + j
        acc[on] = acc[on] + s[perm.long()[p] if perm is not None else p]
    if mean:
        acc = acc / cnt.clamp(min=1).to(F32)[:, None]
    return TORCH_ACT[act](acc)


def weighted_mean_fp32(x, x_idx, w, off):
    cnt, beg = M.counts(off), off.long()[:-1]
    num, den = torch.zeros(cnt.numel(), x.size(1), dtype=F32), torch.zeros(cnt.numel(), dtype=F32)
    for j in range(int(cnt.max()) if cnt.numel() else 0):
        on = cnt > j
        p = beg[on] + j
        num[on] = num[on] + x[x_idx.long()[p]] * w[p][:, None]
        den[on] = den[on] + w[p]
    return num / den[:, None]


def fma32(a, b, c):
    """fmaf: the fp64 product of two fp32 values is exact; one rounding of the sum to fp32."""
    return (a.to(F64) * b.to(F64) + c.to(F64)).to(F32)


def e2n_fp32(e, ui, k):
    n, f = ui.size(0), e.size(1)
    ek = e.reshape(n, k, f)
    s = torch.zeros(n, f, 2, dtype=F32)
    for j in range(k):
        for c in range(2):
            s[:, :, c] = fma32(ui[:, c, j][:, None], ek[:, j], s[:, :, c])
    return s.reshape(n, 2 * f)


def _wave_sum(t):
    """[rows, width] -> [rows, 1]: lane l adds columns l, l + 64, ... in order, then the six-level xor butterfly."""
    rows, width = t.shape
    cpl = -(-width // 64)
    pad = torch.zeros(rows, cpl * 64, dtype=F32)
    pad[:, :width] = t
    lanes = torch.zeros(rows, 64, dtype=F32)
    for j in range(cpl):
        lanes = lanes + pad[:, 64 * j:64 * (j + 1)]
    lane = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[:, lane ^ o]
    return lanes[:, :1]


def layer_norm_fp32(x, gamma, beta, eps, act=None, denom=None):
    x = x.to(F32)
    w = torch.tensor(float(x.size(1) if denom is None else denom), dtype=F32)
    mean = _wave_sum(x) / w
    d = x - mean
    rstd = torch.rsqrt(_wave_sum(d * d) / w + torch.tensor(eps, dtype=F32))
    g = torch.ones(x.size(1)) if gamma is None else gamma
    b = torch.zeros(x.size(1)) if beta is None else beta
    return TORCH_ACT[act](fma32(d * rstd, g[None, :], b[None, :]))


# ================================================================== each reference = the plain torch formulation
def test_segment_reduce_reference_equals_scatter():
    for n_seg, width, perm in ((33, 6, "subset"), (9, 4, "full"), (1031, 3, "none")):
        c = K.seg_case(n_seg, width, perm, "float")
        seg = torch.repeat_interleave(torch.arange(n_seg), M.counts(c["off"]))
        key = torch.full((c["src"].size(0),), -1, dtype=torch.int64)         # the scatter index of every src row (-1: not named)
        key[c["perm"].long() if c["perm"] is not None else torch.arange(c["n"])] = seg
        named = key >= 0
        for mean in (False, True):
            for sa, a in ((None, None), ("selu", "tanh"), ("tanh", "selu")):
                x = TORCH_ACT[sa](c["src"].double())
                want = torch.zeros(n_seg, width, dtype=F64).index_add_(0, key[named], x[named])
                if mean:
                    want = want / torch.bincount(key[named], minlength=n_seg).clamp(min=1)[:, None]
                got, ga = M.segment_reduce(c["src"], c["off"], c["perm"], mean, sa, a)
                torch.testing.assert_close(got, TORCH_ACT[a](want), rtol=1e-12, atol=1e-12)
                assert (got.abs() <= ga * (1 + 1e-12)).all()
    c = K.seg_case(9, 4, "none", "int")          # the empty segments of a mean are 0 / max(0, 1) = 0
    got = M.segment_reduce(c["src"], c["off"], None, True)[0]
    assert (got[M.counts(c["off"]) == 0] == 0).all()


def test_weighted_mean_reference_equals_scatter_quotient():
    c = K.wm_case(5, 65, 257, "float", True)
    y_idx = torch.repeat_interleave(torch.arange(257), M.counts(c["off"]))
    x, w = c["x"].double(), c["w"].double()
    y = torch.zeros(257, 65, dtype=F64).index_add_(0, y_idx, x[c["x_idx"].long()] * w[:, None])
    y /= torch.zeros(257, dtype=F64).index_add_(0, y_idx, w)[:, None]
    init = torch.full((c["n_out"], 65), K.SENT)
    got, ga = M.weighted_segment_mean(c["x"], c["x_idx"], c["w"], c["off"], c["out_idx"], init)
    torch.testing.assert_close(got[c["out_idx"].long()], y, rtol=1e-12, atol=0)
    rest = torch.ones(c["n_out"], dtype=torch.bool)
    rest[c["out_idx"].long()] = False
    assert (got[rest] == K.SENT).all() and (ga[rest] == 0).all() and int(rest.sum()) == c["n_out"] - 257
    torch.testing.assert_close(M.weighted_segment_mean(c["x"], c["x_idx"], c["w"], c["off"])[0], y, rtol=1e-12, atol=0)


def test_remus_references_equal_the_reshape_formulations():
    c = K.proj_case(257, 3, True, "float")
    want = (c["v"].double()[c["node"].long()][:, :6].reshape(257, -1, 2) * c["unit"].double().unsqueeze(1)).sum(-1)
    torch.testing.assert_close(M.project_to_edges(c["v"], c["node"], c["unit"], 3)[0], want, rtol=1e-13, atol=1e-13)
    two = M.project_to_edges_fp32(c["v"], c["node"], c["unit"], 3)
    x = c["v"][c["node"].long()][:, :6].reshape(257, -1, 2)
    assert torch.equal(two, x[:, :, 0] * c["unit"][:, :1] + x[:, :, 1] * c["unit"][:, 1:])     # torch's fp32 ops round the same way
    c = K.e2n_case(255, 3, 5, "float")
    e = c["e"][:, :3].double()
    want = (c["unit_inv"].double() @ e.view(255, -1, 3)).transpose(1, 2).flatten(1, 2)
    torch.testing.assert_close(M.edge_scalar_to_node_vector(c["e"][:, :3], c["unit_inv"], 5)[0], want, rtol=1e-13, atol=1e-13)


def test_column_helpers_and_activations_equal_torch():
    c = K.cc_case(3, True)
    dst = torch.full(c["dst_shape"], K.SENT)
    want = dst.clone()
    want[:23, 3:6] = c["src"][c["idx"].long()[:23], 2:5]
    assert torch.equal(M.copy_cols(c["src"], dst, 3, 2, 3, c["idx"], 23).float(), want)
    a = K.ac_case(3)
    assert torch.equal(M.add_cols(a["a"], 4, a["b_wide"][:, :3]), a["a"][:33, 4:7] + a["b_wide"][:, :3])
    x = torch.cat((K.act_case(1025), torch.tensor(K.SPECIAL))).double()
    for act, fn in (("selu", F.selu), ("tanh", torch.tanh)):
        v, va = M.activation(x, act)
        torch.testing.assert_close(v, fn(x), rtol=1e-14, atol=1e-300)
        assert (v.abs() <= va).all()
    assert float(M.activation(torch.tensor([float("-inf")]), "selu")[0]) == -M.SELU_SA


@pytest.mark.parametrize("width", (1, 65, 1100))
def test_layer_norm_reference_equals_float64_layer_norm(width):
    c = K.ln_case(width)
    x = c["x"].double()
    keep = c["family"] != 4 if width == 1 else slice(None)
    for gamma, beta in ((c["gamma"], c["beta"]), (None, None)):
        want = F.layer_norm(x, (width,), None if gamma is None else gamma.double(), None if beta is None else beta.double(), K.LN_EPS)
        for act in K.ACTS:
            got, ga = M.layer_norm(c["x"], gamma, beta, K.LN_EPS, act)
            torch.testing.assert_close(got[keep], TORCH_ACT[act](want)[keep], rtol=1e-9, atol=1e-9)
            assert (got.abs() <= ga * (1 + 1e-12) + 1e-300).all()


def test_rollout_reference_equals_roll_and_slice_assignment():
    for nf, cols in K.RA_SHAPES:
        c = K.ra_case(257, nf, cols)
        field = c["field"].double()
        rows, steps = torch.full((257, nf * K.RA_SLOTS), K.SENT, dtype=F64), torch.full((K.RA_SLOTS, 257, nf), K.SENT, dtype=F64)
        f2, r2, s2 = field.clone(), rows.clone(), steps.clone()
        for t, pred in enumerate(c["preds"]):
            field = torch.roll(field, -nf, 1)                      # (GNN.solve's bookkeeping)
            field[:, cols - nf:] = pred.double()
            rows[:, nf * t:nf * (t + 1)] = pred.double()
            steps[t] = pred.double()
            f2, r2, t2 = M.rollout_advance(f2, pred, r2, t, "rows")
            _, s2, _ = M.rollout_advance(f2, pred, s2, t, "steps")
            assert t2 == t + 1 and torch.equal(f2, field) and torch.equal(r2, rows) and torch.equal(s2, steps)
        assert (r2[:, nf * K.RA_STEPS:] == K.SENT).all() and (s2[K.RA_STEPS] == K.SENT).all()


# ================================================================== integer generators
def test_integer_generators_stay_below_2_24_at_every_gpu_shape():
    for n_seg in K.N_SEGS:
        for width in (K.VEC_WIDTHS + K.SCALAR_WIDTHS) if n_seg <= 33 else (4, 260, 130):
            for perm in K.PERMS:
                c = K.seg_case(n_seg, width, perm, "int")
                M.check_int_bound(M.segment_reduce(c["src"], c["off"], c["perm"], False)[1])
    for k in K.WM_K:
        for width in K.WM_WIDTHS:
            c = K.wm_case(k, width, 257, "int", False)
            val, vala = M.weighted_segment_mean(c["x"], c["x_idx"], c["w"], c["off"])
            M.check_int_bound(vala * 8 * 8)                # (the numerator: |x| <= 8 times weights <= 4 * 2^3, in units of 2^-3)
            w = c["w"].double().reshape(257, k).sum(1)
            assert torch.equal(torch.log2(w), torch.log2(w).round()), "weights of a segment must sum to a power of two"
            assert torch.equal(val.float().double(), val), "the quotient must be an fp32 number"
    for n in K.RM_N:
        for f in K.RM_FEATS:
            c = K.proj_case(n, f, True, "int")
            M.check_int_bound(M.project_to_edges(c["v"], c["node"], c["unit"], f)[1])
            for k in K.RM_K:
                c = K.e2n_case(n, f, k, "int")
                M.check_int_bound(M.edge_scalar_to_node_vector(c["e"][:, :f], c["unit_inv"], k)[1])
    assert M.rejects(M.check_int_bound, torch.tensor([2.0 ** 24]))


# ================================================================== exact checks: fp32 accepted, perturbations rejected
@pytest.mark.parametrize("n_seg,width,perm", [(33, 128, "subset"), (1031, 6, "full"), (9, 132, "none"), (7, 1, "subset"), (1, 260, "none")])
def test_segment_reduce_exact_checks_and_controls(n_seg, width, perm):
    c = K.seg_case(n_seg, width, perm, "int")
    src, off, p = c["src"], c["off"], c["perm"]
    got_sum, got_mean = seg_reduce_fp32(src, off, p, False), seg_reduce_fp32(src, off, p, True)
    M.assert_exact(got_sum, M.segment_reduce(src, off, p, False)[0], "sum")
    M.assert_exact(got_mean, M.segment_mean_fp32(src, off, p), "mean")
    lens = M.counts(off)
    assert len(set(lens.tolist()) - {0, 1, 2, 4, 8, 16}) >= 1, "counts must include non-powers of two"
    s = int(torch.nonzero(lens > 1)[-1])                      # the last segment of two or more rows
    controls = [("row moved into the next segment", src, M.move_boundary(off, s + 1) if s + 1 < n_seg else M.move_boundary(off, s)),
                ("last row dropped", M.drop_last_row(src, off, p, s), off)]
    for what, src_b, off_b in controls:
        if n_seg == 1 and src_b is src:
            continue                                         # (a single segment has no boundary to move)
        assert M.rejects(M.assert_exact, got_sum, M.segment_reduce(src_b, off_b, p, False)[0], what), what
        assert M.rejects(M.assert_exact, got_mean, M.segment_mean_fp32(src_b, off_b, p), what), what
    # the mean is NOT the fp64 quotient rounded twice nor a product with the rounded reciprocal: the check tells them apart
    recip = seg_reduce_fp32(src, off, p, False) * (1.0 / lens.clamp(min=1).to(F32))[:, None]
    if n_seg >= 33 and width >= 6:
        assert M.rejects(M.assert_exact, recip, M.segment_mean_fp32(src, off, p), "reciprocal product")


def test_segment_reduce_bounded_checks_and_controls():
    ratios = []
    for width in (128, 6):
        c = K.seg_case(33, width, "subset", "float")
        src, off, p = c["src"], c["off"], c["perm"]
        s = int(torch.nonzero(M.counts(off) == 40)[0])
        for mean in (False, True):
            for sa in K.ACTS:
                for a in K.ACTS:
                    got = seg_reduce_fp32(src, off, p, mean, sa, a)
                    n_eff = M.n_eff_segment_reduce(off, mean, sa, a)
                    ref = M.segment_reduce(src, off, p, mean, sa, a)
                    ratios.append(M.assert_fp32_class(got, *ref, n_eff, f"segment_reduce w{width} mean={mean} {sa}/{a}"))
                    for what, bad in (("moved boundary", M.segment_reduce(src, M.move_boundary(off, s), p, mean, sa, a)),
                                      ("dropped row", M.segment_reduce(M.drop_last_row(src, off, p, s - 1), off, p, mean, sa, a))):
                        assert M.rejects(M.assert_fp32_class, got, *bad, n_eff, what), (what, mean, sa, a)
    assert max(ratios) < 0.5, max(ratios)


@pytest.mark.parametrize("k", K.WM_K)
def test_weighted_mean_checks_and_controls(k):
    for width in (3, 65):
        c = K.wm_case(k, width, 257, "int", False)
        got = weighted_mean_fp32(c["x"], c["x_idx"], c["w"], c["off"])
        M.assert_exact(got, M.weighted_segment_mean(c["x"], c["x_idx"], c["w"], c["off"])[0], "exact")
        if k > 1:
            bad = M.weighted_segment_mean(c["x"], c["x_idx"], c["w"], M.move_boundary(c["off"], 100))[0]
            assert M.rejects(M.assert_exact, got, bad.float().double(), "moved boundary")
        c = K.wm_case(k, width, 257, "float", True)
        init = torch.full((c["n_out"], width), K.SENT)
        got = init.clone()
        got[c["out_idx"].long()] = weighted_mean_fp32(c["x"], c["x_idx"], c["w"], c["off"])
        n_eff = M.n_eff_weighted_mean(c["off"])
        assert n_eff == k + 1
        r = M.assert_fp32_class(got, *M.weighted_segment_mean(c["x"], c["x_idx"], c["w"], c["off"], c["out_idx"], init), n_eff, f"weighted mean k{k} w{width}")
        assert r < 0.75, r
        assert float(c["w"].max()) / float(c["w"].min()) > 1e15
        if k > 1:
            for s in (7, 10):                 # (segment 10 holds a coincident point: its last neighbour weighs 1e-16 of the sum)
                bad = M.weighted_segment_mean(c["x"], c["x_idx"], M.drop_last_weight(c["w"], c["off"], s), c["off"], c["out_idx"], init)
                assert M.rejects(M.assert_fp32_class, got, *bad, n_eff, "dropped neighbour") == (s == 7), s
            bad = M.weighted_segment_mean(c["x"], c["x_idx"], c["w"], M.move_boundary(c["off"], 8), c["out_idx"], init)
            assert M.rejects(M.assert_fp32_class, got, *bad, n_eff, "moved boundary")
        wrong = c["out_idx"].clone()
        wrong[[3, 4]] = wrong[[4, 3]]
        bad = M.weighted_segment_mean(c["x"], c["x_idx"], c["w"], c["off"], wrong, init)
        assert M.rejects(M.assert_fp32_class, got, *bad, n_eff, "two output rows exchanged")


def test_remus_helper_checks_and_controls():
    for f in K.RM_FEATS:
        c = K.proj_case(257, f, True, "float")
        x = c["v"][c["node"].long()][:, :2 * f].reshape(257, f, 2)
        got = x[:, :, 0] * c["unit"][:, :1] + x[:, :, 1] * c["unit"][:, 1:]
        assert torch.equal(got, M.project_to_edges_fp32(c["v"], c["node"], c["unit"], f))
        assert not torch.equal(got, M.project_to_edges_fp32(c["v"], c["node"], M.swap_unit(c["unit"]), f))
        assert not torch.equal(got, M.project_to_edges_fp32(c["v"], c["other"], c["unit"], f))
        fused = fma32(x[:, :, 0], c["unit"][:, :1], x[:, :, 1] * c["unit"][:, 1:])
        assert f == 1 or not torch.equal(fused, got), "an fma contraction must be told from the two-rounding form"
        c = K.proj_case(257, f, True, "int")
        x = c["v"][c["node"].long()][:, :2 * f].reshape(257, f, 2)
        got = x[:, :, 0] * c["unit"][:, :1] + x[:, :, 1] * c["unit"][:, 1:]
        M.assert_exact(got, M.project_to_edges(c["v"], c["node"], c["unit"], f)[0], "project int")
        assert M.rejects(M.assert_exact, got, M.project_to_edges(c["v"], c["node"], M.swap_unit(c["unit"]), f)[0], "units swapped")
        assert M.rejects(M.assert_exact, got, M.project_to_edges(c["v"], c["other"], c["unit"], f)[0], "other endpoint")
        for k in K.RM_K:
            c = K.e2n_case(257, f, k, "int")
            e = c["e"][:, :f]
            M.assert_exact(e2n_fp32(e, c["unit_inv"], k), M.edge_scalar_to_node_vector(e, c["unit_inv"], k)[0], "e2n int")
            c = K.e2n_case(257, f, k, "float")
            e = c["e"][:, :f]
            got = e2n_fp32(e, c["unit_inv"], k)
            r = M.assert_fp32_class(got, *M.edge_scalar_to_node_vector(e, c["unit_inv"], k), k, f"edge_scalar_to_node_vector f{f} k{k}")
            assert r <= 0.5, r
            assert M.rejects(M.assert_fp32_class, got, *M.edge_scalar_to_node_vector(e, M.swap_unit(c["unit_inv"]), k), k, "components swapped")


def test_activation_bound_accepts_torch_fp32_and_tells_the_activations_apart():
    x = torch.cat((K.act_case(1025), torch.tensor([v for v in K.SPECIAL if abs(v) != float("inf")])))
    for act in ("selu", "tanh"):
        r = M.assert_fp32_class(TORCH_ACT[act](x), *M.activation(x, act), M.N_EFF_ACT, f"activation {act}")
        assert r < 0.5, r
        other = "tanh" if act == "selu" else "selu"
        assert M.rejects(M.assert_fp32_class, TORCH_ACT[other](x), *M.activation(x, act), M.N_EFF_ACT, "the other activation")


@pytest.mark.parametrize("width", K.LN_WIDTHS)
def test_layer_norm_bound_is_attainable_and_meaningful(width):
    c = K.ln_case(width)
    x, fam = c["x"], c["family"]
    worst = 0.0
    for rows, affine, act, _, _ in K.LN_CONFIGS:
        g, b = (c["gamma"], c["beta"]) if affine else (None, None)
        got = layer_norm_fp32(x[:rows], g, b, K.LN_EPS, act)
        n_eff = M.n_eff_layer_norm(width, act)
        worst = max(worst, M.assert_fp32_class(got, *M.layer_norm(x[:rows], g, b, K.LN_EPS, act), n_eff, f"layer_norm w{width} rows{rows} {act}"))
        if rows and width > 1:
            bad = M.layer_norm(x[:rows], g, b, K.LN_EPS, act, denom=width + 1)
            assert M.rejects(M.assert_fp32_class, got, *bad, n_eff, "normalised by width + 1"), (rows, act)
    assert worst < 0.5, worst
    if width > 1:
        # per family: the width + 1 control is caught on every family but the rows of 1e-20, whose output is beta to 1e-18 either way
        n_eff = M.n_eff_layer_norm(width)
        got = layer_norm_fp32(x, c["gamma"], c["beta"], K.LN_EPS)
        for f_id, name in enumerate(K.LN_FAMILIES):
            sel = fam == f_id
            bad = M.layer_norm(x[sel], c["gamma"], c["beta"], K.LN_EPS, denom=width + 1)
            assert M.rejects(M.assert_fp32_class, got[sel], *bad, n_eff, name) == (name != "tiny"), name
        # the one-pass variance is rejected on the offset rows — and only a two-pass kernel passes them
        off_rows = x[fam == 1]
        one = M.layer_norm_one_pass_fp32(off_rows, c["gamma"], c["beta"], K.LN_EPS)
        assert M.rejects(M.assert_fp32_class, one, *M.layer_norm(off_rows, c["gamma"], c["beta"], K.LN_EPS), n_eff, "one-pass variance")


def test_rollout_and_column_controls():
    for nf, cols in K.RA_SHAPES:
        c = K.ra_case(257, nf, cols)
        pred = c["preds"][0]
        for layout, shape in (("rows", (257, nf * K.RA_SLOTS)), ("steps", (K.RA_SLOTS, 257, nf))):
            out0 = torch.full(shape, K.SENT)
            f1, o1, _ = M.rollout_advance(c["field"], pred, out0, 2, layout)
            got_f = torch.cat((c["field"][:, nf:], pred), 1)
            M.assert_exact(got_f, f1, "field")
            if cols > nf + 1:
                for d in (1, -1):
                    assert M.rejects(M.assert_exact, got_f, M.roll_shifted(c["field"], pred, d), f"roll by nf {d:+d}")
            assert M.rejects(M.assert_exact, o1.float(), M.rollout_advance(c["field"], pred, out0, 3, layout)[1], "slot t + 1")
    c = K.cc_case(128, True)
    dst = torch.full(c["dst_shape"], K.SENT)
    good = M.copy_cols(c["src"], dst, 3, 2, 128, c["idx"], 23)
    assert M.rejects(M.assert_exact, good.float(), M.copy_cols(c["src"], dst, 3, 2, 128, c["idx"].roll(1), 23), "index shifted")
    assert M.rejects(M.assert_exact, good.float(), M.copy_cols(c["src"], dst, 4, 2, 128, c["idx"], 23), "window shifted")
