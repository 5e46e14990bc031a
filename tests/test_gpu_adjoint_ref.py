"""The backward that only the multi-scale, gMuS and REMuS models use, against plain fp64 references (oracle/grad_ref.py, sections
"linear adjoints" and "blocks"), at the cases of tests/adjoint_cases.py (tests/test_adjoint_ref.py proves on the host what the
references and the cases claim).

Op by op — the autograd Functions of autograd.py below _FusedMLP through their public entry points, under torch.enable_grad() with
inputs that require grad, a given `dout` in every layout autograd may hand over: forward value and every input gradient.  Exact
(`assert_exact`) wherever every coefficient can be an integer (the gather adjoint, sums, means over power-of-two segments, the REMuS
helpers with integer unit vectors, the weighted mean with power-of-two totals); bounded (`assert_fp32_class`, the one constant C, n_eff
counted from the code next to each use) on random operands.  Every backward runs twice and must repeat its bits; the interpolation
coefficients equal the sequential-order reference bit for bit.

Block by block — DownMP, UpMP, EdgeMP, DownEdgeMP, UpEdgeMP (public forward and the internal forms the models record) and the gMuS
restriction / interpolation, on synthetic graphs: outputs, every input gradient and every parameter gradient against the composed
references, SELU slopes taken from the fp32 activations the backward used (no row needs an allowance).

Negative controls perturb a reference's inputs only.  With G4C_ADJOINT_REF_REPORT=<path> the largest measured / allowed ratio of every
check is written there (tests/ADJOINT_REF_MEASURED.md)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pytestmark = pytest.mark.gpu

from graphs4cfd_amd import _lib, ops, plan, autograd as A, synthetic as S     # noqa: E402
from graphs4cfd_amd.nn import blocks as B                                     # noqa: E402
from oracle import grad_ref as R                                              # noqa: E402
import adjoint_cases as K                                                     # noqa: E402

DEV = torch.device("cuda", 0)
F64 = torch.float64
I32 = torch.int32
ACT = {"selu": _lib.ACT_SELU, "tanh": _lib.ACT_TANH, None: _lib.ACT_NONE}


@pytest.fixture(scope="module", autouse=True)
def _report():
    del R.STATS[:]
    yield
    path = os.environ.get("G4C_ADJOINT_REF_REPORT")
    if path:
        worst, count = {}, {}
        for what, ratio in R.STATS:
            name = what.split(" @")[0]
            if name == "CONTROL":          # (a negative control the elementwise bound let through: rejected by the other check)
                continue
            worst[name], count[name] = max(worst.get(name, 0.0), ratio), count.get(name, 0) + 1
        with open(path, "w") as f:
            f.write("| check | cases | largest measured / allowed |\n|---|---|---|\n")
            for name in worst:
                f.write(f"| {name} | {count[name]} | {worst[name]:.3g} |\n")


@pytest.fixture(autouse=True)
def _grad():
    with torch.enable_grad():
        yield


def dev(t, grad=False):
    if t is None:
        return None
    t = t.to(DEV)
    return t.requires_grad_(True) if grad else t


def check(kind, got, ref, mag, n_eff, what):
    """Exact on integer cases, bounded on random ones."""
    if kind == "int":
        R.assert_exact(got, ref, what)
    else:
        R.assert_fp32_class(got, ref, mag, n_eff, what)


def rejected(kind, got, bad, n_eff):
    return R.rejects(R.assert_exact, got, bad[0]) if kind == "int" else R.rejects(R.assert_fp32_class, got, bad[0], bad[1], n_eff, "CONTROL")


def twice(fn, leaves, dout):
    """fn() -> output; backpropagates `dout` twice from fresh graphs and requires the same bits.  Returns (output, gradients)."""
    runs = []
    for _ in range(2):
        for t in leaves:
            t.grad = None
        out = fn()
        out.backward(dout)
        runs.append([t.grad.clone() for t in leaves])
    for a, b in zip(*runs):
        assert torch.equal(a, b), "two runs of the same backward differ"
    return out.detach(), runs[0]


def plus_zero(t):
    return bool((t == 0).all()) and not bool(torch.signbit(t).any())


def csr_of(c):
    return plan.build_csr(c["keys"], c["n_seg"] + (1 if c["drop"] else 0), DEV, drop_last_segment=c["drop"])


LAYOUT_CASES = [(257, 6, lay) for lay in K.LAYOUTS[1:]] + [(257, 128, lay) for lay in K.LAYOUTS[1:]] + [(1, 128, "broadcast"), (33, 1, "broadcast"),
                                                                                                         (33, 1, "transposed")]
SHAPE_CASES = [(r, w, "contiguous") for r in K.ROWS for w in K.WIDTHS] + LAYOUT_CASES


# ====================================================================== op by op
@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("rows,width,layout", SHAPE_CASES)
def test_gather_rows(rows, width, layout, kind):
    """_GatherRows (the gMuS restriction): forward = the rows themselves; adjoint = per row of x the sum over the positions that read
    it — n_eff = the multiplicity of the most-read row (added in order by one lane of g4c_segment_reduce)."""
    c = K.gather_case(rows, width, layout, kind)
    x, idx = dev(c["x"], True), dev(c["idx"])
    dout = K.as_layout(dev(c["dout"]), layout)
    out, (gx,) = twice(lambda: A.gather_rows(x, plan.index32(idx)), [x], dout)
    assert torch.equal(out, x.detach()[idx])
    ref, mag = R.gather_rows_adjoint(dev(c["dout"]), idx, c["n_x"])
    check(kind, gx, ref, mag, c["mult"], f"gather adjoint {kind} @ rows={rows} w={width} {layout}")
    unread = torch.bincount(idx, minlength=c["n_x"]) == 0
    assert int(unread.sum()) >= 0.1 * c["n_x"] and plus_zero(gx[unread])
    if (rows, width, layout) == (257, 6, "contiguous"):           # negative controls: a duplicate index counted once; one row dropped
        keep, once = R.dedup_index(idx)
        assert rejected(kind, gx, R.gather_rows_adjoint(dev(c["dout"])[keep], once, c["n_x"]), c["mult"])
        r = int((c["dout"].abs().sum(1) > 0).nonzero()[0])
        assert rejected(kind, gx, R.gather_rows_adjoint(R.drop_row(dev(c["dout"]), r), idx, c["n_x"]), c["mult"])


REDUCE_CASES = ([(n, w, p, "contiguous") for n in K.ROWS for w in K.WIDTHS for p in K.PLANS]
                + [(n, w, "permuted", lay) for n, w, lay in LAYOUT_CASES])


@pytest.mark.parametrize("mean", [False, True])
@pytest.mark.parametrize("n_seg,width,plan_kind,layout", REDUCE_CASES)
def test_segment_reduce_exact(n_seg, width, plan_kind, layout, mean):
    """_SegmentReduce on integer rows: sums of any length, means over segments of power-of-two length (the quotient and the adjoint's
    fp32 reciprocal are then exact); rows of no segment (dropped rows) get +0, empty segments give +0."""
    c = K.reduce_case(n_seg, width, plan_kind, layout, "int", mean)
    csr = csr_of(c)
    src = dev(c["src"], True)
    dout = K.as_layout(dev(c["dout"]), layout)
    out, (gs,) = twice(lambda: ops.segment_reduce(src, csr, mean), [src], dout)
    R.assert_exact(out, R.segment_reduce(src.detach(), csr.off, csr.perm, mean)[0], "segment_reduce")
    R.assert_exact(gs, R.segment_reduce_adjoint(dev(c["dout"]), src.detach(), out, csr.off, csr.perm, mean)[0], "segment_reduce adjoint")
    assert plus_zero(gs[dev(c["keys"]) >= n_seg]) and plus_zero(out[dev(torch.tensor(c["lens"])) == 0])
    if (n_seg, width, layout) == (257, 6, "contiguous"):
        s = next(i for i in range(2, n_seg - 2) if c["lens"][i] >= 2 and float((c["dout"][i] - c["dout"][i - 1]).abs().sum()) > 0)
        moved = R.move_boundary(csr.off, s)
        assert R.rejects(R.assert_exact, gs, R.segment_reduce_adjoint(dev(c["dout"]), src.detach(), out, moved, csr.perm, mean)[0])
        assert R.rejects(R.assert_exact, gs, R.segment_reduce_adjoint(dev(c["dout"]), src.detach(), out, csr.off, csr.perm, not mean)[0])
        assert R.rejects(R.assert_exact, gs, R.segment_reduce_adjoint(R.drop_row(dev(c["dout"]), s), src.detach(), out, csr.off, csr.perm, mean)[0])


@pytest.mark.parametrize("mean", [False, True])
@pytest.mark.parametrize("n_seg,width,plan_kind,layout", REDUCE_CASES)
def test_segment_reduce_bounded(n_seg, width, plan_kind, layout, mean):
    """_SegmentReduce with both activations (tanh behind, SELU on load) on random rows.  Forward: the segment's rows added in order
    (max_deg), the quotient, N_EFF_ACT per activation.  Adjoint: no sum — the two slope products (N_EFF_ACT each; the slopes from the
    fp32 rows the launch itself read and wrote) and for a mean the fp32 reciprocal and its product."""
    c = K.reduce_case(n_seg, width, plan_kind, layout, "float", mean)
    csr = csr_of(c)
    src = dev(c["src"], True)
    dout = K.as_layout(dev(c["dout"]), layout)
    out, (gs,) = twice(lambda: ops.segment_reduce(src, csr, mean, _lib.ACT_TANH, src_act=_lib.ACT_SELU), [src], dout)
    ref, mag = R.segment_reduce(src.detach(), csr.off, csr.perm, mean, "tanh", "selu")
    R.assert_fp32_class(out, ref, mag, R.n_eff_segment_reduce(c["max_deg"], mean, "tanh", "selu"), f"segment_reduce @ {n_seg}x{width} {plan_kind}")
    g, ga = R.segment_reduce_adjoint(dev(c["dout"]), src.detach(), out, csr.off, csr.perm, mean, "tanh", "selu")
    n_b = R.n_eff_segment_reduce_adjoint(mean, "tanh", "selu")
    R.assert_fp32_class(gs, g, ga, n_b, f"segment_reduce adjoint @ {n_seg}x{width} {plan_kind} {layout}")
    assert plus_zero(gs[dev(c["keys"]) >= n_seg])
    if (n_seg, width, layout) == (257, 6, "contiguous"):
        s = next(i for i in range(2, n_seg - 2) if c["lens"][i] >= 2 and float((c["dout"][i] - c["dout"][i - 1]).abs().sum()) > 0)
        bad = R.segment_reduce_adjoint(dev(c["dout"]), src.detach(), out, R.move_boundary(csr.off, s), csr.perm, mean, "tanh", "selu")
        assert rejected("float", gs, bad, n_b)
        bad = R.segment_reduce_adjoint(dev(c["dout"]), src.detach(), out, csr.off, csr.perm, not mean, "tanh", "selu")
        assert rejected("float", gs, bad, n_b)


@pytest.mark.parametrize("reduce", ["sum", "mean"])
@pytest.mark.parametrize("n_seg", [33, 4097])
def test_scatter_public(n_seg, reduce):
    """blocks.scatter(src, index, dim_size, reduce) under grad, index in any order: exact on integers."""
    c = K.reduce_case(n_seg, 6, "permuted", "contiguous", "int", reduce == "mean")
    src, index = dev(c["src"], True), dev(c["keys"])
    out, (gs,) = twice(lambda: B.scatter(src, index, dim_size=n_seg, reduce=reduce), [src], dev(c["dout"]))
    off, perm = K.host_csr(c["keys"], n_seg)
    R.assert_exact(out, R.segment_reduce(c["src"], off, perm, reduce == "mean")[0].to(DEV), "scatter")
    R.assert_exact(gs, R.segment_reduce_adjoint(c["dout"], c["src"], out.cpu(), off, perm, reduce == "mean")[0].to(DEV), "scatter adjoint")


@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("aggr", ["mean", "sum"])
@pytest.mark.parametrize("n_fine", [33, 257, 1031])
def test_pool_edge_public(n_fine, aggr, kind):
    """blocks.pool_edge under grad: the coarse edges in coalesce order, their features and the gradient of the fine features (zero for
    edges inside a cluster).  Integer means are exact on the segments whose length is a power of two; the others are bounded."""
    c = K.pool_case(n_fine, 128 if n_fine == 257 else 6, kind)
    ea, idx, ei = dev(c["edge_attr"], True), dev(c["idx"]), dev(c["edge_index"])
    coarse, off, perm = K.host_pool_plan(c["idx"], c["edge_index"])
    dvals = K.operand((off.numel() - 1, ea.size(1)), kind, K.gen("pool dout", n_fine))
    out, (ge,) = twice(lambda: B.pool_edge(idx, ei, ea, aggr)[1], [ea], dev(dvals))
    assert torch.equal(B.pool_edge(idx, ei, ea, aggr)[0].cpu(), coarse)
    mean = aggr == "mean"
    lens = off[1:] - off[:-1]
    ref, mag = R.pool_edge(c["edge_attr"], off, perm, mean)
    g, ga = R.pool_edge_adjoint(dvals, c["edge_attr"], off, perm, mean)
    if kind == "int":
        pow2 = ((lens & (lens - 1)) == 0) | (not mean)
        rows = torch.zeros(ea.size(0), dtype=torch.bool)
        rows[perm] = pow2[R._seg_ids(off)]
        inside = torch.ones(ea.size(0), dtype=torch.bool)
        inside[perm] = False
        assert int(pow2.sum()) > 1 and int(inside.sum()) > 0
        R.assert_exact(out.cpu()[pow2], ref[pow2], "pool_edge")
        R.assert_exact(ge.cpu()[rows], g[rows], "pool_edge adjoint")
        assert plus_zero(ge.cpu()[inside])
    else:
        R.assert_fp32_class(out.cpu(), ref, mag, R.n_eff_segment_reduce(int(lens.max()), mean), f"pool_edge @ {n_fine} {aggr}")
        R.assert_fp32_class(ge.cpu(), g, ga, R.n_eff_segment_reduce_adjoint(mean), f"pool_edge adjoint @ {n_fine} {aggr}")


WM_CASES = ([(n, k, 6, "contiguous") for n in K.ROWS for k in K.KS] + [(257, 5, w, "contiguous") for w in K.WIDTHS]
            + [(257, 5, 128, lay) for lay in K.LAYOUTS[1:]] + [(33, 3, 1, "broadcast")])


@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("n_seg,k,width,layout", WM_CASES)
def test_weighted_segment_mean(n_seg, k, width, layout, masked, kind):
    """_WeightedSegmentMean.  Unmasked through the public blocks.knn_interpolate; masked (`out_idx32` from plan.mask_index32, a strict
    subset of the output rows) through autograd.weighted_segment_mean with `n_out`, the form UpEdgeMP records.  Forward n_eff: k
    products and k additions of the numerator, k additions of the denominator, the quotient.  Adjoint: the coefficient (k + 1), its
    product, then the sum over the positions that read one row of x (its multiplicity, in order).  The coefficients themselves equal
    the sequential-order fp32 reference bit for bit."""
    c = K.wm_case(n_seg, k, width, kind, masked, layout)
    x, w = dev(c["x"], True), dev(c["w"])
    y_idx, x_idx = dev(c["y_idx"]), dev(c["x_idx"])
    dout = K.as_layout(dev(c["dout"]), layout)
    csr = plan.segments_of_sorted(y_idx)
    if masked:
        out_idx32 = plan.mask_index32(dev(c["mask"]))
        assert torch.equal(out_idx32.cpu().long(), c["out_idx"])
        fn = lambda: A.weighted_segment_mean(x, plan.index32(x_idx), w, csr, c["n_out"], out_idx32)          # noqa: E731
    else:
        fn = lambda: B.knn_interpolate(x, y_idx, x_idx, w)          # noqa: E731
    out, (gx,) = twice(fn, [x], dout)
    oi = dev(c["out_idx"])
    ref, mag = R.weighted_mean(x.detach(), x_idx, w, c["off"], c["n_out"], oi)
    check(kind, out, ref, mag, R.n_eff_weighted_mean(k), f"weighted mean {kind} @ n={n_seg} k={k} w={width} masked={masked}")
    g, ga = R.weighted_mean_adjoint(dev(c["dout"]), x_idx, w, c["off"], c["n_x"], oi)
    n_b = R.n_eff_weighted_mean_adjoint(k, c["mult"])
    check(kind, gx, g, ga, n_b, f"weighted mean adjoint {kind} @ n={n_seg} k={k} w={width} masked={masked} {layout}")
    assert torch.equal(A._segment_coefficients(w, csr).cpu(), R.segment_coefficients(c["w"], c["off"]))
    assert plus_zero(gx[torch.bincount(x_idx, minlength=c["n_x"]) == 0])
    if masked:
        assert plus_zero(out[~dev(c["mask"])])
    if masked and (n_seg, k, width, layout) == (257, 5, 6, "contiguous"):      # a masked row given gradient; a duplicate index counted once
        bad = R.weighted_mean_adjoint(dev(c["dout"]), x_idx, w, c["off"], c["n_x"], dev(R.unmask_row(c["out_idx"], c["n_out"])))
        assert rejected(kind, gx, bad, n_b)
        keep, _ = R.dedup_index(c["x_idx"])
        coef = R.segment_coefficients(c["w"], c["off"]).double()
        gone = torch.ones(c["x_idx"].numel(), dtype=torch.bool)
        gone[keep] = False
        coef[gone] = 0
        assert rejected(kind, gx, R.weighted_mean_adjoint(dev(c["dout"]), x_idx, w, c["off"], c["n_x"], oi, coef=coef), n_b)


PROJ_CASES = [(n, f, "contiguous") for n in K.ROWS for f in K.FEATS] + [(257, f, lay) for f in (3, 64) for lay in K.LAYOUTS[1:]]


@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("indexed", [False, True])
@pytest.mark.parametrize("n_edges,n_feat,layout", PROJ_CASES)
def test_project_to_edges(n_edges, n_feat, layout, indexed, kind):
    """_ProjectToEdges with and without node32.  Forward: two products and a sum, rounded separately (3).  Adjoint: one product per
    element, then through the index the sum over a node's edges in order (its multiplicity)."""
    c = K.proj_case(n_edges, n_feat, indexed, kind, layout)
    v, unit, node = dev(c["v"], True), dev(c["unit"]), dev(c["node"])
    node32 = None if node is None else plan.index32(node)
    dout = K.as_layout(dev(c["dout"]), layout)
    out, (gv,) = twice(lambda: ops.project_to_edges(v, node32, unit, n_edges, n_feat), [v], dout)
    ref, mag = R.project_to_edges(v.detach(), node, unit, n_feat)
    check(kind, out, ref, mag, R.N_EFF_PROJECT, f"project_to_edges {kind} @ E={n_edges} F={n_feat} indexed={indexed}")
    g, ga = R.project_to_edges_adjoint(dev(c["dout"]), node, unit, v.shape)
    n_b = R.n_eff_project_adjoint(c["mult"])
    check(kind, gv, g, ga, n_b, f"project_to_edges adjoint {kind} @ E={n_edges} F={n_feat} indexed={indexed} {layout}")
    if indexed:
        assert plus_zero(gv[torch.bincount(node, minlength=v.size(0)) == 0])
    if (n_edges, n_feat, layout) == (257, 3, "contiguous"):          # the two columns of every unit vector swapped; one edge dropped
        assert rejected(kind, gv, R.project_to_edges_adjoint(dev(c["dout"]), node, R.swap_unit_columns(unit), v.shape), n_b)
        assert rejected(kind, out, R.project_to_edges(v.detach(), node, R.swap_unit_columns(unit), n_feat), R.N_EFF_PROJECT)
        r = int((c["dout"].abs().sum(1) * c["unit"].abs().sum(1) > 0).nonzero()[0])
        assert rejected(kind, gv, R.project_to_edges_adjoint(R.drop_row(dev(c["dout"]), r), node, unit, v.shape), n_b)


E2N_CASES = [(n, f, k, "contiguous") for n in K.ROWS for f in K.FEATS for k in K.KS] + [(257, f, 5, lay) for f in (3, 64) for lay in K.LAYOUTS[1:]]


@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("n_nodes,n_feat,k,layout", E2N_CASES)
def test_edge_scalar_to_node_vector(n_nodes, n_feat, k, layout, kind):
    """_EdgeScalarToNodeVector through blocks.edgeScalarToNodeVector (F = 3: through ops.edge_scalar_to_node_vector).  Forward: k fused
    multiply-adds in order.  Adjoint: g4c_project_to_edges on (dout, the inverse's columns) — two products and a sum (3)."""
    c = K.e2n_case(n_nodes, n_feat, k, kind, layout)
    e, ui = dev(c["e"], True), dev(c["unit_inv"])
    dout = K.as_layout(dev(c["dout"]), layout)
    if n_feat == 3:
        fn = lambda: ops.edge_scalar_to_node_vector(e, ui, n_nodes, k)          # noqa: E731
    else:
        fn = lambda: B.edgeScalarToNodeVector(e, dev(c["edge_index"]), edgeUnitVectorInverse=ui)          # noqa: E731
    out, (ge,) = twice(fn, [e], dout)
    ref, mag = R.edge_scalar_to_node_vector(e.detach(), ui, k)
    check(kind, out, ref, mag, R.n_eff_e2n(k), f"edge_scalar_to_node_vector {kind} @ n={n_nodes} F={n_feat} k={k}")
    g, ga = R.edge_scalar_to_node_vector_adjoint(dev(c["dout"]), ui, k)
    check(kind, ge, g, ga, R.N_EFF_PROJECT, f"edge_scalar_to_node_vector adjoint {kind} @ n={n_nodes} F={n_feat} k={k} {layout}")
    if (n_nodes, n_feat, k, layout) == (257, 3, 5, "contiguous"):          # the two rows of every inverse swapped; one node's gradient dropped
        assert rejected(kind, ge, R.edge_scalar_to_node_vector_adjoint(dev(c["dout"]), ui.flip(1), k), R.N_EFF_PROJECT)
        r = int((c["dout"].abs().sum(1) > 0).nonzero()[0])
        assert rejected(kind, ge, R.edge_scalar_to_node_vector_adjoint(R.drop_row(dev(c["dout"]), r), ui, k), R.N_EFF_PROJECT) or not bool(c["unit_inv"][r].any())


# ====================================================================== the four places a boundary test decides
def test_knn_interpolate_refuses_out_idx32_under_grad():
    """ops.weighted_segment_mean with `out_idx32` and no `out`: the same ValueError with and without gradients (the rows the mask does
    not name have nowhere to be zero); the masked form with gradients is autograd.weighted_segment_mean(..., n_out, out_idx32)."""
    c = K.wm_case(33, 3, 6, "float", True)
    x, oi = dev(c["x"]), plan.mask_index32(dev(c["mask"]))
    args = (dev(c["y_idx"]), dev(c["x_idx"]), dev(c["w"]))
    with torch.no_grad():
        with pytest.raises(ValueError, match="out_idx32: scattered output rows need `out`"):
            B.knn_interpolate(x, *args, out_idx32=oi)
    with pytest.raises(ValueError, match="out_idx32: scattered output rows need `out`"):
        B.knn_interpolate(x.clone().requires_grad_(True), *args, out_idx32=oi)
    with pytest.raises(NotImplementedError):
        B.knn_interpolate(x.clone().requires_grad_(True), *args, out=torch.zeros(c["n_out"], 6, device=DEV), out_idx32=oi)


@pytest.mark.parametrize("extra", [3, 4])
@pytest.mark.parametrize("indexed", [False, True])
@pytest.mark.parametrize("kind", ["int", "float"])
def test_project_to_edges_gradient_has_the_shape_of_v(kind, indexed, extra):
    """A v with `extra` columns behind the 2 F the launch reads and two more rows than it reads: the gradient has v's shape, +0 behind
    what was read.  (extra = 3: an odd row stride, which the launch's 8-byte loads cannot take — the rows are copied first.)"""
    c = K.proj_case(257, 3, indexed, kind)
    g0 = K.gen("proj wide", kind, int(indexed), extra)
    wide = torch.cat([torch.cat([c["v"], K.operand((c["v"].size(0), extra), kind, g0)], 1), K.operand((2, 6 + extra), kind, g0)])
    v, unit, node = dev(wide, True), dev(c["unit"]), dev(c["node"])
    out, (gv,) = twice(lambda: ops.project_to_edges(v, None if node is None else plan.index32(node), unit, 257, 3), [v], dev(c["dout"]))
    check(kind, out, *R.project_to_edges(v.detach(), node, unit, 3), R.N_EFF_PROJECT, f"project_to_edges wide v {kind} @ indexed={indexed} extra={extra}")
    assert tuple(gv.shape) == tuple(wide.shape)
    g, ga = R.project_to_edges_adjoint(dev(c["dout"]), node, unit, wide.shape)
    check(kind, gv, g, ga, R.n_eff_project_adjoint(c["mult"]), f"project_to_edges adjoint wide v {kind} @ indexed={indexed} extra={extra}")
    assert plus_zero(gv[:, 6:]) and plus_zero(gv[-2:])


def test_row_broadcast_gradient_into_a_fused_mlp():
    """`_dense`: a gradient with strides (0, 1) — what stands behind `y.sum(0)` — gives every backward the bits of its materialised
    copy (the linear adjoints take that layout in their own tests above; this is _FusedMLP's)."""
    torch.manual_seed(11)
    mlp = B.MLP(6, (32, 32), True).to(DEV)
    x = torch.randn(257, 6, device=DEV, requires_grad=True)
    row = torch.randn(1, 32, device=DEV)
    grads = []
    for dy in (row.expand(257, 32), row.expand(257, 32).contiguous()):
        x.grad = None
        mlp.zero_grad()
        mlp.run([ops.Source(x)], 257).backward(dy)
        grads.append([x.grad.clone()] + [p.grad.clone() for p in mlp.parameters()])
    assert grads[0][0].abs().sum() > 0
    for a, b in zip(*grads):
        assert torch.equal(a, b)
    x.grad = None
    mlp.run([ops.Source(x)], 257).sum(0).sum().backward()           # autograd's own row-broadcast
    assert tuple(x.grad.shape) == (257, 6)


def test_segment_coefficients_take_no_atomics(monkeypatch):
    """The totals come from the fixed-order segmented sum on the plan: bit for bit the sequential reference at weights spanning 1e16,
    and no index_add_ (atomics on the device) on the way."""
    c = K.wm_case(4097, 8, 1, "float", False)
    w, csr = dev(c["w"]), plan.segments_of_sorted(dev(c["y_idx"]))

    def no_atomics(*a, **k):
        raise AssertionError("index_add_ on the way to the interpolation coefficients")
    monkeypatch.setattr(torch.Tensor, "index_add_", no_atomics)
    coef = A._segment_coefficients(w, csr)
    monkeypatch.undo()
    assert torch.equal(coef.cpu(), R.segment_coefficients(c["w"], c["off"]))
    assert coef.data_ptr() == A._segment_coefficients(w, csr).data_ptr()          # cached on the plan


# ====================================================================== block by block
class Trace:
    """The activations every _FusedMLP backward of a step really used: the operands of its weight-gradient and LayerNorm-adjoint
    calls (tests/test_gpu_train_ref.py), and the number of forwards that saved their activations."""

    def __init__(self, monkeypatch):
        self.saving, self.events = 0, []
        f0, w0, l0 = ops.mlp_forward, A.weight_bias_grad, A.layernorm_grad

        def fwd(*a, **k):
            self.saving += 1 if (k.get("save") is not None and k.get("mul") is None) else 0
            return f0(*a, **k)

        def wg(g, a, want_bias=True):
            self.events.append(("wg", a.detach().clone(), want_bias))
            return w0(g, a, want_bias)

        def lng(z, gamma, dy, eps):
            self.events.append(("ln", z.detach().clone()))
            return l0(z, gamma, dy, eps)

        monkeypatch.setattr(ops, "mlp_forward", fwd)
        monkeypatch.setattr(A, "weight_bias_grad", wg)
        monkeypatch.setattr(A, "layernorm_grad", lng)

    def backwards(self, L):
        """Per _FusedMLP backward with a LayerNorm, in execution order: (acts [None, a1 .. a_{L-1}], z_last)."""
        out = []
        for ev in self.events:
            if ev[0] == "ln":
                out.append({"z": ev[1], "wg": []})
            else:
                out[-1]["wg"].append(ev)
        return [([None] + [c["wg"][L - 2 - i][1].float() for i in range(L - 1)], c["z"].float()) for c in out]


CONFIGS = [(128, True, True), (128, True, False), (128, False, True), (128, False, False), (32, False, True)]      # (hidden, thresholds at 0, save)


def _configure(monkeypatch, zero, save):
    if zero:
        monkeypatch.setattr(A, "HOIST_MIN_ROWS", 0)
        monkeypatch.setattr(A, "FUSED_LINEAR_MIN_ROWS", 0)
    else:
        assert (A.HOIST_MIN_ROWS, A.FUSED_LINEAR_MIN_ROWS) == (32768, 65536)
    monkeypatch.setattr(A, "SAVE_ACTIVATIONS", save)
    return Trace(monkeypatch)


def _mlp_params(mlp):
    lins = mlp._linears()
    ln = mlp.MLP.layer_norm if hasattr(mlp.MLP, "layer_norm") else None
    return ([l.weight.detach() for l in lins], [l.bias.detach() for l in lins], None if ln is None else (ln.weight.detach(), ln.bias.detach()))


def _param_name(k):
    if k == "gamma":
        return "MLP.layer_norm.weight"
    if k == "beta":
        return "MLP.layer_norm.bias"
    return f"MLP.linear_{int(k[1:]) + 1}.{'weight' if k[0] == 'W' else 'bias'}"


def _check_grads(want, module, mlps, inputs, n_eff, block, case):
    """want: {"[pre.]W0" ..: (value, magnitude), input name: ...}; mlps: {"pre." or "": attribute name}; inputs: {name: leaf}."""
    params = dict(module.named_parameters())
    seen = 0
    for k, (val, mag) in want.items():
        pre, _, rest = k.rpartition(".")
        if rest[0] in "Wbg" and rest not in inputs:
            got = params[f"{mlps[pre + '.' if pre else '']}.{_param_name(rest)}"].grad
            R.assert_fp32_class(got, val, mag, n_eff, f"{block} parameter gradients @ {k} {case}")
            R.assert_rel_largest(got, val, f"{block} parameter gradients, of the largest entry @ {k} {case}")
            seen += 1
    assert seen == len(params)
    for name, leaf in inputs.items():
        R.assert_fp32_class(leaf.grad, *want[name], n_eff, f"{block} input gradients @ {name} {case}")
        R.assert_rel_largest(leaf.grad, want[name][0], f"{block} input gradients, of the largest entry @ {name} {case}")


def _out(got, ref, mag, n_eff, block, case):
    R.assert_fp32_class(got, ref, mag, n_eff, f"{block} @ {case}")
    R.assert_rel_largest(got, ref, f"{block}, of the largest entry @ {case}")


def _rejects(leaf, bad, n_eff):
    """A block-level negative control: rejected by the pair of checks.  (The elementwise bound alone lets some of them through — it
    exceeds the gradient itself on these blocks, grad_ref.assert_rel_largest — and is printed for the record.)"""
    print(f"  CONTROL rejected by the elementwise bound alone: {R.rejects(R.assert_fp32_class, leaf.grad, bad[0], bad[1], n_eff, 'CONTROL')}")
    return R.rejects(R.assert_rel_largest, leaf.grad, bad[0], "CONTROL")


def _latent(n, H, g):
    return torch.randn(n, H, generator=g).to(DEV).requires_grad_(True)


@pytest.fixture(scope="module")
def mus():
    return S.mus_graph(1500, levels=2, seed=3).to(DEV)


@pytest.fixture(scope="module")
def remus():
    return S.remus_graph(1500, k=5, seed=4).to(DEV)


@pytest.fixture(scope="module")
def mugs():
    return S.mugs_graph(2500, levels=2, seed=5).to(DEV)


@pytest.mark.parametrize("internal", [False, True])
@pytest.mark.parametrize("H,zero,save", CONFIGS)
def test_down_mp(mus, H, zero, save, internal, monkeypatch):
    """DownMP.forward, and DownMP.pool(..., tanh, e_pre_act=SELU, target_major=True) as the models record it: the pooled field, the
    pooled edge latents, and the gradients of field, e_12, edge_attr and every parameter.  n_eff: the MLP step, the cluster mean
    (largest cluster + 1) and its adjoint (2), tanh and its slope (N_EFF_ACT each); the edge part is a _SegmentReduce of its own."""
    tr = _configure(monkeypatch, zero, save)
    split, g = ops.mlp_precision(), K.gen("down_mp", H, int(internal))
    torch.manual_seed(21)
    blk = B.DownMP((2 + H, (H, H, H), True), 1).to(DEV)
    gr = mus.clone()
    n, E = gr.pos.size(0), gr.edge_index.size(1)
    field, ea = _latent(n, H, g), _latent(E, H, g)
    rel = gr.e_12.detach().clone().requires_grad_(True)
    gr.e_12 = rel
    act, pre = ("tanh", "selu") if internal else (None, None)
    if internal:
        pooled, ei_l, ea_l = blk.pool(gr, field, gr.edge_index, ea, torch.tanh, e_pre_act=_lib.ACT_SELU, target_major=True)
    else:
        gr.field, gr.edge_attr = field, ea
        out = blk.forward(gr)
        pooled, ei_l, ea_l = out.field, out.edge_index, out.edge_attr
    dp, de = torch.randn(pooled.shape, generator=g).to(DEV), torch.randn(ea_l.shape, generator=g).to(DEV)
    torch.autograd.backward([pooled, ea_l], [dp, de])
    assert tr.saving == (1 if save else 0)
    (own,) = tr.backwards(3)
    csr = plan.cluster_plan(mus.cluster_2, mus.mask_2)
    pp = plan.pool_edge_plan(mus.idx1_to_idx2, mus.edge_index, internal)
    assert torch.equal(ei_l, pp.edge_index)
    cluster, params = (csr.off, csr.perm), _mlp_params(blk.down_mlp)
    f, srcs, pre_act, mag = R.down_mp_forward(rel.detach(), field.detach(), cluster, params, split)
    n_pool = R.n_eff_segment_reduce(csr.max_deg, True, act)
    _out(pooled.detach(), R._act(pre_act, act), mag, f.n_fwd[-1] + R.N_EFF_LN_ROW + n_pool, "DownMP pooled field", f"H={H} internal={internal}")
    want = R.down_mp_adjoint(f, srcs, params, cluster, dp, pooled.detach(), act, own)
    n_eff = R.n_eff_mlp_grad(2 + H, 3, n, split, True, 1) + n_pool + R.n_eff_segment_reduce_adjoint(True, act)
    _check_grads(want, blk, {"": "down_mlp"}, {"rel": rel, "field": field}, n_eff, "DownMP", f"H={H} zero={zero} save={save} internal={internal}")
    if (H, zero, save) == (128, True, True):          # negative control: one fine node handed to the neighbouring cluster
        lens = (csr.off[1:] - csr.off[:-1]).tolist()
        s_ = next(i for i in range(1, len(lens) - 1) if lens[i] >= 2)
        bad = R.down_mp_adjoint(f, srcs, params, (R.move_boundary(csr.off, s_), csr.perm), dp, pooled.detach(), act, own)
        assert _rejects(field, bad["field"], n_eff)
    ref, mag = R.pool_edge(ea.detach(), pp.csr.off, pp.csr.perm, True, pre)
    R.assert_fp32_class(ea_l.detach(), ref, mag, R.n_eff_segment_reduce(pp.csr.max_deg, True, None, pre), f"DownMP pooled edge latents @ H={H} internal={internal}")
    R.assert_fp32_class(ea.grad, *R.pool_edge_adjoint(de, ea.detach(), pp.csr.off, pp.csr.perm, True, pre),
                        R.n_eff_segment_reduce_adjoint(True, None, pre), f"DownMP edge latents' gradient @ H={H} internal={internal}")


@pytest.mark.parametrize("internal", [False, True])
@pytest.mark.parametrize("H,zero,save", CONFIGS)
def test_up_mp(mus, H, zero, save, internal, monkeypatch):
    """UpMP.forward, and UpMP.unpool with tanh as the models record it: [-e_12 | field_2[parent] | field_1] -> up_mlp.  The gathered
    block's adjoint adds a parent's children in order (the largest cluster)."""
    tr = _configure(monkeypatch, zero, save)
    split, g = ops.mlp_precision(), K.gen("up_mp", H, int(internal))
    torch.manual_seed(22)
    blk = B.UpMP((2 + 2 * H, (H, H, H), True), 2).to(DEV)
    gr = mus.clone()
    n, n2 = gr.pos.size(0), gr.pos_2.size(0)
    lr, old = _latent(n2, H, g), _latent(n, H, g)
    rel = gr.e_12.detach().clone().requires_grad_(True)
    gr.e_12 = rel
    act = "tanh" if internal else None
    if internal:
        y = blk.unpool(gr, lr, old, activation=torch.tanh)
    else:
        gr.field = lr
        y = blk.forward(gr, old, gr.pos).field
    dy = torch.randn(y.shape, generator=g).to(DEV)
    y.backward(dy)
    assert tr.saving == (1 if save else 0)
    (own,) = tr.backwards(3)
    params = _mlp_params(blk.up_mlp)
    f, srcs = R.up_mp_forward(rel.detach(), lr.detach(), mus.idx1_to_idx2, old.detach(), params, act, split)
    _out(y.detach(), f.y, f.Y0, f.n_fwd[-1] + R.N_EFF_LN_ROW + R.N_EFF_ACT, "UpMP output", f"H={H} internal={internal}")
    want = R.up_mp_adjoint(f, srcs, params, dy, act, own, y_act=y.detach())
    n_eff = R.n_eff_mlp_grad(2 + 2 * H, 3, n, split, True, int(torch.bincount(mus.idx1_to_idx2).max()))
    _check_grads(want, blk, {"": "up_mlp"}, {"rel": rel, "field_lr": lr, "field_hr_old": old}, n_eff, "UpMP",
                 f"H={H} zero={zero} save={save} internal={internal}")
    if (H, zero, save) == (128, True, True):          # negative control: every coarse row counted for one of its children only
        parent = mus.idx1_to_idx2
        keep, once = R.dedup_index(parent)
        rows = R.up_mp_adjoint(f, [srcs[0], R.Src(lr.detach()[parent]), srcs[2]], params, dy, act, own, y_act=y.detach())["field_lr"]
        bad = tuple(torch.zeros(n2, H, dtype=F64, device=DEV).index_add_(0, once, t[keep]) for t in rows)
        assert _rejects(lr, bad, n_eff)


def _n_eff_mp(H, L, rows_msg, rows_upd, split, row, col):
    max_deg = int(max(torch.bincount(row).max(), torch.bincount(col).max()))
    return R.n_eff_mlp_grad(3 * H, L, rows_msg, split, True, max_deg) + R.n_eff_mlp_grad(2 * H, L, rows_upd, split, True, max_deg), max_deg


@pytest.mark.parametrize("internal", [False, True])
@pytest.mark.parametrize("H,zero,save", CONFIGS)
def test_edge_mp(remus, H, zero, save, internal, monkeypatch):
    """EdgeMP.forward, and EdgeMP.step(SELU, a_pre_act=SELU): (SELU(e'), raw a') from (e, raw a) — both outputs, the gradients of e, a
    and of both MLPs.  n_eff as for GNBlock (both MLP steps; the aggregation's max_deg is inside them), SELU's slope from the fp32 e'."""
    tr = _configure(monkeypatch, zero, save)
    split, g = ops.mlp_precision(), K.gen("edge_mp", H, int(internal))
    torch.manual_seed(23)
    blk = B.EdgeMP((3 * H, (H, H), True), (2 * H, (H, H), True)).to(DEV)
    ai = remus.angle_index
    e, a = _latent(remus.edge_index.size(1), H, g), _latent(ai.size(1), H, g)
    act, pre = ("selu", "selu") if internal else (None, None)
    e1, a1 = blk.step(e, a, ai, _lib.ACT_SELU, a_pre_act=_lib.ACT_SELU) if internal else blk.forward(e, a, ai)
    de, da = torch.randn(e1.shape, generator=g).to(DEV), torch.randn(a1.shape, generator=g).to(DEV)
    torch.autograd.backward([e1, a1], [de, da])
    assert tr.saving == (2 if save else 0)
    upd_own, msg_own = tr.backwards(2)
    pa, pe = _mlp_params(blk.angle_mlp), _mlp_params(blk.edge_mlp)
    fm, fu, ms, us = R.edge_mp_forward(e.detach(), a.detach(), ai[0], ai[1], pa, pe, e_pre_act=pre, act=act, split=split)
    n_eff, max_deg = _n_eff_mp(H, 2, ai.size(1), e.size(0), split, ai[0], ai[1])
    _out(a1.detach(), fm.y, fm.Y0, fm.n_fwd[-1] + R.N_EFF_LN_ROW + R.N_EFF_ACT, "EdgeMP a'", f"H={H} internal={internal}")
    _out(e1.detach(), fu.y, fu.Y0, fm.n_fwd[-1] + fu.n_fwd[-1] + 2 * R.N_EFF_LN_ROW + max_deg + 1 + 2 * R.N_EFF_ACT, "EdgeMP e'",
         f"H={H} internal={internal}")
    want = R.edge_mp_adjoint(fm, fu, ms, us, pa, pe, de, da, act, msg_own=msg_own, upd_own=upd_own, v_act=e1.detach())
    _check_grads(want, blk, {"msg.": "angle_mlp", "upd.": "edge_mlp"}, {"v": e, "e": a}, n_eff, "EdgeMP",
                 f"H={H} zero={zero} save={save} internal={internal}")
    if (H, zero, save) == (128, True, True):          # negative control: one row of a' passes no gradient
        bad = R.edge_mp_adjoint(fm, fu, ms, us, pa, pe, de, R.drop_row(da, 777), act, msg_own=msg_own, upd_own=upd_own, v_act=e1.detach())
        assert _rejects(a, bad["e"], n_eff)


@pytest.mark.parametrize("activation", [None, "selu"])
@pytest.mark.parametrize("H,zero,save", CONFIGS)
def test_down_edge_mp(remus, H, zero, save, activation, monkeypatch):
    """DownEdgeMP.forward (senders e1[row], receivers e2[col]; "selu": the activation the model passes): e2' and the gradients of e1,
    e2, a12 and of both MLPs."""
    tr = _configure(monkeypatch, zero, save)
    split, g = ops.mlp_precision(), K.gen("down_edge_mp", H, str(activation))
    torch.manual_seed(24)
    blk = B.DownEdgeMP((3 * H, (H, H), True), (2 * H, (H, H), True)).to(DEV)
    ai = remus.angle_index12
    e1, e2, a12 = _latent(remus.edge_index.size(1), H, g), _latent(remus.edge_index2.size(1), H, g), _latent(ai.size(1), H, g)
    y = blk.forward(e1, e2, a12, ai, activation=activation)
    dy = torch.randn(y.shape, generator=g).to(DEV)
    y.backward(dy)
    assert tr.saving == (2 if save else 0)
    upd_own, msg_own = tr.backwards(2)
    pa, pe = _mlp_params(blk.angle_mlp), _mlp_params(blk.edge_mlp)
    fm, fu, ms, us = R.down_edge_mp_forward(e1.detach(), e2.detach(), a12.detach(), ai[0], ai[1], pa, pe, activation, split)
    n_eff, max_deg = _n_eff_mp(H, 2, ai.size(1), e2.size(0), split, ai[0], ai[1])
    _out(y.detach(), fu.y, fu.Y0, fm.n_fwd[-1] + fu.n_fwd[-1] + 2 * R.N_EFF_LN_ROW + max_deg + 1 + R.N_EFF_ACT, "DownEdgeMP e2'",
         f"H={H} act={activation}")
    want = R.down_edge_mp_adjoint(fm, fu, ms, us, pa, pe, dy, activation, msg_own=msg_own, upd_own=upd_own, v_act=y.detach())
    _check_grads(want, blk, {"msg.": "angle_mlp", "upd.": "edge_mlp"}, {"e1": e1, "e2": e2, "a12": a12}, n_eff, "DownEdgeMP",
                 f"H={H} zero={zero} save={save} act={activation}")


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("H,zero,save", CONFIGS)
def test_up_edge_mp(remus, H, zero, save, masked, monkeypatch):
    """UpEdgeMP.forward without coarse_mask1 (level 2 -> 1: every node is a target) and with it (level 3 -> 2: the targets are the
    level-2 nodes among all, the other rows of the interpolated tensor stay 0 and pass nothing): the output and the gradients of
    edge_attr1, edge_attr2 and the MLP.  n_eff: the MLP step plus the three helpers, forward (k, 3 k + 1, 3) and adjoint (1 + k edges
    of a node; k + 2 + the most-read coarse node; 3)."""
    tr = _configure(monkeypatch, zero, save)
    split, g = ops.mlp_precision(), K.gen("up_edge_mp", H, int(masked))
    torch.manual_seed(25)
    blk = B.UpEdgeMP((2 * H, (H, H, H), True)).to(DEV)
    gr, k = remus, 5
    if masked:
        ei_hi, ei_lo, ui, cm_hi, unit, cm_lo = gr.edge_index3, gr.edge_index2, gr.edgeUnitVectorInverse3, gr.coarse_mask3, gr.edgeUnitVector2, gr.coarse_mask2
        y_idx, x_idx, wt = gr.y_idx_32, gr.x_idx_32, gr.weights_32
    else:
        ei_hi, ei_lo, ui, cm_hi, unit, cm_lo = gr.edge_index2, gr.edge_index, gr.edgeUnitVectorInverse2, gr.coarse_mask2, gr.edgeUnitVector, None
        y_idx, x_idx, wt = gr.y_idx_21, gr.x_idx_21, gr.weights_21
    ea_hi, ea_lo = _latent(ei_hi.size(1), H, g), _latent(ei_lo.size(1), H, g)
    y = blk.forward(gr.pos, y_idx, x_idx, wt, ea_hi, ei_hi, ui, cm_hi, ea_lo, ei_lo, unit, cm_lo)
    dy = torch.randn(y.shape, generator=g).to(DEV)
    y.backward(dy)
    assert tr.saving == (1 if save else 0)
    (own,) = tr.backwards(3)
    params = _mlp_params(blk.up_mlp)
    n_total = gr.pos.size(0)
    off = torch.arange(int(y_idx.max()) + 2, device=DEV) * k
    out_idx = cm_lo.nonzero().reshape(-1) if masked else None
    assert (not masked) or 0 < out_idx.numel() < n_total
    args = (ui, k, x_idx, wt, off, n_total, out_idx, ei_lo[1], unit)
    f, srcs = R.up_edge_mp_forward(ea_hi.detach(), *args, ea_lo.detach(), params, None, split)
    n_fwd = R.n_eff_e2n(k) + R.n_eff_weighted_mean(k) + R.N_EFF_PROJECT
    _out(y.detach(), f.y, f.Y0, f.n_fwd[-1] + R.N_EFF_LN_ROW + n_fwd, "UpEdgeMP output", f"H={H} masked={masked}")
    want = R.up_edge_mp_adjoint(f, srcs, params, dy, *args, None, own)
    mult = int(torch.bincount(x_idx).max())
    n_eff = (R.n_eff_mlp_grad(2 * H, 3, ei_lo.size(1), split, True, 1) + n_fwd + R.n_eff_project_adjoint(int(torch.bincount(ei_lo[1]).max()))
             + R.n_eff_weighted_mean_adjoint(k, mult) + R.N_EFF_PROJECT)
    _check_grads(want, blk, {"": "up_mlp"}, {"edge_attr1": ea_lo, "edge_attr2": ea_hi}, n_eff, "UpEdgeMP", f"H={H} zero={zero} save={save} masked={masked}")
    if (H, zero, save) == (128, True, True):          # negative control: the two columns of every fine unit vector swapped
        bad_args = args[:-1] + (R.swap_unit_columns(unit),)
        bad = R.up_edge_mp_adjoint(f, srcs, params, dy, *bad_args, None, own)
        assert _rejects(ea_hi, bad["edge_attr2"], n_eff)


@pytest.mark.parametrize("kind", ["int", "float"])
def test_mugs_restriction_and_interpolation(mugs, kind):
    """The gMuS pieces on the graph's own plans: the down-sampling's row gather (plan.restricted_level + autograd.gather_rows — every
    kept row is read once, the others never: exact in both kinds) and the up-sampling's knn_interpolate with the graph's weights."""
    H, g = 128, K.gen("mugs", kind)
    n = mugs.pos.size(0)
    keep32, _ = plan.restricted_level(mugs.coarse_mask2, mugs.edge_index2, None)
    v = dev(K.operand((n, H), kind, g), True)
    dv = dev(K.operand((keep32.numel(), H), kind, g))
    out, (gv,) = twice(lambda: A.gather_rows(v, keep32), [v], dv)
    assert torch.equal(out, v.detach()[mugs.coarse_mask2])
    R.assert_exact(gv, R.gather_rows_adjoint(dv, keep32, n)[0], "gMuS restriction adjoint")
    assert plus_zero(gv[~mugs.coarse_mask2]) and 0.1 * n <= keep32.numel() < n
    vc = dev(K.operand((keep32.numel(), H), "float", g), True)
    du = dev(K.operand((n, H), "float", g))
    up, (gc,) = twice(lambda: B.knn_interpolate(vc, mugs.y_idx_21, mugs.x_idx_21, mugs.weights_21), [vc], du)
    k = 6
    off = torch.arange(n + 1, device=DEV) * k
    R.assert_fp32_class(up, *R.weighted_mean(vc.detach(), mugs.x_idx_21, mugs.weights_21, off), R.n_eff_weighted_mean(k), "gMuS interpolation @ graph")
    mult = int(torch.bincount(mugs.x_idx_21).max())
    R.assert_fp32_class(gc, *R.weighted_mean_adjoint(du, mugs.x_idx_21, mugs.weights_21, off, keep32.numel()),
                        R.n_eff_weighted_mean_adjoint(k, mult), "gMuS interpolation adjoint @ graph")
