"""Argument checks of the helper-launch wrappers in graphs4cfd_amd/ops.py, on CPU tensors: every malformed call raises the stated
exception (TypeError for a dtype, ValueError for a shape, the message naming the argument) before anything reaches the library, and
the same call well-formed gets past validation and stops at require_hip's "no CPU fallback" RuntimeError — which proves validation
accepted it without launching anything.  No call here can reach a kernel: every tensor lives on the host."""
import pytest
import torch

from graphs4cfd_amd import _lib, ops, plan

F32, I32, I64 = torch.float32, torch.int32, torch.int64
SELU = _lib.ACT_SELU


def f(*shape):
    return torch.zeros(*shape, dtype=F32)


def i32(n):
    return torch.zeros(n, dtype=I32)


def csr(n=10, n_seg=4, perm=False, off=None):
    perm = i32(n) if perm is True else (None if perm is False else perm)
    return plan.CsrPlan(perm=perm, off=i32(n_seg + 1) if off is None else off, n=n, n_seg=n_seg, max_deg=3)


# (wrapper, well-formed arguments, {argument to replace: (bad value, exception, word the message must hold)})
def _cases():
    C = []

    def add(name, fn, good, bad):
        for label, (patch, exc, word) in bad.items():
            C.append(pytest.param(fn, good, patch, exc, word, id=f"{name}-{label}"))
        C.append(pytest.param(fn, good, {}, None, None, id=f"{name}-wellformed"))

    add("segment_reduce", lambda src, csr, out=None, act=0, src_act=0: ops.segment_reduce(src, csr, True, act, out, src_act),
        dict(src=f(10, 8), csr=csr(), out=f(4, 8)), {
            "src-f64": (dict(src=f(10, 8).double()), TypeError, "src"),
            "src-3d": (dict(src=f(10, 8, 1)), ValueError, "src"),
            "src-short": (dict(src=f(9, 8)), ValueError, "src"),
            "src-empty-perm": (dict(src=f(0, 8), csr=csr(perm=True)), ValueError, "src"),
            "off-i64": (dict(csr=csr(off=torch.zeros(5, dtype=I64))), TypeError, "off"),
            "off-short": (dict(csr=csr(off=i32(4))), ValueError, "off"),
            "perm-i64": (dict(csr=csr(perm=torch.zeros(10, dtype=I64))), TypeError, "perm"),
            "perm-short": (dict(csr=csr(perm=i32(9))), ValueError, "perm"),
            "out-rows": (dict(out=f(3, 8)), ValueError, "out"),
            "out-cols": (dict(out=f(4, 12)), ValueError, "out"),
            "out-f16": (dict(out=f(4, 8).half()), TypeError, "out"),
            "out-colstride": (dict(out=f(8, 4).t()), ValueError, "out"),
            "act": (dict(act=3), ValueError, "act"),
            "src_act": (dict(src_act=-1), ValueError, "src_act"),
        })
    add("weighted_segment_mean", ops.weighted_segment_mean,
        dict(x=f(6, 8), x_idx32=i32(10), w=f(10), csr=csr(), out=f(7, 8), out_idx32=i32(4)), {
            "x-f64": (dict(x=f(6, 8).double()), TypeError, "x"),
            "x-empty": (dict(x=f(0, 8)), ValueError, "x"),
            "idx-i64": (dict(x_idx32=torch.zeros(10, dtype=I64)), TypeError, "x_idx32"),
            "idx-short": (dict(x_idx32=i32(9)), ValueError, "x_idx32"),
            "idx-none": (dict(x_idx32=None), TypeError, "x_idx32"),
            "w-short": (dict(w=f(9)), ValueError, "w"),
            "w-f64": (dict(w=f(10).double()), TypeError, "w"),
            "out_idx-i64": (dict(out_idx32=torch.zeros(4, dtype=I64)), TypeError, "out_idx32"),
            "out_idx-short": (dict(out_idx32=i32(3)), ValueError, "out_idx32"),
            "out-cols": (dict(out=f(7, 9)), ValueError, "out"),
            "out-f64": (dict(out=f(7, 8).double()), TypeError, "out"),
            "out-rows-no-idx": (dict(out=f(3, 8), out_idx32=None), ValueError, "out"),
            "out_idx-without-out": (dict(out=None), ValueError, "out"),
            "off-short": (dict(csr=csr(off=i32(4))), ValueError, "off"),
        })
    add("project_to_edges", ops.project_to_edges,
        dict(v=f(5, 8), node32=i32(9), unit=f(9, 2), n_edges=9, n_feat=3), {
            "v-f64": (dict(v=f(5, 8).double()), TypeError, "v"),
            "v-narrow": (dict(n_feat=5), ValueError, "v"),
            "v-short-direct": (dict(node32=None), ValueError, "v"),
            "node-i64": (dict(node32=torch.zeros(9, dtype=I64)), TypeError, "node32"),
            "node-short": (dict(node32=i32(8)), ValueError, "node32"),
            "unit-rows": (dict(unit=f(8, 2)), ValueError, "edgeUnitVector"),
            "unit-cols": (dict(unit=f(9, 3)), ValueError, "edgeUnitVector"),
            "unit-f64": (dict(unit=f(9, 2).double()), TypeError, "edgeUnitVector"),
            "n_feat-0": (dict(n_feat=0), ValueError, "n_feat"),
        })
    add("edge_scalar_to_node_vector", ops.edge_scalar_to_node_vector,
        dict(e=f(12, 3), unit_inv=f(4, 2, 3), n_nodes=4, k=3, out=f(4, 6)), {
            "e-f64": (dict(e=f(12, 3).double()), TypeError, "edge_attr"),
            "e-rows": (dict(e=f(11, 3)), ValueError, "edge_attr"),
            "unit_inv-short": (dict(unit_inv=f(4, 2, 2)), ValueError, "edgeUnitVectorInverse"),
            "unit_inv-f64": (dict(unit_inv=f(4, 2, 3).double()), TypeError, "edgeUnitVectorInverse"),
            "out-shape": (dict(out=f(4, 3)), ValueError, "out"),
            "out-f64": (dict(out=f(4, 6).double()), TypeError, "out"),
            "k-0": (dict(k=0), ValueError, "k"),
        })
    add("copy_cols", ops.copy_cols,
        dict(src=f(6, 8), dst=f(5, 10), dcol0=2, scol0=1, width=7, idx32=i32(5), n_rows=5), {
            "src-f64": (dict(src=f(6, 8).double()), TypeError, "src"),
            "dst-f16": (dict(dst=f(5, 10).half()), TypeError, "dst"),
            "src-colstride": (dict(src=f(8, 6).t()), ValueError, "src"),
            "dst-colstride": (dict(dst=f(10, 5).t()), ValueError, "dst"),
            "src-window": (dict(scol0=2), ValueError, "scol0"),
            "dst-window": (dict(dcol0=4), ValueError, "dcol0"),
            "idx-i64": (dict(idx32=torch.zeros(5, dtype=I64)), TypeError, "idx32"),
            "idx-short": (dict(idx32=i32(4)), ValueError, "idx32"),
            "n_rows-dst": (dict(n_rows=6, idx32=i32(6)), ValueError, "n_rows"),
            "src-short-direct": (dict(idx32=None, src=f(4, 8)), ValueError, "src"),
            "width-0": (dict(width=0), ValueError, "width"),
        })
    add("add_cols", ops.add_cols,
        dict(a=f(5, 9), a_col0=6, b=f(5, 3), out=f(5, 3)), {
            "a-f64": (dict(a=f(5, 9).double()), TypeError, "a"),
            "b-f64": (dict(b=f(5, 3).double()), TypeError, "b"),
            "out-f64": (dict(out=f(5, 3).double()), TypeError, "out"),
            "a-short": (dict(a=f(4, 9)), ValueError, "a"),
            "a-window": (dict(a_col0=7), ValueError, "a_col0"),
            "a-colstride": (dict(a=f(9, 5).t()), ValueError, "a"),
            "b-colstride": (dict(b=f(3, 5).t()), ValueError, "b"),
            "out-rows": (dict(out=f(4, 3)), ValueError, "out"),
            "out-cols": (dict(out=f(5, 4)), ValueError, "out"),
            "out-colstride": (dict(out=f(3, 5).t()), ValueError, "out"),
        })
    add("activation_", ops.activation_, dict(x=f(7, 3), act=SELU), {
        "x-f64": (dict(x=f(7, 3).double()), TypeError, "x"),
        "x-i32": (dict(x=i32(7)), TypeError, "x"),
        "x-strided": (dict(x=f(7, 6)[:, :3]), ValueError, "x"),
        "act": (dict(act=5), ValueError, "act"),
    })
    add("layer_norm", ops.layer_norm, dict(x=f(5, 130), gamma=f(130), beta=f(130), eps=1e-5, act=0, out=f(5, 130)), {
        "x-f64": (dict(x=f(5, 130).double()), TypeError, "x"),
        "gamma-short": (dict(gamma=f(129)), ValueError, "gamma"),
        "beta-long": (dict(beta=f(131)), ValueError, "beta"),
        "gamma-f64": (dict(gamma=f(130).double()), TypeError, "gamma"),
        "beta-2d": (dict(beta=f(1, 130)), ValueError, "beta"),
        "gamma-strided": (dict(gamma=f(260)[::2]), ValueError, "gamma"),
        "out-rows": (dict(out=f(4, 130)), ValueError, "out"),
        "out-cols": (dict(out=f(5, 128)), ValueError, "out"),
        "out-f16": (dict(out=f(5, 130).half()), TypeError, "out"),
        "out-colstride": (dict(out=f(130, 5).t()), ValueError, "out"),
        "act": (dict(act=9), ValueError, "act"),
    })
    for layout, outputs in (("rows", f(6, 12)), ("steps", f(4, 6, 3))):
        add(f"rollout_advance[{layout}]", ops.rollout_advance,
            dict(field=f(6, 7), pred=f(6, 3), outputs=outputs, step=i32(2), nf=3), {
                "field-f64": (dict(field=f(6, 7).double()), TypeError, "field"),
                "pred-f64": (dict(pred=f(6, 3).double()), TypeError, "pred"),
                "outputs-f64": (dict(outputs=outputs.double()), TypeError, "outputs"),
                "field-strided": (dict(field=f(6, 8)[:, :7]), ValueError, "field"),
                "pred-rows": (dict(pred=f(5, 3)), ValueError, "pred"),
                "pred-cols": (dict(pred=f(6, 2)), ValueError, "pred"),
                "field-narrow": (dict(field=f(6, 2)), ValueError, "field"),
                "step-i64": (dict(step=torch.zeros(2, dtype=I64)), TypeError, "step"),
                "step-short": (dict(step=i32(1)), ValueError, "step"),
                "outputs-nodes": (dict(outputs=f(5, 12) if layout == "rows" else f(4, 5, 3)), ValueError, "outputs"),
                "outputs-narrow": (dict(outputs=f(6, 2) if layout == "rows" else f(4, 6, 2)), ValueError, "outputs"),
                "outputs-1d": (dict(outputs=f(72)), ValueError, "outputs"),
            })
    # the caller's row tensors of the two launches that otherwise allocate them: checked before anything else of the call is looked at
    # (the packed MLPs live on the device; nothing here gets as far as reading them)
    add("mp_layer_forward", lambda e_out=None, agg_out=None, store_rows=True: ops.mp_layer_forward(
            None, [ops.Source(f(10, 128))], 10, csr(), True, None, f(4, 128), 0, store_rows=store_rows, e_out=e_out, agg_out=agg_out),
        dict(e_out=f(10, 128), agg_out=f(4, 128)), {
            "e_out-f64": (dict(e_out=f(10, 128).double()), TypeError, "e_out"),
            "e_out-list": (dict(e_out=[0.0]), TypeError, "e_out"),
            "e_out-3d": (dict(e_out=f(10, 128, 1)), ValueError, "e_out"),
            "e_out-rows": (dict(e_out=f(9, 128)), ValueError, "e_out"),
            "e_out-cols": (dict(e_out=f(10, 136)), ValueError, "e_out"),
            "e_out-colstride": (dict(e_out=f(128, 10).t()), ValueError, "e_out"),
            "e_out-not-stored": (dict(store_rows=False), ValueError, "e_out"),
            "agg_out-bf16": (dict(agg_out=f(4, 128).bfloat16()), TypeError, "agg_out"),
            "agg_out-rows": (dict(agg_out=f(3, 128)), ValueError, "agg_out"),
            "agg_out-cols": (dict(agg_out=f(4, 64)), ValueError, "agg_out"),
            "agg_out-colstride": (dict(agg_out=f(128, 4).t()), ValueError, "agg_out"),
            "agg_out-1d": (dict(agg_out=f(512)), ValueError, "agg_out"),
        })
    add("mp_layer_forward[window]", lambda e_out, agg_out: ops.mp_layer_forward(
            None, [ops.Source(f(10, 128))], 10, csr(), True, None, f(4, 128), 0, e_out=e_out, agg_out=agg_out),
        dict(e_out=f(12, 144)[1:11, 8:136], agg_out=f(6, 144)[1:5, 8:136]), {
            "e_out-rows-overlap": (dict(e_out=f(10, 128).as_strided((10, 128), (64, 1))), ValueError, "e_out"),
        })
    add("mlp_forward_precomputed", lambda out=None, store_rows=True: ops.mlp_forward_precomputed(
            None, f(10, 128), [], 10, (csr(), f(4, 128), True), store_rows=store_rows, out=out),
        dict(out=f(10, 128)), {
            "out-f64": (dict(out=f(10, 128).double()), TypeError, "out"),
            "out-none-tensor": (dict(out=(1, 2)), TypeError, "out"),
            "out-3d": (dict(out=f(10, 128, 1)), ValueError, "out"),
            "out-rows": (dict(out=f(9, 128)), ValueError, "out"),
            "out-cols": (dict(out=f(10, 120)), ValueError, "out"),
            "out-colstride": (dict(out=f(128, 10).t()), ValueError, "out"),
            "out-not-stored": (dict(store_rows=False), ValueError, "out"),
        })
    return C


@pytest.mark.parametrize("fn,good,patch,exc,word", _cases())
def test_wrapper_validates_before_the_library(fn, good, patch, exc, word):
    kw = dict(good, **patch)
    assert all(not t.is_cuda for t in kw.values() if torch.is_tensor(t))          # (nothing here may reach a kernel)
    if exc is None:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(**kw)
        return
    with pytest.raises(exc) as info:
        fn(**kw)
    assert type(info.value) is exc, f"{type(info.value).__name__}: {info.value}"
    assert word in str(info.value), str(info.value)
    assert "no CPU fallback" not in str(info.value)
