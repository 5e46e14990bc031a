"""Thin Python wrappers over the C-ABI of libg4c.so: argument checking, output allocation
(torch is used for device memory and the current HIP stream only), one launch per call.
Nothing here computes on the host or with torch ops."""
from __future__ import annotations

import contextlib
import ctypes as C
import math
import os
from typing import List, Optional, Sequence, Tuple

import torch

from . import _lib
from ._args import Args, record_scratch_doubles
from .plan import CsrPlan

Tensor = torch.Tensor


class KernelTimer:
    """Optional per-launch timing with HIP events on the launch stream (bench.py's roofline leg).
    `with KernelTimer() as kt: ...` brackets every g4c_mlp_run / g4c_segment_reduce launch with an
    event pair and records its algorithmic work; `kt.summary()` after a device sync."""
    active = None

    def __init__(self):
        self.records = []   # (kind, flops, bytes, start_event, end_event)

    def __enter__(self):
        KernelTimer.active = self
        return self

    def __exit__(self, *exc):
        KernelTimer.active = None
        return False

    def launch(self, kind: str, flops: float, nbytes: float, fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        if kind.startswith("mlp_"):
            # the library picks the kernel family per launch (arithmetic, shape, row count): label the record by what ran
            kind = _lib.KERNEL_NAMES.get(int(_lib.load().g4c_mlp_last_kernel()), kind)
        self.records.append((kind, flops, nbytes, a, b))
        return out

    def summary(self):
        out = {}
        for kind, flops, nbytes, a, b in self.records:
            d = out.setdefault(kind, {"launches": 0, "seconds": 0.0, "flops": 0.0, "bytes": 0.0})
            d["launches"] += 1
            d["seconds"] += a.elapsed_time(b) * 1e-3
            d["flops"] += flops
            d["bytes"] += nbytes
        return out


def _timed(kind: str, flops: float, nbytes: float, fn):
    kt = KernelTimer.active
    return fn() if kt is None else kt.launch(kind, flops, nbytes, fn)


class StaticCache:
    """Results of launches whose inputs cannot change between the steps of one rollout (reference: nn/model.py:316-320 — `solve`
    only ever replaces `graph.field`): `selu(edge_encoder(edge_attr))` of the MuS-GNN models (nn/mus_gnn.py:73,178 of the reference)
    and REMuS-GNN's five angle encoders (nn/remus_gnn.py:136-140), and — an entry of its own beside the edge latents — the product
    `b1 + W1e e0` of the first MP layer's first edge-MLP layer with them (nn/blocks.py static_first_layer: that layer's message launch
    then starts from it, mlp_forward_precomputed).  A `Rollout` / `DistributedRollout` activates its cache around
    every step; the first (eager) step fills it, the captured step finds the entries and therefore contains neither the launches
    nor the tensors in its write set.  A bare `model.forward()` has no active cache and recomputes, like the reference.

    An entry is valid for one (weights epoch, arithmetic, identity + version + shape of every input tensor): an in-place edit of
    `edge_attr`, new weights or `set_mlp_precision` recompute it — the same bits either way, the cached tensor is what the launch
    would have produced again."""
    active: Optional["StaticCache"] = None

    def __init__(self):
        self.store = {}
        self.hits = self.misses = 0
        self._prev = None

    def __enter__(self):
        self._prev, StaticCache.active = StaticCache.active, self
        # entries of another arithmetic go: what the step still uses is computed again under the current one (a miss either way), and
        # an entry the step no longer asks for — the first MP layer's product after a rollout has fallen back to bf16x6 — would
        # otherwise read as stale before every step, and the step would never be captured again
        prec = mlp_precision()
        for name in [n for n, hit in self.store.items() if hit[0][1] != prec]:
            del self.store[name]
        return self

    def __exit__(self, *exc):
        StaticCache.active = self._prev
        return False

    def get(self, name: str, inputs: Sequence[Tensor], fn):
        key = (weights_epoch(), mlp_precision()) + tuple((t.data_ptr(), t._version, tuple(t.shape), t.dtype) for t in inputs)
        hit = self.store.get(name)
        global _last_bounds
        if hit is not None and hit[0] == key:
            self.hits += 1
            _last_bounds = hit[3]          # (what take_bounds() would have answered behind the launch: same weights epoch, same inputs)
            return hit[1]
        self.misses += 1
        val = fn()
        self.store[name] = (key, val, tuple(inputs), _last_bounds)      # (the inputs are kept alive: the key holds their addresses)
        return val

    def stale(self) -> bool:
        """True when an entry no longer matches what it was computed from (an in-place edit of a static input, new weights, another
        arithmetic).  A captured step contains neither the cached launches nor a look-up, so a rollout asks this before every replay
        and falls back to one eager step (which recomputes the entry) + a new capture — ADVICE r04: a replay must not keep reading
        latents of an `edge_attr` that was edited since."""
        head = (weights_epoch(), mlp_precision())
        for key, _, inputs, _ in self.store.values():
            if key != head + tuple((t.data_ptr(), t._version, tuple(t.shape), t.dtype) for t in inputs):
                return True
        return False


def static_launch(name: str, inputs: Sequence[Tensor], fn):
    """`fn()` — or its cached result when a rollout's StaticCache is active (never while a call is recorded for autograd)."""
    c = StaticCache.active
    return fn() if (c is None or torch.is_grad_enabled()) else c.get(name, inputs, fn)


def _f32_2d(t: Tensor, name: str) -> Tensor:
    if t.dtype != torch.float32:
        raise TypeError(f"{name}: expected float32, got {t.dtype}")
    if t.dim() != 2:
        raise ValueError(f"{name}: expected a 2-D tensor, got shape {tuple(t.shape)}")
    if t.stride(1) != 1 and t.size(1) > 1:
        t = t.contiguous()
    if t.size(0) > 1 and t.stride(0) < t.size(1):
        t = t.contiguous()
    return t


def _bf16_2d(t: Tensor) -> Tensor:
    if t.dim() != 2 or t.stride(1) != 1:
        raise ValueError(f"bf16 source: expected a 2-D tensor with unit column stride, got shape {tuple(t.shape)}")
    return t


def _ld(t: Tensor) -> int:
    return int(t.stride(0)) if t.size(0) > 1 else int(max(t.size(1), t.stride(0)))


class Source:
    """One column block of a virtually concatenated MLP input."""

    __slots__ = ("tensor", "index", "col0", "width", "negate", "pre_act", "additive", "segments", "seg_mean", "bound")

    def __init__(self, tensor: Tensor, index: Optional[Tensor] = None, col0: int = 0, width: Optional[int] = None,
                 negate: bool = False, pre_act: int = _lib.ACT_NONE, additive: bool = False,
                 segments: Optional[CsrPlan] = None, seg_mean: bool = True, bound: Optional[float] = None):
        # (bf16 rows: the message tensors a fused-aggregation launch stored in the rounded-bf16 mode, mlp_forward(rows_dtype=);
        # only as a plain 128-wide block of a launch in that mode — the C entry point checks)
        self.tensor = _bf16_2d(tensor) if tensor.dtype == torch.bfloat16 else _f32_2d(tensor, "source")
        self.index = index          # int32 gather index or None
        self.col0 = col0
        self.width = int(self.tensor.size(1) - col0 if width is None else width)
        self.negate = negate        # folded into the packed weights
        self.pre_act = pre_act      # activation applied while loading (producer stored the raw tensor)
        self.additive = additive    # already multiplied by its block of the first layer: gathered and added, not multiplied
        # aggregation on load (bf16x6 kernels): row r of the block = sum / mean of the tensor's rows in segment r of this
        # CSR plan (through its permutation, if any; `pre_act` then applies to the rows before they are added), i.e.
        # scatter(pre_act(tensor), col, reduce) without materialising it
        self.segments = segments
        self.seg_mean = seg_mean
        # proven bound on |value| of the STORED rows (before `pre_act`), or None = unknown.  Set only by the code that has just launched
        # the producer of `tensor`, from that launch's weights (take_bounds); it belongs to this use of the tensor, not to the tensor —
        # nothing survives an in-place edit or a slice that way.  A tensor a user hands in has none, and its launches are range-tracked.
        self.bound = bound
        if segments is not None and (index is not None or additive or self.width != 128):
            raise ValueError("aggregation on load needs a 128-wide block without gather index")

    def whole_block(self, width: int, pre_acts: Optional[Sequence[int]] = (_lib.ACT_NONE,), dtypes: Optional[Sequence[torch.dtype]] = None,
                    product: bool = False) -> bool:
        """A whole, plain block of `width` columns: from column 0, not negated, not aggregated on load, read row for row and multiplied
        by its weights (`product=True`: gathered and added instead).  `pre_acts` / `dtypes`: what the caller's kernel admits, None: any."""
        return (self.width == width and self.col0 == 0 and not self.negate and self.segments is None
                and bool(self.additive) == product and (self.index is not None) == product
                and (pre_acts is None or self.pre_act in pre_acts) and (dtypes is None or self.tensor.dtype in dtypes))


def vector_rows(t: Tensor, col0: int = 0) -> bool:
    """Rows a 16-byte vector store (or load) can address from column `col0` on: unit column stride, a 16-byte aligned first element, a
    row stride of whole 16-byte pieces (8 bf16 values, 4 fp32 values)."""
    return t.stride(1) == 1 and (t.data_ptr() + t.element_size() * col0) % 16 == 0 and _ld(t) % (16 // t.element_size()) == 0


# ---- argument checks of the helper launches below: shapes, strides and dtypes only (host metadata — never index VALUES, which would
# synchronise the stream and break graph capture), and before require_hip, so that a malformed call is refused the same way with or
# without a device.  The checks themselves live in _args.py (`Args`): a wrapper says what it expects of each argument, in the order it
# blames them, and adds no check of its own that `Args` already has (DESIGN.md §5 "The wrapper checks").  A wrong dtype is a
# TypeError in the wrappers down to rollout_* and in snapshot_*, a ValueError in the mesh_* / body_forces* / sample_* / tracer_advance /
# voronoi_cells / weighted_integrals family (`Args(what, TypeError)` / `Args(what)`); a wrong shape is a ValueError everywhere; the
# message names the argument first.  The three helpers below are the row-matrix, index and vector forms of the first group, whose
# messages carry no function name.
_plain = Args(None, TypeError)


def _rows_f32(t: Tensor, name: str, cols: Optional[int] = None, min_rows: int = 0, min_cols: int = 0) -> Tensor:
    """A float32 [rows, cols] tensor the launch addresses as t[r * ld + c]: unit column stride, rows that do not overlap."""
    _plain.strided_rows(t, name, cols=cols, min_cols=min_cols)
    if int(t.size(0)) < min_rows:
        raise ValueError(f"{name}: expected at least {min_rows} rows, got shape {tuple(t.shape)}")
    return t


def _index_i32(t: Optional[Tensor], name: str, n: Optional[int] = None, at_least: Optional[int] = None) -> Optional[Tensor]:
    """An int32 index vector (contiguous, 1-D) of exactly `n` / at least `at_least` entries; None passes."""
    if t is None:
        return None
    _plain.tensor(t, name, torch.int32, dim=1)
    if n is not None and t.numel() != n:
        raise ValueError(f"{name}: expected {n} entries, got {t.numel()}")
    if at_least is not None and t.numel() < at_least:
        raise ValueError(f"{name}: expected at least {at_least} entries, got {t.numel()}")
    return t


def _vector_f32(t: Optional[Tensor], name: str, n: int) -> Optional[Tensor]:
    if t is not None:
        _plain.tensor(t, name, torch.float32, shape=(n,))
    return t


def _act_arg(act, name: str) -> int:
    if act not in (_lib.ACT_NONE, _lib.ACT_SELU, _lib.ACT_TANH):
        raise ValueError(f"{name}: unknown activation code {act!r}")
    return int(act)


def _csr_arg(csr: CsrPlan, name: str) -> None:
    if csr.n < 0 or csr.n_seg < 0:
        raise ValueError(f"{name}: negative sizes n={csr.n} n_seg={csr.n_seg}")
    _index_i32(csr.off, f"{name}.off", n=csr.n_seg + 1)
    _index_i32(csr.perm, f"{name}.perm", at_least=csr.n)


def segment_reduce(src: Tensor, csr: CsrPlan, mean: bool, act: int = _lib.ACT_NONE, out: Optional[Tensor] = None,
                   src_act: int = _lib.ACT_NONE) -> Tensor:
    """out[s] = act(sum|mean of src_act(src[perm[p]]) over the plan's segments) (g4c_segment_reduce)."""
    if torch.is_grad_enabled() and src.requires_grad:
        if out is not None:
            raise NotImplementedError("segment_reduce(out=...) is not differentiable")
        from . import autograd as _ag
        return _ag.segment_reduce(src, csr, mean, act, src_act)
    src = _f32_2d(src, "src")
    width = int(src.size(1))
    _csr_arg(csr, "csr")
    act, src_act = _act_arg(act, "act"), _act_arg(src_act, "src_act")
    if csr.perm is None and int(src.size(0)) < csr.n:          # (through a permutation the rows it names cannot be checked here)
        raise ValueError(f"src: the plan reads rows 0 .. {csr.n - 1}, got shape {tuple(src.shape)}")
    if csr.perm is not None and csr.n > 0 and int(src.size(0)) == 0:
        raise ValueError(f"src: the plan reads {csr.n} rows through its permutation, got shape {tuple(src.shape)}")
    if out is not None:
        _rows_f32(out, "out", cols=width, min_rows=csr.n_seg)
    lib = _lib.load()
    dev = _lib.require_hip(src, csr.off, csr.perm, out)
    if out is None:
        out = torch.empty((csr.n_seg, width), dtype=torch.float32, device=dev)
    # algorithmic bytes: messages read + rows written + offsets (+ permutation)
    nbytes = 4.0 * (csr.n * width + csr.n_seg * width + csr.n_seg + 1 + (csr.n if csr.perm is not None else 0))
    _timed("segment_reduce", 0.0, nbytes, lambda: _lib.check(lib.g4c_segment_reduce(
        _lib.ptr(src), _ld(src), _lib.ptr(csr.perm), _lib.ptr(csr.off), csr.n_seg, width,
        1 if mean else 0, src_act, act, _lib.ptr(out), _ld(out), _lib.stream_handle(dev))))
    return out


def activation_(x: Tensor, act: int) -> Tensor:
    """In-place activation of a contiguous tensor (g4c_activation_inplace)."""
    Args("activation_", TypeError).tensor(x, "x", torch.float32)
    act = _act_arg(act, "act")
    lib = _lib.load()
    dev = _lib.require_hip(x)
    _lib.check(lib.g4c_activation_inplace(_lib.ptr(x), x.numel(), act, _lib.stream_handle(dev)))
    return x


def weighted_segment_mean(x: Tensor, x_idx32: Tensor, w: Tensor, csr: CsrPlan, out: Optional[Tensor] = None,
                          out_idx32: Optional[Tensor] = None) -> Tensor:
    if torch.is_grad_enabled() and x.requires_grad:
        if out is not None:
            raise NotImplementedError("weighted_segment_mean(out=...) is not differentiable (autograd.weighted_segment_mean "
                                      "returns the full tensor)")
        if out_idx32 is not None:         # (as without gradients: there is no `out` here whose rows it could name)
            raise ValueError("out_idx32: scattered output rows need `out`")
        from . import autograd as _ag
        return _ag.weighted_segment_mean(x, x_idx32, w, csr)
    x = _f32_2d(x, "x")
    width = int(x.size(1))
    _plain.dtype(w, "w", torch.float32)
    w = w.reshape(-1).contiguous()
    _csr_arg(csr, "csr")
    if csr.perm is not None:
        raise NotImplementedError("knn_interpolate needs y_idx sorted (the BuildKnnInterpWeights layout)")
    if x_idx32 is None:
        raise TypeError("x_idx32: expected an int32 tensor, got None")
    _index_i32(x_idx32, "x_idx32", n=csr.n)
    if w.numel() != csr.n:
        raise ValueError(f"w: expected {csr.n} weights (one per entry of x_idx32), got {w.numel()}")
    if csr.n > 0 and int(x.size(0)) == 0:
        raise ValueError(f"x: x_idx32 reads {csr.n} rows, got shape {tuple(x.shape)}")
    _index_i32(out_idx32, "out_idx32", n=csr.n_seg)
    if out is not None:       # (the rows out_idx32 names cannot be checked here; without it the launch writes rows 0 .. n_seg - 1)
        _rows_f32(out, "out", cols=width, min_rows=csr.n_seg if out_idx32 is None else min(csr.n_seg, 1))
    elif out_idx32 is not None:
        raise ValueError("out_idx32: scattered output rows need `out`")
    lib = _lib.load()
    dev = _lib.require_hip(x, x_idx32, w, csr.off, out, out_idx32)
    if out is None:
        out = torch.empty((csr.n_seg, width), dtype=torch.float32, device=dev)
    _lib.check(lib.g4c_weighted_segment_mean(_lib.ptr(x), _ld(x), _lib.ptr(x_idx32), _lib.ptr(w), _lib.ptr(csr.off),
                                             csr.n_seg, width, _lib.ptr(out), _ld(out), _lib.ptr(out_idx32),
                                             _lib.stream_handle(dev)))
    return out


def project_to_edges(v: Tensor, node32: Optional[Tensor], unit: Tensor, n_edges: int, n_feat: int) -> Tensor:
    if torch.is_grad_enabled() and v.requires_grad:
        from . import autograd as _ag
        return _ag.project_to_edges(v, node32, unit, n_edges, n_feat)
    v = _f32_2d(v, "v")
    unit = _f32_2d(unit, "edgeUnitVector").contiguous()
    n_edges, n_feat = int(n_edges), int(n_feat)
    if n_edges < 0 or n_feat <= 0:
        raise ValueError(f"n_edges / n_feat: expected n_edges >= 0 and n_feat > 0, got {n_edges}, {n_feat}")
    if int(v.size(1)) < 2 * n_feat:
        raise ValueError(f"v: {n_feat} features need {2 * n_feat} columns, got shape {tuple(v.shape)}")
    if tuple(unit.shape) != (n_edges, 2):
        raise ValueError(f"edgeUnitVector: expected shape ({n_edges}, 2), got {tuple(unit.shape)}")
    _index_i32(node32, "node32", n=n_edges)
    if node32 is None and int(v.size(0)) < n_edges:
        raise ValueError(f"v: without node32 edge e reads row e, {n_edges} edges, got shape {tuple(v.shape)}")
    if node32 is not None and n_edges > 0 and int(v.size(0)) == 0:
        raise ValueError(f"v: node32 reads {n_edges} rows, got shape {tuple(v.shape)}")
    if _ld(v) % 2 or v.data_ptr() % 8:          # (the launch reads (x, y) pairs as 8-byte loads: an odd row stride, a window at an odd column)
        v = v[:, :2 * n_feat].contiguous()
    lib = _lib.load()
    dev = _lib.require_hip(v, node32, unit)
    out = torch.empty((n_edges, n_feat), dtype=torch.float32, device=dev)
    _lib.check(lib.g4c_project_to_edges(_lib.ptr(v), _ld(v), _lib.ptr(node32), _lib.ptr(unit), n_edges, n_feat,
                                        _lib.ptr(out), _ld(out), _lib.stream_handle(dev)))
    return out


def edge_scalar_to_node_vector(e: Tensor, unit_inv: Tensor, n_nodes: int, k: int, out: Optional[Tensor] = None) -> Tensor:
    if torch.is_grad_enabled() and e.requires_grad:
        if out is not None:
            raise NotImplementedError("edge_scalar_to_node_vector(out=...) is not differentiable")
        from . import autograd as _ag
        return _ag.edge_scalar_to_node_vector(e, unit_inv, n_nodes, k)
    e = _f32_2d(e, "edge_attr")
    n_nodes, k = int(n_nodes), int(k)
    if n_nodes < 0 or k <= 0:
        raise ValueError(f"n_nodes / k: expected n_nodes >= 0 and k > 0, got {n_nodes}, {k}")
    _plain.dtype(unit_inv, "edgeUnitVectorInverse", torch.float32)
    if unit_inv.numel() != n_nodes * 2 * k:
        raise ValueError(f"edgeUnitVectorInverse: expected {n_nodes} x 2 x {k} entries, got shape {tuple(unit_inv.shape)}")
    unit_inv = unit_inv.contiguous()
    n_feat = int(e.size(1))
    if int(e.size(0)) != n_nodes * k:
        raise ValueError(f"edge_attr: {int(e.size(0))} edges cannot be viewed as {n_nodes} nodes x {k} incoming edges")
    if out is not None:
        _plain.dtype(out, "out", torch.float32)
        if tuple(out.shape) != (n_nodes, 2 * n_feat) or out.stride(1) != 1:
            raise ValueError(f"out must be a float32 [{n_nodes}, {2 * n_feat}] tensor with unit column stride")
    lib = _lib.load()
    dev = _lib.require_hip(e, unit_inv, out)
    if out is None:
        out = torch.empty((n_nodes, 2 * n_feat), dtype=torch.float32, device=dev)
    _lib.check(lib.g4c_edge_scalar_to_node_vector(_lib.ptr(e), _ld(e), _lib.ptr(unit_inv), k, n_nodes, n_feat,
                                                  _lib.ptr(out), _ld(out), _lib.stream_handle(dev)))
    return out


def copy_cols(src: Tensor, dst: Tensor, dcol0: int, scol0: int = 0, width: Optional[int] = None,
              idx32: Optional[Tensor] = None, n_rows: Optional[int] = None) -> None:
    _rows_f32(src, "src")
    _rows_f32(dst, "dst")
    dcol0, scol0 = int(dcol0), int(scol0)
    width = int(src.size(1) - scol0 if width is None else width)
    n_rows = int(dst.size(0) if n_rows is None else n_rows)
    if width <= 0 or scol0 < 0 or scol0 + width > int(src.size(1)):
        raise ValueError(f"scol0 / width: columns {scol0} .. {scol0 + width - 1} of src with shape {tuple(src.shape)}")
    if dcol0 < 0 or dcol0 + width > int(dst.size(1)):
        raise ValueError(f"dcol0 / width: columns {dcol0} .. {dcol0 + width - 1} of dst with shape {tuple(dst.shape)}")
    if n_rows < 0 or n_rows > int(dst.size(0)):
        raise ValueError(f"n_rows: {n_rows} rows of dst with shape {tuple(dst.shape)}")
    _index_i32(idx32, "idx32", at_least=n_rows)
    if idx32 is None and int(src.size(0)) < n_rows:
        raise ValueError(f"src: {n_rows} rows are copied, got shape {tuple(src.shape)}")
    if idx32 is not None and n_rows > 0 and int(src.size(0)) == 0:
        raise ValueError(f"src: idx32 reads {n_rows} rows, got shape {tuple(src.shape)}")
    lib = _lib.load()
    dev = _lib.require_hip(src, dst, idx32)
    _lib.check(lib.g4c_copy_cols(_lib.ptr(src), _ld(src), scol0, _lib.ptr(idx32), _lib.ptr(dst), _ld(dst), dcol0, width,
                                 n_rows, _lib.stream_handle(dev)))


def add_cols(a: Tensor, a_col0: int, b: Tensor, out: Tensor) -> Tensor:
    """out = a[:, a_col0:a_col0+w] + b (g4c_add_cols)."""
    _rows_f32(b, "b", min_cols=1)
    n_rows, width, a_col0 = int(b.size(0)), int(b.size(1)), int(a_col0)
    _rows_f32(a, "a", min_rows=n_rows)
    if a_col0 < 0 or a_col0 + width > int(a.size(1)):
        raise ValueError(f"a_col0: columns {a_col0} .. {a_col0 + width - 1} of a with shape {tuple(a.shape)}")
    _rows_f32(out, "out", cols=width, min_rows=n_rows)
    lib = _lib.load()
    dev = _lib.require_hip(a, b, out)
    _lib.check(lib.g4c_add_cols(_lib.ptr(a), _ld(a), a_col0, _lib.ptr(b), _ld(b), _lib.ptr(out), _ld(out),
                                width, n_rows, _lib.stream_handle(dev)))
    return out


def layer_norm(x: Tensor, gamma: Optional[Tensor], beta: Optional[Tensor], eps: float, act: int = _lib.ACT_NONE,
               out: Optional[Tensor] = None) -> Tensor:
    """Row-wise LayerNorm (+ activation) over any width (g4c_layer_norm): the fused MLP kernels' own epilogue covers <= 128 columns."""
    x = _f32_2d(x, "x")
    n_rows, width = int(x.size(0)), int(x.size(1))
    if width <= 0:
        raise ValueError(f"x: expected at least one column, got shape {tuple(x.shape)}")
    _vector_f32(gamma, "gamma", width)
    _vector_f32(beta, "beta", width)
    act = _act_arg(act, "act")
    if out is not None:
        _rows_f32(out, "out", cols=width)
        if int(out.size(0)) != n_rows:
            raise ValueError(f"out: expected shape ({n_rows}, {width}), got {tuple(out.shape)}")
    lib = _lib.load()
    dev = _lib.require_hip(x, gamma, beta, out)
    if out is None:
        out = torch.empty((n_rows, width), dtype=torch.float32, device=dev)
    _lib.check(lib.g4c_layer_norm(_lib.ptr(x), _ld(x), n_rows, width, _lib.ptr(gamma), _lib.ptr(beta), float(eps), act,
                                  _lib.ptr(out), _ld(out), _lib.stream_handle(dev)))
    return out


def rollout_advance(field: Tensor, pred: Tensor, outputs: Tensor, step: Tensor, nf: int) -> None:
    nf = int(nf)
    a = Args("rollout_advance", TypeError)
    for t, name in ((field, "field"), (pred, "pred"), (outputs, "outputs")):
        a.tensor(t, name, torch.float32)
    a.step_index(step, entries=2)          # ([step index, the launch's ticket counter (zero)])
    if field.dim() != 2 or nf <= 0 or int(field.size(1)) < nf:
        raise ValueError(f"field: expected [n_nodes, >= nf = {nf}], got shape {tuple(field.shape)}")
    n_nodes = int(field.size(0))
    if tuple(pred.shape) != (n_nodes, nf):
        raise ValueError(f"pred: expected shape ({n_nodes}, {nf}), got {tuple(pred.shape)}")
    if outputs.dim() == 3:          # step-major [steps, n_nodes, nf]: a step writes one contiguous block
        if outputs.size(1) != n_nodes or outputs.size(2) != nf:
            raise ValueError(f"outputs: rollout_advance: step-major outputs {tuple(outputs.shape)} for {n_nodes} nodes x {nf} fields")
        out_ld = 0
    elif outputs.dim() == 2:        # row-major [n_nodes, nf * steps] (the reference's layout); the step index lives on the device
        if int(outputs.size(0)) != n_nodes or int(outputs.size(1)) < nf:
            raise ValueError(f"outputs: expected row-major [{n_nodes}, >= {nf}], got shape {tuple(outputs.shape)}")
        out_ld = int(outputs.size(1))
    else:
        raise ValueError(f"outputs: expected [n_nodes, nf * steps] or [steps, n_nodes, nf], got shape {tuple(outputs.shape)}")
    lib = _lib.load()
    dev = _lib.require_hip(field, pred, outputs, step)
    _lib.check(lib.g4c_rollout_advance(_lib.ptr(field), int(field.size(1)), _lib.ptr(pred), nf, _lib.ptr(outputs),
                                       out_ld, _lib.ptr(step), n_nodes, _lib.stream_handle(dev)))


def _scratch_doubles(fn: str, n_nodes: int, count: int) -> int:
    """The library's own size (g4c_*_scratch_doubles) of a step-record scratch: a header and one partial set per workgroup."""
    n = int(getattr(_lib.load(), fn)(int(n_nodes), int(count)))
    if n < 0:
        _lib.check(n)
    return n


def rollout_record_scratch(n_nodes: int, nf: int, device) -> Tensor:
    """The `scratch` buffer of rollout_advance_record's statistics for a mesh of n_nodes and nf fields (the size is the library's:
    g4c_rollout_record_scratch_doubles)."""
    return torch.zeros(_scratch_doubles("g4c_rollout_record_scratch_doubles", n_nodes, nf), dtype=torch.float64, device=device)


def rollout_advance_record(field: Tensor, pred: Tensor, step: Tensor, nf: int, max_steps: int, *, snap: Optional[Tensor] = None,
                           every: int = 0, probe_rows: Optional[Tensor] = None, probe_out: Optional[Tensor] = None,
                           target: Optional[Tensor] = None, mask: Optional[Tensor] = None, stats: Optional[Tensor] = None,
                           scratch: Optional[Tensor] = None) -> None:
    """g4c_rollout_advance_record: rollout_advance's shift of `field` and bump of `step`, and the records of step t = step[0] (read on
    the device; nothing for t >= max_steps):
    snap [n_snap, N, nf] with every = k > 0: steps k - 1, 2k - 1, ... in slots 0, 1, ...;
    probe_out [max_steps, P, nf]: pred's rows probe_rows (int32 [P]; their values are never read here);
    stats float64 [max_steps, nf, _lib.REC_NSTAT]: the error sums against target[:, nf t : nf (t + 1)] (target: [N, >= nf max_steps],
    unit stride along its columns, any row stride), Σ|d| also over the rows of `mask` (uint8 / bool [N]); `scratch` comes from
    rollout_record_scratch."""
    nf, max_steps, every = int(nf), int(max_steps), int(every)
    what = "rollout_advance_record"
    a = Args(what, TypeError)
    a.tensor(field, "field", torch.float32)
    a.tensor(pred, "pred", torch.float32)
    a.step_index(step, entries=2)          # ([step index, the launch's ticket counter (zero)])
    if field.dim() != 2 or nf <= 0 or int(field.size(1)) < nf:
        raise ValueError(f"field: expected [n_nodes, >= nf = {nf}], got shape {tuple(field.shape)}")
    n_nodes = int(field.size(0))
    if tuple(pred.shape) != (n_nodes, nf):
        raise ValueError(f"pred: expected shape ({n_nodes}, {nf}), got {tuple(pred.shape)}")
    a.at_least(max_steps, "max_steps", 0)
    a.lattice(every, max_steps, snap, "snap", "snapshot")
    if snap is not None:
        a.tensor(snap, "snap", torch.float32)
        if snap.dim() != 3 or tuple(snap.shape[1:]) != (n_nodes, nf):
            raise ValueError(f"snap: {what}: expected [n_snap, {n_nodes}, {nf}], got {tuple(snap.shape)}")
    if (probe_rows is None) != (probe_out is None):
        raise ValueError(f"probe_{'out' if probe_out is None else 'rows'}: {what}: probe_rows and probe_out come together")
    n_probe = 0
    if probe_rows is not None:
        a.tensor(probe_rows, "probe_rows", torch.int32, dim=1)
        n_probe = int(probe_rows.numel())
        a.tensor(probe_out, "probe_out", torch.float32, shape=(max_steps, n_probe, nf))
    target_ld = 0
    if target is None:
        for t, name in ((mask, "mask"), (stats, "stats"), (scratch, "scratch")):
            if t is not None:
                raise ValueError(f"{name}: {what}: given without a target")
    else:
        _, _, target_ld = a.strided_rows(target, "target", rows=n_nodes, min_cols=nf * max_steps)
        if mask is not None:
            a.tensor(mask, "mask", (torch.uint8, torch.bool), shape=(n_nodes,))
        if stats is None or scratch is None:
            raise ValueError(f"{'stats' if stats is None else 'scratch'}: {what}: a target needs stats and scratch")
        a.tensor(stats, "stats", torch.float64, shape=(max_steps, nf, _lib.REC_NSTAT))
        a.tensor(scratch, "scratch", torch.float64, dim=1)
    lib = _lib.load()
    dev = _lib.require_hip(field, pred, step, snap, probe_rows, probe_out, target, mask, stats, scratch)
    if target is not None:
        need = _scratch_doubles("g4c_rollout_record_scratch_doubles", n_nodes, nf)
        if int(scratch.numel()) < need:
            raise ValueError(f"scratch: {what}: {need} doubles for {n_nodes} nodes x {nf} fields, got {int(scratch.numel())}")
    rec = _lib.g4c_rollout_rec_t(max_steps=max_steps, snap=_lib.ptr(snap), every=every, n_snap=0 if snap is None else int(snap.size(0)),
                                 probe_rows=_lib.ptr(probe_rows), n_probe=n_probe, probe_out=_lib.ptr(probe_out),
                                 target=_lib.ptr(target), target_ld=target_ld, mask=_lib.ptr(mask), stats=_lib.ptr(stats),
                                 scratch=_lib.ptr(scratch))
    _lib.check(lib.g4c_rollout_advance_record(_lib.ptr(field), int(field.size(1)), _lib.ptr(pred), nf, C.byref(rec),
                                              _lib.ptr(step), n_nodes, _lib.stream_handle(dev)))


def moment_pairs(nf: int) -> int:
    """Planes of `sum2`: the pairs f <= g of nf fields, in the order (0,0), (0,1), ..., (0,nf-1), (1,1), ..."""
    return nf * (nf + 1) // 2


def rollout_moments(pred: Tensor, step: Tensor, nf: int, max_steps: int, window: Tensor, pivot: Tensor, sum: Tensor, sum2: Tensor,
                    lo: Tensor, hi: Tensor, *, stride: int = 1, sub: Optional[Tensor] = None) -> None:
    """g4c_rollout_moments: accumulate step t = step[0] (read on the device) into the per-node time statistics when t is on the window
    — 0 <= t < max_steps, t >= origin = window[0] (int32 [2] on the device: {origin, last}), (t - origin) % stride == 0 — and leave
    window[1] = t; any other step touches nothing.  The sample is pred [N, nf], or pred - sub[:, nf t : nf (t + 1)] with `sub`
    (float32 [N, >= nf max_steps], unit stride along its columns).  pivot / sum / lo / hi: float64 [nf, N], sum2 float64
    [moment_pairs(nf), N], unit stride along the nodes and one common plane stride >= N (views of padded buffers are fine).  `step`
    is not written: the step's closing launch (rollout_advance / rollout_advance_record) bumps it afterwards."""
    nf, max_steps, stride = int(nf), int(max_steps), int(stride)
    what = "rollout_moments"
    a = Args(what, TypeError)
    a.dtype(pred, "pred", torch.float32)
    if nf <= 0 or pred.dim() != 2 or int(pred.size(1)) != nf or not pred.is_contiguous():
        raise ValueError(f"pred: {what}: expected a contiguous [n_nodes, nf = {nf}], got shape {tuple(pred.shape)} strides {tuple(pred.stride())}")
    n_nodes = int(pred.size(0))
    a.step_index(step, entries=2)
    a.step_index(window, "window", entries=2)
    a.at_least(max_steps, "max_steps", 0)
    a.at_least(stride, "stride", 1)
    plane_ld = a.planes_f64(n_nodes, ("pivot", pivot, nf), ("sum", sum, nf), ("sum2", sum2, moment_pairs(nf)), ("lo", lo, nf), ("hi", hi, nf))
    sub_ld = 0
    if sub is not None:
        _, _, sub_ld = a.strided_rows(sub, "sub", rows=n_nodes, min_cols=nf * max_steps)
    lib = _lib.load()
    dev = _lib.require_hip(pred, step, window, pivot, sum, sum2, lo, hi, sub)
    m = _lib.g4c_rollout_moments_t(max_steps=max_steps, stride=stride, window=_lib.ptr(window), sub=_lib.ptr(sub), sub_ld=sub_ld,
                                   plane_ld=plane_ld, pivot=_lib.ptr(pivot), sum=_lib.ptr(sum),
                                   sum2=_lib.ptr(sum2), lo=_lib.ptr(lo), hi=_lib.ptr(hi))
    _lib.check(lib.g4c_rollout_moments(_lib.ptr(pred), nf, C.byref(m), _lib.ptr(step), n_nodes, _lib.stream_handle(dev)))


def spectrum_planes(nf: int, K: int) -> int:
    """Planes of one spectrum's accumulators: pivot and sum (nf each), re and im (nf K each, plane f K + k)."""
    return 2 * nf + 2 * nf * K


def spectrum_table(*, bins=None, freqs=None, samples: int, stride: int = 1, dt: float = 1.0, taper: str = "rect"):
    """The twiddle table g4c_rollout_spectrum multiplies by, built on the host in numpy fp64 (the kernel calls no sin / cos):
    (tw [samples, K, 2], w [samples], freqs [K]), fp64 CPU tensors.  Row j, bin k of `tw` is (w_j cos th_jk, -w_j sin th_jk) with
    th_jk = 2 pi * (phase fraction of sample j at frequency k).  Exactly one of `bins` and `freqs` names the K frequencies:
    bins — integers 0 <= b <= samples // 2, the frequency b / (samples stride dt), the fraction in exact integer arithmetic,
    ((b j) mod samples) / samples; freqs — cycles per unit of time, 0 <= f dt stride <= 0.5 (above is aliasing), the fraction
    fmod(f dt stride j, 1).  `stride` is the number of steps and `dt` the time of one step between two samples' steps.
    taper: "rect" (w_j = 1) or "hann" (periodic: w_j = 0.5 - 0.5 cos(2 pi j / samples))."""
    import numpy as np

    def integer(v):
        return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))

    def real(v):
        return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))

    what = "spectrum_table"
    if not integer(samples) or not integer(stride):
        raise TypeError(f"samples: {what}: samples and stride are integers, got {samples!r} and {stride!r}")
    if not real(dt):
        raise TypeError(f"dt: {what}: expected a number, got {dt!r}")
    if samples < 1 or stride < 1:
        raise ValueError(f"samples: {what}: samples = {samples} and stride = {stride} (both >= 1)")
    if not (dt > 0 and dt < float("inf")):
        raise ValueError(f"dt: {what}: {dt} (a finite time step > 0)")
    if taper not in ("rect", "hann"):
        raise ValueError(f"taper: {what}: {taper!r} ('rect' or 'hann')")
    if (bins is None) == (freqs is None):
        raise ValueError(f"bins: {what}: exactly one of bins= and freqs= names the frequencies")
    samples, stride, dt = int(samples), int(stride), float(dt)
    j = np.arange(samples, dtype=np.int64)
    if bins is not None:
        if torch.is_tensor(bins):
            bins = bins.tolist()
        if isinstance(bins, (str, bytes)) or not hasattr(bins, "__iter__"):
            raise TypeError(f"bins: {what}: expected a sequence of integers, got {bins!r}")
        bins = list(bins)
        if not all(integer(b) for b in bins):
            raise TypeError(f"bins: {what}: expected a sequence of integers, got {bins!r}")
        if not bins:
            raise ValueError(f"bins: {what}: no frequency was given")
        if min(bins) < 0 or max(bins) > samples // 2:
            raise ValueError(f"bins: {what}: bins {min(bins)} .. {max(bins)} of {samples} samples (0 <= b <= samples // 2 = {samples // 2})")
        b = np.asarray(bins, dtype=np.int64)
        f = b.astype(np.float64) / (samples * stride * dt)
        frac = ((j[:, None] * b[None, :]) % samples).astype(np.float64) / samples
    else:
        if torch.is_tensor(freqs):
            freqs = freqs.tolist()
        if isinstance(freqs, (str, bytes)) or not hasattr(freqs, "__iter__"):
            raise TypeError(f"freqs: {what}: expected a sequence of numbers, got {freqs!r}")
        freqs = list(freqs)
        if not all(real(v) for v in freqs):
            raise TypeError(f"freqs: {what}: expected a sequence of numbers, got {freqs!r}")
        if not freqs:
            raise ValueError(f"freqs: {what}: no frequency was given")
        f = np.asarray(freqs, dtype=np.float64)
        per_sample = f * dt * stride                     # cycles between two samples
        if not np.all((per_sample >= 0) & (per_sample <= 0.5 * (1.0 + 1e-12))):          # (the Nyquist frequency as 0.5 / (stride dt), rounded)
            raise ValueError(f"freqs: {what}: 0 <= f dt stride <= 0.5 cycles per sample (above is aliasing), got f dt stride = {per_sample.tolist()}")
        frac = np.fmod(per_sample[None, :] * j[:, None].astype(np.float64), 1.0)
    w = np.ones(samples, dtype=np.float64) if taper == "rect" else 0.5 - 0.5 * np.cos(2.0 * np.pi * j.astype(np.float64) / samples)
    th = 2.0 * np.pi * frac
    tw = np.stack([w[:, None] * np.cos(th), -(w[:, None] * np.sin(th))], axis=-1)
    return torch.from_numpy(np.ascontiguousarray(tw)), torch.from_numpy(w), torch.from_numpy(np.ascontiguousarray(f))


def rollout_spectrum(x: Tensor, step: Tensor, nf: int, max_steps: int, window: Tensor, tw: Tensor, pivot: Tensor, sum: Tensor, re: Tensor,
                     im: Tensor, *, stride: int = 1, x_step: int = 0) -> None:
    """g4c_rollout_spectrum: accumulate step t = step[0] (read on the device) into the per-node Fourier sums when t is sample
    j = (t - origin) / stride of the window — 0 <= t < max_steps, t >= origin = window[0] (int32 [2] on the device: {origin, last}),
    (t - origin) % stride == 0, j < samples — and leave window[1] = t; any other step touches nothing.  The sample is x [N, nf]
    (x_step = 0: the prediction) or x[:, nf t : nf (t + 1)] of x [N, >= nf max_steps] (x_step = nf: a target), float32 with rows of
    unit stride.  tw: float64 [samples, K, 2] (`spectrum_table`, on the device).  pivot / sum: float64 [nf, N]; re / im: float64
    [nf K, N], plane f K + k; unit stride along the nodes and one common plane stride >= N (views of padded buffers are fine).
    `step` is not written: the step's closing launch bumps it afterwards."""
    nf, max_steps, stride, x_step = int(nf), int(max_steps), int(stride), int(x_step)
    what = "rollout_spectrum"
    a = Args(what, TypeError)
    a.dtype(x, "x", torch.float32)
    if nf <= 0 or x_step not in (0, nf):
        raise ValueError(f"x_step: {what}: nf = {nf} (>= 1) and x_step = {x_step} (0: x is the sample, nf: x holds every step's columns)")
    a.at_least(max_steps, "max_steps", 0)
    if x_step:
        n_nodes, _, x_ld = a.strided_rows(x, "x", min_cols=nf * max_steps)
    else:
        n_nodes, _, x_ld = a.strided_rows(x, "x", cols=nf)
    a.step_index(step, entries=2)
    a.step_index(window, "window", entries=2)
    a.at_least(stride, "stride", 1)
    a.dtype(tw, "tw", torch.float64)
    if tw.dim() != 3 or int(tw.size(2)) != 2 or int(tw.size(0)) < 1 or int(tw.size(1)) < 1 or not tw.is_contiguous():
        raise ValueError(f"tw: {what}: expected a contiguous [samples >= 1, K >= 1, 2], got shape {tuple(tw.shape)} strides {tuple(tw.stride())}")
    samples, K = int(tw.size(0)), int(tw.size(1))
    plane_ld = a.planes_f64(n_nodes, ("pivot", pivot, nf), ("sum", sum, nf), ("re", re, nf * K), ("im", im, nf * K))
    lib = _lib.load()
    dev = _lib.require_hip(x, step, window, tw, pivot, sum, re, im)
    s = _lib.g4c_rollout_spectrum_t(max_steps=max_steps, stride=stride, n_samples=samples, n_bins=K, window=_lib.ptr(window), tw=_lib.ptr(tw),
                                    x_ld=x_ld, x_step=x_step, plane_ld=plane_ld, pivot=_lib.ptr(pivot),
                                    sum=_lib.ptr(sum), re=_lib.ptr(re), im=_lib.ptr(im))
    _lib.check(lib.g4c_rollout_spectrum(_lib.ptr(x), nf, C.byref(s), _lib.ptr(step), n_nodes, _lib.stream_handle(dev)))


def welch_planes(nf: int, K: int, reference: bool) -> int:
    """Planes of one Welch spectrum's accumulators: two sets of pivot and sum (nf each) and re and im (nf K each, plane f K + k), the
    averaged power pxx (nf K) and, with a reference, the averaged cross-spectrum cxr_re, cxr_im (nf K each)."""
    return 2 * spectrum_planes(nf, K) + (3 if reference else 1) * nf * K


def welch_split(nf: int, K: int, reference: bool):
    """The plane counts of (pivot, sum, re, im, pxx[, cxr_re, cxr_im]) in a buffer of `welch_planes` planes."""
    return (2 * nf, 2 * nf, 2 * nf * K, 2 * nf * K) + (nf * K,) * (3 if reference else 1)


def welch_weights(tw: Tensor) -> Tensor:
    """W [K, 2] = Σ_q tw[q], the rows added one by one in order (the sum g4c_rollout_welch removes a segment's mean with)."""
    W = torch.zeros(tw.shape[1:], dtype=torch.float64)
    for q in range(int(tw.size(0))):
        W = W + tw[q]
    return W


def rollout_welch(x: Tensor, step: Tensor, nf: int, max_steps: int, window: Tensor, tw: Tensor, W: Tensor, pivot: Tensor, sum: Tensor,
                  re: Tensor, im: Tensor, pxx: Tensor, *, hop: int, stride: int = 1, x_step: int = 0, cxr=None, ref=None, ref_row: int = -1,
                  ref_field: int = -1, track: Optional[Tensor] = None, track_host: Optional[Tensor] = None,
                  seg_power: Optional[Tensor] = None) -> None:
    """g4c_rollout_welch: add step t = step[0] (read on the device) to the segment(s) of Welch's estimator it belongs to and, when it
    ends a segment, the segment's power (and cross-spectrum with a reference) to the averages.  x, step, stride, x_step: as in
    `rollout_spectrum`.  window: int32 [3] on the device, {origin, last, closed}.  tw: float64 [L, K, 2] (`spectrum_table(samples=L)`, on
    the device), L >= 2 the segment's samples; W: float64 [K, 2] (`welch_weights(tw)`, on the device); hop: L (no overlap) or L / 2.
    pivot / sum: float64 [2 nf, N]; re / im: [2 nf K, N] (the two alternating sets); pxx: [nf K, N]; unit stride along the nodes and one
    common plane stride.  A reference: cxr = (cxr_re, cxr_im), [nf K, N] each of the same plane stride, and ref = (sum, re, im) of the
    reference's accumulator (None: this one's own), ref_row >= 0 one row for all rows (< 0: the same row), ref_field >= 0 one field for
    all fields (< 0: the same field).  Tracked rows: track int32 [P] on the device, track_host the same on the host, seg_power float64
    [max_segments, P, nf, K] on the device."""
    nf, max_steps, stride, x_step, hop, ref_row, ref_field = int(nf), int(max_steps), int(stride), int(x_step), int(hop), int(ref_row), int(ref_field)
    what = "rollout_welch"
    a = Args(what, TypeError)
    a.dtype(x, "x", torch.float32)
    if nf <= 0 or x_step not in (0, nf):
        raise ValueError(f"x_step: {what}: nf = {nf} (>= 1) and x_step = {x_step} (0: x is the sample, nf: x holds every step's columns)")
    a.at_least(max_steps, "max_steps", 0)
    if x_step:
        n_nodes, _, x_ld = a.strided_rows(x, "x", min_cols=nf * max_steps)
    else:
        n_nodes, _, x_ld = a.strided_rows(x, "x", cols=nf)
    a.step_index(step, entries=2)
    a.step_index(window, "window", entries=3)
    a.at_least(stride, "stride", 1)
    a.dtype(tw, "tw", torch.float64)
    if tw.dim() != 3 or int(tw.size(2)) != 2 or int(tw.size(0)) < 2 or int(tw.size(1)) < 1 or not tw.is_contiguous():
        raise ValueError(f"tw: {what}: expected a contiguous [L >= 2, K >= 1, 2], got shape {tuple(tw.shape)} strides {tuple(tw.stride())}")
    L, K = int(tw.size(0)), int(tw.size(1))
    a.tensor(W, "W", torch.float64, shape=(K, 2))
    planes = [("pivot", pivot, 2 * nf), ("sum", sum, 2 * nf), ("re", re, 2 * nf * K), ("im", im, 2 * nf * K), ("pxx", pxx, nf * K)]
    with_ref = cxr is not None or ref is not None or ref_row >= 0 or ref_field >= 0
    if with_ref:
        if cxr is None or len(cxr) != 2:
            raise ValueError(f"cxr: {what}: a reference needs cxr = (cxr_re, cxr_im)")
        ref = (sum, re, im) if ref is None else tuple(ref)
        if len(ref) != 3:
            raise ValueError(f"ref: {what}: expected (sum, re, im) of the reference's accumulator, got {len(ref)} tensors")
        planes += [("cxr_re", cxr[0], nf * K), ("cxr_im", cxr[1], nf * K), ("ref_sum", ref[0], 2 * nf), ("ref_re", ref[1], 2 * nf * K),
                   ("ref_im", ref[2], 2 * nf * K)]
        if ref_row >= max(n_nodes, 1):
            raise ValueError(f"ref_row: {what}: row {ref_row} of {n_nodes} nodes")
        if ref_field >= nf:
            raise ValueError(f"ref_field: {what}: field {ref_field} of {nf} fields")
    plane_ld = a.planes_f64(n_nodes, *planes)
    n_track = max_segments = 0
    if track is not None or track_host is not None or seg_power is not None:
        if track is None or track_host is None or seg_power is None:
            raise ValueError(f"track: {what}: tracked rows need track, track_host and seg_power")
        a.tensor(track, "track", torch.int32, dim=1)
        a.tensor(track_host, "track_host", torch.int32, shape=track.shape)
        if track_host.device.type != "cpu":
            raise ValueError(f"track_host: {what}: expected a host tensor, got one on '{track_host.device}'")
        n_track = int(track.numel())
        a.tensor(seg_power, "seg_power", torch.float64, dim=4)
        if tuple(seg_power.shape[1:]) != (n_track, nf, K):
            raise ValueError(f"seg_power: {what}: expected [max_segments, {n_track}, {nf}, {K}], got {tuple(seg_power.shape)}")
        max_segments = int(seg_power.size(0))
    lib = _lib.load()
    dev = _lib.require_hip(x, step, window, tw, W, *(t for _, t, _ in planes), track, seg_power)
    s = _lib.g4c_rollout_welch_t(max_steps=max_steps, stride=stride, seg_len=L, hop=hop, n_bins=K, x_ld=x_ld, x_step=x_step,
                                 ref_row=ref_row if with_ref else -1, ref_field=ref_field if with_ref else -1, n_track=n_track,
                                 max_segments=max_segments, window=_lib.ptr(window), tw=_lib.ptr(tw), W=_lib.ptr(W), inv_L=1.0 / L,
                                 plane_ld=plane_ld, pivot=_lib.ptr(pivot), sum=_lib.ptr(sum), re=_lib.ptr(re), im=_lib.ptr(im),
                                 pxx=_lib.ptr(pxx), cxr_re=_lib.ptr(cxr[0]) if with_ref else None, cxr_im=_lib.ptr(cxr[1]) if with_ref else None,
                                 ref_sum=_lib.ptr(ref[0]) if with_ref else None, ref_re=_lib.ptr(ref[1]) if with_ref else None,
                                 ref_im=_lib.ptr(ref[2]) if with_ref else None, track=_lib.ptr(track) if n_track else None,
                                 track_host=_lib.ptr(track_host) if n_track else None, seg_power=_lib.ptr(seg_power) if n_track else None)
    _lib.check(lib.g4c_rollout_welch(_lib.ptr(x), nf, C.byref(s), _lib.ptr(step), n_nodes, _lib.stream_handle(dev)))


def mesh_gradient_weights(rel: Tensor, csr, src32: Tensor, power: int = 2, out=None):
    """g4c_mesh_gradient_weights: the least-squares gradient weights of a mesh, once per mesh.  `csr` is the CSR-by-target of its
    edges (`plan.edge_csr(edge_index, n_nodes)[1]`: off int32 [N + 1], perm int32 [E] or None), src32 int32 [E] their senders and rel
    float32 [E, dim] their vectors receiver - sender, both in the caller's edge numbering; power 0, 1 or 2 weighs an edge by
    |rel|^(-power).  Returns (g float32 [E, dim], src int32 [E], degenerate uint8 [N]) with the edges in CSR order: the s-th in-edge
    of node i at position off[i] + s (include/g4c.h has the arithmetic).  `out`: the three tensors to write into; a mesh without
    edges or nodes launches nothing (then a fresh `degenerate` is all ones)."""
    return _stencil_weights("mesh_gradient_weights", "g4c_mesh_gradient_weights", lambda dim: dim, "edges", "E", rel, csr, src32, power, out)


def _stencil_weights(what, fn, width, entries, letter, rel, csr, src32, power, out):
    """The checks and the launch of `mesh_gradient_weights` and `mesh_jet_weights`: `fn` the name of the library's function,
    `width(dim)` the row width of its table, `entries` / `letter` what a stencil entry is called in a message ("edges" / "E",
    "entries" / "S")."""
    a = Args(what)
    a.choice(power, "power", (0, 1, 2), "0, 1 or 2")
    a.tensor(rel, "rel", torch.float32, dim=2)
    n_entries, dim = int(rel.size(0)), int(rel.size(1))
    if dim not in (2, 3):
        raise ValueError(f"rel: {what}: expected [{letter}, 2] or [{letter}, 3], got shape {tuple(rel.shape)}")
    W = width(dim)
    off, perm = getattr(csr, "off", None), getattr(csr, "perm", None)
    a.tensor(off, "csr.off", torch.int32, dim=1)
    if off.numel() < 1:
        raise ValueError(f"csr.off: {what}: expected [n_nodes + 1], got shape {tuple(off.shape)}")
    n_nodes = int(off.numel()) - 1
    if int(getattr(csr, "n", n_entries)) != n_entries:
        raise ValueError(f"csr: {what}: a plan of {csr.n} {entries} for rel of {n_entries}")
    if perm is not None:
        a.tensor(perm, "csr.perm", torch.int32, shape=(n_entries,))
    a.tensor(src32, "src32", torch.int32, shape=(n_entries,))
    if out is not None:
        table, src, degenerate = out
        a.tensor(table, "out[0]", torch.float32, shape=(n_entries, W))
        a.tensor(src, "out[1]", torch.int32, shape=(n_entries,))
        a.tensor(degenerate, "out[2]", torch.uint8, shape=(n_nodes,))
    else:
        table = src = degenerate = None
    dev = a.same_device(("rel", rel), ("csr.off", off), ("csr.perm", perm), ("src32", src32), ("out[0]", table), ("out[1]", src),
                        ("out[2]", degenerate))
    if out is None:
        table = torch.empty((n_entries, W), dtype=torch.float32, device=dev)
        src = torch.empty((n_entries,), dtype=torch.int32, device=dev)
        degenerate = torch.ones((n_nodes,), dtype=torch.uint8, device=dev)
    _lib.check(getattr(_lib.load(), fn)(_lib.ptr(off), _lib.ptr(perm), _lib.ptr(src32), _lib.ptr(rel), dim, power, n_nodes, n_entries,
                                        _lib.ptr(table), _lib.ptr(src), _lib.ptr(degenerate), _lib.stream_handle(dev)))
    return table, src, degenerate


def derived_program(program, nf: Optional[int] = None, dim: Optional[int] = None, order: int = 1) -> "_lib.g4c_derived_program_t":
    """A program of `mesh_derived` — a sequence of columns, each a sequence of 1 .. 3 terms (field, axis, coef): the column is
    Σ coef · ∂_axis x[:, field] — as the library's g4c_derived_program_t (returned unchanged if it is one already).  ValueError
    naming `program` on anything else; fields and axes are checked against nf / dim when those are given.  `order=2` is a program
    of `mesh_jet`: with `dim`, axis ranges over 0 .. Q − 1, Q = dim + dim (dim + 1) / 2 — the first derivatives, then the second ones
    xx, xy, yy (2-D) or xx, xy, xz, yy, yz, zz (3-D)."""
    if isinstance(program, _lib.g4c_derived_program_t):
        return program
    if isinstance(order, bool) or order not in (1, 2):
        raise ValueError(f"order: derived_program: expected 1 (mesh_derived) or 2 (mesh_jet), got {order!r}")
    what = "mesh_derived" if order == 1 else "mesh_jet"
    if order == 2 and dim is not None:
        dim = jet_size(dim)
    try:
        cols = [[tuple(t) for t in col] for col in program]
    except TypeError:
        raise ValueError(f"program: {what}: expected a sequence of columns of (field, axis, coef) terms, got {program!r}") from None
    if not 1 <= len(cols) <= _lib.DERIVED_MAX_COLS:
        raise ValueError(f"program: {what}: {len(cols)} columns (1 .. {_lib.DERIVED_MAX_COLS})")
    p = _lib.g4c_derived_program_t(nd=len(cols))
    for c, col in enumerate(cols):
        if not 1 <= len(col) <= _lib.DERIVED_MAX_TERMS:
            raise ValueError(f"program: {what}: column {c} has {len(col)} terms (1 .. {_lib.DERIVED_MAX_TERMS})")
        p.n_terms[c] = len(col)
        for k, term in enumerate(col):
            if len(term) != 3 or any(isinstance(v, bool) or not isinstance(v, int) for v in term[:2]):
                raise ValueError(f"program: {what}: column {c} term {k}: expected (field, axis, coef), got {term!r}")
            f, a, coef = term
            if f < 0 or (nf is not None and f >= nf):
                raise ValueError(f"program: {what}: column {c} term {k}: field {f} of {nf}")
            if a < 0 or (dim is not None and a >= dim):
                raise ValueError(f"program: {what}: column {c} term {k}: axis {a} of {dim}")
            p.field[c][k], p.axis[c][k], p.coef[c][k] = f, a, float(coef)
    if order == 2:
        _jet_fields(what, p)
    return p


def jet_size(dim: int) -> int:
    """Q = dim + dim (dim + 1) / 2: the derivatives per field of a quadratic fit on a mesh of `dim` dimensions (5 or 9)."""
    if isinstance(dim, bool) or dim not in (2, 3):
        raise ValueError(f"dim: mesh_jet: expected 2 or 3, got {dim!r}")
    return dim + dim * (dim + 1) // 2


def _jet_dim(a: Args, c, name="c") -> int:
    """The mesh's dimension from the width of a table of rows [S, Q]."""
    a.tensor(c, name, torch.float32, dim=2)
    if int(c.size(1)) not in (5, 9):
        raise a.fail(name, f"expected [S, 5] (2-D) or [S, 9] (3-D), got shape {tuple(c.shape)}")
    return 2 if int(c.size(1)) == 5 else 3


def mesh_jet_weights(rel: Tensor, csr, src32: Tensor, power: int = 2, out=None):
    """g4c_mesh_jet_weights: the rows of a weighted least-squares quadratic fit over a stencil, once per mesh.  The stencil comes as
    `mesh_gradient_weights` takes the in-edges: `csr` (off int32 [N + 1], perm int32 [S] or None) groups its entries by receiver,
    src32 int32 [S] their senders and rel float32 [S, dim] their vectors receiver - sender in the caller's numbering; power 0, 1 or
    2.  Returns (c float32 [S, Q], src int32 [S], degenerate uint8 [N]) in CSR order, jet(i) = Σ_s c[s] (x[src[s]] - x[i]) with the
    first derivatives in columns 0 .. dim - 1 and the second ones after them (include/g4c.h has the arithmetic).  `out`: the three
    tensors to write into; an empty stencil launches nothing (then a fresh `degenerate` is all ones)."""
    return _stencil_weights("mesh_jet_weights", "g4c_mesh_jet_weights", jet_size, "entries", "S", rel, csr, src32, power, out)


def _fields(a: Args, x, nf):
    """(n_nodes, nf, x_ld) of the fields x[:, :nf] of `mesh_derived`, `mesh_jet` and `sample_points`: float32 [N, >= 1] with rows of
    unit stride, nf defaulting to every column, x_ld the row stride in elements."""
    n_nodes, cols = a.rows(x, "x")
    nf = cols if nf is None else int(nf)
    if not 1 <= nf <= cols:
        raise a.fail("nf", f"{nf} fields of x with {cols} columns")
    return n_nodes, nf, a.row_stride(x, "x")


def mesh_jet(x: Tensor, off: Tensor, c: Tensor, src: Tensor, program, out: Optional[Tensor] = None, *, nf: Optional[int] = None) -> Tensor:
    """g4c_mesh_jet: the columns of `program` (`derived_program(.., order=2)`: axis 0 .. Q - 1) of the fields x[:, :nf] (float32
    [N, x_ld], rows of unit stride; nf defaults to every column) by the quadratic fit (c float32 [S, Q], src int32 [S], off int32
    [N + 1]: the outputs of `mesh_jet_weights` and the stencil's offsets) into out float32 [N, nd] — one thread per node, fp32, its
    entries in CSR order: the same bits on every run.  At most 4 distinct fields per program."""
    what = "mesh_jet"
    a = Args(what)
    dim = _jet_dim(a, c)
    n_entries = int(c.size(0))
    n_nodes, nf, x_ld = _fields(a, x, nf)
    a.tensor(off, "off", torch.int32, shape=(n_nodes + 1,))
    a.tensor(src, "src", torch.int32, shape=(n_entries,))
    prog = derived_program(program, nf, dim, order=2)
    _jet_fields(what, prog)
    nd = int(prog.nd)
    if out is not None:
        a.tensor(out, "out", torch.float32, shape=(n_nodes, nd))
    dev = a.same_device(("x", x), ("off", off), ("c", c), ("src", src), ("out", out))
    if out is None:
        out = torch.empty((n_nodes, nd), dtype=torch.float32, device=dev)
    lib = _lib.load()
    _lib.check(lib.g4c_mesh_jet(_lib.ptr(x), x_ld, nf, dim, _lib.ptr(c), _lib.ptr(src), _lib.ptr(off), C.byref(prog), n_nodes, n_entries,
                                _lib.ptr(out), _lib.stream_handle(dev)))
    return out


def _jet_fields(what, prog) -> None:
    fields = {int(prog.field[c][k]) for c in range(int(prog.nd)) for k in range(int(prog.n_terms[c]))}
    if len(fields) > _lib.JET_MAX_FIELDS:
        raise ValueError(f"program: {what}: {len(fields)} distinct fields (at most {_lib.JET_MAX_FIELDS} per program)")


def mesh_jet_adjoint(gy: Tensor, off: Tensor, c: Tensor, out_off: Tensor, out_c: Tensor, out_dst: Tensor, program, nf: int,
                     gx: Optional[Tensor] = None) -> Tensor:
    """g4c_mesh_jet_adjoint: the transpose of `mesh_jet`'s map x[:, :nf] -> out, applied to gy float32 [N, nd] (contiguous): gx
    float32 [N, nf], every column written (a field the program does not differentiate gets zeros).  off and c as for `mesh_jet`;
    the sender side, built once per operator: with perm the CSR positions grouped by SENDER, ascending within a sender
    (`plan.gather_csr(src, N)`), out_off int32 [N + 1] its offsets, out_c float32 [S, Q] = c[perm] and out_dst int32 [S] the
    receivers of those positions.  One thread per node, fp32, a fixed order (include/g4c.h), no atomics.  `gx`: the tensor to write
    into (not gy)."""
    a = Args("mesh_jet_adjoint")
    dim = _jet_dim(a, c)
    return _stencil_adjoint(a, "g4c_mesh_jet_adjoint", dim, 2, "c", gy, off, c, out_off, out_c, out_dst, program, nf, gx)


def _stencil_adjoint(a: Args, fn, dim, order, name, gy, off, table, out_off, out_table, out_dst, program, nf, gx):
    """The checks and the launch of `mesh_derived_adjoint` and `mesh_jet_adjoint` behind the check of their table (`name`: "g" or
    "c"), which gave `dim`: `fn` the name of the library's function, `order` the program's (`derived_program`)."""
    what = a.what
    n_entries, W = int(table.size(0)), int(table.size(1))
    a.integer(nf, "nf", at_least=1)
    prog = derived_program(program, nf, dim, order=order)
    if order == 2:
        _jet_fields(what, prog)
    nd = int(prog.nd)
    a.tensor(gy, "gy", torch.float32, dim=2)
    if int(gy.size(1)) != nd:
        raise ValueError(f"gy: {what}: expected [n_nodes, {nd}] (one column per column of the program), got shape {tuple(gy.shape)}")
    n_nodes = int(gy.size(0))
    a.tensor(off, "off", torch.int32, shape=(n_nodes + 1,))
    a.tensor(out_off, "out_off", torch.int32, shape=(n_nodes + 1,))
    a.tensor(out_table, f"out_{name}", torch.float32, shape=(n_entries, W))
    a.tensor(out_dst, "out_dst", torch.int32, shape=(n_entries,))
    if gx is not None:
        a.tensor(gx, "gx", torch.float32, shape=(n_nodes, nf))
        a.distinct_storage(gx, "gx", ("gy", gy), identity=True)
    dev = a.same_device(("gy", gy), ("off", off), (name, table), ("out_off", out_off), (f"out_{name}", out_table), ("out_dst", out_dst),
                        ("gx", gx))
    if gx is None:
        gx = torch.empty((n_nodes, nf), dtype=torch.float32, device=dev)
    _lib.check(getattr(_lib.load(), fn)(_lib.ptr(gy), C.byref(prog), dim, nf, _lib.ptr(table), _lib.ptr(off), _lib.ptr(out_table),
                                        _lib.ptr(out_dst), _lib.ptr(out_off), n_nodes, n_entries, _lib.ptr(gx), _lib.stream_handle(dev)))
    return gx


def _gradient_table(a: Args, g, dims=(2, 3)):
    """(E, dim) of the least-squares gradient's table g float32 [E, dim], dim one of `dims`."""
    a.tensor(g, "g", torch.float32, dim=2)
    if int(g.size(1)) not in dims:
        raise a.fail("g", f"expected {' or '.join(f'[E, {d}]' for d in dims)}, got shape {tuple(g.shape)}")
    return int(g.size(0)), int(g.size(1))


def mesh_derived_scratch(n_nodes: int, nd: int, device) -> Tensor:
    """The `scratch` buffer of mesh_derived's statistics for a mesh of n_nodes and nd columns (g4c_mesh_derived_scratch_doubles)."""
    return torch.zeros(_scratch_doubles("g4c_mesh_derived_scratch_doubles", n_nodes, nd), dtype=torch.float64, device=device)


def mesh_derived(x: Tensor, off: Tensor, g: Tensor, src: Tensor, program, cur: Tensor, *, step: Optional[Tensor] = None, every: int = 0,
                 snap: Optional[Tensor] = None, stats: Optional[Tensor] = None, scratch: Optional[Tensor] = None, max_steps: int = 0,
                 nf: Optional[int] = None) -> None:
    """g4c_mesh_derived: the columns of `program` (see `derived_program`) of the fields x[:, :nf] (float32 [N, x_ld], rows of unit
    stride; nf defaults to every column) by the least-squares gradient (g float32 [E, dim], src int32 [E], off int32 [N + 1]: the
    outputs of `mesh_gradient_weights` and the plan's offsets) into cur float32 [N, nd] — one thread per node, fp32, its in-edges in
    CSR order.  With `step` (int32, t = step[0] is read on the device and not written): every = k > 0 and snap float32 [n_snap, N, nd]
    keep steps k - 1, 2k - 1, ... in slots 0, 1, ...; stats float64 [max_steps, nd, 3] receives (Σq², Σ|q|, max|q|) over the nodes
    at row t (overwritten; `scratch` from `mesh_derived_scratch`), in a fixed order: the same bits on every run."""
    what = "mesh_derived"
    every, max_steps = int(every), int(max_steps)
    a = Args(what)
    n_edges, dim = _gradient_table(a, g)
    n_nodes, nf, x_ld = _fields(a, x, nf)
    a.tensor(off, "off", torch.int32, shape=(n_nodes + 1,))
    a.tensor(src, "src", torch.int32, shape=(n_edges,))
    prog = derived_program(program, nf, dim)
    nd = int(prog.nd)
    a.tensor(cur, "cur", torch.float32, shape=(n_nodes, nd))
    a.lattice(every, max_steps, snap, "snap", "snapshot")
    if snap is not None:
        a.tensor(snap, "snap", torch.float32, dim=3)
        if tuple(snap.shape[1:]) != (n_nodes, nd):
            raise ValueError(f"snap: {what}: expected [n_snap, {n_nodes}, {nd}], got {tuple(snap.shape)}")
    if (stats is None) != (scratch is None):
        raise ValueError(f"{'scratch' if scratch is None else 'stats'}: {what}: stats and scratch come together")
    if stats is not None:
        a.tensor(stats, "stats", torch.float64, shape=(max_steps, nd, _lib.DERIVED_NSTAT))
        a.scratch(scratch, "scratch", record_scratch_doubles(n_nodes, nd * _lib.DERIVED_NSTAT), "mesh_derived_scratch")
    if step is None:
        if snap is not None or stats is not None:
            raise ValueError(f"step: {what}: snapshots and stats are addressed by the step index: pass step=")
    else:
        a.step_index(step)
    dev = a.same_device(("x", x), ("off", off), ("g", g), ("src", src), ("cur", cur), ("step", step), ("snap", snap),
                        ("stats", stats), ("scratch", scratch))
    lib = _lib.load()
    d = _lib.g4c_mesh_derived_t(dim=dim, nf=nf, x_ld=x_ld, g=_lib.ptr(g), src=_lib.ptr(src), off=_lib.ptr(off), cur=_lib.ptr(cur),
                                step=_lib.ptr(step), every=every, n_snap=0 if snap is None else int(snap.size(0)), max_steps=max_steps,
                                snap=_lib.ptr(snap), stats=_lib.ptr(stats), scratch=_lib.ptr(scratch))
    _lib.check(lib.g4c_mesh_derived(_lib.ptr(x), C.byref(d), C.byref(prog), n_nodes, _lib.stream_handle(dev)))


def mesh_derived_adjoint(gy: Tensor, off: Tensor, g: Tensor, out_off: Tensor, out_g: Tensor, out_dst: Tensor, program, nf: int,
                         gx: Optional[Tensor] = None) -> Tensor:
    """g4c_mesh_derived_adjoint: the transpose of `mesh_derived`'s map x[:, :nf] -> cur, applied to gy float32 [N, nd] (contiguous):
    gx float32 [N, nf], every column written (a field the program does not differentiate gets zeros).  off int32 [N + 1] and g
    float32 [E, dim] as for `mesh_derived`.  The sender side, built once per mesh: with perm the CSR positions grouped by SENDER,
    ascending within a sender (`plan.gather_csr(src, N)`), out_off int32 [N + 1] its offsets, out_g float32 [E, dim] = g[perm] and
    out_dst int32 [E] the receivers of those positions.  One thread per node, fp32, a fixed order (include/g4c.h), no atomics: the
    same bits on every run.  `gx`: the tensor to write into (not gy)."""
    a = Args("mesh_derived_adjoint")
    _, dim = _gradient_table(a, g)
    return _stencil_adjoint(a, "g4c_mesh_derived_adjoint", dim, 1, "g", gy, off, g, out_off, out_g, out_dst, program, nf, gx)


def body_forces(x: Tensor, item: Tensor, body_off: Tensor, area: Tensor, unit: Tensor, arm: Tensor, cur: Tensor, *, pcol: int,
                ucol: int = 0, vcol: int = 1, mu: float = 0.0, p_scale: float = 1.0, p_shift: float = 0.0, u_scale: float = 1.0,
                v_scale: float = 1.0, off: Optional[Tensor] = None, g: Optional[Tensor] = None, src: Optional[Tensor] = None,
                wall: Optional[Tensor] = None, stats: Optional[Tensor] = None, max_steps: int = 0, step: Optional[Tensor] = None,
                t: int = 0, x_step: int = 0) -> Tensor:
    """g4c_body_forces: the force of the 2-D fields x (float32 [N, x_ld], rows of unit stride) on B bodies whose walls are the W
    items `item` int32 [W] (node rows, body after body: body b holds item[body_off[b] : body_off[b + 1]], body_off int32 [B + 1]) with
    the fp64 tables area / unit / arm [W, 2] (`gfd.BodyForces` builds them).  The pressure is p_scale x[:, pcol] + p_shift, the
    velocity (u_scale x[:, ucol], v_scale x[:, vcol]); mu != 0 adds the viscous traction by the least-squares gradient (off int32
    [N + 1], g float32 [E, 2], src int32 [E]: `gfd.MeshGradient`), mu == 0 reads neither the gradient nor the velocity.  x_step = nf
    reads the columns nf t .. of a target that holds every step's fields.  The step index is `step[0]` (int32, read on the device,
    never written) or, without `step`, `t`.  Writes cur float32 [B, 3] = (F_x, F_y, M) and wall float32 [W, 2] = (pressure, wall
    shear) on every call, and stats float64 [max_steps, B, 6] = (Fp_x, Fp_y, Fv_x, Fv_y, Mp, Mv) at row t when 0 <= t < max_steps
    (overwritten), in a fixed order: the same bits on every run.  include/g4c.h has the arithmetic.  The entries of item are rows
    of x: they are not checked.  Returns cur."""
    what = "body_forces"
    max_steps, t, x_step = int(max_steps), int(t), int(x_step)
    a = Args(what)
    n_nodes, cols, x_ld = a.strided_rows(x, "x")
    a.tensor(item, "item", torch.int32, dim=1)
    n_items = int(item.size(0))
    a.tensor(body_off, "body_off", torch.int32, dim=1)
    n_bodies = int(body_off.size(0)) - 1
    if n_bodies < 0:
        raise ValueError(f"body_off: {what}: expected [n_bodies + 1], got shape {tuple(body_off.shape)}")
    for name, tab in (("area", area), ("unit", unit), ("arm", arm)):
        a.tensor(tab, name, torch.float64, shape=(n_items, 2))
    a.tensor(cur, "cur", torch.float32, shape=(n_bodies, 3))
    for name, v in (("mu", mu), ("p_scale", p_scale), ("p_shift", p_shift), ("u_scale", u_scale), ("v_scale", v_scale)):
        a.number(v, name)
    viscous = float(mu) != 0.0
    a.at_least(max_steps, "max_steps", 0)
    if x_step < 0 or (x_step > 0 and max_steps < 1):
        raise ValueError(f"x_step: {what}: {x_step} (0: x holds the fields, nf: x holds the nf fields of each of max_steps = {max_steps} >= 1 steps)")
    width = x_step if x_step else cols
    for name, c in (("pcol", pcol),) + ((("ucol", ucol), ("vcol", vcol)) if viscous else ()):
        a.column(c, name, width)
    if x_step and cols < x_step * max_steps:
        raise ValueError(f"x: {what}: {cols} columns, x_step = {x_step} and max_steps = {max_steps} need {x_step * max_steps}")
    if viscous:
        for name, tab in (("off", off), ("g", g), ("src", src)):
            if tab is None:
                raise ValueError(f"{name}: {what}: mu != 0 needs the gradient's off, g and src")
        n_edges, _ = _gradient_table(a, g, dims=(2,))          # (the operator is 2-D)
        a.tensor(off, "off", torch.int32, shape=(n_nodes + 1,))
        a.tensor(src, "src", torch.int32, shape=(n_edges,))
    else:
        off = g = src = None
        ucol = vcol = 0
    if wall is not None:
        a.tensor(wall, "wall", torch.float32, shape=(n_items, 2))
    if stats is not None:
        if max_steps < 1:
            raise ValueError(f"max_steps: {what}: stats need max_steps >= 1, got {max_steps}")
        a.tensor(stats, "stats", torch.float64, shape=(max_steps, n_bodies, _lib.FORCES_NSUM))
    if step is not None:
        a.step_index(step)
    dev = a.same_device(("x", x), ("item", item), ("body_off", body_off), ("area", area), ("unit", unit), ("arm", arm), ("cur", cur),
                        ("off", off), ("g", g), ("src", src), ("wall", wall), ("stats", stats), ("step", step))
    lib = _lib.load()
    bf = _lib.g4c_body_forces_t(x=_lib.ptr(x), x_ld=x_ld, x_step=x_step, step=_lib.ptr(step), t0=t, pcol=pcol, ucol=ucol, vcol=vcol,
                                mu=float(mu), p_scale=float(p_scale), p_shift=float(p_shift), u_scale=float(u_scale), v_scale=float(v_scale),
                                g=_lib.ptr(g), src=_lib.ptr(src), off=_lib.ptr(off), item=_lib.ptr(item), body_off=_lib.ptr(body_off),
                                area=_lib.ptr(area), unit=_lib.ptr(unit), arm=_lib.ptr(arm), stats=_lib.ptr(stats), cur=_lib.ptr(cur),
                                wall=_lib.ptr(wall), max_steps=max_steps)
    _lib.check(lib.g4c_body_forces(C.byref(bf), n_bodies, n_items, _lib.stream_handle(dev)))
    return cur


def body_forces_adjoint(gF: Optional[Tensor], gwall: Optional[Tensor], item_body: Tensor, area: Tensor, unit: Tensor, arm: Tensor,
                        own_off: Tensor, own_item: Tensor, n_bodies: int, nf: int, *, pcol: int, ucol: int = 0, vcol: int = 1,
                        mu: float = 0.0, p_scale: float = 1.0, u_scale: float = 1.0, v_scale: float = 1.0, g: Optional[Tensor] = None,
                        off: Optional[Tensor] = None, in_off: Optional[Tensor] = None, in_item: Optional[Tensor] = None,
                        in_g: Optional[Tensor] = None, hw: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """g4c_body_forces_adjoint: the transpose of the linear part of `body_forces`' map x -> (stats [B, 6], wall [W, 2]), applied to
    gF float64 [B, 6] and gwall float32 [W, 2] (contiguous; either may be None: zeros): gx float32 [N, nf], every element written (+0
    where nothing arrives).  area / unit / arm float64 [W, 2] and the constants as for `body_forces` (p_shift drops out).  The node
    side, built once per wall (`gfd.BodyForces` does it): item_body int32 [W] the body of every item; own_off int32 [N + 1] / own_item
    int32 [W] the items grouped by their node, ascending; and, for mu != 0, off int32 [N + 1] / g float32 [E, 2] of the gradient and
    in_off int32 [N + 1] / in_item int32 [Q] / in_g float32 [Q, 2]: the (item, in-edge of its node) pairs grouped by the edge's sender,
    ascending CSR position then item within a sender, with the weights copied into that order.  Two launches (per item into the scratch
    hw float32 [W, 5], then one thread per node), fp32 sums in a fixed order (include/g4c.h), no atomics: the same bits on every run.
    `out`: the tensor to write into; `hw`: the scratch to use."""
    what = "body_forces_adjoint"
    a = Args(what)
    a.integer(n_bodies, "n_bodies", at_least=0)
    a.integer(nf, "nf", at_least=1)
    for name, v in (("mu", mu), ("p_scale", p_scale), ("u_scale", u_scale), ("v_scale", v_scale)):
        a.number(v, name)
    viscous = float(mu) != 0.0
    for name, c in (("pcol", pcol),) + ((("ucol", ucol), ("vcol", vcol)) if viscous else ()):
        a.column(c, name, nf)
    if viscous and len({pcol, ucol, vcol}) != 3:
        raise ValueError(f"ucol: {what}: pcol = {pcol}, ucol = {ucol} and vcol = {vcol} must be distinct")
    a.tensor(item_body, "item_body", torch.int32, dim=1)
    n_items = int(item_body.size(0))
    for name, tab in (("area", area), ("unit", unit), ("arm", arm)):
        a.tensor(tab, name, torch.float64, shape=(n_items, 2))
    a.tensor(own_off, "own_off", torch.int32, dim=1)
    n_nodes = int(own_off.size(0)) - 1
    if n_nodes < 0:
        raise ValueError(f"own_off: {what}: expected [n_nodes + 1], got shape {tuple(own_off.shape)}")
    a.tensor(own_item, "own_item", torch.int32, shape=(n_items,))
    if gF is not None:
        a.tensor(gF, "gF", torch.float64, shape=(n_bodies, _lib.FORCES_NSUM))
    if gwall is not None:
        a.tensor(gwall, "gwall", torch.float32, shape=(n_items, 2))
    n_entries = 0
    if viscous:
        for name, tab in (("g", g), ("off", off), ("in_off", in_off), ("in_item", in_item), ("in_g", in_g)):
            if tab is None:
                raise ValueError(f"{name}: {what}: mu != 0 needs the gradient's g and off and the in-tables")
        _gradient_table(a, g, dims=(2,))          # (the operator is 2-D)
        a.tensor(off, "off", torch.int32, shape=(n_nodes + 1,))
        a.tensor(in_off, "in_off", torch.int32, shape=(n_nodes + 1,))
        a.tensor(in_item, "in_item", torch.int32, dim=1)
        n_entries = int(in_item.size(0))
        if n_entries >= 2 ** 31:
            raise NotImplementedError(f"in_item: {what}: {n_entries} list entries do not fit the int32 offsets")
        a.tensor(in_g, "in_g", torch.float32, shape=(n_entries, 2))
    else:
        g = off = in_off = in_item = in_g = None
        ucol = vcol = 0
    if hw is not None:
        a.tensor(hw, "hw", torch.float32, shape=(n_items, 5))
    if out is not None:
        a.tensor(out, "out", torch.float32, shape=(n_nodes, nf))
        a.distinct_storage(out, "out", ("gF", gF), ("gwall", gwall), ("hw", hw))
    dev = a.same_device(("item_body", item_body), ("area", area), ("unit", unit), ("arm", arm), ("own_off", own_off),
                        ("own_item", own_item), ("gF", gF), ("gwall", gwall), ("g", g), ("off", off), ("in_off", in_off),
                        ("in_item", in_item), ("in_g", in_g), ("hw", hw), ("out", out))
    if hw is None:
        hw = torch.empty((n_items, 5), dtype=torch.float32, device=dev)
    if out is None:
        out = torch.empty((n_nodes, nf), dtype=torch.float32, device=dev)
    lib = _lib.load()
    a = _lib.g4c_body_forces_adjoint_t(gF=_lib.ptr(gF), gwall=_lib.ptr(gwall), nf=nf, pcol=pcol, ucol=ucol, vcol=vcol, mu=float(mu),
                                       p_scale=float(p_scale), u_scale=float(u_scale), v_scale=float(v_scale), g=_lib.ptr(g),
                                       off=_lib.ptr(off), item_body=_lib.ptr(item_body), area=_lib.ptr(area), unit=_lib.ptr(unit),
                                       arm=_lib.ptr(arm), own_off=_lib.ptr(own_off), own_item=_lib.ptr(own_item), in_off=_lib.ptr(in_off),
                                       in_item=_lib.ptr(in_item), in_g=_lib.ptr(in_g), hw=_lib.ptr(hw), gx=_lib.ptr(out))
    _lib.check(lib.g4c_body_forces_adjoint(C.byref(a), n_nodes, n_bodies, n_items, n_entries, _lib.stream_handle(dev)))
    return out


def _sample_tables(a: Args, idx, coef):
    """The j-major tables of ops.sample_*: idx int32 [k, P] (and coef float32 [k, P]) -> (k, P); ValueError naming the argument."""
    a.tensor(idx, "idx", torch.int32, dim=2)
    k, n_points = int(idx.size(0)), int(idx.size(1))
    if not 1 <= k <= _lib.SAMPLE_MAX_K:
        raise a.fail("idx", f"expected [k, P] with 1 <= k <= {_lib.SAMPLE_MAX_K} neighbours, got shape {tuple(idx.shape)}")
    if coef is not None:
        a.tensor(coef, "coef", torch.float32, shape=(k, n_points))
    return k, n_points


def _periodic_axes(what: str, name: str, v, dim: int):
    """`dim` finite numbers >= 0 (0: an axis that is not periodic) padded to 3 floats; ValueError naming the argument."""
    try:
        vals = [float(c) for c in v]
    except (TypeError, ValueError):
        raise ValueError(f"{name}: {what}: expected {dim} numbers >= 0, got {v!r}") from None
    if len(vals) not in (dim, 3) or not all(0.0 <= c < float("inf") for c in vals) or any(vals[dim:]):
        raise ValueError(f"{name}: {what}: expected {dim} finite numbers >= 0 (0: the axis is not periodic), got {v!r}")
    return vals[:dim] + [0.0] * (3 - dim)


def sample_weights(pos: Tensor, queries: Tensor, idx: Tensor, power: int = 2, out=None, *, origin=None, period=None):
    """g4c_sample_weights: the coefficients of a moving-least-squares fit with a linear basis, once per set of points.  pos float32
    [N, dim] the nodes, queries float32 [P, dim] the points, idx int32 [k, P] (j-major, nearest first: `knn_query_device`'s rows,
    transposed) their k <= 16 nearest nodes; power 0, 1 or 2 weighs a neighbour by its distance^(-power).  Returns (coef float32
    [k, P], distance float32 [P] — to the nearest node —, degenerate uint8 [P]); include/g4c.h has the arithmetic.  `out`: the three
    tensors to write into; no points launch nothing.

    `period` (dim fp32 lengths, 0 an axis that is not periodic) with `origin` (dim numbers, the cloud's minimum): the fit over wrapped
    offsets (g4c_sample_weights_periodic) — the points are wrapped into the period, every offset by `connect_knn`'s rule; idx are
    then `knn_query_device(period=)`'s rows and distance is the wrapped one."""
    what = "sample_weights"
    if (origin is None) != (period is None):
        raise ValueError(f"period: {what}: origin and period come together")
    a = Args(what)
    a.choice(power, "power", (0, 1, 2), "0, 1 or 2")
    a.tensor(pos, "pos", torch.float32, dim=2)
    n_nodes, dim = int(pos.size(0)), int(pos.size(1))
    if dim not in (2, 3):
        raise ValueError(f"pos: {what}: expected [N, 2] or [N, 3], got shape {tuple(pos.shape)}")
    k, n_points = _sample_tables(a, idx, None)
    a.tensor(queries, "queries", torch.float32, shape=(n_points, dim))
    if n_points > 0 and n_nodes < k:
        raise ValueError(f"idx: {what}: k = {k} neighbours of {n_nodes} nodes")
    if out is not None:
        coef, distance, degenerate = out
        a.tensor(coef, "out[0]", torch.float32, shape=(k, n_points))
        a.tensor(distance, "out[1]", torch.float32, shape=(n_points,))
        a.tensor(degenerate, "out[2]", torch.uint8, shape=(n_points,))
    else:
        coef = distance = degenerate = None
    dev = a.same_device(("pos", pos), ("queries", queries), ("idx", idx), ("out[0]", coef), ("out[1]", distance), ("out[2]", degenerate))
    if out is None:
        coef = torch.empty((k, n_points), dtype=torch.float32, device=dev)
        distance = torch.empty((n_points,), dtype=torch.float32, device=dev)
        degenerate = torch.empty((n_points,), dtype=torch.uint8, device=dev)
    lib = _lib.load()
    if period is not None:
        per, org = _periodic_axes(what, "period", period, dim), [float(o) for o in origin]
        if len(org) not in (dim, 3) or not all(abs(o) < float("inf") for o in org):
            raise ValueError(f"origin: {what}: expected {dim} finite numbers, got {origin!r}")
        org = org[:dim] + [0.0] * (3 - dim)
        _lib.check(lib.g4c_sample_weights_periodic(_lib.ptr(pos), _lib.ptr(queries), _lib.ptr(idx), dim, power, k, n_nodes, n_points,
                                                   (C.c_float * 3)(*org), (C.c_float * 3)(*per), _lib.ptr(coef), _lib.ptr(distance),
                                                   _lib.ptr(degenerate), _lib.stream_handle(dev)))
        return coef, distance, degenerate
    _lib.check(lib.g4c_sample_weights(_lib.ptr(pos), _lib.ptr(queries), _lib.ptr(idx), dim, power, k, n_nodes, n_points, _lib.ptr(coef),
                                      _lib.ptr(distance), _lib.ptr(degenerate), _lib.stream_handle(dev)))
    return coef, distance, degenerate


def sample_points(x: Tensor, idx: Tensor, coef: Tensor, cur: Optional[Tensor] = None, *, step: Optional[Tensor] = None, every: int = 0,
                  series: Optional[Tensor] = None, max_steps: int = 0, nf: Optional[int] = None) -> Tensor:
    """g4c_sample_points: cur[p, f] = Σ_j coef[j, p] · x[idx[j, p], f] over the columns x[:, :nf] (float32 [N, x_ld], rows of unit
    stride; nf defaults to every column), idx int32 / coef float32 [k, P] (`sample_weights`) — fp32, j ascending, every product
    rounded before it is added: a numpy.float32 loop gives the same bits.  Returns cur float32 [P, nf] (`cur=`: written in place).
    With `step` (int32, t = step[0] is read on the device and not written): every = e > 0 and series float32 [max_steps // e, P, nf]
    keep steps e - 1, 2e - 1, ... in slots 0, 1, ...; any other step writes cur only.  The entries of idx are rows of x: they are
    not checked."""
    what = "sample_points"
    every, max_steps = int(every), int(max_steps)
    a = Args(what)
    k, n_points = _sample_tables(a, idx, coef)
    n_nodes, nf, x_ld = _fields(a, x, nf)
    if n_points > 0 and n_nodes < k:
        raise ValueError(f"idx: {what}: k = {k} neighbours of {n_nodes} nodes")
    if cur is not None:
        a.tensor(cur, "cur", torch.float32, shape=(n_points, nf))
    a.lattice(every, max_steps, series, "series", "series")
    if series is not None:
        a.tensor(series, "series", torch.float32, shape=(max_steps // every, n_points, nf))
        if step is None:
            raise ValueError(f"step: {what}: the slots are addressed by the step index: pass step=")
    if step is not None:
        a.step_index(step)
    dev = a.same_device(("x", x), ("idx", idx), ("coef", coef), ("cur", cur), ("step", step), ("series", series))
    if cur is None:
        cur = torch.empty((n_points, nf), dtype=torch.float32, device=dev)
    lib = _lib.load()
    s = _lib.g4c_sample_points_t(idx=_lib.ptr(idx), coef=_lib.ptr(coef), k=k, nf=nf, x_ld=x_ld, cur=_lib.ptr(cur), step=_lib.ptr(step),
                                 every=every, n_slots=0 if series is None else int(series.size(0)), max_steps=max_steps,
                                 series=_lib.ptr(series))
    _lib.check(lib.g4c_sample_points(_lib.ptr(x), C.byref(s), n_nodes, n_points, _lib.stream_handle(dev)))
    return cur


def sample_points_adjoint(gy: Tensor, in_off: Tensor, in_pt: Tensor, in_coef: Tensor, n_nodes: int, out: Optional[Tensor] = None) -> Tensor:
    """g4c_sample_points_adjoint: the transpose of `sample_points`' map x -> cur, applied to gy float32 [P, nf] (contiguous): gx float32
    [n_nodes, nf], every element written (a node no point uses gets +0).  The node side, built once per set of points
    (`PointSampler` does it): with the entries of the j-major [k, P] tables grouped by the node they name, ascending flat position
    within a node (`plan.gather_csr(idx.reshape(-1), n_nodes)`), in_off int32 [n_nodes + 1] the offsets of that grouping, in_pt int32
    [k·P] the point (position mod P) and in_coef float32 [k·P] the coefficient of each entry, in its order.  One thread per (node,
    chunk of 4 columns), fp32, a fixed order (include/g4c.h), no atomics: the same bits on every run.  The index values are never
    read here.  `out`: the tensor to write into (not gy)."""
    what = "sample_points_adjoint"
    a = Args(what)
    a.integer(n_nodes, "n_nodes", at_least=0)
    a.tensor(gy, "gy", torch.float32, dim=2)
    n_points, nf = int(gy.size(0)), int(gy.size(1))
    if nf < 1:
        raise ValueError(f"gy: {what}: expected [n_points, >= 1], got shape {tuple(gy.shape)}")
    a.tensor(in_off, "in_off", torch.int32, shape=(n_nodes + 1,))
    a.tensor(in_pt, "in_pt", torch.int32, dim=1)
    n_entries = int(in_pt.size(0))
    if n_entries >= 2 ** 31:
        raise NotImplementedError(f"in_pt: {what}: {n_entries} table entries do not fit the int32 offsets")
    if (n_entries > 0) != (n_points > 0) or (n_points > 0 and n_entries % n_points):
        raise ValueError(f"in_pt: {what}: expected [k * {n_points}] (k entries per point), got shape {tuple(in_pt.shape)}")
    a.tensor(in_coef, "in_coef", torch.float32, shape=(n_entries,))
    if out is not None:
        a.tensor(out, "out", torch.float32, shape=(n_nodes, nf))
        a.distinct_storage(out, "out", ("gy", gy), identity=True)
    dev = a.same_device(("gy", gy), ("in_off", in_off), ("in_pt", in_pt), ("in_coef", in_coef), ("out", out))
    if out is None:
        out = torch.empty((n_nodes, nf), dtype=torch.float32, device=dev)
    lib = _lib.load()
    _lib.check(lib.g4c_sample_points_adjoint(_lib.ptr(gy), _lib.ptr(in_off), _lib.ptr(in_pt), _lib.ptr(in_coef), nf, n_nodes, n_points,
                                             _lib.ptr(out), _lib.stream_handle(dev)))
    return out


def _tracer_triple(what, name, v, dim, default):
    """`dim` numbers (or None: `default`) -> a list of 3 floats, padded with `default`."""
    if v is None:
        return [float(default)] * 3
    try:
        vals = [float(c) for c in (v.tolist() if torch.is_tensor(v) else v)]
    except (TypeError, ValueError):
        raise ValueError(f"{name}: {what}: expected {dim} numbers, got {v!r}") from None
    if len(vals) != dim:
        raise ValueError(f"{name}: {what}: expected {dim} numbers, got {v!r}")
    return vals + [float(default)] * (3 - dim)


def tracer_advance(grid: dict, x0: Tensor, x1: Optional[Tensor], q: Tensor, status: Tensor, stopped: Tensor, release: Tensor, *, dt: float,
                   k: int, power: int = 2, scheme: int = _lib.TRACER_HEUN, vcol=None, scale=None, shift=None, box_lo=None, box_hi=None,
                   max_distance: float = float("inf"), step: Optional[Tensor] = None, t: int = 0, max_steps: int = 2 ** 31 - 1,
                   every: int = 0, series: Optional[Tensor] = None, vel: Optional[Tensor] = None) -> Tensor:
    """g4c_tracer_advance: one step of P massless particles through a velocity at the nodes — per particle the k nearest nodes (the
    ring search of `knn_query_device`), the coefficients of `sample_weights`, the sum of `sample_points`, and q += dt v (scheme 0,
    Euler, on x0) or Heun's two stages (scheme 1: x0 at q, x1 at q + dt v0).  `grid`: the cloud's cell grid (`synthetic._bin_cloud` of
    the node positions, built once per mesh); x0, x1 float32 [N, >= 1] (rows of unit stride, any leading dimension; x1 None for Euler);
    vcol the velocity's columns in both (default 0 .. dim - 1), v = scale u + shift; q float32 [P, dim] (updated in place), status uint8
    [P] (0 waiting, 1 moving, 2 left the box, 3 farther than max_distance from every node, 4 a position that is not finite), stopped
    int32 [P], release int32 [P] (the first step a particle moves at), vel float32 [P, dim] (optional: the first stage's velocity).
    The step index is `step[0]` (int32, read on the device, never written) or, without `step`, `t`; steps outside 0 <= t < max_steps
    move nothing.  every = e > 0 and series float32 [n_slots, P, dim] keep every particle's position after steps e - 1, 2e - 1, ... in
    slots 0, 1, ...  include/g4c.h has the rule.  Returns q."""
    what = "tracer_advance"
    a = Args(what)
    dim, n_nodes, cells = a.cell_grid(grid)
    if len(cells) == 3 and all(c >= 1 for c in cells):          # (the entry point refuses any other grid: the kernel reads cell_start by it)
        a.cell_start(grid, cells)
    every, max_steps, t = int(every), int(max_steps), int(t)
    a.integer(k, "k", at_least=1, at_most=_lib.SAMPLE_MAX_K)
    a.choice(power, "power", (0, 1, 2), "0, 1 or 2")
    a.choice(scheme, "scheme", (_lib.TRACER_EULER, _lib.TRACER_HEUN), "0 (Euler) or 1 (Heun)", integer=False)
    _, _, x0_ld = a.strided_rows(x0, "x0", rows=n_nodes)          # (rows of unit stride, any leading dimension)
    if x1 is None:
        if scheme == _lib.TRACER_HEUN:
            raise ValueError(f"x1: {what}: Heun's second stage reads the node tensor of the next time level: pass x1=")
        x1_ld = 0
    else:
        _, _, x1_ld = a.strided_rows(x1, "x1", rows=n_nodes)
    a.tensor(q, "q", torch.float32, dim=2)
    n_particles = int(q.size(0))
    if int(q.size(1)) != dim:
        raise ValueError(f"q: {what}: expected [P, {dim}] (the mesh has {dim} dimensions), got {tuple(q.shape)}")
    a.tensor(status, "status", torch.uint8, shape=(n_particles,))
    a.tensor(stopped, "stopped", torch.int32, shape=(n_particles,))
    a.tensor(release, "release", torch.int32, shape=(n_particles,))
    if vel is not None:
        a.tensor(vel, "vel", torch.float32, shape=(n_particles, dim))
    if n_particles > 0 and n_nodes < k:
        raise ValueError(f"k: {what}: {k} neighbours of {n_nodes} nodes")
    vcol = list(range(dim)) if vcol is None else [v for v in vcol]
    width = min(int(x0.size(1)), int(x1.size(1))) if x1 is not None else int(x0.size(1))
    if len(vcol) != dim or not all(isinstance(v, int) and not isinstance(v, bool) and 0 <= v < width for v in vcol):
        raise ValueError(f"vcol: {what}: expected {dim} columns of node tensors with {width} columns, got {vcol!r}")
    scale, shift = _tracer_triple(what, "scale", scale, dim, 1.0), _tracer_triple(what, "shift", shift, dim, 0.0)
    box_lo = _tracer_triple(what, "box_lo", box_lo, dim, float("-inf"))
    box_hi = _tracer_triple(what, "box_hi", box_hi, dim, float("inf"))
    a.lattice(every, max_steps, series, "series", "series")
    if series is not None:
        a.tensor(series, "series", torch.float32, dim=3)
        if tuple(series.shape[1:]) != (n_particles, dim):
            raise ValueError(f"series: {what}: expected [n_slots, {n_particles}, {dim}], got {tuple(series.shape)}")
    if step is not None:
        a.step_index(step)
    dev = a.same_device(("q", q), ("x0", x0), ("x1", x1), ("status", status), ("stopped", stopped), ("release", release),
                        ("vel", vel), ("step", step), ("series", series), ("grid", grid["pos_sorted"]))
    tr = _lib.g4c_tracer_t(pos_sorted=_lib.ptr(grid["pos_sorted"]), order=_lib.ptr(grid["order"]), cell_start=_lib.ptr(grid["cell_start"]),
                           n_cells=(C.c_int32 * 3)(*grid["n_cells"]), origin=grid["org"], cell_size=float(grid["h"]), dim=dim, k=k,
                           power=power, x0=_lib.ptr(x0), x1=_lib.ptr(x1), x0_ld=x0_ld, x1_ld=x1_ld, vcol=(C.c_int32 * 3)(*(vcol + [0] * (3 - dim))),
                           scale=(C.c_float * 3)(*scale), shift=(C.c_float * 3)(*shift), dt=float(dt), scheme=int(scheme),
                           box_lo=(C.c_float * 3)(*box_lo), box_hi=(C.c_float * 3)(*box_hi), max_distance=float(max_distance),
                           step=_lib.ptr(step), t_host=t, max_steps=max_steps, every=every,
                           n_slots=0 if series is None else int(series.size(0)), series=_lib.ptr(series), q=_lib.ptr(q),
                           status=_lib.ptr(status), stopped=_lib.ptr(stopped), release=_lib.ptr(release), vel=_lib.ptr(vel))
    lib = _lib.load()
    if "periods" in grid:          # (`synthetic._bin_cloud_periodic`'s grid: the periodic launch)
        periods = _periodic_axes(what, "grid['periods']", grid["periods"], dim)
        cell = _periodic_axes(what, "grid['cells']", list(grid.get("cells") or ())[:dim], dim)[:dim] + [1.0] * (3 - dim)
        if not all(c > 0.0 for c in cell):
            raise ValueError(f"grid['cells']: {what}: expected {dim} cell sizes > 0, got {grid.get('cells')!r}")
        trp = _lib.g4c_tracer_periodic_t(base=tr, period=(C.c_float * 3)(*periods), cell=(C.c_double * 3)(*cell))
        _lib.check(lib.g4c_tracer_advance_periodic(C.byref(trp), n_nodes, n_particles, _lib.stream_handle(dev)))
        return q
    _lib.check(lib.g4c_tracer_advance(C.byref(tr), n_nodes, n_particles, _lib.stream_handle(dev)))
    return q


def _box_arg(what: str, box):
    """`box` -> (lo_x, lo_y, hi_x, hi_y) as floats: four finite numbers with lo < hi per axis."""
    try:
        vals = [float(c) for c in (box.reshape(-1).tolist() if torch.is_tensor(box) else box)]
    except (TypeError, ValueError, AttributeError):
        raise ValueError(f"box: {what}: expected (lo_x, lo_y, hi_x, hi_y), got {box!r}") from None
    if len(vals) != 4 or not all(math.isfinite(v) for v in vals) or not (vals[0] < vals[2] and vals[1] < vals[3]):
        raise ValueError(f"box: {what}: expected four finite numbers (lo_x, lo_y, hi_x, hi_y) with lo < hi, got {box!r}")
    return vals


def voronoi_cells(grid: dict, box, normals: Optional[Tensor] = None, out=None):
    """g4c_voronoi_cells: per node of a 2-D cloud the polygon (its Voronoi cell) ∩ (`box` = (lo_x, lo_y, hi_x, hi_y)) ∩ (the half-plane
    (x − pos_i)·normals[i] >= 0 where normals[i] != 0), once per mesh.  `grid`: the cloud's cell grid (`synthetic._bin_cloud` of the
    node positions); normals float64 [N, 2] in the caller's node order or None.  Returns (area float64 [N], centroid float64 [N, 2],
    nvert int32 [N], flags uint8 [N] — bits `_lib.VORONOI_BOX / _WALL / _DUPLICATE / _OVERFLOW` —, rings int32 [N]) in the caller's node
    order; `out`: the five tensors to write into.  include/g4c.h has the construction; a cell of more than `_lib.VORONOI_MAX_VERTS`
    vertices gets OVERFLOW and the area +0."""
    what = "voronoi_cells"
    a = Args(what)
    if isinstance(grid, dict):          # (this launch's own conditions on the grid as a whole go in front of cell_grid's tensor checks)
        if "periods" in grid:
            raise ValueError(f"grid: {what}: a periodic grid (control volumes on periodic axes are out of scope)")
        if int(grid.get("dim", 2)) != 2:
            raise ValueError(f"grid: {what} is 2-D only, the cloud has {grid['dim']} dimensions (3-D cells are out of scope)")
    _, n, cells = a.cell_grid(grid)
    if len(cells) != 3 or not all(c >= 1 for c in cells) or cells[2] != 1:
        raise ValueError(f"grid['n_cells']: {what}: expected [nx, ny, 1] cells, got {cells!r}")
    a.cell_start(grid, cells)
    box = _box_arg(what, box)
    if normals is not None:
        a.tensor(normals, "normals", torch.float64, shape=(n, 2))
    shapes = (("out[0]", torch.float64, (n,)), ("out[1]", torch.float64, (n, 2)), ("out[2]", torch.int32, (n,)),
              ("out[3]", torch.uint8, (n,)), ("out[4]", torch.int32, (n,)))
    if out is not None:
        if not isinstance(out, (tuple, list)) or len(out) != 5:
            raise ValueError(f"out: {what}: expected the five tensors (area, centroid, nvert, flags, rings)")
        for (name, dtype, shape), t in zip(shapes, out):
            a.tensor(t, name, dtype, shape=shape)
    dev = a.same_device(("grid", grid["pos_sorted"]), ("grid['order']", grid["order"]), ("grid['cell_start']", grid["cell_start"]),
                        ("normals", normals), *((name, t) for (name, _, _), t in zip(shapes, out or ())))
    if out is None:
        out = tuple(torch.zeros(shape, dtype=dtype, device=dev) for _, dtype, shape in shapes)
    area, centroid, nvert, flags, rings = out
    vc = _lib.g4c_voronoi_cells_t(pos_sorted=_lib.ptr(grid["pos_sorted"]), order=_lib.ptr(grid["order"]), cell_start=_lib.ptr(grid["cell_start"]),
                                  n_cells=(C.c_int32 * 3)(*cells), origin=grid["org"], cell_size=float(grid["h"]),
                                  box_lo=(C.c_double * 2)(box[0], box[1]), box_hi=(C.c_double * 2)(box[2], box[3]), normals=_lib.ptr(normals),
                                  area=_lib.ptr(area), centroid=_lib.ptr(centroid), nvert=_lib.ptr(nvert), flags=_lib.ptr(flags),
                                  rings=_lib.ptr(rings))
    _lib.check(_lib.load().g4c_voronoi_cells(C.byref(vc), n, _lib.stream_handle(dev)))
    return area, centroid, nvert, flags, rings


def integral_program(entries, nz: Optional[int] = None) -> "_lib.g4c_integral_program_t":
    """The program of `weighted_integrals`: 1 .. `_lib.INTEGRALS_MAX_ENTRIES` entries (a, b) — the sum of w · z[a] · z[b]; a column of −1
    stands for 1, so (a, −1) is the integral of z[a] and (−1, −1) the sum of the weights — over samples of `nz` columns.  A program that
    is one already is checked against nz and returned."""
    if isinstance(entries, _lib.g4c_integral_program_t):
        pairs = [(int(entries.a[e]), int(entries.b[e])) for e in range(int(entries.ne))]
    else:
        try:
            pairs = [tuple(e) for e in entries]
        except TypeError:
            raise ValueError(f"entries: expected a sequence of column pairs (a, b), got {entries!r}") from None
    if not 1 <= len(pairs) <= _lib.INTEGRALS_MAX_ENTRIES:
        raise ValueError(f"entries: expected 1 .. {_lib.INTEGRALS_MAX_ENTRIES} pairs (a, b), got {len(pairs)}")
    if nz is not None:
        _plain.integer(nz, "nz", at_least=1)
    for e, pair in enumerate(pairs):
        if len(pair) != 2 or not all(isinstance(c, int) and not isinstance(c, bool) and c >= -1 for c in pair):
            raise ValueError(f"entries: entry {e}: expected two columns (a, b), each >= 0 or −1 (the constant 1), got {pair!r}")
        if nz is not None and max(pair) >= nz:
            raise ValueError(f"entries: entry {e}: column {max(pair)} of samples with {nz} columns")
    if isinstance(entries, _lib.g4c_integral_program_t):
        return entries
    p = _lib.g4c_integral_program_t(ne=len(pairs))
    for e, (a, b) in enumerate(pairs):
        p.a[e], p.b[e] = a, b
    return p


def weighted_integrals_scratch(n_nodes: int, ne: int, device) -> Tensor:
    """The `scratch` buffer of `weighted_integrals` for n_nodes rows and ne entries (g4c_weighted_integrals_scratch_doubles)."""
    return torch.zeros(_scratch_doubles("g4c_weighted_integrals_scratch_doubles", n_nodes, ne), dtype=torch.float64, device=device)


def _integrals_source(a: Args, x, name: str, n_nodes: Optional[int], nz: int, x_step: int, max_steps: int):
    """A source of weighted_integrals: float32 [N, >= nz] (x_step 0) or [N, >= x_step max_steps] (x_step >= nz), rows of unit stride ->
    (N, its leading dimension)."""
    a.dtype(x, name, torch.float32)
    if isinstance(x_step, bool) or not isinstance(x_step, int) or not (x_step == 0 or x_step >= nz):
        raise a.fail(f"{name}_step", f"expected 0 (one step) or the columns of a step >= nz = {nz}, got {x_step!r}")
    n, _, ld = a.strided_rows(x, name, rows=n_nodes, min_cols=nz if x_step == 0 else x_step * max_steps)
    return n, ld


def weighted_integrals(x: Tensor, w: Tensor, entries, stats: Tensor, scratch: Tensor, *, nz: Optional[int] = None, sub: Optional[Tensor] = None,
                       x_step: int = 0, sub_step: int = 0, step: Optional[Tensor] = None, t: int = 0) -> Tensor:
    """g4c_weighted_integrals: stats[t, e] = Σ_i w[i] · z_i[a_e] · z_i[b_e] over the entries (a_e, b_e) of `entries` (`integral_program`).
    The sample z_i is x[i, x_step t : x_step t + nz] — x float32 [N, >= nz] with x_step 0 (a prediction, the derived columns), or
    [N, >= x_step max_steps] with x_step = the columns of a step (a target holding every step) — or, with `sub` (same rules, sub_step),
    that minus sub's, the difference formed in fp64.  nz defaults to x's columns (x_step 0) or x_step.  w float64 [N]: a row of weight 0
    contributes nothing whatever it holds.  stats float64 [max_steps, ne] (row t overwritten), scratch from
    `weighted_integrals_scratch`.  The step index is `step[0]` (int32, read on the device, never written) or, without `step`, `t`;
    a step outside 0 <= t < max_steps writes nothing.  fp64 sums in a fixed order, no atomics: the bits are a function of the data
    alone.  Returns stats."""
    what = "weighted_integrals"
    if nz is None:
        nz = x_step if (isinstance(x_step, int) and x_step > 0) else (int(x.size(1)) if torch.is_tensor(x) and x.dim() == 2 else 0)
    a = Args(what)
    a.integer(nz, "nz", at_least=1)
    prog = integral_program(entries, nz)
    ne = int(prog.ne)
    a.tensor(stats, "stats", torch.float64, dim=2)
    if int(stats.size(1)) != ne:
        raise ValueError(f"stats: {what}: expected [max_steps, ne = {ne}], got shape {tuple(stats.shape)}")
    max_steps = int(stats.size(0))
    n_nodes, x_ld = _integrals_source(a, x, "x", None, nz, x_step, max_steps)
    sub_ld = 0
    if sub is not None:
        _, sub_ld = _integrals_source(a, sub, "sub", n_nodes, nz, sub_step, max_steps)
    a.tensor(w, "w", torch.float64, shape=(n_nodes,))
    a.scratch(scratch, "scratch", record_scratch_doubles(n_nodes, ne), "weighted_integrals_scratch")
    if step is not None:
        a.step_index(step)
    else:
        a.integer(t, "t")
    dev = a.same_device(("x", x), ("sub", sub), ("w", w), ("stats", stats), ("scratch", scratch), ("step", step))
    wi = _lib.g4c_weighted_integrals_t(x=_lib.ptr(x), x_ld=x_ld, x_step=x_step, sub=_lib.ptr(sub), sub_ld=sub_ld, sub_step=sub_step, nz=nz,
                                       w=_lib.ptr(w), step=_lib.ptr(step), t_host=int(t), max_steps=max_steps, stats=_lib.ptr(stats),
                                       scratch=_lib.ptr(scratch))
    _lib.check(_lib.load().g4c_weighted_integrals(C.byref(wi), C.byref(prog), n_nodes, _lib.stream_handle(dev)))
    return stats


def weighted_integrals_adjoint(x: Tensor, w: Tensor, entries, g: Tensor, *, nz: Optional[int] = None, sub: Optional[Tensor] = None,
                               x_step: int = 0, sub_step: int = 0, t: int = 0, group: Optional[Tensor] = None,
                               out: Optional[Tensor] = None) -> Tensor:
    """g4c_weighted_integrals_adjoint: the transpose of `weighted_integrals`' map x -> I[q, e] = Σ_{i in group q} w[i] · z_i[a_e] · z_i[b_e],
    applied to g float64 [G, ne] (on the device, never read on the host): gx float32 [N, nz],
        gx[i, c] = Σ_e g[q_i, e] · w[i] · ([a_e == c] · z_i[b_e] + [b_e == c] · z_i[a_e])
    in fp64 in the order of include/g4c.h, rounded to float32 once.  x, sub, nz, x_step, sub_step mean what they mean in
    `weighted_integrals`; the step is `t` (host-given: training is not captured) and a strided source needs the columns of steps
    0 .. t.  `group` int32 [N]: the group of every row (None: all rows in group 0, G == 1); a row of weight 0, or of a group outside
    [0, G), is +0 in every column whatever it holds.  One thread per (node, column), no atomics: the same bits on every run.  `out`:
    a caller-owned gx, float32 [N, nz] with rows of unit stride (a view of wider rows is fine: only its nz columns are written).
    Returns gx."""
    what = "weighted_integrals_adjoint"
    if nz is None:
        nz = x_step if (isinstance(x_step, int) and x_step > 0) else (int(x.size(1)) if torch.is_tensor(x) and x.dim() == 2 else 0)
    a = Args(what)
    a.integer(nz, "nz", at_least=1)
    prog = integral_program(entries, nz)
    ne = int(prog.ne)
    a.integer(t, "t", at_least=0, at_most=2 ** 31 - 2)
    max_steps = t + 1
    n_nodes, x_ld = _integrals_source(a, x, "x", None, nz, x_step, max_steps)
    sub_ld = 0
    if sub is not None:
        _, sub_ld = _integrals_source(a, sub, "sub", n_nodes, nz, sub_step, max_steps)
    a.tensor(w, "w", torch.float64, shape=(n_nodes,))
    a.tensor(g, "g", torch.float64, dim=2)
    n_groups = int(g.size(0))
    if int(g.size(1)) != ne or n_groups < 1 or n_groups >= 2 ** 31:
        raise ValueError(f"g: {what}: expected [G >= 1, ne = {ne}], got shape {tuple(g.shape)}")
    if group is not None:
        a.tensor(group, "group", torch.int32, shape=(n_nodes,))
    elif n_groups != 1:
        raise ValueError(f"g: {what}: {n_groups} groups of rows need group= (without it every row is in group 0)")
    if out is not None:
        _, _, gx_ld = a.strided_rows(out, "out", rows=n_nodes, cols=nz)
        a.distinct_storage(out, "out", ("x", x), ("sub", sub), ("w", w), ("g", g), ("group", group), identity=True)
    dev = a.same_device(("x", x), ("sub", sub), ("w", w), ("g", g), ("group", group), ("out", out))
    if out is None:
        out, gx_ld = torch.empty((n_nodes, nz), dtype=torch.float32, device=dev), nz
    wa = _lib.g4c_weighted_integrals_adjoint_t(x=_lib.ptr(x), x_ld=x_ld, x_step=x_step, sub=_lib.ptr(sub), sub_ld=sub_ld, sub_step=sub_step,
                                               nz=nz, w=_lib.ptr(w), g=_lib.ptr(g), n_groups=n_groups, group=_lib.ptr(group), t_host=t,
                                               max_steps=max_steps, gx=_lib.ptr(out), gx_ld=gx_ld)
    _lib.check(_lib.load().g4c_weighted_integrals_adjoint(C.byref(wa), C.byref(prog), n_nodes, _lib.stream_handle(dev)))
    return out


def _snapshot_rows(a: Args, x, name: str):
    """A snapshot matrix float32 [rows >= 1, L >= 1] (or [rows, N, nf], read as L = N nf), contiguous -> (rows, L)."""
    a.dtype(x, name, torch.float32)
    if x.dim() not in (2, 3) or int(x.size(0)) < 1 or x.numel() == 0:
        raise a.fail(name, f"expected snapshots [rows >= 1, L >= 1] or [rows, N, nf], got shape {tuple(x.shape)}")
    if not x.is_contiguous():
        raise a.fail(name, f"needs step-major contiguous snapshots, got shape {tuple(x.shape)} strides {tuple(x.stride())}")
    rows, L = int(x.size(0)), x.numel() // int(x.size(0))
    if L > _lib.SNAPSHOT_MAX_COLUMNS:
        raise a.fail(name, f"L = {L} values in a snapshot (at most {_lib.SNAPSHOT_MAX_COLUMNS})", NotImplementedError)
    return rows, L


def _snapshot_sel(what: str, sel, name: str, rows: int) -> "_lib.g4c_snapshot_sel_t":
    """(first, stride, count) — None: every row — against a buffer of `rows` snapshots."""
    if sel is None:
        sel = (0, 1, rows)
    if not isinstance(sel, (tuple, list)) or len(sel) != 3 or any(isinstance(v, bool) or not isinstance(v, int) for v in sel):
        raise TypeError(f"{name}: {what}: expected (first, stride, count) as three integers, got {sel!r}")
    first, stride, count = sel
    if first < 0 or stride < 1 or count < 1 or first + (count - 1) * stride >= rows:
        raise ValueError(f"{name}: {what}: first = {first} (>= 0), stride = {stride} (>= 1), count = {count} (>= 1) select rows up to "
                         f"{first + (count - 1) * stride} of {rows} snapshots")
    return _lib.g4c_snapshot_sel_t(rows=rows, first=first, stride=stride, count=count)


def _snapshot_vector(a: Args, t, name: str, L: int, dev) -> None:
    """An optional float64 [L] (or [N, nf] with N nf = L), contiguous, on the snapshots' device."""
    if t is None:
        return
    a.dtype(t, name, torch.float64)
    if t.numel() != L or not t.is_contiguous():
        raise a.fail(name, f"expected {L} contiguous values, got shape {tuple(t.shape)} strides {tuple(t.stride())}")
    if t.device != dev:
        raise a.fail(name, f"on '{t.device}', the snapshots are on '{dev}'")


def snapshot_mean(x: Tensor, sel=None, out: Optional[Tensor] = None) -> Tensor:
    """g4c_snapshot_mean: the fp64 mean over the selected snapshots of every column, float64 [L] — the rows first, first + stride, ...
    (sel = (first, stride, count); None: all) of x float32 [rows, L] (or [rows, N, nf]) added in slot order, one division: bit for
    bit the plain fp64 loop."""
    what = "snapshot_mean"
    a = Args(what, TypeError)
    rows, L = _snapshot_rows(a, x, "x")
    s = _snapshot_sel(what, sel, "sel", rows)
    dev = x.device
    _snapshot_vector(a, out, "out", L, dev)
    _lib.require_hip(x)
    if out is None:
        out = torch.empty(L, dtype=torch.float64, device=dev)
    _lib.check(_lib.load().g4c_snapshot_mean(_lib.ptr(x), C.byref(s), L, _lib.ptr(out), _lib.stream_handle(dev)))
    return out


def _gram_symmetric(a, mean_a, sa, b, mean_b, sb) -> bool:
    same_mean = (mean_a is None and mean_b is None) or (mean_a is not None and mean_b is not None and mean_a.data_ptr() == mean_b.data_ptr())
    return (a.data_ptr() == b.data_ptr() and same_mean and (sa.first, sa.stride, sa.count) == (sb.first, sb.stride, sb.count))


def snapshot_gram_scratch_bytes(Ma: int, Mb: int, L: int, symmetric: bool) -> int:
    """g4c_snapshot_gram_scratch_bytes: what one g4c_snapshot_gram launch of these sizes writes into its scratch, in bytes."""
    n = int(_lib.load().g4c_snapshot_gram_scratch_bytes(int(Ma), int(Mb), int(L), 1 if symmetric else 0))
    if n < 0:
        raise NotImplementedError(f"snapshot_gram: Ma = {Ma}, Mb = {Mb} (1 .. {_lib.SNAPSHOT_MAX_ROWS}, equal in the symmetric form), L = {L} "
                                  f"(1 .. {_lib.SNAPSHOT_MAX_COLUMNS})")
    return n


def snapshot_gram(a: Tensor, b: Optional[Tensor] = None, *, mean_a: Optional[Tensor] = None, mean_b: Optional[Tensor] = None, sel_a=None,
                  sel_b=None, w: Optional[Tensor] = None, out: Optional[Tensor] = None, scratch: Optional[Tensor] = None) -> Tensor:
    """g4c_snapshot_gram: G[i][j] = Σ_l w[l] (a_i[l] − mean_a[l]) (b_j[l] − mean_b[l]) in fp64, float64 [Ma, Mb], over the selected rows
    of a, b float32 [rows, L] (b None: b = a with a's mean and selection — the symmetric form, whose G is symmetric bit for bit).
    mean_* float64 [L] or None (no centring), w float64 [L] or None (ones).  The order of the sum is a function of (Ma, Mb, L) alone.
    out: float64 [Ma, Mb] with rows of unit stride; scratch: a contiguous uint8 / float64 buffer of at least
    `snapshot_gram_scratch_bytes` bytes (allocated here when None)."""
    what = "snapshot_gram"
    a_ = Args(what, TypeError)
    if b is None:
        if mean_b is not None or sel_b is not None:
            raise ValueError(f"mean_b: {what}: mean_b / sel_b were given without b")
        b, mean_b, sel_b = a, mean_a, sel_a
    rows_a, L = _snapshot_rows(a_, a, "a")
    rows_b, Lb = _snapshot_rows(a_, b, "b")
    if Lb != L:
        raise ValueError(f"b: {what}: snapshots of {Lb} values, a's hold {L}")
    sa, sb = _snapshot_sel(what, sel_a, "sel_a", rows_a), _snapshot_sel(what, sel_b, "sel_b", rows_b)
    for s, name in ((sa, "sel_a"), (sb, "sel_b")):
        if s.count > _lib.SNAPSHOT_MAX_ROWS:
            raise NotImplementedError(f"{name}: {what}: {s.count} snapshots (at most {_lib.SNAPSHOT_MAX_ROWS})")
    dev = a.device
    if b.device != dev:
        raise ValueError(f"b: {what}: on '{b.device}', a is on '{dev}'")
    for t, name in ((mean_a, "mean_a"), (mean_b, "mean_b"), (w, "w")):
        _snapshot_vector(a_, t, name, L, dev)
    ld = sb.count
    if out is not None:
        if torch.is_tensor(out) and out.device != dev:
            raise TypeError(f"out: {what}: on '{out.device}', a is on '{dev}'")
        _, _, ld = a_.strided_rows(out, "out", torch.float64, rows=sa.count, cols=sb.count)
    # (g4c_snapshot_gram_scratch_bytes restated, so that a scratch that is too small is refused before the library is touched)
    nbi, nbj = -(-sa.count // _lib.SNAPSHOT_GRAM_BLOCK), -(-sb.count // _lib.SNAPSHOT_GRAM_BLOCK)
    blocks = nbi * (nbi + 1) // 2 if _gram_symmetric(a, mean_a, sa, b, mean_b, sb) else nbi * nbj
    need = 8 * _lib.SNAPSHOT_GRAM_BLOCK ** 2 * blocks * -(-L // _lib.SNAPSHOT_GRAM_CHUNK)
    if scratch is not None and (not torch.is_tensor(scratch) or scratch.device != dev or not scratch.is_contiguous()
                                or scratch.numel() * scratch.element_size() < need or scratch.data_ptr() % 8):
        raise ValueError(f"scratch: {what}: expected a contiguous 8-byte aligned buffer of at least {need} bytes on '{dev}'")
    _lib.require_hip(a, b)
    if out is None:
        out = torch.empty((sa.count, sb.count), dtype=torch.float64, device=dev)
    if scratch is None:
        scratch = torch.empty(need // 8, dtype=torch.float64, device=dev)
    _lib.check(_lib.load().g4c_snapshot_gram(_lib.ptr(a), _lib.ptr(mean_a), C.byref(sa), _lib.ptr(b), _lib.ptr(mean_b), C.byref(sb), _lib.ptr(w),
                                             L, _lib.ptr(out), ld, _lib.ptr(scratch), _lib.stream_handle(dev)))
    return out


def snapshot_combine(x: Tensor, coef: Tensor, *, mean: Optional[Tensor] = None, sel=None, out: Optional[Tensor] = None) -> Tensor:
    """g4c_snapshot_combine: out[r][l] = (float) Σ_i coef[i][r] ((double)x_i[l] − mean[l]), float32 [R, L], over the selected rows of x
    float32 [rows, L] in slot order; coef float64 [count, R] with rows of unit stride (on the device), mean float64 [L] or None.
    Product and sum are rounded separately: bit for bit a plain fp64 loop rounded once to fp32."""
    what = "snapshot_combine"
    a = Args(what, TypeError)
    rows, L = _snapshot_rows(a, x, "x")
    s = _snapshot_sel(what, sel, "sel", rows)
    dev = x.device
    _, R, ldc = a.strided_rows(coef, "coef", torch.float64, rows=s.count)
    if coef.device != dev:
        raise ValueError(f"coef: {what}: on '{coef.device}', the snapshots are on '{dev}'")
    if R > _lib.SNAPSHOT_MAX_ROWS or s.count > _lib.SNAPSHOT_MAX_ROWS:
        raise NotImplementedError(f"coef: {what}: {s.count} snapshots into {R} combinations (at most {_lib.SNAPSHOT_MAX_ROWS} each)")
    _snapshot_vector(a, mean, "mean", L, dev)
    if out is not None:
        if torch.is_tensor(out) and out.device != dev:
            raise TypeError(f"out: {what}: on '{out.device}', the snapshots are on '{dev}'")
        a.tensor(out, "out", torch.float32)
        if out.numel() != R * L or int(out.size(0)) != R:
            raise ValueError(f"out: {what}: expected a contiguous [{R}, {L}], got shape {tuple(out.shape)}")
    _lib.require_hip(x)
    if out is None:
        out = torch.empty((R, L), dtype=torch.float32, device=dev)
    _lib.check(_lib.load().g4c_snapshot_combine(_lib.ptr(x), _lib.ptr(mean), C.byref(s), _lib.ptr(coef), ldc, R, L, _lib.ptr(out),
                                                _lib.stream_handle(dev)))
    return out


def steps_to_columns(out_steps: Tensor) -> Tensor:
    """Step-major rollout outputs [steps, n_nodes, nf] -> the reference's layout [n_nodes, nf * steps] (nn/model.py:322-326)."""
    return out_steps.permute(1, 0, 2).reshape(out_steps.size(1), -1)


# Arithmetic of the fused MLPs — all fp32 in, fp32 out:
#   "f16x3" (default)   fp32-class products on the f16 matrix pipe: both operands split two ways into fp16 terms,
#                       x = h + l * 2^-11 (22 significand bits), three partial products, the 2^-11 terms in their own fp32
#                       accumulator (G4C_WFMT_F16X2); measured error against fp64
#                       below that of the fp32-MFMA kernel (scripts/mlp_accuracy.py, test_mlp_precisions_vs_fp64).  Range: fp16's — an MLP
#                       input or hidden activation beyond +-65504 is clipped there (no inf / NaN) AND FLAGGED on the device (the WEIGHTS
#                       are converted when the image is packed, unclipped and unflagged: PackedMLP raises ValueError for a weight of
#                       magnitude >= 65504 — check_weight_range); the
#                       arithmetic is run optimistically: a rollout reads its flags where it hands out results (Rollout.validate) and
#                       recomputes itself in "bf16x6" if anything was clipped, so solve() never returns a clipped value (normalised CFD
#                       fields and LayerNorm'd latents are far inside the range; raw inputs only pass the fp32 vector path);
#   "bf16x6"            the same kernels with both operands split EXACTLY into three bf16 terms (fp32 exponent range), the six
#                       largest partial products accumulated in fp32 (G4C_WFMT_BF16X3): twice the matrix-pipe work;
#                       MLPs outside the envelope of these two (an input block wider than 128) use the fp32 kernels;
#   "fp32"              v_mfma_f32_32x32x2_f32 (G4C_WFMT_FP32): the original kernel;
#   "bf16"              operands ROUNDED to bf16 (~1e-2 deviation): BASELINE config 3's "bf16 edge-MLP MFMA", opt-in only.
PRECISIONS = ("fp32", "bf16", "bf16x6", "f16x3")
_PRECISION = os.environ.get("G4C_MLP_PRECISION", "f16x3")


# Fused aggregation in the edge-MLP launch (g4c_mlp_io_t.agg): bit-identical to the separate g4c_segment_reduce, and the
# node launch no longer re-reads the 307 MB of messages (the largest single stream of a level-1 MP layer after the messages'
# own write).  The launch then runs on tiles of WHOLE segments: with in-degree 6 (or 5) a 32-row tile holds 30 rows, i.e.
# 6.7 % more tiles — speed-neutral on the 100k rollout (+0.8 %), 2.5 GB less traffic per step.  On from FUSE_AGG_MIN_ROWS
# rows (below, launches are latency-bound and the row tiles of whole segments only cost).  (Module attributes, not environment
# switches: the A/B runs that fixed them are in DESIGN.md / HISTORY.md; tests flip them directly.)
FUSE_AGG = True
FUSE_AGG_MIN_ROWS = 50000
# Aggregation on load (g4c_src_t.seg_off): the node-MLP launch averages each target's messages while it gathers its input,
# instead of a separate g4c_segment_reduce pass (bit-identical values; no tile-alignment constraint, unlike FUSE_AGG).
AGG_ON_LOAD = True
# below this many rows to aggregate, the launch that gathers them is latency-bound and a separate g4c_segment_reduce is quicker
# (same-box sweep: 12.5k-node 3-scale mesh 789 -> 822 steps/s, 2-scale 10k nodes 1079 -> 1110, 25k nodes 503 -> 516 with the
# threshold at 50k rows; neutral at 100k nodes)
AGG_ON_LOAD_MIN_ROWS = 50000


# ---- fp16 range of the "f16x3" arithmetic made observable: a kernel that converted a value of magnitude >= 65504 to fp16 (it was
# clipped there) writes 1 into the slot of its MLP (g4c_mlp_t.range_slot) of the int32 flag buffer its launch names
# (g4c_mlp_io_t.range_flag).  Slots are named after the MLP that launched ("NsThreeScaleGNN.mp112.edge_mlp").  The flags a launch
# writes belong to whoever issued it: a consumer — a `Rollout`, a `DistributedRollout`, a validated bare model.forward() — owns a
# RangeFlags buffer and issues its launches inside its scope, reads it where it hands out results (one synchronisation) and RECOMPUTES
# in "bf16x6" if anything was clipped (Rollout.validate, hence Model.solve; DistributedRollout.validate; nn/model.py:
# GNN.__init_subclass__).  Everything launched outside a consumer — training, forwards with validation off or inside a caller's own
# capture, scripts — writes into its device's default buffer: f16_range_report() reads it, check_f16_range() turns a non-empty report
# into a RuntimeWarning (GNN.fit: once per epoch).
RANGE_SLOTS = 4096
_range_bufs = {}            # device -> int32 [RANGE_SLOTS]: the default buffer (created when the first f16x3 MLP is packed there)
_range_sites: List[set] = [set() for _ in range(RANGE_SLOTS)]
_range_slot_of = {}
_range_wrapped = False


def _range_buffer(dev: torch.device) -> Tensor:
    buf = _range_bufs.get(dev)
    if buf is None:
        buf = _range_bufs[dev] = torch.zeros(RANGE_SLOTS, dtype=torch.int32, device=dev)
    return buf


def _range_slot(site: str) -> int:
    global _range_wrapped
    slot = _range_slot_of.get(site)
    if slot is None:
        n = len(_range_slot_of)
        if n >= RANGE_SLOTS and not _range_wrapped:
            _range_wrapped = True
            import warnings
            warnings.warn(f"more than {RANGE_SLOTS} named MLP sites: fp16 range flags are shared between sites from here on "
                          "(a clip is then reported under every name that shares its slot)", RuntimeWarning)
        slot = _range_slot_of[site] = n % RANGE_SLOTS
        _range_sites[slot].add(site)
    return slot


def _indexed(device) -> Optional[torch.device]:
    """torch.device('cuda') / 'cuda' name the CURRENT device: the flag buffers are keyed by indexed devices."""
    if device is None:
        return None
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def _read_flags(buf: Tensor) -> List[Tuple[int, str]]:
    """(slot, site name) of every set word of a flag buffer: its one device -> host copy (synchronises)."""
    slots = torch.nonzero(buf.cpu()).flatten().tolist()
    return [(slot, name) for slot in slots for name in sorted(_range_sites[slot]) or [f"slot {slot}"]]


class RangeFlags:
    """The fp16 range flags of one consumer: an int32 [RANGE_SLOTS] buffer on its device.  Every f16x3 launch on that device issued
    inside `with flags:` writes into it (the innermost scope wins; a hipGraph captured there keeps the pointer), so `take()` answers
    for exactly the launches this consumer issued, before or after it is done with them."""
    active: Optional["RangeFlags"] = None

    def __init__(self, device):
        self.buf = torch.zeros(RANGE_SLOTS, dtype=torch.int32, device=device)
        self.device = self.buf.device
        self._prev = None

    def __enter__(self):
        self._prev, RangeFlags.active = RangeFlags.active, self
        return self

    def __exit__(self, *exc):
        RangeFlags.active = self._prev
        return False

    def take(self) -> List[str]:
        """Names of the MLPs whose launches in this scope clipped a value since the last take (one synchronisation; the buffer is
        cleared only if something was set)."""
        hits = _read_flags(self.buf)
        if hits:
            self.buf.zero_()
        return sorted({name for _, name in hits})


def _launch_flags(dev: torch.device) -> Tensor:
    """The buffer an f16x3 launch on `dev` reports into: the innermost active consumer's if it is on `dev`, else the default one."""
    c = RangeFlags.active
    return c.buf if c is not None and c.device == dev else _range_buffer(dev)


def f16_range_clear(device: Optional[torch.device] = None, sites=None) -> None:
    """Forget the recorded clips of launches outside any consumer: every site, or only `sites` (names as in f16_range_report).
    Synchronises."""
    f16_range_report(device, clear=True, sites=sites)


def f16_range_report(device: Optional[torch.device] = None, clear: bool = True, sites=None) -> List[str]:
    """Names of the MLPs whose launches outside any consumer (the default buffers: training, forwards with validation off, scripts)
    clipped a value at the end of the fp16 range since the last report / clear (all devices, or one; `sites`: only these names are
    looked at and cleared).  Synchronises with the device(s)."""
    device = _indexed(device)
    only = None if sites is None else set(sites)
    names: List[str] = []
    for dev, buf in list(_range_bufs.items()):
        if device is not None and device != dev:
            continue
        hits = [(slot, name) for slot, name in _read_flags(buf) if only is None or name in only]
        if clear and hits:
            buf[[slot for slot, _ in hits]] = 0
        names += sorted(name for _, name in hits)
    return names


def check_f16_range(device: Optional[torch.device] = None, where: str = "", sites=None) -> List[str]:
    """RuntimeWarning when a launch in the "f16x3" arithmetic clipped an MLP input or hidden activation at +-65504 (the reference
    computes these in fp32: nn/model.py:303-321).  Returns the offending MLPs' names.  `sites`: see f16_range_report."""
    hit = f16_range_report(device, sites=sites)
    if hit:
        import warnings
        warnings.warn(f"{where + ': ' if where else ''}the 'f16x3' MLP arithmetic clipped values at the end of the fp16 range (|x| >= 65504) in "
                      f"{', '.join(hit[:8])}{' ...' if len(hit) > 8 else ''}: the result differs from an fp32 evaluation.  "
                      "gfd.set_mlp_precision('bf16x6') keeps fp32's exponent range.", RuntimeWarning, stacklevel=2)
    return hit


# ---- pack-time range proof.  Almost every value the V-cycle converts to fp16 is SELU(LayerNorm(.)) or a bounded linear image of such
# values, so a bound far below 65504 follows from the weights alone.  PackedMLP reads the norms of its weights back once, when the image
# is packed (PackedMLP.norms: recomputed exactly when the image is rebuilt); a launch joins them with the bounds its Sources carry
# (range_bounds) and, when the proof succeeds, passes g4c_mlp_t.range_certified: the library then runs the kernel instantiation without
# the range tracker.  Everything here is host arithmetic on Python floats (fp64): no device synchronisation per launch.
RANGE_PROOFS = True                     # (tests / A-B: False tracks every launch, as before)
SELU_SCALE = 1.0507009873554804934193349852946
SELU_FLOOR = 1.0507009873554804934193349852946 * 1.6732632423543772848170429916717       # |selu(x)| < scale * alpha for x < 0
F16_RANGE_END = 65504.0


def act_bound(bound: Optional[float], act: int) -> Optional[float]:
    """Bound on |act(x)| given |x| <= bound (None: unknown).  tanh is bounded whatever its argument."""
    if act == _lib.ACT_TANH:
        return 1.0
    if bound is None:
        return None
    if act == _lib.ACT_SELU:          # x >= 0: scale * x;  x < 0: inside (-scale * alpha, 0)
        return max(SELU_SCALE * bound, SELU_FLOOR)
    return bound


def certifies(converted_bound: Optional[float]) -> bool:
    """The certificate is given only when TWICE the bound stays below the end of fp16's range: the bound is on the exactly computed
    activations, the kernels convert the f16x3-computed ones, which differ from them by ~1e-6 relative — a factor 2 covers that (and
    the rounding of this fp64 evaluation) many times over."""
    return converted_bound is not None and converted_bound == converted_bound and 2.0 * converted_bound < F16_RANGE_END


def weight_norms(weights: Sequence[Tensor], biases: Sequence[Optional[Tensor]], ln: Optional[Tuple[Tensor, Tensor, float]],
                 heads: Sequence[Tensor], seg_widths: Sequence[int], narrow: Optional[Sequence[bool]] = None) -> dict:
    """The norms range_bounds needs, evaluated in fp64 where the weights live and read back in ONE copy (an image is packed in an eager
    step, never inside a capture): per weighted (not narrow) input block of the first layer, per later layer and per head the largest
    row sum of |W|; max|b| per layer; max|gamma|, max|beta| of the LayerNorm; and, for the same matrices in the same order ("w0_max",
    "w_max", "heads_max"), max|W| — the weights of an f16x3 image are converted to fp16 when it is packed (check_weight_range)."""
    narrow = tuple(bool(x) for x in narrow) if narrow is not None else (False,) * len(seg_widths)

    def rowsum(W: Tensor) -> Tensor:
        return W.detach().to(torch.float64).abs().sum(1).max()

    def largest(W: Tensor) -> Tensor:
        return W.detach().to(torch.float64).abs().max() if W.numel() else torch.zeros((), dtype=torch.float64, device=W.device)
    W0, dev = weights[0], weights[0].device
    vals, col0, n_wide, packed = [], 0, 0, []
    for w_, nar in zip(seg_widths, narrow):
        if not nar:
            packed.append(W0[:, col0:col0 + int(w_)])
            n_wide += 1
        col0 += int(w_)
    packed += list(weights[1:]) + list(heads)
    vals += [rowsum(W) for W in packed]
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    vals += [zero if b is None else b.detach().to(torch.float64).abs().max() for b in biases]
    if ln is not None:
        vals += [ln[0].detach().to(torch.float64).abs().max(), ln[1].detach().to(torch.float64).abs().max()]
    vals += [largest(W) for W in packed]
    it = iter(torch.stack(vals).cpu().tolist())
    nl, nh = len(weights), len(heads)
    norms = {"w0": [next(it) for _ in range(n_wide)], "w": [next(it) for _ in range(nl - 1)], "heads": [next(it) for _ in range(nh)],
             "b": [next(it) for _ in range(nl)]}
    norms["ln"] = (next(it), next(it)) if ln is not None else None
    norms["w0_max"], norms["w_max"], norms["heads_max"] = ([next(it) for _ in range(n_wide)], [next(it) for _ in range(nl - 1)],
                                                           [next(it) for _ in range(nh)])
    norms["n_out"] = int(weights[-1].size(0))
    norms["narrow"] = any(narrow)
    return norms


def check_weight_range(norms: dict, site: str) -> None:
    """An f16x3 image holds its weights as fp16 pairs, converted when it is packed — without the clip and without the flag of the
    activations' conversions: a weight that rounds beyond 65504 is packed as an infinity (measured from |w| = 65520: wrong finite rows,
    flagged only where an activation behind it overflows in turn — a head's weight gives head rows of 3.4e38 and no flag;
    tests/RANGE_SITES_MEASURED.md).  An MLP with |w| >= 65504 cannot run in this arithmetic: ValueError, naming the matrix."""
    for key, what in (("w0_max", "input block {} of the first layer"), ("w_max", "layer {}"), ("heads_max", "head {}")):
        for j, m in enumerate(norms[key]):
            if m >= F16_RANGE_END:          # (a NaN weight is not a range matter: it shows in every row)
                raise ValueError(f"{site}: {what.format(j + 2 if key == 'w_max' else j)} has a weight of magnitude {m:g}, outside the fp16 range "
                                 f"(|w| >= {F16_RANGE_END:g}) of the 'f16x3' MLP arithmetic; set_mlp_precision('bf16x6') keeps fp32's "
                                 "exponent range")


class LaunchBounds:
    """What the range proof of one launch gives: `converted` — bound on every value the launch converts to fp16 (None: no proof),
    `out` — bound on its output rows (after LayerNorm / activation), `heads` — bounds on its head rows, `e` (mp_layer_forward only:
    `out` is v' there) — bound on the message rows; None where unknown."""
    __slots__ = ("converted", "out", "heads", "e")

    def __init__(self, converted=None, out=None, heads=None, e=None):
        self.converted, self.out, self.heads, self.e = converted, out, heads, e

    def head(self, j: int) -> Optional[float]:
        return None if self.heads is None else self.heads[j]


def range_bounds(norms: Optional[dict], sources: Sequence["Source"], act: int, residual: bool = False,
                 seg_len: Optional[int] = None) -> LaunchBounds:
    """The proof for one launch of an MLP with the weight norms `norms` (PackedMLP.norms) on `sources`.
      input that is converted:   act_bound(source.bound, source.pre_act); a mean over rows keeps it, a sum multiplies it by the
                                 longest segment (`seg_len`; unknown: no proof);
      additive rows:             their bound enters layer 0's pre-activation;
      layer l:                   B_l = (largest row sum of |W_l|) . B_{l-1} + max|b_l| (+ additive rows, l = 0); SELU(B_l) is converted
                                 for every layer but the last;
      output rows:               LayerNorm: |y| <= sqrt(n - 1) max|gamma| + max|beta| whatever goes in, else B_last; then `act`;
      heads:                     the output row is converted; head h <= (largest row sum of |W_h|) . out.
    Unknown producers (a source without a bound), narrow blocks multiplied on the vector ALUs, and arithmetics other than f16x3
    (norms None) give no proof."""
    if norms is None:
        return LaunchBounds()
    proof = not norms["narrow"]
    b0, j = norms["b"][0], 0
    converted = 0.0
    for s_ in sources:
        if s_.additive:
            if s_.bound is None:
                proof = False
            else:
                b0 += s_.bound
            continue
        xb = act_bound(s_.bound, s_.pre_act)
        if xb is not None and s_.segments is not None and not s_.seg_mean:
            xb = None if seg_len is None else xb * seg_len
        if xb is None or j >= len(norms["w0"]):
            proof = False
        else:
            converted = max(converted, xb)
            b0 += norms["w0"][j] * xb
        j += 1
    n_layers = len(norms["b"])
    pre = b0 if proof else None          # bound of the current layer's pre-activation
    for l in range(1, n_layers):
        if pre is not None:
            hid = act_bound(pre, _lib.ACT_SELU)
            converted = max(converted, hid)
            pre = norms["w"][l - 1] * hid + norms["b"][l]
    if norms["ln"] is not None:
        g, be = norms["ln"]
        raw = (norms["n_out"] - 1) ** 0.5 * g + be
    else:
        raw = pre
    out = act_bound(raw, act)
    heads = None
    if norms["heads"]:
        if out is None:
            proof = False
        else:
            converted = max(converted, out)
            heads = [h * out for h in norms["heads"]]
    return LaunchBounds(converted if proof else None, None if residual else out, heads)


_last_bounds: Optional[LaunchBounds] = None


def take_bounds() -> LaunchBounds:
    """The proof of the launch that has just been issued through mlp_forward / mp_layer_forward, handed out ONCE: the caller that builds
    the next launch's Source from the tensor it has just received asks here, right behind the call.  Every launch entry point clears
    it first, so a stale answer is never anything but "unknown"."""
    global _last_bounds
    got, _last_bounds = _last_bounds, None
    return got if got is not None else LaunchBounds()


class RangeBounds:
    """The bounds that travel with the latents of one forward, beside the tensors and never on them: of the node latents `v`, of the
    edge latents `e` as stored (their pending activation not applied) and of the hoisted `products`.  A model's forward owns one and
    hands it to its blocks, which read their inputs' bounds from it and leave their outputs' bounds in it; a block called without one
    (GNBlock.forward(v, e, ...) on a user's tensors) knows nothing about its inputs."""
    __slots__ = ("v", "e", "products")

    def __init__(self, v: Optional[float] = None, e: Optional[float] = None, products: Optional[Sequence[Optional[float]]] = None):
        self.v, self.e, self.products = v, e, products

    def product(self, j: int) -> Optional[float]:
        return None if self.products is None else self.products[j]


_weights_epoch = 0


def weights_epoch() -> int:
    """Counter folded into the validity key of every packed-weight image (nn/blocks.py MLP._signature).  The key otherwise
    relies on the parameters' version counters, which in-place updates that bypass autograd's bookkeeping do not advance —
    torch's own `fused=True` optimizers among them (measured: `Adam(fused=True).step()` leaves `p._version` unchanged).  Every
    backward pass through a fused MLP advances the epoch, so the forward after a training step always repacks."""
    return _weights_epoch


def bump_weights_epoch() -> None:
    global _weights_epoch
    _weights_epoch += 1


def grad_mode() -> bool:
    """True when calls are being recorded for autograd: the block / model code then keeps to the plain forms of the
    launches (no heads, no pre-multiplied products, no in-place epilogues), which are the differentiable ones."""
    return torch.is_grad_enabled()


def can_fuse_aggregation(csr: CsrPlan, width: int) -> bool:
    """The edge launch itself can reduce its rows per target (g4c_mlp_io_t.agg): rows in segment order, segments of
    at most 32 rows, the exact-split kernels, a 128-wide output, enough rows to be throughput-bound."""
    return (FUSE_AGG and _PRECISION in ("bf16x6", "f16x3", "bf16") and width == 128 and csr.perm is None and csr.n >= FUSE_AGG_MIN_ROWS
            and not grad_mode() and csr.tiles() is not None)


def can_aggregate_on_load(csr: CsrPlan, width: int, consumer_widths: Sequence[int]) -> bool:
    """`consumer_widths`: input blocks of the MLP that would aggregate while loading (it must run on the bf16x6 kernels)."""
    # (rows in segment order only: through a permutation the kernel supports it too — Source(segments=csr with perm) — but the
    # extra dependent index round trip in the consumer's prologue gives back what the separate reduction costs; measured neutral)
    return (AGG_ON_LOAD and effective_precision(consumer_widths) != "fp32" and csr.perm is None and width == 128
            and csr.n > 0 and csr.n >= AGG_ON_LOAD_MIN_ROWS)


def mlp_precision() -> str:
    return _PRECISION


def effective_precision(seg_widths: Sequence[int]) -> str:
    """Precision an MLP with these input blocks is packed for: the selected one, or fp32 outside the bf16 kernels' envelope."""
    if _PRECISION != "fp32" and any(int(w) > 128 for w in seg_widths):
        return "fp32"
    return _PRECISION


def set_mlp_precision(precision: str) -> str:
    """Select the arithmetic of every fused MLP launched from now on; returns the previous setting."""
    global _PRECISION
    if precision not in PRECISIONS:
        raise ValueError(f"unknown MLP precision {precision!r} ({' | '.join(PRECISIONS)})")
    old, _PRECISION = _PRECISION, precision
    return old


@contextlib.contextmanager
def mlp_precision_as(precision: str):
    """`set_mlp_precision(precision)` for the launches issued inside; the previous setting is put back on the way out."""
    old = set_mlp_precision(precision)
    try:
        yield
    finally:
        set_mlp_precision(old)


TRAIN_PRECISIONS = ("bf16x6", "bf16")
_TRAIN_PRECISION = "bf16x6"


def train_precision() -> str:
    return _TRAIN_PRECISION


SAVED_PRECISIONS = ("fp32", "bf16")
_SAVED_PRECISION = "fp32"


def saved_precision() -> str:
    """The storage format of the rows a recorded forward keeps for the backward (`set_train_precision(..., saved=)`)."""
    return _SAVED_PRECISION


def set_train_precision(precision: str, saved: Optional[str] = None) -> str:
    """Select the arithmetic of the backward pass's matrix products (autograd.py); returns the previous setting.  Independent of
    `set_mlp_precision`, which selects the forward's.
    "bf16x6" (default): input gradients on the exact three-way bf16 split, weight gradients on the fp32 MFMA (g4c_weight_grad).
    "bf16" (mixed-precision training): every product of the backward takes both operands rounded once to bf16 (round to nearest
    even) and accumulates in fp32 — `autograd.linear` / `backward_chain` pack the rounded-bf16 stream, weight gradients run on
    g4c_weight_grad_bf16.  Bias gradients, LayerNorm / activation adjoints, segmented sums and gathers stay fp32.  bf16 has fp32's
    exponent range, so gradient rows of 1e-6 .. 1e-9 need no loss scaling.
    `saved` ("fp32", the meaning of None; or "bf16", with precision "bf16" only): the format of the rows a recorded forward keeps
    for the backward (g4c_mlp_io_t.save).  "bf16": each kept row is stored rounded once to bf16 (nearest even) — half the bytes
    between the passes; every consumer widens it exactly.  As a product operand the row was rounded to bf16 anyway, so weight
    gradients do not move; SELU slopes and the LayerNorm adjoint see the rounding (<= 2^-9 relative).  `saved_precision()` reads
    the setting back."""
    global _TRAIN_PRECISION, _SAVED_PRECISION
    if precision not in TRAIN_PRECISIONS:
        raise ValueError(f"unknown training precision {precision!r} ({' | '.join(TRAIN_PRECISIONS)})")
    saved = "fp32" if saved is None else saved
    if saved not in SAVED_PRECISIONS:
        raise ValueError(f"unknown saved-activation precision {saved!r} ({' | '.join(SAVED_PRECISIONS)})")
    if saved == "bf16" and precision != "bf16":
        raise ValueError(f"saved='bf16' needs the training precision 'bf16' (mixed-precision training), not {precision!r}")
    old, _TRAIN_PRECISION, _SAVED_PRECISION = _TRAIN_PRECISION, precision, saved
    return old


def _rs_k_order(dev) -> Tensor:
    """Column order of the row-split kernel's stream and of its bf16 rows (G4C_ROWS_RS_ORDER): position 32 j + 8 g + 4 h + e holds
    feature 32 j + 16 h + 4 g + e — the eight values a lane of a 16x16x32 MFMA holds of a 32-feature step, side by side."""
    pos = torch.arange(128, device=dev)
    j, g, h, e = pos // 32, (pos % 32) // 8, (pos % 8) // 4, pos % 4
    return 32 * j + 16 * h + 4 * g + e


class RsOrderedRows(Tensor):
    """bf16 [n, 128] rows whose columns are in the row-split kernel's order (`_rs_k_order`): the compact message rows and the hoisted
    product tables its launches exchange (mlp_rs.hip, rounded-bf16 mode).  The subclass is only a tag that travels with the tensor
    (row slices and views keep it): `mlp_forward` hands such rows to that kernel as they are and restores the natural column order
    for every other reader.

    The tag survives only what keeps every row's 128 columns as they are (`_rs_keeps`): row slices / row gathers, views and reshapes to
    [n, 128], contiguous, clone, detach and moves between devices.  Everything else — a column slice, a dtype change, a cat, a column
    gather, arithmetic — returns a plain Tensor: a caller who reorders the columns by hand must not hand the reader a tag that makes it
    reorder them a second time."""

    @staticmethod
    def tag(t: Tensor) -> Tensor:
        if t.dtype != torch.bfloat16 or t.dim() != 2 or t.size(1) != 128:
            raise ValueError("RsOrderedRows: bf16 [n, 128] rows only")
        return t.as_subclass(RsOrderedRows)

    @classmethod
    def __torch_function__(cls, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        with torch._C.DisableTorchFunctionSubclass():
            out = func(*args, **kwargs)
        if not isinstance(out, Tensor):
            if isinstance(out, (tuple, list)):           # (split, chunk, unbind, ...: plain pieces)
                return type(out)(t.as_subclass(Tensor) if isinstance(t, RsOrderedRows) else t for t in out)
            return out
        keep = (_rs_keeps(func, args, kwargs) and out.dtype == torch.bfloat16 and out.dim() == 2 and out.size(1) == 128)
        if keep:
            return out if isinstance(out, RsOrderedRows) else out.as_subclass(RsOrderedRows)
        return out.as_subclass(Tensor) if isinstance(out, RsOrderedRows) else out


def _row_index(ix) -> bool:
    """`t[ix]` selects rows only: an int / slice / index tensor on dim 0, optionally followed by a full `:` on dim 1."""
    if isinstance(ix, tuple):
        if len(ix) == 1:
            return _row_index(ix[0])
        return len(ix) == 2 and _row_index(ix[0]) and isinstance(ix[1], slice) and ix[1] == slice(None)
    return ix is not Ellipsis and ix is not None and not isinstance(ix, int)


def _rs_keeps(func, args, kwargs) -> bool:
    """Whether `func(*args, **kwargs)` keeps each row's columns where they were (RsOrderedRows.__torch_function__)."""
    name = getattr(func, "__name__", "")
    if name in ("contiguous", "clone", "detach", "cuda", "cpu", "to", "view", "reshape", "requires_grad_", "pin_memory"):
        return True
    if name == "__getitem__":
        return _row_index(args[1])
    if name in ("narrow", "index_select"):
        dim = args[1] if len(args) > 1 else kwargs.get("dim")
        return dim == 0
    return False


def rs_rows_to_natural(t: Tensor) -> Tensor:
    """The rows of an RsOrderedRows tensor with their columns in feature order (a copy, plain Tensor)."""
    inv = torch.argsort(_rs_k_order(t.device))
    return t.as_subclass(Tensor).index_select(1, inv)


class PackedMLP:
    """Device-side packed weights of one MLP for a given input block structure."""

    def __init__(self, weights: Sequence[Tensor], biases: Sequence[Tensor], ln: Optional[Tuple[Tensor, Tensor, float]],
                 seg_widths: Sequence[int], seg_negate: Sequence[bool], heads: Sequence[Tensor] = (),
                 precision: str = "fp32", narrow: Optional[Sequence[bool]] = None, site: Optional[str] = None, rs_order: bool = False,
                 rs_blocks: Optional[Sequence[bool]] = None, rs2: int = 0):
        """`heads`: bias-free [128, 128] weights applied to the MLP's final output row (g4c_mlp_io_t heads); their
        packed images continue the weight stream after the last layer.  `precision` "bf16x6" / "f16x3" / "bf16": the three-plane
        bf16 stream (every input block padded to 128 k; "bf16" uses the G4C_WFMT_BF16X3 stream, leading plane only).
        `narrow[s]` (bf16x6 / bf16 only): input block s (<= 8 columns, read without index or activation) is multiplied in
        fp32 on the vector ALUs by its rows of the first layer's weight (g4c_src_t.additive == 2) instead of being padded
        to a 128-k block of the matrix-pipe stream."""
        lib = _lib.load()
        # "f16x3" is the "bf16x6" kernel family (same stream layout and launch envelope) on a stream packed as G4C_WFMT_F16X2;
        # desc.w_format tells the library which arithmetic the stream is for
        self.split = "f16x2" if precision == "f16x3" else ("bf16x3" if precision == "bf16x6" else None)
        if precision == "f16x3":
            precision = "bf16x6"
        self.precision = precision
        bf16 = precision in ("bf16", "bf16x6")
        narrow = tuple(bool(x) for x in narrow) if narrow is not None else (False,) * len(seg_widths)
        if any(narrow) and not bf16:
            raise NotImplementedError("narrow input blocks need the bf16x6 kernels")
        if any(nw and w > _lib.NARROW_MAX for nw, w in zip(narrow, seg_widths)):
            raise ValueError(f"a narrow input block has more than {_lib.NARROW_MAX} columns")
        self.narrow = narrow       # three-plane bf16 weight stream, 128-k input blocks ("bf16" reads plane 0 only)
        planes = 3
        dev = _lib.require_hip(*weights, *[b for b in biases if b is not None], *heads)
        n_layers = len(weights)
        if not 1 <= n_layers <= _lib.MAX_LAYERS:
            raise NotImplementedError(f"MLP with {n_layers} Linear layers (supported: 1..{_lib.MAX_LAYERS})")
        if len(seg_widths) > _lib.MAX_SRC:
            raise NotImplementedError(f"MLP input concatenated from {len(seg_widths)} blocks (max {_lib.MAX_SRC})")
        self.desc = _lib.g4c_mlp_t()
        self.desc.n_layers = n_layers
        # `rs_order` (rounded-bf16 mode, every layer 128 x 128 over ONE 128-wide input block): the stream is written for the row-split
        # kernel (mlp_rs.hip, G4C_WFMT_BF16_RS) — the columns of every layer in the order `_rs_k_order`, the order in which a 16x16x32
        # MFMA leaves a layer's output in the lane that needs it as the next layer's operand.  No other kernel can read such a stream:
        # the library fails a launch outside that kernel's envelope.
        self.rs_order = bool(rs_order)
        if self.rs_order and (precision != "bf16" or heads or len(seg_widths) != 1 or seg_widths[0] != 128 or any(narrow or ())
                              or any(tuple(W.shape) != (128, 128) for W in weights)):
            raise NotImplementedError("rs_order: rounded-bf16 mode, one 128-wide input block, 128 x 128 layers, no heads")
        # `rs2` (4 / 5 = G4C_WFMT_BF16_RS2 / _RS2N): the stream of the row-split UPDATE kernel (mlp_rs2_kernel): two 128-wide input
        # blocks, two layers, optional heads — the columns of every 128-wide block of every layer and head in the order `_rs_k_order`
        self.rs2 = int(rs2)
        if self.rs2 and (self.rs2 not in (4, 5) or precision != "bf16" or self.rs_order or tuple(seg_widths) != (128, 128) or any(narrow or ())
                         or len(weights) != 2 or tuple(weights[0].shape) != (128, 256) or tuple(weights[1].shape) != (128, 128)
                         or len(heads) not in (0, 2) or any(tuple(h.shape) != (128, 128) for h in heads) or any(seg_negate)):
            raise NotImplementedError("rs2: rounded-bf16 mode, [128 | 128] -> 128 -> 128, no or two 128 x 128 heads")
        if precision == "bf16":      # rounded bf16: the plain stream, or one in the row-split kernels' order
            self.desc.w_format = _lib.WFMT_BF16_RS if self.rs_order else (self.rs2 or _lib.WFMT_BF16)
        else:
            self.desc.w_format = {"f16x2": _lib.WFMT_F16X2, "bf16x3": _lib.WFMT_BF16X3, None: _lib.WFMT_FP32}[self.split]
        # `rs_blocks[j]` (rounded-bf16 mode): input block j arrives as RsOrderedRows — bf16 rows in the row-split kernel's column order
        # (its aggregate, G4C_AGG_OUT_BF16) — and is read by a kernel that knows nothing of that order: the COLUMNS of the first layer's
        # block j are packed in the same order instead, the product is the same sum in another order.
        self.rs_blocks = tuple(bool(x) for x in rs_blocks) if rs_blocks is not None else (False,) * len(seg_widths)
        if any(self.rs_blocks) and (self.rs_order or precision != "bf16" or any(narrow) or len(self.rs_blocks) != len(seg_widths)
                                    or any(r and w != 128 for r, w in zip(self.rs_blocks, seg_widths))):
            raise NotImplementedError("rs_blocks: rounded-bf16 mode, 128-wide blocks, no narrow blocks")
        # (`site`: the name a clipped value is reported under — f16_range_report; the device's default flag buffer exists from here on)
        self.site = site or "an MLP created outside a model"
        if self.split == "f16x2":
            _range_buffer(dev)
            self.desc.range_slot = _range_slot(self.site)
        self._keep: List[Tensor] = []
        stream = _lib.stream_handle(dev)
        KC, NP = 32, 128                       # kernel constants: K chunk, computed layer width

        def k_order(l: Optional[int], k_in: int) -> Optional[Tensor]:
            """Column index by which layer `l` (None: a head) is packed, or None for its columns as they are: `_rs_k_order` inside every
            128-wide block of a row-split stream, and inside the first layer's `rs_blocks` of any other."""
            if self.rs_order or self.rs2:
                widths = [128] * (k_in // 128)
                marked = [True] * len(widths)
            elif l == 0 and any(self.rs_blocks):
                widths, marked = seg_widths, self.rs_blocks
            else:
                return None
            cols, c0 = torch.arange(k_in, device=dev), 0
            for w, r in zip(widths, marked):
                if r:
                    cols[c0:c0 + 128] = c0 + _rs_k_order(dev)
                c0 += w
            return cols

        def pack(W: Tensor, l: Optional[int], n_out: int, k_in: int, segs, negs, wptr: int, k_pad: int) -> None:
            Wc, cols = W.detach().to(torch.float32).contiguous(), k_order(l, k_in)
            if cols is not None:
                Wc = Wc[:, cols].contiguous()
            seg_arr, neg_arr = (C.c_int32 * len(segs))(*segs), (C.c_int32 * len(segs))(*negs)
            _lib.check(lib.g4c_mlp_pack_layer(_lib.ptr(Wc), n_out, k_in, seg_arr, neg_arr, len(segs), self.desc.w_format, wptr, k_pad, NP, stream))
        if bf16 and any(s > NP for s in seg_widths):
            raise NotImplementedError("bf16 MLP with an input block wider than 128")
        wide = [j for j in range(len(seg_widths)) if not narrow[j]]            # the blocks that go through the packed stream
        k_pad0 = NP * len(wide) if bf16 else sum((s + KC - 1) // KC * KC for s in seg_widths)
        k_pads = [k_pad0] + [NP] * (n_layers - 1)
        # one contiguous weight stream (layer after layer, 32-k chunk after chunk) + one chunk of slack:
        # the kernel's register ring prefetches one chunk past the end
        if len(heads) > _lib.MAX_HEADS or any(tuple(h.shape) != (NP, NP) for h in heads):
            raise NotImplementedError(f"heads must be at most {_lib.MAX_HEADS} weights of shape [128, 128]")
        if heads and int(weights[-1].size(0)) != NP:
            raise NotImplementedError("heads need a 128-wide MLP output")
        # (bf16: 2-byte elements, one 128-k block of slack)
        stream_buf = torch.zeros((sum(k_pads) + NP * len(heads) + (NP if bf16 else KC)) * NP * planes,
                                 dtype=torch.bfloat16 if bf16 else torch.float32, device=dev)
        esz = 2 * planes if bf16 else 4
        bias_buf = torch.zeros(n_layers * NP, dtype=torch.float32, device=dev)
        self._keep += [stream_buf, bias_buf]
        off = 0
        for l, (W, b) in enumerate(zip(weights, biases)):
            n_out, k_in = int(W.size(0)), int(W.size(1))
            if n_out > NP:
                raise NotImplementedError(f"layer width {n_out} > 128 is outside the fused-MLP kernel envelope")
            if l == 0:
                segs, negs = list(seg_widths), [1 if x else 0 for x in seg_negate]
                self.narrow_w = {}
                if any(narrow):          # fp32 rows of W1^T for the narrow blocks; the stream gets the remaining columns only
                    col0s = [sum(seg_widths[:j]) for j in range(len(seg_widths))]
                    W32 = W.detach().to(torch.float32)
                    for j in range(len(seg_widths)):
                        if narrow[j]:
                            rows = torch.zeros((seg_widths[j], NP), dtype=torch.float32, device=dev)
                            rows[:, :n_out] = W32[:, col0s[j]:col0s[j] + seg_widths[j]].T * (-1.0 if seg_negate[j] else 1.0)
                            self.narrow_w[j] = rows.contiguous()
                            self._keep.append(self.narrow_w[j])
                    if wide:
                        W = torch.cat([W32[:, col0s[j]:col0s[j] + seg_widths[j]] for j in wide], dim=1)
                        segs, negs = [seg_widths[j] for j in wide], [1 if seg_negate[j] else 0 for j in wide]
                        k_in = int(W.size(1))
                    else:
                        W = None
            else:
                prev = int(weights[l - 1].size(0))
                if k_in != prev:
                    raise ValueError(f"layer {l + 1} expects {k_in} inputs, previous layer gives {prev}")
                segs, negs = [k_in], [0]
            wptr = stream_buf.data_ptr() + esz * off
            if W is not None:            # (None: every input block of the first layer is narrow, nothing to stream)
                pack(W, l, n_out, k_in, segs, negs, wptr, k_pads[l])
            if b is not None:
                bias_buf[l * NP: l * NP + n_out].copy_(b.detach())
            self.desc.k_pad[l], self.desc.n_pad[l] = k_pads[l], NP
            self.desc.w[l], self.desc.b[l] = wptr, bias_buf.data_ptr() + 4 * l * NP
            off += k_pads[l] * NP
        self.n_heads = len(heads)
        for W in heads:
            pack(W, None, NP, NP, [NP], [0], stream_buf.data_ptr() + esz * off, NP)
            off += NP * NP
        self.n_out = int(weights[-1].size(0))
        self.desc.n_out = self.n_out
        # nn.Linear MACs x 2 (+ the heads' products)
        self.flops_per_row = float(sum(2 * int(W.size(0)) * int(W.size(1)) for W in list(weights) + list(heads)))
        if ln is not None:
            g, be, eps = ln
            g, be = g.detach().to(torch.float32).contiguous(), be.detach().to(torch.float32).contiguous()
            self.desc.ln_gamma, self.desc.ln_beta, self.desc.ln_eps = g.data_ptr(), be.data_ptr(), float(eps)
            self._keep += [g, be]
        else:
            self.desc.ln_gamma, self.desc.ln_beta, self.desc.ln_eps = None, None, 0.0
        self.seg_widths = tuple(seg_widths)
        self.device = dev
        # (the range proof's half of the image: rebuilt with it, under the same cache key — MLP._image)
        self.norms = weight_norms(weights, biases, ln, heads, seg_widths, narrow) if self.split == "f16x2" else None
        if self.norms is not None:
            check_weight_range(self.norms, self.site)
        # the parameter tensors this image was packed from (the training path differentiates with respect to them: autograd.py)
        self.params = (list(weights), list(biases), ln)
        self.heads_params = bool(heads)


def _src_array(sources: Sequence[Source]):
    arr = (_lib.g4c_src_t * len(sources))()
    for a, s in zip(arr, sources):
        a.ptr, a.idx, a.width, a.ld, a.col0, a.pre_act = (s.tensor.data_ptr(), _lib.ptr(s.index), s.width, _ld(s.tensor),
                                                          s.col0, s.pre_act)
        a.additive = 1 if s.additive else 0
        a.dtype = 1 if s.tensor.dtype == torch.bfloat16 else 0
        if s.segments is not None:
            a.seg_off, a.seg_mean, a.seg_perm = _lib.ptr(s.segments.off), 1 if s.seg_mean else 0, _lib.ptr(s.segments.perm)
    return arr


def agg_bound(bound: Optional[float], csr: CsrPlan, mean: bool) -> Optional[float]:
    """Bound on an aggregate of rows bounded by `bound`: a mean keeps it, a sum multiplies it by the plan's longest segment."""
    return bound if (bound is None or mean) else bound * max(csr.max_deg, 1)


def _certify(packed: "PackedMLP", sources: Sequence[Source], act: int, residual: bool, tracked: bool) -> LaunchBounds:
    """The range proof of the launch that is about to be issued; sets the certificate of its descriptor (g4c_mlp_t.range_certified)
    for this launch.  `tracked`: the launch keeps its tracker whatever the proof says (save / mul: the training forms)."""
    seg_len = max((s_.segments.max_deg for s_ in sources if s_.segments is not None), default=None)
    lb = range_bounds(packed.norms, sources, act, residual, seg_len)
    packed.desc.range_certified = 1 if (RANGE_PROOFS and not tracked and certifies(lb.converted)) else 0
    return lb


def _agg_mode(agg_mean: bool, csr: CsrPlan) -> int:
    """`agg_mode` of a fused-aggregation launch: bit 0 = mean, G4C_AGG_UNIFORM(k) when every segment has k rows."""
    return (1 if agg_mean else 0) | (csr.uniform_deg << 8)


# Dense pairs for segments of any length (csrc/mlp_ws.hip, mlp_ws_any_kernel): an f16x3 launch with the fused aggregation whose segments
# are not the uniform 4 .. 8 rows of the level-1 form also hands the library one row range per persistent workgroup (CsrPlan.row_ranges);
# the library uses them where it has the form (the plain hoisted message launch, the fused MP layer) and ignores them elsewhere.
# G4C_DENSE_ANY=0: the tiles of whole segments, as before (A/B runs) — the same results bit for bit either way.
DENSE_ANY = os.environ.get("G4C_DENSE_ANY", "1") != "0"


@contextlib.contextmanager
def dense_any(on: bool):
    """DENSE_ANY and `on` for the launches issued inside (the partitioned forwards: a rank's sub-mesh keeps its launches)."""
    global DENSE_ANY
    was, DENSE_ANY = DENSE_ANY, DENSE_ANY and on
    try:
        yield
    finally:
        DENSE_ANY = was


def ws_grid(t: Tensor) -> int:
    """Persistent workgroups of a weight-stationary launch on `t`'s device (g4c_mlp_ws_grid: one per compute unit, at most
    G4C_WS_MAX_GRID)."""
    n = C.c_int32(0)
    _lib.check(_lib.load().g4c_mlp_ws_grid(t.data_ptr(), C.byref(n)))
    return int(n.value)


def _ranges_only(packed: "PackedMLP", sources: Sequence["Source"], csr: CsrPlan, agg_out: Tensor) -> bool:
    """A plain message launch whose segments are longer than a tile (no CsrPlan.tiles()) can still reduce its own rows — on the row
    ranges alone, in the one form that needs no tiles: the f16x3 stream, one direct 128-wide block and two additive 128-wide fp32
    blocks, two or three layers (ws_any_takes, csrc/mlp_ws.hip)."""
    if not (DENSE_ANY and packed.split == "f16x2" and packed.desc.n_layers in (2, 3) and packed.seg_widths == (128,) and len(sources) == 3):
        return False
    x, adds = sources[0], sources[1:]
    if x.additive or x.index is not None or x.segments is not None or x.tensor.dtype != torch.float32 or x.col0 % 4 or _ld(x.tensor) % 4 or x.tensor.data_ptr() % 16:
        return False
    if any(not s.additive or s.width != 128 or s.tensor.dtype != torch.float32 or s.col0 % 4 or _ld(s.tensor) % 4 or s.tensor.data_ptr() % 16 for s in adds):
        return False
    return csr.perm is None and agg_out.dtype == torch.float32 and csr.row_ranges(ws_grid(agg_out)) is not None


def _set_agg(io, csr: CsrPlan, agg_out: Tensor, agg_mean: bool, ranges: bool = False) -> None:
    tiles = csr.tiles()
    if tiles is not None:
        io.tile_rows, io.tile_seg, io.n_tiles = _lib.ptr(tiles[0]), _lib.ptr(tiles[1]), tiles[2]
    elif not (ranges and DENSE_ANY and csr.row_ranges(ws_grid(agg_out)) is not None):
        raise ValueError("fused aggregation: the rows must be in segment order with segments of at most 32 rows")
    io.seg_off = _lib.ptr(csr.off)
    io.agg, io.agg_ld, io.agg_mode = _lib.ptr(agg_out), _ld(agg_out), _agg_mode(agg_mean, csr)
    if ranges and DENSE_ANY and not 4 <= csr.uniform_deg <= 8:
        plan = csr.row_ranges(ws_grid(agg_out))
        if plan is not None:
            io.wg_rows, io.wg_seg, io.n_wg, io.wg_pairs, io.wg_max_seg = _lib.ptr(plan[0]), _lib.ptr(plan[1]), int(plan[0].numel()) - 1, plan[2], plan[3]


def _set_heads(io, head_outs: Sequence[Tensor]) -> None:
    io.n_heads, io.head_ld = len(head_outs), _ld(head_outs[0])
    io.head_dtype = 1 if head_outs[0].dtype == torch.bfloat16 else 0
    for j, h in enumerate(head_outs):
        io.head_out[j] = h.data_ptr()


def _run(packed: PackedMLP, arr, n_src: int, n_rows: int, io, dev, flops: float, nbytes: float) -> None:
    """The one launch (g4c_mlp_run), timed when a KernelTimer is active.  An f16x3 launch reports clips into the flag buffer of
    whoever issued it (_launch_flags)."""
    if packed.split == "f16x2":
        io.range_flag = _launch_flags(dev).data_ptr()
    kind = "mlp_split_kernel<4>" if packed.precision == "fp32" else "mlp_bx6_kernel"      # (the timer relabels it by what ran)
    _timed(kind, flops, nbytes, lambda: _lib.check(_lib.load().g4c_mlp_run(C.byref(packed.desc), arr, n_src, n_rows, C.byref(io),
                                                                           _lib.stream_handle(dev))))


def mp_layer_forward(msg: PackedMLP, sources: Sequence[Source], n_rows: int, csr: CsrPlan, agg_mean: bool, upd: PackedMLP,
                     v: Tensor, act: int, store_rows: bool = True, head_outs: Optional[Sequence[Tensor]] = None,
                     v_out: Optional[Tensor] = None, v_bound: Optional[float] = None, e_out: Optional[Tensor] = None,
                     agg_out: Optional[Tensor] = None) -> Tuple[Optional[Tensor], Tensor, Optional[Sequence[Tensor]]]:
    """One launch for a whole MP layer (g4c_mlp_io_t.upd; reference nn/blocks.py:175-186): the hoisted message MLP `msg`
    on `sources` (one 128-wide weighted block + the two gathered node-side products as additive sources) with the aggregation over
    `csr`, and — in the same persistent workgroups — the node MLP `upd` on [aggregate | v] with LayerNorm / `act` and, when
    `head_outs` is given, the heads packed behind `upd` (the next layer's products).  f16x3 arithmetic only, inference only.
    `v_bound`: proven bound on |v| (Source.bound), for the node MLP's half of the range proof.
    `e_out` (float32 [>= n_rows, 128], only with store_rows) / `agg_out` (float32 [>= n_seg, 128]): the caller's tensors for the e' rows
    and for the aggregate the launch writes and re-reads (views of wider buffers are fine); None allocates them here.
    Returns (e' rows or None, v', head_outs); take_bounds() then answers for v' (`out`), the heads and e' (`e`)."""
    global _last_bounds
    _last_bounds = None
    if e_out is not None:
        if not store_rows:
            raise ValueError("e_out: given with store_rows=False (the launch stores no e' rows)")
        _rows_f32(e_out, "e_out", cols=128, min_rows=n_rows)
    if agg_out is not None:
        _rows_f32(agg_out, "agg_out", cols=128, min_rows=csr.n_seg)
    dev = _lib.require_hip(*[s.tensor for s in sources], *[s.index for s in sources], v, v_out, e_out, agg_out)
    if msg.split != "f16x2" or upd.split != "f16x2":
        raise NotImplementedError("mp_layer_forward needs both MLPs packed for the f16x3 arithmetic")
    if csr.tiles() is None or n_rows != csr.n:
        raise ValueError("mp_layer_forward: the rows must be in segment order with segments of at most 32 rows")
    v = _f32_2d(v, "v")
    n_t = csr.n_seg
    if e_out is None and store_rows:
        e_out = torch.empty((n_rows, 128), dtype=torch.float32, device=dev)
    # (scratch: written and re-read by the same workgroup, L2-resident)
    agg = agg_out if agg_out is not None else torch.empty((n_t, 128), dtype=torch.float32, device=dev)
    if v_out is None:
        v_out = torch.empty((n_t, 128), dtype=torch.float32, device=dev)
    n_heads = 0 if head_outs is None else len(head_outs)
    if n_heads and (n_heads != upd.n_heads):
        raise ValueError(f"{n_heads} head outputs for a packing with {upd.n_heads} heads")
    io = _lib.g4c_mlp_io_t(row_count=n_rows, out=_lib.ptr(e_out), out_ld=128 if e_out is None else _ld(e_out), upd=C.pointer(upd.desc),
                           v=_lib.ptr(v), v_ld=_ld(v), v_act=act, v_out=_lib.ptr(v_out), v_out_ld=_ld(v_out))
    _set_agg(io, csr, agg, agg_mean, ranges=True)
    if n_heads:
        _set_heads(io, head_outs)
    in_b = 4.0 * 128 * (n_rows * (2 if store_rows else 1) + n_t * (2 + n_heads))
    # the range proof of both halves: the node MLP reads [aggregate of e' | v], and `v_bound` is what the caller knows about v.  The
    # library drops the trackers only when BOTH descriptors are certified.
    lb_msg = _certify(msg, sources, _lib.ACT_NONE, False, False)
    lb_upd = _certify(upd, [Source(agg, bound=agg_bound(lb_msg.out, csr, agg_mean)), Source(v, bound=v_bound)], act, False, False)
    try:
        _run(msg, _src_array(sources), len(sources), n_rows, io, dev, msg.flops_per_row * n_rows + upd.flops_per_row * n_t, in_b)
    finally:
        msg.desc.range_certified = upd.desc.range_certified = 0          # (the certificates were for this launch: the descriptors are shared)
    _last_bounds = LaunchBounds(None, lb_upd.out, lb_upd.heads, e=lb_msg.out)
    return e_out, v_out, head_outs


# The first MP layer of a MuS model multiplies the same edge latents e0 (StaticCache) by the same W1e in every step of a rollout: with
# this on, a `Rollout` computes T = b1 + W1e e0 once and the layer's message launch starts from it (mlp_forward_precomputed).
# G4C_STATIC_FIRST_LAYER=0: today's launch, bit for bit (A/B runs).
STATIC_FIRST_LAYER = os.environ.get("G4C_STATIC_FIRST_LAYER", "1") != "0"


def mlp_forward_precomputed(packed: PackedMLP, first: Tensor, products: Sequence[Source], n_rows: int,
                            agg: Tuple[CsrPlan, Tensor, bool], act: int = _lib.ACT_NONE, store_rows: bool = True,
                            out: Optional[Tensor] = None) -> Optional[Tensor]:
    """The hoisted message launch of `packed` (one 128-wide weighted block, three 128-wide layers, f16x3) WITHOUT its first layer
    (g4c_mlp_t.k_pad[0] == 0): `first` [n_rows, 128] = b1 + W1x x, computed before, and the two gathered node-side `products`
    (additive Sources with an index) sum to the layer-0 pre-activation, (first + p0[i0]) + p1[i1]; the launch runs the two layers
    left, LayerNorm, `act`, the row stores (`store_rows`) and the fused aggregation `agg` = (csr, out [n_seg, 128], mean), bit-identical
    to segment_reduce of the rows.  `out` (float32 [>= n_rows, 128], only with store_rows): the caller's tensor for the rows (a view of
    a wider buffer is fine); None allocates it here.  Inference only; always range-tracked; a shape the library has not built raises
    NotImplementedError.  take_bounds() then answers for the output rows."""
    global _last_bounds
    _last_bounds = None
    csr, agg_out, agg_mean = agg
    if out is not None:
        if not store_rows:
            raise ValueError("out: given with store_rows=False (the launch stores no rows)")
        _rows_f32(out, "out", cols=128, min_rows=n_rows)
    dev = _lib.require_hip(first, agg_out, out, *[s.tensor for s in products], *[s.index for s in products])
    if dev != packed.device:
        raise RuntimeError(f"MLP weights on {packed.device}, inputs on {dev}")
    if packed.split != "f16x2" or packed.desc.n_layers != 3 or packed.seg_widths != (128,) or packed.n_out != 128 or packed.n_heads:
        raise NotImplementedError("mlp_forward_precomputed: a three-layer 128-wide MLP over one 128-wide block, packed for f16x3, no heads")
    if len(products) != 2 or not all(s.whole_block(128, dtypes=(torch.float32,), product=True) for s in products):
        raise ValueError("mlp_forward_precomputed: two additive 128-wide fp32 sources gathered through an index")
    first = _rows_f32(first, "first", cols=128, min_rows=n_rows)
    if csr.tiles() is None or n_rows != csr.n:
        raise ValueError("mlp_forward_precomputed: the rows must be in segment order with segments of at most 32 rows")
    if agg_out.dtype != torch.float32:
        raise TypeError(f"aggregate: expected float32, got {agg_out.dtype}")
    if out is None and store_rows:
        out = torch.empty((n_rows, 128), dtype=torch.float32, device=dev)
    # the launch's descriptor: the image's own with layer 0 taken out of the stream (the bias block keeps layer 0's unused slot)
    desc = _lib.g4c_mlp_t()
    C.memmove(C.byref(desc), C.byref(packed.desc), C.sizeof(desc))
    desc.k_pad[0], desc.w[0], desc.range_certified = 0, packed.desc.w[1], 0
    srcs = [Source(first, additive=True)] + list(products)
    io = _lib.g4c_mlp_io_t(act=act, row_count=n_rows, out=_lib.ptr(out), out_ld=128 if out is None else _ld(out))
    _set_agg(io, csr, agg_out, agg_mean)
    io.range_flag = _launch_flags(dev).data_ptr()
    flops = float(2 * 2 * 128 * 128) * n_rows
    nbytes = 4.0 * 128 * (n_rows * (2 if store_rows else 1) + csr.n_seg)
    arr = _src_array(srcs)
    _timed("mlp_bx6_kernel", flops, nbytes, lambda: _lib.check(_lib.load().g4c_mlp_run(C.byref(desc), arr, 3, n_rows, C.byref(io),
                                                                                       _lib.stream_handle(dev))))
    # (behind a LayerNorm the rows are bounded whatever went in: the bound the unhoisted launch's proof gives them)
    ln = packed.norms["ln"] if packed.norms is not None else None
    _last_bounds = LaunchBounds(None, act_bound((packed.norms["n_out"] - 1) ** 0.5 * ln[0] + ln[1], act) if ln is not None else None)
    return out


def _rows_dtype(what: str, tensors: Sequence[Tensor]) -> int:
    """G4C_DTYPE_* of the `save` / `mul` rows of one launch: all fp32 or all bf16."""
    kinds = {t.dtype for t in tensors}
    if not kinds <= {torch.float32, torch.bfloat16} or len(kinds) > 1:
        raise TypeError(f"{what} tensors must share one dtype, float32 or bfloat16 (got {sorted(str(k) for k in kinds)})")
    return _lib.DTYPE_BF16 if kinds == {torch.bfloat16} else _lib.DTYPE_F32


def mlp_forward(packed: PackedMLP, sources: Sequence[Source], n_rows: int, act: int = _lib.ACT_NONE,
                out: Optional[Tensor] = None, out_idx32: Optional[Tensor] = None,
                resid: Optional[Tensor] = None, resid_col0: int = 0, rows: Optional[Tuple[int, int]] = None,
                head_outs: Optional[Sequence[Tensor]] = None, agg: Optional[Tuple[CsrPlan, Tensor, bool]] = None,
                save: Optional[Sequence[Optional[Tensor]]] = None, mul: Optional[Sequence[Optional[Tensor]]] = None,
                store_rows: bool = True, rows_dtype: Optional[torch.dtype] = None, rows_act: int = _lib.ACT_NONE) -> Optional[Tensor]:
    """One fused MLP launch (g4c_mlp_run).  `rows` = (begin, count) (tests / tuning): only those rows, begin a multiple of 32 —
    one MLP split over several launches.
    `head_outs` ([n_rows, 128] tensors, one per head of `packed`; all fp32, or all bf16 in the rounded-bf16 mode): the heads.
    `agg` = (csr, out [n_seg, 128], mean): also aggregate the output rows over the segments of `csr` (rows must be in segment
    order) — inside the launch when the kernel can, otherwise with a g4c_segment_reduce afterwards.
    `save` (training forward; bf16x6 / f16x3 and the plain rounded-bf16 stream, not its row-split orders): one [n_rows, 128] fp32 tensor (or None) per layer, receiving that layer's output
    rows; `mul` (with `save`): per hidden layer the SELU-output rows whose slope multiplies that layer's result instead of bias + SELU
    (the backward chain of a block, see include/g4c.h).  On the plain rounded-bf16 stream the `save` tensors, and the `mul` tensors,
    may be bf16 (one dtype per list, TypeError otherwise): kept rows stored rounded once to bf16, `mul` rows widened exactly.
    A bf16 `out` (rounded-bf16 mode): the rows are stored as bf16.
    `rows_dtype=torch.bfloat16` (rounded-bf16 mode, with an aggregation the launch fuses; ignored otherwise): the output rows are
    stored as bf16 — their consumer rounds them to bf16 on load anyway, and the launch is HBM-bound on them; the aggregate stays fp32.
    `rows_act=ACT_SELU` (only together with bf16 rows): the stored rows are bf16(SELU(row)) — the activation their reader would apply
    on load, applied before the one rounding (G4C_DTYPE_BF16_SELU); the aggregate is taken from the un-activated fp32 rows.  Check
    `out.dtype == torch.bfloat16` on the result to know whether the rows came back compact and activated.
    With gradients enabled and a differentiable input / parameter, the call is recorded for autograd (autograd.py)."""
    global _last_bounds
    _last_bounds = None
    if torch.is_grad_enabled():
        from . import autograd as _ag
        if _ag.wants_grad(packed, sources, resid):
            if out is not None or out_idx32 is not None or head_outs is not None or agg is not None or rows is not None or save is not None:
                raise NotImplementedError("out= / heads / fused aggregation are inference-only forms of mlp_forward; "
                                          "call under torch.no_grad() or use the plain form")
            return _ag.mlp(packed, sources, n_rows, act, resid, resid_col0)
    if packed.rs2:
        ok = [isinstance(s.tensor, RsOrderedRows) for s in sources]
        if len(sources) != 2 or not ok[0] or ok[1] != (packed.rs2 == 4) or any(s.tensor.dtype != torch.bfloat16 for s in sources):
            raise ValueError("weights packed for the row-split update kernel: [aggregate | e] as bf16 rows, the aggregate (and, format 4, e) RsOrderedRows")
    elif packed.rs_order and packed.precision == "bf16":
        # (the row-split kernel's rounded-bf16 stream: its bf16 rows are in ITS column order, nobody else's)
        if any(s.tensor.dtype == torch.bfloat16 and not isinstance(s.tensor, RsOrderedRows) for s in sources):
            raise ValueError("weights packed for the row-split kernel: bf16 rows must be RsOrderedRows (its column order)")
    elif any(isinstance(s.tensor, RsOrderedRows) for s in sources) or any(packed.rs_blocks):
        # tagged rows reach a kernel that reads feature order: fine where the pack has that block's columns in the same order
        # (`rs_blocks`), restored to feature order (a copy) anywhere else
        fixed, j = [], 0
        for s in sources:
            tagged = isinstance(s.tensor, RsOrderedRows)
            ok = (not s.additive) and j < len(packed.rs_blocks) and packed.rs_blocks[j] and s.col0 == 0 and s.width == 128
            if not s.additive:
                if j < len(packed.rs_blocks) and packed.rs_blocks[j] and not tagged:
                    raise ValueError(f"input block {j}: the weights expect rows in the row-split order (ops.RsOrderedRows)")
                j += 1
            fixed.append(s if (not tagged or ok) else
                         Source(rs_rows_to_natural(s.tensor), s.index, s.col0, s.width, s.negate, s.pre_act, s.additive, s.segments, s.seg_mean))
        sources = fixed
    dev = _lib.require_hip(*[s.tensor for s in sources], *[s.index for s in sources], out, out_idx32, resid)
    if dev != packed.device:
        raise RuntimeError(f"MLP weights on {packed.device}, inputs on {dev}")
    if tuple(s.width for s in sources if not s.additive) != packed.seg_widths:
        raise ValueError(f"input blocks {[s.width for s in sources if not s.additive]} do not match packed layout {packed.seg_widths}")
    arr = _src_array(sources)
    if any(packed.narrow):
        j = 0
        for a, src in zip(arr, sources):
            if src.additive:
                continue
            if packed.narrow[j]:
                if src.index is not None or src.pre_act != _lib.ACT_NONE:
                    raise ValueError("a narrow input block cannot be gathered through an index or activated on load")
                a.additive, a.w = 2, packed.narrow_w[j].data_ptr()
            j += 1
    # store_rows=False (with a fused aggregation only): the output rows are not written, only their aggregate
    fusable = (agg is not None and FUSE_AGG and packed.precision in ("bf16x6", "bf16") and packed.n_out == 128 and head_outs is None
               and rows is None and out_idx32 is None and resid is None and n_rows == agg[0].n
               and (agg[0].tiles() is not None or _ranges_only(packed, sources, agg[0], agg[1])))
    if not store_rows and not fusable:
        raise ValueError("store_rows=False needs an aggregation the launch can fuse (ops.can_fuse_aggregation)")
    reduce_after = None
    if agg is not None and not fusable:          # the plain launch, then the separate reduction
        reduce_after, agg = agg, None
    rows16 = bool(fusable and store_rows and rows_dtype == torch.bfloat16 and packed.precision == "bf16" and out is None)
    if out is None and store_rows:
        out = torch.empty((n_rows, packed.n_out), dtype=torch.bfloat16 if rows16 else torch.float32, device=dev)
    if out is not None and out.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"out: expected float32 or bfloat16, got {out.dtype}")
    row_begin, row_count = rows if rows is not None else (0, n_rows)
    io = _lib.g4c_mlp_io_t(act=act, row_begin=row_begin, row_count=row_count, out=_lib.ptr(out),
                           out_ld=_ld(out) if out is not None else 128, out_idx=_lib.ptr(out_idx32), resid=_lib.ptr(resid),
                           resid_ld=_ld(resid) if resid is not None else 0, resid_col0=resid_col0)
    if out is not None and out.dtype == torch.bfloat16:
        if agg is None and (packed.precision != "bf16" or out_idx32 is not None or resid is not None):
            raise TypeError("a bf16 `out` needs the rounded-bf16 mode and no output index / residual")
        if rows16 and rows_act not in (_lib.ACT_NONE, _lib.ACT_SELU):
            raise ValueError("rows_act: only ACT_SELU")
        io.out_dtype = 2 if (rows16 and rows_act == _lib.ACT_SELU) else 1
    # algorithmic bytes per row: the weighted input blocks (bf16 rows count 2 bytes per value) and the output row
    in_bytes = float(sum(s.width * (2 if s.tensor.dtype == torch.bfloat16 else 4) for s in sources if not s.additive))
    nbytes = (in_bytes + 4.0 * packed.n_out) * row_count
    if head_outs is not None:
        if len(head_outs) != packed.n_heads or packed.n_heads == 0:
            raise ValueError(f"{len(head_outs)} head outputs for a packing with {packed.n_heads} heads")
        if out_idx32 is not None or resid is not None:
            raise NotImplementedError("heads with an output index / residual")
        _lib.require_hip(*head_outs)
        if any(h.dtype == torch.bfloat16 for h in head_outs):
            # rounded-bf16 mode: the head rows (the next message MLP's first-layer products) stored as bf16
            if packed.precision != "bf16" or any(h.dtype != torch.bfloat16 for h in head_outs):
                raise TypeError("bf16 head outputs need the rounded-bf16 mode, and every head in bf16")
        elif out.dtype != torch.float32:
            raise TypeError("heads stored as fp32 need fp32 output rows (bf16 rows: bf16 heads)")
        _set_heads(io, head_outs)
        if packed.precision == "fp32":
            nbytes = 4.0 * (sum(packed.seg_widths) + packed.n_out * (1 + packed.n_heads)) * n_rows
    if agg is not None:
        csr, agg_out, agg_mean = agg
        _lib.require_hip(agg_out)
        if agg_out.dtype not in (torch.float32, torch.bfloat16):
            raise TypeError(f"aggregate: expected float32 (or bfloat16 on the row-split kernel), got {agg_out.dtype}")
        _set_agg(io, csr, agg_out, agg_mean, ranges=packed.split == "f16x2" and save is None)
        if agg_out.dtype == torch.bfloat16:          # (G4C_AGG_OUT_BF16: bf16 aggregate rows in the row-split kernel's column order)
            io.agg_mode |= 1 << 16
        out_b = 0 if not store_rows else packed.n_out * (2 if out.dtype == torch.bfloat16 else 4)
        nbytes = (in_bytes + out_b) * n_rows + 4.0 * packed.n_out * csr.n_seg
    if save is not None:
        live = [t for t in save if t is not None]
        _lib.require_hip(*live)
        if any(t.dim() != 2 or t.size(0) < n_rows or t.size(1) < 128 or t.stride(1) != 1 or _ld(t) != _ld(live[0]) for t in live):
            raise ValueError("save tensors must be [n_rows, >= 128] fp32 (or bf16) with one common leading dimension")
        if len(save) > _lib.MAX_LAYERS:
            raise ValueError(f"{len(save)} save tensors for {packed.desc.n_layers} layers")
        io.n_save, io.save_ld = len(save), _ld(live[0]) if live else 128
        io.save[:len(save)] = [_lib.ptr(t) for t in save]
        io.save_dtype = _rows_dtype("save", live)
        if mul is not None:
            lm = [t for t in mul if t is not None]
            _lib.require_hip(*lm)
            if len(mul) != len(save) or any(t.size(0) < n_rows or t.size(1) < 128 or t.stride(1) != 1 or _ld(t) != _ld(lm[0]) for t in lm):
                raise ValueError("mul tensors must be [n_rows, >= 128] fp32 (or bf16) with one common leading dimension, one entry per layer")
            io.mul[:len(mul)] = [_lib.ptr(t) for t in mul]
            io.mul_ld = _ld(lm[0]) if lm else 128
            io.mul_dtype = _rows_dtype("mul", lm)
        # (bf16 save / mul rows count 2 bytes per value; the fp32 form's count is what it was)
        nbytes = (4.0 * (sum(packed.seg_widths) + packed.n_out) + 128.0 * sum(t.element_size() for t in live)) * n_rows
    # (a residual adds data to the rows; an output index or a row sub-range writes only some rows of `out`: no bound for the tensor)
    lb = _certify(packed, sources, act, resid is not None or out_idx32 is not None or rows is not None, save is not None)
    try:
        _run(packed, arr, len(sources), n_rows, io, dev, packed.flops_per_row * row_count, nbytes)
    finally:
        packed.desc.range_certified = 0          # (the certificate was for this launch: the descriptor is shared)
    _last_bounds = lb
    if reduce_after is not None:
        segment_reduce(out, reduce_after[0], reduce_after[2], out=reduce_after[1])
    return out
