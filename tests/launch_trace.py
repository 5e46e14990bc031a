"""Test-only helper (no tests in it): the host-visible facts of every MLP launch and segment reduction a piece of code issues, and the
cases `tests/test_gpu_launch_trace.py` and `scripts/mp_host_path.py` run under it.

`LaunchTrace()` is a context manager that swaps `graphs4cfd_amd._lib._lib` — the handle `scripts/ab_test.py` swaps — for a proxy of the
loaded library.  The proxy passes every attribute through and records one row per call of `g4c_mlp_run` and of `g4c_segment_reduce`:
sizes, codes, dtypes and whether a pointer is set — never a pointer's value, never a device read.  Two facts that relate launches are
derived from pointers while recording and stored as booleans: whether an additive indexed source is the output of an earlier one-layer
launch without heads (a separate product launch), and whether a segment reduction reads the rows the MLP launch before it wrote.
The ranks of `tests/partition_harness.py` are threads of one interpreter, so rows are kept per thread name ("main", "rank0", ...).

A row is a flat list (the golden file stays small); `MLP_FIELDS` / `SRC_FIELDS` / `REDUCE_FIELDS` name its entries, `as_dict` makes a
row readable in a failure message."""
import contextlib
import os
import threading
from collections import defaultdict

import torch

import graphs4cfd_amd as gfd
from graphs4cfd_amd import _lib, ops, partition as P, partition_remus as PR, synthetic as S
from graphs4cfd_amd.nn import blocks as B
from graphs4cfd_amd.nn.rollout import Rollout

SRC_FIELDS = ("width", "col0", "pre_act", "additive", "dtype", "idx", "seg_off", "w", "from_product_launch")
MLP_FIELDS = ("n_rows", "n_src", "sources", "n_layers", "k_pad", "n_pad", "n_out", "w_format", "range_certified",
              "act", "out_dtype", "out", "out_idx", "resid", "agg", "upd", "n_heads", "head_dtype", "agg_mode", "n_tiles", "n_wg", "n_save",
              "save_dtype", "mul_dtype", "last_kernel", "last_shape", "last_tile_rows")
REDUCE_FIELDS = ("src_ld", "perm", "n_seg", "width", "mean", "src_act", "act", "out_ld", "behind_mlp")


def as_dict(row):
    """A recorded row with its field names ("mlp" / "reduce" first)."""
    if row[0] == "mlp":
        d = dict(zip(MLP_FIELDS, row[1:]))
        d["sources"] = [dict(zip(SRC_FIELDS, s)) for s in d["sources"]]
        return {"call": "mlp", **d}
    return {"call": "reduce", **dict(zip(REDUCE_FIELDS, row[1:]))}


class _Proxy:
    def __init__(self, lib):
        self._lib = lib
        self.rows = defaultdict(list)            # thread name -> rows
        self._made = defaultdict(dict)           # thread name -> {pointer an MLP launch wrote: it was a separate product launch}
        self._last_out = {}                      # thread name -> `out` of the thread's last MLP launch

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def g4c_mlp_run(self, desc, srcs, n_src, n_rows, io, stream):
        who = threading.current_thread().name
        who = "main" if threading.current_thread() is threading.main_thread() else who
        d, o, made = desc._obj, io._obj, self._made[who]
        sources = [[int(s.width), int(s.col0), int(s.pre_act), int(s.additive), int(s.dtype), bool(s.idx), bool(s.seg_off), bool(s.w),
                    bool(s.additive and s.idx and made.get(s.ptr, False))] for s in (srcs[j] for j in range(int(n_src)))]
        nl = int(d.n_layers)
        row = ["mlp", int(n_rows), int(n_src), sources, nl, list(d.k_pad[:nl]), list(d.n_pad[:nl]), int(d.n_out), int(d.w_format), int(d.range_certified),
               int(o.act), int(o.out_dtype), bool(o.out), bool(o.out_idx), bool(o.resid), bool(o.agg), bool(o.upd), int(o.n_heads), int(o.head_dtype),
               int(o.agg_mode), int(o.n_tiles), int(o.n_wg), int(o.n_save), int(o.save_dtype), int(o.mul_dtype)]
        product = nl == 1 and int(o.n_heads) == 0 and not bool(o.upd)
        for p in [o.out, o.agg, o.v_out] + [o.head_out[j] for j in range(int(o.n_heads))]:
            if p:
                made[p] = bool(product and p == o.out)
        self._last_out[who] = o.out
        code = self._lib.g4c_mlp_run(desc, srcs, n_src, n_rows, io, stream)
        row += [int(self._lib.g4c_mlp_last_kernel()), int(self._lib.g4c_mlp_last_shape()), int(self._lib.g4c_mlp_last_tile_rows())]
        self.rows[who].append(row)
        return code

    def g4c_segment_reduce(self, src, src_ld, perm, off, n_seg, width, mean, src_act, act, out, out_ld, stream):
        who = "main" if threading.current_thread() is threading.main_thread() else threading.current_thread().name
        behind = bool(src) and self._last_out.get(who) == src
        self._last_out[who] = None
        self._made[who].pop(out, None)
        self.rows[who].append(["reduce", int(src_ld), bool(perm), int(n_seg), int(width), int(mean), int(src_act), int(act), int(out_ld), behind])
        return self._lib.g4c_segment_reduce(src, src_ld, perm, off, n_seg, width, mean, src_act, act, out, out_ld, stream)


@contextlib.contextmanager
def LaunchTrace():
    """`with LaunchTrace() as rows:` — `rows` maps a thread's name to the rows it issued inside the block."""
    real = _lib.load()
    proxy = _Proxy(real)
    _lib._lib = proxy
    try:
        yield proxy.rows
    finally:
        _lib._lib = real


# ------------------------------------------------------------------------------------- the cases
# Each is one forward (or two eager rollout steps) on a synthetic mesh, hidden 128, at the smallest sizes on either side of the
# thresholds the host decisions read: HOIST_MIN_ROWS 24 576, RS1_MIN_ROWS 20 000, the weight-stationary threshold 20 000,
# FUSE_LAYER_MIN_ROWS 2 048.  `run(case)` returns {name: tensor}: what the bit comparison saves and compares.
DEV = torch.device("cuda", 0)
H = 128
MUS, MUGS = "NsTwoScaleGNN", "NsTwoGuillardScaleGNN"
PRECISIONS = ("f16x3", "bf16x6", "bf16", "fp32")
REMUS_K = 5
# the row-split UPDATE kernel takes edge launches of RS1_MIN_ROWS rows and more: 5 edges per node.  (At the size where the angle rows
# reach HOIST_MIN_ROWS a level has under 5 000 edges.)
REMUS_RS2_N = 4_000
# Two more thresholds decide routes: ops.FUSE_AGG_MIN_ROWS and ops.AGG_ON_LOAD_MIN_ROWS, both 50 000.  The static first layer
# needs a message launch that reduces its own rows (50 000 edges) in a layer that does not fuse (FUSE_LAYER_MAX_ROWS 120 000 edges): the
# rollout case runs on 20 000 nodes (120 000 edges).  A rank of
# two owns half the edges, and below HOIST_MIN_ROWS of them there are no products in the halo, no overlapped sub-launches and
# HipImpl.hoists is never true; its overlap branch aggregates on load from 50 000 rows on: the partitioned MuS case runs on 17 200
# nodes (51 600 edges per rank).
ROLLOUT_N = 20_000
PART_MUS_N = 17_200

_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def remus_sizes():
    """(n_hi, n_lo): the smallest node count whose level-1 angle rows reach HOIST_MIN_ROWS — counted on the graph — and a quarter of it."""
    def find():
        n = B.HOIST_MIN_ROWS // (REMUS_K * REMUS_K)
        while int(S.remus_graph(n, k=REMUS_K, seed=11).angle_index.size(1)) < B.HOIST_MIN_ROWS:
            n += 1
        return n, n // 4
    return _once("remus_sizes", find)


def _mus(n):
    return _once(("mus", n), lambda: S.mus_graph(n, levels=2, k=6, seed=n))


def _remus(n):
    return _once(("remus", n), lambda: S.remus_graph(n, k=REMUS_K, seed=11))


def _model(kind):
    def make():
        torch.manual_seed(28)
        if kind == "mus":
            return gfd.nn.NsTwoScaleGNN(arch=S.mus_arch(MUS, H), device=DEV)
        if kind == "mugs":
            return gfd.nn.NsTwoGuillardScaleGNN(arch=S.mugs_arch(MUGS, H), device=DEV)
        return gfd.nn.NsRotEquiTreeScaleGNN(arch=S.remus_arch(H), device=DEV)
    return _once(("model", kind), make)


def case_ids():
    n_hi, n_lo = remus_sizes()
    ids = [f"mus-{n}-{p}" for n in (300, 1000, 5000) for p in PRECISIONS]
    ids += [f"mus-{ROLLOUT_N}-f16x3-rollout2", "mus-1000-f16x3-grad"]
    ids += [f"remus-{n}-{p}" for n in (n_lo, n_hi) for p in ("bf16", "f16x3")]
    ids += [f"remus-{REMUS_RS2_N}-bf16", "mugs-5000-f16x3", f"part-mus-{PART_MUS_N}-f16x3-overlap1", f"part-mus-{PART_MUS_N}-f16x3-overlap0", f"part-remus-{n_hi}-bf16"]
    return ids


@contextlib.contextmanager
def _overlap(value):
    old = os.environ.get("G4C_DIST_OVERLAP")
    os.environ["G4C_DIST_OVERLAP"] = value
    try:
        yield
    finally:
        if old is None:
            del os.environ["G4C_DIST_OVERLAP"]
        else:
            os.environ["G4C_DIST_OVERLAP"] = old


def _partitioned(kind, n, overlap):
    import partition_harness as PH
    world = 2
    if kind == "mus":
        g, model = _mus(n), _model("mus")
        parts = _once(("parts", kind, n), lambda: P.build_partition(g, 2, world))
        maps = PH.MusMaps(parts)
        make = PH.mus_factory(g, model._PROGRAM, parts, DEV, lambda r, mesh: P.HipImpl(model), H, 3)
    else:
        g, model = _remus(n), _model("remus")
        parts = _once(("parts", kind, n), lambda: PR.build_remus_partition(g, world))
        maps = PH.RemusMaps(parts)
        make = PH.remus_factory(g, model._PROGRAM, parts, DEV, lambda r, mesh: PR.RemusHipImpl(model, mesh))
    with _overlap(overlap):
        _, preds = PH.run_ranks(world, make, PH.Transport(world, maps), DEV)
    torch.cuda.synchronize()
    return {f"pred.rank{r}": p for r, p in enumerate(preds)}


def run(case):
    """Run one case (call it inside `LaunchTrace()` to record it); returns its outputs by name."""
    words = case.split("-")
    partitioned = words[0] == "part"
    kind, n, prec, mode = (words[1:] if partitioned else words) + [""] * (4 - len(words) + partitioned)
    n = int(n)
    old = ops.set_mlp_precision(prec)
    try:
        if partitioned:
            return _partitioned(kind, n, "0" if mode == "overlap0" else "1")
        model = _model(kind)
        g = _once(("dev", kind, n), lambda: ({"mus": _mus, "remus": _remus}[kind](n) if kind != "mugs"
                                             else S.mugs_graph(n, levels=2, k=6, seed=n)).clone().to(DEV))
        if mode == "grad":
            model.zero_grad(set_to_none=True)
            with torch.enable_grad():
                pred = model.forward(g)
                pred.square().mean().backward()
            out = {"pred": pred.detach()}
            out.update({f"grad.{k}": p.grad.clone() for k, p in model.named_parameters()})
            model.zero_grad(set_to_none=True)
            return out
        with torch.no_grad():
            if mode == "rollout2":
                with Rollout(model, g.clone(), 2, capture=False, reorder=False) as ro:
                    ro.step()
                    ro.step()
                    return {"result": ro.result().clone()}
            return {"pred": model.forward(g)}
    finally:
        ops.set_mlp_precision(old)
        torch.cuda.synchronize()
