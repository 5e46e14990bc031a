"""Test-only references of the default-precision INFERENCE launches (ops.mlp_forward / ops.mp_layer_forward in "f16x3", "bf16x6" and
"fp32"), restated in plain torch, every tensor in feature order.  Nothing here calls the packing or launch code of graphs4cfd_amd:
inputs are the tensors a launch read, outputs are compared with what it wrote.

One launch is a `Launch`: weighted input blocks (grad_ref.Src: direct / indexed, col0 / width windows of a wider tensor, negate,
pre_act, aggregation on load through (off, perm), sum or mean; a narrow fp32 block is a weighted block like any other), additive
pre-multiplied blocks (`Add`), the layers, LayerNorm, output activation, residual window, output index.

- `ref64(launch)`: the fp64 value of the output rows, through grad_ref.mlp_forward (additive blocks enter as extra input blocks under
  identity columns of the first layer, which is exact).
- `evaluate(launch, dtype, linear)`: the same formula written out once more, one torch op per step, in any dtype and with any product
  rule.  dtype float32 + a plain matmul is the COMPARATOR (the yardstick: a reference-side quantity, never kernel output); float32 +
  `split_linear` is the torch emulation of the kernels' operand splits (and of their defects: `lose=`).
- `assert_as_accurate_as_fp32(got, ref64, cmp32, classes, what)`: per row class, max and mean |got - ref64| against max and mean
  |cmp32 - ref64|: max <= 2.0 max32 + 1e-6, mean <= 1.5 mean32 + 1e-7 (the margins of test_mlp_precisions_vs_fp64).  Every element
  belongs to exactly one class; nothing is left out.
- aggregates that the header promises bit for bit: `segment_reduce_fp32` (the kernel's own rows added in fp32 one after the other, IEEE
  quotient for the mean) and torch.equal.
- perturbations (negative controls; applied to a reference or to an emulated kernel, never to a launch): `lose_low_product`,
  `swap_adjacent_columns`, `row_in_next_segment`, `zero_last_partial_row`, `wrong_gather_row`, `skip_pre_act`,
  `head_from_pre_activation`.

Input classes (`mixed_rows`): "A" is the mix of test_mlp_precisions_vs_fp64 (N(0, 3^2), every 7th row x 1e3, every 11th x 1e-4);
"B" has N(0, 1) rows, every 7th with eight columns of magnitude 3e4 .. 6e4 (inside fp16's range: eight, not 128, so that the hidden
activations stay inside it too with default-initialised weights — clipping is the range tests' subject, not this file's) and every
11th scaled to 2^-20 (fp16 subnormals in both terms of the split); "C" is N(0, 1) with every 7th row x 30 and every 11th x 1e-4, the
mix whose bound certifies a launch (Source(bound=)) and that goes with the weight set that has one row x 64.

`REJECTION` holds, per input class and perturbation, the measured / allowed ratio by which the checker rejects it on the CPU
(tests/test_fwd_ref.py recomputes them)."""
from __future__ import annotations

from dataclasses import dataclass, replace
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import torch

from .grad_ref import F64, LN_EPS, Src, _act, _seg_ids, mlp_forward, move_boundary, rejects, swap_columns          # noqa: F401

Tensor = torch.Tensor
F32 = torch.float32
MAX_FACTOR, MAX_ABS = 2.0, 1e-6        # test_mlp_precisions_vs_fp64: err_max <= 2.0 err32_max + 1e-6
MEAN_FACTOR, MEAN_ABS = 1.5, 1e-7      #                              err_mean <= 1.5 err32_mean + 1e-7
CLASS_NAMES = ("ordinary", "large", "small")
F16_RANGE_END = 65504.0                # the largest fp16: an f16x3 launch flags a converted value of this magnitude or more


# ------------------------------------------------------------------ one launch
@dataclass
class Add:
    """An additive pre-multiplied block: rows p[index] (or p) of fp32 products, added to the first layer's pre-activation."""
    p: Tensor
    index: Optional[Tensor] = None
    col0: int = 0

    def rows(self, dtype, width: int) -> Tensor:
        t = self.p.to(dtype)[:, self.col0:self.col0 + width]
        return t if self.index is None else t[self.index.long()]


@dataclass
class Launch:
    srcs: Sequence[Src]
    weights: Sequence[Tensor]                 # weights[0]: [n_1, sum of the weighted blocks' widths]
    biases: Sequence[Optional[Tensor]]
    ln: Optional[Tuple[Tensor, Tensor]] = None
    act: Optional[str] = None
    adds: Sequence[Add] = ()
    resid: Optional[Tensor] = None
    resid_col0: int = 0
    out_idx: Optional[Tensor] = None          # row r of the launch is stored in row out_idx[r] of `out_init`
    out_init: Optional[Tensor] = None         # what the output tensor held before the launch (rows no index names keep it)
    narrow: Sequence[bool] = ()               # per weighted block: multiplied in fp32 on the vector ALUs (never converted to fp16)


def _segment(v: Tensor, off: Tensor, perm: Optional[Tensor], mean: bool) -> Tensor:
    """Row s = sum / mean of v[perm[p]] over segment s, in v's dtype: the rows of a segment added one after the other in their order
    (the same on every device and in every run — an index_add_ on a GPU adds in no fixed order), then the IEEE quotient."""
    dev = v.device
    o = off.long().to(dev)
    start, cnt = o[:-1], o[1:] - o[:-1]
    rows = v if perm is None else v[perm.long().to(dev)]
    out = torch.zeros((int(cnt.numel()), int(v.size(1))), dtype=v.dtype, device=dev)
    for j in range(int(cnt.max()) if cnt.numel() else 0):
        m = cnt > j
        out[m] = out[m] + rows[start[m] + j]
    if mean:
        out = out / cnt.clamp(min=1).to(v.dtype)[:, None]
    return out


def segment_reduce_fp32(rows: Tensor, off: Tensor, mean: bool) -> Tensor:
    """The fused aggregate as include/g4c.h promises it: the fp32 sum of a segment's stored rows in row order, `/ count` for the mean."""
    return _segment(rows.to(F32), off, None, mean)


def block_rows(s: Src, dtype) -> Tensor:
    x = s.x.to(dtype)[:, s.col0:s.col0 + s.w()]
    v = _act(x, s.pre_act)
    if s.segments is not None:
        v = _segment(v, s.segments[0], s.segments[1], s.seg_mean)
    elif s.index is not None:
        v = v[s.index.long()]
    return -v if s.negate else v


def plain_linear(x: Tensor, W: Tensor) -> Tensor:
    return x @ W.to(x.dtype).t()


def layer_norm(z: Tensor, gamma: Tensor, beta: Tensor) -> Tensor:
    mu = z.mean(1, keepdim=True)
    d = z - mu
    rstd = (d.pow(2).mean(1, keepdim=True) + LN_EPS).rsqrt()
    return d * rstd * gamma.to(z.dtype) + beta.to(z.dtype)


def evaluate(L: Launch, dtype=F32, linear: Callable[[Tensor, Tensor], Tensor] = plain_linear, scatter: bool = True) -> Dict[str, Tensor]:
    """{"z": the last layer's rows before LayerNorm, "y": the launch's rows, "out": the output tensor (scattered through out_idx)}."""
    X = torch.cat([block_rows(s, dtype) for s in L.srcs], 1)
    z = linear(X, L.weights[0])
    if L.biases[0] is not None:
        z = z + L.biases[0].to(dtype)
    for a in L.adds:
        z = z + a.rows(dtype, int(z.size(1)))
    for W, b in zip(L.weights[1:], L.biases[1:]):
        z = linear(_act(z, "selu"), W)
        if b is not None:
            z = z + b.to(dtype)
    y = _act(z if L.ln is None else layer_norm(z, L.ln[0], L.ln[1]), L.act)
    if L.resid is not None:
        y = y + L.resid.to(dtype)[:, L.resid_col0:L.resid_col0 + int(y.size(1))]
    return {"z": z, "y": y, "out": _scatter(L, y) if scatter else y}


def _scatter(L: Launch, y: Tensor) -> Tensor:
    if L.out_idx is None:
        return y
    out = L.out_init.to(y.dtype).clone()
    out[L.out_idx.long()] = y
    return out


def ref64(L: Launch) -> Dict[str, Tensor]:
    """The fp64 reference through grad_ref.mlp_forward: {"z", "y", "out"}."""
    srcs, W0 = list(L.srcs), L.weights[0].to(F64)
    n1 = int(W0.size(0))
    for a in L.adds:          # an additive block = an input block under identity columns (exact in fp64)
        srcs.append(Src(a.p, index=a.index, col0=a.col0, width=n1))
        W0 = torch.cat([W0, torch.eye(n1, dtype=F64, device=W0.device)], 1)
    f = mlp_forward(srcs, [W0] + [W.to(F64) for W in L.weights[1:]], list(L.biases), L.ln, L.act, L.resid, L.resid_col0)
    return {"z": f.z[-1], "y": f.y, "out": _scatter(L, f.y)}


def heads(y: Tensor, head_weights: Sequence[Tensor], dtype=F64) -> List[Tensor]:
    """W_h y of the launch's own output rows y (after LayerNorm and the output activation)."""
    return [y.to(dtype) @ W.to(dtype).t() for W in head_weights]


def mp_layer(msg: Launch, off: Tensor, mean: bool, upd_weights, upd_biases, upd_ln, v: Tensor, v_act: Optional[str], dtype=F64,
             e_rows: Optional[Tensor] = None, linear=plain_linear) -> Dict[str, Tensor]:
    """The one-launch MP layer: e' = msg, aggregate over `off`, v' = v_act(upd([aggregate | v])).  `e_rows`: the launch's own stored
    message rows — the aggregate then starts from them (the stage is checked locally); None: end to end."""
    e = evaluate(msg, dtype, linear)["y"] if e_rows is None else e_rows.to(dtype)
    agg = _segment(e, off, None, mean)
    upd = Launch([Src(agg), Src(v)], upd_weights, upd_biases, upd_ln, v_act)
    return {"e": e, "agg": agg, "v": evaluate(upd, dtype, linear)["y"]}


# ------------------------------------------------------------------ what a launch converts to fp16 (the f16x3 range flags)
@dataclass
class MpLayer:
    """ops.mp_layer_forward: the message launch `msg`, its rows aggregated over `off`, the node MLP on [aggregate | v]."""
    msg: Launch
    off: Tensor
    mean: bool
    weights: Sequence[Tensor]
    biases: Sequence[Optional[Tensor]]
    ln: Optional[Tuple[Tensor, Tensor]]
    v: Tensor
    v_act: Optional[str] = None


@dataclass
class Precomputed:
    """ops.mlp_forward_precomputed: layer 0's pre-activation is (first + adds[0]) + adds[1]; `weights` / `biases` are the layers left."""
    first: Tensor
    adds: Sequence[Add]
    weights: Sequence[Tensor]
    biases: Sequence[Optional[Tensor]]
    ln: Optional[Tuple[Tensor, Tensor]] = None
    act: Optional[str] = None


def _hidden(z: Tensor, weights, biases, sites: Dict[str, Tensor], linear, key: str = "") -> Tensor:
    """The layers behind the first: SELU(z_l) is converted (site h{l}) for every layer but the last; returns the last z."""
    for l, (W, b) in enumerate(zip(weights, biases), 1):
        h = _act(z, "selu")
        sites[f"{key}h{l}"] = h
        z = linear(h, W)
        if b is not None:
            z = z + b.to(z.dtype)
    return z


def converted(L: Launch, dtype=F64, heads: bool = False, linear=plain_linear, key: str = "") -> Dict[str, Tensor]:
    """The tensors one launch converts to fp16, by site, written out like `evaluate`:
      in{j}   weighted block j as it is parked: after the column window, `pre_act`, the gather or the sum / mean on load, BEFORE
              `negate` (the sign is folded into the packed weights).  A narrow block (fp32 vector path) and an additive block are no sites;
      h{l}    SELU(z_l) for every layer but the last (the additive blocks are inside z_1);
      heads   the output rows y (after LayerNorm and the output activation), when the launch has heads."""
    sites: Dict[str, Tensor] = {}
    X = []
    for j, s in enumerate(L.srcs):
        v = block_rows(replace(s, negate=False), dtype)
        if not (j < len(L.narrow) and L.narrow[j]):
            sites[f"{key}in{j}"] = v
        X.append(-v if s.negate else v)
    z = linear(torch.cat(X, 1), L.weights[0])
    if L.biases[0] is not None:
        z = z + L.biases[0].to(dtype)
    for a in L.adds:
        z = z + a.rows(dtype, int(z.size(1)))
    z = _hidden(z, L.weights[1:], L.biases[1:], sites, linear, key)
    if heads:
        sites[f"{key}heads"] = _act(z if L.ln is None else layer_norm(z, L.ln[0], L.ln[1]), L.act)
    return sites


def converted_mp_layer(M: MpLayer, dtype=F64, heads: bool = False, linear=plain_linear) -> Dict[str, Tensor]:
    """`converted` of the one-launch MP layer: msg.in0, msg.h*; upd.in0 (the aggregate), upd.in1 (v), upd.h*, upd.heads."""
    sites = converted(M.msg, dtype, False, linear, "msg.")
    e = evaluate(M.msg, dtype, linear)["y"]
    upd = Launch([Src(_segment(e, M.off, None, M.mean)), Src(M.v)], M.weights, M.biases, M.ln, M.v_act)
    sites.update(converted(upd, dtype, heads, linear, "upd."))
    return sites


def converted_precomputed(P: Precomputed, dtype=F64, linear=plain_linear) -> Dict[str, Tensor]:
    """`converted` of the launch without its first layer: no in0; h1 = SELU((first + p0[i0]) + p1[i1]), h2."""
    z = P.first.to(dtype)
    for a in P.adds:
        z = z + a.rows(dtype, int(z.size(1)))
    sites: Dict[str, Tensor] = {}
    _hidden(z, P.weights, P.biases, sites, linear)
    return sites


def precomputed_rows(P: Precomputed, dtype=F64, linear=plain_linear) -> Tensor:
    """The output rows of the launch without its first layer."""
    z = P.first.to(dtype)
    for a in P.adds:
        z = z + a.rows(dtype, int(z.size(1)))
    z = _hidden(z, P.weights, P.biases, {}, linear)
    return _act(z if P.ln is None else layer_norm(z, P.ln[0], P.ln[1]), P.act)


def sites_of(L, dtype=F64, heads: bool = False, linear=plain_linear) -> Dict[str, Tensor]:
    if isinstance(L, MpLayer):
        return converted_mp_layer(L, dtype, heads, linear)
    if isinstance(L, Precomputed):
        return converted_precomputed(L, dtype, linear)
    return converted(L, dtype, heads, linear)


def site_maxima(sites: Dict[str, Tensor]) -> Dict[str, float]:
    return {k: float(v.abs().max()) if v.numel() else 0.0 for k, v in sites.items()}


def expected_flag(sites: Dict[str, Tensor]) -> bool:
    """The contract of the f16x3 range flag: set exactly when a converted value has magnitude >= 65504."""
    return any(bool((v.abs() >= F16_RANGE_END).any()) for v in sites.values())


def emulated_flag(L, skip: Sequence[str] = (), heads: bool = False) -> bool:
    """The flag an f16x3 kernel would raise: the same sites computed in fp32 through the emulated operand split (conversions clipping
    at +-65504, as the kernels' do), `skip` naming the sites whose tracker is left out (negative controls)."""
    sites = sites_of(L, F32, heads, split_linear("f16x3", saturate=True))
    return expected_flag({k: v for k, v in sites.items() if k not in set(skip)})


# ------------------------------------------------------------------ the kernels' operand splits, emulated in torch
def _split_f16(x: Tensor, saturate: bool = False) -> Tuple[Tensor, Tensor]:
    """x = h + l 2^-11 (include/g4c.h, G4C_WFMT_F16X2): h = fp16(x), l = fp16((x - h) 2^11), both held in fp32.  `saturate`: both
    conversions clip at +-65504 instead of overflowing (the kernels' conversion mode; the range emulation)."""
    def f16(t):
        return (t.clamp(-F16_RANGE_END, F16_RANGE_END) if saturate else t).to(torch.float16).to(F32)
    h = f16(x)
    return h, f16((x - h) * 2048.0)


def _split_bf16(x: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    h = x.to(torch.bfloat16).to(F32)
    m = (x - h).to(torch.bfloat16).to(F32)
    return h, m, (x - h - m).to(torch.bfloat16).to(F32)


def split_linear(split: str, lose: Optional[str] = None, saturate: bool = False) -> Callable[[Tensor, Tensor], Tensor]:
    """The product rule of "f16x3" (three products, the 2^-11 terms in an accumulator of their own) or "bf16x6" (the six largest
    products of the exact three-way split), on fp32 tensors with fp32 sums.  `lose` (f16x3; negative controls): "wl_xh", "wh_xl" or
    "both" of the low products dropped.  `saturate` (f16x3): the row operand's conversions clip at the end of fp16's range."""
    def f16x3(x: Tensor, W: Tensor) -> Tensor:
        xh, xl = _split_f16(x.to(F32), saturate)
        wh, wl = _split_f16(W.to(F32))
        low = torch.zeros((), dtype=F32, device=x.device)
        if lose not in ("wh_xl", "both"):
            low = low + xl @ wh.t()
        if lose not in ("wl_xh", "both"):
            low = low + xh @ wl.t()
        return xh @ wh.t() + low * (2.0 ** -11)

    def bf16x6(x: Tensor, W: Tensor) -> Tensor:
        x0, x1, x2 = _split_bf16(x.to(F32))
        w0, w1, w2 = _split_bf16(W.to(F32))
        return (x0 @ w2.t() + x2 @ w0.t() + x1 @ w1.t()) + (x0 @ w1.t() + x1 @ w0.t()) + x0 @ w0.t()
    assert lose is None or split == "f16x3"
    return {"f16x3": f16x3, "bf16x6": bf16x6}[split]


# ------------------------------------------------------------------ the checker
STATS: List[Tuple[str, str, float, float, float, float]] = []      # (what, class, max err, mean err, max / allowed, mean / allowed)


def all_rows(n: int, device=None) -> Dict[str, Tensor]:
    return {"ordinary": torch.ones(n, dtype=torch.bool, device=device)}


def accuracy_ratios(got: Tensor, ref: Tensor, cmp32: Tensor, classes: Dict[str, Tensor]) -> Dict[str, Tuple[float, float, float, float]]:
    """Per class: (max |got - ref|, mean, max / allowed, mean / allowed) with allowed = 2 max32 + 1e-6 and 1.5 mean32 + 1e-7."""
    assert tuple(got.shape) == tuple(ref.shape) == tuple(cmp32.shape), f"shapes {tuple(got.shape)} {tuple(ref.shape)} {tuple(cmp32.shape)}"
    n = int(got.size(0))
    cover = torch.zeros(n, dtype=torch.int64, device=got.device)
    for m in classes.values():
        cover += m.to(got.device).to(torch.int64)
    assert bool((cover == 1).all()), "every row belongs to exactly one class (the share of elements left out is zero)"
    e, c = (got.to(F64) - ref.to(F64)).abs(), (cmp32.to(F64) - ref.to(F64)).abs()
    out = {}
    for name, m in classes.items():
        m = m.to(got.device)
        if not bool(m.any()):
            continue
        em, cm = e[m], c[m]
        if not bool(torch.isfinite(em).all()):
            out[name] = (float("inf"), float("inf"), float("inf"), float("inf"))
            continue
        mx, mean = float(em.max()), float(em.mean())
        out[name] = (mx, mean, mx / (MAX_FACTOR * float(cm.max()) + MAX_ABS), mean / (MEAN_FACTOR * float(cm.mean()) + MEAN_ABS))
    return out


def assert_as_accurate_as_fp32(got: Tensor, ref: Tensor, cmp32: Tensor, classes: Optional[Dict[str, Tensor]], what: str = ""):
    """`got` is as accurate as the plain fp32 evaluation `cmp32` of the same formula, both measured against the fp64 `ref`, in every
    row class separately.  Prints and returns the ratios."""
    classes = all_rows(int(got.size(0)), got.device) if classes is None else classes
    r = accuracy_ratios(got, ref, cmp32, classes)
    bad = []
    for name, (mx, mean, rmax, rmean) in r.items():
        print(f"  {what} [{name}]: max err {mx:.3e} ({rmax:.3f} of allowed), mean err {mean:.3e} ({rmean:.3f} of allowed)")
        STATS.append((what, name, mx, mean, rmax, rmean))
        if not (rmax <= 1.0 and rmean <= 1.0):
            bad.append(f"{name}: max {mx:.3e} = {rmax:.2f} x allowed, mean {mean:.3e} = {rmean:.2f} x allowed")
    if bad:
        raise AssertionError(f"{what}: less accurate than a plain fp32 evaluation — " + "; ".join(bad))
    return r


def worst_ratio(r) -> float:
    return max(max(v[2], v[3]) for v in r.values())


def comparator_agrees(ref: Tensor, cmp32: Tensor, what: str = "") -> None:
    """The fp32 comparator is an evaluation of the SAME formula: it agrees with the fp64 reference in its statistics — on the scale of
    each row's largest magnitude the mean deviation is below 1e-5 and the largest below 1e-3.  fp32 rounding of these launches is
    u n = 6e-8 x (at most 640 terms per sum, 3 + layers sums) ~ 1e-4 in the worst element before LayerNorm, which can amplify it by
    |z| / std(z); its mean is two orders below.  A wrong formula (a block, an index, a column, an activation) deviates by O(1).
    For LayerNorm'd rows: without the normalisation a row may be a small difference of large terms, which fp32 legitimately loses."""
    d = (cmp32.to(F64) - ref.to(F64)).abs() / ref.to(F64).abs().amax(1, keepdim=True).clamp_min(1.0)
    assert float(d.mean()) <= 1e-5 and float(d.max()) <= 1e-3, (f"{what}: the fp32 comparator and the fp64 reference disagree "
                                                                  f"(mean {float(d.mean()):.3e}, max {float(d.max()):.3e})")


# ------------------------------------------------------------------ inputs
def row_classes(n: int, device=None) -> Dict[str, Tensor]:
    """Every 7th row (from 0) is "large", every 11th (from 5) that is not large is "small", the rest "ordinary"."""
    r = torch.arange(n, device=device)
    large = r % 7 == 0
    small = (r % 11 == 5) & ~large
    return {"ordinary": ~(large | small), "large": large, "small": small}


def mixed_rows(n: int, width: int, mix: str, gen: torch.Generator) -> Tensor:
    """fp32 [n, width] rows of input class `mix` (module docstring); classes by `row_classes`."""
    c = row_classes(n)
    if mix == "A":
        x = 3.0 * torch.randn(n, width, generator=gen)
        x[c["large"]] *= 1e3
        x[c["small"]] *= 1e-4
    elif mix == "B":
        x = torch.randn(n, width, generator=gen)
        cols = torch.arange(5, width, max(width // 8, 1))[:8]
        big = (3e4 + 3e4 * torch.rand(n, cols.numel(), generator=gen)) * (2.0 * torch.randint(0, 2, (n, cols.numel()), generator=gen) - 1.0)
        xl = x[c["large"]]
        xl[:, cols] = big[c["large"]]
        x[c["large"]] = xl
        x[c["small"]] *= 2.0 ** -20
    elif mix == "C":
        x = torch.randn(n, width, generator=gen)
        x[c["large"]] *= 30.0
        x[c["small"]] *= 1e-4
    else:
        raise ValueError(mix)
    return x


def classes_through(classes: Dict[str, Tensor], index: Tensor) -> Dict[str, Tensor]:
    """Classes of the rows x[index]."""
    return {k: m.to(index.device)[index.long()] for k, m in classes.items()}


def classes_of_segments(classes: Dict[str, Tensor], off: Tensor, perm: Optional[Tensor] = None) -> Dict[str, Tensor]:
    """A segment is large when it holds a large row, else small when it holds a small row, else ordinary (empty ones too)."""
    dev = classes["large"].device
    seg = _seg_ids(off).to(dev)
    n_seg = int(off.numel()) - 1

    def any_in(m):
        m = m if perm is None else m[perm.long().to(dev)]
        return torch.zeros(n_seg, dtype=torch.int64, device=dev).index_add_(0, seg, m[:seg.numel()].to(torch.int64)) > 0
    large = any_in(classes["large"])
    small = any_in(classes["small"]) & ~large
    return {"ordinary": ~(large | small), "large": large, "small": small}


def default_weights(k_in: int, widths: Sequence[int], gen: torch.Generator, ln: bool, wset: str = "default", n_heads: int = 0):
    """nn.Linear's default initialisation (U(+-1 / sqrt(fan_in)) for weights and biases) and LayerNorm's (1, 0).  `wset`: "default";
    "ln" — LayerNorm gain and bias drawn at random (a swapped gamma / beta or a wrong column shows); "x64" — one row of the first
    layer's weight and one of the second's scaled x 64.  Returns (weights, biases, (gamma, beta) or None, head weights)."""
    Ws, bs, k = [], [], k_in
    for n_out in widths:
        a = k ** -0.5
        Ws.append((2 * torch.rand(n_out, k, generator=gen) - 1) * a)
        bs.append((2 * torch.rand(n_out, generator=gen) - 1) * a)
        k = n_out
    if wset == "x64":
        Ws[0][min(37, widths[0] - 1)] *= 64.0
        if len(Ws) > 1:
            Ws[1][min(90, widths[1] - 1)] *= 64.0
    lnp = None
    if ln:
        lnp = (torch.ones(k), torch.zeros(k))
        if wset == "ln":
            lnp = (0.5 + torch.rand(k, generator=gen), 0.5 * torch.randn(k, generator=gen))
    hs = [(2 * torch.rand(128, k, generator=gen) - 1) * (3 * k) ** -0.5 for _ in range(n_heads)]
    return Ws, bs, lnp, hs


# ------------------------------------------------------------------ perturbations (negative controls: a reference or an emulation only)
def lose_low_product(L: Launch, which: str) -> Tensor:
    """The launch's rows by an f16x3 kernel that loses "wl_xh", "wh_xl" or "both" of its 2^-11 products (torch emulation)."""
    return evaluate(L, F32, split_linear("f16x3", lose=which))["out"]


def swap_adjacent_columns(L: Launch, c: int, layer: int = 0) -> Launch:
    W = list(L.weights)
    W[layer] = swap_columns(W[layer], c)
    return replace(L, weights=W)


def row_in_next_segment(L: Launch, j: int, s: int) -> Launch:
    """Block j aggregates on load: the boundary between segments s - 1 and s moved by one row."""
    srcs = list(L.srcs)
    off, perm = srcs[j].segments
    srcs[j] = replace(srcs[j], segments=(move_boundary(off, s), perm))
    return replace(L, srcs=srcs)


def zero_last_partial_row(y: Tensor) -> Tensor:
    """The last row of a partial 32-row tile zeroed (a reference's OUTPUT rows)."""
    assert y.size(0) % 32 != 0
    out = y.clone()
    out[-1] = 0
    return out


def wrong_gather_row(L: Launch, j: int, r: int, additive: bool = False) -> Launch:
    """Row r of block j (or of additive block j) read from its neighbour: one index off by one."""
    def bump(index, n):
        i = index.clone()
        i[r] = i[r] + 1 if int(i[r]) + 1 < n else i[r] - 1
        return i
    if additive:
        adds = list(L.adds)
        adds[j] = replace(adds[j], index=bump(adds[j].index, int(adds[j].p.size(0))))
        return replace(L, adds=adds)
    srcs = list(L.srcs)
    srcs[j] = replace(srcs[j], index=bump(srcs[j].index, int(srcs[j].x.size(0))))
    return replace(L, srcs=srcs)


def skip_pre_act(L: Launch, j: int) -> Launch:
    srcs = list(L.srcs)
    assert srcs[j].pre_act is not None
    srcs[j] = replace(srcs[j], pre_act=None)
    return replace(L, srcs=srcs)


def head_from_pre_activation(L: Launch, head_weights: Sequence[Tensor]) -> List[Tensor]:
    """The heads computed from the last layer's rows BEFORE LayerNorm and the output activation."""
    return heads(ref64(L)["z"], head_weights)


# measured / allowed of the worst class, per input class and perturbation, on the launch of tests/test_fwd_ref.py (`control_launch`);
# the test recomputes them (within a factor 1.5, the row-local ones within 4: the comparator's fp32 sums depend on the BLAS build and its thread count)
REJECTION: Dict[Tuple[str, str], float] = {
    ('A', 'lose_low_product:wl_xh'): 561,
    ('A', 'lose_low_product:wh_xl'): 552,
    ('A', 'lose_low_product:both'): 779,
    ('A', 'swap_adjacent_columns'): 2.48e+05,
    ('A', 'swap_adjacent_columns:layer2'): 3.07e+05,
    ('A', 'zero_last_partial_row'): 4.85e+05,
    ('A', 'skip_pre_act'): 8.41e+05,
    ('A', 'row_in_next_segment:ordinary'): 3.87e+04,
    ('A', 'wrong_gather_row:ordinary'): 4.2e+05,
    ('A', 'wrong_gather_row:additive:ordinary'): 5.18e+05,
    ('A', 'row_in_next_segment:large'): 1.83e+05,
    ('A', 'wrong_gather_row:large'): 5.32e+05,
    ('A', 'wrong_gather_row:additive:large'): 798,
    ('A', 'row_in_next_segment:small'): 7.54e+04,
    ('A', 'wrong_gather_row:small'): 7.78e+05,
    ('A', 'wrong_gather_row:additive:small'): 5.74e+05,
    ('A', 'head_from_pre_activation'): 3.57e+06,
    ('B', 'lose_low_product:wl_xh'): 549,
    ('B', 'lose_low_product:wh_xl'): 582,
    ('B', 'lose_low_product:both'): 779,
    ('B', 'swap_adjacent_columns'): 1.35e+05,
    ('B', 'swap_adjacent_columns:layer2'): 3.58e+05,
    ('B', 'zero_last_partial_row'): 4.88e+05,
    ('B', 'skip_pre_act'): 7.4e+05,
    ('B', 'row_in_next_segment:ordinary'): 1.89e+05,
    ('B', 'wrong_gather_row:ordinary'): 2.52e+05,
    ('B', 'wrong_gather_row:additive:ordinary'): 6.13e+05,
    ('B', 'row_in_next_segment:large'): 1.44e+05,
    ('B', 'wrong_gather_row:large'): 4.54e+05,
    ('B', 'wrong_gather_row:additive:large'): 150,
    ('B', 'row_in_next_segment:small'): 1.27e+05,
    ('B', 'wrong_gather_row:small'): 3.26e+05,
    ('B', 'wrong_gather_row:additive:small'): 1.12e+06,
    ('B', 'head_from_pre_activation'): 3.87e+06,
    ('C', 'lose_low_product:wl_xh'): 564,
    ('C', 'lose_low_product:wh_xl'): 557,
    ('C', 'lose_low_product:both'): 796,
    ('C', 'swap_adjacent_columns'): 2.24e+05,
    ('C', 'swap_adjacent_columns:layer2'): 3.11e+05,
    ('C', 'zero_last_partial_row'): 5.27e+05,
    ('C', 'skip_pre_act'): 9.18e+05,
    ('C', 'row_in_next_segment:ordinary'): 6.54e+04,
    ('C', 'wrong_gather_row:ordinary'): 2.5e+05,
    ('C', 'wrong_gather_row:additive:ordinary'): 6.66e+05,
    ('C', 'row_in_next_segment:large'): 2.18e+05,
    ('C', 'wrong_gather_row:large'): 5.07e+05,
    ('C', 'wrong_gather_row:additive:large'): 7.56e+04,
    ('C', 'row_in_next_segment:small'): 8e+04,
    ('C', 'wrong_gather_row:small'): 1.03e+06,
    ('C', 'wrong_gather_row:additive:small'): 7.04e+05,
    ('C', 'head_from_pre_activation'): 1.8e+06,
}
