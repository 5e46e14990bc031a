"""Test-only fp64 references of the memory-bound helper launches (csrc/segment_reduce.hip, csrc/remus_ops.hip), restated in plain
torch fp64, every tensor in feature order.  Nothing here calls the packing or launch code of graphs4cfd_amd: inputs are the tensors
a launch read, outputs are compared with what it wrote.  The checkers, the integer generators and the constants U, C, N_EFF_ACT are
those of oracle/grad_ref.py (its docstring states both ways of comparing); every bounded reference returns (value, absref), absref
being the same computation on absolute values.

An activation behind a sum: |act(s + d) - act(s)| <= L |d| with L the activation's Lipschitz constant (SELU: scale * alpha, tanh:
1), so the magnitude carried through it is L * absref(s) + the magnitude of the activation's own formula (`act_abs`), the rule of
grad_ref.mlp_forward (A = SELU_SA * Z).

Perturbations (negative controls, applied to a reference's inputs or output only): grad_ref.move_boundary, `drop_last_row`,
`drop_last_weight`, `swap_unit`, the other endpoint's index (the caller passes it), `roll_shifted`, the step written to slot t + 1
(the caller passes t + 1), `layer_norm(denom=width + 1)`; `layer_norm_one_pass_fp32` is a WRONG implementation (one-pass variance
E[x^2] - E[x]^2 in fp32) that the LayerNorm bound must reject on rows with a large common offset."""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

from .grad_ref import (C, F64, N_EFF_ACT, SELU_ALPHA, SELU_SA, SELU_SCALE, U, _seg_ids, assert_exact,      # noqa: F401
                       assert_fp32_class, check_int_bound, int_operand, move_boundary, rejects, vmax_for)

Tensor = torch.Tensor
F32 = torch.float32


# ------------------------------------------------------------------ activations (g4c_common.h selu_f / tanh_f)
def act_value(x: Tensor, act: Optional[str]) -> Tensor:
    """F.selu / torch.tanh in fp64 (torch's SELU constants)."""
    x = x.to(F64)
    if act is None:
        return x
    if act == "selu":
        return torch.where(x > 0, SELU_SCALE * x, SELU_SA * torch.expm1(torch.clamp(x, max=0.0)))
    if act == "tanh":
        return torch.tanh(x)
    raise ValueError(act)


def act_abs(x: Tensor, act: Optional[str]) -> Tensor:
    """Magnitude of the terms of the kernels' formulas: SELU = scale * max(x, 0) + (scale alpha e - scale alpha), e = exp(min(x, 0));
    tanh = 1 - 2 / (exp(2 |x|) + 1).  Near 0 both cancel (a negative SELU input of 1e-8 is the difference of two numbers of
    magnitude scale * alpha), so the bound there is absolute, not relative to the value."""
    x = x.to(F64)
    if act is None:
        return x.abs()
    if act == "selu":
        return SELU_SCALE * x.clamp(min=0.0) + SELU_SA * (torch.exp(x.clamp(max=0.0)) + 1.0)
    if act == "tanh":
        return 1.0 + 2.0 / (torch.exp(2.0 * x.abs().clamp(max=20.0)) + 1.0)
    raise ValueError(act)


def lipschitz(act: Optional[str]) -> float:
    return SELU_SA if act == "selu" else 1.0


def through_act(s: Tensor, s_abs: Tensor, act: Optional[str]) -> Tuple[Tensor, Tensor]:
    """(act(s), magnitude) of an activation applied to a value s that carries an fp32 error bounded through s_abs (module docstring)."""
    if act is None:
        return s, s_abs
    return act_value(s, act), lipschitz(act) * s_abs + act_abs(s, act)


def activation(x: Tensor, act: Optional[str]) -> Tuple[Tensor, Tensor]:
    """g4c_activation_inplace: (act(x), act_abs(x)); n_eff = N_EFF_ACT (the product x log2(e), v_exp_f32 and v_rcp_f32 at 1 ulp each, the
    SELU / tanh arithmetic)."""
    return act_value(x, act), act_abs(x, act)


# ------------------------------------------------------------------ segmented sums
def _rows(off: Tensor, perm: Optional[Tensor]) -> Tuple[Tensor, Tensor]:
    seg = _seg_ids(off)
    rows = perm.long().cpu()[: seg.numel()] if perm is not None else torch.arange(seg.numel())
    return seg, rows


def counts(off: Tensor) -> Tensor:
    off = off.long().cpu()
    return off[1:] - off[:-1]


def segment_reduce(src: Tensor, off: Tensor, perm: Optional[Tensor], mean: bool, src_act: Optional[str] = None,
                   act: Optional[str] = None) -> Tuple[Tensor, Tensor]:
    """g4c_segment_reduce: out[s] = act(sum | mean over p in off[s] .. off[s+1] of src_act(src[perm[p]])) (row p itself without a
    permutation; `perm` may name only some of the rows of a larger src, in any order); mean = sum / max(count, 1).
    n_eff = the longest segment (one accumulator per column adds its rows in plan order; the masked slots of a batch of eight add
    +0, which rounds nothing) + 1 for the mean's division + N_EFF_ACT per activation: `n_eff_segment_reduce`."""
    src = src.to(F64).cpu()
    seg, rows = _rows(off, perm)
    n_seg = int(off.numel()) - 1
    v, va = activation(src, src_act) if src_act is not None else (src, src.abs())
    out = torch.zeros((n_seg, int(src.size(1))), dtype=F64).index_add_(0, seg, v[rows])
    outa = torch.zeros((n_seg, int(src.size(1))), dtype=F64).index_add_(0, seg, va[rows])
    if mean:
        cnt = counts(off).clamp(min=1).to(F64)[:, None]
        out, outa = out / cnt, outa / cnt
    return through_act(out, outa, act)


def n_eff_segment_reduce(off: Tensor, mean: bool, src_act: Optional[str], act: Optional[str]) -> int:
    c = counts(off)
    longest = int(c.max()) if c.numel() else 0
    return max(longest, 1) + (1 if mean else 0) + N_EFF_ACT * ((src_act is not None) + (act is not None))


def segment_mean_fp32(src: Tensor, off: Tensor, perm: Optional[Tensor]) -> Tensor:
    """The mean of INTEGER rows as the kernel forms it: the exact sum (below 2^24), then ONE correctly rounded fp32 division by
    (float)max(count, 1) — the library is built without fast-math.  Returned as fp64 holding fp32 values: compared bit for bit."""
    s, sa = segment_reduce(src, off, perm, False)
    check_int_bound(sa)
    cnt = counts(off).clamp(min=1).to(F32)[:, None]
    return (s.to(F32) / cnt).to(F64)


def weighted_segment_mean(x: Tensor, x_idx: Tensor, w: Tensor, off: Tensor, out_idx: Optional[Tensor] = None,
                          out_init: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """g4c_weighted_segment_mean: out[o(s)] = sum_p x[x_idx[p]] w[p] / sum_p w[p] over segment s, o(s) = out_idx[s] or s; rows that
    out_idx does not name keep out_init (their absref is 0: they must be untouched).
    n_eff = the longest segment + 1 (`n_eff_weighted_mean`): the numerator is one accumulator over the segment, the division is one
    rounding; the product roundings and the denominator's own sum (positive weights: relative error <= count u) are what C = 2 is
    for."""
    x, w = x.to(F64).cpu(), w.to(F64).cpu().reshape(-1)
    seg = _seg_ids(off)
    n_seg, width = int(off.numel()) - 1, int(x.size(1))
    xi = x_idx.long().cpu()
    num = torch.zeros((n_seg, width), dtype=F64).index_add_(0, seg, x[xi] * w[:, None])
    numa = torch.zeros((n_seg, width), dtype=F64).index_add_(0, seg, x[xi].abs() * w[:, None].abs())
    den = torch.zeros(n_seg, dtype=F64).index_add_(0, seg, w)[:, None]
    val, vala = num / den, numa / den.abs()
    if out_idx is None and out_init is None:
        return val, vala
    base = out_init.to(F64).cpu().clone()
    basea = torch.zeros_like(base)
    o = out_idx.long().cpu() if out_idx is not None else torch.arange(n_seg)
    base[o, :width], basea[o, :width] = val, vala
    return base, basea


def n_eff_weighted_mean(off: Tensor) -> int:
    c = counts(off)
    return max(int(c.max()) if c.numel() else 0, 1) + 1


# ------------------------------------------------------------------ REMuS-GNN helpers
def project_to_edges(v: Tensor, node: Optional[Tensor], unit: Tensor, n_feat: int) -> Tuple[Tensor, Tensor]:
    """g4c_project_to_edges in fp64: out[e, f] = v[n(e), 2f] unit[e, 0] + v[n(e), 2f+1] unit[e, 1], n(e) = node[e] or e."""
    x0, x1, u = _project_operands(v, node, unit, n_feat)
    return x0 * u[:, :1] + x1 * u[:, 1:], x0.abs() * u[:, :1].abs() + x1.abs() * u[:, 1:].abs()


def project_to_edges_fp32(v: Tensor, node: Optional[Tensor], unit: Tensor, n_feat: int) -> Tensor:
    """The kernel's stated fp32 contract (no fma contraction): each product rounded to fp32 — formed in fp64, where the product of
    two fp32 values is exact, then rounded once — and their sum rounded to fp32."""
    x0, x1, u = _project_operands(v, node, unit, n_feat)
    p0, p1 = (x0 * u[:, :1]).to(F32), (x1 * u[:, 1:]).to(F32)
    return (p0.to(F64) + p1.to(F64)).to(F32)


def _project_operands(v, node, unit, n_feat):
    v, u = v.to(F64).cpu(), unit.to(F64).cpu()
    rows = v[node.long().cpu()] if node is not None else v[: int(u.size(0))]
    pairs = rows[:, : 2 * n_feat].reshape(rows.size(0), n_feat, 2)
    return pairs[:, :, 0], pairs[:, :, 1], u


def edge_scalar_to_node_vector(e: Tensor, unit_inv: Tensor, k: int) -> Tuple[Tensor, Tensor]:
    """g4c_edge_scalar_to_node_vector: out[n, 2f + c] = sum_j unit_inv[n, c, j] e[n k + j, f].  n_eff = k (one fma chain of k terms)."""
    e, ui = e.to(F64).cpu(), unit_inv.to(F64).cpu()
    n, f = int(ui.size(0)), int(e.size(1))
    ek = e[: n * k].reshape(n, k, f)
    ui = ui.reshape(n, 2, k)
    out = torch.einsum("ncj,njf->nfc", ui, ek).reshape(n, 2 * f)
    outa = torch.einsum("ncj,njf->nfc", ui.abs(), ek.abs()).reshape(n, 2 * f)
    return out, outa


def swap_unit(unit: Tensor) -> Tensor:
    """The two components of every unit vector (or of unit_inv's two rows per node) swapped."""
    return unit.flip(1) if unit.dim() == 2 else unit.flip(-2)


# ------------------------------------------------------------------ column helpers
def copy_cols(src: Tensor, dst: Tensor, dcol0: int, scol0: int, width: int, idx: Optional[Tensor], n_rows: int) -> Tensor:
    """g4c_copy_cols: the whole new dst — dst[r, dcol0 : dcol0 + width] = src[idx[r] or r, scol0 : scol0 + width] for r < n_rows."""
    out = dst.to(F64).cpu().clone()
    s = src.to(F64).cpu()
    rows = idx.long().cpu()[:n_rows] if idx is not None else torch.arange(n_rows)
    out[:n_rows, dcol0:dcol0 + width] = s[rows, scol0:scol0 + width]
    return out


def add_cols(a: Tensor, a_col0: int, b: Tensor) -> Tensor:
    """g4c_add_cols: a[:, a_col0 : a_col0 + width] + b as ONE fp32 addition (the fp64 sum of two fp32 values rounded once)."""
    b = b.to(F64).cpu()
    n, w = int(b.size(0)), int(b.size(1))
    return (a.to(F64).cpu()[:n, a_col0:a_col0 + w] + b).to(F32)


# ------------------------------------------------------------------ LayerNorm
def layer_norm(x: Tensor, gamma: Optional[Tensor], beta: Optional[Tensor], eps: float, act: Optional[str] = None,
               denom: Optional[int] = None) -> Tuple[Tensor, Tensor]:
    """g4c_layer_norm in two passes (mean, then the centred sum of squares; biased variance, eps inside the root).  absref =
    (|x| + mean|x|) rstd |gamma| + |beta|: the fp32 error of the mean and of x - mean is relative to |x| and mean|x|, not to the
    centred value.  `denom` (negative control only): the normaliser used in place of `width`."""
    x = x.to(F64).cpu()
    w = float(x.size(1) if denom is None else denom)
    mu = x.sum(1, keepdim=True) / w
    var = (x - mu).pow(2).sum(1, keepdim=True) / w
    rstd = (var + eps).rsqrt()
    g = torch.ones(x.size(1), dtype=F64) if gamma is None else gamma.to(F64).cpu()
    b = torch.zeros(x.size(1), dtype=F64) if beta is None else beta.to(F64).cpu()
    y = (x - mu) * rstd * g + b
    ya = (x.abs() + x.abs().sum(1, keepdim=True) / w) * rstd * g.abs() + b.abs()
    return through_act(y, ya, act)


def n_eff_layer_norm(width: int, act: Optional[str] = None) -> int:
    """layer_norm_rows_kernel, one element: two wave reductions (sum, centred squares), each ceil(width / 64) columns added in order
    by one lane, a six-level butterfly and the division by width; then the subtraction, the square's and eps's roundings,
    rsqrtf (~2 ulp), the product with rstd and the fma with gamma / beta: 8; + N_EFF_ACT with an activation."""
    return 2 * (math.ceil(width / 64) + 6 + 1) + 8 + (N_EFF_ACT if act is not None else 0)


def layer_norm_one_pass_fp32(x: Tensor, gamma: Optional[Tensor], beta: Optional[Tensor], eps: float) -> Tensor:
    """A WRONG LayerNorm for the negative control: variance as E[x^2] - E[x]^2 in fp32 (clamped at 0).  With a common offset of 1e4
    the two terms are 1e8 and their fp32 difference carries an error of several units: the result is off by far more than the bound
    of the two-pass kernel allows."""
    x = x.to(F32).cpu()
    w = float(x.size(1))
    mu = x.sum(1, keepdim=True) / w
    var = ((x * x).sum(1, keepdim=True) / w - mu * mu).clamp(min=0.0)
    y = (x - mu) * (var + eps).rsqrt()
    if gamma is not None:
        y = y * gamma.to(F32).cpu()
    if beta is not None:
        y = y + beta.to(F32).cpu()
    return y


# ------------------------------------------------------------------ rollout bookkeeping
def rollout_advance(field: Tensor, pred: Tensor, outputs: Tensor, t: int, layout: str) -> Tuple[Tensor, Tensor, int]:
    """g4c_rollout_advance (GNN.solve's bookkeeping): the field's columns rolled left by nf with pred appended, pred written into
    step t's slot of `outputs` — layout "rows": [n_nodes, >= nf * steps], columns nf t .. nf (t + 1); layout "steps":
    [steps, n_nodes, nf], block t — and the step index t + 1.  Everything else is returned as it was."""
    f, p, o = field.to(F64).cpu(), pred.to(F64).cpu(), outputs.to(F64).cpu().clone()
    nf = int(p.size(1))
    new = torch.cat((f[:, nf:], p), 1)
    if layout == "rows":
        o[:, nf * t:nf * (t + 1)] = p
    elif layout == "steps":
        o[t] = p
    else:
        raise ValueError(layout)
    return new, o, t + 1


def roll_shifted(field: Tensor, pred: Tensor, d: int) -> Tensor:
    """Perturbed new field: the kept columns rolled by nf + d instead of nf (d = +-1)."""
    f, p = field.to(F64).cpu(), pred.to(F64).cpu()
    nf, cols = int(p.size(1)), int(f.size(1))
    return torch.cat((torch.roll(f, -(nf + d), 1)[:, : cols - nf], p), 1)


# ------------------------------------------------------------------ perturbations of segmented inputs
def last_row_of(off: Tensor, perm: Optional[Tensor], s: int) -> int:
    p = int(off[s + 1]) - 1
    assert p >= int(off[s]), f"segment {s} is empty"
    return int(perm[p]) if perm is not None else p


def drop_last_row(src: Tensor, off: Tensor, perm: Optional[Tensor], s: int, value: float = 0.0) -> Tensor:
    """The last row of segment s taken out of the sum (set to `value`: 0, or the argument at which a src_act vanishes)."""
    y = src.clone()
    y[last_row_of(off, perm, s)] = value
    return y


def drop_last_weight(w: Tensor, off: Tensor, s: int) -> Tensor:
    """The last neighbour of segment s taken out of a weighted mean (weight 0: numerator and denominator both lose it)."""
    y = w.clone()
    y.reshape(-1)[last_row_of(off, None, s)] = 0.0
    return y
