"""Test-only fp64 references of the training path's backward (autograd.py + csrc/train_ops.hip + the `save` / `mul` forms of
g4c_mlp_run), restated in plain torch fp64, every tensor in feature order.  Nothing here calls the packing or launch code of
graphs4cfd_amd: inputs are the tensors a launch read, outputs are compared with what it wrote.

Two ways of comparing:

- `assert_exact`: bit for bit.  Used with integer-valued operands (`int_operand`) whose every partial sum stays below 2^24
  (`check_int_bound` asserts it on the sum of absolute values, which bounds every partial sum in any order).  fp32 sums of such
  values are exact in any order, and so is the three-way bf16 split of the fused kernel (an integer of magnitude <= 256 is one bf16
  plane), so a correct kernel matches the fp64 result exactly at any row count: a dropped, doubled or misplaced row fails at 600k
  rows as surely as at 33.
- `assert_fp32_class`: elementwise |got - ref| <= C * 2^-24 * n_eff * absref.  `absref` is the same computation on absolute values
  (|A| @ |B| + |bias|, slopes by magnitude); every reference below returns it next to its value.  `n_eff` is the longest chain of
  sequential fp32 roundings behind one output element, derived from the kernel code next to each use (helpers `n_eff_*`).  C = 2
  once for every bounded check: the classical bound of a recursive sum is n * u * sum|terms| (u = 2^-24), and C = 2 leaves room
  for the product roundings and the transcendental ulps folded into n_eff.

SELU branches: the slope `a > 0 ? scale : a + scale * alpha` is evaluated on the fp32 activations a launch saved or was given,
never on an fp64 recomputation — a pre-activation within an ulp of 0 can land on the other side of the kink in fp64, which moves one
gradient element by 70 %.  The tests take the activations a backward used from its own weight-gradient operands (both the saving
and the recompute path pass them there), so no row needs an allowance.  `Forward.ambiguous_rows` marks, from the fp64 forward, the
rows that hold a hidden pre-activation within its worst-case fp32 reach of 0 (|z| <= C u n_eff Z): every row where a launch took the
other branch than fp64 must lie among them, and the tests count both.

Perturbations (negative controls, applied to a reference's inputs only): `drop_row`, `move_boundary`, `swap_columns`,
`zero_last_partial_row`, `flip_slope`."""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import torch

Tensor = torch.Tensor
F64 = torch.float64

U = 2.0 ** -24                       # fp32 unit roundoff
C = 2.0                              # the one constant of every bounded check (module docstring)
SELU_SCALE = 1.0507009873554804934193349852946
SELU_ALPHA = 1.6732632423543772848170429916717
SELU_SA = SELU_SCALE * SELU_ALPHA    # slope just left of the kink; also the Lipschitz constant of SELU
LN_EPS = 1e-5


# ------------------------------------------------------------------ checkers
def assert_exact(got: Tensor, ref: Tensor, what: str = "") -> None:
    """Bit-exact: fp32 `got` equals the (integer-valued, fp32-representable) fp64 `ref` everywhere."""
    assert tuple(got.shape) == tuple(ref.shape), f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    r32 = ref.to(torch.float32)
    assert torch.equal(r32.to(F64), ref.to(F64)), f"{what}: reference is not fp32-representable (generator bound broken)"
    bad = got.to(torch.float32) != r32
    if bool(bad.any()):
        pos = bad.nonzero()[0].tolist()
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {pos}: "
                             f"got {float(got[tuple(pos)])} want {float(ref[tuple(pos)])}")


STATS: List[Tuple[str, float]] = []       # (what, measured / allowed) of every passing bounded check, for the test log


def assert_fp32_class(got: Tensor, ref: Tensor, absref: Tensor, n_eff: float, what: str = "", c: float = C) -> float:
    """Elementwise |got - ref| <= c * 2^-24 * n_eff * absref.  Returns the largest measured / allowed ratio (printed)."""
    assert tuple(got.shape) == tuple(ref.shape) == tuple(absref.shape), f"{what}: shapes {got.shape} {ref.shape} {absref.shape}"
    err = (got.to(F64) - ref.to(F64)).abs()
    allow = c * U * float(n_eff) * absref.to(F64)
    over = err > allow
    if bool(over.any()):
        i = int((err - allow).flatten().argmax())
        raise AssertionError(f"{what}: {int(over.sum())} of {err.numel()} elements outside c*u*n_eff*|ref| (n_eff {n_eff:.0f}); worst "
                             f"flat index {i}: |diff| {float(err.flatten()[i]):.3e} allowed {float(allow.flatten()[i]):.3e}")
    ratio = float((err / allow.clamp_min(1e-300)).max()) if err.numel() else 0.0
    STATS.append((what, ratio))
    print(f"  {what}: n_eff {n_eff:.0f}, max measured/allowed {ratio:.3e}")
    return ratio


def rejects(check, *args, **kw) -> bool:
    """True when the checker raises AssertionError (negative controls)."""
    try:
        check(*args, **kw)
    except AssertionError:
        return True
    return False


# ------------------------------------------------------------------ integer operands
def int_operand(shape, vmax: int, gen: torch.Generator, density: float = 1.0, device=None) -> Tensor:
    """fp32 tensor of integers in [-vmax, vmax] (a fraction `density` of them nonzero)."""
    x = torch.randint(-vmax, vmax + 1, tuple(shape), generator=gen, dtype=torch.int64)
    if density < 1.0:
        x = x * (torch.rand(tuple(shape), generator=gen) < density)
    return x.to(torch.float32).to(device) if device is not None else x.to(torch.float32)


def vmax_for(n_terms: int, n_factors: int = 2, cap: int = 8) -> int:
    """Largest integer magnitude v (<= cap) with n_terms * v^n_factors < 2^24."""
    v = cap
    while v > 1 and n_terms * v ** n_factors >= 2 ** 24:
        v -= 1
    return v


def check_int_bound(*abs_sums: Tensor) -> None:
    """Every partial sum of a contraction is bounded by the sum of the absolute values of its terms: assert those < 2^24."""
    for s in abs_sums:
        if s.numel():
            assert float(s.max()) < 2 ** 24, f"integer generator: a sum of |terms| reaches {float(s.max()):.0f} >= 2^24"


# ------------------------------------------------------------------ n_eff of the kernels (train_ops.hip)
def colsum_partials(rows: int) -> int:
    """g4c_colsum_partials."""
    return max(1, min(2048, (rows + 127) // 128))


def n_eff_colsum_stage(rows: int, chunk: int, width: int) -> int:
    """colsum_stage_kernel over `chunk` rows of a column: eight interleaved accumulators of ceil(chunk / (8 rpi)) terms, a 3-level
    tree over them, then the rpi row offsets added in order."""
    rpi = 256 // min(width, 256)
    return math.ceil(min(chunk, max(rows, 1)) / (8 * rpi)) + 3 + rpi


def n_eff_colsum(rows: int, width: int) -> int:
    g = colsum_partials(rows)
    chunk = max(1, -(-rows // g))
    return n_eff_colsum_stage(rows, chunk, width) + n_eff_colsum_stage(g, g, width)


def weight_grad_partials(rows: int) -> int:
    """g4c_weight_grad_partials (the cap of 512 is reached at 98,273 rows)."""
    return max(1, min(512, -(-rows // 32) // 6))


def n_eff_weight_grad(rows: int) -> int:
    """weight_grad_kernel: a workgroup's row chunk goes through one MFMA accumulator two rows per step (chunk / 2 roundings, +1
    for the pair), then the two colsum stages over the partial tiles (16 partials, then ceil(G / 16)); with_bias: the column sums
    of g, 2 rows per thread per slab over chunk rows + 16 in order."""
    G = weight_grad_partials(rows)
    slabs = -(-rows // 32)
    chunk = -(-slabs // G) * 32
    g2 = -(-G // 16)
    stages = n_eff_colsum_stage(G, -(-G // g2), 4096) + n_eff_colsum_stage(g2, g2, 4096)
    return chunk // 2 + 1 + 16 + stages


N_EFF_LN_ROW = 3 * (4 + 6) + 8      # layernorm_grad_kernel, one row: three wave reductions (4 columns per lane in order + a 6-level
#                                      shuffle tree: sum, variance, m1 / m2), rsqrtf (~2 ulp), the elementwise epilogue
N_EFF_ACT = 8                       # act_grad: exp2 / rcp (1 ulp each, hardware), the SELU / tanh arithmetic, the product
N_EFF_LAYER_K = 128                 # one 128-k layer of the fused kernel: an fp32 MFMA accumulator over 128 k per output
N_EFF_SPLIT = {"bf16x6": 2, "f16x3": 16}   # per layer: the dropped cross products of the operand split (bf16x3: ~2^-24 relative;
#                                            fp16 x2: lo*lo and the fp16 rounding of both lo parts, ~3 * 2^-22 = 12 u) + the bias add


# ------------------------------------------------------------------ elementwise pieces
def _act(x: Tensor, act: Optional[str]) -> Tensor:
    if act is None:
        return x
    if act == "selu":
        return torch.where(x > 0, SELU_SCALE * x, SELU_SA * torch.expm1(x))
    if act == "tanh":
        return torch.tanh(x)
    raise ValueError(act)


def selu_slope_out(a: Tensor) -> Tensor:
    """d SELU / dz from the output a = SELU(z) (the kernels' formula, train_ops.hip act_slope / mlp_fused.hip `mul`)."""
    a = a.to(F64)
    return torch.where(a > 0, torch.full_like(a, SELU_SCALE), a + SELU_SA)


def act_slope(ref: Tensor, act: Optional[str], from_input: bool) -> Tensor:
    """d act / dx given the fp32 output (from_input False) or input (True), in fp64; branches decided by the given fp32 values."""
    r = ref.to(F64)
    if act is None:
        return torch.ones_like(r)
    if act == "selu":
        return selu_slope_out(_act(r, "selu") if from_input else r)
    if act == "tanh":
        y = torch.tanh(r) if from_input else r
        return 1.0 - y * y
    raise ValueError(act)


def act_slope_abs(ref: Tensor, act: Optional[str], from_input: bool) -> Tensor:
    """The absolute-value form of act_slope: |terms| of the formula (SELU: |a| + scale * alpha; tanh: 1 + y^2)."""
    r = ref.to(F64)
    if act is None:
        return torch.ones_like(r)
    if act == "selu":
        a = _act(r, "selu") if from_input else r
        return torch.where(a > 0, torch.full_like(a, SELU_SCALE), a.abs() + SELU_SA)
    y = torch.tanh(r) if from_input else r
    return 1.0 + y * y


def act_grad(dy: Tensor, ref: Tensor, act: Optional[str], from_input: bool) -> Tuple[Tensor, Tensor]:
    """(dy * act'(.), |dy| * |act'|) — g4c_act_grad."""
    return dy.to(F64) * act_slope(ref, act, from_input), dy.to(F64).abs() * act_slope_abs(ref, act, from_input)


# ------------------------------------------------------------------ building blocks
def weight_bias_grad(g: Tensor, a: Tensor) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """(dW = g^T a, db = column sums of g, |g|^T |a|, column sums of |g|)."""
    g, a = g.to(F64), a.to(F64)
    return g.t() @ a, g.sum(0), g.abs().t() @ a.abs(), g.abs().sum(0)


def colsum(x: Tensor) -> Tuple[Tensor, Tensor]:
    x = x.to(F64)
    return x.sum(0), x.abs().sum(0)


def layernorm_grad(z: Tensor, gamma: Tensor, dy: Tensor, eps: float = LN_EPS, dy_abs: Optional[Tensor] = None,
                   z_abs: Optional[Tensor] = None):
    """Adjoint of y = LayerNorm(z) * gamma + beta (biased variance, eps inside the root): returns (dz, dgamma, dbeta) and their
    absolute-value forms.  xhat's magnitude carrier XH = |xhat| + rstd (Z + mean(Z)) covers the fp32 error of the mean and of z
    itself (Z = |z|, or the abs-forward of z when given)."""
    z, gamma, dy = z.to(F64), gamma.to(F64), dy.to(F64)
    G = dy.abs() if dy_abs is None else dy_abs.to(F64)
    Z = z.abs() if z_abs is None else z_abs.to(F64)
    mu = z.mean(1, keepdim=True)
    rstd = ((z - mu).pow(2).mean(1, keepdim=True) + eps).rsqrt()
    xh = (z - mu) * rstd
    gg = dy * gamma
    dz = rstd * (gg - gg.mean(1, keepdim=True) - xh * (gg * xh).mean(1, keepdim=True))
    XH = xh.abs() + rstd * (Z + Z.mean(1, keepdim=True))
    GG = G * gamma.abs()
    dz_abs = rstd * (GG + GG.mean(1, keepdim=True) + XH * (GG * XH).mean(1, keepdim=True))
    return (dz, (dy * xh).sum(0), dy.sum(0)), (dz_abs, (G * XH).sum(0), G.sum(0))


def gather(src: Tensor, idx: Optional[Tensor], scol0: int, width: int, pre_act: Optional[str] = None, negate: bool = False,
           dst: Optional[Tensor] = None, dcol0: int = 0, accumulate: bool = False) -> Tensor:
    """g4c_train_gather: dst[r, dcol0 + c] (+)= sign * pre_act(src[idx[r], scol0 + c]); returns the whole new dst (fp64)."""
    s = src.to(F64)[:, scol0:scol0 + width]
    v = _act(s if idx is None else s[idx.long()], pre_act)
    v = -v if negate else v
    if dst is None:
        return v
    out = dst.to(F64).clone()
    out[:, dcol0:dcol0 + width] = (out[:, dcol0:dcol0 + width] if accumulate else 0) + v
    return out


def _seg_ids(off: Tensor) -> Tensor:
    off = off.long().cpu()
    return torch.repeat_interleave(torch.arange(off.numel() - 1), off[1:] - off[:-1])


def segment_broadcast(dout: Tensor, off: Tensor, perm: Optional[Tensor], n_src: int, mean: bool, fp32: bool = True) -> Tensor:
    """g4c_segment_broadcast: every row of segment s (rows perm[p] for p in off[s] .. off[s+1], or p itself) receives dout[s], times
    the kernel's own fp32 scale 1.f / max(count, 1) in a fp32 product when `mean` (`fp32` False: dout / count in fp64); rows of no
    segment stay 0."""
    dev = dout.device
    seg = _seg_ids(off).to(dev)
    rows = (perm.long() if perm is not None else torch.arange(seg.numel(), device=dev)).to(dev)
    g = dout.to(torch.float32) if fp32 else dout.to(F64)
    if mean and not fp32:
        g = g / (off[1:] - off[:-1]).to(dev).clamp(min=1).to(F64)[:, None]
    elif mean:
        cnt = (off[1:] - off[:-1]).to(dev).clamp(min=1).to(torch.float32)
        g = g * (torch.ones_like(cnt) / cnt)[:, None]          # (fp32 division, fp32 product: the kernel's formula)
    out = torch.zeros((n_src, int(dout.size(1))), dtype=F64, device=dev)
    out[rows] = g.to(F64)[seg]
    return out


def segment_sum(x: Tensor, off: Tensor, perm: Optional[Tensor], mean: bool) -> Tensor:
    """Forward of an aggregation on load: row s = sum / mean of x[perm[p]] over segment s."""
    dev = x.device
    seg = _seg_ids(off).to(dev)
    rows = (perm.long() if perm is not None else torch.arange(seg.numel(), device=dev)).to(dev)
    n_seg = int(off.numel()) - 1
    out = torch.zeros((n_seg, int(x.size(1))), dtype=F64, device=dev).index_add_(0, seg, x.to(F64)[rows])
    if mean:
        out = out / (off[1:] - off[:-1]).to(dev).clamp(min=1).to(F64)[:, None]
    return out


def linear(x: Tensor, W: Tensor, b: Optional[Tensor] = None, act: Optional[str] = None) -> Tuple[Tensor, Tensor]:
    """(act(x W^T + b), |x| |W|^T + |b|) — autograd.linear / one nn.Linear."""
    x, W = x.to(F64), W.to(F64)
    y, ya = x @ W.t(), x.abs() @ W.abs().t()
    if b is not None:
        y, ya = y + b.to(F64), ya + b.to(F64).abs()
    return _act(y, act), ya


def chain_layer(d_next: Tensor, W: Tensor, act: Tensor, d_next_abs: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """One hidden layer of the backward chain: D[l] = (D[l+1] W[l]) * selu'(a[l]) with the slope of the fp32 activations a[l]."""
    d, W = d_next.to(F64), W.to(F64)
    Da = d.abs() if d_next_abs is None else d_next_abs.to(F64)
    s = selu_slope_out(act)
    return (d @ W) * s, (Da @ W.abs()) * s.abs()


def chain(g: Tensor, weights: Sequence[Tensor], acts: Sequence[Tensor], w_dense: Tensor):
    """autograd.backward_chain restated: D[L] = g; D[l] = (D[l+1] W[l]) * selu'(acts[l]) for l = L-1 .. 1; gX = D[1] W_dense.
    Returns ({l: D[l]}, {l: |D[l]|-form}, gX, |gX|-form)."""
    L = len(weights)
    D, Da = {L: g.to(F64)}, {L: g.to(F64).abs()}
    for l in range(L - 1, 0, -1):
        D[l], Da[l] = chain_layer(D[l + 1], weights[l], acts[l], Da[l + 1])
    return D, Da, D[1] @ w_dense.to(F64), Da[1] @ w_dense.to(F64).abs()


# ------------------------------------------------------------------ one fused MLP launch: forward and adjoint
@dataclass
class Src:
    """One input block of a fused MLP launch (ops.Source restated): fp32 rows `x` [n_x, >= col0 + width], read through `index`
    (int) or aggregated over `segments` = (off, perm or None) (sum, or mean when `seg_mean`), `pre_act` on load, then `negate`."""
    x: Tensor
    index: Optional[Tensor] = None
    col0: int = 0
    width: Optional[int] = None
    negate: bool = False
    pre_act: Optional[str] = None
    segments: Optional[Tuple[Tensor, Optional[Tensor]]] = None
    seg_mean: bool = True
    xa: Optional[Tensor] = None         # magnitude of x when it carries an upstream fp32 error (another launch's abs-forward); |x| if None

    def w(self) -> int:
        return int(self.x.size(1)) - self.col0 if self.width is None else int(self.width)

    def rows(self) -> Tuple[Tensor, Tensor]:
        """(block rows in fp64, their absolute-value form)."""
        x = self.x.to(F64)[:, self.col0:self.col0 + self.w()]
        v = _act(x, self.pre_act)
        va = v.abs() if self.xa is None else (SELU_SA if self.pre_act else 1.0) * self.xa.to(F64)[:, self.col0:self.col0 + self.w()]
        if self.segments is not None:
            off, perm = self.segments
            v, va = segment_sum(v, off, perm, self.seg_mean), segment_sum(va, off, perm, self.seg_mean)
        elif self.index is not None:
            v, va = v[self.index.long()], va[self.index.long()]
        return (-v if self.negate else v), va

    def adjoint(self, gx: Tensor, gxa: Tensor) -> Tuple[Tensor, Tensor]:
        """Gradient [n_x, x.size(1)] of the tensor from the gradient of the block's rows (and the absolute-value form)."""
        s = -1.0 if self.negate else 1.0
        gx, gxa = gx * s, gxa
        n_x, w = int(self.x.size(0)), self.w()
        if self.segments is not None:
            off, perm = self.segments
            gt = segment_broadcast(gx, off, perm, n_x, self.seg_mean, fp32=False)
            gta = segment_broadcast(gxa, off, perm, n_x, self.seg_mean, fp32=False)
        elif self.index is not None:
            i = self.index.long()
            gt = torch.zeros((n_x, w), dtype=F64, device=gx.device).index_add_(0, i, gx)
            gta = torch.zeros((n_x, w), dtype=F64, device=gx.device).index_add_(0, i, gxa)
        else:
            gt, gta = gx, gxa
        x = self.x[:, self.col0:self.col0 + w]
        gt, gta = gt * act_slope(x, self.pre_act, True), gta * act_slope_abs(x, self.pre_act, True)
        full, fulla = torch.zeros(tuple(self.x.shape), dtype=F64, device=gx.device), torch.zeros(tuple(self.x.shape), dtype=F64, device=gx.device)
        full[:, self.col0:self.col0 + w], fulla[:, self.col0:self.col0 + w] = gt, gta
        return full, fulla


@dataclass
class Forward:
    """An fp64 forward of one launch with its absolute-value form.  a[l] = input rows of layer l (a[0] = the concatenation X),
    z[l] = layer l's pre-activation; y0 = the rows before the output activation (after LayerNorm), y = the output."""
    X: Tensor
    XA: Tensor
    a: List[Tensor] = field(default_factory=list)
    A: List[Tensor] = field(default_factory=list)
    z: List[Tensor] = field(default_factory=list)
    Z: List[Tensor] = field(default_factory=list)
    y0: Optional[Tensor] = None
    Y0: Optional[Tensor] = None
    y: Optional[Tensor] = None
    n_fwd: List[int] = field(default_factory=list)      # n_eff of z[l]

    def ambiguous_rows(self, c: float = C) -> Tensor:
        """Rows with a hidden pre-activation inside its own fp32-class bound of 0: the fp32 launch may take either SELU branch."""
        bad = torch.zeros(int(self.X.size(0)), dtype=torch.bool, device=self.X.device)
        for l in range(len(self.z) - 1):
            bad |= (self.z[l].abs() <= c * U * self.n_fwd[l] * self.Z[l]).any(1)
        return bad


def mlp_forward(srcs: Sequence[Src], weights: Sequence[Tensor], biases: Sequence[Optional[Tensor]], ln=None, act: Optional[str] = None,
                resid: Optional[Tensor] = None, resid_col0: int = 0, split: str = "bf16x6") -> Forward:
    """act(LayerNorm(MLP(cat(blocks)))) (+ resid[:, resid_col0:]) in fp64 — `ln` = (gamma, beta) or None, SELU between layers."""
    parts = [s.rows() for s in srcs]
    X, XA = torch.cat([p[0] for p in parts], 1), torch.cat([p[1] for p in parts], 1)
    f = Forward(X, XA, [X], [XA])
    n = 0
    for l, (W, b) in enumerate(zip(weights, biases)):
        n += int(W.size(1)) + N_EFF_SPLIT[split]
        z, _ = linear(f.a[-1], W, b)
        za = linear(f.A[-1], W.abs(), None if b is None else b.abs())[0]     # (the propagated magnitude, not |a|)
        f.z.append(z); f.Z.append(za); f.n_fwd.append(n)
        if l < len(weights) - 1:
            f.a.append(_act(z, "selu")); f.A.append(SELU_SA * za)
    z, za = f.z[-1], f.Z[-1]
    if ln is not None:
        gamma, beta = ln[0].to(F64), ln[1].to(F64)
        mu = z.mean(1, keepdim=True)
        rstd = ((z - mu).pow(2).mean(1, keepdim=True) + LN_EPS).rsqrt()
        xh = (z - mu) * rstd
        f.y0 = xh * gamma + beta
        f.Y0 = (xh.abs() + rstd * (za + za.mean(1, keepdim=True))) * gamma.abs() + beta.abs()
    else:
        f.y0, f.Y0 = z, za
    f.y = _act(f.y0, act)
    if resid is not None:
        f.y = f.y + resid.to(F64)[:, resid_col0:resid_col0 + int(f.y.size(1))]
    return f


def mlp_adjoint(f: Forward, srcs: Sequence[Src], weights: Sequence[Tensor], ln=None, act: Optional[str] = None,
                dy: Optional[Tensor] = None, acts: Optional[Sequence[Tensor]] = None, z_last: Optional[Tensor] = None,
                resid: Optional[Tensor] = None, resid_col0: int = 0, dy_abs: Optional[Tensor] = None) -> Dict[str, Tuple[Tensor, Tensor]]:
    """Every gradient of one launch: {"W{l}", "b{l}", "gamma", "beta", "src{j}", "resid", "D{l}"} -> (value, absolute-value form).
    `acts` (the kernel's saved SELU outputs, acts[l] = input rows of layer l for l >= 1) and `z_last` (its saved pre-LayerNorm rows):
    slopes and products are then taken on those fp32 rows — the backward is checked layer-locally; without them the fp64 forward
    supplies both, and the carried fp32 error of the recomputed activations is folded into the absolute-value form.  `dy_abs`: the
    magnitude of an upstream gradient that carries fp32 error of its own (|dy| if None)."""
    L = len(weights)
    dy = dy.to(F64)
    out: Dict[str, Tuple[Tensor, Tensor]] = {}
    if resid is not None:
        r = torch.zeros(tuple(resid.shape), dtype=F64, device=dy.device)
        r[:, resid_col0:resid_col0 + int(dy.size(1))] = dy
        out["resid"] = (r, r.abs())
    g, ga = dy, (dy.abs() if dy_abs is None else dy_abs.to(F64))
    if act is not None:
        y_act = _act(f.y0, act)
        g = dy * act_slope(y_act, act, False)
        ga = ga * (act_slope_abs(y_act, act, False) + 2.0 * f.Y0)     # (+ the slope's change under y's fp32 error: 2 |y| dy <= 2 Y0 dy)
    own = acts is not None
    a = [f.a[0]] + ([a_.to(F64) for a_ in acts[1:]] if own else f.a[1:])
    A = [f.A[0]] + ([a_.to(F64).abs() for a_ in acts[1:]] if own else f.A[1:])
    if ln is not None:
        zl = f.z[-1] if z_last is None else z_last.to(F64)
        (g, dgam, dbet), (ga, dgam_a, dbet_a) = layernorm_grad(zl, ln[0], g, LN_EPS, ga, None if own else f.Z[-1])
        out["gamma"], out["beta"] = (dgam, dgam_a), (dbet, dbet_a)
    D, Da = {L: g}, {L: ga}
    for l in range(L - 1, -1, -1):
        out[f"W{l}"] = (D[l + 1].t() @ a[l], Da[l + 1].t() @ A[l])
        out[f"b{l}"] = (D[l + 1].sum(0), Da[l + 1].sum(0))
        if l == 0:
            break
        s = selu_slope_out(a[l])
        sa = s.abs() if own else s.abs() + A[l]            # (recomputed slope: moved by the fp32 error of a[l], carried by A[l])
        D[l], Da[l] = (D[l + 1] @ weights[l].to(F64)) * s, (Da[l + 1] @ weights[l].to(F64).abs()) * sa
    for l in range(1, L + 1):
        out[f"D{l}"] = (D[l], Da[l])
    gX, gXa = D[1] @ weights[0].to(F64), Da[1] @ weights[0].to(F64).abs()
    c0 = 0
    for j, s in enumerate(srcs):
        w = s.w()
        out[f"src{j}"] = s.adjoint(gX[:, c0:c0 + w], gXa[:, c0:c0 + w])
        c0 += w
    return out


def n_eff_mlp_grad(k_in: int, n_layers: int, rows: int, split: str = "bf16x6", ln: bool = True, max_deg: int = 1) -> int:
    """n_eff of every gradient of one fused-MLP training step: the forward (k_in + 128 per later layer, plus the operand split per
    layer), the output activation and LayerNorm adjoints, the backward chain (128 k + the bf16x6 split per layer, the first layer's
    input-gradient product over 128 outputs), the weight-gradient contraction over `rows` and the segmented sums of an index
    adjoint (`max_deg` rows in order)."""
    fwd = k_in + N_EFF_LAYER_K * (n_layers - 1) + N_EFF_SPLIT[split] * n_layers
    bwd = (N_EFF_LAYER_K + N_EFF_SPLIT["bf16x6"]) * n_layers + N_EFF_ACT + (N_EFF_LN_ROW if ln else 0)
    return fwd + bwd + max(n_eff_weight_grad(rows), n_eff_colsum(rows, 128)) + max_deg + N_EFF_ACT


# ------------------------------------------------------------------ perturbations (negative controls: reference inputs only)
def drop_row(x: Tensor, r: int) -> Tensor:
    """One row taken out of a contraction over rows (zeroed)."""
    y = x.clone()
    y[r] = 0
    return y


def move_boundary(off: Tensor, s: int) -> Tensor:
    """Segment boundary off[s] moved by one row (one row changes segment)."""
    o = off.clone()
    o[s] += 1 if int(o[s]) < int(o[s + 1]) else -1
    return o


def swap_columns(W: Tensor, c: int) -> Tensor:
    """Weight columns c and c + 1 swapped (both inside one 32-k step when c % 32 != 31)."""
    assert c % 32 != 31
    V = W.clone()
    V[:, [c, c + 1]] = W[:, [c + 1, c]]
    return V


def zero_last_partial_row(x: Tensor) -> Tensor:
    """The last row of a partial 32-row tile zeroed."""
    assert x.size(0) % 32 != 0
    return drop_row(x, int(x.size(0)) - 1)


def flip_slope(act: Tensor, r: int, c: int) -> Tensor:
    """One SELU slope from the other branch: the saved activation a[r, c] replaced by a value on the other side of 0 whose slope
    differs (a > 0: a tiny negative value, slope scale * alpha; a <= 0: a tiny positive one, slope scale)."""
    a = act.clone()
    a[r, c] = -1e-30 if float(a[r, c]) > 0 else 1e-30
    return a


# ------------------------------------------------------------------ GNBlock (nn/blocks.py GNBlock.forward, mean aggregation, no output activation)
def gnblock_forward(v: Tensor, e: Tensor, row: Tensor, col: Tensor, edge_params, node_params, split: str = "bf16x6"):
    """e' = edge_mlp(cat(e, v[row], v[col])), v' = node_mlp(cat(mean of e' over col, v)); `*_params` = (weights, biases, (gamma, beta)).
    Returns (edge Forward, node Forward, edge sources, node sources); the aggregation reads e' through the CSR of col (off, perm)."""
    n = int(v.size(0))
    perm = torch.argsort(col, stable=True)
    off = torch.zeros(n + 1, dtype=torch.int64, device=v.device)
    off[1:] = torch.cumsum(torch.bincount(col, minlength=n), 0)
    es = [Src(e), Src(v, index=row), Src(v, index=col)]
    fe = mlp_forward(es, *edge_params, split=split)
    ns = [Src(fe.y, segments=(off, perm), seg_mean=True, xa=fe.Y0), Src(v)]
    fv = mlp_forward(ns, *node_params, split=split)
    return fe, fv, es, ns


def gnblock_adjoint(fe: Forward, fv: Forward, es, ns, edge_params, node_params, dv: Tensor, de: Tensor, edge_own=(None, None),
                    node_own=(None, None)):
    """Gradients of <dv, v'> + <de, e'>: {"edge.*", "node.*", "v", "e"} -> (value, absolute-value form).  `*_own` = (acts, z_last)
    of the launch's backward (mlp_adjoint)."""
    gn = mlp_adjoint(fv, ns, node_params[0], node_params[2], None, dv, acts=node_own[0], z_last=node_own[1])
    d_e, d_ea = gn["src0"]
    ge = mlp_adjoint(fe, es, edge_params[0], edge_params[2], None, de.to(F64) + d_e, dy_abs=de.to(F64).abs() + d_ea,
                     acts=edge_own[0], z_last=edge_own[1])
    out = {}
    for pre, gr in (("edge.", ge), ("node.", gn)):
        for k, val in gr.items():
            if k[0] in "Wbg":            # W{l}, b{l}, gamma, beta
                out[pre + k] = val
    out["e"] = ge["src0"]
    out["v"] = (gn["src1"][0] + ge["src1"][0] + ge["src2"][0], gn["src1"][1] + ge["src1"][1] + ge["src2"][1])
    return out
