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
`zero_last_partial_row`, `flip_slope`; for the linear adjoints of the multi-scale / REMuS path also `dedup_index`, `unmask_row`,
`swap_unit_columns` (and a mean restated as a sum: the `mean` argument of the reference itself).

Linear ops of the multi-scale, gMuS and REMuS models (autograd.py below _FusedMLP) and the blocks made of them: the section
"linear adjoints" restates each op and its adjoint, "blocks" composes them with `mlp_forward` / `mlp_adjoint` the way `gnblock_*` do."""
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


REL_LARGEST = 2e-5                   # assert_rel_largest: what tests/test_gpu_train.py holds GNBlock's gradients to against float64 autograd


def assert_rel_largest(got: Tensor, ref: Tensor, what: str = "", rel: float = REL_LARGEST) -> float:
    """max |got - ref| <= rel * max |ref|: a whole tensor against its largest entry.  Beside `assert_fp32_class` where that bound is
    loose: through a LayerNorm adjoint and two or three 128-term products of absolute values, c * u * n_eff * absref of a block's
    gradient exceeds the gradient itself, so a row that is simply missing passes it; fp32 arithmetic itself stays some 1e-6 of the
    largest entry away from fp64 on these blocks.  Returns measured / allowed (logged like the other ratios)."""
    assert tuple(got.shape) == tuple(ref.shape), f"{what}: shape {tuple(got.shape)} vs {tuple(ref.shape)}"
    if not ref.numel():
        return 0.0
    err, scale = float((got.to(F64) - ref.to(F64)).abs().max()), float(ref.to(F64).abs().max())
    ratio = err / max(rel * scale, 1e-300)
    print(f"  {what}: max |diff| {err:.3e}, largest entry {scale:.3e}, measured/allowed {ratio:.3e}")
    assert err <= rel * scale, f"{what}: max |diff| {err:.3e} above {rel:g} of the largest entry {scale:.3e}"
    STATS.append((what, ratio))
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
                resid: Optional[Tensor] = None, resid_col0: int = 0, dy_abs: Optional[Tensor] = None,
                y_act: Optional[Tensor] = None) -> Dict[str, Tuple[Tensor, Tensor]]:
    """Every gradient of one launch: {"W{l}", "b{l}", "gamma", "beta", "src{j}", "resid", "D{l}"} -> (value, absolute-value form).
    `acts` (the kernel's saved SELU outputs, acts[l] = input rows of layer l for l >= 1) and `z_last` (its saved pre-LayerNorm rows):
    slopes and products are then taken on those fp32 rows — the backward is checked layer-locally; without them the fp64 forward
    supplies both, and the carried fp32 error of the recomputed activations is folded into the absolute-value form.  `dy_abs`: the
    magnitude of an upstream gradient that carries fp32 error of its own (|dy| if None).  `y_act`: the activated fp32 rows the launch
    wrote (before the residual) — the output activation's slope is then taken from them, as the backward does (a SELU output within an
    ulp of 0 takes the launch's branch, not fp64's)."""
    L = len(weights)
    dy = dy.to(F64)
    out: Dict[str, Tuple[Tensor, Tensor]] = {}
    if resid is not None:
        r = torch.zeros(tuple(resid.shape), dtype=F64, device=dy.device)
        r[:, resid_col0:resid_col0 + int(dy.size(1))] = dy
        out["resid"] = (r, r.abs())
    g, ga = dy, (dy.abs() if dy_abs is None else dy_abs.to(F64))
    if act is not None:
        y_act = _act(f.y0, act) if y_act is None else y_act.to(F64)
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


# ------------------------------------------------------------------ linear adjoints (autograd.py below _FusedMLP)
# Each returns (value, the same computation on absolute values).  An adjoint takes the upstream gradient and, where that carries fp32
# error of its own, its magnitude (`dout_abs`; |dout| if None).
def _abs_of(d: Tensor, d_abs: Optional[Tensor]) -> Tensor:
    return d.to(F64).abs() if d_abs is None else d_abs.to(F64)


def _index_add(n: int, idx: Tensor, rows: Tensor) -> Tensor:
    return torch.zeros((n, int(rows.size(1))), dtype=F64, device=rows.device).index_add_(0, idx.long().to(rows.device), rows)


def gather_rows_adjoint(dout: Tensor, idx: Tensor, n: int, dout_abs: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """Adjoint of out = x[idx] for x [n, w]: row r of dx = the sum of the rows p of dout with idx[p] == r; a row never read gets +0."""
    return _index_add(n, idx, dout.to(F64)), _index_add(n, idx, _abs_of(dout, dout_abs))


def act_terms_abs(x: Tensor, act: Optional[str]) -> Tensor:
    """Magnitude of the terms of the kernels' activation formulas (g4c_common.h selu_f / tanh_f): SELU = scale * max(x, 0) +
    (scale alpha e - scale alpha) with e = exp(min(x, 0)), tanh = 1 - 2 / (exp(2 |x|) + 1).  Near 0 both cancel, so the bound there is
    absolute, not relative to the value."""
    x = x.to(F64)
    if act is None:
        return x.abs()
    if act == "selu":
        return SELU_SCALE * x.clamp(min=0.0) + SELU_SA * (torch.exp(x.clamp(max=0.0)) + 1.0)
    if act == "tanh":
        return 1.0 + 2.0 / (torch.exp(2.0 * x.abs().clamp(max=20.0)) + 1.0)
    raise ValueError(act)


def segment_reduce(src: Tensor, off: Tensor, perm: Optional[Tensor], mean: bool, act: Optional[str] = None,
                   src_act: Optional[str] = None) -> Tuple[Tensor, Tensor]:
    """act(sum | mean of src_act(src[perm[p]]) over segment s) — ops.segment_reduce.  Magnitude: the terms of `src_act`'s formula
    summed like the rows; through `act` a value s with magnitude S carries L S + the terms of act's formula at s (L the activation's
    Lipschitz constant: scale * alpha for SELU, 1 for tanh)."""
    x = src.to(F64)
    out, mag = segment_sum(_act(x, src_act), off, perm, mean), segment_sum(act_terms_abs(x, src_act), off, perm, mean)
    if act is None:
        return out, mag
    return _act(out, act), (SELU_SA if act == "selu" else 1.0) * mag + act_terms_abs(out, act)


def segment_reduce_adjoint(dout: Tensor, src: Tensor, out: Tensor, off: Tensor, perm: Optional[Tensor], mean: bool,
                           act: Optional[str] = None, src_act: Optional[str] = None, dout_abs: Optional[Tensor] = None):
    """Adjoint of `segment_reduce` with respect to src [n_src, w]: dout times the slope of `act` at the given fp32 output rows `out`,
    handed to every row of the segment (divided by the segment's length for a mean), times the slope of `src_act` at the given fp32
    input; rows of no segment get +0."""
    n_src = int(src.size(0))
    g, ga = act_grad(dout, out, act, False)
    if dout_abs is not None:
        ga = dout_abs.to(F64) * act_slope_abs(out, act, False)
    gs = segment_broadcast(g, off, perm, n_src, mean, fp32=False)
    gsa = segment_broadcast(ga, off, perm, n_src, mean, fp32=False)
    return gs * act_slope(src, src_act, True), gsa * act_slope_abs(src, src_act, True)


def segment_totals_sequential(w: Tensor, off: Tensor) -> Tensor:
    """fp32 totals of w over each segment, added one after the other in segment order starting from +0 (what a lane of
    g4c_segment_reduce / g4c_weighted_segment_mean computes): [n_seg] fp32."""
    w = w.detach().reshape(-1).to(torch.float32).cpu()
    off = off.long().cpu()
    lens = off[1:] - off[:-1]
    tot = torch.zeros(int(lens.numel()), dtype=torch.float32)
    for j in range(int(lens.max()) if lens.numel() else 0):
        on = lens > j
        tot[on] = tot[on] + w[off[:-1][on] + j]               # (one fp32 addition per step: IEEE, no re-association)
    return tot


def segment_coefficients(w: Tensor, off: Tensor) -> Tensor:
    """w_p / (sum of w over p's segment) as fp32 [n, 1]: the total by `segment_totals_sequential`, then one fp32 division — the value
    autograd._segment_coefficients holds, bit for bit."""
    w32 = w.detach().reshape(-1).to(torch.float32).cpu()
    tot = segment_totals_sequential(w32, off)
    return (w32 / tot[_seg_ids(off)]).reshape(-1, 1)


def weighted_mean(x: Tensor, x_idx: Tensor, w: Tensor, off: Tensor, n_out: Optional[int] = None,
                  out_idx: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """knn_interpolate: row s = sum_p w_p x[x_idx[p]] / sum_p w_p over segment s (rows in segment order); with `out_idx` row s lands
    at out_idx[s] of a zero [n_out, w] tensor.  (A segment without rows is 0 / 0 here as in the reference: the plans have none.)"""
    dev = x.device
    seg = _seg_ids(off).to(dev)
    n_seg = int(off.numel()) - 1
    wd = w.reshape(-1, 1).to(F64).to(dev)
    xr = x.to(F64)[x_idx.long().to(dev)]
    den = _index_add(n_seg, seg, wd.abs())
    rows, mag = _index_add(n_seg, seg, xr * wd) / den, _index_add(n_seg, seg, xr.abs() * wd.abs()) / den
    if out_idx is None and (n_out is None or n_out == n_seg):
        return rows, mag
    full, fulla = (torch.zeros((int(n_out), int(x.size(1))), dtype=F64, device=dev) for _ in range(2))
    o = torch.arange(n_seg, device=dev) if out_idx is None else out_idx.long().to(dev)
    full[o], fulla[o] = rows, mag
    return full, fulla


def weighted_mean_adjoint(dout: Tensor, x_idx: Tensor, w: Tensor, off: Tensor, n_x: int, out_idx: Optional[Tensor] = None,
                          dout_abs: Optional[Tensor] = None, coef: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """Adjoint of `weighted_mean` with respect to x [n_x, w]: dx[r] = sum over p with x_idx[p] == r of (w_p / total) dout[row of p's
    segment]; output rows `out_idx` does not name pass nothing.  `coef`: the coefficients to use instead of w / total in fp64."""
    dev = dout.device
    seg = _seg_ids(off).to(dev)
    n_seg = int(off.numel()) - 1
    d, da = dout.to(F64), _abs_of(dout, dout_abs)
    o = torch.arange(n_seg, device=dev) if out_idx is None else out_idx.long().to(dev)
    d, da = d[o], da[o]
    if coef is None:
        wd = w.reshape(-1, 1).to(F64).to(dev)
        coef = wd / _index_add(n_seg, seg, wd)[seg]
    coef = coef.reshape(-1, 1).to(F64).to(dev)
    return _index_add(n_x, x_idx.to(dev), d[seg] * coef), _index_add(n_x, x_idx.to(dev), da[seg] * coef.abs())


def project_to_edges(v: Tensor, node: Optional[Tensor], unit: Tensor, n_feat: int, v_abs: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """(v[node][:, :2F].view(E, F, 2) * unit[:, None]).sum(-1); without `node` edge e reads row e."""
    E = int(unit.size(0))
    u = unit.to(F64)
    rows = v.to(F64) if node is None else v.to(F64)[node.long()]
    mag = _abs_of(v, v_abs) if node is None else _abs_of(v, v_abs)[node.long()]
    rows, mag = rows[:E, :2 * n_feat].reshape(E, n_feat, 2), mag[:E, :2 * n_feat].reshape(E, n_feat, 2)
    return (rows * u[:, None]).sum(-1), (mag * u.abs()[:, None]).sum(-1)


def project_to_edges_adjoint(dout: Tensor, node: Optional[Tensor], unit: Tensor, v_shape: Sequence[int],
                             dout_abs: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """Adjoint with respect to v of shape `v_shape`: dv[node[e], 2f + c] += dout[e, f] unit[e, c]; rows and columns the forward did
    not read get +0."""
    E, n_feat = int(dout.size(0)), int(dout.size(1))
    u = unit.to(F64)
    t = (dout.to(F64)[:, :, None] * u[:, None, :]).reshape(E, 2 * n_feat)
    ta = (_abs_of(dout, dout_abs)[:, :, None] * u.abs()[:, None, :]).reshape(E, 2 * n_feat)
    dv, dva = (torch.zeros(tuple(v_shape), dtype=F64, device=dout.device) for _ in range(2))
    if node is None:
        dv[:E, :2 * n_feat], dva[:E, :2 * n_feat] = t, ta
    else:
        dv[:, :2 * n_feat], dva[:, :2 * n_feat] = _index_add(int(v_shape[0]), node, t), _index_add(int(v_shape[0]), node, ta)
    return dv, dva


def edge_scalar_to_node_vector(e: Tensor, unit_inv: Tensor, k: int, e_abs: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """out[n, 2 f + c] = sum_j unit_inv[n, c, j] e[n k + j, f] (feature-major flatten of unit_inv @ e.view(n, k, F))."""
    n, F_ = int(unit_inv.size(0)), int(e.size(1))
    ui = unit_inv.to(F64).reshape(n, 2, k)
    out = (ui @ e.to(F64).reshape(n, k, F_)).transpose(1, 2).reshape(n, 2 * F_)
    mag = (ui.abs() @ _abs_of(e, e_abs).reshape(n, k, F_)).transpose(1, 2).reshape(n, 2 * F_)
    return out, mag


def edge_scalar_to_node_vector_adjoint(dout: Tensor, unit_inv: Tensor, k: int, dout_abs: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """Adjoint with respect to e [n k, F]: de[n k + j, f] = sum_c unit_inv[n, c, j] dout[n, 2 f + c]."""
    n = int(unit_inv.size(0))
    F_ = int(dout.size(1)) // 2
    ui = unit_inv.to(F64).reshape(n, 2, k)
    d = dout.to(F64).reshape(n, F_, 2).transpose(1, 2)                     # [n, 2, F]
    da = _abs_of(dout, dout_abs).reshape(n, F_, 2).transpose(1, 2)
    return (ui.transpose(1, 2) @ d).reshape(n * k, F_), (ui.abs().transpose(1, 2) @ da).reshape(n * k, F_)


# n_eff of these launches, counted from segment_reduce.hip / remus_ops.hip / train_ops.hip and the torch products of autograd.py
def n_eff_segment_reduce(max_deg: int, mean: bool, act: Optional[str] = None, src_act: Optional[str] = None) -> int:
    """One lane adds the segment's rows in order (max_deg roundings), one division for a mean, N_EFF_ACT per activation."""
    return max(max_deg, 1) + (1 if mean else 0) + (N_EFF_ACT if act else 0) + (N_EFF_ACT if src_act else 0)


def n_eff_segment_reduce_adjoint(mean: bool, act: Optional[str] = None, src_act: Optional[str] = None) -> int:
    """No sum: the slope products (N_EFF_ACT each), and for a mean the fp32 reciprocal of the length and its product (2)."""
    return 1 + (2 if mean else 0) + (N_EFF_ACT if act else 0) + (N_EFF_ACT if src_act else 0)


def n_eff_weighted_mean(k: int) -> int:
    """k products and k additions of the numerator (rounded separately at worst), k additions of the denominator, the quotient."""
    return 3 * k + 1


def n_eff_weighted_mean_adjoint(k: int, max_mult: int) -> int:
    """The coefficient (k additions of the total, the quotient), its product with the gradient row, then the segmented sum over the
    positions that read one row of x (max_mult additions in order)."""
    return k + 2 + max(max_mult, 1)


N_EFF_PROJECT = 3                    # project_to_edges_kernel: two products and a sum, rounded separately


def n_eff_project_adjoint(max_mult: int) -> int:
    """One product per element, then (through an index) the segmented sum over the edges of a node."""
    return 1 + max(max_mult, 1)


def n_eff_e2n(k: int) -> int:
    """edge_scalar_to_node_vector_kernel: k fused multiply-adds in order."""
    return k


# ------------------------------------------------------------------ perturbations of the linear adjoints
def dedup_index(idx: Tensor) -> Tuple[Tensor, Tensor]:
    """A duplicated gather index counted once: (positions kept, their indices) with every row of x named by one position only."""
    i = idx.long().cpu()
    first = torch.ones_like(i, dtype=torch.bool)
    order = torch.argsort(i, stable=True)
    s = i[order]
    first[order[1:]] = s[1:] != s[:-1]
    keep = first.nonzero().reshape(-1)
    return keep.to(idx.device), idx[keep.to(idx.device)]


def unmask_row(out_idx: Tensor, n_out: int) -> Tensor:
    """A masked output row given gradient: the last named row replaced by a row the mask does not name."""
    named = torch.zeros(n_out, dtype=torch.bool)
    named[out_idx.long().cpu()] = True
    free = (~named).nonzero().reshape(-1)
    o = out_idx.clone()
    o[-1] = int(free[-1])
    return o


def swap_unit_columns(unit: Tensor) -> Tensor:
    """The two columns of every unit vector swapped."""
    return unit.flip(-1)


# ------------------------------------------------------------------ blocks (nn/blocks.py other than MLP / GNBlock)
def _grads(pre: str, gr: Dict[str, Tuple[Tensor, Tensor]], out: Dict[str, Tuple[Tensor, Tensor]]) -> None:
    for k, val in gr.items():
        if k[0] in "Wbg":            # W{l}, b{l}, gamma, beta
            out[pre + k] = val


def mp_forward(v: Tensor, e: Tensor, row: Tensor, col: Tensor, msg_params, upd_params, v_src: Optional[Tensor] = None,
               e_pre_act: Optional[str] = None, act: Optional[str] = None, split: str = "bf16x6"):
    """The shared body of GNBlock / EdgeMP / DownEdgeMP (blocks._mp_step, mean aggregation): e' = msg([pre_act(e) | s[row] | v[col]])
    with senders s = v_src or v, v' = act(upd([mean of e' over col | v])).  `gnblock_forward` is this with no activations and
    v_src None; EdgeMP reads (e, a, angle_index) for (v, e, edge_index), DownEdgeMP (e2, a12, angle_index12) with v_src = e1.
    Returns (message Forward, update Forward, message sources, update sources)."""
    n = int(v.size(0))
    perm = torch.argsort(col, stable=True)
    off = torch.zeros(n + 1, dtype=torch.int64, device=v.device)
    off[1:] = torch.cumsum(torch.bincount(col, minlength=n), 0)
    ms = [Src(e, pre_act=e_pre_act), Src(v if v_src is None else v_src, index=row), Src(v, index=col)]
    fm = mlp_forward(ms, *msg_params, split=split)
    us = [Src(fm.y, segments=(off, perm), seg_mean=True, xa=fm.Y0), Src(v)]
    fu = mlp_forward(us, *upd_params, act=act, split=split)
    return fm, fu, ms, us


def mp_adjoint(fm: Forward, fu: Forward, ms, us, msg_params, upd_params, dv: Tensor, de: Optional[Tensor], act: Optional[str] = None,
               msg_own=(None, None), upd_own=(None, None), v_act: Optional[Tensor] = None):
    """Gradients of <dv, v'> + <de, e'> (de None: e' is read by nobody): {"msg.*", "upd.*", "v", "e", "v_src"} -> (value,
    absolute-value form); "v_src" only when the senders are another tensor.  `*_own` = (acts, z_last) of each launch's backward,
    `v_act` = the activated fp32 v' the update launch wrote (mlp_adjoint)."""
    gu = mlp_adjoint(fu, us, upd_params[0], upd_params[2], act, dv, acts=upd_own[0], z_last=upd_own[1], y_act=v_act)
    d_e, d_ea = gu["src0"]
    if de is not None:
        d_e, d_ea = d_e + de.to(F64), d_ea + de.to(F64).abs()
    gm = mlp_adjoint(fm, ms, msg_params[0], msg_params[2], None, d_e, dy_abs=d_ea, acts=msg_own[0], z_last=msg_own[1])
    out: Dict[str, Tuple[Tensor, Tensor]] = {}
    _grads("msg.", gm, out)
    _grads("upd.", gu, out)
    out["e"] = gm["src0"]
    if ms[1].x is ms[2].x:
        out["v"] = (gu["src1"][0] + gm["src1"][0] + gm["src2"][0], gu["src1"][1] + gm["src1"][1] + gm["src2"][1])
    else:
        out["v"] = (gu["src1"][0] + gm["src2"][0], gu["src1"][1] + gm["src2"][1])
        out["v_src"] = gm["src1"]
    return out


edge_mp_forward, edge_mp_adjoint = mp_forward, mp_adjoint          # EdgeMP: a GNBlock with (edges, angles) for (nodes, edges)


def down_edge_mp_forward(e1: Tensor, e2: Tensor, a12: Tensor, row: Tensor, col: Tensor, angle_params, edge_params,
                         act: Optional[str] = None, split: str = "bf16x6"):
    """DownEdgeMP: senders are the fine edges e1[row], receivers the coarse edges e2[col]; only e2' leaves the block."""
    return mp_forward(e2, a12, row, col, angle_params, edge_params, v_src=e1, act=act, split=split)


def down_edge_mp_adjoint(fm, fu, ms, us, angle_params, edge_params, de2: Tensor, act: Optional[str] = None, **own):
    """{"msg.*" (angle MLP), "upd.*" (edge MLP), "e1", "e2", "a12"}."""
    g = mp_adjoint(fm, fu, ms, us, angle_params, edge_params, de2, None, act, **own)
    g["e1"], g["e2"], g["a12"] = g.pop("v_src"), g.pop("v"), g.pop("e")
    return g


def pool_edge(edge_attr: Tensor, off: Tensor, perm: Optional[Tensor], mean: bool = True, src_act: Optional[str] = None):
    """The feature part of pool_edge: coarse edge s = mean | sum of src_act(edge_attr[perm[p]]) over the fine edges of segment s of
    the pooling plan (fine edges inside one cluster are in no segment)."""
    return segment_reduce(edge_attr, off, perm, mean, None, src_act)


def pool_edge_adjoint(dout: Tensor, edge_attr: Tensor, off: Tensor, perm: Optional[Tensor], mean: bool = True,
                      src_act: Optional[str] = None):
    return segment_reduce_adjoint(dout, edge_attr, dout, off, perm, mean, None, src_act)


def down_mp_forward(rel: Tensor, field: Tensor, cluster, params, split: str = "bf16x6") -> Tuple[Forward, List[Src], Tensor, Tensor]:
    """DownMP's node part before its activation: m = down_mlp([rel | field]), pooled = mean of m over the clusters of the plan
    `cluster` = (off, perm).  Returns (Forward of the MLP, its sources, pooled rows, their magnitude)."""
    srcs = [Src(rel), Src(field)]
    f = mlp_forward(srcs, *params, split=split)
    return f, srcs, segment_sum(f.y, cluster[0], cluster[1], True), segment_sum(f.Y0, cluster[0], cluster[1], True)


def down_mp_adjoint(f: Forward, srcs, params, cluster, dpooled: Tensor, pooled_out: Tensor, act: Optional[str] = None, own=(None, None)):
    """{"W*", "b*", "gamma", "beta", "rel", "field"} of <dpooled, act(pooled)>; the activation's slope at the given fp32 output."""
    n = int(f.X.size(0))
    g, ga = act_grad(dpooled, pooled_out, act, False)
    dm = segment_broadcast(g, cluster[0], cluster[1], n, True, fp32=False)
    dma = segment_broadcast(ga, cluster[0], cluster[1], n, True, fp32=False)
    gr = mlp_adjoint(f, srcs, params[0], params[2], None, dm, dy_abs=dma, acts=own[0], z_last=own[1])
    out: Dict[str, Tuple[Tensor, Tensor]] = {}
    _grads("", gr, out)
    out["rel"], out["field"] = gr["src0"], gr["src1"]
    return out


def up_mp_forward(rel: Tensor, field_lr: Tensor, parent: Tensor, field_hr_old: Tensor, params, act: Optional[str] = None,
                  split: str = "bf16x6") -> Tuple[Forward, List[Src]]:
    """UpMP: act(up_mlp([-rel | field_lr[parent] | field_hr_old]))."""
    srcs = [Src(rel, negate=True), Src(field_lr, index=parent), Src(field_hr_old)]
    return mlp_forward(srcs, *params, act=act, split=split), srcs


def up_mp_adjoint(f: Forward, srcs, params, dy: Tensor, act: Optional[str] = None, own=(None, None), y_act: Optional[Tensor] = None):
    """{"W*", "b*", "gamma", "beta", "rel", "field_lr", "field_hr_old"}."""
    gr = mlp_adjoint(f, srcs, params[0], params[2], act, dy, acts=own[0], z_last=own[1], y_act=y_act)
    out: Dict[str, Tuple[Tensor, Tensor]] = {}
    _grads("", gr, out)
    out["rel"], out["field_lr"], out["field_hr_old"] = gr["src0"], gr["src1"], gr["src2"]
    return out


def up_edge_mp_forward(edge_attr2: Tensor, unit_inv2: Tensor, k: int, x_idx: Tensor, w: Tensor, off: Tensor, n_total: int,
                       out_idx: Optional[Tensor], col1: Tensor, unit1: Tensor, edge_attr1: Tensor, params, act: Optional[str] = None,
                       split: str = "bf16x6"):
    """UpEdgeMP: coarse edge scalars -> node vectors (edge_scalar_to_node_vector), interpolated to the fine nodes (weighted_mean; the
    rows `out_idx` names of a zero [n_total, 2F] tensor), projected on the fine edges (project_to_edges through their receivers `col1`),
    then act(up_mlp([projection | edge_attr1])).  Returns (Forward, sources)."""
    F_ = int(edge_attr2.size(1))
    v2, v2a = edge_scalar_to_node_vector(edge_attr2, unit_inv2, k)
    v1, v1a = weighted_mean(v2, x_idx, w, off, n_total, out_idx)
    v1a = weighted_mean(v2a, x_idx, w, off, n_total, out_idx)[0]
    p, pa = project_to_edges(v1, col1, unit1, F_, v_abs=v1a)
    srcs = [Src(p, xa=pa), Src(edge_attr1)]
    return mlp_forward(srcs, *params, act=act, split=split), srcs


def up_edge_mp_adjoint(f: Forward, srcs, params, dy: Tensor, unit_inv2: Tensor, k: int, x_idx: Tensor, w: Tensor, off: Tensor,
                       n_total: int, out_idx: Optional[Tensor], col1: Tensor, unit1: Tensor, act: Optional[str] = None,
                       own=(None, None), y_act: Optional[Tensor] = None):
    """{"W*", "b*", "gamma", "beta", "edge_attr1", "edge_attr2"}: the MLP's adjoint, then the three linear adjoints in turn."""
    gr = mlp_adjoint(f, srcs, params[0], params[2], act, dy, acts=own[0], z_last=own[1], y_act=y_act)
    out: Dict[str, Tuple[Tensor, Tensor]] = {}
    _grads("", gr, out)
    out["edge_attr1"] = gr["src1"]
    n2 = int(unit_inv2.size(0))
    F_ = int(gr["src0"][0].size(1))
    dv1, dv1a = project_to_edges_adjoint(gr["src0"][0], col1, unit1, (n_total, 2 * F_), dout_abs=gr["src0"][1])
    dv2, dv2a = weighted_mean_adjoint(dv1, x_idx, w, off, n2, out_idx, dout_abs=dv1a)
    out["edge_attr2"] = edge_scalar_to_node_vector_adjoint(dv2, unit_inv2, k, dout_abs=dv2a)
    return out
