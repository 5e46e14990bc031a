"""Test-only reference of the rounded-bf16 MLP arithmetic (`set_mlp_precision("bf16")`, BASELINE config 3): what ONE fused MLP launch
computes, restated in plain torch fp64 from the module's `state_dict` weights, every tensor in feature order.  Nothing here calls the
packing or column-ordering code of graphs4cfd_amd: a kernel's bf16 rows in the row-split order are put into feature order with
`ops.rs_rows_to_natural` by the caller before they are compared.

Where a launch rounds (derived from csrc/mlp_common.h `split3x4<1>` — one round-to-nearest-even `(__bf16)x` of an fp32 value — the
`SP == 1` branches of mlp_fused.hip / mlp_ws.hip / mlp_rs.hip, and ops.PackedMLP, whose rounded-bf16 stream is the leading plane of
`g4c_mlp_pack_layer`, i.e. bf16_rne(W)):

- Wide input blocks: bf16_rne(act(x)[idx]) times bf16_rne(W_block), the products accumulated (fp64 here, fp32 MFMA in the kernel).
- Narrow blocks (<= 8 columns, read without index or activation, the vector-ALU path): x times W in fp32 class — nothing rounded.
- Additive rows (hoisted products): used as given and added to the first layer's sum; bf16 rows are widened exactly.
- Bias: added to the sum in fp32 class, not rounded.
- Hidden layers: bf16_rne(SELU(h)) — the activation, then the one rounding to the next layer's operand.
- LayerNorm (after the last layer): fp64, eps 1e-5, then the output activation.
- Stored bf16 rows: bf16_rne(y), or bf16_rne(SELU(y)) for `rows_act` = SELU (G4C_DTYPE_BF16_SELU).
- Aggregate: the per-segment mean of the reference's own (un-rounded, un-activated) output rows; with blocks.AGGREGATE_BF16 that mean
  rounded to bf16.
- Hoisted products and heads: bf16_rne(W_blk) . bf16_rne(v); stored as bf16 when blocks.PRODUCTS_BF16: bf16_rne of that.

`assert_bf16_order_noise` bounds how far a kernel may land from this reference.  A correct kernel differs from it only by the order and
precision of its fp32 sums: a hidden pre-activation that ends one fp32 ulp away can round to the neighbouring bf16 — a one-ulp flip of a
hidden activation, which moves the outputs of that row by ~1e-3.  The bounds (`NOISE`) are a stated multiple of exactly that freedom,
measured on CPU by scripts/bf16_noise_bounds.py (this reference in fp64 against the same reference evaluated with fp32 sums in 32-k
steps, like the MFMA chain); its log is profiles/r07_bf16_noise_bounds.log."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn.functional as F

Tensor = torch.Tensor


# ------------------------------------------------------------------ rounding
def bf16_round(x: Tensor, mode: str = "rne") -> Tensor:
    """x rounded to bf16 through its fp32 value (the kernel rounds fp32 values), returned as float64.  `mode` "rne": round to nearest,
    ties to even (the kernel's `(__bf16)x`); "rtz": toward zero (negative controls only).  Finite inputs only."""
    u = x.to(torch.float32).contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    if mode == "rne":
        u = u + 0x7FFF + ((u >> 16) & 1)
    elif mode != "rtz":
        raise ValueError(mode)
    u = u & 0xFFFF0000
    u = torch.where(u >= 1 << 31, u - (1 << 32), u).to(torch.int32)
    return u.view(torch.float32).to(torch.float64)


def bf16_rne(x: Tensor) -> Tensor:
    return bf16_round(x, "rne")


# ------------------------------------------------------------------ launch description
@dataclass
class Block:
    """One weighted input block of the first layer, in concatenation order: rows `x` [n_x, w] (fp32 or bf16, feature order), read
    through `index` [n_rows] when given, with `pre_act` ("selu" or None) applied on load; `narrow` blocks take the fp32 path."""
    x: Tensor
    index: Optional[Tensor] = None
    pre_act: Optional[str] = None
    narrow: bool = False
    negate: bool = False


@dataclass
class Additive:
    """Rows [n_t, 128] (fp32 or bf16, feature order) added to the first layer's sum, gathered through `index` when given."""
    rows: Tensor
    index: Optional[Tensor] = None


class Arith:
    """How the reference adds (fp64 — the reference — or fp32 in 32-k steps, the MFMA chain: the noise derivation) and how it rounds
    weights (negative controls perturb it, the kernels never see it)."""

    def __init__(self, accum: str = "fp64", weight_round: str = "rne"):
        if accum not in ("fp64", "fp32"):
            raise ValueError(accum)
        self.accum, self.weight_round = accum, weight_round
        self.dt = torch.float64 if accum == "fp64" else torch.float32

    def w(self, W: Tensor) -> Tensor:
        return bf16_round(W, self.weight_round)

    def matmul(self, a: Tensor, W: Tensor) -> Tensor:
        """a [n, k] @ W[n_out, k].T: fp64, or fp32 sums of 32-k steps added in order (each step itself an fp32 dot product)."""
        if self.accum == "fp64":
            return a.double() @ W.double().T
        a, W = a.float(), W.float()
        acc = torch.zeros(a.size(0), W.size(0), dtype=torch.float32)
        for k0 in range(0, a.size(1), 32):
            acc = acc + a[:, k0:k0 + 32] @ W[:, k0:k0 + 32].T
        return acc

    def cast(self, t: Tensor) -> Tensor:
        return t.to(self.dt)


FP64 = Arith()


def _linears(w: Dict[str, Tensor], prefix: str) -> List[Tuple[Tensor, Optional[Tensor]]]:
    p = f"{prefix}." if prefix else ""
    out, i = [], 1
    while f"{p}MLP.linear_{i}.weight" in w:
        out.append((w[f"{p}MLP.linear_{i}.weight"].detach().cpu().double(), w.get(f"{p}MLP.linear_{i}.bias")))
        i += 1
    return [(W, None if b is None else b.detach().cpu().double()) for W, b in out]


def _ln(w: Dict[str, Tensor], prefix: str):
    p = f"{prefix}." if prefix else ""
    g = w.get(f"{p}MLP.layer_norm.weight")
    return None if g is None else (g.detach().cpu().double(), w[f"{p}MLP.layer_norm.bias"].detach().cpu().double())


def _act(y: Tensor, act: Optional[str]) -> Tensor:
    if act is None:
        return y
    if act == "selu":
        return F.selu(y)
    if act == "tanh":
        return torch.tanh(y)
    raise ValueError(act)


def _gather(t: Tensor, index: Optional[Tensor]) -> Tensor:
    t = t.detach().cpu()
    return t if index is None else t[index.detach().cpu().long()]


# ------------------------------------------------------------------ one launch
def mlp(w: Dict[str, Tensor], blocks: Sequence[Block], n_rows: int, *, additive: Sequence[Additive] = (), act: Optional[str] = None,
        prefix: str = "", first_cols: Optional[Tuple[int, int]] = None, ar: Arith = FP64, perturb=None) -> Tensor:
    """The fp32-class output rows (after LayerNorm and `act`) of one rounded-bf16 launch of the MLP whose weights are `w[prefix.MLP.*]`.
    The weighted blocks multiply columns [first_cols[0], first_cols[1]) of the first layer (default: all of them, in block order; a
    hoisted launch passes (0, 128) and its products as `additive`).  `perturb(W1) -> W1` (negative controls) edits the first layer."""
    lin, ln = _linears(w, prefix), _ln(w, prefix)
    W1, b1 = lin[0]
    c0, c1 = first_cols if first_cols is not None else (0, int(W1.size(1)))
    W1 = W1[:, c0:c1]
    if perturb is not None:
        W1 = perturb(W1)
    if sum(int(b.x.size(1)) for b in blocks) != int(W1.size(1)):
        raise ValueError("the blocks do not cover the first layer's columns")
    y, k = None, 0
    for b in blocks:
        wd = int(b.x.size(1))
        Wb = W1[:, k:k + wd] * (-1.0 if b.negate else 1.0)
        x = _gather(b.x, b.index).double()
        if b.narrow:
            if b.index is not None or b.pre_act is not None:
                raise ValueError("a narrow block is read without index or activation")
            part = ar.matmul(ar.cast(x), ar.cast(Wb.float().double()))      # (fp32 weights, fp32 values: not rounded)
        else:
            part = ar.matmul(bf16_rne(_act(x, b.pre_act)), ar.w(Wb))
        y = part if y is None else y + part
        k += wd
    if y is None:
        y = torch.zeros(n_rows, int(W1.size(0)), dtype=ar.dt)
    for a in additive:
        y = y + ar.cast(_gather(a.rows, a.index).double())
    if b1 is not None:
        y = y + ar.cast(b1.float().double())
    for W, b in lin[1:]:
        h = bf16_rne(F.selu(y))
        y = ar.matmul(h, ar.w(W)) + (0 if b is None else ar.cast(b.float().double()))
    if ln is not None:
        y = F.layer_norm(y, (int(y.size(1)),), ar.cast(ln[0].float().double()), ar.cast(ln[1].float().double()), 1e-5)
    return _act(y, act).double()


def products(W_blk: Tensor, v: Tensor, *, bf16_out: bool = True, ar: Arith = FP64) -> Tensor:
    """A hoisted first-layer product / a head: bf16_rne(W_blk) . bf16_rne(v) per row of v [n, k] (W_blk [128, k]), stored as bf16
    (`bf16_out`, blocks.PRODUCTS_BF16) or fp32."""
    p = ar.matmul(bf16_rne(v.detach().cpu().double()), ar.w(W_blk.detach().cpu().double())).double()
    return bf16_rne(p) if bf16_out else p


def stored_rows(y: Tensor, fmt: str) -> Tensor:
    """What a launch stores of its fp32-class output rows `y`: "fp32", "bf16" (bf16_rne(y)) or "bf16_selu" (bf16_rne(SELU(y)))."""
    if fmt == "fp32":
        return y
    if fmt == "bf16":
        return bf16_rne(y)
    if fmt == "bf16_selu":
        return bf16_rne(F.selu(y))
    raise ValueError(fmt)


def segment_mean(y: Tensor, off: Tensor, *, bf16_out: bool = False) -> Tensor:
    """Per segment [off[s], off[s + 1]) of the rows (in segment order) the mean of `y` (empty segments: 0); bf16_rne of it with
    `bf16_out` (blocks.AGGREGATE_BF16)."""
    off = off.detach().cpu().long()
    n_seg = int(off.numel()) - 1
    cnt = (off[1:] - off[:-1])
    seg = torch.repeat_interleave(torch.arange(n_seg), cnt)
    s = torch.zeros(n_seg, int(y.size(1)), dtype=torch.float64).index_add_(0, seg, y.double()[: int(off[-1])])
    m = s / cnt.clamp(min=1).double()[:, None]
    return bf16_rne(m) if bf16_out else m


# ------------------------------------------------------------------ the checker
# Bounds of |kernel - reference| per kind of output, each a stated multiple of the CPU-measured freedom of a correct kernel
# (scripts/bf16_noise_bounds.py, profiles/r07_bf16_noise_bounds.log: the worst case over its launch shapes of fp32-in-32-k-steps vs fp64):
#   mean  <= MEAN_X x measured mean + FLIP_ROWS x measured max / rows   (the second term: a launch of few rows, where one flipped row
#            alone moves the mean);
#   fraction of elements above `thr` <= FRAC_X x measured fraction + FRAC_FLOOR + 2 elements (a launch of few rows);
#   max   <= MAX_X x measured max;   per row, elements above half the max limit: <= `row_count` (a misplaced row deviates in ~all 128
#            columns; a correct kernel has at most a few elements that far out in any row — the max check alone would let a whole row sit
#            just under it).
# The CPU derivation does not model all of a kernel's freedom: the kernels' SELU takes its exp from the approximate v_exp_f32
# (g4c::selu_f, mlp_common.h selu4), which moves more hidden pre-activations across a bf16 rounding boundary than torch's fp32 SELU,
# and their LayerNorm / MFMA sums have orders of their own.  On an MI355X they land at up to 3.6x the CPU mean and 1.7x its max (every
# launch of tests/test_gpu_bf16.py, profiles/r07_bf16_kernel_noise.log).  MEAN_X and MAX_X were set with that measurement in view: 2x
# on top of it.  They stay orders of magnitude below what the negative controls produce (weights rounded toward zero: mean 3e-3; a
# swapped column pair: 8e-2; a row counted in the wrong segment: ~100 deviating elements in one row).  The FLIP_ROWS term makes the
# mean bound of a launch of a few dozen rows loose (~3e-4): a small uniform bias is caught by the launches of thousands of rows that
# every test of the file also makes, not by its smallest ones.
# "rows32": fp32 output rows; "rows16": bf16 (or bf16(SELU)) rows — one rounding more; "agg32" / "agg16": segment means;
# "prod16": hoisted products / heads stored as bf16.
MEAN_X, FRAC_X, MAX_X, FRAC_FLOOR, FLIP_ROWS = 8.0, 4.0, 3.0, 1e-5, 2.0
NOISE = {
    # kind: (measured mean, thr, measured fraction above thr, measured max, row_thr (None: half the max limit), row_count) — the "worst case per kind" lines of
    # profiles/r07_bf16_noise_bounds.log (test_bf16_ref.py checks that the two agree)
    "rows32": (1.82e-06, 1e-2, 0.0, 7.42e-03, None, 4),
    "rows16": (1.35e-06, 1e-2, 3.91e-06, 1.56e-02, None, 4),
    "agg32": (1.28e-06, 1e-2, 0.0, 1.74e-03, None, 4),
    "agg16": (1.32e-06, 1e-2, 1.63e-06, 1.56e-02, None, 4),
    "prod16": (6.04e-07, 1e-2, 0.0, 7.81e-03, None, 4),
}


def row_threshold(kind: str) -> float:
    """The per-row count's threshold: half the max limit of that kind of output."""
    return 0.5 * MAX_X * NOISE[kind][3]


def noise_stats(got: Tensor, ref: Tensor, thr: float, row_thr: float) -> Dict[str, float]:
    d = (got.detach().cpu().double() - ref.detach().cpu().double()).abs()
    if not torch.isfinite(got.detach().cpu().double()).all():
        return {"mean": float("inf"), "frac": 1.0, "max": float("inf"), "row_count": int(d.size(-1)), "n": int(d.numel())}
    return {"mean": d.mean().item() if d.numel() else 0.0, "frac": (d > thr).double().mean().item() if d.numel() else 0.0,
            "max": d.max().item() if d.numel() else 0.0, "row_count": int((d > row_thr).sum(1).max().item()) if d.numel() else 0,
            "n": int(d.numel())}


def check_bf16_order_noise(got: Tensor, ref: Tensor, kind: str) -> Tuple[bool, Dict[str, float], Dict[str, float]]:
    """(ok, stats, limits) of kernel output `got` (feature order) against the reference `ref` for one kind of output (NOISE)."""
    if tuple(got.shape) != tuple(ref.shape):
        raise ValueError(f"shapes {tuple(got.shape)} / {tuple(ref.shape)}")
    m, thr, f, mx, _, rc = NOISE[kind]
    s = noise_stats(got, ref, thr, row_threshold(kind))
    lim = {"mean": MEAN_X * m + FLIP_ROWS * mx / max(int(got.size(0)), 1), "frac": FRAC_X * f + FRAC_FLOOR + 2.0 / max(s["n"], 1), "max": MAX_X * mx,
           "row_count": rc}
    ok = all(s[k] <= lim[k] for k in lim)
    return ok, s, lim


def assert_bf16_order_noise(got: Tensor, ref: Tensor, kind: str, what: str = "") -> Dict[str, float]:
    ok, s, lim = check_bf16_order_noise(got, ref, kind)
    assert ok, f"{what} [{kind}]: {s} against limits {lim}"
    return s


# ------------------------------------------------------------------ perturbations of the reference (negative controls)
def swap_adjacent_columns(W: Tensor, col: int = 37) -> Tensor:
    """Two adjacent input columns of one 32-feature step exchanged (`col` and `col + 1`, inside one step)."""
    if col % 32 == 31:
        raise ValueError("the pair must lie in one 32-feature step")
    W = W.clone()
    W[:, [col, col + 1]] = W[:, [col + 1, col]]
    return W


def move_row_to_next_segment(off: Tensor, seg: int) -> Tensor:
    """Segment offsets with the last row of segment `seg` counted in segment `seg + 1` instead."""
    off = off.detach().cpu().clone()
    off[seg + 1] -= 1
    return off
