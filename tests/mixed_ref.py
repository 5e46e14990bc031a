"""Test-only fp64 references of mixed-precision training (`ops.set_train_precision("bf16")`): every matrix product of the backward
takes BOTH operands rounded once to bf16, round to nearest even (`oracle.bf16_ref.bf16_rne`), and is accumulated in fp32 by the
kernels, in fp64 here.  Bias gradients come from the unrounded rows.  The checkers are those of `oracle.grad_ref`
(`assert_exact`, `assert_fp32_class`, C = 2); this module adds only the rounded references and the n_eff of the new kernel.

Not a test module (no `test_` prefix): tests/test_train_mixed_host.py checks these helpers against their own negative controls on the
CPU, tests/test_gpu_train_mixed.py compares the kernels with them."""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

from oracle import grad_ref as R
from oracle.bf16_ref import bf16_rne

Tensor = torch.Tensor
F64 = torch.float64


def rne(x: Tensor) -> Tensor:
    """x rounded to bf16 (nearest, ties to even) as fp64, on x's device (`bf16_rne` views the fp32 bits: any device)."""
    return bf16_rne(x.detach())


# ------------------------------------------------------------------ g4c_weight_grad_bf16
def weight_bias_grad(g: Tensor, a: Tensor) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """(dW = rne(g)^T rne(a), db = column sums of the UNROUNDED g, |rne g|^T |rne a|, column sums of |g|)."""
    gr, ar = rne(g), rne(a)
    g64 = g.detach().to(F64)
    return gr.t() @ ar, g64.sum(0), gr.abs().t() @ ar.abs(), g64.abs().sum(0)


def weight_bias_grad_unrounded(g: Tensor, a: Tensor) -> Tuple[Tensor, Tensor]:
    """What a kernel that skipped the rounding would compute (negative control): (g^T a, |g|^T |a|) in fp64."""
    g64, a64 = g.detach().to(F64), a.detach().to(F64)
    return g64.t() @ a64, g64.abs().t() @ a64.abs()


MFMA_ROWS = 16        # rows contracted by one v_mfma_f32_32x32x16_bf16
SLAB = 64             # rows staged per slab by weight_grad_bf16_kernel (four MFMA steps)


def weight_grad_chunk(rows: int) -> int:
    """Rows per workgroup: the partial rule of g4c_weight_grad (grad_ref.weight_grad_partials, whole 32-row units)."""
    G = R.weight_grad_partials(rows)
    return -(-(-(-rows // 32)) // G) * 32


def n_eff_weight_grad(rows: int) -> int:
    """weight_grad_bf16_kernel, longest chain of fp32 roundings behind one element of dW / db:
    - dW: the products of two bf16 values are exact in fp32; one MFMA adds 16 of them to the accumulator (counted as 16 roundings,
      whatever the order inside the instruction), and a workgroup's chunk is ceil(chunk / 16) such steps on ONE accumulator;
    - db: a thread adds its 4 rows of every 64-row slab in order (chunk / 16 additions), then 16 threads' sums are added in order;
    - then, for both, the two colsum stages over the partial tiles (16 partials per first-stage workgroup, then ceil(G / 16)), as
      grad_ref.n_eff_weight_grad counts them."""
    G = R.weight_grad_partials(rows)
    g2 = -(-G // 16)
    stages = R.n_eff_colsum_stage(G, -(-G // g2), 4096) + R.n_eff_colsum_stage(g2, g2, 4096)
    return math.ceil(weight_grad_chunk(rows) / MFMA_ROWS) + 16 + stages


# ------------------------------------------------------------------ the launches of the fused kernel on the rounded-bf16 stream
N_EFF_LAYER = R.N_EFF_LAYER_K        # one 128-k layer: an fp32 MFMA accumulator over 128 k per output (no split term: ONE product)


def linear(x: Tensor, W: Tensor, b: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """(rne(x) rne(W)^T + b, |rne x| |rne W|^T + |b|) — autograd.linear in the mode (the bias is added in fp32, not rounded)."""
    xr, Wr = rne(x), rne(W)
    y, ya = xr @ Wr.t(), xr.abs() @ Wr.abs().t()
    if b is not None:
        y, ya = y + b.detach().to(F64), ya + b.detach().to(F64).abs()
    return y, ya


def chain_layer(d_next: Tensor, W: Tensor, act: Tensor) -> Tuple[Tensor, Tensor]:
    """One hidden layer of backward_chain in the mode: D[l] = (rne(D[l+1]) rne(W[l])) * selu'(a[l]), D[l+1] the rows the launch
    itself saved (its next layer reads exactly their bf16 rounding), the slope from the fp32 activations (grad_ref.selu_slope_out)."""
    dr, Wr = rne(d_next), rne(W)
    s = R.selu_slope_out(act)
    return (dr @ Wr) * s, (dr.abs() @ Wr.abs()) * s.abs()
