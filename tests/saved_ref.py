"""Test-only helpers of the bf16 saved-activation precision (`ops.set_train_precision("bf16", saved="bf16")`).

The mode's definition is exact: every row a recorded forward keeps is `bf16(round-to-nearest-even(fp32 row))`, and every consumer
widens it exactly.  So a step in the mode equals, bit for bit, today's mixed step with its kept rows replaced by their roundings —
`rounding_forward` makes that step: a wrapper around `ops.mlp_forward` that rounds the fp32 save tensors in place after every
launch that saves (and is not the backward chain).  `rne_bits` is the rounding itself on the integer view, independent of torch's
own conversion.

Not a test module (no `test_` prefix): tests/test_saved_bf16_host.py checks these helpers on the CPU,
tests/test_gpu_train_saved_bf16.py uses them on the device."""
from __future__ import annotations

import contextlib
from typing import List, Tuple

import torch

from graphs4cfd_amd import ops

Tensor = torch.Tensor
SENTINEL = -776.0          # 97 * 8: exact in bf16 and fp32; no kernel under test produces it from the operands used


def rne_bits(x: Tensor) -> Tensor:
    """The 16 bits of bf16(x), round to nearest, ties to even, of a finite fp32 tensor, as int16 — by integer arithmetic on the
    bit pattern: add 0x7fff + (bit 16), keep the upper half."""
    assert x.dtype == torch.float32
    u = x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    r = r & 0xFFFF
    return torch.where(r >= 0x8000, r - 0x10000, r).to(torch.int16)


def bits(x16: Tensor) -> Tensor:
    """The int16 view of a bf16 tensor (contiguous copy)."""
    assert x16.dtype == torch.bfloat16
    return x16.contiguous().view(torch.int16)


def widen(x16: Tensor) -> Tensor:
    """bf16 -> fp32, exact (the bits moved up by 16)."""
    return (bits(x16).to(torch.int32) << 16).view(torch.float32)


@contextlib.contextmanager
def train_mode(saved=None, forward: bool = True):
    """Mixed-precision training as `fit` selects it (both switches), with the given saved-activation precision."""
    old_saved = ops.saved_precision()
    old_t = ops.set_train_precision("bf16", saved=saved)
    old_m = ops.set_mlp_precision("bf16") if forward else None
    try:
        yield
    finally:
        ops.set_train_precision(old_t, saved=old_saved)
        if forward:
            ops.set_mlp_precision(old_m)


class Launches:
    """What `rounding_forward` / `counting_forward` saw: one (rows, dtype, tensors kept) per saving launch (`save` without `mul`)."""

    def __init__(self):
        self.saving: List[Tuple[int, torch.dtype, int]] = []

    def expected_drop(self) -> int:
        """Bytes the bf16 mode frees between the passes, with the allocator's 512-byte rounding: per kept [rows, 128] tensor
        rows * 512 (fp32, already a multiple of 512) - roundup(rows * 256, 512)."""
        return sum(n * (rows * 512 - -(-rows * 256 // 512) * 512) for rows, _, n in self.saving)

    def tensors(self) -> int:
        return sum(n for _, _, n in self.saving)


def _wrap(monkeypatch, round_in_place: bool) -> Launches:
    seen, f0 = Launches(), ops.mlp_forward

    def fwd(*a, **k):
        y = f0(*a, **k)
        save = k.get("save")
        if save is not None and k.get("mul") is None:
            live = [t for t in save if t is not None]
            if live:
                n_rows = int(a[2]) if len(a) > 2 else int(k["n_rows"])
                seen.saving.append((n_rows, live[0].dtype, len(live)))
            if round_in_place:
                for t in live:
                    assert t.dtype == torch.float32
                    t.copy_(t.bfloat16().float())
        return y
    monkeypatch.setattr(ops, "mlp_forward", fwd)
    return seen


def rounding_forward(monkeypatch) -> Launches:
    """ops.mlp_forward with the kept fp32 rows rounded to bf16 (and widened again) in place after every saving launch."""
    return _wrap(monkeypatch, True)


def counting_forward(monkeypatch) -> Launches:
    """ops.mlp_forward unchanged, the saving launches recorded."""
    return _wrap(monkeypatch, False)
