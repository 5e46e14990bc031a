"""bf16 saved activations, the parts that need no device: the `ops.set_train_precision(..., saved=)` switch and its getter,
`TrainConfig(saved_activations=)`, the argument checks of the three new entry points (made before any HIP call), and the helpers of
tests/saved_ref.py."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import saved_ref as SR                        # noqa: E402
import graphs4cfd_amd as gfd                  # noqa: E402
from graphs4cfd_amd import _lib, ops          # noqa: E402
from oracle.bf16_ref import bf16_rne          # noqa: E402


def test_saved_precision_switch():
    assert ops.train_precision() == "bf16x6" and ops.saved_precision() == "fp32"          # the defaults
    # every existing form of the call selects fp32 rows
    assert ops.set_train_precision("bf16") == "bf16x6" and ops.saved_precision() == "fp32"
    assert ops.set_train_precision("bf16", saved=None) == "bf16" and ops.saved_precision() == "fp32"
    assert ops.set_train_precision("bf16", saved="bf16") == "bf16"          # still the previous PRECISION string
    assert (ops.train_precision(), ops.saved_precision()) == ("bf16", "bf16")
    assert ops.set_train_precision("bf16", "fp32") == "bf16" and ops.saved_precision() == "fp32"
    ops.set_train_precision("bf16", saved="bf16")
    assert ops.set_train_precision("bf16x6") == "bf16"                       # a plain call drops back to fp32 rows
    assert (ops.train_precision(), ops.saved_precision()) == ("bf16x6", "fp32")
    # bf16 rows only with the bf16 backward; unknown names; nothing changes on an error
    for prec, saved in (("bf16x6", "bf16"), ("bf16", "fp16"), ("bf16", "BF16"), ("bf16", ""), ("f16x3", "bf16")):
        with pytest.raises(ValueError):
            ops.set_train_precision(prec, saved=saved)
        assert (ops.train_precision(), ops.saved_precision()) == ("bf16x6", "fp32")
    with SR.train_mode(saved="bf16", forward=False):
        assert (ops.train_precision(), ops.saved_precision()) == ("bf16", "bf16")
    assert (ops.train_precision(), ops.saved_precision()) == ("bf16x6", "fp32")


def test_train_config_saved_activations():
    assert gfd.nn.TrainConfig(name="a")["saved_activations"] == "fp32"
    assert gfd.nn.TrainConfig(name="a", mixed_precision=True)["saved_activations"] == "fp32"
    cfg = gfd.nn.TrainConfig(name="a", mixed_precision=True, saved_activations="bf16")
    assert cfg["saved_activations"] == "bf16" and cfg["mixed_precision"] is True
    with pytest.raises(ValueError, match="mixed_precision"):
        gfd.nn.TrainConfig(name="a", saved_activations="bf16")
    with pytest.raises(ValueError, match="saved_activations"):
        gfd.nn.TrainConfig(name="a", mixed_precision=True, saved_activations="fp16")


def _aligned(n_floats: int):
    """A host buffer and a 16-byte aligned address inside it (never dereferenced: every call below fails its argument checks)."""
    buf = (C.c_float * (n_floats + 8))()
    return buf, (C.addressof(buf) + 15) & ~15


def test_weight_grad_bf16_a16_validates_before_any_hip_call():
    lib = _lib.load()
    keep, p = _aligned(64)

    def call(g, g_ld, a, a_ld, rows):
        return lib.g4c_weight_grad_bf16_a16(g, g_ld, a, a_ld, rows, p, p, 1, None), lib.g4c_last_error().decode()

    rc, msg = call(p, 128, p + 8, 128, 8)                 # a: a bf16 window 4 elements into a row is 8 bytes off
    assert rc == _lib.EINVAL and "g4c_weight_grad_bf16_a16" in msg and "16-byte aligned" in msg
    rc, msg = call(p + 4, 128, p, 128, 8)
    assert rc == _lib.EINVAL and "16-byte aligned" in msg
    rc, msg = call(p, 128, p, 130, 8)                     # ld % 4 != 0
    assert rc == _lib.EINVAL and "multiples of 4" in msg and "a_ld=130" in msg
    rc, msg = call(p, 128, p, 124, 8)
    assert rc == _lib.EINVAL and "a_ld=124" in msg
    rc, msg = call(p, 128, p, 128, -1)
    assert rc == _lib.EINVAL and "n_rows -1" in msg
    rc, msg = call(p, 128, None, 128, 8)
    assert rc == _lib.EINVAL and "null pointer" in msg
    del keep


def test_adjoint_entry_points_validate_before_any_hip_call():
    lib = _lib.load()
    keep, p = _aligned(64)
    rc = lib.g4c_act_grad_ref16(p, 128, p, 60, 0, _lib.ACT_SELU, p, 128, 128, 4, None)          # ref_ld below the width
    assert rc == _lib.EINVAL and "g4c_act_grad_ref16" in lib.g4c_last_error().decode()
    rc = lib.g4c_act_grad_ref16(p, 128, p, 128, 0, 5, p, 128, 128, 4, None)                     # unknown activation
    assert rc == _lib.EINVAL and "act=5" in lib.g4c_last_error().decode()
    rc = lib.g4c_act_grad_ref16(p, 128, p + 1, 128, 0, _lib.ACT_SELU, p, 128, 128, 4, None)     # an odd address holds no bf16
    assert rc == _lib.EINVAL and "bf16 pointer" in lib.g4c_last_error().decode()
    rc = lib.g4c_act_grad_ref16(p, 128, None, 128, 0, _lib.ACT_SELU, p, 128, 128, 4, None)
    assert rc == _lib.EINVAL and "null pointer" in lib.g4c_last_error().decode()
    rc = lib.g4c_layernorm_grad_z16(p, 128, p, p, 128, p, 128, p, 300, 4, 1e-5, None)           # wider than a wave covers
    assert rc == _lib.EUNSUPPORTED and "g4c_layernorm_grad_z16" in lib.g4c_last_error().decode()
    rc = lib.g4c_layernorm_grad_z16(p, 60, p, p, 128, p, 128, p, 128, 4, 1e-5, None)            # z_ld below the width
    assert rc == _lib.EUNSUPPORTED
    rc = lib.g4c_layernorm_grad_z16(p, 128, None, p, 128, p, 128, p, 128, 4, 1e-5, None)
    assert rc == _lib.EINVAL and "null pointer" in lib.g4c_last_error().decode()
    for name in ("g4c_weight_grad_bf16_a16", "g4c_act_grad_ref16", "g4c_layernorm_grad_z16"):
        assert name in _lib.EXPORTED_SYMBOLS
    del keep


def test_io_descriptor_carries_the_two_dtypes():
    io = _lib.g4c_mlp_io_t()
    assert (io.save_dtype, io.mul_dtype) == (_lib.DTYPE_F32, _lib.DTYPE_F32) and io.size == C.sizeof(_lib.g4c_mlp_io_t)
    assert (_lib.DTYPE_F32, _lib.DTYPE_BF16) == (0, 1)


def test_rne_bits_is_round_to_nearest_even():
    """By hand on the cases that tell the roundings apart, then against two independent conversions on random values."""
    def f(bits32):
        return torch.tensor([bits32], dtype=torch.int64).to(torch.int32).view(torch.float32) if bits32 < 2 ** 31 else \
            torch.tensor([bits32 - 2 ** 32], dtype=torch.int64).to(torch.int32).view(torch.float32)

    def up(x):
        return int(SR.rne_bits(x)[0]) & 0xFFFF
    assert up(f(0x3F800000)) == 0x3F80                    # 1.0
    assert up(f(0x3F808000)) == 0x3F80                    # a tie, even below: stays
    assert up(f(0x3F818000)) == 0x3F82                    # a tie, odd below: up to even
    assert up(f(0x3F808001)) == 0x3F81                    # just above the tie
    assert up(f(0x3F807FFF)) == 0x3F80                    # just below (truncation and rounding agree)
    assert up(f(0xBF818000)) == 0xBF82                    # sign carried
    assert up(f(0x00000001)) == 0x0000 and up(f(0x0000C000)) == 0x0001          # fp32 subnormals
    assert up(f(0x7F7FFFFF)) == 0x7F80                    # the largest finite value rounds to infinity, as the hardware does
    x = torch.randn(4096, generator=torch.Generator().manual_seed(3)) * torch.logspace(-30, 30, 4096)
    assert torch.equal(SR.rne_bits(x), SR.bits(x.bfloat16()))
    assert torch.equal(SR.widen(x.bfloat16()).double(), bf16_rne(x))
    assert torch.equal(SR.widen(x.bfloat16()), x.bfloat16().float())


def test_expected_drop_counts_the_allocator_rounding():
    seen = SR.Launches()
    seen.saving = [(3000, torch.bfloat16, 3), (1, torch.bfloat16, 2), (17875, torch.bfloat16, 3)]
    # 3000 rows: 1 536 000 - 768 000;  1 row: 512 - 512 (a 256-byte tensor still takes a 512-byte block);  17875 rows: 9 152 000 - roundup(4 576 000, 512) = 9 152 000 - 4 576 256
    assert seen.expected_drop() == 3 * 768000 + 0 + 3 * 4575744 and seen.tensors() == 8
    seen.saving = [(33, torch.bfloat16, 1)]               # 16896 - roundup(8448, 512) = 16896 - 8704
    assert seen.expected_drop() == 8192
