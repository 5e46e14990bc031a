"""Mixed-precision training, the parts that need no device: g4c_weight_grad_bf16 validates its arguments before any HIP call, the
`ops.set_train_precision` switch, and the references of tests/mixed_ref.py against their own negative controls."""
import ctypes as C
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mixed_ref as MR                        # noqa: E402
from graphs4cfd_amd import _lib, ops          # noqa: E402
from oracle import grad_ref as R              # noqa: E402
from oracle.bf16_ref import bf16_rne          # noqa: E402


def _aligned(n_floats: int):
    """A host buffer and a 16-byte aligned address inside it (never dereferenced: every call below fails its argument checks)."""
    buf = (C.c_float * (n_floats + 8))()
    addr = (C.addressof(buf) + 15) & ~15
    return buf, addr


def test_weight_grad_bf16_validates_before_any_hip_call():
    lib = _lib.load()
    keep, p = _aligned(64)

    def call(g, g_ld, a, a_ld, rows):
        return lib.g4c_weight_grad_bf16(g, g_ld, a, a_ld, rows, p, p, 1, None), lib.g4c_last_error().decode()

    rc, msg = call(p + 4, 128, p, 128, 8)                 # g four bytes off a 16-byte boundary
    assert rc == _lib.EINVAL and "g4c_weight_grad_bf16" in msg and "16-byte aligned" in msg
    rc, msg = call(p, 128, p + 8, 128, 8)                 # a eight bytes off
    assert rc == _lib.EINVAL and "16-byte aligned" in msg
    rc, msg = call(p, 130, p, 128, 8)                     # ld % 4 != 0
    assert rc == _lib.EINVAL and "multiples of 4" in msg and "g_ld=130" in msg
    rc, msg = call(p, 128, p, 134, 8)
    assert rc == _lib.EINVAL and "a_ld=134" in msg
    rc, msg = call(p, 124, p, 128, 8)                     # narrower than the 128-wide tile
    assert rc == _lib.EINVAL and "g_ld=124" in msg
    rc, msg = call(p, 128, p, 128, -1)
    assert rc == _lib.EINVAL and "n_rows -1" in msg
    rc, msg = call(None, 128, p, 128, 8)
    assert rc == _lib.EINVAL and "null pointer" in msg
    assert "g4c_weight_grad_bf16" in _lib.EXPORTED_SYMBOLS
    del keep


def test_train_precision_round_trip():
    assert ops.train_precision() == "bf16x6"              # the default: today's backward, bit for bit
    mlp = ops.mlp_precision()
    assert ops.set_train_precision("bf16") == "bf16x6" and ops.train_precision() == "bf16"
    assert ops.mlp_precision() == mlp                     # independent of the forward's switch
    assert ops.set_mlp_precision("bf16x6") == mlp and ops.train_precision() == "bf16"
    ops.set_mlp_precision(mlp)
    assert ops.set_train_precision("bf16x6") == "bf16" and ops.train_precision() == "bf16x6"
    for bad in ("fp32", "f16x3", "BF16", "", None):
        with pytest.raises(ValueError):
            ops.set_train_precision(bad)
        assert ops.train_precision() == "bf16x6"


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def test_rounded_weight_grad_reference_and_its_negative_controls():
    """Integer operands (exact in bf16): the rounded reference equals the plain one and rejects a dropped row and a zeroed last row of
    a partial tile.  Random operands: the reference is the product of the rounded values (element checked by hand), an fp32 evaluation
    of it passes the bounded check with the kernel's n_eff, and the UNROUNDED product, a truncated one, a dropped row and a zeroed
    last row are all rejected by it."""
    g = _gen(1)
    M = 581
    gi, ai = R.int_operand((M, 128), R.vmax_for(M), g), R.int_operand((M, 128), R.vmax_for(M), g)
    dW, db, aW, ab = MR.weight_bias_grad(gi, ai)
    R.check_int_bound(aW, ab)
    R.assert_exact(dW.float(), R.weight_bias_grad(gi, ai)[0])
    R.assert_exact(db.float(), gi.double().sum(0))
    r = int(torch.nonzero((gi.abs().sum(1) * ai.abs().sum(1)) > 0)[M // 2])
    assert R.rejects(R.assert_exact, dW.float(), MR.weight_bias_grad(gi, R.drop_row(ai, r))[0])
    assert R.rejects(R.assert_exact, db.float(), MR.weight_bias_grad(R.drop_row(gi, r), ai)[1])
    assert R.rejects(R.assert_exact, dW.float(), MR.weight_bias_grad(gi, R.zero_last_partial_row(ai))[0])

    gr, ar = torch.randn(M, 128, generator=g), torch.randn(M, 128, generator=g)
    dW, db, aW, ab = MR.weight_bias_grad(gr, ar)
    want = sum(float(bf16_rne(gr[m, 5])) * float(bf16_rne(ar[m, 7])) for m in range(M))
    assert abs(float(dW[5, 7]) - want) <= 1e-12 * float(aW[5, 7])
    assert torch.equal(db, gr.double().sum(0))            # the bias gradient sees the unrounded rows
    n_eff = MR.n_eff_weight_grad(M)
    assert MR.weight_grad_chunk(M) == 224 and R.weight_grad_partials(M) == 3           # 19 units of 32 rows over 3 workgroups
    assert n_eff == 224 // 16 + 16 + (1 + 3 + 1) + (1 + 3 + 1)          # 14 MFMA steps, 16 in order, two short colsum stages
    got = (bf16_rne(gr).float().t() @ bf16_rne(ar).float())             # fp32 sums of the exact products, some order
    R.assert_fp32_class(got, dW, aW, n_eff, "fp32 evaluation of the rounded product")
    plain, plain_abs = MR.weight_bias_grad_unrounded(gr, ar)
    assert R.rejects(R.assert_fp32_class, got, plain, plain_abs, n_eff)                      # a kernel that skipped the rounding
    from oracle.bf16_ref import bf16_round
    trunc = bf16_round(gr, "rtz").t() @ bf16_round(ar, "rtz")
    assert R.rejects(R.assert_fp32_class, got, trunc, aW, n_eff)                             # ... or truncated
    for bad in (MR.weight_bias_grad(gr, R.drop_row(ar, 300)), MR.weight_bias_grad(gr, R.zero_last_partial_row(ar))):
        assert R.rejects(R.assert_fp32_class, got, bad[0], bad[2], n_eff)
    bad = MR.weight_bias_grad(R.drop_row(gr, 300), ar)
    assert R.rejects(R.assert_fp32_class, db.float(), bad[1], bad[3], n_eff)


def test_rounded_chain_and_linear_references_reject_swapped_columns():
    g = _gen(2)
    M = 33
    d, W = torch.randn(M, 128, generator=g), torch.randn(128, 128, generator=g) / 11
    act = torch.nn.functional.selu(torch.randn(M, 128, generator=g))
    ref, absr = MR.chain_layer(d, W, act)
    got = ((bf16_rne(d).float() @ bf16_rne(W).float()).double() * R.selu_slope_out(act)).float()
    R.assert_fp32_class(got, ref, absr, MR.N_EFF_LAYER, "chain layer")
    bad = MR.chain_layer(d, R.swap_columns(W.t(), 40).t(), act)                              # two k of the contraction swapped
    assert R.rejects(R.assert_fp32_class, got, bad[0], bad[1], MR.N_EFF_LAYER)
    plain = R.chain_layer(d, W, act)                                                         # the unrounded chain layer
    assert R.rejects(R.assert_fp32_class, got, plain[0], plain[1], MR.N_EFF_LAYER)
    b = torch.randn(128, generator=g)
    ref, absr = MR.linear(d, W, b)
    got = (bf16_rne(d).float() @ bf16_rne(W).float().t() + b).float()
    R.assert_fp32_class(got, ref, absr, MR.N_EFF_LAYER + 1, "linear")
    bad = MR.linear(d, R.swap_columns(W, 40), b)
    assert R.rejects(R.assert_fp32_class, got, bad[0], bad[1], MR.N_EFF_LAYER + 1)
    bad = MR.linear(R.zero_last_partial_row(d), W, b)
    assert R.rejects(R.assert_fp32_class, got, bad[0], bad[1], MR.N_EFF_LAYER + 1)
