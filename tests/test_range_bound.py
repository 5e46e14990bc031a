"""The pack-time fp16 range proof (ops.weight_norms / ops.range_bounds / ops.certifies): host arithmetic only, no device, no library.

A launch in the f16x3 arithmetic may drop its range tracker when its caller certifies that nothing it converts to fp16 can reach
65504.  The certificate comes from a bound computed from the weights' norms and the bounds of the launch's inputs; these tests
evaluate every converted activation in fp64 — random and adversarial weights, LayerNorm gains / offsets and biases of both signs,
inputs drawn up to (and placed exactly at) the certified input bound — and require it to stay at or below the bound, and they
check that the certificate is refused whenever a part of the proof is missing."""
import math
import types

import pytest
import torch

from graphs4cfd_amd import _lib, ops
from graphs4cfd_amd.ops import Source

NONE, SELU, TANH = _lib.ACT_NONE, _lib.ACT_SELU, _lib.ACT_TANH
F64 = torch.float64


def selu64(x):
    return torch.nn.functional.selu(x.to(F64))


def act64(x, act):
    return selu64(x) if act == SELU else (torch.tanh(x) if act == TANH else x)


def make_mlp(gen, widths, n_layers, ln, heads, scale=1.0, adversarial=False, n_out=128):
    """fp32 parameters of an MLP over input blocks `widths`: weights, biases (both signs), LayerNorm (gamma, beta, eps), heads."""
    k = sum(widths)
    outs = [128] * (n_layers - 1) + [n_out]
    weights, biases = [], []
    for l, o in enumerate(outs):
        kin = k if l == 0 else outs[l - 1]
        W = torch.randn(o, kin, generator=gen) * (scale / math.sqrt(kin))
        if adversarial:          # one sign per row: an input of constant sign lines every product up
            W = W.abs() * torch.where(torch.rand(o, 1, generator=gen) < 0.5, -1.0, 1.0)
        weights.append(W.float())
        biases.append(((torch.rand(o, generator=gen) - 0.5) * 2 * scale).float())
    lnp = None
    if ln:
        lnp = (((torch.rand(n_out, generator=gen) - 0.5) * 4).float(), ((torch.rand(n_out, generator=gen) - 0.5) * 2).float(), 1e-5)
    hs = [(torch.randn(128, 128, generator=gen) / math.sqrt(128)).float() for _ in range(heads)]
    return weights, biases, lnp, hs


def draw(gen, rows, width, bound, mode):
    """Rows with |x| <= bound: uniform, at the corners +-bound, all +bound, all -bound, or a single spike (LayerNorm's worst case)."""
    if mode == "uniform":
        return (torch.rand(rows, width, generator=gen, dtype=F64) * 2 - 1) * bound
    if mode == "corners":
        return torch.where(torch.rand(rows, width, generator=gen) < 0.5, -1.0, 1.0).to(F64) * bound
    if mode == "plus":
        return torch.full((rows, width), bound, dtype=F64)
    if mode == "minus":
        return torch.full((rows, width), -bound, dtype=F64)
    x = torch.zeros(rows, width, dtype=F64)
    x[torch.arange(rows), torch.randint(0, width, (rows,), generator=gen)] = bound
    return x


def evaluate(weights, biases, lnp, hs, blocks, adds, act):
    """fp64 forward of the fused launch; returns (max |value converted to fp16|, max |output|, [max |head row|])."""
    x = torch.cat(blocks, 1)
    conv = float(x.abs().max())
    z = x @ weights[0].to(F64).T + biases[0].to(F64)
    for a in adds:
        z = z + a
    for l in range(1, len(weights)):
        h = selu64(z)
        conv = max(conv, float(h.abs().max()))
        z = h @ weights[l].to(F64).T + biases[l].to(F64)
    if lnp is not None:
        g, b, eps = lnp
        mu = z.mean(1, keepdim=True)
        var = ((z - mu) ** 2).mean(1, keepdim=True)
        z = (z - mu) / torch.sqrt(var + eps) * g.to(F64) + b.to(F64)
    y = act64(z, act)
    heads = []
    if hs:
        conv = max(conv, float(y.abs().max()))
        heads = [float((y @ H.to(F64).T).abs().max()) for H in hs]
    return conv, float(y.abs().max()), heads


CASES = [
    # (input block widths, additive blocks, layers, LayerNorm, heads, pre_act of block 0, output activation)
    ((128,), 2, 3, True, 0, SELU, NONE),           # the hoisted message launch of an MP layer
    ((128, 128), 0, 3, True, 2, NONE, SELU),       # the node launch with the next layer's two product heads
    ((128,), 0, 1, False, 0, NONE, NONE),          # a hoisted first-layer product (one bias-free-like layer, no LayerNorm)
    ((128, 128), 0, 2, True, 0, NONE, TANH),       # a pool / unpool MLP
    ((96, 128), 1, 2, False, 1, SELU, SELU),       # no LayerNorm: the output bound is the propagated one
]


@pytest.mark.parametrize("case", range(len(CASES)))
@pytest.mark.parametrize("adversarial", [False, True])
def test_fp64_activations_stay_below_the_bound(case, adversarial):
    widths, n_add, n_layers, ln, n_heads, pre0, act = CASES[case]
    gen = torch.Generator().manual_seed(100 * case + int(adversarial))
    for scale in (0.3, 1.0, 7.0):
        weights, biases, lnp, hs = make_mlp(gen, widths, n_layers, ln, n_heads, scale, adversarial)
        norms = ops.weight_norms(weights, biases, lnp, hs, widths)
        in_bounds = [2.5 * scale + 0.1 * j for j in range(len(widths))]          # bounds of the STORED rows
        add_bounds = [1.5 * scale] * n_add
        for mode in ("uniform", "corners", "plus", "minus", "spike"):
            rows = 64
            stored = [draw(gen, rows, w, b, mode) for w, b in zip(widths, in_bounds)]
            adds = [draw(gen, rows, 128, b, mode) for b in add_bounds]
            pre = [pre0] + [NONE] * (len(widths) - 1)
            sources = [Source(t.float(), pre_act=p, bound=b) for t, p, b in zip(stored, pre, in_bounds)]
            sources += [Source(a.float(), additive=True, bound=b) for a, b in zip(adds, add_bounds)]
            lb = ops.range_bounds(norms, sources, act)
            assert lb.converted is not None and lb.out is not None
            conv, out, heads = evaluate(weights, biases, lnp, hs, [act64(t, p) for t, p in zip(stored, pre)], adds, act)
            # (1e-9 relative: the reference evaluation itself rounds in fp64)
            assert conv <= lb.converted * (1 + 1e-9), (case, scale, mode, conv, lb.converted)
            assert out <= lb.out * (1 + 1e-9), (case, scale, mode, out, lb.out)
            assert all(h <= b * (1 + 1e-9) for h, b in zip(heads, lb.heads or [])), (heads, lb.heads)
            assert (lb.heads is None) == (n_heads == 0)


def test_layer_norm_bound_is_attained_by_a_spike_and_never_below_selu_floor():
    # one huge entry in a row: (x - mean) / std = sqrt(n - 1) exactly (eps -> 0): the bound's first term is sharp
    gen = torch.Generator().manual_seed(7)
    weights, biases, _, _ = make_mlp(gen, (128,), 2, False, 0)
    g, b = torch.full((128,), -3.0), torch.full((128,), 0.5)
    norms = ops.weight_norms(weights, biases, (g, b, 1e-12), [], (128,))
    lb = ops.range_bounds(norms, [Source(torch.zeros(4, 128), bound=1.0)], NONE)
    assert lb.out == pytest.approx(math.sqrt(127) * 3.0 + 0.5, rel=1e-12)
    z = torch.zeros(1, 128, dtype=F64)
    z[0, 5] = 1e6
    y = (z - z.mean()) / torch.sqrt(((z - z.mean()) ** 2).mean() + 1e-12) * g.to(F64) + b.to(F64)
    assert float(y.abs().max()) <= lb.out and float(y.abs().max()) > 0.98 * (lb.out - 1.0)
    # SELU on load of rows with a tiny bound: negative arguments still reach towards -scale * alpha = -1.7581
    assert ops.act_bound(1e-3, SELU) == pytest.approx(1.7580993408473766)
    assert ops.act_bound(10.0, SELU) == pytest.approx(10.507009873554805)
    assert ops.act_bound(None, TANH) == 1.0 and ops.act_bound(None, SELU) is None and ops.act_bound(3.0, NONE) == 3.0


def test_certificate_needs_twice_the_bound_below_the_end_of_the_range():
    assert ops.certifies(32751.99) and not ops.certifies(32752.0) and not ops.certifies(65503.0)
    assert not ops.certifies(None) and not ops.certifies(float("nan")) and not ops.certifies(float("inf"))
    gen = torch.Generator().manual_seed(3)
    weights, biases, lnp, hs = make_mlp(gen, (128,), 3, True, 0)
    src = [Source(torch.zeros(4, 128), pre_act=SELU, bound=40.0)]
    assert ops.certifies(ops.range_bounds(ops.weight_norms(weights, biases, lnp, hs, (128,)), src, NONE).converted)
    # the same MLP with its second layer scaled up: the hidden bound passes 65504 / 2 and the certificate is refused
    big = [weights[0], weights[1] * 3e4, weights[2]]
    lb = ops.range_bounds(ops.weight_norms(big, biases, lnp, hs, (128,)), src, NONE)
    assert lb.converted is not None and 2 * lb.converted >= 65504 and not ops.certifies(lb.converted)
    # ... while its OUTPUT bound (LayerNorm) does not depend on what goes in
    assert lb.out == ops.range_bounds(ops.weight_norms(weights, biases, lnp, hs, (128,)), src, NONE).out
    # a producer whose LayerNorm gain is 3e4: its readers are refused, whatever their own weights
    hot = ops.range_bounds(ops.weight_norms(weights, biases, (lnp[0] * 3e4, lnp[1], lnp[2]), hs, (128,)), src, NONE).out
    assert not ops.certifies(ops.range_bounds(ops.weight_norms(weights, biases, lnp, hs, (128,)),
                                              [Source(torch.zeros(4, 128), pre_act=SELU, bound=hot)], NONE).converted)


def test_no_certificate_without_a_complete_proof():
    gen = torch.Generator().manual_seed(5)
    weights, biases, lnp, hs = make_mlp(gen, (128, 128), 3, True, 2)
    norms = ops.weight_norms(weights, biases, lnp, hs, (128, 128))
    t = torch.zeros(4, 128)
    ok = ops.range_bounds(norms, [Source(t, bound=2.0), Source(t, bound=3.0)], SELU)
    assert ops.certifies(ok.converted) and ok.heads is not None
    # a source without a bound (a tensor handed in by a user, data entering an encoder)
    lb = ops.range_bounds(norms, [Source(t, bound=2.0), Source(t)], SELU)
    assert lb.converted is None and not ops.certifies(lb.converted)
    assert lb.out == ok.out          # (what comes out of a LayerNorm is bounded all the same)
    # an additive block without a bound
    n1 = ops.weight_norms(weights[:1] + weights[1:], biases, lnp, [], (128, 128))
    assert ops.range_bounds(n1, [Source(t, bound=1.0), Source(t, bound=1.0), Source(t, additive=True)], NONE).converted is None
    # another arithmetic (no norms), a narrow block multiplied on the vector ALUs
    assert ops.range_bounds(None, [Source(t, bound=1.0)], NONE).converted is None
    wn, bn, _, _ = make_mlp(gen, (4, 128), 2, False, 0)
    nn_ = ops.weight_norms(wn, bn, None, [], (4, 128), narrow=(True, False))
    assert nn_["narrow"] and ops.range_bounds(nn_, [Source(torch.zeros(4, 4), bound=1.0), Source(t, bound=1.0)], NONE).converted is None
    # a residual, an output index or a row sub-range: nothing is known about the output tensor
    assert ops.range_bounds(norms, [Source(t, bound=2.0), Source(t, bound=3.0)], SELU, residual=True).out is None
    # sums over segments multiply the bound by the longest segment; without its length there is no proof
    plan = types.SimpleNamespace(max_deg=6)
    s_sum = Source(t, bound=2.0)
    s_sum.segments, s_sum.seg_mean = plan, False
    a = ops.range_bounds(norms, [s_sum, Source(t, bound=3.0)], SELU, seg_len=6)
    b = ops.range_bounds(norms, [Source(t, bound=12.0), Source(t, bound=3.0)], SELU)
    assert a.converted == b.converted and ops.range_bounds(norms, [s_sum, Source(t, bound=3.0)], SELU).converted is None
    assert ops.agg_bound(2.0, plan, True) == 2.0 and ops.agg_bound(2.0, plan, False) == 12.0 and ops.agg_bound(None, plan, True) is None


def test_launch_certificate_is_set_per_launch_and_only_with_a_proof(monkeypatch):
    gen = torch.Generator().manual_seed(9)
    weights, biases, lnp, hs = make_mlp(gen, (128,), 3, True, 0)
    packed = types.SimpleNamespace(norms=ops.weight_norms(weights, biases, lnp, hs, (128,)), desc=_lib.g4c_mlp_t())
    t = torch.zeros(4, 128)
    assert ops._certify(packed, [Source(t, bound=2.0)], NONE, False, False).converted is not None and packed.desc.range_certified == 1
    ops._certify(packed, [Source(t)], NONE, False, False)
    assert packed.desc.range_certified == 0          # no bound on the input
    ops._certify(packed, [Source(t, bound=2.0)], NONE, False, True)
    assert packed.desc.range_certified == 0          # save / mul: the training forms keep their tracker
    monkeypatch.setattr(ops, "RANGE_PROOFS", False)
    ops._certify(packed, [Source(t, bound=2.0)], NONE, False, False)
    assert packed.desc.range_certified == 0
    # the answer of take_bounds() is handed out once
    monkeypatch.setattr(ops, "_last_bounds", ops.LaunchBounds(1.0, 2.0, [3.0]))
    assert ops.take_bounds().out == 2.0 and ops.take_bounds().out is None


def test_bounds_do_not_travel_on_tensors():
    t = torch.zeros(4, 128)
    s = Source(t, bound=2.0)
    assert Source(t).bound is None and Source(s.tensor).bound is None and not hasattr(t, "bound")
    rb = ops.RangeBounds()
    assert rb.v is None and rb.e is None and rb.product(0) is None
