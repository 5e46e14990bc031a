"""The fp64 backward references (oracle/grad_ref.py) and their checkers, on CPU: each restated adjoint equals torch autograd in
float64 over an nn.Sequential / GNBlock restatement, the integer generators keep every partial sum below 2^24, and the bounded
checker accepts the same computation done in fp32 with 32-k chunked sums while rejecting each perturbation the GPU tests use as a
negative control."""
import pytest
import torch
import torch.nn.functional as F

from oracle import grad_ref as R

F64 = torch.float64
H = 32


def _mlp_params(k_in, widths, ln, gen):
    Ws, bs, k = [], [], k_in
    for w in widths:
        Ws.append(torch.randn(w, k, generator=gen, dtype=F64) / k ** 0.5)
        bs.append(torch.randn(w, generator=gen, dtype=F64) * 0.1)
        k = w
    lnp = (1 + 0.2 * torch.randn(widths[-1], generator=gen, dtype=F64), 0.1 * torch.randn(widths[-1], generator=gen, dtype=F64)) if ln else None
    return Ws, bs, lnp


def _sequential(Ws, bs, lnp):
    layers = []
    for l, (W, b) in enumerate(zip(Ws, bs)):
        lin = torch.nn.Linear(W.size(1), W.size(0)).double()
        with torch.no_grad():
            lin.weight.copy_(W); lin.bias.copy_(b)
        layers.append(lin)
        if l < len(Ws) - 1:
            layers.append(torch.nn.SELU())
    if lnp is not None:
        ln = torch.nn.LayerNorm(Ws[-1].size(0), eps=R.LN_EPS).double()
        with torch.no_grad():
            ln.weight.copy_(lnp[0]); ln.bias.copy_(lnp[1])
        layers.append(ln)
    return torch.nn.Sequential(*layers)


def _csr(key, n_seg):
    perm = torch.argsort(key, stable=True)
    off = torch.zeros(n_seg + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(torch.bincount(key, minlength=n_seg), 0)
    return off, perm


@pytest.mark.parametrize("ln,act", [(True, "tanh"), (False, None), (True, None)])
def test_mlp_adjoint_equals_float64_autograd_every_source_kind(ln, act):
    g = torch.Generator().manual_seed(1)
    M, n_a, n_s = 97, 40, 300
    rel = torch.randn(M, 2, generator=g)                       # narrow, negated
    a = torch.randn(n_a, H, generator=g)                       # through an index, SELU on load
    b = torch.randn(M, H + 5, generator=g)                     # column window
    s = torch.randn(n_s, H, generator=g)                       # aggregated on load (mean, through a permutation; empty segments)
    key = torch.randint(2, M - 2, (n_s,), generator=g)         # segments 0, 1, M-2, M-1 stay empty
    off, perm = _csr(key, M)
    idx = torch.randint(0, n_a, (M,), generator=g)
    resid = torch.randn(M, H + 2, generator=g)
    srcs = [R.Src(rel, negate=True), R.Src(a, index=idx, pre_act="selu"), R.Src(b, col0=5, width=H),
            R.Src(s, segments=(off, perm), seg_mean=True, pre_act="selu"), R.Src(s[:M], segments=(torch.arange(M + 1), None), seg_mean=False)]
    k_in = 2 + 4 * H
    Ws, bs, lnp = _mlp_params(k_in, (H, H, H), ln, g)
    f = R.mlp_forward(srcs, Ws, bs, lnp, act, resid, 2)      # (fp64 against fp64: both take the same SELU branches)
    dy = torch.randn(M, H, generator=g, dtype=F64)
    got = R.mlp_adjoint(f, srcs, Ws, lnp, act, dy, resid=resid, resid_col0=2)
    # autograd over the restatement
    ins = [t.double().requires_grad_(True) for t in (rel, a, b, s, resid)]
    seq = _sequential(Ws, bs, lnp)
    seg = torch.repeat_interleave(torch.arange(M), off[1:] - off[:-1])
    agg = torch.zeros(M, H, dtype=F64).index_add_(0, seg, F.selu(ins[3])[perm]) / (off[1:] - off[:-1]).clamp(min=1)[:, None]
    x = torch.cat((-ins[0], F.selu(ins[1])[idx], ins[2][:, 5:5 + H], agg, ins[3][:M]), 1)
    y = seq(x)
    y = (torch.tanh(y) if act == "tanh" else y) + ins[4][:, 2:2 + H]
    torch.testing.assert_close(f.y, y.detach(), rtol=1e-12, atol=1e-12)
    y.backward(dy)
    lins = [m for m in seq if isinstance(m, torch.nn.Linear)]
    for l, lin in enumerate(lins):
        torch.testing.assert_close(got[f"W{l}"][0], lin.weight.grad, rtol=1e-10, atol=1e-10)
        torch.testing.assert_close(got[f"b{l}"][0], lin.bias.grad, rtol=1e-10, atol=1e-10)
    if ln:
        torch.testing.assert_close(got["gamma"][0], seq[-1].weight.grad, rtol=1e-10, atol=1e-10)
        torch.testing.assert_close(got["beta"][0], seq[-1].bias.grad, rtol=1e-10, atol=1e-10)
    for j in range(3):
        torch.testing.assert_close(got[f"src{j}"][0], ins[j].grad, rtol=1e-10, atol=1e-10)
    gs = got["src3"][0].clone()                                # (s feeds two blocks: the aggregated one and one-row plain sums)
    gs[:M] += got["src4"][0]
    torch.testing.assert_close(gs, ins[3].grad, rtol=1e-10, atol=1e-10)
    torch.testing.assert_close(got["resid"][0], ins[4].grad, rtol=1e-12, atol=1e-12)
    # the absolute-value forms bound the values
    for k, (v, va) in got.items():
        assert (v.abs() <= va * (1 + 1e-12) + 1e-300).all(), k
    # the saved-activation form (acts given) is the same adjoint when the given rows are the forward's own
    own = R.mlp_adjoint(f, srcs, Ws, lnp, act, dy, acts=[None] + f.a[1:], z_last=f.z[-1], resid=resid, resid_col0=2)
    for k in got:
        torch.testing.assert_close(own[k][0], got[k][0], rtol=1e-12, atol=1e-12)


def test_chain_equals_the_adjoint_layers():
    g = torch.Generator().manual_seed(2)
    Ws, bs, _ = _mlp_params(128, (128, 128, 128, 128), False, g)
    x = torch.randn(50, 128, generator=g, dtype=F64)
    f = R.mlp_forward([R.Src(x)], Ws, bs)
    dy = torch.randn(50, 128, generator=g, dtype=F64)
    full = R.mlp_adjoint(f, [R.Src(x)], Ws, None, None, dy)
    D, Da, gX, gXa = R.chain(dy, Ws, [None] + f.a[1:], Ws[0])
    for l in range(1, 5):
        torch.testing.assert_close(D[l], full[f"D{l}"][0], rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(gX, full["src0"][0], rtol=1e-12, atol=1e-12)


def test_building_blocks_equal_autograd():
    g = torch.Generator().manual_seed(3)
    z = (torch.randn(40, 65, generator=g, dtype=F64) * 2 + 0.3).requires_grad_(True)
    gam, bet = torch.randn(65, generator=g, dtype=F64).requires_grad_(True), torch.randn(65, generator=g, dtype=F64).requires_grad_(True)
    dy = torch.randn(40, 65, generator=g, dtype=F64)
    F.layer_norm(z, (65,), gam, bet, R.LN_EPS).backward(dy)
    (dz, dg, db), _ = R.layernorm_grad(z.detach(), gam.detach(), dy)
    for a, b in ((dz, z.grad), (dg, gam.grad), (db, bet.grad)):
        torch.testing.assert_close(a, b, rtol=1e-10, atol=1e-12)
    for act, fn in (("selu", F.selu), ("tanh", torch.tanh)):
        x = torch.randn(30, 7, generator=g, dtype=F64).requires_grad_(True)
        y = fn(x)
        dy = torch.randn_like(y)
        y.backward(dy)
        torch.testing.assert_close(R.act_grad(dy, x.detach(), act, True)[0], x.grad, rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(R.act_grad(dy, y.detach(), act, False)[0], x.grad, rtol=1e-12, atol=1e-12)
    # segment broadcast = adjoint of the segmented sum (through a permutation, empty segments at both ends)
    key = torch.randint(1, 9, (50,), generator=g)
    off, perm = _csr(key, 10)
    x = torch.randn(50, 3, generator=g, dtype=F64).requires_grad_(True)
    d = torch.randn(10, 3, generator=g, dtype=F64)
    R.segment_sum(x, off, perm, False).backward(d)
    torch.testing.assert_close(R.segment_broadcast(d, off, perm, 50, False), x.grad.float().double(), rtol=0, atol=0)
    # weight / bias gradient, linear
    W = torch.randn(5, 7, generator=g, dtype=F64).requires_grad_(True)
    b = torch.randn(5, generator=g, dtype=F64).requires_grad_(True)
    a = torch.randn(11, 7, generator=g, dtype=F64)
    y = a @ W.t() + b
    torch.testing.assert_close(R.linear(a, W.detach(), b.detach())[0], y.detach())
    gy = torch.randn_like(y)
    y.backward(gy)
    dW, db_, _, _ = R.weight_bias_grad(gy, a)
    torch.testing.assert_close(dW, W.grad)
    torch.testing.assert_close(db_, b.grad)


def test_gnblock_composition_equals_autograd():
    g = torch.Generator().manual_seed(4)
    n, E = 60, 300
    row, col = torch.randint(0, n, (E,), generator=g), torch.randint(0, n, (E,), generator=g)
    v, e = torch.randn(n, H, generator=g, dtype=F64), torch.randn(E, H, generator=g, dtype=F64)
    ep, np_ = _mlp_params(3 * H, (H, H, H), True, g), _mlp_params(2 * H, (H, H, H), True, g)
    fe, fv, es, ns = R.gnblock_forward(v, e, row, col, ep, np_)
    dv, de = torch.randn(n, H, generator=g, dtype=F64), torch.randn(E, H, generator=g, dtype=F64)
    got = R.gnblock_adjoint(fe, fv, es, ns, ep, np_, dv, de)
    se, sn = _sequential(*ep), _sequential(*np_)
    v2, e2 = v.clone().requires_grad_(True), e.clone().requires_grad_(True)
    e1 = se(torch.cat((e2, v2[row], v2[col]), 1))
    agg = torch.zeros(n, H, dtype=F64).index_add_(0, col, e1) / torch.bincount(col, minlength=n).clamp(min=1)[:, None]
    v1 = sn(torch.cat((agg, v2), 1))
    torch.testing.assert_close(fe.y, e1.detach())
    torch.testing.assert_close(fv.y, v1.detach())
    torch.autograd.backward([v1, e1], [dv, de])
    torch.testing.assert_close(got["v"][0], v2.grad)
    torch.testing.assert_close(got["e"][0], e2.grad)
    for pre, seq in (("edge.", se), ("node.", sn)):
        lins = [m for m in seq if isinstance(m, torch.nn.Linear)]
        for l, lin in enumerate(lins):
            torch.testing.assert_close(got[f"{pre}W{l}"][0], lin.weight.grad)
            torch.testing.assert_close(got[f"{pre}b{l}"][0], lin.bias.grad)
        torch.testing.assert_close(got[pre + "gamma"][0], seq[-1].weight.grad)
        torch.testing.assert_close(got[pre + "beta"][0], seq[-1].bias.grad)


# ------------------------------------------------------------------ integer generators
@pytest.mark.parametrize("M,K", [(33, 1300), (100003, 640), (600001, 128)])
def test_integer_generator_keeps_partial_sums_below_2_24(M, K):
    g = torch.Generator().manual_seed(M)
    v = R.vmax_for(M)
    a, b = R.int_operand((M, 8), v, g), R.int_operand((M, 8), v, g)
    abs_sum = a.abs().double().t() @ b.abs().double()
    R.check_int_bound(abs_sum)
    assert float((a.double()[:, :1] * b.double()).abs().cumsum(0).max()) <= float(abs_sum.max())
    assert K * R.vmax_for(K) ** 2 < 2 ** 24 and M * v ** 2 < 2 ** 24
    # fp32 sums of such values in any order are the exact sum
    exact = (a.double() * b.double()).sum(0)
    R.assert_exact((a * b).sum(0), exact, "fp32 sum")
    R.assert_exact((a * b).flip(0).cumsum(0)[-1], exact, "fp32 sum, reversed, sequential")
    assert R.rejects(R.check_int_bound, torch.tensor([2.0 ** 24]))


# ------------------------------------------------------------------ the bounded checker: accepts fp32 sums, rejects perturbations
def _mm32(a, b, kc=32):
    """a @ b in fp32, the contraction in 32-k steps added one after another (the MFMA chain's order)."""
    a, b = a.float(), b.float()
    out = torch.zeros(a.size(0), b.size(1))
    for k0 in range(0, a.size(1), kc):
        out = out + a[:, k0:k0 + kc] @ b[k0:k0 + kc]
    return out


def test_fp32_class_accepts_fp32_and_rejects_perturbations():
    g = torch.Generator().manual_seed(5)
    M = 1000 + 13                                         # a partial last 32-row tile
    gr, a = torch.randn(M, 128, generator=g), torch.randn(M, 128, generator=g)
    n_eff = R.n_eff_weight_grad(M)
    dW, _, dWa, _ = R.weight_bias_grad(gr, a)
    got = _mm32(gr.t(), a)
    R.assert_fp32_class(got, dW, dWa, n_eff, "dW fp32 32-k")
    for r in (M // 2, M - 1):                             # one row dropped
        bad = R.weight_bias_grad(gr, R.drop_row(a, r))
        assert R.rejects(R.assert_fp32_class, got, bad[0], bad[2], n_eff, "drop row")
    bad = R.weight_bias_grad(gr, R.zero_last_partial_row(a))
    assert R.rejects(R.assert_fp32_class, got, bad[0], bad[2], n_eff, "zero last partial row")
    # a layer with two adjacent weight columns swapped inside one 32-k step
    W = torch.randn(128, 128, generator=g) / 11
    y, ya = R.linear(a, W)
    got = _mm32(a, W.t())
    R.assert_fp32_class(got, y, ya, R.N_EFF_LAYER_K + R.N_EFF_SPLIT["bf16x6"], "linear fp32 32-k")
    bad = R.linear(a, R.swap_columns(W, 40))
    assert R.rejects(R.assert_fp32_class, got, bad[0], bad[1], R.N_EFF_LAYER_K, "swap columns")
    # a segment boundary moved by one
    key = torch.randint(0, 100, (M,), generator=g)
    off, perm = _csr(key, 100)
    d = torch.randn(100, 128, generator=g)
    ref = R.segment_broadcast(d, off, perm, M, True)
    got = ref.float()
    R.assert_fp32_class(got, ref, ref.abs(), 1, "broadcast")
    s = int(torch.nonzero((off[1:] - off[:-1]) > 1)[3])
    bad = R.segment_broadcast(d, R.move_boundary(off, s + 1), perm, M, True)
    assert R.rejects(R.assert_fp32_class, got, bad, bad.abs(), 1, "moved boundary")
    # one SELU slope from the other branch
    acts = F.selu(torch.randn(M, 128, generator=g))
    D, Da = R.chain_layer(gr, W, acts)
    got = _mm32(gr, W) * R.selu_slope_out(acts).float()
    R.assert_fp32_class(got, D, Da, R.N_EFF_LAYER_K + R.N_EFF_SPLIT["bf16x6"], "chain layer fp32")
    r = 7
    c = int(torch.argmax((gr[r].double() @ W.double()).abs()))
    bad = R.chain_layer(gr, W, R.flip_slope(acts, r, c))
    assert R.rejects(R.assert_fp32_class, got, bad[0], bad[1], R.N_EFF_LAYER_K, "flipped slope")
    # the exact checker: integer operands in fp32 32-k steps are exact; a dropped row is not
    ia, ib = R.int_operand((M, 4), 3, g), R.int_operand((M, 4), 3, g)
    got = _mm32(ia.t(), ib)
    R.assert_exact(got, ia.double().t() @ ib.double(), "int")
    r = int(torch.nonzero(ia.abs().sum(1) * ib.abs().sum(1) > 0)[0])
    assert R.rejects(R.assert_exact, got, ia.double().t() @ R.drop_row(ib.double(), r), "int, dropped row")
