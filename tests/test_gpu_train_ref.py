"""The training backward against plain fp64 references, launch by launch (oracle/grad_ref.py).

Exact (integer-valued operands, every partial sum below 2^24 — `assert_exact`): weight_bias_grad, colsum, autograd.linear,
train_gather, segment_broadcast.  Bounded (`assert_fp32_class`, C = 2, n_eff derived per kernel in grad_ref.py; SELU slopes from the
kernel's own fp32 activations): layernorm_grad, act_grad, backward_chain (layer-locally), the forward `save` rows, the _FusedMLP
backward per source kind, and one GNBlock training step at the headline size with the thresholds as shipped.  Each test that
depends on a switch sets it and proves the path it took (ops.mlp_forward / autograd calls counted).  Negative controls: perturbed
references must be rejected by the same checkers on correct kernel output."""
import os
import sys
import time

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pytestmark = pytest.mark.gpu

from graphs4cfd_amd import _lib, ops, plan, autograd as A, synthetic as S     # noqa: E402
from graphs4cfd_amd.nn import blocks as B                                     # noqa: E402
from oracle import grad_ref as R                                              # noqa: E402

DEV = torch.device("cuda", 0)
F64 = torch.float64
H = 128
ACT = {"selu": _lib.ACT_SELU, "tanh": _lib.ACT_TANH, None: _lib.ACT_NONE}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ints(shape, vmax, g, density=1.0):
    return R.int_operand(shape, vmax, g, density).to(DEV)


class Trace:
    """Counts the paths a training step takes: every ops.mlp_forward call's `save` / `mul` / precision, and the operands of the
    backward's weight-gradient and LayerNorm-adjoint calls (the activations the backward really used)."""

    def __init__(self, monkeypatch):
        self.fwd, self.events, self.chains = [], [], 0
        f0, w0, l0, c0 = ops.mlp_forward, A.weight_bias_grad, A.layernorm_grad, A.backward_chain

        def fwd(*a, **k):
            self.fwd.append(dict(save=k.get("save") is not None, mul=k.get("mul") is not None, split=a[0].split,
                                 additive=any(s.additive for s in a[1])))
            return f0(*a, **k)

        def wg(g, a, want_bias=True):
            self.events.append(("wg", g.detach().clone(), a.detach().clone(), want_bias))
            return w0(g, a, want_bias)

        def lng(z, gamma, dy, eps):
            self.events.append(("ln", z.detach().clone()))
            return l0(z, gamma, dy, eps)

        def chain(*a):
            self.chains += 1
            return c0(*a)

        monkeypatch.setattr(ops, "mlp_forward", fwd)
        monkeypatch.setattr(A, "weight_bias_grad", wg)
        monkeypatch.setattr(A, "layernorm_grad", lng)
        monkeypatch.setattr(A, "backward_chain", chain)

    def saving_forwards(self):
        return sum(1 for c in self.fwd if c["save"] and not c["mul"])

    def chain_launches(self):
        return sum(1 for c in self.fwd if c["mul"])

    def backwards(self, L, has_ln=True):
        """Per _FusedMLP backward (in execution order): (acts [None, a1 .. a_{L-1}], z_last, hoisted weight-gradient calls)."""
        out, cur = [], None
        for ev in self.events:
            if ev[0] == "ln" or cur is None:
                cur = {"z": ev[1] if ev[0] == "ln" else None, "wg": []}
                out.append(cur)
            if ev[0] == "wg":
                cur["wg"].append(ev)
        res = []
        for c in out:
            acts = [None] + [c["wg"][L - 2 - i][2] for i in range(L - 1)]
            res.append((acts, c["z"], sum(1 for e in c["wg"] if not e[3])))
        return res


# ====================================================================== exact
WG_CASES = ([(M, 128, 128, True, False) for M in (0, 1, 31, 32, 33, 63, 65, 191, 193, 98500, 600001)]
            + [(M, 129, 131, True, True) for M in (1, 33, 193, 98500)]
            + [(193, N, 128, True, False) for N in (1, 3, 32, 127, 129, 200, 256)]
            + [(193, 128, K, False, False) for K in (2, 5, 131, 256, 259)]
            + [(600001, 3, 5, True, True), (65, 200, 259, False, True), (193, 128, 128, False, True)])


@pytest.mark.parametrize("M,N,K,want_bias,window", WG_CASES)
def test_weight_bias_grad_exact(M, N, K, want_bias, window):
    """window: g and a are column windows at offset 3 of tensors with a leading dimension that is not a multiple of 4 (the
    zero-padded copy of _pad128)."""
    g = _gen(M * 7 + N + K)
    v = R.vmax_for(max(M, 1), cap=5)
    if window:
        gw, aw = _ints((M, N + 7), v, g), _ints((M, K + 6), v, g)          # ld N + 7 / K + 6: ld % 4 != 0 for these shapes or offset 3
        go, ao = gw[:, 3:3 + N], aw[:, 3:3 + K]
    else:
        go, ao = _ints((M, N), v, g), _ints((M, K), v, g)
    R.check_int_bound(go.abs().double().t() @ ao.abs().double(), go.abs().double().sum(0))
    dW, db = A.weight_bias_grad(go, ao, want_bias)
    ref, rb, _, _ = R.weight_bias_grad(go, ao)
    R.assert_exact(dW, ref, f"dW M={M} N={N} K={K}")
    if want_bias:
        R.assert_exact(db, rb, "db")
    else:
        assert db is None
    if M == 600001 and N == 128:           # negative controls of the exact checker at size: one row dropped, the last row of the partial tile
        r = int(torch.nonzero((go.abs().sum(1) * ao.abs().sum(1)) > 0)[len(go) // 2])
        assert R.rejects(R.assert_exact, dW, R.weight_bias_grad(go, R.drop_row(ao, r))[0])
        assert R.rejects(R.assert_exact, dW, R.weight_bias_grad(go, R.zero_last_partial_row(ao))[0]) or not bool(
            (go[-1].abs().sum() * ao[-1].abs().sum()) > 0)


@pytest.mark.parametrize("width", [1, 3, 255, 256, 257])
@pytest.mark.parametrize("rows", [0, 1, 127, 129, 2048 * 128 + 77])
def test_colsum_exact(width, rows):
    g = _gen(width * 31 + rows)
    x = _ints((rows, width), R.vmax_for(max(rows, 1), 1, cap=50), g)
    R.check_int_bound(x.abs().double().sum(0))
    R.assert_exact(A.colsum(x), R.colsum(x)[0], f"colsum {rows}x{width}")
    if rows > 2048 * 128:
        assert int(_lib.load().g4c_colsum_partials(rows)) == 2048       # past the cap: more rows per stage-1 workgroup


LIN_CASES = ([(n, k, 33, True) for n in (1, 3, 128, 129, 300) for k in (1, 2, 5, 128, 131, 640, 1300)]
             + [(129, 640, M, b) for M in (1, 31, 100003) for b in (True, False)]
             + [(3, 131, M, False) for M in (1, 31, 33)] + [(128, 128, 100003, True), (300, 1300, 100003, False)])


@pytest.mark.parametrize("n_out,k,M,bias", LIN_CASES)
def test_linear_exact(n_out, k, M, bias, monkeypatch):
    """autograd.linear in bf16x6 (the backward's product launches): > 128 outputs 128 columns at a time, > 4 input blocks grouped
    through an additive partial (k = 640, 1300)."""
    monkeypatch.setattr(ops, "_PRECISION", "bf16x6")
    tr = Trace(monkeypatch)
    g = _gen(n_out * 1000 + k + M)
    v = R.vmax_for(k + 1, cap=8)
    x, W = _ints((M, k), v, g), _ints((n_out, k), v, g)
    b = _ints((n_out,), v, g) if bias else None
    R.check_int_bound(x.abs().double() @ W.abs().double().t() + (b.abs().double() if bias else 0))
    y = A.linear(x, W, b)
    R.assert_exact(y, R.linear(x, W, b)[0], f"linear n_out={n_out} k={k} M={M}")
    assert tr.fwd and all(c["split"] == "bf16x3" for c in tr.fwd)
    blocks = -(-k // 128)
    assert any(c["additive"] for c in tr.fwd) == (blocks > _lib.MAX_SRC)
    assert len(tr.fwd) == -(-n_out // 128) * (1 if blocks <= _lib.MAX_SRC else 1 + -(-(blocks - _lib.MAX_SRC) // (_lib.MAX_SRC - 1)))
    if (n_out, k, M) == (129, 640, 100003) and bias:        # negative control: two weight columns swapped inside one 32-k step
        assert R.rejects(R.assert_exact, y, R.linear(x, R.swap_columns(W, 520), b)[0])


@pytest.mark.parametrize("width,scol0,dcol0,v4", [(128, 0, 0, True), (64, 4, 8, True), (5, 0, 1, False), (128, 3, 0, False), (8, 0, 2, False)])
@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("negate", [False, True])
@pytest.mark.parametrize("indexed", [False, True])
def test_train_gather_exact(width, scol0, dcol0, v4, accumulate, negate, indexed):
    g = _gen(width + scol0 * 3 + dcol0 * 5 + 2 * accumulate + negate)
    n_src, n = 700, 1000
    src = _ints((n_src if indexed else n, scol0 + width + 4), 50, g)
    dst = _ints((n, dcol0 + width + 4), 50, g)
    idx = torch.randint(0, n_src // 2, (n,), generator=g).to(DEV) if indexed else None     # repeated rows; rows >= n_src / 2 unused
    want = R.gather(src, idx, scol0, width, None, negate, dst, dcol0, accumulate)
    assert (src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0 and src.stride(0) % 4 == 0 and dst.stride(0) % 4 == 0
            and scol0 % 4 == 0 and dcol0 % 4 == 0 and width % 4 == 0) == v4           # (the launcher's condition for the V = 4 kernel)
    A.train_gather(src, dst, dcol0, scol0, width, None if idx is None else plan.index32(idx), _lib.ACT_NONE, negate, n, accumulate)
    R.assert_exact(dst, want, "train_gather")


@pytest.mark.parametrize("width", [1, 3, 64, 65, 128, 200])
@pytest.mark.parametrize("mean", [False, True])
@pytest.mark.parametrize("permuted", [False, True])
def test_segment_broadcast_exact(width, mean, permuted):
    """Empty segments at both ends, one long segment; mean restated with the kernel's fp32 `g * (1.f / count)`."""
    g = _gen(width * 4 + 2 * mean + permuted)
    n_seg, n = 300, 6000
    key = torch.cat([torch.randint(3, n_seg - 3, (n - 2500,), generator=g), torch.full((2500,), 150)])
    key = key[torch.randperm(n, generator=g)] if permuted else key.sort().values
    csr = plan.build_csr(key, n_seg, DEV)
    assert (csr.perm is None) == (not permuted)
    dout = torch.randn(n_seg, width, generator=g).to(DEV)
    got = A.segment_broadcast(dout, csr, mean, n)
    want = R.segment_broadcast(dout, csr.off, csr.perm, n, mean)
    R.assert_exact(got, want, "segment_broadcast")
    if width == 65 and mean and permuted:                     # negative control: a boundary moved by one
        s = 150 if int(csr.off[151] - csr.off[150]) > 1 else 100
        assert R.rejects(R.assert_exact, got, R.segment_broadcast(dout, R.move_boundary(csr.off, s), csr.perm, n, mean))


# ====================================================================== bounded
@pytest.mark.parametrize("width", [1, 2, 63, 64, 65, 128, 200, 255, 256])
@pytest.mark.parametrize("rows", [0, 1, 3, 5, 70001])
def test_layernorm_grad_bounded(width, rows):
    g = _gen(width * 13 + rows)
    z = (torch.randn(rows, width, generator=g) * 2 + 0.3).to(DEV)
    gamma, dy = torch.randn(width, generator=g).to(DEV), torch.randn(rows, width, generator=g).to(DEV)
    dz, dg, db = A.layernorm_grad(z, gamma, dy, R.LN_EPS)
    (rz, rg, rb), (az, ag, ab) = R.layernorm_grad(z, gamma, dy)
    nwg = int(_lib.load().g4c_layernorm_grad_partials(rows))
    # dgamma / dbeta: each wave adds its rows in order (rows / (4 waves x nwg workgroups)), 4 waves in a 2-level tree, the colsum of
    # the nwg partial rows, on top of the per-row error of xhat
    n_col = -(-rows // (4 * nwg)) + 2 + R.n_eff_colsum(nwg, 2 * width) + R.N_EFF_LN_ROW
    R.assert_fp32_class(dz, rz, az, R.N_EFF_LN_ROW, f"LN dz w={width} rows={rows}")
    R.assert_fp32_class(dg, rg, ag, n_col, "LN dgamma")
    R.assert_fp32_class(db, rb, ab, n_col, "LN dbeta")
    if rows == 70001:
        assert nwg == 1024                                    # past the cap: the grid-stride loop
        if width == 128:                                      # negative control: one row dropped from the dgamma contraction
            (_, bad, _), (_, bada, _) = R.layernorm_grad(z, gamma, R.drop_row(dy, 777))
            assert R.rejects(R.assert_fp32_class, dg, bad, bada, n_col, "dropped row")


def test_launches_without_rows():
    """No rows: the row operands of an empty tensor may be null pointers; the sums are zero, nothing is written."""
    z = torch.empty(0, 64, device=DEV)
    assert torch.equal(A.colsum(z), torch.zeros(64, device=DEV))
    dz, dg, db = A.layernorm_grad(z, torch.ones(64, device=DEV), z, R.LN_EPS)
    assert dz.shape == (0, 64) and torch.equal(dg, torch.zeros(64, device=DEV)) and torch.equal(db, torch.zeros(64, device=DEV))
    assert A.act_grad(z, z, _lib.ACT_SELU, False).shape == (0, 64)
    A.train_gather(z, z, 0, 0, 64, None, _lib.ACT_NONE, False, 0)
    empty = plan.build_csr(torch.empty(0, dtype=torch.int64), 0, DEV)
    assert torch.equal(A.segment_broadcast(torch.empty(0, 64, device=DEV), empty, True, 5), torch.zeros(5, 64, device=DEV))


def test_layernorm_grad_refuses_257():
    z = torch.zeros(4, 257, device=DEV)
    with pytest.raises(NotImplementedError):
        A.layernorm_grad(z, torch.ones(257, device=DEV), z, R.LN_EPS)


@pytest.mark.parametrize("act", ["selu", "tanh"])
@pytest.mark.parametrize("from_input", [False, True])
@pytest.mark.parametrize("width", [128, 7])                 # V = 4 / V = 1
def test_act_grad_bounded(act, from_input, width):
    g = _gen(width + from_input)
    tiny = 2.0 ** -149
    special = torch.tensor([0.0, -0.0, tiny, -tiny, 2 * tiny, -2 * tiny, 3 * tiny, -3 * tiny, 1.1754944e-38, -1.1754944e-38, 1e-7, -1e-7])
    x = torch.randn(999, width, generator=g) * 2
    x.view(-1)[:special.numel()] = special
    ref = x if from_input else torch.tanh(x) if act == "tanh" else torch.nn.functional.selu(x)
    ref = ref.to(DEV)
    dy = torch.randn(999, width, generator=g).to(DEV)
    got = A.act_grad(dy, ref, ACT[act], from_input)
    want, absw = R.act_grad(dy, ref, act, from_input)
    R.assert_fp32_class(got, want, absw, R.N_EFF_ACT, f"act_grad {act} from_input={from_input} w={width}")


CHAIN_N = R.N_EFF_LAYER_K + R.N_EFF_SPLIT["bf16x6"] + 1        # one 128-k layer, the bf16x3 split, the slope product


@pytest.mark.parametrize("L", [2, 3, 4])
@pytest.mark.parametrize("M", [1, 31, 32, 33, 65537, 100003])
def test_backward_chain_layer_local(L, M):
    """backward_chain (the fused kernel's `mul` epilogue): each D[l] against (D_got[l+1] W[l]) * slope(a[l]) on the given fp32
    activations (exact zeros and values a few ulps from 0 among them), then gX = D_got[1] W_dense."""
    g = _gen(L * 1000 + M)
    Ws = [torch.randn(H, H, generator=g).to(DEV) / 11 for _ in range(L)]
    wd = torch.randn(H, H, generator=g).to(DEV) / 11
    acts = [None] + [torch.nn.functional.selu(torch.randn(M, H, generator=g)).to(DEV) for _ in range(L - 1)]
    for a in acts[1:]:
        a.view(-1)[:6] = torch.tensor([0.0, -0.0, 2.0 ** -149, -(2.0 ** -149), 1e-30, -1e-30], device=DEV)
    gr = torch.randn(M, H, generator=g).to(DEV)
    D, gX = A.backward_chain(gr, Ws, acts, wd)
    D[L] = gr
    for l in range(L - 1, 0, -1):
        ref, absr = R.chain_layer(D[l + 1], Ws[l], acts[l])
        R.assert_fp32_class(D[l], ref, absr, CHAIN_N, f"chain L={L} M={M} D[{l}]")
    ref, absr = R.linear(D[1], wd.t())
    R.assert_fp32_class(gX, ref, absr, CHAIN_N, f"chain L={L} M={M} gX")
    if M == 100003:                  # negative controls of the bounded checker: one slope from the other branch; two k swapped
        r = M - 1
        c = int((D[L][r].double() @ Ws[L - 1].double()).abs().argmax())
        bad = R.chain_layer(D[L], Ws[L - 1], R.flip_slope(acts[L - 1], r, c))
        assert R.rejects(R.assert_fp32_class, D[L - 1], bad[0], bad[1], CHAIN_N, "flipped slope")
        bad = R.chain_layer(D[L], R.swap_columns(Ws[L - 1].t(), 40).t(), acts[L - 1])
        assert R.rejects(R.assert_fp32_class, D[L - 1], bad[0], bad[1], CHAIN_N, "swapped k")


def _mlp_params(mlp):
    lins = mlp._linears()
    ln = mlp.MLP.layer_norm if hasattr(mlp.MLP, "layer_norm") else None
    return ([l.weight.detach() for l in lins], [l.bias.detach() for l in lins],
            None if ln is None else (ln.weight.detach(), ln.bias.detach()))


def _param_name(k):
    if k == "gamma":
        return "MLP.layer_norm.weight"
    if k == "beta":
        return "MLP.layer_norm.bias"
    return f"MLP.linear_{int(k[1:]) + 1}.{'weight' if k[0] == 'W' else 'bias'}"


@pytest.mark.parametrize("precision", ["f16x3", "bf16x6"])
@pytest.mark.parametrize("ln", [True, False])
@pytest.mark.parametrize("M", [1, 33, 1013, 65537])
def test_forward_save_rows(precision, ln, M):
    """The training forward's `save` rows (SELU outputs of the hidden layers, the pre-LayerNorm rows) and its output, against an fp64
    forward of the same launch; M with a partial last 32-row tile."""
    g = _gen(M + 2 * ln)
    torch.manual_seed(M)
    mlp = B.MLP(H + H + 3, (H, H, H), ln).to(DEV)
    Ws, bs, lnp = _mlp_params(mlp)
    x, a, c = (torch.randn(M, H, generator=g).to(DEV), torch.randn(50, H, generator=g).to(DEV), torch.randn(M, 3, generator=g).to(DEV))
    idx = torch.randint(0, 50, (M,), generator=g).to(DEV)
    pk = ops.PackedMLP(Ws, bs, None if lnp is None else (lnp[0], lnp[1], R.LN_EPS), [H, H, 3], [False] * 3, precision=precision)
    saves = [torch.empty(M, H, device=DEV) for _ in range(2)] + [torch.empty(M, H, device=DEV) if ln else None]
    with torch.no_grad():
        y = ops.mlp_forward(pk, [ops.Source(x), ops.Source(a, plan.index32(idx), pre_act=_lib.ACT_SELU), ops.Source(c)], M,
                            _lib.ACT_TANH, save=saves)
    f = R.mlp_forward([R.Src(x), R.Src(a, index=idx, pre_act="selu"), R.Src(c)], Ws, bs, lnp, "tanh", split=precision)
    for l in range(2):
        R.assert_fp32_class(saves[l], f.a[l + 1], f.A[l + 1], f.n_fwd[l] + R.N_EFF_ACT, f"save {precision} M={M} a[{l + 1}]")
    if ln:
        R.assert_fp32_class(saves[2], f.z[-1], f.Z[-1], f.n_fwd[-1], "save z_last")
    R.assert_fp32_class(y, f.y, f.Y0, f.n_fwd[-1] + R.N_EFF_LN_ROW + R.N_EFF_ACT, "output")


# ---------------------------------------------------------------------- _FusedMLP backward per source kind
def _config(kind, g):
    """(k_in, M, torch sources, reference sources, resid, act, ln, max_deg)."""
    if kind == "mixed":                 # the kinds of test_fused_mlp_gradients_all_source_kinds
        M, n_a = 3000, 500
        rel, a = torch.randn(M, 2, generator=g), torch.randn(n_a, H, generator=g)
        b, c = torch.randn(M, H + 5, generator=g), torch.randn(M, 3, generator=g)
        idx = torch.randint(0, n_a, (M,), generator=g)
        t = [x.to(DEV).requires_grad_(True) for x in (rel, a, b, c)]
        idx = idx.to(DEV)
        srcs = [ops.Source(t[0], negate=True), ops.Source(t[1], plan.index32(idx), pre_act=_lib.ACT_SELU), ops.Source(t[2], col0=5, width=H),
                ops.Source(t[3])]
        refs = [R.Src(t[0].detach(), negate=True), R.Src(t[1].detach(), index=idx, pre_act="selu"), R.Src(t[2].detach(), col0=5, width=H),
                R.Src(t[3].detach())]
        resid = torch.randn(M, H + 2, generator=g).to(DEV).requires_grad_(True)
        return 2 + H + H + 3, M, t, srcs, refs, resid, "tanh", True, int(torch.bincount(idx).max())
    if kind == "edge":                  # one dense 128-wide block + two gathered node blocks: hoisted, the chain can engage
        M, n = 3000, 700
        e, v = torch.randn(M, H, generator=g), torch.randn(n, H, generator=g)
        row, col = torch.randint(0, n, (M,), generator=g).to(DEV), torch.randint(0, n, (M,), generator=g).to(DEV)
        t = [x.to(DEV).requires_grad_(True) for x in (e, v)]
        srcs = [ops.Source(t[0]), ops.Source(t[1], plan.index32(row)), ops.Source(t[1], plan.index32(col))]
        refs = [R.Src(t[0].detach()), R.Src(t[1].detach(), index=row), R.Src(t[1].detach(), index=col)]
        return 3 * H, M, t, srcs, refs, None, None, True, int(max(torch.bincount(row).max(), torch.bincount(col).max()))
    # aggregation on load: segments in order with empty segments at both ends (mean), or through a permutation (sum, SELU on load)
    n_seg, n_e = 1000, 3000
    key = torch.randint(2, n_seg - 2, (n_e,), generator=g)
    key = key.sort().values if kind == "node-mean" else key
    csr = plan.build_csr(key, n_seg, DEV)
    e, v = torch.randn(n_e, H, generator=g), torch.randn(n_seg, H, generator=g)
    t = [x.to(DEV).requires_grad_(True) for x in (e, v)]
    mean, pa = kind == "node-mean", (_lib.ACT_NONE if kind == "node-mean" else _lib.ACT_SELU)
    srcs = [ops.Source(t[0], segments=csr, seg_mean=mean, pre_act=pa), ops.Source(t[1])]
    refs = [R.Src(t[0].detach(), segments=(csr.off, csr.perm), seg_mean=mean, pre_act=None if mean else "selu"), R.Src(t[1].detach())]
    return 2 * H, n_seg, t, srcs, refs, None, None, True, int(csr.max_deg)


FUSED_CASES = ([(k, p, s, False) for k in ("mixed", "node-mean", "node-sum-perm") for p in ("f16x3", "bf16x6") for s in (True, False)]
               + [("edge", p, s, ch) for p in ("f16x3", "bf16x6") for s in (True, False) for ch in (True, False)])


@pytest.mark.parametrize("kind,precision,save,chain", FUSED_CASES)
def test_fused_mlp_backward_per_source_kind(kind, precision, save, chain, monkeypatch):
    """_FusedMLP backward (hoisting and single-layer launches forced on at this size; FUSED_CHAIN = `chain`): parameter gradients
    elementwise, input gradients per element (each row against its own |g| |W|), the backward's activations against the fp64 forward."""
    monkeypatch.setattr(ops, "_PRECISION", precision)
    monkeypatch.setattr(A, "SAVE_ACTIVATIONS", save)
    monkeypatch.setattr(A, "FUSED_CHAIN", chain)
    monkeypatch.setattr(A, "HOIST_MIN_ROWS", 0)
    monkeypatch.setattr(A, "FUSED_LINEAR_MIN_ROWS", 0)
    g = _gen(hash((kind, precision, save, chain)) % 10007)
    torch.manual_seed(3)
    k_in, M, t, srcs, refs, resid, act, ln, max_deg = _config(kind, g)
    mlp = B.MLP(k_in, (H, H, H), ln).to(DEV)
    tr = Trace(monkeypatch)
    y = mlp.run(srcs, M, activation=torch.tanh if act == "tanh" else None, resid=resid, resid_col0=2)
    dy = torch.randn(y.shape, generator=g).to(DEV)
    y.backward(dy)
    # the path taken
    assert tr.saving_forwards() == (1 if save else 0)           # (f16x3 too: its pack is the bf16x6 kernel family, precision "bf16x6")
    assert tr.chain_launches() == (1 if (chain and kind == "edge") else 0)
    (acts, z_last, n_hoisted), = tr.backwards(3, ln)
    assert n_hoisted == {"mixed": 1, "edge": 2}.get(kind, 0)
    # reference on the backward's own activations
    Ws, bs, lnp = _mlp_params(mlp)
    f = R.mlp_forward(refs, Ws, bs, lnp, act, resid.detach() if resid is not None else None, 2, split=precision)
    for l in (1, 2):
        R.assert_fp32_class(acts[l], f.a[l], f.A[l], f.n_fwd[l - 1] + R.N_EFF_ACT, f"{kind} activations a[{l}]")
    want = R.mlp_adjoint(f, refs, Ws, lnp, act, dy, acts=acts, z_last=z_last, resid=None if resid is None else resid.detach(), resid_col0=2)
    n_eff = R.n_eff_mlp_grad(k_in, 3, max(M, max(int(x.size(0)) for x in t)), precision, ln, max_deg)
    params = dict(mlp.named_parameters())
    for k, (val, absv) in want.items():
        if k[0] in "Wbg":
            R.assert_fp32_class(params[_param_name(k)].grad, val, absv, n_eff, f"{kind} {precision} save={save} chain={chain} {k}")
    for j, x in enumerate(t):
        val = sum(want[f"src{i}"][0] for i, r in enumerate(refs) if r.x.data_ptr() == x.data_ptr())
        absv = sum(want[f"src{i}"][1] for i, r in enumerate(refs) if r.x.data_ptr() == x.data_ptr())
        R.assert_fp32_class(x.grad, val, absv, n_eff, f"{kind} input {j}")
    if resid is not None:
        R.assert_fp32_class(resid.grad, *want["resid"], 1, "resid")


# ---------------------------------------------------------------------- at size
@pytest.mark.parametrize("precision", ["f16x3", "bf16x6"])
def test_gnblock_training_step_at_size(precision, monkeypatch):
    """One GNBlock step at the headline shape (100k nodes, 600k edges, H = 128) with the thresholds as shipped: the edge MLP's first
    layer is hoisted and its hidden layers go through the one-launch chain on their own.  Against float64 autograd restated on the
    GPU (grad_ref.gnblock_*), slopes on the backward's own activations; the rows where fp64 could take the other SELU branch are
    counted, and every branch the kernel took differently lies in them."""
    monkeypatch.setattr(ops, "_PRECISION", precision)
    assert (A.HOIST_MIN_ROWS, A.FUSED_LINEAR_MIN_ROWS, A.SAVE_ACTIVATIONS, A.FUSED_CHAIN) == (32768, 65536, True, True)
    tr = Trace(monkeypatch)
    graph = S.mus_graph(100_000, levels=1, seed=9, device=DEV)
    ei = graph.edge_index
    n, E = graph.num_nodes, int(ei.size(1))
    assert n == 100_000 and E == 600_000
    torch.manual_seed(5)
    blk = B.GNBlock((3 * H, (H, H, H), True), (2 * H, (H, H, H), True)).to(DEV)
    g = _gen(6)
    v = torch.randn(n, H, generator=g).to(DEV).requires_grad_(True)
    e = torch.randn(E, H, generator=g).to(DEV).requires_grad_(True)
    dv, de = torch.randn(n, H, generator=g).to(DEV), torch.randn(E, H, generator=g).to(DEV)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    v1, e1 = blk.forward(v, e, ei)
    torch.autograd.backward([v1, e1], [dv, de])
    torch.cuda.synchronize()
    t_step = time.perf_counter() - t0
    assert tr.chain_launches() == 1 and tr.saving_forwards() == 2
    (node_acts, node_z, node_h), (edge_acts, edge_z, edge_h) = tr.backwards(3)
    assert (node_h, edge_h) == (0, 2)
    t1 = time.perf_counter()
    row, col = ei
    ep, np_ = _mlp_params(blk.edge_mlp), _mlp_params(blk.node_mlp)
    fe, fv, es, ns = R.gnblock_forward(v.detach(), e.detach(), row, col, ep, np_, split=precision)
    for name, fw, acts in (("edge", fe, edge_acts), ("node", fv, node_acts)):
        amb = fw.ambiguous_rows()
        flips = torch.zeros_like(amb)
        for l in (1, 2):
            flips |= ((acts[l] > 0) != (fw.z[l - 1] > 0)).any(1)
        print(f"  {name} MLP ({precision}): {int(amb.sum())} of {amb.numel()} rows within fp32 reach of the SELU kink, "
              f"{int(flips.sum())} rows where the kernel took the other branch than fp64")
        assert not bool((flips & ~amb).any()), "a SELU branch differs from fp64 outside the ambiguous rows"
        assert int(flips.sum()) <= max(10, amb.numel() // 200)
    want = R.gnblock_adjoint(fe, fv, es, ns, ep, np_, dv, de, (edge_acts, edge_z), (node_acts, node_z))
    max_deg = int(max(torch.bincount(row).max(), torch.bincount(col).max()))
    n_eff = R.n_eff_mlp_grad(3 * H, 3, E, precision, True, max_deg) + R.n_eff_mlp_grad(2 * H, 3, n, precision, True, max_deg)
    params = dict(blk.named_parameters())
    for k, (val, absv) in want.items():
        if k in ("v", "e"):
            continue
        pre, rest = k.split(".", 1)
        R.assert_fp32_class(params[f"{pre}_mlp.{_param_name(rest)}"].grad, val, absv, n_eff, f"at size {precision} {k}")
    R.assert_fp32_class(v.grad, *want["v"], n_eff, f"at size {precision} dv")
    R.assert_fp32_class(e.grad, *want["e"], n_eff, f"at size {precision} de")
    print(f"  GNBlock step at 100k nodes / 600k edges ({precision}): HIP forward + backward {1e3 * t_step:.1f} ms (first call, "
          f"includes plan building), fp64 reference + checks {time.perf_counter() - t1:.1f} s")
