"""Mixed-precision training (`ops.set_train_precision("bf16")`, `TrainConfig(mixed_precision=True)`) on the GPU.

Launch by launch against fp64 references of the mode's own arithmetic (tests/mixed_ref.py: both operands of every product rounded
once to bf16, round to nearest even; bias gradients from the unrounded rows), with the checkers of oracle/grad_ref.py: exact for
integer operands (magnitudes <= 8 are exact in bf16), `assert_fp32_class` with C = 2 for random ones.  Every bounded check also
asserts that the UNROUNDED fp64 product is rejected: a kernel that skipped the rounding or truncated would sit ~2^-9 away.  Then one
training step of two models against the oracle's fp64 autograd, and `fit(mixed_precision=True)`."""
import contextlib
import math
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pytestmark = pytest.mark.gpu

import graphs4cfd_amd as gfd                                              # noqa: E402
import mixed_ref as MR                                                    # noqa: E402
from graphs4cfd_amd import _lib, ops, plan, autograd as A, synthetic as S    # noqa: E402
from graphs4cfd_amd.nn import blocks as B                                 # noqa: E402
from oracle import bf16_ref as R16, g4c_oracle as O, grad_ref as R        # noqa: E402

DEV = torch.device("cuda", 0)
H = 128


@contextlib.contextmanager
def mixed(forward: bool = False):
    """The backward in the mode; `forward`: the recorded forward too (what `fit` selects)."""
    old_t = ops.set_train_precision("bf16")
    old_m = ops.set_mlp_precision("bf16") if forward else None
    try:
        yield
    finally:
        ops.set_train_precision(old_t)
        if forward:
            ops.set_mlp_precision(old_m)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _ints(shape, vmax, g):
    return R.int_operand(shape, vmax, g).to(DEV)


def _randn(shape, g, scale=1.0):
    return (torch.randn(shape, generator=g) * scale).to(DEV)


def _launches(monkeypatch):
    """Every ops.mlp_forward call: (precision of the packed image, save given, mul given)."""
    calls, f0 = [], ops.mlp_forward

    def fwd(*a, **k):
        calls.append((a[0].precision, k.get("save") is not None, k.get("mul") is not None))
        return f0(*a, **k)
    monkeypatch.setattr(ops, "mlp_forward", fwd)
    return calls


# ====================================================================== g4c_weight_grad_bf16
# Row counts, the smallest that reach each boundary of weight_grad_bf16_kernel (64-row slabs; the partial rule of g4c_weight_grad,
# whole 32-row units per workgroup):  1 row;  33 = one row into a second 32-row unit (chunk 64, one slab);  65 = one row past a
# 64-row slab (chunk 96: a full slab and a 1-row one);  581 = 3 workgroups of 224 rows (3.5 slabs each: a half-filled last slab in
# every workgroup, and 133 rows = 2 slabs + 5 rows in the last);  98337 = one 64-row slab past 98273, where the partials reach
# their cap of 512 (chunk 224: workgroups past row 98337 get no rows and must write zero tiles).
WG_ROWS = (1, 33, 65, 581, 98337)


def test_partial_rule_at_the_chosen_row_counts():
    lib = _lib.load()
    assert [int(lib.g4c_weight_grad_partials(m)) for m in WG_ROWS] == [1, 1, 1, 3, 512]
    assert int(lib.g4c_weight_grad_partials(98272)) == 511 and int(lib.g4c_weight_grad_partials(98273)) == 512
    assert [MR.weight_grad_chunk(m) for m in WG_ROWS] == [32, 64, 96, 224, 224]
    assert 512 * 224 > 98337 > 439 * 224          # workgroups 440 .. 511 own no rows


@pytest.mark.parametrize("M", WG_ROWS)
def test_weight_grad_bf16_exact(M):
    g = _gen(M)
    v = R.vmax_for(M)
    go, ao = _ints((M, H), v, g), _ints((M, H), v, g)
    ref, rb, aW, ab = MR.weight_bias_grad(go, ao)
    R.check_int_bound(aW, ab)
    with mixed():
        dW, db = A.weight_bias_grad(go, ao)
        dW2, db2 = A.weight_bias_grad(go, ao)
    R.assert_exact(dW, ref, f"dW M={M}")
    R.assert_exact(db, rb, f"db M={M}")
    assert torch.equal(dW, dW2) and torch.equal(db, db2)
    if M > 1:          # negative controls at every size: a dropped row; the last row of the ragged slab
        r = int(torch.nonzero((go.abs().sum(1) * ao.abs().sum(1)) > 0)[M // 2])
        assert R.rejects(R.assert_exact, dW, MR.weight_bias_grad(go, R.drop_row(ao, r))[0])
        assert R.rejects(R.assert_exact, dW, MR.weight_bias_grad(go, R.zero_last_partial_row(ao))[0]) or not bool(
            (go[-1].abs().sum() * ao[-1].abs().sum()) > 0)


@pytest.mark.parametrize("M", WG_ROWS)
def test_weight_grad_bf16_random(M):
    """n_eff: mixed_ref.n_eff_weight_grad (16 rows per MFMA step on one accumulator over the chunk, the two reduction stages).
    Gradient-sized g (1e-7 per element: fp16's subnormal range, bf16 keeps it) in half of the columns."""
    g = _gen(1000 + M)
    go, ao = _randn((M, H), g), _randn((M, H), g, 2.0)
    go[:, 64:] *= 1e-7
    ref, rb, aW, ab = MR.weight_bias_grad(go, ao)
    n_eff = MR.n_eff_weight_grad(M)
    with mixed():
        dW, db = A.weight_bias_grad(go, ao)
        dW2, db2 = A.weight_bias_grad(go, ao)
    R.assert_fp32_class(dW, ref, aW, n_eff, f"dW M={M}")
    R.assert_fp32_class(db, rb, ab, n_eff, f"db M={M}")
    assert torch.equal(dW, dW2) and torch.equal(db, db2)                  # fixed-order reduction: bit-reproducible
    plain, plain_abs = MR.weight_bias_grad_unrounded(go, ao)
    assert R.rejects(R.assert_fp32_class, dW, plain, plain_abs, n_eff, "unrounded product")
    dW0, db0 = A.weight_bias_grad(go, ao)                                 # the default mode is the fp32 MFMA kernel: not this product
    assert R.rejects(R.assert_fp32_class, dW0, ref, aW, n_eff, "default mode against the rounded reference")
    R.assert_fp32_class(dW0, plain, plain_abs, R.n_eff_weight_grad(M), "default mode")


WRAP_CASES = [(3, 128, None), (128, 5, None), (128, 128, 128)]


@pytest.mark.parametrize("N,K,window", WRAP_CASES, ids=["N3", "K5", "window"])
def test_weight_bias_grad_wrapper_shapes(N, K, window):
    """Through autograd.weight_bias_grad at 33 rows: a 3-wide g and a 5-wide a (zero-padded 128-wide copies, _pad128), and a
    128-column window at column 128 of a 384-wide tensor, read in place."""
    M = 33
    g = _gen(N * 7 + K)
    for kind in ("int", "random"):
        v = R.vmax_for(M)
        mk = (lambda s: _ints(s, v, g)) if kind == "int" else (lambda s: _randn(s, g))
        go = mk((M, N))
        if window is None:
            ao = mk((M, K))
        else:
            big = mk((M, 384))
            ao = big[:, window:window + K]
            assert A._pad128(ao, 0, K).data_ptr() == ao.data_ptr()        # a view: the launch reads the window in place
        ref, rb, aW, ab = MR.weight_bias_grad(go, ao)
        with mixed():
            dW, db = A.weight_bias_grad(go, ao)
        assert tuple(dW.shape) == (N, K) and tuple(db.shape) == (N,)
        if kind == "int":
            R.assert_exact(dW, ref, f"dW {N}x{K}")
            R.assert_exact(db, rb, "db")
        else:
            n_eff = MR.n_eff_weight_grad(M)
            R.assert_fp32_class(dW, ref, aW, n_eff, f"dW {N}x{K}")
            R.assert_fp32_class(db, rb, ab, n_eff, "db")
            plain, plain_abs = MR.weight_bias_grad_unrounded(go, ao)
            assert R.rejects(R.assert_fp32_class, dW, plain, plain_abs, n_eff, "unrounded product")


# ====================================================================== save / mul on the rounded-bf16 stream
@pytest.mark.parametrize("M", [1, 33, 4113])
def test_backward_chain_in_the_mode(M, monkeypatch):
    """L = 3.  Layer by layer: D[l] against (rne(D_got[l+1]) rne(W[l])) * slope(acts[l]) — the launch's own saved rows are what its
    next layer rounds — then gX = rne(D_got[1]) rne(W_dense).  Bound C u N_EFF_LAYER_K."""
    L = 3
    g = _gen(L * 1000 + M)
    Ws = [_randn((H, H), g, 1 / 11) for _ in range(L)]
    wd = _randn((H, H), g, 1 / 11)
    acts = [None] + [F.selu(torch.randn(M, H, generator=g)).to(DEV) for _ in range(L - 1)]
    for a in acts[1:]:
        a.view(-1)[:6] = torch.tensor([0.0, -0.0, 2.0 ** -149, -(2.0 ** -149), 1e-30, -1e-30], device=DEV)[:a.numel()]
    gr = _randn((M, H), g)
    calls = _launches(monkeypatch)
    with mixed():
        D, gX = A.backward_chain(gr, Ws, acts, wd)
    assert calls == [("bf16", True, True)]
    assert int(_lib.load().g4c_mlp_last_kernel()) == _lib.KERNEL_MLP_BX6
    D[L] = gr
    for l in range(L - 1, 0, -1):
        ref, absr = MR.chain_layer(D[l + 1], Ws[l], acts[l])
        R.assert_fp32_class(D[l], ref, absr, MR.N_EFF_LAYER, f"chain M={M} D[{l}]")
        plain = R.chain_layer(D[l + 1], Ws[l], acts[l])
        assert R.rejects(R.assert_fp32_class, D[l], plain[0], plain[1], MR.N_EFF_LAYER, "unrounded layer")
    ref, absr = MR.linear(D[1], wd.t())
    R.assert_fp32_class(gX, ref, absr, MR.N_EFF_LAYER, f"chain M={M} gX")
    # negative controls: one slope from the other branch; two k of the contraction swapped
    r = M - 1
    c = int((D[L][r].double() @ Ws[L - 1].double()).abs().argmax())
    bad = MR.chain_layer(D[L], Ws[L - 1], R.flip_slope(acts[L - 1], r, c))
    assert R.rejects(R.assert_fp32_class, D[L - 1], bad[0], bad[1], MR.N_EFF_LAYER, "flipped slope")
    bad = MR.chain_layer(D[L], R.swap_columns(Ws[L - 1].t(), 40).t(), acts[L - 1])
    assert R.rejects(R.assert_fp32_class, D[L - 1], bad[0], bad[1], MR.N_EFF_LAYER, "swapped k")


def _sub(w, n_layers, ln):
    """The state dict of the MLP cut after `n_layers` Linear layers (with or without its LayerNorm)."""
    keep = {k: t for k, t in w.items() if k.startswith("MLP.linear_") and int(k.split("_")[1].split(".")[0]) <= n_layers}
    if ln:
        keep.update({k: t for k, t in w.items() if "layer_norm" in k})
    return keep


@pytest.mark.parametrize("rows", [1, 33, 700])
def test_saving_forward_on_the_rounded_bf16_stream(rows):
    """The `save` rows of a rounded-bf16 launch (the plain tile form: [SELU(e) | v[row] | v[col]] with gathers, three layers,
    LayerNorm, tanh) against oracle.bf16_ref.mlp of the same inputs cut after each layer, at the bound tests/test_gpu_bf16.py uses
    for this launch form ("rows32"); the launch's output against the whole MLP.  The row-split streams keep refusing `save`."""
    n = max(rows // 6, 1)
    g = _gen(rows)
    e, v = _randn((rows, H), g), _randn((n, H), g)
    row, col = (torch.randint(0, n, (rows,), generator=g).to(DEV, torch.int32) for _ in range(2))
    torch.manual_seed(rows)
    m = B.MLP(3 * H, (H, H, H), True)
    with torch.no_grad():
        m.MLP.layer_norm.weight.copy_(1.0 + 0.1 * torch.randn(H))
        m.MLP.layer_norm.bias.copy_(0.1 * torch.randn(H))
    m = m.to(DEV)
    w = {k: t.detach().cpu() for k, t in m.state_dict().items()}
    lins = m._linears()
    Ws, bs = [l.weight.detach() for l in lins], [l.bias.detach() for l in lins]
    ln = (m.MLP.layer_norm.weight.detach(), m.MLP.layer_norm.bias.detach(), 1e-5)
    pk = ops.PackedMLP(Ws, bs, ln, [H, H, H], [False] * 3, precision="bf16")
    saves = [torch.empty(rows, H, device=DEV) for _ in range(3)]
    srcs = [ops.Source(e, pre_act=_lib.ACT_SELU), ops.Source(v, index=row), ops.Source(v, index=col)]
    with torch.no_grad():
        y = ops.mlp_forward(pk, srcs, rows, _lib.ACT_TANH, save=saves)
        assert int(_lib.load().g4c_mlp_last_kernel()) == _lib.KERNEL_MLP_BX6
    blocks = [R16.Block(e, pre_act="selu"), R16.Block(v, index=row), R16.Block(v, index=col)]
    for l in range(2):
        s = R16.assert_bf16_order_noise(saves[l], R16.mlp(_sub(w, l + 1, False), blocks, rows, act="selu"), "rows32", f"save a[{l + 1}]")
        print(f"  save a[{l + 1}] rows={rows}: mean {s['mean']:.3e} max {s['max']:.3e}")
    R16.assert_bf16_order_noise(saves[2], R16.mlp(_sub(w, 3, False), blocks, rows), "rows32", "save z_last")
    R16.assert_bf16_order_noise(y, R16.mlp(w, blocks, rows, act="tanh"), "rows32", "output")
    # negative control: a reference with two weight columns of the first layer swapped is rejected on the first saved layer
    bad = R16.mlp(_sub(w, 1, False), blocks, rows, act="selu", perturb=R16.swap_adjacent_columns)
    assert not R16.check_bf16_order_noise(saves[0], bad, "rows32")[0]
    # the row-split order of the same weights: no saving launch
    pk_rs = ops.PackedMLP([Ws[1], Ws[2]], [bs[1], bs[2]], None, [H], [False], precision="bf16", rs_order=True)
    with torch.no_grad(), pytest.raises(NotImplementedError):
        ops.mlp_forward(pk_rs, [ops.Source(e)], rows, save=[torch.empty(rows, H, device=DEV), None])


@pytest.mark.parametrize("M,k,n_out", [(33, 128, 128), (70000, 256, 128)])
def test_autograd_linear_in_the_mode(M, k, n_out, monkeypatch):
    """[33, 128] x [128, 128] and [70000, 256] x [128, 256] (two input blocks, above FUSED_LINEAR_MIN_ROWS): packed as the
    rounded-bf16 stream; exact on integers, bounded on random operands (n_eff: one 128-k accumulator chain per input block + the
    bias), the unrounded product rejected; the default mode packs the three-way split as before."""
    assert M < A.FUSED_LINEAR_MIN_ROWS or M == 70000
    g = _gen(M + k)
    calls = _launches(monkeypatch)
    v = R.vmax_for(k + 1, cap=8)
    x, W, b = _ints((M, k), v, g), _ints((n_out, k), v, g), _ints((n_out,), v, g)
    with mixed():
        y = A.linear(x, W, b)
    R.assert_exact(y, R.linear(x, W, b)[0], f"linear ints M={M} k={k}")
    assert calls == [("bf16", False, False)]
    x, W, b = _randn((M, k), g), _randn((n_out, k), g, 1 / 11), _randn((n_out,), g)
    x[:, : k // 2] *= 1e-7                                                 # gradient-sized rows
    with mixed():
        y = A.linear(x, W, b)
    n_eff = MR.N_EFF_LAYER * (k // 128) + 1
    ref, absr = MR.linear(x, W, b)
    R.assert_fp32_class(y, ref, absr, n_eff, f"linear M={M} k={k}")
    plain = R.linear(x, W, b)
    assert R.rejects(R.assert_fp32_class, y, plain[0], plain[1], n_eff, "unrounded product")
    bad = MR.linear(x, R.swap_columns(W, k - 28), b)                      # (two k of the full-sized half of the rows)
    assert R.rejects(R.assert_fp32_class, y, bad[0], bad[1], n_eff, "swapped k")
    del calls[:]
    y0 = A.linear(x, W, b)
    assert calls == [("bf16x6", False, False)]
    R.assert_fp32_class(y0, plain[0], plain[1], n_eff + R.N_EFF_SPLIT["bf16x6"], "default mode")


# ====================================================================== end to end
def _step(model, graph, target):
    model.zero_grad(set_to_none=True)
    model.train()
    loss = F.mse_loss(model.forward(graph), target)
    loss.backward()
    return float(loss), {k: p.grad.detach().clone() for k, p in model.named_parameters()}


def _oracle_grads_fp64(name, g_cpu, model, target):
    """The oracle's autograd gradient in fp64 (built as tests/test_gpu_train.py builds its fp32 one)."""
    w = {k: v.detach().cpu().double().clone().requires_grad_(True) for k, v in model.state_dict().items()}
    gd = {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in g_cpu.to_dict().items()}
    F.mse_loss(O.mus_forward(name, gd, w, 3), target.cpu().double()).backward()
    return {k: v.grad for k, v in w.items()}


def _deviation(got, ref):
    return max(float((got[k].cpu().double() - ref[k]).abs().max()) / max(float(ref[k].abs().max()), 1e-300) for k in ref)


# 2 x the worst per-parameter deviation measured on an MI355X over these six cases (tests/MIXED_TRAIN_MEASURED.md); the margin
# covers the seed-to-seed spread of the rounding noise, nothing else
MIXED_GRAD_BOUND = 2 * 1.4493e-01
E2E_CASES = [(name, levels, nodes, seed) for name, levels, nodes in (("NsOneScaleGNN", 1, 2000), ("NsTwoScaleGNN", 2, 3000))
             for seed in (11, 12, 13)]


@pytest.mark.parametrize("name,levels,nodes,seed", E2E_CASES)
def test_training_step_gradient_deviation(name, levels, nodes, seed, monkeypatch):
    """One training step, H = 128: per parameter tensor max|g - g_ref| / max|g_ref| against the oracle's fp64 autograd gradient.
    The mixed step stays within 2 x the worst measured deviation, differs from the default step (the mode engaged: rounded-bf16
    saving forwards, bf16 weight gradients), and the default step still passes today's 2e-3 — before and after the mode was used."""
    g_cpu = S.mus_graph(nodes, levels=levels, seed=seed)
    torch.manual_seed(seed + 1)
    model = getattr(gfd.nn, name)(arch=S.mus_arch(name, H), device=DEV)
    target = torch.randn(nodes, 3, generator=_gen(seed)).to(DEV)
    graph = g_cpu.clone().to(DEV)
    ref = _oracle_grads_fp64(name, g_cpu, model, target)
    assert ops.train_precision() == "bf16x6"
    loss0, g0 = _step(model, graph, target)
    calls = _launches(monkeypatch)
    with mixed(forward=True):
        loss1, g1 = _step(model, graph, target)
    assert calls and not any(p == "bf16x6" for p, _, _ in calls)          # no launch of the step packs the three-way split
    assert any(p == "bf16" and s and not m for p, s, m in calls)          # the recorded forwards save on the rounded-bf16 stream
    loss2, g2 = _step(model, graph, target)
    assert set(g0) == set(g1) == set(ref)
    d0, d1 = _deviation(g0, ref), _deviation(g1, ref)
    per = {k: float((g1[k].cpu().double() - ref[k]).abs().max()) / float(ref[k].abs().max()) for k in ref}
    worst = max(per, key=per.get)
    print(f"[mixed-grad] {name} nodes={nodes} seed={seed}: mixed {d1:.4e} (worst tensor {worst}), default {d0:.4e}, "
          f"loss mixed {loss1:.6e} default {loss0:.6e}")
    assert d0 < 2e-3, d0
    assert any(not torch.equal(g0[k], g1[k]) for k in g0)
    assert loss2 == loss0 and all(torch.equal(g0[k], g2[k]) for k in g0)           # default mode unchanged by having used the mode
    assert d1 <= MIXED_GRAD_BOUND, (d1, MIXED_GRAD_BOUND)


def _dataset(n_graphs, nodes, n_out, seed=0):
    """As tests/test_gpu_train.py: synthetic meshes with a learnable target (the field advanced by a fixed linear map)."""
    data = []
    for i in range(n_graphs):
        g = S.mus_graph(nodes, levels=1, seed=seed + i)
        f, tgt = g.field, []
        for _ in range(n_out):
            f = 0.9 * f + 0.1 * g.glob
            tgt.append(f)
        g.target = torch.cat(tgt, 1)
        data.append(g)
    return data


class _FailingLoader:
    """One good batch, then an error in the middle of the epoch."""

    def __init__(self, loader):
        self.loader = loader

    def __iter__(self):
        it = iter(self.loader)
        yield next(it)
        raise RuntimeError("loader failed")

    def __len__(self):
        return len(self.loader)


def test_fit_with_mixed_precision(tmp_path, capsys):
    """The setting of test_fit_reduces_the_loss_checkpoints_and_resumes (700-node two-scale model) with mixed_precision=True."""
    torch.manual_seed(0)
    model = gfd.nn.NsTwoScaleGNN(arch=S.mus_arch("NsTwoScaleGNN", 32), device=DEV)
    coarsen = gfd.transforms.GridClustering(S.default_cells(700, 2, 2))
    train = gfd.DataLoader(_dataset(4, 700, 2), batch_size=2, shuffle=False, transform=coarsen)
    val = gfd.DataLoader(_dataset(2, 700, 2, seed=50), batch_size=1, transform=coarsen)

    def config(name, epochs):
        return gfd.nn.TrainConfig(name=name, folder=str(tmp_path), epochs=epochs, num_steps=[1, 2], add_steps={'tolerance': 1e9, 'loss': 'training'},
                                  training_loss=gfd.nn.GraphLoss(lambda_d=0.25), validation_loss=gfd.nn.GraphLoss(), lr=2e-3,
                                  grad_clip={'epoch': 0, 'limit': 1.0}, scheduler={'factor': 0.5, 'patience': 2, 'loss': 'validation'},
                                  batch_size=2, mixed_precision=True, device=DEV)
    before = (ops.mlp_precision(), ops.train_precision())
    assert before[1] == "bf16x6" and before[0] != "bf16"
    seen, step0 = [], model.forward

    def spy(*a, **k):
        seen.append((ops.mlp_precision(), ops.train_precision(), torch.is_grad_enabled()))
        return step0(*a, **k)
    model.forward = spy
    model.fit(config("m", 6), train, val)
    del model.forward
    assert (ops.mlp_precision(), ops.train_precision()) == before
    assert seen and all(s[:2] == ("bf16", "bf16") for s in seen) and {s[2] for s in seen} == {True, False}       # training and validation
    out = capsys.readouterr().out
    assert sum(1 for line in out.splitlines() if line.startswith("[fit] mixed_precision")) == 1 and "bf16-rounded operands" in out
    h = model.history
    assert len(h) == 6 and h[-1]['training_loss'] < h[0]['training_loss']
    assert all(math.isfinite(v) for r in h for v in r.values() if isinstance(v, float))
    # the checkpoint is the usual one (no scaler entry) and loads into a default-precision model
    chk = torch.load(os.path.join(tmp_path, "m.chk"), weights_only=False)
    assert 'scaler' not in chk and set(chk) >= {'arch', 'weights', 'optimiser', 'n_out', 'lr', 'epoch', 'scheduler'} and chk['epoch'] == 6
    again = gfd.nn.NsTwoScaleGNN(checkpoint=os.path.join(tmp_path, "m.chk"), device=DEV)
    g = coarsen(_dataset(1, 700, 2, seed=99)[0])
    sol = again.solve(g.clone(), 2)
    assert torch.isfinite(sol).all() and torch.equal(sol, model.solve(g.clone(), 2))
    # a fit that raises restores both switches too
    with pytest.raises(RuntimeError, match="loader failed"):
        model.fit(config("m2", 2), _FailingLoader(train), val)
    assert (ops.mlp_precision(), ops.train_precision()) == before
