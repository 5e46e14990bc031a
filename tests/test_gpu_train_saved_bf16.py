"""bf16 saved activations (`ops.set_train_precision("bf16", saved="bf16")`, `TrainConfig(saved_activations="bf16")`) on the GPU.

The mode is defined exactly — a kept row is `bf16(rne(fp32 row))`, every consumer widens it exactly and does what it did — so every
check but one is `torch.equal`: per launch against the same launch on fp32 rows (the forward against the roundings of its fp32 saves,
the backward kernels against the fp32 kernels fed the widened rows), then whole training steps against today's mixed step with its
kept rows rounded in place (tests/saved_ref.py), the bytes the mode frees, `fit`, and the six cases of tests/MIXED_TRAIN_MEASURED.md
against the oracle's fp64 autograd at the project's MIXED_GRAD_BOUND (measured values: tests/SAVED_BF16_MEASURED.md).

Buffers a launch writes start as a sentinel; rows and columns the launch does not own must still hold it."""
import gc
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pytestmark = pytest.mark.gpu

import graphs4cfd_amd as gfd                                              # noqa: E402
import saved_ref as SR                                                    # noqa: E402
import test_gpu_train_mixed as TM                                         # noqa: E402  (its cases, bound and fp64 oracle step)
from graphs4cfd_amd import _lib, ops, autograd as A, synthetic as S       # noqa: E402
from oracle import grad_ref as R                                          # noqa: E402

DEV = torch.device("cuda", 0)
H = 128
BF16 = torch.bfloat16


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(shape, g, scale=1.0):
    return (torch.randn(shape, generator=g) * scale).to(DEV)


def _sentinel(rows, cols, dtype):
    return torch.full((rows, cols), SR.SENTINEL, dtype=dtype, device=DEV)


def _holds_sentinel(t):
    return bool((t.float() == SR.SENTINEL).all())


# ====================================================================== 1. the saving forward
def _pack(n_layers, ln, g, precision="bf16", k_blocks=1):
    Ws = [_randn((H, H * (k_blocks if l == 0 else 1)), g, 1 / 11) for l in range(n_layers)]
    bs = [_randn((H,), g, 0.3) for _ in range(n_layers)]
    lnp = (1.0 + 0.1 * _randn((H,), g), 0.1 * _randn((H,), g), 1e-5) if ln else None
    return ops.PackedMLP(Ws, bs, lnp, [H] * k_blocks, [False] * k_blocks, precision=precision)


@pytest.mark.parametrize("save_ld", [128, 136])
@pytest.mark.parametrize("n_layers,ln", [(3, True), (2, False)], ids=["L3-LN", "L2"])
@pytest.mark.parametrize("rows", [1, 33, 700])
def test_saving_forward_keeps_the_rounded_rows(rows, n_layers, ln, save_ld):
    """The same launch with fp32 and with bf16 save tensors (three rows of slack below, save_ld - 128 columns beside them): the output
    is bit for bit the same and every bf16 row is the round-to-nearest-even of the fp32 row."""
    g = _gen(rows * 10 + n_layers)
    pk = _pack(n_layers, ln, g, k_blocks=2)
    x, v = _randn((rows, H), g), _randn((max(rows // 5, 1), H), g)
    idx = torch.randint(0, v.size(0), (rows,), generator=g).to(DEV, torch.int32)
    srcs = [ops.Source(x, pre_act=_lib.ACT_SELU), ops.Source(v, index=idx)]
    got = {}
    for dt in (torch.float32, BF16):
        full = [_sentinel(rows + 3, save_ld, dt) for _ in range(n_layers)]
        with torch.no_grad():
            y = ops.mlp_forward(pk, srcs, rows, _lib.ACT_TANH, save=[t[:, :H] for t in full])
        assert int(_lib.load().g4c_mlp_last_kernel()) == _lib.KERNEL_MLP_BX6
        torch.cuda.synchronize()
        for t in full:
            assert _holds_sentinel(t[rows:]) and _holds_sentinel(t[:, H:]), "a row / column the launch does not own was written"
            assert not bool((t[:rows, :H].float() == SR.SENTINEL).any())
        got[dt] = (y, [t[:rows, :H] for t in full])
    assert torch.equal(got[torch.float32][0], got[BF16][0])
    for l in range(n_layers):
        s32, s16 = got[torch.float32][1][l], got[BF16][1][l]
        assert torch.equal(SR.bits(s16), SR.rne_bits(s32.contiguous())), f"save[{l}]"
        assert not torch.equal(SR.widen(s16), s32.contiguous())          # (the fp32 rows do carry more than eight bits)


# ====================================================================== 2. the weight gradient on bf16 rows
@pytest.mark.parametrize("window", [False, True], ids=["ld128", "window256"])
@pytest.mark.parametrize("M", TM.WG_ROWS)
def test_weight_grad_reads_bf16_rows_in_place(M, window):
    """All 128 * 128 + 128 outputs of g4c_weight_grad_bf16_a16 against g4c_weight_grad_bf16 on the widened rows (random operands with
    gradient-sized columns; integer operands, also against the fp64 product), `a` a bf16 tensor of its own and columns 128..255 of a
    256-wide one; then through autograd.weight_bias_grad, which must read the window in place."""
    lib = _lib.load()
    g = _gen(7000 + M)
    scratch = torch.empty(int(lib.g4c_weight_grad_scratch_floats(M)), device=DEV)
    for kind in ("random", "int"):
        if kind == "random":
            go, ao = _randn((M, H), g), _randn((M, 256 if window else H), g, 2.0)
            go[:, 64:] *= 1e-7
        else:
            v = R.vmax_for(M)
            go, ao = R.int_operand((M, H), v, g).to(DEV), R.int_operand((M, 256 if window else H), v, g).to(DEV)
        a16 = ao.to(BF16)
        blk = a16[:, 128:256] if window else a16
        assert blk.data_ptr() % 16 == 0 and blk.stride(0) == (256 if window else 128)
        wide = blk.float().contiguous()
        with SR.train_mode(saved="bf16", forward=False):
            want = A._wgrad_tile(go, wide, M, True, scratch).clone()
            got = A._wgrad_tile(go, blk, M, True, scratch).clone()
            dW, db = A.weight_bias_grad(go, blk)
        assert torch.equal(got, want), f"{kind} M={M}"
        assert torch.equal(dW.reshape(-1), want[:H * H]) and torch.equal(db, want[H * H:])
        if kind == "int":
            R.assert_exact(got[:H * H].view(H, H), go.double().t() @ blk.double(), f"dW M={M}")
            R.assert_exact(got[H * H:], go.double().sum(0), f"db M={M}")
    # in place: the wrapper hands the bf16 window itself to the launch
    seen, f0 = [], A._wgrad_tile

    def spy(g_, blk_, *a):
        seen.append((blk_.dtype, blk_.data_ptr()))
        return f0(g_, blk_, *a)
    A._wgrad_tile = spy
    try:
        with SR.train_mode(saved="bf16", forward=False):
            A.weight_bias_grad(go, blk)
            narrow = A.weight_bias_grad(go, blk[:, :64])          # any other shape: widened, the padded path
        wide_narrow = A.weight_bias_grad(go, blk[:, :64])         # (outside the mode a bf16 operand is widened too: the fp32 MFMA kernel)
    finally:
        A._wgrad_tile = f0
    assert seen[0] == (BF16, blk.data_ptr()) and seen[1][0] == torch.float32 and seen[2][0] == torch.float32
    with SR.train_mode(forward=False):
        assert torch.equal(narrow[0], A.weight_bias_grad(go, blk[:, :64].float())[0])
    assert torch.equal(wide_narrow[0], A.weight_bias_grad(go, blk[:, :64].float())[0])


# ====================================================================== 3. the backward chain with bf16 `mul`
@pytest.mark.parametrize("M", [1, 33, 4113])
def test_backward_chain_takes_bf16_mul(M):
    L = 3
    g = _gen(L * 1000 + M)
    Ws = [_randn((H, H), g, 1 / 11) for _ in range(L)]
    wd = _randn((H, H), g, 1 / 11)
    acts16 = [None] + [F.selu(torch.randn(M, H, generator=g)).to(DEV).to(BF16) for _ in range(L - 1)]
    for a in acts16[1:]:          # both branches of the slope, the zeros, the smallest bf16 values
        a.view(-1)[:6] = torch.tensor([0.0, -0.0, 2.0 ** -133, -(2.0 ** -133), 1e-30, -1e-30], device=DEV)[:a.numel()].to(BF16)
    gr = _randn((M, H), g)
    with SR.train_mode(saved="bf16", forward=False):
        D16, gX16 = A.backward_chain(gr, Ws, acts16, wd)
        assert int(_lib.load().g4c_mlp_last_kernel()) == _lib.KERNEL_MLP_BX6
        D32, gX32 = A.backward_chain(gr, Ws, [None] + [a.float() for a in acts16[1:]], wd)
    assert set(D16) == set(D32) == {1, 2}
    for l in D32:
        assert D16[l].dtype == torch.float32 and torch.equal(D16[l], D32[l]), f"D[{l}] M={M}"
    assert torch.equal(gX16, gX32)
    assert bool((D32[1] != 0).any()) and bool((gX32 != 0).any())


# ====================================================================== 4. activation and LayerNorm adjoints
@pytest.mark.parametrize("width,ld", [(128, 128), (60, 60), (60, 61)], ids=["w128", "w60", "w60-scalar"])
@pytest.mark.parametrize("rows", [1, 5, 1027])
def test_adjoints_widen_bf16_rows(rows, width, ld):
    """g4c_act_grad_ref16 (SELU and tanh, from the output and from the input) and g4c_layernorm_grad_z16 against the fp32 kernels on
    the widened rows.  ld 61: an odd leading dimension, the one-column-per-thread path."""
    g = _gen(rows * 3 + width + ld)
    dy = _randn((rows, width), g)
    ref16 = _randn((rows, ld), g).to(BF16)[:, :width]
    ref16[0, :2] = torch.tensor([0.0, -0.0], device=DEV).to(BF16)
    assert ref16.stride(0) == ld
    ref32 = ref16.float()
    for act in (_lib.ACT_SELU, _lib.ACT_TANH):
        for from_input in (False, True):
            out16, out32 = _sentinel(rows + 2, width + 4, torch.float32), _sentinel(rows + 2, width + 4, torch.float32)
            A.act_grad(dy, ref16, act, from_input, out=out16[:rows, :width])
            A.act_grad(dy, ref32, act, from_input, out=out32[:rows, :width])
            assert torch.equal(out16, out32), (act, from_input)
            assert _holds_sentinel(out16[rows:]) and _holds_sentinel(out16[:, width:])
            assert not bool((out16[:rows, :width] == SR.SENTINEL).any())
    gamma = 1.0 + 0.1 * _randn((width,), g)
    dz16, dg16, db16 = A.layernorm_grad(ref16, gamma, dy, 1e-5)
    dz32, dg32, db32 = A.layernorm_grad(ref32, gamma, dy, 1e-5)
    assert torch.equal(dz16, dz32) and torch.equal(dg16, dg32) and torch.equal(db16, db32)
    assert bool(torch.isfinite(dz32).all())


# ====================================================================== 5. refusals
def test_refusals():
    rows = 33
    g = _gen(5)
    x = _randn((rows, H), g)
    pk16, pk6 = _pack(3, True, g), _pack(3, True, g, precision="bf16x6")

    def run(pk, save, mul=None):
        with torch.no_grad():
            return ops.mlp_forward(pk, [ops.Source(x)], rows, save=save, mul=mul)

    def buf(dt, cols=H):
        return torch.empty((rows, cols), dtype=dt, device=DEV)
    run(pk16, [buf(BF16) for _ in range(3)])                                        # the form itself is fine
    with pytest.raises(ValueError, match="G4C_WFMT_BF16"):                            # the split streams keep fp32 rows
        run(pk6, [buf(BF16) for _ in range(3)])
    with pytest.raises(ValueError, match="G4C_WFMT_BF16"):
        run(pk6, [buf(torch.float32) for _ in range(3)], mul=[buf(BF16), buf(BF16), None])
    with pytest.raises(TypeError, match="one dtype"):                                 # mixed dtypes in one list
        run(pk16, [buf(BF16), buf(torch.float32), buf(BF16)])
    with pytest.raises(TypeError, match="one dtype"):
        run(pk16, [buf(torch.float32) for _ in range(3)], mul=[buf(BF16), buf(torch.float32), None])
    with pytest.raises(TypeError):
        run(pk16, [buf(torch.float16) for _ in range(3)])
    off = [buf(BF16, 136) for _ in range(3)]
    with pytest.raises(ValueError, match="16-byte aligned"):                          # a bf16 window 4 elements in: 8 bytes off
        run(pk16, [t[:, 4:132] for t in off])
    with pytest.raises(ValueError, match="16-byte aligned"):
        run(pk16, [buf(torch.float32) for _ in range(3)], mul=[off[0][:, 4:132], off[1][:, 4:132], None])
    with pytest.raises((ValueError, NotImplementedError), match="multiple of 4"):     # a leading dimension of 130 elements
        run(pk16, [buf(BF16, 130)[:, :H] for _ in range(3)])
    with pytest.raises(ValueError, match="mul_ld"):
        run(pk16, [buf(torch.float32) for _ in range(3)], mul=[buf(BF16, 130)[:, :H], buf(BF16, 130)[:, :H], None])
    # the weight gradient: a misaligned window or an odd leading dimension is not read in place but widened (the result is unchanged)
    go, a16 = _randn((rows, H), g), _randn((rows, 136), g).to(BF16)
    with SR.train_mode(saved="bf16", forward=False):
        for blk in (a16[:, 4:132], _randn((rows, 130), g).to(BF16)[:, :H]):
            assert torch.equal(A.weight_bias_grad(go, blk)[0], A.weight_bias_grad(go, blk.float())[0])
    lib = _lib.load()
    scratch = torch.empty(int(lib.g4c_weight_grad_scratch_floats(rows)), device=DEV)
    out = torch.empty(H * H + H, device=DEV)
    blk = a16[:, 4:132]
    rc = lib.g4c_weight_grad_bf16_a16(go.data_ptr(), H, blk.data_ptr(), 136, rows, scratch.data_ptr(), out.data_ptr(), 1, None)
    assert rc == _lib.EINVAL and "16-byte aligned" in lib.g4c_last_error().decode()


# ====================================================================== whole steps, exact
def _step(model, graph, target):
    model.zero_grad(set_to_none=True)
    model.train()
    loss = F.mse_loss(model.forward(graph), target)
    loss.backward()
    return float(loss), {k: p.grad.detach().clone() for k, p in model.named_parameters()}


def _case(name):
    if name == "REMuS":          # the small REMuS case of tests/test_gpu_train.py
        g_cpu, nf = S.remus_graph(1500, k=5, seed=4), 2
        torch.manual_seed(13)
        model = gfd.nn.NsRotEquiTreeScaleGNN(arch=S.remus_arch(64), device=DEV)
    else:
        levels, nodes = {"NsOneScaleGNN": (1, 2000), "NsTwoScaleGNN": (2, 3000)}[name]
        g_cpu, nf = S.mus_graph(nodes, levels=levels, seed=11), 3
        torch.manual_seed(12)
        model = getattr(gfd.nn, name)(arch=S.mus_arch(name, H), device=DEV)
    target = torch.randn(g_cpu.num_nodes, nf, generator=_gen(11)).to(DEV)
    return model, g_cpu.clone().to(DEV), target


@pytest.mark.parametrize("thresholds", ["shipped", "zero"])
@pytest.mark.parametrize("name", ["NsOneScaleGNN", "NsTwoScaleGNN", "REMuS"])
def test_step_equals_the_mixed_step_on_rounded_rows(name, thresholds, monkeypatch):
    """One step with saved="bf16" against one step in today's mixed mode whose kept rows are rounded in place after every saving
    launch: the loss and every parameter gradient bit-equal — at the shipped thresholds and with FUSED_LINEAR_MIN_ROWS /
    HOIST_MIN_ROWS at 0 (the one-launch chain and the hoisted first layers at this size).  The default and the plain mixed step are
    afterwards what they were before."""
    if thresholds == "zero":
        monkeypatch.setattr(A, "FUSED_LINEAR_MIN_ROWS", 0)
        monkeypatch.setattr(A, "HOIST_MIN_ROWS", 0)
    model, graph, target = _case(name)
    assert (ops.train_precision(), ops.saved_precision()) == ("bf16x6", "fp32")
    loss0, g0 = _step(model, graph, target)
    with SR.train_mode():
        loss_m, g_m = _step(model, graph, target)
        with monkeypatch.context() as mp:
            seen_r = SR.rounding_forward(mp)
            loss_r, g_r = _step(model, graph, target)
    with SR.train_mode(saved="bf16"):
        with monkeypatch.context() as mp:
            seen_s = SR.counting_forward(mp)
            loss_s, g_s = _step(model, graph, target)
    assert seen_s.saving and all(dt == BF16 for _, dt, _ in seen_s.saving)            # the mode engaged: every kept row is bf16
    assert [(r, n) for r, _, n in seen_s.saving] == [(r, n) for r, _, n in seen_r.saving] and all(dt == torch.float32 for _, dt, _ in seen_r.saving)
    assert loss_s == loss_r == loss_m                                                  # the forward is untouched
    assert set(g_s) == set(g_r)
    bad = [k for k in g_r if not torch.equal(g_s[k], g_r[k])]
    assert not bad, bad
    assert any(not torch.equal(g_m[k], g_r[k]) for k in g_r)                          # (the rounding of the rows is visible in the gradients)
    with SR.train_mode():
        loss_m2, g_m2 = _step(model, graph, target)
    loss1, g1 = _step(model, graph, target)
    assert loss_m2 == loss_m and all(torch.equal(g_m[k], g_m2[k]) for k in g_m)
    assert loss1 == loss0 and all(torch.equal(g0[k], g1[k]) for k in g0)


# ====================================================================== against exact arithmetic
@pytest.mark.parametrize("name,levels,nodes,seed", TM.E2E_CASES)
def test_gradient_deviation_from_fp64(name, levels, nodes, seed):
    """The six cases of tests/MIXED_TRAIN_MEASURED.md against the oracle's fp64 autograd, at the project's MIXED_GRAD_BOUND.
    Measured on an MI355X (tests/SAVED_BF16_MEASURED.md): the bf16 rows move the worst deviation by less than its own seed-to-seed spread."""
    g_cpu = S.mus_graph(nodes, levels=levels, seed=seed)
    torch.manual_seed(seed + 1)
    model = getattr(gfd.nn, name)(arch=S.mus_arch(name, H), device=DEV)
    target = torch.randn(nodes, 3, generator=_gen(seed)).to(DEV)
    graph = g_cpu.clone().to(DEV)
    ref = TM._oracle_grads_fp64(name, g_cpu, model, target)
    with SR.train_mode():
        loss_m, g_m = _step(model, graph, target)
    with SR.train_mode(saved="bf16"):
        loss_s, g_s = _step(model, graph, target)
    d_m, d_s = TM._deviation(g_m, ref), TM._deviation(g_s, ref)
    per = {k: float((g_s[k].cpu().double() - ref[k]).abs().max()) / float(ref[k].abs().max()) for k in ref}
    worst = max(per, key=per.get)
    print(f"[saved-bf16-grad] {name} nodes={nodes} seed={seed}: saved-bf16 {d_s:.4e} (worst tensor {worst}), mixed {d_m:.4e}, "
          f"loss {loss_s:.6e}")
    assert loss_s == loss_m
    assert d_s <= TM.MIXED_GRAD_BOUND, (d_s, TM.MIXED_GRAD_BOUND)


# ====================================================================== memory
def test_forward_keeps_half_the_bytes():
    """After a grad-mode forward of NsTwoScaleGNN at 3000 nodes the bytes held fall by rows * 512 - roundup(rows * 256, 512) per kept
    tensor, within 512 bytes per tensor — and by exactly rows * 256 per tensor before the 512-byte rounding.

    The figure is the caching allocator's `requested_bytes` (what the tensors asked for).  `torch.cuda.memory_allocated()` is that plus
    the allocator's own slack: it does not split a cached block of more than 1 MiB when the remainder is 1 MiB or less, so a kept
    tensor can be charged up to 1 MiB more than its size, in either setting.  Measured on an MI355X: requested 440 653 472 -> 282 344 096 B
    (drop 158 309 376 = the unrounded sum, computed with rounding 158 306 304, 84 tensors); memory_allocated 460 844 032 -> 293 678 080 B,
    i.e. 20.2 MB and 11.3 MB of slack.  So memory_allocated is held to the same drop within the slack the allocator itself reports
    (allocated - requested of the two runs), and must fall."""
    model, graph, target = _case("NsTwoScaleGNN")
    model.train()
    keys = ("requested_bytes.all.current", "allocated_bytes.all.current")

    def held(saved):
        with SR.train_mode(saved=saved), pytest.MonkeyPatch.context() as mp:
            seen = SR.counting_forward(mp)
            gc.collect()
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            s0, base = torch.cuda.memory_stats(), torch.cuda.memory_allocated()
            pred = model.forward(graph)
            torch.cuda.synchronize()
            s1, used = torch.cuda.memory_stats(), torch.cuda.memory_allocated() - base
            del pred
        req, alloc = (s1[k] - s0[k] for k in keys)
        assert alloc == used
        return req, used, seen
    held(None), held("bf16")                    # (packed weight images and plans are cached by the first forwards)
    req32, used32, seen32 = held(None)
    req16, used16, seen16 = held("bf16")
    n = seen16.tensors()
    assert n == seen32.tensors() > 0 and all(dt == BF16 for _, dt, _ in seen16.saving) and all(dt == torch.float32 for _, dt, _ in seen32.saving)
    want, exact = seen16.expected_drop(), sum(k * rows * 256 for rows, _, k in seen16.saving)
    slack = (used32 - req32) + (used16 - req16)
    print(f"[saved-bf16-memory] kept tensors {n}: requested fp32 {req32} B, bf16 {req16} B, drop {req32 - req16} B, computed {want} B "
          f"(unrounded {exact} B); memory_allocated fp32 {used32} B, bf16 {used16} B, drop {used32 - used16} B, allocator slack {slack} B")
    assert want > 0 and req32 - req16 == exact
    assert abs((req32 - req16) - want) <= 512 * n, (req32 - req16, want)
    assert used16 < used32 and abs((used32 - used16) - want) <= 512 * n + slack, (used32 - used16, want, slack)


# ====================================================================== fit
def test_fit_with_bf16_saved_activations(tmp_path, capsys):
    """`fit` with saved_activations="bf16" (the 700-node two-scale setting of test_fit_with_mixed_precision): the switches are set
    during the run and restored after a normal return and after an exception inside the loop; the checkpoint is the usual one."""
    torch.manual_seed(0)
    model = gfd.nn.NsTwoScaleGNN(arch=S.mus_arch("NsTwoScaleGNN", 32), device=DEV)
    coarsen = gfd.transforms.GridClustering(S.default_cells(700, 2, 2))
    train = gfd.DataLoader(TM._dataset(4, 700, 2), batch_size=2, shuffle=False, transform=coarsen)

    def config(name, epochs):
        return gfd.nn.TrainConfig(name=name, folder=str(tmp_path), epochs=epochs, num_steps=[1], training_loss=gfd.nn.GraphLoss(lambda_d=0.25),
                                  lr=2e-3, batch_size=2, mixed_precision=True, saved_activations="bf16", device=DEV)
    before = (ops.mlp_precision(), ops.train_precision(), ops.saved_precision())
    assert before[1:] == ("bf16x6", "fp32")
    seen, step0 = [], model.forward

    def spy(*a, **k):
        seen.append((ops.mlp_precision(), ops.train_precision(), ops.saved_precision()))
        return step0(*a, **k)
    model.forward = spy
    model.fit(config("s", 4), train)
    del model.forward
    assert (ops.mlp_precision(), ops.train_precision(), ops.saved_precision()) == before
    assert seen and all(s == ("bf16", "bf16", "bf16") for s in seen)
    out = capsys.readouterr().out
    lines = [line for line in out.splitlines() if line.startswith("[fit] mixed_precision")]
    assert len(lines) == 1 and "saved activations bf16" in lines[0]
    h = model.history
    assert len(h) == 4 and h[-1]['training_loss'] < h[0]['training_loss']
    chk = torch.load(os.path.join(tmp_path, "s.chk"), weights_only=False)
    assert 'scaler' not in chk and set(chk) >= {'arch', 'weights', 'optimiser', 'n_out', 'lr', 'epoch'} and chk['epoch'] == 4
    again = gfd.nn.NsTwoScaleGNN(checkpoint=os.path.join(tmp_path, "s.chk"), device=DEV)          # a default model
    g = coarsen(TM._dataset(1, 700, 2, seed=99)[0])
    sol = again.solve(g.clone(), 2)
    assert torch.isfinite(sol).all() and torch.equal(sol, model.solve(g.clone(), 2))
    with pytest.raises(RuntimeError, match="loader failed"):
        model.fit(config("s2", 2), TM._FailingLoader(train))
    assert (ops.mlp_precision(), ops.train_precision(), ops.saved_precision()) == before
