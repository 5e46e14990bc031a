"""GPU parity of the training path (autograd.py + train_ops.hip) against torch autograd over the oracle's restatement of
the reference blocks (the reference itself differentiates these ops with torch autograd: nn/model.py:232-236).
Tolerances: gradients are sums over up to ~1e5 rows of O(1) terms in fp32 — compared relative to the largest entry of each
gradient tensor (5e-4 of that scale for one block: the backward re-associates the first layer — per-node products gathered and
added instead of one long dot product — so it differs from torch's order at the 1e-4 level), far below anything an optimiser
step can see."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pytestmark = pytest.mark.gpu

import graphs4cfd_amd as gfd                      # noqa: E402
from graphs4cfd_amd import _lib, ops, plan, synthetic as S       # noqa: E402
from graphs4cfd_amd.nn import blocks as B         # noqa: E402
from oracle import g4c_oracle as O                # noqa: E402

DEV = torch.device("cuda", 0)


def close(a, b, rel=5e-4, what=""):
    scale = max(float(b.abs().max()), 1e-6)
    err = float((a - b).abs().max())
    assert err <= rel * scale, f"{what}: max |diff| {err:.3e} vs scale {scale:.3e}"


# ------------------------------------------------------------------ kernels
@pytest.mark.parametrize("act", [_lib.ACT_SELU, _lib.ACT_TANH])
@pytest.mark.parametrize("from_input", [False, True])
def test_act_grad(act, from_input):
    from graphs4cfd_amd import autograd as A
    torch.manual_seed(0)
    x = torch.randn(777, 96, device=DEV, requires_grad=True)
    y = F.selu(x) if act == _lib.ACT_SELU else torch.tanh(x)
    dy = torch.randn_like(y)
    y.backward(dy)
    got = A.act_grad(dy, x.detach() if from_input else y.detach(), act, from_input)
    close(got, x.grad, 1e-5, "act_grad")


@pytest.mark.parametrize("rows,width", [(1, 128), (333, 128), (5000, 32), (70000, 128), (100, 200)])
def test_layernorm_grad_and_colsum(rows, width):
    from graphs4cfd_amd import autograd as A
    torch.manual_seed(1)
    z = (torch.randn(rows, width, device=DEV) * 2 + 0.3).requires_grad_(True)
    gamma = torch.randn(width, device=DEV, requires_grad=True)
    beta = torch.randn(width, device=DEV, requires_grad=True)
    dy = torch.randn(rows, width, device=DEV)
    F.layer_norm(z, (width,), gamma, beta, 1e-5).backward(dy)
    dz, dg, db = A.layernorm_grad(z.detach(), gamma.detach(), dy, 1e-5)
    close(dz, z.grad, 2e-5, "dz")
    close(dg, gamma.grad, 1e-4, "dgamma")
    close(db, beta.grad, 1e-4, "dbeta")
    close(A.colsum(dy), dy.double().sum(0).float(), 1e-5, "colsum")
    # fixed summation order: bit-reproducible
    assert torch.equal(A.colsum(dy), A.colsum(dy))
    assert torch.equal(A.layernorm_grad(z.detach(), gamma.detach(), dy, 1e-5)[1], dg)


def test_segment_reduce_autograd_with_permutation_and_activations():
    torch.manual_seed(2)
    n, n_seg, w = 4000, 700, 128
    key = torch.randint(0, n_seg + 1, (n,))                 # key == n_seg: dropped rows (pool_edge's self loops)
    csr = plan.build_csr(key, n_seg + 1, DEV, drop_last_segment=True)
    src = torch.randn(n, w, device=DEV, requires_grad=True)
    out = ops.segment_reduce(src, csr, True, _lib.ACT_TANH, src_act=_lib.ACT_SELU)
    dy = torch.randn_like(out)
    out.backward(dy)
    ref_src = src.detach().clone().requires_grad_(True)
    keep = (key < n_seg).to(DEV)
    k = key.to(DEV)[keep]
    s = torch.zeros(n_seg, w, device=DEV).index_add_(0, k, F.selu(ref_src)[keep])
    cnt = torch.zeros(n_seg, device=DEV).index_add_(0, k, torch.ones_like(k, dtype=torch.float32)).clamp(min=1)
    ref = torch.tanh(s / cnt[:, None])
    ref.backward(dy)
    close(out.detach(), ref.detach(), 1e-5, "forward")
    close(src.grad, ref_src.grad, 1e-5, "d src")


# ------------------------------------------------------------------ one fused MLP with every kind of input block
def _count_saving_forwards(monkeypatch):
    """Wraps ops.mlp_forward: the returned list receives one entry per launch that saved its activations (`save=` without `mul=`)."""
    calls, f0 = [], ops.mlp_forward

    def fwd(*a, **k):
        if k.get("save") is not None and k.get("mul") is None:
            calls.append(1)
        return f0(*a, **k)
    monkeypatch.setattr(ops, "mlp_forward", fwd)
    return calls


def _expect_saves(saves, save, precision):
    """save=True takes the saving forward in both arithmetics (an f16x3 pack is the bf16x6 kernel family: its `precision` reads
    "bf16x6", autograd._FusedMLP.forward), save=False never does."""
    assert (len(saves) > 0) == save, (len(saves), save, precision)


@pytest.mark.parametrize("save", [True, False])
@pytest.mark.parametrize("hoist_min_rows", [0, 1 << 30])
def test_fused_mlp_gradients_all_source_kinds(hoist_min_rows, save, monkeypatch):
    """hoist_min_rows 0: the gathered block is differentiated on its tensor's rows (autograd.py), 1 << 30: as a dense block.
    save: hidden activations kept by the forward launch (g4c_mlp_io_t.save) / recomputed in the backward pass (default f16x3
    forward)."""
    _fused_mlp_all_source_kinds(hoist_min_rows, save, "f16x3", monkeypatch)


@pytest.mark.parametrize("save", [True, False])
@pytest.mark.parametrize("hoist_min_rows", [0, 1 << 30])
def test_fused_mlp_gradients_all_source_kinds_bf16x6(hoist_min_rows, save, monkeypatch):
    """The same cases with a bf16x6 forward (the bf16x3 weight stream)."""
    _fused_mlp_all_source_kinds(hoist_min_rows, save, "bf16x6", monkeypatch)


def _fused_mlp_all_source_kinds(hoist_min_rows, save, precision, monkeypatch):
    from graphs4cfd_amd import autograd as A
    monkeypatch.setattr(A, "HOIST_MIN_ROWS", hoist_min_rows)
    monkeypatch.setattr(A, "SAVE_ACTIVATIONS", save)
    monkeypatch.setattr(ops, "_PRECISION", precision)
    saves = _count_saving_forwards(monkeypatch)
    torch.manual_seed(3)
    M, n_a, n_b, H = 3000, 500, 3000, 128
    mlp = B.MLP(2 + H + H + 3, (H, H, H), True).to(DEV)
    rel = torch.randn(M, 2, device=DEV, requires_grad=True)                       # narrow, negated
    a = torch.randn(n_a, H, device=DEV, requires_grad=True)                       # gathered through an index, activated on load
    b = torch.randn(n_b, H + 5, device=DEV, requires_grad=True)                   # column window of a wider tensor
    c = torch.randn(M, 3, device=DEV, requires_grad=True)
    idx = torch.randint(0, n_a, (M,), device=DEV)
    resid = torch.randn(M, H + 2, device=DEV, requires_grad=True)
    srcs = [ops.Source(rel, negate=True), ops.Source(a, plan.index32(idx), pre_act=_lib.ACT_SELU),
            ops.Source(b, col0=5, width=H), ops.Source(c)]
    y = mlp.run(srcs, M, activation=torch.tanh, resid=resid, resid_col0=2)
    _expect_saves(saves, save, precision)
    dy = torch.randn_like(y)
    y.backward(dy)
    got = {n: p.grad.clone() for n, p in mlp.named_parameters()}
    got_in = [t.grad.clone() for t in (rel, a, b, c, resid)]
    for p in mlp.parameters():
        p.grad = None
    ins = [t.detach().clone().requires_grad_(True) for t in (rel, a, b, c, resid)]
    x = torch.cat((-ins[0], F.selu(ins[1])[idx], ins[2][:, 5:5 + H], ins[3]), 1)
    ref = torch.tanh(mlp.MLP(x)) + ins[4][:, 2:2 + H]
    close(y.detach(), ref.detach(), 1e-4, "forward")
    ref.backward(dy)
    for n, p in mlp.named_parameters():
        close(got[n], p.grad, what=n)
    for name, g, t in zip(("rel", "a", "b", "c", "resid"), got_in, ins):
        close(g, t.grad, what=name)


@pytest.mark.parametrize("activation", [None, "selu", torch.tanh])
def test_gnblock_public_forward_gradients(activation, monkeypatch):
    """GNBlock.forward(v, e, edge_index) (nn/blocks.py:175-186) under autograd: gradients of both outputs with respect to
    v, e and every parameter (first layer differentiated on the node rows: hoisting forced on at this small size)."""
    from graphs4cfd_amd import autograd as A
    monkeypatch.setattr(A, "HOIST_MIN_ROWS", 0)
    monkeypatch.setattr(A, "FUSED_LINEAR_MIN_ROWS", 0)
    torch.manual_seed(5)
    n, H = 1500, 128
    g = S.mus_graph(n, levels=1, seed=9)
    ei = g.edge_index.to(DEV)
    blk = B.GNBlock((3 * H, (H, H, H), True), (2 * H, (H, H, H), True)).to(DEV)
    v = torch.randn(n, H, device=DEV, requires_grad=True)
    e = torch.randn(ei.size(1), H, device=DEV, requires_grad=True)
    v1, e1 = blk.forward(v, e, ei, activation=activation)
    dv, de = torch.randn_like(v1), torch.randn_like(e1)
    torch.autograd.backward([v1, e1], [dv, de])
    got = {k: p.grad.clone() for k, p in blk.named_parameters()}
    got_v, got_e = v.grad.clone(), e.grad.clone()
    # reference: the same block in float64 under torch autograd (torch's own fp32 autograd on the GPU is itself up to 1e-2 of
    # the largest entry away from float64 on this case — atomics + cancellation — while the HIP path is at 5e-7)
    f = {None: lambda x: x, "selu": F.selu, torch.tanh: torch.tanh}[activation]
    ref_blk = B.GNBlock((3 * H, (H, H, H), True), (2 * H, (H, H, H), True)).to(DEV).double()
    ref_blk.load_state_dict({k: p.double() for k, p in blk.state_dict().items()})
    v2, e2 = v.detach().double().requires_grad_(True), e.detach().double().requires_grad_(True)
    row, col = ei
    e_ref = ref_blk.edge_mlp.MLP(torch.cat((e2, v2[row], v2[col]), 1))
    agg = torch.zeros(n, H, device=DEV, dtype=torch.float64).index_add_(0, col, e_ref)
    cnt = torch.zeros(n, device=DEV, dtype=torch.float64).index_add_(0, col, torch.ones(col.numel(), device=DEV, dtype=torch.float64)).clamp(min=1)
    v_ref = ref_blk.node_mlp.MLP(torch.cat((agg / cnt[:, None], v2), 1))
    torch.autograd.backward([f(v_ref), f(e_ref)], [dv.double(), de.double()])
    close(v1.detach().double(), f(v_ref).detach(), 1e-5, "v'")
    close(e1.detach().double(), f(e_ref).detach(), 1e-5, "e'")
    close(got_v.double(), v2.grad, 2e-5, "dv")
    close(got_e.double(), e2.grad, 2e-5, "de")
    for k, p in ref_blk.named_parameters():
        close(got[k].double(), p.grad, 2e-5, k)


def _model_and_oracle_grads(model_name, levels, nodes, hidden, seed):
    adv = model_name.startswith("Adv")            # advection models: one field, `loc` among the node inputs
    nf = 1 if adv else 3
    g = S.mus_graph(nodes, levels=levels, seed=seed, nf=nf, loc=adv)
    torch.manual_seed(seed + 1)
    model = getattr(gfd.nn, model_name)(arch=S.mus_arch(model_name, hidden, nf=nf, node_in=nf + 2 + (2 if adv else 0)), device=DEV)
    target = torch.randn(nodes, nf, device=DEV)
    gd = g.clone().to(DEV)
    model.train()
    pred = model.forward(gd)
    loss = F.mse_loss(pred, target)
    loss.backward()
    got = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    w = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in model.state_dict().items()}
    pred_ref = O.mus_forward(model_name, g.to_dict(), w, nf)
    loss_ref = F.mse_loss(pred_ref, target.cpu())
    loss_ref.backward()
    return model, float(loss), float(loss_ref), got, {k: v.grad for k, v in w.items()}


MODEL_CASES = [("NsOneScaleGNN", 1, 128), ("NsThreeScaleGNN", 3, 128), ("NsTwoScaleGNN", 2, 32), ("NsFourScaleGNN", 4, 64),
               ("AdvThreeScaleGNN", 3, 128)]


@pytest.mark.parametrize("save", [True, False])
@pytest.mark.parametrize("model_name,levels,hidden", MODEL_CASES)
def test_model_parameter_gradients_match_oracle_autograd(model_name, levels, hidden, save, monkeypatch):
    """Default (f16x3) forward; save=True keeps the forward's activations, save=False recomputes them."""
    _model_parameter_gradients(model_name, levels, hidden, save, "f16x3", monkeypatch)


@pytest.mark.parametrize("save", [True, False])
@pytest.mark.parametrize("model_name,levels,hidden", MODEL_CASES)
def test_model_parameter_gradients_match_oracle_autograd_bf16x6(model_name, levels, hidden, save, monkeypatch):
    """The same models with a bf16x6 forward (the bf16x3 weight stream)."""
    _model_parameter_gradients(model_name, levels, hidden, save, "bf16x6", monkeypatch)


def _model_parameter_gradients(model_name, levels, hidden, save, precision, monkeypatch):
    from graphs4cfd_amd import autograd as A
    monkeypatch.setattr(A, "SAVE_ACTIVATIONS", save)
    monkeypatch.setattr(ops, "_PRECISION", precision)
    if save:       # also the large-launch forms at this small size: single-layer products and the one-launch backward chain
        monkeypatch.setattr(A, "FUSED_LINEAR_MIN_ROWS", 0)
        monkeypatch.setattr(A, "HOIST_MIN_ROWS", 0)
    saves = _count_saving_forwards(monkeypatch)
    model, loss, loss_ref, got, ref = _model_and_oracle_grads(model_name, levels, 2500, hidden, 7)
    _expect_saves(saves, save, precision)
    assert abs(loss - loss_ref) <= 1e-4 * max(1.0, abs(loss_ref))
    assert set(got) == set(ref)
    worst = 0.0
    for k in ref:
        scale = max(float(ref[k].abs().max()), 1e-7)
        worst = max(worst, float((got[k].cpu() - ref[k]).abs().max()) / scale)
    assert worst < 2e-3, worst


def test_training_step_is_bit_reproducible_and_rollout_still_matches():
    """Deterministic reductions: two backward passes give identical gradients; and the inference path (hoisting, heads,
    hipGraph) of the same model is unaffected by having trained (packed weights follow the parameter versions)."""
    g_cpu = S.mus_graph(3000, levels=2, seed=3)
    g = g_cpu.clone().to(DEV)
    torch.manual_seed(4)
    model = gfd.nn.NsTwoScaleGNN(arch=S.mus_arch("NsTwoScaleGNN", 128), device=DEV)
    target = torch.randn(3000, 3, device=DEV)
    grads = []
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        F.mse_loss(model.forward(g), target).backward()
        grads.append([p.grad.clone() for p in model.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*grads))
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    opt.step()
    with torch.no_grad():
        a = model.forward(g)
    w = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    with torch.no_grad():
        ref = O.mus_forward("NsTwoScaleGNN", g_cpu.to_dict(), w, 3)
    torch.testing.assert_close(a.cpu(), ref, rtol=5e-4, atol=5e-4)


def test_training_steps_against_reference_golden():
    """The HIP training path against the REFERENCE's recorded loss / gradients (tests/golden/training.pt: its own train-mode
    forward, GraphLoss with the Dirichlet term, backward; second step on the fed-back prediction)."""
    c = torch.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "training.pt"), weights_only=False)
    model = gfd.nn.NsThreeScaleGNN(arch=c["arch"], device=DEV)
    model.load_state_dict(c["weights"])
    g = gfd.Graph(**c["graph"]).to(DEV)
    crit = gfd.nn.GraphLoss(lambda_d=c["lambda_d"])
    model.train()
    pred = None
    for t, ref in enumerate(c["steps"]):
        if t > 0:
            g.field = model.shift_and_replace(g.field, pred.detach())
        model.zero_grad()
        pred = model.forward(g, t)
        loss = crit(g, pred, g.target[:, 3 * t:3 * (t + 1)])
        loss.backward()
        assert abs(float(loss) - float(ref["loss"])) <= 1e-4 * float(ref["loss"])
        close(pred.detach().cpu(), ref["pred"], 5e-4, "prediction")
        for k, p in model.named_parameters():
            close(p.grad.cpu(), ref["grads"][k], 2e-3, k)
        assert abs(model.grad_norm2() - ref["grad_norm2"]) <= 1e-3 * ref["grad_norm2"]


# ------------------------------------------------------------------ the training loop (nn/model.py:152-301)
def _dataset(n_graphs, nodes, n_out, seed=0):
    """A list of synthetic meshes with a smooth target: `target[:, 3t:3t+3]` = the field advanced t+1 times by a fixed
    linear map of (field, glob) — learnable, so the loss must fall."""
    data = []
    for i in range(n_graphs):
        g = S.mus_graph(nodes, levels=1, seed=seed + i)     # level-1 edges only: the coarse levels are a batch-level transform
        f, tgt = g.field, []
        for _ in range(n_out):
            f = 0.9 * f + 0.1 * g.glob
            tgt.append(f)
        g.target = torch.cat(tgt, 1)
        data.append(g)
    return data


def test_fit_reduces_the_loss_checkpoints_and_resumes(tmp_path, capsys):
    torch.manual_seed(0)
    model = gfd.nn.NsTwoScaleGNN(arch=S.mus_arch("NsTwoScaleGNN", 32), device=DEV)
    # as in the reference's examples (examples/training/NsMuSGNN/*.py): GridClustering runs on the collated batch
    coarsen = gfd.transforms.GridClustering(S.default_cells(700, 2, 2))
    train = gfd.DataLoader(_dataset(4, 700, 2), batch_size=2, shuffle=False, transform=coarsen)
    val = gfd.DataLoader(_dataset(2, 700, 2, seed=50), batch_size=1, transform=coarsen)
    cfg = gfd.nn.TrainConfig(name="m", folder=str(tmp_path), epochs=6, num_steps=[1, 2], add_steps={'tolerance': 1e9, 'loss': 'training'},
                             training_loss=gfd.nn.GraphLoss(lambda_d=0.25), validation_loss=gfd.nn.GraphLoss(), lr=2e-3,
                             grad_clip={'epoch': 0, 'limit': 1.0}, scheduler={'factor': 0.5, 'patience': 2, 'loss': 'validation'},
                             batch_size=2, device=DEV)
    model.fit(cfg, train, val)
    h = model.history
    assert [r['n_out'] for r in h] == [1, 2, 2, 2, 2, 2]           # tolerance passed after the first epoch: longer rollouts
    assert h[-1]['training_loss'] < 0.6 * h[1]['training_loss']
    assert h[-1]['validation_loss'] < h[1]['validation_loss']
    assert all(r['gradients_norm'] > 0 for r in h)
    chk = torch.load(os.path.join(tmp_path, "m.chk"), weights_only=False)
    assert set(chk) >= {'arch', 'weights', 'optimiser', 'n_out', 'lr', 'epoch', 'scheduler'} and chk['epoch'] == 6 and chk['n_out'] == 2
    # the checkpoint is a model file of the reference's format ...
    again = gfd.nn.NsTwoScaleGNN(checkpoint=os.path.join(tmp_path, "m.chk"), device=DEV)
    g = coarsen(_dataset(1, 700, 2, seed=99)[0])
    assert torch.equal(again.solve(g.clone(), 2), model.solve(g.clone(), 2))
    # ... and training resumes from it (epoch 7 only)
    cfg2 = gfd.nn.TrainConfig(name="m2", folder=str(tmp_path), checkpoint=os.path.join(tmp_path, "m.chk"), epochs=7, num_steps=[1, 2],
                              training_loss=gfd.nn.GraphLoss(), lr=2e-3, device=DEV)
    again.fit(cfg2, train)
    assert [r['epoch'] for r in again.history] == [7] and again.history[0]['n_out'] == 2
    assert again.history[0]['training_loss'] < h[1]['training_loss']


def _f64(graph_dict):
    return {k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in graph_dict.items()}


def _grad_parity(model, pred, target, ref_fn, tol=2e-3):
    """Gradients against the oracle evaluated in float64 (torch autograd over the restatement): for these deeper models the
    fp32 oracle itself sits 2-3e-3 from float64 (measured: REMuS worst 3.4e-3), the HIP path 6e-4."""
    loss = F.mse_loss(pred, target)
    loss.backward()
    got = {k: p.grad.detach().cpu().double() for k, p in model.named_parameters()}
    w = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.state_dict().items()}
    pred_ref = ref_fn(w)
    close(pred.detach().cpu().double(), pred_ref.detach(), 5e-4, "forward")
    F.mse_loss(pred_ref, target.cpu().double()).backward()
    assert set(got) == set(w) and all(v.grad is not None for v in w.values())
    worst = max(float((got[k] - w[k].grad).abs().max()) / max(float(w[k].grad.abs().max()), 1e-12) for k in w)
    assert worst < tol, worst


@pytest.mark.parametrize("cls,levels", [("NsTwoGuillardScaleGNN", 2), ("NsThreeGuillardScaleGNN", 3)])
def test_gmus_parameter_gradients_match_oracle_autograd(cls, levels):
    """gMuS-GNN (nn/mugs_gnn.py): restriction = row gather, knn_interpolate, 2H-wide node latents after each up-sampling."""
    g = S.mugs_graph(2500 if levels == 2 else 3000, levels=levels, seed=11)
    torch.manual_seed(12)
    model = getattr(gfd.nn, cls)(arch=S.mugs_arch(cls, 64), device=DEV)
    target = torch.randn(g.num_nodes, 3, device=DEV)
    pred = model.forward(g.clone().to(DEV))
    _grad_parity(model, pred, target, lambda w: O.mugs_forward(cls, _f64(g.to_dict()), w, 3))


def test_remus_parameter_gradients_match_oracle_autograd():
    """REMuS-GNN (nn/remus_gnn.py:119-199): EdgeMP / DownEdgeMP / UpEdgeMP (edge scalars -> node vectors, interpolation with a
    masked write, projection on the edges), decoder through edgeScalarToNodeVector, residual on the last two fields."""
    g = S.remus_graph(1500, k=5, seed=4)
    torch.manual_seed(13)
    model = gfd.nn.NsRotEquiTreeScaleGNN(arch=S.remus_arch(64), device=DEV)
    target = torch.randn(g.num_nodes, 2, device=DEV)
    pred = model.forward(g.clone().to(DEV))
    _grad_parity(model, pred, target, lambda w: O.remus_forward(_f64(g.to_dict()), w))


@pytest.mark.parametrize("rows,k", [(4096, 128), (33333, 128), (70001, 256), (600000, 128)])
def test_weight_grad_kernel(rows, k):
    """g4c_weight_grad: dW = g^T a and db = column sums of g in one pass, against float64; bit-reproducible."""
    from graphs4cfd_amd import autograd as A
    torch.manual_seed(rows)
    g = torch.randn(rows, 128, device=DEV)
    wide = torch.randn(rows, k + 4, device=DEV)
    a = wide[:, 4:]                                       # a 16-byte aligned column window of a wider tensor
    dW, db = A.weight_bias_grad(g, a)
    ref = (g.double().t() @ a.double())
    close(dW.double(), ref, 2e-6, "dW")
    close(db.double(), g.double().sum(0), 2e-6, "db")
    dW2, db2 = A.weight_bias_grad(g, a)
    assert torch.equal(dW, dW2) and torch.equal(db, db2)


def test_plans_use_registered_host_images_and_drop_stale_ones():
    """Graph.to(device) registers the host image of index tensors (plan.remember_host): plan builders then never read them
    back; an image whose source CPU tensor was modified in place afterwards is ignored (the device tensor is read back)."""
    g = S.mus_graph(900, levels=2, seed=31)
    ei_cpu = g.edge_index
    gd = g.to(DEV)
    assert plan._host_image(gd.edge_index) is not None
    ep, csr = plan.edge_csr(gd.edge_index, 900)
    assert plan._host_image(ep.row) is not None and plan._host_image(csr.off) is not None
    ref = plan.build_csr(gd.edge_index[1].cpu(), 900, DEV)
    assert torch.equal(csr.off, ref.off)
    ei_cpu += 1                                            # in-place change of the source tensor: image is stale now
    assert plan._host_image(gd.edge_index) is None
    plan.clear_caches()
    ep2, csr2 = plan.edge_csr(gd.edge_index, 900)          # falls back to reading the device tensor
    assert torch.equal(csr2.off, ref.off)


def test_packed_weights_follow_an_optimizer_that_does_not_bump_versions():
    """torch's fused optimizers update parameters without advancing their version counters; the packed-weight cache must not
    serve the old image afterwards (ops.weights_epoch)."""
    g = S.mus_graph(1200, levels=1, seed=41).to(DEV)
    torch.manual_seed(42)
    model = gfd.nn.NsOneScaleGNN(arch=S.mus_arch("NsOneScaleGNN", 32), device=DEV)
    opt = torch.optim.Adam(model.parameters(), lr=1e-2, fused=True)
    target = torch.randn(1200, 3, device=DEV)
    for _ in range(2):
        F.mse_loss(model.forward(g), target).backward()
        v0 = next(model.parameters())._version
        opt.step(); opt.zero_grad()
    with torch.no_grad():
        got = model.forward(g)
    w = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    gc = S.mus_graph(1200, levels=1, seed=41)
    with torch.no_grad():
        ref = O.mus_forward("NsOneScaleGNN", gc.to_dict(), w, 3)
    torch.testing.assert_close(got.cpu(), ref, rtol=5e-4, atol=5e-4)


def test_remus_batch_through_collater_equals_individual_graphs_and_fit_runs(tmp_path):
    """A collated REMuS batch (node-, edge- and cross-level-indexed attributes offset by the Collater) gives every graph the
    prediction it gets alone; `fit` over such batches runs and lowers the loss."""
    graphs = [S.remus_graph(900 + 100 * i, k=5, seed=80 + i) for i in range(2)]
    torch.manual_seed(81)
    model = gfd.nn.NsRotEquiTreeScaleGNN(arch=S.remus_arch(32), device=DEV)
    with torch.no_grad():
        alone = [model.forward(g.clone().to(DEV)) for g in graphs]
        both = model.forward(gfd.Collater(gfd.transforms.BuildKnnInterpWeights(5))(graphs).to(DEV))
    torch.testing.assert_close(both, torch.cat(alone), rtol=1e-4, atol=1e-4)
    for g in graphs:
        g.target = 0.5 * g.field[:, -2:]
    cfg = gfd.nn.TrainConfig(name="r", folder=str(tmp_path), epochs=5, num_steps=[1], training_loss=gfd.nn.GraphLoss(), lr=2e-3, device=DEV)
    model.fit(cfg, gfd.DataLoader(graphs, batch_size=2, transform=gfd.transforms.BuildKnnInterpWeights(5)))
    assert model.history[-1]['training_loss'] < model.history[0]['training_loss']


def test_gmus_batch_through_collater_equals_individual_graphs():
    """gMuS-GNN batches as in examples/training/NsMuGSGNN/*.py:42-48 (BuildKnnInterpWeights as the batch transform)."""
    graphs = [S.mugs_graph(1500 + 200 * i, levels=3, seed=85 + i) for i in range(2)]
    torch.manual_seed(86)
    model = gfd.nn.NsThreeGuillardScaleGNN(arch=S.mugs_arch("NsThreeGuillardScaleGNN", 32), device=DEV)
    with torch.no_grad():
        alone = [model.forward(g.clone().to(DEV)) for g in graphs]
        both = model.forward(gfd.Collater(gfd.transforms.BuildKnnInterpWeights(6))(graphs).to(DEV))
    torch.testing.assert_close(both, torch.cat(alone), rtol=1e-4, atol=1e-4)


def test_training_in_fp32_mfma_mode(monkeypatch):
    """`gfd.set_mlp_precision("fp32")`: the forward runs the fp32-MFMA kernels (no activation saving there: the backward
    recomputes), gradients still match the oracle."""
    old = ops.mlp_precision()
    ops.set_mlp_precision("fp32")
    try:
        model, loss, loss_ref, got, ref = _model_and_oracle_grads("NsTwoScaleGNN", 2, 2500, 128, 17)
    finally:
        ops.set_mlp_precision(old)
    assert abs(loss - loss_ref) <= 1e-4 * max(1.0, abs(loss_ref))
    worst = max(float((got[k].cpu() - ref[k]).abs().max()) / max(float(ref[k].abs().max()), 1e-7) for k in ref)
    assert worst < 2e-3, worst


# ------------------------------------------------------------------ MLPs outside the one-launch envelope
@pytest.mark.parametrize("shape", [(8, (256, 16), False), (300, (200, 300, 64), True), (128, (128,) * 6, True), (8, (16, 256), True),
                                   (8, (1024, 16), False), (600, (700, 48), True)],
                         ids=["wide-hidden", "wide-in-and-hidden", "six-layers", "wide-layernorm", "hidden-over-512", "wide-in-over-512"])
def test_mlp_any_widths_and_depth_gradients(shape):
    """The same launch chains recorded for autograd (gradients enabled is torch's default, so a bare `mlp(x)` takes this path): output,
    input gradient and every parameter gradient against float64 autograd over the module's own torch layers."""
    k_in, widths, ln = shape
    torch.manual_seed(sum(widths) + 1)
    mlp = B.MLP(k_in, widths, ln).to(DEV)
    assert not mlp.fits_one_launch()
    x = torch.randn(3000, k_in, device=DEV, requires_grad=True)
    t = torch.randn(3000, widths[-1], device=DEV)
    y = mlp(x)
    (y * t).sum().backward()
    got = {"x": x.grad.clone(), **{k: p.grad.clone() for k, p in mlp.named_parameters()}}
    mlp.zero_grad(); x.grad = None
    ref_net = mlp.MLP.double()
    xd = x.detach().double().requires_grad_(True)
    yd = ref_net(xd)
    (yd * t.double()).sum().backward()
    ref = {"x": xd.grad.float(), **{"MLP." + k: p.grad.float() for k, p in ref_net.named_parameters()}}
    mlp.MLP.float()
    torch.testing.assert_close(y.detach(), yd.detach().float(), rtol=1e-4, atol=1e-4)
    # (a hidden pre-activation within rounding of 0 sits on SELU's kink — slope 1.76 on one side, 1.05 on the other — and the fp32 and
    # fp64 paths may take different sides: isolated rows of a gradient then differ by a percent.  Hence the error in norm.)
    for k in ref:
        err = (got[k] - ref[k]).norm()
        assert float(err) <= 2e-3 * float(ref[k].norm()) + 1e-30, (k, float(err), float(ref[k].norm()))
