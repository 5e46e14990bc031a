"""The differentiable mesh operator and `gfd.nn.FlowLoss` on the device: `MeshGradient.derived` of an x that requires grad is recorded
(its backward is the adjoint launch, bit for bit), FlowLoss's gradient against the fp64 formula of tests/adjoint_op_ref.py
(∂GraphLoss + Σ (2 w / (N nd_name)) Dᵀ D (pred − ref), within the allowance derived at `FlowRef.grad`) and against a central
difference of the fp64 loss, its operator cache, and a two-epoch `fit`.  The worst measured / allowed ratios are printed by the last
test (tests/FLOW_LOSS_MEASURED.md)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

import adjoint_op_ref as A                               # noqa: E402
import gradient_ref as R                                 # noqa: E402
import graphs4cfd_amd as gfd                             # noqa: E402
from graphs4cfd_amd import synthetic as S                # noqa: E402

DEV = torch.device("cuda", 0)
RATIOS = {}


def note(name, r):
    RATIOS[name] = max(RATIOS.get(name, 0.0), float(r))


def bits(t):
    return t.detach().contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def mesh_of(dim):
    return R.ragged_mesh(300, dim).shuffled(11)


def graph_of(m, seed=0):
    g = gfd.Graph(pos=torch.from_numpy(m.pos).float(), edge_index=torch.from_numpy(np.stack([m.row, m.col])))
    g.rel = torch.from_numpy(m.rel)
    omega = torch.zeros(m.n, 2)
    omega[torch.randperm(m.n, generator=torch.Generator().manual_seed(seed))[:40], 0] = 1          # 40 Dirichlet nodes
    g.omega = omega
    return g.to(DEV)


def fields(m, seed, nf=3):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((m.n, nf)).astype(np.float32), rng.standard_normal((m.n, nf)).astype(np.float32)


# ====================================================================== derived() under autograd
@pytest.mark.parametrize("dim", [2, 3])
def test_derived_is_recorded_and_its_backward_is_the_adjoint(dim):
    m = mesh_of(dim)
    op = gfd.MeshGradient(graph_of(m), edge_vectors=graph_of(m).rel)
    names = ("div", "vort", "grad:2") if dim == 2 else ("div", "vort")
    x0 = torch.from_numpy(fields(m, 3)[0]).to(DEV)
    plain = op.derived(x0, names)
    assert plain.grad_fn is None and not plain.requires_grad and op._adjoint_tables is None
    x = x0.clone().requires_grad_(True)
    with torch.no_grad():
        assert op.derived(x, names).grad_fn is None
    y = op.derived(x, names)
    assert y.grad_fn is not None and y.requires_grad and torch.equal(bits(y), bits(plain))          # the same launch: the same bits
    nd = int(y.size(1))
    # .sum(): autograd hands over a stride-0 expanded tensor of ones
    (gx,) = torch.autograd.grad(y.sum(), x, retain_graph=True)
    assert torch.equal(bits(gx), bits(op.adjoint(torch.ones(m.n, nd, device=DEV), names, 3)))
    # a column slice: a dense gy that is zero outside the slice
    w = torch.from_numpy(np.random.default_rng(4).standard_normal((m.n, 1)).astype(np.float32)).to(DEV)
    (gx,) = torch.autograd.grad((y[:, 1:2] * w).sum(), x, retain_graph=True)
    gy = torch.zeros(m.n, nd, device=DEV)
    gy[:, 1:2] = w
    assert torch.equal(bits(gx), bits(op.adjoint(gy, names, 3)))
    # gradient() goes through derived(): recorded as well, and a field nobody differentiates gets exact zeros
    x2 = x0.clone().requires_grad_(True)
    grad = op.gradient(x2)
    assert grad.grad_fn is not None and torch.equal(bits(grad), bits(op.gradient(x0)))
    (gx,) = torch.autograd.grad(grad[:, 1].sum(), x2)
    assert not bits(gx[:, [0, 2]]).any() and bool(gx[:, 1].any())
    with pytest.raises(RuntimeError):          # once_differentiable: no double backward
        (g1,) = torch.autograd.grad(op.derived(x, names).sum(), x, create_graph=True)
        g1.sum().backward()


# ====================================================================== FlowLoss against the fp64 formula
TERMS = {"div": 0.1, "vort": 0.05, "grad:2": 0.01}


def reference(op, m, dim, lambda_d, mask):
    """FlowRef for TERMS with zero=("div",): one call on pred − target (vort, grad:2), one on pred (div), from the DEVICE's weights
    (pinned against the restatement by tests/test_gpu_mesh_gradient.py)."""
    g_dev, src = op.g.cpu().numpy(), op.src.cpu().numpy()
    nv = 1 if dim == 2 else 3
    groups = [(R.program(("vort", "grad:2"), dim, 3), [(TERMS["vort"], 0, nv), (TERMS["grad:2"], nv, nv + dim)], False),
              (R.program(("div",), dim, 3), [(TERMS["div"], 0, 1)], True)]
    return A.FlowRef(m.off, g_dev, src, m.max_deg, groups, lambda_d, mask)


@pytest.mark.parametrize("dim", [2, 3])
def test_flow_loss_gradient_against_the_fp64_formula(dim):
    m = mesh_of(dim)
    graph = graph_of(m)
    p, t = fields(m, 10 + dim)
    target = torch.from_numpy(t).to(DEV)
    mask = (graph.omega[:, 0] == 1).cpu().numpy()
    for lambda_d in (0.25, 0):
        crit = gfd.nn.FlowLoss(lambda_d, TERMS, zero=("div",), edge_vectors="rel")
        pred = torch.from_numpy(p).to(DEV).requires_grad_(True)
        loss = crit(graph, pred, target)
        (got,) = torch.autograd.grad(loss, pred)
        ref = reference(crit.operator(graph), m, dim, lambda_d, mask)
        want, allowed = ref.grad(p, t)
        note("FlowLoss: |grad - fp64| / allowed", R.within(got, want, allowed, f"dim {dim} lambda_d {lambda_d}"))
        value = ref.loss(p.astype(np.float64), t.astype(np.float64))
        assert abs(float(loss.detach()) - value) <= 1e-5 * abs(value), (float(loss.detach()), value)
        with torch.no_grad():          # Trainer.validate: the forward launches alone, the same value
            fresh = gfd.nn.FlowLoss(lambda_d, TERMS, zero=("div",), edge_vectors="rel")
            assert torch.equal(fresh(graph, pred, target), loss) and fresh.operator(graph)._adjoint_tables is None
        assert crit.operator(graph)._adjoint_tables is not None and crit.builds == 1
    # a central difference of the fp64 loss (lambda_d = 0: a quadratic, so the quotient is exact up to the fp64
    # rounding of the two values, sums of a few n terms each) along a random
    # direction against <grad, v>, inside the same allowance carried along v
    v = np.random.default_rng(20 + dim).standard_normal(p.shape)
    h = 1e-3
    p64, t64 = p.astype(np.float64), t.astype(np.float64)
    up, down = ref.loss(p64 + h * v, t64), ref.loss(p64 - h * v, t64)
    quotient = (up - down) / (2 * h)
    slack = float((allowed * np.abs(v)).sum()) + (4 * m.n + 64) * 2.0 ** -53 * (abs(up) + abs(down)) / h
    along = float((got.cpu().numpy().astype(np.float64) * v).sum())
    assert abs(along - quotient) <= slack, (along, quotient, slack)
    note("FlowLoss: |<grad, v> - central difference| / allowed", abs(along - quotient) / slack)
    assert abs(quotient) > 1e2 * slack          # (the check has teeth: the allowance is far below the derivative)


def test_flow_loss_without_a_live_term_is_graph_loss():
    m = mesh_of(2)
    graph = graph_of(m)
    p, t = fields(m, 30)
    target = torch.from_numpy(t).to(DEV)
    for lambda_d in (0, 0.25):
        out = []
        for crit in (gfd.nn.GraphLoss(lambda_d), gfd.nn.FlowLoss(lambda_d, {"div": 0.0, "vort": 0}), gfd.nn.FlowLoss(lambda_d)):
            pred = torch.from_numpy(p).to(DEV).requires_grad_(True)
            loss = crit(graph, pred, target)
            out.append((loss.detach(), torch.autograd.grad(loss, pred)[0]))
            assert getattr(crit, "builds", 0) == 0
        for loss, grad in out[1:]:
            assert torch.equal(bits(loss), bits(out[0][0])) and torch.equal(bits(grad), bits(out[0][1]))


# ====================================================================== the operator cache
def test_the_operator_cache_follows_the_batch_object():
    m = mesh_of(2)
    graph = graph_of(m)
    p, t = fields(m, 40)
    pred, target = torch.from_numpy(p).to(DEV), torch.from_numpy(t).to(DEV)
    crit = gfd.nn.FlowLoss(0, {"div": 0.1, "vort": 0.05})
    first = crit(graph, pred, target)
    op = crit.operator(graph)
    assert crit.builds == 1 and torch.equal(crit(graph, pred, target), first) and crit.builds == 1 and crit.operator(graph) is op
    # a fresh batch that sits at the address of the old one (other tensor objects over the same memory): rebuilt
    again = gfd.Graph(pos=graph.pos.view_as(graph.pos), edge_index=graph.edge_index.view_as(graph.edge_index), omega=graph.omega)
    assert again.edge_index is not graph.edge_index and again.edge_index.data_ptr() == graph.edge_index.data_ptr()
    assert torch.equal(crit(again, pred, target), first) and crit.builds == 2 and crit.operator(again) is not op
    assert crit.builds == 2
    # the same edge_index object with other positions: rebuilt
    moved = gfd.Graph(pos=graph.pos * 2.0, edge_index=again.edge_index, omega=graph.omega)
    assert not torch.equal(crit(moved, pred, target), first) and crit.builds == 3
    # an in-place edit of edge_index: rebuilt, and what a fresh loss makes of the edited batch
    crit(graph, pred, target)
    assert crit.builds == 4
    graph.edge_index[0, :5] = graph.edge_index[0, 5:10].clone()
    edited = crit(graph, pred, target)
    assert crit.builds == 5
    assert torch.equal(edited, gfd.nn.FlowLoss(0, {"div": 0.1, "vort": 0.05})(graph, pred, target)) and not torch.equal(edited, first)
    # an in-place edit of the positions as well
    graph.pos[:3] += 0.01
    crit(graph, pred, target)
    assert crit.builds == 6


# ====================================================================== fit
def _dataset(n_graphs, nodes, n_out, seed=0):
    """tests/test_gpu_train.py's: synthetic meshes with a smooth, learnable target."""
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


def test_fit_with_a_flow_loss(tmp_path):
    torch.manual_seed(0)
    model = gfd.nn.NsTwoScaleGNN(arch=S.mus_arch("NsTwoScaleGNN", 32), device=DEV)
    coarsen = gfd.transforms.GridClustering(S.default_cells(700, 2, 2))
    train = gfd.DataLoader(_dataset(4, 700, 2), batch_size=2, shuffle=False, transform=coarsen)
    # the first batch: parameter gradients under GraphLoss, under a FlowLoss with no live term (the same bits) and under a live one
    batch = next(iter(train)).to(DEV)
    grads = []
    model.train()
    for crit in (gfd.nn.GraphLoss(0.25), gfd.nn.FlowLoss(0.25, {"div": 0, "vort": 0.0}), gfd.nn.FlowLoss(0.25, {"div": 0.1, "vort": 0.05})):
        model.zero_grad()
        loss = crit(batch, model.forward(batch, 0), batch.target[:, :3])
        loss.backward()
        grads.append((loss.detach().clone(), [p.grad.detach().clone() for p in model.parameters()]))
    assert torch.equal(bits(grads[1][0]), bits(grads[0][0])) and all(torch.equal(bits(a), bits(b)) for a, b in zip(grads[1][1], grads[0][1]))
    assert float(grads[2][0]) > float(grads[0][0]) and any(not torch.equal(a, b) for a, b in zip(grads[2][1], grads[0][1]))
    model.zero_grad()
    before = [p.detach().clone() for p in model.parameters()]
    crit = gfd.nn.FlowLoss(0.25, {"div": 0.1, "vort": 0.05})
    cfg = gfd.nn.TrainConfig(name="flow", folder=str(tmp_path), epochs=2, num_steps=[2], training_loss=crit, validation_loss=crit, lr=2e-3,
                             batch_size=2, device=DEV)
    model.fit(cfg, train, train)
    h = model.history
    assert len(h) == 2 and all(np.isfinite(r["training_loss"]) and np.isfinite(r["validation_loss"]) and r["gradients_norm"] > 0 for r in h)
    assert any(not torch.equal(a, b.detach()) for a, b in zip(before, model.parameters()))
    # two output steps per batch: the second call on a batch reuses the operator (2 batches x 2 epochs of training, 2 of validation each)
    assert 0 < crit.builds <= 8


def test_zz_print_the_measured_ratios():
    """Not a check of its own: the measured / allowed ratio of every bound above, for tests/FLOW_LOSS_MEASURED.md (pytest -s)."""
    for k, v in sorted(RATIOS.items()):
        print(f"MEASURED {k}: {v:.3f}")
        assert v <= 1.0
