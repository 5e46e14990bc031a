"""`gfd.nn.ResidualLoss` on the device: its value and its gradient with respect to the prediction against the fp64 restatement of
tests/jet_ref.py (`ResidualRef`, within the allowances derived term by term at `ResidualRef.value_and_grad`), that gradient against a
central difference of the fp64 loss, `weight=0` against `GraphLoss` bit for bit, the operator cache, and a two-epoch `fit`.  The
worst measured / allowed ratios are printed by the last test (tests/JET_MEASURED.md)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

import jet_ref as J                                      # noqa: E402
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
    return J.stencil_mesh(300, dim).shuffled(11)


def graph_of(m, nf, seed=0):
    """The planted stencil as the graph's in-edges (k=None), two previous steps in `field`, a per-node viscosity and a mask."""
    rng = np.random.default_rng(seed)
    g = gfd.Graph(pos=torch.from_numpy(m.pos).float(), edge_index=torch.from_numpy(np.stack([m.row, m.col])))
    g.rel = torch.from_numpy(m.rel)
    omega = torch.zeros(m.n, 2)
    omega[torch.randperm(m.n, generator=torch.Generator().manual_seed(seed))[:40], 0] = 1          # 40 Dirichlet nodes
    g.omega = omega
    g.field = torch.from_numpy(rng.standard_normal((m.n, 2 * nf)).astype(np.float32))
    g.visc = torch.from_numpy((0.02 + 0.08 * rng.random((m.n, 1))).astype(np.float32))
    g.inner = torch.from_numpy((rng.random(m.n) < 0.8).astype(np.int64))
    return g.to(DEV)


def fields(m, seed, nf):
    rng = np.random.default_rng(seed)
    p = rng.standard_normal((m.n, nf)).astype(np.float32)
    return p, (p + 0.2 * rng.standard_normal((m.n, nf))).astype(np.float32)


CASES = {          # dim -> the keywords of the loss beyond (lambda_d, weight, node_weight)
    2: [dict(nu=0.05, dt=0.1), dict(nu="visc", dt=0.05, rho=1.3, velocity=(2, 0), pressure=1, scale=[2.0, 0.5, 1.5], shift=[0.1, -0.2, 0.3],
                                    continuity=0.7, reference="zero", mask="inner")],
    3: [dict(nu="visc", dt=0.1, rho=0.8, scale=[2.0, 0.5, 1.5, 0.7], shift=[0.1, -0.2, 0.3, 0.0], continuity=0.5, mask="inner")],
}


def reference(op, m, graph, nf, lambda_d, weight, node_weight, kw):
    nu = graph.visc.cpu().numpy().astype(np.float64).reshape(-1) if isinstance(kw["nu"], str) else kw["nu"]
    counted = ~op.degenerate.cpu().numpy()
    if kw.get("mask"):
        counted &= graph.inner.cpu().numpy() != 0
    rest = {k: v for k, v in kw.items() if k not in ("nu", "mask")}
    return J.ResidualRef(m.off, op.c.cpu().numpy(), op.src.cpu().numpy(), m.max_deg, m.dim, nf, nu=nu, counted=counted, lambda_d=lambda_d,
                         weight=weight, node_weight=node_weight, dirichlet=(graph.omega[:, 0] == 1).cpu().numpy(), **rest)


@pytest.mark.parametrize("dim", [2, 3])
def test_value_and_gradient_against_the_fp64_restatement(dim):
    m = mesh_of(dim)
    nf = dim + 1
    graph = graph_of(m, nf)
    p, t = fields(m, 10 + dim, nf)
    target = torch.from_numpy(t).to(DEV)
    prev = graph.field[:, -nf:].cpu().numpy()
    for j, kw in enumerate(CASES[dim]):
        lambda_d, weight, node_weight = (0.25, 0.3, 0.8) if j else (0.0, 1.0, 1.0)
        crit = gfd.nn.ResidualLoss(lambda_d, weight, node_weight, k=None, edge_vectors="rel", **kw)
        pred = torch.from_numpy(p).to(DEV).requires_grad_(True)
        loss = crit(graph, pred, target)
        (got,) = torch.autograd.grad(loss, pred)
        op = crit.operator(graph)
        assert crit.builds == 1 and op._adjoint_tables is not None
        ref = reference(op, m, graph, nf, lambda_d, weight, node_weight, kw)
        value, e_value, want, allowed = ref.value_and_grad(p, t, prev)
        print(f"MEASURED dim {dim} case {j}: loss {float(loss.detach()):.9g} fp64 {value:.12g} allowed {e_value:.3g}")
        assert abs(float(loss.detach()) - value) <= e_value, (float(loss.detach()), value, e_value)
        note("ResidualLoss: |value - fp64| / allowed", abs(float(loss.detach()) - value) / e_value)
        note("ResidualLoss: |grad - fp64| / allowed", J.within(got, want, allowed, f"dim {dim} case {j}"))
        assert abs(ref.loss(p, t, prev) - value) <= 1e-12 * abs(value)
        # the restatement with one wrong term is outside the same allowance
        for wrong in J.WRONG_RESIDUAL:
            bad = reference(op, m, graph, nf, lambda_d, weight, node_weight, dict(kw, wrong=wrong)).loss(p, t, prev)
            assert abs(float(loss.detach()) - bad) > 10 * e_value, wrong
        with torch.no_grad():          # Trainer.validate: the forward launches alone, the same value
            fresh = gfd.nn.ResidualLoss(lambda_d, weight, node_weight, k=None, edge_vectors="rel", **kw)
            assert torch.equal(fresh(graph, pred, target), loss) and fresh.operator(graph)._adjoint_tables is None
    # a central difference of the fp64 loss along a random direction against <grad, v>: the loss is a quartic in pred, so the quotient
    # is off the derivative by h² |third derivative| / 6 — bounded here by the difference of the quotients at h and 2h, which is three
    # times that — plus the fp64 rounding of the two values; <grad, v> carries the gradient's allowance along v
    v = np.random.default_rng(20 + dim).standard_normal(p.shape)
    p64 = p.astype(np.float64)

    def quotient(h):
        up, down = ref.loss(p64 + h * v, t, prev), ref.loss(p64 - h * v, t, prev)
        return (up - down) / (2 * h), (4 * m.n * nf + 64) * 2.0 ** -53 * (abs(up) + abs(down)) / h

    (q1, r1), (q2, _) = quotient(1e-3), quotient(2e-3)
    slack = float((allowed * np.abs(v)).sum()) + abs(q2 - q1) + r1
    along = float((got.cpu().numpy().astype(np.float64) * v).sum())
    assert abs(along - q1) <= slack, (along, q1, slack)
    note("ResidualLoss: |<grad, v> - central difference| / allowed", abs(along - q1) / slack)
    assert abs(q1) > 1e2 * slack          # (the check has teeth: the allowance is far below the derivative)


def test_the_own_stencil_is_the_default_and_searches_per_graph():
    """k=12 (the default) on a batch of two graphs over the same square: the operator's stencil stays inside each graph, and the value
    is the restatement's on the operator's own tables."""
    rng = np.random.default_rng(4)
    n0, n1, nf = 300, 250, 3
    pos = np.concatenate([rng.random((n0, 2)), rng.random((n1, 2))]).astype(np.float32)
    g = gfd.Graph(pos=torch.from_numpy(pos), omega=torch.zeros(n0 + n1, 2))
    g.batch = torch.cat([torch.zeros(n0, dtype=torch.long), torch.ones(n1, dtype=torch.long)])
    g.field = torch.from_numpy(rng.standard_normal((n0 + n1, nf)).astype(np.float32))
    g = g.to(DEV)
    p = rng.standard_normal((n0 + n1, nf)).astype(np.float32)
    t = (p + 0.2 * rng.standard_normal(p.shape)).astype(np.float32)
    crit = gfd.nn.ResidualLoss(0, nu=0.05, dt=0.1)
    assert crit.k == 12
    pred = torch.from_numpy(p).to(DEV).requires_grad_(True)
    loss = crit(g, pred, torch.from_numpy(t).to(DEV))
    (got,) = torch.autograd.grad(loss, pred)
    op = crit.operator(g)
    src = op.src.cpu().numpy().reshape(-1, 12)
    assert (src[:n0] < n0).all() and (src[n0:] >= n0).all()
    ref = J.ResidualRef(op.off.cpu().numpy(), op.c.cpu().numpy(), op.src.cpu().numpy(), 12, 2, nf, nu=0.05, dt=0.1,
                        counted=~op.degenerate.cpu().numpy())
    value, e_value, want, allowed = ref.value_and_grad(p, t, g.field.cpu().numpy())
    assert abs(float(loss.detach()) - value) <= e_value
    note("ResidualLoss (k=12, a batch): |grad - fp64| / allowed", J.within(got, want, allowed, "batch"))


def test_weight_zero_is_graph_loss_bit_for_bit_and_builds_nothing():
    m = mesh_of(2)
    graph = graph_of(m, 3)
    p, t = fields(m, 30, 3)
    target = torch.from_numpy(t).to(DEV)
    for lambda_d in (0, 0.25):
        for node_weight in (1.0, 0.5):
            out = []
            for crit in (gfd.nn.GraphLoss(lambda_d), gfd.nn.ResidualLoss(lambda_d, 0.0, node_weight, nu=0.05, dt=0.1),
                         gfd.nn.ResidualLoss(lambda_d, 0, node_weight, nu="visc", dt=0.1, k=None, edge_vectors="rel")):
                pred = torch.from_numpy(p).to(DEV).requires_grad_(True)
                loss = crit(graph, pred, target)
                if isinstance(crit, gfd.nn.GraphLoss) and node_weight != 1.0:
                    loss = node_weight * loss
                out.append((loss.detach(), torch.autograd.grad(loss, pred)[0]))
                assert getattr(crit, "builds", 0) == 0 and getattr(crit, "_cache", None) is None
            for loss, grad in out[1:]:
                assert torch.equal(bits(loss), bits(out[0][0])) and torch.equal(bits(grad), bits(out[0][1]))


def test_the_operator_cache_follows_the_batch_object():
    m = mesh_of(2)
    graph = graph_of(m, 3)
    p, t = fields(m, 40, 3)
    pred, target = torch.from_numpy(p).to(DEV), torch.from_numpy(t).to(DEV)
    crit = gfd.nn.ResidualLoss(0, nu=0.05, dt=0.1, k=None)
    first = crit(graph, pred, target)
    op = crit.operator(graph)
    # the steps of one batch: the same operator, whatever the prediction and `field` are
    graph.field = torch.roll(graph.field, 3, 1)
    assert crit.builds == 1 and not torch.equal(crit(graph, pred * 1.5, target), first) and crit.builds == 1 and crit.operator(graph) is op
    graph.field = torch.roll(graph.field, -3, 1)
    assert torch.equal(crit(graph, pred, target), first) and crit.builds == 1
    # a fresh batch that sits at the address of the old one (other tensor objects over the same memory): rebuilt
    again = gfd.Graph(pos=graph.pos.view_as(graph.pos), edge_index=graph.edge_index.view_as(graph.edge_index), omega=graph.omega, field=graph.field)
    assert again.edge_index is not graph.edge_index and again.edge_index.data_ptr() == graph.edge_index.data_ptr()
    assert torch.equal(crit(again, pred, target), first) and crit.builds == 2 and crit.operator(again) is not op
    # an in-place edit of the positions: rebuilt
    crit(graph, pred, target)
    assert crit.builds == 3
    graph.pos[:3] += 0.01
    assert not torch.equal(crit(graph, pred, target), first) and crit.builds == 4
    # the own stencil is keyed by pos and batch
    own = gfd.nn.ResidualLoss(0, nu=0.05, dt=0.1)
    a = own(graph, pred, target)
    assert own.builds == 1 and torch.equal(own(graph, pred, target), a) and own.builds == 1
    graph.pos[:3] -= 0.01
    own(graph, pred, target)
    assert own.builds == 2


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


def test_fit_with_a_residual_loss(tmp_path):
    torch.manual_seed(0)
    model = gfd.nn.NsTwoScaleGNN(arch=S.mus_arch("NsTwoScaleGNN", 32), device=DEV)
    coarsen = gfd.transforms.GridClustering(S.default_cells(700, 2, 2))
    train = gfd.DataLoader(_dataset(4, 700, 2), batch_size=2, shuffle=False, transform=coarsen)
    batch = next(iter(train)).to(DEV)
    grads = []
    model.train()
    for crit in (gfd.nn.GraphLoss(0.25), gfd.nn.ResidualLoss(0.25, 0.0, nu=0.01, dt=0.1), gfd.nn.ResidualLoss(0.25, 1e-3, nu=0.01, dt=0.1)):
        model.zero_grad()
        loss = crit(batch, model.forward(batch, 0), batch.target[:, :3])
        loss.backward()
        grads.append((loss.detach().clone(), [p.grad.detach().clone() for p in model.parameters()]))
    assert torch.equal(bits(grads[1][0]), bits(grads[0][0])) and all(torch.equal(bits(a), bits(b)) for a, b in zip(grads[1][1], grads[0][1]))
    assert float(grads[2][0]) > float(grads[0][0]) and any(not torch.equal(a, b) for a, b in zip(grads[2][1], grads[0][1]))
    model.zero_grad()
    before = [p.detach().clone() for p in model.parameters()]
    crit = gfd.nn.ResidualLoss(0.25, 1e-3, nu=0.01, dt=0.1)
    cfg = gfd.nn.TrainConfig(name="residual", folder=str(tmp_path), epochs=2, num_steps=[2], training_loss=crit, validation_loss=crit, lr=2e-3,
                             batch_size=2, device=DEV)
    model.fit(cfg, train, train)
    h = model.history
    assert len(h) == 2 and all(np.isfinite(r["training_loss"]) and np.isfinite(r["validation_loss"]) and r["gradients_norm"] > 0 for r in h)
    assert any(not torch.equal(a, b.detach()) for a, b in zip(before, model.parameters()))
    # two output steps per batch: the second call on a batch reuses the operator (2 batches x 2 epochs of training, 2 of validation each)
    assert 0 < crit.builds <= 8


def test_zz_print_the_measured_ratios():
    """Not a check of its own: the measured / allowed ratio of every bound above, for tests/JET_MEASURED.md (pytest -s)."""
    for k, v in sorted(RATIOS.items()):
        print(f"MEASURED {k}: {v:.3f}")
        assert v <= 1.0
