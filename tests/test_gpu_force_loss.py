"""`gfd.nn.ForceLoss` on the device: its value and its gradient with respect to the prediction against the fp64 restatement of
tests/forces_adjoint_ref.py (`ForceRef`, on the DEVICE's own wall and gradient tables, which tests/test_gpu_body_forces.py and
tests/test_gpu_forces_adjoint.py pin) within the allowance derived there, and against a central difference of the fp64 loss; the
paths that build nothing; collated batches; measured loads per output step; the operator cache; and a fit on loads alone."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

import forces_adjoint_ref as A                           # noqa: E402
import forces_ref as FR                                  # noqa: E402
import graphs4cfd_amd as gfd                             # noqa: E402
from graphs4cfd_amd import synthetic as S                # noqa: E402

DEV = torch.device("cuda", 0)
RATIOS = {}
NF, T = 3, 3
SCALE, SHIFT, MU = [1.5, 0.75, 2.5], [0.25, -0.5, 0.125], 0.03125 * 1.3
PHYS = dict(mu=MU, scale=SCALE, shift=SHIFT)


def note(name, r):
    RATIOS[name] = max(RATIOS.get(name, 0.0), float(r))


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def graph_of(counts, seed=0, n=300, comps=2):
    """An annulus round len(counts) bodies: `bound` == 4 on every wall node, `which` the body's label, 40 Dirichlet nodes, and loads
    [B, comps · T] somebody measured."""
    pos, wall, label = FR.annulus(n, counts, seed=seed)
    g = gfd.Graph(pos=torch.from_numpy(pos).to(DEV))
    g.edge_index = S.connect_knn(g.pos, 6)[0]
    m = len(pos)
    bound, which = torch.zeros(m, dtype=torch.long), torch.zeros(m, dtype=torch.long)
    bound[torch.from_numpy(wall)] = 4
    which[torch.from_numpy(wall)] = torch.from_numpy(label)
    omega = torch.zeros(m, 2)
    omega[torch.randperm(m, generator=torch.Generator().manual_seed(seed))[:40], 0] = 1
    g.bound, g.which, g.omega = bound.to(DEV), which.to(DEV), omega.to(DEV)
    g.loads = dev(np.random.default_rng(50 + seed).standard_normal((len(counts), comps * T)).astype(np.float32))
    return g


def fields(n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, NF)).astype(np.float32), rng.standard_normal((n, NF)).astype(np.float32)


def reference(crit, graph):
    """ForceRef from the DEVICE's tables of the loss's operator."""
    op = crit.operator(graph)
    geo = dict(items=op.items.cpu().numpy(), body_offsets=op.body_offsets.cpu().numpy(), area=op.area.cpu().numpy(), unit=op.unit.cpu().numpy(),
               arm=op.arm.cpu().numpy(), n_bodies=op.n_bodies)
    c = op.constants()
    if op.mu != 0:
        c.update(off=op.gradient.off.cpu().numpy(), g=op.gradient.g.cpu().numpy(), src=op.gradient.src.cpu().numpy())
    return A.ForceRef(geo, op.n_nodes, c, weight=crit.weight, node_weight=crit.node_weight, lambda_d=crit.lambda_d,
                      dirichlet=(graph.omega[:, 0] == 1).cpu().numpy(), components=crit.components, force_scale=crit.force_scale,
                      wall={"pressure": crit.wall_pressure, "shear": crit.wall_shear})


def check(crit, graph, p, t, ref, what, values=None, step=None):
    """Value and gradient of one call against the fp64 restatement: (the device's gradient, the allowance)."""
    pred = dev(p).requires_grad_(True)
    loss = crit(graph, pred, dev(t)) if step is None else crit(graph, pred, dev(t), step=step)
    (got,) = torch.autograd.grad(loss, pred)
    want, allowed = ref.grad(p, t, values)
    err = np.abs(got.cpu().numpy().astype(np.float64) - want)
    print(f"{what}: worst |grad - fp64| / allowed {float(np.where(allowed > 0, err / np.maximum(allowed, 1e-300), 0).max())!r}")
    note("ForceLoss: |grad - fp64| / allowed", FR.within(got, want, allowed, what))
    value, slack = ref.value(p, t, values)
    print(f"{what}: loss {float(loss.detach())!r} fp64 {value!r} allowed {slack!r}")
    assert abs(float(loss.detach()) - value) <= slack, (what, float(loss.detach()), value, slack)
    note("ForceLoss: |value - fp64| / allowed", abs(float(loss.detach()) - value) / slack)
    return got.cpu().numpy().astype(np.float64), allowed


# ====================================================================== value and gradient
@pytest.mark.parametrize("viscous", [True, False], ids=["viscous", "pressure only"])
def test_force_loss_gradient_against_the_fp64_formula(viscous):
    graph = graph_of((37,))
    n = int(graph.pos.size(0))
    p, t = fields(n, 10 + viscous)
    phys = PHYS if viscous else dict(scale=SCALE, shift=SHIFT)
    kw = dict(weight=0.7, node_weight=0.5, components=("fx", "fy", "m"), force_scale=0.5, wall={"pressure": 0.3, "shear": 0.2 if viscous else 0}, **phys)
    for lambda_d in (0.25, 0):
        crit = gfd.nn.ForceLoss(lambda_d, **kw)
        ref = reference(crit, graph)
        got, allowed = check(crit, graph, p, t, ref, f"viscous {viscous} lambda_d {lambda_d}")
        assert crit.builds == 1 and crit.operator(graph)._adjoint_tables is not None
        with torch.no_grad():          # Trainer.validate: the forward launches alone, the same value
            fresh = gfd.nn.ForceLoss(lambda_d, **kw)
            assert torch.equal(fresh(graph, dev(p), dev(t)), crit(graph, dev(p), dev(t))) and fresh.operator(graph)._adjoint_tables is None
    # a central difference of the fp64 loss (lambda_d = 0: a quadratic, so the quotient is exact up to the fp64 rounding of the two
    # values) along a random direction against <grad, v>, inside the same allowance carried along v
    v = np.random.default_rng(20 + viscous).standard_normal(p.shape)
    h = 1e-3
    p64, t64 = p.astype(np.float64), t.astype(np.float64)
    up, down = ref.loss(p64 + h * v, t64), ref.loss(p64 - h * v, t64)
    quotient = (up - down) / (2 * h)
    slack = float((allowed * np.abs(v)).sum()) + (16 * n + 64) * 2.0 ** -53 * (abs(up) + abs(down)) / h
    along = float((got * v).sum())
    assert abs(along - quotient) <= slack, (along, quotient, slack)
    note("ForceLoss: |<grad, v> - central difference| / allowed", abs(along - quotient) / slack)
    assert abs(quotient) > 1e2 * slack          # (the check has teeth: the allowance is far below the derivative)
    # on the loads alone: the gradient lives on the wall nodes and their senders only
    crit = gfd.nn.ForceLoss(weight=2.0, node_weight=0, **phys)
    got, _ = check(crit, graph, p, t, reference(crit, graph), f"viscous {viscous} loads alone")
    op = crit.operator(graph)
    reached = torch.zeros(n, dtype=torch.bool, device=DEV)
    reached[op.items] = True
    if viscous:
        gr = op.gradient
        dst = torch.repeat_interleave(torch.arange(n, device=DEV), (gr.off[1:] - gr.off[:-1]).long())
        reached[gr.src.long()[reached[dst]]] = True
    assert not got[~reached.cpu().numpy()].any() and got[op.items.cpu().numpy()].any()


def test_two_labelled_bodies_and_measured_loads():
    graph = graph_of((21, 5), seed=1)
    n = int(graph.pos.size(0))
    p, t = fields(n, 30)
    crit = gfd.nn.ForceLoss(0.25, weight=1.5, bodies="which", values="loads", **PHYS)
    assert crit.operator(graph).n_bodies == 2 and crit.operator(graph).body_offsets.tolist() == [0, 21, 26]
    loads = graph.loads.cpu().numpy().astype(np.float64)
    ref = reference(crit, graph)
    grads = [check(crit, graph, p, t, ref, f"step {step}", values=loads[:, 2 * step:2 * step + 2], step=step)[0] for step in range(T)]
    assert not np.array_equal(grads[0], grads[1]) and not np.array_equal(grads[1], grads[2]) and crit.builds == 1
    with pytest.raises(ValueError, match="^step:"):
        crit(graph, dev(p), dev(t))
    with pytest.raises(ValueError, match="^step:"):
        crit(graph, dev(p), dev(t), step=T)
    with pytest.raises(ValueError, match="^values:"):
        gfd.nn.ForceLoss(values="nothing", **PHYS)(graph, dev(p), dev(t), step=0)
    # the same wall named by an attribute: a bool mask and integer flags
    graph.mask = graph.bound == 4
    graph.flag = (graph.bound == 4).to(torch.int32) * 7
    for nodes in ("mask", "flag"):
        other = gfd.nn.ForceLoss(0.25, weight=1.5, bodies="which", values="loads", nodes=nodes, **PHYS)
        assert torch.equal(bits(other(graph, dev(p), dev(t), step=1)), bits(crit(graph, dev(p), dev(t), step=1)))


def test_a_batch_of_two_graphs_gives_two_bodies():
    g1, g2 = graph_of((37,), seed=1), graph_of((37,), seed=2)
    batch = gfd.nn.collate([g1, g2])
    n1 = int(g1.pos.size(0))
    assert tuple(batch.loads.shape) == (2, 2 * T) and int(batch.batch.max()) == 1
    (p1, t1), (p2, t2) = fields(n1, 41), fields(int(g2.pos.size(0)), 42)
    p, t = np.concatenate([p1, p2]), np.concatenate([t1, t2])
    for values in (None, "loads"):
        crit = gfd.nn.ForceLoss(0.25, weight=0.7, values=values, wall={"pressure": 0.5}, **PHYS)
        op = crit.operator(batch)
        assert crit.builds == 1 and op.n_bodies == 2 and op.body_offsets.tolist() == [0, 37, 74]
        assert int(op.items[:37].max()) < n1 <= int(op.items[37:].min())          # each body holds the wall nodes of its own graph
        one = gfd.nn.ForceLoss(0.25, weight=0.7, values=values, wall={"pressure": 0.5}, **PHYS).operator(g1)
        assert torch.equal(op.items[:37], one.items) and torch.equal(op.area[:37], one.area)
        obs = None if values is None else batch.loads.cpu().numpy().astype(np.float64)[:, 2:4]
        check(crit, batch, p, t, reference(crit, batch), f"batch values {values}", values=obs, step=1)
    # two labelled bodies per graph: four bodies, graph-major
    b1, b2 = graph_of((21, 5), seed=3), graph_of((21, 5), seed=4)
    both = gfd.nn.collate([b1, b2])
    crit = gfd.nn.ForceLoss(weight=1.0, bodies="which", values="loads", **PHYS)
    op = crit.operator(both)
    assert op.n_bodies == 4 and op.body_offsets.tolist() == [0, 21, 26, 47, 52] and tuple(both.loads.shape) == (4, 2 * T)
    pb, tb = fields(int(both.pos.size(0)), 43)
    check(crit, both, pb, tb, reference(crit, both), "four bodies", values=both.loads.cpu().numpy().astype(np.float64)[:, :2], step=0)


# ====================================================================== the terms that vanish
def test_without_a_live_term_it_is_graph_loss():
    graph = graph_of((37,))
    n = int(graph.pos.size(0))
    p, t = fields(n, 60)
    for lambda_d in (0, 0.25):
        out = []
        crits = (gfd.nn.GraphLoss(lambda_d), gfd.nn.ForceLoss(lambda_d, weight=0, **PHYS), gfd.nn.ForceLoss(lambda_d, weight=0.0, values="loads", **PHYS),
                 gfd.nn.ForceLoss(lambda_d, weight=0, wall={"pressure": 0, "shear": 0.0}, **PHYS))
        for crit in crits:
            pred = dev(p).requires_grad_(True)
            loss = crit(graph, pred, dev(t))
            out.append((loss.detach(), torch.autograd.grad(loss, pred)[0]))
        for c in crits[1:]:
            assert c.builds == 0 and c._cache is None                    # nothing built, nothing launched
        for loss, grad in out[1:]:
            assert torch.equal(bits(loss), bits(out[0][0])) and torch.equal(bits(grad), bits(out[0][1]))
    half = gfd.nn.ForceLoss(0.25, weight=0, node_weight=0.5, **PHYS)(graph, dev(p), dev(t))
    assert torch.equal(bits(half), bits(0.5 * gfd.nn.GraphLoss(0.25)(graph, dev(p), dev(t))))
    pred = dev(p).requires_grad_(True)
    zero = gfd.nn.ForceLoss(weight=0, node_weight=0, **PHYS)(graph, pred, dev(t))
    assert float(zero.detach()) == 0.0 and not torch.autograd.grad(zero, pred)[0].any()


# ====================================================================== the operator cache
def test_the_operator_cache_follows_the_batch_object():
    graph = graph_of((37,))
    n = int(graph.pos.size(0))
    p, t = fields(n, 70)
    pred, target = dev(p), dev(t)
    crit = gfd.nn.ForceLoss(values="loads", **PHYS)
    first = crit(graph, pred, target, step=0)
    op = crit.operator(graph)
    for step in range(T):          # Trainer.train_epoch: one call per output step of the same batch
        crit(graph, pred, target, step=step)
    assert crit.builds == 1 and crit.operator(graph) is op and torch.equal(crit(graph, pred, target, step=0), first)
    # a fresh batch that sits at the address of the old one (another tensor object over the same memory): rebuilt
    again = gfd.Graph(pos=graph.pos.view_as(graph.pos), edge_index=graph.edge_index, omega=graph.omega, bound=graph.bound, loads=graph.loads)
    assert again.pos is not graph.pos and again.pos.data_ptr() == graph.pos.data_ptr()
    assert torch.equal(crit(again, pred, target, step=0), first) and crit.builds == 2 and crit.operator(again) is not op
    # an in-place edit of the wall codes: two nodes fewer
    crit(graph, pred, target, step=0)
    assert crit.builds == 3
    graph.bound[crit.operator(graph).items[:2]] = 0
    edited = crit(graph, pred, target, step=0)
    assert crit.builds == 4 and crit.operator(graph).n_items == 35 and not torch.equal(edited, first)
    # other edges (mu != 0: the gradient is built on them)
    graph.edge_index = graph.edge_index[:, : -6].contiguous()
    crit(graph, pred, target, step=0)
    assert crit.builds == 5
    # a batch vector appears: rebuilt
    graph.batch = torch.zeros(n, dtype=torch.long, device=DEV)
    assert crit(graph, pred, target, step=1) is not None and crit.builds == 6
    crit(graph, pred, target, step=2)
    assert crit.builds == 6
    # mu == 0: the edges are not looked at
    inviscid = gfd.nn.ForceLoss(values="loads")
    inviscid(graph, pred, target, step=0)
    graph.edge_index = graph.edge_index[:, : -6].contiguous()
    inviscid(graph, pred, target, step=0)
    assert inviscid.builds == 1


# ====================================================================== fit
def _ring(pos, m=12, radius=0.22):
    """The nodes nearest to m points of a circle round the middle of the unit square, ordered by angle: a bool mask [N]."""
    th = 2.0 * np.pi * (torch.arange(m) + 0.25) / m
    pts = torch.stack([0.5 + radius * torch.cos(th), 0.5 + radius * torch.sin(th)], 1).to(pos.dtype)
    rows = torch.unique(torch.cdist(pts, pos.cpu()).argmin(1))
    mask = torch.zeros(int(pos.size(0)), dtype=torch.bool)
    mask[rows] = True
    return mask


def _dataset(n_graphs, nodes, n_out, seed=0):
    """tests/test_gpu_train.py's: synthetic meshes with a smooth, learnable target — and the loads somebody measured on a ring of nodes."""
    data = []
    for i in range(n_graphs):
        g = S.mus_graph(nodes, levels=1, seed=seed + i)
        f, tgt = g.field, []
        for _ in range(n_out):
            f = 0.9 * f + 0.1 * g.glob
            tgt.append(f)
        g.target = torch.cat(tgt, 1)
        g.wall = _ring(g.pos)
        g.loads = torch.tensor([[0.05 * (k + 1), -0.02 * (k + 1)] for k in range(n_out)]).reshape(1, 2 * n_out)
        data.append(g)
    return data


def test_fit_on_loads_alone(tmp_path):
    torch.manual_seed(0)
    model = gfd.nn.NsOneScaleGNN(arch=S.mus_arch("NsOneScaleGNN", 32), device=DEV)
    train = gfd.DataLoader(_dataset(4, 300, 2), batch_size=2, shuffle=False)
    before = [p.detach().clone() for p in model.parameters()]
    crit = gfd.nn.ForceLoss(node_weight=0, nodes="wall", values="loads", mu=0.01)
    cfg = gfd.nn.TrainConfig(name="force", folder=str(tmp_path), epochs=2, num_steps=[2], training_loss=crit, validation_loss=crit, lr=2e-3,
                             batch_size=2, device=DEV)
    model.fit(cfg, train, train)
    h = model.history
    assert len(h) == 2 and all(np.isfinite(r["training_loss"]) and np.isfinite(r["validation_loss"]) and r["gradients_norm"] > 0 for r in h)
    assert any(not torch.equal(a, b.detach()) for a, b in zip(before, model.parameters()))
    # two output steps per batch: the second call on a batch reuses the operator (2 batches x 2 epochs of training, 2 of validation each)
    assert 0 < crit.builds <= 8


def test_zz_print_the_measured_ratios():
    """Not a check of its own: the measured / allowed ratio of every bound above, for tests/FORCE_LOSS_MEASURED.md (pytest -s)."""
    for k, v in sorted(RATIOS.items()):
        print(f"MEASURED {k}: {v:.3f}")
        assert v <= 1.0
