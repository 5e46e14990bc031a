"""`gfd.nn.SampleLoss` on the device: its value and its gradient with respect to the prediction against the fp64 restatement of
tests/sample_adjoint_ref.py (node_weight ∂GraphLoss + (2 weight / (P_kept F')) Sᵀ mask (S pred − ref), within the allowances derived
at `SampleRef.grad` and `SampleRef.value`) and against a central difference of the fp64 loss; a batch of two graphs that overlap in
space; observations per output step; the point mask; the one-entry sampler cache; `Trainer`'s step argument; a two-epoch `fit` on
observations alone.  The worst measured / allowed ratios are printed by the last test (tests/SAMPLE_LOSS_MEASURED.md)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

import sample_adjoint_ref as A                           # noqa: E402
import sampler_ref as SR                                 # noqa: E402
import graphs4cfd_amd as gfd                             # noqa: E402
from graphs4cfd_amd import synthetic as S                # noqa: E402

DEV = torch.device("cuda", 0)
RATIOS = {}
N, P, NF, T = 300, 257, 3, 3


def note(name, r):
    RATIOS[name] = max(RATIOS.get(name, 0.0), float(r))


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def graph_of(dim, seed=0, obs_fields=NF):
    g = gfd.Graph(pos=torch.from_numpy(SR.cloud(N, dim)))
    omega = torch.zeros(N, 2)
    omega[torch.randperm(N, generator=torch.Generator().manual_seed(seed))[:40], 0] = 1          # 40 Dirichlet nodes
    g.omega = omega
    g.obs = torch.from_numpy(np.random.default_rng(50 + seed).standard_normal((P, obs_fields * T)).astype(np.float32))
    return g.to(DEV)


def fields(seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((N, NF)).astype(np.float32), rng.standard_normal((N, NF)).astype(np.float32)


def reference(crit, graph, keep=None, **kw):
    """SampleRef from the DEVICE's tables of the loss's sampler (pinned against the restatement by tests/test_gpu_point_sampler.py)."""
    s = crit.sampler(graph)[0]
    return A.SampleRef(s._idx.cpu().numpy(), s._coef.cpu().numpy(), s.n_nodes, weight=crit.weight, node_weight=crit.node_weight,
                       lambda_d=crit.lambda_d, dirichlet=(graph.omega[:, 0] == 1).cpu().numpy(), fields=crit.fields, keep=keep, **kw)


def check(crit, graph, p, t, ref, what, obs=None, step=None):
    """Value and gradient of one call against the fp64 restatement: (the device's gradient, the allowance)."""
    pred = dev(p).requires_grad_(True)
    loss = crit(graph, pred, dev(t)) if step is None else crit(graph, pred, dev(t), step=step)
    (got,) = torch.autograd.grad(loss, pred)
    want, allowed = ref.grad(p, t, obs)
    note("SampleLoss: |grad - fp64| / allowed", SR.within(got, want, allowed, what))
    value, slack = ref.value(p, t, obs)
    print(f"{what}: loss {float(loss.detach())!r} fp64 {value!r} allowed {slack!r}")
    assert abs(float(loss.detach()) - value) <= slack, (what, float(loss.detach()), value, slack)
    note("SampleLoss: |value - fp64| / allowed", abs(float(loss.detach()) - value) / slack)
    return got.cpu().numpy().astype(np.float64), allowed


# ====================================================================== value and gradient
@pytest.mark.parametrize("dim", [2, 3])
def test_sample_loss_gradient_against_the_fp64_formula(dim):
    graph = graph_of(dim)
    pts = torch.from_numpy(SR.queries(P, dim))
    p, t = fields(10 + dim)
    for lambda_d in (0.25, 0):
        crit = gfd.nn.SampleLoss(pts, lambda_d, weight=0.7, node_weight=0.5)
        ref = reference(crit, graph)
        got, allowed = check(crit, graph, p, t, ref, f"dim {dim} lambda_d {lambda_d}")
        assert crit.builds == 1 and crit.sampler(graph)[0]._adjoint_tables is not None
        with torch.no_grad():          # Trainer.validate: the forward launches alone, the same value
            fresh = gfd.nn.SampleLoss(pts, lambda_d, weight=0.7, node_weight=0.5)
            assert torch.equal(fresh(graph, dev(p), dev(t)), crit(graph, dev(p), dev(t))) and fresh.sampler(graph)[0]._adjoint_tables is None
    # a central difference of the fp64 loss (lambda_d = 0: a quadratic, so the quotient is exact up to the fp64 rounding of the two
    # values, sums of a few n terms each) along a random direction against <grad, v>, inside the same allowance carried along v
    v = np.random.default_rng(20 + dim).standard_normal(p.shape)
    h = 1e-3
    p64, t64 = p.astype(np.float64), t.astype(np.float64)
    up, down = ref.loss(p64 + h * v, t64), ref.loss(p64 - h * v, t64)
    quotient = (up - down) / (2 * h)
    slack = float((allowed * np.abs(v)).sum()) + (4 * (N + P) + 64) * 2.0 ** -53 * (abs(up) + abs(down)) / h
    along = float((got * v).sum())
    assert abs(along - quotient) <= slack, (along, quotient, slack)
    note("SampleLoss: |<grad, v> - central difference| / allowed", abs(along - quotient) / slack)
    assert abs(quotient) > 1e2 * slack          # (the check has teeth: the allowance is far below the derivative)
    # the observed columns only, points far from every node dropped, on the samples alone
    s = crit.sampler(graph)[0]
    distance = s.distance.cpu().numpy()
    limit = float(np.sort(distance)[P // 2] + np.sort(distance)[P // 2 + 1]) / 2          # between two distances: no tie with the limit
    keep = distance <= np.float32(limit)
    assert 0 < keep.sum() < P and np.abs(distance - np.float32(limit)).min() > 0
    crit = gfd.nn.SampleLoss(pts, weight=2.0, node_weight=0, fields=(2, 0), max_distance=limit)
    check(crit, graph, p, t, reference(crit, graph, keep=keep), f"dim {dim} fields, max_distance")
    assert crit.sampler(graph)[2] == int(keep.sum())


@pytest.mark.parametrize("dim", [2, 3])
def test_observations_select_the_columns_of_the_step(dim):
    graph = graph_of(dim, obs_fields=2)
    pts = torch.from_numpy(SR.queries(P, dim))
    p, t = fields(30 + dim)
    crit = gfd.nn.SampleLoss(pts, 0.25, weight=1.5, values="obs", fields=(0, 1))
    obs = graph.obs.cpu().numpy()
    ref = reference(crit, graph)
    grads = [check(crit, graph, p, t, ref, f"dim {dim} step {step}", obs=obs[:, 2 * step:2 * step + 2], step=step)[0] for step in range(T)]
    assert not np.array_equal(grads[0], grads[1]) and not np.array_equal(grads[1], grads[2]) and crit.builds == 1
    with pytest.raises(ValueError, match="^step:"):
        crit(graph, dev(p), dev(t))
    with pytest.raises(ValueError, match="^step:"):
        crit(graph, dev(p), dev(t), step=T)
    with pytest.raises(ValueError, match="^values:"):
        gfd.nn.SampleLoss(pts, values="nothing")(graph, dev(p), dev(t), step=0)


# ====================================================================== a batch of graphs that overlap in space
def test_a_batch_gives_every_graph_its_own_nodes():
    g1, g2 = graph_of(2, seed=1), graph_of(2, seed=2)          # identical positions: one search over the merged cloud would mix them
    batch = gfd.nn.collate([g1, g2])
    assert tuple(batch.pos.shape) == (2 * N, 2) and tuple(batch.obs.shape) == (2 * P, NF * T) and torch.equal(batch.pos[:N], batch.pos[N:])
    pts = torch.from_numpy(SR.queries(P, 2))
    (p1, t1), (p2, t2) = fields(41), fields(42)
    p, t = np.concatenate([p1, p2]), np.concatenate([t1, t2])
    for values in (None, "obs"):
        crit = gfd.nn.SampleLoss(pts, 0.25, weight=0.7, values=values)
        s = crit.sampler(batch)[0]
        assert crit.builds == 1 and s.n_points == 2 * P and s.n_nodes == 2 * N
        idx = s.idx.cpu().numpy()
        assert idx[:P].max() < N and idx[P:].min() >= N          # every neighbour of the second graph's points is a node of the second graph
        one = gfd.nn.SampleLoss(pts, 0.25, weight=0.7, values=values).sampler(g1)[0]
        assert torch.equal(s._idx[:, :P], one._idx) and torch.equal(s._idx[:, P:], one._idx + N) and torch.equal(bits(s._coef[:, P:]), bits(one._coef))
        assert torch.equal(bits(s.distance), bits(one.distance.repeat(2))) and torch.equal(s.degenerate, one.degenerate.repeat(2))
        obs = None if values is None else batch.obs.cpu().numpy()[:, NF:2 * NF]
        check(crit, batch, p, t, reference(crit, batch), f"batch values {values}", obs=obs, step=1)
        # the sum-weighted mean of the two single-graph losses (equal N, equal P: their mean), each within its own allowance
        singles, slack = [], 0.0
        for g, pi, ti in ((g1, p1, t1), (g2, p2, t2)):
            c = gfd.nn.SampleLoss(pts, 0.25, weight=0.7, values=values)
            with torch.no_grad():
                singles.append(float(c(g, dev(pi), dev(ti), step=1)))
            slack += 0.5 * reference(c, g).value(pi, ti, None if values is None else g.obs.cpu().numpy()[:, NF:2 * NF])[1]
        with torch.no_grad():
            both = float(crit(batch, dev(p), dev(t), step=1))
        value, allowed = reference(crit, batch).value(p, t, obs)
        # (the Dirichlet term is a mean over each graph's own 40 boundary nodes, the same number in both: the mean of the means as well)
        assert abs(both - 0.5 * (singles[0] + singles[1])) <= allowed + slack, (both, singles, allowed, slack)
        note("SampleLoss: |batch - mean of the singles| / allowed", abs(both - 0.5 * (singles[0] + singles[1])) / (allowed + slack))


# ====================================================================== the terms that vanish
def test_without_a_live_sample_term_it_is_graph_loss():
    graph = graph_of(2)
    pts = torch.from_numpy(SR.queries(P, 2))          # (none of them sits on a node: no distance is 0)
    p, t = fields(60)
    for lambda_d in (0, 0.25):
        out = []
        for crit in (gfd.nn.GraphLoss(lambda_d), gfd.nn.SampleLoss(pts, lambda_d, weight=0), gfd.nn.SampleLoss(pts, lambda_d, weight=0.0, values="obs"),
                     gfd.nn.SampleLoss(pts, lambda_d, max_distance=0.0)):
            pred = dev(p).requires_grad_(True)
            loss = crit(graph, pred, dev(t))
            out.append((loss.detach(), torch.autograd.grad(loss, pred)[0]))
        assert crit.builds == 1 and crit.sampler(graph)[2] == 0          # max_distance: a sampler was built, no point kept
        for c in (gfd.nn.SampleLoss(pts, lambda_d, weight=0),):
            c(graph, dev(p), dev(t))
            assert c.builds == 0 and c._cache is None                    # weight = 0: nothing built
        for loss, grad in out[1:]:
            assert torch.equal(bits(loss), bits(out[0][0])) and torch.equal(bits(grad), bits(out[0][1]))
    # node_weight scales GraphLoss; node_weight = 0 with no kept point is an exact, differentiable zero
    pred = dev(p).requires_grad_(True)
    zero = gfd.nn.SampleLoss(pts, node_weight=0, max_distance=0.0)(graph, pred, dev(t))
    assert float(zero.detach()) == 0.0 and not torch.autograd.grad(zero, pred)[0].any()
    half = gfd.nn.SampleLoss(pts, 0.25, weight=0, node_weight=0.5)(graph, dev(p), dev(t))
    assert torch.equal(bits(half), bits(0.5 * gfd.nn.GraphLoss(0.25)(graph, dev(p), dev(t))))


# ====================================================================== the sampler cache
def test_the_sampler_cache_follows_the_batch_object():
    graph = graph_of(2)
    pts = torch.from_numpy(SR.queries(P, 2))
    p, t = fields(70)
    pred, target = dev(p), dev(t)
    crit = gfd.nn.SampleLoss(pts, values="obs")
    first = crit(graph, pred, target, step=0)
    s = crit.sampler(graph)[0]
    for step in range(T):          # Trainer.train_epoch: one call per output step of the same batch
        crit(graph, pred, target, step=step)
    assert crit.builds == 1 and crit.sampler(graph)[0] is s and torch.equal(crit(graph, pred, target, step=0), first)
    # a fresh batch that sits at the address of the old one (another tensor object over the same memory): rebuilt
    again = gfd.Graph(pos=graph.pos.view_as(graph.pos), omega=graph.omega, obs=graph.obs)
    assert again.pos is not graph.pos and again.pos.data_ptr() == graph.pos.data_ptr()
    assert torch.equal(crit(again, pred, target, step=0), first) and crit.builds == 2 and crit.sampler(again)[0] is not s
    # other positions: rebuilt, another value
    moved = gfd.Graph(pos=graph.pos * 0.5, omega=graph.omega, obs=graph.obs)
    assert not torch.equal(crit(moved, pred, target, step=0), first) and crit.builds == 3
    # an in-place edit of the positions
    crit(graph, pred, target, step=0)
    assert crit.builds == 4
    graph.pos[:3] += 0.01
    edited = crit(graph, pred, target, step=0)
    assert crit.builds == 5 and torch.equal(edited, gfd.nn.SampleLoss(pts, values="obs")(graph, pred, target, step=0))
    # a batch vector appears: rebuilt
    graph.batch = torch.zeros(N, dtype=torch.long, device=DEV)
    assert torch.equal(crit(graph, pred, target, step=0), edited) and crit.builds == 6
    crit(graph, pred, target, step=1)
    assert crit.builds == 6


# ====================================================================== fit
def _dataset(n_graphs, nodes, n_out, pts, seed=0):
    """tests/test_gpu_train.py's: synthetic meshes with a smooth, learnable target — and what a rake would have measured of it."""
    data = []
    for i in range(n_graphs):
        g = S.mus_graph(nodes, levels=1, seed=seed + i)
        f, tgt = g.field, []
        for _ in range(n_out):
            f = 0.9 * f + 0.1 * g.glob
            tgt.append(f)
        g.target = torch.cat(tgt, 1)
        g.obs = torch.cat([0.1 * (k + 1) * torch.cat([pts, pts[:, :1] * pts[:, 1:]], 1) for k in range(n_out)], 1)          # [P, 3 n_out]
        data.append(g)
    return data


class _Plain:
    """A loss without `takes_step`: it must be called as (graph, pred, target), nothing more."""

    def __init__(self):
        self.base, self.calls = gfd.nn.GraphLoss(0.25), []

    def __call__(self, *args, **kwargs):
        self.calls.append((len(args), dict(kwargs)))
        return self.base(*args)


def test_fit_on_observations_alone(tmp_path):
    torch.manual_seed(0)
    model = gfd.nn.NsOneScaleGNN(arch=S.mus_arch("NsOneScaleGNN", 32), device=DEV)
    pts = torch.rand(64, 2, generator=torch.Generator().manual_seed(5))
    train = gfd.DataLoader(_dataset(4, 300, 2, pts), batch_size=2, shuffle=False)
    before = [p.detach().clone() for p in model.parameters()]
    crit = gfd.nn.SampleLoss(pts, values="obs", node_weight=0)
    cfg = gfd.nn.TrainConfig(name="sample", folder=str(tmp_path), epochs=2, num_steps=[2], training_loss=crit, validation_loss=crit, lr=2e-3,
                             batch_size=2, device=DEV)
    model.fit(cfg, train, train)
    h = model.history
    assert len(h) == 2 and all(np.isfinite(r["training_loss"]) and np.isfinite(r["validation_loss"]) and r["gradients_norm"] > 0 for r in h)
    assert any(not torch.equal(a, b.detach()) for a, b in zip(before, model.parameters()))
    # two output steps per batch: the second call on a batch reuses the sampler (2 batches x 2 epochs of training, 2 of validation each)
    assert 0 < crit.builds <= 8
    # every other loss is called exactly as before
    plain = _Plain()
    cfg = gfd.nn.TrainConfig(name="plain", folder=str(tmp_path), epochs=1, num_steps=[2], training_loss=plain, validation_loss=plain, lr=2e-3,
                             batch_size=2, device=DEV)
    model.fit(cfg, train, train)
    assert len(plain.calls) == 8 and all(c == (3, {}) for c in plain.calls)


def test_zz_print_the_measured_ratios():
    """Not a check of its own: the measured / allowed ratio of every bound above, for tests/SAMPLE_LOSS_MEASURED.md (pytest -s)."""
    for k, v in sorted(RATIOS.items()):
        print(f"MEASURED {k}: {v:.3f}")
        assert v <= 1.0
