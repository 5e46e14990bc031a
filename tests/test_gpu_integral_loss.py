"""`gfd.nn.IntegralLoss` on a 2-D cloud of a few hundred nodes round a wall, alone and as a collated batch of two: every integral
the loss forms is `ControlVolumes.integrate`'s, bit for bit; the value is the table of its docstring restated in fp64 (`table` below),
within 64 · 2⁻⁵³ relative on the fp64 term and 2⁻²⁴ after the cast; with equal areas 'mse' is `F.mse_loss`; a batch is the mean of its
graphs; the gradient of a one-source loss is `ControlVolumes.adjoint` of the g that autograd derives from the restated table, bit for
bit, and a loss over S sources the sum of S such launches; 'enstrophy' / 'div2' reach the prediction through `MeshGradient.adjoint`;
the operators are kept per batch; and a fit runs on it, twice the same."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

import voronoi_ref as V                                  # noqa: E402
import graphs4cfd_amd as gfd                             # noqa: E402
from graphs4cfd_amd import synthetic as S                # noqa: E402

DEV = torch.device("cuda", 0)
NF = 3
ALL = {"mse": 1.0, "mse:2": 0.5, "rel_mse": 0.25, "int:1": 2.0, "ke": 1.5, "circulation": 0.75, "enstrophy": 0.125, "div2": 3.0}


def bits(t):
    t = t.detach().contiguous()
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def graph_of(n, counts, seed):
    """An annulus round its bodies: `nrm` [N, 2] the outward wall normals (zero rows off the wall), kNN edges, and fixed fields."""
    pos, _, nrm, _, _ = V.annulus_case(n, counts)
    g = gfd.Graph(pos=torch.from_numpy(pos).to(DEV))
    g.edge_index = S.connect_knn(g.pos, 6)[0]
    g.nrm = torch.from_numpy(nrm).to(DEV)
    gen = torch.Generator().manual_seed(seed)
    g.p = torch.randn((pos.shape[0], NF), generator=gen).to(DEV)
    g.t = torch.randn((pos.shape[0], NF), generator=gen).to(DEV)
    return g


@pytest.fixture(scope="module")
def world():
    """Two graphs, their collated batch and the batch's volumes and gradient operator, built once from public calls (never modified)."""
    g1, g2 = graph_of(300, (37,), 1), graph_of(420, (24, 16), 2)
    both = gfd.nn.collate([g1, g2])
    return dict(g1=g1, g2=g2, both=both, cv=gfd.ControlVolumes(both, normals=both.nrm), op=gfd.MeshGradient(both, power=2))


def loss_of(terms, **kw):
    kw.setdefault("node_weight", 0.0)
    return gfd.nn.IntegralLoss(terms=terms, normals="nrm", **kw)


def sources(terms, velocity=(0, 1)):
    """The entries per source the table needs — written out here, not taken from the loss."""
    e = {"error": [], "target": [], "fields": [], "derived": []}
    if any(n in terms for n in ("mse", "rel_mse", "mse:2")):
        e["error"] = [(f, f) for f in range(NF)] if ("mse" in terms or "rel_mse" in terms) else [(2, 2)]
    if "rel_mse" in terms:
        e["target"] = [(f, f) for f in range(NF)]
    if "int:1" in terms:
        e["fields"].append((1, -1))
    if "ke" in terms:
        e["fields"] += [(v, v) for v in velocity]
    cols = [c for c, names in (("vort", ("circulation", "enstrophy")), ("div", ("div2",))) if any(n in terms for n in names)]
    for name, form in (("circulation", lambda c: (c, -1)), ("enstrophy", lambda c: (c, c)), ("div2", lambda c: (c, c))):
        if name in terms:
            c = cols.index("div" if name == "div2" else "vort")
            e["derived"].append(form(c))
    return e, tuple(cols)


def integrals(cv, op, terms, pred, target, velocity=(0, 1)):
    """(the entries per source, V [G] and the per-graph integrals of every source) from public calls:
    `ControlVolumes.integrate(per_graph=True)`."""
    e, cols = sources(terms, velocity)
    one = torch.zeros((cv.n_nodes, 1), device=DEV)
    out = {"V": cv.integrate(one, [(-1, -1)], per_graph=True)[:, 0]}
    if e["error"]:
        out["error"] = cv.integrate(pred, e["error"], sub=target, per_graph=True)
    if e["target"]:
        out["target"] = cv.integrate(target, e["target"], per_graph=True)
    if e["fields"]:
        out["fields"] = cv.integrate(pred, e["fields"], per_graph=True)
        out["fields_target"] = cv.integrate(target, e["fields"], per_graph=True)
    if e["derived"]:
        out["derived"] = cv.integrate(op.derived(pred, cols, velocity=velocity), e["derived"], per_graph=True)
        out["derived_target"] = cv.integrate(op.derived(target, cols, velocity=velocity), e["derived"], per_graph=True)
    return e, out


def table(terms, e, s, velocity=(0, 1), weight=1.0):
    """The docstring's table in fp64 torch (on whatever device `s` lives): (the term, Σ|parts|)."""
    Vq = s["V"]
    total, parts = 0.0, 0.0
    for name, w in terms.items():
        if w == 0:
            continue
        if name == "mse":
            val = sum(s["error"][:, e["error"].index((f, f))] for f in range(NF)) / (NF * Vq)
        elif name == "mse:2":
            val = s["error"][:, e["error"].index((2, 2))] / Vq
        elif name == "rel_mse":
            val = sum(s["error"][:, e["error"].index((f, f))] for f in range(NF)) / sum(s["target"][:, e["target"].index((f, f))] for f in range(NF))
        else:
            def I(src):
                if name == "int:1":
                    return s[src][:, e["fields"].index((1, -1))]
                if name == "ke":
                    return 0.5 * sum(s[src][:, e["fields"].index((v, v))] for v in velocity)
                form = {"circulation": lambda c: (c, -1), "enstrophy": lambda c: (c, c), "div2": lambda c: (c, c)}[name]
                c = 0 if name != "div2" else max(max(pair) for pair in e["derived"])          # 'vort' comes first, 'div' last
                return (0.5 if name == "enstrophy" else 1.0) * s[src][:, e["derived"].index(form(c))]
            src = "fields" if name in ("int:1", "ke") else "derived"
            val = ((I(src) - I(src + "_target")) / Vq).square()
        part = w * val.mean()
        total = total + part
        parts = parts + part.detach().abs()
    return weight * total, weight * parts


# ====================================================================== the integrals and the value
@pytest.mark.parametrize("which", ["g1", "both"])
def test_every_integral_is_integrate_and_the_value_is_the_table(world, which):
    graph = world[which]
    cv = world["cv"] if which == "both" else gfd.ControlVolumes(graph, normals=graph.nrm)
    op = world["op"] if which == "both" else gfd.MeshGradient(graph, power=2)
    crit = loss_of(ALL, weight=0.5)
    Vq, sums, _ = crit.integrals(graph, graph.p, graph.t)
    e, want = integrals(cv, op, ALL, graph.p, graph.t)
    assert crit.plan(NF)[0] == e
    assert tuple(Vq.shape) == (len(cv.counts),) and torch.equal(bits(Vq), bits(want["V"]))
    assert set(sums) == set(want) - {"V"}
    for key in sums:
        assert sums[key].dtype == torch.float64 and torch.equal(bits(sums[key]), bits(want[key])), key
    # the value: fp64 table on the host from the same integrals
    term64, parts = table(ALL, e, {k: v.cpu() for k, v in want.items()}, weight=0.5)
    got = crit(graph, graph.p, graph.t)
    assert got.dtype == torch.float32 and got.dim() == 0
    err, allowed = abs(float(got) - float(term64)), 64 * 2.0 ** -53 * float(parts) + 2.0 ** -24 * abs(float(term64))
    print(f"{which}: loss {float(got)!r} fp64 {float(term64)!r} |diff| / allowed {err / allowed:.3e}")
    assert err <= allowed
    # every single term too
    for name, w in ALL.items():
        e1, s1 = integrals(cv, op, {name: w}, graph.p, graph.t)
        one64, p1 = table({name: w}, e1, {k: v.cpu() for k, v in s1.items()})
        one = loss_of({name: w})(graph, graph.p, graph.t)
        assert abs(float(one) - float(one64)) <= 64 * 2.0 ** -53 * float(p1) + 2.0 ** -24 * abs(float(one64)), name
    # the node term in front: GraphLoss's bits plus the term's
    with_node = loss_of(ALL, weight=0.5, node_weight=1.0)(graph, graph.p, graph.t)
    assert torch.equal(bits(with_node), bits(F.mse_loss(graph.p, graph.t) + got))


def test_with_equal_areas_mse_is_mse_loss():
    m, pitch = 16, 2.0 ** -5
    pos = V.lattice(m, pitch)
    g = gfd.Graph(pos=torch.from_numpy(pos).to(DEV))
    half, far = 0.5 * pitch, (m - 1) * pitch + 0.5 * pitch
    crit = gfd.nn.IntegralLoss(node_weight=0.0, terms={"mse": 1.0}, box=(-half, -half, far, far))
    cv, Vq, _ = crit.operators(g)
    assert bool((cv.area == pitch * pitch).all()) and float(Vq[0]) == (m * pitch) ** 2
    gen = torch.Generator().manual_seed(9)
    p, t = torch.randn((m * m, NF), generator=gen).to(DEV), torch.randn((m * m, NF), generator=gen).to(DEV)
    got, want = float(crit(g, p, t)), float(F.mse_loss(p, t))
    allowed = NF * m * m * 2.0 ** -24 * float((p - t).square().max())
    print(f"equal areas: IntegralLoss {got!r} mse_loss {want!r} |diff| / allowed {abs(got - want) / allowed:.3e}")
    assert abs(got - want) <= allowed


def test_a_batch_is_the_mean_of_its_graphs(world):
    for terms in (ALL, {"mse": 1.0}, {"ke": 1.0}):
        crit = loss_of(terms)
        l1, l2 = float(crit(world["g1"], world["g1"].p, world["g1"].t)), float(crit(world["g2"], world["g2"].p, world["g2"].t))
        lb = float(crit(world["both"], world["both"].p, world["both"].t))
        want = 0.5 * (l1 + l2)
        # three casts to float32 (2⁻²⁴ relative each: the two graphs' average to 2⁻²⁴ of the mean) and the fp64 algebra's 64 · 2⁻⁵³
        assert abs(lb - want) <= (2 * 2.0 ** -24 + 64 * 2.0 ** -53) * (abs(l1) + abs(l2)) / 2, (terms, lb, want)


# ====================================================================== the gradient
def upstream(terms, e, sums, weight=1.0):
    """g per source: autograd of the restated table (cast to float32, as the loss is) by the prediction's integrals."""
    leaves = {k: (v.detach().clone().requires_grad_(True) if k in ("error", "fields", "derived") else v.detach()) for k, v in sums.items()}
    term, _ = table(terms, e, leaves, weight=weight)
    term.to(torch.float32).backward()
    return {k: v.grad for k, v in leaves.items() if v.requires_grad}


@pytest.mark.parametrize("terms,source,kw", [({"ke": 1.0}, "fields", {}), ({"mse": 1.0}, "error", {}), ({"mse": 0.5}, "error", dict(weight=3.0))])
def test_the_gradient_of_a_one_source_loss_is_the_adjoint(world, terms, source, kw):
    graph, cv = world["both"], world["cv"]
    pred = graph.p.clone().requires_grad_(True)
    loss_of(terms, **kw)(graph, pred, graph.t).backward()
    e, sums = integrals(cv, None, terms, graph.p, graph.t)
    g = upstream(terms, e, sums, **kw)
    assert list(g) == [source]
    want = cv.adjoint(g[source], graph.p, e[source], sub=graph.t if source == "error" else None, per_graph=True)
    assert torch.equal(bits(pred.grad), bits(want))
    again = graph.p.clone().requires_grad_(True)
    loss_of(terms, **kw)(graph, again, graph.t).backward()
    assert torch.equal(bits(again.grad), bits(pred.grad))


def test_a_loss_over_two_sources_adds_two_launches(world):
    graph, cv = world["both"], world["cv"]
    terms = {"mse": 1.0, "rel_mse": 0.25, "int:1": 2.0, "ke": 1.5}
    pred = graph.p.clone().requires_grad_(True)
    loss_of(terms)(graph, pred, graph.t).backward()
    e, sums = integrals(cv, None, terms, graph.p, graph.t)
    g = upstream(terms, e, sums)
    assert sorted(g) == ["error", "fields"]
    parts = [cv.adjoint(g["error"], graph.p, e["error"], sub=graph.t, per_graph=True).double(),
             cv.adjoint(g["fields"], graph.p, e["fields"], per_graph=True).double()]
    err = (pred.grad.double() - (parts[0] + parts[1])).abs()
    allowed = len(parts) * 2.0 ** -24 * (parts[0].abs() + parts[1].abs())
    print(f"two sources: largest |grad − Σ parts| / allowed {float((err / allowed.clamp(min=1e-300)).max()):.3e}")
    assert bool((err <= allowed).all())


def test_the_derived_terms_reach_the_prediction_through_the_mesh_gradient(world):
    graph, cv, op = world["both"], world["cv"], world["op"]
    terms = {"enstrophy": 1.0, "div2": 0.5}
    pred = graph.p.clone().requires_grad_(True)
    got = loss_of(terms)(graph, pred, graph.t)
    got.backward()
    # the same chain from public calls: derived (recorded) -> integrate (recorded) -> the table -> float32
    chain = graph.p.clone().requires_grad_(True)
    e, sums = integrals(cv, op, terms, chain, graph.t)
    assert sums["derived"].requires_grad and not sums["derived_target"].requires_grad
    term, _ = table(terms, e, sums)
    want = term.to(torch.float32)
    want.backward()
    assert torch.equal(bits(got), bits(want)) and torch.equal(bits(pred.grad), bits(chain.grad))
    assert bool(pred.grad.abs().sum() > 0) and bool(torch.isfinite(pred.grad).all())
    # and by hand: the adjoint of the integrals, then MeshGradient.adjoint
    d = op.derived(graph.p, ("vort", "div"), velocity=(0, 1))
    g = upstream(terms, e, {k: v.detach() for k, v in sums.items()})["derived"]
    gd = cv.adjoint(g, d, e["derived"], per_graph=True)
    by_hand = op.adjoint(gd, ("vort", "div"), NF, velocity=(0, 1))
    assert torch.equal(bits(by_hand), bits(pred.grad))


# ====================================================================== the operator cache
def test_the_operators_are_kept_per_batch():
    graph = graph_of(300, (37,), 3)
    crit = loss_of({"mse": 1.0, "enstrophy": 1.0})
    first = crit(graph, graph.p, graph.t)
    assert crit.builds == 1
    assert torch.equal(bits(crit(graph, graph.p, graph.t)), bits(first)) and crit.builds == 1
    cv = crit.operators(graph)[0]
    graph.pos[5, 0] += 1e-3          # in place: the same object, another version
    moved = crit(graph, graph.p, graph.t)
    assert crit.builds == 2 and crit.operators(graph)[0] is not cv and not torch.equal(bits(moved), bits(first))
    crit(graph, graph.p, graph.t)
    assert crit.builds == 2
    # without a derived term the edges are not looked at
    plain = loss_of({"mse": 1.0})
    plain(graph, graph.p, graph.t)
    graph.edge_index = graph.edge_index[:, :-6].contiguous()
    plain(graph, graph.p, graph.t)
    assert plain.builds == 1
    crit(graph, graph.p, graph.t)
    assert crit.builds == 3


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


def test_two_fit_steps_are_finite_and_repeat_bit_for_bit(tmp_path):
    runs = []
    for attempt in range(2):
        torch.manual_seed(0)
        model = gfd.nn.NsTwoScaleGNN(arch=S.mus_arch("NsTwoScaleGNN", 32), device=DEV)
        coarsen = gfd.transforms.GridClustering(S.default_cells(300, 2, 2))
        train = gfd.DataLoader(_dataset(2, 300, 1), batch_size=2, shuffle=False, transform=coarsen)
        before = [p.detach().clone() for p in model.parameters()]
        crit = gfd.nn.IntegralLoss(0.25, 1.0, 0.5, terms={"mse": 1.0, "rel_mse": 0.1, "ke": 1.0, "enstrophy": 0.01, "div2": 0.01})
        cfg = gfd.nn.TrainConfig(name=f"integral{attempt}", folder=str(tmp_path), epochs=2, num_steps=[1], training_loss=crit,
                                 validation_loss=crit, lr=2e-3, batch_size=2, device=DEV)
        model.fit(cfg, train, train)          # one batch of two graphs an epoch: two steps
        h = model.history
        assert len(h) == 2 and all(np.isfinite(r["training_loss"]) and np.isfinite(r["validation_loss"]) and r["gradients_norm"] > 0 for r in h)
        after = [p.detach().clone() for p in model.parameters()]
        assert all(bool(torch.isfinite(p).all()) for p in after) and any(not torch.equal(a, b) for a, b in zip(before, after))
        assert 0 < crit.builds <= 4
        runs.append(after)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(*runs))
