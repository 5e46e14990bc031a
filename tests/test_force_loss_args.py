"""Every argument error of gfd.nn.ForceLoss, gfd.BodyForces.adjoint and ops.body_forces_adjoint is raised in Python, on the arguments
as they were passed, before the library is touched: `_lib.load` is replaced by a function that fails the test."""
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import graphs4cfd_amd as gfd                               # noqa: E402
from graphs4cfd_amd import _lib, ops                       # noqa: E402

F32, F64, I32 = torch.float32, torch.float64, torch.int32
N, W, B, Q = 9, 5, 2, 7


@pytest.fixture(autouse=True)
def no_library(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", refuse)
    monkeypatch.setattr(_lib, "require_hip", refuse)


def raises(word, fn, *a, kind=ValueError, **k):
    with pytest.raises(kind, match=word) as e:
        fn(*a, **k)
    return str(e.value)


def test_the_symbol_is_declared():
    assert "g4c_body_forces_adjoint" in _lib.EXPORTED_SYMBOLS
    assert [f[0] for f in _lib.g4c_body_forces_adjoint_t._fields_][:6] == ["gF", "gwall", "nf", "pcol", "ucol", "vcol"]


def good():
    return dict(gF=torch.zeros(B, 6, dtype=F64), gwall=torch.zeros(W, 2), item_body=torch.zeros(W, dtype=I32), area=torch.zeros(W, 2, dtype=F64),
                unit=torch.zeros(W, 2, dtype=F64), arm=torch.zeros(W, 2, dtype=F64), own_off=torch.zeros(N + 1, dtype=I32),
                own_item=torch.zeros(W, dtype=I32), n_bodies=B, nf=3, pcol=2, ucol=0, vcol=1, mu=0.5, g=torch.zeros(11, 2),
                off=torch.zeros(N + 1, dtype=I32), in_off=torch.zeros(N + 1, dtype=I32), in_item=torch.zeros(Q, dtype=I32), in_g=torch.zeros(Q, 2))


def test_body_forces_adjoint_arguments():
    a = ops.body_forces_adjoint
    for kw, word in ((dict(nf=0), "^nf:"), (dict(nf=True), "^nf:"), (dict(nf=3.0), "^nf:"), (dict(n_bodies=-1), "^n_bodies:"),
                     (dict(mu="1"), "^mu:"), (dict(p_scale=None), "^p_scale:"), (dict(u_scale=True), "^u_scale:"), (dict(v_scale="x"), "^v_scale:"),
                     (dict(pcol=3), "^pcol:"), (dict(pcol=-1), "^pcol:"), (dict(ucol=3), "^ucol:"), (dict(vcol=1.0), "^vcol:"),
                     (dict(ucol=2), "distinct"), (dict(vcol=0), "distinct"),
                     (dict(item_body=torch.zeros(W, dtype=torch.int64)), "^item_body:"), (dict(area=torch.zeros(W, 2)), "^area:"),
                     (dict(unit=torch.zeros(W + 1, 2, dtype=F64)), "^unit:"), (dict(arm=torch.zeros(W, 3, dtype=F64)), "^arm:"),
                     (dict(own_off=torch.zeros(0, dtype=I32)), "^own_off:"), (dict(own_item=torch.zeros(W + 1, dtype=I32)), "^own_item:"),
                     (dict(gF=torch.zeros(B, 6)), "^gF:"), (dict(gF=torch.zeros(B + 1, 6, dtype=F64)), "^gF:"),
                     (dict(gF=torch.zeros(1, 1, dtype=F64).expand(B, 6)), "^gF:"),          # a stride-0 view: made dense by the caller
                     (dict(gwall=torch.zeros(W, 2, dtype=F64)), "^gwall:"), (dict(gwall=torch.zeros(W, 4)[:, ::2]), "^gwall:"),
                     (dict(g=None), "^g:.*mu != 0"), (dict(off=None), "^off:.*mu != 0"), (dict(in_off=None), "^in_off:.*mu != 0"),
                     (dict(in_item=None), "^in_item:"), (dict(in_g=None), "^in_g:"), (dict(g=torch.zeros(11, 3)), "^g:"),
                     (dict(off=torch.zeros(N, dtype=I32)), "^off:"), (dict(in_off=torch.zeros(N + 2, dtype=I32)), "^in_off:"),
                     (dict(in_g=torch.zeros(Q + 1, 2)), "^in_g:"), (dict(hw=torch.zeros(W, 4)), "^hw:"), (dict(out=torch.zeros(N, 4)), "^out:"),
                     (dict(out=torch.zeros(N, 3, dtype=F64)), "^out:")):
        k = good()
        k.update(kw)
        raises(word, a, **k)
    both = torch.zeros(N * 3 + W * 2)
    k = good()
    k.update(gwall=both[:W * 2].view(W, 2), out=both[W * 2:].view(N, 3))
    raises("^out:.*shares its storage with gwall", a, **k)
    k = good()
    k.update(mu=0.0, g=None, off=None, in_off=None, in_item=None, in_g=None, ucol=2, vcol=2)          # mu == 0: none of them is looked at
    raises("^item_body:.*HIP device only", a, **k)
    raises("^item_body:.*HIP device only", a, **good())
    k = good()
    k.update(in_item=torch.empty(2 ** 31, dtype=I32, device="meta"), in_g=torch.empty((2 ** 31, 2), device="meta"))
    raises("int32 offsets", a, kind=NotImplementedError, **k)


def operator(mu=0.5, scale=None):
    op = gfd.BodyForces.__new__(gfd.BodyForces)
    op.n_nodes, op.n_bodies, op.mu, op.pressure, op.velocity, op.scale, op.shift = N, B, mu, 2, (0, 1), scale, None
    op.items, op.area, op._adjoint_tables = torch.zeros(W, dtype=torch.int64), torch.zeros(W, 2, dtype=F64), None
    return op


def test_body_forces_adjoint_method_on_shapes_and_dtypes_alone():
    op = operator()
    for bad in (2, 0, 3.0, True, "3"):
        raises("^nf:", op.adjoint, nf=bad)
    assert raises("^nf:", operator(mu=0.0).adjoint, nf=2)          # the pressure is field 2
    for bad in (torch.zeros(B, 6), torch.zeros(B, 5, dtype=F64), torch.zeros(B + 1, 6, dtype=F64), [[0.0] * 6] * B):
        raises("^gF:", op.adjoint, gF=bad)
    for bad in (torch.zeros(W, 2, dtype=F64), torch.zeros(W, 3), torch.zeros(W), 1.0):
        raises("^gwall:", op.adjoint, gwall=bad)
    raises("^gwall:.*no CPU fallback", op.adjoint, gwall=torch.zeros(W, 2, device="meta"))


def test_too_many_list_entries_are_refused_from_the_shapes_alone():
    op = operator()
    op.items = torch.empty(2 ** 28, dtype=torch.int64, device="meta")          # no storage: the shapes alone
    op.gradient = types.SimpleNamespace(max_deg=8)
    raises("268435456 · 8", op._node_side, kind=NotImplementedError)


def test_force_loss_constructor_arguments():
    L = gfd.nn.ForceLoss
    for name in ("lambda_d", "weight", "node_weight"):
        for bad in (-1, -0.5, float("nan"), float("inf"), "1", None, True, torch.tensor(1.0)):
            raises(f"^{name}:", L, **{name: bad})
    for bad in (float("nan"), float("inf"), "1", None, True):
        raises("^mu:", L, mu=bad)
    for bad in (-1, 1.0, True, "p"):
        raises("^pressure:", L, pressure=bad)
    for bad in (3, (0,), (0, 1, 2), (0, -1), (0.0, 1.0), (True, 1)):
        raises("^velocity:", L, velocity=bad)
    for name in ("scale", "shift"):
        for bad in (3, (), ("a",), (1.0, float("nan")), (float("inf"),)):
            raises(f"^{name}:", L, **{name: bad})
    for bad in ((), ("fz",), ("fx", "fx"), 3, ("fx", 1)):
        raises("^components:", L, components=bad)
    for bad in (0, -1.0, float("nan"), float("inf"), "1", None, True):
        raises("^force_scale:", L, force_scale=bad)
    for bad in (3, ("pressure", 1.0), {"cp": 1.0}, {"pressure": 1.0, "tau": 2.0}):
        raises("^wall:", L, kind=TypeError, wall=bad)
    for key in ("pressure", "shear"):
        for bad in (-1, float("nan"), float("inf"), "1", None, True):
            raises(rf"^wall\['{key}'\]:", L, wall={key: bad})
    for bad in ("", 3, "loads_index", ["loads"]):
        raises("^values:", L, values=bad)
    for name in ("nodes", "bodies", "edge_vectors"):
        for bad in ("", 3, torch.zeros(3, dtype=torch.bool), ["wall"]):
            raises(f"^{name}:", L, kind=TypeError, **{name: bad})
    for bad in ("c", (0.0,), (0.0, float("nan")), ()):
        raises("^centre:", L, centre=bad)
    for bad in (3, -1, 1.0, True, None, "2"):
        raises("^power:", L, power=bad)
    ok = L(0.25, 2, 0, mu=0.01, pressure=2, velocity=[0, 1], scale=torch.ones(3), shift=[0, 0, 0], components="m", force_scale=0.5,
           wall={"pressure": 1, "shear": 0}, values="loads", nodes="wall", bodies="which", centre=(0.0, 0.0), power=1, edge_vectors="rel")
    assert ok.takes_step is True and ok.builds == 0 and ok.components == ("m",) and ok.scale == [1.0, 1.0, 1.0] and ok.velocity == (0, 1)
    assert (ok.wall_pressure, ok.wall_shear) == (1.0, 0.0)
    import graphs4cfd
    assert graphs4cfd.nn.ForceLoss is L and graphs4cfd.nn.losses.ForceLoss is L


def test_force_loss_call_arguments():
    L = gfd.nn.ForceLoss
    pred = torch.zeros(N, 3)
    bound = torch.zeros(N, dtype=torch.long)
    bound[:4] = 4
    pos = torch.zeros(N, 2)
    pos[:4] = torch.tensor([[1.0, 0.0], [0.0, 1.0], [-1.0, 0.0], [0.0, -1.0]])          # a square of four wall nodes
    graph = gfd.Graph(pos=pos, omega=torch.zeros(N, 1), bound=bound)
    raises("^step:", L(values="loads"), graph, pred, pred)                      # measured loads are per output step
    raises("^graph:", L(), gfd.Graph(x=pred), pred, pred)
    raises("^nodes:", L(), gfd.Graph(pos=torch.zeros(N, 2)), pred, pred)        # no bound, no nodes=
    raises("^nodes:", L(nodes="wall"), graph, pred, pred)
    raises("^nodes:", L(nodes="omega"), graph, pred, pred)                      # a floating-point attribute
    raises("^bodies:", L(bodies="which"), graph, pred, pred)
    graph.which = torch.zeros(N, dtype=torch.bool)
    raises("^bodies:", L(bodies="which"), graph, pred, pred)
    raises("^edge_vectors:", L(edge_vectors="rel"), graph, pred, pred)
    raises("HIP device only", L(), graph, pred, pred)                           # everything else is in order: there is no CPU path
    # weight = 0 and no wall weight: GraphLoss alone — nothing is built, on the host as well, with or without a step
    a, b = torch.randn(N, 3, generator=torch.Generator().manual_seed(0)), torch.randn(N, 3, generator=torch.Generator().manual_seed(1))
    base = gfd.nn.GraphLoss(0)
    for crit in (L(weight=0, values="loads"), L(weight=0, wall={"pressure": 0, "shear": 0.0})):
        assert torch.equal(crit(graph, a, b), base(graph, a, b)) and torch.equal(crit(graph, a, b, step=1), base(graph, a, b)) and crit.builds == 0
    assert torch.equal(L(0, 0, 0.5)(graph, a, b), 0.5 * base(graph, a, b))
