"""Every ValueError of gfd.nn.FlowLoss, gfd.MeshGradient.adjoint and ops.mesh_derived_adjoint is raised in Python, on the arguments as
they were passed, before the library is touched: `_lib.load` is replaced by a function that fails the test."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import graphs4cfd_amd as gfd                               # noqa: E402
from graphs4cfd_amd import _lib, ops                       # noqa: E402

F32, F64, I32 = torch.float32, torch.float64, torch.int32
N, E, K = 6, 12, 2


@pytest.fixture(autouse=True)
def no_library(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", refuse)
    monkeypatch.setattr(_lib, "require_hip", refuse)


def raises(word, fn, *a, **k):
    with pytest.raises(ValueError, match=word) as e:
        fn(*a, **k)
    return str(e.value)


def test_mesh_derived_adjoint_arguments():
    off, g, idx = torch.arange(0, E + 1, K, dtype=I32), torch.zeros(E, 2), torch.zeros(E, dtype=I32)
    prog, gy = [[(0, 0, 1.0), (1, 1, 1.0)]], torch.zeros(N, 1)
    a = ops.mesh_derived_adjoint
    raises("^g:", a, gy, off, g.double(), off, g, idx, prog, 3)
    raises("^g:", a, gy, off, torch.zeros(E, 4), off, g, idx, prog, 3)
    raises("^g:", a, gy, off, torch.zeros(2, E).t(), off, g, idx, prog, 3)
    for nf in (0, -1, 3.0, True, None):
        raises("^nf:", a, gy, off, g, off, g, idx, prog, nf)
    raises("^program", a, gy, off, g, off, g, idx, [], 3)
    raises("^program", a, gy, off, g, off, g, idx, [[(0, 0, 1.0)]] * 9, 3)
    raises("^program", a, gy, off, g, off, g, idx, [[(0, 0, 1.0)] * 4], 3)
    raises("^program.*field", a, gy, off, g, off, g, idx, [[(3, 0, 1.0)]], 3)
    raises("^program.*field", a, gy, off, g, off, g, idx, prog, 1)
    raises("^program.*axis", a, gy, off, g, off, g, idx, [[(0, 2, 1.0)]], 3)
    raises("^gy:", a, gy.double(), off, g, off, g, idx, prog, 3)
    raises("^gy:", a, torch.zeros(N, 2), off, g, off, g, idx, prog, 3)
    raises("^gy:", a, torch.zeros(N), off, g, off, g, idx, prog, 3)
    raises("^gy:", a, torch.zeros(N, 1).expand(N, 2)[:, :1], off, g, off, g, idx, prog, 3)          # a stride-0 view: made dense by the caller
    raises("^off:", a, gy, off[:-1], g, off, g, idx, prog, 3)
    raises("^off:", a, gy, off.long(), g, off, g, idx, prog, 3)
    raises("^out_off:", a, gy, off, g, off[:-1], g, idx, prog, 3)
    raises("^out_off:", a, gy, off, g, off.long(), g, idx, prog, 3)
    raises("^out_g:", a, gy, off, g, off, g[:-1], idx, prog, 3)
    raises("^out_g:", a, gy, off, g, off, g.double(), idx, prog, 3)
    raises("^out_g:", a, gy, off, g, off, torch.zeros(E, 3), idx, prog, 3)
    raises("^out_dst:", a, gy, off, g, off, g, idx[:-1], prog, 3)
    raises("^out_dst:", a, gy, off, g, off, g, idx.long(), prog, 3)
    raises("^gx:", a, gy, off, g, off, g, idx, prog, 3, torch.zeros(N, 2))
    raises("^gx:", a, gy, off, g, off, g, idx, prog, 3, torch.zeros(N, 3, dtype=F64))
    raises("^gx:", a, gy, off, g, off, g, idx, prog, 3, torch.zeros(3, N).t())
    both = torch.zeros(N, 4)
    raises("^gx:.*gy", a, both[:, :1].contiguous().set_(both.untyped_storage(), 0, (N, 1)), off, g, off, g, idx, prog, 3,
           torch.empty(0).set_(both.untyped_storage(), 0, (N, 3)))
    raises("^gx:.*gy", a, gy, off, g, off, g, idx, [[(0, 0, 1.0)]], 1, gy)
    raises("^gy.*HIP", a, gy, off, g, off, g, idx, prog, 3, torch.zeros(N, 3))          # everything else in order: a host tensor
    assert "g4c_mesh_derived_adjoint" in _lib.EXPORTED_SYMBOLS


def host_operator(dim=2):
    """A MeshGradient with host tables (the class itself refuses to be built off the device): enough for `adjoint` to check its
    arguments against."""
    op = object.__new__(gfd.MeshGradient)
    op.dim, op.n_nodes, op.power = dim, N, 2
    op.off, op.g, op.src = torch.arange(0, E + 1, K, dtype=I32), torch.zeros(E, dim), torch.zeros(E, dtype=I32)
    op._adjoint_tables = None
    return op


def test_mesh_gradient_adjoint_arguments():
    op = host_operator()
    gy = torch.zeros(N, 2)
    for nf in (0, 2.0, False, None):
        raises("^nf", op.adjoint, gy, ("div", "vort"), nf)
    raises("unknown name", op.adjoint, gy, ("curl",), 3)
    raises("expected", op.adjoint, gy, (), 3)
    raises("needs the velocity", op.adjoint, gy, ("div", "vort"), 1)
    raises("field 3", op.adjoint, gy, ("grad:3",), 3)
    raises("^velocity", op.adjoint, gy, ("div", "vort"), 3, velocity=(0,))
    raises("^field_scale", op.adjoint, gy, ("div", "vort"), 3, field_scale=[1.0])
    raises("^gy", op.adjoint, gy.double(), ("div", "vort"), 3)
    raises("^gy", op.adjoint, torch.zeros(N, 3), ("div", "vort"), 3)
    raises("^gy", op.adjoint, torch.zeros(N - 1, 2), ("div", "vort"), 3)
    raises("^gy", op.adjoint, torch.zeros(N * 2), ("div", "vort"), 3)
    raises("^gy", op.adjoint, [[0.0, 0.0]] * N, ("div", "vort"), 3)
    op.g = torch.zeros(E, 2, device="meta")
    raises("^gy: on 'cpu'", op.adjoint, gy, ("div", "vort"), 3)
    raises("^x", op.derived, torch.zeros(N, 3, dtype=F64, requires_grad=True), ("div",))


def small_graph(dim=2, nf=3):
    gen = torch.Generator().manual_seed(0)
    g = gfd.Graph(pos=torch.rand(N, dim, generator=gen))
    col = torch.arange(N).repeat_interleave(K)
    g.edge_index = torch.stack([(col + 1 + torch.arange(E) % K) % N, col])
    g.edge_attr = g.pos[g.edge_index[1]] - g.pos[g.edge_index[0]]
    g.field = torch.randn(N, nf, generator=gen)
    return g


def test_flow_loss_arguments():
    FL = gfd.nn.FlowLoss
    for lam in (-1, "a", None, float("nan"), True):
        raises("^lambda_d", FL, lam)
    raises("^terms", FL, 0, [("div", 1.0)])
    raises("^terms", FL, 0, "div")
    raises("^terms.*unknown name", FL, 0, {"curl": 1.0})
    raises("^terms.*unknown name", FL, 0, {"grad:u": 1.0})
    raises("^terms.*unknown name", FL, 0, {3: 1.0})
    for w in (-0.1, "1", None, float("inf"), False):
        raises(r"^terms\['div'\]", FL, 0, {"div": w})
    raises("^zero", FL, 0, {"div": 1.0}, zero=3)
    raises("^zero.*unknown name", FL, 0, {"div": 1.0}, zero=("divergence",))
    for power in (3, 2.0, False):
        raises("^power", FL, 0, {"div": 1.0}, power=power)
    for velocity in (1, (0,), (0, 1, 2, 3), (0, -1), (0, 1.0)):
        raises("^velocity", FL, 0, {"div": 1.0}, velocity=velocity)
    for scale in (2.0, [], ["a"], [1.0, float("nan")]):
        raises("^field_scale", FL, 0, {"div": 1.0}, field_scale=scale)
    for ev in (torch.zeros(E, 2), "", 3):
        raises("^edge_vectors", FL, 0, {"div": 1.0}, edge_vectors=ev)
    import graphs4cfd
    assert graphs4cfd.nn.FlowLoss is FL and graphs4cfd.nn.losses.FlowLoss is FL
    ok = FL(0.25, {"div": 0.1, "vort": 0.05, "grad:2": 0.0}, zero="div", velocity=[0, 1], field_scale=torch.ones(3), edge_vectors="edge_attr")
    assert ok._on_pred == [("div", 0.1)] and ok._on_error == [("vort", 0.05)] and ok.zero == ("div",) and ok.builds == 0


def test_flow_loss_at_call_time():
    g = small_graph()
    pred, target = torch.randn(N, 3, requires_grad=True), torch.randn(N, 3)
    crit = gfd.nn.FlowLoss(0, {"div": 0.1})
    raises("^graph.*HIP", crit, g, pred, target)                                   # as MeshGradient: there is no CPU fallback
    raises("^edge_vectors", gfd.nn.FlowLoss(0, {"div": 0.1}, edge_vectors="wrapped"), g, pred, target)
    raises("^graph", crit, gfd.Graph(pos=g.pos), pred, target)
    # nothing to launch: GraphLoss itself, bit for bit, on any device
    for terms in ({}, None, {"div": 0.0, "vort": 0}):
        flow, plain = gfd.nn.FlowLoss(0, terms), gfd.nn.GraphLoss(0)
        a, b = flow(g, pred, target), plain(g, pred, target)
        ga, gb = torch.autograd.grad(a, pred)[0], torch.autograd.grad(b, pred)[0]
        assert torch.equal(a, b) and torch.equal(ga, gb) and flow.builds == 0
