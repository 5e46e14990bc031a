"""Every ValueError of gfd.MeshJet, ops.mesh_jet_weights, ops.mesh_jet, ops.mesh_jet_adjoint and ops.derived_program(order=2) is raised
in Python, on the arguments as they were passed, before the library is touched: `_lib.load` is replaced by a function that fails
the test."""
import os
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import graphs4cfd_amd as gfd                               # noqa: E402
from graphs4cfd_amd import _lib, mesh_jet, ops             # noqa: E402

F32, F64, I32 = torch.float32, torch.float64, torch.int32
N, K, Q = 8, 5, 5
S = N * K


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


def tables():
    return torch.arange(0, S + 1, K, dtype=I32), torch.zeros(S, Q), torch.zeros(S, dtype=I32)


def test_derived_program_of_order_two():
    p = ops.derived_program([[(0, 4, 1.0)], [(1, 2, 0.5), (1, 4, 0.5)]], 2, 2, order=2)
    assert p.nd == 2 and p.axis[0][0] == 4 and ops.derived_program(p, order=2) is p
    assert ops.derived_program([[(0, 8, 1.0)]], 1, 3, order=2).axis[0][0] == 8
    raises("^program.*axis 5", ops.derived_program, [[(0, 5, 1.0)]], 1, 2, order=2)
    raises("^program.*axis 9", ops.derived_program, [[(0, 9, 1.0)]], 1, 3, order=2)
    raises("^program.*axis 2", ops.derived_program, [[(0, 2, 1.0)]], 1, 2)          # order 1 is unchanged
    raises("^program.*axis 2", ops.derived_program, [[(0, 2, 1.0)]], 1, 2, order=1)
    for order in (0, 3, True, None, "2"):
        raises("^order", ops.derived_program, [[(0, 0, 1.0)]], 1, 2, order=order)
    raises("^dim", ops.derived_program, [[(0, 0, 1.0)]], 1, 4, order=2)
    assert ops.jet_size(2) == 5 and ops.jet_size(3) == 9


def test_mesh_jet_weights_arguments():
    off, _, idx = tables()
    rel, csr = torch.zeros(S, 2), SimpleNamespace(off=off, perm=None, n=S)
    w = ops.mesh_jet_weights
    for power in (3, -1, 2.0, True, None):
        raises("^power", w, rel, csr, idx, power)
    raises("^rel", w, rel.double(), csr, idx)
    raises("^rel", w, torch.zeros(S, 4), csr, idx)
    raises("^rel", w, torch.zeros(S), csr, idx)
    raises("^rel", w, torch.zeros(2, S).t(), csr, idx)
    raises(r"^csr\.off", w, rel, SimpleNamespace(off=off.long(), perm=None, n=S), idx)
    raises(r"^csr\.off", w, rel, SimpleNamespace(off=torch.zeros(0, dtype=I32), perm=None, n=S), idx)
    raises("^csr:", w, rel, SimpleNamespace(off=off, perm=None, n=S - 1), idx)
    raises(r"^csr\.perm", w, rel, SimpleNamespace(off=off, perm=idx[:-1], n=S), idx)
    raises(r"^csr\.perm", w, rel, SimpleNamespace(off=off, perm=idx.long(), n=S), idx)
    raises("^src32", w, rel, csr, idx.long())
    raises("^src32", w, rel, csr, idx[:-1])
    good = (torch.zeros(S, Q), torch.zeros(S, dtype=I32), torch.zeros(N, dtype=torch.uint8))
    raises(r"^out\[0\]", w, rel, csr, idx, 2, (torch.zeros(S, 2), good[1], good[2]))
    raises(r"^out\[1\]", w, rel, csr, idx, 2, (good[0], good[1].long(), good[2]))
    raises(r"^out\[2\]", w, rel, csr, idx, 2, (good[0], good[1], torch.zeros(N, dtype=torch.bool)))
    raises("^rel.*HIP", w, rel, csr, idx)          # everything else in order: a host tensor


def test_mesh_jet_arguments():
    off, c, idx = tables()
    x, prog = torch.zeros(N, 3), [[(0, 2, 1.0), (0, 4, 1.0)]]
    j = ops.mesh_jet
    raises("^c:", j, x, off, c.double(), idx, prog)
    raises("^c:", j, x, off, torch.zeros(S, 2), idx, prog)          # a gradient table is no jet table
    raises("^c:", j, x, off, torch.zeros(S, 6), idx, prog)
    raises("^x:", j, x.double(), off, c, idx, prog)
    raises("^x:", j, torch.zeros(N), off, c, idx, prog)
    raises("^x:", j, torch.zeros(3, N).t(), off, c, idx, prog)
    raises("^nf:", j, x, off, c, idx, prog, nf=4)
    raises("^nf:", j, x, off, c, idx, prog, nf=0)
    raises("^off:", j, x, off[:-1], c, idx, prog)
    raises("^src:", j, x, off, c, idx.long(), prog)
    raises("^program", j, x, off, c, idx, [])
    raises("^program", j, x, off, c, idx, [[(0, 0, 1.0)]] * 9)
    raises("^program", j, x, off, c, idx, [[(0, 0, 1.0)] * 4])
    raises("^program.*field", j, x, off, c, idx, [[(3, 0, 1.0)]])
    raises("^program.*axis", j, x, off, c, idx, [[(0, 5, 1.0)]])
    raises("^program.*distinct fields", j, torch.zeros(N, 5), off, c, idx, [[(f, 0, 1.0)] for f in range(5)])
    raises("^out:", j, x, off, c, idx, prog, torch.zeros(N, 2))
    raises("^out:", j, x, off, c, idx, prog, torch.zeros(N, 1, dtype=F64))
    raises("^x.*HIP", j, x, off, c, idx, prog)


def test_mesh_jet_adjoint_arguments():
    off, c, idx = tables()
    prog, gy = [[(0, 2, 1.0), (1, 4, 1.0)]], torch.zeros(N, 1)
    a = ops.mesh_jet_adjoint
    raises("^c:", a, gy, off, c.double(), off, c, idx, prog, 3)
    raises("^c:", a, gy, off, torch.zeros(S, 3), off, c, idx, prog, 3)
    for nf in (0, -1, 3.0, True, None):
        raises("^nf:", a, gy, off, c, off, c, idx, prog, nf)
    raises("^program", a, gy, off, c, off, c, idx, [], 3)
    raises("^program.*field", a, gy, off, c, off, c, idx, prog, 1)
    raises("^program.*axis", a, gy, off, c, off, c, idx, [[(0, 5, 1.0)]], 3)
    raises("^program.*distinct fields", a, torch.zeros(N, 5), off, c, off, c, idx, [[(f, 0, 1.0)] for f in range(5)], 5)
    raises("^gy:", a, gy.double(), off, c, off, c, idx, prog, 3)
    raises("^gy:", a, torch.zeros(N, 2), off, c, off, c, idx, prog, 3)
    raises("^gy:", a, torch.zeros(N, 1).expand(N, 2)[:, :1], off, c, off, c, idx, prog, 3)
    raises("^off:", a, gy, off[:-1], c, off, c, idx, prog, 3)
    raises("^out_off:", a, gy, off, c, off.long(), c, idx, prog, 3)
    raises("^out_c:", a, gy, off, c, off, c[:-1], idx, prog, 3)
    raises("^out_c:", a, gy, off, c, off, torch.zeros(S, 9), idx, prog, 3)
    raises("^out_dst:", a, gy, off, c, off, c, idx.long(), prog, 3)
    raises("^gx:", a, gy, off, c, off, c, idx, prog, 3, torch.zeros(N, 2))
    raises("^gx:.*gy", a, gy, off, c, off, c, idx, [[(0, 0, 1.0)]], 1, gy)
    raises("^gy.*HIP", a, gy, off, c, off, c, idx, prog, 3, torch.zeros(N, 3))
    for name in ("g4c_mesh_jet_weights", "g4c_mesh_jet", "g4c_mesh_jet_adjoint"):
        assert name in _lib.EXPORTED_SYMBOLS


def small_graph(dim=2, n=40):
    gen = torch.Generator().manual_seed(0)
    g = gfd.Graph(pos=torch.rand(n, dim, generator=gen))
    col = torch.arange(n).repeat_interleave(6)
    g.edge_index = torch.stack([(col + 1 + torch.arange(6 * n) % 6) % n, col])
    g.edge_attr = g.pos[g.edge_index[1]] - g.pos[g.edge_index[0]]
    return g


def test_mesh_jet_constructor():
    g = small_graph()
    MJ = gfd.MeshJet
    for power in (3, 2.0, False, None):
        raises("^power", MJ, g, power=power)
        raises("^power", MJ, g, 12, power)
    for k in (4, 33, 12.0, True, "12", 0, -1):
        raises("^k:", MJ, g, k)
    raises("^k:", MJ, small_graph(3), 8)          # Q = 9 in 3-D
    raises("^edge_vectors", MJ, g, 12, 2, g.edge_attr)          # the two stencils exclude each other
    raises("^edge_vectors", MJ, g, None, 2, g.edge_attr[:-1])
    raises("^edge_vectors", MJ, g, None, 2, g.edge_attr.long())
    raises("^graph", MJ, gfd.Graph(pos=g.pos), None)          # k=None needs the edges
    raises("^graph", MJ, gfd.Graph(edge_index=g.edge_index), 12)          # k= needs the positions
    raises("^graph", MJ, gfd.Graph(pos=torch.rand(40, 4)), 12)
    raises("^graph.*HIP", MJ, g, None)          # everything in order: a host graph, in-edges
    raises("^graph.*HIP", MJ, g, 12)            # ... and its own stencil
    import graphs4cfd
    assert graphs4cfd.MeshJet is MJ


def host_operator(dim=2):
    """A MeshJet with host tables (the class itself refuses to be built off the device): enough for `derived` and `adjoint` to check
    their arguments against."""
    q = ops.jet_size(dim)
    op = object.__new__(gfd.MeshJet)
    op.dim, op.n_nodes, op.power, op.k = dim, N, 2, None
    op.off, op.c, op.src = torch.arange(0, S + 1, K, dtype=I32), torch.zeros(S, q), torch.zeros(S, dtype=I32)
    op._adjoint_tables = None
    return op


def test_mesh_jet_names_and_call_arguments():
    assert mesh_jet.jet_columns(("lap:1", "hess:0", "div"), 2) == ["lap1", "d20/dxx", "d20/dxy", "d20/dyy", "div"]
    assert mesh_jet.jet_columns(("hess:2", "lap:0"), 3) == ["d22/dxx", "d22/dxy", "d22/dxz", "d22/dyy", "d22/dyz", "d22/dzz", "lap0"]
    raises("9 columns", mesh_jet.jet_columns, ("hess:2", "vort"), 3)
    assert mesh_jet.jet_terms(("lap:1",), 3, 2) == [[(1, 3, 1.0), (1, 6, 1.0), (1, 8, 1.0)]]
    assert mesh_jet.jet_terms(("hess:0",), 2, 1, field_scale=[0.5]) == [[(0, 2, 0.5)], [(0, 3, 0.5)], [(0, 4, 0.5)]]
    assert mesh_jet.jet_terms(("div", "grad:1"), 2, 2) == [[(0, 0, 1.0), (1, 1, 1.0)], [(1, 0, 1.0)], [(1, 1, 1.0)]]
    op = host_operator()
    gy = torch.zeros(N, 2)
    for nf in (0, 2.0, False, None):
        raises("^nf", op.adjoint, gy, ("div", "lap:0"), nf)
    raises("unknown name", op.adjoint, gy, ("laplacian:0",), 3)
    raises("unknown name", op.adjoint, gy, ("curl",), 3)
    raises("expected 'lap:<field>'", op.adjoint, gy, ("lap:u",), 3)
    raises("expected 'hess:<field>'", op.adjoint, gy, ("hess:",), 3)
    raises("expected", op.adjoint, gy, (), 3)
    raises("needs the velocity", op.adjoint, gy, ("div", "lap:0"), 1)
    raises("field 3", op.adjoint, gy, ("lap:3", "lap:0"), 3)
    raises("field 3", op.adjoint, torch.zeros(N, 3), ("hess:3",), 3)
    raises("9 columns", op.adjoint, gy, ("hess:0", "hess:1", "hess:2"), 3)
    raises("^velocity", op.adjoint, gy, ("lap:0", "lap:1"), 3, velocity=(0,))
    raises("^field_scale", op.adjoint, gy, ("lap:0", "lap:1"), 3, field_scale=[1.0])
    raises("^gy", op.adjoint, gy.double(), ("div", "lap:0"), 3)
    raises("^gy", op.adjoint, torch.zeros(N, 3), ("div", "lap:0"), 3)
    raises("^gy", op.adjoint, torch.zeros(N - 1, 2), ("div", "lap:0"), 3)
    raises("^program.*distinct fields", op.adjoint, torch.zeros(N, 5), tuple(f"lap:{f}" for f in range(5)), 5)
    op.c = torch.zeros(S, 5, device="meta")
    raises("^gy: on 'cpu'", op.adjoint, gy, ("div", "lap:0"), 3)
    raises("^x", op.derived, torch.zeros(N, 3, dtype=F64), ("lap:0",))
    raises("^x", op.derived, torch.zeros(N + 1, 3), ("lap:0",))
    raises("unknown name", op.derived, torch.zeros(N, 3), ("lapl:0",))
    assert "MeshJet(nodes=8, entries=40, dim=2, in-edges, power=2)" == repr(op)
