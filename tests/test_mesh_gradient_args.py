"""Every ValueError of ops.mesh_gradient_weights / ops.mesh_derived, gfd.MeshGradient, Rollout(derived=) and GNN.diagnostics is
raised in Python, on the tensors as they were passed, before the library is touched: `_lib.load` is replaced by a function that
fails the test."""
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import graphs4cfd_amd as gfd                               # noqa: E402
from graphs4cfd_amd import _lib, ops                       # noqa: E402
from graphs4cfd_amd.nn.model import Rollout                # noqa: E402

F32, F64, I32, U8 = torch.float32, torch.float64, torch.int32, torch.uint8
N, E, K = 6, 12, 2


@pytest.fixture(autouse=True)
def no_library(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", refuse)
    monkeypatch.setattr(_lib, "require_hip", refuse)


def csr(off=None, perm=None, n=E):
    return types.SimpleNamespace(off=torch.arange(0, E + 1, K, dtype=I32) if off is None else off, perm=perm, n=n)


def raises(word, fn, *a, **k):
    with pytest.raises(ValueError, match=word) as e:
        fn(*a, **k)
    return str(e.value)


def test_mesh_gradient_weights_arguments():
    rel, src = torch.zeros(E, 2), torch.zeros(E, dtype=I32)
    w = ops.mesh_gradient_weights
    for power in (3, -1, 1.0, True, None):
        raises("^power", w, rel, csr(), src, power)
    raises("^rel", w, rel.double(), csr(), src)
    raises("^rel", w, torch.zeros(E, 4), csr(), src)
    raises("^rel", w, torch.zeros(E), csr(), src)
    raises("^rel", w, torch.zeros(2, E).t(), csr(), src)
    raises(r"^csr\.off", w, rel, csr(off=torch.arange(0, E + 1, K)), src)
    raises(r"^csr\.off", w, rel, csr(off=torch.zeros(0, dtype=I32)), src)
    raises("^csr", w, rel, csr(n=E + 1), src)
    raises(r"^csr\.perm", w, rel, csr(perm=torch.zeros(E - 1, dtype=I32)), src)
    raises(r"^csr\.perm", w, rel, csr(perm=torch.zeros(E, dtype=torch.int64)), src)
    raises("^src32", w, rel, csr(), src.long())
    raises("^src32", w, rel, csr(), src[:-1])
    out = (torch.zeros(E, 2), torch.zeros(E, dtype=I32), torch.zeros(N, dtype=U8))
    raises(r"^out\[0\]", w, rel, csr(), src, 2, (out[0][:, :1].contiguous(), out[1], out[2]))
    raises(r"^out\[1\]", w, rel, csr(), src, 2, (out[0], out[1].long(), out[2]))
    raises(r"^out\[2\]", w, rel, csr(), src, 2, (out[0], out[1], torch.zeros(N + 1, dtype=U8)))
    raises("^rel.*HIP", w, rel, csr(), src, 2, out)          # everything else in order: a host tensor


def test_mesh_derived_arguments():
    x, off, g, src = torch.zeros(N, 3), torch.arange(0, E + 1, K, dtype=I32), torch.zeros(E, 2), torch.zeros(E, dtype=I32)
    prog, cur = [[(0, 0, 1.0), (1, 1, 1.0)]], torch.zeros(N, 1)
    d = ops.mesh_derived
    raises("^g:", d, x, off, g.double(), src, prog, cur)
    raises("^g:", d, x, off, torch.zeros(E, 1), src, prog, cur)
    raises("^x:", d, x.double(), off, g, src, prog, cur)
    raises("^x:", d, torch.zeros(N), off, g, src, prog, cur)
    raises("^x:", d, torch.zeros(3, N).t(), off, g, src, prog, cur)
    raises("^nf:", d, x, off, g, src, prog, cur, nf=4)
    raises("^off:", d, x, off[:-1], g, src, prog, cur)
    raises("^off:", d, x, off.long(), g, src, prog, cur)
    raises("^src:", d, x, off, g, src[:-1], prog, cur)
    raises("^program", d, x, off, g, src, [], cur)
    raises("^program", d, x, off, g, src, [[(0, 0, 1.0)]] * 9, torch.zeros(N, 9))
    raises("^program", d, x, off, g, src, [[(0, 0, 1.0)] * 4], cur)
    raises("^program", d, x, off, g, src, [[]], cur)
    raises("^program.*field", d, x, off, g, src, [[(3, 0, 1.0)]], cur)
    raises("^program.*field", d, x, off, g, src, [[(2, 0, 1.0)]], cur, nf=2)
    raises("^program.*axis", d, x, off, g, src, [[(0, 2, 1.0)]], cur)
    raises("^program", d, x, off, g, src, [[(0.0, 0, 1.0)]], cur)
    raises("^program", d, x, off, g, src, 5, cur)
    raises("^cur:", d, x, off, g, src, prog, torch.zeros(N, 2))
    raises("^cur:", d, x, off, g, src, prog, cur.double())
    step, stats, scratch, snap = torch.zeros(2, dtype=I32), torch.zeros(4, 1, 3, dtype=F64), torch.zeros(11, dtype=F64), torch.zeros(2, N, 1)
    raises("^every:", d, x, off, g, src, prog, cur, step=step, every=-1)
    raises("^max_steps:", d, x, off, g, src, prog, cur, step=step, max_steps=-1)
    raises("^snap:", d, x, off, g, src, prog, cur, step=step, every=2)
    raises("^snap:", d, x, off, g, src, prog, cur, step=step, every=0, snap=snap)
    raises("^snap:", d, x, off, g, src, prog, cur, step=step, every=2, snap=torch.zeros(2, N, 2))
    raises("^scratch:", d, x, off, g, src, prog, cur, step=step, stats=stats, max_steps=4)
    raises("^stats:", d, x, off, g, src, prog, cur, step=step, scratch=scratch, max_steps=4)
    raises("^stats:", d, x, off, g, src, prog, cur, step=step, stats=stats, scratch=scratch, max_steps=5)
    raises("^scratch:", d, x, off, g, src, prog, cur, step=step, stats=stats, scratch=scratch[:-1], max_steps=4)
    raises("^step:", d, x, off, g, src, prog, cur, stats=stats, scratch=scratch, max_steps=4)
    raises("^step:", d, x, off, g, src, prog, cur, every=2, snap=snap)
    raises("^step:", d, x, off, g, src, prog, cur, step=step.long())
    raises("^x:.*HIP", d, x, off, g, src, prog, cur, step=step, every=2, snap=snap, stats=stats, scratch=scratch, max_steps=4)


def small_graph(dim=2, nf=3):
    gen = torch.Generator().manual_seed(0)
    g = gfd.Graph(pos=torch.rand(N, dim, generator=gen))
    col = torch.arange(N).repeat_interleave(K)
    g.edge_index = torch.stack([(col + 1 + torch.arange(E) % K) % N, col])
    g.edge_attr = g.pos[g.edge_index[1]] - g.pos[g.edge_index[0]]
    g.field = torch.randn(N, nf, generator=gen)
    return g


def test_mesh_gradient_class_arguments():
    g = small_graph()
    for power in (3, 2.0, False):
        raises("^power", gfd.MeshGradient, g, power)
    raises("^edge_vectors", gfd.MeshGradient, g, 2, torch.zeros(E - 1, 2))
    raises("^edge_vectors", gfd.MeshGradient, g, 2, torch.zeros(E, 4))
    raises("^edge_vectors", gfd.MeshGradient, g, 2, torch.zeros(E, 2, dtype=torch.int64))
    raises("^graph", gfd.MeshGradient, gfd.Graph(pos=g.pos))
    raises("^graph", gfd.MeshGradient, gfd.Graph(pos=torch.rand(N, 4), edge_index=g.edge_index))
    raises("^graph.*HIP", gfd.MeshGradient, g)
    import graphs4cfd
    assert graphs4cfd.MeshGradient is gfd.MeshGradient and gfd.nn.RolloutDerived is graphs4cfd.nn.RolloutDerived


def test_names_columns_and_programs():
    from graphs4cfd_amd.mesh_gradient import derived_columns, derived_terms
    assert derived_columns(("div", "vort", "grad:2"), 2) == ["div", "vort", "d2/dx", "d2/dy"]
    assert derived_columns("vort", 3) == ["vort_x", "vort_y", "vort_z"]
    assert derived_terms(("div", "vort"), 2, 3) == [[(0, 0, 1.0), (1, 1, 1.0)], [(1, 0, 1.0), (0, 1, -1.0)]]
    assert derived_terms(("vort",), 3, 3)[2] == [(1, 0, 1.0), (0, 1, -1.0)]
    assert derived_terms(("div",), 2, 3, velocity=(2, 0), field_scale=[2.0, 1.0, 0.5]) == [[(2, 0, 0.5), (0, 1, 2.0)]]
    raises("unknown name", derived_columns, ("curl",), 2)
    raises("expected", derived_columns, (), 2)
    raises("expected", derived_columns, (1,), 2)
    raises("grad:", derived_columns, ("grad:u",), 2)
    raises("columns", derived_columns, ("div", "vort", "grad:0", "grad:1", "grad:2", "grad:0"), 2)          # 10 columns
    raises("columns", derived_columns, ("vort", "grad:0", "grad:1"), 3)                                     # 9 columns
    raises("needs the velocity", derived_terms, ("div",), 2, 1)
    raises("needs the velocity", derived_terms, ("vort",), 3, 2)
    raises("field 3", derived_terms, ("grad:3",), 2, 3)
    raises("^velocity", derived_terms, ("div",), 2, 3, velocity=(0,))
    raises("^velocity", derived_terms, ("div",), 2, 3, velocity=(0, -1))
    raises("^field_scale", derived_terms, ("div",), 2, 3, field_scale=[1.0, 2.0])


class Model:
    num_fields = 3


def test_rollout_derived_arguments():
    g = small_graph()
    r = lambda **kw: Rollout(Model(), g, 8, **kw)          # noqa: E731
    raises("unknown name", r, derived=("curl",))
    raises("columns", r, derived=("div", "vort", "grad:0", "grad:1", "grad:2", "grad:0"))
    raises("^derived_every", r, derived=("div",), derived_every=-1)
    raises("^derived_every", r, derived=("div",), derived_every=1.5)
    raises("^derived_moments", r, derived=("div",), derived_moments=8)
    raises("^derived_moments", r, derived=("div",), derived_moments=(0, 0))
    raises("^derived_options", r, derived=("div",), derived_options=dict(weights=1))
    raises("^power", r, derived=("div",), derived_options=dict(power=5))
    raises("^edge_vectors", r, derived=("div",), derived_options=dict(edge_vectors=torch.zeros(3, 2)))
    raises("^velocity", r, derived=("div",), derived_options=dict(velocity=(0, 1, 2)))
    raises("^field_scale", r, derived=("div",), derived_options=dict(field_scale=[1.0]))
    raises("without derived", r, derived_every=2)
    raises("without derived", r, derived_moments=True)
    raises("without derived", r, derived_options=dict(power=1))
    one = Model()
    one.num_fields = 1
    raises("needs the velocity", Rollout, one, small_graph(nf=1), 8, derived=("div",))
    raises("^graph", Rollout, Model(), gfd.Graph(field=g.field, edge_index=g.edge_index), 8, derived=("div",))


def test_diagnostics_arguments():
    model = gfd.nn.NsOneScaleGNN(arch=gfd.synthetic.mus_arch("NsOneScaleGNN", 16), device=torch.device("cpu"))
    g = small_graph()
    raises("unknown name", model.diagnostics, g, 4, ("curl",))
    raises("^derived_every", model.diagnostics, g, 4, every=-2)
    raises("^derived_moments", model.diagnostics, g, 4, discard=4)
    raises("^derived_moments", model.diagnostics, g, 4, discard=0, stride=0)
    raises("^derived_options", model.diagnostics, g, 4, weights=2)
    raises("^power", model.diagnostics, g, 4, power=7)
    raises("edge_vectors of a list", model.diagnostics, [g, small_graph()], 4, edge_vectors=g.edge_attr)
    g.target = torch.zeros(N, 12)
    raises("unknown name", model.evaluate, g, 4, derived=("rot",))
