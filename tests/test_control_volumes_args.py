"""Every ValueError / TypeError of gfd.ControlVolumes, ops.voronoi_cells, ops.integral_program and ops.weighted_integrals is raised in
Python, on the arguments as they were passed, before the library is touched: `_lib.load` is replaced by a function that fails the
test."""
import os
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import graphs4cfd_amd as gfd                               # noqa: E402
from graphs4cfd_amd import _lib, control_volumes, ops      # noqa: E402

F32, F64, I32, U8 = torch.float32, torch.float64, torch.int32, torch.uint8
N = 8


@pytest.fixture(autouse=True)
def no_library(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", refuse)
    monkeypatch.setattr(_lib, "require_hip", refuse)


def raises(word, fn, *a, exc=ValueError, **k):
    with pytest.raises(exc, match=word) as e:
        fn(*a, **k)
    return str(e.value)


def graph(n=N, dim=2, **kw):
    return SimpleNamespace(pos=torch.rand(n, dim), **kw)


def grid(n=N, **kw):
    import ctypes as C
    g = dict(pos_sorted=torch.zeros(n, 2), order=torch.zeros(n, dtype=I32), cell_start=torch.zeros(7, dtype=I32), n_cells=[3, 2, 1],
             org=(C.c_float * 3)(0.0, 0.0, 0.0), h=0.5, dim=2, n=n)
    g.update(kw)
    return g


def test_the_exports():
    assert gfd.ControlVolumes is control_volumes.ControlVolumes
    for name in ("g4c_voronoi_cells", "g4c_weighted_integrals", "g4c_weighted_integrals_scratch_doubles"):
        assert name in _lib.EXPORTED_SYMBOLS
    assert (_lib.VORONOI_BOX, _lib.VORONOI_WALL, _lib.VORONOI_DUPLICATE, _lib.VORONOI_OVERFLOW) == (1, 2, 4, 8)
    assert _lib.VORONOI_MAX_VERTS == 32 and _lib.INTEGRALS_MAX_ENTRIES == 8


def test_control_volumes_arguments():
    cv = gfd.ControlVolumes
    raises("^graph.*pos", cv, SimpleNamespace())
    raises("^graph.*pos", cv, SimpleNamespace(pos=torch.zeros(N)))
    raises("^graph.*2-D only.*3-D cells", cv, graph(dim=3))
    raises("^graph.*empty", cv, graph(0))
    raises("^graph.*batch", cv, graph(batch=torch.zeros(N - 1, dtype=torch.long)))
    raises("^graph.*batch", cv, graph(batch=torch.zeros(N)))
    raises("^graph.*without nodes", cv, graph(batch=torch.tensor([0, 0, 0, 0, 2, 2, 2, 2])))
    for box in ((0, 0, 1), "box", (0, 0, 1, float("nan")), (0, 0, 0, 1), (1, 0, 0, 1), (0, 0, float("inf"), 1), 3.0):
        raises("^box", cv, graph(), box=box)
    raises("^box.*2 boxes.*1 graphs", cv, graph(), box=[(0, 0, 1, 1), (0, 0, 2, 2)])
    raises("^bodies", cv, graph(), bodies="wall", exc=TypeError)
    raises("^bodies", cv, graph(), bodies=False, exc=TypeError)
    raises("^normals.*bodies", cv, graph(), bodies=True, normals=torch.zeros(N, 2))
    raises("^normals", cv, graph(), normals=torch.zeros(N, 3))
    raises("^normals", cv, graph(), normals=torch.zeros(N, 2, dtype=torch.long))
    raises("^normals", cv, graph(), normals=[[0.0, 0.0]] * N)
    bad = torch.zeros(N, 2)
    bad[3, 1] = float("nan")
    raises("^normals.*finite", cv, graph(), normals=bad)
    raises("^graph.*HIP", cv, graph())          # everything else in order: a host tensor
    raises("^graph.*HIP", cv, graph(), box=(0, 0, 1, 1), normals=torch.zeros(N, 2))


def test_voronoi_cells_arguments():
    v = ops.voronoi_cells
    box = (0.0, 0.0, 1.0, 1.0)
    raises("^grid", v, None, box)
    raises("^grid.*'cell_start'", v, {k: w for k, w in grid().items() if k != "cell_start"}, box)
    raises("^grid.*periodic", v, grid(periods=[1.0, 0.0]), box)
    raises("^grid.*2-D only", v, grid(dim=3), box)
    raises(r"^grid\['pos_sorted'\]", v, grid(pos_sorted=torch.zeros(N, 3)), box)
    raises(r"^grid\['pos_sorted'\]", v, grid(pos_sorted=torch.zeros(N, 2, dtype=F64)), box)
    raises(r"^grid\['order'\]", v, grid(order=torch.zeros(N, dtype=torch.long)), box)
    raises(r"^grid\['n_cells'\]", v, grid(n_cells=[3, 2]), box)
    raises(r"^grid\['n_cells'\]", v, grid(n_cells=[3, 2, 2]), box)
    raises(r"^grid\['cell_start'\]", v, grid(cell_start=torch.zeros(6, dtype=I32)), box)
    for b in ((0, 0, 1), (0, 1, 1, 1), None):
        raises("^box", v, grid(), b)
    raises("^normals", v, grid(), box, torch.zeros(N, 2))
    raises("^normals", v, grid(), box, torch.zeros(N + 1, 2, dtype=F64))
    good = (torch.zeros(N, dtype=F64), torch.zeros(N, 2, dtype=F64), torch.zeros(N, dtype=I32), torch.zeros(N, dtype=U8),
            torch.zeros(N, dtype=I32))
    raises("^out:", v, grid(), box, out=good[:4])
    raises(r"^out\[0\]", v, grid(), box, out=(good[0].float(),) + good[1:])
    raises(r"^out\[1\]", v, grid(), box, out=(good[0], torch.zeros(N, dtype=F64)) + good[2:])
    raises(r"^out\[3\]", v, grid(), box, out=good[:3] + (torch.zeros(N, dtype=torch.bool), good[4]))
    raises(r"^out\[4\]", v, grid(), box, out=good[:4] + (torch.zeros(N + 1, dtype=I32),))
    raises("^grid.*HIP", v, grid(), box, torch.zeros(N, 2, dtype=F64), out=good)


def test_integral_program():
    p = ops.integral_program([(0, 1), (2, -1), (-1, -1)], 3)
    assert p.ne == 3 and list(p.a)[:3] == [0, 2, -1] and list(p.b)[:3] == [1, -1, -1]
    assert ops.integral_program(p, 3) is p
    raises("^entries.*column 2", ops.integral_program, p, 2)
    raises("^entries", ops.integral_program, [])
    raises("^entries", ops.integral_program, [(0, 0)] * 9)
    raises("^entries", ops.integral_program, 5)
    for e in ((0,), (0, 1, 2), (0, 1.0), (True, 0), (-2, 0), ("a", 0)):
        raises("^entries.*entry 0", ops.integral_program, [e])
    raises("^entries.*column 4", ops.integral_program, [(0, 0), (4, -1)], 4)
    for nz in (0, -1, 2.0, True):
        raises("^nz", ops.integral_program, [(0, 0)], nz)


def test_weighted_integrals_arguments():
    wi = ops.weighted_integrals
    x, w, ent = torch.zeros(N, 5), torch.zeros(N, dtype=F64), [(0, 1), (2, -1)]
    stats, scratch = torch.zeros(4, 2, dtype=F64), torch.zeros(10, dtype=F64)
    raises("^nz", wi, x, w, ent, stats, scratch, nz=0)
    raises("^entries.*column 2", wi, x, w, ent, stats, scratch, nz=2)
    raises("^stats", wi, x, w, ent, stats.float(), scratch)
    raises("^stats", wi, x, w, ent, torch.zeros(4, 3, dtype=F64), scratch)
    raises("^stats", wi, x, w, ent, torch.zeros(2, 4, dtype=F64).t(), scratch)
    raises("^x:", wi, x.double(), w, ent, stats, scratch)
    raises("^x:", wi, torch.zeros(N), w, ent, stats, scratch, nz=3)
    raises("^x:", wi, torch.zeros(N, 2), w, ent, stats, scratch, nz=3)
    raises("^x:", wi, torch.zeros(5, N).t(), w, ent, stats, scratch)
    raises("^x_step", wi, x, w, ent, stats, scratch, nz=3, x_step=2)
    raises("^x_step", wi, x, w, ent, stats, scratch, nz=3, x_step=3.0)
    raises("^x:.*>= 12", wi, x, w, ent, stats, scratch, x_step=3)          # four steps of three columns
    raises("^sub:", wi, x, w, ent, stats, scratch, sub=torch.zeros(N + 1, 5))
    raises("^sub:", wi, x, w, ent, stats, scratch, sub=torch.zeros(N, 5, dtype=F64))
    raises("^sub:.*>= 20", wi, x, w, ent, stats, scratch, sub=torch.zeros(N, 19), sub_step=5)
    raises("^sub_step", wi, x, w, ent, stats, scratch, sub=torch.zeros(N, 19), sub_step=4)
    raises("^w:", wi, x, w.float(), ent, stats, scratch)
    raises("^w:", wi, x, w[:-1], ent, stats, scratch)
    raises("^scratch", wi, x, w, ent, stats, scratch.float())
    raises("^scratch.*needs 10", wi, x, w, ent, stats, scratch[:9])
    raises("^step", wi, x, w, ent, stats, scratch, step=torch.zeros(2, dtype=torch.long))
    raises("^step", wi, x, w, ent, stats, scratch, step=torch.zeros(0, dtype=I32))
    raises("^t:", wi, x, w, ent, stats, scratch, t=1.0)
    raises("^x.*HIP", wi, x, w, ent, stats, scratch)          # everything else in order: a host tensor


def test_integrate_arguments():
    cv = object.__new__(gfd.ControlVolumes)
    cv.n_nodes, cv.area = N, torch.zeros(N, dtype=F64)
    raises("^entries", cv.integrate, torch.zeros(N, 3), [])
    raises("^x:", cv.integrate, torch.zeros(N + 1, 3), [(0, 0)])
    raises("^x:", cv.integrate, torch.zeros(N), [(0, 0)])
    raises("^t:", cv.integrate, torch.zeros(N, 3), [(0, 0)], t=-1)


def test_rollout_integrals_keywords():
    from graphs4cfd_amd.nn import rollout as R
    g = SimpleNamespace(pos=torch.rand(N, 2), edge_index=torch.zeros(2, 5, dtype=torch.long), num_nodes=N)

    def check(has_target=False, graph=g, **kw):
        return R._check_parts(kw, graph, 3, 6, has_target)["integrals"]

    assert gfd.nn.RolloutIntegrals is R.RolloutIntegrals and R._PARTS.index(R._Integrals) == R._PARTS.index(R._Derived) + 1
    assert check() is None
    spec = check(integrals=("volume", "ke", "mean:2"))
    assert spec["entries"]["prediction"] == [(-1, -1), (0, 0), (1, 1), (2, -1)] and not spec["entries"]["derived"]
    assert check(integrals="ke", integral_options=dict(velocity=(2, 0)))["entries"]["prediction"] == [(2, 2), (0, 0)]
    assert check(True, integrals=("rel_l2",))["entries"]["target"] == [(0, 0), (1, 1), (2, 2)]
    assert check(integrals=("div2", "circulation"), derived=("vort", "div"))["entries"]["derived"] == [(1, 1), (0, -1)]
    raises("^integrals.*without integrals=", check, integral_options=dict(velocity=(0, 1)))
    raises("^integrals.*without integrals=", check, integral_volumes=object())
    for names in ((), 3, ("ke", 1), ("ke", "ke")):
        raises("^integrals", check, integrals=names)
    raises("^integrals.*unknown name 'energy'", check, integrals=("energy",))
    raises("^integrals.*'int:3'", check, integrals=("int:3",))
    raises("^integrals.*'mean:u'", check, integrals=("mean:u",))
    raises("^integrals.*'enstrophy'.*add 'vort' to derived=", check, integrals=("enstrophy",))
    raises("^integrals.*'circulation'.*add 'vort' to derived=", check, integrals=("circulation",), derived=("div",))
    raises("^integrals.*'div2'.*add 'div' to derived=", check, integrals=("div2",), derived=("vort",))
    for name in ("l2:0", "l2", "rel_l2"):
        raises("^integrals.*target=", check, integrals=(name,))
    raises("^integral_options.*unknown", check, integrals=("ke",), integral_options=dict(k=6))
    raises("^integral_options: velocity", check, integrals=("ke",), integral_options=dict(velocity=(0, 3)))
    raises("^integral_options: velocity", check, integrals=("ke",), integral_options=dict(velocity=(0,)))
    raises("^integral_volumes", check, integrals=("ke",), integral_volumes="cells", exc=TypeError)
    cv = object.__new__(gfd.ControlVolumes)
    cv.n_nodes = N + 1
    raises("^integral_volumes.*nodes", check, integrals=("ke",), integral_volumes=cv)
    cv.n_nodes = N
    raises("^integral_options.*integral_volumes", check, integrals=("ke",), integral_volumes=cv, integral_options=dict(box=(0, 0, 1, 1)))
    raises("^integral_volumes.*list", check, graph=[g, g], integrals=("ke",), integral_volumes=cv)
    raises("^box", check, integrals=("ke",), integral_options=dict(box=(0, 0, 0, 1)))
    g3 = SimpleNamespace(pos=torch.rand(N, 3), edge_index=g.edge_index, num_nodes=N)
    raises("^graph.*2-D only", check, graph=g3, integrals=("ke",))
    nine = tuple(f"int:{f}" for f in range(9))
    raises("^integrals.*9 sums over the prediction", lambda: R._Integrals.plan(nine, 9))


def test_rollout_integrals_values():
    from graphs4cfd_amd.nn import rollout as R
    entries, recipes = R._Integrals.plan(("volume", "mean:1", "ke", "enstrophy", "l2:0", "rel_l2"), 2, (0, 1), ["vort"])
    sums = dict(prediction=torch.tensor([[2.0, 3.0, 8.0, 10.0], [2.0, 5.0, 2.0, 4.0]], dtype=F64), derived=torch.tensor([[6.0], [1.0]], dtype=F64),
                error=torch.tensor([[4.0, 12.0], [9.0, 7.0]], dtype=F64), target=torch.tensor([[1.0, 3.0], [2.0, 2.0]], dtype=F64))
    assert entries["prediction"] == [(-1, -1), (1, -1), (0, 0), (1, 1)]
    ig = R.RolloutIntegrals(("volume", "mean:1", "ke", "enstrophy", "l2:0", "rel_l2"), recipes, sums, 2.0, entries)
    assert ig.values.tolist() == [[2.0, 1.5, 9.0, 3.0, 2.0, 2.0], [2.0, 2.5, 3.0, 0.5, 3.0, 2.0]]
    assert ig.drift("ke").tolist() == [0.0, 3.0 / 9.0 - 1.0] and ig.steps == 2 and ig["volume"].tolist() == [2.0, 2.0]
    with pytest.raises(KeyError):
        ig["div2"]
