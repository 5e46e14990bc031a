"""Every ValueError of gfd.nn.SampleLoss, gfd.PointSampler.from_tables and ops.sample_points_adjoint is raised in Python, on the
arguments as they were passed, before the library is touched: `_lib.load` is replaced by a function that fails the test."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import graphs4cfd_amd as gfd                               # noqa: E402
from graphs4cfd_amd import _lib, ops                       # noqa: E402

F32, F64, I32 = torch.float32, torch.float64, torch.int32
N, P, K = 6, 4, 2


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


def test_sample_points_adjoint_arguments():
    gy, off, pt, cf = torch.zeros(P, 3), torch.zeros(N + 1, dtype=I32), torch.zeros(K * P, dtype=I32), torch.zeros(K * P)
    a = ops.sample_points_adjoint
    for n in (-1, 2.0, True, None):
        raises("^n_nodes:", a, gy, off, pt, cf, n)
    raises("^gy:", a, gy.double(), off, pt, cf, N)
    raises("^gy:", a, torch.zeros(P), off, pt, cf, N)
    raises("^gy:", a, torch.zeros(P, 0), off, pt, cf, N)
    raises("^gy:", a, torch.zeros(P, 1).expand(P, 3), off, pt, cf, N)          # a stride-0 view: made dense by the caller
    raises("^gy:", a, torch.zeros(P, 6)[:, ::2], off, pt, cf, N)
    raises("^in_off:", a, gy, off[:-1], pt, cf, N)
    raises("^in_off:", a, gy, off.long(), pt, cf, N)
    raises("^in_pt:", a, gy, off, pt.long(), cf, N)
    raises("^in_pt:", a, gy, off, pt[:-1], cf[:-1], N)                         # not k entries per point
    raises("^in_pt:", a, gy, off, pt[:0], cf[:0], N)                           # points without entries
    raises("^in_pt:", a, gy[:0], off, pt, cf, N)                               # entries without points
    raises("^in_pt:", a, gy, off, pt.view(K, P), cf, N)
    raises("^in_coef:", a, gy, off, pt, cf[:-1], N)
    raises("^in_coef:", a, gy, off, pt, cf.double(), N)
    raises("^out:", a, gy, off, pt, cf, N, torch.zeros(N, 2))
    raises("^out:", a, gy, off, pt, cf, N, torch.zeros(N, 3).double())
    raises("^out:", a, gy, off, pt, cf, N, torch.zeros(N, 6)[:, ::2])
    both = torch.zeros(N + P, 3)
    raises("^out:.*shares its storage", a, both[:P], off, pt, cf, N, both[P:])
    raises("^gy:.*HIP device only", a, gy, off, pt, cf, N)                     # everything else is in order: there is no CPU path


def test_from_tables_arguments():
    idx, coef = torch.zeros(K, P, dtype=I32), torch.zeros(K, P)
    f = gfd.PointSampler.from_tables
    for n in (-1, 2.0, True, None):
        raises("^n_nodes:", f, idx, coef, n)
    raises("^idx:", f, idx.long(), coef, N)
    raises("^idx:", f, idx[0], coef, N)
    raises("^idx:", f, torch.zeros(17, P, dtype=I32), torch.zeros(17, P), N)
    raises("^idx:", f, torch.zeros(P, K, dtype=I32).t(), coef, N)              # the tables are j-major and contiguous
    raises("^coef:", f, idx, coef.double(), N)
    raises("^coef:", f, idx, coef[:, :-1], N)
    raises("^idx:.*HIP device only", f, idx, coef, N)


def test_too_many_table_entries_are_refused_from_the_shapes_alone():
    s = gfd.PointSampler.__new__(gfd.PointSampler)          # k · P = 2^31 entries: no storage, the shapes alone (a meta tensor)
    s.k, s.n_nodes, s._adjoint_tables = 16, 100, None
    s._idx = s._coef = torch.empty((16, 2 ** 27), dtype=I32, device="meta")
    with pytest.raises(NotImplementedError, match="2147483648|16 · 134217728"):
        s._node_side()
    with pytest.raises(NotImplementedError, match="int32 offsets"):
        s.adjoint(torch.empty((2 ** 27, 1), device="meta"))


def test_sample_loss_constructor_arguments():
    pts = torch.zeros(P, 2)
    L = gfd.nn.SampleLoss
    for bad in (None, [[0.0, 0.0]], torch.zeros(P, 2, dtype=torch.int64), torch.zeros(P), torch.zeros(P, 4), torch.zeros(P, 1),
                torch.tensor([[0.0, float("nan")]]), torch.tensor([[float("inf"), 0.0]])):
        raises("^points:", L, bad)
    for name in ("lambda_d", "weight", "node_weight"):
        for bad in (-1, -0.5, float("nan"), float("inf"), "1", None, True, torch.tensor(1.0)):
            raises(f"^{name}:", L, pts, **{name: bad})
    for bad in ("", 3, "obs_index", ["obs"]):
        raises("^values:", L, pts, values=bad)
    for bad in (3, (), (0, 0), (-1,), (0.0,), (True,), ("u",)):
        raises("^fields:", L, pts, fields=bad)
    for bad in (0, 17, -1, 6.0, True, "6"):
        raises("^k:", L, pts, k=bad)
    for bad in (3, -1, 1.0, True, None, "2"):
        raises("^power:", L, pts, power=bad)
    for bad in (-1.0, float("nan"), float("inf"), "0.1", True):
        raises("^max_distance:", L, pts, max_distance=bad)
    ok = L(pts, lambda_d=0.25, weight=0, node_weight=2, values="obs", fields=(0, 1), k=6, power=1, max_distance=0.1)
    assert ok.takes_step is True and ok.builds == 0 and ok.fields == (0, 1)
    assert L(pts.double(), fields=[2]).fields == (2,) and L(torch.zeros(0, 3)).points.shape == (0, 3)


def test_sample_loss_call_arguments():
    pts = torch.zeros(P, 2)
    pred = torch.zeros(N, 3)
    graph = gfd.Graph(pos=torch.zeros(N, 2), omega=torch.zeros(N, 1))
    raises("^step:", gfd.nn.SampleLoss(pts, values="obs"), graph, pred, pred)          # observations are per output step
    raises("^graph:", gfd.nn.SampleLoss(pts), gfd.Graph(x=pred), pred, pred)
    # weight = 0: GraphLoss alone — nothing is built, on the host as well, with or without a step
    crit = gfd.nn.SampleLoss(pts, weight=0, values="obs")
    base = gfd.nn.GraphLoss(0)
    a, b = torch.randn(N, 3, generator=torch.Generator().manual_seed(0)), torch.randn(N, 3, generator=torch.Generator().manual_seed(1))
    assert torch.equal(crit(graph, a, b), base(graph, a, b)) and torch.equal(crit(graph, a, b, step=1), base(graph, a, b)) and crit.builds == 0
