"""Every ValueError / TypeError of gfd.Modes, Modes.fit / from_gram, the host algebra, ops.snapshot_mean / _gram / _combine, GNN.modes and
GNN.evaluate(modes=) is raised in Python, on the arguments as they were passed, before the library is touched: `_lib.load` and
`_lib.require_hip` are replaced by functions that fail the test."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import graphs4cfd_amd as gfd                               # noqa: E402
from graphs4cfd_amd import _lib, ops                       # noqa: E402
from graphs4cfd_amd import modes as Mo                     # noqa: E402

F32, F64 = torch.float32, torch.float64


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


def test_exports():
    import graphs4cfd
    assert graphs4cfd.Modes is gfd.Modes is gfd.nn.Modes is Mo.Modes
    assert graphs4cfd.SnapshotModes is gfd.SnapshotModes is gfd.nn.SnapshotModes and graphs4cfd.DynamicModes is gfd.DynamicModes
    assert graphs4cfd.modes is Mo
    assert (_lib.SNAPSHOT_MAX_ROWS, _lib.SNAPSHOT_GRAM_BLOCK, _lib.SNAPSHOT_GRAM_CHUNK, _lib.SNAPSHOT_COMBINE_BLOCK) == (1024, 64, 2048, 8)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "g4c.h")).read()
    for name, value in (("MAX_ROWS", 1024), ("GRAM_BLOCK", 64), ("GRAM_CHUNK", 2048), ("COMBINE_BLOCK", 8), ("MAX_COLUMNS", "2147483647LL")):
        assert f"#define G4C_SNAPSHOT_{name} {value}" in header


def test_modes_arguments():
    M = gfd.Modes
    for bad in (0, -1, 1.5, True, "3", _lib.SNAPSHOT_MAX_ROWS + 1):
        raises("^rank:", M, rank=bad)
    for bad in (0, 0.0, -0.1, 1.1, "0.9", True, float("nan")):
        raises("^energy:", M, energy=bad)
    raises("^centre:", M, centre=1, kind=TypeError)
    raises("^dmd:", M, dmd="yes", kind=TypeError)
    for bad in (-1, 1.0, True, None):
        raises("^start:", M, start=bad)
    for bad in (0, -2, 2.0, False):
        raises("^stride:", M, stride=bad)
    for bad in (0, -1, 2.5, True, _lib.SNAPSHOT_MAX_ROWS + 1):
        raises("^count:", M, count=bad)
    for bad in (0, -1.0, float("inf"), "1", None, True):
        raises("^dt:", M, dt=bad)
    for name in ("node_weights", "field_weights"):
        raises(f"^{name}:", M, **{name: "abc"}, kind=TypeError)
        raises(f"^{name}:", M, **{name: torch.tensor([True, False])}, kind=TypeError)
        raises(f"^{name}:", M, **{name: torch.ones(2, 2)})
        raises(f"^{name}:", M, **{name: torch.ones(0)})
        raises(f"^{name}:", M, **{name: [1.0, -1.0]})
        raises(f"^{name}:", M, **{name: [1.0, float("nan")]})
        raises(f"^{name}:.*every weight is 0", M, **{name: [0.0, 0.0]})
    spec = M(rank=2, energy=1, node_weights=[1, 2, 3], field_weights=torch.tensor([1.0, 0.0]), start=1, stride=2, count=3, dt=0.5, dmd=True)
    assert spec.node_weights.dtype == F64 and spec.field_weights.tolist() == [1.0, 0.0] and spec.energy == 1.0
    assert spec.selection(6) == (1, 2, 3) and M(start=1, stride=2).selection(6) == (1, 2, 3) and M().selection(5) == (0, 1, 5)
    raises("^start:", spec.selection, 1)
    raises("^count:", spec.selection, 5)
    raises("^count:.*DMD", M(dmd=True).selection, 1)
    raises("^count:", M().selection, _lib.SNAPSHOT_MAX_ROWS + 1, kind=NotImplementedError)
    w = spec.weights(3, 2, "cpu")
    assert w.dtype == F64 and w.tolist() == [1.0, 0.0, 2.0, 0.0, 3.0, 0.0]
    assert spec.weights(3, 2, "cpu", perm=torch.tensor([2, 0, 1])).tolist() == [3.0, 0.0, 1.0, 0.0, 2.0, 0.0]
    assert M().weights(3, 2, "cpu") is None
    raises("^node_weights:", spec.weights, 4, 2, "cpu")
    raises("^field_weights:", spec.weights, 3, 3, "cpu")


def test_fit_arguments():
    spec = gfd.Modes()
    x = torch.zeros(4, 5, 3)
    raises("^layout:", spec.fit, x, layout="rows")
    raises("^snapshots:", spec.fit, x.double(), kind=TypeError)
    raises("^snapshots:", spec.fit, [[1.0]], kind=TypeError)
    raises("^snapshots:", spec.fit, torch.zeros(4, 15))
    raises("^snapshots:", spec.fit, torch.zeros(4, 0, 3))
    raises("^snapshots:", spec.fit, x.permute(1, 0, 2))
    raises("^nf:", spec.fit, x, nf=2)
    raises("^nf:", spec.fit, torch.zeros(5, 12), layout="columns")
    raises("^nf:", spec.fit, torch.zeros(5, 12), layout="columns", nf=0)
    raises("^snapshots:", spec.fit, torch.zeros(5, 13), layout="columns", nf=3)
    raises("^snapshots:", spec.fit, x, layout="columns", nf=3)
    raises("^snapshots:", gfd.Modes(field_weights=[1.0, 1.0, 1.0, 1.0, 1.0]).fit, torch.zeros(5, 12), layout="columns")
    raises("^gram:", spec.from_gram, torch.zeros(3, 3), kind=TypeError)
    raises("^gram:", spec.from_gram, "G", kind=TypeError)
    raises("^gram:", spec.from_gram, torch.zeros(3, 2, dtype=F64))
    raises("^gram:", spec.from_gram, torch.full((2, 2), float("nan"), dtype=F64))
    raises("^dmd_gram:", gfd.Modes(dmd=True).from_gram, torch.eye(3, dtype=F64))
    raises("^gram:.*DMD", Mo.dmd_from_gram, torch.eye(1, dtype=F64))
    pod = Mo.pod_from_gram(torch.eye(3, dtype=F64))
    raises("^cross:", Mo.principal_cosines, pod, torch.zeros(3, 2, dtype=F64), pod)
    raises("^cross:", Mo.principal_cosines, pod, torch.zeros(3, 3), pod)
    got = spec.from_gram(torch.diag(torch.tensor([4.0, 1.0, 0.25], dtype=F64)))
    assert got.modes is None and got.mean is None and got.dmd is None and got.singular_values.tolist() == [2.0, 1.0, 0.5]
    for name, args in (("project", (x,)), ("reconstruct", ()), ("alignment", (got,))):
        raises(f"^{name}:.*no snapshots", getattr(got, name), *args, kind=RuntimeError)
    raises("^other:", got.alignment, x, kind=TypeError)


def test_launch_arguments():
    x, m, w = torch.zeros(6, 10), torch.zeros(10, dtype=F64), torch.ones(10, dtype=F64)
    for f in (ops.snapshot_mean, lambda t, **k: ops.snapshot_gram(t, **k), lambda t, **k: ops.snapshot_combine(t, torch.zeros(6, 2, dtype=F64), **k)):
        raises("^(x|a):", f, x.double(), kind=TypeError)
        raises("^(x|a):", f, torch.zeros(10))
        raises("^(x|a):", f, torch.zeros(0, 10))
        raises("^(x|a):", f, torch.zeros(6, 0))
        raises("^(x|a):", f, torch.zeros(10, 6).t())
    for name, f in (("sel", lambda s: ops.snapshot_mean(x, s)), ("sel_a", lambda s: ops.snapshot_gram(x, sel_a=s)),
                    ("sel_b", lambda s: ops.snapshot_gram(x, x, sel_b=s)), ("sel", lambda s: ops.snapshot_combine(x, torch.zeros(6, 2, dtype=F64), sel=s))):
        for bad in ((0, 1), (0, 1, 2.0), "012", (0, True, 2)):
            raises(f"^{name}:", f, bad, kind=TypeError)
        for bad in ((-1, 1, 2), (0, 0, 2), (0, 1, 0), (0, 1, 7), (2, 3, 3), (6, 1, 1)):
            raises(f"^{name}:", f, bad)
    raises("^out:", ops.snapshot_mean, x, out=torch.zeros(10), kind=TypeError)
    raises("^out:", ops.snapshot_mean, x, out=torch.zeros(9, dtype=F64))
    g = ops.snapshot_gram
    raises("^mean_b:", g, x, mean_b=m)
    raises("^mean_b:", g, x, sel_b=(0, 1, 2))
    raises("^b:", g, x, torch.zeros(6, 11))
    raises("^b:", g, x, torch.zeros(6, 10).double(), kind=TypeError)
    for name in ("mean_a", "w"):
        raises(f"^{name}:", g, x, **{name: m.float()}, kind=TypeError)
        raises(f"^{name}:", g, x, **{name: torch.zeros(11, dtype=F64)})
        raises(f"^{name}:", g, x, **{name: torch.zeros(20, dtype=F64)[::2]})
    raises("^mean_b:", g, x, x, mean_b=torch.zeros(9, dtype=F64))
    raises("^out:", g, x, out=torch.zeros(6, 6), kind=TypeError)
    raises("^out:", g, x, out=torch.zeros(6, 5, dtype=F64))
    raises("^out:", g, x, out=torch.zeros(6, 6, dtype=F64).t())
    raises("^scratch:", g, x, scratch=torch.zeros(4095, dtype=F64))
    raises("^scratch:", g, x, scratch=torch.zeros(2 * 4096, dtype=F64)[::2])
    raises("^scratch:", g, x, x, sel_a=(0, 1, 2), sel_b=(1, 1, 2), scratch="s")
    big = torch.zeros(_lib.SNAPSHOT_MAX_ROWS + 1, 1)
    raises("^sel_a:", g, big, kind=NotImplementedError)
    raises("^sel_b:", g, x, big[:, :1].expand(-1, 1).contiguous().repeat(1, 10), kind=NotImplementedError)
    c = ops.snapshot_combine
    coef = torch.zeros(6, 2, dtype=F64)
    raises("^coef:", c, x, coef.float(), kind=TypeError)
    raises("^coef:", c, x, torch.zeros(5, 2, dtype=F64))
    raises("^coef:", c, x, torch.zeros(6, dtype=F64))
    raises("^coef:", c, x, torch.zeros(6, 0, dtype=F64))
    raises("^coef:", c, x, torch.zeros(2, 6, dtype=F64).t())
    raises("^coef:", c, x, torch.zeros(6, _lib.SNAPSHOT_MAX_ROWS + 1, dtype=F64), kind=NotImplementedError)
    raises("^mean:", c, x, coef, mean=m.float(), kind=TypeError)
    raises("^mean:", c, x, coef, mean=torch.zeros(3, dtype=F64))
    raises("^out:", c, x, coef, out=torch.zeros(2, 10, dtype=F64), kind=TypeError)
    raises("^out:", c, x, coef, out=torch.zeros(10, 2))
    raises("^out:", c, x, coef, out=torch.zeros(2, 20)[:, ::2])


def test_model_arguments():
    model = gfd.nn.NsOneScaleGNN(arch=gfd.synthetic.mus_arch("NsOneScaleGNN", 16), device=torch.device("cpu"))
    g = gfd.Graph(pos=torch.rand(8, 2))
    g.field, g.target = torch.zeros(8, 3), torch.zeros(8, 12)
    raises("^modes:", model.modes, g, 4, "pod", kind=TypeError)
    raises("^modes:.*own options", model.modes, g, 4, gfd.Modes(), rank=2)
    raises("^rank:", model.modes, g, 4, rank=0)
    for bad in (0, -1, 1.0, True):
        raises("^every:", model.modes, g, 4, every=bad)
    raises("^start:", model.modes, g, 4, every=2, start=2)
    raises("^count:", model.modes, g, 4, count=5)
    raises("^count:.*DMD", model.modes, g, 4, every=4, dmd=True)
    raises("^modes:", model.evaluate, g, 4, modes=dict(rank=2), kind=TypeError)
    raises("^modes:.*every", model.evaluate, g, 4, modes=gfd.Modes())
