"""The `period=` arguments of the off-node operators, checked before anything touches a device: every refusal is a ValueError that
names the argument.  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import graphs4cfd_amd as gfd                                   # noqa: E402
from graphs4cfd_amd import _lib, synthetic as S                # noqa: E402
from graphs4cfd_amd.mesh_jet import check_stencil              # noqa: E402
from graphs4cfd_amd.nn.losses import ResidualLoss, SampleLoss  # noqa: E402
from graphs4cfd_amd.tracers import check_tracers               # noqa: E402


def graph(n=40, dim=2):
    return gfd.Graph(pos=torch.rand(n, dim, generator=torch.Generator().manual_seed(0)))


@pytest.mark.parametrize("bad", [(1.0,), (1.0, None, None), 1.0, "auto"])
def test_a_period_of_the_wrong_length(bad):
    g, pts = graph(), torch.zeros(3, 2)
    with pytest.raises(ValueError, match="^period"):
        S.check_period(bad, 2)
    with pytest.raises(ValueError, match="^period"):
        gfd.PointSampler(g, pts, period=bad)
    with pytest.raises(ValueError, match="^period"):
        check_stencil(g, 12, 2, None, bad)
    with pytest.raises(ValueError, match="^period"):
        check_tracers(g, pts, 0.1, period=bad)
    with pytest.raises(ValueError, match="^period"):
        SampleLoss(pts, period=bad)


@pytest.mark.parametrize("bad", [(0.0, None), (-1.0, None), (None, float("nan")), (float("inf"), None), (True, None), ("Auto", None)])
def test_a_length_that_is_not_positive(bad):
    g, pts = graph(), torch.zeros(3, 2)
    for call in (lambda: S.check_period(bad, 2), lambda: gfd.PointSampler(g, pts, period=bad), lambda: check_stencil(g, 12, 2, None, bad),
                 lambda: check_tracers(g, pts, 0.1, period=bad), lambda: SampleLoss(pts, period=bad)):
        with pytest.raises(ValueError, match="^period"):
            call()


def test_a_length_shorter_than_the_extent():
    lo, hi = torch.tensor([0.0, 0.0]), torch.tensor([1.0, 0.5])
    with pytest.raises(ValueError, match="^period.*shorter"):
        S.period_lengths([0.75, None], lo, hi)
    with pytest.raises(ValueError, match="^period"):
        S.period_lengths([None, "auto"], lo, torch.tensor([1.0, 0.0]))          # "auto" along an axis without extent
    assert S.period_lengths([1.0, "auto"], lo, hi) == [1.0, 0.5] and S.period_lengths([None, 2], lo, hi) == [0.0, 2.0]
    # "auto" is the fp32 extent rounded UP: never shorter than the cloud
    lo, hi = torch.tensor([0.1, 0.0]), torch.tensor([0.7, 1.0])
    L = S.period_lengths(["auto", None], lo, hi)[0]
    assert L >= float(hi[0]) - float(lo[0]) and np.float32(L) == L


def test_all_none_is_no_period():
    assert S.check_period(None, 2) is None and S.check_period((None, None), 2) is None and S.check_period([None] * 3, 3) is None
    assert S.check_period((None, "auto", 2), 3) == [None, "auto", 2.0]


def test_period_with_edge_vectors_or_without_k_or_above_16():
    g = graph()
    with pytest.raises(ValueError, match="^period"):
        check_stencil(g, 12, 2, torch.zeros(5, 2), (1.0, None))          # with edge_vectors
    with pytest.raises(ValueError, match="^period"):
        check_stencil(g, None, 2, None, (1.0, None))                     # with k=None
    with pytest.raises(ValueError, match="^k"):
        check_stencil(g, 17, 2, None, (1.0, None))                       # k > 16
    assert check_stencil(g, 17, 2, None, None) == 2 and check_stencil(g, 16, 2, None, (1.0, None)) == 2
    with pytest.raises(ValueError, match="^period"):
        gfd.MeshJet(g, k=None, period=(1.0, None))
    with pytest.raises(ValueError, match="^period"):
        ResidualLoss(nu=0.01, dt=0.1, k=None, period=(1.0, None))
    with pytest.raises(ValueError, match="^period"):
        ResidualLoss(nu=0.01, dt=0.1, k=None, edge_vectors="rel", period=(1.0, None))
    with pytest.raises(ValueError, match="^k"):
        ResidualLoss(nu=0.01, dt=0.1, k=17, period=(1.0, None))
    assert ResidualLoss(nu=0.01, dt=0.1, period=(1.0, None)).period == [1.0, None] and ResidualLoss(nu=0.01, dt=0.1).period is None
    with pytest.raises(ValueError, match="^k"):
        gfd.PointSampler(g, torch.zeros(3, 2), k=17, period=(1.0, None))
    with pytest.raises(ValueError, match="k"):
        check_tracers(g, torch.zeros(3, 2), 0.1, k=17, period=(1.0, None))


def test_the_new_entry_points_are_declared():
    for name in ("g4c_knn_grid_periodic", "g4c_knn_grid_query_periodic", "g4c_sample_weights_periodic", "g4c_tracer_advance_periodic"):
        assert name in _lib.EXPORTED_SYMBOLS
    import ctypes as C
    assert C.sizeof(_lib.g4c_tracer_periodic_t) == C.sizeof(_lib.g4c_tracer_t) + 40          # three floats, padding, three doubles
    assert _lib.g4c_tracer_periodic_t.base.offset == 0          # g4c_tracer_t keeps its layout, in front


def test_a_period_far_above_the_extent_is_refused_before_anything_is_allocated():
    lo, hi = torch.tensor([0.0, 0.0]), torch.tensor([1.0, 0.5])
    cells, counts = S._periodic_grid_shape(lo, hi, 2000, 12, [1.0, 0.5], "t")
    assert counts[:2] == [22, 11] and counts[0] * counts[1] <= S.MAX_PERIODIC_CELLS
    with pytest.raises(ValueError, match="^period.*cells"):
        S._periodic_grid_shape(lo, hi, 2000, 12, [1e6, 1e3], "t")
    with pytest.raises(ValueError, match="^period.*cells"):
        S._periodic_grid_shape(torch.zeros(3), torch.ones(3), 300, 12, [1e4, 1e4, 0.0], "t")
