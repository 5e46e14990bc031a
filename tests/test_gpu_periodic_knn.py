"""g4c_knn_grid_periodic and g4c_knn_grid_query_periodic (csrc/knn_periodic.hip) through `synthetic.knn_neighbours_device(period=)`
and `knn_query_device(period=)` against the brute-force wrapped distance matrix of tests/periodic_ref.py, on the cases of
tests/periodic_cases.py (tests/test_periodic_ref.py proves what each case exercises).  The clouds are dyadic and tie-free, so the
tables equal the brute-force tables exactly, order included."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

import periodic_ref as P                       # noqa: E402
from periodic_cases import CASES, IDS          # noqa: E402
from oracle import knn_ref as K                # noqa: E402
from graphs4cfd_amd import synthetic as S      # noqa: E402

DEV = torch.device("cuda", 0)
SLACK = K.NONPERIODIC
SENT = -12345


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_self_and_query_tables_are_the_brute_force_tables(case):
    pos, k, per, q = case["pos"], case["k"], case["period"], case["queries"]
    D_self, D_q = P.distances(pos, per), P.distances(pos, per, q)
    out_s = torch.full((pos.shape[0], k), SENT, dtype=torch.long, device=DEV)
    out_q = torch.full((q.shape[0], k), SENT, dtype=torch.long, device=DEV)
    got_s = S.knn_neighbours_device(dev(pos), k, out=out_s, period=per)
    got_q = S.knn_query_device(dev(pos), dev(q), k, out=out_q, period=per)
    assert got_s is out_s and got_q is out_q
    got_s, got_q = got_s.cpu(), got_q.cpu()
    assert not bool((got_s == SENT).any()) and not bool((got_q == SENT).any())          # every entry of `out` is written
    K.assert_knn(D_self, got_s, k, **SLACK)
    K.assert_knn(D_q, got_q, k, **SLACK, self_mode=False)
    assert torch.equal(got_s, P.brute_force_table(D_self, k)) and torch.equal(got_q, P.brute_force_table(D_q, k))
    if case["far"]:          # a query and the same query ± 3 L: the same row (the periods are powers of two)
        n = case["far"]
        assert torch.equal(got_q[-n:], got_q[:n])


def test_an_explicit_period_equal_to_auto_gives_autos_table():
    pos = CASES[3]["pos"]
    o, L = P.frame(pos, (None, "auto"))
    a = S.knn_neighbours_device(dev(pos), 12, period=(None, "auto"))
    b = S.knn_neighbours_device(dev(pos), 12, period=(None, float(L[1])))
    assert torch.equal(a, b)


@pytest.mark.parametrize("dim", [2, 3])
def test_without_a_periodic_axis_the_call_is_todays(dim):
    pos = dev(CASES[1 if dim == 2 else 7]["pos"])
    q = dev(CASES[1 if dim == 2 else 7]["queries"])
    for k in (6, 12):
        plain_s, plain_q = S.knn_neighbours_device(pos, k), S.knn_query_device(pos, q, k)
        for per in (None, (None,) * dim, [None] * dim):
            assert torch.equal(S.knn_neighbours_device(pos, k, period=per), plain_s)
            assert torch.equal(S.knn_query_device(pos, q, k, period=per), plain_q)


def test_the_limits_are_the_existing_ones():
    pos = dev(CASES[4]["pos"])
    with pytest.raises(ValueError):
        S.knn_neighbours_device(pos, 17, period=(1.0, None))
    with pytest.raises(ValueError):
        S.knn_neighbours_device(pos[:6], 6, period=(1.0, None))          # self: n > k
    assert tuple(S.knn_query_device(pos[:6], pos, 6, period=(1.0, None)).shape) == (40, 6)          # query: n >= k
    with pytest.raises(ValueError, match="period"):
        S.knn_neighbours_device(pos, 6, period=(0.5, None))              # shorter than the extent


def test_a_query_that_does_not_wrap_is_searched_from_the_origin():
    """Finite but so large that (q − o) / L overflows (L = 0.5: |q| above 1.7e38), infinite, or NaN along a PERIODIC axis: the wrap
    answers the origin (include/g4c.h), so the row is the origin's row — k node indices, never −1."""
    case = CASES[1]
    pos, k, per = case["pos"], case["k"], case["period"]
    o, L = P.frame(pos, per)
    wild = np.array([[0.3, 2e38], [0.3, -3e38], [0.3, np.inf], [0.3, np.nan], [np.inf, 0.1], [-np.inf, np.nan], [0.3, float(o[1])],
                     [float(o[0]), 0.1], [float(o[0]), float(o[1])]], np.float32)
    assert not P.wraps_finite(wild[:6], o, L).any()
    got = S.knn_query_device(dev(pos), dev(wild), k, period=per).cpu()
    assert int(got.min()) >= 0 and int(got.max()) < pos.shape[0]
    assert torch.equal(got[:4], got[6:7].expand(4, k)) and torch.equal(got[4], got[7]) and torch.equal(got[5], got[8])
    K.assert_knn(P.distances(pos, per, wild), got, k, **SLACK, self_mode=False)          # (tie-aware: these queries were not chosen tie-free)
