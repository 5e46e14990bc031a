"""The device neighbour searches (`g4c_knn_grid`, `g4c_knn_grid_query`, csrc/knn_grid.hip) and the three constructions on top of them
against the brute-force float64 reference of oracle/knn_ref.py, through the public entry points with the positions on the device, on
every cloud of tests/knn_cases.py (tests/test_knn_ref.py proves on the host what each cloud claims).

Per case: the returned table is a k-nearest table of the reference distances of the cloud the device searches (`assert_knn`, with the
derived slack); edge_index[1] = arange(n).repeat_interleave(k); edge_attr = pos[col] - pos[row], periodic components wrapped,
recomputed here from the returned indices; the results are device tensors; the raw searches write every entry of a sentinel-filled
buffer.  Where no two candidate distances tie, the host path's table is additionally required bit for bit.  The multi-axis periodic
construction is called itself and must run, or hand over for the reason the case names; `connect_knn` is then checked either way.
Each family has one negative control: a launch's correct table rejected against a perturbed distance matrix."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import knn_cases as K                                    # noqa: E402
from graphs4cfd_amd import synthetic as S                # noqa: E402
from oracle import knn_ref as R                          # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SENTINEL = -7

SELF, QUERY, PER1, PERN = K.by_kind("self"), K.by_kind("query"), K.by_kind("per1"), K.by_kind("perN")


def on_device(t):
    """`t` on the device with its strides kept (a view stays a view)."""
    if t.is_contiguous():
        return t.to(DEV)
    d = torch.empty_strided(t.shape, t.stride(), dtype=t.dtype, device=DEV)
    d.copy_(t)
    assert not d.is_contiguous()
    return d


def check_edges(pos, ei, ea, k, period=None):
    n = pos.size(0)
    assert ei.is_cuda and ea.is_cuda and ei.dtype == torch.long and tuple(ei.shape) == (2, n * k)
    assert torch.equal(ei[1], torch.arange(n, device=DEV).repeat_interleave(k))
    assert ea.dtype == pos.dtype and torch.equal(ea, R.edge_attr_ref(pos, ei, period))
    for ax, d in enumerate(period or ()):
        if d is not None:
            extent = float(pos[:, ax].double().max() - pos[:, ax].double().min())
            d = extent if d == "auto" else float(d)
            if extent <= d:                              # (one wrap, as in the reference: enough when the cloud fits its period)
                assert float(ea[:, ax].abs().max()) <= d / 2 * (1 + 1e-6)
    return ei[0].reshape(n, k)


def control(D, table, k, slack):
    assert R.rejects(R.assert_knn, R.worsen_first_neighbour(D, table), table, k, **slack)


# ------------------------------------------------------------------ self search
@pytest.mark.parametrize("case", SELF, ids=K.ids(SELF))
def test_self_search(case):
    pos, k = on_device(case.pos), case.k
    n = pos.size(0)
    D = R.distances(case.cloud32.to(DEV))
    raw = torch.full((n, k), SENTINEL, dtype=torch.long, device=DEV)
    assert S.knn_neighbours_device(pos, k, out=raw) is raw
    assert not bool((raw == SENTINEL).any())
    R.assert_knn(D, raw, k, **R.NONPERIODIC)
    ei, ea = S.connect_knn(pos, k)
    table = check_edges(pos, ei, ea, k)
    assert torch.equal(table, raw)
    if not case.ties:
        assert torch.equal(ei.cpu(), S.connect_knn(case.cloud32, k)[0])          # (the host path on the cloud the device searches)
    if case.name == "self_k9_3d":
        control(D, raw, k, R.NONPERIODIC)


# ------------------------------------------------------------------ query search
@pytest.mark.parametrize("case", QUERY, ids=K.ids(QUERY))
def test_query_search(case):
    pts, q, k = case.pos.to(DEV), case.queries.to(DEV), case.k
    m = q.size(0)
    D = R.distances(pts, q)
    raw = torch.full((m, k), SENTINEL, dtype=torch.long, device=DEV)
    assert S.knn_query_device(pts, q, k, out=raw) is raw
    assert not bool((raw == SENTINEL).any())
    R.assert_knn(D, raw, k, **R.NONPERIODIC)
    y_idx, x_idx, w = S.knn_interp_weights(pts, q, k)
    assert x_idx.is_cuda and y_idx.is_cuda and w.is_cuda
    assert torch.equal(x_idx.reshape(m, k), raw)
    assert torch.equal(y_idx, torch.arange(m, device=DEV).repeat_interleave(k))
    diff = pts[x_idx] - q[y_idx]
    assert torch.equal(w, 1.0 / torch.clamp((diff * diff).sum(-1, keepdim=True), min=1e-16))
    if not case.ties:
        assert torch.equal(x_idx.cpu(), S.knn_interp_weights(case.pos, case.queries, k)[1])
    if case.name == "query_mixed_k9_3d":
        control(D, raw, k, R.NONPERIODIC)


# ------------------------------------------------------------------ one periodic axis of a 2-D cloud
@pytest.mark.parametrize("case", PER1, ids=K.ids(PER1))
def test_one_periodic_axis(case):
    pos, k = case.pos.to(DEV), case.k
    D = R.distances(pos, None, case.period)
    ei, ea = S.connect_knn(pos, k, period=case.period)
    table = check_edges(pos, ei, ea, k, case.period)
    R.assert_knn(D, table, k, **R.PERIODIC)
    if not case.ties:
        assert torch.equal(ei.cpu(), S.connect_knn(case.pos.clone(), k, period=case.period)[0])
    if case.name == "per1_random_auto":
        control(D, table, k, R.PERIODIC)


# ------------------------------------------------------------------ two or more periodic axes
@pytest.mark.parametrize("case", PERN, ids=K.ids(PERN))
def test_any_periodic_axes(case):
    pos, k = case.pos.to(DEV), case.k
    D = R.distances(pos, None, case.period)
    why = []
    hit = S._connect_knn_periodic_device(pos, k, list(case.period), why)
    if case.fallback is None:
        assert hit is not None, why
        assert why == (["margin grown"] if case.grown else [])
        R.assert_knn(D, check_edges(pos, hit[0], hit[1], k, case.period), k, **R.PERIODIC)
    else:
        assert hit is None and why[-1] == case.fallback, why
    ei, ea = S.connect_knn(pos, k, period=case.period)
    table = check_edges(pos, ei, ea, k, case.period)
    R.assert_knn(D, table, k, **R.PERIODIC)
    if hit is not None:
        assert torch.equal(ei, hit[0]) and torch.equal(ea, hit[1])
    if not case.ties:
        assert torch.equal(ei.cpu(), S.connect_knn(case.pos.clone(), k, period=case.period)[0])
    if case.name == "perN_random_3d_two_axes":
        control(D, table, k, R.PERIODIC)


# ------------------------------------------------------------------ argument errors (device)
def test_argument_errors_on_the_device():
    g = torch.Generator().manual_seed(0)
    p2, p3 = torch.rand(50, 2, generator=g).to(DEV), torch.rand(50, 3, generator=g).to(DEV)
    with pytest.raises(ValueError, match="knn_query_device.*g4c_knn_grid_query"):
        S.knn_query_device(p2, p3[:7], 3)                                         # (used to search 2-D over a 3-wide array)
    with pytest.raises(ValueError, match="knn_query_device.*g4c_knn_grid_query"):
        S.knn_query_device(p3, p2[:7], 3)
    with pytest.raises(ValueError, match="knn_interp_weights"):
        S.knn_interp_weights(p2, p3, 3)
    with pytest.raises(ValueError, match="knn_interp_weights: k=4"):
        S.knn_interp_weights(p2[:3], p2, 4)
    for dim in (1, 4):
        with pytest.raises(ValueError, match="g4c_knn_grid"):
            S.knn_neighbours_device(torch.rand(20, dim, device=DEV), 3)
        with pytest.raises(ValueError, match="connect_knn"):
            S.connect_knn(torch.rand(20, dim, device=DEV), 3)
    for period in (None, (1.0, None), ("auto", "auto")):
        for n in (5, 6):
            with pytest.raises(ValueError, match="connect_knn: n="):
                S.connect_knn(p2[:n], 6, period=period)
    for bad in (float("nan"), float("inf")):
        broken = p2.clone()
        broken[4, 1] = bad
        with pytest.raises(ValueError, match="g4c_knn_grid.*non-finite"):
            S.knn_neighbours_device(broken, 3)
        with pytest.raises(ValueError, match="g4c_knn_grid_query.*non-finite"):
            S.knn_query_device(broken, p2, 3)
        for period in (None, ("auto", None), (None, 2.0), ("auto", "auto")):
            with pytest.raises(ValueError, match="non-finite"):
                S.connect_knn(broken, 3, period=period)
    with pytest.raises(ValueError, match="out must be"):
        S.knn_neighbours_device(p2, 3, out=torch.empty((50, 3), dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="out must be"):
        S.knn_query_device(p2, p2[:4], 3, out=torch.empty((5, 3), dtype=torch.long, device=DEV))
