"""The neighbour searches against a brute-force float64 reference, host side (oracle/knn_ref.py, tests/knn_cases.py; the device side is
tests/test_gpu_knn_ref.py):
  * every case's claims hold — tier separation (the slack decides nothing), ties, duplicates, the ring count of the kernel's stop
    rule, the fallback a multi-axis periodic cloud takes (the construction's host-side logic run with a brute-force search in place
    of the launch);
  * the host paths (`knn_neighbours`, `connect_knn` on CPU tensors, `knn_interp_weights`) return k-nearest tables on every case;
  * `assert_knn` needs each of its four conditions: a perturbed table is rejected, and by exactly the condition it was built to break;
  * the argument errors."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import knn_cases as K                                    # noqa: E402
from graphs4cfd_amd import synthetic as S                # noqa: E402
from oracle import knn_ref as R                          # noqa: E402

ALL = K.all_cases()
_D = {}


def slack_of(case):
    return R.PERIODIC if case.periodic else R.NONPERIODIC


def reference(case):
    """The case's distance matrix (computed once, never modified): the float32 cloud for the plain searches, the embedding of the
    positions as given for the periodic ones."""
    if case.name not in _D:
        if case.periodic:
            _D[case.name] = R.distances(case.pos, None, case.period)
        else:
            _D[case.name] = R.distances(case.cloud32, None if case.queries is None else case.queries.float())
    return _D[case.name]


def host_table(case):
    """[m, k] neighbours from the host path of the entry point the case is about."""
    n, k = case.pos.size(0), case.k
    if case.kind == "query":
        y_idx, x_idx, w = S.knn_interp_weights(case.cloud32, case.queries.float(), k)
        m = case.queries.size(0)
        assert torch.equal(y_idx, torch.arange(m).repeat_interleave(k))
        direct = S.knn_neighbours(case.cloud32.double().numpy(), case.queries.double().numpy(), k)
        assert np.array_equal(direct, x_idx.reshape(m, k).numpy())
        return x_idx.reshape(m, k)
    pos = case.pos.clone() if case.periodic else case.cloud32
    ei, ea = S.connect_knn(pos, k, period=case.period)
    assert ei.dtype == torch.long and tuple(ei.shape) == (2, n * k)
    assert torch.equal(ei[1], torch.arange(n).repeat_interleave(k))
    assert torch.equal(ea, R.edge_attr_ref(pos, ei, case.period))
    return ei[0].reshape(n, k)


# ------------------------------------------------------------------ what the cases claim
def test_the_case_list_covers_what_it_must():
    names = set(K.ids(ALL))
    assert len(ALL) == len(names) and max(c.pos.size(0) for c in ALL) <= 3000
    for dim in (2, 3):
        for stem in ("n_k+1", "n17_k16", "k1", "k8", "k9", "k16", "n255", "n256", "n257", "lattice", "duplicates", "coincident",
                     "degenerate_axes", "thin_strip", "clusters_outlier"):
            assert f"self_{stem}_{dim}d" in names
    assert {c.fallback for c in K.by_kind("perN")} == {None, "few points", "extent", "margin", "own image", "completeness"}
    q = {(c.pos.size(1), c.k <= 8) for c in K.by_kind("query")}
    assert q == {(2, True), (2, False), (3, True), (3, False)}
    assert {c.queries.size(0) for c in K.by_kind("query")} >= {0, 1, 257}
    f64 = next(c for c in ALL if c.name == "self_float64_2d")
    assert f64.pos.dtype == torch.float64 and not torch.equal(f64.pos, f64.cloud32.double())
    assert not any(c.pos.is_contiguous() for c in ALL if "view" in c.name)
    strip = next(c for c in ALL if c.name == "self_thin_strip_2d").cloud32
    ext = strip.max(0).values - strip.min(0).values
    assert float(ext.max() / ext.min()) >= 1e4


@pytest.mark.parametrize("case", ALL, ids=K.ids(ALL))
def test_case_claims_hold(case, monkeypatch):
    D, s, k = reference(case), slack_of(case), case.k
    assert R.tier_gap_ok(D, k, **s), "two distances of one row are neither tied nor clearly apart: choose another seed"
    assert R.tie_free(D, k, **s) == (not case.ties)
    if not case.periodic:
        cloud = case.cloud32
        counts = torch.unique(cloud, dim=0, return_counts=True)[1]
        assert int(counts[counts > 1].sum()) >= case.dups
        if case.dups == 0 and case.kind == "self":
            assert int(counts.max()) == 1
        q = None if case.queries is None else case.queries.float()
        rings, whole = R.rings_needed(cloud, k, q)
        if case.min_rings:
            assert int(rings[~whole].max()) >= case.min_rings
        assert all(bool(whole[i]) for i in case.whole)
        if "outlier" in case.name:
            assert int(rings[case.whole[0]]) >= case.min_rings
    if case.kind == "perN":
        # the construction's host-side logic with a brute-force search in place of the launch (no ties among the fallback clouds'
        # candidates except on the lattice, whose reason does not depend on their order)
        monkeypatch.setattr(S, "knn_query_device", lambda p, q, kq, out=None: R.brute_force_table(p, q, kq))
        why = []
        hit = S._connect_knn_periodic_device(case.pos, k, list(case.period), why)
        if case.fallback is None:
            assert hit is not None and why == (["margin grown"] if case.grown else [])
            R.assert_knn(D, hit[0][0].reshape(-1, k), k, **s)
        else:
            assert hit is None and why[-1] == case.fallback, why


# ------------------------------------------------------------------ the host paths
@pytest.mark.parametrize("case", ALL, ids=K.ids(ALL))
def test_host_path_returns_a_k_nearest_table(case):
    R.assert_knn(reference(case), host_table(case), case.k, **slack_of(case))


# ------------------------------------------------------------------ assert_knn needs every condition
REJECT_ON = [next(c for c in ALL if c.name == n) for n in ("self_lattice_2d", "self_k8_3d", "query_mixed_k12_2d", "per1_lattice_period", "perN_random_2d")]


@pytest.mark.parametrize("case", REJECT_ON, ids=K.ids(REJECT_ON))
def test_perturbed_tables_are_rejected_by_the_condition_they_break(case):
    D, s, k = reference(case), slack_of(case), case.k
    good = host_table(case)
    assert R.violations(D, good, k, **s) == set()
    # the k-th neighbour replaced by the first point of a strictly farther tier: still distinct, complete and ascending
    assert R.violations(D, R.replace_kth_by_farther(D, good, k, **s), k, **s) == {"near"}
    # a repeated index in the last place: the distances still ascend, nothing nearer than the k-th tier is missing
    assert R.violations(D, R.repeat_index(good), k, **s) == {"range"}
    # two neighbours of different tiers swapped
    assert R.violations(D, R.swap_two_tiers(D, good, k, **s), k, **s) == {"ascending"}
    if case.kind != "query":
        # the row's own index: on the inf diagonal, so also "near"; with a zero diagonal only the range condition can object
        assert "range" in R.violations(D, R.own_index(good), k, **s)
        D0 = D.clone().fill_diagonal_(0.0)
        assert "range" in R.violations(D0, R.own_index(good), k, self_mode=True, **s)
        assert R.rejects(R.assert_knn, D, R.own_index(good), k, **s)
    if case.name == "self_lattice_2d":                  # (k = 6 cuts the tier of the four diagonal neighbours: two are spare)
        # a strictly nearer neighbour traded for an unreturned member of the k-th tier: distinct, within kth, ascending
        assert R.violations(D, R.nearer_replaced_by_kth_tier(D, good, k, **s), k, **s) == {"complete"}
    out_of_range = good.clone()
    out_of_range[-1, 0] = -1
    assert R.violations(D, out_of_range, k, **s) == {"range"}
    out_of_range[-1, 0] = D.size(1)
    assert R.rejects(R.assert_knn, D, out_of_range, k, **s)
    assert R.rejects(R.assert_knn, R.worsen_first_neighbour(D, good), good, k, **s)


def test_a_dropped_nearer_neighbour_is_caught_on_a_random_cloud_too():
    """Without ties the k-nearest table is unique, so any change breaks `near` or `range` as well; `complete` must still fire."""
    case = next(c for c in ALL if c.name == "self_k8_3d")
    D, s, k = reference(case), slack_of(case), case.k
    bad = host_table(case).clone()
    far = R.first_of_farther_tier(D, k, **s)
    bad[3] = torch.cat((bad[3, 1:], far[3:4]))
    assert R.violations(D, bad, k, **s) == {"near", "complete"}


def test_rings_needed_on_a_cloud_worked_by_hand():
    """Forty points on a line, unit spacing, k = 1: the stop rule by hand."""
    pts = torch.zeros(40, 2)
    pts[:, 0] = torch.arange(40.0)
    rings, whole = R.rings_needed(pts, 1)
    # cell size h = 39 * (2 / pi) / 40 = 0.62: every point has its own cell, its neighbours are 1 / h = 1.6 cells away: ring 2
    # holds them, and the k-th distance 1 is inside the block's face (>= 2 h = 1.24 away) there
    assert int(rings[20]) == 2 and not bool(whole[20])
    assert int(rings.max()) == 2 and not bool(whole.any())
    q_rings, q_whole = R.rings_needed(pts, 1, torch.tensor([[-1000.0, 0.0], [20.0, 1000.0]]))
    # far beyond the end of the line: cell 0 (clamped), and the face of its first block is 1000 + 2 h away, farther than point 0
    assert int(q_rings[0]) == 1 and not bool(q_whole[0])
    # far off the line's side, above cell 32 of 63: no face is ever 1000 away, the block grows to the whole grid, 32 rings
    assert int(q_rings[1]) == 32 and bool(q_whole[1])


# ------------------------------------------------------------------ argument errors (host)
def test_argument_errors_on_the_host():
    pos = torch.rand(10, 2, generator=torch.Generator().manual_seed(0))
    for dim in (1, 4):
        with pytest.raises(ValueError, match="connect_knn"):
            S.connect_knn(torch.rand(20, dim), 3)
    for period in (None, (1.0, None), ("auto", "auto")):
        for n in (5, 6):                                                       # n < k and n == k
            with pytest.raises(ValueError, match="connect_knn: n="):
                S.connect_knn(pos[:n], 6, period=period)
    with pytest.raises(ValueError, match="connect_knn: n="):
        S.connect_knn(torch.rand(6, 3), 6, period=(None, "auto", None))
    with pytest.raises(ValueError, match="connect_knn: period"):
        S.connect_knn(pos, 3, period=(1.0,))
    for bad in (float("nan"), float("inf")):
        broken = pos.clone()
        broken[4, 1] = bad
        with pytest.raises(ValueError, match="connect_knn: non-finite"):
            S.connect_knn(broken, 3)
        with pytest.raises(ValueError, match="connect_knn: non-finite"):
            S.connect_knn(broken, 3, period=("auto", None))
        with pytest.raises(ValueError, match="non-finite"):
            S.knn_interp_weights(broken, pos, 3)
        with pytest.raises(ValueError, match="non-finite"):
            S.knn_interp_weights(pos, broken, 3)
    with pytest.raises(ValueError, match="knn_interp_weights: k=4"):
        S.knn_interp_weights(pos[:3], pos, 4)
    with pytest.raises(ValueError, match="knn_interp_weights"):
        S.knn_interp_weights(pos, torch.rand(5, 3), 3)
    with pytest.raises(ValueError, match="knn_neighbours"):
        S.knn_neighbours(np.zeros((3, 2)), np.zeros((2, 2)), 4)
    with pytest.raises(ValueError, match="knn_neighbours"):
        S.knn_neighbours(np.zeros((5, 2)), np.zeros((2, 3)), 2)
    y_idx, x_idx, w = S.knn_interp_weights(pos[:3], pos, 3)                    # n == k is allowed for a query
    assert x_idx.numel() == 30


def test_grid_shape_rejects_what_it_cannot_bin():
    lo, hi = torch.tensor([0.0, 0.0]), torch.tensor([1.0, float("nan")])
    with pytest.raises(ValueError, match="g4c_knn_grid.*non-finite"):
        S._grid_shape(lo, hi, 10, 3)
    with pytest.raises(ValueError, match="g4c_knn_grid.*non-finite"):
        S._grid_shape(torch.tensor([float("-inf"), 0.0]), torch.tensor([1.0, 1.0]), 10, 3)
    h, cells = S._grid_shape(torch.tensor([0.5, 0.5]), torch.tensor([0.5, 0.5]), 10, 3)
    assert (h, cells) == (1.0, [1, 1, 1])
