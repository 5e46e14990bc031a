"""g4c_plan_row_ranges (csrc/plan.cpp): one contiguous row range per persistent workgroup for the weight-stationary kernel's dense pairs
over segments of any length.  Checked against a brute-force restatement: the ranges are contiguous, start and end on segment
boundaries, cover every row once, wg_seg agrees with wg_rows, a range without rows has no segments, and the longest range holds at most
64 P rows for the SMALLEST P for which n_wg such ranges exist.  And the premise the form rests on, on the headline mesh: at 256
workgroups the tiles of whole segments need one round of pairs more than the row ranges, at both coarse levels."""
import ctypes as C

import numpy as np
import pytest
import torch

from graphs4cfd_amd import _lib, plan
from graphs4cfd_amd import synthetic as S


def greedy_count(off, cap):
    """Fewest contiguous ranges of whole segments with at most `cap` rows each (greedy is optimal); None: a segment is longer."""
    n_seg, s, count = len(off) - 1, 0, 0
    while s < n_seg and off[s] < off[-1]:
        e = s
        while e < n_seg and off[e + 1] - off[s] <= cap:
            e += 1
        if e == s:
            return None
        count, s = count + 1, e
    return count


def smallest_pairs(off, n_wg):
    if off[-1] == 0:
        return 0
    p = 1
    while True:
        c = greedy_count(off, 64 * p)
        if c is not None and c <= n_wg:
            return p
        p += 1


def check(off, n_wg):
    off = np.asarray(off, dtype=np.int32)
    rows, seg, pairs, max_seg = plan.row_ranges_host(off, n_wg)
    n_seg = len(off) - 1
    assert rows.shape == (n_wg + 1,) and seg.shape == (n_wg + 1,)
    assert rows[0] == 0 and seg[0] == 0 and rows[-1] == off[-1] and seg[-1] == n_seg          # every row, every segment, once
    assert (np.diff(rows) >= 0).all() and (np.diff(seg) >= 0).all()                            # contiguous, in order
    assert (off[seg] == rows).all()                                                            # on segment boundaries; wg_seg consistent with wg_rows
    lens, segs = np.diff(rows), np.diff(seg)
    if off[-1] > 0:
        assert (segs[lens == 0] == 0).all()                                                    # a range without rows has no segments (no rows at all: nothing launches)
    assert max_seg == segs.max()
    assert pairs == smallest_pairs(off.tolist(), n_wg)
    assert lens.max() <= 64 * pairs
    return rows, seg, pairs


def offsets(deg):
    return np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)


@pytest.mark.parametrize("n_wg", [1, 4, 256])
@pytest.mark.parametrize("seed", [0, 1])
def test_random_degrees_with_empty_segments(n_wg, seed):
    rng = np.random.default_rng(seed)
    for n_seg in (1, 7, 300, 5000):
        check(offsets(rng.integers(0, 9, n_seg)), n_wg)


@pytest.mark.parametrize("n_wg", [1, 4, 256])
@pytest.mark.parametrize("k", [3, 5, 7, 9])
def test_equal_degrees_that_do_not_divide_64(n_wg, k):
    for n_seg in (13, 1000, 4001):
        check(offsets(np.full(n_seg, k)), n_wg)


@pytest.mark.parametrize("n_wg", [1, 4, 256])
def test_one_segment_longer_than_the_lower_bound_capacity(n_wg):
    rng = np.random.default_rng(2)
    deg = rng.integers(1, 9, 2000)
    deg[777] = 3000          # lower bound at 256 workgroups: one pair; this segment alone needs 47
    rows, seg, pairs = check(offsets(deg), n_wg)
    assert pairs >= 47
    if n_wg == 256:
        assert pairs == 47          # P grows until the ranges fit, no further


@pytest.mark.parametrize("n_wg", [4, 256])
def test_fewer_segments_than_workgroups(n_wg):
    rows, seg, pairs = check(offsets([5, 0, 2]), n_wg)
    assert pairs == 1 and (np.diff(rows) > 0).sum() <= 2
    check(offsets([0, 0, 0]), n_wg)          # no rows at all
    check(offsets([0, 0, 3, 0, 0]), n_wg)    # empty segments in front and behind


def test_rows_are_spread_evenly():
    rng = np.random.default_rng(3)
    off = offsets(rng.integers(1, 9, 25000))
    rows, seg, pairs = check(off, 256)
    lens = np.diff(rows)
    assert lens.min() > 0 and lens.max() - lens.min() <= 2 * 8          # each boundary within one segment of the even share


def coarse_offsets(n, seed):
    """Receiver-sorted CSR offsets of the coarse levels' edges of synthetic.mus_graph(n, levels=3), formed as the models' pool_edge
    forms them (g4c_plan_pool_edge_ordered, target-major), on the host."""
    lib = _lib.load()
    g = S.mus_graph(n, levels=3, seed=seed)
    ei = np.ascontiguousarray(g.edge_index.numpy().astype(np.int64))
    out = []
    for h, l in ((1, 2), (2, 3)):
        idx = np.ascontiguousarray(getattr(g, f"idx{h}_to_idx{l}").numpy().astype(np.int64))
        n_edges = ei.shape[1]
        coarse = np.empty((2, max(n_edges, 1)), dtype=np.int64)
        perm, off, kept = np.empty(max(n_edges, 1), np.int32), np.empty(n_edges + 1, np.int32), C.c_int64(0)
        n_coarse = int(lib.g4c_plan_pool_edge_ordered(idx.ctypes.data, idx.shape[0], ei.ctypes.data, n_edges, 1, coarse.ctypes.data,
                                                      perm.ctypes.data, off.ctypes.data, C.byref(kept)))
        assert n_coarse > 0
        ei = np.ascontiguousarray(coarse.reshape(-1)[: 2 * n_coarse].reshape(2, n_coarse))
        n_lr = int(idx.max()) + 1
        col = ei[1]
        assert (np.diff(col) >= 0).all()          # grouped by receiver
        out.append(offsets(np.bincount(col, minlength=n_lr)))
    return out


@pytest.mark.parametrize("seed", [0, 1])
def test_headline_mesh_saves_a_round_of_pairs_at_both_coarse_levels(seed):
    lib = _lib.load()
    for off, want in zip(coarse_offsets(100_000, seed), (7, 2)):
        rows, seg, pairs = check(off, 256)
        assert pairs == want
        n_seg = len(off) - 1
        t_rows, t_seg = np.empty(n_seg + 2, np.int32), np.empty(n_seg + 2, np.int32)
        n_tiles = int(lib.g4c_plan_tiles(off.ctypes.data, n_seg, 32, t_rows.ctypes.data, t_seg.ctypes.data, n_seg + 2))
        assert n_tiles > 0
        whole_segment_pairs = (n_tiles + 1) // 2
        print(f"seed {seed}: {off[-1]} rows, {whole_segment_pairs} whole-segment pairs ({whole_segment_pairs / 256:.2f} per workgroup), "
              f"{(off[-1] + 63) // 64} dense pairs, P = {pairs}")
        assert whole_segment_pairs / 256 > want          # the premise: today's plan needs a round more
