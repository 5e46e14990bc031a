"""Seeded clouds of the periodic tests; each case names the property it exists for (tests/test_periodic_ref.py proves on the CPU that
it has it).  Every coordinate is a multiple of 2^-16 (a dyadic cloud), so coordinates, wrapped offsets and squared distances are
exact in fp32 / fp64 and a table is either right or wrong, never close.

A case: name, pos fp32 [n, dim], k, period (one entry per axis), queries fp32 [m, dim], and the claims:
  nc      the cells per axis of its search grid;
  rings   the largest ring count a self row or a query must reach;
  whole   True: some row ends at "every axis is covered"; split: some row's fastest-axis range splits in two runs;
  queries_only  the case exists for its query rows: few of its self rows have a neighbour across the seam;
  far     the number of trailing queries that are earlier queries shifted by ±3 periods (the periods are powers of two there)."""
from __future__ import annotations

from typing import List

import numpy as np

F32 = np.float32
GRID = 2.0 ** -16


def dyadic(n: int, box, seed: int) -> np.ndarray:
    """n distinct points with coordinates k · 2^-16 in [0, box_a)."""
    rng = np.random.default_rng(seed)
    size = [int(round(b / GRID)) for b in box]
    seen, rows = set(), []
    while len(rows) < n:
        p = tuple(int(rng.integers(0, s)) for s in size)
        if p not in seen:
            seen.add(p)
            rows.append(p)
    return (np.array(rows, dtype=np.float64) * GRID).astype(F32)


def seam_queries(box, m: int, seed: int) -> np.ndarray:
    """m dyadic queries, a third anywhere in the box, two thirds within 1/16 of the box of a face of axis 0 or of the last axis."""
    rng = np.random.default_rng(seed)
    dim = len(box)
    q = np.stack([rng.integers(0, int(round(b / GRID)), m) for b in box], 1).astype(np.float64) * GRID
    for i in range(m):
        if i % 3 == 0:
            continue
        a = 0 if i % 2 else dim - 1
        band = rng.integers(0, int(round(box[a] / 16 / GRID))) * GRID
        q[i, a] = band if i % 4 < 2 else box[a] - GRID - band
    return q.astype(F32)


def with_far(q: np.ndarray, periods, count: int) -> np.ndarray:
    """q and, appended, its first `count` rows shifted by +3 periods (even rows) or −3 periods (odd rows) along every periodic axis."""
    far = q[:count].astype(np.float64).copy()
    for a, L in enumerate(periods):
        if L:
            far[:, a] += np.where(np.arange(count) % 2 == 0, 3.0 * L, -3.0 * L)
    return np.concatenate([q, far.astype(F32)], 0)


def edge_queries_2d() -> np.ndarray:
    """Queries of the [0, 1) x [0, 0.5) box with 8 x 4 cells of 1/8: in the first and the last cell, on a cell face, on the seam."""
    e = GRID
    xs = [0.0, e, 0.125 - e, 0.125, 0.125 + e, 0.5, 0.875 - e, 0.875, 1.0 - e, 1.0]
    ys = [0.0, e, 0.125, 0.25, 0.375, 0.5 - e, 0.5]
    return np.array([(x, y) for x in xs for y in ys], dtype=np.float64).astype(F32)


def sparse_seam(seed: int) -> np.ndarray:
    """A cloud that is dense in the middle of [0, 1) and thin next to the seam of axis 0: the k nearest of a point near the seam lie
    on both sides of it and beyond the first ring of cells."""
    mid = dyadic(140, (0.5, 0.5), seed)
    mid[:, 0] += F32(0.25)
    thin = dyadic(40, (0.375, 0.5), seed + 100)          # -> [0.0625, 0.25) and [0.75, 0.9375): the period 1 exceeds the extent
    thin[:, 0] = np.where(thin[:, 0] < 0.1875, thin[:, 0] + F32(0.0625), thin[:, 0] + F32(0.5625)).astype(F32)
    return np.concatenate([mid, thin], 0).astype(F32)


def cases() -> List[dict]:
    out = []

    def add(name, pos, k, period, queries, far=0, **claims):
        out.append(dict(name=name, pos=pos, k=k, period=period, queries=queries, far=far, **claims))

    b2, b3 = (1.0, 0.5), (1.0, 0.5, 0.25)
    # the dyadic random clouds: 2 000 / 300 / 40 points at k = 12 / 12 / 6
    # (seed 3: seeds 0, 4 and 5 of this generator hold an exact tie among some row's k + 2 nearest)
    add("2000 both axes", dyadic(2000, b2, 3), 12, (1.0, 0.5), with_far(seam_queries(b2, 96, 10), (1.0, 0.5), 16), far=16,
        prop="the dyadic cloud of the accuracy claim; far queries", split=True)
    add("300 both axes, cell edges", dyadic(300, b2, 1), 12, (1.0, 0.5), edge_queries_2d(), nc=(8, 4),
        prop="queries in the first and last cell, on cell faces and on the seam", split=True)
    add("300 axis 0 only", dyadic(300, b2, 2), 12, (1.0, None), seam_queries(b2, 64, 12), prop="one periodic axis of two: the fastest", split=True)
    add("300 axis 1 auto", dyadic(300, b2, 0), 12, (None, "auto"), seam_queries(b2, 64, 13), prop="one periodic axis of two: the slow one, \"auto\"")
    add("40 both axes", dyadic(40, b2, 1), 6, (1.0, 0.5), with_far(seam_queries(b2, 32, 14), (1.0, 0.5), 8), far=8, nc=(4, 2),
        prop="4 and 2 cells along the periodic axes")
    add("20 both axes", dyadic(20, b2, 2), 6, (1.0, 0.5), seam_queries(b2, 32, 15), nc=(3, 1), whole=True,
        prop="3 cells and 1 cell along the periodic axes; ends at the whole grid")
    add("sparse seam, explicit period", sparse_seam(3), 12, (1.0, None), with_far(seam_queries((1.0, 0.5), 64, 16), (1.0, 0.0), 8), far=8, rings=2,
        queries_only=True, prop="QUERIES in the thin band need a second ring across the seam; an explicit period larger than the extent", split=True)
    # 3-D
    add("3-D 300, axis 2 of three", dyadic(300, b3, 0), 12, (None, None, 0.25), seam_queries(b3, 48, 17), prop="one periodic axis of three")
    add("3-D 300, three of three", dyadic(300, b3, 1), 12, (1.0, 0.5, 0.25), with_far(seam_queries(b3, 48, 18), b3, 8), far=8,
        prop="three periodic axes of three", split=True)
    add("3-D 40, three of three", dyadic(40, b3, 2), 6, (1.0, "auto", 0.25), seam_queries(b3, 24, 19),
        prop="a small 3-D grid")
    return out


CASES = cases()
IDS = [c["name"] for c in CASES]
