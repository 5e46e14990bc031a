"""Point clouds for the neighbour-search pins (tests/test_knn_ref.py on the host, tests/test_gpu_knn_ref.py on the device): seeded
clouds of at most 3 000 points, the smallest at which each thing can still go wrong.  Every case names the property it exists for
(`why`) and states what it claims, which tests/test_knn_ref.py proves on the CPU with oracle/knn_ref.py:
  ties        some centre has two of its k + 1 nearest reference distances within slack (lattices, duplicates): host and device may
              then return different, equally correct tables, and only `assert_knn` applies;
  min_rings   the kernel's stop rule (knn_ref.rings_needed) sends some query that ends by the DISTANCE rule to at least that ring;
  whole       the listed queries end at "the block is the whole grid";
  dups        at least that many points coincide with another point of the float32 cloud;
  fallback    the reason `_connect_knn_periodic_device` hands the cloud to the host path (None: it must run on the device);
  grown       the ghost margin of the multi-axis periodic construction has to grow once.
The lattices have a power-of-two spacing, so that their float32 coordinates and the float64 distances between them are exact and
every tier is an exact tie.

Fallbacks of `_connect_knn_periodic_device`: "few points", "extent", "margin", "own image" and "completeness" each have a case.
The sixth `return None` (four margin attempts used up) has none because no input reaches it: ghosts are only ever added, so the
candidates' radius cannot grow from one attempt to the next, the second attempt's need is at most the first's, and the second
margin is 1.25 times the first need."""
from __future__ import annotations

import dataclasses
import math
from typing import Dict, List, Optional, Sequence, Tuple

import torch

Tensor = torch.Tensor


@dataclasses.dataclass
class Case:
    name: str
    kind: str                        # "self" | "query" | "per1" | "perN"
    why: str
    pos: Tensor                      # positions as handed to the entry point (float32 unless the case is about something else)
    k: int
    queries: Optional[Tensor] = None
    period: Optional[Tuple] = None
    ties: bool = False
    min_rings: int = 0
    whole: Sequence[int] = ()
    dups: int = 0
    fallback: Optional[str] = None
    grown: bool = False

    @property
    def cloud32(self) -> Tensor:
        """The cloud the device searches: the float32 rounding of `pos`, contiguous."""
        return self.pos.detach().float().contiguous()

    @property
    def periodic(self) -> bool:
        return self.kind in ("per1", "perN")


def _gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def _rand(n: int, dim: int, seed: int) -> Tensor:
    return torch.rand(n, dim, generator=_gen(seed))


def _lattice(shape: Sequence[int], dx: float = 1.0 / 32) -> Tensor:
    axes = [torch.arange(s, dtype=torch.float64) * dx for s in shape]
    return torch.stack([g.reshape(-1) for g in torch.meshgrid(*axes, indexing="ij")], 1).float()


def _shuffled(x: Tensor, seed: int) -> Tensor:
    return x[torch.randperm(x.size(0), generator=_gen(seed))].contiguous()


# ------------------------------------------------------------------ self search
def _clusters_and_outlier(dim: int, seed: int) -> Tuple[Tensor, List[int]]:
    """Two crowded clusters, a third of 4 points (fewer than k = 6: its points must widen until they reach a crowded one, several
    cells away, and stop there by the distance rule) and one outlier that stretches the grid and can only end at the whole grid."""
    g = _gen(seed)
    L = 64.0
    c = torch.zeros(3, dim)
    c[1, 0] = 0.5 * L
    c[2, 1] = 0.45 * L
    crowd = 200 if dim == 2 else 1000                 # (a 3-D grid over 405 points is 6 cells wide: too coarse for 3 rings)
    pts = [c[0] + 0.01 * torch.randn(crowd, dim, generator=g), c[1] + 0.01 * torch.randn(crowd, dim, generator=g),
           c[2] + 0.01 * torch.randn(4, dim, generator=g), torch.full((1, dim), L)]
    return torch.cat(pts, 0).float(), [2 * crowd + 4]


def self_cases() -> List[Case]:
    out: List[Case] = []
    for dim in (2, 3):
        t = f"{dim}d"
        out.append(Case(f"self_n_k+1_{t}", "self", "n = k + 1: every other point is a neighbour, the grid is a handful of cells", _rand(7, dim, 11 + dim), 6))
        out.append(Case(f"self_n17_k16_{t}", "self", "n = 17, k = 16: the largest k with the fewest points", _rand(17, dim, 13 + dim), 16))
        for k in (1, 8, 9, 16):
            out.append(Case(f"self_k{k}_{t}", "self", "k = 1 / the register instantiations' switch at k <= 8 / the largest k", _rand(300, dim, 100 * k + dim), k))
        for n in (255, 256, 257):
            out.append(Case(f"self_n{n}_{t}", "self", "the 256-thread block edge: last lane of one block, first of a second", _rand(n, dim, n + dim), 6))
        shape = (24, 24) if dim == 2 else (9, 9, 9)
        out.append(Case(f"self_lattice_{t}", "self", "exact ties at every tier; k cuts the second tier", _shuffled(_lattice(shape), 5), 6 if dim == 2 else 9, ties=True))
        base = _rand(600, dim, 17 + dim)
        dup = torch.cat((base, base[:200], base[:50]), 0)
        out.append(Case(f"self_duplicates_{t}", "self", "a third of the points duplicated, some tripled: zero distances, the centre's copies first",
                        _shuffled(dup, 7), 6, ties=True, dups=450))
        out.append(Case(f"self_coincident_{t}", "self", "all points coincident: no extent, the grid collapses to one cell",
                        torch.full((40, dim), 0.375), 6 if dim == 2 else 9, ties=True, dups=40, whole=tuple(range(40))))
        flat = _rand(300, dim, 23 + dim)
        flat[:, 1:] = 0.25
        out.append(Case(f"self_degenerate_axes_{t}", "self", "one (2-D) / two (3-D) axes without extent: one cell along them, out of the cell size", flat, 6 if dim == 2 else 9))
        strip = _rand(1000, dim, 29 + dim)
        strip[:, -1] *= 1e-4
        out.append(Case(f"self_thin_strip_{t}", "self", "extent ratio 1e4: a grid of one cell across", strip, 6))
        pts, whole = _clusters_and_outlier(dim, 31 + dim)
        out.append(Case(f"self_clusters_outlier_{t}", "self", "the search widens ring by ring; the outlier ends at the whole grid", pts, 6, min_rings=3, whole=whole))
    shifted = (_lattice((32, 32), 2.0 ** -13).double() + 4096.0).float()
    out.append(Case("self_lattice_at_4096_2d", "self", "a lattice finer than float32 at its offset: quantisation makes duplicates", _shuffled(shifted, 9), 6, ties=True, dups=512))
    wide = torch.rand(500, 4, generator=_gen(41))
    out.append(Case("self_strided_view_2d", "self", "positions that are a non-contiguous view", wide[:, ::2], 5))
    out.append(Case("self_transposed_view_3d", "self", "positions that are a transposed view", torch.rand(3, 500, generator=_gen(43)).t(), 5))
    out.append(Case("self_float64_2d", "self", "float64 positions that float32 cannot hold: the rounded cloud is searched",
                    torch.rand(400, 2, generator=_gen(47), dtype=torch.float64), 6))
    return out


# ------------------------------------------------------------------ query search
def _queries(points: Tensor, k: int, seed: int, inside: int, outside: int, coincident: int) -> Tensor:
    """Queries inside the box, up to 10 cell sizes outside it, coincident with cloud points, and one 100 extents away."""
    g = _gen(seed)
    n, dim = points.shape
    lo, hi = points.min(0).values, points.max(0).values
    ext = hi - lo
    h = float((ext.prod() * 2.0 * k / (math.pi if dim == 2 else 4.19) / n) ** (1.0 / dim))      # about the search grid's cell size
    q_in = lo + ext * torch.rand(inside, dim, generator=g)
    q_out = lo - 10.0 * h + (ext + 20.0 * h) * torch.rand(outside, dim, generator=g)
    side = torch.randint(0, dim, (outside,), generator=g)
    sign = torch.randint(0, 2, (outside,), generator=g).float()
    push = torch.rand(outside, generator=g) * 10.0 * h
    rows = torch.arange(outside)
    q_out[rows, side] = torch.where(sign > 0, hi[side] + push, lo[side] - push)                  # certainly outside, along one axis
    q_on = points[torch.randperm(n, generator=g)[:coincident]]
    q_far = (hi + 100.0 * ext)[None, :]
    return torch.cat((q_in, q_out, q_on, q_far), 0).float().contiguous()


def query_cases() -> List[Case]:
    out: List[Case] = []
    for dim, k in ((2, 4), (2, 12), (3, 8), (3, 9)):
        pts = _rand(500, dim, 300 + 10 * dim + k)
        q = _queries(pts, k, 400 + 10 * dim + k, 120, 100, 36)
        assert q.size(0) == 257
        out.append(Case(f"query_mixed_k{k}_{dim}d", "query", "queries inside, outside (clamped cells), coincident, 100 extents away; m = 257 spans two blocks",
                        pts, k, queries=q, whole=(256,)))
    out.append(Case("query_n_eq_k_2d", "query", "n == k: every point is a neighbour of every query", _rand(5, 2, 51), 5, queries=_rand(9, 2, 52) * 2 - 0.5))
    out.append(Case("query_n_eq_k_3d", "query", "n == k above the register switch", _rand(9, 3, 53), 9, queries=_rand(9, 3, 54) * 2 - 0.5))
    out.append(Case("query_m0_2d", "query", "no queries: nothing is launched", _rand(50, 2, 55), 3, queries=torch.zeros(0, 2)))
    out.append(Case("query_m1_3d", "query", "one query", _rand(50, 3, 56), 3, queries=_rand(1, 3, 57)))
    lat = _shuffled(_lattice((16, 16)), 58)
    out.append(Case("query_on_lattice_2d", "query", "queries at lattice points and cell centres: exact ties among the hits", lat, 5,
                    queries=torch.cat((lat[:40], lat[40:80] + 1.0 / 64), 0), ties=True))
    return out


# ------------------------------------------------------------------ one periodic axis (2-D)
def per1_cases() -> List[Case]:
    scale = torch.tensor([2.5, 1.0])
    out = [
        Case("per1_random_numeric", "per1", "a numeric period along x", _rand(800, 2, 61) * scale, 6, period=(2.5, None)),
        Case("per1_random_auto", "per1", "period = the extent along y", _rand(800, 2, 62) * scale, 6, period=(None, "auto")),
        Case("per1_lattice_period", "per1", "a lattice whose period is N dx: ties at every tier, through the seam", _shuffled(_lattice((32, 20)), 63), 4,
             period=(1.0, None), ties=True),
        Case("per1_lattice_auto", "per1", "period = extent: the first and last columns coincide in the embedding", _shuffled(_lattice((33, 20)), 64), 4,
             period=("auto", None), ties=True),
        Case("per1_n_2k+3", "per1", "n = 2k + 3: one more point than the 2k + 2 candidates", _rand(13, 2, 65), 5, period=(None, 1.0)),
        Case("per1_n_k+1", "per1", "n = k + 1: fewer points than candidates", _rand(6, 2, 66), 5, period=(1.0, None)),
    ]
    return out


# ------------------------------------------------------------------ two or more periodic axes
def _own_image_cloud() -> Tensor:
    """18 points, x periodic with period 2 pi.  p = (0.1, 0, 0) has 16 tight neighbours 1.3 away in y; c = (pi + 0.2, 0, 0) has
    nothing nearer than p's ghost (pi - 0.1 away) and p itself (pi + 0.1): both are among c's candidates."""
    g = _gen(71)
    crowd = torch.tensor([0.1, 1.3, 0.0]) + 0.01 * torch.randn(16, 3, generator=g)
    crowd[0, 0] = 0.0                                                                  # (the cloud's low corner along x)
    return torch.cat((torch.tensor([[0.1, 0.0, 0.0], [math.pi + 0.2, 0.0, 0.0]]), crowd), 0).float()


def perN_cases() -> List[Case]:
    g = _gen(81)                      # (the existing large graded cloud, shrunk: at 1 500 points x ** 2 is not graded enough for the
    graded = torch.rand(1500, 2, generator=g)   # margin to grow, so 3 % of the points get half of the x range to themselves)
    sparse = torch.rand(1500, generator=g) < 0.03
    graded[:, 0] = torch.where(sparse, 0.5 + 0.5 * graded[:, 0], 0.5 * graded[:, 0])
    graded = graded * torch.tensor([2.5, 1.0])
    lat = _shuffled(_lattice((30, 30)), 82)
    out = [
        Case("perN_random_2d", "perN", "two periodic axes: ghosts at both faces and the corners", _rand(900, 2, 83) * torch.tensor([2.5, 1.0]), 6, period=("auto", "auto")),
        Case("perN_random_3d_one_axis", "perN", "a periodic 3-D cloud, numeric period longer than the extent", _rand(900, 3, 84), 6, period=(None, 1.25, None)),
        Case("perN_random_3d_two_axes", "perN", "two periodic axes of a 3-D cloud", _rand(900, 3, 85) * torch.tensor([2.5, 1.0, 1.5]), 5, period=("auto", None, "auto")),
        Case("perN_lattice_2d", "perN", "a doubly periodic lattice: ties at every tier, through both seams", lat, 4, period=(30.0 / 32, 30.0 / 32), ties=True),
        Case("perN_graded_2d", "perN", "a graded cloud (sparse towards the far x face): the ghost margin has to grow", graded, 6, period=("auto", "auto"), grown=True),
        Case("perN_few_points", "perN", "kc + 1 = 16 points: no room for 16 candidates besides the centre", _rand(16, 2, 86), 6, period=("auto", "auto"), fallback="few points"),
        Case("perN_k14", "perN", "k = 14: the 16 candidates of the grid search are fewer than k + 3", _rand(900, 2, 87), 14, period=("auto", "auto"), fallback="few points"),
        Case("perN_extent_beyond_period", "perN", "an extent longer than the period", _rand(900, 2, 88), 6, period=(0.5, "auto"), fallback="extent"),
        Case("perN_margin_half_period", "perN", "60 points: the ghost margin reaches half a period", _rand(60, 2, 89), 6, period=("auto", "auto"), fallback="margin"),
        Case("perN_own_image", "perN", "a point and its own ghost among one centre's candidates (after the margin grew)", _own_image_cloud(), 6,
             period=(2 * math.pi, None, None), fallback="own image"),
        Case("perN_completeness", "perN", "k = 13 on a lattice: the 14th embedded distance sits in the candidates' outermost tier", lat, 13,
             period=(30.0 / 32, 30.0 / 32), ties=True, fallback="completeness"),
    ]
    return out


_CACHE: Dict[str, List[Case]] = {}


def all_cases() -> List[Case]:
    if "all" not in _CACHE:
        _CACHE["all"] = self_cases() + query_cases() + per1_cases() + perN_cases()
        names = [c.name for c in _CACHE["all"]]
        assert len(set(names)) == len(names)
    return _CACHE["all"]


def by_kind(*kinds: str) -> List[Case]:
    return [c for c in all_cases() if c.kind in kinds]


def ids(cases: Sequence[Case]) -> List[str]:
    return [c.name for c in cases]
