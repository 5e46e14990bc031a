"""Test-only float64 reference of the neighbour searches (csrc/knn_grid.hip and the three constructions of
graphs4cfd_amd/synthetic.py on top of it): the dense distance matrix, brute force, no grid and no tree, and a tie-aware check of
a returned neighbour table against it.

Why tie-aware.  The device search breaks exact ties by cell-sorted position, the host k-d tree its own way; on a lattice or a
cloud with duplicated points the two return different, equally correct tables.  `assert_knn` therefore states what a k-nearest
table IS, per row, with kth the k-th smallest reference distance and slack = rel * kth + abs_:
  (range)     the indices are in range, distinct, and none is the row's own point in self mode;
  (near)      every returned distance is <= kth + slack;
  (complete)  every point with distance < kth - slack is returned;
  (ascending) the returned distances ascend to within slack.
`violations` names the conditions a table breaks, so that a negative control can show that each one is needed.

The slack is derived, not measured:
  NONPERIODIC  rel = 2^-50, abs_ = 0.  Kernel and reference both form the squared distance in float64 from float32 coordinates: the
               differences are exact, at most 3 products and 2 sums are rounded once each (u = 2^-53), on either side of an fma
               contraction: the squared distances agree to 5u each way, the distances to half of that; 2^-50 = 8u covers both sides.
  PERIODIC     abs_ = 2^-46, rel = 0.  The embedding is (cos, sin)(2 pi x / d), coordinates of magnitude at most 1; a device-built
               and a host-built embedding differ by up to 8 ulp (2^-50) per coordinate, over at most 6 coordinates and two
               points: 12 * 2^-50 < 2^-46.  It matters only where a case falls back to the host path.
A case must not let the slack decide anything: any two reference distances of one row are within slack of each other (a tie) or
more than 2^10 * slack apart (`tier_gap_ok`).

`rings_needed` is a plain transcription of the kernel's stop rule (knn_grid_kernel: scan the block of cells within R rings, stop when
the block is the whole grid or the k-th distance is inside the nearest face with cells behind it) on the binning of
`synthetic._bin_cloud`.  It runs on the CPU only, to prove that a case reaches the ring count it claims."""
from __future__ import annotations

from typing import Optional, Sequence, Set, Tuple

import numpy as np
import torch

from .grad_ref import rejects      # noqa: F401

Tensor = torch.Tensor
F64 = torch.float64

NONPERIODIC = dict(rel=2.0 ** -50, abs_=0.0)
PERIODIC = dict(rel=0.0, abs_=2.0 ** -46)
TIER_FACTOR = 2.0 ** 10


# ------------------------------------------------------------------ the reference
def embed(x: Tensor, period: Optional[Sequence], extent_of: Optional[Tensor] = None) -> Tensor:
    """The reference transform's embedding in float64: (cos, sin)(2 pi x / d) per periodic axis, the raw coordinate otherwise;
    d = "auto" is the extent of `extent_of` (the cloud; default x itself) along that axis."""
    x = x.to(F64)
    if period is None or all(d is None for d in period):
        return x
    ref = x if extent_of is None else extent_of.to(F64)
    cols = []
    for ax, d in enumerate(period):
        if d is None:
            cols.append(x[:, ax:ax + 1])
            continue
        d = float(ref[:, ax].max() - ref[:, ax].min()) if isinstance(d, str) and d == "auto" else float(d)
        a = 2 * np.pi / d * x[:, ax]
        cols.append(torch.stack((torch.cos(a), torch.sin(a)), 1))
    return torch.cat(cols, 1)


def distances(points: Tensor, queries: Optional[Tensor] = None, period: Optional[Sequence] = None) -> Tensor:
    """Dense [m, n] Euclidean distances in float64 between the queries (default: the points themselves, then with an inf
    diagonal) and the points, after `embed`; evaluated with torch on the device that holds `points`."""
    p = embed(points, period)
    q = p if queries is None else embed(queries.to(points.device), period, extent_of=points)
    d2 = torch.zeros((q.size(0), p.size(0)), dtype=F64, device=p.device)
    for ax in range(p.size(1)):
        t = q[:, ax, None] - p[None, :, ax]
        d2 += t * t
    D = d2.sqrt()
    if queries is None:
        D.fill_diagonal_(float("inf"))
    return D


def is_self_mode(D: Tensor) -> bool:
    return D.dim() == 2 and D.size(0) == D.size(1) and D.size(0) > 0 and bool(torch.isinf(D.diagonal()).all())


def kth_and_slack(D: Tensor, k: int, rel: float, abs_: float) -> Tuple[Tensor, Tensor]:
    kth = torch.topk(D, k, dim=1, largest=False).values[:, k - 1]
    return kth, rel * kth + abs_


def edge_attr_ref(pos: Tensor, edge_index: Tensor, period: Optional[Sequence]) -> Tensor:
    """pos[col] - pos[row] in the dtype of `pos`, the components of a periodic axis wrapped into [-d/2, d/2] (transforms/connect.py
    :62-71), recomputed from the returned indices."""
    row, col = edge_index.to(pos.device)
    ea = pos[col] - pos[row]
    for ax, d in enumerate(period or ()):
        if d is None:
            continue
        x = pos[:, ax].detach().double()
        d = float(x.max() - x.min()) if isinstance(d, str) and d == "auto" else float(d)
        c = ea[:, ax].clone()
        ea[:, ax] = torch.where(c < -d / 2, c + d, torch.where(c > d / 2, c - d, c))
    return ea


def worsen_first_neighbour(D: Tensor, nbr: Tensor) -> Tensor:
    """A perturbed distance matrix (negative control for a launch's correct table): row 0's first neighbour moved beyond every
    other point."""
    out = D.clone()
    fin = D[0][torch.isfinite(D[0])]
    out[0, int(nbr[0, 0])] = 2.0 * float(fin.max()) + 1.0
    return out


# ------------------------------------------------------------------ the check
def violations(D: Tensor, nbr: Tensor, k: int, rel: float, abs_: float, self_mode: Optional[bool] = None) -> Set[str]:
    """The conditions (module docstring) that the table `nbr` [m, k] breaks against the distance matrix D [m, n]."""
    m, n = int(D.size(0)), int(D.size(1))
    nbr = nbr.to(D.device)
    assert tuple(nbr.shape) == (m, k) and nbr.dtype == torch.long, f"table {tuple(nbr.shape)} {nbr.dtype}, expected [{m}, {k}] int64"
    assert 1 <= k <= n - (1 if (is_self_mode(D) if self_mode is None else self_mode) else 0), f"k={k} of n={n}"
    bad: Set[str] = set()
    if m == 0:
        return bad
    self_mode = is_self_mode(D) if self_mode is None else self_mode
    in_range = (nbr >= 0) & (nbr < n)
    if not bool(in_range.all()):
        return {"range"}                                  # (nothing else can be read off an index outside the matrix)
    if k > 1 and bool((torch.sort(nbr, dim=1).values.diff(dim=1) == 0).any()):
        bad.add("range")
    if self_mode and bool((nbr == torch.arange(m, device=D.device)[:, None]).any()):
        bad.add("range")
    kth, slack = kth_and_slack(D, k, rel, abs_)
    d = torch.gather(D, 1, nbr)
    if not bool((d <= (kth + slack)[:, None]).all()):
        bad.add("near")
    returned = torch.zeros((m, n), dtype=torch.bool, device=D.device)
    returned.scatter_(1, nbr, True)
    if bool(((D < (kth - slack)[:, None]) & ~returned).any()):
        bad.add("complete")
    if k > 1 and not bool((d[:, 1:] >= d[:, :-1] - slack[:, None]).all()):
        bad.add("ascending")
    return bad


def assert_knn(D: Tensor, nbr: Tensor, k: int, rel: float, abs_: float, self_mode: Optional[bool] = None) -> None:
    bad = violations(D, nbr, k, rel, abs_, self_mode)
    assert not bad, f"not a k-nearest table (k={k}, rows={int(D.size(0))}, points={int(D.size(1))}): breaks {sorted(bad)}"


def tier_gap_ok(D: Tensor, k: int, rel: float, abs_: float) -> bool:
    """No two distances of one row lie more than slack and at most 2^10 * slack apart (module docstring): for every distance s, as
    many distances are <= s + slack as are <= s + 2^10 * slack."""
    if D.size(0) == 0:
        return True
    _, slack = kth_and_slack(D, k, rel, abs_)
    s = torch.sort(D, dim=1).values.contiguous()
    near = torch.searchsorted(s, (s + slack[:, None]).contiguous(), right=True)
    far = torch.searchsorted(s, (s + TIER_FACTOR * slack[:, None]).contiguous(), right=True)
    return bool((near == far).all())


def tie_free(D: Tensor, k: int, rel: float, abs_: float) -> bool:
    """True when, in every row, the k + 1 smallest distances are pairwise more than slack apart: the k-nearest table is then
    unique, order included, and the host and device paths must return the same one."""
    if D.size(0) == 0:
        return True
    finite = int(torch.isfinite(D[0]).sum())
    kk = min(k + 1, finite)
    _, slack = kth_and_slack(D, k, rel, abs_)
    s = torch.topk(D, kk, dim=1, largest=False).values
    return kk < 2 or bool((s.diff(dim=1) > slack[:, None]).all())


# ------------------------------------------------------------------ perturbed tables (negative controls; nothing perturbs a launch)
def first_of_farther_tier(D: Tensor, k: int, rel: float, abs_: float) -> Tensor:
    """Per row, the index of the nearest point strictly farther than the k-th tier (distance > kth + slack); -1 where none."""
    kth, slack = kth_and_slack(D, k, rel, abs_)
    far = torch.where(D > (kth + slack)[:, None], D, torch.full_like(D, float("inf")))
    far = torch.where(torch.isinf(D), torch.full_like(D, float("inf")), far)
    val, idx = far.min(dim=1)
    return torch.where(torch.isinf(val), torch.full_like(idx, -1), idx)


def replace_kth_by_farther(D, nbr, k, rel, abs_) -> Tensor:
    out = nbr.clone()
    f = first_of_farther_tier(D, k, rel, abs_).to(nbr.device)
    assert bool((f >= 0).any()), "no row has a point beyond its k-th tier"
    rows = (f >= 0).nonzero().reshape(-1)[:1]
    out[rows, k - 1] = f[rows]
    return out


def repeat_index(nbr: Tensor) -> Tensor:
    """Row 0: the k-th entry replaced by the (k-1)-th (needs k >= 2)."""
    out = nbr.clone()
    out[0, -1] = out[0, -2]
    return out


def own_index(nbr: Tensor) -> Tensor:
    out = nbr.clone()
    out[0, -1] = 0
    return out


def swap_two_tiers(D: Tensor, nbr: Tensor, k: int, rel: float, abs_: float) -> Tensor:
    """The first row that returns two neighbours more than slack apart, with those two swapped."""
    _, slack = kth_and_slack(D, k, rel, abs_)
    d = torch.gather(D, 1, nbr.to(D.device))
    steps = (d.diff(dim=1) > slack[:, None]).nonzero()
    assert steps.numel(), "every row's neighbours are tied"
    r, u = int(steps[0, 0]), int(steps[0, 1])
    out = nbr.clone()
    out[r, u], out[r, u + 1] = nbr[r, u + 1], nbr[r, u]
    return out


def nearer_replaced_by_kth_tier(D: Tensor, nbr: Tensor, k: int, rel: float, abs_: float) -> Tensor:
    """A row whose k-th tier has a member that is not returned and whose first neighbour is strictly nearer than that tier: the
    first neighbour is dropped, the unreturned tier member appended (distinct, in range, within kth, ascending: only
    `complete` can object).  Exists on lattices."""
    kth, slack = kth_and_slack(D, k, rel, abs_)
    nb = nbr.to(D.device)
    returned = torch.zeros_like(D, dtype=torch.bool).scatter_(1, nb, True)
    spare = ((D - kth[:, None]).abs() <= slack[:, None]) & ~returned
    d0 = torch.gather(D, 1, nb[:, :1])[:, 0]
    rows = (spare.any(1) & (d0 < kth - slack)).nonzero().reshape(-1)
    assert rows.numel(), "no row has a spare member of its k-th tier"
    r = int(rows[0])
    out = nbr.clone()
    out[r] = torch.cat((nbr[r, 1:], spare[r].nonzero().reshape(-1)[:1].to(nbr.device)))
    return out


# ------------------------------------------------------------------ the kernel's stop rule, transcribed
def rings_needed(points32: Tensor, k: int, queries32: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """(R, whole) per query: the ring count R at which knn_grid_kernel leaves its loop and whether it left at "the block is the
    whole grid" (R >= max_r) rather than by the distance rule.  Self mode without queries (the point itself is skipped)."""
    from graphs4cfd_amd.synthetic import _grid_shape
    p32 = points32.detach().cpu().float().contiguous()
    n, dim = int(p32.size(0)), int(p32.size(1))
    lo, hi = p32.min(0)[0], p32.max(0)[0]
    h, n_cells = _grid_shape(lo, hi, n, k)
    nc = np.array(n_cells[:dim], dtype=np.int64)
    lo64 = lo.double().numpy()
    org = lo.numpy().astype(np.float64)                      # (the kernel's float origin, widened)

    def cells(x32: Tensor) -> np.ndarray:                    # synthetic._cell_ids
        c = np.floor((x32.double().numpy() - lo64) / h).astype(np.int64)
        return np.clip(c, 0, nc - 1)

    P = p32.double().numpy()
    pc = cells(p32)
    self_mode = queries32 is None
    q32 = p32 if self_mode else queries32.detach().cpu().float().contiguous()
    Q, qc = q32.double().numpy(), cells(q32)
    m = int(q32.size(0))
    R_out, whole = np.zeros(m, dtype=np.int64), np.zeros(m, dtype=bool)
    hd = float(h)
    for s in range(m):
        c = qc[s]
        max_r = int(np.max(np.maximum(c, nc - 1 - c)))
        d2 = ((P - Q[s]) ** 2).sum(1)
        if self_mode:
            d2[s] = np.inf
        ring = np.abs(pc - c).max(1)                         # the block within R rings, clipped to the grid, holds ring <= R
        R = 1
        while True:
            inside = np.sort(d2[ring <= R])
            kth = inside[k - 1] if inside.size >= k else 1e300
            if R >= max_r:
                whole[s] = True
                break
            safe = 1e300
            for a in range(dim):
                if c[a] - R > 0:
                    safe = min(safe, Q[s, a] - (org[a] + float(c[a] - R) * hd))
                if c[a] + R < nc[a] - 1:
                    safe = min(safe, (org[a] + float(c[a] + R + 1) * hd) - Q[s, a])
            safe -= 1e-5 * hd
            if safe > 0.0 and kth <= safe * safe:
                break
            R += 1
        R_out[s] = R
    return torch.from_numpy(R_out), torch.from_numpy(whole)


def brute_force_table(points: Tensor, queries: Tensor, k: int) -> Tensor:
    """[m, k] indices by ascending float64 distance over the float32 roundings of both clouds (ties: lowest index first).  A stand-in
    for `knn_query_device` where the host-side logic of a construction is exercised without a GPU."""
    D = distances(points.float(), queries.float())
    return torch.sort(D, dim=1, stable=True).indices[:, :k].contiguous()
