"""Test-only numpy restatement of gfd.BodyForces' geometry and of csrc/body_forces.hip (g4c_body_forces), and the clouds and checkers
its tests share.  Nothing here calls graphs4cfd_amd.

(a) `geometry`: per body the wall nodes sorted by atan2(y − c_y, x − c_x) about the centre c (default: the fp64 mean of the body's
    nodes), ties by node row — or a loop as given, reversed when its shoelace area is negative —; for item w with predecessor a and
    successor b: area[w] = ½ (y_b − y_a, −(x_b − x_a)), ds = |area|, unit = area / ds, arm = pos − c, angle = atan2(arm).  All fp64 from
    the fp32 positions.  The differences and halvings are exact — and so the areas of a loop sum to exactly 0 — as long as the
    coordinates' exponents lie within 29 binades of each other (an fp32 difference then fits fp64's 53 bits).
(b) `terms`: per item, the fp32 gradient loop of tests/gradient_ref.py (`derived32` of 'grad:u', 'grad:v': coefficient 1, so the
    column IS the accumulator), then in fp64, one rounding per operation (numpy never contracts): P = p_scale x[i, p] + p_shift;
    sxx = 2 u_scale G[u][0], sxy = u_scale G[u][1] + v_scale G[v][0], syy = 2 v_scale G[v][1]; tp = (−P a_x, −P a_y);
    tv = mu (sxx a_x + sxy a_y, sxy a_x + syy a_y); the moments r_x t_y − r_y t_x; wall = ((float)P, (float)(mu ((t̂_x sxx + t̂_y sxy) n̂_x
    + (t̂_x sxy + t̂_y syy) n̂_y))), t̂ = (−n̂_y, n̂_x).  mu == 0 skips the gradient: the viscous terms and the shear are 0.
(c) `sum_plain`: numpy's fp64 sum per body; `sum_tree`: the kernel's own order — thread tid adds the items tid, tid + 256, ... of its
    body in that order from 0, then the step-record core's workgroup reduction (tests/step_sum_ref.py).
(d) `sum_bound`: the records' bound on a sum of n terms in any fixed order, 2 (n + 4) 2⁻⁵³ Σ|terms|.

The lumped rule integrates the FORCE of a linear pressure exactly on any polygon (it is the trapezoid rule edge by edge).  The MOMENT's
integrand is quadratic along an edge, so the lumped moment of a linear pressure vanishes not about the polygon's area centroid but
about the rule's own centroid `lumped_centroid` (the two agree to O(h²), and exactly on a regular polygon, whose area vectors are
radial)."""
from __future__ import annotations

import numpy as np

import gradient_ref as GR
from step_sum_ref import THREADS, WAVE, _reduce          # noqa: F401

F32, F64, I32 = np.float32, np.float64, np.int32
NAMES = ("Fp_x", "Fp_y", "Fv_x", "Fv_y", "Mp", "Mv")


# ------------------------------------------------------------------ (a) geometry
def shoelace(xy: np.ndarray) -> float:
    nx = np.roll(xy, -1, 0)
    return 0.5 * float((xy[:, 0] * nx[:, 1] - nx[:, 0] * xy[:, 1]).sum())


def polygon_centroid(xy: np.ndarray) -> np.ndarray:
    """The area centroid of the closed polygon xy [n, 2] (fp64)."""
    nx = np.roll(xy, -1, 0)
    cr = xy[:, 0] * nx[:, 1] - nx[:, 0] * xy[:, 1]
    return ((xy + nx) * cr[:, None]).sum(0) / (6.0 * 0.5 * cr.sum())


def lumped_centroid(xy: np.ndarray, area: np.ndarray) -> np.ndarray:
    """The centre about which the lumped moment of every linear pressure vanishes (module docstring)."""
    x, y, ax, ay = xy[:, 0], xy[:, 1], area[:, 0], area[:, 1]
    a = float((x * ax).sum())                                  # = the shoelace area
    cy = float((x * y * ax).sum() - (x * x * ay).sum()) / a
    cx = float((y * y * ax).sum() - (x * y * ay).sum()) / -a
    return np.array([cx, cy])


def geometry(pos, nodes=None, labels=None, loops=None, centre=None) -> dict:
    xy = np.asarray(pos, dtype=F32).astype(F64)
    if loops is not None:
        members = [np.asarray(lp, dtype=np.int64) for lp in loops]
    else:
        nodes = np.asarray(nodes)
        rows = np.nonzero(nodes)[0] if nodes.dtype == bool else nodes.astype(np.int64)
        members = [rows] if labels is None else [rows[np.asarray(labels) == v] for v in np.unique(labels)]
    c = None if centre is None else np.asarray(centre, dtype=F64).reshape(-1, 2)
    out = dict(items=[], body_offsets=[0], area=[], arm=[], angle=[], centre=[])
    for b, rows in enumerate(members):
        assert rows.size >= 3 and np.unique(rows).size == rows.size
        cb = xy[rows].mean(0) if c is None else c[b]
        if loops is None:
            rows = np.sort(rows)
            d = xy[rows] - cb
            rows = rows[np.argsort(np.arctan2(d[:, 1], d[:, 0]), kind="stable")]
        a2 = shoelace(xy[rows])
        assert a2 != 0.0
        if a2 < 0.0:
            rows = rows[::-1].copy()
        p = xy[rows]
        nxt, prv = np.roll(p, -1, 0), np.roll(p, 1, 0)
        arm = p - cb
        out["items"].append(rows)
        out["body_offsets"].append(out["body_offsets"][-1] + rows.size)
        out["area"].append(np.stack([0.5 * (nxt[:, 1] - prv[:, 1]), -(0.5 * (nxt[:, 0] - prv[:, 0]))], axis=1))
        out["arm"].append(arm)
        out["angle"].append(np.arctan2(arm[:, 1], arm[:, 0]))
        out["centre"].append(cb)
    area = np.concatenate(out["area"])
    ds = np.sqrt(area[:, 0] * area[:, 0] + area[:, 1] * area[:, 1])
    return dict(items=np.concatenate(out["items"]), body_offsets=np.asarray(out["body_offsets"], dtype=I32), area=area,
                unit=area / ds[:, None], ds=ds, arm=np.concatenate(out["arm"]), angle=np.concatenate(out["angle"]),
                centre=np.stack(out["centre"]), n_bodies=len(members))


# ------------------------------------------------------------------ clouds
def ring(n: int, radius=0.5, ratio=1.0, phase=0.25, centre=(0.0, 0.0)) -> np.ndarray:
    """n points on an ellipse of semi-axes (radius, ratio radius), uniform in the parameter, none on an axis (fp32)."""
    th = 2.0 * np.pi * (np.arange(n) + phase) / n
    return np.stack([centre[0] + radius * np.cos(th), centre[1] + ratio * radius * np.sin(th)], axis=1).astype(F32)


def annulus(n: int, counts, seed: int = 0, k: int = 6, lone: bool = True):
    """A cloud of about n nodes round len(counts) circular bodies (counts[b] wall nodes on body b, side by side along x), the fluid
    nodes uniform-random outside every body, in a shuffled node order.  Returns (pos fp32 [N, 2], wall rows [W], labels [W])."""
    rng = np.random.default_rng(1000 * n + 7 * len(counts) + seed)
    centres = [(2.0 * b, 0.0) for b in range(len(counts))]
    walls = [ring(m, 0.5, 1.0, 0.25, centres[b]) for b, m in enumerate(counts)]
    lo, hi = np.array([-1.5, -1.5]), np.array([2.0 * (len(counts) - 1) + 1.5, 1.5])
    fluid = np.zeros((0, 2))
    while fluid.shape[0] < n:
        q = lo + (hi - lo) * rng.random((2 * n, 2))
        keep = np.all([np.hypot(q[:, 0] - cx, q[:, 1] - cy) > 0.56 for cx, cy in centres], axis=0)
        fluid = np.concatenate([fluid, q[keep]])
    pos = np.concatenate(walls + [fluid[:n].astype(F32)])
    label = np.concatenate([np.full(m, 3 + 2 * b) for b, m in enumerate(counts)])          # (labels that need compacting)
    order = rng.permutation(pos.shape[0])
    inv = np.argsort(order)
    return pos[order], inv[:label.size], label


def knn_mesh(pos: np.ndarray, k: int = 6, ragged_seed=None, lone=None) -> GR.Mesh:
    """The k nearest neighbours by brute force (gradient_ref.nearest); ragged_seed drops 0 .. 2 of the farthest per node, `lone` is a
    node left without in-edges."""
    p = np.asarray(pos, dtype=F32).astype(F64)
    nbr = [list(v) for v in GR.nearest(p, k)]
    if ragged_seed is not None:
        drop = np.random.default_rng(ragged_seed).integers(0, 3, len(nbr))
        nbr = [v[:k - int(d)] for v, d in zip(nbr, drop)]
    if lone is not None:
        nbr[int(lone)] = []
    return GR.Mesh(p, *GR._edges(p, nbr))


# ------------------------------------------------------------------ (b) per item
def gradients32(x, off, g, src, ucol: int, vcol: int) -> np.ndarray:
    """[n, 4] fp32 = (du/dx, du/dy, dv/dx, dv/dy) at every node, by gradient_ref's loop."""
    prog = [[(ucol, 0, F32(1.0))], [(ucol, 1, F32(1.0))], [(vcol, 0, F32(1.0))], [(vcol, 1, F32(1.0))]]
    return GR.derived32(np.asarray(x, dtype=F32), off, g, src, prog)


def terms(x, geo: dict, *, pcol: int, ucol: int = 0, vcol: int = 1, mu: float = 0.0, p_scale=1.0, p_shift=0.0, u_scale=1.0, v_scale=1.0,
          off=None, g=None, src=None, col0: int = 0):
    """(T [W, 6] fp64 per-item terms in the order of NAMES, wall [W, 2] fp32, G [W, 4] fp32) of the fields x[:, col0:]."""
    x = np.asarray(x, dtype=F32)[:, col0:]
    it = geo["items"]
    n_items = it.size
    ax, ay, rx, ry = geo["area"][:, 0], geo["area"][:, 1], geo["arm"][:, 0], geo["arm"][:, 1]
    P = F64(p_scale) * x[it, pcol].astype(F64) + F64(p_shift)
    tpx, tpy = -(P * ax), -(P * ay)
    T = np.zeros((n_items, 6), F64)
    T[:, 0], T[:, 1], T[:, 4] = tpx, tpy, rx * tpy - ry * tpx
    G = np.zeros((n_items, 4), F32)
    shear = np.zeros(n_items, F64)
    if mu != 0:
        G = gradients32(np.ascontiguousarray(x), off, g, src, ucol, vcol)[it]
        Gd = G.astype(F64)
        ugx, ugy, vgx, vgy = F64(u_scale) * Gd[:, 0], F64(u_scale) * Gd[:, 1], F64(v_scale) * Gd[:, 2], F64(v_scale) * Gd[:, 3]
        sxx, sxy, syy = 2.0 * ugx, ugy + vgx, 2.0 * vgy
        tvx, tvy = F64(mu) * (sxx * ax + sxy * ay), F64(mu) * (sxy * ax + syy * ay)
        T[:, 2], T[:, 3], T[:, 5] = tvx, tvy, rx * tvy - ry * tvx
        nx, ny = geo["unit"][:, 0], geo["unit"][:, 1]
        tx, ty = -ny, nx
        shear = F64(mu) * ((tx * sxx + ty * sxy) * nx + (tx * sxy + ty * syy) * ny)
    return T, np.stack([P.astype(F32), shear.astype(F32)], axis=1), G


# ------------------------------------------------------------------ (c), (d) sums
def sum_plain(T: np.ndarray, body_offsets) -> np.ndarray:
    return np.stack([T[a:b].sum(0) for a, b in zip(body_offsets[:-1], body_offsets[1:])]) if len(body_offsets) > 1 else np.zeros((0, 6))


def sum_tree(T: np.ndarray, body_offsets) -> np.ndarray:
    out = np.zeros((len(body_offsets) - 1, T.shape[1]), F64)
    for b, (a, e) in enumerate(zip(body_offsets[:-1], body_offsets[1:])):
        acc = np.zeros((THREADS, T.shape[1]), F64)
        for w0 in range(int(a), int(e), THREADS):
            blk = T[w0:min(w0 + THREADS, int(e))]
            acc[:blk.shape[0]] = acc[:blk.shape[0]] + blk
        out[b] = _reduce(acc)
    return out


def sum_bound(T: np.ndarray, body_offsets) -> np.ndarray:
    return np.stack([2.0 * ((b - a) + 4) * 2.0 ** -53 * np.abs(T[a:b]).sum(0) for a, b in zip(body_offsets[:-1], body_offsets[1:])])


def cur32(S: np.ndarray) -> np.ndarray:
    """[B, 3] fp32 = ((float)(Fp_x + Fv_x), (float)(Fp_y + Fv_y), (float)(Mp + Mv)), each sum in fp64 first."""
    return np.stack([S[:, 0] + S[:, 2], S[:, 1] + S[:, 3], S[:, 4] + S[:, 5]], axis=1).astype(F32)


def gradient_bound(x, mesh: GR.Mesh, g64: np.ndarray, g32: np.ndarray, src: np.ndarray, col: int) -> np.ndarray:
    """[n, 2]: |fp32 gradient of x[:, col] − the exact-weights gradient of the same fp32 data| <= 2⁻²³ max_e ||g_e||_inf Σ_e |diff_e| (the
    weights' rounding to fp32, tests/gradient_ref.weights_bound) + (deg + 3) 2⁻²⁴ Σ_e |g_e diff_e| (the fp32 sum, gradient_ref.bound32)."""
    off = mesh.off.astype(np.int64)
    n = off.size - 1
    node = np.repeat(np.arange(n), np.diff(off))
    xd = np.asarray(x, dtype=F32)[:, col].astype(F64)
    diff = np.abs(xd[src] - xd[node])
    top, sdiff = np.zeros(n), np.zeros(n)
    if g64.size:
        np.maximum.at(top, node, np.abs(g64).max(1))
        np.add.at(sdiff, node, diff)
    mag = np.zeros((n, 2))
    for a in range(2):
        np.add.at(mag[:, a], node, np.abs(g32[:, a].astype(F64)) * diff)
    return 2.0 ** -23 * (top * sdiff)[:, None] + (np.diff(off)[:, None] + 3) * 2.0 ** -24 * mag


same, within = GR.same, GR.within
