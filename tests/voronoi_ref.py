"""Test-only restatement of csrc/control_volumes.hip (g4c_voronoi_cells) in plain fp64 — Python floats, one rounding per operation,
never contracted — in two forms, and the clouds their tests share.  Nothing here calls graphs4cfd_amd.

(a) `bin_cloud`: synthetic._bin_cloud on the host (the same cell size, cell ids, stable sort and offsets); `bins_of` takes the device's
    own grid apart instead.
(b) `cells_ring(pos, bins, box, normals)`: the device's order exactly (include/g4c.h, points 1 - 7): the polygon relative to the node,
    the wall half-plane first, the rings of the cell grid row by row, the clip vertex by vertex from vertex 0 with the crossing
    v + (s / (s − s')) (v' − v), the stop on lb² > 4 R², the shoelace sum in vertex order.  Its results are the device's bit for bit.
(c) `cells_sorted(pos, box, normals)`: independent of the grid and of the clip's form: all other points in ascending distance (ties by
    row), the classical Sutherland-Hodgman walk over the edges (previous → current) with the crossing taken from the INSIDE end of
    the edge, duplicates skipped, the stop when the next point is farther than twice the farthest vertex.  `stop=False` is the brute
    force over all points.
Both return a dict of area, centroid, nvert, flags, rings (rings: `cells_ring` only) and `rmax` — the farthest vertex of the final
polygon, the unit 2⁻⁵² rmax² of the area tolerance (tests/VOLUMES_MEASURED.md)."""
from __future__ import annotations

import math

import numpy as np

F32, F64, I32 = np.float32, np.float64, np.int32
MAX_VERTS = 32
BOX, WALL, DUPLICATE, OVERFLOW = 1, 2, 4, 8
TAG_BOX, TAG_BISECTOR, TAG_WALL = 0, 1, 2
GRID_K = 6                 # control_volumes.GRID_K: the cell grid is the one of a k = 6 neighbour search


# ------------------------------------------------------------------ (a) the cell grid
def bin_cloud(pos, k: int = GRID_K) -> dict:
    p32 = np.ascontiguousarray(np.asarray(pos, dtype=F32))
    n = p32.shape[0]
    lo, hi = p32.min(0), p32.max(0)
    ext = hi.astype(F64) - lo.astype(F64)
    live = ext[ext > 0]
    per_cell = 2.0 * k / np.pi
    h = float(F32((float(live.prod()) * per_cell / n) ** (1.0 / live.size))) if live.size else 1.0
    nc = [int(np.floor(float(e) / h)) + 1 for e in ext]
    coord = np.floor((p32.astype(F64) - lo.astype(F64)) / h).astype(np.int64)
    cell = np.clip(coord[:, 0], 0, nc[0] - 1) + np.clip(coord[:, 1], 0, nc[1] - 1) * nc[0]
    order = np.argsort(cell, kind="stable")
    cell_sorted = cell[order]
    return dict(pos_sorted=p32[order], order=order.astype(I32), n_cells=nc, origin=[float(lo[0]), float(lo[1])], h=h,
                cell_start=np.searchsorted(cell_sorted, np.arange(nc[0] * nc[1] + 1)).astype(I32))


def bins_of(grid: dict) -> dict:
    """The device's grid (synthetic._bin_cloud) as host arrays."""
    return dict(pos_sorted=grid["pos_sorted"].cpu().numpy(), order=grid["order"].cpu().numpy(), n_cells=[int(c) for c in grid["n_cells"][:2]],
                origin=[float(grid["org"][0]), float(grid["org"][1])], h=float(grid["h"]), cell_start=grid["cell_start"].cpu().numpy())


def bounding_box(pos) -> tuple:
    p = np.asarray(pos, dtype=F32).astype(F64)
    return (float(p[:, 0].min()), float(p[:, 1].min()), float(p[:, 0].max()), float(p[:, 1].max()))


# ------------------------------------------------------------------ (b) the device's order
def _clip_device(px, py, pt, a, b, c, tag):
    """The polygon (lists) clipped to c − (x a + y b) >= 0 as vc_clip does it: (px, py, pt) or None on overflow."""
    nv = len(px)
    s = [c - (px[j] * a + py[j] * b) for j in range(nv)]
    if not any(v < 0.0 for v in s):
        return px, py, pt
    ox, oy, ot = [], [], []
    for j in range(nv):
        jn = j + 1 if j + 1 < nv else 0
        cs, ns = s[j], s[jn]
        cx, cy, nx, ny = px[j], py[j], px[jn], py[jn]
        if cs >= 0.0:
            if len(ox) >= MAX_VERTS:
                return None
            ox.append(cx)
            oy.append(cy)
            ot.append(tag if (cs == 0.0 and ns < 0.0) else pt[j])
        if (cs > 0.0 and ns < 0.0) or (cs < 0.0 and ns > 0.0):
            if len(ox) >= MAX_VERTS:
                return None
            t = cs / (cs - ns)
            ox.append(cx + t * (nx - cx))
            oy.append(cy + t * (ny - cy))
            ot.append(tag if cs > 0.0 else pt[j])
    return ox, oy, ot


def _finish(px, py, q0, q1):
    """(area, cx, cy, rmax) by the device's shoelace sum about the node."""
    nv = len(px)
    a2 = sx = sy = 0.0
    for j in range(nv):
        jn = j + 1 if j + 1 < nv else 0
        x, y, xn, yn = px[j], py[j], px[jn], py[jn]
        cr = x * yn - xn * y
        a2 += cr
        sx += (x + xn) * cr
        sy += (y + yn) * cr
    rmax = math.sqrt(max([x * x + y * y for x, y in zip(px, py)], default=0.0))
    if nv >= 3 and a2 > 0.0:
        d = 3.0 * a2
        return 0.5 * a2, q0 + sx / d, q1 + sy / d, rmax
    return 0.0, q0, q1, rmax


def _outputs(n):
    return dict(area=np.zeros(n, F64), centroid=np.zeros((n, 2), F64), nvert=np.zeros(n, I32), flags=np.zeros(n, np.uint8),
                rings=np.zeros(n, I32), rmax=np.zeros(n, F64))


def cells_ring(pos, bins: dict, box, normals=None) -> dict:
    ps = np.asarray(bins["pos_sorted"], dtype=F32).astype(F64)
    xs, ys = ps[:, 0].tolist(), ps[:, 1].tolist()
    order = np.asarray(bins["order"]).tolist()
    cstart = np.asarray(bins["cell_start"]).tolist()
    nc0, nc1 = int(bins["n_cells"][0]), int(bins["n_cells"][1])
    o0, o1 = float(F32(bins["origin"][0])), float(F32(bins["origin"][1]))
    h = float(F32(bins["h"]))
    lo0, lo1, hi0, hi1 = (float(v) for v in box)
    nrm = None if normals is None else np.asarray(normals, dtype=F64)
    n = len(xs)
    out = _outputs(n)
    for s in range(n):
        row = order[s]
        q0, q1 = xs[s], ys[s]
        c0 = int(min(max(math.floor((q0 - o0) / h), 0.0), float(nc0 - 1)))
        c1 = int(min(max(math.floor((q1 - o1) / h), 0.0), float(nc1 - 1)))
        px = [lo0 - q0, hi0 - q0, hi0 - q0, lo0 - q0]
        py = [lo1 - q1, lo1 - q1, hi1 - q1, hi1 - q1]
        pt = [TAG_BOX] * 4
        fl, walked, done, overflow = 0, 0, False, False

        def clip(a, b, c, tag):
            nonlocal px, py, pt, done, overflow, fl
            r = _clip_device(px, py, pt, a, b, c, tag)
            if r is None:
                fl |= OVERFLOW
                overflow = done = True
                px, py, pt = [], [], []
                return
            px, py, pt = r
            if len(px) < 3:
                px, py, pt = [], [], []
                done = True

        if nrm is not None:
            n0, n1 = float(nrm[row, 0]), float(nrm[row, 1])
            if n0 != 0.0 or n1 != 0.0:
                fl |= WALL
                clip(-n0, -n1, 0.0, TAG_WALL)
        max_r = max(c0, nc0 - 1 - c0, c1, nc1 - 1 - c1)
        rho = 0
        while rho <= max_r and not done:
            if rho >= 1:
                r2 = 0.0
                for x, y in zip(px, py):
                    r2 = max(r2, x * x + y * y)
                lb = 1e300
                if c0 - rho + 1 > 0:
                    lb = min(lb, q0 - (o0 + float(c0 - rho + 1) * h))
                if c0 + rho - 1 < nc0 - 1:
                    lb = min(lb, (o0 + float(c0 + rho) * h) - q0)
                if c1 - rho + 1 > 0:
                    lb = min(lb, q1 - (o1 + float(c1 - rho + 1) * h))
                if c1 + rho - 1 < nc1 - 1:
                    lb = min(lb, (o1 + float(c1 + rho) * h) - q1)
                lb -= 1e-5 * h
                if lb > 0.0 and lb * lb > 4.0 * r2:
                    break
            walked += 1
            for y in range(c1 - rho, c1 + rho + 1):
                if y < 0 or y >= nc1 or done:
                    continue
                if y == c1 - rho or y == c1 + rho:
                    runs = [(max(c0 - rho, 0), min(c0 + rho, nc0 - 1))]
                else:
                    runs = [(x, x) for x in (c0 - rho, c0 + rho) if 0 <= x < nc0]
                for x0, x1 in runs:
                    if done:
                        break
                    for j in range(cstart[y * nc0 + x0], cstart[y * nc0 + x1 + 1]):
                        if j == s:
                            continue
                        rx, ry = xs[j] - q0, ys[j] - q1
                        d2 = rx * rx + ry * ry
                        if d2 == 0.0:
                            fl |= DUPLICATE
                            continue
                        clip(rx, ry, 0.5 * d2, TAG_BISECTOR)
                        if done:
                            break
            rho += 1
        if any(t == TAG_BOX for t in pt):
            fl |= BOX
        A, g0, g1, rmax = _finish(px, py, q0, q1)
        out["area"][row], out["centroid"][row], out["nvert"][row] = A, (g0, g1), len(px)
        out["flags"][row], out["rings"][row], out["rmax"][row] = fl, walked, rmax
    return out


# ------------------------------------------------------------------ (c) independent of the grid
def _clip_classic(poly, rx, ry, c):
    """poly: a list of (x, y) relative to the node, clipped to x rx + y ry <= c: the textbook walk over the edges previous -> current."""
    out = []
    n = len(poly)
    for j in range(n):
        ax, ay = poly[j - 1]
        bx, by = poly[j]
        da, db = ax * rx + ay * ry - c, bx * rx + by * ry - c          # <= 0: inside
        if db <= 0.0:
            if da > 0.0 and db < 0.0:
                t = db / (db - da)          # from the inside end b
                out.append((bx + t * (ax - bx), by + t * (ay - by)))
            out.append((bx, by))
        elif da < 0.0:
            t = da / (da - db)              # from the inside end a
            out.append((ax + t * (bx - ax), ay + t * (by - ay)))
    return out


def cells_sorted(pos, box, normals=None, stop: bool = True) -> dict:
    p = np.asarray(pos, dtype=F32).astype(F64)
    n = p.shape[0]
    lo0, lo1, hi0, hi1 = (float(v) for v in box)
    nrm = None if normals is None else np.asarray(normals, dtype=F64)
    out = _outputs(n)
    for i in range(n):
        q0, q1 = float(p[i, 0]), float(p[i, 1])
        poly = [(lo0 - q0, lo1 - q1), (hi0 - q0, lo1 - q1), (hi0 - q0, hi1 - q1), (lo0 - q0, hi1 - q1)]
        fl = 0
        if nrm is not None and (nrm[i, 0] != 0.0 or nrm[i, 1] != 0.0):
            fl |= WALL
            poly = _clip_classic(poly, -float(nrm[i, 0]), -float(nrm[i, 1]), 0.0)
        rel = p - p[i]
        d2 = rel[:, 0] * rel[:, 0] + rel[:, 1] * rel[:, 1]
        rows = np.argsort(d2, kind="stable") if stop else np.arange(n)
        for j in rows.tolist():
            if j == i:
                continue
            if d2[j] == 0.0:
                fl |= DUPLICATE
                continue
            if len(poly) < 3:
                break
            if stop and d2[j] > 4.0 * max(x * x + y * y for x, y in poly):
                break
            poly = _clip_classic(poly, float(rel[j, 0]), float(rel[j, 1]), 0.5 * float(d2[j]))
        if len(poly) < 3:
            poly = []
        if len(poly) > MAX_VERTS:
            fl |= OVERFLOW
            poly = []
        A, g0, g1, rmax = _finish([v[0] for v in poly], [v[1] for v in poly], q0, q1)
        out["area"][i], out["centroid"][i], out["nvert"][i], out["flags"][i], out["rmax"][i] = A, (g0, g1), len(poly), fl, rmax
    return out


def area_units(a, b, rmax) -> np.ndarray:
    """|a − b| in units of 2⁻⁵² rmax² per cell (0 where both are 0)."""
    d = np.abs(np.asarray(a) - np.asarray(b))
    with np.errstate(divide="ignore", invalid="ignore"):
        u = d / (2.0 ** -52 * np.asarray(rmax) ** 2)
    return np.where(d == 0.0, 0.0, u)


# ------------------------------------------------------------------ clouds
def uniform_cloud(n: int, seed: int = 0) -> np.ndarray:
    return np.random.default_rng(100 + 7 * n + seed).random((n, 2)).astype(F32)


def jittered_lattice(n: int, seed: int = 0, jitter: float = 0.3) -> np.ndarray:
    """About-square lattice of n nodes (the last row may be short), each moved by up to jitter pitches."""
    m = int(math.ceil(math.sqrt(n)))
    ij = np.stack(np.divmod(np.arange(n), m), axis=1)[:, ::-1].astype(F64)
    rng = np.random.default_rng(300 + 11 * n + seed)
    return ((ij + 0.5 + jitter * (2.0 * rng.random((n, 2)) - 1.0)) / m).astype(F32)


def lattice(m: int, pitch: float = 2.0 ** -5) -> np.ndarray:
    """m × m nodes of pitch 2⁻⁵: every operation on it is exact, and four cells meet at every vertex."""
    j, i = np.divmod(np.arange(m * m), m)
    return (np.stack([i, j], axis=1) * pitch).astype(F32)


def central_ring(m: int, r: float = 0.25, extra: int = 0, seed: int = 0) -> np.ndarray:
    """Node 0 at the centre of m nodes at radius r (none on an axis), and `extra` uniform-random nodes outside radius 2 r in the
    square [−1, 1]²."""
    th = 2.0 * np.pi * (np.arange(m) + 0.25) / m
    pts = [np.zeros((1, 2)), np.stack([r * np.cos(th), r * np.sin(th)], axis=1)]
    if extra:
        rng = np.random.default_rng(500 + m + seed)
        far = np.zeros((0, 2))
        while far.shape[0] < extra:
            c = 2.0 * rng.random((4 * extra, 2)) - 1.0
            far = np.concatenate([far, c[np.hypot(c[:, 0], c[:, 1]) > 2.0 * r]])
        pts.append(far[:extra])
    return np.concatenate(pts).astype(F32)


def shuffled(pos: np.ndarray, seed: int = 0):
    """(pos in a shuffled node order, perm) with shuffled[i] = pos[perm[i]]."""
    perm = np.random.default_rng(900 + seed).permutation(pos.shape[0])
    return np.ascontiguousarray(pos[perm]), perm


def wall_normals(n: int, geo: dict) -> np.ndarray:
    """normals [n, 2] fp64 from forces_ref.geometry: unit[w] at the wall items, zero rows elsewhere."""
    nrm = np.zeros((n, 2), F64)
    nrm[geo["items"]] = geo["unit"]
    return nrm


# ------------------------------------------------------------------ the cases the host and the device tests share
SIZES = (1, 2, 3, 63, 64, 65, 257, 1500)
UNIT_BOX = (0.0, 0.0, 1.0, 1.0)
ANNULI = ((1500, (64,)), (1500, (16,)), (600, (48, 24)))


def duplicates_cloud(n: int = 65):
    """A uniform cloud whose rows 5 and 40 coincide, and rows 7, 8, 9 as well."""
    pos = uniform_cloud(n, seed=3)
    pos[40] = pos[5]
    pos[8] = pos[9] = pos[7]
    return pos


def annulus_case(n: int, counts):
    """(pos, box, normals, geo, exact) of forces_ref.annulus: the wall normals of its bodies, and box − Σ shoelace(body)."""
    import forces_ref as FR
    pos, wall, label = FR.annulus(n, list(counts))
    geo = FR.geometry(pos, nodes=wall, labels=label)
    box = (-1.5, -1.5, 2.0 * (len(counts) - 1) + 1.5, 1.5)
    p = np.asarray(pos, dtype=F32).astype(F64)
    off = geo["body_offsets"]
    bodies = sum(FR.shoelace(p[geo["items"][a:b]]) for a, b in zip(off[:-1], off[1:]))
    return pos, box, wall_normals(pos.shape[0], geo), geo, (box[2] - box[0]) * (box[3] - box[1]) - bodies


def cases():
    """(name, pos, box, normals) of every cloud the area tolerance is measured on (tests/VOLUMES_MEASURED.md)."""
    for gen in (uniform_cloud, jittered_lattice):
        for n in SIZES:
            yield f"{gen.__name__}-{n}", gen(n), UNIT_BOX, None
    yield "lattice-9", lattice(9), bounding_box(lattice(9)), None
    for m in (24, 40):
        yield f"central-ring-{m}", central_ring(m, 0.25, 200), (-1.0, -1.0, 1.0, 1.0), None
    yield "duplicates-65", duplicates_cloud(), UNIT_BOX, None
    yield "box-twice-257", uniform_cloud(257), (-0.5, -0.5, 1.5, 1.5), None
    for n, counts in ANNULI:
        pos, box, nrm, _, _ = annulus_case(n, counts)
        yield f"annulus-{n}-{'-'.join(str(c) for c in counts)}", pos, box, nrm


# The largest |cells_ring − cells_sorted| over `cases()`, in units of 2⁻⁵² rmax² (measured on the host before any kernel ran:
# tests/test_voronoi_ref.py pins it, tests/VOLUMES_MEASURED.md records it), and what the device is held to: 8 × that.
MEASURED_UNITS = 128.3          # (128.233.. on annulus-1500-64, rounded up)
DEVICE_UNITS = 8.0 * MEASURED_UNITS
