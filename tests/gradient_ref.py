"""Test-only numpy restatement of csrc/mesh_gradient.hip (g4c_mesh_gradient_weights, g4c_mesh_derived) and the meshes, programs and
checkers its tests share.  Nothing here calls graphs4cfd_amd.

(a) `weights`: per node i over its in-edges in CSR order (edge pe = perm[off[i] + s], or off[i] + s without perm), all fp64:
    d_e = -rel_e, w_e = |d_e|^-power, M = Σ w_e d_e d_eᵀ; degenerate iff not det M > 1e-12 (tr M / dim)^dim (det <= the threshold, or a
    determinant that is no number); g_e = 0 there, else w_e M⁻¹ d_e with M⁻¹ by the adjugate; g rounded to fp32 once; src = src32[pe].
(b) `derived32`: the per-step arithmetic as a numpy.float32 loop in the stated order: G[f][a] = 0; over the in-edges in CSR order
    diff = x[src_e, f] - x[i, f], p = g[e][a] * diff, G[f][a] += p; column = (c0 G0 + c1 G1) + c2 G2.  (The loop runs over the
    in-edge slot s = 0, 1, ... and is vectorised over the nodes: every node still adds its own terms one at a time, in order.)
(c) `derived64`: the same in fp64 from the fp32 g and x, and Σ|terms| = Σ_k |c_k| Σ_e |g[e][a]| |diff_e| per node and column.
(d) `stats64`: (Σq², Σ|q|, max|q|) over the nodes in fp64.

`wrong=` names ONE deliberate mistake for the negative controls: "transposed-g" (the weights of the reversed edge direction,
d_e = +rel_e), "src-unpermuted" (src = src32[off[i] + s], the permutation forgotten), "vort-sign" (∂₁u − ∂₀v)."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

F32, F64, I32 = np.float32, np.float64, np.int32
WRONG = ("transposed-g", "src-unpermuted", "vort-sign")
AXES = "xyz"


# ------------------------------------------------------------------ meshes
def csr_of(col: np.ndarray, n: int) -> Tuple[np.ndarray, Optional[np.ndarray]]:
    """(off int32 [n + 1], perm int32 [E] or None when the edges are grouped by target already) — stable grouping."""
    col = np.asarray(col, dtype=np.int64)
    perm = np.argsort(col, kind="stable").astype(I32)
    off = np.zeros(n + 1, dtype=I32)
    off[1:] = np.cumsum(np.bincount(col, minlength=n))[:n] if n else 0
    return off, (None if np.array_equal(perm, np.arange(col.size)) else perm)


def nearest(pos: np.ndarray, k: int) -> np.ndarray:
    """[n, k] brute-force nearest OTHER points, nearest first (fp64 distances, ties by index)."""
    d = ((pos[:, None, :] - pos[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d, np.inf)
    return np.argsort(d, axis=1, kind="stable")[:, :k]


def ratio(off, perm, rel, dim: int, power: int) -> np.ndarray:
    """det M / (tr M / dim)^dim per node (nan where it is no number, 0 for a node without in-edges)."""
    det, tr = _normal(off, perm, rel, dim, power)[1:3]
    with np.errstate(all="ignore"):
        r = det / (tr / dim) ** dim
    r[tr == 0] = 0.0
    return r


class Mesh:
    """pos [n, dim] fp64, row (senders) / col (receivers) int64 [E], rel [E, dim] fp32 = receiver - sender (planted nodes: edited),
    planted: the nodes whose rel was edited (they have no slope to give back), kinds: node -> what was planted."""

    def __init__(self, pos, row, col, rel, planted=()):
        self.pos, self.row, self.col, self.rel, self.planted = pos, row.astype(np.int64), col.astype(np.int64), rel.astype(F32), dict(planted)
        self.n, self.dim = int(pos.shape[0]), int(pos.shape[1])
        self.off, self.perm = csr_of(self.col, self.n)
        self.src32 = self.row.astype(I32)
        self.max_deg = int(np.diff(self.off).max()) if self.n else 0

    def shuffled(self, seed: int) -> "Mesh":
        p = np.random.default_rng(seed).permutation(self.row.size)
        return Mesh(self.pos, self.row[p], self.col[p], self.rel[p], self.planted)


def _edges(pos, nbr_lists) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    col = np.concatenate([np.full(len(v), i, dtype=np.int64) for i, v in enumerate(nbr_lists)] + [np.zeros(0, np.int64)])
    row = np.concatenate([np.asarray(v, dtype=np.int64) for v in nbr_lists] + [np.zeros(0, np.int64)])
    rel = (pos[col] - pos[row]).astype(F32) if row.size else np.zeros((0, pos.shape[1]), F32)
    return row, col, rel


def uniform_mesh(n: int, dim: int, k: int = 6, seed: int = 0) -> Mesh:
    """Uniform in-degree k: the k nearest neighbours of a uniform-random cloud; with n <= k the senders are drawn from all the nodes
    (self-loops included: such meshes are degenerate everywhere)."""
    rng = np.random.default_rng(100 * n + 10 * dim + seed)
    pos = rng.random((n, dim))
    if n == 0:
        return Mesh(pos, np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, dim), F32))
    nbr = nearest(pos, k) if n > k else rng.integers(0, n, (n, k))
    return Mesh(pos, *_edges(pos, list(nbr)))


def ragged_mesh(n: int, dim: int, seed: int = 0) -> Mesh:
    """In-degrees 0 .. 11 (the nearest neighbours first) with empty segments and planted degenerate nodes: no in-edge, one in-edge,
    collinear neighbours, coplanar neighbours (3-D), a zero-length edge.  Every other node whose neighbours condition its normal
    matrix worse than 1e-2 (under any power) is given more of them, so that no node sits near the threshold."""
    rng = np.random.default_rng(100 * n + 10 * dim + 5 + seed)
    pos = rng.random((n, dim))
    if n == 0:
        return Mesh(pos, np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, dim), F32))
    kmax = min(11, n - 1)
    order = nearest(pos, kmax) if kmax else np.zeros((n, 0), np.int64)
    deg = rng.integers(0, kmax + 1, n)
    kinds = ["none", "one", "collinear", "zero-edge"] + (["coplanar"] if dim == 3 else [])
    planted = {}
    if n >= 20:
        for j, node in enumerate(rng.choice(n, size=2 * len(kinds), replace=False)):
            planted[int(node)] = kinds[j % len(kinds)]
    for node, kind in planted.items():
        deg[node] = {"none": 0, "one": 1, "collinear": 4, "coplanar": 5, "zero-edge": 7}[kind]

    def build(deg):
        row, col, rel = _edges(pos, [order[i, :deg[i]] for i in range(n)])
        off = np.zeros(n + 1, np.int64)
        off[1:] = np.cumsum(deg)
        for node, kind in planted.items():
            e = slice(off[node], off[node + 1])
            m = int(deg[node])
            if kind == "collinear":
                rel[e] = np.outer(np.arange(1, m + 1) * np.where(np.arange(m) % 2, -1.0, 1.0), np.linspace(0.25, 0.5, dim)).astype(F32)
            elif kind == "coplanar":
                rel[e, 2] = 0.0          # (the plane z = 0 exactly: a rounded oblique plane would not be one)
            elif kind == "zero-edge":
                rel[off[node] + 2] = 0.0
        return row, col, rel

    for _ in range(3):
        row, col, rel = build(deg)
        off, _ = csr_of(col, n)
        with np.errstate(all="ignore"):
            worst = np.nanmin(np.stack([np.nan_to_num(ratio(off, None, rel, dim, p), nan=np.inf) for p in (0, 1, 2)]), axis=0)
        bad = [i for i in range(n) if i not in planted and deg[i] > 0 and (deg[i] <= dim or worst[i] < 1e-2) and kmax > dim]
        bad += [i for i, kind in planted.items() if kind == "zero-edge" and worst[i] < 1e-2 and deg[i] < kmax]
        if not bad:
            break
        for i in bad:
            deg[i] = min(max(deg[i] + 3, 6), kmax)
    return Mesh(pos, row, col, rel, planted)


# ------------------------------------------------------------------ (a) weights
def _normal(off, perm, rel, dim: int, power: int, sign: float = -1.0):
    """Per node, in CSR order, fp64: (M [n, dim, dim], det [n], tr [n], d [E, dim] in CSR order, w [E] in CSR order)."""
    off = np.asarray(off, dtype=np.int64)
    n, n_e = off.size - 1, int(off[-1]) if off.size else 0
    pe = np.arange(n_e) if perm is None else np.asarray(perm, dtype=np.int64)
    d = sign * np.asarray(rel, dtype=F32)[pe].astype(F64)
    with np.errstate(all="ignore"):
        r2 = np.zeros(n_e)
        for a in range(dim):
            r2 = r2 + d[:, a] * d[:, a]
        w = np.ones(n_e) if power == 0 else (1.0 / np.sqrt(r2) if power == 1 else 1.0 / r2)
        m = np.zeros((n, dim, dim))
        deg = np.diff(off)
        for s in range(int(deg.max()) if n else 0):          # the s-th in-edge of every node that has one: M += w d dᵀ in CSR order
            nodes = np.nonzero(deg > s)[0]
            e = off[nodes] + s
            for a in range(dim):
                for b in range(a, dim):
                    m[nodes, a, b] += (w[e] * d[e, a]) * d[e, b]
        for a in range(dim):
            for b in range(a):
                m[:, a, b] = m[:, b, a]
        if dim == 2:
            det = m[:, 0, 0] * m[:, 1, 1] - m[:, 0, 1] * m[:, 0, 1]
            tr = m[:, 0, 0] + m[:, 1, 1]
        else:
            det = ((m[:, 0, 0] * (m[:, 1, 1] * m[:, 2, 2] - m[:, 1, 2] * m[:, 1, 2])
                    + m[:, 0, 1] * (m[:, 0, 2] * m[:, 1, 2] - m[:, 0, 1] * m[:, 2, 2]))
                   + m[:, 0, 2] * (m[:, 0, 1] * m[:, 1, 2] - m[:, 0, 2] * m[:, 1, 1]))
            tr = (m[:, 0, 0] + m[:, 1, 1]) + m[:, 2, 2]
    return m, det, tr, d, w


def _adjugate(m, dim):
    adj = np.empty_like(m)
    if dim == 2:
        adj[:, 0, 0], adj[:, 1, 1] = m[:, 1, 1], m[:, 0, 0]
        adj[:, 0, 1] = adj[:, 1, 0] = -m[:, 0, 1]
        return adj
    for a in range(3):
        for b in range(3):
            r = [i for i in range(3) if i != b]
            c = [i for i in range(3) if i != a]
            minor = m[:, r[0], c[0]] * m[:, r[1], c[1]] - m[:, r[0], c[1]] * m[:, r[1], c[0]]
            adj[:, a, b] = minor if (a + b) % 2 == 0 else -minor
    return adj


def weights(off, perm, src32, rel, dim: int, power: int, wrong: Optional[str] = None):
    """(g64 [E, dim] fp64, g [E, dim] fp32 = its rounding, src int32 [E], degenerate uint8 [n]) in CSR order."""
    assert wrong is None or wrong in WRONG, wrong
    off = np.asarray(off, dtype=np.int64)
    n, n_e = off.size - 1, int(off[-1]) if off.size else 0
    m, det, tr, d, w = _normal(off, perm, rel, dim, power, sign=1.0 if wrong == "transposed-g" else -1.0)
    with np.errstate(all="ignore"):
        thr = 1e-12 * (tr / dim) ** dim
        degen = ~(det > thr)
        adj = _adjugate(m, dim)
        node = np.repeat(np.arange(n), np.diff(off))
        v = np.einsum("eab,eb->ea", adj[node], d)
        g64 = (w / det[node])[:, None] * v
    g64[degen[node]] = 0.0
    pe = np.arange(n_e) if (perm is None or wrong == "src-unpermuted") else np.asarray(perm, dtype=np.int64)
    return g64, g64.astype(F32), np.asarray(src32, dtype=I32)[pe], degen.astype(np.uint8)


def lstsq_weights(off, perm, rel, dim: int, power: int) -> np.ndarray:
    """The same g by numpy.linalg.lstsq per node (non-degenerate nodes only make sense): row a of pinv(√w D) √w."""
    off = np.asarray(off, dtype=np.int64)
    n_e = int(off[-1])
    pe = np.arange(n_e) if perm is None else np.asarray(perm, dtype=np.int64)
    d = -np.asarray(rel, dtype=F32)[pe].astype(F64)
    out = np.zeros((n_e, dim))
    for i in range(off.size - 1):
        e = slice(off[i], off[i + 1])
        if off[i + 1] - off[i] < dim:
            continue
        with np.errstate(all="ignore"):
            sw = np.sqrt(np.linalg.norm(d[e], axis=1) ** -float(power)) if power else np.ones(off[i + 1] - off[i])
        if not np.isfinite(sw).all():
            continue
        a = sw[:, None] * d[e]
        sol = np.linalg.lstsq(a, np.diag(sw), rcond=None)[0]          # [dim, deg]: grad = sol @ (x_j - x_i)
        out[e] = sol.T
    return out


# ------------------------------------------------------------------ programs
def columns(names: Sequence[str], dim: int) -> List[str]:
    out = []
    for name in names:
        if name == "div":
            out.append("div")
        elif name == "vort":
            out += ["vort"] if dim == 2 else [f"vort_{a}" for a in AXES]
        else:
            assert name.startswith("grad:"), name
            out += [f"d{int(name[5:])}/d{AXES[a]}" for a in range(dim)]
    return out


def program(names: Sequence[str], dim: int, nf: int, velocity=None, field_scale=None, wrong: Optional[str] = None):
    """[[(field, axis, coef fp32), ...] per column]."""
    vel = tuple(range(dim)) if velocity is None else tuple(velocity)
    sc = np.ones(nf, F32) if field_scale is None else np.asarray(field_scale, dtype=F32)
    flip = F32(-1.0) if wrong == "vort-sign" else F32(1.0)

    def t(field, axis, sign=1.0):
        return (int(field), int(axis), F32(F32(sign) * sc[field]))

    prog = []
    for name in names:
        if name == "div":
            prog.append([t(vel[a], a) for a in range(dim)])
        elif name == "vort":
            if dim == 2:
                prog.append([t(vel[1], 0, flip), t(vel[0], 1, -flip)])
            else:
                u, v, w = vel
                prog += [[t(w, 1, flip), t(v, 2, -flip)], [t(u, 2, flip), t(w, 0, -flip)], [t(v, 0, flip), t(u, 1, -flip)]]
        else:
            prog += [[t(int(name[5:]), a)] for a in range(dim)]
    return prog


# ------------------------------------------------------------------ (b), (c) per step
def _gradients(x, off, g, src, fields, dtype):
    """{f: G [n, dim]} and {f: A [n, dim]} with A = Σ_e |g[e][a]| |diff_e| (fp64), accumulated in CSR order in `dtype`."""
    off = np.asarray(off, dtype=np.int64)
    n, dim = off.size - 1, g.shape[1]
    xx, gg = np.asarray(x).astype(dtype), np.asarray(g).astype(dtype)
    deg = np.diff(off)
    G = {f: np.zeros((n, dim), dtype) for f in fields}
    A = {f: np.zeros((n, dim), F64) for f in fields}
    for s in range(int(deg.max()) if n else 0):
        nodes = np.nonzero(deg > s)[0]
        e = off[nodes] + s
        for f in fields:
            diff = xx[src[e], f] - xx[nodes, f]
            for a in range(dim):
                p = gg[e, a] * diff
                G[f][nodes, a] += p
                A[f][nodes, a] += np.abs(gg[e, a].astype(F64)) * np.abs(diff.astype(F64))
    return G, A


def _combine(G, A, prog, n, dtype):
    cur, mag = np.zeros((n, len(prog)), dtype), np.zeros((n, len(prog)), F64)
    for c, col in enumerate(prog):
        q = None
        for (f, a, coef) in col:
            pr = dtype(coef) * G[f][:, a]
            q = pr if q is None else q + pr
            mag[:, c] += abs(float(coef)) * A[f][:, a]
        cur[:, c] = q
    return cur, mag


def derived32(x, off, g, src, prog) -> np.ndarray:
    """(b): cur [n, nd] fp32, the bits the device must give."""
    fields = sorted({f for col in prog for (f, _, _) in col})
    G, A = _gradients(np.asarray(x, dtype=F32), off, np.asarray(g, dtype=F32), src, fields, F32)
    return _combine(G, A, prog, len(off) - 1, F32)[0]


def derived64(x, off, g, src, prog) -> Tuple[np.ndarray, np.ndarray]:
    """(c): (cur [n, nd] fp64 from the fp32 g and x, Σ|terms| [n, nd])."""
    fields = sorted({f for col in prog for (f, _, _) in col})
    G, A = _gradients(np.asarray(x, dtype=F32), off, np.asarray(g, dtype=F32), src, fields, F64)
    return _combine(G, A, prog, len(off) - 1, F64)


def bound32(mag: np.ndarray, max_deg: int) -> np.ndarray:
    """|cur32 − cur64| <= (max_deg + 3) 2⁻²⁴ Σ|terms|."""
    return (max_deg + 3) * 2.0 ** -24 * mag


# ------------------------------------------------------------------ (d) statistics, slots
def stats64(cur) -> np.ndarray:
    """[nd, 3] = (Σq², Σ|q|, max|q|) over the nodes, fp64 (max of no node: 0)."""
    q = np.asarray(cur).astype(F64)
    mx = np.abs(q).max(0) if q.shape[0] else np.zeros(q.shape[1])
    return np.stack([(q * q).sum(0), np.abs(q).sum(0), mx], axis=1)


def stats_bound(cur) -> np.ndarray:
    """The records' bound on a sum of n terms added in any fixed order: 2 (n + 4) 2⁻⁵³ Σ|terms|, for Σq² and Σ|q| ([nd, 2])."""
    q = np.asarray(cur).astype(F64)
    n = q.shape[0]
    return 2.0 * (n + 4) * 2.0 ** -53 * np.stack([(q * q).sum(0), np.abs(q).sum(0)], axis=1)


def snap_slot(t: int, every: int, n_snap: int) -> Optional[int]:
    if every > 0 and t >= 0 and (t + 1) % every == 0 and (t + 1) // every - 1 < n_snap:
        return (t + 1) // every - 1
    return None


# ------------------------------------------------------------------ checkers
def same(got, ref: np.ndarray, what: str = "") -> None:
    """Bit for bit (values; nan equals nan)."""
    g = got.detach().cpu().numpy() if hasattr(got, "detach") else np.asarray(got)
    ref = np.asarray(ref)
    assert g.dtype == ref.dtype and tuple(g.shape) == tuple(ref.shape), f"{what}: {g.dtype} {g.shape} vs {ref.dtype} {ref.shape}"
    bad = ~((g == ref) | ((g != g) & (ref != ref)))
    if bad.any():
        pos = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at {list(pos)}: got {g[pos]!r} want {ref[pos]!r}")


def within(got, ref: np.ndarray, allowed: np.ndarray, what: str = "") -> float:
    """|got − ref| <= allowed elementwise; returns the largest measured / allowed ratio (0 where both are 0)."""
    g = got.detach().cpu().numpy() if hasattr(got, "detach") else np.asarray(got)
    assert tuple(g.shape) == tuple(np.shape(ref)), f"{what}: {g.shape} vs {np.shape(ref)}"
    err = np.abs(g.astype(F64) - np.asarray(ref, dtype=F64))
    allowed = np.broadcast_to(np.asarray(allowed, dtype=F64), err.shape)
    bad = ~(err <= allowed)
    if bad.any():
        pos = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements are outside the bound, first at {list(pos)}: got {g[pos]!r} "
                             f"want {np.asarray(ref)[pos]!r}, allowed {allowed[pos]!r}")
    with np.errstate(all="ignore"):
        r = np.where(allowed > 0, err / allowed, 0.0)
    return float(r.max()) if r.size else 0.0


def weights_bound(g64: np.ndarray, off) -> np.ndarray:
    """[E, 1]: 2⁻²³ max_e ||g_ref,e||_inf per node, spread over its edges."""
    off = np.asarray(off, dtype=np.int64)
    n = off.size - 1
    node = np.repeat(np.arange(n), np.diff(off))
    top = np.zeros(n)
    if g64.size:
        np.maximum.at(top, node, np.abs(g64).max(1))
    return (2.0 ** -23 * top[node])[:, None]


def rejects(check, *args, **kw) -> bool:
    try:
        check(*args, **kw)
    except AssertionError:
        return True
    return False
