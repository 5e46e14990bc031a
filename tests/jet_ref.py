"""Test-only numpy restatement of csrc/mesh_jet.hip (g4c_mesh_jet_weights, g4c_mesh_jet, g4c_mesh_jet_adjoint), of what
`ResidualLoss` (nn/losses.py) makes of them, and the meshes their tests share.  No torch device; nothing here calls graphs4cfd_amd.

Q = dim + dim (dim + 1) / 2 derivatives per field: 0 .. dim − 1 the first, then xx, xy, yy (2-D) or xx, xy, xz, yy, yz, zz (3-D).

(a) `weights`: per node over its stencil entries in CSR order (entry pe = perm[off[i] + s], or off[i] + s without perm), all fp64, in
    the kernel's order of operations (include/g4c.h): d = −rel, r² = Σ d_a d_a, w = |d|^−power; the row b = (d, then d_a d_b', halved on
    the diagonal); A_ij += (w b_i) b_j (lower triangle); sc_i = 1 / sqrt(A_ii), A_ij <- (A_ij sc_i) sc_j; Cholesky by columns with the
    pivots pivot_j = A_jj − Σ_k L_jk² subtracted one by one; degenerate iff fewer than Q entries, a weight that is not finite, or a
    pivot that is not > 1e-12; per entry L y = sc·b, Lᵀ z = y, c = (w sc) z rounded to fp32 once; src = src32[pe].  (Vectorised over
    the nodes: every node still does its own operations one at a time, in order.)
(b) `lstsq_weights`: the same rows by numpy.linalg.lstsq per node — no normal matrix, no Cholesky.
(c) `derived32` / `derived64`, `adjoint32` / `adjoint64`: the per-call arithmetic.  With c [S, Q] in the place of g [E, dim] these are
    the loops of tests/gradient_ref.py and tests/adjoint_op_ref.py word for word (both are written over the width of their table),
    so they are taken from there.
(d) `residual64`: R_a = (U_a − U_a^prev) / dt + Σ_b U_b ∂_b U_a + (1 / ρ) ∂_a P − ν ∇²U_a and C = Σ_a ∂_a U_a from a jet table in fp64.
(e) `ResidualRef`: ResidualLoss's value in fp64, its gradient with respect to pred, and how far fp32 may sit from both.

`wrong=` names ONE deliberate mistake for the negative controls — weights: "sign" (d = +rel), "diagonal-factor" (the ½ on the
diagonal second-order terms forgotten), "src-unpermuted"; residual: "advection-sign", "viscous-factor" (2ν), "pressure-sign",
"no-time"."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

import adjoint_op_ref as A
import gradient_ref as R

F32, F64, I32 = np.float32, np.float64, np.int32
U = 2.0 ** -24
WRONG_WEIGHTS = ("sign", "diagonal-factor", "src-unpermuted")
WRONG_RESIDUAL = ("advection-sign", "viscous-factor", "pressure-sign", "no-time")
AXES = "xyz"
SUGGESTED_K = {2: 12, 3: 20}

same, within, rejects, weights_bound, csr_of, nearest = R.same, R.within, R.rejects, R.weights_bound, R.csr_of, R.nearest
sender_csr, dst_of, fields_of = A.sender_csr, A.dst_of, A.fields_of


def q_of(dim: int) -> int:
    return dim + dim * (dim + 1) // 2


def pairs(dim: int) -> List[Tuple[int, int]]:
    return [(a, b) for a in range(dim) for b in range(a, dim)]


# ------------------------------------------------------------------ (a) weights
def _rows(rel, pe, dim: int, power: int, wrong=None):
    """(b [S, Q], w [S]) in CSR order, fp64."""
    d = (1.0 if wrong == "sign" else -1.0) * np.asarray(rel, dtype=F32)[pe].astype(F64)
    n_e = d.shape[0]
    with np.errstate(all="ignore"):
        r2 = np.zeros(n_e)
        for a in range(dim):
            r2 = r2 + d[:, a] * d[:, a]
        w = np.ones(n_e) if power == 0 else (1.0 / np.sqrt(r2) if power == 1 else 1.0 / r2)
    b = np.zeros((n_e, q_of(dim)))
    b[:, :dim] = d
    for j, (a, c) in enumerate(pairs(dim)):
        t = d[:, a] * d[:, c]
        b[:, dim + j] = (0.5 * t if wrong != "diagonal-factor" else t) if a == c else t
    return b, w


def factor(off, perm, rel, dim: int, power: int, wrong=None):
    """The per-node part of (a): (L [n, Q, Q] lower, inv [n, Q], sc [n, Q], pivots [n, Q], degenerate bool [n], b, w)."""
    off = np.asarray(off, dtype=np.int64)
    n, n_e, Q = off.size - 1, (int(off[-1]) if off.size else 0), q_of(dim)
    pe = np.arange(n_e) if perm is None else np.asarray(perm, dtype=np.int64)
    b, w = _rows(rel, pe, dim, power, wrong)
    deg = np.diff(off)
    m = np.zeros((n, Q, Q))
    bad = deg < Q
    node = np.repeat(np.arange(n), deg)
    np.logical_or.at(bad, node, ~(w <= np.finfo(F64).max))
    with np.errstate(all="ignore"):
        for s in range(int(deg.max()) if n else 0):
            nodes = np.nonzero(deg > s)[0]
            e = off[nodes] + s
            for i in range(Q):
                wb = w[e] * b[e, i]
                for j in range(i + 1):
                    m[nodes, i, j] += wb * b[e, j]
        sc = np.stack([1.0 / np.sqrt(m[:, i, i]) for i in range(Q)], axis=1) if n else np.zeros((0, Q))
        for i in range(Q):
            for j in range(i + 1):
                m[:, i, j] = (m[:, i, j] * sc[:, i]) * sc[:, j]
        inv, piv = np.zeros((n, Q)), np.zeros((n, Q))
        for j in range(Q):
            s_ = m[:, j, j].copy()
            for k in range(j):
                s_ = s_ - m[:, j, k] * m[:, j, k]
            piv[:, j] = s_
            bad = bad | ~(s_ > 1e-12)
            root = np.sqrt(s_)
            m[:, j, j] = root
            inv[:, j] = 1.0 / root
            for i in range(j + 1, Q):
                r = m[:, i, j].copy()
                for k in range(j):
                    r = r - m[:, i, k] * m[:, j, k]
                m[:, i, j] = r * inv[:, j]
    return m, inv, sc, piv, bad, b, w


def weights(off, perm, src32, rel, dim: int, power: int, wrong: Optional[str] = None):
    """(c64 [S, Q] fp64, c [S, Q] fp32 = its rounding, src int32 [S], degenerate uint8 [n]) in CSR order."""
    assert wrong is None or wrong in WRONG_WEIGHTS, wrong
    off = np.asarray(off, dtype=np.int64)
    n, n_e, Q = off.size - 1, (int(off[-1]) if off.size else 0), q_of(dim)
    L, inv, sc, _, bad, b, w = factor(off, perm, rel, dim, power, wrong)
    node = np.repeat(np.arange(n), np.diff(off))
    y = np.zeros((n_e, Q))
    with np.errstate(all="ignore"):
        for i in range(Q):
            s_ = b[:, i] * sc[node, i]
            for k in range(i):
                s_ = s_ - L[node, i, k] * y[:, k]
            y[:, i] = s_ * inv[node, i]
        for i in range(Q - 1, -1, -1):
            s_ = y[:, i].copy()
            for k in range(i + 1, Q):
                s_ = s_ - L[node, k, i] * y[:, k]
            y[:, i] = s_ * inv[node, i]
        c64 = np.stack([(w * sc[node, i]) * y[:, i] for i in range(Q)], axis=1) if n_e else np.zeros((0, Q))
    c64[bad[node]] = 0.0
    pe = np.arange(n_e) if (perm is None or wrong == "src-unpermuted") else np.asarray(perm, dtype=np.int64)
    return c64, c64.astype(F32), np.asarray(src32, dtype=I32)[pe], bad.astype(np.uint8)


def min_pivot(off, perm, rel, dim: int, power: int) -> np.ndarray:
    """[n]: the smallest pivot of the scaled normal matrix (nan where it is no number; −inf below Q entries)."""
    piv, deg = factor(off, perm, rel, dim, power)[3], np.diff(np.asarray(off, dtype=np.int64))
    with np.errstate(all="ignore"):
        out = np.where(np.isnan(piv).any(1), np.nan, piv.min(1)) if piv.size else np.zeros(0)
    out[deg < q_of(dim)] = -np.inf
    return out


def lstsq_weights(off, perm, rel, dim: int, power: int):
    """(b): (c [S, Q] by numpy.linalg.lstsq per node, cond [n]: the 2-norm condition number of the node's unit-column-scaled weighted
    design matrix, squared — that of the scaled normal matrix).  Rows of nodes with fewer than Q entries or a weight that is not
    finite stay 0 (cond inf)."""
    off = np.asarray(off, dtype=np.int64)
    n, n_e, Q = off.size - 1, int(off[-1]), q_of(dim)
    pe = np.arange(n_e) if perm is None else np.asarray(perm, dtype=np.int64)
    b, w = _rows(rel, pe, dim, power)
    out, cond = np.zeros((n_e, Q)), np.full(n, np.inf)
    for i in range(n):
        e = slice(off[i], off[i + 1])
        if off[i + 1] - off[i] < Q or not np.isfinite(w[e]).all():
            continue
        sw = np.sqrt(w[e])
        a = sw[:, None] * b[e]
        norms = np.sqrt((a * a).sum(0))
        if not (norms > 0).all():
            continue
        sv = np.linalg.svd(a / norms, compute_uv=False)
        cond[i] = (sv[0] / sv[-1]) ** 2 if sv[-1] > 0 else np.inf
        # (solved in the unit-column coordinates, whose condition number `cond` is: the columns d and d d differ by a factor h)
        out[e] = (np.linalg.lstsq(a / norms, np.diag(sw), rcond=None)[0] / norms[:, None]).T          # [Q, deg]: jet = sol @ (x_j − x_i)
    return out, cond


# ------------------------------------------------------------------ meshes
PLANTED_2D = ("isolated", "short", "collinear", "zero-length")
PLANTED_3D = PLANTED_2D + ("coplanar",)
PIVOT_FLOOR = 1e-4


def stencil_mesh(n: int, dim: int, k: Optional[int] = None, kind: str = "cloud", seed: int = 0, plant: bool = True) -> R.Mesh:
    """A stencil of the k nearest other nodes (default 12 in 2-D, 20 in 3-D) over a uniform-random cloud or a jittered lattice, as a
    `gradient_ref.Mesh` (row = senders, col = receivers, rel = receiver − sender in fp32), with planted nodes when n allows it: an
    isolated node (no entry), a node with Q − 1 entries, a collinear stencil, a coplanar one (3-D), a zero-length vector.  Asserts
    that every unplanted node's smallest scaled pivot is >= 1e-4 under every power — and the zero-length node's under power 0, where
    that entry has weight 1 and a zero row — so that no node sits near the 1e-12 threshold."""
    Q = q_of(dim)
    k = SUGGESTED_K[dim] if k is None else k
    rng = np.random.default_rng(1000 * n + 10 * dim + seed + (500 if kind == "lattice" else 0))
    if kind == "cloud":
        pos = rng.random((n, dim))
    else:
        m = int(np.ceil(n ** (1.0 / dim)))
        grid = np.stack(np.meshgrid(*[np.arange(m)] * dim, indexing="ij"), -1).reshape(-1, dim)[:n].astype(F64)
        pos = (grid + 0.5 + 0.3 * (rng.random((n, dim)) - 0.5)) / m
    if n <= k:
        lists = [[] for _ in range(n)]          # (too few nodes for a stencil: every node is isolated)
        return R.Mesh(pos, *R._edges(pos, lists), {i: "isolated" for i in range(n)})
    order = nearest(pos, k)
    kinds = (PLANTED_2D if dim == 2 else PLANTED_3D) if (plant and n >= 40) else ()
    planted = {int(node): kinds[j % len(kinds)] for j, node in enumerate(rng.choice(n, size=2 * len(kinds), replace=False))} if kinds else {}
    lists = []
    for i in range(n):
        kind_i = planted.get(i)
        lists.append(list(order[i, :{"isolated": 0, "short": Q - 1}.get(kind_i, k)]))
    row, col, rel = R._edges(pos, lists)
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum([len(v) for v in lists])
    for node, kind_i in planted.items():
        e = slice(off[node], off[node + 1])
        if kind_i == "collinear":
            steps = np.arange(1, k + 1) * np.where(np.arange(k) % 2, -1.0, 1.0)
            rel[e] = np.outer(steps, np.linspace(0.25, 0.5, dim) / k).astype(F32)
        elif kind_i == "coplanar":
            rel[e, 2] = 0.0          # (the plane z = 0 exactly: a rounded oblique plane would not be one)
        elif kind_i == "zero-length":
            rel[off[node] + 2] = 0.0
    mesh = R.Mesh(pos, row, col, rel, planted)
    for power in (0, 1, 2):
        with np.errstate(all="ignore"):
            piv = min_pivot(mesh.off, mesh.perm, mesh.rel, dim, power)
        free = np.array([i not in planted or (planted[i] == "zero-length" and power == 0) for i in range(n)])
        assert (piv[free] >= PIVOT_FLOOR).all(), f"stencil_mesh({n}, {dim}, {k}, {kind}): smallest pivot {np.nanmin(piv[free]):.2e} under power {power}"
    return mesh


# ------------------------------------------------------------------ programs
def columns(names: Sequence[str], dim: int) -> List[str]:
    out = []
    for name in names:
        if name.startswith("lap:"):
            out.append(f"lap{int(name[4:])}")
        elif name.startswith("hess:"):
            out += [f"d2{int(name[5:])}/d{AXES[a]}{AXES[b]}" for a, b in pairs(dim)]
        else:
            out += R.columns((name,), dim)
    return out


def program(names: Sequence[str], dim: int, nf: int, velocity=None, field_scale=None):
    """[[(field, derivative, coef fp32), ...] per column]."""
    sc = np.ones(nf, F32) if field_scale is None else np.asarray(field_scale, dtype=F32)
    prog = []
    for name in names:
        if name.startswith("lap:"):
            f = int(name[4:])
            prog.append([(f, dim + pairs(dim).index((a, a)), F32(sc[f])) for a in range(dim)])
        elif name.startswith("hess:"):
            f = int(name[5:])
            prog += [[(f, dim + q, F32(sc[f]))] for q in range(len(pairs(dim)))]
        else:
            prog += R.program((name,), dim, nf, velocity, field_scale)
    return prog


# ------------------------------------------------------------------ (c) per call
def derived32(x, off, c, src, prog) -> np.ndarray:
    """out [n, nd] fp32, the bits the device must give: J[f][q] = 0; over the entries in CSR order diff = x[src, f] − x[i, f],
    p = c[e][q] · diff, J[f][q] += p; column = (coef₀ J₀ + coef₁ J₁) + coef₂ J₂."""
    return R.derived32(x, off, c, src, prog)


def derived64(x, off, c, src, prog) -> Tuple[np.ndarray, np.ndarray]:
    """(out [n, nd] fp64 from the fp32 c and x, Σ|terms| [n, nd])."""
    return R.derived64(x, off, c, src, prog)


def jets64(x, off, c64, src) -> np.ndarray:
    """[n, F, Q] fp64 from an fp64 table and fp64 fields (for the host tests: no fp32 anywhere)."""
    off = np.asarray(off, dtype=np.int64)
    n = off.size - 1
    node = np.repeat(np.arange(n), np.diff(off))
    x = np.asarray(x, dtype=F64)
    diff = x[np.asarray(src, dtype=np.int64)] - x[node]          # [S, F]
    out = np.zeros((n, x.shape[1], c64.shape[1]))
    np.add.at(out, node, diff[:, :, None] * np.asarray(c64, dtype=F64)[:, None, :])
    return out


def bound32(mag: np.ndarray, max_deg: int) -> np.ndarray:
    """|out32 − out64| <= (max_deg + 3) 2⁻²⁴ Σ|terms| (gradient_ref.bound32: the same sum of max_deg products and <= 3 terms)."""
    return R.bound32(mag, max_deg)


def adjoint32(gy, off, c, src, prog, nf: int, wrong: Optional[str] = None, row=None) -> np.ndarray:
    """gx [n, nf] fp32, the bits the device must give (adjoint_op_ref.adjoint32 over Q derivatives per field)."""
    return A.adjoint32(gy, off, c, src, prog, nf, wrong, row)


def adjoint64(gy, off, c, src, prog, nf: int):
    """(gx [n, nf] fp64 from the fp32 c and gy, Σ|terms| [n, nf], n_add [n, nf])."""
    return A.adjoint64(gy, off, c, src, prog, nf)


def adjoint_bound(mag, n_add, prog) -> np.ndarray:
    """|gx32 − gx64| <= (n_add + t + 1) 2⁻²⁴ Σ|terms| with t the most picks of one derivative: adjoint_op_ref's derivation gives
    γ_{n_add + t}, and m u / (1 − m u) <= (m + 1) u while m (m + 1) u <= 1, asserted here."""
    t = A.max_picks(prog)
    m = (int(n_add.max()) if n_add.size else 0) + t
    assert m * (m + 1) * U <= 1.0
    return (n_add + t + 1) * U * mag


# ------------------------------------------------------------------ (d) the residual
def residual64(jet, u, prev, dim: int, nu, dt: float, rho: float, velocity, pressure: int, wrong: Optional[str] = None):
    """(R [n, dim], C [n]) from jet [n, F, Q] (fp64) of the physical fields u [n, F] and the previous step prev [n, F]."""
    assert wrong is None or wrong in WRONG_RESIDUAL, wrong
    diag = [dim + pairs(dim).index((a, a)) for a in range(dim)]
    nu = np.asarray(nu, dtype=F64).reshape(-1)
    r = np.zeros((u.shape[0], dim))
    for a, fa in enumerate(velocity):
        t = np.zeros(u.shape[0]) if wrong == "no-time" else (u[:, fa] - prev[:, fa]) / dt
        adv = sum(u[:, fb] * jet[:, fa, b] for b, fb in enumerate(velocity))
        lap = sum(jet[:, fa, q] for q in diag)
        r[:, a] = (t + (-adv if wrong == "advection-sign" else adv) + (-1.0 if wrong == "pressure-sign" else 1.0) * jet[:, pressure, a] / rho
                   - (2.0 if wrong == "viscous-factor" else 1.0) * nu * lap)
    c = sum(jet[:, fa, a] for a, fa in enumerate(velocity))
    return r, c


# ------------------------------------------------------------------ (e) ResidualLoss
def loss_groups(dim: int, vel, p) -> List[List[str]]:
    """The names of each `MeshJet.derived` launch of one ResidualLoss call."""
    if dim == 2:
        return [[f"grad:{vel[0]}", f"grad:{vel[1]}", f"grad:{p}", f"lap:{vel[0]}", f"lap:{vel[1]}"]]
    return [[f"grad:{vel[0]}", f"grad:{vel[1]}", f"lap:{vel[0]}", f"lap:{vel[1]}"], [f"grad:{vel[2]}", f"grad:{p}", f"lap:{vel[2]}"]]


class ResidualRef:
    """ResidualLoss in fp64 on one mesh (off, c fp32 — the device's own table —, src), from fp64 inputs: `loss`; from the fp32 inputs
    with its gradient with respect to pred and how far fp32 may sit from both: `value_and_grad`.  nu: a number or [n]; counted: bool
    [n] (not degenerate, and in the mask); dirichlet: GraphLoss's boundary mask or None."""

    def __init__(self, off, c, src, max_deg, dim, nf, *, nu, dt, rho=1.0, velocity=None, pressure=None, scale=None, shift=None,
                 continuity=1.0, reference="target", weight=1.0, node_weight=1.0, lambda_d=0.0, dirichlet=None, counted=None,
                 wrong: Optional[str] = None):
        self.off, self.c, self.src, self.max_deg, self.dim, self.nf = off, np.asarray(c, dtype=F32), src, max_deg, dim, nf
        self.n = len(off) - 1
        self.nu, self.dt, self.rho = np.broadcast_to(np.asarray(nu, dtype=F64).reshape(-1), (self.n,)), float(dt), float(rho)
        self.vel = tuple(range(dim)) if velocity is None else tuple(velocity)
        self.p = pressure if pressure is not None else next(f for f in range(dim + 1) if f not in self.vel)
        self.scale = np.ones(nf, F32) if scale is None else np.asarray(scale, dtype=F32)          # (the coefficients are fp32)
        self.shift = np.zeros(nf, F32) if shift is None else np.asarray(shift, dtype=F32)
        self.continuity, self.reference, self.weight, self.node_weight = float(continuity), reference, float(weight), float(node_weight)
        self.lambda_d, self.dirichlet = float(lambda_d), dirichlet
        self.counted = np.ones(self.n, bool) if counted is None else np.asarray(counted, dtype=bool)
        self.wrong = wrong
        self.groups = [program(g, dim, nf, field_scale=self.scale) for g in loss_groups(dim, self.vel, self.p)]
        flat = [name for g in loss_groups(dim, self.vel, self.p) for name in g]
        self.where, c0 = {}, 0          # name -> its columns among all the launches' columns, in launch order
        for name in flat:
            w = dim if name.startswith("grad") else 1
            self.where[name] = slice(c0, c0 + w)
            c0 += w
        self.diag = [dim + pairs(dim).index((a, a)) for a in range(dim)]

    # -- the pieces
    def _physical(self, x):
        return x * self.scale.astype(F64) + self.shift.astype(F64)

    def _derivs(self, x, mags=False):
        outs = [A._derived64_of64(x, self.off, self.c, self.src, g, mags=mags) for g in self.groups]
        if mags:
            return np.concatenate([o[0] for o in outs], 1), np.concatenate([o[1] for o in outs], 1)
        return np.concatenate(outs, 1)

    def _residual(self, x, prev, d):
        """(R [n, dim], C [n], Σ|terms of R| [n, dim]) from the derivatives d [n, all columns]."""
        u, up = self._physical(x), self._physical(prev)
        sign = {"advection-sign": (-1.0, 1.0, 1.0), "pressure-sign": (1.0, -1.0, 1.0), "viscous-factor": (1.0, 1.0, 2.0)}.get(self.wrong, (1.0, 1.0, 1.0))
        r, mag = np.zeros((self.n, self.dim)), np.zeros((self.n, self.dim))
        for a, fa in enumerate(self.vel):
            g = d[:, self.where[f"grad:{fa}"]]
            t1 = np.zeros(self.n) if self.wrong == "no-time" else (u[:, fa] - up[:, fa]) / self.dt
            adv = sum(u[:, fb] * g[:, b] for b, fb in enumerate(self.vel))
            t3 = d[:, self.where[f"grad:{self.p}"]][:, a] / self.rho
            t4 = self.nu * d[:, self.where[f"lap:{fa}"]][:, 0]
            r[:, a] = t1 + sign[0] * adv + sign[1] * t3 - sign[2] * t4
            mag[:, a] = ((np.abs(u[:, fa]) + np.abs(up[:, fa])) / self.dt + sum(np.abs(u[:, fb] * g[:, b]) for b, fb in enumerate(self.vel))
                         + np.abs(t3) + np.abs(t4))
        c = sum(d[:, self.where[f"grad:{fa}"]][:, a] for a, fa in enumerate(self.vel))
        return r, c, mag

    def _graph_loss(self, pred, target):
        val, grad = A.graph_loss64(pred, target, self.lambda_d, self.dirichlet)
        return self.node_weight * val, self.node_weight * grad

    def loss(self, pred, target, prev) -> float:
        """The value in fp64 from fp64 inputs (so that a difference quotient of it means something)."""
        pred, target, prev = (np.asarray(v, dtype=F64) for v in (pred, target, prev))
        d = pred - target
        val = float((d * d).mean())
        if self.lambda_d > 0 and self.dirichlet is not None and self.dirichlet.any():
            val += self.lambda_d * float(np.abs(d[self.dirichlet]).mean())
        val *= self.node_weight
        r, c, _ = self._residual(pred, prev, self._derivs(pred))
        if self.reference == "target":
            r0, c0, _ = self._residual(target, prev, self._derivs(target))
            r, c = r - r0, c - c0
        cnt = max(int(self.counted.sum()), 1)
        k = self.counted.astype(F64)
        return val + self.weight * (float((r * r * k[:, None]).sum()) / (cnt * self.dim) + self.continuity * float((c * c * k).sum()) / cnt)

    def value_and_grad(self, pred, target, prev):
        """(value, how far the fp32 value may sit from it, ∂value/∂pred [n, nf], how far the fp32 gradient may sit from it), all from the
        fp32 inputs as fp64.  The allowances, u = 2⁻²⁴, per node i and component a, with T the terms of R_a —
        T1 = (U_a − U_a^prev) / dt, T2_b = U_b ∂_b U_a, T3 = ∂_a P / ρ, T4 = ν ∇²U_a:
          * U = scale x + shift is two roundings: eU = 2 u (|scale x| + |shift|);
          * a derivative q comes from the launch: eq = bound32(Σ|c||Δx| of its column) (jet_ref.bound32; x itself is exact fp32);
          * eT1 = (eU_a + eU_a^prev) / dt + 2 u |T1|-terms, eT2_b = |U_b| eq + |∂_b U_a| eU_b + u |T2_b|, eT3 = eq / ρ + u |T3|,
            eT4 = ν eq + u |T4|, and adding the dim + 3 terms one by one costs (dim + 3) u Σ|T|: eR = Σ eT + (dim + 5) u Σ|T|;
            the continuity sum: eC = Σ_a eq + dim u Σ|∂_a U_a|;
          * with reference = "target": r = R(pred) − R(target), er = eR(pred) + eR(target) + u |r| (likewise c);
          * value: r² is off by 2 |r| er + er² + u r²; the masked mean of N dim terms added in any order, its division and the weight:
            (2 (N dim + 4) + 6) u Σ r² / (count dim) — likewise the continuity's and GraphLoss's own means;
          * backward: gr = 2 w k r / (count dim) is a handful of fp32 products: egr = s er + 5 u |gr| (s the factor), egc likewise;
          * the gradient handed to the launch's columns: y(∂_b U_a) = gr_a U_b (+ gc for b = a), y(∂_a P) = gr_a / ρ, y(∇²U_a) = −ν gr_a:
            ey = |U_b| egr + |gr_a| eU_b + u |·| (+ egc + u |·|), egr / ρ + u |·|, ν egr + u |·|;
          * Dᵀ per launch: |gx32 − Dᵀ y| <= adjoint_bound on y's Σ|terms| + |Dᵀ| ey, widened by 1e-3 as at adjoint_op_ref.FlowRef.grad
            for taking Σ|terms| from the fp64 y;
          * the direct part scale_a gr_a / dt + scale_b Σ_a gr_a ∂_b U_a: |scale| (egr / dt + Σ (|∂_b U_a| egr + |gr_a| eq)) + 6 u Σ|its terms|;
          * autograd adds the parts (GraphLoss's, the direct one, one per launch): 4 u of the magnitudes added; GraphLoss's own
            gradient is 6 u of its magnitude (FlowRef.grad)."""
        assert self.wrong is None
        n, nf, dim = self.n, self.nf, self.dim
        x, t, pv = (np.asarray(v, dtype=F32).astype(F64) for v in (pred, target, prev))
        sc, sh = self.scale.astype(F64), self.shift.astype(F64)

        def parts(v):
            d, dmag = self._derivs(v, mags=True)
            eq = bound32(dmag, self.max_deg)
            r, c, tmag = self._residual(v, pv, d)
            u = self._physical(v)
            eu = 2 * U * (np.abs(v * sc) + np.abs(sh))
            eup = 2 * U * (np.abs(pv * sc) + np.abs(sh))
            er = np.zeros((n, dim))
            for a, fa in enumerate(self.vel):
                g, eg = d[:, self.where[f"grad:{fa}"]], eq[:, self.where[f"grad:{fa}"]]
                e = (eu[:, fa] + eup[:, fa]) / self.dt
                for b, fb in enumerate(self.vel):
                    e = e + np.abs(u[:, fb]) * eg[:, b] + np.abs(g[:, b]) * eu[:, fb]
                e = e + eq[:, self.where[f"grad:{self.p}"]][:, a] / self.rho + self.nu * eq[:, self.where[f"lap:{fa}"]][:, 0]
                er[:, a] = e + (dim + 5) * U * tmag[:, a]
            ec = sum(eq[:, self.where[f"grad:{fa}"]][:, a] for a, fa in enumerate(self.vel))
            ec = ec + dim * U * sum(np.abs(d[:, self.where[f"grad:{fa}"]][:, a]) for a, fa in enumerate(self.vel))
            return d, eq, u, eu, r, c, er, ec

        d, eq, u, eu, r, c, er, ec = parts(x)
        if self.reference == "target":
            _, _, _, _, r0, c0, er0, ec0 = parts(t)
            r, c = r - r0, c - c0
            er, ec = er + er0 + U * np.abs(r), ec + ec0 + U * np.abs(c)
        k = self.counted.astype(F64)
        cnt = max(int(self.counted.sum()), 1)
        base, gbase = self._graph_loss(x, t)
        sum_r, sum_c = float((r * r * k[:, None]).sum()), float((c * c * k).sum())
        value = base + self.weight * (sum_r / (cnt * dim) + self.continuity * sum_c / cnt)
        e_value = ((2 * (n * nf + 4) + 8) * U * abs(base)
                   + self.weight / (cnt * dim) * (float(((2 * np.abs(r) * er + er * er) * k[:, None]).sum()) + (2 * (n * dim + 4) + 6) * U * sum_r)
                   + self.weight * self.continuity / cnt * (float(((2 * np.abs(c) * ec + ec * ec) * k).sum()) + (2 * (n + 4) + 6) * U * sum_c)
                   + 3 * U * abs(value))
        # ---- the gradient
        s_r, s_c = 2.0 * self.weight / (cnt * dim), 2.0 * self.weight * self.continuity / cnt
        gr, gc = s_r * r * k[:, None], s_c * c * k
        egr, egc = (s_r * er + 5 * U * np.abs(gr)) * k[:, None], (s_c * ec + 5 * U * np.abs(gc)) * k
        y, ey = np.zeros_like(d), np.zeros_like(d)
        direct, edirect, dsize = np.zeros((n, nf)), np.zeros((n, nf)), np.zeros((n, nf))
        for a, fa in enumerate(self.vel):
            w_g, w_p, w_l = self.where[f"grad:{fa}"], self.where[f"grad:{self.p}"], self.where[f"lap:{fa}"]
            for b, fb in enumerate(self.vel):
                term = gr[:, a] * u[:, fb]
                y[:, w_g][:, b] += term
                ey[:, w_g][:, b] += np.abs(u[:, fb]) * egr[:, a] + np.abs(gr[:, a]) * eu[:, fb] + U * np.abs(term)
                dterm = sc[fb] * gr[:, a] * d[:, w_g][:, b]
                direct[:, fb] += dterm
                dsize[:, fb] += np.abs(dterm)
                edirect[:, fb] += abs(sc[fb]) * (np.abs(d[:, w_g][:, b]) * egr[:, a] + np.abs(gr[:, a]) * eq[:, w_g][:, b])
            y[:, w_g][:, a] += gc
            ey[:, w_g][:, a] += egc + U * (np.abs(gc) + np.abs(y[:, w_g][:, a]))
            y[:, w_p][:, a] += gr[:, a] / self.rho
            ey[:, w_p][:, a] += egr[:, a] / self.rho + U * np.abs(gr[:, a]) / self.rho
            y[:, w_l][:, 0] += -self.nu * gr[:, a]
            ey[:, w_l][:, 0] += self.nu * egr[:, a] + U * self.nu * np.abs(gr[:, a])
            dterm = sc[fa] * gr[:, a] / self.dt
            direct[:, fa] += dterm
            dsize[:, fa] += np.abs(dterm)
            edirect[:, fa] += abs(sc[fa]) * egr[:, a] / self.dt
        edirect += 6 * U * dsize
        graph_mse = A.graph_loss64(x, t, 0.0, None)[1] * self.node_weight
        size = np.abs(graph_mse) + np.abs(gbase - graph_mse)
        total, allowed = gbase + direct, 6 * U * size + edirect
        size = size + dsize
        c0 = 0
        for prog in self.groups:
            nd = len(prog)
            gx, mag, n_add = A._adjoint64_of64(y[:, c0:c0 + nd], self.off, self.c, self.src, prog, nf)
            allowed += (adjoint_bound(mag, n_add, prog) + A.abs_adjoint(ey[:, c0:c0 + nd], self.off, self.c, self.src, prog, nf)) * (1 + 1e-3)
            total += gx
            size += np.abs(gx)
            c0 += nd
        return value, e_value, total, allowed + 4 * U * size
