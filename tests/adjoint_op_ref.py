"""Test-only numpy restatement of g4c_mesh_derived_adjoint (csrc/mesh_gradient.hip), the transpose of the per-step launch that
tests/gradient_ref.py restates, and of what `FlowLoss` (nn/losses.py) makes of it.  Nothing here calls graphs4cfd_amd.

With G_i[f][a] = Σ_{e in in(i)} g[e][a] (x[src_e, f] − x[i, f]) and cur[i, c] = Σ_k coef[c][k] G_i[row(c, k)], for gy [n, nd]:
    H_i[f][a] = Σ_{(c, k): row(c, k) = (f, a)} coef[c][k] gy[i, c]
    gx[j, f]  = Σ_{e: src_e = j} Σ_a g[e][a] H_{dst_e}[f][a] − Σ_{e in in(j)} Σ_a g[e][a] H_j[f][a]

(a) `adjoint32`: a numpy.float32 loop in the stated order (include/g4c.h): H from +0, its terms added in program order; acc[f] = +0;
    over j's out-edges in ascending CSR position, for a = 0 .. dim − 1, acc[f] += g[e][a] · H_{dst_e}[f][a]; then over j's own in-edges
    in CSR order, for a, acc[f] −= g[e][a] · H_j[f][a].  Every product is rounded before it is added.  (The loop runs over the
    out-edge rank r = 0, 1, ... and the in-edge slot s and is vectorised over the nodes: every node still adds its own terms one at a
    time, in order.)  Every column of gx is written; a field the program does not name is +0.
(b) `adjoint64`: the same in fp64 from the fp32 g and gy, and Σ|terms| = Σ_e Σ_a |g[e][a]| Σ_k |coef_k| |gy[., c_k]| per output.
(c) `bound`: |gx32 − gx64| <= (n_add + 3) 2⁻²⁴ Σ|terms|, n_add = dim (outdeg_j + indeg_j) the fp32 additions into that output.
    Derivation, u = 2⁻²⁴, γ_m = m u / (1 − m u): a term is T = g · H, H = Σ_{k <= t} c_k y_k.  H's t products are rounded (u each) and
    added from +0 (the first addition is exact: t − 1 roundings), so |fl(H) − H| <= γ_t Σ|c_k y_k|; the product with g is rounded:
    |fl(T) − T| <= γ_{t+1} |g| Σ|c_k y_k|.  The n_add terms are added one at a time from +0 (the first exact), so a term passes through
    at most n_add − 1 more roundings: |gx32 − gx| <= γ_{n_add + t} Σ|terms|.  With t <= 2 picks per derivative and
    (n_add + 2)(n_add + 3) u <= 1 (n_add <= 4000) that is <= (n_add + 3) u Σ|terms|; `bound` asserts both conditions.  The fp64
    restatement's own error (2⁻⁵³ relative per operation) is nine orders below.
(d) `wrong=` names ONE deliberate mistake for the negative controls: "no-diagonal" (the second sum forgotten), "untransposed" (node j
    walks its IN-edges, reading H at their senders, where its out-edges belong), "sender-order" (the sender-side grouping built from
    the senders in the CALLER's edge order, its entries then used as CSR positions: needs `row`, the caller's senders).

`FlowRef`: FlowLoss's value in fp64, its gradient with respect to pred, and how far the device's fp32 gradient may sit from it
(derived at `FlowRef.grad`)."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

import gradient_ref as R

F32, F64, I32 = np.float32, np.float64, np.int32
U = 2.0 ** -24
WRONG = ("no-diagonal", "untransposed", "sender-order")


# ------------------------------------------------------------------ tables
def dst_of(off) -> np.ndarray:
    """[E] int32: the receiver of CSR position e."""
    off = np.asarray(off, dtype=np.int64)
    return np.repeat(np.arange(off.size - 1), np.diff(off)).astype(I32)


def sender_csr(src, n: int) -> Tuple[np.ndarray, np.ndarray]:
    """(out_off int32 [n + 1], out_perm int32 [E]): the positions of `src` grouped by sender, ascending within a sender (stable)."""
    src = np.asarray(src, dtype=np.int64)
    out_perm = np.argsort(src, kind="stable").astype(I32)
    out_off = np.zeros(n + 1, dtype=I32)
    if n:
        out_off[1:] = np.cumsum(np.bincount(src, minlength=n))[:n]
    return out_off, out_perm


def hub_mesh(n: int = 600, dim: int = 2, seed: int = 0) -> R.Mesh:
    """Every node's FIRST in-edge comes from node 0 (out-degree n − 1), then its five nearest neighbours — so the edge 0 -> i is there
    twice wherever node 0 is among those (duplicated edges), and node 0 itself has its five neighbours only."""
    rng = np.random.default_rng(1000 * n + dim + seed)
    pos = rng.random((n, dim))
    nbr = R.nearest(pos, 5)
    lists = [list(nbr[0])] + [[0] + list(nbr[i]) for i in range(1, n)]
    return R.Mesh(pos, *R._edges(pos, lists))


def lattice_tables(n: int, w: int, dim: int, rng) -> Tuple[np.ndarray, np.ndarray, np.ndarray, int]:
    """(off, g, src, max_deg) of a lattice given by its tables alone: node i receives from i ± 1 and i ± w (those inside 0 .. n − 1),
    random weights — for sizes a brute-force neighbour search cannot reach."""
    i = np.arange(n, dtype=np.int64)
    cand = np.stack([i - w, i - 1, i + 1, i + w], axis=1)
    ok = (cand >= 0) & (cand < n)
    deg = ok.sum(1)
    off = np.zeros(n + 1, dtype=I32)
    off[1:] = np.cumsum(deg)
    src = cand[ok].astype(I32)
    g = rng.standard_normal((src.size, dim)).astype(F32)
    return off, g, src, 4


# ------------------------------------------------------------------ (a), (b)
def fields_of(prog) -> List[int]:
    """The distinct fields of a program in the order of their first appearance (the library's list)."""
    out = []
    for col in prog:
        for (f, _, _) in col:
            if f not in out:
                out.append(f)
    return out


def max_picks(prog) -> int:
    picks: Dict[Tuple[int, int], int] = {}
    for col in prog:
        for (f, a, _) in col:
            picks[(f, a)] = picks.get((f, a), 0) + 1
    return max(picks.values())


def _rows(gy, prog, fields, dim, dtype):
    """{f: H [n, dim]} and {f: |H| [n, dim]} (Σ|coef| |gy|, fp64): every entry from +0, its terms added in program order."""
    n = gy.shape[0]
    H = {f: np.zeros((n, dim), dtype) for f in fields}
    A = {f: np.zeros((n, dim), F64) for f in fields}
    yy = np.asarray(gy).astype(dtype)
    for c, col in enumerate(prog):
        for (f, a, coef) in col:
            pr = dtype(coef) * yy[:, c]
            H[f][:, a] += pr
            A[f][:, a] += abs(float(coef)) * np.abs(yy[:, c].astype(F64))
    return H, A


def _adjoint(gy, off, g, src, prog, nf, dtype, wrong=None, row=None):
    assert wrong is None or wrong in WRONG, wrong
    off = np.asarray(off, dtype=np.int64)
    n, dim = off.size - 1, g.shape[1]
    src = np.asarray(src, dtype=np.int64)
    fields = fields_of(prog)
    H, A = _rows(np.asarray(gy, dtype=F32), prog, fields, dim, dtype)
    gg = np.asarray(g, dtype=F32).astype(dtype)
    ga = np.abs(np.asarray(g, dtype=F32).astype(F64))
    gx, mag, n_add = np.zeros((n, nf), dtype), np.zeros((n, nf), F64), np.zeros((n, nf), np.int64)
    deg = np.diff(off)
    if wrong == "untransposed":
        out_off, out_perm, far = off, np.arange(src.size), src
    else:
        out_off, out_perm = sender_csr(src if wrong != "sender-order" else np.asarray(row, dtype=np.int64), n)
        out_off, out_perm, far = out_off.astype(np.int64), out_perm.astype(np.int64), dst_of(off).astype(np.int64)
    odeg = np.diff(out_off)
    for r in range(int(odeg.max()) if n and src.size else 0):          # the r-th edge of every node that sends (reads, if untransposed) one
        nodes = np.nonzero(odeg > r)[0]
        e = out_perm[out_off[nodes] + r]
        i = far[e]
        for f in fields:
            for a in range(dim):
                p = gg[e, a] * H[f][i, a]
                gx[nodes, f] += p
                mag[nodes, f] += ga[e, a] * A[f][i, a]
                n_add[nodes, f] += 1
    if wrong != "no-diagonal":
        for s in range(int(deg.max()) if n and src.size else 0):
            nodes = np.nonzero(deg > s)[0]
            e = off[nodes] + s
            for f in fields:
                for a in range(dim):
                    p = gg[e, a] * H[f][nodes, a]
                    gx[nodes, f] -= p
                    mag[nodes, f] += ga[e, a] * A[f][nodes, a]
                    n_add[nodes, f] += 1
    return gx, mag, n_add


def adjoint32(gy, off, g, src, prog, nf: int, wrong: Optional[str] = None, row=None) -> np.ndarray:
    """(a): gx [n, nf] fp32, the bits the device must give."""
    return _adjoint(gy, off, g, src, prog, nf, F32, wrong, row)[0]


def adjoint64(gy, off, g, src, prog, nf: int, wrong: Optional[str] = None, row=None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(b): (gx [n, nf] fp64 from the fp32 g and gy, Σ|terms| [n, nf], n_add [n, nf])."""
    return _adjoint(gy, off, g, src, prog, nf, F64, wrong, row)


def bound(mag: np.ndarray, n_add: np.ndarray, prog) -> np.ndarray:
    """(c): |gx32 − gx64| <= (n_add + 3) 2⁻²⁴ Σ|terms| (the docstring above derives it, under the two conditions asserted here)."""
    assert max_picks(prog) <= 2 and (n_add.max() if n_add.size else 0) <= 4000
    return (n_add + 3) * U * mag


# ------------------------------------------------------------------ FlowLoss
def abs_derived(v, off, g, src, prog) -> np.ndarray:
    """|D| v for v >= 0 [n, nf]: Σ_k |coef_k| Σ_e |g[e][a]| (v[src_e, f] + v[i, f]) — how far D x moves when x moves by at most v."""
    off = np.asarray(off, dtype=np.int64)
    n = off.size - 1
    node = np.repeat(np.arange(n), np.diff(off))
    ga = np.abs(np.asarray(g, dtype=F32).astype(F64))
    out = np.zeros((n, len(prog)))
    for c, col in enumerate(prog):
        for (f, a, coef) in col:
            np.add.at(out[:, c], node, abs(float(coef)) * ga[:, a] * (v[np.asarray(src, dtype=np.int64), f] + v[node, f]))
    return out


def abs_adjoint(v, off, g, src, prog, nf: int) -> np.ndarray:
    """|Dᵀ| v for v >= 0 [n, nd]: every term of the adjoint with |g|, |coef| and a plus sign."""
    off = np.asarray(off, dtype=np.int64)
    n, dim = off.size - 1, g.shape[1]
    src = np.asarray(src, dtype=np.int64)
    node = np.repeat(np.arange(n), np.diff(off))
    ga = np.abs(np.asarray(g, dtype=F32).astype(F64))
    out = np.zeros((n, nf))
    for c, col in enumerate(prog):
        for (f, a, coef) in col:
            t = abs(float(coef)) * ga[:, a] * v[node, c]          # the term of edge e, read at its receiver
            np.add.at(out[:, f], src, t)
            np.add.at(out[:, f], node, t)
    return out


def graph_loss64(pred, target, lambda_d: float, mask) -> Tuple[float, np.ndarray]:
    """GraphLoss in fp64 from the fp32 inputs: (value, its gradient with respect to pred)."""
    p, t = np.asarray(pred, dtype=F32).astype(F64), np.asarray(target, dtype=F32).astype(F64)
    d = p - t
    val, grad = float((d * d).mean()), 2.0 * d / d.size
    if lambda_d > 0 and mask is not None and mask.any():
        dm = d[mask]
        val += lambda_d * float(np.abs(dm).mean())
        grad[mask] += lambda_d * np.sign(dm) / dm.size
    return val, grad


class FlowRef:
    """FlowLoss in fp64 on one mesh: `groups` is [(prog, [(w, c0, c1) per name], on_pred)] — one entry per differentiable `derived`
    call: its program, per name its weight and columns, and whether it reads pred (names in `zero`) or pred − target."""

    def __init__(self, off, g, src, max_deg, groups, lambda_d=0.0, mask=None):
        self.off, self.g, self.src, self.max_deg, self.groups, self.lambda_d, self.mask = off, g, src, max_deg, groups, lambda_d, mask

    def _scale(self, n, parts, nd):
        s = np.zeros(nd)
        for (w, c0, c1) in parts:
            s[c0:c1] = w / (n * (c1 - c0))
        return s

    def loss(self, pred, target) -> float:
        """The value in fp64, from fp64 inputs (so that a difference quotient of it means something)."""
        p, t = np.asarray(pred, dtype=F64), np.asarray(target, dtype=F64)
        d = p - t
        val = float((d * d).mean())
        if self.lambda_d > 0 and self.mask is not None and self.mask.any():
            val += self.lambda_d * float(np.abs(d[self.mask]).mean())
        n = p.shape[0]
        for prog, parts, on_pred in self.groups:
            q = _derived64_of64(p if on_pred else d, self.off, self.g, self.src, prog)
            val += float((self._scale(n, parts, len(prog))[None, :] * q * q).sum())
        return val

    def grad(self, pred, target) -> Tuple[np.ndarray, np.ndarray]:
        """(∂loss/∂pred in fp64 from the fp32 inputs = ∂GraphLoss + Σ (2 w / (N nd_name)) Dᵀ D (pred − ref), how far the device's fp32
        gradient may sit from it).

        The allowance, u = 2⁻²⁴, per `derived` call with x = pred − ref, q = D x, y = 2 s q (s = w / (N nd_name) per column), Dᵀ y:
          * x: pred − target is rounded once, |x32 − x| <= u |x| (pred itself: 0);
          * q: |q32 − q| <= bound32(Σ|terms| of q) + |D| (u |x|)                                   — the forward's bound carried along;
          * y: the square's backward, the mean's and the weight are four fp32 products: |y32 − y| <= 2 s |q32 − q| + 5 u |y|;
          * Dᵀ: |gx32 − Dᵀ y| <= bound (c) on y32's Σ|terms| + |Dᵀ| |y32 − y|;
          * the two Σ|terms| are taken from the fp64 x and y: those of x32 and y32 exceed them by |D| |x32 − x| and |Dᵀ| |y32 − y| at most,
            times (deg + 3) u < 1e-3 — both sums are widened by 1e-3 for it;
        and the sum of GraphLoss's own gradient (a handful of fp32 products: 6 u of its magnitude) and the calls' gradients by autograd
        (one rounding per addition: 3 u of the magnitudes added)."""
        n, nf = np.shape(pred)
        base = graph_loss64(pred, target, self.lambda_d, self.mask)[1]
        mse = graph_loss64(pred, target, 0.0, None)[1]
        p, t = np.asarray(pred, dtype=F32).astype(F64), np.asarray(target, dtype=F32).astype(F64)
        size = np.abs(mse) + np.abs(base - mse)          # the MSE's and the Dirichlet term's parts, which may cancel
        total, allowed = base.copy(), 6 * U * size
        for prog, parts, on_pred in self.groups:
            x = p if on_pred else p - t
            ex = np.zeros_like(x) if on_pred else U * np.abs(x)
            q, qmag = _derived64_of64(x, self.off, self.g, self.src, prog, mags=True)
            eq = (R.bound32(qmag, self.max_deg) + abs_derived(ex, self.off, self.g, self.src, prog)) * (1 + 1e-3)
            s2 = 2.0 * self._scale(n, parts, len(prog))[None, :]
            y = s2 * q
            ey = s2 * eq + 5 * U * np.abs(y)
            gx, mag, n_add = _adjoint64_of64(y, self.off, self.g, self.src, prog, nf)
            egx = ((n_add + 3) * U * mag + abs_adjoint(ey, self.off, self.g, self.src, prog, nf)) * (1 + 1e-3)
            total += gx
            allowed += egx
            size += np.abs(gx)
        return total, allowed + 3 * U * size


def _derived64_of64(x, off, g, src, prog, mags=False):
    """gradient_ref.derived64 on an fp64 x (that one rounds x to fp32 first)."""
    fields = sorted({f for col in prog for (f, _, _) in col})
    G, A = _gradients64(x, off, g, src, fields)
    cur, mag = R._combine(G, A, prog, len(off) - 1, F64)
    return (cur, mag) if mags else cur


def _gradients64(x, off, g, src, fields):
    off = np.asarray(off, dtype=np.int64)
    n, dim = off.size - 1, g.shape[1]
    gg = np.asarray(g, dtype=F32).astype(F64)
    node = np.repeat(np.arange(n), np.diff(off))
    src = np.asarray(src, dtype=np.int64)
    G = {f: np.zeros((n, dim)) for f in fields}
    A = {f: np.zeros((n, dim)) for f in fields}
    for f in fields:
        diff = x[src, f] - x[node, f]
        for a in range(dim):
            np.add.at(G[f][:, a], node, gg[:, a] * diff)
            np.add.at(A[f][:, a], node, np.abs(gg[:, a]) * np.abs(diff))
    return G, A


def _adjoint64_of64(y, off, g, src, prog, nf):
    """`adjoint64` on an fp64 gy (that one rounds gy to fp32 first): (gx, Σ|terms|, n_add)."""
    off = np.asarray(off, dtype=np.int64)
    n, dim = off.size - 1, g.shape[1]
    src = np.asarray(src, dtype=np.int64)
    node = np.repeat(np.arange(n), np.diff(off))
    gg = np.asarray(g, dtype=F32).astype(F64)
    gx, mag = np.zeros((n, nf)), np.zeros((n, nf))
    for c, col in enumerate(prog):
        for (f, a, coef) in col:
            t = float(coef) * gg[:, a] * y[node, c]
            np.add.at(gx[:, f], src, t)
            np.add.at(gx[:, f], node, -t)
            np.add.at(mag[:, f], src, np.abs(t))
            np.add.at(mag[:, f], node, np.abs(t))
    n_add = np.zeros((n, nf), np.int64)
    cnt = dim * (np.bincount(src, minlength=n)[:n] + np.diff(off)) if n else np.zeros(0, np.int64)
    for f in fields_of(prog):
        n_add[:, f] = cnt
    return gx, mag, n_add
