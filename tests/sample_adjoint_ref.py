"""Test-only numpy restatement of g4c_sample_points_adjoint (csrc/point_sample.hip) and of gfd.nn.SampleLoss: the node-side table of
a j-major [k, P] neighbour table (a stable argsort of the flattened idx), the adjoint as a numpy.float32 loop in the contract's order
and in fp64 with its bound, the deliberate mistakes the tests must reject, the inputs the GPU tests launch on (so that the host test
can check the loop against the bound on the very same data), and SampleLoss in fp64 with the allowance of its gradient.  numpy only;
the forward is tests/sampler_ref.py's (idx [P, k] there, j-major [k, P] here)."""
from typing import Optional, Tuple

import numpy as np

import sampler_ref as SR

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
WRONG = ("dropped-slot", "quotient", "table-order-coef", "shifted-list")


# ------------------------------------------------------------------ the node-side table
def node_tables(idx_jm, coef_jm, n_nodes: int, wrong: Optional[str] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(in_off int32 [N + 1], in_pt int32 [k P], in_coef [k P]) of the j-major tables idx, coef [k, P]: the entries grouped by the node
    they name, ascending flat position j·P + p within a node; in_pt = position mod P, in_coef the coefficients in that order.
    `wrong`: one of WRONG — the same with one mistake."""
    idx_jm, coef_jm = np.asarray(idx_jm), np.asarray(coef_jm)
    k, n_points = idx_jm.shape
    flat = idx_jm.reshape(-1).astype(np.int64)
    pos = np.arange(flat.size, dtype=np.int64)
    if wrong == "dropped-slot":          # the last slot never reaches its nodes
        pos = pos[: (k - 1) * n_points]
    perm = pos[np.argsort(flat[pos], kind="stable")]
    off = np.zeros(n_nodes + 1, np.int64)
    np.cumsum(np.bincount(flat[pos], minlength=n_nodes), out=off[1:])
    in_pt = perm // n_points if wrong == "quotient" else perm % max(n_points, 1)          # (the quotient is the slot j, not the point)
    in_coef = coef_jm.reshape(-1)[pos] if wrong == "table-order-coef" else coef_jm.reshape(-1)[perm]          # (coefficients not regrouped)
    if wrong == "shifted-list":          # node i walks the list of node i − 1
        off = np.concatenate([[0], off[:-1]])
    return off.astype(np.int32), in_pt.astype(np.int32), np.ascontiguousarray(in_coef)


def _walk(gy, in_off, in_pt, in_coef, dtype):
    """(acc, Σ|terms|, list lengths): acc[f] = +0, then acc[f] = acc[f] + (in_coef[q] · gy[in_pt[q], f]) for q ascending over list(i),
    every product and every sum rounded to `dtype` — the s-th entry of every list at once."""
    gy, in_coef = np.asarray(gy).astype(dtype), np.asarray(in_coef).astype(dtype)
    in_off = np.asarray(in_off).astype(np.int64)
    n = in_off.size - 1
    acc = np.zeros((n, gy.shape[1]), dtype)
    mag = np.zeros((n, gy.shape[1]), F64)
    length = np.diff(in_off)
    for s in range(int(length.max()) if n else 0):
        nodes = np.nonzero(length > s)[0]
        q = in_off[nodes] + s
        pr = (in_coef[q, None] * gy[in_pt[q]]).astype(dtype)
        acc[nodes] = (acc[nodes] + pr).astype(dtype)
        mag[nodes] += np.abs(pr.astype(F64))
    return acc, mag, length


def adjoint32(gy, in_off, in_pt, in_coef) -> np.ndarray:
    """gx float32 [N, F]: the contract's loop in numpy.float32."""
    return _walk(gy, in_off, in_pt, in_coef, F32)[0]


def adjoint64(gy, in_off, in_pt, in_coef) -> Tuple[np.ndarray, np.ndarray]:
    """(gx in fp64 from the values as given, the bound (n_i + 1) 2^-24 Σ_q |in_coef[q] · gy[in_pt[q], f]| on the fp32 loop's distance
    from it: one rounding per product and one per addition, n_i the list's length)."""
    gx, mag, length = _walk(gy, in_off, in_pt, in_coef, F64)
    return gx, (length[:, None] + 1) * U * mag


def abs_adjoint(v, in_off, in_pt, in_coef) -> np.ndarray:
    """|Sᵀ| v for v >= 0: how far an error of v in gy reaches."""
    return _walk(np.abs(v), in_off, in_pt, np.abs(np.asarray(in_coef, F64)), F64)[0]


# ------------------------------------------------------------------ the inputs of the GPU tests
LIST_LENGTHS = (0, 1, 3, 4, 5, 9)          # around the unroll of four; node 0 is the node nobody uses


def synthetic(n_nodes: int, k: int, n_points: int, seed: int = 0):
    """(idx int32 [k, P], coef float32 [k, P]) of no search: nodes 0 .. 5 are named by exactly LIST_LENGTHS entries, node 6 by none
    either, the other entries name random nodes from 7 on, at random table positions; random coefficients.  (The launch trusts its
    tables: they need not be a fit.)"""
    rng = np.random.default_rng(100 * n_nodes + 10 * k + n_points + seed)
    total = k * n_points
    head = np.repeat(np.arange(len(LIST_LENGTHS)), LIST_LENGTHS)
    assert total >= head.size and n_nodes > 8
    flat = np.concatenate([head, rng.integers(7, n_nodes, total - head.size)])
    rng.shuffle(flat)
    return np.ascontiguousarray(flat.reshape(k, n_points).astype(np.int32)), rng.standard_normal((k, n_points)).astype(F32)


def hub(dim: int = 2, n_nodes: int = 400, near: int = 600, far: int = 57, k: int = 6):
    """(pos, points, idx [k, P], coef [k, P]) of a real fit: `near` points within a small fraction of the node spacing of ONE node of a
    random cloud (its list is longer than a workgroup of 256) and `far` points anywhere."""
    pos = SR.cloud(n_nodes, dim)
    rng = np.random.default_rng(5 + dim)
    spacing = n_nodes ** (-1.0 / dim)
    pts = np.concatenate([pos[17][None, :] + (rng.random((near, dim)) - 0.5) * 0.05 * spacing, SR.queries(far, dim)]).astype(F32)
    idx = SR.nearest(pos, pts, k)
    c32 = SR.coefficients(pos, pts, idx, 2)[1]
    return pos, pts, np.ascontiguousarray(idx.T), np.ascontiguousarray(c32.T)


BIG = (90_000, 9)          # N · ceil(F / 4) = 270 000 > 262 144 = 1024 workgroups of 256: the grid-stride loop runs


def cases():
    """name -> (idx [k, P], coef [k, P], n_nodes, F list): every table the GPU test launches on."""
    out = {}
    for k in (1, 6, 16):
        out[f"synthetic k={k}"] = synthetic(300, k, 257) + (300, (1, 3, 4, 5, 9))
    for dim in (2, 3):
        out[f"hub {dim}-D"] = hub(dim)[2:] + (400, (3,))
    out["big"] = synthetic(BIG[0], 6, 20_000) + (BIG[0], (BIG[1],))
    return out


def gy_of(n_points: int, nf: int, seed: int = 0) -> np.ndarray:
    return np.random.default_rng(1000 * n_points + 10 * nf + seed).standard_normal((n_points, nf)).astype(F32)


# ------------------------------------------------------------------ SampleLoss in fp64
class SampleRef:
    """gfd.nn.SampleLoss in fp64 over the tables idx, coef [k, P] (the device's own, for a batch the merged ones) of n_nodes nodes:
    node_weight · GraphLoss + weight · Σ mask (S pred − ref)² / (P_kept F')."""

    def __init__(self, idx_jm, coef_jm, n_nodes, weight=1.0, node_weight=1.0, lambda_d=0.0, dirichlet=None, fields=None, keep=None):
        self.idx, self.c = np.asarray(idx_jm).T, np.asarray(coef_jm, F32).T          # [P, k], tests/sampler_ref.py's layout
        self.k = self.idx.shape[1]
        self.tables = node_tables(idx_jm, coef_jm, n_nodes)
        self.weight, self.node_weight, self.lambda_d, self.dirichlet, self.fields = weight, node_weight, lambda_d, dirichlet, fields
        n_points = self.idx.shape[0]
        self.keep = np.ones(n_points, bool) if keep is None else np.asarray(keep, bool)

    def _cols(self, nf):
        return list(range(nf)) if self.fields is None else list(self.fields)

    def _base64(self, p, t):
        d = p - t
        val = float((d * d).mean())
        if self.lambda_d > 0 and self.dirichlet is not None and self.dirichlet.any():
            val += self.lambda_d * float(np.abs(d[self.dirichlet]).mean())
        return val

    def loss(self, pred, target, obs=None) -> float:
        """The value in fp64 from fp64 inputs (a difference quotient of it means something).  `obs` [P, F']: the observations of the
        step; None: ref = S target."""
        p, t = np.asarray(pred, F64), np.asarray(target, F64)
        val = self.node_weight * self._base64(p, t) if self.node_weight > 0 else 0.0
        kept = int(self.keep.sum())
        if self.weight == 0 or kept == 0:
            return val
        cols = self._cols(p.shape[1])
        d = SR.apply64(p - t, self.idx, self.c)[0][:, cols] if obs is None else SR.apply64(p, self.idx, self.c)[0][:, cols] - np.asarray(obs, F64)
        return val + self.weight * float((self.keep[:, None] * d * d).sum()) / (kept * len(cols))

    def value(self, pred, target, obs=None) -> Tuple[float, float]:
        """(the loss in fp64 from the fp32 inputs, how far the device's fp32 value may sit from it): a sum of M non-negative fp32 terms
        is within M u of its exact sum whatever the order (M = N F for the MSE, the Dirichlet nodes for the L1 term, P F' for the
        samples), each term carries the roundings of its own difference, square and scale (6 u), and the sampled differences carry
        `grad`'s |d32 − d| into their squares: 2 |d| e + e²."""
        p, t = np.asarray(pred, F32).astype(F64), np.asarray(target, F32).astype(F64)
        val = self.loss(p, t, None if obs is None else np.asarray(obs, F32).astype(F64))
        base = self.node_weight * self._base64(p, t) if self.node_weight > 0 else 0.0
        allowed = (p.size + 6) * U * base
        kept = int(self.keep.sum())
        if self.weight == 0 or kept == 0:
            return val, allowed
        cols = self._cols(p.shape[1])
        x = p - t if obs is None else p
        ex = U * np.abs(x) if obs is None else np.zeros_like(x)
        q, qmag = SR.apply64(x, self.idx, self.c)
        ed = ((SR.bound32(qmag, self.k) + SR.apply64(ex, self.idx, np.abs(self.c))[0]) * (1 + 1e-3))[:, cols]
        d = q[:, cols]
        if obs is not None:
            d = d - np.asarray(obs, F32).astype(F64)
            ed = ed + U * np.abs(d)
        scale = self.weight / (kept * len(cols))
        carried = scale * float((self.keep[:, None] * (2 * np.abs(d) * ed + ed * ed)).sum())
        return val, allowed + carried + (d.size + 6) * U * (val - base) + 3 * U * val

    def grad(self, pred, target, obs=None) -> Tuple[np.ndarray, np.ndarray]:
        """(∂loss/∂pred in fp64 from the fp32 inputs = node_weight ∂GraphLoss + (2 weight / (P_kept F')) Sᵀ mask (S pred − ref), how far
        the device's fp32 gradient may sit from it).

        The allowance, u = 2⁻²⁴, term by term in the order the device computes, with q = S x, d = q − obs (or q), y = (2 weight /
        (P_kept F')) mask d scattered into the chosen columns, Sᵀ y:
          * x: pred − target is rounded once, |x32 − x| <= u |x| (values given: x = pred, no rounding);
          * q: |q32 − q| <= sampler_ref.bound32(Σ|terms| of q, k) + |S| (u |x|)                     — the forward's bound carried along;
          * d: with observations one subtraction more, |d32 − d| <= |q32 − q| + u |d|;
          * y: the square's backward (2 d, exact), the mask (0 or 1, exact), the sum's, the division's and the weight's backward are
            at most four fp32 roundings of the scale and its product with d: |y32 − y| <= s |d32 − d| + 5 u |y|, s = 2 weight / (P_kept F');
          * Sᵀ: |gx32 − Sᵀ y| <= (n_i + 1) u Σ|terms of y32| + |Sᵀ| |y32 − y|;
          * the two Σ|terms| are taken from the fp64 x and y: those of x32 and y32 exceed them by |S| |x32 − x| and |Sᵀ| |y32 − y| at most,
            times (k + 3) u or (n_i + 1) u < 1e-3 — both sums are widened by 1e-3 for it;
        and GraphLoss's own gradient (a handful of fp32 products, one more for node_weight: 7 u of its magnitude, the MSE's and the
        Dirichlet term's parts taken apart since they may cancel) and autograd's sum of the two gradients (one rounding per addition:
        3 u of the magnitudes added)."""
        import adjoint_op_ref as A
        p, t = np.asarray(pred, F32).astype(F64), np.asarray(target, F32).astype(F64)
        n, nf = p.shape
        total, allowed, size = np.zeros((n, nf)), np.zeros((n, nf)), np.zeros((n, nf))
        if self.node_weight > 0:
            base = A.graph_loss64(pred, target, self.lambda_d, self.dirichlet)[1]
            mse = A.graph_loss64(pred, target, 0.0, None)[1]
            size = self.node_weight * (np.abs(mse) + np.abs(base - mse))
            total, allowed = self.node_weight * base, 7 * U * size
        kept = int(self.keep.sum())
        if self.weight == 0 or kept == 0:
            return total, allowed
        cols = self._cols(nf)
        x = p - t if obs is None else p
        ex = U * np.abs(x) if obs is None else np.zeros_like(x)
        q, qmag = SR.apply64(x, self.idx, self.c)
        eq = (SR.bound32(qmag, self.k) + SR.apply64(ex, self.idx, np.abs(self.c))[0]) * (1 + 1e-3)
        d, ed = q[:, cols], eq[:, cols]
        if obs is not None:
            d = d - np.asarray(obs, F32).astype(F64)
            ed = ed + U * np.abs(d)
        s = 2.0 * self.weight / (kept * len(cols))
        y, ey = np.zeros_like(q), np.zeros_like(q)
        y[:, cols] = s * self.keep[:, None] * d
        ey[:, cols] = self.keep[:, None] * (s * ed + 5 * U * np.abs(s * d))
        gx, bound = adjoint64(y, *self.tables)
        egx = (bound + abs_adjoint(ey, *self.tables)) * (1 + 1e-3)
        return total + gx, allowed + egx + 3 * U * (size + np.abs(gx))
