"""Test-only numpy restatement of g4c_weighted_integrals (csrc/control_volumes.hip).  Nothing here calls graphs4cfd_amd.

`terms(x, w, entries, ...)` [N, ne] fp64: per row and entry (a, b) the term w · (z[a] · z[b]) — z = (double)x or (double)x − (double)sub,
a column of −1 is 1, the product of the two samples rounded once, then the product with w (numpy never contracts); a row of w == 0 is
LEFT OUT (`keep`), whatever it holds.  `sum_order(T, keep)`: the device's order — at most 1024 workgroups of 256, thread tid of workgroup
b adds the rows 256 b + tid, + 256 · workgroups, ... from +0, a xor butterfly 32, 16, .., 1 per wave of 64, the four waves in order; then
thread i of one workgroup adds the partials of workgroups i, i + 256, ... and reduces the same way.  `sum_bound(T, keep)`: the records'
bound on a sum of n terms in any fixed order, 2 (n + 4) 2⁻⁵³ Σ|terms|.  `scratch_doubles(n, ne)`: 8 + workgroups · ne."""
from __future__ import annotations

import math

import numpy as np

F32, F64 = np.float32, np.float64
THREADS, WAVE, MAX_BLOCKS, HEADER = 256, 64, 1024, 8


def blocks(n: int) -> int:
    return min(max(-(-n // THREADS), 1), MAX_BLOCKS)


def scratch_doubles(n: int, ne: int) -> int:
    return HEADER + blocks(n) * ne


def terms(x, w, entries, sub=None, x_step: int = 0, sub_step: int = 0, t: int = 0):
    """(T [N, ne], keep [N] bool)."""
    x = np.asarray(x, dtype=F32)
    w = np.asarray(w, dtype=F64)
    z = x[:, x_step * t:].astype(F64)
    if sub is not None:
        s = np.asarray(sub, dtype=F32)[:, sub_step * t:].astype(F64)
        width = min(z.shape[1], s.shape[1])
        z = z[:, :width] - s[:, :width]
    one = np.ones(x.shape[0], F64)
    with np.errstate(all="ignore"):
        T = np.stack([w * ((one if a < 0 else z[:, a]) * (one if b < 0 else z[:, b])) for a, b in entries], axis=1)
    return T, w != 0.0


def _reduce(acc: np.ndarray) -> np.ndarray:
    """acc [256, ne]: butterfly per wave, then the four waves in order."""
    lane = np.arange(THREADS)
    with np.errstate(all="ignore"):
        for m in (32, 16, 8, 4, 2, 1):
            acc = acc + acc[lane ^ m]
        s = acc[0]
        for wv in range(1, THREADS // WAVE):
            s = s + acc[wv * WAVE]
    return s


def sum_order(T: np.ndarray, keep: np.ndarray) -> np.ndarray:
    n, ne = T.shape
    nb = blocks(n)
    stride = nb * THREADS
    T = np.where(keep[:, None], T, 0.0)          # (acc + (+0) == acc for every acc this sum can hold: it starts at +0)
    pad = np.zeros((-(-max(n, 1) // stride) * stride, ne), F64)
    pad[:n] = T
    acc = np.zeros((stride, ne), F64)
    with np.errstate(all="ignore"):
        for r in range(pad.shape[0] // stride):
            acc = acc + pad[r * stride:(r + 1) * stride]
    partial = np.stack([_reduce(acc[b * THREADS:(b + 1) * THREADS]) for b in range(nb)])
    acc2 = np.zeros((THREADS, ne), F64)
    with np.errstate(all="ignore"):
        for r in range(-(-nb // THREADS)):
            blk = partial[r * THREADS:(r + 1) * THREADS]
            acc2[:blk.shape[0]] = acc2[:blk.shape[0]] + blk
    return _reduce(acc2)


def sum_exact(T: np.ndarray, keep: np.ndarray) -> np.ndarray:
    return np.array([math.fsum(T[keep, e].tolist()) for e in range(T.shape[1])])


def sum_bound(T: np.ndarray, keep: np.ndarray) -> np.ndarray:
    n = T.shape[0]
    return 2.0 * (n + 4) * 2.0 ** -53 * np.abs(T[keep]).sum(0)
