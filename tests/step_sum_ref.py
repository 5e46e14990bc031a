"""Test-only numpy restatement of the step-record core's summation order (csrc/step_record.h).  Nothing here calls graphs4cfd_amd.

`sum_order(T, keep)`: the device's order — at most 1024 workgroups of 256, thread tid of workgroup b adds the rows 256 b + tid,
+ 256 · workgroups, ... from +0, a xor butterfly 32, 16, .., 1 per wave of 64, the four waves in order; then thread i of one workgroup
adds the partials of workgroups i, i + 256, ... and reduces the same way.  `is_max` [ne] bool marks the columns that are maxima instead
of sums (of values >= 0, as every |·| the device takes a maximum of: they start at +0 too); a NaN stays one, as on the device.
`scratch_doubles(n, ne)`: 8 + workgroups · ne."""
from __future__ import annotations

import numpy as np

F64 = np.float64
THREADS, WAVE, MAX_BLOCKS, HEADER = 256, 64, 1024, 8


def blocks(n: int) -> int:
    return min(max(-(-n // THREADS), 1), MAX_BLOCKS)


def scratch_doubles(n: int, ne: int) -> int:
    return HEADER + blocks(n) * ne


def _combine(a: np.ndarray, b: np.ndarray, is_max) -> np.ndarray:
    """a + b, or the NaN-true maximum in the columns of is_max (numpy.maximum returns NaN if either is one)."""
    return a + b if is_max is None else np.where(is_max, np.maximum(a, b), a + b)


def _reduce(acc: np.ndarray, is_max=None) -> np.ndarray:
    """acc [256, ne]: butterfly per wave, then the four waves in order."""
    lane = np.arange(THREADS)
    with np.errstate(all="ignore"):
        for m in (32, 16, 8, 4, 2, 1):
            acc = _combine(acc, acc[lane ^ m], is_max)
        s = acc[0]
        for wv in range(1, THREADS // WAVE):
            s = _combine(s, acc[wv * WAVE], is_max)
    return s


def sum_order(T: np.ndarray, keep: np.ndarray, is_max=None) -> np.ndarray:
    n, ne = T.shape
    nb = blocks(n)
    stride = nb * THREADS
    T = np.where(keep[:, None], T, 0.0)          # (acc + (+0) == acc for every acc this sum can hold: it starts at +0)
    pad = np.zeros((-(-max(n, 1) // stride) * stride, ne), F64)
    pad[:n] = T
    acc = np.zeros((stride, ne), F64)
    with np.errstate(all="ignore"):
        for r in range(pad.shape[0] // stride):
            acc = _combine(acc, pad[r * stride:(r + 1) * stride], is_max)
    partial = np.stack([_reduce(acc[b * THREADS:(b + 1) * THREADS], is_max) for b in range(nb)])
    acc2 = np.zeros((THREADS, ne), F64)
    with np.errstate(all="ignore"):
        for r in range(-(-nb // THREADS)):
            blk = partial[r * THREADS:(r + 1) * THREADS]
            acc2[:blk.shape[0]] = _combine(acc2[:blk.shape[0]], blk, is_max)
    return _reduce(acc2, is_max)
