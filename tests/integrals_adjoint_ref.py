"""Test-only numpy restatement of g4c_weighted_integrals_adjoint (csrc/control_volumes.hip).  Nothing here calls graphs4cfd_amd.

`adjoint64(x, w, entries, g, ...)` -> (acc [N, nz] fp64, addends [N, nz] fp64): the loop of include/g4c.h, vectorised over the nodes —
numpy works element by element in IEEE fp64 and never contracts, so the bits are the device's —: per column c, acc = +0, then for
e = 0 .. ne − 1 in order gw = g[q, e] · w (rounded), `acc += gw · z[b_e]` when a_e == c and `acc += gw · z[a_e]` when b_e == c (both, in
this order, when a_e == b_e == c), z = (double)x or (double)x − (double)sub, a column of −1 is 1.  An entry that does not name c is
SKIPPED; a row of w == 0, or of a group outside [0, G), is +0 whatever it holds.  `addends` is Σ|addend| of the same loop.
`cast(acc)`: the final rounding to float32 (nearest even, IEEE on overflow).  `bound(acc, addends, ne)`: what separates the device's
float32 from the exact gradient — 2⁻²⁴ |acc| for the cast and 2 (2 ne + 4) 2⁻⁵³ Σ|addends| for a sum of at most 2 ne addends, each a
product of two rounded factors, in any fixed order (the records' bound, tests/integrals_ref.py).  `cases()`: the inputs the device
test walks."""
from __future__ import annotations

import numpy as np

F32, F64, I32 = np.float32, np.float64, np.int32


def samples(x, sub=None, x_step: int = 0, sub_step: int = 0, t: int = 0, nz=None):
    x = np.asarray(x, dtype=F32)
    if nz is None:
        nz = x_step if x_step > 0 else x.shape[1]
    z = x[:, x_step * t: x_step * t + nz].astype(F64)
    if sub is not None:
        with np.errstate(all="ignore"):
            z = z - np.asarray(sub, dtype=F32)[:, sub_step * t: sub_step * t + nz].astype(F64)
    return z


def adjoint64(x, w, entries, g, sub=None, x_step: int = 0, sub_step: int = 0, t: int = 0, group=None, nz=None):
    z = samples(x, sub, x_step, sub_step, t, nz)
    n, nz = z.shape
    w = np.asarray(w, dtype=F64)
    g = np.asarray(g, dtype=F64).reshape(-1, len(entries))
    q = np.zeros(n, dtype=np.int64) if group is None else np.asarray(group).astype(np.int64)
    live = (w != 0.0) & (q >= 0) & (q < g.shape[0])
    qs = np.where(live, q, 0)
    one = np.ones(n, F64)
    acc, addends = np.zeros((n, nz), F64), np.zeros((n, nz), F64)
    with np.errstate(all="ignore"):
        for c in range(nz):
            for e, (a, b) in enumerate(entries):
                if a != c and b != c:
                    continue
                gw = g[qs, e] * w
                if a == c:
                    term = gw * (one if b < 0 else z[:, b])
                    acc[:, c] = acc[:, c] + term
                    addends[:, c] += np.abs(term)
                if b == c:
                    term = gw * (one if a < 0 else z[:, a])
                    acc[:, c] = acc[:, c] + term
                    addends[:, c] += np.abs(term)
    acc[~live] = 0.0
    addends[~live] = 0.0
    return acc, addends


def cast(acc):
    with np.errstate(all="ignore"):
        return np.asarray(acc, dtype=F64).astype(F32)


def bound(acc, addends, ne: int):
    return 2.0 ** -24 * np.abs(acc) + 2.0 * (2 * ne + 4) * 2.0 ** -53 * addends


# every entry form over columns 0 .. 2: (a, b) with a != b, a == b, (a, −1), (−1, −1), (−1, b); column 0 is named by several entries, and
# with nz > 3 the columns from 3 on by none
ENTRIES = [(0, 1), (2, 2), (1, -1), (-1, -1), (-1, 2), (0, 0), (1, 0), (2, 0)]
ENTRIES_1 = [(0, 0), (-1, -1), (0, -1), (-1, 0), (0, 0), (-1, 0), (0, -1), (0, 0)]          # nz == 1: column 0 and the constant
MAX_ROWS_A_PASS = 1024 * 256          # g4c::MAX_BLOCKS · THREADS: beyond it a thread of the launch takes several items


def entries_for(nz: int, ne: int):
    if nz == 1:
        return ENTRIES_1[:ne]
    if nz >= 3:
        return ENTRIES[:ne]
    raise ValueError(nz)


def make(n, nz, ne, *, sub, strided, groups, t=0, pad=3, seed=0):
    """One case.  `sub`: None / "plain" / "strided"; `strided`: x holds every step (x_step = nz + 1); `groups`: 0 (group NULL) or G,
    then one row names a group outside [0, G) and one a negative one (n permitting); a tenth of the rows has weight 0 (one of them −0)
    and holds NaN / inf in x and sub."""
    rng = np.random.default_rng(1000 * nz + 10 * ne + n % 997 + seed)
    steps = t + 1
    x_step = nz + 1 if strided else 0
    x = rng.standard_normal((n, (x_step * steps if strided else nz) + pad)).astype(F32)
    s, sub_step = None, 0
    if sub is not None:
        sub_step = nz + 2 if sub == "strided" else 0
        s = rng.standard_normal((n, (sub_step * steps if sub_step else nz) + pad + 1)).astype(F32)
    w = rng.random(n) * 10.0 ** rng.integers(-3, 1, n)
    zero = np.nonzero(rng.random(n) < 0.1)[0] if n > 4 else np.zeros(0, np.int64)
    w[zero] = 0.0
    if zero.size:
        w[zero[0]] = -0.0
        x[zero[0::2]] = np.nan
        x[zero[1::2]] = np.inf
        if s is not None:
            s[zero[0::3]] = -np.inf
    G = max(groups, 1)
    g = rng.standard_normal((G, ne))
    group = None
    if groups:
        group = rng.integers(0, G, n).astype(I32)
        if n > 2:
            live = np.nonzero(w != 0.0)[0]
            group[live[0]] = G
            group[live[-1]] = -1
    return dict(x=x, sub=s, w=w, g=g, group=group, entries=entries_for(nz, ne), nz=nz, x_step=x_step, sub_step=sub_step, t=t,
                gx_pad=2 if pad else 0)


def cases():
    """(id, case) pairs: N = 1, 255, 256, 257 and one above MAX_ROWS_A_PASS; ne = 1 .. 8; nz = 1, 3, 4, 5, 9; leading dimensions above nz;
    strided sources at t > 0; group NULL and G = 3 with rows out of range; zero-weight rows that hold NaN."""
    out = []
    for n in (1, 255, 256, 257):
        out.append((f"n{n}", make(n, 4, 8, sub="strided", strided=False, groups=3, t=2)))
    for ne in range(1, 9):
        out.append((f"ne{ne}", make(257, 3, ne, sub=None, strided=False, groups=0)))
    for nz in (1, 3, 4, 5, 9):
        out.append((f"nz{nz}", make(257, nz, 8, sub="plain", strided=True, groups=3, t=1)))
    out.append(("dense", make(300, 3, 2, sub="plain", strided=False, groups=0, pad=0)))          # x_ld == sub_ld − 1 == gx_ld == nz
    out.append(("tall", make(MAX_ROWS_A_PASS + 300, 3, 8, sub="plain", strided=False, groups=3)))
    return out
