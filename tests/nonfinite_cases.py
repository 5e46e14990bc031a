"""Non-finite and edge-of-range samples for the in-step diagnostics: the poisons, where they are placed, and the checkers the host
tests (tests/test_nonfinite_ref.py) and the GPU tests (tests/test_gpu_nonfinite.py) share.  CPU data only (numpy); nothing here
calls graphs4cfd_amd.

The rule under test (include/g4c.h, DESIGN §5 "non-finite samples"): (1) sums follow IEEE; (2) an extremum over samples of which one
is NaN is NaN, at every stage of the reduction; (3) masks select; (4) a poisoned value changes only what depends on it.

Only FIELD VALUES, TARGETS and INCOMING GRADIENTS are poisoned — never coordinates, indices or weight tables.

Clean data are small integers (`clean`), so every fp64 sum of the clean part is exact in any order and the comparison with a
restatement that adds in another order can be exact.  The poisons keep that property:
  nan, +inf, -inf   one value at every placed row of one column;
  inf_pair          +Inf at the placed rows and -Inf at a partner row of the SAME column (the next row, or the one before the last
                    row): the column's sum is NaN (Inf - Inf), its extrema are +-Inf.  A single row (n = 1) has no partner: +Inf alone;
  flt_max           +3.4028235e38 in the column and, when there is another column, -3.4028235e38 at the same rows of the column
                    before it: finite data whose fp32 products and differences overflow.  One sign per column, so that an fp64 sum
                    holds FLT_MAX-sized terms of one sign only (small integers beside them are absorbed in any order);
  subnormal         the WHOLE array scaled by 2^-133 (integers up to 8 become fp32 subnormals, exact multiples of 2^-133): products
                    w * diff and coef * x of the fp32 launches land below 2^-126 and are rounded on the 2^-149 grid, differences of
                    neighbours cancel inside that range; in fp64 everything stays exact.  Every entry is dirty;
  neg_zero          -0.0 at the placed rows.
`poison` returns the poisoned copy and the mask of the entries whose BITS changed."""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np

F32, F64 = np.float32, np.float64
FLT_MAX = np.float32(3.4028235e38)
TINY = np.float32(2.0 ** -133)
POISONS = ("nan", "+inf", "-inf", "inf_pair", "flt_max", "subnormal", "neg_zero")
SIZES = (1, 65, 257, 1000)
BIG = 65_537          # 257 workgroups of 256: thread 0 of a stats kernel adds a second partial, that of the last node alone
FIELDS = (1, 3)
BINS = (1, 9)
TIMES = ("first", "middle", "last")          # of a time accumulator: the pivot, a middle sample, the last


def placements(n: int) -> Dict[str, Tuple[int, ...]]:
    """name -> rows: each makes ONE stage of the records' reduction the only carrier of the poison."""
    out = {"node0": (0,)}
    if n >= 65:
        out["wave_edge"] = (63, 64)          # the last lane of wave 0 and the first of wave 1
    if n >= 257:
        out["wave4"] = (200,)                # a lane of the fourth wave of workgroup 0 only
    if n == 257:
        out["wg2"] = (256,)                  # the second workgroup only (one live thread)
    if n > 1 and (n - 1,) not in out.values():
        out["last"] = (n - 1,)
    return out


def cases() -> List[Tuple[int, str]]:
    """[(n, placement)] over SIZES, and the last node of BIG."""
    return [(n, p) for n in SIZES for p in placements(n)] + [(BIG, "last")]


def rows_of(n: int, placement: str) -> Tuple[int, ...]:
    return placements(n)[placement]


def clean(rng, *shape, lo: int = -8, hi: int = 8) -> np.ndarray:
    return rng.integers(lo, hi + 1, shape).astype(F32)


def bits(a) -> np.ndarray:
    a = np.ascontiguousarray(a)
    return a.view({2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize])


def partner(n: int, rows) -> Optional[int]:
    if n < 2:
        return None
    return rows[-1] + 1 if rows[-1] + 1 < n else rows[0] - 1


def poison(x: np.ndarray, name: str, rows, col: int) -> Tuple[np.ndarray, np.ndarray]:
    """(poisoned copy of x [n, w] fp32, dirty bool [n, w]): `name` at `rows` of column `col`."""
    assert name in POISONS and x.dtype == F32 and x.ndim == 2
    y = x.copy()
    rows = list(rows)
    if name == "subnormal":
        y = (y * TINY).astype(F32)
    elif name == "inf_pair":
        y[rows, col] = np.inf
        p = partner(x.shape[0], rows)
        if p is not None:
            y[p, col] = -np.inf
    elif name == "flt_max":
        y[rows, col] = FLT_MAX
        if x.shape[1] > 1:
            y[rows, (col - 1) % x.shape[1]] = -FLT_MAX
    else:
        y[rows, col] = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf, "neg_zero": -0.0}[name]
    return y, bits(y) != bits(x)


def same_bits(got, ref, what: str = "", where=None) -> None:
    """Equal as integers, except that a NaN equals a NaN of any payload (rule 1).  `where`: a bool mask of the elements compared."""
    g = got.detach().cpu().numpy() if hasattr(got, "detach") else np.asarray(got)
    r = np.asarray(ref)
    assert g.dtype == r.dtype and g.shape == r.shape, f"{what}: {g.dtype} {g.shape} vs {r.dtype} {r.shape}"
    bad = (bits(g) != bits(r)) & ~((g != g) & (r != r))
    if where is not None:
        bad &= np.broadcast_to(np.asarray(where), bad.shape)
    if bad.any():
        pos = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at {list(pos)}: got {g[pos]!r} "
                             f"(0x{int(bits(g)[pos]) & (2 ** (8 * g.dtype.itemsize) - 1):x}) want {r[pos]!r} "
                             f"(0x{int(bits(r)[pos]) & (2 ** (8 * r.dtype.itemsize) - 1):x})")


def identical(a, b, what: str = "", where=None) -> None:
    """Equal as integers, payloads included (locality against the clean run; two runs of one launch)."""
    x = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    y = b.detach().cpu().numpy() if hasattr(b, "detach") else np.asarray(b)
    assert x.dtype == y.dtype and x.shape == y.shape, f"{what}: {x.dtype} {x.shape} vs {y.dtype} {y.shape}"
    bad = bits(x) != bits(y)
    if where is not None:
        bad &= np.broadcast_to(np.asarray(where), bad.shape)
    if bad.any():
        pos = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ in their bits, first at {list(pos)}: {x[pos]!r} vs {y[pos]!r}")


def rejects(check, *args, **kw) -> bool:
    try:
        check(*args, **kw)
    except AssertionError:
        return True
    return False


# ------------------------------------------------------------------ what a poisoned entry reaches
def receivers(off, src, dirty_rows: np.ndarray) -> np.ndarray:
    """bool [n]: the nodes whose stencil (themselves and the senders of their in-edges, CSR off / src) touches a dirty row."""
    off = np.asarray(off, dtype=np.int64)
    n = off.size - 1
    hit = np.asarray(dirty_rows, dtype=bool).copy()
    node = np.repeat(np.arange(n), np.diff(off))
    e = np.nonzero(hit[np.asarray(src, dtype=np.int64)])[0] if len(src) else np.zeros(0, np.int64)
    hit[node[e]] = True
    return hit


def senders(off, src, dirty_rows: np.ndarray) -> np.ndarray:
    """bool [n]: the dirty rows and the senders of their in-edges (where an adjoint carries an incoming gradient)."""
    off = np.asarray(off, dtype=np.int64)
    hit = np.asarray(dirty_rows, dtype=bool).copy()
    for i in np.nonzero(dirty_rows)[0]:
        hit[np.asarray(src, dtype=np.int64)[off[i]:off[i + 1]]] = True
    return hit


# ------------------------------------------------------------------ the cases of the records and of the time accumulators
T_REC, STEPS_REC = 2, 4


def record_case(n, placement, name, nf, where, mask_kind):
    """(pred, target, mask, dirty rows): `name` in column nf - 1 of pred or of the target's columns of step T_REC."""
    rng = np.random.default_rng(7 * n + nf)
    rows = rows_of(n, placement)
    pred, target = clean(rng, n, nf), clean(rng, n, nf * STEPS_REC, lo=1)
    if where == "pred":
        pred, dirty = poison(pred, name, rows, nf - 1)
    else:
        cols, dirty = poison(target[:, nf * T_REC:nf * (T_REC + 1)].copy(), name, rows, nf - 1)
        target[:, nf * T_REC:nf * (T_REC + 1)] = cols
    dirty_rows = dirty.any(1)
    mask = {None: None, "in": dirty_rows | (rng.random(n) < 0.3), "out": ~dirty_rows & (rng.random(n) < 0.5)}[mask_kind]
    return pred, target, mask, dirty_rows


T_ACC = 6          # steps 0 .. 5; the window (1, 2) takes 1, 3, 5
TIME_OF = {"first": 1, "middle": 3, "last": 5}


def time_samples(n, nf, name, rows, when, seed=0):
    """Six predictions; `name` in column nf - 1 of the one at TIME_OF[when] (inf_pair: -Inf at the SAME rows of another window step, so
    that Inf - Inf happens in time, at one node)."""
    rng = np.random.default_rng(11 * n + nf + seed)
    samples = [clean(rng, n, nf) for _ in range(T_ACC)]
    t = TIME_OF[when]
    dirty = np.zeros((n, nf), bool)
    if name == "inf_pair":
        other = 5 if t != 5 else 3
        samples[t][list(rows), nf - 1] = np.inf
        samples[other][list(rows), nf - 1] = -np.inf
        dirty[list(rows), nf - 1] = True
    elif name == "subnormal":
        samples = [(s * TINY).astype(F32) for s in samples]
        dirty[:] = True
    else:
        samples[t], dirty = poison(samples[t], name, rows, nf - 1)
    return samples, dirty


def same_values(got, ref, what: str = "") -> None:
    """fp64 outputs: equal values, a NaN equals a NaN of any payload."""
    g = got.detach().cpu().numpy() if hasattr(got, "detach") else np.asarray(got)
    r = np.asarray(ref)
    assert g.dtype == r.dtype == F64 and g.shape == r.shape, f"{what}: {g.dtype} {g.shape} vs {r.dtype} {r.shape}"
    bad = ~((g == r) | ((g != g) & (r != r)))
    if bad.any():
        pos = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at {list(pos)}: got {g[pos]!r} want {r[pos]!r}")
