"""Test-only numpy restatement of csrc/point_sample.hip (g4c_sample_weights, g4c_sample_points): the fp64 coefficients of the linear
moving-least-squares fit from a given neighbour table, the fp32 loop of the apply and its fp64 form, the clouds the tests use and the
checkers.  numpy only; `idx` is [P, k] here (the library's tables are j-major, [k, P])."""
from typing import Optional

import numpy as np

F32, F64 = np.float32, np.float64
THRESHOLD = 1e-12


# ------------------------------------------------------------------ clouds
def cloud(n: int, dim: int, seed: int = 0) -> np.ndarray:
    """n uniform random points in [0, 1]^dim, float32."""
    return np.random.default_rng(1000 * dim + n + seed).random((n, dim)).astype(F32)


MAX_QUERIES = 257


def queries(p: int, dim: int, seed: int = 0) -> np.ndarray:
    """The first p <= 257 of one fixed set of uniform random points in [-0.1, 1.1]^dim (some outside the cloud's hull), float32: what
    holds for the 257 holds for every shorter set."""
    assert 0 <= p <= MAX_QUERIES
    return np.ascontiguousarray((np.random.default_rng(77 * dim + seed).random((MAX_QUERIES, dim)) * 1.2 - 0.1).astype(F32)[:p])


# the clouds, neighbour counts and powers of the weight tolerance test (tests/test_gpu_point_sampler.py); tests/test_sampler_ref.py
# asserts that none of their points sits near the degeneracy threshold
WEIGHT_CLOUDS = (65, 1000)
WEIGHT_K = {2: (1, 2, 6, 8, 16), 3: (1, 3, 8, 10, 16)}
POWERS = (0, 1, 2)


def nearest(pos32: np.ndarray, q32: np.ndarray, k: int) -> np.ndarray:
    """[P, k] the k nearest nodes of every query by brute force in fp64, nearest first (ties: the lower row) — for the host tests;
    the GPU tests take the device's table."""
    d = pos32.astype(F64)[None, :, :] - q32.astype(F64)[:, None, :]
    r2 = np.zeros(d.shape[:2])
    for a in range(d.shape[2]):
        r2 = r2 + d[:, :, a] * d[:, :, a]
    return np.argsort(r2, axis=1, kind="stable")[:, :k].astype(np.int32)


# ------------------------------------------------------------------ coefficients
def _adjugate(m, dim):
    """(adj, det, tr) of the symmetric matrices m [P, NM] (upper triangle, row-major), in the kernel's order of operations."""
    if dim == 2:
        adj = np.stack([m[:, 2], -m[:, 1], m[:, 0]], axis=1)
        det = m[:, 0] * m[:, 2] - m[:, 1] * m[:, 1]
        tr = m[:, 0] + m[:, 2]
    else:
        adj = np.stack([m[:, 3] * m[:, 5] - m[:, 4] * m[:, 4], m[:, 2] * m[:, 4] - m[:, 1] * m[:, 5], m[:, 1] * m[:, 4] - m[:, 2] * m[:, 3],
                        m[:, 0] * m[:, 5] - m[:, 2] * m[:, 2], m[:, 1] * m[:, 2] - m[:, 0] * m[:, 4], m[:, 0] * m[:, 3] - m[:, 1] * m[:, 1]], axis=1)
        det = (m[:, 0] * adj[:, 0] + m[:, 1] * adj[:, 1]) + m[:, 2] * adj[:, 2]
        tr = (m[:, 0] + m[:, 3]) + m[:, 5]
    return adj, det, tr


def _sym_times(adj, v, dim):
    """adj v for the symmetric adj [P, NM]."""
    if dim == 2:
        return np.stack([adj[:, 0] * v[:, 0] + adj[:, 1] * v[:, 1], adj[:, 1] * v[:, 0] + adj[:, 2] * v[:, 1]], axis=1)
    return np.stack([(adj[:, 0] * v[:, 0] + adj[:, 1] * v[:, 1]) + adj[:, 2] * v[:, 2],
                     (adj[:, 1] * v[:, 0] + adj[:, 3] * v[:, 1]) + adj[:, 4] * v[:, 2],
                     (adj[:, 2] * v[:, 0] + adj[:, 4] * v[:, 1]) + adj[:, 5] * v[:, 2]], axis=1)


def coefficients(pos32: np.ndarray, q32: np.ndarray, idx: np.ndarray, power: int):
    """(c64 [P, k], c32 [P, k], distance float32 [P], degenerate uint8 [P], ratio [P]) — the rule of include/g4c.h in fp64, every sum
    over j ascending; `ratio` = det M / (tr M / dim)^dim (nan at an exact hit), what the degeneracy test compares with 1e-12."""
    pos32, q32, idx = np.asarray(pos32, F32), np.asarray(q32, F32), np.asarray(idx)
    P, k = idx.shape
    dim = pos32.shape[1]
    with np.errstate(all="ignore"):
        d = pos32.astype(F64)[idx] - q32.astype(F64)[:, None, :]            # [P, k, dim]
        r2 = np.zeros((P, k))
        for a in range(dim):
            r2 = r2 + d[:, :, a] * d[:, :, a]
        w = np.ones((P, k)) if power == 0 else (1.0 / np.sqrt(r2) if power == 1 else 1.0 / r2)
        W = np.zeros(P)
        dbar = np.zeros((P, dim))
        for j in range(k):
            W = W + w[:, j]
            dbar = dbar + w[:, j, None] * d[:, j]
        dbar = dbar / W[:, None]
        e = d - dbar[:, None, :]
        pairs = [(a, b) for a in range(dim) for b in range(a, dim)]
        m = np.zeros((P, len(pairs)))
        for j in range(k):
            for i, (a, b) in enumerate(pairs):
                m[:, i] = m[:, i] + (w[:, j] * e[:, j, a]) * e[:, j, b]
        adj, det, tr = _adjugate(m, dim)
        mean = tr / dim
        thr = mean * mean * mean if dim == 3 else mean * mean
        ratio = det / thr
        degen = ~(det > THRESHOLD * thr) | (k <= dim)
        v = _sym_times(adj, dbar, dim)
        s = np.zeros((P, k))
        for a in range(dim):
            s = s + e[:, :, a] * v[:, None, a]
        c = w * (1.0 / W[:, None] - s / det[:, None])
        c = np.where(degen[:, None], w / W[:, None], c)
        hit = r2[:, 0] == 0.0 if k else np.zeros(P, bool)
        unit = np.zeros(k)
        unit[:1] = 1.0
        c = np.where(hit[:, None], unit[None, :], c)
        degen = degen & ~hit
        ratio = np.where(hit, np.nan, ratio)
        distance = np.sqrt(r2[:, 0]).astype(F32)
    return c, c.astype(F32), distance, degen.astype(np.uint8), ratio


def coefficient_bound(c64: np.ndarray) -> np.ndarray:
    """[P, 1]: 2^-23 max_j |c_ref,j| per point — half an ulp of the one rounding to fp32 and a margin of the same size."""
    return 2.0 ** -23 * np.abs(c64).max(1, keepdims=True) if c64.shape[1] else np.zeros((c64.shape[0], 1))


# ------------------------------------------------------------------ apply
def apply32(x: np.ndarray, idx: np.ndarray, c32: np.ndarray) -> np.ndarray:
    """cur[p, f] = Σ_j c[p, j] x[idx[p, j], f] as a numpy.float32 loop: j ascending, each product rounded, the first starts the sum."""
    x, c32 = np.asarray(x, F32), np.asarray(c32, F32)
    acc = np.zeros((idx.shape[0], x.shape[1]), F32)
    for j in range(idx.shape[1]):
        pr = (c32[:, j, None] * x[idx[:, j]]).astype(F32)
        acc = pr if j == 0 else (acc + pr).astype(F32)
    return acc


def apply64(x: np.ndarray, idx: np.ndarray, c) -> tuple:
    """(Σ_j c_j x_j, Σ_j |c_j x_j|) in fp64 over the coefficients as given."""
    x, c = np.asarray(x).astype(F64), np.asarray(c).astype(F64)
    val = np.zeros((idx.shape[0], x.shape[1]))
    mag = np.zeros_like(val)
    for j in range(idx.shape[1]):
        t = c[:, j, None] * x[idx[:, j]]
        val, mag = val + t, mag + np.abs(t)
    return val, mag


def bound32(mag: np.ndarray, k: int) -> np.ndarray:
    """|cur32 − cur64| <= (k + 3) 2^-24 Σ_j |c_j x_j|: k product roundings and k − 1 additions, with a margin of 4."""
    return (k + 3) * 2.0 ** -24 * mag


def slot_of(t: int, every: int, n_slots: int) -> Optional[int]:
    if every > 0 and t >= 0 and (t + 1) % every == 0 and (t + 1) // every - 1 < n_slots:
        return (t + 1) // every - 1
    return None


# ------------------------------------------------------------------ checkers
def _np(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def same(got, ref, what: str = "") -> None:
    """Bit for bit (values; nan equals nan; -0 and +0 are told apart through the sign)."""
    g, ref = _np(got), np.asarray(ref)
    assert g.dtype == ref.dtype and tuple(g.shape) == tuple(ref.shape), f"{what}: {g.dtype} {g.shape} vs {ref.dtype} {ref.shape}"
    bad = ~((g == ref) | ((g != g) & (ref != ref)))
    if g.dtype.kind == "f":
        bad |= np.signbit(g) != np.signbit(ref)
    if bad.any():
        at = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at {list(at)}: got {g[at]!r} want {ref[at]!r}")


def within(got, ref, allowed, what: str = "") -> float:
    """|got − ref| <= allowed elementwise; returns the largest measured / allowed ratio (0 where both are 0)."""
    g = _np(got)
    assert tuple(g.shape) == tuple(np.shape(ref)), f"{what}: {g.shape} vs {np.shape(ref)}"
    err = np.abs(g.astype(F64) - np.asarray(ref, dtype=F64))
    allowed = np.broadcast_to(np.asarray(allowed, dtype=F64), err.shape)
    bad = ~(err <= allowed)
    if bad.any():
        at = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements are outside the bound, first at {list(at)}: got {g[at]!r} "
                             f"want {np.asarray(ref)[at]!r}, allowed {allowed[at]!r}")
    with np.errstate(all="ignore"):
        r = np.where(allowed > 0, err / allowed, 0.0)
    return float(r.max()) if r.size else 0.0


def ulps32(got, ref) -> int:
    """The largest distance in float32 ulps between two arrays of non-negative finite float32."""
    g, r = _np(got).astype(F32).view(np.int32).astype(np.int64), np.asarray(ref, F32).view(np.int32).astype(np.int64)
    return int(np.abs(g - r).max()) if g.size else 0


def rejects(check, *args, **kw) -> bool:
    try:
        check(*args, **kw)
    except AssertionError:
        return True
    return False
