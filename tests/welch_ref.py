"""Test-only fp64 restatement of g4c_rollout_welch (csrc/rollout_welch.hip) as a plain numpy loop over steps in time order, the
derived quantities of Welch's estimator formed from its sums, and the checkers its tests share.  Nothing here calls graphs4cfd_amd.

State (all fp64, plane-major, planes first): two alternating sets of pivot [2 nf, n], sum [2 nf, n], re [2 nf K, n], im [2 nf K, n] —
set c, field f at plane c nf + f, bin k at plane (c nf + f) K + k —, the averages pxx [nf K, n] and, with a reference, cxr_re, cxr_im
[nf K, n], seg_power [max_segments, P, nf, K] for P tracked rows, and window = [origin, last, closed] (integers).  The table tw [L, K, 2]
and its column sums W [K, 2] are inputs (any values).

One call, at step index t, is `accumulate` then `close`, with the sample x_f = x[:, x_step t + f] widened to fp64 and j = (t - origin) /
stride, on the lattice iff n > 0, 0 <= t < max_steps, t >= origin and (t - origin) % stride == 0; otherwise NOTHING changes.
  accumulate: for every segment s with 0 <= q = j - s H < L, in set s & 1:  q == 0: pivot = x, sum = re = im = 0 — stored, whatever the
      set held;  later: d = x - pivot; sum += d; re += d tw[q, k, 0]; im += d tw[q, k, 1] (the product rounded, then added);  last = t.
  close: iff j >= L - 1 and (j - (L - 1)) % H == 0, s = (j - (L - 1)) / H, set s & 1:  m = sum inv_L; ar = re - m W[k, 0]; ai = im - m
      W[k, 1]; p = ar ar + ai ai; pxx = p (s == 0) or pxx + p;  with a reference (its state, a row or the same row, a field or the same
      field) (rr, ri) the same of the reference's set: cr = ar rr + ai ri, ci = ai rr - ar ri, stored or added alike;  seg_power[s, p] =
      p of row track[p] when s < max_segments;  closed = s + 1.
Every operation is one numpy operation on fp64: rounded on its own.  The device's bits must equal these exactly.

`wrong=` names ONE deliberate mistake for the negative controls: "parity" (set s instead of s & 1), "no-detrend" (m = 0), "conj" (the
sign of ci), "hop+1" (segments every H + 1 samples), "close-early" (closing at q = L - 2), "ref-row+1" (the reference's row + 1,
wrapped), "add-at-0" (segment 0 adds to what the averages held)."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

F64 = np.float64
SETS = ("pivot", "sum", "re", "im")
WRONG = ("parity", "no-detrend", "conj", "hop+1", "close-early", "ref-row+1", "add-at-0")
PARITY_SETS = 64          # room for the "parity" control, which never reuses a set


def names(st) -> tuple:
    return SETS + ("pxx",) + (("cxr_re", "cxr_im") if "cxr_re" in st else ())


def new_state(n: int, nf: int, K: int, origin: int = 0, reference: bool = False, tracked: int = 0, max_segments: int = 0,
              fill: float = 0.0, sets: int = 2) -> Dict[str, np.ndarray]:
    st = {k: np.full((sets * nf * (K if k in ("re", "im") else 1), n), fill, dtype=F64) for k in SETS}
    st["pxx"] = np.full((nf * K, n), fill, dtype=F64)
    if reference:
        st["cxr_re"], st["cxr_im"] = np.full((nf * K, n), fill, dtype=F64), np.full((nf * K, n), fill, dtype=F64)
    if tracked:
        st["seg_power"] = np.full((max_segments, tracked, nf, K), fill, dtype=F64)
    st["window"] = np.array([origin, -1, 0], dtype=np.int64)
    return st


def sample_index(st, t: int, max_steps: int, stride: int) -> int:
    """j of step t, or -1 off the lattice."""
    origin = int(st["window"][0])
    if not (0 <= t < max_steps) or t < origin or (t - origin) % stride != 0:
        return -1
    return (t - origin) // stride


def sample(x, nf: int, t: int, x_step: int = 0) -> np.ndarray:
    """x [nf, n] in fp64."""
    a = np.asarray(x, dtype=np.float32)
    return np.ascontiguousarray(a[:, x_step * t:x_step * t + nf].astype(F64).T)


def accumulate(st, x, t: int, max_steps: int, tw, stride: int, H: int, x_step: int = 0, wrong: Optional[str] = None):
    """The accumulate kernel at step index t, on `st` in place (which is returned)."""
    with np.errstate(all="ignore"):          # (inf and NaN samples follow IEEE, silently)
        return _accumulate(st, x, t, max_steps, tw, stride, H, x_step, wrong)


def _accumulate(st, x, t, max_steps, tw, stride, H, x_step, wrong):
    assert wrong is None or wrong in WRONG, wrong
    tw = np.asarray(tw, dtype=F64)
    L, K = tw.shape[0], tw.shape[1]
    nf, n = st["pxx"].shape[0] // K, st["pxx"].shape[1]
    j = sample_index(st, t, max_steps, stride)
    if n == 0 or j < 0:
        return st
    hop = H + 1 if wrong == "hop+1" else H
    xs = sample(x, nf, t, x_step)
    for s in range(j // hop + 1):
        q = j - s * hop
        if not 0 <= q < L:
            continue
        c = s if wrong == "parity" else s & 1
        pv, sm = st["pivot"][c * nf:(c + 1) * nf], st["sum"][c * nf:(c + 1) * nf]
        re, im = st["re"][c * nf * K:(c + 1) * nf * K], st["im"][c * nf * K:(c + 1) * nf * K]
        if q == 0:
            pv[:] = xs
            sm[:], re[:], im[:] = 0.0, 0.0, 0.0
            continue
        d = xs - pv
        sm += d
        for f in range(nf):
            for k in range(K):
                pr = d[f] * tw[q, k, 0]
                pi = d[f] * tw[q, k, 1]
                re[f * K + k] += pr
                im[f * K + k] += pi
    st["window"][1] = t
    return st


def _modes(st, c: int, nf: int, K: int, W, inv_L: float, detrend: bool):
    """(ar, ai) [nf, K, n] of set c."""
    m = st["sum"][c * nf:(c + 1) * nf] * inv_L
    if not detrend:
        m = np.zeros_like(m)
    re = st["re"][c * nf * K:(c + 1) * nf * K].reshape(nf, K, -1)
    im = st["im"][c * nf * K:(c + 1) * nf * K].reshape(nf, K, -1)
    mr = m[:, None, :] * W[None, :, 0, None]
    mi = m[:, None, :] * W[None, :, 1, None]
    return re - mr, im - mi


def close(st, t: int, max_steps: int, L: int, W, stride: int, H: int, ref=None, ref_row: int = -1, ref_field: int = -1, track=None,
          wrong: Optional[str] = None):
    """The close kernel at step index t, on `st` in place.  `ref`: the reference's state (st itself for the "node" kind, another
    accumulator's for the "target" kind), or None without a reference."""
    assert wrong is None or wrong in WRONG, wrong
    W = np.asarray(W, dtype=F64)
    K = W.shape[0]
    nf, n = st["pxx"].shape[0] // K, st["pxx"].shape[1]
    j = sample_index(st, t, max_steps, stride)
    if n == 0 or j < 0:
        return st
    hop = H + 1 if wrong == "hop+1" else H
    end = L - 2 if wrong == "close-early" else L - 1
    if j < end or (j - end) % hop != 0:
        return st
    s = (j - end) // hop
    c = s if wrong == "parity" else s & 1
    inv_L = 1.0 / L
    with np.errstate(all="ignore"):
        ar, ai = _modes(st, c, nf, K, W, inv_L, wrong != "no-detrend")
        p0 = ar * ar
        p1 = ai * ai
        p = p0 + p1                                             # [nf, K, n]
        store = s == 0 and wrong != "add-at-0"
        st["pxx"][:] = p.reshape(nf * K, n) if store else st["pxx"] + p.reshape(nf * K, n)
        if ref is not None:
            rr, ri = _modes(ref, c, nf, K, W, inv_L, wrong != "no-detrend")
            if ref_row >= 0:
                row = (ref_row + 1) % n if wrong == "ref-row+1" else ref_row
                rr, ri = rr[:, :, row:row + 1], ri[:, :, row:row + 1]
            elif wrong == "ref-row+1":
                rr, ri = np.roll(rr, -1, axis=2), np.roll(ri, -1, axis=2)
            if ref_field >= 0:
                rr, ri = rr[ref_field:ref_field + 1], ri[ref_field:ref_field + 1]
            a = ar * rr
            b = ai * ri
            cc = ai * rr
            d = ar * ri
            cr = a + b
            ci = (d - cc) if wrong == "conj" else (cc - d)
            st["cxr_re"][:] = cr.reshape(nf * K, n) if store else st["cxr_re"] + cr.reshape(nf * K, n)
            st["cxr_im"][:] = ci.reshape(nf * K, n) if store else st["cxr_im"] + ci.reshape(nf * K, n)
        if track is not None and "seg_power" in st and s < st["seg_power"].shape[0]:
            for i, row in enumerate(track):
                st["seg_power"][s, i] = p[:, :, int(row)]
    st["window"][2] = s + 1
    return st


def step(st, x, t: int, max_steps: int, tw, W, stride: int, H: int, x_step: int = 0, ref=None, ref_row: int = -1, ref_field: int = -1,
         track=None, wrong: Optional[str] = None):
    """One call of g4c_rollout_welch: accumulate, then close."""
    accumulate(st, x, t, max_steps, tw, stride, H, x_step, wrong=wrong)
    return close(st, t, max_steps, np.asarray(tw).shape[0], W, stride, H, ref=ref, ref_row=ref_row, ref_field=ref_field, track=track, wrong=wrong)


def table(L: int, bins, taper: str = "hann"):
    """(tw [L, K, 2], w [L]) of the integer bins of a segment: tw[q, k] = (w_q cos th, -w_q sin th), th = 2 pi ((b q) mod L) / L; "hann" is
    the periodic window 0.5 - 0.5 cos(2 pi q / L), "rect" is 1."""
    q = np.arange(L, dtype=np.int64)
    b = np.asarray(list(bins), dtype=np.int64)
    th = 2.0 * np.pi * ((q[:, None] * b[None, :]) % L).astype(F64) / L
    w = np.ones(L, dtype=F64) if taper == "rect" else 0.5 - 0.5 * np.cos(2.0 * np.pi * q.astype(F64) / L)
    return np.stack([w[:, None] * np.cos(th), -(w[:, None] * np.sin(th))], axis=-1), w


def weights(tw) -> np.ndarray:
    """W [K, 2] = Σ_q tw[q], the rows added one by one in order."""
    tw = np.asarray(tw, dtype=F64)
    W = np.zeros(tw.shape[1:], dtype=F64)
    for q in range(tw.shape[0]):
        W = W + tw[q]
    return W


def lattice_origin(start: int, stride: int, first: int) -> int:
    behind = max(first - start, 0)
    return start + -(-behind // stride) * stride


def run(xs, max_steps: int, tw, H: int, start: int = 0, stride: int = 1, first: int = 0, x_step: int = 0, steps: Optional[int] = None,
        W=None, reference=None, track=None, max_segments: int = 0, wrong: Optional[str] = None, fill: float = 0.0):
    """The state after the steps first, first + 1, ..., with the origin a `Rollout` sets.  x_step = 0: xs[i] [n, nf] is the sample of step
    first + i; x_step = nf: xs [n, >= nf max_steps] holds every step's columns and `steps` of them are taken.  reference: None,
    (row, field) — this state's own sums, either may be -1 — or ("target", xt): a second state over the columns of xt [n, >= nf
    max_steps], accumulated first at every step; then (state, target's state) is returned."""
    tw = np.asarray(tw, dtype=F64)
    W = weights(tw) if W is None else np.asarray(W, dtype=F64)
    origin = lattice_origin(start, stride, first)
    if x_step:
        x0, nf, count = np.asarray(xs), x_step, int(steps)
    else:
        x0, nf, count = np.asarray(xs[0]), int(np.asarray(xs[0]).shape[1]), len(xs)
    n, K = x0.shape[0], tw.shape[1]
    sets = PARITY_SETS if wrong == "parity" else 2
    target = reference is not None and reference[0] == "target"
    st = new_state(n, nf, K, origin, reference is not None, 0 if track is None else len(track), max_segments, fill=fill, sets=sets)
    tg = new_state(n, nf, K, origin, fill=fill, sets=sets) if target else None
    for i in range(count):
        t = first + i
        if target:
            step(tg, reference[1], t, max_steps, tw, W, stride, H, x_step=nf, wrong=wrong)
            step(st, xs if x_step else xs[i], t, max_steps, tw, W, stride, H, x_step, ref=tg, track=track, wrong=wrong)
        elif reference is not None:
            step(st, xs if x_step else xs[i], t, max_steps, tw, W, stride, H, x_step, ref=st, ref_row=reference[0], ref_field=reference[1],
                 track=track, wrong=wrong)
        else:
            step(st, xs if x_step else xs[i], t, max_steps, tw, W, stride, H, x_step, track=track, wrong=wrong)
    return (st, tg) if target else st


# ------------------------------------------------------------------ derived quantities (those of `RolloutWelch`, restated)
def power(st, w, K: int) -> np.ndarray:
    """[nf, K, n]: pxx / (segments S²), S = Σ w."""
    S = float(np.sum(np.asarray(w, dtype=F64)))
    return st["pxx"].reshape(-1, K, st["pxx"].shape[1]) / (int(st["window"][2]) * S * S)


def cross(st, w, K: int) -> np.ndarray:
    """[nf, K, n] complex: (cxr_re + i cxr_im) / (segments S²) — the average of X conj(R)."""
    S = float(np.sum(np.asarray(w, dtype=F64)))
    c = st["cxr_re"] + 1j * st["cxr_im"]
    return c.reshape(-1, K, c.shape[1]) / (int(st["window"][2]) * S * S)


# ------------------------------------------------------------------ checkers
def same(got, ref: np.ndarray, what: str = "") -> None:
    """Bit for bit: `got` (a torch tensor on any device, or an array) holds exactly the fp64 values of `ref` (NaN equals NaN)."""
    g = got.detach().cpu().numpy() if hasattr(got, "detach") else np.asarray(got)
    assert g.dtype == F64 and tuple(g.shape) == tuple(ref.shape), f"{what}: {g.dtype} {g.shape} vs float64 {ref.shape}"
    bad = ~((g == ref) | (np.isnan(g) & np.isnan(ref)))
    if bad.any():
        pos = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at {list(pos)}: got {float(g[pos])!r} "
                             f"want {float(ref[pos])!r}")


def same_state(got: Dict[str, object], ref: Dict[str, np.ndarray], what: str = "") -> None:
    """Every array of `ref` against `got` (of the sets, the first two: what the device holds), and the window as integers."""
    K = ref["re"].shape[0] // ref["pivot"].shape[0]
    sets = ref["pivot"].shape[0] // (ref["pxx"].shape[0] // K)
    for k in names(ref) + (("seg_power",) if "seg_power" in ref else ()):
        want = ref[k][:ref[k].shape[0] * 2 // sets] if k in SETS else ref[k]
        same(got[k], want, f"{what}, {k}")
    w = [int(v) for v in (got["window"].tolist() if hasattr(got["window"], "tolist") else got["window"])]
    assert w == [int(v) for v in ref["window"]], f"{what}, window: {w} vs {ref['window'].tolist()}"


def rejects(check, *args, **kw) -> bool:
    """True when the checker raises AssertionError (negative controls)."""
    try:
        check(*args, **kw)
    except AssertionError:
        return True
    return False
