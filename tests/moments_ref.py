"""Test-only fp64 restatement of g4c_rollout_moments (csrc/rollout_moments.hip) as a plain numpy loop over steps in time order, and the
checkers its tests share.  Nothing here calls graphs4cfd_amd.

State (all fp64, plane-major, planes first): pivot [nf, n], sum [nf, n], sum2 [nf (nf + 1) / 2, n] — the pairs f <= g in the order
(0,0), (0,1), ..., (0,nf-1), (1,1), ... — lo [nf, n], hi [nf, n], and window = [origin, last] (integers).

One call, at step index t, with the sample x = pred (or pred - sub[:, nf t : nf (t + 1)], both widened to fp64 first):
  accumulated iff n > 0, 0 <= t < max_steps, t >= origin and (t - origin) % stride == 0; otherwise NOTHING changes;
  t == origin: pivot = lo = hi = x, sum = sum2 = 0 — stored, whatever the state held;
  later:       d = x - pivot; sum += d; sum2[fg] += d_f * d_g (numpy rounds the product to fp64, then adds: two roundings, no fused
               multiply-add); lo = minimum(lo, x); hi = maximum(hi, x) — numpy's NaN-propagating pair, not fmin / fmax: after a NaN
               sample lo and hi are NaN, as the sums are, until the origin is run through again (±Inf are ordinary values);
  and last = t.
Each accumulator gets one add per accumulated step, in time order: the device's bits must equal these exactly, on any data.

`wrong=` names ONE deliberate mistake for the negative controls: "pair-order" (sum2 in column-major pair order), "no-pivot" (d = x),
"window+1" (the lattice shifted by one step), "sub+1" (the target's columns of step t + 1)."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

F64 = np.float64
NAMES = ("pivot", "sum", "sum2", "lo", "hi")
WRONG = ("pair-order", "no-pivot", "window+1", "sub+1")


def pairs(nf: int, wrong: Optional[str] = None):
    """[(f, g)] in the order of sum2's planes."""
    if wrong == "pair-order":
        return [(f, g) for g in range(nf) for f in range(g + 1)]
    return [(f, g) for f in range(nf) for g in range(f, nf)]


def new_state(n: int, nf: int, origin: int = 0, fill: float = 0.0) -> Dict[str, np.ndarray]:
    st = {k: np.full((len(pairs(nf)) if k == "sum2" else nf, n), fill, dtype=F64) for k in NAMES}
    st["window"] = np.array([origin, -1], dtype=np.int64)
    return st


def copy_state(st: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    return {k: v.copy() for k, v in st.items()}


def on_window(t: int, origin: int, stride: int, max_steps: int) -> bool:
    return 0 <= t < max_steps and t >= origin and (t - origin) % stride == 0


def sample(pred, t: int, sub=None, wrong: Optional[str] = None) -> np.ndarray:
    """x [nf, n] in fp64."""
    p = np.asarray(pred, dtype=np.float32)
    nf = p.shape[1]
    x = p.astype(F64)
    if sub is not None:
        tt = t + 1 if wrong == "sub+1" else t
        x = x - np.asarray(sub, dtype=np.float32)[:, nf * tt:nf * (tt + 1)].astype(F64)
    return np.ascontiguousarray(x.T)


def accumulate(st: Dict[str, np.ndarray], pred, t: int, max_steps: int, stride: int = 1, sub=None,
               wrong: Optional[str] = None) -> Dict[str, np.ndarray]:
    """One call at step index t: the new state (a copy; `st` is left as it was)."""
    assert wrong is None or wrong in WRONG, wrong
    out = copy_state(st)
    origin = int(st["window"][0]) + (1 if wrong == "window+1" else 0)
    n, nf = int(np.asarray(pred).shape[0]), int(np.asarray(pred).shape[1])
    if n == 0 or not on_window(t, origin, stride, max_steps):
        return out
    x = sample(pred, t, sub, wrong)
    if t == origin:
        out["pivot"][:], out["lo"][:], out["hi"][:] = x, x, x
        out["sum"][:], out["sum2"][:] = 0.0, 0.0
    else:
        d = x if wrong == "no-pivot" else x - out["pivot"]
        out["sum"] += d
        for p, (f, g) in enumerate(pairs(nf, wrong)):
            prod = d[f] * d[g]
            out["sum2"][p] += prod
        out["lo"], out["hi"] = np.minimum(out["lo"], x), np.maximum(out["hi"], x)
    out["window"][1] = t
    return out


def run(samples, max_steps: int, start: int = 0, stride: int = 1, subs=None, first: int = 0) -> Dict[str, np.ndarray]:
    """The state after the steps first, first + 1, ... (samples[i] is the prediction of step first + i), with the origin a `Rollout`
    sets: the first step of the lattice start, start + stride, ... at or after `first`."""
    behind = max(first - start, 0)
    origin = start + -(-behind // stride) * stride
    p0 = np.asarray(samples[0])
    st = new_state(p0.shape[0], p0.shape[1], origin)
    for i, p in enumerate(samples):
        st = accumulate(st, p, first + i, max_steps, stride, subs)
    return st


def count(st: Dict[str, np.ndarray], stride: int) -> int:
    origin, last = (int(v) for v in st["window"])
    return (last - origin) // stride + 1 if last >= origin else 0


# ------------------------------------------------------------------ checkers
def same(got, ref: np.ndarray, what: str = "") -> None:
    """Bit for bit: `got` (a torch tensor on any device, or an array) holds exactly the fp64 values of `ref`."""
    g = got.detach().cpu().numpy() if hasattr(got, "detach") else np.asarray(got)
    assert g.dtype == F64 and tuple(g.shape) == tuple(ref.shape), f"{what}: {g.dtype} {g.shape} vs float64 {ref.shape}"
    bad = ~((g == ref) | (np.isnan(g) & np.isnan(ref)))
    if bad.any():
        pos = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ, first at {list(pos)}: got {float(g[pos])!r} "
                             f"want {float(ref[pos])!r}")


def same_state(got: Dict[str, object], ref: Dict[str, np.ndarray], what: str = "") -> None:
    for k in NAMES:
        same(got[k], ref[k], f"{what}, {k}")
    w = [int(v) for v in (got["window"].tolist() if hasattr(got["window"], "tolist") else got["window"])]
    assert w == [int(v) for v in ref["window"]], f"{what}, window: {w} vs {ref['window'].tolist()}"


def rejects(check, *args, **kw) -> bool:
    """True when the checker raises AssertionError (negative controls)."""
    try:
        check(*args, **kw)
    except AssertionError:
        return True
    return False
