"""Test-only fp64 restatement of g4c_rollout_spectrum (csrc/rollout_spectrum.hip) as a plain numpy loop over steps in time order, and
the checkers its tests share.  Nothing here calls graphs4cfd_amd.

State (all fp64, plane-major, planes first): pivot [nf, n], sum [nf, n], re [nf K, n], im [nf K, n] — plane f K + k — and window =
[origin, last] (integers).  The table tw [samples, K, 2] fp64 is an input (any values).

One call, at step index t, with the sample x_f = x[:, x_step t + f] widened to fp64 (x_step = 0: x is the prediction [n, nf]; x_step =
nf: x holds every step's columns) and j = (t - origin) / stride:
  accumulated iff n > 0, 0 <= t < max_steps, t >= origin, (t - origin) % stride == 0 and j < samples; otherwise NOTHING changes;
  j == 0: pivot = x, sum = re = im = 0 — stored, whatever the state held;
  later:  d = x - pivot; sum += d; re[f K + k] += d_f * tw[j, k, 0]; im[f K + k] += d_f * tw[j, k, 1] (numpy rounds the product to
          fp64, then adds: two roundings, no fused multiply-add);
  and last = t.
Each accumulator gets one add per accumulated step, in time order: the device's bits must equal these exactly, on any data and table.

`wrong=` names ONE deliberate mistake for the negative controls: "no-pivot" (d = x), "plane-order" (plane k nf + f), "im-sign" (im
-= d tw[j, k, 1]), "window+1" (the lattice shifted by one step), "row+1" (table row j + 1, wrapped), "x-step" (with x_step = nf: the
columns of step t + 1)."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

F64 = np.float64
NAMES = ("pivot", "sum", "re", "im")
WRONG = ("no-pivot", "plane-order", "im-sign", "window+1", "row+1", "x-step")


def new_state(n: int, nf: int, K: int, origin: int = 0, fill: float = 0.0) -> Dict[str, np.ndarray]:
    st = {k: np.full((nf * K if k in ("re", "im") else nf, n), fill, dtype=F64) for k in NAMES}
    st["window"] = np.array([origin, -1], dtype=np.int64)
    return st


def copy_state(st: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    return {k: v.copy() for k, v in st.items()}


def on_window(t: int, origin: int, stride: int, max_steps: int, samples: int) -> bool:
    return 0 <= t < max_steps and t >= origin and (t - origin) % stride == 0 and (t - origin) // stride < samples


def sample(x, nf: int, t: int, x_step: int = 0, wrong: Optional[str] = None) -> np.ndarray:
    """x [nf, n] in fp64."""
    a = np.asarray(x, dtype=np.float32)
    tt = t + 1 if (wrong == "x-step" and x_step) else t
    return np.ascontiguousarray(a[:, x_step * tt:x_step * tt + nf].astype(F64).T)


def accumulate(st: Dict[str, np.ndarray], x, t: int, max_steps: int, tw, stride: int = 1, x_step: int = 0,
               wrong: Optional[str] = None) -> Dict[str, np.ndarray]:
    """One call at step index t: the new state (a copy; `st` is left as it was)."""
    assert wrong is None or wrong in WRONG, wrong
    tw = np.asarray(tw, dtype=F64)
    samples, K = tw.shape[0], tw.shape[1]
    out = copy_state(st)
    nf, n = st["pivot"].shape
    assert st["re"].shape == (nf * K, n) and x_step in (0, nf)
    origin = int(st["window"][0]) + (1 if wrong == "window+1" else 0)
    if n == 0 or not on_window(t, origin, stride, max_steps, samples):
        return out
    j = (t - origin) // stride
    xs = sample(x, nf, t, x_step, wrong)
    if j == 0:
        out["pivot"][:] = xs
        out["sum"][:], out["re"][:], out["im"][:] = 0.0, 0.0, 0.0
    else:
        row = tw[(j + 1) % samples] if wrong == "row+1" else tw[j]
        d = xs if wrong == "no-pivot" else xs - out["pivot"]
        out["sum"] += d
        for f in range(nf):
            for k in range(K):
                p = k * nf + f if wrong == "plane-order" else f * K + k
                pr = d[f] * row[k, 0]
                pi = d[f] * row[k, 1]
                out["re"][p] += pr
                if wrong == "im-sign":
                    out["im"][p] -= pi
                else:
                    out["im"][p] += pi
    out["window"][1] = t
    return out


def run(xs, max_steps: int, tw, start: int = 0, stride: int = 1, first: int = 0, x_step: int = 0, steps: Optional[int] = None,
        wrong: Optional[str] = None) -> Dict[str, np.ndarray]:
    """The state after the steps first, first + 1, ..., with the origin a `Rollout` sets: the first step of the lattice start, start +
    stride, ... at or after `first`.  x_step = 0: xs[i] [n, nf] is the sample of step first + i; x_step = nf: xs [n, >= nf max_steps]
    holds every step's columns and `steps` of them are taken."""
    behind = max(first - start, 0)
    origin = start + -(-behind // stride) * stride
    if x_step:
        x0, nf, count = np.asarray(xs), x_step, int(steps)
    else:
        x0, nf, count = np.asarray(xs[0]), int(np.asarray(xs[0]).shape[1]), len(xs)
    st = new_state(x0.shape[0], nf, int(np.asarray(tw).shape[1]), origin)
    for i in range(count):
        st = accumulate(st, xs if x_step else xs[i], first + i, max_steps, tw, stride, x_step, wrong=wrong)
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
