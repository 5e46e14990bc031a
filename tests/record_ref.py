"""Test-only fp64 restatement of ONE call of g4c_rollout_advance_record (csrc/rollout_record.hip) in plain torch on the host, and the
checkers its tests share.  Nothing here calls graphs4cfd_amd: inputs are the tensors a launch read and the step index it found,
outputs are what it must leave — the new field, the snapshot buffer, the probe buffer, `stats`, the new step index.

Records of step t (0-based), for 0 <= t < max_steps and a mesh of at least one node; nothing otherwise:
  snapshots   every = k > 0 keeps the steps with (t + 1) % k == 0 in slot (t + 1) // k - 1, while the slot exists;
  probes      probe_out[t] = pred[probe_rows] (a row outside the mesh is left as it was);
  statistics  with y = target[:, nf t : nf (t + 1)] and d = pred - y in fp64, per field: [sum d^2, sum |d|, max |d|, sum y, sum y^2,
              sum |d| over the rows of `mask`] — stats[t] is replaced.  Non-finite samples: the sums follow IEEE, max |d| is NaN when
              |d| is NaN at any node (torch's max propagates), and a row outside the mask contributes nothing whatever it holds.

Two ways of comparing, as in oracle/grad_ref.py: `same` (bit for bit — data movement on any data, every statistic on small integers,
whose sums are exact in fp64 in any order, and max |d| on any data: one rounding of d on each side) and `stats_close` (the five sums
on float data: |got - ref| <= 2 (n + 4) 2^-53 sum|terms|, the bound of an n-term fp64 sum of terms each rounded once, n = n_nodes).

`wrong=` names ONE deliberate mistake for the negative controls: "slot+1" (snapshot slot off by one), "keep-t" (the kept step taken
as t % every == 0), "probe+1" (probe row + 1), "target+1" (target columns of step t + 1), "mask-inverted", "abs-for-sq" (sum |d| in
place of sum d^2)."""
from __future__ import annotations

from typing import Dict, Optional

import torch

Tensor = torch.Tensor
F64 = torch.float64
SQ_ERR, ABS_ERR, MAX_ABS_ERR, TGT_SUM, TGT_SQ_SUM, ABS_ERR_MASK, NSTAT = range(7)        # G4C_REC_* of include/g4c.h
SUMS = (SQ_ERR, ABS_ERR, TGT_SUM, TGT_SQ_SUM, ABS_ERR_MASK)
NAMES = ("sum d^2", "sum |d|", "max |d|", "sum y", "sum y^2", "masked sum |d|")
U64 = 2.0 ** -53
WRONG = ("slot+1", "keep-t", "probe+1", "target+1", "mask-inverted", "abs-for-sq")


def _f64(x: Optional[Tensor]) -> Optional[Tensor]:
    return None if x is None else x.detach().to("cpu", F64)


def step_stats(pred: Tensor, target: Tensor, t: int, mask: Optional[Tensor], wrong: Optional[str] = None):
    """(stats [nf, NSTAT], sum|terms| [nf, NSTAT]) of step t; both fp64.  The second is what `stats_close` scales its bound with."""
    p, nf = _f64(pred), int(pred.size(1))
    tt = t + 1 if wrong == "target+1" else t
    y = _f64(target)[:, nf * tt:nf * (tt + 1)]
    m = torch.zeros(p.size(0), dtype=torch.bool) if mask is None else mask.detach().cpu() != 0
    if wrong == "mask-inverted":
        m = ~m
    d = p - y
    ad = d.abs()
    s = torch.zeros((nf, NSTAT), dtype=F64)
    s[:, SQ_ERR] = (ad if wrong == "abs-for-sq" else d * d).sum(0)
    s[:, ABS_ERR] = ad.sum(0)
    s[:, MAX_ABS_ERR] = ad.max(0).values if p.size(0) else 0.0
    s[:, TGT_SUM] = y.sum(0)
    s[:, TGT_SQ_SUM] = (y * y).sum(0)
    s[:, ABS_ERR_MASK] = torch.where(m[:, None], ad, torch.zeros_like(ad)).sum(0)          # the mask selects: never ad * m
    a = s.clone()
    a[:, TGT_SUM] = y.abs().sum(0)
    return s, a


def advance_record(field: Tensor, pred: Tensor, t: int, max_steps: int, *, snap: Optional[Tensor] = None, every: int = 0,
                   probe_rows: Optional[Tensor] = None, probe_out: Optional[Tensor] = None, target: Optional[Tensor] = None,
                   mask: Optional[Tensor] = None, stats: Optional[Tensor] = None, wrong: Optional[str] = None) -> Dict[str, object]:
    """One call: {"field", "snap", "probe_out", "stats", "step"} — fp64 host copies; a buffer that was not given stays None."""
    assert wrong is None or wrong in WRONG, wrong
    f, p = _f64(field), _f64(pred)
    n, nf = int(p.size(0)), int(p.size(1))
    out = {"field": torch.cat((f[:, nf:], p), 1), "snap": _f64(snap), "probe_out": _f64(probe_out), "stats": _f64(stats), "step": t + 1}
    for k in ("snap", "probe_out", "stats"):
        if out[k] is not None:
            out[k] = out[k].clone()
    if not (0 <= t < max_steps) or n == 0:
        return out
    if snap is not None and every > 0 and ((t if wrong == "keep-t" else t + 1) % every == 0):
        slot = (t + 1) // every - 1 + (1 if wrong == "slot+1" else 0)
        if 0 <= slot < int(snap.size(0)):
            out["snap"][slot] = p
    if probe_rows is not None:
        rows = probe_rows.detach().cpu().long() + (1 if wrong == "probe+1" else 0)
        ok = (rows >= 0) & (rows < n)
        out["probe_out"][t, ok] = p[rows[ok]]
    if target is not None:
        out["stats"][t] = step_stats(pred, target, t, mask, wrong)[0]
    return out


# ------------------------------------------------------------------ checkers
def same(got: Tensor, ref: Tensor, what: str = "") -> None:
    """Bit for bit: `got` (any dtype, any device) holds exactly the fp64 values of `ref`."""
    g = got.detach().to("cpu", F64)
    assert tuple(g.shape) == tuple(ref.shape), f"{what}: shape {tuple(g.shape)} vs {tuple(ref.shape)}"
    bad = ~((g == ref) | (g.isnan() & ref.isnan()))
    if bool(bad.any()):
        pos = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, first at {list(pos)}: got {float(g[pos])!r} "
                             f"want {float(ref[pos])!r}")


def stats_close(got: Tensor, ref: Tensor, absref: Tensor, n: int, what: str = "") -> float:
    """One step's statistics [nf, NSTAT] on float data: max |d| bit for bit, the five sums within 2 (n + 4) 2^-53 sum|terms|.
    Returns (and prints) the largest measured / allowed ratio."""
    g = got.detach().to("cpu", F64)
    assert tuple(g.shape) == tuple(ref.shape) == tuple(absref.shape), f"{what}: shapes {g.shape} {ref.shape} {absref.shape}"
    same(g[:, MAX_ABS_ERR], ref[:, MAX_ABS_ERR], f"{what}, {NAMES[MAX_ABS_ERR]}")
    worst = 0.0
    for k in SUMS:
        err = (g[:, k] - ref[:, k]).abs()
        allow = 2.0 * (n + 4) * U64 * absref[:, k]
        over = ~(err <= allow)
        if bool(over.any()):
            f = int(over.nonzero()[0])
            raise AssertionError(f"{what}, {NAMES[k]}, field {f}: |diff| {float(err[f]):.3e} allowed {float(allow[f]):.3e} "
                                 f"(got {float(g[f, k])!r} want {float(ref[f, k])!r})")
        if err.numel():
            worst = max(worst, float((err / allow.clamp_min(1e-300)).max()))
    print(f"  {what}: n {n}, max measured/allowed {worst:.3e}")
    return worst


def rejects(check, *args, **kw) -> bool:
    """True when the checker raises AssertionError (negative controls)."""
    try:
        check(*args, **kw)
    except AssertionError:
        return True
    return False
