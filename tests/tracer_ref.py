"""Test-only numpy restatement of csrc/tracer.hip (g4c_tracer_advance): the per-particle rule of include/g4c.h — skip rules, the
non-finite test, a stage (neighbours, tests/sampler_ref.py's fp64 coefficients and numpy.float32 sum, the physical velocity), the
too-far test, the Euler / Heun advance with every product rounded before its add, the box, the series' slot.  numpy only; the
neighbours come from `sampler_ref.nearest` (brute force) unless a table is handed in."""
from types import SimpleNamespace

import numpy as np

import sampler_ref as R

F32, F64 = np.float32, np.float64
WAITING, MOVING, LEFT, FAR, NONFINITE = 0, 1, 2, 3, 4
EULER, HEUN = 0, 1


def params(dim, dt, k, power=2, scheme=HEUN, vcol=None, scale=None, shift=None, box_lo=None, box_hi=None, max_distance=np.inf,
           max_steps=2 ** 31 - 1):
    one = lambda v, d: np.full(dim, d, F32) if v is None else np.asarray(v, F32).reshape(dim)          # noqa: E731
    return SimpleNamespace(dim=dim, dt=F32(dt), k=k, power=power, scheme=scheme, vcol=list(range(dim)) if vcol is None else list(vcol),
                           scale=one(scale, 1.0), shift=one(shift, 0.0), box_lo=one(box_lo, -np.inf), box_hi=one(box_hi, np.inf),
                           max_distance=F32(max_distance), max_steps=max_steps)


def stage(pos32, r, x, p, idx=None):
    """The physical velocity [M, dim] at the finite positions r [M, dim] from the node tensor x, the distance to the nearest node
    [M] and what the bounds need (idx, c64, c32, the gathered velocity columns)."""
    if idx is None:
        idx = R.nearest(pos32, r, p.k)
    c64, c32, distance, _, _ = R.coefficients(pos32, r, idx, p.power)
    xv = np.ascontiguousarray(np.asarray(x, F32)[:, p.vcol])
    u = R.apply32(xv, idx, c32)
    with np.errstate(all="ignore"):
        v = ((p.scale[None, :] * u).astype(F32) + p.shift[None, :]).astype(F32)
    return v, distance, SimpleNamespace(idx=idx, c64=c64, c32=c32, x=xv)


def advance(pos32, q, status, stopped, release, x0, x1, t, p, idx0=None, aux=None):
    """One launch at step t: returns (q, status, stopped, vel) — new arrays; `vel` is nan where the launch writes none.  `aux`, a
    list, receives the stages' tables (rows `moved`)."""
    q, status, stopped = np.array(q, F32), np.array(status, np.uint8), np.array(stopped, np.int32)
    vel = np.full(q.shape, np.nan, F32)
    if not 0 <= t < p.max_steps:
        return q, status, stopped, vel
    act = (t >= np.asarray(release)) & (status < LEFT)
    status[act] = MOVING
    fin = np.isfinite(q).all(1)
    bad = act & ~fin
    status[bad], stopped[bad] = NONFINITE, t
    go = np.flatnonzero(act & fin)
    if go.size == 0:
        return q, status, stopped, vel
    with np.errstate(all="ignore"):
        v0, dist, a0 = stage(pos32, q[go], x0, p, None if idx0 is None else idx0[go])
        far = dist > p.max_distance
        status[go[far]], stopped[go[far]] = FAR, t
        go, v0, q0 = go[~far], v0[~far], q[go[~far]]
        vel[go] = v0
        qn = (q0 + (p.dt * v0).astype(F32)).astype(F32)
        ok = np.ones(go.size, bool)
        a1 = None
        if p.scheme == HEUN:
            ok = np.isfinite(qn).all(1)
            status[go[~ok]], stopped[go[~ok]] = NONFINITE, t
            if ok.any():
                v1, _, a1 = stage(pos32, qn[ok], x1, p)
                s = (v0[ok] + v1).astype(F32)
                qn[ok] = (q0[ok] + (F32(F32(0.5) * p.dt) * s).astype(F32)).astype(F32)
        moved = go[ok]
        q[moved] = qn[ok]
        inside = ((qn[ok] >= p.box_lo) & (qn[ok] <= p.box_hi)).all(1)
        status[moved[~inside]], stopped[moved[~inside]] = LEFT, t
    if aux is not None:
        aux.append(SimpleNamespace(rows=go, far=far, ok=ok, first=a0, second=a1, v0=v0))
    return q, status, stopped, vel


def run(pos32, seeds, release, fields, p, every=1, n=None):
    """n = len(fields) − 1 steps from the seeds: step t uses fields[t] (level t) and fields[t + 1].  Returns (series [slots, P, dim], q,
    status, stopped)."""
    n = len(fields) - 1 if n is None else n
    q, status, stopped = np.array(seeds, F32), np.zeros(len(seeds), np.uint8), np.full(len(seeds), -1, np.int32)
    series = []
    for t in range(n):
        q, status, stopped, _ = advance(pos32, q, status, stopped, release, fields[t], fields[t + 1], t, p)
        if R.slot_of(t, every, n // every if every else 0) is not None:
            series.append(q.copy())
    return np.stack(series) if series else np.zeros((0,) + q.shape, F32), q, status, stopped
