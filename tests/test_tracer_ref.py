"""The numpy restatement of the tracers' rule (tests/tracer_ref.py), checked against flows whose pathlines are known: a uniform flow
moves every particle by n dt U, a solid-body rotation — a linear field, which the fit reproduces — makes Heun's radius grow by exactly
sqrt(1 + (w dt)^4 / 4) a step; the release steps, the three stopping rules and the freezing.  Host only."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sampler_ref as R          # noqa: E402
import tracer_ref as T           # noqa: E402

F32, F64 = np.float32, np.float64
EPS = 2.0 ** -24


def seeds_in(p, dim, lo=0.3, hi=0.7, seed=0):
    return (lo + (hi - lo) * np.random.default_rng(50 + dim + seed).random((p, dim))).astype(F32)


@pytest.mark.parametrize("dim, k", [(2, 6), (3, 10)])
@pytest.mark.parametrize("scheme", [T.EULER, T.HEUN])
def test_a_uniform_flow_moves_every_particle_by_n_dt_u(dim, k, scheme):
    pos, n, dt = R.cloud(1000, dim), 12, 0.01
    U = np.array([1.0, -0.5, 0.25][:dim], F32)
    x = np.tile(U, (len(pos), 1)).astype(F32)
    q0 = seeds_in(33, dim)
    p = T.params(dim, dt, k, scheme=scheme)
    q, status, stopped = q0.copy(), np.zeros(33, np.uint8), np.full(33, -1, np.int32)
    sum_c = 0.0
    for t in range(n):
        aux = []
        q, status, stopped, _ = T.advance(pos, q, status, stopped, np.zeros(33, np.int32), x, x, t, p, aux=aux)
        for tab in (aux[0].first, aux[0].second):
            if tab is not None:
                sum_c = max(sum_c, float(np.abs(tab.c32.astype(F64)).sum(1).max()))
    assert (status == T.MOVING).all() and (stopped == -1).all()
    want = q0.astype(F64) + n * F64(F32(dt)) * U.astype(F64)
    # per step: the fp32 sum of a stage errs by (k + 3) 2^-24 Σ|c_j| |U| (sampler_ref.bound32), times dt — its margin covers the rounding
    # of dt v, of v0 + v1 and of scale, shift —, and the stored position is rounded once: half an ulp of |q|
    allowed = n * (k + 3) * EPS * sum_c * np.abs(U).astype(F64) * dt + n * EPS * np.abs(want)
    ratio = R.within(q, want, allowed, "uniform flow")
    print(f"uniform flow dim {dim} scheme {scheme}: measured / allowed {ratio:.3f}")


def rotation(pos, centre, w):
    d = pos.astype(F64) - centre
    return np.stack([-w * d[:, 1], w * d[:, 0]], axis=1).astype(F32)


def test_heun_radius_grows_by_its_known_factor_in_a_solid_body_rotation():
    pos, n, dt, w, k = R.cloud(1000, 2), 20, 0.1, 4.0, 6
    centre = np.array([0.5, 0.5])
    x = rotation(pos, centre, w)
    ang = np.linspace(0, 2 * np.pi, 17, endpoint=False)
    q0 = (centre + 0.2 * np.stack([np.cos(ang), np.sin(ang)], 1)).astype(F32)
    p = T.params(2, dt, k, scheme=T.HEUN)
    q, status, stopped = q0.copy(), np.zeros(17, np.uint8), np.full(17, -1, np.int32)
    a = w * F64(F32(dt))
    g = np.sqrt(1.0 + a ** 4 / 4.0)
    delta = 0.0
    for t in range(n):
        aux = []
        q, status, stopped, _ = T.advance(pos, q, status, stopped, np.zeros(17, np.int32), x, x, t, p, aux=aux)
        e = 0.0
        for tab in (aux[0].first, aux[0].second):
            # a stage's velocity against the linear field: k products, k - 1 adds, k coefficient roundings, margin 4 — (2k + 3) 2^-24 Σ|c_j x_j|;
            # and the node values themselves are the field rounded to fp32: 2^-24 Σ|c_j x_j| more
            mag = np.abs(tab.c32.astype(F64))[:, :, None] * np.abs(tab.x.astype(F64))[tab.idx]          # [M, k, dim]
            e += float(((2 * k + 4) * EPS * mag.sum(1)).max())
        # the position: dt (e0 + e1) through both stages (the second sees the first's error times w dt < 1), four roundings of |q| <= 1
        delta = max(delta, float(F32(dt)) * e * (1 + a) + 4 * EPS)
    assert (status == T.MOVING).all()
    radius = np.sqrt(((q.astype(F64) - centre) ** 2).sum(1))
    r0 = np.sqrt(((q0.astype(F64) - centre) ** 2).sum(1))
    # |q_n - exact_n| <= Σ_i g^(n - i) delta_i, per component; the radius errs by at most sqrt(2) of it
    allowed = np.sqrt(2.0) * n * g ** n * delta
    ratio = R.within(radius, r0 * g ** n, allowed, "Heun radius")
    print(f"rotation: growth {g ** n:.9f}, measured / allowed {ratio:.3f}")
    assert g ** n - 1 > 20 * allowed / r0.min()          # (the growth itself is far above the bound: the test can tell g from 1)
    # and the angle advanced by n atan(a / (1 - a^2 / 2))
    turn = n * np.arctan2(a, 1 - a * a / 2)
    d0, d1 = q0.astype(F64) - centre, q.astype(F64) - centre
    got = np.arctan2(d0[:, 0] * d1[:, 1] - d0[:, 1] * d1[:, 0], (d0 * d1).sum(1))
    assert np.abs(np.angle(np.exp(1j * (got - turn)))).max() <= allowed / r0.min()


def test_release_steps_hold_a_particle_at_its_seed():
    pos = R.cloud(65, 2)
    x = np.tile(np.array([1.0, 0.0], F32), (65, 1))
    q0 = seeds_in(4, 2)
    release = np.array([0, 2, 5, 9], np.int32)
    p = T.params(2, 0.01, 6, scheme=T.EULER)
    series, q, status, stopped = T.run(pos, q0, release, [x] * 8, p)
    assert series.shape == (7, 4, 2)
    for i, rel in enumerate(release):
        for t in range(7):
            moved = max(t + 1 - int(rel), 0)
            assert (series[t, i, 1] == q0[i, 1]) and abs(float(series[t, i, 0]) - float(q0[i, 0]) - moved * 0.01) < 1e-6, (i, t)
            if moved == 0:
                assert (series[t, i] == q0[i]).all()
    assert status.tolist() == [1, 1, 1, 0] and (stopped == -1).all()


def test_the_stopping_rules_freeze_a_particle_with_their_status_and_step():
    pos = R.cloud(65, 2)
    x = np.tile(np.array([1.0, 0.0], F32), (65, 1))
    q0 = np.array([[0.50, 0.5], [0.58, 0.5], [0.5, 3.0], [0.5, 0.4], [0.55, 0.45]], F32)
    p = T.params(2, 0.01, 6, scheme=T.HEUN, box_lo=[-np.inf, -np.inf], box_hi=[0.6, np.inf], max_distance=1.0)
    q, status, stopped = q0.copy(), np.zeros(5, np.uint8), np.full(5, -1, np.int32)
    release = np.zeros(5, np.int32)
    history = []
    for t in range(9):
        if t == 4:
            q[3, 0] = np.nan          # planted
        q, status, stopped, vel = T.advance(pos, q, status, stopped, release, x, x, t, p)
        history.append(q.copy())
    # particle 1 crosses x = 0.6 in its third step (0.58 -> 0.59 -> 0.60 -> 0.61: the stored position is outside) and stays there
    assert status.tolist() == [T.MOVING, T.LEFT, T.FAR, T.NONFINITE, T.LEFT]
    assert stopped[0] == -1 and stopped[2] == 0 and stopped[3] == 4 and stopped[1] in (1, 2) and stopped[4] in (4, 5)
    assert history[-1][1, 0] > 0.6 and (history[-1][1] == history[int(stopped[1])][1]).all()
    assert (history[-1][2] == q0[2]).all()                       # too far: never moved
    assert np.isnan(history[-1][3, 0]) and history[-1][3, 1] == history[3][3, 1]
    for i in (1, 2, 4):                                          # frozen particles never move again
        for t in range(int(stopped[i]), 9):
            assert (history[t][i] == history[int(stopped[i])][i]).all(), (i, t)
    assert np.isnan(vel[1:]).all() and not np.isnan(vel[0]).any()          # the last launch moved particle 0 only
    # a step index out of range moves nothing
    p.max_steps = 9
    q2, s2, st2, v2 = T.advance(pos, q, status, stopped, release, x, x, 9, p)
    assert np.array_equal(q2, q, equal_nan=True) and (s2 == status).all() and (st2 == stopped).all() and np.isnan(v2).all()
    q2, s2, st2, v2 = T.advance(pos, q, status, stopped, release, x, x, -1, p)
    assert np.array_equal(q2, q, equal_nan=True) and (s2 == status).all()


def test_a_predictor_that_leaves_the_finite_range_freezes_the_particle_where_it_was():
    pos = R.cloud(65, 2)
    x = np.tile(np.array([3e38, 0.0], F32), (65, 1))
    q0 = np.array([[0.5, 0.5]], F32)
    q, status, stopped, vel = T.advance(pos, q0, np.zeros(1, np.uint8), np.full(1, -1, np.int32), np.zeros(1, np.int32), x, x, 3,
                                        T.params(2, 10.0, 6, scheme=T.HEUN))
    assert status[0] == T.NONFINITE and stopped[0] == 3 and (q == q0).all() and vel[0, 0] == F32(3e38)
    # Euler stores the position it formed; the next launch finds it not finite
    q, status, stopped, _ = T.advance(pos, q0, np.zeros(1, np.uint8), np.full(1, -1, np.int32), np.zeros(1, np.int32), x, None, 3,
                                      T.params(2, 10.0, 6, scheme=T.EULER))
    assert status[0] == T.MOVING and np.isinf(q[0, 0])
    q, status, stopped, _ = T.advance(pos, q, status, stopped, np.zeros(1, np.int32), x, None, 4, T.params(2, 10.0, 6, scheme=T.EULER))
    assert status[0] == T.NONFINITE and stopped[0] == 4
