"""g4c_sample_weights and g4c_sample_points (csrc/point_sample.hip) through ops.sample_* and `gfd.PointSampler` against the numpy
restatement of tests/sampler_ref.py.

Weights: the neighbour table is the device's (the search is pinned by its own tests); the coefficients are compared with the fp64
restatement within 2^-23 max_j |c_ref,j| per point (half an ulp of the one rounding to fp32 and a margin of the same size;
tests/test_sampler_ref.py asserts that no point of these clouds sits near the degeneracy threshold, so the flags are exact), the
distance within one ulp of fp32.  Apply: `cur` is bit for bit the restatement's numpy.float32 loop and within (k + 3) 2^-24 Σ|c x| of
its fp64 form; every output lives in a guard arena (tests/footprint.py) and every input is frozen."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

import sampler_ref as R                                  # noqa: E402
from footprint import assert_footprint, flat_arena, frozen     # noqa: E402
import graphs4cfd_amd as gfd                             # noqa: E402
from graphs4cfd_amd import _lib, ops, synthetic as S     # noqa: E402

DEV = torch.device("cuda", 0)
F32, F64, I32, U8 = torch.float32, torch.float64, torch.int32, torch.uint8
SENT, USENT, PAD = -7777.0, 77, 64
RATIOS = {}          # bound -> the largest measured / allowed seen (printed by the last test; tests/SAMPLER_MEASURED.md)


def note(name, r):
    RATIOS[name] = max(RATIOS.get(name, 0.0), float(r))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def device_table(pos, q, k):
    """The device's neighbour table of the queries, j-major [k, P] int32 (and [P, k] on the host)."""
    if q.shape[0] == 0:
        return torch.empty((k, 0), dtype=I32, device=DEV), np.zeros((0, k), np.int32)
    nearest = S.knn_query_device(dev(pos), dev(q), k)
    return nearest.t().to(I32).contiguous(), nearest.cpu().numpy().astype(np.int32)


def run_weights(pos, q, idx_dev, power):
    """One guarded launch: (coef [P, k], distance, degenerate) as numpy."""
    k, p = int(idx_dev.size(0)), int(idx_dev.size(1))
    coef, coef_all = flat_arena(max(k * p, 1), F32, device=DEV)
    dist, dist_all = flat_arena(max(p, 1), F32, device=DEV)
    deg_all = torch.full((p + 2 * PAD,), USENT, dtype=U8, device=DEV)
    pos_d, q_d = dev(pos), dev(q)
    with frozen(pos_d, q_d, idx_dev, what="sample_weights"):
        out = ops.sample_weights(pos_d, q_d, idx_dev, power, out=(coef[:k * p].view(k, p), dist[:p], deg_all[PAD:PAD + p]))
        torch.cuda.synchronize(DEV)
    assert_footprint(coef_all, coef[:k * p], what="coef", inside=p > 0)
    assert_footprint(dist_all, dist[:p], what="distance", inside=p > 0)
    assert bool((deg_all[:PAD] == USENT).all()) and bool((deg_all[PAD + p:] == USENT).all())
    return out[0].t().cpu().numpy(), out[1].cpu().numpy(), out[2].cpu().numpy()


# ====================================================================== weights
@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("n", R.WEIGHT_CLOUDS)
def test_weights_match_the_restatement(n, dim):
    pos = R.cloud(n, dim)
    for p in (0, 1, 63, 64, 65, 257):
        q = R.queries(p, dim)
        for k in R.WEIGHT_K[dim]:
            idx_dev, idx = device_table(pos, q, k)
            for power in R.POWERS:
                what = f"n {n} dim {dim} P {p} k {k} power {power}"
                got_c, got_d, got_deg = run_weights(pos, q, idx_dev, power)
                c64, c32, dist, degen, ratio = R.coefficients(pos, q, idx, power)
                note("weights: |c - c_ref| / (2^-23 max_j |c_ref,j|)", R.within(got_c, c64, R.coefficient_bound(c64), what))
                ulps = R.ulps32(got_d, dist)
                note("distance: ulps of fp32 from the restatement / 1", ulps)
                assert ulps <= 1, what
                R.same(got_deg, degen, what + ", degenerate")
                assert degen.all() if k <= dim else not degen.any(), what


@pytest.mark.parametrize("dim", [2, 3])
def test_a_query_on_a_node_takes_that_nodes_row(dim):
    pos = R.cloud(1000, dim)
    rows = np.random.default_rng(3).choice(1000, 65, replace=False)
    q = R.queries(257, dim).copy()
    q[::4] = pos[rows]                                   # every fourth query is a node
    x = np.random.default_rng(4).standard_normal((1000, 5)).astype(np.float32)
    for k in (1, dim, R.WEIGHT_K[dim][2], 16):
        idx_dev, idx = device_table(pos, q, k)
        assert (idx[::4, 0] == rows).all()
        for power in R.POWERS:
            got_c, got_d, got_deg = run_weights(pos, q, idx_dev, power)
            c64, c32, dist, degen, ratio = R.coefficients(pos, q, idx, power)
            assert (got_c[::4, 0] == 1).all() and (got_c[::4, 1:] == 0).all() and (got_d[::4] == 0).all() and (got_deg[::4] == 0).all()
            R.same(got_deg, degen, "degenerate")
            R.within(got_c, c64, R.coefficient_bound(c64), f"dim {dim} k {k} power {power}")
            cur = ops.sample_points(dev(x), idx_dev, dev(np.ascontiguousarray(got_c.T)))
            R.same(cur[::4], x[rows], "the node's row")


def test_weights_negative_controls():
    pos, q = R.cloud(1000, 2), R.queries(257, 2)
    idx_dev, idx = device_table(pos, q, 6)
    got_c, got_d, got_deg = run_weights(pos, q, idx_dev, 2)
    c64 = R.coefficients(pos, q, idx, 2)[0]
    R.within(got_c, c64, R.coefficient_bound(c64))
    assert R.rejects(R.within, got_c, R.coefficients(pos, q, idx, 1)[0], R.coefficient_bound(c64))
    assert R.rejects(R.within, got_c, c64 * (1 + 2.0 ** -21), R.coefficient_bound(c64))


# ====================================================================== apply
def tables(n, p, k, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, n, (p, k)).astype(np.int32), rng.standard_normal((p, k)).astype(np.float32)


def run_apply(x_wide, col0, nf, idx, coef, step=None, every=0, series=None, max_steps=0):
    """One guarded launch on the columns col0 .. col0 + nf of x_wide: cur [P, nf] as numpy."""
    p, k = idx.shape
    cur, cur_all = flat_arena(max(p * nf, 1), F32, device=DEV)
    idx_d, coef_d = dev(idx.T), dev(coef.T)
    x = x_wide[:, col0:col0 + nf]
    with frozen(x_wide, idx_d, coef_d, step, what="sample_points"):
        out = ops.sample_points(x, idx_d, coef_d, cur[:p * nf].view(p, nf), step=step, every=every, series=series, max_steps=max_steps)
        torch.cuda.synchronize(DEV)
    assert_footprint(cur_all, cur[:p * nf], what="cur", inside=p > 0)
    return out.cpu().numpy()


@pytest.mark.parametrize("nf", [1, 2, 3, 5, 8, 37])
def test_the_apply_is_the_fp32_loop_bit_for_bit(nf):
    n = 1000
    for p, k in ((0, 6), (1, 1), (65, 6), (257, 10), (257, 16)):
        idx, coef = tables(n, p, k, 10 * nf + k)
        x_wide = torch.randn(n, nf + 5, generator=torch.Generator().manual_seed(nf)).to(DEV)
        x = x_wide[:, 2:2 + nf].cpu().numpy()
        got = run_apply(x_wide, 2, nf, idx, coef)
        R.same(got, R.apply32(x, idx, coef), f"nf {nf} P {p} k {k}")
        val, mag = R.apply64(x, idx, coef)
        note("apply: |cur - fp64| / ((k + 3) 2^-24 sum|c x|)", R.within(got, val, R.bound32(mag, k), f"nf {nf} P {p} k {k}"))
    # the contiguous case (the leading dimension equals nf), and a negative control: the neighbours in another order give other bits
    got = run_apply(x_wide[:, 2:2 + nf].contiguous(), 0, nf, idx, coef)
    R.same(got, R.apply32(x, idx, coef), "contiguous")
    assert R.rejects(R.same, got, R.apply32(x, idx[:, ::-1], coef[:, ::-1]))


BIG = 262_144 + 300          # 1024 workgroups of 256: 300 threads take a second point


@pytest.mark.parametrize("nf", [3, 5])
def test_many_points_take_several_per_thread(nf):
    n, k = 1000, 6
    idx, coef = tables(n, BIG, k, 99)
    x_wide = torch.randn(n, nf + 1, generator=torch.Generator().manual_seed(8)).to(DEV)
    x = x_wide[:, 1:1 + nf].cpu().numpy()
    got = run_apply(x_wide, 1, nf, idx, coef)
    R.same(got, R.apply32(x, idx, coef), f"P {BIG} nf {nf}")
    again = run_apply(x_wide, 1, nf, idx, coef)
    assert np.array_equal(got.view(np.int32), again.view(np.int32))          # two runs, the same bits


@pytest.mark.parametrize("every", [1, 3])
def test_the_series_follows_the_step_index(every):
    n, p, k, nf, steps = 257, 65, 6, 3, 7
    idx, coef = tables(n, p, k, 5)
    slots = steps // every
    series, series_all = flat_arena(slots * p * nf, F32, device=DEV)
    series3 = series.view(slots, p, nf)
    step = torch.zeros(2, dtype=I32, device=DEV)
    written = {}
    for t in (-1, 0, 1, 2, 3, 4, 5, 6, 7, 2):          # out of range on both sides, and step 2 once more: its slot is overwritten
        step[0], step[1] = t, 40 + t
        x_wide = torch.randn(n, nf, generator=torch.Generator().manual_seed(100 + t + len(written))).to(DEV)
        before = series_all.clone()
        got = run_apply(x_wide, 0, nf, idx, coef, step=step, every=every, series=series3, max_steps=steps)
        want = R.apply32(x_wide.cpu().numpy(), idx, coef)
        R.same(got, want, f"cur at step {t}")
        assert step.tolist() == [t, 40 + t]
        slot = R.slot_of(t, every, slots) if t < steps else None
        if slot is None:
            assert torch.equal(series_all.view(I32), before.view(I32)), f"step {t} is off the slots and wrote the series"
        else:
            written[slot] = want
            R.same(series3[slot], want, f"slot {slot} at step {t}")
            rest = [s for s in range(slots) if s != slot]
            assert torch.equal(series3[rest].view(I32), before[0, 4096:4096 + slots * p * nf].view(slots, p, nf)[rest].view(I32))
    assert sorted(written) == list(range(slots))
    assert_footprint(series_all, series, what="series")
    for slot, want in written.items():
        R.same(series3[slot], want, f"slot {slot} at the end")
    # without a series the step index is not needed; with one it is
    R.same(ops.sample_points(x_wide, dev(idx.T), dev(coef.T)), R.apply32(x_wide.cpu().numpy(), idx, coef), "no step")


def test_refusals_return_their_code_without_launching():
    lib = _lib.load()
    n, p, k, nf = 64, 32, 4, 3
    x, pos, q = torch.ones(n, nf, device=DEV), torch.rand(n, 2, device=DEV), torch.rand(p, 2, device=DEV)
    idx, coef_in = torch.zeros(k, p, dtype=I32, device=DEV), torch.ones(k, p, device=DEV)
    cur, series = torch.full((p, nf), SENT, device=DEV), torch.full((2, p, nf), SENT, device=DEV)
    coef, dist, deg = torch.full((k, p), SENT, device=DEV), torch.full((p,), SENT, device=DEV), torch.full((p,), USENT, dtype=U8, device=DEV)
    step = torch.zeros(2, dtype=I32, device=DEV)

    def points(n_nodes=n, n_points=p, xp=x.data_ptr(), **kw):
        d = _lib.g4c_sample_points_t(**dict(dict(idx=idx.data_ptr(), coef=coef_in.data_ptr(), k=k, nf=nf, x_ld=nf, cur=cur.data_ptr(),
                                                 step=step.data_ptr(), every=1, n_slots=2, max_steps=2, series=series.data_ptr()), **kw))
        rc = lib.g4c_sample_points(xp, C.byref(d), n_nodes, n_points, _lib.stream_handle(DEV))
        return rc, lib.g4c_last_error().decode()

    for kw, code, word in ((dict(k=17), _lib.EUNSUPPORTED, "k=17"), (dict(k=0), _lib.EINVAL, "bad sizes"), (dict(nf=0), _lib.EINVAL, "bad sizes"),
                           (dict(x_ld=2), _lib.EINVAL, "x_ld"), (dict(every=-1), _lib.EINVAL, "bad sizes"), (dict(max_steps=-1), _lib.EINVAL, "bad sizes"),
                           (dict(n_slots=-1), _lib.EINVAL, "bad sizes"), (dict(every=0), _lib.EINVAL, "every=0"), (dict(step=None), _lib.EINVAL, "step"),
                           (dict(cur=None), _lib.EINVAL, "null"), (dict(idx=None), _lib.EINVAL, "null"), (dict(coef=None), _lib.EINVAL, "null"),
                           (dict(n_nodes=3), _lib.EINVAL, "neighbours of"), (dict(n_nodes=-1), _lib.EINVAL, "bad sizes"),
                           (dict(n_points=-1), _lib.EINVAL, "bad sizes"), (dict(xp=None), _lib.EINVAL, "null")):
        args = {a: kw.pop(a) for a in ("n_nodes", "n_points", "xp") if a in kw}
        rc, msg = points(**args, **kw)
        assert rc == code and "g4c_sample_points" in msg and word in msg, (kw, args, rc, msg)
    assert points(n_points=0)[0] == _lib.OK and points(n_nodes=0, n_points=0)[0] == _lib.OK          # no points: nothing to do

    def weights(dim=2, power=2, kk=k, n_nodes=n, n_points=p, out=coef.data_ptr()):
        rc = lib.g4c_sample_weights(pos.data_ptr(), q.data_ptr(), idx.data_ptr(), dim, power, kk, n_nodes, n_points, out, dist.data_ptr(),
                                    deg.data_ptr(), _lib.stream_handle(DEV))
        return rc, lib.g4c_last_error().decode()

    for kw, code in ((dict(dim=4), _lib.EUNSUPPORTED), (dict(dim=1), _lib.EUNSUPPORTED), (dict(power=3), _lib.EINVAL), (dict(power=-1), _lib.EINVAL),
                     (dict(kk=17), _lib.EUNSUPPORTED), (dict(kk=0), _lib.EINVAL), (dict(n_nodes=3), _lib.EINVAL), (dict(n_nodes=-1), _lib.EINVAL),
                     (dict(n_points=-1), _lib.EINVAL), (dict(out=None), _lib.EINVAL)):
        rc, msg = weights(**kw)
        assert rc == code and "g4c_sample_weights" in msg, (kw, rc, msg)
    assert weights(n_points=0)[0] == _lib.OK and weights(n_nodes=0, n_points=0)[0] == _lib.OK
    torch.cuda.synchronize(DEV)
    for t, s in ((cur, SENT), (series, SENT), (coef, SENT), (dist, SENT), (deg, USENT)):
        assert bool((t == s).all())
    assert step.tolist() == [0, 0]
    with pytest.raises(NotImplementedError, match="dim=4"):          # the binding turns the code into the exception
        _lib.check(weights(dim=4)[0])


# ====================================================================== gfd.PointSampler
def cloud_graph(n, dim):
    return gfd.Graph(pos=dev(R.cloud(n, dim)), field=torch.zeros(n, 3, device=DEV))


@pytest.mark.parametrize("dim", [2, 3])
def test_point_sampler_reproduces_linear_fields(dim):
    g = cloud_graph(1000, dim)
    q = R.queries(257, dim)
    s = gfd.PointSampler(g, torch.from_numpy(q))                      # host points, default k and power
    k = {2: 6, 3: 10}[dim]
    assert s.k == k and s.power == 2 and s.n_points == 257 and s.shape is None and s.points.is_cuda
    assert tuple(s.idx.shape) == (257, k) and s.idx.dtype == I32 and tuple(s.coef.shape) == (257, k) and s.coef.stride() == (1, 257)
    assert s.distance.dtype == F32 and s.degenerate.dtype == torch.bool and not bool(s.degenerate.any())
    pos, idx = g.pos.cpu().numpy(), s.idx.cpu().numpy()
    c64, c32, dist, degen, ratio = R.coefficients(pos, q, idx, 2)
    R.within(s.coef, c64, R.coefficient_bound(c64), "PointSampler.coef")
    assert R.ulps32(s.distance, dist) <= 1
    # a linear field: the fp32 sample against the exact value — the apply's bound, the coefficients' rounding (2^-23 max|c| per
    # neighbour), the rounding of the node values to fp32 (2^-24 each), and the restatement's own fp64 identity error
    slope, const = np.random.default_rng(dim).standard_normal((dim, 3)), np.array([0.5, -1.0, 2.0])
    x64 = pos.astype(np.float64) @ slope + const
    x = x64.astype(np.float32)
    got = s.sample(dev(x))
    coef = s.coef.cpu().numpy()
    R.same(got, R.apply32(x, idx, coef), "sample")
    val, mag = R.apply64(x, idx, coef)
    absx = np.abs(x64)[idx].sum(1)
    allowed = R.bound32(mag, k) + 2.0 ** -23 * np.abs(c64).max(1, keepdims=True) * absx + 2.0 ** -24 * mag + 256 * k * 2.0 ** -53 * mag / ratio[:, None]
    note("linear field: |sample - exact| / (apply + coefficient + input roundings)", R.within(got, q.astype(np.float64) @ slope + const, allowed, "linear"))
    assert R.rejects(R.within, s.sample(dev((x64 ** 2).astype(np.float32))), (q.astype(np.float64) @ slope + const) ** 2, allowed)
    # a column slice of a wider tensor, and the refusals of sample()
    wide = torch.randn(1000, 40, device=DEV)
    assert torch.equal(s.sample(wide[:, 3:40]), s.sample(wide[:, 3:40].contiguous()))
    for bad in (wide[:-1], wide.double(), wide[:, 0], wide.cpu()):
        with pytest.raises(ValueError, match="^x"):
            s.sample(bad)
    # k = 1: the nearest node's row; device points are taken as they are
    s1 = gfd.PointSampler(g, dev(q), k=1, power=0)
    assert bool(s1.degenerate.all()) and torch.equal(s1.sample(wide), wide[s1.idx[:, 0].long()])
    empty = gfd.PointSampler(g, torch.zeros(0, dim))
    assert tuple(empty.sample(wide).shape) == (0, 40) and tuple(empty.idx.shape) == (0, k)


def test_lines_and_grids():
    g = cloud_graph(1000, 2)
    s = gfd.PointSampler.line(g, (0.1, 0.2), (0.9, 0.2), 9, k=8, power=1)
    assert s.k == 8 and s.power == 1 and s.shape is None
    want = np.stack([0.1 + (np.arange(9) / 8) * (0.9 - 0.1), np.full(9, 0.2)], axis=1).astype(np.float32)
    R.same(s.points, want, "line")
    r = gfd.PointSampler.grid(g, (5, 3))
    lo, hi = g.pos.min(0).values.double().cpu().numpy(), g.pos.max(0).values.double().cpu().numpy()
    xs, ys = lo[0] + (hi[0] - lo[0]) * (np.arange(5) / 4), lo[1] + (hi[1] - lo[1]) * (np.arange(3) / 2)
    R.same(r.points, np.stack(np.meshgrid(xs, ys, indexing="ij"), axis=-1).reshape(-1, 2).astype(np.float32), "grid")
    assert r.shape == (5, 3) and r.n_points == 15
    # orientation: the field x on a raster varies along the first axis and is constant along the second
    b = gfd.PointSampler.grid(g, (4, 6), box=((0.2, 0.3), (0.8, 0.7)))
    img = b.sample(g.pos.float().contiguous()).view(4, 6, 2).cpu().numpy()
    assert np.allclose(img[:, :, 0], np.linspace(0.2, 0.8, 4)[:, None], atol=1e-5) and np.allclose(img[:, :, 1], np.linspace(0.3, 0.7, 6)[None, :], atol=1e-5)
    g3 = cloud_graph(257, 3)
    r3 = gfd.PointSampler.grid(g3, (2, 1, 3), box=((0, 0, 0), (1, 1, 1)))
    assert r3.shape == (2, 1, 3) and r3.k == 10 and torch.equal(r3.points[:, 1].cpu(), torch.full((6,), 0.5))
    import graphs4cfd
    assert graphs4cfd.PointSampler is gfd.PointSampler


def test_zz_print_the_measured_ratios():
    """Not a check: the measured / allowed ratio of every bound above, for tests/SAMPLER_MEASURED.md (pytest -s)."""
    for k, v in sorted(RATIOS.items()):
        print(f"MEASURED {k}: {v:.3f}")
        assert v <= 1.0
