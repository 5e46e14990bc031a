"""The restatements of the diagnostics (record_ref, moments_ref, spectrum_ref, gradient_ref.stats64) on non-finite samples, against
naive Python loops written here — one scalar at a time, Python floats (IEEE fp64), the maximum and minimum spelled out as compares.
Pins rules 1 – 3 of tests/nonfinite_cases.py on the host; tests/test_gpu_nonfinite.py then holds the kernels to the restatements.

One negative control per rule must be rejected: the old `fmax` (rule 2), the old `ad * m` (rule 3), a sum that skips NaN (rule 1)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gradient_ref as GR          # noqa: E402
import moments_ref as M            # noqa: E402
import nonfinite_cases as NC       # noqa: E402
import record_ref as R             # noqa: E402
import spectrum_ref as SP          # noqa: E402

pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")          # (numpy says so when Inf - Inf happens: it is meant to)


# ------------------------------------------------------------------ the naive loops
def nan_max(a, b):
    """NaN if either is; else the larger."""
    if a != a:
        return a
    if b != b:
        return b
    return a if a >= b else b


def nan_min(a, b):
    if a != a:
        return a
    if b != b:
        return b
    return a if a <= b else b


def old_fmax(a, b):
    """C's fmax: the other argument when one is NaN (what the kernels used)."""
    if a != a:
        return b
    if b != b:
        return a
    return a if a >= b else b


def naive_step_stats(pred, target, t, mask, maximum=nan_max, masked="select", skip_nan=False):
    n, nf = pred.shape
    out = np.zeros((nf, R.NSTAT))
    for f in range(nf):
        sq = ab = mx = ys = y2 = mk = 0.0
        for i in range(n):
            y = float(target[i, nf * t + f])
            d = float(pred[i, f]) - y
            ad = abs(d)
            if skip_nan and ad != ad:
                continue
            sq += d * d
            ab += ad
            mx = maximum(mx, ad)
            ys += y
            y2 += y * y
            if masked == "select":
                if mask is not None and mask[i]:
                    mk += ad
            else:          # the old restatement: ad * m
                mk += ad * (1.0 if (mask is not None and mask[i]) else 0.0)
        out[f] = (sq, ab, mx, ys, y2, mk)
    return out


def naive_moments(samples, subs, origin, stride, max_steps, minimum=nan_min, maximum=nan_max):
    """samples[t] [n, nf] fp32 for t = 0 .. ; -> the state dict of moments_ref after all of them."""
    n, nf = samples[0].shape
    pairs = M.pairs(nf)
    st = M.new_state(n, nf, origin)
    for i in range(n):
        pivot, s, lo, hi, s2, last = [0.0] * nf, [0.0] * nf, [0.0] * nf, [0.0] * nf, [0.0] * len(pairs), -1
        for t, smp in enumerate(samples):
            if not (0 <= t < max_steps and t >= origin and (t - origin) % stride == 0):
                continue
            x = [float(smp[i, f]) - (float(subs[i, nf * t + f]) if subs is not None else 0.0) for f in range(nf)]
            if subs is None:
                x = [float(smp[i, f]) for f in range(nf)]
            if t == origin:
                pivot, lo, hi, s, s2 = list(x), list(x), list(x), [0.0] * nf, [0.0] * len(pairs)
            else:
                d = [x[f] - pivot[f] for f in range(nf)]
                for f in range(nf):
                    s[f] += d[f]
                    lo[f], hi[f] = minimum(lo[f], x[f]), maximum(hi[f], x[f])
                for p, (f, g) in enumerate(pairs):
                    s2[p] += d[f] * d[g]
            last = t
        for f in range(nf):
            st["pivot"][f, i], st["sum"][f, i], st["lo"][f, i], st["hi"][f, i] = pivot[f], s[f], lo[f], hi[f]
        for p in range(len(pairs)):
            st["sum2"][p, i] = s2[p]
        st["window"][1] = last
    return st


def naive_spectrum(samples, tw, origin, stride, max_steps):
    n, nf = samples[0].shape
    count, K = tw.shape[0], tw.shape[1]
    st = SP.new_state(n, nf, K, origin)
    for i in range(n):
        for f in range(nf):
            pivot = s = 0.0
            re, im = [0.0] * K, [0.0] * K
            for t, smp in enumerate(samples):
                if not (0 <= t < max_steps and t >= origin and (t - origin) % stride == 0 and (t - origin) // stride < count):
                    continue
                j = (t - origin) // stride
                x = float(smp[i, f])
                if j == 0:
                    pivot, s, re, im = x, 0.0, [0.0] * K, [0.0] * K
                else:
                    d = x - pivot
                    s += d
                    for k in range(K):
                        re[k] += d * float(tw[j, k, 0])
                        im[k] += d * float(tw[j, k, 1])
                st["window"][1] = t
            st["pivot"][f, i], st["sum"][f, i] = pivot, s
            for k in range(K):
                st["re"][f * K + k, i], st["im"][f * K + k, i] = re[k], im[k]
    return st


def naive_stats64(cur, maximum=nan_max):
    n, nd = cur.shape
    out = np.zeros((nd, 3))
    for c in range(nd):
        sq = ab = mx = 0.0
        for i in range(n):
            q = float(cur[i, c])
            sq += q * q
            ab += abs(q)
            mx = maximum(mx, abs(q))
        out[c] = (sq, ab, mx)
    return out


def same64(got, ref, what=""):
    """fp64 values, NaN equals NaN (any payload)."""
    g, r = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert g.shape == r.shape, f"{what}: {g.shape} vs {r.shape}"
    bad = ~((g == r) | ((g != g) & (r != r)))
    if bad.any():
        pos = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} differ, first at {list(pos)}: got {g[pos]!r} want {r[pos]!r}")


# ------------------------------------------------------------------ records
T_REC, record_case = NC.T_REC, NC.record_case


@pytest.mark.parametrize("n,placement", NC.cases())
def test_record_statistics_equal_the_naive_loop(n, placement):
    poisons = NC.POISONS if n < NC.BIG else ("nan", "inf_pair")
    for name in poisons:
        for nf in (NC.FIELDS if n < NC.BIG else (1,)):
            for where in ("pred", "target"):
                for mask_kind in ((None, "in", "out") if n <= 257 else ("out",)):
                    pred, target, mask, dirty_rows = record_case(n, placement, name, nf, where, mask_kind)
                    what = f"n {n} {placement} {name} nf {nf} {where} mask {mask_kind}"
                    got = R.step_stats(torch.from_numpy(pred), torch.from_numpy(target), T_REC, None if mask is None else torch.from_numpy(mask))[0]
                    want = naive_step_stats(pred, target, T_REC, mask)
                    same64(got.numpy(), want, what)
                    # what the rule says, spelled out
                    f = nf - 1
                    if name == "nan":
                        assert math.isnan(want[f, R.MAX_ABS_ERR]) and math.isnan(want[f, R.ABS_ERR]), what
                        assert math.isnan(want[f, R.ABS_ERR_MASK]) == (mask_kind == "in"), what
                    if name in ("+inf", "-inf", "inf_pair"):
                        assert want[f, R.MAX_ABS_ERR] == math.inf, what
                        assert math.isfinite(want[f, R.ABS_ERR_MASK]) == (mask_kind != "in"), what
                    if name == "inf_pair" and where == "target" and n > 1:
                        assert math.isnan(want[f, R.TGT_SUM]) and want[f, R.TGT_SQ_SUM] == math.inf, what
                    if nf > 1 and name != "subnormal" and name != "flt_max":
                        assert np.isfinite(want[:f]).all(), what          # the other fields never see it


def test_record_negative_controls():
    """Rule 2: the old fmax is rejected.  Rule 3: the old `ad * m` is rejected.  Rule 1: a sum that skips NaN is rejected."""
    n, nf = 65, 3
    pred, target, mask, _ = record_case(n, "wave_edge", "nan", nf, "pred", "out")
    good = R.step_stats(torch.from_numpy(pred), torch.from_numpy(target), T_REC, torch.from_numpy(mask))[0].numpy()
    same64(good, naive_step_stats(pred, target, T_REC, mask), "control, as it should be")
    fmax = naive_step_stats(pred, target, T_REC, mask, maximum=old_fmax)
    assert math.isfinite(fmax[nf - 1, R.MAX_ABS_ERR]) and NC.rejects(same64, good, fmax, "old fmax")
    assert NC.rejects(same64, good, naive_step_stats(pred, target, T_REC, mask, skip_nan=True), "nan-skipping sum")
    for name in ("nan", "+inf"):          # outside the mask: `ad * 0` is NaN for both
        pred, target, mask, _ = record_case(n, "node0", name, nf, "target", "out")
        good = R.step_stats(torch.from_numpy(pred), torch.from_numpy(target), T_REC, torch.from_numpy(mask))[0].numpy()
        assert math.isfinite(good[nf - 1, R.ABS_ERR_MASK])
        old = naive_step_stats(pred, target, T_REC, mask, masked="multiply")
        assert math.isnan(old[nf - 1, R.ABS_ERR_MASK]) and NC.rejects(same64, good, old, "old ad * m")


def test_record_restatement_moves_no_bit_on_finite_data():
    """`where` for `ad * m`: the same sums on clean data (integers and floats alike: 0 * ad = 0 and ad + 0 = ad exactly)."""
    rng = np.random.default_rng(3)
    for n, nf in ((1, 1), (257, 3), (1000, 3)):
        pred, target = rng.standard_normal((n, nf)).astype(np.float32), rng.standard_normal((n, nf * NC.STEPS_REC)).astype(np.float32)
        mask = rng.random(n) < 0.3
        got = R.step_stats(torch.from_numpy(pred), torch.from_numpy(target), 1, torch.from_numpy(mask))[0]
        d = torch.from_numpy(pred).double() - torch.from_numpy(target).double()[:, nf:2 * nf]
        old = (d.abs() * torch.from_numpy(mask)[:, None]).sum(0)
        assert torch.equal(got[:, R.ABS_ERR_MASK], old)


# ------------------------------------------------------------------ moments and spectra (every node on its own)
T_ACC, time_samples = NC.T_ACC, NC.time_samples


@pytest.mark.parametrize("when", NC.TIMES)
@pytest.mark.parametrize("n,placement", [(n, p) for n in (1, 65) for p in NC.placements(n)])
def test_moments_equal_the_naive_loop(n, placement, when):
    rows = NC.rows_of(n, placement)
    for name in NC.POISONS:
        for nf in NC.FIELDS:
            for with_sub in (False, True):
                samples, dirty = time_samples(n, nf, name, rows, when)
                sub = NC.clean(np.random.default_rng(5), n, nf * T_ACC) if with_sub else None
                what = f"n {n} {placement} {name} nf {nf} {when} sub {with_sub}"
                st = M.new_state(n, nf, 1)
                for t in range(T_ACC):
                    st = M.accumulate(st, samples[t], t, T_ACC, 2, sub)
                want = naive_moments(samples, sub, 1, 2, T_ACC)
                for k in M.NAMES:
                    same64(st[k], want[k], f"{what}, {k}")
                assert list(st["window"]) == list(want["window"]) == [1, 5]
                f = nf - 1
                r = list(rows)
                if name == "nan":          # sticky in time, whenever it came
                    assert np.isnan(st["lo"][f, r]).all() and np.isnan(st["hi"][f, r]).all() and np.isnan(st["sum"][f, r]).all(), what
                    assert np.isnan(st["pivot"][f, r]).all() == (when == "first"), what
                if name == "+inf" and when != "first":
                    assert (st["hi"][f, r] == np.inf).all() and np.isfinite(st["lo"][f, r]).all(), what
                if name == "inf_pair":
                    assert (st["hi"][f, r] == np.inf).all() and (st["lo"][f, r] == -np.inf).all(), what
                    # (+Inf as the pivot: every later d is -Inf and so is their sum; +Inf later: d = +Inf, then -Inf, the sum is NaN)
                    assert (st["sum"][f, r] == -np.inf).all() if when == "first" else np.isnan(st["sum"][f, r]).all(), what
                clean_nodes = ~dirty.any(1)
                if clean_nodes.any():
                    assert np.isfinite(np.concatenate([st[k][:, clean_nodes].ravel() for k in M.NAMES])).all(), what


def test_moments_negative_control_and_finite_data():
    rows = (63, 64)
    samples, _ = time_samples(65, 3, "nan", rows, "middle")
    st = M.new_state(65, 3, 1)
    for t in range(T_ACC):
        st = M.accumulate(st, samples[t], t, T_ACC, 2)
    old = naive_moments(samples, None, 1, 2, T_ACC, minimum=lambda a, b: -old_fmax(-a, -b), maximum=old_fmax)
    assert np.isfinite(old["hi"]).all() and np.isfinite(old["lo"]).all()
    assert NC.rejects(same64, st["hi"], old["hi"], "old fmax") and NC.rejects(same64, st["lo"], old["lo"], "old fmin")
    # np.minimum / np.maximum for np.fmin / np.fmax: not a bit moves on finite data
    rng = np.random.default_rng(2)
    a, b = rng.standard_normal((3, 1000)), rng.standard_normal((3, 1000))
    assert np.array_equal(np.minimum(a, b), np.fmin(a, b)) and np.array_equal(np.maximum(a, b), np.fmax(a, b))


@pytest.mark.parametrize("K", NC.BINS)
@pytest.mark.parametrize("n,placement", [(n, p) for n in (1, 65) for p in NC.placements(n)])
def test_spectrum_equals_the_naive_loop(n, placement, K):
    rows = NC.rows_of(n, placement)
    count = 3
    j = np.arange(count)[:, None] * np.arange(K)[None, :]
    tw = np.stack([np.cos(2 * np.pi * j / count), -np.sin(2 * np.pi * j / count)], axis=-1)
    tw[:, 0, 1] = 0.0          # bin 0: an exact zero in the table, so that Inf * 0 happens
    for name in NC.POISONS:
        for nf in NC.FIELDS:
            for when in NC.TIMES:
                samples, dirty = time_samples(n, nf, name, rows, when)
                what = f"n {n} {placement} {name} nf {nf} K {K} {when}"
                st = SP.new_state(n, nf, K, 1)
                for t in range(T_ACC):
                    st = SP.accumulate(st, samples[t], t, T_ACC, tw, 2)
                want = naive_spectrum(samples, tw, 1, 2, T_ACC)
                for k in SP.NAMES:
                    same64(st[k], want[k], f"{what}, {k}")
                if name in ("+inf", "-inf") and when == "first":          # an Inf pivot: d = -+Inf, and d * 0 is NaN
                    assert np.isnan(st["im"][(nf - 1) * K, list(rows)]).all(), what
                clean_nodes = ~dirty.any(1)
                if clean_nodes.any():
                    assert np.isfinite(np.concatenate([st[k][:, clean_nodes].ravel() for k in SP.NAMES])).all(), what


# ------------------------------------------------------------------ the derived fields' norms
@pytest.mark.parametrize("n,placement", NC.cases())
def test_derived_statistics_equal_the_naive_loop(n, placement):
    rows = NC.rows_of(n, placement)
    for name in (NC.POISONS if n < NC.BIG else ("nan", "inf_pair")):
        for nd in (NC.FIELDS if n < NC.BIG else (1,)):
            cur, _ = NC.poison(NC.clean(np.random.default_rng(n + nd), n, nd), name, rows, nd - 1)
            got, want = GR.stats64(cur), naive_stats64(cur)
            what = f"n {n} {placement} {name} nd {nd}"
            same64(got, want, what)
            if name == "nan":
                assert np.isnan(got[nd - 1]).all(), what
                assert NC.rejects(same64, got, naive_stats64(cur, maximum=old_fmax), what + ", old fmax")
            if name in ("+inf", "-inf", "inf_pair"):
                assert (got[nd - 1] == np.inf).all(), what
