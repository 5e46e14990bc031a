"""The definition tests/welch_ref.py restates (and csrc/rollout_welch.hip computes) is Welch's estimator as scipy.signal has it:
`welch` / `csd` with window=w, nperseg=L, noverlap=L - H, detrend="constant", scaling="spectrum", return_onesided=False.  The
restatement runs step by step on fp32 samples; scipy gets the same samples in fp64.  Bounds: 1e-13 relative to the largest value of the
spectrum for `power` and `cross` (both are sums of L ~ 16 products of fp64 numbers, averaged over a few segments: some 1e-15; 1e-13
leaves two digits) and, for a cosine on a bin sampled in fp32, 2e-6 relative (fp32 rounding of samples of size <= 7 is <= 4e-7
absolute against A / 2 = 0.85, doubled for the square).  Every negative control of the restatement is rejected."""
import os
import sys

import numpy as np
import pytest
import scipy.signal

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import welch_ref as R                                          # noqa: E402
from welch_ref import table                                    # noqa: E402

F64 = np.float64
CASES = [(8, 8), (8, 4), (16, 8), (7, 7)]


def samples_of(x, nf):
    """x [n, nf steps] -> the list of [n, nf] samples."""
    return [x[:, nf * t:nf * (t + 1)] for t in range(x.shape[1] // nf)]


@pytest.mark.parametrize("taper", ["rect", "hann"])
@pytest.mark.parametrize("L,H", CASES)
def test_power_and_cross_are_scipys(L, H, taper):
    n, nf, segments = 5, 2, 4
    steps = (segments - 1) * H + L + 2                      # four closed segments and a partial one
    bins = list(range(L // 2 + 1))
    tw, w = table(L, bins, taper)
    rng = np.random.default_rng(10 * L + H)
    x = (rng.standard_normal((n, nf * steps)) + 3.0).astype(np.float32)
    ref_row, ref_field = 3, 1
    st = R.run(samples_of(x, nf), steps, tw, H, reference=(ref_row, ref_field))
    assert int(st["window"][2]) == segments and int(st["window"][1]) == steps - 1
    power, cross = R.power(st, w, len(bins)), R.cross(st, w, len(bins))          # [nf, K, n]
    series = x.astype(F64).reshape(n, steps, nf)                                  # [n, t, f]
    kw = dict(window=w, nperseg=L, noverlap=L - H, detrend="constant", scaling="spectrum", return_onesided=False, axis=1)
    _, pxx = scipy.signal.welch(series, **kw)                                     # [n, L, f]
    _, pxy = scipy.signal.csd(series[ref_row:ref_row + 1, :, ref_field:ref_field + 1], series, **kw)
    want_p = np.transpose(pxx[:, bins, :], (2, 1, 0))
    want_c = np.transpose(pxy[:, bins, :], (2, 1, 0))
    err_p = np.abs(power - want_p).max() / np.abs(want_p).max()
    err_c = np.abs(cross - want_c).max() / np.abs(want_c).max()
    print(f"L {L} H {H} {taper}: power {err_p:.3e} cross {err_c:.3e}")
    assert err_p <= 1e-13 and err_c <= 1e-13


@pytest.mark.parametrize("taper", ["rect", "hann"])
@pytest.mark.parametrize("L,H", [(8, 8), (8, 4), (16, 8)])
def test_a_cosine_on_a_bin(L, H, taper):
    """A cos(2 pi b j / L + phi_n) + c, sampled in fp32: power (A / 2)², phase lag phi_n - phi_r, coherence 1."""
    n, b, A, c, segments = 6, 2, 1.7, 5.0, 3
    steps = (segments - 1) * H + L
    phi = np.linspace(-1.2, 1.4, n)
    j = np.arange(steps)
    x = (A * np.cos(2.0 * np.pi * b * j[None, :] / L + phi[:, None]) + c).astype(np.float32)          # [n, steps], nf = 1
    assert np.abs(x).max() <= 7.0
    tw, w = table(L, [b - 1, b, b + 1], taper)
    st = R.run(samples_of(x, 1), steps, tw, H, reference=(1, 0))
    power, cross = R.power(st, w, 3)[0, 1], R.cross(st, w, 3)[0, 1]                                   # the bin itself, [n]
    ref_pxx = st["pxx"][1, 1]
    coherence = (st["cxr_re"][1] ** 2 + st["cxr_im"][1] ** 2) / (st["pxx"][1] * ref_pxx)
    err_p = np.abs(power / (A / 2) ** 2 - 1.0).max()
    err_l = np.abs(np.angle(cross * np.exp(-1j * (phi - phi[1])))).max()
    err_c = np.abs(coherence - 1.0).max()
    print(f"L {L} H {H} {taper}: power {err_p:.3e} lag {err_l:.3e} coherence {err_c:.3e}")
    assert err_p <= 2e-6 and err_l <= 2e-6 and err_c <= 2e-6


def test_a_partial_segment_contributes_nothing_and_sets_alternate():
    L, H, n, nf = 8, 4, 3, 2
    tw, w = table(L, [0, 1, 3], "hann")
    rng = np.random.default_rng(3)
    x = rng.standard_normal((n, nf * 30)).astype(np.float32)
    xs = samples_of(x, nf)
    a = R.run(xs[:L + 2 * H], 30, tw, H)                      # three segments, closed at its last step
    b = R.run(xs[:L + 3 * H - 1], 30, tw, H)                  # and all but the last sample of a fourth
    assert int(a["window"][2]) == int(b["window"][2]) == 3
    R.same(b["pxx"], a["pxx"], "pxx")
    assert R.rejects(R.same, b["re"], a["re"], "re")          # the open segments went on
    one = R.run(xs[:L], 30, tw, H)
    assert int(one["window"][2]) == 1 and int(R.run(xs[:L - 1], 30, tw, H)["window"][2]) == 0


def test_start_stride_and_first_slot_move_the_lattice():
    L, H, n, nf, steps = 4, 4, 2, 1, 40
    tw, w = table(L, [1], "rect")
    rng = np.random.default_rng(4)
    x = rng.standard_normal((n, steps)).astype(np.float32)
    st = R.run(samples_of(x, nf), steps, tw, H, start=2, stride=3)
    want = R.run(samples_of(x[:, 2::3], nf), steps, tw, H)
    R.same(st["pxx"], want["pxx"], "pxx")
    assert int(st["window"][0]) == 2 and int(st["window"][2]) == len(range(2, steps, 3)) // L
    assert R.lattice_origin(2, 3, 0) == 2 and R.lattice_origin(2, 3, 3) == 5 and R.lattice_origin(2, 3, 5) == 5
    target = R.run(x, steps, tw, H, x_step=nf, steps=steps)
    R.same(target["pxx"], R.run(samples_of(x, nf), steps, tw, H)["pxx"], "x_step")


def test_nonfinite_samples_poison_their_row_and_field_only():
    L, H, n, nf, steps = 4, 2, 4, 2, 14
    tw, w = table(L, [0, 1], "hann")
    rng = np.random.default_rng(5)
    x = rng.standard_normal((n, nf * steps)).astype(np.float32)
    clean = R.run(samples_of(x, nf), steps, tw, H, reference=(0, 0))
    x[2, nf * 5 + 1] = np.nan                                  # row 2, field 1, sample 5: segments 1 and 2
    st = R.run(samples_of(x, nf), steps, tw, H, reference=(0, 0))
    pxx = st["pxx"].reshape(nf, 2, n)
    assert np.isnan(pxx[1, :, 2]).all() and np.isnan(st["cxr_re"].reshape(nf, 2, n)[1, :, 2]).all()
    keep = np.ones((nf, 2, n), dtype=bool)
    keep[1, :, 2] = False
    assert np.array_equal(pxx[keep], clean["pxx"].reshape(nf, 2, n)[keep]) and np.isfinite(pxx[keep]).all()
    x[2, nf * 5 + 1], x[0, 0] = 0.5, np.inf                    # the reference itself: every cxr, and no pxx but its own
    st = R.run(samples_of(x, nf), steps, tw, H, reference=(0, 0))
    assert not np.isfinite(st["cxr_re"]).any() and np.isfinite(st["pxx"].reshape(nf, 2, n)[:, :, 1:]).all()


@pytest.mark.parametrize("wrong", R.WRONG)
def test_negative_controls(wrong):
    L, H, n, nf = 8, 4, 5, 2
    steps = 3 * H + L + 2
    tw, w = table(L, [0, 1, 2, 4], "hann")
    rng = np.random.default_rng(6)
    x = (rng.standard_normal((n, nf * steps)) + 2.0).astype(np.float32)
    kw = dict(reference=(3, 1), track=[0, 4, 0], max_segments=4, fill=-7777.0)
    good = R.run(samples_of(x, nf), steps, tw, H, **kw)
    again = R.run(samples_of(x, nf), steps, tw, H, **kw)
    R.same_state(again, good, "twice")
    bad = R.run(samples_of(x, nf), steps, tw, H, wrong=wrong, **kw)
    assert R.rejects(R.same_state, good, bad, wrong), wrong
