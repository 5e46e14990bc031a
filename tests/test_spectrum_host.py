"""Host side of the rollout spectra (no GPU): `ops.spectrum_table` against numpy's FFT, the restatement tests/spectrum_ref.py against
its own definition, `RolloutSpectrum` built from the sums the restatement produces on sinusoids rounded to fp32, and every argument
error of `gfd.Spectrum` in `Rollout(spectrum=, target_spectrum=, derived_spectrum=)`, `ops.rollout_spectrum` and
`g4c_rollout_spectrum` that can be raised without a device.

Bound of the algebra test.  The samples are x_j = a cos(2 pi b j / J + phi) + m rounded to fp32, so each is within 2^-24 |x_j| <=
2^-24 (a + |m|) of the real one.  `coeff` is linear in the samples with weights w_j e^{-i th_j} / S, sum_j w_j / S = 1, so the rounding
moves it by at most 2^-24 (a + |m|), and the exact samples give (a / 2) e^{i phi} (2 <= b <= J / 2 - 2: neither the image at -b nor
the mean leaks into bin b through a Hann window's three lines).  Hence |amplitude - a| = |2 |coeff| - a| <= 2 * 2^-24 (a + |m|), and
a |phase - phi| <= the same (the chord 2 |coeff - (a / 2) e^{i phi}| bounds a sin|dphi|; the 1e-12 covers the fp64 evaluation).  The
fp64 loop alone reaches 1.05 * 2^-24 (a + |m|) on these inputs."""
import ctypes as C
import os
import sys
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import spectrum_ref as R                                        # noqa: E402
import graphs4cfd_amd as gfd                                    # noqa: E402
from graphs4cfd_amd import _lib, ops                            # noqa: E402
from graphs4cfd_amd.nn.model import Rollout, RolloutSpectrum, _check_spectrum    # noqa: E402

F32, F64, I32, I64 = torch.float32, torch.float64, torch.int32, torch.int64


# ------------------------------------------------------------------ spectrum_table
@pytest.mark.parametrize("taper", ["rect", "hann"])
@pytest.mark.parametrize("J", [8, 15, 16])
def test_table_is_the_fft_of_the_tapered_samples(J, taper):
    bins = list(range(J // 2 + 1))
    tw, w, freqs = ops.spectrum_table(bins=bins, samples=J, taper=taper)
    assert tw.dtype == w.dtype == freqs.dtype == F64 and tuple(tw.shape) == (J, len(bins), 2) and tuple(w.shape) == (J,)
    assert tw.device.type == "cpu" and tw.is_contiguous()
    x = np.random.default_rng(J).standard_normal(J)
    got = (x[:, None] * (tw[..., 0].numpy() + 1j * tw[..., 1].numpy())).sum(0)
    want = np.fft.fft(w.numpy() * x)[bins]
    err = np.abs(got - want).max()
    print(f"  J {J} {taper}: max error {err:.3e}, allowed {1e-13 * np.abs(x).sum():.3e}")
    assert err <= 1e-13 * np.abs(x).sum()
    assert np.array_equal(freqs.numpy(), np.asarray(bins, dtype=np.float64) / J)


@pytest.mark.parametrize("taper", ["rect", "hann"])
@pytest.mark.parametrize("J,stride,dt", [(8, 1, 1.0), (15, 2, 0.1), (16, 3, 0.05), (16, 1, 0.37)])
def test_freqs_on_the_bins_give_the_bins_table(J, stride, dt, taper):
    bins = list(range(J // 2 + 1))
    by_bin, w, f = ops.spectrum_table(bins=bins, samples=J, stride=stride, dt=dt, taper=taper)
    by_freq, w2, f2 = ops.spectrum_table(freqs=[b / (J * stride * dt) for b in bins], samples=J, stride=stride, dt=dt, taper=taper)
    assert float((by_bin - by_freq).abs().max()) <= 1e-13 and torch.equal(w, w2) and float((f - f2).abs().max()) <= 1e-13 * float(f.max())
    assert np.allclose(f.numpy(), np.asarray(bins) / (J * stride * dt), rtol=1e-15)


def test_tapers():
    for J in (1, 8, 15):
        _, w, _ = ops.spectrum_table(bins=[0], samples=J, taper="hann")
        j = np.arange(J)
        assert np.array_equal(w.numpy(), 0.5 - 0.5 * np.cos(2 * np.pi * j / J)) and w[0] == 0.0
        if J > 1:
            assert abs(float(w.sum()) - J / 2) < 1e-12          # the periodic window: its weights sum to J / 2
        _, w, _ = ops.spectrum_table(bins=[0], samples=J)
        assert np.array_equal(w.numpy(), np.ones(J))
    tw, _, _ = ops.spectrum_table(bins=[0, 2], samples=8)
    assert np.array_equal(tw[:, 0].numpy(), np.stack([np.ones(8), -np.zeros(8)], -1))            # bin 0: (1, -0)
    assert np.abs(tw[:, 1, 0].numpy() - np.cos(np.pi * np.arange(8) / 2)).max() < 1e-15
    assert np.abs(tw[:, 1, 1].numpy() + np.sin(np.pi * np.arange(8) / 2)).max() < 1e-15          # the imaginary part is -sin


def test_exact_integer_phase_of_the_bins():
    """(b j) mod samples before the division: a long window's last rows are as exact as its first."""
    J = 4096
    tw, _, _ = ops.spectrum_table(bins=[1024], samples=J)          # a quarter turn per sample
    want = np.array([[1, 0], [0, -1], [-1, 0], [0, 1]], dtype=np.float64)[np.arange(J) % 4]
    assert np.abs(tw[:, 0].numpy() - want).max() < 2e-16


TABLE_BAD = {
    "neither": (dict(), ValueError, "exactly one"),
    "both": (dict(bins=[1], freqs=[0.1]), ValueError, "exactly one"),
    "bins-empty": (dict(bins=[]), ValueError, "bins"),
    "bins-negative": (dict(bins=[-1]), ValueError, "bins"),
    "bins-past-half": (dict(bins=[5]), ValueError, "bins"),
    "bins-float": (dict(bins=[1.0]), TypeError, "bins"),
    "bins-bool": (dict(bins=[True]), TypeError, "bins"),
    "bins-scalar": (dict(bins=3), TypeError, "bins"),
    "bins-str": (dict(bins="12"), TypeError, "bins"),
    "freqs-empty": (dict(freqs=[]), ValueError, "freqs"),
    "freqs-negative": (dict(freqs=[-0.1]), ValueError, "freqs"),
    "freqs-aliased": (dict(freqs=[0.51]), ValueError, "aliasing"),
    "freqs-aliased-by-stride": (dict(freqs=[0.3], stride=2), ValueError, "aliasing"),
    "freqs-aliased-by-dt": (dict(freqs=[0.3], dt=2.0), ValueError, "aliasing"),
    "freqs-nan": (dict(freqs=[float("nan")]), ValueError, "freqs"),
    "freqs-str": (dict(freqs=["a"]), TypeError, "freqs"),
    "freqs-scalar": (dict(freqs=0.1), TypeError, "freqs"),
    "samples-zero": (dict(bins=[0], samples=0), ValueError, "samples"),
    "samples-float": (dict(bins=[0], samples=8.0), TypeError, "samples"),
    "stride-zero": (dict(bins=[0], stride=0), ValueError, "stride"),
    "stride-float": (dict(bins=[0], stride=1.5), TypeError, "stride"),
    "dt-zero": (dict(bins=[0], dt=0.0), ValueError, "dt"),
    "dt-negative": (dict(bins=[0], dt=-1.0), ValueError, "dt"),
    "dt-str": (dict(bins=[0], dt="1"), TypeError, "dt"),
    "taper-unknown": (dict(bins=[0], taper="hamming"), ValueError, "taper"),
}


@pytest.mark.parametrize("label", sorted(TABLE_BAD))
def test_table_refuses(label):
    kw, exc, word = TABLE_BAD[label]
    with pytest.raises(exc) as info:
        ops.spectrum_table(**dict(dict(samples=9), **kw))
    assert type(info.value) is exc and word in str(info.value) and "spectrum_table" in str(info.value), f"{type(info.value).__name__}: {info.value}"


def test_planes():
    assert ops.spectrum_planes(3, 16) == 2 * 3 + 2 * 3 * 16 and ops.spectrum_planes(1, 1) == 4


# ------------------------------------------------------------------ the restatement
def draws(kind, n, nf, steps, seed):
    rng = np.random.default_rng(seed)
    if kind == "int":
        return [rng.integers(-8, 9, (n, nf)).astype(np.float32) for _ in range(steps)]
    return [(rng.standard_normal((n, nf)) + 1e4).astype(np.float32) for _ in range(steps)]


def test_window_first_step_and_sample_limit():
    n, nf, K, steps = 5, 2, 3, 8
    xs = draws("int", n, nf, steps + 1, 0)
    for start, stride in ((0, 1), (2, 1), (0, 3), (2, 3)):
        lattice = list(range(start, steps, stride))
        for samples in (len(lattice), len(lattice) - 1):
            if samples < 1:
                continue
            tw = np.random.default_rng(1).standard_normal((samples, K, 2))
            st = R.new_state(n, nf, K, start, fill=-7777.0)
            taken = []
            for t in range(steps + 1):
                new = R.accumulate(st, xs[t], t, steps, tw, stride)
                if t in lattice[:samples]:
                    taken.append(t)
                    assert int(new["window"][1]) == t
                else:
                    R.same_state(new, st, f"off-window step {t}")
                st = new
            assert taken == lattice[:samples] and R.count(st, stride) == samples
            d = np.stack([xs[t].astype(np.float64) - xs[start].astype(np.float64) for t in taken])          # [count, n, nf], exact
            R.same(st["pivot"], xs[start].astype(np.float64).T, "pivot")
            R.same(st["sum"], d.sum(0).T, "sum")
            # small integers times a table: every plane is the plain sum of its products, f K + k
            for f in range(nf):
                for k in range(K):
                    want = np.zeros(n)
                    for j in range(1, len(taken)):
                        want = want + d[j, :, f] * tw[j, k, 0]
                    R.same(st["re"][f * K + k], want, f"re plane ({f}, {k})")
            # running through the origin again replaces the record
            again = R.accumulate(st, xs[start], start, steps, tw, stride)
            R.same_state(again, R.accumulate(R.new_state(n, nf, K, start), xs[start], start, steps, tw, stride))


def test_x_step_takes_the_columns_of_the_step():
    n, nf, K, steps = 6, 3, 2, 5
    target = np.random.default_rng(3).standard_normal((n, nf * steps + 2)).astype(np.float32)
    tw = np.random.default_rng(4).standard_normal((steps, K, 2))
    a = R.run(target, steps, tw, x_step=nf, steps=steps)
    b = R.run([target[:, nf * t:nf * (t + 1)] for t in range(steps)], steps, tw)
    R.same_state(a, b, "target against its own columns")


def test_negative_controls():
    """Each deliberate mistake fails `same` against the correct run, on float data with a random table."""
    n, nf, K, steps = 9, 3, 4, 8
    target = (np.random.default_rng(5).standard_normal((n, nf * (steps + 1))) + 1e4).astype(np.float32)
    tw = np.random.default_rng(6).standard_normal((4, K, 2))
    ref = R.run(target, steps, tw, start=1, stride=2, x_step=nf, steps=steps)
    assert R.count(ref, 2) == 4
    for wrong in R.WRONG:
        st = R.run(target, steps, tw, start=1, stride=2, x_step=nf, steps=steps, wrong=wrong)
        assert R.rejects(R.same_state, st, ref, wrong), wrong
    R.same_state(R.run(target, steps, tw, start=1, stride=2, x_step=nf, steps=steps), ref, "the correct run again")


# ------------------------------------------------------------------ RolloutSpectrum algebra
def spectrum_of(st, stride, table, dt=1.0, taper="rect"):
    tw, w, freqs = table
    nf, n = st["pivot"].shape
    K = int(tw.size(1))
    t = {k: torch.from_numpy(np.ascontiguousarray(st[k].T)) for k in R.NAMES}
    return RolloutSpectrum(R.count(st, stride), int(st["window"][0]), stride, dt, taper, freqs, tw, w, t["pivot"], t["sum"],
                           t["re"].unflatten(1, (nf, K)), t["im"].unflatten(1, (nf, K)))


@pytest.mark.parametrize("taper", ["rect", "hann"])
@pytest.mark.parametrize("J", [16, 32])
def test_amplitude_phase_and_dominant_of_sinusoids(J, taper):
    n, dt, stride = 257, 0.25, 2
    bins = list(range(J // 2 + 1))
    table = ops.spectrum_table(bins=bins, samples=J, stride=stride, dt=dt, taper=taper)
    worst_a = worst_p = 0.0
    for b in range(2, J // 2 - 1):
        rng = np.random.default_rng(100 * J + b)
        a, m, phi = rng.uniform(0.5, 2.0, n), rng.uniform(-100.0, 100.0, n), rng.uniform(-np.pi, np.pi, n)
        xs = [(a * np.cos(2 * np.pi * b * j / J + phi) + m).astype(np.float32)[:, None] for j in range(J)]
        # the samples sit on the steps 3, 3 + stride, ...
        st = R.new_state(n, 1, len(bins), 3)
        for j in range(J):
            st = R.accumulate(st, xs[j], 3 + stride * j, 3 + stride * J, table[0].numpy(), stride)
        sp = spectrum_of(st, stride, table, dt, taper)
        assert sp.complete and sp.count == J and tuple(sp.coeff.shape) == (n, 1, len(bins)) and sp.coeff.dtype == torch.complex128
        allow = 2 * 2.0 ** -24 * (a + np.abs(m)) + 1e-12
        amp_err = np.abs(sp.amplitude[:, 0, b].numpy() - a)
        dphi = np.angle(np.exp(1j * (sp.phase[:, 0, b].numpy() - phi)))
        worst_a, worst_p = max(worst_a, float((amp_err / allow).max())), max(worst_p, float((np.abs(dphi) * a / allow).max()))
        assert (amp_err <= allow).all(), (b, float((amp_err / allow).max()))
        assert (np.abs(dphi) * a <= allow).all(), (b, float((np.abs(dphi) * a / allow).max()))
        assert sp.dominant() == float(table[2][b]) == b / (J * stride * dt)
        assert torch.equal(sp.power, sp.coeff.abs() ** 2) or torch.allclose(sp.power, sp.coeff.abs() ** 2, rtol=1e-14, atol=0)
        assert np.abs(sp.mean[:, 0].numpy() - m).max() < 1e-4            # (the mean of the fp32 samples)
        mask = torch.zeros(n, dtype=torch.bool)
        mask[:10] = True
        assert torch.allclose(sp.band_power(mask), sp.power[:10].sum(0)) and tuple(sp.band_power().shape) == (1, len(bins))
        assert sp.dominant(0, mask) == float(table[2][b])
    print(f"  J {J} {taper}: measured / allowed  amplitude {worst_a:.3f}  phase {worst_p:.3f}")


def test_coeff_is_the_transform_of_the_samples_minus_their_mean():
    """On any data and an incomplete window: coeff = sum_j w_j (x_j - mean) e^{-i th_j} / sum_j w_j over the samples taken."""
    n, nf, J, taken = 7, 2, 12, 9
    table = ops.spectrum_table(freqs=[0.0, 0.11, 0.3], samples=J)
    xs = draws("offset", n, nf, taken, 2)
    st = R.run(xs, taken, table[0].numpy())
    sp = spectrum_of(st, 1, table)
    assert not sp.complete and sp.count == taken and sp.samples == J
    x = np.stack([v.astype(np.float64) for v in xs])                       # [taken, n, nf]
    e = table[0][:taken, :, 0].numpy() + 1j * table[0][:taken, :, 1].numpy()          # [taken, K]
    want = np.einsum("jnf,jk->nfk", x - x.mean(0), e) / taken
    assert np.abs(sp.coeff.numpy() - want).max() < 1e-9 and np.abs(sp.mean.numpy() - x.mean(0)).max() < 1e-9


def test_count_zero_raises_and_an_incomplete_hann_window_warns():
    table = ops.spectrum_table(bins=[1, 2], samples=8, taper="hann")
    sp = spectrum_of(R.new_state(3, 2, 2, 4), 1, table, taper="hann")
    assert sp.count == 0 and not sp.complete and sp.fields == 2 and "count=0" in repr(sp)
    for name in ("mean", "coeff", "amplitude", "phase", "power"):
        with pytest.raises(RuntimeError, match="count == 0"):
            getattr(sp, name)
    with pytest.raises(RuntimeError, match="count == 0"):
        sp.band_power()
    with pytest.raises(RuntimeError, match="count == 0"):
        sp.dominant()
    xs = draws("offset", 3, 2, 8, 1)
    part = spectrum_of(R.run(xs[:5], 8, table[0].numpy()), 1, table, taper="hann")
    with pytest.warns(RuntimeWarning, match="hann"):
        part.amplitude
    full = spectrum_of(R.run(xs, 8, table[0].numpy()), 1, table, taper="hann")
    rect = spectrum_of(R.run(xs[:5], 8, ops.spectrum_table(bins=[1, 2], samples=8)[0].numpy()), 1, ops.spectrum_table(bins=[1, 2], samples=8))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        full.amplitude, rect.amplitude
    with pytest.raises(ValueError, match="re"):
        RolloutSpectrum(1, 0, 1, 1.0, "rect", table[2], table[0], table[1], full.pivot, full.sum, full.re[:, :, :1], full.im)
    with pytest.raises(ValueError, match="mask"):
        full.band_power(torch.ones(4, dtype=torch.bool))


def test_exports():
    import graphs4cfd
    assert gfd.nn.RolloutSpectrum is RolloutSpectrum and graphs4cfd.nn.RolloutSpectrum is RolloutSpectrum
    assert gfd.Spectrum is gfd.nn.Spectrum is graphs4cfd.Spectrum
    e = gfd.nn.RolloutErrors(torch.zeros(2, 3, _lib.REC_NSTAT, dtype=F64), 10)
    assert e.spectrum is None and e.target_spectrum is None
    assert "g4c_rollout_spectrum" in _lib.EXPORTED_SYMBOLS


# ------------------------------------------------------------------ gfd.Spectrum / Rollout(spectrum=, ...) argument errors
def host_graph(n=6, nf=3):
    return gfd.Graph(field=torch.zeros(n, nf), pos=torch.zeros(n, 2))


S = gfd.Spectrum
SPEC_BAD = {
    "not-a-spectrum": ((1, 2), TypeError),
    "true": (True, TypeError),
    "start-float": (S([1], start=1.0), TypeError),
    "start-bool": (S([1], start=True), TypeError),
    "stride-float": (S([1], stride=2.0), TypeError),
    "samples-float": (S([1], samples=4.0), TypeError),
    "dt-str": (S([1], dt="1"), TypeError),
    "taper-none": (S([1], taper=None), TypeError),
    "bins-float": (S([1.5]), TypeError),
    "freqs-str": (S(freqs=["x"]), TypeError),
    "start-negative": (S([1], start=-1), ValueError),
    "start-at-max": (S([0], start=7), ValueError),
    "stride-zero": (S([1], stride=0), ValueError),
    "samples-zero": (S([0], samples=0), ValueError),
    "samples-past-the-lattice": (S([1], start=1, stride=2, samples=4), ValueError),
    "neither": (S(), ValueError),
    "both": (S([1], [0.1]), ValueError),
    "bins-past-half": (S([4]), ValueError),
    "bins-past-half-of-samples": (S([3], samples=4), ValueError),
    "freqs-aliased": (S(freqs=[0.6]), ValueError),
    "freqs-aliased-by-stride": (S(freqs=[0.3], stride=2), ValueError),
    "dt-zero": (S([1], dt=0), ValueError),
    "taper-unknown": (S([1], taper="hamming"), ValueError),
    "too-many-bins": (S(freqs=[0.5 * k / 65 for k in range(65)]), NotImplementedError),
}


@pytest.mark.parametrize("name", ["spectrum", "derived_spectrum"])
@pytest.mark.parametrize("label", sorted(SPEC_BAD))
def test_check_spectrum_refuses(label, name):
    spec, exc = SPEC_BAD[label]
    with pytest.raises(exc) as info:
        _check_spectrum(name, spec, 3, 7)
    assert type(info.value) is exc and str(info.value).startswith(name + ":"), f"{type(info.value).__name__}: {info.value}"


def test_check_spectrum_resolves_the_window():
    assert _check_spectrum("spectrum", None, 3, 7) is None
    got = _check_spectrum("spectrum", S([0, 1], start=1, stride=2, dt=0.5, taper="hann"), 3, 7)
    assert (got["start"], got["stride"], got["samples"], got["dt"], got["taper"]) == (1, 2, 3, 0.5, "hann")
    want = ops.spectrum_table(bins=[0, 1], samples=3, stride=2, dt=0.5, taper="hann")
    assert all(torch.equal(got[k], v) for k, v in zip(("tw", "w", "freqs"), want))
    assert _check_spectrum("spectrum", S(freqs=[0.1], samples=2), 8, 7)["samples"] == 2
    assert tuple(_check_spectrum("spectrum", S(freqs=[0.5 * k / 64 for k in range(64)]), 8, 7)["tw"].shape) == (7, 64, 2)
    with pytest.raises(NotImplementedError, match="spectrum"):
        _check_spectrum("spectrum", S([1]), 9, 7)


ROLLOUT_BAD = {
    "spectrum-tuple": (dict(spectrum=(0, 1)), TypeError, "spectrum"),
    "spectrum-start": (dict(spectrum=S([1], start=7)), ValueError, "spectrum"),
    "spectrum-bins": (dict(spectrum=S([4])), ValueError, "spectrum"),
    "target_spectrum-int": (dict(spectrum=S([1]), target=torch.zeros(6, 21), target_spectrum=1), TypeError, "target_spectrum"),
    "target_spectrum-without-target": (dict(spectrum=S([1]), target_spectrum=True), ValueError, "target_spectrum"),
    "target_spectrum-without-spectrum": (dict(target=torch.zeros(6, 21), target_spectrum=True), ValueError, "target_spectrum"),
    "derived_spectrum-without-derived": (dict(derived_spectrum=S([1])), ValueError, "derived_spectrum"),
}


@pytest.mark.parametrize("label", sorted(ROLLOUT_BAD))
def test_rollout_refuses_malformed_spectra(label):
    kw, exc, word = ROLLOUT_BAD[label]
    with pytest.raises(exc) as info:
        Rollout(SimpleNamespace(num_fields=3), host_graph(), 7, **kw)
    assert type(info.value) is exc and word in str(info.value), f"{type(info.value).__name__}: {info.value}"
    assert "no CPU fallback" not in str(info.value)


def test_rollout_refuses_more_than_eight_fields():
    with pytest.raises(NotImplementedError, match="spectrum"):
        Rollout(SimpleNamespace(num_fields=9), host_graph(nf=9), 7, spectrum=S([1]))


@pytest.mark.parametrize("kw", [dict(spectrum=S([0, 3])), dict(spectrum=S(freqs=[0.1], start=2, stride=2, taper="hann")),
                                dict(spectrum=S([1], samples=4), target=torch.zeros(6, 21), target_spectrum=True)])
def test_rollout_with_wellformed_spectra_stops_at_the_device_check(kw):
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Rollout(SimpleNamespace(num_fields=3), host_graph(), 7, **kw)


# ------------------------------------------------------------------ ops.rollout_spectrum argument errors
N, NF, K, STEPS, J = 6, 3, 2, 7, 4


def good():
    planes = torch.zeros(ops.spectrum_planes(NF, K), N + 4, dtype=F64)[:, 2:N + 2]
    pivot, s, re, im = planes.split((NF, NF, NF * K, NF * K))
    return dict(x=torch.zeros(N, NF), step=torch.zeros(2, dtype=I32), nf=NF, max_steps=STEPS, window=torch.zeros(2, dtype=I32),
                tw=torch.zeros(J, K, 2, dtype=F64), pivot=pivot, sum=s, re=re, im=im, stride=2, x_step=0)


def z64(*shape):
    return torch.zeros(*shape, dtype=F64)


OPS_BAD = {
    "x-f64": (dict(x=z64(N, NF)), TypeError, "x"),
    "x-cols": (dict(x=torch.zeros(N, NF + 1)), ValueError, "x"),
    "x-colstride": (dict(x=torch.zeros(NF, N).t()), ValueError, "x"),
    "x-1d": (dict(x=torch.zeros(N * NF)), ValueError, "x"),
    "x-target-short": (dict(x=torch.zeros(N, NF * STEPS - 1), x_step=NF), ValueError, "x"),
    "x-target-colstride": (dict(x=torch.zeros(NF * STEPS, N).t(), x_step=NF), ValueError, "x"),
    "x_step-other": (dict(x_step=1), ValueError, "x_step"),
    "nf-zero": (dict(nf=0), ValueError, "nf"),
    "step-i64": (dict(step=torch.zeros(2, dtype=I64)), TypeError, "step"),
    "step-short": (dict(step=torch.zeros(1, dtype=I32)), ValueError, "step"),
    "window-i64": (dict(window=torch.zeros(2, dtype=I64)), TypeError, "window"),
    "window-short": (dict(window=torch.zeros(1, dtype=I32)), ValueError, "window"),
    "max_steps-negative": (dict(max_steps=-1), ValueError, "max_steps"),
    "stride-zero": (dict(stride=0), ValueError, "stride"),
    "tw-f32": (dict(tw=torch.zeros(J, K, 2)), TypeError, "tw"),
    "tw-2d": (dict(tw=z64(J, K)), ValueError, "tw"),
    "tw-pairs": (dict(tw=z64(J, K, 3)), ValueError, "tw"),
    "tw-no-rows": (dict(tw=z64(0, K, 2)), ValueError, "tw"),
    "tw-strided": (dict(tw=z64(J, K, 4)[:, :, :2]), ValueError, "tw"),
    "pivot-f32": (dict(pivot=torch.zeros(NF, N)), TypeError, "pivot"),
    "sum-nodes": (dict(sum=z64(NF, N + 1)), ValueError, "sum"),
    "re-planes": (dict(re=z64(NF, N)), ValueError, "re"),
    "im-node-major": (dict(im=z64(N, NF * K).t()), ValueError, "im"),
    "im-other-plane-stride": (dict(im=z64(NF * K, N)), ValueError, "plane stride"),
}


@pytest.fixture
def library_must_not_load(monkeypatch):
    def load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", load)


@pytest.mark.parametrize("label", sorted(OPS_BAD))
def test_malformed_call_raises_before_the_library(label, library_must_not_load):
    patch, exc, word = OPS_BAD[label]
    with pytest.raises(exc) as info:
        ops.rollout_spectrum(**dict(good(), **patch))
    assert type(info.value) is exc and word in str(info.value) and "rollout_spectrum" in str(info.value), f"{type(info.value).__name__}: {info.value}"
    assert "no CPU fallback" not in str(info.value)


@pytest.mark.parametrize("patch", [{}, dict(stride=1), dict(x=torch.zeros(N, NF * STEPS + 3)[:, 1:NF * STEPS + 2], x_step=NF),
                                   dict(x=torch.zeros(N, NF + 2)[:, :NF])])
def test_wellformed_call_stops_at_the_device_check(patch):
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rollout_spectrum(**dict(good(), **patch))


def test_descriptor_matches_the_header_and_the_library_checks_it_before_any_launch():
    """The ctypes descriptor has the C struct's layout (LP64: four int32, two pointers, two int32, one int64, four pointers), and every
    G4C_EINVAL / G4C_EUNSUPPORTED of g4c_rollout_spectrum comes back from the host checks — on a machine without a GPU too."""
    assert C.sizeof(_lib.g4c_rollout_spectrum_t) == 80 and C.sizeof(_lib.g4c_rollout_moments_t) == 80
    t = _lib.g4c_rollout_spectrum_t
    assert (t.window.offset, t.tw.offset, t.x_ld.offset, t.x_step.offset, t.plane_ld.offset, t.pivot.offset, t.im.offset) == (16, 24, 32, 36, 40, 48, 72)
    lib = _lib.load()
    assert lib.g4c_version() == 3
    two = (C.c_int32 * 2)()
    one = C.addressof(two)           # (any non-null address: nothing is dereferenced before the checks)
    ok = dict(max_steps=7, stride=1, n_samples=4, n_bins=2, window=one, tw=one, x_ld=3, x_step=0, plane_ld=5, pivot=one, sum=one, re=one, im=one)

    def call(nf=3, n=5, x=one, step=one, desc=True, **kw):
        s = _lib.g4c_rollout_spectrum_t(**dict(ok, **kw))
        return lib.g4c_rollout_spectrum(x, nf, C.byref(s) if desc else None, step, n, None)

    for kw, word in ((dict(desc=False), "null"), (dict(step=None), "null"), (dict(window=None), "null"), (dict(tw=None), "null"),
                     (dict(x=None), "null"), (dict(pivot=None), "null"), (dict(sum=None), "null"), (dict(re=None), "null"),
                     (dict(im=None), "null"), (dict(stride=0), "stride"), (dict(stride=-3), "stride"), (dict(n_samples=0), "n_samples"),
                     (dict(plane_ld=4), "plane_ld"), (dict(x_ld=2), "x_ld"), (dict(x_step=1), "x_step"), (dict(x_step=-3), "x_step"),
                     (dict(x_step=3, x_ld=20), "x_ld"), (dict(n=-1), "bad sizes"), (dict(nf=0), "bad sizes"), (dict(n_bins=0), "bad sizes"),
                     (dict(max_steps=-1), "bad sizes")):
        assert call(**kw) == _lib.EINVAL, kw
        msg = lib.g4c_last_error().decode()
        assert "g4c_rollout_spectrum" in msg and word in msg, (kw, msg)
    for kw in (dict(nf=9, x_ld=9), dict(n_bins=65)):
        assert call(**kw) == _lib.EUNSUPPORTED and "g4c_rollout_spectrum" in lib.g4c_last_error().decode(), kw
    # no nodes: nothing to launch, success without a device (null data pointers are fine then)
    assert call(n=0, x=None, pivot=None, sum=None, re=None, im=None, plane_ld=0) == _lib.OK
    assert call(n=0, x_step=3, x_ld=21) == _lib.OK
