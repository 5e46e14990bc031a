"""Host side of the Welch spectra: every refusal of `gfd.Welch` / `_check_welch` / `Rollout.open(welch=)` / `GNN.welch` /
`ops.rollout_welch` / g4c_rollout_welch by its message — all before a device is touched —, the descriptor's layout, the exports, and the
derived quantities of `RolloutWelch` formed from the restatement's sums (tests/welch_ref.py) against scipy.signal."""
import ctypes as C
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import scipy.signal
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import welch_ref as R                                          # noqa: E402
import graphs4cfd_amd as gfd                                   # noqa: E402
from graphs4cfd_amd import _lib, ops                           # noqa: E402
from graphs4cfd_amd.nn import rollout as RO                    # noqa: E402
from graphs4cfd_amd.nn.model import GNN, Rollout, RolloutWelch  # noqa: E402

F64, I32, I64 = torch.float64, torch.int32, torch.int64
W = gfd.Welch


def test_exports():
    import graphs4cfd
    assert gfd.Welch is gfd.nn.Welch is graphs4cfd.Welch is RO.Welch
    assert gfd.nn.RolloutWelch is RolloutWelch and graphs4cfd.nn.RolloutWelch is RolloutWelch
    assert "g4c_rollout_welch" in _lib.EXPORTED_SYMBOLS
    assert RO.KEYWORDS["welch"] is None and RO.KEYWORDS["target_welch"] is False
    assert RO._PARTS.index(RO._Welch) == RO._PARTS.index(RO._DerivedSpectrum) + 1 and RO._PARTS[-1] is RO._Tracers
    e = gfd.nn.RolloutErrors(torch.zeros(2, 3, _lib.REC_NSTAT, dtype=F64), 10)
    assert e.welch is None and e.target_welch is None
    assert callable(GNN.welch) and callable(GNN.evaluate_welch) and callable(Rollout.welch) and callable(Rollout.target_welch)


def test_planes_and_weights():
    assert ops.welch_planes(3, 5, False) == 2 * ops.spectrum_planes(3, 5) + 15 and ops.welch_planes(3, 5, True) == 2 * ops.spectrum_planes(3, 5) + 45
    assert ops.welch_split(2, 3, True) == (4, 4, 12, 12, 6, 6, 6) and sum(ops.welch_split(2, 3, False)) == ops.welch_planes(2, 3, False)
    tw = torch.from_numpy(np.random.default_rng(0).standard_normal((7, 3, 2)))
    assert np.array_equal(ops.welch_weights(tw).numpy(), R.weights(tw.numpy()))           # row by row, in order: the same bits


# ------------------------------------------------------------------ gfd.Welch / _check_welch
SPEC_BAD = {
    "not-a-welch": ((8, [1]), TypeError, "expected a gfd.Welch"),
    "a-spectrum": (gfd.Spectrum([1]), TypeError, "expected a gfd.Welch"),
    "segment-float": (W(8.0, [1]), TypeError, "integers"),
    "segment-bool": (W(True, [1]), TypeError, "integers"),
    "start-float": (W(8, [1], start=1.0), TypeError, "integers"),
    "stride-float": (W(8, [1], stride=2.0), TypeError, "integers"),
    "dt-str": (W(8, [1], dt="1"), TypeError, "dt"),
    "taper-none": (W(8, [1], taper=None), TypeError, "taper"),
    "overlap-quarter": (W(8, [1], overlap=0.25), ValueError, "overlap"),
    "overlap-true": (W(8, [1], overlap=True), ValueError, "overlap"),
    "overlap-odd-segment": (W(7, [1], overlap=0.5), ValueError, "even segment"),
    "segment-one": (W(1, [0]), ValueError, "segment 1"),
    "start-negative": (W(8, [1], start=-1), ValueError, "start"),
    "start-at-max": (W(8, [1], start=40), ValueError, "start"),
    "stride-zero": (W(8, [1], stride=0), ValueError, "stride"),
    "no-complete-segment": (W(8, [1], start=33), ValueError, "not one segment"),
    "no-complete-segment-by-stride": (W(8, [1], stride=6), ValueError, "not one segment"),
    "neither": (W(8), ValueError, "exactly one of"),
    "both": (W(8, [1], [0.1]), ValueError, "exactly one of"),
    "bins-float": (W(8, [1.5]), TypeError, "bins"),
    "bins-past-half": (W(8, [5]), ValueError, "bins"),
    "freqs-aliased": (W(8, freqs=[0.6]), ValueError, "freqs"),
    "dt-zero": (W(8, [1], dt=0), ValueError, "dt"),
    "taper-unknown": (W(8, [1], taper="hamming"), ValueError, "taper"),
    "too-many-bins": (W(8, freqs=[0.5 * k / 65 for k in range(65)]), NotImplementedError, "65 frequencies"),
    "reference-str": (W(8, [1], reference="node"), TypeError, "reference"),
    "reference-one": (W(8, [1], reference=(1,)), TypeError, "reference"),
    "reference-float": (W(8, [1], reference=(1.0, 0)), TypeError, "reference"),
    "reference-node": (W(8, [1], reference=(6, 0)), ValueError, "node 6 of 6"),
    "reference-field": (W(8, [1], reference=(0, 3)), ValueError, "field 3 of 3"),
    "reference-target-without-target": (W(8, [1], reference="target"), ValueError, "needs target="),
    "track-str": (W(8, [1], track="01"), TypeError, "track"),
    "track-float": (W(8, [1], track=[0.5]), TypeError, "track"),
    "track-float-tensor": (W(8, [1], track=torch.zeros(2)), TypeError, "track"),
    "track-2d": (W(8, [1], track=torch.zeros(2, 2, dtype=I64)), TypeError, "track"),
    "track-range": (W(8, [1], track=[0, 6]), ValueError, "rows 0 .. 6"),
    "track-negative": (W(8, [1], track=[-1]), ValueError, "rows -1"),
    "track-too-many": (W(8, [1], track=[0] * 1025), NotImplementedError, "1025 rows"),
}


@pytest.mark.parametrize("label", sorted(SPEC_BAD))
def test_check_welch_refuses(label):
    spec, exc, word = SPEC_BAD[label]
    with pytest.raises(exc) as info:
        RO._check_welch("welch", spec, 3, 40, 6, False)
    assert type(info.value) is exc and str(info.value).startswith("welch:") and word in str(info.value), f"{type(info.value).__name__}: {info.value}"


def test_check_welch_resolves_the_segments():
    assert RO._check_welch("welch", None, 3, 40, 6, False) is None
    got = RO._check_welch("welch", W(8, [0, 1], overlap=0.5, start=1, stride=2, dt=0.5, reference=(5, 2), track=torch.tensor([5, 0, 5])), 3, 40, 6, False)
    assert (got["start"], got["stride"], got["L"], got["H"], got["dt"], got["taper"]) == (1, 2, 8, 4, 0.5, "hann")
    assert got["reference"] == (5, 2) and got["track"] == [5, 0, 5]
    assert got["max_segments"] == (len(range(1, 40, 2)) - 8) // 4 + 1 == 4
    want = ops.spectrum_table(bins=[0, 1], samples=8, stride=2, dt=0.5, taper="hann")
    assert all(torch.equal(got[k], v) for k, v in zip(("tw", "w", "freqs"), want))
    assert np.array_equal(got["W"].numpy(), R.weights(want[0].numpy()))
    assert np.array_equal(want[0].numpy(), R.table(8, [0, 1], "hann")[0])                  # the restatement's table is the package's
    assert got["freqs"].tolist() == [0.0, 1.0 / (8 * 2 * 0.5)]
    side = RO._check_welch("welch", W(7, [3], taper="rect", reference="target", track=[]), 8, 40, 6, True)
    assert (side["L"], side["H"], side["reference"], side["track"], side["max_segments"]) == (7, 7, "target", None, 5)
    with pytest.raises(NotImplementedError, match="welch"):
        RO._check_welch("welch", W(8, [1]), 9, 40, 6, False)


def host_graph(n=6, nf=3):
    return gfd.Graph(field=torch.zeros(n, nf), pos=torch.zeros(n, 2))


ROLLOUT_BAD = {
    "welch-tuple": (dict(welch=(8, [1])), TypeError, "welch"),
    "welch-segment": (dict(welch=W(80, [1])), ValueError, "not one segment"),
    "welch-reference-target": (dict(welch=W(8, [1], reference="target")), ValueError, "needs target="),
    "welch-reference-node": (dict(welch=W(8, [1], reference=(6, 0))), ValueError, "node 6"),
    "target_welch-int": (dict(welch=W(8, [1]), target=torch.zeros(6, 120), target_welch=1), TypeError, "target_welch"),
    "target_welch-without-target": (dict(welch=W(8, [1]), target_welch=True), ValueError, "target_welch"),
    "target_welch-without-welch": (dict(target=torch.zeros(6, 120), target_welch=True), ValueError, "target_welch"),
    "unknown-keyword": (dict(welsh=W(8, [1])), TypeError, "welsh"),
}


@pytest.mark.parametrize("label", sorted(ROLLOUT_BAD))
def test_rollout_refuses_malformed_requests(label):
    kw, exc, word = ROLLOUT_BAD[label]
    with pytest.raises(exc) as info:
        Rollout.open(SimpleNamespace(num_fields=3), host_graph(), 40, **kw)
    assert type(info.value) is exc and word in str(info.value), f"{type(info.value).__name__}: {info.value}"
    assert "no CPU fallback" not in str(info.value)


def test_a_list_of_graphs_counts_the_nodes_of_all():
    check = lambda ref: RO._check_parts(dict(welch=W(8, [1], reference=ref, track=[11])), [host_graph(), host_graph()], 3, 40, False)      # noqa: E731
    assert check((11, 2))["welch"]["reference"] == (11, 2)
    with pytest.raises(ValueError, match="node 12 of 12"):
        check((12, 0))


@pytest.mark.parametrize("kw", [dict(welch=W(8, [0, 3])), dict(welch=W(8, freqs=[0.1], overlap=0.5, start=2, stride=2, taper="rect", track=[0, 5])),
                                dict(welch=W(8, [1], reference="target"), target=torch.zeros(6, 120), target_welch=True)])
def test_rollout_with_wellformed_requests_stops_at_the_device_check(kw):
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Rollout.open(SimpleNamespace(num_fields=3), host_graph(), 40, **kw)


def test_the_model_refuses_before_anything_is_moved():
    model = SimpleNamespace(num_fields=3, _rollout=None)
    g = host_graph()
    with pytest.raises(ValueError, match="no `target`"):
        GNN.welch(model, g, 40, 8, [1], reference="target")
    with pytest.raises(ValueError, match="no `target`"):
        GNN.welch(model, g, 40, 8, [1], target=True)
    with pytest.raises(TypeError, match="target"):
        GNN.welch(model, g, 40, 8, [1], target=1)
    g.target = torch.zeros(6, 120)
    with pytest.raises(TypeError, match="gfd.Welch"):
        GNN.evaluate_welch(model, g, gfd.Spectrum([1]))

    def rollout(graph, n_out, capture, label, evaluate=False, **records):          # (what `GNN._rollout` does first)
        RO._check_parts(records, graph, 3, n_out, evaluate)
        raise KeyError("checked")
    model._rollout = rollout
    with pytest.raises(ValueError, match="welch: segment 80"):
        GNN.welch(model, g, 40, 80, [1])
    with pytest.raises(KeyError, match="checked"):
        GNN.evaluate_welch(model, g, W(8, [1], reference="target"))


# ------------------------------------------------------------------ ops.rollout_welch
N, NF, K, STEPS, L, P, SEGS = 6, 3, 2, 40, 8, 3, 4


def z64(*shape):
    return torch.zeros(*shape, dtype=F64)


def good(reference=False, tracked=False):
    planes = z64(ops.welch_planes(NF, K, reference), N + 4)[:, 2:N + 2].split(ops.welch_split(NF, K, reference))
    kw = dict(x=torch.zeros(N, NF), step=torch.zeros(2, dtype=I32), nf=NF, max_steps=STEPS, window=torch.zeros(3, dtype=I32), tw=z64(L, K, 2),
              W=z64(K, 2), pivot=planes[0], sum=planes[1], re=planes[2], im=planes[3], pxx=planes[4], hop=4, stride=2, x_step=0)
    if reference:
        kw.update(cxr=(planes[5], planes[6]), ref_row=2, ref_field=1)
    if tracked:
        kw.update(track=torch.zeros(P, dtype=I32), track_host=torch.zeros(P, dtype=I32), seg_power=z64(SEGS, P, NF, K))
    return kw


OPS_BAD = {
    "x-f64": (dict(x=z64(N, NF)), TypeError, "x"),
    "x-cols": (dict(x=torch.zeros(N, NF + 1)), ValueError, "x"),
    "x-colstride": (dict(x=torch.zeros(NF, N).t()), ValueError, "x"),
    "x-target-short": (dict(x=torch.zeros(N, NF * STEPS - 1), x_step=NF), ValueError, "x"),
    "x_step-other": (dict(x_step=1), ValueError, "x_step"),
    "nf-zero": (dict(nf=0), ValueError, "nf"),
    "step-i64": (dict(step=torch.zeros(2, dtype=I64)), TypeError, "step"),
    "step-short": (dict(step=torch.zeros(1, dtype=I32)), ValueError, "step"),
    "window-i64": (dict(window=torch.zeros(3, dtype=I64)), TypeError, "window"),
    "window-two": (dict(window=torch.zeros(2, dtype=I32)), ValueError, "window"),
    "max_steps-negative": (dict(max_steps=-1), ValueError, "max_steps"),
    "stride-zero": (dict(stride=0), ValueError, "stride"),
    "tw-f32": (dict(tw=torch.zeros(L, K, 2)), TypeError, "tw"),
    "tw-2d": (dict(tw=z64(L, K)), ValueError, "tw"),
    "tw-one-row": (dict(tw=z64(1, K, 2)), ValueError, "tw"),
    "tw-strided": (dict(tw=z64(L, K, 4)[:, :, :2]), ValueError, "tw"),
    "W-f32": (dict(W=torch.zeros(K, 2)), TypeError, "W"),
    "W-shape": (dict(W=z64(K + 1, 2)), ValueError, "W"),
    "pivot-one-set": (dict(pivot=z64(NF, N)), ValueError, "pivot"),
    "sum-f32": (dict(sum=torch.zeros(2 * NF, N)), TypeError, "sum"),
    "re-planes": (dict(re=z64(NF * K, N)), ValueError, "re"),
    "im-node-major": (dict(im=z64(N, 2 * NF * K).t()), ValueError, "im"),
    "pxx-planes": (dict(pxx=z64(2 * NF * K, N)), ValueError, "pxx"),
    "pxx-other-plane-stride": (dict(pxx=z64(NF * K, N)), ValueError, "plane stride"),
    "cxr-missing": (dict(ref_row=1), ValueError, "cxr"),
    "cxr-one": (dict(cxr=(z64(NF * K, N),)), ValueError, "cxr"),
    "track-without-seg_power": (dict(track=torch.zeros(P, dtype=I32), track_host=torch.zeros(P, dtype=I32)), ValueError, "track"),
    "track-i64": (dict(track=torch.zeros(P, dtype=I64), track_host=torch.zeros(P, dtype=I32), seg_power=z64(SEGS, P, NF, K)), TypeError, "track"),
    "track_host-length": (dict(track=torch.zeros(P, dtype=I32), track_host=torch.zeros(P + 1, dtype=I32), seg_power=z64(SEGS, P, NF, K)), ValueError,
                          "track_host"),
    "seg_power-shape": (dict(track=torch.zeros(P, dtype=I32), track_host=torch.zeros(P, dtype=I32), seg_power=z64(SEGS, P, K, NF)), ValueError,
                        "seg_power"),
}
REF_BAD = {
    "ref_row-range": (dict(ref_row=N), ValueError, "ref_row"),
    "ref_field-range": (dict(ref_field=NF), ValueError, "ref_field"),
    "ref-two": (dict(ref=(z64(2 * NF, N), z64(2 * NF * K, N))), ValueError, "ref"),
    "ref-other-plane-stride": (dict(ref=(z64(2 * NF, N), z64(2 * NF * K, N), z64(2 * NF * K, N))), ValueError, "plane stride"),
    "cxr-f32": (dict(cxr=(torch.zeros(NF * K, N), torch.zeros(NF * K, N))), TypeError, "cxr_re"),
}


@pytest.fixture
def library_must_not_load(monkeypatch):
    def load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", load)


@pytest.mark.parametrize("label", sorted(OPS_BAD) + sorted(REF_BAD))
def test_malformed_call_raises_before_the_library(label, library_must_not_load):
    patch, exc, word = OPS_BAD[label] if label in OPS_BAD else REF_BAD[label]
    with pytest.raises(exc) as info:
        ops.rollout_welch(**dict(good(reference=label in REF_BAD), **patch))
    assert type(info.value) is exc and word in str(info.value) and "rollout_welch" in str(info.value), f"{type(info.value).__name__}: {info.value}"
    assert "no CPU fallback" not in str(info.value)


@pytest.mark.parametrize("kw", [dict(), dict(reference=True), dict(tracked=True), dict(reference=True, tracked=True)])
def test_wellformed_call_stops_at_the_device_check(kw):
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rollout_welch(**good(**kw))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rollout_welch(**dict(good(**kw), x=torch.zeros(N, NF * STEPS + 3)[:, 1:NF * STEPS + 2], x_step=NF))


def test_descriptor_matches_the_header_and_the_library_checks_it_before_any_launch():
    """The ctypes descriptor has the C struct's layout (LP64: eleven int32 and four bytes of padding, three pointers, a double, an int64,
    thirteen pointers), and every G4C_EINVAL / G4C_EUNSUPPORTED of g4c_rollout_welch comes back from the host checks — on a machine
    without a GPU too."""
    t = _lib.g4c_rollout_welch_t
    assert C.sizeof(t) == 48 + 3 * 8 + 8 + 8 + 13 * 8
    assert (t.max_segments.offset, t.window.offset, t.W.offset, t.inv_L.offset, t.plane_ld.offset, t.pivot.offset, t.seg_power.offset) == (40, 48, 64, 72, 80, 88, 184)
    lib = _lib.load()
    assert lib.g4c_version() == 3
    rows = (C.c_int32 * 4)(0, 4, 0, 2)
    one = C.addressof(rows)           # (any non-null address: nothing on the device is dereferenced before the checks)
    ok = dict(max_steps=40, stride=1, seg_len=8, hop=4, n_bins=2, x_ld=3, x_step=0, ref_row=-1, ref_field=-1, n_track=0, max_segments=0, window=one,
              tw=one, W=one, inv_L=0.125, plane_ld=5, pivot=one, sum=one, re=one, im=one, pxx=one)
    ref = dict(cxr_re=one, cxr_im=one, ref_sum=one, ref_re=one, ref_im=one)
    trk = dict(n_track=4, max_segments=3, track=one, track_host=one, seg_power=one)

    def call(nf=3, n=5, x=one, step=one, desc=True, **kw):
        s = t(**dict(ok, **kw))
        return lib.g4c_rollout_welch(x, nf, C.byref(s) if desc else None, step, n, None)

    for kw, word in ((dict(desc=False), "null"), (dict(step=None), "null"), (dict(window=None), "null"), (dict(tw=None), "null"),
                     (dict(W=None), "null"), (dict(x=None), "null"), (dict(pivot=None), "null"), (dict(sum=None), "null"), (dict(re=None), "null"),
                     (dict(im=None), "null"), (dict(pxx=None), "null"), (dict(stride=0), "stride"), (dict(seg_len=1, hop=1), "seg_len"),
                     (dict(plane_ld=4), "plane_ld"), (dict(x_ld=2), "x_ld"), (dict(x_step=1), "x_step"), (dict(x_step=3, x_ld=20), "x_ld"),
                     (dict(n=-1), "bad sizes"), (dict(nf=0), "bad sizes"), (dict(n_bins=0), "bad sizes"), (dict(max_steps=-1), "bad sizes"),
                     (dict(ref, cxr_im=None), "reference"), (dict(cxr_re=one), "reference"), (dict(ref, ref_row=5), "ref_row"),
                     (dict(ref, ref_field=3), "ref_field"), (dict(trk, n=4), "track[1]=4"), (dict(trk, track_host=None), "track"),
                     (dict(trk, seg_power=None), "track"), (dict(n_track=-1), "n_track")):
        assert call(**kw) == _lib.EINVAL, kw
        msg = lib.g4c_last_error().decode()
        assert "g4c_rollout_welch" in msg and word in msg, (kw, msg)
    for kw, word in ((dict(nf=9, x_ld=9), "nf=9"), (dict(n_bins=65), "n_bins=65"), (dict(hop=3), "hop=3"), (dict(hop=8, seg_len=7), "hop=8"),
                     (dict(seg_len=7, hop=3), "hop=3"), (dict(hop=0), "hop=0"), (dict(trk, n_track=1025), "n_track=1025")):
        assert call(**kw) == _lib.EUNSUPPORTED, kw
        msg = lib.g4c_last_error().decode()
        assert "g4c_rollout_welch" in msg and word in msg, (kw, msg)
    # no nodes: nothing to launch, success without a device (null data pointers are fine then)
    assert call(n=0, x=None, pivot=None, sum=None, re=None, im=None, pxx=None, plane_ld=0) == _lib.OK
    assert call(n=0, x_step=3, x_ld=120, hop=8) == _lib.OK and call(n=0, seg_len=7, hop=7) == _lib.OK and call(n=0, seg_len=2, hop=1) == _lib.OK


# ------------------------------------------------------------------ RolloutWelch
def result_of(st, tg, w, freqs, L, H, stride=1, dt=1.0, taper="hann", track=None, reference=None, segments=None):
    """A `RolloutWelch` from the restatement's state(s), as `_Welch.read` builds it: rows first."""
    K, n = len(freqs), st["pxx"].shape[1]
    rows = lambda a: torch.from_numpy(np.ascontiguousarray(a.T)).unflatten(1, (-1, K))          # noqa: E731
    more = {}
    if reference is not None:
        pxx = rows(st["pxx"])
        more.update(cxr_re=rows(st["cxr_re"]), cxr_im=rows(st["cxr_im"]), reference=reference,
                    ref_pxx=rows(tg["pxx"]) if reference == "target" else pxx[reference[0], reference[1]].reshape(1, 1, -1))
    closed = int(st["window"][2]) if segments is None else segments
    if track is not None:
        more.update(seg_power=torch.from_numpy(st["seg_power"][:closed].copy()), track=torch.tensor(track))
    return RolloutWelch(closed, int(st["window"][0]), stride, L, H, dt, taper, torch.tensor(freqs, dtype=F64), torch.from_numpy(w), rows(st["pxx"]), **more)


@pytest.mark.filterwarnings("ignore:invalid value encountered")          # (scipy's own 0 / 0 at frequency 0 of a "rect" segment)
@pytest.mark.parametrize("L,H,taper", [(8, 8, "rect"), (8, 4, "hann"), (16, 8, "hann")])
def test_derived_quantities_are_scipys(L, H, taper):
    n, nf, segments, stride, dt = 5, 2, 4, 3, 0.25
    steps = (segments - 1) * H + L + 1
    bins = list(range(L // 2 + 1))
    tw, w, freqs = (t.numpy() for t in ops.spectrum_table(bins=bins, samples=L, stride=stride, dt=dt, taper=taper))
    rng = np.random.default_rng(L + H)
    x = (rng.standard_normal((n, nf * steps)) + 3.0).astype(np.float32)
    xs = [x[:, nf * t:nf * (t + 1)] for t in range(steps)]
    track = [4, 0, 4]
    st = R.run(xs, steps, tw, H, reference=(3, 1), track=track, max_segments=segments + 1)
    we = result_of(st, None, w, freqs.tolist(), L, H, stride, dt, taper, track, (3, 1))
    assert we.segments == segments and we.fields == nf and (we.S, we.S2) == pytest.approx((w.sum(), (w * w).sum()), rel=1e-14)
    series = x.astype(np.float64).reshape(n, steps, nf)
    fs = 1.0 / (stride * dt)
    kw = dict(fs=fs, window=w, nperseg=L, noverlap=L - H, detrend="constant", axis=1)
    f, psd = scipy.signal.welch(series, scaling="density", return_onesided=True, **kw)           # [n, L / 2 + 1, nf]
    _, power = scipy.signal.welch(series, scaling="spectrum", return_onesided=False, **kw)
    _, coh = scipy.signal.coherence(series[3:4, :, 1:2], series, **kw)
    _, pxy = scipy.signal.csd(series[3:4, :, 1:2], series, scaling="spectrum", return_onesided=False, **kw)
    rel = lambda got, want: float(np.abs(got.numpy() - np.transpose(want, (0, 2, 1))).max() / np.abs(want).max())          # noqa: E731
    assert np.allclose(freqs, f, rtol=1e-14, atol=0)
    assert rel(we.power, power[:, bins]) <= 1e-13 and rel(we.psd, psd) <= 1e-13 and rel(we.cross, pxy[:, bins]) <= 1e-13
    # (a "rect" segment with its mean removed has no power at frequency 0: the coherence there is 0 / 0, here as in scipy)
    got, want = we.coherence.numpy()[:, :, 1:], np.transpose(coh, (0, 2, 1))[:, :, 1:]
    assert float(np.abs(got - want).max()) <= 1e-12 and float(got.max()) <= 1.0 + 1e-12
    if taper == "rect":
        assert bool(torch.isnan(we.coherence[:, :, 0]).all()) and np.isnan(coh[:, 0]).all()
    turn = we.phase_lag.numpy() - np.angle(np.transpose(pxy[:, bins], (0, 2, 1)))          # (compared on the circle: -pi is pi)
    assert float(np.abs(np.angle(np.exp(1j * turn))).max()) <= 1e-12
    assert torch.equal(we.coherence[3, 1, 1:], torch.ones(len(bins) - 1, dtype=F64))                    # the reference against itself
    # the spectrogram is the power of each segment on its own
    for s in range(segments):
        seg = series[track][:, s * H:s * H + L]
        _, one = scipy.signal.welch(seg, scaling="spectrum", return_onesided=False, **kw)
        assert float(np.abs(we.spectrogram[s].numpy() - np.transpose(one[:, bins], (0, 2, 1))).max()) <= 1e-13 * np.abs(one).max()
    assert torch.allclose(we.spectrogram.sum(0) / segments, we.power[track], rtol=1e-13, atol=0)
    assert tuple(we.dominant_by_segment(1, 0).shape) == (segments,) and we.dominant(1) in freqs.tolist()
    assert torch.equal(we.band_power(), we.power.sum(0))
    mask = torch.tensor([True, False, True, False, False])
    assert torch.equal(we.band_power(mask), we.power[mask].sum(0))
    with pytest.raises(ValueError, match="mask"):
        we.band_power(torch.ones(4, dtype=torch.bool))


def test_a_drifting_frequency_shows_in_the_segments():
    L, n_seg = 16, 3
    tw, w, freqs = (t.numpy() for t in ops.spectrum_table(bins=list(range(9)), samples=L, taper="hann"))
    parts = [np.cos(2.0 * np.pi * b * np.arange(L) / L) for b in (2, 3, 5)]
    x = np.concatenate(parts)[None, :].astype(np.float32)
    st = R.run([x[:, t:t + 1] for t in range(L * n_seg)], L * n_seg, tw, L, track=[0], max_segments=n_seg)
    we = result_of(st, None, w, freqs.tolist(), L, L, track=[0])
    assert we.dominant_by_segment(0, 0).tolist() == [2 / 16, 3 / 16, 5 / 16]


def test_segments_zero_and_missing_parts_raise():
    L, K, n, nf = 8, 2, 3, 2
    w = np.ones(L)
    st = R.new_state(n, nf, K, 0, reference=True, tracked=2, max_segments=3)
    we = result_of(st, None, w, [0.0, 0.125], L, L, taper="rect", track=[0, 1], reference=(0, 0))
    assert we.segments == 0 and "segments=0" in repr(we)
    for name in ("power", "psd", "cross", "coherence", "phase_lag", "spectrogram"):
        with pytest.raises(RuntimeError, match="segments == 0"):
            getattr(we, name)
    for call in (we.band_power, we.dominant, we.dominant_by_segment):
        with pytest.raises(RuntimeError, match="segments == 0"):
            call()
    plain = result_of(R.new_state(n, nf, K, 0), None, w, [0.0, 0.125], L, L, taper="rect", segments=2)
    assert plain.power.shape == (n, nf, K) and plain.target is None
    for name in ("cross", "coherence", "phase_lag"):
        with pytest.raises(RuntimeError, match="reference"):
            getattr(plain, name)
    with pytest.raises(RuntimeError, match="track"):
        plain.spectrogram
    with pytest.raises(ValueError, match="pxx"):
        RolloutWelch(1, 0, 1, L, L, 1.0, "rect", torch.zeros(3, dtype=F64), torch.ones(L, dtype=F64), torch.zeros(n, nf, K, dtype=F64))
    with pytest.raises(ValueError, match="cxr_re"):
        RolloutWelch(1, 0, 1, L, L, 1.0, "rect", torch.zeros(K, dtype=F64), torch.ones(L, dtype=F64), torch.zeros(n, nf, K, dtype=F64),
                     cxr_re=torch.zeros(n, nf, K, dtype=F64))
