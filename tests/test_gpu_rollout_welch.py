"""g4c_rollout_welch (csrc/rollout_welch.hip) through ops.rollout_welch against the fp64 restatement of tests/welch_ref.py, and the
Welch spectra of `Rollout.open(welch=, target_welch=)` / `GNN.welch` / `GNN.evaluate_welch` against the restatement run over the
rollout's own `result()` and target.

Kernel level: one call per step index 0 .. STEPS (the last is past the record) — enough for four closed segments and a partial one.  All
accumulator planes live in ONE sentinel-filled buffer with padding columns on both sides of every plane, the window and the
per-segment power in sentinel-padded buffers of their own; after every call on the lattice the whole buffers are compared with the
restatement — bit for bit (torch.equal on fp64; NaN equals NaN), with RANDOM fp64 tables tw and W (plane order and row order cannot
cancel) —, after every call off the lattice with what they held before; `x`, the tables and `step` must be what they were."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

import welch_ref as R                                    # noqa: E402
import graphs4cfd_amd as gfd                             # noqa: E402
from graphs4cfd_amd import ops, synthetic as S           # noqa: E402
from graphs4cfd_amd.nn.model import Rollout              # noqa: E402

DEV = torch.device("cuda", 0)
F32, F64, I32 = torch.float32, torch.float64, torch.int32
SENT, ISENT = -7777.0, -7777
PAD, CLOSED, KEPT = 3, 4, 3          # four closed segments; seg_power has room for three: the fourth must not be written
SEGMENTS = ((2, 2), (2, 1), (7, 7), (8, 8), (8, 4))
WINDOWS = ((0, 1), (2, 1), (0, 3), (1, 3))
REFS = (None, "node", "own", "target")
KINDS = ("int", "offset")


def draw(kind, rng, *shape):
    if kind == "int":
        return torch.from_numpy(rng.integers(-8, 9, shape).astype(np.float32))
    return torch.from_numpy((rng.standard_normal(shape) + 1e4).astype(np.float32))


def same_bits(a, b):
    """Equal element by element, NaN equal to NaN."""
    return a.shape == b.shape and bool(((a == b) | (a.isnan() & b.isnan())).all())


class Buffers:
    """The device buffers of one accumulator — planes, window, per-segment power —, each inside sentinels, and the restatement's state."""

    def __init__(self, n, nf, K, start, reference, track):
        self.n, self.reference, self.track = n, reference, track
        self.buf = torch.full((ops.welch_planes(nf, K, reference), n + 2 * PAD), SENT, dtype=F64, device=DEV)
        self.views = self.buf[:, PAD:PAD + n].split(ops.welch_split(nf, K, reference))
        self.wbuf = torch.full((7,), ISENT, dtype=I32, device=DEV)
        self.window = self.wbuf[2:5]
        self.window.copy_(torch.tensor([start, -1, 0], dtype=I32))
        self.ref = R.new_state(n, nf, K, start, reference, len(track or ()), KEPT, fill=SENT)
        self.sbuf = self.seg_power = self.track_host = self.track_dev = None
        if track:
            self.sbuf = torch.full((KEPT + 2, len(track), nf, K), SENT, dtype=F64, device=DEV)
            self.seg_power = self.sbuf[1:KEPT + 1]
            self.track_host = torch.tensor(track, dtype=I32)
            self.track_dev = self.track_host.to(DEV)

    def snapshot(self):
        return self.buf.clone(), self.wbuf.clone(), None if self.sbuf is None else self.sbuf.clone()

    def unchanged(self, before, what):
        assert same_bits(self.buf, before[0]) and torch.equal(self.wbuf, before[1]), f"{what}: a step off the lattice wrote"
        assert self.sbuf is None or same_bits(self.sbuf, before[2]), f"{what}: a step off the lattice wrote seg_power"

    def check(self, what):
        full = np.full(tuple(self.buf.shape), SENT)
        full[:, PAD:PAD + self.n] = np.concatenate([self.ref[k] for k in R.names(self.ref)])
        if not same_bits(self.buf, torch.from_numpy(full).to(DEV)):
            for k, v in zip(R.names(self.ref), self.views):               # (says which plane; the padding is what is left)
                R.same(v, self.ref[k], f"{what}, {k}")
            raise AssertionError(f"{what}: the padding around the planes was written")
        w = [int(v) for v in self.ref["window"]]
        assert self.wbuf.tolist() == [ISENT, ISENT] + w + [ISENT, ISENT], f"{what}: window {self.wbuf.tolist()} vs {w}"
        if self.sbuf is not None:
            R.same(self.seg_power, self.ref["seg_power"], f"{what}, seg_power")
            assert bool((self.sbuf[0] == SENT).all()) and bool((self.sbuf[-1] == SENT).all()), f"{what}: seg_power was written past its segments"


class Launches:
    """One case: the accumulator of the samples (and, for the "target" kind of reference, the one of the target's columns, launched
    first), the restatement beside them, and one checked call per step."""

    def __init__(self, n, nf, K, L, H, start, stride, x_kind, kind, reference=None, tracked=False, seed=0, poison=False):
        self.n, self.nf, self.K, self.L, self.H, self.stride, self.x_kind, self.kind = n, nf, K, L, H, stride, x_kind, kind
        self.what = f"n {n} nf {nf} K {K} L {L} H {H} window ({start}, {stride}) x {x_kind} {kind} ref {reference} tracked {tracked}"
        self.rng = np.random.default_rng(100000 * L + 1000 * n + 100 * K + 10 * nf + seed)
        # the last sample is the one before a fifth segment would close: four closed segments and a partial one
        self.steps = start + stride * ((CLOSED - 1) * H + L - 1 + H - 1) + 1
        self.reference = reference if n else None
        track = [0, n - 1, 0] if (tracked and n) else None                           # first row, last row, a repeated row
        self.acc = Buffers(n, nf, K, start, self.reference is not None, track)
        self.tgt = Buffers(n, nf, K, start, False, None) if self.reference == "target" else None
        self.ref_row, self.ref_field = {"node": (n - 1, nf - 1), "own": (-1, 0)}.get(self.reference, (-1, -1))
        self.step = torch.zeros(2, dtype=I32, device=DEV)
        self.tw_host, self.W_host = torch.from_numpy(self.rng.standard_normal((L, K, 2))), torch.from_numpy(self.rng.standard_normal((K, 2)))
        self.tw, self.W = self.tw_host.to(DEV), self.W_host.to(DEV)
        self.poison = poison

        def wide():
            t = draw(kind, self.rng, n, nf * self.steps + 5)
            return t[:, :nf * self.steps], t.to(DEV)[:, :nf * self.steps]
        self.x_host = self.x = self.xt_host = self.xt = None
        if x_kind == "padded":
            self.x_host, self.x = wide()
        if self.tgt is not None:
            self.xt_host, self.xt = wide()

    def set_origin(self, origin):
        for b in (self.acc, self.tgt):
            if b is not None:
                b.window.copy_(torch.tensor([origin, -1, 0], dtype=I32))
                b.ref["window"][:] = (origin, -1, 0)

    def launch(self, t, check=True):
        if self.x is None:
            host = draw(self.kind, self.rng, self.n, self.nf)
            if self.poison and self.n:
                host[self.n // 2, 0] = float("nan") if t % 5 == 3 else host[self.n // 2, 0]
                host[0, self.nf - 1] = float("inf") if t == 6 else host[0, self.nf - 1]
                host[self.n - 1, self.nf - 1] = float("-inf") if t == 9 else host[self.n - 1, self.nf - 1]
            dev, x_step = host.to(DEV), 0
        else:
            host, dev, x_step = self.x_host, self.x, self.nf
        kept = dev.clone()
        on = R.sample_index(self.acc.ref, t, self.steps, self.stride) >= 0 and self.n > 0
        before = None if on else [b.snapshot() for b in (self.acc, self.tgt) if b is not None]
        self.step.copy_(torch.tensor([t, 0], dtype=I32))
        a, ref = self.acc, None
        if self.tgt is not None:
            g = self.tgt
            ops.rollout_welch(self.xt, self.step, self.nf, self.steps, g.window, self.tw, self.W, *g.views, hop=self.H, stride=self.stride, x_step=self.nf)
            R.step(g.ref, self.xt_host.numpy(), t, self.steps, self.tw_host.numpy(), self.W_host.numpy(), self.stride, self.H, x_step=self.nf)
            ref = g.views[1:4]
        ops.rollout_welch(dev, self.step, self.nf, self.steps, a.window, self.tw, self.W, *a.views[:5], hop=self.H, stride=self.stride, x_step=x_step,
                          cxr=a.views[5:] if self.reference else None, ref=ref, ref_row=self.ref_row, ref_field=self.ref_field, track=a.track_dev,
                          track_host=a.track_host, seg_power=a.seg_power)
        R.step(a.ref, host.numpy(), t, self.steps, self.tw_host.numpy(), self.W_host.numpy(), self.stride, self.H, x_step=x_step,
               ref=None if not self.reference else (self.tgt.ref if self.tgt is not None else a.ref), ref_row=self.ref_row, ref_field=self.ref_field,
               track=a.track)
        if not check:
            return
        what = f"{self.what} call {t}"
        if not on:
            for b, snap in zip([b for b in (self.acc, self.tgt) if b is not None], before):
                b.unchanged(snap, what)
        else:
            a.check(what)
            if self.tgt is not None:
                self.tgt.check(what + ", target")
        assert self.step.tolist() == [t, 0], f"{what}: step {self.step.tolist()}"
        assert torch.equal(self.tw.cpu(), self.tw_host) and torch.equal(self.W.cpu(), self.W_host), f"{what}: a table was written"
        assert torch.equal(torch.nan_to_num(dev, nan=7.0), torch.nan_to_num(kept, nan=7.0)), f"{what}: x was written"

    def run(self, check=True):
        for t in range(self.steps + 1):
            self.launch(t, check)
        if self.n:
            assert int(self.acc.ref["window"][2]) == CLOSED and self.acc.window.tolist()[2] == CLOSED, self.what
        else:
            assert self.acc.window.tolist() == [int(self.acc.ref["window"][0]), -1, 0]
        return self


@pytest.mark.parametrize("K", [1, 5, 9, 64])
@pytest.mark.parametrize("nf", [1, 3, 8])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 1000])
def test_welch_matches_the_restatement(n, nf, K):
    """Two cases at this (n, nf, K); segment shapes, windows, the form of `x`, the kind of data, the kind of reference and the tracked rows
    go round with the sizes so that every one of them occurs at every n, nf and K (the full product would be hundreds of cases per size)."""
    i = [0, 1, 63, 64, 65, 257, 1000].index(n) + 2 * [1, 3, 8].index(nf) + 3 * [1, 5, 9, 64].index(K)
    for rep in (0, 1):
        i += 3 * rep + 1
        (L, H), (start, stride) = SEGMENTS[i % 5], WINDOWS[(i // 2) % 4]
        Launches(n, nf, K, L, H, start, stride, ("pred", "padded")[(i // 3) % 2], KINDS[i % 2], REFS[(i + rep) % 4], tracked=bool((i // 2) % 2)).run()


@pytest.mark.parametrize("L,H", SEGMENTS)
@pytest.mark.parametrize("reference", REFS)
def test_every_reference_on_every_segment_shape(reference, L, H):
    """n = 257: the reference node 256 is in another workgroup than rows 0 .. 255; K = 9: two bin groups; stride 3 from step 1."""
    for x_kind, kind in (("pred", "offset"), ("padded", "int")):
        Launches(257, 3, 9, L, H, 1, 3, x_kind, kind, reference, tracked=True).run()


@pytest.mark.parametrize("reference", REFS)
def test_nan_and_inf_samples_follow_ieee(reference):
    c = Launches(257, 3, 5, 8, 4, 0, 1, "pred", "int", reference, tracked=True, poison=True).run()
    pxx = c.acc.views[4].unflatten(0, (3, 5))
    assert bool(torch.isnan(pxx[0, :, 128]).all()) and bool(torch.isfinite(pxx[1, :, 128]).all()) and bool(torch.isfinite(pxx[0, :, 127]).all())
    assert not bool(torch.isfinite(pxx[2, :, 0]).any()) and not bool(torch.isfinite(pxx[2, :, 256]).any())
    if reference == "node":          # the reference (row 256, field 2) was poisoned: every cross-spectrum is, and no other power
        assert not bool(torch.isfinite(c.acc.views[5]).any()) and bool(torch.isfinite(pxx[:, :, 1:128]).all())


BIG = 262_144 + 300          # 1024 workgroups of 256: 300 threads take a second row


def test_large_mesh_takes_several_rows_per_thread():
    Launches(BIG, 1, 9, 2, 1, 0, 3, "pred", "offset", "node", tracked=True).run()


def test_two_runs_give_the_same_bits():
    a = Launches(1000, 3, 5, 8, 4, 0, 1, "padded", "offset", "node", tracked=True).run(check=False)
    b = Launches(1000, 3, 5, 8, 4, 0, 1, "padded", "offset", "node", tracked=True).run(check=False)
    assert torch.equal(a.acc.buf, b.acc.buf) and torch.equal(a.acc.sbuf, b.acc.sbuf) and a.acc.window.tolist() == b.acc.window.tolist()
    assert bool((a.acc.buf[:, PAD:-PAD] != SENT).all()) and a.acc.window.tolist() == [0, a.steps - 1, CLOSED]


@pytest.mark.parametrize("x_kind", ["pred", "padded"])
def test_running_through_a_rewritten_origin_replaces_the_record(x_kind):
    c = Launches(257, 3, 5, 8, 4, 0, 1, x_kind, "offset", "node", tracked=True).run()
    before = c.acc.buf.clone()
    c.set_origin(3)
    for t in range(c.steps + 1):            # steps 0 .. 2 are now in front of the window: they leave the old record as it is
        c.launch(t)
        if t < 3:
            assert torch.equal(c.acc.buf, before) and c.acc.window.tolist() == [3, -1, 0]
    assert c.acc.window.tolist() == [3, c.steps - 1, (c.steps - 3 - 8) // 4 + 1] and not torch.equal(c.acc.buf, before)


@pytest.mark.parametrize("nf,K,L,H", [(9, 2, 8, 8), (2, 65, 8, 8), (2, 2, 8, 3), (2, 2, 7, 3), (2, 2, 8, 2)])
def test_what_the_launch_does_not_cover_is_refused(nf, K, L, H):
    n = 50
    buf = torch.full((ops.welch_planes(nf, K, False), n), SENT, dtype=F64, device=DEV)
    window, step = torch.tensor([0, -1, 0], dtype=I32, device=DEV), torch.zeros(2, dtype=I32, device=DEV)
    tw, W = torch.zeros(L, K, 2, dtype=F64, device=DEV), torch.zeros(K, 2, dtype=F64, device=DEV)
    with pytest.raises(NotImplementedError, match="g4c_rollout_welch"):
        ops.rollout_welch(torch.zeros(n, nf, device=DEV), step, nf, 40, window, tw, W, *buf.split(ops.welch_split(nf, K, False)), hop=H)
    assert bool((buf == SENT).all()) and window.tolist() == [0, -1, 0] and step.tolist() == [0, 0]


def test_negative_controls_on_the_launch():
    """The launch's own sums fail the comparison against a restatement with one mistake."""
    c = Launches(257, 3, 5, 8, 4, 1, 2, "padded", "offset", "node", tracked=True).run()
    got = dict(zip(R.names(c.acc.ref), c.acc.views), window=c.acc.window, seg_power=c.acc.seg_power)
    R.same_state(got, c.acc.ref, "launch")
    x = c.x_host.numpy()
    for wrong in (None,) + R.WRONG:
        st = R.new_state(257, 3, 5, 1, True, 3, KEPT, fill=SENT, sets=R.PARITY_SETS if wrong == "parity" else 2)
        for t in range(c.steps + 1):
            R.step(st, x, t, c.steps, c.tw_host.numpy(), c.W_host.numpy(), 2, 4, x_step=3, ref=st, ref_row=256, ref_field=2, track=[0, 256, 0],
                   wrong=wrong)
        assert R.rejects(R.same_state, got, st, str(wrong)) == (wrong is not None), wrong


# ====================================================================== Rollout / GNN.welch / evaluate_welch
N_OUT, NF = 13, 3
L, H = 4, 2
SPEC = dict(bins=[0, 1, 2], overlap=0.5, start=1, dt=0.5)          # samples: the 12 steps 1 .. 12 — five closed segments, none partial


@pytest.fixture(scope="module")
def mesh():
    g = S.mus_graph(3000, levels=3, seed=3).to(DEV)
    g.batch = torch.zeros(g.num_nodes, dtype=torch.long, device=DEV)
    torch.manual_seed(4)
    model = gfd.nn.NsThreeScaleGNN(arch=S.mus_arch("NsThreeScaleGNN", 128), device=DEV)
    model.eval()
    target = torch.randn(g.num_nodes, NF * N_OUT + 2, generator=torch.Generator().manual_seed(5)).to(DEV)
    full = model.solve(g.clone(), N_OUT)
    return dict(g=g, model=model, target=target, full=full)


def samples_of(result, nf=NF):
    r = result.cpu().numpy()
    return [r[:, nf * t:nf * (t + 1)] for t in range(r.shape[1] // nf)]


def rows(a):
    return np.ascontiguousarray(a.T)


def same_as_restatement(we, st, what):
    """The raw sums of a `RolloutWelch` are bit for bit the restatement's state `st`."""
    assert we.segments == int(st["window"][2]) > 0 and we.origin == int(st["window"][0]), (what, we, st["window"])
    assert we.pxx.dtype == F64 and we.pxx.is_cuda
    R.same(we.pxx.flatten(1), rows(st["pxx"]), f"{what}, pxx")
    if "cxr_re" in st:
        R.same(we.cxr_re.flatten(1), rows(st["cxr_re"]), f"{what}, cxr_re")
        R.same(we.cxr_im.flatten(1), rows(st["cxr_im"]), f"{what}, cxr_im")
    else:
        assert we.cxr_re is None and we.cxr_im is None and we.ref_pxx is None
    if "seg_power" in st:
        R.same(we.seg_power, st["seg_power"][:we.segments], f"{what}, seg_power")
    else:
        assert we.seg_power is None


@pytest.mark.parametrize("capture", [True, False])
@pytest.mark.parametrize("reorder", [False, True])
def test_rollout_welch_equals_the_restatement(mesh, reorder, capture):
    """Prediction and target in one rollout, with a node and with the target as the reference: each against the restatement over what
    the same rollout returns, in the caller's numbering."""
    n = int(mesh["g"].num_nodes)
    track = [0, n - 1, 1234, 0]
    for reference in ((n - 2, 1), "target"):
        spec = gfd.Welch(L, reference=reference, track=track, **SPEC)
        with Rollout.open(mesh["model"], mesh["g"], N_OUT, capture=capture, reorder=reorder, every=1, target=mesh["target"], welch=spec,
                          target_welch=True) as ro:
            ro.run(N_OUT)
            assert (ro._perm is not None) == reorder
            res, we, twe = ro.result(), ro.welch(), ro.target_welch()
        what = f"reorder {reorder} capture {capture} reference {reference}"
        if not reorder:
            assert torch.equal(res, mesh["full"])
        tw = ops.spectrum_table(bins=SPEC["bins"], samples=L, dt=0.5, taper="hann")[0].numpy()
        tgt = mesh["target"].cpu().numpy()
        kw = dict(start=1, track=track, max_segments=5)
        if reference == "target":
            st, tg = R.run(samples_of(res), N_OUT, tw, H, reference=("target", tgt), **kw)
        else:
            st, tg = R.run(samples_of(res), N_OUT, tw, H, reference=reference, **kw), R.run(tgt, N_OUT, tw, H, start=1, x_step=NF, steps=N_OUT)
        assert we.segments == 5 and (we.segment, we.hop, we.stride, we.dt, we.taper) == (L, H, 1, 0.5, "hann")
        same_as_restatement(we, st, what)
        same_as_restatement(twe, tg, what + ", target")
        assert we.freqs.tolist() == [0.0, 0.5, 1.0] and torch.equal(we.track, torch.tensor(track))
        want = twe.pxx if reference == "target" else we.pxx[n - 2, 1].reshape(1, 1, -1)
        assert torch.equal(we.ref_pxx, want)
        # the derived quantities are those of the samples, in the caller's rows
        coh = we.coherence
        assert bool((coh[torch.isfinite(coh)] <= 1.0 + 1e-12).all()) and bool(torch.isfinite(coh[:, :, 1:]).all())
        if reference != "target":
            assert torch.equal(coh[n - 2, 1], torch.ones(3, dtype=F64, device=DEV))
        x = torch.stack([res[:, NF * t:NF * (t + 1)].double() for t in range(1, N_OUT)])                  # [12, N, nf]
        seg = torch.stack([x[s * H:s * H + L] for s in range(5)])                                         # [5, L, N, nf]
        e = torch.complex(torch.from_numpy(tw[..., 0]), torch.from_numpy(tw[..., 1])).to(DEV)             # [L, K]
        a = torch.einsum("sqnf,qk->snfk", (seg - seg.mean(1, keepdim=True)).to(torch.complex128), e)
        power = (a.real ** 2 + a.imag ** 2).mean(0) / we.S ** 2
        assert float((we.power - power).abs().max()) <= 1e-12 * float(power.max())
        assert float((we.spectrogram - (a.real ** 2 + a.imag ** 2)[:, track] / we.S ** 2).abs().max()) <= 1e-12 * float(power.max())
        assert we.dominant() in we.freqs.tolist() and tuple(we.band_power().shape) == (NF, 3) and tuple(we.dominant_by_segment(2, 1).shape) == (5,)
        assert torch.allclose(we.psd, we.power * (we.S ** 2 / (2.0 * we.S2)) * torch.tensor([1.0, 2.0, 1.0], dtype=F64, device=DEV), rtol=1e-14, atol=0)


LAUNCHES = ("mesh_derived", "rollout_moments", "sample_points", "rollout_spectrum", "rollout_welch", "body_forces", "tracer_advance",
            "rollout_advance_record", "rollout_advance")


def test_a_rollout_without_welch_is_what_it_was(mesh, monkeypatch):
    calls = []

    def recorded(name, fn):
        def call(*a, **k):
            calls.append(name)
            return fn(*a, **k)
        return call

    for name in LAUNCHES:
        monkeypatch.setattr(ops, name, recorded(name, getattr(ops, name)))
    with Rollout.open(mesh["model"], mesh["g"], N_OUT, capture=False, reorder=False, spectrum=gfd.Spectrum([1]), welch=gfd.Welch(L, **SPEC)) as ro:
        ro.run(2)
        assert calls == ["rollout_spectrum", "rollout_welch", "rollout_advance"] * 2          # behind the spectra, in front of the closing launch
        ro.run(N_OUT - 2)
        with_welch = ro.result().clone()
    del calls[:]
    with Rollout(mesh["model"], mesh["g"], N_OUT, capture=False, reorder=False, spectrum=gfd.Spectrum([1])) as ro:
        ro.run(2)
        assert calls == ["rollout_spectrum", "rollout_advance"] * 2                           # the launches of a step, as before
        ro.run(N_OUT - 2)
        assert ro._welch is None and torch.equal(ro.result(), mesh["full"])
        for name in ("welch", "target_welch"):
            with pytest.raises(RuntimeError, match=name):
                getattr(ro, name)()
    assert torch.equal(with_welch, mesh["full"])
    del calls[:]
    assert torch.equal(mesh["model"].solve(mesh["g"].clone(), N_OUT), mesh["full"]) and "rollout_welch" not in calls


def test_rewind_leaves_the_segments_closed_since(mesh):
    g, f0 = mesh["g"], mesh["g"].field
    spec = gfd.Welch(L, [0, 1], overlap=0.5, stride=2, taper="rect", reference="target")
    tw = ops.spectrum_table(bins=[0, 1], samples=L, stride=2, taper="rect")[0].numpy()
    tgt = mesh["target"].cpu().numpy()
    try:
        with Rollout.open(mesh["model"], g, N_OUT, reorder=False, every=1, target=mesh["target"], welch=spec) as ro:
            ro.run(9)                                     # samples at steps 0, 2, 4, 6, 8: one closed segment, a second one open
            first = ro.welch()
            same_as_restatement(first, R.run(samples_of(ro.result())[:9], N_OUT, tw, H, stride=2, reference=("target", tgt))[0], "before rewind")
            assert first.segments == 1
            with pytest.raises(RuntimeError, match="target_welch"):
                ro.target_welch()                         # (the target's accumulator is there for the reference; its result was not asked for)
            ro.rewind()                                   # the device step index is 1 again: slots 1, 2, ... are written next
            assert ro.welch().segments == 0
            ro.run(12)
            res, we = ro.result(), ro.welch()
        after = samples_of(res)[1:13]                     # samples at steps 2, 4, ..., 12: six — two closed segments
        same_as_restatement(we, R.run(after, N_OUT, tw, H, stride=2, first=1, reference=("target", tgt))[0], "after rewind")
        assert we.origin == 2 and we.segments == 2 and not torch.equal(we.pxx, first.pxx)
    finally:
        g.field = f0


def test_a_clipped_rollout_leaves_the_welch_spectrum_of_its_recomputation(mesh):
    """Inputs of 1e5 leave the fp16 range: the steps are computed again in bf16x6 and the segments start again with them."""
    g, f0 = mesh["g"], mesh["g"].field

    def run(precision=None):
        old = ops.set_mlp_precision(precision) if precision else None
        try:
            g.field = f0 * 1e5
            with Rollout.open(mesh["model"], g, N_OUT, reorder=False, every=1, welch=gfd.Welch(L, reference=(7, 0), track=[7], **SPEC)) as ro:
                ro.run(N_OUT)
                return ro.result().clone(), ro.welch(), ro
        finally:
            g.field = f0
            if old:
                ops.set_mlp_precision(old)

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res, we, ro = run()
        res_x, we_x, ro_x = run("bf16x6")
    assert ro.exact_range and not ro_x.exact_range and bool(torch.isfinite(res).all()) and torch.equal(res, res_x)
    tw = ops.spectrum_table(bins=SPEC["bins"], samples=L, dt=0.5, taper="hann")[0].numpy()
    same_as_restatement(we, R.run(samples_of(res), N_OUT, tw, H, start=1, reference=(7, 0), track=[7], max_segments=5), "clipped")
    assert we.segments == we_x.segments == 5 and torch.equal(we.pxx, we_x.pxx) and torch.equal(we.cxr_im, we_x.cxr_im)
    assert torch.equal(we.seg_power, we_x.seg_power)


def test_gnn_welch_and_evaluate_welch(mesh):
    g, model, full = mesh["g"].clone(), mesh["model"], mesh["full"]
    g.target = mesh["target"][:, :NF * N_OUT].contiguous()
    tw = ops.spectrum_table(bins=SPEC["bins"], samples=L, dt=0.5, taper="hann")[0].numpy()
    kw = dict(bins=SPEC["bins"], overlap=0.5, discard=1, dt=0.5)
    we = model.welch(g.clone(), N_OUT, L, track=[5], **kw)
    assert type(we) is gfd.nn.RolloutWelch and we.target is None and we.cxr_re is None and (we.segments, we.origin, we.stride) == (5, 1, 1)
    same_as_restatement(we, R.run(samples_of(full), N_OUT, tw, H, start=1, track=[5], max_segments=5), "GNN.welch")
    with Rollout.open(model, g.clone(), N_OUT, reorder=False, welch=gfd.Welch(L, track=[5], **SPEC)) as ro:
        ro.run(N_OUT)
        direct = ro.welch()
    for name in ("pxx", "seg_power", "w", "freqs", "track"):
        assert torch.equal(getattr(we, name), getattr(direct, name)), name
    tgt = g.target.cpu().numpy()
    st, tg = R.run(samples_of(full), N_OUT, tw, H, start=1, reference=("target", tgt))
    against = model.welch(g.clone(), N_OUT, L, reference="target", capture=False, **kw)
    same_as_restatement(against, st, "GNN.welch, target")
    same_as_restatement(against.target, tg, "GNN.welch, the target's")
    assert torch.equal(against.pxx, we.pxx) and torch.equal(against.ref_pxx, against.target.pxx)
    only = model.welch(g.clone(), N_OUT, L, target=True, **kw)
    assert only.cxr_re is None and torch.equal(only.target.pxx, against.target.pxx)
    with pytest.raises(ValueError, match="welch"):
        model.welch(g.clone(), N_OUT, 2 * N_OUT, [1])
    errs = model.evaluate(g.clone())
    assert errs.welch is None and errs.target_welch is None
    both = model.evaluate_welch(g.clone(), gfd.Welch(L, reference="target", **SPEC))
    assert torch.equal(both.sums, errs.sums)
    same_as_restatement(both.welch, st, "evaluate_welch")
    same_as_restatement(both.target_welch, tg, "evaluate_welch, target")
    coh = both.welch.coherence
    assert tuple(coh.shape) == (int(g.num_nodes), NF, 3) and bool((coh[torch.isfinite(coh)] <= 1.0 + 1e-12).all())


def test_list_of_two_graphs():
    gen = torch.Generator().manual_seed(8)
    graphs = [S.mus_graph(n, levels=1, seed=20 + n).to(DEV) for n in (300, 500)]
    for gr in graphs:
        gr.target = torch.randn(gr.num_nodes, NF * N_OUT, generator=gen).to(DEV)
    torch.manual_seed(9)
    model = gfd.nn.NsOneScaleGNN(arch=S.mus_arch("NsOneScaleGNN", 64), device=DEV)
    full = model.solve([gr.clone() for gr in graphs], N_OUT)
    tw = ops.spectrum_table(bins=[0, 2], samples=L, taper="hann")[0].numpy()
    we = model.welch([gr.clone() for gr in graphs], N_OUT, L, [0, 2], reference=(799, 2), track=[799, 0, 300])          # rows of the collated graph
    assert tuple(we.pxx.shape) == (800, NF, 2) and we.segments == 3
    same_as_restatement(we, R.run(samples_of(full), N_OUT, tw, L, reference=(799, 2), track=[799, 0, 300], max_segments=3), "two graphs")
    errs = model.evaluate_welch([gr.clone() for gr in graphs], gfd.Welch(L, [0, 2], reference="target"))
    target = torch.cat([gr.target for gr in graphs]).cpu().numpy()
    st, tg = R.run(samples_of(full), N_OUT, tw, L, reference=("target", target))
    same_as_restatement(errs.welch, st, "two graphs, evaluate_welch")
    same_as_restatement(errs.target_welch, tg, "two graphs, target")


@pytest.mark.parametrize("L,H", [(8, 8), (8, 4), (2, 1)])
def test_coherence_is_at_most_one(L, H):
    """Cauchy-Schwarz over the segments, up to rounding: |Σ A conj R|² <= Σ|A|² Σ|R|² (1 + 1e-12), on data with a large common offset."""
    n, nf, K, segments = 1000, 2, min(L // 2 + 1, 5), 6
    steps = (segments - 1) * H + L
    tw, w, freqs = ops.spectrum_table(bins=list(range(K)), samples=L, taper="hann")
    rng = np.random.default_rng(L + H)
    x = torch.from_numpy((rng.standard_normal((n, nf * steps)) + 1e3).astype(np.float32)).to(DEV)
    planes = torch.zeros(ops.welch_planes(nf, K, True), n, dtype=F64, device=DEV).split(ops.welch_split(nf, K, True))
    window, step = torch.tensor([0, -1, 0], dtype=I32, device=DEV), torch.zeros(2, dtype=I32, device=DEV)
    for t in range(steps):
        step[:1].fill_(t)
        ops.rollout_welch(x, step, nf, steps, window, tw.to(DEV), ops.welch_weights(tw).to(DEV), *planes[:5], hop=H, x_step=nf, cxr=planes[5:],
                          ref_row=n // 2, ref_field=1)
    assert window.tolist() == [0, steps - 1, segments]
    pxx = planes[4].unflatten(0, (nf, K))
    coh = (planes[5] ** 2 + planes[6] ** 2).unflatten(0, (nf, K)) / (pxx * pxx[1, :, n // 2].reshape(1, K, 1))
    finite = torch.isfinite(coh)
    assert bool(finite[:, 1:].all()) and bool((coh[finite] <= 1.0 + 1e-12).all()) and float(coh[finite].min()) >= 0.0
