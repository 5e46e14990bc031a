"""g4c_rollout_spectrum (csrc/rollout_spectrum.hip) through ops.rollout_spectrum against the fp64 restatement of tests/spectrum_ref.py,
and the spectra of `Rollout(spectrum=, target_spectrum=, derived_spectrum=)` / `GNN.spectrum` / `GNN.evaluate(spectrum=)` against the
restatement run over the rollout's own `result()`, target and derived snapshots.

Kernel level: nine launches with the step index set by hand to 0 .. 8 against max_steps = 8 (the ninth is past the record).  All
accumulator planes live in ONE sentinel-filled buffer with padding columns on both sides of every plane, the window in a padded
buffer of its own; after every launch the whole buffers are compared with the restatement — bit for bit (torch.equal on fp64), on
small integers and on float data with a common offset of 1e4 alike, with a RANDOM fp64 table (plane order and row order cannot
cancel): every accumulator gets one add per step in time order — and `x`, `tw` and `step` must be what they were."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

import spectrum_ref as R                                 # noqa: E402
import graphs4cfd_amd as gfd                             # noqa: E402
from graphs4cfd_amd import ops, synthetic as S           # noqa: E402
from graphs4cfd_amd.nn.model import Rollout              # noqa: E402

DEV = torch.device("cuda", 0)
F32, F64, I32 = torch.float32, torch.float64, torch.int32
SENT, ISENT = -7777.0, -7777
STEPS, PAD = 8, 3
WINDOWS = ((0, 1), (2, 1), (0, 3), (2, 3))
XS = ("pred", "dense", "padded")
KINDS = ("int", "offset")


def draw(kind, rng, *shape):
    if kind == "int":
        return torch.from_numpy(rng.integers(-8, 9, shape).astype(np.float32))
    return torch.from_numpy((rng.standard_normal(shape) + 1e4).astype(np.float32))


class Launches:
    """The device buffers of one case, the restatement's state beside them, and one checked launch."""

    def __init__(self, n, nf, K, start, stride, x_kind, kind, short=0, seed=0):
        self.n, self.nf, self.K, self.stride, self.x_kind = n, nf, K, stride, x_kind
        self.what = f"n {n} nf {nf} K {K} window ({start}, {stride}) short {short} x {x_kind} {kind}"
        self.rng, self.kind = np.random.default_rng(1000 * n + 100 * K + 10 * nf + seed), kind
        self.samples = max(len(range(start, STEPS, stride)) - short, 1)
        self.sizes = (nf, nf, nf * K, nf * K)
        self.buf = torch.full((ops.spectrum_planes(nf, K), n + 2 * PAD), SENT, dtype=F64, device=DEV)
        self.views = self.buf[:, PAD:PAD + n].split(self.sizes)
        self.wbuf = torch.full((6,), ISENT, dtype=I32, device=DEV)
        self.window = self.wbuf[2:4]
        self.window.copy_(torch.tensor([start, -1], dtype=I32))
        self.step = torch.zeros(2, dtype=I32, device=DEV)
        self.tw_host = torch.from_numpy(self.rng.standard_normal((self.samples, K, 2)))
        self.tw = self.tw_host.to(DEV)
        self.x = self.x_host = None
        if x_kind != "pred":
            wide = draw(kind, self.rng, n, nf * STEPS + (5 if x_kind == "padded" else 0))
            self.x_host = wide[:, :nf * STEPS]
            self.x = wide.to(DEV)[:, :nf * STEPS]
            self.x_dev0 = self.x.clone()
        self.ref = R.new_state(n, nf, K, start, fill=SENT)

    def set_origin(self, origin):
        self.window.copy_(torch.tensor([origin, -1], dtype=I32))
        self.ref["window"][:] = (origin, -1)

    def expected(self):
        full = np.full(tuple(self.buf.shape), SENT)
        full[:, PAD:PAD + self.n] = np.concatenate([self.ref[k] for k in R.NAMES])
        return torch.from_numpy(full)

    def launch(self, t, check=True):
        if self.x is None:
            host = draw(self.kind, self.rng, self.n, self.nf)
            dev, x_step = host.to(DEV), 0
        else:
            host, dev, x_step = self.x_host, self.x, self.nf
        self.step.copy_(torch.tensor([t, 0], dtype=I32))
        ops.rollout_spectrum(dev, self.step, self.nf, STEPS, self.window, self.tw, *self.views, stride=self.stride, x_step=x_step)
        self.ref = R.accumulate(self.ref, host.numpy(), t, STEPS, self.tw_host.numpy(), self.stride, x_step)
        if not check:
            return
        what = f"{self.what} launch {t}"
        if not torch.equal(self.buf, self.expected().to(DEV)):
            for k, v in zip(R.NAMES, self.views):                      # (says which plane; the padding is what is left)
                R.same(v, self.ref[k], f"{what}, {k}")
            raise AssertionError(f"{what}: the padding around the planes was written")
        w = self.ref["window"]
        assert self.wbuf.tolist() == [ISENT, ISENT, int(w[0]), int(w[1]), ISENT, ISENT], f"{what}: window {self.wbuf.tolist()} vs {w}"
        assert self.step.tolist() == [t, 0], f"{what}: step {self.step.tolist()}"
        assert torch.equal(self.tw.cpu(), self.tw_host), f"{what}: tw was written"
        if self.x is None:
            assert torch.equal(dev.cpu(), host), f"{what}: x was written"
        else:
            assert torch.equal(self.x, self.x_dev0), f"{what}: x was written"

    def run(self, check=True):
        for t in range(STEPS + 1):
            self.launch(t, check)
        return self


@pytest.mark.parametrize("K", [1, 2, 5, 64])
@pytest.mark.parametrize("nf", [1, 3, 8])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1000])
def test_spectrum_matches_the_restatement(n, nf, K):
    """Every window, full and one sample short, at this (n, nf, K); the form of `x` and the kind of data go round with the windows so
    that every pairing of them occurs at this size (2 x 4 x 3 x 2 cases of nine checked launches would be 48 per size: 8 are run)."""
    i = 0
    for short in (0, 1):
        for start, stride in WINDOWS:
            x_kind, kind = XS[(i + n + K) % 3], KINDS[(i // 3 + nf) % 2]
            i += 1
            c = Launches(n, nf, K, start, stride, x_kind, kind, short=short).run()
            lattice = [t for t in range(start, STEPS, stride)][:c.samples]
            assert c.window.tolist() == [start, lattice[-1] if n else -1]
            if n:
                assert R.count(c.ref, stride) == c.samples == len(lattice)
                if short and len(range(start, STEPS, stride)) > 1:
                    assert lattice[-1] < max(range(start, STEPS, stride))          # the last lattice step touched nothing


@pytest.mark.parametrize("x_kind", XS)
@pytest.mark.parametrize("kind", KINDS)
def test_every_form_of_x_on_both_kinds_of_data(x_kind, kind):
    for start, stride in WINDOWS:
        for short in (0, 1):
            Launches(257, 3, 5, start, stride, x_kind, kind, short=short).run()
            Launches(65, 8, 9, start, stride, x_kind, kind, short=short).run()


BIG = 262_144 + 300          # 1024 workgroups of 256: 300 threads take a second row


@pytest.mark.parametrize("nf,K,window,x_kind,kind", [(1, 2, (2, 3), "padded", "offset"), (1, 9, (0, 3), "pred", "offset")])
def test_large_mesh_takes_several_rows_per_thread(nf, K, window, x_kind, kind):
    """K = 9: two bin groups on the grid's second axis, the second of one bin, each thread of both taking two rows."""
    Launches(BIG, nf, K, window[0], window[1], x_kind, kind).run()


def test_two_runs_give_the_same_bits():
    a = Launches(1000, 3, 5, 0, 1, "padded", "offset").run(check=False)
    b = Launches(1000, 3, 5, 0, 1, "padded", "offset").run(check=False)
    assert torch.equal(a.buf, b.buf) and a.window.tolist() == b.window.tolist() == [0, STEPS - 1]
    assert bool((a.buf[:, PAD:-PAD] != SENT).all())


@pytest.mark.parametrize("x_kind", ["pred", "padded"])
def test_running_through_a_rewritten_origin_replaces_the_record(x_kind):
    c = Launches(257, 3, 5, 0, 1, x_kind, "offset").run()
    before = c.buf.clone()
    c.set_origin(3)
    for t in range(STEPS + 1):            # steps 0 .. 2 are now in front of the window: they leave the old record as it is
        c.launch(t)
        if t < 3:
            assert torch.equal(c.buf, before) and c.window.tolist() == [3, -1]
    assert c.window.tolist() == [3, STEPS - 1] and not torch.equal(c.buf, before)
    assert R.count(c.ref, 1) == STEPS - 3


@pytest.mark.parametrize("nf,K", [(9, 2), (2, 65)])
def test_nine_fields_and_sixty_five_bins_are_refused(nf, K):
    n = 50
    buf = torch.full((ops.spectrum_planes(nf, K), n), SENT, dtype=F64, device=DEV)
    window, step = torch.tensor([0, -1], dtype=I32, device=DEV), torch.zeros(2, dtype=I32, device=DEV)
    tw = torch.zeros(STEPS, K, 2, dtype=F64, device=DEV)
    with pytest.raises(NotImplementedError, match="g4c_rollout_spectrum"):
        ops.rollout_spectrum(torch.zeros(n, nf, device=DEV), step, nf, STEPS, window, tw, *buf.split((nf, nf, nf * K, nf * K)))
    assert bool((buf == SENT).all()) and window.tolist() == [0, -1] and step.tolist() == [0, 0]


def test_negative_controls_on_the_launch():
    """The launch's own sums fail the comparison against a restatement with one mistake."""
    c = Launches(257, 3, 5, 1, 2, "padded", "offset").run()
    got = dict(zip(R.NAMES, c.views), window=c.window)
    R.same_state(got, c.ref, "launch")
    rng = np.random.default_rng(1000 * 257 + 100 * 5 + 10 * 3)          # the case's draws again: the table first, then x
    tw = rng.standard_normal((c.samples, 5, 2))
    x = draw("offset", rng, 257, 3 * STEPS + 5).numpy()                 # (all its columns: "x-step" reads past the record's)
    for wrong in (None,) + R.WRONG:
        st = R.new_state(257, 3, 5, 1, fill=SENT)
        for t in range(STEPS + 1):
            st = R.accumulate(st, x, t, STEPS, tw, 2, 3, wrong=wrong)
        assert R.rejects(R.same_state, got, st, str(wrong)) == (wrong is not None), wrong


# ====================================================================== Rollout / GNN.spectrum / evaluate
N_OUT, NF = 7, 3
SPEC = dict(freqs=[0.0, 0.1, 0.25, 0.4, 0.5], start=1, stride=1, taper="hann")          # samples default to the 6 steps 1 .. 6


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


def same_as_restatement(sp, st, stride, what):
    """The raw sums of a `RolloutSpectrum` are bit for bit the restatement's state `st`."""
    assert sp.count == R.count(st, stride) > 0 and sp.origin == int(st["window"][0]) and sp.stride == stride, (what, sp)
    nf, K = sp.fields, int(sp.tw.size(1))
    for k, got in zip(R.NAMES, (sp.pivot, sp.sum, sp.re.flatten(1), sp.im.flatten(1))):
        assert got.dtype == F64 and got.is_cuda
        R.same(got, np.ascontiguousarray(st[k].T), f"{what}, {k}")
    assert tuple(sp.re.shape) == (int(sp.pivot.size(0)), nf, K)


@pytest.mark.parametrize("capture", [True, False])
@pytest.mark.parametrize("reorder", [False, True])
def test_rollout_spectra_equal_the_restatement(mesh, reorder, capture):
    """Prediction, target and derived columns in one rollout: each against the restatement over what the same rollout returns."""
    spec, dspec = gfd.Spectrum(**SPEC), gfd.Spectrum([0, 1], start=0, stride=2, samples=3)
    with Rollout(mesh["model"], mesh["g"], N_OUT, capture=capture, reorder=reorder, every=1, target=mesh["target"], spectrum=spec,
                 target_spectrum=True, derived=("vort",), derived_every=1, derived_spectrum=dspec) as ro:
        ro.run(N_OUT)
        assert (ro._perm is not None) == reorder
        res, sp, tsp, dsp, der = ro.result(), ro.spectrum(), ro.target_spectrum(), ro.derived_spectrum(), ro.derived()
    what = f"reorder {reorder} capture {capture}"
    if not reorder:
        assert torch.equal(res, mesh["full"])
    tw = sp.tw.numpy()
    assert sp.complete and sp.samples == 6 and sp.taper == "hann" and torch.equal(sp.tw, tsp.tw) and sp.tw.device.type == "cpu"
    same_as_restatement(sp, R.run(samples_of(res), N_OUT, tw, 1, 1), 1, what)
    same_as_restatement(tsp, R.run(mesh["target"].cpu().numpy(), N_OUT, tw, 1, 1, x_step=NF, steps=N_OUT), 1, what + ", target")
    assert tuple(der.snapshots.shape) == (mesh["g"].num_nodes, N_OUT) and dsp.fields == 1 and dsp.count == 3 and dsp.complete
    same_as_restatement(dsp, R.run(samples_of(der.snapshots, 1), N_OUT, dsp.tw.numpy(), 0, 2), 2, what + ", derived")
    # the derived quantities are those of the samples on the window, in the caller's rows
    x = torch.stack([res[:, NF * t:NF * (t + 1)].double() for t in range(1, 7)])                     # [6, N, nf]
    e = torch.complex(sp.tw[..., 0], sp.tw[..., 1]).to(DEV)                                          # [6, K]
    want = torch.einsum("jnf,jk->nfk", (x - x.mean(0)).to(torch.complex128), e) / float(sp.w.sum())
    assert torch.allclose(sp.mean, x.mean(0), rtol=1e-12, atol=1e-12)
    assert float((sp.coeff - want).abs().max()) <= 1e-10 * float(x.abs().max())
    assert sp.dominant() in sp.freqs.tolist() and tuple(sp.band_power().shape) == (NF, 5)


def test_a_rollout_without_spectrum_is_what_it_was(mesh, monkeypatch):
    with Rollout(mesh["model"], mesh["g"], N_OUT, reorder=False, spectrum=gfd.Spectrum(**SPEC)) as ro:
        ro.run(N_OUT)
        with_spectrum = ro.result().clone()

    def refuse(*a, **k):
        raise AssertionError("a rollout without spectrum launched rollout_spectrum")
    monkeypatch.setattr(ops, "rollout_spectrum", refuse)
    with Rollout(mesh["model"], mesh["g"], N_OUT, reorder=False) as ro:
        ro.run(N_OUT)
        assert ro._spectrum is None and ro._target_spectrum is None and torch.equal(ro.result(), mesh["full"])
        for name in ("spectrum", "target_spectrum", "derived_spectrum"):
            with pytest.raises(RuntimeError, match=name):
                getattr(ro, name)()
    assert torch.equal(with_spectrum, mesh["full"])
    assert torch.equal(mesh["model"].solve(mesh["g"].clone(), N_OUT), mesh["full"])
    with pytest.raises(AssertionError, match="rollout_spectrum"):
        with Rollout(mesh["model"], mesh["g"], N_OUT, reorder=False, spectrum=gfd.Spectrum([1])) as ro:
            ro.run(1)


def test_rewind_leaves_the_spectra_of_the_steps_since(mesh):
    g, f0 = mesh["g"], mesh["g"].field
    spec = gfd.Spectrum([0, 1], start=0, stride=2, samples=3)
    try:
        with Rollout(mesh["model"], g, N_OUT, reorder=False, every=1, target=mesh["target"], spectrum=spec, target_spectrum=True) as ro:
            ro.run(3)
            first = ro.spectrum()
            same_as_restatement(first, R.run(samples_of(ro.result())[:3], N_OUT, first.tw.numpy(), 0, 2), 2, "before rewind")
            assert first.count == 2 and not first.complete
            ro.rewind()                                   # the device step index is 1 again: slots 1, 2, ... are written next
            assert ro.spectrum().count == 0 and ro.target_spectrum().count == 0
            ro.run(4)
            res, sp, tsp = ro.result(), ro.spectrum(), ro.target_spectrum()
        after = samples_of(res)[1:5]
        same_as_restatement(sp, R.run(after, N_OUT, sp.tw.numpy(), 0, 2, first=1), 2, "after rewind")
        tgt = R.new_state(g.num_nodes, NF, 2, 2)
        for t in range(1, 5):
            tgt = R.accumulate(tgt, mesh["target"].cpu().numpy(), t, N_OUT, sp.tw.numpy(), 2, NF)
        same_as_restatement(tsp, tgt, 2, "after rewind, target")
        assert sp.origin == 2 and sp.count == 2 and not torch.equal(sp.pivot, first.pivot)
    finally:
        g.field = f0


def test_a_clipped_rollout_leaves_the_spectrum_of_its_recomputation(mesh):
    """Inputs of 1e5 leave the fp16 range: the steps are computed again in bf16x6 and the spectra restart with them."""
    g, f0 = mesh["g"], mesh["g"].field

    def run(precision=None):
        old = ops.set_mlp_precision(precision) if precision else None
        try:
            g.field = f0 * 1e5
            with Rollout(mesh["model"], g, N_OUT, reorder=False, every=1, spectrum=gfd.Spectrum(**SPEC)) as ro:
                ro.run(N_OUT)
                return ro.result().clone(), ro.spectrum(), ro
        finally:
            g.field = f0
            if old:
                ops.set_mlp_precision(old)

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res, sp, ro = run()
        res_x, sp_x, ro_x = run("bf16x6")
    assert ro.exact_range and not ro_x.exact_range and bool(torch.isfinite(res).all()) and torch.equal(res, res_x)
    same_as_restatement(sp, R.run(samples_of(res), N_OUT, sp.tw.numpy(), 1, 1), 1, "clipped")
    assert sp.count == sp_x.count and torch.equal(sp.re, sp_x.re) and torch.equal(sp.im, sp_x.im) and torch.equal(sp.sum, sp_x.sum)


def test_gnn_spectrum_and_evaluate(mesh):
    g, model, full = mesh["g"].clone(), mesh["model"], mesh["full"]
    g.target = mesh["target"][:, :NF * N_OUT].contiguous()
    kw = dict(freqs=SPEC["freqs"], discard=1, taper="hann")
    sp = model.spectrum(g.clone(), N_OUT, **kw)
    assert type(sp) is gfd.nn.RolloutSpectrum and sp.snapshots is None and sp.derived is None and (sp.count, sp.origin, sp.stride) == (6, 1, 1)
    same_as_restatement(sp, R.run(samples_of(full), N_OUT, sp.tw.numpy(), 1, 1), 1, "GNN.spectrum")
    with Rollout(model, g.clone(), N_OUT, reorder=False, spectrum=gfd.Spectrum(**SPEC)) as ro:
        ro.run(N_OUT)
        direct = ro.spectrum()
    for name in ("pivot", "sum", "re", "im", "tw", "w", "freqs"):
        assert torch.equal(getattr(sp, name), getattr(direct, name)), name
    kept = model.spectrum(g.clone(), N_OUT, every=1, capture=False, derived=("vort",), **kw)
    assert torch.equal(kept.snapshots, full) and torch.equal(kept.re, sp.re) and torch.equal(kept.pivot, sp.pivot)
    assert type(kept.derived) is gfd.nn.RolloutSpectrum and kept.derived.fields == 1 and kept.derived.count == 6
    by_bins = model.spectrum(g.clone(), N_OUT, bins=[0, 1, 2, 3], dt=0.5)
    assert by_bins.samples == N_OUT and by_bins.freqs.tolist() == [b / (N_OUT * 0.5) for b in range(4)] and by_bins.complete
    with pytest.raises(ValueError, match="spectrum"):
        model.spectrum(g.clone(), N_OUT, bins=[1], discard=N_OUT)
    errs = model.evaluate(g.clone())
    assert errs.spectrum is None and errs.target_spectrum is None
    both = model.evaluate(g.clone(), spectrum=gfd.Spectrum(**SPEC))
    assert torch.equal(both.sums, errs.sums) and torch.equal(both.spectrum.re, sp.re) and torch.equal(both.spectrum.sum, sp.sum)
    same_as_restatement(both.target_spectrum, R.run(g.target.cpu().numpy(), N_OUT, sp.tw.numpy(), 1, 1, x_step=NF, steps=N_OUT), 1, "evaluate, target")


def test_list_of_two_graphs():
    gen = torch.Generator().manual_seed(8)
    graphs = [S.mus_graph(n, levels=1, seed=20 + n).to(DEV) for n in (300, 500)]
    for gr in graphs:
        gr.target = torch.randn(gr.num_nodes, NF * N_OUT, generator=gen).to(DEV)
    torch.manual_seed(9)
    model = gfd.nn.NsOneScaleGNN(arch=S.mus_arch("NsOneScaleGNN", 64), device=DEV)
    full = model.solve([gr.clone() for gr in graphs], N_OUT)
    sp = model.spectrum([gr.clone() for gr in graphs], N_OUT, bins=[0, 1], discard=1, stride=2)
    assert tuple(sp.re.shape) == (800, NF, 2)
    same_as_restatement(sp, R.run(samples_of(full), N_OUT, sp.tw.numpy(), 1, 2), 2, "two graphs")
    errs = model.evaluate([gr.clone() for gr in graphs], spectrum=gfd.Spectrum([0, 3]))
    target = torch.cat([gr.target for gr in graphs]).cpu().numpy()
    same_as_restatement(errs.target_spectrum, R.run(target, N_OUT, errs.spectrum.tw.numpy(), 0, 1, x_step=NF, steps=N_OUT), 1, "two graphs, target")
