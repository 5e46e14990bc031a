"""g4c_rollout_moments (csrc/rollout_moments.hip) through ops.rollout_moments against the fp64 restatement of tests/moments_ref.py, and
the time statistics of `Rollout(moments=, error_moments=)` / `GNN.time_statistics` / `GNN.evaluate(moments=)` against the restatement
run over the rollout's own `result()`.

Kernel level: nine launches with the step index set by hand to 0 .. 8 against max_steps = 8 (the ninth is past the record).  All
accumulator planes live in ONE sentinel-filled buffer with padding columns on both sides of every plane, the window in a padded
buffer of its own; after every launch the whole buffers are compared with the restatement — bit for bit (torch.equal on fp64), on
small integers and on float data with a common offset of 1e4 alike: every accumulator gets one add per step in time order — and
`pred`, `sub` and `step` must be what they were."""
import os
import sys
import warnings

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

import moments_ref as M                                  # noqa: E402
import graphs4cfd_amd as gfd                             # noqa: E402
from graphs4cfd_amd import _lib, ops, synthetic as S     # noqa: E402
from graphs4cfd_amd.nn.model import Rollout              # noqa: E402

DEV = torch.device("cuda", 0)
F32, F64, I32 = torch.float32, torch.float64, torch.int32
SENT, ISENT = -7777.0, -7777
STEPS, PAD = 8, 3
WINDOWS = ((0, 1), (2, 1), (0, 3), (2, 3))
SUBS = (None, "dense", "padded")
KINDS = ("int", "offset")


def draw(kind, rng, *shape):
    if kind == "int":
        return torch.from_numpy(rng.integers(-8, 9, shape).astype(np.float32))
    return torch.from_numpy((rng.standard_normal(shape) + 1e4).astype(np.float32))


class Launches:
    """The device buffers of one case, the restatement's state beside them, and one checked launch."""

    def __init__(self, n, nf, start, stride, sub_kind, kind, seed=0):
        self.n, self.nf, self.stride, self.what = n, nf, stride, f"n {n} nf {nf} window ({start}, {stride}) sub {sub_kind} {kind}"
        self.rng, self.kind = np.random.default_rng(1000 * n + 10 * nf + seed), kind
        pairs = ops.moment_pairs(nf)
        self.sizes = (nf, nf, pairs, nf, nf)
        self.buf = torch.full((4 * nf + pairs, n + 2 * PAD), SENT, dtype=F64, device=DEV)
        self.views = self.buf[:, PAD:PAD + n].split(self.sizes)
        self.wbuf = torch.full((6,), ISENT, dtype=I32, device=DEV)
        self.window = self.wbuf[2:4]
        self.window.copy_(torch.tensor([start, -1], dtype=I32))
        self.step = torch.zeros(2, dtype=I32, device=DEV)
        self.sub = self.sub_host = None
        if sub_kind is not None:
            wide = draw(kind, self.rng, n, nf * STEPS + (5 if sub_kind == "padded" else 0))
            self.sub_host = wide[:, :nf * STEPS]
            self.sub = wide.to(DEV)[:, :nf * STEPS]
            self.sub_dev0 = self.sub.clone()
        self.ref = M.new_state(n, nf, start, fill=SENT)

    def set_origin(self, origin):
        self.window.copy_(torch.tensor([origin, -1], dtype=I32))
        self.ref["window"][:] = (origin, -1)

    def expected(self):
        full = np.full(tuple(self.buf.shape), SENT)
        full[:, PAD:PAD + self.n] = np.concatenate([self.ref[k] for k in M.NAMES])
        return torch.from_numpy(full)

    def launch(self, t, check=True):
        pred = draw(self.kind, self.rng, self.n, self.nf)
        dpred = pred.to(DEV)
        self.step.copy_(torch.tensor([t, 0], dtype=I32))
        ops.rollout_moments(dpred, self.step, self.nf, STEPS, self.window, *self.views, stride=self.stride, sub=self.sub)
        self.ref = M.accumulate(self.ref, pred.numpy(), t, STEPS, self.stride, None if self.sub_host is None else self.sub_host.numpy())
        if not check:
            return
        what = f"{self.what} launch {t}"
        if not torch.equal(self.buf, self.expected().to(DEV)):
            for k, v in zip(M.NAMES, self.views):                      # (says which plane; the padding is what is left)
                M.same(v, self.ref[k], f"{what}, {k}")
            raise AssertionError(f"{what}: the padding around the planes was written")
        w = self.ref["window"]
        assert self.wbuf.tolist() == [ISENT, ISENT, int(w[0]), int(w[1]), ISENT, ISENT], f"{what}: window {self.wbuf.tolist()} vs {w}"
        assert self.step.tolist() == [t, 0], f"{what}: step {self.step.tolist()}"
        assert torch.equal(dpred.cpu(), pred), f"{what}: pred was written"
        if self.sub is not None:
            assert torch.equal(self.sub, self.sub_dev0), f"{what}: sub was written"

    def run(self, check=True):
        for t in range(STEPS + 1):
            self.launch(t, check)
        return self


@pytest.mark.parametrize("nf", [1, 2, 3, 5, 8])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 1000])
def test_moments_match_the_restatement(n, nf):
    """Every window, every form of `sub` and both kinds of data at this (n, nf)."""
    for start, stride in WINDOWS:
        for sub_kind in SUBS:
            for kind in KINDS:
                c = Launches(n, nf, start, stride, sub_kind, kind).run()
                last = max((t for t in range(STEPS) if M.on_window(t, start, stride, STEPS)), default=-1) if n else -1
                assert c.window.tolist() == [start, last]
                if n:
                    assert M.count(c.ref, stride) == len(range(start, STEPS, stride))


BIG = 262_144 + 300          # 1024 workgroups of 256: 300 threads take a second row


@pytest.mark.parametrize("nf,window,sub_kind,kind", [(1, (2, 3), "padded", "offset"), (2, (0, 3), "dense", "int"), (3, (0, 1), "padded", "offset"),
                                                     (5, (2, 1), None, "offset"), (8, (2, 3), "dense", "offset")])
def test_large_mesh_takes_several_rows_per_thread(nf, window, sub_kind, kind):
    Launches(BIG, nf, window[0], window[1], sub_kind, kind).run()


def test_two_runs_give_the_same_bits():
    a = Launches(1000, 3, 0, 1, "padded", "offset").run(check=False)
    b = Launches(1000, 3, 0, 1, "padded", "offset").run(check=False)
    assert torch.equal(a.buf, b.buf) and a.window.tolist() == b.window.tolist() == [0, STEPS - 1]
    assert bool((a.buf[:, PAD:-PAD] != SENT).all())


@pytest.mark.parametrize("sub_kind", [None, "padded"])
def test_running_through_a_reset_origin_replaces_the_record(sub_kind):
    c = Launches(257, 3, 0, 1, sub_kind, "offset").run()
    before = c.buf.clone()
    c.set_origin(3)
    for t in range(STEPS + 1):            # steps 0 .. 2 are now in front of the window: they leave the old record as it is
        c.launch(t)
        if t < 3:
            assert torch.equal(c.buf, before) and c.window.tolist() == [3, -1]
    assert c.window.tolist() == [3, STEPS - 1] and not torch.equal(c.buf, before)
    assert M.count(c.ref, 1) == STEPS - 3


def test_nine_fields_are_refused():
    n, nf = 50, 9
    buf = torch.full((4 * nf + ops.moment_pairs(nf), n), SENT, dtype=F64, device=DEV)
    window, step = torch.tensor([0, -1], dtype=I32, device=DEV), torch.zeros(2, dtype=I32, device=DEV)
    with pytest.raises(NotImplementedError, match="g4c_rollout_moments"):
        ops.rollout_moments(torch.zeros(n, nf, device=DEV), step, nf, STEPS, window, *buf.split((nf, nf, ops.moment_pairs(nf), nf, nf)))
    assert bool((buf == SENT).all()) and window.tolist() == [0, -1] and step.tolist() == [0, 0]


def test_invalid_descriptors_return_their_error_without_launching():
    """G4C_EINVAL straight from the library, on device buffers: nothing is written."""
    import ctypes as C
    n, nf = 64, 3
    lib = _lib.load()
    buf = torch.full((18, n), SENT, dtype=F64, device=DEV)
    pivot, s, s2, lo, hi = buf.split((3, 3, 6, 3, 3))
    window, step = torch.tensor([0, -1], dtype=I32, device=DEV), torch.zeros(2, dtype=I32, device=DEV)
    pred, sub = torch.ones(n, nf, device=DEV), torch.ones(n, nf * STEPS, device=DEV)
    ok = dict(max_steps=STEPS, stride=1, window=window.data_ptr(), plane_ld=n, pivot=pivot.data_ptr(), sum=s.data_ptr(), sum2=s2.data_ptr(),
              lo=lo.data_ptr(), hi=hi.data_ptr())
    for kw, word in ((dict(stride=0), "stride"), (dict(sub=sub.data_ptr(), sub_ld=nf * STEPS - 1), "sub_ld"), (dict(window=None), "null"),
                     (dict(hi=None), "null"), (dict(max_steps=-1), "bad sizes"), (dict(plane_ld=n - 1), "plane_ld")):
        m = _lib.g4c_rollout_moments_t(**dict(ok, **kw))
        rc = lib.g4c_rollout_moments(pred.data_ptr(), nf, C.byref(m), step.data_ptr(), n, _lib.stream_handle(DEV))
        msg = lib.g4c_last_error().decode()
        assert rc == _lib.EINVAL and "g4c_rollout_moments" in msg and word in msg, (kw, rc, msg)
    m = _lib.g4c_rollout_moments_t(**ok)
    assert lib.g4c_rollout_moments(pred.data_ptr(), nf, C.byref(m), step.data_ptr(), -1, _lib.stream_handle(DEV)) == _lib.EINVAL
    assert lib.g4c_rollout_moments(None, nf, C.byref(m), step.data_ptr(), n, _lib.stream_handle(DEV)) == _lib.EINVAL
    torch.cuda.synchronize(DEV)
    assert bool((buf == SENT).all()) and window.tolist() == [0, -1] and step.tolist() == [0, 0]


def test_negative_controls_on_the_launch():
    """The launch's own sums fail the comparison against a restatement with one mistake."""
    c = Launches(257, 3, 1, 2, "padded", "offset").run()
    got = dict(zip(M.NAMES, c.views), window=c.window)
    M.same_state(got, c.ref, "launch")
    rng = np.random.default_rng(1000 * 257 + 10 * 3)          # the case's draws again: sub first, then the nine predictions
    sub = draw("offset", rng, 257, 3 * STEPS + 5).numpy()          # (all its columns: "sub+1" reads past the record's)
    preds = [draw("offset", rng, 257, 3).numpy() for _ in range(STEPS + 1)]
    for wrong in (None,) + M.WRONG:
        st = M.new_state(257, 3, 1, fill=SENT)
        for t in range(STEPS + 1):
            st = M.accumulate(st, preds[t], t, STEPS, 2, sub, wrong=wrong)
        assert M.rejects(M.same_state, got, st, str(wrong)) == (wrong is not None), wrong


# ====================================================================== Rollout / time_statistics / evaluate
N_OUT, NF = 7, 3


@pytest.fixture(scope="module")
def mesh():
    g = S.mus_graph(3000, levels=3, seed=3).to(DEV)
    g.batch = torch.zeros(g.num_nodes, dtype=torch.long, device=DEV)
    torch.manual_seed(4)
    model = gfd.nn.NsThreeScaleGNN(arch=S.mus_arch("NsThreeScaleGNN", 128), device=DEV)
    model.eval()
    target = torch.randn(g.num_nodes, NF * N_OUT + 2, generator=torch.Generator().manual_seed(5)).to(DEV)
    full = model.solve(g.clone(), N_OUT)
    with Rollout(model, g, N_OUT, reorder=True) as ro:           # (the renumbered mesh adds its neighbours in another order)
        ro.run(N_OUT)
        assert ro._perm is not None
        renumbered = ro.result().clone()
    return dict(g=g, model=model, target=target, full=full, renumbered=renumbered)


def samples_of(result, nf=NF):
    r = result.cpu().numpy()
    return [r[:, nf * t:nf * (t + 1)] for t in range(r.shape[1] // nf)]


def same_as_restatement(mo, samples, steps, start, stride, what, sub=None, first=0):
    """The raw sums of a `RolloutMoments` are bit for bit the restatement's over `samples` (the predictions of steps first, first + 1, ...)."""
    st = M.run(samples, steps, start, stride, None if sub is None else sub.cpu().numpy(), first=first)
    assert mo.count == M.count(st, stride) > 0 and mo.origin == int(st["window"][0]) and mo.stride == stride, (what, mo)
    for k, got in zip(M.NAMES, (mo.pivot, mo.sum, mo.sum2, mo.min, mo.max)):
        assert got.dtype == F64 and got.is_cuda
        M.same(got, np.ascontiguousarray(st[k].T), f"{what}, {k}")
    return st


@pytest.mark.parametrize("capture", [True, False])
@pytest.mark.parametrize("reorder", [False, True])
def test_rollout_moments_equal_the_restatement_over_the_result(mesh, reorder, capture):
    with Rollout(mesh["model"], mesh["g"], N_OUT, capture=capture, reorder=reorder, every=1, moments=(1, 2), target=mesh["target"],
                 error_moments=(0, 3)) as ro:
        ro.run(N_OUT)
        assert (ro._perm is not None) == reorder
        res, mo, emo = ro.result(), ro.moments(), ro.error_moments()
    # the plain solve() of the same model (a mesh of this size is renumbered only when forced: then the plain rollout forced alike)
    assert torch.equal(res, mesh["renumbered" if reorder else "full"])
    what = f"reorder {reorder} capture {capture}"
    same_as_restatement(mo, samples_of(res), N_OUT, 1, 2, what)
    same_as_restatement(emo, samples_of(res), N_OUT, 0, 3, what + ", error", sub=mesh["target"])
    assert mo.count == 3 and emo.count == 3
    # the derived quantities are those of the steps on the window, in the caller's rows
    x = torch.stack([res[:, NF * t:NF * (t + 1)].double() for t in (1, 3, 5)])
    assert torch.allclose(mo.mean, x.mean(0), rtol=1e-12, atol=1e-12) and torch.allclose(mo.var, x.var(0, unbiased=False), rtol=1e-9, atol=1e-12)
    assert torch.equal(mo.min, x.min(0).values) and torch.equal(mo.max, x.max(0).values)
    d = torch.stack([(res[:, NF * t:NF * (t + 1)].double() - mesh["target"][:, NF * t:NF * (t + 1)].double()) for t in (0, 3, 6)])
    assert torch.allclose(emo.mean, d.mean(0), rtol=1e-12, atol=1e-12)


def test_moments_alone_keep_the_plain_closing_launch(mesh, monkeypatch):
    """`moments=` is no record: the step still ends in rollout_advance and keeps the buffer of every step."""
    def refuse(*a, **k):
        raise AssertionError("a rollout with moments only went through rollout_advance_record")
    calls, plain = [], ops.rollout_advance
    monkeypatch.setattr(ops, "rollout_advance_record", refuse)
    monkeypatch.setattr(ops, "rollout_advance", lambda *a, **k: (calls.append(1), plain(*a, **k))[1])
    with Rollout(mesh["model"], mesh["g"], N_OUT, capture=False, reorder=False, moments=True) as ro:
        ro.run(N_OUT)
        assert ro._rec is None and len(calls) == N_OUT and tuple(ro._out_steps.shape) == (N_OUT, mesh["g"].num_nodes, NF)
        res, mo = ro.result(), ro.moments()
    assert torch.equal(res, mesh["full"])
    same_as_restatement(mo, samples_of(res), N_OUT, 0, 1, "moments only")


def test_a_rollout_without_moments_is_what_it_was(mesh, monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a rollout without moments launched rollout_moments")
    monkeypatch.setattr(ops, "rollout_moments", refuse)
    with Rollout(mesh["model"], mesh["g"], N_OUT, reorder=False) as ro:
        ro.run(N_OUT)
        assert ro._moments is None and ro._error_moments is None and torch.equal(ro.result(), mesh["full"])
        with pytest.raises(RuntimeError, match="moments"):
            ro.moments()
        with pytest.raises(RuntimeError, match="error_moments"):
            ro.error_moments()
    assert torch.equal(mesh["model"].solve(mesh["g"].clone(), N_OUT), mesh["full"])
    with pytest.raises(AssertionError, match="rollout_moments"):
        with Rollout(mesh["model"], mesh["g"], N_OUT, reorder=False, moments=True) as ro:
            ro.run(1)


def test_every_zero_with_moments_holds_no_prediction_buffer(mesh):
    with Rollout(mesh["model"], mesh["g"], N_OUT, reorder=False, every=0, moments=(1, 2)) as ro:
        ro.run(N_OUT)
        assert ro._out_steps is None
        mo = ro.moments()
        with pytest.raises(RuntimeError, match="every=0"):
            ro.result()
    same_as_restatement(mo, samples_of(mesh["full"]), N_OUT, 1, 2, "every=0")


def test_rewind_leaves_the_statistics_of_the_steps_since(mesh):
    g, f0 = mesh["g"], mesh["g"].field
    try:
        with Rollout(mesh["model"], g, N_OUT, reorder=False, every=1, moments=(0, 2), target=mesh["target"], error_moments=1) as ro:
            ro.run(3)
            first = ro.moments()
            same_as_restatement(first, samples_of(ro.result())[:3], N_OUT, 0, 2, "before rewind")
            ro.rewind()                                   # the device step index is 1 again: slots 1, 2, ... are written next
            assert ro.moments().count == 0 and ro.error_moments().count == 0
            ro.run(4)
            res = ro.result()
            mo, emo = ro.moments(), ro.error_moments()
        assert torch.equal(res[:, 3:15], mesh["full"][:, 9:21])          # steps 3 .. 6 of the rollout sit in slots 1 .. 4
        after = samples_of(res)[1:5]
        same_as_restatement(mo, after, N_OUT, 0, 2, "after rewind", first=1)
        same_as_restatement(emo, after, N_OUT, 1, 1, "after rewind, error", sub=mesh["target"], first=1)
        assert mo.origin == 2 and mo.count == 2 and emo.origin == 1 and emo.count == 4
        assert not torch.equal(mo.pivot, first.pivot)
    finally:
        g.field = f0


def test_a_clipped_rollout_leaves_the_statistics_of_its_recomputation(mesh):
    g, f0 = mesh["g"], mesh["g"].field

    def run(precision=None):
        old = ops.set_mlp_precision(precision) if precision else None
        try:
            g.field = f0 * 1e5
            with Rollout(mesh["model"], g, N_OUT, reorder=False, every=1, moments=(1, 2), target=mesh["target"], error_moments=True) as ro:
                ro.run(N_OUT)
                return ro.result().clone(), ro.moments(), ro.error_moments(), ro
        finally:
            g.field = f0
            if old:
                ops.set_mlp_precision(old)

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res, mo, emo, ro = run()
        res_x, mo_x, emo_x, ro_x = run("bf16x6")
    assert ro.exact_range and not ro_x.exact_range and bool(torch.isfinite(res).all()) and torch.equal(res, res_x)
    same_as_restatement(mo, samples_of(res), N_OUT, 1, 2, "clipped")
    same_as_restatement(emo, samples_of(res), N_OUT, 0, 1, "clipped, error", sub=mesh["target"])
    for a, b in ((mo, mo_x), (emo, emo_x)):
        assert a.count == b.count and torch.equal(a.sum, b.sum) and torch.equal(a.sum2, b.sum2) and torch.equal(a.max, b.max)


def test_time_statistics_and_evaluate(mesh):
    g, model, full = mesh["g"].clone(), mesh["model"], mesh["full"]
    g.target = mesh["target"][:, :NF * N_OUT].contiguous()
    mo = model.time_statistics(g.clone(), N_OUT, discard=2, stride=2)
    assert type(mo) is gfd.nn.RolloutMoments and mo.snapshots is None and (mo.count, mo.origin, mo.stride) == (3, 2, 2)
    same_as_restatement(mo, samples_of(full), N_OUT, 2, 2, "time_statistics")
    kept = model.time_statistics(g.clone(), N_OUT, discard=2, stride=2, every=1, capture=False)
    assert torch.equal(kept.snapshots, full) and torch.equal(kept.sum2, mo.sum2) and torch.equal(kept.pivot, mo.pivot)
    every_step = model.time_statistics(g.clone(), N_OUT)
    assert every_step.count == N_OUT and torch.equal(every_step.min, torch.stack(samples_from(full)).min(0).values.double())
    with pytest.raises(ValueError, match="moments"):
        model.time_statistics(g.clone(), N_OUT, discard=N_OUT)
    errs = model.evaluate(g.clone())
    assert errs.moments is None and errs.error_moments is None
    both = model.evaluate(g.clone(), moments=(2, 2), error_moments=True)
    assert torch.equal(both.sums, errs.sums)
    assert torch.equal(both.moments.sum2, mo.sum2) and torch.equal(both.moments.sum, mo.sum) and both.moments.count == 3
    same_as_restatement(both.error_moments, samples_of(full), N_OUT, 0, 1, "evaluate, error", sub=g.target)
    # the bias and the mean-square error at every node, averaged over the nodes, are evaluate()'s own per-step figures averaged over time
    em = both.error_moments
    mse_nodes = (em.mean ** 2 + em.var).mean(0)
    assert torch.allclose(mse_nodes.cpu(), errs.mse.mean(0), rtol=1e-10, atol=0)
    with pytest.raises(ValueError, match="error_moments"):
        Rollout(model, g, N_OUT, error_moments=True)


def samples_from(full, nf=NF):
    return [full[:, nf * t:nf * (t + 1)] for t in range(full.size(1) // nf)]


def test_list_of_two_graphs():
    gen = torch.Generator().manual_seed(8)
    graphs = [S.mus_graph(n, levels=1, seed=20 + n).to(DEV) for n in (300, 500)]
    for gr in graphs:
        gr.target = torch.randn(gr.num_nodes, NF * N_OUT, generator=gen).to(DEV)
    torch.manual_seed(9)
    model = gfd.nn.NsOneScaleGNN(arch=S.mus_arch("NsOneScaleGNN", 64), device=DEV)
    full = model.solve([gr.clone() for gr in graphs], N_OUT)
    mo = model.time_statistics([gr.clone() for gr in graphs], N_OUT, discard=1, stride=2)
    assert tuple(mo.pivot.shape) == (800, NF)
    same_as_restatement(mo, samples_of(full), N_OUT, 1, 2, "two graphs")
    errs = model.evaluate([gr.clone() for gr in graphs], moments=True, error_moments=(1, 2))
    same_as_restatement(errs.moments, samples_of(full), N_OUT, 0, 1, "two graphs, evaluate")
    same_as_restatement(errs.error_moments, samples_of(full), N_OUT, 1, 2, "two graphs, evaluate, error", sub=torch.cat([gr.target for gr in graphs]))


def test_remus():
    g = S.remus_graph(1500, k=5, seed=4).to(DEV)
    torch.manual_seed(6)
    model = gfd.nn.NsRotEquiTreeScaleGNN(arch=S.remus_arch(64), device=DEV)
    g.target = torch.randn(g.num_nodes, 2 * N_OUT, generator=torch.Generator().manual_seed(7)).to(DEV)
    full = model.solve(g.clone(), N_OUT)
    mo = model.time_statistics(g.clone(), N_OUT, discard=1, stride=2, every=1)
    assert torch.equal(mo.snapshots, full) and tuple(mo.sum2.shape) == (1500, 3) and tuple(mo.cov.shape) == (1500, 2, 2)
    same_as_restatement(mo, samples_of(full, 2), N_OUT, 1, 2, "REMuS")
    errs = model.evaluate(g.clone(), error_moments=(0, 3))
    same_as_restatement(errs.error_moments, samples_of(full, 2), N_OUT, 0, 3, "REMuS, error", sub=g.target)
