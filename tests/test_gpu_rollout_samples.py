"""`Rollout(samples=, sample_*=)`, `GNN.sample` and `GNN.evaluate(samples=)` against the restatements run over what the same rollout
returns: the series at the points is bit for bit tests/sampler_ref.py's numpy.float32 loop over `result()` (from the DEVICE's tables,
which tests/test_gpu_point_sampler.py pins) — with and without capture, with and without the Morton renumbering, whose bits it does
not depend on —, the sampled derived columns the same loop over the derived snapshots, and the time statistics and Fourier modes at
the points bit for bit tests/moments_ref.py and tests/spectrum_ref.py run over the series."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

import sampler_ref as R                                  # noqa: E402
import moments_ref as M                                  # noqa: E402
import spectrum_ref as SP                                # noqa: E402
import graphs4cfd_amd as gfd                             # noqa: E402
from graphs4cfd_amd import ops, synthetic as S           # noqa: E402
from graphs4cfd_amd.nn.model import Rollout              # noqa: E402

DEV = torch.device("cuda", 0)
N_OUT, NF, N_POINTS = 7, 3, 101
NAMES = ("div", "vort")


def points_in(g, n, seed):
    lo, hi = g.pos.min(0).values.cpu(), g.pos.max(0).values.cpu()
    return lo + (hi - lo) * (torch.rand(n, int(g.pos.size(1)), generator=torch.Generator().manual_seed(seed)) * 1.1 - 0.05)


@pytest.fixture(scope="module")
def mesh():
    g = S.mus_graph(3000, levels=3, seed=3).to(DEV)
    g.batch = torch.zeros(g.num_nodes, dtype=torch.long, device=DEV)
    torch.manual_seed(4)
    model = gfd.nn.NsThreeScaleGNN(arch=S.mus_arch("NsThreeScaleGNN", 128), device=DEV)
    model.eval()
    full = model.solve(g.clone(), N_OUT)
    pts = points_in(g, N_POINTS, 5)
    pts[:7] = g.pos[[0, 17, 500, 999, 1500, 2222, 2999]].cpu()          # seven points on nodes
    sampler = gfd.PointSampler(g, pts)
    assert int((sampler.distance == 0).sum()) == 7
    return dict(g=g, model=model, full=full, pts=pts, sampler=sampler, idx=sampler.idx.cpu().numpy(), coef=sampler.coef.cpu().numpy(), runs={})


def per_step(cols, nf=NF):
    r = cols.cpu().numpy()
    return [np.ascontiguousarray(r[:, nf * t:nf * (t + 1)]) for t in range(r.shape[1] // nf)]


def series_equal_over(series, preds, steps, mesh, what, nf=NF):
    """Slot s of `series` is the fp32 loop over the prediction of step steps[s]."""
    got = per_step(series, nf)
    assert len(got) >= len(steps), what
    for s, t in enumerate(steps):
        R.same(got[s], R.apply32(preds[t], mesh["idx"], mesh["coef"]), f"{what}, slot {s} (step {t})")


def moments_equal_over(mo, samples, steps, start, stride, what, first=0):
    st = M.run(samples, steps, start, stride, None, first=first)
    assert mo.count == M.count(st, stride) > 0 and mo.origin == int(st["window"][0]) and mo.stride == stride, (what, mo)
    for k, got in zip(M.NAMES, (mo.pivot, mo.sum, mo.sum2, mo.min, mo.max)):
        M.same(got, np.ascontiguousarray(st[k].T), f"{what}, {k}")


def spectrum_equal_over(sp, samples, steps, start, stride, what, first=0):
    st = SP.run(samples, steps, sp.tw.numpy(), start, stride, first=first)
    assert sp.count == SP.count(st, stride) > 0 and sp.origin == int(st["window"][0]), (what, sp)
    for k, got in zip(SP.NAMES, (sp.pivot, sp.sum, sp.re.flatten(1), sp.im.flatten(1))):
        SP.same(got, np.ascontiguousarray(st[k].T), f"{what}, {k}")


def zeros_between(kept, steps, shape):
    """The samples of steps 0 .. steps − 1 for the restatements: the kept ones, zeros where nothing was kept (those lie off the window)."""
    return [kept.get(t, np.zeros(shape, np.float32)) for t in range(steps)]


@pytest.mark.parametrize("capture", [True, False])
@pytest.mark.parametrize("reorder", [False, True])
def test_rollout_samples_equal_the_restatement_over_the_result(mesh, reorder, capture):
    spec = gfd.Spectrum([0, 1], start=1, stride=2, samples=3)
    with Rollout(mesh["model"], mesh["g"], N_OUT, capture=capture, reorder=reorder, every=1, derived=NAMES, derived_every=2,
                 samples=mesh["sampler"], sample_every=2, sample_moments=(1, 2), sample_spectrum=spec, sample_derived=True) as ro:
        ro.run(N_OUT)
        assert (ro._perm is not None) == reorder
        res, d, rs = ro.result(), ro.derived(), ro.samples()
    what = f"reorder {reorder} capture {capture}"
    if not reorder:
        assert torch.equal(res, mesh["full"])
    assert type(rs) is gfd.nn.RolloutSamples and rs.sampler is mesh["sampler"] and rs.columns == ["div", "vort"] and rs.slots == 3 and rs.target is None
    assert tuple(rs.series.shape) == (N_POINTS, NF * 3) and tuple(rs.derived.shape) == (N_POINTS, 2 * 3)
    assert torch.equal(rs.points, mesh["sampler"].points) and torch.equal(rs.distance, mesh["sampler"].distance)
    series_equal_over(rs.series, per_step(res), [1, 3, 5], mesh, what)
    series_equal_over(rs.derived, per_step(d.snapshots, 2), [0, 1, 2], mesh, what + ", derived", nf=2)
    # a point on a node holds that node's prediction
    assert torch.equal(rs.series[:7], res[[0, 17, 500, 999, 1500, 2222, 2999]][:, [c for t in (1, 3, 5) for c in range(NF * t, NF * t + NF)]])
    kept = dict(zip((1, 3, 5), per_step(rs.series)))
    moments_equal_over(rs.moments, zeros_between(kept, N_OUT, (N_POINTS, NF)), N_OUT, 1, 2, what + ", moments")
    spectrum_equal_over(rs.spectrum, zeros_between(kept, N_OUT, (N_POINTS, NF)), N_OUT, 1, 2, what + ", spectrum")
    assert rs.moments.count == 3 and rs.spectrum.complete and tuple(rs.moments.pivot.shape) == (N_POINTS, NF)
    # the same bits whatever the numbering and the capture: the same values enter every sum in the same order
    mesh["runs"][(reorder, capture)] = (res, rs)
    other = mesh["runs"].get((reorder, not capture))
    if other is not None:
        assert torch.equal(rs.series, other[1].series) and torch.equal(rs.derived, other[1].derived)
        for k in ("pivot", "sum", "sum2", "min", "max"):
            assert torch.equal(getattr(rs.moments, k), getattr(other[1].moments, k)), k
        assert torch.equal(rs.spectrum.re, other[1].spectrum.re) and torch.equal(rs.spectrum.im, other[1].spectrum.im)


def test_points_are_enough_and_every_step_can_be_kept(mesh):
    with Rollout(mesh["model"], mesh["g"], N_OUT, reorder=False, every=0, samples=mesh["pts"], sample_moments=True) as ro:
        ro.run(N_OUT)
        rs = ro.samples()
        assert ro._out_steps is None
    assert rs.derived is None and rs.columns is None and rs.spectrum is None and rs.sampler.k == 6
    series_equal_over(rs.series, per_step(mesh["full"]), list(range(N_OUT)), mesh, "points, every step")
    moments_equal_over(rs.moments, per_step(rs.series), N_OUT, 0, 1, "every step, moments")
    with Rollout(mesh["model"], mesh["g"], N_OUT, reorder=False, samples=mesh["sampler"], sample_every=0, sample_moments=2) as ro:
        ro.run(N_OUT)
        none = ro.samples()
    assert none.series is None and none.slots == 0 and none.moments.count == 5
    moments_equal_over(none.moments, per_step(rs.series), N_OUT, 2, 1, "no series, moments")


def test_a_rollout_without_samples_is_what_it_was(mesh, monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a rollout without samples launched sample_points")
    calls, plain = [], ops.rollout_advance
    for name in ("sample_points", "sample_weights", "rollout_moments", "rollout_spectrum", "mesh_derived", "rollout_advance_record"):
        monkeypatch.setattr(ops, name, refuse)
    monkeypatch.setattr(S, "knn_query_device", refuse)
    monkeypatch.setattr(ops, "rollout_advance", lambda *a, **k: (calls.append(1), plain(*a, **k))[1])
    with Rollout(mesh["model"], mesh["g"], N_OUT, reorder=False, capture=False) as ro:
        ro.run(N_OUT)
        assert ro._samples is None and len(calls) == N_OUT and torch.equal(ro.result(), mesh["full"])
        with pytest.raises(RuntimeError, match="samples"):
            ro.samples()
    assert torch.equal(mesh["model"].solve(mesh["g"].clone(), N_OUT), mesh["full"])
    with pytest.raises(AssertionError, match="without samples"):
        with Rollout(mesh["model"], mesh["g"], N_OUT, reorder=False, samples=mesh["sampler"]) as ro:
            ro.run(1)


def test_rewind_leaves_the_samples_of_the_steps_since(mesh):
    g, f0 = mesh["g"], mesh["g"].field
    spec = gfd.Spectrum([0, 1], start=0, stride=2)
    try:
        with Rollout(mesh["model"], g, N_OUT, reorder=False, every=1, samples=mesh["sampler"], sample_moments=(0, 2), sample_spectrum=spec) as ro:
            ro.run(3)
            before = ro.samples()
            series_equal_over(before.series, per_step(ro.result()), [0, 1, 2], mesh, "before rewind")
            ro.rewind()                                   # the device step index is 1 again: slots 1, 2, ... are written next
            assert ro.samples().moments.count == 0 and ro.samples().spectrum.count == 0
            ro.run(4)
            res, rs = ro.result(), ro.samples()
        assert torch.equal(res[:, 3:15], mesh["full"][:, 9:21])          # steps 3 .. 6 of the rollout sit in slots 1 .. 4
        series_equal_over(rs.series, per_step(res), [0, 1, 2, 3, 4], mesh, "after rewind")
        assert torch.equal(rs.series[:, :3], before.series[:, :3]) and not torch.equal(rs.series[:, 3:6], before.series[:, 3:6])
        moments_equal_over(rs.moments, per_step(rs.series)[1:5], N_OUT, 0, 2, "after rewind, moments", first=1)
        spectrum_equal_over(rs.spectrum, per_step(rs.series)[1:5], N_OUT, 0, 2, "after rewind, spectrum", first=1)
        assert rs.moments.origin == 2 and rs.moments.count == 2
    finally:
        g.field = f0


def test_a_clipped_rollout_leaves_the_samples_of_its_recomputation(mesh):
    import warnings
    g, f0 = mesh["g"], mesh["g"].field

    def run(precision=None):
        old = ops.set_mlp_precision(precision) if precision else None
        try:
            g.field = f0 * 1e5
            with Rollout(mesh["model"], g, N_OUT, reorder=False, every=1, samples=mesh["sampler"], sample_moments=(1, 2)) as ro:
                ro.run(N_OUT)
                return ro.result().clone(), ro.samples(), ro
        finally:
            g.field = f0
            if old:
                ops.set_mlp_precision(old)

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res, rs, ro = run()
        res_x, rs_x, ro_x = run("bf16x6")
    assert ro.exact_range and not ro_x.exact_range and torch.equal(res, res_x)
    assert torch.equal(rs.series, rs_x.series) and torch.equal(rs.moments.sum2, rs_x.moments.sum2)
    series_equal_over(rs.series, per_step(res), list(range(N_OUT)), mesh, "clipped")
    moments_equal_over(rs.moments, per_step(rs.series), N_OUT, 1, 2, "clipped, moments")


def test_sample_and_evaluate_agree_with_the_rollout(mesh):
    g, model = mesh["g"].clone(), mesh["model"]
    rs = model.sample(g.clone(), N_OUT, mesh["sampler"], every=1, discard=1, stride=2, spectrum=gfd.Spectrum([0, 1], start=1, stride=2),
                      derived=("vort",), capture=False, power=1)
    assert rs.columns == ["vort"] and tuple(rs.derived.shape) == (N_POINTS, N_OUT) and rs.moments.count == 3 and rs.spectrum.count == 3
    series_equal_over(rs.series, per_step(mesh["full"]), list(range(N_OUT)), mesh, "sample()")
    vort = gfd.MeshGradient(g, power=1).derived(mesh["full"][:, 3 * 4:3 * 5].contiguous(), ("vort",))
    assert torch.equal(rs.derived[:, 4:5], mesh["sampler"].sample(vort))
    moments_equal_over(rs.moments, per_step(rs.series), N_OUT, 1, 2, "sample(), moments")
    spectrum_equal_over(rs.spectrum, per_step(rs.series), N_OUT, 1, 2, "sample(), spectrum")
    by_points = model.sample(g.clone(), N_OUT, mesh["pts"], every=3)
    assert by_points.slots == 2 and torch.equal(by_points.series, rs.series[:, [6, 7, 8, 15, 16, 17]]) and by_points.moments is None
    # evaluate: the same samples, and the target at the same points by one launch
    g.target = torch.randn(g.num_nodes, NF * N_OUT + 2, generator=torch.Generator().manual_seed(5)).to(DEV)
    plain = model.evaluate(g.clone(), N_OUT)
    assert plain.samples is None
    errs = model.evaluate(g.clone(), N_OUT, samples=mesh["sampler"], sample_moments=(1, 2))
    assert torch.equal(errs.sums, plain.sums) and torch.equal(errs.samples.series, rs.series)
    assert torch.equal(errs.samples.moments.sum2, rs.moments.sum2)
    want = mesh["sampler"].sample(g.target[:, :NF * N_OUT])
    assert tuple(errs.samples.target.shape) == (N_POINTS, NF * N_OUT) and torch.equal(errs.samples.target, want)
    R.same(want, R.apply32(g.target[:, :NF * N_OUT].cpu().numpy(), mesh["idx"], mesh["coef"]), "target")
    with pytest.raises(ValueError, match="^samples"):
        model.sample([g.clone(), g.clone()], N_OUT, mesh["pts"])
    with pytest.raises(ValueError, match="^samples"):
        model.evaluate([g.clone(), g.clone()], N_OUT, samples=mesh["pts"])
    with pytest.raises(ValueError, match="^sample_derived"):
        Rollout(model, mesh["g"], N_OUT, samples=mesh["pts"], sample_derived=True)


def test_a_raster_has_the_shape_and_the_orientation_of_its_grid(mesh):
    g, model = mesh["g"], mesh["model"]
    lo, hi = g.pos.min(0).values.cpu().tolist(), g.pos.max(0).values.cpu().tolist()
    box = ([lo[0] + 0.1 * (hi[0] - lo[0]), lo[1] + 0.1 * (hi[1] - lo[1])], [hi[0] - 0.1 * (hi[0] - lo[0]), hi[1] - 0.1 * (hi[1] - lo[1])])
    raster = gfd.PointSampler.grid(g, (16, 8), box=box)
    rs = model.sample(g.clone(), N_OUT, raster, every=N_OUT, derived=("vort",))
    assert rs.slots == 1 and tuple(rs.image().shape) == (16, 8) and tuple(rs.image(0, "vort").shape) == (16, 8)
    assert torch.equal(rs.image(-1, 2), rs.series[:, 2].view(16, 8)) and torch.equal(rs.image(0, "vort"), rs.derived[:, 0].view(16, 8))
    assert torch.equal(rs.series, raster.sample(mesh["full"][:, NF * (N_OUT - 1):].contiguous()))
    # the fields (x, y, x + y) as a one-slot series: the picture of x runs along the first axis, that of y along the second
    xy = g.pos.float()
    field = torch.stack([xy[:, 0], xy[:, 1], xy[:, 0] + xy[:, 1]], dim=1).contiguous()
    pic = gfd.nn.RolloutSamples(raster, series=raster.sample(field), fields=3)
    xs = torch.linspace(box[0][0], box[1][0], 16, dtype=torch.float64)
    ys = torch.linspace(box[0][1], box[1][1], 8, dtype=torch.float64)
    tol = 1e-5 * max(abs(v) for v in lo + hi)
    assert float((pic.image(0, 0).cpu().double() - xs[:, None]).abs().max()) <= tol
    assert float((pic.image(0, 1).cpu().double() - ys[None, :]).abs().max()) <= tol
    with pytest.raises(ValueError, match="^image"):
        gfd.nn.RolloutSamples(mesh["sampler"], series=mesh["sampler"].sample(field), fields=3).image()


def test_remus():
    g = S.remus_graph(1500, k=5, seed=4).to(DEV)
    torch.manual_seed(6)
    model = gfd.nn.NsRotEquiTreeScaleGNN(arch=S.remus_arch(64), device=DEV)
    full = model.solve(g.clone(), N_OUT)
    sampler = gfd.PointSampler.line(g, g.pos.min(0).values.cpu(), g.pos.max(0).values.cpu(), 33)
    rs = model.sample(g.clone(), N_OUT, sampler, every=3, discard=0, derived=("vort",))
    assert rs.fields == 2 and rs.slots == 2 and rs.moments.count == N_OUT and rs.columns == ["vort"]
    tab = dict(idx=sampler.idx.cpu().numpy(), coef=sampler.coef.cpu().numpy())
    series_equal_over(rs.series, per_step(full, 2), [2, 5], tab, "REMuS", nf=2)
