"""Every argument error of `gfd.PointSampler`, `PointSampler.line`, `PointSampler.grid`, `Rollout(samples=, sample_*=)`, `GNN.sample`,
`GNN.evaluate(samples=)`, `ops.sample_weights` and `ops.sample_points` is a ValueError naming the argument, raised on the tensors as
they were passed: nothing is moved and the library is not loaded (no GPU needed).  A well-formed call on host tensors stops at the
device check."""
import ctypes as C
import os
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import graphs4cfd_amd as gfd                                          # noqa: E402
from graphs4cfd_amd import _lib, ops                                  # noqa: E402
from graphs4cfd_amd.nn.model import GNN, Rollout, RolloutSamples      # noqa: E402

PS = gfd.PointSampler
I32, I64, F64, U8 = torch.int32, torch.int64, torch.float64, torch.uint8


@pytest.fixture(autouse=True)
def library_must_not_load(monkeypatch):
    def load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", load)


def host_graph(n=20, dim=2, nf=3):
    return gfd.Graph(field=torch.zeros(n, nf), pos=torch.rand(n, dim, generator=torch.Generator().manual_seed(1)),
                     edge_index=torch.zeros(2, 4, dtype=torch.long), target=torch.zeros(n, nf * 7))


def pts(p=5, dim=2):
    return torch.rand(p, dim, generator=torch.Generator().manual_seed(2))


def refused(word, call, *a, **kw):
    with pytest.raises(ValueError) as info:
        call(*a, **kw)
    msg = str(info.value)
    assert type(info.value) is ValueError and msg.startswith(word + ":"), f"{type(info.value).__name__}: {msg}"
    return msg


def bad(word, call, *a, **kw):
    msg = refused(word, call, *a, **kw)
    assert "no CPU fallback" not in msg, msg          # (the argument was refused for what it is, not for where it lives)
    return msg


SAMPLER_BAD = {
    "graph-without-pos": ("graph", lambda: PS(gfd.Graph(field=torch.zeros(4, 3)), pts())),
    "graph-pos-1d": ("graph", lambda: PS(gfd.Graph(pos=torch.zeros(4)), pts())),
    "graph-pos-4d": ("graph", lambda: PS(gfd.Graph(pos=torch.zeros(4, 4)), pts(5, 4))),
    "graph-pos-int": ("graph", lambda: PS(gfd.Graph(pos=torch.zeros(4, 2, dtype=I64)), pts())),
    "power-3": ("power", lambda: PS(host_graph(), pts(), power=3)),
    "power-float": ("power", lambda: PS(host_graph(), pts(), power=2.0)),
    "power-bool": ("power", lambda: PS(host_graph(), pts(), power=True)),
    "k-zero": ("k", lambda: PS(host_graph(), pts(), k=0)),
    "k-17": ("k", lambda: PS(host_graph(), pts(), k=17)),
    "k-float": ("k", lambda: PS(host_graph(), pts(), k=6.0)),
    "k-bool": ("k", lambda: PS(host_graph(), pts(), k=True)),
    "k-more-than-nodes": ("k", lambda: PS(host_graph(n=5), pts(), k=6)),
    "k-default-more-than-nodes": ("k", lambda: PS(host_graph(n=9, dim=3), pts(5, 3))),
    "points-list": ("points", lambda: PS(host_graph(), [[0.0, 0.0]])),
    "points-int": ("points", lambda: PS(host_graph(), torch.zeros(5, 2, dtype=I64))),
    "points-1d": ("points", lambda: PS(host_graph(), torch.zeros(2))),
    "points-other-dim": ("points", lambda: PS(host_graph(), pts(5, 3))),
    "points-nan": ("points", lambda: PS(host_graph(), torch.tensor([[0.0, float("nan")]]))),
    "points-inf": ("points", lambda: PS(host_graph(), torch.tensor([[float("inf"), 0.0]]))),
    "line-a-short": ("a", lambda: PS.line(host_graph(), (0.0,), (1.0, 1.0), 5)),
    "line-a-str": ("a", lambda: PS.line(host_graph(), "ab", (1.0, 1.0), 5)),
    "line-b-nan": ("b", lambda: PS.line(host_graph(), (0.0, 0.0), (1.0, float("nan")), 5)),
    "line-b-3d": ("b", lambda: PS.line(host_graph(), (0.0, 0.0), (1.0, 1.0, 1.0), 5)),
    "line-n-one": ("n", lambda: PS.line(host_graph(), (0.0, 0.0), (1.0, 1.0), 1)),
    "line-n-float": ("n", lambda: PS.line(host_graph(), (0.0, 0.0), (1.0, 1.0), 5.0)),
    "line-k": ("k", lambda: PS.line(host_graph(), (0.0, 0.0), (1.0, 1.0), 5, k=17)),
    "line-graph": ("graph", lambda: PS.line(gfd.Graph(field=torch.zeros(4, 3)), (0.0, 0.0), (1.0, 1.0), 5)),
    "grid-shape-int": ("shape", lambda: PS.grid(host_graph(), 8)),
    "grid-shape-short": ("shape", lambda: PS.grid(host_graph(), (8,))),
    "grid-shape-zero": ("shape", lambda: PS.grid(host_graph(), (8, 0))),
    "grid-shape-float": ("shape", lambda: PS.grid(host_graph(), (8, 4.0))),
    "grid-box-one-corner": ("box", lambda: PS.grid(host_graph(), (8, 4), box=((0.0, 0.0),))),
    "grid-box-3d-corner": ("box", lambda: PS.grid(host_graph(), (8, 4), box=((0.0, 0.0), (1.0, 1.0, 1.0)))),
    "grid-box-inf": ("box", lambda: PS.grid(host_graph(), (8, 4), box=((0.0, 0.0), (1.0, float("inf"))))),
    "grid-box-number": ("box", lambda: PS.grid(host_graph(), (8, 4), box=3)),
    "grid-power": ("power", lambda: PS.grid(host_graph(), (8, 4), power=5)),
}


@pytest.mark.parametrize("label", sorted(SAMPLER_BAD))
def test_point_sampler_refuses(label):
    word, call = SAMPLER_BAD[label]
    bad(word, call)


@pytest.mark.parametrize("call", [lambda: PS(host_graph(), pts()), lambda: PS(host_graph(), pts(0)), lambda: PS(host_graph(dim=3), pts(5, 3), k=16, power=0),
                                  lambda: PS.line(host_graph(), (0.0, 0.0), torch.tensor([1.0, 1.0]), 2),
                                  lambda: PS.grid(host_graph(), (8, 4)), lambda: PS.grid(host_graph(), (1, 1), box=((0.0, 0.0), (1.0, 1.0)))])
def test_a_wellformed_sampler_on_the_host_stops_at_the_device_check(call):
    assert "no CPU fallback" in refused("graph", call)


def fake_sampler(n_nodes=20, p=5, shape=None):
    s = object.__new__(PS)
    s.n_nodes, s.points, s.distance, s.degenerate, s.shape, s.dim, s.k = n_nodes, pts(p), torch.zeros(p), torch.zeros(p, dtype=torch.bool), shape, 2, 6
    return s


S = gfd.Spectrum
ROLLOUT_BAD = {
    "samples-list": ("samples", dict(samples=[[0.0, 0.0]])),
    "samples-int": ("samples", dict(samples=torch.zeros(5, 2, dtype=I64))),
    "samples-other-dim": ("samples", dict(samples=pts(5, 3))),
    "samples-nan": ("samples", dict(samples=torch.tensor([[0.0, float("nan")]]))),
    "samples-sampler-of-another-graph": ("samples", dict(samples=fake_sampler(21))),
    "sample_every-negative": ("sample_every", dict(samples=pts(), sample_every=-1)),
    "sample_every-float": ("sample_every", dict(samples=pts(), sample_every=1.0)),
    "sample_every-bool": ("sample_every", dict(samples=pts(), sample_every=True)),
    "sample_derived-without-derived": ("sample_derived", dict(samples=pts(), sample_derived=True)),
    "sample_derived-int": ("sample_derived", dict(samples=pts(), sample_derived=1)),
    "sample_moments-without-samples": ("samples", dict(sample_moments=True)),
    "sample_spectrum-without-samples": ("samples", dict(sample_spectrum=S([1]))),
    "sample_derived-without-samples": ("samples", dict(sample_derived=True, derived=("div",))),
    "sample_moments-str": ("sample_moments", dict(samples=pts(), sample_moments="all")),
    "sample_moments-start": ("sample_moments", dict(samples=pts(), sample_moments=7)),
    "sample_moments-stride": ("sample_moments", dict(samples=pts(), sample_moments=(0, 0))),
    "sample_spectrum-tuple": ("sample_spectrum", dict(samples=pts(), sample_spectrum=(0, 1))),
    "sample_spectrum-bins": ("sample_spectrum", dict(samples=pts(), sample_spectrum=S([4]))),
    "sample_spectrum-too-many-bins": ("sample_spectrum", dict(samples=pts(), sample_spectrum=S(freqs=[0.5 * k / 65 for k in range(65)]))),
}


@pytest.mark.parametrize("label", sorted(ROLLOUT_BAD))
def test_rollout_refuses(label):
    word, kw = ROLLOUT_BAD[label]
    bad(word, Rollout, SimpleNamespace(num_fields=3), host_graph(), 7, **kw)


@pytest.mark.parametrize("kw", [dict(sample_moments=True), dict(sample_spectrum=S([1]))])
def test_rollout_refuses_sample_statistics_of_more_than_eight_fields(kw):
    name = next(iter(kw))
    bad(name, Rollout, SimpleNamespace(num_fields=9), host_graph(nf=9), 7, samples=pts(), **kw)


@pytest.mark.parametrize("kw", [dict(samples=pts()), dict(samples=fake_sampler(), sample_every=0, sample_moments=(1, 2), sample_spectrum=S([0, 3])),
                                dict(samples=pts(0), sample_every=3), dict(samples=pts(), derived=("vort",), sample_derived=True)])
def test_a_rollout_with_wellformed_samples_stops_at_the_device_check(kw):
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Rollout(SimpleNamespace(num_fields=3), host_graph(), 7, **kw)


def fake_model(nf=3):
    m = SimpleNamespace(num_fields=nf)
    m._rollout = lambda *a, **kw: GNN._rollout(m, *a, **kw)
    m.eval = lambda: (_ for _ in ()).throw(AssertionError("the model was touched before the arguments were checked"))
    return m


MODEL_BAD = {
    "points-int": ("samples", lambda m: GNN.sample(m, host_graph(), 7, torch.zeros(5, 2, dtype=I64))),
    "points-other-dim": ("samples", lambda m: GNN.sample(m, host_graph(), 7, pts(5, 3))),
    "every": ("sample_every", lambda m: GNN.sample(m, host_graph(), 7, pts(), every=-1)),
    "discard": ("sample_moments", lambda m: GNN.sample(m, host_graph(), 7, pts(), discard=7)),
    "stride": ("sample_moments", lambda m: GNN.sample(m, host_graph(), 7, pts(), discard=0, stride=0)),
    "spectrum": ("sample_spectrum", lambda m: GNN.sample(m, host_graph(), 7, pts(), spectrum=S([4]))),
    "derived": ("derived", lambda m: GNN.sample(m, host_graph(), 7, pts(), derived=("curl",))),
    "derived-option": ("derived_options", lambda m: GNN.sample(m, host_graph(), 7, pts(), derived=("div",), strength=2)),
    "list": ("samples", lambda m: GNN.sample(m, [host_graph(), host_graph()], 7, pts())),
    "evaluate-list": ("samples", lambda m: GNN.evaluate(m, [host_graph(), host_graph()], 7, samples=pts())),
    "evaluate-points": ("samples", lambda m: GNN.evaluate(m, host_graph(), 7, samples=pts(5, 3))),
    "evaluate-sample_derived": ("sample_derived", lambda m: GNN.evaluate(m, host_graph(), 7, samples=pts(), sample_derived=True)),
}


@pytest.mark.parametrize("label", sorted(MODEL_BAD))
def test_the_model_refuses_before_anything_is_moved(label):
    word, call = MODEL_BAD[label]
    bad(word, call, fake_model())


def test_image_needs_a_grid_and_a_known_column():
    series = torch.arange(8 * 3 * 2, dtype=torch.float32).reshape(8, 6)
    derived = torch.arange(8 * 2, dtype=torch.float32).reshape(8, 2)
    rs = RolloutSamples(fake_sampler(p=8, shape=(4, 2)), series=series, derived=derived, columns=["vort"], fields=3)
    assert rs.slots == 2 and rs.target is None
    assert torch.equal(rs.image(-1, 1), series[:, 4].reshape(4, 2)) and torch.equal(rs.image(0, 2), series[:, 2].reshape(4, 2))
    assert torch.equal(rs.image(0, "vort"), derived[:, 0].reshape(4, 2))
    for word, kw in (("column", dict(column=3)), ("column", dict(column="div")), ("column", dict(column=True)), ("slot", dict(slot=2)),
                     ("slot", dict(slot=-3)), ("slot", dict(slot=0.0))):
        refused(word, rs.image, **kw)
    refused("image", RolloutSamples(fake_sampler(p=8), series=series, fields=3).image)
    refused("image", RolloutSamples(fake_sampler(p=8, shape=(4, 2)), fields=3).image)


# ------------------------------------------------------------------ ops.sample_weights / ops.sample_points
N, P, K, NF, STEPS = 12, 5, 4, 3, 7


def good_weights():
    return dict(pos=torch.zeros(N, 2), queries=torch.zeros(P, 2), idx=torch.zeros(K, P, dtype=I32), power=2)


def good_points():
    return dict(x=torch.zeros(N, NF), idx=torch.zeros(K, P, dtype=I32), coef=torch.zeros(K, P), cur=torch.zeros(P, NF), step=torch.zeros(2, dtype=I32),
                every=2, series=torch.zeros(STEPS // 2, P, NF), max_steps=STEPS)


WEIGHTS_BAD = {
    "power": ("power", dict(power=3)),
    "pos-f64": ("pos", dict(pos=torch.zeros(N, 2, dtype=F64))),
    "pos-4d": ("pos", dict(pos=torch.zeros(N, 4))),
    "pos-strided": ("pos", dict(pos=torch.zeros(2, N).t())),
    "queries-dim": ("queries", dict(queries=torch.zeros(P, 3))),
    "queries-rows": ("queries", dict(queries=torch.zeros(P + 1, 2))),
    "idx-i64": ("idx", dict(idx=torch.zeros(K, P, dtype=I64))),
    "idx-point-major": ("idx", dict(idx=torch.zeros(P, K, dtype=I32).t())),
    "idx-k-17": ("idx", dict(idx=torch.zeros(17, P, dtype=I32))),
    "idx-k-zero": ("idx", dict(idx=torch.zeros(0, P, dtype=I32))),
    "idx-more-than-nodes": ("idx", dict(idx=torch.zeros(13, P, dtype=I32))),
    "out-coef": ("out[0]", dict(out=(torch.zeros(P, K), torch.zeros(P), torch.zeros(P, dtype=U8)))),
    "out-distance": ("out[1]", dict(out=(torch.zeros(K, P), torch.zeros(P, dtype=F64), torch.zeros(P, dtype=U8)))),
    "out-degenerate": ("out[2]", dict(out=(torch.zeros(K, P), torch.zeros(P), torch.zeros(P, dtype=torch.bool)))),
}

POINTS_BAD = {
    "x-f64": ("x", dict(x=torch.zeros(N, NF, dtype=F64))),
    "x-1d": ("x", dict(x=torch.zeros(N))),
    "x-colstride": ("x", dict(x=torch.zeros(NF, N).t())),
    "nf-zero": ("nf", dict(nf=0)),
    "nf-past": ("nf", dict(nf=NF + 1)),
    "idx-i64": ("idx", dict(idx=torch.zeros(K, P, dtype=I64))),
    "idx-k-17": ("idx", dict(idx=torch.zeros(17, P, dtype=I32), coef=torch.zeros(17, P))),
    "idx-more-than-nodes": ("idx", dict(x=torch.zeros(3, NF))),
    "coef-shape": ("coef", dict(coef=torch.zeros(K, P + 1))),
    "coef-f64": ("coef", dict(coef=torch.zeros(K, P, dtype=F64))),
    "coef-point-major": ("coef", dict(coef=torch.zeros(P, K).t())),
    "cur-shape": ("cur", dict(cur=torch.zeros(P, NF + 1))),
    "cur-strided": ("cur", dict(cur=torch.zeros(P, NF + 1)[:, :NF])),
    "every-negative": ("every", dict(every=-1)),
    "max_steps-negative": ("max_steps", dict(max_steps=-1)),
    "series-without-every": ("series", dict(every=0)),
    "every-without-series": ("series", dict(series=None)),
    "series-slots": ("series", dict(series=torch.zeros(STEPS // 2 + 1, P, NF))),
    "series-f64": ("series", dict(series=torch.zeros(STEPS // 2, P, NF, dtype=F64))),
    "step-missing": ("step", dict(step=None)),
    "step-i64": ("step", dict(step=torch.zeros(2, dtype=I64))),
}


@pytest.mark.parametrize("label", sorted(WEIGHTS_BAD))
def test_sample_weights_refuses(label):
    word, patch = WEIGHTS_BAD[label]
    assert "sample_weights" in bad(word, ops.sample_weights, **dict(good_weights(), **patch))


@pytest.mark.parametrize("label", sorted(POINTS_BAD))
def test_sample_points_refuses(label):
    word, patch = POINTS_BAD[label]
    assert "sample_points" in bad(word, ops.sample_points, **dict(good_points(), **patch))


@pytest.mark.parametrize("word, call", [("pos", lambda: ops.sample_weights(**good_weights())), ("x", lambda: ops.sample_points(**good_points())),
                                        ("x", lambda: ops.sample_points(torch.zeros(N, NF + 4)[:, 2:2 + NF], torch.zeros(K, P, dtype=I32), torch.zeros(K, P)))])
def test_a_wellformed_call_on_the_host_stops_at_the_device_check(word, call):
    assert "no CPU fallback" in refused(word, call)


def test_the_descriptor_matches_the_header():
    """LP64: two pointers, three int32 (+ 4 bytes of padding), two pointers, three int32 (+ 4), one pointer."""
    t = _lib.g4c_sample_points_t
    assert C.sizeof(t) == 72
    assert (t.idx.offset, t.coef.offset, t.k.offset, t.nf.offset, t.x_ld.offset, t.cur.offset, t.step.offset, t.every.offset, t.n_slots.offset,
            t.max_steps.offset, t.series.offset) == (0, 8, 16, 20, 24, 32, 40, 48, 52, 56, 64)
    assert _lib.SAMPLE_MAX_K == 16 and gfd.point_sampler.MAX_K == 16 and gfd.point_sampler.DEFAULT_K == {2: 6, 3: 10}
    assert "g4c_sample_weights" in _lib.EXPORTED_SYMBOLS and "g4c_sample_points" in _lib.EXPORTED_SYMBOLS
