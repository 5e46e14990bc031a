"""Every argument error of `gfd.Tracers`, `Tracers.streak`, `Rollout(tracers=, tracer_every=)`, `GNN.trace`, `GNN.evaluate(tracers=)`
and `ops.tracer_advance` names the argument and is raised on the tensors as they were passed: nothing is moved and the library is not
loaded (no GPU needed).  A well-formed call on host tensors stops at the device check."""
import ctypes as C
import os
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import graphs4cfd_amd as gfd                                          # noqa: E402
from graphs4cfd_amd import _lib, ops                                  # noqa: E402
from graphs4cfd_amd.nn.model import GNN, Rollout                      # noqa: E402
from graphs4cfd_amd.tracers import RolloutTracers, check_tracers      # noqa: E402

TR = gfd.Tracers
I32, I64, F64, U8 = torch.int32, torch.int64, torch.float64, torch.uint8
INF = float("inf")


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


def refused(word, call, *a, error=ValueError, **kw):
    with pytest.raises(error) as info:
        call(*a, **kw)
    msg = str(info.value)
    assert type(info.value) is error and msg.startswith(word + ":"), f"{type(info.value).__name__}: {msg}"
    assert "no CPU fallback" not in msg, msg          # (the argument was refused for what it is, not for where it lives)
    return msg


def fake_tracers(n_nodes=20, **kw):
    t = object.__new__(TR)
    t._spec = check_tracers(host_graph(n_nodes), pts(), 0.1, **kw)
    return t


TRACERS_BAD = {
    "graph-without-pos": ("graph", ValueError, lambda: TR(gfd.Graph(field=torch.zeros(4, 3)), pts(), 0.1)),
    "graph-pos-4d": ("graph", ValueError, lambda: TR(gfd.Graph(pos=torch.zeros(4, 4)), pts(5, 4), 0.1)),
    "seeds-list": ("seeds", ValueError, lambda: TR(host_graph(), [[0.0, 0.0]], 0.1)),
    "seeds-int": ("seeds", ValueError, lambda: TR(host_graph(), torch.zeros(5, 2, dtype=I64), 0.1)),
    "seeds-1d": ("seeds", ValueError, lambda: TR(host_graph(), torch.zeros(2), 0.1)),
    "seeds-other-dim": ("seeds", ValueError, lambda: TR(host_graph(), pts(5, 3), 0.1)),
    "seeds-nan": ("seeds", ValueError, lambda: TR(host_graph(), torch.tensor([[0.0, float("nan")]]), 0.1)),
    "dt-str": ("dt", TypeError, lambda: TR(host_graph(), pts(), "0.1")),
    "dt-bool": ("dt", TypeError, lambda: TR(host_graph(), pts(), True)),
    "dt-none": ("dt", TypeError, lambda: TR(host_graph(), pts(), None)),
    "dt-inf": ("dt", ValueError, lambda: TR(host_graph(), pts(), INF)),
    "dt-nan": ("dt", ValueError, lambda: TR(host_graph(), pts(), float("nan"))),
    "scheme-rk4": ("scheme", ValueError, lambda: TR(host_graph(), pts(), 0.1, scheme="rk4")),
    "scheme-int": ("scheme", ValueError, lambda: TR(host_graph(), pts(), 0.1, scheme=1)),
    "k-zero": ("k", ValueError, lambda: TR(host_graph(), pts(), 0.1, k=0)),
    "k-17": ("k", ValueError, lambda: TR(host_graph(), pts(), 0.1, k=17)),
    "k-float": ("k", ValueError, lambda: TR(host_graph(), pts(), 0.1, k=6.0)),
    "k-more-than-nodes": ("k", ValueError, lambda: TR(host_graph(n=5), pts(), 0.1)),
    "power-3": ("power", ValueError, lambda: TR(host_graph(), pts(), 0.1, power=3)),
    "power-bool": ("power", ValueError, lambda: TR(host_graph(), pts(), 0.1, power=True)),
    "velocity-short": ("velocity", ValueError, lambda: TR(host_graph(), pts(), 0.1, velocity=(0,))),
    "velocity-negative": ("velocity", ValueError, lambda: TR(host_graph(), pts(), 0.1, velocity=(0, -1))),
    "velocity-float": ("velocity", ValueError, lambda: TR(host_graph(), pts(), 0.1, velocity=(0, 1.0))),
    "velocity-int": ("velocity", ValueError, lambda: TR(host_graph(), pts(), 0.1, velocity=3)),
    "scale-short": ("scale", ValueError, lambda: TR(host_graph(), pts(), 0.1, scale=(1.0,))),
    "scale-inf": ("scale", ValueError, lambda: TR(host_graph(), pts(), 0.1, scale=(1.0, INF))),
    "shift-str": ("shift", ValueError, lambda: TR(host_graph(), pts(), 0.1, shift="ab")),
    "shift-nan": ("shift", ValueError, lambda: TR(host_graph(), pts(), 0.1, shift=float("nan"))),
    "box-number": ("box", ValueError, lambda: TR(host_graph(), pts(), 0.1, box=3)),
    "box-one-corner": ("box", ValueError, lambda: TR(host_graph(), pts(), 0.1, box=((0.0, 0.0),))),
    "box-3d-corner": ("box", ValueError, lambda: TR(host_graph(), pts(), 0.1, box=((0.0, 0.0), (1.0, 1.0, 1.0)))),
    "box-nan": ("box", ValueError, lambda: TR(host_graph(), pts(), 0.1, box=((0.0, float("nan")), (1.0, 1.0)))),
    "box-inverted": ("box", ValueError, lambda: TR(host_graph(), pts(), 0.1, box=((0.0, 2.0), (1.0, 1.0)))),
    "max_distance-negative": ("max_distance", ValueError, lambda: TR(host_graph(), pts(), 0.1, max_distance=-1.0)),
    "max_distance-nan": ("max_distance", ValueError, lambda: TR(host_graph(), pts(), 0.1, max_distance=float("nan"))),
    "max_distance-str": ("max_distance", ValueError, lambda: TR(host_graph(), pts(), 0.1, max_distance="far")),
    "release-float": ("release", TypeError, lambda: TR(host_graph(), pts(), 0.1, release=torch.zeros(5))),
    "release-bool": ("release", TypeError, lambda: TR(host_graph(), pts(), 0.1, release=torch.zeros(5, dtype=torch.bool))),
    "release-list-of-floats": ("release", TypeError, lambda: TR(host_graph(), pts(), 0.1, release=[0.0] * 5)),
    "release-number": ("release", TypeError, lambda: TR(host_graph(), pts(), 0.1, release=3)),
    "release-shape": ("release", ValueError, lambda: TR(host_graph(), pts(), 0.1, release=torch.zeros(4, dtype=I32))),
    "release-negative": ("release", ValueError, lambda: TR(host_graph(), pts(), 0.1, release=[0, 0, -1, 0, 0])),
    "release-too-late": ("release", ValueError, lambda: TR(host_graph(), pts(), 0.1, release=torch.full((5,), 2 ** 31, dtype=I64))),
    "streak-release_every-zero": ("release_every", ValueError, lambda: TR.streak(host_graph(), pts(), 0.1, release_every=0, releases=3)),
    "streak-release_every-float": ("release_every", ValueError, lambda: TR.streak(host_graph(), pts(), 0.1, release_every=2.0, releases=3)),
    "streak-releases-zero": ("releases", ValueError, lambda: TR.streak(host_graph(), pts(), 0.1, release_every=2, releases=0)),
    "streak-releases-bool": ("releases", ValueError, lambda: TR.streak(host_graph(), pts(), 0.1, release_every=2, releases=True)),
    "streak-releases-too-late": ("releases", ValueError, lambda: TR.streak(host_graph(), pts(1), 0.1, release_every=2 ** 30, releases=3)),
    "streak-release": ("release", ValueError, lambda: TR.streak(host_graph(), pts(), 0.1, releases=2, release=[0] * 10)),
    "streak-seeds": ("seeds", ValueError, lambda: TR.streak(host_graph(), [[0.0, 0.0]], 0.1, releases=2)),
    "streak-seeds-dim": ("seeds", ValueError, lambda: TR.streak(host_graph(), pts(5, 3), 0.1, releases=2)),
    "streak-scheme": ("scheme", ValueError, lambda: TR.streak(host_graph(), pts(), 0.1, releases=2, scheme="midpoint")),
}


@pytest.mark.parametrize("label", sorted(TRACERS_BAD))
def test_tracers_refuse(label):
    word, error, call = TRACERS_BAD[label]
    refused(word, call, error=error)


@pytest.mark.parametrize("call", [lambda: TR(host_graph(), pts(), 0.1), lambda: TR(host_graph(), pts(0), -0.5, scheme="euler"),
                                  lambda: TR(host_graph(dim=3), pts(5, 3), 1, k=16, power=0, velocity=(2, 0, 1), scale=2.0, shift=(0.0, 1.0, 2.0),
                                             box=((-INF, 0.0, 0.0), (INF, 1.0, 1.0)), max_distance=0.0, release=[0, 1, 2, 3, 4]),
                                  lambda: TR.streak(host_graph(), pts(), 0.1, release_every=3, releases=4, max_distance=0.5)])
def test_wellformed_tracers_on_the_host_stop_at_the_device_check(call):
    with pytest.raises(ValueError, match="no CPU fallback") as info:
        call()
    assert str(info.value).startswith("graph:")


def test_the_checked_description_holds_what_the_launch_needs():
    s = check_tracers(host_graph(dim=3), pts(5, 3), 1, scheme="euler", velocity=[2, 0, 1], scale=2, box=((-INF, 0, 0), (INF, 1, 1)), release=[4, 3, 2, 1, 0])
    assert (s["dim"], s["k"], s["power"], s["dt"], s["scheme"], s["velocity"]) == (3, 10, 2, 1.0, _lib.TRACER_EULER, [2, 0, 1])
    assert s["scale"] == [2.0] * 3 and s["shift"] == [0.0] * 3 and s["box_lo"] == [-INF, 0.0, 0.0] and s["max_distance"] == INF
    assert s["release"].dtype == I32 and s["release"].tolist() == [4, 3, 2, 1, 0] and s["seeds"].dtype == torch.float32 and s["groups"] is None
    assert check_tracers(host_graph(), pts(), 0.1)["k"] == 6 and check_tracers(host_graph(), pts(), 0.1)["release"].tolist() == [0] * 5


ROLLOUT_BAD = {
    "tracers-tensor": ("tracers", TypeError, dict(tracers=pts())),
    "tracers-list": ("tracers", TypeError, dict(tracers=[pts(), 0.1])),
    "tracers-one": ("tracers", TypeError, dict(tracers=(pts(),))),
    "tracers-options-no-dict": ("tracers", TypeError, dict(tracers=(pts(), 0.1, "heun"))),
    "tracers-unknown-option": ("tracers", TypeError, dict(tracers=(pts(), 0.1, dict(order=4)))),
    "tracers-seeds-int": ("tracers", ValueError, dict(tracers=(torch.zeros(5, 2, dtype=I64), 0.1))),
    "tracers-seeds-other-dim": ("tracers", ValueError, dict(tracers=(pts(5, 3), 0.1))),
    "tracers-dt": ("tracers", TypeError, dict(tracers=(pts(), None))),
    "tracers-dt-inf": ("tracers", ValueError, dict(tracers=(pts(), INF))),
    "tracers-velocity-beyond-the-fields": ("tracers", ValueError, dict(tracers=(pts(), 0.1, dict(velocity=(2, 3))))),
    "tracers-of-another-graph": ("tracers", ValueError, dict(tracers=fake_tracers(21))),
    "tracers-velocity-of-another-model": ("tracers", ValueError, dict(tracers=fake_tracers(velocity=(0, 3)))),
    "tracer_every-negative": ("tracer_every", ValueError, dict(tracers=(pts(), 0.1), tracer_every=-1)),
    "tracer_every-float": ("tracer_every", ValueError, dict(tracers=(pts(), 0.1), tracer_every=1.0)),
    "tracer_every-bool": ("tracer_every", ValueError, dict(tracers=(pts(), 0.1), tracer_every=True)),
    "tracer_every-without-tracers": ("tracers", ValueError, dict(tracer_every=2)),
}


@pytest.mark.parametrize("label", sorted(ROLLOUT_BAD))
def test_rollout_refuses(label):
    word, error, kw = ROLLOUT_BAD[label]
    refused(word, Rollout, SimpleNamespace(num_fields=3), host_graph(), 7, error=error, **kw)


def test_rollout_refuses_a_velocity_the_model_does_not_have():
    refused("tracers", Rollout, SimpleNamespace(num_fields=1), host_graph(nf=1), 7, tracers=(pts(), 0.1))
    refused("tracers", Rollout, SimpleNamespace(num_fields=2), host_graph(dim=3, nf=2), 7, tracers=(pts(5, 3), 0.1))


@pytest.mark.parametrize("kw", [dict(tracers=(pts(), 0.1)), dict(tracers=fake_tracers(), tracer_every=0), dict(tracers=(pts(0), 0.1), tracer_every=3),
                                dict(tracers=(pts(), 0.1, dict(scheme="euler", velocity=(2, 0))), samples=pts())])
def test_a_rollout_with_wellformed_tracers_stops_at_the_device_check(kw):
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Rollout(SimpleNamespace(num_fields=3), host_graph(), 7, **kw)


def fake_model(nf=3):
    m = SimpleNamespace(num_fields=nf)
    m._rollout = lambda *a, **kw: GNN._rollout(m, *a, **kw)
    m.eval = lambda: (_ for _ in ()).throw(AssertionError("the model was touched before the arguments were checked"))
    return m


MODEL_BAD = {
    "seeds-int": ("tracers", ValueError, lambda m: GNN.trace(m, host_graph(), 7, torch.zeros(5, 2, dtype=I64), 0.1)),
    "dt-missing": ("tracers", TypeError, lambda m: GNN.trace(m, host_graph(), 7, pts())),
    "option": ("tracers", ValueError, lambda m: GNN.trace(m, host_graph(), 7, pts(), 0.1, scheme="rk4")),
    "unknown-option": ("tracers", TypeError, lambda m: GNN.trace(m, host_graph(), 7, pts(), 0.1, order=2)),
    "every": ("tracer_every", ValueError, lambda m: GNN.trace(m, host_graph(), 7, pts(), 0.1, every=-1)),
    "tracers-with-dt": ("tracers", ValueError, lambda m: GNN.trace(m, host_graph(), 7, fake_tracers(), 0.1)),
    "list": ("tracers", ValueError, lambda m: GNN.trace(m, [host_graph(), host_graph()], 7, pts(), 0.1)),
    "evaluate-list": ("tracers", ValueError, lambda m: GNN.evaluate(m, [host_graph(), host_graph()], 7, tracers=(pts(), 0.1))),
    "evaluate-seeds": ("tracers", ValueError, lambda m: GNN.evaluate(m, host_graph(), 7, tracers=(pts(5, 3), 0.1))),
    "evaluate-tracer_every": ("tracer_every", ValueError, lambda m: GNN.evaluate(m, host_graph(), 7, tracers=(pts(), 0.1), tracer_every=-2)),
}


@pytest.mark.parametrize("label", sorted(MODEL_BAD))
def test_the_model_refuses_before_anything_is_moved(label):
    word, error, call = MODEL_BAD[label]
    refused(word, call, fake_model(), error=error)


SIGNATURES = {          # (name,) or (name, default); "=name": keyword-only, "**name": the rest
    "Rollout.__init__": [('self',), ('model',), ('graph',), ('max_steps',), ('capture', True), ('reorder', None), ('label', 'Rollout'), ('every', 1),
                         ('probes', None), ('target', None), ('mask', None), ('moments', None), ('error_moments', None), ('derived', None),
                         ('derived_every', 0), ('derived_moments', None), ('derived_options', None), ('spectrum', None), ('target_spectrum', False),
                         ('derived_spectrum', None), ('samples', None), ('sample_every', 1), ('sample_moments', None), ('sample_spectrum', None),
                         ('sample_derived', False), ('tracers', None), ('tracer_every', 1), ('forces', None), ('force_moments', None),
                         ('force_spectrum', None), ('wall_moments', None), ('target_forces', False)],
    "GNN.evaluate": [('self',), ('graph',), ('n_out', None), ('=every', 0), ('=probes', None), ('=capture', None), ('=moments', None),
                     ('=error_moments', None), ('=derived', None), ('=derived_every', 0), ('=derived_moments', None), ('=derived_options', None),
                     ('=spectrum', None), ('=samples', None), ('=sample_every', 1), ('=sample_moments', None), ('=sample_spectrum', None),
                     ('=sample_derived', False), ('=tracers', None), ('=tracer_every', 1), ('=forces', None), ('=force_moments', None),
                     ('=force_spectrum', None), ('=wall_moments', None), ('=modes', None)],
    "GNN._rollout": [('self',), ('graph',), ('n_out',), ('capture',), ('label',), ('evaluate', False), ('**records',)],
    "GNN.solve": [('self',), ('graph',), ('n_out',), ('=capture', None), ('=every', 1)],
    "GNN.diagnostics": [('self',), ('graph',), ('n_out',), ('derived', ('div', 'vort')), ('=every', 0), ('=discard', None), ('=stride', 1),
                        ('=capture', None), ('**derived_options',)],
    "GNN.sample": [('self',), ('graph',), ('n_out',), ('points',), ('=every', 1), ('=discard', None), ('=stride', 1), ('=spectrum', None),
                   ('=derived', None), ('=capture', None), ('**derived_options',)],
    "GNN.trace": [('self',), ('graph',), ('n_out',), ('seeds',), ('dt', None), ('=every', 1), ('=capture', None), ('**options',)],
    "GNN.forces": [('self',), ('graph',), ('n_out',), ('bodies', None), ('=discard', None), ('=stride', 1), ('=spectrum', None), ('=wall', False),
                   ('=capture', None), ('**options',)],
    "GNN.time_statistics": [('self',), ('graph',), ('n_out',), ('=discard', 0), ('=stride', 1), ('=every', 0), ('=capture', None)],
    "GNN.spectrum": [('self',), ('graph',), ('n_out',), ('bins', None), ('freqs', None), ('=discard', 0), ('=stride', 1), ('=samples', None),
                     ('=dt', 1.0), ('=taper', 'rect'), ('=derived', None), ('=every', 0), ('=capture', None), ('**derived_options',)],
    "GNN.modes": [('self',), ('graph',), ('n_out',), ('modes', None), ('=every', 1), ('=capture', None), ('**spec',)],
}


@pytest.mark.parametrize("name", sorted(SIGNATURES))
def test_the_public_signatures_of_the_rollout_stand(name):
    """Names, order, kinds and defaults of `Rollout.__init__` and of every `GNN` entry point that builds one, as literals."""
    import inspect
    owner, attr = name.split(".")
    got = []
    for p in inspect.signature(getattr({"Rollout": Rollout, "GNN": GNN}[owner], attr)).parameters.values():
        assert p.kind != p.VAR_POSITIONAL
        label = {p.VAR_KEYWORD: "**", p.KEYWORD_ONLY: "="}.get(p.kind, "") + p.name
        got.append((label,) if p.default is p.empty else (label, p.default))
    assert got == SIGNATURES[name]


def test_streaklines_and_residence_read_the_paths():
    m, n_seeds, dim, slots, every = 3, 2, 2, 4, 2
    paths = torch.arange(m * n_seeds * dim * slots, dtype=torch.float32).reshape(m * n_seeds, dim * slots)
    release = (torch.arange(m, dtype=I32) * 3).repeat_interleave(n_seeds)          # steps 0, 3, 6
    status = torch.tensor([1, 2, 3, 0, 4, 0], dtype=U8)
    stopped = torch.tensor([-1, 5, 3, -1, 7, -1], dtype=I32)
    rt = RolloutTracers(paths, paths[:, -dim:], status, stopped, release, paths[:, :dim], every=every, groups=(m, n_seeds))
    assert rt.slots == slots and rt.dim == dim and rt.target_paths is None
    line, released = rt.streakline(1)                                               # after step 3: the releases of steps 0 and 3 moved
    assert tuple(line.shape) == (n_seeds, m, dim) and tuple(released.shape) == (n_seeds, m)
    assert released.tolist() == [[True, True, False]] * 2
    for s in range(n_seeds):
        for i in range(m):
            assert torch.equal(line[s, i], paths[i * n_seeds + s, 2:4])
    assert rt.streakline(0)[1].tolist() == [[True, False, False]] * 2 and rt.streakline(-1)[1].all()
    assert torch.equal(rt.streakline()[0], rt.streakline(3)[0])
    assert rt.residence().tolist() == [-1, 5, 0, -1, 1, -1]
    for word, call in (("slot", lambda: rt.streakline(4)), ("slot", lambda: rt.streakline(-5)), ("slot", lambda: rt.streakline(0.0)),
                       ("streakline", RolloutTracers(paths, paths[:, -dim:], status, stopped, release, paths[:, :dim]).streakline),
                       ("streakline", RolloutTracers(None, paths[:, -dim:], status, stopped, release, paths[:, :dim], groups=(m, n_seeds)).streakline)):
        refused(word, call)


# ------------------------------------------------------------------ ops.tracer_advance
N, P, NF, STEPS = 12, 5, 3, 7


def grid(n=N, dim=2):
    return dict(pos_sorted=torch.zeros(n, dim), order=torch.zeros(n, dtype=I32), cell_start=torch.zeros(2, dtype=I32), n_cells=[1, 1, 1],
                org=(C.c_float * 3)(0.0, 0.0, 0.0), h=1.0, dim=dim, n=n)


def good():
    return dict(grid=grid(), x0=torch.zeros(N, NF), x1=torch.zeros(N, NF), q=torch.zeros(P, 2), status=torch.zeros(P, dtype=U8),
                stopped=torch.zeros(P, dtype=I32), release=torch.zeros(P, dtype=I32), dt=0.1, k=4, step=torch.zeros(2, dtype=I32), every=2,
                series=torch.zeros(STEPS // 2, P, 2), max_steps=STEPS, vel=torch.zeros(P, 2))


ADVANCE_BAD = {
    "grid-none": ("grid", dict(grid=None)),
    "grid-incomplete": ("grid", dict(grid=dict(pos_sorted=torch.zeros(N, 2)))),
    "k-zero": ("k", dict(k=0)),
    "k-17": ("k", dict(k=17)),
    "k-more-than-nodes": ("k", dict(k=13)),
    "power": ("power", dict(power=3)),
    "scheme": ("scheme", dict(scheme=2)),
    "x0-f64": ("x0", dict(x0=torch.zeros(N, NF, dtype=F64))),
    "x0-rows": ("x0", dict(x0=torch.zeros(N + 1, NF))),
    "x0-colstride": ("x0", dict(x0=torch.zeros(NF, N).t())),
    "x1-missing-for-heun": ("x1", dict(x1=None)),
    "x1-1d": ("x1", dict(x1=torch.zeros(N))),
    "q-dim": ("q", dict(q=torch.zeros(P, 3))),
    "q-f64": ("q", dict(q=torch.zeros(P, 2, dtype=F64))),
    "q-strided": ("q", dict(q=torch.zeros(P, 3)[:, :2])),
    "status-bool": ("status", dict(status=torch.zeros(P, dtype=torch.bool))),
    "status-rows": ("status", dict(status=torch.zeros(P + 1, dtype=U8))),
    "stopped-i64": ("stopped", dict(stopped=torch.zeros(P, dtype=I64))),
    "release-i64": ("release", dict(release=torch.zeros(P, dtype=I64))),
    "vel-shape": ("vel", dict(vel=torch.zeros(P, 3))),
    "vcol-short": ("vcol", dict(vcol=[0])),
    "vcol-past": ("vcol", dict(vcol=[0, NF])),
    "vcol-past-x1": ("vcol", dict(vcol=[0, 2], x1=torch.zeros(N, 2))),
    "vcol-negative": ("vcol", dict(vcol=[-1, 0])),
    "scale-short": ("scale", dict(scale=[1.0])),
    "shift-str": ("shift", dict(shift="ab")),
    "box_lo-3d": ("box_lo", dict(box_lo=[0.0, 0.0, 0.0])),
    "box_hi-short": ("box_hi", dict(box_hi=[1.0])),
    "every-negative": ("every", dict(every=-1)),
    "max_steps-negative": ("max_steps", dict(max_steps=-1)),
    "series-without-every": ("series", dict(every=0)),
    "every-without-series": ("series", dict(series=None)),
    "series-shape": ("series", dict(series=torch.zeros(STEPS // 2, P, 3))),
    "series-f64": ("series", dict(series=torch.zeros(STEPS // 2, P, 2, dtype=F64))),
    "step-i64": ("step", dict(step=torch.zeros(2, dtype=I64))),
    "step-empty": ("step", dict(step=torch.zeros(0, dtype=I32))),
}


@pytest.mark.parametrize("label", sorted(ADVANCE_BAD))
def test_tracer_advance_refuses(label):
    word, patch = ADVANCE_BAD[label]
    assert "tracer_advance" in refused(word, ops.tracer_advance, **dict(good(), **patch))


@pytest.mark.parametrize("patch", [dict(), dict(x1=None, scheme=_lib.TRACER_EULER, step=None, t=3, every=0, series=None, vel=None),
                                   dict(x0=torch.zeros(N, NF + 4)[:, 2:2 + NF], vcol=[2, 0], scale=[2.0, 0.5], shift=[0.1, 0.2], box_lo=[0.0, -INF], box_hi=[1.0, INF])])
def test_a_wellformed_launch_on_the_host_stops_at_the_device_check(patch):
    with pytest.raises(ValueError, match="no CPU fallback") as info:
        ops.tracer_advance(**dict(good(), **patch))
    assert str(info.value).startswith("q:")


def test_the_descriptor_matches_the_header():
    """LP64: three pointers; 3 + 3 + 1 + 3 four-byte words; two pointers; 2 + 3 + 3 + 3 + 1 + 1 + 3 + 3 + 1 = 20 words; one pointer; four
    words; six pointers — no padding anywhere."""
    t = _lib.g4c_tracer_t
    assert (t.pos_sorted.offset, t.order.offset, t.cell_start.offset, t.n_cells.offset, t.origin.offset, t.cell_size.offset, t.dim.offset, t.k.offset,
            t.power.offset, t.x0.offset, t.x1.offset, t.x0_ld.offset, t.x1_ld.offset, t.vcol.offset, t.scale.offset, t.shift.offset, t.dt.offset,
            t.scheme.offset, t.box_lo.offset, t.box_hi.offset, t.max_distance.offset, t.step.offset, t.t_host.offset, t.max_steps.offset, t.every.offset,
            t.n_slots.offset, t.series.offset, t.q.offset, t.status.offset, t.stopped.offset, t.release.offset, t.vel.offset) == (
        0, 8, 16, 24, 36, 48, 52, 56, 60, 64, 72, 80, 84, 88, 100, 112, 124, 128, 132, 144, 156, 160, 168, 172, 176, 180, 184, 192, 200, 208, 216, 224)
    assert C.sizeof(t) == 232
    assert (_lib.TRACER_EULER, _lib.TRACER_HEUN) == (0, 1) and gfd.tracers.SCHEMES == {"euler": 0, "heun": 1}
    assert (gfd.tracers.WAITING, gfd.tracers.MOVING, gfd.tracers.LEFT, gfd.tracers.FAR, gfd.tracers.NONFINITE) == (0, 1, 2, 3, 4)
    assert "g4c_tracer_advance" in _lib.EXPORTED_SYMBOLS
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "g4c.h")).read()
    body = header[header.index("typedef struct g4c_tracer {"):header.index("} g4c_tracer_t;")]
    import re
    names = [n for line in body.splitlines()[1:] for n in re.findall(r"\*?\b([a-z_0-9]+)(?:\[3\])?\s*[,;]", line.split("/*")[0])]
    assert names == [f[0] for f in t._fields_], names
