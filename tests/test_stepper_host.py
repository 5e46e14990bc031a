"""`_stepper.StepDriver` on the host: the decision trace (eager / capture / replay) of one scripted life and what `validate()` does
after a clip, on a stand-in subclass — no GPU, no library call."""
import warnings

import pytest
import torch

from graphs4cfd_amd import ops
from graphs4cfd_amd._stepper import StepDriver


class _Graph:
    def __init__(self, trace):
        self.trace = trace

    def replay(self):
        self.trace.append("replay")


class _Static:
    def __init__(self):
        self.answers = []           # what the next stale() calls say (then False)

    def stale(self):
        return self.answers.pop(0) if self.answers else False


class _Flags:
    def __init__(self):
        self.script = []            # what the next take() calls return (then nothing)

    def take(self):
        return self.script.pop(0) if self.script else []


class Driver(StepDriver):
    def __init__(self, max_steps=64, capture=True, elsewhere=False):
        self._init_driver(torch.zeros(3, 2), torch.zeros(max_steps, 3, 2), max_steps, capture)
        self.static, self.flags = _Static(), _Flags()
        self.trace, self.precisions, self.warned, self.restarts = [], [], [], []
        self.elsewhere = elsewhere

    def _step(self):
        self.precisions.append(ops.mlp_precision())         # (the arithmetic every step of whatever kind runs in)
        super()._step()

    def _one(self):
        self.trace.append("eager")

    def _capture(self):
        self.trace.append("capture")
        self._hipgraph = _Graph(self.trace)
        self._hipgraph.replay()

    def _any_rank(self, flag):
        return flag or self.elsewhere

    def _warn_clipped(self, hit, n):
        self.warned.append((list(hit), n))
        warnings.warn(f"stand-in: {n} step(s) recomputed", RuntimeWarning, stacklevel=3)

    def _restarted(self, again):
        self.restarts.append(again)


@pytest.fixture
def f16x3():
    old = ops.set_mlp_precision("f16x3")
    yield
    ops.set_mlp_precision(old)


def test_decision_trace_of_one_scripted_life():
    d = Driver()
    assert (d._hipgraph, d._pins, d._epoch, d._first_slot, d.capture_error, d.captured) == (None, None, -1, 0, None, False)
    d.run(3)
    assert d.trace == ["eager", "capture", "replay", "replay"] and d.captured
    del d.trace[:]
    ops.bump_weights_epoch()                    # new weights: one eager step, then a new capture
    d.run(2)
    assert d.trace == ["eager", "capture", "replay"] and d.captured
    del d.trace[:]
    d.static.answers = [True]                   # an edited per-mesh constant: the same
    d.run(2)
    assert d.trace == ["eager", "capture", "replay"] and d.captured
    del d.trace[:]
    d.run(2)
    assert d.trace == ["replay", "replay"] and d.steps_done == 9
    # the stale check also sits in front of a capture (a step ABOUT to be captured): that step is eager, the next one captures
    e = Driver()
    e.run(1)
    e.static.answers = [True]
    e.run(2)
    assert e.trace == ["eager", "eager", "capture", "replay"]


def test_without_capture_every_step_is_eager_and_the_buffer_bounds_the_steps():
    d = Driver(max_steps=4, capture=False)
    assert d.capture_error == "capture not requested"
    d.run(2)
    ops.bump_weights_epoch()
    d.run(2)
    assert d.trace == ["eager"] * 4 and not d.captured and d.steps_done == 4
    with pytest.raises(RuntimeError, match=r"^rollout buffer holds 4 steps$"):
        d.step()
    assert d.steps_done == 4 and d.trace == ["eager"] * 4


def test_validate_without_a_hit_changes_nothing(f16x3):
    d = Driver()
    d.run(3)
    graph, trace = d._hipgraph, list(d.trace)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert d.validate() is False
    assert (d.steps_done, d.exact_range, d._hipgraph, d.trace, d.restarts) == (3, False, graph, trace, [])
    ops.set_mlp_precision("bf16x6")             # another arithmetic: the flags are not even read
    d.flags.script = [["mlp"]]
    assert d.validate() is False and d.flags.script == [["mlp"]]


@pytest.mark.parametrize("first_slot", [0, 2])
def test_validate_after_a_clip_takes_the_steps_again_in_bf16x6(f16x3, first_slot):
    d = Driver()
    d.run(5)
    d._first_slot = first_slot                  # (what Rollout.rewind() sets: the recomputation starts from this slot)
    d.field.fill_(7.0)
    d.flags.script = [["a.edge_mlp", "b.node_mlp"]]
    del d.trace[:], d.precisions[:]
    with pytest.warns(RuntimeWarning, match="recomputed") as rec:
        assert d.validate() is True
    n = 5 - first_slot
    assert len(rec) == 1 and rec[0].filename == __file__                         # (attributed to the caller of validate())
    assert d.warned == [(["a.edge_mlp", "b.node_mlp"], n)] and d.restarts == [True]
    assert d.exact_range and d.steps_done == 5 and d.precisions == ["bf16x6"] * n
    assert d.trace == ["eager", "capture"] + ["replay"] * (n - 1)                # (the old graph was dropped with the epoch)
    assert ops.mlp_precision() == "f16x3"                                        # (put back behind every step)
    assert torch.equal(d.field, d._field0) and d.step_counter.tolist() == [first_slot, 0]
    d.flags.script = [["a.edge_mlp"]]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert d.validate() is False            # silent, and the flags are left alone
    assert d.flags.script == [["a.edge_mlp"]] and d.steps_done == 5
    d.step()
    assert d.precisions[-1] == "bf16x6" and ops.mlp_precision() == "f16x3"      # the rollout stays in it, the process does not


def test_a_clip_on_another_rank_recomputes_this_one_too(f16x3):
    d = Driver(elsewhere=True)
    d.run(3)
    with pytest.warns(RuntimeWarning, match="recomputed"):
        assert d.validate() is True
    assert d.warned == [([], 3)] and d.exact_range and d.steps_done == 3


class _BaseCapture(Driver):
    """The stand-in with `StepDriver._capture` itself, the three torch.cuda names it uses replaced by recorders."""
    _capture = StepDriver._capture

    def __init__(self, monkeypatch, fail=False):
        super().__init__()
        self.fail = fail
        trace = self.trace

        class Capture:
            def __init__(self, graph):
                trace.append("capture-begin")

            def __enter__(self):
                return self

            def __exit__(self, *exc):
                trace.append("capture-end")
                return False

        monkeypatch.setattr(torch.cuda, "synchronize", lambda device=None: trace.append("synchronise"))
        monkeypatch.setattr(torch.cuda, "CUDAGraph", lambda: _Graph(trace))
        monkeypatch.setattr(torch.cuda, "graph", Capture)

    def _one(self):
        if self.fail and self.steps_done == 1:
            raise ValueError("the launch could not be captured")
        super()._one()


def test_base_capture_order_and_a_capture_that_raises_leaves_no_graph_behind(monkeypatch):
    d = _BaseCapture(monkeypatch)
    d.run(3)
    assert d.trace == ["eager", "synchronise", "capture-begin", "eager", "capture-end", "replay", "replay"]
    assert d.captured and isinstance(d._pins, list)
    d = _BaseCapture(monkeypatch, fail=True)
    d.step()
    with pytest.raises(ValueError, match="could not be captured"):          # the exception still propagates ...
        d.step()
    assert d._hipgraph is None and not d.captured and d.steps_done == 1     # ... and nothing is left that the next step would replay
    assert d.trace == ["eager", "synchronise", "capture-begin", "capture-end"]
