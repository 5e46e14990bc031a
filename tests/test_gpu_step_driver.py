"""`_stepper.StepDriver` under both rollouts, on the device: what only `Rollout` had a test for.  A captured `DistributedRollout`
(world = 1) drops its hipGraph and captures again after new weights and after an in-place edit of a per-mesh constant, bit for bit
the eager steps; and the clip warning of either class keeps its text and the frame it is attributed to.

The frames were recorded on the parent commit (`f635923`) with the lines of `test_clip_warning_*` below run as a script:
    Rollout.validate()                   -> the line that called it                       (script.py:35, the call)
    Rollout.result()                     -> graphs4cfd_amd/nn/rollout.py:315, the `self.validate()` of `Rollout.result`
    DistributedRollout.gather_outputs()  -> the line that called it                       (script.py:43, the call)
i.e. `Rollout` blames the caller of `validate()`, `DistributedRollout` the caller of what called `validate()`."""
import inspect
import re

import pytest
import torch

import graphs4cfd_amd as gfd
from graphs4cfd_amd import ops, partition as P, synthetic as S
from graphs4cfd_amd.nn.model import Rollout

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _model(seed):
    torch.manual_seed(seed)
    return gfd.nn.NsTwoScaleGNN(arch=S.mus_arch("NsTwoScaleGNN", 128), device=DEV)


def _halve_decoder(model):
    for p in model.node_decoder.parameters():
        p.data.mul_(0.5)                       # does not advance p._version
    model.invalidate_packed()


def test_distributed_rollout_recaptures_after_new_weights():
    """The shape of test_invalidate_packed_and_rollout_recapture, on DistributedRollout."""
    g = S.mus_graph(3000, levels=2, seed=41)
    model = _model(42)
    w_old = {k: v.clone() for k, v in model.state_dict().items()}
    dr = P.DistributedRollout(model, g, 6, 0, 1, DEV)
    dr.run(3)
    assert dr.captured and dr.capture_error is None
    first = dr._hipgraph
    _halve_decoder(model)
    dr.run(3)                                  # eager on the new weights, captured again, replayed
    assert dr.captured and dr._hipgraph is not first
    got = dr.gather_outputs()
    # the same 3 + 3 steps with eager launches only
    model.load_state_dict(w_old)
    ref = P.DistributedRollout(model, g, 6, 0, 1, DEV, capture=False)
    ref.run(3)
    _halve_decoder(model)
    ref.run(3)
    assert not ref.captured and ref.capture_error == "capture not requested"
    want = ref.gather_outputs()
    assert torch.equal(got, want), (got - want).abs().max().item()
    # (the edit shows: with the old weights throughout, the last three steps differ)
    model.load_state_dict(w_old)
    same = P.DistributedRollout(model, g, 6, 0, 1, DEV)
    same.run(6)
    unedited = same.gather_outputs()
    nf = dr.nf
    assert torch.equal(unedited[:, : 3 * nf], got[:, : 3 * nf]) and not torch.equal(unedited[:, 3 * nf:], got[:, 3 * nf:])


def test_distributed_rollout_recaptures_after_an_edited_constant():
    """The captured part of test_static_encoder_cache_is_bit_identical_and_invalidates, on DistributedRollout: `edge_attr` of the
    rank's sub-mesh edited in place between two steps."""
    g = S.mus_graph(3000, levels=2, seed=71)
    model = _model(72)
    outs = {}
    for capture in (True, False):
        dr = P.DistributedRollout(model, g, 6, 0, 1, DEV, capture=capture)
        dr.run(3)                                  # eager, captured, replayed
        assert dr.captured == capture and dr.static.misses >= 1
        first, misses = dr._hipgraph, dr.static.misses
        dr.mesh.edge_attr.mul_(1.5)
        dr.run(1)                                  # stale: eager again
        assert dr.static.misses > misses and not dr.captured
        dr.run(2)                                  # captured again, replayed
        assert dr.captured == capture and (not capture or dr._hipgraph is not first)
        outs[capture] = dr.gather_outputs()
    assert torch.isfinite(outs[True]).all()
    assert torch.equal(outs[True], outs[False]), (outs[True] - outs[False]).abs().max().item()
    plain = P.DistributedRollout(model, g, 6, 0, 1, DEV)
    plain.run(6)
    nf = plain.nf
    unedited = plain.gather_outputs()
    assert torch.equal(unedited[:, : 3 * nf], outs[True][:, : 3 * nf]) and not torch.equal(unedited[:, 3 * nf:], outs[True][:, 3 * nf:])


ROLLOUT_TEXT = (r"^Rollout: the default 'f16x3' MLP arithmetic reached the end of the fp16 range \(\|x\| >= 65504\) in NsTwoScaleGNN\.[\w., ]+: "
                r"the 4 step\(s\) were recomputed in 'bf16x6' \(fp32's exponent range\) and this rollout continues in it — the result holds no "
                r"clipped value\.  gfd\.set_mlp_precision\('bf16x6'\) avoids the second pass for this model\.$")
DISTRIBUTED_TEXT = (r"^DistributedRollout \(rank 0\): the default 'f16x3' MLP arithmetic reached the end of the fp16 range \(\|x\| >= 65504\) in "
                    r"NsTwoScaleGNN\.[\w., ]+: the 4 step\(s\) were recomputed in 'bf16x6' \(fp32's exponent range\) and this rollout "
                    r"continues in it\.$")


@pytest.fixture(scope="module")
def clipping():
    """(model, graph) of the suite's clip recipe: one LayerNorm gain scaled by 3e4 takes the next MLP's input past 65504."""
    g = S.mus_graph(3000, levels=2, seed=16)
    model = _model(17)
    with torch.no_grad():
        model.mp111.edge_mlp.MLP.layer_norm.weight.mul_(3e4)
    model.invalidate_packed()
    return model, g


@pytest.fixture
def f16x3():
    old = ops.set_mlp_precision("f16x3")
    ops.f16_range_clear()
    yield
    ops.set_mlp_precision(old)


def _line() -> int:
    return inspect.currentframe().f_back.f_lineno


def _only(rec, text):
    clips = [r for r in rec if "fp16 range" in str(r.message)]
    assert len(clips) == 1 and clips[0].category is RuntimeWarning and re.match(text, str(clips[0].message)), [str(r.message) for r in rec]
    return clips[0].filename, clips[0].lineno


@pytest.mark.parametrize("how", ["validate", "result"])
def test_clip_warning_of_rollout_keeps_text_and_frame(clipping, f16x3, how):
    model, g = clipping
    with Rollout(model, g.clone().to(DEV), 4, capture=True) as ro:
        ro.run(4)
        with pytest.warns(RuntimeWarning) as rec:
            here = _line() + 1
            ro.validate() if how == "validate" else ro.result()
        assert ro.exact_range and ro.steps_done == 4 and ro.captured
    if how == "validate":
        want = (__file__, here)
    else:       # (the `self.validate()` of `Rollout.result`: line 315 of nn/rollout.py on the parent)
        src, first = inspect.getsourcelines(Rollout.result)
        want = (inspect.getsourcefile(Rollout), first + [k for k, text in enumerate(src) if text.strip() == "self.validate()"][0])
    assert _only(rec, ROLLOUT_TEXT) == want


def test_clip_warning_of_distributed_rollout_keeps_text_and_frame(clipping, f16x3):
    model, g = clipping
    dr = P.DistributedRollout(model, g, 4, 0, 1, DEV)
    dr.run(4)
    with pytest.warns(RuntimeWarning) as rec:
        here = _line() + 1
        dr.gather_outputs()
    assert dr.exact_range and dr.steps_done == 4 and dr.captured
    assert _only(rec, DISTRIBUTED_TEXT) == (__file__, here)
