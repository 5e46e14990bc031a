"""The rule by which the operator losses (FlowLoss, SampleLoss, ForceLoss, ResidualLoss) keep what they built from a batch: the base
class's `keep(tensors, build)` alone, on host tensors — no operator, no device."""
import torch

from graphs4cfd_amd.nn.losses import FlowLoss, ForceLoss, ResidualLoss, SampleLoss, _OperatorLoss


def counting():
    made = []

    def build():
        made.append(object())
        return made[-1]
    return made, build


def test_nothing_is_kept_before_the_first_build():
    for loss in (_OperatorLoss(0), FlowLoss(), SampleLoss(torch.zeros(3, 2)), ForceLoss(), ResidualLoss(nu=0.01, dt=0.1)):
        assert loss._cache is None and loss.builds == 0


def test_the_same_objects_unmodified_are_not_rebuilt():
    loss, (made, build) = _OperatorLoss(0), counting()
    a, b = torch.zeros(4, 2), torch.arange(6)
    first = loss.keep([a, b], build)
    assert first is made[0] and loss.builds == 1 and loss._cache is not None
    for _ in range(3):
        assert loss.keep([a, b], build) is first
    assert loss.builds == 1 and len(made) == 1


def test_an_in_place_write_to_any_key_tensor_rebuilds():
    loss, (made, build) = _OperatorLoss(0), counting()
    key = [torch.zeros(4, 2), torch.arange(6), torch.ones(3)]
    loss.keep(key, build)
    for i, t in enumerate(key):
        t.add_(1)          # the same object, a new `_version`
        assert loss.keep(key, build) is made[-1] and loss.builds == i + 2
        assert loss.keep(key, build) is made[-1] and loss.builds == i + 2          # ... and kept again from then on
    key[0].view(-1)[0] = 5.0          # a write through a view counts
    loss.keep(key, build)
    assert loss.builds == 5 and len(made) == 5


def test_an_equal_valued_different_object_rebuilds():
    loss, (made, build) = _OperatorLoss(0), counting()
    a, b = torch.zeros(4, 2), torch.arange(6)
    first = loss.keep([a, b], build)
    assert loss.keep([a.clone(), b], build) is not first and loss.builds == 2
    assert loss.keep([a, b.clone()], build) is made[2] and loss.builds == 3
    assert loss.keep([a.view(4, 2), b], build) is made[3] and loss.builds == 4          # a view of the same storage is another object
    assert loss.keep([a, b], build) is made[4] and loss.builds == 5                     # one entry: the first key was dropped


def test_a_none_entry_is_stable_and_is_not_a_tensor():
    loss, (made, build) = _OperatorLoss(0), counting()
    a = torch.zeros(4, 2)
    first = loss.keep([a, None], build)
    assert loss.keep([a, None], build) is first and loss.builds == 1
    assert loss.keep([a, torch.zeros(0)], build) is made[1] and loss.builds == 2          # None -> a tensor
    assert loss.keep([a, None], build) is made[2] and loss.builds == 3                    # ... and back
    assert loss.keep([a], build) is made[3] and loss.builds == 4                          # a key of another length


def test_a_build_that_raises_keeps_nothing_and_counts_nothing():
    loss = _OperatorLoss(0)

    def build():
        raise ValueError("graph: no")
    for _ in range(2):
        try:
            loss.keep([torch.zeros(2)], build)
        except ValueError:
            pass
    assert loss._cache is None and loss.builds == 0
