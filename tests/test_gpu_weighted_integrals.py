"""g4c_weighted_integrals (csrc/control_volumes.hip) through ops.weighted_integrals against tests/integrals_ref.py: stats[t] EQUAL — bit
for bit — to the numpy restatement of the device's order, and within 2 (N + 4) 2⁻⁵³ Σ|terms| of math.fsum over the same terms; rows of
zero weight contribute nothing whatever they hold (the rule of tests/test_gpu_nonfinite.py), a NaN in a weighted row poisons only the
entries that read its column, a step outside the record writes nothing, two runs agree, the scratch is exactly the promised size."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

import integrals_ref as R                                      # noqa: E402
from footprint import assert_footprint, flat_arena, frozen     # noqa: E402
from graphs4cfd_amd import _lib, ops                           # noqa: E402

DEV = torch.device("cuda", 0)
F32, F64, I32 = torch.float32, torch.float64, torch.int32
NZ, LD, MAX_STEPS, T = 4, 7, 5, 3
# every entry form: (a, b), (a, a), (a, −1), (−1, −1) — eight of them, the most a launch takes
ENTRIES = [(0, 1), (2, 2), (3, -1), (-1, -1), (1, 3), (0, 0), (-1, 2), (1, 1)]
SIZES = (1, 63, 64, 65, 257, 1500, 1024 * 256 + 300)          # the last: above one workgroup's share of one row a thread


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def data(n, seed=0):
    rng = np.random.default_rng(40 + n + seed)
    x = rng.standard_normal((n, LD)).astype(np.float32)                      # a prediction: x_ld = 7 > nz = 4
    tgt = rng.standard_normal((n, NZ * MAX_STEPS + 3)).astype(np.float32)      # a target holding every step
    w = rng.random(n) * 10.0 ** rng.integers(-3, 1, n)
    w[rng.random(n) < 0.1] = 0.0
    return x, tgt, w


SOURCES = {
    "prediction": lambda x, tgt: dict(x=x, sub=None, x_step=0, sub_step=0),
    "prediction-target": lambda x, tgt: dict(x=x, sub=tgt, x_step=0, sub_step=NZ),
    "target": lambda x, tgt: dict(x=tgt, sub=None, x_step=NZ, sub_step=0),
}


def launch(src, w, entries, t=T, step=None, stats=None, scratch=None):
    n, ne = src["x"].shape[0], len(entries)
    xd, sd, wd = dev(src["x"]), None if src["sub"] is None else dev(src["sub"]), dev(w)
    if stats is None:
        stats, stats_whole = flat_arena(MAX_STEPS * ne, F64, device=DEV)
    else:
        stats_whole = None
    if scratch is None:
        scratch, scratch_whole = flat_arena(R.scratch_doubles(n, ne), F64, device=DEV)
    else:
        scratch_whole = None
    with frozen(xd, sd, wd, step, what="weighted_integrals"):
        ops.weighted_integrals(xd, wd, entries, stats.view(MAX_STEPS, ne), scratch, nz=NZ, sub=sd, x_step=src["x_step"],
                               sub_step=src["sub_step"], step=step, t=t)
        torch.cuda.synchronize()
    return stats.view(MAX_STEPS, ne), stats_whole, scratch, scratch_whole


@pytest.mark.parametrize("source", list(SOURCES))
@pytest.mark.parametrize("n", SIZES)
def test_sums_against_the_restatement(n, source):
    x, tgt, w = data(n)
    src = SOURCES[source](x, tgt)
    stats, stats_whole, scratch, scratch_whole = launch(src, w, ENTRIES)
    # row T and nothing else of stats; the scratch: exactly the promised size, nothing beyond it
    rows = torch.zeros(MAX_STEPS * len(ENTRIES), dtype=torch.bool)
    rows[T * len(ENTRIES):(T + 1) * len(ENTRIES)] = True
    assert_footprint(stats_whole, stats.view(-1), rows.view(1, -1), what="stats")
    used = torch.ones((1, scratch.numel()), dtype=torch.bool)
    used[0, 1:R.HEADER] = False          # (the header's unused entries: the partials start on a 64-byte boundary)
    assert_footprint(scratch_whole, scratch, used, what="scratch")
    assert scratch.numel() == int(_lib.load().g4c_weighted_integrals_scratch_doubles(n, len(ENTRIES)))
    Tm, keep = R.terms(src["x"], w, ENTRIES, src["sub"], src["x_step"], src["sub_step"], T)
    got = stats[T].cpu().numpy()
    want = R.sum_order(Tm, keep)
    assert np.array_equal(got.view(np.int64), want.view(np.int64)), (got, want)
    err, bound = np.abs(got - R.sum_exact(Tm, keep)), R.sum_bound(Tm, keep)
    print(f"{source}-{n}: largest |device − fsum| / bound = {np.divide(err, bound, out=np.zeros_like(err), where=bound > 0).max():.3e}")
    assert (err <= bound).all()


@pytest.mark.parametrize("ne", [1, 2, 3, 5, 7])
def test_every_entry_count(ne):
    x, tgt, w = data(1500, seed=ne)
    src = SOURCES["prediction-target"](x, tgt)
    stats, _, _, _ = launch(src, w, ENTRIES[:ne])
    Tm, keep = R.terms(src["x"], w, ENTRIES[:ne], src["sub"], 0, NZ, T)
    assert np.array_equal(stats[T].cpu().numpy().view(np.int64), R.sum_order(Tm, keep).view(np.int64))


def test_rows_of_zero_weight_contribute_nothing():
    x, tgt, w = data(1500)
    clean = launch(SOURCES["prediction-target"](x, tgt), w, ENTRIES)[0][T].clone()
    zero = np.nonzero(w == 0.0)[0]
    assert zero.size > 50
    x2, tgt2 = x.copy(), tgt.copy()
    x2[zero[0::3]] = np.nan
    x2[zero[1::3]] = np.inf
    tgt2[zero[2::3]] = -np.inf
    got = launch(SOURCES["prediction-target"](x2, tgt2), w, ENTRIES)[0][T]
    assert torch.equal(got.view(torch.int64), clean.view(torch.int64))
    w2 = w.copy()
    w2[zero[0]] = -0.0          # a negative zero is a zero
    got = launch(SOURCES["prediction-target"](x2, tgt2), w2, ENTRIES)[0][T]
    assert torch.equal(got.view(torch.int64), clean.view(torch.int64))


def test_a_nan_poisons_only_the_entries_that_read_its_column():
    x, tgt, w = data(1500)
    clean = launch(SOURCES["prediction"](x, tgt), w, ENTRIES)[0][T].clone()
    row = int(np.nonzero(w != 0.0)[0][7])
    x2 = x.copy()
    x2[row, 2] = np.nan
    got = launch(SOURCES["prediction"](x2, tgt), w, ENTRIES)[0][T]
    reads = torch.tensor([2 in e for e in ENTRIES], device=DEV)
    assert bool(torch.isnan(got[reads]).all()) and int(reads.sum()) == 2
    assert torch.equal(got[~reads].view(torch.int64), clean[~reads].view(torch.int64))


@pytest.mark.parametrize("t", [MAX_STEPS, MAX_STEPS + 100, -1])
def test_a_step_outside_the_record_writes_nothing(t):
    x, tgt, w = data(257)
    step = torch.tensor([t, 0], dtype=I32, device=DEV)
    stats, stats_whole, _, _ = launch(SOURCES["prediction"](x, tgt), w, ENTRIES, step=step)
    assert_footprint(stats_whole, stats.view(-1), torch.zeros((1, stats.numel()), dtype=torch.bool), what="stats")
    assert step.tolist() == [t, 0]


def test_the_step_index_is_read_on_the_device_and_two_runs_agree():
    x, tgt, w = data(1500)
    src = SOURCES["target"](x, tgt)
    ne = len(ENTRIES)
    stats = torch.zeros(MAX_STEPS * ne, dtype=F64, device=DEV)
    scratch = ops.weighted_integrals_scratch(1500, ne, DEV)
    step = torch.zeros(2, dtype=I32, device=DEV)
    for t in range(MAX_STEPS):
        step[0] = t
        launch(src, w, ENTRIES, t=99, step=step, stats=stats, scratch=scratch)          # (`t` is ignored when `step` is given)
    again = torch.zeros_like(stats)
    for t in reversed(range(MAX_STEPS)):
        launch(src, w, ENTRIES, t=t, stats=again, scratch=scratch)
    assert torch.equal(stats.view(torch.int64), again.view(torch.int64))
    for t in (0, MAX_STEPS - 1):
        Tm, keep = R.terms(src["x"], w, ENTRIES, None, NZ, 0, t)
        assert np.array_equal(stats.view(MAX_STEPS, ne)[t].cpu().numpy().view(np.int64), R.sum_order(Tm, keep).view(np.int64))


def test_no_rows():
    stats = torch.full((2, 3), 7.0, dtype=F64, device=DEV)
    ops.weighted_integrals(torch.zeros((0, 4), device=DEV), torch.zeros(0, dtype=F64, device=DEV), [(0, 0), (1, -1), (-1, -1)], stats,
                           ops.weighted_integrals_scratch(0, 3, DEV), t=1)
    assert stats.tolist() == [[7.0] * 3, [0.0] * 3]
