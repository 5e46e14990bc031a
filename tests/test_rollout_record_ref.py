"""The fp64 restatement of g4c_rollout_advance_record (tests/record_ref.py) against oracle/mem_ref.py where the two overlap, and the
negative controls of the checkers the GPU test (test_gpu_rollout_record.py) uses: what a correct launch leaves (the restatement's
own result, rounded to the buffers' formats) fails each checker against a restatement with one deliberate mistake.  Host only."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import record_ref as R                                   # noqa: E402
from oracle import mem_ref as M                          # noqa: E402

F32, F64, I32 = torch.float32, torch.float64, torch.int32
SENT = -7777.0
N, NF, COLS, STEPS = 257, 3, 7, 7


def _data(kind, seed=0):
    g = torch.Generator().manual_seed(seed)
    if kind == "int":
        draw = lambda *s: torch.randint(-8, 9, s, generator=g).to(F32)      # noqa: E731
    else:
        draw = lambda *s: torch.randn(*s, generator=g)                       # noqa: E731
    return dict(field=draw(N, COLS), preds=[draw(N, NF) for _ in range(STEPS + 1)], target=draw(N, NF * STEPS + 5),
                mask=torch.rand(N, generator=g) < 0.3, probe_rows=torch.tensor([0, 5, 5, 100, N - 2], dtype=I32))


def _buffers(every):
    n_snap = STEPS // every if every else 0
    return dict(snap=torch.full((n_snap, N, NF), SENT, dtype=F64) if every else None,
                probe_out=torch.full((STEPS, 5, NF), SENT, dtype=F64), stats=torch.full((STEPS, NF, R.NSTAT), SENT, dtype=F64))


def _run(c, every, wrong=None, steps=STEPS + 1):
    """`steps` consecutive calls; returns the state after each."""
    b, f, states = _buffers(every), c["field"], []
    for t in range(steps):
        o = R.advance_record(f, c["preds"][t], t, STEPS, every=every, probe_rows=c["probe_rows"], target=c["target"][:, 2:],
                             mask=c["mask"], wrong=wrong, **b)
        f, b = o["field"], dict(snap=o["snap"], probe_out=o["probe_out"], stats=o["stats"])
        assert o["step"] == t + 1
        states.append(o)
    return states


@pytest.mark.parametrize("every", [1, 2, 3, 9])
def test_restatement_agrees_with_mem_ref(every):
    c = _data("float")
    states = _run(c, every)
    f, outs = c["field"].double(), torch.full((STEPS, N, NF), SENT, dtype=F64)
    for t in range(STEPS):
        f, outs, t1 = M.rollout_advance(f, c["preds"][t], outs, t, "steps")
        assert torch.equal(states[t]["field"], f) and states[t]["step"] == t1
    kept = [t for t in range(STEPS) if (t + 1) % every == 0][: STEPS // every]
    assert torch.equal(states[STEPS - 1]["snap"], outs[kept])
    if every == 1:
        assert torch.equal(states[STEPS - 1]["snap"], outs)
    # the call past max_steps moves the field and the step and leaves every record alone
    last, past = states[STEPS - 1], states[STEPS]
    assert torch.equal(past["field"], torch.cat((f[:, NF:], c["preds"][STEPS].double()), 1)) and past["step"] == STEPS + 1
    for k in ("snap", "probe_out", "stats"):
        assert torch.equal(past[k], last[k]), k
    # probes and statistics against their definitions
    rows = c["probe_rows"].long()
    tg = c["target"][:, 2:].double()
    for t in range(STEPS):
        p, y = c["preds"][t].double(), tg[:, NF * t:NF * (t + 1)]
        assert torch.equal(last["probe_out"][t], p[rows])
        d = p - y
        want = torch.stack(((d * d).sum(0), d.abs().sum(0), d.abs().max(0).values, y.sum(0), (y * y).sum(0),
                            (d.abs() * c["mask"][:, None]).sum(0)), 1)
        assert torch.equal(last["stats"][t], want)


def test_every_zero_and_no_nodes_record_nothing():
    c = _data("int")
    o = R.advance_record(c["field"], c["preds"][0], 0, STEPS, every=0, probe_rows=None, target=None)
    assert o["snap"] is None and o["probe_out"] is None and o["stats"] is None and o["step"] == 1
    e = R.advance_record(torch.zeros(0, COLS), torch.zeros(0, NF), 3, STEPS, snap=torch.full((STEPS, 0, NF), SENT), every=1,
                         target=torch.zeros(0, NF * STEPS), stats=torch.full((STEPS, NF, R.NSTAT), SENT))
    assert e["step"] == 4 and bool((e["stats"] == SENT).all())


@pytest.mark.parametrize("kind", ["int", "float"])
@pytest.mark.parametrize("wrong", R.WRONG)
def test_checkers_reject_each_mistake(wrong, kind):
    """`got` is what a correct launch leaves after three calls (fp32 buffers, fp64 statistics); the reference makes one mistake."""
    c = _data(kind)
    every = 2
    good, bad = _run(c, every, steps=3)[-1], _run(c, every, wrong=wrong, steps=3)[-1]
    got = dict(snap=good["snap"].to(F32), probe_out=good["probe_out"].to(F32), stats=good["stats"])
    for k in ("snap", "probe_out", "stats"):
        R.same(got[k], good[k], k)                         # (the checker accepts the right answer)
    t = 1                                                  # the step every = 2 keeps in slot 0
    n = N
    tgt = c["target"][:, 2:]

    def stats_check(ref_run):
        for s in range(3):
            R.stats_close(got["stats"][s], ref_run["stats"][s], R.step_stats(c["preds"][s], tgt, s, c["mask"])[1], n, f"step {s}")

    stats_check(good)
    if wrong in ("slot+1", "keep-t"):
        assert R.rejects(R.same, got["snap"], bad["snap"], wrong)
        assert not torch.equal(good["snap"][0], torch.full_like(good["snap"][0], SENT)), t
    elif wrong == "probe+1":
        assert R.rejects(R.same, got["probe_out"], bad["probe_out"], wrong)
    else:
        assert R.rejects(R.same, got["stats"], bad["stats"], wrong)
        assert R.rejects(stats_check, bad), wrong
