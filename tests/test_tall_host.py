"""The negative control of the tall-operand scheme (tests/tall_cases.py, tests/test_gpu_tall.py), on the host with no library: an
operand is modelled as its row function, a gather and a scatter are evaluated with each of three WRONG addressings — the row's byte
offset in a signed and in an unsigned 32-bit integer, its element index in a signed one — and the window checks of the device tests
must reject all six, and accept the right addressing.  Second half: no two rows 2^22, 2^23, 2^24 (or a sum or difference of those)
apart are equal in the compared columns, so a wrapped offset never lands on an equal row."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import tall_cases as T          # noqa: E402

SEED = 5
ROW_BYTES, COLS = 4 * T.H, T.H          # an fp32 [M_TALL, 128] operand
PRIOR = -77.0                           # what an output row holds before the launch (no operand value: those lie in -8 .. 8)
WINS = T.tall_windows()
ROWS = T.window_rows(WINS)


def test_boundaries_and_windows():
    assert T.boundary_rows(ROW_BYTES, COLS, T.M_TALL) == [2 ** 22, 2 ** 23, 2 ** 24]
    assert T.boundary_rows(2 * T.H, T.H, T.M_TALL, elements=False) == [2 ** 23, 2 ** 24]          # bf16 rows
    assert T.boundary_rows(ROW_BYTES, COLS, 2 ** 23 + 1) == [2 ** 22, 2 ** 23]                      # an operand that ends sooner
    assert WINS == [(0, 256), (2 ** 22 - 256, 2 ** 22 + 256), (2 ** 23 - 256, 2 ** 23 + 256), (2 ** 24 - 256, 2 ** 24 + 256),
                    (T.M_TALL - 256, T.M_TALL)]
    assert T.windows(1000, [100, 300], tail=37) == [(0, 556), (1000 - 293, 1000)]                   # overlapping spans merge
    assert int(ROWS.numel()) == 256 * 8 and T.M_TALL % 32 == 5 and T.M_TALL % 64 == 37              # a partial last tile and pair
    assert T.M_TALL * COLS >= 2 ** 31 + 4096 * COLS and T.M_TALL * ROW_BYTES >= 2 ** 32


def test_value_is_a_function_of_seed_row_and_column():
    full = T.fill_(torch.empty(1000, 128), SEED, "float", chunk=300)
    assert torch.equal(full[37:61], T.value(SEED, torch.arange(37, 61), 128))
    assert torch.equal(full[:, 5:9], T.value(SEED, torch.arange(1000), 4, col0=5))
    assert not torch.equal(full, T.fill_(torch.empty(1000, 128), SEED + 1, "float"))
    ints = T.value(SEED, ROWS, 128, "int")
    assert float(ints.abs().max()) == 8.0 and torch.equal(ints, ints.round()) and len(ints.unique()) == 17
    fl = T.value(SEED, ROWS, 128, "float")
    assert -3.0 <= float(fl.min()) < -2.99 and 2.99 < float(fl.max()) < 3.0
    assert torch.equal(T.value(SEED, ROWS, 128, "float", torch.bfloat16), fl.to(torch.bfloat16))
    flat = torch.tensor([[0, 5, 127], [128 * 37 + 3, 128 * 999 + 127, 128 * 500]])          # elements by their flat index
    assert torch.equal(T.value_at(SEED, flat, 128), full.reshape(-1)[flat])


def _gather(idx, how):
    """What a gather of the rows `idx` returns: right (`how` None) or with the row's offset wrapped."""
    rows = idx if how is None else T.wrapped_row(idx, ROW_BYTES, COLS, how)
    return T.value(SEED, rows, COLS, "int")


def _scatter(how):
    """The window rows of the output of a launch that writes value(r) to row r for every r < M_TALL — to the wrapped row under a wrong
    addressing: a window row holds what the last row that lands on it wrote, or PRIOR if none does."""
    out = torch.full((int(ROWS.numel()), COLS), PRIOR)
    best = torch.full((int(ROWS.numel()),), -1, dtype=T.I64)
    periods = [j * 2 ** 23 for j in range(-4, 5)] + [-2 ** 25, 2 ** 25]          # byte offsets repeat every 2^23 rows, elements every 2^25
    for d in periods:
        r = ROWS + d
        lands = (r >= 0) & (r < T.M_TALL)
        if how is not None:
            lands &= T.wrapped_row(r, ROW_BYTES, COLS, how) == ROWS
        else:
            lands &= r == ROWS
        best = torch.where(lands & (r > best), r, best)
    hit = best >= 0
    out[hit] = T.value(SEED, best[hit], COLS, "int")
    return out


def window_check(got, want):
    """The device tests' criterion for exact launches: bit equality on the window rows."""
    assert torch.equal(got, want), f"{int((got != want).any(1).sum())} window rows differ"


def test_right_addressing_passes():
    window_check(_gather(ROWS, None), T.value(SEED, ROWS, COLS, "int"))
    window_check(_scatter(None), T.value(SEED, ROWS, COLS, "int"))


@pytest.mark.parametrize("how", T.WRAPS)
def test_window_checks_reject_a_wrapped_gather(how):
    got = _gather(ROWS, how)
    with pytest.raises(AssertionError):
        window_check(got, T.value(SEED, ROWS, COLS, "int"))
    # ... and exactly from that addressing's first boundary on: the rows below it are right
    first = {"signed_bytes": 2 ** 22, "unsigned_bytes": 2 ** 23, "signed_elements": 2 ** 24}[how]
    wrong = (got != T.value(SEED, ROWS, COLS, "int")).any(1)
    assert not bool(wrong[ROWS < first].any()) and bool(wrong[(ROWS >= first) & (ROWS < first + 256)].all())


@pytest.mark.parametrize("how", T.WRAPS)
def test_window_checks_reject_a_wrapped_scatter(how):
    with pytest.raises(AssertionError):
        window_check(_scatter(how), T.value(SEED, ROWS, COLS, "int"))


@pytest.mark.parametrize("kind,cols", [("int", 128), ("float", 128), ("float", 3)])
def test_rows_a_wrap_apart_differ(kind, cols):
    """Otherwise a wrap onto an equal row passes: every window row differs somewhere in the compared columns from the rows 2^22, 2^23,
    2^24 and every sum and difference of those away (inside the operand or not: a wrapped offset may point outside it)."""
    deltas = T.wrap_deltas()
    assert deltas == [j * 2 ** 22 for j in range(-7, 8) if j] and {2 ** 22, 2 ** 23, 2 ** 24, -2 ** 22, 2 ** 24 - 2 ** 22, 2 ** 22 + 2 ** 23 + 2 ** 24} <= set(deltas)
    here = T.value(SEED, ROWS, cols, kind)
    for d in deltas:
        there = T.value(SEED, ROWS + d, cols, kind)
        same = (here == there).all(1)
        assert not bool(same.any()), f"{int(same.sum())} rows equal the row {d:+d} away ({kind}, {cols} columns)"
