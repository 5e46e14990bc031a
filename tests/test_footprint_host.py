"""The negative control of the write-footprint tests (tests/footprint.py), on the host: a clean arena passes; one stray element in each
of the five regions — guard above, guard below, left pad, right pad, an owned element left unwritten — is rejected with its
coordinates; `frozen` rejects a one-bit change.  Nothing perturbs a launch: the "launch" here is a host assignment."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import footprint as FP          # noqa: E402

DTYPES = [torch.float32, torch.bfloat16, torch.float64]
ROWS, COLS = 5, 12


def written(dtype, **kw):
    """An arena whose window a well-behaved launch has written (ordinary values, a NaN and an infinity among them)."""
    view, whole = FP.arena(ROWS, COLS, dtype, **kw)
    view.copy_(torch.arange(ROWS * COLS, dtype=torch.float32).reshape(ROWS, COLS).to(dtype))
    view[1, 2], view[2, 3] = float("nan"), float("inf")
    return view, whole


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_layout_and_pattern(dtype):
    view, whole = FP.arena(ROWS, COLS, dtype, guard_rows=64, col0=8, pad_cols=4)
    assert tuple(whole.shape) == (ROWS + 128, 8 + COLS + 4) and tuple(view.shape) == (ROWS, COLS)
    assert view.data_ptr() == whole.data_ptr() + (64 * whole.size(1) + 8) * whole.element_size() and view.stride(0) == whole.size(1)
    idt, pat = FP.PATTERN[whole.element_size()]
    assert bool((whole.view(idt) == pat).all()) and bool(torch.isnan(whole).all())
    # an untouched arena: nothing stray, and nothing written either
    FP.assert_footprint(whole, view, written_rows=[], what="untouched")
    with pytest.raises(AssertionError, match=rf"{ROWS * COLS} owned element\(s\) left unwritten, the first at \(row 0, column 0\)"):
        FP.assert_footprint(whole, view, what="untouched")
    flat, fw = FP.flat_arena(10, dtype, guard=7)
    assert tuple(fw.shape) == (1, 24) and flat.data_ptr() == fw.data_ptr() + 7 * fw.element_size() and tuple(flat.shape) == (10,)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_a_clean_arena_passes(dtype):
    view, whole = written(dtype)
    FP.assert_footprint(whole, view, what="clean")
    # a launch that owns rows 1 and 3 only (an output index, a row sub-range) and wrote exactly those
    view, whole = FP.arena(ROWS, COLS, dtype)
    view[1], view[3] = 1.0, -2.0
    for rows in ([1, 3], torch.tensor([3, 1]), torch.tensor([False, True, False, True, False])):
        FP.assert_footprint(whole, view, written_rows=rows, what="two rows")
    view[3:5] = 0.5
    with pytest.raises(AssertionError, match=r"first at \(row 1, column 0\).*in a row nobody owns"):
        FP.assert_footprint(whole, view, written_rows=range(3, 5), what="sub-range")
    # scratch: less written than promised is fine, anything outside is not
    flat, fw = FP.flat_arena(10, dtype, guard=7)
    flat[:4] = 1.0
    FP.assert_footprint(fw, flat, what="scratch", inside=False)
    fw[0, 17] = 0.0
    with pytest.raises(AssertionError, match=r"first at \(row 0, column 10\).*right of"):
        FP.assert_footprint(fw, flat, what="scratch", inside=False)


STRAY = {          # region -> ((row, column) in `whole` of the stray element, its coordinates relative to the window, the words of the message)
    "guard-above": ((63, 8 + 5), (-1, 5), "above"),
    "guard-below": ((64 + ROWS, 8), (ROWS, 0), "below"),
    "left-pad": ((64 + 2, 7), (2, -1), "left of"),
    "right-pad": ((64 + 4, 8 + COLS), (4, COLS), "right of"),
}


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("region", sorted(STRAY))
def test_a_stray_element_is_rejected_with_its_coordinates(region, dtype):
    view, whole = written(dtype)
    (r, c), (wr, wc), word = STRAY[region]
    whole[r, c] = 0.0
    with pytest.raises(AssertionError) as info:
        FP.assert_footprint(whole, view, what=region)
    msg = str(info.value)
    assert f"{region}: 1 element(s) written outside" in msg and f"(row {wr}, column {wc})" in msg and f"({word} the window)" in msg, msg
    # a different NaN is a write too: only the integer comparison sees it
    view, whole = written(dtype)
    whole[r, c] = float("nan")
    with pytest.raises(AssertionError, match="1 element"):
        FP.assert_footprint(whole, view, what=region)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_an_owned_element_left_unwritten_is_rejected(dtype):
    view, whole = written(dtype)
    FP.assert_footprint(whole, view, what="clean")
    idt, pat = FP.PATTERN[whole.element_size()]
    whole.view(idt)[64 + 3, 8 + 7] = pat
    with pytest.raises(AssertionError) as info:
        FP.assert_footprint(whole, view, what="hole")
    assert "hole: 1 owned element(s) left unwritten, the first at (row 3, column 7)" in str(info.value), str(info.value)
    # a row the launch does not own must hold the pattern in every column, not in one
    with pytest.raises(AssertionError, match=r"11 element\(s\) written outside .* first at \(row 3, column 0\).*in a row nobody owns"):
        FP.assert_footprint(whole, view, written_rows=[0, 1, 2, 4], what="hole")


def test_owned_mask():
    view, whole = FP.arena(ROWS, COLS, torch.float32, guard_rows=2, col0=1, pad_cols=3)
    m = FP.owned(whole, view)
    assert int(m.sum()) == ROWS * COLS and bool(m[2:2 + ROWS, 1:1 + COLS].all())
    m = FP.owned(whole, view, rows=[0, 4])
    assert int(m.sum()) == 2 * COLS and bool(m[2, 1:1 + COLS].all()) and bool(m[6, 1:1 + COLS].all())
    part = torch.zeros(ROWS, COLS, dtype=torch.bool)
    part[:, :5] = True
    assert int(FP.owned(whole, view, rows=part).sum()) == 5 * ROWS


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64, torch.int32, torch.int64, torch.uint8, torch.bool], ids=str)
def test_frozen_rejects_a_one_bit_change(dtype):
    t = (torch.arange(24).reshape(4, 6) % 2).to(dtype) if dtype == torch.bool else torch.arange(24).reshape(4, 6).to(dtype)
    window = t[1:3, 2:5]          # (a strided view is frozen as it is)
    with FP.frozen(t, None, window, what="untouched"):
        pass
    bits = t.view(torch.uint8) if dtype == torch.bool else (t.view(FP.PATTERN[t.element_size()][0]) if dtype.is_floating_point else t)
    with pytest.raises(AssertionError) as info:
        with FP.frozen(None, t, what="one bit"):
            bits[2, 3] ^= 1
    assert "one bit: input 1" in str(info.value) and "1 element(s), the first at (2, 3)" in str(info.value), str(info.value)
    with pytest.raises(AssertionError, match=r"input 0 .* the first at \(1, 1\)"):
        with FP.frozen(window, what="window"):
            bits[2, 3] ^= 1
    if dtype.is_floating_point:          # NaN -> the same NaN is no change; NaN -> another NaN is one
        t[0, 0] = float("nan")
        with FP.frozen(t):
            t[0, 0] = t[0, 0].clone()
        with pytest.raises(AssertionError, match=r"the first at \(0, 0\)"):
            with FP.frozen(t):
                bits[0, 0] ^= 1


@pytest.mark.parametrize("chunk", [1, 7, 1000])
def test_the_chunked_forms_agree_with_the_whole_ones(chunk):
    """assert_footprint_chunked / equal_bits_chunked (tall arenas: tests/test_gpu_tall.py) accept and reject what the whole-tensor forms
    do, whatever the chunk: a clean arena, a stray element in a guard row and in a row nobody owns, an owned element left unwritten."""
    view, whole = FP.arena(20, 8, torch.float32, guard_rows=3, col0=0, pad_cols=0)
    rows = torch.zeros(20, dtype=torch.bool)
    rows[[0, 5, 19]] = True
    view[rows] = 1.0
    FP.assert_footprint(whole, view, rows)
    FP.assert_footprint_chunked(whole, view, rows, chunk_rows=chunk)
    for r, c, inside in ((1, 2, False), (3 + 6, 0, False), (3 + 5, 4, True)):          # guard row, unowned row, owned element
        keep = whole[r, c].clone()
        if inside:
            FP.fill(whole[r:r + 1, c:c + 1])
        else:
            whole[r, c] = 2.0
        for check in (lambda: FP.assert_footprint(whole, view, rows), lambda: FP.assert_footprint_chunked(whole, view, rows, chunk_rows=chunk)):
            with pytest.raises(AssertionError, match="left unwritten" if inside else "outside what the launch owns"):
                check()
        whole[r, c] = keep
    FP.assert_footprint_chunked(whole, view, rows, chunk_rows=chunk)
    view[:] = 1.0
    FP.assert_footprint_chunked(whole, view, chunk_rows=chunk)
    a = torch.arange(60, dtype=torch.float32).reshape(20, 3)
    b = a.clone()
    assert FP.equal_bits_chunked(a, b, chunk_rows=chunk) is None
    b[13, 1] = -b[13, 1]
    assert FP.equal_bits_chunked(a, b, chunk_rows=chunk) == 13
    n = torch.full((4, 2), float("nan"))
    assert FP.equal_bits_chunked(n, n.clone(), chunk_rows=chunk) is None          # (bits, not floats: NaN equals the same NaN)
