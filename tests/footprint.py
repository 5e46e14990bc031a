"""Where a launch writes: guard arenas around every output, bit-exact copies of every input (test-only helpers).

`arena` puts the [rows, cols] window a launch is given into the middle of one allocation that is filled with a bit pattern no launch
produces (a quiet NaN with a payload); `assert_footprint` compares as integers — NaN never compares equal as a float — and demands
that every element outside the window still holds the pattern and that every element of every row the launch owns no longer does.
`frozen` is the same promise for inputs: bit-exact copies on entry, bit equality on exit.  tests/test_footprint_host.py is the negative
control of all of it, on the host: nothing perturbs a launch."""
import contextlib

import torch

# quiet NaNs with a payload, one per element size; the integer view they are compared through
PATTERN = {2: (torch.int16, 0x7FD3), 4: (torch.int32, 0x7FC12345), 8: (torch.int64, 0x7FF8000012345678)}
GUARD_ROWS = 64          # a whole pair of 32-row tiles: the largest row block of any MLP kernel (mlp_ws_kernel, mlp_bx6i_kernel)


def _int_view(t):
    """`t` reinterpreted as integers of its element size (same shape, same strides: a view)."""
    t = t.as_subclass(torch.Tensor)
    if t.dtype == torch.bool:
        return t.view(torch.uint8)
    if not (t.dtype.is_floating_point or t.dtype.is_complex):
        return t
    return t.view(PATTERN[t.element_size()][0])


def fill(whole):
    idt, pat = PATTERN[whole.element_size()]
    whole.view(idt).fill_(pat)
    return whole


def arena(rows, cols, dtype, *, guard_rows=GUARD_ROWS, col0=8, pad_cols=8, device="cpu"):
    """(view, whole): `whole` is one allocation of rows + 2 guard_rows rows and col0 + cols + pad_cols columns filled with the pattern,
    `view` its [rows, cols] window in the middle — what the launch is given.  The defaults keep a window of 128 columns on the vector
    paths of every kernel (16-byte aligned rows of fp32 and bf16 alike, a leading dimension that is a multiple of 8); an odd col0 or
    pad_cols gives the unaligned paths their window."""
    assert rows >= 0 and cols >= 1 and guard_rows >= 0 and col0 >= 0 and pad_cols >= 0
    whole = fill(torch.empty((rows + 2 * guard_rows, col0 + cols + pad_cols), dtype=dtype, device=device))
    return whole[guard_rows:guard_rows + rows, col0:col0 + cols], whole


def flat_arena(n, dtype, *, guard=4096, device="cpu"):
    """(view, whole) for a 1-D buffer of n elements (scratch, a flat output): `guard` pattern elements in front of it and behind it."""
    whole = fill(torch.empty((1, n + 2 * guard), dtype=dtype, device=device))
    return whole[0, guard:guard + n], whole


def _window(whole, view):
    """(first row, first column, rows, columns) of `view` inside `whole`."""
    assert whole.dim() == 2 and whole.is_contiguous() and view.dtype == whole.dtype
    ld = int(whole.size(1))
    off = int(view.storage_offset() - whole.storage_offset())
    r0, c0 = divmod(off, ld)
    rows, cols = (1, int(view.size(0))) if view.dim() == 1 else (int(view.size(0)), int(view.size(1)))
    assert view.dim() == 1 or rows <= 1 or int(view.stride(0)) == ld
    assert 0 <= r0 and r0 + rows <= whole.size(0) and 0 <= c0 and c0 + cols <= ld
    return r0, c0, rows, cols


def owned(whole, view, rows=None):
    """Bool mask over `whole`: the elements the launch owns.  `rows` None: the whole window; a bool mask / an index tensor / a range
    over the window's rows: those rows of it; a bool mask of the window's shape: those elements."""
    r0, c0, n, cols = _window(whole, view)
    mask = torch.zeros(whole.shape, dtype=torch.bool, device=whole.device)
    win = mask[r0:r0 + n, c0:c0 + cols]
    if rows is None:
        win[:] = True
    elif torch.is_tensor(rows) and rows.dtype == torch.bool and rows.dim() == 2:
        win[:] = rows.to(whole.device)
    else:
        sel = torch.zeros(n, dtype=torch.bool, device=whole.device)
        if isinstance(rows, range):
            rows = torch.arange(rows.start, rows.stop, rows.step)
        rows = torch.as_tensor(rows).to(whole.device)
        if rows.dtype == torch.bool:
            sel[:] = rows
        elif rows.numel():
            assert int(rows.min()) >= 0 and int(rows.max()) < n
            sel[rows.long()] = True
        win[:] = sel[:, None]
    return mask


def assert_footprint(whole, view, written_rows=None, what="", inside=True):
    """Every element of `whole` outside the owned part of the window still holds the pattern — the guard rows above and below, the
    columns left and right, the rows of the window that `written_rows` (see `owned`) does not name — and, with `inside`, every owned
    element no longer holds it.  (`inside=False`: scratch, of which a launch may use less than it was promised.)"""
    idt, pat = PATTERN[whole.element_size()]
    changed = whole.view(idt) != pat
    own = owned(whole, view, written_rows)
    r0, c0, n, cols = _window(whole, view)
    stray = changed & ~own
    if bool(stray.any()):
        at = torch.nonzero(stray)
        r, c = int(at[0, 0]) - r0, int(at[0, 1]) - c0
        where = ("above" if r < 0 else "below" if r >= n else "left of" if c < 0 else "right of" if c >= cols else "in a row nobody owns of")
        raise AssertionError(f"{what}: {int(at.size(0))} element(s) written outside what the launch owns, the first at (row {r}, column {c}) "
                             f"relative to the [{n}, {cols}] window ({where} the window)")
    if inside:
        left = own & ~changed
        if bool(left.any()):
            at = torch.nonzero(left)
            raise AssertionError(f"{what}: {int(at.size(0))} owned element(s) left unwritten, the first at (row {int(at[0, 0]) - r0}, "
                                 f"column {int(at[0, 1]) - c0}) relative to the [{n}, {cols}] window")


def assert_footprint_chunked(whole, view, written_rows=None, what="", inside=True, chunk_rows=1 << 20):
    """`assert_footprint` for an arena too tall for masks of its own size (tests/test_gpu_tall.py): the same two demands, checked
    `chunk_rows` rows of `whole` at a time.  `written_rows`: None (the whole window) or a bool mask over the window's rows (on the
    arena's device)."""
    idt, pat = PATTERN[whole.element_size()]
    r0, c0, n, cols = _window(whole, view)
    assert written_rows is None or (written_rows.dtype == torch.bool and tuple(written_rows.shape) == (n,))
    ints = whole.view(idt)
    for lo in range(0, int(whole.size(0)), chunk_rows):
        hi = min(lo + chunk_rows, int(whole.size(0)))
        changed = ints[lo:hi] != pat
        own = torch.zeros(changed.shape, dtype=torch.bool, device=whole.device)
        a, b = max(lo, r0), min(hi, r0 + n)
        if a < b:
            if written_rows is None:
                own[a - lo:b - lo, c0:c0 + cols] = True
            else:
                own[a - lo:b - lo, c0:c0 + cols] = written_rows[a - r0:b - r0, None]
        stray = changed & ~own
        if bool(stray.any()):
            at = torch.nonzero(stray)
            raise AssertionError(f"{what}: {int(at.size(0))} element(s) written outside what the launch owns, the first at (row "
                                 f"{int(at[0, 0]) + lo - r0}, column {int(at[0, 1]) - c0}) relative to the [{n}, {cols}] window")
        if inside:
            left = own & ~changed
            if bool(left.any()):
                at = torch.nonzero(left)
                raise AssertionError(f"{what}: {int(at.size(0))} owned element(s) left unwritten, the first at (row "
                                     f"{int(at[0, 0]) + lo - r0}, column {int(at[0, 1]) - c0}) relative to the [{n}, {cols}] window")


def equal_bits_chunked(a, b, chunk_rows=1 << 20):
    """Bit equality of two tensors of one shape and dtype, `chunk_rows` of the first dimension at a time: None, or the first row
    (index into the first dimension) at which they differ."""
    assert a.shape == b.shape and a.dtype == b.dtype
    for lo in range(0, int(a.size(0)), chunk_rows):
        x, y = _int_view(a[lo:lo + chunk_rows]), _int_view(b[lo:lo + chunk_rows])
        if not torch.equal(x, y):
            return lo + int(torch.nonzero((x != y).reshape(x.size(0), -1).any(1))[0])
    return None


@contextlib.contextmanager
def frozen(*tensors, what=""):
    """Bit-exact copies of `tensors` (any dtype, any strides; None entries are skipped) on entry, bit equality on exit."""
    live = [(j, t) for j, t in enumerate(tensors) if t is not None]
    before = [_int_view(t.detach()).clone() for _, t in live]
    yield
    for (j, t), b in zip(live, before):
        now = _int_view(t.detach())
        if not torch.equal(now, b):
            at = torch.nonzero(now != b)
            raise AssertionError(f"{what}: input {j} (shape {tuple(t.shape)}, {t.dtype}) changed in {int(at.size(0))} element(s), the first at "
                                 f"{tuple(int(x) for x in at[0])}")
