"""Operands tall enough that a row offset held in 32 bits wraps, and the row windows that see such a wrap (shared by
tests/test_tall_host.py — the negative control, CPU only — and tests/test_gpu_tall.py — the launches).

A [M, 128] operand has three places where a 32-bit quantity wraps: the signed byte offset at 2^31 bytes, the unsigned byte offset
(a buffer instruction's vector offset) at 2^32 bytes and, for fp32, the `int` element index at 2^31 elements — rows 2^22, 2^23 and
2^24 of an fp32 operand, rows 2^23 and 2^24 of a bf16 one.  M_TALL = 2^24 + 4096 + 37 rows cross all of them at the production
leading dimension and leave a partial last tile.

Data.  An operand's value is a pure function `value(seed, row, column)` of integer arithmetic that torch evaluates identically on
the host and on the device (int64 products that stay below 2^63, shifts, masks): any window of an 8.6 GB operand is generated
without the operand, and `fill_` writes the operand on the device chunk by chunk.  Kind "int": integers in -8 .. 8 (the sums of the
exact helper launches stay exact, as oracle.mem_ref.int_operand); kind "float": k / 2^15 * 3 - 3 for a 16-bit k, in [-3, 3) (the MLP
launches, and narrow operands — two rows of three columns collide with probability 2^-48, not 17^-3).

Windows of an operand: rows [0, 256), [b - 256, b + 256) around every boundary row b of the operand, and the last 256 + tail rows.
256 rows are four of the largest row block of any kernel (footprint.GUARD_ROWS = 64).  A wrapped offset reads or writes a row that
is 2^22, 2^23 or 2^24 rows (or a sum or difference of those) away; `wrap_deltas` lists those distances and test_tall_host.py checks
that no two rows that far apart are equal in the compared columns, so a wrap cannot land on an equal row."""
import torch

M_TALL = 2 ** 24 + 4096 + 37
MARGIN = 256
H = 128
I64 = torch.int64


# ---------------------------------------------------------------- boundaries and windows
def boundary_rows(row_bytes, cols, n_rows, elements=True):
    """The rows of an operand of `n_rows` rows of `row_bytes` bytes and `cols` elements each at which a 32-bit quantity wraps: the
    first row at or beyond 2^31 bytes, at or beyond 2^32 bytes and (elements: fp32 operands, whose kernels index by element) at or
    beyond 2^31 elements — those that the operand reaches, ascending, without repeats."""
    limits = [(2 ** 31, row_bytes), (2 ** 32, row_bytes)] + ([(2 ** 31, cols)] if elements else [])
    rows = sorted({-(-lim // per) for lim, per in limits})
    return [b for b in rows if b < n_rows]


def windows(n_rows, bounds, tail=0, margin=MARGIN):
    """[(lo, hi)] row ranges, ascending and disjoint: the first `margin` rows, `margin` rows on either side of every boundary, the last
    `margin + tail` rows."""
    spans = [(0, margin)] + [(b - margin, b + margin) for b in bounds] + [(n_rows - margin - tail, n_rows)]
    spans = sorted((max(lo, 0), min(hi, n_rows)) for lo, hi in spans)
    out = []
    for lo, hi in spans:
        if hi <= lo:
            continue
        if out and lo <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], hi))
        else:
            out.append((lo, hi))
    return out


def window_rows(wins, device=None):
    """The rows of `wins` as one int64 vector."""
    return torch.cat([torch.arange(lo, hi, dtype=I64, device=device) for lo, hi in wins])


def tall_windows(n_rows=M_TALL, row_bytes=4 * H, cols=H, tail=0, elements=True):
    return windows(n_rows, boundary_rows(row_bytes, cols, n_rows, elements), tail)


def wrap_deltas():
    """Every non-zero a 2^22 + b 2^23 + c 2^24 with a, b, c in {-1, 0, 1}: how far from the right row a wrapped offset can land."""
    out = set()
    for a in (-1, 0, 1):
        for b in (-1, 0, 1):
            for c in (-1, 0, 1):
                out.add(a * 2 ** 22 + b * 2 ** 23 + c * 2 ** 24)
    out.discard(0)
    return sorted(out)


# ---------------------------------------------------------------- row-keyed data
def _mix(seed, r, c):
    """32 mixed bits per (seed, row, column) of the broadcast int64 tensors r, c; every product stays below 2^63 for |row| < 2^27."""
    h = (r * 2654435761 + c * 40503 + (int(seed) * 7919 + 12345)) & 0xFFFFFFFF
    h = ((h ^ (h >> 15)) * 0x2545F491) & 0xFFFFFFFF
    h = ((h ^ (h >> 13)) * 0x1B873593) & 0xFFFFFFFF
    return h ^ (h >> 16)


def _hash(seed, rows, cols):
    """int64 [len(rows), len(cols)]."""
    return _mix(seed, rows[:, None], cols[None, :])


def _as_values(h, kind, dtype):
    if kind == "int":
        v = (h % 17 - 8).to(torch.float32)
    elif kind == "float":
        v = (h & 0xFFFF).to(torch.float32) * (3.0 / 32768.0) - 3.0          # (exact: 16 bits x 3, then an exact subtraction)
    else:
        raise ValueError(kind)
    return v.to(dtype)


def value_at(seed, flat, n_cols, kind="float", dtype=torch.float32):
    """The elements `flat` (int64, any shape: row x n_cols + column) of the operand `seed` of `n_cols` columns."""
    flat = torch.as_tensor(flat, dtype=I64)
    return _as_values(_mix(seed, flat // n_cols, flat % n_cols), kind, dtype)


def value(seed, rows, n_cols, kind="float", dtype=torch.float32, col0=0):
    """[len(rows), n_cols] of the operand `seed`: its rows `rows` (an int64 vector on any device, any values), columns col0 .. ."""
    rows = torch.as_tensor(rows, dtype=I64)
    cols = torch.arange(col0, col0 + n_cols, dtype=I64, device=rows.device)
    return _as_values(_hash(seed, rows, cols), kind, dtype)


def fill_(t, seed, kind="float", chunk=2 ** 18, row0=0):
    """t[r, c] = value(seed, row0 + r, c) for a 2-D tensor on any device, `chunk` rows at a time (the int64 temporaries stay small)."""
    n, c = int(t.size(0)), int(t.size(1))
    for lo in range(0, n, chunk):
        hi = min(lo + chunk, n)
        t[lo:hi] = value(seed, torch.arange(row0 + lo, row0 + hi, dtype=I64, device=t.device), c, kind, t.dtype)
    return t


# ---------------------------------------------------------------- wrong addressings (the host control's subject)
def _signed32(x):
    return ((x + 2 ** 31) % 2 ** 32) - 2 ** 31


def wrapped_row(row, row_bytes, cols, how):
    """The row that `row`'s first element is found in when its offset is held in 32 bits: "signed_bytes" (offset = row x row_bytes
    as int32), "unsigned_bytes" (as uint32), "signed_elements" (row x cols as int32).  Negative: in front of the allocation."""
    if how == "signed_bytes":
        return _signed32(row * row_bytes) // row_bytes
    if how == "unsigned_bytes":
        return ((row * row_bytes) % 2 ** 32) // row_bytes
    if how == "signed_elements":
        return _signed32(row * cols) // cols
    raise ValueError(how)


WRAPS = ("signed_bytes", "unsigned_bytes", "signed_elements")
