"""graphs4cfd_amd/_args.py, function by function, on the smallest inputs that separate right from wrong: CPU tensors, host metadata
only.  The wrappers' own refusals are pinned by tests/test_*_args.py, test_moments_host.py and test_spectrum_host.py."""
import numpy as np
import pytest
import torch

from graphs4cfd_amd import _args, _lib
from graphs4cfd_amd._args import Args

F32, F64, I32, I64, U8 = torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8
V, T = Args("fn"), Args("fn", TypeError)          # the two conventions for a wrong dtype


def refused(kind, name, call, *a, **k):
    with pytest.raises(kind) as e:
        call(*a, **k)
    assert type(e.value) is kind and str(e.value).startswith(f"{name}: fn: "), f"{type(e.value).__name__}: {e.value}"


def f(*shape, dtype=F32):
    return torch.zeros(*shape, dtype=dtype)


def test_dtype_and_tensor():
    for a, kind in ((V, ValueError), (T, TypeError)):
        refused(kind, "x", a.dtype, f(2, dtype=F64), "x", F32)
        refused(kind, "x", a.dtype, [0.0], "x", F32)
        refused(kind, "x", a.tensor, f(2, 2, dtype=I64), "x", I32)
        refused(kind, "m", a.tensor, f(3, dtype=I32), "m", (U8, torch.bool))
        a.tensor(f(3, dtype=torch.bool), "m", (U8, torch.bool), shape=(3,))
        refused(ValueError, "x", a.tensor, f(2, 4)[:, :2], "x", F32)          # contiguity
        refused(ValueError, "x", a.tensor, f(4), "x", F32, dim=2)
        refused(ValueError, "x", a.tensor, f(2, 3), "x", F32, shape=(3, 2))
        a.tensor(f(2, 3), "x", F32, dim=2, shape=(2, 3))
        a.tensor(f(0, 3), "x", F32, shape=(0, 3))


def test_strided_rows_shapes_and_layouts():
    a = V
    assert a.strided_rows(f(0, 3), "x") == (0, 3, 3)
    assert a.strided_rows(f(1, 3), "x") == (1, 3, 3)
    assert a.strided_rows(f(4, 1), "x") == (4, 1, 1)
    assert a.strided_rows(f(2, 2), "x") == (2, 2, 2)
    assert a.strided_rows(f(2, 6)[:, 1:3], "x") == (2, 2, 6)                          # a column window of a wider buffer
    assert a.strided_rows(f(1, 6)[:, 1:3], "x") == (1, 2, 2)                          # (one row: its stride is never used)
    assert a.strided_rows(f(4, 3)[:, 1:2], "x") == (4, 1, 3)                          # one column of a wider buffer
    refused(ValueError, "x", a.strided_rows, f(2, 2).t(), "x")                        # a transposed view
    assert a.strided_rows(f(1, 4).t(), "x") == (4, 1, 1)                              # n x 1: the column stride is never used
    assert a.strided_rows(f(3, 0).t(), "x", min_cols=0) == (0, 3, 3)                  # 0 x c: no row is addressed
    refused(ValueError, "x", a.strided_rows, torch.as_strided(f(4), (2, 2), (1, 1)), "x")          # overlapping rows
    refused(ValueError, "x", a.strided_rows, torch.as_strided(f(4), (2, 2), (0, 1)), "x")
    refused(ValueError, "x", a.strided_rows, f(2, 2, dtype=F64), "x")
    refused(TypeError, "x", T.strided_rows, f(2, 2, dtype=F64), "x")
    assert T.strided_rows(f(2, 2, dtype=F64), "x", F64) == (2, 2, 2)
    refused(ValueError, "x", a.strided_rows, f(4), "x")
    refused(ValueError, "x", a.strided_rows, f(2, 0), "x")                            # min_cols = 1
    refused(ValueError, "x", a.strided_rows, f(2, 3), "x", rows=3)
    refused(ValueError, "x", a.strided_rows, f(2, 3), "x", min_cols=4)
    refused(ValueError, "x", a.strided_rows, f(2, 3), "x", cols=2)
    assert a.strided_rows(f(2, 3), "x", rows=2, cols=3) == (2, 3, 3)
    assert a.rows(f(2, 2).t(), "x") == (2, 2)                                          # (the shape alone: strides are row_stride's)


def test_strided_rows_refuses_a_stride_of_2_to_the_31():
    one = torch.zeros(1, device="meta")          # (one element, no storage behind the view: the checks read metadata only)
    below = torch.as_strided(one, (2, 1), (2 ** 31 - 1, 1))
    assert V.strided_rows(below, "x") == (2, 1, 2 ** 31 - 1)
    at = torch.as_strided(one, (2, 1), (2 ** 31, 1))
    refused(ValueError, "x", V.strided_rows, at, "x")
    refused(ValueError, "x", T.strided_rows, at, "x")
    assert V.strided_rows(torch.as_strided(one, (1, 1), (2 ** 31, 1)), "x") == (1, 1, 1)          # one row: ld is its width


def test_planes_f64():
    N = 5
    dense = lambda p: f(p, N, dtype=F64)
    padded = lambda p, ld=8: f(p, ld, dtype=F64)[:, :N]
    assert V.planes_f64(N, ("a", dense(2), 2), ("b", dense(3), 3)) == N
    assert V.planes_f64(N, ("a", padded(2), 2), ("b", padded(3), 3)) == 8              # views of padded buffers
    refused(ValueError, "a", V.planes_f64, N, ("a", padded(2), 2), ("b", dense(3), 3))          # two different plane strides
    refused(ValueError, "a", V.planes_f64, N, ("a", padded(2, 8), 2), ("b", padded(2, 9), 2))
    assert V.planes_f64(N, ("a", padded(1), 1), ("b", dense(1), 1)) == N              # single planes have no stride to agree on
    assert V.planes_f64(N, ("a", padded(1), 1), ("b", padded(2), 2)) == 8
    assert V.planes_f64(0, ("a", f(2, 0, dtype=F64), 2)) == 1
    refused(ValueError, "b", V.planes_f64, N, ("a", dense(2), 2), ("b", dense(2), 3))
    refused(ValueError, "b", V.planes_f64, N, ("a", dense(2), 2), ("b", f(N, 2, dtype=F64).t(), 2))
    refused(ValueError, "a", V.planes_f64, N, ("a", torch.as_strided(f(8, dtype=F64), (2, N), (3, 1)), 2))          # planes overlap
    refused(TypeError, "b", T.planes_f64, N, ("a", dense(2), 2), ("b", f(2, N), 2))
    refused(ValueError, "b", V.planes_f64, N, ("a", dense(2), 2), ("b", f(2, N), 2))


def test_step_index():
    for a, kind in ((V, ValueError), (T, TypeError)):
        for entries in (1, 2):
            a.step_index(f(entries, dtype=I32), entries=entries)
            a.step_index(f(4, dtype=I32), "window", entries=entries)
            refused(kind, "step", a.step_index, f(2, dtype=I64), entries=entries)                   # wrong dtype
            refused(kind, "step", a.step_index, 3, entries=entries)
            refused(ValueError, "step", a.step_index, f(entries - 1, dtype=I32), entries=entries)   # too few entries
            refused(ValueError, "window", a.step_index, f(4, dtype=I32)[::2], "window", entries=entries)          # strided
            refused(ValueError, "step", a.step_index, f(2, 2, dtype=I32), entries=entries)


def test_lattice():
    buf = f(1)
    V.lattice(0, 5, None, "snap", "snapshot")
    V.lattice(2, 5, buf, "snap", "snapshot")
    refused(ValueError, "snap", V.lattice, 2, 5, None, "snap", "snapshot")
    refused(ValueError, "series", V.lattice, 0, 5, buf, "series", "series")
    refused(ValueError, "every", V.lattice, -1, 5, buf, "snap", "snapshot")
    refused(ValueError, "max_steps", V.lattice, 2, -1, buf, "snap", "snapshot")
    refused(ValueError, "every", V.lattice, -1, -1, None, "snap", "snapshot")          # every is looked at first


def test_scalars():
    np1 = np.int64(1)
    V.integer(0, "n")
    V.integer(-1, "n")
    V.integer(3, "k", at_least=1, at_most=3)
    for v in (True, 1.0, np1):
        refused(ValueError, "n", V.integer, v, "n")
        refused(ValueError, "c", V.column, v, "c", 4)
        refused(ValueError, "p", V.choice, v, "p", (0, 1, 2), "0, 1 or 2")
    refused(ValueError, "n", V.integer, -1, "n", at_least=0)
    refused(ValueError, "k", V.integer, 4, "k", at_least=1, at_most=3)
    V.column(0, "c", 1)
    refused(ValueError, "c", V.column, -1, "c", 4)
    refused(ValueError, "c", V.column, 4, "c", 4)
    V.choice(2, "p", (0, 1, 2), "0, 1 or 2")
    refused(ValueError, "p", V.choice, -1, "p", (0, 1, 2), "0, 1 or 2")
    V.choice(1.0, "s", (0, 1), "0 or 1", integer=False)          # (tracer_advance's scheme: any number that compares equal)
    refused(ValueError, "s", V.choice, True, "s", (0, 1), "0 or 1", integer=False)
    refused(ValueError, "s", V.choice, -1, "s", (0, 1), "0 or 1", integer=False)
    for v in (1, 1.0, -1):
        V.number(v, "mu")
    for v in (True, np1, "1", None):
        refused(ValueError, "mu", V.number, v, "mu")
    V.at_least(0, "m", 0)
    V.at_least(True, "m", 0)          # (for values the wrapper has already passed through int())
    refused(ValueError, "m", V.at_least, -1, "m", 0)


def test_distinct_storage():
    buf = f(8)
    out, other = buf[:4].view(2, 2), buf[4:].view(2, 2)          # two windows of one storage
    refused(ValueError, "out", V.distinct_storage, out, "out", ("a", None), ("gy", other))
    V.distinct_storage(out, "out", ("a", None), ("gy", f(2, 2)))
    empty = f(0, 2)
    V.distinct_storage(empty, "out", ("gy", empty))
    refused(ValueError, "out", V.distinct_storage, empty, "out", ("gy", empty), identity=True)


def test_same_device():
    x = f(2)
    with pytest.raises(ValueError, match="^x: fn: .*no CPU fallback"):
        V.same_device(("x", x), ("y", None))
    meta = torch.empty(2, device="meta")

    class OnDevice:          # (a stand-in with a HIP device: same_device reads `.device` alone)
        device = torch.device("cuda", 0)
    assert V.same_device(("x", OnDevice), ("y", None), ("z", OnDevice)) == torch.device("cuda", 0)
    refused(ValueError, "y", V.same_device, ("x", OnDevice), ("y", meta))


def grid(**kw):
    g = dict(pos_sorted=f(6, 2), order=f(6, dtype=I32), cell_start=f(2 * 3 + 1, dtype=I32), n_cells=[2, 3, 1], org=None, h=0.5, dim=2, n=6)
    g.update(kw)
    return g


def test_cell_grid():
    assert V.cell_grid(grid()) == (2, 6, [2, 3, 1])
    V.cell_start(grid(), [2, 3, 1])
    refused(ValueError, "grid", V.cell_grid, None)
    refused(ValueError, "grid", V.cell_grid, {k: v for k, v in grid().items() if k != "h"})
    refused(ValueError, "grid['pos_sorted']", V.cell_grid, grid(pos_sorted=f(6, 3)))
    refused(ValueError, "grid['pos_sorted']", V.cell_grid, grid(pos_sorted=f(6, 2, dtype=F64)))
    refused(ValueError, "grid['order']", V.cell_grid, grid(order=f(6, dtype=I64)))
    refused(ValueError, "grid['order']", V.cell_grid, grid(order=f(5, dtype=I32)))
    assert V.cell_grid(grid(n_cells=[0, 3]))[2] == [0, 3]          # (what the cells must be is the launch's business)
    refused(ValueError, "grid['cell_start']", V.cell_start, grid(), [2, 3, 2])
    refused(ValueError, "grid['cell_start']", V.cell_start, grid(cell_start=f(7, dtype=I64)), [2, 3, 1])


def test_scratch():
    V.scratch(f(16, dtype=F64), "scratch", 16, "fn_scratch")
    refused(ValueError, "scratch", V.scratch, f(15, dtype=F64), "scratch", 16, "fn_scratch")
    refused(ValueError, "scratch", V.scratch, f(4, 4, dtype=F64), "scratch", 16, "fn_scratch")
    refused(TypeError, "scratch", T.scratch, f(16), "scratch", 16, "fn_scratch")


@pytest.mark.parametrize("n", [0, 1, 256, 257, 262144, 262145])
def test_record_scratch_size_is_the_library_s(n):
    """Both sides of the workgroup count (256 rows) and of the cap of 1024 workgroups — the corners tests/step_sum_ref.py names."""
    lib = _lib.load()          # (needs no GPU)
    for count in (1, 3):
        want = _args.record_scratch_doubles(n, count)
        assert want == 8 + min(max((n + 255) // 256, 1), 1024) * count
        assert lib.g4c_weighted_integrals_scratch_doubles(n, count) == want
        assert lib.g4c_rollout_record_scratch_doubles(n, count) == _args.record_scratch_doubles(n, count * _lib.REC_NSTAT)
        assert lib.g4c_mesh_derived_scratch_doubles(n, count) == _args.record_scratch_doubles(n, count * _lib.DERIVED_NSTAT)
