"""The argument checks of the launch wrappers in ops.py, once: `Args(what, dtype_error)` carries the wrapper's name and the exception
class it raises for a wrong dtype, its methods are the checks.  They read host metadata only (types, shapes, strides, devices) — never
a tensor's values, which would synchronise the stream and break graph capture — and never touch the library, so a malformed call is
refused the same way with or without a device.  Every message starts with the argument's name, then the wrapper's.  DESIGN.md §5
"The wrapper checks" has the conventions."""
from __future__ import annotations

import torch

LD_LIMIT = 2 ** 31          # every *_ld field of include/g4c.h is an int32_t (the two 64-bit `ld` of snapshot_* keep to the one rule)


def record_scratch_doubles(n_nodes: int, count: int) -> int:
    """The doubles of a step-record scratch (csrc/step_record.h: a header of 8 and `count` partial sums per workgroup of 256 rows, at
    most 1024 workgroups), restated from g4c_*_scratch_doubles so that a scratch that is too small is refused before the library is
    loaded.  `count` is what one workgroup leaves: fields x statistics, columns x statistics, or entries."""
    return 8 + min(max(-(-int(n_nodes) // 256), 1), 1024) * int(count)


def _got(t) -> str:
    return str(getattr(t, "dtype", type(t).__name__))


def _layout(t) -> str:
    return f"shape {tuple(t.shape)} strides {tuple(t.stride())}"


class Args:
    __slots__ = ("what", "dtype_error")

    def __init__(self, what: str, dtype_error=ValueError):
        self.what, self.dtype_error = what, dtype_error

    def fail(self, name: str, text: str, kind=ValueError):
        return kind(f"{name}: {self.what}: {text}" if self.what else f"{name}: {text}")

    # ---- tensors (a torch accessor costs about as much as everything else in a check: shape and strides are read once)
    def dtype(self, t, name: str, dtype) -> None:
        """A tensor of `dtype` (one, or a tuple of acceptable ones)."""
        if not isinstance(t, torch.Tensor) or (t.dtype != dtype and not (isinstance(dtype, tuple) and t.dtype in dtype)):
            names = " / ".join(str(d).replace("torch.", "") for d in (dtype if isinstance(dtype, tuple) else (dtype,)))
            raise self.fail(name, f"expected {'an' if names[0] == 'i' else 'a'} {names} tensor, got {_got(t)}", self.dtype_error)

    def tensor(self, t, name: str, dtype, *, dim=None, shape=None) -> None:
        """dtype, contiguity, then the number of dimensions and / or the exact shape (a tuple) of one tensor."""
        self.dtype(t, name, dtype)
        if not t.is_contiguous():
            raise self.fail(name, f"needs a contiguous tensor, got {_layout(t)}")
        if dim is not None and t.dim() != dim:
            raise self.fail(name, f"expected a {dim}-D tensor, got shape {tuple(t.shape)}")
        if shape is not None and t.shape != shape:
            raise self.fail(name, f"expected shape {shape}, got {tuple(t.shape)}")

    def rows(self, t, name: str, dtype=torch.float32, *, rows=None, cols=None, min_cols: int = 1):
        """(n_rows, cols) of a 2-D tensor of `dtype` with exactly `rows` rows (None: any) and exactly `cols` / at least `min_cols`
        columns; its strides are `row_stride`'s business."""
        self.dtype(t, name, dtype)
        shape = t.shape
        if len(shape) != 2 or (rows is not None and shape[0] != rows) or (shape[1] != cols if cols is not None else shape[1] < min_cols):
            raise self.fail(name, f"expected [{'n_rows' if rows is None else rows}, {f'>= {min_cols}' if cols is None else cols}], "
                                  f"got shape {tuple(shape)}")
        return shape[0], shape[1]

    def row_stride(self, t, name: str) -> int:
        """The leading dimension of a 2-D tensor a launch addresses as t[r * ld + c]: unit column stride and rows that do not
        overlap (neither is asked of a tensor without rows, or of its only column / row), ld below 2^31."""
        (n, cols), (s0, s1) = t.shape, t.stride()
        if (n > 0 and cols > 1 and s1 != 1) or (n > 1 and s0 < cols):
            raise self.fail(name, f"needs rows of unit stride, got {_layout(t)}")
        ld = max(s0, cols) if n > 1 else cols
        if ld >= LD_LIMIT:
            raise self.fail(name, f"a row stride of {ld} elements does not fit the descriptor's 32 bits")
        return ld

    def strided_rows(self, t, name: str, dtype=torch.float32, *, rows=None, cols=None, min_cols: int = 1):
        """`rows` then `row_stride`: (n_rows, cols, ld)."""
        n, c = self.rows(t, name, dtype, rows=rows, cols=cols, min_cols=min_cols)
        return n, c, self.row_stride(t, name)

    def step_index(self, t, name: str = "step", entries: int = 1) -> None:
        """The step tensor a launch reads on the device: contiguous int32 [>= entries] — entries = 1: [step index]; 2: [step index,
        the closing launch's ticket counter], or a window {origin, last}."""
        typed = isinstance(t, torch.Tensor) and t.dtype == torch.int32
        if not typed or t.dim() != 1 or t.numel() < entries or not t.is_contiguous():
            text = "whose first entry is the step index" if entries == 1 else "of two entries"
            raise self.fail(name, f"expected a contiguous int32 tensor {text}, got {_layout(t) if typed else _got(t)}",
                            ValueError if typed else self.dtype_error)

    def planes_f64(self, n_nodes: int, *named) -> int:
        """The fp64 accumulators (name, tensor, planes) of a per-node statistic: each float64 [planes, n_nodes] with unit stride along
        the nodes, all with one plane stride >= n_nodes (views of padded buffers are fine), which is returned."""
        lds = set()
        for name, t, planes in named:
            self.dtype(t, name, torch.float64)
            if t.shape != (planes, n_nodes):
                raise self.fail(name, f"expected shape ({planes}, {n_nodes}), got {tuple(t.shape)}")
            plane_ld, node_stride = t.stride()
            if n_nodes > 1 and node_stride != 1:
                raise self.fail(name, f"needs unit stride along the nodes, got strides {tuple(t.stride())}")
            if planes > 1 and n_nodes > 0:
                lds.add(plane_ld)
        if len(lds) > 1 or (lds and min(lds) < n_nodes):
            raise self.fail(named[0][0], f"the accumulators need one common plane stride >= n_nodes = {n_nodes}, got {sorted(lds)}")
        return lds.pop() if lds else max(n_nodes, 1)

    def distinct_storage(self, out, name: str, *named, identity: bool = False) -> None:
        """`out` shares its storage with none of the (name, tensor) it is computed from; `identity`: nor is it one of them, even empty."""
        for other, t in named:
            if t is not None and ((identity and out is t) or (out.numel() and t.numel()
                                                              and out.untyped_storage().data_ptr() == t.untyped_storage().data_ptr())):
                raise self.fail(name, f"{name} shares its storage with {other}")

    def same_device(self, first, *named):
        """Every (name, tensor) on the HIP device of the first one, which is returned (nothing is moved, there is no CPU path)."""
        name0, t0 = first
        if t0.device.type != "cuda":
            raise self.fail(name0, f"runs on a HIP device only, got a tensor on '{t0.device}' (there is no CPU fallback)")
        for name, t in named:
            if t is not None and t.device != t0.device:
                raise self.fail(name, f"on '{t.device}', {name0} is on '{t0.device}'")
        return t0.device

    def scratch(self, t, name: str, need: int, maker: str) -> None:
        """A float64 vector of at least `need` doubles (`maker` names the function that allocates it)."""
        self.tensor(t, name, torch.float64, dim=1)
        if t.numel() < need:
            raise self.fail(name, f"{t.numel()} doubles, needs {need} ({maker})")

    def cell_grid(self, grid):
        """The cell grid of a node cloud (`synthetic._bin_cloud`): its keys and the shapes of pos_sorted and order -> (dim, n, cells).
        What a launch asks of `cells` is its own business; `cell_start` follows once they are known to be [nx, ny, nz], each >= 1."""
        for key in ("pos_sorted", "order", "cell_start", "n_cells", "org", "h", "dim", "n"):
            if not isinstance(grid, dict) or key not in grid:
                raise self.fail("grid", f"expected the cell grid of the node cloud (synthetic._bin_cloud), got {type(grid).__name__}"
                                        f"{'' if not isinstance(grid, dict) else f' without {key!r}'}")
        dim, n = int(grid["dim"]), int(grid["n"])
        self.tensor(grid["pos_sorted"], "grid['pos_sorted']", torch.float32, shape=(n, dim))
        self.tensor(grid["order"], "grid['order']", torch.int32, shape=(n,))
        return dim, n, [int(c) for c in grid["n_cells"]]

    def cell_start(self, grid, cells) -> None:
        self.tensor(grid["cell_start"], "grid['cell_start']", torch.int32, shape=(cells[0] * cells[1] * cells[2] + 1,))

    # ---- scalars (a bool is not an integer here, nor is a numpy scalar: the values go into ctypes fields as they are)
    def at_least(self, v, name: str, k: int) -> None:
        if v < k:
            raise self.fail(name, f"{v} (>= {k})")

    def integer(self, v, name: str, at_least=None, at_most=None) -> None:
        if isinstance(v, bool) or not isinstance(v, int) or (at_least is not None and v < at_least) or (at_most is not None and v > at_most):
            bounds = "" if at_least is None else f" >= {at_least}" if at_most is None else f" {at_least} .. {at_most}"
            raise self.fail(name, f"expected an integer{bounds}, got {v!r}")

    def number(self, v, name: str) -> None:
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise self.fail(name, f"expected a number, got {v!r}")

    def choice(self, v, name: str, options, text: str, integer: bool = True) -> None:
        """One of `options`; `integer`: as an int (False: any number that compares equal, but no bool)."""
        if isinstance(v, bool) or (integer and not isinstance(v, int)) or v not in options:
            raise self.fail(name, f"expected {text}, got {v!r}")

    def column(self, v, name: str, width: int) -> None:
        if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v < width:
            raise self.fail(name, f"expected a column 0 .. {width - 1}, got {v!r}")

    def lattice(self, every: int, max_steps: int, buf, name: str, noun: str) -> None:
        """The slots of a record kept every `every`-th step: every >= 0 and max_steps >= 0, and the buffer `name` given exactly when
        every > 0."""
        if every < 0:
            raise self.fail("every", f"{every} (0 keeps no {noun}, k > 0 every k-th step)")
        self.at_least(max_steps, "max_steps", 0)
        if (every > 0) != (buf is not None):
            raise self.fail(name, f"every = {every} {'needs a' if every else 'takes no'} {noun} buffer")
