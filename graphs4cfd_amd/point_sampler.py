"""Values of node fields at points that are no nodes (new functionality — the reference interpolates on the host, through matplotlib
triangulations, in its plot.py): a wake profile along a line, a PIV window, a hot-wire at a coordinate, the raster of a picture.

At point q with its k nearest nodes j = 0 .. k − 1 (nearest first, `knn_query_device` over `graph.pos`; d_j = pos[j] − q), the sample of
a field x is the value at q of the plane fitted to the neighbours' values by weighted least squares, w_j = |d_j|^(−power) — a
moving-least-squares fit with a linear basis:  x(q) = Σ_j c_j x[j]  with  c_j = w_j (1/W − e_jᵀ M⁻¹ d̄),  W = Σ w_j,  d̄ = Σ w_j d_j / W,
e_j = d_j − d̄,  M = Σ w_j e_j e_jᵀ  — exact on constants and on linear fields, whatever the weights, inside the cloud and outside it.
The coefficients are built once per set of points on the device in fp64 (`g4c_sample_weights`, csrc/point_sample.hip) and kept as
fp32; every application is one memory-bound launch (`g4c_sample_points`): one thread per point and chunk of columns, fp32, the
neighbours nearest first, so the bits are a function of the data alone.  A point on a node (distance 0) takes that node's row, bit for
bit.  A point whose neighbours do not span the space (k <= dim, collinear / coplanar neighbours) is `degenerate`: it gets Shepard's
c_j = w_j / W, exact on constants only."""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch

from . import _lib, ops, plan

MAX_K = _lib.SAMPLE_MAX_K
DEFAULT_K = {2: 6, 3: 10}


def _integer(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool)


def _graph_dim(graph) -> int:
    pos = getattr(graph, "pos", None)
    if not torch.is_tensor(pos) or pos.dim() != 2 or int(pos.size(1)) not in (2, 3) or not pos.dtype.is_floating_point:
        raise ValueError("graph: PointSampler needs graph.pos, a floating-point tensor [N, 2] or [N, 3]")
    return int(pos.size(1))


def _coords(name: str, v, dim: int) -> Tuple[float, ...]:
    """`dim` finite numbers (a sequence or a 1-D tensor) -> a tuple of floats; ValueError naming the argument."""
    try:
        vals = [float(c) for c in (v.tolist() if torch.is_tensor(v) else v)]
    except (TypeError, ValueError):
        raise ValueError(f"{name}: expected {dim} coordinates, got {v!r}") from None
    if len(vals) != dim or not all(c == c and abs(c) != float("inf") for c in vals):
        raise ValueError(f"{name}: expected {dim} finite coordinates, got {v!r}")
    return tuple(vals)


def check_points(graph, points, k, power) -> Tuple[int, int]:
    """The arguments of `PointSampler` on the tensors as they were passed (nothing is moved, the library is not touched): (the
    mesh's dimension, k), or ValueError naming the argument."""
    dim = _graph_dim(graph)
    n = int(graph.pos.size(0))
    if isinstance(power, bool) or not isinstance(power, int) or power not in (0, 1, 2):
        raise ValueError(f"power: expected 0, 1 or 2 (a neighbour weighs |d|^-power), got {power!r}")
    if k is None:
        k = DEFAULT_K[dim]
    if not _integer(k) or not 1 <= k <= MAX_K:
        raise ValueError(f"k: expected an integer 1 <= k <= {MAX_K} (the neighbour search's limit), got {k!r}")
    if k > n:
        raise ValueError(f"k: {k} neighbours of a graph of {n} nodes")
    if not torch.is_tensor(points) or not points.dtype.is_floating_point:
        raise ValueError(f"points: expected a floating-point tensor [P, {dim}], got {getattr(points, 'dtype', type(points).__name__)}")
    if points.dim() != 2 or int(points.size(1)) != dim:
        raise ValueError(f"points: expected [P, {dim}] (the mesh has {dim} dimensions), got {tuple(points.shape)}")
    if points.device.type == "cpu" and not bool(torch.isfinite(points).all()):
        raise ValueError("points: a coordinate that is not finite")
    return dim, int(k)


class PointSampler:
    """The interpolation of node fields of `graph` (a Graph on the GPU with `pos` [N, dim]) to `points` [P, dim] (a floating-point
    tensor, host or device), built once: `k` nearest nodes per point (default 6 in 2-D, 10 in 3-D; 1 <= k <= 16 and k <= N), `power`
    0, 1 or 2 weighs a neighbour by |d|^(−power).

    `sample(x)` [P, F]: the values of x [N, F] (float32, on the device, rows of unit stride — a column slice of a wider tensor will
    do) at the points; `idx`, `coef` [P, k]: the neighbours (the caller's node rows, nearest first) and their coefficients;
    `distance` [P]: the distance to the nearest node — the search knows no boundary, so a point inside a body or outside the domain
    is sampled from the nodes nearest to it: mask by `distance`; `degenerate` bool [P]: the points whose neighbours do not span the
    space (Shepard's weights there: exact on constants only).  `PointSampler.line` and `PointSampler.grid` build rakes and rasters.

    `period` (one entry per axis: None, a length >= the mesh's extent, or "auto", the extent; as `connect_knn`'s): the search and the
    fit run in the wrapped metric (`knn_query_device(period=)`, `g4c_sample_weights_periodic`) — a point next to the seam is fitted
    from both sides of it, `distance` is the wrapped distance, and a point may lie periods away (wrapped exactly as far as fp32
    resolves (point − origin) / period).  Finite points are the caller's to provide: a device coordinate that is not finite is
    searched from the origin along a periodic axis; along another axis the point has no neighbours — its row names node 0 and its
    coefficients are NaN.  `sampler.period` keeps (origin, lengths): the mesh's minimum and the fp32 periods, 0 for an axis that is
    not periodic.  All None: the plain search.

    `sample` of an x that requires grad is recorded for autograd: its backward is `adjoint(gy)` [N, F], the transpose of the same
    linear map (`g4c_sample_points_adjoint`; the coefficients are constants: no gradient reaches the points or the mesh).  The
    node-side tables the adjoint walks are built on its first use.  `PointSampler.from_tables` takes tables fitted elsewhere."""

    def __init__(self, graph, points: torch.Tensor, k: Optional[int] = None, power: int = 2, period=None):
        self.dim, self.k = check_points(graph, points, k, power)
        from .synthetic import check_period, knn_query_device, periodic_frame
        per = check_period(period, self.dim, "PointSampler")
        pos = graph.pos
        if pos.device.type != "cuda":
            raise ValueError(f"graph: PointSampler runs on a HIP device only, graph.pos is on '{pos.device}' (there is no CPU fallback)")
        self.power, self.n_nodes, self.shape = power, int(pos.size(0)), None
        dev = pos.device
        pos32 = pos.detach().to(torch.float32).contiguous()
        self.points = points.detach().to(dev, torch.float32).contiguous()
        n_points = int(self.points.size(0))
        # (origin, lengths) of the periodic frame — the cloud's minimum and the fp32 periods, 0 a non-periodic axis — or None
        self.period = None if per is None else periodic_frame(pos32, per, "PointSampler")
        wrapped = {} if self.period is None else dict(origin=self.period[0], period=self.period[1])
        if n_points:
            nearest = knn_query_device(pos32, self.points, self.k,                          # [P, k] int64, nearest first
                                       period=None if per is None else [L or None for L in self.period[1]])
            if per is not None:          # (a point that is not finite along a non-periodic axis has the row −1: it never forms an address)
                nearest = nearest.clamp_(min=0)
            self._idx = nearest.t().to(torch.int32).contiguous()                            # j-major: lane p reads consecutive entries
        else:
            self._idx = torch.empty((self.k, 0), dtype=torch.int32, device=dev)
        self._coef, self.distance, degenerate = ops.sample_weights(pos32, self.points, self._idx, power, **wrapped)
        self.degenerate = degenerate.bool()
        self._adjoint_tables = None

    @classmethod
    def from_tables(cls, idx: torch.Tensor, coef: torch.Tensor, n_nodes: int, points: Optional[torch.Tensor] = None,
                    distance: Optional[torch.Tensor] = None, degenerate: Optional[torch.Tensor] = None) -> "PointSampler":
        """A sampler from given tables, without a search: `idx` int32 and `coef` float32, both j-major [k, P] (neighbour j of point
        p in row j; `sampler.idx.t()` of another sampler), contiguous and on the HIP device, over `n_nodes` node rows — the
        concatenation of the samplers of a batch's graphs, or a fit computed elsewhere.  Every idx must be a row 0 .. n_nodes − 1:
        the values are not read here.  `points` [P, dim], `distance` [P] and `degenerate` bool [P] are kept as given (None: the
        attribute is None, and `dim`, `power` are None)."""
        if isinstance(n_nodes, bool) or not isinstance(n_nodes, int) or n_nodes < 0:
            raise ValueError(f"n_nodes: expected a number of nodes >= 0, got {n_nodes!r}")
        k, n_points = ops._sample_tables(ops.Args("PointSampler.from_tables"), idx, coef)
        if idx.device.type != "cuda" or coef.device != idx.device:
            raise ValueError(f"idx: PointSampler runs on a HIP device only, idx is on '{idx.device}' and coef on '{coef.device}' "
                             "(there is no CPU fallback)")
        if n_points and k > n_nodes:
            raise ValueError(f"idx: {k} neighbours of {n_nodes} nodes")
        if points is not None and (not torch.is_tensor(points) or points.dim() != 2 or int(points.size(0)) != n_points):
            raise ValueError(f"points: expected a tensor [{n_points}, dim], got {tuple(getattr(points, 'shape', ()))}")
        for name, t in (("distance", distance), ("degenerate", degenerate)):
            if t is not None and (not torch.is_tensor(t) or tuple(t.shape) != (n_points,)):
                raise ValueError(f"{name}: expected a tensor [{n_points}], got {tuple(getattr(t, 'shape', ()))}")
        s = cls.__new__(cls)
        s.dim = None if points is None else int(points.size(1))
        s.k, s.power, s.n_nodes, s.shape, s.period = k, None, n_nodes, None, None
        s.points = None if points is None else points.detach().to(idx.device, torch.float32).contiguous()
        s._idx, s._coef = idx, coef.detach()
        s.distance = None if distance is None else distance.detach().to(idx.device, torch.float32)
        s.degenerate = None if degenerate is None else degenerate.detach().to(idx.device).bool()
        s._adjoint_tables = None
        return s

    @classmethod
    def line(cls, graph, a: Sequence[float], b: Sequence[float], n: int, **kw) -> "PointSampler":
        """A rake: `n` >= 2 points from `a` to `b`, both included, equally spaced (formed in fp64)."""
        dim = _graph_dim(graph)
        a, b = _coords("a", a, dim), _coords("b", b, dim)
        if not _integer(n) or n < 2:
            raise ValueError(f"n: expected an integer >= 2 (the points a and b included), got {n!r}")
        t = torch.arange(n, dtype=torch.float64) / (n - 1)
        a64, b64 = torch.tensor(a, dtype=torch.float64), torch.tensor(b, dtype=torch.float64)
        return cls(graph, (a64 + t[:, None] * (b64 - a64)).to(torch.float32), **kw)

    @classmethod
    def grid(cls, graph, shape: Sequence[int], box=None, **kw) -> "PointSampler":
        """A raster: `shape` = (n_x, n_y[, n_z]) points along the axes, equally spaced from corner to corner of `box` = (lo, hi), both
        included (an axis of one point sits at the middle); `box` defaults to the bounding box of `graph.pos`.  The points are in C
        order of `shape` — the last axis runs fastest —, so `sample(x).view(*s.shape, F)[i, j]` is the value at (x_i, y_j); `s.shape`
        keeps the shape."""
        dim = _graph_dim(graph)
        try:
            shape = tuple(shape)
        except TypeError:
            raise ValueError(f"shape: expected {dim} integers >= 1, got {shape!r}") from None
        if len(shape) != dim or not all(_integer(s) and s >= 1 for s in shape):
            raise ValueError(f"shape: expected {dim} integers >= 1 (points along each axis), got {shape!r}")
        if box is None:
            if int(graph.pos.size(0)) < 1:
                raise ValueError("box: a graph without nodes has no bounding box")
            p = graph.pos.detach()
            lo, hi = _coords("box", p.min(0).values.double().cpu(), dim), _coords("box", p.max(0).values.double().cpu(), dim)
        else:
            try:
                lo, hi = box
            except (TypeError, ValueError):
                raise ValueError(f"box: expected (lo, hi), two corners of {dim} coordinates, got {box!r}") from None
            lo, hi = _coords("box", lo, dim), _coords("box", hi, dim)
        axes = [l + (h - l) * (torch.arange(s, dtype=torch.float64) / (s - 1)) if s > 1 else torch.tensor([0.5 * (l + h)], dtype=torch.float64)
                for l, h, s in zip(lo, hi, shape)]
        pts = torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1).reshape(-1, dim)
        s = cls(graph, pts.to(torch.float32), **kw)
        s.shape = shape
        return s

    @property
    def n_points(self) -> int:
        return int(self._idx.size(1))

    @property
    def idx(self) -> torch.Tensor:
        """[P, k] int32: the neighbours' node rows, nearest first (a view of the j-major table)."""
        return self._idx.t()

    @property
    def coef(self) -> torch.Tensor:
        """[P, k] float32: their coefficients (a view of the j-major table)."""
        return self._coef.t()

    def sample(self, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """[P, F]: x [N, F] (float32, on the device, rows of unit stride, any leading dimension) at the points — one launch.  Of an x
        that requires grad (with grad enabled) the result carries a `grad_fn` whose backward is `adjoint`; `out=` is then refused."""
        if not torch.is_tensor(x) or x.dtype != torch.float32 or x.dim() != 2 or int(x.size(0)) != self.n_nodes or int(x.size(1)) < 1:
            raise ValueError(f"x: expected a float32 tensor [{self.n_nodes}, F], got {getattr(x, 'dtype', type(x).__name__)} "
                             f"{tuple(getattr(x, 'shape', ()))}")
        if torch.is_grad_enabled() and x.requires_grad:
            if out is not None:
                raise NotImplementedError("PointSampler.sample(out=...) is an inference-only path (the input requires grad)")
            from . import autograd as _ag
            return _ag.sample_points(self, x)
        return ops.sample_points(x, self._idx, self._coef, out)

    def _node_side(self):
        """(in_off, in_pt, in_coef): the entries of the j-major tables grouped by the node they name, ascending flat position j·P + p
        within a node — the offsets of that grouping, and the points (position mod P) and coefficients copied into its order.  Built
        on the first adjoint and kept: the plain forward pays nothing."""
        if self._adjoint_tables is None:
            n_entries = self.k * self.n_points
            if n_entries > 2 ** 31 - 1:
                raise NotImplementedError(f"PointSampler.adjoint: k·P = {self.k} · {self.n_points} table entries do not fit the int32 offsets")
            flat = self._idx.reshape(-1)
            if n_entries == 0:          # (no points: every list is empty)
                dev = flat.device
                self._adjoint_tables = (torch.zeros(self.n_nodes + 1, dtype=torch.int32, device=dev), flat,
                                        torch.empty(0, dtype=torch.float32, device=dev))
                return self._adjoint_tables
            csr = plan.gather_csr(flat, self.n_nodes)
            if csr.perm is not None:
                perm = csr.perm.to(torch.int64)
                in_pt = (csr.perm % self.n_points).to(torch.int32).contiguous()
                in_coef = self._coef.reshape(-1).index_select(0, perm).contiguous()
            else:          # (None: the entries are grouped already)
                in_pt = (torch.arange(n_entries, dtype=torch.int32, device=flat.device) % self.n_points).contiguous()
                in_coef = self._coef.reshape(-1).contiguous()
            self._adjoint_tables = (csr.off, in_pt, in_coef)
        return self._adjoint_tables

    def _adjoint(self, gy: torch.Tensor) -> torch.Tensor:
        in_off, in_pt, in_coef = self._node_side()
        return ops.sample_points_adjoint(gy, in_off, in_pt, in_coef, self.n_nodes)

    def adjoint(self, gy: torch.Tensor) -> torch.Tensor:
        """[N, F]: the transpose of `sample`, applied to gy [P, F] (float32; made dense first) — for all x and gy, ⟨sample(x), gy⟩ =
        ⟨x, adjoint(gy)⟩ up to rounding.  One launch (`g4c_sample_points_adjoint`): a gather over the table entries that name a node,
        in a fixed order, no atomics.  A node no point uses gets zeros."""
        if not torch.is_tensor(gy) or gy.dtype != torch.float32 or gy.dim() != 2 or int(gy.size(0)) != self.n_points or int(gy.size(1)) < 1:
            raise ValueError(f"gy: expected a float32 tensor [{self.n_points}, F], got {getattr(gy, 'dtype', type(gy).__name__)} "
                             f"{tuple(getattr(gy, 'shape', ()))}")
        if gy.device != self._idx.device:
            raise ValueError(f"gy: on '{gy.device}', the sampler is on '{self._idx.device}' (there is no CPU fallback)")
        return self._adjoint(gy.detach().contiguous())

    def __repr__(self):
        return (f"PointSampler(points={self.n_points}, nodes={self.n_nodes}, dim={self.dim}, k={self.k}, power={self.power}"
                f"{'' if self.shape is None else f', shape={self.shape}'})")
