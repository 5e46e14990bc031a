"""Control volumes of the nodes of a 2-D mesh (new functionality — the reference has none): the areas that turn a sum over node rows
into an integral over the domain.

A kNN cloud has no cells, so they are built: node i gets the polygon  (its Voronoi cell within its graph's cloud) ∩ (a clipping `box`) ∩
(for a wall node, the half-plane {x : (x − pos_i)·n_i >= 0} of its outward normal n_i — `gfd.BodyForces.unit` points out of the body into
the fluid —, so that the cell does not reach into the body).  One launch per graph (`g4c_voronoi_cells`, csrc/control_volumes.hip): one
thread per node walks the rings of the cloud's cell grid and clips by the bisector with every point it meets until no unseen point
can cut the polygon, in fp64 on the fp32 positions — exact for any cloud and any density, no fixed k.  Built once per mesh.

`integrate(x, entries)` is the standalone form of the rollout's per-step launch (`g4c_weighted_integrals`): fp64 sums of
area · z[a] · z[b] in a fixed order.  The wall half-plane is tangent: round a convex body it leaves slivers between tangent and wall,
so Σ area falls short of (box − bodies) by a little (tests/VOLUMES_MEASURED.md has the closure).

The integrals are differentiable in x (the areas are constants of the mesh): `adjoint(g, x, entries)` is the transpose of `integrate`
at x (`g4c_weighted_integrals_adjoint`: one launch, fp64 in a pinned order), `integrate` of a tensor that requires a gradient is
recorded for autograd, and `integrate(..., per_graph=True)` keeps the graphs of a collated batch apart — what `gfd.nn.IntegralLoss`
trains against.  2-D only; periodic axes and 3-D cells are out of scope."""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib, ops
from .body_forces import BodyForces

GRID_K = 6                  # the cell grid is the one of a k = 6 neighbour search: about four nodes a cell


def _counts(graph, n: int):
    batch = getattr(graph, "batch", None)
    if batch is None:
        return [n]
    if not torch.is_tensor(batch) or batch.numel() != n or batch.dtype.is_floating_point:
        raise ValueError(f"graph: graph.batch names {getattr(batch, 'numel', lambda: 0)()} nodes, graph.pos has {n}")
    return [n] if n == 0 else torch.bincount(batch.reshape(-1)).tolist()


def check_volumes(graph, box=None, bodies=None, normals=None) -> dict:
    """The arguments of `ControlVolumes` on the tensors as they were passed (nothing is moved, the library is not touched): ValueError /
    TypeError naming the argument, or a description: n_nodes, counts (nodes per graph of the batch), boxes (None: each graph's bounding
    box), bodies (a BodyForces, True or None), normals."""
    pos = getattr(graph, "pos", None)
    if not torch.is_tensor(pos) or pos.dim() != 2 or not pos.dtype.is_floating_point:
        raise ValueError("graph: ControlVolumes needs graph.pos [N, 2]")
    if int(pos.size(1)) != 2:
        raise ValueError(f"graph: ControlVolumes is 2-D only, graph.pos is {tuple(pos.shape)} (3-D cells are out of scope)")
    n = int(pos.size(0))
    if n < 1:
        raise ValueError("graph: ControlVolumes of an empty point cloud")
    counts = _counts(graph, n)
    if min(counts) < 1:
        raise ValueError(f"graph: graph.batch leaves a graph of the batch without nodes (counts {counts})")
    boxes = None
    if box is not None:
        if torch.is_tensor(box) and box.dim() == 2 or (isinstance(box, (list, tuple)) and len(box) and isinstance(box[0], (list, tuple))):
            rows = box.tolist() if torch.is_tensor(box) else list(box)
            if len(rows) != len(counts):
                raise ValueError(f"box: {len(rows)} boxes for a batch of {len(counts)} graphs")
            boxes = [ops._box_arg("ControlVolumes", r) for r in rows]
        else:
            boxes = [ops._box_arg("ControlVolumes", box)] * len(counts)
    if bodies is not None and bodies is not True and not isinstance(bodies, BodyForces):
        raise TypeError(f"bodies: expected a gfd.BodyForces of this graph, True (build one with its defaults) or None, got {type(bodies).__name__}")
    if isinstance(bodies, BodyForces) and bodies.n_nodes != n:
        raise ValueError(f"bodies: a BodyForces over {bodies.n_nodes} nodes for a graph of {n}")
    if normals is not None:
        if bodies is not None:
            raise ValueError("normals: given together with bodies= (the bodies carry their own)")
        if not torch.is_tensor(normals) or not normals.dtype.is_floating_point or tuple(normals.shape) != (n, 2):
            raise ValueError(f"normals: expected a floating-point tensor [{n}, 2] (zero rows: no wall), got "
                             f"{getattr(normals, 'dtype', type(normals).__name__)} {tuple(getattr(normals, 'shape', ()))}")
        if normals.device != pos.device:
            raise ValueError(f"normals: on '{normals.device}', graph.pos is on '{pos.device}'")
        if not bool(torch.isfinite(normals).all()):
            raise ValueError("normals: a normal that is not finite")
    return dict(n_nodes=n, counts=counts, boxes=boxes, bodies=bodies, normals=normals)


class ControlVolumes:
    """The control volumes of the nodes of `graph` (a 2-D Graph on the GPU), built once per mesh.

    `box` = (lo_x, lo_y, hi_x, hi_y): what the outermost cells are clipped to; None: the bounding box of the (fp32) cloud.  A box far
    larger than the cloud makes the hull nodes scan the whole grid (`rings` shows it).  `bodies`: a `gfd.BodyForces` of this graph (or
    True: one built with its defaults, from `graph.bound == 4`): its `items` and `unit` become the wall half-planes.  `normals` [N, 2]
    gives them directly; zero rows mean none.  With `graph.batch` every graph of the batch is one construction with its own box (graphs
    of a batch overlap in space, as in `MeshJet`); `box` may then be one box for all or a list of one per graph.

    `area` float64 [N], `centroid` float64 [N, 2], `nvert` int32 [N], `flags` uint8 [N] (bits `BOX`: the box cut the cell, `WALL`,
    `DUPLICATE`: another node at the same position — the pair shares one cell, each gets all of it —, `OVERFLOW`: more than
    `_lib.VORONOI_MAX_VERTS` vertices, area +0), `rings` int32 [N], `degenerate` bool [N] (area == 0), `total` (Σ area, a float),
    `box` float64 [graphs, 4], `counts` (the nodes of every graph, a list), `group` int32 [N] (the graph of every node).
    `integrate(x, entries)` [ne] float64: Σ_i area_i · x[i, a] · x[i, b] per entry (a, b), −1 for 1 (`per_graph=True`: [graphs, ne]);
    `adjoint(g, x, entries)` its transpose; `weights(dtype)` the areas for `Modes(node_weights=)`."""

    BOX, WALL, DUPLICATE, OVERFLOW = _lib.VORONOI_BOX, _lib.VORONOI_WALL, _lib.VORONOI_DUPLICATE, _lib.VORONOI_OVERFLOW

    def __init__(self, graph, box=None, bodies=None, normals=None):
        spec = check_volumes(graph, box, bodies, normals)
        pos = graph.pos
        dev = pos.device
        if dev.type != "cuda":
            raise ValueError(f"graph: ControlVolumes runs on a HIP device only, graph.pos is on '{dev}' (there is no CPU fallback)")
        n = self.n_nodes = spec["n_nodes"]
        if bodies is True:
            bodies = BodyForces(graph)
        if bodies is not None:
            normals = torch.zeros((n, 2), dtype=torch.float64, device=dev)
            normals[bodies.items] = bodies.unit
        elif normals is not None:
            normals = normals.detach().to(torch.float64)
        self.bodies = bodies
        from .synthetic import _bin_cloud
        p32 = pos.detach().to(torch.float32)
        self.area = torch.zeros(n, dtype=torch.float64, device=dev)
        self.centroid = torch.zeros((n, 2), dtype=torch.float64, device=dev)
        self.nvert = torch.zeros(n, dtype=torch.int32, device=dev)
        self.flags = torch.zeros(n, dtype=torch.uint8, device=dev)
        self.rings = torch.zeros(n, dtype=torch.int32, device=dev)
        boxes, a = [], 0
        for b, c in enumerate(spec["counts"]):          # (contiguous ranges: `collate` numbers the nodes graph after graph)
            own = p32[a:a + c].contiguous()
            grid = _bin_cloud(own, GRID_K, "ControlVolumes (g4c_voronoi_cells)")
            if spec["boxes"] is None:
                bx = [float(v) for v in grid["lo"].tolist()] + [float(v) for v in own.max(0)[0].double().tolist()]
                for ax in range(2):          # a cloud without extent along an axis has no bounding box to clip to
                    if not bx[ax] < bx[2 + ax]:
                        raise ValueError(f"box: the cloud{'' if len(spec['counts']) == 1 else f' of graph {b}'} has no extent along axis {ax}: "
                                         f"pass box=")
            else:
                bx = spec["boxes"][b]
            out = (self.area[a:a + c], self.centroid[a:a + c], self.nvert[a:a + c], self.flags[a:a + c], self.rings[a:a + c])
            ops.voronoi_cells(grid, bx, None if normals is None else normals[a:a + c].contiguous(), out=out)
            boxes.append(bx)
            a += c
        self.box = torch.tensor(boxes, dtype=torch.float64)
        self.degenerate = self.area == 0
        self.total = float(self.area.sum())
        self.counts = [int(c) for c in spec["counts"]]
        self.group = torch.repeat_interleave(torch.arange(len(self.counts), dtype=torch.int32, device=dev),
                                             torch.tensor(self.counts, device=dev), output_size=n)

    def weights(self, dtype=torch.float64) -> torch.Tensor:
        """The areas [N] as `dtype`: the `node_weights` of `gfd.Modes`."""
        return self.area.to(dtype)

    def integrate(self, x: torch.Tensor, entries, *, sub: Optional[torch.Tensor] = None, nz: Optional[int] = None, x_step: int = 0,
                  sub_step: int = 0, t: int = 0, weights: Optional[torch.Tensor] = None, per_graph: bool = False) -> torch.Tensor:
        """[ne] float64: Σ_i area_i · z_i[a] · z_i[b] for every entry (a, b) of `entries` (a column of −1 stands for 1), z the rows of
        x float32 [N, >= nz] — or of x − sub, formed in fp64.  With x_step = nf, x holds every step (a target) and `t` names the step.
        The standalone form of the rollout's launch (`ops.weighted_integrals`): the same order, the same bits.

        `per_graph=True`: [G, ne], row q the integrals over graph q of the batch alone — one launch over its (contiguous) row range,
        bit for bit what a `ControlVolumes` of that graph returns.  When gradients are enabled and x requires one, the call is
        recorded (`autograd._WeightedIntegrals`: the same launches on x.detach(), the same bits; `adjoint` in the backward, which
        keeps x and `sub` — the map is quadratic); a `sub` that requires a gradient is a ValueError: subtract it in torch instead."""
        prog = ops.integral_program(entries, nz)
        self._check_x(x, t)
        if not isinstance(per_graph, bool):
            raise ValueError(f"per_graph: expected a bool, got {per_graph!r}")
        if torch.is_tensor(sub) and sub.requires_grad and torch.is_grad_enabled():
            raise ValueError("sub: a `sub` that requires a gradient is not differentiated through: pass x − sub as x, or detach it")
        if torch.is_grad_enabled() and x.requires_grad:
            from . import autograd
            return autograd.weighted_integrals(self, x, prog, sub, nz, x_step, sub_step, t, weights, per_graph)
        return self._integrate(x, prog, sub, nz, x_step, sub_step, t, weights, per_graph)

    def _check_x(self, x, t):
        if not torch.is_tensor(x) or x.dim() != 2 or int(x.size(0)) != self.n_nodes:
            raise ValueError(f"x: expected a float32 tensor [{self.n_nodes}, >= 1], got {getattr(x, 'dtype', type(x).__name__)} "
                             f"{tuple(getattr(x, 'shape', ()))}")
        if isinstance(t, bool) or not isinstance(t, int) or t < 0:
            raise ValueError(f"t: expected a step index >= 0, got {t!r}")

    def _integrate(self, x, prog, sub, nz, x_step, sub_step, t, weights, per_graph):
        dev = self.area.device
        w = self.area if weights is None else weights
        ne = int(prog.ne)
        if not per_graph:
            stats = torch.zeros((t + 1, ne), dtype=torch.float64, device=dev)
            scratch = ops.weighted_integrals_scratch(self.n_nodes, ne, dev)
            ops.weighted_integrals(x, w, prog, stats, scratch, nz=nz, sub=sub, x_step=x_step, sub_step=sub_step, t=t)
            return stats[t]
        if not torch.is_tensor(w) or w.dim() != 1 or int(w.size(0)) != self.n_nodes:
            raise ValueError(f"weights: expected a float64 tensor [{self.n_nodes}], got {tuple(getattr(w, 'shape', ()))}")
        if torch.is_tensor(sub) and (sub.dim() != 2 or int(sub.size(0)) != self.n_nodes):
            raise ValueError(f"sub: expected a float32 tensor [{self.n_nodes}, >= 1], got {tuple(sub.shape)}")
        stats = torch.zeros((len(self.counts), t + 1, ne), dtype=torch.float64, device=dev)
        scratch = ops.weighted_integrals_scratch(max(self.counts), ne, dev)          # (the launches follow each other on one stream)
        a = 0
        for q, c in enumerate(self.counts):          # (contiguous ranges: `collate` numbers the nodes graph after graph)
            ops.weighted_integrals(x[a:a + c], w[a:a + c], prog, stats[q], scratch, nz=nz, sub=None if sub is None else sub[a:a + c],
                                   x_step=x_step, sub_step=sub_step, t=t)
            a += c
        return stats[:, t]

    def adjoint(self, g: torch.Tensor, x: torch.Tensor, entries, *, sub: Optional[torch.Tensor] = None, nz: Optional[int] = None,
                x_step: int = 0, sub_step: int = 0, t: int = 0, per_graph: bool = False,
                weights: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The transpose of `integrate` at x: gx float32 [N, nz] = the derivative of Σ g · integrate(x, entries, ...) by the sample's
        columns (x's columns x_step · t .. + nz), for g float64 [ne] — or [G, ne] with `per_graph=True`.  One launch
        (`ops.weighted_integrals_adjoint`), fp64 in a fixed order, no atomics: the same bits on every run."""
        prog = ops.integral_program(entries, nz)
        self._check_x(x, t)
        ne, groups = int(prog.ne), (len(self.counts) if per_graph else 1)
        if not torch.is_tensor(g) or g.dtype != torch.float64 or tuple(g.shape) != ((groups, ne) if per_graph else (ne,)):
            raise ValueError(f"g: expected a float64 tensor {[groups, ne] if per_graph else [ne]}, got "
                             f"{getattr(g, 'dtype', type(g).__name__)} {tuple(getattr(g, 'shape', ()))}")
        return ops.weighted_integrals_adjoint(x.detach(), self.area if weights is None else weights, prog,
                                              g.detach().reshape(groups, ne).contiguous(), nz=nz, sub=None if sub is None else sub.detach(),
                                              x_step=x_step, sub_step=sub_step, t=t, group=self.group if per_graph else None)

    def __repr__(self):
        return f"ControlVolumes(nodes={self.n_nodes}, graphs={int(self.box.size(0))}, total={self.total:.6g})"
