"""The force a 2-D flow exerts on the bodies it passes (new functionality — the reference has none): drag, lift and moment from the
pressure and the viscous stress at the wall nodes, and the pressure and wall-shear distribution round the surface.

A body's wall is a closed polygon through its wall nodes (`graph.bound == 4`, the reference's wall code), counter-clockwise.  Wall
item w with predecessor a and successor b carries the area vector  area[w] = ½ (y_b − y_a, −(x_b − x_a))  — the trapezoid rule lumped
at the node: it points out of the body into the fluid; every operation is exact in fp64 for fp32 coordinates whose exponents lie
within 29 binades of each other, and the areas of a loop then sum to exactly zero —, ds = |area[w]|, the unit normal unit[w] = area[w] / ds and the arm[w] = pos − centre.  With the pressure P and the
stress s = mu (∇u + ∇uᵀ) at the node — the velocity gradient is `gfd.MeshGradient`'s —, the pressure force is Σ −P area, the viscous
force Σ s · area, the moments Σ arm × traction.  One launch (`g4c_body_forces`, csrc/body_forces.hip) forms them: one workgroup per
body, fp64 sums in a fixed order, so the bits are a function of the data alone.  The geometry is built once per mesh, in fp64.

The map from the fields to the loads is affine with constant geometry; `BodyForces.adjoint` applies the transpose of its linear part
(`g4c_body_forces_adjoint`), and `forces` / `wall` of a tensor that requires grad are recorded for autograd with it as their backward
(`gfd.nn.ForceLoss` trains against drag, lift and the wall loads)."""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib, ops, plan
from .mesh_gradient import MeshGradient, check_mesh

WALL = 4                    # the reference's code of a wall node in graph.bound


def _integer(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool)


def _number(v) -> bool:
    return isinstance(v, (int, float)) and not isinstance(v, bool)


def _rows(name: str, t, n: int) -> torch.Tensor:
    """A 1-D integer tensor of node rows of a graph of n nodes -> int64 (on its own device)."""
    if not torch.is_tensor(t) or t.dtype.is_floating_point or t.is_complex() or t.dtype == torch.bool:
        raise TypeError(f"{name}: expected a 1-D integer tensor of node rows, got {getattr(t, 'dtype', type(t).__name__)}")
    if t.dim() != 1:
        raise ValueError(f"{name}: expected a 1-D integer tensor of node rows, got shape {tuple(t.shape)}")
    if t.numel() and (int(t.min()) < 0 or int(t.max()) >= n):
        raise ValueError(f"{name}: rows {int(t.min())} .. {int(t.max())} of a graph of {n} nodes")
    return t.long()


def shoelace(xy: torch.Tensor) -> float:
    """The signed area of the closed polygon xy [n, 2] (fp64; positive: counter-clockwise)."""
    nx = torch.roll(xy, -1, 0)
    return 0.5 * float((xy[:, 0] * nx[:, 1] - nx[:, 0] * xy[:, 1]).sum())


def wall_geometry(pos: torch.Tensor, nodes=None, bodies=None, loops=None, centre=None) -> dict:
    """The wall tables of `BodyForces` from pos [N, 2] (used as fp32, computed in fp64, on pos's device): items int64 [W],
    body_offsets (a list of B + 1 integers), area / unit / arm fp64 [W, 2], angle fp64 [W], centre fp64 [B, 2].  `nodes`: the rows of
    the wall nodes or a bool mask [N]; `bodies`: an integer label per selected node (None: one body); `loops`: a list of 1-D row
    tensors, one per body, already in order (overrides nodes and bodies); `centre` [B, 2] (or [2] for one body; None: the fp64 mean
    of each body's wall nodes).  ValueError / TypeError naming the argument."""
    n = int(pos.size(0))
    xy = pos.detach().to(torch.float32).to(torch.float64)
    dev = xy.device
    if loops is not None:
        if not isinstance(loops, (list, tuple)) or not len(loops):
            raise TypeError(f"loops: expected a non-empty list of 1-D integer tensors (one per body), got {type(loops).__name__}")
        members = [_rows(f"loops[{b}]", lp, n).to(dev) for b, lp in enumerate(loops)]
    else:
        if nodes is None:
            raise ValueError("nodes: the graph has no `bound` to take the wall nodes (bound == 4) from, and no nodes= were given")
        if torch.is_tensor(nodes) and nodes.dtype == torch.bool:
            if tuple(nodes.shape) != (n,):
                raise ValueError(f"nodes: a bool mask of shape {tuple(nodes.shape)} for a graph of {n} nodes")
            rows = torch.nonzero(nodes.to(dev)).flatten()
        else:
            rows = _rows("nodes", nodes, n).to(dev)
        if not rows.numel():
            raise ValueError("nodes: no wall node (the set is empty)")
        if bodies is None:
            members = [rows]
        else:
            if not torch.is_tensor(bodies) or bodies.dtype.is_floating_point or bodies.is_complex() or bodies.dtype == torch.bool:
                raise TypeError(f"bodies: expected an integer label per wall node, got {getattr(bodies, 'dtype', type(bodies).__name__)}")
            if tuple(bodies.shape) != (int(rows.numel()),):
                raise ValueError(f"bodies: expected shape ({int(rows.numel())},) (a label per selected node), got {tuple(bodies.shape)}")
            labels = bodies.to(dev).long()
            members = [rows[labels == v] for v in torch.unique(labels, sorted=True).tolist()]
    n_bodies = len(members)
    if centre is not None:
        try:
            c = torch.as_tensor(centre, dtype=torch.float64).to(dev).reshape(-1, 2)
        except (TypeError, ValueError, RuntimeError):
            raise ValueError(f"centre: expected [{n_bodies}, 2] numbers, got {centre!r}") from None
        if int(c.size(0)) != n_bodies or not bool(torch.isfinite(c).all()):
            raise ValueError(f"centre: expected [{n_bodies}, 2] finite numbers, got shape {tuple(torch.as_tensor(centre).shape)}")
    items, offsets, areas, arms, angles, centres = [], [0], [], [], [], []
    for b, rows in enumerate(members):
        what = f"loops[{b}]" if loops is not None else ("nodes" if bodies is None else f"bodies: body {b}")
        if int(rows.numel()) < 3:
            raise ValueError(f"{what}: a body of {int(rows.numel())} wall node(s) (a closed polygon needs 3)")
        if int(torch.unique(rows).numel()) != int(rows.numel()):
            raise ValueError(f"{what}: a node is repeated within the body")
        cb = xy[rows].mean(0) if centre is None else c[b]
        if loops is None:                          # counter-clockwise about the centre: by angle, ties by node row
            rows = torch.sort(rows).values
            d = xy[rows] - cb
            rows = rows[torch.argsort(torch.atan2(d[:, 1], d[:, 0]), stable=True)]
        a2 = shoelace(xy[rows])
        if a2 == 0.0 or a2 != a2:
            raise ValueError(f"{what}: the polygon through the wall nodes has a zero area")
        if a2 < 0.0:
            rows = torch.flip(rows, (0,))
        p = xy[rows]
        nxt, prv = torch.roll(p, -1, 0), torch.roll(p, 1, 0)
        area = torch.stack([0.5 * (nxt[:, 1] - prv[:, 1]), -(0.5 * (nxt[:, 0] - prv[:, 0]))], dim=1)
        arm = p - cb
        items.append(rows)
        offsets.append(offsets[-1] + int(rows.numel()))
        areas.append(area)
        arms.append(arm)
        angles.append(torch.atan2(arm[:, 1], arm[:, 0]))
        centres.append(cb)
    area = torch.cat(areas)
    ds = torch.sqrt(area[:, 0] * area[:, 0] + area[:, 1] * area[:, 1])
    if bool((ds == 0).any()):
        raise ValueError(f"{'loops' if loops is not None else 'nodes'}: a wall item has a zero area vector (its two neighbours coincide)")
    return dict(items=torch.cat(items), body_offsets=offsets, area=area, unit=area / ds[:, None], arm=torch.cat(arms),
                angle=torch.cat(angles), centre=torch.stack(centres), n_bodies=n_bodies)


def check_forces(graph, nodes=None, bodies=None, loops=None, centre=None, *, mu=0.0, pressure=None, velocity=None, scale=None,
                 shift=None, gradient=None, power=2, edge_vectors=None) -> dict:
    """The arguments of `BodyForces` on the tensors as they were passed (nothing is moved, the library is not touched): its
    description (the wall tables of `wall_geometry` on the device of graph.pos, the columns, the constants), or ValueError /
    TypeError naming the argument."""
    pos = getattr(graph, "pos", None)
    if not torch.is_tensor(pos) or pos.dim() != 2 or not pos.dtype.is_floating_point:
        raise ValueError("graph: BodyForces needs graph.pos [N, 2]")
    if int(pos.size(1)) != 2:
        raise ValueError(f"graph: BodyForces is 2-D only, graph.pos is {tuple(pos.shape)} (a surface triangulation is out of scope)")
    n = int(pos.size(0))
    if not _number(mu) or mu != mu or mu in (float("inf"), float("-inf")):
        raise ValueError(f"mu: expected a finite number (the dynamic viscosity), got {mu!r}")
    pressure = 2 if pressure is None else pressure
    if not _integer(pressure) or pressure < 0:
        raise ValueError(f"pressure: expected a field number, got {pressure!r}")
    if velocity is None:
        velocity = (0, 1)
    else:
        try:
            velocity = tuple(velocity)
        except TypeError:
            raise ValueError(f"velocity: expected 2 field numbers, got {velocity!r}") from None
        if len(velocity) != 2 or not all(_integer(v) and v >= 0 for v in velocity):
            raise ValueError(f"velocity: expected 2 field numbers, got {velocity!r}")
    top = max((pressure,) + (velocity if mu != 0 else ()))
    factors = {}
    for name, v, default in (("scale", scale, 1.0), ("shift", shift, 0.0)):
        if v is None:
            factors[name] = None
            continue
        try:
            vals = [float(q) for q in (v.tolist() if torch.is_tensor(v) else v)]
        except (TypeError, ValueError):
            raise ValueError(f"{name}: expected [F] numbers (one per field), got {v!r}") from None
        if len(vals) <= top:
            raise ValueError(f"{name}: expected [F] numbers (one per field), F > field {top}, got {len(vals)}")
        factors[name] = vals
    if scale is not None and shift is not None and len(factors["scale"]) != len(factors["shift"]):
        raise ValueError(f"shift: {len(factors['shift'])} numbers, scale has {len(factors['scale'])}")
    if gradient is not None:
        if not isinstance(gradient, MeshGradient):
            raise TypeError(f"gradient: expected a gfd.MeshGradient of this graph or None, got {type(gradient).__name__}")
        if gradient.n_nodes != n or gradient.dim != 2:
            raise ValueError(f"gradient: a MeshGradient over {gradient.n_nodes} nodes in {gradient.dim} dimensions for a 2-D graph of {n}")
        if edge_vectors is not None:
            raise ValueError("edge_vectors: given together with gradient= (the operator carries its own)")
    elif mu != 0 or edge_vectors is not None or power != 2:
        if check_mesh(graph, power, edge_vectors) != 2:
            raise ValueError(f"edge_vectors: expected [E, 2] (the operator is 2-D), got {tuple(edge_vectors.shape)}")
    if loops is None and nodes is None:
        bound = getattr(graph, "bound", None)
        if torch.is_tensor(bound):
            if bound.numel() != n:
                raise ValueError(f"graph: graph.bound has {bound.numel()} entries for {n} nodes")
            nodes = bound.reshape(-1) == WALL
    geo = wall_geometry(pos, nodes, bodies, loops, centre)
    return dict(geo, n_nodes=n, mu=float(mu), pressure=pressure, velocity=velocity, scale=factors["scale"], shift=factors["shift"],
                power=power)


class BodyForces:
    """The force of the fields of `graph` (a 2-D Graph on the GPU) on the bodies in the flow, built once per mesh.

    The wall: `nodes` — the rows of the wall nodes (integer) or a bool mask [N]; None: `graph.bound == 4` —, `bodies` — an integer
    label per selected node (compacted to 0 .. B − 1 in ascending order); None: one body.  Each body's nodes are ordered
    counter-clockwise by atan2(y − c_y, x − c_x) about its `centre` c (default: the fp64 mean of its wall nodes), ties by node row:
    valid for a body that is STAR-SHAPED about c — circles and ellipses are.  For anything else pass `loops`, a list of 1-D index
    tensors, one per body and already in order (a clockwise loop is reversed); it overrides nodes and bodies.  ValueError for a 3-D
    mesh, an empty set, a body of fewer than 3 nodes or of zero area, a node repeated within a body.

    The physics: `pressure` the field number of p (default 2), `velocity` the pair (u, v) (default (0, 1)); `scale`, `shift` [F]: the
    physical field is scale · x + shift; `mu` the dynamic viscosity in those units — mu = 0 gives the pressure force only and the
    velocity fields need not exist.  `gradient`: a `gfd.MeshGradient` of this graph; None builds one with `power` and `edge_vectors`
    (on a periodic mesh pass the wrapped `edge_attr`, as for `MeshGradient`) when mu != 0.

    `forces(x)` [B, 6] float64 = (Fp_x, Fp_y, Fv_x, Fv_y, Mp, Mv) of the fields x [N, F] float32 — pressure and viscous force, and
    their moments about the centre; `wall(x)` [W, 2] float32: the surface pressure and the wall shear at every wall item;
    `history(x, n)` [n, B, 6]: the same for the n steps held in x [N, >= nf n] (a target; nf: the fields of a step).  `items` [W]
    the node rows, body after body (`body_offsets` [B + 1]), `area`, `unit`, `arm` [W, 2] float64, `angle` [W] — what Cp(θ) is plotted
    against —, `centre` [B, 2], `n_bodies`, `gradient`.

    `forces` and `wall` of an x that requires grad are recorded for autograd: their backward is `adjoint(gF, gwall, nf)` [N, nf], the
    transpose of the map's linear part (no gradient reaches the mesh or the wall geometry); `history` is not differentiable.  The
    node-side tables the adjoint walks are built on its first use."""

    def __init__(self, graph, nodes=None, bodies=None, loops=None, centre=None, *, mu: float = 0.0, pressure: Optional[int] = None,
                 velocity=None, scale=None, shift=None, gradient: Optional[MeshGradient] = None, power: int = 2,
                 edge_vectors: Optional[torch.Tensor] = None):
        spec = check_forces(graph, nodes, bodies, loops, centre, mu=mu, pressure=pressure, velocity=velocity, scale=scale, shift=shift,
                            gradient=gradient, power=power, edge_vectors=edge_vectors)
        dev = graph.pos.device
        if dev.type != "cuda":
            raise ValueError(f"graph: BodyForces runs on a HIP device only, graph.pos is on '{dev}' (there is no CPU fallback)")
        self._spec = spec
        self.n_nodes, self.n_bodies, self.mu = spec["n_nodes"], spec["n_bodies"], spec["mu"]
        self.pressure, self.velocity, self.scale, self.shift, self.power = spec["pressure"], spec["velocity"], spec["scale"], spec["shift"], power
        self.items, self.area, self.unit, self.arm = spec["items"], spec["area"].contiguous(), spec["unit"].contiguous(), spec["arm"].contiguous()
        self.angle, self.centre = spec["angle"], spec["centre"]
        self.body_offsets = torch.tensor(spec["body_offsets"], dtype=torch.int32, device=dev)
        self._item32 = self.items.to(torch.int32).contiguous()
        if gradient is None and self.mu != 0:
            gradient = MeshGradient(graph, power, edge_vectors)
        self.gradient = gradient
        self._adjoint_tables = None

    @property
    def n_items(self) -> int:
        return int(self.items.numel())

    def constants(self) -> dict:
        """The columns and fp64 constants of the launch (`ops.body_forces`'s keywords)."""
        sc, sh = self.scale, self.shift
        u, v = self.velocity
        viscous = self.mu != 0
        return dict(pcol=self.pressure, ucol=u if viscous else 0, vcol=v if viscous else 0, mu=self.mu,
                    p_scale=1.0 if sc is None else sc[self.pressure], p_shift=0.0 if sh is None else sh[self.pressure],
                    u_scale=1.0 if sc is None or not viscous else sc[u], v_scale=1.0 if sc is None or not viscous else sc[v])

    def fields_needed(self) -> int:
        return max((self.pressure,) + (self.velocity if self.mu != 0 else ())) + 1

    def _x(self, x, width: int) -> torch.Tensor:
        if not torch.is_tensor(x) or x.dtype != torch.float32 or x.dim() != 2 or int(x.size(0)) != self.n_nodes or int(x.size(1)) < width:
            raise ValueError(f"x: expected a float32 tensor [{self.n_nodes}, >= {width}], got {getattr(x, 'dtype', type(x).__name__)} "
                             f"{tuple(getattr(x, 'shape', ()))}")
        return x

    def _launch(self, x, stats, t: int, x_step: int, cur=None, wall=None):
        dev, g = self.area.device, self.gradient if self.mu != 0 else None
        cur = torch.empty((self.n_bodies, 3), dtype=torch.float32, device=dev) if cur is None else cur
        ops.body_forces(x, self._item32, self.body_offsets, self.area, self.unit, self.arm, cur, **self.constants(),
                        off=None if g is None else g.off, g=None if g is None else g.g, src=None if g is None else g.src, wall=wall,
                        stats=stats, max_steps=int(stats.size(0)), t=t, x_step=x_step)
        return cur

    def forces(self, x: torch.Tensor) -> torch.Tensor:
        """[B, 6] float64: (Fp_x, Fp_y, Fv_x, Fv_y, Mp, Mv) of the fields x [N, F] (float32, rows of unit stride).  Of an x that requires
        grad (with grad enabled) the result carries a `grad_fn` whose backward is `adjoint(gF=...)`."""
        x = self._x(x, self.fields_needed())
        if torch.is_grad_enabled() and x.requires_grad:
            from . import autograd as _ag
            return _ag.body_forces(self, x)
        return self._forces(x)

    def _forces(self, x: torch.Tensor) -> torch.Tensor:
        stats = torch.zeros((1, self.n_bodies, _lib.FORCES_NSUM), dtype=torch.float64, device=self.area.device)
        self._launch(x, stats, 0, 0)
        return stats[0]

    def wall(self, x: torch.Tensor) -> torch.Tensor:
        """[W, 2] float32: the surface pressure and the wall shear of the fields x [N, F] at every wall item.  Of an x that requires
        grad (with grad enabled) the result carries a `grad_fn` whose backward is `adjoint(gwall=...)`."""
        x = self._x(x, self.fields_needed())
        if torch.is_grad_enabled() and x.requires_grad:
            from . import autograd as _ag
            return _ag.body_wall(self, x)
        return self._wall(x)

    def _wall(self, x: torch.Tensor) -> torch.Tensor:
        stats = torch.zeros((1, self.n_bodies, _lib.FORCES_NSUM), dtype=torch.float64, device=self.area.device)
        wall = torch.empty((self.n_items, 2), dtype=torch.float32, device=self.area.device)
        self._launch(x, stats, 0, 0, wall=wall)
        return wall

    def _node_side(self) -> dict:
        """The node-side tables of the adjoint (include/g4c.h): item_body [W]; own_off [N + 1] / own_item [W], the items grouped by
        their node, ascending; and, for mu != 0, in_off [N + 1] / in_item [Q] / in_g [Q, 2]: the pairs (item w, in-edge e of its node)
        grouped by the sender of e, ascending CSR position e, then w, within a sender, the weights copied into that order.  Built on
        the first adjoint and kept: the plain forward pays nothing."""
        if self._adjoint_tables is None:
            n_items, n = self.n_items, self.n_nodes
            viscous = self.mu != 0
            if viscous and n_items * max(int(self.gradient.max_deg), 0) > 2 ** 31 - 1:
                raise NotImplementedError(f"BodyForces.adjoint: up to {n_items} · {int(self.gradient.max_deg)} (items · in-edges) list "
                                          f"entries do not fit the int32 offsets")
            dev = self._item32.device
            sizes = (self.body_offsets[1:] - self.body_offsets[:-1]).to(torch.int64)
            item_body = torch.repeat_interleave(torch.arange(self.n_bodies, dtype=torch.int32, device=dev), sizes, output_size=n_items)
            own = plan.gather_csr(self._item32, n)
            own_item = own.perm if own.perm is not None else torch.arange(n_items, dtype=torch.int32, device=dev)
            tabs = dict(item_body=item_body.contiguous(), own_off=own.off, own_item=own_item.contiguous())
            if viscous:
                gr = self.gradient
                off = gr.off.to(torch.int64)
                first = off[self.items]
                deg = off[self.items + 1] - first
                q = int(deg.sum())
                w = torch.repeat_interleave(torch.arange(n_items, dtype=torch.int64, device=dev), deg, output_size=q)
                e = first[w] + (torch.arange(q, dtype=torch.int64, device=dev) - (torch.cumsum(deg, 0) - deg)[w])
                order = torch.argsort(e, stable=True)          # ascending CSR position; a node that is an item twice: ascending w
                w, e = w[order], e[order]
                sender = gr.src.index_select(0, e).contiguous() if q else torch.zeros(0, dtype=torch.int32, device=dev)
                if q:
                    by = plan.build_csr(sender, n, dev)          # (a stable grouping; not cached: `sender` lives only here)
                    if by.perm is not None:
                        perm = by.perm.to(torch.int64)
                        w, e = w[perm], e[perm]
                    in_off = by.off
                else:
                    in_off = torch.zeros(n + 1, dtype=torch.int32, device=dev)
                tabs.update(in_off=in_off, in_item=w.to(torch.int32).contiguous(),
                            in_g=gr.g.index_select(0, e).contiguous() if q else torch.zeros((0, 2), dtype=torch.float32, device=dev))
            self._adjoint_tables = tabs
        return self._adjoint_tables

    def _adjoint(self, gF, gwall, nf: int, out=None, hw=None) -> torch.Tensor:
        t = self._node_side()
        c = self.constants()
        c.pop("p_shift")
        gr = self.gradient if self.mu != 0 else None
        return ops.body_forces_adjoint(gF, gwall, t["item_body"], self.area, self.unit, self.arm, t["own_off"], t["own_item"], self.n_bodies,
                                       nf, **c, g=None if gr is None else gr.g, off=None if gr is None else gr.off, in_off=t.get("in_off"),
                                       in_item=t.get("in_item"), in_g=t.get("in_g"), hw=hw, out=out)

    def adjoint(self, gF: Optional[torch.Tensor] = None, gwall: Optional[torch.Tensor] = None, nf: Optional[int] = None) -> torch.Tensor:
        """[N, nf] float32: the transpose of the linear part of `forces` and `wall`, applied to gF [B, 6] (float64) and gwall [W, 2]
        (float32), either may be None (zeros); both are made dense first.  For all x,

            ⟨forces(x) − forces(0), gF⟩ + ⟨wall(x) − wall(0), gwall⟩ = ⟨x, adjoint(gF, gwall)⟩   up to rounding

        (forces(0) and wall(0) are what `shift` alone gives).  nf defaults to the length of `scale`, else to `fields_needed()`.  Two
        small launches (`g4c_body_forces_adjoint`): per item, then a gather per node in a fixed order, no atomics.  A node that
        neither is a wall node nor sends to one gets zeros."""
        if nf is None:
            nf = len(self.scale) if self.scale is not None else self.fields_needed()
        if not _integer(nf) or nf < self.fields_needed():
            raise ValueError(f"nf: {nf!r} fields, the operator reads field {self.fields_needed() - 1}")
        for name, t, dtype, shape in (("gF", gF, torch.float64, (self.n_bodies, _lib.FORCES_NSUM)),
                                      ("gwall", gwall, torch.float32, (self.n_items, 2))):
            if t is None:
                continue
            if not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != shape:
                raise ValueError(f"{name}: expected a {str(dtype).replace('torch.', '')} tensor {list(shape)}, got "
                                 f"{getattr(t, 'dtype', type(t).__name__)} {tuple(getattr(t, 'shape', ()))}")
            if t.device != self.area.device:
                raise ValueError(f"{name}: on '{t.device}', the operator is on '{self.area.device}' (there is no CPU fallback)")
        return self._adjoint(None if gF is None else gF.detach().contiguous(), None if gwall is None else gwall.detach().contiguous(), nf)

    def history(self, x: torch.Tensor, n: int, nf: Optional[int] = None) -> torch.Tensor:
        """[n, B, 6] float64: `forces` of the n steps held in x [N, >= nf n] — a target: step t in the columns nf t .. nf (t + 1).
        nf defaults to the length of `scale`, else to x's columns // n.  n launches.  Not differentiable: no gradient reaches x."""
        if not _integer(n) or n < 1:
            raise ValueError(f"n: expected a number of steps >= 1, got {n!r}")
        if nf is None:
            nf = len(self.scale) if self.scale is not None else (int(x.size(1)) // n if torch.is_tensor(x) and x.dim() == 2 else 0)
        if not _integer(nf) or nf < self.fields_needed():
            raise ValueError(f"nf: {nf!r} fields a step, the operator reads field {self.fields_needed() - 1}")
        x = self._x(x, nf * n)
        stats = torch.zeros((n, self.n_bodies, _lib.FORCES_NSUM), dtype=torch.float64, device=self.area.device)
        cur = torch.empty((self.n_bodies, 3), dtype=torch.float32, device=self.area.device)
        for t in range(n):
            self._launch(x, stats, t, nf, cur=cur)
        return stats

    def __repr__(self):
        return f"BodyForces(nodes={self.n_nodes}, bodies={self.n_bodies}, items={self.n_items}, mu={self.mu})"
