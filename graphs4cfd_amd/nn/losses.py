"""Training losses (reference: graphs4cfd/nn/losses.py:5-16)."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F


class GraphLoss(nn.Module):
    """MSE over all nodes, plus `lambda_d` times the L1 error on the Dirichlet-boundary nodes (`graph.omega[:, 0] == 1`) when
    `lambda_d > 0` and the batch has any (nn/losses.py:10-16).  The loss works on the [N, num_fields] prediction — a few
    hundred kB — and is ordinary torch arithmetic; its gradient enters the fused blocks through autograd.py."""

    def __init__(self, lambda_d=0):
        super().__init__()
        self.lambda_d = lambda_d

    def forward(self, graph, pred, target):
        loss = F.mse_loss(pred, target)
        if self.lambda_d > 0:
            dirichlet_boundary = (graph.omega[:, 0] == 1)
            if dirichlet_boundary.any():
                loss = loss + self.lambda_d * F.l1_loss(pred[dirichlet_boundary], target[dirichlet_boundary])
        return loss


def _number(v, name, what="a finite number >= 0"):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
        raise ValueError(f"{name}: expected {what}, got {v!r}")
    return float(v)


def _power(v, noun):
    if isinstance(v, bool) or not isinstance(v, int) or v not in (0, 1, 2):
        raise ValueError(f"power: expected 0, 1 or 2 ({noun} weighs |d|^-power), got {v!r}")
    return v


def _field_numbers(v, name, noun, lengths=None, distinct=False):
    """None, or `v` as a tuple of field numbers >= 0: `lengths` the allowed counts (None: any but none), `distinct`: none twice."""
    if v is None:
        return None
    try:
        v = tuple(v)
    except TypeError:
        raise ValueError(f"{name}: expected {noun}, got {v!r}") from None
    if ((not v if lengths is None else len(v) not in lengths) or any(isinstance(f, bool) or not isinstance(f, int) or f < 0 for f in v)
            or (distinct and len(set(v)) != len(v))):
        raise ValueError(f"{name}: expected {noun}, got {v!r}")
    return v


def _per_field(v, name, noun):
    """None, or `v` (a tensor or a sequence) as a list of floats: one finite `noun` per field."""
    if v is None:
        return None
    try:
        v = [float(q) for q in (v.tolist() if torch.is_tensor(v) else v)]
    except (TypeError, ValueError):
        raise ValueError(f"{name}: expected one {noun} per field, got {v!r}") from None
    if not v or not all(math.isfinite(q) for q in v):
        raise ValueError(f"{name}: expected one finite {noun} per field, got {v!r}")
    return v


def _attribute(v, name, what="a graph attribute", kind=ValueError):
    if v is not None and (not isinstance(v, str) or not v):
        raise kind(f"{name}: expected None or the name of {what}, got {v!r}")
    return v


def _values(v, noun):
    if v is not None and (not isinstance(v, str) or not v or "index" in v):
        raise ValueError(f"values: expected None or the name of a graph attribute holding {noun} (without 'index' in it: such "
                         f"attributes collate along the last dimension), got {v!r}")
    return v


class _OperatorLoss(nn.Module):
    """What `FlowLoss`, `SampleLoss`, `ForceLoss` and `ResidualLoss` share: node_weight · `GraphLoss(lambda_d)` in front of their own
    term, the operator that term needs — built from tensors of the batch and kept while those are the same objects, unmodified —
    and the columns of an observed attribute that belong to one output step."""

    def __init__(self, lambda_d, weight=1.0, node_weight=1.0):
        super().__init__()
        self.lambda_d = _number(lambda_d, "lambda_d")
        self.weight = _number(weight, "weight", "a finite weight >= 0")
        self.node_weight = _number(node_weight, "node_weight", "a finite weight >= 0")
        self.base = GraphLoss(lambda_d)
        self._cache = None          # ([(tensor or None, its version), ...], what `build` returned)
        self.builds = 0             # operators built so far (a batch seen again costs none)

    def keep(self, tensors, build):
        """`build()`, or what it returned last time when every entry of `tensors` (tensors, or None) is the object it was then,
        unmodified — identity and `_version`: an address says nothing, the allocator hands a freed batch's to the next one.  One
        entry is kept."""
        hit = self._cache
        if (hit is None or len(hit[0]) != len(tensors)
                or not all(a is t and (not torch.is_tensor(t) or v == t._version) for (a, v), t in zip(hit[0], tensors))):
            self._cache = ([(t, t._version if torch.is_tensor(t) else None) for t in tensors], build())
            self.builds += 1
        return self._cache[1]

    def node_term(self, graph, pred, target):
        """node_weight · GraphLoss, or None at node_weight == 0; at exactly 1.0 it is not multiplied (GraphLoss's bits)."""
        if not self.node_weight > 0:
            return None
        loss = self.base(graph, pred, target)
        return loss if self.node_weight == 1.0 else self.node_weight * loss

    @staticmethod
    def nothing_more(pred, loss):
        """The value when the loss's own term is absent: the node term, or a zero that still depends on pred."""
        return pred.sum() * 0.0 if loss is None else loss

    @staticmethod
    def observed(graph, name, rows, per_step, step, what):
        """Columns per_step · t .. per_step · (t + 1) of graph.<name> [rows, per_step · T] for output step t = `step`."""
        obs = getattr(graph, name, None)
        if not torch.is_tensor(obs) or obs.dim() != 2 or int(obs.size(0)) != rows:
            raise ValueError(f"values: graph.{name}: expected {what}, got {tuple(getattr(obs, 'shape', ()))}")
        t = int(step)
        if t < 0 or per_step * (t + 1) > int(obs.size(1)):
            raise ValueError(f"step: {t}: graph.{name} holds {int(obs.size(1))} columns, {per_step} per step")
        return obs[:, per_step * t: per_step * (t + 1)]


class FlowLoss(_OperatorLoss):
    """`GraphLoss(lambda_d)` plus penalties on what the mesh's least-squares gradient (`gfd.MeshGradient`) makes of the prediction
    (new functionality — the reference has none):

        GraphLoss(lambda_d)(graph, pred, target) + Σ_name terms[name] · mean over all N nodes and the name's columns of D_name(pred − ref_name)²

    `terms` maps the names of `MeshGradient.derived` ('div', 'vort', 'grad:<field>') to weights >= 0; ref_name is 0 for the names in
    `zero` (a continuity penalty: the divergence itself is driven to 0) and `target` for the others (Sobolev terms: the derivative of
    the error).  Degenerate nodes have no derivative and contribute 0.  `power`, `velocity`, `field_scale` mean what they mean in
    `MeshGradient` / `MeshGradient.derived`; `edge_vectors` is None (differences of `graph.pos`) or the name of a graph attribute that
    holds the unscaled, wrapped [E, dim] edge vectors (a periodic mesh: see `MeshGradient`).

    At most two differentiable `derived` launches per call (one on pred − target, one on pred), each with its transpose
    (`g4c_mesh_derived_adjoint`) in the backward; under `torch.no_grad()` the forward launches alone.  With no term of non-zero weight
    nothing is launched and the value and gradients are `GraphLoss`'s, bit for bit.  A collated batch is block-diagonal: the operator
    is built on the batch as it is, and kept (one entry) while the batch's `edge_index` and positions / vectors are the same tensor
    objects, unmodified — `Trainer.train_epoch` calls the loss once per output step of the same batch.  HIP device only."""

    def __init__(self, lambda_d=0, terms=None, zero=("div",), power=2, velocity=None, field_scale=None, edge_vectors=None):
        super().__init__(lambda_d)
        if terms is None:
            terms = {}
        if not isinstance(terms, dict):
            raise ValueError(f"terms: expected a dict of names ('div', 'vort', 'grad:<field>') to weights, got {terms!r}")
        for name, w in terms.items():
            self._name(name, "terms")
            _number(w, f"terms[{name!r}]", "a finite weight >= 0")
        if isinstance(zero, str):
            zero = (zero,)
        try:
            zero = tuple(zero)
        except TypeError:
            raise ValueError(f"zero: expected a tuple of names, got {zero!r}") from None
        for name in zero:
            self._name(name, "zero")
        power = _power(power, "an edge")
        velocity = _field_numbers(velocity, "velocity", "2 or 3 field numbers", lengths=(2, 3))
        field_scale = _per_field(field_scale, "field_scale", "factor")
        _attribute(edge_vectors, "edge_vectors", "a graph attribute holding [E, dim] vectors")
        live = [(name, float(w)) for name, w in terms.items() if w > 0]
        self.terms = dict(terms)
        self.zero = zero
        self._on_error = [(n, w) for n, w in live if n not in zero]          # D(pred − target)
        self._on_pred = [(n, w) for n, w in live if n in zero]               # D(pred)
        self.power, self.velocity, self.field_scale, self.edge_vectors = power, velocity, field_scale, edge_vectors

    @staticmethod
    def _name(name, arg):
        if not isinstance(name, str) or not (name in ("div", "vort") or (name.startswith("grad:") and name[5:].isdigit())):
            raise ValueError(f"{arg}: unknown name {name!r} ('div', 'vort' and 'grad:<field>' are known)")

    def operator(self, graph):
        """The `MeshGradient` of `graph` — the cached one while graph.edge_index and the tensor its vectors came from are the objects
        it was built from, unmodified (identity and `_version`: an address says nothing, the allocator hands a freed batch's to the
        next one)."""
        from ..mesh_gradient import MeshGradient
        ei = getattr(graph, "edge_index", None)
        if self.edge_vectors is None:
            vec = getattr(graph, "pos", None)
        else:
            vec = getattr(graph, self.edge_vectors, None)
            if not torch.is_tensor(vec):
                raise ValueError(f"edge_vectors: the graph has no tensor attribute {self.edge_vectors!r}")
        return self.keep([ei, vec], lambda: MeshGradient(graph, power=self.power, edge_vectors=None if self.edge_vectors is None else vec))

    def forward(self, graph, pred, target):
        loss = self.node_term(graph, pred, target)
        if not self._on_error and not self._on_pred:
            return loss
        op = self.operator(graph)
        for group, x in ((self._on_error, None), (self._on_pred, pred)):
            if not group:
                continue
            if x is None:
                x = pred - target
            names = tuple(n for n, _ in group)
            d = op.derived(x, names, velocity=self.velocity, field_scale=self.field_scale)
            c0 = 0
            for name, w in group:
                c1 = c0 + len(op.columns((name,)))
                loss = loss + w * d[:, c0:c1].square().mean()
                c0 = c1
        return loss


class SampleLoss(_OperatorLoss):
    """`GraphLoss(lambda_d)` plus the error at points that are no nodes — sparse, off-node observations: a PIV window, a wake rake, a
    few taps (new functionality — the reference has none):

        node_weight · GraphLoss(lambda_d)(graph, pred, target) + weight · mean over the kept points and the chosen fields of (S·pred − ref)²

    S is `gfd.PointSampler(graph, points, k, power)`: the moving-least-squares interpolation from the nodes to `points` [P, dim].  The
    points are FIXED in the coordinates of `graph.pos` as the loss sees it — sensors in the lab frame: an augmentation that moves or
    scales the mesh does not move the points.  `fields`: the columns of the prediction that were observed (default: all; PIV gives
    no pressure), F' of them.  ref is S·target when `values` is None (a loss weighted towards a region: no data beyond the node
    targets), otherwise `getattr(graph, values)[:, F'·t : F'·(t + 1)]` — observations [P, F'·T] per graph, for output step t = `step`
    (`takes_step`: `Trainer` passes step=t; `values=` without a step is a ValueError).  `max_distance` drops the points farther than
    that from their nearest node (inside a body, outside the domain); with no point kept the term is 0.  `period`: `PointSampler`'s,
    passed to each graph's sampler (a periodic mesh: the points next to the seam are fitted from both sides of it).

    `node_weight == 0` skips `GraphLoss` (training on observations alone); `weight == 0` launches nothing, builds nothing and is
    node_weight · GraphLoss bit for bit.  The sample is differentiable (`g4c_sample_points_adjoint` in the backward).

    A collated batch: graphs of a batch usually overlap in space, so every graph gets a search of its own over its node range of
    `graph.batch` (contiguous, ascending), its neighbours are offset by the range's start, and the tables are joined along P,
    graph-major, into one sampler (`PointSampler.from_tables`); observations collate along dim 0 by `collate`'s rule (`values` must
    not contain 'index') into [B·P, F'·T], the same order.  The sampler is kept (one entry) while `graph.pos` and `graph.batch` are
    the same tensor objects, unmodified — `Trainer.train_epoch` calls the loss once per output step of the same batch; `builds`
    counts the samplers built.  HIP device only."""

    takes_step = True

    def __init__(self, points, lambda_d=0, weight=1.0, node_weight=1.0, values=None, fields=None, k=None, power=2, max_distance=None,
                 period=None):
        from ..point_sampler import MAX_K
        from ..synthetic import check_period
        if not torch.is_tensor(points) or not points.dtype.is_floating_point or points.dim() != 2 or int(points.size(1)) not in (2, 3):
            raise ValueError(f"points: expected a floating-point tensor [P, 2] or [P, 3], got "
                             f"{getattr(points, 'dtype', type(points).__name__)} {tuple(getattr(points, 'shape', ()))}")
        if points.device.type == "cpu" and not bool(torch.isfinite(points).all()):
            raise ValueError("points: a coordinate that is not finite")
        super().__init__(lambda_d, weight, node_weight)
        values = _values(values, "[P, F'·T] observations")
        fields = _field_numbers(fields, "fields", "distinct column numbers >= 0", distinct=True)
        if k is not None and (isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= MAX_K):
            raise ValueError(f"k: expected None or an integer 1 <= k <= {MAX_K}, got {k!r}")
        power = _power(power, "a neighbour")
        if max_distance is not None:
            max_distance = _number(max_distance, "max_distance", "None or a finite distance >= 0")
        self.points, self.values, self.fields, self.k, self.power, self.max_distance = points.detach(), values, fields, k, power, max_distance
        self.period = check_period(period, int(points.size(1)), "SampleLoss")

    def sampler(self, graph):
        """(the `PointSampler` of `graph` — of all its graphs, when it is a batch —, the bool [P] mask of the kept points or None for
        all, their number): the cached ones while graph.pos and graph.batch are the objects they were built from, unmodified
        (identity and `_version`, never an address)."""
        pos, batch = getattr(graph, "pos", None), getattr(graph, "batch", None)
        if not torch.is_tensor(pos):
            raise ValueError("graph: SampleLoss needs graph.pos")
        return self.keep([pos, batch], lambda: self._build(graph, pos, batch))

    def _build(self, graph, pos, batch):
        from ..graph import Graph
        from ..point_sampler import PointSampler
        n = int(pos.size(0))
        counts = [n] if batch is None else torch.bincount(batch).tolist()
        if sum(counts) != n:
            raise ValueError(f"graph: graph.batch names {sum(counts)} nodes, graph.pos has {n}")
        if len(counts) == 1:
            s = PointSampler(graph, self.points, k=self.k, power=self.power, period=self.period)
        else:
            parts, a = [], 0
            for c in counts:          # (contiguous ranges: `collate` numbers the nodes graph after graph)
                one = PointSampler(Graph(pos=pos[a:a + c]), self.points, k=self.k, power=self.power, period=self.period)
                parts.append((one._idx + a, one._coef, one.distance, one.degenerate))
                a += c
            idx, coef, distance, degenerate = (torch.cat(t, dim=-1).contiguous() for t in zip(*parts))
            s = PointSampler.from_tables(idx, coef, n, points=self.points.repeat(len(counts), 1), distance=distance, degenerate=degenerate)
        mask, kept = None, s.n_points
        if self.max_distance is not None:
            mask = s.distance <= self.max_distance
            kept = int(mask.sum())
        return s, mask, kept

    def forward(self, graph, pred, target, step=None):
        loss = self.node_term(graph, pred, target)
        if self.weight == 0:
            return self.nothing_more(pred, loss)
        if self.values is not None and step is None:
            raise ValueError("step: SampleLoss(values=...) needs the output step: call loss(graph, pred, target, step=t)")
        s, mask, kept = self.sampler(graph)
        cols = list(range(int(pred.size(1)))) if self.fields is None else list(self.fields)
        if max(cols) >= int(pred.size(1)):
            raise ValueError(f"fields: column {max(cols)} of a prediction with {int(pred.size(1))} columns")
        nfp = len(cols)
        if kept == 0:
            return self.nothing_more(pred, loss)
        if self.values is None:
            d = s.sample(pred - target)          # S is linear: S·pred − S·target in one launch
            if self.fields is not None:
                d = d[:, cols]
        else:
            obs = self.observed(graph, self.values, s.n_points, nfp, step, f"observations [{s.n_points}, F'·T]")
            sp = s.sample(pred)
            if self.fields is not None:
                sp = sp[:, cols]
            d = sp - obs.to(sp.dtype)
        sq = d.square()
        if mask is not None:
            sq = sq * mask[:, None].to(sq.dtype)
        term = self.weight * (sq.sum() / (kept * nfp))
        return term if loss is None else loss + term


class ForceLoss(_OperatorLoss):
    """`GraphLoss(lambda_d)` plus the error of the loads on the bodies in the flow — what a load cell and pressure taps measure (new
    functionality — the reference has none):

        node_weight · GraphLoss(lambda_d)(graph, pred, target)
          + weight · mean over the bodies and `components` of ((F(pred) − F_ref) / force_scale)²
          + wall["pressure"] · mean_w (P_w(pred) − P_w(target))² + wall["shear"] · mean_w (shear_w(pred) − shear_w(target))²

    F is `gfd.BodyForces(graph, ...).forces`: per body the totals 'fx' = Fp_x + Fv_x, 'fy' and 'm' (the moment about the centre), kept
    in float64 until the mean and then cast to the prediction's dtype.  F_ref is forces(target) when `values` is None, otherwise
    `getattr(graph, values)[:, C·t : C·(t + 1)]` — measured loads [B, C·T] per graph, C = len(components), for output step t = `step`
    (`takes_step`: `Trainer` passes step=t; `values=` without a step is a ValueError).  The wall term (Cp(θ) and the wall shear, from
    `BodyForces.wall`) exists when `wall` gives one of its two weights.  `mu`, `pressure`, `velocity`, `scale`, `shift`, `centre`,
    `power` mean what they mean in `BodyForces`; `edge_vectors` is None or the name of a graph attribute holding the unscaled, wrapped
    [E, 2] edge vectors (a periodic mesh).

    The wall on a collated batch: `nodes` is None (`graph.bound == 4`) or the name of a per-node graph attribute [N], bool or integer
    (non-zero: a wall node); `bodies` is None — one body per graph of `graph.batch`: a wall node's label is its batch number — or the
    name of a per-node integer attribute whose value at a wall node, combined with the batch number, labels its body.  The gradient
    operator is built on the batch as it is (a collated batch is block-diagonal).  The operator is kept (one entry) while the batch's
    `pos`, `edge_index` (when mu != 0), `batch` and the tensors the nodes, bodies and vectors came from are the same tensor objects,
    unmodified (identity and `_version`, never an address) — `Trainer.train_epoch` calls the loss once per output step of the same
    batch; `builds` counts the operators built.

    Both loads are differentiable (`g4c_body_forces_adjoint` in the backward).  With `weight == 0` and no live wall weight nothing is
    built or launched and the value is node_weight · GraphLoss bit for bit; `node_weight == 0` skips `GraphLoss` (training on loads
    alone).  HIP device only."""

    takes_step = True
    COMPONENTS = {"fx": (0, 2), "fy": (1, 3), "m": (4, 5)}          # the columns of BodyForces.forces each total adds

    def __init__(self, lambda_d=0, weight=1.0, node_weight=1.0, *, mu=0.0, pressure=None, velocity=None, scale=None, shift=None,
                 components=("fx", "fy"), force_scale=1.0, wall=None, values=None, nodes=None, bodies=None, centre=None, power=2,
                 edge_vectors=None):
        super().__init__(lambda_d, weight, node_weight)
        if isinstance(mu, bool) or not isinstance(mu, (int, float)) or not math.isfinite(mu):
            raise ValueError(f"mu: expected a finite number (the dynamic viscosity), got {mu!r}")
        if pressure is not None and (isinstance(pressure, bool) or not isinstance(pressure, int) or pressure < 0):
            raise ValueError(f"pressure: expected a field number, got {pressure!r}")
        velocity = _field_numbers(velocity, "velocity", "2 field numbers", lengths=(2,))
        scale, shift = _per_field(scale, "scale", "number"), _per_field(shift, "shift", "number")
        if isinstance(components, str):
            components = (components,)
        try:
            components = tuple(components)
        except TypeError:
            raise ValueError(f"components: expected distinct names of 'fx', 'fy', 'm', got {components!r}") from None
        if not components or any(c not in self.COMPONENTS for c in components) or len(set(components)) != len(components):
            raise ValueError(f"components: expected distinct names of 'fx', 'fy', 'm', got {components!r}")
        if isinstance(force_scale, bool) or not isinstance(force_scale, (int, float)) or not math.isfinite(force_scale) or force_scale <= 0:
            raise ValueError(f"force_scale: expected a finite number > 0, got {force_scale!r}")
        if wall is not None:
            if not isinstance(wall, dict) or not set(wall) <= {"pressure", "shear"}:
                raise TypeError(f"wall: expected None or a dict with the weights 'pressure' and / or 'shear', got {wall!r}")
        wall = dict(wall or {})
        self.wall_pressure = _number(wall.get("pressure", 0.0), "wall['pressure']", "a finite weight >= 0")
        self.wall_shear = _number(wall.get("shear", 0.0), "wall['shear']", "a finite weight >= 0")
        values = _values(values, "[B, C·T] measured loads")
        for name, v in (("nodes", nodes), ("bodies", bodies), ("edge_vectors", edge_vectors)):
            _attribute(v, name, kind=TypeError)
        if centre is not None:
            try:
                c = torch.as_tensor(centre, dtype=torch.float64).reshape(-1, 2)
            except (TypeError, ValueError, RuntimeError):
                raise ValueError(f"centre: expected [B, 2] numbers, got {centre!r}") from None
            if not c.numel() or not bool(torch.isfinite(c).all()):
                raise ValueError(f"centre: expected [B, 2] finite numbers, got {centre!r}")
        power = _power(power, "an edge")
        self.mu, self.pressure, self.velocity, self.scale, self.shift = float(mu), pressure, velocity, scale, shift
        self.components, self.force_scale, self.wall, self.values = components, float(force_scale), wall, values
        self.nodes, self.bodies, self.centre, self.power, self.edge_vectors = nodes, bodies, centre, power, edge_vectors

    def _attr(self, graph, arg, name, n):
        t = getattr(graph, name, None)
        if not torch.is_tensor(t) or t.dtype.is_floating_point or t.is_complex() or t.numel() != n:
            raise ValueError(f"{arg}: graph.{name}: expected a per-node {'bool or ' if arg == 'nodes' else ''}integer tensor [{n}], got "
                             f"{getattr(t, 'dtype', type(t).__name__)} {tuple(getattr(t, 'shape', ()))}")
        return t

    def operator(self, graph):
        """The `BodyForces` of `graph` — of all its graphs, when it is a batch —: the cached one while the tensors it was built from
        are the same objects, unmodified (identity and `_version`: an address says nothing, the allocator hands a freed batch's to the
        next one)."""
        pos = getattr(graph, "pos", None)
        if not torch.is_tensor(pos) or pos.dim() != 2:
            raise ValueError("graph: ForceLoss needs graph.pos [N, 2]")
        n = int(pos.size(0))
        batch = getattr(graph, "batch", None)
        if self.nodes is None:
            flag = getattr(graph, "bound", None)
            if not torch.is_tensor(flag) or flag.numel() != n:
                raise ValueError("nodes: the graph has no `bound` [N] to take the wall nodes (bound == 4) from, and no nodes= names an attribute")
        else:
            flag = self._attr(graph, "nodes", self.nodes, n)
        label = None if self.bodies is None else self._attr(graph, "bodies", self.bodies, n)
        if label is not None and label.dtype == torch.bool:
            raise ValueError(f"bodies: graph.{self.bodies}: expected a per-node integer tensor [{n}], got torch.bool")
        vec = None
        if self.edge_vectors is not None:
            vec = getattr(graph, self.edge_vectors, None)
            if not torch.is_tensor(vec):
                raise ValueError(f"edge_vectors: the graph has no tensor attribute {self.edge_vectors!r}")
        ei = getattr(graph, "edge_index", None) if self.mu != 0 else None
        return self.keep([pos, ei, batch, flag, label, vec], lambda: self._build(graph, n, batch, flag, label, vec))

    def _build(self, graph, n, batch, flag, label, vec):
        from ..body_forces import WALL, BodyForces
        if batch is not None and (not torch.is_tensor(batch) or batch.numel() != n):
            raise ValueError(f"graph: graph.batch names {getattr(batch, 'numel', lambda: 0)()} nodes, graph.pos has {n}")
        mask = (flag.reshape(-1) == WALL) if self.nodes is None else (flag.reshape(-1) != 0)
        rows = torch.nonzero(mask).flatten()
        labels = None
        if batch is not None or label is not None:
            labels = torch.zeros_like(rows) if batch is None else batch.reshape(-1)[rows].long()
            if label is not None:
                own = label.reshape(-1)[rows].long()
                if own.numel():
                    lo = int(own.min())
                    labels = labels * (int(own.max()) - lo + 1) + (own - lo)
        return BodyForces(graph, nodes=rows, bodies=labels, centre=self.centre, mu=self.mu, pressure=self.pressure, velocity=self.velocity,
                          scale=self.scale, shift=self.shift, power=self.power, edge_vectors=vec)

    def _totals(self, sums):
        return torch.stack([sums[:, self.COMPONENTS[c][0]] + sums[:, self.COMPONENTS[c][1]] for c in self.components], dim=1)

    def forward(self, graph, pred, target, step=None):
        loss = self.node_term(graph, pred, target)
        on_wall = self.wall_pressure > 0 or self.wall_shear > 0
        if self.weight == 0 and not on_wall:
            return self.nothing_more(pred, loss)
        if self.weight > 0 and self.values is not None and step is None:
            raise ValueError("step: ForceLoss(values=...) needs the output step: call loss(graph, pred, target, step=t)")
        op = self.operator(graph)
        if self.weight > 0:
            if self.values is None:
                with torch.no_grad():
                    ref = self._totals(op.forces(target.detach()))
            else:
                ref = self.observed(graph, self.values, op.n_bodies, len(self.components), step,
                                    f"measured loads [{op.n_bodies}, C·T]").to(torch.float64)
            d = (self._totals(op.forces(pred)) - ref) / self.force_scale
            term = (self.weight * d.square().mean()).to(pred.dtype)
            loss = term if loss is None else loss + term
        if on_wall:
            with torch.no_grad():
                ref = op.wall(target.detach())
            d = op.wall(pred) - ref
            for w, k in ((self.wall_pressure, 0), (self.wall_shear, 1)):
                if w > 0:
                    term = w * d[:, k].square().mean()
                    loss = term if loss is None else loss + term
        return loss


class ResidualLoss(_OperatorLoss):
    """`GraphLoss(lambda_d)` plus the residual of the incompressible momentum and continuity equations the model is a surrogate
    for — a physics-informed term (new functionality — the reference has none):

        node_weight · GraphLoss(lambda_d)(graph, pred, target)
          + weight · [ mean over the counted nodes and components a of (R_a(pred) − R_a(ref))² + continuity · mean (C(pred) − C(ref))² ]

        R_a(x) = (U_a − U_a^prev) / dt + Σ_b U_b ∂_b U_a + (1 / ρ) ∂_a P − ν ∇²U_a          C(x) = Σ_a ∂_a U_a

    U = scale · x + shift is the physical field (`BodyForces`' convention: one number per field, default 1 and 0), `velocity` its
    velocity columns (default 0 .. dim − 1), `pressure` its pressure column (default: the first column that is no velocity component —
    dim, with the default velocity).  U^prev is the last input step
    `graph.field[:, −F:]` in the same units, detached — `Trainer` feeds the prediction back into it that way.  `reference="target"`
    subtracts the same expression of `target`, computed under `no_grad`: the dataset's frame spacing is not the solver's time step,
    so the truth's own discrete residual is not zero; `reference="zero"` drives the residual itself to zero.  `nu` is a number, or
    the name of a per-node graph attribute [N] or [N, 1] (1 / Re per sample: it collates along the nodes); `dt`, `rho` are numbers.
    `mask` is None or the name of a per-node attribute (non-zero: the node is counted); degenerate nodes never count.

    The derivatives are `gfd.MeshJet`'s (a quadratic fit: ∇² from a composed linear gradient does not converge): `k` its own stencil
    (default 12; 20 is the suggestion in 3-D) or None for the graph's in-edges, then with `edge_vectors` None or the name of a graph
    attribute holding the unscaled, wrapped [E, dim] vectors (a periodic mesh); `edge_vectors` together with `k` is a ValueError.
    `period` (with `k`, k <= 16): `MeshJet`'s — the stencil search and its offsets are wrapped, per graph of a batch.
    All derivatives of one tensor come from ONE `MeshJet.derived` launch in 2-D (grad u, grad v, grad p, ∇²u, ∇²v: eight columns)
    and from two in 3-D (fifteen columns); the products are torch arithmetic, and their gradients reach the model through
    `MeshJet.adjoint` (`g4c_mesh_jet_adjoint`).  No double backward.  The operator is kept (one entry) while the tensors it was
    built from are the same objects, unmodified (identity and `_version`) — `Trainer.train_epoch` calls the loss once per output
    step of the same batch; `builds` counts the operators built.  With `weight == 0` nothing is built or launched and the value is
    node_weight · GraphLoss bit for bit; `node_weight == 0` skips `GraphLoss`.  HIP device only."""

    def __init__(self, lambda_d=0, weight=1.0, node_weight=1.0, *, nu, dt, rho=1.0, velocity=None, pressure=None, scale=None, shift=None,
                 continuity=1.0, reference="target", k=12, power=2, edge_vectors=None, mask=None, period=None):
        super().__init__(lambda_d, weight, node_weight)
        from ..mesh_jet import MAX_K, PERIODIC_MAX_K
        if isinstance(nu, str):
            if not nu:
                raise ValueError(f"nu: expected a finite number >= 0 or the name of a per-node graph attribute, got {nu!r}")
        else:
            nu = _number(nu, "nu", "a finite number >= 0 (the kinematic viscosity) or the name of a per-node graph attribute")
        for name, v in (("dt", dt), ("rho", rho)):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v <= 0:
                raise ValueError(f"{name}: expected a finite number > 0, got {v!r}")
        velocity = _field_numbers(velocity, "velocity", "2 or 3 distinct field numbers", lengths=(2, 3), distinct=True)
        if pressure is not None and (isinstance(pressure, bool) or not isinstance(pressure, int) or pressure < 0
                                     or (velocity is not None and pressure in velocity)):
            raise ValueError(f"pressure: expected a field number that is no velocity component, got {pressure!r}")
        scale, shift = _per_field(scale, "scale", "number"), _per_field(shift, "shift", "number")
        self.continuity = _number(continuity, "continuity", "a finite weight >= 0")
        if reference not in ("target", "zero"):
            raise ValueError(f"reference: expected 'target' or 'zero', got {reference!r}")
        if k is not None and (isinstance(k, bool) or not isinstance(k, int) or not 5 <= k <= MAX_K):
            raise ValueError(f"k: expected None (the graph's in-edges) or an integer 5 <= k <= {MAX_K} (9 <= k in 3-D), got {k!r}")
        power = _power(power, "a stencil entry")
        _attribute(edge_vectors, "edge_vectors")
        _attribute(mask, "mask")
        if edge_vectors is not None and k is not None:
            raise ValueError("edge_vectors: they belong to the graph's edges; pass k=None with them (on a periodic mesh: the wrapped "
                             "edge_attr with k=None, or k= with period=)")
        if period is not None:
            if edge_vectors is not None or k is None:
                raise ValueError("period: it belongs to the operator's own stencil search: pass k= (<= 16) with it, and no edge_vectors")
            if k > PERIODIC_MAX_K:
                raise ValueError(f"k: the periodic search returns at most {PERIODIC_MAX_K} neighbours, got k={k!r} with period=")
            try:
                period = list(period)
            except TypeError:
                raise ValueError(f"period: expected one entry per axis (None, a length > 0 or \"auto\"), got {period!r}") from None
        self.period = period
        self.nu, self.dt, self.rho = nu, float(dt), float(rho)
        self.velocity, self.pressure, self.scale, self.shift = velocity, pressure, scale, shift
        self.reference, self.k, self.power, self.edge_vectors, self.mask = reference, k, power, edge_vectors, mask

    def operator(self, graph):
        """The `MeshJet` of `graph` — of all its graphs, when it is a batch —: the cached one while the tensors it was built from are
        the same objects, unmodified (identity and `_version`: an address says nothing, the allocator hands a freed batch's to the
        next one)."""
        from ..mesh_jet import MeshJet
        vec = None
        if self.k is not None:
            key = [getattr(graph, "pos", None), getattr(graph, "batch", None)]
        else:
            if self.edge_vectors is not None:
                vec = getattr(graph, self.edge_vectors, None)
                if not torch.is_tensor(vec):
                    raise ValueError(f"edge_vectors: the graph has no tensor attribute {self.edge_vectors!r}")
            key = [getattr(graph, "edge_index", None), getattr(graph, "pos", None) if vec is None else vec]
        return self.keep(key, lambda: MeshJet(graph, k=self.k, power=self.power, edge_vectors=vec, period=self.period))

    @staticmethod
    def _launches(names, columns, fields):
        """`names` packed greedily into launches of at most 8 columns and 4 distinct fields each."""
        from .. import _lib
        out, cur, nc, used = [], [], 0, set()
        for name, c, f in zip(names, columns, fields):
            if cur and (nc + c > _lib.DERIVED_MAX_COLS or len(used | {f}) > _lib.JET_MAX_FIELDS):
                out.append(cur)
                cur, nc, used = [], 0, set()
            cur.append(name)
            nc += c
            used.add(f)
        return out + [cur]

    def _residual(self, op, x, prev, vel, p, nu, scale, shift):
        """(R [N, dim], C [N]) of the fields x [N, F] (in the model's units)."""
        dim = op.dim
        if dim == 2:          # grad u, grad v, grad p, ∇²u, ∇²v: exactly eight columns, one launch
            fields = [vel[0], vel[1], p, vel[0], vel[1]]
            names = [f"grad:{f}" for f in fields[:3]] + [f"lap:{f}" for f in fields[3:]]
        else:                 # fifteen columns: (grad u, grad v, ∇²u, ∇²v) and (grad w, grad p, ∇²w) — two launches
            fields = [vel[0], vel[1], vel[0], vel[1], vel[2], p, vel[2]]
            names = [f"{kind}:{f}" for kind, f in zip(("grad", "grad", "lap", "lap", "grad", "grad", "lap"), fields)]
        widths = [dim if name.startswith("grad") else 1 for name in names]
        d = {}
        for group in self._launches(names, widths, fields):
            out = op.derived(x, tuple(group), field_scale=scale)          # the derivatives of the PHYSICAL fields: the shift drops out
            c0 = 0
            for name in group:
                w = widths[names.index(name)]
                d[name] = out[:, c0:c0 + w]
                c0 += w
        sc = x.new_tensor(scale)
        u = x * sc + x.new_tensor(shift)
        u_prev = prev * sc + x.new_tensor(shift)
        rows = []
        for a, fa in enumerate(vel):
            g = d[f"grad:{fa}"]
            adv = u[:, vel[0]] * g[:, 0]
            for b in range(1, dim):
                adv = adv + u[:, vel[b]] * g[:, b]
            rows.append((u[:, fa] - u_prev[:, fa]) / self.dt + adv + d[f"grad:{p}"][:, a] / self.rho - nu * d[f"lap:{fa}"][:, 0])
        cont = d[f"grad:{vel[0]}"][:, 0]
        for a in range(1, dim):
            cont = cont + d[f"grad:{vel[a]}"][:, a]
        return torch.stack(rows, dim=1), cont

    def forward(self, graph, pred, target):
        loss = self.node_term(graph, pred, target)
        if self.weight == 0:
            return self.nothing_more(pred, loss)
        op = self.operator(graph)
        n, nf, dim = op.n_nodes, int(pred.size(1)), op.dim
        vel = tuple(range(dim)) if self.velocity is None else self.velocity
        p = self.pressure if self.pressure is not None else next(f for f in range(len(vel) + 1) if f not in vel)
        if len(vel) != dim:
            raise ValueError(f"velocity: {vel!r} on a mesh of {dim} dimensions")
        if max(vel + (p,)) >= nf or p in vel:
            raise ValueError(f"pressure: the fields {vel!r} and {p} of a prediction with {nf} columns")
        for name, v in (("scale", self.scale), ("shift", self.shift)):
            if v is not None and len(v) != nf:
                raise ValueError(f"{name}: expected {nf} numbers (one per field), got {len(v)}")
        scale = [1.0] * nf if self.scale is None else self.scale
        shift = [0.0] * nf if self.shift is None else self.shift
        field = getattr(graph, "field", None)
        if not torch.is_tensor(field) or field.dim() != 2 or int(field.size(0)) != n or int(field.size(1)) < nf:
            raise ValueError(f"graph: ResidualLoss needs graph.field [{n}, >= {nf}] (its last {nf} columns are the previous step), got "
                             f"{tuple(getattr(field, 'shape', ()))}")
        prev = field[:, -nf:].detach().to(pred.dtype)
        nu = self.nu
        if isinstance(nu, str):
            nu = getattr(graph, self.nu, None)
            if not torch.is_tensor(nu) or nu.numel() != n or not nu.dtype.is_floating_point:
                raise ValueError(f"nu: graph.{self.nu}: expected a per-node floating-point tensor [{n}] or [{n}, 1], got "
                                 f"{getattr(nu, 'dtype', type(nu).__name__)} {tuple(getattr(nu, 'shape', ()))}")
            nu = nu.detach().reshape(-1).to(pred.dtype)
        counted = ~op.degenerate
        if self.mask is not None:
            m = getattr(graph, self.mask, None)
            if not torch.is_tensor(m) or m.numel() != n:
                raise ValueError(f"mask: graph.{self.mask}: expected a per-node tensor [{n}], got {tuple(getattr(m, 'shape', ()))}")
            counted = counted & (m.reshape(-1) != 0)
        r, c = self._residual(op, pred, prev, vel, p, nu, scale, shift)
        if self.reference == "target":
            with torch.no_grad():
                r0, c0 = self._residual(op, target.detach(), prev, vel, p, nu, scale, shift)
            r, c = r - r0, c - c0
        keep = counted.to(pred.dtype)
        count = keep.sum().clamp(min=1.0)
        term = (r.square() * keep[:, None]).sum() / (count * dim)
        if self.continuity > 0:
            term = term + self.continuity * ((c.square() * keep).sum() / count)
        term = self.weight * term
        return term if loss is None else loss + term


class IntegralLoss(_OperatorLoss):
    """`GraphLoss(lambda_d)` plus errors of integrals over the domain — the node rows weighted by their control volumes
    (`gfd.ControlVolumes`: the Voronoi areas of the cloud), so that a refined wake or boundary layer counts by the area it covers
    and not by its node count (new functionality — the reference has none):

        node_weight · GraphLoss(lambda_d)(graph, pred, target) + weight · Σ_name terms[name] · T_name

    Every T_name is the mean over the graphs of the batch of a per-graph value; V is the graph's ∫1, p and t the prediction and
    the target, nf their columns:

        'mse'       Σ_f ∫(p_f − t_f)² / (nf · V)       the area-weighted MSE: `F.mse_loss` when all areas are equal
        'mse:<f>'   ∫(p_f − t_f)² / V                  the same for one field
        'rel_mse'   Σ_f ∫(p_f − t_f)² / Σ_f ∫t_f²      the square of the rollout's 'rel_l2' (no root: smooth at 0)
        'int:<f>', 'ke', 'circulation', 'enstrophy', 'div2'      ((I(p) − I(t)) / V)²

    with I the rollout's integral of that name (`Rollout(integrals=)`: ∫p_f, ½∫(u² + v²) over `velocity`, ∫ω, ½∫ω², ∫(∇·u)²) —
    the conserved quantities whose drift a rollout reports afterwards.  Dividing by V makes the matching terms intensive: no free
    scale, and safe where the target's own integral is zero.  `terms`: a dict (or a sequence of pairs) of names to weights >= 0.

    'circulation', 'enstrophy' and 'div2' read the 'vort' / 'div' columns of `MeshGradient.derived(pred, ...)` (`power`,
    `edge_vectors` as in `FlowLoss`): that call is recorded, so their gradient chains into `MeshGradient.adjoint`.  Every integral
    is one `ControlVolumes.integrate(..., per_graph=True)` — recorded for the prediction (`g4c_weighted_integrals_adjoint` in the
    backward), under `no_grad` for the target; the few numbers behind them are combined in fp64 torch on the device (nothing is
    read back, nothing synchronises) and the term is cast to the prediction's dtype before it joins the node term.

    `box`, `bodies` (None or True: the wall from `graph.bound == 4`) are `ControlVolumes`'; `normals` is None or the name of a
    per-node graph attribute [N, 2] holding the outward wall normals (zero rows: no wall; it collates along the nodes).  The
    volumes — and the `MeshGradient` when a term needs it — are kept (one entry) while `graph.pos`, `graph.batch`, the normals
    and the edge tensors are the same tensor objects, unmodified; `builds` counts the builds.  `node_weight == 0` skips `GraphLoss`;
    `weight == 0` or no term of non-zero weight builds and launches nothing.  2-D, HIP device only."""

    MATCHING = ("ke", "circulation", "enstrophy", "div2")
    MAX_ENTRIES = 8          # _lib.INTEGRALS_MAX_ENTRIES: what one launch over a source sums (checked without the library)

    def __init__(self, lambda_d=0, weight=1.0, node_weight=1.0, *, terms, velocity=(0, 1), box=None, bodies=None, normals=None, power=2,
                 edge_vectors=None):
        super().__init__(lambda_d, weight, node_weight)
        pairs = list(terms.items()) if isinstance(terms, dict) else terms
        try:
            pairs = [tuple(p) for p in pairs]
        except TypeError:
            pairs = None
        if not pairs or any(len(p) != 2 for p in pairs):
            raise ValueError(f"terms: expected a non-empty dict of names ('mse', 'mse:<f>', 'rel_mse', 'int:<f>', 'ke', 'circulation', "
                             f"'enstrophy', 'div2') to weights, got {terms!r}")
        seen, self.terms = set(), []
        for name, w in pairs:
            key = self._name(name)
            if key in seen:
                raise ValueError(f"terms: {name!r} is named twice")
            seen.add(key)
            self.terms.append((key, _number(w, f"terms[{name!r}]", "a finite weight >= 0")))
        velocity = _field_numbers(velocity, "velocity", "2 distinct field numbers", lengths=(2,), distinct=True)
        if velocity is None:
            raise ValueError("velocity: expected 2 distinct field numbers, got None")
        if bodies is not None and bodies is not True:
            raise TypeError(f"bodies: expected None or True (the wall from graph.bound == 4), got {type(bodies).__name__}")
        _attribute(normals, "normals", "a per-node graph attribute holding [N, 2] wall normals")
        if normals is not None and bodies is not None:
            raise ValueError("normals: given together with bodies= (the bodies carry their own)")
        if box is not None:
            try:
                rows = box.tolist() if torch.is_tensor(box) else list(box)
                flat = [float(v) for r in rows for v in (r if isinstance(r, (list, tuple)) else [r])]
            except (TypeError, ValueError):
                flat = None
            if not flat or len(flat) % 4 or not all(math.isfinite(v) for v in flat):
                raise ValueError(f"box: expected (lo_x, lo_y, hi_x, hi_y), or one such box per graph of the batch, got {box!r}")
        self.power = _power(power, "an edge")
        _attribute(edge_vectors, "edge_vectors", "a graph attribute holding [E, 2] vectors")
        self.velocity, self.box, self.bodies, self.normals, self.edge_vectors = velocity, box, bodies, normals, edge_vectors
        self._live = [(n, w) for n, w in self.terms if w > 0]
        self._derived = tuple(c for c in ("vort", "div") if any(self._column(n) == c for n, _ in self._live))

    @staticmethod
    def _name(name):
        """`name` in its canonical form ('mse:01' is 'mse:1'), or ValueError naming `terms`."""
        if isinstance(name, str):
            if name in ("mse", "rel_mse") + IntegralLoss.MATCHING:
                return name
            head, _, tail = name.partition(":")
            if head in ("mse", "int") and tail.isdigit():
                return f"{head}:{int(tail)}"
        raise ValueError(f"terms: unknown name {name!r} ('mse', 'mse:<f>', 'rel_mse', 'int:<f>', 'ke', 'circulation', 'enstrophy' and "
                         f"'div2' are known)")

    @staticmethod
    def _column(name):
        return {"circulation": "vort", "enstrophy": "vort", "div2": "div"}.get(name)

    def plan(self, nf: int):
        """Per source — 'error' (pred − target), 'target', 'fields' (pred, and target again), 'derived' — its entries, and per live term
        (name, weight, kind, slots): `kind` 'mse' (Σ slots / (count · V)), 'rel' (Σ error slots / Σ target slots) or 'match' with a
        factor (((factor · Σ slots)(pred) − (same)(target)) / V)².  ValueError naming `terms` / `velocity` on a field that the
        prediction does not have or more than 8 entries over one source."""
        if max(self.velocity) >= nf:
            raise ValueError(f"velocity: the fields {self.velocity!r} of a prediction with {nf} columns")
        entries = {"error": [], "target": [], "fields": [], "derived": []}

        def slot(src, a, b=-1):
            if (a, b) not in entries[src]:
                entries[src].append((a, b))
            return entries[src].index((a, b))

        def field(name):
            f = int(name.split(":")[1])
            if f >= nf:
                raise ValueError(f"terms: {name!r}: field {f} of a prediction with {nf} columns")
            return f

        recipes = []
        for name, w in self._live:
            if name == "mse":
                recipes.append((name, w, "mse", [slot("error", f, f) for f in range(nf)]))
            elif name.startswith("mse:"):
                recipes.append((name, w, "mse", [slot("error", field(name), field(name))]))
            elif name == "rel_mse":
                recipes.append((name, w, "rel", ([slot("error", f, f) for f in range(nf)], [slot("target", f, f) for f in range(nf)])))
            elif name.startswith("int:"):
                recipes.append((name, w, ("fields", 1.0), [slot("fields", field(name))]))
            elif name == "ke":
                recipes.append((name, w, ("fields", 0.5), [slot("fields", v, v) for v in self.velocity]))
            else:
                c = self._derived.index(self._column(name))
                recipes.append((name, w, ("derived", 0.5 if name == "enstrophy" else 1.0),
                                [slot("derived", c, -1 if name == "circulation" else c)]))
        for src, e in entries.items():
            if len(e) > self.MAX_ENTRIES:
                raise ValueError(f"terms: they need {len(e)} sums over the {src} source, at most {self.MAX_ENTRIES} fit one launch")
        return entries, recipes

    def _graph(self, graph, pred):
        pos = getattr(graph, "pos", None)
        if not torch.is_tensor(pos) or pos.dim() != 2:
            raise ValueError("graph: IntegralLoss needs graph.pos [N, 2]")
        if int(pos.size(1)) != 2:
            raise ValueError(f"graph: IntegralLoss is 2-D only, graph.pos is {tuple(pos.shape)} (3-D cells are out of scope)")
        if pos.device.type != "cuda" or pred.device.type != "cuda":
            raise ValueError(f"graph: IntegralLoss runs on a HIP device only, graph.pos is on '{pos.device}' and the prediction on "
                             f"'{pred.device}' (there is no CPU fallback)")
        return pos

    def operators(self, graph):
        """(the `ControlVolumes` of `graph` — of all its graphs, when it is a batch —, V float64 [G] their ∫1, the `MeshGradient` the
        derived terms read or None): the cached ones while graph.pos, graph.batch, the normals, graph.bound (with `bodies`) and — when
        a derived term is live — graph.edge_index and the edge vectors are the objects they were built from, unmodified."""
        pos, batch = graph.pos, getattr(graph, "batch", None)
        nrm = None
        if self.normals is not None:
            nrm = getattr(graph, self.normals, None)
            if not torch.is_tensor(nrm):
                raise ValueError(f"normals: the graph has no tensor attribute {self.normals!r}")
        bound = getattr(graph, "bound", None) if self.bodies else None
        ei = vec = None
        if self._derived:
            ei = getattr(graph, "edge_index", None)
            if self.edge_vectors is not None:
                vec = getattr(graph, self.edge_vectors, None)
                if not torch.is_tensor(vec):
                    raise ValueError(f"edge_vectors: the graph has no tensor attribute {self.edge_vectors!r}")

        def build():
            from ..control_volumes import ControlVolumes
            from ..mesh_gradient import MeshGradient
            cv = ControlVolumes(graph, box=self.box, bodies=self.bodies, normals=nrm)
            one = torch.zeros((cv.n_nodes, 1), dtype=torch.float32, device=cv.area.device)          # (the entry (−1, −1) reads no column)
            V = cv.integrate(one, [(-1, -1)], per_graph=True)[:, 0]
            return cv, V, (MeshGradient(graph, power=self.power, edge_vectors=vec) if self._derived else None)

        return self.keep([pos, batch, nrm, bound, ei, vec], build)

    def integrals(self, graph, pred, target):
        """(V [G], sums, recipes): `sums` maps 'error', 'target', 'fields', 'fields_target', 'derived', 'derived_target' to the float64
        [G, ne] integrals the live terms need (absent: not needed) — each `ControlVolumes.integrate(..., per_graph=True)` of
        `plan(nf)`'s entries; those of the prediction are recorded for autograd."""
        entries, recipes = self.plan(int(pred.size(1)))
        cv, V, op = self.operators(graph)
        tgt = target.detach()
        sums = {}
        if entries["error"]:
            sums["error"] = cv.integrate(pred, entries["error"], sub=tgt, per_graph=True)
        if entries["fields"]:
            sums["fields"] = cv.integrate(pred, entries["fields"], per_graph=True)
        if entries["derived"]:
            sums["derived"] = cv.integrate(op.derived(pred, self._derived, velocity=self.velocity), entries["derived"], per_graph=True)
        with torch.no_grad():
            if entries["target"]:
                sums["target"] = cv.integrate(tgt, entries["target"], per_graph=True)
            if entries["fields"]:
                sums["fields_target"] = cv.integrate(tgt, entries["fields"], per_graph=True)
            if entries["derived"]:
                sums["derived_target"] = cv.integrate(op.derived(tgt, self._derived, velocity=self.velocity), entries["derived"], per_graph=True)
        return V, sums, recipes

    @staticmethod
    def _add(s, slots):
        out = s[:, slots[0]]
        for j in slots[1:]:          # (a fixed order: one add after the other)
            out = out + s[:, j]
        return out

    def forward(self, graph, pred, target):
        loss = self.node_term(graph, pred, target)
        if self.weight == 0 or not self._live:
            return self.nothing_more(pred, loss)
        self.plan(int(pred.size(1)))          # (the terms against the prediction's columns first: refused the same way without a device)
        self._graph(graph, pred)
        V, sums, recipes = self.integrals(graph, pred, target)
        total = None
        for name, w, kind, slots in recipes:
            if kind == "mse":
                value = self._add(sums["error"], slots) / (len(slots) * V)
            elif kind == "rel":
                value = self._add(sums["error"], slots[0]) / self._add(sums["target"], slots[1])
            else:
                src, factor = kind
                ip, it = self._add(sums[src], slots), self._add(sums[src + "_target"], slots)
                if factor != 1.0:
                    ip, it = factor * ip, factor * it
                value = ((ip - it) / V).square()
            part = w * value.mean()
            total = part if total is None else total + part
        if self.weight != 1.0:
            total = self.weight * total
        term = total.to(pred.dtype)
        return term if loss is None else loss + term
