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


class FlowLoss(nn.Module):
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
        super().__init__()
        self.lambda_d = _number(lambda_d, "lambda_d")
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
        if isinstance(power, bool) or not isinstance(power, int) or power not in (0, 1, 2):
            raise ValueError(f"power: expected 0, 1 or 2 (an edge weighs |d|^-power), got {power!r}")
        if velocity is not None:
            try:
                velocity = tuple(velocity)
            except TypeError:
                raise ValueError(f"velocity: expected 2 or 3 field numbers, got {velocity!r}") from None
            if len(velocity) not in (2, 3) or any(isinstance(v, bool) or not isinstance(v, int) or v < 0 for v in velocity):
                raise ValueError(f"velocity: expected 2 or 3 field numbers, got {velocity!r}")
        if field_scale is not None:
            try:
                field_scale = [float(v) for v in (field_scale.tolist() if torch.is_tensor(field_scale) else field_scale)]
            except (TypeError, ValueError):
                raise ValueError(f"field_scale: expected one factor per field, got {field_scale!r}") from None
            if not field_scale or not all(math.isfinite(v) for v in field_scale):
                raise ValueError(f"field_scale: expected one finite factor per field, got {field_scale!r}")
        if edge_vectors is not None and (not isinstance(edge_vectors, str) or not edge_vectors):
            raise ValueError(f"edge_vectors: expected None or the name of a graph attribute holding [E, dim] vectors, got {edge_vectors!r}")
        self.base = GraphLoss(lambda_d)
        live = [(name, float(w)) for name, w in terms.items() if w > 0]
        self.terms = dict(terms)
        self.zero = zero
        self._on_error = [(n, w) for n, w in live if n not in zero]          # D(pred − target)
        self._on_pred = [(n, w) for n, w in live if n in zero]               # D(pred)
        self.power, self.velocity, self.field_scale, self.edge_vectors = power, velocity, field_scale, edge_vectors
        self._cache = None          # (edge_index, its version, the vectors / pos tensor, its version, MeshGradient)
        self.builds = 0             # operators built so far (a batch seen again costs none)

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
        hit = self._cache
        if (hit is not None and hit[0] is ei and hit[2] is vec and torch.is_tensor(ei) and torch.is_tensor(vec) and hit[1] == ei._version
                and hit[3] == vec._version):
            return hit[4]
        op = MeshGradient(graph, power=self.power, edge_vectors=None if self.edge_vectors is None else vec)
        self._cache = (ei, ei._version, vec, vec._version, op)
        self.builds += 1
        return op

    def forward(self, graph, pred, target):
        loss = self.base(graph, pred, target)
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
