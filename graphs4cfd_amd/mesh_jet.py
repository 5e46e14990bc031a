"""First and second derivatives on the mesh (new functionality — the reference has none): a weighted least-squares fit of a
QUADRATIC through the node's own value, over the graph's in-edges or over a wider stencil of the operator's own.

`MeshGradient` fits a plane: its error is O(h)·f″, and differentiating its output once more (the divergence of `grad:<f>`) leaves
an O(1) error — a composed Laplacian does not converge.  Here, at node i with stencil entries s (sender j_s, d_s = pos[j_s] − pos[i]),
the jet J = (∂_a x, ∂_a∂_b x) — Q = dim + dim (dim + 1) / 2 numbers: 5 in 2-D, 9 in 3-D — minimises
Σ_s w_s (x[j_s] − x[i] − Σ_a J_a d_a − ½ Σ_ab J_ab d_a d_b)², w_s = |d_s|^(−power):  J(i) = Σ_s c_s (x[j_s] − x[i]).  The fit is exact on
quadratics; second derivatives converge at first order, first derivatives at second order.  The rows c_s are built once per mesh on
the device in fp64 by a Cholesky factorisation of the unit-diagonal-scaled normal matrix (`g4c_mesh_jet_weights`,
csrc/mesh_jet.hip); every application is one memory-bound launch (`g4c_mesh_jet`): one thread per node, fp32, its entries in CSR
order, so the bits are a function of the data alone.  A node whose stencil does not determine the fit (fewer than Q entries,
collinear / coplanar neighbours, a zero-length vector) is `degenerate`: its derivatives are 0.

Out of scope: rollout records of the jet (no step index, snapshots or statistics), `DistributedRollout`, double backward, gradients
with respect to the mesh, a periodic search for the operator's own stencil."""
from __future__ import annotations

from types import SimpleNamespace
from typing import List, Optional, Tuple

import torch

from . import _lib, ops, plan
from .mesh_gradient import AXES, _names, _StencilOperator, check_mesh, derived_columns, derived_terms

MAX_COLUMNS = _lib.DERIVED_MAX_COLS
MAX_K = 32
KNOWN = "'div', 'vort', 'grad:<field>', 'lap:<field>' and 'hess:<field>'"


def second_axes(dim: int) -> List[Tuple[int, int]]:
    """The pairs (a, b), a <= b, in the order of the second derivatives: derivative number dim + their place."""
    return [(a, b) for a in range(dim) for b in range(a, dim)]


def _field_of(name: str, head: str) -> Optional[int]:
    if not name.startswith(head):
        return None
    tail = name[len(head):]
    if not tail.isdigit():
        raise ValueError(f"derived: {name!r}: expected '{head}<field>' with a field number")
    return int(tail)


def jet_columns(names, dim: int) -> List[str]:
    """The labels of the columns `names` produce: those of `MeshGradient` for 'div', 'vort' and 'grad:<f>'; 'lap<f>' for 'lap:<f>';
    'd2<f>/dxx', 'd2<f>/dxy', .. for 'hess:<f>'.  ValueError on an unknown name or more than 8 columns."""
    out = []
    for name in _names(names):
        if _field_of(name, "lap:") is not None:
            out.append(f"lap{_field_of(name, 'lap:')}")
        elif _field_of(name, "hess:") is not None:
            out += [f"d2{_field_of(name, 'hess:')}/d{AXES[a]}{AXES[b]}" for a, b in second_axes(dim)]
        elif name in ("div", "vort") or name.startswith("grad:"):
            out += derived_columns((name,), dim)
        else:
            raise ValueError(f"derived: unknown name {name!r} ({KNOWN} are known)")
    if len(out) > MAX_COLUMNS:
        raise ValueError(f"derived: {names!r} make {len(out)} columns, at most {MAX_COLUMNS} fit one launch")
    return out


def jet_terms(names, dim: int, nf: int, velocity=None, field_scale=None) -> List[List[Tuple[int, int, float]]]:
    """The program of `ops.mesh_jet` for `names` over nf fields: per column its terms (field, derivative, coef), derivative
    0 .. dim − 1 a first one and dim .. Q − 1 a second one.  `velocity`, `field_scale` as in `mesh_gradient.derived_terms`."""
    jet_columns(names, dim)
    if dim not in (2, 3):
        raise ValueError(f"derived: a mesh of {dim} dimensions (2 or 3)")
    derived_terms(("grad:0",), dim, nf, velocity, field_scale)          # (checks velocity and field_scale whatever the names)
    pairs = second_axes(dim)
    prog = []
    for name in _names(names):
        f = _field_of(name, "lap:")
        g = _field_of(name, "hess:") if f is None else None
        if f is None and g is None:
            prog += derived_terms((name,), dim, nf, velocity, field_scale)
            continue
        field = f if f is not None else g
        if field >= nf:
            raise ValueError(f"derived: {name!r}: field {field} of {nf}")
        coef = derived_terms((f"grad:{field}",), dim, nf, velocity, field_scale)[0][0][2]          # the field's scale as float32
        if f is not None:
            prog.append([(field, dim + pairs.index((a, a)), coef) for a in range(dim)])
        else:
            prog += [[(field, dim + q, coef)] for q in range(len(pairs))]
    return prog


def check_stencil(graph, k, power, edge_vectors, period=None) -> int:
    """The arguments of `MeshJet` on the tensors as they were passed (nothing is moved, the library is not touched): the mesh's
    dimension, or ValueError naming the argument."""
    if period is not None:
        if edge_vectors is not None:
            raise ValueError("period: it belongs to the operator's own search (k=); edge_vectors belong to the graph's edges — on a "
                             "periodic mesh pass the wrapped edge_attr OR k= with period=")
        if k is None:
            raise ValueError("period: with k=None the stencil is the graph's in-edges and nothing is searched; pass k= (<= 16) with "
                             "period=, or the wrapped edge_attr as edge_vectors")
        if isinstance(k, int) and not isinstance(k, bool) and k > PERIODIC_MAX_K:
            raise ValueError(f"k: the periodic search returns at most {PERIODIC_MAX_K} neighbours, got k={k!r} with period=")
    if k is None:
        try:
            return check_mesh(graph, power, edge_vectors)
        except ValueError as e:          # (the same rules, under this operator's name)
            raise ValueError(str(e).replace("MeshGradient", "MeshJet")) from None
    if isinstance(power, bool) or not isinstance(power, int) or power not in (0, 1, 2):
        raise ValueError(f"power: expected 0, 1 or 2 (a stencil entry weighs |d|^-power), got {power!r}")
    if edge_vectors is not None:
        raise ValueError("edge_vectors: they belong to the graph's edges; with k= the operator searches a stencil of its own over "
                         "graph.pos — pass one of the two")
    pos = getattr(graph, "pos", None)
    if not torch.is_tensor(pos) or pos.dim() != 2 or int(pos.size(1)) not in (2, 3) or not pos.dtype.is_floating_point:
        raise ValueError("graph: MeshJet(k=) needs graph.pos [N, 2] or [N, 3]")
    dim = int(pos.size(1))
    Q = ops.jet_size(dim)
    if isinstance(k, bool) or not isinstance(k, int) or not Q <= k <= MAX_K:
        raise ValueError(f"k: expected None (the graph's in-edges) or an integer {Q} <= k <= {MAX_K} on a {dim}-D mesh, got {k!r}")
    if period is not None:
        from .synthetic import check_period
        check_period(period, dim, "MeshJet")
    return dim


PERIODIC_MAX_K = 16          # the periodic search's limit (g4c_knn_grid_periodic)


class MeshJet(_StencilOperator):
    """The quadratic least-squares fit over a stencil of `graph` (a Graph on the GPU), built once; `power` 0, 1 or 2 weighs a stencil
    entry by |d|^(−power).

    `k=None`: the stencil is the graph's in-edges (`edge_index` [2, E], row = sender, col = receiver); `edge_vectors` [E, dim] as in
    `MeshGradient` — on a PERIODIC mesh pass the wrapped, unscaled `edge_attr`.  Mind the conditioning: a k = 6 graph in 2-D gives 6
    rows for 5 unknowns — most of its nodes are not degenerate but are badly conditioned (scaled pivots down to 1e-5 on a random
    cloud, against 1e-2 with 12 neighbours), and their second derivatives are noisy.
    `k=int`: the stencil is the k nearest other nodes of `graph.pos` (`knn_neighbours_device`), Q <= k <= 32, searched per graph of
    `graph.batch` when the graph is a collated batch (graphs of a batch overlap in space).  `edge_vectors` together with `k` is a
    ValueError.  Suggested: k = 12 in 2-D, 20 in 3-D (2 Q + 2; not tuned).
    `period` (with `k=int`, k <= 16; one entry per axis: None, a length >= the extent, or "auto", the extent — as `connect_knn`'s):
    the stencil is searched in the wrapped metric (`knn_neighbours_device(period=)`) and its offsets are wrapped, so a node at the
    seam of a periodic mesh gets a two-sided stencil.  In a batch each graph is searched from its own origin, with its own "auto"
    extent.  `period` with `k=None` or `edge_vectors` is a ValueError.

    `derived(x, names)` [N, nd] with the names of `MeshGradient` — 'div', 'vort', 'grad:<f>', here from the quadratic fit's first
    derivatives — and 'lap:<f>' (one column, Σ_a ∂_a∂_a) and 'hess:<f>' (Q − dim columns: xx, xy, yy or xx, xy, xz, yy, yz, zz);
    `columns(names)` their labels; `degenerate` bool [N].  At most 8 columns and 4 distinct fields per call.

    `derived` of an x that requires grad is recorded for autograd: its backward is `adjoint(gy, names, nf)` [N, nf], the transpose
    of the same linear map (`g4c_mesh_jet_adjoint`; the rows c are constants: no gradient reaches the mesh, and there is no double
    backward).  The sender-side tables the adjoint walks are built on its first use.  HIP device only."""

    def __init__(self, graph, k: Optional[int] = None, power: int = 2, edge_vectors: Optional[torch.Tensor] = None, period=None):
        self.dim = check_stencil(graph, k, power, edge_vectors, period)
        self.k, self.power = k, power
        self.n_nodes = int(graph.num_nodes)
        if k is None:
            ei = graph.edge_index
            if ei.device.type != "cuda":
                raise ValueError(f"graph: MeshJet runs on a HIP device only, graph.edge_index is on '{ei.device}' (there is no CPU fallback)")
            if edge_vectors is None:
                pos = graph.pos.to(ei.device)
                edge_vectors = pos[ei[1]] - pos[ei[0]]
            rel = edge_vectors.detach().to(torch.float32).contiguous()
            ep, csr = plan.edge_csr(ei, self.n_nodes)
            src32 = ep.row
            self.max_deg = csr.max_deg
        else:
            pos = graph.pos
            if pos.device.type != "cuda":
                raise ValueError(f"graph: MeshJet runs on a HIP device only, graph.pos is on '{pos.device}' (there is no CPU fallback)")
            csr, src32, rel = self._own_stencil(pos.detach().to(torch.float32), getattr(graph, "batch", None), k, period)
            self.max_deg = k
        self.off = csr.off
        self.c, self.src, degenerate = ops.mesh_jet_weights(rel, csr, src32, power)
        self.degenerate = degenerate.bool()
        self._adjoint_tables = None

    @staticmethod
    def _own_stencil(pos, batch, k, period=None):
        """(csr, src32 [N·k], rel [N·k, dim]): the k nearest other nodes of every node within its own graph, nearest first.  With
        `period`: in the wrapped metric of each graph's own frame, rel the fp32 rounding of the search's wrapped fp64 offset."""
        from .synthetic import check_period, knn_neighbours_device, periodic_frame
        per = check_period(period, int(pos.size(1)), "MeshJet")
        n = int(pos.size(0))
        if batch is None:
            counts = [n]
        else:
            if not torch.is_tensor(batch) or batch.numel() != n:
                raise ValueError(f"graph: graph.batch names {getattr(batch, 'numel', lambda: 0)()} nodes, graph.pos has {n}")
            counts = torch.bincount(batch.reshape(-1)).tolist()
        if min(counts) <= k:
            raise ValueError(f"k: {k} neighbours of a graph with {min(counts)} nodes (a node's stencil holds k OTHER nodes)")
        nbr, a = torch.empty((n, k), dtype=torch.long, device=pos.device), 0
        lengths = None if per is None else torch.zeros((n, int(pos.size(1))), dtype=torch.float32, device=pos.device)
        for c in counts:          # (contiguous ranges: `collate` numbers the nodes graph after graph)
            own = pos[a:a + c].contiguous()
            if per is None:
                knn_neighbours_device(own, k, out=nbr[a:a + c])
            else:
                L = periodic_frame(own, per, "MeshJet")[1]
                knn_neighbours_device(own, k, out=nbr[a:a + c], period=[v or None for v in L])
                lengths[a:a + c] = torch.tensor(L, dtype=torch.float32, device=pos.device)
            nbr[a:a + c] += a
            a += c
        src = nbr.reshape(-1)
        rel = (pos.repeat_interleave(k, dim=0) - pos[src]).contiguous()
        if per is not None:
            # the search's own rule on the fp64 difference (strict, applied once; a length 0: not periodic), so rel is the image
            # the search ranked; rounded to fp32 once — where nothing wraps that IS the fp32 difference above
            L = lengths.repeat_interleave(k, dim=0).double()
            d = pos.double().repeat_interleave(k, dim=0) - pos.double()[src]
            d = torch.where((L > 0) & (d > 0.5 * L), d - L, torch.where((L > 0) & (d < -0.5 * L), d + L, d))
            rel = d.to(torch.float32).contiguous()
        off = torch.arange(0, n * k + 1, k, dtype=torch.int32, device=pos.device)
        return SimpleNamespace(off=off, perm=None, n=n * k), src.to(torch.int32), rel

    _table, _order = "c", 2
    _columns, _terms, _adjoint_op = staticmethod(jet_columns), staticmethod(jet_terms), staticmethod(ops.mesh_jet_adjoint)

    def _launch(self, x: torch.Tensor, prog) -> torch.Tensor:
        return ops.mesh_jet(x, self.off, self.c, self.src, prog)

    def __repr__(self):
        stencil = "in-edges" if self.k is None else f"k={self.k}"
        return f"MeshJet(nodes={self.n_nodes}, entries={int(self.src.numel())}, dim={self.dim}, {stencil}, power={self.power})"
