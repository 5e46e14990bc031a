"""A spatial differential operator on the mesh (new functionality — the reference has none): the least-squares gradient over the kNN
edges a Graph already carries, and the flow diagnostics built on it — divergence, vorticity, gradients of single fields.

At node i with in-edges e (sender j_e, d_e = pos[j_e] − pos[i]), the gradient of a field x is the ∇ that minimises
Σ_e w_e (x[j_e] − x[i] − ∇·d_e)², w_e = |d_e|^(−power):  ∇x(i) = Σ_e g_e (x[j_e] − x[i])  with  g_e = w_e M⁻¹ d_e,  M = Σ_e w_e d_e d_eᵀ
— exact on linear fields, whatever the weights.  The vectors g_e are built once per mesh on the device in fp64
(`g4c_mesh_gradient_weights`, csrc/mesh_gradient.hip); every application is one memory-bound launch (`g4c_mesh_derived`): one thread
per node, fp32, its in-edges in CSR order, so the bits are a function of the data alone.  A node whose neighbours do not span the
space (fewer than `dim` in-edges, collinear / coplanar neighbours, a zero-length edge) is `degenerate`: its derivatives are 0."""
from __future__ import annotations

from typing import List, Optional, Tuple

import torch

from . import _lib, ops, plan

AXES = "xyz"
MAX_COLUMNS = _lib.DERIVED_MAX_COLS


def _names(names) -> Tuple[str, ...]:
    if isinstance(names, str):
        names = (names,)
    try:
        names = tuple(names)
    except TypeError:
        raise ValueError(f"derived: expected a tuple of names ('div', 'vort', 'grad:<field>'), got {names!r}") from None
    if not names or not all(isinstance(n, str) for n in names):
        raise ValueError(f"derived: expected a non-empty tuple of names ('div', 'vort', 'grad:<field>'), got {names!r}")
    return names


def _grad_field(name: str) -> Optional[int]:
    if not name.startswith("grad:"):
        return None
    tail = name[5:]
    if not tail.isdigit():
        raise ValueError(f"derived: {name!r}: expected 'grad:<field>' with a field number")
    return int(tail)


def derived_columns(names, dim: int) -> List[str]:
    """The labels of the columns `names` produce on a mesh of `dim` dimensions: 'div'; 'vort' (2-D: ∂₀v − ∂₁u) or 'vort_x', 'vort_y',
    'vort_z'; 'd<f>/dx', 'd<f>/dy' (, 'd<f>/dz') for 'grad:<f>'.  ValueError on an unknown name or more than 8 columns."""
    out = []
    for name in _names(names):
        if name == "div":
            out.append("div")
        elif name == "vort":
            out += ["vort"] if dim == 2 else [f"vort_{a}" for a in AXES]
        elif _grad_field(name) is not None:
            out += [f"d{_grad_field(name)}/d{AXES[a]}" for a in range(dim)]
        else:
            raise ValueError(f"derived: unknown name {name!r} ('div', 'vort' and 'grad:<field>' are known)")
    if len(out) > MAX_COLUMNS:
        raise ValueError(f"derived: {names!r} make {len(out)} columns, at most {MAX_COLUMNS} fit one launch")
    return out


def derived_terms(names, dim: int, nf: int, velocity=None, field_scale=None) -> List[List[Tuple[int, int, float]]]:
    """The program of `ops.mesh_derived` for `names` over nf fields: per column its terms (field, axis, coef).  `velocity`: the fields
    holding the velocity components (default 0 .. dim − 1); `field_scale` [nf]: multiplied into the coefficients (as float32)."""
    derived_columns(names, dim)
    if dim not in (2, 3):
        raise ValueError(f"derived: a mesh of {dim} dimensions (2 or 3)")
    if velocity is None:
        velocity = tuple(range(dim))
    else:
        try:
            velocity = tuple(velocity)
        except TypeError:
            raise ValueError(f"velocity: expected {dim} field numbers, got {velocity!r}") from None
        if len(velocity) != dim or any(isinstance(v, bool) or not isinstance(v, int) or v < 0 for v in velocity):
            raise ValueError(f"velocity: expected {dim} field numbers, got {velocity!r}")
    if field_scale is None:
        scale = [1.0] * nf
    else:
        scale = [float(v) for v in (field_scale.tolist() if torch.is_tensor(field_scale) else field_scale)]
        if len(scale) != nf:
            raise ValueError(f"field_scale: expected {nf} factors (one per field), got {len(scale)}")

    def term(field, axis, sign=1.0):
        return (field, axis, float(torch.tensor(sign * scale[field], dtype=torch.float32)))

    def need_velocity(name):
        if max(velocity) >= nf:
            raise ValueError(f"derived: {name!r} needs the velocity fields {velocity}, the model has {nf} field(s)")

    prog = []
    for name in _names(names):
        if name == "div":
            need_velocity(name)
            prog.append([term(velocity[a], a) for a in range(dim)])
        elif name == "vort":
            need_velocity(name)
            if dim == 2:
                prog.append([term(velocity[1], 0), term(velocity[0], 1, -1.0)])
            else:
                u, v, w = velocity
                prog += [[term(w, 1), term(v, 2, -1.0)], [term(u, 2), term(w, 0, -1.0)], [term(v, 0), term(u, 1, -1.0)]]
        else:
            f = _grad_field(name)
            if f >= nf:
                raise ValueError(f"derived: {name!r}: field {f} of {nf}")
            prog += [[term(f, a)] for a in range(dim)]
    return prog


def check_mesh(graph, power, edge_vectors) -> int:
    """The arguments of `MeshGradient` on the tensors as they were passed (nothing is moved, the library is not touched): the mesh's
    dimension, or ValueError naming the argument."""
    if isinstance(power, bool) or not isinstance(power, int) or power not in (0, 1, 2):
        raise ValueError(f"power: expected 0, 1 or 2 (an edge weighs |d|^-power), got {power!r}")
    ei = getattr(graph, "edge_index", None)
    if not torch.is_tensor(ei) or ei.dim() != 2 or int(ei.size(0)) != 2 or ei.dtype.is_floating_point:
        raise ValueError("graph: MeshGradient needs graph.edge_index, an integer tensor [2, E]")
    if edge_vectors is None:
        pos = getattr(graph, "pos", None)
        if not torch.is_tensor(pos) or pos.dim() != 2 or int(pos.size(1)) not in (2, 3) or not pos.dtype.is_floating_point:
            raise ValueError("graph: MeshGradient needs graph.pos [N, 2] or [N, 3] (or edge_vectors=)")
        return int(pos.size(1))
    if not torch.is_tensor(edge_vectors) or not edge_vectors.dtype.is_floating_point:
        raise ValueError(f"edge_vectors: expected a floating-point tensor [E, dim], got {getattr(edge_vectors, 'dtype', type(edge_vectors).__name__)}")
    if edge_vectors.dim() != 2 or int(edge_vectors.size(0)) != int(ei.size(1)) or int(edge_vectors.size(1)) not in (2, 3):
        raise ValueError(f"edge_vectors: expected [E = {int(ei.size(1))}, 2 or 3], got {tuple(edge_vectors.shape)}")
    if edge_vectors.device != ei.device:
        raise ValueError(f"edge_vectors: on '{edge_vectors.device}', graph.edge_index is on '{ei.device}'")
    return int(edge_vectors.size(1))


class _StencilOperator:
    """What `MeshGradient` and `MeshJet` share: a table of fp32 rows per stencil entry in CSR order (`off`, `src`, and the table under
    the attribute `_table` names — read at every call), applied by one launch per call and transposed by one launch in the backward.
    A subclass names its table and supplies `_columns` / `_terms` (names -> labels / program terms), `_order` (`ops.derived_program`),
    `_launch` (the plain forward) and `_adjoint_op` (the `ops` function of the transpose)."""

    _table = _columns = _terms = _order = _adjoint_op = None

    def _launch(self, x: torch.Tensor, prog) -> torch.Tensor:
        raise NotImplementedError

    def columns(self, names) -> List[str]:
        return type(self)._columns(names, self.dim)

    def program(self, names, nf: int, velocity=None, field_scale=None):
        return ops.derived_program(type(self)._terms(names, self.dim, int(nf), velocity, field_scale), int(nf), self.dim, order=self._order)

    def _x(self, x) -> torch.Tensor:
        if not torch.is_tensor(x) or x.dtype != torch.float32 or x.dim() != 2 or int(x.size(0)) != self.n_nodes or int(x.size(1)) < 1:
            raise ValueError(f"x: expected a float32 tensor [{self.n_nodes}, F], got {getattr(x, 'dtype', type(x).__name__)} "
                             f"{tuple(getattr(x, 'shape', ()))}")
        return x

    def derived(self, x: torch.Tensor, names, velocity=None, field_scale=None) -> torch.Tensor:
        """[N, nd]: the columns of `names` of the fields x [N, F] (float32, rows of unit stride).  `velocity` defaults to fields
        0 .. dim − 1; `field_scale` [F] (default ones) multiplies into the coefficients — it undoes an affine scaling of the fields
        (the offsets drop out of every derivative)."""
        x = self._x(x)
        prog = self.program(names, int(x.size(1)), velocity, field_scale)
        if torch.is_grad_enabled() and x.requires_grad:
            from . import autograd as _ag
            return _ag.stencil_derived(self, x, prog)
        return self._launch(x, prog)

    def _sender_side(self):
        """(out_off, out_table, out_dst): the stencil entries grouped by sender, ascending CSR position within a sender — the offsets
        of that grouping, and the rows and receivers copied into its order.  Built on the first adjoint and kept: the plain forward
        pays nothing."""
        if self._adjoint_tables is None:
            table = getattr(self, self._table)
            n_entries = int(self.src.numel())
            deg = (self.off[1:] - self.off[:-1]).to(torch.int64)
            dst = torch.repeat_interleave(torch.arange(self.n_nodes, dtype=torch.int32, device=self.off.device), deg, output_size=n_entries)
            out = plan.gather_csr(self.src, self.n_nodes)
            if out.perm is not None:          # (None: the senders are grouped already)
                perm = out.perm.to(torch.int64)
                self._adjoint_tables = (out.off, table.index_select(0, perm).contiguous(), dst.index_select(0, perm).contiguous())
            else:
                self._adjoint_tables = (out.off, table, dst.contiguous())
        return self._adjoint_tables

    def _gy(self, gy, nd: int) -> torch.Tensor:
        device = getattr(self, self._table).device
        if not torch.is_tensor(gy) or gy.dtype != torch.float32 or gy.dim() != 2 or tuple(gy.shape) != (self.n_nodes, nd):
            raise ValueError(f"gy: expected a float32 tensor [{self.n_nodes}, {nd}] (one column per derived column), got "
                             f"{getattr(gy, 'dtype', type(gy).__name__)} {tuple(getattr(gy, 'shape', ()))}")
        if gy.device != device:
            raise ValueError(f"gy: on '{gy.device}', the operator is on '{device}' (there is no CPU fallback)")
        return gy.detach().contiguous()

    def _adjoint(self, gy: torch.Tensor, prog, nf: int) -> torch.Tensor:
        out_off, out_table, out_dst = self._sender_side()
        return type(self)._adjoint_op(gy, self.off, getattr(self, self._table), out_off, out_table, out_dst, prog, nf)

    def adjoint(self, gy: torch.Tensor, names, nf: int, velocity=None, field_scale=None) -> torch.Tensor:
        """[N, nf]: the transpose of `derived(·, names, velocity, field_scale)` on nf fields, applied to gy [N, nd] (float32; made
        dense first) — for all x and gy, ⟨derived(x), gy⟩ = ⟨x, adjoint(gy)⟩ up to rounding.  One launch (`g4c_mesh_derived_adjoint`
        or `g4c_mesh_jet_adjoint`): a gather over the entries a node SENDS, in a fixed order, no atomics.  A field `names` does not
        differentiate gets zeros."""
        if isinstance(nf, bool) or not isinstance(nf, int) or nf < 1:
            raise ValueError(f"nf: expected the number of fields (>= 1), got {nf!r}")
        terms = type(self)._terms(names, self.dim, nf, velocity, field_scale)
        gy = self._gy(gy, len(terms))
        return self._adjoint(gy, ops.derived_program(terms, nf, self.dim, order=self._order), nf)


class MeshGradient(_StencilOperator):
    """The least-squares gradient over the edges of `graph` (a Graph on the GPU with `edge_index` [2, E], row = sender, col =
    receiver, and `pos`), built once; `power` 0, 1 or 2 weighs an edge by |d|^(−power).

    `edge_vectors` [E, dim]: the edge vectors receiver − sender in physical units.  None uses `graph.pos[col] − graph.pos[row]`.  On
    a PERIODIC mesh pass the wrapped, unscaled `edge_attr` that `ConnectKNN` produced (before any `ScaleEdgeAttr`): the difference of
    the positions of an edge across the seam is a period off.

    `gradient(x)` [N, F, dim]; `derived(x, names)` [N, nd] with names 'div' (Σ_a ∂_a of the velocity components), 'vort' (one column
    in 2-D, ∂₀v − ∂₁u; three in 3-D) and 'grad:<f>' (dim columns); `columns(names)` their labels; `degenerate` bool [N]: the nodes
    whose neighbours do not span the space — their derivatives are 0.  Works on any [N, F] float32 device tensor: `graph.target`'s
    columns of a step as well as a prediction.

    `derived` (and `gradient`) of an x that requires grad is recorded for autograd: its backward is `adjoint(gy, names, nf)` [N, nf],
    the transpose of the same linear map (`g4c_mesh_derived_adjoint`; the weights g are constants: no gradient reaches the mesh).  The
    sender-side tables the adjoint walks are built on its first use."""

    def __init__(self, graph, power: int = 2, edge_vectors: Optional[torch.Tensor] = None):
        self.dim = check_mesh(graph, power, edge_vectors)
        ei = graph.edge_index
        if ei.device.type != "cuda":
            raise ValueError(f"graph: MeshGradient runs on a HIP device only, graph.edge_index is on '{ei.device}' (there is no CPU fallback)")
        self.power = power
        self.n_nodes = int(graph.num_nodes)
        if edge_vectors is None:
            pos = graph.pos.to(ei.device)
            edge_vectors = pos[ei[1]] - pos[ei[0]]
        rel = edge_vectors.detach().to(torch.float32).contiguous()
        ep, csr = plan.edge_csr(ei, self.n_nodes)
        self.off, self.max_deg = csr.off, csr.max_deg
        self.g, self.src, degenerate = ops.mesh_gradient_weights(rel, csr, ep.row, power)
        self.degenerate = degenerate.bool()
        self._adjoint_tables = None

    _table, _order = "g", 1
    _columns, _terms, _adjoint_op = staticmethod(derived_columns), staticmethod(derived_terms), staticmethod(ops.mesh_derived_adjoint)

    def _launch(self, x: torch.Tensor, prog) -> torch.Tensor:
        cur = torch.empty((self.n_nodes, int(prog.nd)), dtype=torch.float32, device=self.g.device)
        ops.mesh_derived(x, self.off, self.g, self.src, prog, cur)
        return cur

    def gradient(self, x: torch.Tensor) -> torch.Tensor:
        """[N, F, dim]: ∂_a x[:, f]."""
        x = self._x(x)
        nfld, per = int(x.size(1)), MAX_COLUMNS // self.dim
        out = torch.empty((self.n_nodes, nfld, self.dim), dtype=torch.float32, device=self.g.device)
        for f0 in range(0, nfld, per):
            fields = range(f0, min(f0 + per, nfld))
            out[:, f0:f0 + len(fields)] = self.derived(x, tuple(f"grad:{f}" for f in fields)).view(self.n_nodes, len(fields), self.dim)
        return out

    def __repr__(self):
        return f"MeshGradient(nodes={self.n_nodes}, edges={int(self.src.numel())}, dim={self.dim}, power={self.power})"
