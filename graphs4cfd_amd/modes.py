"""Modal analysis of a set of snapshots: POD and DMD by the method of snapshots, from a Gram matrix formed on the device.

Everything of the size of a snapshot (L = N nf values) goes through three HIP launches (`ops.snapshot_mean`, `ops.snapshot_gram`,
`ops.snapshot_combine`, csrc/snapshot_modes.hip): the fp64 mean, the fp64 Gram matrix G = (X − mean) W (X − mean)ᵀ of the M selected
snapshots in a fixed order of summation, and linear combinations of the snapshots.  Everything of size M — the eigen-decomposition of
G, the truncation, DMD's reduced operator — is fp64 `torch.linalg` on the host (`pod_from_gram`, `dmd_from_gram`: they take a Gram
matrix and nothing else, so a test can feed them one from anywhere).

Conventions.  The inner product is ⟨x, y⟩ = Σ_l w[l] x[l] y[l], w[n nf + f] = node_weights[n] field_weights[f] (ones when absent).
POD: G = V Σ² Vᵀ, singular values σ_k descending, coefficients a_k(t_i) = V[i, k] σ_k, modes φ_k = Σ_i V[i, k] / σ_k (x_i − mean),
orthonormal in that inner product; the sign of a mode is fixed by V alone (the largest-magnitude entry of each column of V is
positive, the first such entry on ties), so equal Gram matrices give equal modes.  Modes with λ_k ≤ M 2⁻⁵² λ_0 are dropped whatever was
asked for: the Gram route cannot resolve them.  DMD (exact DMD, snapshot variant) uses the uncentred Gram matrix of the same
snapshots: G11 = G[:-1, :-1] = V Σ² Vᵀ truncated the same way, Ã = Σ⁻¹ Vᵀ G12 V Σ⁻¹ with G12 = G[:-1, 1:], eigenpairs (μ, W), modes
X₂ V Σ⁻¹ W, amplitudes by least squares against the first snapshot — from G alone."""
from __future__ import annotations

import math
from typing import Optional

import torch

from . import _lib, ops

__all__ = ["Modes", "SnapshotModes", "DynamicModes", "ModesComparison", "pod_from_gram", "dmd_from_gram", "principal_cosines"]


def _is_int(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool)


def _is_real(v) -> bool:
    return isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v)


def _gram_arg(G, name: str) -> torch.Tensor:
    if not torch.is_tensor(G):
        try:
            G = torch.as_tensor(G)
        except Exception:
            raise TypeError(f"{name}: expected a square float64 matrix, got {type(G).__name__}") from None
    if G.dtype != torch.float64:
        raise TypeError(f"{name}: expected a float64 matrix (the Gram route works in fp64), got {G.dtype}")
    if G.dim() != 2 or G.size(0) != G.size(1) or G.size(0) < 1:
        raise ValueError(f"{name}: expected a square matrix [M >= 1, M], got shape {tuple(G.shape)}")
    G = G.detach().cpu()
    if not bool(torch.isfinite(G).all()):
        raise ValueError(f"{name}: the Gram matrix holds a non-finite value")
    return G


def _truncate(lam: torch.Tensor, M: int, rank: Optional[int], energy: Optional[float]):
    """lam: eigenvalues, descending.  -> (R, resolved, dropped, fractions over the resolved ones)."""
    lam0 = float(lam[0])
    if not lam0 > 0.0:
        raise ValueError("snapshots: the Gram matrix has no positive eigenvalue (the centred snapshots are all zero)")
    resolved = int((lam > M * 2.0 ** -52 * lam0).sum())          # (descending: the resolved ones come first)
    frac = lam[:resolved] / lam[:resolved].sum()
    R = resolved
    if energy is not None:
        cum = torch.cumsum(frac, 0)
        R = min(R, int((cum < energy * (1.0 - 1e-15)).sum()) + 1)
    if rank is not None:
        R = min(R, rank)
    return R, resolved, int(lam.numel()) - resolved, frac


def _fix_signs(V: torch.Tensor) -> torch.Tensor:
    """The largest-magnitude entry of each column positive, the first such entry on ties."""
    idx = torch.argmax((V.abs() == V.abs().max(dim=0, keepdim=True).values).to(torch.int8), dim=0)     # first maximum of each column
    s = torch.sign(V[idx, torch.arange(V.size(1))])
    s[s == 0] = 1.0
    return V * s


def _eigh_desc(G: torch.Tensor):
    lam, V = torch.linalg.eigh(0.5 * (G + G.T))
    return torch.flip(lam, (0,)), torch.flip(V, (1,))


def pod_from_gram(gram, rank: Optional[int] = None, energy: Optional[float] = None) -> dict:
    """POD of the snapshots whose (centred, weighted) Gram matrix is `gram` float64 [M, M] -> dict: singular_values [R], energy [R]
    (fractions of the resolved total), cumulative_energy [R], coefficients [M, R] = V σ, V [M, R], combine [M, R] = V / σ (the modes
    are Σ_i combine[i, k] (x_i − mean)), dropped (modes at or below M 2⁻⁵² λ_0).  fp64 on the host."""
    G = _gram_arg(gram, "gram")
    M = int(G.size(0))
    lam, V = _eigh_desc(G)
    R, _, dropped, frac = _truncate(lam, M, rank, energy)
    V = _fix_signs(V[:, :R].contiguous())
    sigma = torch.sqrt(lam[:R])
    return dict(singular_values=sigma, energy=frac[:R].clone(), cumulative_energy=torch.cumsum(frac, 0)[:R].clone(), coefficients=V * sigma,
                V=V, combine=V / sigma, dropped=dropped)


def dmd_from_gram(gram, rank: Optional[int] = None, energy: Optional[float] = None, step: float = 1.0) -> dict:
    """Exact DMD (snapshot variant) of the M snapshots whose uncentred, weighted Gram matrix is `gram` float64 [M >= 2, M]; `step` is
    the time between two of them.  -> dict: eigenvalues μ [R] complex, frequency = Im log μ / (2π step), growth = Re log μ / step,
    amplitudes [R] complex (least squares against the first snapshot), combine [M − 1, R] complex (the modes are
    Σ_i combine[i, k] x_{i+1}), dropped; sorted by |amplitude|, descending (of a conjugate pair, the member above the real axis first).  fp64 / complex128 on the host."""
    G = _gram_arg(gram, "gram")
    M = int(G.size(0))
    if M < 2:
        raise ValueError(f"gram: DMD needs at least 2 snapshots, got {M}")
    G11, G12, G22, g20 = G[:-1, :-1], G[:-1, 1:], G[1:, 1:], G[1:, 0]
    lam, V = _eigh_desc(G11)
    R, _, dropped, _ = _truncate(lam, M - 1, rank, energy)
    V = _fix_signs(V[:, :R].contiguous())
    B = V / torch.sqrt(lam[:R])                                   # V Σ⁻¹
    mu, W = torch.linalg.eig(B.T @ G12 @ B)
    Cd = B.to(torch.complex128) @ W                               # Φ = X₂ Cd
    # least squares of x_0 on Φ in the w inner product: (Φᴴ W Φ) b = Φᴴ W x_0, both from G
    lhs = Cd.conj().T @ G22.to(torch.complex128) @ Cd
    rhs = Cd.conj().T @ g20.to(torch.complex128)
    amp = torch.linalg.lstsq(lhs, rhs[:, None]).solution[:, 0]
    # by amplitude, descending; the two members of a conjugate pair have equal amplitudes up to rounding, which must not decide their
    # order: amplitudes are compared to 2^-20 of the largest, then the member above the real axis comes first
    q = torch.round(amp.abs() / amp.abs().max().clamp_min(1e-300) * 2.0 ** 20).tolist()
    order = torch.tensor(sorted(range(R), key=lambda k: (-q[k], -float(mu[k].imag), -float(mu[k].real))), dtype=torch.long)
    mu, Cd, amp = mu[order], Cd[:, order].contiguous(), amp[order]
    logmu = torch.log(mu)
    return dict(eigenvalues=mu, frequency=logmu.imag / (2.0 * math.pi * step), growth=logmu.real / step, amplitudes=amp, combine=Cd,
                dropped=dropped, gram=G)


def principal_cosines(pod_a: dict, cross, pod_b: dict) -> torch.Tensor:
    """The principal cosines between two mode subspaces from their `pod_from_gram` parts and the cross-Gram matrix
    cross[i][j] = ⟨a_i − mean_a, b_j − mean_b⟩ of their centred snapshots: the singular values of Σ_a⁻¹ V_aᵀ cross V_b Σ_b⁻¹, descending."""
    if not torch.is_tensor(cross):
        cross = torch.as_tensor(cross)
    if cross.dtype != torch.float64 or tuple(cross.shape) != (int(pod_a["combine"].size(0)), int(pod_b["combine"].size(0))):
        raise ValueError(f"cross: expected float64 [{int(pod_a['combine'].size(0))}, {int(pod_b['combine'].size(0))}], got "
                         f"{cross.dtype} {tuple(cross.shape)}")
    return torch.linalg.svdvals(pod_a["combine"].T @ cross.detach().cpu() @ pod_b["combine"])


class Modes:
    """A request for the modal analysis of a set of snapshots (`Modes.fit`, `Rollout.modes`, `GNN.modes`, `GNN.evaluate(modes=)`).

    rank / energy truncate: at most `rank` modes, and the smallest number whose cumulative energy reaches the fraction `energy`.
    centre: subtract the fp64 mean of the selected snapshots (POD of the fluctuation).  node_weights [N] (cell areas) and
    field_weights [nf] (0 leaves a field out) define the inner product, w[n nf + f] = node_weights[n] field_weights[f] in fp64.
    start / stride / count select the snapshots start, start + stride, ... among those given (a rollout's kept slots); dt is the
    time between two given snapshots.  dmd=True also computes the dynamic modes (`SnapshotModes.dmd`), from the uncentred Gram matrix."""

    def __init__(self, rank: Optional[int] = None, energy: Optional[float] = None, centre: bool = True, node_weights=None,
                 field_weights=None, start: int = 0, stride: int = 1, count: Optional[int] = None, dt: float = 1.0, dmd: bool = False):
        if rank is not None and (not _is_int(rank) or not 1 <= rank <= _lib.SNAPSHOT_MAX_ROWS):
            raise ValueError(f"rank: expected None or an integer in 1 .. {_lib.SNAPSHOT_MAX_ROWS}, got {rank!r}")
        if energy is not None and (not _is_real(energy) or not 0.0 < energy <= 1.0):
            raise ValueError(f"energy: expected None or a fraction in (0, 1], got {energy!r}")
        if not isinstance(centre, bool):
            raise TypeError(f"centre: expected a bool, got {centre!r}")
        if not isinstance(dmd, bool):
            raise TypeError(f"dmd: expected a bool, got {dmd!r}")
        if not _is_int(start) or start < 0:
            raise ValueError(f"start: expected an integer >= 0 (the first snapshot taken), got {start!r}")
        if not _is_int(stride) or stride < 1:
            raise ValueError(f"stride: expected an integer >= 1, got {stride!r}")
        if count is not None and (not _is_int(count) or not 1 <= count <= _lib.SNAPSHOT_MAX_ROWS):
            raise ValueError(f"count: expected None or an integer in 1 .. {_lib.SNAPSHOT_MAX_ROWS}, got {count!r}")
        if not _is_real(dt) or not dt > 0:
            raise ValueError(f"dt: expected a positive finite number, got {dt!r}")
        self.rank, self.energy, self.centre, self.dmd = rank, None if energy is None else float(energy), centre, dmd
        self.node_weights = self._weights("node_weights", node_weights)
        self.field_weights = self._weights("field_weights", field_weights)
        self.start, self.stride, self.count, self.dt = start, stride, count, float(dt)

    @staticmethod
    def _weights(name: str, w) -> Optional[torch.Tensor]:
        if w is None:
            return None
        if not torch.is_tensor(w):
            try:
                w = torch.as_tensor(w)
            except Exception:
                raise TypeError(f"{name}: expected a 1-D tensor or sequence of numbers, got {type(w).__name__}") from None
        if w.dtype == torch.bool or w.is_complex():
            raise TypeError(f"{name}: expected real numbers, got {w.dtype}")
        if w.dim() != 1 or w.numel() < 1:
            raise ValueError(f"{name}: expected a 1-D tensor of at least one weight, got shape {tuple(w.shape)}")
        w = w.detach().to(torch.float64)
        if not bool(torch.isfinite(w).all()) or bool((w < 0).any()):
            raise ValueError(f"{name}: weights are finite and >= 0 (0 leaves the entry out)")
        if not bool((w > 0).any()):
            raise ValueError(f"{name}: every weight is 0")
        return w

    # ---- what a fit needs of its snapshots

    def selection(self, available: int):
        """(first, stride, count) among `available` snapshots."""
        if self.start >= available:
            raise ValueError(f"start: {self.start} is past the {available} snapshot(s) at hand")
        most = (available - self.start + self.stride - 1) // self.stride
        count = most if self.count is None else self.count
        if count > most:
            raise ValueError(f"count: {count} snapshots from {self.start} in strides of {self.stride} need "
                             f"{self.start + (count - 1) * self.stride + 1}, {available} are at hand")
        if count > _lib.SNAPSHOT_MAX_ROWS:
            raise NotImplementedError(f"count: {count} snapshots (at most {_lib.SNAPSHOT_MAX_ROWS}: give count= or a larger stride=)")
        if self.dmd and count < 2:
            raise ValueError(f"count: DMD needs at least 2 snapshots, {count} selected")
        return self.start, self.stride, count

    def weights(self, n_nodes: int, nf: int, device, perm: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
        """w float64 [n_nodes nf] on `device`, or None for ones; `perm` (a renumbered rollout: its row r is the caller's row perm[r])
        takes the node weights into the rollout's numbering."""
        nw, fw = self.node_weights, self.field_weights
        if nw is not None and nw.numel() != n_nodes:
            raise ValueError(f"node_weights: {nw.numel()} weights for {n_nodes} nodes")
        if fw is not None and fw.numel() != nf:
            raise ValueError(f"field_weights: {fw.numel()} weights for {nf} fields")
        if nw is None and fw is None:
            return None
        nw = torch.ones(n_nodes, dtype=torch.float64) if nw is None else nw
        fw = torch.ones(nf, dtype=torch.float64) if fw is None else fw
        nw = nw.to(device)
        if perm is not None:
            nw = nw[perm.to(device)]
        return (nw[:, None] * fw.to(device)[None, :]).reshape(-1).contiguous()

    # ---- fits

    def fit(self, snapshots: torch.Tensor, layout: str = "steps", nf: Optional[int] = None) -> "SnapshotModes":
        """The modes of `snapshots` (float32 on the HIP device): layout "steps" — [M, N, nf], step-major and contiguous, a rollout's own
        buffer — or "columns" — [N, nf M], the layout of `GNN.solve`'s result and of `graph.target`, transposed once on the device
        (nf: the number of fields; taken from field_weights when those are given)."""
        if layout not in ("steps", "columns"):
            raise ValueError(f"layout: expected 'steps' or 'columns', got {layout!r}")
        if not torch.is_tensor(snapshots) or snapshots.dtype != torch.float32:
            raise TypeError(f"snapshots: expected a float32 tensor, got {getattr(snapshots, 'dtype', type(snapshots).__name__)}")
        if layout == "steps":
            if snapshots.dim() != 3 or snapshots.numel() == 0:
                raise ValueError(f"snapshots: layout 'steps' is [M, N, nf], got shape {tuple(snapshots.shape)}")
            if nf is not None and nf != int(snapshots.size(2)):
                raise ValueError(f"nf: {nf!r}, the snapshots hold {int(snapshots.size(2))} fields")
            if not snapshots.is_contiguous():
                raise ValueError(f"snapshots: layout 'steps' is step-major and contiguous, got strides {tuple(snapshots.stride())}")
        else:
            if nf is None and self.field_weights is not None:
                nf = int(self.field_weights.numel())
            if not _is_int(nf) or nf < 1:
                raise ValueError(f"nf: layout 'columns' needs the number of fields (an integer >= 1, or field_weights=), got {nf!r}")
            if snapshots.dim() != 2 or snapshots.numel() == 0 or int(snapshots.size(1)) % nf:
                raise ValueError(f"snapshots: layout 'columns' is [N, nf M] with nf = {nf}, got shape {tuple(snapshots.shape)}")
            _lib.require_hip(snapshots)
            n = int(snapshots.size(0))
            snapshots = snapshots.reshape(n, -1, nf).permute(1, 0, 2).contiguous()
        _lib.require_hip(snapshots)
        return self._fit_steps(snapshots, int(snapshots.size(0)))

    def _fit_steps(self, x: torch.Tensor, available: int, perm: Optional[torch.Tensor] = None) -> "SnapshotModes":
        """x float32 [slots, N, nf] on the device, of which the first `available` are filled; perm: the rollout's renumbering."""
        sel = self.selection(available)
        n, nf = int(x.size(1)), int(x.size(2))
        dev = x.device
        w = self.weights(n, nf, dev, perm)
        mean = ops.snapshot_mean(x, sel) if self.centre else None
        gram = ops.snapshot_gram(x, mean_a=mean, sel_a=sel, w=w)
        dmd_gram = None
        if self.dmd:
            dmd_gram = ops.snapshot_gram(x, sel_a=sel, w=w) if self.centre else gram
        return SnapshotModes(self, gram.cpu(), None if dmd_gram is None else dmd_gram.cpu(), x=x, sel=sel, w=w, mean=mean, perm=perm)

    def from_gram(self, gram, dmd_gram=None) -> "SnapshotModes":
        """The M-sized algebra alone, on a Gram matrix from anywhere (float64 [M, M]; `dmd_gram`: the uncentred one, for dmd=True):
        a `SnapshotModes` without `mean` and `modes`, and without the methods that need the snapshots."""
        if self.dmd and dmd_gram is None:
            raise ValueError("dmd_gram: dmd=True needs the uncentred Gram matrix")
        return SnapshotModes(self, _gram_arg(gram, "gram"), None if dmd_gram is None or not self.dmd else _gram_arg(dmd_gram, "dmd_gram"))


class DynamicModes:
    """The dynamic modes of a set of snapshots (`SnapshotModes.dmd`), sorted by amplitude, descending: `eigenvalues` μ [R] complex,
    `frequency` = Im log μ / (2π dt stride) and `growth` = Re log μ / (dt stride) (fp64), `amplitudes` [R] complex, `modes` complex64
    [R, N, nf] (None without snapshots), `dropped`, `gram` (the uncentred Gram matrix they were formed from)."""

    def __init__(self, parts: dict, modes: Optional[torch.Tensor]):
        self.eigenvalues, self.frequency, self.growth = parts["eigenvalues"], parts["frequency"], parts["growth"]
        self.amplitudes, self.dropped, self.modes, self.gram = parts["amplitudes"], parts["dropped"], modes, parts["gram"]

    def dominant(self) -> int:
        """The index of the mode of largest amplitude among those with frequency > 0 (of a conjugate pair, the one above the axis)."""
        for k in range(int(self.frequency.numel())):          # (sorted by amplitude)
            if float(self.frequency[k]) > 0.0:
                return k
        raise ValueError("dominant: no mode oscillates (every frequency is <= 0)")


class SnapshotModes:
    """POD of a set of snapshots (`Modes.fit`): `gram` [M, M] and `singular_values`, `energy`, `cumulative_energy` [R], `coefficients`
    [M, R] (fp64, host); `mean` [N, nf] fp64 (None without centring) and `modes` [R, N, nf] fp32 on the device, rows in the caller's
    numbering; `dropped`; `dmd` (`DynamicModes`, with `Modes(dmd=True)`)."""

    def __init__(self, spec: Modes, gram: torch.Tensor, dmd_gram: Optional[torch.Tensor], x=None, sel=None, w=None, mean=None, perm=None):
        self.spec, self.gram = spec, gram
        pod = pod_from_gram(gram, spec.rank, spec.energy)
        self.singular_values, self.energy, self.cumulative_energy = pod["singular_values"], pod["energy"], pod["cumulative_energy"]
        self.coefficients, self.dropped, self._V, self._combine = pod["coefficients"], pod["dropped"], pod["V"], pod["combine"]
        self._x, self._sel, self._w, self._mean, self._perm = x, sel, w, mean, perm
        self.mean = self.modes = self.dmd = None
        parts = dmd_from_gram(dmd_gram, spec.rank, spec.energy, spec.dt * spec.stride) if dmd_gram is not None else None
        if x is None:
            self.dmd = None if parts is None else DynamicModes(parts, None)
            return
        n, nf = int(x.size(1)), int(x.size(2))
        dev = x.device
        self.modes = self._rows_out(ops.snapshot_combine(x, self._combine.to(dev), mean=mean, sel=sel).view(-1, n, nf))
        if mean is not None:
            self.mean = self._rows_out(mean.view(1, n, nf))[0]
        if parts is not None:
            first, stride, count = sel
            cd = parts["combine"]
            sel2 = (first + stride, stride, count - 1)            # X₂: the snapshots from the second on
            re = ops.snapshot_combine(x, cd.real.contiguous().to(dev), sel=sel2)
            im = ops.snapshot_combine(x, cd.imag.contiguous().to(dev), sel=sel2)
            self.dmd = DynamicModes(parts, self._rows_out(torch.complex(re, im).view(-1, n, nf)))

    def _rows_out(self, t: torch.Tensor) -> torch.Tensor:
        """[k, N, nf] in the rollout's numbering -> the caller's."""
        if self._perm is None:
            return t
        out = torch.empty_like(t)
        out[:, self._perm.to(t.device)] = t
        return out

    def _need_snapshots(self, what: str) -> None:
        if self._x is None:
            raise RuntimeError(f"{what}: these modes were formed from a Gram matrix alone (Modes.from_gram): there are no snapshots")

    def _in_numbering(self, x: torch.Tensor, own_perm, mean=None):
        """Snapshots [k, N, nf] (and a flat fp64 mean) numbered by `own_perm` (None: the caller's) -> this object's numbering."""
        if own_perm is self._perm or (own_perm is not None and self._perm is not None and torch.equal(own_perm, self._perm)):
            return x, mean
        n, nf = int(x.size(1)), int(x.size(2))
        m = None if mean is None else mean.view(1, n, nf)
        if own_perm is not None:                                   # -> the caller's
            xc = torch.empty_like(x)
            xc[:, own_perm] = x
            x = xc
            if m is not None:
                mc = torch.empty_like(m)
                mc[:, own_perm] = m
                m = mc
        if self._perm is not None:                                 # -> this rollout's
            x = x[:, self._perm]
            m = None if m is None else m[:, self._perm]
        return x.contiguous(), None if m is None else m.contiguous().view(-1)

    def project(self, snapshots: torch.Tensor) -> torch.Tensor:
        """The coefficients of other snapshots [K, N, nf] (float32, device, the caller's rows) on these modes, fp64 [K, R] on the host:
        ⟨y_i − mean, φ_k⟩, formed from one cross-Gram launch against the snapshots of the fit."""
        self._need_snapshots("project")
        if not torch.is_tensor(snapshots) or snapshots.dtype != torch.float32:
            raise TypeError(f"snapshots: expected a float32 tensor, got {getattr(snapshots, 'dtype', type(snapshots).__name__)}")
        if snapshots.dim() != 3 or tuple(snapshots.shape[1:]) != tuple(self._x.shape[1:]) or snapshots.size(0) < 1:
            raise ValueError(f"snapshots: expected [K >= 1, {int(self._x.size(1))}, {int(self._x.size(2))}], got shape {tuple(snapshots.shape)}")
        _lib.require_hip(snapshots, self._x)
        y, _ = self._in_numbering(snapshots.contiguous(), None)
        cross = ops.snapshot_gram(y, self._x, mean_a=self._mean, mean_b=self._mean, sel_b=self._sel, w=self._w)
        return cross.cpu() @ self._combine

    def reconstruct(self, rank: Optional[int] = None) -> torch.Tensor:
        """The selected snapshots rebuilt from the first `rank` modes (default all), float32 [M, N, nf] on the device in the caller's
        rows: mean + Σ_k a_k(t_i) φ_k, one combine launch over the modes."""
        self._need_snapshots("reconstruct")
        R = int(self.singular_values.numel())
        if rank is None:
            rank = R
        if not _is_int(rank) or not 1 <= rank <= R:
            raise ValueError(f"rank: expected an integer in 1 .. {R}, got {rank!r}")
        modes = self.modes.contiguous()
        out = ops.snapshot_combine(modes, self.coefficients[:, :rank].T.contiguous().to(modes.device), sel=(0, 1, rank)).view(-1, *modes.shape[1:])
        if self.mean is not None:
            out = (out.double() + self.mean[None]).float()
        return out

    def alignment(self, other: "SnapshotModes") -> torch.Tensor:
        """The principal cosines between this mode subspace and `other`'s, fp64 [min(R, R')] descending, in this object's inner
        product: the singular values of Σ_p⁻¹ V_pᵀ (A_p W A_tᵀ) V_t Σ_t⁻¹, A the centred snapshots, from one cross-Gram launch."""
        if not isinstance(other, SnapshotModes):
            raise TypeError(f"other: expected a SnapshotModes, got {type(other).__name__}")
        self._need_snapshots("alignment")
        other._need_snapshots("alignment")
        if tuple(other._x.shape[1:]) != tuple(self._x.shape[1:]):
            raise ValueError(f"other: snapshots of shape {tuple(other._x.shape[1:])}, these are {tuple(self._x.shape[1:])}")
        _lib.require_hip(self._x, other._x)
        if other is self:
            yx, ym = self._x, self._mean
        else:
            yx, ym = self._in_numbering(other._x, other._perm, other._mean)
        cross = ops.snapshot_gram(self._x, yx, mean_a=self._mean, mean_b=ym, sel_a=self._sel, sel_b=other._sel, w=self._w)
        return principal_cosines(dict(combine=self._combine), cross, dict(combine=other._combine))


class ModesComparison:
    """`GNN.evaluate(modes=)`: `prediction` and `target` (`SnapshotModes` of the kept predictions and of the target's columns of the
    same steps) and `alignment`, the principal cosines between their mode subspaces."""

    def __init__(self, prediction: SnapshotModes, target: SnapshotModes):
        self.prediction, self.target = prediction, target
        self.alignment = prediction.alignment(target)
