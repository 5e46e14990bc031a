"""`GNN` base class: model construction / checkpoint loading and the entry points that roll a model out (the rollout itself —
`Rollout`, what rides along in its step, the result classes — is rollout.py; its names are re-exported here).

Mirrors the inference-side surface of the reference's graphs4cfd/nn/model.py: constructor
`(arch, weights, checkpoint, device)`, `load_model` (:112-130), `solve` (:303-321),
`shift_and_replace` (:323-327), `save_checkpoint` (:329-349), `num_params` (:351-354), and the training side:
`TrainConfig` (:14-82), `fit` (:152-301), `grad_norm2` (:356-362) — the forward of a training step is the same fused
launches, recorded for autograd (../autograd.py).

`solve` keeps the whole rollout on the device: the history-window shift and the write into
`outputs[:, nf*t:nf*(t+1)]` are one kernel reading the step index from device memory, so a step has no
host synchronisation and can be captured once in a hipGraph and replayed (`capture=True`).
"""
from __future__ import annotations

import os
import warnings
from typing import Callable, List, Optional, Union

import torch
from torch import nn

from .. import _lib, ops
from ..graph import Graph
# the rollout and what rides along in its step live in rollout.py; every name stays importable from here
from .rollout import (KEYWORDS, REORDER_MIN_NODES, Rollout, RolloutDerived, RolloutErrors, RolloutForces, RolloutIntegrals,      # noqa: F401
                      RolloutMoments, RolloutSamples, RolloutSpectrum, RolloutWelch, Spectrum, Welch, _check_moments, _check_parts,
                      _check_records, _check_spectrum)


def collate(graphs: List[Graph]) -> Graph:
    """Minimal stand-in for `torch_geometric.data.Batch.from_data_list` (called at nn/model.py:309):
    tensors are concatenated along dim 0 (dim -1 for attributes whose name contains 'index', which are
    also offset by the running node count), and `batch` holds the graph id of every node."""
    out, offset, batch = {}, 0, []
    keys = graphs[0].keys()
    for gi, g in enumerate(graphs):
        n = g.num_nodes
        for k in keys:
            v = getattr(g, k)
            if not torch.is_tensor(v):
                out[k] = v
                continue
            out.setdefault(k, []).append(v + offset if "index" in k else v)
        batch.append(torch.full((n,), gi, dtype=torch.long, device=g.pos.device if "pos" in g else None))
        offset += n
    merged = {k: (torch.cat(v, dim=-1 if "index" in k else 0) if isinstance(v, list) else v) for k, v in out.items()}
    merged["batch"] = torch.cat(batch)
    return Graph(**merged)


class TrainConfig():
    r"""Training configuration of a model (reference: nn/model.py:14-82; same fields, same defaults, dict-style access).

    name, folder, checkpoint (resume from), tensor_board (log dir or None), chk_interval (epochs), training_loss /
    validation_loss (callables `(graph, pred, target)`), epochs, num_steps (rollout lengths, advanced when the monitored
    loss falls below `add_steps['tolerance']`), batch_size, lr, grad_clip ({'epoch', 'limit'} or None), scheduler
    ({'factor', 'patience', 'loss'} or None), stopping (minimum lr), mixed_precision, device.
    saved_activations ("fp32" | "bf16", not in the reference; "bf16" needs mixed_precision=True): the format of the rows the forward
    keeps for the backward — "bf16" halves them (ops.set_train_precision(..., saved="bf16"))."""

    def __init__(self, name: str, folder: str = './', checkpoint: Union[None, str] = None, tensor_board: Union[None, str] = None,
                 chk_interval: int = 1, training_loss: Callable = None, validation_loss: Callable = None, epochs: int = 1,
                 num_steps: Union[int, List[int]] = [1], add_steps: dict = {'tolerance': 0, 'loss': 'training'},
                 batch_size: int = 1, lr: float = 1e-3, grad_clip: Union[None, dict] = None, scheduler: Union[None, dict] = None,
                 stopping: float = 0., mixed_precision: bool = False, device: Optional[torch.device] = None,
                 saved_activations: str = "fp32"):
        if saved_activations not in ("fp32", "bf16"):
            raise ValueError(f"saved_activations {saved_activations!r}: expected 'fp32' or 'bf16'")
        if saved_activations == "bf16" and not mixed_precision:
            raise ValueError("saved_activations='bf16' needs mixed_precision=True")
        self.saved_activations = saved_activations
        self.name, self.folder, self.checkpoint, self.tensor_board, self.chk_interval = name, folder, checkpoint, tensor_board, chk_interval
        self.training_loss, self.validation_loss, self.epochs = training_loss, validation_loss, epochs
        self.num_steps = [num_steps] if isinstance(num_steps, int) else num_steps
        self.add_steps, self.batch_size, self.lr, self.grad_clip, self.scheduler = add_steps, batch_size, lr, grad_clip, scheduler
        self.stopping, self.mixed_precision, self.device = stopping, mixed_precision, device

    def __repr__(self):
        return repr(self.__dict__)

    def __getitem__(self, key):
        return self.__dict__.get(key)


class GNN(nn.Module):
    r"""Base class for all the GNN models.

    Args:
        arch (Optional[dict]): Dictionary with the model architecture. Defaults to `None`.
        weights (Optional[str]): Path of the weights file. Defaults to `None`.
        checkpoint (Optional[str]): Path of the checkpoint file. Defaults to `None`.
        device (Optional[torch.device]): Device where the model is loaded. Defaults to `torch.device('cpu')`
            (the reference's default); forward/solve need a HIP device.
    """

    def __init__(self, arch: Optional[dict] = None, weights: Optional[str] = None, checkpoint: Optional[str] = None,
                 device: Optional[torch.device] = torch.device('cpu')):
        super().__init__()
        self.device = torch.device(device) if device is not None else torch.device('cpu')
        self.load_model(arch, weights, checkpoint)

    def __init_subclass__(cls, **kwargs):
        """Every model class's `forward` (the reference's other public entry point, e.g. nn/mus_gnn.py:173-218) is wrapped so that a
        BARE call — outside `solve` / `Rollout`, outside autograd — carries the same range guarantee as `solve`: VERDICT r05 item 6."""
        super().__init_subclass__(**kwargs)
        f = cls.__dict__.get("forward")
        if f is not None and not getattr(f, "_g4c_range_checked", False):
            cls.forward = _range_checked_forward(f)

    def load_model(self, arch, weights, checkpoint):
        """Builds the modules and fills them: either from an arch dict (+ an optional state-dict file), or from a `.chk` written by
        `save_checkpoint` (the reference's format, nn/model.py:112-150: 'arch', 'weights', optimiser state ...).  Any other
        combination leaves the model without modules, like the reference does."""
        source = None
        if checkpoint is not None and arch is None and weights is None:
            source = torch.load(checkpoint, map_location=self.device, weights_only=False)
            arch, state = source['arch'], source['weights']
        elif arch is not None and checkpoint is None:
            state = torch.load(weights, map_location=self.device) if weights is not None else None
        else:
            return
        self.load_arch(arch)
        self.to(self.device)
        if state is not None:
            self.load_state_dict(state)
        self.num_fields = arch["decoder"][1][-1] if 'decoder' in arch else None
        # names under which clipped fp16 values are reported (ops.f16_range_report)
        from .blocks import MLP as _MLP
        sites = []
        for name, m in self.named_modules():
            if isinstance(m, _MLP):
                m._site = f"{type(self).__name__}.{name}"
                sites.append(m._site)
        self._range_sites = frozenset(sites)     # this model's names in a report (ops.check_f16_range(sites=))

    def to(self, *args, **kwargs):
        out = super().to(*args, **kwargs)
        try:
            self.device = next(self.parameters()).device
        except StopIteration:
            pass
        return out

    # To be overwritten
    def load_arch(self, arch: dict):
        """Defines the hyper-parameters of the model; overloaded by each model class."""
        pass

    def _pretrained(self, table: dict, model: str) -> str:
        if model not in table:
            raise ValueError(f"Model {model} not recognized.")
        path = os.path.join(os.path.dirname(__file__), table[model])
        if not os.path.exists(path):
            raise FileNotFoundError(f"pretrained checkpoint {path} is not shipped (Git-LFS blob of the reference); "
                                    "pass checkpoint=<path to .chk> instead")
        return path

    # ---------------------------------------------------------------------------------- training
    def fit(self, train_config: TrainConfig, train_loader, val_loader=None):
        """Trains the model (the behaviour of the reference's nn/model.py:152-301: Adam, optional ReduceLROnPlateau, gradient
        clipping, one optimiser step per rollout step with the prediction fed back detached, validation over the longest rollout,
        `.chk` files in the reference's format, the rollout length advanced when the monitored loss passes the tolerance).  The
        loop itself is nn/training.py (`Trainer`: a rollout curriculum, an optimiser factory, a checkpoint file, one method per pass).

        Differences, all deliberate: `scheduler=None` / `tensor_board=None` work (the reference dereferences both
        unconditionally, :279,:299); `mixed_precision` runs every matrix product of the run (forward, input and weight
        gradients) on bf16-rounded operands with fp32 accumulation (ops.set_mlp_precision("bf16") + ops.set_train_precision("bf16"),
        both restored when `fit` returns or raises) and needs no loss scaling — bf16 has fp32's exponent range, and master weights,
        biases, LayerNorm, sums and Adam stay fp32; checkpoints are unchanged; a clip of the default
        fp16-split arithmetic during an epoch is reported (ops.check_f16_range).  `self.history` holds one record per epoch."""
        from .training import Trainer
        Trainer(self, train_config, train_loader, val_loader).run()
        return

    def grad_norm2(self):
        """L2 norm of the gradients (nn/model.py:356-362): multi-tensor norms and one device->host transfer instead of a
        norm launch and a transfer per parameter."""
        grads = [p.grad.detach() for p in self.parameters() if p.requires_grad and p.grad is not None]
        if not grads:
            return 0.0
        return float(torch.linalg.vector_norm(torch.stack(torch._foreach_norm(grads))))

    # ---------------------------------------------------------------------------------- rollout
    def solve(self, graph: Union[Graph, List[Graph]], n_out: int, *, capture: Optional[bool] = None, every: int = 1) -> torch.Tensor:
        """Evaluate the model on the graph for n_out time-steps. Returns [N, num_fields*n_out].

        capture: replay steps 2..n_out from a hipGraph captured on step 2 (default: on when
        n_out >= 4 and the environment variable G4C_HIPGRAPH is not '0').
        every (not in the reference): keep only every k-th step — steps k - 1, 2k - 1, ... (0-based) — and return
        [N, num_fields * (n_out // k)]; the buffer of all n_out steps is then never allocated (`Rollout(every=)`)."""
        assert n_out > 0, "n_out must be greater than 0."
        if int(every) < 1:
            raise ValueError(f"every: solve() keeps every k-th step, k >= 1, got {every} (evaluate() runs a rollout without snapshots)")
        with self._rollout(graph, n_out, capture, "solve()", every=int(every)) as ro:
            ro.run(n_out)
            return ro.result()       # (reports a clip of the default arithmetic in this model's own launches)

    def evaluate(self, graph: Union[Graph, List[Graph]], n_out: Optional[int] = None, *, every: int = 0, probes: Optional[torch.Tensor] = None,
                 capture: Optional[bool] = None, moments=None, error_moments=None, derived=None, derived_every: int = 0,
                 derived_moments=None, derived_options: Optional[dict] = None, spectrum: Optional["Spectrum"] = None, samples=None,
                 sample_every: int = 1, sample_moments=None, sample_spectrum: Optional["Spectrum"] = None,
                 sample_derived: bool = False, tracers=None, tracer_every: int = 1, forces=None, force_moments=None,
                 force_spectrum: Optional["Spectrum"] = None, wall_moments=None, modes=None) -> "RolloutErrors":
        """Roll the model out against `graph.target` ([N, >= num_fields * n_out]; n_out defaults to all the steps it holds) and return
        the error of every step (`RolloutErrors`: mse, mae, max_abs, r2 per step and field, `mae_masked` over the Dirichlet nodes
        `graph.omega[:, 0] == 1` when the graph has `omega`, `graph_loss(lambda_d)`), formed on the device inside the step — the
        predictions of every step are not held.  every = k > 0 also keeps the snapshots solve(every=k)
        returns (`.snapshots`), probes (1-D integer tensor of node rows) the prediction's time series there (`.probes`,
        [P, num_fields * n_out]).  moments / error_moments (None, True, `start` or `(start, stride)`, as in `Rollout`) also attach the
        per-node time statistics of the prediction / of prediction − target (`.moments` / `.error_moments`: `RolloutMoments`).
        derived (a tuple of names: 'div', 'vort', 'grad:<f>') with derived_every / derived_moments / derived_options, as in `Rollout`,
        attaches the flow diagnostics of the prediction (`.derived`: `RolloutDerived`).  spectrum (a `gfd.Spectrum`) attaches the
        Fourier modes of the prediction and, by the same table, of the target (`.spectrum` / `.target_spectrum`: `RolloutSpectrum`).
        samples (a `gfd.PointSampler` or points [P, dim]) with sample_every / sample_moments / sample_spectrum / sample_derived, as in
        `Rollout`, attaches the prediction at those points (`.samples`: `RolloutSamples`) and, as its `.target`, the target's first
        num_fields * n_out columns at the same points (one launch, outside the step).
        tracers (a `gfd.Tracers` or a tuple (seeds, dt)) with tracer_every, as in `Rollout`, attaches the particles carried by the
        prediction (`.tracers`: `RolloutTracers`) and, as its `.target_paths`, the paths of the same particles carried by the target:
        n_out launches outside the step, from the input field through the target's columns.
        forces (a `gfd.BodyForces` built on this graph) with force_moments / force_spectrum / wall_moments, as in `Rollout`, attaches
        the forces of the prediction on the bodies (`.forces`: `RolloutForces`) and, as its `.target`, those of the target's columns
        (one more launch inside the step).
        modes (a `gfd.Modes`; needs every >= 1: the kept snapshots are its data) attaches the modal analysis of the prediction and of
        the target's columns of the same steps (`.modes`: `.prediction`, `.target` — `SnapshotModes` — and `.alignment`, the principal
        cosines between the two mode subspaces), formed after the rollout: no launch inside the step.
        (The errors weighted by the nodes' control volumes — 'rel_l2', the mesh-independent relative L2 error — are `integrals()`'s.)
        A list of graphs is collated as in `solve`."""
        records = {k: v for k, v in locals().items() if k in KEYWORDS}          # (the keywords this signature shares with `Rollout`)
        if modes is not None:
            from ..modes import Modes
            if not isinstance(modes, Modes):
                raise TypeError(f"modes: expected a gfd.Modes, got {type(modes).__name__}")
            if int(every) < 1:
                raise ValueError("modes: the modes are formed from the kept snapshots: give every=k >= 1 (every=0 keeps none)")
        target = graph[0].target if type(graph) is list else graph.target
        if n_out is None:
            n_out = int(target.size(1)) // int(self.num_fields)
        assert n_out > 0, "n_out must be greater than 0."
        records.update(every=int(every), target_spectrum=spectrum is not None, target_forces=forces is not None)
        with self._rollout(graph, n_out, capture, "evaluate()", evaluate=True, **records) as ro:
            ro.run(n_out)
            errs = ro.errors()
            for name in ("forces", "tracers", "samples", "spectrum", "target_spectrum", "moments", "error_moments", "derived"):
                setattr(errs, name, getattr(ro, name)() if name in ro._parts else None)
            if errs.tracers is not None:
                errs.tracers.target_paths = ro._parts["tracers"].through_target(ro, n_out)
            if errs.samples is not None:
                tgt = ro._caller_graph.target.to(torch.float32)
                errs.samples.target = errs.samples.sampler.sample(tgt[:, :int(self.num_fields) * n_out])
            errs.modes = None
            if modes is not None:
                from ..modes import ModesComparison
                nf, k = int(self.num_fields), int(every)
                tgt = ro._rec.target[:, :nf * n_out].reshape(-1, n_out, nf).permute(1, 0, 2)[k - 1::k].contiguous()    # (the rollout's rows)
                errs.modes = ModesComparison(ro.modes(modes), modes._fit_steps(tgt, int(tgt.size(0)), ro._perm))
            return errs

    def diagnostics(self, graph: Union[Graph, List[Graph]], n_out: int, derived=("div", "vort"), *, every: int = 0, discard: Optional[int] = None,
                    stride: int = 1, capture: Optional[bool] = None, **derived_options) -> "RolloutDerived":
        """Roll the model out for n_out steps and return the flow diagnostics of every predicted step (`RolloutDerived`): the
        columns `derived` names — 'div' (divergence of the velocity), 'vort' (vorticity), 'grad:<f>' — formed on the device inside the
        step by the mesh's least-squares gradient (`gfd.MeshGradient`), with their `rms`, `mean_abs` and `max_abs` over the nodes per
        step.  No prediction is held.  every = k > 0 also keeps the derived columns of steps k - 1, 2k - 1, ... (`.snapshots`);
        discard = d (not None) their per-node time statistics over the steps d, d + stride, ... (`.moments`: `RolloutMoments` — the
        mean vorticity, its fluctuation).  derived_options: power, edge_vectors (periodic meshes: the wrapped, unscaled `edge_attr`
        of `ConnectKNN`), velocity, field_scale.  A list of graphs is collated as in `solve`."""
        assert n_out > 0, "n_out must be greater than 0."
        with self._rollout(graph, n_out, capture, "diagnostics()", every=0, derived=derived, derived_every=every,
                           derived_moments=None if discard is None else (discard, stride), derived_options=derived_options or None) as ro:
            ro.run(n_out)
            return ro.derived()

    def sample(self, graph: Graph, n_out: int, points, *, every: int = 1, discard: Optional[int] = None, stride: int = 1,
               spectrum: Optional["Spectrum"] = None, derived=None, capture: Optional[bool] = None, **derived_options) -> "RolloutSamples":
        """Roll the model out for n_out steps and return the prediction at `points` — a `gfd.PointSampler` built on this graph (a
        rake, a raster), or points [P, dim] off the nodes — (`RolloutSamples`), interpolated on the device inside the step by a
        linear moving-least-squares fit over the nearest nodes.  No prediction is held at the nodes.  every = k keeps the samples of
        steps k - 1, 2k - 1, ... (`.series`; 0 keeps none); discard = d (not None) their time statistics at every point over the steps
        d, d + stride, ... (`.moments`); spectrum (a `gfd.Spectrum`) their Fourier modes (`.spectrum`); derived (a tuple of names, as
        in `diagnostics`, with its derived_options) also samples those columns (`.derived`, `.columns`: the vorticity on a raster).
        One graph only: a list of graphs overlaps in space."""
        assert n_out > 0, "n_out must be greater than 0."
        with self._rollout(graph, n_out, capture, "sample()", every=0, samples=points, sample_every=every,
                           sample_moments=None if discard is None else (discard, stride), sample_spectrum=spectrum, derived=derived,
                           sample_derived=derived is not None, derived_options=derived_options or None) as ro:
            ro.run(n_out)
            return ro.samples()

    def trace(self, graph: Graph, n_out: int, seeds, dt: Optional[float] = None, *, every: int = 1, capture: Optional[bool] = None,
              **options) -> "RolloutTracers":
        """Roll the model out for n_out steps and return the particles its velocity carried (`RolloutTracers`: paths, last positions,
        status, stopped) — `seeds` [S, dim] with `dt` and the options of `gfd.Tracers` (scheme, k, power, velocity, scale, shift, box,
        max_distance, release, period — a periodic domain: `.paths` then hold wrapped positions), or a `gfd.Tracers` built on this graph (a streak) — advected on the device inside the step.  No
        prediction is held.  every = k keeps the positions after steps k - 1, 2k - 1, ... (`.paths`; 0 keeps none).  One graph only:
        a list of graphs overlaps in space."""
        assert n_out > 0, "n_out must be greater than 0."
        from ..tracers import Tracers
        if isinstance(seeds, Tracers):
            if dt is not None or options:
                raise ValueError("tracers: a gfd.Tracers carries its own dt and options")
            tracers = seeds
        else:
            tracers = (seeds, dt, options)
        with self._rollout(graph, n_out, capture, "trace()", every=0, tracers=tracers, tracer_every=every) as ro:
            ro.run(n_out)
            return ro.tracers()

    def forces(self, graph: Graph, n_out: int, bodies=None, *, discard: Optional[int] = None, stride: int = 1,
               spectrum: Optional["Spectrum"] = None, wall: bool = False, capture: Optional[bool] = None, **options) -> "RolloutForces":
        """Roll the model out for n_out steps and return the forces of every predicted step on the bodies in the flow
        (`RolloutForces`: pressure and viscous force and moment per step and body, `coefficients`, `strouhal`) — `bodies` a
        `gfd.BodyForces` built on this graph, or None / an integer label per wall node with the options of `gfd.BodyForces` (nodes,
        loops, centre, mu, pressure, velocity, scale, shift, gradient, power, edge_vectors), from which one is built here — formed on
        the device inside the step.  No prediction is held.  discard = d (not None) also accumulates the time statistics of the
        total force over the steps d, d + stride, ... (`.moments`: the mean drag, the r.m.s. lift) and, with wall=True, of the
        surface pressure and wall shear (`.wall_moments`); spectrum (a `gfd.Spectrum`) the Fourier modes of the total (`.spectrum`).
        One graph only: a list of graphs overlaps in space."""
        assert n_out > 0, "n_out must be greater than 0."
        from ..body_forces import BodyForces, check_forces
        if not isinstance(wall, bool):
            raise ValueError(f"wall: expected a bool, got {wall!r}")
        if wall and discard is None:
            raise ValueError("wall: the wall's time statistics need discard=")
        if type(graph) is list:
            raise ValueError("forces: a list of graphs is collated into one cloud in which the graphs overlap in space: take each graph's forces on its own")
        if isinstance(bodies, BodyForces):
            if options:
                raise ValueError(f"forces: a gfd.BodyForces carries its own options, got {sorted(options)}")
        else:
            check_forces(graph, options.get("nodes"), bodies, options.get("loops"), options.get("centre"),
                         **{k: v for k, v in options.items() if k not in ("nodes", "loops", "centre")})
            graph.to(self.device)
            bodies = BodyForces(graph, options.get("nodes"), bodies, options.get("loops"), options.get("centre"),
                                **{k: v for k, v in options.items() if k not in ("nodes", "loops", "centre")})
        window = None if discard is None else (discard, stride)
        with self._rollout(graph, n_out, capture, "forces()", every=0, forces=bodies, force_moments=window, force_spectrum=spectrum,
                           wall_moments=window if wall else None) as ro:
            ro.run(n_out)
            return ro.forces()

    def integrals(self, graph: Union[Graph, List[Graph]], n_out: int, names=("volume", "ke"), volumes=None, velocity=(0, 1), *,
                  capture: Optional[bool] = None, derived_options: Optional[dict] = None, **options) -> "RolloutIntegrals":
        """Roll the model out for n_out steps and return the integrals of every predicted step over the domain (`RolloutIntegrals`:
        `values` [steps, names], `drift(name)`), the node sums weighted by the nodes' control volumes — `volumes` a `gfd.ControlVolumes`
        of this graph, or None: one is built here (2-D; options box, bodies) —, formed on the device inside the step in fp64 in a
        fixed order.  names: 'volume', 'int:<f>', 'mean:<f>', 'ke' (½ ∫ |u|², `velocity` the fields of u and v), 'circulation' (∫ ω),
        'enstrophy' (½ ∫ ω²), 'div2' (∫ div²); the derived columns the last three read ('vort', 'div') are added by themselves, formed
        with `derived_options` (as in `diagnostics`).  'l2:<f>', 'l2' and 'rel_l2' — the errors against a target, 'rel_l2' =
        √(Σ_f ∫ (prediction − target)² / Σ_f ∫ target²) the mesh-independent relative L2 error — roll out against `graph.target`
        ([N, >= num_fields * n_out]), as `evaluate` does.  No prediction is held.  A list of graphs is collated as in `solve`: each
        graph gets its own cells."""
        assert n_out > 0, "n_out must be greater than 0."
        wanted = ((names,) if isinstance(names, str) else names) if isinstance(names, (str, tuple, list)) else ()
        need = [d for d, users in (("vort", ("circulation", "enstrophy")), ("div", ("div2",))) if any(u in wanted for u in users)]
        against = any(isinstance(nm, str) and (nm in ("l2", "rel_l2") or nm.startswith("l2:")) for nm in wanted)
        if against and not torch.is_tensor(getattr(graph[0] if type(graph) is list else graph, "target", None)):
            raise ValueError("integrals: 'l2:<f>', 'l2' and 'rel_l2' are errors against the target: the graph has no `target`")
        with self._rollout(graph, n_out, capture, "integrals()", evaluate=against, every=0, integrals=names, integral_volumes=volumes,
                           integral_options=dict(options, velocity=velocity), derived=tuple(need) or None,
                           derived_options=derived_options if need else None) as ro:
            ro.run(n_out)
            return ro.integrals()

    def time_statistics(self, graph: Union[Graph, List[Graph]], n_out: int, *, discard: int = 0, stride: int = 1, every: int = 0,
                        capture: Optional[bool] = None) -> "RolloutMoments":
        """Roll the model out for n_out steps and return the time statistics of the prediction at every node (`RolloutMoments`: mean,
        cov / var / std of the fields, per-node min and max) over the steps discard, discard + stride, ... < n_out (0-based),
        accumulated on the device inside the step in fp64.  No prediction is held (every = 0); every = k > 0 also keeps the
        snapshots solve(every=k) returns (`.snapshots`).  A list of graphs is collated as in `solve`."""
        assert n_out > 0, "n_out must be greater than 0."
        with self._rollout(graph, n_out, capture, "time_statistics()", every=int(every), moments=(discard, stride)) as ro:
            ro.run(n_out)
            mo = ro.moments()
            mo.snapshots = ro.result() if int(every) else None
            return mo

    def spectrum(self, graph: Union[Graph, List[Graph]], n_out: int, bins=None, freqs=None, *, discard: int = 0, stride: int = 1,
                 samples: Optional[int] = None, dt: float = 1.0, taper: str = "rect", derived=None, every: int = 0,
                 capture: Optional[bool] = None, **derived_options) -> "RolloutSpectrum":
        """Roll the model out for n_out steps and return the Fourier modes of the prediction at every node (`RolloutSpectrum`: coeff,
        amplitude, phase, power, band_power, dominant) at the frequencies `bins` or `freqs` name (`gfd.Spectrum`), over the samples
        discard, discard + stride, ... < n_out (0-based; `samples` of them, default all), accumulated on the device inside the step in
        fp64.  No prediction is held (every = 0); every = k > 0 also keeps the snapshots solve(every=k) returns (`.snapshots`).
        derived (a tuple of names, as in `diagnostics`, with its derived_options) also carries the spectrum of those columns
        (`.derived`: the mode shape of the vorticity at the shedding frequency).  A list of graphs is collated as in `solve`."""
        assert n_out > 0, "n_out must be greater than 0."
        spec = Spectrum(bins, freqs, start=discard, stride=stride, samples=samples, dt=dt, taper=taper)
        with self._rollout(graph, n_out, capture, "spectrum()", every=int(every), spectrum=spec, derived=derived,
                           derived_spectrum=spec if derived is not None else None, derived_options=derived_options or None) as ro:
            ro.run(n_out)
            sp = ro.spectrum()
            sp.snapshots = ro.result() if int(every) else None
            sp.derived = ro.derived_spectrum() if derived is not None else None
            return sp

    def welch(self, graph: Union[Graph, List[Graph]], n_out: int, segment: int, bins=None, freqs=None, *, overlap=0, discard: int = 0,
              stride: int = 1, dt: float = 1.0, taper: str = "hann", reference=None, track=None, target: bool = False,
              capture: Optional[bool] = None) -> "RolloutWelch":
        """Roll the model out for n_out steps and return the segment-averaged spectra of the prediction at every node (`RolloutWelch`:
        power, psd, band_power, dominant; with a reference cross, coherence, phase_lag; with tracked rows spectrogram,
        dominant_by_segment) — Welch's estimator over segments of `segment` samples of the steps discard, discard + stride, ... < n_out,
        side by side (overlap = 0) or half overlapping (0.5), at the frequencies `bins` or `freqs` name (`gfd.Welch`), accumulated on the
        device inside the step in fp64.  No prediction is held.  reference = (node, field): the coherence with and the phase lag behind
        that signal; reference = "target": against `graph.target` ([N, >= num_fields * n_out]) at the same node and field — what is left
        of the error once a slow phase drift is taken out — and then, or with target=True, `.target` is the spectrum of the target's
        columns.  A list of graphs is collated as in `solve`: node and track are rows of the collated graph."""
        assert n_out > 0, "n_out must be greater than 0."
        if not isinstance(target, bool):
            raise TypeError(f"target: expected a bool, got {target!r}")
        against = target or reference == "target"
        if against and not torch.is_tensor(getattr(graph[0] if type(graph) is list else graph, "target", None)):
            raise ValueError("welch: reference='target' and target=True roll out against the target: the graph has no `target`")
        spec = Welch(segment, bins, freqs, overlap=overlap, start=discard, stride=stride, dt=dt, taper=taper, reference=reference, track=track)
        with self._rollout(graph, n_out, capture, "welch()", evaluate=against, every=0, welch=spec, target_welch=against) as ro:
            ro.run(n_out)
            we = ro.welch()
            we.target = ro.target_welch() if against else None
            return we

    def evaluate_welch(self, graph: Union[Graph, List[Graph]], welch: "Welch", n_out: Optional[int] = None, *,
                       capture: Optional[bool] = None) -> "RolloutErrors":
        """`evaluate(graph, n_out)` with the spectral fidelity beside the errors of every step: `welch` (a `gfd.Welch`, as a rule with
        reference="target") attaches the segment-averaged spectra of the prediction and of the target's columns (`.welch` /
        `.target_welch`: `RolloutWelch`) — `.welch.coherence` per node, field and frequency separates wrong physics from a slow phase
        drift, which per-step errors cannot.  (`evaluate` keeps the signature its callers know; this is its entry for `welch`.)"""
        tgt = graph[0].target if type(graph) is list else graph.target
        if n_out is None:
            n_out = int(tgt.size(1)) // int(self.num_fields)
        assert n_out > 0, "n_out must be greater than 0."
        if not isinstance(welch, Welch):
            raise TypeError(f"welch: expected a gfd.Welch, got {welch!r}")
        with self._rollout(graph, n_out, capture, "evaluate_welch()", evaluate=True, every=0, welch=welch, target_welch=True) as ro:
            ro.run(n_out)
            errs = ro.errors()
            errs.welch, errs.target_welch = ro.welch(), ro.target_welch()
            return errs

    def modes(self, graph: Union[Graph, List[Graph]], n_out: int, modes=None, *, every: int = 1, capture: Optional[bool] = None, **spec):
        """Roll the model out for n_out steps and return the modal analysis of the predictions kept (`SnapshotModes`: POD singular
        values, energies, time coefficients and modes; with dmd=True the dynamic modes, their frequencies and growth rates) — `modes` a
        `gfd.Modes`, or its arguments as keywords (rank, energy, centre, node_weights, field_weights, start, stride, count, dt, dmd).
        every = k keeps steps k - 1, 2k - 1, ... as the snapshots; start / stride / count are in those.  Formed after the rollout from
        its own step-major buffer: a fp64 Gram matrix in a fixed order of summation (`g4c_snapshot_gram`), no launch inside the step.
        A list of graphs is collated as in `solve`: the modes are over the batched node set."""
        assert n_out > 0, "n_out must be greater than 0."
        from ..modes import Modes
        if modes is None:
            modes = Modes(**spec)
        elif not isinstance(modes, Modes):
            raise TypeError(f"modes: expected a gfd.Modes or None, got {type(modes).__name__}")
        elif spec:
            raise ValueError(f"modes: a gfd.Modes carries its own options, got {sorted(spec)}")
        if isinstance(every, bool) or not isinstance(every, int) or every < 1:
            raise ValueError(f"every: modes() keeps every k-th step as a snapshot, k >= 1, got {every!r}")
        modes.selection(n_out // every)                   # (argument errors before anything is moved)
        with self._rollout(graph, n_out, capture, "modes()", every=every) as ro:
            ro.run(n_out)
            return ro.modes(modes)

    def _rollout(self, graph, n_out: int, capture: Optional[bool], label: str, evaluate: bool = False, **records) -> "Rollout":
        """The Rollout of solve() / evaluate(): the graph (or the collated list) on the model's device, the capture default."""
        specs = _check_parts(records, graph, int(self.num_fields), n_out, evaluate)        # (argument errors before anything is collated or moved)
        self.eval()
        with torch.no_grad():
            if type(graph) is list:
                graph = collate(graph)
            else:
                graph.batch = torch.zeros(graph.num_nodes, dtype=torch.long, device=self.device)
            graph.to(self.device)
            if capture is None:
                capture = n_out >= 4 and os.environ.get("G4C_HIPGRAPH", "1") != "0"
            if ops.mlp_precision() == "f16x3":
                _warn_f16_range(graph)
            if evaluate:
                records["target"] = graph.target
                omega = getattr(graph, "omega", None)
                records["mask"] = (omega[:, 0] == 1) if torch.is_tensor(omega) else None
            return Rollout._checked(specs, self, graph, n_out, capture, label, **records)

    def invalidate_packed(self) -> None:
        """Declare every packed weight image stale (they are rebuilt on the next launch).  The images are keyed on the parameters'
        version counters, which updates that bypass autograd's bookkeeping do not advance (`p.data.copy_`, EMA / SWA `lerp_`, a manual
        broadcast, torch's `fused=True` optimisers): call this after any such update.  `fit`, `load_state_dict` and `_apply`
        (`.to()`, `.float()` ...) do it themselves; a live `Rollout` re-captures its hipGraph on the next step."""
        ops.bump_weights_epoch()

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        self.invalidate_packed()
        return out

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        ops.bump_weights_epoch()
        return out

    def shift_and_replace(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """Shift the fields in x by num_fields and replace the last num_fields with y (nn/model.py:323-327).
        Returns a new tensor; `solve` uses the fused in-place device kernel instead."""
        _lib.require_hip(x, y)
        out = torch.empty_like(x, memory_format=torch.contiguous_format)
        nf, w = self.num_fields, int(x.size(1))
        if w > nf:
            ops.copy_cols(x, out, 0, scol0=nf, width=w - nf)
        ops.copy_cols(y, out, w - nf, scol0=0, width=nf)
        return out

    def save_checkpoint(self, file_name: str, n_out: int = 1, epoch: int = 0, optimiser=None, scheduler=None, scaler=None):
        """Writes `{'arch', 'weights', ...}` in the reference's checkpoint format (nn/model.py:329-349)."""
        checkpoint = {'arch': self.arch, 'weights': self.state_dict(), 'n_out': n_out, 'epoch': epoch}
        if optimiser is not None:
            checkpoint['optimiser'] = optimiser.state_dict()
            checkpoint['lr'] = optimiser.param_groups[0]['lr']
        if scheduler is not None:
            checkpoint['scheduler'] = scheduler.state_dict()
        if scaler is not None:
            checkpoint['scaler'] = scaler.state_dict()
        torch.save(checkpoint, file_name)
        return

    @property
    def num_params(self):
        """Returns the number of trainable parameters."""
        return sum(p.numel() for p in self.parameters() if p.requires_grad)


FORWARD_VALIDATION = os.environ.get("G4C_FORWARD_VALIDATION", "1") != "0"


def set_forward_validation(on: bool) -> bool:
    """Bare `model.forward(graph)` calls in the default "f16x3" arithmetic read the fp16 range flags of their own launches when they
    return (one 16 KB device -> host copy = one synchronisation per call) and run again in "bf16x6" if a value was clipped.  Turn it
    off for forwards issued inside your own stream capture or a latency-critical loop (then `gfd.check_f16_range()` is yours to
    call).  Returns the previous setting."""
    global FORWARD_VALIDATION
    old, FORWARD_VALIDATION = FORWARD_VALIDATION, bool(on)
    return old


_spare_flags = {}       # device -> the flag buffer of a validated bare forward that returned (zero: take() clears what it finds)


def _range_checked_forward(f):
    import functools

    @functools.wraps(f)
    def forward(self, graph, *args, **kwargs):
        field = getattr(graph, "field", None)
        if (not FORWARD_VALIDATION or ops.StaticCache.active is not None or ops.mlp_precision() != "f16x3" or ops.grad_mode()
                or not torch.is_tensor(field) or field.device.type != "cuda" or torch.cuda.is_current_stream_capturing()):
            return f(self, graph, *args, **kwargs)          # (inside a rollout step / training / another arithmetic: validated elsewhere)
        # this call's launches report into a buffer of its own (a nested call finds none spare and makes one)
        flags = _spare_flags.pop(field.device, None) or ops.RangeFlags(field.device)
        with flags:
            out = f(self, graph, *args, **kwargs)
        hit = flags.take()
        _spare_flags[field.device] = flags
        if hit:
            warnings.warn(f"{type(self).__name__}.forward(): the default 'f16x3' MLP arithmetic reached the end of the fp16 range (|x| >= "
                          f"65504) in {', '.join(hit[:8])}{' ...' if len(hit) > 8 else ''}: the forward was computed again in 'bf16x6' (fp32's "
                          "exponent range) — the result holds no clipped value.  gfd.set_mlp_precision('bf16x6') avoids the second pass.",
                          RuntimeWarning, stacklevel=2)
            with ops.mlp_precision_as("bf16x6"):
                out = f(self, graph, *args, **kwargs)
        return out
    forward._g4c_range_checked = True
    return forward


F16_INPUT_WARN = 4096.0


def _warn_f16_range(graph: Graph) -> None:
    """The default "f16x3" MLP arithmetic has fp16's exponent range (ops.py; a rollout that leaves it is recomputed in "bf16x6":
    Rollout.validate).  Raw inputs go through the fp32 vector path, but the first hidden layer they feed is split into fp16: inputs
    of this size mean un-normalised data, where that layer can get there — say so up front.  One small reduction per input tensor
    and one synchronisation per solve() call."""
    big = []
    for name in ("field", "edge_attr", "loc", "glob", "omega"):
        x = getattr(graph, name, None)
        if torch.is_tensor(x) and x.is_floating_point() and x.numel():
            big.append(x.detach().abs().amax().reshape(1).float())
    if big and float(torch.cat(big).amax()) > F16_INPUT_WARN:
        warnings.warn(f"solve(): an input tensor has magnitudes beyond {F16_INPUT_WARN:g}: the default 'f16x3' MLP arithmetic (fp16 "
                      "exponent range, +-65504) will probably be left and the rollout recomputed in 'bf16x6' — "
                      "gfd.set_mlp_precision('bf16x6') runs un-normalised data in the full fp32 range straight away.",
                      RuntimeWarning)

