"""`Rollout`: the device-resident autoregressive rollout of one (model, Graph) pair, and everything that rides along in its step.

A step is the forward, the launches of the parts attached to it, and one closing launch (`Rollout._one`).  A part is a plain class
with one small surface (`_Part`): its keywords are checked on the host (`check`), it allocates everything once (`Part(ro, spec)`),
enqueues its launches of a step (`launch`), is told when steps are about to be taken again (`restart`) and hands out its result
(`read`).  `_PARTS` lists them in launch order; `Rollout` loops over those asked for and never reaches inside one.  `_check_parts`
turns the keywords into checked specs, once per call: `Rollout.__init__` calls it, and so does `GNN._rollout` before it collates or
moves anything.  The result classes (`RolloutErrors`, `RolloutMoments`, `RolloutSpectrum`, `RolloutDerived`, `RolloutSamples`,
`RolloutForces`, `RolloutIntegrals`, `RolloutWelch`) and the requests `Spectrum` and `Welch` live here too; nn/model.py re-exports every name."""
from __future__ import annotations

import functools
import inspect
import os
import warnings
from types import SimpleNamespace
from typing import Optional

import torch

from .. import _lib, ops
from .._stepper import StepDriver
from ..graph import Graph


REORDER_MIN_NODES = 50_000      # below, the gathered rows stay in L2 whatever the numbering


class Rollout(StepDriver):
    """Device-resident autoregressive rollout state for one (model, Graph) pair (GNN.solve,
    nn/model.py:303-321).

    `step()` = one forward + one `g4c_rollout_advance` (writes outputs[:, nf*t:nf*(t+1)], shifts the
    history window, bumps the device-side step counter).  The first step runs eagerly and builds all
    static plans / packed weights; with `capture=True` the second step is captured into a hipGraph and
    every later step is a replay: no host synchronisation, no per-kernel launch cost (`_stepper.StepDriver` decides which).
    The caller's `graph.field` is swapped for a private working copy and restored on close()."""

    def __init__(self, model: "GNN", graph: Graph, max_steps: int, capture: bool = True, reorder: Optional[bool] = None,
                 label: str = "Rollout", every: int = 1, probes: Optional[torch.Tensor] = None, target: Optional[torch.Tensor] = None,
                 mask: Optional[torch.Tensor] = None, moments=None, error_moments=None, derived=None, derived_every: int = 0,
                 derived_moments=None, derived_options: Optional[dict] = None, spectrum: Optional["Spectrum"] = None,
                 target_spectrum: bool = False, derived_spectrum: Optional["Spectrum"] = None, samples=None, sample_every: int = 1,
                 sample_moments=None, sample_spectrum: Optional["Spectrum"] = None, sample_derived: bool = False, tracers=None,
                 tracer_every: int = 1, forces=None, force_moments=None, force_spectrum: Optional["Spectrum"] = None, wall_moments=None,
                 target_forces: bool = False):
        """`reorder` (default: meshes of >= REORDER_MIN_NODES nodes, unless G4C_REORDER=0): run on a copy of the Graph whose level-1
        nodes are numbered along a Morton curve (reorder.py: the senders an edge tile gathers are then rows its neighbours
        just touched) and map the output rows back in `result()`; Graph layouts the renumbering does not know run as they are.

        Records (all opt-in; with none of them the step ends in `g4c_rollout_advance` and every prediction is kept, as `solve`
        does; with any, it ends in `g4c_rollout_advance_record`, which writes them inside the step, captured or not):
        `every` = k: keep steps k - 1, 2k - 1, ... (0-based) only — `result()` is [N, nf * (max_steps // k)] and the buffer has
        max_steps // k slots; 0 keeps none (`result()` raises).  `probes`: 1-D integer tensor of node rows (repeats allowed) —
        `probes()` is their predictions at every step, [P, nf * max_steps].  `target` [N, >= nf * max_steps] (and `mask` [N] bool:
        the Dirichlet nodes): `errors()` is the error of every step against it (`RolloutErrors`).  Rows are the caller's numbering.

        Time statistics at every node (opt-in, and no record in the sense above: the step keeps the closing launch it would have
        had, one `g4c_rollout_moments` launch per statistic goes in front of it): `moments` — of the prediction — and
        `error_moments` — of prediction − target, needs `target=` — are each None, True (every step), `start` (steps start,
        start + 1, ...) or `(start, stride)` (steps start, start + stride, ...; 0-based).  `moments()` / `error_moments()` return
        them (`RolloutMoments`); after `rewind()` or a recomputation they hold the steps taken since.

        Flow diagnostics (opt-in, no record either): `derived` — a tuple of names, 'div' (divergence of the velocity), 'vort'
        (vorticity: one column in 2-D, three in 3-D), 'grad:<f>' (dim columns), at most 8 columns — are formed from every prediction
        by the mesh's least-squares gradient (`gfd.MeshGradient`, built here on the rollout's own numbering): one `g4c_mesh_derived`
        launch and its statistics launch after the forward, in front of the moments and the closing launch.  `derived()` returns
        them (`RolloutDerived`): rms / mean_abs / max_abs over the nodes per step; with `derived_every` = k > 0 the columns of steps
        k - 1, 2k - 1, ...; with `derived_moments` (the forms `moments` takes) their per-node time statistics, by the same
        `g4c_rollout_moments`.  `derived_options`: power (0, 1, 2; default 2), edge_vectors ([E, dim], caller's edge order: the
        wrapped, unscaled `edge_attr` of a periodic mesh), velocity (the fields of the velocity components, default 0 .. dim - 1),
        field_scale ([nf], multiplied into the coefficients).  Steps run again after `rewind()` or a recomputation overwrite
        their slots.

        Fourier modes at every node (opt-in, no record either): `spectrum` — a `gfd.Spectrum`: K frequencies, a lattice of samples
        start, start + stride, ..., a taper — accumulates the discrete Fourier transform of the prediction at those frequencies, one
        `g4c_rollout_spectrum` launch per step after the moments, in front of the closing launch; `target_spectrum=True` (needs
        `target=` and `spectrum=`) the same of the target's columns, by the same table; `derived_spectrum` (a `gfd.Spectrum`, needs
        `derived=`) of the derived columns.  `spectrum()` / `target_spectrum()` / `derived_spectrum()` return them
        (`RolloutSpectrum`); after `rewind()` or a recomputation they hold the steps taken since.

        Values off the nodes (opt-in, no record either): `samples` — a `gfd.PointSampler` built on this graph, or points [P, dim] (a
        sampler with its defaults is built here) — interpolates every prediction to the points: one `g4c_sample_points` launch after
        the forward and the derived columns, in front of the node moments and spectra and of the closing launch; with
        `sample_derived=True` (needs `derived=`) one more on the derived columns.  `sample_every` = k keeps the samples of steps
        k - 1, 2k - 1, ... (0 keeps no series); `sample_moments` (the forms `moments` takes) and `sample_spectrum` (a `gfd.Spectrum`)
        accumulate the time statistics and Fourier modes of the sampled prediction at every point, by the kernels the nodes use.
        `samples()` returns them (`RolloutSamples`), the points in the caller's order; after `rewind()` or a recomputation the
        accumulators hold the steps taken since and the slots of the steps run again are overwritten.  A tensor of points is searched without
        a period; on a periodic mesh pass a `gfd.PointSampler(graph, points, period=...)`.  A list of graphs — they overlap in
        space — is refused.

        Lagrangian tracers (opt-in, no record either): `tracers` — a `gfd.Tracers` built on this graph, or a tuple (seeds [S, dim], dt)
        (tracers with their defaults are built here) — moves a copy of the particles through every step: one `g4c_tracer_advance`
        launch after the forward, in front of the closing launch (it reads the field window — time level t — and the prediction —
        level t + 1 — before the window is shifted); the velocity must be among the model's fields.  `tracer_every` = k keeps the
        positions after steps k - 1, 2k - 1, ... (0 keeps no series).  `tracers()` returns them (`RolloutTracers`), the particles in
        the caller's order.  `rewind()` continues from the current positions (release steps then count from the rewound step index); a
        recomputation starts again from the positions of the last `rewind()` (the seeds, without one).  A list of graphs is refused.

        Body forces (opt-in, no record either): `forces` — a `gfd.BodyForces` built on this graph — forms the pressure and viscous
        force and moment on every body from every prediction: one `g4c_body_forces` launch (one workgroup per body) after the forward,
        the derived columns and the samples, in front of the node moments and spectra and of the closing launch.  `force_moments` and
        `wall_moments` (the forms `moments` takes) accumulate the time statistics of the total (F_x, F_y, M) of every body and of
        (pressure, wall shear) at every wall item, `force_spectrum` (a `gfd.Spectrum`) the Fourier modes of the total — the lift's
        dominant frequency is the shedding frequency —, by the kernels the nodes use.  `target_forces=True` (needs `target=`) adds one
        more launch per step on the target's columns.  `forces()` returns them (`RolloutForces`); steps run again after `rewind()` or
        a recomputation overwrite their rows, the accumulators hold the steps taken since.  A list of graphs is refused.

        Integrals over the domain (opt-in, no record either; 2-D; keywords of `Rollout.open`, which takes every keyword of this
        signature and these three): `integrals` — a tuple of names: 'volume', 'int:<f>' (∫ field f),
        'mean:<f>' (∫ f / volume), 'ke' (½ ∫ |u|²), 'circulation' (∫ ω), 'enstrophy' (½ ∫ ω²), 'div2' (∫ div²) and, with `target=`,
        'l2:<f>' (√∫ (prediction − target)² of field f), 'l2' (over all fields) and 'rel_l2' (that over √∫ target²) — are the sums over the
        nodes weighted by the nodes' control volumes: `integral_volumes`, a `gfd.ControlVolumes` of this graph (None: one is built here,
        with `box` and `bodies` of `integral_options`), permuted into the rollout's numbering once.  'circulation' and 'enstrophy' read
        the 'vort' column, 'div2' the 'div' column of `derived=`, which must name them.  One `g4c_weighted_integrals` launch (and its
        one-workgroup sum) per source and step — the prediction, prediction − target, the target, the derived columns, as far as the
        names need them — behind the derived columns' launches.  `integral_options`: velocity (the fields of u and v, default (0, 1)),
        box, bodies.  `integrals()` returns them (`RolloutIntegrals`); steps run again after `rewind()` or a recomputation overwrite
        their rows.

        Segment-averaged spectra at every node (opt-in, no record either; keywords of `Rollout.open`): `welch` — a `gfd.Welch`: segments
        of L samples of a lattice, side by side or half overlapping, K frequencies, a taper, a reference — accumulates Welch's estimate
        of the power spectrum of the prediction and, with a reference (a node's signal, or the target at the same node), of the
        cross-spectrum with it: one `g4c_rollout_welch` call (two launches) per step behind the spectra, in front of the closing launch.
        `target_welch=True` (needs `target=` and `welch=`) the same of the target's columns.  `welch()` / `target_welch()` return them
        (`RolloutWelch`: power, psd, coherence, phase_lag, spectrogram); after `rewind()` or a recomputation they hold the segments
        closed since."""
        specs = _check_parts(locals(), graph, int(model.num_fields), int(max_steps), target is not None)
        self._build(specs, model, graph, max_steps, capture, reorder, label, every, probes, target, mask)

    @classmethod
    def open(cls, model: "GNN", graph: Graph, max_steps: int, *, capture: bool = True, reorder: Optional[bool] = None, label: str = "Rollout",
             **keywords) -> "Rollout":
        """`Rollout(model, graph, max_steps, ...)` with every record and part named by keyword: those of the constructor's signature and
        the parts that came after it — `integrals=`, `integral_volumes=`, `integral_options=`, `welch=`, `target_welch=` (`KEYWORDS` lists
        them all).  The
        constructor's own signature stays what its callers know."""
        if set(keywords) - set(KEYWORDS):
            raise TypeError(f"Rollout.open: unexpected keyword argument(s) {sorted(set(keywords) - set(KEYWORDS))}")
        kw = {**KEYWORDS, **keywords}
        specs = _check_parts(kw, graph, int(model.num_fields), int(max_steps), kw["target"] is not None)
        ro = cls.__new__(cls)
        ro._build(specs, model, graph, max_steps, capture, reorder, label, kw["every"], kw["probes"], kw["target"], kw["mask"])
        return ro

    @classmethod
    def _checked(cls, specs: dict, model: "GNN", graph: Graph, max_steps: int, capture: bool, label: str, **keywords) -> "Rollout":
        """The Rollout of keywords `_check_parts` has already turned into `specs` (`GNN._rollout`: before it collated or moved anything)."""
        if set(keywords) - set(KEYWORDS):
            raise TypeError(f"Rollout: unexpected keyword argument(s) {sorted(set(keywords) - set(KEYWORDS))}")
        ro, kw = cls.__new__(cls), {**KEYWORDS, **keywords}
        ro._build(specs, model, graph, max_steps, capture, None, label, kw["every"], kw["probes"], kw["target"], kw["mask"])
        return ro

    def _build(self, specs: dict, model, graph: Graph, max_steps: int, capture: bool, reorder, label: str, every, probes, target, mask) -> None:
        _lib.require_hip(graph.field)
        # (the records are checked here alone: `target`, `mask` and the probes' rows are those of the graph the rollout runs on)
        recording = _check_records(graph, int(model.num_fields), int(max_steps), every, probes, target, mask)
        self._caller_graph, self._perm = graph, None
        if reorder is None:
            reorder = graph.num_nodes >= REORDER_MIN_NODES and os.environ.get("G4C_REORDER", "1") != "0"
        if reorder:
            from ..reorder import reorder_nodes
            re = reorder_nodes(graph)
            if re is not None:
                graph, self._perm = re
        self.model, self.graph, self.label = model, graph, label
        self.nf = int(model.num_fields)
        dev = graph.field.device
        self._orig_field = graph.field
        field = graph.field.to(torch.float32).clone(memory_format=torch.contiguous_format)
        # step-major [steps, N, nf]: a step's predictions are one contiguous block (`outputs` gives the reference's [N, nf * steps])
        out_steps = None if recording else torch.zeros((int(max_steps), graph.num_nodes, self.nf), dtype=torch.float32, device=dev)
        self._init_driver(field, out_steps, max_steps, capture)
        self._rec = _Records(self, int(every), probes, target, mask) if recording else None     # (its snapshots are `_out_steps`)
        graph.field = self.field
        self._parts = {}                         # name -> part, of those asked for, in launch order (a part may read an earlier one's buffers)
        for part in _PARTS:
            if specs[part.name] is not None:
                self._parts[part.name] = part(self, specs[part.name])
            setattr(self, "_" + part.name, self._parts.get(part.name))      # (`ro._forces`: the part, None when it was not asked for)

    @functools.cached_property
    def _inv(self) -> Optional[torch.Tensor]:
        """The inverse of the renumbering: the caller's row r is the rollout's row _inv[r] (None when the rows are the caller's)."""
        if self._perm is None:
            return None
        inv = torch.empty_like(self._perm)
        inv[self._perm] = torch.arange(int(self.graph.num_nodes), device=self._perm.device)
        return inv

    def _to_caller(self, t: torch.Tensor) -> torch.Tensor:
        """`t` [N, ...] in the rollout's node numbering -> the same rows in the caller's."""
        if self._perm is None:
            return t
        out = torch.empty_like(t)
        out[self._perm] = t
        return out

    @property
    def outputs(self) -> torch.Tensor:
        """`StepDriver.outputs`, in the rollout's node numbering (`result()` is the delivered form)."""
        if self._out_steps is None:
            raise RuntimeError(f"{self.label}: every=0 keeps no snapshot of the predictions (probes() and errors() hold the records)")
        return StepDriver.outputs.fget(self)

    def _one(self):
        with self.static, self.flags:
            pred = self.model.forward(self.graph, self.steps_done)
        for part in self._parts.values():       # (all read the step index, and the window of level t, before the closing launch moves them)
            part.launch(self, pred)
        if self._rec is not None:
            self._rec.advance(self.field, pred, self.step_counter)
            return
        ops.rollout_advance(self.field, pred, self._out_steps, self.step_counter, self.nf)

    def rewind(self) -> None:
        """Restart writing at step 0 (benchmarks: keeps the captured hipGraph and the current field).  Validates first: the
        field a later recomputation restarts from must not come from steps that clipped."""
        self.validate()
        self.step_counter.zero_()
        self.steps_done = 1 if self.steps_done > 0 else 0
        if self.steps_done:   # slot 0 is kept so that replays continue from slot 1
            self.step_counter[:1].fill_(1)
        self._field0.copy_(self.field)            # (a recomputation restarts here)
        self._first_slot = self.steps_done
        self._restarted(False)

    def _restarted(self, again: bool) -> None:
        for part in self._parts.values():
            part.restart(self, again)

    def _warn_clipped(self, hit, n: int) -> None:
        warnings.warn(f"{self.label}: the default 'f16x3' MLP arithmetic reached the end of the fp16 range (|x| >= 65504) in "
                      f"{', '.join(hit[:8])}{' ...' if len(hit) > 8 else ''}: the {n} step(s) were recomputed in 'bf16x6' (fp32's exponent "
                      "range) and this rollout continues in it — the result holds no clipped value.  gfd.set_mlp_precision('bf16x6') "
                      "avoids the second pass for this model.", RuntimeWarning, stacklevel=3)      # (the caller of `validate()`)

    def _rerun(self, n: int) -> None:
        field, self.graph.field = self.graph.field, self.field        # (after close() the graph holds its own field again)
        try:
            self.run(n)
        finally:
            self.graph.field = field

    def result(self) -> torch.Tensor:
        """`outputs` with its rows in the caller's node numbering — validated first (`validate()`): the tensor returned never
        contains a value the default arithmetic clipped."""
        self.validate()
        return self._to_caller(self.outputs)

    def _deliver(self, asked: bool, complaint: str, read):
        """What every accessor below does: refuse what was not asked for, validate, read."""
        if not asked:
            raise RuntimeError(f"{self.label}: {complaint}")
        self.validate()
        return read()

    def _read(self, name: str, verb: str = "were"):
        return self._deliver(name in self._parts, f"no {name}= {verb} asked for", lambda: self._parts[name].read(self))

    def probes(self) -> torch.Tensor:
        """[P, nf * max_steps]: the predictions at the `probes=` rows, in the order given, step after step (columns of steps not yet
        taken are zero) — validated first, like `result()`."""
        return self._deliver(self._rec is not None and self._rec.probe_out is not None, "no probes= were given",
                             lambda: ops.steps_to_columns(self._rec.probe_out))

    def errors(self) -> "RolloutErrors":
        """The error of the `steps_done` steps taken against `target=` (`RolloutErrors`, fp64 host tensors) — validated first, like
        `result()`; one device -> host copy of [steps_done, nf, 6] sums."""
        return self._deliver(self._rec is not None and self._rec.stats is not None, "no target= was given", lambda: self._rec.read(self))

    def moments(self) -> "RolloutMoments":
        """The time statistics of the prediction at every node over the window `moments=` asked for (`RolloutMoments`, fp64 device
        tensors in the caller's rows) — validated first, like `result()`; one device -> host copy of two integers."""
        return self._read("moments")

    def error_moments(self) -> "RolloutMoments":
        """The same of prediction − target over the window `error_moments=` asked for: `mean` is the bias field, `mean² + var` the
        mean-square error at every node."""
        return self._read("error_moments")

    def spectrum(self) -> "RolloutSpectrum":
        """The Fourier modes of the prediction at every node at the frequencies `spectrum=` asked for (`RolloutSpectrum`, fp64 device
        tensors in the caller's rows) — validated first, like `result()`; one device -> host copy of two integers."""
        return self._read("spectrum", "was")

    def target_spectrum(self) -> "RolloutSpectrum":
        """The same of the target's columns of the steps taken, by the same table (`target_spectrum=True`)."""
        return self._read("target_spectrum", "was")

    def derived_spectrum(self) -> "RolloutSpectrum":
        """The same of the derived columns (`derived_spectrum=`): its fields are `derived().columns`."""
        return self._read("derived_spectrum", "was")

    def welch(self) -> "RolloutWelch":
        """The segment-averaged spectra of the prediction `welch=` asked for (`RolloutWelch`, fp64 device tensors in the caller's rows) —
        validated first, like `result()`; one device -> host copy of three integers per accumulator."""
        return self._read("welch", "was")

    def target_welch(self) -> "RolloutWelch":
        """The same of the target's columns of the steps taken, by the same tables (`target_welch=True`)."""
        part = self._parts.get("welch")
        return self._deliver(part is not None and part.spec["target_welch"], "no target_welch= was asked for", lambda: part.read_target(self))

    def derived(self) -> "RolloutDerived":
        """The flow diagnostics `derived=` asked for, of the `steps_done` steps taken (`RolloutDerived`) — validated first, like
        `result()`; one device -> host copy of [steps_done, nd, 3] sums."""
        return self._read("derived")

    def samples(self) -> "RolloutSamples":
        """What `samples=` asked for, of the steps taken (`RolloutSamples`: the series at the points, their time statistics and
        Fourier modes, the sampled derived columns) — validated first, like `result()`."""
        return self._read("samples")

    def tracers(self) -> "RolloutTracers":
        """What `tracers=` asked for, after the steps taken (`RolloutTracers`: the paths, the last positions, status, stopped) —
        validated first, like `result()`."""
        return self._read("tracers")

    def forces(self) -> "RolloutForces":
        """What `forces=` asked for, of the `steps_done` steps taken (`RolloutForces`: the pressure and viscous force and moment on
        every body per step, their time statistics and Fourier modes, the wall's statistics) — validated first, like `result()`; one
        device -> host copy of [steps_done, B, 6] sums."""
        return self._read("forces")

    def integrals(self) -> "RolloutIntegrals":
        """What `integrals=` asked for, of the `steps_done` steps taken (`RolloutIntegrals`: the integrals over the domain per step,
        weighted by the nodes' control volumes) — validated first, like `result()`; one device -> host copy of the sums."""
        return self._read("integrals")

    def modes(self, spec) -> "SnapshotModes":
        """The modal analysis `spec` (a `gfd.Modes`) asks for of the snapshots kept so far (`SnapshotModes`; mean and modes in the
        caller's rows) — validated first, like `result()`.  It reads the step-major buffer `result()` is a transposed copy of, and of it
        only the slots of steps taken; start / stride / count of `spec` are in kept slots.  Nothing is allocated or launched for it
        before this call."""
        from ..modes import Modes
        if not isinstance(spec, Modes):
            raise TypeError(f"modes: expected a gfd.Modes, got {type(spec).__name__}")
        every = self._rec.every if self._rec is not None else 1
        return self._deliver(self._out_steps is not None, "every=0 keeps no snapshot of the predictions to form modes of",
                             lambda: spec._fit_steps(self._out_steps, self.steps_done // every, self._perm))

    def close(self) -> None:
        self.graph.field = self._orig_field

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def _integer(v) -> bool:
    return isinstance(v, int) and not isinstance(v, bool)


def _check_every(name: str, every, kept: str) -> None:
    """An `every=` / `*_every=` argument: k keeps every k-th step, 0 none of the `kept`."""
    if not _integer(every) or every < 0:
        raise ValueError(f"{name}: expected an integer >= 0 (0: no {kept}, k: every k-th step), got {every!r}")


def _check_records(graph: Graph, nf: int, max_steps: int, every, probes, target, mask) -> bool:
    """The record arguments of `Rollout` against the caller's graph, on the tensors as they were passed (probe rows are read on the
    host copy the caller holds: nothing is uploaded first).  Returns whether any record was asked for."""
    n = int(graph.num_nodes)
    _check_every("every", every, "snapshots")
    if probes is not None:
        if not torch.is_tensor(probes) or probes.dtype.is_floating_point or probes.dtype == torch.bool or probes.is_complex():
            raise TypeError(f"probes: expected a 1-D integer tensor of node rows, got {getattr(probes, 'dtype', type(probes).__name__)}")
        if probes.dim() != 1:
            raise ValueError(f"probes: expected a 1-D integer tensor of node rows, got shape {tuple(probes.shape)}")
        if probes.numel() and (int(probes.min()) < 0 or int(probes.max()) >= n):
            raise ValueError(f"probes: rows {int(probes.min())} .. {int(probes.max())} of a graph of {n} nodes")
    if target is not None:
        if not torch.is_tensor(target) or not target.dtype.is_floating_point:
            raise TypeError(f"target: expected a floating-point tensor, got {getattr(target, 'dtype', type(target).__name__)}")
        if target.dim() != 2 or int(target.size(0)) != n or int(target.size(1)) < nf * max_steps:
            raise ValueError(f"target: expected [{n}, >= nf * max_steps = {nf * max_steps}], got {tuple(target.shape)}")
        if nf > _lib.REC_MAX_NF:
            raise NotImplementedError(f"target: the error statistics cover models of up to {_lib.REC_MAX_NF} fields, this one has {nf}")
    if mask is not None:
        if target is None:
            raise ValueError("mask: given without a target")
        if not torch.is_tensor(mask) or mask.dtype != torch.bool:
            raise TypeError(f"mask: expected a bool tensor, got {getattr(mask, 'dtype', type(mask).__name__)}")
        if tuple(mask.shape) != (n,):
            raise ValueError(f"mask: expected shape ({n},), got {tuple(mask.shape)}")
    return every != 1 or probes is not None or target is not None


def _check_moments(name: str, spec, nf: int, max_steps: int):
    """A `moments=` / `error_moments=` argument of `Rollout` -> (start, stride), or None when the statistic is not asked for."""
    if spec is None or spec is False:
        return None
    if spec is True:
        start, stride = 0, 1
    elif _integer(spec):
        start, stride = spec, 1
    elif isinstance(spec, (tuple, list)) and len(spec) == 2 and all(_integer(v) for v in spec):
        start, stride = spec
    else:
        raise TypeError(f"{name}: expected None, True, an integer start or a pair of integers (start, stride), got {spec!r}")
    if start < 0 or start >= max_steps:
        raise ValueError(f"{name}: start {start} of a rollout of {max_steps} steps (0 <= start < max_steps)")
    if stride < 1:
        raise ValueError(f"{name}: stride {stride} (>= 1)")
    if nf > _lib.REC_MAX_NF:
        raise NotImplementedError(f"{name}: the time statistics cover models of up to {_lib.REC_MAX_NF} fields, this one has {nf}")
    return int(start), int(stride)


def _lattice_origin(start: int, stride: int, first_slot: int) -> int:
    """The first step of the lattice start, start + stride, ... at or after `first_slot`."""
    behind = max(first_slot - start, 0)
    return start + -(-behind // stride) * stride


class _Part:
    """What `Rollout` asks of everything attached to its step — the classes of `_PARTS`, each with its `name`:
    `check(kw, ctx, specs)` (static): the caller's keywords `kw` -> a checked spec, or None when the part is not asked for.  On the host
    tensors as they were passed: neither the library nor a device is touched.  `ctx`: graphs (the caller's; more than one or
    `in_list`: a list to be collated), graph (the first), nf, max_steps, has_target; `specs`: those of the parts checked before it.
    `Part(ro, spec)`: allocates everything, once.  `launch(ro, pred)`: enqueues the part's launches of one step.
    `restart(ro, again)`: steps are about to be taken anew from `ro._first_slot` — after `rewind()`, or (`again`) once more from the
    last rewind because the first pass clipped.  `read(ro)`: the result object."""
    nested = ()         # the accumulators a part owns: launched behind its own launches and restarted with it, in this order

    def restart(self, ro: "Rollout", again: bool) -> None:
        for acc in self.nested:
            acc.restart(ro, again)


def _read(part: Optional[_Part], ro: "Rollout"):
    return None if part is None else part.read(ro)


class _Accumulator(_Part):
    """What `_Moments` and `_Spectrum` share: fp64 planes over the rows — the nodes, in the rollout's numbering, or `rows` of them
    (sample points, bodies, wall items: in the caller's order already) — of the samples `x` (None: the prediction), and the
    device-side window {origin, last} over the lattice start, start + stride, ...  The captured launch reads the origin on the
    device, so `restart()` — a two-integer fill on the stream, outside the graph — is all `rewind()` and a recomputation need: the
    step that finds itself at the origin stores the accumulators without reading them."""

    def __init__(self, ro: "Rollout", start: int, stride: int, planes: int, x: Optional[torch.Tensor], rows: Optional[int]):
        dev, self.node_rows = ro.field.device, rows is None
        self.max_steps, self.start, self.stride, self.x = ro.max_steps, start, stride, x
        self.planes = torch.zeros((planes, int(ro.graph.num_nodes) if rows is None else int(rows)), dtype=torch.float64, device=dev)
        self.window = torch.zeros(2, dtype=torch.int32, device=dev)
        self.restart(ro, False)

    def restart(self, ro: "Rollout", again: bool) -> None:
        """origin = the first step of the lattice start, start + stride, ... at or after the first slot; nothing accumulated yet."""
        self.origin = _lattice_origin(self.start, self.stride, ro._first_slot)
        self.window[:1].fill_(self.origin)
        self.window[1:].fill_(-1)

    def count(self):
        """(the number of samples accumulated, the origin they were counted from): one device -> host copy of two integers."""
        origin, last = self.window.tolist()
        return ((last - origin) // self.stride + 1 if last >= origin else 0), origin

    def rows(self, ro: "Rollout", planes: torch.Tensor) -> torch.Tensor:
        """[planes, rows] as accumulated -> [rows, planes], node rows in the caller's numbering."""
        cols = planes.t().contiguous()
        return ro._to_caller(cols) if self.node_rows else cols


class _Moments(_Accumulator):
    """The accumulators of one time statistic of a `Rollout` and the launch that updates them: 4 nf + nf (nf + 1) / 2 planes (pivot,
    sum, sum2, min, max) of the nf columns of the samples (default: the model's fields), less `sub` when given."""

    def __init__(self, ro: "Rollout", start: int, stride: int, sub: Optional[torch.Tensor] = None, x: Optional[torch.Tensor] = None,
                 nf: Optional[int] = None, rows: Optional[int] = None):
        self.nf, self.sub = ro.nf if nf is None else int(nf), sub
        nf, pairs = self.nf, ops.moment_pairs(self.nf)
        super().__init__(ro, start, stride, 4 * nf + pairs, x, rows)
        self.pivot, self.sum, self.sum2, self.lo, self.hi = self.planes.split((nf, nf, pairs, nf, nf))

    def launch(self, ro: "Rollout", pred: torch.Tensor) -> None:
        ops.rollout_moments(pred if self.x is None else self.x, ro.step_counter, self.nf, self.max_steps, self.window, self.pivot, self.sum,
                            self.sum2, self.lo, self.hi, stride=self.stride, sub=self.sub)

    def read(self, ro: "Rollout") -> "RolloutMoments":
        count, origin = self.count()
        return RolloutMoments(count, origin, self.stride, *(self.rows(ro, p) for p in (self.pivot, self.sum, self.sum2, self.lo, self.hi)))


class _NodeMoments(_Moments):
    name = "moments"

    @staticmethod
    def check(kw, ctx, specs):
        return _check_moments("moments", kw["moments"], ctx.nf, ctx.max_steps)

    def __init__(self, ro: "Rollout", window):
        super().__init__(ro, *window)


class _ErrorMoments(_Moments):
    name = "error_moments"

    @staticmethod
    def check(kw, ctx, specs):
        window = _check_moments("error_moments", kw["error_moments"], ctx.nf, ctx.max_steps)
        if window is not None and not ctx.has_target:
            raise ValueError("error_moments: the statistics of prediction - target need target=")
        return window

    def __init__(self, ro: "Rollout", window):
        super().__init__(ro, *window, sub=ro._rec.target)


class RolloutMoments:
    """Per-node time statistics of a rollout (`Rollout.moments()` / `error_moments()`, `GNN.time_statistics()`, `GNN.evaluate(moments=)`)
    over the `count` steps origin, origin + stride, ...: the raw fp64 sums, as the device accumulated them — `pivot` [N, nf] (the
    first sample), `sum` [N, nf] = Σ d, `sum2` [N, nf (nf + 1) / 2] = Σ d_f d_g over the pairs (0,0), (0,1), ..., (0,nf-1), (1,1), ...,
    with d = sample − pivot, and `min`, `max` [N, nf] of the samples — and, from them, `mean` = pivot + Σd / count, `cov`
    [N, nf, nf] = Σ d_f d_g / count − (Σd_f / count)(Σd_g / count) (symmetric, population-normalised; the shift by the first sample
    keeps it well-conditioned when the mean is far larger than the fluctuation), `var` = its diagonal, `std` = √max(var, 0).
    `count == 0` (no step of the window was taken) raises on the derived quantities.  Works on tensors of any device.
    `snapshots`: the rollout's `result()` when `GNN.time_statistics(every=)` kept any, else None.
    Non-finite samples: a NaN sample at a node makes `min` and `max` of that node and field NaN, as it makes `sum` and `mean` (they
    are NOT the extrema of the other samples), and they stay NaN for the rest of the window; ±inf are ordinary values.  Other nodes
    and fields are untouched."""

    def __init__(self, count: int, origin: int, stride: int, pivot: torch.Tensor, sum: torch.Tensor, sum2: torch.Tensor,
                 min: torch.Tensor, max: torch.Tensor, snapshots: Optional[torch.Tensor] = None):
        nf = int(pivot.size(-1))
        pairs = nf * (nf + 1) // 2
        for t, name, width in ((pivot, "pivot", nf), (sum, "sum", nf), (sum2, "sum2", pairs), (min, "min", nf), (max, "max", nf)):
            if t.dim() != 2 or tuple(t.shape) != (int(pivot.size(0)), width):
                raise ValueError(f"{name}: expected shape ({int(pivot.size(0))}, {width}), got {tuple(t.shape)}")
        self.count, self.origin, self.stride = int(count), int(origin), int(stride)
        self.pivot, self.sum, self.sum2, self.min, self.max, self.snapshots = pivot, sum, sum2, min, max, snapshots

    @property
    def fields(self) -> int:
        return int(self.pivot.size(1))

    def _n(self) -> float:
        if self.count <= 0:
            raise RuntimeError("RolloutMoments: no step of the window was accumulated (count == 0)")
        return float(self.count)

    @property
    def mean(self) -> torch.Tensor:
        return self.pivot + self.sum / self._n()

    @property
    def cov(self) -> torch.Tensor:
        n, nf = self._n(), self.fields
        s = self.sum / n
        f, g = torch.triu_indices(nf, nf, device=self.sum2.device)        # row-major upper triangle: the pair order of sum2
        c = self.sum2 / n - s[:, f] * s[:, g]
        out = torch.empty((int(s.size(0)), nf, nf), dtype=c.dtype, device=c.device)
        out[:, f, g] = c
        out[:, g, f] = c
        return out

    @property
    def var(self) -> torch.Tensor:
        return torch.diagonal(self.cov, dim1=1, dim2=2)

    @property
    def std(self) -> torch.Tensor:
        return self.var.clamp_min(0.0).sqrt()

    def __repr__(self):
        return (f"RolloutMoments(count={self.count}, origin={self.origin}, stride={self.stride}, fields={self.fields}, "
                f"nodes={int(self.pivot.size(0))})")


class Spectrum:
    """A request for the Fourier modes of a rollout at every node (`Rollout(spectrum=)`, `GNN.evaluate(spectrum=)`; `GNN.spectrum`
    builds one): the discrete Fourier transform at K chosen frequencies — `bins` (integers 0 <= b <= samples // 2: the frequencies
    b / (samples stride dt), the exact bins of the window) or `freqs` (cycles per unit of time, at most the Nyquist frequency
    0.5 / (stride dt)), exactly one of them — over the `samples` steps start, start + stride, ... (0-based; default: all of them up to
    the rollout's end), `dt` the time of one step, `taper` "rect" or "hann".  Checked when the rollout is built."""

    def __init__(self, bins=None, freqs=None, *, start: int = 0, stride: int = 1, samples: Optional[int] = None, dt: float = 1.0,
                 taper: str = "rect"):
        self.bins, self.freqs, self.start, self.stride, self.samples, self.dt, self.taper = bins, freqs, start, stride, samples, dt, taper

    def __repr__(self):
        which = f"bins={self.bins!r}" if self.bins is not None else f"freqs={self.freqs!r}"
        return f"Spectrum({which}, start={self.start}, stride={self.stride}, samples={self.samples}, dt={self.dt}, taper={self.taper!r})"


def _check_spectrum(name: str, spec, nf: int, max_steps: int):
    """A `spectrum=` / `derived_spectrum=` argument of `Rollout` -> the window and the host table (a dict: start, stride, samples, dt,
    taper, tw, w, freqs), or None when no spectrum is asked for.  Nothing is moved or allocated on a device."""
    if spec is None:
        return None
    if not isinstance(spec, Spectrum):
        raise TypeError(f"{name}: expected a gfd.Spectrum or None, got {spec!r}")
    if not _integer(spec.start) or not _integer(spec.stride) or not (spec.samples is None or _integer(spec.samples)):
        raise TypeError(f"{name}: start, stride and samples are integers (samples may be None), got {spec!r}")
    if isinstance(spec.dt, bool) or not isinstance(spec.dt, (int, float)):
        raise TypeError(f"{name}: dt: expected a number, got {spec.dt!r}")
    if not isinstance(spec.taper, str):
        raise TypeError(f"{name}: taper: expected 'rect' or 'hann', got {spec.taper!r}")
    if spec.start < 0 or spec.start >= max_steps:
        raise ValueError(f"{name}: start {spec.start} of a rollout of {max_steps} steps (0 <= start < max_steps)")
    if spec.stride < 1:
        raise ValueError(f"{name}: stride {spec.stride} (>= 1)")
    lattice = len(range(spec.start, max_steps, spec.stride))
    samples = lattice if spec.samples is None else spec.samples
    if samples < 1 or samples > lattice:
        raise ValueError(f"{name}: samples {samples} of the {lattice} steps {spec.start}, {spec.start + spec.stride}, ... < {max_steps} (1 <= samples <= {lattice})")
    try:
        tw, w, freqs = ops.spectrum_table(bins=spec.bins, freqs=spec.freqs, samples=samples, stride=spec.stride, dt=spec.dt, taper=spec.taper)
    except (TypeError, ValueError) as e:
        raise type(e)(f"{name}: {e}") from None
    if nf > _lib.REC_MAX_NF:
        raise NotImplementedError(f"{name}: the spectra cover up to {_lib.REC_MAX_NF} fields, got {nf}")
    if int(tw.size(1)) > _lib.SPECTRUM_MAX_BINS:
        raise NotImplementedError(f"{name}: {int(tw.size(1))} frequencies (at most {_lib.SPECTRUM_MAX_BINS} per spectrum)")
    return dict(start=int(spec.start), stride=int(spec.stride), samples=int(samples), dt=float(spec.dt), taper=spec.taper, tw=tw, w=w, freqs=freqs)


class _Spectrum(_Accumulator):
    """The accumulators of one spectrum of a `Rollout` and the launch that updates them: `ops.spectrum_planes(nf, K)` planes (pivot,
    sum, re, im) of nf columns of the samples (`x_step`, as `ops.rollout_spectrum` takes it: nf for the records' target, whose columns
    advance with the step), and the twiddle table `spec` (`_check_spectrum`) holds, uploaded once."""

    def __init__(self, ro: "Rollout", spec: dict, x: Optional[torch.Tensor] = None, x_step: int = 0, nf: Optional[int] = None,
                 rows: Optional[int] = None):
        self.nf, self.spec, self.x_step, self.K = ro.nf if nf is None else int(nf), spec, x_step, int(spec["tw"].size(1))
        nf = self.nf
        super().__init__(ro, spec["start"], spec["stride"], ops.spectrum_planes(nf, self.K), x, rows)
        self.pivot, self.sum, self.re, self.im = self.planes.split((nf, nf, nf * self.K, nf * self.K))
        self.tw = spec["tw"].to(ro.field.device)

    def launch(self, ro: "Rollout", pred: torch.Tensor) -> None:
        ops.rollout_spectrum(pred if self.x is None else self.x, ro.step_counter, self.nf, self.max_steps, self.window, self.tw, self.pivot,
                             self.sum, self.re, self.im, stride=self.stride, x_step=self.x_step)

    def read(self, ro: "Rollout") -> "RolloutSpectrum":
        count, origin = self.count()
        sp = self.spec
        return RolloutSpectrum(count, origin, self.stride, sp["dt"], sp["taper"], sp["freqs"], sp["tw"], sp["w"], self.rows(ro, self.pivot),
                               self.rows(ro, self.sum), self.rows(ro, self.re).unflatten(1, (self.nf, self.K)),
                               self.rows(ro, self.im).unflatten(1, (self.nf, self.K)))


class _NodeSpectrum(_Spectrum):
    name = "spectrum"

    @staticmethod
    def check(kw, ctx, specs):
        return _check_spectrum("spectrum", kw["spectrum"], ctx.nf, ctx.max_steps)


class _TargetSpectrum(_Spectrum):
    name = "target_spectrum"

    @staticmethod
    def check(kw, ctx, specs):
        if not isinstance(kw["target_spectrum"], bool):
            raise TypeError(f"target_spectrum: expected a bool, got {kw['target_spectrum']!r}")
        if kw["target_spectrum"] and (not ctx.has_target or specs["spectrum"] is None):
            raise ValueError("target_spectrum: the spectrum of the target needs target= and spectrum= (it uses the same table)")
        return specs["spectrum"] if kw["target_spectrum"] else None

    def __init__(self, ro: "Rollout", spec: dict):
        super().__init__(ro, spec, x=ro._rec.target, x_step=ro.nf)


class _DerivedSpectrum(_Spectrum):
    """(a part of its own, not nested in `_Derived`: its launch goes behind the node spectra)"""
    name = "derived_spectrum"

    @staticmethod
    def check(kw, ctx, specs):
        if specs["derived"] is None:
            if kw["derived_spectrum"] is not None:
                raise ValueError("derived_spectrum: the spectrum of the derived columns needs derived=")
            return None
        return _check_spectrum("derived_spectrum", kw["derived_spectrum"], specs["derived"]["nd"], ctx.max_steps)

    def __init__(self, ro: "Rollout", spec: dict):
        derived = ro._parts["derived"]
        super().__init__(ro, spec, x=derived.cur, nf=derived.nd)


class RolloutSpectrum:
    """Per-node Fourier modes of a rollout (`Rollout.spectrum()` / `target_spectrum()` / `derived_spectrum()`, `GNN.spectrum()`,
    `GNN.evaluate(spectrum=)`) at the K frequencies `freqs` (cycles per unit of time) over the `count` samples of the steps origin,
    origin + stride, ... (`samples` make the window `complete`): the raw fp64 sums, as the device accumulated them — `pivot` [N, nf]
    (the first sample), `sum` [N, nf] = Σ d, `re`, `im` [N, nf, K] = Σ_j d_j tw[j, k, 0 / 1] with d = sample − pivot — and the host table
    they were formed with (`tw` [samples, K, 2] = (w_j cos θ_jk, −w_j sin θ_jk), `w` [samples]: the taper).  From them, `mean` =
    pivot + Σd / count; `coeff` [N, nf, K] complex128 = ((re + i im) − (mean − pivot) W_k) / S with W_k = Σ_{j<count} tw[j, k] and S =
    Σ_{j<count} w_j — the tapered Fourier transform of sample − mean, normalised so that A cos(ωt + φ) on a bin (t counted from the
    origin) has coeff = (A / 2) e^{iφ}; `amplitude` = 2 |coeff|, `phase` = arg coeff, `power` = |coeff|²; `band_power(mask)` [nf, K]
    their sum over the (masked) nodes; `dominant(field, mask)` the frequency of the largest band power (× D / U: the Strouhal
    number).  `count == 0` raises on the derived quantities; a "hann" window that is not complete warns (its weights do not sum as
    a Hann window's).  Works on tensors of any device.  `snapshots`: the rollout's `result()` when `GNN.spectrum(every=)` kept any;
    `derived`: the spectrum of the derived columns when `GNN.spectrum(derived=)` asked for it; else None."""

    def __init__(self, count: int, origin: int, stride: int, dt: float, taper: str, freqs: torch.Tensor, tw: torch.Tensor, w: torch.Tensor,
                 pivot: torch.Tensor, sum: torch.Tensor, re: torch.Tensor, im: torch.Tensor, snapshots: Optional[torch.Tensor] = None):
        if tw.dim() != 3 or int(tw.size(2)) != 2 or tuple(w.shape) != (int(tw.size(0)),) or tuple(freqs.shape) != (int(tw.size(1)),):
            raise ValueError(f"tw: expected [samples, K, 2] with w [samples] and freqs [K], got {tuple(tw.shape)}, {tuple(w.shape)}, {tuple(freqs.shape)}")
        n, nf, K = int(pivot.size(0)), int(pivot.size(-1)), int(tw.size(1))
        for t, name, shape in ((pivot, "pivot", (n, nf)), (sum, "sum", (n, nf)), (re, "re", (n, nf, K)), (im, "im", (n, nf, K))):
            if tuple(t.shape) != shape:
                raise ValueError(f"{name}: expected shape {shape}, got {tuple(t.shape)}")
        self.count, self.samples, self.origin, self.stride, self.dt, self.taper = int(count), int(tw.size(0)), int(origin), int(stride), float(dt), taper
        if not 0 <= self.count <= self.samples:
            raise ValueError(f"count: {self.count} of a window of {self.samples} samples")
        self.freqs, self.tw, self.w = freqs, tw, w
        self.pivot, self.sum, self.re, self.im, self.snapshots, self.derived = pivot, sum, re, im, snapshots, None

    @property
    def fields(self) -> int:
        return int(self.pivot.size(1))

    @property
    def complete(self) -> bool:
        return self.count == self.samples

    def _n(self) -> float:
        if self.count <= 0:
            raise RuntimeError("RolloutSpectrum: no sample of the window was accumulated (count == 0)")
        return float(self.count)

    @property
    def mean(self) -> torch.Tensor:
        return self.pivot + self.sum / self._n()

    @property
    def coeff(self) -> torch.Tensor:
        n = self._n()
        if self.taper == "hann" and not self.complete:
            warnings.warn(f"RolloutSpectrum: {self.count} of the {self.samples} samples of a 'hann' window were accumulated: the taper was "
                          "cut off, the coefficients are those of the truncated weights", RuntimeWarning, stacklevel=2)
        tw, w = self.tw[:self.count].to(torch.float64), self.w[:self.count].to(torch.float64)
        W = torch.complex(tw[..., 0].sum(0), tw[..., 1].sum(0)).to(self.re.device)           # [K]
        S = float(w.sum())
        shift = (self.sum / n).to(torch.complex128).unsqueeze(-1) * W                          # (mean − pivot) W_k, [N, nf, K]
        return (torch.complex(self.re, self.im) - shift) / S

    @property
    def amplitude(self) -> torch.Tensor:
        return 2.0 * self.coeff.abs()

    @property
    def phase(self) -> torch.Tensor:
        return self.coeff.angle()

    @property
    def power(self) -> torch.Tensor:
        c = self.coeff
        return c.real ** 2 + c.imag ** 2

    def band_power(self, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """[nf, K]: the power summed over the nodes (`mask` bool [N]: over those nodes only)."""
        p = self.power
        if mask is not None:
            if not torch.is_tensor(mask) or mask.dtype != torch.bool or tuple(mask.shape) != (int(p.size(0)),):
                raise ValueError(f"mask: expected a bool tensor of shape ({int(p.size(0))},), got {getattr(mask, 'dtype', type(mask).__name__)} "
                                 f"{tuple(getattr(mask, 'shape', ()))}")
            p = p[mask.to(p.device)]
        return p.sum(0)

    def dominant(self, field: int = 0, mask: Optional[torch.Tensor] = None) -> float:
        """The frequency (of `freqs`) with the largest band power of `field`."""
        return float(self.freqs[int(self.band_power(mask)[field].argmax())])

    def __repr__(self):
        return (f"RolloutSpectrum(count={self.count}, samples={self.samples}, origin={self.origin}, stride={self.stride}, taper={self.taper!r}, "
                f"fields={self.fields}, bins={int(self.tw.size(1))}, nodes={int(self.pivot.size(0))})")


class Welch:
    """A request for segment-averaged spectra of a rollout at every node (`Rollout.open(welch=)`, `GNN.welch` builds one): Welch's
    estimator over segments of `segment` samples (L >= 2) of the lattice start, start + stride, ..., each tapered ("hann" or "rect"),
    its mean removed, transformed at K chosen frequencies — `bins` (integers 0 <= b <= L // 2: the frequencies b / (L stride dt)) or
    `freqs` (cycles per unit of time, at most the Nyquist frequency), exactly one of them — and averaged.  `overlap`: 0 (segments side
    by side) or 0.5 (each starts half a segment after the one before; L even).  `reference`: None, "target" (the rollout's target at
    the same node and field: the coherence of prediction and ground truth) or (node, field) in the caller's numbering (one signal for
    all nodes and fields: phase lags, the part of the wake locked to it) — with one, the cross-spectrum is averaged too.  `track`: node
    rows (caller's numbering, at most 1024, repeats allowed) whose power is also kept segment by segment (`spectrogram`).  A last
    partial segment contributes nothing.  Checked when the rollout is built."""

    def __init__(self, segment, bins=None, freqs=None, *, overlap=0, start: int = 0, stride: int = 1, dt: float = 1.0, taper: str = "hann",
                 reference=None, track=None):
        self.segment, self.bins, self.freqs, self.overlap, self.start, self.stride = segment, bins, freqs, overlap, start, stride
        self.dt, self.taper, self.reference, self.track = dt, taper, reference, track

    def __repr__(self):
        which = f"bins={self.bins!r}" if self.bins is not None else f"freqs={self.freqs!r}"
        return (f"Welch({self.segment}, {which}, overlap={self.overlap}, start={self.start}, stride={self.stride}, dt={self.dt}, "
                f"taper={self.taper!r}, reference={self.reference!r}, track={'None' if self.track is None else '[...]'})")


def _check_welch(name: str, spec, nf: int, max_steps: int, n_nodes: int, has_target: bool):
    """A `welch=` argument of `Rollout` -> the lattice, the segments and the host tables (a dict: start, stride, L, H, dt, taper, tw, w, W,
    freqs, reference — None, "target" or (node, field) —, track — None or a list of rows —, max_segments), or None when none is asked
    for.  Nothing is moved or allocated on a device."""
    if spec is None:
        return None
    if not isinstance(spec, Welch):
        raise TypeError(f"{name}: expected a gfd.Welch or None, got {spec!r}")
    if not _integer(spec.segment) or not _integer(spec.start) or not _integer(spec.stride):
        raise TypeError(f"{name}: segment, start and stride are integers, got {spec!r}")
    if isinstance(spec.dt, bool) or not isinstance(spec.dt, (int, float)):
        raise TypeError(f"{name}: dt: expected a number, got {spec.dt!r}")
    if not isinstance(spec.taper, str):
        raise TypeError(f"{name}: taper: expected 'rect' or 'hann', got {spec.taper!r}")
    if isinstance(spec.overlap, bool) or not isinstance(spec.overlap, (int, float)) or spec.overlap not in (0, 0.5):
        raise ValueError(f"{name}: overlap: expected 0 or 0.5 (segments side by side, or half overlapping), got {spec.overlap!r}")
    L = spec.segment
    if L < 2:
        raise ValueError(f"{name}: segment {L} (>= 2 samples)")
    if spec.overlap and L % 2:
        raise ValueError(f"{name}: overlap 0.5 needs an even segment, got segment {L}")
    H = L // 2 if spec.overlap else L
    if spec.start < 0 or spec.start >= max_steps:
        raise ValueError(f"{name}: start {spec.start} of a rollout of {max_steps} steps (0 <= start < max_steps)")
    if spec.stride < 1:
        raise ValueError(f"{name}: stride {spec.stride} (>= 1)")
    lattice = len(range(spec.start, max_steps, spec.stride))
    if lattice < L:
        raise ValueError(f"{name}: segment {L} of the {lattice} steps {spec.start}, {spec.start + spec.stride}, ... < {max_steps}: not one "
                         "segment would be complete")
    try:
        tw, w, freqs = ops.spectrum_table(bins=spec.bins, freqs=spec.freqs, samples=L, stride=spec.stride, dt=spec.dt, taper=spec.taper)
    except (TypeError, ValueError) as e:
        raise type(e)(f"{name}: {e}") from None
    if nf > _lib.REC_MAX_NF:
        raise NotImplementedError(f"{name}: the spectra cover up to {_lib.REC_MAX_NF} fields, got {nf}")
    if int(tw.size(1)) > _lib.SPECTRUM_MAX_BINS:
        raise NotImplementedError(f"{name}: {int(tw.size(1))} frequencies (at most {_lib.SPECTRUM_MAX_BINS} per spectrum)")
    reference = spec.reference
    if reference is not None and reference != "target":
        if (isinstance(reference, str) or not isinstance(reference, (tuple, list)) or len(reference) != 2
                or not all(_integer(v) for v in reference)):
            raise TypeError(f"{name}: reference: expected None, 'target' or a pair of integers (node, field), got {reference!r}")
        node, field = reference
        if not 0 <= node < n_nodes or not 0 <= field < nf:
            raise ValueError(f"{name}: reference: node {node} of {n_nodes} nodes, field {field} of {nf} fields")
        reference = (int(node), int(field))
    if reference == "target" and not has_target:
        raise ValueError(f"{name}: reference='target': the coherence with the target needs target=")
    track = spec.track
    if track is not None:
        if torch.is_tensor(track):
            if track.dtype.is_floating_point or track.dtype == torch.bool or track.is_complex() or track.dim() != 1:
                raise TypeError(f"{name}: track: expected a 1-D integer tensor or a sequence of node rows, got {track.dtype} {tuple(track.shape)}")
            track = track.tolist()
        elif isinstance(track, (str, bytes)) or not hasattr(track, "__iter__"):
            raise TypeError(f"{name}: track: expected a 1-D integer tensor or a sequence of node rows, got {track!r}")
        track = list(track)
        if not all(_integer(v) for v in track):
            raise TypeError(f"{name}: track: expected integers, got {track!r}")
        if len(track) > _lib.WELCH_MAX_TRACK:
            raise NotImplementedError(f"{name}: track: {len(track)} rows (at most {_lib.WELCH_MAX_TRACK})")
        if track and (min(track) < 0 or max(track) >= n_nodes):
            raise ValueError(f"{name}: track: rows {min(track)} .. {max(track)} of a graph of {n_nodes} nodes")
        track = track or None
    return dict(start=int(spec.start), stride=int(spec.stride), L=int(L), H=int(H), dt=float(spec.dt), taper=spec.taper, tw=tw, w=w,
                W=ops.welch_weights(tw), freqs=freqs, reference=reference, track=track, max_segments=(lattice - L) // H + 1)


class _WelchSet(_Accumulator):
    """One Welch accumulator of a `Rollout` and the call that updates it: `ops.welch_planes` planes (two alternating sets of pivot, sum,
    re, im; pxx; with a reference cxr_re, cxr_im) of the model's nf columns of the samples, the device-side window {origin, last,
    closed}, and the tables `spec` (`_check_welch`) holds, uploaded once.  `restart()` is a fill of the window alone: segment 0 stores."""

    def __init__(self, ro: "Rollout", spec: dict, reference: bool, x: Optional[torch.Tensor] = None, x_step: int = 0, tracked=None):
        dev, nf, K = ro.field.device, ro.nf, int(spec["tw"].size(1))
        self.node_rows, self.max_steps, self.start, self.stride, self.x, self.x_step = True, ro.max_steps, spec["start"], spec["stride"], x, x_step
        self.nf, self.K, self.spec, self.reference = nf, K, spec, reference
        self.planes = torch.zeros((ops.welch_planes(nf, K, reference), int(ro.graph.num_nodes)), dtype=torch.float64, device=dev)
        parts = self.planes.split(ops.welch_split(nf, K, reference))
        self.pivot, self.sum, self.re, self.im, self.pxx = parts[:5]
        self.cxr = tuple(parts[5:]) if reference else None
        self.window = torch.zeros(3, dtype=torch.int32, device=dev)
        self.tw, self.W = spec["tw"].to(dev), spec["W"].to(dev)
        self.track = self.track_host = self.seg_power = None
        if tracked is not None:
            self.track_host = tracked.to(torch.int32).cpu().contiguous()
            self.track = self.track_host.to(dev)
            self.seg_power = torch.zeros((spec["max_segments"], int(tracked.numel()), nf, K), dtype=torch.float64, device=dev)
        self.restart(ro, False)

    def restart(self, ro: "Rollout", again: bool) -> None:
        """origin = the first step of the lattice at or after the first slot; nothing accumulated, no segment closed."""
        self.origin = _lattice_origin(self.start, self.stride, ro._first_slot)
        self.window[:1].fill_(self.origin)
        self.window[1:2].fill_(-1)
        self.window[2:].fill_(0)

    def launch(self, ro: "Rollout", pred: torch.Tensor, ref=None, ref_row: int = -1, ref_field: int = -1) -> None:
        ops.rollout_welch(pred if self.x is None else self.x, ro.step_counter, self.nf, self.max_steps, self.window, self.tw, self.W, self.pivot,
                          self.sum, self.re, self.im, self.pxx, hop=self.spec["H"], stride=self.stride, x_step=self.x_step, cxr=self.cxr,
                          ref=ref, ref_row=ref_row, ref_field=ref_field, track=self.track, track_host=self.track_host,
                          seg_power=self.seg_power)

    def table(self, ro: "Rollout", planes: torch.Tensor) -> torch.Tensor:
        """[nf K, N] as accumulated -> [N, nf, K] in the caller's rows."""
        return self.rows(ro, planes).unflatten(1, (self.nf, self.K))


class _Welch(_Part):
    """The Welch spectra of a `Rollout`: the prediction's accumulator and, when `reference="target"` or `target_welch=True` asks for it,
    the one over the target's columns, which is launched first (the prediction's close reads its finished sums).  A reference node and
    the tracked rows are mapped into the rollout's numbering here, once."""
    name = "welch"

    @staticmethod
    def check(kw, ctx, specs):
        if not isinstance(kw["target_welch"], bool):
            raise TypeError(f"target_welch: expected a bool, got {kw['target_welch']!r}")
        n_nodes = sum(int(g.num_nodes) for g in ctx.graphs)
        spec = _check_welch("welch", kw["welch"], ctx.nf, ctx.max_steps, n_nodes, ctx.has_target)
        if kw["target_welch"] and (spec is None or not ctx.has_target):
            raise ValueError("target_welch: the Welch spectrum of the target needs target= and welch= (it uses the same tables)")
        return None if spec is None else dict(spec, target_welch=kw["target_welch"])

    def __init__(self, ro: "Rollout", spec: dict):
        dev, ref = ro.field.device, spec["reference"]
        self.spec, self.ref_row, self.ref_field = spec, -1, -1
        self.tgt = _WelchSet(ro, spec, False, x=ro._rec.target, x_step=ro.nf) if (ref == "target" or spec["target_welch"]) else None
        tracked = None
        if spec["track"] is not None:
            tracked = torch.tensor(spec["track"], dtype=torch.long)
            if ro._perm is not None:
                tracked = ro._inv.cpu()[tracked]
        if ref is not None and ref != "target":
            self.ref_row, self.ref_field = (ref[0] if ro._perm is None else int(ro._inv[ref[0]])), ref[1]
        self.pred = _WelchSet(ro, spec, ref is not None, tracked=tracked)
        self.nested = [acc for acc in (self.tgt, self.pred) if acc is not None]
        self.device = dev

    def launch(self, ro: "Rollout", pred: torch.Tensor) -> None:
        if self.tgt is not None:
            self.tgt.launch(ro, pred)
        if self.spec["reference"] == "target":
            self.pred.launch(ro, pred, ref=(self.tgt.sum, self.tgt.re, self.tgt.im))
        else:
            self.pred.launch(ro, pred, ref_row=self.ref_row, ref_field=self.ref_field)

    def _result(self, ro: "Rollout", acc: _WelchSet, **more) -> "RolloutWelch":
        sp = self.spec
        origin, _, closed = acc.window.tolist()
        return RolloutWelch(closed, origin, sp["stride"], sp["L"], sp["H"], sp["dt"], sp["taper"], sp["freqs"], sp["w"], acc.table(ro, acc.pxx), **more)

    def read_target(self, ro: "Rollout") -> "RolloutWelch":
        return self._result(ro, self.tgt)

    def read(self, ro: "Rollout") -> "RolloutWelch":
        acc, ref, more = self.pred, self.spec["reference"], {}
        pxx = acc.table(ro, acc.pxx)
        if ref is not None:
            more.update(cxr_re=acc.table(ro, acc.cxr[0]), cxr_im=acc.table(ro, acc.cxr[1]), reference=ref,
                        ref_pxx=self.tgt.table(ro, self.tgt.pxx) if ref == "target" else pxx[ref[0], ref[1]].reshape(1, 1, -1))
        if acc.seg_power is not None:
            closed = int(acc.window[2])
            more.update(seg_power=acc.seg_power[:closed].clone(), track=torch.tensor(self.spec["track"], dtype=torch.long))
        return self._result(ro, acc, **more)


class RolloutWelch:
    """Segment-averaged spectra of a rollout at every node (`Rollout.welch()` / `target_welch()`, `GNN.welch()`) at the K frequencies
    `freqs` (cycles per unit of time) over the `segments` closed segments of `segment` samples, `hop` samples apart, of the steps origin,
    origin + stride, ...: the raw fp64 sums, as the device accumulated them — `pxx` [N, nf, K] = Σ_s |A_s|², A_s the tapered transform of
    segment s with its mean removed; with a reference R, `cxr_re`, `cxr_im` [N, nf, K] = Σ_s A_s conj(R_s) and `ref_pxx` (Σ_s |R_s|²,
    broadcast against pxx); with tracked rows `seg_power` [segments, P, nf, K] = |A_s|² at the rows `track` — and the taper `w` with `S` =
    Σw and `S2` = Σw².  From them, `power` = pxx / (segments S²) — A cos(ωt + φ) on a bin gives (A / 2)², the scale of
    `RolloutSpectrum.power` —; `psd` the one-sided density power S² / (fs S2), fs = 1 / (stride dt), doubled away from 0 and the Nyquist
    frequency; `cross` = (cxr_re + i cxr_im) / (segments S²), complex; `coherence` = |Σ A conj R|² / (Σ|A|² Σ|R|²) in [0, 1] (identically 1
    after one segment; NaN where either power is zero); `phase_lag` = arg cross, the phase of the node minus that of the reference;
    `band_power(mask)` [nf, K] and `dominant(field, mask)` as in `RolloutSpectrum`; `spectrogram` = seg_power / S² and
    `dominant_by_segment(p, field)` [segments]: the frequency of the largest power of tracked row p in every segment — its drift over
    the rollout.  `segments == 0` raises on the derived quantities.  Works on tensors of any device.  `target`: the spectrum of the
    target's columns when `GNN.welch` formed it, else None."""

    def __init__(self, segments: int, origin: int, stride: int, segment: int, hop: int, dt: float, taper: str, freqs: torch.Tensor,
                 w: torch.Tensor, pxx: torch.Tensor, cxr_re: Optional[torch.Tensor] = None, cxr_im: Optional[torch.Tensor] = None,
                 ref_pxx: Optional[torch.Tensor] = None, seg_power: Optional[torch.Tensor] = None, track: Optional[torch.Tensor] = None,
                 reference=None):
        if pxx.dim() != 3 or tuple(freqs.shape) != (int(pxx.size(2)),) or tuple(w.shape) != (int(segment),):
            raise ValueError(f"pxx: expected [N, nf, K] with freqs [K] and w [segment], got {tuple(pxx.shape)}, {tuple(freqs.shape)}, {tuple(w.shape)}")
        if (cxr_re is None) != (cxr_im is None) or (cxr_re is None) != (ref_pxx is None):
            raise ValueError("cxr_re: a cross-spectrum is cxr_re, cxr_im and ref_pxx together")
        for t, name in ((cxr_re, "cxr_re"), (cxr_im, "cxr_im")):
            if t is not None and t.shape != pxx.shape:
                raise ValueError(f"{name}: expected shape {tuple(pxx.shape)}, got {tuple(t.shape)}")
        if seg_power is not None and (track is None or seg_power.dim() != 4 or int(seg_power.size(0)) != int(segments)
                                      or tuple(seg_power.shape[1:]) != (int(track.numel()),) + tuple(pxx.shape[1:])):
            raise ValueError(f"seg_power: expected [segments, P, nf, K] with track [P], got {tuple(seg_power.shape)}")
        if int(segments) < 0:
            raise ValueError(f"segments: {segments}")
        self.segments, self.origin, self.stride, self.segment, self.hop = int(segments), int(origin), int(stride), int(segment), int(hop)
        self.dt, self.taper, self.freqs, self.w = float(dt), taper, freqs, w
        self.S, self.S2 = float(w.to(torch.float64).sum()), float((w.to(torch.float64) ** 2).sum())
        self.pxx, self.cxr_re, self.cxr_im, self.ref_pxx, self.seg_power, self.track = pxx, cxr_re, cxr_im, ref_pxx, seg_power, track
        self.reference, self.target = reference, None

    @property
    def fields(self) -> int:
        return int(self.pxx.size(1))

    def _norm(self) -> float:
        if self.segments <= 0:
            raise RuntimeError("RolloutWelch: no segment was closed (segments == 0)")
        return float(self.segments) * self.S * self.S

    def _crossed(self):
        if self.cxr_re is None:
            raise RuntimeError("RolloutWelch: no reference= was asked for: there is no cross-spectrum")
        return self._norm()

    @property
    def power(self) -> torch.Tensor:
        return self.pxx / self._norm()

    @property
    def psd(self) -> torch.Tensor:
        fs = 1.0 / (self.stride * self.dt)
        f = self.freqs.to(torch.float64)
        sides = (1.0 + ((f > 0) & (f < 0.5 * fs * (1.0 - 1e-12))).to(torch.float64)).to(self.pxx.device)
        return self.power * (self.S * self.S / (fs * self.S2)) * sides

    @property
    def cross(self) -> torch.Tensor:
        norm = self._crossed()
        return torch.complex(self.cxr_re, self.cxr_im) / norm

    @property
    def coherence(self) -> torch.Tensor:
        self._crossed()
        return (self.cxr_re ** 2 + self.cxr_im ** 2) / (self.pxx * self.ref_pxx.to(self.pxx.device))

    @property
    def phase_lag(self) -> torch.Tensor:
        self._crossed()
        return torch.atan2(self.cxr_im, self.cxr_re)

    def band_power(self, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """[nf, K]: the power summed over the nodes (`mask` bool [N]: over those nodes only)."""
        p = self.power
        if mask is not None:
            if not torch.is_tensor(mask) or mask.dtype != torch.bool or tuple(mask.shape) != (int(p.size(0)),):
                raise ValueError(f"mask: expected a bool tensor of shape ({int(p.size(0))},), got {getattr(mask, 'dtype', type(mask).__name__)} "
                                 f"{tuple(getattr(mask, 'shape', ()))}")
            p = p[mask.to(p.device)]
        return p.sum(0)

    def dominant(self, field: int = 0, mask: Optional[torch.Tensor] = None) -> float:
        """The frequency (of `freqs`) with the largest band power of `field`."""
        return float(self.freqs[int(self.band_power(mask)[field].argmax())])

    @property
    def spectrogram(self) -> torch.Tensor:
        """[segments, P, nf, K]: the power of every closed segment at the tracked rows, on the scale of `power`."""
        if self.seg_power is None:
            raise RuntimeError("RolloutWelch: no track= was asked for: there is no per-segment power")
        self._norm()
        return self.seg_power / (self.S * self.S)

    def dominant_by_segment(self, p: int = 0, field: int = 0) -> torch.Tensor:
        """[segments]: the frequency (of `freqs`) of the largest power of tracked row `p`, field `field`, in every closed segment."""
        return self.freqs.to(self.spectrogram.device)[self.spectrogram[:, p, field].argmax(dim=1)]

    def __repr__(self):
        return (f"RolloutWelch(segments={self.segments}, segment={self.segment}, hop={self.hop}, origin={self.origin}, stride={self.stride}, "
                f"taper={self.taper!r}, fields={self.fields}, bins={int(self.pxx.size(2))}, nodes={int(self.pxx.size(0))}, "
                f"reference={self.reference!r})")


class _Derived(_Part):
    """The flow diagnostics of a `Rollout` and the launches that form them.  Everything is allocated here, once, in the rollout's
    node numbering: the operator (`MeshGradient` on the rollout's own graph — the caller's edge vectors follow the renumbered
    edges), the program, `cur` [N, nd], the per-step sums [max_steps, nd, 3] with their scratch, the snapshot slots, and the
    accumulators of `g4c_rollout_moments` over `cur` (those of `g4c_rollout_spectrum` over it are `_DerivedSpectrum`)."""
    name = "derived"

    @staticmethod
    def check(kw, ctx, specs):
        """The `derived*=` arguments against the caller's graph(s) -> names, every, window or None, options, nd."""
        from ..mesh_gradient import check_mesh, derived_terms
        derived, every, moments = kw["derived"], kw["derived_every"], kw["derived_moments"]
        if derived is None or derived is False:
            if (every not in (0, None)) or moments not in (None, False) or kw["derived_options"]:
                raise ValueError("derived: derived_every / derived_moments / derived_options were given without derived=")
            return None
        for graph in ctx.graphs:              # (every graph of a list in full before the next)
            _check_every("derived_every", every, "snapshots")
            options = dict(kw["derived_options"] or {})
            unknown = set(options) - {"power", "edge_vectors", "velocity", "field_scale"}
            if unknown:
                raise ValueError(f"derived_options: unknown option(s) {sorted(unknown)} (power, edge_vectors, velocity, field_scale)")
            if ctx.in_list and options.get("edge_vectors") is not None:
                raise ValueError("derived_options: edge_vectors of a list of graphs: collate the graphs and their edge vectors yourself")
            dim = check_mesh(graph, options.get("power", 2), options.get("edge_vectors"))
            names = (derived,) if isinstance(derived, str) else derived
            terms = derived_terms(names, dim, ctx.nf, options.get("velocity"), options.get("field_scale"))
            window = _check_moments("derived_moments", moments, len(terms), ctx.max_steps)
        return dict(names=tuple(names), every=int(every), window=window, options=options, nd=len(terms))

    def __init__(self, ro: "Rollout", spec: dict):
        from ..mesh_gradient import MeshGradient
        dev, n, names, every, options = ro.field.device, int(ro.graph.num_nodes), spec["names"], spec["every"], spec["options"]
        ev = options.get("edge_vectors")
        if ev is not None:
            ev = ev.to(dev)
            if ro._perm is not None:          # reorder.reorder_nodes: the edges re-sorted stably by their new target
                ev = ev[torch.argsort(ro._inv[ro._caller_graph.edge_index[1].to(ro._inv.device)], stable=True).to(dev)]
        self.op = MeshGradient(ro.graph, options.get("power", 2), ev)
        self.names, self.columns = names, self.op.columns(names)
        self.program = self.op.program(names, ro.nf, options.get("velocity"), options.get("field_scale"))
        self.nd, self.every, self.max_steps = len(self.columns), every, ro.max_steps
        self.cur = torch.zeros((n, self.nd), dtype=torch.float32, device=dev)
        self.stats = torch.zeros((ro.max_steps, self.nd, _lib.DERIVED_NSTAT), dtype=torch.float64, device=dev)
        self.scratch = ops.mesh_derived_scratch(n, self.nd, dev)
        self.snap = torch.zeros((ro.max_steps // every, n, self.nd), dtype=torch.float32, device=dev) if every else None
        self.moments = None if spec["window"] is None else _Moments(ro, *spec["window"], x=self.cur, nf=self.nd)
        self.nested = [acc for acc in (self.moments,) if acc is not None]

    def launch(self, ro: "Rollout", pred: torch.Tensor) -> None:
        ops.mesh_derived(pred, self.op.off, self.op.g, self.op.src, self.program, self.cur, step=ro.step_counter, every=self.every,
                         snap=self.snap, stats=self.stats, scratch=self.scratch, max_steps=self.max_steps)
        for acc in self.nested:
            acc.launch(ro, pred)

    def read(self, ro: "Rollout") -> "RolloutDerived":
        return RolloutDerived(self.names, self.columns, self.stats[:ro.steps_done].cpu(), int(self.cur.size(0)),
                              snapshots=ro._to_caller(ops.steps_to_columns(self.snap)) if self.snap is not None else None,
                              moments=_read(self.moments, ro), degenerate=ro._to_caller(self.op.degenerate))


class RolloutDerived:
    """Flow diagnostics of a rollout (`Rollout.derived()`, `GNN.diagnostics()`, `GNN.evaluate(derived=)`): `names` as asked for,
    `columns` their nd labels, and per step taken `rms` = √(Σq² / N), `mean_abs` = Σ|q| / N and `max_abs` = max|q| over the N nodes,
    each [steps, nd] — from `sums` [steps, nd, 3] = (Σq², Σ|q|, max|q|), which the step accumulated on the device in fp64 in a fixed
    order (fp64 host tensors).  `snapshots` [N, nd * (max_steps // k)]: the columns of steps k - 1, 2k - 1, ... (`derived_every=k`), else
    None; `moments`: their per-node time statistics (`RolloutMoments`, `derived_moments=`), else None; `degenerate` bool [N]: the
    nodes whose neighbours do not span the space — their derivatives are 0.  Rows are the caller's numbering.
    Non-finite samples: a column that is NaN at any node of a step has `max_abs` = NaN at that step (not the maximum over the other
    nodes), as `rms` and `mean_abs` are; +inf where the largest |q| is.  Other steps and columns are untouched."""

    def __init__(self, names, columns, sums: torch.Tensor, n_nodes: int, snapshots: Optional[torch.Tensor] = None,
                 moments: Optional["RolloutMoments"] = None, degenerate: Optional[torch.Tensor] = None):
        self.names, self.columns, self.sums, self.n_nodes = tuple(names), list(columns), sums, int(n_nodes)
        self.snapshots, self.moments, self.degenerate = snapshots, moments, degenerate
        n = float(max(n_nodes, 1))
        self.rms = (sums[..., _lib.DERIVED_SQ] / n).sqrt()
        self.mean_abs = sums[..., _lib.DERIVED_ABS] / n
        self.max_abs = sums[..., _lib.DERIVED_MAX_ABS]

    def column(self, label: str) -> int:
        return self.columns.index(label)

    def __repr__(self):
        return f"RolloutDerived(columns={self.columns}, steps={int(self.sums.size(0))}, nodes={self.n_nodes})"


class _Samples(_Part):
    """The samples of a `Rollout` at points off the nodes and the launches that form them.  Everything is allocated here, once: the
    sampler (built on the caller's graph when points were given), its neighbour table mapped through the inverse of the rollout's
    renumbering — the same values then enter every sum in the same order, so the bits do not depend on `reorder` —, `cur` [P, nf], the
    series' slots, the same for the derived columns, and the accumulators of `g4c_rollout_moments` and `g4c_rollout_spectrum` over
    `cur` (P rows).  The points keep the caller's order: nothing is permuted on read."""
    name = "samples"

    @staticmethod
    def check(kw, ctx, specs):
        """The `samples=` / `sample_*=` arguments against the caller's graph -> samples, every, window, spectrum, sample_derived."""
        from ..point_sampler import PointSampler, check_points
        samples, every, moments, spectrum, sample_derived = (kw[k] for k in ("samples", "sample_every", "sample_moments", "sample_spectrum",
                                                                            "sample_derived"))
        if not isinstance(sample_derived, bool):
            raise ValueError(f"sample_derived: expected a bool, got {sample_derived!r}")
        if samples is None:
            if moments not in (None, False) or spectrum is not None or sample_derived:
                raise ValueError("samples: sample_moments / sample_spectrum / sample_derived were given without samples=")
            return None
        if ctx.in_list:
            raise ValueError("samples: a list of graphs is collated into one cloud in which the graphs overlap in space: sample each graph on its own")
        if isinstance(samples, PointSampler):
            if samples.n_nodes != int(ctx.graph.num_nodes):
                raise ValueError(f"samples: a PointSampler over {samples.n_nodes} nodes for a graph of {int(ctx.graph.num_nodes)}")
        else:
            try:
                check_points(ctx.graph, samples, None, 2)
            except ValueError as e:
                raise ValueError(f"samples: {e}") from None
        _check_every("sample_every", every, "series")
        if sample_derived and specs["derived"] is None:
            raise ValueError("sample_derived: the samples of the derived columns need derived=")
        for name, asked, what in (("sample_moments", moments not in (None, False), "time statistics"), ("sample_spectrum", spectrum is not None, "spectra")):
            if asked and ctx.nf > _lib.REC_MAX_NF:
                raise ValueError(f"{name}: the {what} cover up to {_lib.REC_MAX_NF} fields, this model has {ctx.nf}")
        try:
            window = _check_moments("sample_moments", moments, ctx.nf, ctx.max_steps)
            table = _check_spectrum("sample_spectrum", spectrum, ctx.nf, ctx.max_steps)
        except (TypeError, NotImplementedError) as e:
            raise ValueError(str(e)) from None
        return dict(samples=samples, every=int(every), window=window, spectrum=table, sample_derived=sample_derived)

    def __init__(self, ro: "Rollout", spec: dict):
        from ..point_sampler import PointSampler
        dev, nf, steps, samples, every = ro.field.device, ro.nf, ro.max_steps, spec["samples"], spec["every"]
        self.sampler = samples if isinstance(samples, PointSampler) else PointSampler(ro._caller_graph, samples)
        self.idx, self.coef = self.sampler._idx.to(dev), self.sampler._coef.to(dev)
        if ro._perm is not None:
            self.idx = ro._inv.to(dev)[self.idx.long()].to(torch.int32).contiguous()
        n = self.sampler.n_points
        self.every, self.max_steps = every, steps
        self.cur = torch.zeros((n, nf), dtype=torch.float32, device=dev)
        self.series = torch.zeros((steps // every, n, nf), dtype=torch.float32, device=dev) if every else None
        self.derived_cur = self.dcur = self.dseries = self.columns = None
        if spec["sample_derived"]:
            derived = ro._parts["derived"]
            self.columns, self.derived_cur = list(derived.columns), derived.cur
            self.dcur = torch.zeros((n, derived.nd), dtype=torch.float32, device=dev)
            self.dseries = torch.zeros((steps // every, n, derived.nd), dtype=torch.float32, device=dev) if every else None
        self.moments = None if spec["window"] is None else _Moments(ro, *spec["window"], x=self.cur, rows=n)
        self.spectrum = None if spec["spectrum"] is None else _Spectrum(ro, spec["spectrum"], x=self.cur, rows=n)
        self.nested = [acc for acc in (self.moments, self.spectrum) if acc is not None]

    def launch(self, ro: "Rollout", pred: torch.Tensor) -> None:
        step = ro.step_counter
        ops.sample_points(pred, self.idx, self.coef, self.cur, step=step, every=self.every, series=self.series, max_steps=self.max_steps)
        if self.dcur is not None:
            ops.sample_points(self.derived_cur, self.idx, self.coef, self.dcur, step=step, every=self.every, series=self.dseries,
                              max_steps=self.max_steps)
        for acc in self.nested:
            acc.launch(ro, pred)

    def read(self, ro: "Rollout") -> "RolloutSamples":
        return RolloutSamples(self.sampler, series=ops.steps_to_columns(self.series) if self.series is not None else None,
                              derived=ops.steps_to_columns(self.dseries) if self.dseries is not None else None, columns=self.columns,
                              moments=_read(self.moments, ro), spectrum=_read(self.spectrum, ro), fields=int(self.cur.size(1)))


class RolloutSamples:
    """A rollout at points off the nodes (`Rollout.samples()`, `GNN.sample()`, `GNN.evaluate(samples=)`): `sampler` (the
    `gfd.PointSampler`) with its `points` [P, dim], `distance` [P] (to the nearest node: mask the points inside a body or outside the
    domain by it) and `degenerate` [P]; `series` [P, nf * slots]: the sampled prediction of steps k - 1, 2k - 1, ... (`sample_every=k`;
    None with 0), laid out as `Rollout.probes()`; `derived` [P, nd * slots] and `columns`, the labels: the sampled derived columns
    (`sample_derived=True`), else None; `moments` / `spectrum`: the time statistics (`RolloutMoments`) and Fourier modes
    (`RolloutSpectrum`) of the sampled prediction at every point, else None; `target`: the ground truth at the points
    [P, nf * n_out], filled by `GNN.evaluate`.  `image(slot, column)` is one column of one slot as a raster, for a grid sampler.  The
    points are in the caller's order."""

    def __init__(self, sampler, series: Optional[torch.Tensor] = None, derived: Optional[torch.Tensor] = None, columns=None,
                 moments: Optional["RolloutMoments"] = None, spectrum: Optional["RolloutSpectrum"] = None, fields: int = 0):
        self.sampler, self.points, self.distance, self.degenerate = sampler, sampler.points, sampler.distance, sampler.degenerate
        self.series, self.derived, self.columns, self.moments, self.spectrum, self.fields = series, derived, columns, moments, spectrum, int(fields)
        self.target = None

    @property
    def slots(self) -> int:
        return 0 if self.series is None else int(self.series.size(1)) // max(self.fields, 1)

    def image(self, slot: int = -1, column=0) -> torch.Tensor:
        """Column `column` — a field number of the prediction, or a label of `columns` (the sampled derived columns) — of slot `slot`
        (negative: from the last) as a tensor of the sampler's `shape` (`PointSampler.grid`): entry [i, j] is the value at
        (x_i, y_j).  ValueError for a sampler that is no grid."""
        shape = getattr(self.sampler, "shape", None)
        if shape is None:
            raise ValueError("image: the sampler is no grid (PointSampler.grid builds one)")
        if isinstance(column, str):
            if self.derived is None or column not in self.columns:
                raise ValueError(f"column: {column!r} is no sampled derived column ({self.columns})")
            data, width, col = self.derived, len(self.columns), self.columns.index(column)
        else:
            if isinstance(column, bool) or not isinstance(column, int) or not 0 <= column < self.fields:
                raise ValueError(f"column: expected a field 0 .. {self.fields - 1} or a derived column's label, got {column!r}")
            data, width, col = self.series, self.fields, column
        if data is None:
            raise ValueError("image: no series was kept (sample_every=0)")
        slots = int(data.size(1)) // width
        if isinstance(slot, bool) or not isinstance(slot, int) or not -slots <= slot < slots:
            raise ValueError(f"slot: expected -{slots} <= slot < {slots}, got {slot!r}")
        return data[:, width * (slot % slots) + col].reshape(*shape)

    def __repr__(self):
        return (f"RolloutSamples(points={int(self.points.size(0))}, fields={self.fields}, slots={self.slots}, derived={self.columns}, "
                f"moments={self.moments is not None}, spectrum={self.spectrum is not None})")


class _Tracers(_Part):
    """The tracers of a `Rollout` and the launch that moves them.  Everything is allocated here, once: the cell grid over the
    rollout's own (possibly renumbered) positions, a copy of the particles, the series' slots.  The particles keep the caller's order
    and a neighbour sum runs nearest first whatever the nodes are called, so nothing is permuted on read and the bits do not depend on
    `reorder`.  x0 is the last nf columns of the field window, x1 the prediction."""
    name = "tracers"

    @staticmethod
    def check(kw, ctx, specs):
        """The `tracers=` / `tracer_every=` arguments against the caller's graph -> (the particles' description, every)."""
        from ..tracers import Tracers, check_tracers
        tracers, every, graph, nf = kw["tracers"], kw["tracer_every"], ctx.graph, ctx.nf
        _check_every("tracer_every", every, "series")
        if tracers is None:
            if every != 1:
                raise ValueError("tracers: tracer_every was given without tracers=")
            return None
        if ctx.in_list:
            raise ValueError("tracers: a list of graphs is collated into one cloud in which the graphs overlap in space: trace each graph on its own")
        if isinstance(tracers, Tracers):
            spec = tracers._spec
            if spec["n_nodes"] != int(graph.num_nodes):
                raise ValueError(f"tracers: Tracers over {spec['n_nodes']} nodes for a graph of {int(graph.num_nodes)}")
            if max(spec["velocity"]) >= nf:
                raise ValueError(f"tracers: velocity: fields {spec['velocity']} of a model of {nf} (the velocity must be among the model's fields)")
            return spec, int(every)
        if not isinstance(tracers, tuple) or len(tracers) not in (2, 3) or (len(tracers) == 3 and not isinstance(tracers[2], dict)):
            raise TypeError(f"tracers: expected a gfd.Tracers or a tuple (seeds, dt), got {type(tracers).__name__}")
        try:
            return check_tracers(graph, tracers[0], tracers[1], nf=nf, **(tracers[2] if len(tracers) == 3 else {})), int(every)
        except ValueError as e:
            raise ValueError(f"tracers: {e}") from None
        except TypeError as e:
            raise TypeError(f"tracers: {e}") from None

    def __init__(self, ro: "Rollout", spec):
        from ..tracers import TracerState
        self.state = TracerState(spec[0], ro.graph.pos.detach().to(ro.field.device, torch.float32).contiguous(), spec[1], ro.max_steps)
        self.state.save()                              # (a recomputation starts again from here)
        self.nf = ro.nf

    def launch(self, ro: "Rollout", pred: torch.Tensor) -> None:
        self.state.launch(ro.field[:, int(ro.field.size(1)) - self.nf:], pred, step=ro.step_counter)

    def restart(self, ro: "Rollout", again: bool) -> None:
        """`rewind()` continues from the current positions; a recomputation starts again from those of the last rewind."""
        (self.state.restore if again else self.state.save)()

    def through_target(self, ro: "Rollout", n_out: int) -> Optional[torch.Tensor]:
        """[P, dim * slots]: a copy of the same particles carried by the target instead — n_out launches outside the step: the first
        from the input field (level 0) to the target's first nf columns (level 1), then from column block to column block."""
        from ..tracers import TracerState
        st, nf, target = self.state, self.nf, ro._rec.target
        if not st.every:
            return None
        other = TracerState(st.spec, ro.graph.pos.detach().to(target.device, torch.float32).contiguous(), st.every, n_out)
        x0 = ro._orig_field.to(target.device, torch.float32)
        x0 = x0[:, int(x0.size(1)) - nf:]
        for t in range(n_out):
            x1 = target[:, nf * t:nf * (t + 1)]
            other.launch(x0, x1, t=t)
            x0 = x1
        return ops.steps_to_columns(other.series)

    def read(self, ro: "Rollout") -> "RolloutTracers":
        from ..tracers import RolloutTracers
        st = self.state
        return RolloutTracers(ops.steps_to_columns(st.series) if st.series is not None else None, st.q.clone(), st.status.clone(),
                              st.stopped.clone(), st.release, st.seeds, every=st.every, groups=st.spec["groups"])


class _Forces(_Part):
    """The body forces of a `Rollout` and the launches that form them.  Everything is allocated here, once: the wall items mapped
    through the inverse of the rollout's renumbering, the gradient's tables re-indexed to it — every node keeps its in-edges in the
    caller's CSR order, so the same values enter every sum in the same order and the bits do not depend on `reorder` —, the per-step
    sums [max_steps, B, 6], `cur` [B, 3], `wall` [W, 2], the same sums for the target, and the accumulators of `g4c_rollout_moments`
    and `g4c_rollout_spectrum` over `cur` (B rows) and `wall` (W rows).  Bodies and items keep the caller's order: nothing is permuted
    on read."""
    name = "forces"

    @staticmethod
    def check(kw, ctx, specs):
        """The `forces=` / `force_*=` / `wall_moments=` / `target_forces=` arguments against the caller's graph -> forces, window,
        wall_window, spectrum, target_forces."""
        from ..body_forces import BodyForces
        forces, force_moments, force_spectrum, wall_moments, target_forces = (kw[k] for k in ("forces", "force_moments", "force_spectrum",
                                                                                             "wall_moments", "target_forces"))
        nf = ctx.nf
        if not isinstance(target_forces, bool):
            raise TypeError(f"target_forces: expected a bool, got {target_forces!r}")
        if forces is None:
            if force_moments not in (None, False) or wall_moments not in (None, False) or force_spectrum is not None or target_forces:
                raise ValueError("forces: force_moments / force_spectrum / wall_moments / target_forces were given without forces=")
            return None
        if ctx.in_list:
            raise ValueError("forces: a list of graphs is collated into one cloud in which the graphs overlap in space: take each graph's forces on its own")
        if not isinstance(forces, BodyForces):
            raise TypeError(f"forces: expected a gfd.BodyForces built on this graph, got {type(forces).__name__}")
        if forces.n_nodes != int(ctx.graph.num_nodes):
            raise ValueError(f"forces: a BodyForces over {forces.n_nodes} nodes for a graph of {int(ctx.graph.num_nodes)}")
        if forces.fields_needed() > nf:
            raise ValueError(f"forces: the operator reads field {forces.fields_needed() - 1}, the model has {nf} field(s)")
        for name, v in (("scale", forces.scale), ("shift", forces.shift)):
            if v is not None and len(v) != nf:
                raise ValueError(f"forces: {name}: {len(v)} numbers for a model of {nf} field(s)")
        if target_forces and not ctx.has_target:
            raise ValueError("target_forces: the forces of the target need target=")
        window = _check_moments("force_moments", force_moments, 3, ctx.max_steps)
        wall_window = _check_moments("wall_moments", wall_moments, 2, ctx.max_steps)
        table = _check_spectrum("force_spectrum", force_spectrum, 3, ctx.max_steps)
        return dict(forces=forces, window=window, wall_window=wall_window, spectrum=table, target_forces=target_forces)

    def __init__(self, ro: "Rollout", spec: dict):
        forces, window, wall_window, spectrum, target_forces = (spec[k] for k in ("forces", "window", "wall_window", "spectrum", "target_forces"))
        dev, steps = ro.field.device, ro.max_steps
        self.op, self.nf, self.max_steps = forces, ro.nf, steps
        self.item, self.body_off = forces._item32.to(dev), forces.body_offsets.to(dev)
        self.area, self.unit, self.arm = forces.area.to(dev), forces.unit.to(dev), forces.arm.to(dev)
        self.constants = forces.constants()
        grad = forces.gradient if forces.mu != 0 else None
        self.off, self.g, self.src = (None, None, None) if grad is None else (grad.off.to(dev), grad.g.to(dev), grad.src.to(dev))
        if ro._perm is not None:
            perm, inv = ro._perm.to(dev), ro._inv.to(dev)
            self.item = inv[self.item.long()].to(torch.int32).contiguous()
            if grad is not None:                      # the rollout's node j owns the caller's segment of node perm[j], in its order
                off = self.off.long()
                deg = (off[1:] - off[:-1])[perm]
                new_off = torch.zeros_like(off)
                new_off[1:] = torch.cumsum(deg, 0)
                e = torch.arange(int(new_off[-1]), device=dev) + torch.repeat_interleave(off[:-1][perm] - new_off[:-1], deg)
                self.off, self.g = new_off.to(torch.int32), self.g[e].contiguous()
                self.src = inv[self.src[e].long()].to(torch.int32).contiguous()
        n_bodies, n_items = forces.n_bodies, forces.n_items
        self.stats = torch.zeros((steps, n_bodies, _lib.FORCES_NSUM), dtype=torch.float64, device=dev)
        self.cur = torch.zeros((n_bodies, 3), dtype=torch.float32, device=dev)
        self.wall = torch.zeros((n_items, 2), dtype=torch.float32, device=dev)
        self.moments = None if window is None else _Moments(ro, *window, x=self.cur, nf=3, rows=n_bodies)
        self.wall_moments = None if wall_window is None else _Moments(ro, *wall_window, x=self.wall, nf=2, rows=n_items)
        self.spectrum = None if spectrum is None else _Spectrum(ro, spectrum, x=self.cur, nf=3, rows=n_bodies)
        self.nested = [acc for acc in (self.moments, self.wall_moments, self.spectrum) if acc is not None]
        self.target = ro._rec.target if target_forces else None
        self.target_stats = torch.zeros_like(self.stats) if target_forces else None
        self.target_cur = torch.zeros_like(self.cur) if target_forces else None

    def _launch(self, x, step, stats, cur, wall, x_step) -> None:
        ops.body_forces(x, self.item, self.body_off, self.area, self.unit, self.arm, cur, **self.constants, off=self.off, g=self.g,
                        src=self.src, wall=wall, stats=stats, max_steps=self.max_steps, step=step, x_step=x_step)

    def launch(self, ro: "Rollout", pred: torch.Tensor) -> None:
        self._launch(pred, ro.step_counter, self.stats, self.cur, self.wall, 0)
        for acc in self.nested:
            acc.launch(ro, pred)
        if self.target is not None:
            self._launch(self.target, ro.step_counter, self.target_stats, self.target_cur, None, self.nf)

    def read(self, ro: "Rollout") -> "RolloutForces":
        return RolloutForces(self.stats[:ro.steps_done].cpu(), angle=self.op.angle, body_offsets=self.op.body_offsets,
                             moments=_read(self.moments, ro), wall_moments=_read(self.wall_moments, ro), spectrum=_read(self.spectrum, ro),
                             target=self.target_stats[:ro.steps_done].cpu() if self.target_stats is not None else None)


class RolloutForces:
    """The forces of a rollout on the bodies in the flow (`Rollout.forces()`, `GNN.forces()`, `GNN.evaluate(forces=)`), per step
    taken and body, fp64 host tensors: `pressure` [n, B, 3] = (F_x, F_y, M) of the pressure, `viscous` [n, B, 3] the same of the
    viscous stress, `total` their sum — from `sums` [n, B, 6] = (Fp_x, Fp_y, Fv_x, Fv_y, Mp, Mv), which the step formed on the device
    in fp64 in a fixed order.  `moments`: the time statistics of the total (F_x, F_y, M) of every body (`RolloutMoments` over B rows,
    `force_moments=`), `wall_moments`: of (pressure, wall shear) at every wall item (W rows, `wall_moments=` — the mean Cp(θ) against
    `angle` [W]; `body_offsets` [B + 1] delimits the bodies), `spectrum`: the Fourier modes of the total (`RolloutSpectrum`,
    `force_spectrum=`), each None when not asked for; `target` [n, B, 6]: the sums of the target's fields (`target_forces=True`,
    `GNN.evaluate(forces=)`), else None.  `coefficients(rho, U, D)` = (Cd, Cl, Cm) [n, B] = (F_x, F_y, M / D) / (½ rho U² D);
    `strouhal(D, U, body)` = the dominant frequency of that body's lift × D / U."""

    def __init__(self, sums: torch.Tensor, angle: Optional[torch.Tensor] = None, body_offsets: Optional[torch.Tensor] = None,
                 moments: Optional["RolloutMoments"] = None, wall_moments: Optional["RolloutMoments"] = None,
                 spectrum: Optional["RolloutSpectrum"] = None, target: Optional[torch.Tensor] = None):
        if sums.dim() != 3 or int(sums.size(2)) != _lib.FORCES_NSUM:
            raise ValueError(f"sums: expected [steps, bodies, {_lib.FORCES_NSUM}], got {tuple(sums.shape)}")
        self.sums, self.angle, self.body_offsets = sums, angle, body_offsets
        self.moments, self.wall_moments, self.spectrum, self.target = moments, wall_moments, spectrum, target
        self.pressure = sums[..., [_lib.FORCES_FPX, _lib.FORCES_FPY, _lib.FORCES_MP]]
        self.viscous = sums[..., [_lib.FORCES_FVX, _lib.FORCES_FVY, _lib.FORCES_MV]]
        self.total = self.pressure + self.viscous

    @property
    def steps(self) -> int:
        return int(self.sums.size(0))

    def coefficients(self, rho: float, U: float, D: float):
        """(Cd, Cl, Cm), each [steps, B]: the total (F_x, F_y, M / D) over ½ rho U² D."""
        for name, v in (("rho", rho), ("U", U), ("D", D)):
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not v > 0:
                raise ValueError(f"{name}: expected a positive number, got {v!r}")
        q = 0.5 * float(rho) * float(U) * float(U) * float(D)
        return self.total[..., 0] / q, self.total[..., 1] / q, self.total[..., 2] / (q * float(D))

    def strouhal(self, D: float, U: float, body: int = 0) -> float:
        """The frequency with the largest power of the lift of `body` (`spectrum.dominant(field=1)` of that body) × D / U."""
        if self.spectrum is None:
            raise RuntimeError("RolloutForces: no force_spectrum= was asked for")
        n_bodies = int(self.spectrum.pivot.size(0))
        if isinstance(body, bool) or not isinstance(body, int) or not 0 <= body < n_bodies:
            raise ValueError(f"body: expected 0 .. {n_bodies - 1}, got {body!r}")
        mask = torch.zeros(n_bodies, dtype=torch.bool)
        mask[body] = True
        return self.spectrum.dominant(1, mask) * float(D) / float(U)

    def __repr__(self):
        return (f"RolloutForces(steps={self.steps}, bodies={int(self.sums.size(1))}, moments={self.moments is not None}, "
                f"wall_moments={self.wall_moments is not None}, spectrum={self.spectrum is not None}, target={self.target is not None})")


class _Integrals(_Part):
    """The integrals of a `Rollout` over the domain and the launches that form them: per source — the prediction, prediction − target,
    the target, the derived columns — a program of up to 8 entries, the sums [max_steps, ne] and a scratch, and ONE copy of the control
    volumes' areas in the rollout's node numbering (permuted here, once: a captured step allocates and permutes nothing)."""
    name = "integrals"
    SOURCES = ("prediction", "error", "target", "derived")

    @staticmethod
    def plan(names, nf: int, velocity=(0, 1), derived_columns=None, has_target: bool = True):
        """names -> (per source its list of entries, per name its recipe (kind, [(source, entry index), ...])).  ValueError naming
        `integrals` on an unknown name, a field out of range, a missing derived column or target, or more than 8 entries a source."""
        names = (names,) if isinstance(names, str) else names
        if not isinstance(names, (tuple, list)) or not len(names) or not all(isinstance(nm, str) for nm in names):
            raise ValueError(f"integrals: expected a non-empty tuple of names ('volume', 'int:<f>', 'mean:<f>', 'ke', 'circulation', "
                             f"'enstrophy', 'div2', 'l2:<f>', 'l2', 'rel_l2'), got {names!r}")
        if len(set(names)) != len(names):
            raise ValueError(f"integrals: a name is repeated in {tuple(names)!r}")
        try:
            velocity = tuple(velocity)
        except TypeError:
            raise ValueError(f"integral_options: velocity: expected 2 field numbers, got {velocity!r}") from None
        if len(velocity) != 2 or not all(_integer(v) and 0 <= v < nf for v in velocity):
            raise ValueError(f"integral_options: velocity: expected 2 field numbers below {nf}, got {velocity!r}")
        entries = {src: [] for src in _Integrals.SOURCES}

        def slot(src, a, b=-1):
            if (a, b) not in entries[src]:
                entries[src].append((a, b))
            return (src, entries[src].index((a, b)))

        def field(nm):
            tail = nm.split(":", 1)[1]
            if not tail.isdigit() or int(tail) >= nf:
                raise ValueError(f"integrals: {nm!r}: expected a field number below {nf} after the colon")
            return int(tail)

        def column(nm, label):
            if derived_columns is None or label not in derived_columns:
                raise ValueError(f"integrals: {nm!r} reads the {label!r} column of the derived fields: add {label!r} to derived=")
            return derived_columns.index(label)

        def target(nm):
            if not has_target:
                raise ValueError(f"integrals: {nm!r} is an error against the target: it needs target= (GNN.integrals reads graph.target)")

        recipes = []
        for nm in names:
            if nm == "volume":
                recipes.append(("sum", [slot("prediction", -1)]))
            elif nm.startswith("int:"):
                recipes.append(("sum", [slot("prediction", field(nm))]))
            elif nm.startswith("mean:"):
                recipes.append(("ratio", [slot("prediction", field(nm)), slot("prediction", -1)]))
            elif nm == "ke":
                recipes.append(("half", [slot("prediction", v, v) for v in velocity]))
            elif nm == "circulation":
                recipes.append(("sum", [slot("derived", column(nm, "vort"))]))
            elif nm == "enstrophy":
                c = column(nm, "vort")
                recipes.append(("half", [slot("derived", c, c)]))
            elif nm == "div2":
                c = column(nm, "div")
                recipes.append(("sum", [slot("derived", c, c)]))
            elif nm.startswith("l2:"):
                target(nm)
                f = field(nm)
                recipes.append(("root", [slot("error", f, f)]))
            elif nm in ("l2", "rel_l2"):
                target(nm)
                num = [slot("error", f, f) for f in range(nf)]
                den = [slot("target", f, f) for f in range(nf)]          # (`l2` keeps ∫ target² in `sums` too: the norm it is read against)
                recipes.append(("root" if nm == "l2" else "rel", [num, den]))
            else:
                raise ValueError(f"integrals: unknown name {nm!r} ('volume', 'int:<f>', 'mean:<f>', 'ke', 'circulation', 'enstrophy', 'div2', "
                                 f"'l2:<f>', 'l2' and 'rel_l2' are known)")
        for src, e in entries.items():
            if len(e) > _lib.INTEGRALS_MAX_ENTRIES:
                raise ValueError(f"integrals: {tuple(names)!r} need {len(e)} sums over the {src}, at most {_lib.INTEGRALS_MAX_ENTRIES} fit one launch")
        return entries, recipes

    @staticmethod
    def check(kw, ctx, specs):
        """The `integrals=` / `integral_volumes=` / `integral_options=` arguments against the caller's graph -> names, entries, recipes,
        volumes, options."""
        from ..control_volumes import ControlVolumes, check_volumes
        from ..mesh_gradient import derived_columns
        names, volumes, options = kw["integrals"], kw["integral_volumes"], kw["integral_options"]
        if names is None or names is False:
            if volumes is not None or options:
                raise ValueError("integrals: integral_volumes / integral_options were given without integrals=")
            return None
        options = dict(options or {})
        unknown = set(options) - {"velocity", "box", "bodies"}
        if unknown:
            raise ValueError(f"integral_options: unknown option(s) {sorted(unknown)} (velocity, box, bodies)")
        derived = specs.get("derived")
        entries, recipes = _Integrals.plan(names, ctx.nf, options.get("velocity", (0, 1)),
                                           None if derived is None else derived_columns(derived["names"], 2), ctx.has_target)
        if volumes is not None:
            if not isinstance(volumes, ControlVolumes):
                raise TypeError(f"integral_volumes: expected a gfd.ControlVolumes of this graph or None, got {type(volumes).__name__}")
            if ctx.in_list:
                raise ValueError("integral_volumes: the volumes of a list of graphs: leave it None (each graph of the batch gets its own cells)")
            if volumes.n_nodes != int(ctx.graph.num_nodes):
                raise ValueError(f"integral_volumes: a ControlVolumes over {volumes.n_nodes} nodes for a graph of {int(ctx.graph.num_nodes)}")
            if "box" in options or "bodies" in options:
                raise ValueError("integral_options: box / bodies were given together with integral_volumes= (the volumes carry their own)")
        else:
            if ctx.in_list and options.get("bodies") is not None:
                raise ValueError("integral_options: bodies of a list of graphs: build the gfd.ControlVolumes of the collated graph yourself")
            for graph in ctx.graphs:
                check_volumes(graph, options.get("box"), options.get("bodies"))
        return dict(names=tuple((names,) if isinstance(names, str) else names), entries=entries, recipes=recipes, volumes=volumes,
                    options=options)

    def __init__(self, ro: "Rollout", spec: dict):
        from ..control_volumes import ControlVolumes
        dev, n, steps = ro.field.device, int(ro.graph.num_nodes), ro.max_steps
        self.names, self.recipes, self.nf, self.max_steps = spec["names"], spec["recipes"], ro.nf, steps
        volumes = spec["volumes"]
        if volumes is None:          # (on the caller's graph: its numbering, its batch — each graph of a batch has its own cells)
            volumes = ControlVolumes(ro._caller_graph, spec["options"].get("box"), spec["options"].get("bodies"))
        self.volumes = volumes
        w = volumes.area.to(dev)
        self.w = (w[ro._perm.to(dev)] if ro._perm is not None else w).contiguous()
        self.programs, self.sums, self.scratch = {}, {}, {}
        for src, entries in spec["entries"].items():
            if entries:
                nz = ro._derived.nd if src == "derived" else ro.nf
                self.programs[src] = ops.integral_program(entries, nz)
                self.sums[src] = torch.zeros((steps, len(entries)), dtype=torch.float64, device=dev)
                self.scratch[src] = ops.weighted_integrals_scratch(n, len(entries), dev)
        self.target = ro._rec.target if ("error" in self.programs or "target" in self.programs) else None
        self.cur = ro._derived.cur if "derived" in self.programs else None

    def launch(self, ro: "Rollout", pred: torch.Tensor) -> None:
        nf, step = self.nf, ro.step_counter
        for src, prog in self.programs.items():
            if src == "prediction":
                ops.weighted_integrals(pred, self.w, prog, self.sums[src], self.scratch[src], nz=nf, step=step)
            elif src == "error":
                ops.weighted_integrals(pred, self.w, prog, self.sums[src], self.scratch[src], nz=nf, sub=self.target, sub_step=nf, step=step)
            elif src == "target":
                ops.weighted_integrals(self.target, self.w, prog, self.sums[src], self.scratch[src], nz=nf, x_step=nf, step=step)
            else:
                ops.weighted_integrals(self.cur, self.w, prog, self.sums[src], self.scratch[src], nz=int(self.cur.size(1)), step=step)

    def read(self, ro: "Rollout") -> "RolloutIntegrals":
        sums = {src: s[:ro.steps_done].cpu() for src, s in self.sums.items()}
        return RolloutIntegrals(self.names, self.recipes, sums, float(self.volumes.total), {src: [(int(p.a[e]), int(p.b[e])) for e in range(int(p.ne))]
                                                                                            for src, p in self.programs.items()})


class RolloutIntegrals:
    """Integrals of a rollout over the domain (`Rollout.integrals()`, `GNN.integrals()`, `GNN.evaluate(integrals=)`), per step taken,
    fp64 host tensors: `values` [steps, names] in the order of `names`; `sums` — per source ('prediction', 'error' = prediction −
    target, 'target', 'derived') the raw Σ_i area_i z_i[a] z_i[b] [steps, entries] the step formed on the device in fp64 in a fixed order,
    `entries` their column pairs (−1: the constant 1); `volume`: Σ area of the control volumes.  'ke' and 'enstrophy' are half their
    sums, 'mean:<f>' is ∫ f over the 'volume' sum of the same step, 'l2:<f>' and 'l2' the square roots, 'rel_l2' = √(Σ_f ∫ (p − t)² / Σ_f
    ∫ t²).  `drift(name)` = value / first value − 1.  A NaN at a node of non-zero area makes the integrals that read its column NaN at
    that step; a node of zero area contributes nothing whatever it holds."""

    def __init__(self, names, recipes, sums: dict, volume: float, entries: dict):
        self.names, self.sums, self.volume, self.entries = tuple(names), sums, float(volume), entries
        self._recipes = recipes
        steps = int(next(iter(sums.values())).size(0)) if sums else 0

        def take(ref):
            if isinstance(ref, list):
                out = torch.zeros(steps, dtype=torch.float64)
                for r in ref:          # (in the order of the fields)
                    out = out + take(r)
                return out
            return sums[ref[0]][:, ref[1]]

        cols = []
        for kind, refs in recipes:
            if kind == "sum":
                cols.append(take(refs[0]))
            elif kind == "half":
                cols.append(0.5 * take(list(refs)))
            elif kind == "ratio":
                cols.append(take(refs[0]) / take(refs[1]))
            elif kind == "root":
                cols.append(take(refs[0]).sqrt())
            else:
                cols.append((take(refs[0]) / take(refs[1])).sqrt())
        self.values = torch.stack(cols, dim=1) if cols else torch.zeros((steps, 0), dtype=torch.float64)

    @property
    def steps(self) -> int:
        return int(self.values.size(0))

    def __getitem__(self, name: str) -> torch.Tensor:
        """[steps]: the values of one name."""
        if name not in self.names:
            raise KeyError(f"{name!r} is not among {self.names}")
        return self.values[:, self.names.index(name)]

    def drift(self, name: str) -> torch.Tensor:
        """[steps]: value / first value − 1 (the kinetic energy's drift over the rollout)."""
        v = self[name]
        return v / v[0] - 1.0

    def __repr__(self):
        return f"RolloutIntegrals(names={self.names}, steps={self.steps}, volume={self.volume:.6g})"


class _Records:
    """The record buffers of a `Rollout` and the launch that fills them.  Everything is allocated here, once, in the rollout's node
    numbering (probe rows, target rows and mask rows are mapped through the Morton permutation at construction), so a captured
    step allocates nothing; every slot is addressed by the device-side step index alone, so `rewind()` and a recomputation
    (`Rollout.validate`) overwrite the records of the steps they run again."""

    def __init__(self, ro: "Rollout", every: int, probes, target, mask):
        dev, n, nf, steps, perm = ro.field.device, int(ro.graph.num_nodes), ro.nf, ro.max_steps, ro._perm
        self.nf, self.max_steps, self.every = nf, steps, every
        self.snap = torch.zeros((steps // every, n, nf), dtype=torch.float32, device=dev) if every else None
        ro._out_steps = self.snap
        self.probe_rows = self.probe_out = self.target = self.mask = self.stats = self.scratch = None
        self.n_masked = None
        if probes is not None:
            rows = probes.to(dev, torch.long)
            if perm is not None:
                rows = ro._inv.to(dev)[rows]
            self.probe_rows = rows.to(torch.int32).contiguous()
            self.probe_out = torch.zeros((steps, int(rows.numel()), nf), dtype=torch.float32, device=dev)
        if target is not None:
            t = target.to(dev, torch.float32)
            if perm is not None:
                t = t[perm.to(dev)]
            if t.stride(1) != 1 or t.stride(0) < t.size(1):
                t = t.contiguous()
            self.target = t
            if mask is not None:
                m = mask.to(dev)
                self.n_masked = int(m.sum())
                self.mask = (m[perm.to(dev)] if perm is not None else m).contiguous()
            self.stats = torch.zeros((steps, nf, _lib.REC_NSTAT), dtype=torch.float64, device=dev)
            self.scratch = ops.rollout_record_scratch(n, nf, dev)

    def advance(self, field, pred, step) -> None:
        ops.rollout_advance_record(field, pred, step, self.nf, self.max_steps, snap=self.snap, every=self.every,
                                   probe_rows=self.probe_rows, probe_out=self.probe_out, target=self.target, mask=self.mask,
                                   stats=self.stats, scratch=self.scratch)

    def read(self, ro: "Rollout") -> "RolloutErrors":
        return RolloutErrors(self.stats[:ro.steps_done].cpu(), int(ro.graph.num_nodes), self.n_masked,
                             snapshots=ro.result() if ro._out_steps is not None else None,
                             probes=ops.steps_to_columns(self.probe_out) if self.probe_out is not None else None)


class RolloutErrors:
    """Per-step errors of a rollout against its target (`Rollout.errors()`, `GNN.evaluate()`): fp64 host tensors [steps, nf] —
    `mse` = Σd²/N, `mae` = Σ|d|/N, `max_abs` = max|d|, `r2` = 1 − Σd² / (Σy² − (Σy)²/N) (inf or nan where the target is constant),
    `mae_masked` = Σ|d| over the masked (Dirichlet) nodes / their number (None without a mask) — with d = prediction − target and
    y = the target, all from `sums` [steps, nf, 6] = (Σd², Σ|d|, max|d|, Σy, Σy², Σ_masked|d|), which the step's last launch
    accumulated on the device in fp64 in a fixed order.  `snapshots` / `probes`: the rollout's `result()` / `probes()` when it kept
    any, else None.  `moments` / `error_moments`: None unless `GNN.evaluate` was asked for them.
    Non-finite samples (a rollout that blew up, a target with holes): `mse`, `mae` AND `max_abs` of a step and field are NaN when d is
    NaN at any node — `max_abs` is never the maximum over the remaining nodes: a record does not read better than the rollout was —
    and inf where the largest |d| is.  A row outside the mask contributes nothing to `mae_masked`, whatever it holds.  Every other
    step and field is untouched."""

    def __init__(self, sums: torch.Tensor, n_nodes: int, n_masked: Optional[int] = None, snapshots: Optional[torch.Tensor] = None,
                 probes: Optional[torch.Tensor] = None):
        self.sums, self.n_nodes, self.n_masked, self.snapshots, self.probes = sums, int(n_nodes), n_masked, snapshots, probes
        self.moments = self.error_moments = None        # `RolloutMoments` when GNN.evaluate(moments= / error_moments=) asked for them
        self.derived = None                             # `RolloutDerived` when GNN.evaluate(derived=) asked for it
        self.spectrum = self.target_spectrum = None     # `RolloutSpectrum` when GNN.evaluate(spectrum=) asked for them
        self.welch = self.target_welch = None           # `RolloutWelch` when GNN.evaluate_welch formed them
        n = float(n_nodes)
        sq, ab, mx, ty, ty2, abm = (sums[..., k] for k in range(_lib.REC_NSTAT))
        self.mse, self.mae, self.max_abs = sq / n, ab / n, mx
        self.r2 = 1.0 - sq / (ty2 - ty * ty / n)
        self.mae_masked = None if n_masked is None else abm / float(n_masked)

    @property
    def steps(self) -> int:
        return int(self.sums.size(0))

    def graph_loss(self, lambda_d: float = 0.0) -> torch.Tensor:
        """`GraphLoss(lambda_d)` of every step, [steps], from the same sums: Σ_f Σd² / (N nf) + lambda_d Σ_f Σ_masked|d| / (N_masked nf),
        the second term only with lambda_d > 0 and at least one masked node (nn/losses.py)."""
        nf = int(self.sums.size(1))
        loss = self.sums[..., _lib.REC_SQ_ERR].sum(1) / (self.n_nodes * nf)
        if lambda_d > 0 and self.n_masked:
            loss = loss + lambda_d * self.sums[..., _lib.REC_ABS_ERR_MASK].sum(1) / (self.n_masked * nf)
        return loss

    def __repr__(self):
        return f"RolloutErrors(steps={self.steps}, fields={int(self.sums.size(1))}, nodes={self.n_nodes}, masked={self.n_masked})"


# The parts of a step, in the order `Rollout._one` launches them (the records' closing launch comes last, outside this list) ...
_PARTS = (_Derived, _Integrals, _Samples, _Forces, _NodeMoments, _ErrorMoments, _NodeSpectrum, _TargetSpectrum, _DerivedSpectrum, _Welch, _Tracers)
# ... and in the order their keywords are checked: the precedence of the argument errors
_CHECKED = (_Derived, _DerivedSpectrum, _NodeSpectrum, _TargetSpectrum, _Samples, _Tracers, _Forces, _NodeMoments, _ErrorMoments, _Integrals,
            _Welch)
# every keyword of `Rollout` that asks for a record or a part, with its default: named once, in the signature of `Rollout.__init__`
KEYWORDS = {name: p.default for name, p in inspect.signature(Rollout.__init__).parameters.items()
            if name not in ("self", "model", "graph", "max_steps", "capture", "reorder", "label")}
# ... and those of the parts `Rollout.open` and `GNN._rollout` take beyond that signature
KEYWORDS.update(integrals=None, integral_volumes=None, integral_options=None, welch=None, target_welch=False)


def _check_parts(keywords: dict, graph, nf: int, max_steps: int, has_target: bool) -> dict:
    """The keywords of a rollout (those left out take their defaults; other entries are ignored) -> {part's name: its checked spec, or
    None when it is not asked for}, against the caller's graph, or list of graphs, as passed: nothing is collated or moved, neither the
    library nor a device is touched.  `has_target`: a target will be given (the records themselves are checked by `Rollout`)."""
    kw = {**KEYWORDS, **keywords}
    graphs = graph if type(graph) is list else [graph]
    ctx = SimpleNamespace(graphs=graphs, graph=graphs[0], in_list=type(graph) is list, nf=nf, max_steps=max_steps, has_target=has_target)
    specs = {}
    for part in _CHECKED:
        specs[part.name] = part.check(kw, ctx, specs)
    return specs
