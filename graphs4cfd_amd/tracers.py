"""Lagrangian tracers (new functionality — the reference has none): massless particles carried by a velocity that lives at the mesh
nodes — pathlines, the streakline picture of a wake (smoke released behind the cylinder), where the fluid released at a point ends
up and how long it stays in the recirculation bubble.

One launch (`g4c_tracer_advance`, csrc/tracer.hip) moves every particle one step: at its position q the k nearest nodes by the exact
cell-grid search of `knn_query_device`, the coefficients of `gfd.PointSampler`'s linear moving-least-squares fit over them, the
velocity as their fp32 sum nearest first, v = scale u + shift, and q += dt v (Euler) or Heun's predictor–corrector, whose second
stage reads the NEXT time level at the predicted position.  A particle is `waiting` (0) before its release step, `moving` (1), and
frozen once it `left` the box (2), got `far`ther than max_distance from every node (3 — the search knows no boundary: this is how a
particle that enters a body or leaves the mesh is stopped) or its position is no longer finite (4); `stopped` holds the step.
With `period=` the domain is periodic along the named axes (`g4c_tracer_advance_periodic`): a particle that crosses a periodic face
comes back in through the opposite one and stays moving.  Walls do not reflect."""
from __future__ import annotations

import math
from typing import Optional, Sequence

import torch

from . import _lib, ops
from .point_sampler import _integer, check_points

WAITING, MOVING, LEFT, FAR, NONFINITE = (_lib.TRACER_WAITING, _lib.TRACER_MOVING, _lib.TRACER_LEFT, _lib.TRACER_FAR,
                                         _lib.TRACER_NONFINITE)
SCHEMES = {"euler": _lib.TRACER_EULER, "heun": _lib.TRACER_HEUN}


def _numbers(name: str, v, dim: int, *, infinite: bool = False):
    """`dim` numbers (a sequence or a 1-D tensor; one number stands for all axes) -> a list of floats; ValueError naming the argument."""
    if isinstance(v, (int, float)) and not isinstance(v, bool):
        v = [v] * dim
    try:
        vals = [float(c) for c in (v.tolist() if torch.is_tensor(v) else v)]
    except (TypeError, ValueError):
        raise ValueError(f"{name}: expected {dim} numbers, got {v!r}") from None
    if len(vals) != dim or any(c != c for c in vals) or (not infinite and any(math.isinf(c) for c in vals)):
        raise ValueError(f"{name}: expected {dim} {'numbers (no NaN)' if infinite else 'finite numbers'}, got {v!r}")
    return vals


def check_tracers(graph, seeds, dt, scheme="heun", k=None, power=2, velocity=None, scale=None, shift=None, box=None, max_distance=None,
                  release=None, nf: Optional[int] = None, period=None) -> dict:
    """The arguments of `Tracers` on the tensors as they were passed (nothing is moved, the library is not touched) -> what the launch
    needs, as a dict; ValueError / TypeError naming the argument.  `nf`: the columns the velocity is taken from, when known."""
    try:
        dim, k = check_points(graph, seeds, k, power)
    except ValueError as e:
        msg = str(e)
        raise ValueError("seeds:" + msg[len("points:"):] if msg.startswith("points:") else msg) from None
    from .synthetic import check_period
    period = check_period(period, dim, "Tracers")
    n = int(seeds.size(0))
    if isinstance(dt, bool) or not isinstance(dt, (int, float)):
        raise TypeError(f"dt: expected a number (the time between two predictions), got {dt!r}")
    if not math.isfinite(dt):
        raise ValueError(f"dt: expected a finite number (the time between two predictions), got {dt!r}")
    if not isinstance(scheme, str) or scheme not in SCHEMES:
        raise ValueError(f"scheme: expected 'euler' or 'heun', got {scheme!r}")
    if velocity is None:
        velocity = list(range(dim))
    try:
        velocity = list(velocity)
    except TypeError:
        raise ValueError(f"velocity: expected the {dim} fields of the velocity components, got {velocity!r}") from None
    if len(velocity) != dim or not all(_integer(v) and v >= 0 for v in velocity):
        raise ValueError(f"velocity: expected the {dim} fields of the velocity components (integers >= 0), got {velocity!r}")
    if nf is not None and max(velocity) >= nf:
        raise ValueError(f"velocity: fields {velocity} of {nf} (the velocity must be among the fields)")
    scale = [1.0] * dim if scale is None else _numbers("scale", scale, dim)
    shift = [0.0] * dim if shift is None else _numbers("shift", shift, dim)
    if box is None:
        lo, hi = [-math.inf] * dim, [math.inf] * dim
    else:
        try:
            lo, hi = box
        except (TypeError, ValueError):
            raise ValueError(f"box: expected (lo, hi), two corners of {dim} coordinates, got {box!r}") from None
        lo, hi = _numbers("box", lo, dim, infinite=True), _numbers("box", hi, dim, infinite=True)
        if any(l > h for l, h in zip(lo, hi)):
            raise ValueError(f"box: a lower corner above the upper one, got {box!r}")
    if max_distance is None:
        max_distance = math.inf
    if isinstance(max_distance, bool) or not isinstance(max_distance, (int, float)) or not max_distance >= 0:
        raise ValueError(f"max_distance: expected a distance >= 0 (None: no limit), got {max_distance!r}")
    if release is None:
        release = torch.zeros(n, dtype=torch.int32)
    else:
        if not torch.is_tensor(release):
            try:
                ok = all(_integer(r) for r in release)
            except TypeError:
                ok = False
            if not ok:
                raise TypeError(f"release: expected one integer step per particle, got {release!r}")
            release = torch.tensor(list(release), dtype=torch.int64)
        if release.dtype.is_floating_point or release.dtype == torch.bool or release.is_complex():
            raise TypeError(f"release: expected an integer tensor (one step per particle), got {release.dtype}")
        if tuple(release.shape) != (n,):
            raise ValueError(f"release: expected shape ({n},), one step per particle, got {tuple(release.shape)}")
        if n and (int(release.min()) < 0 or int(release.max()) >= 2 ** 31):
            raise ValueError(f"release: steps {int(release.min())} .. {int(release.max())} (0 <= release < 2^31)")
        release = release.detach().to(torch.int32)
    return dict(dim=dim, k=k, power=power, dt=float(dt), scheme=SCHEMES[scheme], scheme_name=scheme, velocity=velocity, scale=scale, shift=shift,
                box_lo=lo, box_hi=hi, max_distance=float(max_distance), seeds=seeds.detach().to(torch.float32), release=release,
                n_nodes=int(graph.pos.size(0)), groups=None, period=period)


class TracerState:
    """The particles of one tracer set on a device and the launch that moves them: the cell grid over `pos` (built here, once), the
    positions `q` [P, dim], `status`, `stopped`, `vel`, and — with every > 0 — the `series` of max_steps // every slots."""

    def __init__(self, spec: dict, pos: torch.Tensor, every: int = 0, max_steps: int = 0):
        from .synthetic import _bin_cloud, _bin_cloud_periodic
        dev = pos.device
        self.spec, self.every, self.max_steps = spec, int(every), int(max_steps)
        if spec.get("period") is None:
            self.grid = _bin_cloud(pos, spec["k"], "Tracers (g4c_tracer_advance)")
        else:          # (the periodic grid: `ops.tracer_advance` takes the periodic launch with it)
            self.grid = _bin_cloud_periodic(pos, spec["k"], spec["period"], "Tracers (g4c_tracer_advance_periodic)")
        self.seeds, self.release = spec["seeds"].to(dev).contiguous(), spec["release"].to(dev).contiguous()
        n, dim = int(self.seeds.size(0)), spec["dim"]
        self.q = self.seeds.clone()
        self.status = torch.zeros(n, dtype=torch.uint8, device=dev)
        self.stopped = torch.full((n,), -1, dtype=torch.int32, device=dev)
        self.vel = torch.zeros((n, dim), dtype=torch.float32, device=dev)
        self.series = torch.zeros((self.max_steps // self.every, n, dim), dtype=torch.float32, device=dev) if self.every else None
        self._saved = None

    def launch(self, x0, x1, step=None, t: int = 0, max_steps: Optional[int] = None) -> None:
        s = self.spec
        ops.tracer_advance(self.grid, x0, x1 if s["scheme"] == _lib.TRACER_HEUN else None, self.q, self.status, self.stopped, self.release,
                           dt=s["dt"], k=s["k"], power=s["power"], scheme=s["scheme"], vcol=s["velocity"], scale=s["scale"], shift=s["shift"],
                           box_lo=s["box_lo"], box_hi=s["box_hi"], max_distance=s["max_distance"], step=step, t=t,
                           max_steps=self.max_steps if max_steps is None else max_steps, every=self.every, series=self.series, vel=self.vel)

    def reset(self) -> None:
        """Every particle back at its seed, waiting."""
        self.q.copy_(self.seeds)
        self.status.zero_()
        self.stopped.fill_(-1)
        self.vel.zero_()

    def save(self) -> None:
        """Keep q, status and stopped (plain copies on the stream): `restore()` starts again from them."""
        if self._saved is None:
            self._saved = (self.q.clone(), self.status.clone(), self.stopped.clone())
        else:
            for kept, live in zip(self._saved, (self.q, self.status, self.stopped)):
                kept.copy_(live)

    def restore(self) -> None:
        for kept, live in zip(self._saved, (self.q, self.status, self.stopped)):
            live.copy_(kept)


class Tracers:
    """Particles released at `seeds` [S, dim] (a floating-point tensor, host or device) into the velocity at the nodes of `graph` (a
    Graph on the GPU with `pos` [N, dim]); `dt` is the time between two predictions, in the units that make dt · velocity a length of
    `graph.pos`.

    scheme     'heun' (default: second order, the second stage reads the next time level) or 'euler'.
    k, power   the neighbours and the weight of the interpolation, as `gfd.PointSampler`'s (k defaults to 6 in 2-D, 10 in 3-D).
    velocity   the fields of the velocity components (default 0 .. dim - 1); scale, shift (a number or one per axis): the physical
               velocity is scale · field + shift (normalised data).
    box        (lo, hi): a particle that leaves it is frozen where it left (status 2; corners may be infinite);
    max_distance  a particle farther than this from every node is frozen (status 3): inside a body, outside the mesh.
    release    int [S]: the first step each particle moves at (default 0).
    period     one entry per axis — None, a length >= the mesh's extent, or "auto", the extent (as `connect_knn`'s): along such an
               axis every stage searches and fits in the wrapped metric, and the new position is wrapped into [origin, origin +
               length), origin the mesh's minimum, before it is stored, tested against `box` and recorded.  A particle that crosses
               a periodic face stays moving.  Recorded `paths` therefore hold WRAPPED positions: a jump of more than half a period
               between two slots is a crossing (no winding count is kept).

    Give `box` or `max_distance` whenever particles can leave the mesh: the search is exact, and for a particle D away from the cloud it
    grows ring by ring to D / cell size rings, scanning every block on the way — the whole grid at every stage of every step until the
    particle is frozen.

    `advance(x0, x1, t)` is one launch outside any rollout on this object's own state — for stored snapshots; `Rollout(tracers=)`,
    `GNN.trace` and `GNN.evaluate(tracers=)` advect a copy of the particles inside the step and leave this object as it is.
    `positions` [S, dim], `status` uint8 [S], `stopped` int32 [S] (the step a particle was frozen at, -1 before), `velocity_used`
    [S, dim] (the first stage's velocity of the last step a particle moved), `reset()`.  `Tracers.streak` builds a streakline's."""

    def __init__(self, graph, seeds: torch.Tensor, dt: float, *, scheme: str = "heun", k: Optional[int] = None, power: int = 2,
                 velocity: Optional[Sequence[int]] = None, scale=None, shift=None, box=None, max_distance: Optional[float] = None,
                 release=None, period=None):
        self._spec = check_tracers(graph, seeds, dt, scheme, k, power, velocity, scale, shift, box, max_distance, release, period=period)
        pos = graph.pos
        if pos.device.type != "cuda":
            raise ValueError(f"graph: Tracers run on a HIP device only, graph.pos is on '{pos.device}' (there is no CPU fallback)")
        s = self._spec
        self.dim, self.k, self.power, self.dt, self.scheme, self.n_nodes, self.groups = s["dim"], s["k"], s["power"], s["dt"], s["scheme_name"], s["n_nodes"], None
        self._state = TracerState(s, pos.detach().to(torch.float32).contiguous())

    @classmethod
    def streak(cls, graph, seeds: torch.Tensor, dt: float, release_every: int = 1, releases: int = 1, **kw) -> "Tracers":
        """A streakline's particles: `releases` = m particles per seed, the i-th released at step i · release_every — S · m particles,
        particle (i, s) at row i · S + s; `.groups` is (m, S).  `RolloutTracers.streakline(slot)` orders them [S, m, dim]."""
        if not _integer(release_every) or release_every < 1:
            raise ValueError(f"release_every: expected an integer >= 1 (steps between two releases), got {release_every!r}")
        if not _integer(releases) or releases < 1:
            raise ValueError(f"releases: expected an integer >= 1 (particles per seed), got {releases!r}")
        if "release" in kw:
            raise ValueError("release: a streak sets the release steps itself (release_every, releases)")
        if not torch.is_tensor(seeds) or seeds.dim() != 2:
            raise ValueError(f"seeds: expected a floating-point tensor [S, dim], got {getattr(seeds, 'shape', type(seeds).__name__)}")
        n_seeds = int(seeds.size(0))
        release = (torch.arange(releases, dtype=torch.int64) * release_every).repeat_interleave(n_seeds)
        if releases and int(release[-1]) >= 2 ** 31:
            raise ValueError(f"releases: the last release step {int(release[-1])} does not fit an int32")
        tr = cls(graph, seeds.repeat(releases, 1), dt, release=release, **kw)
        tr.groups = tr._spec["groups"] = (releases, n_seeds)
        return tr

    @property
    def n_particles(self) -> int:
        return int(self._state.q.size(0))

    @property
    def seeds(self) -> torch.Tensor:
        return self._state.seeds

    @property
    def release(self) -> torch.Tensor:
        return self._state.release

    @property
    def positions(self) -> torch.Tensor:
        return self._state.q

    @property
    def status(self) -> torch.Tensor:
        return self._state.status

    @property
    def stopped(self) -> torch.Tensor:
        return self._state.stopped

    @property
    def velocity_used(self) -> torch.Tensor:
        return self._state.vel

    def reset(self) -> None:
        """Every particle back at its seed, waiting."""
        self._state.reset()

    def advance(self, x0: torch.Tensor, x1: Optional[torch.Tensor] = None, t: int = 0) -> torch.Tensor:
        """One step, one launch: x0 [N, F] the node fields at the time level the particles are at, x1 [N, F] those of the next one
        (Heun's second stage; not read by 'euler'), float32 on the device, rows of unit stride (a column slice will do); `t` the step
        index the release steps are compared with and `stopped` records.  Returns `positions`."""
        if not _integer(t) or not 0 <= t < 2 ** 31 - 1:
            raise ValueError(f"t: expected a step index 0 <= t < 2^31 - 1, got {t!r}")
        for name, x in (("x0", x0),) + ((("x1", x1),) if self._spec["scheme"] == _lib.TRACER_HEUN else ()):
            if x is None:
                raise ValueError(f"{name}: the 'heun' scheme reads the next time level at the predicted position: pass x1")
            if not torch.is_tensor(x) or x.dtype != torch.float32 or x.dim() != 2 or int(x.size(0)) != self.n_nodes:
                raise ValueError(f"{name}: expected a float32 tensor [{self.n_nodes}, F], got {getattr(x, 'dtype', type(x).__name__)} "
                                 f"{tuple(getattr(x, 'shape', ()))}")
            if max(self._spec["velocity"]) >= int(x.size(1)):
                raise ValueError(f"velocity: fields {self._spec['velocity']} of {name} with {int(x.size(1))} columns")
        self._state.launch(x0, x1, t=t, max_steps=2 ** 31 - 1)
        return self._state.q

    def __repr__(self):
        return (f"Tracers(particles={self.n_particles}, nodes={self.n_nodes}, dim={self.dim}, dt={self.dt}, scheme={self.scheme!r}, k={self.k}, "
                f"power={self.power}{'' if self.groups is None else f', groups={self.groups}'})")


class RolloutTracers:
    """The tracers of a rollout (`Rollout.tracers()`, `GNN.trace()`, `GNN.evaluate(tracers=)`), the particles in the caller's order:
    `paths` [P, dim * slots] — the positions after steps k - 1, 2k - 1, ... (`tracer_every=k`; None with 0), laid out as
    `Rollout.probes()`; a particle not yet released sits at its seed, a frozen one where it stopped —, `positions` [P, dim] (the
    last), `status` uint8 [P] (0 waiting, 1 moving, 2 left the box, 3 too far from every node, 4 not finite), `stopped` int32 [P] (-1
    while not frozen), `release` int32 [P], `seeds`; `target_paths`: the same particles advected through the ground truth, filled by
    `GNN.evaluate`.  `streakline(slot)` and `residence()` read them."""

    def __init__(self, paths: Optional[torch.Tensor], positions: torch.Tensor, status: torch.Tensor, stopped: torch.Tensor,
                 release: torch.Tensor, seeds: torch.Tensor, every: int = 1, groups=None):
        self.paths, self.positions, self.status, self.stopped, self.release, self.seeds = paths, positions, status, stopped, release, seeds
        self.every, self.groups, self.dim = int(every), groups, int(positions.size(1))
        self.target_paths = None

    @property
    def slots(self) -> int:
        return 0 if self.paths is None else int(self.paths.size(1)) // self.dim

    def streakline(self, slot: int = -1):
        """(line [S, m, dim], released bool [S, m]) for the particles of `Tracers.streak`: `line[s]` joins the particles released at
        seed s, the oldest first, after the step of slot `slot` (negative: from the last); `released` is False for those still
        waiting at the seed."""
        if self.groups is None:
            raise ValueError("streakline: the particles are no streak (Tracers.streak builds one)")
        if self.paths is None:
            raise ValueError("streakline: no series was kept (tracer_every=0)")
        slots = self.slots
        if isinstance(slot, bool) or not isinstance(slot, int) or not -slots <= slot < slots:
            raise ValueError(f"slot: expected -{slots} <= slot < {slots}, got {slot!r}")
        slot %= slots
        m, n_seeds = self.groups
        line = self.paths[:, self.dim * slot:self.dim * (slot + 1)].reshape(m, n_seeds, self.dim).permute(1, 0, 2)
        step = (slot + 1) * self.every - 1
        return line, (self.release <= step).reshape(m, n_seeds).t()

    def residence(self) -> torch.Tensor:
        """int32 [P]: the steps between a particle's release and the step it was frozen at; -1 while it moves or waits."""
        return torch.where(self.status >= LEFT, self.stopped - self.release, torch.full_like(self.stopped, -1))

    def __repr__(self):
        return f"RolloutTracers(particles={int(self.positions.size(0))}, dim={self.dim}, slots={self.slots}, every={self.every}, groups={self.groups})"
