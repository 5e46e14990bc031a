"""Everything a `Rollout` can carry, attached at once, through the public API only: the launches of one step come in one fixed order,
and no part changes what another returns — every accessor's result is bit for bit that of a rollout with only its own family
attached, run straight, after `rewind()`, and after a clipped rollout was computed again.  (That each part alone is right is the
business of its own test file: each is pinned there to a replay.)"""
import os
import sys
import warnings

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pytestmark = pytest.mark.gpu

import graphs4cfd_amd as gfd                             # noqa: E402
from graphs4cfd_amd import ops, synthetic as S           # noqa: E402
from graphs4cfd_amd.nn.model import Rollout              # noqa: E402

DEV = torch.device("cuda", 0)
N_OUT, NF, ND, N_POINTS, N_SEEDS = 6, 3, 2, 7, 5
WALLS = (((0.35, 0.5), 0.15, 64), ((0.75, 0.5), 0.1, 40))          # (centre, radius, wall nodes) of the two bodies: B = 2, W = 104


def points_in(g, n, seed):
    lo, hi = g.pos.min(0).values.cpu(), g.pos.max(0).values.cpu()
    return lo + (hi - lo) * (torch.rand(n, int(g.pos.size(1)), generator=torch.Generator().manual_seed(seed)) * 0.9 + 0.05)


@pytest.fixture(scope="module")
def mesh():
    g = S.mus_graph(1500, levels=2, seed=11).to(DEV)
    g.batch = torch.zeros(g.num_nodes, dtype=torch.long, device=DEV)
    pos = g.pos.cpu().double()
    wall, labels = torch.zeros(g.num_nodes, dtype=torch.bool), torch.zeros(g.num_nodes, dtype=torch.long)
    for b, ((cx, cy), r, m) in enumerate(WALLS):                  # the m nodes nearest to each circle: a ring, star-shaped about its mean
        ring = torch.argsort(((pos[:, 0] - cx).hypot(pos[:, 1] - cy) - r).abs())[:m]
        wall[ring], labels[ring] = True, 10 * (b + 1)
    nodes = torch.nonzero(wall).flatten()
    torch.manual_seed(12)
    model = gfd.nn.NsTwoScaleGNN(arch=S.mus_arch("NsTwoScaleGNN", 128), device=DEV)
    model.eval()
    full = model.solve(g.clone(), N_OUT)
    op = gfd.BodyForces(g, nodes.to(DEV), labels[nodes], mu=0.0125, scale=[2.0, 0.5, 1.25], shift=[0.5, 0.0, -0.25])
    assert op.n_bodies == 2 and op.n_items == 104
    gen = torch.Generator().manual_seed(5)
    lo, hi = g.pos.min(0).values, g.pos.max(0).values
    vmax = max(float(full.view(-1, N_OUT, NF)[:, :, :2].abs().max()), float(g.field[:, -NF:-1].abs().max()))
    return dict(g=g, model=model, op=op, target=torch.randn(g.num_nodes, NF * N_OUT + 2, generator=gen).to(DEV),
                mask=(torch.rand(g.num_nodes, generator=gen) < 0.2).to(DEV), probes=torch.tensor([3, 1499, 3, 700]),
                points=points_in(g, N_POINTS, 3), seeds=points_in(g, N_SEEDS, 7),
                dt=float(((hi - lo).prod() / g.num_nodes).sqrt()) / vmax)          # the largest |v| dt is about one mean node spacing


def everything(mesh, scale=1.0):
    """Every keyword of `Rollout` that attaches something (`scale`: of the input field — the tracers' dt shrinks by it)."""
    sp = gfd.Spectrum([0, 1])
    return dict(every=2, probes=mesh["probes"], target=mesh["target"], mask=mesh["mask"], moments=True, error_moments=(1, 2), spectrum=sp,
                target_spectrum=True, derived=("div", "vort"), derived_every=2, derived_moments=1, derived_spectrum=sp, samples=mesh["points"],
                sample_moments=(1, 2), sample_spectrum=sp, sample_derived=True, tracers=(mesh["seeds"], mesh["dt"] / scale), forces=mesh["op"],
                force_moments=(0, 2), wall_moments=1, force_spectrum=sp, target_forces=True)


# ------------------------------------------------------------------ the launches of one step
LAUNCHES = ("mesh_derived", "rollout_moments", "sample_points", "rollout_spectrum", "body_forces", "tracer_advance", "rollout_advance_record",
            "rollout_advance")


def test_the_launches_of_a_step_come_in_one_order(mesh, monkeypatch):
    """(name, shape of the first tensor argument or None where the order does not tell launches apart by it, x_step, sub given)"""
    n, width, calls = int(mesh["g"].num_nodes), int(mesh["target"].size(1)), []

    def recorded(name, fn):
        def call(*a, **k):
            first = next((t for t in a if torch.is_tensor(t)), None)
            calls.append((name, None if first is None or name in ("tracer_advance", "rollout_advance_record") else tuple(first.shape),
                          k.get("x_step", 0), k.get("sub") is not None))
            return fn(*a, **k)
        return call

    for name in LAUNCHES:
        monkeypatch.setattr(ops, name, recorded(name, getattr(ops, name)))
    with Rollout(mesh["model"], mesh["g"], 2, capture=False, reorder=False, **everything(mesh)) as ro:
        del calls[:]
        ro.run(2)
    step = [("mesh_derived", (n, NF), 0, False),
            ("rollout_moments", (n, ND), 0, False),
            ("sample_points", (n, NF), 0, False),
            ("sample_points", (n, ND), 0, False),
            ("rollout_moments", (N_POINTS, NF), 0, False),
            ("rollout_spectrum", (N_POINTS, NF), 0, False),
            ("body_forces", (n, NF), 0, False),
            ("rollout_moments", (2, 3), 0, False),
            ("rollout_moments", (104, 2), 0, False),
            ("rollout_spectrum", (2, 3), 0, False),
            ("body_forces", (n, width), NF, False),
            ("rollout_moments", (n, NF), 0, False),
            ("rollout_moments", (n, NF), 0, True),
            ("rollout_spectrum", (n, NF), 0, False),
            ("rollout_spectrum", (n, width), NF, False),
            ("rollout_spectrum", (n, ND), 0, False),
            ("tracer_advance", None, 0, False),
            ("rollout_advance_record", None, 0, False)]
    assert len(calls) == 2 * len(step), calls
    for t in range(2):
        for i, (got, want) in enumerate(zip(calls[t * len(step):(t + 1) * len(step)], step)):
            assert got == want, (t, i, got, want)


# ------------------------------------------------------------------ the parts do not interfere
FAMILIES = {          # name: (the keywords that attach it and what it needs, the accessors compared)
    "records": (("every", "probes", "target", "mask"), ("result", "probes", "errors")),
    "moments": (("moments",), ("moments",)),
    "error_moments": (("error_moments", "target"), ("error_moments",)),
    "spectra": (("spectrum", "target_spectrum", "target"), ("spectrum", "target_spectrum")),
    "derived": (("derived", "derived_every", "derived_moments", "derived_spectrum"), ("derived", "derived_spectrum")),
    "samples": (("samples", "sample_moments", "sample_spectrum", "sample_derived", "derived"), ("samples",)),
    "tracers": (("tracers",), ("tracers",)),
    "forces": (("forces", "force_moments", "wall_moments", "force_spectrum", "target_forces", "target"), ("forces",)),
}


def flat(value, name, out):
    """The tensors, numbers and names a result holds, by dotted attribute path (nested `Rollout*` results are walked)."""
    if torch.is_tensor(value) or value is None or isinstance(value, (bool, int, float, str, tuple, list)):
        out[name] = value
    elif type(value).__name__.startswith("Rollout"):
        for k, v in vars(value).items():
            flat(v, f"{name}.{k}", out)
    return out


def run(mesh, scenario, accessors, **kw):
    g, f0 = mesh["g"], mesh["g"].field
    try:
        g.field = f0 * 1e5 if scenario == "clipped" else f0
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            with Rollout(mesh["model"], g, N_OUT, reorder=False, **kw) as ro:
                if scenario == "rewound":
                    ro.run(3)
                    ro.rewind()
                    ro.run(4)
                else:
                    ro.run(N_OUT)
                out = {}
                for name in accessors:
                    flat(getattr(ro, name)(), name, out)
                assert ro.exact_range == (scenario == "clipped")
                return out
    finally:
        g.field = f0


@pytest.mark.parametrize("scenario", ["straight", "rewound", "clipped"])
def test_no_part_changes_what_another_returns(mesh, scenario):
    kw = everything(mesh, 1e5 if scenario == "clipped" else 1.0)
    together = run(mesh, scenario, [a for _, accessors in FAMILIES.values() for a in accessors], **kw)
    steps = 5 if scenario == "rewound" else N_OUT
    assert together["moments.count"] == steps - (scenario == "rewound") and together["forces.moments.count"] > 0 and together["samples.spectrum.count"] > 0
    assert tuple(together["errors.sums"].shape) == (steps, NF, 6) and tuple(together["tracers.paths"].shape) == (N_SEEDS, 2 * N_OUT)
    compared = 0
    for family, (keywords, accessors) in FAMILIES.items():
        alone = run(mesh, scenario, accessors, **{k: kw[k] for k in keywords})
        mine = {k: v for k, v in together.items() if k.split(".")[0] in accessors}
        assert sorted(alone) == sorted(mine) and any(torch.is_tensor(v) for v in alone.values()), (family, sorted(alone), sorted(mine))
        for k, v in alone.items():
            same = torch.equal(v, mine[k]) if torch.is_tensor(v) else v == mine[k]
            assert same, f"{scenario}: {k} of a rollout with everything attached differs from that of a rollout with {family} alone"
            compared += torch.is_tensor(v)
    # tensors: records 10, moments 5, error_moments 5, spectra 2 x 7, derived 6 + 5 + 7, samples 5 + 5 + 7, tracers 6, forces 7 + 5 + 5 + 7
    assert compared >= 99, compared
