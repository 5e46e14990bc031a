"""Launch time of g4c_tracer_advance, 100k nodes, nf = 3, k = 6, at P = 1 000, 131 072 and 1 048 576 particles, for both schemes, the
seeds a rake (a line across the mesh: neighbouring lanes scan the same cells) and uniformly random (every lane scans cells of its
own), alone; and the captured headline step with tracers off and on.  Every launch variant is a hipGraph of LAUNCHES consecutive
calls (as the launch runs inside a captured rollout), timed with device events, the variants alternated REPS times.  The particles
move by about a thousandth of a node spacing a launch: the work of a launch stays what it was at the seeds.

--headline-only --tree DIR times the headline step of ANOTHER checkout (the parent commit's, with its own library) with this script:
only the tracers-off rollout, which needs nothing this feature adds.  Run it alternately with this tree's in the same visit."""
import argparse
import json
import os
import sys
import time

import torch

ap = argparse.ArgumentParser()
ap.add_argument("--short", action="store_true", help="few launches, no headline part")
ap.add_argument("--no-headline", action="store_true")
ap.add_argument("--no-launch", action="store_true", help="the headline part only, tracers on and off")
ap.add_argument("--headline-only", action="store_true")
ap.add_argument("--tree", default=None, help="root of the checkout to import graphs4cfd_amd from (default: this one)")
a = ap.parse_args()
ROOT = os.path.abspath(a.tree) if a.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))          # scripts/..
sys.path.insert(0, ROOT)
from graphs4cfd_amd import ops, synthetic as S                 # noqa: E402
import graphs4cfd_amd as gfd                                   # noqa: E402
from graphs4cfd_amd.nn.model import Rollout                    # noqa: E402

DEV = torch.device("cuda", 0)
HAS_TRACERS = hasattr(ops, "tracer_advance")
N, NF, KNN, PARTICLES = 100_000, 3, 6, (1_000, 131_072, 1_048_576)
LAUNCHES, REPS = (10, 2) if a.short else (50, 10)


def seeds_of(graph, p, how, seed=1):
    lo, hi = graph.pos.min(0).values.cpu(), graph.pos.max(0).values.cpu()
    if how == "rake":
        t = (torch.arange(p, dtype=torch.float64) / max(p - 1, 1))[:, None]
        return (lo.double() + t * (hi - lo).double()).float()
    return lo + (hi - lo) * torch.rand(p, int(graph.pos.size(1)), generator=torch.Generator().manual_seed(seed))


graph = S.mus_graph(N, levels=3, dim=2, seed=0, device=DEV)
graph.batch = torch.zeros(graph.num_nodes, dtype=torch.long, device=DEV)
lo, hi = graph.pos.min(0).values, graph.pos.max(0).values
SPACING = float(((hi - lo).prod() / N).sqrt())

if not (a.headline_only or a.no_launch):
    gen = torch.Generator().manual_seed(0)
    x0, x1 = torch.randn(N, NF, generator=gen).to(DEV), torch.randn(N, NF, generator=gen).to(DEV)
    VARIANTS = {}
    for p in PARTICLES:
        for how in ("rake", "random"):
            for scheme in ("euler", "heun"):
                tr = gfd.Tracers(graph, seeds_of(graph, p, how), 1e-3 * SPACING, scheme=scheme, k=KNN)
                VARIANTS[f"{p:>9,d} {how:6s} {scheme:5s}".replace(",", " ")] = (lambda tr=tr: tr.advance(x0, x1, 0), tr)
    graphs = {}
    for name, (fn, _) in VARIANTS.items():
        fn()                                       # warm: code object loaded
        torch.cuda.synchronize(DEV)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for _ in range(LAUNCHES):
                fn()
        gr.replay()
        torch.cuda.synchronize(DEV)
        graphs[name] = gr
    times = {k: [] for k in graphs}
    for rep in range(REPS):
        for name, gr in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            gr.replay()
            e1.record()
            e1.synchronize()
            times[name].append(1e3 * e0.elapsed_time(e1) / LAUNCHES)
    print(f"launch time of g4c_tracer_advance, {N} nodes, nf {NF}, k {KNN}: us per call (a hipGraph of {LAUNCHES} calls, {REPS} alternated "
          "repetitions); particles per us at the median")
    out = {}
    for name, t in times.items():
        t = sorted(t)
        tr = VARIANTS[name][1]
        moving = int((tr.status == 1).sum())
        out[name] = dict(median=t[len(t) // 2], min=t[0], max=t[-1], particles=tr.n_particles, moving=moving)
        print(f"  {name:28s} median {t[len(t) // 2]:9.2f}   min {t[0]:9.2f}   max {t[-1]:9.2f}   {tr.n_particles / t[len(t) // 2]:9.1f} particles / us   "
              f"({moving} still moving)")
    print("JSON " + json.dumps({"launch_us": out}))

if not (a.short or a.no_headline):
    # the captured headline step (bench.py: NsThreeScaleGNN, 100k nodes, 2-D, f16x3) with tracers off, and on at two sizes
    K, WARM = 100, 5
    torch.manual_seed(0)
    model = gfd.nn.NsThreeScaleGNN(arch=S.mus_arch("NsThreeScaleGNN", 128), device=DEV)
    model.eval()
    steps = K + WARM + 4
    runs = {"tracers off": Rollout(model, graph.clone(), steps, capture=True)}
    if HAS_TRACERS and not a.headline_only:
        # The untrained model's velocity grows step after step and the timed rollouts go on from one another's field: without limits
        # the particles end up hundreds of cells off the mesh, where the exact ring search scans the whole grid at every stage.  As a
        # user would: a particle that leaves the mesh's bounding box, or is two spacings from every node, is frozen.
        kw = dict(box=(lo.tolist(), hi.tolist()), max_distance=2 * SPACING)
        dt = 1e-2 * SPACING
        runs["tracers on: a rake of 1 000, heun, every step"] = Rollout(model, graph.clone(), steps, capture=True,
                                                                       tracers=(seeds_of(graph, 1_000, "rake"), dt, kw))
        runs["tracers on: 131 072 random, heun, no series"] = Rollout(model, graph.clone(), steps, capture=True,
                                                                     tracers=(seeds_of(graph, 131_072, "random"), dt, kw), tracer_every=0)
    for ro in runs.values():
        ro.run(2 + WARM)
    torch.cuda.synchronize(DEV)
    ht = {k: [] for k in runs}
    for rep in range(6):
        for name, ro in runs.items():
            ro.rewind()
            torch.cuda.synchronize(DEV)
            t0 = time.perf_counter()
            ro.run(K)
            ro.validate()
            torch.cuda.synchronize(DEV)
            ht[name].append(1e3 * (time.perf_counter() - t0) / K)
    where = "checkout " + os.path.basename(ROOT) if a.tree else "this checkout"
    print(f"captured headline step (NsThreeScaleGNN, 100k nodes, f16x3; {where}), ms per step over {K} replays, 6 alternated repetitions")
    for name, t in ht.items():
        t = sorted(t)
        print(f"  {name:48s} median {t[len(t) // 2]:8.4f}   min {t[0]:8.4f}   max {t[-1]:8.4f}")
    res = {"headline_ms": {k: sorted(v) for k, v in ht.items()}}
    if len(runs) > 1:
        res["results_equal"] = all(torch.equal(runs["tracers off"].result(), ro.result()) for ro in runs.values())
        print(f"  results equal with tracers on and off: {res['results_equal']}")
        for name, ro in runs.items():
            if ro._tracers is not None:
                rt = ro.tracers()
                print(f"  {name}: {rt}; particles by status 0 .. 4: {torch.bincount(rt.status.long(), minlength=5).tolist()}")
    print("JSON " + json.dumps(res))
