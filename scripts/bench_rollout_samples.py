"""Launch time of g4c_sample_points, 100k nodes, nf = 3, k = 6, at P = 1 000 (a rake), 131 072 (a 512 x 256 raster) and 1 048 576
points, alone, with its algorithmic bytes as a fraction of 8 TB/s, and the captured headline step with samples off, on (the rake) and
at the raster's size (profiles/r19_rollout_samples_times.log).  Every launch variant is a hipGraph of LAUNCHES consecutive calls (as
the launch runs inside a captured rollout), timed with device events, the variants alternated REPS times.

--headline-only --tree DIR times the headline step of ANOTHER checkout (the parent commit's, with its own library) with this script:
only the samples-off rollout, which needs nothing this feature adds.  Run it alternately with this tree's in the same visit."""
import argparse
import json
import os
import sys
import time

import torch

ap = argparse.ArgumentParser()
ap.add_argument("--short", action="store_true", help="few launches, no headline part")
ap.add_argument("--no-headline", action="store_true")
ap.add_argument("--headline-only", action="store_true")
ap.add_argument("--tree", default=None, help="root of the checkout to import graphs4cfd_amd from (default: this one)")
a = ap.parse_args()
ROOT = os.path.abspath(a.tree) if a.tree else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))          # scripts/..
sys.path.insert(0, ROOT)
from graphs4cfd_amd import ops, synthetic as S                 # noqa: E402
import graphs4cfd_amd as gfd                                   # noqa: E402
from graphs4cfd_amd.nn.model import Rollout                    # noqa: E402

DEV = torch.device("cuda", 0)
HAS_SAMPLES = hasattr(ops, "sample_points")
N, NF, KNN, POINTS = 100_000, 3, 6, (1_000, 131_072, 1_048_576)
LAUNCHES, REPS = (20, 2) if a.short else (100, 10)
HBM = 8e12                                                     # bytes / s


def in_box(graph, p, seed):
    """p uniform random points in the bounding box of the mesh (host)."""
    lo, hi = graph.pos.min(0).values.cpu(), graph.pos.max(0).values.cpu()
    return lo + (hi - lo) * torch.rand(p, int(graph.pos.size(1)), generator=torch.Generator().manual_seed(seed))


graph = S.mus_graph(N, levels=3, dim=2, seed=0, device=DEV)
graph.batch = torch.zeros(graph.num_nodes, dtype=torch.long, device=DEV)

if not a.headline_only:
    pred = torch.randn(N, NF, generator=torch.Generator().manual_seed(0)).to(DEV)
    samplers = {"rake: a line of 1 000 points": gfd.PointSampler.line(graph, graph.pos.min(0).values.cpu(), graph.pos.max(0).values.cpu(), POINTS[0]),
                "raster: 512 x 256 points": gfd.PointSampler.grid(graph, (512, 256)),
                "1 048 576 random points": gfd.PointSampler(graph, in_box(graph, POINTS[2], 1))}
    # algorithmic bytes of a launch: per point k indices and k coefficients, k rows of nf values gathered, nf values written
    VARIANTS = {}
    for name, s in samplers.items():
        cur = torch.zeros(s.n_points, NF, device=DEV)
        VARIANTS[name] = (lambda s=s, cur=cur: ops.sample_points(pred, s._idx, s._coef, cur), s.n_points * (8 * KNN + 4 * KNN * NF + 4 * NF))
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
    print(f"launch time of g4c_sample_points, {N} nodes, nf {NF}, k {KNN}: us per call (a hipGraph of {LAUNCHES} calls, {REPS} alternated "
          "repetitions); algorithmic bytes of a launch / median time as a fraction of 8 TB/s")
    out = {}
    for name, t in times.items():
        t = sorted(t)
        nbytes = VARIANTS[name][1]
        frac = nbytes / (t[len(t) // 2] * 1e-6) / HBM
        out[name] = dict(median=t[len(t) // 2], min=t[0], max=t[-1], bytes=nbytes, fraction_of_8TBs=frac)
        print(f"  {name:32s} median {t[len(t) // 2]:7.2f}   min {t[0]:7.2f}   max {t[-1]:7.2f}   {nbytes / 1e6:7.2f} MB   {100 * frac:5.2f} % of 8 TB/s")
    print("JSON " + json.dumps({"launch_us": out}))

if not (a.short or a.no_headline):
    # the captured headline step (bench.py: NsThreeScaleGNN, 100k nodes, 2-D, f16x3) with samples off, on a rake and on a raster
    K, WARM = 100, 5
    torch.manual_seed(0)
    model = gfd.nn.NsThreeScaleGNN(arch=S.mus_arch("NsThreeScaleGNN", 128), device=DEV)
    model.eval()
    steps = K + WARM + 4
    runs = {"samples off": Rollout(model, graph.clone(), steps, capture=True)}
    if HAS_SAMPLES and not a.headline_only:
        runs["samples on: the rake, every step"] = Rollout(model, graph.clone(), steps, capture=True, samples=samplers["rake: a line of 1 000 points"])
        runs["samples on: the raster, no series"] = Rollout(model, graph.clone(), steps, capture=True, samples=samplers["raster: 512 x 256 points"],
                                                            sample_every=0)
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
        print(f"  {name:36s} median {t[len(t) // 2]:8.4f}   min {t[0]:8.4f}   max {t[-1]:8.4f}")
    res = {"headline_ms": {k: sorted(v) for k, v in ht.items()}}
    if len(runs) > 1:
        res["results_equal"] = all(torch.equal(runs["samples off"].result(), ro.result()) for ro in runs.values())
        rs = runs["samples on: the rake, every step"].samples()
        print(f"  results equal with samples on and off: {res['results_equal']}; {rs}")
    print("JSON " + json.dumps(res))
