"""Launch time of g4c_rollout_spectrum, 100k nodes, nf = 3, K = 4, 16 and 64 frequencies, alone (with its fraction of 8 TB/s beside
the moments launch's, the same access pattern) and off its window, and the captured headline step with a spectrum on and off
(profiles/r17_rollout_spectrum_times.log).  Every launch variant is a hipGraph of LAUNCHES consecutive calls (as the launch runs
inside a captured rollout), timed with device events, the variants alternated REPS times.

--headline-only --tree DIR times the headline step of ANOTHER checkout (the parent commit's, with its own library) with this script:
only the spectrum-off rollout, which needs nothing this feature adds.  Run it alternately with this tree's in the same visit."""
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
HAS_SPECTRUM = hasattr(ops, "rollout_spectrum")
N, NF, BINS = 100_000, 3, (4, 16, 64)
LAUNCHES, REPS = (20, 2) if a.short else (100, 10)
HBM = 8e12                                                     # bytes / s
g = torch.Generator().manual_seed(0)

if not a.headline_only:
    pred = torch.randn(N, NF, generator=g).to(DEV)
    fixed = torch.tensor([1, 0], dtype=torch.int32, device=DEV)          # the step after the origin's: the steady state, launch after launch

    def spectrum(K, origin):
        planes = torch.zeros(ops.spectrum_planes(NF, K), N, dtype=torch.float64, device=DEV)
        tw = ops.spectrum_table(freqs=[0.5 * k / K for k in range(K)], samples=LAUNCHES, taper="hann")[0].to(DEV)
        return (torch.tensor([origin, -1], dtype=torch.int32, device=DEV), tw) + tuple(planes.split((NF, NF, NF * K, NF * K)))

    def moments():
        pairs = ops.moment_pairs(NF)
        planes = torch.zeros(4 * NF + pairs, N, dtype=torch.float64, device=DEV)
        return (torch.tensor([0, -1], dtype=torch.int32, device=DEV),) + tuple(planes.split((NF, NF, pairs, NF, NF)))

    on, off, mom = {K: spectrum(K, 0) for K in BINS}, spectrum(16, LAUNCHES + 5), moments()
    # bytes of a launch: every accumulator read and written, the sample read (the moments: 4 nf + nf (nf + 1) / 2 planes)
    VARIANTS = {f"spectrum alone, K = {K:2d}, fixed step": (lambda K=K: ops.rollout_spectrum(pred, fixed, NF, LAUNCHES, *on[K]),
                                                           (2 * (2 * NF * K + NF) * 8 + 4 * NF) * N) for K in BINS}
    VARIANTS["off-window spectrum alone, K = 16"] = (lambda: ops.rollout_spectrum(pred, fixed, NF, LAUNCHES, *off), 0)
    VARIANTS["moments alone, fixed step"] = (lambda: ops.rollout_moments(pred, fixed, NF, LAUNCHES, *mom),
                                             (2 * (4 * NF + ops.moment_pairs(NF)) * 8 + 4 * NF) * N)
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
    assert all(acc[0].tolist() == [0, 1] for acc in on.values()) and off[0].tolist() == [LAUNCHES + 5, -1] and mom[0].tolist() == [0, 1]
    times = {k: [] for k in graphs}
    for rep in range(REPS):
        for name, gr in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            gr.replay()
            e1.record()
            e1.synchronize()
            times[name].append(1e3 * e0.elapsed_time(e1) / LAUNCHES)
    print(f"launch time, {N} nodes, nf {NF}: us per call (a hipGraph of {LAUNCHES} calls, {REPS} alternated repetitions); bytes of a launch "
          "/ median time as a fraction of 8 TB/s")
    out = {}
    for name, t in times.items():
        t = sorted(t)
        nbytes = VARIANTS[name][1]
        frac = nbytes / (t[len(t) // 2] * 1e-6) / HBM
        out[name] = dict(median=t[len(t) // 2], min=t[0], max=t[-1], bytes=nbytes, fraction_of_8TBs=frac)
        tail = f"   {nbytes / 1e6:7.1f} MB   {100 * frac:5.1f} % of 8 TB/s" if nbytes else ""
        print(f"  {name:40s} median {t[len(t) // 2]:7.2f}   min {t[0]:7.2f}   max {t[-1]:7.2f}{tail}")
    print("JSON " + json.dumps({"launch_us": out}))

if not (a.short or a.no_headline):
    # the captured headline step (bench.py: NsThreeScaleGNN, 100k nodes, 2-D, f16x3) with the spectrum of the prediction on and off
    K, WARM = 100, 5
    graph = S.mus_graph(100_000, levels=3, dim=2, seed=0, device=DEV)
    graph.batch = torch.zeros(graph.num_nodes, dtype=torch.long, device=DEV)
    torch.manual_seed(0)
    model = gfd.nn.NsThreeScaleGNN(arch=S.mus_arch("NsThreeScaleGNN", 128), device=DEV)
    model.eval()
    steps = K + WARM + 4
    runs = {"spectrum off": Rollout(model, graph.clone(), steps, capture=True)}
    if HAS_SPECTRUM and not a.headline_only:
        spec = gfd.Spectrum(freqs=[0.5 * k / 16 for k in range(16)])
        runs["spectrum on: K = 16, every step"] = Rollout(model, graph.clone(), steps, capture=True, spectrum=spec)
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
        print(f"  {name:34s} median {t[len(t) // 2]:8.4f}   min {t[0]:8.4f}   max {t[-1]:8.4f}")
    res = {"headline_ms": {k: sorted(v) for k, v in ht.items()}}
    if len(runs) > 1:
        on = runs["spectrum on: K = 16, every step"]
        res["results_equal"] = torch.equal(runs["spectrum off"].result(), on.result())
        sp = on.spectrum()
        print(f"  results equal with the spectrum on and off: {res['results_equal']}; {sp}; dominant frequency of field 0: {sp.dominant()}")
    print("JSON " + json.dumps(res))
