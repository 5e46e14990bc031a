"""Launch time of g4c_rollout_moments, 100k nodes, nf = 3, with and without `sub`, alone and in front of g4c_rollout_advance, and the
captured headline step with the time statistics on and off (profiles/r14_rollout_moments_times.log).  Every launch variant is a
hipGraph of LAUNCHES consecutive calls (as the launch runs inside a captured rollout), timed with device events, the variants
alternated REPS times.

--headline-only --tree DIR times the headline step of ANOTHER checkout (the parent commit's, with its own library) with this script:
only the moments-off rollout, which needs nothing this feature adds.  Run it alternately with this tree's in the same visit."""
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
HAS_MOMENTS = hasattr(ops, "rollout_moments")
N, NF = 100_000, 3
LAUNCHES, REPS = (20, 2) if a.short else (100, 10)
g = torch.Generator().manual_seed(0)

if not a.headline_only:
    pairs = ops.moment_pairs(NF)
    pred = torch.randn(N, NF, generator=g).to(DEV)
    field = torch.randn(N, NF, generator=g).to(DEV)
    sub = torch.randn(N, NF * LAUNCHES, generator=g).to(DEV)
    outputs = torch.zeros(LAUNCHES, N, NF, device=DEV)
    step = torch.zeros(2, dtype=torch.int32, device=DEV)
    fixed = torch.tensor([1, 0], dtype=torch.int32, device=DEV)          # the step after the origin's: the steady state, launch after launch

    def accumulators(origin):
        planes = torch.zeros(4 * NF + pairs, N, dtype=torch.float64, device=DEV)
        return (torch.tensor([origin, -1], dtype=torch.int32, device=DEV),) + tuple(planes.split((NF, NF, pairs, NF, NF)))

    acc, acc_sub, acc_off = accumulators(0), accumulators(0), accumulators(LAUNCHES + 5)
    fix, fix_sub = accumulators(0), accumulators(0)

    def advance():
        ops.rollout_advance(field, pred, outputs, step, NF)

    def moments(st, accs, s=None):
        ops.rollout_moments(pred, st, NF, LAUNCHES, *accs, stride=1, sub=s)

    VARIANTS = {
        "advance alone": (advance, True),
        "moments + advance": (lambda: (moments(step, acc), advance()), True),
        "moments(sub) + advance": (lambda: (moments(step, acc_sub, sub), advance()), True),
        "off-window moments + advance": (lambda: (moments(step, acc_off), advance()), True),
        "moments alone, fixed step": (lambda: moments(fixed, fix), False),
        "moments(sub) alone, fixed step": (lambda: moments(fixed, fix_sub, sub), False),
        "off-window moments alone": (lambda: moments(fixed, acc_off), False),
    }
    graphs = {}
    for name, (fn, steps) in VARIANTS.items():
        step.zero_()
        fn()                                       # warm: code object loaded
        torch.cuda.synchronize(DEV)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            step.zero_()
            for _ in range(LAUNCHES):
                fn()
        gr.replay()
        torch.cuda.synchronize(DEV)
        assert step.tolist() == [LAUNCHES if steps else 0, 0], (name, step.tolist())
        graphs[name] = gr
    assert acc[0].tolist() == [0, LAUNCHES - 1] and acc_sub[0].tolist() == [0, LAUNCHES - 1] and acc_off[0].tolist() == [LAUNCHES + 5, -1] and fix[0].tolist() == [0, 1]
    times = {k: [] for k in graphs}
    for rep in range(REPS):
        for name, gr in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            gr.replay()
            e1.record()
            e1.synchronize()
            times[name].append(1e3 * e0.elapsed_time(e1) / LAUNCHES)
    print(f"launch time, {N} nodes, nf {NF}: us per call (a hipGraph of {LAUNCHES} calls, {REPS} alternated repetitions)")
    out = {}
    for name, t in times.items():
        t = sorted(t)
        out[name] = dict(median=t[len(t) // 2], min=t[0], max=t[-1])
        print(f"  {name:34s} median {t[len(t) // 2]:7.2f}   min {t[0]:7.2f}   max {t[-1]:7.2f}")
    print("JSON " + json.dumps({"launch_us": out}))

if not (a.short or a.no_headline):
    # the captured headline step (bench.py: NsThreeScaleGNN, 100k nodes, 2-D, f16x3) with the statistics of the prediction on and off
    K, WARM = 100, 5
    graph = S.mus_graph(100_000, levels=3, dim=2, seed=0, device=DEV)
    graph.batch = torch.zeros(graph.num_nodes, dtype=torch.long, device=DEV)
    torch.manual_seed(0)
    model = gfd.nn.NsThreeScaleGNN(arch=S.mus_arch("NsThreeScaleGNN", 128), device=DEV)
    model.eval()
    steps = K + WARM + 4
    runs = {"moments off": Rollout(model, graph.clone(), steps, capture=True)}
    if HAS_MOMENTS and not a.headline_only:
        runs["moments on: every step"] = Rollout(model, graph.clone(), steps, capture=True, moments=True)
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
        print(f"  {name:28s} median {t[len(t) // 2]:8.4f}   min {t[0]:8.4f}   max {t[-1]:8.4f}")
    res = {"headline_ms": {k: sorted(v) for k, v in ht.items()}}
    if len(runs) > 1:
        on = runs["moments on: every step"]
        res["results_equal"] = torch.equal(runs["moments off"].result(), on.result())
        mo = on.moments()
        print(f"  results equal with moments on and off: {res['results_equal']}; {mo}; mean of the node variances {mo.var.mean(0).tolist()}")
    print("JSON " + json.dumps(res))
