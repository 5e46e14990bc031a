"""Launch time of g4c_mesh_derived (with its statistics launch: "the pair"), 100k nodes, k = 6, nf = 3, ("div", "vort"), alone and in
front of g4c_rollout_advance, on the mesh as numbered and on its Morton renumbering (what a rollout of this size runs on), and the
captured headline step with the diagnostics on and off (profiles/r15_mesh_derived_times.log).  Every launch variant is a hipGraph of
LAUNCHES consecutive calls (as the launch runs inside a captured rollout), timed with device events, the variants alternated REPS
times; median (min - max).

--headline-only --tree DIR times the headline step of ANOTHER checkout (the parent commit's, with its own library) with this script:
only the diagnostics-off rollout, which needs nothing this feature adds.  Run it alternately with this tree's in the same visit."""
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
HAS_DERIVED = hasattr(ops, "mesh_derived")
N, NF, NAMES = 100_000, 3, ("div", "vort")
COPY_RATE = 6.3e12          # bytes/s: the copy rate DESIGN.md section 5 quotes
LAUNCHES, REPS = (20, 2) if a.short else (100, 10)
gen = torch.Generator().manual_seed(0)
graph = S.mus_graph(N, levels=3, dim=2, seed=0, device=DEV)          # bench.py's mesh: kNN, k = 6
graph.batch = torch.zeros(graph.num_nodes, dtype=torch.long, device=DEV)

if not a.headline_only:
    from graphs4cfd_amd.reorder import reorder_nodes
    pred = torch.randn(N, NF, generator=gen).to(DEV)
    field = torch.randn(N, NF, generator=gen).to(DEV)
    outputs = torch.zeros(LAUNCHES, N, NF, device=DEV)
    step = torch.zeros(2, dtype=torch.int32, device=DEV)
    fixed = torch.tensor([1, 0], dtype=torch.int32, device=DEV)
    ops_by_numbering = {"as numbered": gfd.MeshGradient(graph), "Morton": gfd.MeshGradient(reorder_nodes(graph)[0])}
    prog = ops_by_numbering["Morton"].program(NAMES, NF)
    nd = int(prog.nd)
    n_edges = int(ops_by_numbering["Morton"].src.numel())
    # what the algorithm has to move once: x, g, src, off in, cur out (the gathered rows of x counted once; the partials are KB)
    algo_bytes = 4 * (N * NF + n_edges * 2 + n_edges + (N + 1) + N * nd)

    def buffers():
        return dict(cur=torch.zeros(N, nd, device=DEV), stats=torch.zeros(LAUNCHES, nd, 3, dtype=torch.float64, device=DEV),
                    scratch=ops.mesh_derived_scratch(N, nd, DEV))

    def advance():
        ops.rollout_advance(field, pred, outputs, step, NF)

    def derived(op, b, st, stats=True):
        if stats:
            ops.mesh_derived(pred, op.off, op.g, op.src, prog, b["cur"], step=st, stats=b["stats"], scratch=b["scratch"], max_steps=LAUNCHES)
        else:
            ops.mesh_derived(pred, op.off, op.g, op.src, prog, b["cur"])

    VARIANTS = {"advance alone": (advance, True)}
    for name, op in ops_by_numbering.items():
        b1, b2, b3 = buffers(), buffers(), buffers()
        VARIANTS[f"derived pair alone, fixed step ({name})"] = (lambda op=op, b=b1: derived(op, b, fixed), False)
        VARIANTS[f"derived without statistics ({name})"] = (lambda op=op, b=b2: derived(op, b, fixed, stats=False), False)
        VARIANTS[f"derived pair + advance ({name})"] = (lambda op=op, b=b3: (derived(op, b, step), advance()), True)
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
    times = {k: [] for k in graphs}
    for rep in range(REPS):
        for name, gr in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            gr.replay()
            e1.record()
            e1.synchronize()
            times[name].append(1e3 * e0.elapsed_time(e1) / LAUNCHES)
    print(f"launch time, {N} nodes, {n_edges} edges, nf {NF}, {NAMES}: us per call (a hipGraph of {LAUNCHES} calls, {REPS} alternated repetitions)")
    out = {}
    for name, t in times.items():
        t = sorted(t)
        out[name] = dict(median=t[len(t) // 2], min=t[0], max=t[-1])
        print(f"  {name:50s} median {t[len(t) // 2]:7.2f}   min {t[0]:7.2f}   max {t[-1]:7.2f}")
    print(f"  algorithmic bytes of one call: {algo_bytes} = {1e6 * algo_bytes / COPY_RATE:.2f} us at {COPY_RATE / 1e12:.1f} TB/s")
    print("JSON " + json.dumps({"launch_us": out, "algorithmic_bytes": algo_bytes}))

if not (a.short or a.no_headline):
    # the captured headline step (bench.py: NsThreeScaleGNN, 100k nodes, 2-D, f16x3) with the diagnostics on and off
    K, WARM = 100, 5
    torch.manual_seed(0)
    model = gfd.nn.NsThreeScaleGNN(arch=S.mus_arch("NsThreeScaleGNN", 128), device=DEV)
    model.eval()
    steps = K + WARM + 4
    runs = {"diagnostics off": Rollout(model, graph.clone(), steps, capture=True)}
    if HAS_DERIVED and not a.headline_only:
        runs["diagnostics on: div, vort"] = Rollout(model, graph.clone(), steps, capture=True, derived=NAMES)
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
        on = runs["diagnostics on: div, vort"]
        res["results_equal"] = torch.equal(runs["diagnostics off"].result(), on.result())
        d = on.derived()
        print(f"  results equal with diagnostics on and off: {res['results_equal']}; {d}; rms of the last step {d.rms[-1].tolist()}")
    print("JSON " + json.dumps(res))
