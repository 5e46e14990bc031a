"""Times of the control volumes on a cloud of 100k nodes (bench.py's mesh: kNN, k = 6, 2-D): the construction (`gfd.ControlVolumes`:
binning + g4c_voronoi_cells, and the kernel alone), the per-step launches of `Rollout.open(integrals=("ke", "enstrophy", "div2", "rel_l2"))`
(g4c_weighted_integrals on the prediction, prediction − target, the target and the derived columns: four pairs of launches), the
captured headline step with the integrals off and on; and, with --parent DIR, this tree with the integrals off against the parent
commit's tree and library, headline step and bench.py, in alternated separate processes.  Every launch variant is a hipGraph of
LAUNCHES consecutive calls (as the launch runs inside a captured rollout), timed with device events, the variants alternated REPS
times; median (min - max).

--headline-only --tree DIR times the headline step of ANOTHER checkout (the parent commit's, with its own library) with this script:
only the integrals-off rollout, which needs nothing this feature adds."""
import argparse
import json
import os
import subprocess
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--short", action="store_true", help="few launches, no headline part")
ap.add_argument("--no-headline", action="store_true")
ap.add_argument("--headline-only", action="store_true")
ap.add_argument("--tree", default=None, help="root of the checkout to import graphs4cfd_amd from (default: this one)")
ap.add_argument("--parent", default=None, help="root of the parent commit's checkout, built: alternate this tree (integrals off) with it")
ap.add_argument("--pairs", type=int, default=3, help="alternated pairs of processes with --parent")
a = ap.parse_args()
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))          # scripts/..
ROOT = os.path.abspath(a.tree) if a.tree else HERE

if a.parent:
    # Fresh child processes, one at a time, this tree and the parent's in turn: each imports its own package and loads its own library.
    parent = os.path.abspath(a.parent)

    def child(cmd, cwd, key):
        done = subprocess.run(cmd, cwd=cwd, capture_output=True, text=True, timeout=600)
        if done.returncode:
            raise SystemExit(f"{' '.join(cmd)} (in {cwd}) ended with {done.returncode}:\n{done.stderr[-2000:]}")
        rows = [json.loads(ln[5:] if ln.startswith("JSON ") else ln) for ln in done.stdout.splitlines() if ln.startswith("JSON ") or ln.startswith("{")]
        return [r for r in rows if key in r][-1][key]

    head = {"this tree": [], "parent": []}
    bench = {"this tree": [], "parent": []}
    for pair in range(a.pairs):
        for name, tree in (("this tree", HERE), ("parent", parent)):
            ms = child([sys.executable, os.path.abspath(__file__), "--headline-only", "--tree", tree], HERE, "headline_ms")["integrals off"]
            head[name].append(ms[len(ms) // 2])
            bench[name].append(child([sys.executable, "bench.py", "--gpus", "1", "--steps", "200", "--warmup", "20"], tree, "value"))
            print(f"  pair {pair} {name:9s} headline median {head[name][-1]:8.4f} ms / step   bench.py {bench[name][-1]}", flush=True)
    for label, rows in (("captured headline step, integrals off, ms per step (median of 6 in each process)", head), ("bench.py --steps 200 --warmup 20, value", bench)):
        print(label)
        for name, v in rows.items():
            print(f"  {name:9s} {['%.4f' % x for x in v]}   min {min(v):.4f}   max {max(v):.4f}   spread {max(v) - min(v):.4f}")
    print("JSON " + json.dumps({"alternated_headline_ms": head, "alternated_bench": bench}))
    sys.exit(0)

sys.path.insert(0, ROOT)
import torch                                                   # noqa: E402
from graphs4cfd_amd import ops, synthetic as S                 # noqa: E402
import graphs4cfd_amd as gfd                                   # noqa: E402
from graphs4cfd_amd.nn.model import Rollout                    # noqa: E402

DEV = torch.device("cuda", 0)
HAS_VOLUMES = hasattr(gfd, "ControlVolumes")
N, NF = 100_000, 3
LAUNCHES, REPS = (20, 2) if a.short else (100, 10)
NAMES = ("ke", "enstrophy", "div2", "rel_l2")


def timed(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize(DEV)
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize(DEV)
        out.append(1e3 * (time.perf_counter() - t0))
    return sorted(out)


graph = S.mus_graph(N, levels=3, dim=2, seed=0, device=DEV)          # bench.py's mesh
graph.batch = torch.zeros(graph.num_nodes, dtype=torch.long, device=DEV)

if HAS_VOLUMES and not a.headline_only:
    from graphs4cfd_amd.control_volumes import GRID_K
    cv = gfd.ControlVolumes(graph)          # warm: code object loaded
    grid = S._bin_cloud(graph.pos.float(), GRID_K)
    box = cv.box[0].tolist()
    out = ops.voronoi_cells(grid, box)
    build = timed(lambda: gfd.ControlVolumes(graph), 3 if a.short else 7)
    kernel = timed(lambda: ops.voronoi_cells(grid, box, out=out), 3 if a.short else 7)
    rings, nvert = cv.rings.float(), cv.nvert.float()
    print(f"construction, {N} nodes (uniform-random, bounding box): gfd.ControlVolumes median {build[len(build) // 2]:.3f} ms "
          f"(min {build[0]:.3f}, max {build[-1]:.3f}); g4c_voronoi_cells alone median {kernel[len(kernel) // 2]:.3f} ms (min {kernel[0]:.3f}, "
          f"max {kernel[-1]:.3f}); rings median {int(rings.median())} max {int(rings.max())}, vertices median {int(nvert.median())} max "
          f"{int(nvert.max())}, degenerate {int(cv.degenerate.sum())}, total − box {cv.total - (box[2] - box[0]) * (box[3] - box[1]):.3e}")
    print("JSON " + json.dumps({"construction_ms": build, "voronoi_kernel_ms": kernel, "rings_max": int(rings.max()), "nvert_max": int(nvert.max())}))

    # the per-step launches of NAMES: four sources, each g4c_weighted_integrals + its one-workgroup sum
    gen = torch.Generator().manual_seed(0)
    pred = torch.randn(N, NF, generator=gen).to(DEV)
    target = torch.randn(N, NF * LAUNCHES, generator=gen).to(DEV)
    cur = torch.randn(N, 2, generator=gen).to(DEV)
    step = torch.zeros(2, dtype=torch.int32, device=DEV)
    field, outputs = torch.randn(N, NF, generator=gen).to(DEV), torch.zeros(LAUNCHES, N, NF, device=DEV)
    sources = {"prediction: ke": dict(x=pred, entries=[(0, 0), (1, 1)], nz=NF),
               "prediction − target: rel_l2": dict(x=pred, entries=[(0, 0), (1, 1), (2, 2)], nz=NF, sub=target, sub_step=NF),
               "target: rel_l2": dict(x=target, entries=[(0, 0), (1, 1), (2, 2)], nz=NF, x_step=NF),
               "derived: enstrophy, div2": dict(x=cur, entries=[(1, 1), (0, 0)], nz=2)}
    calls = {}
    for name, kw in sources.items():
        kw = dict(kw)
        x, entries = kw.pop("x"), kw.pop("entries")
        stats = torch.zeros(LAUNCHES, len(entries), dtype=torch.float64, device=DEV)
        scratch = ops.weighted_integrals_scratch(N, len(entries), DEV)
        calls[name] = (lambda x=x, e=ops.integral_program(entries, kw["nz"]), st=stats, sc=scratch, kw=kw: ops.weighted_integrals(x, cv.area, e, st, sc, step=step, **kw))

    def advance():
        ops.rollout_advance(field, pred, outputs, step, NF)

    VARIANTS = {"advance alone": lambda: advance()}
    for name, fn in calls.items():
        VARIANTS[f"{name} + advance"] = lambda fn=fn: (fn(), advance())
    VARIANTS["all four + advance"] = lambda: ([fn() for fn in calls.values()], advance())
    graphs = {}
    for name, fn in VARIANTS.items():
        step.zero_()
        fn()
        torch.cuda.synchronize(DEV)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            step.zero_()
            for _ in range(LAUNCHES):
                fn()
        gr.replay()
        torch.cuda.synchronize(DEV)
        assert step.tolist() == [LAUNCHES, 0], (name, step.tolist())
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
    print(f"per-step launches of g4c_weighted_integrals, {N} nodes, nf {NF}: us per step (a hipGraph of {LAUNCHES} steps, {REPS} alternated repetitions)")
    res = {}
    for name, t in times.items():
        t = sorted(t)
        res[name] = dict(median=t[len(t) // 2], min=t[0], max=t[-1])
        print(f"  {name:42s} median {t[len(t) // 2]:7.2f}   min {t[0]:7.2f}   max {t[-1]:7.2f}")
    print("JSON " + json.dumps({"launch_us": res}))

if not (a.short or a.no_headline):
    # the captured headline step (bench.py: NsThreeScaleGNN, 100k nodes, 2-D, f16x3) with the integrals off and on
    K, WARM = 100, 5
    torch.manual_seed(0)
    model = gfd.nn.NsThreeScaleGNN(arch=S.mus_arch("NsThreeScaleGNN", 128), device=DEV)
    model.eval()
    steps = K + WARM + 4
    runs = {"integrals off": Rollout(model, graph.clone(), steps, capture=True)}
    if HAS_VOLUMES and not a.headline_only:
        tgt = torch.randn(N, NF * steps, generator=torch.Generator().manual_seed(1)).to(DEV)
        runs["integrals on: ke (one source)"] = Rollout.open(model, graph.clone(), steps, capture=True, integrals=("ke",), integral_volumes=cv)
        runs["integrals on: ke, enstrophy, div2, rel_l2"] = Rollout.open(model, graph.clone(), steps, capture=True, every=1, target=tgt, derived=("vort", "div"),
                                                                         integrals=NAMES, integral_volumes=cv)
        runs["the same without integrals (target, derived)"] = Rollout(model, graph.clone(), steps, capture=True, every=1, target=tgt, derived=("vort", "div"))
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
        print(f"  {name:46s} median {t[len(t) // 2]:8.4f}   min {t[0]:8.4f}   max {t[-1]:8.4f}")
    out = {"headline_ms": {k: sorted(v) for k, v in ht.items()}}
    if len(runs) > 1:
        out["results_equal"] = all(torch.equal(runs["integrals off"].result(), ro.result()) for ro in runs.values() if ro._out_steps is not None)
        print(f"  results equal with the integrals on and off: {out['results_equal']}")
        for name, ro in runs.items():
            if getattr(ro, "_integrals", None) is not None:
                print(f"  {name}: {ro.integrals()}")
    print("JSON " + json.dumps(out))
