"""Launch time of g4c_body_forces on a cloud of 100k nodes (k = 6, nf = 3) round one circular body whose wall holds W = 256 and
W = 4096 items, with and without the viscous term, alone and in front of g4c_rollout_advance; the captured headline step with the
forces on and off; and, with --parent DIR, this tree with the forces off against the parent commit's tree and library, headline step
and bench.py, in alternated separate processes (profiles/r21_body_forces_times.log).  Every launch variant is a hipGraph of LAUNCHES
consecutive calls (as the launch runs inside a captured rollout), timed with device events, the variants alternated REPS times;
median (min - max).  The launch is one workgroup per body — one dependent chain step index -> item -> off -> src -> x -> reduce —: a
latency figure, not a bandwidth figure.

--headline-only --tree DIR times the headline step of ANOTHER checkout (the parent commit's, with its own library) with this script:
only the forces-off rollout, which needs nothing this feature adds."""
import argparse
import json
import os
import subprocess
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--short", action="store_true", help="few launches, no headline part")
ap.add_argument("--no-headline", action="store_true")
ap.add_argument("--no-launch", action="store_true", help="the headline part only, forces on and off")
ap.add_argument("--headline-only", action="store_true")
ap.add_argument("--tree", default=None, help="root of the checkout to import graphs4cfd_amd from (default: this one)")
ap.add_argument("--parent", default=None, help="root of the parent commit's checkout, built: alternate this tree (forces off) with it")
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
        out = done.stdout
        rows = [json.loads(ln[5:] if ln.startswith("JSON ") else ln) for ln in out.splitlines() if ln.startswith("JSON ") or ln.startswith("{")]
        return [r for r in rows if key in r][-1][key]

    head = {"this tree": [], "parent": []}
    bench = {"this tree": [], "parent": []}
    for pair in range(a.pairs):
        for name, tree in (("this tree", HERE), ("parent", parent)):
            ms = child([sys.executable, os.path.abspath(__file__), "--headline-only", "--tree", tree], HERE, "headline_ms")["forces off"]
            head[name].append(ms[len(ms) // 2])
            bench[name].append(child([sys.executable, "bench.py", "--gpus", "1", "--steps", "200", "--warmup", "20"], tree, "value"))
            print(f"  pair {pair} {name:9s} headline median {head[name][-1]:8.4f} ms / step   bench.py {bench[name][-1]}", flush=True)
    for label, rows in (("captured headline step, forces off, ms per step (median of 6 in each process)", head), ("bench.py --steps 200 --warmup 20, value", bench)):
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
HAS_FORCES = hasattr(ops, "body_forces")
N, NF, KNN, WALLS = 100_000, 3, 6, (256, 4096)
LAUNCHES, REPS = (20, 2) if a.short else (100, 10)
MU, SCALE, SHIFT = 1e-3, [1.0, 1.0, 2.0], [0.0, 0.0, 0.5]


def ring_of(graph, m, centre=(0.5, 0.5), radius=0.1):
    """The m nodes of the cloud nearest to a circle: a wall that is star-shaped about its mean."""
    pos = graph.pos.double()
    return torch.argsort(((pos[:, 0] - centre[0]).hypot(pos[:, 1] - centre[1]) - radius).abs())[:m]


if not (a.headline_only or a.no_launch):
    import math
    gen = torch.Generator().manual_seed(0)
    pred = torch.randn(N, NF, generator=gen).to(DEV)
    field = torch.randn(N, NF, generator=gen).to(DEV)
    outputs = torch.zeros(LAUNCHES, N, NF, device=DEV)
    step = torch.zeros(2, dtype=torch.int32, device=DEV)
    fixed = torch.tensor([1, 0], dtype=torch.int32, device=DEV)

    def advance():
        ops.rollout_advance(field, pred, outputs, step, NF)

    VARIANTS = {"advance alone": (advance, True)}
    for w in WALLS:
        # W nodes on a circle of radius 0.1, the rest of the cloud uniform-random outside it
        th = 2 * math.pi * (torch.arange(w, dtype=torch.float64) + 0.25) / w
        wall = torch.stack([0.5 + 0.1 * th.cos(), 0.5 + 0.1 * th.sin()], 1).float()
        rest = torch.rand(2 * N, 2, generator=gen)
        rest = rest[((rest[:, 0] - 0.5).hypot(rest[:, 1] - 0.5) > 0.1 + 0.5 / math.sqrt(N))][:N - w]
        g = gfd.Graph(pos=torch.cat([wall, rest]).to(DEV))
        g.edge_index, _ = S.connect_knn(g.pos, KNN)
        for mu in (0.0, MU):
            bf = gfd.BodyForces(g, torch.arange(w), mu=mu, scale=SCALE, shift=SHIFT)
            grad = bf.gradient
            kw = dict(bf.constants(), off=grad and grad.off, g=grad and grad.g, src=grad and grad.src, max_steps=LAUNCHES)

            def forces(st, bf=bf, kw=kw, b=dict(cur=torch.zeros(1, 3, device=DEV), wall=torch.zeros(w, 2, device=DEV),
                                                stats=torch.zeros(LAUNCHES, 1, 6, dtype=torch.float64, device=DEV))):
                ops.body_forces(pred, bf._item32, bf.body_offsets, bf.area, bf.unit, bf.arm, b["cur"], wall=b["wall"], stats=b["stats"], step=st, **kw)

            tag = f"W {w:5d}, {'viscous ' if mu else 'pressure'}"
            VARIANTS[f"forces alone, fixed step ({tag})"] = (lambda f=forces: f(fixed), False)
            VARIANTS[f"forces + advance ({tag})"] = (lambda f=forces: (f(step), advance()), True)
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
    print(f"launch time of g4c_body_forces, {N} nodes, k {KNN}, nf {NF}, one body: us per call (a hipGraph of {LAUNCHES} calls, {REPS} alternated repetitions)")
    out = {}
    for name, t in times.items():
        t = sorted(t)
        out[name] = dict(median=t[len(t) // 2], min=t[0], max=t[-1])
        print(f"  {name:52s} median {t[len(t) // 2]:7.2f}   min {t[0]:7.2f}   max {t[-1]:7.2f}")
    print("JSON " + json.dumps({"launch_us": out}))

if not (a.short or a.no_headline):
    # the captured headline step (bench.py: NsThreeScaleGNN, 100k nodes, 2-D, f16x3) with the forces off and on
    K, WARM = 100, 5
    graph = S.mus_graph(N, levels=3, dim=2, seed=0, device=DEV)          # bench.py's mesh: kNN, k = 6
    graph.batch = torch.zeros(graph.num_nodes, dtype=torch.long, device=DEV)
    torch.manual_seed(0)
    model = gfd.nn.NsThreeScaleGNN(arch=S.mus_arch("NsThreeScaleGNN", 128), device=DEV)
    model.eval()
    steps = K + WARM + 4
    runs = {"forces off": Rollout(model, graph.clone(), steps, capture=True)}
    if HAS_FORCES and not a.headline_only:
        bf = gfd.BodyForces(graph, ring_of(graph, 256), mu=MU, scale=SCALE, shift=SHIFT)
        runs["forces on: W 256, viscous"] = Rollout(model, graph.clone(), steps, capture=True, forces=bf)
        runs["forces on: + moments, wall moments, spectrum"] = Rollout(model, graph.clone(), steps, capture=True, forces=bf, force_moments=True,
                                                                      wall_moments=True, force_spectrum=gfd.Spectrum([0, 1, 2, 4, 8]))
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
    res = {"headline_ms": {k: sorted(v) for k, v in ht.items()}}
    if len(runs) > 1:
        res["results_equal"] = all(torch.equal(runs["forces off"].result(), ro.result()) for ro in runs.values())
        print(f"  results equal with the forces on and off: {res['results_equal']}")
        for name, ro in runs.items():
            if ro._forces is not None:
                print(f"  {name}: {ro.forces()}")
    print("JSON " + json.dumps(res))
