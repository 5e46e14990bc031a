"""Launch time of g4c_rollout_advance_record against g4c_rollout_advance (this build's and, with --parent-lib, another build's), 100k
nodes, nf = 3, and the captured headline step with the records on and off (profiles/r13_rollout_record_times.log; --short under
`rocprofv3 --kernel-trace --stats` gave profiles/r13_rollout_record_kernel_stats.csv).  Every variant is a hipGraph of LAUNCHES consecutive launches
(as a step's last launch runs inside a captured rollout), timed with device events, the variants alternated REPS times."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))          # scripts/..
sys.path.insert(0, ROOT)
from graphs4cfd_amd import _lib, ops, synthetic as S          # noqa: E402
import graphs4cfd_amd as gfd                                  # noqa: E402
from graphs4cfd_amd.nn.model import Rollout                    # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--short", action="store_true", help="few launches, no headline part (for a kernel trace)")
ap.add_argument("--no-headline", action="store_true")
ap.add_argument("--parent-lib", default=None, help="libg4c.so of the parent commit: its g4c_rollout_advance is timed beside this build's")
a = ap.parse_args()
DEV = torch.device("cuda", 0)
N, NF, COLS = 100_000, 3, 3
LAUNCHES, REPS = (20, 2) if a.short else (100, 10)
g = torch.Generator().manual_seed(0)
pred = torch.randn(N, NF, generator=g).to(DEV)
field = torch.randn(N, COLS, generator=g).to(DEV)
target = torch.randn(N, NF * LAUNCHES, generator=g).to(DEV)
mask = (torch.rand(N, generator=g) < 0.1).to(DEV)
rows = torch.randint(0, N, (1000,), generator=g).to(torch.int32).to(DEV)
outputs = torch.zeros(LAUNCHES, N, NF, device=DEV)
snap = torch.zeros(LAUNCHES, N, NF, device=DEV)
probe_out = torch.zeros(LAUNCHES, 1000, NF, device=DEV)
stats = torch.zeros(LAUNCHES, NF, _lib.REC_NSTAT, dtype=torch.float64, device=DEV)
scratch = ops.rollout_record_scratch(N, NF, DEV)
step = torch.zeros(2, dtype=torch.int32, device=DEV)

parent = C.CDLL(a.parent_lib) if a.parent_lib else None
if parent is not None:
    parent.g4c_rollout_advance.restype = C.c_int
    parent.g4c_rollout_advance.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]


def plain_parent():
    rc = parent.g4c_rollout_advance(field.data_ptr(), COLS, pred.data_ptr(), NF, outputs.data_ptr(), 0, step.data_ptr(), N,
                                    torch.cuda.current_stream(DEV).cuda_stream)
    assert rc == 0


VARIANTS = {
    "plain (parent library)": plain_parent,
    "plain (this library)": lambda: ops.rollout_advance(field, pred, outputs, step, NF),
    "(a) record, every=1": lambda: ops.rollout_advance_record(field, pred, step, NF, LAUNCHES, snap=snap, every=1),
    "(b) = (a) + target + mask": lambda: ops.rollout_advance_record(field, pred, step, NF, LAUNCHES, snap=snap, every=1, target=target,
                                                                  mask=mask, stats=stats, scratch=scratch),
    "(c) = (b) + 1000 probes": lambda: ops.rollout_advance_record(field, pred, step, NF, LAUNCHES, snap=snap, every=1, target=target,
                                                                mask=mask, stats=stats, scratch=scratch, probe_rows=rows,
                                                                probe_out=probe_out),
    "statistics only, every=0": lambda: ops.rollout_advance_record(field, pred, step, NF, LAUNCHES, target=target, mask=mask, stats=stats,
                                                                 scratch=scratch),
}
if parent is None:
    del VARIANTS["plain (parent library)"]
graphs = {}
for name, fn in VARIANTS.items():
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
print(f"launch time, {N} nodes, nf {NF}, field_cols {COLS}: us per call (a hipGraph of {LAUNCHES} calls, {REPS} alternated repetitions)")
out = {}
for name, t in times.items():
    t = sorted(t)
    out[name] = dict(median=t[len(t) // 2], min=t[0], max=t[-1])
    print(f"  {name:32s} median {t[len(t) // 2]:7.2f}   min {t[0]:7.2f}   max {t[-1]:7.2f}")
print("JSON " + json.dumps({"launch_us": out}))

if not (a.short or a.no_headline):
    # the captured headline step (bench.py: NsThreeScaleGNN, 100k nodes, 2-D, f16x3) with (b) on and off
    K, WARM = 100, 5
    graph = S.mus_graph(100_000, levels=3, dim=2, seed=0, device=DEV)
    graph.batch = torch.zeros(graph.num_nodes, dtype=torch.long, device=DEV)
    torch.manual_seed(0)
    model = gfd.nn.NsThreeScaleGNN(arch=S.mus_arch("NsThreeScaleGNN", 128), device=DEV)
    model.eval()
    steps = K + WARM + 4
    tgt = torch.randn(graph.num_nodes, 3 * steps, generator=g).to(DEV)
    msk = graph.omega[:, 0] == 1
    runs = {"records off": Rollout(model, graph.clone(), steps, capture=True),
            "records on: every=1, target, mask": Rollout(model, graph.clone(), steps, capture=True, every=1, target=tgt, mask=msk)}
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
    print(f"captured headline step (NsThreeScaleGNN, 100k nodes, f16x3), ms per step over {K} replays, 6 alternated repetitions")
    for name, t in ht.items():
        t = sorted(t)
        print(f"  {name:36s} median {t[len(t) // 2]:8.4f}   min {t[0]:8.4f}   max {t[-1]:8.4f}")
    e = runs["records on: every=1, target, mask"].errors()
    same = torch.equal(runs["records off"].result(), runs["records on: every=1, target, mask"].result())
    print(f"  results equal with records on and off: {same}; mse of the last step {e.mse[-1].tolist()}")
    print("JSON " + json.dumps({"headline_ms": {k: sorted(v) for k, v in ht.items()}, "results_equal": same}))
