"""What the periodic searches cost (tests/PERIODIC_MEASURED.md): `g4c_knn_grid_periodic` / `g4c_knn_grid_query_periodic` against
`g4c_knn_grid` / `g4c_knn_grid_query` on the same cloud, and the tracer launch `g4c_tracer_advance_periodic` (Euler and Heun) against
`g4c_tracer_advance`.
Usage: python scripts/bench_periodic.py [--nodes 100000] [--particles 131072] [--reps 50] [--rounds 5]
A uniform random cloud in [0, 1]², one periodic axis (the first, "auto"), k = 6 and 12; the queries are the particles, a rake across the
domain.  The launches alone are timed — the grids are built once, outside —, device events around `reps` back-to-back launches, the two
forms alternating round by round; the median and the spread of the rounds are printed as one JSON line per k."""
import argparse, ctypes as C, json, os, statistics, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from graphs4cfd_amd import _lib, ops, synthetic as S

ap = argparse.ArgumentParser()
ap.add_argument("--nodes", type=int, default=100_000)
ap.add_argument("--particles", type=int, default=131_072)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--rounds", type=int, default=5)
a = ap.parse_args()
dev = torch.device("cuda", 0)
pos = S.mus_graph(a.nodes, levels=1, seed=0).pos.to(dev).float().contiguous()          # uniform random points in [0, 1]²
n, P = int(pos.size(0)), a.particles
rake = torch.stack([torch.full((P,), 0.3), torch.linspace(0.02, 0.98, P)], 1).to(dev)
x0, x1 = torch.randn(n, 3, device=dev) * 0.1, torch.randn(n, 3, device=dev) * 0.1
lib, med, PER = _lib.load(), statistics.median, ["auto", None]
stream = _lib.stream_handle(dev)


def timed(fn):
    for _ in range(5):
        fn()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(a.reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return 1e3 * t0.elapsed_time(t1) / a.reps          # µs per call


for k in (6, 12):
    g, gp = S._bin_cloud(pos, k), S._bin_cloud_periodic(pos, k, PER)
    q_cell = S._cell_ids(rake, g).int()
    out_s, out_q = torch.empty((n, k), dtype=torch.long, device=dev), torch.empty((P, k), dtype=torch.long, device=dev)
    ptr = _lib.ptr
    forms = {
        "self": lambda: _lib.check(lib.g4c_knn_grid(ptr(g["pos_sorted"]), ptr(g["cell_sorted"]), ptr(g["order"]), ptr(g["cell_start"]), n, 2,
                                                    g["nc"], g["org"], C.c_float(g["h"]), k, ptr(out_s), stream)),
        "self_periodic": lambda: _lib.check(lib.g4c_knn_grid_periodic(ptr(gp["pos_sorted"]), ptr(gp["order"]), ptr(gp["cell_start"]), n, 2,
                                                                      C.byref(gp["c_grid"]), k, ptr(out_s), stream)),
        "query": lambda: _lib.check(lib.g4c_knn_grid_query(ptr(g["pos_sorted"]), ptr(g["order"]), ptr(g["cell_start"]), n, 2, g["nc"], g["org"],
                                                           C.c_float(g["h"]), ptr(rake), ptr(q_cell), P, k, ptr(out_q), stream)),
        "query_periodic": lambda: _lib.check(lib.g4c_knn_grid_query_periodic(ptr(gp["pos_sorted"]), ptr(gp["order"]), ptr(gp["cell_start"]), n, 2,
                                                                             C.byref(gp["c_grid"]), ptr(rake), P, k, ptr(out_q), stream)),
    }
    state = dict(status=torch.zeros(P, dtype=torch.uint8, device=dev), stopped=torch.full((P,), -1, dtype=torch.int32, device=dev),
                 release=torch.zeros(P, dtype=torch.int32, device=dev))
    q = rake.clone()

    def tracer(grid, scheme):
        def launch():
            q.copy_(rake)                                # (every launch moves the same particles: the copy is in both forms)
            ops.tracer_advance(grid, x0, x1, q, state["status"], state["stopped"], state["release"], dt=0.01, k=k, scheme=scheme)
        return launch
    for name, scheme in (("euler", _lib.TRACER_EULER), ("heun", _lib.TRACER_HEUN)):
        forms[f"tracer_{name}"], forms[f"tracer_{name}_periodic"] = tracer(g, scheme), tracer(gp, scheme)
    times = {name: [] for name in forms}
    for _ in range(a.rounds):
        for name, fn in forms.items():
            times[name].append(timed(fn))
    line = {"nodes": n, "particles": P, "k": k, "cells": g["n_cells"][:2], "cells_periodic": gp["n_cells"][:2]}
    for name, t in times.items():
        line[name + "_us"], line[name + "_us_range"] = med(t), [min(t), max(t)]
    for name in ("self", "query", "tracer_euler", "tracer_heun"):
        line[name + "_periodic_over_plain"] = med(times[name + "_periodic"]) / med(times[name])
    print(json.dumps(line), flush=True)
