"""What the differentiable domain integrals cost (tests/INTEGRAL_LOSS_MEASURED.md): the adjoint launch `g4c_weighted_integrals_adjoint`
against the forward `g4c_weighted_integrals` at the same shape and against the torch expression of the same gradient, and the build a
fresh batch pays once.
Usage: python scripts/bench_integral_loss.py [--nodes 100000] [--tall 4000000] [--reps 200] [--rounds 5]
Two sizes: `--nodes` rows (a training batch: the launch is expected to be launch-latency bound) and `--tall` rows (bandwidth: algorithmic
bytes per row 4 nz read of x, 4 nz of sub, 8 of w, 4 of group, 4 nz written, against 8 TB/s).  nz = 3; programs of 2, 3 and 8 entries; the
program of 3 is the area-weighted MSE's — (f, f) on pred − target — whose gradient torch writes as 2 · g · w[:, None] · (pred − target) in
fp64, cast to float32: the same numbers in an order torch chooses, through an fp64 copy of the fields.  Device events around `reps`
back-to-back calls, the paths alternating round by round; the median and the spread of the rounds, one JSON line per case."""
import argparse, json, os, statistics, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import graphs4cfd_amd as gfd
from graphs4cfd_amd import ops, plan, synthetic as S

ap = argparse.ArgumentParser()
ap.add_argument("--nodes", type=int, default=100_000)
ap.add_argument("--tall", type=int, default=4_000_000)
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--rounds", type=int, default=5)
a = ap.parse_args()
dev = torch.device("cuda", 0)
NZ, G = 3, 4
med = statistics.median
PROGRAMS = {2: [(0, 0), (1, 1)], 3: [(0, 0), (1, 1), (2, 2)], 8: [(0, 0), (1, 1), (2, 2), (0, 1), (1, 2), (0, -1), (-1, 2), (-1, -1)]}


def timed(fn, reps):
    for _ in range(10):
        fn()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return 1e3 * t0.elapsed_time(t1) / reps          # µs per call


for n in (a.nodes, a.tall):
    reps = a.reps if n <= 1_000_000 else max(a.reps // 10, 10)
    gen = torch.Generator().manual_seed(0)
    pred, target = torch.randn((n, NZ), generator=gen).to(dev), torch.randn((n, NZ), generator=gen).to(dev)
    w = torch.rand(n, generator=gen).double().to(dev) / n
    group = torch.repeat_interleave(torch.arange(G, dtype=torch.int32), -(-n // G))[:n].contiguous().to(dev)
    gx = torch.empty((n, NZ), device=dev)
    for ne, entries in PROGRAMS.items():
        prog = ops.integral_program(entries, NZ)
        g = torch.randn((G, ne), generator=gen).double().to(dev)
        stats = torch.zeros((1, ne), dtype=torch.float64, device=dev)
        scratch = ops.weighted_integrals_scratch(n, ne, dev)

        def forward():
            ops.weighted_integrals(pred, w, prog, stats, scratch, sub=target)

        def adjoint():
            ops.weighted_integrals_adjoint(pred, w, prog, g, sub=target, group=group, out=gx)

        def in_torch():
            # the MSE program only: d/d pred of Σ_q Σ_f g[q, f] Σ_{i in q} w_i (pred − target)²
            return (2.0 * g[group.long()] * w[:, None] * (pred.double() - target.double())).float()

        paths = {"forward": forward, "adjoint": adjoint}
        if ne == 3:
            paths["torch"] = in_torch
            adjoint()
            ref = in_torch()
            torch.cuda.synchronize()
            agree = float((gx - ref).abs().max()) / max(float(ref.abs().max()), 1e-300)
        times = {k: [] for k in paths}
        for _ in range(a.rounds):
            for k, fn in paths.items():
                times[k].append(timed(fn, reps))
        bytes_adj = n * (4 * NZ + 4 * NZ + 8 + 4 + 4 * NZ)
        out = {"rows": n, "nz": NZ, "ne": ne, "groups": G, "reps": reps, "rounds": a.rounds}
        for k, v in times.items():
            out[f"{k}_us"], out[f"{k}_us_range"] = med(v), [min(v), max(v)]
        out["adjoint_algorithmic_bytes"] = bytes_adj
        out["adjoint_GBps"] = bytes_adj / med(times["adjoint"]) / 1e3
        out["adjoint_fraction_of_8TBps"] = out["adjoint_GBps"] / 8000.0
        out["adjoint_over_forward"] = med(times["adjoint"]) / med(times["forward"])
        if ne == 3:
            out["adjoint_over_torch"] = med(times["adjoint"]) / med(times["torch"])
            out["torch_vs_adjoint_max_rel_diff"] = agree
        print(json.dumps(out), flush=True)
    del pred, target, w, group, gx

# the build a fresh batch pays once: the control volumes of `--nodes` uniform random points, and the loss's first call on it
g = S.mus_graph(a.nodes, levels=1, seed=0).to(dev)
g.target = torch.randn(a.nodes, NZ, device=dev)
builds = []
for _ in range(a.rounds):
    plan.clear_caches()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cv = gfd.ControlVolumes(g)
    torch.cuda.synchronize()
    builds.append(1e3 * (time.perf_counter() - t0))
crit = gfd.nn.IntegralLoss(node_weight=0.0, terms={"mse": 1.0, "rel_mse": 0.1, "ke": 1.0})
leaf = torch.randn(a.nodes, NZ, device=dev, requires_grad=True)
loss_us = [timed(lambda: crit(g, leaf, g.target).backward(), max(a.reps // 4, 10)) for _ in range(a.rounds)]
print(json.dumps({"nodes": a.nodes, "volumes_build_ms": med(builds), "volumes_build_ms_range": [min(builds), max(builds)],
                  "loss_terms": "mse, rel_mse, ke (three sources forward, two adjoints)", "loss_forward_backward_us": med(loss_us),
                  "loss_forward_backward_us_range": [min(loss_us), max(loss_us)], "builds": crit.builds}), flush=True)
