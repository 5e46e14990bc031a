"""Device time of the quadratic-fit operator (gfd.MeshJet, csrc/mesh_jet.hip) on a 100k-node 2-D mesh with its own k = 12 stencil and the
fields u, v, p: the weights build (g4c_mesh_jet_weights, once per mesh), `derived` with ResidualLoss's eight columns (grad u, grad v,
grad p, lap u, lap v) and its adjoint — each against the bytes the algorithm has to move once, over 8 TB/s — and the only way the
same quantities could be had before: two g4c_mesh_derived launches on the graph's k = 6 edges (the three gradients, then the
divergence of the two velocity gradients).  That alternative computes something less accurate (its Laplacian does not converge), so
its ratio is a record, not a pass mark.  Every per-call variant is a hipGraph of LAUNCHES consecutive calls timed with device events,
the variants alternated REPS times; median (min - max).  Results: tests/JET_MEASURED.md."""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

import torch

ap = argparse.ArgumentParser()
ap.add_argument("--nodes", type=int, default=100_000)
ap.add_argument("--k", type=int, default=12)
ap.add_argument("--short", action="store_true", help="few launches")
a = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import graphs4cfd_amd as gfd                                   # noqa: E402
from graphs4cfd_amd import ops, synthetic as S                 # noqa: E402

DEV = torch.device("cuda", 0)
N, K, NF, PEAK = a.nodes, a.k, 3, 8e12
NAMES = ("grad:0", "grad:1", "grad:2", "lap:0", "lap:1")
LAUNCHES, REPS = (10, 3) if a.short else (50, 10)
gen = torch.Generator().manual_seed(0)
graph = S.mus_graph(N, levels=1, dim=2, seed=0, device=DEV)          # bench.py's kind of mesh: kNN, k = 6
x = torch.randn(N, NF, generator=gen).to(DEV)

jet = gfd.MeshJet(graph, k=K)
prog = jet.program(NAMES, NF)
nd, S_ = int(prog.nd), int(jet.src.numel())
out, gy, gx = torch.empty(N, nd, device=DEV), torch.randn(N, nd, generator=gen).to(DEV), torch.empty(N, NF, device=DEV)
out_off, out_c, out_dst = jet._sender_side()
# the stencil as the weights launch takes it
pos = graph.pos.float()
rel = (pos.repeat_interleave(K, dim=0) - pos[jet.src.long()]).contiguous()
csr = SimpleNamespace(off=jet.off, perm=None, n=S_)
w_out = (torch.empty_like(jet.c), torch.empty_like(jet.src), torch.empty(N, dtype=torch.uint8, device=DEV))

grad = gfd.MeshGradient(graph)
E = int(grad.src.numel())
p1 = grad.program(("grad:0", "grad:1", "grad:2"), NF)
p2 = ops.derived_program([[(0, 0, 1.0), (1, 1, 1.0)], [(2, 0, 1.0), (3, 1, 1.0)]], 6, 2)          # lap u, lap v as divergences of the gradients
g1, g2 = torch.empty(N, 6, device=DEV), torch.empty(N, 2, device=DEV)
# the sender side of the alternative's adjoint
a_off, a_g, a_dst = grad._sender_side()
gx2, gx1 = torch.empty(N, 6, device=DEV), torch.empty(N, NF, device=DEV)


def alt_forward():
    ops.mesh_derived(x, grad.off, grad.g, grad.src, p1, g1)
    ops.mesh_derived(g1, grad.off, grad.g, grad.src, p2, g2)


def alt_adjoint():
    ops.mesh_derived_adjoint(g2, grad.off, grad.g, a_off, a_g, a_dst, p2, 6, gx2)
    ops.mesh_derived_adjoint(gx2, grad.off, grad.g, a_off, a_g, a_dst, p1, NF, gx1)


VARIANTS = {
    "weights build": (lambda: ops.mesh_jet_weights(rel, csr, jet.src, 2, out=w_out),
                      4 * (S_ * 2 + S_ + (N + 1) + S_ * 5 + S_) + N),
    "derived, 8 columns": (lambda: ops.mesh_jet(x, jet.off, jet.c, jet.src, prog, out),
                           4 * (N * NF + S_ * 5 + S_ + (N + 1) + N * nd)),
    "adjoint, 8 columns": (lambda: ops.mesh_jet_adjoint(gy, jet.off, jet.c, out_off, out_c, out_dst, prog, NF, gx),
                           4 * (N * nd + 2 * S_ * 5 + S_ + 2 * (N + 1) + N * NF)),
    "alternative: two mesh_derived launches (k = 6)": (alt_forward, 4 * (N * NF + 2 * (E * 2 + E + (N + 1)) + 2 * N * 6 + N * 2)),
    "alternative: their two adjoints": (alt_adjoint, 4 * (N * 2 + 2 * (2 * E * 2 + E + 2 * (N + 1)) + 2 * N * 6 + N * NF)),
}
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
times = {name: [] for name in VARIANTS}
for _ in range(REPS):
    for name, gr in graphs.items():          # alternated
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        gr.replay()
        t1.record()
        torch.cuda.synchronize(DEV)
        times[name].append(1e3 * t0.elapsed_time(t1) / LAUNCHES)          # microseconds per call
res = {"workload": f"MeshJet on a {N}-node 2-D mesh, k = {K}, fields u, v, p; {S_} stencil entries, table {S_ * 20 / 1e6:.1f} MB",
       "launches_per_graph": LAUNCHES, "reps": REPS, "degenerate_nodes": int(jet.degenerate.sum())}
for name, ts in times.items():
    med, nbytes = statistics.median(ts), VARIANTS[name][1]
    res[name] = {"us_median": round(med, 2), "us_min": round(min(ts), 2), "us_max": round(max(ts), 2), "algorithm_MB": round(nbytes / 1e6, 2),
                 "TB_per_s": round(nbytes / med / 1e6, 3), "share_of_8_TB_per_s": round(nbytes / med * 1e6 / PEAK, 3)}
res["derived / alternative forward"] = round(res["derived, 8 columns"]["us_median"] / res["alternative: two mesh_derived launches (k = 6)"]["us_median"], 3)
res["adjoint / alternative adjoints"] = round(res["adjoint, 8 columns"]["us_median"] / res["alternative: their two adjoints"]["us_median"], 3)
print(json.dumps(res))
