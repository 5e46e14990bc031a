"""What the differentiable mesh gradient costs (tests/FLOW_LOSS_MEASURED.md): the adjoint launch `g4c_mesh_derived_adjoint` against
the forward `g4c_mesh_derived` at the headline shape, and the operator build a fresh batch pays once.
Usage: python scripts/bench_flow_loss.py [--nodes 100000] [--reps 200] [--rounds 5]
Device events around `reps` back-to-back launches, the two launches alternating round by round; the median and the spread of the
rounds are printed as one JSON line."""
import argparse, json, os, statistics, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import graphs4cfd_amd as gfd
from graphs4cfd_amd import ops, plan, synthetic as S

ap = argparse.ArgumentParser()
ap.add_argument("--nodes", type=int, default=100_000)
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--rounds", type=int, default=5)
a = ap.parse_args()
dev = torch.device("cuda", 0)
NAMES, NF = ("div", "vort"), 3
g = S.mus_graph(a.nodes, levels=1, seed=0).to(dev)
op = gfd.MeshGradient(g)
n, n_e = op.n_nodes, int(op.src.numel())
prog = op.program(NAMES, NF)
nd = int(prog.nd)
x = torch.randn(n, NF, device=dev)
gy = torch.randn(n, nd, device=dev)
cur = torch.empty(n, nd, device=dev)
gx = torch.empty(n, NF, device=dev)
out_off, out_g, out_dst = op._sender_side()


def forward():
    ops.mesh_derived(x, op.off, op.g, op.src, prog, cur)


def adjoint():
    ops.mesh_derived_adjoint(gy, op.off, op.g, out_off, out_g, out_dst, prog, NF, gx)


def timed(fn):
    for _ in range(10):
        fn()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(a.reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return 1e3 * t0.elapsed_time(t1) / a.reps          # µs per launch


fwd, adj = [], []
for _ in range(a.rounds):
    fwd.append(timed(forward))
    adj.append(timed(adjoint))


def build(fresh):
    """Host wall time of one operator build, device work included (a synchronise at both ends): MeshGradient on a batch whose plans
    are not cached, then the sender-side tables of its first adjoint."""
    plan.clear_caches()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    o = gfd.MeshGradient(fresh)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    o._sender_side()
    torch.cuda.synchronize()
    return 1e3 * (t1 - t0), 1e3 * (time.perf_counter() - t1)


builds = [build(g.clone().to(dev)) for _ in range(a.rounds)]
# the bytes either launch needs: the weights, one index per edge and one row of the other side per edge (counted once per node where
# they are re-read from cache), the offsets, its own rows in and out
bytes_fwd = 4 * (n_e * (2 + 1) + n * (NF + nd + 1))
bytes_adj = 4 * (n_e * (2 + 1 + 2) + n * (NF + nd + 2))          # (the weights twice: in sender order, and in CSR order for the diagonal)
med = statistics.median
print(json.dumps({"nodes": n, "edges": n_e, "names": NAMES, "nf": NF,
                  "forward_us": med(fwd), "forward_us_range": [min(fwd), max(fwd)],
                  "adjoint_us": med(adj), "adjoint_us_range": [min(adj), max(adj)], "adjoint_over_forward": med(adj) / med(fwd),
                  "forward_GBps": bytes_fwd / med(fwd) / 1e3, "adjoint_GBps": bytes_adj / med(adj) / 1e3,
                  "build_ms_operator": med([b[0] for b in builds]), "build_ms_sender_side": med([b[1] for b in builds]),
                  "build_ms_range": [min(sum(b) for b in builds), max(sum(b) for b in builds)]}))
