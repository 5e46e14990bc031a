"""What the differentiable point sampler costs (tests/SAMPLE_LOSS_MEASURED.md): the adjoint launch `g4c_sample_points_adjoint` against
the forward `g4c_sample_points` at the same shape and against the composition of the launches that existed before it (expand
coef·gy to [k·P, F], then `segment_reduce` on `plan.gather_csr(idx)`), and the table build a fresh batch pays once.
Usage: python scripts/bench_sample_loss.py [--nodes 100000] [--nf 3] [--k 6] [--reps 200] [--rounds 5]
Three sets of points: a rake of 1 000 points, a 512 × 256 raster over the whole mesh, and the same raster over 1 % of the mesh's area
(every node near it is used by very many points: long lists).  Device events around `reps` back-to-back launches, the three paths
alternating round by round; the median and the spread of the rounds are printed as one JSON line per set."""
import argparse, json, os, statistics, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import graphs4cfd_amd as gfd
from graphs4cfd_amd import _lib, ops, plan, synthetic as S

ap = argparse.ArgumentParser()
ap.add_argument("--nodes", type=int, default=100_000)
ap.add_argument("--nf", type=int, default=3)
ap.add_argument("--k", type=int, default=6)
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--rounds", type=int, default=5)
a = ap.parse_args()
dev = torch.device("cuda", 0)
NF, K = a.nf, a.k
g = S.mus_graph(a.nodes, levels=1, seed=0).to(dev)          # uniform random points in [0, 1]²
n = int(g.pos.size(0))
x = torch.randn(n, NF, device=dev)
med = statistics.median


def timed(fn):
    for _ in range(10):
        fn()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(a.reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return 1e3 * t0.elapsed_time(t1) / a.reps          # µs per call


def build(make):
    """Host wall time of one sampler build, device work included (a synchronise at both ends): the search and the fit on a batch whose
    plans are not cached, then the node-side tables of its first adjoint."""
    plan.clear_caches()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    s = make()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    s._node_side()
    torch.cuda.synchronize()
    return 1e3 * (t1 - t0), 1e3 * (time.perf_counter() - t1)


SETS = {"rake 1000": lambda: gfd.PointSampler.line(g, (0.6, 0.05), (0.6, 0.95), 1000, k=K),
        "raster 512x256, whole mesh": lambda: gfd.PointSampler.grid(g, (512, 256), box=((0.0, 0.0), (1.0, 1.0)), k=K),
        "raster 512x256, 1% of the area": lambda: gfd.PointSampler.grid(g, (512, 256), box=((0.45, 0.45), (0.55, 0.55)), k=K)}
for name, make in SETS.items():
    s = make()
    p = s.n_points
    in_off, in_pt, in_coef = s._node_side()
    gy = torch.randn(p, NF, device=dev)
    cur = torch.empty(p, NF, device=dev)
    gx = torch.empty(n, NF, device=dev)
    csr = plan.gather_csr(s._idx.reshape(-1), n)
    coef_flat = s._coef.reshape(-1, 1)
    gx2 = torch.empty(n, NF, device=dev)

    def forward():
        ops.sample_points(x, s._idx, s._coef, cur)

    def adjoint():
        ops.sample_points_adjoint(gy, in_off, in_pt, in_coef, n, out=gx)

    def composed():
        # what the launches before this one allow: every table entry's contribution as a row of [k·P, F] (slot-major, as the tables),
        # summed per node by the deterministic segmented sum on the gather's CSR plan
        rows = (gy.unsqueeze(0) * coef_flat.view(K, p, 1)).reshape(K * p, NF)
        ops.segment_reduce(rows, csr, False, _lib.ACT_NONE, out=gx2)

    adjoint(), composed()
    torch.cuda.synchronize()
    agree = float((gx - gx2).abs().max()) / max(float(gx.abs().max()), 1e-30)
    fwd, adj, com = [], [], []
    for _ in range(a.rounds):
        fwd.append(timed(forward))
        adj.append(timed(adjoint))
        com.append(timed(composed))
    builds = [build(make) for _ in range(a.rounds)]
    lengths = (in_off[1:] - in_off[:-1]).float()
    # the bytes each path needs: per table entry an index and a coefficient (4 + 4) and one gathered row of the other side (re-read from
    # cache where rows repeat: counted once per row), its own rows out, the offsets; the composition writes and re-reads [k·P, F] and
    # reads the permutation
    e = K * p
    bytes_fwd = 4 * (2 * e + min(e, n) * NF + p * NF)
    bytes_adj = 4 * (2 * e + p * NF + n * NF + n + 1)
    bytes_com = 4 * (e + p * NF + 2 * e * NF + e + n * NF + n + 1)
    print(json.dumps({"points": name, "nodes": n, "n_points": p, "nf": NF, "k": K, "longest_list": int(lengths.max()),
                      "mean_list_of_used_nodes": float(lengths[lengths > 0].mean()), "unused_nodes": int((lengths == 0).sum()),
                      "forward_us": med(fwd), "forward_us_range": [min(fwd), max(fwd)],
                      "adjoint_us": med(adj), "adjoint_us_range": [min(adj), max(adj)],
                      "composed_us": med(com), "composed_us_range": [min(com), max(com)],
                      "adjoint_over_forward": med(adj) / med(fwd), "adjoint_over_composed": med(adj) / med(com),
                      "forward_GBps": bytes_fwd / med(fwd) / 1e3, "adjoint_GBps": bytes_adj / med(adj) / 1e3,
                      "composed_GBps": bytes_com / med(com) / 1e3, "composed_vs_adjoint_max_rel_diff": agree,
                      "build_ms_sampler": med([b[0] for b in builds]), "build_ms_node_side": med([b[1] for b in builds]),
                      "build_ms_range": [min(sum(b) for b in builds), max(sum(b) for b in builds)]}), flush=True)
