"""What the differentiable body forces cost (tests/FORCE_LOSS_MEASURED.md): the adjoint `g4c_body_forces_adjoint` (its two launches)
against the forward `g4c_body_forces` on the same wall, and against the composition of the launches that existed before it — the
staged rows H scattered into a zero [N, 4] tensor, `MeshGradient.adjoint` on it, and an indexed add of cp into the pressure column —
at the same bits.
Usage: python scripts/bench_force_loss.py [--reps 200] [--rounds 5]
scripts/bench_body_forces.py's cloud: 100k nodes, k = 6, nf = 3, one circular body whose wall holds 256 and 4 096 items, pressure-only
and viscous.  Device events around `reps` back-to-back calls, the paths alternating round by round; the median and the spread of the
rounds are printed as one JSON line per case — once as eager calls (what a training step pays: the host's share included) and once as a
hipGraph of `--launches` consecutive calls (the device's share alone, as scripts/bench_body_forces.py measures the forward)."""
import argparse, json, math, os, statistics, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import graphs4cfd_amd as gfd
from graphs4cfd_amd import ops, plan, synthetic as S

ap = argparse.ArgumentParser()
ap.add_argument("--nodes", type=int, default=100_000)
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--launches", type=int, default=50, help="calls per captured graph")
a = ap.parse_args()
dev = torch.device("cuda", 0)
N, NF, KNN = a.nodes, 3, 6
MU, SCALE, SHIFT = 1e-3, [1.0, 1.0, 2.0], [0.0, 0.0, 0.5]
med = statistics.median
gen = torch.Generator().manual_seed(0)
x = torch.randn(N, NF, generator=gen).to(dev)


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


def captured(fn):
    """A hipGraph of a.launches consecutive calls on one stream."""
    fn()
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        for _ in range(a.launches):
            fn()
    gr.replay()
    torch.cuda.synchronize()
    return gr


def replayed(gr):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    gr.replay()
    t1.record()
    t1.synchronize()
    return 1e3 * t0.elapsed_time(t1) / a.launches


for w in (256, 4096):
    th = 2 * math.pi * (torch.arange(w, dtype=torch.float64) + 0.25) / w
    wall = torch.stack([0.5 + 0.1 * th.cos(), 0.5 + 0.1 * th.sin()], 1).float()
    rest = torch.rand(2 * N, 2, generator=gen)
    rest = rest[((rest[:, 0] - 0.5).hypot(rest[:, 1] - 0.5) > 0.1 + 0.5 / math.sqrt(N))][:N - w]
    g = gfd.Graph(pos=torch.cat([wall, rest]).to(dev))
    g.edge_index, _ = S.connect_knn(g.pos, KNN)
    mg = gfd.MeshGradient(g)
    for mu in (0.0, MU):
        bf = gfd.BodyForces(g, torch.arange(w), mu=mu, scale=SCALE, shift=SHIFT, gradient=mg if mu else None)
        plan.clear_caches()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tabs = bf._node_side()
        torch.cuda.synchronize()
        build_ms = 1e3 * (time.perf_counter() - t0)
        gF = torch.randn(1, 6, generator=gen, dtype=torch.float64).to(dev)
        gw = torch.randn(w, 2, generator=gen).to(dev)
        cur, wl = torch.zeros(1, 3, device=dev), torch.zeros(w, 2, device=dev)
        stats = torch.zeros(1, 1, 6, dtype=torch.float64, device=dev)
        kw = dict(bf.constants(), off=mg.off if mu else None, g=mg.g if mu else None, src=mg.src if mu else None, max_steps=1)
        hw, gx = torch.empty(w, 5, device=dev), torch.empty(N, NF, device=dev)
        dense, gx2 = torch.zeros(N, 4, device=dev), torch.empty(N, NF, device=dev)

        def forward():
            ops.body_forces(x, bf._item32, bf.body_offsets, bf.area, bf.unit, bf.arm, cur, wall=wl, stats=stats, **kw)

        def adjoint():
            bf._adjoint(gF, gw, NF, out=gx, hw=hw)

        def composed():
            # what the launches before this one allow, given the staged rows: H into a zero [N, 4] tensor, the mesh adjoint of it (every
            # node walks all its out-edges, wall or not), an indexed add of cp; without the viscous part only the last
            gx2.zero_()
            if mu:
                dense.zero_()
                dense[bf.items] = hw[:, :4]
                gx2.copy_(mg.adjoint(dense, ("grad:0", "grad:1"), NF))
            gx2[:, 2].index_add_(0, bf.items, hw[:, 4])

        adjoint(), composed()
        torch.cuda.synchronize()
        same = bool(torch.equal(gx.view(torch.int32), gx2.view(torch.int32)))
        fwd, adj, com = [], [], []
        for _ in range(a.rounds):
            fwd.append(timed(forward))
            adj.append(timed(adjoint))
            com.append(timed(composed))
        graphs = [captured(f) for f in (forward, adjoint, composed)]
        dfwd, dadj, dcom = [], [], []
        for _ in range(2 * a.rounds):
            dfwd.append(replayed(graphs[0]))
            dadj.append(replayed(graphs[1]))
            dcom.append(replayed(graphs[2]))
        q = int(tabs["in_item"].numel()) if mu else 0
        print(json.dumps({"wall_items": w, "viscous": bool(mu), "nodes": N, "nf": NF, "k": KNN, "in_list_entries": q,
                          "nodes_reached": int((gx != 0).any(1).sum()), "forward_us": med(fwd), "forward_us_range": [min(fwd), max(fwd)],
                          "adjoint_us": med(adj), "adjoint_us_range": [min(adj), max(adj)], "composed_us": med(com),
                          "composed_us_range": [min(com), max(com)], "adjoint_over_forward": med(adj) / med(fwd),
                          "adjoint_over_composed": med(adj) / med(com), "composed_has_the_same_bits": same,
                          "captured_forward_us": med(dfwd), "captured_adjoint_us": med(dadj), "captured_adjoint_us_range": [min(dadj), max(dadj)],
                          "captured_composed_us": med(dcom), "captured_composed_us_range": [min(dcom), max(dcom)],
                          "captured_adjoint_over_composed": med(dadj) / med(dcom),
                          "bytes_gx": 4 * N * NF, "adjoint_GBps_of_gx": 4 * N * NF / med(adj) / 1e3, "build_ms_node_side": build_ms}), flush=True)
