"""Drop-in use of the MI355X path with the reference's API: build a mesh with `gfd.transforms`, create (or load) a MuS-GNN,
roll it out with `solve`.  With a trained checkpoint of the reference: `gfd.nn.NsThreeScaleGNN(checkpoint="NsThreeScaleGNN.chk")`.

    python examples/rollout_mus_gnn.py [--nodes 20000] [--steps 50] [--checkpoint file.chk] [--raster vorticity.npy] [--streak streak.npy] [--body 64] [--integrals]
"""
import argparse, os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import graphs4cfd_amd as gfd          # instead of: import graphs4cfd as gfd

ap = argparse.ArgumentParser()
ap.add_argument("--nodes", type=int, default=20000); ap.add_argument("--steps", type=int, default=50)
ap.add_argument("--checkpoint", default=None)
ap.add_argument("--raster", default=None, help="write the vorticity of the last step on a 256 x 256 raster to this .npy file")
ap.add_argument("--streak", default=None, help="write the streaklines of five seeds after the last step to this .npy file")
ap.add_argument("--body", type=int, default=0, help="mark the W nodes nearest to a circle as a wall (bound == 4) and print its force coefficients")
ap.add_argument("--integrals", action="store_true", help="print the kinetic-energy drift and the relative L2 error, weighted by the nodes' Voronoi areas")
ap.add_argument("--welch", action="store_true", help="print the segment-averaged spectrum, the coherence with the ground truth and the frequency drift at a probe")
a = ap.parse_args()
dev = torch.device("cuda")

# a synthetic flow domain: random points, the pre-processing pipeline of examples/training/NsMuSGNN/NsThreeScaleGNN.py
torch.manual_seed(0)
graph = gfd.Graph(pos=torch.rand(a.nodes, 2))
h = 2.0 * a.nodes ** -0.5
graph = gfd.transforms.Compose([
    gfd.transforms.ConnectKNN(6),
    gfd.transforms.ScaleEdgeAttr(h),
    gfd.transforms.GridClustering([2 * h, 4 * h]),
])(graph)
graph.field = torch.randn(a.nodes, 3)                      # u, v, p at the last time step
graph.glob = torch.rand(a.nodes, 1)                        # e.g. the Reynolds number
graph.omega = (torch.rand(a.nodes, 1) > 0.9).float()       # boundary marker
if a.body:                                                 # the reference's NsCircle / NsEllipse records carry `bound` already (4: a wall node)
    ring = torch.argsort(((graph.pos - 0.5).norm(dim=1) - 0.1).abs())[:a.body]
    graph.bound = torch.zeros(a.nodes, dtype=torch.uint8)
    graph.bound[ring] = 4

if a.checkpoint:
    model = gfd.nn.NsThreeScaleGNN(checkpoint=a.checkpoint, device=dev)
else:
    model = gfd.nn.NsThreeScaleGNN(arch=gfd.synthetic.mus_arch("NsThreeScaleGNN", 128), device=dev)   # random weights

model.solve(graph, 3)                                      # builds the static mesh plan, packs the weights, captures the step
torch.cuda.synchronize(); t0 = time.perf_counter()
out = model.solve(graph, a.steps)                          # [N, 3 * steps], device-resident rollout (hipGraph replay)
torch.cuda.synchronize(); dt = time.perf_counter() - t0
print(f"{a.steps} steps on {a.nodes} nodes: {a.steps / dt:.1f} steps/s, output {tuple(out.shape)}, finite={bool(torch.isfinite(out).all())}")
diag = model.diagnostics(graph, a.steps, ("div", "vort"))      # divergence and vorticity of every step, formed on the device: no prediction is held
print("divergence RMS per step:", " ".join(f"{v:.3e}" for v in diag.rms[:, 0].tolist()))
spec = model.spectrum(graph, a.steps, bins=range(a.steps // 2 + 1))     # Fourier modes of u, v, p at every node, accumulated inside the step
print(f"dominant frequency of u: {spec.dominant(0):.4f} cycles per step, largest amplitude there {spec.amplitude[:, 0].max():.3e}")
# the coherent structures of the same rollout: POD of the fluctuation and DMD of the snapshots, from one fp64 Gram matrix formed on the
# device (every second step is kept as a snapshot; pressure is left out of the inner product; dt = 1 per step)
every = 2 if a.steps >= 8 else 1
pod = model.modes(graph, a.steps, every=every, rank=6, field_weights=[1.0, 1.0, 0.0], dt=float(every), dmd=True)
print("POD energy of the first modes:", " ".join(f"{e:.3f}" for e in pod.energy.tolist()), f"({pod.dropped} unresolved of {pod.gram.size(0)})")
try:
    k = pod.dmd.dominant()
    print(f"dominant DMD mode: {float(pod.dmd.frequency[k]):.4f} cycles per step (the spectrum's: {spec.dominant(0):.4f}), "
          f"growth {float(pod.dmd.growth[k]):+.4f} per step, |mu| {float(pod.dmd.eigenvalues[k].abs()):.4f}")
except ValueError:                                          # (no oscillating mode among the first six)
    print("no dynamic mode of the first six oscillates")
if getattr(graph, "bound", None) is not None and bool((graph.bound == 4).any()):      # a body in the flow: its drag, lift and shedding frequency
    D, U, rho, nu = 0.2, 1.0, 1.0, 1e-3
    fo = model.forces(graph, a.steps, mu=rho * nu, discard=a.steps // 4, spectrum=gfd.Spectrum(bins=range(a.steps // 2 + 1)))
    cd, cl, _ = fo.coefficients(rho, U, D)
    print(f"mean Cd {float(cd[a.steps // 4:, 0].mean()):.4f}, r.m.s. Cl {float(cl[a.steps // 4:, 0].std(unbiased=False)):.4f}, St {fo.strouhal(D, U):.4f} (dt = 1)")
if a.integrals:                                             # integrals over the domain, not means over node rows: every node weighs its Voronoi cell
    cells = gfd.ControlVolumes(graph.to(dev), bodies=True if a.body else None)      # built once per mesh; a wall node's cell ends at the wall's tangent
    ig = model.integrals(graph, a.steps, ("volume", "ke", "enstrophy", "div2"), cells)
    print(f"domain area {ig.volume:.4f} over {int((~cells.degenerate).sum())} cells; kinetic-energy drift over {a.steps} steps "
          f"{float(ig.drift('ke')[-1]):+.3e}, enstrophy {float(ig['enstrophy'][-1]):.3e}, ||div||_L2 {float(ig['div2'][-1]) ** 0.5:.3e}")
    graph.target = out                                      # (stands in for the ground truth a dataset carries: the error is then 0)
    print("relative L2 error per step:", " ".join(f"{v:.3e}" for v in model.integrals(graph, a.steps, ("rel_l2",), cells)["rel_l2"].tolist()))
if a.welch:                                                 # spectra with a usable variance: half-overlapping Hann segments, averaged inside the step
    seg = max(2 * (a.steps // 8), 4)                        # (some seven segments: one periodogram has 100 % scatter however long the rollout)
    probe = int(((graph.pos - torch.tensor([0.7, 0.5], device=graph.pos.device)).norm(dim=1)).argmin())
    graph.target = out                                      # (stands in for the ground truth a dataset carries: the coherence is then 1)
    we = model.welch(graph, a.steps, seg, bins=range(seg // 2 + 1), overlap=0.5, reference="target", track=[probe])
    k = int(we.band_power()[0].argmax())
    print(f"Welch PSD of u over {we.segments} segments of {seg} steps: peak at {float(we.freqs[k]):.4f} cycles per step; coherence with the "
          f"target there, median over the nodes: {float(we.coherence[:, 0, k].nanmedian()):.4f}")
    print(f"dominant frequency of u at node {probe}, segment by segment:", " ".join(f"{f:.4f}" for f in we.dominant_by_segment(0, 0).tolist()))
    lag = model.welch(graph, a.steps, seg, bins=range(seg // 2 + 1), overlap=0.5, reference=(probe, 0))      # phase lags behind the probe's u
    print(f"phase lag of u behind node {probe} at that frequency: {float(lag.phase_lag[:, 0, k].min()):+.3f} .. {float(lag.phase_lag[:, 0, k].max()):+.3f} rad")
if a.raster:                                                # the picture of a field: sampled on the device inside the step, no plotting dependency
    import numpy as np
    raster = gfd.PointSampler.grid(graph, (256, 256))          # the mesh's bounding box; .distance masks points far from every node
    rs = model.sample(graph, a.steps, raster, every=a.steps, derived=("vort",))
    np.save(a.raster, rs.image(-1, "vort").cpu().numpy())      # [256, 256]: entry [i, j] is the vorticity at (x_i, y_j)
    print(f"vorticity of step {a.steps - 1} on a 256 x 256 raster -> {a.raster}")
if a.streak:                                                # smoke released at five points: particles carried by (u, v) inside the step
    import numpy as np
    seeds = torch.stack([torch.full((5,), 0.1), torch.linspace(0.3, 0.7, 5)], dim=1)
    smoke = gfd.Tracers.streak(graph.to(dev), seeds, dt=0.2 * h, release_every=2, releases=max(a.steps // 2, 1), max_distance=2 * h)
    rt = model.trace(graph, a.steps, smoke)                    # RolloutTracers: paths, status, stopped; no prediction is held
    line, released = rt.streakline(-1)                         # [5, releases, 2]: each seed's particles, the oldest first
    np.save(a.streak, torch.where(released[:, :, None], line, torch.full_like(line, float("nan"))).cpu().numpy())
    gone = rt.status >= 2                                      # frozen: left the mesh (farther than 2 h from every node)
    stay = f"{rt.residence()[gone].float().mean():.1f} steps in the domain on average" if bool(gone.any()) else "none has left the domain"
    print(f"streaklines of 5 seeds after step {a.steps - 1} -> {a.streak}; {int(gone.sum())} of {gone.numel()} particles stopped, {stay}")
