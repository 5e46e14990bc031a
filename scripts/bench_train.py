"""Training-step throughput of the autograd path: forward + GraphLoss + backward + Adam step of a
MuS-GNN on a synthetic mesh, on the GPU (fused forward, recompute backward: autograd.py) and — on a bounded sample — with
the oracle on the host cores (torch autograd over the op-for-op restatement = what the reference's fit() executes).
Usage: python scripts/bench_train.py [--nodes 100000] [--model NsThreeScaleGNN] [--steps 10] [--cpu-steps 1] [--phases] [--mixed [--saved-bf16]]
       [--flow-loss | --sample-loss | --force-loss | --residual-loss | --integral-loss]
--flow-loss: the same run with FlowLoss(0.25, terms={"div": 0.1, "vort": 0.05}) on the GPU (a continuity penalty and a vorticity-matching
term through the differentiable mesh gradient: two `derived` launches and their adjoints per step; the host-side sample keeps GraphLoss).
--sample-loss: the same run with SampleLoss(a 128 × 64 raster over the wake window [0.5, 1] × [0.25, 0.75], 0.25, weight=1.0): GraphLoss plus
the error at 8 192 points that are no nodes, through the differentiable point sampler: one `sample` launch and its adjoint per step.
--force-loss: the same run with ForceLoss(0.25, weight=1.0, mu=1e-3, wall={"pressure": 0.5, "shear": 0.5}, nodes="wall") on a loop of 256 nodes
picked from the mesh — nearest to a circle of radius 0.1 round (0.5, 0.5): the synthetic mesh has no `bound` —: GraphLoss plus the error of drag,
lift and the wall loads through the differentiable body forces: a `forces` and a `wall` launch on the prediction and on the target and the two
adjoints per step.
--residual-loss: the same run with ResidualLoss(0.25, weight=1e-3, nu=1e-3, dt=0.1): GraphLoss plus the momentum and continuity residuals
through the differentiable quadratic-fit operator (gfd.MeshJet, its own k = 12 stencil): a `derived` launch of eight columns on the prediction and
on the target and one adjoint per step.
--integral-loss: the same run with IntegralLoss(0.25, terms={"mse": 1.0, "rel_mse": 0.1, "ke": 1.0, "enstrophy": 0.01}): GraphLoss plus the
area-weighted errors through the differentiable control-volume integrals (gfd.ControlVolumes): four `integrate` launches on the prediction and
the target, a `derived` launch on each, and the adjoints of the prediction's three per step; "loss_ms" is the loss alone (its forward and backward on a leaf that stands for the
prediction, device events; "graph_loss_ms" the same of GraphLoss(0.25)) and "operators_build_ms" what a fresh batch pays once (the control
volumes and the mesh gradient).
--mixed: the same step in mixed precision (what fit(mixed_precision=True) selects: every matrix product on bf16-rounded operands).
--saved-bf16 (with --mixed): the rows the forward keeps for the backward as bf16 (TrainConfig(saved_activations="bf16"))."""
import argparse, json, os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import graphs4cfd_amd as gfd
from graphs4cfd_amd import synthetic as S

ap = argparse.ArgumentParser()
ap.add_argument("--nodes", type=int, default=100_000)
ap.add_argument("--model", default="NsThreeScaleGNN", help="a MuS-GNN class, NsThreeGuillardScaleGNN (gMuS) or NsRotEquiTreeScaleGNN (REMuS)")
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--cpu-steps", type=int, default=1)
ap.add_argument("--phases", action="store_true", help="HIP-event time per phase of the backward pass (one extra step)")
ap.add_argument("--mixed", action="store_true", help="mixed-precision training: set_mlp_precision('bf16') + set_train_precision('bf16')")
ap.add_argument("--saved-bf16", action="store_true", help="with --mixed: saved activations as bf16 (set_train_precision('bf16', saved='bf16'))")
ap.add_argument("--flow-loss", action="store_true", help="FlowLoss(0.25, terms={'div': 0.1, 'vort': 0.05}) instead of GraphLoss(0.25) on the GPU")
ap.add_argument("--sample-loss", action="store_true", help="SampleLoss(a 128 x 64 raster over the wake window, 0.25) instead of GraphLoss(0.25) on the GPU")
ap.add_argument("--force-loss", action="store_true", help="ForceLoss(0.25, mu=1e-3, wall=...) on a loop of 256 nodes instead of GraphLoss(0.25) on the GPU")
ap.add_argument("--residual-loss", action="store_true", help="ResidualLoss(0.25, weight=1e-3, nu=1e-3, dt=0.1) instead of GraphLoss(0.25) on the GPU")
ap.add_argument("--integral-loss", action="store_true", help="IntegralLoss(0.25, terms={'mse', 'rel_mse', 'ke', 'enstrophy'}) instead of GraphLoss(0.25) on the GPU")
a = ap.parse_args()
if a.flow_loss + a.sample_loss + a.force_loss + a.residual_loss + a.integral_loss > 1:
    ap.error("--flow-loss, --sample-loss, --force-loss, --residual-loss and --integral-loss are separate runs")
if a.saved_bf16 and not a.mixed:
    ap.error("--saved-bf16 needs --mixed")
if a.mixed:
    gfd.ops.set_mlp_precision("bf16")
    gfd.ops.set_train_precision("bf16", saved="bf16" if a.saved_bf16 else None)
dev = torch.device("cuda", 0)
nf = 3
if a.model == "NsRotEquiTreeScaleGNN":
    g_cpu, arch, nf = S.remus_graph(a.nodes, k=5, seed=0), S.remus_arch(128), 2
elif "Guillard" in a.model:
    g_cpu, arch = S.mugs_graph(a.nodes, levels={"Two": 2, "Three": 3, "Four": 4}[a.model[2:].split("Guillard")[0]], seed=0), S.mugs_arch(a.model, 128)
else:
    levels = {"NsOneScaleGNN": 1, "NsTwoScaleGNN": 2, "NsThreeScaleGNN": 3, "NsFourScaleGNN": 4}[a.model]
    g_cpu, arch = S.mus_graph(a.nodes, levels=levels, seed=0), S.mus_arch(a.model, 128)
g_cpu.target = torch.randn(a.nodes, nf)
torch.manual_seed(0)
model = getattr(gfd.nn, a.model)(arch=arch, device=dev)
g = g_cpu.clone().to(dev)
if a.sample_loss:
    ax, ay = torch.linspace(0.5, 1.0, 128), torch.linspace(0.25, 0.75, 64)
    crit = gfd.nn.SampleLoss(torch.stack(torch.meshgrid(ax, ay, indexing="ij"), -1).reshape(-1, 2), 0.25, weight=1.0)
elif a.force_loss:
    pos = g.pos.double()
    ring = torch.argsort(((pos[:, 0] - 0.5).hypot(pos[:, 1] - 0.5) - 0.1).abs())[:256]          # BodyForces orders them by angle
    g.wall = torch.zeros(a.nodes, dtype=torch.bool, device=dev)
    g.wall[ring] = True
    crit = gfd.nn.ForceLoss(0.25, weight=1.0, mu=1e-3, wall={"pressure": 0.5, "shear": 0.5}, nodes="wall")
elif a.residual_loss:
    crit = gfd.nn.ResidualLoss(0.25, weight=1e-3, nu=1e-3, dt=0.1)
elif a.integral_loss:
    crit = gfd.nn.IntegralLoss(0.25, terms={"mse": 1.0, "rel_mse": 0.1, "ke": 1.0, "enstrophy": 0.01})
else:
    crit = gfd.nn.FlowLoss(0.25, terms={"div": 0.1, "vort": 0.05}) if a.flow_loss else gfd.nn.GraphLoss(lambda_d=0.25)
opt = torch.optim.Adam(model.parameters(), lr=1e-4, fused=True)        # (as GNN.fit does on the GPU)
model.train()


def step():
    pred = model.forward(g, 0)
    loss = crit(g, pred, g.target)
    loss.backward()
    opt.step()
    opt.zero_grad()
    return loss


for _ in range(2):
    step()
torch.cuda.synchronize()
torch.cuda.reset_peak_memory_stats()
t0 = time.perf_counter()
for _ in range(a.steps):
    loss = step()
torch.cuda.synchronize()
dt = (time.perf_counter() - t0) / a.steps
# forward only (same launches, recorded for autograd) and inference forward for scale
t0 = time.perf_counter()
for _ in range(a.steps):
    pred = None                      # (release the previous graph and the activations it keeps before building the next)
    pred = model.forward(g, 0)
torch.cuda.synchronize()
fwd = (time.perf_counter() - t0) / a.steps
pred = None
with torch.no_grad():
    model.forward(g, 0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        model.forward(g, 0)
    torch.cuda.synchronize()
    inf = (time.perf_counter() - t0) / a.steps
out = {"workload": f"{a.model} H=128 training step (forward + {type(crit).__name__} + backward + Adam) on a {a.nodes}-node synthetic 2D mesh",
       "gpu_ms_per_training_step": 1e3 * dt, "gpu_training_steps_per_s": 1 / dt, "gpu_ms_forward_recorded": 1e3 * fwd,
       "gpu_ms_forward_inference_eager": 1e3 * inf, "gpu_peak_memory_GB": torch.cuda.max_memory_allocated() / 2 ** 30,
       "loss": float(loss), "mlp_precision": gfd.ops.mlp_precision(), "train_precision": gfd.ops.train_precision(),
       "saved_precision": gfd.ops.saved_precision(), "loss_function": type(crit).__name__}
if a.integral_loss:
    # the loss alone: its forward and backward on a leaf that stands for the prediction (device events round `steps` calls), and the build
    # a fresh batch pays once (host wall time, device work included)
    leaf = torch.randn(a.nodes, nf, device=dev, requires_grad=True)
    for fn_name, fn in (("loss_ms", lambda: crit(g, leaf, g.target).backward()),
                        ("graph_loss_ms", lambda: gfd.nn.GraphLoss(lambda_d=0.25)(g, leaf, g.target).backward())):
        fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out[fn_name] = e0.elapsed_time(e1) / a.steps
    builds = []
    for _ in range(3):
        crit._cache = None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        crit.operators(g)
        torch.cuda.synchronize()
        builds.append(1e3 * (time.perf_counter() - t0))
    out["operators_build_ms"] = sorted(builds)[1]
    out["loss_share_of_step"] = out["loss_ms"] / out["gpu_ms_per_training_step"]
if a.phases:
    from graphs4cfd_amd import autograd as A
    A.PROFILE = {}
    t0 = time.perf_counter()
    step()
    ph = A.profile_summary()
    A.PROFILE = None
    out["backward_phases_ms"] = {k: round(v, 2) for k, v in sorted(ph.items(), key=lambda kv: -kv[1])}
    out["backward_phases_total_ms"] = round(sum(ph.values()), 2)
if a.cpu_steps > 0:
    from oracle import g4c_oracle as O
    import torch.nn.functional as F
    w = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in model.state_dict().items()}
    copt = torch.optim.Adam(list(w.values()), lr=1e-4)
    gd = g_cpu.to_dict()
    threads = min(16, os.cpu_count())          # (more threads are slower and erratic on the 2-socket host: profiles/r01_cpu_thread_sweep.log)
    torch.set_num_threads(threads)
    t0 = time.perf_counter()
    fwd = (lambda: O.remus_forward(gd, w)) if a.model == "NsRotEquiTreeScaleGNN" else \
          (lambda: O.mugs_forward(a.model, gd, w, 3)) if "Guillard" in a.model else (lambda: O.mus_forward(a.model, gd, w, 3))
    for _ in range(a.cpu_steps):
        closs = O.graph_loss(gd, fwd(), gd["target"], 0.25)
        closs.backward()
        copt.step()
        copt.zero_grad()
    cdt = (time.perf_counter() - t0) / a.cpu_steps
    out.update({"cpu_ms_per_training_step": 1e3 * cdt, "cpu_cores": threads, "cpu_kind": "port (oracle + torch autograd)",
                "cpu_sample": f"{a.cpu_steps} training step(s) of the same mesh and weights", "gpu_over_cpu": cdt / dt})
print(json.dumps(out))
