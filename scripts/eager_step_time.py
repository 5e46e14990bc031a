"""Host-bound eager step: ms per step of `Rollout(capture=False)` on the 12.5k-node mesh of scripts/dist_check.py's host-bound leg
(NsThreeScaleGNN, hidden 128, three levels) — every launch of the step is issued from Python, so this is what a change to the host
path (nn/blocks.py, the models) can slow down while the captured headline stays where it is.
Usage: python scripts/eager_step_time.py [--root DIR] [--nodes 12500] [--steps 300] [--warmup 20]
`--root`: the tree whose package is timed (default: this one) — for interleaved rounds against another checkout."""
import argparse, os, sys, time
ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--nodes", type=int, default=12500); ap.add_argument("--steps", type=int, default=300); ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--label", default="")
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.root))
import torch
import graphs4cfd_amd as gfd
from graphs4cfd_amd import synthetic as S
from graphs4cfd_amd.nn.rollout import Rollout

dev = torch.device("cuda", 0)
torch.manual_seed(0)
model = gfd.nn.NsThreeScaleGNN(arch=S.mus_arch("NsThreeScaleGNN", 128), device=dev)
g = S.mus_graph(a.nodes, levels=3, seed=1).to(dev)
with torch.no_grad(), Rollout(model, g, a.warmup + a.steps, capture=False) as ro:
    for _ in range(a.warmup):
        ro.step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        ro.step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / a.steps * 1e3
print(f"eager {a.label or os.path.basename(os.path.abspath(a.root))}: Rollout(capture=False) NsThreeScaleGNN {a.nodes} nodes: {ms:.3f} ms/step over {a.steps} steps")
