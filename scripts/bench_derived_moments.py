"""Launch time of g4c_mesh_derived (with its statistics) and g4c_rollout_moments (with and without `sub`) at 100k nodes, nf = 3: each a
hipGraph of LAUNCHES consecutive launches (as they run inside a captured rollout step), timed with device events, the variants
alternated REPS times.  G4C_LIB_PATH names another build's libg4c.so for an A/B of two builds (tests/NONFINITE_MEASURED.md)."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))          # scripts/..
sys.path.insert(0, ROOT)
from graphs4cfd_amd import ops          # noqa: E402

DEV = torch.device("cuda", 0)
N, NF, DIM, DEG = 100_000, 3, 2, 6
LAUNCHES, REPS = 100, 10
gen = torch.Generator().manual_seed(0)
rng = np.random.default_rng(0)
x = torch.randn(N, NF, generator=gen).to(DEV)
sub = torch.randn(N, NF * LAUNCHES, generator=gen).to(DEV)
step = torch.zeros(2, dtype=torch.int32, device=DEV)

# a mesh of in-degree 6 given by its tables (senders i +- 1, 2, 3 mod N), random weights
off = torch.arange(0, DEG * N + 1, DEG, dtype=torch.int32, device=DEV)
src = torch.from_numpy(((np.arange(N)[:, None] + np.array([1, 2, 3, N - 1, N - 2, N - 3])[None, :]) % N).reshape(-1).astype(np.int32)).to(DEV)
g = torch.randn(DEG * N, DIM, generator=gen).to(DEV)
prog = [[(0, 0, 1.0), (1, 1, 1.0)], [(1, 0, 1.0), (0, 1, -1.0)]]          # divergence and vorticity
nd = len(prog)
cur = torch.zeros(N, nd, device=DEV)
dstats = torch.zeros(LAUNCHES, nd, 3, dtype=torch.float64, device=DEV)
dscratch = ops.mesh_derived_scratch(N, nd, DEV)

planes = (NF, NF, ops.moment_pairs(NF), NF, NF)
acc = torch.zeros(sum(planes), N, dtype=torch.float64, device=DEV)
window = torch.tensor([0, -1], dtype=torch.int32, device=DEV)


def bump():
    step[0] += 1          # (the step's closing launch does this in a rollout)


VARIANTS = {
    "mesh_derived, div + vort, stats": lambda: (ops.mesh_derived(x, off, g, src, prog, cur, step=step, stats=dstats, scratch=dscratch,
                                                                 max_steps=LAUNCHES, nf=NF), bump()),
    "rollout_moments": lambda: (ops.rollout_moments(x, step, NF, LAUNCHES, window, *acc.split(planes)), bump()),
    "rollout_moments, sub": lambda: (ops.rollout_moments(x, step, NF, LAUNCHES, window, *acc.split(planes), sub=sub), bump()),
    "step index alone": bump,
}
graphs = {}
for name, fn in VARIANTS.items():
    step.zero_()
    fn()
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
print(f"launch time, {N} nodes, nf {NF}: us per call, the step index's bump included (a hipGraph of {LAUNCHES} calls, {REPS} alternated repetitions)")
out = {}
for name, t in times.items():
    t = sorted(t)
    out[name] = dict(median=t[len(t) // 2], min=t[0], max=t[-1])
    print(f"  {name:34s} median {t[len(t) // 2]:7.2f}   min {t[0]:7.2f}   max {t[-1]:7.2f}")
print("JSON " + json.dumps({"launch_us": out}))
