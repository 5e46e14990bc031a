"""Launch times of g4c_snapshot_mean / _gram / _combine at N = 100k nodes, nf = 3 (L = 300k), M = 64 and 256 snapshots
(profiles/r22_snapshot_modes_times.log): device events around single launches, the variants alternated REPS times in one visit.

The Gram launch is timed beside what a user had before it: `X.double()` and `torch.matmul(Xd, Xd.T)` — the upcast included, since the
fp64 copy is part of that route — and reported as a fraction of the public fp64 peak (78.6 TFLOP/s vector = matrix on MI355X; the
symmetric form does M (M + 1) / 2 · L multiply-adds on 64 x 64 blocks, the library product M² L).  Combine is reported against a
device copy of the bytes it moves (R = 8 and 16 combinations: the snapshots are read once per block of 8)."""
import argparse
import json
import os
import sys

import torch

ap = argparse.ArgumentParser()
ap.add_argument("--short", action="store_true", help="two repetitions, M = 64 only")
a = ap.parse_args()
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from graphs4cfd_amd import ops, _lib                        # noqa: E402

DEV = torch.device("cuda", 0)
N, NF = 100_000, 3
L = N * NF
MS, REPS = ((64,), 2) if a.short else ((64, 256), 10)
FP64_PEAK = 78.6e12                                        # FLOP/s, AMD's public figure for MI355X (vector and matrix alike)
B = _lib.SNAPSHOT_GRAM_BLOCK
gen = torch.Generator().manual_seed(0)
variants = {}

for M in MS:
    x = (torch.randn(M, N, NF, generator=gen) + 1.0).to(DEV)
    mean = ops.snapshot_mean(x)
    w = (torch.rand(L, generator=gen, dtype=torch.float64) + 0.5).to(DEV)
    G = torch.empty(M, M, dtype=torch.float64, device=DEV)
    scratch = torch.empty(ops.snapshot_gram_scratch_bytes(M, M, L, True) // 8, dtype=torch.float64, device=DEV)
    nb = -(-M // B)
    flops_sym = 2.0 * (nb * (nb + 1) // 2) * B * B * L       # what the launch computes: whole blocks on and below the diagonal
    mean_out = torch.empty(L, dtype=torch.float64, device=DEV)
    variants[f"M {M:3d} mean"] = (lambda x=x, o=mean_out: ops.snapshot_mean(x, out=o), dict(bytes=4.0 * M * L + 8 * L))
    variants[f"M {M:3d} gram, uncentred"] = (lambda x=x, G=G, s=scratch: ops.snapshot_gram(x, out=G, scratch=s), dict(flops=flops_sym))
    variants[f"M {M:3d} gram, centred and weighted"] = (lambda x=x, G=G, s=scratch, m=mean, w=w: ops.snapshot_gram(x, mean_a=m, w=w, out=G, scratch=s),
                                                        dict(flops=flops_sym))

    def library(x=x):
        xd = x.view(x.size(0), -1).double()
        return torch.matmul(xd, xd.t())
    variants[f"M {M:3d} X.double() @ X.double().T (library)"] = (library, dict(flops=2.0 * M * M * L))
    xd_kept = x.view(M, -1).double()
    variants[f"M {M:3d} the library product alone (fp64 copy at hand)"] = (lambda xd=xd_kept: torch.matmul(xd, xd.t()), dict(flops=2.0 * M * M * L))
    for R in (8, 16):
        coef = torch.randn(M, R, generator=gen, dtype=torch.float64).to(DEV)
        out = torch.empty(R, L, dtype=torch.float32, device=DEV)
        variants[f"M {M:3d} combine, R = {R:2d}"] = (lambda x=x, c=coef, m=mean, o=out: ops.snapshot_combine(x, c, mean=m, out=o),
                                                    dict(bytes=4.0 * M * L * (R // 8) + 8 * L * (R // 8) + 4.0 * R * L))
    src = torch.empty(M * L // 2, dtype=torch.float32, device=DEV)
    dst = torch.empty_like(src)
    variants[f"M {M:3d} device copy of {4 * M * L / 1e6:.0f} MB read + written"] = (lambda s=src, d=dst: d.copy_(s), dict(bytes=4.0 * M * L))
    # what the launch is for: the same bits twice, and the library's product within the Gram bound's scale
    G1 = ops.snapshot_gram(x).clone()
    assert torch.equal(G1, ops.snapshot_gram(x)) and torch.equal(G1, G1.t())
    print(f"M {M}: max |G - library| / max |G| = {float((G1 - library()).abs().max() / G1.abs().max()):.3e}; scratch "
          f"{scratch.numel() * 8 / 1e6:.1f} MB")

for fn, _ in variants.values():                            # warm: code objects loaded, the allocator's blocks at hand
    fn()
torch.cuda.synchronize(DEV)
times = {k: [] for k in variants}
for rep in range(REPS):
    for name, (fn, _) in variants.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times[name].append(1e3 * e0.elapsed_time(e1))
print(f"launch time, {N} nodes, nf {NF} (L = {L}): us per call, device events, {REPS} alternated repetitions")
res = {}
for name, t in times.items():
    t = sorted(t)
    med, info = t[len(t) // 2], variants[name][1]
    tail = ""
    if "flops" in info:
        tail = f"   {info['flops'] / (med * 1e-6) / 1e12:6.2f} TFLOP/s   {100 * info['flops'] / (med * 1e-6) / FP64_PEAK:5.1f} % of the fp64 peak"
    if "bytes" in info:
        tail = f"   {info['bytes'] / 1e6:7.1f} MB   {info['bytes'] / (med * 1e-6) / 1e12:5.2f} TB/s"
    res[name] = dict(median=med, min=t[0], max=t[-1], **info)
    print(f"  {name:58s} median {med:9.1f}   min {t[0]:9.1f}   max {t[-1]:9.1f}{tail}")
print("JSON " + json.dumps({"launch_us": res}))
