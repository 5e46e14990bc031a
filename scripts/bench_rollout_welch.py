"""The two kernels of g4c_rollout_welch at 100k nodes, nf = 3, K = 8, L = 64, for a `rocprofv3 --kernel-trace --stats` run of its own
(tests/WELCH_MEASURED.md has the command): the call at every step index 0 .. 4 L - 1, so that the trace holds the accumulate kernel on
ordinary steps and the close kernel on the steps that end a segment (the others return at once), and, for the same K on the same box,
g4c_rollout_spectrum over as many steps.  `--hop` 64 (segments side by side) or 32 (half overlapping: two sets per step); `--reference`
none, node (one row for all) or target (a second accumulator, launched first).

--summary FILE reads the kernel trace the run left (CSV) and prints, per kernel, the dispatches, the median duration and — for the close
kernel — the median over the dispatches that closed a segment alone, with the algorithmic bytes of a call as a fraction of 8 TB/s."""
import argparse
import csv
import json
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--hop", type=int, default=64, choices=(64, 32))
ap.add_argument("--reference", default="node", choices=("none", "node", "target"))
ap.add_argument("--summary", default=None, help="a rocprofv3 kernel-trace CSV to summarise instead of running")
a = ap.parse_args()

N, NF, K, L, HBM = 100_000, 3, 8, 64, 8e12
STEPS = 4 * L
SETS = L // a.hop                                                     # segments a sample belongs to
# bytes of a dispatch: per set the pivot read, the sum read and written, re and im read and written, and the sample read ...
ACC_BYTES = (SETS * (3 * NF + 4 * NF * K) * 8 + 4 * NF) * N
# ... and of one that closes a segment: sum, re, im read, pxx read and written; with a reference cxr_re, cxr_im read and written (the
# reference's own sums: one row for a node, a second set of planes for the target — whose own, shorter closing dispatches are left out)
CLOSE_BYTES = ((NF + 4 * NF * K) * 8 + (4 * NF * K * 8 if a.reference != "none" else 0) + ((NF + 2 * NF * K) * 8 if a.reference == "target" else 0)) * N
SPEC_BYTES = ((3 * NF + 4 * NF * K) * 8 + 4 * NF) * N

if a.summary:
    rows = list(csv.DictReader(open(a.summary)))
    by = {}
    for r in rows:
        by.setdefault(r["Kernel_Name"], []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3)
    out = {}
    for name, t in by.items():
        for key, nbytes in (("welch_accumulate", ACC_BYTES), ("welch_close", CLOSE_BYTES), ("rollout_spectrum_kernel", SPEC_BYTES)):
            if key not in name:
                continue
            t = sorted(t)
            if key == "welch_close":                                  # the closing dispatches: far longer than those that return at once
                t = t[-((STEPS - L) // a.hop + 1):]
            med = t[len(t) // 2]
            out[key] = dict(dispatches=len(t), median_us=med, min_us=t[0], max_us=t[-1], bytes=nbytes, fraction_of_8TBs=nbytes / (med * 1e-6) / HBM)
            print(f"  {key:26s} {len(t):4d} dispatches   median {med:8.2f} us   min {t[0]:8.2f}   max {t[-1]:8.2f}   {nbytes / 1e6:7.1f} MB   "
                  f"{100 * out[key]['fraction_of_8TBs']:5.1f} % of 8 TB/s")
    print("JSON " + json.dumps({"hop": a.hop, "reference": a.reference, "kernels": out}))
    sys.exit(0)

import torch                                                          # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from graphs4cfd_amd import ops                                        # noqa: E402

DEV = torch.device("cuda", 0)
g = torch.Generator().manual_seed(0)
pred = torch.randn(N, NF, generator=g).to(DEV)
target = torch.randn(N, NF * STEPS, generator=g).to(DEV) if a.reference == "target" else None
tw, w, _ = ops.spectrum_table(bins=list(range(K)), samples=L, taper="hann")
tw_dev, W_dev = tw.to(DEV), ops.welch_weights(tw).to(DEV)


def accumulator(reference):
    planes = torch.zeros(ops.welch_planes(NF, K, reference), N, dtype=torch.float64, device=DEV).split(ops.welch_split(NF, K, reference))
    return torch.tensor([0, -1, 0], dtype=torch.int32, device=DEV), planes


step = torch.zeros(2, dtype=torch.int32, device=DEV)
win, acc = accumulator(a.reference != "none")
twin, tacc = accumulator(False) if target is not None else (None, None)
spec = torch.zeros(ops.spectrum_planes(NF, K), N, dtype=torch.float64, device=DEV).split((NF, NF, NF * K, NF * K))
swin = torch.tensor([0, -1], dtype=torch.int32, device=DEV)
stw = ops.spectrum_table(bins=list(range(K)), samples=STEPS, taper="hann")[0].to(DEV)
for t in range(STEPS):
    step[:1].fill_(t)
    if target is not None:
        ops.rollout_welch(target, step, NF, STEPS, twin, tw_dev, W_dev, *tacc, hop=a.hop, x_step=NF)
        ops.rollout_welch(pred, step, NF, STEPS, win, tw_dev, W_dev, *acc[:5], hop=a.hop, cxr=acc[5:], ref=tacc[1:4])
    elif a.reference == "node":
        ops.rollout_welch(pred, step, NF, STEPS, win, tw_dev, W_dev, *acc[:5], hop=a.hop, cxr=acc[5:], ref_row=N // 2, ref_field=1)
    else:
        ops.rollout_welch(pred, step, NF, STEPS, win, tw_dev, W_dev, *acc, hop=a.hop)
    ops.rollout_spectrum(pred, step, NF, STEPS, swin, stw, *spec)
torch.cuda.synchronize(DEV)
closed = (STEPS - L) // a.hop + 1
assert win.tolist() == [0, STEPS - 1, closed] and swin.tolist() == [0, STEPS - 1], (win.tolist(), swin.tolist())
print(json.dumps({"nodes": N, "nf": NF, "K": K, "L": L, "hop": a.hop, "reference": a.reference, "steps": STEPS, "closed": closed,
                  "bytes": {"accumulate": ACC_BYTES, "close": CLOSE_BYTES, "spectrum": SPEC_BYTES}}))
