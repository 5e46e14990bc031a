"""Within-process A/B timing of two builds of libg4c.so on the hoisted edge MLP / node MLP (interleaved rounds,
median + min), because run-to-run (box-to-box, DVFS) noise between separate invocations is ~5 %.
Both builds must have this tree's ABI version (g4c_version(): the layout of g4c_mlp_io_t / g4c_mlp_t and the entry points).
Usage: python scripts/ab_test.py libA.so libB.so [--rows 600000] [--rounds 15]"""
import argparse, ctypes as C, os, statistics, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from graphs4cfd_amd import _lib, ops
from graphs4cfd_amd.nn import blocks as B

ap = argparse.ArgumentParser(description="Within-process A/B timing of builds of libg4c.so of the SAME ABI version (g4c_version).")
ap.add_argument("libs", nargs="+", help="builds of libg4c.so with this tree's g4c_version(): other versions are refused")
ap.add_argument("--rows", type=int, default=600000)
ap.add_argument("--rounds", type=int, default=15); ap.add_argument("--inner", type=int, default=3)
ap.add_argument("--precision", default="fp32")
a = ap.parse_args()


def load(path):
    lib = C.CDLL(os.path.abspath(path))
    for name, (res, args) in _lib._SIGNATURES.items():
        fn = getattr(lib, name); fn.restype, fn.argtypes = res, args
    if lib.g4c_version() != _lib.load().g4c_version():
        sys.exit(f"{path}: ABI version {lib.g4c_version()}, this tree's is {_lib.load().g4c_version()}: A/B needs builds of the same version")
    return lib


libs = [load(p) for p in a.libs]
ops.set_mlp_precision(a.precision)
torch.set_grad_enabled(False)
dev = torch.device("cuda", 0); H = 128
torch.manual_seed(0)
_lib._lib = libs[0]
blk = B.GNBlock((3 * H, (H, H, H), True), (2 * H, (H, H, H), True)).to(dev)
rows = a.rows; n = rows // 6
e = torch.randn(rows, H, device=dev); v = torch.randn(n, H, device=dev); agg = torch.randn(n, H, device=dev)
row = torch.randint(0, n, (rows,), device=dev, dtype=torch.int32)
col = (torch.arange(rows, device=dev) // 6).clamp(max=n - 1).to(torch.int32)
pr, pc = torch.randn(n, H, device=dev), torch.randn(n, H, device=dev)
out_e, out_v = torch.empty(rows, H, device=dev), torch.empty(n, H, device=dev)
def pack_for(lib):   # weights are packed by the library that consumes them (the stream layout may differ)
    _lib._lib = lib
    blk.edge_mlp._packed.clear(); blk.node_mlp._packed.clear()
    return blk.edge_mlp._packed_cols(0, H, [H], [False], False), blk.node_mlp.packed([H, H], [False, False])


packs = [pack_for(lib) for lib in libs]
cur = [0]
src_e = [ops.Source(e), ops.Source(pr, index=row, additive=True), ops.Source(pc, index=col, additive=True)]
src_v = [ops.Source(agg), ops.Source(v)]
cases = {"edge(hoisted)": lambda: ops.mlp_forward(packs[cur[0]][0], src_e, rows, 0, out=out_e),
         "node": lambda: ops.mlp_forward(packs[cur[0]][1], src_v, n, 1, out=out_v)}
ref = {}
for cname, fn in cases.items():
    times = [[] for _ in libs]
    for li, lib in enumerate(libs):
        _lib._lib = lib; cur[0] = li; fn(); fn(); torch.cuda.synchronize()
        ref.setdefault(cname, []).append((out_e if cname.startswith("edge") else out_v).clone())
    for r in range(a.rounds):
        for li, lib in enumerate(libs):
            _lib._lib = lib; cur[0] = li
            s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record(); [fn() for _ in range(a.inner)]; t.record(); torch.cuda.synchronize()
            times[li].append(s.elapsed_time(t) / a.inner * 1e3)
    for li, p in enumerate(a.libs):
        d = (ref[cname][li] - ref[cname][0]).abs().max().item()
        print(f"{cname:14s} {os.path.basename(p):28s} median {statistics.median(times[li]):8.1f} us   min {min(times[li]):8.1f} us   max|out - out_A| {d:.1e}")
