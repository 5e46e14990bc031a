"""Derives the bounds of oracle/bf16_ref.py (NOISE) on CPU, from no kernel output: the rounded-bf16 reference evaluated once in fp64
and once with fp32 sums in 32-k steps (the MFMA chain's order and precision, fp32 bias / SELU / LayerNorm), over the launch shapes the
GPU tests use (tests/test_gpu_bf16.py).  The difference is one-ulp flips of hidden bf16 activations plus fp32 round-off — exactly
the freedom a correct kernel has.  Per kind of output it prints the worst case over the shapes of: mean |d|, the fraction of
elements above 1e-2, max |d|, and the largest number of elements in one row above half the max limit.

    python scripts/bf16_noise_bounds.py > profiles/r07_bf16_noise_bounds.log

Deterministic (fixed seeds, one CPU thread): a second run reproduces the log."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import bf16_ref as R          # noqa: E402

H = 128


def mlp_weights(k_in: int, layers: int, ln: bool, seed: int):
    """state_dict of an nn.Linear-initialised MLP (the module's own initialisation: U(-1/sqrt(k), 1/sqrt(k))), LayerNorm with a
    non-trivial gain / shift."""
    g = torch.Generator().manual_seed(seed)
    w, k = {}, k_in
    for i in range(1, layers + 1):
        bound = 1.0 / k ** 0.5
        w[f"MLP.linear_{i}.weight"] = (torch.rand(H, k, generator=g) * 2 - 1) * bound
        w[f"MLP.linear_{i}.bias"] = (torch.rand(H, generator=g) * 2 - 1) * bound
        k = H
    if ln:
        w["MLP.layer_norm.weight"] = 1.0 + 0.1 * torch.randn(H, generator=g)
        w["MLP.layer_norm.bias"] = 0.1 * torch.randn(H, generator=g)
    return w


def memo(f):
    """f(arith) evaluated once per arithmetic (the stored-row / aggregate forms reuse a launch's rows)."""
    seen = {}
    return lambda ar: seen[ar.accum] if ar.accum in seen else seen.setdefault(ar.accum, f(ar))


def cases(n_rows: int = 24000):
    """(name, kind, evaluate(arith) -> tensor) for the launch forms of the GPU tests."""
    out = []
    for layers in (2, 3):
        for ln in (True, False):
            seed = 10 * layers + ln
            g = torch.Generator().manual_seed(seed + 1000)
            # plain launch: [selu(e) | v[row] | v[col]] (tile kernel form)
            n = n_rows // 6
            w = mlp_weights(3 * H, layers, ln, seed)
            e, v = torch.randn(n_rows, H, generator=g), torch.randn(n, H, generator=g)
            row, col = torch.randint(0, n, (n_rows,), generator=g), torch.arange(n).repeat_interleave(6)
            blocks = [R.Block(e, pre_act="selu"), R.Block(v, index=row), R.Block(v, index=col)]
            out.append((f"plain L{layers} ln{int(ln)}", "rows32", lambda ar, w=w, b=blocks: R.mlp(w, b, n_rows, ar=ar)))
            # hoisted launch: x (SELU on load) + two bf16 product rows (given)
            pr = R.products(w["MLP.linear_1.weight"][:, H:2 * H], v)
            pc = R.products(w["MLP.linear_1.weight"][:, 2 * H:], v)
            adds = [R.Additive(pr, row), R.Additive(pc, col)]
            hoisted = memo(lambda ar, w=w, e=e, adds=adds: R.mlp(w, [R.Block(e, pre_act="selu")], n_rows, additive=adds, first_cols=(0, H), ar=ar))
            out.append((f"hoisted L{layers} ln{int(ln)}", "rows32", hoisted))
            out.append((f"hoisted L{layers} ln{int(ln)} bf16 rows", "rows16", lambda ar, f=hoisted: R.stored_rows(f(ar), "bf16")))
            out.append((f"hoisted L{layers} ln{int(ln)} bf16(SELU) rows", "rows16", lambda ar, f=hoisted: R.stored_rows(f(ar), "bf16_selu")))
            for K in (4, 5, 8):
                off = torch.arange(0, n_rows + 1, K)
                out.append((f"hoisted L{layers} ln{int(ln)} mean K{K}", "agg32", lambda ar, f=hoisted, off=off: R.segment_mean(f(ar), off)))
                out.append((f"hoisted L{layers} ln{int(ln)} bf16 mean K{K}", "agg16",
                            lambda ar, f=hoisted, off=off: R.segment_mean(f(ar), off, bf16_out=True)))
    # update-MLP form with heads (rs2 / run_with_heads): [agg | e] bf16 rows -> 2 layers -> LN -> SELU; heads bf16_rne(bf16(W) bf16(y))
    g = torch.Generator().manual_seed(77)
    w = mlp_weights(2 * H, 2, True, 77)
    wn = mlp_weights(3 * H, 2, True, 78)
    a16, e16 = bf16_rows(torch.randn(n_rows, H, generator=g)), bf16_rows(torch.selu(torch.randn(n_rows, H, generator=g)))
    upd = memo(lambda ar, w=w: R.mlp(w, [R.Block(a16), R.Block(e16)], n_rows, act="selu", ar=ar))
    out.append(("update L2 ln1 selu", "rows32", upd))
    out.append(("update L2 ln1 selu bf16 rows", "rows16", lambda ar: R.stored_rows(upd(ar), "bf16")))
    for j in (1, 2):
        Wh = wn["MLP.linear_1.weight"][:, j * H:(j + 1) * H]
        # (a head multiplies the launch's OWN output rows: their noise is part of the head's)
        out.append((f"update head {j}", "prod16", lambda ar, Wh=Wh: R.products(Wh, upd(ar), ar=ar)))
    # a hoisted product of given rows (only the output rounding can flip)
    Wp = wn["MLP.linear_1.weight"][:, H:2 * H]
    out.append(("product of given rows", "prod16", lambda ar: R.products(Wp, a16, ar=ar)))
    # narrow + wide mix (node MLP with a 3-wide narrow block)
    w = mlp_weights(2 * H + 3, 3, True, 91)
    x3 = torch.randn(n_rows, 3, generator=g)
    out.append(("narrow mix L3 ln1 tanh", "rows32",
                lambda ar, w=w: R.mlp(w, [R.Block(e), R.Block(e), R.Block(x3, narrow=True)], n_rows, act="tanh", ar=ar)))
    return out


def bf16_rows(t):
    return R.bf16_rne(t).float()


def derive(n_rows: int = 24000):
    torch.set_num_threads(1)
    worst = {}
    lines = []
    for name, kind, f in cases(n_rows):
        thr, row_thr = R.NOISE[kind][1], R.row_threshold(kind)
        ref, alt = f(R.FP64), f(R.Arith("fp32"))
        s = R.noise_stats(alt, ref, thr, row_thr)
        lines.append(f"{name:40s} {kind:7s} mean {s['mean']:.3e}  frac>{thr:g} {s['frac']:.3e}  max {s['max']:.3e}  "
                     f"row>{row_thr:.3g} {s['row_count']}  ({s['n']} elements)")
        wv = worst.setdefault(kind, dict(mean=0.0, frac=0.0, max=0.0, row_count=0))
        for k in wv:
            wv[k] = max(wv[k], s[k])
    return lines, worst


if __name__ == "__main__":
    lines, worst = derive()
    print("# rounded-bf16 reference: fp32 sums in 32-k steps vs fp64 (scripts/bf16_noise_bounds.py)")
    for ln in lines:
        print(ln)
    print("# worst case per kind (-> oracle/bf16_ref.py NOISE: mean, frac, max as measured; limits = "
          f"{R.MEAN_X:g} x mean + {R.FLIP_ROWS:g} x max / rows, {R.FRAC_X:g} x frac + {R.FRAC_FLOOR:g}, {R.MAX_X:g} x max)")
    for kind, wv in sorted(worst.items()):
        print(f"{kind:7s} mean {wv['mean']:.2e}  frac {wv['frac']:.2e}  max {wv['max']:.2e}  row_count {wv['row_count']}")
