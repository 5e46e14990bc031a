"""oracle/fwd_ref.py against the reference project's recorded outputs (tests/golden/blocks.pt) and against oracle.g4c_oracle; its
checker accepts what is as accurate as fp32 (the comparator under another summation order, the torch emulations of f16x3 and of the
three-way bf16 split) and rejects every perturbation, at each input class the GPU tests use.  No GPU."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import fwd_ref as R          # noqa: E402
from oracle import g4c_oracle as O       # noqa: E402

F64, F32 = torch.float64, torch.float32
BLOCK = dict(rtol=1e-4, atol=1e-4)
MIXES = ("A", "B", "C")


def _mlp_params(w, prefix=""):
    """(weights, biases, ln) from a state dict of the reference's MLP."""
    Ws, bs, i = [], [], 1
    while f"{prefix}MLP.linear_{i}.weight" in w:
        Ws.append(w[f"{prefix}MLP.linear_{i}.weight"]); bs.append(w[f"{prefix}MLP.linear_{i}.bias"]); i += 1
    g = w.get(f"{prefix}MLP.layer_norm.weight")
    return Ws, bs, (None if g is None else (g, w[f"{prefix}MLP.layer_norm.bias"]))


def _csr(col, n):
    """(off, perm) of the rows grouped by `col` (stable)."""
    off = torch.zeros(n + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(torch.bincount(col, minlength=n), 0)
    return off, torch.argsort(col, stable=True)


# ------------------------------------------------------------------ the fp64 reference restates the reference project's outputs
@pytest.mark.parametrize("i", range(8))
def test_golden_mlp(golden, i):
    c = golden("blocks.pt")[f"mlp_{i}"]
    L = R.Launch([R.Src(c["x"])], *_mlp_params(c["weights"]))
    torch.testing.assert_close(R.ref64(L)["y"].float(), c["y"], **BLOCK)
    torch.testing.assert_close(R.evaluate(L, F64)["y"], R.ref64(L)["y"], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("tag", ["gnblock_h128_mean", "gnblock_h32_sum", "gnblock_h32_mean", "gnblock_irregular", "edgemp"])
def test_golden_message_passing(golden, tag):
    """GNBlock / EdgeMP: message launch on [e | v[row] | v[col]], node launch that aggregates e' on load through the CSR of col — and
    the same through mp_layer (aggregate, then update)."""
    c = golden("blocks.pt")[tag]
    if tag == "edgemp":
        v, e, ei, names, mean = c["e"], c["a"], c["angle_index"], ("angle_mlp.", "edge_mlp."), True
        v_out, e_out = c["e_out"], c["a_out"]
    else:
        v, e, ei, names, mean = c["v"], c["e"], c["edge_index"], ("edge_mlp.", "node_mlp."), c["aggr"] == "mean"
        v_out, e_out = c["v_out"], c["e_out"]
    row, col = ei[0], ei[1]
    msg = R.Launch([R.Src(e), R.Src(v, index=row), R.Src(v, index=col)], *_mlp_params(c["weights"], names[0]))
    e64 = R.ref64(msg)["y"]
    torch.testing.assert_close(e64.float(), e_out, **BLOCK)
    off, perm = _csr(col, int(v.size(0)))
    uW, ub, uln = _mlp_params(c["weights"], names[1])
    node = R.Launch([R.Src(e64, segments=(off, perm), seg_mean=mean), R.Src(v)], uW, ub, uln)
    torch.testing.assert_close(R.ref64(node)["y"].float(), v_out, **BLOCK)
    torch.testing.assert_close(R.evaluate(node, F64)["y"], R.ref64(node)["y"], rtol=1e-11, atol=1e-11)
    if bool((col[1:] >= col[:-1]).all()):          # rows in segment order: the one-launch form
        got = R.mp_layer(msg, off, mean, uW, ub, uln, v, None)
        torch.testing.assert_close(got["v"].float(), v_out, **BLOCK)


@pytest.mark.parametrize("H", [32, 128])
def test_golden_down_up(golden, H):
    """DownMP ([e_12 | field], pooled by cluster, tanh) and UpMP ([-e_12 | field_lr[parent] | skip] with the sign folded, tanh)."""
    c = golden("blocks.pt")[f"downup_h{H}"]
    g = c["graph"]
    down = R.Launch([R.Src(g["e_12"]), R.Src(c["field1"])], *_mlp_params(c["down_weights"], "down_mlp."))
    m = R.ref64(down)["y"]
    cl = g["cluster_2"]
    n_cl = int(cl.max()) + 1
    pooled = torch.zeros(n_cl, H, dtype=F64).index_add_(0, cl, m) / torch.bincount(cl, minlength=n_cl).clamp(min=1)[:, None]
    f2 = torch.tanh(pooled[g["mask_2"]])
    torch.testing.assert_close(f2.float(), c["down_field"], **BLOCK)
    up = R.Launch([R.Src(g["e_12"], negate=True), R.Src(c["down_field"], index=g["idx1_to_idx2"]), R.Src(c["field1"])],
                  *_mlp_params(c["up_weights"], "up_mlp."), act="tanh")
    torch.testing.assert_close(R.ref64(up)["y"].float(), c["up_field"], **BLOCK)
    torch.testing.assert_close(R.evaluate(up, F64)["y"], R.ref64(up)["y"], rtol=1e-12, atol=1e-12)


def test_agrees_with_the_oracle_mlp_on_random_inputs():
    gen = torch.Generator().manual_seed(3)
    for k_in, widths, ln in ((384, (128, 128, 128), True), (5, (64, 3), False), (130, (128,), True), (256, (128, 128, 128, 128), True)):
        Ws, bs, lnp, _ = R.default_weights(k_in, widths, gen, ln, "ln")
        w = {}
        for i, (W, b) in enumerate(zip(Ws, bs)):
            w[f"m.MLP.linear_{i + 1}.weight"], w[f"m.MLP.linear_{i + 1}.bias"] = W, b
        if ln:
            w["m.MLP.layer_norm.weight"], w["m.MLP.layer_norm.bias"] = lnp
        x = torch.randn(77, k_in, generator=gen)
        L = R.Launch([R.Src(x[:, :k_in // 2]), R.Src(x, col0=k_in // 2)], Ws, bs, lnp)
        torch.testing.assert_close(R.ref64(L)["y"].float(), O.mlp(x, w, "m"), **BLOCK)
        R.comparator_agrees(R.ref64(L)["y"], R.evaluate(L, F32)["y"], "random")


# ------------------------------------------------------------------ the checker: what it accepts, what it rejects
N, NT, H = 1000, 700, 128


def control_launch(mix, seed=0):
    """A launch with every feature a perturbation needs: block 0 = rows of input class `mix` read through an index with SELU on load,
    block 1 = an aggregation on load (mean, through a permutation) of N(0, 1) messages, one gathered additive block, three layers,
    a random LayerNorm, two heads; 1000 rows (a partial last tile).  Returns (launch, row classes, head weights)."""
    gen = torch.Generator().manual_seed(100 + seed)
    table = R.mixed_rows(N, H, mix, gen)
    gidx = torch.randperm(N, generator=gen)
    deg = torch.randint(1, 9, (N,), generator=gen)
    col = torch.arange(N).repeat_interleave(deg)
    col = col[torch.randperm(int(col.numel()), generator=gen)]
    off, perm = _csr(col, N)
    msgs = torch.randn(int(col.numel()), H, generator=gen)
    P, pidx = torch.randn(NT, H, generator=gen), torch.randint(0, NT, (N,), generator=gen)
    Ws, bs, lnp, hs = R.default_weights(2 * H, (H, H, H), gen, True, "ln", n_heads=2)
    L = R.Launch([R.Src(table, index=gidx, pre_act="selu"), R.Src(msgs, segments=(off, perm), seg_mean=True)], Ws, bs, lnp, "selu",
                 adds=[R.Add(P, pidx)])
    return L, R.classes_through(R.row_classes(N), gidx), hs


def _row_of(classes, name):
    return int(torch.nonzero(classes[name])[3])


def perturbed_pairs(mix, split="f16x3"):
    """{perturbation: (got, ref64, cmp32, classes)} — each pair must be REJECTED.  `got` is the emulated kernel's correct output against
    a perturbed reference, or (lose_*) a defective emulation against the correct reference."""
    L, cls, hs = control_launch(mix)
    good = R.evaluate(L, F32, R.split_linear(split))["out"]
    ref, cmp32 = R.ref64(L)["out"], R.evaluate(L, F32)["out"]
    out = {}
    for which in ("wl_xh", "wh_xl", "both"):
        out[f"lose_low_product:{which}"] = (R.lose_low_product(L, which), ref, cmp32, cls)
    def pair(Lp):          # a wrong formula, with the comparator OF that formula
        return good, R.ref64(Lp)["out"], R.evaluate(Lp, F32)["out"], cls
    out["swap_adjacent_columns"] = pair(R.swap_adjacent_columns(L, 40))
    out["swap_adjacent_columns:layer2"] = pair(R.swap_adjacent_columns(L, 77, layer=2))
    out["zero_last_partial_row"] = (good, R.zero_last_partial_row(ref), R.zero_last_partial_row(cmp32), cls)
    out["skip_pre_act"] = pair(R.skip_pre_act(L, 0))
    for name in R.CLASS_NAMES:          # the row-local ones at a row of each class
        r = _row_of(cls, name)
        out[f"row_in_next_segment:{name}"] = pair(R.row_in_next_segment(L, 1, r))
        out[f"wrong_gather_row:{name}"] = pair(R.wrong_gather_row(L, 0, r))
        out[f"wrong_gather_row:additive:{name}"] = pair(R.wrong_gather_row(L, 0, r, additive=True))
    h_got = R.heads(good, hs, F32)[1]          # (an fp32 product of the emulated rows stands in for the kernel's head)
    z = R.ref64(L)["z"]
    out["head_from_pre_activation"] = (h_got, R.heads(z, hs)[1], R.heads(z.float(), hs, F32)[1], cls)
    return out


@pytest.mark.parametrize("mix", MIXES)
def test_checker_accepts_what_is_as_accurate_as_fp32(mix):
    L, cls, hs = control_launch(mix)
    ref, cmp32 = R.ref64(L)["out"], R.evaluate(L, F32)["out"]
    R.comparator_agrees(ref, cmp32, mix)
    torch.testing.assert_close(R.evaluate(L, F64)["out"], ref, rtol=1e-11, atol=1e-11)
    gen = torch.Generator().manual_seed(9)

    def permuted(x, W):          # the comparator under another summation order
        p = torch.randperm(int(W.size(1)), generator=gen)
        return x[:, p] @ W.to(x.dtype)[:, p].t()
    R.assert_as_accurate_as_fp32(R.evaluate(L, F32, permuted)["out"], ref, cmp32, cls, f"{mix} permuted fp32")
    for split in ("f16x3", "bf16x6"):
        y = R.evaluate(L, F32, R.split_linear(split))["out"]
        R.assert_as_accurate_as_fp32(y, ref, cmp32, cls, f"{mix} {split} emulation")
        for j, h in enumerate(R.heads(y, hs, F32)):
            R.assert_as_accurate_as_fp32(h, R.heads(y, hs)[j], R.heads(y, hs, F32)[j], cls, f"{mix} {split} head {j}")


@pytest.mark.parametrize("mix", MIXES)
def test_checker_rejects_every_perturbation(mix):
    for name, (got, ref, cmp32, cls) in perturbed_pairs(mix).items():
        assert R.rejects(R.assert_as_accurate_as_fp32, got, ref, cmp32, cls, f"{mix} {name}"), f"{mix}: {name} passes the checker"


def test_fused_aggregate_reference_is_a_sequential_fp32_sum():
    gen = torch.Generator().manual_seed(4)
    deg = torch.tensor([0, 0, 3, 32, 0, 1, 7, 0])
    rows = torch.randn(int(deg.sum()), 8, generator=gen)
    off = torch.zeros(9, dtype=torch.int64); off[1:] = torch.cumsum(deg, 0)
    want = torch.zeros(8, 8)
    for s in range(8):
        for r in range(int(off[s]), int(off[s + 1])):
            want[s] += rows[r]
    assert torch.equal(R.segment_reduce_fp32(rows, off, False), want)
    assert torch.equal(R.segment_reduce_fp32(rows, off, True), want / deg.clamp(min=1)[:, None].float())
    moved = R.segment_reduce_fp32(rows, R.move_boundary(off, 3), False)
    assert not torch.equal(moved, want)


def rejection_ratios():
    out = {}
    for mix in MIXES:
        for name, (got, ref, cmp32, cls) in perturbed_pairs(mix).items():
            out[(mix, name)] = R.worst_ratio(R.accuracy_ratios(got, ref, cmp32, cls))
    return out


def test_committed_rejection_ratios_are_what_the_code_measures():
    got = rejection_ratios()
    assert set(got) == set(R.REJECTION)
    for k, want in R.REJECTION.items():
        # (one row's error over the comparator's largest: the row-local entries move more with the BLAS build's summation order)
        band = 4.0 if k[1].split(":")[0] in ("wrong_gather_row", "row_in_next_segment", "zero_last_partial_row") else 1.5
        assert want > 10.0 and got[k] > 10.0 and want / band <= got[k] <= want * band, (k, got[k], want)


if __name__ == "__main__":          # prints the table for oracle/fwd_ref.py
    for k, v in rejection_ratios().items():
        print(f"    {k!r}: {v:.3g},")
