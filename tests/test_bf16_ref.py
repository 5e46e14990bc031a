"""The rounded-bf16 reference (oracle/bf16_ref.py) and its checker, on CPU: the rounding is torch's own round-to-nearest-even bf16, the
reference restates one launch the way a straightforward torch evaluation does, the committed bounds are what the derivation script
measures, and the checker accepts the freedom of a correct kernel (fp32 sums) while rejecting each perturbation the GPU tests use as
a negative control."""
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from oracle import bf16_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 128


def test_bf16_rne_is_torchs_rounding():
    g = torch.Generator().manual_seed(0)
    x = torch.cat([torch.randn(100000, generator=g) * 10 ** torch.randint(-30, 30, (100000,), generator=g).float(),
                   torch.tensor([0.0, -0.0, 1.0, -1.0, 3.0e38, -3.0e38, 1e-40, -1e-40])])
    # exact ties: the 16 dropped bits are 0x8000, with an even and an odd kept bit
    ties = torch.tensor([0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x00018000, 0x7F008000], dtype=torch.int64)
    x = torch.cat([x, torch.where(ties >= 1 << 31, ties - (1 << 32), ties).to(torch.int32).view(torch.float32)])
    assert torch.equal(R.bf16_rne(x), x.to(torch.bfloat16).double())
    assert torch.equal(R.bf16_rne(x.double()), x.to(torch.bfloat16).double())
    rtz = R.bf16_round(x, "rtz")
    assert (rtz.abs() <= x.double().abs()).all() and not torch.equal(rtz, R.bf16_rne(x))


def test_reference_restates_one_launch():
    """A small three-block launch with SELU on load, a gather, a narrow block and LayerNorm == the same arithmetic written out with
    torch's bf16 casts; the hoisted form with the products as additive rows is the same launch up to the products' rounding."""
    g = torch.Generator().manual_seed(1)
    w = {"MLP.linear_1.weight": torch.randn(H, 2 * H + 3, generator=g) * 0.06, "MLP.linear_1.bias": torch.randn(H, generator=g) * 0.1,
         "MLP.linear_2.weight": torch.randn(H, H, generator=g) * 0.09, "MLP.linear_2.bias": torch.randn(H, generator=g) * 0.1,
         "MLP.layer_norm.weight": 1 + 0.1 * torch.randn(H, generator=g), "MLP.layer_norm.bias": 0.1 * torch.randn(H, generator=g)}
    n = 50
    e, v, x3 = torch.randn(n, H, generator=g), torch.randn(9, H, generator=g), torch.randn(n, 3, generator=g)
    idx = torch.randint(0, 9, (n,), generator=g)
    got = R.mlp(w, [R.Block(e, pre_act="selu"), R.Block(v, index=idx), R.Block(x3, narrow=True)], n, act="tanh")
    r = lambda t: t.float().to(torch.bfloat16).double()
    W1, W2 = w["MLP.linear_1.weight"].double(), w["MLP.linear_2.weight"].double()
    h = (r(F.selu(e)) @ r(W1[:, :H]).T + r(v[idx]) @ r(W1[:, H:2 * H]).T + x3.double() @ W1[:, 2 * H:].float().double().T
         + w["MLP.linear_1.bias"].double())
    y = r(F.selu(h)) @ r(W2).T + w["MLP.linear_2.bias"].double()
    want = torch.tanh(F.layer_norm(y, (H,), w["MLP.layer_norm.weight"].double(), w["MLP.layer_norm.bias"].double(), 1e-5))
    torch.testing.assert_close(got, want, rtol=0, atol=1e-12)
    # hoisted: the gathered block's product as additive rows, fp32 (exact products of the rounded operands) -> the same launch
    p32 = R.products(W1[:, H:2 * H].float(), v, bf16_out=False)
    w2 = dict(w)
    w2["MLP.linear_1.weight"] = w["MLP.linear_1.weight"][:, :2 * H]
    full = R.mlp(w2, [R.Block(e, pre_act="selu"), R.Block(v, index=idx)], n)
    hoisted = R.mlp(w2, [R.Block(e, pre_act="selu")], n, additive=[R.Additive(p32, idx)], first_cols=(0, H))
    torch.testing.assert_close(hoisted, full, rtol=0, atol=1e-6)
    # stored rows / aggregate
    assert torch.equal(R.stored_rows(full, "bf16_selu"), F.selu(full).float().to(torch.bfloat16).double())
    off = torch.tensor([0, 3, 3, 10, n])
    agg = R.segment_mean(full, off)
    assert torch.equal(agg[1], torch.zeros(H, dtype=torch.float64))
    torch.testing.assert_close(agg[2], full[3:10].mean(0), rtol=0, atol=1e-12)


def _numbers(text):
    return [(re.sub(r"[-+0-9.e]+(?=\s|\)|$)", "#", ln), [float(x) for x in re.findall(r"(?<![\w>])[-+]?\d+\.\d+e[-+]\d+|(?<=\s)\d+(?=\s|$)", ln)])
            for ln in text.splitlines()]


def test_committed_bounds_are_what_the_derivation_measures():
    """scripts/bf16_noise_bounds.py reproduces profiles/r07_bf16_noise_bounds.log — the same lines, every number within 5 % (the fp32
    CPU sums may differ in their last bits with another BLAS build) — and NOISE holds its worst cases."""
    log = open(os.path.join(ROOT, "profiles", "r07_bf16_noise_bounds.log")).read()
    run = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "bf16_noise_bounds.py")], capture_output=True, text=True,
                         timeout=600, check=True)
    got, want = _numbers(run.stdout), _numbers(log)
    assert [t for t, _ in got] == [t for t, _ in want]
    for (text, a), (_, b) in zip(got, want):
        assert len(a) == len(b) and all(abs(x - y) <= 0.05 * abs(y) + 1e-9 for x, y in zip(a, b)), (text, a, b)
    for kind, mean, frac, mx in re.findall(r"^(\w+)\s+mean (\S+)\s+frac (\S+)\s+max (\S+)\s+row_count", log, re.M):
        m, _, f, x, _, _ = R.NOISE[kind]
        assert (m, f, x) == (float(mean), float(frac), float(mx)), kind


@pytest.fixture(scope="module")
def launch():
    """A hoisted two-layer message launch (K = 5 rows per receiver) evaluated in fp64 and with fp32 sums."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import bf16_noise_bounds as D
    finally:
        sys.path.pop(0)
    g = torch.Generator().manual_seed(5)
    n, K = 800, 5
    E = n * K
    w = D.mlp_weights(3 * H, 2, True, 5)
    e, v = torch.randn(E, H, generator=g), torch.randn(n, H, generator=g)
    row, col = torch.randint(0, n, (E,), generator=g), torch.arange(n).repeat_interleave(K)
    adds = [R.Additive(R.products(w["MLP.linear_1.weight"][:, H:2 * H], v), row),
            R.Additive(R.products(w["MLP.linear_1.weight"][:, 2 * H:], v), col)]
    run = lambda ar=R.FP64, **kw: R.mlp(w, [R.Block(e, pre_act="selu")], E, additive=adds, first_cols=(0, H), ar=ar, **kw)
    off = torch.arange(0, E + 1, K)
    y32 = run(R.Arith("fp32"))
    return dict(run=run, off=off, y=run(), y32=y32, agg32=R.segment_mean(y32, off), n=n)


def test_checker_accepts_fp32_sums(launch):
    R.assert_bf16_order_noise(launch["y32"], launch["y"], "rows32")
    R.assert_bf16_order_noise(launch["agg32"], R.segment_mean(launch["y"], launch["off"]), "agg32")
    R.assert_bf16_order_noise(R.stored_rows(launch["y32"], "bf16_selu"), R.stored_rows(launch["y"], "bf16_selu"), "rows16")


@pytest.mark.parametrize("perturbation", ["round_toward_zero", "swap_adjacent_columns", "row_in_next_segment"])
def test_checker_rejects_a_perturbed_reference(launch, perturbation):
    """The negative controls of tests/test_gpu_bf16.py, here against the fp32-sum evaluation: each must be rejected."""
    if perturbation == "row_in_next_segment":
        ok, s, lim = R.check_bf16_order_noise(launch["agg32"], R.segment_mean(launch["y"], R.move_row_to_next_segment(launch["off"], launch["n"] // 2)),
                                             "agg32")
    elif perturbation == "round_toward_zero":
        ok, s, lim = R.check_bf16_order_noise(launch["y32"], launch["run"](R.Arith(weight_round="rtz")), "rows32")
    else:
        ok, s, lim = R.check_bf16_order_noise(launch["y32"], launch["run"](perturb=R.swap_adjacent_columns), "rows32")
    assert not ok, (perturbation, s, lim)
