"""The numpy restatement of g4c_sample_points_adjoint (tests/sample_adjoint_ref.py) on the host: it is the transpose of
tests/sampler_ref.py's forward — ⟨S x, y⟩ = ⟨x, Sᵀ y⟩ to fp64 rounding, in 2-D and 3-D —, each deliberate mistake breaks that identity
by orders of magnitude, and the numpy.float32 loop stays inside the fp64 bound on every input the GPU test launches on."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sample_adjoint_ref as A                           # noqa: E402
import sampler_ref as SR                                 # noqa: E402


def _identity(idx_jm, coef_jm, n_nodes, nf, wrong=None, seed=0):
    """(|⟨S x, y⟩ − ⟨x, Sᵀ y⟩|, Σ of the magnitudes of every term of either side) in fp64."""
    rng = np.random.default_rng(seed)
    k, n_points = idx_jm.shape
    x, y = rng.standard_normal((n_nodes, nf)), rng.standard_normal((n_points, nf))
    sx, smag = SR.apply64(x, idx_jm.T, coef_jm.T)
    tables = A.node_tables(idx_jm, coef_jm, n_nodes, wrong=wrong)
    gx = A._walk(y, *tables, np.float64)[0]
    gmag = A.abs_adjoint(np.abs(y), *A.node_tables(idx_jm, coef_jm, n_nodes))
    return abs(float((sx * y).sum()) - float((x * gx).sum())), float((smag * np.abs(y)).sum() + (np.abs(x) * gmag).sum())


@pytest.mark.parametrize("dim", [2, 3])
def test_the_restatement_is_the_transpose_of_the_forward(dim):
    _, _, idx, coef = A.hub(dim)
    k, n_points = idx.shape
    off, in_pt, in_coef = A.node_tables(idx, coef, 400)
    assert off[0] == 0 and off[-1] == k * n_points and np.diff(off).max() >= 600 and (np.diff(off) == 0).any()
    # every list names its own node, in ascending flat position
    flat = idx.reshape(-1)
    perm = np.argsort(flat, kind="stable")
    assert np.array_equal(in_pt, perm % n_points) and np.array_equal(in_coef, coef.reshape(-1)[perm])
    for i in (0, 17, 399):
        q = perm[off[i]:off[i + 1]]
        assert (flat[q] == i).all() and (np.diff(q) > 0).all()
    for nf in (1, 3):
        err, scale = _identity(idx, coef, 400, nf)
        assert err <= (k * n_points + 400) * 2.0 ** -53 * scale, (err, scale)
        for wrong in A.WRONG:          # orders of magnitude, not ulps
            bad, _ = _identity(idx, coef, 400, nf, wrong=wrong)
            assert bad > 1e6 * max(err, 2.0 ** -53 * scale), (wrong, bad, err, scale)


def test_the_synthetic_tables_have_the_list_lengths_they_promise():
    for k in (1, 6, 16):
        idx, coef = A.synthetic(300, k, 257)
        off = A.node_tables(idx, coef, 300)[0]
        assert tuple(np.diff(off)[:7]) == A.LIST_LENGTHS + (0,) and idx.min() >= 0 and idx.max() < 300
        for wrong in A.WRONG:
            err, scale = _identity(idx, coef, 300, 3)
            bad, _ = _identity(idx, coef, 300, 3, wrong=wrong)
            assert bad > 1e6 * max(err, 2.0 ** -53 * scale), (k, wrong)
    assert A.BIG[0] * ((A.BIG[1] + 3) // 4) > 262_144


def test_the_fp32_loop_stays_inside_the_fp64_bound_on_the_gpu_tests_inputs():
    worst = 0.0
    for name, (idx, coef, n_nodes, widths) in A.cases().items():
        tables = A.node_tables(idx, coef, n_nodes)
        for nf in widths:
            gy = A.gy_of(idx.shape[1], nf)
            got = A.adjoint32(gy, *tables)
            assert got.dtype == np.float32 and got.shape == (n_nodes, nf)
            want, bound = A.adjoint64(gy, *tables)
            worst = max(worst, SR.within(got, want, bound, f"{name} F={nf}"))
            unused = np.diff(tables[0]) == 0
            assert unused.any() and not got[unused].view(np.int32).any()          # +0, sign bit clear
    assert 0.0 < worst <= 1.0
    print(f"MEASURED fp32 loop: |gx32 - fp64| / ((n_i + 1) 2^-24 sum|terms|): {worst:.3f}")
