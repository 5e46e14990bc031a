"""The numpy restatement of the mesh gradient (tests/gradient_ref.py) against independent references, on the host: the fp64 weights
against numpy.linalg.lstsq, a linear field's slope, the degenerate rule on hand-made nodes, and the precondition the GPU tests
(tests/test_gpu_mesh_gradient.py) rely on — no node of any test mesh sits near the degeneracy threshold."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gradient_ref as R          # noqa: E402

SIZES = (0, 1, 2, 63, 64, 65, 257, 1000)


def meshes():
    for n in SIZES:
        for dim in (2, 3):
            yield f"uniform n {n} dim {dim}", R.uniform_mesh(n, dim)
            yield f"ragged n {n} dim {dim}", R.ragged_mesh(n, dim)


@pytest.mark.parametrize("power", [0, 1, 2])
def test_fp64_weights_equal_lstsq(power):
    for what, m in meshes():
        for mesh in (m, m.shuffled(1)):
            g64, g32, src, degen = R.weights(mesh.off, mesh.perm, mesh.src32, mesh.rel, mesh.dim, power)
            ref = R.lstsq_weights(mesh.off, mesh.perm, mesh.rel, mesh.dim, power)
            node = np.repeat(np.arange(mesh.n), np.diff(mesh.off))
            ok = degen[node] == 0
            scale = np.abs(ref[ok]).max() if ok.any() else 1.0
            assert np.abs(g64[ok] - ref[ok]).max(initial=0.0) <= 1e-10 * scale, (what, power)
            assert not g64[~ok].any() and g32.dtype == np.float32
            pe = np.arange(mesh.row.size) if mesh.perm is None else mesh.perm
            assert np.array_equal(src, mesh.src32[pe]) and np.array_equal(mesh.col[pe], node)


@pytest.mark.parametrize("dim", [2, 3])
def test_a_linear_field_gives_back_its_slope(dim):
    for mesh in (R.uniform_mesh(257, dim), R.ragged_mesh(257, dim).shuffled(2)):
        rng = np.random.default_rng(7)
        slope = rng.standard_normal((3, dim))
        x = (mesh.pos @ slope.T + rng.standard_normal(3)).astype(np.float32)
        nfld = min(3, 8 // dim)
        for power in (0, 1, 2):
            g64, g32, src, degen = R.weights(mesh.off, mesh.perm, mesh.src32, mesh.rel, mesh.dim, power)
            prog = R.program(tuple(f"grad:{f}" for f in range(nfld)), dim, 3)
            cur64, mag = R.derived64(x, mesh.off, g32, src, prog)
            cur32 = R.derived32(x, mesh.off, g32, src, prog)
            keep = (degen == 0) & ~np.isin(np.arange(mesh.n), list(mesh.planted))
            want = np.concatenate([slope[f] for f in range(nfld)])
            # x is rounded to fp32 (2^-24 relative per value, both ends of a difference) and g once: the slope comes back within the
            # magnitude of the terms times a few roundings
            x_mag = np.abs(x).max()
            gsum = np.zeros(mesh.n)
            np.add.at(gsum, np.repeat(np.arange(mesh.n), np.diff(mesh.off)), np.abs(g32).max(1))
            tol = (2.0 ** -23 * x_mag * gsum * dim)[:, None] + 2.0 ** -23 * mag
            assert (np.abs(cur64 - want)[keep] <= tol[keep]).all(), (dim, power)
            assert R.within(cur32, cur64, R.bound32(mag, mesh.max_deg)) <= 1.0
            assert not cur32[degen == 1].any()


def test_the_degenerate_rule_on_hand_made_nodes():
    # node 0: no in-edge; 1: one in-edge; 2: three collinear neighbours; 3: a proper triangle; 4: a proper triangle and a zero-length edge
    rel = np.array([[0.1, 0.2],
                    [0.1, 0.1], [-0.2, -0.2], [0.3, 0.3],
                    [0.1, 0.0], [0.0, 0.1], [-0.1, -0.1],
                    [0.1, 0.0], [0.0, 0.1], [-0.1, -0.1], [0.0, 0.0]], dtype=np.float32)
    col = np.array([1, 2, 2, 2, 3, 3, 3, 4, 4, 4, 4])
    off, perm = R.csr_of(col, 5)
    assert perm is None and off.tolist() == [0, 0, 1, 4, 7, 11]
    src32 = np.arange(11, dtype=np.int32) % 5
    for power, want in ((0, [1, 1, 1, 0, 0]), (1, [1, 1, 1, 0, 1]), (2, [1, 1, 1, 0, 1])):
        g64, g32, src, degen = R.weights(off, perm, src32, rel, 2, power)
        assert degen.tolist() == want, (power, degen)
        assert not g32[:4].any() and g32[4:7].any() and (g32[7:].any() == (power == 0))
        if power == 0:
            assert not g32[10].any()          # the zero-length edge itself carries no weight
    # 3-D: coplanar neighbours, and two in-edges
    rel3 = np.array([[0.1, 0, 0], [0, 0.1, 0], [-0.1, -0.1, 0], [0.2, -0.1, 0], [0.1, 0, 0], [0, 0.1, 0.1],
                     [0.1, 0, 0], [0, 0.1, 0], [0, 0, 0.1], [-0.1, -0.1, -0.1]], dtype=np.float32)
    off3, _ = R.csr_of(np.array([0, 0, 0, 0, 1, 1, 2, 2, 2, 2]), 3)
    for power in (0, 1, 2):
        assert R.weights(off3, None, np.zeros(10, np.int32), rel3, 3, power)[3].tolist() == [1, 1, 0]


def test_no_node_of_a_test_mesh_sits_near_the_threshold():
    """The precondition of the GPU tests: det M / (tr M / dim)^dim >= 1e-3 at every non-degenerate node, <= 1e-14 (or no number) at
    every degenerate one, for every power.  The smallest ratio of a kNN cloud of 257 - 1000 points here (k = 6 in 2-D, k = 6, 8 in
    3-D, the three powers) is 1.06e-2: a factor of ten inside the precondition."""
    lowest = np.inf
    for what, m in meshes():
        for power in (0, 1, 2):
            degen = R.weights(m.off, m.perm, m.src32, m.rel, m.dim, power)[3]
            r = R.ratio(m.off, m.perm, m.rel, m.dim, power)
            good = r[degen == 0]
            assert (good >= 1e-3).all(), (what, power, good.min())
            bad = r[degen == 1]
            assert (~np.isfinite(bad) | (bad <= 1e-14)).all(), (what, power, bad)
            if what.startswith("uniform") and m.n >= 257 and good.size:
                lowest = min(lowest, good.min())
            if m.planted:
                kinds = {k: degen[i] for i, k in m.planted.items()}
                assert all(degen[i] == 1 for i, k in m.planted.items() if k != "zero-edge" or power > 0), (what, power, kinds)
    for k, dim in ((6, 2), (6, 3), (8, 3)):
        for n in (257, 1000):
            m = R.uniform_mesh(n, dim, k=k, seed=3)
            for power in (0, 1, 2):
                lowest = min(lowest, R.ratio(m.off, m.perm, m.rel, dim, power).min())
    print(f"smallest ratio of a non-degenerate node of the kNN clouds: {lowest:.3e}")
    assert lowest >= 1e-2, lowest


def test_the_fp32_bound_on_the_test_clouds():
    """(max_deg + 3) 2^-24 Σ|terms| against the fp64 restatement, in numpy, before any device run: the bound holds on these clouds (measured / allowed = 0.35 at the worst node)."""
    worst = 0.0
    for dim, k in ((2, 6), (3, 6), (3, 8)):
        m = R.uniform_mesh(1000, dim, k=k, seed=3)
        x = np.random.default_rng(1).standard_normal((m.n, 3)).astype(np.float32)
        g32, src = R.weights(m.off, m.perm, m.src32, m.rel, dim, 2)[1:3]
        prog = R.program(("div", "vort"), dim, 3)
        cur64, mag = R.derived64(x, m.off, g32, src, prog)
        worst = max(worst, R.within(R.derived32(x, m.off, g32, src, prog), cur64, R.bound32(mag, m.max_deg), f"dim {dim} k {k}"))
    print(f"fp32 loop against fp64, measured / allowed: {worst:.3f}")
    assert 0.0 < worst <= 1.0, worst


def test_statistics_and_slots():
    q = np.array([[1.0, -2.0], [3.0, 0.5], [-4.0, 0.0]], dtype=np.float32)
    assert R.stats64(q).tolist() == [[26.0, 8.0, 4.0], [4.25, 2.5, 2.0]]
    assert R.stats64(q[:0]).tolist() == [[0.0, 0.0, 0.0]] * 2
    assert [R.snap_slot(t, 3, 2) for t in range(-1, 9)] == [None, None, None, 0, None, None, 1, None, None, None]
    assert [R.snap_slot(t, 1, 3) for t in range(4)] == [0, 1, 2, None] and R.snap_slot(2, 0, 5) is None


def test_the_negative_controls_differ():
    m = R.ragged_mesh(257, 2).shuffled(3)
    x = np.random.default_rng(2).standard_normal((m.n, 2)).astype(np.float32)
    g64, g32, src, degen = R.weights(m.off, m.perm, m.src32, m.rel, 2, 2)
    cur = R.derived32(x, m.off, g32, src, R.program(("vort",), 2, 2))
    t = R.weights(m.off, m.perm, m.src32, m.rel, 2, 2, wrong="transposed-g")
    assert np.array_equal(t[1], -g32) and np.array_equal(t[3], degen)
    u = R.weights(m.off, m.perm, m.src32, m.rel, 2, 2, wrong="src-unpermuted")
    assert not np.array_equal(u[2], src)
    assert np.array_equal(R.derived32(x, m.off, g32, src, R.program(("vort",), 2, 2, wrong="vort-sign")), -cur)
