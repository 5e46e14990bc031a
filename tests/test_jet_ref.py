"""The numpy restatement of the quadratic-fit operator (tests/jet_ref.py) against independent references, on the host, all fp64: its
Cholesky weights against numpy.linalg.lstsq, exactness on quadratics, the adjoint identity, the degenerate rule on the planted
nodes, convergence on a smooth field — with the composed linear Laplacian as the negative control that says why the operator
exists — and manufactured flows whose momentum residual is zero.  The worst measured / allowed ratios are printed by the last test
(tests/JET_MEASURED.md)."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import gradient_ref as R          # noqa: E402
import jet_ref as J               # noqa: E402

EPS = 2.0 ** -53
RATIOS = {}


def note(name, r):
    RATIOS[name] = max(RATIOS.get(name, 0.0), float(r))


@functools.lru_cache(maxsize=None)
def mesh_of(n, dim, kind="cloud", k=None, shuffled=False):
    m = J.stencil_mesh(n, dim, k=k, kind=kind)
    return m.shuffled(3) if shuffled else m


def scaled_norm(c64, sc, node):
    """[S]: ‖c_s / sc‖₂ — the size of an entry's solution in the unit-diagonal coordinates the factorisation works in."""
    with np.errstate(all="ignore"):
        return np.sqrt(((c64 / sc[node]) ** 2).sum(1))


# ------------------------------------------------------------------ weights
@pytest.mark.parametrize("power", [0, 1, 2])
@pytest.mark.parametrize("dim,kind,shuffled", [(2, "cloud", False), (2, "lattice", True), (3, "cloud", True), (3, "lattice", False)])
def test_cholesky_weights_equal_lstsq_within_the_condition_number(dim, kind, shuffled, power):
    """Both forms solve the same least-squares problem.  A Cholesky solve of the scaled normal equations A z = t is backward stable:
    (A + δA) z = t with ‖δA‖ <= ~Q² 2⁻⁵³ ‖A‖, so ‖δz‖ <= Q² 2⁻⁵³ κ(A) ‖z‖; lstsq's own error is of the order of sqrt(κ).  In the unscaled
    unknowns c_q = sc_q z_q: allowed = 4 Q² 2⁻⁵³ κ(A) sc_q max_s ‖c_s / sc‖₂ (the 4: both solves, and the two triangular solves; the
    largest entry of the node, because lstsq solves for all the node's entries at once and its error is relative to the whole
    pseudo-inverse: a zero row under power 0 comes back as 1e-16, not 0)."""
    m = mesh_of(300, dim, kind, None, shuffled)
    Q = J.q_of(dim)
    c64, c32, src, degen = J.weights(m.off, m.perm, m.src32, m.rel, dim, power)
    ref, cond = J.lstsq_weights(m.off, m.perm, m.rel, dim, power)
    sc = J.factor(m.off, m.perm, m.rel, dim, power)[2]
    node = np.repeat(np.arange(m.n), np.diff(m.off))
    ok = degen[node] == 0
    assert ok.sum() > 0.9 * ok.size and np.isfinite(cond[degen == 0]).all()
    top = np.zeros(m.n)
    np.maximum.at(top, node[ok], scaled_norm(ref, sc, node)[ok])
    with np.errstate(all="ignore"):
        allowed = 4 * Q * Q * EPS * (cond * top)[node][:, None] * sc[node]
    note(f"weights vs lstsq dim {dim} {kind} power {power}", J.within(c64[ok], ref[ok], allowed[ok], "c64"))
    assert not c64[~ok].any() and c32.dtype == np.float32
    pe = np.arange(m.row.size) if m.perm is None else m.perm
    assert np.array_equal(src, m.src32[pe]) and np.array_equal(m.col[pe], node)


@pytest.mark.parametrize("dim", [2, 3])
def test_the_planted_nodes_and_only_they_are_degenerate(dim):
    m = mesh_of(300, dim)
    assert set(m.planted.values()) == set(J.PLANTED_2D if dim == 2 else J.PLANTED_3D)
    for power in (0, 1, 2):
        degen = J.weights(m.off, m.perm, m.src32, m.rel, dim, power)[3]
        want = np.zeros(m.n, np.uint8)
        for node, kind in m.planted.items():
            want[node] = 0 if (kind == "zero-length" and power == 0) else 1          # (weight 1 and a zero row: the other entries decide)
        assert np.array_equal(degen, want), power


@pytest.mark.parametrize("dim", [2, 3])
def test_the_threshold_is_invariant_under_scaling_the_mesh(dim):
    """x -> λx multiplies the normal matrix's entries by powers of λ that differ by 10^±24 over λ = 1e-3 .. 1e3; the pivots of the
    unit-diagonal matrix, where the threshold sits, move by rounding only."""
    m = mesh_of(300, dim)
    base = J.min_pivot(m.off, m.perm, m.rel, dim, 2)
    for lam in (1e-3, 1e3):
        piv = J.min_pivot(m.off, m.perm, (m.rel.astype(np.float64) * lam).astype(np.float32), dim, 2)
        ok = np.isfinite(base) & (base > 1e-12)
        assert np.array_equal(np.isfinite(piv) & (piv > 1e-12), ok)
        assert np.abs(piv[ok] / base[ok] - 1.0).max() < 1e-3          # (rel is rounded to fp32 after the scaling)


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("power", [0, 2])
def test_the_fit_is_exact_on_random_quadratics(dim, power):
    """x = a + g·p + ½ pᵀ H p: the jet at every non-degenerate node is (g + H p_i, H) up to the solve's error — per derivative q
    allowed = 4 Q² 2⁻⁵³ κ Σ_s sc_q ‖c_s / sc‖₂ |x_s − x_i| (the bound on the weights above, through the sum).  The fields are evaluated
    from the fp32 vectors the weights saw, so nothing else enters."""
    m = mesh_of(300, dim, "cloud", None, True)
    Q, rng = J.q_of(dim), np.random.default_rng(7)
    c64, _, src, degen = J.weights(m.off, m.perm, m.src32, m.rel, dim, power)
    cond = J.lstsq_weights(m.off, m.perm, m.rel, dim, power)[1]
    sc = J.factor(m.off, m.perm, m.rel, dim, power)[2]
    node = np.repeat(np.arange(m.n), np.diff(m.off))
    pe = np.arange(m.row.size) if m.perm is None else m.perm
    d = -m.rel[pe].astype(np.float64)          # sender − receiver, as the weights saw it
    for trial in range(3):
        g, H = rng.standard_normal(dim), rng.standard_normal((dim, dim))
        H = H + H.T
        # the field's differences along every entry, about the receiver's own point p_i (taken at the origin: exact for a quadratic)
        gi = rng.standard_normal((m.n, dim))          # the gradient AT node i (any: g + H p_i for some p_i)
        diff = (gi[node] * d).sum(1) + 0.5 * np.einsum("sa,ab,sb->s", d, H, d)
        jet = np.zeros((m.n, Q))
        np.add.at(jet, node, c64 * diff[:, None])
        want = np.concatenate([gi, np.tile([H[a, b] for a, b in J.pairs(dim)], (m.n, 1))], axis=1)
        mag = np.zeros((m.n, Q))
        with np.errstate(all="ignore"):          # (the planted nodes' scales are no numbers: they are not compared)
            np.add.at(mag, node, sc[node] * (scaled_norm(c64, sc, node) * np.abs(diff))[:, None])
        ok = degen == 0
        note(f"exact on quadratics dim {dim} power {power}", J.within(jet[ok], want[ok], (4 * Q * Q * EPS * cond[:, None] * mag)[ok], "jet"))
    for wrong in ("sign", "diagonal-factor"):
        bad = J.weights(m.off, m.perm, m.src32, m.rel, dim, power, wrong=wrong)[0]
        jet = np.zeros((m.n, Q))
        np.add.at(jet, node, bad * diff[:, None])
        assert J.rejects(J.within, jet[ok], want[ok], (4 * Q * Q * EPS * cond[:, None] * mag)[ok]), wrong


@pytest.mark.parametrize("dim", [2, 3])
def test_the_adjoint_identity_holds_in_fp64(dim):
    """⟨D x, y⟩ = ⟨x, Dᵀ y⟩ for the fp64 forms on the same fp32 table: both sides are the same Σ c·coef·x·y reordered — allowed
    2 (n_terms + 4) 2⁻⁵³ Σ|terms| (the records' bound on a sum added in any order)."""
    m = mesh_of(300, dim, "cloud", None, True)
    rng = np.random.default_rng(5)
    c32, src = J.weights(m.off, m.perm, m.src32, m.rel, dim, 2)[1:3]
    nf = 4
    for names in (("grad:0", "lap:1", "div"), ("hess:2", "vort") if dim == 2 else ("hess:3", "lap:0")):
        prog = J.program(names, dim, nf, field_scale=[1.0, 0.5, 2.0, 1.5])
        x = rng.standard_normal((m.n, nf)).astype(np.float32)
        y = rng.standard_normal((m.n, len(prog))).astype(np.float32)
        dx, mag = J.derived64(x, m.off, c32, src, prog)
        gx, mag_t, _ = J.adjoint64(y, m.off, c32, src, prog, nf)
        lhs, rhs = (dx * y).sum(), (gx * x).sum()
        total = (mag * np.abs(y)).sum() + (mag_t * np.abs(x)).sum()
        n_terms = 2 * c32.size * nf
        allowed = 2 * (n_terms + 4) * EPS * total
        assert abs(lhs - rhs) <= allowed
        note(f"adjoint identity dim {dim}", abs(lhs - rhs) / allowed)
        wrong = J.adjoint32(y, m.off, c32, src, prog, nf, wrong="no-diagonal").astype(np.float64)
        assert abs(lhs - (wrong * x).sum()) > allowed


# ------------------------------------------------------------------ convergence
def _nearest(pos, k):
    from scipy.spatial import cKDTree
    return cKDTree(pos).query(pos, k + 1)[1][:, 1:]


@functools.lru_cache(maxsize=None)
def convergence(n):
    """Relative r.m.s. errors over the nodes with 0.1 < x, y < 0.9 of f = sin 2πx sin 2πy on np.random.default_rng(1).random((n, 2)),
    weights |d|⁻²: (∇²f composed from the linear fit over the 6 nearest, ∇²f by the quadratic fit over the 12 nearest, ∂ₓf linear,
    ∂ₓf quadratic)."""
    pos = np.random.default_rng(1).random((n, 2))
    f = (np.sin(2 * np.pi * pos[:, 0]) * np.sin(2 * np.pi * pos[:, 1]))[:, None]
    fx = 2 * np.pi * np.cos(2 * np.pi * pos[:, 0]) * np.sin(2 * np.pi * pos[:, 1])
    lap = -8 * np.pi ** 2 * f[:, 0]
    inner = ((pos > 0.1) & (pos < 0.9)).all(1)

    def rel_rms(got, want):
        return float(np.sqrt(((got - want)[inner] ** 2).mean()) / np.sqrt((want[inner] ** 2).mean()))

    def stencil(k):
        row, col, rel = R._edges(pos, list(_nearest(pos, k)))
        off, perm = J.csr_of(col, n)
        return off, perm, row.astype(np.int32), (pos[col] - pos[row])

    off, perm, src32, rel = stencil(6)
    g64, _, src, degen = R.weights(off, perm, src32, rel.astype(np.float32), 2, 2)
    assert not degen.any()
    node = np.repeat(np.arange(n), np.diff(off))

    def grad(x):
        out = np.zeros((n, 2))
        np.add.at(out, node, g64 * (x[src] - x[node])[:, None])
        return out

    g1 = grad(f[:, 0])
    composed = grad(g1[:, 0])[:, 0] + grad(g1[:, 1])[:, 1]
    off, perm, src32, rel = stencil(12)
    c64, _, src, degen = J.weights(off, perm, src32, rel.astype(np.float32), 2, 2)
    assert not degen.any()
    jet = J.jets64(f, off, c64, src)[:, 0]
    return rel_rms(composed, lap), rel_rms(jet[:, 2] + jet[:, 4], lap), rel_rms(g1[:, 0], fx), rel_rms(jet[:, 0], fx)


def test_second_derivatives_converge_and_the_composed_laplacian_does_not():
    coarse, fine = convergence(2500), convergence(10000)
    print(f"MEASURED convergence n 2500: composed {coarse[0]:.4f} quadratic lap {coarse[1]:.4f} linear dx {coarse[2]:.4f} quadratic dx {coarse[3]:.5f}")
    print(f"MEASURED convergence n 10000: composed {fine[0]:.4f} quadratic lap {fine[1]:.4f} linear dx {fine[2]:.4f} quadratic dx {fine[3]:.5f}")
    assert fine[1] <= 0.7 * coarse[1]          # first order in h = n^(−1/2): a factor 0.5
    assert fine[3] <= 0.35 * coarse[3]         # second order: a factor 0.25
    assert coarse[0] >= 0.3 and fine[0] >= 0.3          # the negative control: differentiating the linear fit twice leaves an O(1) error
    note("laplacian error ratio / 0.7", fine[1] / coarse[1] / 0.7)
    note("gradient error ratio / 0.35", fine[3] / coarse[3] / 0.35)


# ------------------------------------------------------------------ manufactured flows
NU, RHO, DT = 0.05, 1.3, 0.01


def flows(pos):
    """name -> (u [n, 3] = (u, v, p), prev [n, 3]): exact solutions of the discrete residual — every field is a quadratic at most."""
    x, y = pos[:, 0], pos[:, 1]
    a, b, c, om, acc = 0.7, -0.4, 0.3, 1.1, np.array([0.3, -0.2])
    zero = np.zeros_like(x)
    pois = np.stack([a * y * y + b * y + c, zero, 2 * NU * RHO * a * x], 1)
    rot = np.stack([-om * y, om * x, RHO * om * om * (x * x + y * y) / 2], 1)
    # a uniform acceleration: U = U0 + acc t, no gradient of velocity, p = 0: (U − prev) / dt = acc needs the body force −acc … as a
    # pressure gradient: p = −ρ acc·x
    now = np.stack([0.5 + zero, -0.1 + zero, -RHO * (acc[0] * x + acc[1] * y)], 1)
    before = now.copy()
    before[:, :2] -= acc * DT
    return {"poiseuille": (pois, pois.copy()), "rotation": (rot, rot.copy()), "acceleration": (now, before)}


def test_manufactured_flows_have_zero_residual_and_wrong_forms_do_not():
    """Plane Poiseuille flow, solid-body rotation and a uniform acceleration are quadratics at most: the fit differentiates them
    exactly, so R and C vanish up to the solve's error — allowed 1e-9 of the largest single term of R (κ <= 1e5 2⁻⁵³ Q² ≈ 1e-9 at
    the pivots these meshes are asserted to have).  Each wrong form of the residual leaves a term of order one."""
    m = mesh_of(2000, 2)
    # the weights are rebuilt from vectors that are EXACT differences of the positions the fields are evaluated at (coordinates
    # rounded to multiples of 2⁻¹²): a vector rounded to fp32 on its own would move a difference by 2⁻²⁴ |∇f| |d|
    pos = np.round(m.pos * 4096) / 4096
    rel = (pos[m.col] - pos[m.row]).astype(np.float32)
    assert np.array_equal(rel.astype(np.float64), pos[m.col] - pos[m.row])
    keep = np.array([i not in m.planted for i in range(m.n)])
    c64, _, src, degen = J.weights(m.off, m.perm, m.src32, rel, 2, 2)
    assert not degen[keep].any()
    for name, (u, prev) in flows(pos).items():
        jet = J.jets64(u, m.off, c64, src)
        r, c = J.residual64(jet, u, prev, 2, NU, DT, RHO, (0, 1), 2)
        scale = max(np.abs(u[:, :2]).max() ** 2 * np.abs(jet[keep][:, :2, :2]).max(), np.abs(jet[keep][:, 2, :2]).max() / RHO,
                    NU * np.abs(jet[keep][:, :2, 2:]).max(), np.abs(u - prev).max() / DT, 1.0)
        worst = max(np.abs(r[keep]).max(), np.abs(c[keep]).max())
        assert worst <= 1e-9 * scale, (name, worst, scale)
        note(f"residual of {name}", worst / (1e-9 * scale))
    caught = {"advection-sign": "rotation", "viscous-factor": "poiseuille", "pressure-sign": "poiseuille", "no-time": "acceleration"}
    for wrong, name in caught.items():
        u, prev = flows(pos)[name]
        r, _ = J.residual64(J.jets64(u, m.off, c64, src), u, prev, 2, NU, DT, RHO, (0, 1), 2, wrong=wrong)
        assert np.abs(r[keep]).max() > 1e-3, wrong


def test_zz_print_the_measured_ratios():
    """Not a check of its own: the measured / allowed ratio of every bound above, for tests/JET_MEASURED.md (pytest -s)."""
    for k, v in sorted(RATIOS.items()):
        print(f"MEASURED {k}: {v:.3f}")
        assert v <= 1.0
