"""The restatement of the mesh operator's adjoint (tests/adjoint_op_ref.py) is the transpose of the restatement of the forward
(tests/gradient_ref.py): on the ragged meshes ⟨D x, y⟩ = ⟨x, Dᵀ y⟩ in fp64 up to the rounding of the two sums, and each deliberate
mistake (`wrong=`) breaks the identity by orders of magnitude.  Host only."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import adjoint_op_ref as A          # noqa: E402
import gradient_ref as R            # noqa: E402

NAMES = {2: ("div", "vort", "grad:2"), 3: ("div", "vort")}


@functools.lru_cache(maxsize=None)
def case(dim):
    m = R.ragged_mesh(300, dim).shuffled(11)
    g32, src = R.weights(m.off, m.perm, m.src32, m.rel, dim, 2)[1:3]
    prog = R.program(NAMES[dim], dim, 3)
    rng = np.random.default_rng(7 + dim)
    x = rng.standard_normal((m.n, 3)).astype(np.float32)
    y = rng.standard_normal((m.n, len(prog))).astype(np.float32)
    return m, g32, src, prog, x, y


def residual(dim, wrong=None):
    """(|⟨D x, y⟩ − ⟨x, Dᵀ y⟩|, the fp64 rounding of the two sums: 2⁻⁵³ per operation on Σ|terms| of either side)."""
    m, g32, src, prog, x, y = case(dim)
    dx, dmag = R.derived64(x, m.off, g32, src, prog)
    gx, gmag, n_add = A.adjoint64(y, m.off, g32, src, prog, 3, wrong=wrong, row=m.row)
    lhs, rhs = float((dx * y.astype(np.float64)).sum()), float((x.astype(np.float64) * gx).sum())
    terms = float((dmag * np.abs(y)).sum() + (np.abs(x) * gmag).sum())
    ops = m.max_deg + int(n_add.max()) + 3 * m.n + 16          # every term's own chain, then the sums over 3 n outputs
    return abs(lhs - rhs), ops * 2.0 ** -53 * terms, abs(lhs)


@pytest.mark.parametrize("dim", [2, 3])
def test_the_restatement_is_the_transpose_of_the_forward(dim):
    err, allowed, size = residual(dim)
    assert err <= allowed and allowed < 1e-9 * size, (err, allowed, size)


@pytest.mark.parametrize("wrong", A.WRONG)
@pytest.mark.parametrize("dim", [2, 3])
def test_each_mistake_breaks_the_identity(dim, wrong):
    err, allowed, size = residual(dim, wrong)
    assert err > 1e6 * allowed and err > 1e-3 * size, (wrong, err, allowed, size)


@pytest.mark.parametrize("dim", [2, 3])
def test_fp32_sits_within_its_bound_of_fp64_and_unused_fields_are_zero(dim):
    m, g32, src, prog, x, y = case(dim)
    gx64, mag, n_add = A.adjoint64(y, m.off, g32, src, prog, 5)
    gx32 = A.adjoint32(y, m.off, g32, src, prog, 5)
    assert gx32.dtype == np.float32 and R.within(gx32, gx64, A.bound(mag, n_add, prog)) <= 1.0
    assert not gx32[:, 3:].any() and not np.signbit(gx32[:, 3:]).any() and gx32[:, :2].any()
    senders = np.bincount(src, minlength=m.n)
    assert (np.diff(m.off) == 0).any() and senders.max() > senders.min()          # empty in-segments, uneven out-degrees
    assert np.array_equal(n_add[:, 0], dim * (senders + np.diff(m.off)))


def test_tables():
    m = A.hub_mesh()
    g32, src = R.weights(m.off, m.perm, m.src32, m.rel, 2, 2)[1:3]
    out_off, out_perm = A.sender_csr(src, m.n)
    assert out_off[1] - out_off[0] >= 599 and np.array_equal(src[m.off[1:-1]], np.zeros(m.n - 1))          # every first in-edge from node 0
    pairs = np.stack([src, A.dst_of(m.off)], 1)
    assert len(np.unique(pairs, axis=0)) < len(pairs)                                                        # duplicated edges
    assert all(np.all(np.diff(out_perm[out_off[j]:out_off[j + 1]]) > 0) for j in range(m.n))                 # ascending within a sender
    off, g, s, _ = A.lattice_tables(1000, 31, 2, np.random.default_rng(0))
    assert off[-1] == s.size and s.min() >= 0 and s.max() < 1000 and np.diff(off).min() == 2
    assert A.max_picks(R.program(("div", "div", "grad:0"), 2, 2)) == 3
