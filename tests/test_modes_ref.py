"""The host algebra of graphs4cfd_amd/modes.py (`pod_from_gram`, `dmd_from_gram`, `principal_cosines`, `Modes.from_gram`) fed the Gram
matrices of the numpy restatement (tests/modes_ref.py), against that file's independent route — a direct SVD of the centred, √w-scaled
snapshots — and against the values the cases were built from.  No GPU, no library.

Tolerances: 10 x what was measured between the two routes on the CPU (tests/MODES_MEASURED.md; `modes_ref.MEASURED`), and, against
the values the cases were built from, 10 x what was measured there — that distance is the fp32 rounding of the snapshots, which
both routes share."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import modes_ref as R                                      # noqa: E402
import graphs4cfd_amd as gfd                               # noqa: E402
from graphs4cfd_amd import modes as Mo                     # noqa: E402

T = torch.from_numpy


def test_restatement_launches_on_hand_values():
    """The restatement itself, on values small enough to do by hand (its negative control: a wrong order or a dropped mean shows)."""
    x = np.array([[1, 2], [3, 6], [5, 1], [7, 0]], dtype=np.float32)
    assert R.mean(x).tolist() == [4.0, 2.25] and R.mean(x, (1, 2, 2)).tolist() == [5.0, 3.0]
    G, S = R.gram(x, sel_a=(0, 2, 2))
    assert G.tolist() == [[5.0, 7.0], [7.0, 26.0]] and S.tolist() == G.tolist()
    G, _ = R.gram(x, x, mean_a=np.array([1.0, 1.0]), sel_a=(0, 1, 2), sel_b=(2, 1, 2), w=np.array([2.0, 1.0]))
    assert G.tolist() == [[0 * 2 * 5 + 1 * 1, 0 * 2 * 7 + 0], [2 * 2 * 5 + 5 * 1, 2 * 2 * 7 + 0]]
    out = R.combine(x, np.array([[1.0, 0.5], [-1.0, 0.5]]), mean=np.array([1.0, 0.0]), sel=(1, 2, 2))
    assert out.dtype == np.float32 and out.tolist() == [[2.0 - 6.0, 6.0 - 0.0], [1.0 + 3.0, 3.0 + 0.0]]


def rank3_parts():
    x, w, nw, fw, sigma, u, phi, m = R.rank3_case()
    flat = x.reshape(x.shape[0], -1)
    mean = R.mean(flat)
    G, _ = R.gram(flat, mean_a=mean, w=w)
    return flat, w, sigma, u, phi, mean, G


def test_rank3_field_recovers_its_modes():
    flat, w, sigma, u, phi, mean, G = rank3_parts()
    got = gfd.Modes(rank=3).from_gram(T(G))
    ref = R.pod_svd(flat, w=w, rank=3)
    tol, s0 = R.tolerance("rank3"), sigma[0]
    sv, co = got.singular_values.numpy(), got.coefficients.numpy()
    modes = R.combine(flat, got._combine.numpy(), mean=mean).astype(np.float64)
    fig = dict(sigma=np.abs(sv - ref["singular_values"]).max() / s0, energy=np.abs(got.energy.numpy() - ref["energy"]).max(),
               coefficients=np.abs(co - ref["coefficients"]).max() / s0, modes=np.abs(modes - ref["modes"]).max(),
               sigma_known=np.abs(sv - sigma).max() / s0, coefficients_known=np.abs(np.abs(co) - np.abs(u * sigma)).max() / s0,
               modes_known=np.abs(np.abs(modes) - np.abs(phi)).max())
    print("rank3 (measured, allowed):", {k: (float(v), tol[k]) for k, v in fig.items()})
    for k, v in fig.items():
        assert v <= tol[k], f"{k}: {v:.3e} > {tol[k]:.3e}"
    # (centring makes the Gram matrix singular: its null eigenvalue is dropped, with whatever else of the rounding noise is unresolved)
    assert 1 <= got.dropped <= flat.shape[0] - 3 and got.singular_values.numel() == 3
    assert np.allclose(got.cumulative_energy.numpy(), np.cumsum(got.energy.numpy()), rtol=0, atol=1e-15)
    # the sign convention: the largest-magnitude entry of every column of V is positive
    V = got._V.numpy()
    assert all(V[np.argmax(np.abs(V[:, k])), k] > 0 for k in range(3))
    # orthonormal in the w inner product, to the fp32 rounding of the stored modes
    assert np.abs((modes * w) @ modes.T - np.eye(3)).max() <= 16 * flat.shape[0] * 2.0 ** -24


def test_energy_picks_the_smallest_rank_that_reaches_it():
    *_, G = rank3_parts()                                  # energies 25, 4, 0.25 of 29.25: 0.8547, 0.1368, 0.0085
    for energy, rank in ((0.5, 1), (0.85, 1), (0.86, 2), (0.99, 2), (0.9999, 3)):
        got = gfd.Modes(energy=energy).from_gram(T(G))
        assert got.singular_values.numel() == rank, (energy, rank, got.cumulative_energy)
        assert float(got.cumulative_energy[-1]) >= energy * (1 - 1e-15)
    assert gfd.Modes(energy=0.9999, rank=2).from_gram(T(G)).singular_values.numel() == 2
    full = gfd.Modes().from_gram(T(G))                     # the rounding noise of fp32 snapshots is resolved: nothing asked, nothing cut
    assert full.singular_values.numel() + full.dropped == G.shape[0]
    assert float(full.cumulative_energy[-1]) == pytest.approx(1.0, abs=1e-14)


def test_exact_rank_two_drops_four():
    """Six snapshots of exact rank 2 on small integers: the Gram matrix is exact, and what eigh leaves of the four null eigenvalues
    is below M 2^-52 lambda_0 — dropped whatever was asked for."""
    rng = np.random.default_rng(11)
    p, q = rng.integers(-4, 5, 20), rng.integers(-4, 5, 20)
    c = np.array([[1, 0], [0, 1], [1, 1], [2, -1], [-1, 3], [3, 2]])
    x = (c[:, :1] * p + c[:, 1:] * q).astype(np.float32)
    G, _ = R.gram(x)
    for spec in (gfd.Modes(centre=False), gfd.Modes(centre=False, rank=5), gfd.Modes(centre=False, energy=1.0)):
        got = spec.from_gram(T(G))
        assert got.dropped == 4 and got.singular_values.numel() == 2, (got.dropped, got.singular_values)
    ref = np.linalg.svd(x.astype(np.float64), compute_uv=False)[:2]
    assert np.abs(got.singular_values.numpy() - ref).max() <= 1e-13 * ref[0]
    with pytest.raises(ValueError, match="no positive eigenvalue"):
        gfd.Modes().from_gram(torch.zeros(3, 3, dtype=torch.float64))


def test_linear_dynamics_recovers_its_eigenvalues():
    x, w, nw, fw, mu, step = R.dynamics_case()
    flat = x.reshape(x.shape[0], -1)
    G, _ = R.gram(flat, w=w)
    got = gfd.Modes(rank=5, dmd=True, centre=False, dt=step).from_gram(T(G), T(G)).dmd
    ref = R.dmd_svd(flat, w=w, rank=5, step=step)
    fig = R.dynamics_figures(got, ref, mu, step)
    tol = R.tolerance("dynamics")
    print("dynamics (measured, allowed):", {k: (float(v), tol[k]) for k, v in fig.items()})
    for k, v in fig.items():
        assert v <= tol[k], f"{k}: {v:.3e} > {tol[k]:.3e}"
    # sorted by amplitude; the dominant mode is the growing pair's member above the axis
    amp = got.amplitudes.abs().numpy()
    assert (np.diff(amp) <= 2.0 ** -20 * amp[0]).all()      # (the members of a conjugate pair are equal up to rounding)
    assert [float(f) > 0 for f in got.frequency[:4]] == [True, False, True, False]       # of a pair, the member above the axis first
    k = got.dominant()
    assert abs(complex(got.eigenvalues[k]) - mu[0]) <= tol["mu_known"] and float(got.frequency[k]) > 0 and float(got.growth[k]) > 0
    # dt and stride scale time: the same Gram matrix read with twice the step halves frequency and growth
    spec2 = gfd.Modes(rank=5, dmd=True, centre=False, dt=step, stride=2)
    two = spec2.from_gram(T(G), T(G)).dmd
    assert torch.allclose(two.eigenvalues, got.eigenvalues, rtol=0, atol=1e-13)
    assert torch.allclose(two.frequency * 2, got.frequency, rtol=1e-15, atol=0) and torch.allclose(two.growth * 2, got.growth, rtol=1e-15, atol=0)


def test_alignment_of_planes():
    rng = np.random.default_rng(2)
    e, _ = np.linalg.qr(rng.standard_normal((30, 3)))
    e = e.T
    for theta in (0.0, 0.3, 1.0, np.pi / 2):
        a = (rng.standard_normal((5, 2)) @ e[:2]).astype(np.float32)
        b = (rng.standard_normal((4, 2)) @ np.stack([e[0], np.cos(theta) * e[1] + np.sin(theta) * e[2]])).astype(np.float32)
        pa, pb = Mo.pod_from_gram(T(R.gram(a)[0]), rank=2), Mo.pod_from_gram(T(R.gram(b)[0]), rank=2)
        cos = Mo.principal_cosines(pa, T(R.gram(a, b)[0]), pb).numpy()
        # the planes are spanned by fp32-rounded vectors: the angle is exact to that rounding
        assert np.abs(cos - np.array([1.0, abs(np.cos(theta))])).max() <= 64 * 2.0 ** -24, (theta, cos)
        own = Mo.principal_cosines(pa, T(R.gram(a)[0]), pa).numpy()
        assert np.abs(own - 1.0).max() <= 64 * 2.0 ** -52, own


def test_equal_gram_matrices_give_equal_parts():
    *_, G = rank3_parts()
    a, b = Mo.pod_from_gram(T(G), rank=3), Mo.pod_from_gram(T(G.copy()), rank=3)
    assert all(torch.equal(a[k], b[k]) for k in ("singular_values", "V", "combine", "coefficients"))
    flip = Mo._fix_signs(-a["V"])
    assert torch.equal(flip, a["V"])
    tie = Mo._fix_signs(torch.tensor([[-0.5, 0.5], [0.5, 0.5], [0.5, -0.5]], dtype=torch.float64))      # the first of equal magnitudes decides
    assert tie[0, 0] > 0 and tie[0, 1] > 0
