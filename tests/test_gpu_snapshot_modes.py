"""g4c_snapshot_mean / _gram / _combine (csrc/snapshot_modes.hip) through ops.snapshot_* against the numpy restatement of
tests/modes_ref.py, and `Modes.fit` end to end on the device against the host tests' cases.

Every output and the Gram launch's scratch sit in guard arenas (tests/footprint.py) and every input is frozen: a launch writes its
window, all of it, and nothing else — the scratch included, whose size `snapshot_gram_scratch_bytes` must state exactly.  Shapes walk
the Gram block edge B = 64 (M = 1, 2, 3, B − 1, B, B + 1, 2B + 2), the chunk K = 2048 (L = 1, 63, 64, 65, K − 1, K, K + 1, 2K + 3) and
combine's block of 8 accumulators.

Mean and combine are bit for bit the restatement's loops on any data.  The Gram matrix is bit for bit on small integers (every order
of summation gives the same bits) and, on floats with a common offset of 1e4, within 2 (L + 4) 2^-53 Σ|terms| of the restatement fed
the device's own mean: L − 1 additions in another order on either side, the rounding of the centred, weighted factors and of the
product.  Measured / allowed: tests/MODES_MEASURED.md."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

import modes_ref as R                                      # noqa: E402
import graphs4cfd_amd as gfd                               # noqa: E402
from graphs4cfd_amd import _lib, ops                       # noqa: E402
from footprint import arena, flat_arena, assert_footprint, frozen      # noqa: E402

DEV = torch.device("cuda", 0)
F32, F64 = torch.float32, torch.float64
B, K, RB = _lib.SNAPSHOT_GRAM_BLOCK, _lib.SNAPSHOT_GRAM_CHUNK, _lib.SNAPSHOT_COMBINE_BLOCK
MS = (1, 2, 3, B - 1, B, B + 1, 2 * B + 2)
LS = (1, 63, 64, 65, K - 1, K, K + 1, 2 * K + 3)
WORST = {}                                                 # the largest measured / allowed of the float bound, per test


def draw(kind, rng, rows, L):
    if kind == "int":
        return rng.integers(-8, 9, (rows, L)).astype(np.float32)
    return (rng.standard_normal((rows, L)) + 1e4).astype(np.float32)


def selections(M):
    """(rows of the buffer, selection): every row, and M rows from the third in strides of three (with a row to spare behind)."""
    return ((M, None), (2 + 3 * (M - 1) + 2, (2, 3, M)))


def as_snapshots(x, L, nf):
    """The host array on the device, flat [rows, L] or — the rollout's shape — [rows, L / nf, nf]."""
    t = torch.from_numpy(x).to(DEV)
    return t.view(t.size(0), L // nf, nf) if nf > 1 and L % nf == 0 else t


def dev64(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(DEV)


def launch_mean(x, sel, what):
    L = x.numel() // x.size(0)
    out, whole = flat_arena(L, F64, device=DEV)
    with frozen(x, what=what):
        ops.snapshot_mean(x, sel, out=out)
    assert_footprint(whole, out, what=what)
    return out


def launch_gram(a, b=None, *, what, **kw):
    """One checked launch: out and scratch in arenas, inputs frozen, the scratch exactly `snapshot_gram_scratch_bytes`."""
    L = a.numel() // a.size(0)
    Ma = (kw.get("sel_a") or (0, 1, a.size(0)))[2]
    other = a if b is None else b
    Mb = Ma if b is None else (kw.get("sel_b") or (0, 1, other.size(0)))[2]
    symmetric = b is None or ops._gram_symmetric(a, kw.get("mean_a"), ops._snapshot_sel("t", kw.get("sel_a"), "sel_a", a.size(0)), b,
                                                 kw.get("mean_b"), ops._snapshot_sel("t", kw.get("sel_b"), "sel_b", b.size(0)))
    need = ops.snapshot_gram_scratch_bytes(Ma, Mb, L, symmetric)
    nbi, nbj = -(-Ma // B), -(-Mb // B)
    assert need == 8 * B * B * (nbi * (nbi + 1) // 2 if symmetric else nbi * nbj) * -(-L // K), what
    out, whole = arena(Ma, Mb, F64, device=DEV)
    scratch, swhole = flat_arena(need // 8, F64, device=DEV)
    with frozen(a, b, kw.get("mean_a"), kw.get("mean_b"), kw.get("w"), what=what):
        ops.snapshot_gram(a, b, out=out, scratch=scratch, **kw)
    assert_footprint(whole, out, what=what)
    assert_footprint(swhole, scratch, what=f"{what}, scratch")
    return out


def within(G, ref, S, L, what, key):
    allowed = 2.0 * (L + 4) * 2.0 ** -53 * S
    err = np.abs(G.cpu().numpy() - ref)
    ratio = float((err / np.where(allowed > 0, allowed, 1.0)).max())
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    print(f"{what}: measured / allowed = {ratio:.3f}")
    assert (err <= allowed).all(), f"{what}: |G - G_ref| is {ratio:.3f} of 2 (L + 4) 2^-53 sum|terms|"


@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("M", MS)
def test_mean_is_the_fp64_loop(M, L):
    rng = np.random.default_rng(100 * M + L)
    for kind in ("int", "offset"):
        for rows, sel in selections(M):
            x = draw(kind, rng, rows, L)
            for nf in (1, 3):
                what = f"mean M {M} L {L} {kind} sel {sel} nf {nf}"
                R.same_bits(launch_mean(as_snapshots(x, L, nf), sel, what), R.mean(x, sel), what)


@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("M", MS)
def test_gram_symmetric_form(M, L):
    rng = np.random.default_rng(7 * M + 13 * L)
    wi = rng.integers(1, 4, L).astype(np.float64)
    wf = rng.uniform(0.5, 1.5, L)
    # small integers: bit for bit, uncentred, and centred when M is a power of two and the means are integral
    for rows, sel in selections(M):
        x = draw("int", rng, rows, L)
        first, stride, _ = sel or (0, 1, M)
        centred = M & (M - 1) == 0
        if centred:                                        # the last selected row makes every column sum a multiple of M
            last = first + (M - 1) * stride
            x[last] += ((-R.rows(x, sel).sum(axis=0)) % M).astype(np.float32)
        for w in (None, wi):
            for mean in ((None, R.mean(x, sel)) if centred else (None,)):
                what = f"gram int M {M} L {L} sel {sel} w {w is not None} centred {mean is not None}"
                xd = as_snapshots(x, L, 3 if w is None else 1)
                G = launch_gram(xd, what=what, sel_a=sel, mean_a=dev64(mean), w=dev64(w))
                R.same_bits(G, R.gram(x, mean_a=mean, sel_a=sel, w=w)[0], what)
                assert torch.equal(G, G.t()), f"{what}: not symmetric bit for bit"
    # floats with a common offset: the bound, symmetry, determinism
    for i, (w, centre) in enumerate(((None, False), (wf, False), (None, True), (wf, True))):
        rows, sel = selections(M)[i % 2]
        x = draw("offset", rng, rows, L)
        xd = as_snapshots(x, L, 1)
        what = f"gram float M {M} L {L} sel {sel} w {w is not None} centred {centre}"
        mean = launch_mean(xd, sel, what) if centre else None
        G = launch_gram(xd, what=what, sel_a=sel, mean_a=mean, w=dev64(w))
        ref, S = R.gram(x, mean_a=None if mean is None else mean.cpu().numpy(), sel_a=sel, w=w)
        within(G, ref, S, L, what, "symmetric")
        assert torch.equal(G, G.t()), f"{what}: not symmetric bit for bit"
        again = launch_gram(xd, what=what, sel_a=sel, mean_a=mean, w=dev64(w))
        assert torch.equal(G, again), f"{what}: two runs differ"


@pytest.mark.parametrize("L", (1, 65, K + 1, 2 * K + 3))
@pytest.mark.parametrize("Ma,Mb", ((3, B + 1), (B + 1, 2), (2 * B + 2, B - 1), (1, B), (B, B)))
def test_gram_cross_form(Ma, Mb, L):
    rng = np.random.default_rng(1000 * Ma + 10 * Mb + L)
    w = rng.uniform(0.5, 1.5, L)
    (rows_a, sel_a), (rows_b, sel_b) = selections(Ma)[1], selections(Mb)[0]
    for kind in ("int", "offset"):
        a, b = draw(kind, rng, rows_a, L), draw(kind, rng, rows_b, L)
        if kind == "offset":
            b = b - np.float32(3.0)                        # (two different means)
        ad, bd = as_snapshots(a, L, 1), as_snapshots(b, L, 3)
        what = f"cross {kind} Ma {Ma} Mb {Mb} L {L}"
        if kind == "int":
            G = launch_gram(ad, bd, what=what, sel_a=sel_a, sel_b=sel_b)
            R.same_bits(G, R.gram(a, b, sel_a=sel_a, sel_b=sel_b)[0], what)
            continue
        ma, mb = launch_mean(ad, sel_a, what), launch_mean(bd, sel_b, what)
        assert not torch.equal(ma, mb)
        G = launch_gram(ad, bd, what=what, sel_a=sel_a, sel_b=sel_b, mean_a=ma, mean_b=mb, w=dev64(w))
        ref, S = R.gram(a, b, mean_a=ma.cpu().numpy(), mean_b=mb.cpu().numpy(), sel_a=sel_a, sel_b=sel_b, w=w)
        within(G, ref, S, L, what, "cross")
        assert torch.equal(G, launch_gram(ad, bd, what=what, sel_a=sel_a, sel_b=sel_b, mean_a=ma, mean_b=mb, w=dev64(w))), f"{what}: two runs differ"
    if Ma == Mb:
        # one buffer, two selections: not the symmetric form (every block is computed), and the transposed call is the transpose
        x = draw("int", rng, 2 * Ma, L)
        xd = as_snapshots(x, L, 1)
        G = launch_gram(xd, xd, what="shifted", sel_a=(0, 1, Ma), sel_b=(Ma, 1, Ma))
        R.same_bits(G, R.gram(x, x, sel_a=(0, 1, Ma), sel_b=(Ma, 1, Ma))[0], "one buffer, two selections")
        assert torch.equal(G.t(), launch_gram(xd, xd, what="shifted", sel_a=(Ma, 1, Ma), sel_b=(0, 1, Ma)))


@pytest.mark.parametrize("L", (1, 65, K + 1))
@pytest.mark.parametrize("M", (1, 3, B + 1))
@pytest.mark.parametrize("Rn", (1, RB - 1, RB, RB + 1, 2 * RB + 1))
def test_combine_is_the_fp64_loop(Rn, M, L):
    rng = np.random.default_rng(100 * Rn + 10 * M + L)
    for i, (rows, sel) in enumerate(selections(M)):
        x = draw("offset", rng, rows, L)
        wide = rng.standard_normal((M, Rn + 3))                          # (a window of a wider matrix: the leading dimension is not R)
        coef = wide[:, 1:1 + Rn]
        mean = R.mean(x, sel) + 0.25 if i == 0 else None
        what = f"combine R {Rn} M {M} L {L} sel {sel} mean {mean is not None}"
        xd, cd, md = as_snapshots(x, L, 1), dev64(wide)[:, 1:1 + Rn], dev64(mean)
        out, whole = flat_arena(Rn * L, F32, device=DEV)
        with frozen(xd, cd, md, what=what):
            ops.snapshot_combine(xd, cd, mean=md, sel=sel, out=out.view(Rn, L))
        assert_footprint(whole, out, what=what)
        R.same_bits(out.view(Rn, L), R.combine(x, coef, mean=mean, sel=sel), what)


def test_envelope():
    lib = _lib.load()
    assert lib.g4c_snapshot_gram_scratch_bytes(_lib.SNAPSHOT_MAX_ROWS + 1, 1, 1, 0) == -1
    assert lib.g4c_snapshot_gram_scratch_bytes(2, 3, 1, 1) == -1 and lib.g4c_snapshot_gram_scratch_bytes(1, 1, 0, 0) == -1
    assert ops.snapshot_gram_scratch_bytes(1024, 1024, 2 ** 31 - 1, True) == 8 * B * B * 136 * 2 ** 20
    assert ops.snapshot_gram_scratch_bytes(256, 256, 300000, True) == 8 * B * B * 10 * 147
    with pytest.raises(NotImplementedError):
        ops.snapshot_gram_scratch_bytes(1025, 1025, 10, True)
    # the library's own checks (the wrappers refuse these first): a selection past the buffer, too many rows
    import ctypes as C
    x, out = torch.zeros(4, 8, device=DEV), torch.zeros(8, dtype=F64, device=DEV)
    sel = _lib.g4c_snapshot_sel_t(rows=4, first=2, stride=1, count=3)
    assert lib.g4c_snapshot_mean(x.data_ptr(), C.byref(sel), 8, out.data_ptr(), None) == _lib.EINVAL
    assert b"outside the 4 snapshots" in lib.g4c_last_error()
    sel = _lib.g4c_snapshot_sel_t(rows=2000, first=0, stride=1, count=1025)
    assert lib.g4c_snapshot_gram(x.data_ptr(), None, C.byref(sel), x.data_ptr(), None, C.byref(sel), None, 1, out.data_ptr(), 1025,
                                 out.data_ptr(), None) == _lib.EUNSUPPORTED
    assert lib.g4c_snapshot_combine(x.data_ptr(), None, C.byref(sel), out.data_ptr(), 1, 1, 2 ** 31, x.data_ptr(), None) == _lib.EUNSUPPORTED


# ---- end to end on the device: the host tests' cases, within the tolerances recorded for them

def test_rank3_field_on_the_device():
    x, w, nw, fw, sigma, u, phi, m = R.rank3_case()
    xd = torch.from_numpy(x).to(DEV)
    spec = gfd.Modes(rank=3, node_weights=torch.from_numpy(nw), field_weights=torch.from_numpy(fw))
    got = spec.fit(xd)
    flat = x.reshape(x.shape[0], -1)
    ref = R.pod_svd(flat, w=w, rank=3)
    tol, s0, M = R.tolerance("rank3"), sigma[0], x.shape[0]
    R.same_bits(got.mean.reshape(-1), R.mean(flat), "mean")
    sv, co = got.singular_values.numpy(), got.coefficients.numpy()
    modes = got.modes.cpu().numpy().reshape(3, -1).astype(np.float64)
    fig = dict(sigma=np.abs(sv - ref["singular_values"]).max() / s0, energy=np.abs(got.energy.numpy() - ref["energy"]).max(),
               coefficients=np.abs(co - ref["coefficients"]).max() / s0, modes=np.abs(modes - ref["modes"]).max(),
               sigma_known=np.abs(sv - sigma).max() / s0, coefficients_known=np.abs(np.abs(co) - np.abs(u * sigma)).max() / s0,
               modes_known=np.abs(np.abs(modes) - np.abs(phi)).max())
    orth = np.abs((modes * w) @ modes.T - np.eye(3)).max()
    print("rank3 on the device (measured, allowed):", {k: (float(v), tol[k]) for k, v in fig.items()}, "orthonormality", orth, 16 * M * 2.0 ** -24)
    for k, v in fig.items():
        assert v <= tol[k], f"{k}: {v:.3e} > {tol[k]:.3e}"
    assert orth <= 16 * M * 2.0 ** -24
    assert got.modes.dtype == F32 and tuple(got.modes.shape) == (3,) + x.shape[1:] and got.mean.dtype == F64
    # the modes are the combine launch on V / sigma, bit for bit
    R.same_bits(got.modes.view(3, -1), R.combine(flat, got._combine.numpy(), mean=R.mean(flat)), "modes")
    # the columns layout is the same data: the same bits
    cols = spec.fit(xd.permute(1, 0, 2).reshape(x.shape[1], -1).contiguous(), layout="columns")
    assert torch.equal(cols.gram, got.gram) and torch.equal(cols.mean, got.mean) and torch.equal(cols.modes, got.modes)
    # projecting the fit's own snapshots gives its coefficients; three modes rebuild a rank-3 field to fp32 rounding
    assert np.abs(got.project(xd).numpy() - co).max() <= tol["coefficients"] * s0
    assert np.abs(got.project(xd[2:5]).numpy() - co[2:5]).max() <= tol["coefficients"] * s0
    rebuilt = got.reconstruct()
    assert rebuilt.dtype == F32 and rebuilt.shape == xd.shape
    assert float((rebuilt - xd).abs().max()) <= 8 * 2.0 ** -24 * float(xd.abs().max())
    assert float((got.reconstruct(1) - xd).abs().max()) > 0.01
    # a subspace against itself: all ones; against the first two of its modes: ones; the third mode alone against the first two: zero
    assert np.abs(got.alignment(got).numpy() - 1.0).max() <= 64 * 2.0 ** -52
    two = gfd.Modes(rank=2, node_weights=torch.from_numpy(nw), field_weights=torch.from_numpy(fw)).fit(xd)
    assert np.abs(got.alignment(two).numpy() - 1.0).max() <= 64 * 2.0 ** -52
    # a field left out by a zero weight has no part in the Gram matrix
    fw0 = fw.copy()
    fw0[2] = 0.0
    out = gfd.Modes(rank=3, node_weights=torch.from_numpy(nw), field_weights=torch.from_numpy(fw0)).fit(xd)
    ref0, S0 = R.gram(flat, mean_a=R.mean(flat), w=(nw[:, None] * fw0[None, :]).reshape(-1))
    assert (np.abs(out.gram.numpy() - ref0) <= 2.0 * (flat.shape[1] + 4) * 2.0 ** -53 * S0).all()


def test_linear_dynamics_on_the_device():
    x, w, nw, fw, mu, step = R.dynamics_case()
    xd = torch.from_numpy(x).to(DEV)
    flat = x.reshape(x.shape[0], -1)
    kw = dict(node_weights=torch.from_numpy(nw), field_weights=torch.from_numpy(fw), dt=step, dmd=True, rank=5)
    got = gfd.Modes(centre=False, **kw).fit(xd).dmd
    ref = R.dmd_svd(flat, w=w, rank=5, step=step)
    fig, tol = R.dynamics_figures(got, ref, mu, step), R.tolerance("dynamics")
    print("dynamics on the device (measured, allowed):", {k: (float(v), tol[k]) for k, v in fig.items()})
    for k, v in fig.items():
        assert v <= tol[k], f"{k}: {v:.3e} > {tol[k]:.3e}"
    # DMD ignores centre: one more launch, the same uncentred Gram matrix, the same dynamic modes
    both = gfd.Modes(centre=True, **kw).fit(xd)
    assert torch.equal(both.dmd.gram, got.gram) and both.mean is not None and not torch.equal(both.gram, got.gram)
    assert torch.allclose(both.dmd.eigenvalues, got.eigenvalues, rtol=0, atol=tol["mu"])
    # the dynamic modes against the SVD route's, mode by mode: a dynamic mode is defined up to a complex factor, which a projection
    # takes out; what is left is the fp32 rounding of the stored real and imaginary parts (2^-24 each) and of the snapshots, with a
    # margin of 64 for the conditioning of the five-mode basis
    assert got.modes.dtype == torch.complex64 and tuple(got.modes.shape) == (5,) + x.shape[1:]
    i, _ = R.match(got.eigenvalues.numpy(), mu)
    j, _ = R.match(ref["eigenvalues"], mu)
    a = got.modes.cpu().numpy().reshape(5, -1)[i]
    b = ref["modes"][j]
    for p, q in zip(a, b):
        c = np.vdot(q, p) / np.vdot(q, q)
        print("dynamic mode against the SVD route's, relative:", np.abs(p - c * q).max() / np.abs(p).max(), "allowed", 64 * 2.0 ** -24)
        assert np.abs(p - c * q).max() <= 64 * 2.0 ** -24 * np.abs(p).max()
    assert both.dmd.dominant() == got.dominant() and abs(complex(got.eigenvalues[got.dominant()]) - mu[0]) <= tol["mu_known"]


def test_zz_report():
    print("largest measured / allowed of the Gram bound:", WORST)
