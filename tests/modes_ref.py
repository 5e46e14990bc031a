"""numpy restatement of the snapshot-mode launches and an independent route to POD and DMD (test-only).

The three launches (csrc/snapshot_modes.hip) as plain fp64 loops in the orders include/g4c.h states: `mean` adds the selected rows in
slot order, `combine` adds C[i][r] (x_i − mean) in slot order with product and sum rounded separately, `gram` adds the columns one
after the other (the device adds them four at a time within a chunk and the chunks in order: its sum is the same set of terms in
another order, which is what the Gram tests bound; on small integers every order gives the same bits).  `gram` also returns Σ|terms|,
the scale of that bound.

POD and DMD go through a direct SVD of the centred, √w-scaled snapshot matrix — never through a Gram matrix — so they share nothing
with graphs4cfd_amd/modes.py but the definition."""
import numpy as np

F32, F64 = np.float32, np.float64


def rows(x, sel):
    """The selected snapshots of x [rows, L] as fp64 [count, L]."""
    first, stride, count = (0, 1, x.shape[0]) if sel is None else sel
    assert first >= 0 and stride >= 1 and count >= 1 and first + (count - 1) * stride < x.shape[0]
    return np.asarray(x, dtype=F32).reshape(x.shape[0], -1)[first:first + (count - 1) * stride + 1:stride].astype(F64)


def mean(x, sel=None):
    a = rows(x, sel)
    s = np.zeros(a.shape[1], dtype=F64)
    for i in range(a.shape[0]):
        s = s + a[i]
    return s / F64(a.shape[0])


def gram(a, b=None, mean_a=None, mean_b=None, sel_a=None, sel_b=None, w=None):
    """(G [Ma, Mb], Σ_l |terms| [Ma, Mb]), the terms (a_i − mean_a) w (b_j − mean_b) rounded as the device rounds them."""
    if b is None:
        b, mean_b, sel_b = a, mean_a, sel_a
    A, B = rows(a, sel_a), rows(b, sel_b)
    if mean_a is not None:
        A = A - np.asarray(mean_a, dtype=F64).reshape(-1)
    if mean_b is not None:
        B = B - np.asarray(mean_b, dtype=F64).reshape(-1)
    if w is not None:
        A = A * np.asarray(w, dtype=F64).reshape(-1)
    G = np.zeros((A.shape[0], B.shape[0]), dtype=F64)
    S = np.zeros_like(G)
    for l in range(A.shape[1]):
        t = np.multiply.outer(A[:, l], B[:, l])
        G = G + t
        S = S + np.abs(t)
    return G, S


def combine(x, coef, mean=None, sel=None):
    """out [R, L] fp32: Σ_i coef[i][r] (x_i − mean) in slot order, fp64, rounded once."""
    a = rows(x, sel)
    coef = np.asarray(coef, dtype=F64)
    assert coef.shape[0] == a.shape[0]
    if mean is not None:
        a = a - np.asarray(mean, dtype=F64).reshape(-1)
    acc = np.zeros((coef.shape[1], a.shape[1]), dtype=F64)
    for i in range(a.shape[0]):
        acc = acc + coef[i][:, None] * a[i][None, :]
    return acc.astype(F32)


def fix_signs(V):
    """(Columns of V with their largest-magnitude entry — the first on ties — positive, the signs applied)."""
    V = np.array(V, dtype=F64)
    sign = np.ones(V.shape[1])
    for k in range(V.shape[1]):
        if V[int(np.argmax(np.abs(V[:, k]))), k] < 0:
            sign[k] = -1.0
    return V * sign, sign


def pod_svd(x, w=None, centre=True, rank=None, sel=None):
    """POD by the SVD of the centred, √w-scaled snapshots -> dict(singular_values, energy, coefficients [M, R], modes [R, L], mean)."""
    X = rows(x, sel)
    m = X.mean(axis=0) if centre else None
    A = X - m if centre else X
    sw = np.ones(X.shape[1]) if w is None else np.sqrt(np.asarray(w, dtype=F64).reshape(-1))
    U, s, Vt = np.linalg.svd(A * sw, full_matrices=False)
    R = len(s) if rank is None else rank
    U, sign = fix_signs(U[:, :R])
    with np.errstate(divide="ignore", invalid="ignore"):
        modes = np.where(sw > 0, (Vt[:R] * sign[:, None]) / sw, 0.0)
    lam = s ** 2
    return dict(singular_values=s[:R], energy=(lam / lam.sum())[:R], coefficients=U * s[:R], modes=modes, mean=m)


def dmd_svd(x, w=None, rank=None, step=1.0, sel=None):
    """Exact DMD by the SVD of the √w-scaled X₁ -> dict(eigenvalues, frequency, growth, amplitudes, modes [R, L]), by |amplitude|."""
    X = rows(x, sel)
    sw = np.ones(X.shape[1]) if w is None else np.sqrt(np.asarray(w, dtype=F64).reshape(-1))
    A = (X * sw).T                                     # [L, M]
    X1, X2 = A[:, :-1], A[:, 1:]
    U, s, Vh = np.linalg.svd(X1, full_matrices=False)
    R = len(s) if rank is None else rank
    U, s, V = U[:, :R], s[:R], Vh[:R].conj().T
    At = U.T @ X2 @ V / s
    mu, W = np.linalg.eig(At)
    Phi = X2 @ (V / s) @ W
    amp = np.linalg.lstsq(Phi, A[:, 0].astype(complex), rcond=None)[0]
    order = np.argsort(-np.abs(amp), kind="stable")
    mu, Phi, amp = mu[order], Phi[:, order], amp[order]
    with np.errstate(divide="ignore", invalid="ignore"):
        modes = np.where(sw[:, None] > 0, Phi / sw[:, None], 0.0).T
    return dict(eigenvalues=mu, frequency=np.log(mu).imag / (2 * np.pi * step), growth=np.log(mu).real / step, amplitudes=amp, modes=modes)


# ---- the two cases the host and the device tests share

RANK3 = dict(M=12, N=50, nf=3, sigma=(5.0, 2.0, 0.5))
DYNAMICS = dict(M=24, N=40, nf=3, step=0.25,
                mu=(1.01 * np.exp(0.6j), 1.01 * np.exp(-0.6j), 0.97 * np.exp(1.3j), 0.97 * np.exp(-1.3j), 0.99 + 0j))


def weights(N, nf, seed=7):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.5, 1.5, N), np.array([1.0, 2.0, 0.5][:nf])


def rank3_case():
    """Snapshots [M, N, nf] fp32 = mean + Σ_k σ_k u_k φ_k: u orthonormal and orthogonal to ones (so the fp64 mean over time is the
    mean given), φ orthonormal in the w inner product -> (x, w flat, node_weights, field_weights, sigma, u [M, 3], phi [3, L], mean)."""
    c = RANK3
    rng = np.random.default_rng(3)
    nw, fw = weights(c["N"], c["nf"])
    w = (nw[:, None] * fw[None, :]).reshape(-1)
    L = w.size
    q, _ = np.linalg.qr(np.concatenate([np.ones((c["M"], 1)), rng.standard_normal((c["M"], 3))], axis=1))
    u = q[:, 1:]
    p, _ = np.linalg.qr(rng.standard_normal((L, 3)))
    phi = (p / np.sqrt(w)[:, None]).T
    m = rng.standard_normal(L)
    sigma = np.array(c["sigma"])
    x = m + (u * sigma) @ phi
    return x.astype(F32).reshape(c["M"], c["N"], c["nf"]), w, nw, fw, sigma, u, phi, m


def dynamics_case():
    """Snapshots [M, N, nf] fp32 of x_{t+1} = A x_t whose non-zero eigenvalues are DYNAMICS['mu'], rounded to fp32 ->
    (x, w flat, node_weights, field_weights, mu, step)."""
    c = DYNAMICS
    rng = np.random.default_rng(5)
    nw, fw = weights(c["N"], c["nf"])
    w = (nw[:, None] * fw[None, :]).reshape(-1)
    L = w.size
    mu = np.array(c["mu"])
    vec = rng.standard_normal((L, 3)) + 1j * rng.standard_normal((L, 3))
    t = np.arange(c["M"])[:, None]
    x = (2 * (mu[0] ** t * vec[:, 0]).real + 1.5 * (mu[2] ** t * vec[:, 1]).real + (mu[4].real ** t) * vec[:, 2].real)
    return x.astype(F32).reshape(c["M"], c["N"], c["nf"]), w, nw, fw, mu, c["step"]


# What was measured between the Gram route (graphs4cfd_amd/modes.py fed this file's Gram matrices) and the SVD route of this file, and —
# the *_known entries — between the Gram route and the values the cases were built from (tests/MODES_MEASURED.md).  Singular values
# and coefficients are relative to σ_0; everything else is absolute.  A test allows 10 x these.
MEASURED = dict(
    rank3=dict(sigma=1.8e-16, energy=2.6e-15, coefficients=6.5e-16, modes=1.5e-8, sigma_known=9.9e-9, coefficients_known=1.2e-8,
               modes_known=3.4e-7),
    dynamics=dict(mu=8.3e-16, frequency=2.3e-16, growth=3.4e-15, amplitude=2.2e-14, mu_known=5.2e-10, frequency_known=2.6e-10,
                  growth_known=1.6e-9))


def tolerance(case):
    return {k: 10.0 * v for k, v in MEASURED[case].items()}


def dynamics_figures(got, ref, mu, step):
    """The distances of a `DynamicModes` to `dmd_svd`'s result and to the known eigenvalues, mode by mode (matched by eigenvalue)."""
    ev, fr, gr, am = (np.asarray(t.cpu().numpy()) for t in (got.eigenvalues, got.frequency, got.growth, got.amplitudes))
    i, d_known = match(ev, mu)
    j, _ = match(ref["eigenvalues"], mu)
    assert sorted(i.tolist()) == list(range(len(mu))) and sorted(j.tolist()) == list(range(len(mu))), "the eigenvalues were not told apart"
    return dict(mu=np.abs(ev[i] - ref["eigenvalues"][j]).max(), frequency=np.abs(fr[i] - ref["frequency"][j]).max(),
                growth=np.abs(gr[i] - ref["growth"][j]).max(), amplitude=np.abs(np.abs(am[i]) - np.abs(ref["amplitudes"][j])).max(),
                mu_known=d_known.max(), frequency_known=np.abs(fr[i] - np.log(mu).imag / (2 * np.pi * step)).max(),
                growth_known=np.abs(gr[i] - np.log(mu).real / step).max())


def match(found, known):
    """For each known complex value the nearest found one: (indices, distances)."""
    found, known = np.asarray(found), np.asarray(known)
    d = np.abs(found[None, :] - known[:, None])
    return d.argmin(axis=1), d.min(axis=1)


def same_bits(dev, ref, what):
    """A device tensor (moved to the host) and a numpy array of the same dtype hold the same values (−0 equals +0)."""
    got = dev.detach().cpu().numpy()
    assert got.dtype == ref.dtype and got.shape == ref.shape, f"{what}: {got.dtype} {got.shape} vs {ref.dtype} {ref.shape}"
    bad = ~((got == ref) | (np.isnan(got) & np.isnan(ref)))
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ, the first at {tuple(np.argwhere(bad)[0])}: " \
                          f"{got[tuple(np.argwhere(bad)[0])]!r} vs {ref[tuple(np.argwhere(bad)[0])]!r}"
