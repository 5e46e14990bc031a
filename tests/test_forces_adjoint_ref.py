"""tests/forces_adjoint_ref.py — the numpy restatement of g4c_body_forces_adjoint — is the transpose of the forward tests/forces_ref.py
restates, on forces_ref's own clouds: two bodies, a ragged mesh, one wall node without in-edges.  No GPU, nothing of the package."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import forces_adjoint_ref as A          # noqa: E402
import forces_ref as FR                 # noqa: E402
import gradient_ref as GR               # noqa: E402

F32, F64 = np.float32, np.float64
NF = 4
CONST = dict(pcol=3, ucol=2, vcol=0, mu=0.0406, p_scale=2.5, p_shift=0.125, u_scale=1.5, v_scale=0.75)


def case(counts=(17, 5), n=180, seed=0):
    pos, wall, label = FR.annulus(n, counts, seed=seed)
    lone = int(wall[len(wall) // 2])
    m = FR.knn_mesh(pos, 6, ragged_seed=3 + seed, lone=lone)
    _, g32, src, degen = GR.weights(m.off, m.perm, m.src32, m.rel, 2, 2)
    assert degen[lone] and np.diff(m.off).min() == 0 and np.diff(m.off).max() == 6
    geo = FR.geometry(pos, nodes=wall, labels=label)
    c = dict(CONST, off=m.off, g=g32, src=src)
    tabs = A.node_tables(geo["items"], geo["body_offsets"], len(pos), m.off, src, g32)
    return pos, geo, c, tabs


def draws(geo, n, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, NF)).astype(F32), rng.standard_normal((geo["n_bodies"], 6)),
            rng.standard_normal((geo["items"].size, 2)).astype(F32))


def identity(x, gF, gw, geo, c, tabs, wrong=None, tables=None):
    """(⟨J x, (gF, gwall)⟩ − ⟨x, Jᵀ(gF, gwall)⟩ in fp64, the rounding of the two sides: 2⁻⁵³ times a few times the magnitudes summed)."""
    n = x.shape[0]
    S, W, _, _ = A.forward64(x, geo, **c)
    S0, W0, _, _ = A.forward64(np.zeros_like(x), geo, **c)
    lhs = A.inner(S - S0, W - W0, gF, gw)
    ca = {k: v for k, v in c.items() if k not in ("p_shift", "src")}
    gx, _ = A.adjoint64(gF, gw, geo, tables or tabs, n, NF, wrong=wrong, **ca)
    rhs = float((x.astype(F64) * gx).sum())
    mag = float((np.abs(x).astype(F64) * A.abs_adjoint(np.abs(gF), np.abs(gw), geo, tabs, n, NF, **ca)).sum())
    return lhs - rhs, 64 * 2.0 ** -53 * mag


def test_the_tables():
    pos, geo, c, tabs = case()
    n, items = len(pos), geo["items"]
    assert tabs["item_body"].tolist() == [0] * 17 + [1] * 5
    for j in range(n):
        own = tabs["own_item"][tabs["own_off"][j]:tabs["own_off"][j + 1]]
        assert own.tolist() == [w for w in range(items.size) if items[w] == j]
    # the in-list of j: the pairs (w, e) with src_e == j, by ascending e (one item per node here: e decides)
    pairs = [(int(e), w) for w in range(items.size) for e in range(c["off"][items[w]], c["off"][items[w] + 1])]
    for j in range(n):
        want = sorted(p for p in pairs if c["src"][p[0]] == j)
        q0, q1 = tabs["in_off"][j], tabs["in_off"][j + 1]
        assert tabs["in_item"][q0:q1].tolist() == [w for _, w in want]
        assert np.array_equal(tabs["in_g"][q0:q1], c["g"][[e for e, _ in want]].reshape(-1, 2))
    assert tabs["in_off"][-1] == len(pairs)


def test_the_forward_is_forces_ref():
    """forward64 is forces_ref.terms + sum_plain up to the fp32 gradient loop: within forces_ref's own bounds."""
    pos, geo, c, tabs = case()
    x, _, _ = draws(geo, len(pos), 1)
    T, wall, G = FR.terms(x, geo, **c)
    S, W, G64, Gm = A.forward64(x.astype(F64), geo, **c)
    deg = np.diff(c["off"])[geo["items"]]
    assert (np.abs(G - G64) <= (deg[:, None] + 3) * A.U * Gm).all()
    ref = A.ForceRef(geo, len(pos), c, wall={"pressure": 1.0, "shear": 1.0})
    eF, eW = ref._forward_errors(x.astype(F64), np.zeros_like(x, F64), Gm, 0 * Gm)
    plain = FR.sum_plain(T, geo["body_offsets"])
    assert (np.abs(ref._total(plain) - ref._total(S)) <= eF + 1e-300).all()
    assert (np.abs(wall.astype(F64) - W) <= eW + 1e-300).all()


@pytest.mark.parametrize("seed", [0, 1])
def test_the_restatement_is_the_transpose(seed):
    pos, geo, c, tabs = case(seed=seed)
    x, gF, gw = draws(geo, len(pos), 10 + seed)
    for a, b in ((gF, gw), (gF, None), (None, gw)):
        diff, rounding = identity(x, np.zeros_like(gF) if a is None else a, np.zeros_like(gw) if b is None else b, geo, c, tabs)
        assert abs(diff) <= rounding, (diff, rounding)
    inviscid = dict(c, mu=0.0)
    diff, rounding = identity(x, gF, gw, geo, inviscid, tabs)
    assert abs(diff) <= rounding


@pytest.mark.parametrize("wrong", A.WRONG)
def test_a_mistake_breaks_the_identity(wrong):
    pos, geo, c, tabs = case()
    x, gF, gw = draws(geo, len(pos), 20)
    tables = A.node_tables(geo["items"], geo["body_offsets"], len(pos), c["off"], c["src"], c["g"], wrong=wrong)
    diff, rounding = identity(x, gF, gw, geo, c, tabs, wrong=wrong, tables=tables)
    assert abs(diff) > 1e6 * rounding, (wrong, diff, rounding)


def test_the_fp32_loop_is_within_its_bound_of_the_fp64_one():
    pos, geo, c, tabs = case()
    _, gF, gw = draws(geo, len(pos), 30)
    ca = {k: v for k, v in c.items() if k not in ("p_shift", "src")}
    for a, b in ((gF, gw), (gF, None), (None, gw), (None, None)):
        g32 = A.adjoint32(a, b, geo, tabs, len(pos), NF, **ca)
        g64, bound = A.adjoint64(a, b, geo, tabs, len(pos), NF, **ca)
        assert g32.dtype == F32 and (np.abs(g32 - g64) <= bound).all()
        assert not g32[:, 1].view(np.int32).any()          # the column nobody names: +0
    assert not A.adjoint32(None, None, geo, tabs, len(pos), NF, **ca).view(np.int32).any()
    far = np.setdiff1d(np.arange(len(pos)), np.concatenate([geo["items"], c["src"][A.item_edges(geo["items"], c["off"])[1]]]))
    assert far.size and not A.adjoint32(gF, gw, geo, tabs, len(pos), NF, **ca)[far].view(np.int32).any()


def test_a_central_difference_of_the_forces_agrees():
    pos, geo, c, tabs = case(counts=(9, 4), n=60)
    n = len(pos)
    x, gF, gw = draws(geo, n, 40)
    ca = {k: v for k, v in c.items() if k not in ("p_shift", "src")}
    gx, _ = A.adjoint64(gF, gw, geo, tabs, n, NF, **ca)

    def phi(z):
        S, W, _, _ = A.forward64(z, geo, **c)
        return A.inner(S, W, gF, gw)

    x64, h = x.astype(F64), 2.0 ** -10          # (φ is affine: the quotient is exact up to the fp64 roundings of φ itself)
    scale = abs(phi(x64)) + 1.0
    for j, f in [(int(geo["items"][0]), c["pcol"]), (int(geo["items"][3]), c["ucol"]), (int(c["src"][c["off"][geo["items"][1]]]), c["vcol"]),
                 (int(geo["items"][-1]), c["vcol"]), (int(geo["items"][2]), 1)]:
        e = np.zeros_like(x64)
        e[j, f] = h
        q = (phi(x64 + e) - phi(x64 - e)) / (2 * h)
        assert abs(q - gx[j, f]) <= 1e3 * 2.0 ** -53 * scale / h, (j, f, q, gx[j, f])


def test_force_ref_gradient_is_the_derivative_of_its_loss():
    pos, geo, c, tabs = case(counts=(9, 4), n=60)
    n = len(pos)
    rng = np.random.default_rng(5)
    pred, target = rng.standard_normal((n, NF)).astype(F32), rng.standard_normal((n, NF)).astype(F32)
    ref = A.ForceRef(geo, n, c, weight=0.7, node_weight=0.3, components=("fx", "fy", "m"), force_scale=0.5, wall={"pressure": 0.2, "shear": 0.4})
    grad, allowed = ref.grad(pred, target)
    assert np.isfinite(grad).all() and (allowed >= 0).all()
    p64, t64, h = pred.astype(F64), target.astype(F64), 2.0 ** -12
    for j, f in [(int(geo["items"][0]), 3), (int(geo["items"][4]), 2), (int(geo["items"][5]), 0), (7, 1)]:
        e = np.zeros_like(p64)
        e[j, f] = h
        q = (ref.loss(p64 + e, t64) - ref.loss(p64 - e, t64)) / (2 * h)          # (the loss is quadratic: a central difference is exact)
        assert abs(q - grad[j, f]) <= 1e-9 * (1 + abs(q)), (j, f, q, grad[j, f])
