"""tests/forces_ref.py — the numpy restatement of gfd.BodyForces and g4c_body_forces — against analytic cases, on the host with numpy
only: the areas of a loop sum to exactly zero, a constant pressure exerts no force, a linear pressure the force −∇p A and no moment,
a linear shear the wall shear of its constant stress and no net force.  Every tolerance is a rounding bound worked out from the data
(the records' 2 (n + 4) 2⁻⁵³ Σ|terms| for a sum, tests/gradient_ref.py's bounds for the fp32 gradient); measured / allowed is printed,
the largest ratios are in tests/FORCES_MEASURED.md, and a ratio above 1 fails."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import forces_ref as R                                   # noqa: E402
import gradient_ref as GR                                # noqa: E402

F32, F64 = np.float32, np.float64
PENTAGON_CW = np.array([[0.0, 1.0], [1.25, 0.25], [0.75, -1.0], [-0.5, -0.75], [-1.0, 0.5]], dtype=F32)      # clockwise


def polygons():
    """name -> geometry: a circle of 64 points, an ellipse of 97, a 5-gon given clockwise through loops=."""
    out = {}
    for name, pos in (("circle64", R.ring(64)), ("ellipse97", R.ring(97, 0.75, 0.4, 0.25, (0.25, -0.125)))):
        shuffle = np.random.default_rng(len(pos)).permutation(len(pos))
        out[name] = (pos[shuffle], R.geometry(pos[shuffle], nodes=np.arange(len(pos))))
    out["pentagon-cw"] = (PENTAGON_CW, R.geometry(PENTAGON_CW, loops=[np.arange(5)]))
    return out


POLY = polygons()


def ratio(err, allowed, what):
    err, allowed = np.abs(np.asarray(err, dtype=F64)), np.asarray(allowed, dtype=F64)
    with np.errstate(all="ignore"):
        r = float(np.where(allowed > 0, err / allowed, np.where(err > 0, np.inf, 0.0)).max())
    print(f"{what}: measured / allowed = {r:.3f}")
    assert r <= 1.0, f"{what}: measured / allowed = {r}"
    return r


@pytest.mark.parametrize("name", list(POLY))
def test_the_areas_of_a_loop_sum_to_exactly_zero(name):
    pos, geo = POLY[name]
    assert geo["area"].sum(0).tolist() == [0.0, 0.0] and np.cumsum(geo["area"], 0)[-1].tolist() == [0.0, 0.0]
    xy = pos.astype(F64)[geo["items"]]
    assert R.shoelace(xy) > 0                                       # counter-clockwise, whatever was given
    nxt = np.roll(xy, -1, 0)
    edge = nxt - xy                                                 # the area vector is the mean of the two edges' outward normals
    normal = np.stack([edge[:, 1], -edge[:, 0]], axis=1)
    assert np.array_equal(geo["area"], 0.5 * (normal + np.roll(normal, 1, 0)))
    assert np.all((geo["area"] * (xy - R.polygon_centroid(xy))).sum(1) > 0)          # out of the body (these bodies are star-shaped)
    assert np.abs(np.hypot(geo["unit"][:, 0], geo["unit"][:, 1]) - 1.0).max() <= 2.0 ** -52
    if name == "pentagon-cw":
        assert geo["items"].tolist() == [4, 3, 2, 1, 0]
    else:
        assert np.all(np.diff(geo["angle"]) > 0) and sorted(geo["items"].tolist()) == list(range(len(pos)))


@pytest.mark.parametrize("name", list(POLY))
def test_a_constant_pressure_exerts_no_force(name):
    pos, geo = POLY[name]
    x = np.full((len(pos), 3), 1.7, F32)
    T, wall, _ = R.terms(x, geo, pcol=2, p_scale=3.0, p_shift=0.125)
    assert np.array_equal(wall[:, 0], np.full(len(pos), F32(F64(3.0) * F64(F32(1.7)) + 0.125))) and not wall[:, 1].any()
    for label, S in (("plain", R.sum_plain(T, geo["body_offsets"])), ("tree", R.sum_tree(T, geo["body_offsets"]))):
        ratio(S[:, :2], R.sum_bound(T, geo["body_offsets"])[:, :2], f"{name}, constant pressure, force, {label} sum")
        assert not S[:, 2:4].any() and not S[:, 5].any()


@pytest.mark.parametrize("name", list(POLY))
def test_a_linear_pressure_gives_minus_gradient_times_area_and_no_moment(name):
    """The force on every polygon; the moment about the rule's own centroid (forces_ref's docstring) on every polygon and, on the
    circle — a regular polygon up to the rounding of its vertices to fp32 —, about the polygon's area centroid too."""
    pos, _ = POLY[name]
    a, b, c = 1.5, -0.75, 0.3
    xy = pos.astype(F64)
    p64 = a * xy[:, 0] + b * xy[:, 1] + c
    x = np.zeros((len(pos), 3), F32)
    x[:, 2] = p64.astype(F32)
    kw = dict(nodes=np.arange(len(pos))) if name != "pentagon-cw" else dict(loops=[np.arange(5)])
    loop = R.geometry(pos, **kw)
    poly = xy[loop["items"]]
    A = R.shoelace(poly)
    centres = {"lumped": R.lumped_centroid(poly, loop["area"])}
    if name == "circle64":
        centres["polygon"] = R.polygon_centroid(poly)
    for which, centre in centres.items():
        geo = R.geometry(pos, centre=centre, **kw)
        T, _, _ = R.terms(x, geo, pcol=2)
        it, ar, arm = geo["items"], np.abs(geo["area"]), np.abs(geo["arm"])
        # the pressure is rounded to fp32 once (2⁻²⁴ |p| per node), then the sum's own bound
        rounding = 2.0 ** -24 * np.abs(p64[it])
        allowed_f = (rounding[:, None] * ar).sum(0) + R.sum_bound(T, geo["body_offsets"])[0, :2] + 4 * 2.0 ** -53 * abs(A) * np.abs([a, b])
        allowed_m = (rounding * (arm[:, 0] * ar[:, 1] + arm[:, 1] * ar[:, 0])).sum() + R.sum_bound(T, geo["body_offsets"])[0, 4]
        if which == "polygon":
            # a regular polygon's area vectors are radial; its vertices were rounded to fp32: each coordinate moved by <= 2⁻²⁴ R, so
            # |δr| and |δa| <= 2⁻²³ R and |r × a| <= 2⁻²³ R (|r| + |a|) per item — and the centroid moved by no more than a vertex did
            r = np.hypot(geo["arm"][:, 0], geo["arm"][:, 1])
            allowed_m += 2.0 ** -23 * (np.abs(p64[it]) * r * (r + np.hypot(ar[:, 0], ar[:, 1]))).sum() + 2.0 ** -23 * r.max() * np.hypot(a, b) * abs(A)
        for label, S in (("plain", R.sum_plain(T, geo["body_offsets"])), ("tree", R.sum_tree(T, geo["body_offsets"]))):
            ratio(S[0, :2] - (-np.array([a, b]) * A), allowed_f, f"{name}, linear pressure, force, {label} sum, centre {which}")
            ratio(S[0, 4], allowed_m, f"{name}, linear pressure, moment, {label} sum, centre {which}")
    # the rule's centroid and the polygon's agree to O(h²): a wrong formula for either is off by O(1)
    h = np.hypot(*(np.roll(poly, -1, 0) - poly).T).max()
    assert np.abs(centres["lumped"] - R.polygon_centroid(poly)).max() <= h * h


@pytest.fixture(scope="module")
def shear_mesh():
    pos, wall, label = R.annulus(300, (48,), seed=2)
    pos = (np.round(pos.astype(F64) * 4096.0) / 4096.0).astype(F32)          # on a grid of 2⁻¹²: every edge vector is exact in fp32, so the
    #                                                                          fp64 weights reproduce a linear field to fp64 rounding
    mesh = R.knn_mesh(pos, 6, ragged_seed=5)
    g64, g32, src, degen = GR.weights(mesh.off, mesh.perm, mesh.src32, mesh.rel, 2, 2)
    assert not degen[wall].any()
    return dict(pos=pos, wall=wall, mesh=mesh, g64=g64, g=g32, src=src, geo=R.geometry(pos, nodes=wall))


def test_a_linear_shear_gives_its_wall_shear_and_no_net_viscous_force(shear_mesh):
    m, geo = shear_mesh, shear_mesh["geo"]
    gamma, mu = 2.0, 0.375                                          # u = 2 y is exact in fp32: the data carry no rounding of their own
    x = np.zeros((len(m["pos"]), 3), F32)
    x[:, 0] = F32(gamma) * m["pos"][:, 1]
    x[:, 2] = 1.0
    T, wall, G = R.terms(x, geo, pcol=2, mu=mu, off=m["mesh"].off, g=m["g"], src=m["src"])
    it, nx, ny = geo["items"], geo["unit"][:, 0], geo["unit"][:, 1]
    tx, ty = -ny, nx
    # the exact-weights gradient of the linear field is (0, γ): what is left is the weights' rounding and the fp32 sum
    dG = np.concatenate([R.gradient_bound(x, m["mesh"], m["g64"], m["g"], m["src"], 0)[it], R.gradient_bound(x, m["mesh"], m["g64"], m["g"], m["src"], 1)[it]], axis=1)
    off = m["mesh"].off.astype(np.int64)
    node = np.repeat(np.arange(off.size - 1), np.diff(off))
    exact64 = np.zeros((off.size - 1, 2))
    np.add.at(exact64, node, m["g64"] * (x[m["src"], 0].astype(F64) - x[node, 0].astype(F64))[:, None])
    exact64 = exact64[it]
    slack = np.abs(exact64 - np.array([0.0, gamma])).max()          # fp64 weights on a linear field: exact to fp64 rounding
    assert slack <= 1e-10
    ratio(G.astype(F64) - np.array([0.0, gamma, 0.0, 0.0]), dG + slack, "linear shear, the four gradient numbers")
    want = mu * gamma * (tx * ny + ty * nx)
    d_sxx, d_sxy, d_syy = 2 * dG[:, 0], dG[:, 1] + dG[:, 2], 2 * dG[:, 3]
    allowed = mu * ((np.abs(tx * nx) * d_sxx + np.abs(ty * nx) * d_sxy) + (np.abs(tx * ny) * d_sxy + np.abs(ty * ny) * d_syy))
    allowed = allowed + 2.0 ** -24 * np.abs(want) + 16 * 2.0 ** -53 * mu * gamma + mu * 4 * slack
    ratio(wall[:, 1].astype(F64) - want, allowed, "linear shear, wall shear")
    ar = np.abs(geo["area"])
    allowed_f = mu * np.array([(d_sxx * ar[:, 0] + d_sxy * ar[:, 1]).sum(), (d_sxy * ar[:, 0] + d_syy * ar[:, 1]).sum()])
    allowed_f = allowed_f + R.sum_bound(T, geo["body_offsets"])[0, 2:4] + mu * 4 * slack * ar.sum()
    for label, S in (("plain", R.sum_plain(T, geo["body_offsets"])), ("tree", R.sum_tree(T, geo["body_offsets"]))):
        ratio(S[0, 2:4], allowed_f, f"linear shear, net viscous force, {label} sum")


def test_the_tree_sum_is_the_plain_sum_within_the_bound_and_exact_on_integers():
    rng = np.random.default_rng(3)
    for counts in ((3,), (5, 63), (64, 65, 255), (256, 257, 1000)):
        off = np.concatenate([[0], np.cumsum(counts)])
        T = rng.standard_normal((off[-1], 6)) * 10.0 ** rng.integers(-3, 4, (off[-1], 6))
        ratio(R.sum_tree(T, off) - R.sum_plain(T, off), 2 * R.sum_bound(T, off), f"tree against plain, bodies of {counts}")
        Ti = rng.integers(-1000, 1000, (off[-1], 6)).astype(F64)
        assert np.array_equal(R.sum_tree(Ti, off), R.sum_plain(Ti, off))
    assert R.sum_tree(np.zeros((0, 6)), np.array([0, 0])).tolist() == [[0.0] * 6]


def test_the_negative_controls_are_caught():
    pos, geo = POLY["ellipse97"]
    x = np.zeros((len(pos), 3), F32)
    x[:, 2] = (1.5 * pos[:, 0].astype(F64)).astype(F32)
    T, _, _ = R.terms(x, geo, pcol=2)
    S = R.sum_plain(T, geo["body_offsets"])
    A = R.shoelace(pos.astype(F64)[geo["items"]])
    assert abs(S[0, 0] + 1.5 * A) < 1e-6 * A
    flipped = dict(geo, area=-geo["area"])                          # an inward normal: the sign of the force
    assert abs(R.sum_plain(R.terms(x, flipped, pcol=2)[0], geo["body_offsets"])[0, 0] - 1.5 * A) < 1e-6 * A
    unordered = R.geometry(pos, loops=[np.arange(len(pos))])        # the shuffled rows taken as a loop: no polygon
    assert abs(R.sum_plain(R.terms(x, unordered, pcol=2)[0], unordered["body_offsets"])[0, 0] + 1.5 * A) > 0.1 * A
