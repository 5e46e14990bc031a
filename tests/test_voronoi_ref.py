"""tests/voronoi_ref.py pinned on the host, before any kernel runs: its two forms of the Voronoi construction (`cells_ring`, the
device's order over the cell grid; `cells_sorted`, independent of the grid and of the clip's form) against brute force, against
scipy.spatial.Voronoi where scipy imports, against closed forms — and the area tolerance the device is held to, measured here.

The tolerance's unit is 2⁻⁵² r_i², r_i the farthest vertex of cell i.  The largest |cells_ring − cells_sorted| over `voronoi_ref.cases()`
is `MEASURED_UNITS`; the device, which follows `cells_ring`'s order and formulas and should add nothing, gets 8 × that against
`cells_sorted` (the factor pays for the cases the list does not hold).  tests/VOLUMES_MEASURED.md records the figures."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import voronoi_ref as V                                        # noqa: E402

_RESULTS = {}


def both(name):
    """(ring, sorted) of a case of V.cases(), computed once."""
    if not _RESULTS:
        for nm, pos, box, nrm in V.cases():
            _RESULTS[nm] = (pos, box, nrm, None)
    pos, box, nrm, res = _RESULTS[name]
    if res is None:
        res = (V.cells_ring(pos, V.bin_cloud(pos), box, nrm), V.cells_sorted(pos, box, nrm))
        _RESULTS[name] = (pos, box, nrm, res)
    return res


def units(r, s):
    return V.area_units(r["area"], s["area"], np.maximum(r["rmax"], s["rmax"]))


@pytest.mark.parametrize("gen", [V.uniform_cloud, V.jittered_lattice])
def test_both_forms_against_brute_force(gen):
    pos = gen(200)
    brute = V.cells_sorted(pos, V.UNIT_BOX, stop=False)
    for res in (V.cells_ring(pos, V.bin_cloud(pos), V.UNIT_BOX), V.cells_sorted(pos, V.UNIT_BOX)):
        assert np.array_equal(res["nvert"], brute["nvert"])
        assert units(res, brute).max() <= V.MEASURED_UNITS
        assert np.abs(res["centroid"] - brute["centroid"]).max() <= 1e-12


def test_against_scipy_on_interior_cells():
    spatial = pytest.importorskip("scipy.spatial")
    pos = V.uniform_cloud(257)
    r, s = both("uniform_cloud-257")
    vor = spatial.Voronoi(pos.astype(np.float64))
    checked = 0
    for i in range(pos.shape[0]):
        if r["flags"][i] & V.BOX:
            continue
        region = vor.regions[vor.point_region[i]]
        assert -1 not in region and len(region) >= 3
        poly = vor.vertices[region] - pos[i].astype(np.float64)
        poly = poly[np.argsort(np.arctan2(poly[:, 1], poly[:, 0]))]
        nx = np.roll(poly, -1, 0)
        a = 0.5 * float((poly[:, 0] * nx[:, 1] - nx[:, 0] * poly[:, 1]).sum())
        for res in (r, s):          # (qhull's vertices carry their own rounding: a relative 1e-9 of the cell's disc is far above it)
            assert abs(res["area"][i] - a) <= 1e-9 * res["rmax"][i] ** 2, (i, res["area"][i], a)
            assert res["nvert"][i] == len(region)
        checked += 1
    assert checked > 150


@pytest.mark.parametrize("name,box", [(f"{g}-{n}", V.UNIT_BOX) for g in ("uniform_cloud", "jittered_lattice") for n in V.SIZES]
                         + [("box-twice-257", (-0.5, -0.5, 1.5, 1.5)), ("central-ring-24", (-1.0, -1.0, 1.0, 1.0))])
def test_areas_sum_to_the_box(name, box):
    size = (box[2] - box[0]) * (box[3] - box[1])
    for res in both(name):
        n = res["area"].size
        assert abs(float(res["area"].sum()) - size) <= n * 2.0 ** -52 * size
        assert not (res["flags"] & (V.WALL | V.DUPLICATE | V.OVERFLOW)).any()


def test_lattice_is_exact():
    """Pitch 2⁻⁵: four cells meet at every vertex (the cocircular case); every interior cell is h², its centroid the node."""
    m, h = 9, 2.0 ** -5
    pos = V.lattice(m)
    j, i = np.divmod(np.arange(m * m), m)
    inner = (i > 0) & (i < m - 1) & (j > 0) & (j < m - 1)
    for res in both("lattice-9"):
        assert np.array_equal(res["area"][inner], np.full(int(inner.sum()), h * h))
        assert np.abs(res["centroid"][inner] - pos[inner]).max() <= 2.0 ** -52
        assert float(res["area"].sum()) == ((m - 1) * h) ** 2
    ring = both("lattice-9")[0]          # (BOX is the ring form's: the independent form does not follow the edges' origin)
    assert not (ring["flags"][inner] & V.BOX).any() and (ring["flags"][~inner] & V.BOX).all()


def test_central_ring():
    """A node at the centre of a ring of m nodes at radius r owns the regular m-gon of inradius r / 2: m (r / 2)² tan(π / m).  m = 24
    fits; m = 40 exceeds the 32 vertices: OVERFLOW, area +0 — and only that node."""
    r = 0.25
    for res in both("central-ring-24"):
        exact = 24 * (r / 2) ** 2 * math.tan(math.pi / 24)
        assert res["nvert"][0] == 24 and res["flags"][0] == 0
        assert abs(res["area"][0] - exact) <= 1e-7 * exact          # (the ring's fp32 positions are 2⁻²⁴-relative off the circle)
    for res in both("central-ring-40"):
        assert res["flags"][0] == V.OVERFLOW and res["nvert"][0] == 0
        assert res["area"][0] == 0.0 and not np.signbit(res["area"][0])
        assert np.array_equal(res["centroid"][0], [0.0, 0.0])
        assert not (res["flags"][1:] & V.OVERFLOW).any() and (res["area"][1:] > 0).all()
        exact = 40 * (r / 2) ** 2 * math.tan(math.pi / 40)
        assert abs(float(res["area"].sum()) + exact - 4.0) <= 1e-7


def test_small_clouds():
    box = (0.0, 0.0, 1.0, 1.0)
    one = np.array([[0.25, 0.5]], np.float32)
    assert V.cells_ring(one, V.bin_cloud(one), box)["flags"][0] == V.BOX
    for res in (V.cells_ring(one, V.bin_cloud(one), box), V.cells_sorted(one, box)):
        assert res["area"][0] == 1.0 and res["nvert"][0] == 4 and int(res["flags"][0]) & ~V.BOX == 0
        assert np.array_equal(res["centroid"][0], [0.5, 0.5])
    two = np.array([[0.25, 0.5], [0.75, 0.5]], np.float32)
    for res in (V.cells_ring(two, V.bin_cloud(two), box), V.cells_sorted(two, box)):
        assert np.array_equal(res["area"], [0.5, 0.5]) and np.array_equal(res["centroid"], [[0.25, 0.5], [0.75, 0.5]])
    line = np.array([[0.125, 0.5], [0.5, 0.5], [0.75, 0.5]], np.float32)          # three collinear nodes: strips
    for res in (V.cells_ring(line, V.bin_cloud(line), box), V.cells_sorted(line, box)):
        assert np.array_equal(res["area"], [0.3125, 0.3125, 0.375]) and np.array_equal(res["nvert"], [4, 4, 4])
    pair = np.array([[0.25, 0.5], [0.75, 0.5], [0.25, 0.5]], np.float32)          # a duplicate pair: both flagged, both own the cell
    for res in (V.cells_ring(pair, V.bin_cloud(pair), box), V.cells_sorted(pair, box)):
        assert np.array_equal(res["flags"] & ~np.uint8(V.BOX), [V.DUPLICATE, 0, V.DUPLICATE])
        assert np.array_equal(res["area"], [0.5, 0.5, 0.5])


def test_duplicates_are_flagged():
    for res in both("duplicates-65"):
        dup = (res["flags"] & V.DUPLICATE) != 0
        assert np.array_equal(np.nonzero(dup)[0], [5, 7, 8, 9, 40])
        assert res["area"][5] == res["area"][40] and res["area"][7] == res["area"][8] == res["area"][9]


@pytest.mark.parametrize("n,counts", V.ANNULI)
def test_wall_closure(n, counts):
    """Σ area against box − Σ shoelace(body).  The wall half-plane is tangent: the wall cells end at the polygon of the tangents, the
    bodies are measured by the polygon through the nodes, so the sum falls SHORT — for m nodes on a circle of radius R by at most
    m R² (tan(π/m) − ½ sin(2π/m)) a body (all of it when no fluid cell reaches behind the tangents).  Only the sign, that bound, and the
    equality of the two forms are asserted; tests/VOLUMES_MEASURED.md records the values."""
    pos, box, nrm, geo, exact = V.annulus_case(n, counts)
    name = f"annulus-{n}-{'-'.join(str(c) for c in counts)}"
    sliver = sum(m * 0.25 * (math.tan(math.pi / m) - 0.5 * math.sin(2.0 * math.pi / m)) for m in counts)
    closures = []
    for res in both(name):
        wall = (res["flags"] & V.WALL) != 0
        assert np.array_equal(np.nonzero(wall)[0], np.sort(geo["items"]))
        assert not (res["flags"] & V.OVERFLOW).any() and (res["area"] > 0).all()
        closure = float(res["area"].sum()) - exact
        print(f"{name}: closure {closure:.6e} (tangent slivers at most {-sliver:.6e})")
        assert -sliver * (1.0 + 1e-6) <= closure < 0.0
        closures.append(closure)
    assert abs(closures[0] - closures[1]) <= pos.shape[0] * 2.0 ** -52 * exact


def test_the_measured_tolerance():
    """The largest |cells_ring − cells_sorted| over every case, in units of 2⁻⁵² r²: what `MEASURED_UNITS` records."""
    worst = {}
    for name, _, _, _ in V.cases():
        r, s = both(name)
        # (on the cocircular lattice a clip through an existing vertex may split it into two a rounding apart — which of the four
        # cells' bisectors comes first decides it, so the count follows the order of traversal there, and the area does not; the
        # neighbours of a duplicate pair meet one bisector twice, with the same effect)
        assert name in ("lattice-9", "duplicates-65") or np.array_equal(r["nvert"], s["nvert"]), name
        assert np.array_equal(r["flags"] & ~np.uint8(V.BOX), s["flags"]), name
        worst[name] = float(units(r, s).max())
    top = max(worst, key=worst.get)
    print(f"largest |ring − sorted| = {worst[top]:.3f} units on {top}")
    assert worst[top] <= V.MEASURED_UNITS and V.DEVICE_UNITS == 8.0 * V.MEASURED_UNITS
    assert worst[top] >= 0.5 * V.MEASURED_UNITS          # the record is the measurement, not a guess far above it
