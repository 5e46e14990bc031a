"""g4c_voronoi_cells (csrc/control_volumes.hip) through ops.voronoi_cells and gfd.ControlVolumes against tests/voronoi_ref.py:
`area`, `centroid`, `nvert`, `flags`, `rings` EQUAL — bit for bit — to `cells_ring` on the device's own bins (the kernel's order in plain
Python floats), `area` within `DEVICE_UNITS` · 2⁻⁵² r² of the independent `cells_sorted` (8 × what the two forms differ by on the host:
tests/test_voronoi_ref.py, tests/VOLUMES_MEASURED.md), Σ area against the box within N 2⁻⁵² |box|.  Every output is sentinel-filled
beforehand and lives between guards, every input is frozen."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

import voronoi_ref as V                                        # noqa: E402
from footprint import assert_footprint, flat_arena, frozen     # noqa: E402
import graphs4cfd_amd as gfd                                   # noqa: E402
from graphs4cfd_amd import _lib, ops, synthetic as S           # noqa: E402

DEV = torch.device("cuda", 0)
F64, I32, U8 = torch.float64, torch.int32, torch.uint8
GUARD = 4096


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(pos, box, normals=None):
    """(device results as numpy, the reference on the device's own bins): outputs between guards, inputs frozen."""
    n = pos.shape[0]
    grid = S._bin_cloud(dev(pos), V.GRID_K)
    nrm = None if normals is None else dev(normals)
    arenas = [flat_arena(n, F64, device=DEV), flat_arena(2 * n, F64, device=DEV), flat_arena(n, I32, device=DEV),
              flat_arena(n, I32, device=DEV)]
    fl_whole = torch.full((n + 2 * GUARD,), 0xA5, dtype=U8, device=DEV)
    out = (arenas[0][0], arenas[1][0].view(n, 2), arenas[2][0], fl_whole[GUARD:GUARD + n], arenas[3][0])
    with frozen(grid["pos_sorted"], grid["order"], grid["cell_start"], nrm, what="voronoi_cells"):
        got = ops.voronoi_cells(grid, box, nrm, out=out)
        torch.cuda.synchronize()
    assert all(g is o for g, o in zip(got, out))
    for (view, whole), name in zip(arenas, ("area", "centroid", "nvert", "rings")):
        assert_footprint(whole, view, what=name)
    assert bool((fl_whole[:GUARD] == 0xA5).all()) and bool((fl_whole[GUARD + n:] == 0xA5).all())
    assert bool((out[3] != 0xA5).all())
    res = dict(area=out[0].cpu().numpy(), centroid=out[1].cpu().numpy(), nvert=out[2].cpu().numpy(), flags=out[3].cpu().numpy(),
               rings=out[4].cpu().numpy())
    return res, V.cells_ring(pos, V.bins_of(grid), box, normals)


def assert_equal_bits(res, ref, what=""):
    for key in ("area", "centroid"):
        assert np.array_equal(res[key].view(np.int64), ref[key].view(np.int64)), (what, key, np.nonzero(res[key] != ref[key])[0][:8])
    for key in ("nvert", "flags", "rings"):
        assert np.array_equal(res[key], ref[key]), (what, key, np.nonzero(res[key] != ref[key])[0][:8])


def assert_within(res, ref, pos, box, normals=None, what=""):
    s = V.cells_sorted(pos, box, normals)
    u = V.area_units(res["area"], s["area"], np.maximum(ref["rmax"], s["rmax"]))
    print(f"{what}: largest |device − sorted| = {u.max():.3f} units of 2^-52 r² (allowed {V.DEVICE_UNITS})")
    assert u.max() <= V.DEVICE_UNITS


@pytest.mark.parametrize("shuffle", [False, True])
@pytest.mark.parametrize("gen", [V.uniform_cloud, V.jittered_lattice])
@pytest.mark.parametrize("n", V.SIZES)
def test_cells_against_the_restatement(n, gen, shuffle):
    pos = gen(n)
    if shuffle:
        pos, _ = V.shuffled(pos, n)
    res, ref = run(pos, V.UNIT_BOX)
    what = f"{gen.__name__}-{n}{'-shuffled' if shuffle else ''}"
    assert_equal_bits(res, ref, what)
    assert_within(res, ref, pos, V.UNIT_BOX, what=what)
    assert abs(float(res["area"].sum()) - 1.0) <= n * 2.0 ** -52
    assert not (res["flags"] & ~np.uint8(V.BOX)).any() and (res["area"] > 0).all()


def test_a_shuffled_order_permutes_the_cells():
    pos = V.uniform_cloud(257)
    shuf, perm = V.shuffled(pos, 1)
    a, _ = run(pos, V.UNIT_BOX)
    b, _ = run(shuf, V.UNIT_BOX)
    u = V.area_units(b["area"], a["area"][perm], V.cells_sorted(shuf, V.UNIT_BOX)["rmax"])
    assert u.max() <= V.DEVICE_UNITS          # (another order of the rows is another stable sort within a cell: the clips' order may differ)
    assert np.array_equal(b["flags"], a["flags"][perm])


def test_the_lattice_is_exact():
    m, h = 9, 2.0 ** -5
    pos = V.lattice(m)
    box = V.bounding_box(pos)
    res, ref = run(pos, box)
    assert_equal_bits(res, ref, "lattice")
    j, i = np.divmod(np.arange(m * m), m)
    inner = (i > 0) & (i < m - 1) & (j > 0) & (j < m - 1)
    assert np.array_equal(res["area"][inner], np.full(int(inner.sum()), h * h))
    assert not (res["flags"][inner] & V.BOX).any() and (res["flags"][~inner] & V.BOX).all()
    assert float(res["area"].sum()) == ((m - 1) * h) ** 2


def test_the_central_ring_fits_or_overflows():
    box, r = (-1.0, -1.0, 1.0, 1.0), 0.25
    pos = V.central_ring(24, r, 200)
    res, ref = run(pos, box)
    assert_equal_bits(res, ref, "ring-24")
    assert_within(res, ref, pos, box, what="ring-24")
    exact = 24 * (r / 2) ** 2 * math.tan(math.pi / 24)
    assert res["nvert"][0] == 24 and res["flags"][0] == 0 and abs(res["area"][0] - exact) <= 1e-7 * exact
    assert abs(float(res["area"].sum()) - 4.0) <= pos.shape[0] * 2.0 ** -52 * 4.0
    pos = V.central_ring(40, r, 200)
    res, ref = run(pos, box)
    assert_equal_bits(res, ref, "ring-40")
    assert_within(res, ref, pos, box, what="ring-40")
    assert res["flags"][0] == V.OVERFLOW and res["nvert"][0] == 0
    assert res["area"][0] == 0.0 and not np.signbit(res["area"][0]) and np.array_equal(res["centroid"][0], [0.0, 0.0])
    assert not (res["flags"][1:] & V.OVERFLOW).any() and (res["area"][1:] > 0).all()          # the neighbours are unaffected
    exact = 40 * (r / 2) ** 2 * math.tan(math.pi / 40)
    assert abs(float(res["area"].sum()) + exact - 4.0) <= 1e-7


def test_duplicates_are_flagged():
    pos = V.duplicates_cloud()
    res, ref = run(pos, V.UNIT_BOX)
    assert_equal_bits(res, ref, "duplicates")
    assert_within(res, ref, pos, V.UNIT_BOX, what="duplicates")
    assert np.array_equal(np.nonzero(res["flags"] & V.DUPLICATE)[0], [5, 7, 8, 9, 40])
    assert res["area"][5] == res["area"][40] and res["area"][7] == res["area"][8] == res["area"][9]


def test_all_nodes_in_one_grid_cell():
    pos = (0.5 + 0.001 * (V.uniform_cloud(40, seed=9).astype(np.float64) - 0.5)).astype(np.float32)
    pos = np.concatenate([pos, pos[:1] + np.float32(0.0005)])
    grid = S._bin_cloud(dev(pos), 200)          # cells of ~127 nodes: this cloud is one cell
    assert [int(c) for c in grid["n_cells"]] == [1, 1, 1]
    area, _, nvert, flags, rings = ops.voronoi_cells(grid, V.UNIT_BOX)
    ref = V.cells_ring(pos, V.bins_of(grid), V.UNIT_BOX)
    assert np.array_equal(area.cpu().numpy().view(np.int64), ref["area"].view(np.int64))
    assert np.array_equal(nvert.cpu().numpy(), ref["nvert"]) and np.array_equal(flags.cpu().numpy(), ref["flags"])
    assert bool((rings == 1).all()) and abs(float(area.sum()) - 1.0) <= pos.shape[0] * 2.0 ** -52


def test_a_box_twice_the_cloud():
    pos, box = V.uniform_cloud(257), (-0.5, -0.5, 1.5, 1.5)
    res, ref = run(pos, box)
    assert_equal_bits(res, ref, "box-twice")
    assert_within(res, ref, pos, box, what="box-twice")
    assert abs(float(res["area"].sum()) - 4.0) <= 257 * 2.0 ** -52 * 4.0
    assert res["rings"].max() > 4          # the hull nodes scan the grid: what `rings` is there to show


def graph_of(pos, bound=None, batch=None):
    g = gfd.Graph()
    g.pos = dev(pos)
    if bound is not None:
        g.bound = dev(bound)
    if batch is not None:
        g.batch = dev(batch)
    return g


@pytest.mark.parametrize("n,counts", V.ANNULI)
def test_wall_cells_and_the_closure(n, counts):
    pos, box, nrm, geo, exact = V.annulus_case(n, counts)
    res, ref = run(pos, box, nrm)
    assert_equal_bits(res, ref, "annulus")
    assert_within(res, ref, pos, box, nrm, what=f"annulus-{n}-{counts}")
    # the same through the public class, the normals from a BodyForces of the graph's wall nodes
    bound = np.zeros(pos.shape[0], np.int64)
    bound[geo["items"]] = 4
    import forces_ref as FR
    _, wall, label = FR.annulus(n, list(counts))
    graph = graph_of(pos, bound)
    cv = gfd.ControlVolumes(graph, box=box, bodies=gfd.BodyForces(graph, nodes=dev(wall), bodies=dev(label)))
    assert np.array_equal(cv.area.cpu().numpy().view(np.int64), ref["area"].view(np.int64))
    flags = cv.flags.cpu().numpy()
    assert np.array_equal(np.nonzero(flags & cv.WALL)[0], np.sort(geo["items"]))          # WALL exactly on the wall items
    assert not bool(cv.degenerate.any()) and not (flags & cv.OVERFLOW).any()
    closure, ref_closure = float(cv.area.cpu().numpy().sum()) - exact, float(ref["area"].sum()) - exact
    print(f"annulus-{n}-{counts}: closure {closure:.6e}")
    assert closure == ref_closure and closure < 0.0
    assert cv.total == pytest.approx(exact + closure, abs=1e-12)


def test_bodies_true_takes_the_wall_from_bound():
    pos, box, nrm, geo, _ = V.annulus_case(1500, (64,))
    bound = np.zeros(pos.shape[0], np.int64)
    bound[geo["items"]] = 4
    graph = graph_of(pos, bound)
    a = gfd.ControlVolumes(graph, box=box, bodies=True)
    b = gfd.ControlVolumes(graph, box=box, normals=dev(nrm))
    assert torch.equal(a.area, b.area) and torch.equal(a.flags, b.flags)
    assert isinstance(a.bodies, gfd.BodyForces)


def test_a_batch_of_two_overlapping_graphs():
    p0, p1 = V.uniform_cloud(257), V.jittered_lattice(300, seed=2)
    batch = np.concatenate([np.zeros(257, np.int64), np.ones(300, np.int64)])
    both = gfd.ControlVolumes(graph_of(np.concatenate([p0, p1]), batch=batch))
    one, two = gfd.ControlVolumes(graph_of(p0)), gfd.ControlVolumes(graph_of(p1))
    for key in ("area", "centroid", "nvert", "flags", "rings"):
        assert torch.equal(getattr(both, key), torch.cat([getattr(one, key), getattr(two, key)])), key
    assert torch.equal(both.box, torch.cat([one.box, two.box])) and tuple(both.box.shape) == (2, 4)
    assert both.box[0].tolist() == list(V.bounding_box(p0))


def test_the_class_and_its_standalone_integral():
    pos = V.uniform_cloud(1500)
    cv = gfd.ControlVolumes(graph_of(pos))
    box = V.bounding_box(pos)
    size = (box[2] - box[0]) * (box[3] - box[1])
    assert abs(cv.total - size) <= 1500 * 2.0 ** -52 * size and cv.weights(torch.float32).dtype == torch.float32
    x = torch.ones((1500, 3), device=DEV)
    x[:, 1] = dev(pos[:, 0])
    got = cv.integrate(x, [(-1, -1), (0, 0), (1, -1)]).cpu().numpy()
    assert abs(got[0] - size) <= 1504 * 2.0 ** -52 * size and got[0] == got[1]
    # ∫ x over the box = Σ area · centroid_x exactly in exact arithmetic; the node value stands for the centroid's here
    assert abs(got[2] - 0.5 * (box[0] + box[2]) * size) <= 0.02 * size
