"""The launch `g4c_body_forces` alone (ops.body_forces, gfd.BodyForces) against tests/forces_ref.py: the surface pressure and wall shear
bit for bit the restatement's, the per-body sums bit for bit its sum in the kernel's own order and within the records' bound of the
plain fp64 sum, `cur` the fp32 rounding of the fp64 totals, the four gradient numbers bit for bit `MeshGradient.derived` at the wall
rows, the write footprint (guard arenas round stats, cur and wall, the inputs frozen), and the geometry `gfd.BodyForces` builds.

The clouds are annuli of about 600 fluid nodes round circular bodies whose walls hold 3 .. 1000 items (the wave and thread-stride
edges: 63, 64, 65, 255, 256, 257), connected by the device's kNN at k = 6 and then thinned to a ragged in-degree, with one wall node
left without in-edges (its gradient is zero)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

import footprint as FP                                   # noqa: E402
import forces_ref as R                                   # noqa: E402
import graphs4cfd_amd as gfd                             # noqa: E402
from graphs4cfd_amd import ops, synthetic as S           # noqa: E402

DEV = torch.device("cuda", 0)
F32, F64, I32 = torch.float32, torch.float64, torch.int32
NF, STEPS = 3, 4
CASES = [(3,), (5,), (63,), (64,), (65,), (255,), (256,), (257,), (1000,), (5, 257), (64, 3, 1000, 65, 255)]
SCALE, SHIFT, MU = [1.5, 0.75, 2.5], [0.25, -0.5, 0.125], 0.03125 * 1.3
_cache = {}


def cloud(counts):
    """The graph of one case (shared by the tests that use it, never changed), its gradient, its operators and the host tables."""
    if counts in _cache:
        return _cache[counts]
    pos, wall, label = R.annulus(600, counts, seed=len(counts))
    g = gfd.Graph(pos=torch.from_numpy(pos).to(DEV))
    ei, _ = S.connect_knn(g.pos, 6)
    rng = np.random.default_rng(sum(counts))
    keep = torch.from_numpy(rng.random(int(ei.size(1))) > 0.15).to(DEV)          # a ragged in-degree, the edges still grouped by target
    lone = int(wall[len(wall) // 2])
    keep &= ei[1] != lone                                                         # a wall node without in-edges
    g.edge_index = ei[:, keep].contiguous()
    g.bound = torch.zeros(len(pos), dtype=torch.long, device=DEV)
    g.bound[torch.from_numpy(wall).to(DEV)] = 4
    mg = gfd.MeshGradient(g)
    assert bool(mg.degenerate[lone]) and int((mg.off[1:] - mg.off[:-1]).max()) == 6 and int((mg.off[1:] - mg.off[:-1]).min()) == 0
    labels = torch.from_numpy(label) if len(counts) > 1 else None
    nodes = torch.from_numpy(wall) if len(counts) > 1 else None                   # (one body: the graph's own bound == 4)
    kw = dict(nodes=nodes, bodies=labels, scale=SCALE, shift=SHIFT)
    geo = R.geometry(pos, nodes=wall, labels=None if labels is None else label)
    tabs = dict(off=mg.off.cpu().numpy(), g=mg.g.cpu().numpy(), src=mg.src.cpu().numpy())
    gen = torch.Generator().manual_seed(7)
    target = torch.randn(len(pos), NF * STEPS + 3, generator=gen).to(DEV)         # x_ld > nf for a step's view and for the target
    visc, inviscid = gfd.BodyForces(g, mu=MU, gradient=mg, **kw), gfd.BodyForces(g, **kw)
    assert visc.items.tolist() == geo["items"].tolist() and torch.equal(visc.arm, inviscid.arm) and torch.equal(visc.unit, inviscid.unit)
    # the launch is compared on the DEVICE's tables (test_the_geometry_is_the_restatements pins them: the unit normals may differ from
    # numpy's by an ulp, the arms by the order in which the mean of a body's nodes was summed)
    tables = dict(geo, area=visc.area.cpu().numpy(), unit=visc.unit.cpu().numpy(), arm=visc.arm.cpu().numpy())
    out = dict(g=g, mg=mg, pos=pos, wall=wall, label=label, geo=geo, tables=tables, tabs=tabs, target=target, lone=lone, visc=visc, inviscid=inviscid)
    _cache[counts] = out
    return out


def ref_of(c, x, t, x_step, viscous):
    """(stats row [B, 6] in tree order, the plain sums, the bound, wall [W, 2], cur [B, 3]) of the restatement."""
    kw = dict(pcol=2, p_scale=SCALE[2], p_shift=SHIFT[2], col0=x_step * t)
    if viscous:
        kw.update(mu=MU, u_scale=SCALE[0], v_scale=SCALE[1], **c["tabs"])
    T, wall, G = R.terms(x.cpu().numpy(), c["tables"], **kw)
    off = c["geo"]["body_offsets"]
    tree = R.sum_tree(T, off)
    return tree, R.sum_plain(T, off), R.sum_bound(T, off), wall, R.cur32(tree), G


def launch(c, x, *, viscous, t, x_step, on_device, stats, cur, wall):
    op = c["visc"] if viscous else c["inviscid"]
    mg = c["mg"] if viscous else None
    step = torch.tensor([t, 99], dtype=I32, device=DEV) if on_device else None
    with FP.frozen(x, op._item32, op.body_offsets, op.area, op.unit, op.arm, step, c["mg"].g, c["mg"].src, c["mg"].off, what="body_forces"):
        ops.body_forces(x, op._item32, op.body_offsets, op.area, op.unit, op.arm, cur, **op.constants(), off=mg and mg.off, g=mg and mg.g,
                        src=mg and mg.src, wall=wall, stats=stats, max_steps=STEPS, step=step, t=0 if on_device else t, x_step=x_step)
    torch.cuda.synchronize()


def arenas(n_bodies, n_items):
    st, st_whole = FP.flat_arena(STEPS * n_bodies * 6, F64, device=DEV)
    cur, cur_whole = FP.flat_arena(n_bodies * 3, F32, device=DEV)
    wall, wall_whole = FP.flat_arena(n_items * 2, F32, device=DEV)
    return (st, st_whole), (cur, cur_whole), (wall, wall_whole)


def stats_rows(n_bodies, t):
    m = torch.zeros((1, STEPS * n_bodies * 6), dtype=torch.bool)
    if 0 <= t < STEPS:
        m[0, t * n_bodies * 6:(t + 1) * n_bodies * 6] = True
    return m


@pytest.mark.parametrize("counts", CASES, ids=lambda c: "-".join(map(str, c)))
def test_the_launch_is_the_restatement(counts):
    c = cloud(counts)
    nb, nw = len(counts), sum(counts)
    worst, k = 0.0, 0
    for viscous in (False, True):
        for x_step in (0, NF):
            for on_device in (False, True):
                t = (1, 3, 0, 2)[k % 4]
                k += 1
                x = c["target"] if x_step else c["target"][:, NF * t:NF * (t + 1)]          # (a step's view: rows of x_ld = 15 floats)
                (st, st_w), (cur, cur_w), (wall, wall_w) = arenas(nb, nw)
                launch(c, x, viscous=viscous, t=t, x_step=x_step, on_device=on_device, stats=st.view(STEPS, nb, 6), cur=cur.view(nb, 3), wall=wall.view(nw, 2))
                what = f"bodies {counts}, mu {MU if viscous else 0}, x_step {x_step}, step {'on the device' if on_device else 'by value'}, t {t}"
                FP.assert_footprint(st_w, st, stats_rows(nb, t), what + ": stats")
                FP.assert_footprint(cur_w, cur, None, what + ": cur")
                FP.assert_footprint(wall_w, wall, None, what + ": wall")
                tree, plain, bound, rwall, rcur, _ = ref_of(c, c["target"], t, NF, viscous)
                got = st.view(STEPS, nb, 6)[t]
                R.same(wall.view(nw, 2), rwall, what + ": wall")
                R.same(got, tree, what + ": stats, the kernel's order")
                worst = max(worst, R.within(got, plain, bound, what + ": stats against the plain sum"))
                R.same(cur.view(nb, 3), R.cur32(got.cpu().numpy()), what + ": cur")
                if not viscous:
                    assert not bool(got[:, [2, 3, 5]].any()) and not bool(wall.view(nw, 2)[:, 1].any())
                # a second run: the same bits
                (st2, _), (cur2, _), (wall2, _) = arenas(nb, nw)
                launch(c, x, viscous=viscous, t=t, x_step=x_step, on_device=on_device, stats=st2.view(STEPS, nb, 6), cur=cur2.view(nb, 3), wall=wall2.view(nw, 2))
                assert torch.equal(FP._int_view(st2), FP._int_view(st)) and torch.equal(FP._int_view(cur2), FP._int_view(cur)) and torch.equal(FP._int_view(wall2), FP._int_view(wall))
    print(f"bodies {counts}: stats against the plain fp64 sum, measured / allowed = {worst:.3f}")


def test_one_item_bodies_expose_the_four_gradient_numbers():
    """W bodies of one item each: with area (1, 0) and the v fields scaled away Fv = (2 G[u][0], G[u][1]); with area (0, 1) and the u
    fields scaled away Fv = (G[v][0], 2 G[v][1]) — the numbers the kernel formed, against MeshGradient.derived at the wall rows."""
    c = cloud((65,))
    op, mg, nw = c["visc"], c["mg"], 65
    x = c["target"][:, :NF]
    want = mg.derived(x.contiguous(), ("grad:0", "grad:1"))[op.items].double()
    R.same(want.float(), R.gradients32(x.cpu().numpy(), c["tabs"]["off"], c["tabs"]["g"], c["tabs"]["src"], 0, 1)[c["geo"]["items"]], "derived against the restatement")
    assert not bool(want[op.items == c["lone"]].any()) and bool(want.abs().sum() > 0)
    boff = torch.arange(nw + 1, dtype=I32, device=DEV)
    got = {}
    for name, area, us, vs in (("u", [1.0, 0.0], 1.0, 0.0), ("v", [0.0, 1.0], 0.0, 1.0)):
        tab = torch.tensor(area, dtype=F64, device=DEV).repeat(nw, 1).contiguous()
        stats = torch.zeros((1, nw, 6), dtype=F64, device=DEV)
        ops.body_forces(x, op._item32, boff, tab, tab, tab, torch.zeros((nw, 3), device=DEV), pcol=2, ucol=0, vcol=1, mu=1.0, u_scale=us, v_scale=vs,
                        off=mg.off, g=mg.g, src=mg.src, stats=stats, max_steps=1)
        got[name] = stats[0, :, 2:4]
    assert torch.equal(got["u"][:, 0], 2.0 * want[:, 0]) and torch.equal(got["u"][:, 1], want[:, 1])
    assert torch.equal(got["v"][:, 0], want[:, 2]) and torch.equal(got["v"][:, 1], 2.0 * want[:, 3])


def test_small_integers_sum_exactly():
    """Integer pressure on a polygon of integer coordinates, mu = 0: every product and every partial sum is exact, whatever the order."""
    n = 257
    th = 2.0 * np.pi * (np.arange(n) + 0.25) / n
    pos = np.round(np.stack([900.0 * np.cos(th), 700.0 * np.sin(th)], axis=1)).astype(np.float32)
    assert len({tuple(p) for p in pos.tolist()}) == n
    shuffle = np.random.default_rng(1).permutation(n)
    pos = pos[shuffle]
    x = torch.from_numpy(np.random.default_rng(2).integers(-50, 50, (n, 3)).astype(np.float32)).to(DEV)
    op = gfd.BodyForces(gfd.Graph(pos=torch.from_numpy(pos).to(DEV)), torch.arange(n), centre=[3.0, -2.0])
    geo = R.geometry(pos, nodes=np.arange(n), centre=[3.0, -2.0])
    T, wall, _ = R.terms(x.cpu().numpy(), geo, pcol=2)
    assert np.array_equal(T, np.round(2 * T) / 2) and np.array_equal(R.sum_tree(T, geo["body_offsets"]), R.sum_plain(T, geo["body_offsets"]))
    R.same(op.forces(x), R.sum_plain(T, geo["body_offsets"]), "integers: stats")
    R.same(op.wall(x), wall, "integers: wall")
    hist = op.history(torch.cat([x, 2 * x, x + 1], 1).contiguous(), 3, nf=3)
    R.same(hist[1], 2 * R.sum_plain(T, geo["body_offsets"]), "integers: history")
    R.same(hist[0], R.sum_plain(T, geo["body_offsets"]), "integers: history, step 0")


@pytest.mark.parametrize("t", [-1, STEPS])
def test_a_step_off_the_range_writes_cur_and_wall_and_no_stats(t):
    c = cloud((5, 257))
    nb, nw = 2, 262
    x = c["target"][:, :NF]
    for on_device in (False, True):
        (st, st_w), (cur, cur_w), (wall, wall_w) = arenas(nb, nw)
        launch(c, x, viscous=True, t=t, x_step=0, on_device=on_device, stats=st.view(STEPS, nb, 6), cur=cur.view(nb, 3), wall=wall.view(nw, 2))
        FP.assert_footprint(st_w, st, stats_rows(nb, t), f"t {t}: stats")
        FP.assert_footprint(cur_w, cur, None, f"t {t}: cur")
        FP.assert_footprint(wall_w, wall, None, f"t {t}: wall")
        tree, _, _, rwall, rcur, _ = ref_of(c, x, 0, 0, True)
        R.same(wall.view(nw, 2), rwall, f"t {t}: wall")
        R.same(cur.view(nb, 3), rcur, f"t {t}: cur")
        # a target's columns are addressed by the step: off the range nothing is read and nothing written
        (st, st_w), (cur, cur_w), (wall, wall_w) = arenas(nb, nw)
        launch(c, c["target"], viscous=True, t=t, x_step=NF, on_device=on_device, stats=st.view(STEPS, nb, 6), cur=cur.view(nb, 3), wall=wall.view(nw, 2))
        for whole, view, name in ((st_w, st, "stats"), (cur_w, cur, "cur"), (wall_w, wall, "wall")):
            FP.assert_footprint(whole, view, torch.zeros((1, view.numel()), dtype=torch.bool), f"t {t}, x_step {NF}: {name}")


def test_no_body_and_no_item_launch_nothing():
    x = torch.zeros((8, 3), device=DEV)
    empty = torch.zeros((0, 2), dtype=F64, device=DEV)
    for boff, nb in ((torch.zeros(1, dtype=I32, device=DEV), 0), (torch.zeros(2, dtype=I32, device=DEV), 1)):
        st, st_w = FP.flat_arena(max(STEPS * nb * 6, 1), F64, device=DEV)
        cur, cur_w = FP.flat_arena(max(nb * 3, 1), F32, device=DEV)
        ops.body_forces(x, torch.zeros(0, dtype=I32, device=DEV), boff, empty, empty, empty, cur[:nb * 3].view(nb, 3), pcol=2,
                        wall=torch.zeros((0, 2), device=DEV), stats=st[:STEPS * nb * 6].view(STEPS, nb, 6), max_steps=STEPS, t=1)
        torch.cuda.synchronize()
        FP.assert_footprint(st_w, st, torch.zeros((1, st.numel()), dtype=torch.bool), f"{nb} bodies, no item: stats")
        FP.assert_footprint(cur_w, cur, torch.zeros((1, cur.numel()), dtype=torch.bool), f"{nb} bodies, no item: cur")


@pytest.mark.parametrize("counts", [(64,), (5, 257), (64, 3, 1000, 65, 255)], ids=lambda c: "-".join(map(str, c)))
def test_the_geometry_is_the_restatements(counts):
    c = cloud(counts)
    op, geo = c["visc"], c["geo"]
    assert op.n_bodies == len(counts) and op.n_items == sum(counts) and op.gradient is c["mg"]
    assert op.body_offsets.tolist() == geo["body_offsets"].tolist() and op.items.tolist() == geo["items"].tolist()
    R.same(op.area, geo["area"], "area")
    assert float(op.area.sum(0).abs().max()) == 0.0
    ulp = np.spacing(np.abs(geo["unit"]))
    worst = R.within(op.unit, geo["unit"], ulp, "unit")
    print(f"bodies {counts}: unit against the restatement, measured / one ulp = {worst:.3f}")
    R.within(op.angle, geo["angle"], 64 * 2.0 ** -52 * np.pi * np.ones_like(geo["angle"]), "angle")          # (the library's atan2, the mean's own order)
    # arm = pos - the mean of the body's nodes: a sum of n coordinates in another order, 2 (n + 4) 2^-53 max|pos| at the most
    R.within(op.arm, geo["arm"], 2 * (max(counts) + 4) * 2.0 ** -53 * float(np.abs(c["pos"]).max()) * np.ones_like(geo["arm"]), "arm")
    for b in range(len(counts)):
        a, e = geo["body_offsets"][b], geo["body_offsets"][b + 1]
        assert bool((op.angle[a:e].diff() > 0).all())
    # forces / wall / history of the class are the launch
    x = c["target"]
    tree, _, _, rwall, _, _ = ref_of(c, x, 2, NF, True)
    step = x[:, 2 * NF:3 * NF]
    R.same(op.forces(step), tree, "forces()")
    R.same(op.wall(step), rwall, "wall()")
    hist = op.history(x, STEPS)
    assert tuple(hist.shape) == (STEPS, len(counts), 6)
    R.same(hist[2], tree, "history()[2]")
    with pytest.raises(ValueError, match="^x"):
        op.forces(x[:-1])
    with pytest.raises(ValueError, match="^nf"):
        op.history(x, STEPS, nf=2)
    with pytest.raises(ValueError, match="^n:"):
        op.history(x, 0)
