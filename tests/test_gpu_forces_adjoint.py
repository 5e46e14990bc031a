"""g4c_body_forces_adjoint (csrc/body_forces.hip) through ops.body_forces_adjoint and gfd.BodyForces.adjoint against the numpy
restatement of tests/forces_adjoint_ref.py.

The launch is bit for bit the restatement's loops — compared as integers (−0 is not +0), with gx and the scratch hw in guard arenas
(tests/footprint.py: every element of the window written, nothing around it) and every input frozen.  The shapes are the smallest at
which the kernels can go wrong: own-lists and in-lists of 0, 1, 3, 4, 5 and 9 entries around the unroll of four, a degenerate wall
node, a node no table names, a node that is an item of two bodies, a sender that feeds more wall items than a workgroup has threads,
bodies of 3, 256 and 257 items, nf = 3, 4, 5 with the columns permuted, mu == 0 without gradient tables, either or both incoming
gradients missing, no nodes, no items, and once more nodes than the grid covers in one pass."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

import footprint as FP                                   # noqa: E402
import forces_adjoint_ref as A                           # noqa: E402
import forces_ref as FR                                  # noqa: E402
import gradient_ref as GR                                # noqa: E402
import graphs4cfd_amd as gfd                             # noqa: E402
from graphs4cfd_amd import _lib, ops, synthetic as S     # noqa: E402

DEV = torch.device("cuda", 0)
F32, F64, I32 = torch.float32, torch.float64, torch.int32
SCALE, SHIFT, MU = [1.5, 0.75, 2.5], [0.25, -0.5, 0.125], 0.03125 * 1.3
COLUMNS = {3: dict(pcol=2, ucol=0, vcol=1), 4: dict(pcol=1, ucol=3, vcol=0), 5: dict(pcol=0, ucol=2, vcol=4)}


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_bits(got, ref, what=""):
    """Equal as integers: −0 is not +0, and a NaN equals only the same NaN."""
    g = got.detach().cpu().numpy() if hasattr(got, "detach") else np.asarray(got)
    ref = np.ascontiguousarray(ref)
    assert g.dtype == ref.dtype == np.float32 and g.shape == ref.shape, f"{what}: {g.dtype} {g.shape} vs {ref.dtype} {ref.shape}"
    bad = np.ascontiguousarray(g).view(np.int32) != ref.view(np.int32)
    if bad.any():
        pos = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ in their bits, first at {list(pos)}: got {g[pos]!r} want {ref[pos]!r}")


def run(geo, tabs, n_nodes, nf, gF, gwall, what, *, mu, off=None, g=None, consts=None, check=True):
    """One checked launch on numpy tables: the device's gx [N, nf] as numpy.  With mu == 0 the gradient's tables are not passed at all."""
    c = dict(COLUMNS[nf], mu=mu, p_scale=SCALE[2], u_scale=SCALE[0], v_scale=SCALE[1])
    c.update(consts or {})
    viscous = mu != 0
    n_items, n_bodies = int(geo["items"].size), int(geo["n_bodies"])
    d = {k: dev(v) for k, v in tabs.items()}
    ins = dict(gF=dev(gF), gwall=dev(gwall), area=dev(geo["area"]), unit=dev(geo["unit"]), arm=dev(geo["arm"]), g=dev(g) if viscous else None,
               off=dev(off) if viscous else None)
    gx, whole = FP.arena(n_nodes, nf, F32, col0=0, pad_cols=0, device=DEV)
    hw, hw_whole = FP.arena(n_items, 5, F32, col0=0, pad_cols=0, device=DEV)
    with FP.frozen(*ins.values(), *d.values(), what=what):
        got = ops.body_forces_adjoint(ins["gF"], ins["gwall"], d["item_body"], ins["area"], ins["unit"], ins["arm"], d["own_off"], d["own_item"],
                                      n_bodies, nf, **c, g=ins["g"], off=ins["off"], in_off=d.get("in_off") if viscous else None,
                                      in_item=d.get("in_item") if viscous else None, in_g=d.get("in_g") if viscous else None, hw=hw, out=gx)
        torch.cuda.synchronize(DEV)
    assert got is gx
    FP.assert_footprint(whole, gx, what=what + ": gx")          # every element of every row written, nothing outside
    live = n_nodes > 0 and n_items > 0 and n_bodies > 0 and (gF is not None or gwall is not None)
    FP.assert_footprint(hw_whole, hw, None if live else range(0), what=what + ": hw")
    ref_c = dict(c, off=off, g=g)
    if live:
        H, cp, _, _ = A.stage(gF, gwall, geo, tabs["item_body"], **ref_c)
        same_bits(hw, np.concatenate([H.astype(np.float32), cp.astype(np.float32)[:, None]], axis=1), what + ": hw")
    if check:
        same_bits(gx, A.adjoint32(gF, gwall, geo, tabs, n_nodes, nf, **ref_c), what)
        want, bound = A.adjoint64(gF, gwall, geo, tabs, n_nodes, nf, **ref_c)
        FR.within(gx, want, bound, what + ", fp64")
    return gx.cpu().numpy()


@functools.lru_cache(maxsize=None)
def synthetic(n_nodes=700, n_items=620, n_bodies=3):
    geo, off, src, g = A.synthetic(n_nodes, n_items, n_bodies)
    return geo, off, src, g, A.node_tables(geo["items"], geo["body_offsets"], n_nodes, off, src, g)


# ====================================================================== the launch on synthetic tables
@pytest.mark.parametrize("nf", [3, 4, 5])
def test_the_adjoint_launch_matches_the_restatement(nf):
    geo, off, src, g, tabs = synthetic()
    n = 700
    assert tuple(np.diff(tabs["own_off"])[:6]) == A.LIST_LENGTHS and tuple(np.diff(tabs["in_off"])[6:12]) == A.LIST_LENGTHS
    assert np.diff(tabs["in_off"])[13] == A.HUB > 256 and np.diff(tabs["own_off"])[12] == np.diff(tabs["in_off"])[12] == np.diff(off)[12] == 0
    gF, gw = A.incoming(3, 620, seed=nf)
    cols = COLUMNS[nf]
    for a, b, name in ((gF, gw, "both"), (gF, None, "gwall NULL"), (None, gw, "gF NULL")):
        gx = run(geo, tabs, n, nf, a, b, f"nf {nf} {name}", mu=MU, off=off, g=g)
        assert not gx[12].view(np.int32).any()          # the node no table names: +0
        spare = [c for c in range(nf) if c not in cols.values()]
        assert not gx[:, spare].view(np.int32).any()    # the columns nobody names: +0, the sign bit clear
        assert gx[13, cols["ucol"]] != 0 and gx[13, cols["pcol"]] == 0          # the hub sends, it is no wall node
        # mu == 0: NULL gradient tables, the velocity columns +0 and nothing of them read
        gx = run(geo, tabs, n, nf, a, b, f"nf {nf} {name} inviscid", mu=0.0)
        assert not gx[:, [c for c in range(nf) if c != cols["pcol"]]].view(np.int32).any() and gx[:, cols["pcol"]].any()
    gx = run(geo, tabs, n, nf, None, None, f"nf {nf} no gradient", mu=MU, off=off, g=g)
    assert not gx.view(np.int32).any()                  # both NULL: zero-filled, the sign bit clear
    zero = run(geo, tabs, n, nf, np.zeros((3, 6)), -np.zeros((620, 2), np.float32), f"nf {nf} zeros", mu=MU, off=off, g=g)
    assert not zero.any()                               # (zeros given: −0 may arrive, the restatement has its bits)


def test_more_nodes_than_the_grid_covers_in_one_pass():
    n = A.BIG
    assert n > 262_144
    geo, off, src, g = A.synthetic(n, 2000, 2)
    tabs = A.node_tables(geo["items"], geo["body_offsets"], n, off, src, g)
    gF, gw = A.incoming(2, 2000)
    gx = run(geo, tabs, n, 5, gF, gw, "big", mu=MU, off=off, g=g)
    assert gx[262_144:].any()


def test_no_nodes_no_items_no_bodies():
    geo, off, src, g, tabs = synthetic()
    empty = dict(items=np.zeros(0, np.int64), body_offsets=np.zeros(1, np.int32), area=np.zeros((0, 2)), unit=np.zeros((0, 2)),
                 arm=np.zeros((0, 2)), n_bodies=0)
    for n in (1, 300):          # W = 0 (and B = 0): zero-filled
        t = A.node_tables(empty["items"], empty["body_offsets"], n, np.zeros(n + 1, np.int32), np.zeros(0, np.int32), np.zeros((0, 2), np.float32))
        for mu in (0.0, MU):
            gx = run(empty, t, n, 3, np.zeros((0, 6)), np.zeros((0, 2), np.float32), f"W = 0, N = {n}", mu=mu, off=np.zeros(n + 1, np.int32),
                     g=np.zeros((0, 2), np.float32), check=False)
            assert gx.shape == (n, 3) and not gx.view(np.int32).any()
    t = A.node_tables(empty["items"], empty["body_offsets"], 0, np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros((0, 2), np.float32))
    gx = run(empty, t, 0, 4, None, None, "N = 0", mu=MU, off=np.zeros(1, np.int32), g=np.zeros((0, 2), np.float32), check=False)
    assert gx.shape == (0, 4)


def test_captured_and_eager_runs_give_the_same_bits():
    geo, off, src, g, tabs = synthetic()
    gF, gw = A.incoming(3, 620, seed=9)
    d = {k: dev(v) for k, v in tabs.items()}
    args = (dev(gF), dev(gw), d["item_body"], dev(geo["area"]), dev(geo["unit"]), dev(geo["arm"]), d["own_off"], d["own_item"], 3, 3)
    kw = dict(COLUMNS[3], mu=MU, p_scale=SCALE[2], u_scale=SCALE[0], v_scale=SCALE[1], g=dev(g), off=dev(off), in_off=d["in_off"],
              in_item=d["in_item"], in_g=d["in_g"])
    eager = ops.body_forces_adjoint(*args, **kw)
    again = ops.body_forces_adjoint(*args, **kw)
    out, hw = torch.full((700, 3), float("nan"), device=DEV), torch.empty((620, 5), device=DEV)
    torch.cuda.synchronize(DEV)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):          # one stream: the two launches in order, no parallel branches
            ops.body_forces_adjoint(*args, **kw, hw=hw, out=out)
    torch.cuda.current_stream(DEV).wait_stream(side)
    graph.replay()
    torch.cuda.synchronize(DEV)
    for t in (again, out):
        assert torch.equal(t.view(I32), eager.view(I32))
    same_bits(out, A.adjoint32(gF, gw, geo, tabs, 700, 3, **dict(COLUMNS[3], mu=MU, p_scale=SCALE[2], u_scale=SCALE[0], v_scale=SCALE[1], off=off, g=g)),
              "captured")


# ====================================================================== gfd.BodyForces.adjoint on a real mesh
_cache = {}


def cloud(counts=(3, 256, 257), twice=False, order=None):
    """An annulus round bodies of `counts` wall nodes, the device's kNN thinned to a ragged in-degree, one wall node without in-edges;
    `twice`: the bodies as loops=, the first node of body 1 also closing body 0 (a node that is an item of two bodies); `order`: a
    renumbering of the nodes (new row of every old row)."""
    key = (counts, twice, None if order is None else "renumbered")
    if key in _cache:
        return _cache[key]
    pos, wall, label = FR.annulus(500, counts, seed=len(counts))
    g0 = gfd.Graph(pos=torch.from_numpy(pos).to(DEV))
    ei, _ = S.connect_knn(g0.pos, 6)
    keep = torch.from_numpy(np.random.default_rng(sum(counts)).random(int(ei.size(1))) > 0.15).to(DEV)
    lone = int(wall[len(wall) // 2])
    keep &= ei[1] != lone
    ei = ei[:, keep].contiguous()
    if order is not None:
        new = torch.from_numpy(order).to(DEV)
        inv = np.argsort(order)
        pos, wall, lone = pos[inv], order[wall], int(order[lone])
        ei = new[ei]
        ei = ei[:, torch.argsort(ei[1], stable=True)].contiguous()          # grouped by receiver again, each node's in-edges in their old order
    g = gfd.Graph(pos=torch.from_numpy(pos).to(DEV), edge_index=ei)
    mg = gfd.MeshGradient(g)
    geo = FR.geometry(pos, nodes=wall, labels=label)
    kw = dict(scale=SCALE, shift=SHIFT)
    if twice:
        bo = geo["body_offsets"]
        loops = [geo["items"][a:b].copy() for a, b in zip(bo[:-1], bo[1:])]
        loops[0] = np.concatenate([loops[0], loops[1][:1]])
        geo = FR.geometry(pos, loops=loops)
        kw.update(loops=[torch.from_numpy(lp).to(DEV) for lp in loops])
    else:
        kw.update(nodes=torch.from_numpy(wall).to(DEV), bodies=torch.from_numpy(label).to(DEV))
    visc, inviscid = gfd.BodyForces(g, mu=MU, gradient=mg, **kw), gfd.BodyForces(g, **kw)
    assert visc.items.tolist() == geo["items"].tolist()
    tables = dict(geo, area=visc.area.cpu().numpy(), unit=visc.unit.cpu().numpy(), arm=visc.arm.cpu().numpy())          # the device's own
    mesh = dict(off=mg.off.cpu().numpy(), g=mg.g.cpu().numpy(), src=mg.src.cpu().numpy())
    out = dict(g=g, mg=mg, pos=pos, wall=wall, lone=lone, geo=tables, mesh=mesh, visc=visc, inviscid=inviscid, n=len(pos))
    _cache[key] = out
    return out


def consts(nf=3, mu=MU):
    return dict(pcol=2, ucol=0, vcol=1, mu=mu, p_scale=SCALE[2], u_scale=SCALE[0], v_scale=SCALE[1])


@pytest.mark.parametrize("twice", [False, True], ids=["bodies", "a node of two bodies"])
def test_body_forces_adjoint(twice):
    c = cloud(twice=twice)
    n, geo, mesh, op = c["n"], c["geo"], c["mesh"], c["visc"]
    assert np.diff(geo["body_offsets"]).tolist() == ([4, 256, 257] if twice else [3, 256, 257])
    x = torch.randn(n, 3, generator=torch.Generator().manual_seed(3)).to(DEV)
    op.forces(x), op.wall(x)
    assert op._adjoint_tables is None                               # the plain forward builds nothing for the adjoint
    tabs = A.node_tables(geo["items"], geo["body_offsets"], n, mesh["off"], mesh["src"], mesh["g"])
    assert (np.diff(tabs["own_off"]).max() == 2) == twice
    gF, gw = A.incoming(3, geo["items"].size, seed=twice)
    wide = torch.zeros(geo["items"].size, 4, device=DEV)
    wide[:, 1:3] = dev(gw)
    for given in (dev(gw), wide[:, 1:3]):                           # dense, a column slice
        with FP.frozen(given, op.area, op.unit, op.arm, c["mg"].g, c["mg"].off, what="adjoint"):
            gx = op.adjoint(dev(gF), given)
        assert tuple(gx.shape) == (n, 3) and gx.is_contiguous()
        same_bits(gx, A.adjoint32(gF, gw, geo, tabs, n, 3, **consts(), off=mesh["off"], g=mesh["g"]), f"twice {twice}")
    got = op._adjoint_tables
    assert op._node_side() is got                                   # built once, kept
    for name, want in tabs.items():
        FR.same(got[name], want, name)
    # nf defaults to len(scale); a wider nf leaves the spare columns +0; gF or gwall alone; the pressure-only operator
    same_bits(op.adjoint(dev(gF), None, nf=5)[:, :3].contiguous(), A.adjoint32(gF, None, geo, tabs, n, 3, **consts(), off=mesh["off"], g=mesh["g"]), "gF")
    assert not op.adjoint(dev(gF), None, nf=5)[:, 3:].view(I32).any()
    same_bits(op.adjoint(gwall=dev(gw)), A.adjoint32(None, gw, geo, tabs, n, 3, **consts(), off=mesh["off"], g=mesh["g"]), "gwall")
    assert not op.adjoint().view(I32).any()
    inv = c["inviscid"]
    same_bits(inv.adjoint(dev(gF), dev(gw)), A.adjoint32(gF, gw, geo, tabs, n, 3, **consts(mu=0.0)), "inviscid")
    assert "in_off" not in inv._adjoint_tables
    # ⟨J x, (gF, gwall)⟩ = ⟨x, Jᵀ(gF, gwall)⟩ on the device's own outputs: the forward's fp32 gradient and the adjoint's fp32 sums within
    # their bounds
    zero = torch.zeros_like(x)
    lhs = A.inner((op.forces(x) - op.forces(zero)).cpu().numpy(), (op.wall(x).double() - op.wall(zero).double()).cpu().numpy(), gF, gw)
    xs = x.cpu().numpy()
    rhs = float((xs.astype(np.float64) * gx.cpu().numpy().astype(np.float64)).sum())
    ref = A.ForceRef(geo, n, dict(consts(), p_shift=SHIFT[2], **mesh), wall={"pressure": 1.0, "shear": 1.0}, components=("fx", "fy", "m"))
    _, _, _, Gm = A.forward64(xs, geo, **ref.c)
    eF6, eW = ref._forward_errors(xs.astype(np.float64), np.zeros_like(xs, np.float64), Gm, 0 * Gm)
    # (|gF| on each of the six sums is at most |gF_p| + |gF_v| on their total: eF6 bounds the totals' errors)
    gtot = np.stack([np.abs(gF[:, [0, 2]]).max(1), np.abs(gF[:, [1, 3]]).max(1), np.abs(gF[:, [4, 5]]).max(1)], axis=1)
    bound = A.adjoint64(gF, gw, geo, tabs, n, 3, **consts(), off=mesh["off"], g=mesh["g"])[1]
    allowed = float((eF6 * gtot).sum() + (eW * np.abs(gw)).sum() + (bound * np.abs(xs)).sum()) * (1 + 1e-6)
    assert abs(lhs - rhs) <= allowed, (lhs, rhs, allowed)
    assert abs(lhs) > 1e2 * allowed


def test_the_velocity_columns_are_the_mesh_adjoint_of_the_staged_rows():
    """Every node an item at most once: gx[:, (u, v)] has the bits of MeshGradient.adjoint applied to a dense [N, 4] tensor that holds
    H_w at the wall rows (its extra terms are g · (+0)); the pressure column is an indexed add of cp."""
    c = cloud()
    n, geo, op = c["n"], c["geo"], c["visc"]
    gF, gw = A.incoming(3, geo["items"].size, seed=5)
    hw = torch.empty((geo["items"].size, 5), device=DEV)
    gx = op._adjoint(dev(gF), dev(gw), 3, hw=hw)
    dense = torch.zeros((n, 4), device=DEV)
    dense[op.items] = hw[:, :4]
    composed = c["mg"].adjoint(dense, ("grad:0", "grad:1"), 3, field_scale=None)
    assert torch.equal(composed[:, :2].contiguous().view(I32), gx[:, :2].contiguous().view(I32))
    assert not composed[:, 2].view(I32).any()
    p = torch.zeros(n, device=DEV).index_add_(0, op.items, hw[:, 4])
    assert torch.equal(p.view(I32), gx[:, 2].contiguous().view(I32))


def test_a_renumbered_mesh_gives_the_permuted_result():
    """The pressure column follows the wall's own order: the same bits at the new rows.  A node's in-list follows the CSR positions,
    which the renumbering reorders: the velocity columns are bit for bit the restatement on the renumbered tables, and the two results
    sit within their two bounds of each other."""
    c = cloud()
    n = c["n"]
    order = np.random.default_rng(8).permutation(n)
    r = cloud(order=order)
    assert r["geo"]["items"].tolist() == order[c["geo"]["items"]].tolist()          # the same wall, the same item order
    gF, gw = A.incoming(3, c["geo"]["items"].size, seed=6)
    a, b = c["visc"].adjoint(dev(gF), dev(gw)).cpu().numpy(), r["visc"].adjoint(dev(gF), dev(gw)).cpu().numpy()
    tabs = A.node_tables(r["geo"]["items"], r["geo"]["body_offsets"], n, r["mesh"]["off"], r["mesh"]["src"], r["mesh"]["g"])
    same_bits(b, A.adjoint32(gF, gw, r["geo"], tabs, n, 3, **consts(), off=r["mesh"]["off"], g=r["mesh"]["g"]), "renumbered")
    same_bits(b[order][:, 2], a[:, 2], "pressure column")
    tabs0 = A.node_tables(c["geo"]["items"], c["geo"]["body_offsets"], n, c["mesh"]["off"], c["mesh"]["src"], c["mesh"]["g"])
    b0 = A.adjoint64(gF, gw, c["geo"], tabs0, n, 3, **consts(), off=c["mesh"]["off"], g=c["mesh"]["g"])[1]
    b1 = A.adjoint64(gF, gw, r["geo"], tabs, n, 3, **consts(), off=r["mesh"]["off"], g=r["mesh"]["g"])[1]
    # (the weights g of the renumbered mesh are the same numbers: the fp64 normal matrix of a node adds its in-edges in their old order)
    assert (np.abs(b[order].astype(np.float64) - a) <= b0 + b1[order]).all() and np.abs(a[:, :2]).max() > 0


# ====================================================================== refusals
def test_refusals_return_their_code_without_launching():
    lib = _lib.load()
    import ctypes as C
    geo, off, src, g, tabs = synthetic()
    n, n_items, nb, nf = 700, 620, 3, 3
    gF, gw = A.incoming(nb, n_items)
    d = {k: dev(v) for k, v in tabs.items()}
    keep = dict(gF=dev(gF), gwall=dev(gw), g=dev(g), off=dev(off), area=dev(geo["area"]), unit=dev(geo["unit"]), arm=dev(geo["arm"]),
                hw=torch.empty((n_items, 5), device=DEV), **d)
    gx, whole = FP.arena(n, nf, F32, col0=0, pad_cols=0, device=DEV)
    big = torch.ones(n * nf + n_items * 5 + 64, device=DEV)          # gx and another buffer inside one allocation: their ranges are known

    def call(sizes=None, **kw):
        a = dict(nf=nf, pcol=2, ucol=0, vcol=1, mu=MU, p_scale=1.0, u_scale=1.0, v_scale=1.0, gx=gx.data_ptr())
        a.update({k: v.data_ptr() for k, v in keep.items()})
        a.update(kw)
        s = dict(n_nodes=n, n_bodies=nb, n_items=n_items, n_entries=int(tabs["in_item"].size))
        s.update(sizes or {})
        rc = lib.g4c_body_forces_adjoint(C.byref(_lib.g4c_body_forces_adjoint_t(**a)), s["n_nodes"], s["n_bodies"], s["n_items"], s["n_entries"],
                                         _lib.stream_handle(DEV))
        return rc, lib.g4c_last_error().decode()

    cases = [(dict(sizes=dict(n_nodes=-1)), "bad sizes"), (dict(sizes=dict(n_bodies=-1)), "bad sizes"), (dict(sizes=dict(n_items=-1)), "bad sizes"),
             (dict(sizes=dict(n_entries=-1)), "bad sizes"), (dict(sizes=dict(n_entries=2 ** 31)), "bad sizes"), (dict(nf=0), "bad sizes"),
             (dict(pcol=3), "pcol"), (dict(pcol=-1), "pcol"), (dict(ucol=3), "ucol"), (dict(vcol=-1), "vcol"),
             (dict(ucol=2), "not distinct"), (dict(vcol=0), "not distinct"), (dict(pcol=1), "not distinct"),
             (dict(gx=None), "null"), (dict(item_body=None), "null"), (dict(area=None), "null"), (dict(arm=None), "null"), (dict(unit=None), "null"),
             (dict(own_off=None), "null"), (dict(own_item=None), "null"), (dict(hw=None), "null"),
             (dict(g=None), "mu != 0"), (dict(off=None), "mu != 0"), (dict(in_off=None), "mu != 0"), (dict(in_item=None), "mu != 0"),
             (dict(in_g=None), "mu != 0"),
             (dict(gx=keep["gwall"].data_ptr()), "aliases gwall"), (dict(gx=keep["hw"].data_ptr()), "aliases hw"),
             (dict(gx=keep["gF"].data_ptr()), "aliases gF"),
             (dict(gx=big.data_ptr(), hw=big.data_ptr() + 4 * (n * nf - 1)), "aliases hw"),                    # the last element of gx
             (dict(hw=big.data_ptr(), gx=big.data_ptr() + 4 * (n_items * 5 - 1)), "aliases hw"),              # the last element of hw
             (dict(gx=big.data_ptr(), gwall=big.data_ptr() + 4 * (n * nf - 1)), "aliases gwall")]
    for kw, word in cases:
        rc, msg = call(**kw)
        assert rc == _lib.EINVAL and "g4c_body_forces_adjoint" in msg and word in msg, (kw, rc, msg)
    rc = lib.g4c_body_forces_adjoint(None, n, nb, n_items, 0, _lib.stream_handle(DEV))
    assert rc == _lib.EINVAL and "g4c_body_forces_adjoint" in lib.g4c_last_error().decode()
    torch.cuda.synchronize(DEV)
    FP.assert_footprint(whole, gx, written_rows=range(0), what="refusals")          # nothing was written
    assert call(sizes=dict(n_nodes=0), gx=None)[0] == _lib.OK                       # no nodes: nothing launched
    assert call(mu=0.0, ucol=2, vcol=2, g=None, off=None, in_off=None, in_item=None, in_g=None, unit=None)[0] == _lib.OK          # mu == 0 reads none of them
    torch.cuda.synchronize(DEV)
