"""g4c_sample_points_adjoint (csrc/point_sample.hip) through ops.sample_points_adjoint and gfd.PointSampler.adjoint against the numpy
restatement of tests/sample_adjoint_ref.py.

The launch is bit for bit the restatement's numpy.float32 loop — compared as integers (−0 is not +0), with gx in a guard arena
(tests/footprint.py: every element of the window written, nothing around it) and gy and the tables frozen.  The shapes are the smallest
at which the kernel can go wrong: lists of 0, 1, 3, 4, 5 and 9 entries around the unroll of four, a node nobody uses, a hub whose list
is longer than a workgroup, F at the chunk edges, k = 1, 6, 16, and once more items than the grid covers in one pass."""
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
import sample_adjoint_ref as A                           # noqa: E402
import sampler_ref as SR                                 # noqa: E402
import graphs4cfd_amd as gfd                             # noqa: E402
from graphs4cfd_amd import _lib, ops                     # noqa: E402

DEV = torch.device("cuda", 0)
F32, I32 = torch.float32, torch.int32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_bits(got, ref, what=""):
    """Equal as integers: −0 is not +0, and a NaN equals only the same NaN."""
    g = got.detach().cpu().numpy() if hasattr(got, "detach") else np.asarray(got)
    ref = np.ascontiguousarray(ref)
    assert g.dtype == ref.dtype == np.float32 and g.shape == ref.shape, f"{what}: {g.dtype} {g.shape} vs {ref.dtype} {ref.shape}"
    bad = np.ascontiguousarray(g).view(np.int32) != ref.view(np.int32)
    if bad.any():
        pos = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ in their bits, first at {list(pos)}: got {g[pos]!r} want {ref[pos]!r}")


@functools.lru_cache(maxsize=None)
def cases():
    return A.cases()


def run(tables, n_nodes, gy, what, check=True):
    """One checked launch on the node-side tables (numpy): the device's gx [N, F] as numpy."""
    n_points, nf = gy.shape
    ins = [dev(gy), dev(tables[0]), dev(tables[1]), dev(tables[2])]
    gx, whole = FP.arena(n_nodes, nf, F32, col0=0, pad_cols=0, device=DEV)
    with FP.frozen(*ins, what=what):
        got = ops.sample_points_adjoint(ins[0], ins[1], ins[2], ins[3], n_nodes, out=gx)
        torch.cuda.synchronize(DEV)
    assert got is gx
    FP.assert_footprint(whole, gx, what=what)          # every element of every row written, nothing outside
    if check:
        same_bits(gx, A.adjoint32(gy, *tables), what)
    return gx.cpu().numpy()


@pytest.mark.parametrize("k", [1, 6, 16])
def test_the_adjoint_launch_matches_the_restatement(k):
    idx, coef, n_nodes, widths = cases()[f"synthetic k={k}"]
    tables = A.node_tables(idx, coef, n_nodes)
    assert tuple(np.diff(tables[0])[:7]) == A.LIST_LENGTHS + (0,)          # around the unroll, and two nodes nobody uses
    for nf in widths:          # 1, 3, 4, 5, 9: the chunk edges
        gx = run(tables, n_nodes, A.gy_of(idx.shape[1], nf), f"k {k} F {nf}")
        assert not gx[[0, 6]].view(np.int32).any()          # +0: the sign bit clear
        want, bound = A.adjoint64(A.gy_of(idx.shape[1], nf), *tables)
        SR.within(gx, want, bound, f"k {k} F {nf}, fp64")


@pytest.mark.parametrize("dim", [2, 3])
def test_a_hub_longer_than_a_workgroup(dim):
    idx, coef, n_nodes, widths = cases()[f"hub {dim}-D"]
    tables = A.node_tables(idx, coef, n_nodes)
    assert np.diff(tables[0]).max() >= 600
    for nf in widths:
        run(tables, n_nodes, A.gy_of(idx.shape[1], nf), f"hub {dim}-D F {nf}")


def test_more_items_than_the_grid_covers_in_one_pass():
    idx, coef, n_nodes, (nf,) = cases()["big"]
    assert n_nodes * ((nf + 3) // 4) > 262_144
    run(A.node_tables(idx, coef, n_nodes), n_nodes, A.gy_of(idx.shape[1], nf), "big")


def test_no_nodes_and_no_points():
    empty = (np.zeros(1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))
    gx = run(empty, 0, np.zeros((5, 3), np.float32)[:0], "N = 0", check=False)
    assert gx.shape == (0, 3)
    gx = ops.sample_points_adjoint(torch.ones(7, 3, device=DEV), torch.zeros(1, dtype=I32, device=DEV), torch.zeros(14, dtype=I32, device=DEV),
                                   torch.ones(14, device=DEV), 0)          # points, no nodes: nothing is launched
    assert tuple(gx.shape) == (0, 3)
    for n, nf in ((1, 1), (300, 5)):          # no points: zero-filled, +0
        tables = (np.zeros(n + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float32))
        gx = run(tables, n, np.zeros((0, nf), np.float32), f"P = 0, N = {n}")
        assert gx.shape == (n, nf) and not gx.view(np.int32).any()


def test_captured_and_eager_runs_give_the_same_bits():
    idx, coef, n_nodes, _ = cases()["hub 2-D"]
    tables = [dev(t) for t in A.node_tables(idx, coef, n_nodes)]
    gy = dev(A.gy_of(idx.shape[1], 3))
    eager = ops.sample_points_adjoint(gy, *tables, n_nodes)
    again = ops.sample_points_adjoint(gy, *tables, n_nodes)
    out = torch.full((n_nodes, 3), float("nan"), device=DEV)
    torch.cuda.synchronize(DEV)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):          # one stream: no parallel branches
            ops.sample_points_adjoint(gy, *tables, n_nodes, out=out)
    torch.cuda.current_stream(DEV).wait_stream(side)
    graph.replay()
    torch.cuda.synchronize(DEV)
    for t in (again, out):
        assert torch.equal(t.view(I32), eager.view(I32))
    same_bits(out, A.adjoint32(A.gy_of(idx.shape[1], 3), *A.node_tables(idx, coef, n_nodes)), "captured")


# ====================================================================== gfd.PointSampler.adjoint
@pytest.mark.parametrize("dim,k", [(2, 6), (3, 10), (2, 1)])
def test_point_sampler_adjoint(dim, k):
    pos, pts, _, _ = A.hub(dim)
    n, n_points = pos.shape[0], pts.shape[0]
    s = gfd.PointSampler(gfd.Graph(pos=dev(pos)), dev(pts), k=k)
    x = dev(np.random.default_rng(3).standard_normal((n, 3)).astype(np.float32))
    fwd = s.sample(x)
    assert s._adjoint_tables is None                             # the plain forward builds nothing for the adjoint
    idx, coef = s._idx.cpu().numpy(), s._coef.cpu().numpy()      # the device's own tables (pinned by tests/test_gpu_point_sampler.py)
    tables = A.node_tables(idx, coef, n)
    gy = A.gy_of(n_points, 3, seed=1)
    wide = torch.zeros(n_points, 5, device=DEV)
    wide[:, 1:-1] = dev(gy)
    for given in (dev(gy), wide[:, 1:-1], dev(gy.T.copy()).t()):          # dense, a column slice, a transposed view
        with FP.frozen(given, s._idx, s._coef, what=f"dim {dim}"):
            gx = s.adjoint(given)
        assert tuple(gx.shape) == (n, 3) and gx.is_contiguous()
        same_bits(gx, A.adjoint32(gy, *tables), f"dim {dim} k {k}")
    got = s._adjoint_tables
    assert s._node_side()[2] is got[2]                            # built once, kept
    for g, want, name in zip(got, tables, ("in_off", "in_pt", "in_coef")):
        SR.same(g, want, name)
    # from_tables: the same tables, no search, the same bits
    t = gfd.PointSampler.from_tables(s._idx, s._coef, n, points=s.points, distance=s.distance, degenerate=s.degenerate)
    assert t.n_points == n_points and t.k == k and torch.equal(t.sample(x).view(I32), fwd.view(I32))
    assert torch.equal(t.adjoint(dev(gy)).view(I32), gx.view(I32))
    # ⟨S x, y⟩ = ⟨x, Sᵀ y⟩ on the device's own outputs, within the two fp32 bounds
    xs = x.cpu().numpy()
    mag = SR.apply64(xs, idx.T, coef.T)[1]
    bound = A.adjoint64(gy, *tables)[1]
    lhs = float((fwd.cpu().numpy().astype(np.float64) * gy).sum())
    rhs = float((xs.astype(np.float64) * gx.cpu().numpy().astype(np.float64)).sum())
    allowed = float((SR.bound32(mag, k) * np.abs(gy)).sum() + (bound * np.abs(xs)).sum()) * (1 + 1e-6)
    assert abs(lhs - rhs) <= allowed, (lhs, rhs, allowed)


def test_tables_that_are_grouped_already():
    """A flattened idx that is ascending needs no permutation (`plan.gather_csr` returns none): in_pt is the position mod P."""
    idx = np.array([[0, 0, 1], [2, 2, 3]], np.int32)          # k = 2, P = 3, node 4 unused
    coef = np.array([[1.5, -2.0, 0.25], [3.0, -0.5, 4.0]], np.float32)
    s = gfd.PointSampler.from_tables(dev(idx), dev(coef), 5)
    gy = A.gy_of(3, 5)
    tables = A.node_tables(idx, coef, 5)
    same_bits(s.adjoint(dev(gy)), A.adjoint32(gy, *tables), "grouped")
    for g, want, name in zip(s._adjoint_tables, tables, ("in_off", "in_pt", "in_coef")):
        SR.same(g, want, name)
    x = np.random.default_rng(2).standard_normal((5, 5)).astype(np.float32)
    same_bits(s.sample(dev(x)), SR.apply32(x, idx.T, coef.T), "forward")


def test_argument_errors():
    with pytest.raises(ValueError, match="gy"):
        ops.sample_points_adjoint(torch.ones(4, 3, device=DEV, dtype=torch.float64), torch.zeros(9, dtype=I32, device=DEV),
                                  torch.zeros(8, dtype=I32, device=DEV), torch.ones(8, device=DEV), 8)
    gy = torch.ones(4, 3, device=DEV)
    off, pt, cf = torch.zeros(9, dtype=I32, device=DEV), torch.zeros(8, dtype=I32, device=DEV), torch.ones(8, device=DEV)
    for kw, word in ((dict(in_off=off[:-1]), "in_off"), (dict(in_pt=pt[:7]), "in_pt"), (dict(in_coef=cf[:4]), "in_coef"),
                     (dict(in_pt=pt.long()), "in_pt"), (dict(gy=torch.ones(4, 6, device=DEV)[:, ::2]), "gy"),
                     (dict(out=torch.ones(8, 4, device=DEV)), "out"), (dict(gy=gy.cpu()), "gy"), (dict(n_nodes=-1), "n_nodes")):
        a = dict(gy=gy, in_off=off, in_pt=pt, in_coef=cf, n_nodes=8)
        a.update(kw)
        with pytest.raises(ValueError, match=word):
            ops.sample_points_adjoint(**a)
    both = torch.ones(8, 3, device=DEV)
    with pytest.raises(ValueError, match="shares its storage"):
        ops.sample_points_adjoint(both[:4], off[:5], pt, cf, 4, out=both[4:])
    s = gfd.PointSampler(gfd.Graph(pos=dev(SR.cloud(65, 2))), dev(SR.queries(9, 2)))
    for bad in (torch.ones(9, 3), torch.ones(8, 3, device=DEV), torch.ones(9, 3, device=DEV, dtype=torch.float64), torch.ones(9, device=DEV)):
        with pytest.raises(ValueError, match="gy"):
            s.adjoint(bad)


def test_refusals_return_their_code_without_launching():
    lib = _lib.load()
    n, n_points, nf = 64, 32, 3
    gy, pt, cf = torch.ones(n_points, nf, device=DEV), torch.zeros(2 * n_points, dtype=I32, device=DEV), torch.ones(2 * n_points, device=DEV)
    off = torch.arange(0, n + 1, dtype=I32, device=DEV)
    gx, whole = FP.arena(n, nf, F32, col0=0, pad_cols=0, device=DEV)

    def call(**kw):
        a = dict(gy=gy.data_ptr(), in_off=off.data_ptr(), in_pt=pt.data_ptr(), in_coef=cf.data_ptr(), nf=nf, n_nodes=n, n_points=n_points,
                 gx=gx.data_ptr())
        a.update(kw)
        rc = lib.g4c_sample_points_adjoint(a["gy"], a["in_off"], a["in_pt"], a["in_coef"], a["nf"], a["n_nodes"], a["n_points"], a["gx"],
                                           _lib.stream_handle(DEV))
        return rc, lib.g4c_last_error().decode()

    big = torch.ones(n + n_points, nf, device=DEV)          # gy and gx inside one allocation: their ranges are known
    for kw, word in ((dict(nf=0), "bad sizes"), (dict(nf=-1), "bad sizes"), (dict(n_nodes=-1), "bad sizes"), (dict(n_points=-1), "bad sizes"),
                     (dict(gx=None), "null"), (dict(gy=None), "null"), (dict(in_off=None), "null"), (dict(in_pt=None), "null"),
                     (dict(in_coef=None), "null"), (dict(gx=gy.data_ptr()), "aliases"),
                     (dict(gy=big.data_ptr(), gx=big.data_ptr() + 4 * (n_points * nf - 1)), "aliases"),          # the last element of gy
                     (dict(gx=big.data_ptr(), gy=big.data_ptr() + 4 * (n * nf - 1)), "aliases")):                # the last element of gx
        rc, msg = call(**kw)
        assert rc == _lib.EINVAL and "g4c_sample_points_adjoint" in msg and word in msg, (kw, rc, msg)
    torch.cuda.synchronize(DEV)
    FP.assert_footprint(whole, gx, written_rows=range(0), what="refusals")          # nothing was written
    assert call(n_nodes=0, gx=None, gy=None)[0] == _lib.OK                          # no nodes: nothing to check, nothing launched
