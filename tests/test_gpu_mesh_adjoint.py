"""g4c_mesh_derived_adjoint (csrc/mesh_gradient.hip) through ops.mesh_derived_adjoint and gfd.MeshGradient.adjoint against the numpy
restatement of tests/adjoint_op_ref.py.

The launch is bit for bit the restatement's numpy.float32 loop — compared as integers (−0 is not +0), with the output in a guard
arena (tests/footprint.py: every element of the window written, nothing around it) and every input frozen — and within
(n_add + 3) 2^-24 Σ|terms| of its fp64 form; the worst measured / allowed ratio is printed by the last test
(tests/FLOW_LOSS_MEASURED.md).  Each deliberate mistake of the restatement is rejected by the same checker."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

import adjoint_op_ref as A                               # noqa: E402
import footprint as FP                                   # noqa: E402
import gradient_ref as R                                 # noqa: E402
import graphs4cfd_amd as gfd                             # noqa: E402
from graphs4cfd_amd import _lib, ops                     # noqa: E402

DEV = torch.device("cuda", 0)
F32, I32 = torch.float32, torch.int32
RATIOS = {}


def note(name, r):
    RATIOS[name] = max(RATIOS.get(name, 0.0), float(r))


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
def mesh_of(kind, n, dim, shuffled):
    m = {"uniform": R.uniform_mesh, "ragged": R.ragged_mesh, "hub": A.hub_mesh}[kind](n, dim)
    return m.shuffled(11) if shuffled else m


@functools.lru_cache(maxsize=None)
def tables_of(kind, n, dim, shuffled, power=2):
    """(off, g fp32, src, row: the caller's senders) — the restatement's weights of a mesh; "single": one node, no edge; "pair": two nodes,
    three edges (a self-loop among them) with random weights; "lattice": one node above what the grid covers in one pass."""
    rng = np.random.default_rng(17 + n + dim)
    if kind == "single":
        return np.zeros(2, np.int32), np.zeros((0, dim), np.float32), np.zeros(0, np.int32), None
    if kind == "pair":
        return np.array([0, 2, 3], np.int32), rng.standard_normal((3, dim)).astype(np.float32), np.array([1, 0, 0], np.int32), None
    if kind == "lattice":
        return A.lattice_tables(n, 509, dim, rng)[:3] + (None,)
    m = mesh_of(kind, n, dim, shuffled)
    g32, src = R.weights(m.off, m.perm, m.src32, m.rel, dim, power)[1:3]
    return m.off, g32, src, m.row


def run(tables, dim, nf, names, velocity=None, field_scale=None, seed=0, check=True):
    """One checked launch: (the device's gx [n, nf] as numpy, gy, prog)."""
    off, g, src, _ = tables
    n = len(off) - 1
    prog = R.program(names, dim, nf, velocity, field_scale)
    nd = len(prog)
    what = f"n {n} dim {dim} nf {nf} {names} velocity {velocity} scale {field_scale}"
    gy = np.random.default_rng(1000 * n + 10 * nf + seed).standard_normal((n, nd)).astype(np.float32)
    out_off, out_perm = A.sender_csr(src, n)
    ins = [dev(gy), dev(off), dev(g), dev(out_off), dev(g[out_perm]), dev(A.dst_of(off)[out_perm])]          # the sender-ordered copies
    gx, whole = FP.arena(n, nf, F32, col0=0, pad_cols=0, device=DEV)
    with FP.frozen(*ins, what=what):
        got = ops.mesh_derived_adjoint(ins[0], ins[1], ins[2], ins[3], ins[4], ins[5], prog, nf, gx)
        torch.cuda.synchronize(DEV)
    assert got is gx
    FP.assert_footprint(whole, gx, what=what)          # every column of every row written, nothing outside
    if check:
        same_bits(gx, A.adjoint32(gy, off, g, src, prog, nf), what)
        gx64, mag, n_add = A.adjoint64(gy, off, g, src, prog, nf)
        note("adjoint: |gx - fp64| / ((n_add + 3) 2^-24 sum|terms|)", R.within(gx, gx64, A.bound(mag, n_add, prog), what + ", fp64"))
        used = A.fields_of(prog)
        rest = [f for f in range(nf) if f not in used]
        assert not gx[:, rest].cpu().numpy().view(np.int32).any(), what + ": a field the program does not differentiate is not +0"
    return gx.cpu().numpy(), gy, prog


PROGRAMS = {          # dim -> [(nf, names, velocity, field_scale)]
    2: [(3, ("div",), None, None), (3, ("vort",), None, None), (3, ("div", "vort", "grad:2"), None, None),
        (3, ("div", "vort"), (2, 0), None), (3, ("div", "vort", "grad:0"), None, [0.5, 2.0, -4.0]), (1, ("grad:0",), None, None),
        (9, ("grad:8", "grad:1", "grad:4", "grad:6"), None, None),                      # eight columns of grad:, none of a leading field
        (9, ("div", "vort", "grad:4", "grad:6", "grad:8"), (7, 2), None)],              # five distinct fields: the widest instantiation
    3: [(3, ("div",), None, None), (3, ("vort",), None, None), (3, ("div", "vort"), None, None), (1, ("grad:0",), None, None),
        (9, ("grad:8", "grad:3"), None, None), (9, ("vort", "grad:5"), (6, 2, 7), [1.0, 1.0, 0.5, 1.0, 1.0, -2.0, 3.0, 0.25, 1.0])],
}
MESHES = [("single", 1, False), ("pair", 2, False), ("uniform", 257, False), ("ragged", 300, True), ("hub", 600, False), ("hub", 600, True)]


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("kind,n,shuffled", MESHES)
def test_the_adjoint_launch_matches_the_restatement(kind, n, shuffled, dim):
    tables = tables_of(kind, n, dim, shuffled)
    if kind == "hub":
        out_off = A.sender_csr(tables[2], n)[0]
        assert np.diff(out_off).max() >= n - 1 and (np.diff(out_off) == 0).any()          # one node sends to all, one to nobody
    for nf, names, velocity, scale in PROGRAMS[dim]:
        run(tables, dim, nf, names, velocity, scale)


BIG = 262_144 + 300          # 1024 workgroups of 256: 300 threads take a second row


def test_large_mesh_takes_several_rows_per_thread():
    run(tables_of("lattice", BIG, 2, False), 2, 3, ("div", "vort"))


def test_a_mesh_without_edges_and_a_mesh_without_nodes_are_zero_filled():
    for n in (0, 1, 300):
        off = np.zeros(n + 1, np.int32)
        gx, _, _ = run((off, np.zeros((0, 3), np.float32), np.zeros(0, np.int32), None), 3, 4, ("div", "vort"))
        assert gx.shape == (n, 4) and not gx.view(np.int32).any()


def test_two_runs_give_the_same_bits():
    tables = tables_of("hub", 600, 2, True)
    a = run(tables, 2, 3, ("div", "vort", "grad:2"), check=False)[0]
    b = run(tables, 2, 3, ("div", "vort", "grad:2"), check=False)[0]
    assert np.array_equal(a.view(np.int32), b.view(np.int32))


def test_negative_controls():
    """The launch's own output fails the comparison with a restatement that makes one mistake."""
    for dim in (2, 3):
        off, g, src, row = tables = tables_of("ragged", 300, dim, True)
        gx, gy, prog = run(tables, dim, 3, ("div", "vort"))
        same_bits(gx, A.adjoint32(gy, off, g, src, prog, 3), "right")
        for wrong in A.WRONG:
            ref = A.adjoint32(gy, off, g, src, prog, 3, wrong=wrong, row=row)
            assert R.rejects(same_bits, gx, ref, wrong), wrong
            r64, mag, n_add = A.adjoint64(gy, off, g, src, prog, 3, wrong=wrong, row=row)
            assert R.rejects(R.within, gx, r64, (n_add + 3) * A.U * mag, wrong), wrong


# ====================================================================== gfd.MeshGradient.adjoint
def graph_of(m):
    g = gfd.Graph(pos=torch.from_numpy(m.pos).float(), edge_index=torch.from_numpy(np.stack([m.row, m.col])))
    g.rel = torch.from_numpy(m.rel)
    return g.to(DEV)


@pytest.mark.parametrize("kind,n,dim", [("ragged", 300, 2), ("ragged", 300, 3), ("hub", 600, 2)])
def test_mesh_gradient_adjoint(kind, n, dim):
    m = mesh_of(kind, n, dim, True)
    graph = graph_of(m)
    op = gfd.MeshGradient(graph, power=1, edge_vectors=graph.rel)
    g64, g32, src, degen = R.weights(m.off, m.perm, m.src32, m.rel, dim, 1)
    R.within(op.g, g64, R.weights_bound(g64, m.off), "g")
    R.same(op.src, src, "src")
    g_dev = op.g.cpu().numpy()                                   # the operator's own weights (pinned above): the loop runs from them
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.standard_normal((n, 3)).astype(np.float32)).to(DEV)
    fwd = op.derived(x, ("div", "vort"))
    assert op._adjoint_tables is None                            # the plain forward builds nothing for the adjoint
    for names, velocity, scale in ((("div", "vort"), None, None), (("vort", "grad:2"), (2, 0) if dim == 2 else (2, 0, 1), [2.0, -0.5, 1.5])):
        prog = R.program(names, dim, 3, velocity, scale)
        gy = rng.standard_normal((n, len(prog))).astype(np.float32)
        wide = torch.zeros(n, len(prog) + 2, device=DEV)
        wide[:, 1:-1] = dev(gy)
        for given in (dev(gy), wide[:, 1:-1], dev(gy.T.copy()).t()):          # dense, a column slice, a transposed view
            with FP.frozen(given, op.g, op.src, op.off, what=str(names)):
                gx = op.adjoint(given, names, 3, velocity=velocity, field_scale=scale)
            assert tuple(gx.shape) == (n, 3) and gx.is_contiguous()
            same_bits(gx, A.adjoint32(gy, m.off, g_dev, src, prog, 3), f"{kind} {dim} {names}")
    got_off, got_g, got_dst = op._adjoint_tables
    assert op._sender_side()[1] is got_g                         # built once, kept
    out_off, out_perm = A.sender_csr(src, n)
    R.same(got_off, out_off, "out_off")
    R.same(got_dst, A.dst_of(m.off)[out_perm], "out_dst")
    R.same(got_g, g_dev[out_perm], "out_g")
    # ⟨D x, y⟩ = ⟨x, Dᵀ y⟩ on the device's own outputs, within the two fp32 bounds
    y = rng.standard_normal((n, fwd.size(1))).astype(np.float32)
    gx = op.adjoint(dev(y), ("div", "vort"), 3).cpu().numpy().astype(np.float64)
    prog = R.program(("div", "vort"), dim, 3)
    xs = x.cpu().numpy()
    mag = R.derived64(xs, m.off, g_dev, src, prog)[1]
    gmag, n_add = A.adjoint64(y, m.off, g_dev, src, prog, 3)[1:]
    lhs, rhs = float((fwd.cpu().numpy().astype(np.float64) * y).sum()), float((xs.astype(np.float64) * gx).sum())
    allowed = float((R.bound32(mag, m.max_deg) * np.abs(y)).sum() + (A.bound(gmag, n_add, prog) * np.abs(xs)).sum()) * (1 + 1e-6)
    assert abs(lhs - rhs) <= allowed, (lhs, rhs, allowed)
    note("adjoint identity: |<Dx, y> - <x, DTy>| / the two fp32 bounds", abs(lhs - rhs) / allowed)


def test_refusals_return_their_code_without_launching():
    lib = _lib.load()
    n, n_e, nf = 64, 128, 3
    gy, g, idx = torch.ones(n, 1, device=DEV), torch.ones(n_e, 2, device=DEV), torch.zeros(n_e, dtype=I32, device=DEV)
    off = torch.arange(0, n_e + 1, 2, dtype=I32, device=DEV)
    gx, whole = FP.arena(n, nf, F32, col0=0, pad_cols=0, device=DEV)

    def call(prog_kw=None, **kw):
        a = dict(gy=gy.data_ptr(), dim=2, nf=nf, g=g.data_ptr(), off=off.data_ptr(), out_g=g.data_ptr(), out_dst=idx.data_ptr(),
                 out_off=off.data_ptr(), n_nodes=n, n_edges=n_e, gx=gx.data_ptr())
        a.update(kw)
        p = _lib.g4c_derived_program_t(nd=1)
        p.n_terms[0], p.coef[0][0] = 1, 1.0
        for k, v in (prog_kw or {}).items():
            if k == "nd":
                p.nd = v
            elif k == "n_terms":
                p.n_terms[0] = v
            else:
                getattr(p, k)[0][0] = v
        rc = lib.g4c_mesh_derived_adjoint(a["gy"], C.byref(p) if a.get("prog", 1) else None, a["dim"], a["nf"], a["g"], a["off"], a["out_g"],
                                          a["out_dst"], a["out_off"], a["n_nodes"], a["n_edges"], a["gx"], _lib.stream_handle(DEV))
        return rc, lib.g4c_last_error().decode()

    for prog_kw, kw, code, word in ((dict(nd=9), {}, _lib.EUNSUPPORTED, "nd=9"), (dict(n_terms=4), {}, _lib.EUNSUPPORTED, "4 terms"),
                                    ({}, dict(dim=4), _lib.EUNSUPPORTED, "dim=4"), ({}, dict(dim=1), _lib.EUNSUPPORTED, "dim=1"),
                                    (dict(field=3), {}, _lib.EINVAL, "field 3"), (dict(field=-1), {}, _lib.EINVAL, "field -1"),
                                    (dict(axis=2), {}, _lib.EINVAL, "axis 2"), (dict(n_terms=0), {}, _lib.EINVAL, "0 terms"),
                                    (dict(nd=0), {}, _lib.EINVAL, "bad sizes"), ({}, dict(nf=0), _lib.EINVAL, "bad sizes"),
                                    ({}, dict(n_nodes=-1), _lib.EINVAL, "bad sizes"), ({}, dict(n_edges=-1), _lib.EINVAL, "bad sizes"),
                                    ({}, dict(prog=0), _lib.EINVAL, "null"), ({}, dict(gy=None), _lib.EINVAL, "null"),
                                    ({}, dict(gx=None), _lib.EINVAL, "null"), ({}, dict(g=None), _lib.EINVAL, "null"),
                                    ({}, dict(off=None), _lib.EINVAL, "null"), ({}, dict(out_dst=None), _lib.EINVAL, "null"),
                                    ({}, dict(out_g=None), _lib.EINVAL, "null"),
                                    ({}, dict(out_off=None), _lib.EINVAL, "null"), ({}, dict(gx=gy.data_ptr()), _lib.EINVAL, "aliases"),
                                    ({}, dict(gx=gy.data_ptr() + 4 * (n - 1)), _lib.EINVAL, "aliases")):
        rc, msg = call(prog_kw, **kw)
        assert rc == code and "g4c_mesh_derived_adjoint" in msg and word in msg, (prog_kw, kw, rc, msg)
    torch.cuda.synchronize(DEV)
    FP.assert_footprint(whole, gx, written_rows=range(0), what="refusals")          # nothing was written
    with pytest.raises(NotImplementedError, match="distinct fields"):                # nine fields in one program
        ops.mesh_derived_adjoint(torch.ones(n, 8, device=DEV), off, g, off, g, idx,
                                 [[(f, 0, 1.0)] for f in range(7)] + [[(7, 0, 1.0), (8, 1, 1.0)]], 9)


def test_zz_print_the_measured_ratios():
    """Not a check of its own: the measured / allowed ratio of every bound above, for tests/FLOW_LOSS_MEASURED.md (pytest -s)."""
    for k, v in sorted(RATIOS.items()):
        print(f"MEASURED {k}: {v:.3f}")
        assert v <= 1.0
