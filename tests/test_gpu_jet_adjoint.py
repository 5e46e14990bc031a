"""g4c_mesh_jet_adjoint (csrc/mesh_jet.hip) through ops.mesh_jet_adjoint, gfd.MeshJet.adjoint and autograd against the numpy
restatement of tests/jet_ref.py.

The launch is bit for bit the restatement's numpy.float32 loop over the DEVICE's own table — compared as integers (−0 is not +0),
the output in a guard arena (tests/footprint.py), every input frozen — and within (n_add + t + 1) 2^-24 Σ|terms| of its fp64 form
(jet_ref.adjoint_bound); `.backward()` through `MeshJet.derived` is that launch.  The worst measured / allowed ratios are printed by
the last test (tests/JET_MEASURED.md)."""
import ctypes as C
import functools
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

import adjoint_op_ref as A                               # noqa: E402
import footprint as FP                                   # noqa: E402
import jet_ref as J                                      # noqa: E402
import graphs4cfd_amd as gfd                             # noqa: E402
from graphs4cfd_amd import _lib, ops                     # noqa: E402

DEV = torch.device("cuda", 0)
F32, I32 = torch.float32, torch.int32
RATIOS = {}


def note(name, r):
    RATIOS[name] = max(RATIOS.get(name, 0.0), float(r))


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


@functools.lru_cache(maxsize=None)
def mesh_of(n, dim, kind="cloud", shuffled=False):
    m = J.stencil_mesh(n, dim, kind=kind)
    return m.shuffled(11) if shuffled else m


@functools.lru_cache(maxsize=None)
def tables_of(kind, n, dim, shuffled=False):
    """(off, c fp32 — the DEVICE's own table —, src, row: the caller's senders); "empty": no entry; "pair": two nodes, three entries (a
    self-reference among them) with random rows; "lattice": one node above what the grid covers in one pass."""
    Q = J.q_of(dim)
    rng = np.random.default_rng(29 + n + dim)
    if kind == "empty":
        return np.zeros(n + 1, np.int32), np.zeros((0, Q), np.float32), np.zeros(0, np.int32), None
    if kind == "pair":
        return np.array([0, 2, 3], np.int32), rng.standard_normal((3, Q)).astype(np.float32), np.array([1, 0, 0], np.int32), None
    if kind == "lattice":
        return A.lattice_tables(n, 509, Q, rng)[:3] + (None,)
    m = mesh_of(n, dim, kind, shuffled)
    csr = SimpleNamespace(off=dev(m.off), perm=dev(m.perm), n=int(m.row.size))
    c, src, _ = ops.mesh_jet_weights(dev(m.rel), csr, dev(m.src32), 2)
    return m.off, c.cpu().numpy(), src.cpu().numpy(), m.row


def run(tables, dim, nf, names, velocity=None, field_scale=None, seed=0, check=True):
    """One checked launch: (the device's gx [n, nf] as numpy, gy, prog)."""
    off, c, src, _ = tables
    n = len(off) - 1
    prog = J.program(names, dim, nf, velocity, field_scale)
    nd = len(prog)
    what = f"n {n} dim {dim} nf {nf} {names} velocity {velocity} scale {field_scale}"
    gy = np.random.default_rng(1000 * n + 10 * nf + seed).standard_normal((n, nd)).astype(np.float32)
    out_off, out_perm = J.sender_csr(src, n)
    ins = [dev(gy), dev(off), dev(c), dev(out_off), dev(c[out_perm]), dev(J.dst_of(off)[out_perm])]          # the sender-ordered copies
    gx, whole = FP.arena(n, nf, F32, col0=0, pad_cols=0, device=DEV)
    with FP.frozen(*ins, what=what):
        got = ops.mesh_jet_adjoint(ins[0], ins[1], ins[2], ins[3], ins[4], ins[5], prog, nf, gx)
        torch.cuda.synchronize(DEV)
    assert got is gx
    FP.assert_footprint(whole, gx, what=what)          # every column of every row written, nothing outside
    if check:
        same_bits(gx, J.adjoint32(gy, off, c, src, prog, nf), what)
        gx64, mag, n_add = J.adjoint64(gy, off, c, src, prog, nf)
        note("adjoint: |gx - fp64| / ((n_add + t + 1) 2^-24 sum|terms|)", J.within(gx, gx64, J.adjoint_bound(mag, n_add, prog), what + ", fp64"))
        rest = [f for f in range(nf) if f not in J.fields_of(prog)]
        assert not gx[:, rest].cpu().numpy().view(np.int32).any(), what + ": a field the program does not differentiate is not +0"
    return gx.cpu().numpy(), gy, prog


PROGRAMS = {          # dim -> [(nf, names, velocity, field_scale)]: every name, 1 .. 8 columns, 1 .. 4 distinct fields
    2: [(1, ("lap:0",), None, None), (1, ("hess:0",), None, None), (3, ("div", "vort"), None, None),
        (3, ("grad:0", "grad:1", "grad:2", "lap:0", "lap:1"), None, None),          # the loss's eight columns
        (5, ("div", "vort", "lap:4", "hess:3"), (3, 1), [0.5, 2.0, -4.0, 1.5, 0.25]),
        (6, ("grad:5", "lap:2", "lap:0", "lap:3", "hess:0"), None, None), (4, ("lap:3", "lap:2", "lap:1", "lap:0", "div", "vort", "grad:3"), None, None)],
    3: [(1, ("lap:0",), None, None), (1, ("hess:0",), None, None), (3, ("div",), None, None), (3, ("vort", "grad:1", "lap:2"), None, None),
        (4, ("grad:3", "lap:0", "lap:1", "lap:2", "div"), None, None), (7, ("vort", "lap:6", "grad:0"), (4, 2, 0), [1.0, 1.0, 0.5, 1.0, -2.0, 1.0, 3.0])],
}
MESHES = [("empty", 1, False), ("pair", 2, False), ("cloud", 257, False), ("cloud", 1500, True)]


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("kind,n,shuffled", MESHES)
def test_the_adjoint_launch_matches_the_restatement(kind, n, shuffled, dim):
    tables = tables_of(kind, n, dim, shuffled)
    for nf, names, velocity, scale in PROGRAMS[dim]:
        run(tables, dim, nf, names, velocity, scale)


BIG = 262_144 + 300          # 1024 workgroups of 256: 300 threads take a second row


def test_large_mesh_takes_several_rows_per_thread():
    run(tables_of("lattice", BIG, 2), 2, 3, ("grad:0", "grad:1", "grad:2", "lap:0", "lap:1"))


def test_an_empty_stencil_and_a_mesh_without_nodes_are_zero_filled():
    for n in (0, 1, 300):
        gx, _, _ = run(tables_of("empty", n, 3), 3, 4, ("div", "lap:3"))
        assert gx.shape == (n, 4) and not gx.view(np.int32).any()


def test_two_runs_give_the_same_bits():
    tables = tables_of("cloud", 1500, 2, True)
    a = run(tables, 2, 3, ("grad:0", "grad:1", "grad:2", "lap:0", "lap:1"), check=False)[0]
    b = run(tables, 2, 3, ("grad:0", "grad:1", "grad:2", "lap:0", "lap:1"), check=False)[0]
    assert np.array_equal(a.view(np.int32), b.view(np.int32))


def test_negative_controls():
    """The launch's own output fails the comparison with a restatement that makes one mistake."""
    for dim in (2, 3):
        off, c, src, row = tables = tables_of("cloud", 1500, dim, True)
        gx, gy, prog = run(tables, dim, 3, ("lap:0", "div", "hess:2") if dim == 2 else ("lap:0", "div"))
        for wrong in A.WRONG:
            ref = J.adjoint32(gy, off, c, src, prog, 3, wrong=wrong, row=row)
            assert J.rejects(same_bits, gx, ref, wrong), wrong


# ====================================================================== gfd.MeshJet: adjoint and autograd
def graph_of(m):
    g = gfd.Graph(pos=torch.from_numpy(m.pos).float(), edge_index=torch.from_numpy(np.stack([m.row, m.col])))
    g.rel = torch.from_numpy(m.rel)
    return g.to(DEV)


@pytest.mark.parametrize("dim", [2, 3])
def test_mesh_jet_adjoint_and_backward(dim):
    n, nf = 300, 4
    m = mesh_of(n, dim, "cloud", True)
    graph = graph_of(m)
    op = gfd.MeshJet(graph, power=1, edge_vectors=graph.rel)          # k=None: the planted stencil as the graph's in-edges
    c64, _, src, degen = J.weights(m.off, m.perm, m.src32, m.rel, dim, 1)
    J.within(op.c, c64, J.weights_bound(c64, m.off), "c")
    J.same(op.src, src, "src")
    J.same(op.degenerate.cpu().numpy().astype(np.uint8), degen, "degenerate")
    c_dev = op.c.cpu().numpy()
    rng = np.random.default_rng(5)
    xs = rng.standard_normal((n, nf)).astype(np.float32)
    x = dev(xs)
    names0 = ("grad:0", "lap:1", "div")
    fwd = op.derived(x, names0)
    assert fwd.grad_fn is None and not fwd.requires_grad          # no autograd node without requires_grad
    assert op._adjoint_tables is None                            # and the plain forward builds nothing for the adjoint
    same_bits(fwd, J.derived32(xs, m.off, c_dev, src, J.program(names0, dim, nf)), "derived")
    with torch.no_grad():
        assert op.derived(x.clone().requires_grad_(True), names0).grad_fn is None and op._adjoint_tables is None
    cases = ((names0, None, None), (("vort", "hess:3") if dim == 2 else ("hess:3", "lap:0"), (2, 0) if dim == 2 else (2, 0, 1), [2.0, -0.5, 1.5, 0.25]))
    for names, velocity, scale in cases:
        prog = J.program(names, dim, nf, velocity, scale)
        gy = rng.standard_normal((n, len(prog))).astype(np.float32)
        want = J.adjoint32(gy, m.off, c_dev, src, prog, nf)
        wide = torch.zeros(n, len(prog) + 2, device=DEV)
        wide[:, 1:-1] = dev(gy)
        for given in (dev(gy), wide[:, 1:-1], dev(gy.T.copy()).t()):          # dense, a column slice, a transposed view
            with FP.frozen(given, op.c, op.src, op.off, what=str(names)):
                gx = op.adjoint(given, names, nf, velocity=velocity, field_scale=scale)
            assert tuple(gx.shape) == (n, nf) and gx.is_contiguous()
            same_bits(gx, want, f"adjoint {dim} {names}")
        # .backward() is that launch: the gradient of Σ gy · derived(x) is adjoint(gy), bit for bit
        xg = x.clone().requires_grad_(True)
        out = op.derived(xg, names, velocity=velocity, field_scale=scale)
        assert out.grad_fn is not None
        same_bits(out, J.derived32(xs, m.off, c_dev, src, prog), "recorded forward")
        (out * dev(gy)).sum().backward()
        same_bits(xg.grad, want, f"backward {dim} {names}")
        # `.sum().backward()` hands over a stride-0 expanded tensor
        xg = x.clone().requires_grad_(True)
        op.derived(xg, names, velocity=velocity, field_scale=scale).sum().backward()
        same_bits(xg.grad, J.adjoint32(np.ones_like(gy), m.off, c_dev, src, prog, nf), "backward of the sum")
    got_off, got_c, got_dst = op._adjoint_tables
    assert op._sender_side()[1] is got_c                         # built once, kept
    out_off, out_perm = J.sender_csr(src, n)
    J.same(got_off, out_off, "out_off")
    J.same(got_dst, J.dst_of(m.off)[out_perm], "out_dst")
    J.same(got_c, c_dev[out_perm], "out_c")
    # ⟨D x, y⟩ = ⟨x, Dᵀ y⟩ on the device's own outputs, within the two fp32 bounds
    prog = J.program(names0, dim, nf)
    y = rng.standard_normal((n, len(prog))).astype(np.float32)
    gx = op.adjoint(dev(y), names0, nf).cpu().numpy().astype(np.float64)
    mag = J.derived64(xs, m.off, c_dev, src, prog)[1]
    gmag, n_add = J.adjoint64(y, m.off, c_dev, src, prog, nf)[1:]
    lhs, rhs = float((fwd.cpu().numpy().astype(np.float64) * y).sum()), float((xs.astype(np.float64) * gx).sum())
    allowed = float((J.bound32(mag, m.max_deg) * np.abs(y)).sum() + (J.adjoint_bound(gmag, n_add, prog) * np.abs(xs)).sum()) * (1 + 1e-6)
    assert abs(lhs - rhs) <= allowed, (lhs, rhs, allowed)
    note("adjoint identity: |<Dx, y> - <x, DTy>| / the two fp32 bounds", abs(lhs - rhs) / allowed)


def test_backward_agrees_with_differences_of_the_forward():
    """gradcheck's comparison, in the arithmetic this operator has: the map is linear, so (D(x + h e) − D(x)) · gy / h is the e-th entry of
    Dᵀ gy exactly; in fp32 the two forwards each carry their bound, so |difference − backward| <= (2 bound32 · |gy| summed) / h +
    the adjoint's own bound.  Checked for a handful of entries with h = 1."""
    dim, n, nf = 2, 300, 3
    m = mesh_of(n, dim, "cloud", True)
    graph = graph_of(m)
    op = gfd.MeshJet(graph, power=2, edge_vectors=graph.rel)
    c_dev, src = op.c.cpu().numpy(), op.src.cpu().numpy()
    names = ("grad:0", "grad:1", "grad:2", "lap:0", "lap:1")
    prog = J.program(names, dim, nf)
    rng = np.random.default_rng(9)
    xs = rng.standard_normal((n, nf)).astype(np.float32)
    gy = rng.standard_normal((n, len(prog))).astype(np.float32)
    xg = dev(xs).requires_grad_(True)
    (op.derived(xg, names) * dev(gy)).sum().backward()
    grad = xg.grad.cpu().numpy().astype(np.float64)
    base = op.derived(dev(xs), names).cpu().numpy().astype(np.float64)
    gmag, n_add = J.adjoint64(gy, m.off, c_dev, src, prog, nf)[1:]
    own = J.adjoint_bound(gmag, n_add, prog)
    keep = [i for i in range(n) if i not in m.planted]
    for node, f in [(keep[3], 0), (keep[57], 1), (keep[120], 2), (keep[-1], 0)]:
        moved = xs.copy()
        moved[node, f] += np.float32(1.0)
        d = op.derived(dev(moved), names).cpu().numpy().astype(np.float64)
        fd = float(((d - base) * gy).sum())
        mags = J.derived64(moved, m.off, c_dev, src, prog)[1] + J.derived64(xs, m.off, c_dev, src, prog)[1]
        touched = np.abs(d - base).sum(1) > 0          # (only the rows whose stencil holds the moved value differ at all)
        allowed = float((J.bound32(mags, m.max_deg) * np.abs(gy))[touched].sum() + own[node, f]) * (1 + 1e-6)
        assert abs(fd - grad[node, f]) <= allowed, (node, f, fd, grad[node, f], allowed)
        note("backward vs a difference of two forwards / the fp32 bounds", abs(fd - grad[node, f]) / allowed)


def test_refusals_return_their_code_without_launching():
    lib = _lib.load()
    n, S, nf = 64, 320, 3
    gy, c, idx = torch.ones(n, 1, device=DEV), torch.ones(S, 5, device=DEV), torch.zeros(S, dtype=I32, device=DEV)
    off = torch.arange(0, S + 1, 5, dtype=I32, device=DEV)
    gx, whole = FP.arena(n, nf, F32, col0=0, pad_cols=0, device=DEV)

    def call(prog_kw=None, **kw):
        a = dict(gy=gy.data_ptr(), dim=2, nf=nf, c=c.data_ptr(), off=off.data_ptr(), out_c=c.data_ptr(), out_dst=idx.data_ptr(),
                 out_off=off.data_ptr(), n_nodes=n, n_entries=S, gx=gx.data_ptr())
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
        rc = lib.g4c_mesh_jet_adjoint(a["gy"], C.byref(p) if a.get("prog", 1) else None, a["dim"], a["nf"], a["c"], a["off"], a["out_c"],
                                      a["out_dst"], a["out_off"], a["n_nodes"], a["n_entries"], a["gx"], _lib.stream_handle(DEV))
        return rc, lib.g4c_last_error().decode()

    for prog_kw, kw, code, word in ((dict(nd=9), {}, _lib.EUNSUPPORTED, "nd=9"), (dict(n_terms=4), {}, _lib.EUNSUPPORTED, "4 terms"),
                                    ({}, dict(dim=4), _lib.EUNSUPPORTED, "dim=4"), ({}, dict(dim=1), _lib.EUNSUPPORTED, "dim=1"),
                                    (dict(field=3), {}, _lib.EINVAL, "field 3"), (dict(field=-1), {}, _lib.EINVAL, "field -1"),
                                    (dict(axis=5), {}, _lib.EINVAL, "derivative 5"), (dict(n_terms=0), {}, _lib.EINVAL, "0 terms"),
                                    (dict(nd=0), {}, _lib.EINVAL, "bad sizes"), ({}, dict(nf=0), _lib.EINVAL, "bad sizes"),
                                    ({}, dict(n_nodes=-1), _lib.EINVAL, "bad sizes"), ({}, dict(n_entries=-1), _lib.EINVAL, "bad sizes"),
                                    ({}, dict(prog=0), _lib.EINVAL, "null"), ({}, dict(gy=None), _lib.EINVAL, "null"),
                                    ({}, dict(gx=None), _lib.EINVAL, "null"), ({}, dict(c=None), _lib.EINVAL, "null"),
                                    ({}, dict(off=None), _lib.EINVAL, "null"), ({}, dict(out_dst=None), _lib.EINVAL, "null"),
                                    ({}, dict(out_c=None), _lib.EINVAL, "null"),
                                    ({}, dict(out_off=None), _lib.EINVAL, "null"), ({}, dict(gx=gy.data_ptr()), _lib.EINVAL, "aliases"),
                                    ({}, dict(gx=gy.data_ptr() + 4 * (n - 1)), _lib.EINVAL, "aliases")):
        rc, msg = call(prog_kw, **kw)
        assert rc == code and "g4c_mesh_jet_adjoint" in msg and word in msg, (prog_kw, kw, rc, msg)
    torch.cuda.synchronize(DEV)
    FP.assert_footprint(whole, gx, written_rows=range(0), what="refusals")          # nothing was written
    with pytest.raises(ValueError, match="distinct fields"):                         # five fields in one program
        ops.mesh_jet_adjoint(torch.ones(n, 5, device=DEV), off, c, off, c, idx, [[(f, 0, 1.0)] for f in range(5)], 5)
    with pytest.raises(ValueError, match="shares its storage"):
        both = torch.ones(n, 3, device=DEV)
        ops.mesh_jet_adjoint(both, off, c, off, c, idx, [[(0, 0, 1.0)], [(1, 2, 1.0)], [(2, 4, 1.0)]], 3, gx=both)


def test_zz_print_the_measured_ratios():
    """Not a check of its own: the measured / allowed ratio of every bound above, for tests/JET_MEASURED.md (pytest -s)."""
    for k, v in sorted(RATIOS.items()):
        print(f"MEASURED {k}: {v:.3f}")
        assert v <= 1.0
