"""g4c_mesh_jet_weights and g4c_mesh_jet (csrc/mesh_jet.hip) through ops.mesh_jet_weights / ops.mesh_jet and gfd.MeshJet against
the numpy restatement of tests/jet_ref.py.

The weights sit within 2^-23 of the largest |c| of the node's rows of their fp64 restatement, `degenerate` and `src` are exact.
The per-call launch is bit for bit the restatement's numpy.float32 loop over the DEVICE's own table — compared as integers, the
output in a guard arena (tests/footprint.py), every input frozen — and within (deg + 3) 2^-24 Σ|c||Δx| of its fp64 form.  The
worst measured / allowed ratios are printed by the last test (tests/JET_MEASURED.md)."""
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


def device_weights(m, power):
    """The three outputs of one checked ops.mesh_jet_weights launch, as numpy."""
    Q, S = J.q_of(m.dim), int(m.row.size)
    csr = SimpleNamespace(off=dev(m.off), perm=dev(m.perm), n=S)
    c, c_whole = FP.arena(S, Q, F32, col0=0, pad_cols=0, device=DEV)
    src, s_whole = FP.flat_arena(S, I32, device=DEV)
    deg = torch.full((m.n,), 7, dtype=torch.uint8, device=DEV)          # (neither 0 nor 1: every flag is written)
    ins = [dev(m.rel), csr.off, dev(m.src32)] + ([csr.perm] if csr.perm is not None else [])
    with FP.frozen(*ins, what="weights"):
        got = ops.mesh_jet_weights(ins[0], csr, ins[2], power, out=(c, src, deg))
        torch.cuda.synchronize(DEV)
    assert got[0] is c
    if S:
        FP.assert_footprint(c_whole, c, what="c")
        FP.assert_footprint(s_whole, src, what="src")
        assert int((deg == 7).sum()) == 0
    return c.cpu().numpy().copy(), src.cpu().numpy().copy(), deg.cpu().numpy().copy()


# ====================================================================== weights
SIZES = (1, 63, 64, 65, 257, 1500)


@pytest.mark.parametrize("power", [0, 1, 2])
@pytest.mark.parametrize("dim", [2, 3])
def test_the_weights_match_the_restatement(dim, power):
    for n in SIZES:
        for shuffled in (False, True):
            m = mesh_of(n, dim, "lattice" if n == 257 else "cloud", shuffled)
            assert (m.perm is not None) == (shuffled and m.row.size > 1)
            what = f"n {n} dim {dim} power {power} perm {shuffled}"
            if not m.row.size:          # (a single node: no entry, no launch — the caller's flags stay as the caller filled them)
                c, src, deg = ops.mesh_jet_weights(dev(m.rel), SimpleNamespace(off=dev(m.off), perm=None, n=0), dev(m.src32), power)
                assert tuple(c.shape) == (0, J.q_of(dim)) and bool(deg.all())
                continue
            c, src, deg = device_weights(m, power)
            c64, _, src_ref, degen = J.weights(m.off, m.perm, m.src32, m.rel, dim, power)
            J.same(deg, degen, what + ": degenerate")
            J.same(src, src_ref, what + ": src")
            note(f"weights dim {dim}: |c - fp64| / (2^-23 max|c| of the node)", J.within(c, c64, J.weights_bound(c64, m.off), what))
            node = np.repeat(np.arange(m.n), np.diff(m.off))
            assert not c[degen[node] == 1].view(np.int32).any(), what + ": a degenerate node's rows are not +0"
            if n == 1500 and not shuffled:
                for wrong in J.WRONG_WEIGHTS[:2]:
                    bad = J.weights(m.off, m.perm, m.src32, m.rel, dim, power, wrong=wrong)[0]
                    assert J.rejects(J.within, c, bad, J.weights_bound(bad, m.off)), wrong
            if n == 1500 and shuffled:
                assert J.rejects(J.same, src, J.weights(m.off, m.perm, m.src32, m.rel, dim, power, wrong="src-unpermuted")[2])


# ====================================================================== per call
@functools.lru_cache(maxsize=None)
def tables_of(kind, n, dim, shuffled=False, power=2):
    """(off, c fp32 — the DEVICE's own table —, src, max_deg); "empty": no entry at all; "lattice": random rows over i ± 1, i ± w, one
    node above what the grid covers in one pass."""
    Q = J.q_of(dim)
    if kind == "empty":
        return np.zeros(n + 1, np.int32), np.zeros((0, Q), np.float32), np.zeros(0, np.int32), 0
    if kind == "lattice":
        return A.lattice_tables(n, 509, Q, np.random.default_rng(23 + n + dim))
    m = mesh_of(n, dim, kind, shuffled)
    c, src, _ = device_weights(m, power)
    return m.off, c, src, m.max_deg


def run(tables, dim, nf, names, velocity=None, field_scale=None, pad=0, seed=0, check=True):
    """One checked launch: (the device's out [n, nd] as numpy, x, prog)."""
    off, c, src, max_deg = tables
    n = len(off) - 1
    prog = J.program(names, dim, nf, velocity, field_scale)
    nd = len(prog)
    what = f"n {n} dim {dim} nf {nf} pad {pad} {names} velocity {velocity} scale {field_scale}"
    x = np.random.default_rng(1000 * n + 10 * nf + seed).standard_normal((n, nf)).astype(np.float32)
    wide = torch.full((n, nf + pad), float("nan"), device=DEV)          # (the padding is never read: a NaN there would show)
    wide[:, :nf] = dev(x)
    ins = [wide, dev(off), dev(c), dev(src)]
    out, whole = FP.arena(n, nd, F32, col0=0, pad_cols=0, device=DEV)
    with FP.frozen(*ins, what=what):
        got = ops.mesh_jet(wide, ins[1], ins[2], ins[3], prog, out, nf=nf)
        torch.cuda.synchronize(DEV)
    assert got is out
    FP.assert_footprint(whole, out, what=what)
    if check:
        same_bits(out, J.derived32(x, off, c, src, prog), what)
        o64, mag = J.derived64(x, off, c, src, prog)
        note("derived: |out - fp64| / ((deg + 3) 2^-24 sum|c||dx|)", J.within(out, o64, J.bound32(mag, max_deg), what + ", fp64"))
    return out.cpu().numpy(), x, prog


PROGRAMS = {          # dim -> [(nf, names, velocity, field_scale)]: every name, 1 .. 8 columns, 1 .. 4 distinct fields
    2: [(1, ("lap:0",), None, None), (1, ("grad:0",), None, None), (1, ("hess:0",), None, None), (3, ("div", "vort"), None, None),
        (3, ("grad:0", "grad:1", "grad:2", "lap:0", "lap:1"), None, None),          # the loss's eight columns
        (5, ("div", "vort", "lap:4", "hess:3"), (3, 1), [0.5, 2.0, -4.0, 1.5, 0.25]), (6, ("grad:5", "lap:2", "lap:0", "lap:3", "hess:0"), None, None),
        (2, ("grad:1", "lap:1", "hess:1", "lap:0"), None, None), (4, ("lap:3", "lap:2", "lap:1", "lap:0", "div", "vort", "grad:3"), None, None)],
    3: [(1, ("lap:0",), None, None), (1, ("hess:0",), None, None), (3, ("div",), None, None), (3, ("vort", "grad:1", "lap:2"), None, None),
        (4, ("grad:3", "lap:0", "lap:1", "lap:2", "div"), None, None), (6, ("hess:5", "lap:2"), None, [1.0, 1.0, 0.5, 1.0, 1.0, -2.0]),
        (7, ("vort", "lap:6", "grad:0"), (4, 2, 0), None)],
}


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("kind,n,shuffled", [("cloud", 63, False), ("lattice", 257, True), ("cloud", 1500, True)])
def test_the_launch_matches_the_restatement(kind, n, shuffled, dim):
    tables = tables_of(kind, n, dim, shuffled)
    for j, (nf, names, velocity, scale) in enumerate(PROGRAMS[dim]):
        run(tables, dim, nf, names, velocity, scale, pad=(0, 3, 1)[j % 3])


BIG = 262_144 + 300          # 1024 workgroups of 256: 300 threads take a second row


def test_large_mesh_takes_several_rows_per_thread():
    run(tables_of("lattice", BIG, 2), 2, 3, ("grad:0", "grad:1", "grad:2", "lap:0", "lap:1"))


def test_an_empty_stencil_writes_zeros_and_no_node_launches_nothing():
    for n in (0, 1, 300):
        out, _, _ = run(tables_of("empty", n, 3), 3, 4, ("div", "lap:3"))
        assert out.shape == (n, 2) and not out.view(np.int32).any()


def test_two_runs_give_the_same_bits():
    tables = tables_of("cloud", 1500, 2, True)
    a = run(tables, 2, 3, ("grad:0", "grad:1", "grad:2", "lap:0", "lap:1"), check=False)[0]
    b = run(tables, 2, 3, ("grad:0", "grad:1", "grad:2", "lap:0", "lap:1"), check=False)[0]
    assert np.array_equal(a.view(np.int32), b.view(np.int32))


def test_negative_controls():
    """The launch's own output fails the comparison with a table that makes one mistake."""
    for dim in (2, 3):
        m = mesh_of(1500, dim, "cloud", True)
        off, c, src, max_deg = tables = tables_of("cloud", 1500, dim, True)
        out, x, prog = run(tables, dim, 3, ("lap:0", "grad:1"))
        for wrong in ("sign", "diagonal-factor"):
            bad = J.weights(m.off, m.perm, m.src32, m.rel, dim, 2, wrong=wrong)[1]
            o64, mag = J.derived64(x, off, bad, src, prog)
            assert J.rejects(J.within, out, o64, J.bound32(mag, max_deg)), wrong
        assert J.rejects(same_bits, out, J.derived32(x, off, c, m.src32[:src.size], prog))          # the senders unpermuted


def test_refusals_return_their_code_without_launching():
    lib = _lib.load()
    n, S, nf = 64, 320, 3
    x, c, idx = torch.ones(n, nf, device=DEV), torch.ones(S, 5, device=DEV), torch.zeros(S, dtype=I32, device=DEV)
    off = torch.arange(0, S + 1, 5, dtype=I32, device=DEV)
    out, whole = FP.arena(n, 8, F32, col0=0, pad_cols=0, device=DEV)
    stream = _lib.stream_handle(DEV)

    def call(prog_kw=None, **kw):
        a = dict(x=x.data_ptr(), x_ld=nf, nf=nf, dim=2, c=c.data_ptr(), src=idx.data_ptr(), off=off.data_ptr(), n_nodes=n, n_entries=S,
                 out=out.data_ptr(), prog=1)
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
        rc = lib.g4c_mesh_jet(a["x"], a["x_ld"], a["nf"], a["dim"], a["c"], a["src"], a["off"], C.byref(p) if a["prog"] else None,
                              a["n_nodes"], a["n_entries"], a["out"], stream)
        return rc, lib.g4c_last_error().decode()

    for prog_kw, kw, code, word in ((dict(nd=9), {}, _lib.EUNSUPPORTED, "nd=9"), (dict(n_terms=4), {}, _lib.EUNSUPPORTED, "4 terms"),
                                    ({}, dict(dim=4), _lib.EUNSUPPORTED, "dim=4"), ({}, dict(dim=1), _lib.EUNSUPPORTED, "dim=1"),
                                    (dict(field=3), {}, _lib.EINVAL, "field 3"), (dict(field=-1), {}, _lib.EINVAL, "field -1"),
                                    (dict(axis=5), {}, _lib.EINVAL, "derivative 5"), (dict(axis=-1), {}, _lib.EINVAL, "derivative -1"),
                                    (dict(n_terms=0), {}, _lib.EINVAL, "0 terms"), (dict(nd=0), {}, _lib.EINVAL, "bad sizes"),
                                    ({}, dict(nf=0), _lib.EINVAL, "bad sizes"), ({}, dict(x_ld=2), _lib.EINVAL, "x_ld=2"),
                                    ({}, dict(n_nodes=-1), _lib.EINVAL, "bad sizes"), ({}, dict(n_entries=-1), _lib.EINVAL, "bad sizes"),
                                    ({}, dict(prog=0), _lib.EINVAL, "null"), ({}, dict(x=None), _lib.EINVAL, "null"),
                                    ({}, dict(out=None), _lib.EINVAL, "null"), ({}, dict(c=None), _lib.EINVAL, "null"),
                                    ({}, dict(src=None), _lib.EINVAL, "null"), ({}, dict(off=None), _lib.EINVAL, "null")):
        rc, msg = call(prog_kw, **kw)
        assert rc == code and "g4c_mesh_jet" in msg and word in msg, (prog_kw, kw, rc, msg)
    torch.cuda.synchronize(DEV)
    FP.assert_footprint(whole, out, written_rows=range(0), what="refusals")          # nothing was written
    # derivative 8 is refused in 2-D only: it is zz in 3-D
    c9 = torch.ones(S, 9, device=DEV)
    assert call(dict(axis=8), dim=3, c=c9.data_ptr())[0] == _lib.OK
    torch.cuda.synchronize(DEV)
    out2, whole2 = FP.arena(n, 8, F32, col0=0, pad_cols=0, device=DEV)
    five = _lib.g4c_derived_program_t(nd=5)
    for col in range(5):
        five.n_terms[col], five.field[col][0], five.coef[col][0] = 1, col, 1.0
    wide = torch.ones(n, 5, device=DEV)
    rc = lib.g4c_mesh_jet(wide.data_ptr(), 5, 5, 2, c.data_ptr(), idx.data_ptr(), off.data_ptr(), C.byref(five), n, S, out2.data_ptr(), stream)
    assert rc == _lib.EUNSUPPORTED and "distinct fields" in lib.g4c_last_error().decode()
    with pytest.raises(ValueError, match="distinct fields"):
        ops.mesh_jet(wide, off, c, idx, [[(f, 0, 1.0)] for f in range(5)])
    # the weights' refusals
    deg = torch.full((n,), 7, dtype=torch.uint8, device=DEV)
    rel = torch.ones(S, 2, device=DEV)
    c_out, c_whole = FP.arena(S, 5, F32, col0=0, pad_cols=0, device=DEV)

    def weights(**kw):
        a = dict(off=off.data_ptr(), perm=None, src32=idx.data_ptr(), rel=rel.data_ptr(), dim=2, power=2, n_nodes=n, n_entries=S,
                 c=c_out.data_ptr(), src=idx.data_ptr(), degenerate=deg.data_ptr())
        a.update(kw)
        rc = lib.g4c_mesh_jet_weights(a["off"], a["perm"], a["src32"], a["rel"], a["dim"], a["power"], a["n_nodes"], a["n_entries"], a["c"],
                                      a["src"], a["degenerate"], stream)
        return rc, lib.g4c_last_error().decode()

    for kw, code, word in ((dict(dim=4), _lib.EUNSUPPORTED, "dim=4"), (dict(power=3), _lib.EINVAL, "power=3"), (dict(power=-1), _lib.EINVAL, "power=-1"),
                           (dict(n_nodes=-1), _lib.EINVAL, "bad sizes"), (dict(n_entries=-1), _lib.EINVAL, "bad sizes"),
                           (dict(off=None), _lib.EINVAL, "null"), (dict(src32=None), _lib.EINVAL, "null"), (dict(rel=None), _lib.EINVAL, "null"),
                           (dict(c=None), _lib.EINVAL, "null"), (dict(src=None), _lib.EINVAL, "null"), (dict(degenerate=None), _lib.EINVAL, "null")):
        rc, msg = weights(**kw)
        assert rc == code and "g4c_mesh_jet_weights" in msg and word in msg, (kw, rc, msg)
    assert weights(n_entries=0)[0] == _lib.OK and weights(n_nodes=0)[0] == _lib.OK          # nothing to do: no launch
    torch.cuda.synchronize(DEV)
    FP.assert_footprint(whole2, out2, written_rows=range(0), what="refusals: five fields")
    FP.assert_footprint(c_whole, c_out, written_rows=range(0), what="refusals: weights")
    assert int((deg == 7).sum()) == n


# ====================================================================== gfd.MeshJet
def test_k_stencils_stay_inside_their_graph_of_a_batch():
    """Two graphs over the same unit square, collated: a search over the collated positions would mix them."""
    rng = np.random.default_rng(3)
    n0, n1, k = 400, 300, 12
    pos = np.concatenate([rng.random((n0, 2)), rng.random((n1, 2))]).astype(np.float32)
    g = gfd.Graph(pos=torch.from_numpy(pos))
    g.batch = torch.cat([torch.zeros(n0, dtype=torch.long), torch.ones(n1, dtype=torch.long)])
    op = gfd.MeshJet(g.to(DEV), k=k)
    src = op.src.cpu().numpy().reshape(n0 + n1, k)
    assert (src[:n0] < n0).all() and (src[n0:] >= n0).all() and not (src == np.arange(n0 + n1)[:, None]).any()
    # and they are the k nearest of that graph (as sets: ties aside, which a random cloud in fp32 does not have)
    for a, b in ((0, n0), (n0, n0 + n1)):
        want = J.nearest(pos[a:b].astype(np.float64), k) + a
        assert np.array_equal(np.sort(src[a:b], 1), np.sort(want, 1))
    assert not bool(op.degenerate.any()) and "k=12" in repr(op)
    mixed = gfd.MeshJet(gfd.Graph(pos=torch.from_numpy(pos)).to(DEV), k=k).src.cpu().numpy().reshape(n0 + n1, k)
    assert (mixed[:n0] >= n0).any()          # the control: without `batch` the search does cross


def test_a_periodic_mesh_is_differentiated_across_its_seam():
    """k=None with the wrapped edge vectors of a mesh that is periodic in x and y: f = sin 2πx sin 2πy.  The device's Laplacian equals
    the fp64 restatement's on the same vectors within the fp32 bounds (the table: 2^-23 max|c| Σ|Δf| for each of its two columns; the
    sum: (deg + 3) 2^-24 Σ|c||Δf|), and
    that restatement is no worse at the nodes whose stencil crosses the seam than at the others (allowed: twice the others' relative
    r.m.s. — the same fit on the same kind of stencil); with the unwrapped differences of the positions, a period off on those
    entries, it is at least ten times worse at those nodes."""
    n, k = 1600, 12
    m = int(np.sqrt(n))
    rng = np.random.default_rng(8)
    grid = np.stack(np.meshgrid(np.arange(m), np.arange(m), indexing="ij"), -1).reshape(-1, 2)
    pos = ((grid + 0.5 + 0.3 * (rng.random((n, 2)) - 0.5)) / m).astype(np.float32).astype(np.float64)
    d = pos[None, :, :] - pos[:, None, :]
    d -= np.round(d)                                   # the minimum image: sender − receiver, wrapped
    r2 = (d ** 2).sum(-1)
    np.fill_diagonal(r2, np.inf)
    nbr = np.argsort(r2, axis=1, kind="stable")[:, :k]
    col = np.repeat(np.arange(n), k)
    row = nbr.reshape(-1)
    wrapped = (-d[col, row]).astype(np.float32)          # receiver − sender
    g = gfd.Graph(pos=torch.from_numpy(pos).float(), edge_index=torch.from_numpy(np.stack([row, col])))
    g = g.to(DEV)
    f = (np.sin(2 * np.pi * pos[:, 0]) * np.sin(2 * np.pi * pos[:, 1])).astype(np.float32)[:, None]
    lap = -8 * np.pi ** 2 * f[:, 0].astype(np.float64)
    op = gfd.MeshJet(g, power=2, edge_vectors=dev(wrapped))
    assert not bool(op.degenerate.any()) and "in-edges" in repr(op)
    got = op.derived(dev(f), ("lap:0",)).cpu().numpy()[:, 0]
    off = np.arange(0, n * k + 1, k)
    c64, _, src, _ = J.weights(off, None, row.astype(np.int32), wrapped, 2, 2)
    ref = J.jets64(f.astype(np.float64), off, c64, src)[:, 0]
    ref = ref[:, 2] + ref[:, 4]
    adiff = np.abs(f[src, 0].astype(np.float64) - f[col, 0])
    top = np.abs(c64).max(1).reshape(n, k).max(1)
    mag = ((np.abs(c64[:, 2]) + np.abs(c64[:, 4])) * adiff).reshape(n, k).sum(1)
    allowed = 2 * 2.0 ** -23 * top * adiff.reshape(n, k).sum(1) + (k + 3) * 2.0 ** -24 * mag * (1 + 2.0 ** -20)
    note("periodic: |lap - fp64| / the fp32 bounds", J.within(got, ref, allowed, "lap"))
    seam = (np.abs(wrapped.astype(np.float64) - (pos[col] - pos[row])).max(1) > 0.5).reshape(n, k).any(1)
    assert 0.05 * n < seam.sum() < 0.5 * n

    def rel_rms(v, sel):
        return float(np.sqrt(((v - lap)[sel] ** 2).mean() / (lap ** 2).mean()))

    assert rel_rms(ref, seam) <= 2.0 * rel_rms(ref, ~seam)
    note("periodic: seam error / twice the interior's", rel_rms(ref, seam) / (2.0 * rel_rms(ref, ~seam)))
    plain = gfd.MeshJet(g, power=2).derived(dev(f), ("lap:0",)).cpu().numpy()[:, 0]          # the control: pos[col] − pos[row], a period off
    assert rel_rms(plain, seam) >= 10.0 * rel_rms(got, seam)


def test_manufactured_flows_have_zero_residual_on_the_device():
    """Plane Poiseuille flow and solid-body rotation on a jittered lattice whose coordinates are multiples of 2^-10, with dyadic
    constants (ν = 1/16, ρ = 2, a = 1/2, Ω = 1): positions, stencil vectors and all three fields are exact in fp32, and the fit is
    exact on them in exact arithmetic.  So each derivative the device returns is off its true value by at most
        E = 2 · 2^-23 max|c| Σ_s |Δx_s|  (the table: 2^-23 max|c| per entry from the fp64 solve's rounding to fp32, pinned above, and
                                          as much again for the fp64 restatement's own distance from the exact fit: < 1e-9 relative)
          + (k + 3) 2^-24 Σ_s |c_s| |Δx_s|  (the fp32 sum)
    and the residual, formed in fp64 from the device's eight columns, by Σ_b |U_b| E(∂_b U_a) + E(∂_a P) / ρ + ν E(∇²U_a)."""
    n, k, nu, rho = 2025, 12, 1.0 / 16, 2.0
    m = J.stencil_mesh(n, 2, kind="lattice", plant=False)
    pos = np.round(m.pos * 1024) / 1024
    assert len({tuple(p) for p in pos}) == n
    x, y = pos[:, 0], pos[:, 1]
    flows = {"poiseuille": np.stack([0.5 * y * y - 0.25 * y + 0.25, 0 * x, 2 * nu * rho * 0.5 * x], 1),
             "rotation": np.stack([-y, x, rho * (x * x + y * y) / 2], 1)}
    g = gfd.Graph(pos=torch.from_numpy(pos).float()).to(DEV)
    assert np.array_equal(g.pos.cpu().numpy().astype(np.float64), pos)
    op = gfd.MeshJet(g, k=k, power=2)
    assert not bool(op.degenerate.any())
    c, src, off = op.c.cpu().numpy().astype(np.float64), op.src.cpu().numpy(), op.off.cpu().numpy()
    names = ("grad:0", "grad:1", "grad:2", "lap:0", "lap:1")
    for name, u in flows.items():
        assert np.array_equal(u.astype(np.float32).astype(np.float64), u), name
        d = op.derived(dev(u.astype(np.float32)), names).cpu().numpy().astype(np.float64)
        adiff = np.abs(u[src] - np.repeat(u, k, axis=0))                               # [S, 3]
        top = np.abs(c).max(1).reshape(n, k).max(1)[:, None]
        e_tab = 2 * 2.0 ** -23 * top * adiff.reshape(n, k, 3).sum(1)                    # [n, 3]: any derivative of field f
        first = lambda f, a: e_tab[:, f] + (k + 3) * 2.0 ** -24 * (np.abs(c[:, a]) * adiff[:, f]).reshape(n, k).sum(1)          # noqa: E731
        lapl = lambda f: 2 * e_tab[:, f] + (k + 3) * 2.0 ** -24 * ((np.abs(c[:, 2]) + np.abs(c[:, 4])) * adiff[:, f]).reshape(n, k).sum(1)  # noqa: E731
        worst = 0.0
        for a in (0, 1):
            r = u[:, 0] * d[:, 2 * a] + u[:, 1] * d[:, 2 * a + 1] + d[:, 4 + a] / rho - nu * d[:, 6 + a]          # prev = the same field
            allowed = np.abs(u[:, 0]) * first(a, 0) + np.abs(u[:, 1]) * first(a, 1) + first(2, a) / rho + nu * lapl(a)
            worst = max(worst, J.within(r, np.zeros(n), allowed * (1 + 2.0 ** -20), f"{name} R_{a}"))
        cont = d[:, 0] + d[:, 3]
        worst = max(worst, J.within(cont, np.zeros(n), (first(0, 0) + first(1, 1)) * (1 + 2.0 ** -20), f"{name} C"))
        note(f"device residual of {name} / the fp32 bound", worst)
        # the control: a wrong sign of the advection leaves 2 Ω² |x| in the rotation
        if name == "rotation":
            r = -(u[:, 0] * d[:, 0] + u[:, 1] * d[:, 1]) + d[:, 4] / rho - nu * d[:, 6]
            assert np.abs(r).max() > 1.0


def test_zz_print_the_measured_ratios():
    """Not a check of its own: the measured / allowed ratio of every bound above, for tests/JET_MEASURED.md (pytest -s)."""
    for k, v in sorted(RATIOS.items()):
        print(f"MEASURED {k}: {v:.3f}")
        assert v <= 1.0
