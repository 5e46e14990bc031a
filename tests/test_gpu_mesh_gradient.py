"""g4c_mesh_gradient_weights and g4c_mesh_derived (csrc/mesh_gradient.hip) through ops.mesh_* against the numpy restatement of
tests/gradient_ref.py, and the flow diagnostics of `Rollout(derived=)` / `GNN.diagnostics` / `GNN.evaluate(derived=)` /
`gfd.MeshGradient` against the restatement run over the rollout's own `result()`.

Kernel level: every output lives in a sentinel-filled buffer with padding on both sides that is compared whole.  The weights are
compared with the fp64 restatement within 2^-23 max_e ||g_e||_inf per node (half an ulp of the one rounding to fp32 and a margin of
the same size; tests/test_gradient_ref.py asserts that no node of these meshes sits near the degeneracy threshold, so the flags are
exact); the per-step launch is bit for bit the restatement's numpy.float32 loop, within (max_deg + 3) 2^-24 Σ|terms| of its fp64 form,
its statistics bit for bit on integers and within the records' 2 (n + 4) 2^-53 Σ|terms| on floats (the maximum bit for bit).

End to end the restatement's per-step loop runs from the DEVICE's weights (they are pinned above): the rollout's snapshots are then
bit for bit the loop's over `result()` when the rollout keeps the caller's numbering, and within the fp32 bound when it renumbers."""
import ctypes as C
import functools
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

import gradient_ref as R                                 # noqa: E402
import moments_ref as M                                  # noqa: E402
import graphs4cfd_amd as gfd                             # noqa: E402
from graphs4cfd_amd import _lib, ops, synthetic as S     # noqa: E402
from graphs4cfd_amd.nn.model import Rollout              # noqa: E402

DEV = torch.device("cuda", 0)
F32, F64, I32, U8 = torch.float32, torch.float64, torch.int32, torch.uint8
SENT, ISENT, USENT, PAD = -7777.0, -7777, 77, 3
RATIOS = {}          # bound -> the largest measured / allowed seen (printed by the last test; tests/DERIVED_MEASURED.md)


def note(name, r):
    RATIOS[name] = max(RATIOS.get(name, 0.0), float(r))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@functools.lru_cache(maxsize=None)
def mesh_of(kind, n, dim, shuffled):
    m = R.uniform_mesh(n, dim) if kind == "uniform" else R.ragged_mesh(n, dim)
    return m.shuffled(11) if shuffled else m


def csr_of(m):
    return types.SimpleNamespace(off=dev(m.off), perm=None if m.perm is None else dev(m.perm), n=int(m.row.size))


# ====================================================================== weights
@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 257, 1000])
def test_weights_match_the_restatement(n, dim):
    for kind in ("uniform", "ragged"):
        for shuffled in (False, True):
            m = mesh_of(kind, n, dim, shuffled)
            n_e = int(m.row.size)
            assert not shuffled or n < 63 or m.perm is not None
            for power in (0, 1, 2):
                what = f"{kind} n {n} dim {dim} shuffled {shuffled} power {power}"
                gbuf = torch.full((n_e + 2 * PAD, dim), SENT, dtype=F32, device=DEV)
                sbuf = torch.full((n_e + 2 * PAD,), ISENT, dtype=I32, device=DEV)
                dbuf = torch.full((n + 2 * PAD,), USENT, dtype=U8, device=DEV)
                rel, src32 = dev(m.rel), dev(m.src32)
                rel0, src0 = rel.clone(), src32.clone()
                out = ops.mesh_gradient_weights(rel, csr_of(m), src32, power, out=(gbuf[PAD:PAD + n_e], sbuf[PAD:PAD + n_e], dbuf[PAD:PAD + n]))
                g64, g32, src, degen = R.weights(m.off, m.perm, m.src32, m.rel, dim, power)
                wrote = n > 0 and n_e > 0
                want_d = np.full(n + 2 * PAD, USENT, np.uint8)
                want_s = np.full(n_e + 2 * PAD, ISENT, np.int32)
                if wrote:
                    want_d[PAD:PAD + n], want_s[PAD:PAD + n_e] = degen, src
                R.same(dbuf, want_d, what + ", degenerate")
                R.same(sbuf, want_s, what + ", src")
                assert bool((gbuf[:PAD] == SENT).all()) and bool((gbuf[PAD + n_e:] == SENT).all()), what + ": the padding of g was written"
                if wrote:
                    note("weights: |g - g_ref| / (2^-23 max ||g_ref||_inf)", R.within(out[0], g64, R.weights_bound(g64, m.off), what + ", g"))
                    node = np.repeat(np.arange(n), np.diff(m.off))
                    assert not out[0].cpu().numpy()[degen[node] == 1].any(), what
                else:
                    assert bool((gbuf == SENT).all()), what
                assert torch.equal(rel, rel0) and torch.equal(src32, src0)


def test_weights_without_out_and_negative_controls():
    m = mesh_of("ragged", 257, 2, True)
    g, src, degen = ops.mesh_gradient_weights(dev(m.rel), csr_of(m), dev(m.src32), 2)
    g64, g32, src_ref, degen_ref = R.weights(m.off, m.perm, m.src32, m.rel, 2, 2)
    R.within(g, g64, R.weights_bound(g64, m.off), "g")
    R.same(src, src_ref, "src")
    R.same(degen, degen_ref, "degenerate")
    t64 = R.weights(m.off, m.perm, m.src32, m.rel, 2, 2, wrong="transposed-g")[0]
    assert R.rejects(R.within, g, t64, R.weights_bound(t64, m.off), "transposed")
    assert R.rejects(R.same, src, R.weights(m.off, m.perm, m.src32, m.rel, 2, 2, wrong="src-unpermuted")[2], "unpermuted")
    empty = types.SimpleNamespace(off=torch.zeros(5, dtype=I32, device=DEV), perm=None, n=0)          # four nodes, no edge
    g, src, degen = ops.mesh_gradient_weights(torch.zeros(0, 3, device=DEV), empty, torch.zeros(0, dtype=I32, device=DEV), 1)
    assert tuple(g.shape) == (0, 3) and degen.tolist() == [1, 1, 1, 1]


# ====================================================================== the per-step launch
MAX_STEPS = 7


def structured(n, dim, rng, integer):
    """A mesh of uniform in-degree 6 given by its tables alone (no geometry): for the sizes a brute-force search cannot reach."""
    off = (np.arange(n + 1) * 6).astype(np.int32)
    src = ((np.arange(n)[:, None] + np.array([1, 2, 3, n - 1, n - 2, n - 3])[None, :]) % max(n, 1)).reshape(-1).astype(np.int32)
    g = rng.integers(-4, 5, (6 * n, dim)).astype(np.float32) if integer else rng.standard_normal((6 * n, dim)).astype(np.float32)
    return off, g, src, 6


class Step:
    """The device buffers of one case of g4c_mesh_derived, and one checked launch."""

    def __init__(self, tables, dim, nf, names, kind, every=1, padded=True, velocity=None, field_scale=None, seed=0, wrong=None):
        self.off, self.g, self.src, self.max_deg = tables
        n = self.n = len(self.off) - 1
        self.nf, self.kind, self.every = nf, kind, every
        self.rng = np.random.default_rng(1000 * n + 10 * nf + seed)
        if kind == "int":
            self.g = self.rng.integers(-4, 5, self.g.shape).astype(np.float32)
        self.prog = R.program(names, dim, nf, velocity, field_scale)
        self.ref_prog = R.program(names, dim, nf, velocity, field_scale, wrong=wrong)
        nd = self.nd = len(self.prog)
        self.what = f"n {n} dim {dim} nf {nf} {names} {kind} every {every}"
        self.dg, self.dsrc, self.doff = dev(self.g), dev(self.src), dev(self.off)
        self.wide = torch.full((n, nf + (3 if padded else 0)), SENT, dtype=F32, device=DEV)
        self.x = self.wide[:, :nf]
        self.curbuf = torch.full((n + 2 * PAD, nd), SENT, dtype=F32, device=DEV)
        self.cur = self.curbuf[PAD:PAD + n]
        self.n_snap = MAX_STEPS // every if every else 0
        self.snapbuf = torch.full((self.n_snap + 2, n, nd), SENT, dtype=F32, device=DEV) if every else None
        self.statbuf = torch.full((MAX_STEPS + 2, nd, 3), SENT, dtype=F64, device=DEV)
        self.scratch = ops.mesh_derived_scratch(n, nd, DEV)
        self.step = torch.zeros(2, dtype=I32, device=DEV)
        self.want_snap = None if every == 0 else np.full((self.n_snap + 2, n, nd), SENT, np.float32)
        self.want_stat = np.full((MAX_STEPS + 2, nd, 3), SENT, np.float64)

    def draw(self):
        if self.kind == "int":
            return self.rng.integers(-8, 9, (self.n, self.nf)).astype(np.float32)
        return self.rng.standard_normal((self.n, self.nf)).astype(np.float32)

    def launch(self, t, check=True):
        x = self.draw()
        self.x.copy_(dev(x))
        wide0 = self.wide.clone()
        self.step.copy_(torch.tensor([t, 0], dtype=I32))
        ops.mesh_derived(self.x, self.doff, self.dg, self.dsrc, self.prog, self.cur, step=self.step, every=self.every,
                         snap=None if self.snapbuf is None else self.snapbuf[1:-1], stats=self.statbuf[1:-1], scratch=self.scratch,
                         max_steps=MAX_STEPS, nf=self.nf)
        self.last_x = x
        if not check:
            return
        what = f"{self.what} launch {t}"
        cur = R.derived32(x, self.off, self.g, self.src, self.ref_prog)
        want = np.full(tuple(self.curbuf.shape), SENT, np.float32)
        want[PAD:PAD + self.n] = cur
        R.same(self.curbuf, want, what + ", cur")
        cur64, mag = R.derived64(x, self.off, self.g, self.src, self.ref_prog)
        note("per step: |cur - fp64| / ((max_deg + 3) 2^-24 sum|terms|)", R.within(self.cur, cur64, R.bound32(mag, self.max_deg), what + ", fp64"))
        slot = R.snap_slot(t, self.every, self.n_snap)
        if slot is not None and self.n:
            self.want_snap[1 + slot] = cur
        if self.snapbuf is not None:
            R.same(self.snapbuf, self.want_snap, what + ", snapshots")
        if 0 <= t < MAX_STEPS and self.n:
            st = R.stats64(cur)
            got = self.statbuf[1 + t].cpu().numpy()
            if self.kind == "int":
                self.want_stat[1 + t] = st
            else:
                R.same(got[:, 2], st[:, 2], what + ", max|q|")
                note("statistics: |sum - fp64| / (2 (n + 4) 2^-53 sum|terms|)", R.within(got[:, :2], st[:, :2], R.stats_bound(cur), what + ", sums"))
                self.want_stat[1 + t] = got
        R.same(self.statbuf, self.want_stat, what + ", stats")
        assert self.step.tolist() == [t, 0], what
        assert torch.equal(self.wide, wide0), what + ": x was written"
        R.same(self.dg, self.g, what + ", g")
        R.same(self.dsrc, self.src, what + ", src")


def tables_of(kind, n, dim, shuffled, power=2):
    m = mesh_of(kind, n, dim, shuffled)
    g32, src = R.weights(m.off, m.perm, m.src32, m.rel, dim, power)[1:3]
    return m.off, g32, src, m.max_deg


PROGRAMS = {          # (dim, nf) -> [(names, velocity, field_scale)]
    (2, 1): [(("grad:0",), None, None)],
    (3, 1): [(("grad:0",), None, None)],
    (2, 2): [(("div",), None, None), (("vort",), None, None), (("div", "vort", "grad:1"), None, [2.0, -0.5])],
    (3, 2): [(("grad:0", "grad:1"), None, None)],
    (2, 3): [(("div", "vort"), None, None), (("div", "vort", "grad:0", "grad:1", "grad:2"), None, None)],
    (3, 3): [(("div", "vort"), None, None), (("div", "vort", "grad:0", "div"), None, [0.5, 2.0, -4.0])],
    (2, 5): [(("grad:4", "div", "vort"), (3, 1), [1.0, 2.0, 1.0, -0.25, 8.0])],
    (3, 5): [(("div", "grad:3", "vort"), (4, 2, 0), None)],
}


@pytest.mark.parametrize("nf", [1, 2, 3, 5])
@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("n", [0, 1, 65, 257, 1000])
def test_the_per_step_launch_matches_the_restatement(n, dim, nf):
    for kind, shuffled in (("uniform", False), ("ragged", True)):
        tables = tables_of(kind, n, dim, shuffled)
        for names, velocity, scale in PROGRAMS[(dim, nf)]:
            for data in ("float", "int"):
                c = Step(tables, dim, nf, names, data, every=1, padded=data == "float", velocity=velocity, field_scale=scale)
                c.launch(1)
                c.launch(MAX_STEPS)          # past the record: cur only


@pytest.mark.parametrize("every", [0, 1, 3])
def test_snapshots_and_statistics_follow_the_step_index(every):
    for dim, nf, n in ((2, 3, 257), (3, 3, 65)):
        c = Step(tables_of("ragged", n, dim, True, power=1), dim, nf, ("div", "vort"), "float", every=every)
        for t in list(range(MAX_STEPS + 2)) + [-1, 2]:          # (and step 2 once more: its slot and its row are overwritten)
            c.launch(t)
        if every:
            assert bool((c.snapbuf[1:-1] != SENT).all()) and bool((c.snapbuf[0] == SENT).all()) and bool((c.snapbuf[-1] == SENT).all())


def test_a_linear_field_gives_back_its_slope():
    for dim in (2, 3):
        m = mesh_of("uniform", 1000, dim, False)
        off, g32, src, max_deg = tables_of("uniform", 1000, dim, False)
        slope = np.random.default_rng(3).standard_normal((2, dim))
        x = (m.pos @ slope.T).astype(np.float32)
        prog = R.program(("grad:0", "grad:1"), dim, 2)
        cur = torch.empty(m.n, 2 * dim, device=DEV)
        ops.mesh_derived(dev(x), dev(off), dev(g32), dev(src), prog, cur)
        cur64, mag = R.derived64(x, off, g32, src, prog)
        note("per step: |cur - fp64| / ((max_deg + 3) 2^-24 sum|terms|)", R.within(cur, cur64, R.bound32(mag, max_deg), f"dim {dim}"))
        R.within(cur, np.tile(slope.reshape(-1), (m.n, 1)), slope_bound(x, off, g32, src, m.rel, prog, max_deg, np.abs(slope).max()), f"slope, dim {dim}")


def slope_bound(x, off, g, src, rel, prog, max_deg, smax):
    """How far the fp32 gradient of a linear field may sit from its slope.  The fp64 weights give the slope back exactly for the edge
    vectors they were built from; what is left are roundings to fp32, 2^-24 relative each: of the launch's own arithmetic
    ((max_deg + 3) Σ|terms|), of g (Σ|terms|), of the two values of x in a difference (Σ|c| |g| (|x_src| + |x_i|)), and of the edge
    vectors rel (built from rounded coordinates, two roundings: Σ|c| |g| ||rel||_1 max|slope| twice) — summed, with one unit of margin
    on the first."""
    n = len(off) - 1
    node = np.repeat(np.arange(n), np.diff(off))
    mag = R.derived64(x, off, g, src, prog)[1]
    ends, geom = np.zeros((n, len(prog))), np.zeros((n, len(prog)))
    for c, col in enumerate(prog):
        for (f, a, coef) in col:
            ga = abs(float(coef)) * np.abs(g[:, a].astype(np.float64))
            np.add.at(ends[:, c], node, ga * (np.abs(x[src, f]) + np.abs(x[node, f])))
            np.add.at(geom[:, c], node, ga * np.abs(rel.astype(np.float64)).sum(1) * smax)
    return 2.0 ** -24 * ((max_deg + 5) * mag + ends + 2 * geom)


BIG = 262_144 + 300          # 1024 workgroups of 256: 300 threads take a second row


@pytest.mark.parametrize("kind", ["float", "int"])
def test_large_mesh_takes_several_rows_per_thread(kind):
    tables = structured(BIG, 2, np.random.default_rng(9), kind == "int")
    c = Step(tables, 2, 3, ("div", "vort"), kind, every=3)
    c.launch(2)


def test_two_runs_give_the_same_bits():
    runs = []
    for _ in range(2):
        c = Step(structured(BIG, 3, np.random.default_rng(9), False), 3, 3, ("div", "vort"), "float", every=1, seed=4)
        for t in range(3):
            c.launch(t, check=False)
        torch.cuda.synchronize(DEV)
        runs.append(c)
    a, b = runs
    assert torch.equal(a.statbuf, b.statbuf) and torch.equal(a.curbuf, b.curbuf) and torch.equal(a.snapbuf, b.snapbuf)
    assert bool((a.statbuf[1:4] != SENT).all()) and bool((a.statbuf[4:] == SENT).all())


def test_negative_controls_on_the_launch():
    """The launch's own output fails the comparison with a restatement that makes one mistake."""
    m = mesh_of("ragged", 257, 2, True)
    right = tables_of("ragged", 257, 2, True)
    Step(right, 2, 3, ("div", "vort"), "float").launch(0)
    c = Step(right, 2, 3, ("div", "vort"), "float", wrong="vort-sign")
    with pytest.raises(AssertionError, match="cur"):
        c.launch(0)
    for wrong in ("transposed-g", "src-unpermuted"):
        g32, src = R.weights(m.off, m.perm, m.src32, m.rel, 2, 2, wrong=wrong)[1:3]
        c = Step(right, 2, 3, ("div", "vort"), "float")
        c.launch(0, check=False)
        ref = R.derived32(c.last_x, m.off, g32, src, c.prog)
        assert R.rejects(R.same, c.cur, ref, wrong), wrong
        assert not R.rejects(R.same, c.cur, R.derived32(c.last_x, m.off, right[1], right[2], c.prog), "right")


def test_refusals_return_their_code_without_launching():
    lib = _lib.load()
    n, n_e, nf = 64, 128, 3
    x, g, src = torch.ones(n, nf, device=DEV), torch.ones(n_e, 2, device=DEV), torch.zeros(n_e, dtype=I32, device=DEV)
    off = torch.arange(0, n_e + 1, 2, dtype=I32, device=DEV)
    cur = torch.full((n, 8), SENT, device=DEV)
    stats, scratch = torch.full((4, 8, 3), SENT, dtype=F64, device=DEV), torch.full((64,), SENT, dtype=F64, device=DEV)
    step = torch.zeros(2, dtype=I32, device=DEV)

    def run(prog_kw=None, n_nodes=n, **kw):
        d = _lib.g4c_mesh_derived_t(**dict(dict(dim=2, nf=nf, x_ld=nf, g=g.data_ptr(), src=src.data_ptr(), off=off.data_ptr(), cur=cur.data_ptr(),
                                                step=step.data_ptr(), every=0, n_snap=0, max_steps=4, snap=None, stats=stats.data_ptr(),
                                                scratch=scratch.data_ptr()), **kw))
        p = _lib.g4c_derived_program_t(nd=1)
        p.n_terms[0], p.coef[0][0] = 1, 1.0
        for k, v in (prog_kw or {}).items():
            if k == "nd":
                p.nd = v
            elif k == "n_terms":
                p.n_terms[0] = v
            else:
                getattr(p, k)[0][0] = v
        rc = lib.g4c_mesh_derived(x.data_ptr(), C.byref(d), C.byref(p), n_nodes, _lib.stream_handle(DEV))
        return rc, lib.g4c_last_error().decode()

    for prog_kw, kw, code, word in ((dict(nd=9), {}, _lib.EUNSUPPORTED, "nd=9"), (dict(n_terms=4), {}, _lib.EUNSUPPORTED, "4 terms"),
                                    ({}, dict(dim=4), _lib.EUNSUPPORTED, "dim=4"), ({}, dict(dim=1), _lib.EUNSUPPORTED, "dim=1"),
                                    (dict(field=3), {}, _lib.EINVAL, "field 3"), (dict(field=-1), {}, _lib.EINVAL, "field -1"),
                                    (dict(axis=2), {}, _lib.EINVAL, "axis 2"), ({}, dict(x_ld=2), _lib.EINVAL, "x_ld"),
                                    ({}, dict(max_steps=-1), _lib.EINVAL, "bad sizes"), ({}, dict(every=-1), _lib.EINVAL, "bad sizes"),
                                    (dict(n_terms=0), {}, _lib.EINVAL, "0 terms"), (dict(nd=0), {}, _lib.EINVAL, "bad sizes"),
                                    ({}, dict(scratch=None), _lib.EINVAL, "scratch"), ({}, dict(step=None), _lib.EINVAL, "step"),
                                    ({}, dict(cur=None), _lib.EINVAL, "null")):
        rc, msg = run(prog_kw, **kw)
        assert rc == code and "g4c_mesh_derived" in msg and word in msg, (prog_kw, kw, rc, msg)
    assert run(n_nodes=-1)[0] == _lib.EINVAL
    gout, sout, dout = torch.full((n_e, 2), SENT, device=DEV), torch.full((n_e,), ISENT, dtype=I32, device=DEV), torch.full((n,), USENT, dtype=U8, device=DEV)
    for dim, power, nn, code in ((4, 2, n, _lib.EUNSUPPORTED), (2, 3, n, _lib.EINVAL), (2, -1, n, _lib.EINVAL), (2, 2, -1, _lib.EINVAL)):
        rc = lib.g4c_mesh_gradient_weights(off.data_ptr(), None, src.data_ptr(), g.data_ptr(), dim, power, nn, n_e, gout.data_ptr(),
                                           sout.data_ptr(), dout.data_ptr(), _lib.stream_handle(DEV))
        assert rc == code and "g4c_mesh_gradient_weights" in lib.g4c_last_error().decode(), (dim, power, nn, rc)
    assert lib.g4c_mesh_gradient_weights(off.data_ptr(), None, src.data_ptr(), g.data_ptr(), 2, 2, n, n_e, None, sout.data_ptr(), dout.data_ptr(),
                                         _lib.stream_handle(DEV)) == _lib.EINVAL
    torch.cuda.synchronize(DEV)
    for t, s in ((cur, SENT), (stats, SENT), (scratch, SENT), (gout, SENT), (sout, ISENT), (dout, USENT)):
        assert bool((t == s).all())
    assert step.tolist() == [0, 0]
    with pytest.raises(NotImplementedError, match="distinct fields"):          # nine fields in one program
        ops.mesh_derived(torch.ones(n, 9, device=DEV), off, g, src, [[(f, 0, 1.0)] for f in range(8)][:7] + [[(7, 0, 1.0), (8, 1, 1.0)]],
                         torch.empty(n, 8, device=DEV))


# ====================================================================== Rollout / diagnostics / evaluate / MeshGradient
N_OUT, NF = 7, 3
NAMES = ("div", "vort")


@pytest.fixture(scope="module")
def mesh():
    g = S.mus_graph(3000, levels=3, seed=3).to(DEV)
    g.batch = torch.zeros(g.num_nodes, dtype=torch.long, device=DEV)
    torch.manual_seed(4)
    model = gfd.nn.NsThreeScaleGNN(arch=S.mus_arch("NsThreeScaleGNN", 128), device=DEV)
    model.eval()
    full = model.solve(g.clone(), N_OUT)
    op = gfd.MeshGradient(g)                      # the caller's numbering; its weights are the restatement's within their bound
    col = g.edge_index[1].cpu().numpy()
    off, perm = R.csr_of(col, g.num_nodes)
    assert perm is None
    rel = (g.pos[g.edge_index[1]] - g.pos[g.edge_index[0]]).float().cpu().numpy()
    g64, g32, src, degen = R.weights(off, perm, g.edge_index[0].cpu().numpy().astype(np.int32), rel, 2, 2)
    R.within(op.g, g64, R.weights_bound(g64, off), "MeshGradient.g")
    R.same(op.src, src, "MeshGradient.src")
    R.same(op.degenerate.to(U8), degen, "MeshGradient.degenerate")
    assert not degen.any() and op.max_deg == 6
    tables = (off, op.g.cpu().numpy(), src, 6)
    return dict(g=g, model=model, full=full, op=op, tables=tables, runs={})


def per_step(result, nf=NF):
    r = result.cpu().numpy()
    return [np.ascontiguousarray(r[:, nf * t:nf * (t + 1)]) for t in range(r.shape[1] // nf)]


def check_against_result(d, res, tables, names, nf, every, exact, what, steps=None, first=0):
    """`d` (RolloutDerived) against the restatement run over the predictions `res` of the steps first, first + 1, ..."""
    off, g32, src, max_deg = tables
    prog = R.program(names, g32.shape[1], nf)
    nd = len(prog)
    preds = per_step(res, nf)
    assert d.columns == R.columns(names, g32.shape[1]) and d.names == tuple(names)
    snaps = None if d.snapshots is None else d.snapshots.cpu().numpy()
    sums = d.sums.numpy()
    for t in (range(first, len(preds)) if steps is None else steps):
        cur = R.derived32(preds[t], off, g32, src, prog)
        slot = R.snap_slot(t, every, 10 ** 6)
        got = None if slot is None else snaps[:, nd * slot:nd * (slot + 1)]
        if got is not None:
            if exact:
                R.same(got, cur, f"{what}, snapshot of step {t}")
            else:
                cur64, mag = R.derived64(preds[t], off, g32, src, prog)
                note("end to end, renumbered: |snapshot - fp64| / ((max_deg + 3) 2^-24 sum|terms|)",
                     R.within(got, cur64, R.bound32(mag, max_deg), f"{what}, snapshot of step {t}"))
        basis = cur if exact else got          # (a renumbered rollout: its sums against its own snapshot)
        if basis is not None:
            st = R.stats64(basis)
            R.same(sums[t][:, 2], st[:, 2], f"{what}, max|q| of step {t}")
            note("end to end: |sum - fp64| / (2 (n + 4) 2^-53 sum|terms|)", R.within(sums[t][:, :2], st[:, :2], R.stats_bound(basis), f"{what}, sums of step {t}"))
            n = basis.shape[0]
            assert np.allclose(d.rms[t].numpy(), np.sqrt(st[:, 0] / n), rtol=1e-12) and np.allclose(d.mean_abs[t].numpy(), st[:, 1] / n, rtol=1e-12)
            assert np.array_equal(d.max_abs[t].numpy(), st[:, 2])


def moments_equal_over(mo, samples, steps, start, stride, what, first=0):
    """The raw sums of `mo` are bit for bit tests/moments_ref.py's over `samples` (the derived columns of steps first, first + 1, ...;
    None for a step nobody kept — it must then lie off the window)."""
    shape = next(s for s in samples if s is not None).shape
    assert all(s is not None or not M.on_window(first + i, start, stride, steps) for i, s in enumerate(samples)), what
    samples = [np.zeros(shape, np.float32) if s is None else s for s in samples]
    st = M.run(samples, steps, start, stride, None, first=first)
    assert mo.count == M.count(st, stride) > 0 and mo.origin == int(st["window"][0]) and mo.stride == stride, (what, mo)
    for k, got in zip(M.NAMES, (mo.pivot, mo.sum, mo.sum2, mo.min, mo.max)):
        M.same(got, np.ascontiguousarray(st[k].T), f"{what}, {k}")


@pytest.mark.parametrize("capture", [True, False])
@pytest.mark.parametrize("reorder", [False, True])
def test_rollout_derived_equals_the_restatement_over_the_result(mesh, reorder, capture):
    with Rollout(mesh["model"], mesh["g"], N_OUT, capture=capture, reorder=reorder, every=1, derived=NAMES, derived_every=2,
                 derived_moments=(1, 2)) as ro:
        ro.run(N_OUT)
        assert (ro._perm is not None) == reorder
        res, d = ro.result(), ro.derived()
    what = f"reorder {reorder} capture {capture}"
    if not reorder:
        assert torch.equal(res, mesh["full"])
    assert type(d) is gfd.nn.RolloutDerived and tuple(d.sums.shape) == (N_OUT, 2, 3) and tuple(d.snapshots.shape) == (3000, 2 * (N_OUT // 2))
    assert d.degenerate.dtype == torch.bool and not bool(d.degenerate.any()) and d.moments.count == 3
    check_against_result(d, res, mesh["tables"], NAMES, NF, 2, not reorder, what)
    # the moments of steps 1, 3, 5 are those of the three snapshots kept (the same steps)
    snaps = per_step(d.snapshots, 2)
    moments_equal_over(d.moments, [None, snaps[0], None, snaps[1], None, snaps[2], None], N_OUT, 1, 2, what + ", moments")
    mesh["runs"][(reorder, capture)] = d
    other = mesh["runs"].get((reorder, not capture))
    if other is not None:          # captured == eager, bit for bit
        assert torch.equal(d.sums, other.sums) and torch.equal(d.snapshots, other.snapshots)
        for k in ("pivot", "sum", "sum2", "min", "max"):
            assert torch.equal(getattr(d.moments, k), getattr(other.moments, k)), k


@pytest.mark.parametrize("reorder", [False, True])
def test_derived_moments_equal_the_moments_restatement_over_the_derived_snapshots(mesh, reorder):
    with Rollout(mesh["model"], mesh["g"], N_OUT, reorder=reorder, every=0, derived=NAMES, derived_every=1, derived_moments=(1, 2)) as ro:
        ro.run(N_OUT)
        d = ro.derived()
        assert ro._out_steps is None
    assert d.moments.count == 3 and tuple(d.moments.sum2.shape) == (3000, 3)
    moments_equal_over(d.moments, per_step(d.snapshots, 2), N_OUT, 1, 2, f"reorder {reorder}")
    if not reorder:
        check_against_result(d, mesh["full"], mesh["tables"], NAMES, NF, 1, True, "every step")


def test_a_rollout_without_derived_is_what_it_was(mesh, monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("a rollout without derived launched mesh_derived")
    calls, plain = [], ops.rollout_advance
    monkeypatch.setattr(ops, "mesh_derived", refuse)
    monkeypatch.setattr(ops, "mesh_gradient_weights", refuse)
    monkeypatch.setattr(ops, "rollout_moments", refuse)
    monkeypatch.setattr(ops, "rollout_advance_record", refuse)
    monkeypatch.setattr(ops, "rollout_advance", lambda *a, **k: (calls.append(1), plain(*a, **k))[1])
    with Rollout(mesh["model"], mesh["g"], N_OUT, reorder=False, capture=False) as ro:
        ro.run(N_OUT)
        assert ro._derived is None and len(calls) == N_OUT and torch.equal(ro.result(), mesh["full"])
        with pytest.raises(RuntimeError, match="derived"):
            ro.derived()
    assert torch.equal(mesh["model"].solve(mesh["g"].clone(), N_OUT), mesh["full"])
    with pytest.raises(AssertionError, match="mesh_derived|rollout without derived"):
        with Rollout(mesh["model"], mesh["g"], N_OUT, reorder=False, derived=NAMES) as ro:
            ro.run(1)


def test_rewind_leaves_the_diagnostics_of_the_steps_since(mesh):
    g, f0 = mesh["g"], mesh["g"].field
    try:
        with Rollout(mesh["model"], g, N_OUT, reorder=False, every=1, derived=NAMES, derived_every=1, derived_moments=(0, 2)) as ro:
            ro.run(3)
            before = ro.derived()
            check_against_result(before, ro.result(), mesh["tables"], NAMES, NF, 1, True, "before rewind", steps=range(3))
            ro.rewind()                                   # the device step index is 1 again: slots 1, 2, ... are written next
            assert ro.derived().moments.count == 0
            ro.run(4)
            res, d = ro.result(), ro.derived()
        assert torch.equal(res[:, 3:15], mesh["full"][:, 9:21])          # steps 3 .. 6 of the rollout sit in slots 1 .. 4
        check_against_result(d, res, mesh["tables"], NAMES, NF, 1, True, "after rewind", steps=range(1, 5))
        assert torch.equal(d.sums[0], before.sums[0]) and not torch.equal(d.sums[1], before.sums[1])
        moments_equal_over(d.moments, per_step(d.snapshots, 2)[1:5], N_OUT, 0, 2, "after rewind, moments", first=1)
        assert d.moments.origin == 2 and d.moments.count == 2
    finally:
        g.field = f0


def test_a_clipped_rollout_leaves_the_diagnostics_of_its_recomputation(mesh):
    import warnings
    g, f0 = mesh["g"], mesh["g"].field

    def run(precision=None):
        old = ops.set_mlp_precision(precision) if precision else None
        try:
            g.field = f0 * 1e5
            with Rollout(mesh["model"], g, N_OUT, reorder=False, every=1, derived=NAMES, derived_every=1, derived_moments=(1, 2)) as ro:
                ro.run(N_OUT)
                return ro.result().clone(), ro.derived(), ro
        finally:
            g.field = f0
            if old:
                ops.set_mlp_precision(old)

    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res, d, ro = run()
        res_x, d_x, ro_x = run("bf16x6")
    assert ro.exact_range and not ro_x.exact_range and torch.equal(res, res_x)
    assert torch.equal(d.sums, d_x.sums) and torch.equal(d.snapshots, d_x.snapshots) and torch.equal(d.moments.sum2, d_x.moments.sum2)
    moments_equal_over(d.moments, per_step(d.snapshots, 2), N_OUT, 1, 2, "clipped")


def test_diagnostics_and_evaluate(mesh):
    g, model = mesh["g"].clone(), mesh["model"]
    d = model.diagnostics(g.clone(), N_OUT)
    assert d.snapshots is None and d.moments is None and d.columns == ["div", "vort"] and tuple(d.rms.shape) == (N_OUT, 2)
    check_against_result(d, mesh["full"], mesh["tables"], NAMES, NF, 0, True, "diagnostics")
    kept = model.diagnostics(g.clone(), N_OUT, ("vort", "grad:2"), every=1, discard=2, stride=2, capture=False, power=1, field_scale=[1.0, 2.0, 0.5])
    assert kept.columns == ["vort", "d2/dx", "d2/dy"] and kept.moments.count == 3 and tuple(kept.snapshots.shape) == (3000, 3 * N_OUT)
    op1 = gfd.MeshGradient(g, power=1)
    want = op1.derived(mesh["full"][:, 3 * 4:3 * 5].contiguous(), ("vort", "grad:2"), field_scale=[1.0, 2.0, 0.5])
    assert torch.equal(kept.snapshots[:, 3 * 4:3 * 5], want)
    moments_equal_over(kept.moments, per_step(kept.snapshots, 3), N_OUT, 2, 2, "diagnostics, moments")
    g.target = torch.randn(g.num_nodes, NF * N_OUT, generator=torch.Generator().manual_seed(5)).to(DEV)
    plain = model.evaluate(g.clone())
    assert plain.derived is None
    errs = model.evaluate(g.clone(), derived=NAMES, derived_every=1)
    assert torch.equal(errs.sums, plain.sums) and torch.equal(errs.derived.sums, d.sums)
    check_against_result(errs.derived, mesh["full"], mesh["tables"], NAMES, NF, 1, True, "evaluate")


def tables_on(graph, power=2):
    op = gfd.MeshGradient(graph, power=power)
    off, perm = R.csr_of(graph.edge_index[1].cpu().numpy(), graph.num_nodes)
    rel = (graph.pos[graph.edge_index[1]] - graph.pos[graph.edge_index[0]]).float().cpu().numpy()
    g64, g32, src, degen = R.weights(off, perm, graph.edge_index[0].cpu().numpy().astype(np.int32), rel, int(graph.pos.size(1)), power)
    R.within(op.g, g64, R.weights_bound(g64, off), "g")
    R.same(op.src, src, "src")
    R.same(op.degenerate.to(U8), degen, "degenerate")
    return op, (off, op.g.cpu().numpy(), src, op.max_deg)


def test_list_of_two_graphs():
    gen = torch.Generator().manual_seed(8)
    graphs = [S.mus_graph(n, levels=1, seed=20 + n).to(DEV) for n in (300, 500)]
    for gr in graphs:
        gr.target = torch.randn(gr.num_nodes, NF * N_OUT, generator=gen).to(DEV)
    torch.manual_seed(9)
    model = gfd.nn.NsOneScaleGNN(arch=S.mus_arch("NsOneScaleGNN", 64), device=DEV)
    full = model.solve([gr.clone() for gr in graphs], N_OUT)
    both = gfd.nn.collate([gr.clone() for gr in graphs])
    op, tables = tables_on(both)
    d = model.diagnostics([gr.clone() for gr in graphs], N_OUT, every=2, discard=1, stride=2)
    assert tuple(d.snapshots.shape) == (800, 2 * 3) and d.moments.count == 3
    check_against_result(d, full, tables, NAMES, NF, 2, True, "two graphs")
    errs = model.evaluate([gr.clone() for gr in graphs], derived=("grad:1", "div"), derived_every=1)
    check_against_result(errs.derived, full, tables, ("grad:1", "div"), NF, 1, True, "two graphs, evaluate")


def test_remus():
    g = S.remus_graph(1500, k=5, seed=4).to(DEV)
    torch.manual_seed(6)
    model = gfd.nn.NsRotEquiTreeScaleGNN(arch=S.remus_arch(64), device=DEV)
    g.target = torch.randn(g.num_nodes, 2 * N_OUT, generator=torch.Generator().manual_seed(7)).to(DEV)
    full = model.solve(g.clone(), N_OUT)
    op, tables = tables_on(g)
    d = model.diagnostics(g.clone(), N_OUT, every=1, discard=0)
    assert d.columns == ["div", "vort"] and d.moments.count == N_OUT
    check_against_result(d, full, tables, NAMES, 2, 1, True, "REMuS")
    errs = model.evaluate(g.clone(), derived=("vort",), derived_every=3, derived_moments=True)
    check_against_result(errs.derived, full, tables, ("vort",), 2, 3, True, "REMuS, evaluate")
    with pytest.raises(ValueError, match="velocity"):
        model.diagnostics(g.clone(), N_OUT, velocity=(0, 2))


def test_mesh_gradient_on_the_target(mesh):
    g, op = mesh["g"], mesh["op"]
    slope = torch.tensor([[1.5, -2.0], [0.25, 3.0], [-1.0, 0.5]])
    target = (g.pos.cpu().double() @ slope.double().t()).float().to(DEV)          # [N, 3]: linear fields
    grad = op.gradient(target)
    assert tuple(grad.shape) == (3000, 3, 2) and op.columns(("div", "vort")) == ["div", "vort"]
    off, g32, src, max_deg = mesh["tables"]
    x = target.cpu().numpy()
    prog = R.program(("grad:0", "grad:1", "grad:2"), 2, 3)
    R.same(grad.reshape(3000, 6), R.derived32(x, off, g32, src, prog), "gradient")
    rel = (g.pos[g.edge_index[1]] - g.pos[g.edge_index[0]]).float().cpu().numpy()
    allowed = slope_bound(x, off, g32, src, rel, prog, max_deg, float(slope.abs().max()))
    R.within(grad.reshape(3000, 6), np.tile(slope.numpy().reshape(-1).astype(np.float64), (3000, 1)), allowed, "slope")
    dv = op.derived(target, ("div", "vort"))
    assert torch.allclose(dv[:, 0], torch.full((3000,), 1.5 + 3.0, device=DEV), atol=1e-3) and torch.allclose(dv[:, 1], torch.full((3000,), 0.25 + 2.0, device=DEV), atol=1e-3)
    with pytest.raises(ValueError, match="^x"):
        op.gradient(target[:-1])


def test_zz_print_the_measured_ratios():
    """Not a check: the measured / allowed ratio of every bound above, for tests/DERIVED_MEASURED.md (pytest -s)."""
    for k, v in sorted(RATIOS.items()):
        print(f"MEASURED {k}: {v:.3f}")
        assert v <= 1.0
