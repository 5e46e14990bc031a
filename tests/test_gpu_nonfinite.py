"""The in-step diagnostic launches on non-finite samples (tests/nonfinite_cases.py: NaN, +-Inf, an Inf pair, +-FLT_MAX, subnormals,
-0) placed so that one stage of a reduction is the only carrier: node 0, the wave edge, the fourth wave, the second workgroup, the
last node, inside / outside the mask, the first / a middle / the last sample in time, the last node of 65 537.

Every test runs its launch on clean and on poisoned data, outputs in guard arenas (tests/footprint.py), inputs frozen, and asserts
  (a) equality with the restatement — as integers where the output is fp32, NaN-equals-NaN where it is fp64;
  (b) locality: every output element that does not depend on a poisoned entry has the bits of the clean run;
  (c) the footprint;
  (d) two poisoned runs give identical bits, payloads included.
The rule (include/g4c.h): sums follow IEEE, an extremum over samples of which one is NaN is NaN, masks select."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]

import footprint as FP                                   # noqa: E402
import gradient_ref as GR                                # noqa: E402
import moments_ref as M                                  # noqa: E402
import nonfinite_cases as NC                             # noqa: E402
import record_ref as R                                   # noqa: E402
import spectrum_ref as SP                                # noqa: E402
from graphs4cfd_amd import _lib, ops                     # noqa: E402

DEV = torch.device("cuda", 0)
F32, F64, I32 = torch.float32, torch.float64, torch.int32


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def rows_arena(rows, cols, dtype):
    """(contiguous [rows, cols] view, whole): guard rows above and below, no padding columns (the launches want dense buffers)."""
    return FP.arena(rows, cols, dtype, col0=0, pad_cols=0, device=DEV)


def wholes_identical(a, b, what):
    for k in a:
        assert torch.equal(FP._int_view(a[k]), FP._int_view(b[k])), f"{what}: two runs differ in the bits of {k}"


def poisons_of(n):
    return NC.POISONS if n < NC.BIG else ("nan", "inf_pair")


def fields_of(n):
    return NC.FIELDS if n < NC.BIG else (3,)


# ====================================================================== g4c_rollout_advance_record
def run_record(pred, target, mask, nf, probe_rows, what):
    """One launch at step T_REC of STEPS_REC, every = 1: (views, wholes) of field, snap, probe_out, stats, scratch."""
    n, t, steps, P = pred.shape[0], NC.T_REC, NC.STEPS_REC, len(probe_rows)
    field0 = NC.clean(np.random.default_rng(n), n, 2 * nf)
    field, wf = rows_arena(n, 2 * nf, F32)
    field.copy_(dev(field0))
    snap, ws = rows_arena(steps * n, nf, F32)
    probe, wp = rows_arena(steps * P, nf, F32)
    stats, wst = rows_arena(steps * nf, R.NSTAT, F64)
    need = int(ops.rollout_record_scratch(n, nf, DEV).numel())
    scratch, wsc = FP.flat_arena(need, F64, device=DEV)
    step = torch.tensor([t, 0], dtype=I32, device=DEV)
    dpred, dtarget, dmask, drows = dev(pred), dev(target), None if mask is None else dev(mask), dev(np.asarray(probe_rows, np.int32))
    with FP.frozen(dpred, dtarget, dmask, drows, what=what):
        ops.rollout_advance_record(field, dpred, step, nf, steps, snap=snap.view(steps, n, nf), every=1, probe_rows=drows,
                                   probe_out=probe.view(steps, P, nf), target=dtarget, mask=dmask, stats=stats.view(steps, nf, R.NSTAT),
                                   scratch=scratch)
        torch.cuda.synchronize(DEV)
    assert step.tolist() == [t + 1, 0], what
    FP.assert_footprint(wf, field, None, what + ", field")
    FP.assert_footprint(ws, snap, range(t * n, (t + 1) * n), what + ", snap")
    FP.assert_footprint(wp, probe, range(t * P, (t + 1) * P), what + ", probe_out")
    FP.assert_footprint(wst, stats, range(t * nf, (t + 1) * nf), what + ", stats")
    FP.assert_footprint(wsc, scratch, None, what + ", scratch", inside=False)
    views = dict(field=field, snap=snap.view(steps, n, nf)[t], probe=probe.view(steps, P, nf)[t], stats=stats.view(steps, nf, R.NSTAT)[t])
    # data movement carries every bit, payloads included
    NC.identical(views["field"], np.concatenate([field0[:, nf:], pred], 1), what + ", field")
    NC.identical(views["snap"], pred, what + ", snap")
    NC.identical(views["probe"], pred[list(probe_rows)], what + ", probes")
    return views, dict(field=wf, snap=ws, probe=wp, stats=wst)


@pytest.mark.parametrize("n,placement", NC.cases())
def test_rollout_advance_record(n, placement):
    rows = NC.rows_of(n, placement)
    probe_rows = sorted(set(rows) | {0, n // 2})
    for nf in fields_of(n):
        for where in ("pred", "target"):
            for mask_kind in ("in", "out"):
                rng = np.random.default_rng(7 * n + nf)          # (record_case's clean draws)
                pred0, target0 = NC.clean(rng, n, nf), NC.clean(rng, n, nf * NC.STEPS_REC, lo=1)
                clean_runs = {}
                for name in poisons_of(n):
                    pred, target, mask_p, dirty_rows = NC.record_case(n, placement, name, nf, where, mask_kind)
                    what = f"n {n} {placement} {name} nf {nf} {where} mask {mask_kind}"
                    if mask_p.tobytes() not in clean_runs:          # the clean launch under the same mask
                        clean_runs[mask_p.tobytes()] = run_record(pred0, target0, mask_p, nf, probe_rows, what + ", clean")[0]
                        R.same(clean_runs[mask_p.tobytes()]["stats"],
                               R.step_stats(torch.from_numpy(pred0), torch.from_numpy(target0), NC.T_REC, torch.from_numpy(mask_p))[0], what + ", clean stats")
                    clean = clean_runs[mask_p.tobytes()]
                    got, wholes = run_record(pred, target, mask_p, nf, probe_rows, what)
                    want = R.step_stats(torch.from_numpy(pred), torch.from_numpy(target), NC.T_REC, torch.from_numpy(mask_p))[0]
                    R.same(got["stats"], want, what + ", stats")                                                          # (a)
                    f = nf - 1
                    if name == "nan":
                        s = got["stats"].cpu()
                        assert bool(s[f, R.MAX_ABS_ERR].isnan()) and bool(s[f, R.ABS_ERR_MASK].isnan()) == (mask_kind == "in"), what
                    if name == "subnormal":
                        continue          # (every entry is dirty: nothing is local)
                    # (b) what the poisoned column of `where` cannot reach keeps the clean run's bits
                    poisoned_fields = [f] + ([f - 1] if name == "flt_max" and nf > 1 else [])
                    local = np.ones((nf, R.NSTAT), bool)
                    for pf in poisoned_fields:
                        local[pf] = False
                        if where == "pred":
                            local[pf, [R.TGT_SUM, R.TGT_SQ_SUM]] = True
                        if mask_kind == "out":
                            local[pf, R.ABS_ERR_MASK] = True
                    NC.identical(got["stats"], clean["stats"], what + ", locality", where=local)
                    got2, wholes2 = run_record(pred, target, mask_p, nf, probe_rows, what)                                # (d)
                    wholes_identical(wholes, wholes2, what)


def test_record_negative_controls_on_the_launch():
    """The launch's statistics are rejected by a restatement with the old fmax, and by one with the old `ad * m`."""
    n, nf = 257, 3
    pred, target, mask, _ = NC.record_case(n, "wg2", "nan", nf, "pred", "out")
    got, _ = run_record(pred, target, mask, nf, [0, 256], "control")
    want = R.step_stats(torch.from_numpy(pred), torch.from_numpy(target), NC.T_REC, torch.from_numpy(mask))[0]
    R.same(got["stats"], want, "as it should be")
    d = torch.from_numpy(pred).double() - torch.from_numpy(target).double()[:, nf * NC.T_REC:nf * (NC.T_REC + 1)]
    old = want.clone()
    old[:, R.MAX_ABS_ERR] = torch.from_numpy(np.fmax.reduce(d.abs().numpy(), axis=0))
    assert bool(old[:, R.MAX_ABS_ERR].isfinite().all()) and R.rejects(R.same, got["stats"], old, "old fmax")
    old = want.clone()
    old[:, R.ABS_ERR_MASK] = (d.abs() * torch.from_numpy(mask)[:, None]).sum(0)
    assert bool(old[nf - 1, R.ABS_ERR_MASK].isnan()) and R.rejects(R.same, got["stats"], old, "old ad * m")


# ====================================================================== g4c_rollout_moments, g4c_rollout_spectrum
def run_accumulator(kind, samples, nf, K, sub, what, origin=1, state=None):
    """T_ACC launches (steps 0 .. T_ACC - 1, window (origin, 2)) of the moments (kind "moments") or the spectrum; all planes in one arena.
    `state`: (views, whole, window) of an earlier run to go on with."""
    n, steps = samples[0].shape[0], NC.T_ACC
    sizes = (nf, nf, ops.moment_pairs(nf), nf, nf) if kind == "moments" else (nf, nf, nf * K, nf * K)
    if state is None:
        view, whole = FP.arena(sum(sizes), n, F64, device=DEV)
        window = torch.tensor([origin, -1], dtype=I32, device=DEV)
    else:
        view, whole, window = state
        window.copy_(torch.tensor([origin, -1], dtype=I32))
    planes = view.split(sizes)
    step = torch.zeros(2, dtype=I32, device=DEV)
    dsub = None if sub is None else dev(sub)
    tw = None if kind == "moments" else spectrum_table(K).to(DEV)
    for t in range(steps):
        x = dev(samples[t])
        step.copy_(torch.tensor([t, 0], dtype=I32))
        with FP.frozen(x, dsub, tw, step, what=f"{what} step {t}"):
            if kind == "moments":
                ops.rollout_moments(x, step, nf, steps, window, *planes, stride=2, sub=dsub)
            else:
                ops.rollout_spectrum(x, step, nf, steps, window, tw, *planes, stride=2)
            torch.cuda.synchronize(DEV)
    FP.assert_footprint(whole, view, None, what)
    return planes, whole, (view, whole, window)


def spectrum_table(K):
    """Three samples, K frequencies from 0 up: bin 0 has sin = 0 exactly, so an infinite d meets a zero."""
    return ops.spectrum_table(freqs=[0.25 * k / max(K - 1, 1) for k in range(K)], samples=3, stride=2)[0]


def accumulator_ref(kind, samples, nf, K, sub, origin=1):
    n = samples[0].shape[0]
    if kind == "moments":
        st = M.new_state(n, nf, origin)
        for t in range(NC.T_ACC):
            st = M.accumulate(st, samples[t], t, NC.T_ACC, 2, sub)
        return [st[k] for k in M.NAMES]
    tw = spectrum_table(K).numpy()
    st = SP.new_state(n, nf, K, origin)
    for t in range(NC.T_ACC):
        st = SP.accumulate(st, samples[t], t, NC.T_ACC, tw, 2)
    return [st[k] for k in SP.NAMES]


def accumulator_local(kind, nf, K, dirty):
    """Per plane group, bool [planes, n]: the accumulators a dirty (node, field) entry cannot reach."""
    d = dirty.T          # [nf, n]
    if kind == "moments":
        pair = np.stack([d[f] | d[g] for f, g in M.pairs(nf)])
        return [~d, ~d, ~pair, ~d, ~d]
    return [~d, ~d, ~np.repeat(d, K, axis=0), ~np.repeat(d, K, axis=0)]


def accumulator_test(kind, n, placement, when, K=1):
    rows = NC.rows_of(n, placement)
    names = M.NAMES if kind == "moments" else SP.NAMES
    for nf in fields_of(n):
        for with_sub in ((False, True) if kind == "moments" else (False,)):
            sub = NC.clean(np.random.default_rng(5), n, nf * NC.T_ACC) if with_sub else None
            clean_samples = NC.time_samples(n, nf, "neg_zero", (), when)[0]
            clean, _, _ = run_accumulator(kind, clean_samples, nf, K, sub, f"{kind} n {n} nf {nf} clean")
            for name in poisons_of(n):
                samples, dirty = NC.time_samples(n, nf, name, rows, when)
                what = f"{kind} n {n} {placement} {name} nf {nf} K {K} {when} sub {with_sub}"
                got, whole, state = run_accumulator(kind, samples, nf, K, sub, what)
                want = accumulator_ref(kind, samples, nf, K, sub)
                for k, g, w in zip(names, got, want):
                    M.same(g, w, f"{what}, {k}")                                                                        # (a)
                if name != "subnormal":
                    for k, g, c, loc in zip(names, got, clean, accumulator_local(kind, nf, K, dirty)):
                        NC.identical(g, c, f"{what}, locality of {k}", where=loc)                                       # (b)
                _, whole2, _ = run_accumulator(kind, samples, nf, K, sub, what)
                assert torch.equal(FP._int_view(whole), FP._int_view(whole2)), what + ": two runs differ in their bits"  # (d)
                r, f = list(rows), nf - 1
                if kind == "moments" and name == "nan":
                    lo, hi = got[3].cpu().numpy(), got[4].cpu().numpy()
                    assert np.isnan(lo[f, r]).all() and np.isnan(hi[f, r]).all(), what + ": lo / hi lost the NaN"
                    # running through a rewritten origin replaces the record: the NaN is gone, and the restatement says the same
                    got3, _, _ = run_accumulator(kind, clean_samples, nf, K, sub, what + ", origin rewritten", origin=0, state=state)
                    want3 = accumulator_ref(kind, clean_samples, nf, K, sub, origin=0)
                    for k, g, w in zip(names, got3, want3):
                        M.same(g, w, f"{what}, origin rewritten, {k}")
                        assert bool(g.isfinite().all()), f"{what}, origin rewritten, {k}"
                if kind == "spectrum" and name in ("+inf", "-inf") and when == "first":
                    assert np.isnan(got[3].cpu().numpy()[f * K, r]).all(), what + ": Inf * 0 in bin 0"


# (the accumulators of a node are its own: one time placement at the large size)
@pytest.mark.parametrize("n,placement,when", [(n, p, w) for n, p in NC.cases() for w in NC.TIMES if n != NC.BIG or w == "middle"])
def test_rollout_moments(n, placement, when):
    accumulator_test("moments", n, placement, when)


@pytest.mark.parametrize("K", NC.BINS)
@pytest.mark.parametrize("n,placement", [c for c in NC.cases() if c[0] != NC.BIG])
def test_rollout_spectrum(n, placement, K):
    for when in NC.TIMES:
        accumulator_test("spectrum", n, placement, when, K)


def test_moments_negative_control_on_the_launch():
    samples, _ = NC.time_samples(65, 3, "nan", (63, 64), "middle")
    got, _, _ = run_accumulator("moments", samples, 3, 1, None, "control")
    st = M.new_state(65, 3, 1)
    for t in range(NC.T_ACC):
        st = M.accumulate(st, samples[t], t, NC.T_ACC, 2)
        if t == 1:
            lo, hi = st["lo"].copy(), st["hi"].copy()
        elif t in (3, 5):
            lo, hi = np.fmin(lo, M.sample(samples[t], t)), np.fmax(hi, M.sample(samples[t], t))
    M.same(got[3], st["lo"], "lo")
    M.same(got[4], st["hi"], "hi")
    assert np.isfinite(lo).all() and M.rejects(M.same, got[3], lo, "old fmin") and M.rejects(M.same, got[4], hi, "old fmax")


# ====================================================================== g4c_mesh_derived
def structured(n, dim, integer, seed=0):
    """A mesh of in-degree 6 given by its tables alone (senders i +- 1, 2, 3 mod n): (off, g, src).  The weight table is clean."""
    rng = np.random.default_rng(100 * n + dim + seed)
    off = (np.arange(n + 1) * 6).astype(np.int32)
    src = ((np.arange(n)[:, None] + np.array([1, 2, 3, n - 1, n - 2, n - 3])[None, :]) % n).reshape(-1).astype(np.int32)
    g = rng.integers(-4, 5, (6 * n, dim)).astype(np.float32) if integer else rng.standard_normal((6 * n, dim)).astype(np.float32)
    return off, g, src


DERIVED_NAMES = {(2, 1): ("grad:0",), (3, 1): ("grad:0",), (2, 3): ("div", "vort", "grad:2"), (3, 3): ("div", "vort")}
MAX_STEPS_D = 4


def column_reach(prog, off, src, dirty):
    """bool [n, nd]: the output elements whose stencil touches a dirty entry of a field their column names."""
    n = len(off) - 1
    out = np.zeros((n, len(prog)), bool)
    for c, col in enumerate(prog):
        for (f, _, _) in col:
            out[:, c] |= NC.receivers(off, src, dirty[:, f])
    return out


def run_derived(tables, prog, x, nf, what, t=1):
    off, g, src = tables
    n, nd = len(off) - 1, len(prog)
    cur, wc = rows_arena(n, nd, F32)
    snap, ws = rows_arena(MAX_STEPS_D * n, nd, F32)
    stats, wst = rows_arena(MAX_STEPS_D * nd, 3, F64)
    scratch, wsc = FP.flat_arena(int(ops.mesh_derived_scratch(n, nd, DEV).numel()), F64, device=DEV)
    step = torch.tensor([t, 0], dtype=I32, device=DEV)
    dx, doff, dg, dsrc = dev(x), dev(off), dev(g), dev(src)
    with FP.frozen(dx, doff, dg, dsrc, step, what=what):
        ops.mesh_derived(dx, doff, dg, dsrc, prog, cur, step=step, every=1, snap=snap.view(MAX_STEPS_D, n, nd),
                         stats=stats.view(MAX_STEPS_D, nd, 3), scratch=scratch, max_steps=MAX_STEPS_D, nf=nf)
        torch.cuda.synchronize(DEV)
    FP.assert_footprint(wc, cur, None, what + ", cur")
    FP.assert_footprint(ws, snap, range(t * n, (t + 1) * n), what + ", snap")
    FP.assert_footprint(wst, stats, range(t * nd, (t + 1) * nd), what + ", stats")
    FP.assert_footprint(wsc, scratch, None, what + ", scratch", inside=False)
    views = dict(cur=cur, snap=snap.view(MAX_STEPS_D, n, nd)[t], stats=stats.view(MAX_STEPS_D, nd, 3)[t])
    return views, dict(cur=wc, snap=ws, stats=wst)


def same_fp32(launch, got, ref, what, where=None):
    """An fp32 output against the restatement's numpy.float32 loop — which keeps subnormals: equal as integers, NaN = NaN.  The
    subnormal poison would show a launch that flushes them (none does: tests/NONFINITE_MEASURED.md), and a restatement that flushes is
    rejected wherever the result holds a subnormal (the negative control of that claim)."""
    NC.same_bits(got, ref, f"{launch}: {what}", where)
    r = np.asarray(ref)
    tiny = (r != 0) & (np.abs(r) < np.float32(2.0 ** -126))
    if tiny.any():
        SUBNORMAL_RESULTS[launch] = SUBNORMAL_RESULTS.get(launch, 0) + int(tiny.sum())
        assert NC.rejects(NC.same_bits, got, np.where(tiny, np.float32(0.0) * r, r).astype(np.float32), what), f"{launch}: {what}: a flushed result passed"


SUBNORMAL_RESULTS = {}          # launch -> how many subnormal results were compared (printed by the last test)


# (the large size tests the statistics' loop over more than 256 partials: one dimension)
@pytest.mark.parametrize("n,placement,dim", [(n, p, d) for n, p in NC.cases() for d in (2, 3) if n != NC.BIG or d == 2])
def test_mesh_derived(n, placement, dim):
    rows = NC.rows_of(n, placement)
    for nf in fields_of(n):
        prog = GR.program(DERIVED_NAMES[(dim, nf)], dim, nf)
        nd = len(prog)
        for integer in (True, False):
            tables = structured(n, dim, integer)
            off, g, src = tables
            x0 = NC.clean(np.random.default_rng(3 * n + nf), n, nf)
            clean, _ = run_derived(tables, prog, x0, nf, f"derived n {n} dim {dim} nf {nf} clean")
            NC.same_bits(clean["cur"], GR.derived32(x0, off, g, src, prog), "clean cur")
            for name in poisons_of(n):
                x, dirty = NC.poison(x0, name, rows, nf - 1)
                what = f"derived n {n} dim {dim} {placement} {name} nf {nf} g {'int' if integer else 'float'}"
                got, wholes = run_derived(tables, prog, x, nf, what)
                cur = GR.derived32(x, off, g, src, prog)
                same_fp32("g4c_mesh_derived", got["cur"], cur, what + ", cur")                                     # (a)
                NC.identical(got["snap"], got["cur"], what + ", snap")
                reach = column_reach(prog, off, src, dirty)
                NC.identical(got["cur"], clean["cur"], what + ", locality of cur", where=~reach)                         # (b)
                if integer:          # (integer weights: every clean term is an integer and the fp64 sums are exact in any order)
                    GR.same(got["stats"].cpu().numpy(), GR.stats64(got["cur"].cpu().numpy()), what + ", stats")
                    NC.identical(got["stats"], clean["stats"], what + ", locality of stats", where=~reach.any(0)[:, None])
                    if name == "nan":
                        assert bool(got["stats"].cpu()[reach.any(0)].isnan().all()), what + ": max_abs lost the NaN"
                else:          # (float weights: the maximum is exact in any order, and a sum is NaN / Inf exactly when the restatement's is)
                    s, w = got["stats"].cpu().numpy(), GR.stats64(got["cur"].cpu().numpy())
                    GR.same(s[:, 2], w[:, 2], what + ", max|q|")
                    assert np.array_equal(np.isnan(s), np.isnan(w)) and np.array_equal(np.isinf(s), np.isinf(w)), what + ", sums"
                    fin = np.isfinite(w[:, :2])
                    b = GR.stats_bound(np.where(np.isfinite(got["cur"].cpu().numpy()), got["cur"].cpu().numpy(), 0.0))
                    assert (np.abs(s[:, :2] - w[:, :2])[fin] <= b[fin]).all(), what + ", finite sums"
                _, wholes2 = run_derived(tables, prog, x, nf, what)                                                      # (d)
                wholes_identical(wholes, wholes2, what)


def test_derived_negative_control_on_the_launch():
    n, dim, nf = 257, 2, 3
    prog = GR.program(DERIVED_NAMES[(dim, nf)], dim, nf)
    tables = structured(n, dim, True)
    x, _ = NC.poison(NC.clean(np.random.default_rng(1), n, nf), "nan", (256,), nf - 1)
    got, _ = run_derived(tables, prog, x, nf, "control")
    q = got["cur"].cpu().numpy().astype(np.float64)
    old = GR.stats64(q)
    GR.same(got["stats"].cpu().numpy(), old, "as it should be")
    old[:, 2] = np.fmax.reduce(np.abs(q), axis=0)
    assert np.isfinite(old[:, 2]).all() and GR.rejects(GR.same, got["stats"].cpu().numpy(), old, "old fmax")


# ====================================================================== g4c_mesh_jet and the two stencil adjoints
import adjoint_op_ref as A                               # noqa: E402
import jet_ref as J                                      # noqa: E402
import sample_adjoint_ref as SA                          # noqa: E402
import sampler_ref as S                                  # noqa: E402

SMALL = [(n, p) for n, p in NC.cases() if n != NC.BIG]          # (no statistics kernel behind these launches: the four sizes)
JET_NAMES = {(2, 1): ("lap:0", "grad:0"), (3, 1): ("hess:0",), (2, 3): ("div", "vort", "lap:2", "hess:1"), (3, 3): ("div", "lap:2", "grad:1")}


def stencil_case(kind, dim, nf):
    """(program, table columns): the gradient's programs over `dim` weights per entry, the jet's over q_of(dim)."""
    if kind == "gradient":
        return GR.program(DERIVED_NAMES[(dim, nf)], dim, nf), dim
    return J.program(JET_NAMES[(dim, nf)], dim, nf), J.q_of(dim)


def run_jet(tables, prog, x, nf, what):
    off, c, src = tables
    n, nd = len(off) - 1, len(prog)
    out, whole = rows_arena(n, nd, F32)
    ins = [dev(x), dev(off), dev(c), dev(src)]
    with FP.frozen(*ins, what=what):
        got = ops.mesh_jet(ins[0], ins[1], ins[2], ins[3], prog, out, nf=nf)
        torch.cuda.synchronize(DEV)
    assert got is out
    FP.assert_footprint(whole, out, None, what)
    return out, whole


@pytest.mark.parametrize("n,placement,dim", [(n, p, d) for n, p in SMALL for d in (2, 3)])
def test_mesh_jet(n, placement, dim):
    rows = NC.rows_of(n, placement)
    for nf in NC.FIELDS:
        prog, width = stencil_case("jet", dim, nf)
        for integer in (True, False):
            tables = structured(n, width, integer, seed=1)
            off, c, src = tables
            x0 = NC.clean(np.random.default_rng(3 * n + nf), n, nf)
            clean, _ = run_jet(tables, prog, x0, nf, f"jet n {n} dim {dim} nf {nf} clean")
            for name in NC.POISONS:
                x, dirty = NC.poison(x0, name, rows, nf - 1)
                what = f"jet n {n} dim {dim} {placement} {name} nf {nf} c {'int' if integer else 'float'}"
                got, whole = run_jet(tables, prog, x, nf, what)
                same_fp32("g4c_mesh_jet", got, J.derived32(x, off, c, src, prog), what)                              # (a)
                NC.identical(got, clean, what + ", locality", where=~column_reach(prog, off, src, dirty))               # (b)
                _, whole2 = run_jet(tables, prog, x, nf, what)
                assert torch.equal(FP._int_view(whole), FP._int_view(whole2)), what + ": two runs differ in their bits"   # (d)


def adjoint_reach(prog, off, src, dirty, nf):
    """bool [n, nf]: gx[j, f] for j a dirty row's node or one of its senders and f a field of a dirty column."""
    out = np.zeros((len(off) - 1, nf), bool)
    for c, col in enumerate(prog):
        hit = NC.senders(off, src, dirty[:, c])
        for (f, _, _) in col:
            out[:, f] |= hit
    return out


def run_stencil_adjoint(kind, tables, prog, gy, nf, what):
    off, c, src = tables
    n = len(off) - 1
    out_off, out_perm = A.sender_csr(src, n)
    ins = [dev(gy), dev(off), dev(c), dev(out_off), dev(c[out_perm]), dev(A.dst_of(off)[out_perm])]
    gx, whole = rows_arena(n, nf, F32)
    fn = ops.mesh_derived_adjoint if kind == "gradient" else ops.mesh_jet_adjoint
    with FP.frozen(*ins, what=what):
        got = fn(ins[0], ins[1], ins[2], ins[3], ins[4], ins[5], prog, nf, gx)
        torch.cuda.synchronize(DEV)
    assert got is gx
    FP.assert_footprint(whole, gx, None, what)
    return gx, whole


def stencil_adjoint_test(kind, n, placement, dim):
    rows = NC.rows_of(n, placement)
    for nf in NC.FIELDS:
        prog, width = stencil_case(kind, dim, nf)
        nd = len(prog)
        for integer in (True, False):
            tables = structured(n, width, integer, seed=2)
            off, c, src = tables
            gy0 = NC.clean(np.random.default_rng(5 * n + nf), n, nd)
            clean, _ = run_stencil_adjoint(kind, tables, prog, gy0, nf, f"{kind} adjoint n {n} clean")
            for name in NC.POISONS:
                gy, dirty = NC.poison(gy0, name, rows, nd - 1)
                what = f"{kind} adjoint n {n} dim {dim} {placement} {name} nf {nf} table {'int' if integer else 'float'}"
                got, whole = run_stencil_adjoint(kind, tables, prog, gy, nf, what)
                same_fp32(f"g4c_mesh_{'derived' if kind == 'gradient' else 'jet'}_adjoint", got, A.adjoint32(gy, off, c, src, prog, nf), what)
                NC.identical(got, clean, what + ", locality", where=~adjoint_reach(prog, off, src, dirty, nf))
                _, whole2 = run_stencil_adjoint(kind, tables, prog, gy, nf, what)
                assert torch.equal(FP._int_view(whole), FP._int_view(whole2)), what + ": two runs differ in their bits"


@pytest.mark.parametrize("n,placement,dim", [(n, p, d) for n, p in SMALL for d in (2, 3)])
def test_mesh_derived_adjoint(n, placement, dim):
    stencil_adjoint_test("gradient", n, placement, dim)


@pytest.mark.parametrize("n,placement,dim", [(n, p, d) for n, p in SMALL for d in (2, 3)])
def test_mesh_jet_adjoint(n, placement, dim):
    stencil_adjoint_test("jet", n, placement, dim)


# ====================================================================== g4c_sample_points and its adjoint
POINTS, K_SAMPLE = 257, 6


def sample_tables(n, p, integer, seed=0):
    """(idx [P, k] int32 into the n nodes, coef [P, k] fp32): the weight table is clean."""
    rng = np.random.default_rng(1000 * n + p + seed)
    k = min(K_SAMPLE, n)          # (the launch refuses more neighbours than nodes)
    idx = rng.integers(0, n, (p, k)).astype(np.int32)
    coef = rng.integers(-4, 5, (p, k)).astype(np.float32) if integer else rng.standard_normal((p, k)).astype(np.float32)
    return idx, coef


def run_sample(x, idx, coef, what):
    p, nf = idx.shape[0], x.shape[1]
    cur, whole = rows_arena(p, nf, F32)
    ins = [dev(x), dev(idx.T), dev(coef.T)]
    with FP.frozen(*ins, what=what):
        ops.sample_points(ins[0], ins[1], ins[2], cur)
        torch.cuda.synchronize(DEV)
    FP.assert_footprint(whole, cur, None, what)
    return cur, whole


@pytest.mark.parametrize("n,placement", SMALL)
def test_sample_points(n, placement):
    rows = NC.rows_of(n, placement)
    for nf in NC.FIELDS:
        for integer in (True, False):
            idx, coef = sample_tables(n, POINTS, integer)
            x0 = NC.clean(np.random.default_rng(3 * n + nf), n, nf)
            clean, _ = run_sample(x0, idx, coef, f"sample n {n} nf {nf} clean")
            for name in NC.POISONS:
                x, dirty = NC.poison(x0, name, rows, nf - 1)
                what = f"sample n {n} {placement} {name} nf {nf} coef {'int' if integer else 'float'}"
                got, whole = run_sample(x, idx, coef, what)
                same_fp32("g4c_sample_points", got, S.apply32(x, idx, coef), what)                                 # (a)
                reach = np.stack([dirty[:, f][idx].any(1) for f in range(nf)], axis=1)          # the points whose neighbour set names a dirty node
                NC.identical(got, clean, what + ", locality", where=~reach)                                              # (b)
                _, whole2 = run_sample(x, idx, coef, what)
                assert torch.equal(FP._int_view(whole), FP._int_view(whole2)), what + ": two runs differ in their bits"   # (d)


def run_sample_adjoint(gy, tabs, n_nodes, what):
    gx, whole = rows_arena(n_nodes, gy.shape[1], F32)
    ins = [dev(gy)] + [dev(t) for t in tabs]
    with FP.frozen(*ins, what=what):
        ops.sample_points_adjoint(ins[0], ins[1], ins[2], ins[3], n_nodes, gx)
        torch.cuda.synchronize(DEV)
    FP.assert_footprint(whole, gx, None, what)
    return gx, whole


@pytest.mark.parametrize("n,placement", SMALL)
def test_sample_points_adjoint(n, placement):
    """`n` points (the placements are rows of gy) over 300 nodes."""
    rows, n_nodes = NC.rows_of(n, placement), 300
    for nf in NC.FIELDS:
        for integer in (True, False):
            idx, coef = sample_tables(n_nodes, n, integer, seed=1)
            tabs = SA.node_tables(np.ascontiguousarray(idx.T), np.ascontiguousarray(coef.T), n_nodes)
            gy0 = NC.clean(np.random.default_rng(5 * n + nf), n, nf)
            clean, _ = run_sample_adjoint(gy0, tabs, n_nodes, f"sample adjoint n {n} nf {nf} clean")
            for name in NC.POISONS:
                gy, dirty = NC.poison(gy0, name, rows, nf - 1)
                what = f"sample adjoint points {n} {placement} {name} nf {nf} coef {'int' if integer else 'float'}"
                got, whole = run_sample_adjoint(gy, tabs, n_nodes, what)
                same_fp32("g4c_sample_points_adjoint", got, SA.adjoint32(gy, *tabs), what)
                reach = np.zeros((n_nodes, nf), bool)
                for f in range(nf):
                    reach[np.unique(idx[dirty[:, f]]), f] = True          # the nodes the dirty points name
                NC.identical(got, clean, what + ", locality", where=~reach)
                _, whole2 = run_sample_adjoint(gy, tabs, n_nodes, what)
                assert torch.equal(FP._int_view(whole), FP._int_view(whole2)), what + ": two runs differ in their bits"


# ====================================================================== g4c_body_forces (forces and wall) and its adjoint
import forces_adjoint_ref as FA                          # noqa: E402
import test_gpu_body_forces as TBF                       # noqa: E402  (its cloud, launch and arenas: the graph and the operators of a case)


@pytest.mark.parametrize("counts", [(257,), (5, 257)], ids=lambda c: "-".join(map(str, c)))
def test_body_forces(counts):
    """The poison sits in the pressure column (flt_max: also in v) at wall items of the LAST body: item 0, items 63 / 64, an item of
    the fourth wave, item 256 — the stages of the body's tree sum."""
    c = TBF.cloud(counts)
    nb, nw, nf, steps, t = len(counts), sum(counts), TBF.NF, TBF.STEPS, 2
    items, boff = np.asarray(c["geo"]["items"]), np.asarray(c["geo"]["body_offsets"])
    off, src = c["tabs"]["off"], c["tabs"]["src"]
    base = c["target"].cpu().numpy()
    body_of = np.repeat(np.arange(nb), np.diff(boff))

    def run(x_np, viscous, what):
        x = dev(x_np)
        (st, st_w), (cur, cur_w), (wall, wall_w) = TBF.arenas(nb, nw)
        TBF.launch(c, x, viscous=viscous, t=t, x_step=nf, on_device=True, stats=st.view(steps, nb, 6), cur=cur.view(nb, 3), wall=wall.view(nw, 2))
        FP.assert_footprint(st_w, st, TBF.stats_rows(nb, t), what + ": stats")
        FP.assert_footprint(cur_w, cur, None, what + ": cur")
        FP.assert_footprint(wall_w, wall, None, what + ": wall")
        return dict(stats=st.view(steps, nb, 6)[t], cur=cur.view(nb, 3), wall=wall.view(nw, 2)), dict(stats=st_w, cur=cur_w, wall=wall_w)

    for viscous in (False, True):
        clean, _ = run(base, viscous, "forces clean")
        for placement, w_rows in NC.placements(257).items():
            node_rows = [int(items[boff[nb - 1] + w]) for w in w_rows]
            for name in NC.POISONS:
                cols, dirty = NC.poison(np.ascontiguousarray(base[:, nf * t:nf * (t + 1)]), name, node_rows, 2)
                x_np = base.copy()
                x_np[:, nf * t:nf * (t + 1)] = cols
                what = f"forces {counts} mu {'on' if viscous else 'off'} {placement} {name}"
                got, wholes = run(x_np, viscous, what)
                tree, _, _, rwall, _, _ = TBF.ref_of(c, torch.from_numpy(x_np), t, nf, viscous)
                same_fp32("g4c_body_forces", got["wall"], rwall, what + ": wall")                                  # (a)
                NC.same_values(got["stats"], tree, what + ": stats, the kernel's order")
                NC.same_bits(got["cur"], TBF.R.cur32(got["stats"].cpu().numpy()), what + ": cur")
                hit_p = dirty[items, 2]
                hit_v = NC.receivers(off, src, dirty[:, 0] | dirty[:, 1])[items] if viscous else np.zeros(nw, bool)
                NC.identical(got["wall"], clean["wall"], what + ": locality of wall", where=~np.stack([hit_p, hit_v], axis=1))   # (b)
                body_p = np.array([hit_p[body_of == b].any() for b in range(nb)])
                body_v = np.array([hit_v[body_of == b].any() for b in range(nb)])
                reach = np.stack([body_p, body_p, body_v, body_v, body_p, body_v], axis=1)          # Fp_x, Fp_y, Fv_x, Fv_y, Mp, Mv
                NC.identical(got["stats"], clean["stats"], what + ": locality of stats", where=~reach)
                NC.identical(got["cur"], clean["cur"], what + ": locality of cur", where=~(body_p | body_v)[:, None])
                if name == "nan":
                    assert bool(got["stats"].cpu()[nb - 1, [0, 1, 4]].isnan().all()) and bool(got["cur"].cpu()[nb - 1].isnan().all()), what
                    assert nb == 1 or bool(got["stats"].cpu()[0].isfinite().all()), what + ": the other body"
                _, wholes2 = run(x_np, viscous, what)                                                                    # (d)
                wholes_identical(wholes, wholes2, what)


def run_forces_adjoint(geo, tabs, off, g, n_nodes, nf, gF, gwall, what):
    cols = dict(pcol=2, ucol=0, vcol=1)
    c = dict(cols, mu=0.04, p_scale=2.5, u_scale=1.5, v_scale=0.75)
    d = {k: dev(v) for k, v in tabs.items()}
    ins = dict(gF=dev(gF), gwall=dev(gwall), area=dev(geo["area"]), unit=dev(geo["unit"]), arm=dev(geo["arm"]), g=dev(g), off=dev(off))
    gx, whole = rows_arena(n_nodes, nf, F32)
    with FP.frozen(*ins.values(), *d.values(), what=what):
        ops.body_forces_adjoint(ins["gF"], ins["gwall"], d["item_body"], ins["area"], ins["unit"], ins["arm"], d["own_off"], d["own_item"],
                                int(geo["n_bodies"]), nf, **c, g=ins["g"], off=ins["off"], in_off=d["in_off"], in_item=d["in_item"], in_g=d["in_g"],
                                out=gx)
        torch.cuda.synchronize(DEV)
    FP.assert_footprint(whole, gx, None, what)
    return gx, whole, dict(c, off=off, g=g)


@pytest.mark.parametrize("where", ["gF", "gwall"])
def test_body_forces_adjoint(where):
    n_nodes, n_items, nb, nf = 700, 620, 3, 3
    geo, off, src, g = FA.synthetic(n_nodes, n_items, nb)
    tabs = FA.node_tables(geo["items"], geo["body_offsets"], n_nodes, off, src, g)
    items, boff = np.asarray(geo["items"]), np.asarray(geo["body_offsets"])
    gF0, gw0 = FA.incoming(nb, n_items, seed=3)
    clean, _, ref_c = run_forces_adjoint(geo, tabs, off, g, n_nodes, nf, gF0, gw0, "forces adjoint clean")
    NC.same_bits(clean, FA.adjoint32(gF0, gw0, geo, tabs, n_nodes, nf, **ref_c), "clean")
    placements = {"first": (0,), "wave_edge": (63, 64), "wave4": (200,), "wg2": (256,), "last": (n_items - 1,)} if where == "gwall" else {"body": (1,)}
    for placement, rows in placements.items():
        for name in NC.POISONS:
            for col in ((0, 1) if where == "gwall" else (0, 3, 5)):
                gF, gw = gF0.copy(), gw0.copy()
                if where == "gwall":
                    gw, dirty = NC.poison(gw0, name, rows, col)
                    hit_items = dirty.any(1)
                else:
                    g32, dirty = NC.poison(gF0.astype(np.float32), name, rows, col)          # (the poison's values; clean entries keep their fp64)
                    gF[dirty] = g32[dirty].astype(np.float64)
                    hit_items = np.repeat(dirty.any(1), np.diff(boff))
                if name == "subnormal":          # both incoming gradients, so that nothing of O(1) is added to the subnormal terms
                    gF, gw = gF0 * float(NC.TINY), (gw0 * NC.TINY).astype(np.float32)
                    hit_items = np.ones(n_items, bool)
                what = f"forces adjoint {where} {placement} {name} col {col}"
                got, whole, _ = run_forces_adjoint(geo, tabs, off, g, n_nodes, nf, gF, gw, what)
                same_fp32("g4c_body_forces_adjoint", got, FA.adjoint32(gF, gw, geo, tabs, n_nodes, nf, **ref_c), what)
                wall_nodes = np.zeros(n_nodes, bool)
                wall_nodes[items[hit_items]] = True
                NC.identical(got, clean, what + ", locality", where=~NC.senders(off, src, wall_nodes)[:, None])          # the items' nodes and their senders
                _, whole2, _ = run_forces_adjoint(geo, tabs, off, g, n_nodes, nf, gF, gw, what)
                assert torch.equal(FP._int_view(whole), FP._int_view(whole2)), what + ": two runs differ in their bits"


# ====================================================================== g4c_tracer_advance
import test_gpu_tracers as TT                            # noqa: E402  (its particles, fields and guarded launch)


@pytest.mark.parametrize("dim", [2, 3])
def test_tracer_advance_with_a_nan_velocity(dim):
    """One node's velocity is NaN (or infinite): under Heun the particles whose neighbours include it get status 4 with q unchanged
    (include/g4c.h, step 5: a q* that is not finite); under Euler, which has no q*, their q' is stored as it is and counts as outside
    the box (steps 5 and 6: status 2).  Either way they stop at this step, and all the others keep the clean run's bits."""
    n, p, k, power, t = 1000, 257, 6, 2, TT.T_STEP
    pos = TT.R.cloud(n, dim)
    pos_d = dev(pos)
    grid = TT.S._bin_cloud(pos_d, k)
    cfg = TT.config(dim, True)
    w0, w1, x0, x1 = TT.fields(n, 5 + dim)
    q, status, stopped, release = TT.initial(TT.particles(pos, p, dim, grid["h"]))
    nearest = TT.S.knn_query_device(pos_d, q, k).cpu().numpy()
    for scheme in (_lib.TRACER_EULER, _lib.TRACER_HEUN):
        la = TT.Launch(grid, q, status, stopped, release)
        clean = [v.clone() for v in la.run(x0, x1, cfg, k, power, scheme, t, True, frozen_too=(w0, w1))]
        moved = (clean[1] == 1).cpu().numpy() & (release.cpu().numpy() <= t)          # moving after the clean step
        bad = int(nearest[np.nonzero(moved)[0][3], 0])          # the nearest node of a moving particle
        hit = torch.from_numpy((nearest == bad).any(1)).to(DEV)
        act = (release <= t) & (status < 2) & (clean[1] != 3)          # (a particle too far from every node stops before it interpolates)
        for name in ("nan", "+inf"):          # (an infinite velocity gives an infinite q*: the same status)
            w0p = w0.clone()
            w0p[bad, 2 + cfg["vcol"][0]] = float(name.replace("+", ""))
            runs = []
            for _ in range(2):
                lb = TT.Launch(grid, q, status, stopped, release)
                runs.append([v.clone() for v in lb.run(w0p[:, 2:7], x1, cfg, k, power, scheme, t, True, frozen_too=(w0p, w1))])
            got = runs[0]
            what = f"tracers dim {dim} scheme {scheme} {name}"
            stop = hit & act
            assert int(stop.sum()) >= 1 and int((~hit & act).sum()) >= 100, what
            assert bool((got[2][stop] == t).all()), what + ": stopped at step t"
            if scheme == _lib.TRACER_HEUN:          # step 5: a q* that is not finite is status 4, q unchanged
                assert bool((got[1][stop] == _lib.TRACER_NONFINITE).all()), what + ": status 4"
                assert torch.equal(got[0][stop].view(I32), q[stop].view(I32)), what + ": q of a stopped particle changed"
            else:          # Euler has no q*: steps 5 and 6 store q' = q + dt v0 as it is, and a position that is not finite is outside the box
                assert bool((got[1][stop] == _lib.TRACER_LEFT).all()), what + ": status 2"
                assert bool((~torch.isfinite(got[0][stop])).any(1).all()), what + ": q' of a particle carried by a NaN is not finite"
            keep = ~stop
            for j, nm in enumerate(("q", "status", "stopped")):
                a, b = got[j][keep], clean[j][keep]
                assert torch.equal(a.view(I32) if a.dtype == F32 else a, b.view(I32) if b.dtype == F32 else b), f"{what}: {nm} of the others"
            go = keep & act
            assert torch.equal(got[3][go].view(I32), clean[3][go].view(I32)), what + ": vel of the others"
            assert torch.equal(got[4][0].view(I32), got[0].view(I32)), what + ": the slot holds every particle's position"
            for a, b in zip(*runs):
                assert torch.equal(a.view(I32) if a.dtype == F32 else a, b.view(I32) if b.dtype == F32 else b), what + ": two runs"


# ====================================================================== g4c_snapshot_gram
import modes_ref as MR                                   # noqa: E402
import graphs4cfd_amd as gfd                             # noqa: E402


def test_snapshot_gram_with_a_nan_under_a_zero_weight():
    """0 * NaN is NaN: the plain fp64 loop says the row and the column of that snapshot are NaN, and so does the launch; `Modes.fit`
    refuses the matrix."""
    M_, N_, nf = 5, 300, 2
    rng = np.random.default_rng(9)
    x0 = NC.clean(rng, M_, N_ * nf)
    w = rng.integers(1, 4, N_ * nf).astype(np.float64)
    node = 123
    w[node * nf:(node + 1) * nf] = 0.0
    outs = {}
    for name in ("clean", "nan"):
        x = x0.copy()
        if name == "nan":
            x[2, node * nf] = np.nan
        a, dw = dev(x), dev(w)
        out, whole = FP.arena(M_, M_, F64, device=DEV)
        with FP.frozen(a, dw, what=name):
            ops.snapshot_gram(a, w=dw, out=out)
            torch.cuda.synchronize(DEV)
        FP.assert_footprint(whole, out, None, name)
        NC.same_values(out.contiguous(), MR.gram(x, w=w)[0], f"gram {name}")          # (small integers: the sums are exact in any order)
        outs[name] = out.cpu().numpy()
    hit = np.zeros((M_, M_), bool)
    hit[2, :] = hit[:, 2] = True
    assert np.isnan(outs["nan"][hit]).all() and np.isfinite(outs["clean"]).all()
    NC.identical(outs["nan"], outs["clean"], "gram, locality", where=~hit)
    nw = torch.ones(N_, dtype=F64)
    nw[node] = 0.0
    xs = torch.from_numpy(x0.reshape(M_, N_, nf).copy())
    xs[2, node, 0] = float("nan")
    with pytest.raises(ValueError, match="non-finite"):
        gfd.Modes(rank=2, node_weights=nw).fit(xs.to(DEV))


# ====================================================================== the module level, through the target
def test_evaluate_through_a_poisoned_target():
    """The prediction does not depend on the target: one NaN and one Inf in `graph.target` change `RolloutErrors` at exactly their step
    and field — mse / mae / max_abs NaN (Inf) there — and the error moments at exactly their node and field; every other entry, and
    the returned prediction, keep the clean evaluation's bits."""
    from graphs4cfd_amd import synthetic as SY
    n_out, n = 4, 2000
    g = SY.mus_graph(n, levels=2, seed=3).to(DEV)
    g.batch = torch.zeros(g.num_nodes, dtype=torch.long, device=DEV)
    torch.manual_seed(4)
    model = gfd.nn.NsTwoScaleGNN(arch=SY.mus_arch("NsTwoScaleGNN", 128), device=DEV)
    model.eval()
    nf = int(model.num_fields)
    target = torch.randn(n, nf * n_out, generator=torch.Generator().manual_seed(5))
    masked = (g.omega[:, 0] == 1).cpu()
    a, b = int(torch.nonzero(masked)[0]), int(torch.nonzero(~masked)[0])          # the NaN inside the Dirichlet mask, the Inf outside
    poisoned = target.clone()
    poisoned[a, nf * 1 + 0] = float("nan")          # step 1, field 0
    poisoned[b, nf * 2 + 2] = float("inf")          # step 2, field 2

    def evaluate(tgt):
        gg = g.clone()
        gg.target = tgt.to(DEV)
        return model.evaluate(gg, every=1, error_moments=True)

    clean, got, again = evaluate(target), evaluate(poisoned), evaluate(poisoned)
    assert torch.equal(got.snapshots.view(I32), clean.snapshots.view(I32)), "the prediction changed with the target"
    hit = torch.zeros(n_out, nf, dtype=torch.bool)
    hit[1, 0] = hit[2, 2] = True
    for name in ("mse", "mae", "max_abs"):
        v, c = getattr(got, name), getattr(clean, name)
        assert bool(v[1, 0].isnan()) and bool(v[2, 2] == float("inf")), f"{name}: {v}"
        NC.identical(v, c, name, where=~hit.numpy())
    assert bool(got.mae_masked[1, 0].isnan()) and bool(got.mae_masked[2, 2].isfinite()), "the Inf sits outside the mask"
    mm_hit = np.zeros((n_out, nf), bool)
    mm_hit[1, 0] = True
    NC.identical(got.mae_masked, clean.mae_masked, "mae_masked", where=~mm_hit)
    NC.identical(got.sums, clean.sums, "sums", where=~hit.numpy()[:, :, None])
    NC.identical(got.sums, again.sums, "two evaluations")
    em, ec = got.error_moments, clean.error_moments
    node_hit = np.zeros((n, nf), bool)
    node_hit[a, 0] = node_hit[b, 2] = True
    for name in ("pivot", "sum", "min", "max", "mean"):
        v, c = getattr(em, name), getattr(ec, name)
        NC.identical(v, c, f"error_moments.{name}", where=~node_hit)
    assert bool(em.min[a, 0].isnan()) and bool(em.max[a, 0].isnan()) and bool(em.mean[a, 0].isnan()), "min / max lost the NaN sample"
    assert bool(em.min[b, 2] == float("-inf")) and bool(em.max[b, 2].isfinite()) and bool(em.sum[b, 2] == float("-inf")), (em.min[b, 2], em.max[b, 2])
    pair_hit = np.zeros((n, nf * (nf + 1) // 2), bool)
    for p_, (f, h) in enumerate(M.pairs(nf)):
        pair_hit[a, p_] = 0 in (f, h)
        pair_hit[b, p_] = 2 in (f, h)
    NC.identical(em.sum2, ec.sum2, "error_moments.sum2", where=~pair_hit)
    NC.identical(em.sum2, again.error_moments.sum2, "two evaluations, sum2")


def test_zz_print_what_was_measured():
    """Not a check of its own: how many subnormal results each fp32 launch was held to (tests/NONFINITE_MEASURED.md; pytest -s)."""
    for k, v in sorted(SUBNORMAL_RESULTS.items()):
        print(f"MEASURED {k}: {v} subnormal results compared bit for bit, none flushed")
