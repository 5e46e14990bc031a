"""Host side of the rollout time statistics (no GPU): the restatement tests/moments_ref.py against its own definition, `RolloutMoments`
built from the sums the restatement produces against a two-pass evaluation in extended precision (numpy.longdouble, so that the
reference's own round-off does not consume the bound), and every argument error of `Rollout(moments=, error_moments=)`,
`ops.rollout_moments` and `g4c_rollout_moments` that can be raised without a device.

Bounds (n = count, d = sample - pivot, exact in fp64 for fp32 samples):
  |mean - ref| <= (n + 4) 2^-53 (|pivot| + sum|d| / n)
  |cov  - ref| <= 2 (n + 4) 2^-53 (sum|d_f d_g| / n + 2 mean|d_f| mean|d_g|)
The largest measured / allowed ratios are recorded in tests/MOMENTS_MEASURED.md."""
import ctypes as C
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import moments_ref as M                                        # noqa: E402
import graphs4cfd_amd as gfd                                   # noqa: E402
from graphs4cfd_amd import _lib, ops                           # noqa: E402
from graphs4cfd_amd.nn.model import Rollout, RolloutMoments    # noqa: E402

U64 = 2.0 ** -53
F32, F64, I32, I64 = torch.float32, torch.float64, torch.int32, torch.int64


def draws(kind, n, nf, steps, seed):
    rng = np.random.default_rng(seed)
    if kind == "int":
        return [rng.integers(-8, 9, (n, nf)).astype(np.float32) for _ in range(steps)]
    off = {"random": 0.0, "offset": 1e4}[kind]
    return [(rng.standard_normal((n, nf)) * np.array([1.0, 0.3, 2.0, 1.0, 0.1, 1.0, 5.0, 1.0])[:nf] + off).astype(np.float32)
            for _ in range(steps)]


def moments_of(st, stride):
    t = {k: torch.from_numpy(np.ascontiguousarray(st[k].T)) for k in M.NAMES}
    return RolloutMoments(M.count(st, stride), int(st["window"][0]), stride, t["pivot"], t["sum"], t["sum2"], t["lo"], t["hi"])


# ------------------------------------------------------------------ the restatement
def test_window_and_first_step():
    n, nf, steps = 5, 2, 8
    preds = draws("random", n, nf, steps + 1, 0)
    for start, stride in ((0, 1), (2, 1), (0, 3), (2, 3)):
        st = M.new_state(n, nf, start, fill=-7777.0)
        taken = []
        for t in range(steps + 1):
            new = M.accumulate(st, preds[t], t, steps, stride)
            if M.on_window(t, start, stride, steps):
                taken.append(t)
                assert int(new["window"][1]) == t
            else:
                M.same_state(new, st, f"off-window step {t}")
            st = new
        assert taken == list(range(start, steps, stride)) and M.count(st, stride) == len(taken)
        x = np.stack([preds[t].astype(np.float64).T for t in taken])
        M.same(st["pivot"], x[0], "pivot")
        M.same(st["lo"], x.min(0), "lo")
        M.same(st["hi"], x.max(0), "hi")
        # running through the origin again replaces the record
        M.same_state(M.accumulate(st, preds[start], start, steps, stride), M.accumulate(M.new_state(n, nf, start), preds[start], start, steps, stride))


def test_pair_order_of_sum2():
    """sum2's planes are the pairs (0,0), (0,1), ..., (0,nf-1), (1,1), ...; on small integers every sum is exact."""
    assert M.pairs(3) == [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    n, nf, steps = 7, 4, 6
    preds = draws("int", n, nf, steps, 1)
    st = M.run(preds, steps)
    d = np.stack([p.astype(np.float64) - preds[0].astype(np.float64) for p in preds])          # [steps, n, nf]
    for p, (f, g) in enumerate(M.pairs(nf)):
        M.same(st["sum2"][p], (d[:, :, f] * d[:, :, g]).sum(0), f"pair {p} = ({f}, {g})")
    mo = moments_of(st, 1)
    x = np.stack([p.astype(np.float64) for p in preds])
    xc = x - x.mean(0)
    want = np.einsum("tnf,tng->nfg", xc, xc) / steps
    assert np.abs(mo.cov.numpy() - want).max() < 1e-12
    # (a cov built from sums in another pair order is wrong where the fields differ)
    bad = moments_of(M.run(preds, steps), 1)
    bad.sum2 = bad.sum2[:, [M.pairs(nf, "pair-order").index(fg) for fg in M.pairs(nf)]]
    assert np.abs(bad.cov.numpy() - want).max() > 1e-3


def test_sub_takes_the_columns_of_the_step():
    n, nf, steps = 6, 3, 5
    preds = draws("random", n, nf, steps, 2)
    sub = np.random.default_rng(3).standard_normal((n, nf * steps + 2)).astype(np.float32)
    st = M.run(preds, steps, subs=sub)
    diffs = [(p.astype(np.float64) - sub[:, nf * t:nf * (t + 1)].astype(np.float64)).astype(np.float64) for t, p in enumerate(preds)]
    M.same(st["pivot"], diffs[0].T, "pivot")
    M.same(st["hi"], np.stack(diffs).max(0).T, "hi")


def test_negative_controls():
    n, nf, steps = 9, 3, 8
    preds = draws("offset", n, nf, steps, 4)
    sub = np.random.default_rng(5).standard_normal((n, nf * (steps + 1))).astype(np.float32)
    ref = M.new_state(n, nf, 1)
    for t in range(steps):
        ref = M.accumulate(ref, preds[t], t, steps, 2, sub)
    for wrong in M.WRONG:
        st = M.new_state(n, nf, 1)
        for t in range(steps):
            st = M.accumulate(st, preds[t], t, steps, 2, sub, wrong=wrong)
        assert M.rejects(M.same_state, st, ref, wrong), wrong


# ------------------------------------------------------------------ RolloutMoments against two passes in extended precision
def two_pass(samples):
    x = np.stack([np.asarray(s, dtype=np.float64) for s in samples]).astype(np.longdouble)          # [count, n, nf]
    mean = x.sum(0) / x.shape[0]
    xc = x - mean
    cov = np.einsum("tnf,tng->nfg", xc, xc) / x.shape[0]
    return mean, cov


CASES = [("random", 50, 3, 40, 0, 1), ("offset", 50, 3, 40, 0, 1), ("offset", 33, 3, 41, 2, 3), ("random", 20, 8, 30, 1, 2),
         ("offset", 20, 8, 30, 0, 1), ("offset", 10, 1, 600, 0, 1), ("random", 10, 2, 600, 5, 1)]


@pytest.mark.parametrize("kind,n,nf,steps,start,stride", CASES)
def test_mean_and_cov_within_the_bounds(kind, n, nf, steps, start, stride):
    preds = draws(kind, n, nf, steps, 10 + steps + nf)
    st = M.run(preds, steps, start, stride)
    mo = moments_of(st, stride)
    taken = list(range(start, steps, stride))
    cnt = len(taken)
    assert mo.count == cnt and mo.origin == start and mo.stride == stride
    x = [preds[t] for t in taken]
    mean_ref, cov_ref = two_pass(x)
    d = np.abs(np.stack([s.astype(np.float64) - x[0].astype(np.float64) for s in x]))                # |d|, [count, n, nf]
    mean_allow = (cnt + 4) * U64 * (np.abs(x[0].astype(np.float64)) + d.sum(0) / cnt)
    mean_err = np.abs(mo.mean.numpy().astype(np.longdouble) - mean_ref).astype(np.float64)
    cov_allow = 2 * (cnt + 4) * U64 * (np.einsum("tnf,tng->nfg", d, d) / cnt + 2 * np.einsum("nf,ng->nfg", d.mean(0), d.mean(0)))
    cov_err = np.abs(mo.cov.numpy().astype(np.longdouble) - cov_ref).astype(np.float64)
    r_mean = float((mean_err / np.maximum(mean_allow, 1e-300)).max())
    r_cov = float((cov_err / np.maximum(cov_allow, 1e-300)).max())
    print(f"  {kind} n {n} nf {nf} count {cnt}: measured / allowed  mean {r_mean:.3e}  cov {r_cov:.3e}")
    assert (mean_err <= mean_allow).all(), r_mean
    assert (cov_err <= cov_allow).all(), r_cov
    cov = mo.cov
    assert tuple(cov.shape) == (n, nf, nf) and torch.equal(cov, cov.transpose(1, 2))
    assert torch.equal(mo.var, torch.diagonal(cov, dim1=1, dim2=2)) and torch.equal(mo.std, mo.var.clamp_min(0).sqrt())
    assert bool((mo.std >= 0).all()) and bool((mo.min <= mo.mean + 1e-9).all()) and bool((mo.max >= mo.mean - 1e-9).all())


def test_the_pivot_is_what_keeps_an_offset_covariance():
    """The same sums without the shift (d = x) lose the covariance of data at 1e4 by orders of magnitude more than the bound."""
    kind, n, nf, steps = "offset", 50, 3, 40
    preds = draws(kind, n, nf, steps, 10 + steps + nf)
    st = M.new_state(n, nf, 0)
    for t in range(steps):
        st = M.accumulate(st, preds[t], t, steps, 1, wrong="no-pivot")
    st["pivot"][:] = 0.0
    _, cov_ref = two_pass(preds)
    err = np.abs(moments_of(st, 1).cov.numpy().astype(np.longdouble) - cov_ref).astype(np.float64).max()
    good = np.abs(moments_of(M.run(preds, steps), 1).cov.numpy().astype(np.longdouble) - cov_ref).astype(np.float64).max()
    assert err > 100 * good


def test_a_constant_field_has_zero_variance_and_a_clamped_std():
    n, nf, steps = 4, 2, 5
    preds = [np.full((n, nf), 1e4, dtype=np.float32) for _ in range(steps)]
    mo = moments_of(M.run(preds, steps), 1)
    assert bool((mo.var == 0).all()) and bool((mo.std == 0).all()) and bool((mo.mean == 1e4).all())
    mo.sum2 = mo.sum2 - 1e-12                      # round-off of the wrong sign: var < 0, std clamped
    assert bool((mo.var < 0).all()) and bool((mo.std == 0).all())


def test_count_zero_raises_on_the_derived_quantities():
    st = M.new_state(3, 2, 4)
    mo = moments_of(st, 2)
    assert mo.count == 0 and mo.fields == 2 and "count=0" in repr(mo)
    for name in ("mean", "cov", "var", "std"):
        with pytest.raises(RuntimeError, match="count == 0"):
            getattr(mo, name)
    assert tuple(mo.sum2.shape) == (3, 3) and mo.snapshots is None
    with pytest.raises(ValueError, match="sum2"):
        RolloutMoments(1, 0, 1, mo.pivot, mo.sum, mo.sum, mo.min, mo.max)


def test_exports():
    import graphs4cfd
    assert gfd.nn.RolloutMoments is RolloutMoments and graphs4cfd.nn.RolloutMoments is RolloutMoments
    e = gfd.nn.RolloutErrors(torch.zeros(2, 3, _lib.REC_NSTAT, dtype=F64), 10)
    assert e.moments is None and e.error_moments is None
    assert "g4c_rollout_moments" in _lib.EXPORTED_SYMBOLS


# ------------------------------------------------------------------ Rollout(moments=, error_moments=) argument errors
def host_graph(n=6, nf=3):
    return gfd.Graph(field=torch.zeros(n, nf), pos=torch.zeros(n, 2))


ROLLOUT_BAD = {
    "moments-float": (dict(moments=1.5), TypeError, "moments"),
    "moments-str": (dict(moments="all"), TypeError, "moments"),
    "moments-triple": (dict(moments=(0, 1, 2)), TypeError, "moments"),
    "moments-float-stride": (dict(moments=(0, 2.0)), TypeError, "moments"),
    "moments-bool-start": (dict(moments=(True, 1)), TypeError, "moments"),
    "moments-negative-start": (dict(moments=-1), ValueError, "moments"),
    "moments-negative-start-pair": (dict(moments=(-2, 1)), ValueError, "moments"),
    "moments-zero-stride": (dict(moments=(0, 0)), ValueError, "moments"),
    "moments-start-at-max": (dict(moments=7), ValueError, "moments"),
    "moments-start-past-max": (dict(moments=(9, 2)), ValueError, "moments"),
    "error_moments-float": (dict(error_moments=0.5, target=torch.zeros(6, 21)), TypeError, "error_moments"),
    "error_moments-zero-stride": (dict(error_moments=(1, 0), target=torch.zeros(6, 21)), ValueError, "error_moments"),
    "error_moments-start-at-max": (dict(error_moments=7, target=torch.zeros(6, 21)), ValueError, "error_moments"),
    "error_moments-without-target": (dict(error_moments=True), ValueError, "error_moments"),
}


@pytest.mark.parametrize("label", sorted(ROLLOUT_BAD))
def test_rollout_refuses_malformed_moments(label):
    kw, exc, word = ROLLOUT_BAD[label]
    with pytest.raises(exc) as info:
        Rollout(SimpleNamespace(num_fields=3), host_graph(), 7, **kw)
    assert type(info.value) is exc and word in str(info.value), f"{type(info.value).__name__}: {info.value}"
    assert "no CPU fallback" not in str(info.value)


def test_rollout_refuses_more_than_eight_fields():
    for kw in (dict(moments=True), dict(error_moments=(1, 2), target=torch.zeros(6, 63))):
        with pytest.raises(NotImplementedError, match="moments"):
            Rollout(SimpleNamespace(num_fields=9), host_graph(nf=9), 7, **kw)


@pytest.mark.parametrize("kw", [dict(moments=True), dict(moments=False), dict(moments=3), dict(moments=(6, 5)), dict(moments=[0, 2]),
                                dict(moments=(1, 2), error_moments=0, target=torch.zeros(6, 21))])
def test_rollout_with_wellformed_moments_stops_at_the_device_check(kw):
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Rollout(SimpleNamespace(num_fields=3), host_graph(), 7, **kw)


# ------------------------------------------------------------------ ops.rollout_moments argument errors
N, NF, STEPS = 6, 3, 7


def good():
    planes = torch.zeros(4 * NF + 6, N + 4, dtype=F64)[:, 2:N + 2]
    pivot, s, s2, lo, hi = planes.split((NF, NF, 6, NF, NF))
    return dict(pred=torch.zeros(N, NF), step=torch.zeros(2, dtype=I32), nf=NF, max_steps=STEPS, window=torch.zeros(2, dtype=I32),
                pivot=pivot, sum=s, sum2=s2, lo=lo, hi=hi, stride=2, sub=torch.zeros(N, NF * STEPS + 4)[:, 1:NF * STEPS + 2])


def z64(*shape):
    return torch.zeros(*shape, dtype=F64)


OPS_BAD = {
    "pred-f64": (dict(pred=z64(N, NF)), TypeError, "pred"),
    "pred-cols": (dict(pred=torch.zeros(N, NF + 1)), ValueError, "pred"),
    "pred-strided": (dict(pred=torch.zeros(N, 2 * NF)[:, :NF]), ValueError, "pred"),
    "step-i64": (dict(step=torch.zeros(2, dtype=I64)), TypeError, "step"),
    "step-short": (dict(step=torch.zeros(1, dtype=I32)), ValueError, "step"),
    "window-i64": (dict(window=torch.zeros(2, dtype=I64)), TypeError, "window"),
    "window-short": (dict(window=torch.zeros(1, dtype=I32)), ValueError, "window"),
    "max_steps-negative": (dict(max_steps=-1), ValueError, "max_steps"),
    "stride-zero": (dict(stride=0), ValueError, "stride"),
    "pivot-f32": (dict(pivot=torch.zeros(NF, N)), TypeError, "pivot"),
    "sum-nodes": (dict(sum=z64(NF, N + 1)), ValueError, "sum"),
    "sum2-planes": (dict(sum2=z64(NF, N)), ValueError, "sum2"),
    "lo-node-major": (dict(lo=z64(N, NF).t()), ValueError, "lo"),
    "hi-other-plane-stride": (dict(hi=z64(NF, N)), ValueError, "plane stride"),
    "sub-f64": (dict(sub=z64(N, NF * STEPS)), TypeError, "sub"),
    "sub-short": (dict(sub=torch.zeros(N, NF * STEPS - 1)), ValueError, "sub"),
    "sub-rows": (dict(sub=torch.zeros(N + 1, NF * STEPS)), ValueError, "sub"),
    "sub-colstride": (dict(sub=torch.zeros(NF * STEPS, N).t()), ValueError, "sub"),
}


@pytest.fixture
def library_must_not_load(monkeypatch):
    def load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", load)


@pytest.mark.parametrize("label", sorted(OPS_BAD))
def test_malformed_call_raises_before_the_library(label, library_must_not_load):
    patch, exc, word = OPS_BAD[label]
    with pytest.raises(exc) as info:
        ops.rollout_moments(**dict(good(), **patch))
    assert type(info.value) is exc and word in str(info.value), f"{type(info.value).__name__}: {info.value}"
    assert "no CPU fallback" not in str(info.value)


@pytest.mark.parametrize("patch", [{}, dict(sub=None), dict(sub=torch.zeros(N, NF * STEPS)), dict(stride=1)])
def test_wellformed_call_stops_at_the_device_check(patch):
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rollout_moments(**dict(good(), **patch))


def test_descriptor_matches_the_header_and_the_library_checks_it_before_any_launch():
    """The ctypes descriptor has the C struct's layout (LP64), and every G4C_EINVAL of g4c_rollout_moments comes back from the host
    checks — on a machine without a GPU too."""
    assert C.sizeof(_lib.g4c_rollout_moments_t) == 80
    lib = _lib.load()
    two = (C.c_int32 * 2)()
    one = C.addressof(two)           # (any non-null address: nothing is dereferenced before the checks)
    ok = dict(max_steps=7, stride=1, window=one, plane_ld=5, pivot=one, sum=one, sum2=one, lo=one, hi=one)

    def call(nf=3, n=5, pred=one, step=one, desc=True, **kw):
        m = _lib.g4c_rollout_moments_t(**dict(ok, **kw))
        return lib.g4c_rollout_moments(pred, nf, C.byref(m) if desc else None, step, n, None)

    for kw, word in ((dict(desc=False), "null"), (dict(step=None), "null"), (dict(window=None), "null"), (dict(pred=None), "null"),
                     (dict(pivot=None), "null"), (dict(sum=None), "null"), (dict(sum2=None), "null"), (dict(lo=None), "null"),
                     (dict(hi=None), "null"), (dict(stride=0), "stride"), (dict(stride=-3), "stride"),
                     (dict(sub=one, sub_ld=20), "sub_ld"), (dict(n=-1), "bad sizes"), (dict(nf=0), "bad sizes"),
                     (dict(max_steps=-1), "bad sizes"), (dict(plane_ld=4), "plane_ld")):
        assert call(**kw) == _lib.EINVAL, kw
        msg = lib.g4c_last_error().decode()
        assert "g4c_rollout_moments" in msg and word in msg, (kw, msg)
    assert call(nf=9) == _lib.EUNSUPPORTED and "g4c_rollout_moments" in lib.g4c_last_error().decode()
    # no nodes: nothing to launch, success without a device (null data pointers are fine then)
    assert call(n=0, pred=None, pivot=None, sum=None, sum2=None, lo=None, hi=None, plane_ld=0) == _lib.OK
