"""Argument checks of ops.rollout_advance_record on CPU tensors, in the pattern of test_ops_args.py: every malformed call raises the
stated exception (TypeError for a dtype, ValueError for a shape or a contradiction, the message naming the argument) before the
library is loaded, and the same call well-formed stops at require_hip's "no CPU fallback" RuntimeError.  No call here can reach a
kernel: every tensor lives on the host."""
import pytest
import torch

from graphs4cfd_amd import _lib, ops

F32, F64, I32, I64, U8 = torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8
N, NF, STEPS, P = 6, 3, 7, 4


def f(*shape):
    return torch.zeros(*shape, dtype=F32)


def good():
    return dict(field=f(N, 7), pred=f(N, NF), step=torch.zeros(2, dtype=I32), nf=NF, max_steps=STEPS,
                snap=f(3, N, NF), every=2, probe_rows=torch.zeros(P, dtype=I32), probe_out=f(STEPS, P, NF),
                target=f(N, NF * STEPS + 4)[:, 1:NF * STEPS + 2], mask=torch.zeros(N, dtype=torch.bool),
                stats=torch.zeros(STEPS, NF, _lib.REC_NSTAT, dtype=F64), scratch=torch.zeros(64, dtype=F64))


BAD = {
    "field-f64": (dict(field=f(N, 7).double()), TypeError, "field"),
    "field-strided": (dict(field=f(N, 8)[:, :7]), ValueError, "field"),
    "field-narrow": (dict(field=f(N, 2)), ValueError, "field"),
    "pred-f64": (dict(pred=f(N, NF).double()), TypeError, "pred"),
    "pred-rows": (dict(pred=f(N - 1, NF)), ValueError, "pred"),
    "pred-cols": (dict(pred=f(N, NF - 1)), ValueError, "pred"),
    "step-i64": (dict(step=torch.zeros(2, dtype=I64)), TypeError, "step"),
    "step-short": (dict(step=torch.zeros(1, dtype=I32)), ValueError, "step"),
    "max_steps-negative": (dict(max_steps=-1), ValueError, "max_steps"),
    "every-negative": (dict(every=-1), ValueError, "every"),
    "every-without-snap": (dict(snap=None), ValueError, "snap"),
    "snap-without-every": (dict(every=0), ValueError, "snap"),
    "snap-f64": (dict(snap=f(3, N, NF).double()), TypeError, "snap"),
    "snap-nodes": (dict(snap=f(3, N + 1, NF)), ValueError, "snap"),
    "snap-fields": (dict(snap=f(3, N, NF + 1)), ValueError, "snap"),
    "snap-2d": (dict(snap=f(N, 3 * NF)), ValueError, "snap"),
    "snap-strided": (dict(snap=f(3, N, 2 * NF)[:, :, :NF]), ValueError, "snap"),
    "probe_rows-i64": (dict(probe_rows=torch.zeros(P, dtype=I64)), TypeError, "probe_rows"),
    "probe_rows-2d": (dict(probe_rows=torch.zeros(P, 1, dtype=I32)), ValueError, "probe_rows"),
    "probe_rows-strided": (dict(probe_rows=torch.zeros(2 * P, dtype=I32)[::2]), ValueError, "probe_rows"),
    "probe_rows-alone": (dict(probe_out=None), ValueError, "probe_out"),
    "probe_out-alone": (dict(probe_rows=None), ValueError, "probe_rows"),
    "probe_out-f64": (dict(probe_out=f(STEPS, P, NF).double()), TypeError, "probe_out"),
    "probe_out-steps": (dict(probe_out=f(STEPS - 1, P, NF)), ValueError, "probe_out"),
    "probe_out-probes": (dict(probe_out=f(STEPS, P + 1, NF)), ValueError, "probe_out"),
    "probe_out-fields": (dict(probe_out=f(STEPS, P, NF + 1)), ValueError, "probe_out"),
    "target-f64": (dict(target=f(N, NF * STEPS).double()), TypeError, "target"),
    "target-rows": (dict(target=f(N + 1, NF * STEPS)), ValueError, "target"),
    "target-short": (dict(target=f(N, NF * STEPS - 1)), ValueError, "target"),
    "target-1d": (dict(target=f(N * NF * STEPS)), ValueError, "target"),
    "target-colstride": (dict(target=f(NF * STEPS, N).t()), ValueError, "target"),
    "mask-i32": (dict(mask=torch.zeros(N, dtype=I32)), TypeError, "mask"),
    "mask-short": (dict(mask=torch.zeros(N - 1, dtype=U8)), ValueError, "mask"),
    "mask-2d": (dict(mask=torch.zeros(N, 1, dtype=U8)), ValueError, "mask"),
    "mask-without-target": (dict(target=None, stats=None, scratch=None), ValueError, "mask"),
    "stats-without-target": (dict(target=None, mask=None, scratch=None), ValueError, "stats"),
    "scratch-without-target": (dict(target=None, mask=None, stats=None), ValueError, "scratch"),
    "target-without-stats": (dict(stats=None), ValueError, "stats"),
    "target-without-scratch": (dict(scratch=None), ValueError, "scratch"),
    "stats-f32": (dict(stats=f(STEPS, NF, _lib.REC_NSTAT)), TypeError, "stats"),
    "stats-steps": (dict(stats=torch.zeros(STEPS + 1, NF, _lib.REC_NSTAT, dtype=F64)), ValueError, "stats"),
    "stats-fields": (dict(stats=torch.zeros(STEPS, NF + 1, _lib.REC_NSTAT, dtype=F64)), ValueError, "stats"),
    "stats-nstat": (dict(stats=torch.zeros(STEPS, NF, _lib.REC_NSTAT - 1, dtype=F64)), ValueError, "stats"),
    "scratch-f32": (dict(scratch=f(64)), TypeError, "scratch"),
    "scratch-2d": (dict(scratch=torch.zeros(8, 8, dtype=F64)), ValueError, "scratch"),
}

GOOD = {
    "all-records": {},
    "mask-u8": dict(mask=torch.zeros(N, dtype=U8)),
    "no-mask": dict(mask=None),
    "snapshots-only": dict(probe_rows=None, probe_out=None, target=None, mask=None, stats=None, scratch=None),
    "no-record": dict(snap=None, every=0, probe_rows=None, probe_out=None, target=None, mask=None, stats=None, scratch=None),
    "no-slot": dict(snap=f(0, N, NF), every=9),
    "no-probe": dict(probe_rows=torch.zeros(0, dtype=I32), probe_out=f(STEPS, 0, NF)),
    "target-dense": dict(target=f(N, NF * STEPS)),
}


@pytest.fixture
def library_must_not_load(monkeypatch):
    def load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", load)


@pytest.mark.parametrize("label", sorted(BAD))
def test_malformed_call_raises_before_the_library(label, library_must_not_load):
    patch, exc, word = BAD[label]
    kw = dict(good(), **patch)
    assert all(not t.is_cuda for t in kw.values() if torch.is_tensor(t))          # (nothing here may reach a kernel)
    with pytest.raises(exc) as info:
        ops.rollout_advance_record(**kw)
    assert type(info.value) is exc, f"{type(info.value).__name__}: {info.value}"
    assert word in str(info.value), str(info.value)
    assert "no CPU fallback" not in str(info.value)


@pytest.mark.parametrize("label", sorted(GOOD))
def test_wellformed_call_stops_at_the_device_check(label):
    kw = dict(good(), **GOOD[label])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rollout_advance_record(**kw)


def test_descriptor_matches_the_header():
    """The ctypes descriptor has the C struct's layout (LP64: 4-byte counts padded in front of pointers), and the library rejects
    contradictory descriptors with G4C_EINVAL before any HIP call — on a machine without a GPU too."""
    import ctypes as C
    assert C.sizeof(_lib.g4c_rollout_rec_t) == 88
    lib = _lib.load()
    step = (C.c_int32 * 2)()

    def call(nf=3, field_cols=3, **kw):
        rec = _lib.g4c_rollout_rec_t(**kw)
        return lib.g4c_rollout_advance_record(None, field_cols, None, nf, C.byref(rec), C.addressof(step), 0, None)

    one = C.addressof(step)          # (any non-null address: nothing is dereferenced before the checks)
    for kw, word in ((dict(every=-1), "every"), (dict(every=0, snap=one), "snapshot"), (dict(n_probe=2), "probe_rows"),
                     (dict(n_probe=0, probe_rows=one), "probe_rows"), (dict(mask=one), "mask"),
                     (dict(max_steps=7, target=one, target_ld=20, stats=one, scratch=one), "target_ld"),
                     (dict(max_steps=7, target=one, target_ld=21, scratch=one), "stats"),
                     (dict(max_steps=7, target=one, target_ld=21, stats=one), "scratch")):
        assert call(**kw) == _lib.EINVAL, kw
        assert word in lib.g4c_last_error().decode(), (kw, lib.g4c_last_error().decode())
    assert call(nf=9, field_cols=9, max_steps=1, target=one, target_ld=9, stats=one, scratch=one) == _lib.EUNSUPPORTED
    assert lib.g4c_rollout_record_scratch_doubles(1000, 9) == _lib.EUNSUPPORTED
    assert lib.g4c_rollout_record_scratch_doubles(-1, 3) == _lib.EINVAL
    assert lib.g4c_rollout_record_scratch_doubles(0, 3) == lib.g4c_rollout_record_scratch_doubles(256, 3) > 0
