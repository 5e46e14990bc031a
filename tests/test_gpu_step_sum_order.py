"""The order of the step-record core's sums (csrc/step_record.h), pinned bit for bit against tests/step_sum_ref.sum_order for the two
launches that the integrals' and the forces' tests do not cover: the record's error statistics (g4c_rollout_advance_record) and the
norms of g4c_mesh_derived.

Every term the device adds is exact in fp64, so only the ORDER of the additions can change a bit:
  * record: pred and target are fp32 in [1, 2), so d = (double)y − (double)t is a multiple of 2⁻²³ below 1 in magnitude, d·d has at most
    46 significant bits and t·t at most 48 — a contracted multiply-add rounds exactly as the separate operations do;
  * derived: the reference's input is the device's own `cur`, and q·q of an fp32 q has at most 48 significant bits.
The maxima are free of order and compared with ==.  n = 257 is two workgroups, 1500 is six with a ragged last one, 262 444 is one past
the cap of 1024 workgroups (some threads take two rows, and the second launch's threads take four partials each)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

import gradient_ref as GR                                # noqa: E402
import step_sum_ref as SR                                # noqa: E402
from graphs4cfd_amd import _lib, ops                     # noqa: E402

DEV = torch.device("cuda", 0)
NODES = (257, 1500, 262_444)
REC_MAX, DERIVED_MAX = 2, 2          # G4C_REC_MAX_ABS_ERR, G4C_DERIVED_MAX_ABS (include/g4c.h)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_bits(got, want, is_max, what):
    """got, want [sets, nstat] fp64: the sums bit for bit, the maxima equal."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    sums = ~is_max
    bad = got.view(np.int64)[:, sums] != want.view(np.int64)[:, sums]
    assert not bad.any(), f"{what}: sums differ at {np.argwhere(bad).tolist()}: got {got[:, sums][bad]!r}, want {want[:, sums][bad]!r}"
    assert (got[:, is_max] == want[:, is_max]).all(), f"{what}: maxima {got[:, is_max]!r} != {want[:, is_max]!r}"


@pytest.mark.parametrize("nf", [1, 3])
@pytest.mark.parametrize("n", NODES)
def test_record_statistics_are_summed_in_the_core_order(n, nf):
    nstat = _lib.REC_NSTAT
    rng = np.random.default_rng(100 * n + nf)
    pred = (1.0 + rng.random((n, nf))).astype(np.float32)
    target = (1.0 + rng.random((n, nf))).astype(np.float32)
    mask = rng.random(n) < 0.3
    field = torch.zeros((n, nf), dtype=torch.float32, device=DEV)
    step = torch.zeros(2, dtype=torch.int32, device=DEV)
    stats = torch.full((1, nf, nstat), -7777.0, dtype=torch.float64, device=DEV)
    ops.rollout_advance_record(field, dev(pred), step, nf, 1, target=dev(target), mask=dev(mask), stats=stats,
                               scratch=ops.rollout_record_scratch(n, nf, DEV))
    y, tg = pred.astype(np.float64), target.astype(np.float64)
    d = y - tg
    ad = np.abs(d)
    # [n, nf, nstat] in the order of the enum: Σd², Σ|d|, max|d|, Σt, Σt², Σ_masked|d|
    T = np.stack([d * d, ad, ad, tg, tg * tg, np.where(mask[:, None], ad, 0.0)], axis=2).reshape(n, nf * nstat)
    is_max = np.arange(nf * nstat) % nstat == REC_MAX
    want = SR.sum_order(T, np.ones(n, bool), is_max).reshape(nf, nstat)
    assert step.tolist() == [1, 0]
    same_bits(stats[0].cpu().numpy(), want, is_max[:nstat], f"record n {n} nf {nf}")


@pytest.mark.parametrize("names", [("div",), ("div", "grad:0")], ids=["nd1", "nd3"])
@pytest.mark.parametrize("n", NODES)
def test_derived_norms_are_summed_in_the_core_order(n, names):
    nstat = _lib.DERIVED_NSTAT
    rng = np.random.default_rng(100 * n + len(names))
    # a mesh of uniform in-degree 6 given by its tables alone (no geometry)
    off = (np.arange(n + 1) * 6).astype(np.int32)
    src = ((np.arange(n)[:, None] + np.array([1, 2, 3, n - 1, n - 2, n - 3])[None, :]) % n).reshape(-1).astype(np.int32)
    g = rng.standard_normal((6 * n, 2)).astype(np.float32)
    x = rng.standard_normal((n, 2)).astype(np.float32)
    prog = GR.program(names, 2, 2, None, None)
    nd = len(prog)
    assert nd == {1: 1, 2: 3}[len(names)]
    cur = torch.empty((n, nd), dtype=torch.float32, device=DEV)
    step = torch.zeros(2, dtype=torch.int32, device=DEV)
    stats = torch.full((1, nd, nstat), -7777.0, dtype=torch.float64, device=DEV)
    ops.mesh_derived(dev(x), dev(off), dev(g), dev(src), prog, cur, step=step, stats=stats, scratch=ops.mesh_derived_scratch(n, nd, DEV),
                     max_steps=1, nf=2)
    q = cur.cpu().numpy().astype(np.float64)
    aq = np.abs(q)
    T = np.stack([q * q, aq, aq], axis=2).reshape(n, nd * nstat)          # Σq², Σ|q|, max|q|
    is_max = np.arange(nd * nstat) % nstat == DERIVED_MAX
    want = SR.sum_order(T, np.ones(n, bool), is_max).reshape(nd, nstat)
    same_bits(stats[0].cpu().numpy(), want, is_max[:nstat], f"derived n {n} nd {nd}")
