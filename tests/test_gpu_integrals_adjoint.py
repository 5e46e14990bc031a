"""g4c_weighted_integrals_adjoint (csrc/control_volumes.hip) through ops.weighted_integrals_adjoint against
tests/integrals_adjoint_ref.py: gx EQUAL — bit for bit, compared as integers — to the numpy restatement of the device's loop, written
into columns 0 .. nz − 1 of its rows and nowhere else (a guard arena), every input untouched; rows of zero weight and rows of a group
outside [0, G) are +0 whatever they hold; a NaN in g or in a column of x poisons exactly the outputs that depend on it; two runs agree."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

import integrals_adjoint_ref as A                                      # noqa: E402
from footprint import arena, assert_footprint, frozen                  # noqa: E402
from graphs4cfd_amd import _lib, ops                                   # noqa: E402

DEV = torch.device("cuda", 0)
CASES = dict(A.cases())


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def launch(case):
    """(gx as numpy float32 [N, nz], its arena)."""
    n, nz = case["x"].shape[0], case["nz"]
    xd, sd, wd, gd, qd = dev(case["x"]), dev(case["sub"]), dev(case["w"]), dev(case["g"]), dev(case["group"])
    gx, whole = arena(n, nz, torch.float32, guard_rows=8, col0=1 if case["gx_pad"] else 0, pad_cols=case["gx_pad"], device=DEV)
    with frozen(xd, sd, wd, gd, qd, what="weighted_integrals_adjoint"):
        out = ops.weighted_integrals_adjoint(xd, wd, case["entries"], gd, nz=nz, sub=sd, x_step=case["x_step"], sub_step=case["sub_step"],
                                             t=case["t"], group=qd, out=gx)
        torch.cuda.synchronize()
    assert out is gx
    assert_footprint(whole, gx, what="gx")
    return gx.cpu().numpy(), whole


def want(case):
    acc, _ = A.adjoint64(case["x"], case["w"], case["entries"], case["g"], case["sub"], case["x_step"], case["sub_step"], case["t"],
                         case["group"], case["nz"])
    return A.cast(acc)


def same_bits(got, ref):
    return np.array_equal(np.ascontiguousarray(got).view(np.int32), np.ascontiguousarray(ref).view(np.int32))


@pytest.mark.parametrize("name", list(CASES))
def test_bits_against_the_restatement(name):
    case = CASES[name]
    got, _ = launch(case)
    ref = want(case)
    differ = np.nonzero(got.view(np.int32) != ref.view(np.int32))
    assert differ[0].size == 0, (name, differ[0][:4], differ[1][:4], got[differ][:4], ref[differ][:4])
    dead = case["w"] == 0.0
    if case["group"] is not None:
        dead |= (case["group"] < 0) | (case["group"] >= case["g"].shape[0])
    assert not got[dead].view(np.int32).any()          # +0: the sign bit clear, whatever the row holds
    named = {c for e in case["entries"] for c in e if c >= 0}
    for c in set(range(case["nz"])) - named:
        assert not got[:, c].view(np.int32).any()      # a column no entry names


def test_without_out_and_two_runs_agree():
    case = CASES["nz5"]
    args = (dev(case["x"]), dev(case["w"]), case["entries"], dev(case["g"]))
    kw = dict(nz=case["nz"], sub=dev(case["sub"]), x_step=case["x_step"], sub_step=case["sub_step"], t=case["t"], group=dev(case["group"]))
    a = ops.weighted_integrals_adjoint(*args, **kw)
    b = ops.weighted_integrals_adjoint(*args, **kw)
    assert a.shape == (257, 5) and a.dtype == torch.float32 and a.is_contiguous()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert same_bits(a.cpu().numpy(), want(case))


def test_a_nan_poisons_exactly_the_outputs_that_depend_on_it():
    base = CASES["n257"]
    clean, _ = launch(base)
    entries, nz, G = base["entries"], base["nz"], base["g"].shape[0]
    live = np.nonzero((base["w"] != 0.0) & (base["group"] >= 0) & (base["group"] < G))[0]
    # a NaN in g[q][e]: the columns entry e names, in the rows of group q
    q, e = 1, 2
    case = dict(base, g=base["g"].copy())
    case["g"][q, e] = np.nan
    got, _ = launch(case)
    hit = np.zeros_like(clean, dtype=bool)
    rows = live[base["group"][live] == q]
    for c in entries[e]:
        if c >= 0:
            hit[rows, c] = True
    assert hit.any() and np.isnan(got[hit]).all()
    assert same_bits(got[~hit], clean[~hit])
    assert same_bits(got, want(case))
    # a NaN in column k of one row of x: in that row, the columns c that have an entry pairing c with k
    row, k = int(live[5]), 2
    case = dict(base, x=base["x"].copy())
    case["x"][row, base["x_step"] * base["t"] + k] = np.nan
    got, _ = launch(case)
    hit = np.zeros_like(clean, dtype=bool)
    for a, b in entries:
        if b == k and a >= 0:
            hit[row, a] = True
        if a == k and b >= 0:
            hit[row, b] = True
    assert hit.any() and np.isnan(got[hit]).all()
    assert same_bits(got[~hit], clean[~hit])


def test_no_rows_and_refusals():
    g = torch.zeros((1, 2), dtype=torch.float64, device=DEV)
    out = ops.weighted_integrals_adjoint(torch.zeros((0, 3), device=DEV), torch.zeros(0, dtype=torch.float64, device=DEV), [(0, 1), (2, -1)], g)
    assert tuple(out.shape) == (0, 3)
    x, w = torch.zeros((5, 3), device=DEV), torch.ones(5, dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError, match="^entries:"):
        ops.weighted_integrals_adjoint(x, w, [(0, 3)], g[:, :1].contiguous())
    with pytest.raises(ValueError, match="^g:"):
        ops.weighted_integrals_adjoint(x, w, [(0, 1)], g)
    with pytest.raises(ValueError, match="^g:"):
        ops.weighted_integrals_adjoint(x, w, [(0, 1), (1, 1)], torch.zeros((2, 2), dtype=torch.float64, device=DEV))
    with pytest.raises(ValueError, match="^group:"):
        ops.weighted_integrals_adjoint(x, w, [(0, 1), (1, 1)], g, group=torch.zeros(5, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="^x:"):
        ops.weighted_integrals_adjoint(x, w, [(0, 1), (1, 1)], g, x_step=3, t=1)          # the columns of step 1 are not there
    with pytest.raises(ValueError, match="^out:"):
        ops.weighted_integrals_adjoint(x, w, [(0, 1), (1, 1)], g, out=torch.zeros((5, 4), device=DEV))
    # the library's own checks (a descriptor that bypasses the wrapper): refused before any launch
    import ctypes as C
    lib = _lib.load()
    prog = ops.integral_program([(0, 1)], 3)
    gx = torch.zeros((5, 3), device=DEV)
    for field, value, text in (("t_host", 1, "t_host"), ("gx_ld", 2, "gx_ld"), ("n_groups", 0, "n_groups"), ("x_ld", 2, "x_ld")):
        kw = dict(x=_lib.ptr(x), x_ld=3, x_step=0, sub=None, sub_ld=0, sub_step=0, nz=3, w=_lib.ptr(w), g=_lib.ptr(g), n_groups=1, group=None,
                  t_host=0, max_steps=1, gx=_lib.ptr(gx), gx_ld=3)
        kw[field] = value
        wa = _lib.g4c_weighted_integrals_adjoint_t(**kw)
        assert lib.g4c_weighted_integrals_adjoint(C.byref(wa), C.byref(prog), 5, None) == _lib.EINVAL
        assert text in lib.g4c_last_error().decode()
