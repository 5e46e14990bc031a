"""Where the launches of csrc/train_ops.hip write, and whether they stay inside the scratch their size functions promise
(tests/footprint.py).  They are called through the ctypes entry points, as autograd.py calls them, so that the test owns every buffer:
outputs and scratch sit in guard arenas, inputs are frozen bit for bit.  Values are tests/test_gpu_train_ref.py's business; here only
the footprint and the finiteness of what a launch owns are asserted.

Row counts: 1, odd counts, and one past each kernel's rows per workgroup (g4c_train_gather / g4c_act_grad: 256 threads over
width / 4 or width columns — 8 rows of 128 columns on the vector path, 6 whole rows of 37 on the scalar one; g4c_layernorm_grad: 4 rows
per iteration, 64 per workgroup before a second one is launched; g4c_segment_broadcast: 4 segments; g4c_colsum: 128 rows per partial).
The scratch contracts take their row counts from the size functions themselves: the largest count with one partial, the smallest with
two, one below and one at the cap, and one well past it.  g4c_rollout_record_scratch_doubles and g4c_mesh_derived_scratch_doubles get
the same treatment through ops.rollout_advance_record / ops.mesh_derived, which take the caller's scratch."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

import footprint as FP                               # noqa: E402
from graphs4cfd_amd import _lib, ops                 # noqa: E402

DEV = torch.device("cuda", 0)
F32, BF16, F64, I32 = torch.float32, torch.bfloat16, torch.float64, torch.int32
H = 128
SELU, TANH = _lib.ACT_SELU, _lib.ACT_TANH
# (width, columns left of the window, columns right of it, columns left of the source window): the vector path — 16-byte aligned windows,
# leading dimensions that are multiples of 4 — and the scalar one — odd everything
VEC, SCALAR = (H, 8, 8, 4), (37, 5, 3, 3)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(rows, cols, seed, dtype=F32):
    return torch.randn(rows, cols, generator=gen(seed)).to(DEV).to(dtype)


def big(rows, cols, seed, dtype=F32):
    """N(0, 1) rows drawn on the device (the cap cases: several hundred thousand rows)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(rows, cols, generator=g, device=DEV).to(dtype)


def arena(rows, cols, dtype=F32, **kw):
    return FP.arena(rows, cols, dtype, device=DEV, **kw)


def flat(n, dtype=F32):
    return FP.flat_arena(n, dtype, device=DEV)


def stream():
    return _lib.stream_handle(DEV)


def ok(rc):
    assert rc == _lib.OK, _lib.load().g4c_last_error().decode()
    torch.cuda.synchronize()


def check(what, *arenas):
    """(whole, view, written rows or None, inside) per arena."""
    for name, whole, view, written, inside in arenas:
        FP.assert_footprint(whole, view, written_rows=written, what=f"{what}: {name}", inside=inside)
        if inside and written is None:
            assert bool(torch.isfinite(view.double()).all()), f"{what}: {name} holds a non-finite value"


def boundaries(partials, cap):
    """Row counts from a size function's own formula (`partials`: rows -> workgroups, monotone): the largest with one partial, the
    smallest with two, one below the cap, the smallest at the cap, one well past it."""
    def smallest(p):
        lo, hi = 1, 1 << 28
        while lo < hi:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if partials(mid) >= p else (mid + 1, hi)
        return lo
    two, at = smallest(2), smallest(cap)
    ns = [two - 1, two, at - 1, at, 5 * at // 2]
    assert [partials(n) for n in ns] == [1, 2, cap - 1, cap, cap] and partials(1 << 28) == cap, (ns, cap)
    return ns


# ====================================================================== g4c_train_gather
@pytest.mark.parametrize("accumulate", [0, 1], ids=["store", "accumulate"])
@pytest.mark.parametrize("indexed", [False, True], ids=["direct", "indexed"])
@pytest.mark.parametrize("path", [VEC, SCALAR], ids=["vec", "scalar"])
def test_train_gather(path, indexed, accumulate):
    """The window [dcol0, dcol0 + width) of a wider dst, rows [0, n): nothing left or right of it, nothing below row n."""
    lib = _lib.load()
    width, col0, pad, scol0 = path
    for n in (1, 5, 6, 7, 8, 9, 33):
        n_src = max(n // 2, 1) if indexed else n
        src = randn(n_src, scol0 + width + 5 - (scol0 + width + 5) % 4 + (0 if path is VEC else 1), 10 + n)
        idx = torch.randint(0, n_src, (n,), generator=gen(11 + n)).to(DEV, I32) if indexed else None
        view, whole = arena(n, width, col0=col0, pad_cols=pad)
        if accumulate:          # (the launch adds into what the window holds: numbers, not the pattern)
            view.copy_(randn(n, width, 12 + n))
        dst = view.data_ptr() - 4 * col0          # the wider tensor's row 0: the launch is told dcol0
        assert (path is VEC) == (dst % 16 == 0 and whole.size(1) % 4 == 0 and src.size(1) % 4 == 0)
        what = f"train_gather width={width} n={n} indexed={indexed} accumulate={accumulate}"
        with FP.frozen(src, idx, what=what):
            ok(lib.g4c_train_gather(src.data_ptr(), int(src.size(1)), scol0, _lib.ptr(idx), SELU, n % 2, dst, int(whole.size(1)), col0, width, n,
                                    accumulate, stream()))
            check(what, ("dst", whole, view, None, True))


# ====================================================================== g4c_act_grad / g4c_act_grad_ref16
@pytest.mark.parametrize("ref16", [False, True], ids=["ref32", "ref16"])
@pytest.mark.parametrize("path", [VEC, SCALAR], ids=["vec", "scalar"])
def test_act_grad(path, ref16):
    lib = _lib.load()
    width, col0, pad, _ = path
    fn = lib.g4c_act_grad_ref16 if ref16 else lib.g4c_act_grad
    for i, n in enumerate((1, 5, 6, 7, 8, 9, 33)):
        dy = randn(n, width + (8 if path is VEC else 4), 20 + n)
        ref = randn(n, width + (8 if path is VEC else 2), 21 + n, BF16 if ref16 else F32)
        view, whole = arena(n, width, col0=col0, pad_cols=pad)          # dz_ld > width
        assert (path is VEC) == (view.data_ptr() % 16 == 0 and whole.size(1) % 4 == 0)
        what = f"act_grad width={width} n={n} ref16={ref16}"
        with FP.frozen(dy, ref, what=what):
            ok(fn(dy.data_ptr(), int(dy.size(1)), ref.data_ptr(), int(ref.size(1)), i % 2, (SELU, TANH)[i % 2], view.data_ptr(), int(whole.size(1)),
                  width, n, stream()))
            check(what, ("dz", whole, view, None, True))


# ====================================================================== g4c_layernorm_grad / _z16 and its partials
def ln_grad(lib, z16, n, width, seed, what):
    z = (big if n > 10000 else randn)(n, width + 8, seed, BF16 if z16 else F32)
    dy = (big if n > 10000 else randn)(n, width + 4, seed + 1)
    gamma = 1.0 + 0.1 * randn(1, width, seed + 2).reshape(-1)
    dz, dz_whole = arena(n, width, col0=8 if width % 4 == 0 else 5, pad_cols=8 if width % 4 == 0 else 3)
    n_part = int(lib.g4c_layernorm_grad_partials(n))
    part, part_whole = flat(n_part * 2 * width)
    fn = lib.g4c_layernorm_grad_z16 if z16 else lib.g4c_layernorm_grad
    with FP.frozen(z, dy, gamma, what=what):
        ok(fn(z.data_ptr(), int(z.size(1)), gamma.data_ptr(), dy.data_ptr(), int(dy.size(1)), dz.data_ptr(), int(dz_whole.size(1)), part.data_ptr(),
              width, n, 1e-5, stream()))
        # every workgroup writes its whole partial row [dgamma | dbeta]: the scratch is owned in full
        check(what, ("dz", dz_whole, dz, None, True), ("partials", part_whole, part, None, True))


@pytest.mark.parametrize("z16", [False, True], ids=["z32", "z16"])
@pytest.mark.parametrize("width", [H, 37])
def test_layernorm_grad(width, z16):
    lib = _lib.load()
    for n in (1, 3, 4, 5, 63, 64, 65, 129):
        ln_grad(lib, z16, n, width, 30 + n, f"layernorm_grad width={width} n={n} z16={z16}")


@pytest.mark.parametrize("z16", [False, True], ids=["z32", "z16"])
def test_layernorm_grad_partials_contract(z16):
    lib = _lib.load()
    for n in boundaries(lambda n: int(lib.g4c_layernorm_grad_partials(n)), 1024):
        ln_grad(lib, z16, n, H, 40, f"layernorm_grad partials n={n} z16={z16}")


# ====================================================================== g4c_segment_broadcast
@pytest.mark.parametrize("mean", [0, 1], ids=["sum", "mean"])
@pytest.mark.parametrize("through", ["direct", "perm", "perm-drops-rows"])
@pytest.mark.parametrize("path", [VEC, SCALAR], ids=["w128", "w37"])
def test_segment_broadcast(path, through, mean):
    """Every row of a segment receives the segment's row; the rows of no segment — behind the last segment, or not named by a
    permutation that drops rows — are the wrapper's to zero: the launch must not write them."""
    lib = _lib.load()
    width, col0, pad, _ = path
    for n_seg in (1, 3, 4, 5, 9, 23):
        deg = torch.randint(0, 5, (n_seg,), generator=gen(50 + n_seg))
        deg[n_seg // 2] = 3
        n_kept = int(deg.sum())
        off = torch.cat([torch.zeros(1, dtype=torch.int64), deg.cumsum(0)]).to(DEV, I32)
        n_src = n_kept + (0 if through == "perm" else 3)
        perm = None if through == "direct" else torch.randperm(n_src, generator=gen(51 + n_seg))[:n_kept].to(DEV, I32)
        dout = randn(n_seg, width + 4, 52 + n_seg)
        view, whole = arena(n_src, width, col0=col0, pad_cols=pad)
        what = f"segment_broadcast width={width} n_seg={n_seg} {through} mean={mean}"
        with FP.frozen(dout, off, perm, what=what):
            ok(lib.g4c_segment_broadcast(dout.data_ptr(), int(dout.size(1)), off.data_ptr(), _lib.ptr(perm), n_seg, width, mean, view.data_ptr(),
                                         int(whole.size(1)), stream()))
            owned = torch.arange(n_kept) if perm is None else perm.long().cpu()
            check(what, ("dsrc", whole, view, owned, True))
            assert bool(torch.isfinite(view[owned.to(DEV)]).all())


# ====================================================================== g4c_colsum and its partials
def colsum(lib, n, width, seed, what):
    x = (big if n > 10000 else randn)(n, width + 3, seed)
    scratch, s_whole = flat(int(lib.g4c_colsum_partials(n)) * width)
    out, o_whole = flat(width)
    with FP.frozen(x, what=what):
        ok(lib.g4c_colsum(x.data_ptr(), int(x.size(1)), width, n, scratch.data_ptr(), out.data_ptr(), stream()))
        # (every partial row is written in full: the scratch is owned in full)
        check(what, ("scratch", s_whole, scratch, None, True), ("out", o_whole, out, None, True))


@pytest.mark.parametrize("width", [H, 37, 300])
def test_colsum(width):
    lib = _lib.load()
    for n in (1, 2, 127, 128, 129, 257, 1001):
        colsum(lib, n, width, 60 + n, f"colsum width={width} n={n}")


def test_colsum_partials_contract():
    lib = _lib.load()
    for n in boundaries(lambda n: int(lib.g4c_colsum_partials(n)), 2048):
        colsum(lib, n, 40, 61, f"colsum partials n={n}")


# ====================================================================== g4c_weight_grad* and g4c_weight_grad_scratch_floats
@pytest.mark.parametrize("entry", ["g4c_weight_grad", "g4c_weight_grad_bf16", "g4c_weight_grad_bf16_a16"])
def test_weight_grad_scratch_contract(entry):
    """The scratch is exactly g4c_weight_grad_scratch_floats(n_rows) floats (the partial tiles of both reduction stages): the guard behind
    it must hold, and so must the arena around `out` = 128 * 128 + 128 floats, of which the last 128 are not owned without a bias."""
    lib = _lib.load()
    fn = getattr(lib, entry)
    rows = [1, 33] + boundaries(lambda n: int(lib.g4c_weight_grad_partials(n)), 512)
    for n in rows:
        g = (big if n > 10000 else randn)(n, H + 8, 70)[:, 4:4 + H]          # 128-column windows of wider tensors: g_ld = a_ld = 136
        a = (big if n > 10000 else randn)(n, H + 8, 71, BF16 if entry.endswith("a16") else F32)[:, 8:8 + H]
        assert g.data_ptr() % 16 == 0 and a.data_ptr() % 16 == 0
        n_scratch = int(lib.g4c_weight_grad_scratch_floats(n))
        G = int(lib.g4c_weight_grad_partials(n))
        assert n_scratch == (G + (G + 15) // 16) * (H * H + H)
        for with_bias in (1, 0):
            scratch, s_whole = flat(n_scratch)
            out, o_whole = flat(H * H + H)
            what = f"{entry} n={n} with_bias={with_bias}"
            with FP.frozen(g, a, what=what):
                ok(fn(g.data_ptr(), int(g.stride(0)), a.data_ptr(), int(a.stride(0)), n, scratch.data_ptr(), out.data_ptr(), with_bias, stream()))
                own = torch.ones(1, H * H + H, dtype=torch.bool)
                own[0, H * H:] = bool(with_bias)
                # (without a bias the partial tiles' last 128 floats are never written: the scratch is checked from outside only)
                check(what, ("scratch", s_whole, scratch, None, bool(with_bias)), ("out", o_whole, out, own, True))
                assert bool(torch.isfinite(out[:H * H + (H if with_bias else 0)]).all())


# ====================================================================== the rollout launches' scratch
NF, MAX_STEPS = 3, 2


def test_rollout_record_scratch_contract():
    lib = _lib.load()
    nstat = _lib.REC_NSTAT
    for n in [1, 255] + boundaries(lambda n: (int(lib.g4c_rollout_record_scratch_doubles(n, NF)) - 8) // (NF * nstat), 1024):
        field, pred, target = big(n, NF + 2, 80), big(n, NF, 81), big(n, NF * MAX_STEPS + 1, 82)
        step = torch.zeros(2, dtype=I32, device=DEV)
        need = int(lib.g4c_rollout_record_scratch_doubles(n, NF))
        scratch, s_whole = flat(need, F64)
        stats, st_whole = flat(MAX_STEPS * NF * nstat, F64)
        what = f"rollout_advance_record n={n}"
        with FP.frozen(pred, target, what=what):
            ops.rollout_advance_record(field, pred, step, NF, MAX_STEPS, target=target, stats=stats.view(MAX_STEPS, NF, nstat), scratch=scratch)
            torch.cuda.synchronize()
            # scratch: [0] the step, [1, 8) unused, then one set of partials per workgroup; stats: row t = 0 only
            own_s = torch.ones(1, need, dtype=torch.bool)
            own_s[0, 1:8] = False
            own_t = torch.zeros(1, MAX_STEPS * NF * nstat, dtype=torch.bool)
            own_t[0, :NF * nstat] = True
            check(what, ("scratch", s_whole, scratch, own_s, True), ("stats", st_whole, stats, own_t, True))
        assert step.tolist() == [1, 0] and bool(torch.isfinite(stats[:NF * nstat]).all())


def test_mesh_derived_scratch_contract():
    lib = _lib.load()
    nstat, nd = _lib.DERIVED_NSTAT, 2
    program = [[(0, 0, 1.0)], [(1, 0, 1.0), (0, 1, -1.0)]]
    for n in [1, 255] + boundaries(lambda n: (int(lib.g4c_mesh_derived_scratch_doubles(n, nd)) - 8) // (nd * nstat), 1024):
        x = big(n, NF, 90)
        off = (2 * torch.arange(n + 1)).to(DEV, I32)          # two in-edges per node
        g = big(2 * n, 2, 91)
        src = torch.randint(0, n, (2 * n,), generator=gen(92)).to(DEV, I32)
        step = torch.zeros(2, dtype=I32, device=DEV)
        cur, c_whole = arena(n, nd, col0=0, pad_cols=0)          # (contiguous rows: the wrapper asks for a contiguous [N, nd])
        need = int(lib.g4c_mesh_derived_scratch_doubles(n, nd))
        scratch, s_whole = flat(need, F64)
        stats, st_whole = flat(MAX_STEPS * nd * nstat, F64)
        what = f"mesh_derived n={n}"
        with FP.frozen(x, off, g, src, step, what=what):
            ops.mesh_derived(x, off, g, src, program, cur, step=step, stats=stats.view(MAX_STEPS, nd, nstat), scratch=scratch, max_steps=MAX_STEPS)
            torch.cuda.synchronize()
            own_s = torch.ones(1, need, dtype=torch.bool)
            own_s[0, 1:8] = False
            own_t = torch.zeros(1, MAX_STEPS * nd * nstat, dtype=torch.bool)
            own_t[0, :nd * nstat] = True
            check(what, ("cur", c_whole, cur, None, True), ("scratch", s_whole, scratch, own_s, True), ("stats", st_whole, stats, own_t, True))


# ====================================================================== the check itself, on a real launch
def test_the_check_rejects_a_correct_launch_against_a_smaller_scratch():
    """Nothing perturbs a launch: g4c_colsum gets the scratch its size function promises and passes; the CHECK is then told that the
    scratch is one partial row shorter, and must name that row's first float as written behind the scratch."""
    import re
    lib = _lib.load()
    n, width = 129, 40
    assert int(lib.g4c_colsum_partials(n)) == 2
    x = randn(n, width, 100)
    scratch, s_whole = flat(2 * width)
    out, o_whole = flat(width)
    ok(lib.g4c_colsum(x.data_ptr(), width, width, n, scratch.data_ptr(), out.data_ptr(), stream()))
    check("control", ("scratch", s_whole, scratch, None, True), ("out", o_whole, out, None, True))
    with pytest.raises(AssertionError, match=re.escape(f"{width} element(s) written outside what the launch owns, the first at (row 0, column {width})") + ".*right of"):
        FP.assert_footprint(s_whole, scratch[:width], what="control")
    with pytest.raises(AssertionError, match=re.escape("1 element(s) written outside what the launch owns, the first at (row 0, column -1)") + ".*left of"):
        FP.assert_footprint(o_whole, out[1:], what="control")
