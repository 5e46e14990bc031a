"""Dense pairs for segments of any length (csrc/mlp_ws.hip, mlp_ws_any_kernel; routing: ops._set_agg / ops.DENSE_ANY, G4C_DENSE_ANY).

A row's arithmetic does not depend on the tile it sits in and a segment's rows are added in order from 0.f wherever a pair's end cuts
it, so EVERY comparison here is exact (torch.equal): the rows against the launch on tiles of whole segments (DENSE_ANY off), the
aggregate against that launch's and against ops.segment_reduce of the rows, the fused layer's v', e', heads and range-flag words against
the switched-off layer's.  G4C_WS_MAX_GRID (read by the launcher at every launch) caps the grid, so that a few thousand rows give
workgroups of 1, 2, 3 and 5 pairs — carries across several pairs — where 256 workgroups would get one pair each."""
import contextlib
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

import footprint as FP                               # noqa: E402
import test_gpu_fwd_ref as F                         # noqa: E402  (its case builders: net, message_blocks, table, csr_of)
import graphs4cfd_amd as gfd                         # noqa: E402
from graphs4cfd_amd import _lib, ops, plan           # noqa: E402
from graphs4cfd_amd import synthetic as S            # noqa: E402

DEV = F.DEV
H = 128
K_WS, K_WS_CERT = _lib.KERNEL_MLP_WS, _lib.KERNEL_MLP_WS_CERT


@pytest.fixture(autouse=True)
def _inference():
    with torch.no_grad():
        yield


@contextlib.contextmanager
def form(on, grid=None):
    """DENSE_ANY on / off, the grid capped at `grid` workgroups; both restored."""
    was, old = ops.DENSE_ANY, os.environ.get("G4C_WS_MAX_GRID")
    ops.DENSE_ANY = on
    if grid is not None:
        os.environ["G4C_WS_MAX_GRID"] = str(grid)
    try:
        yield
    finally:
        ops.DENSE_ANY = was
        if grid is not None:
            if old is None:
                del os.environ["G4C_WS_MAX_GRID"]
            else:
                os.environ["G4C_WS_MAX_GRID"] = old


def gen(seed):
    return torch.Generator().manual_seed(seed)


def grid_for(csr, pairs):
    """A grid cap at which the longest row range of `csr` has exactly `pairs` pairs."""
    for g in range(1, 257):
        rows, seg, p, _ = plan.row_ranges_host(csr.off.cpu().numpy(), g)
        if p == pairs:
            return g
        if p < pairs:
            break
    raise AssertionError(f"no grid gives {pairs} pairs on {csr.n} rows")


def sweep_degrees():
    """A segment cut at every row offset of a tile and of a pair: segments of 1 .. 8 rows in an order whose boundaries, over 61 blocks,
    walk through every residue modulo 64 (each block of segments sums to 65 rows, one more than a pair)."""
    block = [8, 7, 6, 5, 4, 3, 2, 1, 8, 7, 6, 5, 3]
    assert sum(block) == 65
    deg = torch.tensor(block * 61)
    cuts = set((torch.cumsum(deg, 0) % 64).tolist())
    assert cuts == set(range(64))
    return deg


def plain_cases():
    """(name, degrees, pairs per workgroup).  300 .. 4 000 rows."""
    long = torch.tensor([31, 32, 33, 63, 64, 65, 130, 1, 0, 64, 64, 2, 130, 5])
    return [("random 1..8", torch.randint(1, 9, (400,), generator=gen(1)), 3),
            ("random 1..8, one pair", torch.randint(1, 9, (300,), generator=gen(2)), 1),
            ("empty segments", F.ragged_degrees(500, 3, 9), 2),
            ("31 32 33 63 64 65 130", torch.cat([long, torch.randint(0, 9, (60,), generator=gen(4)), long.flip(0)]), 5),
            ("one segment over three pairs", torch.tensor([40, 130, 7, 3]), 3),
            ("last range shorter than a tile", torch.tensor([64] * 5 + [20]), 1),
            ("last pair shorter than a tile", torch.cat([torch.full((48,), 8), torch.tensor([5, 2])]), 7),
            ("cut sweep", sweep_degrees(), 5)]


def message_launch(nt, blks, csr, mean, keep_e, cert, expect_ranges, scale_flags=False):
    """One ops.mlp_forward with the fused aggregation in guard arenas -> (rows or None, aggregate, flag words)."""
    E, n = csr.n, csr.n_seg
    with F.switches("f16x3", 2) as lib:
        pk = nt.pack(blks, "f16x3")
        srcs = [b.source(cert) for b in blks]
        out, out_whole = FP.arena(E, H, torch.float32, device=DEV) if keep_e else (None, None)
        agg, agg_whole = FP.arena(n, H, torch.float32, device=DEV)
        with ops.RangeFlags(DEV) as flags:
            y = ops.mlp_forward(pk, srcs, E, agg=(csr, agg, mean), out=out, store_rows=keep_e)
            k, r = int(lib.g4c_mlp_last_kernel()), int(lib.g4c_mlp_last_row_ranges())
            words = flags.buf.clone()
        torch.cuda.synchronize()
        assert k == (K_WS_CERT if cert else K_WS), k
        assert (r > 0) == expect_ranges, (r, expect_ranges)
        if keep_e:
            FP.assert_footprint(out_whole, out, what="rows")
        FP.assert_footprint(agg_whole, agg, what="aggregate")
    return (y.clone() if keep_e else None), agg.clone(), words


@pytest.mark.parametrize("cert", [False, True], ids=["tracked", "certified"])
@pytest.mark.parametrize("layers", [3, 2])
def test_message_launch_with_fused_aggregation(layers, cert):
    nt = F.net(H, (H,) * layers, 700 + layers, True, "ln" if cert else "default")
    for i, (name, deg, pairs) in enumerate(plain_cases()):
        csr = F.csr_of(deg)
        assert 300 <= csr.n <= 4000 or name.startswith("one segment"), (name, csr.n)
        grid = grid_for(csr, pairs)
        if name == "last range shorter than a tile":
            wg_rows = csr.row_ranges(grid)[0].cpu()
            assert grid == 6 and int(wg_rows[-1] - wg_rows[-2]) == 20
        blks, _ = F.message_blocks(csr.n, csr.n_seg, "C", 710 + i)
        with form(False, grid):
            # today's path: tiles of whole segments (segments longer than a tile: the plain launch and the separate reduction)
            rows_off, agg_off, words_off = message_launch(nt, blks, csr, bool(i % 2), True, cert, False)
        ref = ops.segment_reduce(rows_off, csr, bool(i % 2))
        assert torch.equal(agg_off, ref), name
        for keep_e in (True, False):
            with form(True, grid):
                assert csr.row_ranges(grid)[2] == pairs
                rows_on, agg_on, words_on = message_launch(nt, blks, csr, bool(i % 2), keep_e, cert, True)
            what = f"{name}, {pairs} pairs per workgroup, keep_e={keep_e}"
            if keep_e:
                assert torch.equal(rows_on, rows_off), what
            assert torch.equal(agg_on, agg_off), what
            assert torch.equal(agg_on, ref), what
            assert torch.equal(words_on, words_off), what


def test_message_launch_sum_and_mean_on_every_pattern():
    """(the loop above alternates mean and sum over the patterns: here the other one of each)"""
    nt = F.net(H, (H, H, H), 720)
    for i, (name, deg, pairs) in enumerate(plain_cases()):
        csr = F.csr_of(deg)
        grid = grid_for(csr, pairs)
        blks, _ = F.message_blocks(csr.n, csr.n_seg, "C", 730 + i)
        mean = not bool(i % 2)
        with form(False, grid):
            rows_off, agg_off, _ = message_launch(nt, blks, csr, mean, True, False, False)
        with form(True, grid):
            rows_on, agg_on, _ = message_launch(nt, blks, csr, mean, True, False, True)
        assert torch.equal(rows_on, rows_off) and torch.equal(agg_on, agg_off), name
        assert torch.equal(agg_on, ops.segment_reduce(rows_off, csr, mean)), name


def test_a_clipped_value_sets_the_same_flag_word():
    nt = F.net(H, (H, H, H), 740)
    csr = F.csr_of(torch.randint(1, 9, (300,), generator=gen(5)))
    blks, _ = F.message_blocks(csr.n, csr.n_seg, "C", 741)
    blks[0].x = blks[0].x * 3e4
    grid = grid_for(csr, 2)
    with form(False, grid):
        _, _, words_off = message_launch(nt, blks, csr, True, True, False, False)
    with form(True, grid):
        _, _, words_on = message_launch(nt, blks, csr, True, True, False, True)
    assert int(words_off.sum()) >= 1 and torch.equal(words_on, words_off)


# ---------------------------------------------------------------------------------------------------------------- the fused MP layer
def layer_launch(msg, upd, blks, v, csr, mean, heads, cert, expect_ranges):
    E, n = csr.n, csr.n_seg
    with F.switches("f16x3", 2) as lib:
        pm, pu = msg.pack(blks, "f16x3"), upd.pack([F.Blk(v), F.Blk(v)], "f16x3", heads=True)
        srcs = [b.source(cert) for b in blks]
        arenas = {name: FP.arena(rows, H, torch.float32, device=DEV) for name, rows in
                  [("e'", E), ("agg", n), ("v'", n)] + ([("head0", n), ("head1", n)] if heads else [])}
        head_outs = [arenas["head0"][0], arenas["head1"][0]] if heads else None
        with FP.frozen(v, csr.off, *[b.x for b in blks], what="fused layer"), ops.RangeFlags(DEV) as flags:
            ops.mp_layer_forward(pm, srcs, E, csr, mean, pu, v, _lib.ACT_SELU, head_outs=head_outs, v_out=arenas["v'"][0],
                                 v_bound=float(v.abs().max()) if cert else None, e_out=arenas["e'"][0], agg_out=arenas["agg"][0])
            k, r = int(lib.g4c_mlp_last_kernel()), int(lib.g4c_mlp_last_row_ranges())
            words = flags.buf.clone()
        torch.cuda.synchronize()
        assert k == (K_WS_CERT if cert else K_WS) and (r > 0) == expect_ranges, (k, r)
        for name, (view, whole) in arenas.items():
            FP.assert_footprint(whole, view, what=name)          # the write footprint is clean
    return {name: view.clone() for name, (view, _) in arenas.items()}, words


@pytest.mark.parametrize("cert", [False, True], ids=["tracked", "certified"])
@pytest.mark.parametrize("layers", [3, 2])
def test_fused_layer(layers, cert):
    msg = F.net(H, (H,) * layers, 750 + layers, True, "ln" if cert else "default")
    upd = F.net(2 * H, (H,) * layers, 760 + layers, True, "ln" if cert else "default", n_heads=2)
    # 2 048 .. 6 000 edges over 400 .. 1 200 targets, in-degrees 1 .. 8
    for i, (n, pairs) in enumerate([(460, 1), (800, 3), (1200, 5)]):
        deg = torch.randint(1, 9, (n,), generator=gen(770 + i))
        csr = F.csr_of(deg)
        assert 2048 <= csr.n <= 6000 and csr.uniform_deg == 0
        grid = grid_for(csr, pairs)
        blks, _ = F.message_blocks(csr.n, n, "C", 780 + i)
        v = F.table(n, H, 790 + i)
        for heads in (False, True):
            with form(False, grid):
                off, words_off = layer_launch(msg, upd, blks, v, csr, bool(i % 2), heads, cert, False)
            with form(True, grid):
                on, words_on = layer_launch(msg, upd, blks, v, csr, bool(i % 2), heads, cert, True)
            for name in off:
                assert torch.equal(on[name], off[name]), f"{name}: {n} targets, {pairs} pairs per workgroup, heads={heads}"
            assert torch.equal(words_on, words_off)
            assert torch.equal(on["agg"], ops.segment_reduce(off["e'"], csr, bool(i % 2)))


# ---------------------------------------------------------------------------------------------------------------- model level
class Recorder:
    """g4c_mlp_run through a stand-in that notes (rows, with aggregation, row ranges of the launch) of every call."""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        return getattr(self._lib, name)

    def g4c_mlp_run(self, mlp, srcs, n_src, n_rows, io, stream):
        rc = self._lib.g4c_mlp_run(mlp, srcs, n_src, n_rows, io, stream)
        self.calls.append((int(n_rows), bool(io._obj.agg), bool(io._obj.upd), int(self._lib.g4c_mlp_last_row_ranges())))
        return rc


def test_three_scale_model_forward(monkeypatch):
    g = S.mus_graph(3000, levels=3, seed=21).to(DEV)
    g.batch = torch.zeros(g.num_nodes, dtype=torch.long, device=DEV)
    torch.manual_seed(22)
    model = gfd.nn.NsThreeScaleGNN(arch=S.mus_arch("NsThreeScaleGNN", 128), device=DEV)
    model.eval()
    E1 = int(g.edge_index.size(1))
    f0 = g.field.clone()

    def forward(on):
        g.field = f0.clone()
        with form(on):
            rec = Recorder(_lib.load())
            monkeypatch.setattr(_lib, "_lib", rec)
            try:
                out = model.solve(g.clone(), 1).clone()
            finally:
                monkeypatch.undo()
        return out, rec.calls

    off, calls_off = forward(False)
    on, calls_on = forward(True)
    assert torch.equal(on, off)
    assert [c[:3] for c in calls_on] == [c[:3] for c in calls_off]          # the same launches
    assert all(r == 0 for _, _, _, r in calls_off)
    level1 = [c for c in calls_on if c[0] == E1]
    assert level1 and all(r == 0 for _, _, _, r in level1), level1          # uniform in-degree: DENSE / tiles, untouched
    fused_coarse = [c for c in calls_on if c[2] and c[0] != E1]
    assert fused_coarse and all(r > 0 for _, _, _, r in fused_coarse), calls_on          # every fused coarse layer took the row-range form
    assert all(r == 0 for _, agg, _, r in calls_on if not agg)
