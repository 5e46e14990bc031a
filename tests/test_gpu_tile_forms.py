"""The tile forms of mlp_bx6_kernel's launch shapes (include/g4c.h g4c_mlp_tile_form): 64-row tiles (form 1, the one form shipped beside
form 0) against form 0, the 32-row tiles.  A row's arithmetic does not depend on its tile, so the form gives, bit for bit, what form 0
gives — output rows and both heads —, writes nothing past row M of any buffer, sets the same fp16 range flag and, certified, none.  Launches are reached through blocks.MLP as the models reach them; the chip-filling form (the one the tile forms
exist for) is selected at these small sizes with g4c_mlp_small_launch_tiles(0)."""
import pytest
import torch

import graphs4cfd_amd as gfd
from graphs4cfd_amd import _lib, ops, synthetic as S
from graphs4cfd_amd.nn.blocks import MLP
from graphs4cfd_amd.ops import Source

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
H = 128
NODE, UP, DOWN = _lib.TILE_SHAPE_NODE, _lib.TILE_SHAPE_UP, _lib.TILE_SHAPE_DOWN
TILE_KERNEL = {False: _lib.KERNEL_MLP_BX6, True: _lib.KERNEL_MLP_BX6_CERT}
DIM = 2          # columns of the narrow block (relative positions)
SENTINEL = -12345.0
PAD = 72         # rows behind M in every written buffer: more than a 64-row tile
FORMS = (1,)          # the shipped forms beside form 0
# every remainder at the 32- and 64-row boundaries; one 64-row tile, two, three
ROWS = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 193)


def tile_rows_of(form, shape=NODE):
    """Rows per workgroup g4c_mlp_last_tile_rows reports for a launch of `shape` under `form` (the DownMP shape has no 64-row form: it
    did not win its headline launch, and runs form 0)."""
    return 64 if form == 1 and shape != DOWN else 32


@pytest.fixture()
def tile_form():
    """f16x3 arithmetic, inference forms, no other kernel family, the two-step weight ring at every size, shapes on; everything restored."""
    lib = _lib.load()
    old = (ops.set_mlp_precision("f16x3"), lib.g4c_mlp_ws_enable(0), lib.g4c_mlp_bx6i_enable(0), lib.g4c_mlp_small_launch_tiles(0),
           lib.g4c_mlp_shapes_enable(1), lib.g4c_mlp_tile_form(-1))
    try:
        with torch.no_grad():
            yield lib
    finally:
        ops.set_mlp_precision(old[0]); lib.g4c_mlp_ws_enable(old[1]); lib.g4c_mlp_bx6i_enable(old[2])
        lib.g4c_mlp_small_launch_tiles(old[3]); lib.g4c_mlp_shapes_enable(old[4]); lib.g4c_mlp_tile_form(old[5])


_MLPS = {}


def mlps(layers, kind="node"):
    """(MLP of `layers` layers with the inputs of `kind`, the message MLP whose first-layer column blocks are its heads) — built once."""
    if (layers, kind) not in _MLPS:
        torch.manual_seed(20 + layers + 7 * len(kind))
        k_in = {"node": 2 * H, "up": DIM + 2 * H, "down": DIM + H}[kind]
        _MLPS[layers, kind] = (MLP(k_in, (H,) * layers, True).to(DEV), MLP(3 * H, (H, H, H), True).to(DEV))
    return _MLPS[layers, kind]


def rows(m, seed):
    return torch.randn(m, H, generator=torch.Generator().manual_seed(seed)).clamp_(-4, 4).to(DEV)


def narrow(m, seed):
    return torch.randn(m, DIM, generator=torch.Generator().manual_seed(seed)).clamp_(-4, 4).to(DEV)


def padded(m):
    return torch.full((m + PAD, H), SENTINEL, device=DEV)


def launch(lib, form, mlp, nxt, m, heads, srcs, act):
    """One launch under `form`: (every buffer it wrote, whole — output, then the heads; shape; kernel; rows per workgroup)."""
    lib.g4c_mlp_tile_form(form)
    bufs = [padded(m) for _ in range(1 + heads)]
    if heads:
        got = mlp.run_with_heads(srcs, m, _lib.act_code(act), nxt, H, [H, H], out=bufs[0][:m], head_outs=[b[:m] for b in bufs[1:]])
        assert got is not None
    else:
        mlp.run(srcs, m, act, out=bufs[0][:m])
    return bufs, int(lib.g4c_mlp_last_shape()), int(lib.g4c_mlp_last_kernel()), int(lib.g4c_mlp_last_tile_rows())


def same_bits(lib, mlp, nxt, m, heads, srcs, act, shape, certified):
    b0, s0, k0, r0 = launch(lib, 0, mlp, nxt, m, heads, srcs, act)
    assert (s0, k0, r0) == (shape, TILE_KERNEL[certified], 32), (m, s0, k0, r0)
    assert all(bool(torch.isfinite(x[:m]).all()) and bool((x[:m] != SENTINEL).any()) for x in b0), m
    for form in FORMS:
        b1, s1, k1, r1 = launch(lib, form, mlp, nxt, m, heads, srcs, act)
        assert (s1, k1, r1) == (shape, TILE_KERNEL[certified], tile_rows_of(form, shape)), (form, m, s1, k1, r1)
        for j, (x1, x0) in enumerate(zip(b1, b0)):
            assert torch.equal(x1, x0), (form, m, j)          # out, then both heads: rows below M and the rows behind them


@pytest.mark.parametrize("certified", [False, True], ids=["tracked", "certified"])
@pytest.mark.parametrize("heads", [0, 2])
@pytest.mark.parametrize("layers", [2, 3])
def test_node_update_forms_equal_form_0(tile_form, layers, heads, certified):
    lib = tile_form
    upd, nxt = mlps(layers)
    bound = 4.0 if certified else None
    for m in ROWS:
        srcs = [Source(rows(m, 100 + m), bound=bound), Source(rows(m, 200 + m), bound=bound)]
        same_bits(lib, upd, nxt, m, heads, srcs, "selu", NODE, certified)


def parents(m, n_coarse):
    """An int32 gather index that walks the coarse rows backwards, each one repeated: fine row r reads coarse row (m - 1 - r) // 3."""
    idx = (m - 1 - torch.arange(m)) // 3
    assert int(idx.max()) == n_coarse - 1 and int(idx.min()) == 0
    return idx.to(DEV, torch.int32)


@pytest.mark.parametrize("heads", [0, 2])
@pytest.mark.parametrize("layers", [2, 3])
def test_upmp_forms_equal_form_0(tile_form, layers, heads):
    """[-e (2 columns) | v_coarse[parent] | v_fine_old] -> MLP -> LayerNorm -> tanh (+ the next layer's two products); tracked (a
    launch with a narrow block has no range proof)."""
    lib = tile_form
    up, nxt = mlps(layers, "up")
    for m in ROWS:
        n_coarse = (m - 1) // 3 + 1
        srcs = [Source(narrow(m, 300 + m), negate=True), Source(rows(n_coarse, 500 + m), index=parents(m, n_coarse)), Source(rows(m, 600 + m))]
        same_bits(lib, up, nxt, m, heads, srcs, "tanh", UP, False)


@pytest.mark.parametrize("layers", [2, 3])
def test_downmp_forms_equal_form_0(tile_form, layers):
    """[e (2 columns) | v] -> MLP -> LayerNorm, no activation: the narrow block's rows are the tile's own.  (Routing only: this shape
    keeps its 32-row tiles under every form.)"""
    lib = tile_form
    down, nxt = mlps(layers, "down")
    for m in ROWS:
        srcs = [Source(narrow(m, 700 + m)), Source(rows(m, 800 + m))]
        same_bits(lib, down, nxt, m, 0, srcs, None, DOWN, False)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("m", [33, 65])
def test_write_footprint(tile_form, form, m):
    """Output and head tensors inside larger buffers pre-filled with a sentinel: every element outside rows [0, M) is unchanged, every row
    below M is written — node update with heads, UpMP with heads, DownMP."""
    lib = tile_form
    cases = [(NODE, mlps(3), 2, [Source(rows(m, 1)), Source(rows(m, 2))], "selu"),
             (UP, mlps(3, "up"), 2, [Source(narrow(m, 3), negate=True), Source(rows((m - 1) // 3 + 1, 4), index=parents(m, (m - 1) // 3 + 1)),
                                 Source(rows(m, 5))], "tanh"),
             (DOWN, mlps(3, "down"), 0, [Source(narrow(m, 6)), Source(rows(m, 7))], None)]
    for shape, (mlp, nxt), heads, srcs, act in cases:
        bufs, _, _, r = launch(lib, form, mlp, nxt, m, heads, srcs, act)
        assert r == tile_rows_of(form, shape)
        for j, x in enumerate(bufs):
            assert bool((x[m:] == SENTINEL).all()), (j, "rows past M")
            assert bool(torch.isfinite(x[:m]).all()) and bool((x[:m] != SENTINEL).any(dim=1).all()), (j, "rows below M")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("m,row", [(64, 40), (193, 40), (193, 192), (97, 96)], ids=["second-row-tile", "second-row-tile-of-3", "last-partial-tile", "last-tile-1-row"])
def test_range_flag_as_form_0(tile_form, form, m, row):
    """One input value beyond the fp16 range (its conversion reaches 65 504) in the second row tile of a 64-row tile, or in the last
    partial tile: the tracked node launch sets the slot of the caller's flag buffer that form 0 sets; without it no slot is set; the
    certified launch — a false bound, set by hand — writes no flag word."""
    lib = tile_form
    upd, nxt = mlps(3)
    a, b = rows(m, 11), rows(m, 12)
    hot = a.clone()
    hot[row, 77] = 1.0e5

    def flags_of(f, x, bound=None):
        flags = ops.RangeFlags(DEV)
        with flags:
            _, _, k, r = launch(lib, f, upd, nxt, m, 2, [Source(x, bound=bound), Source(b, bound=bound)], "selu")
        assert k == TILE_KERNEL[bound is not None] and r == tile_rows_of(f)
        return flags.buf.clone()
    want = flags_of(0, hot)
    assert int((want != 0).sum()) == 1
    assert torch.equal(flags_of(form, hot), want)
    assert not bool(flags_of(form, a).any())
    assert not bool(flags_of(form, hot, bound=4.0).any())


def test_64_row_tiles_from_three_times_the_small_launch_limit(tile_form):
    """64-row tiles run three workgroups per CU: a launch takes them when it has more than three times g4c_mlp_small_launch_tiles 32-row
    tiles, and its 32-row tiles below (same bits either way)."""
    lib = tile_form
    upd, nxt = mlps(3)
    lib.g4c_mlp_small_launch_tiles(2)
    got = {}
    for m in (192, 193):          # six 32-row tiles, seven
        srcs = [Source(rows(m, 31)), Source(rows(m, 32))]
        b1, s1, _, r1 = launch(lib, 1, upd, nxt, m, 2, srcs, "selu")
        b0, s0, _, r0 = launch(lib, 0, upd, nxt, m, 2, srcs, "selu")
        assert (s1, s0, r0) == (NODE, NODE, 32) and all(torch.equal(x1, x0) for x1, x0 in zip(b1, b0))
        got[m] = r1
    assert got == {192: 32, 193: 64}


def test_whole_model_forms_equal_form_0(tile_form, monkeypatch):
    """An eager NsThreeScaleGNN forward on a 3 000-node synthetic mesh, every launch in its chip-filling form: each tile form's prediction
    equals form 0's bit for bit, and its shaped launches ran in that form."""
    lib = tile_form
    lib.g4c_mlp_ws_enable(1); lib.g4c_mlp_bx6i_enable(1)          # (the model's own choice of kernel families)
    g = S.mus_graph(3000, levels=3, seed=3).to(DEV)
    torch.manual_seed(4)
    model = gfd.nn.NsThreeScaleGNN(arch=S.mus_arch("NsThreeScaleGNN", 128), device=DEV)
    model.eval()
    ran = []
    run = ops._run

    def recording(*args, **kw):
        run(*args, **kw)
        ran.append((int(lib.g4c_mlp_last_shape()), int(lib.g4c_mlp_last_tile_rows())))
    monkeypatch.setattr(ops, "_run", recording)
    preds = {}
    for form in (0,) + FORMS:
        lib.g4c_mlp_tile_form(form)
        del ran[:]
        preds[form] = model(g.clone()).clone()
        shaped = [r for s, r in ran if s in (NODE, UP)]
        assert shaped and set(shaped) == {tile_rows_of(form)}, (form, ran)
    assert bool(torch.isfinite(preds[0]).all())
    for form in FORMS:
        assert torch.equal(preds[form], preds[0]), form
