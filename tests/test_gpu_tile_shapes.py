"""mlp_bx6_kernel's compile-time launch shapes (include/g4c.h G4C_TILE_SHAPE_*, g4c_mlp_shapes_enable): a launch that matches a shape —
the MP layers' node update, UpMP's MLP (narrow block, indexed source, direct source), DownMP's MLP (narrow block, direct source) — gives,
bit for bit, what the all-runtime kernel gives — output rows, both heads, and nothing written past row M of any buffer — and a launch
that differs from a shape in one field runs the all-runtime kernel.  Launches are reached through blocks.MLP as the models reach them;
the two-step-ring form (the one the shapes exist for) is selected at these small sizes with g4c_mlp_small_launch_tiles(0)."""
import pytest
import torch

from graphs4cfd_amd import _lib, ops, plan
from graphs4cfd_amd.nn.blocks import MLP
from graphs4cfd_amd.ops import Source

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
H = 128
SELU, TANH = _lib.ACT_SELU, _lib.ACT_TANH
GENERIC, NODE, UP, DOWN = _lib.TILE_SHAPE_GENERIC, _lib.TILE_SHAPE_NODE, _lib.TILE_SHAPE_UP, _lib.TILE_SHAPE_DOWN
DIM = 2          # columns of the narrow block (relative positions)
TILE_KERNEL = {False: _lib.KERNEL_MLP_BX6, True: _lib.KERNEL_MLP_BX6_CERT}
SENTINEL = -12345.0
PAD = 40          # rows behind M in every written buffer: more than a tile
# one partial tile, an exact tile, one row into the second tile, several tiles with a partial last one; 289: ten tiles (the tile order's
# 8-way interleave with a remainder)
ROWS = (1, 31, 32, 33, 97, 289)


@pytest.fixture()
def tile_form():
    """f16x3 arithmetic, inference forms, no other kernel family, the two-step weight ring at every size; everything restored."""
    lib = _lib.load()
    old = (ops.set_mlp_precision("f16x3"), lib.g4c_mlp_ws_enable(0), lib.g4c_mlp_bx6i_enable(0), lib.g4c_mlp_small_launch_tiles(0),
           lib.g4c_mlp_shapes_enable(-1))
    try:
        with torch.no_grad():
            yield lib
    finally:
        ops.set_mlp_precision(old[0]); lib.g4c_mlp_ws_enable(old[1]); lib.g4c_mlp_bx6i_enable(old[2])
        lib.g4c_mlp_small_launch_tiles(old[3]); lib.g4c_mlp_shapes_enable(old[4])


_MLPS = {}


def mlps(layers, kind="node"):
    """(MLP of `layers` layers with the inputs of `kind`, the message MLP whose first-layer column blocks are its heads) — built once."""
    if (layers, kind) not in _MLPS:
        torch.manual_seed(10 + layers + 7 * len(kind))
        k_in = {"node": 2 * H, "up": DIM + 2 * H, "down": DIM + H}[kind]
        _MLPS[layers, kind] = (MLP(k_in, (H,) * layers, True).to(DEV), MLP(3 * H, (H, H, H), True).to(DEV))
    return _MLPS[layers, kind]


def rows(m, seed, window):
    """[m, 128] values in [-4, 4] as a Source argument list: a tensor of its own, or a column window of a wider one (ld > 128, col0 > 0)."""
    gen = torch.Generator().manual_seed(seed)
    if not window:
        return dict(tensor=torch.randn(m, H, generator=gen).clamp_(-4, 4).to(DEV))
    wide = torch.randn(m, 3 * H + 8, generator=gen).clamp_(-4, 4).to(DEV)
    return dict(tensor=wide, col0=H + 4, width=H)


def padded(m):
    return torch.full((m + PAD, H), SENTINEL, device=DEV)


def launch(lib, on, upd, nxt, m, heads, srcs, act="selu", **kw):
    """One launch with the shapes switched `on`: (every buffer it wrote, whole; shape; kernel)."""
    lib.g4c_mlp_shapes_enable(on)
    bufs = [padded(m) for _ in range(1 + heads)]
    if heads:
        got = upd.run_with_heads(srcs, m, _lib.act_code(act), nxt, H, [H, H], out=bufs[0][:m], head_outs=[b[:m] for b in bufs[1:]])
        assert got is not None
    else:
        upd.run(srcs, m, act, out=bufs[0][:m], **kw)
    return bufs, int(lib.g4c_mlp_last_shape()), int(lib.g4c_mlp_last_kernel())


def same_bits(lib, upd, nxt, m, heads, srcs, act, shape, certified):
    b1, s1, k1 = launch(lib, 1, upd, nxt, m, heads, srcs, act)
    b0, s0, k0 = launch(lib, 0, upd, nxt, m, heads, srcs, act)
    assert (s1, s0) == (shape, GENERIC), (m, s1, s0)
    assert k1 == k0 == TILE_KERNEL[certified], (m, k1, k0)
    for j, (x1, x0) in enumerate(zip(b1, b0)):
        assert torch.equal(x1, x0), (m, j)          # out, then both heads: rows below M and the rows behind them
        assert bool((x1[m:] == SENTINEL).all()) and bool((x0[m:] == SENTINEL).all()), (m, j)
        assert bool(torch.isfinite(x1[:m]).all()) and bool((x1[:m] != SENTINEL).any()), (m, j)


@pytest.mark.parametrize("window", [False, True], ids=["own", "window"])
@pytest.mark.parametrize("certified", [False, True], ids=["tracked", "certified"])
@pytest.mark.parametrize("heads", [0, 2])
@pytest.mark.parametrize("layers", [2, 3])
def test_node_update_shape_equals_generic(tile_form, layers, heads, certified, window):
    lib = tile_form
    upd, nxt = mlps(layers)
    bound = 4.0 if certified else None
    for m in ROWS:
        srcs = [Source(bound=bound, **rows(m, 100 + m, window)), Source(bound=bound, **rows(m, 200 + m, window))]
        same_bits(lib, upd, nxt, m, heads, srcs, "selu", NODE, certified)


def narrow(m, seed):
    return torch.randn(m, DIM, generator=torch.Generator().manual_seed(seed)).clamp_(-4, 4).to(DEV)


def parents(m, n_coarse, seed):
    """An int32 gather index with repeats (three fine rows per coarse row and more), the largest coarse row last."""
    idx = torch.randint(0, n_coarse, (m,), generator=torch.Generator().manual_seed(seed))
    idx[-1] = n_coarse - 1
    return idx.to(DEV, torch.int32)


@pytest.mark.parametrize("window", [False, True], ids=["own", "window"])
@pytest.mark.parametrize("heads", [0, 2])
@pytest.mark.parametrize("layers", [2, 3])
def test_upmp_shape_equals_generic(tile_form, layers, heads, window):
    """[-e (2 columns) | v_coarse[parent] | v_fine_old] -> MLP -> LayerNorm -> tanh (+ the next layer's two products), as
    UpMP.sources / the models' launch of it.  A launch with a narrow block has no range proof (ops.range_bounds): tracked, whatever
    bounds its sources carry."""
    lib = tile_form
    up, nxt = mlps(layers, "up")
    bound, certified = 4.0, False
    for m in ROWS:
        n_coarse = m // 3 + 1
        srcs = [Source(narrow(m, 300 + m), negate=True, bound=bound),
                Source(index=parents(m, n_coarse, 400 + m), bound=bound, **rows(n_coarse, 500 + m, window)),
                Source(bound=bound, **rows(m, 600 + m, window))]
        same_bits(lib, up, nxt, m, heads, srcs, "tanh", UP, certified)


@pytest.mark.parametrize("window", [False, True], ids=["own", "window"])
@pytest.mark.parametrize("layers", [2, 3])
def test_downmp_shape_equals_generic(tile_form, layers, window):
    """[e (2 columns) | v] -> MLP -> LayerNorm, no activation, as DownMP.pool launches it (tracked: see the UpMP case)."""
    lib = tile_form
    down, nxt = mlps(layers, "down")
    bound, certified = 4.0, False
    for m in ROWS:
        srcs = [Source(narrow(m, 700 + m), bound=bound), Source(bound=bound, **rows(m, 800 + m, window))]
        same_bits(lib, down, nxt, m, 0, srcs, None, DOWN, certified)


def test_a_source_of_2_gib_runs_the_generic_kernel(tile_form):
    """Row addressing with 32-bit offsets needs a source below 2^31 bytes: rows 8 300 000 floats apart (33 of them, 1.1 GB; only the
    128 columns that are read are written) take the all-runtime kernel, and give what the same rows give from a compact tensor."""
    lib = tile_form
    upd, nxt = mlps(3)
    m, ld = 33, 8_300_000
    assert (m + 32) * ld * 4 >= 2 ** 31
    far = torch.empty(m, ld, device=DEV)
    near = rows(m, 7, False)["tensor"]
    far[:, :H] = near
    other = Source(**rows(m, 8, False))
    b_far, s_far, _ = launch(lib, 1, upd, nxt, m, 2, [Source(far, col0=0, width=H), other])
    b_near, s_near, _ = launch(lib, 1, upd, nxt, m, 2, [Source(near), other])
    assert (s_far, s_near) == (GENERIC, NODE)
    assert all(torch.equal(a, b) for a, b in zip(b_far, b_near))


def test_an_output_of_2_gib_runs_the_generic_kernel(tile_form):
    """The output rows go through a buffer descriptor with 32-bit offsets too: an output whose rows lie 8 300 000 floats apart (33 of
    them; only the 128 columns the launch owns are written) takes the all-runtime kernel, the sources being compact, and holds what
    the same launch writes into a compact output.  (tests/test_gpu_tall.py has the same decision at the production leading dimension:
    16.8 million rows.)"""
    lib = tile_form
    upd, nxt = mlps(3)
    m, ld = 33, 8_300_000
    assert (m + 32) * ld * 4 >= 2 ** 31
    srcs = [Source(**rows(m, 7, False)), Source(**rows(m, 8, False))]
    far = torch.full((m, ld), SENTINEL, device=DEV)
    lib.g4c_mlp_shapes_enable(1)
    upd.run(srcs, m, "selu", out=far[:, :H])
    s_far, k_far = int(lib.g4c_mlp_last_shape()), int(lib.g4c_mlp_last_kernel())
    b_near, s_near, k_near = launch(lib, 1, upd, nxt, m, 0, srcs)
    assert (s_far, s_near) == (GENERIC, NODE) and k_far == k_near == TILE_KERNEL[False]
    assert torch.equal(far[:, :H], b_near[0][:m])
    assert bool((far[:, H:H + 4096] == SENTINEL).all()) and bool((far[:, -4096:] == SENTINEL).all())


def test_one_field_off_the_shape_runs_the_generic_kernel(tile_form):
    """Each launch matches the node-update shape in all but one field: shape 0, still the tile kernel."""
    lib = tile_form
    upd, nxt = mlps(3)
    m = 97
    a, b = rows(m, 1, False)["tensor"], rows(m, 2, False)["tensor"]

    def shape_of(srcs, mlp=upd, **kw):
        _, s, k = launch(lib, 1, mlp, nxt, m, 0, srcs, **kw)
        assert k in TILE_KERNEL.values(), k
        return s
    assert shape_of([Source(a), Source(b)]) == NODE          # (the launch the cases below vary)
    # a source with a pending activation
    assert shape_of([Source(a, pre_act=SELU), Source(b)]) == GENERIC
    # a source with aggregation on load: 3 rows per target, mean
    k = 3
    col = torch.arange(m).repeat_interleave(k)
    ei = torch.stack([torch.randint(0, m, (m * k,), generator=torch.Generator().manual_seed(3)), col]).to(DEV)
    _, csr = plan.edge_csr(ei, m)
    e = torch.randn(m * k, H, generator=torch.Generator().manual_seed(4)).to(DEV)
    assert shape_of([Source(e, segments=csr), Source(b)]) == GENERIC
    # a 64-wide source
    torch.manual_seed(5)
    half = MLP(H + 64, (H, H, H), True).to(DEV)
    assert shape_of([Source(a), Source(b, col0=0, width=64)], mlp=half) == GENERIC
    # an output index
    perm = torch.randperm(m, generator=torch.Generator().manual_seed(6)).to(DEV, torch.int32)
    assert shape_of([Source(a), Source(b)], out_idx32=perm) == GENERIC
    # a residual
    assert shape_of([Source(a), Source(b)], resid=a) == GENERIC
    # UpMP's blocks with the index on the second weighted source too; DownMP's blocks with an index
    up, down = mlps(3, "up")[0], mlps(3, "down")[0]
    idx = parents(m, m, 9)
    assert shape_of([Source(narrow(m, 10)), Source(a, index=idx), Source(b)], mlp=up) == UP
    assert shape_of([Source(narrow(m, 10)), Source(a, index=idx), Source(b, index=idx)], mlp=up) == GENERIC
    assert shape_of([Source(narrow(m, 10)), Source(a)], mlp=down) == DOWN
    assert shape_of([Source(narrow(m, 10)), Source(a, index=idx)], mlp=down) == GENERIC
