"""The launcher's policy (csrc/mlp_run.hip `choose`) at the sizes where it changes its mind, every knob as shipped: the kernel family and
tile shape on either side of the weight-stationary kernel's 20 000-row threshold, the dual-tile kernel's 400 000-row threshold and the
tile kernel's 512-tile deep-ring limit — the other tests force the modes to 0 / 2 or sit far from these sizes — and the two launches the
launcher refuses instead of computing something else.  Each case is one launch; which kernel ran (g4c_mlp_last_kernel /
g4c_mlp_last_shape) is the subject, the output is only checked to be finite (tests/test_gpu_fwd_ref.py owns correctness)."""
import pytest
import torch

from graphs4cfd_amd import _lib, ops, plan

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
H = 128
N_NODES = 1000
NONE, BX6, BX6I, WS, BX6_CERT, WS_CERT = 0, _lib.KERNEL_MLP_BX6, 3, _lib.KERNEL_MLP_WS, _lib.KERNEL_MLP_BX6_CERT, _lib.KERNEL_MLP_WS_CERT
GENERIC, NODE = _lib.TILE_SHAPE_GENERIC, _lib.TILE_SHAPE_NODE

# (form, arithmetic, certified, rows) -> (g4c_mlp_last_kernel, g4c_mlp_last_shape).  Recorded from the library of commit 09ec35e (the
# launcher before it was taken apart), same launches, same device — not read off the code under test.
EXPECT = {
    ("message", "f16x3", False, 19_999): (BX6, GENERIC),
    ("message", "f16x3", False, 20_000): (WS, GENERIC),
    ("message", "f16x3", True, 19_999): (BX6_CERT, GENERIC),
    ("message", "f16x3", True, 20_000): (WS_CERT, GENERIC),
    ("message", "bf16x6", False, 399_999): (BX6, GENERIC),
    ("message", "bf16x6", False, 400_000): (BX6I, GENERIC),
    ("node", "f16x3", False, 512 * 32): (BX6, GENERIC),
    ("node", "f16x3", False, 512 * 32 + 1): (BX6, NODE),
}


@pytest.fixture()
def shipped():
    """Every knob at its shipped default — asserted, not set — and restored."""
    lib = _lib.load()
    assert ops.mlp_precision() == "f16x3" and lib.g4c_mlp_ws_enable(-1) == 1 and lib.g4c_mlp_bx6i_enable(-1) == 1
    assert lib.g4c_mlp_small_launch_tiles(-1) == 512 and lib.g4c_mlp_shapes_enable(-1) == 1 and ops.RANGE_PROOFS
    old = (lib.g4c_mlp_ws_enable(-1), lib.g4c_mlp_bx6i_enable(-1), lib.g4c_mlp_small_launch_tiles(-1), lib.g4c_mlp_shapes_enable(-1))
    try:
        with torch.no_grad():
            yield lib
    finally:
        lib.g4c_mlp_ws_enable(old[0]); lib.g4c_mlp_bx6i_enable(old[1]); lib.g4c_mlp_small_launch_tiles(old[2]); lib.g4c_mlp_shapes_enable(old[3])


_ROWS = {}


def rows(n, width=H, seed=0):
    """[n, width] values in [-4, 4]: the first n rows of one tensor per (width, seed), grown when a case asks for more."""
    if (width, seed) not in _ROWS or _ROWS[width, seed].size(0) < n:
        gen = torch.Generator(device=DEV).manual_seed(width + seed)
        _ROWS[width, seed] = torch.randn(n, width, generator=gen, device=DEV).clamp_(-4, 4)
    return _ROWS[width, seed][:n]


def index(n, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randint(0, N_NODES, (n,), generator=gen, device=DEV, dtype=torch.int32)


def packed(k_blocks, layers, precision, **kw):
    """`layers` 128-wide Linear layers over `k_blocks` 128-wide input blocks + LayerNorm, nn.Linear's initial scale."""
    gen = torch.Generator().manual_seed(7 * k_blocks + layers)
    Ws = [((torch.rand(H, k, generator=gen) * 2 - 1) / k ** 0.5).to(DEV) for k in [k_blocks * H] + [H] * (layers - 1)]
    bs = [((torch.rand(H, generator=gen) * 2 - 1) / H ** 0.5).to(DEV) for _ in Ws]
    ln = (torch.ones(H, device=DEV), torch.zeros(H, device=DEV), 1e-5)
    return ops.PackedMLP(Ws, bs, ln, [H] * k_blocks, [False] * k_blocks, precision=precision, site="policy", **kw)


def message_sources(n, bound=None, x=None):
    """The hoisted message form: one weighted 128-wide block + two indexed 128-wide additive blocks."""
    return [ops.Source(rows(n) if x is None else x, bound=bound, **({} if x is None else dict(col0=1, width=H))),
            ops.Source(rows(N_NODES, seed=1), index(n, 1), additive=True, bound=bound),
            ops.Source(rows(N_NODES, seed=2), index(n, 2), additive=True, bound=bound)]


@pytest.mark.parametrize("case", list(EXPECT), ids=lambda c: f"{c[0]}-{c[1]}-{'certified' if c[2] else 'tracked'}-{c[3]}")
def test_family_on_either_side_of_a_threshold(shipped, case):
    lib = shipped
    form, precision, certified, n = case
    if form == "message":
        y = ops.mlp_forward(packed(1, 3, precision), message_sources(n, 4.0 if certified else None), n)
    else:          # the node-update form: two direct 128-wide blocks, no heads
        y = ops.mlp_forward(packed(2, 3, precision), [ops.Source(rows(n)), ops.Source(rows(n, seed=3))], n, _lib.ACT_SELU)
    ran = (int(lib.g4c_mlp_last_kernel()), int(lib.g4c_mlp_last_shape()))
    assert ran == EXPECT[case], f"{case}: (kernel, shape) = {ran}, the launcher of 09ec35e chose {EXPECT[case]}"
    assert tuple(y.shape) == (n, H) and bool(torch.isfinite(y).all())


def test_row_split_image_outside_its_envelope_is_refused(shipped):
    """A stream in the row-split kernel's k order can run on no other kernel: an output activation, which mlp_rs1_kernel does not
    apply, fails the call — nothing launches."""
    lib = shipped
    n = 640
    pk = packed(1, 3, "bf16", rs_order=True)
    ops.mlp_forward(pk, message_sources(n), n)          # (inside the envelope the same launch runs, on the row-split kernel)
    assert int(lib.g4c_mlp_last_kernel()) == _lib.KERNEL_MLP_RS
    with pytest.raises(NotImplementedError, match="G4C_WFMT_BF16_RS"):          # (G4C_EUNSUPPORTED)
        ops.mlp_forward(pk, message_sources(n), n, _lib.ACT_SELU)
    assert int(lib.g4c_mlp_last_kernel()) == NONE and int(lib.g4c_mlp_last_shape()) == GENERIC


def test_fused_mp_layer_outside_the_weight_stationary_envelope_is_refused(shipped):
    """io->upd runs on mlp_ws_kernel or not at all: a message block whose rows are not 16-byte addressable (a window at column 1 of a
    130-wide tensor) fails the call — nothing launches."""
    lib = shipped
    csr = plan.build_csr(torch.arange(100).repeat_interleave(6), 100, DEV)
    msg, upd, v = packed(1, 3, "f16x3"), packed(2, 3, "f16x3"), rows(100, seed=3)
    e, v_out, _ = ops.mp_layer_forward(msg, message_sources(csr.n), csr.n, csr, True, upd, v, _lib.ACT_SELU)      # (aligned: it runs)
    assert int(lib.g4c_mlp_last_kernel()) == WS and bool(torch.isfinite(v_out).all())
    with pytest.raises(NotImplementedError, match="outside the weight-stationary kernel's envelope"):          # (G4C_EUNSUPPORTED)
        ops.mp_layer_forward(msg, message_sources(csr.n, x=rows(csr.n, H + 2)), csr.n, csr, True, upd, v, _lib.ACT_SELU)
    assert int(lib.g4c_mlp_last_kernel()) == NONE and int(lib.g4c_mlp_last_shape()) == GENERIC
