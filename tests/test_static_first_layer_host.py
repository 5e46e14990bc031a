"""The "first layer precomputed" message launch, host side (no GPU): which MP layer takes it (nn/blocks.py static_first_layer) and what
g4c_mlp_run accepts as such a launch (every source additive, g4c_mlp_t.k_pad[0] == 0) — every combination that is not built comes back as G4C_EUNSUPPORTED
(or G4C_EINVAL for a malformed call) before the device is touched."""
import ctypes as C

import pytest
import torch

from graphs4cfd_amd import _lib, ops
from graphs4cfd_amd.nn import blocks as B
from graphs4cfd_amd.ops import Source


# ------------------------------------------------------------------ the routing predicate
@pytest.fixture
def layer(monkeypatch):
    """An MP layer of the headline shape whose launch would reduce its own rows and is not a fused layer; the knobs the cases turn."""
    msg, upd = B.MLP(384, (128, 128, 128), True), B.MLP(256, (128, 128, 128), True)
    state = {"fuses": False, "agg": True}
    monkeypatch.setattr(B, "will_fuse_layer", lambda *a: state["fuses"])
    monkeypatch.setattr(ops, "can_fuse_aggregation", lambda *a: state["agg"])
    monkeypatch.setattr(ops, "STATIC_FIRST_LAYER", True)
    prev = ops.set_mlp_precision("f16x3")
    e0, attr = torch.zeros(64, 128), torch.zeros(64, 3)

    def takes(e_src=None, e_static=(attr,), hoists=True, m=msg):
        return B.static_first_layer(m, upd, Source(e0) if e_src is None else e_src, e_static, torch.zeros(2, 64, dtype=torch.long), 16, None, hoists)
    yield takes, state, e0
    ops.set_mlp_precision(prev)


def test_only_the_static_layer_of_an_f16x3_rollout_takes_the_precomputed_form(layer, monkeypatch):
    takes, state, e0 = layer
    with torch.no_grad():
        assert ops.StaticCache.active is None and not takes()               # a bare forward(): no cache, today's launch
        with ops.StaticCache():
            assert takes()
            assert not takes(e_static=None) and not takes(e_static=())          # any other layer: its e is not the program's e0
            assert not takes(hoists=False)                                      # a launch that multiplies its node rows itself
            state["fuses"] = True
            assert not takes()                                                  # one launch per MP layer has no such form
            state["fuses"] = False
            state["agg"] = False
            assert not takes()                                                  # the launch does not reduce its own rows
            state["agg"] = True
            for prec in ("bf16x6", "fp32", "bf16"):
                old = ops.set_mlp_precision(prec)
                try:
                    assert not takes(), prec
                finally:
                    ops.set_mlp_precision(old)
            assert takes()
            # the edge latents as the launch reads them: stored activated, a plain 128-wide fp32 block
            assert not takes(e_src=Source(e0, pre_act=_lib.ACT_SELU))
            assert not takes(e_src=Source(e0, index=torch.zeros(64, dtype=torch.int32)))
            assert not takes(e_src=Source(torch.zeros(64, 256), col0=128, width=128))
            assert not takes(e_src=Source(e0, negate=True))
            # another message MLP: two layers, another width
            assert not takes(m=B.MLP(384, (128, 128), True)) and not takes(m=B.MLP(384, (128, 64, 128), True))
            assert not takes(m=B.MLP(320, (128, 128, 128), True))
            monkeypatch.setattr(ops, "STATIC_FIRST_LAYER", False)               # G4C_STATIC_FIRST_LAYER=0
            assert not takes()
            monkeypatch.setattr(ops, "STATIC_FIRST_LAYER", True)
        with ops.StaticCache():
            with torch.enable_grad():
                assert not takes()                                              # training: recorded for autograd
    assert ops.StaticCache.active is None


def test_a_cache_entered_under_another_arithmetic_drops_the_entries_of_the_old_one():
    """A rollout that falls back to bf16x6 no longer asks for T: left in the cache, its key (arithmetic f16x3) would read as stale before
    every step and the step would never be captured again.  The step that follows a change of arithmetic enters the cache, which drops
    the old arithmetic's entries; what the step still uses (the edge latents) is computed again — a miss, as it was before."""
    attr = torch.zeros(4, 3)
    prev = ops.set_mlp_precision("f16x3")
    try:
        c = ops.StaticCache()
        with torch.no_grad(), c:
            ops.static_launch("edge_encoder", [attr], lambda: torch.ones(1))
            ops.static_launch(B.STATIC_FIRST_NAME, [attr], lambda: torch.ones(1))
        assert not c.stale() and c.misses == 2
        with torch.no_grad(), c:                          # the same arithmetic: nothing goes, both are hits
            ops.static_launch("edge_encoder", [attr], lambda: torch.ones(1))
            ops.static_launch(B.STATIC_FIRST_NAME, [attr], lambda: torch.ones(1))
        assert (c.hits, c.misses) == (2, 2)
        ops.set_mlp_precision("bf16x6")
        assert c.stale()
        with torch.no_grad(), c:                          # the step of a rollout that fell back: it asks for the edge latents only
            assert c.store == {}
            ops.static_launch("edge_encoder", [attr], lambda: torch.ones(1))
        assert c.misses == 3 and set(c.store) == {"edge_encoder"} and not c.stale()
    finally:
        ops.set_mlp_precision(prev)


# ------------------------------------------------------------------ g4c_mlp_run's argument checks
BASE = 0x10000          # (addresses are only compared and checked for alignment: nothing is launched)


def call(**edit):
    """A well-formed "first layer precomputed" call — three layers of the f16x3 stream without layer 0, T direct + two gathered
    products, the fused aggregation over a plan of no tiles (so a call that passes every check launches nothing) — with `edit`s."""
    NP, blk = 128, 128 * 128 * 6
    mlp = _lib.g4c_mlp_t(n_layers=3, n_out=NP, w_format=_lib.WFMT_F16X2)
    for l in range(3):
        mlp.k_pad[l], mlp.n_pad[l] = (0 if l == 0 else NP), NP
        mlp.w[l] = BASE + max(l - 1, 0) * blk
        mlp.b[l] = 16 * BASE + 4 * NP * l
    srcs = (_lib.g4c_src_t * 4)()
    for j in range(3):
        srcs[j].ptr, srcs[j].width, srcs[j].ld, srcs[j].additive = 32 * BASE * (j + 1), NP, NP, 1
        srcs[j].idx = None if j == 0 else 48 * BASE * j
    io = _lib.g4c_mlp_io_t(row_count=64, out=64 * BASE, out_ld=NP, tile_rows=65 * BASE, tile_seg=66 * BASE, seg_off=67 * BASE, n_tiles=0,
                           agg=68 * BASE, agg_ld=NP, agg_mode=1)
    n_src, keep = 3, []
    for key, val in edit.items():
        if key == "n_src":
            n_src = val
        elif key == "mlp":
            for k, v in val.items():
                setattr(mlp, k, v)
        elif key == "layers":
            val(mlp)
        elif key == "io":
            for k, v in val.items():
                setattr(io, k, v)
        elif key == "src":
            j, fields = val
            for k, v in fields.items():
                setattr(srcs[j], k, v)
        elif key == "upd":
            upd = _lib.g4c_mlp_t(n_layers=3, n_out=NP, w_format=_lib.WFMT_F16X2)
            keep.append(upd)
            io.upd = C.pointer(upd)
    lib = _lib.load()
    rc = lib.g4c_mlp_run(C.byref(mlp), srcs, n_src, 64, C.byref(io), None)
    return rc, lib.g4c_last_error().decode()


def test_a_well_formed_call_passes_every_check():
    rc, msg = call()
    assert rc == _lib.OK, msg
    assert _lib.load().g4c_mlp_last_kernel() == 0          # (a plan of no tiles: nothing launched)
    assert _lib.KERNEL_MLP_WS_PRE == 9


def two_layers(mlp):
    mlp.n_layers = 2


def fp32_stream(mlp):          # (four bytes per weight: where layer 2 starts in that stream)
    mlp.w[2] = mlp.w[1] + 128 * 128 * 4


# what the launcher's own checks of the form say, and what the stages in front of them say for calls they refuse first
ENVELOPE = "every source additive (first layer precomputed) is outside the weight-stationary kernel's envelope"
FORMAT = "every source additive (first layer precomputed) needs the f16x3 format (G4C_WFMT_F16X2), got w_format "
AGG_STAGE = "the fused aggregation needs a split-operand w_format and a plain 128-wide output"
UNSUPPORTED = {
    "the bf16x6 stream": (dict(mlp={"w_format": _lib.WFMT_BF16X3}), FORMAT + "2"),
    "the rounded-bf16 stream": (dict(mlp={"w_format": _lib.WFMT_BF16}), FORMAT + "6"),
    "the fp32 stream": (dict(mlp={"w_format": _lib.WFMT_FP32}, layers=fp32_stream), AGG_STAGE),
    "one layer left": (dict(layers=two_layers), "every source additive (first layer precomputed) needs three layers (two left), got 2"),
    "no fused aggregation": (dict(io={"agg": None}), "every source additive (first layer precomputed) needs the fused aggregation and no save"),
    "the fused MP layer": (dict(upd=True), "upd must have the message MLP's depth (3), two 128-wide input blocks"),
    "T through an index": (dict(src=(0, {"idx": BASE})), ENVELOPE),
    "a product without its index": (dict(src=(1, {"idx": None})), ENVELOPE),
    "a narrow additive block": (dict(src=(2, {"width": 64})), ENVELOPE),
    "rows that are not 16-byte aligned": (dict(src=(0, {"ptr": 32 * BASE + 4})), ENVELOPE),
    "a leading dimension that is no multiple of 4": (dict(src=(1, {"ld": 130})), ENVELOPE),
    "bf16 additive rows": (dict(src=(2, {"dtype": 1})), "bf16 additive rows need the rounded-bf16 mode"),
    "two additive blocks": (dict(n_src=2), ENVELOPE),
    "an output activation on compact rows": (dict(io={"out_dtype": 1}), "bf16 output rows need the rounded-bf16 mode"),
    "misaligned output rows": (dict(io={"out": 64 * BASE + 8}), ENVELOPE),
    "a residual": (dict(io={"resid": 70 * BASE, "resid_ld": 128}), AGG_STAGE),
    "a narrower output": (dict(mlp={"n_out": 64}), AGG_STAGE),
}


@pytest.mark.parametrize("what", sorted(UNSUPPORTED))
def test_every_combination_that_is_not_built_is_refused(what):
    edit, text = UNSUPPORTED[what]
    rc, msg = call(**edit)
    assert rc == _lib.EUNSUPPORTED, (what, rc, msg)
    assert msg.startswith("g4c_mlp_run: " + text), (what, msg)


def test_heads_and_training_forms_are_refused():
    heads = (C.c_void_p * _lib.MAX_HEADS)(71 * BASE, 72 * BASE)
    rc, msg = call(io={"n_heads": 2, "head_ld": 128, "head_out": heads})
    assert rc == _lib.EUNSUPPORTED and msg == "g4c_mlp_run: heads with the fused aggregation", (rc, msg)
    rc, msg = call(io={"n_save": 3, "save_ld": 128})
    assert rc == _lib.EUNSUPPORTED and msg.startswith("g4c_mlp_run: save needs w_format BF16X3 / F16X2 / BF16 without heads / aggregation"), (rc, msg)
    rc, msg = call(io={"out_idx": 73 * BASE})
    assert rc == _lib.EUNSUPPORTED and msg == "g4c_mlp_run: " + AGG_STAGE, (rc, msg)


def test_malformed_calls_are_invalid():
    # a weighted (or narrow) block beside "no layer-0 weights"
    rc, msg = call(src=(0, {"additive": 0}))
    assert rc == _lib.EINVAL and "padded columns" in msg, (rc, msg)
    # no source at all that could stand for the first layer
    rc, msg = call(n_src=0)
    assert rc == _lib.EUNSUPPORTED and msg == "g4c_mlp_run: 0 sources (max 4)", (rc, msg)
    # the stream of such a descriptor starts with layer 1: w[0] == w[1]
    rc, msg = call(mlp={})
    assert rc == _lib.OK

    def shifted(mlp):
        mlp.w[1] = mlp.w[0] + 128 * 128 * 6
    rc, msg = call(layers=shifted)
    assert rc == _lib.EINVAL and "contiguous" in msg, (rc, msg)
