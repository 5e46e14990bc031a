"""The host decisions of the MP-layer path, tabulated on the CPU (no library): `blocks.hoist_decision` as each site asks it, against
the expression that site spelled out itself before the decision had one place (commit 2543cc0), over rows on either side of
HOIST_MIN_ROWS x the four arithmetics x HOIST_BF16 x grad mode x products given; and the two block predicates, `Source.whole_block`
and `ops.vector_rows`, over blocks that violate exactly one clause each.  The sites disagree, on purpose and visibly: the rows of
`SITES` differ where the parent's sites differed."""
import itertools
from types import SimpleNamespace

import pytest
import torch

from graphs4cfd_amd import _lib, ops, partition as P
from graphs4cfd_amd.nn import blocks as B

T = B.HOIST_MIN_ROWS
H = 128

# site -> (how the site asks now: keywords of hoist_decision from (products given), what it computed before: from (rows, arithmetic,
# HOIST_BF16, grad mode, products given))
SITES = {
    "MLP.run_hoisted": (lambda given: dict(forced=given, vetoes="consumer"),
                        lambda n, p, hb, grad, given: not ((n < T or (p == "bf16" and not hb) or grad) and not given)),
    "_MuSGNN._launch_for": (lambda given: dict(), lambda n, p, hb, grad, given: n >= T),          # (+ will_fuse_layer: below)
    "_mp_step next_msg": (lambda given: dict(), lambda n, p, hb, grad, given: n >= T),
    "_mp_step static_first_layer(hoists=)": (lambda given: dict(forced=given), lambda n, p, hb, grad, given: n >= T or given),
    "UpEdgeMP.step / REMuS level entry": (lambda given: dict(), lambda n, p, hb, grad, given: n >= T),
    "HipImpl.hoists": (lambda given: dict(vetoes="bf16"), lambda n, p, hb, grad, given: n >= T and p != "bf16"),
}
GRID = list(itertools.product((T - 1, T), ("f16x3", "bf16x6", "bf16", "fp32"), (True, False), (False, True), (False, True)))


@pytest.fixture()
def mlp():
    return B.MLP(3 * H, (H, H, H), True)


@pytest.mark.parametrize("site", list(SITES))
def test_hoisting_decision_site_by_site(site, mlp, monkeypatch):
    now, before = SITES[site]
    for n, prec, hb, grad, given in GRID:
        monkeypatch.setattr(B, "HOIST_BF16", hb)
        with ops.mlp_precision_as(prec), torch.set_grad_enabled(grad):
            got = B.hoist_decision(mlp, n, **now(given))
            assert got == (before(n, prec, hb, grad, given), False), (site, n, prec, hb, grad, given)
            if site == "HipImpl.hoists":
                assert P.HipImpl(None).hoists(n) == got[0]


def test_the_sites_disagree_where_they_did():
    """The kept disagreements, as rows: bf16 without HOIST_BF16 and grad mode stop the consumer, not the producers that ask for it;
    HipImpl excludes bf16 whatever HOIST_BF16 says; products handed in move the consumer and the static first layer only."""
    def table(site):
        return [SITES[site][1](*row) for row in GRID]
    assert table("MLP.run_hoisted") != table("_mp_step next_msg") != table("HipImpl.hoists") != table("MLP.run_hoisted")
    assert table("_mp_step static_first_layer(hoists=)") != table("_mp_step next_msg")


def test_decision_rows_replace_the_launchs_own_count(mlp):
    with torch.no_grad():
        assert B.hoist_decision(mlp, T, decision_rows=T - 1) == (False, False)
        assert B.hoist_decision(mlp, T - 1, decision_rows=T) == (True, False)
    with pytest.raises(ValueError, match="vetoes"):
        B.hoist_decision(mlp, T, vetoes="all")


def test_a_layer_that_will_fuse_hoists_at_any_size(mlp, monkeypatch):
    """_launch_for's addition: below HOIST_MIN_ROWS the consumer still hoists when its layer runs as one fused launch."""
    upd, ei = B.MLP(2 * H, (H, H, H), True), torch.zeros(2, B.FUSE_LAYER_MIN_ROWS, dtype=torch.long)
    asked = []
    monkeypatch.setattr(B, "will_fuse_layer", lambda *a: asked.append(a) or True)
    with torch.no_grad():
        assert B.hoist_decision(mlp, B.FUSE_LAYER_MIN_ROWS, layer=(upd, ei, 16)) == (True, False)
        assert asked == [(mlp, upd, ei, 16)]
        assert B.hoist_decision(mlp, T, layer=(upd, ei, 16)) == (True, False) and len(asked) == 1          # (rows alone decide first)


def test_row_split_order_follows_rs1_ready(monkeypatch):
    """rs_rows is MLP.rs1_ready of the launch's own rows and CSR — asked only of a consumer that hoists."""
    m = B.MLP(3 * H, (H, H), True)
    csr = SimpleNamespace(n=T, uniform_deg=5, tiles=lambda: ((), (), 1))
    with ops.mlp_precision_as("bf16"), torch.no_grad():
        assert m.rs1_ready(T, csr)
        assert B.hoist_decision(m, T, csr) == (True, True)
        assert B.hoist_decision(m, T, csr, decision_rows=T - 1) == (False, False)
        assert B.hoist_decision(m, T, SimpleNamespace(n=T, uniform_deg=9, tiles=lambda: ((), (), 1))) == (True, False)
    with ops.mlp_precision_as("f16x3"), torch.no_grad():
        assert B.hoist_decision(m, T, csr) == (True, False)


def test_node_heads_arithmetic(mlp):
    assert mlp.node_heads(H) == (H, [H, H]) and B.MLP(5 * H, (H, H), True).node_heads(2 * H) == (H, [2 * H, 2 * H])


# ------------------------------------------------------------------------------------- the two predicates
def _block(**kw):
    return ops.Source(kw.pop("tensor", torch.zeros(4, H)), **kw)


ONE_CLAUSE = {
    "width": dict(tensor=torch.zeros(4, H + 8), width=H + 8),
    "col0": dict(tensor=torch.zeros(4, H + 8), col0=8),
    "negate": dict(negate=True),
    "index": dict(index=torch.zeros(4, dtype=torch.int32)),
    "segments": dict(segments=SimpleNamespace()),
    "additive": dict(additive=True),
    "pre_act": dict(pre_act=_lib.ACT_TANH),
    "dtype": dict(tensor=torch.zeros(4, H, dtype=torch.bfloat16)),
}


def test_whole_block_one_clause_at_a_time():
    kw = dict(pre_acts=(_lib.ACT_NONE, _lib.ACT_SELU), dtypes=(torch.float32,))
    assert _block().whole_block(H, **kw) and _block(pre_act=_lib.ACT_SELU).whole_block(H, **kw)
    for clause, bad in ONE_CLAUSE.items():
        assert not _block(**bad).whole_block(H, **kw), clause
    # what a caller admits: any activation on load, any tensor type
    assert _block(pre_act=_lib.ACT_TANH).whole_block(H, pre_acts=None) and not _block(pre_act=_lib.ACT_SELU).whole_block(H)
    assert _block(tensor=torch.zeros(4, H, dtype=torch.bfloat16)).whole_block(H)
    # the other plain form: a gathered, additive product — both or neither
    idx = torch.zeros(4, dtype=torch.int32)
    assert _block(index=idx, additive=True).whole_block(H, product=True)
    assert not _block(additive=True).whole_block(H, product=True) and not _block(index=idx).whole_block(H, product=True)
    assert not _block().whole_block(H, product=True)


def test_vector_rows_one_clause_at_a_time():
    wide = torch.zeros(8, H + 4)
    assert wide.data_ptr() % 16 == 0
    assert ops.vector_rows(torch.zeros(8, H)) and ops.vector_rows(wide[:, :H]) and ops.vector_rows(wide[:, 4:])
    assert ops.vector_rows(wide, 4) and not ops.vector_rows(wide, 2)                      # (from a column on)
    assert not ops.vector_rows(torch.zeros(H, 8).t())                                      # unit column stride
    assert not ops.vector_rows(wide[:, 1:H + 1])                                           # a 16-byte aligned first element
    assert not ops.vector_rows(torch.zeros(8, H + 2)[:, :H])                               # a row stride of whole 16-byte pieces
    w16 = torch.zeros(8, H + 4, dtype=torch.bfloat16)
    assert ops.vector_rows(torch.zeros(8, H, dtype=torch.bfloat16)) and not ops.vector_rows(w16[:, :H])     # (bf16: 8 values, not 4)
    assert ops.vector_rows(torch.zeros(8, H + 8, dtype=torch.bfloat16)[:, 8:])
