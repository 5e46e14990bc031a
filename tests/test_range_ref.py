"""The planted cases of tests/range_cases.py on the CPU: every case meets its conditions on the fp64 reference (oracle/fwd_ref.py
`converted`), the flag contract `expected_flag` agrees with the torch emulation of the f16x3 operand split (`emulated_flag`), and — the
negative controls — for every site of every launch form there is a case that a kernel WITHOUT a tracker at that site would get wrong:
`emulated_flag(skip={site})` is False where the expected flag is True.  Nothing here launches anything."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import range_cases as K                      # noqa: E402
from oracle import fwd_ref as R              # noqa: E402


def emulated(c, skip=()):
    return R.emulated_flag(c.launch(), skip, c.has_heads())


@pytest.mark.parametrize("group", K.GROUPS)
def test_every_case_meets_its_conditions_and_the_emulation_agrees(group):
    cases = K.catalogue(group)
    assert cases
    for c in cases:
        for case in (c,) + ((c.twin,) if c.twin is not None else ()):
            K.conditions(case)
            assert emulated(case) == case.expect == R.expected_flag(case.sites()), case.name
        if c.level == "element":          # one element of one site
            v = c.sites()[c.site].abs()
            assert int((v >= K.END).sum()) == (1 if c.expect else 0), (c.name, int((v >= K.END).sum()))


@pytest.mark.parametrize("group", K.PLANTED_GROUPS)
def test_a_tracker_missing_at_any_site_is_caught(group):
    """Per launch form: every site the form converts has a planted case, and with that site's tracker left out the emulated kernel
    stays silent on it (so the GPU test, which demands the flag, fails) — while with any OTHER tracker left out it still flags."""
    forms = {}
    for c in K.catalogue(group):
        if c.expect:
            forms.setdefault(c.form, []).append(c)
    assert forms
    for form, cases in forms.items():
        sites = set(cases[0].sites())
        assert all(set(c.sites()) == sites for c in cases), form
        caught = {c.site for c in cases if not emulated(c, skip={c.site})}
        assert caught == sites, (form, "no planted case pins", sorted(sites - caught))
        for c in cases:
            assert all(emulated(c, skip={s}) for s in sites - {c.site}), (c.name, "another site flags as well")


def test_positions_cover_rows_columns_and_both_blocks():
    """Rows 0, a middle tile and n - 1; columns 0, 37, 70, 127; the first and the second block of the 256-wide first layer."""
    rows, cols = set(), {}
    for c in K.catalogue("node"):
        if c.level == "element" and c.site.startswith("in"):
            v = c.sites()[c.site].abs()
            r, col = divmod(int(v.argmax()), int(v.size(1)))
            rows.add((c.n, r)); cols.setdefault(c.site, set()).add(col)
    assert rows == {(n, r) for n in K.TILE_N for r in K.rows_at(n)}
    assert cols["in0"] | cols["in1"] == set(K.COLS) and len(cols["in0"]) >= 2 and len(cols["in1"]) >= 2
    through = {c.name.split("through ")[1].split(" ")[0] for c in K.catalogue("node") if c.site == "h1"}
    assert through == {"in0", "in1"}


def test_threshold_triple_in_the_emulation():
    for group in ("threshold", "threshold_ws"):
        seen = set()
        for c in K.catalogue(group):
            v = c.sites(torch.float32)[c.site]
            big = v[v.abs() > 3e4]
            assert big.numel() == 1 and abs(float(big)) == c.site_exact, c.name
            assert c.expect == (c.site_exact == K.END) == emulated(c), c.name
            seen.add((float(big) > 0, c.expect))
        assert seen == {(True, True), (False, True), (True, False), (False, False)}
    assert K.BELOW < K.END and K.BELOW == 65504.0 - 2.0 ** -8


def test_selu_on_load_sign():
    for group in ("selu_sign", "selu_sign_ws"):
        neg, pos = K.catalogue(group)[:2]
        assert not neg.expect and pos.expect and not emulated(neg) and emulated(pos)
        assert abs(float(neg.sites()["in0"].min()) + 1.7580993408473766) < 1e-9 or float(neg.sites()["in0"].abs().max()) < 200


def test_segments_on_the_host_drop_the_unnamed_rows():
    b = K.Blk(torch.zeros(6, 4), keys=torch.tensor([2, 0, 3, 2, 1, 3]), n_seg=3)
    off, perm = b.segments()
    assert off.tolist() == [0, 1, 2, 4] and perm.tolist() == [1, 4, 0, 3] and b.drops()


def test_weights_beyond_the_fp16_range_are_refused_by_name():
    """ops.weight_norms carries max|W| of every matrix an f16x3 image converts (narrow blocks are not converted), and
    ops.check_weight_range refuses 65504 and beyond — naming the site and the matrix, pointing to bf16x6."""
    from graphs4cfd_amd import ops
    W, b, ln, hs = R.default_weights(4 + 128, (128, 128, 128), K.gen(1), True, "ln", 2)
    lnp = (ln[0], ln[1], R.LN_EPS)

    def norms():
        return ops.weight_norms(W, b, lnp, hs, (4, 128), narrow=(True, False))
    n = norms()
    assert n["w0_max"] == [float(W[0][:, 4:].abs().max())] and n["w_max"] == [float(x.abs().max()) for x in W[1:]]
    assert n["heads_max"] == [float(h.abs().max()) for h in hs]
    ops.check_weight_range(n, "site")
    W[0][3, 2] = 1e6                      # a narrow block's weight stays fp32
    ops.check_weight_range(norms(), "site")
    for M, what in ((W[0], "input block 0 of the first layer"), (W[1], "layer 2"), (W[2], "layer 3"), (hs[1], "head 1")):
        old = float(M[5, 9])
        M[5, 9] = K.BELOW
        ops.check_weight_range(norms(), "site")
        for bad in (-K.END, 1e5, float("inf")):
            M[5, 9] = bad
            with pytest.raises(ValueError, match=rf"some\.site: {what} .*bf16x6"):
                ops.check_weight_range(norms(), "some.site")
        M[5, 9] = old
