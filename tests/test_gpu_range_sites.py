"""The fp16 range flags of the "f16x3" launches, site by site (tests/range_cases.py; the CPU half is tests/test_range_ref.py).  The flag
is the only thing between a clipped value and a silently wrong result, and the model-level range tests raise dozens of sites at once:
a tracker missing at ONE conversion site goes unnoticed there.  Here every case raises one site (or none), and for every launch:

- the case's conditions are asserted on the fp64 reference first (planted site >= 1e5, every other site <= 16 376);
- the launch runs inside its own ops.RangeFlags with a site name of its own; the kernel code (and the launch shape, where one is
  meant) is asserted; `flags.take()` is exactly [that name] or [] as `fwd_ref.expected_flag` of the reference says;
- the twin launch (the plant removed) reports [], and where the large value meets zero weights the planted launch's rows / heads /
  aggregate equal the twin's bit for bit;
- the same launch in "bf16x6" reports [] and its rows match the fp64 reference by `assert_as_accurate_as_fp32`: the plants are legal
  data for the exact-range arithmetic.  (ops.mp_layer_forward is f16x3 only: its two halves run as two bf16x6 launches;
  ops.mlp_forward_precomputed has no bf16x6 form at all.)
- every test states the matrix lines it must hit — (kernel code, launch form, site) — and `_matrix_lines` compares.

All launches are uncertified (no Source(bound=)): tracked instantiations.  With G4C_RANGE_SITES_REPORT=<path> what was read is
written there (tests/RANGE_SITES_MEASURED.md)."""
import os
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

import range_cases as K                                                                          # noqa: E402
from graphs4cfd_amd import _lib, ops, plan                                                       # noqa: E402
from oracle import fwd_ref as R                                                                  # noqa: E402
from test_gpu_fwd_ref import ACT, DEEP, K_BX6, K_WS, RING, switches                              # noqa: E402

DEV = torch.device("cuda", 0)
F32, F64 = torch.float32, torch.float64
H = 128
K_PRE = _lib.KERNEL_MLP_WS_PRE
GENERIC = _lib.TILE_SHAPE_GENERIC
SHAPES = {"node": _lib.TILE_SHAPE_NODE, "up": _lib.TILE_SHAPE_UP, "down": _lib.TILE_SHAPE_DOWN}
FORMS = (("ring", RING), ("deep", DEEP))
HIT = set()              # (kernel code, launch form, site) of every planted / control launch whose kernel code and flag were asserted
LINES = {}
REPORT = []              # (kernel form, launch form, site, level, planted max, largest other-site max, flag read, note)
_serial = [0]


def lines(fn):
    def deco(test):
        LINES[test.__name__] = fn
        return test
    return deco


def lines_of(code, groups, prefix=""):
    return {(code, prefix + c.form, c.site) for g in groups for c in K.catalogue(g)}


@pytest.fixture(autouse=True)
def _matrix_lines(request):
    before = set(HIT)
    HIT.clear()
    yield
    got = set(HIT)
    HIT.clear(); HIT.update(before | got)
    want = LINES[request.node.originalname](**getattr(getattr(request.node, "callspec", None), "params", {}))
    assert got == want, f"matrix lines missing {sorted(want - got, key=str)}, unexpected {sorted(got - want, key=str)}"


@pytest.fixture(autouse=True)
def _inference():
    with torch.no_grad():
        yield


@pytest.fixture(scope="module", autouse=True)
def _report():
    del REPORT[:]
    yield
    path = os.environ.get("G4C_RANGE_SITES_REPORT")
    if path:
        rows = {}
        for kf, form, site, level, planted, worst, flag, note in REPORT:
            r = rows.setdefault((kf, form, str(site), level, note), [float("inf"), 0.0, set(), 0])
            r[0], r[1], r[3] = min(r[0], planted if planted is not None else float("inf")), max(r[1], worst), r[3] + 1
            r[2].add(flag)
        with open(path, "w") as f:
            f.write("| kernel form | launch form | site | level | launches | planted max (smallest) | largest other-site max | flag read |\n|---|---|---|---|---|---|---|---|\n")
            for (kf, form, site, level, note), (pm, wm, flags, cnt) in sorted(rows.items()):
                pm = "-" if site == "None" else f"{pm:.4g}"
                f.write(f"| {kf} | {form} | {site} | {level}{' ' + note if note else ''} | {cnt} | {pm} | {wm:.4g} | {' / '.join(sorted(flags))} |\n")


def site_name(what):
    _serial[0] += 1
    return f"range_sites.{what}.{_serial[0]}"


# ---------------------------------------------------------------------------------------------------------------- a case on the device
def csr_of_deg(deg):
    c = plan.build_csr(torch.arange(int(deg.numel())).repeat_interleave(deg), int(deg.numel()), DEV)
    assert c.perm is None
    return c


def sources(c):
    out = []
    for b in c.blks:
        csr = None
        if b.keys is not None:
            csr = plan.build_csr(b.keys, b.n_seg + (1 if b.drops() else 0), DEV, drop_last_segment=b.drops())
            off, perm = b.segments()          # (the reference groups the rows as the plan does)
            assert torch.equal(csr.off.cpu().long(), off) and (perm is None) == (csr.perm is None)
            assert perm is None or torch.equal(csr.perm.cpu().long(), perm)
        out.append(ops.Source(b.x.to(DEV), None if b.index is None else b.index.to(DEV, torch.int32), b.col0, b.w(), b.negate, ACT[b.pre_act],
                              b.additive, csr, b.mean))
    return out


def pack(c, prec, name):
    wide = [b for b in c.blks if not b.additive] if c.first is None else [K.Blk(c.first)]
    ln = None if c.ln is None else (c.ln[0].to(DEV), c.ln[1].to(DEV), R.LN_EPS)
    return ops.PackedMLP([w.to(DEV) for w in c.W], [b.to(DEV) for b in c.b], ln, [b.w() for b in wide], [b.negate for b in wide],
                         [h.to(DEV) for h in c.heads], precision=prec, narrow=[b.narrow for b in wide] if any(b.narrow for b in wide) else None,
                         site=name)


def same_weights(a, b):
    def flat(c):
        return list(c.W) + list(c.b) + list(c.ln or ()) + list(c.heads)
    if a.msg is not None:
        return same_weights(a.msg, b.msg) and same_weights(a.upd, b.upd)
    return all(torch.equal(x, y) for x, y in zip(flat(a), flat(b)))


def run(c, prec, sw, packs=None):
    """One launch of the case under the switches `sw` inside a RangeFlags scope of its own: rows (through out_idx: the whole output
    tensor), heads, aggregate, the flags read, the kernel code and launch shape, the site names, the packed images."""
    what = c.form.replace(" ", "_")
    with switches(prec, sw.get("ws", 0), 0, sw.get("small")) as lib:
        old_shapes = lib.g4c_mlp_shapes_enable(sw.get("shapes", -1))
        try:
            if c.msg is not None:          # ops.mp_layer_forward
                names = (site_name(what + ".msg"), site_name(what + ".upd")) if packs is None else (packs[0].site, packs[1].site)
                pm, pu = packs or (pack(c.msg, prec, names[0]), pack(c.upd, prec, names[1]))
                csr = csr_of_deg(c.msg.agg_deg)
                heads = [torch.full((c.upd.n, H), float("nan"), device=DEV) for _ in c.upd.heads] or None
                with ops.RangeFlags(DEV) as flags:
                    e, v, _ = ops.mp_layer_forward(pm, sources(c.msg), c.msg.n, csr, c.msg.agg_mean, pu, c.upd.blks[1].x.to(DEV), ACT[c.upd.act],
                                                   store_rows=c.msg.store_rows, head_outs=heads)
                    kernel, shape = int(lib.g4c_mlp_last_kernel()), int(lib.g4c_mlp_last_shape())
                return SimpleNamespace(rows=v, e=e, heads=heads, agg=None, flags=flags.take(), kernel=kernel, shape=shape, names=names, packs=(pm, pu))
            name = site_name(what) if packs is None else packs[0].site
            pk = packs[0] if packs else pack(c, prec, name)
            agg = agg_out = None
            if c.agg_deg is not None:
                agg_out = torch.full((int(c.agg_deg.numel()), H), float("nan"), device=DEV)
                agg = (csr_of_deg(c.agg_deg), agg_out, c.agg_mean)
            with ops.RangeFlags(DEV) as flags:
                if c.first is not None:          # ops.mlp_forward_precomputed
                    adds = [ops.Source(b.x.to(DEV), b.index.to(DEV, torch.int32), additive=True) for b in c.blks]
                    y, heads = ops.mlp_forward_precomputed(pk, c.first.to(DEV), adds, c.n, agg, ACT[c.act], store_rows=c.store_rows), None
                else:
                    heads = [torch.full((c.n, H), float("nan"), device=DEV) for _ in c.heads] or None
                    y = ops.mlp_forward(pk, sources(c), c.n, ACT[c.act], out=None if c.out_idx is None else c.out_init.to(DEV).clone(),
                                        out_idx32=None if c.out_idx is None else c.out_idx.to(DEV, torch.int32),
                                        resid=None if c.resid is None else c.resid.to(DEV), resid_col0=c.resid_col0, head_outs=heads, agg=agg,
                                        store_rows=c.store_rows)
                kernel, shape = int(lib.g4c_mlp_last_kernel()), int(lib.g4c_mlp_last_shape())
            return SimpleNamespace(rows=y, e=None, heads=heads, agg=agg_out, flags=flags.take(), kernel=kernel, shape=shape, names=(name,), packs=(pk,))
        finally:
            lib.g4c_mlp_shapes_enable(old_shapes)


def written(c, o):
    """Every tensor the launch wrote, by name."""
    out = {}
    if o.rows is not None:
        out["rows"] = o.rows
    if o.e is not None:
        out["e"] = o.e
    if o.agg is not None:
        out["agg"] = o.agg
    for j, h in enumerate(o.heads or ()):
        out[f"head{j}"] = h
    return out


def expected_names(c, o):
    if not c.expect:
        return []
    return [o.names[1 if (c.msg is not None and c.site.startswith("upd.")) else 0]]


def accurate(what, got, ref, cmp32):
    R.assert_as_accurate_as_fp32(got.cpu(), ref, cmp32, None, what)


def exact_range(c, sw):
    """The case in "bf16x6": no flag, and what it wrote matches the fp64 reference as accurately as a plain fp32 evaluation does."""
    if c.first is not None:
        return          # (no bf16x6 form: ops.mlp_forward_precomputed is an f16x3 launch)
    if c.msg is not None:          # the two halves as two launches: the message launch with its aggregate, the node launch on [aggregate | v]
        m = c.msg
        o = run(m, "bf16x6", {})
        assert o.flags == []
        L = m.launch()
        ref, c32 = R.ref64(L)["y"], R.evaluate(L, F32)["y"]
        full = m.agg_deg > 0
        if m.store_rows:
            accurate(f"{c.name} bf16x6 e'", o.rows, ref, c32)
        accurate(f"{c.name} bf16x6 aggregate", o.agg[full.to(DEV)], R._segment(ref, m.agg_off(), None, m.agg_mean)[full],
                 R._segment(c32, m.agg_off(), None, m.agg_mean)[full])
        u = K._dc(c.upd)
        u.blks[0].x = o.agg.cpu()          # (the node launch's reference starts from the aggregate it read)
        c, sw = u, {}
    o = run(c, "bf16x6", sw)
    assert o.flags == [], (c.name, o.flags)
    L = c.launch()
    ref, c32 = R.ref64(L), R.evaluate(L, F32)
    if o.rows is not None:
        y = o.rows if c.out_idx is None else o.rows[c.out_idx.to(DEV)]
        accurate(f"{c.name} bf16x6 rows", y, ref["y"], c32["y"])
    elif o.agg is not None:
        full = c.agg_deg > 0
        accurate(f"{c.name} bf16x6 aggregate", o.agg[full.to(DEV)], R._segment(ref["y"], c.agg_off(), None, c.agg_mean)[full],
                 R._segment(c32["y"], c.agg_off(), None, c.agg_mean)[full])


def pin(c, kernel_form, code, sw, shape=None, prefix="", exact=True):
    """The planted (or control) case and its twin in f16x3, then the case in bf16x6."""
    planted, worst = K.conditions(c)
    assert R.expected_flag(c.sites()) == c.expect
    o = run(c, "f16x3", sw)
    assert o.kernel == code, f"{c.name}: kernel {_lib.KERNEL_NAMES.get(o.kernel)} ({o.kernel}) ran, expected code {code}"
    if shape is not None:
        assert o.shape == shape, (c.name, o.shape, shape)
    note = ""
    if c.level.startswith("huge"):
        fin = all(bool(torch.isfinite(t).all()) for t in written(c, o).values())
        note = "rows finite" if fin else "rows NOT finite"
    if c.level == "threshold":
        note = c.name.split("threshold ")[1].split(" ", 1)[1]
    REPORT.append((kernel_form, c.form, c.site, c.level, planted, worst, "set" if o.flags else "clear", note))
    assert o.flags == expected_names(c, o), f"{c.name}: flags {o.flags}, expected {expected_names(c, o)} (planted maximum {planted}, others {worst})"
    HIT.add((code, prefix + c.form, c.site))
    if c.twin is not None:
        K.conditions(c.twin)
        t = run(c.twin, "f16x3", sw, o.packs if same_weights(c, c.twin) else None)
        assert t.kernel == code and t.flags == [], f"{c.name}: the twin launch reports {t.flags}"
        a, b = written(c, o), written(c.twin, t)
        assert a.keys() == b.keys()
        if c.bit_equal is True:
            if not c.level.startswith("huge") or c.level == "huge:1e30":
                assert all(bool(torch.isfinite(x).all()) for x in a.values()), c.name
            for k in a:
                x, y = a[k], b[k]
                if k == "rows" and c.out_idx is not None:          # rows no index names keep what they held; the named ones are compared
                    kept = torch.ones(int(x.size(0)), dtype=torch.bool, device=DEV)
                    kept[c.out_idx.to(DEV)] = False
                    assert torch.equal(x[kept], c.out_init.to(DEV)[kept]) and torch.equal(y[kept], c.twin.out_init.to(DEV)[kept]), c.name
                    x, y = x[~kept], y[~kept]
                if k == "rows" and c.resid is not None:            # (read and added in fp32 after everything else: one rounding)
                    w = slice(c.resid_col0, c.resid_col0 + H)
                    y = y + (c.resid[:, w] - c.twin.resid[:, w]).to(DEV)
                assert torch.equal(x, y), f"{c.name}: {k} differs from the twin launch's"
        elif c.bit_equal == "heads":
            assert all(torch.equal(a[k], b[k]) for k in a if k.startswith("head")), f"{c.name}: the heads differ from the twin launch's"
    if exact and not (c.level.startswith("huge") and c.level != "huge:1e30"):
        exact_range(c, {k: v for k, v in sw.items() if k == "small"})
    return o


# ====================================================================== the tile kernel, ring and deep
TILE_GROUPS = ("node", "window", "agg_on_load", "message_tile", "threshold", "selu_sign", "unread", "huge")


@lines(lambda form, group: lines_of(K_BX6, [group], f"bx6:{form[0]}:"))
@pytest.mark.parametrize("group", TILE_GROUPS)
@pytest.mark.parametrize("form", FORMS, ids=lambda f: f[0])
def test_tile_kernel_sites(form, group):
    """mlp_bx6_kernel in both ring forms.  node: three layers, two heads (in0, in1, h1, h2, heads); window: the vec and unaligned source
    paths; agg_on_load: ordered / seg_perm x sum / mean x pending SELU; message_tile: the fused aggregation on ragged tiles of whole
    segments, rows stored and not; the threshold triple, the SELU sign, unread data and huge inputs.  (The second block of these node
    launches is gathered: no compile-time shape.)"""
    for c in K.catalogue(group):
        pin(c, f"tile:{form[0]}", K_BX6, dict(small=form[1]), shape=GENERIC, prefix=f"bx6:{form[0]}:")


@lines(lambda: lines_of(K_BX6, ["shapes"]))
def test_tile_kernel_compile_time_shapes():
    """The node-update shapes (2 / 3 layers x 0 / 2 heads), UpMP's and DownMP's: every site of each, and the same flag from the
    all-runtime kernel (g4c_mlp_shapes_enable(0))."""
    for c in K.catalogue("shapes"):
        kind = c.form.split(":")[1]
        o = pin(c, f"tile:shape:{kind}", K_BX6, dict(small=RING, shapes=1), shape=SHAPES[kind])
        g = run(c, "f16x3", dict(small=RING, shapes=0), o.packs)
        assert (g.kernel, g.shape) == (K_BX6, GENERIC) and g.flags == o.flags, (c.name, g.flags, o.flags)
        assert all(torch.equal(x, y) for x, y in zip(written(c, o).values(), written(c, g).values())), c.name


# ====================================================================== mlp_ws_kernel
WS_GROUPS = ("ws", "threshold_ws", "selu_sign_ws", "huge_ws")


@lines(lambda group: lines_of(K_WS, [group]))
@pytest.mark.parametrize("group", WS_GROUPS)
def test_ws_kernel_sites(group):
    """The hoisted message form (SELU on load, two additive blocks; and without the SELU: in0 with both signs), two and three layers,
    1 / 64 / 65 / 130 rows, with and without the fused aggregation (ragged: the general form; uniform degree 6: the dense form), rows
    stored and not stored: in0, h1 through the weighted block and through each additive table, h2."""
    for c in K.catalogue(group):
        pin(c, "ws", K_WS, dict(ws=2))


@lines(lambda group: lines_of(K_WS, [group]))
@pytest.mark.parametrize("group", ["mp_layer", "huge_mp"])
def test_fused_mp_layer_sites(group):
    """ops.mp_layer_forward: every msg.* and upd.* site, 0 and 2 heads, two and three layers.  A message-phase plant sets the message
    MLP's name and not the node MLP's; a node-phase plant the reverse (`expected_names`).  upd.in0 — the aggregate, which exists only
    inside the launch — is raised by a sum of LayerNorm'd rows; under a mean the same rows must not flag."""
    for c in K.catalogue(group):
        pin(c, "ws:mp_layer", K_WS, dict(ws=2))


@lines(lambda: lines_of(K_PRE, ["precomputed"]))
def test_static_first_layer_sites():
    """ops.mlp_forward_precomputed: h1 planted in `first`, in p0 and in p1; h2."""
    for c in K.catalogue("precomputed"):
        pin(c, "ws:precomputed", K_PRE, {})


# ====================================================================== weights beyond the fp16 range
def weight_case(where, value):
    """Mix "C" rows through a three-layer 128-wide MLP with two heads; one weight = `value`, and what it multiplies scaled to ~1e-2, so
    that every ACTIVATION stays far inside the range (at most 1e5 x 0.03 in the pre-activation it feeds)."""
    c = K.node_case(65, 950, layers=3, n_heads=2)
    if where == "W0":
        c.blks[0].x[:, 70] = 0.01 * K.table(65, 1, 951)[:, 0]
    elif where == "W1":
        c.W[0][70] *= 1e-3
        c.b[0][70] = 1e-3
    else:
        c.ln[0][70] = c.ln[1][70] = 1e-3
    {"W0": c.W[0], "W1": c.W[1], "head": c.heads[0]}[where][37, 70] = value
    c.name, c.form = f"weight {where}[37, 70]={value:g}", f"weights:{where}"
    return c


@lines(lambda where: {(K_BX6, f"weights:{where}", None)})
@pytest.mark.parametrize("where", ["W0", "W1", "head"])
def test_a_weight_beyond_the_fp16_range(where):
    """The weights of an f16x3 image are converted to fp16 when it is packed, unclipped (tests/RANGE_SITES_MEASURED.md: from |w| = 65520
    on, a first-layer or hidden-layer weight gave rows wrong by ~6 under a flag that names no cause, a head weight gave head rows of
    3.4e38 and NO flag).  Such an image is refused when it is packed; 6.5e4 still packs and matches the fp64 reference (on these rows no
    activation leaves the range: no flag); the refused weights run in "bf16x6"."""
    big = weight_case(where, 1e5)
    with pytest.raises(ValueError, match=r"weights\.big.*(first layer|layer 2|head 0).*bf16x6"):
        pack(big, "f16x3", "weights.big")
    exact_range(big, {})
    c = weight_case(where, 6.5e4)
    planted, worst = K.conditions(c)          # (every site inside a quarter of the range)
    o = run(c, "f16x3", {})
    assert o.kernel == K_BX6 and o.flags == [], (c.name, o.flags)
    HIT.add((K_BX6, c.form, None))
    L = c.launch()
    accurate(f"{c.name} rows", o.rows, R.ref64(L)["y"], R.evaluate(L, F32)["y"])
    for j, h in enumerate(o.heads):
        accurate(f"{c.name} head{j}", h, R.heads(o.rows.cpu(), c.heads)[j], R.heads(o.rows.cpu(), c.heads, F32)[j])
