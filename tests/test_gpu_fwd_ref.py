"""Every default-precision inference launch against fp64 references of its own (oracle/fwd_ref.py): each case sets the switches it
depends on (arithmetic, g4c_mlp_ws_enable, g4c_mlp_bx6i_enable, g4c_mlp_small_launch_tiles, a Source(bound=) certificate) and restores
them, asserts which kernel ran (g4c_mlp_last_kernel) and checks EVERY tensor the launch wrote:

- output rows, heads, aggregates that are not promised bit for bit: `assert_as_accurate_as_fp32` — per row class (ordinary / large /
  small input rows) the max and mean error against fp64 within 2.0 x + 1e-6 / 1.5 x + 1e-7 of the error of a plain torch float32
  evaluation of the same formula (the comparator, run on the device; a reference-side quantity).  Where a launch stores an intermediate
  (the output rows under its heads, e' under the MP layer's aggregate, v' under its heads) the next stage's reference starts from
  the launch's own fp32 tensor; with store_rows=False the reference runs end to end;
- the fused aggregate of stored rows: torch.equal with the launch's own rows added in fp32 one after the other on the host, `/ count`
  for the mean; rows of an output tensor that no output index names: torch.equal with what they held (they are not part of any
  statistic, and neither are the zero rows of empty segments);
- every test states the matrix lines it must hit — (kernel code, case label, arithmetic) — and the `_matrix_lines` fixture compares
  them with what its launches asserted;
- the range flags of every tracked f16x3 launch stay clear (nothing here clips: the range tests own clipping).

One negative control per kernel family: the launch's correct output is rejected against a perturbed reference.  Nothing perturbs a
launch.  With G4C_FWD_REF_REPORT=<path> the ratios of every check are written there as a table (tests/FWD_REF_MEASURED.md)."""
import contextlib
import os
import sys
from dataclasses import dataclass
from typing import Optional

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
pytestmark = pytest.mark.gpu

from graphs4cfd_amd import _lib, ops, plan          # noqa: E402
from oracle import fwd_ref as R                      # noqa: E402

DEV = torch.device("cuda", 0)
F32, F64 = torch.float32, torch.float64
H = 128
ACT = {None: _lib.ACT_NONE, "selu": _lib.ACT_SELU, "tanh": _lib.ACT_TANH}
K_SPLIT, K_BX6, K_BX6I, K_WS, K_BX6_CERT, K_WS_CERT = 1, _lib.KERNEL_MLP_BX6, 3, _lib.KERNEL_MLP_WS, _lib.KERNEL_MLP_BX6_CERT, _lib.KERNEL_MLP_WS_CERT
RING, DEEP = 0, 1 << 30          # g4c_mlp_small_launch_tiles: no launch / every launch takes the deep-ring form
MIXES = ("A", "B", "C")
WSETS = {"A": ("default", "ln"), "B": ("ln", "default"), "C": ("x64", "ln")}      # (x64 with the mix that keeps it inside fp16's range)
HIT = set()          # (kernel code, case label, arithmetic) of every launch whose kernel code was asserted
LINES = {}           # test function -> (its parameters -> the lines it must hit); filled next to each test (`lines`)


def lines(fn):
    """Decorator: `fn(**parameters)` gives the set of (kernel code, case label, arithmetic) the decorated test must hit."""
    def deco(test):
        LINES[test.__name__] = fn
        return test
    return deco


@pytest.fixture(autouse=True)
def _matrix_lines(request):
    """Every test hits exactly the matrix lines it states, whatever else of this file runs with it and in whatever order."""
    before = set(HIT)
    HIT.clear()
    yield
    got = set(HIT)
    HIT.clear(); HIT.update(before | got)
    want = LINES[request.node.originalname](**getattr(getattr(request.node, "callspec", None), "params", {}))
    assert got == want, f"matrix lines missing {sorted(want - got)}, unexpected {sorted(got - want)}"


@pytest.fixture(autouse=True)
def _inference():
    with torch.no_grad():
        yield


@pytest.fixture(scope="module", autouse=True)
def _report():
    # the comparator is an fp32 evaluation: no TF32, no reduced-precision matmul
    assert torch.backends.cuda.matmul.allow_tf32 is False and torch.get_float32_matmul_precision() == "highest"
    del R.STATS[:]
    yield
    path = os.environ.get("G4C_FWD_REF_REPORT")
    if path:
        with open(path, "w") as f:
            f.write("| case / output | row class | max err | mean err | max / allowed | mean / allowed |\n|---|---|---|---|---|---|\n")
            for what, cls, mx, mean, rmax, rmean in R.STATS:
                if what.endswith("CONTROL"):          # (the negative controls: rejected on purpose)
                    continue
                f.write(f"| {what} | {cls} | {mx:.2e} | {mean:.2e} | {rmax:.3f} | {rmean:.3f} |\n")


@contextlib.contextmanager
def switches(prec, ws=0, bx6i=0, small=None):
    """Arithmetic + kernel selection for one case; everything restored.  `small` None leaves g4c_mlp_small_launch_tiles as shipped."""
    lib = _lib.load()
    old = (ops.set_mlp_precision(prec), lib.g4c_mlp_ws_enable(ws), lib.g4c_mlp_bx6i_enable(bx6i), lib.g4c_mlp_small_launch_tiles(-1))
    if small is not None:
        lib.g4c_mlp_small_launch_tiles(small)
    try:
        yield lib
    finally:
        ops.set_mlp_precision(old[0]); lib.g4c_mlp_ws_enable(old[1]); lib.g4c_mlp_bx6i_enable(old[2]); lib.g4c_mlp_small_launch_tiles(old[3])


def _gen(seed):
    return torch.Generator().manual_seed(seed)


@dataclass
class Blk:
    """One input block, as the launch (ops.Source) and as the reference (fwd_ref.Src / Add) see it."""
    x: torch.Tensor
    index: Optional[torch.Tensor] = None          # int64 on the device
    col0: int = 0
    width: Optional[int] = None
    negate: bool = False
    pre_act: Optional[str] = None
    csr: Optional[plan.CsrPlan] = None
    mean: bool = True
    narrow: bool = False
    additive: bool = False
    bound: Optional[float] = None

    def w(self):
        return int(self.x.size(1)) - self.col0 if self.width is None else self.width

    def source(self, certify):
        b = None
        if certify:          # a TRUE bound of the stored values this source reads
            b = float(self.x[:, self.col0:self.col0 + self.w()].abs().max())
        return ops.Source(self.x, None if self.index is None else self.index.to(torch.int32), self.col0, self.w(), self.negate,
                          ACT[self.pre_act], self.additive, self.csr, self.mean, bound=b)

    def ref(self):
        if self.additive:
            return R.Add(self.x, self.index, self.col0)
        seg = None if self.csr is None else (self.csr.off, self.csr.perm)
        return R.Src(self.x, self.index, self.col0, self.w(), self.negate, self.pre_act, seg, self.mean)

    def vec(self):
        return self.w() % 4 == 0 and self.x.stride(0) % 4 == 0 and self.col0 % 4 == 0 and self.x.data_ptr() % 16 == 0


@dataclass
class Net:
    W: list
    b: list
    ln: Optional[tuple]
    heads: list

    def pack(self, blks, prec, heads=False):
        wide = [b for b in blks if not b.additive]
        ln = None if self.ln is None else (self.ln[0], self.ln[1], R.LN_EPS)
        return ops.PackedMLP(self.W, self.b, ln, [b.w() for b in wide], [b.negate for b in wide], self.heads if heads else (), precision=prec,
                             narrow=[b.narrow for b in wide] if any(b.narrow for b in wide) else None, site="fwd_ref")


def net(k_in, widths, seed, ln=True, wset="default", n_heads=0):
    Ws, bs, lnp, hs = R.default_weights(k_in, widths, _gen(seed), ln, wset, n_heads)
    return Net([w.to(DEV) for w in Ws], [b.to(DEV) for b in bs], None if lnp is None else (lnp[0].to(DEV), lnp[1].to(DEV)), [h.to(DEV) for h in hs])


def rows_of(n, width, mix, seed):
    return R.mixed_rows(n, width, mix, _gen(seed)).to(DEV)


def table(n, width, seed):
    return torch.randn(n, width, generator=_gen(seed)).to(DEV)


def index(n, hi, seed):
    return torch.randint(0, hi, (n,), generator=_gen(seed)).to(DEV)


def csr_of(deg, shuffle_seed=None):
    """A plan over segments of `deg` rows each; `shuffle_seed`: the rows arrive in random order (the plan has a permutation)."""
    keys = torch.arange(int(deg.numel())).repeat_interleave(deg)
    if shuffle_seed is not None:
        keys = keys[torch.randperm(int(keys.numel()), generator=_gen(shuffle_seed))]
    c = plan.build_csr(keys, int(deg.numel()), DEV)
    assert (c.perm is not None) == (shuffle_seed is not None and int(keys.numel()) > 1)
    return c


def ragged_degrees(n, seed, hi=10):
    """Empty segments at both ends and in runs, one segment of exactly 32 rows."""
    deg = torch.randint(0, hi, (n,), generator=_gen(seed))
    if n >= 40:
        deg[:3] = 0; deg[-2:] = 0; deg[10:17] = 0; deg[20] = 32
    return deg


def check(what, got, ref, cmp32, classes, agrees=False):
    if agrees:          # (LayerNorm'd rows: O(1) outputs, no cancellation between large terms behind them)
        R.comparator_agrees(ref, cmp32, what)
    return R.assert_as_accurate_as_fp32(got, ref, cmp32, classes, what)


def launch(what, prec, nt, blks, n_rows, classes, expect, *, act=None, heads=False, agg=None, store_rows=True, out_rows=None,
           out_idx=None, resid=None, resid_col0=0, certify=False, ws=0, bx6i=0, small=None, control=None):
    """One ops.mlp_forward launch under its switches, the asserted kernel code, and every tensor it wrote against the references.
    `agg` = (csr, mean).  `control`: Launch -> perturbed Launch; the correct rows must be rejected against its reference."""
    n_out = int(nt.W[-1].size(0))
    out = out_init = None
    if out_idx is not None:
        out_init = table(out_rows, n_out, 77)
        out = out_init.clone()
    L = R.Launch([b.ref() for b in blks if not b.additive], nt.W, nt.b, nt.ln, act, [b.ref() for b in blks if b.additive], resid, resid_col0,
                 out_idx, out_init)
    with switches(prec, ws, bx6i, small) as lib:
        pk = nt.pack(blks, prec, heads)
        head_outs = [torch.full((n_rows, H), float("nan"), device=DEV) for _ in nt.heads] if heads else None
        agg_out = torch.full((agg[0].n_seg, H), float("nan"), device=DEV) if agg else None
        with ops.RangeFlags(DEV) as flags:
            y = ops.mlp_forward(pk, [b.source(certify) for b in blks], n_rows, ACT[act], out=out,
                                out_idx32=None if out_idx is None else out_idx.to(torch.int32), resid=resid, resid_col0=resid_col0,
                                head_outs=head_outs, agg=None if agg is None else (agg[0], agg_out, agg[1]), store_rows=store_rows)
            ran = int(lib.g4c_mlp_last_kernel())
        assert ran == expect, f"{what}: kernel {_lib.KERNEL_NAMES.get(ran)} ({ran}) ran, expected code {expect}"
        if prec == "f16x3":
            assert flags.take() == [], f"{what}: a range flag is set"
    HIT.add((expect, what.split(" ")[0], prec))
    ref, c32 = R.ref64(L), R.evaluate(L, F32)
    ratios = {}
    if store_rows:
        assert y is not None and torch.isfinite(y).all()
        if out_idx is not None:          # rows no index names keep what they held, bit for bit; the statistics see the written rows only
            kept = torch.ones(out_rows, dtype=torch.bool, device=DEV)
            kept[out_idx] = False
            assert torch.equal(y[kept], out_init[kept]), f"{what}: a row that out_idx does not name changed"
            y = y[out_idx]
        ratios["rows"] = check(f"{what} rows", y, ref["y"], c32["y"], classes, agrees=nt.ln is not None and resid is None)
        if callable(control):
            Lp = control(L)
            assert R.rejects(R.assert_as_accurate_as_fp32, y, R.ref64(Lp)["y"], R.evaluate(Lp, F32)["y"], classes, f"{what} CONTROL")
    else:
        assert y is None
    if heads:
        for j, h in enumerate(head_outs):
            ratios[f"head{j}"] = check(f"{what} head{j}", h, R.heads(y, nt.heads)[j], R.heads(y, nt.heads, F32)[j], classes)
            if control == "head":
                z = ref["z"]
                assert R.rejects(R.assert_as_accurate_as_fp32, h, R.heads(z, nt.heads)[j], R.heads(z.float(), nt.heads, F32)[j], classes,
                                 f"{what} head{j} CONTROL")
    if agg:
        csr, mean = agg
        if store_rows:          # the header's promise: the segment reduction of the stored rows, the IEEE quotient for the mean
            want = R.segment_reduce_fp32(y.cpu(), csr.off.cpu(), mean)
            assert torch.equal(agg_out.cpu(), want), f"{what}: fused aggregate is not the fp32 segment reduction of the stored rows"
            moved = R.segment_reduce_fp32(y.cpu(), R.move_boundary(csr.off.cpu(), int(csr.n_seg) // 2), mean)
            assert not torch.equal(agg_out.cpu(), moved)
        else:
            full = (csr.off[1:] > csr.off[:-1]).to(DEV)          # empty segments: exactly zero, and no part of the statistics
            assert torch.equal(agg_out[~full], torch.zeros_like(agg_out[~full])), f"{what}: the aggregate of an empty segment is not 0"
            seg_cls = {k: m[full] for k, m in R.classes_of_segments(classes, csr.off).items()}
            ratios["agg"] = check(f"{what} agg", agg_out[full], R._segment(ref["y"], csr.off, None, mean)[full],
                                  R._segment(c32["y"], csr.off, None, mean)[full], seg_cls)
    return y, ratios


def node_blocks(n, mix, seed, path="full"):
    """The node form [mixed rows | a gathered N(0, 1) table] in the three source paths of mlp_bx6_kernel."""
    a = rows_of(n, H, mix, seed)
    if path == "full":          # every block 128 wide and 16-byte addressable
        blks = [Blk(a), Blk(table(max(n // 2, 1), H, seed + 1), index=index(n, max(n // 2, 1), seed + 2))]
    elif path == "vec":         # aligned, not all 128 wide: a 64-wide window at column 4 of a 72-wide tensor
        blks = [Blk(a), Blk(table(n, 72, seed + 1), col0=4, width=64)]
    else:                       # unaligned: a 37-wide window at column 3 of a 45-wide tensor (odd col0 and ld)
        blks = [Blk(a), Blk(table(n, 45, seed + 1), col0=3, width=37)]
    assert all(b.vec() for b in blks) == (path != "unaligned")
    return blks


def message_blocks(n_rows, n_nodes, mix, seed, adds=True, indexed=False, pre_act="selu"):
    """The hoisted message form: e (mixed rows, SELU on load) + two gathered product tables."""
    if indexed:
        e = rows_of(max(n_rows // 2, 1), H, mix, seed)
        ix = index(n_rows, int(e.size(0)), seed + 5)
        blks, cls = [Blk(e, index=ix, pre_act=pre_act)], R.classes_through(R.row_classes(int(e.size(0)), DEV), ix)
    else:
        blks, cls = [Blk(rows_of(n_rows, H, mix, seed), pre_act=pre_act)], R.row_classes(n_rows, DEV)
    if adds:
        blks += [Blk(table(n_nodes, H, seed + 1), index=index(n_rows, n_nodes, seed + 2), additive=True),
                 Blk(table(n_nodes, H, seed + 3), index=index(n_rows, n_nodes, seed + 4), additive=True)]
    return blks, cls


PRECS = ("f16x3", "bf16x6")
FORMS = (("ring", RING), ("deep", DEEP))


# ====================================================================== MLP_SPLIT (fp32)
@lines(lambda path, n: {(K_SPLIT, f"split:{path}", "fp32")})
@pytest.mark.parametrize("path", ["vec", "unaligned"])
@pytest.mark.parametrize("n", [1, 33, 2047])
def test_split_kernel(path, n):
    mix = MIXES[n % 3]
    blks = node_blocks(n, mix, 10 + n, path)
    nt = net(sum(b.w() for b in blks), (H, H, H), 11, True, WSETS[mix][0], n_heads=2)
    launch(f"split:{path} n={n} mix={mix}", "fp32", nt, blks, n, R.row_classes(n, DEV), K_SPLIT, act="selu", heads=True,
           control=(lambda L: R.swap_adjacent_columns(L, 40)) if n == 2047 else None)


# ====================================================================== MLP_BX6: the tile kernel, ring and deep
@lines(lambda path, prec, form: {(K_BX6, f"bx6:{form[0]}:{path}", prec)})
@pytest.mark.parametrize("form", FORMS, ids=lambda f: f[0])
@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("path", ["full", "vec", "unaligned"])
def test_bx6_source_paths_and_row_counts(path, prec, form):
    """The three source paths at every boundary row count (a grid of one tile per 32 rows: 1 .. 65 end inside, at and behind a tile)."""
    for i, n in enumerate((1, 31, 32, 33, 63, 64, 65, 2047)):
        mix = MIXES[i % 3]
        blks = node_blocks(n, mix, 20 + n, path)
        nt = net(sum(b.w() for b in blks), (H, H, H), 21 + i, True, WSETS[mix][i % 2])
        launch(f"bx6:{form[0]}:{path} {prec} n={n} mix={mix}", prec, nt, blks, n, R.row_classes(n, DEV), K_BX6, small=form[1],
               control=(lambda L: R.wrong_gather_row(L, 1, 2040)) if (n == 2047 and path == "full") else None)


@lines(lambda prec, form: {(K_BX6, f"bx6:{form[0]}:depth:L{l}:ln={ln}:{a}", prec) for l in (1, 2, 3, 4) for ln in (True, False)
                    for a in (None, "selu", "tanh")} - {(K_BX6, f"bx6:{form[0]}:depth:L3:ln=True:None", prec)})
@pytest.mark.parametrize("form", FORMS, ids=lambda f: f[0])
@pytest.mark.parametrize("prec", PRECS)
def test_bx6_depth_layernorm_activation_width(prec, form):
    """1 - 4 layers, LayerNorm on and off, output activation none / SELU / tanh, n_out < 128."""
    n, i = 1000, 0
    for layers in (1, 2, 3, 4):
        for ln in (True, False):
            for act, n_out in ((None, H), ("selu", 64), ("tanh", 3)):
                if layers == 3 and ln and act is None:
                    continue          # (test_bx6_source_paths_and_row_counts)
                mix = MIXES[i % 3]; i += 1
                blks = node_blocks(n, mix, 40 + i, "full")
                nt = net(2 * H, (H,) * (layers - 1) + (n_out,), 41 + i, ln, WSETS[mix][i % 2])
                launch(f"bx6:{form[0]}:depth:L{layers}:ln={ln}:{act} {prec} n_out={n_out} mix={mix}", prec, nt, blks, n,
                       R.row_classes(n, DEV), K_BX6, act=act, small=form[1])


@lines(lambda prec, form: {(K_BX6, f"bx6:{form[0]}:{x}", prec) for x in ("heads", "out_idx", "resid", "resid-unaligned")})
@pytest.mark.parametrize("form", FORMS, ids=lambda f: f[0])
@pytest.mark.parametrize("prec", PRECS)
def test_bx6_heads_scatter_residual(prec, form):
    n = 1333
    for i, mix in enumerate(MIXES):
        blks = node_blocks(n, mix, 60 + i, "full")
        nt = net(2 * H, (H, H, H), 61 + i, True, WSETS[mix][1], n_heads=2)
        launch(f"bx6:{form[0]}:heads {prec} mix={mix}", prec, nt, blks, n, R.row_classes(n, DEV), K_BX6, act="selu", heads=True, small=form[1],
               control="head" if i == 0 else None)
        # scattered through out_idx into a larger tensor whose other rows keep what they held
        oi = torch.randperm(2 * n, generator=_gen(62 + i))[:n].to(DEV)
        launch(f"bx6:{form[0]}:out_idx {prec} mix={mix}", prec, nt, blks, n, R.row_classes(n, DEV), K_BX6, act="tanh", out_idx=oi, out_rows=2 * n, small=form[1])
        # residual: a 128-wide window at column 4 of a 140-wide tensor
        launch(f"bx6:{form[0]}:resid {prec} mix={mix}", prec, nt, blks, n, R.row_classes(n, DEV), K_BX6, act="selu", resid=table(n, 140, 63 + i),
               resid_col0=4, small=form[1])
    ub = node_blocks(n, "A", 66, "unaligned")
    nt = net(sum(b.w() for b in ub), (H, H, 64), 67, False)
    launch(f"bx6:{form[0]}:resid-unaligned {prec}", prec, nt, ub, n, R.row_classes(n, DEV), K_BX6, resid=table(n, 71, 68), resid_col0=3, small=form[1])


@lines(lambda prec, form: {(K_BX6, f"bx6:{form[0]}:agg:{m}:{st}", prec) for m in ("mean", "sum") for st in ("stored", "not-stored")})
@pytest.mark.parametrize("form", FORMS, ids=lambda f: f[0])
@pytest.mark.parametrize("prec", PRECS)
def test_bx6_fused_aggregation(prec, form):
    """The message launch on tiles of whole segments, rows stored and not stored, mean and sum, ragged and uniform degrees."""
    for i, (deg, mix) in enumerate(((ragged_degrees(400, 70), "A"), (torch.full((301,), 6), "B"), (ragged_degrees(333, 71, 33), "C"))):
        csr = csr_of(deg)
        E = csr.n
        blks, cls = message_blocks(E, 400, mix, 72 + i)
        nt = net(H, (H, H, H), 73 + i, True, WSETS[mix][i % 2])
        for mean in (True, False):
            for store in (True, False):
                launch(f"bx6:{form[0]}:agg:{'mean' if mean else 'sum'}:{'stored' if store else 'not-stored'} {prec} case={i} mix={mix}", prec, nt, blks, E, cls, K_BX6, agg=(csr, mean),
                       store_rows=store, small=form[1])


@lines(lambda prec, form: {(K_BX6, f"bx6:{form[0]}:agg_on_load:{o}:{m}", prec) for o in ("ordered", "seg_perm") for m in ("mean", "sum")})
@pytest.mark.parametrize("form", FORMS, ids=lambda f: f[0])
@pytest.mark.parametrize("prec", PRECS)
def test_bx6_aggregation_on_load(prec, form):
    """The node launch sums / averages each target's messages while it loads: rows in segment order and through seg_perm, the pending
    SELU of the stored rows applied before they are added."""
    n = 500
    deg = ragged_degrees(n, 80, 12)
    # (the sums over up to 32 rows take the mix whose sums stay inside fp16's range)
    for i, (shuffle, mean, pre, mix) in enumerate(((None, True, None, "A"), (None, False, "selu", "C"), (81, True, "selu", "B"), (82, False, None, "C"))):
        csr = csr_of(deg, shuffle)
        msgs = rows_of(csr.n, H, mix, 83 + i)
        cls = R.classes_of_segments(R.row_classes(csr.n, DEV), csr.off, csr.perm)
        blks = [Blk(msgs, csr=csr, mean=mean, pre_act=pre), Blk(table(n, H, 84 + i))]
        nt = net(2 * H, (H, H, H), 85 + i, True, WSETS[mix][i % 2])
        launch(f"bx6:{form[0]}:agg_on_load:{'ordered' if shuffle is None else 'seg_perm'}:{'mean' if mean else 'sum'} {prec} pre_act={pre} mix={mix}", prec, nt, blks, n, cls, K_BX6,
               act="selu", small=form[1], control=(lambda L: R.row_in_next_segment(L, 0, 250)) if i == 2 else None)


@lines(lambda prec, form: {(K_BX6, f"bx6:{form[0]}:{x}", prec) for x in ("narrow-only", "narrow+wide")})
@pytest.mark.parametrize("form", FORMS, ids=lambda f: f[0])
@pytest.mark.parametrize("prec", PRECS)
def test_bx6_narrow_blocks(prec, form):
    """fp32 blocks of 2, 3, 5 and G4C_NARROW_MAX columns multiplied on the vector ALUs: alone (an encoder), next to wide blocks with a
    folded sign, as column windows of one buffer."""
    assert _lib.NARROW_MAX == 8
    n = 777
    for i, mix in enumerate(("A", "C")):          # (not "B": under a 10-column first layer its 6e4 columns would leave fp16's range one layer on)
        buf = rows_of(n, 24, mix, 90 + i)
        nb = [Blk(buf, col0=1, width=2, narrow=True), Blk(buf, col0=4, width=3, narrow=True), Blk(buf, col0=8, width=5, narrow=True)]
        nt = net(10, (H, H, H), 91 + i, False, WSETS[mix][0])
        launch(f"bx6:{form[0]}:narrow-only {prec} mix={mix}", prec, nt, nb, n, R.row_classes(n, DEV), K_BX6, act="selu", small=form[1])
        mb = [Blk(buf, col0=16, width=8, narrow=True, negate=True), Blk(rows_of(n, H, mix, 92 + i)), Blk(buf, col0=2, width=2, narrow=True)]
        nt = net(8 + H + 2, (H, H, H), 93 + i, True, WSETS[mix][1])
        launch(f"bx6:{form[0]}:narrow+wide {prec} mix={mix}", prec, nt, mb, n, R.row_classes(n, DEV), K_BX6, act="tanh", small=form[1])


# ====================================================================== MLP_BX6_CERT
@lines(lambda form: {(K_BX6_CERT, f"bx6_cert:{form[0]}", "f16x3"), (K_BX6, f"bx6:{form[0]}:uncertified", "f16x3")})
@pytest.mark.parametrize("form", FORMS, ids=lambda f: f[0])
def test_bx6_certified_node_form_with_heads(form):
    """The node form with heads from rows that carry a true bound: the tracker-free instantiation."""
    for n in (1, 33, 64, 2047, 5000):
        blks = node_blocks(n, "C", 100 + n, "full")
        nt = net(2 * H, (H, H, H), 101 + n, True, "ln", n_heads=2)
        launch(f"bx6_cert:{form[0]} n={n}", "f16x3", nt, blks, n, R.row_classes(n, DEV), K_BX6_CERT, act="selu", heads=True, certify=True,
               small=form[1], control=(lambda L: R.swap_adjacent_columns(L, 200)) if n == 2047 else None)
    # the same launch without the bound keeps its tracker
    launch(f"bx6:{form[0]}:uncertified n=5000", "f16x3", nt, blks, 5000, R.row_classes(5000, DEV), K_BX6, act="selu", heads=True, small=form[1])


# ====================================================================== MLP_BX6I (bf16x6, mode 2)
@lines(lambda n_nodes: {(K_BX6I, f"bx6i:{x}", "bf16x6") for x in ("plain", "agg", "agg-only", "indexed+out_idx")})
@pytest.mark.parametrize("n_nodes", [1, 11, 350, 6001])
def test_bx6i_message_launch(n_nodes):
    deg = ragged_degrees(n_nodes, 110 + n_nodes) if n_nodes > 11 else torch.full((n_nodes,), 6)
    csr = csr_of(deg)
    E = csr.n
    mix = MIXES[n_nodes % 3]
    nt = net(H, (H, H, H), 111, True, WSETS[mix][1])
    blks, cls = message_blocks(E, n_nodes, mix, 112)
    kw = dict(bx6i=2)
    launch(f"bx6i:plain E={E} mix={mix}", "bf16x6", nt, blks, E, cls, K_BX6I, control=(lambda L: R.skip_pre_act(L, 0)) if n_nodes == 350 else None, **kw)
    for mean in (True, False):
        launch(f"bx6i:agg E={E} mean={mean}", "bf16x6", nt, blks, E, cls, K_BX6I, agg=(csr, mean), **kw)
        launch(f"bx6i:agg-only E={E} mean={mean}", "bf16x6", nt, blks, E, cls, K_BX6I, agg=(csr, mean), store_rows=False, **kw)
    ib, icls = message_blocks(E, n_nodes, mix, 113, indexed=True, pre_act=None)
    oi = torch.randperm(E + 50, generator=_gen(114))[:E].to(DEV)
    launch(f"bx6i:indexed+out_idx E={E}", "bf16x6", nt, ib, E, icls, K_BX6I, act="selu", out_idx=oi, out_rows=E + 50, **kw)


# ====================================================================== MLP_WS / MLP_WS_CERT (f16x3)
@lines(lambda layers, cert: {(K_WS_CERT if cert else K_WS, f"ws:{x}:L{layers}", "f16x3") for x in ("plain", "indexed", "out_idx")}
       | (set() if cert else {(K_WS, f"ws:no-adds:L{layers}", "f16x3")}))
@pytest.mark.parametrize("cert", [False, True], ids=["tracked", "certified"])
@pytest.mark.parametrize("layers", [2, 3])
def test_ws_plain_indexed_scattered(layers, cert):
    """Row counts around the 64-row pairs of the general form (its workgroups take whole pairs: 1 .. 65 rows are one or two pairs with a
    partial last tile, 2047 and 40 037 rows leave a partial last pair, 40 037 rows give most workgroups three pairs and some two).
    Ranges that end inside a tile, and more workgroups than pairs, exist only in the dense form: test_ws_fused_aggregation.
    (A certified launch has the two additive blocks; without them the launch keeps the tracked kernel.)"""
    code = K_WS_CERT if cert else K_WS
    mix = "C" if cert else None
    for i, n in enumerate((1, 31, 32, 33, 63, 64, 65, 2047, 40037)):
        m = mix or MIXES[i % 3]
        nt = net(H, (H,) * layers, 120 + i, True, "ln" if cert else WSETS[m][i % 2])
        blks, cls = message_blocks(n, max(n // 6, 1), m, 121 + i)
        launch(f"ws:plain:L{layers} cert={cert} n={n} mix={m}", "f16x3", nt, blks, n, cls, code, ws=2, certify=cert,
               control=(lambda L: R.wrong_gather_row(L, 1, 2046, additive=True)) if n == 2047 else None)
        if n in (33, 2047, 40037):
            ib, icls = message_blocks(n, max(n // 6, 1), m, 122 + i, indexed=True, pre_act=None)
            launch(f"ws:indexed:L{layers} cert={cert} n={n} mix={m}", "f16x3", nt, ib, n, icls, code, ws=2, act="selu", certify=cert)
            oi = torch.randperm(n + 40, generator=_gen(123 + i))[:n].to(DEV)
            launch(f"ws:out_idx:L{layers} cert={cert} n={n} mix={m}", "f16x3", nt, blks, n, cls, code, ws=2,
                   out_idx=oi, out_rows=n + 40, certify=cert)
            if not cert:
                nb, ncls = message_blocks(n, max(n // 6, 1), m, 124 + i, adds=False, indexed=True, pre_act=None)
                launch(f"ws:no-adds:L{layers} n={n} mix={m}", "f16x3", nt, nb, n, ncls, K_WS, ws=2, act="selu")


@lines(lambda layers, cert: {(K_WS_CERT if cert else K_WS, f"ws:{x}:{f}:L{layers}", "f16x3") for x in ("agg", "agg-only")
                                    for f in ("ragged", "dense", "general")})
@pytest.mark.parametrize("cert", [False, True], ids=["tracked", "certified"])
@pytest.mark.parametrize("layers", [2, 3])
def test_ws_fused_aggregation(layers, cert):
    """Ragged segments (empty ones at both ends and in runs, one of exactly 32 rows), uniform degrees 4 - 8 (the dense form) and 3 and
    9 (the general form): rows against fp64, the aggregate bit for bit; rows not stored: the aggregate against fp64 end to end.
    The dense form cuts the rows per workgroup at segment boundaries, not at tiles: with 173 or 1201 segments there are more
    workgroups than 64-row pairs, with 20 011 segments of 5 or 6 rows every workgroup's range ends inside a tile."""
    code = K_WS_CERT if cert else K_WS
    cases = [("ragged", ragged_degrees(2999, 130))] + [(f"k={k}", torch.full((173 if k % 2 else 1201,), k)) for k in (3, 4, 5, 6, 7, 8, 9)] + [
        (f"k={k} n=20011", torch.full((20011,), k)) for k in (5, 6)]
    for i, (name, deg) in enumerate(cases):
        csr = csr_of(deg)
        assert csr.uniform_deg == (0 if name == "ragged" else int(deg[0])) and csr.tiles() is not None
        # (ws_launch: uniform segments of 4 .. 8 rows take the dense form, every other plan the general one)
        form = "ragged" if name == "ragged" else ("dense" if 4 <= csr.uniform_deg <= 8 else "general")
        mix = "C" if cert else MIXES[i % 3]
        nt = net(H, (H,) * layers, 131 + i, True, "ln" if cert else WSETS[mix][i % 2])
        blks, cls = message_blocks(csr.n, csr.n_seg, mix, 132 + i)
        for mean in (True, False):
            launch(f"ws:agg:{form}:L{layers} {name} cert={cert} mean={mean} mix={mix}", "f16x3", nt, blks, csr.n, cls, code, ws=2, agg=(csr, mean),
                   certify=cert)
            launch(f"ws:agg-only:{form}:L{layers} {name} cert={cert} mean={mean} mix={mix}", "f16x3", nt, blks, csr.n, cls, code, ws=2,
                   agg=(csr, mean), store_rows=False, certify=cert)


def mp_layer(what, layers, deg, mix, seed, v_act, heads, store, mean, cert, expect, control=False, ws=0, bx6i=0):
    """ops.mp_layer_forward: e' (when stored), v' and the heads against their references; the aggregate is internal — v' is checked from
    the launch's own e' rows when they are stored (the k rows are associated differently: statistics, not bits), end to end otherwise."""
    csr = csr_of(deg)
    n, E = csr.n_seg, csr.n
    msg = net(H, (H,) * layers, seed, True, "ln" if cert else WSETS[mix][0])
    upd = net(2 * H, (H,) * layers, seed + 1, True, "ln" if cert else WSETS[mix][1], n_heads=2)
    blks, cls = message_blocks(E, n, mix, seed + 2)
    v = table(n, H, seed + 3)
    with switches("f16x3", ws, bx6i) as lib:
        pm, pu = msg.pack(blks, "f16x3"), upd.pack([Blk(v), Blk(v)], "f16x3", heads=True)
        head_outs = [torch.full((n, H), float("nan"), device=DEV) for _ in range(2)] if heads else None
        with ops.RangeFlags(DEV) as flags:
            e, v_out, _ = ops.mp_layer_forward(pm, [b.source(cert) for b in blks], E, csr, mean, pu, v, ACT[v_act], store_rows=store,
                                               head_outs=head_outs, v_bound=float(v.abs().max()) if cert else None)
            ran = int(lib.g4c_mlp_last_kernel())
        assert ran == expect, f"{what}: kernel code {ran}, expected {expect}"
        assert flags.take() == []
    HIT.add((expect, what.split(" ")[0], "f16x3"))
    L = R.Launch([b.ref() for b in blks if not b.additive], msg.W, msg.b, msg.ln, None, [b.ref() for b in blks if b.additive])
    seg_cls = R.classes_of_segments(cls, csr.off)
    if store:
        check(f"{what} e'", e, R.ref64(L)["y"], R.evaluate(L, F32)["y"], cls)
    else:
        assert e is None
    r64 = R.mp_layer(L, csr.off, mean, upd.W, upd.b, upd.ln, v, v_act, F64, e_rows=e)
    r32 = R.mp_layer(L, csr.off, mean, upd.W, upd.b, upd.ln, v, v_act, F32, e_rows=e)
    check(f"{what} v'", v_out, r64["v"], r32["v"], seg_cls)
    if heads:
        for j, h in enumerate(head_outs):
            check(f"{what} head{j}", h, R.heads(v_out, upd.heads)[j], R.heads(v_out, upd.heads, F32)[j], seg_cls)
    if control:          # one row counted in the next segment
        off2 = R.move_boundary(csr.off, n // 2)
        p64 = R.mp_layer(L, off2, mean, upd.W, upd.b, upd.ln, v, v_act, F64, e_rows=e)
        p32 = R.mp_layer(L, off2, mean, upd.W, upd.b, upd.ln, v, v_act, F32, e_rows=e)
        assert R.rejects(R.assert_as_accurate_as_fp32, v_out, p64["v"], p32["v"], seg_cls, f"{what} CONTROL")


@lines(lambda layers, cert: {(K_WS_CERT if cert else K_WS, f"mp_layer:L{layers}:v_act={a}:heads={h}:store={st}:{m}", "f16x3")
                                    for a in (None, "selu") for h in (False, True) for st in (True, False) for m in ("mean", "sum")})
@pytest.mark.parametrize("cert", [False, True], ids=["tracked", "certified"])
@pytest.mark.parametrize("layers", [2, 3])
def test_ws_one_launch_mp_layer(layers, cert):
    i = 0
    for v_act in (None, "selu"):
        for heads in (False, True):
            for store in (True, False):
                for mean in (True, False):
                    deg = ragged_degrees(1500, 140 + i) if i % 2 else torch.full((37 if i % 4 else 1201,), 6)
                    mix = "C" if cert else MIXES[i % 3]
                    mp_layer(f"mp_layer:L{layers}:v_act={v_act}:heads={heads}:store={store}:{'mean' if mean else 'sum'} cert={cert} mix={mix}", layers, deg, mix,
                             141 + 3 * i, v_act, heads, store, mean, cert, K_WS_CERT if cert else K_WS, control=(i == 1))
                    i += 1


# ====================================================================== the headline sizes, every switch as shipped
@lines(lambda: {(K_WS_CERT, "headline:message", "f16x3"), (K_WS, "headline:message-tracked", "f16x3"), (K_BX6_CERT, "headline:node", "f16x3"),
                (K_WS_CERT, "headline:mp_layer", "f16x3"), (K_BX6I, "headline:bx6i", "bf16x6")})
def test_headline_sizes_with_the_shipped_switches():
    lib = _lib.load()
    assert ops.mlp_precision() == "f16x3" and lib.g4c_mlp_ws_enable(-1) == 1 and lib.g4c_mlp_bx6i_enable(-1) == 1
    assert lib.g4c_mlp_small_launch_tiles(-1) == 512 and ops.RANGE_PROOFS
    keep = dict(ws=1, bx6i=1, small=None)
    # the level-1 message launch: 600 000 rows, k = 6, fused mean, certified inputs
    csr = csr_of(torch.full((100_000,), 6))
    nt = net(H, (H, H, H), 150, True, "ln")
    blks, cls = message_blocks(csr.n, csr.n_seg, "C", 151)
    launch("headline:message 600k k=6 mean", "f16x3", nt, blks, csr.n, cls, K_WS_CERT, agg=(csr, True), certify=True, **keep)
    launch("headline:message-tracked 600k k=6 mean mix=A", "f16x3", nt, message_blocks(csr.n, csr.n_seg, "A", 152)[0], csr.n, cls, K_WS,
           agg=(csr, True), **keep)
    # the node launch with heads: 100 000 rows
    nb = node_blocks(100_000, "C", 153, "full")
    nn = net(2 * H, (H, H, H), 154, True, "ln", n_heads=2)
    launch("headline:node 100k heads", "f16x3", nn, nb, 100_000, R.row_classes(100_000, DEV), K_BX6_CERT, act="selu", heads=True, certify=True, **keep)
    # a ragged fused MP layer at a coarse-level size
    mp_layer("headline:mp_layer ragged 25k nodes", 3, ragged_degrees(25_000, 155, 11), "C", 156, "selu", True, True, True, True, K_WS_CERT, ws=1, bx6i=1)
    # the recompute arithmetic at >= 400 000 rows: the dual-tile kernel in its default mode
    c4 = csr_of(torch.full((70_000,), 6))
    b4, cls4 = message_blocks(c4.n, c4.n_seg, "A", 157)
    launch("headline:bx6i 420k", "bf16x6", nt, b4, c4.n, cls4, K_BX6I, agg=(c4, True), **keep)
