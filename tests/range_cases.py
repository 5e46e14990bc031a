"""Planted cases for the fp16 range flags of the "f16x3" launches, shared by tests/test_range_ref.py (CPU: the cases meet their
conditions on the fp64 reference, and a tracker left out at any one site is caught) and tests/test_gpu_range_sites.py (the launches).
Everything here is a CPU tensor.

A launch converts to fp16, site by site (oracle/fwd_ref.py `converted`): its weighted wide input blocks as they are parked (in{j}), the
SELU output of every layer but the last (h{l}) and, with heads, its output rows (heads).  The flag contract is `any(|v| >= 65504)` over
exactly these values.  A model-level clipping test raises dozens of sites at once; a case here raises ONE, by routing through weights:

  in{j} at (r, c)      the stored element behind row r, column c of block j = 1e5 (1.2e5 times the row count under a sum / mean on load),
                       W0[:, c] = 0: the clipped operand meets a zero weight, so the rows equal, bit for bit, the twin launch with 0 there;
  h1 at (r, j)         column c of one block zeroed in every row, then x[r, c] = 1000, W0[:, c] = 0, W0[j, c] = 100, W1[:, j] = 0;
  h1 through an add    p[i[r], j] = 1e5 in a table row that only launch row r names, W1[:, j] = 0: the tracker sees the value after the adds;
  h2 at (r, j2)        the same column, W0[j, :] = 0, b0[j] = 0, W0[j, c] = 1, W1[:, j] = 0, W1[j2, j] = 100, W2[:, j2] = 0;
  heads (site level)   behind a LayerNorm no single output element can be large: beta[j] = 1e5 raises column j of every row;
  upd.in0 (site level) the fused layer's aggregate is a sum of LayerNorm'd rows: the message MLP's beta[j] = 3e4 over segments of three to
                       six rows.  With a mean the same data stays at 3e4 and must not flag.

Conditions (`conditions`), asserted on the fp64 reference before anything is launched: the planted site's maximum >= 1e5 (1.5 x the
range end), every other site's <= 16 376 (a quarter of it).  The kernels' values differ from the exact ones by ~1e-6 relative, so no
case is near the threshold except the threshold cases, whose converted value is the stored fp32 number itself.

Positions: rows 0, n // 2 (a middle tile) and n - 1 (the last row of a partial tile: masked lanes re-read it); columns / features
0, 37, 70, 127 (one per 32-column wave slice); the first and the second block of a 256-wide first layer.

Every element plant routes the large value to zero weights, so the planted launch's rows equal its twin's bit for bit (0 x finite = 0
in every partial product); the heads plant's HEAD rows do (the head weights' column j is zero)."""
import copy
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import torch

from oracle import fwd_ref as R

H = 128
F32, F64 = torch.float32, torch.float64
END = 65504.0
BELOW = float(torch.nextafter(torch.tensor(END), torch.tensor(0.0)))          # the largest fp32 below the range end
PLANT, PLANT_MIN, OTHERS_MAX = 1e5, 1e5, 16376.0
FLT_MAX = float(torch.finfo(F32).max)
COLS = (0, 37, 70, 127)
TILE_N = (1, 33, 65)               # 32-row tiles: one partial tile, one row into the second, one into the third
WS_N = (1, 64, 65, 130)            # 64-row pairs: a partial pair, exactly one, one row into the second, a partial third


def gen(seed):
    return torch.Generator().manual_seed(seed)


def rows_at(n):
    return sorted({0, n // 2, n - 1})


def cols_in(w):
    return sorted({0, 37 % w, 70 % w, w - 1})


@dataclass
class Blk:
    """One input block on the host: what ops.Source and fwd_ref.Src / Add are built from."""
    x: torch.Tensor
    index: Optional[torch.Tensor] = None
    col0: int = 0
    width: Optional[int] = None
    negate: bool = False
    pre_act: Optional[str] = None
    keys: Optional[torch.Tensor] = None          # aggregation on load: segment of every stored row (== n_seg: a row no segment names)
    n_seg: int = 0
    mean: bool = True
    additive: bool = False
    narrow: bool = False

    def w(self):
        return int(self.x.size(1)) - self.col0 if self.width is None else self.width

    def drops(self):
        return self.keys is not None and bool((self.keys == self.n_seg).any())

    def segments(self) -> Optional[Tuple[torch.Tensor, Optional[torch.Tensor]]]:
        """(off, perm or None) as plan.build_csr groups `keys` (stable; the rows of key n_seg dropped)."""
        if self.keys is None:
            return None
        perm = torch.argsort(self.keys, stable=True)
        perm = perm[self.keys[perm] < self.n_seg]
        off = torch.zeros(self.n_seg + 1, dtype=torch.int64)
        off[1:] = torch.cumsum(torch.bincount(self.keys[self.keys < self.n_seg], minlength=self.n_seg), 0)
        identity = perm.numel() == self.keys.numel() and torch.equal(perm, torch.arange(perm.numel()))
        return off, (None if identity else perm)

    def ref(self, n):
        """(a direct source may hold more than the launch's n rows: the reference reads the rows the launch computes)"""
        if self.additive:
            return R.Add(self.x, self.index, self.col0)
        x = self.x[:n] if self.index is None and self.keys is None else self.x
        return R.Src(x, self.index, self.col0, self.w(), self.negate, self.pre_act, self.segments(), self.mean)

    def stored_row(self, r):
        """The stored row behind launch row r (an aggregate: the first row of segment r)."""
        if self.keys is not None:
            off, perm = self.segments()
            assert int(off[r + 1]) > int(off[r])
            p = int(off[r])
            return p if perm is None else int(perm[p])
        return r if self.index is None else int(self.index[r])

    def count(self, r):
        if self.keys is None or not self.mean:
            return 1
        off, _ = self.segments()
        return int(off[r + 1] - off[r])


@dataclass
class Case:
    name: str
    form: str                                    # the launch form: one line of the site matrix
    n: int = 0
    blks: List[Blk] = field(default_factory=list)
    W: list = field(default_factory=list)
    b: list = field(default_factory=list)
    ln: Optional[tuple] = None
    heads: list = field(default_factory=list)
    act: Optional[str] = None
    resid: Optional[torch.Tensor] = None
    resid_col0: int = 0
    out_idx: Optional[torch.Tensor] = None
    out_init: Optional[torch.Tensor] = None
    agg_deg: Optional[torch.Tensor] = None       # fused aggregation over segments of these row counts (rows in segment order)
    agg_mean: bool = True
    store_rows: bool = True
    first: Optional[torch.Tensor] = None         # form "precomputed": layer 0's rows; blks are the two additive tables
    msg: Optional["Case"] = None                 # form "mp_layer": the message launch and the node MLP on [aggregate | v]
    upd: Optional["Case"] = None
    # what the case pins
    site: Optional[str] = None                   # the one site it raises (None: none)
    expect: bool = False
    site_min: float = PLANT_MIN                  # the planted site's maximum is at least this (expect) ...
    site_exact: Optional[float] = None           # ... or exactly this (threshold cases)
    limit: float = OTHERS_MAX                    # every other site's maximum is at most this
    twin: Optional["Case"] = None                # the same launch with the plant removed
    bit_equal: bool = False                      # ... whose rows it must equal bit for bit
    level: str = "element"
    others_from_twin: bool = False               # (an infinite input: 0 x inf is NaN in the reference too)

    def has_heads(self):
        return bool(self.upd.heads if self.msg is not None else self.heads)

    def agg_off(self):
        off = torch.zeros(int(self.agg_deg.numel()) + 1, dtype=torch.int64)
        off[1:] = torch.cumsum(self.agg_deg, 0)
        return off

    def launch(self):
        if self.msg is not None:
            u = self.upd
            return R.MpLayer(self.msg.launch(), self.msg.agg_off(), self.msg.agg_mean, u.W, u.b, u.ln, u.blks[1].x, u.act)
        if self.first is not None:
            return R.Precomputed(self.first, [a.ref(self.n) for a in self.blks], self.W[1:], self.b[1:], self.ln, self.act)
        wide = [k for k in self.blks if not k.additive]
        return R.Launch([k.ref(self.n) for k in wide], self.W, self.b, self.ln, self.act, [k.ref(self.n) for k in self.blks if k.additive], self.resid,
                        self.resid_col0, self.out_idx, self.out_init, narrow=[k.narrow for k in wide])

    def sites(self, dtype=F64):
        """(memoised: a case is not modified once it is built — the plants work on copies made by _dc / _sc)"""
        memo = self.__dict__.setdefault("_memo", {})
        if dtype not in memo:
            memo[dtype] = R.sites_of(self.launch(), dtype, self.has_heads())
        return memo[dtype]


def _dc(c):
    """A deep copy to be modified (without the memo of `sites`)."""
    out = copy.deepcopy(c)
    out.__dict__.pop("_memo", None)
    return out


def _sc(c):
    out = copy.copy(c)
    out.__dict__.pop("_memo", None)
    return out


def conditions(c: Case):
    """Assert the case's conditions on the fp64 reference; (planted site's maximum or None, the largest other-site maximum)."""
    m = R.site_maxima(c.sites())
    assert c.site is None or c.site in m, (c.name, c.site, sorted(m))
    others = {k: v for k, v in (R.site_maxima(c.twin.sites()) if c.others_from_twin else m).items() if k != c.site}
    worst = max(others.values(), default=0.0)
    assert worst <= c.limit, (c.name, "another site is outside its limit", others)
    planted = None if c.site is None else m[c.site]
    if c.site_exact is not None:
        assert planted == c.site_exact, (c.name, planted)
    elif c.site is not None and c.expect:
        assert planted >= c.site_min, (c.name, planted)
    elif c.site is not None:
        assert planted <= c.limit, (c.name, planted)
    assert R.expected_flag(c.sites()) == c.expect == (planted is not None and planted >= END), (c.name, planted)
    if c.twin is not None and c.expect:
        assert not R.expected_flag(c.twin.sites()) and max(R.site_maxima(c.twin.sites()).values()) <= c.limit, c.name
    return planted, worst


# ---------------------------------------------------------------------------------------------------------------- base launches
def table(n, width, seed):
    return torch.randn(n, width, generator=gen(seed))


def unique_index(n, seed):
    """(index [n], table rows): rows 0, n // 2 and n - 1 each name a table row of their own, the last table row is named by nobody."""
    special = rows_at(n)
    t_rows = max(n // 2, 1) + len(special) + 1
    idx = torch.randint(0, t_rows - len(special) - 1, (n,), generator=gen(seed))
    for k, r in enumerate(special):
        idx[r] = t_rows - 2 - k
    return idx, t_rows


def weights(k_in, layers, seed, wset="ln", n_heads=0):
    Ws, bs, lnp, hs = R.default_weights(k_in, (H,) * layers, gen(seed), True, wset, n_heads)
    return dict(W=Ws, b=bs, ln=lnp, heads=hs)


def node_case(n, seed, layers=3, n_heads=2, direct=False, form="node"):
    """[mix "C" rows | a gathered (or direct) N(0, 1) table] -> MLP -> LayerNorm -> SELU (+ heads)."""
    idx, t_rows = unique_index(n, seed + 2)
    second = Blk(table(n, H, seed + 1)) if direct else Blk(table(t_rows, H, seed + 1), index=idx)
    return Case(f"{form} n={n} L{layers} heads={n_heads}", form, n, [Blk(R.mixed_rows(n, H, "C", gen(seed))), second], act="selu",
                **weights(2 * H, layers, seed + 3, "ln", n_heads))


def window_case(n, seed, path):
    """The second block a column window: 64 wide at column 4 of a 72-wide tensor (16-byte addressable), or 37 wide at column 3 of a
    45-wide one (odd col0 and leading dimension)."""
    wide, col0, w = (72, 4, 64) if path == "vec" else (45, 3, 37)
    return Case(f"window:{path} n={n}", f"window:{path}", n, [Blk(R.mixed_rows(n, H, "C", gen(seed))), Blk(table(n, wide, seed + 1), col0=col0, width=w)],
                **weights(H + w, 3, seed + 3, "default"))


def degrees(n_seg, special_min, pattern):
    deg = torch.tensor([pattern[i % len(pattern)] for i in range(n_seg)])
    for k, r in enumerate(rows_at(n_seg)):
        deg[r] = special_min + k
    return deg


def agg_on_load_case(n, seed, shuffle, mean, pre):
    """The node launch sums / averages each target's messages while it loads them: rows in segment order or through seg_perm."""
    deg = degrees(n, 2, (2, 1, 4, 0, 3, 5))
    keys = torch.arange(n).repeat_interleave(deg)
    if shuffle:
        keys = keys[torch.randperm(int(keys.numel()), generator=gen(seed + 5))]
    msgs = R.mixed_rows(int(keys.numel()), H, "C", gen(seed))
    order = "seg_perm" if shuffle else "ordered"
    form = f"agg_on_load:{order}:{'mean' if mean else 'sum'}:pre={pre}"
    c = Case(f"{form} n={n}", form, n, [Blk(msgs, keys=keys, n_seg=n, mean=mean, pre_act=pre), Blk(table(n, H, seed + 1))], act="selu",
             **weights(2 * H, 3, seed + 3, "ln"))
    assert n == 1 or (c.blks[0].segments()[1] is not None) == shuffle
    return c


def degrees_summing_to(n, pattern=(3, 1, 4, 6, 0, 2, 5)):
    deg, i = [], 0
    while sum(deg) < n:
        deg.append(min(pattern[i % len(pattern)], n - sum(deg)))
        i += 1
    return torch.tensor(deg + [0])          # (an empty segment last)


def message_case(n, seed, layers=3, pre="selu", adds=True, agg=None, store=True, deg=None, form=None):
    """The hoisted message form: e (mix "C" rows, SELU on load) + two gathered product tables; `agg`: None / "mean" / "sum" fused."""
    blks = [Blk(R.mixed_rows(n, H, "C", gen(seed)), pre_act=pre)]
    if adds:
        for j in range(2):
            idx, t_rows = unique_index(n, seed + 10 + j)
            blks.append(Blk(table(t_rows, H, seed + 20 + j), index=idx, additive=True))
    form = form or f"message:L{layers}:pre={pre}:agg={agg}:{'stored' if store else 'not-stored'}"
    c = Case(f"{form} n={n}", form, n, blks, act=None if pre else "selu", **weights(H, layers, seed + 3, "ln"))
    if agg or deg is not None:
        c.agg_deg = degrees_summing_to(n) if deg is None else deg
        assert int(c.agg_deg.sum()) == n
        c.agg_mean, c.store_rows = agg != "sum", store
    return c


def mp_layer_case(n_seg, seed, layers, n_heads, mean=False, v_act="selu", store=True):
    """ops.mp_layer_forward: segments of three to six rows (and empty ones), so that a sum over any of them triples a row."""
    deg = torch.tensor([(4, 3, 5, 0, 6, 3)[i % 6] for i in range(n_seg)])
    n = int(deg.sum())
    form = f"mp_layer:L{layers}:heads={n_heads}"
    msg = message_case(n, seed, layers, agg="mean" if mean else "sum", store=store, deg=deg, form=form + ":msg")
    upd = Case(form + ":upd", form + ":upd", n_seg, [Blk(torch.zeros(n_seg, H)), Blk(table(n_seg, H, seed + 30))], act=v_act,
               **weights(2 * H, layers, seed + 31, "ln", n_heads))
    return Case(f"{form} segs={n_seg} rows={n} {'mean' if mean else 'sum'}", form, n, msg=msg, upd=upd)


def precomputed_case(n, seed, mean=True, store=True):
    """ops.mlp_forward_precomputed: `first` rows of N(0, 1) in T's place + the two gathered tables; W[0] is packed but never read."""
    c = message_case(n, seed, 3, pre=None, agg="mean" if mean else "sum", store=store, form="precomputed")
    c.first, c.blks, c.act = c.blks[0].x, c.blks[1:], None
    return c


def shape_case(kind, n, seed, layers, n_heads):
    """The launches that match a compile-time shape of the tile kernel: the node update [128 | 128], UpMP's [narrow, negated | gathered
    | direct] and DownMP's [narrow | direct]; every wide block 128 wide, direct or as the shape has it."""
    form = f"shape:{kind}:L{layers}:heads={n_heads}"
    nar = Blk(table(n, 2, seed + 7).clamp_(-4, 4), narrow=True, negate=(kind == "up"))
    if kind == "node":
        c = node_case(n, seed, layers, n_heads, direct=True, form=form)
    elif kind == "up":
        c = node_case(n, seed, layers, n_heads, form=form)
        c.blks = [nar, c.blks[1], c.blks[0]]
    else:
        c = node_case(n, seed, layers, n_heads, form=form)
        c.blks, c.act = [nar, c.blks[0]], None
    k_in = sum(k.w() for k in c.blks)
    for key, val in weights(k_in, layers, seed + 3, "ln", n_heads).items():
        setattr(c, key, val)
    return c


# ---------------------------------------------------------------------------------------------------------------- plants
def _wide(c: Case, j):
    """(block j of the weighted blocks, the first column of its part of W0)."""
    wide = [k for k in c.blks if not k.additive]
    return wide[j], sum(k.w() for k in wide[:j])


def _pair(c: Case, planted: Case, twin: Case, site, what, **kw):
    planted.name, twin.name = f"{c.name} {what}", f"{c.name} {what} TWIN"
    planted.site, planted.expect, planted.twin = site, True, twin
    twin.site, twin.expect, twin.twin = site, False, None
    for k, v in kw.items():
        setattr(planted, k, v)
    return planted


def plant_in(c: Case, j, r, col, value=PLANT, expect=True, what=None, **kw):
    """Element (r, col) of weighted block j; the rows must equal the twin's (0 there) bit for bit."""
    p, t = _dc(c), _dc(c)
    for case, val in ((p, value), (t, 0.0)):
        blk, c0 = _wide(case, j)
        # (an aggregate on load: 1.2 x, the segment's other rows add a few hundred at most; a mean divides by the row count)
        blk.x[blk.stored_row(r), blk.col0 + col] = val * blk.count(r) * (1.2 if blk.keys is not None else 1.0)
        case.W[0][:, c0 + col] = 0
    out = _pair(c, p, t, f"in{j}", what or f"in{j}@({r},{col})={value:g}", bit_equal=True, **kw)
    out.expect = expect
    return out


def _route(case: Case, jb, r, col, x_val, w0):
    """Column `col` of block jb zeroed in every stored row, then x[r, col] = x_val; W0[:, col] = 0 but for the entries `w0`."""
    blk, c0 = _wide(case, jb)
    assert blk.keys is None
    blk.x[:, blk.col0 + col] = 0
    blk.x[blk.stored_row(r), blk.col0 + col] = x_val
    case.W[0][:, c0 + col] = 0
    for row, val in w0.items():
        case.W[0][row, c0 + col] = val


def plant_h1(c: Case, jb, r, col, j):
    p, t = _dc(c), _dc(c)
    for case, val in ((p, 1000.0), (t, 0.0)):
        _route(case, jb, r, col, val, {j: 100.0})
        case.W[1][:, j] = 0
    return _pair(c, p, t, "h1", f"h1@({r},{j}) through in{jb} column {col}", bit_equal=True)


def plant_h2(c: Case, jb, r, col, j, j2):
    assert len(c.W) >= 3
    p, t = _dc(c), _dc(c)
    for case, val in ((p, 1000.0), (t, 0.0)):
        case.W[0][j, :] = 0
        case.b[0][j] = 0
        _route(case, jb, r, col, val, {j: 1.0})
        case.W[1][:, j] = 0
        case.W[1][j2, j] = 100.0
        case.W[2][:, j2] = 0
    return _pair(c, p, t, "h2", f"h2@({r},{j2}) through in{jb} column {col}, h1 feature {j}", bit_equal=True)


def plant_h1_add(c: Case, a, r, j):
    """Through additive block a: the table row that only launch row r names."""
    p, t = _dc(c), _dc(c)
    for case, val in ((p, PLANT), (t, 0.0)):
        blk = [k for k in case.blks if k.additive][a]
        assert int((blk.index == blk.index[r]).sum()) == 1
        blk.x[int(blk.index[r]), blk.col0 + j] = val
        case.W[1][:, j] = 0
    return _pair(c, p, t, "h1", f"h1@({r},{j}) through additive block {a}", bit_equal=True)


def plant_heads(c: Case, j):
    """Site level: behind a LayerNorm no single element of the output rows can be large; beta[j] raises column j of every row."""
    p, t = _dc(c), _dc(c)
    p.ln[1][j] = PLANT
    for case in (p, t):          # (the clipped column meets a zero weight in every head: the HEAD rows equal the twin's)
        for Wh in case.heads:
            Wh[:, j] = 0
    return _pair(c, p, t, "heads", f"heads: beta[{j}]=1e5", level="site", bit_equal="heads")


def first_plants(c: Case, r, j, j2):
    """form "precomputed": h1 through `first`, h2 through `first`."""
    out = []
    p, t = _dc(c), _dc(c)
    for case, val in ((p, PLANT), (t, 0.0)):
        case.first[r, j] = val
        case.W[1][:, j] = 0
    out.append(_pair(c, p, t, "h1", f"h1@({r},{j}) through first", bit_equal=True))
    p, t = _dc(c), _dc(c)
    for case, val in ((p, 1000.0), (t, 0.0)):
        case.first[:, j] = 0
        case.first[r, j] = val
        case.W[1][:, j] = 0
        case.W[1][j2, j] = 100.0
        case.W[2][:, j2] = 0
    out.append(_pair(c, p, t, "h2", f"h2@({r},{j2}) through first feature {j}", bit_equal=True))
    return out


def all_plants(c: Case, rows=None):
    """Every site of a plain launch, planted one at a time: per row of interest one element of every in-site, h1 through a weighted
    block and through every additive block, h2; the heads once.  Columns and features cycle through 0, 37, 70, 127."""
    out, k = [], 0
    wide = [b for b in c.blks if not b.additive]
    direct = [j for j, b in enumerate(wide) if b.keys is None and not b.narrow]
    n_add = sum(b.additive for b in c.blks)
    for r in (rows_at(c.n) if rows is None else rows):
        for j, b in enumerate(wide):
            if not b.narrow:
                cs = cols_in(b.w())
                out.append(plant_in(c, j, r, cs[k % len(cs)]))
                k += 1
        jb = direct[k % len(direct)]          # (the first and the second block of a 256-wide first layer in turn)
        cs = cols_in(wide[jb].w())
        out.append(plant_h1(c, jb, r, cs[k % len(cs)], COLS[(k + 1) % 4]))
        for a in range(n_add):
            out.append(plant_h1_add(c, a, r, COLS[(k + a) % 4]))
        if len(c.W) >= 3:
            out.append(plant_h2(c, jb, r, cs[(k + 2) % len(cs)], COLS[(k + 3) % 4], COLS[k % 4]))
        k += 1
    if c.heads:
        out.append(plant_heads(c, COLS[c.n % 4]))
    return out


def precomputed_plants(c: Case):
    out = []
    for k, r in enumerate(rows_at(c.n)):
        out += first_plants(c, r, COLS[k % 4], COLS[(k + 1) % 4])
        out += [plant_h1_add(c, a, r, COLS[(k + 2 + a) % 4]) for a in range(2)]
    return out


def _mp(c: Case, inner: Case, which: str):
    """The MP-layer case whose message (or node) MLP is the planted `inner`, its twin likewise."""
    def wrap(x, name):
        m = _sc(c)
        m.msg, m.upd = (x, c.upd) if which == "msg" else (c.msg, x)
        m.name = f"{c.name} {name}"
        return m
    p, t = wrap(inner, f":: {inner.name}"), wrap(inner.twin, f":: {inner.twin.name}")
    p.site, p.expect, p.twin, p.level, p.bit_equal = f"{which}.{inner.site}", inner.expect, t, inner.level, inner.bit_equal
    p.others_from_twin, t.site = inner.others_from_twin, p.site
    return p


def mp_layer_plants(c: Case):
    """Every msg.* and upd.* site.  upd.in0 (the aggregate, computed inside the launch) is site level: the message MLP's beta."""
    out = [_mp(c, p, "msg") for p in all_plants(c.msg, rows_at(c.msg.n)[1:])]
    # the node MLP's input block 0 is the aggregate: element plants go through block 1 (v)
    u, k = c.upd, 0
    for r in rows_at(u.n):
        out.append(_mp(c, plant_in(u, 1, r, COLS[k % 4]), "upd"))
        out.append(_mp(c, plant_h1(u, 1, r, COLS[(k + 1) % 4], COLS[(k + 2) % 4]), "upd"))
        if len(u.W) >= 3:
            out.append(_mp(c, plant_h2(u, 1, r, COLS[(k + 2) % 4], COLS[(k + 3) % 4], COLS[k % 4]), "upd"))
        k += 1
    if u.heads:
        out.append(_mp(c, plant_heads(u, 37), "upd"))
    assert not c.msg.agg_mean
    msg, upd = _dc(c.msg), _dc(c.upd)
    msg.ln[1][70] = 3e4
    upd.W[0][:, 70] = 0          # (the clipped aggregate column meets a zero weight)
    p, t = _sc(c), _sc(c)
    p.upd = t.upd = upd
    p.msg, p.name, t.name = msg, f"{c.name} upd.in0: message beta[70]=3e4, summed", f"{c.name} upd.in0 TWIN"
    p.site, p.expect, p.twin, p.level, t.site = "upd.in0", True, t, "site", "upd.in0"
    out.append(p)
    return out


def mean_control(c: Case):
    """The upd.in0 plant under a mean: every aggregate row holds 3e4 — inside the range (below half its end), no flag."""
    m = mp_layer_case(c.upd.n, 400, len(c.upd.W), len(c.upd.heads), mean=True)
    m.msg.ln[1][70] = 3e4
    m.upd.W[0][:, 70] = 0
    m.name += " message beta[70]=3e4, MEAN"
    m.site, m.expect, m.limit, m.level = None, False, END / 2, "mean control"
    return m


# ---------------------------------------------------------------------------------------------------------------- thresholds, signs, unread data, huge values
def threshold_cases(c: Case, j, r, col):
    """Direct in-sites only (the converted value is the stored fp32 number): 65504 and -65504 flag, the next fp32 below does not.
    A sum on load: two rows of 32752 (and 32752 + (the next fp32 below 65504 - 32752), whose fp32 sum is exact)."""
    blk, _ = _wide(c, j)
    out = []
    for name, val, expect in (("+65504", END, True), ("-65504", -END, True), ("below", BELOW, False), ("-below", -BELOW, False)):
        if blk.keys is None:
            p = plant_in(c, j, r, col, val, expect, what=f"threshold in{j}@({r},{col}) {name}")
        else:
            assert not blk.mean
            p, t = _dc(c), _dc(c)
            for case, on in ((p, True), (t, False)):
                b, c0 = _wide(case, j)
                off, perm = b.segments()
                assert int(off[r + 1] - off[r]) == 2
                rows2 = [int(off[r]) + i if perm is None else int(perm[int(off[r]) + i]) for i in range(2)]
                half = torch.tensor(32752.0)
                rest = torch.tensor(abs(val)) - half          # exact in fp32
                sgn = 1.0 if val > 0 else -1.0
                b.x[rows2[0], b.col0 + col], b.x[rows2[1], b.col0 + col] = (sgn * half, sgn * rest) if on else (0.0, 0.0)
                case.W[0][:, c0 + col] = 0
            p = _pair(c, p, t, f"in{j}", f"threshold in{j}@({r},{col}) {name} as a sum of two rows", bit_equal=True)
            p.expect = expect
        p.site_exact, p.level = abs(val), "threshold"
        out.append(p)
    return out


def selu_sign_cases(c: Case, j, r, col):
    """Under SELU on load -1e5 is converted as -1.76: no flag; +1e5 flags."""
    assert _wide(c, j)[0].pre_act == "selu"
    neg = plant_in(c, j, r, col, -PLANT, False, what=f"selu sign in{j}@({r},{col})=-1e5", level="selu sign -1e5")
    return [neg, plant_in(c, j, r, col, PLANT, True, what=f"selu sign in{j}@({r},{col})=+1e5", level="selu sign +1e5")]


def huge_cases(c: Case, j, r, col):
    """In-site values 1e30, FLT_MAX and +inf: the flag is mandatory; at 1e30 the rows are finite and equal the zeroed launch's."""
    out = []
    for name, val in (("1e30", 1e30), ("FLT_MAX", FLT_MAX), ("inf", float("inf"))):
        p = plant_in(c, j, r, col, val, True, what=f"huge in{j}@({r},{col})={name}", level="huge:" + name)
        p.bit_equal, p.others_from_twin = name == "1e30", True
        out.append(p)
    return out


UNREAD = 1e6


def _unread(c: Case, filled: Case, what):
    filled.name, filled.twin, filled.bit_equal, filled.level = f"{c.name} UNREAD {what}", c, True, "unread"
    filled.site, filled.expect = None, False
    return filled


def unread_cases(n, seed):
    """Data the launch must not read holds 1e6: no flag, and the rows of the launch with zeros there, bit for bit."""
    out = []
    # rows >= n_rows of a direct source; table rows no index names (the last one: unique_index)
    c = node_case(n, seed)
    c.blks[0].x = torch.cat([c.blks[0].x, torch.zeros(9, H)])
    f = _dc(c)
    f.blks[0].x[n:] = UNREAD
    out.append(_unread(c, f, "rows >= n_rows of a direct source"))
    f = _dc(c)
    named = torch.zeros(int(f.blks[1].x.size(0)), dtype=torch.bool)
    named[f.blks[1].index] = True
    assert not bool(named.all())
    c2 = _dc(c)
    c2.blks[1].x[~named] = 0
    f.blks[1].x[~named] = UNREAD
    out.append(_unread(c2, f, "table rows no index names"))
    # columns outside a col0 / width window
    for path in ("vec", "unaligned"):
        c = window_case(n, seed + 1, path)
        b = c.blks[1]
        outside = torch.ones(int(b.x.size(1)), dtype=torch.bool)
        outside[b.col0:b.col0 + b.w()] = False
        c.blks[1].x[:, outside] = 0
        f = _dc(c)
        f.blks[1].x[:, outside] = UNREAD
        out.append(_unread(c, f, f"columns outside the {path} window"))
    # rows of an aggregate-on-load source that seg_perm does not name
    for mean in (True, False):
        c = agg_on_load_case(n, seed + 2, True, mean, "selu")
        b = c.blks[0]
        drop = torch.zeros(int(b.keys.numel()), dtype=torch.bool)
        drop[::3] = True
        drop &= ~torch.isin(b.keys, torch.tensor(rows_at(n)))          # (the segments of interest keep their rows)
        b.keys[drop] = b.n_seg
        assert b.drops()
        b.x[b.keys == b.n_seg] = 0
        f = _dc(c)
        f.blks[0].x[b.keys == b.n_seg] = UNREAD
        out.append(_unread(c, f, f"rows seg_perm does not name ({'mean' if mean else 'sum'})"))
    # rows of `out` that out_idx does not name
    c = node_case(n, seed + 3, n_heads=0)
    c.out_idx = torch.randperm(n + 7, generator=gen(seed + 4))[:n]
    c.out_init = torch.zeros(n + 7, H)
    f = _dc(c)
    f.out_init[:] = UNREAD
    out.append(_unread(c, f, "out rows no out_idx names"))
    # the residual: read and added in fp32, never converted — a window at column 4 of a 140-wide tensor, 1e6 everywhere
    c = node_case(n, seed + 5, n_heads=0)
    c.act, c.resid, c.resid_col0 = None, torch.zeros(n, 140), 4
    f = _dc(c)
    f.resid[:] = UNREAD
    out.append(_unread(c, f, "the residual tensor"))
    return out


# ---------------------------------------------------------------------------------------------------------------- the catalogue
import functools          # noqa: E402


@functools.lru_cache(maxsize=None)
def catalogue(group: str) -> tuple:
    """The cases of one group of launches (built once; nothing modifies a case)."""
    out = []
    if group == "node":                       # tile kernel: three layers, two heads — in0, in1, h1, h2, heads
        for n in TILE_N:
            out += all_plants(node_case(n, 100 + n))
    elif group == "window":                   # tile kernel, vec and unaligned source paths
        for path in ("vec", "unaligned"):
            for n in TILE_N:
                out += all_plants(window_case(n, 120 + n, path), rows_at(n)[-2:])
    elif group == "agg_on_load":              # ordered and through seg_perm, sum and mean, with and without the pending SELU
        for i, (shuffle, mean, pre) in enumerate(((False, True, None), (False, False, "selu"), (True, True, "selu"), (True, False, None))):
            for n in TILE_N:
                out += all_plants(agg_on_load_case(n, 140 + 10 * i + n, shuffle, mean, pre), rows_at(n)[-2:])
    elif group == "message_tile":             # tile kernel: the message form with the fused aggregation on ragged tiles of whole segments
        for n in TILE_N:
            for agg, store in (("mean", True), ("sum", False)):
                out += all_plants(message_case(n, 200 + n, 3, agg=agg, store=store), rows_at(n)[-2:])
    elif group == "shapes":                   # tile kernel, compile-time shapes: every site of each
        for kind, layers, n_heads in (("node", 2, 0), ("node", 2, 2), ("node", 3, 0), ("node", 3, 2), ("up", 3, 0), ("up", 3, 2), ("down", 3, 0)):
            for n in (33, 65):
                out += all_plants(shape_case(kind, n, 300 + n + layers + n_heads, layers, n_heads), [0, 32] if n == 33 else [32])
    elif group == "ws":                       # mlp_ws_kernel: SELU on load, two additive blocks; with / without the fused aggregation
        for i, n in enumerate(WS_N):
            layers = 2 + i % 2
            out += all_plants(message_case(n, 400 + n, layers))
            out += all_plants(message_case(n, 410 + n, 5 - layers, agg="mean", store=True), rows_at(n)[-2:])
            out += all_plants(message_case(n, 420 + n, layers, agg="sum", store=False), rows_at(n)[:2])
        dense = message_case(66, 430, 3, agg="mean", store=True, deg=torch.full((11,), 6))          # (uniform degree 6: the dense form)
        out += all_plants(dense)
        for n in (65, 130):                   # in0 with both signs: a block without SELU on load (the converted value is the stored one)
            c = message_case(n, 440 + n, 3, pre=None)
            if n == 130:
                out += all_plants(c, rows_at(n)[1:])
            for k, r in enumerate(rows_at(n)):
                out += [plant_in(c, 0, r, COLS[k], PLANT), plant_in(c, 0, r, COLS[k + 1], -PLANT)]
    elif group == "mp_layer":
        for i, (layers, n_heads) in enumerate(((2, 0), (2, 2), (3, 0), (3, 2))):
            c = mp_layer_case((17, 37)[i % 2], 500 + i, layers, n_heads, store=bool(i % 3))
            out += mp_layer_plants(c)
            out.append(mean_control(c))
    elif group == "precomputed":
        for i, n in enumerate((1, 65, 130)):
            out += precomputed_plants(precomputed_case(n, 600 + n, mean=bool(i % 2), store=i != 1))
    elif group == "threshold":                # a direct, full-width, aligned block; an indexed one; a sum on load of two rows
        out += threshold_cases(node_case(33, 700), 0, 32, 127)
        out += threshold_cases(node_case(65, 701), 1, 32, 37)
        out += threshold_cases(agg_on_load_case(33, 702, False, False, None), 0, 0, 70)
        out += threshold_cases(agg_on_load_case(65, 703, True, False, None), 0, 0, 0)
    elif group == "threshold_ws":
        out += threshold_cases(message_case(65, 710, 3, pre=None), 0, 64, 127)
        out += threshold_cases(message_case(130, 711, 2, pre=None, agg="mean"), 0, 65, 37)
    elif group == "selu_sign":
        out += selu_sign_cases(message_case(33, 720, 3, agg="mean"), 0, 32, 70)
        out += selu_sign_cases(agg_on_load_case(33, 721, False, False, "selu"), 0, 16, 37)
    elif group == "selu_sign_ws":
        out += selu_sign_cases(message_case(65, 722, 3), 0, 64, 0)
        out += selu_sign_cases(message_case(130, 723, 2, agg="sum", store=False), 0, 65, 127)
    elif group == "unread":
        out += unread_cases(33, 800) + unread_cases(65, 810)
    elif group == "huge":
        out += huge_cases(node_case(33, 900), 0, 32, 37)
        out += huge_cases(node_case(65, 901), 1, 0, 127)
    elif group == "huge_ws":
        out += huge_cases(message_case(65, 910, 3, pre=None), 0, 64, 70)
        out += huge_cases(message_case(130, 911, 3, agg="mean"), 0, 65, 0)
    elif group == "huge_mp":
        c = mp_layer_case(17, 920, 3, 2)
        out += [_mp(c, p, "msg") for p in huge_cases(c.msg, 0, c.msg.n - 1, 37)]
        out += [_mp(c, p, "upd") for p in huge_cases(c.upd, 1, 16, 70)]
    else:
        raise ValueError(group)
    return tuple(out)


GROUPS = ("node", "window", "agg_on_load", "message_tile", "shapes", "ws", "mp_layer", "precomputed", "threshold", "threshold_ws",
          "selu_sign", "selu_sign_ws", "unread", "huge", "huge_ws", "huge_mp")
PLANTED_GROUPS = GROUPS[:8]          # the groups that pin every site of every launch form they hold
