"""Shapes and seeded host data shared by tests/test_adjoint_ref.py (CPU) and tests/test_gpu_adjoint_ref.py (the launches): the linear
adjoints of the multi-scale / gMuS / REMuS path (autograd.py below _FusedMLP).  Everything here is a CPU tensor; the shapes are the
smallest at which these launches can go wrong, not a workload's."""
import math

import torch

from oracle import grad_ref as R

F32, I32, I64 = torch.float32, torch.int32, torch.int64

ROWS = (1, 33, 257, 4097)            # rows / segments: 257 is one row past a 256-thread workgroup, 4097 one past 16 of them
FEATS = (1, 3, 64)                   # REMuS helpers (width 2F): F = 3 the scalar path, F = 64 the 128-wide vector path
KS = (1, 3, 5, 8)                    # in-degree
WIDTHS = (1, 6, 128, 132)            # gather and reduction adjoints: scalar kernel (1, 6), 32 lanes per row, a second column pass
LAYOUTS = ("contiguous", "window", "broadcast", "transposed")
PLANS = ("ordered", "permuted", "dropped")
HOT = 41                             # reads of the most-read row of every gather index (at least 40)
SEG_LENGTHS = (0, 1, 2, 3, 5, 7, 8, 9, 13, 17, 40)        # the reduction's batch of 8 and its half-batch switch are the edges
POW2_LENGTHS = (0, 1, 2, 4, 8, 16, 32)                     # a mean over such a segment is exact on integers


def gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + (sum(map(ord, k)) if isinstance(k, str) else int(k) + 17)) % (2 ** 31)
    return torch.Generator().manual_seed(seed)


def operand(shape, kind, g, vmax=8):
    """"int": integers in [-vmax, vmax]; "float": N(0.2, 1.5^2)."""
    return R.int_operand(shape, vmax, g) if kind == "int" else torch.randn(tuple(shape), generator=g) * 1.5 + 0.2


# ---------------------------------------------------------------- gradient layouts
def dout_values(rows, width, layout, kind, g, vmax=8):
    """The values of a gradient as autograd may hand it over; a row-broadcast one has one row repeated."""
    if layout == "broadcast":
        return operand((1, width), kind, g, vmax).expand(rows, width).contiguous()
    return operand((rows, width), kind, g, vmax)


def as_layout(values, layout):
    """`values` [r, w] (any device) as a tensor of that layout with the same elements: contiguous; a column window at offset 3 of a
    tensor 5 columns wider; strides (0, 1) (what stands behind `out.sum(0)`); a transposed view (strides (1, r))."""
    r, w = values.shape
    if layout == "contiguous":
        return values.contiguous()
    if layout == "window":
        wide = torch.full((r, w + 5), 7.0, dtype=values.dtype, device=values.device)
        wide[:, 3:3 + w] = values
        return wide[:, 3:3 + w]
    if layout == "broadcast":
        assert r == 0 or bool((values == values[:1]).all())
        return values[:1].contiguous().expand(r, w)
    if layout == "transposed":
        return values.t().contiguous().t()
    raise ValueError(layout)


# ---------------------------------------------------------------- gather indices
def gather_index(rows, g):
    """(idx int64 [rows + HOT - 1], n_x, max multiplicity): `rows` rows of x are read — one HOT times, the others once — and
    ceil(rows / 8) + 1 more rows (at least 10 % of n_x, scattered among them) are never read."""
    n_free = math.ceil(rows / 8) + 1
    n_x = rows + n_free
    ids = torch.randperm(n_x, generator=g)
    read = ids[:rows]
    idx = torch.cat([read, read[:1].expand(HOT - 1)])
    idx = idx[torch.randperm(idx.numel(), generator=g)]
    assert n_free >= 0.1 * n_x
    return idx.to(I64), n_x, HOT


def gather_case(rows, width, layout, kind):
    """dict(idx, n_x, mult, x [n_x, width], dout [len(idx), width] values)."""
    g = gen("gather", rows, width, layout, kind)
    idx, n_x, mult = gather_index(rows, g)
    return dict(idx=idx, n_x=n_x, mult=mult, x=operand((n_x, width), kind, g), dout=dout_values(idx.numel(), width, layout, kind, g))


# ---------------------------------------------------------------- segment plans
def seg_lengths(n_seg, pow2, g):
    """Empty segments at both ends and in the middle, a segment of length 1, the longest length present (from 33 segments)."""
    pool = POW2_LENGTHS if pow2 else SEG_LENGTHS
    if n_seg == 1:
        return [1]
    lens = [pool[int(i)] for i in torch.randint(0, len(pool), (n_seg,), generator=g)]
    lens[0] = lens[-1] = 0
    if n_seg >= 33:
        lens[n_seg // 2 - 1:n_seg // 2 + 2] = [0, 0, 0]
        lens[1], lens[2], lens[n_seg // 2 + 2] = 1, pool[-1], 1
    return lens


def seg_keys(n_seg, plan_kind, pow2, g):
    """(keys int64 [n_src], lens): the segment of every source row.  "ordered": rows in segment order (no permutation); "permuted":
    shuffled; "dropped": shuffled, with n_src / 6 + 1 more rows of key n_seg — the trash bin of build_csr(..., n_seg + 1,
    drop_last_segment=True), rows that are in no segment."""
    lens = seg_lengths(n_seg, pow2, g)
    keys = torch.repeat_interleave(torch.arange(n_seg), torch.tensor(lens))
    if plan_kind == "dropped":
        keys = torch.cat([keys, torch.full((keys.numel() // 6 + 1,), n_seg)])
    if plan_kind != "ordered":
        keys = keys[torch.randperm(keys.numel(), generator=g)]
    return keys.to(I64), lens


def host_csr(keys, n_seg, drop_last=False):
    """(off int64 [n_seg + 1], perm int64 or None) as plan.build_csr groups `keys` (stable), for the CPU tests."""
    nk = n_seg + (1 if drop_last else 0)
    perm = torch.argsort(keys, stable=True)
    off = torch.zeros(nk + 1, dtype=I64)
    off[1:] = torch.cumsum(torch.bincount(keys, minlength=nk), 0)
    if drop_last:
        off = off[:n_seg + 1]
        perm = perm[:int(off[-1])]
    identity = perm.numel() == keys.numel() and bool((perm == torch.arange(keys.numel())).all())
    return off, (None if identity else perm)


def reduce_case(n_seg, width, plan_kind, layout, kind, mean):
    """dict(keys, n_seg, drop, lens, max_deg, src [n_src, width], dout [n_seg, width]).  Integer means use power-of-two lengths."""
    g = gen("reduce", n_seg, width, plan_kind, layout, kind, int(mean))
    keys, lens = seg_keys(n_seg, plan_kind, kind == "int" and mean, g)
    return dict(keys=keys, n_seg=n_seg, drop=plan_kind == "dropped", lens=lens, max_deg=max(lens),
                src=operand((keys.numel(), width), kind, g), dout=dout_values(n_seg, width, layout, kind, g))


# ---------------------------------------------------------------- weighted mean (knn_interpolate)
_POW2_PATTERN = {1: [1], 3: [2, 1, 1], 5: [4, 1, 1, 1, 1], 8: [1] * 8}     # integer weights, each pattern sums to a power of two


def wm_case(n_seg, k, width, kind, masked, layout="contiguous"):
    """dict(x [n_x, width], x_idx int64 [n_seg k] (a row read HOT times or more, rows never read), w [n_seg k, 1], off, y_idx,
    mask bool [n_out] or None, out_idx int64 or None, n_out, mult, dout [n_out, width]).  Every segment has k rows (an interpolation
    target always has its k neighbours: an empty segment would be 0 / 0 in the reference too).  "int": integer x, weights pattern * 2^a
    (a per segment in 0 .. 3): totals are powers of two, every coefficient a dyadic fraction, every product and sum exact.  "float":
    weights 1 / clamp(d^2, 1e-16) with a coincident point (d = 0) in every fifth segment."""
    g = gen("wm", n_seg, k, width, kind, int(masked), layout)
    n = n_seg * k
    n_x = max(n_seg // 2, 1) + max(n_seg // 10, 1) + 1
    n_read = n_x - max(n_seg // 10, 1) - (1 if n_x > 2 else 0)
    n_read = max(n_read, 1)
    ids = torch.randperm(n_x, generator=g)[:n_read]
    x_idx = ids[torch.randint(0, n_read, (n,), generator=g)]
    x_idx[torch.randperm(n, generator=g)[:min(n, HOT)]] = ids[0]
    off = torch.arange(n_seg + 1, dtype=I64) * k
    if kind == "int":
        x = R.int_operand((n_x, width), 8, g)
        a = torch.randint(0, 4, (n_seg, 1), generator=g).to(F32)
        w = (torch.tensor(_POW2_PATTERN[k], dtype=F32)[None, :] * torch.exp2(a)).reshape(-1, 1)
    else:
        x = torch.randn(n_x, width, generator=g) * 2 + 0.5
        d = torch.rand(n_seg, k, generator=g) * 1.5
        d[::5, 0] = 0.0
        w = (1.0 / torch.clamp(d * d, min=1e-16)).reshape(-1, 1).to(F32)
    if masked:
        n_out = n_seg + n_seg // 3 + 2
        mask = torch.zeros(n_out, dtype=torch.bool)
        mask[torch.randperm(n_out, generator=g)[:n_seg]] = True
        out_idx = mask.nonzero().reshape(-1)
    else:
        n_out, mask, out_idx = n_seg, None, None
    mult = int(torch.bincount(x_idx, minlength=n_x).max())
    return dict(x=x, x_idx=x_idx.to(I64), w=w, off=off, y_idx=torch.arange(n_seg).repeat_interleave(k), mask=mask, out_idx=out_idx,
                n_out=n_out, n_x=n_x, k=k, mult=mult, dout=dout_values(n_out, width, layout, kind, g))


# ---------------------------------------------------------------- REMuS helpers
def proj_case(n_edges, n_feat, indexed, kind, layout="contiguous"):
    """dict(v [n_v, 2F], node int64 [n_edges] or None, unit [n_edges, 2], mult, dout [n_edges, F]).  Indexed: the gather index of
    `gather_index` cut to n_edges reads (the hot row HOT times where there are that many edges), so rows of v stay unread."""
    g = gen("proj", n_edges, n_feat, int(indexed), kind, layout)
    if indexed:
        n_v = max(n_edges // 3, 1) + max(n_edges // 10, 1) + 1
        n_read = max(n_edges // 3, 1)
        ids = torch.randperm(n_v, generator=g)[:n_read]
        node = ids[torch.randint(0, n_read, (n_edges,), generator=g)]
        node[torch.randperm(n_edges, generator=g)[:min(n_edges, HOT)]] = ids[0]
        mult = int(torch.bincount(node, minlength=n_v).max())
    else:
        n_v, node, mult = n_edges, None, 1
    unit = R.int_operand((n_edges, 2), 8, g) if kind == "int" else torch.nn.functional.normalize(torch.randn(n_edges, 2, generator=g), dim=1)
    return dict(v=operand((n_v, 2 * n_feat), kind, g), node=node, unit=unit, n_edges=n_edges, n_feat=n_feat, mult=mult,
                dout=dout_values(n_edges, n_feat, layout, kind, g))


def e2n_case(n_nodes, n_feat, k, kind, layout="contiguous"):
    """dict(e [n_nodes k, F], unit_inv [n_nodes, 2, k], edge_index (k edges into every node, grouped by receiver), dout [n_nodes, 2F])."""
    g = gen("e2n", n_nodes, n_feat, k, kind, layout)
    col = torch.arange(n_nodes).repeat_interleave(k)
    row = torch.randint(0, n_nodes, (n_nodes * k,), generator=g)
    return dict(e=operand((n_nodes * k, n_feat), kind, g), unit_inv=operand((n_nodes, 2, k), kind, g), k=k, n_nodes=n_nodes,
                edge_index=torch.stack([row, col]), dout=dout_values(n_nodes, 2 * n_feat, layout, kind, g))


# ---------------------------------------------------------------- pool_edge
def pool_case(n_fine, width, kind):
    """dict(idx int64 [n_fine] fine -> coarse node, edge_index [2, E], edge_attr [E, width], dout values come from the test): clusters
    of ~4 nodes, 6 edges per node among which edges inside a cluster (dropped by pool_edge) and parallel coarse edges (merged)."""
    g = gen("pool", n_fine, width, kind)
    n_c = max(n_fine // 4, 2)
    idx = torch.randint(0, n_c, (n_fine,), generator=g)
    idx[:n_c] = torch.arange(n_c)
    E = 6 * n_fine
    ei = torch.stack([torch.randint(0, n_fine, (E,), generator=g), torch.randint(0, n_fine, (E,), generator=g)])
    ei[:, :4] = torch.tensor([[0, 0, 0, 0], [1, 1, 1, 1]])          # four parallel fine edges: a power-of-two segment for sure
    return dict(idx=idx, edge_index=ei, edge_attr=operand((E, width), kind, g), n_coarse=n_c)


def host_pool_plan(idx, edge_index, target_major=False):
    """(coarse edge_index [2, E_c], off, perm) as plan.pool_edge_plan orders them: fine edges renumbered, those inside one cluster
    dropped, the others grouped by coarse edge — sorted by (row, col), or by (col, row) when `target_major` — stably."""
    r, c = idx[edge_index[0]], idx[edge_index[1]]
    keep = (r != c).nonzero().reshape(-1)
    n_c = int(idx.max()) + 1
    key = (c[keep] * n_c + r[keep]) if target_major else (r[keep] * n_c + c[keep])
    uniq, inv = torch.unique(key, sorted=True, return_inverse=True)
    order = torch.argsort(inv, stable=True)
    off = torch.zeros(uniq.numel() + 1, dtype=I64)
    off[1:] = torch.cumsum(torch.bincount(inv, minlength=uniq.numel()), 0)
    hi, lo = uniq // n_c, uniq % n_c
    coarse = torch.stack([lo, hi]) if target_major else torch.stack([hi, lo])
    return coarse, off, keep[order]
