"""Shapes and seeded host data shared by tests/test_mem_ref.py (CPU) and tests/test_gpu_mem_ref.py (the launches): the negative
controls of the host file run at exactly the shapes and data the GPU file launches.  Everything here is a CPU tensor."""
import torch

from oracle import mem_ref as M

F32, I32 = torch.float32, torch.int32
SENT = -(2.0 ** 111)                  # what every output buffer holds before a launch; an element the launch does not own keeps it
ACTS = (None, "selu", "tanh")

# ---------------------------------------------------------------- segment_reduce
SEG_LENGTHS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 12, 13, 16, 17, 40)      # the batch of 8 and its half-batch switch at 4 are the edges
N_SEGS = (1, 7, 8, 9, 33, 1031)                                     # a 256-thread workgroup holds 8, 16 or 32 segments
VEC_WIDTHS = (4, 32, 36, 64, 68, 128, 132, 200, 256, 260)           # all three lanes-per-row instantiations, a second column pass
SCALAR_WIDTHS = (1, 3, 6, 130)
PERMS = ("none", "full", "subset")


def gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + (hash(k) if not isinstance(k, str) else sum(map(ord, k)))) % (2 ** 31)
    return torch.Generator().manual_seed(seed)


def seg_lengths(n_seg):
    """Lengths cycling through SEG_LENGTHS (the short plans start at different places of the cycle, so that 7, 8 and 9 segments
    together see every length): an empty segment first, one last, and (from 33 segments) a run of four."""
    if n_seg == 1:
        return [13]
    start = {7: 7, 9: 5}.get(n_seg, 0)
    lens = [SEG_LENGTHS[(i + start) % len(SEG_LENGTHS)] for i in range(n_seg)]
    lens[0] = lens[-1] = 0
    if n_seg >= 33:
        lens[14:18] = [0, 0, 0, 0]
    return lens


def offsets(lens):
    off = torch.zeros(len(lens) + 1, dtype=torch.int64)
    off[1:] = torch.cumsum(torch.tensor(lens, dtype=torch.int64), 0)
    return off.to(I32)


def seg_case(n_seg, width, perm, kind):
    """dict(src [n_src, width], off int32 [n_seg + 1], perm int32 [n] or None, n, n_seg, max_deg).  `kind`: "int" (|v| <= 8: every sum
    of a segment of <= 40 rows is far below 2^24) or "float".  perm "none": src has two rows more than the plan reads; "subset":
    the plan names n rows of a src of 1.5 n + 3 rows, in random order (the pool_edge plan)."""
    g = gen("seg", n_seg, width, perm, kind)
    lens = seg_lengths(n_seg)
    off = offsets(lens)
    n = int(off[-1])
    n_src = {"none": n + 2, "full": n, "subset": n + n // 2 + 3}[perm]
    p = None if perm == "none" else torch.randperm(n_src, generator=g)[:n].to(I32)
    src = M.int_operand((n_src, width), 8, g) if kind == "int" else torch.randn(n_src, width, generator=g) * 1.5 + 0.2
    return dict(src=src, off=off, perm=p, n=n, n_seg=n_seg, max_deg=max(lens))


# ---------------------------------------------------------------- weighted_segment_mean
WM_K = (1, 2, 3, 4, 5, 8)
WM_WIDTHS = (1, 3, 63, 64, 65, 128, 200)        # 64 lanes per segment
WM_NSEG = (0, 1, 257)
_POW2_PATTERN = {1: [1], 2: [1, 1], 3: [2, 1, 1], 4: [1, 1, 1, 1], 5: [4, 1, 1, 1, 1], 8: [1] * 8}     # each sums to a power of two


def wm_case(k, width, n_seg, kind, scattered):
    """dict(x [n_x, width], x_idx int32 [n_seg k], w [n_seg k], off, out_idx int32 [n_seg] or None, n_out).  "int": integer x and
    weights pattern * 2^a (a per segment in -3 .. 3): every product, sum and the quotient are exact.  "float": random x, weights
    1 / clamp(d^2, 1e-16) for distances d from 0 (a coincident point, every fifth segment) to O(1): they span 1e16."""
    g = gen("wm", k, width, n_seg, kind, scattered)
    n_x = 41
    n = n_seg * k
    x_idx = torch.randint(0, n_x, (n,), generator=g).to(I32)
    off = (torch.arange(n_seg + 1) * k).to(I32)
    if kind == "int":
        x = M.int_operand((n_x, width), 8, g)
        a = torch.randint(-3, 4, (n_seg, 1), generator=g).to(F32)
        w = (torch.tensor(_POW2_PATTERN[k], dtype=F32)[None, :] * torch.exp2(a)).reshape(-1)
    else:
        x = torch.randn(n_x, width, generator=g) * 2 + 0.5
        d = torch.rand(n_seg, k, generator=g) * 1.5
        d[::5, 0] = 0.0
        w = (1.0 / torch.clamp(d * d, min=1e-16)).reshape(-1).to(F32)
    n_out = 2 * n_seg + 5 if scattered else n_seg
    out_idx = torch.randperm(n_out, generator=g)[:n_seg].to(I32) if scattered else None
    return dict(x=x, x_idx=x_idx, w=w, off=off, out_idx=out_idx, n_out=n_out, n=n, n_seg=n_seg, k=k)


# ---------------------------------------------------------------- REMuS-GNN helpers
RM_FEATS = (1, 3, 64, 128)
RM_K = (1, 4, 5, 8)
RM_N = (0, 1, 255, 257)


def proj_case(n_edges, n_feat, indexed, kind):
    """dict(v [n_v, 2 n_feat + 2] (v_ld > 2 n_feat), node int32 [n_edges] (with repeats) or None, other (the other endpoint), unit)."""
    g = gen("proj", n_edges, n_feat, indexed, kind)
    n_v = max(n_edges // 3, 2) if indexed else n_edges + 1
    cols = 2 * n_feat + 2
    v = M.int_operand((n_v, cols), 8, g) if kind == "int" else torch.randn(n_v, cols, generator=g)
    unit = M.int_operand((n_edges, 2), 8, g) if kind == "int" else torch.nn.functional.normalize(torch.randn(n_edges, 2, generator=g), dim=1)
    node = torch.randint(0, n_v, (n_edges,), generator=g).to(I32) if indexed else None
    other = ((node + 1) % n_v).to(I32) if indexed else None
    return dict(v=v, node=node, other=other, unit=unit, n_edges=n_edges, n_feat=n_feat)


def e2n_case(n_nodes, n_feat, k, kind):
    """dict(e [n_nodes k, n_feat + 3] (e_ld > n_feat; the launch reads the first n_feat columns), unit_inv [n_nodes, 2, k])."""
    g = gen("e2n", n_nodes, n_feat, k, kind)
    if kind == "int":
        e, ui = M.int_operand((n_nodes * k, n_feat + 3), 8, g), M.int_operand((n_nodes, 2, k), 8, g)
    else:
        e, ui = torch.randn(n_nodes * k, n_feat + 3, generator=g), torch.randn(n_nodes, 2, k, generator=g)
    return dict(e=e, unit_inv=ui, n_nodes=n_nodes, n_feat=n_feat, k=k)


# ---------------------------------------------------------------- activation_
ACT_N = (0, 1, 2, 3, 4, 5, 7, 1023, 1025)
SPECIAL = (0.0, -0.0, 1e-40, -1e-40, 20.0, -20.0, 88.0, -88.0, 1e30, -1e30, float("inf"), float("-inf"))


def act_case(n):
    return torch.randn(n, generator=gen("act", n)) * 3


# ---------------------------------------------------------------- layer_norm
LN_WIDTHS = (1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 1100)     # the lane boundary; registers -> re-reading at 64 x 16 columns
LN_ROWS = (0, 1, 3, 4, 5, 301)                                            # four rows per workgroup
LN_FAMILIES = ("normal", "offset", "constant", "outlier", "tiny")
LN_EPS = 1e-5
# (rows, gamma / beta present, activation, in place, strided in and out): every width runs all six
LN_CONFIGS = ((301, True, None, False, False), (5, False, "selu", True, False), (4, True, "tanh", False, True),
              (3, True, "selu", True, True), (1, False, None, False, True), (0, True, None, False, False))


def ln_case(width):
    """dict(x [301, width]: row r of family LN_FAMILIES[r % 5], gamma, beta)."""
    g = gen("ln", width)
    x = torch.empty(301, width)
    fam = torch.arange(301) % 5
    x[fam == 0] = torch.randn(int((fam == 0).sum()), width, generator=g) * 3 + 0.7
    x[fam == 1] = 1e4 + torch.randn(int((fam == 1).sum()), width, generator=g)          # (the two-pass property)
    x[fam == 2] = (torch.randn(int((fam == 2).sum()), 1, generator=g) * 5 + 3.7).expand(-1, width)
    o = torch.randn(int((fam == 3).sum()), width, generator=g)
    o[:, width // 2] = 1e6
    x[fam == 3] = o
    x[fam == 4] = torch.randn(int((fam == 4).sum()), width, generator=g) * 1e-20
    gamma = 1 + 0.3 * torch.randn(width, generator=g)
    beta = 0.2 * torch.randn(width, generator=g)
    return dict(x=x, gamma=gamma, beta=beta, family=fam)


# ---------------------------------------------------------------- rollout_advance
RA_NODES = (0, 1, 255, 256, 257, 1000)
RA_SHAPES = ((1, 1), (3, 3), (3, 15), (2, 7))         # (nf, field_cols); field_cols == nf: no roll
RA_STEPS, RA_SLOTS = 6, 7                             # six launches into seven slots: the last slot is never written


def ra_case(n_nodes, nf, cols):
    g = gen("ra", n_nodes, nf, cols)
    return dict(field=torch.randn(n_nodes, cols, generator=g), preds=[torch.randn(n_nodes, nf, generator=g) for _ in range(RA_STEPS)])


# ---------------------------------------------------------------- copy_cols / add_cols
CC_WIDTHS = (1, 3, 128)


def cc_case(width, indexed):
    """dict(src [37, width + 5], dst0 [29, width + 7], idx int32 [29] or None, scol0 = 2, dcol0 = 3, n_rows = 23)."""
    g = gen("cc", width, indexed)
    src = torch.randn(37, width + 5, generator=g)
    idx = torch.randint(0, 37, (29,), generator=g).to(I32) if indexed else None
    return dict(src=src, idx=idx, scol0=2, dcol0=3, n_rows=23, width=width, dst_shape=(29, width + 7))


def ac_case(width):
    """dict(a [35, width + 6] read from column 4, b [33, width] as a window of [33, width + 3])."""
    g = gen("ac", width)
    return dict(a=torch.randn(35, width + 6, generator=g) * 1e3, b_wide=torch.randn(33, width + 3, generator=g), a_col0=4, width=width)
