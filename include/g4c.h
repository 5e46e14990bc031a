/*
 * g4c.h — C-ABI of libg4c.so: the MI355X (gfx950) implementation of graphs4cfd's
 * message-passing hot path.
 *
 * The reference (mario-linov/graphs4cfd) has no FFI / operator registry: its hot path is
 * Python calling torch + torch_geometric ops.  Each entry point below
 * therefore names the reference *op sequence* (file:line under graphs4cfd/) that it
 * replaces.  All pointers are raw device pointers unless marked "host"; `stream` is a
 * hipStream_t passed as void*; indices are int32 (the reference's int64 index tensors are
 * narrowed once, when the static mesh plan is built).  Every function returns 0 on
 * success or a negative G4C_E* code; g4c_last_error() returns a thread-local message.
 * No entry point synchronises the stream or allocates device memory, so a whole rollout
 * step can be captured in a hipGraph.
 *
 * Reference-side binding: see INTEGRATION.md (ctypes stub for graphs4cfd/nn/blocks.py).
 */
#ifndef G4C_H
#define G4C_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define G4C_OK 0
#define G4C_EINVAL (-1)   /* bad argument (the Python binding raises ValueError) */
#define G4C_ELAUNCH (-2)  /* HIP launch / runtime failure (RuntimeError) */
#define G4C_EUNSUPPORTED (-3) /* shape outside the kernels' envelope (NotImplementedError) */

/* Activations (every fused epilogue, source activation on load, g4c_activation_inplace): branch-free on the hardware exponential and
 * reciprocal, fp32 round-off class against F.selu / torch.tanh (bounded per element in tests/test_gpu_mem_ref.py).  Infinities: SELU(+inf)
 * = +inf, SELU(-inf) = -scale * alpha, tanh(+-inf) = +-1; tanh keeps the sign of zero, SELU(-0) = +0.
 * DIFFERENCE FROM THE REFERENCE — NaN is NOT propagated (measured on gfx950, pinned by test_activation_nan_is_not_propagated):
 *   SELU(NaN) = -scale * alpha = -1.7580993 (0xbfe10966), whatever the NaN's sign or payload: max(NaN, 0) = 0 and the [0, 1] clamp of
 *               exp2(NaN) gives 0, i.e. a NaN is treated like -inf;
 *   tanh(NaN) = +1 or -1 by the NaN's sign bit: min(|NaN|, 20) = 20.
 * F.selu and torch.tanh return NaN.  A NaN that enters an activated launch therefore leaves it as a finite number; NaNs in data are
 * the caller's to find before the rollout (ACT_NONE passes them through unchanged). */
#define G4C_ACT_NONE 0
#define G4C_ACT_SELU 1
#define G4C_ACT_TANH 2

#define G4C_MAX_SRC 4
#define G4C_MAX_LAYERS 4
#define G4C_MAX_HEADS 2
#define G4C_NARROW_MAX 8

int g4c_version(void);
/* Where a launch on `device_ptr`'s buffers goes: the ordinal of the device that owns it (every launching entry point switches to that
 * device for the call, whatever the caller's current device is) and the compute-unit count the persistent kernels size their grids
 * with there (cached per ordinal).  A multi-GPU job checks both on every rank before it times anything (bench.py partition_check). */
int g4c_device_info(const void *device_ptr, int32_t *device /*host, out*/, int32_t *cu_count /*host, out*/);
const char *g4c_last_error(void);

/* ---------------------------------------------------------------- static mesh plan (host)
 * The reference recomputes topology every step with host syncs: `scatter(dim_size=None)`,
 * `idx.max().item()`, `remove_self_loops`, `coalesce` (nn/blocks.py:45,63-67,109,231).  The
 * plan builders do that work once per mesh.  Host pointers in, host pointers out. */

/* Stable counting sort of `n` keys in [0, n_seg): perm[p] = original position of the p-th
 * entry in key order, off[s]..off[s+1] = its segment.  Replaces the index handling inside
 * torch_geometric.utils.scatter as called at nn/blocks.py:183,231,330,378. */
int g4c_plan_csr(const int64_t *keys /*host*/, int64_t n, int64_t n_seg,
                 int32_t *perm /*host, n*/, int32_t *off /*host, n_seg+1*/);

/* Topology part of pool_edge (nn/blocks.py:51-68): remap endpoints through idx_hr_to_lr,
 * drop intra-cluster edges, merge duplicates; coarse edges ordered by (row, col) exactly as
 * torch_geometric.utils.coalesce orders them.  Outputs: coarse edge_index (2 x n_coarse,
 * row-major), `perm` = surviving fine edges grouped by coarse edge (stable), `off` =
 * n_coarse+1 segment offsets into perm.  Returns n_coarse (>= 0) or a negative error. */
int64_t g4c_plan_pool_edge(const int64_t *idx_hr_to_lr /*host, n_hr*/, int64_t n_hr,
                           const int64_t *edge_index /*host, 2 x n_edges*/, int64_t n_edges,
                           int64_t *coarse_edge_index /*host, 2 x n_edges capacity*/,
                           int32_t *perm /*host, n_edges capacity*/,
                           int32_t *off /*host, n_edges+1 capacity*/,
                           int64_t *n_kept /*host, 1*/);
/* Same, with the order of the coarse edges selectable: target_major = 0 is the function above; target_major = 1 groups the
 * coarse edges by TARGET (sorted by (col, row)) — the order the models use internally: the reference never exposes the
 * coarse edge order and in this order the coarse MP layers need no permutation.  O(n) (two stable
 * counting-sort passes). */
int64_t g4c_plan_pool_edge_ordered(const int64_t *idx_hr_to_lr, int64_t n_hr, const int64_t *edge_index, int64_t n_edges,
                                   int32_t target_major, int64_t *coarse_edge_index, int32_t *perm, int32_t *off,
                                   int64_t *n_kept);

/* ---------------------------------------------------------------- aggregation (HBM-bound)
 * out[s, :] = act( reduce_{p in [off[s], off[s+1])} src_act( src[perm ? perm[p] : p, :] ) )
 * mean = sum / max(count, 1) (empty segments give 0).  Summation runs in p order, so with a
 * stable plan the result equals a sequential scatter_add_.  Replaces
 * torch_geometric.utils.scatter(reduce='sum'|'mean') at nn/blocks.py:183,231,330,378 and the
 * feature part of coalesce(reduce='mean') at nn/blocks.py:67. */
int g4c_segment_reduce(const float *src, int32_t src_ld, const int32_t *perm, const int32_t *off,
                       int32_t n_seg, int32_t width, int32_t mean, int32_t src_act, int32_t act,
                       float *out, int32_t out_ld, void *stream);

/* knn_interpolate (nn/blocks.py:34-48) with fixed, y-sorted segments:
 * out[o(s), :] = sum_p w[p] * x[x_idx[p], :] / sum_p w[p],  o(s) = out_idx ? out_idx[s] : s. */
int g4c_weighted_segment_mean(const float *x, int32_t x_ld, const int32_t *x_idx, const float *w,
                              const int32_t *off, int32_t n_seg, int32_t width,
                              float *out, int32_t out_ld, const int32_t *out_idx, void *stream);

/* ---------------------------------------------------------------- fused MLP (MFMA-bound)
 * One launch for: gather + concatenate up to 4 sources -> Linear -> (SELU -> Linear)* ->
 * [LayerNorm] -> [SELU|tanh] -> [+ residual] -> store (optionally row-scattered).
 * Replaces `MLP.forward` (nn/blocks.py:117-144) together with the torch.cat / index ops that
 * feed it and the F.selu / torch.tanh / residual add that follow it at every call site
 * (nn/blocks.py:181,185,229,285,328,332,373,380,456; nn/mus_gnn.py:178-218).
 * g4c_mlp_t describes the packed weights and names their arithmetic (w_format), g4c_src_t one input
 * block, g4c_mlp_io_t everything the launch writes; g4c_mlp_run is the one entry point. */
#define G4C_DTYPE_F32 0
#define G4C_DTYPE_BF16 1
#define G4C_DTYPE_BF16_SELU 2   /* g4c_mlp_io_t.out_dtype with a fused aggregation only: rows stored as bf16(SELU(row)) */

typedef struct {
    const float *ptr;   /* [rows, ld] row-major */
    const int32_t *idx; /* NULL: row r of the tile reads row r; else reads row idx[r] */
    int32_t width;      /* columns taken from this source */
    int32_t ld;         /* row stride in floats */
    int32_t col0;       /* first column taken */
    int32_t pre_act;    /* G4C_ACT_*: applied to the values as they are loaded (lets a producer store the
                           un-activated tensor its aggregation needs, nn/blocks.py:181-183 vs nn/mus_gnn.py:182) */
    int32_t additive;   /* 0: a column block of the concatenated input (multiplied by the first layer's weights);
                           1: a term ALREADY multiplied by its block of the first layer's weights, at the row count of
                           the tensor it was gathered from; row idx[r] is added to row r of the first layer's output.
                           Linearity: W1 [e | v[row] | v[col]] = W1e e + (W1r v)[row] + (W1c v)[col], so the node-side
                           products cost N rows instead of E (nn/blocks.py:181, :328, :373).
                           2 (split-operand formats only): a NARROW column block (width <= G4C_NARROW_MAX, idx == NULL, no pre_act)
                           multiplied in fp32 on the vector ALUs by its rows of the first layer's weight, `w`, instead of
                           being padded to a 128-k block of the matrix-pipe stream (the 2..5-wide encoder / DownMP / UpMP
                           inputs: nn/mus_gnn.py:71,176-177, nn/blocks.py:229,285); such blocks are NOT part of the packed
                           stream (k_pad[0] counts the other blocks only). */
    int32_t seg_mean;   /* with seg_off: 1 = mean over the segment (divided by max(count, 1)), 0 = sum */
    const float *w;     /* additive == 2: fp32 [width][128] = W1^T rows of this block (sign folded in), zero padded */
    const int32_t *seg_off; /* split-operand formats, additive == 0, idx == NULL, width 128: row r of this block is the sum / mean of rows
                           [seg_off[r], seg_off[r+1]) of ptr — the aggregation `scatter(e', col, reduce)` (nn/blocks.py:183) done
                           while the node MLP gathers its input, in the order and with the formula of g4c_segment_reduce, instead
                           of a separate pass that writes and re-reads the aggregate.  `pre_act` is then applied to every
                           source row BEFORE it is added (g4c_segment_reduce's src_act). */
    const int32_t *seg_perm; /* with seg_off: NULL = the segment's rows are [seg_off[r], seg_off[r+1]) themselves; else those are
                           positions in seg_perm, which holds the row numbers (pool_edge's fine -> coarse edge plan,
                           nn/blocks.py:67: the pooled coarse edge latents are formed while the first coarse edge MLP gathers them). */
    int32_t dtype;      /* G4C_DTYPE_F32 (0): the rows are fp32.  G4C_DTYPE_BF16 (1), rounded-bf16 mode only, width 128, no seg_off:
                           the rows are bf16 (ptr is a bf16 pointer, ld / col0 in elements) — additive == 0: message rows a launch
                           stored with out_dtype G4C_DTYPE_BF16 / _BF16_SELU; additive == 1: first-layer products a launch stored as
                           bf16 rows or heads (widened exactly and added to the fp32 accumulators: half the bytes of the largest
                           gather stream). */
} g4c_src_t;

typedef struct {
    int32_t n_layers;                /* number of Linear layers, 1..G4C_MAX_LAYERS */
    int32_t k_pad[G4C_MAX_LAYERS];   /* padded input width of each layer (see g4c_mlp_pack_layer).  k_pad[0] == 0 (w[0] == w[1]: the
                                        stream starts with layer 1): no block of layer 0 goes through the stream — its blocks are all
                                        narrow, or, in a call whose sources are ALL ADDITIVE, THE FIRST LAYER IS PRECOMPUTED: b[0] keeps
                                        its unused slot and the additive sources sum to the layer-0 pre-activation, bias included: rows of layer 0's output = (src0 + src1) + src2
                                        in fp32, in this order.  Built for one shape (anything else: G4C_EUNSUPPORTED): G4C_WFMT_F16X2,
                                        three layers, the fused aggregation, three 128-wide 16-byte aligned fp32 additive sources of
                                        which the first is direct (idx NULL: the static product of an MP layer's first layer with its
                                        edge block, computed once per rollout) and the other two are gathered, plain fp32 128-wide
                                        output rows or none, no heads / residual / out_idx / out_dtype / save / upd.  Always
                                        range-tracked. */
    int32_t n_pad[G4C_MAX_LAYERS];   /* padded output width: 128 */
    const float *w[G4C_MAX_LAYERS];  /* packed weights of each layer: one contiguous stream, layer after layer */
    const float *b[G4C_MAX_LAYERS];  /* bias padded with zeros to n_pad, layer after layer */
    const float *ln_gamma;           /* NULL: no LayerNorm */
    const float *ln_beta;
    float ln_eps;
    int32_t n_out;                   /* true output width of the last layer */
    int32_t w_format;                /* G4C_WFMT_*: the stream's layout and the arithmetic of every launch of this MLP */
    int32_t range_slot;              /* >= 0: the word of g4c_mlp_io_t.range_flag a clip in a launch of this MLP is reported in */
    /* The caller's range certificate for the launch this descriptor is passed to (G4C_WFMT_F16X2 only; 0 = unknown, the default):
     * non-zero states that NO value the launch converts to fp16 for this MLP — its weighted inputs after their activation on load,
     * every hidden activation, and with heads the final output row — can reach the end of fp16's range, whatever the input data.
     * That is a proof obligation of the caller (bounds of the producers of its inputs joined with the norms of these weights:
     * graphs4cfd_amd/ops.py range_bound), not something the library checks.  When every MLP of the launch (mlp, and upd if given) is
     * certified and io->save / io->mul are not in use, the library may run an instantiation without the range tracker, and the launch
     * NEVER WRITES its words of io->range_flag; otherwise the field is ignored and the launch is tracked as before. */
    int32_t range_certified;
} g4c_mlp_t;

/* Weight formats (g4c_mlp_t.w_format, g4c_mlp_pack_layer).  All take fp32 in and give fp32 out.
 * G4C_WFMT_FP32: fp32 MFMA (mlp_split_kernel).  Stream [k_pad/2][n_pad][2] floats, input blocks padded to multiples of 32.
 * The other formats are SPLIT-OPERAND streams: every input block padded to 128 k (k_pad = 128 * blocks), three bf16 planes per
 * weight (k_pad * n_pad * 3 bf16 per layer), one 128-k block of slack after the last layer (heads included).
 * G4C_WFMT_BF16X3 ("bf16x6"): both operands of every Linear split exactly into three bf16 terms (x = h + m + l), the six largest
 *   partial products accumulated in fp32; dropped terms are <= 2^-23 relative.  The whole fp32 range.
 * G4C_WFMT_F16X2 ("f16x3"): a TWO-way fp16 split of both operands, x = h + l * 2^-11 (h = fp16(x) rounded to nearest,
 *   l = fp16((x - h) * 2^11): 22 significand bits per operand), three products per MAC — (Wh, xh) in one fp32 accumulator, (Wh, xl) +
 *   (Wl, xh) in a second one folded in with 2^-11 at the end of the layer; the dropped (Wl, xl) term and the operand representation are
 *   <= 2^-22 relative each: within the rounding error of an fp32 GEMM of the same shape (measured against fp64: scripts/mlp_accuracy.py,
 *   test_mlp_precisions_vs_fp64) at half the matrix-pipe work of BF16X3.  Range: an input or hidden activation with |x| > 65504 is
 *   clipped to +-65504 (1 + 2^-11) when it is converted (MODE.FP16_OVFL; no infinities or NaNs; reported through io->range_flag); small
 *   values lose nothing.  The WEIGHTS are converted by g4c_mlp_pack_layer, in the default rounding mode and with no report: every
 *   |w| must be below 65504 (the caller's obligation; graphs4cfd_amd/ops.py PackedMLP raises ValueError for a weight beyond it and
 *   points to "bf16x6").  Planes 0 / 1 of the same layout, plane 2 zero.
 * G4C_WFMT_BF16 (rounded bf16, BASELINE config 3 "bf16 edge-MLP MFMA", opt-in): the BF16X3 stream, of which only the LEADING plane is
 *   used: weights and the activations entering each Linear are rounded to bf16 (one product per multiply-add), accumulation / bias /
 *   SELU / LayerNorm / additive sources / residual stay fp32.  Expected deviation from fp32: ~1e-2 on LayerNorm-scale outputs.  Heads
 *   are bf16(act(y)) x bf16(head weights): the operands the consumer's own first layer would form from the gathered rows of y.
 * G4C_WFMT_BF16_RS, _RS2, _RS2N: rounded bf16 in the ROW-SPLIT ORDER (csrc/mlp_rs.hip, a wave owns 16 rows through all layers).  The
 *   caller packs the weights with the COLUMNS of every layer permuted: position 32 j + 8 g + 4 h + e (j < 4, g < 4, h < 2, e < 4) of the
 *   128 input columns takes column 32 j + 16 h + 4 g + e, and every bf16 row of such a launch — the bf16 weighted block, bf16 additive
 *   tables, bf16 output rows / head rows / aggregate — has its 128 values in the SAME order (position -> feature): producers of the
 *   additive tables permute the ROWS of the weight that makes them, readers other than these kernels must undo the order.  fp32 rows,
 *   the bias / LayerNorm vectors and the fp32 aggregate are in feature order.  A launch outside the kernel's envelope fails with
 *   G4C_EUNSUPPORTED instead of computing something else.
 *   _RS (mlp_rs1_kernel): the message launch of an MP layer whose receivers all have the same in-degree k, 4 <= k <= 8 (agg_mode |
 *   G4C_AGG_UNIFORM(k); REMuS-GNN: every edge of a kNN graph receives k angles) — ONE weighted 128-wide direct block (fp32, optional
 *   SELU on load, or bf16), two additive 128-wide blocks through indices, two or three 128-wide layers, LayerNorm, no output activation.
 *   Its aggregate is a fixed-order segmented scan, not the sequential order of g4c_segment_reduce: last-bit differences.
 *   _RS2 (mlp_rs2_kernel): the update MLP of such a layer — TWO weighted 128-wide bf16 blocks [aggregate | e], two layers
 *   (256 -> 128 -> 128), LayerNorm, activation none / SELU, no heads or two bf16 heads (the heads' columns are packed in the row-split
 *   order too, their ROWS are not permuted); bf16 output and head rows come out in the row-split order, fp32 rows in feature order.
 *   _RS2N: the same with the e block's rows in FEATURE order (rows a launch of another kernel stored). */
#define G4C_WFMT_FP32 0
#define G4C_WFMT_F16X2 1
#define G4C_WFMT_BF16X3 2
#define G4C_WFMT_BF16_RS 3
#define G4C_WFMT_BF16_RS2 4
#define G4C_WFMT_BF16_RS2N 5
#define G4C_WFMT_BF16 6

/* Packs one nn.Linear weight W[n_out, k_in] (row-major, device) into the stream of `w_format`.  The input dimension is the
 * concatenation of `n_seg` column blocks of widths seg_width[]; seg_negate[s] != 0 folds a sign flip of that block into the weights
 * (UpMP's `-e_hl`, nn/blocks.py:283).  n_pad = 128.  G4C_WFMT_FP32: k_pad = sum of the block widths padded to multiples of 32 (or
 * more), `packed` holds k_pad*n_pad floats.  Split-operand formats: k_pad = 128 * n_seg, `packed` holds k_pad*n_pad*3 bf16.  The
 * row-split formats take the same planes as G4C_WFMT_BF16X3: the caller permutes the columns of W. */
int g4c_mlp_pack_layer(const float *W, int32_t n_out, int32_t k_in, const int32_t *seg_width /*host*/,
                       const int32_t *seg_negate /*host*/, int32_t n_seg, int32_t w_format, void *packed,
                       int32_t k_pad, int32_t n_pad, void *stream);

/* Aggregation mode (g4c_mlp_io_t.agg_mode): bit 0 = mean (else sum).  OR-ed with G4C_AGG_UNIFORM(k) the caller promises that EVERY
 * segment has exactly k rows (1 <= k <= 32: the in-degree of a kNN mesh) — the weight-stationary kernel then aggregates with static
 * addressing instead of reading segment offsets (same sums in the same order; the mean as the correctly rounded quotient by
 * Markstein's correction, which differs from the IEEE division only below 2^-100).  OR-ed with G4C_AGG_OUT_BF16 (G4C_WFMT_BF16_RS
 * only): `agg` points to bf16 rows (agg_ld in elements, a multiple of 8) and the aggregate is stored rounded to bf16 in the row-split
 * order — what the layer's update MLP, its one reader, rounds it to on load anyway. */
#define G4C_AGG_UNIFORM(k) ((int32_t)(k) << 8)
#define G4C_AGG_OUT_BF16 ((int32_t)1 << 16)

/* Everything one launch writes.  Zero-initialise, set `size`, fill what the launch uses. */
typedef struct {
    int32_t size;               /* sizeof(g4c_mlp_io_t), checked first: a binding out of step with this header gets G4C_EINVAL */
    int32_t act;                /* G4C_ACT_* applied to the output rows after LayerNorm */
    int64_t row_begin;          /* the launch covers rows [row_begin, row_begin + row_count) of n_rows; row_begin a multiple of 32.  A sub- */
    int64_t row_count;          /* range splits one MLP over several launches (plain launches only: no heads / aggregation / save / upd) */
    /* output rows: out[o(r), :] (+ resid[r, resid_col0 : ...]), o(r) = out_idx ? out_idx[r] : r.  out_dtype G4C_DTYPE_BF16 (rounded-bf16
     * formats, 128-wide output, no out_idx / resid, out_ld a multiple of 4, out 8-byte aligned): the rows are stored as bf16 (out_ld in
     * elements) — for rows whose one reader rounds them to bf16 on load anyway (first-layer products, REMuS-GNN's edge latents between
     * EdgeMPs, message rows); heads and the aggregate are computed from the fp32 rows.  G4C_DTYPE_BF16_SELU (with the fused aggregation,
     * act NONE): bf16(SELU(row)) — the activation the model applies to the messages after the aggregation (nn/blocks.py:331-333,
     * nn/remus_gnn.py:150-190), which their reader would otherwise apply on load BEFORE rounding: bit for bit the same operand. */
    void *out;                  /* NULL only with the fused aggregation: the rows are not stored, only their aggregate */
    int32_t out_ld;
    int32_t out_dtype;
    const int32_t *out_idx;
    const float *resid;
    int32_t resid_ld, resid_col0;
    /* heads: head_out[h][r, :] = W_h y[r, :], y = the final 128-wide output row (after LayerNorm / activation), W_h a bias-free
     * 128x128 layer packed (k_pad = n_pad = 128) right after the MLP's last layer, heads back to back — the library finds them there.
     * One launch of the node MLP (nn/blocks.py:185) thereby also emits the two node-side first-layer terms W1[:, H:2H] v',
     * W1[:, 2H:3H] v' of the NEXT GNBlock's edge MLP (nn/blocks.py:181), which that edge MLP gathers as additive sources.  128-wide
     * output, no out_idx / resid; head_ld >= 128 (a multiple of 4 in the split-operand formats).  head_dtype G4C_DTYPE_BF16
     * (rounded-bf16 formats): the head rows are stored as bf16 (head_ld in elements, even; outputs 4-byte aligned). */
    int32_t n_heads;
    int32_t head_ld;
    int32_t head_dtype;
    void *head_out[G4C_MAX_HEADS];
    /* fused aggregation (split-operand formats, 128-wide output, no out_idx / resid; enabled by agg != NULL): g4c_plan_tiles cuts the
     * CSR-ordered rows into tiles of whole segments (max_rows 32): tile t = segments [tile_seg[t], tile_seg[t+1]) = rows
     * [tile_rows[t], tile_rows[t+1]) (device int32 arrays, seg_off the CSR offsets).  The launch runs the MLP on those tiles and, from
     * the on-chip copy of each tile's output rows, writes agg[s, :] = sum or mean of the rows of segment s — same order and formula as
     * g4c_segment_reduce, i.e. the `scatter(e', col, reduce)` of nn/blocks.py:183 without re-reading e' from HBM.  With out == NULL
     * the rows are not stored — the last MP layer of a level, whose edge output the reference discards (nn/mus_gnn.py:199-200,211-212). */
    const int32_t *tile_rows, *tile_seg, *seg_off;
    int32_t n_tiles;
    void *agg;
    int32_t agg_ld;             /* >= 128 */
    int32_t agg_mode;           /* bit 0 mean | G4C_AGG_UNIFORM(k) | G4C_AGG_OUT_BF16 */
    /* training form (G4C_WFMT_BF16X3 / _F16X2, and the plain rounded-bf16 stream G4C_WFMT_BF16 — mixed-precision training; not the
     * row-split streams _BF16_RS / _RS2 / _RS2N, not with out_dtype; no heads / aggregation / out_idx; n_save = n_layers, 0 = off): save[l] (or NULL)
     * receives the rows layer l produces — SELU(hidden) for l < n_layers-1, the pre-LayerNorm rows for the last layer — as fp32
     * (or, save_dtype, bf16) [n_rows, 128] (save_ld >= 128, a multiple of 4; 16-byte aligned), so the backward pass of the block recomputes nothing
     * (autograd.py).  mul[l] != NULL (hidden layers; mul_ld >= 128, a multiple of 4): the same launch as the BACKWARD chain of a block —
     * hidden layer l's result is multiplied by the SELU slope of the rows mul[l] holds (SELU outputs) instead of bias + SELU.  Packing
     * the transposed weights last layer first (zero biases) and passing the kept activations as `mul` gives
     *   g_{k-1} = (g_k W_k) * selu'(a_{k-1})   for every hidden layer, each g written through save[], and the input gradient as the
     * launch's output — one launch instead of a product + an elementwise pass per layer. */
    int32_t n_save;
    void *save[G4C_MAX_LAYERS];       /* fp32 rows, or bf16 rows with save_dtype G4C_DTYPE_BF16 (below) */
    int32_t save_ld;
    const void *mul[G4C_MAX_LAYERS];  /* fp32 rows, or bf16 rows with mul_dtype G4C_DTYPE_BF16 (below) */
    int32_t mul_ld;
    /* one launch per MP layer — `GNBlock.forward` (nn/blocks.py:175-186): e' = edge_mlp([e | v[row] | v[col]]), aggregation of e' per
     * target, v' = v_act(upd([aggr | v])) — for the f16x3 format.  `mlp` is the hoisted message MLP (one 128-wide weighted block `e`,
     * the two node-side products as additive sources, two or three 128-wide layers, act NONE) with the fused aggregation (agg: scratch,
     * written and re-read on chip, L2-resident); a persistent workgroup's tile pairs cover a contiguous range of targets, so once they
     * are done it runs the node MLP `upd` (same depth; input blocks [aggregate | v], both 128 wide) on exactly those targets and stores
     * v' to v_out; the heads (n_heads, head_out, head_ld) then belong to `upd` (the NEXT layer's node-side products).  Same arithmetic
     * per element as the two separate launches; sums over k associated as in the weight-stationary kernel.  Small and medium levels of
     * a multi-scale model are bound by the dependent chain inside each launch, not by throughput: this halves the chains per layer. */
    const g4c_mlp_t *upd;       /* NULL: no node update */
    const float *v;
    int32_t v_ld, v_act;
    float *v_out;
    int32_t v_out_ld;
    /* NULL (not tracked), or a device array of int32: a launch in the f16x3 arithmetic writes 1 into range_flag[mlp->range_slot]
     * (and range_flag[upd->range_slot]) when an MLP input or a hidden activation it converted to fp16 reached the end of fp16's range
     * (|x| >= 65504: the value was CLIPPED there) — never written otherwise, never cleared by the library.  The reference computes in
     * fp32 (nn/model.py:303-321), so a set word means the result may differ from it: rerun with the bf16x3 stream (fp32 exponent
     * range).  The array belongs to the caller of the launch, like every other output here: each consumer can pass its own.
     * A launch whose MLPs all carry g4c_mlp_t.range_certified (without save / mul) writes nothing here. */
    int32_t *range_flag;
    /* Storage format of the save[] / mul[] rows: G4C_DTYPE_F32 (0, the default) or G4C_DTYPE_BF16 — G4C_WFMT_BF16 (the plain
     * rounded-bf16 stream) only, every other format returns G4C_EINVAL.  save_dtype BF16: every kept row is stored as
     * bf16(round-to-nearest-even(the fp32 value the launch stores with save_dtype F32)) — save[] are bf16 pointers, save_ld in elements
     * (a multiple of 4), the bases 16-byte aligned; the launch's output and everything else it computes are bit for bit unchanged.
     * mul_dtype BF16: the mul[] rows are bf16 (mul_ld in elements, a multiple of 4; 16-byte aligned), widened exactly to fp32 before
     * the same slope expression.  The two are independent (the backward chain reads bf16 activations and writes fp32 gradients). */
    int32_t save_dtype;
    int32_t mul_dtype;
    /* Row ranges for the fused aggregation over segments of any length (NULL: none; g4c_plan_row_ranges made them for n_wg =
     * g4c_mlp_ws_grid workgroups): workgroup slot i takes rows [wg_rows[i], wg_rows[i + 1]) = segments [wg_seg[i], wg_seg[i + 1]) and
     * cuts them into pairs of full 32-row tiles itself, wg_pairs = the most pairs of a range, wg_max_seg = the most segments of one.
     * Used by the f16x3 launches of the weight-stationary kernel whose rows are not gathered (plain hoisted message launch with the
     * aggregation, and the fused MP layer) when the segments are not uniform with 4 .. 8 rows; every other launch ignores them and
     * runs on the tiles of whole segments above, which stay required.  Same rows, same aggregates, bit for bit. */
    const int32_t *wg_rows, *wg_seg;
    int32_t n_wg, wg_pairs, wg_max_seg;
} g4c_mlp_io_t;

/* One fused-MLP launch over `n_rows` rows of the input `srcs`, writing what `io` names. */
int g4c_mlp_run(const g4c_mlp_t *mlp /*host*/, const g4c_src_t *srcs /*host*/, int32_t n_src, int64_t n_rows,
                const g4c_mlp_io_t *io /*host*/, void *stream);

/* The dual-tile software-pipelined form of the split-operand tile kernel (mlp_bx6i.hip: a workgroup alternates between two 32-row
 * tiles, the vector work of one running under the MFMAs of the other, the layer's weights stationary in registers for both) takes the
 * launches of the MP layers' message MLP (one weighted 128-wide block + 0 or 2 additive blocks, three layers, plain 128-wide output
 * rows — through out_idx too — with or without the fused aggregation) in G4C_WFMT_BF16X3: 0 = never, 1 = launches of at least
 * 400 000 rows (the default mode), 2 = every launch it can take (tests); -1 only queries.  Returns the previous setting. */
int g4c_mlp_bx6i_enable(int on);

/* Weight-stationary persistent form of the same launches for G4C_WFMT_F16X2 and G4C_WFMT_BF16 (mlp_ws.hip: one 8-wave workgroup per
 * CU, every wave keeps its 16-column slice of all layers' weights in registers for the whole launch, the loop over tile pairs
 * prefetches the next pair's indices and rows): same per-element arithmetic as the tile kernel (sums over k in a different
 * association: equal within fp32 rounding, the fused aggregation still bit-identical to g4c_segment_reduce of the stored rows).
 * 0 = never, 1 = launches of at least 20 000 rows (the default mode), 2 = every launch it can take (tests); -1 only queries.
 * Returns the previous setting. */
int g4c_mlp_ws_enable(int on);

/* Small launches of the tile kernel (at most n_tiles 32-row tiles; default 512 = two workgroups per CU) run an instantiation that
 * keeps a whole 128-k block of weights in flight per wave — the next block's weights are requested while this block multiplies —
 * instead of the two-step ring the chip-filling launches use: with one or two waves per SIMD nothing else hides the L2 round trip.
 * Same arithmetic, bit-identical results.  n_tiles >= 0 sets the limit (0 = never), -1 only queries.  Returns the previous limit. */
int g4c_mlp_small_launch_tiles(int n_tiles);

/* Which kernel family the calling thread's most recent g4c_mlp_run ran on — the library picks it per launch (arithmetic, shape,
 * row count), so a profiler-free caller that times launches with events (bench.py's roofline leg) can label them by the kernel that
 * executed: G4C_KERNEL_NONE (no launch yet, or the last call launched nothing), _MLP_SPLIT (mlp_split_kernel: fp32 MFMA), _MLP_BX6
 * (mlp_bx6_kernel: split-operand tile kernel), _MLP_BX6I (mlp_bx6i_kernel: dual-tile), _MLP_WS (mlp_ws_kernel: weight-stationary
 * persistent), _MLP_RS / _MLP_RS2 (mlp_rs1_kernel / mlp_rs2_kernel: the row-split formats), _MLP_BX6_CERT / _MLP_WS_CERT (the
 * instantiations of mlp_bx6_kernel / mlp_ws_kernel WITHOUT the fp16 range tracker: a launch with g4c_mlp_t.range_certified whose shape
 * has one — a certified launch of any other shape reports the tracked kernel's code and runs it with no flag to write). */
#define G4C_KERNEL_NONE 0
#define G4C_KERNEL_MLP_SPLIT 1
#define G4C_KERNEL_MLP_BX6 2
#define G4C_KERNEL_MLP_BX6I 3
#define G4C_KERNEL_MLP_WS 4
#define G4C_KERNEL_MLP_RS 5
#define G4C_KERNEL_MLP_RS2 6
#define G4C_KERNEL_MLP_BX6_CERT 7
#define G4C_KERNEL_MLP_WS_CERT 8
#define G4C_KERNEL_MLP_WS_PRE 9   /* mlp_ws_pre_kernel: the weight-stationary kernel's "first layer precomputed" form (g4c_mlp_t.k_pad[0] == 0) */
int g4c_mlp_last_kernel(void);
/* Workgroups (= row ranges, g4c_mlp_io_t.n_wg) of this thread's last g4c_mlp_run call when it ran the weight-stationary kernel's dense
 * pairs for segments of any length on the caller's row ranges — reported under G4C_KERNEL_MLP_WS / _WS_CERT like the kernel's other
 * forms —, else 0. */
int g4c_mlp_last_row_ranges(void);

/* Compile-time launch shapes of the tile kernel (mlp_bx6_kernel): a launch of G4C_WFMT_F16X2 whose every field matches a shape runs an
 * instantiation in which that shape's fields are constants — no source interpretation, index staging only for a source that has an
 * index, 32-bit row addressing of direct sources through a buffer descriptor; same arithmetic, bit-identical results, same
 * g4c_mlp_last_kernel() code.  Common to the shapes: the chip-filling (two-step ring) form; weighted sources of fp32 rows, 128 wide,
 * 16-byte aligned, no pending activation, no aggregation on load, a direct one of less than 2^31 bytes; no additive blocks; 2 or 3 layers
 * with LayerNorm; plain fp32 128-wide output rows (16-byte aligned; no out_idx, resid, agg, save); 0 or 2 fp32 heads.
 *   G4C_TILE_SHAPE_NODE  the MP layers' node update: two direct sources, no narrow block
 *   G4C_TILE_SHAPE_UP    UpMP: one narrow block, an indexed source, a direct source (in this order of weighted sources)
 *   G4C_TILE_SHAPE_DOWN  DownMP: one narrow block, one direct source, no heads
 * Everything else runs the all-runtime kernel (shape 0).
 * g4c_mlp_shapes_enable: 0 = never, 1 = every launch a shape matches (the default); a negative argument only queries.  Returns the
 * previous setting.  g4c_mlp_last_shape: the shape of the calling thread's most recent g4c_mlp_run (0 when it launched nothing). */
#define G4C_TILE_SHAPE_GENERIC 0
#define G4C_TILE_SHAPE_NODE 1
#define G4C_TILE_SHAPE_UP 2
#define G4C_TILE_SHAPE_DOWN 3
int g4c_mlp_shapes_enable(int on);
int g4c_mlp_last_shape(void);
/* The form a launch that runs a shape takes (process-wide, like the switches above).  Both forms compute the same rows bit for bit: a
 * row's arithmetic does not depend on its tile.
 *   0  32-row tiles, registers bounded for four workgroups per CU
 *   1  64-row tiles (a weight fragment feeds two row tiles: half the weight stream per row), three workgroups per CU (the default):
 *      G4C_TILE_SHAPE_NODE and G4C_TILE_SHAPE_UP launches of more than three times g4c_mlp_small_launch_tiles 32-row tiles whose direct
 *      sources and output stay below 2^31 bytes with a whole last tile of 64 rows; every other launch runs form 0
 * g4c_mlp_tile_form: sets the form, returns the previous one; a negative argument only queries.  g4c_mlp_last_tile_rows: rows per
 * workgroup of the calling thread's most recent g4c_mlp_run when the tile kernel ran it (32 or 64), else 0. */
int g4c_mlp_tile_form(int form);
int g4c_mlp_last_tile_rows(void);

/* Tiles of whole segments for the fused aggregation (g4c_mlp_io_t.tile_rows / tile_seg): returns the tile count, -1 if a segment is
 * longer than max_rows. */
int64_t g4c_plan_tiles(const int32_t *off /*host*/, int32_t n_seg, int32_t max_rows, int32_t *tile_rows /*host, out*/,
                       int32_t *tile_seg /*host, out*/, int64_t capacity);
/* Row ranges for g4c_mlp_io_t.wg_rows / wg_seg: the rows of a CSR (off[0 .. n_seg], off[0] == 0) cut into n_wg contiguous ranges that
 * start and end on segment boundaries, range i = rows [wg_rows[i], wg_rows[i + 1]) = segments [wg_seg[i], wg_seg[i + 1]) (host int32
 * [n_wg + 1] each).  Every range holds at most 64 P rows for the smallest P for which n_wg such ranges exist — P = ceil(rows / (64
 * n_wg)) unless the segment boundaries (one long segment) force more — and among those plans the rows are spread evenly.  A range
 * without rows has no segments (empty ranges come last); empty segments belong to the range they fall in.  Returns P (0: no rows),
 * *max_seg = the most segments of a range, or a negative G4C_E* code. */
int64_t g4c_plan_row_ranges(const int32_t *off /*host*/, int32_t n_seg, int32_t n_wg, int32_t *wg_rows /*host, out*/,
                            int32_t *wg_seg /*host, out*/, int32_t *max_seg /*out*/);
/* Persistent workgroups of a weight-stationary launch on the device of `device_ptr`: one per compute unit, at most G4C_WS_MAX_GRID
 * (environment, read at every call: tests reach workgroups of several tile pairs on small inputs with it). */
int g4c_mlp_ws_grid(const void *device_ptr, int32_t *n_wg);

/* Row-wise LayerNorm (+ activation G4C_ACT_*) over rows of any width: out[r, :] = act((x[r, :] - mean) * rsqrt(var + eps) * gamma + beta),
 * mean / biased variance over the row's `width` columns in two passes, as torch.nn.functional.layer_norm (nn/blocks.py:137-141: the
 * reference's MLP puts a LayerNorm of the output width behind its last Linear layer, whatever that width is).  The fused MLP kernels
 * normalise up to 128 columns in their own epilogue; wider outputs are produced without it and normalised by this launch.
 * gamma / beta may be NULL (1 / 0).  In place (out == x) is allowed. */
int g4c_layer_norm(const float *x, int32_t x_ld, int64_t n_rows, int32_t width, const float *gamma, const float *beta, float eps,
                   int32_t act, float *out, int32_t out_ld, void *stream);

/* Test hook: out[4 i .. 4 i + 3] = a[4 i .. 4 i + 3] / count[i] by the quotient routine the fused aggregation's mean uses (a shared
 * reciprocal + one correction per value, with the division itself as the fallback): must equal the IEEE quotient bit for bit
 * (tests/test_gpu_parity.py::test_mean_div_is_the_ieee_quotient).  count[i] >= 1; a, out 16-byte aligned. */
int g4c_debug_mean_div(const float *a, const int32_t *count, float *out, int64_t n4, void *stream);

/* ---------------------------------------------------------------- REMuS helpers (HBM-bound)
 * out[e, f] = v[node[e], 2f]*U[e,0] + v[node[e], 2f+1]*U[e,1]
 * (nn/remus_gnn.py:124-126, nn/blocks.py:454). node == NULL reads row e. */
int g4c_project_to_edges(const float *v, int32_t v_ld, const int32_t *node, const float *unit,
                         int64_t n_edges, int32_t n_feat, float *out, int32_t out_ld, void *stream);

/* edgeScalarToNodeVector with edgeUnitVectorInverse (nn/blocks.py:88-114):
 * out[n, 2f+c] = sum_j unit_inv[n, c, j] * e[n*k + j, f]. */
int g4c_edge_scalar_to_node_vector(const float *e, int32_t e_ld, const float *unit_inv, int32_t k,
                                   int64_t n_nodes, int32_t n_feat, float *out, int32_t out_ld,
                                   void *stream);

/* ---------------------------------------------------------------- pre-processing
 * The neighbour search of connect_knn (transforms/connect.py:9-72; torch_cluster.knn / k-d tree on the host in the
 * reference): for every point its k nearest OTHER points, ascending distance, exact.  The caller bins the cloud into a
 * uniform grid of `cell_size` cells starting at `origin` (cell id = x + n_cells[0]*(y + n_cells[1]*z)) and hands over the
 * points in cell-sorted order: pos_sorted [n, dim] fp32, cell_sorted [n] their cell ids, order [n] their original
 * indices, cell_start [prod(n_cells)+1] the first sorted point of each cell (all device, int32).  n_cells and origin are
 * host arrays of 3.  out [n, k] int64 (device): row = original index of the query, entries = original indices. */
int g4c_knn_grid(const float *pos_sorted, const int32_t *cell_sorted, const int32_t *order,
                 const int32_t *cell_start, int64_t n, int32_t dim, const int32_t *n_cells, const float *origin,
                 float cell_size, int32_t k, int64_t *out, void *stream);

/* The same search for m separate query points (get_knn_interpolate_weights, transforms/interpolate.py:110-131: the k
 * nearest nodes of pos_x for every node of pos_y): q_pos [m, dim] fp32 and q_cell [m] (each query's cell in the cloud's
 * grid, coordinates clamped into it) in any order; no point is excluded; out [m, k] int64, row = query. */
int g4c_knn_grid_query(const float *pos_sorted, const int32_t *order, const int32_t *cell_start, int64_t n, int32_t dim,
                       const int32_t *n_cells, const float *origin, float cell_size, const float *q_pos,
                       const int32_t *q_cell, int64_t m, int32_t k, int64_t *out, void *stream);

/* The same two searches in the WRAPPED metric of a domain that is periodic along some axes (csrc/knn_periodic.hip; the search under
 * the periodic sampler, jet and tracers).  This is the library's own metric, not the chord embedding connect_knn ranks by.
 *
 * Axis a is periodic when period[a] > 0 (0: not periodic).  With o = origin[a] (the cloud's minimum) and L = period[a] >= the cloud's
 * extent, every cloud coordinate lies in [o, o + L].  All of the following is fixed, so that a numpy loop repeats it bit for bit:
 *   wrap      a QUERY coordinate q (a particle's; never a cloud point's) is first brought into [o, o + L) in fp32, every operation
 *             rounded once and nothing contracted:  f = floorf((q − o) / L);  w = q − (f · L);  if (w < o) w = w + L;
 *             if (w >= o + L) w = w − L   (o + L rounded to fp32).  A self search takes the cloud's points as they are.
 *             The result is ALWAYS finite: where the sequence gives no finite number (q not finite, or q − o, (q − o) / L or f · L
 *             overflows — with L < 1 a finite |q − o| above FLT_MAX · L does) w = o.  A search from a wrapped coordinate therefore
 *             has finite distances to every point and returns k indices whenever n >= k: no row holds −1 because of a periodic
 *             axis.  The wrap is exact to the fp32 resolution of (q − o) / L: beyond |q − o| ~ 2^24 L the rounded product is whole
 *             periods off and w, though finite, lies outside [o, o + L) — the neighbours are then those of that w.
 *   offset    from q to p, both widened to fp64: t = p − q, then t − L if t > L / 2, t + L if t < −L / 2 (strict; connect_knn's rule),
 *             applied once.  A non-periodic axis: t = p − q.
 *   distance  the fp64 sum over the axes of t², as g4c_knn_grid forms it.
 * Images of two points that coincide are duplicates, as duplicated points are in g4c_knn_grid.
 *
 * The grid: a periodic axis is tiled exactly, n_cells[a] cells of cell[a] = L / n_cells[a] (fp64); a non-periodic axis has cells of
 * the caller's size from origin[a], as g4c_knn_grid's.  The cell of a coordinate x is floor((x − origin[a]) / cell[a]) in fp64, clamped
 * to 0 .. n_cells[a] − 1; the caller sorts the cloud by it (cell id = x + n_cells[0]*(y + n_cells[1]*z)); the queries' cells are formed
 * on the device, after the wrap.  Ring R scans the min(2R + 1, n_cells[a]) distinct cells c − R .. c + R modulo n_cells[a] of a periodic
 * axis, and the search ends when the k-th distance is inside the nearest face of the block that has cells behind it (both faces of a
 * periodic axis until 2R + 1 >= n_cells[a]) or the block is the whole grid.  Exact; ties follow the scan order.
 * pos_sorted, order, cell_start, out: as g4c_knn_grid[_query].  Limits: dim 2 or 3, k <= 16, n < 2^31; self n > k, query n >= k. */
typedef struct g4c_periodic_grid {
    int32_t n_cells[3];          /* unused axes: 1 */
    float origin[3];             /* the cloud's minimum along each axis */
    float period[3];             /* L per axis; 0: the axis is not periodic */
    double cell[3];              /* the cell size per axis */
} g4c_periodic_grid_t;
int g4c_knn_grid_periodic(const float *pos_sorted, const int32_t *order, const int32_t *cell_start, int64_t n, int32_t dim,
                          const g4c_periodic_grid_t *grid /*host*/, int32_t k, int64_t *out, void *stream);
int g4c_knn_grid_query_periodic(const float *pos_sorted, const int32_t *order, const int32_t *cell_start, int64_t n, int32_t dim,
                                const g4c_periodic_grid_t *grid /*host*/, const float *q_pos, int64_t m, int32_t k, int64_t *out,
                                void *stream);

/* ---------------------------------------------------------------- rollout (nn/model.py:303-327)
 * One step's bookkeeping without host involvement: t = *step;
 * outputs[:, nf*t : nf*(t+1)] = pred;  field = roll(field, -nf, dim=1); field[:, -nf:] = pred;
 * then step[0] = t + 1, written by the last workgroup of the launch to finish.  `step` points to TWO int32: [0] the step index, [1] a
 * ticket counter the launch uses for that (zero before the first launch; it leaves it zero).
 * out_ld == 0: `outputs` is step-major, [steps][n_nodes][nf] contiguous — outputs[t] = pred (one contiguous block per step; the
 * caller transposes once at the end of the rollout). */
int g4c_rollout_advance(float *field, int32_t field_cols, const float *pred, int32_t nf,
                        float *outputs, int32_t out_ld, int32_t *step, int64_t n_nodes, void *stream);

/* The recording form of the launch above (csrc/rollout_record.hip): everything g4c_rollout_advance does to `field` and `step`, and,
 * addressed by the step index t the launch reads on the device, up to three records of the step — no `outputs` buffer of every step
 * is needed.  The descriptor is read on the host and travels with the launch by value (a captured launch carries it).
 * A step index outside [0, max_steps), or a snapshot slot >= n_snap, leaves no record; field and step advance all the same, and no
 * probe row outside [0, n_nodes) is read.  n_nodes == 0 advances the step and records nothing.
 * Statistics (target != NULL, 1 <= nf <= 8, G4C_EUNSUPPORTED above): with d = (double)pred - (double)target[:, nf t + f], per field f
 * stats[t][f] = { sum d^2, sum |d|, max |d|, sum y, sum y^2, sum |d| over the rows with mask != 0 } (y = the target), accumulated in
 * fp64 without floating-point atomics in an order that depends on (n_nodes, nf) alone: bit-identical between runs and between captured
 * and eager launches.  stats[t] is overwritten.  The workgroups' partials go through `scratch` and are combined by a second, one-
 * workgroup launch on the same stream (g4c::partials_kernel, csrc/step_record.h).
 * NON-FINITE SAMPLES (the rule of every in-step diagnostic): (1) sums follow IEEE — NaN where a NaN or an Inf − Inf
 * entered; (2) an extremum over samples of which one is NaN IS NaN, at every stage of the reduction (±Inf are ordinary values): a
 * record never reads better than the rollout was; (3) masks select — a row outside `mask` contributes nothing to
 * G4C_REC_ABS_ERR_MASK, whatever it holds; (4) a poisoned value changes only the outputs that depend on it. */
typedef struct g4c_rollout_rec {
    int32_t max_steps;           /* capacity of probe_out / stats / target, in steps */
    /* snapshots: step t (0-based) is kept iff every > 0 and (t + 1) % every == 0, in slot (t + 1) / every - 1, while slot < n_snap */
    float  *snap;                /* [n_snap][n_nodes][nf], step-major like `outputs` with out_ld == 0; NULL iff every == 0 (or n_snap == 0) */
    int32_t every, n_snap;
    /* probes: rows probe_rows[0 .. n_probe) of every step */
    const int32_t *probe_rows;   /* NULL iff n_probe == 0 */
    int32_t n_probe;
    float  *probe_out;           /* [max_steps][n_probe][nf] */
    /* error statistics of every step against target[:, nf t : nf (t + 1)] */
    const float *target;         /* [n_nodes, target_ld], target_ld >= nf * max_steps; NULL: no statistics */
    int32_t target_ld;
    const uint8_t *mask;         /* [n_nodes] or NULL: the subset for G4C_REC_ABS_ERR_MASK (Dirichlet nodes) */
    double *stats;               /* [max_steps][nf][G4C_REC_NSTAT] */
    double *scratch;             /* g4c_rollout_record_scratch_doubles(n_nodes, nf) doubles */
} g4c_rollout_rec_t;
/* G4C_REC_MAX_ABS_ERR is NaN when |d| is NaN at any node (not the maximum over the other nodes); +Inf when the largest |d| is. */
enum { G4C_REC_SQ_ERR, G4C_REC_ABS_ERR, G4C_REC_MAX_ABS_ERR, G4C_REC_TGT_SUM, G4C_REC_TGT_SQ_SUM, G4C_REC_ABS_ERR_MASK, G4C_REC_NSTAT };
/* Size of `scratch` in doubles (host; negative G4C_E* code for n_nodes < 0, nf < 1 or nf > 8). */
int64_t g4c_rollout_record_scratch_doubles(int64_t n_nodes, int32_t nf);
int g4c_rollout_advance_record(float *field, int32_t field_cols, const float *pred, int32_t nf, const g4c_rollout_rec_t *rec /*host*/,
                               int32_t *step, int64_t n_nodes, void *stream);

/* Time statistics of a rollout at every node (csrc/rollout_moments.hip): one launch per step, AFTER the forward and BEFORE the step's
 * closing launch above (which bumps the step index this one reads, t = step[0], on the same stream).  Writes neither field nor step.
 * The sample of node n and field f is x = (double)pred[n nf + f], or, with `sub`, x = (double)pred[n nf + f] - (double)sub[n sub_ld +
 * nf t + f] (statistics of the error against a target).  Step t is accumulated iff 0 <= t < max_steps, t >= origin and (t - origin) %
 * stride == 0, origin = window[0] read on the device (a captured launch follows a rewritten origin); an accumulated step leaves
 * window[1] = t, any other step touches nothing.  At t == origin the accumulators are STORED, not read: pivot = lo = hi = x, sum =
 * sum2 = 0 (no memset is ever needed; running through the origin again replaces the record).  On later steps, with d_f = x_f - pivot_f:
 * sum_f += d_f, sum2_fg += d_f d_g (the product rounded to fp64 once, then added: no fused multiply-add), lo = min(lo, x),
 * hi = max(hi, x), both NaN once either argument is (not fmin / fmax: after a NaN sample lo and hi of that node and field are NaN,
 * as its sums are, and stay NaN until the origin is run through again; ±Inf are ordinary values).  Every accumulator receives one add per accumulated step, in time order, from one thread: the bits are a function
 * of the data alone (no atomics, nothing depends on the grid).
 * All accumulators are fp64 and plane-major: plane p of node n at base[p * plane_ld + n], plane_ld >= n_nodes.  sum2 holds the
 * nf (nf + 1) / 2 pairs f <= g in the order (0,0), (0,1), ..., (0,nf-1), (1,1), ...   nf = 1 .. 8 (G4C_EUNSUPPORTED above).
 * n_nodes == 0 launches nothing and succeeds. */
typedef struct g4c_rollout_moments {
    int32_t max_steps;           /* capacity of the rollout (and of `sub`), in steps */
    int32_t stride;              /* >= 1 */
    int32_t *window;             /* device, {origin, last} */
    const float *sub;            /* [n_nodes, sub_ld], sub_ld >= nf * max_steps, or NULL */
    int32_t sub_ld;
    int64_t plane_ld;
    double *pivot, *sum, *sum2, *lo, *hi;       /* nf, nf, nf (nf + 1) / 2, nf, nf planes */
} g4c_rollout_moments_t;
int g4c_rollout_moments(const float *pred, int32_t nf, const g4c_rollout_moments_t *m /*host*/, const int32_t *step, int64_t n_nodes,
                        void *stream);

/* Fourier modes of a rollout at every node (csrc/rollout_spectrum.hip): a discrete Fourier transform at n_bins chosen frequencies,
 * accumulated per node and field inside the step.  One launch per step and accumulator set, AFTER the forward (and after
 * g4c_mesh_derived for derived columns) and BEFORE the step's closing launch (which bumps the step index this one reads, t = step[0],
 * on the same stream).  Writes neither x nor step.
 * The sample of node n and field f < nf is x_f = (double)x[n x_ld + x_step t + f]: the prediction has x_ld = nf, x_step = 0; a target
 * [n_nodes, >= nf max_steps] has x_ld = its row stride and x_step = nf (the spectrum of the ground truth, by the same code).
 * With origin = window[0] read on the device (a captured launch follows a rewritten origin) and j = (t - origin) / stride, step t is
 * accumulated iff n_nodes > 0, 0 <= t < max_steps, t >= origin, (t - origin) % stride == 0 and j < n_samples; an accumulated step
 * leaves window[1] = t, any other step touches nothing.
 * The twiddles are an input: tw is a device fp64 table [n_samples, n_bins, 2]; row j, bin k holds (w_j cos th_jk, -w_j sin th_jk), built
 * on the host (the kernel calls no sin / cos, and any table will do).  At j == 0 the accumulators are STORED, not read: pivot = x,
 * sum = re = im = 0 (no memset is ever needed; running through the origin again replaces the record).  At j > 0, with d_f = x_f -
 * pivot_f: sum_f += d_f, re_fk += d_f tw[j,k,0], im_fk += d_f tw[j,k,1] (each product rounded to fp64 once, then added: no fused
 * multiply-add).  Every accumulator receives one add per accumulated step, in time order, from one thread: the bits are a function of
 * the data and the table alone (no atomics, nothing depends on the grid).
 * All accumulators are fp64 and plane-major: plane p of node n at base[p * plane_ld + n], plane_ld >= n_nodes.  pivot and sum have nf
 * planes, re and im nf n_bins planes each, plane f n_bins + k.  nf = 1 .. 8, n_bins = 1 .. 64 (G4C_EUNSUPPORTED above).
 * n_nodes == 0 launches nothing and succeeds. */
typedef struct g4c_rollout_spectrum {
    int32_t max_steps;           /* capacity of the rollout (and of a target `x`), in steps */
    int32_t stride;              /* >= 1 */
    int32_t n_samples;           /* >= 1: rows of `tw` */
    int32_t n_bins;              /* K */
    int32_t *window;             /* device, {origin, last} */
    const double *tw;            /* device, [n_samples, n_bins, 2] */
    int32_t x_ld;                /* >= nf; >= nf * max_steps with x_step == nf */
    int32_t x_step;              /* 0 or nf */
    int64_t plane_ld;
    double *pivot, *sum, *re, *im;              /* nf, nf, nf n_bins, nf n_bins planes */
} g4c_rollout_spectrum_t;
int g4c_rollout_spectrum(const float *x, int32_t nf, const g4c_rollout_spectrum_t *s /*host*/, const int32_t *step, int64_t n_nodes,
                         void *stream);

/* Segment-averaged spectra of a rollout at every node (csrc/rollout_welch.hip): Welch's estimator of the power spectrum, and of the
 * cross-spectrum with a reference signal, at n_bins chosen frequencies.  One call per step and spectrum, behind g4c_rollout_spectrum
 * and BEFORE the step's closing launch; it enqueues two kernels (accumulate, close), reads t = step[0] and origin = window[0] on the
 * device, synchronises nothing, allocates nothing, and writes neither x nor step.  The sample x_f is that of g4c_rollout_spectrum
 * (x_ld, x_step).  Step t is sample j = (t - origin) / stride iff 0 <= t < max_steps, t >= origin and (t - origin) % stride == 0; any
 * other step touches nothing.  Sample j is position q = j - s hop of segment s when 0 <= q < seg_len; hop == seg_len (no overlap) or
 * 2 hop == seg_len (half overlap): one or two segments.  Segment s lives in accumulator set c = s & 1: pivot and sum have 2 nf planes
 * (plane c nf + f), re and im 2 nf n_bins (plane (c nf + f) n_bins + k).
 * Accumulate: at q == 0 the set is STORED, pivot = x, sum = re = im = 0; else d = x - pivot, sum += d, re_fk += d tw[q,k,0], im_fk +=
 * d tw[q,k,1] (tw: device fp64 [seg_len, n_bins, 2], any table will do); it leaves window[1] = t.
 * Close: acts only when j is the last sample of a segment, j >= seg_len - 1 and (j - (seg_len - 1)) % hop == 0, s = (j - (seg_len - 1)) /
 * hop.  With W[k] = Σ_q tw[q,k] (device fp64 [n_bins, 2], summed on the host) and inv_L = 1.0 / seg_len:
 *   m = sum_f inv_L;  ar = re_fk - m W[k,0];  ai = im_fk - m W[k,1];  p = ar ar + ai ai;  pxx_fk = (s == 0) ? p : pxx_fk + p
 * and, with a reference (ref_sum / ref_re / ref_im: the two sets of an accumulator of the same nf, n_bins and plane_ld — this one's own
 * or one an earlier call of the step accumulated; ref_row >= 0: that row for every row, < 0: the same row; ref_field >= 0: that field
 * for every field, < 0: the same field), (rr, ri) the same (ar, ai) of the reference's set s & 1,
 *   cr = ar rr + ai ri;  ci = ai rr - ar ri  (X conj R);  cxr_re_fk, cxr_im_fk = (s == 0) ? cr, ci : + cr, ci
 * and, for each of n_track rows track[p] (device; track_host: the same on the host, checked here) and s < max_segments,
 * seg_power[s][p][f][k] = p of that row; it leaves window[2] = s + 1.  A last partial segment is never closed.
 * Every operation above is rounded to fp64 on its own (no fused multiply-add), every accumulator belongs to one thread: the bits are
 * a function of the data and the tables alone.  NaN and inf follow IEEE: a poisoned sample poisons its row and field of its
 * segment(s) and from there its pxx; a poisoned reference every cxr and no pxx.
 * All planes are fp64, plane p of node n at base[p * plane_ld + n], plane_ld >= n_nodes; pxx, cxr_re, cxr_im have nf n_bins planes.
 * nf = 1 .. 8, n_bins = 1 .. 64, n_track <= 1024, hop in {seg_len, seg_len / 2} (G4C_EUNSUPPORTED); seg_len >= 2, track rows in range,
 * x_step in {0, nf} (G4C_EINVAL), all before any launch.  n_nodes == 0 launches nothing and succeeds. */
typedef struct g4c_rollout_welch {
    int32_t max_steps;           /* capacity of the rollout (and of a target `x`), in steps */
    int32_t stride;              /* >= 1 */
    int32_t seg_len;             /* L >= 2: rows of `tw` */
    int32_t hop;                 /* H: L or L / 2 */
    int32_t n_bins;              /* K */
    int32_t x_ld;                /* >= nf; >= nf * max_steps with x_step == nf */
    int32_t x_step;              /* 0 or nf */
    int32_t ref_row, ref_field;  /* >= 0: one row / field of the reference for all; < 0: the same row / field */
    int32_t n_track;             /* P */
    int32_t max_segments;        /* leading extent of seg_power */
    int32_t *window;             /* device, {origin, last, closed} */
    const double *tw;            /* device, [seg_len, n_bins, 2] */
    const double *W;             /* device, [n_bins, 2] */
    double inv_L;                /* 1.0 / seg_len */
    int64_t plane_ld;
    double *pivot, *sum, *re, *im;              /* 2 nf, 2 nf, 2 nf n_bins, 2 nf n_bins planes */
    double *pxx;                                /* nf n_bins planes */
    double *cxr_re, *cxr_im;                    /* nf n_bins planes each, or NULL without a reference */
    const double *ref_sum, *ref_re, *ref_im;    /* the reference's sets, or NULL */
    const int32_t *track;        /* device, [n_track] */
    const int32_t *track_host;   /* host, [n_track]: the same rows */
    double *seg_power;           /* device, [max_segments, n_track, nf, n_bins] */
} g4c_rollout_welch_t;
int g4c_rollout_welch(const float *x, int32_t nf, const g4c_rollout_welch_t *s /*host*/, const int32_t *step, int64_t n_nodes, void *stream);

/* A least-squares gradient over the in-edges of a mesh, and the flow diagnostics of a rollout built on it (csrc/mesh_gradient.hip).
 *
 * g4c_mesh_gradient_weights — once per mesh.  Edges grouped by receiver: the s-th in-edge of node i is edge pe = perm[off[i] + s]
 * (perm == NULL: pe = off[i] + s) of the caller's numbering; src32[E] its senders, rel[E, dim] fp32 its vectors receiver − sender
 * (the sign of `edge_attr`).  Per node i, over its in-edges in that order, in fp64: d_e = −rel_e, w_e = |d_e|^(−power) (power 0, 1
 * or 2), M = Σ w_e d_e d_eᵀ.  The node is DEGENERATE iff not det M > 1e-12 (tr M / dim)^dim — that is det M <= the threshold, or a
 * determinant that is no number (a zero-length edge has no weight under power >= 1): fewer than dim in-edges, collinear / coplanar
 * neighbours.  Then every g_e = 0 and degenerate[i] = 1; otherwise g_e = w_e M⁻¹ d_e, M⁻¹ = adj M / det M in closed form, rounded to
 * fp32 once, so that  grad x (i) = Σ_e g_e (x[src_e] − x[i])  is exact on linear fields.
 * Outputs in CSR order (position off[i] + s): g[E, dim] fp32, src[E] = src32[pe] (the permutation is resolved here), and
 * degenerate[n_nodes].  n_nodes == 0 or n_edges == 0 launches nothing, writes nothing and succeeds.  dim 2 or 3 (G4C_EUNSUPPORTED). */
int g4c_mesh_gradient_weights(const int32_t *off, const int32_t *perm /*or NULL*/, const int32_t *src32, const float *rel, int32_t dim,
                              int32_t power, int64_t n_nodes, int64_t n_edges, float *g, int32_t *src, uint8_t *degenerate, void *stream);

/* g4c_mesh_derived — once per step, AFTER the forward and BEFORE the step's closing launch (it reads the step index t = step[0] and
 * never writes it).  A program of nd <= 8 columns, each the sum of 1 .. 3 terms coef · ∂_axis x[:, field] (more: G4C_EUNSUPPORTED; a
 * program may name at most 8 distinct fields).  fp32, no contraction, in this order: for every field f the program names and every
 * axis a, G[f][a] = 0, then over the in-edges e of node i in CSR order diff = x[src_e, f] − x[i, f], p = g[e][a] · diff (rounded),
 * G[f][a] += p; column c = (coef₀ G₀ + coef₁ G₁) + coef₂ G₂ with every product rounded and the terms added left to right from the
 * first.  One thread per node: the bits are a function of the data alone, and a numpy.float32 loop reproduces them.
 * cur[n_nodes, nd] is written on every call.  If every > 0, (t + 1) % every == 0 and slot = (t + 1) / every − 1 < n_snap (t >= 0), the
 * same values go to snap[slot][n_nodes][nd] (the records' slot convention).  If stats != NULL and 0 <= t < max_steps, stats[t][c] =
 * {Σq², Σ|q|, max|q|} over the nodes in fp64 — OVERWRITTEN, never accumulated — by the records' rule: register accumulators, rows dealt
 * gid, gid + grid, ... over at most 1024 workgroups of 256, a xor butterfly per wave, the waves in order through LDS, one partial set
 * per workgroup into `scratch` (g4c_mesh_derived_scratch_doubles doubles), and a second one-workgroup launch that adds the partials
 * in a fixed order.  No floating-point atomics: the bits are the same on every run.
 * G4C_EINVAL before any launch: a field or axis out of range, negative sizes, x_ld < nf, a column without terms, records without
 * their buffers.  n_nodes == 0 launches nothing and succeeds. */
#define G4C_DERIVED_MAX_COLS 8
#define G4C_DERIVED_MAX_TERMS 3
/* G4C_DERIVED_MAX_ABS is NaN when q is NaN at any node (the records' rule for non-finite samples, above), as the two sums are. */
enum { G4C_DERIVED_SQ, G4C_DERIVED_ABS, G4C_DERIVED_MAX_ABS, G4C_DERIVED_NSTAT };
typedef struct g4c_derived_program {
    int32_t nd;
    int32_t n_terms[G4C_DERIVED_MAX_COLS];
    int32_t field[G4C_DERIVED_MAX_COLS][G4C_DERIVED_MAX_TERMS];
    int32_t axis[G4C_DERIVED_MAX_COLS][G4C_DERIVED_MAX_TERMS];
    float coef[G4C_DERIVED_MAX_COLS][G4C_DERIVED_MAX_TERMS];
} g4c_derived_program_t;
typedef struct g4c_mesh_derived {
    int32_t dim, nf, x_ld;       /* x[n_nodes, x_ld] fp32, its first nf columns are the fields */
    const float *g;              /* [E, dim], CSR order (g4c_mesh_gradient_weights); NULL, with src, for a mesh without edges */
    const int32_t *src;          /* [E], CSR order */
    const int32_t *off;          /* [n_nodes + 1] */
    float *cur;                  /* [n_nodes, nd] */
    const int32_t *step;         /* device; may be NULL without snap and stats */
    int32_t every, n_snap, max_steps;
    float *snap;                 /* [n_snap][n_nodes][nd] or NULL */
    double *stats;               /* [max_steps][nd][G4C_DERIVED_NSTAT] or NULL */
    double *scratch;             /* g4c_mesh_derived_scratch_doubles(n_nodes, nd) doubles, with stats */
} g4c_mesh_derived_t;
int64_t g4c_mesh_derived_scratch_doubles(int64_t n_nodes, int32_t nd);
int g4c_mesh_derived(const float *x, const g4c_mesh_derived_t *d /*host*/, const g4c_derived_program_t *prog /*host*/, int64_t n_nodes,
                     void *stream);

/* g4c_mesh_derived_adjoint — the transpose of g4c_mesh_derived's map x -> cur (the map is linear: its backward).  With
 * G_i[f][a] = Σ_{e in in(i)} g[e][a] (x[src_e, f] − x[i, f]) and cur[i, c] = Σ_k coef[c][k] G_i[row(c, k)], for gy[n_nodes, nd] (dense):
 *   H_i[f][a] = Σ_{(c, k): row(c, k) = (f, a)} coef[c][k] gy[i, c]
 *   gx[j, f]  = Σ_{e: src_e = j} Σ_a g[e][a] H_{dst_e}[f][a]  −  Σ_{e in in(j)} Σ_a g[e][a] H_j[f][a]
 * A scatter to the senders, taken as a gather: ONE thread per node j walks j's out-edges through a sender-side CSR built once per
 * mesh.  With perm the CSR positions e grouped by sender, ASCENDING within a sender (a stable grouping of src), and dst[e] the
 * receiver of position e (`off` expanded): out_off[n_nodes + 1] the offsets of that grouping, out_g[E, dim] = g[perm[q]] and
 * out_dst[E] = dst[perm[q]] the weights and receivers copied into its order — so the walk streams them as the forward streams g and
 * src, and only the receiver's row of gy is a gather.  fp32, no contraction, every product rounded before it is added, in this order:
 *   H_i[f][a] = +0, then += coef[c][k] · gy[i, c] over the terms that pick (f, a), in program order (c ascending, then k);
 *   acc[f] = +0; over j's out-edges q = out_off[j] .. (ascending CSR position), i = out_dst[q]: for every field f the program names,
 *   for a = 0 .. dim − 1: acc[f] += out_g[q][a] · H_i[f][a]; then over j's own in-edges e = off[j] .. in CSR order, for a = 0 ..
 *   dim − 1: acc[f] −= g[e][a] · H_j[f][a].
 * No atomics, no reduction across threads: the bits are a function of the data alone, and a numpy.float32 loop reproduces them.
 * EVERY column of gx[n_nodes, nf] (dense) is written: a field the program does not differentiate gets +0.  n_edges == 0 still zero-fills
 * gx (the tables may then be NULL); n_nodes == 0 launches nothing.  The tables are trusted as g4c_mesh_derived trusts src: out_dst in
 * [0, n_nodes), both offset arrays ascending from 0 to n_edges.
 * G4C_EINVAL before any launch: null pointers, negative sizes, gx == gy (or overlapping), a field or axis out of range, a column
 * without terms; G4C_EUNSUPPORTED: dim not 2 or 3, nd > 8, more than 3 terms, more than 8 distinct fields. */
int g4c_mesh_derived_adjoint(const float *gy, const g4c_derived_program_t *prog /*host*/, int32_t dim, int32_t nf, const float *g,
                             const int32_t *off, const float *out_g, const int32_t *out_dst, const int32_t *out_off,
                             int64_t n_nodes, int64_t n_edges, float *gx, void *stream);

/* First and second derivatives on the mesh: a weighted least-squares fit of a quadratic through the node's own value, over a
 * stencil the caller brings — the mesh's in-edges or a wider one (csrc/mesh_jet.hip).  Q = dim + dim (dim + 1) / 2 unknowns per node
 * (5 or 9): the first derivatives 0 .. dim − 1, then the second ones xx, xy, yy (2-D) or xx, xy, xz, yy, yz, zz (3-D).
 *
 * g4c_mesh_jet_weights — once per mesh.  The stencil in CSR form exactly as g4c_mesh_gradient_weights takes the in-edges: the s-th
 * entry of node i is pe = perm[off[i] + s] (perm == NULL: off[i] + s), src32[S] the senders, rel[S, dim] fp32 receiver − sender.  One
 * thread per node, fp64, no contraction, in this order.  Per entry: d = −rel, r² = Σ_a d_a d_a from 0, w = 1, 1 / sqrt(r²) or 1 / r²
 * (power 0, 1, 2); the row b = (d_0 .., then for a <= b' in the order above t = d_a d_b', halved where a == b'), so that for a quadratic
 * x[src] − x[i] = Σ_q b_q jet_q.  The normal matrix, lower triangle, A_ij += (w b_i) b_j over the entries in CSR order.  Scaled to a
 * unit diagonal: sc_i = 1 / sqrt(A_ii), A_ij <- (A_ij sc_i) sc_j.  Cholesky L Lᵀ = A by columns j = 0 .. Q − 1: pivot_j = A_jj − L_j0² −
 * .. − L_j,j−1² (subtracted one by one), L_jj = sqrt(pivot_j), inv_j = 1 / L_jj, and for i > j  L_ij = (A_ij − L_i0 L_j0 − ..) inv_j.  Per
 * entry then y_i = (b_i sc_i − L_i0 y_0 − .. − L_i,i−1 y_i−1) inv_i for i ascending, z_i = (y_i − L_i+1,i z_i+1 − .. − L_Q−1,i z_Q−1) inv_i
 * for i descending, and c[s][i] = (float)((w sc_i) z_i).  The node is DEGENERATE — every c of it +0, degenerate[i] = 1 — iff it has
 * fewer than Q entries, or a weight is not finite (a zero-length vector under power >= 1), or some pivot is not > 1e-12 (that is <=
 * the threshold, or no number): the threshold sits on the unit-diagonal matrix, where it is invariant under x -> λx.
 * Outputs in CSR order: c[S, Q] fp32 with jet(i) = Σ_s c[s] (x[src_s] − x[i]), src[S] = src32[pe], degenerate[n_nodes].  n_nodes == 0
 * or n_entries == 0 launches nothing, writes nothing and succeeds.  dim 2 or 3 (G4C_EUNSUPPORTED); power outside 0 .. 2, negative
 * sizes, null pointers: G4C_EINVAL before any launch. */
#define G4C_JET_MAX_FIELDS 4
int g4c_mesh_jet_weights(const int32_t *off, const int32_t *perm /*or NULL*/, const int32_t *src32, const float *rel, int32_t dim,
                         int32_t power, int64_t n_nodes, int64_t n_entries, float *c, int32_t *src, uint8_t *degenerate, void *stream);

/* g4c_mesh_jet — per call: out[n_nodes, nd] (dense) from x[n_nodes, x_ld] (its first nf columns are the fields) by a program as
 * g4c_mesh_derived's, whose `axis` ranges over 0 .. Q − 1: 0 .. dim − 1 the first derivatives, dim .. Q − 1 the second ones in the
 * order above.  nd <= 8 columns of 1 .. 3 terms, at most G4C_JET_MAX_FIELDS distinct fields (more: G4C_EUNSUPPORTED).  fp32, no
 * contraction, one thread per node: for every field f the program names and q = 0 .. Q − 1, J[f][q] = 0, then over the entries e of
 * node i in CSR order diff = x[src_e, f] − x[i, f], p = c[e][q] · diff (rounded), J[f][q] += p; column = (coef₀ J₀ + coef₁ J₁) + coef₂ J₂
 * with every product rounded and the terms added left to right from the first.  A numpy.float32 loop reproduces the bits.  No step
 * index, snapshots or statistics: this launch is not part of the rollout.  n_nodes == 0 launches nothing; an empty stencil
 * (n_entries == 0; c and src may be NULL) writes zeros.  G4C_EINVAL before any launch: null pointers, negative sizes, x_ld < nf, a
 * field or derivative out of range, a column without terms. */
int g4c_mesh_jet(const float *x, int32_t x_ld, int32_t nf, int32_t dim, const float *c, const int32_t *src, const int32_t *off,
                 const g4c_derived_program_t *prog /*host*/, int64_t n_nodes, int64_t n_entries, float *out, void *stream);

/* g4c_mesh_jet_adjoint — the transpose of g4c_mesh_jet's map x -> out, in g4c_mesh_derived_adjoint's form and order with Q in the
 * place of dim: H_i[f][q] = +0, then += coef[c][k] · gy[i, c] over the terms that pick (f, q) in program order; acc[f] = +0; over the
 * entries node j SENDS, by ascending CSR position (out_off[n_nodes + 1], out_c[S, Q] = c[perm[·]], out_dst[S] — the sender-side
 * tables, built once per operator), for q = 0 .. Q − 1: acc[f] += out_c[·][q] · H_dst[f][q]; then over j's own entries in CSR order,
 * for q = 0 .. Q − 1: acc[f] −= c[e][q] · H_j[f][q].  No atomics.  EVERY column of gx[n_nodes, nf] is written: a field the program does
 * not name gets +0; n_entries == 0 zero-fills gx (the tables may be NULL); n_nodes == 0 launches nothing.  G4C_EINVAL before any
 * launch: null pointers, negative sizes, gx overlapping gy, a field or derivative out of range; G4C_EUNSUPPORTED as g4c_mesh_jet. */
int g4c_mesh_jet_adjoint(const float *gy, const g4c_derived_program_t *prog /*host*/, int32_t dim, int32_t nf, const float *c,
                         const int32_t *off, const float *out_c, const int32_t *out_dst, const int32_t *out_off, int64_t n_nodes,
                         int64_t n_entries, float *gx, void *stream);

/* g4c_body_forces (csrc/body_forces.hip) — the force of a 2-D flow on the bodies it passes, once per step: AFTER the forward and
 * BEFORE the step's closing launch (it reads the step index t = step[0] and never writes it; with step == NULL, t = t0).  A body's
 * wall is a closed polygon of W_b items, each a mesh node with an area vector (the outward normal times the length lumped at the
 * node), a unit normal and a moment arm, all fp64 and built once by the caller; the items of body b are item[body_off[b] ..
 * body_off[b + 1]).  The fields are x[i, col] (x_step == 0: a prediction) or x[i, x_step t + col] (x_step = nf: a target holding
 * every step's columns; a step outside 0 <= t < max_steps then reads and writes nothing).
 * For item w at node i = item[w], no contraction anywhere (every product is rounded before it is added):
 *   1. fp32, as g4c_mesh_derived: G[f][a] = 0 for f = u, v and a = 0, 1, then over the in-edges e of i in CSR order
 *      diff = x[src_e, f] − x[i, f], p = g[e][a] · diff, G[f][a] += p — bit for bit that launch's 'grad:u', 'grad:v' at row i (zero
 *      at a degenerate node).  Skipped entirely when mu == 0: the velocity columns are then not read.
 *   2. fp64: P = p_scale (double)x[i, pcol] + p_shift; sxx = 2 u_scale G[u][0], sxy = u_scale G[u][1] + v_scale G[v][0],
 *      syy = 2 v_scale G[v][1]; with a = area[w], r = arm[w], n̂ = unit[w], t̂ = (−n̂_y, n̂_x):
 *      pressure traction tp = (−P a_x, −P a_y); viscous traction tv = mu (sxx a_x + sxy a_y, sxy a_x + syy a_y);
 *      the moments r_x t_y − r_y t_x of each;
 *      wall[w] = ((float)P, (float)(mu ((t̂_x sxx + t̂_y sxy) n̂_x + (t̂_x sxy + t̂_y syy) n̂_y))), written on every call (if not NULL).
 *   3. per body the six sums {Fp_x, Fp_y, Fv_x, Fv_y, Mp, Mv} by the records' rule with ONE workgroup of 256 per body: thread tid
 *      adds the items tid, tid + 256, ... of its body, in that order, into fp64 registers; a 6-level xor butterfly per wave; the four
 *      waves in order through LDS.  If stats != NULL and 0 <= t < max_steps, stats[t][b] = the six sums — OVERWRITTEN, never
 *      accumulated; any other t writes no stats.  cur[b] = ((float)(Fp_x + Fv_x), (float)(Fp_y + Fv_y), (float)(Mp + Mv)), each
 *      sum formed in fp64 first, is written on every call.
 * Plain loads and stores, no atomics, nothing passes between workgroups: the bits are a function of the data alone.  Every item
 * must be a row of x (not checked on the device).
 * G4C_EINVAL before any launch: negative sizes, a column out of range (negative, or >= x_step when x_step != 0), x_ld below a
 * column the launch reads, mu != 0 without g / src / off, stats (or x_step != 0) without max_steps, a null pointer.  n_bodies == 0
 * or n_items == 0 launches nothing, writes nothing and succeeds. */
enum { G4C_FORCES_FPX, G4C_FORCES_FPY, G4C_FORCES_FVX, G4C_FORCES_FVY, G4C_FORCES_MP, G4C_FORCES_MV, G4C_FORCES_NSUM };
typedef struct g4c_body_forces {
    const float *x;              /* [n_nodes, x_ld] fp32 */
    int32_t x_ld, x_step;        /* x_step 0: the fields are columns pcol, ucol, vcol; nf: columns nf t + pcol, .. of a target */
    const int32_t *step;         /* device; NULL: t = t0 */
    int32_t t0;
    int32_t pcol, ucol, vcol;    /* ucol, vcol are not read when mu == 0 */
    double mu, p_scale, p_shift, u_scale, v_scale;
    const float *g;              /* [E, 2], CSR order (g4c_mesh_gradient_weights); may be NULL, with src and off, when mu == 0 */
    const int32_t *src;          /* [E], CSR order */
    const int32_t *off;          /* [n_nodes + 1] */
    const int32_t *item;         /* [n_items] node rows, body after body, each body in counter-clockwise order */
    const int32_t *body_off;     /* [n_bodies + 1] */
    const double *area;          /* [n_items, 2] */
    const double *unit;          /* [n_items, 2] */
    const double *arm;           /* [n_items, 2] */
    double *stats;               /* [max_steps][n_bodies][G4C_FORCES_NSUM] or NULL */
    float *cur;                  /* [n_bodies, 3] */
    float *wall;                 /* [n_items, 2] or NULL */
    int32_t max_steps;
} g4c_body_forces_t;
int g4c_body_forces(const g4c_body_forces_t *bf /*host*/, int64_t n_bodies, int64_t n_items, void *stream);

/* g4c_body_forces_adjoint — the transpose of the linear part of g4c_body_forces' map x -> (the six sums per body, wall[W, 2]): its
 * backward (p_shift drops out; the (float) casts of wall count as the identity).  Inputs gF[n_bodies, 6] fp64 and gwall[n_items, 2]
 * fp32, either may be NULL (zeros); output gx[n_nodes, nf] fp32, dense.  Two launches on the same stream, no contraction anywhere
 * (every product is rounded before it is added):
 *   1. per wall item w of body b = item_body[w], ONE thread, fp64, staged into hw[n_items, 5] fp32 = (H_w[u][0], H_w[u][1], H_w[v][0],
 *      H_w[v][1], cp_w).  With a = area[w], r = arm[w], n̂ = unit[w], t̂ = (−n̂_y, n̂_x), gs = (double)gwall[w][1]:
 *        A   = gF[b][FVX] − r_y·gF[b][MV]                    Bc = gF[b][FVY] + r_x·gF[b][MV]
 *        dxx = mu·(A·a_x + gs·(t̂_x·n̂_x))
 *        dxy = mu·((A·a_y + Bc·a_x) + gs·(t̂_y·n̂_x + t̂_x·n̂_y))
 *        dyy = mu·(Bc·a_y + gs·(t̂_y·n̂_y))
 *        H_w[u][0] = (float)(u_scale·(2·dxx))   H_w[u][1] = (float)(u_scale·dxy)
 *        H_w[v][0] = (float)(v_scale·dxy)       H_w[v][1] = (float)(v_scale·(2·dyy))
 *        cp_w = (float)(p_scale·((double)gwall[w][0] − ((gF[b][FPX]·a_x + gF[b][FPY]·a_y) + gF[b][MP]·(r_x·a_y − r_y·a_x))))
 *      With mu == 0 the four H are +0 and unit is not read.
 *   2. per node j, ONE thread, fp32.  own(j) = own_item[own_off[j] .. own_off[j + 1]): the items w with item[w] == j, ascending w (a
 *      node may be an item of several bodies).  in(j) = in_off[j] .. in_off[j + 1]: the pairs (w, e) with e an in-edge of item[w] and
 *      src_e == j, by ASCENDING CSR position e, then ascending w — the order in which g4c_mesh_derived_adjoint walks j's out-edges —
 *      with in_item[q] = w and in_g[q] = g[e] copied into that order, so the walk streams them and only the row of hw is a gather.
 *        p = +0; over own(j): p += cp_w.
 *        mu != 0: acc[f] = +0 for f = u, v; over in(j) ascending, for a = 0, 1: acc[f] += in_g[q][a] · H_w[f][a]; then for every w of
 *        own(j), over j's own in-edges e = off[j] .. in CSR order, for a = 0, 1: acc[f] −= g[e][a] · H_w[f][a].
 *        gx[j, pcol] = p, gx[j, ucol] = acc[u], gx[j, vcol] = acc[v]; EVERY other column of the row is +0 (sign bit clear), and with
 *        mu == 0 so are the velocity columns: g, off and the in-tables are then not read and may be NULL.
 *      When every node is an item at most once, gx[:, (ucol, vcol)] has the bits of g4c_mesh_derived_adjoint applied to a dense
 *      [n_nodes, 4] gradient that holds H_w at the wall rows and +0 elsewhere (its extra terms are g · (+0)).
 * Both launches: at most 1024 workgroups of 256, the items / nodes dealt gid, gid + grid, ..., four list entries per trip with their
 * loads in flight together and the additions in order; plain loads and stores, no LDS, no atomics, nothing passes between threads: the
 * bits are a function of the data alone and a numpy loop reproduces them.  The tables are trusted as g4c_body_forces trusts item:
 * item_body in [0, n_bodies), own_item and in_item in [0, n_items), the offset arrays ascending from 0 to n_items / n_entries.
 * n_nodes == 0 launches nothing; n_items == 0, n_bodies == 0 or gF == gwall == NULL zero-fills gx (nothing else is read).
 * G4C_EINVAL before any launch: null pointers, negative sizes (or n_entries > 2^31 − 1), nf < 1, a column >= nf, pcol / ucol / vcol
 * not distinct when mu != 0, mu != 0 without g, off or the in-tables, gx overlapping gF, gwall or hw (by their sizes). */
typedef struct g4c_body_forces_adjoint {
    const double *gF;            /* [n_bodies, G4C_FORCES_NSUM] or NULL */
    const float *gwall;          /* [n_items, 2] or NULL */
    int32_t nf, pcol, ucol, vcol;          /* ucol, vcol are not read when mu == 0 */
    double mu, p_scale, u_scale, v_scale;
    const float *g;              /* [E, 2], CSR order; may be NULL, with off and the in-tables, when mu == 0 */
    const int32_t *off;          /* [n_nodes + 1] */
    const int32_t *item_body;    /* [n_items] the body of every item */
    const double *area;          /* [n_items, 2] */
    const double *unit;          /* [n_items, 2] */
    const double *arm;           /* [n_items, 2] */
    const int32_t *own_off;      /* [n_nodes + 1] */
    const int32_t *own_item;     /* [n_items] */
    const int32_t *in_off;       /* [n_nodes + 1] */
    const int32_t *in_item;      /* [n_entries] */
    const float *in_g;           /* [n_entries, 2] */
    float *hw;                   /* [n_items, 5] scratch, written by the first launch */
    float *gx;                   /* [n_nodes, nf] */
} g4c_body_forces_adjoint_t;
int g4c_body_forces_adjoint(const g4c_body_forces_adjoint_t *a /*host*/, int64_t n_nodes, int64_t n_bodies, int64_t n_items,
                            int64_t n_entries, void *stream);

/* Values at points that are no mesh nodes (csrc/point_sample.hip): a moving-least-squares interpolation with a linear basis over the
 * k nearest nodes of every point, 1 <= k <= G4C_SAMPLE_MAX_K (above: G4C_EUNSUPPORTED).  The tables idx and coef are j-major, [k, P]:
 * neighbour j of point p at [j * n_points + p], nearest first, node rows of `x` / `pos`.
 *
 * g4c_sample_weights — once per set of points, one thread per point, fp64.  pos[n_nodes, dim] and queries[n_points, dim] are fp32.
 * For point q and j = 0 .. k − 1, every sum over j ascending: d_j = (double)pos[idx_j] − (double)q, r2_j = Σ_a d_j,a².
 *   exact hit   r2_0 == 0: c = (1, 0, .., 0), not degenerate;
 *   linear fit  w_j = 1, r2_j^(−1/2) or 1 / r2_j (power 0, 1, 2), W = Σ w_j, d̄ = Σ w_j d_j / W, e_j = d_j − d̄, M = Σ w_j e_j e_jᵀ,
 *               M⁻¹ = adj M / det M in closed form, c_j = w_j (1 / W − e_jᵀ M⁻¹ d̄): Σ c_j = 1 and Σ c_j d_j = 0, so constants and
 *               linear fields are reproduced (the centred form: when one weight dominates, d̄ → 0 and the correction vanishes);
 *   degenerate  k <= dim, or not det M > 1e-12 (tr M / dim)^dim (the gradient's rule): Shepard's c_j = w_j / W, exact on constants.
 * Outputs: coef[k, P] (each rounded to fp32 once), distance[P] = (float)sqrt(r2_0), degenerate[P].  n_points == 0 launches nothing
 * and succeeds; n_points > 0 with n_nodes < k is G4C_EINVAL; dim 2 or 3 (G4C_EUNSUPPORTED). */
#define G4C_SAMPLE_MAX_K 16
int g4c_sample_weights(const float *pos, const float *queries, const int32_t *idx, int32_t dim, int32_t power, int32_t k,
                       int64_t n_nodes, int64_t n_points, float *coef, float *distance, uint8_t *degenerate, void *stream);

/* The same fit over wrapped offsets (the periodic searches above have the metric): origin and period are host arrays of 3, period[a]
 * == 0 an axis that is not periodic.  The point is wrapped into the period first (the fp32 wrap sequence), then d_j = (double)pos[idx_j]
 * − (double)q' with the offset rule applied per periodic axis; everything after d_j is g4c_sample_weights', statement for statement.
 * distance is the wrapped distance to the nearest node.  With every period 0 the outputs are g4c_sample_weights' bits. */
int g4c_sample_weights_periodic(const float *pos, const float *queries, const int32_t *idx, int32_t dim, int32_t power, int32_t k,
                                int64_t n_nodes, int64_t n_points, const float *origin, const float *period, float *coef,
                                float *distance, uint8_t *degenerate, void *stream);

/* g4c_sample_points — cur[p, f] = Σ_j coef[j, p] · x[idx[j, p], f] for f < nf, fp32, j ascending, every product rounded before it is
 * added (the first product starts the sum): one thread per (point, chunk of 4 columns), so the bits are a function of the data alone
 * and a numpy.float32 loop reproduces them.  The same launch serves nf = 3 inside a step (AFTER the forward, BEFORE the step's closing
 * launch: it reads the step index t = step[0] and never writes it) and nf = all the columns of a target, once.  At most 1024
 * workgroups of 256, the items dealt gid, gid + grid, ...  cur[n_points, nf] is written on every call.  If series != NULL, every > 0,
 * 0 <= t < max_steps, (t + 1) % every == 0 and slot = (t + 1) / every − 1 < n_slots, the same values go to series[slot][n_points][nf]
 * (the records' slot convention); any other step writes cur only.  Every idx must be a row of x (0 <= idx < n_nodes: not checked on
 * the device).  G4C_EINVAL before any launch: negative sizes, x_ld < nf, k < 1, a series without a step index or with every == 0,
 * n_points > 0 with n_nodes < k.  n_points == 0 launches nothing and succeeds.  No atomics. */
typedef struct g4c_sample_points {
    const int32_t *idx;          /* [k, n_points] */
    const float *coef;           /* [k, n_points] */
    int32_t k, nf, x_ld;         /* x[n_nodes, x_ld] fp32, its first nf columns are sampled */
    float *cur;                  /* [n_points, nf] */
    const int32_t *step;         /* device; may be NULL without series */
    int32_t every, n_slots, max_steps;
    float *series;               /* [n_slots][n_points][nf] or NULL */
} g4c_sample_points_t;
int g4c_sample_points(const float *x, const g4c_sample_points_t *s /*host*/, int64_t n_nodes, int64_t n_points, void *stream);

/* g4c_sample_points_adjoint — the transpose of g4c_sample_points' map x -> cur (the map is linear with constant coefficients: its
 * backward).  Forward: y[p, f] = Σ_j coef[j, p] · x[idx[j, p], f].  Adjoint of gy[n_points, nf] (dense):
 *   gx[i, f] = Σ_{q in list(i)} in_coef[q] · gy[in_pt[q], f],   list(i) = in_off[i] .. in_off[i + 1] − 1
 * A scatter from the points to the nodes, taken as a gather through a node-side table built once per set of points: list(i) holds the
 * entries of the j-major [k, P] tables whose idx is i, in ASCENDING flat position j · P + p (slot first, then point — a stable grouping
 * of the flattened idx); in_off[n_nodes + 1] its offsets, in_pt[k · P] = position mod P the point of each entry and in_coef[k · P] its
 * coefficient, both copied into that order, so a walk streams them and only the point's row of gy is a gather.
 * fp32, no contraction, in this order: acc[f] = +0; for q ascending over list(i): acc[f] = acc[f] + (in_coef[q] · gy[in_pt[q], f]),
 * the product rounded before it is added.  One thread per (node, chunk of 4 columns), at most 1024 workgroups of 256, the items dealt
 * gid, gid + grid, ...; plain loads and stores, no atomics, nothing passes between threads: the bits are a function of the data alone
 * and a numpy.float32 loop reproduces them.  A node's list is walked by one thread whatever its length.
 * EVERY element of gx[n_nodes, nf] (dense) is written: a node that no point uses gets +0 (sign bit clear).  n_points == 0 still
 * zero-fills gx (gy and the tables may then be NULL); n_nodes == 0 launches nothing.  The tables are trusted as g4c_sample_points trusts
 * idx: in_pt in [0, n_points), in_off ascending from 0 to at most 2^31 − 1 entries.
 * G4C_EINVAL before any launch: negative sizes, nf < 1, a null pointer, gx overlapping gy (by their sizes). */
int g4c_sample_points_adjoint(const float *gy, const int32_t *in_off, const int32_t *in_pt, const float *in_coef, int32_t nf,
                              int64_t n_nodes, int64_t n_points, float *gx, void *stream);

/* Lagrangian tracers (csrc/tracer.hip): massless particles carried by a velocity that lives at the nodes.  g4c_tracer_advance moves
 * every particle one step in one launch — one thread per particle, at most 1024 workgroups of 256, the particles dealt gid, gid + grid,
 * ..., plain loads and stores, no atomics — and may sit inside a captured step: AFTER the forward, BEFORE the step's closing launch
 * (it reads the field window and the step index t = step[0], and never writes the index).  With step == NULL, t = t_host.
 *
 * The cloud's cell grid (pos_sorted, order, cell_start, n_cells, origin, cell_size) is the one g4c_knn_grid_query takes, built once
 * per mesh by the caller.  For particle p, with t read once:
 *   1. t < 0, t >= max_steps or t < release[p]: nothing of p changes (status 0, waiting).  status[p] >= 2: frozen, nothing changes.
 *      Otherwise status[p] = 1 (moving) and
 *   2. a coordinate of q[p] that is not finite: status 4, stopped[p] = t, no search (the test comes before any cell arithmetic, and a
 *      cell coordinate is clamped as a double before it becomes an integer);
 *   3. a stage at position r on the node tensor x: the cell floor(((double)r − (double)origin) / (double)cell_size) clamped per axis;
 *      the k nearest nodes by g4c_knn_grid_query's ring search (same scan order, strict <, same termination), rows through `order`;
 *      g4c_sample_weights' coefficients c_j over them (fp64, exact-hit and degenerate rules, one rounding to fp32); u_a = Σ_j c_j
 *      x[idx_j ld + vcol_a] as g4c_sample_points sums (fp32, j ascending, each product rounded, the first starts the sum); the
 *      physical velocity v_a = scale_a u_a + shift_a, the product rounded, then added;
 *   4. the first stage's distance to the nearest node, (float)sqrt(r2_0), above max_distance: status 3, stopped[p] = t, q unchanged,
 *      vel[p] not written;
 *   5. Euler: q'_a = q_a + dt v0_a, v0 from the stage at q on x0.  Heun: q*_a = q_a + dt v0_a, v1 from the stage at q* on x1,
 *      q'_a = q_a + (0.5f dt)(v0_a + v1_a); a q* that is not finite: status 4 as in 2, q unchanged.  All fp32, every product rounded
 *      before its add.  vel[p] (if given) = v0;
 *   6. q' is stored; outside [box_lo, box_hi] (a NaN is outside; the corners may be infinite): status 2, stopped[p] = t — the particle
 *      stays where it left.
 *   7. If series != NULL, every > 0, 0 <= t < max_steps, (t + 1) % every == 0 and slot = (t + 1) / every − 1 < n_slots (the records'
 *      slot convention), the current q of EVERY particle — waiting, moving or frozen — goes to series[slot][n_particles][dim].
 * G4C_EINVAL before any launch: negative sizes, k < 1, power, scheme, a vcol outside its tensor's row, a bad grid, a series with
 * every == 0, n_particles > 0 with n_nodes < k or a null pointer (x1 may be NULL for Euler; step, series and vel may be NULL).
 * n_particles == 0 launches nothing and succeeds.  dim 2 or 3, k <= G4C_SAMPLE_MAX_K (G4C_EUNSUPPORTED). */
#define G4C_TRACER_EULER 0
#define G4C_TRACER_HEUN 1
#define G4C_TRACER_WAITING 0
#define G4C_TRACER_MOVING 1
#define G4C_TRACER_LEFT 2        /* left the box */
#define G4C_TRACER_FAR 3         /* farther than max_distance from every node */
#define G4C_TRACER_NONFINITE 4   /* a position that is not finite */
typedef struct g4c_tracer {
    const float *pos_sorted;     /* [n_nodes, dim] the cloud in cell-sorted order */
    const int32_t *order;        /* [n_nodes] node row of each sorted point */
    const int32_t *cell_start;   /* [n_cells + 1] first sorted point of each cell */
    int32_t n_cells[3];
    float origin[3], cell_size;
    int32_t dim, k, power;
    const float *x0;             /* [n_nodes, x0_ld] time level t */
    const float *x1;             /* [n_nodes, x1_ld] time level t + 1; may be NULL for Euler */
    int32_t x0_ld, x1_ld;
    int32_t vcol[3];             /* the velocity's columns, in x0 and in x1 */
    float scale[3], shift[3], dt;
    int32_t scheme;              /* G4C_TRACER_EULER / G4C_TRACER_HEUN */
    float box_lo[3], box_hi[3], max_distance;
    const int32_t *step;         /* device; NULL: t = t_host */
    int32_t t_host, max_steps, every, n_slots;
    float *series;               /* [n_slots][n_particles][dim] or NULL */
    float *q;                    /* [n_particles, dim], updated in place */
    uint8_t *status;             /* [n_particles] G4C_TRACER_WAITING .. */
    int32_t *stopped;            /* [n_particles] the step at which status became >= 2 */
    const int32_t *release;      /* [n_particles] the first step at which the particle moves */
    float *vel;                  /* [n_particles, dim] the first stage's physical velocity, or NULL */
} g4c_tracer_t;
int g4c_tracer_advance(const g4c_tracer_t *tr /*host*/, int64_t n_nodes, int64_t n_particles, void *stream);

/* The same step in a domain that is periodic along some axes: g4c_tracer_t as it is, and after it the periods and the per-axis cell
 * sizes of the periodic grid (g4c_periodic_grid_t: base.n_cells and base.origin are that grid's, base.cell_size is not read).
 * Differences from the seven points above:
 *   3. a stage first wraps a COPY of its position r (the wrap sequence above, per periodic axis), forms its cell from the wrapped
 *      copy, searches by g4c_knn_grid_query_periodic's ring search and fits g4c_sample_weights_periodic's coefficients;
 *   5. the updates add to the STORED position q (itself wrapped by the step before: a first position is taken as given);
 *   6. q' is wrapped (the same sequence) BEFORE it is stored, tested against the box and written to the series: a particle that
 *      crosses a periodic face stays moving, and the series holds wrapped positions — a jump of more than L / 2 between two slots
 *      is a crossing.
 *   2'. A position "does not wrap" when the wrap sequence reaches no finite number by itself (above).  It is treated as a position
 *      that is not finite, wherever a position is tested: q[p] before the first stage, Heun's q* before the second, and q' before it
 *      is stored — status 4, stopped[p] = t, q unchanged.  No stage ever starts from the origin standing in for such a position.
 * Everything else, the errors included, is g4c_tracer_advance's; a period must be finite and >= 0, a cell size finite and > 0. */
typedef struct g4c_tracer_periodic {
    g4c_tracer_t base;
    float period[3];             /* L per axis; 0: the axis is not periodic */
    double cell[3];              /* the cell size per axis */
} g4c_tracer_periodic_t;
int g4c_tracer_advance_periodic(const g4c_tracer_periodic_t *tr /*host*/, int64_t n_nodes, int64_t n_particles, void *stream);

/* g4c_snapshot_mean / _gram / _combine (csrc/snapshot_modes.hip) — the three launches of POD and DMD by the method of snapshots that
 * touch L-sized data (graphs4cfd_amd/modes.py holds the M-sized algebra; the reference has no counterpart).  They run AFTER a
 * rollout, outside the step.  A snapshot matrix is float32 [rows, L], rows contiguous with leading dimension L — a rollout's
 * step-major buffer [slots, N, nf] with L = N nf — and a selection names the rows first, first + stride, ... (count of them).  All sums
 * are fp64 in an order that is a function of the shapes alone; no floating-point atomics.
 *   mean[l]  = (sum_i (double)x[first + i stride][l]) / count, i in slot order: bit for bit the plain fp64 loop.
 *   G[i][j]  = sum_l w[l] ((double)a_i[l] - mean_a[l]) ((double)b_j[l] - mean_b[l]); mean_* NULL: no centring; w NULL: ones.  The product
 *              of two fp32 values is exact in fp64, so the uncentred unweighted form is a sum of exact terms.  A workgroup owns a block
 *              of G4C_SNAPSHOT_GRAM_BLOCK^2 entries and a chunk of G4C_SNAPSHOT_GRAM_CHUNK columns, stages (a - mean_a) w and b - mean_b
 *              through LDS as fp64 and accumulates with v_mfma_f64_16x16x4_f64 (four columns a step, in the pipe's own order); a second
 *              launch adds the chunks' partial blocks in chunk order.  When a == b, mean_a == mean_b and the selections are equal only
 *              the blocks on and below the diagonal are computed, and that launch writes each entry below the diagonal and its mirror
 *              image: G is symmetric bit for bit.  scratch: g4c_snapshot_gram_scratch_bytes(Ma, Mb, L, symmetric) bytes, all written
 *              (-1 for sizes outside the envelope).
 *   out[r][l] = (float) sum_i C[i][r] ((double)x_i[l] - mean[l]), i in slot order, product and sum rounded separately: bit for bit a
 *              plain fp64 loop rounded once to fp32.  C: float64 [count, R] with leading dimension ldc, read uniformly; a thread owns
 *              one column and G4C_SNAPSHOT_COMBINE_BLOCK values of r, so x is read once per block of r. */
#define G4C_SNAPSHOT_MAX_ROWS 1024              /* Ma, Mb, R: G4C_EUNSUPPORTED above */
#define G4C_SNAPSHOT_MAX_COLUMNS 2147483647LL   /* L: 32-bit indices within one snapshot */
#define G4C_SNAPSHOT_GRAM_BLOCK 64
#define G4C_SNAPSHOT_GRAM_CHUNK 2048
#define G4C_SNAPSHOT_COMBINE_BLOCK 8
typedef struct g4c_snapshot_sel {
    int32_t rows;                /* snapshots in the buffer */
    int32_t first, stride, count; /* the rows first + i stride, i < count, all < rows */
} g4c_snapshot_sel_t;
int g4c_snapshot_mean(const float *x, const g4c_snapshot_sel_t *sel /*host*/, int64_t L, double *mean_out /*[L]*/, void *stream);
int64_t g4c_snapshot_gram_scratch_bytes(int32_t Ma, int32_t Mb, int64_t L, int32_t symmetric);
int g4c_snapshot_gram(const float *a, const double *mean_a, const g4c_snapshot_sel_t *sel_a /*host*/, const float *b, const double *mean_b,
                      const g4c_snapshot_sel_t *sel_b /*host*/, const double *w, int64_t L, double *G_out /*[Ma, Mb]*/, int64_t ld,
                      void *scratch, void *stream);
int g4c_snapshot_combine(const float *x, const double *mean, const g4c_snapshot_sel_t *sel /*host*/, const double *C, int64_t ldc, int32_t R,
                         int64_t L, float *out /*[R, L]*/, void *stream);

/* Node control volumes (csrc/control_volumes.hip) — the areas that turn the node sums of the diagnostics into integrals over a 2-D
 * domain, and the sums weighted by them.  The reference has no counterpart: a kNN cloud has no cells.
 *
 * g4c_voronoi_cells, once per mesh.  Node i gets the polygon  (its Voronoi cell within the cloud) ∩ (the box [box_lo, box_hi]) ∩
 * (optionally the half-plane {x : (x − pos_i)·n_i >= 0} through the node itself, n_i = normals[i] != (0, 0): a wall node, whose cell
 * would otherwise reach into the body).  One thread per node, fp64 without contraction on the fp32 positions (g4c_mesh_jet_weights'
 * conventions), the polygon — at most G4C_VORONOI_MAX_VERTS vertices, relative to the node, counter-clockwise — in the thread's own
 * LDS column.  The cloud's cell grid (pos_sorted, order, cell_start, n_cells, origin, cell_size) is the one g4c_knn_grid takes.
 *   1. The polygon starts as the box: (lo_x, lo_y), (hi_x, lo_y), (hi_x, hi_y), (lo_x, hi_y), each minus the node.
 *   2. A clip keeps {v : s(v) = c − (v_x a + v_y b) >= 0}: Sutherland-Hodgman, vertex by vertex from vertex 0; a vertex with s >= 0 is
 *      kept (exactly on the line: kept), and an edge whose ends have s of strictly opposite signs adds its crossing
 *      v + (s / (s − s')) (v' − v), v the edge's first vertex.  A polygon with no vertex of s < 0 is left as it is.
 *   3. The wall half-plane first: (a, b, c) = (−n_x, −n_y, 0).
 *   4. The node's cell is floor(((double)pos − (double)origin) / (double)cell_size) clamped per axis.  Ring rho = 0, 1, ... of the grid
 *      about it (the cells at Chebyshev distance rho that lie in the grid) is walked row by row, y ascending: a first or last row is
 *      one run of sorted points from its first cell to its last, any other row its left cell, then its right one; every point j but
 *      the node itself clips by the bisector: r = pos_j − pos_i, (a, b, c) = (r_x, r_y, ½ |r|²).  A point at zero distance cuts
 *      nothing and sets DUPLICATE (in both nodes of the pair).
 *   5. Before ring rho >= 1: R² = the largest |v|² of the polygon's vertices, lb = the least distance from the node to a face of the
 *      block of rings < rho that has cells behind it, less 1e-5 cell_size.  The walk stops if lb > 0 and lb² > 4 R² (no unseen point
 *      can cut the polygon), or when no ring is left in the grid.  rings[i] = the rings walked: what to look at when a box far
 *      larger than the cloud makes the hull nodes scan the grid.
 *   6. A clip that would give more than G4C_VORONOI_MAX_VERTS vertices stops the node: flag OVERFLOW, area +0, nvert 0.  A polygon
 *      left with fewer than 3 vertices is empty: area +0, nvert 0.
 *   7. area = ½ Σ_j (x_j y_j+1 − x_j+1 y_j) about the node in vertex order, centroid = pos_i + Σ_j (v_j + v_j+1) cross_j / (3 Σ cross);
 *      a sum that is not > 0 gives area +0, and every row of area +0 has the node as its centroid.  BOX: an edge of the final polygon
 *      lies on the box; WALL: the node has a normal.
 * Outputs are in the caller's node order (row order[s] for sorted point s); every row is written.  The grid is trusted as
 * g4c_knn_grid trusts it.  G4C_EINVAL before any launch: a bad grid, an empty or non-finite box, n_nodes outside [0, 2^31), a null
 * pointer (normals may be NULL).  n_nodes == 0 launches nothing. */
#define G4C_VORONOI_MAX_VERTS 32
#define G4C_VORONOI_BOX 1
#define G4C_VORONOI_WALL 2
#define G4C_VORONOI_DUPLICATE 4
#define G4C_VORONOI_OVERFLOW 8
typedef struct g4c_voronoi_cells {
    const float *pos_sorted;     /* [n_nodes, 2] the cloud in cell-sorted order */
    const int32_t *order;        /* [n_nodes] node row of each sorted point */
    const int32_t *cell_start;   /* [n_cells[0] n_cells[1] + 1] first sorted point of each cell */
    int32_t n_cells[3];          /* (the third is not read) */
    float origin[3], cell_size;
    double box_lo[2], box_hi[2];
    const double *normals;       /* [n_nodes, 2] by node row, (0, 0): none; or NULL */
    double *area;                /* [n_nodes] */
    double *centroid;            /* [n_nodes, 2] */
    int32_t *nvert;              /* [n_nodes] */
    uint8_t *flags;              /* [n_nodes] G4C_VORONOI_* */
    int32_t *rings;              /* [n_nodes] */
} g4c_voronoi_cells_t;
int g4c_voronoi_cells(const g4c_voronoi_cells_t *vc /*host*/, int64_t n_nodes, void *stream);

/* g4c_weighted_integrals, once per step and source: stats[t][e] = Σ_i w_i z_i[a_e] z_i[b_e] for the ne <= G4C_INTEGRALS_MAX_ENTRIES
 * entries (a_e, b_e) of the program; a column of −1 stands for 1.  The sample is z_i[c] = (double)x[i x_ld + x_step t + c] — x_step == 0:
 * a prediction or the derived columns `cur`; x_step = nf: a target holding every step, read by the same code — or, with sub, that
 * minus (double)sub[i sub_ld + sub_step t + c], the difference formed in fp64, where it is exact.  The product z[a] z[b] is rounded to
 * fp64 once, then multiplied by w_i and rounded once, then added.  A row with w_i == 0 contributes nothing whatever it holds.
 * Two launches in a fixed order, no atomics: at most 1024 workgroups of 256 — a function of n_nodes alone —, thread tid of workgroup b
 * adds the rows 256 b + tid, + 256 · workgroups, ... from +0 in that order, a xor butterfly 32, 16, .., 1 per wave of 64, the four waves
 * added in order; then one workgroup whose thread i adds the partials of workgroups i, i + 256, ... and reduces the same way.  scratch:
 * g4c_weighted_integrals_scratch_doubles(n_nodes, ne) doubles.  t = step[0] read on the device and never written (step NULL: t_host);
 * stats[t] is OVERWRITTEN iff 0 <= t < max_steps, any other step writes no statistic: capturable, and bit-identical between captured
 * and eager steps.  G4C_EINVAL before any launch: bad sizes, an entry outside [−1, nz), a leading dimension below what the columns and
 * steps need, a null pointer; G4C_EUNSUPPORTED: ne > G4C_INTEGRALS_MAX_ENTRIES. */
#define G4C_INTEGRALS_MAX_ENTRIES 8
typedef struct g4c_integral_program {
    int32_t ne;
    int32_t a[G4C_INTEGRALS_MAX_ENTRIES], b[G4C_INTEGRALS_MAX_ENTRIES];
} g4c_integral_program_t;
typedef struct g4c_weighted_integrals {
    const float *x;              /* [n_nodes, x_ld] */
    int32_t x_ld, x_step;        /* x_step 0, or >= nz with x_ld >= x_step max_steps */
    const float *sub;            /* [n_nodes, sub_ld] or NULL */
    int32_t sub_ld, sub_step;
    int32_t nz;                  /* columns of a sample */
    const double *w;             /* [n_nodes] */
    const int32_t *step;         /* device; NULL: t = t_host */
    int32_t t_host, max_steps;
    double *stats;               /* [max_steps][ne] */
    double *scratch;
} g4c_weighted_integrals_t;
int64_t g4c_weighted_integrals_scratch_doubles(int64_t n_nodes, int32_t ne);
int g4c_weighted_integrals(const g4c_weighted_integrals_t *wi /*host*/, const g4c_integral_program_t *prog /*host*/, int64_t n_nodes,
                           void *stream);

/* g4c_weighted_integrals_adjoint: the transpose of the map x -> I[q][e] = Σ_{i in group q} w_i z_i[a_e] z_i[b_e] (the forward above,
 * once per group of rows), applied to the upstream gradient g fp64 [n_groups, ne] — read on the device, never on the host —: gx float32
 * [n_nodes, gx_ld >= nz], columns 0 .. nz − 1 of every row written and nothing else.  The samples z are the forward's (x, or x − sub in
 * fp64, at the step t_host: the step is host-given only, training is not captured).  Node i, group q = group ? group[i] : 0, for every
 * column c in 0 .. nz − 1:
 *     acc = +0.0                                   (fp64)
 *     for e = 0 .. ne − 1, in order:
 *         gw = g[q][e] · w_i                       (rounded)
 *         if a_e == c: acc += gw · z_i[b_e]        (the product rounded, then added; z of column −1 is 1.0)
 *         if b_e == c: acc += gw · z_i[a_e]        (both hits when a_e == b_e == c: two adds, in this order)
 *     gx[i][c] = (float) acc                       (round to nearest even, IEEE on overflow)
 * No contraction; an entry that does not name column c is skipped, not multiplied by zero, so a NaN in g[q][e] or in a column of x
 * changes only the outputs that depend on it.  A row with w_i == 0, or with group[i] outside [0, n_groups), is +0 in every column and
 * reads neither x nor g (no address is formed from an unchecked index).  One thread per (node, column), no atomics: the bits are a
 * function of the data alone.  n_nodes == 0: G4C_OK without a launch.  G4C_EINVAL before any launch: bad sizes, an entry outside
 * [−1, nz), t_host outside [0, max_steps), a leading dimension below what the columns and steps need (the forward's rules; gx_ld < nz),
 * a null pointer; G4C_EUNSUPPORTED: ne > G4C_INTEGRALS_MAX_ENTRIES. */
typedef struct g4c_weighted_integrals_adjoint {
    const float *x;              /* [n_nodes, x_ld] */
    int32_t x_ld, x_step;        /* x_step 0, or >= nz with x_ld >= x_step max_steps */
    const float *sub;            /* [n_nodes, sub_ld] or NULL */
    int32_t sub_ld, sub_step;
    int32_t nz;                  /* columns of a sample */
    const double *w;             /* [n_nodes] */
    const double *g;             /* [n_groups][ne], device */
    int32_t n_groups;
    const int32_t *group;        /* [n_nodes] the group of each row, or NULL: all rows in group 0 */
    int32_t t_host, max_steps;
    float *gx;                   /* [n_nodes, gx_ld] */
    int32_t gx_ld;
} g4c_weighted_integrals_adjoint_t;
int g4c_weighted_integrals_adjoint(const g4c_weighted_integrals_adjoint_t *wa /*host*/, const g4c_integral_program_t *prog /*host*/,
                                   int64_t n_nodes, void *stream);

/* out[r, c] = a[r, a_col0 + c] + b[r, c]: the residual time step `field[:, -nf:] + output`
 * (nn/remus_gnn.py:199; the MuS-GNN decoder fuses it into g4c_mlp_run's epilogue instead). */
int g4c_add_cols(const float *a, int32_t a_ld, int32_t a_col0, const float *b, int32_t b_ld,
                 float *out, int32_t out_ld, int32_t width, int64_t n_rows, void *stream);

/* x[i] = act(x[i]) in place, n contiguous floats (F.selu / torch.tanh on a block output; NaN: see G4C_ACT_*). */
int g4c_activation_inplace(float *x, int64_t n, int32_t act, void *stream);

/* dst[r, dcol0 : dcol0+width] = src[r, scol0 : scol0+width]  (torch.cat of the narrow node inputs,
 * nn/mus_gnn.py:71; also used to assemble halo send buffers when idx != NULL: reads src[idx[r]]). */
int g4c_copy_cols(const float *src, int32_t src_ld, int32_t scol0, const int32_t *idx,
                  float *dst, int32_t dst_ld, int32_t dcol0, int32_t width, int64_t n_rows, void *stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Training path: the backward pass of the fused blocks.  The reference differentiates
 * cat / index / nn.Linear / SELU / LayerNorm / scatter with torch autograd (GNN.fit, nn/model.py:152-301); here the forward
 * is the fused launch above, the backward recomputes the block's activations (nothing but the block's inputs and output is
 * kept between the passes) with rocBLAS for the plain GEMMs and these kernels for everything else.  All reductions run
 * in a fixed order: gradients are bit-reproducible.
 * ------------------------------------------------------------------------------------------------------------------ */

/* dst[r, dcol0 : dcol0+width] (+)= (negate ? -1 : 1) * pre_act(src[idx ? idx[r] : r, scol0 : scol0+width]): one column block
 * of the concatenated MLP input (nn/blocks.py:181,185,229,285), recomputed for the backward pass; `accumulate` != 0 adds
 * into dst (the recomputed first layer: pre-multiplied node-side terms gathered through their index). */
int g4c_train_gather(const float *src, int32_t src_ld, int32_t scol0, const int32_t *idx, int32_t pre_act, int32_t negate,
                     float *dst, int32_t dst_ld, int32_t dcol0, int32_t width, int64_t n_rows, int32_t accumulate, void *stream);

/* dz = dy * act'(.)  — `ref` holds the activation's OUTPUT (from_input = 0) or its INPUT (from_input = 1).  dz may alias dy. */
int g4c_act_grad(const float *dy, int32_t dy_ld, const float *ref, int32_t ref_ld, int32_t from_input, int32_t act,
                 float *dz, int32_t dz_ld, int32_t width, int64_t n_rows, void *stream);

/* g4c_act_grad with `ref` stored as bf16 rows (ref_ld in elements): each value is widened exactly to fp32, everything after the load
 * is g4c_act_grad — the result is bit for bit g4c_act_grad's on the widened rows.  Four columns per thread when width % 4 == 0, dy / dz
 * are 16-byte aligned with leading dimensions that are multiples of 4 and ref is 8-byte aligned with ref_ld % 4 == 0; else one. */
int g4c_act_grad_ref16(const float *dy, int32_t dy_ld, const void *ref, int32_t ref_ld, int32_t from_input, int32_t act,
                       float *dz, int32_t dz_ld, int32_t width, int64_t n_rows, void *stream);

/* LayerNorm backward (nn/blocks.py:141, eps 1e-5, affine): dz from the pre-norm rows z, gamma and dy; `partial` receives
 * g4c_layernorm_grad_partials(n_rows) rows of [dgamma(width) | dbeta(width)] partial sums — add them with g4c_colsum. */
int32_t g4c_layernorm_grad_partials(int64_t n_rows);
int g4c_layernorm_grad(const float *z, int32_t z_ld, const float *gamma, const float *dy, int32_t dy_ld, float *dz,
                       int32_t dz_ld, float *partial, int32_t width, int64_t n_rows, float eps, void *stream);

/* g4c_layernorm_grad with the pre-norm rows z stored as bf16 (z_ld in elements), widened exactly at the load: bit for bit
 * g4c_layernorm_grad on the widened rows, the same partials. */
int g4c_layernorm_grad_z16(const void *z, int32_t z_ld, const float *gamma, const float *dy, int32_t dy_ld, float *dz,
                           int32_t dz_ld, float *partial, int32_t width, int64_t n_rows, float eps, void *stream);

/* out[c] = sum_r x[r, c] (bias gradients; the LayerNorm partials).  `scratch`: g4c_colsum_partials(n_rows) * width floats. */
int32_t g4c_colsum_partials(int64_t n_rows);
int g4c_colsum(const float *x, int32_t ld, int32_t width, int64_t n_rows, float *scratch, float *out, void *stream);

/* Weight / bias gradient of one nn.Linear with 128 inputs and 128 outputs (every hidden layer of every published arch):
 * out[0 : 128*128] = dW[n, k] = sum_r g[r, n] a[r, k] (row-major [128, 128]), and, if with_bias, out[128*128 : +128] =
 * db[n] = sum_r g[r, n].  g = dL/d(layer output) [n_rows, 128], a = the layer's input rows [n_rows, 128] (a 128-column window
 * of a wider tensor is fine: a_ld).  One pass over g and a (HBM-bound), fp32 MFMA, partial tiles per workgroup added in a
 * fixed order.  `scratch`: g4c_weight_grad_scratch_floats(n_rows) floats; `out`: 128*128 + 128 floats. */
int32_t g4c_weight_grad_partials(int64_t n_rows);
int64_t g4c_weight_grad_scratch_floats(int64_t n_rows);
int g4c_weight_grad(const float *g, int32_t g_ld, const float *a, int32_t a_ld, int64_t n_rows, float *scratch, float *out,
                    int32_t with_bias, void *stream);

/* The same call for mixed-precision training: dW[n, k] = sum_r bf16(g[r, n]) * bf16(a[r, k]) — both operands rounded once to
 * bf16 (round to nearest even) as they are staged, products on the bf16 MFMA, fp32 accumulation; db[n] = sum_r g[r, n] from the
 * UNROUNDED fp32 rows.  Same operands, same scratch (g4c_weight_grad_scratch_floats), same partial-tile rule and fixed-order
 * reduction: bit-reproducible, no atomics.  Arguments are validated before any HIP call: g / a not 16-byte aligned, a leading
 * dimension below 128 or not a multiple of 4, or n_rows < 0 return G4C_EINVAL (g4c_last_error() says which). */
int g4c_weight_grad_bf16(const float *g, int32_t g_ld, const float *a, int32_t a_ld, int64_t n_rows, float *scratch, float *out,
                         int32_t with_bias, void *stream);

/* g4c_weight_grad_bf16 with operand `a` ALREADY stored as bf16 rows (rows a forward launch kept with save_dtype G4C_DTYPE_BF16;
 * a_ld in elements, a multiple of 4 and >= 128; a 16-byte aligned — a 128-column window of a wider bf16 tensor is fine): the rows
 * are staged without a conversion, g stays fp32 (rounded as it is staged, db from the unrounded rows).  Same slabs, LDS image, MFMA
 * sequence, partial-tile rule, scratch and reduction: the result is bit for bit g4c_weight_grad_bf16's on the widened rows, at
 * 768 instead of 1024 bytes per row.  The same validation before any HIP call. */
int g4c_weight_grad_bf16_a16(const float *g, int32_t g_ld, const void *a, int32_t a_ld, int64_t n_rows, float *scratch, float *out,
                             int32_t with_bias, void *stream);

/* Adjoint of g4c_segment_reduce: dsrc[perm ? perm[p] : p] = dout[s] (/ max(count_s, 1) if mean) for p in segment s.
 * Rows of dsrc that belong to no segment are left untouched (zero them first when perm is not a full permutation). */
int g4c_segment_broadcast(const float *dout, int32_t dout_ld, const int32_t *off, const int32_t *perm, int32_t n_seg,
                          int32_t width, int32_t mean, float *dsrc, int32_t dsrc_ld, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* G4C_H */
