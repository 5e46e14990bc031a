// g4c_mlp_run: the one launcher of the fused-MLP kernels.  Host code only — the kernels are in mlp_fused.hip (fp32 and tile kernels),
// mlp_bx6i.hip, mlp_ws.hip and mlp_rs.hip, each behind two functions (mlp_common.h): X_takes(Launch) = the envelope of its kernels,
// X_launch(Launch) = pick the instantiation, launch it, report what ran.
//
// A call passes through stages, each of which checks its part of g4c_mlp_t / g4c_src_t / g4c_mlp_io_t and fills its part of the
// Launch: call, sources, stream, outputs, save / mul, range, heads, node update.  Then `choose` picks the family and it launches.
//
// Order of precedence (the first row that applies; capability = X_takes, everything else is policy and lives in `choose`):
//
//   family            when                                                                     if its envelope does not hold
//   ws  (+ node)      io->upd: the fused MP layer                                              G4C_EUNSUPPORTED
//   ws  (pre)         every source additive: the first layer precomputed (g4c_mlp_t.k_pad)     G4C_EUNSUPPORTED
//   rs                w_format G4C_WFMT_BF16_RS (and no save)                                  G4C_EUNSUPPORTED
//   rs2               w_format G4C_WFMT_BF16_RS2 / _RS2N (and no save, no aggregation)         G4C_EUNSUPPORTED
//   ws                split-operand stream; g4c_mlp_ws_enable 2, or 1 and >= 20 000 rows       next row
//   bx6i              split-operand stream; g4c_mlp_bx6i_enable 2, or 1 and >= 400 000 rows    next row
//   tile              split-operand stream.  At most g4c_mlp_small_launch_tiles tiles: the     -
//                     deep weight ring; above, with g4c_mlp_shapes_enable: a compile-time
//                     shape where one matches, in the form g4c_mlp_tile_form names
//   split             G4C_WFMT_FP32                                                            -
//
// (A stream in the row-split k order can run on no other kernel: outside the envelope the call fails instead of computing something else.)
#include "mlp_common.h"
#include <atomic>
#include <climits>
using namespace g4cm;

// ---- policy knobs (g4c.h): process-wide, each returns its previous value, a negative argument only queries ----------------------------
namespace {

std::atomic<int> g_ws_mode{1};          // 0 off, 1 launches of at least WS_MIN_ROWS rows, 2 every launch the kernel takes (tests)
std::atomic<int> g_bx6i_mode{1};        // likewise, BX6I_MIN_ROWS
std::atomic<int> g_deep_tiles{512};     // launches of at most this many 32-row tiles run the tile kernel's deep-ring instantiation (Ring6)
// compile-time launch shapes of the tile kernel (mlp_common.h TileShape*): on by default (-DG4C_TILE_SHAPES_DEFAULT=0: a library for
// whole-benchmark A/B legs, scripts/ab_bench.sh)
#ifndef G4C_TILE_SHAPES_DEFAULT
#define G4C_TILE_SHAPES_DEFAULT 1
#endif
std::atomic<int> g_shapes{G4C_TILE_SHAPES_DEFAULT};
// the form a shaped chip-filling launch of the tile kernel runs in (mlp_fused.hip tile_go_rows64): 0 32-row tiles, 1 64-row tiles
// (-DG4C_TILE_FORM_DEFAULT=: A/B legs, as above).  64-row tiles run three workgroups per CU, so a launch takes them from
// TILE_ROWS64_FILL times the small-launch limit on (1 536 32-row tiles at the default 512 = 768 64-row tiles, three per CU of 256):
// below that they leave CUs short of workgroups (replayed headline step, the coarse levels' UpMP / DownMP launches at positions 16 and
// 25: 18.6 against 17.6 us and 32.7 against 31.8)
#ifndef G4C_TILE_FORM_DEFAULT
#define G4C_TILE_FORM_DEFAULT 1
#endif
std::atomic<int> g_tile_form{G4C_TILE_FORM_DEFAULT};

// mlp_ws_kernel against the two-way instantiation of mlp_bx6i_kernel, which it replaces, on the level-1 message launch: 322 us against
// 339 us with the fused aggregation, 288 against 292 without; same-box sweeps of round 3: ahead of the tile kernel from ~20 k rows
constexpr long long WS_MIN_ROWS = 20000;
// mlp_bx6i_kernel needs a full machine of its two workgroups per CU: same-box crossover against the tile kernel ~300 k rows
constexpr long long BX6I_MIN_ROWS = 400000;
constexpr long long TILE_ROWS64_FILL = 3;

int knob(std::atomic<int> &k, int value, int max_value) {
    const int prev = k.load(std::memory_order_relaxed);
    if (value >= 0) k.store(value > max_value ? max_value : value, std::memory_order_relaxed);
    return prev;
}

thread_local Ran g_last;

// ---- stage: the call itself — format, row range, the switches of io ------------------------------------------------------------------
int stage_call(const g4c_mlp_t *mlp, const g4c_src_t *srcs, int32_t n_src, int64_t n_rows, const g4c_mlp_io_t *io, Launch &L) {
    G4C_REQUIRE(io && io->size == (int32_t)sizeof(g4c_mlp_io_t), G4C_EINVAL,
                "g4c_mlp_run: io->size %d, this library's g4c_mlp_io_t has %d bytes (a binding out of step with g4c.h)", io ? io->size : 0,
                (int)sizeof(g4c_mlp_io_t));
    G4C_REQUIRE(mlp && srcs, G4C_EINVAL, "g4c_mlp_run: null pointer");
    const int fmt = L.fmt = mlp->w_format;
    G4C_REQUIRE(fmt >= G4C_WFMT_FP32 && fmt <= G4C_WFMT_BF16, G4C_EINVAL, "g4c_mlp_run: unknown w_format %d", fmt);
    L.row_split = fmt == G4C_WFMT_BF16_RS || fmt == G4C_WFMT_BF16_RS2 || fmt == G4C_WFMT_BF16_RS2N;
    L.round1 = fmt == G4C_WFMT_BF16 || L.row_split;
    L.f16x2 = fmt == G4C_WFMT_F16X2;
    L.bx6 = fmt != G4C_WFMT_FP32;
    L.agg = io->agg != nullptr; L.save = io->n_save != 0; L.has_node = io->upd != nullptr;
    L.row_begin = io->row_begin; L.row_count = io->row_count; L.io_n_tiles = io->n_tiles;
    G4C_REQUIRE(L.row_begin >= 0 && L.row_count >= 0 && L.row_begin + L.row_count <= n_rows && L.row_begin % 32 == 0, G4C_EINVAL,
                "g4c_mlp_run: bad row range [%lld, +%lld) of %lld (row_begin must be a multiple of 32)", L.row_begin, L.row_count,
                (long long)n_rows);
    G4C_REQUIRE(n_src >= 1 && n_src <= G4C_MAX_SRC, G4C_EUNSUPPORTED, "g4c_mlp_run: %d sources (max %d)", n_src, G4C_MAX_SRC);
    G4C_REQUIRE(mlp->n_layers >= 1 && mlp->n_layers <= G4C_MAX_LAYERS, G4C_EUNSUPPORTED,
                "g4c_mlp_run: %d layers (supported 1..%d)", mlp->n_layers, G4C_MAX_LAYERS);
    G4C_REQUIRE(n_rows >= 0 && n_rows < (1LL << 31), G4C_EINVAL, "g4c_mlp_run: n_rows %lld out of range", (long long)n_rows);
    G4C_REQUIRE(io->act >= 0 && io->act <= 2, G4C_EINVAL, "g4c_mlp_run: bad activation %d", io->act);
    G4C_REQUIRE(io->n_heads >= 0 && io->n_heads <= G4C_MAX_HEADS, G4C_EINVAL, "g4c_mlp_run: bad heads (n=%d)", io->n_heads);
    G4C_REQUIRE((L.row_begin == 0 && L.row_count == n_rows) || (!L.agg && !L.save && !L.has_node && !io->n_heads && !io->out_dtype),
                G4C_EUNSUPPORTED, "g4c_mlp_run: a row sub-range needs a plain launch (no heads / aggregation / save / upd / out_dtype)");
    // (the plan: tiles of whole segments; row ranges alone — segments longer than a tile — run on the one form that needs no tiles)
    G4C_REQUIRE(!L.agg || (io->seg_off && io->agg_ld >= NP && ((io->tile_rows && io->tile_seg && io->n_tiles >= 0) || (io->wg_rows && !io->tile_rows))),
                G4C_EINVAL, "g4c_mlp_run: bad aggregation plan");
    G4C_REQUIRE(io->out_dtype == G4C_DTYPE_F32 || io->out_dtype == G4C_DTYPE_BF16 || io->out_dtype == G4C_DTYPE_BF16_SELU, G4C_EINVAL,
                "g4c_mlp_run: unknown out_dtype %d", io->out_dtype);
    G4C_REQUIRE(io->out_dtype != G4C_DTYPE_BF16_SELU || (L.agg && io->act == G4C_ACT_NONE), G4C_EINVAL,
                "g4c_mlp_run: G4C_DTYPE_BF16_SELU needs the fused aggregation and no output activation");
    G4C_REQUIRE(io->head_dtype == G4C_DTYPE_F32 || io->head_dtype == G4C_DTYPE_BF16, G4C_EINVAL, "g4c_mlp_run: unknown head_dtype %d", io->head_dtype);
    G4C_REQUIRE(!io->range_flag || (mlp->range_slot >= 0 && (!L.has_node || io->upd->range_slot >= 0)), G4C_EINVAL,
                "g4c_mlp_run: negative range_slot (mlp %d, upd %d)", mlp->range_slot, L.has_node ? io->upd->range_slot : 0);
    return G4C_OK;
}

// ---- stage: the input blocks — weighted (Params::src), additive (::add) and narrow (::nar) -----------------------------------------------
int stage_sources(const g4c_src_t *srcs, int32_t n_src, int32_t k_pad0, Launch &L) {
    Params &p = L.p;
    const bool bx6 = L.bx6, round1 = L.round1;
    int kp = 0, nk = 0;
    L.all_vec = true;
    for (int s = 0; s < n_src; ++s) {
        const g4c_src_t &g = srcs[s];
        G4C_REQUIRE(g.ptr && g.width > 0 && g.ld >= g.col0 + g.width && g.col0 >= 0, G4C_EINVAL,
                    "g4c_mlp_run: bad source %d (width=%d ld=%d col0=%d)", s, g.width, g.ld, g.col0);
        if (g.additive == 2) {
            G4C_REQUIRE(bx6, G4C_EUNSUPPORTED, "g4c_mlp_run: narrow sources (additive == 2) need a split-operand w_format");
            G4C_REQUIRE(g.width <= G4C_NARROW_MAX && !g.idx && g.pre_act == G4C_ACT_NONE && g.w && ((uintptr_t)g.w & 15) == 0, G4C_EINVAL,
                        "g4c_mlp_run: bad narrow source %d (width %d <= %d, no index, no pre_act, 16-byte aligned weights)", s,
                        g.width, G4C_NARROW_MAX);
            NarSrc &a = p.nar[p.n_nar++];
            a.ptr = g.ptr + g.col0; a.w = g.w; a.width = g.width; a.ld = g.ld;
            continue;
        }
        if (g.additive) {
            G4C_REQUIRE(g.pre_act == G4C_ACT_NONE && g.width <= NP && (g.dtype == G4C_DTYPE_F32 || g.dtype == G4C_DTYPE_BF16), G4C_EINVAL,
                        "g4c_mlp_run: bad additive source %d", s);
            AddSrc &a = p.add[p.n_add++];
            a.idx = g.idx; a.width = g.width; a.ld = g.ld; a.bf16 = g.dtype == G4C_DTYPE_BF16;
            if (a.bf16) {
                G4C_REQUIRE(round1 && g.width == NP && g.ld % 4 == 0 && g.col0 % 4 == 0 && (uintptr_t)g.ptr % 8 == 0, G4C_EUNSUPPORTED,
                            "g4c_mlp_run: bf16 additive rows need the rounded-bf16 mode (w_format G4C_WFMT_BF16*) and a 128-wide, 8-byte aligned block");
                a.ptr = reinterpret_cast<const float *>(reinterpret_cast<const __bf16 *>(g.ptr) + g.col0);
            } else {
                a.ptr = g.ptr + g.col0;
            }
            continue;
        }
        G4C_REQUIRE(g.pre_act == G4C_ACT_NONE || g.pre_act == G4C_ACT_SELU, G4C_EUNSUPPORTED,
                    "g4c_mlp_run: source %d pre_act %d (only NONE / SELU can be applied on load)", s, g.pre_act);
        Src &d = p.src[nk++];
        if (bx6) G4C_REQUIRE(g.width <= NP, G4C_EUNSUPPORTED, "g4c_mlp_run: input block %d is %d wide (max 128 in a split-operand w_format)", s, g.width);
        d.ptr = g.ptr; d.idx = g.idx; d.width = g.width; d.wpad = bx6 ? NP : (g.width + KC - 1) / KC * KC; d.ld = g.ld; d.col0 = g.col0;
        d.pre_act = g.pre_act;
        d.bf16 = g.dtype == G4C_DTYPE_BF16;
        if (d.bf16)
            G4C_REQUIRE(round1 && g.width == NP && !g.seg_off && g.ld % 4 == 0 && g.col0 % 4 == 0 && (uintptr_t)g.ptr % 8 == 0, G4C_EUNSUPPORTED,
                        "g4c_mlp_run: bf16 rows need the rounded-bf16 mode (w_format G4C_WFMT_BF16*) and a 128-wide, 8-byte aligned block");
        else
            G4C_REQUIRE(g.dtype == G4C_DTYPE_F32, G4C_EINVAL, "g4c_mlp_run: source %d has unknown dtype %d", s, g.dtype);
        d.seg_off = g.seg_off; d.seg_mean = g.seg_mean; d.seg_perm = g.seg_off ? g.seg_perm : nullptr;
        if (g.seg_off)
            G4C_REQUIRE(bx6 && !g.idx && g.width == NP && g.ld % 4 == 0 && g.col0 % 4 == 0 && (uintptr_t)g.ptr % 16 == 0, G4C_EUNSUPPORTED,
                        "g4c_mlp_run: aggregation on load needs a split-operand w_format and a 128-wide aligned block without gather index");
        d.vec = (g.width % 4 == 0) && (g.ld % 4 == 0) && (g.col0 % 4 == 0) && ((uintptr_t)g.ptr % (d.bf16 ? 8 : 16) == 0);
        L.all_vec = L.all_vec && d.vec;
        kp += d.wpad;
    }
    // (every source additive: the first layer is precomputed, g4c_mlp_t.k_pad — the stream then has no layer 0, checked below)
    L.pre = nk == 0 && p.n_nar == 0 && p.n_add >= 1;
    G4C_REQUIRE(nk >= 1 || p.n_nar >= 1 || L.pre, G4C_EINVAL, "g4c_mlp_run: no input block goes through the weights");
    p.n_src = nk;
    if (nk == 0) p.src[0] = Src{nullptr, nullptr, 0, 0, 0, 0, 1, 0, nullptr, 0, nullptr, 0};
    for (int s = (nk ? nk : 1); s < G4C_MAX_SRC; ++s) p.src[s] = p.src[0];
    G4C_REQUIRE(kp == k_pad0, G4C_EINVAL, "g4c_mlp_run: sources give %d padded columns, layer 1 packed for %d", kp, k_pad0);
    p.chunks0 = kp / KC;
    return G4C_OK;
}

// One contiguous stream and one contiguous bias block: layer l starts where layer l-1 ends (`mlp` and `upd` alike; the texts name whose)
int check_contiguous(const g4c_mlp_t *m, int wbytes, const char *w_text, const char *b_text) {
    for (int l = 1; l < m->n_layers; ++l) {
        G4C_REQUIRE((const char *)m->w[l] == (const char *)m->w[l - 1] + (size_t)m->k_pad[l - 1] * NP * wbytes, G4C_EINVAL, w_text, l);
        G4C_REQUIRE((const float *)m->b[l] == (const float *)m->b[l - 1] + NP, G4C_EINVAL, b_text, l);
    }
    return G4C_OK;
}

// ---- stage: the layers — packed stream, biases, LayerNorm ------------------------------------------------------------------------------
int stage_stream(const g4c_mlp_t *mlp, Launch &L) {
    Params &p = L.p;
    p.n_layers = mlp->n_layers;
    for (int l = 0; l < mlp->n_layers; ++l) {
        G4C_REQUIRE(mlp->n_pad[l] == NP, G4C_EINVAL, "g4c_mlp_run: layer %d n_pad %d (must be 128)", l, mlp->n_pad[l]);
        if (l > 0) G4C_REQUIRE(mlp->k_pad[l] == NP, G4C_EINVAL, "g4c_mlp_run: layer %d k_pad %d (must be 128)", l, mlp->k_pad[l]);
    }
    if (const int rc = check_contiguous(mlp, L.bx6 ? 6 : 4, "g4c_mlp_run: packed layers must be contiguous (layer %d)",
                                        "g4c_mlp_run: padded biases must be contiguous (layer %d)"))
        return rc;
    p.w = (const float *)mlp->w[0]; p.b = (const float *)mlp->b[0];
    G4C_REQUIRE(p.w && p.b, G4C_EINVAL, "g4c_mlp_run: null weights");
    p.gamma = mlp->ln_gamma; p.beta = mlp->ln_beta; p.eps = mlp->ln_eps;
    G4C_REQUIRE((p.gamma == nullptr) == (p.beta == nullptr), G4C_EINVAL, "g4c_mlp_run: LayerNorm needs both gamma and beta");
    p.n_out = mlp->n_out;
    return G4C_OK;
}

// ---- stage: what the launch writes — output rows, residual, output index, bf16 rows, the fused aggregation ------------------------------
int stage_outputs(const g4c_mlp_io_t *io, Launch &L) {
    Params &p = L.p;
    p.out = (float *)io->out; p.out_ld = io->out_ld; p.out_idx = io->out_idx; p.act = io->act;
    G4C_REQUIRE(p.out || L.agg, G4C_EINVAL, "g4c_mlp_run: null output");
    G4C_REQUIRE(p.n_out > 0 && p.n_out <= NP && p.out_ld >= p.n_out, G4C_EINVAL, "g4c_mlp_run: n_out=%d out_ld=%d", p.n_out, p.out_ld);
    p.resid = io->resid; p.resid_ld = io->resid_ld; p.resid_col0 = io->resid_col0;
    p.row_base = L.row_begin;
    p.M = L.row_begin + L.row_count;          // rows past the range are neither gathered nor stored
    if (L.agg) {
        G4C_REQUIRE(L.bx6 && p.n_out == NP && !p.out_idx && !p.resid, G4C_EUNSUPPORTED,
                    "g4c_mlp_run: the fused aggregation needs a split-operand w_format and a plain 128-wide output");
        const int32_t mode = io->agg_mode;
        p.tile_rows = io->tile_rows; p.tile_seg = io->tile_seg; p.seg_off = io->seg_off;
        p.agg = (float *)io->agg; p.agg_ld = io->agg_ld; p.agg_mean = mode & 1; p.agg_deg = (mode >> 8) & 0xff; p.agg_bf16 = (mode >> 16) & 1;
        const bool rs_fmt = L.fmt == G4C_WFMT_BF16_RS;
        G4C_REQUIRE((mode >> 17) == 0 && (!p.agg_bf16 || rs_fmt) && p.agg_deg <= 32 && (p.agg_deg == 0 || L.row_count % p.agg_deg == 0), G4C_EINVAL,
                    "fused aggregation: agg_mode = %d is not 0 / 1 [| G4C_AGG_UNIFORM(k), 1 <= k <= 32, k dividing the %lld rows]", mode,
                    L.row_count);
        // (uniform segments: the kernels derive them as row / k over [0, M) and cannot honour a sub-range.  A guard only: stage_call has
        // already tied an aggregation to the whole row range.)
        G4C_REQUIRE(p.agg_deg == 0 || L.row_begin == 0, G4C_EINVAL,
                    "g4c_mlp_run: uniform segments (G4C_AGG_UNIFORM) need the whole row range, got rows [%lld, %lld)", L.row_begin, p.M);
        if (io->wg_rows) {
            G4C_REQUIRE(io->wg_seg && io->n_wg >= 1 && io->n_wg <= g4c::cu_count() && io->wg_pairs >= 1 && io->wg_max_seg >= 1 && L.row_begin == 0,
                        G4C_EINVAL, "g4c_mlp_run: bad row ranges (n_wg=%d wg_pairs=%d wg_max_seg=%d)", io->n_wg, io->wg_pairs, io->wg_max_seg);
            p.wg_rows = io->wg_rows; p.wg_seg = io->wg_seg; p.n_wg = io->n_wg; p.wg_pairs = io->wg_pairs; p.wg_max_seg = io->wg_max_seg;
        }
    }
    if (io->out_dtype) {
        G4C_REQUIRE(L.round1 && !p.resid && !p.out_idx && p.n_out == NP && (!p.out || ((p.out_ld & 3) == 0 && ((uintptr_t)p.out & 7) == 0)), G4C_EUNSUPPORTED,
                    "g4c_mlp_run: bf16 output rows need the rounded-bf16 mode, a plain 128-wide output, out_ld a multiple of 4 and an 8-byte aligned out");
        p.out_bf16 = io->out_dtype;
    }
    return G4C_OK;
}

// ---- stage: the training forms — save[] of every layer's rows, mul[] of the backward chain ------------------------------------------------
int stage_save(const g4c_mlp_io_t *io, Launch &L) {
    Params &p = L.p;
    const int n_layers = p.n_layers;
    if (!L.save) return G4C_OK;
    // (the rounded-bf16 stream saves on the plain tile kernel only: the row-split streams keep refusing)
    G4C_REQUIRE(L.bx6 && (!L.round1 || L.fmt == G4C_WFMT_BF16) && !io->out_dtype && !L.agg && !io->n_heads && !p.out_idx && io->save_ld >= NP &&
                    (io->save_ld & 3) == 0,
                G4C_EUNSUPPORTED,
                "g4c_mlp_run: save needs w_format BF16X3 / F16X2 / BF16 without heads / aggregation / output index / bf16 rows, save_ld >= 128 "
                "and a multiple of 4");
    G4C_REQUIRE(io->n_save == n_layers, G4C_EINVAL, "g4c_mlp_run: n_save %d for %d layers", io->n_save, n_layers);
    // bf16 save / mul rows: the SP = 1 instantiations only (the plain rounded-bf16 stream); the split streams keep fp32 rows
    G4C_REQUIRE((io->save_dtype == G4C_DTYPE_F32 || io->save_dtype == G4C_DTYPE_BF16) &&
                    (io->mul_dtype == G4C_DTYPE_F32 || io->mul_dtype == G4C_DTYPE_BF16),
                G4C_EINVAL, "g4c_mlp_run: save_dtype %d / mul_dtype %d (G4C_DTYPE_F32 or G4C_DTYPE_BF16)", io->save_dtype, io->mul_dtype);
    G4C_REQUIRE((!io->save_dtype && !io->mul_dtype) || L.fmt == G4C_WFMT_BF16, G4C_EINVAL,
                "g4c_mlp_run: bf16 save / mul rows need w_format G4C_WFMT_BF16 (the plain rounded-bf16 stream); w_format %d keeps fp32 rows",
                L.fmt);
    bool mul = false;
    for (int l = 0; l < n_layers; ++l) {
        G4C_REQUIRE(((uintptr_t)io->save[l] & 15) == 0, G4C_EINVAL, "g4c_mlp_run: save[%d] is not 16-byte aligned", l);
        p.save[l] = static_cast<float *>(io->save[l]);
        if (l + 1 == n_layers) break;
        G4C_REQUIRE(((uintptr_t)io->mul[l] & 15) == 0, G4C_EINVAL, "g4c_mlp_run: mul[%d] is not 16-byte aligned", l);
        p.mul[l] = static_cast<const float *>(io->mul[l]);
        mul = mul || io->mul[l];
    }
    p.save_bf16 = io->save_dtype == G4C_DTYPE_BF16;
    p.mul_bf16 = io->mul_dtype == G4C_DTYPE_BF16;
    p.save_ld = io->save_ld;
    G4C_REQUIRE(!mul || (io->mul_ld >= NP && (io->mul_ld & 3) == 0), G4C_EINVAL, "g4c_mlp_run: mul_ld=%d", io->mul_ld);
    p.mul_ld = io->mul_ld;
    return G4C_OK;
}

// ---- stage: the fp16 range — the caller's certificate, else its flag words --------------------------------------------------------------
// The certificate (g4c_mlp_t.range_certified) holds for the launch when every MLP of it carries one, in the f16x3 stream, without
// save / mul — then nothing is tracked and no flag word is written.
void stage_range(const g4c_mlp_t *mlp, const g4c_mlp_io_t *io, Launch &L) {
    L.p.range_certified = (L.f16x2 && mlp->range_certified && !L.save && (!L.has_node || io->upd->range_certified)) ? 1 : 0;
    L.p.range_flag = (L.f16x2 && !L.p.range_certified) ? io->range_flag : nullptr;
    L.p.range_slot = mlp->range_slot;
}

// ---- stage: heads (the kernels read their weights where the stream of the MLP that owns them ends; with `upd`, that MLP's) ------------
int stage_heads(const g4c_mlp_io_t *io, Launch &L) {
    Params &p = L.p;
    const int n_heads = io->n_heads;
    for (int hd = 0; hd < n_heads; ++hd) G4C_REQUIRE(io->head_out[hd], G4C_EINVAL, "g4c_mlp_run: null head output %d", hd);
    if (L.has_node || !n_heads) return G4C_OK;          // (with `upd` the heads are its: stage_node)
    p.n_heads = n_heads; p.head_ld = io->head_ld;
    for (int hd = 0; hd < n_heads; ++hd) p.head_out[hd] = (float *)io->head_out[hd];
    if (io->head_dtype) {
        G4C_REQUIRE(L.round1 && (p.head_ld & 1) == 0, G4C_EUNSUPPORTED, "g4c_mlp_run: bf16 head rows need the rounded-bf16 mode and an even head_ld");
        for (int hd = 0; hd < n_heads; ++hd)
            G4C_REQUIRE(((uintptr_t)io->head_out[hd] & 3) == 0, G4C_EINVAL, "g4c_mlp_run: head output %d is not 4-byte aligned", hd);
        p.head_bf16 = 1;
    }
    G4C_REQUIRE(!L.agg, G4C_EUNSUPPORTED, "g4c_mlp_run: heads with the fused aggregation");
    G4C_REQUIRE((p.head_ld & 3) == 0 || !L.bx6, G4C_EINVAL, "g4c_mlp_run: head outputs need a leading dimension that is a multiple of 4");
    G4C_REQUIRE(p.n_out == NP && !p.resid && !p.out_idx && p.head_ld >= NP, G4C_EINVAL,
                "g4c_mlp_run: heads need a 128-wide output without residual / output index (n_out=%d)", p.n_out);
    return G4C_OK;
}

// ---- stage: the node update fused behind the message launch (io->upd; mlp_ws.hip, NODE) ---------------------------------------------------
int stage_node(const g4c_mlp_io_t *io, Launch &L) {
    if (!L.has_node) return G4C_OK;
    const g4c_mlp_t *u = io->upd;
    const int n_heads = io->n_heads;
    G4C_REQUIRE(L.f16x2 && L.agg && u->w_format == G4C_WFMT_F16X2 && io->act == G4C_ACT_NONE, G4C_EUNSUPPORTED,
                "g4c_mlp_run: the fused node update needs the f16x3 format (G4C_WFMT_F16X2) for both MLPs, the aggregation plan and act NONE");
    G4C_REQUIRE(u->n_layers == L.p.n_layers && u->k_pad[0] == 2 * NP && u->n_out == NP && u->w[0] && u->b[0], G4C_EUNSUPPORTED,
                "g4c_mlp_run: upd must have the message MLP's depth (%d), two 128-wide input blocks and a 128-wide output", L.p.n_layers);
    for (int l = 0; l < u->n_layers; ++l)
        G4C_REQUIRE(u->n_pad[l] == NP && (l == 0 || u->k_pad[l] == NP), G4C_EUNSUPPORTED, "g4c_mlp_run: upd layer %d is not 128 wide", l);
    const char *const text = "g4c_mlp_run: upd's packed layers / biases must be contiguous (layer %d)";
    if (const int rc = check_contiguous(u, 6, text, text)) return rc;
    G4C_REQUIRE((u->ln_gamma == nullptr) == (u->ln_beta == nullptr), G4C_EINVAL, "g4c_mlp_run: upd's LayerNorm needs both gamma and beta");
    G4C_REQUIRE(!u->ln_gamma || (((uintptr_t)u->ln_gamma & 15) == 0 && ((uintptr_t)u->ln_beta & 15) == 0), G4C_EINVAL,
                "g4c_mlp_run: upd's LayerNorm parameters must be 16-byte aligned");
    G4C_REQUIRE(io->v && io->v_out && (io->v_ld & 3) == 0 && io->v_ld >= NP && (io->v_out_ld & 3) == 0 && io->v_out_ld >= NP &&
                ((uintptr_t)io->v & 15) == 0 && ((uintptr_t)io->v_out & 15) == 0 && (io->agg_ld & 3) == 0 && ((uintptr_t)io->agg & 15) == 0,
                G4C_EINVAL, "g4c_mlp_run: v / v_out / agg need 16-byte aligned rows of at least 128 columns");
    G4C_REQUIRE(io->v_act >= 0 && io->v_act <= 2, G4C_EINVAL, "g4c_mlp_run: bad v_act %d", io->v_act);
    NodeParams &q = L.node;
    q.v = io->v; q.v_ld = io->v_ld; q.w = (const float *)u->w[0]; q.b = (const float *)u->b[0];
    q.gamma = u->ln_gamma; q.beta = u->ln_beta; q.eps = u->ln_eps; q.act = io->v_act;
    q.out = io->v_out; q.out_ld = io->v_out_ld; q.n_heads = n_heads; q.head_ld = io->head_ld;
    q.range_flag = L.p.range_certified ? nullptr : io->range_flag; q.range_slot = u->range_slot;
    if (n_heads) {
        G4C_REQUIRE(io->head_dtype == G4C_DTYPE_F32 && (io->head_ld & 3) == 0 && io->head_ld >= NP, G4C_EINVAL,
                    "g4c_mlp_run: upd's heads need fp32 rows, head_ld a multiple of 4 and >= 128");
        for (int hd = 0; hd < n_heads; ++hd) {
            G4C_REQUIRE(((uintptr_t)io->head_out[hd] & 15) == 0, G4C_EINVAL, "g4c_mlp_run: bad head output %d", hd);
            q.head_out[hd] = (float *)io->head_out[hd];
        }
    }
    return G4C_OK;
}

// ---- choose: the family of this launch, by the table at the top of the file.  All policy is here. ----------------------------------------
typedef int (*LaunchFn)(const Launch &, hipStream_t, Ran &);

bool at_size(const std::atomic<int> &mode_knob, long long min_rows, const Launch &L) {
    const int mode = mode_knob.load(std::memory_order_relaxed);
    return mode == 2 || (mode == 1 && L.row_count >= min_rows);
}

// (nullptr: refused — G4C_EUNSUPPORTED, the text set)
LaunchFn choose(Launch &L) {
    L.deep_ring = L.p.n_tiles <= g_deep_tiles.load(std::memory_order_relaxed);
    L.shapes = g_shapes.load(std::memory_order_relaxed) != 0;
    L.tile_form = L.p.n_tiles > TILE_ROWS64_FILL * g_deep_tiles.load(std::memory_order_relaxed) ? g_tile_form.load(std::memory_order_relaxed) : 0;
    if (L.pre) {
        G4C_REQUIRE(!L.has_node, nullptr, "g4c_mlp_run: every source additive (first layer precomputed) with upd: the fused MP layer has no such form");
        G4C_REQUIRE(L.f16x2, nullptr, "g4c_mlp_run: every source additive (first layer precomputed) needs the f16x3 format (G4C_WFMT_F16X2), got w_format %d", L.fmt);
        G4C_REQUIRE(L.p.n_layers == 3, nullptr, "g4c_mlp_run: every source additive (first layer precomputed) needs three layers (two left), got %d", L.p.n_layers);
        G4C_REQUIRE(L.agg && !L.save, nullptr, "g4c_mlp_run: every source additive (first layer precomputed) needs the fused aggregation and no save");
        G4C_REQUIRE(L.p.tile_rows, nullptr, "g4c_mlp_run: every source additive (first layer precomputed) needs the tiles of whole segments");
        G4C_REQUIRE(ws_pre_takes(L), nullptr,
                    "g4c_mlp_run: every source additive (first layer precomputed) is outside the weight-stationary kernel's envelope (three aligned "
                    "128-wide fp32 additive blocks — the first direct, two through indices —, a plain fp32 128-wide output, no heads / residual "
                    "/ output index / out_dtype)");
        return ws_launch;
    }
    if (L.has_node) {
        G4C_REQUIRE(ws_takes(L), nullptr,
                    "g4c_mlp_run: the message launch of the fused MP layer is outside the weight-stationary kernel's envelope (one 128-wide "
                    "weighted block, two 128-wide additive blocks, two or three 128-wide layers, aligned rows)");
        G4C_REQUIRE(L.p.tile_rows || ws_any_takes(L), nullptr, "g4c_mlp_run: a fused MP layer without tiles of whole segments is outside the row-range form's envelope");
        return ws_launch;
    }
    if (L.agg && !L.p.tile_rows) {
        G4C_REQUIRE(!L.row_split && ws_takes(L) && ws_any_takes(L), nullptr,
                    "g4c_mlp_run: an aggregation plan of row ranges alone needs the weight-stationary kernel's row-range form (f16x3, one direct "
                    "128-wide weighted block, two 128-wide additive blocks, two or three layers, fp32 rows, ranges within what it stages on chip)");
        return ws_launch;
    }
    if (L.fmt == G4C_WFMT_BF16_RS) {
        G4C_REQUIRE(!L.save && rs_takes(L), nullptr,
                    "g4c_mlp_run: weights packed for the row-split kernel (G4C_WFMT_BF16_RS), launch outside its envelope");
        return rs_launch;
    }
    if (L.row_split) {
        G4C_REQUIRE(!L.save && !L.agg && rs2_takes(L), nullptr,
                    "g4c_mlp_run: weights packed for the row-split update kernel (G4C_WFMT_BF16_RS2), launch outside its envelope");
        return rs2_launch;
    }
    if (at_size(g_ws_mode, WS_MIN_ROWS, L) && ws_takes(L)) return ws_launch;
    if (at_size(g_bx6i_mode, BX6I_MIN_ROWS, L) && bx6i_takes(L)) return bx6i_launch;
    return tile_takes(L) ? tile_launch : split_launch;
}

}  // namespace

extern "C" int g4c_mlp_run(const g4c_mlp_t *mlp, const g4c_src_t *srcs, int32_t n_src, int64_t n_rows, const g4c_mlp_io_t *io,
                           void *stream) {
    g_last = Ran{};
    Launch L{};          // (zeros: every stage fills what its part of the call uses)
    int rc;
    if ((rc = stage_call(mlp, srcs, n_src, n_rows, io, L))) return rc;
    if (n_rows == 0) return G4C_OK;
    g4c::DeviceGuard on_device(mlp->w[0]);
    if ((rc = stage_sources(srcs, n_src, mlp->k_pad[0], L))) return rc;
    if ((rc = stage_stream(mlp, L))) return rc;
    if ((rc = stage_outputs(io, L))) return rc;
    if ((rc = stage_save(io, L))) return rc;
    stage_range(mlp, io, L);
    if ((rc = stage_heads(io, L))) return rc;
    if (L.row_count == 0) return G4C_OK;
    if ((rc = stage_node(io, L))) return rc;
    // tiles: whole segments from the caller's plan with the fused aggregation (the row-split kernels cut the rows themselves and
    // do not look at it), else 32 rows each
    L.p.n_tiles = (L.agg && !L.row_split && io->tile_rows) ? L.io_n_tiles : (int)((L.row_count + 31) / 32);
    const LaunchFn launch = choose(L);
    if (!launch) return G4C_EUNSUPPORTED;
    if (L.p.n_tiles == 0) return G4C_OK;          // (nothing launches: g4c_mlp_last_kernel stays G4C_KERNEL_NONE)
    return launch(L, (hipStream_t)stream, g_last);
}

extern "C" int g4c_mlp_ws_enable(int on) { return knob(g_ws_mode, on, 2); }
extern "C" int g4c_mlp_bx6i_enable(int on) { return knob(g_bx6i_mode, on, 2); }
extern "C" int g4c_mlp_small_launch_tiles(int n_tiles) { return knob(g_deep_tiles, n_tiles, INT_MAX); }
extern "C" int g4c_mlp_shapes_enable(int on) { return knob(g_shapes, on, 1); }
extern "C" int g4c_mlp_tile_form(int form) { return knob(g_tile_form, form, 1); }
extern "C" int g4c_mlp_last_tile_rows(void) { return g_last.tile_rows; }
extern "C" int g4c_mlp_last_kernel(void) { return g_last.kernel; }
extern "C" int g4c_mlp_last_shape(void) { return g_last.shape; }
extern "C" int g4c_mlp_last_row_ranges(void) { return g_last.ranges; }
