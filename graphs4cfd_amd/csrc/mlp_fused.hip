// Fused gather -> concat -> MLP (fp32 MFMA) -> LayerNorm -> activation -> residual -> store.
//
// Replaces, in ONE launch, what the reference issues as ~10-25 torch kernels per MLP call:
// `torch.cat((e, v[row], v[col]))` + nn.Linear/nn.SELU chain + nn.LayerNorm (MLP.forward,
// graphs4cfd/nn/blocks.py:117-144) + the F.selu / torch.tanh applied by the caller
// (nn/mus_gnn.py:178-212, nn/blocks.py:233,288) + the residual time step (nn/mus_gnn.py:218).
// The concatenated input is never materialised: each source is gathered row-wise into LDS.
//
// Design (CDNA4, wave64): ONE WAVE owns RT*32 rows (RT = 2 for large launches, 1 otherwise) through
// every layer, so there is no workgroup barrier anywhere and waves never wait for each other.
//   * every layer is computed 128 wide (narrower layers are zero-padded when packed) on
//     v_mfma_f32_32x32x2_f32: RT x 4 accumulators of 16 VGPRs; per 4 k: RT ds_read_b64 of A,
//     two 16-byte global loads of B, RT*8 MFMAs (1024 cycles at RT = 2);
//   * weights (B) stream L2 -> registers through an 8-deep ring (one ring slot per 4 k, refilled
//     for the next 32-k chunk right after use): no LDS staging of weights, ~3.5 us of prefetch;
//   * the gathered input chunk [RT*32 x 32] goes global -> registers -> wave-private LDS, one chunk
//     ahead; hidden activations live in wave-private LDS ([RT*32][132] fp32, aliasing the input
//     buffers) between layers;
//   * LayerNorm / activation / residual: one lane per (row, half), one cross-half exchange, then
//     whole-row 16-byte stores.
// 64-thread workgroups, 34 KiB LDS at RT = 2 -> 4 waves per CU (one per SIMD, 512 VGPRs each).
//
// MFMA-bound in fp32: 2*K*128 FLOP per row per layer against ~(K_in + N_out)*4 bytes per row.
#include "mlp_common.h"
#include <type_traits>
using namespace g4cm;

// Timing-only ablations, compile-time so that the production kernel has no extra control flow
// (a runtime switch between two mma_chunk instantiations makes hipcc reconcile the weight-ring
// registers at the join, i.e. wait for the in-flight loads at every chunk):
//   -DG4C_ABLATE=1 no ring refill, 2 no input staging, 4 no epilogues / final pass (bits can be OR-ed)
#ifndef G4C_ABLATE
#define G4C_ABLATE 0
#endif

// -DG4C_TIMING: per-phase s_memtime stamps of the first 4096 tiles into g4c_dbg_stamps (debug builds only)
#ifdef G4C_TIMING
__device__ unsigned long long g4c_dbg_stamps[4096 * 16];
#define G4C_STAMP(k) do { if (tile < 4096 && lane == 0) g4c_dbg_stamps[tile * 16 + (k)] = __builtin_readcyclecounter(); } while (0)
extern "C" int g4c_debug_read_stamps(unsigned long long *host, int n) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g4c_dbg_stamps), sizeof(unsigned long long) * n);
}
#define G4C_STAMPW(k) do { if (tile < 4096 && tid == 0) g4c_dbg_stamps[tile * 16 + (k)] = __builtin_readcyclecounter(); } while (0)
#else
#define G4C_STAMP(k) do {} while (0)
#define G4C_STAMPW(k) do {} while (0)
#endif

namespace {


// offset of 4-k step U inside a chunk of the weight stream: steps are stored in pairs (see pack_layer_kernel)
__host__ __device__ constexpr int step_off(int U) { return (U >> 1) * 1024 + (U & 1) * 2; }


// ---- gathered input chunk: lane (r = lane>>3 [+8q], c4 = lane&7) loads 4 consecutive columns.
// VEC: every source is 16-byte addressable (width, ld, col0 multiples of 4, aligned base) -> one
// unconditional 16-byte load per row; the generic path does 4 clamped scalar loads.
template <bool VEC>
__device__ __forceinline__ f32x4 ldx1(const Src &s, int srow, int c) {
    const float *base = s.ptr + (long long)srow * s.ld + s.col0;
    f32x4 t;
    if (VEC) {
        // columns beyond the source width (padding up to 32) are zero-filled by select; the load
        // itself is unconditional from a clamped column (no path-dependent load count: hipcc can
        // then wait for these loads with an exact vmcnt instead of draining the weight ring)
        // (the zero fill itself happens in finish_x, after the MFMAs: touching the loaded value here
        // would make the wave wait for the gather before it starts computing)
        t = *reinterpret_cast<const f32x4 *>(base + (c < s.width ? c : 0));
    } else {
        const int w1 = s.width - 1;
        t[0] = base[c + 0 < w1 ? c + 0 : w1];
        t[1] = base[c + 1 < w1 ? c + 1 : w1];
        t[2] = base[c + 2 < w1 ? c + 2 : w1];
        t[3] = base[c + 3 < w1 ? c + 3 : w1];
    }
    return t;
}

// ======================================================================================================
// The fp32-MFMA kernel (precision "fp32", and the launches the bf16x6 kernel cannot take): NW = 4 waves share
// one 32-row tile, each computing NCT = 4/NW of the four 32-column tiles.  (Round 1 also carried single-wave 64- / 32-row
// tiles, a 2-wave split, a 64-row split and a small-launch variant; the 4-wave split was the fastest or within 2 % of the
// fastest at every launch size, and the others were removed.)
// The waves of a tile share the gathered input chunk and the hidden activations through LDS:
// one barrier per layer-0 chunk, two per layer.  Weights still stream L2 -> registers (each wave only its
// own column tiles), accumulators stay in registers.
template <int NCT> struct BVec;
template <> struct BVec<2> { typedef f32x4 type; };
template <> struct BVec<1> { typedef float2 type; };

__device__ __forceinline__ void load_bn(float2 &b, const float *wstep, unsigned lane_off) {
    b = *reinterpret_cast<const float2 *>(wstep + lane_off);
}
__device__ __forceinline__ void load_bn(f32x4 &b, const float *wstep, unsigned lane_off) {
    const float2 c0 = *reinterpret_cast<const float2 *>(wstep + lane_off);
    const float2 c1 = *reinterpret_cast<const float2 *>(wstep + lane_off + 256);
    b[0] = c0.x; b[1] = c0.y; b[2] = c1.x; b[3] = c1.y;
}

template <int NCT> struct AccN { f32x16 t[NCT]; };
template <int NCT> struct RingN { typename BVec<NCT>::type s0, s1, s2, s3, s4, s5, s6, s7; };

__device__ __forceinline__ float bget(const f32x4 &b, int k) { return b[k]; }
__device__ __forceinline__ float bget(const float2 &b, int k) { return k ? b.y : b.x; }

// (tried on this kernel and measured neutral or worse in round 1, now constants: s_setprio around the MFMAs, LayerNorm parameters
// from global memory at 8 workgroups per CU ("slim"), 7 waves per SIMD)
constexpr int G4C_SPLIT_PRIO = 0;
constexpr int G4C_SPLIT_SLIM = 0;
template <int NCT>
__device__ __forceinline__ void mma_chunk_n(const float *pa, RingN<NCT> &g, const float *wnext, unsigned lo, AccN<NCT> &acc) {
    float2 a = *reinterpret_cast<const float2 *>(pa);
#define G4C_STEP(U, SLOT)                                                                  \
    {                                                                                      \
        const float2 an = (G4C_ABLATE & 64) ? a : *reinterpret_cast<const float2 *>(pa + (((U) + 1) & 7) * 4); \
        __builtin_amdgcn_sched_barrier(0);                                                 \
        if (G4C_SPLIT_PRIO) __builtin_amdgcn_s_setprio(1);                                 \
        _Pragma("unroll") for (int c = 0; c < NCT; ++c) {                                  \
            acc.t[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, bget(g.SLOT, 2 * c), acc.t[c], 0, 0, 0);     \
        }                                                                                  \
        _Pragma("unroll") for (int c = 0; c < NCT; ++c) {                                  \
            acc.t[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, bget(g.SLOT, 2 * c + 1), acc.t[c], 0, 0, 0); \
        }                                                                                  \
        if (G4C_SPLIT_PRIO) __builtin_amdgcn_s_setprio(0);                                 \
        if (!(G4C_ABLATE & 32) && !((G4C_ABLATE & 256) && ((U) & 1))) load_bn(g.SLOT, wnext + step_off(U), lo); \
        __builtin_amdgcn_sched_barrier(0);                                                 \
        a = an;                                                                            \
    }
    G4C_STEP(0, s0) G4C_STEP(1, s1) G4C_STEP(2, s2) G4C_STEP(3, s3)
    G4C_STEP(4, s4) G4C_STEP(5, s5) G4C_STEP(6, s6) G4C_STEP(7, s7)
#undef G4C_STEP
}

// LayerNorm / activation / store of a finished 32-row tile held in sH; rows split over the NW waves of the workgroup.
// Shared by the column-split kernels.  Needs: all waves' last-layer columns visible in sH (barrier done by the caller).
// PLAIN (the tile kernel's shaped instantiations, mlp_common.h TileShapeNode): LayerNorm present, 128 columns, fp32 rows stored by whole
// 16-byte groups to their own row numbers — no column masks, no output index / residual / bf16 form.
template <int NW, int ROWS = 32, bool PLAIN = false>
__device__ __forceinline__ void split_finish(const Params &p, float *sH, const float *sGB, int wave, int lane, long long row0,
                                             long long mlim = -1) {
    if (mlim < 0) mlim = p.M;          // rows >= mlim are not stored (mlim < p.M: tiles of whole segments)
    const int i = lane & 31, h = lane >> 5;
    // ---------------------------------------------------------------- LayerNorm / activation: rows split over the waves
    // wave w owns rows [w*RPW, (w+1)*RPW); lane = part * RPW + row_local, each part = NC consecutive columns
    constexpr int RPW = ROWS / NW, PARTS = 64 / RPW, NC = NP / PARTS;
    const int n_out = PLAIN ? NP : p.n_out;
    const int rloc = lane % RPW, part = lane / RPW;
    const int myrow = wave * RPW + rloc;
    const int cb = part * NC;
    if ((PLAIN || p.gamma || p.act) && !(G4C_ABLATE & 4)) {
        float *rowp = sH + myrow * HS + cb;
        const float inv_n = 1.0f / (float)n_out;
        float x[NC];
#pragma unroll
        for (int c = 0; c < NC; c += 4) {
            const f32x4 t = *reinterpret_cast<const f32x4 *>(rowp + c);
            x[c] = t[0]; x[c + 1] = t[1]; x[c + 2] = t[2]; x[c + 3] = t[3];
        }
        if (PLAIN || p.gamma) {
            float sum = 0.f;
#pragma unroll
            for (int c = 0; c < NC; ++c) sum += (cb + c < n_out) ? x[c] : 0.f;
#pragma unroll
            for (int o = RPW; o < 64; o <<= 1) sum += __shfl_xor(sum, o);
            const float mean = sum * inv_n;
            float var = 0.f;
#pragma unroll
            for (int c = 0; c < NC; ++c) { const float d = x[c] - mean; var += (cb + c < n_out) ? d * d : 0.f; }
#pragma unroll
            for (int o = RPW; o < 64; o <<= 1) var += __shfl_xor(var, o);
            const float rstd = rsqrtf(var * inv_n + p.eps);
#pragma unroll
            for (int c = 0; c < NC; c += 4) {
                f32x4 g4, b4;
                if (G4C_SPLIT_SLIM) {
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int cc = (cb + c + u < n_out) ? cb + c + u : 0;
                        g4[u] = p.gamma[cc]; b4[u] = p.beta[cc];
                    }
                } else {
                    g4 = *reinterpret_cast<const f32x4 *>(sGB + cb + c);
                    b4 = *reinterpret_cast<const f32x4 *>(sGB + NP + cb + c);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) x[c + u] = fmaf((x[c + u] - mean) * rstd, g4[u], b4[u]);
            }
        }
        if (p.act == G4C_ACT_SELU) {
#pragma unroll
            for (int c = 0; c < NC; ++c) x[c] = g4c::selu_f(x[c]);
        } else if (p.act == G4C_ACT_TANH) {
#pragma unroll
            for (int c = 0; c < NC; ++c) x[c] = g4c::tanh_f(x[c]);
        }
#pragma unroll
        for (int c = 0; c < NC; c += 4) {
            f32x4 t;
            t[0] = x[c]; t[1] = x[c + 1]; t[2] = x[c + 2]; t[3] = x[c + 3];
            *reinterpret_cast<f32x4 *>(rowp + c) = t;
        }
    }
    // (each wave reads back only the rows it normalised itself: no barrier needed)

    // ---------------------------------------------------------------- store this wave's rows
    if (!PLAIN && p.out == nullptr) return;          // (only the aggregate of the rows is wanted: g4c_mlp_io_t.agg with out == NULL)
    const bool fast = (n_out == NP) && ((p.out_ld & 3) == 0) && (((uintptr_t)p.out & 15) == 0) && (p.resid == nullptr);
    if (!PLAIN && p.out_bf16) {
        // rows kept in bf16 (the rounded-bf16 mode's message tensors: their consumer rounds them to bf16 anyway): 8 bytes per lane
        __bf16 *o16 = reinterpret_cast<__bf16 *>(p.out);
#pragma unroll
        for (int r = h; r < RPW; r += 2) {
            const int row = wave * RPW + r;
            const long long grow = row0 + row;
            if (grow < mlim) {
                f32x4 t = *reinterpret_cast<const f32x4 *>(sH + row * HS + 4 * i);
                if (p.out_bf16 == 2) t = selu4(t);          // (G4C_DTYPE_BF16_SELU: the reader's pending activation, applied before the one rounding)
                bf16x4 b;
#pragma unroll
                for (int u = 0; u < 4; ++u) b[u] = (__bf16)t[u];
                *reinterpret_cast<bf16x4 *>(o16 + grow * p.out_ld + 4 * i) = b;
            }
        }
    } else if (PLAIN) {
        // the tile's rows through a buffer descriptor of exactly the rows below mlim (base and extent scalar, a 32-bit lane offset):
        // a row past mlim falls outside it and the hardware drops the store — no 64-bit row address, no branch per row
        const int left = __builtin_amdgcn_readfirstlane((int)(mlim - row0 >= ROWS ? ROWS : (mlim - row0 > 0 ? mlim - row0 : 0)));
        const int ld = p.out_ld;
        float *const tb = p.out + (long long)__builtin_amdgcn_readfirstlane((int)row0) * ld;
        const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(tb, 0, left ? ((left - 1) * ld + NP) * 4 : 0, 0x00020000);
#pragma unroll
        for (int r = h; r < RPW; r += 2) {
            const int row = wave * RPW + r;
            const f32x4 t = *reinterpret_cast<const f32x4 *>(sH + row * HS + 4 * i);
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, t), ro, (unsigned)(row * ld + 4 * i) * 4u, 0, 0);
        }
    } else if (fast) {
#pragma unroll
        for (int r = h; r < RPW; r += 2) {
            const int row = wave * RPW + r;
            const long long grow = row0 + row;
            if (grow < mlim) {
                const long long orow = p.out_idx ? p.out_idx[grow] : grow;
                const f32x4 t = *reinterpret_cast<const f32x4 *>(sH + row * HS + 4 * i);
                *reinterpret_cast<f32x4 *>(p.out + orow * p.out_ld + 4 * i) = t;
            }
        }
    } else {
        for (int e = lane; e < RPW * n_out; e += 64) {
            const int r = e / n_out, c = e - r * n_out;
            const int row = wave * RPW + r;
            const long long grow = row0 + row;
            if (grow < mlim) {
                const long long orow = p.out_idx ? p.out_idx[grow] : grow;
                float y = sH[row * HS + c];
                if (p.resid) y += p.resid[grow * p.resid_ld + p.resid_col0 + c];
                p.out[orow * p.out_ld + c] = y;
            }
        }
    }
}

constexpr int G4C_SPLIT_B4 = 1;        // 16-byte weight ring slots (two steps per load)
// ring of four 16-byte slots, each holding this lane's B operands of TWO consecutive steps (NCT == 1)
struct Ring4 { f32x4 p0, p1, p2, p3; };
__device__ __forceinline__ void ring4_fill(Ring4 &g, const float *w, unsigned lo4) {
    g.p0 = *reinterpret_cast<const f32x4 *>(w + 0 * 1024 + lo4); g.p1 = *reinterpret_cast<const f32x4 *>(w + 1 * 1024 + lo4);
    g.p2 = *reinterpret_cast<const f32x4 *>(w + 2 * 1024 + lo4); g.p3 = *reinterpret_cast<const f32x4 *>(w + 3 * 1024 + lo4);
}
__device__ __forceinline__ void mma_chunk_4(const float *pa, Ring4 &g, const float *wnext, unsigned lo4, AccN<1> &acc) {
    float2 a = *reinterpret_cast<const float2 *>(pa);
#define G4C_PAIR(V, SLOT)                                                                             \
    {                                                                                                  \
        const float2 a1 = *reinterpret_cast<const float2 *>(pa + (2 * (V) + 1) * 4);                   \
        __builtin_amdgcn_sched_barrier(0);                                                             \
        acc.t[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, g.SLOT[0], acc.t[0], 0, 0, 0);            \
        acc.t[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, g.SLOT[1], acc.t[0], 0, 0, 0);            \
        const float2 a2 = *reinterpret_cast<const float2 *>(pa + ((2 * (V) + 2) & 7) * 4);             \
        __builtin_amdgcn_sched_barrier(0);                                                             \
        acc.t[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.x, g.SLOT[2], acc.t[0], 0, 0, 0);           \
        acc.t[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.y, g.SLOT[3], acc.t[0], 0, 0, 0);           \
        g.SLOT = *reinterpret_cast<const f32x4 *>(wnext + (V) * 1024 + lo4);                           \
        __builtin_amdgcn_sched_barrier(0);                                                             \
        a = a2;                                                                                        \
    }
    G4C_PAIR(0, p0) G4C_PAIR(1, p1) G4C_PAIR(2, p2) G4C_PAIR(3, p3)
#undef G4C_PAIR
}

constexpr int G4C_SPLIT_MINW = 1;
template <int NW, bool VEC>
__global__ __launch_bounds__(64 * NW, G4C_SPLIT_MINW) void mlp_split_kernel(const Params p) {
    constexpr int ROWS = 32, NCT = 4 / NW, NPIECE = 4 / NW;   // pieces (8 rows x 32 cols) of a chunk gathered per wave
    // LDS budget: 8 workgroups of NW = 4 waves per CU (= the 32-wave limit) need <= 20 KiB each, so the LayerNorm
    // parameters are read from global memory (L1/L2 hits) instead of being staged
    constexpr int GB_ROWS = G4C_SPLIT_SLIM ? 0 : 2;
    __shared__ __attribute__((aligned(16))) float lds[ROWS * HS + 2 * G4C_MAX_SRC * ROWS + (G4C_MAX_LAYERS + GB_ROWS) * NP];
    float *sH = lds;
    float *sX0 = lds;
    float *sX1 = lds + ROWS * XS;
    int *sRow = reinterpret_cast<int *>(lds + ROWS * HS);
    int *sRowAdd = sRow + G4C_MAX_SRC * ROWS;
    float *sBias = lds + ROWS * HS + 2 * G4C_MAX_SRC * ROWS;
    float *sGB = sBias + G4C_MAX_LAYERS * NP;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31, h = lane >> 5;
    const int ct0 = wave * NCT;

    int tile;
    {
        const int b = blockIdx.x, nt = p.n_tiles;
        const int q = nt >> 3, r = nt & 7, x = b & 7, j = b >> 3;
        tile = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + j;
    }
    const long long row0 = p.row_base + (long long)tile * ROWS;
    G4C_STAMPW(0);

    // row indices of every input block: one (block, row) per thread, so all index loads are in flight together
    for (int e = tid; e < 2 * G4C_MAX_SRC * ROWS; e += 64 * NW) {
        const int slot = e / ROWS, r = e % ROWS;
        long long gr = row0 + r;
        if (gr >= p.M) gr = p.M - 1;
        const int *ix = nullptr;
        bool used;
        if (slot < G4C_MAX_SRC) { used = slot < p.n_src; if (used) ix = p.src[slot].idx; }
        else { used = slot - G4C_MAX_SRC < p.n_add; if (used) ix = p.add[slot - G4C_MAX_SRC].idx; }
        if (used) sRow[e] = ix ? ix[gr] : (int)gr;      // sRowAdd == sRow + G4C_MAX_SRC * ROWS
    }
    for (int e = tid; e < p.n_layers * NP; e += 64 * NW) sBias[e] = p.b[e];
    if (p.gamma && !G4C_SPLIT_SLIM) {
        for (int e = tid; e < NP; e += 64 * NW) {
            const int ee = e < p.n_out ? e : 0;
            sGB[e] = p.gamma[ee];
            sGB[NP + e] = p.beta[ee];
        }
    }
    __syncthreads();
    G4C_STAMPW(1);

    AccN<NCT> acc;
    constexpr bool B4 = G4C_SPLIT_B4 && NCT == 1;
    RingN<NCT> ring;
    Ring4 ring4;
    const unsigned lo4 = (unsigned)(ct0 * 256 + lane * 4);
    const float *w = p.w;
    const unsigned lo = (unsigned)(ct0 * 256 + lane * 4);
#pragma unroll
    for (int c = 0; c < NCT; ++c)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc.t[c][q] = 0.f;
    // pre-multiplied node-side terms of the first layer: one source at a time, its 16*NCT loads issued together
    // (16 temporaries keep the kernel at 7 waves per SIMD; batching both sources at once costs occupancy and is slower)
    for (int a = 0; a < ((G4C_ABLATE & 8) ? 0 : p.n_add); ++a) {
        float t[16][NCT];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int row = (q & 3) + 8 * (q >> 2) + 4 * h;
            const float *pr = p.add[a].ptr + (long long)sRowAdd[a * ROWS + row] * p.add[a].ld;
#pragma unroll
            for (int c = 0; c < NCT; ++c) {
                const int col = (ct0 + c) * 32 + i;
                t[q][c] = pr[col < p.add[a].width ? col : 0];
            }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q < 16; ++q)
#pragma unroll
            for (int c = 0; c < NCT; ++c) acc.t[c][q] += ((ct0 + c) * 32 + i < p.add[a].width) ? t[q][c] : 0.f;
        __builtin_amdgcn_sched_barrier(0);
    }
    G4C_STAMPW(2);
    if constexpr (B4) {
        ring4_fill(ring4, w, lo4);
    } else {
        load_bn(ring.s0, w + step_off(0), lo); load_bn(ring.s1, w + step_off(1), lo);
        load_bn(ring.s2, w + step_off(2), lo); load_bn(ring.s3, w + step_off(3), lo);
        load_bn(ring.s4, w + step_off(4), lo); load_bn(ring.s5, w + step_off(5), lo);
        load_bn(ring.s6, w + step_off(6), lo); load_bn(ring.s7, w + step_off(7), lo);
    }
    __builtin_amdgcn_sched_barrier(0);

    // ---------------------------------------------------------------- layer 0: shared gather, one barrier per chunk
    {
        const int c4 = (lane & 7) * 4;
        f32x4 xp[NPIECE];
        const float *rp[NPIECE];
        int s = 0, k0 = 0;
        int cur_width = p.src[0].width, cur_wpad = p.src[0].wpad, cur_act = p.src[0].pre_act;
        auto set_rows = [&](int sidx) {
#pragma unroll
            for (int q = 0; q < NPIECE; ++q)
                rp[q] = p.src[sidx].ptr + (long long)sRow[sidx * ROWS + (lane >> 3) + 8 * (wave + NW * q)] * p.src[sidx].ld + p.src[sidx].col0;
        };
        auto gather = [&](int kk) {
            const int c = kk + c4;
#pragma unroll
            for (int q = 0; q < NPIECE; ++q) {
                if (VEC) {
                    xp[q] = *reinterpret_cast<const f32x4 *>(rp[q] + (c < cur_width ? c : 0));
                } else {
                    const int w1 = cur_width - 1;
                    xp[q][0] = rp[q][c + 0 < w1 ? c + 0 : w1]; xp[q][1] = rp[q][c + 1 < w1 ? c + 1 : w1];
                    xp[q][2] = rp[q][c + 2 < w1 ? c + 2 : w1]; xp[q][3] = rp[q][c + 3 < w1 ? c + 3 : w1];
                }
            }
        };
        auto park = [&](float *dst, int kk) {
            const int c = kk + c4;
#pragma unroll
            for (int q = 0; q < NPIECE; ++q) {
                float t[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) t[e] = (c + e < cur_width) ? xp[q][e] : 0.f;
                if (cur_act) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) t[e] = g4c::selu_f(t[e]);
                }
                float *d = dst + ((lane >> 3) + 8 * (wave + NW * q)) * XS + c4;
                *reinterpret_cast<float2 *>(d) = make_float2(t[0], t[1]);
                *reinterpret_cast<float2 *>(d + 2) = make_float2(t[2], t[3]);
            }
        };
        set_rows(0);
        gather(0);
        park(sX0, 0);
        __syncthreads();
        G4C_STAMPW(3);
        for (int c = 0; c < p.chunks0; ++c) {
            int nk0 = k0 + KC;
            if (nk0 >= cur_wpad) {
                if (s + 1 < p.n_src) {
                    ++s; nk0 = 0;
                    cur_width = p.src[s].width; cur_wpad = p.src[s].wpad; cur_act = p.src[s].pre_act;
                    set_rows(s);
                } else {
                    nk0 = k0;
                }
            }
            if (!(G4C_ABLATE & 2)) gather(nk0);
            __builtin_amdgcn_sched_barrier(0);
            w += CHUNK_FLOATS;
            if constexpr (B4) mma_chunk_4(((c & 1) ? sX1 : sX0) + i * XS + 2 * h, ring4, w, lo4, acc);
            else mma_chunk_n<NCT>(((c & 1) ? sX1 : sX0) + i * XS + 2 * h, ring, w, lo, acc);
            if (!(G4C_ABLATE & 2)) park((c & 1) ? sX0 : sX1, nk0);
            k0 = nk0;
            if (!(G4C_ABLATE & 16)) __syncthreads();
        }
    }

    G4C_STAMPW(4);
    // ---------------------------------------------------------------- layers 1..L-1
    for (int l = 0;; ++l) {
        const bool last = (l == p.n_layers - 1);
        {   // this wave's column tiles of the layer output -> shared hidden buffer
            float *base = sH + (4 * h) * HS + i;
#pragma unroll
            for (int c = 0; c < NCT; ++c) {
                const float bv = sBias[l * NP + (ct0 + c) * 32 + i];
#pragma unroll
                for (int q0 = 0; q0 < 16; q0 += 4) {   // 4 at a time: more temporaries cost a wave of occupancy
                    float x[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q) x[q] = acc.t[c][q0 + q] + bv;
                    if (!last && !(G4C_ABLATE & 4)) {   // uniform branch per group, not per element
#pragma unroll
                        for (int q = 0; q < 4; ++q) x[q] = g4c::selu_f(x[q]);
                    }
#pragma unroll
                    for (int q = 0; q < 4; ++q) base[(q + 2 * q0) * HS + (ct0 + c) * 32] = x[q];
                }
            }
        }
        __syncthreads();
        G4C_STAMPW(5 + 2 * l);
        if (last) break;
#pragma unroll
        for (int c = 0; c < NCT; ++c)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc.t[c][q] = 0.f;
#pragma unroll 1
        for (int k0 = 0; k0 < NP; k0 += KC) {
            w += CHUNK_FLOATS;
            if constexpr (B4) mma_chunk_4(sH + i * HS + k0 + 2 * h, ring4, w, lo4, acc);
            else mma_chunk_n<NCT>(sH + i * HS + k0 + 2 * h, ring, w, lo, acc);
        }
        __syncthreads();   // everybody is done reading sH before the next layer's output overwrites it
        G4C_STAMPW(6 + 2 * l);
    }

    G4C_STAMPW(12);
    split_finish<NW>(p, sH, sGB, wave, lane, row0);
    G4C_STAMPW(13);
    if (p.n_heads) {
        __syncthreads();                   // every wave's rows of the final tile are in sH
        for (int hd = 0; hd < p.n_heads; ++hd) {
#pragma unroll
            for (int c = 0; c < NCT; ++c)
#pragma unroll
                for (int q = 0; q < 16; ++q) acc.t[c][q] = 0.f;
#pragma unroll 1
            for (int k0 = 0; k0 < NP; k0 += KC) {
                w += CHUNK_FLOATS;
                if constexpr (B4) mma_chunk_4(sH + i * HS + k0 + 2 * h, ring4, w, lo4, acc);
                else mma_chunk_n<NCT>(sH + i * HS + k0 + 2 * h, ring, w, lo, acc);
            }
            float *ho = p.head_out[hd];
#pragma unroll
            for (int c = 0; c < NCT; ++c)
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const long long grow = row0 + (q & 3) + 8 * (q >> 2) + 4 * h;
                    if (grow < p.M) ho[grow * p.head_ld + (ct0 + c) * 32 + i] = acc.t[c][q];
                }
        }
    }
}

// W[n_out, k_in] (nn.Linear layout) -> this layer's chunks of the packed stream:
// chunk c = k/32 (4096 floats), step U = (k%32)/4, step pair V = U/2 (1024 floats), then
// [ct = n/32][lane = ((k%4)/2)*32 + n%32][u = U%2][e = k%2]:
// packed[c*4096 + V*1024 + ct*256 + lane*4 + u*2 + e] = W^T[k][n], zero padded to k_pad x 128,
// with an optional per-block sign flip.  seg tables live in the kernel argument.
struct PackSegs {
    int n_seg;
    int width[G4C_MAX_SRC], wpad[G4C_MAX_SRC], neg[G4C_MAX_SRC];
};

__global__ void pack_layer_kernel(const float *__restrict__ W, int n_out, int k_in, PackSegs segs,
                                  float *__restrict__ packed, int k_pad) {
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= k_pad * NP) return;
    const int kp = gid / NP, n = gid % NP;
    int k = -1, base_p = 0, base = 0, neg = 0;
    for (int s = 0; s < segs.n_seg; ++s) {
        if (kp >= base_p && kp < base_p + segs.wpad[s]) {
            const int j = kp - base_p;
            if (j < segs.width[s]) { k = base + j; neg = segs.neg[s]; }
        }
        base_p += segs.wpad[s];
        base += segs.width[s];
    }
    float v = 0.f;
    if (k >= 0 && n < n_out) v = W[(long long)n * k_in + k];
    if (neg) v = -v;
    const int U = (kp & 31) >> 2;
    packed[(long long)(kp >> 5) * CHUNK_FLOATS + (U >> 1) * 1024 + (n >> 5) * 256 + (((kp >> 1) & 1) * 32 + (n & 31)) * 4 + (U & 1) * 2 + (kp & 1)] = v;
}


// ======================================================================================================
// fp32-accurate MLP on the bf16 matrix pipe ("bf16x6", opt-in: G4C_WFMT_BF16X3).  Every fp32 operand is split
// EXACTLY into three bf16 terms x = h + m + l (8 + 8 + 8 significand bits); of the nine partial products the six
// largest are formed (hh, hm, mh, mm, hl, lh — each exact in fp32) and accumulated in fp32 by
// v_mfma_f32_32x32x16_bf16.  The dropped terms (ml, lm, ll) are <= 2^-23 relative: the same order as ONE fp32 rounding,
// so the result is as accurate as the fp32-MFMA kernel (tests compare both against fp64), at 6 x 32 = 192 MFMA cycles
// per 16 k instead of 8 x 64 = 512.  A whole 128-k block is staged per barrier pair; weights are split at pack time
// (g4c_mlp_pack_layer: [128-k block][column tile][16-k step][plane][lane][8], 6 bytes per weight).
// Template parameter SP = 3: the above.  SP = 1: only the leading terms (operands ROUNDED to bf16, one product) — the
// opt-in "bf16" mode of BASELINE config 3 ("bf16 edge-MLP MFMA", ~1e-2 deviation) on the same stream and structure.
// weight ring depth in 16-k steps.  2 where the launch fills the chip (4 / 8 measured slower: 483 / 563 us against 446 on the level-1
// launch — registers, i.e. waves per SIMD, are what hides the L2 latency there).  8 (a whole 128-k block in flight: the NEXT block's
// weights are requested while this block multiplies) for SMALL launches, <= g_bx6_deep_tiles tiles: with one wave per SIMD nothing else
// covers the L2 round trip, and a ring of 2 exposes it four times per block (2 800 cycles per block against 770 of MFMAs;
// scripts/small_launch_stamps.py)
template <int RD6> struct Ring6 { bf16x8 h[RD6], m[RD6], l[RD6]; };

// one 128-k block for RT row tiles of 32: per 16-k step and row tile 6 MFMAs from the three LDS planes (plane stride
// `plane`, row-tile stride 32*HB); the weight fragments of a step are shared by the row tiles; ring slot s % RD6 is
// refilled RD6 steps ahead.  A fragments are double-buffered per (step, row tile) item: the next item's three
// ds_read_b128 are issued before this item's MFMAs.

constexpr int G4C_BX6_TUNE = 0;      // (1 = s_setprio around the MFMAs, 2 = no sched_barriers in the MFMA loop: both measured neutral)
// SP == 2 (two-way fp16 split, mlp_common.h): planes h / l, three products per step — (Wh, xl) and (Wl, xh) into acc1 (the terms
// that carry the factor 2^-11), (Wh, xh) into acc.
// SWAP (the heads): the two MFMA operands trade places, so the accumulator comes out untransposed — a lane holds ONE output feature
// (lane & 31 of the wave's 32-column slice) of the 16 sample rows 8 (q / 4) + 4 (lane / 32) + q % 4 — and a store instruction writes
// 128 contiguous bytes of each of two rows (same products, same order of k inside the MFMA).
// ZC (SP == 2): accumulation chains that START at zero in this block — bit 0: acc1, bit 1: acc.  Their first MFMA takes a zero C operand (an
// inline constant; 0 + x is exact) instead of reading registers the caller had to clear with 16 moves each; the caller passes them
// uninitialised.  The first group of steps is peeled off the rolled loop for it.
template <int RT, int SP, bool SWAP = false, int RD6 = 2, int ZC = 0>
__device__ __forceinline__ void mma_block_bx6(const __bf16 *pa, int plane, Ring6<RD6> &g, __amdgpu_buffer_rsrc_t rs, unsigned wofs, unsigned lo_b,
                                              f32x16 (&acc)[RT], f32x16 (&acc1)[RT]) {
    bf16x8 ah = *reinterpret_cast<const bf16x8 *>(pa), am = ah, al = ah;
    if (SP >= 2) am = *reinterpret_cast<const bf16x8 *>(pa + plane);
    if (SP == 3) al = *reinterpret_cast<const bf16x8 *>(pa + 2 * plane);
    // ROLLED over groups of RD6 steps (ring slots are compile-time inside a group): unrolling all 8 steps lets hipcc give
    // every refill fresh registers, which costs a wave of occupancy
    static_assert(ZC == 0 || SP == 2, "zero-start chains: the f16x3 products");
    unsigned so = wofs + 2u * RD6 * STEP6;          // byte offset of the step that refills slot 0 (RD6 steps ahead)
    const f32x16 zero16 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    auto group = [&](const int j, auto first_tag) __attribute__((always_inline)) {
        constexpr bool FIRST = decltype(first_tag)::value;          // the peeled first group of a block with zero-start chains
        const __bf16 *pj = pa + j * RD6 * 16;
        if (j == 8 / RD6 - 1) so = wofs + 2u * BLOCK6;      // the last group refills from the NEXT block's first steps
#pragma unroll
        for (int r = 0; r < RD6; ++r) {
#pragma unroll
            for (int t = 0; t < RT; ++t) {
                // next (row tile, step) item; after the last step of the block the prefetch wraps to step 0 (unused values)
                const int nt = (t + 1) % RT, nr = (t + 1 == RT) ? r + 1 : r;
                const __bf16 *pn = ((nr == RD6 && j == 8 / RD6 - 1) ? pa : pj + nr * 16) + nt * 32 * HB;
                const bf16x8 nh = (G4C_ABLATE & 64) ? ah : *reinterpret_cast<const bf16x8 *>(pn),
                             nm = (SP == 1 || (G4C_ABLATE & 64)) ? am : *reinterpret_cast<const bf16x8 *>(pn + plane),
                             nl = (SP != 3 || (G4C_ABLATE & 64)) ? al : *reinterpret_cast<const bf16x8 *>(pn + 2 * plane);
                if (!(G4C_BX6_TUNE & 2)) __builtin_amdgcn_sched_barrier(0);
                if (G4C_BX6_TUNE & 1) __builtin_amdgcn_s_setprio(1);
                if (SP == 3 && !(G4C_ABLATE & 128)) {
                if (SWAP) {
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, g.h[r], acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, g.l[r], acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, g.m[r], acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(am, g.h[r], acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, g.m[r], acc[t], 0, 0, 0);
                } else {
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(g.h[r], al, acc[t], 0, 0, 0);     // small terms first
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(g.l[r], ah, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(g.m[r], am, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(g.h[r], am, acc[t], 0, 0, 0);
                acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(g.m[r], ah, acc[t], 0, 0, 0);
                }
                } else if (SP == 3) {      // (ablation) keep every operand live with one cheap VALU op instead of five MFMAs
                    acc[t][0] += (float)al[0] + (float)am[0] + (float)g.l[r][0] + (float)g.m[r][0];
                }
                if (SP == 2) {
                    const bool z1 = FIRST && r == 0 && (ZC & 1), z0 = FIRST && r == 0 && (ZC & 2);
                    if (SWAP) {
                        acc1[t] = mfma_f16(am, g.h[r], z1 ? zero16 : acc1[t]);
                        acc1[t] = mfma_f16(ah, g.m[r], acc1[t]);
                        acc[t] = mfma_f16(ah, g.h[r], z0 ? zero16 : acc[t]);
                    } else {
                        acc1[t] = mfma_f16(g.h[r], am, z1 ? zero16 : acc1[t]);
                        acc1[t] = mfma_f16(g.m[r], ah, acc1[t]);
                        acc[t] = mfma_f16(g.h[r], ah, z0 ? zero16 : acc[t]);
                    }
                } else
                acc[t] = SWAP ? __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, g.h[r], acc[t], 0, 0, 0) : __builtin_amdgcn_mfma_f32_32x32x16_bf16(g.h[r], ah, acc[t], 0, 0, 0);
                if (G4C_BX6_TUNE & 1) __builtin_amdgcn_s_setprio(0);
                if (t + 1 == RT && !(G4C_ABLATE & 32)) {
                    const unsigned sx = (G4C_ABLATE & 1024) ? 0u : so + 2u * r * STEP6;     // (1024: always the same 3 KB -> L1 hits)
                    g.h[r] = ldw(rs, lo_b, sx);
                    if (SP >= 2) g.m[r] = ldw(rs, lo_b + 1024u, sx);
                    if (SP == 3) g.l[r] = ldw(rs, lo_b + 2048u, sx);
                }
                if (!(G4C_BX6_TUNE & 2)) __builtin_amdgcn_sched_barrier(0);
                ah = nh; am = nm; al = nl;
            }
        }
        so += 2u * RD6 * STEP6;
    };
    if constexpr (ZC != 0) {
        group(0, std::true_type{});
#pragma unroll 1
        for (int j = 1; j < 8 / RD6; ++j) group(j, std::false_type{});
    } else {
#pragma unroll 1
        for (int j = 0; j < 8 / RD6; ++j) group(j, std::false_type{});
    }
}


constexpr int G4C_SEG_CHUNKS = 1;
constexpr int G4C_SEG_INFLIGHT = 6;     // rows of a segment in flight per column chunk when a source is aggregated on load
constexpr int G4C_BX6_MINW = 4;         // workgroups per CU the instantiations are register-limited for (launch_bounds)
constexpr int G4C_F16_MINW = 4;
constexpr int G4C_RT2_MINW = 3;         // ... of the 64-row shaped instantiations: 192 rows in flight per CU
// RT = 1: 32-row tile.  RT = 2: 64-row tile — every weight fragment feeds two row tiles (half the L2 -> register weight
// traffic per row, which is what this kernel stalls on) and every memory round trip of the tile's critical path serves
// twice the rows.
// FULL: every weighted input block and every additive block is exactly 128 wide and 16-byte aligned (the MP layers):
// no column masks anywhere.
// TRACK (SP = 2): the fp16 range tracker (mlp_common.h RangeS); false for a launch whose caller certifies that nothing it converts can
// reach the end of the range (Params::range_certified): three vector instructions per four converted values less, no flag word written.
// SH: the launch shape (mlp_common.h TileShapeGeneric / TileShapeNode).  A shaped instantiation (SH::ID != 0) reads no field of Params
// that its shape fixes: no aggregation-on-load path, no index staging, constant trip counts over sources / layers / heads, only its own
// layers' biases staged, and the input rows loaded through a per-tile buffer descriptor with a 32-bit lane offset (rows of the last
// tile past M come back as zeros from the descriptor's range check instead of being clamped; they are never stored).  Same
// arithmetic in the same order: bit-identical to the generic instantiation.
// The training forms' rows as bf16, four columns of one thread — the plain rounded-bf16 stream (SP == 1) only, selected by the
// wave-uniform Params.save_bf16 / mul_bf16, which only the SAVE instantiations read; the SP = 2 / 3 instantiations keep fp32 rows (the
// launcher refuses bf16 for them).  save: each value rounded once to bf16 (nearest even, v_cvt_pk_bf16_f32), one 8-byte store (save_ld
// in elements, a multiple of 4, the base 16-byte aligned).  mul: an 8-byte load, widened exactly.
__device__ __forceinline__ void save_row4_bf16(const Params &p, int l, long long gr, int col, f32x4 x) {
    bf16x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (__bf16)x[e];
    *reinterpret_cast<bf16x4 *>(reinterpret_cast<__bf16 *>(p.save[l]) + gr * p.save_ld + col) = v;
}
__device__ __forceinline__ f32x4 mul_row4_bf16(const Params &p, int l, long long gr, int col) {
    const bf16x4 v = *reinterpret_cast<const bf16x4 *>(reinterpret_cast<const __bf16 *>(p.mul[l]) + gr * p.mul_ld + col);
    f32x4 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = (float)v[e];
    return r;
}

// Workgroups per CU the registers of an instantiation are bounded for: two on the deep ring, three for 64-row tiles (168 registers), else
// four (128)
template <int RT, bool VEC, bool FULL, int SP, bool SAVE = false, int RD6 = 2, bool TRACK = true, class SH = TileShapeGeneric>
__global__ __launch_bounds__(256, RD6 > 2 ? 2 : (RT == 2 ? G4C_RT2_MINW : (SP == 2 ? G4C_F16_MINW : G4C_BX6_MINW))) void mlp_bx6_kernel(const Params p) {
    static_assert(TRACK || (SP == 2 && !SAVE), "the tracker-free instantiations: f16x3 stream, inference");
    constexpr bool SHAPED = SH::ID != G4C_TILE_SHAPE_GENERIC;
    static_assert(!SHAPED || (VEC && FULL && SP == 2 && !SAVE && RD6 == 2), "launch shapes: the chip-filling f16x3 inference form");
    static_assert(RT == 1 || (RT == 2 && SHAPED),
                  "64-row tiles (RT = 2): the shaped f16x3 inference instantiations only (three workgroups per CU at no more than 168 registers).  Everywhere "
                  "else they measured slower (split streams, round 3: 480 against 446 us, at 203 registers; rounded-bf16 mode, round 6, "
                  "500k-row edge update with heads: 288 against 255 us) and cannot take the fused aggregation: not instantiated");
    constexpr int ROWS = 32 * RT, NW = 4;
    constexpr int PLN = ROWS * HB;              // one bf16 operand plane [ROWS][136]
    // three operand planes; the fp32 final tile [ROWS][132] aliases them
    constexpr int BUF_FLOATS = (SP == 2 ? 2 : 3) * PLN / 2;      // (SP == 2: two planes; [ROWS][132] floats still fit in [2][ROWS][136] halves)
    static_assert(BUF_FLOATS >= ROWS * HS, "final tile must fit");
    // RT = 2 keeps three workgroups per CU (<= 53 KB of LDS each): two index slots per kind (a shape has at most one indexed source).
    // (Two f16x3 planes of 64 rows leave room for the biases' LDS copy: 38 KB in all.  LDS_BIAS false — biases from global memory — is
    // the form three planes would need.)
    constexpr int NSLOT = RT == 2 ? 2 : G4C_MAX_SRC;
    constexpr bool LDS_BIAS = RT == 1 || SP == 2;
    constexpr int BIAS_FLOATS = LDS_BIAS ? G4C_MAX_LAYERS * NP : 0;
    // SMALL (the deep-ring instantiation of launches of few tiles: one or two workgroups per CU, LDS to spare): the fp32 final tile
    // has its own buffer instead of aliasing the planes — one barrier less in front of the heads — and both heads' MFMA blocks run
    // back to back on separate accumulators, all head stores behind them
    constexpr bool SMALL = RD6 > 2;
    constexpr int FIN_FLOATS = SMALL ? ROWS * HS : 0;
    __shared__ __attribute__((aligned(16))) float lds[BUF_FLOATS + 2 * NSLOT * ROWS + BIAS_FLOATS + 2 * NP + FIN_FLOATS];
    float *sH = SMALL ? lds + BUF_FLOATS + 2 * NSLOT * ROWS + BIAS_FLOATS + 2 * NP : lds;
    __bf16 *sB = reinterpret_cast<__bf16 *>(lds);
    int *sRow = reinterpret_cast<int *>(lds + BUF_FLOATS);
    int *sRowAdd = sRow + NSLOT * ROWS;
    float *sBias = lds + BUF_FLOATS + 2 * NSLOT * ROWS;
    float *sGB = sBias + BIAS_FLOATS;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 31, h = lane >> 5;
    const int ct0 = wave;
    if (SP == 2) f16_range_mode();
    typename std::conditional<TRACK, RangeS, RangeNone>::type rng;          // lanes that converted a value beyond the fp16 range (SP == 2: mlp_common.h range_track)

    int tile;
    {
        const int b = blockIdx.x, nt = p.n_tiles;
        const int q = nt >> 3, r = nt & 7, x = b & 7, j = b >> 3;
        tile = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + j;
    }
    // (wave-uniform 32-bit values in scalar registers — the launcher checks n_rows < 2^31: as 64-bit per-lane values they were the
    // registers the SP == 2 instantiations spilled, and a spilled uniform costs 64 lanes of scratch traffic per wave)
    int row0 = __builtin_amdgcn_readfirstlane((int)(p.row_base + (long long)tile * ROWS)), mlim = __builtin_amdgcn_readfirstlane((int)p.M);
    if constexpr (!SHAPED) {
        if (p.tile_rows) {      // tile of whole segments (<= ROWS rows)
            row0 = __builtin_amdgcn_readfirstlane(p.tile_rows[tile]); mlim = __builtin_amdgcn_readfirstlane(p.tile_rows[tile + 1]);
        }
    }
    G4C_STAMPW(0);

    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(p.w), 0, 0x7fffffff, 0x00020000);
    const unsigned lo_b = 2u * (unsigned)(ct0 * 8 * STEP6 + lane * 8);    // this lane's byte offset inside a block of the stream
    unsigned wofs = 0;                                                     // byte offset of the current block (wave-uniform)
    Ring6<RD6> ring;

    // this wave's rows of an input block: lane -> row (lane>>3) + 8*wave (+ 32 per row tile), 4 floats at column
    // 4*(lane&7) of each 32-k chunk.  A block whose rows are not gathered through an index can start right away.
    const int grow_l = (lane >> 3) + 8 * wave, c4 = (lane & 7) * 4;
    f32x4 xp[RT][4];
    // (shaped: rows of this tile present in the launch — the record count of the tile's row descriptors)
    const int trows = SHAPED ? __builtin_amdgcn_readfirstlane(mlim - row0 >= ROWS ? ROWS : (mlim - row0 > 0 ? mlim - row0 : 0)) : 0;
    auto gather = [&](int sidx, bool direct) __attribute__((always_inline)) {
        if constexpr (SHAPED) if (direct || !SH::IDX0) {
            // the tile's rows of a direct 128-wide fp32 source through a buffer descriptor of exactly those rows (base and extent are
            // scalar; one 32-bit lane offset per source instead of a 64-bit address and a row clamp per load).  (A shape's indexed
            // source — `direct` false where the shape has one — goes on below: its extent is not part of the launch.)
            const int ld = p.src[sidx].ld;
            const float *tb = p.src[sidx].ptr + p.src[sidx].col0 + (long long)row0 * ld;
            const __amdgpu_buffer_rsrc_t rx = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(tb), 0, trows ? ((trows - 1) * ld + NP) * 4 : 0, 0x00020000);
#pragma unroll
            for (int t = 0; t < RT; ++t) {
                const unsigned vo = (unsigned)((grow_l + 32 * t) * ld + c4) * 4u;
#pragma unroll
                for (int q = 0; q < 4; ++q) xp[t][q] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rx, vo + q * KC * 4u, 0, 0));
            }
            return;
        }
        const int width = p.src[sidx].width;
        if (!SHAPED && p.src[sidx].seg_off) {
            // aggregation on load: this lane's row is the sum / mean of a CSR segment of the source's rows, added in
            // order (bit-identical to segment_reduce_kernel); four rows in flight per column chunk
            const int *so = p.src[sidx].seg_off, *sp = p.src[sidx].seg_perm;
            const int ld = p.src[sidx].ld, sact = p.src[sidx].pre_act;
#pragma unroll
            for (int t = 0; t < RT; ++t) {
                long long gr = row0 + grow_l + 32 * t;
                if (gr >= mlim) gr = mlim - 1;
                const int b = so[gr], e = so[gr + 1];
                const float *rp = p.src[sidx].ptr + p.src[sidx].col0 + c4;
                // G4C_SEG_CHUNKS 32-column chunks at a time, G4C_SEG_INFLIGHT rows of each in flight (bounded registers; the
                // row order of the additions is the segment order whichever way the loads are batched)
#pragma unroll
                for (int q0 = 0; q0 < 4; q0 += G4C_SEG_CHUNKS) {
                    f32x4 a[G4C_SEG_CHUNKS];
#pragma unroll
                    for (int qq = 0; qq < G4C_SEG_CHUNKS; ++qq) a[qq] = f32x4{0.f, 0.f, 0.f, 0.f};
                    for (int r = b; r < e; r += G4C_SEG_INFLIGHT) {
                        f32x4 v[G4C_SEG_INFLIGHT][G4C_SEG_CHUNKS];
#pragma unroll
                        for (int u = 0; u < G4C_SEG_INFLIGHT; ++u) {
                            int rr = (r + u < e) ? r + u : e - 1;
                            if (sp) rr = sp[rr];
#pragma unroll
                            for (int qq = 0; qq < G4C_SEG_CHUNKS; ++qq)
                                v[u][qq] = *reinterpret_cast<const f32x4 *>(rp + (long long)rr * ld + (q0 + qq) * KC);
                        }
                        if (sact) {          // the pending activation of the stored rows applies BEFORE the reduction
#pragma unroll
                            for (int u = 0; u < G4C_SEG_INFLIGHT; ++u)
#pragma unroll
                                for (int qq = 0; qq < G4C_SEG_CHUNKS; ++qq) v[u][qq] = selu4(v[u][qq]);
                        }
#pragma unroll
                        for (int u = 0; u < G4C_SEG_INFLIGHT; ++u) {
                            const bool on = r + u < e;
#pragma unroll
                            for (int qq = 0; qq < G4C_SEG_CHUNKS; ++qq)
#pragma unroll
                                for (int el = 0; el < 4; ++el) a[qq][el] += on ? v[u][qq][el] : 0.f;
                        }
                    }
#pragma unroll
                    for (int qq = 0; qq < G4C_SEG_CHUNKS; ++qq) xp[t][q0 + qq] = a[qq];
                }
                if (p.src[sidx].seg_mean) {
                    const float cnt = (float)((e - b) > 1 ? (e - b) : 1);
#pragma unroll
                    for (int q = 0; q < 4; ++q)
#pragma unroll
                        for (int el = 0; el < 4; ++el) xp[t][q][el] /= cnt;
                }
            }
            return;
        }
#pragma unroll
        for (int t = 0; t < RT; ++t) {
            long long gr;
            if (direct) { gr = row0 + grow_l + 32 * t; if (gr >= mlim) gr = mlim - 1; }
            else gr = sRow[sidx * ROWS + grow_l + 32 * t];
            const float *rp = p.src[sidx].ptr + gr * p.src[sidx].ld + p.src[sidx].col0;
            if (SP == 1 && p.src[sidx].bf16) {        // bf16 rows (128 wide, 8-byte aligned: the launcher checks): widen by a shift / a mask
                const __bf16 *rp16 = reinterpret_cast<const __bf16 *>(p.src[sidx].ptr) + gr * p.src[sidx].ld + p.src[sidx].col0;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
                    const u32x2 w = *reinterpret_cast<const u32x2 *>(rp16 + q * KC + c4);
                    xp[t][q][0] = __builtin_bit_cast(float, w[0] << 16); xp[t][q][1] = __builtin_bit_cast(float, w[0] & 0xffff0000u);
                    xp[t][q][2] = __builtin_bit_cast(float, w[1] << 16); xp[t][q][3] = __builtin_bit_cast(float, w[1] & 0xffff0000u);
                }
            } else
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int c = q * KC + c4;
                if (FULL) {
                    xp[t][q] = *reinterpret_cast<const f32x4 *>(rp + c);
                } else if (VEC) {
                    xp[t][q] = *reinterpret_cast<const f32x4 *>(rp + (c < width ? c : 0));
                } else {
                    const int w1 = width - 1;
                    xp[t][q][0] = rp[c + 0 < w1 ? c + 0 : w1]; xp[t][q][1] = rp[c + 1 < w1 ? c + 1 : w1];
                    xp[t][q][2] = rp[c + 2 < w1 ? c + 2 : w1]; xp[t][q][3] = rp[c + 3 < w1 ? c + 3 : w1];
                }
            }
        }
    };
    auto park_impl = [&](int sidx, auto act_tag) __attribute__((always_inline)) {
        constexpr bool ACT = decltype(act_tag)::value;
        const int width = p.src[sidx].width;
#pragma unroll
        for (int t = 0; t < RT; ++t) {
            __bf16 *d = sB + (grow_l + 32 * t) * HB + c4;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int c = q * KC + c4;
                f32x4 v = xp[t][q];
                if (!FULL) {
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = (c + e < width) ? v[e] : 0.f;
                }
                if (ACT) v = selu4(v);
                bf16x4 vh, vm, vl;
                split3x4<SP>(v, vh, vm, vl, rng);
                *reinterpret_cast<bf16x4 *>(d + q * KC) = vh;
                if (SP >= 2) *reinterpret_cast<bf16x4 *>(d + PLN + q * KC) = vm;
                if (SP == 3) *reinterpret_cast<bf16x4 *>(d + 2 * PLN + q * KC) = vl;
                __builtin_amdgcn_sched_barrier(0);      // one group of four at a time: bounds the live temporaries
            }
        }
    };
    auto park = [&](int sidx) __attribute__((always_inline)) {            // one uniform branch per block, not one per element
        if constexpr (SHAPED) park_impl(sidx, std::false_type{});
        else
        if (p.src[sidx].pre_act && !p.src[sidx].seg_off) park_impl(sidx, std::true_type{});
        else park_impl(sidx, std::false_type{});
    };
    // Memory instructions return in order per wave, so the loads that head a dependent chain go FIRST: row indices (the
    // additive gathers wait for them), then the parameters, then the long-latency streams (weights, directly indexed input).
    // (a shape without indexed sources stages none: no loads, no select chains, no sRow read-backs)
    int idx_v[(2 * NSLOT * ROWS + 64 * NW - 1) / (64 * NW)];
    if constexpr (SHAPED) {
        if constexpr (SH::IDX0) {          // slot 0 only: ROWS entries, one thread each
            const int gr = row0 + tid < mlim ? row0 + tid : mlim - 1;
            idx_v[0] = tid < ROWS ? p.src[0].idx[gr] : 0;
        }
    } else
#pragma unroll
    for (int it = 0; it < (2 * NSLOT * ROWS + 64 * NW - 1) / (64 * NW); ++it) {
        const int e = tid + it * 64 * NW;
        const int slot = e / ROWS, r = e % ROWS;
        long long gr = row0 + r;
        if (gr >= mlim) gr = mlim - 1;
        // selects among the (uniform) index pointers: p.src[slot] with the per-lane slot would be a load from the kernel argument
        // segment — one more dependent round trip in front of every tile's index loads
        const int *ix = nullptr;
#pragma unroll
        for (int s2 = 0; s2 < NSLOT; ++s2) {
            const int *is = s2 < p.n_src ? p.src[s2].idx : nullptr, *ia = s2 < p.n_add ? p.add[s2].idx : nullptr;
            ix = slot == s2 ? is : (slot == NSLOT + s2 ? ia : ix);
        }
        idx_v[it] = ix ? ix[gr] : (int)gr;
    }
    const int n_layers = [&] { if constexpr (SHAPED) return SH::N_LAYERS; else return p.n_layers; }();
    const int n_out = SHAPED ? NP : p.n_out;
    const bool has_ln = SHAPED || p.gamma;
    constexpr int BIAS_IT = ([] { if constexpr (SHAPED) return SH::N_LAYERS; else return G4C_MAX_LAYERS; }() * NP + 64 * NW - 1) / (64 * NW);
    float bias_v[BIAS_IT], gb_v = 0.f;          // (shaped: only the shape's own layers)
#pragma unroll
    for (int it = 0; it < BIAS_IT; ++it) {
        const int e = tid + it * 64 * NW;
        bias_v[it] = LDS_BIAS ? p.b[e < n_layers * NP ? e : 0] : 0.f;
    }
    if (has_ln) {
        const int e = tid & (NP - 1);
        const int ee = e < n_out ? e : 0;
        gb_v = tid < NP ? p.gamma[ee] : p.beta[ee];
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int s = 0; s < RD6; ++s) {
        ring.h[s] = ldw(rs, lo_b, 2u * s * STEP6);
        if (SP >= 2) ring.m[s] = ldw(rs, lo_b + 1024u, 2u * s * STEP6);
        if (SP == 3) ring.l[s] = ldw(rs, lo_b + 2048u, 2u * s * STEP6);
    }
    const bool direct0 = [&] { if constexpr (SHAPED) return !SH::IDX0; else return p.n_src > 0 && (p.src[0].idx == nullptr); }();
    if (direct0) gather(0, true);
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (SHAPED) {
        if constexpr (SH::IDX0) { if (tid < ROWS) sRow[tid] = idx_v[0]; }
    } else
#pragma unroll
    for (int it = 0; it < (2 * NSLOT * ROWS + 64 * NW - 1) / (64 * NW); ++it) {
        const int e = tid + it * 64 * NW;
        if (e < 2 * NSLOT * ROWS) sRow[e] = idx_v[it];
    }
    if (LDS_BIAS) {
#pragma unroll
        for (int it = 0; it < BIAS_IT; ++it) sBias[tid + it * 64 * NW] = bias_v[it];
    }
    if (has_ln) sGB[tid] = gb_v;          // [gamma(128) | beta(128)] = 256 threads
    __syncthreads();          // (publishes the biases and gamma / beta too: stays where no index is staged)
    G4C_STAMPW(1);
    if (!direct0 && (SHAPED || p.n_src > 0)) gather(0, false);
    __builtin_amdgcn_sched_barrier(0);

    if (SHAPED || p.n_src > 0) park(0);          // (before the additive gathers: the input registers are free again while those are in flight)
    G4C_STAMPW(2);
    // Operands are swapped in the MFMAs (weights as A, activations as B), so the accumulators are TRANSPOSED: this lane
    // holds sample row i (= lane & 31, + 32 per row tile) and the 16 output features 32*ct0 + 8*(q>>2) + 4*h + (q&3):
    // four runs of four consecutive features -> 16-byte gathers / LDS accesses instead of 16 scalar ones.
    f32x16 acc[RT], acc1[RT];       // acc1: the 2^-11 terms of the two-way fp16 split (SP == 2 only)
    const int fbase = ct0 * 32 + 4 * h;
    // a layer's accumulators start at its bias (then the additive rows, then the products — the order mlp_ws_kernel adds them in):
    // no bias add in the epilogues
    auto bias_start = [&](int l) __attribute__((always_inline)) {
#pragma unroll
        for (int gq = 0; gq < 4; ++gq) {
            const f32x4 b4 = *reinterpret_cast<const f32x4 *>((LDS_BIAS ? sBias : p.b) + l * NP + fbase + 8 * gq);
#pragma unroll
            for (int t = 0; t < RT; ++t)
#pragma unroll
                for (int e = 0; e < 4; ++e) { acc[t][4 * gq + e] = b4[e]; if (!SHAPED) acc1[t][4 * gq + e] = 0.f; }          // (shaped: ZC of mma_block_bx6)
        }
    };
    bias_start(0);
    if constexpr (!SHAPED)
    for (int a = 0; a < p.n_add; ++a) {
        const int width = p.add[a].width;
        const bool vec = FULL || (((p.add[a].ld & 3) == 0) && ((width & 3) == 0) && (((uintptr_t)p.add[a].ptr & 15) == 0));
        f32x4 tt[RT][4];
#pragma unroll
        for (int t = 0; t < RT; ++t) {
            const float *pr = p.add[a].ptr + (long long)sRowAdd[a * ROWS + i + 32 * t] * p.add[a].ld;
            if (SP == 1 && p.add[a].bf16) {          // bf16 rows (128 wide, 8-byte aligned: the launcher checks), widened by a shift / a mask
                const __bf16 *pr16 = reinterpret_cast<const __bf16 *>(p.add[a].ptr) + (long long)sRowAdd[a * ROWS + i + 32 * t] * p.add[a].ld;
#pragma unroll
                for (int gq = 0; gq < 4; ++gq) tt[t][gq] = widen_bf16x4(*reinterpret_cast<const u32x2 *>(pr16 + fbase + 8 * gq));
            } else
            if (vec) {
#pragma unroll
                for (int gq = 0; gq < 4; ++gq) {
                    const int f = fbase + 8 * gq;
                    tt[t][gq] = *reinterpret_cast<const f32x4 *>(pr + ((FULL || f < width) ? f : 0));
                }
            } else {
#pragma unroll
                for (int gq = 0; gq < 4; ++gq)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int f = fbase + 8 * gq + e;
                        tt[t][gq][e] = pr[f < width ? f : 0];
                    }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < RT; ++t)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[t][4 * gq + e] += (FULL || fbase + 8 * gq + e < width) ? tt[t][gq][e] : 0.f;
        __builtin_amdgcn_sched_barrier(0);
    }
    // narrow input blocks (2..8 columns): x[row, k] * W1^T[k, :] in fp32 on the vector ALUs — a padded 128-k block of
    // six-product MFMAs for 2 columns of input would cost 48 MFMAs per wave; this costs 16 FMAs per column
    const int n_nar = [&] { if constexpr (SHAPED) return SH::N_NAR; else return p.n_nar; }();
    for (int a = 0; a < n_nar; ++a) {
        const float *wn = p.nar[a].w + fbase;
#pragma unroll
        for (int t = 0; t < RT; ++t) {
            long long gr = row0 + i + 32 * t;
            if (gr >= mlim) gr = mlim - 1;
            const float *xr = p.nar[a].ptr + gr * p.nar[a].ld;
            for (int kk = 0; kk < p.nar[a].width; ++kk) {
                const float x = xr[kk];
#pragma unroll
                for (int gq = 0; gq < 4; ++gq) {
                    const f32x4 w4 = *reinterpret_cast<const f32x4 *>(wn + kk * NP + 8 * gq);
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[t][4 * gq + e] = fmaf(x, w4[e], acc[t][4 * gq + e]);
                }
            }
        }
    }
    __syncthreads();
    G4C_STAMPW(3);

    // ---------------------------------------------------------------- layer 0: one (padded) 128-k input block at a time
    const __bf16 *pa = sB + i * HB + 8 * h;
    auto block0 = [&](int s, bool more, auto zc_tag) __attribute__((always_inline)) {
        if (more && RT == 1) gather(s + 1, SHAPED);          // (RT = 2: 32 more live registers would cost a wave per SIMD; a shape's sources behind the first are direct)
        __builtin_amdgcn_sched_barrier(0);
        mma_block_bx6<RT, SP, false, RD6, decltype(zc_tag)::value>(pa, PLN, ring, rs, wofs, lo_b, acc, acc1);
        wofs += 2u * BLOCK6;
        __syncthreads();                   // everybody is done reading the planes
        if (more) {
            if (RT != 1) gather(s + 1, SHAPED);
            park(s + 1);
            __syncthreads();
        }
    };
    if constexpr (SHAPED) {
        block0(0, 1 < SH::N_SRC, std::integral_constant<int, 1>{});          // (acc1 starts at zero here)
#pragma unroll
        for (int s = 1; s < SH::N_SRC; ++s) block0(s, s + 1 < SH::N_SRC, std::integral_constant<int, 0>{});
    } else {
        for (int s = 0; s < p.n_src; ++s) block0(s, s + 1 < p.n_src, std::integral_constant<int, 0>{});
    }
    G4C_STAMPW(4);
    // one layer boundary: the epilogue of layer l, then (unless it was the last: true) the block of layer l + 1
    auto layer_step = [&](const int l) __attribute__((always_inline)) -> bool {
        const bool last = (l == n_layers - 1);
        if (last) {
            // final tile in fp32 for the LayerNorm / store epilogue (aliases the operand planes: everybody finished
            // reading them at the barrier that closed the previous block)
#pragma unroll
            for (int t = 0; t < RT; ++t)
#pragma unroll
                for (int gq = 0; gq < 4; ++gq) {
                    f32x4 x;
#pragma unroll
                    for (int e = 0; e < 4; ++e) x[e] = SP == 2 ? fmaf(acc1[t][4 * gq + e], F16_LO_UNSCALE, acc[t][4 * gq + e]) : acc[t][4 * gq + e];
                    *reinterpret_cast<f32x4 *>(sH + (i + 32 * t) * HS + fbase + 8 * gq) = x;
                    if (SAVE) {
                        const long long gr = row0 + i + 32 * t;
                        if (p.save[l] && gr < mlim) {
                            if (SP == 1 && p.save_bf16) save_row4_bf16(p, l, gr, fbase + 8 * gq, x);
                            else *reinterpret_cast<f32x4 *>(p.save[l] + gr * p.save_ld + fbase + 8 * gq) = x;
                        }
                    }
                    __builtin_amdgcn_sched_barrier(0);
                }
            __syncthreads();
            G4C_STAMPW(5 + 2 * l);
            return true;
        }
#pragma unroll
        for (int t = 0; t < RT; ++t)
#pragma unroll
            for (int gq = 0; gq < 4; ++gq) {
                f32x4 x;
#pragma unroll
                for (int e = 0; e < 4; ++e) x[e] = SP == 2 ? fmaf(acc1[t][4 * gq + e], F16_LO_UNSCALE, acc[t][4 * gq + e]) : acc[t][4 * gq + e];
                bf16x4 vh, vm, vl;
                f32x4 y;
                if (SAVE && p.mul[l]) {
                    const long long gr = row0 + i + 32 * t;
                    const f32x4 r = (SP == 1 && p.mul_bf16)
                                        ? mul_row4_bf16(p, l, gr < mlim ? gr : mlim - 1, fbase + 8 * gq)
                                        : *reinterpret_cast<const f32x4 *>(p.mul[l] + (gr < mlim ? gr : mlim - 1) * p.mul_ld + fbase + 8 * gq);
                    const float sc = 1.0507009873554804934193349852946f, sa = 1.7580993408473768599402175208123f;   // scale, scale * alpha
#pragma unroll
                    for (int e = 0; e < 4; ++e) y[e] = x[e] * (r[e] > 0.f ? sc : r[e] + sa);
                } else {
                    y = selu4(x);
                }
                if (SAVE) {
                    const long long gr = row0 + i + 32 * t;
                    if (p.save[l] && gr < mlim) {
                        if (SP == 1 && p.save_bf16) save_row4_bf16(p, l, gr, fbase + 8 * gq, y);
                        else *reinterpret_cast<f32x4 *>(p.save[l] + gr * p.save_ld + fbase + 8 * gq) = y;
                    }
                }
                split3x4<SP>(y, vh, vm, vl, rng);
                __bf16 *d = sB + (i + 32 * t) * HB + fbase + 8 * gq;
                *reinterpret_cast<bf16x4 *>(d) = vh;
                if (SP >= 2) *reinterpret_cast<bf16x4 *>(d + PLN) = vm;
                if (SP == 3) *reinterpret_cast<bf16x4 *>(d + 2 * PLN) = vl;
                __builtin_amdgcn_sched_barrier(0);
            }
        __syncthreads();
        G4C_STAMPW(5 + 2 * l);
        bias_start(l + 1);
        mma_block_bx6<RT, SP, false, RD6, SHAPED ? 1 : 0>(pa, PLN, ring, rs, wofs, lo_b, acc, acc1);
        wofs += 2u * BLOCK6;
        __syncthreads();
        G4C_STAMPW(6 + 2 * l);
        return false;
    };
    if constexpr (RT == 2) {
        // (64-row tiles: unrolled over the shape's layers.  Rolled, hipcc keeps the finished layer's four accumulators beside the next
        // layer's across the loop's back edge: 196 registers instead of 138.)
#pragma unroll
        for (int l = 0; l < SH::N_LAYERS; ++l) if (layer_step(l)) break;
    } else {
        for (int l = 0;; ++l) if (layer_step(l)) break;
    }
    G4C_STAMPW(12);
    if constexpr (RT == 1) {
        split_finish<NW, ROWS, SHAPED>(p, sH, sGB, wave, lane, row0, mlim);
    } else {
        // a 64-row tile finishes as its two 32-row tiles would: a row's LayerNorm sums run over the same eight lanes of sixteen columns
        // in the same order, and each half stores through a descriptor of its own rows below mlim
#pragma unroll
        for (int t = 0; t < RT; ++t) split_finish<NW, 32, SHAPED>(p, sH + 32 * t * HS, sGB, wave, lane, row0 + 32 * t, mlim);
    }
    G4C_STAMPW(13);
    if constexpr (!SHAPED)
    if (p.agg) {
        // aggregation of the targets whose messages this tile holds (rows in CSR order): same summation order and the
        // same mean formula as segment_reduce_kernel, so the result is bit-identical to the separate launch
        __syncthreads();
        const int s0 = p.tile_seg[tile], s1 = p.tile_seg[tile + 1];
        const int col = tid & (NP - 1);
        for (int sg = s0 + (tid >> 7); sg < s1; sg += (64 * NW) >> 7) {
            const int b = p.seg_off[sg] - (int)row0, e = p.seg_off[sg + 1] - (int)row0;
            float a = 0.f;
            for (int r = b; r < e; ++r) a += sH[r * HS + col];
            if (p.agg_mean) a /= (float)((e - b) > 1 ? (e - b) : 1);
            p.agg[(long long)sg * p.agg_ld + col] = a;
        }
    }
    const int n_heads = [&] { if constexpr (SHAPED) return SH::N_HEADS; else return p.n_heads; }();
    if (n_heads) {
        // heads (see Params): the finished fp32 tile -> three operand planes (they alias it: read everything, barrier,
        // then overwrite), then one 128-k block per head whose weights continue the stream
        __syncthreads();
        f32x4 v[RT][4];
#pragma unroll
        for (int t = 0; t < RT; ++t)
#pragma unroll
            for (int q = 0; q < 4; ++q) v[t][q] = *reinterpret_cast<const f32x4 *>(sH + (grow_l + 32 * t) * HS + q * KC + c4);
        if (!SMALL) __syncthreads();          // (SMALL: the planes do not alias the tile; their last readers are behind older barriers)
#pragma unroll
        for (int t = 0; t < RT; ++t)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                bf16x4 vh, vm, vl;
                split3x4<SP>(v[t][q], vh, vm, vl, rng);
                __bf16 *d = sB + (grow_l + 32 * t) * HB + q * KC + c4;
                *reinterpret_cast<bf16x4 *>(d) = vh;
                if (SP >= 2) *reinterpret_cast<bf16x4 *>(d + PLN) = vm;
                if (SP == 3) *reinterpret_cast<bf16x4 *>(d + 2 * PLN) = vl;
            }
        __syncthreads();
        G4C_STAMPW(14);
        // untransposed accumulator (SWAP): lane (i, h) holds column ct0 * 32 + i of the rows 32 t + 8 gq + 4 h + e; one dword
        // store per value, 32 lanes = one 128-byte line of a row.  The rows of the tile past mlim fall outside the buffer
        // descriptor's range (num_records) and are dropped by the hardware.
        const long long left = mlim - row0;
        // (wave-uniform by construction, but a value the vector ALU produced — the clamp below is a v_med3 — lives in a vector register,
        // and a buffer descriptor built from vector registers makes hipcc wrap EVERY store in a readfirstlane "waterfall" loop: twelve
        // instructions per stored dword, 1 450 cycles per head of a tile.  Explicitly scalar:)
        const int nrows = __builtin_amdgcn_readfirstlane(left >= ROWS ? ROWS : (left > 0 ? (int)left : 0));
        const unsigned vo = (unsigned)(4 * h * p.head_ld + ct0 * 32 + i) * 4u;
        auto head_store = [&](int hd, const f32x16 (&a)[RT], const f32x16 (&a1)[RT]) __attribute__((always_inline)) {
            // (rounded-bf16 mode, head_bf16: the rows are stored as bf16 — 2-byte elements: a store instruction writes 64 contiguous
            // bytes of each of two rows; their reader adds them to fp32 accumulators after widening)
            const int esz = (SP == 1 && p.head_bf16) ? 2 : 4;
            const unsigned long long hb = reinterpret_cast<unsigned long long>(p.head_out[hd]) + (unsigned long long)row0 * p.head_ld * esz;
            float *const hbase = reinterpret_cast<float *>(((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(hb >> 32)) << 32) |
                                                           (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)hb));
            const __amdgpu_buffer_rsrc_t rh = __builtin_amdgcn_make_buffer_rsrc(hbase, 0, nrows * p.head_ld * esz, 0x00020000);
#pragma unroll
            for (int t = 0; t < RT; ++t)
#pragma unroll
                for (int gq = 0; gq < 4; ++gq)
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float x = SP == 2 ? fmaf(a1[t][4 * gq + e], F16_LO_UNSCALE, a[t][4 * gq + e]) : a[t][4 * gq + e];
                        // (the row offset is part of the VECTOR offset: the scalar offset is not range-checked)
                        if (SP == 1 && p.head_bf16)
                            __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(unsigned short, (__bf16)x), rh,
                                                                  (vo >> 1) + (unsigned)((32 * t + 8 * gq + e) * p.head_ld) * 2u, 0, 0);
                        else
                        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, x), rh, vo + (unsigned)((32 * t + 8 * gq + e) * p.head_ld) * 4u, 0, 0);
                    }
        };
        auto head_zero = [&](f32x16 (&a)[RT], f32x16 (&a1)[RT]) __attribute__((always_inline)) {
#pragma unroll
            for (int t = 0; t < RT; ++t)
#pragma unroll
                for (int q = 0; q < 16; ++q) { a[t][q] = 0.f; a1[t][q] = 0.f; }
        };
        if constexpr (SMALL) {
            static_assert(G4C_MAX_HEADS == 2, "the small-launch head path multiplies both heads before it stores either");
            f32x16 acc2[RT], acc21[RT];
            head_zero(acc, acc1); head_zero(acc2, acc21);
            mma_block_bx6<RT, SP, true, RD6>(pa, PLN, ring, rs, wofs, lo_b, acc, acc1);
            wofs += 2u * BLOCK6;
            if (n_heads > 1) mma_block_bx6<RT, SP, true, RD6>(pa, PLN, ring, rs, wofs, lo_b, acc2, acc21);
            head_store(0, acc, acc1);
            if (n_heads > 1) head_store(1, acc2, acc21);
        } else {
            for (int hd = 0; hd < n_heads; ++hd) {
                if (!SHAPED) head_zero(acc, acc1);
                mma_block_bx6<RT, SP, true, RD6, SHAPED ? 3 : 0>(pa, PLN, ring, rs, wofs, lo_b, acc, acc1);
                wofs += 2u * BLOCK6;
                head_store(hd, acc, acc1);
            }
        }
    }
    G4C_STAMPW(15);
    if constexpr (SP == 2 && TRACK) range_report(p, rng);
}

// bf16x6 image of one layer: three planes (h, m, l) of the exact split of every weight.  F16: the two-way fp16 split (h, l * 2^11)
// in planes 0 / 1 of the same layout, plane 2 zero.
template <bool F16>
__global__ void pack_layer_bx6_kernel(const float *__restrict__ W, int n_out, int k_in, PackSegs segs,
                                      __bf16 *__restrict__ packed, int k_pad) {
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= k_pad * NP) return;
    const int kp = gid / NP, n = gid % NP;
    int k = -1, base_p = 0, base = 0, neg = 0;
    for (int s = 0; s < segs.n_seg; ++s) {
        if (kp >= base_p && kp < base_p + segs.wpad[s]) {
            const int j = kp - base_p;
            if (j < segs.width[s]) { k = base + j; neg = segs.neg[s]; }
        }
        base_p += segs.wpad[s];
        base += segs.width[s];
    }
    float v = 0.f;
    if (k >= 0 && n < n_out) v = W[(long long)n * k_in + k];
    if (neg) v = -v;
    __bf16 a, b, c;
    if (F16) { split2(v, a, b); c = (__bf16)0.f; }
    else split3(v, a, b, c);
    const int kk = kp & 127;
    __bf16 *d = packed + (long long)(kp >> 7) * BLOCK6 + (n >> 5) * 8 * STEP6 + (kk >> 4) * STEP6 + (((kk >> 3) & 1) * 32 + (n & 31)) * 8 + (kk & 7);
    d[0] = a; d[512] = b; d[1024] = c;
}

#ifdef G4C_TILE_ISA_ONLY
// -DG4C_TILE_ISA_ONLY (tests/test_tile_isa.py, with --cuda-device-only -S): nothing but the chip-filling f16x3 inference instantiations —
// the node-update shapes, the generic kernel they replace (tracked and certified) and the three-layer UpMP / DownMP shapes (tracked) — — for a look at their registers and instructions
// in seconds instead of the minute the whole file takes
#define G4C_TILE_ISA(TRACK)                                                                                              \
    template __global__ void mlp_bx6_kernel<1, true, true, 2, false, 2, TRACK, TileShapeGeneric>(const Params);          \
    template __global__ void mlp_bx6_kernel<1, true, true, 2, false, 2, TRACK, TileShapeNode<2, 0>>(const Params);       \
    template __global__ void mlp_bx6_kernel<1, true, true, 2, false, 2, TRACK, TileShapeNode<2, 2>>(const Params);       \
    template __global__ void mlp_bx6_kernel<1, true, true, 2, false, 2, TRACK, TileShapeNode<3, 0>>(const Params);       \
    template __global__ void mlp_bx6_kernel<1, true, true, 2, false, 2, TRACK, TileShapeNode<3, 2>>(const Params);
G4C_TILE_ISA(true)
G4C_TILE_ISA(false)
#undef G4C_TILE_ISA
template __global__ void mlp_bx6_kernel<1, true, true, 2, false, 2, true, TileShapeUp<3, 0>>(const Params);
template __global__ void mlp_bx6_kernel<1, true, true, 2, false, 2, true, TileShapeUp<3, 2>>(const Params);
template __global__ void mlp_bx6_kernel<1, true, true, 2, false, 2, true, TileShapeDown<3>>(const Params);
// the 64-row tile form (g4c_mlp_tile_form; tests/test_tile_forms_isa.py): every instantiation tile_go_rows64 launches
#define G4C_TILE_ISA(TRACK)                                                                                              \
    template __global__ void mlp_bx6_kernel<2, true, true, 2, false, 2, TRACK, TileShapeNode<2, 0>>(const Params);       \
    template __global__ void mlp_bx6_kernel<2, true, true, 2, false, 2, TRACK, TileShapeNode<2, 2>>(const Params);       \
    template __global__ void mlp_bx6_kernel<2, true, true, 2, false, 2, TRACK, TileShapeNode<3, 0>>(const Params);       \
    template __global__ void mlp_bx6_kernel<2, true, true, 2, false, 2, TRACK, TileShapeNode<3, 2>>(const Params);
G4C_TILE_ISA(true)
G4C_TILE_ISA(false)
#undef G4C_TILE_ISA
template __global__ void mlp_bx6_kernel<2, true, true, 2, false, 2, true, TileShapeUp<2, 0>>(const Params);
template __global__ void mlp_bx6_kernel<2, true, true, 2, false, 2, true, TileShapeUp<2, 2>>(const Params);
template __global__ void mlp_bx6_kernel<2, true, true, 2, false, 2, true, TileShapeUp<3, 0>>(const Params);
template __global__ void mlp_bx6_kernel<2, true, true, 2, false, 2, true, TileShapeUp<3, 2>>(const Params);
#endif

}  // namespace

#ifndef G4C_TILE_ISA_ONLY
extern "C" int g4c_mlp_pack_layer(const float *W, int32_t n_out, int32_t k_in, const int32_t *seg_width,
                                  const int32_t *seg_negate, int32_t n_seg, int32_t w_format, void *packed,
                                  int32_t k_pad, int32_t n_pad, void *stream) {
    G4C_REQUIRE(W && packed && seg_width, G4C_EINVAL, "g4c_mlp_pack_layer: null pointer");
    G4C_REQUIRE(n_seg >= 1 && n_seg <= G4C_MAX_SRC, G4C_EUNSUPPORTED, "g4c_mlp_pack_layer: %d input blocks (max %d)", n_seg, G4C_MAX_SRC);
    G4C_REQUIRE(n_out >= 1 && n_out <= NP, G4C_EUNSUPPORTED, "g4c_mlp_pack_layer: layer width %d unsupported (max 128)", n_out);
    G4C_REQUIRE(w_format >= G4C_WFMT_FP32 && w_format <= G4C_WFMT_BF16, G4C_EINVAL, "g4c_mlp_pack_layer: unknown w_format %d", w_format);
    const bool planes = w_format != G4C_WFMT_FP32;     // the three-plane bf16 stream: every input block padded to 128 k
    if (planes)
        G4C_REQUIRE(n_pad == NP && k_pad == NP * n_seg, G4C_EINVAL, "g4c_mlp_pack_layer: n_pad must be 128 and k_pad 128 per input block (got %d, %d)",
                    n_pad, k_pad);
    else
        G4C_REQUIRE(n_pad == NP, G4C_EINVAL, "g4c_mlp_pack_layer: n_pad must be 128, got %d", n_pad);
    PackSegs segs;
    segs.n_seg = n_seg;
    int ksum = 0, kpsum = 0;
    for (int s = 0; s < n_seg; ++s) {
        if (planes)
            G4C_REQUIRE(seg_width[s] > 0 && seg_width[s] <= NP, G4C_EUNSUPPORTED, "g4c_mlp_pack_layer: input block %d is %d wide (1..128)", s, seg_width[s]);
        else
            G4C_REQUIRE(seg_width[s] > 0, G4C_EINVAL, "g4c_mlp_pack_layer: empty input block %d", s);
        segs.width[s] = seg_width[s];
        segs.wpad[s] = planes ? NP : (seg_width[s] + KC - 1) / KC * KC;
        segs.neg[s] = seg_negate ? seg_negate[s] : 0;
        ksum += segs.width[s];
        kpsum += segs.wpad[s];
    }
    G4C_REQUIRE(ksum == k_in, G4C_EINVAL, "g4c_mlp_pack_layer: blocks sum to %d columns, weight has %d", ksum, k_in);
    G4C_REQUIRE(kpsum <= k_pad && k_pad % KC == 0, G4C_EINVAL, "g4c_mlp_pack_layer: k_pad %d too small for %d (or not a multiple of 32)", k_pad, kpsum);
    const dim3 grid((k_pad * NP + 255) / 256), blk(256);
    hipStream_t st = (hipStream_t)stream;
    g4c::DeviceGuard on_device(packed);
    if (!planes) pack_layer_kernel<<<grid, blk, 0, st>>>(W, n_out, k_in, segs, (float *)packed, k_pad);
    else if (w_format == G4C_WFMT_F16X2) pack_layer_bx6_kernel<true><<<grid, blk, 0, st>>>(W, n_out, k_in, segs, (__bf16 *)packed, k_pad);
    else pack_layer_bx6_kernel<false><<<grid, blk, 0, st>>>(W, n_out, k_in, segs, (__bf16 *)packed, k_pad);
    return g4c::check_launch("g4c_mlp_pack_layer");
}

namespace g4cm {

// ---- the fp32 kernel --------------------------------------------------------------------------------------------------------------------
bool split_takes(const Launch &L) { return !L.bx6; }

int split_launch(const Launch &L, hipStream_t st, Ran &ran) {
    const Params &p = L.p;
    ran.kernel = G4C_KERNEL_MLP_SPLIT;
    if (L.all_vec) mlp_split_kernel<4, true><<<dim3(p.n_tiles), dim3(256), 0, st>>>(p);
    else mlp_split_kernel<4, false><<<dim3(p.n_tiles), dim3(256), 0, st>>>(p);
    return g4c::check_launch("g4c_mlp_run");
}

// ---- the tile kernel --------------------------------------------------------------------------------------------------------------------
bool tile_takes(const Launch &L) { return L.bx6 && !L.row_split; }

// The shape whose every field this f16x3 inference launch of whole 128-wide aligned blocks on the two-step ring matches, or
// G4C_TILE_SHAPE_GENERIC.  (`full` has checked: every weighted source 128 wide, fp32 rows on 16-byte boundaries.)
static int tile_shape_of(const Params &p) {
    const int G = G4C_TILE_SHAPE_GENERIC;
    if (p.n_src < 1 || p.n_src > 2 || p.n_add || p.n_nar > 1 || (p.n_layers != 2 && p.n_layers != 3) || (p.n_heads != 0 && p.n_heads != 2)) return G;
    for (int s = 0; s < p.n_src; ++s) {
        const Src &d = p.src[s];
        if (d.seg_off || d.pre_act != G4C_ACT_NONE || d.bf16 || d.width != NP || !d.vec) return G;
        // a direct source's rows go through a buffer descriptor with 32-bit offsets: its byte extent (a whole last tile included) stays below 2^31
        if (!d.idx && (p.M + 32) * (long long)d.ld * 4 >= (1LL << 31)) return G;
    }
    if ((p.M + 32) * (long long)p.out_ld * 4 >= (1LL << 31)) return G;          // (the output rows likewise)
    if (!p.gamma || p.n_out != NP || !p.out || ((uintptr_t)p.out & 15) || (p.out_ld & 3) || p.out_idx || p.resid || p.out_bf16 || p.agg ||
        p.tile_rows || p.head_bf16)
        return G;
    const bool idx0 = p.src[0].idx != nullptr, idx1 = p.n_src > 1 && p.src[1].idx != nullptr;
    if (p.n_src == 2 && p.n_nar == 0 && !idx0 && !idx1) return G4C_TILE_SHAPE_NODE;
    // (a narrow block has no range proof — ops.range_bounds — so the launches that carry one are tracked: no tracker-free form of their shapes)
    if (p.n_nar != 1 || p.range_certified) return G;
    if (p.n_src == 2 && idx0 && !idx1) return G4C_TILE_SHAPE_UP;
    if (p.n_src == 1 && !idx0 && p.n_heads == 0) return G4C_TILE_SHAPE_DOWN;
    return G;
}

// The instantiation ladder, in two rungs.  tile_go: (VEC, FULL) of an instantiation whose other parameters are fixed, by how the
// input blocks can be addressed — whole 128-wide aligned blocks, 16-byte addressable ones, anything.
template <int SP, bool SAVE, int RD6>
static void tile_go(const Launch &L, bool full, hipStream_t st) {
    const Params &p = L.p;
    const dim3 grid(p.n_tiles), blk(256);
    if (full) mlp_bx6_kernel<1, true, true, SP, SAVE, RD6><<<grid, blk, 0, st>>>(p);
    else if (L.all_vec) mlp_bx6_kernel<1, true, false, SP, SAVE, RD6><<<grid, blk, 0, st>>>(p);
    else mlp_bx6_kernel<1, false, false, SP, SAVE, RD6><<<grid, blk, 0, st>>>(p);
}
// ... of the instantiations that exist for whole blocks only (f16x3 inference): a compile-time shape on the two-step ring — tracked,
// or certified where the shape has a tracker-free form — and the tracker-free generic kernel on either ring
template <bool TRACK>
static void tile_go_full(int shape, const Launch &L, hipStream_t st) {
    const Params &p = L.p;
#define G4C_FULL(RD6, ...) mlp_bx6_kernel<1, true, true, 2, false, RD6, TRACK, __VA_ARGS__><<<dim3(p.n_tiles), dim3(256), 0, st>>>(p)
    const bool l3 = p.n_layers == 3, h2 = p.n_heads == 2;
    if (shape == G4C_TILE_SHAPE_NODE) {
        if (l3) { if (h2) G4C_FULL(2, TileShapeNode<3, 2>); else G4C_FULL(2, TileShapeNode<3, 0>); }
        else { if (h2) G4C_FULL(2, TileShapeNode<2, 2>); else G4C_FULL(2, TileShapeNode<2, 0>); }
    } else if constexpr (TRACK) {
        if (shape == G4C_TILE_SHAPE_UP) {
            if (l3) { if (h2) G4C_FULL(2, TileShapeUp<3, 2>); else G4C_FULL(2, TileShapeUp<3, 0>); }
            else { if (h2) G4C_FULL(2, TileShapeUp<2, 2>); else G4C_FULL(2, TileShapeUp<2, 0>); }
        } else {
            if (l3) G4C_FULL(2, TileShapeDown<3>); else G4C_FULL(2, TileShapeDown<2>);
        }
    } else {
        if (L.deep_ring) G4C_FULL(8, TileShapeGeneric); else G4C_FULL(2, TileShapeGeneric);
    }
#undef G4C_FULL
}
// The tile form of a shaped launch (g4c_mlp_tile_form; Launch::tile_form) — 1: 64-row tiles (a weight fragment feeds two row tiles:
// half the weight stream per row), registers bounded for three workgroups per CU.  Same arithmetic in the same order per row:
// bit-identical to form 0.  False: the shape has no 64-row form or the launch does not fit it — the caller launches form 0.
// (A 32-row form bounded for FIVE workgroups per CU was measured beside it and is not built: scripts/variants/r23_tile_five_workgroups.patch.)
template <bool TRACK>
static bool tile_go_rows64(int shape, const Launch &L, hipStream_t st) {
    Params p = L.p;
    const bool l3 = p.n_layers == 3, h2 = p.n_heads == 2;
    // (a whole last tile of 64 rows inside the 32-bit offsets of the row descriptors, as tile_shape_of asks for 32)
    for (int s = 0; s < p.n_src; ++s)
        if (!p.src[s].idx && (p.M + 64) * (long long)p.src[s].ld * 4 >= (1LL << 31)) return false;
    if ((p.M + 64) * (long long)p.out_ld * 4 >= (1LL << 31)) return false;
    p.n_tiles = (int)((L.row_count + 63) / 64);
#define G4C_ROWS64(...) mlp_bx6_kernel<2, true, true, 2, false, 2, TRACK, __VA_ARGS__><<<dim3(p.n_tiles), dim3(256), 0, st>>>(p)
    if (shape == G4C_TILE_SHAPE_NODE) {
        if (l3) { if (h2) G4C_ROWS64(TileShapeNode<3, 2>); else G4C_ROWS64(TileShapeNode<3, 0>); }
        else { if (h2) G4C_ROWS64(TileShapeNode<2, 2>); else G4C_ROWS64(TileShapeNode<2, 0>); }
    } else if constexpr (TRACK) {
        // (DownMP's shape has no 64-row form: its headline launch did not move, 49.5 against 49.6 us — DESIGN.md 6, round 23)
        if (shape != G4C_TILE_SHAPE_UP) return false;
        if (l3) { if (h2) G4C_ROWS64(TileShapeUp<3, 2>); else G4C_ROWS64(TileShapeUp<3, 0>); }
        else { if (h2) G4C_ROWS64(TileShapeUp<2, 2>); else G4C_ROWS64(TileShapeUp<2, 0>); }
    } else {
        return false;          // (the UpMP shape has no tracker-free form)
    }
#undef G4C_ROWS64
    return true;
}
// The other rung: (SAVE, RD6) of a split SP — the training form on the two-step ring; inference on the deep ring when the launch is small
template <int SP>
static void tile_go_sp(const Launch &L, bool full, hipStream_t st) {
    if (L.save) tile_go<SP, true, 2>(L, full, st);
    else if (L.deep_ring) tile_go<SP, false, 8>(L, full, st);
    else tile_go<SP, false, 2>(L, full, st);
}

int tile_launch(const Launch &L, hipStream_t st, Ran &ran) {
    const Params &p = L.p;
    bool full = L.all_vec;
    for (int s2 = 0; s2 < p.n_src; ++s2) full = full && p.src[s2].width == NP;
    for (int a = 0; a < p.n_add; ++a)
        full = full && p.add[a].width == NP && (p.add[a].ld & 3) == 0 && ((uintptr_t)p.add[a].ptr & (p.add[a].bf16 ? 7 : 15)) == 0;
    const bool infer_full = L.f16x2 && !L.save && full;
    // (a launch every field of which matches a compile-time shape: same kernel code, tracked or certified)
    const int shape = infer_full && !L.deep_ring && L.shapes ? tile_shape_of(p) : G4C_TILE_SHAPE_GENERIC;
    // (the tracker-free instantiations: whole 128-wide aligned blocks — every launch of a model's MP layers, pools and unpools)
    const bool cert = infer_full && p.range_certified;
    ran.kernel = cert ? G4C_KERNEL_MLP_BX6_CERT : G4C_KERNEL_MLP_BX6;
    ran.shape = shape;
    ran.tile_rows = 32;
    if (shape != G4C_TILE_SHAPE_GENERIC && L.tile_form == 1 && (cert ? tile_go_rows64<false>(shape, L, st) : tile_go_rows64<true>(shape, L, st)))
        ran.tile_rows = 64;
    else
    if (cert) tile_go_full<false>(shape, L, st);
    else if (shape != G4C_TILE_SHAPE_GENERIC) tile_go_full<true>(shape, L, st);
    else if (L.f16x2) tile_go_sp<2>(L, full, st);
    else if (L.round1) tile_go_sp<1>(L, full, st);          // (with save: mixed-precision training, one product per element, fp32 save / mul rows)
    else tile_go_sp<3>(L, full, st);
    return g4c::check_launch("g4c_mlp_run");
}

}  // namespace g4cm
#endif  // G4C_TILE_ISA_ONLY
