// Modal analysis of a snapshot matrix (g4c_snapshot_mean / _gram / _combine, include/g4c.h): the three launches of POD and DMD by the
// method of snapshots that touch L-sized data.  Snapshots are fp32 rows of L values (x[i][l], leading dimension L); every sum is fp64
// in an order that depends on the shapes alone: no floating-point atomics, nothing that depends on the grid a device happens to get.
//   mean     one thread per column, the selected rows added in slot order, one division.
//   gram     G = A' W B'^T like a GEMM with a huge K: blockIdx.y is a 64 x 64 block of G, blockIdx.x a chunk of GRAM_CHUNK columns;
//            both row blocks go through LDS as fp64 (centred, the a side times w), v_mfma_f64_16x16x4_f64 accumulates, and every
//            (block, chunk) writes one partial block into scratch; a second launch adds the chunks in chunk order and mirrors the
//            symmetric form.
//   combine  out[r] = (float) sum_i C[i][r] (x_i - mean): one thread per column, COMBINE_R accumulators, C through the scalar cache.
#include "g4c_common.h"

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int MODES_THREADS = 256;

constexpr int GRAM_BLOCK = G4C_SNAPSHOT_GRAM_BLOCK;      // edge of a block of G: 4 waves of 32 x 32, each 2 x 2 MFMA tiles of 16 x 16
constexpr int GRAM_CHUNK = G4C_SNAPSHOT_GRAM_CHUNK;      // columns of one workgroup
constexpr int GRAM_KT = 32;                              // columns staged at a time
// row stride of a staged block in doubles: 34 = 68 banks, so the 16 rows x 2 columns a half-wave reads for one MFMA operand fall on
// 32 different bank pairs, and the 32 consecutive columns a half-wave writes when it stages a row fall on all 64 banks
constexpr int GRAM_LDS_LD = GRAM_KT + 2;
constexpr int COMBINE_R = G4C_SNAPSHOT_COMBINE_BLOCK;    // accumulators of one thread

static_assert(GRAM_CHUNK % GRAM_KT == 0 && GRAM_BLOCK == 64 && MODES_THREADS == 256, "the staging below is written for these");

__global__ __launch_bounds__(MODES_THREADS) void snapshot_mean_kernel(const float *__restrict__ x, long long L, g4c_snapshot_sel_t sel,
                                                                      double *__restrict__ mean) {
    const long long l = (long long)blockIdx.x * MODES_THREADS + threadIdx.x;
    if (l >= L) return;
    const float *p = x + (long long)sel.first * L + l;
    const long long step = (long long)sel.stride * L;
    double s = 0.0;
    for (int i = 0; i < sel.count; ++i) s += (double)p[i * step];
    mean[l] = s / (double)sel.count;
}

// One (block, chunk): the partial block sum over the chunk's columns of (a_i - mean_a) w (b_j - mean_b), 64 x 64 doubles to scratch.
// Rows past the selection and columns past L are staged as zeros, so every partial block is written whole and nothing outside the
// snapshots is read.  The next tile of 32 columns is fetched into registers while the matrix pipe works on the staged one.
__global__ __launch_bounds__(MODES_THREADS) void snapshot_gram_kernel(const float *__restrict__ a, const double *__restrict__ mean_a,
                                                                      g4c_snapshot_sel_t sa, const float *__restrict__ b,
                                                                      const double *__restrict__ mean_b, g4c_snapshot_sel_t sb,
                                                                      const double *__restrict__ w, long long L, int symmetric, int nbj,
                                                                      double *__restrict__ scratch) {
    __shared__ double As[GRAM_BLOCK * GRAM_LDS_LD];
    __shared__ double Bs[GRAM_BLOCK * GRAM_LDS_LD];
    // the block: row-major over (bi, bj), the symmetric form over bj <= bi only (blk = bi (bi + 1) / 2 + bj)
    int bi, bj;
    const int blk = blockIdx.y;
    if (symmetric) {
        bi = 0;
        while ((bi + 1) * (bi + 2) / 2 <= blk) ++bi;       // (at most 16 rounds: 1024 / 64 block rows)
        bj = blk - bi * (bi + 1) / 2;
    } else {
        bi = blk / nbj;
        bj = blk - bi * nbj;
    }
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wi = wave >> 1, wj = wave & 1;
    const int kcol = tid & 31, row0 = tid >> 5;             // staging: column kcol of rows row0, row0 + 8, ...
    const long long l0 = (long long)blockIdx.x * GRAM_CHUNK;
    const long long l1 = l0 + GRAM_CHUNK < L ? l0 + GRAM_CHUNK : L;

    f64x4 acc[2][2];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int q = 0; q < 2; ++q) acc[p][q] = f64x4{0.0, 0.0, 0.0, 0.0};

    // the rows this thread stages (row0, row0 + 8, ...) of both blocks: their first elements.  A row past the selection reads the
    // first selected row instead and a column past the chunk the chunk's last one — every load is of a snapshot's own element and
    // needs no branch — and bit p of va / vb says whether the value counts.
    const float *pa[GRAM_BLOCK / 8], *pb[GRAM_BLOCK / 8];
    unsigned va = 0, vb = 0;
#pragma unroll
    for (int p = 0; p < GRAM_BLOCK / 8; ++p) {
        const int ia = bi * GRAM_BLOCK + p * 8 + row0, ib = bj * GRAM_BLOCK + p * 8 + row0;
        va |= (ia < sa.count ? 1u : 0u) << p;
        vb |= (ib < sb.count ? 1u : 0u) << p;
        pa[p] = a + ((long long)sa.first + (long long)(ia < sa.count ? ia : 0) * sa.stride) * L;
        pb[p] = b + ((long long)sb.first + (long long)(ib < sb.count ? ib : 0) * sb.stride) * L;
    }
    // one tile ahead in registers: the loads of tile t + 1 are in flight while the matrix pipe works on tile t
    float fa[GRAM_BLOCK / 8], fb[GRAM_BLOCK / 8];
    double ma = 0.0, mb = 0.0, wl = 1.0;
    bool in = false;                                        // this thread's column of the fetched tile lies inside the chunk
    auto fetch = [&](long long lt) {
        in = lt + kcol < l1;
        const long long l = in ? lt + kcol : l1 - 1;
        ma = mean_a ? mean_a[l] : 0.0;
        mb = mean_b ? mean_b[l] : 0.0;
        wl = w ? w[l] : 1.0;
#pragma unroll
        for (int p = 0; p < GRAM_BLOCK / 8; ++p) {
            fa[p] = pa[p][l];
            fb[p] = pb[p][l];
        }
    };
    fetch(l0);
    for (long long lt = l0; lt < l1; lt += GRAM_KT) {
        {
#pragma clang fp contract(off)
#pragma unroll
            for (int p = 0; p < GRAM_BLOCK / 8; ++p) {
                const int r = p * 8 + row0;
                // (a column past the chunk or a row past the selection is staged as zero, whatever mean and weight say)
                As[r * GRAM_LDS_LD + kcol] = in && (va >> p & 1u) ? ((double)fa[p] - ma) * wl : 0.0;
                Bs[r * GRAM_LDS_LD + kcol] = in && (vb >> p & 1u) ? (double)fb[p] - mb : 0.0;
            }
        }
        __syncthreads();
        if (lt + GRAM_KT < l1) fetch(lt + GRAM_KT);
        // A operand of v_mfma_f64_16x16x4_f64: lane holds A[lane & 15][lane >> 4]; B operand: B[lane >> 4][lane & 15] = b_row[lane & 15]
        const double *ar = As + (wi * 32 + (lane & 15)) * GRAM_LDS_LD + (lane >> 4);
        const double *br = Bs + (wj * 32 + (lane & 15)) * GRAM_LDS_LD + (lane >> 4);
#pragma unroll
        for (int kk = 0; kk < GRAM_KT; kk += 4) {
            const double a0 = ar[kk], a1 = ar[16 * GRAM_LDS_LD + kk];
            const double b0 = br[kk], b1 = br[16 * GRAM_LDS_LD + kk];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
        __syncthreads();
    }
    // D of the f64 form: register r of a lane is D[(lane >> 4) + 4 r][lane & 15]
    double *out = scratch + ((long long)blk * gridDim.x + blockIdx.x) * (GRAM_BLOCK * GRAM_BLOCK);
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = wi * 32 + p * 16 + (lane >> 4) + 4 * r;
                const int j = wj * 32 + q * 16 + (lane & 15);
                out[i * GRAM_BLOCK + j] = acc[p][q][r];
            }
}

// The chunks of one entry added in chunk order; the symmetric form writes the entries on and below the diagonal and their mirror images.
__global__ __launch_bounds__(MODES_THREADS) void snapshot_gram_reduce_kernel(const double *__restrict__ scratch, int chunks, int ma, int mb,
                                                                             int symmetric, int nbj, double *__restrict__ G, long long ld) {
    const int blk = blockIdx.y;
    int bi, bj;
    if (symmetric) {
        bi = 0;
        while ((bi + 1) * (bi + 2) / 2 <= blk) ++bi;
        bj = blk - bi * (bi + 1) / 2;
    } else {
        bi = blk / nbj;
        bj = blk - bi * nbj;
    }
    const int e = blockIdx.x * MODES_THREADS + threadIdx.x;       // (< 4096: the grid is 16 x blocks)
    const int i = bi * GRAM_BLOCK + e / GRAM_BLOCK, j = bj * GRAM_BLOCK + e % GRAM_BLOCK;
    if (i >= ma || j >= mb || (symmetric && j > i)) return;
    const double *p = scratch + (long long)blk * chunks * (GRAM_BLOCK * GRAM_BLOCK) + e;
    double s = 0.0;
    for (int c = 0; c < chunks; ++c) s += p[(long long)c * (GRAM_BLOCK * GRAM_BLOCK)];
    G[(long long)i * ld + j] = s;
    if (symmetric && i != j) G[(long long)j * ld + i] = s;
}

// RN accumulators r0 .. r0 + RN - 1 of one column; the product is rounded before it is added (a plain fp64 loop gives the same bits)
template <int RN>
__device__ __forceinline__ void combine_cols(const float *__restrict__ x, const double *__restrict__ mean, const g4c_snapshot_sel_t &sel,
                                             const double *__restrict__ c, long long ldc, int r0, long long L, long long l,
                                             float *__restrict__ out) {
#pragma clang fp contract(off)
    double acc[RN];
#pragma unroll
    for (int r = 0; r < RN; ++r) acc[r] = 0.0;
    const double m = mean ? mean[l] : 0.0;
    const float *p = x + (long long)sel.first * L + l;
    const long long step = (long long)sel.stride * L;
#pragma unroll 4
    for (int i = 0; i < sel.count; ++i) {
        const double d = (double)p[i * step] - m;
        const double *ci = c + i * ldc + r0;            // (uniform over the launch)
#pragma unroll
        for (int r = 0; r < RN; ++r) {
            const double t = ci[r] * d;
            acc[r] = acc[r] + t;
        }
    }
#pragma unroll
    for (int r = 0; r < RN; ++r) out[(long long)(r0 + r) * L + l] = (float)acc[r];
}

__global__ __launch_bounds__(MODES_THREADS) void snapshot_combine_kernel(const float *__restrict__ x, const double *__restrict__ mean,
                                                                         g4c_snapshot_sel_t sel, const double *__restrict__ c, long long ldc,
                                                                         int R, long long L, float *__restrict__ out) {
    const long long l = (long long)blockIdx.x * MODES_THREADS + threadIdx.x;
    if (l >= L) return;
    const int r0 = blockIdx.y * COMBINE_R;
    const int rn = R - r0 < COMBINE_R ? R - r0 : COMBINE_R;
    switch (rn) {            // (uniform over the workgroup)
        case 1: combine_cols<1>(x, mean, sel, c, ldc, r0, L, l, out); break;
        case 2: combine_cols<2>(x, mean, sel, c, ldc, r0, L, l, out); break;
        case 3: combine_cols<3>(x, mean, sel, c, ldc, r0, L, l, out); break;
        case 4: combine_cols<4>(x, mean, sel, c, ldc, r0, L, l, out); break;
        case 5: combine_cols<5>(x, mean, sel, c, ldc, r0, L, l, out); break;
        case 6: combine_cols<6>(x, mean, sel, c, ldc, r0, L, l, out); break;
        case 7: combine_cols<7>(x, mean, sel, c, ldc, r0, L, l, out); break;
        default: combine_cols<8>(x, mean, sel, c, ldc, r0, L, l, out); break;
    }
}
static_assert(COMBINE_R == 8, "the switch above names the block's sizes");

// A selection of rows of a buffer of sel.rows snapshots: EINVAL with the entry point's and the argument's name
int check_sel(const char *me, const char *name, const g4c_snapshot_sel_t *s) {
    G4C_REQUIRE(s, G4C_EINVAL, "%s: null pointer (%s)", me, name);
    G4C_REQUIRE(s->rows >= 1 && s->first >= 0 && s->stride >= 1 && s->count >= 1, G4C_EINVAL,
                "%s: %s: rows=%d first=%d stride=%d count=%d (rows, stride, count >= 1, first >= 0)", me, name, s->rows, s->first, s->stride,
                s->count);
    G4C_REQUIRE((long long)s->first + (long long)(s->count - 1) * s->stride < s->rows, G4C_EINVAL,
                "%s: %s: the last selected row %lld is outside the %d snapshots", me, name,
                (long long)s->first + (long long)(s->count - 1) * s->stride, s->rows);
    return G4C_OK;
}

int check_columns(const char *me, int64_t L) {
    G4C_REQUIRE(L >= 1, G4C_EINVAL, "%s: L=%lld (>= 1)", me, (long long)L);
    G4C_REQUIRE(L <= G4C_SNAPSHOT_MAX_COLUMNS, G4C_EUNSUPPORTED, "%s: L=%lld values in a snapshot (at most %lld: 32-bit indices within one)", me,
                (long long)L, (long long)G4C_SNAPSHOT_MAX_COLUMNS);
    return G4C_OK;
}

long long gram_blocks(int ma, int mb, bool symmetric) {
    const long long nbi = (ma + GRAM_BLOCK - 1) / GRAM_BLOCK, nbj = (mb + GRAM_BLOCK - 1) / GRAM_BLOCK;
    return symmetric ? nbi * (nbi + 1) / 2 : nbi * nbj;
}

}  // namespace

extern "C" int g4c_snapshot_mean(const float *x, const g4c_snapshot_sel_t *sel, int64_t L, double *mean_out, void *stream) {
    const char *me = "g4c_snapshot_mean";
    int rc = check_sel(me, "sel", sel);
    if (rc == G4C_OK) rc = check_columns(me, L);
    if (rc != G4C_OK) return rc;
    G4C_REQUIRE(x && mean_out, G4C_EINVAL, "%s: null pointer", me);
    g4c::DeviceGuard on_device(x);
    const unsigned blocks = (unsigned)((L + MODES_THREADS - 1) / MODES_THREADS);
    snapshot_mean_kernel<<<dim3(blocks), dim3(MODES_THREADS), 0, (hipStream_t)stream>>>(x, L, *sel, mean_out);
    return g4c::check_launch(me);
}

extern "C" int64_t g4c_snapshot_gram_scratch_bytes(int32_t ma, int32_t mb, int64_t L, int32_t symmetric) {
    if (ma < 1 || mb < 1 || L < 1 || ma > G4C_SNAPSHOT_MAX_ROWS || mb > G4C_SNAPSHOT_MAX_ROWS || L > G4C_SNAPSHOT_MAX_COLUMNS ||
        (symmetric && ma != mb))
        return -1;
    const long long chunks = (L + GRAM_CHUNK - 1) / GRAM_CHUNK;
    return 8ll * GRAM_BLOCK * GRAM_BLOCK * gram_blocks(ma, mb, symmetric != 0) * chunks;
}

extern "C" int g4c_snapshot_gram(const float *a, const double *mean_a, const g4c_snapshot_sel_t *sel_a, const float *b, const double *mean_b,
                                 const g4c_snapshot_sel_t *sel_b, const double *w, int64_t L, double *G_out, int64_t ld, void *scratch,
                                 void *stream) {
    const char *me = "g4c_snapshot_gram";
    int rc = check_sel(me, "sel_a", sel_a);
    if (rc == G4C_OK) rc = check_sel(me, "sel_b", sel_b);
    if (rc == G4C_OK) rc = check_columns(me, L);
    if (rc != G4C_OK) return rc;
    G4C_REQUIRE(a && b && G_out && scratch, G4C_EINVAL, "%s: null pointer", me);
    const int ma = sel_a->count, mb = sel_b->count;
    G4C_REQUIRE(ld >= mb, G4C_EINVAL, "%s: ld=%lld < Mb=%d", me, (long long)ld, mb);
    G4C_REQUIRE(ma <= G4C_SNAPSHOT_MAX_ROWS && mb <= G4C_SNAPSHOT_MAX_ROWS, G4C_EUNSUPPORTED,
                "%s: a Gram matrix of %d x %d snapshots (at most %d a side)", me, ma, mb, G4C_SNAPSHOT_MAX_ROWS);
    const bool symmetric = a == b && mean_a == mean_b && sel_a->first == sel_b->first && sel_a->stride == sel_b->stride && ma == mb;
    const long long chunks = (L + GRAM_CHUNK - 1) / GRAM_CHUNK;
    const int nbj = (mb + GRAM_BLOCK - 1) / GRAM_BLOCK;
    const long long blocks = gram_blocks(ma, mb, symmetric);
    g4c::DeviceGuard on_device(a);
    snapshot_gram_kernel<<<dim3((unsigned)chunks, (unsigned)blocks), dim3(MODES_THREADS), 0, (hipStream_t)stream>>>(
        a, mean_a, *sel_a, b, mean_b, *sel_b, w, L, symmetric ? 1 : 0, nbj, (double *)scratch);
    rc = g4c::check_launch(me);
    if (rc != G4C_OK) return rc;
    snapshot_gram_reduce_kernel<<<dim3(GRAM_BLOCK * GRAM_BLOCK / MODES_THREADS, (unsigned)blocks), dim3(MODES_THREADS), 0, (hipStream_t)stream>>>(
        (const double *)scratch, (int)chunks, ma, mb, symmetric ? 1 : 0, nbj, G_out, ld);
    return g4c::check_launch(me);
}

extern "C" int g4c_snapshot_combine(const float *x, const double *mean, const g4c_snapshot_sel_t *sel, const double *C, int64_t ldc, int32_t R,
                                    int64_t L, float *out, void *stream) {
    const char *me = "g4c_snapshot_combine";
    int rc = check_sel(me, "sel", sel);
    if (rc == G4C_OK) rc = check_columns(me, L);
    if (rc != G4C_OK) return rc;
    G4C_REQUIRE(x && C && out, G4C_EINVAL, "%s: null pointer", me);
    G4C_REQUIRE(R >= 1 && ldc >= R, G4C_EINVAL, "%s: R=%d (>= 1), ldc=%lld (>= R)", me, R, (long long)ldc);
    G4C_REQUIRE(R <= G4C_SNAPSHOT_MAX_ROWS, G4C_EUNSUPPORTED, "%s: R=%d combinations (at most %d)", me, R, G4C_SNAPSHOT_MAX_ROWS);
    G4C_REQUIRE(sel->count <= G4C_SNAPSHOT_MAX_ROWS, G4C_EUNSUPPORTED, "%s: %d snapshots (at most %d)", me, sel->count, G4C_SNAPSHOT_MAX_ROWS);
    g4c::DeviceGuard on_device(x);
    const unsigned blocks = (unsigned)((L + MODES_THREADS - 1) / MODES_THREADS);
    snapshot_combine_kernel<<<dim3(blocks, (unsigned)((R + COMBINE_R - 1) / COMBINE_R)), dim3(MODES_THREADS), 0, (hipStream_t)stream>>>(
        x, mean, *sel, C, ldc, R, L, out);
    return g4c::check_launch(me);
}
