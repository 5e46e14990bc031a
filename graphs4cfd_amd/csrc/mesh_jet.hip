// First AND second derivatives on the mesh by a weighted least-squares fit of a quadratic over a stencil the caller brings
// (include/g4c.h):
//   g4c_mesh_jet_weights   once per mesh: per node the fp64 normal matrix of its stencil, scaled to a unit diagonal, factored by
//                          Cholesky, and per stencil entry the fp32 row c_s with  jet(i) = sum_s c_s (x[src_s] - x[i]);
//   g4c_mesh_jet           per call: the derivatives a small program names (first: 0 .. dim - 1, second: dim .. Q - 1);
//   g4c_mesh_jet_adjoint   the transpose of that linear map (its backward): a scatter to the senders taken as a gather over
//                          sender-side tables, one thread per node in a fixed order.
// The program, the forward's node body and the adjoint are the stencil operators' common ones (stencil_op.h, shared with
// mesh_gradient.hip): here are the weights, the forward kernel round that body and the entry points.
// A node's sum is taken by ONE thread over its entries in CSR order, in fp32 without contraction: the bits are a function of the
// data alone.  Nothing here is part of the rollout: no step index, no snapshots, no statistics.
#include "g4c_common.h"
#include "stencil_op.h"

// No contraction anywhere in this file: every product is rounded before it is added, so a plain host loop reproduces the per-call
// bits, and the fp64 weights differ from their restatement by the library's square root and division at most.
#pragma clang fp contract(off)

namespace {

constexpr int JT_THREADS = ST_THREADS;
constexpr int MAX_USED = jet_traits::MAX_USED;
constexpr int MAX_Q = jet_traits::MAX_W;
using jet_prog_t = stencil_prog_t<MAX_USED>;          // (a kernel argument, copied to LDS by the workgroup's first thread)

constexpr int jet_q(int dim) { return dim + dim * (dim + 1) / 2; }
constexpr int tri(int i, int j) { return i * (i + 1) / 2 + j; }          // the lower triangle, row-major: (0,0), (1,0), (1,1), ..

// ------------------------------------------------------------------------------------------------------------------ weights
// The row of the fit for one stencil entry: d = -rel; b = (d_0 .., then for a <= b: d_a d_b, halved where a == b), so that
// x_s - x_i = sum_q b_q jet_q for a quadratic x.  Returns w = |d|^(-power).
template <int DIM>
__device__ __forceinline__ double jet_basis(const float *__restrict__ rel, long long pe, int power, double (&b)[jet_q(DIM)]) {
    double d[DIM], r2 = 0.0;
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
        d[a] = -(double)rel[pe * DIM + a];
        const double sq = d[a] * d[a];
        r2 += sq;
        b[a] = d[a];
    }
    int j = DIM;
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
#pragma unroll
        for (int c = a; c < DIM; ++c, ++j) {
            const double t = d[a] * d[c];
            b[j] = a == c ? 0.5 * t : t;
        }
    }
    return power == 0 ? 1.0 : (power == 1 ? 1.0 / sqrt(r2) : 1.0 / r2);
}

template <int DIM>
__global__ __launch_bounds__(JT_THREADS) void mesh_jet_weights_kernel(
    const int *__restrict__ off, const int *__restrict__ perm, const int *__restrict__ src32, const float *__restrict__ rel, int power,
    long long n_nodes, float *__restrict__ c, int *__restrict__ src, unsigned char *__restrict__ degenerate) {
    constexpr int Q = jet_q(DIM), NA = Q * (Q + 1) / 2;
    const long long n = (long long)blockIdx.x * JT_THREADS + threadIdx.x;
    if (n >= n_nodes) return;
    const int e0 = off[n], e1 = off[n + 1];
    // (every index below is a compile-time one: the matrix lives in registers)
    double A[NA];
#pragma unroll
    for (int j = 0; j < NA; ++j) A[j] = 0.0;
    bool bad = e1 - e0 < Q;
    for (int e = e0; e < e1; ++e) {
        const long long pe = perm ? perm[e] : e;
        double b[Q];
        const double w = jet_basis<DIM>(rel, pe, power, b);
        bad = bad || !(w <= 1.7976931348623157e308);          // a weight that is no number, or infinite (a zero-length vector)
#pragma unroll
        for (int i = 0; i < Q; ++i) {
            const double wb = w * b[i];
#pragma unroll
            for (int j = 0; j <= i; ++j) {
                const double t = wb * b[j];
                A[tri(i, j)] += t;
            }
        }
    }
    // unit diagonal: A_ij <- (A_ij sc_i) sc_j, sc_i = 1 / sqrt(A_ii) — the threshold below is then the same for x -> lambda x
    double sc[Q];
#pragma unroll
    for (int i = 0; i < Q; ++i) sc[i] = 1.0 / sqrt(A[tri(i, i)]);
#pragma unroll
    for (int i = 0; i < Q; ++i) {
#pragma unroll
        for (int j = 0; j <= i; ++j) {
            const double t = A[tri(i, j)] * sc[i];
            A[tri(i, j)] = t * sc[j];
        }
    }
    // Cholesky in place, column by column: L L^T = A; inv_j = 1 / L_jj
    double inv[Q];
#pragma unroll
    for (int j = 0; j < Q; ++j) {
        double s = A[tri(j, j)];
#pragma unroll
        for (int k = 0; k < j; ++k) {
            const double t = A[tri(j, k)] * A[tri(j, k)];
            s -= t;
        }
        bad = bad || !(s > 1e-12);          // the pivot: <= the threshold, or no number
        const double l = sqrt(s);
        A[tri(j, j)] = l;
        inv[j] = 1.0 / l;
#pragma unroll
        for (int i = j + 1; i < Q; ++i) {
            double r = A[tri(i, j)];
#pragma unroll
            for (int k = 0; k < j; ++k) {
                const double t = A[tri(i, k)] * A[tri(j, k)];
                r -= t;
            }
            A[tri(i, j)] = r * inv[j];
        }
    }
    degenerate[n] = bad ? 1 : 0;
    for (int e = e0; e < e1; ++e) {
        const long long pe = perm ? perm[e] : e;
        src[e] = src32[pe];
        float out[Q];
        if (bad) {
#pragma unroll
            for (int i = 0; i < Q; ++i) out[i] = 0.f;
        } else {
            double b[Q], y[Q];
            const double w = jet_basis<DIM>(rel, pe, power, b);
#pragma unroll
            for (int i = 0; i < Q; ++i) {          // L y = sc * b
                double s = b[i] * sc[i];
#pragma unroll
                for (int k = 0; k < i; ++k) {
                    const double t = A[tri(i, k)] * y[k];
                    s -= t;
                }
                y[i] = s * inv[i];
            }
#pragma unroll
            for (int i = Q - 1; i >= 0; --i) {          // L^T z = y (z over y)
                double s = y[i];
#pragma unroll
                for (int k = i + 1; k < Q; ++k) {
                    const double t = A[tri(k, i)] * y[k];
                    s -= t;
                }
                y[i] = s * inv[i];
            }
#pragma unroll
            for (int i = 0; i < Q; ++i) {
                const double ws = w * sc[i];
                out[i] = (float)(ws * y[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < Q; ++i) c[(long long)e * Q + i] = out[i];
    }
}

// ------------------------------------------------------------------------------------------------------------------ per call
template <int DIM, int NU>
__global__ __launch_bounds__(JT_THREADS) void mesh_jet_kernel(const float *__restrict__ x, int x_ld, const float *__restrict__ cw,
                                                             const int *__restrict__ src, const int *__restrict__ off, const jet_prog_t kp,
                                                             long long n_nodes, float *__restrict__ out) {
    constexpr int Q = jet_q(DIM);
    // The program is read from LDS, not from the kernel arguments: held in scalar registers over the node loop it spilt them.
    __shared__ jet_prog_t sp;
    __shared__ float mine[NU * Q][JT_THREADS];
    if (threadIdx.x == 0) sp = kp;
    __syncthreads();
    const jet_prog_t &p = sp;
    const int nd = uniform<jet_traits>(p.nd);
    const long long stride = (long long)gridDim.x * JT_THREADS;
    for (long long n = (long long)blockIdx.x * JT_THREADS + threadIdx.x; n < n_nodes; n += stride) {
        // (no contraction: every product is rounded to fp32 before it is added, so a plain numpy.float32 loop gives the same bits)
#pragma clang fp contract(off)
        stencil_accumulate<Q, NU, 2>(x, x_ld, n, cw, src, off, p, mine);
        float *cur = out + n * nd;
#pragma unroll
        for (int c = 0; c < MAX_COLS; ++c) {
            if (c < nd) cur[c] = stencil_column<jet_traits>(p, c, mine);          // (wave-uniform, as every test on the program is)
        }
    }
}

}  // namespace

extern "C" int g4c_mesh_jet_weights(const int32_t *off, const int32_t *perm, const int32_t *src32, const float *rel, int32_t dim,
                                    int32_t power, int64_t n_nodes, int64_t n_entries, float *c, int32_t *src, uint8_t *degenerate,
                                    void *stream) {
    const char *me = "g4c_mesh_jet_weights";
    G4C_REQUIRE(n_nodes >= 0 && n_entries >= 0 && n_entries <= 0x7fffffffll / MAX_Q, G4C_EINVAL, "%s: bad sizes n_nodes=%lld n_entries=%lld",
                me, (long long)n_nodes, (long long)n_entries);
    G4C_REQUIRE(power >= 0 && power <= 2, G4C_EINVAL, "%s: power=%d (0, 1 or 2)", me, power);
    G4C_REQUIRE(dim == 2 || dim == 3, G4C_EUNSUPPORTED, "%s: dim=%d (2 or 3 are supported)", me, dim);
    if (n_nodes == 0 || n_entries == 0) {
        // no entry: no launch.  (Every node of an empty stencil is degenerate: the caller's flags are filled by the caller.)
        return G4C_OK;
    }
    G4C_REQUIRE(off && src32 && rel && c && src && degenerate, G4C_EINVAL, "%s: null pointer", me);
    g4c::DeviceGuard on_device(off);
    hipStream_t s = (hipStream_t)stream;
    const unsigned blocks = (unsigned)((n_nodes + JT_THREADS - 1) / JT_THREADS);
    if (dim == 2)
        mesh_jet_weights_kernel<2><<<dim3(blocks), dim3(JT_THREADS), 0, s>>>(off, perm, src32, rel, power, n_nodes, c, src, degenerate);
    else
        mesh_jet_weights_kernel<3><<<dim3(blocks), dim3(JT_THREADS), 0, s>>>(off, perm, src32, rel, power, n_nodes, c, src, degenerate);
    return g4c::check_launch(me);
}

extern "C" int g4c_mesh_jet(const float *x, int32_t x_ld, int32_t nf, int32_t dim, const float *c, const int32_t *src, const int32_t *off,
                            const g4c_derived_program_t *prog, int64_t n_nodes, int64_t n_entries, float *out, void *stream) {
    const char *me = "g4c_mesh_jet";
    G4C_REQUIRE(prog, G4C_EINVAL, "%s: null pointer", me);
    G4C_REQUIRE(n_nodes >= 0 && n_entries >= 0 && n_entries <= 0x7fffffffll / MAX_Q && nf >= 1 && x_ld >= 0 && prog->nd >= 1, G4C_EINVAL,
                "%s: bad sizes n_nodes=%lld n_entries=%lld nf=%d x_ld=%d nd=%d", me, (long long)n_nodes, (long long)n_entries, nf, x_ld,
                prog->nd);
    G4C_REQUIRE(x_ld >= nf, G4C_EINVAL, "%s: x_ld=%d < nf=%d", me, x_ld, nf);
    G4C_REQUIRE(dim == 2 || dim == 3, G4C_EUNSUPPORTED, "%s: dim=%d (2 or 3 are supported)", me, dim);
    G4C_REQUIRE(prog->nd <= MAX_COLS, G4C_EUNSUPPORTED, "%s: nd=%d columns (1 .. %d are supported)", me, prog->nd, MAX_COLS);
    jet_prog_t u = {};
    int nu = 0;
    if (const int rc = stencil_program<jet_traits>(me, prog, nf, dim, jet_q(dim), u, nu)) return rc;
    if (n_nodes == 0) return G4C_OK;
    // (c and src of an empty stencil are empty and have no address: no node reads them)
    G4C_REQUIRE(x && off && out, G4C_EINVAL, "%s: null pointer", me);
    G4C_REQUIRE(n_entries == 0 || (c && src), G4C_EINVAL, "%s: null pointer", me);
    g4c::DeviceGuard on_device(x);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)g4c::blocks_or_one(n_nodes)), block(JT_THREADS);
    launch_nu<MAX_USED>(nu, [&](auto NU) {
        if (dim == 2)
            mesh_jet_kernel<2, decltype(NU)::value><<<grid, block, 0, s>>>(x, x_ld, c, src, off, u, n_nodes, out);
        else
            mesh_jet_kernel<3, decltype(NU)::value><<<grid, block, 0, s>>>(x, x_ld, c, src, off, u, n_nodes, out);
    });
    return g4c::check_launch(me);
}

extern "C" int g4c_mesh_jet_adjoint(const float *gy, const g4c_derived_program_t *prog, int32_t dim, int32_t nf, const float *c,
                                    const int32_t *off, const float *out_c, const int32_t *out_dst, const int32_t *out_off,
                                    int64_t n_nodes, int64_t n_entries, float *gx, void *stream) {
    return stencil_adjoint<jet_traits, jet_q(2), jet_q(3)>("g4c_mesh_jet_adjoint", 0x7fffffffll / MAX_Q, gy, prog, dim, nf, c, off,
                                                           out_c, out_dst, out_off, n_nodes, n_entries, gx, stream);
}
