// First AND second derivatives on the mesh by a weighted least-squares fit of a quadratic over a stencil the caller brings
// (include/g4c.h):
//   g4c_mesh_jet_weights   once per mesh: per node the fp64 normal matrix of its stencil, scaled to a unit diagonal, factored by
//                          Cholesky, and per stencil entry the fp32 row c_s with  jet(i) = sum_s c_s (x[src_s] - x[i]);
//   g4c_mesh_jet           per call: the derivatives a small program names (first: 0 .. dim - 1, second: dim .. Q - 1);
//   g4c_mesh_jet_adjoint   the transpose of that linear map (its backward): a scatter to the senders taken as a gather over
//                          sender-side tables, one thread per node in a fixed order.
// A node's sum is taken by ONE thread over its entries in CSR order, in fp32 without contraction: the bits are a function of the
// data alone.  Nothing here is part of the rollout: no step index, no snapshots, no statistics.
#include "g4c_common.h"

// No contraction anywhere in this file: every product is rounded before it is added, so a plain host loop reproduces the per-call
// bits, and the fp64 weights differ from their restatement by the library's square root and division at most.
#pragma clang fp contract(off)

namespace {

constexpr int JT_THREADS = 256;
constexpr int JT_MAX_BLOCKS = 1024;          // as the gradient: 4 workgroups of 256 per CU on 256 CUs
constexpr int MAX_COLS = G4C_DERIVED_MAX_COLS, MAX_TERMS = G4C_DERIVED_MAX_TERMS;
constexpr int MAX_USED = G4C_JET_MAX_FIELDS;          // distinct fields one program may differentiate (u, v, w, p)
constexpr int MAX_Q = 9;

constexpr int jet_q(int dim) { return dim + dim * (dim + 1) / 2; }
constexpr int tri(int i, int j) { return i * (i + 1) / 2 + j; }          // the lower triangle, row-major: (0,0), (1,0), (1,1), ..

inline long long jt_blocks(long long n_nodes) {
    const long long b = (n_nodes + JT_THREADS - 1) / JT_THREADS;
    return b < 1 ? 1 : (b > JT_MAX_BLOCKS ? JT_MAX_BLOCKS : b);
}

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
// A number every lane holds alike (read from LDS), as a scalar: the tests and loop bounds on it stay wave-uniform branches.
__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// The program as the kernel reads it (a kernel argument, copied to LDS by the workgroup's first thread): its distinct fields in the
// order of their first appearance, and per term the derivative it picks — row = (place of its field in that list) * Q + axis — and
// its coefficient.
struct jet_prog_t {
    int nd;
    unsigned char n_terms[MAX_COLS];
    unsigned char row[MAX_COLS][MAX_TERMS];
    float coef[MAX_COLS][MAX_TERMS];
    int field[MAX_USED];
};

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
    const int nd = uniform(p.nd);
    const long long stride = (long long)gridDim.x * JT_THREADS;
    for (long long n = (long long)blockIdx.x * JT_THREADS + threadIdx.x; n < n_nodes; n += stride) {
        // (no contraction: every product is rounded to fp32 before it is added, so a plain numpy.float32 loop gives the same bits)
#pragma clang fp contract(off)
        float xi[NU], J[NU][Q];
        const float *xr = x + n * x_ld;
#pragma unroll
        for (int f = 0; f < NU; ++f) {
            xi[f] = xr[p.field[f]];
#pragma unroll
            for (int a = 0; a < Q; ++a) J[f][a] = 0.f;
        }
        const int e0 = off[n], e1 = off[n + 1];
        // (two entries at a time: their index, row and weight loads are in flight together — the adds keep the CSR order)
#pragma unroll 2
        for (int e = e0; e < e1; ++e) {
            const float *xs = x + (long long)src[e] * x_ld;
            float ce[Q];
#pragma unroll
            for (int a = 0; a < Q; ++a) ce[a] = cw[(long long)e * Q + a];
#pragma unroll
            for (int f = 0; f < NU; ++f) {
                const float diff = xs[p.field[f]] - xi[f];
#pragma unroll
                for (int a = 0; a < Q; ++a) {
                    const float pr = ce[a] * diff;
                    J[f][a] += pr;
                }
            }
        }
        // The program picks its derivatives by run-time (wave-uniform) numbers: they go through this thread's own column of LDS, so
        // that the pick is an address, not a chain of selects over registers.  No barrier: a thread reads back only what it wrote.
#pragma unroll
        for (int f = 0; f < NU; ++f) {
#pragma unroll
            for (int a = 0; a < Q; ++a) mine[f * Q + a][threadIdx.x] = J[f][a];
        }
        float *cur = out + n * nd;
#pragma unroll
        for (int c = 0; c < MAX_COLS; ++c) {
            if (c < nd) {                           // (wave-uniform, as every test on the program is)
                float q = 0.f;
#pragma unroll
                for (int k = 0; k < MAX_TERMS; ++k) {
                    if (k < uniform(p.n_terms[c])) {
                        const float pr = p.coef[c][k] * mine[p.row[c][k]][threadIdx.x];
                        q = k == 0 ? pr : q + pr;
                    }
                }
                cur[c] = q;
            }
        }
    }
}

// The caller's program (1 <= nd <= MAX_COLS checked by the caller) as the kernels read it, and the number of distinct fields.
int jet_program(const char *me, const g4c_derived_program_t *prog, int nf, int dim, jet_prog_t &u, int &nu) {
    const int Q = jet_q(dim);
    u.nd = prog->nd;
    nu = 0;
    for (int c = 0; c < prog->nd; ++c) {
        G4C_REQUIRE(prog->n_terms[c] >= 1, G4C_EINVAL, "%s: column %d has %d terms", me, c, prog->n_terms[c]);
        G4C_REQUIRE(prog->n_terms[c] <= MAX_TERMS, G4C_EUNSUPPORTED, "%s: column %d has %d terms (1 .. %d are supported)", me, c,
                    prog->n_terms[c], MAX_TERMS);
    }
    for (int c = 0; c < prog->nd; ++c) {
        u.n_terms[c] = (unsigned char)prog->n_terms[c];
        for (int k = 0; k < prog->n_terms[c]; ++k) {
            const int f = prog->field[c][k], a = prog->axis[c][k];
            G4C_REQUIRE(f >= 0 && f < nf, G4C_EINVAL, "%s: column %d term %d: field %d out of range (nf=%d)", me, c, k, f, nf);
            G4C_REQUIRE(a >= 0 && a < Q, G4C_EINVAL, "%s: column %d term %d: derivative %d out of range (dim=%d: 0 .. %d)", me, c, k, a, dim,
                        Q - 1);
            int at = 0;
            while (at < nu && u.field[at] != f) ++at;
            if (at == nu) {
                G4C_REQUIRE(nu < MAX_USED, G4C_EUNSUPPORTED, "%s: the program differentiates more than %d distinct fields", me, MAX_USED);
                u.field[nu++] = f;
            }
            u.row[c][k] = (unsigned char)(at * Q + a);
            u.coef[c][k] = prog->coef[c][k];
        }
    }
    for (int f = nu; f < MAX_USED; ++f) u.field[f] = u.field[0];
    return G4C_OK;
}

template <int DIM>
void jet_launch_dim(int nu, const float *x, int x_ld, const float *c, const int *src, const int *off, const jet_prog_t &p, long long n_nodes,
                    float *out, hipStream_t s) {
    const dim3 grid((unsigned)jt_blocks(n_nodes)), block(JT_THREADS);
    // (a list shorter than its instantiation is padded with its first field: the spare accumulators are never picked)
    if (nu <= 1) mesh_jet_kernel<DIM, 1><<<grid, block, 0, s>>>(x, x_ld, c, src, off, p, n_nodes, out);
    else if (nu == 2) mesh_jet_kernel<DIM, 2><<<grid, block, 0, s>>>(x, x_ld, c, src, off, p, n_nodes, out);
    else if (nu == 3) mesh_jet_kernel<DIM, 3><<<grid, block, 0, s>>>(x, x_ld, c, src, off, p, n_nodes, out);
    else mesh_jet_kernel<DIM, 4><<<grid, block, 0, s>>>(x, x_ld, c, src, off, p, n_nodes, out);
}

// ------------------------------------------------------------------------------------------------------------------ adjoint
// jet_prog_t transposed: per derivative row r = (place of the field) * Q + axis the terms that pick it — t0[r] .. t0[r + 1], in
// program order — each the column of gy it reads and its coefficient.  Read by wave-uniform numbers from the kernel arguments.
struct jet_adj_t {
    int nd, nu, nf;
    unsigned char t0[MAX_USED * MAX_Q + 1];
    unsigned char col[MAX_COLS * MAX_TERMS];
    float coef[MAX_COLS * MAX_TERMS];
    int field[MAX_USED];
};

void jet_transpose(const jet_prog_t &u, int nu, int nf, int dim, jet_adj_t &t) {
    const int Q = jet_q(dim);
    t.nd = u.nd;
    t.nu = nu;
    t.nf = nf;
    int n = 0;
    for (int r = 0; r < MAX_USED * MAX_Q; ++r) {
        t.t0[r] = (unsigned char)n;
        if (r >= nu * Q) continue;
        for (int c = 0; c < u.nd; ++c)
            for (int k = 0; k < u.n_terms[c]; ++k)
                if (u.row[c][k] == r) {
                    t.col[n] = (unsigned char)c;
                    t.coef[n] = u.coef[c][k];
                    ++n;
                }
    }
    t.t0[MAX_USED * MAX_Q] = (unsigned char)n;
    for (int f = 0; f < MAX_USED; ++f) t.field[f] = u.field[f];
}

// H_i (include/g4c.h): every row from +0, its terms added in program order.  The counts and columns are the same in every lane.
template <int Q, int NU>
__device__ __forceinline__ void jet_adjoint_rows(const float *__restrict__ gy, long long i, const jet_adj_t &p, float (&h)[NU][Q]) {
    const float *r = gy + i * p.nd;
#pragma unroll
    for (int f = 0; f < NU; ++f) {
#pragma unroll
        for (int a = 0; a < Q; ++a) {
            float s = 0.f;
            const int t1 = uniform(p.t0[f * Q + a + 1]);
            for (int t = uniform(p.t0[f * Q + a]); t < t1; ++t) {
                const float pr = p.coef[t] * r[p.col[t]];
                s += pr;
            }
            h[f][a] = s;
        }
    }
}

template <int DIM, int NU>
__global__ __launch_bounds__(JT_THREADS) void mesh_jet_adjoint_kernel(
    const float *__restrict__ gy, const float *__restrict__ cw, const int *__restrict__ off, const float *__restrict__ out_c,
    const int *__restrict__ out_dst, const int *__restrict__ out_off, const jet_adj_t kp, long long n_nodes, float *__restrict__ gx) {
    constexpr int Q = jet_q(DIM);
    __shared__ jet_adj_t sp;          // (as the forward: the transposed program is read from LDS)
    if (threadIdx.x == 0) sp = kp;
    __syncthreads();
    const jet_adj_t &p = sp;
    const int nf = uniform(p.nf), nu = uniform(p.nu);
    const long long stride = (long long)gridDim.x * JT_THREADS;
    for (long long n = (long long)blockIdx.x * JT_THREADS + threadIdx.x; n < n_nodes; n += stride) {
#pragma clang fp contract(off)
        float acc[NU];
#pragma unroll
        for (int f = 0; f < NU; ++f) acc[f] = 0.f;
        if (cw) {          // (an empty stencil has no tables: every row is zero)
            // the entries this node sends, in ascending CSR position: their rows and receivers were copied into that order once per
            // operator, so they stream as the forward's do and only the receiver's row of gy is a gather
            const int q0 = out_off[n], q1 = out_off[n + 1];
            for (int q = q0; q < q1; ++q) {
                float ce[Q], h[NU][Q];
#pragma unroll
                for (int a = 0; a < Q; ++a) ce[a] = out_c[(long long)q * Q + a];
                jet_adjoint_rows<Q, NU>(gy, out_dst[q], p, h);
#pragma unroll
                for (int f = 0; f < NU; ++f) {
#pragma unroll
                    for (int a = 0; a < Q; ++a) {
                        const float pr = ce[a] * h[f][a];
                        acc[f] += pr;
                    }
                }
            }
            // the diagonal: this node's own entries in CSR order
            float hj[NU][Q];
            jet_adjoint_rows<Q, NU>(gy, n, p, hj);
            const int e0 = off[n], e1 = off[n + 1];
#pragma unroll 2
            for (int e = e0; e < e1; ++e) {
#pragma unroll
                for (int a = 0; a < Q; ++a) {
                    const float ca = cw[(long long)e * Q + a];
#pragma unroll
                    for (int f = 0; f < NU; ++f) {
                        const float pr = ca * hj[f][a];
                        acc[f] -= pr;
                    }
                }
            }
        }
        // every column of the row: a field the program does not name gets +0 (the fields of the list are distinct below nu)
        float *row = gx + n * nf;
        for (int c = 0; c < nf; ++c) {
            float v = 0.f;
#pragma unroll
            for (int f = 0; f < NU; ++f)
                if (f < nu && p.field[f] == c) v = acc[f];
            row[c] = v;
        }
    }
}

template <int DIM>
void jet_adjoint_launch_dim(int nu, const float *gy, const float *c, const int *off, const float *out_c, const int *out_dst, const int *out_off,
                            const jet_adj_t &p, long long n_nodes, float *gx, hipStream_t s) {
    const dim3 grid((unsigned)jt_blocks(n_nodes)), block(JT_THREADS);
    // (the rows of a list shorter than its instantiation have no terms: their accumulators stay +0 and are not written)
    if (nu <= 1) mesh_jet_adjoint_kernel<DIM, 1><<<grid, block, 0, s>>>(gy, c, off, out_c, out_dst, out_off, p, n_nodes, gx);
    else if (nu == 2) mesh_jet_adjoint_kernel<DIM, 2><<<grid, block, 0, s>>>(gy, c, off, out_c, out_dst, out_off, p, n_nodes, gx);
    else if (nu == 3) mesh_jet_adjoint_kernel<DIM, 3><<<grid, block, 0, s>>>(gy, c, off, out_c, out_dst, out_off, p, n_nodes, gx);
    else mesh_jet_adjoint_kernel<DIM, 4><<<grid, block, 0, s>>>(gy, c, off, out_c, out_dst, out_off, p, n_nodes, gx);
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
    if (const int rc = jet_program(me, prog, nf, dim, u, nu)) return rc;
    if (n_nodes == 0) return G4C_OK;
    // (c and src of an empty stencil are empty and have no address: no node reads them)
    G4C_REQUIRE(x && off && out, G4C_EINVAL, "%s: null pointer", me);
    G4C_REQUIRE(n_entries == 0 || (c && src), G4C_EINVAL, "%s: null pointer", me);
    g4c::DeviceGuard on_device(x);
    hipStream_t s = (hipStream_t)stream;
    if (dim == 2)
        jet_launch_dim<2>(nu, x, x_ld, c, src, off, u, n_nodes, out, s);
    else
        jet_launch_dim<3>(nu, x, x_ld, c, src, off, u, n_nodes, out, s);
    return g4c::check_launch(me);
}

extern "C" int g4c_mesh_jet_adjoint(const float *gy, const g4c_derived_program_t *prog, int32_t dim, int32_t nf, const float *c,
                                    const int32_t *off, const float *out_c, const int32_t *out_dst, const int32_t *out_off,
                                    int64_t n_nodes, int64_t n_entries, float *gx, void *stream) {
    const char *me = "g4c_mesh_jet_adjoint";
    G4C_REQUIRE(prog, G4C_EINVAL, "%s: null pointer", me);
    G4C_REQUIRE(n_nodes >= 0 && n_entries >= 0 && n_entries <= 0x7fffffffll / MAX_Q && nf >= 1 && prog->nd >= 1, G4C_EINVAL,
                "%s: bad sizes n_nodes=%lld n_entries=%lld nf=%d nd=%d", me, (long long)n_nodes, (long long)n_entries, nf, prog->nd);
    G4C_REQUIRE(dim == 2 || dim == 3, G4C_EUNSUPPORTED, "%s: dim=%d (2 or 3 are supported)", me, dim);
    G4C_REQUIRE(prog->nd <= MAX_COLS, G4C_EUNSUPPORTED, "%s: nd=%d columns (1 .. %d are supported)", me, prog->nd, MAX_COLS);
    jet_prog_t u = {};
    int nu = 0;
    if (const int rc = jet_program(me, prog, nf, dim, u, nu)) return rc;
    if (n_nodes == 0) return G4C_OK;
    G4C_REQUIRE(gy && gx, G4C_EINVAL, "%s: null pointer", me);
    G4C_REQUIRE(n_entries == 0 || (c && off && out_c && out_dst && out_off), G4C_EINVAL, "%s: null pointer", me);
    {          // gx [n_nodes, nf] and gy [n_nodes, nd] must not share a byte: a thread reads rows of gy that other threads' rows of gx would cover
        const char *a = (const char *)gy, *b = (const char *)gx;
        const long long na = n_nodes * prog->nd * 4ll, nb = n_nodes * nf * 4ll;
        G4C_REQUIRE(a + na <= b || b + nb <= a, G4C_EINVAL, "%s: gx aliases gy", me);
    }
    jet_adj_t t = {};
    jet_transpose(u, nu, nf, dim, t);
    g4c::DeviceGuard on_device(gx);
    hipStream_t s = (hipStream_t)stream;
    if (n_entries == 0) c = nullptr;
    if (dim == 2)
        jet_adjoint_launch_dim<2>(nu, gy, c, off, out_c, out_dst, out_off, t, n_nodes, gx, s);
    else
        jet_adjoint_launch_dim<3>(nu, gy, c, off, out_c, out_dst, out_off, t, n_nodes, gx, s);
    return g4c::check_launch(me);
}
