// A least-squares gradient over the in-edges a mesh already carries, and the flow diagnostics built on it (include/g4c.h):
//   g4c_mesh_gradient_weights  once per mesh: per node the fp64 normal matrix of its in-edges, inverted in closed form, and per edge
//                              the fp32 vector g_e with  grad x (i) = sum_e g_e (x[src_e] - x[i]);
//   g4c_mesh_derived           once per step: the derivatives a small program names (divergence, vorticity, gradients), written to
//                              `cur`, to a strided snapshot slot, and reduced to per-step norms;
//   g4c_mesh_derived_adjoint   the transpose of that linear map (its backward): a scatter to the senders taken as a gather over a
//                              sender-side CSR, one thread per node in a fixed order.
// A node's sum is taken by ONE thread over its in-edges in CSR order, in fp32 without contraction: the bits are a function of the
// data alone.  The norms follow the records' rule (rollout_record.hip): register accumulators, rows dealt gid, gid + grid, ..., a
// xor butterfly per wave, the waves in order through LDS, one partial set per workgroup, a second one-workgroup launch.  No atomics.
#include "g4c_common.h"

// No contraction anywhere in this file: every product is rounded before it is added, so a plain host loop reproduces the per-step
// bits, and the fp64 weights differ from their restatement by the library's square root and division at most.
#pragma clang fp contract(off)

namespace {

constexpr int MG_THREADS = 256;
constexpr int MG_MAX_BLOCKS = 1024;          // as the records: 4 workgroups of 256 per CU on 256 CUs
constexpr int MG_HEADER = 8;                 // scratch[0]: the step whose partials follow (-1: none); the partials start at 64 bytes
constexpr int MAX_COLS = G4C_DERIVED_MAX_COLS, MAX_TERMS = G4C_DERIVED_MAX_TERMS, NSTAT = G4C_DERIVED_NSTAT;
constexpr int MAX_USED = 8;                  // distinct fields one program may differentiate

inline long long mg_blocks(long long n_nodes) {
    const long long b = (n_nodes + MG_THREADS - 1) / MG_THREADS;
    return b < 1 ? 1 : (b > MG_MAX_BLOCKS ? MG_MAX_BLOCKS : b);
}

// ------------------------------------------------------------------------------------------------------------------ weights
template <int DIM>
__global__ __launch_bounds__(MG_THREADS) void mesh_gradient_weights_kernel(
    const int *__restrict__ off, const int *__restrict__ perm, const int *__restrict__ src32, const float *__restrict__ rel, int power,
    long long n_nodes, float *__restrict__ g, int *__restrict__ src, unsigned char *__restrict__ degenerate) {
    const long long n = (long long)blockIdx.x * MG_THREADS + threadIdx.x;
    if (n >= n_nodes) return;
    const int e0 = off[n], e1 = off[n + 1];
    constexpr int NM = DIM * (DIM + 1) / 2;          // M's upper triangle, row-major: (0,0), (0,1), .., (1,1), ..
    double m[NM];
#pragma unroll
    for (int j = 0; j < NM; ++j) m[j] = 0.0;
    auto edge = [&](int e, double (&d)[DIM]) -> double {          // d_e = -rel_e, returns w_e = |d_e|^(-power)
        const long long pe = perm ? perm[e] : e;
        double r2 = 0.0;
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
            d[a] = -(double)rel[pe * DIM + a];
            const double sq = d[a] * d[a];
            r2 += sq;
        }
        return power == 0 ? 1.0 : (power == 1 ? 1.0 / sqrt(r2) : 1.0 / r2);
    };
    for (int e = e0; e < e1; ++e) {
        double d[DIM];
        const double w = edge(e, d);
        int j = 0;
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
#pragma unroll
            for (int b = a; b < DIM; ++b, ++j) {
                const double wd = w * d[a];
                const double t = wd * d[b];
                m[j] += t;
            }
        }
    }
    // adjugate (symmetric, upper triangle in the order of m) and determinant
    double adj[NM], det, tr;
    if constexpr (DIM == 2) {
        adj[0] = m[2];
        adj[1] = -m[1];
        adj[2] = m[0];
        const double p0 = m[0] * m[2], p1 = m[1] * m[1];
        det = p0 - p1;
        tr = m[0] + m[2];
    } else {
        // m = [m00 m01 m02; . m11 m12; . . m22] = m[0], m[1], m[2], m[3], m[4], m[5]
        const double c00a = m[3] * m[5], c00b = m[4] * m[4];
        const double c01a = m[2] * m[4], c01b = m[1] * m[5];
        const double c02a = m[1] * m[4], c02b = m[2] * m[3];
        const double c11a = m[0] * m[5], c11b = m[2] * m[2];
        const double c12a = m[1] * m[2], c12b = m[0] * m[4];
        const double c22a = m[0] * m[3], c22b = m[1] * m[1];
        adj[0] = c00a - c00b;
        adj[1] = c01a - c01b;
        adj[2] = c02a - c02b;
        adj[3] = c11a - c11b;
        adj[4] = c12a - c12b;
        adj[5] = c22a - c22b;
        const double t0 = m[0] * adj[0], t1 = m[1] * adj[1], t2 = m[2] * adj[2];
        det = (t0 + t1) + t2;
        tr = (m[0] + m[3]) + m[5];
    }
    const double mean = tr / (double)DIM;
    double thr = mean * mean;
    if constexpr (DIM == 3) thr = thr * mean;
    thr = 1e-12 * thr;
    // `!(det > thr)`: det <= thr, and a determinant that is no number (a zero-length edge under power >= 1 has no weight)
    const bool degen = !(det > thr);
    degenerate[n] = degen ? 1 : 0;
    for (int e = e0; e < e1; ++e) {
        const long long pe = perm ? perm[e] : e;
        src[e] = src32[pe];
        float out[DIM];
        if (degen) {
#pragma unroll
            for (int a = 0; a < DIM; ++a) out[a] = 0.f;
        } else {
            double d[DIM];
            const double w = edge(e, d);
            const double s = w / det;
            double v[DIM];
            if constexpr (DIM == 2) {
                const double a0 = adj[0] * d[0], a1 = adj[1] * d[1], b0 = adj[1] * d[0], b1 = adj[2] * d[1];
                v[0] = a0 + a1;
                v[1] = b0 + b1;
            } else {
                const double a0 = adj[0] * d[0], a1 = adj[1] * d[1], a2 = adj[2] * d[2];
                const double b0 = adj[1] * d[0], b1 = adj[3] * d[1], b2 = adj[4] * d[2];
                const double c0 = adj[2] * d[0], c1 = adj[4] * d[1], c2 = adj[5] * d[2];
                v[0] = (a0 + a1) + a2;
                v[1] = (b0 + b1) + b2;
                v[2] = (c0 + c1) + c2;
            }
#pragma unroll
            for (int a = 0; a < DIM; ++a) out[a] = (float)(s * v[a]);
        }
#pragma unroll
        for (int a = 0; a < DIM; ++a) g[(long long)e * DIM + a] = out[a];
    }
}

// ------------------------------------------------------------------------------------------------------------------ per step
// The program as the kernel reads it (in scalar registers, so it is kept small): its distinct fields in the order of their first
// appearance, and per term the derivative it picks — row = (place of its field in that list) * dim + axis — and its coefficient.
struct mg_prog_t {
    int nd;
    unsigned char n_terms[MAX_COLS];
    unsigned char row[MAX_COLS][MAX_TERMS];
    float coef[MAX_COLS][MAX_TERMS];
    int field[MAX_USED];
};

__device__ __forceinline__ double mg_combine(int j, double a, double b) { return j % NSTAT == G4C_DERIVED_MAX_ABS ? fmax(a, b) : a + b; }

// The workgroup's 256 sets of nstat (<= MAX_COLS * NSTAT) values -> one set at dst: rec_block_reduce of rollout_record.hip with a
// run-time count (the loops are unrolled over the maximum and guarded by a wave-uniform test: every index is a compile-time one).
__device__ __forceinline__ void mg_block_reduce(double (&a)[MAX_COLS * NSTAT], int nstat, double *__restrict__ dst) {
    __shared__ double part[MG_THREADS / 64][MAX_COLS * NSTAT];
#pragma unroll
    for (int j = 0; j < MAX_COLS * NSTAT; ++j) {
        if (j < nstat) {
            double x = a[j];
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) x = mg_combine(j, x, __shfl_xor(x, m, 64));
            a[j] = x;
        }
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int j = 0; j < MAX_COLS * NSTAT; ++j)
            if (j < nstat) part[wave][j] = a[j];
    }
    __syncthreads();
    if ((int)threadIdx.x < nstat) {
        const int j = threadIdx.x;
        double x = part[0][j];
#pragma unroll
        for (int w = 1; w < MG_THREADS / 64; ++w) x = mg_combine(j, x, part[w][j]);
        dst[j] = x;
    }
}

template <int DIM, int NU, bool STATS>
__global__ __launch_bounds__(MG_THREADS) void mesh_derived_kernel(const float *__restrict__ x, const g4c_mesh_derived_t d,
                                                                 const mg_prog_t p, long long n_nodes) {
    const int nd = p.nd;
    const int t = d.step ? d.step[0] : -1;
    const bool live = t >= 0 && t < d.max_steps;
    // every record address below is formed from a checked t
    float *snap = nullptr;
    if (d.snap && t >= 0 && d.every > 0 && (t + 1) % d.every == 0) {
        const int slot = (t + 1) / d.every - 1;
        if (slot < d.n_snap) snap = d.snap + (long long)slot * n_nodes * nd;
    }
    const bool stats = STATS && live;
    __shared__ float mine[NU * DIM][MG_THREADS];
    double acc[STATS ? MAX_COLS * NSTAT : 1];
#pragma unroll
    for (int j = 0; j < (STATS ? MAX_COLS * NSTAT : 1); ++j) acc[j] = 0.0;

    const long long stride = (long long)gridDim.x * MG_THREADS;
    const long long gid = (long long)blockIdx.x * MG_THREADS + threadIdx.x;
    for (long long n = gid; n < n_nodes; n += stride) {
        // (no contraction: every product is rounded to fp32 before it is added, so a plain numpy.float32 loop gives the same bits)
#pragma clang fp contract(off)
        float xi[NU], G[NU][DIM];
        const float *xr = x + n * d.x_ld;
#pragma unroll
        for (int f = 0; f < NU; ++f) {
            xi[f] = xr[p.field[f]];
#pragma unroll
            for (int a = 0; a < DIM; ++a) G[f][a] = 0.f;
        }
        const int e0 = d.off[n], e1 = d.off[n + 1];
        // (four in-edges at a time: their index, row and weight loads are in flight together — the adds keep the CSR order)
#pragma unroll 4
        for (int e = e0; e < e1; ++e) {
            const float *xs = x + (long long)d.src[e] * d.x_ld;
            float ge[DIM];
#pragma unroll
            for (int a = 0; a < DIM; ++a) ge[a] = d.g[(long long)e * DIM + a];
#pragma unroll
            for (int f = 0; f < NU; ++f) {
                const float diff = xs[p.field[f]] - xi[f];
#pragma unroll
                for (int a = 0; a < DIM; ++a) {
                    const float pr = ge[a] * diff;
                    G[f][a] += pr;
                }
            }
        }
        // The program picks its derivatives by run-time (wave-uniform) numbers: they go through this thread's own column of LDS, so
        // that the pick is an address, not a chain of selects over registers (whose hoisted conditions spilt hundreds of SGPRs).
        // No barrier: a thread reads back only what it wrote itself.
#pragma unroll
        for (int f = 0; f < NU; ++f) {
#pragma unroll
            for (int a = 0; a < DIM; ++a) mine[f * DIM + a][threadIdx.x] = G[f][a];
        }
        float *cur = d.cur + n * nd;
#pragma unroll
        for (int c = 0; c < MAX_COLS; ++c) {
            if (c < nd) {                           // (wave-uniform, as every test on the program is)
                float q = 0.f;
#pragma unroll
                for (int k = 0; k < MAX_TERMS; ++k) {
                    if (k < p.n_terms[c]) {
                        const float pr = p.coef[c][k] * mine[p.row[c][k]][threadIdx.x];
                        q = k == 0 ? pr : q + pr;
                    }
                }
                cur[c] = q;
                if (snap) snap[n * nd + c] = q;
                if constexpr (STATS) {
                    if (stats) {
                        const double qd = (double)q, aq = fabs(qd);
                        const double sq = qd * qd;
                        acc[c * NSTAT + G4C_DERIVED_SQ] += sq;
                        acc[c * NSTAT + G4C_DERIVED_ABS] += aq;
                        acc[c * NSTAT + G4C_DERIVED_MAX_ABS] = fmax(acc[c * NSTAT + G4C_DERIVED_MAX_ABS], aq);
                    }
                }
            }
        }
    }
    if constexpr (STATS) {
        // (`stats` is the same in every workgroup: nothing in this launch writes the step index)
        if (stats) mg_block_reduce(acc, nd * NSTAT, d.scratch + MG_HEADER + (long long)blockIdx.x * (nd * NSTAT));
        if (gid == 0) d.scratch[0] = stats ? (double)t : -1.0;
    }
}

// The workgroups' partials -> stats[t], one workgroup, behind the launch above on the same stream (rollout_record_stats_kernel's
// order: thread i adds the partials of workgroups i, i + 256, ..., then the same reduction).  stats[t] is overwritten.
__global__ __launch_bounds__(MG_THREADS) void mesh_derived_stats_kernel(const double *__restrict__ scratch, int n_blocks, int nd,
                                                                       double *__restrict__ stats, int max_steps) {
    const double tt = scratch[0];
    if (!(tt >= 0.0 && tt < (double)max_steps)) return;
    const int nstat = nd * NSTAT;
    double acc[MAX_COLS * NSTAT];
#pragma unroll
    for (int j = 0; j < MAX_COLS * NSTAT; ++j) acc[j] = 0.0;
    for (int b = threadIdx.x; b < n_blocks; b += MG_THREADS) {
        const double *q = scratch + MG_HEADER + (long long)b * nstat;
#pragma unroll
        for (int j = 0; j < MAX_COLS * NSTAT; ++j)
            if (j < nstat) acc[j] = mg_combine(j, acc[j], q[j]);
    }
    mg_block_reduce(acc, nstat, stats + (long long)(int)tt * nstat);
}

template <int DIM, int NU>
void derived_launch(const float *x, const g4c_mesh_derived_t &d, const mg_prog_t &p, long long n_nodes, hipStream_t s) {
    const int blocks = (int)mg_blocks(n_nodes);
    if (d.stats) {
        mesh_derived_kernel<DIM, NU, true><<<dim3((unsigned)blocks), dim3(MG_THREADS), 0, s>>>(x, d, p, n_nodes);
        mesh_derived_stats_kernel<<<dim3(1), dim3(MG_THREADS), 0, s>>>(d.scratch, blocks, p.nd, d.stats, d.max_steps);
    } else {
        mesh_derived_kernel<DIM, NU, false><<<dim3((unsigned)blocks), dim3(MG_THREADS), 0, s>>>(x, d, p, n_nodes);
    }
}

template <int DIM>
void derived_launch_dim(int nu, const float *x, const g4c_mesh_derived_t &d, const mg_prog_t &p, long long n_nodes, hipStream_t s) {
    // (a list shorter than its instantiation is padded with its first field: the spare accumulators are never picked)
    if (nu <= 1) derived_launch<DIM, 1>(x, d, p, n_nodes, s);
    else if (nu == 2) derived_launch<DIM, 2>(x, d, p, n_nodes, s);
    else if (nu == 3) derived_launch<DIM, 3>(x, d, p, n_nodes, s);
    else if (nu == 4) derived_launch<DIM, 4>(x, d, p, n_nodes, s);
    else derived_launch<DIM, MAX_USED>(x, d, p, n_nodes, s);
}

// The caller's program (1 <= nd <= MAX_COLS checked by the caller) as the kernels read it, and the number of distinct fields.
int mg_program(const char *me, const g4c_derived_program_t *prog, int nf, int dim, mg_prog_t &u, int &nu) {
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
            G4C_REQUIRE(a >= 0 && a < dim, G4C_EINVAL, "%s: column %d term %d: axis %d out of range (dim=%d)", me, c, k, a, dim);
            int at = 0;
            while (at < nu && u.field[at] != f) ++at;
            if (at == nu) {
                G4C_REQUIRE(nu < MAX_USED, G4C_EUNSUPPORTED, "%s: the program differentiates more than %d distinct fields", me, MAX_USED);
                u.field[nu++] = f;
            }
            u.row[c][k] = (unsigned char)(at * dim + a);
            u.coef[c][k] = prog->coef[c][k];
        }
    }
    for (int f = nu; f < MAX_USED; ++f) u.field[f] = u.field[0];
    return G4C_OK;
}

// ------------------------------------------------------------------------------------------------------------------ adjoint
// mg_prog_t transposed: per derivative row r = (place of the field) * dim + axis the terms that pick it — t0[r] .. t0[r + 1], in
// program order — each the column of gy it reads and its coefficient.  Read by wave-uniform numbers from the kernel arguments.
struct mg_adj_t {
    int nd, nu, nf;
    unsigned char t0[MAX_USED * 3 + 1];
    unsigned char col[MAX_COLS * MAX_TERMS];
    float coef[MAX_COLS * MAX_TERMS];
    int field[MAX_USED];
};

void mg_transpose(const mg_prog_t &u, int nu, int nf, int dim, mg_adj_t &t) {
    t.nd = u.nd;
    t.nu = nu;
    t.nf = nf;
    int n = 0;
    for (int r = 0; r < MAX_USED * 3; ++r) {
        t.t0[r] = (unsigned char)n;
        if (r >= nu * dim) continue;
        for (int c = 0; c < u.nd; ++c)
            for (int k = 0; k < u.n_terms[c]; ++k)
                if (u.row[c][k] == r) {
                    t.col[n] = (unsigned char)c;
                    t.coef[n] = u.coef[c][k];
                    ++n;
                }
    }
    t.t0[MAX_USED * 3] = (unsigned char)n;
    for (int f = 0; f < MAX_USED; ++f) t.field[f] = u.field[f];
}

// H_i (include/g4c.h): every row from +0, its terms added in program order.  The counts and columns are the same in every lane.
template <int DIM, int NU>
__device__ __forceinline__ void mg_adjoint_rows(const float *__restrict__ gy, long long i, const mg_adj_t &p, float (&h)[NU][DIM]) {
    const float *r = gy + i * p.nd;
#pragma unroll
    for (int f = 0; f < NU; ++f) {
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
            float s = 0.f;
            const int t1 = p.t0[f * DIM + a + 1];
            for (int t = p.t0[f * DIM + a]; t < t1; ++t) {
                const float pr = p.coef[t] * r[p.col[t]];
                s += pr;
            }
            h[f][a] = s;
        }
    }
}

template <int DIM, int NU>
__global__ __launch_bounds__(MG_THREADS) void mesh_derived_adjoint_kernel(
    const float *__restrict__ gy, const float *__restrict__ g, const int *__restrict__ off, const float *__restrict__ out_g,
    const int *__restrict__ out_dst, const int *__restrict__ out_off, const mg_adj_t p, long long n_nodes, float *__restrict__ gx) {
    const long long stride = (long long)gridDim.x * MG_THREADS;
    for (long long n = (long long)blockIdx.x * MG_THREADS + threadIdx.x; n < n_nodes; n += stride) {
#pragma clang fp contract(off)
        float acc[NU];
#pragma unroll
        for (int f = 0; f < NU; ++f) acc[f] = 0.f;
        if (g) {          // (a mesh without a single edge has no tables: every row is zero)
            // the edges this node sends, in ascending CSR position: their weights and receivers were copied into that order once per
            // mesh, so they stream as the forward's do and only the receiver's row of gy is a gather (four edges at a time: their
            // receiver, weight and row loads are in flight together — the adds keep the order)
            const int q0 = out_off[n], q1 = out_off[n + 1];
#pragma unroll 4
            for (int q = q0; q < q1; ++q) {
                float ge[DIM], h[NU][DIM];
#pragma unroll
                for (int a = 0; a < DIM; ++a) ge[a] = out_g[(long long)q * DIM + a];
                mg_adjoint_rows<DIM, NU>(gy, out_dst[q], p, h);
#pragma unroll
                for (int f = 0; f < NU; ++f) {
#pragma unroll
                    for (int a = 0; a < DIM; ++a) {
                        const float pr = ge[a] * h[f][a];
                        acc[f] += pr;
                    }
                }
            }
            // the diagonal: this node's own in-edges in CSR order
            float hj[NU][DIM];
            mg_adjoint_rows<DIM, NU>(gy, n, p, hj);
            const int e0 = off[n], e1 = off[n + 1];
#pragma unroll 4
            for (int e = e0; e < e1; ++e) {
#pragma unroll
                for (int a = 0; a < DIM; ++a) {
                    const float ga = g[(long long)e * DIM + a];
#pragma unroll
                    for (int f = 0; f < NU; ++f) {
                        const float pr = ga * hj[f][a];
                        acc[f] -= pr;
                    }
                }
            }
        }
        // every column of the row: a field the program does not name gets +0 (the fields of the list are distinct below nu)
        float *row = gx + n * p.nf;
        for (int c = 0; c < p.nf; ++c) {
            float v = 0.f;
#pragma unroll
            for (int f = 0; f < NU; ++f)
                if (f < p.nu && p.field[f] == c) v = acc[f];
            row[c] = v;
        }
    }
}

template <int DIM, int NU>
void adjoint_launch(const float *gy, const float *g, const int *off, const float *out_g, const int *out_dst, const int *out_off,
                    const mg_adj_t &p, long long n_nodes, float *gx, hipStream_t s) {
    mesh_derived_adjoint_kernel<DIM, NU><<<dim3((unsigned)mg_blocks(n_nodes)), dim3(MG_THREADS), 0, s>>>(gy, g, off, out_g, out_dst, out_off, p,
                                                                                                      n_nodes, gx);
}

template <int DIM>
void adjoint_launch_dim(int nu, const float *gy, const float *g, const int *off, const float *out_g, const int *out_dst, const int *out_off,
                        const mg_adj_t &p, long long n_nodes, float *gx, hipStream_t s) {
    // (the rows of a list shorter than its instantiation have no terms: their accumulators stay +0 and are not written)
    if (nu <= 1) adjoint_launch<DIM, 1>(gy, g, off, out_g, out_dst, out_off, p, n_nodes, gx, s);
    else if (nu == 2) adjoint_launch<DIM, 2>(gy, g, off, out_g, out_dst, out_off, p, n_nodes, gx, s);
    else if (nu == 3) adjoint_launch<DIM, 3>(gy, g, off, out_g, out_dst, out_off, p, n_nodes, gx, s);
    else if (nu == 4) adjoint_launch<DIM, 4>(gy, g, off, out_g, out_dst, out_off, p, n_nodes, gx, s);
    else adjoint_launch<DIM, MAX_USED>(gy, g, off, out_g, out_dst, out_off, p, n_nodes, gx, s);
}

}  // namespace

extern "C" int g4c_mesh_gradient_weights(const int32_t *off, const int32_t *perm, const int32_t *src32, const float *rel, int32_t dim,
                                         int32_t power, int64_t n_nodes, int64_t n_edges, float *g, int32_t *src, uint8_t *degenerate,
                                         void *stream) {
    const char *me = "g4c_mesh_gradient_weights";
    G4C_REQUIRE(n_nodes >= 0 && n_edges >= 0 && n_edges <= 0x7fffffffll, G4C_EINVAL, "%s: bad sizes n_nodes=%lld n_edges=%lld", me,
                (long long)n_nodes, (long long)n_edges);
    G4C_REQUIRE(power >= 0 && power <= 2, G4C_EINVAL, "%s: power=%d (0, 1 or 2)", me, power);
    G4C_REQUIRE(dim == 2 || dim == 3, G4C_EUNSUPPORTED, "%s: dim=%d (2 or 3 are supported)", me, dim);
    if (n_nodes == 0 || n_edges == 0) {
        // no edge: no launch.  (Every node of a mesh without edges is degenerate: the caller's flags are filled by the caller.)
        return G4C_OK;
    }
    G4C_REQUIRE(off && src32 && rel && g && src && degenerate, G4C_EINVAL, "%s: null pointer", me);
    g4c::DeviceGuard on_device(off);
    hipStream_t s = (hipStream_t)stream;
    const unsigned blocks = (unsigned)((n_nodes + MG_THREADS - 1) / MG_THREADS);
    if (dim == 2)
        mesh_gradient_weights_kernel<2><<<dim3(blocks), dim3(MG_THREADS), 0, s>>>(off, perm, src32, rel, power, n_nodes, g, src, degenerate);
    else
        mesh_gradient_weights_kernel<3><<<dim3(blocks), dim3(MG_THREADS), 0, s>>>(off, perm, src32, rel, power, n_nodes, g, src, degenerate);
    return g4c::check_launch(me);
}

extern "C" int64_t g4c_mesh_derived_scratch_doubles(int64_t n_nodes, int32_t nd) {
    G4C_REQUIRE(n_nodes >= 0 && nd >= 1, G4C_EINVAL, "g4c_mesh_derived_scratch_doubles: bad sizes n_nodes=%lld nd=%d", (long long)n_nodes, nd);
    G4C_REQUIRE(nd <= MAX_COLS, G4C_EUNSUPPORTED, "g4c_mesh_derived_scratch_doubles: nd=%d columns (1 .. %d are supported)", nd, MAX_COLS);
    return MG_HEADER + mg_blocks(n_nodes) * nd * NSTAT;
}

extern "C" int g4c_mesh_derived(const float *x, const g4c_mesh_derived_t *d, const g4c_derived_program_t *prog, int64_t n_nodes,
                                void *stream) {
    const char *me = "g4c_mesh_derived";
    G4C_REQUIRE(d && prog, G4C_EINVAL, "%s: null pointer", me);
    G4C_REQUIRE(n_nodes >= 0 && d->nf >= 1 && d->x_ld >= 0 && d->max_steps >= 0 && d->every >= 0 && d->n_snap >= 0 && prog->nd >= 1,
                G4C_EINVAL, "%s: bad sizes n_nodes=%lld nf=%d x_ld=%d max_steps=%d every=%d n_snap=%d nd=%d", me, (long long)n_nodes, d->nf,
                d->x_ld, d->max_steps, d->every, d->n_snap, prog->nd);
    G4C_REQUIRE(d->x_ld >= d->nf, G4C_EINVAL, "%s: x_ld=%d < nf=%d", me, d->x_ld, d->nf);
    G4C_REQUIRE(d->dim == 2 || d->dim == 3, G4C_EUNSUPPORTED, "%s: dim=%d (2 or 3 are supported)", me, d->dim);
    G4C_REQUIRE(prog->nd <= MAX_COLS, G4C_EUNSUPPORTED, "%s: nd=%d columns (1 .. %d are supported)", me, prog->nd, MAX_COLS);
    mg_prog_t u = {};
    int nu = 0;
    if (const int rc = mg_program(me, prog, d->nf, d->dim, u, nu)) return rc;
    G4C_REQUIRE(d->every > 0 || !d->snap, G4C_EINVAL, "%s: a snapshot buffer with every=0", me);
    G4C_REQUIRE(!d->stats || d->scratch, G4C_EINVAL, "%s: stats without scratch", me);
    G4C_REQUIRE(d->step || (!d->snap && !d->stats), G4C_EINVAL, "%s: snapshots or stats without a step index", me);
    if (n_nodes == 0) return G4C_OK;
    // (g and src of a mesh without a single edge are empty and have no address: no node reads them)
    G4C_REQUIRE(x && d->off && d->cur && (d->g != nullptr) == (d->src != nullptr), G4C_EINVAL, "%s: null pointer", me);
    g4c::DeviceGuard on_device(x);
    hipStream_t s = (hipStream_t)stream;
    g4c_mesh_derived_t dd = *d;
    if (dd.every == 0 || dd.n_snap == 0) dd.snap = nullptr;
    if (dd.dim == 2)
        derived_launch_dim<2>(nu, x, dd, u, n_nodes, s);
    else
        derived_launch_dim<3>(nu, x, dd, u, n_nodes, s);
    return g4c::check_launch(me);
}

extern "C" int g4c_mesh_derived_adjoint(const float *gy, const g4c_derived_program_t *prog, int32_t dim, int32_t nf, const float *g,
                                        const int32_t *off, const float *out_g, const int32_t *out_dst, const int32_t *out_off,
                                        int64_t n_nodes, int64_t n_edges, float *gx, void *stream) {
    const char *me = "g4c_mesh_derived_adjoint";
    G4C_REQUIRE(prog, G4C_EINVAL, "%s: null pointer", me);
    G4C_REQUIRE(n_nodes >= 0 && n_edges >= 0 && n_edges <= 0x7fffffffll && nf >= 1 && prog->nd >= 1, G4C_EINVAL,
                "%s: bad sizes n_nodes=%lld n_edges=%lld nf=%d nd=%d", me, (long long)n_nodes, (long long)n_edges, nf, prog->nd);
    G4C_REQUIRE(dim == 2 || dim == 3, G4C_EUNSUPPORTED, "%s: dim=%d (2 or 3 are supported)", me, dim);
    G4C_REQUIRE(prog->nd <= MAX_COLS, G4C_EUNSUPPORTED, "%s: nd=%d columns (1 .. %d are supported)", me, prog->nd, MAX_COLS);
    mg_prog_t u = {};
    int nu = 0;
    if (const int rc = mg_program(me, prog, nf, dim, u, nu)) return rc;
    if (n_nodes == 0) return G4C_OK;
    G4C_REQUIRE(gy && gx, G4C_EINVAL, "%s: null pointer", me);
    G4C_REQUIRE(n_edges == 0 || (g && off && out_g && out_dst && out_off), G4C_EINVAL, "%s: null pointer", me);
    {          // gx [n_nodes, nf] and gy [n_nodes, nd] must not share a byte: a thread reads rows of gy that other threads' rows of gx would cover
        const char *a = (const char *)gy, *b = (const char *)gx;
        const long long na = n_nodes * prog->nd * 4ll, nb = n_nodes * nf * 4ll;
        G4C_REQUIRE(a + na <= b || b + nb <= a, G4C_EINVAL, "%s: gx aliases gy", me);
    }
    mg_adj_t t = {};
    mg_transpose(u, nu, nf, dim, t);
    g4c::DeviceGuard on_device(gx);
    hipStream_t s = (hipStream_t)stream;
    if (n_edges == 0) g = nullptr;
    if (dim == 2)
        adjoint_launch_dim<2>(nu, gy, g, off, out_g, out_dst, out_off, t, n_nodes, gx, s);
    else
        adjoint_launch_dim<3>(nu, gy, g, off, out_g, out_dst, out_off, t, n_nodes, gx, s);
    return g4c::check_launch(me);
}
