// The core that the mesh's stencil operators share (mesh_gradient.hip: rows of width dim; mesh_jet.hip: rows of width
// Q = dim + dim (dim + 1) / 2).  Per node i and stencil entry e (sender src_e) a table row w_e of W floats; per field f of a small
// program S[f] = sum_e w_e (x[src_e, f] - x[i, f]), and every output column a combination of up to three of those numbers.  Here:
// the program as the kernels read it and its host translator, its transpose, the forward's node body, the adjoint kernel behind
// its entry points with their argument checks, and the ladder over the number of distinct fields.  What differs between the two
// operators is a traits struct; the weights kernels and the forward kernels stay with their operators.
// A node's sum is taken by ONE thread over its entries in CSR order, in fp32 without contraction: the bits are a function of the
// data alone.
#pragma once
#include <type_traits>

#include "g4c_common.h"
#include "step_record.h"

// No contraction in anything below (nor in the file that includes this): every product is rounded before it is added.
#pragma clang fp contract(off)

namespace {

constexpr int ST_THREADS = g4c::THREADS;          // the forward and the adjoint launch g4c::blocks_or_one(n_nodes) workgroups (step_record.h)
constexpr int MAX_COLS = G4C_DERIVED_MAX_COLS, MAX_TERMS = G4C_DERIVED_MAX_TERMS;

// What differs between the operators:
//   MAX_USED, MAX_W   distinct fields one program may differentiate, and the widest row (they size the program);
//   PROGRAM_IN_LDS    the program is copied to LDS by the workgroup's first thread (held in scalar registers over the node loop
//                     the jet's spilt them), or read from the kernel arguments;
//   SENDER_UNROLL     entries of the adjoint's sender loop in flight together (1: none — the loop as the compiler leaves it);
//   DIAGONAL_UNROLL   the same for its diagonal loop.  The adds keep their order whatever the factor;
//   AXIS, COUNT       what an error text calls a derivative's number and the number of stencil entries.
struct gradient_traits {
    static constexpr int MAX_USED = 8, MAX_W = 3;
    static constexpr bool PROGRAM_IN_LDS = false;
    static constexpr int SENDER_UNROLL = 4, DIAGONAL_UNROLL = 4;
    static constexpr const char *AXIS = "axis", *COUNT = "n_edges";
};
struct jet_traits {
    static constexpr int MAX_USED = G4C_JET_MAX_FIELDS, MAX_W = 9;          // (u, v, w, p)
    static constexpr bool PROGRAM_IN_LDS = true;
    static constexpr int SENDER_UNROLL = 1, DIAGONAL_UNROLL = 2;
    static constexpr const char *AXIS = "derivative", *COUNT = "n_entries";
};

// A number of the program every lane holds alike: read from LDS it is made a scalar, so that the tests and loop bounds on it stay
// wave-uniform branches; a kernel argument is one already.
template <class Traits>
__device__ __forceinline__ int uniform(int v) {
    if constexpr (Traits::PROGRAM_IN_LDS) return __builtin_amdgcn_readfirstlane(v);
    else return v;
}

// ------------------------------------------------------------------------------------------------------------------ the program
// The program as the forward reads it: its distinct fields in the order of their first appearance, and per term the derivative it
// picks — row = (place of its field in that list) * W + axis — and its coefficient.
template <int MAX_USED>
struct stencil_prog_t {
    int nd;
    unsigned char n_terms[MAX_COLS];
    unsigned char row[MAX_COLS][MAX_TERMS];
    float coef[MAX_COLS][MAX_TERMS];
    int field[MAX_USED];
};

// The caller's program (1 <= nd <= MAX_COLS checked by the caller) as the kernels read it for rows of width W, and the number of
// distinct fields.
template <class Traits>
int stencil_program(const char *me, const g4c_derived_program_t *prog, int nf, int dim, int W, stencil_prog_t<Traits::MAX_USED> &u, int &nu) {
    constexpr int MAX_USED = Traits::MAX_USED;
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
            G4C_REQUIRE(a >= 0 && a < W, G4C_EINVAL, "%s: column %d term %d: %s %d out of range (dim=%d: 0 .. %d)", me, c, k, Traits::AXIS, a,
                        dim, W - 1);
            int at = 0;
            while (at < nu && u.field[at] != f) ++at;
            if (at == nu) {
                G4C_REQUIRE(nu < MAX_USED, G4C_EUNSUPPORTED, "%s: the program differentiates more than %d distinct fields", me, MAX_USED);
                u.field[nu++] = f;
            }
            u.row[c][k] = (unsigned char)(at * W + a);
            u.coef[c][k] = prog->coef[c][k];
        }
    }
    for (int f = nu; f < MAX_USED; ++f) u.field[f] = u.field[0];
    return G4C_OK;
}

// stencil_prog_t transposed, as the adjoint reads it: per derivative row r = (place of the field) * W + axis the terms that pick
// it — t0[r] .. t0[r + 1], in program order — each the column of gy it reads and its coefficient.
template <int MAX_USED, int MAX_W>
struct stencil_adj_t {
    int nd, nu, nf;
    unsigned char t0[MAX_USED * MAX_W + 1];
    unsigned char col[MAX_COLS * MAX_TERMS];
    float coef[MAX_COLS * MAX_TERMS];
    int field[MAX_USED];
};

template <int MAX_USED, int MAX_W>
void stencil_transpose(const stencil_prog_t<MAX_USED> &u, int nu, int nf, int W, stencil_adj_t<MAX_USED, MAX_W> &t) {
    t.nd = u.nd;
    t.nu = nu;
    t.nf = nf;
    int n = 0;
    for (int r = 0; r < MAX_USED * MAX_W; ++r) {
        t.t0[r] = (unsigned char)n;
        if (r >= nu * W) continue;
        for (int c = 0; c < u.nd; ++c)
            for (int k = 0; k < u.n_terms[c]; ++k)
                if (u.row[c][k] == r) {
                    t.col[n] = (unsigned char)c;
                    t.coef[n] = u.coef[c][k];
                    ++n;
                }
    }
    t.t0[MAX_USED * MAX_W] = (unsigned char)n;
    for (int f = 0; f < MAX_USED; ++f) t.field[f] = u.field[f];
}

// One launch per number of distinct fields: f(std::integral_constant<int, NU>) with NU = 1, 2, 3, 4 or, above 4, MAX_USED.  (The
// forward pads a list shorter than its instantiation with its first field: the spare accumulators are never picked.  The rows of
// such a list have no terms in the adjoint: their accumulators stay +0 and are not written.)
template <int MAX_USED, class F>
void launch_nu(int nu, F &&f) {
    if (nu <= 1) f(std::integral_constant<int, 1>());
    else if (nu == 2) f(std::integral_constant<int, 2>());
    else if (nu == 3) f(std::integral_constant<int, 3>());
    else if (nu == 4 || MAX_USED == 4) f(std::integral_constant<int, 4>());
    else f(std::integral_constant<int, MAX_USED>());
}

// ------------------------------------------------------------------------------------------------------------------ forward
// S[f][a] = sum over the entries e of node n, in CSR order, of w[e][a] * (x[src_e, field_f] - x[n, field_f]), every product rounded
// before it is added (UNROLL entries at a time: their index, row and weight loads are in flight together — the adds keep the order),
// parked at mine[f * W + a] in this thread's own column of LDS for `stencil_column`.  (The sums are parked here, not by a function
// of its own between the two: that one cost the jet's forward up to 14 VGPRs and a wave per SIMD.)
template <int W, int NU, int UNROLL, class P>
__device__ __forceinline__ void stencil_accumulate(const float *x, int x_ld, long long n, const float *w, const int *src, const int *off,
                                                   const P &p, float (&mine)[NU * W][ST_THREADS]) {
    float xi[NU], S[NU][W];
    const float *xr = x + n * x_ld;
#pragma unroll
    for (int f = 0; f < NU; ++f) {
        xi[f] = xr[p.field[f]];
#pragma unroll
        for (int a = 0; a < W; ++a) S[f][a] = 0.f;
    }
    const int e0 = off[n], e1 = off[n + 1];
#pragma unroll UNROLL
    for (int e = e0; e < e1; ++e) {
        const float *xs = x + (long long)src[e] * x_ld;
        float we[W];
#pragma unroll
        for (int a = 0; a < W; ++a) we[a] = w[(long long)e * W + a];
#pragma unroll
        for (int f = 0; f < NU; ++f) {
            const float diff = xs[p.field[f]] - xi[f];
#pragma unroll
            for (int a = 0; a < W; ++a) {
                const float pr = we[a] * diff;
                S[f][a] += pr;
            }
        }
    }
#pragma unroll
    for (int f = 0; f < NU; ++f) {
#pragma unroll
        for (int a = 0; a < W; ++a) mine[f * W + a][threadIdx.x] = S[f][a];
    }
}

// Column c (< nd) of the program from the parked sums: (coef0 S0 + coef1 S1) + coef2 S2, every product rounded.  The program picks
// its derivatives by run-time (wave-uniform) numbers: they go through this thread's own column of LDS, so that the pick is an
// address, not a chain of selects over registers (whose hoisted conditions spilt hundreds of SGPRs).  No barrier: a thread reads
// back only what it wrote itself.
template <class Traits, int ROWS, class P>
__device__ __forceinline__ float stencil_column(const P &p, int c, const float (&mine)[ROWS][ST_THREADS]) {
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < MAX_TERMS; ++k) {
        if (k < uniform<Traits>(p.n_terms[c])) {
            const float pr = p.coef[c][k] * mine[p.row[c][k]][threadIdx.x];
            q = k == 0 ? pr : q + pr;
        }
    }
    return q;
}

// ------------------------------------------------------------------------------------------------------------------ adjoint
// H_i (include/g4c.h): every row from +0, its terms added in program order.  The counts and columns are the same in every lane.
template <int W, int NU, class Traits, class A>
__device__ __forceinline__ void adjoint_rows(const float *__restrict__ gy, long long i, const A &p, float (&h)[NU][W]) {
    const float *r = gy + i * p.nd;
#pragma unroll
    for (int f = 0; f < NU; ++f) {
#pragma unroll
        for (int a = 0; a < W; ++a) {
            float s = 0.f;
            const int t1 = uniform<Traits>(p.t0[f * W + a + 1]);
            for (int t = uniform<Traits>(p.t0[f * W + a]); t < t1; ++t) {
                const float pr = p.coef[t] * r[p.col[t]];
                s += pr;
            }
            h[f][a] = s;
        }
    }
}

// The transpose of the forward's map: a scatter to the senders taken as a gather over a sender-side CSR, one thread per node in a
// fixed order.  w [S, W] and off as the forward's; out_w, out_dst: the rows and receivers of the entries grouped by sender.
template <int W, int NU, class Traits>
__global__ __launch_bounds__(ST_THREADS) void stencil_adjoint_kernel(
    const float *__restrict__ gy, const float *__restrict__ w, const int *__restrict__ off, const float *__restrict__ out_w,
    const int *__restrict__ out_dst, const int *__restrict__ out_off, const stencil_adj_t<Traits::MAX_USED, Traits::MAX_W> kp,
    long long n_nodes, float *__restrict__ gx) {
    using adj_t = stencil_adj_t<Traits::MAX_USED, Traits::MAX_W>;
    const adj_t *pp = &kp;
    if constexpr (Traits::PROGRAM_IN_LDS) {
        __shared__ adj_t sp;
        if (threadIdx.x == 0) sp = kp;
        __syncthreads();
        pp = &sp;
    }
    const adj_t &p = *pp;
    const int nf = uniform<Traits>(p.nf), nu = uniform<Traits>(p.nu);
    const long long stride = (long long)gridDim.x * ST_THREADS;
    for (long long n = (long long)blockIdx.x * ST_THREADS + threadIdx.x; n < n_nodes; n += stride) {
#pragma clang fp contract(off)
        float acc[NU];
#pragma unroll
        for (int f = 0; f < NU; ++f) acc[f] = 0.f;
        if (w) {          // (an empty stencil has no tables: every row is zero)
            // the entries this node sends, in ascending CSR position: their rows and receivers were copied into that order once per
            // operator, so they stream as the forward's do and only the receiver's row of gy is a gather
            const int q0 = out_off[n], q1 = out_off[n + 1];
#pragma unroll Traits::SENDER_UNROLL
            for (int q = q0; q < q1; ++q) {
                float we[W], h[NU][W];
#pragma unroll
                for (int a = 0; a < W; ++a) we[a] = out_w[(long long)q * W + a];
                adjoint_rows<W, NU, Traits>(gy, out_dst[q], p, h);
#pragma unroll
                for (int f = 0; f < NU; ++f) {
#pragma unroll
                    for (int a = 0; a < W; ++a) {
                        const float pr = we[a] * h[f][a];
                        acc[f] += pr;
                    }
                }
            }
            // the diagonal: this node's own entries in CSR order
            float hj[NU][W];
            adjoint_rows<W, NU, Traits>(gy, n, p, hj);
            const int e0 = off[n], e1 = off[n + 1];
#pragma unroll Traits::DIAGONAL_UNROLL
            for (int e = e0; e < e1; ++e) {
#pragma unroll
                for (int a = 0; a < W; ++a) {
                    const float wa = w[(long long)e * W + a];
#pragma unroll
                    for (int f = 0; f < NU; ++f) {
                        const float pr = wa * hj[f][a];
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

// The adjoint of one operator behind its entry point: the argument checks, the program for rows of width W2 (dim 2) or W3 (dim 3),
// its transpose and the launch.  `limit` bounds the entries, so that an index into the operator's table fits 31 bits.
template <class Traits, int W2, int W3>
int stencil_adjoint(const char *me, long long limit, const float *gy, const g4c_derived_program_t *prog, int dim, int nf,
                    const float *w, const int *off, const float *out_w, const int *out_dst, const int *out_off, long long n_nodes,
                    long long n_entries, float *gx, void *stream) {
    G4C_REQUIRE(prog, G4C_EINVAL, "%s: null pointer", me);
    G4C_REQUIRE(n_nodes >= 0 && n_entries >= 0 && n_entries <= limit && nf >= 1 && prog->nd >= 1, G4C_EINVAL,
                "%s: bad sizes n_nodes=%lld %s=%lld nf=%d nd=%d", me, n_nodes, Traits::COUNT, n_entries, nf, prog->nd);
    G4C_REQUIRE(dim == 2 || dim == 3, G4C_EUNSUPPORTED, "%s: dim=%d (2 or 3 are supported)", me, dim);
    G4C_REQUIRE(prog->nd <= MAX_COLS, G4C_EUNSUPPORTED, "%s: nd=%d columns (1 .. %d are supported)", me, prog->nd, MAX_COLS);
    stencil_prog_t<Traits::MAX_USED> u = {};
    int nu = 0;
    if (const int rc = stencil_program<Traits>(me, prog, nf, dim, dim == 2 ? W2 : W3, u, nu)) return rc;
    if (n_nodes == 0) return G4C_OK;
    G4C_REQUIRE(gy && gx, G4C_EINVAL, "%s: null pointer", me);
    G4C_REQUIRE(n_entries == 0 || (w && off && out_w && out_dst && out_off), G4C_EINVAL, "%s: null pointer", me);
    {          // gx [n_nodes, nf] and gy [n_nodes, nd] must not share a byte: a thread reads rows of gy that other threads' rows of gx would cover
        const char *a = (const char *)gy, *b = (const char *)gx;
        const long long na = n_nodes * prog->nd * 4ll, nb = n_nodes * nf * 4ll;
        G4C_REQUIRE(a + na <= b || b + nb <= a, G4C_EINVAL, "%s: gx aliases gy", me);
    }
    stencil_adj_t<Traits::MAX_USED, Traits::MAX_W> t = {};
    stencil_transpose(u, nu, nf, dim == 2 ? W2 : W3, t);
    g4c::DeviceGuard on_device(gx);
    hipStream_t s = (hipStream_t)stream;
    if (n_entries == 0) w = nullptr;
    const dim3 grid((unsigned)g4c::blocks_or_one(n_nodes)), block(ST_THREADS);
    launch_nu<Traits::MAX_USED>(nu, [&](auto NU) {
        if (dim == 2)
            stencil_adjoint_kernel<W2, decltype(NU)::value, Traits><<<grid, block, 0, s>>>(gy, w, off, out_w, out_dst, out_off, t, n_nodes, gx);
        else
            stencil_adjoint_kernel<W3, decltype(NU)::value, Traits><<<grid, block, 0, s>>>(gy, w, off, out_w, out_dst, out_off, t, n_nodes, gx);
    });
    return g4c::check_launch(me);
}

}  // namespace
