// A least-squares gradient over the in-edges a mesh already carries, and the flow diagnostics built on it (include/g4c.h):
//   g4c_mesh_gradient_weights  once per mesh: per node the fp64 normal matrix of its in-edges, inverted in closed form, and per edge
//                              the fp32 vector g_e with  grad x (i) = sum_e g_e (x[src_e] - x[i]);
//   g4c_mesh_derived           once per step: the derivatives a small program names (divergence, vorticity, gradients), written to
//                              `cur`, to a strided snapshot slot, and reduced to per-step norms;
//   g4c_mesh_derived_adjoint   the transpose of that linear map (its backward): a scatter to the senders taken as a gather over a
//                              sender-side CSR, one thread per node in a fixed order.
// The program, the forward's node body and the adjoint are the stencil operators' common ones (stencil_op.h, shared with mesh_jet.hip).
// A node's sum is taken by ONE thread over its in-edges in CSR order, in fp32 without contraction: the bits are a function of the
// data alone.  The norms are register accumulators over rows dealt gid, gid + grid, ..., reduced by the step-record core
// (step_record.h): one partial set per workgroup, a second one-workgroup launch.  No atomics.
#include "g4c_common.h"
#include "stencil_op.h"
#include "step_record.h"

// No contraction anywhere in this file: every product is rounded before it is added, so a plain host loop reproduces the per-step
// bits, and the fp64 weights differ from their restatement by the library's square root and division at most.
#pragma clang fp contract(off)

namespace {

constexpr int MG_THREADS = ST_THREADS;
constexpr int NSTAT = G4C_DERIVED_NSTAT;
// scratch (step_record.h): the header, then [workgroup][nd][NSTAT]; of every column's set one position is a maximum
using mg_policy = g4c::max_at<NSTAT, G4C_DERIVED_MAX_ABS>;
constexpr int MAX_USED = gradient_traits::MAX_USED;
using mg_prog_t = stencil_prog_t<MAX_USED>;          // (read from the kernel arguments: in scalar registers, so it is kept small)

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
template <int DIM, int NU, bool STATS>
__global__ __launch_bounds__(MG_THREADS) void mesh_derived_kernel(const float *__restrict__ x, const g4c_mesh_derived_t d,
                                                                 const mg_prog_t p, long long n_nodes) {
    const int nd = p.nd;
    const int t = d.step ? d.step[0] : -1;
    const bool live = t >= 0 && t < d.max_steps;
    // every record address below is formed from a checked t
    float *snap = nullptr;
    int slot;
    if (d.snap && t >= 0 && d.every > 0 && g4c::snapshot_slot(t, d.every, d.n_snap, slot)) snap = d.snap + (long long)slot * n_nodes * nd;
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
        stencil_accumulate<DIM, NU, 4>(x, d.x_ld, n, d.g, d.src, d.off, p, mine);
        float *cur = d.cur + n * nd;
#pragma unroll
        for (int c = 0; c < MAX_COLS; ++c) {
            if (c < nd) {                           // (wave-uniform, as every test on the program is)
                const float q = stencil_column<gradient_traits>(p, c, mine);
                cur[c] = q;
                if (snap) snap[n * nd + c] = q;
                if constexpr (STATS) {
                    if (stats) {
                        const double qd = (double)q, aq = fabs(qd);
                        const double sq = qd * qd;
                        acc[c * NSTAT + G4C_DERIVED_SQ] += sq;
                        acc[c * NSTAT + G4C_DERIVED_ABS] += aq;
                        acc[c * NSTAT + G4C_DERIVED_MAX_ABS] = g4c::nan_max(acc[c * NSTAT + G4C_DERIVED_MAX_ABS], aq);
                    }
                }
            }
        }
    }
    if constexpr (STATS) {
        // (`stats` is the same in every workgroup: nothing in this launch writes the step index)
        if (stats) g4c::block_reduce<mg_policy>(acc, nd * NSTAT, g4c::partials(d.scratch, blockIdx.x, nd * NSTAT));
        if (gid == 0) g4c::post_step(d.scratch, stats, t);
    }
}

template <int DIM, int NU>
void derived_launch(const float *x, const g4c_mesh_derived_t &d, const mg_prog_t &p, long long n_nodes, hipStream_t s) {
    const int blocks = (int)g4c::blocks_or_one(n_nodes);
    if (d.stats) {
        mesh_derived_kernel<DIM, NU, true><<<dim3((unsigned)blocks), dim3(MG_THREADS), 0, s>>>(x, d, p, n_nodes);
        g4c::partials_kernel<mg_policy, MAX_COLS, false><<<dim3(1), dim3(MG_THREADS), 0, s>>>(d.scratch, blocks, p.nd, d.stats, d.max_steps);
    } else {
        mesh_derived_kernel<DIM, NU, false><<<dim3((unsigned)blocks), dim3(MG_THREADS), 0, s>>>(x, d, p, n_nodes);
    }
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
    return g4c::HEADER + g4c::blocks_or_one(n_nodes) * nd * NSTAT;
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
    if (const int rc = stencil_program<gradient_traits>(me, prog, d->nf, d->dim, d->dim, u, nu)) return rc;
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
    launch_nu<MAX_USED>(nu, [&](auto NU) {
        if (dd.dim == 2)
            derived_launch<2, decltype(NU)::value>(x, dd, u, n_nodes, s);
        else
            derived_launch<3, decltype(NU)::value>(x, dd, u, n_nodes, s);
    });
    return g4c::check_launch(me);
}

extern "C" int g4c_mesh_derived_adjoint(const float *gy, const g4c_derived_program_t *prog, int32_t dim, int32_t nf, const float *g,
                                        const int32_t *off, const float *out_g, const int32_t *out_dst, const int32_t *out_off,
                                        int64_t n_nodes, int64_t n_edges, float *gx, void *stream) {
    return stencil_adjoint<gradient_traits, 2, 3>("g4c_mesh_derived_adjoint", 0x7fffffffll, gy, prog, dim, nf, g, off, out_g, out_dst,
                                                  out_off, n_nodes, n_edges, gx, stream);
}
