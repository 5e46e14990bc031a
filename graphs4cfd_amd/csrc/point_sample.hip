// Values at points that are no mesh nodes (include/g4c.h): a moving-least-squares interpolation with a linear basis over the k
// nearest nodes of every point.
//   g4c_sample_weights  once per set of points: per point the fp64 fit over its neighbours, centred on their weighted mean, the
//                       normal matrix inverted in closed form, and per neighbour one fp32 coefficient c_j with
//                       value(q) = sum_j c_j x[idx_j];
//   g4c_sample_points   once per step (or once per target): that sum for every point and column, written to `cur` and, on a slot
//                       step, to a strided slot of a step-major series;
//   g4c_sample_points_adjoint  the transpose of that sum (its backward): the scatter from points to nodes taken as a gather — one
//                       thread per (node, chunk of columns) walks the table entries that name its node, through a node-side table
//                       built once per set of points, in ascending table position.
// A point's sum is taken by ONE thread over its neighbours nearest first, in fp32 without contraction: the bits are a function of
// the data alone.  The tables are j-major [k, P]: lane p reads consecutive addresses.  Plain loads and stores, no atomics.
#include "g4c_common.h"
#include "point_fit.h"
#include "knn_periodic.h"
#include "step_record.h"

// No contraction anywhere in this file: every product is rounded before it is added, so a plain host loop reproduces the per-step
// bits, and the fp64 coefficients differ from their restatement by the library's square root and division at most.
#pragma clang fp contract(off)

namespace {

constexpr int PS_THREADS = g4c::THREADS;          // the per-step launches take g4c::blocks(items) workgroups (step_record.h)
constexpr int PS_MAX_K = G4C_SAMPLE_MAX_K;
constexpr int PS_CHUNK = 4;                  // columns one thread sums: nf = 3 is one chunk, a whole target ceil(F / 4) per point

// ------------------------------------------------------------------------------------------------------------------ weights
template <int DIM>
__global__ __launch_bounds__(PS_THREADS) void sample_weights_kernel(const float *__restrict__ pos, const float *__restrict__ q,
                                                                   const int *__restrict__ idx, int k, int power, long long n_points,
                                                                   float *__restrict__ coef, float *__restrict__ distance,
                                                                   unsigned char *__restrict__ degenerate) {
    const long long p = (long long)blockIdx.x * PS_THREADS + threadIdx.x;
    if (p >= n_points) return;
    double qd[DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a) qd[a] = (double)q[p * DIM + a];
    auto nb = [&](int j, double (&d)[DIM]) -> double {          // d_j = pos[idx_j] - q, returns r2_j
        const long long i = idx[(long long)j * n_points + p];
        double r2 = 0.0;
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
            d[a] = (double)pos[i * DIM + a] - qd[a];
            const double sq = d[a] * d[a];
            r2 += sq;
        }
        return r2;
    };
    const bool degen = g4c::mls_fit<DIM, 0>(k, power, nb, [&](double r20) { distance[p] = (float)sqrt(r20); },          // point_fit.h
                                            [&](int j, float c) { coef[(long long)j * n_points + p] = c; });
    degenerate[p] = degen ? 1 : 0;
}

// The same fit in the wrapped metric (g4c_sample_weights_periodic): the point is wrapped into the period first, and the neighbour
// lambda wraps every d_j.  A kernel of its own: sample_weights_kernel keeps its body and its bits.
template <int DIM>
__global__ __launch_bounds__(PS_THREADS) void sample_weights_periodic_kernel(const float *__restrict__ pos, const float *__restrict__ q,
                                                                            const int *__restrict__ idx, int k, int power,
                                                                            long long n_points, float o0, float o1, float o2, float l0,
                                                                            float l1, float l2, float *__restrict__ coef,
                                                                            float *__restrict__ distance,
                                                                            unsigned char *__restrict__ degenerate) {
    const long long p = (long long)blockIdx.x * PS_THREADS + threadIdx.x;
    if (p >= n_points) return;
    const float org[3] = {o0, o1, o2}, per32[3] = {l0, l1, l2};
    double qd[DIM], per[DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
        float v = q[p * DIM + a];
        if (per32[a] > 0.f) v = g4c::wrap_coordinate(v, org[a], per32[a]);          // knn_periodic.h
        qd[a] = (double)v;
        per[a] = (double)per32[a];
    }
    auto nb = [&](int j, double (&d)[DIM]) -> double {          // d_j = the wrapped pos[idx_j] - q, returns r2_j
        const long long i = idx[(long long)j * n_points + p];
        double r2 = 0.0;
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
            d[a] = (double)pos[i * DIM + a] - qd[a];
            if (per[a] > 0.0) d[a] = g4c::wrapped_offset(d[a], per[a]);
            const double sq = d[a] * d[a];
            r2 += sq;
        }
        return r2;
    };
    const bool degen = g4c::mls_fit<DIM, 0>(k, power, nb, [&](double r20) { distance[p] = (float)sqrt(r20); },
                                            [&](int j, float c) { coef[(long long)j * n_points + p] = c; });
    degenerate[p] = degen ? 1 : 0;
}

// ------------------------------------------------------------------------------------------------------------------ per step
// One thread per (point, chunk of PS_CHUNK columns); the items are chunk-major — item = chunk * P + p — so the lanes of a wave hold
// consecutive points of one chunk and read consecutive table entries.
__global__ __launch_bounds__(PS_THREADS) void sample_points_kernel(const float *__restrict__ x, const g4c_sample_points_t s,
                                                                  long long n_points) {
    const int F = s.nf, k = s.k;
    const int t = s.step ? s.step[0] : -1;
    // the slot address is formed from a checked t
    float *series = nullptr;
    int slot;
    if (s.series && t >= 0 && t < s.max_steps && s.every > 0 && g4c::snapshot_slot(t, s.every, s.n_slots, slot))
        series = s.series + (long long)slot * n_points * F;
    const int n_chunks = (F + PS_CHUNK - 1) / PS_CHUNK;
    const long long items = n_points * n_chunks;
    const long long stride = (long long)gridDim.x * PS_THREADS;
    for (long long it = (long long)blockIdx.x * PS_THREADS + threadIdx.x; it < items; it += stride) {
        // (no contraction: every product is rounded to fp32 before it is added, so a plain numpy.float32 loop gives the same bits)
#pragma clang fp contract(off)
        const long long chunk = n_chunks == 1 ? 0 : it / n_points;          // (nf <= 4, the step's shape: no division)
        const long long p = it - chunk * n_points;
        const int c0 = (int)chunk * PS_CHUNK;
        const int width = F - c0 < PS_CHUNK ? F - c0 : PS_CHUNK;
        float acc[PS_CHUNK];
#pragma unroll
        for (int f = 0; f < PS_CHUNK; ++f) acc[f] = 0.f;
        // (four neighbours at a time: their index, coefficient and row loads are in flight together — the adds keep the order)
#pragma unroll 4
        for (int j = 0; j < k; ++j) {
            const long long at = (long long)j * n_points + p;
            const float c = s.coef[at];
            const float *row = x + (long long)s.idx[at] * s.x_ld + c0;
#pragma unroll
            for (int f = 0; f < PS_CHUNK; ++f) {
                if (f < width) {
                    const float pr = c * row[f];
                    acc[f] = j == 0 ? pr : acc[f] + pr;
                }
            }
        }
        const long long o = p * F + c0;
#pragma unroll
        for (int f = 0; f < PS_CHUNK; ++f) {
            if (f < width) {
                s.cur[o + f] = acc[f];
                if (series) series[o + f] = acc[f];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ adjoint
// gx[i, f] = Σ_{q in list(i)} in_coef[q] · gy[in_pt[q], f]: one thread per (node, chunk of PS_CHUNK columns), items chunk-major — item =
// chunk * N + i — so the lanes of a wave hold consecutive nodes of one chunk, and their lists lie one after the other in the tables.
// A node's list is walked by ONE thread in ascending position, whatever its length: a node that very many points use (a raster far
// finer than the mesh) makes its thread the launch's last; there is no second summation order for it.
__global__ __launch_bounds__(PS_THREADS) void sample_points_adjoint_kernel(const float *__restrict__ gy, const int *__restrict__ in_off,
                                                                          const int *__restrict__ in_pt, const float *__restrict__ in_coef,
                                                                          int F, long long n_nodes, float *__restrict__ gx) {
    const int n_chunks = (F + PS_CHUNK - 1) / PS_CHUNK;
    const long long items = n_nodes * n_chunks;
    const long long stride = (long long)gridDim.x * PS_THREADS;
    for (long long it = (long long)blockIdx.x * PS_THREADS + threadIdx.x; it < items; it += stride) {
#pragma clang fp contract(off)
        const long long chunk = n_chunks == 1 ? 0 : it / n_nodes;
        const long long i = it - chunk * n_nodes;
        const int c0 = (int)chunk * PS_CHUNK;
        const int width = F - c0 < PS_CHUNK ? F - c0 : PS_CHUNK;
        float acc[PS_CHUNK];
#pragma unroll
        for (int f = 0; f < PS_CHUNK; ++f) acc[f] = 0.f;
        if (in_off) {          // (no points: no tables, every row is +0)
            const int q0 = in_off[i], q1 = in_off[i + 1];
            // (four entries at a time: their point, coefficient and row loads are in flight together — the adds keep the order)
#pragma unroll 4
            for (int q = q0; q < q1; ++q) {
                const float c = in_coef[q];
                const float *row = gy + (long long)in_pt[q] * F + c0;
#pragma unroll
                for (int f = 0; f < PS_CHUNK; ++f) {
                    if (f < width) {
                        const float pr = c * row[f];
                        acc[f] = acc[f] + pr;
                    }
                }
            }
        }
        const long long o = i * F + c0;
#pragma unroll
        for (int f = 0; f < PS_CHUNK; ++f)
            if (f < width) gx[o + f] = acc[f];
    }
}

}  // namespace

extern "C" int g4c_sample_weights(const float *pos, const float *queries, const int32_t *idx, int32_t dim, int32_t power, int32_t k,
                                  int64_t n_nodes, int64_t n_points, float *coef, float *distance, uint8_t *degenerate, void *stream) {
    const char *me = "g4c_sample_weights";
    G4C_REQUIRE(n_nodes >= 0 && n_points >= 0 && k >= 1, G4C_EINVAL, "%s: bad sizes n_nodes=%lld n_points=%lld k=%d", me,
                (long long)n_nodes, (long long)n_points, k);
    G4C_REQUIRE(power >= 0 && power <= 2, G4C_EINVAL, "%s: power=%d (0, 1 or 2)", me, power);
    G4C_REQUIRE(dim == 2 || dim == 3, G4C_EUNSUPPORTED, "%s: dim=%d (2 or 3 are supported)", me, dim);
    G4C_REQUIRE(k <= PS_MAX_K, G4C_EUNSUPPORTED, "%s: k=%d neighbours (1 .. %d are supported)", me, k, PS_MAX_K);
    if (n_points == 0) return G4C_OK;
    G4C_REQUIRE(n_nodes >= k, G4C_EINVAL, "%s: k=%d neighbours of n_nodes=%lld", me, k, (long long)n_nodes);
    G4C_REQUIRE(pos && queries && idx && coef && distance && degenerate, G4C_EINVAL, "%s: null pointer", me);
    g4c::DeviceGuard on_device(pos);
    hipStream_t s = (hipStream_t)stream;
    const unsigned blocks = (unsigned)((n_points + PS_THREADS - 1) / PS_THREADS);
    if (dim == 2)
        sample_weights_kernel<2><<<dim3(blocks), dim3(PS_THREADS), 0, s>>>(pos, queries, idx, k, power, n_points, coef, distance, degenerate);
    else
        sample_weights_kernel<3><<<dim3(blocks), dim3(PS_THREADS), 0, s>>>(pos, queries, idx, k, power, n_points, coef, distance, degenerate);
    return g4c::check_launch(me);
}

extern "C" int g4c_sample_weights_periodic(const float *pos, const float *queries, const int32_t *idx, int32_t dim, int32_t power, int32_t k,
                                           int64_t n_nodes, int64_t n_points, const float *origin /*host[3]*/,
                                           const float *period /*host[3]*/, float *coef, float *distance, uint8_t *degenerate,
                                           void *stream) {
    const char *me = "g4c_sample_weights_periodic";
    G4C_REQUIRE(n_nodes >= 0 && n_points >= 0 && k >= 1, G4C_EINVAL, "%s: bad sizes n_nodes=%lld n_points=%lld k=%d", me,
                (long long)n_nodes, (long long)n_points, k);
    G4C_REQUIRE(power >= 0 && power <= 2, G4C_EINVAL, "%s: power=%d (0, 1 or 2)", me, power);
    G4C_REQUIRE(dim == 2 || dim == 3, G4C_EUNSUPPORTED, "%s: dim=%d (2 or 3 are supported)", me, dim);
    G4C_REQUIRE(k <= PS_MAX_K, G4C_EUNSUPPORTED, "%s: k=%d neighbours (1 .. %d are supported)", me, k, PS_MAX_K);
    G4C_REQUIRE(origin && period, G4C_EINVAL, "%s: null pointer", me);
    float o[3] = {0.f, 0.f, 0.f}, l[3] = {0.f, 0.f, 0.f};
    for (int a = 0; a < dim; ++a) {
        o[a] = origin[a];
        l[a] = period[a];
        G4C_REQUIRE(l[a] >= 0.f && l[a] < __builtin_inff() && (l[a] == 0.f || (o[a] == o[a] && fabsf(o[a]) < __builtin_inff())),
                    G4C_EINVAL, "%s: axis %d: period %g (0: not periodic) from origin %g", me, a, (double)l[a], (double)o[a]);
    }
    if (n_points == 0) return G4C_OK;
    G4C_REQUIRE(n_nodes >= k, G4C_EINVAL, "%s: k=%d neighbours of n_nodes=%lld", me, k, (long long)n_nodes);
    G4C_REQUIRE(pos && queries && idx && coef && distance && degenerate, G4C_EINVAL, "%s: null pointer", me);
    g4c::DeviceGuard on_device(pos);
    hipStream_t s = (hipStream_t)stream;
    const unsigned blocks = (unsigned)((n_points + PS_THREADS - 1) / PS_THREADS);
    if (dim == 2)
        sample_weights_periodic_kernel<2><<<dim3(blocks), dim3(PS_THREADS), 0, s>>>(pos, queries, idx, k, power, n_points, o[0], o[1], o[2],
                                                                                   l[0], l[1], l[2], coef, distance, degenerate);
    else
        sample_weights_periodic_kernel<3><<<dim3(blocks), dim3(PS_THREADS), 0, s>>>(pos, queries, idx, k, power, n_points, o[0], o[1], o[2],
                                                                                   l[0], l[1], l[2], coef, distance, degenerate);
    return g4c::check_launch(me);
}

extern "C" int g4c_sample_points(const float *x, const g4c_sample_points_t *sp, int64_t n_nodes, int64_t n_points, void *stream) {
    const char *me = "g4c_sample_points";
    G4C_REQUIRE(sp, G4C_EINVAL, "%s: null pointer", me);
    G4C_REQUIRE(n_nodes >= 0 && n_points >= 0 && sp->nf >= 1 && sp->k >= 1 && sp->x_ld >= 0 && sp->max_steps >= 0 && sp->every >= 0 &&
                    sp->n_slots >= 0,
                G4C_EINVAL, "%s: bad sizes n_nodes=%lld n_points=%lld nf=%d k=%d x_ld=%d max_steps=%d every=%d n_slots=%d", me,
                (long long)n_nodes, (long long)n_points, sp->nf, sp->k, sp->x_ld, sp->max_steps, sp->every, sp->n_slots);
    G4C_REQUIRE(sp->x_ld >= sp->nf, G4C_EINVAL, "%s: x_ld=%d < nf=%d", me, sp->x_ld, sp->nf);
    G4C_REQUIRE(sp->k <= PS_MAX_K, G4C_EUNSUPPORTED, "%s: k=%d neighbours (1 .. %d are supported)", me, sp->k, PS_MAX_K);
    G4C_REQUIRE(sp->every > 0 || !sp->series, G4C_EINVAL, "%s: a series buffer with every=0", me);
    G4C_REQUIRE(sp->step || !sp->series, G4C_EINVAL, "%s: a series without a step index", me);
    if (n_points == 0) return G4C_OK;
    G4C_REQUIRE(n_nodes >= sp->k, G4C_EINVAL, "%s: k=%d neighbours of n_nodes=%lld", me, sp->k, (long long)n_nodes);
    G4C_REQUIRE(x && sp->idx && sp->coef && sp->cur, G4C_EINVAL, "%s: null pointer", me);
    g4c::DeviceGuard on_device(x);
    hipStream_t s = (hipStream_t)stream;
    g4c_sample_points_t d = *sp;
    if (d.every == 0 || d.n_slots == 0) d.series = nullptr;
    const long long items = (long long)n_points * ((d.nf + PS_CHUNK - 1) / PS_CHUNK);
    sample_points_kernel<<<dim3((unsigned)g4c::blocks(items)), dim3(PS_THREADS), 0, s>>>(x, d, (long long)n_points);
    return g4c::check_launch(me);
}

extern "C" int g4c_sample_points_adjoint(const float *gy, const int32_t *in_off, const int32_t *in_pt, const float *in_coef, int32_t nf,
                                         int64_t n_nodes, int64_t n_points, float *gx, void *stream) {
    const char *me = "g4c_sample_points_adjoint";
    G4C_REQUIRE(n_nodes >= 0 && n_points >= 0 && nf >= 1, G4C_EINVAL, "%s: bad sizes n_nodes=%lld n_points=%lld nf=%d", me,
                (long long)n_nodes, (long long)n_points, nf);
    if (n_nodes == 0) return G4C_OK;
    G4C_REQUIRE(gx, G4C_EINVAL, "%s: null pointer", me);
    // (without points the tables and gy are empty and may have no address: gx is zero-filled)
    G4C_REQUIRE(n_points == 0 || (gy && in_off && in_pt && in_coef), G4C_EINVAL, "%s: null pointer", me);
    if (n_points > 0) {          // gx [n_nodes, nf] and gy [n_points, nf] must not share a byte: a thread reads rows of gy that other threads' rows of gx would cover
        const char *a = (const char *)gy, *b = (const char *)gx;
        const long long na = (long long)n_points * nf * 4ll, nb = (long long)n_nodes * nf * 4ll;
        G4C_REQUIRE(a + na <= b || b + nb <= a, G4C_EINVAL, "%s: gx aliases gy", me);
    }
    g4c::DeviceGuard on_device(gx);
    hipStream_t s = (hipStream_t)stream;
    if (n_points == 0) in_off = nullptr;
    const long long items = (long long)n_nodes * ((nf + PS_CHUNK - 1) / PS_CHUNK);
    sample_points_adjoint_kernel<<<dim3((unsigned)g4c::blocks(items)), dim3(PS_THREADS), 0, s>>>(gy, in_off, in_pt, in_coef, nf, (long long)n_nodes, gx);
    return g4c::check_launch(me);
}
