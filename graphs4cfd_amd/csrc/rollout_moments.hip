// Time statistics of a rollout at every node (g4c_rollout_moments, include/g4c.h): one memory-bound launch per step between the forward
// and the step's closing launch.  It reads the prediction (and, for the statistics of the error, the target's columns of the step),
// and keeps per node and field a pivot (the first sample), the sum of the shifted samples, the sums of their pairwise products, and
// the extrema — all fp64, plane-major, one add per accumulator and accumulated step, each accumulator owned by one thread: the bits
// depend on the data alone.  No LDS, no scratch, nothing between workgroups.  The extrema carry a NaN sample (g4c::nan_min / nan_max)
// and keep it until the window's origin is rewritten.
#include "g4c_common.h"
#include "step_record.h"

namespace {

constexpr int MOM_THREADS = g4c::THREADS;          // a launch takes g4c::blocks(n_nodes) workgroups (step_record.h)

template <int NF, bool SUB>
__global__ __launch_bounds__(MOM_THREADS) void rollout_moments_kernel(const float *__restrict__ pred, const g4c_rollout_moments_t m,
                                                                     const int *__restrict__ step, long long n_nodes) {
    const int t = step[0];
    const int origin = m.window[0];
    // every address below is formed from a checked t; an off-window step touches nothing
    if (t < 0 || t >= m.max_steps || t < origin || (t - origin) % m.stride != 0) return;
    const bool first = t == origin;
    const long long ld = m.plane_ld;
    const long long stride = (long long)gridDim.x * MOM_THREADS;
    const long long gid = (long long)blockIdx.x * MOM_THREADS + threadIdx.x;
    for (long long n = gid; n < n_nodes; n += stride) {
        // (no contraction in this block: d_f * d_g is rounded to fp64 before it is added, so a plain host loop gives the same bits)
#pragma clang fp contract(off)
        double x[NF];
        const float *pr = pred + n * NF;
#pragma unroll
        for (int f = 0; f < NF; ++f) x[f] = (double)pr[f];
        if constexpr (SUB) {
            const float *sr = m.sub + n * m.sub_ld + (long long)NF * t;
#pragma unroll
            for (int f = 0; f < NF; ++f) x[f] -= (double)sr[f];
        }
        if (first) {
#pragma unroll
            for (int f = 0; f < NF; ++f) {
                m.pivot[f * ld + n] = x[f];
                m.sum[f * ld + n] = 0.0;
                m.lo[f * ld + n] = x[f];
                m.hi[f * ld + n] = x[f];
            }
#pragma unroll
            for (int p = 0; p < NF * (NF + 1) / 2; ++p) m.sum2[p * ld + n] = 0.0;
        } else {
            // every load first, then every store (the planes are not declared disjoint: interleaved, each load would wait for the
            // store before it)
            double d[NF], s[NF], lo[NF], hi[NF], s2[NF * (NF + 1) / 2];
#pragma unroll
            for (int f = 0; f < NF; ++f) {
                d[f] = m.pivot[f * ld + n];
                s[f] = m.sum[f * ld + n];
                lo[f] = m.lo[f * ld + n];
                hi[f] = m.hi[f * ld + n];
            }
#pragma unroll
            for (int p = 0; p < NF * (NF + 1) / 2; ++p) s2[p] = m.sum2[p * ld + n];
#pragma unroll
            for (int f = 0; f < NF; ++f) {
                d[f] = x[f] - d[f];
                m.sum[f * ld + n] = s[f] + d[f];
                m.lo[f * ld + n] = g4c::nan_min(lo[f], x[f]);
                m.hi[f * ld + n] = g4c::nan_max(hi[f], x[f]);
            }
            int p = 0;
#pragma unroll
            for (int f = 0; f < NF; ++f) {
#pragma unroll
                for (int g = f; g < NF; ++g, ++p) {
                    const double prod = d[f] * d[g];
                    m.sum2[p * ld + n] = s2[p] + prod;
                }
            }
        }
    }
    // nothing in the launch reads `last`: no ordering between workgroups is needed
    if (gid == 0) m.window[1] = t;
}

template <int NF>
void mom_launch(const float *pred, const g4c_rollout_moments_t &m, const int *step, long long n_nodes, hipStream_t s) {
    const long long b = g4c::blocks(n_nodes);
    if (m.sub)
        rollout_moments_kernel<NF, true><<<dim3((unsigned)b), dim3(MOM_THREADS), 0, s>>>(pred, m, step, n_nodes);
    else
        rollout_moments_kernel<NF, false><<<dim3((unsigned)b), dim3(MOM_THREADS), 0, s>>>(pred, m, step, n_nodes);
}

}  // namespace

extern "C" int g4c_rollout_moments(const float *pred, int32_t nf, const g4c_rollout_moments_t *m, const int32_t *step, int64_t n_nodes,
                                   void *stream) {
    const char *me = "g4c_rollout_moments";
    G4C_REQUIRE(m && step, G4C_EINVAL, "%s: null pointer", me);
    G4C_REQUIRE(nf >= 1 && n_nodes >= 0 && m->max_steps >= 0, G4C_EINVAL, "%s: bad sizes nf=%d n_nodes=%lld max_steps=%d", me, nf,
                (long long)n_nodes, m->max_steps);
    G4C_REQUIRE(m->stride >= 1, G4C_EINVAL, "%s: stride=%d (>= 1)", me, m->stride);
    G4C_REQUIRE(m->window, G4C_EINVAL, "%s: null pointer (window)", me);
    if (m->sub)
        G4C_REQUIRE((long long)m->sub_ld >= (long long)nf * m->max_steps, G4C_EINVAL, "%s: sub_ld=%d < nf * max_steps = %lld", me, m->sub_ld,
                    (long long)nf * m->max_steps);
    if (n_nodes > 0) {        // (no nodes: pred and the accumulators are empty and have no address)
        G4C_REQUIRE(pred && m->pivot && m->sum && m->sum2 && m->lo && m->hi, G4C_EINVAL, "%s: null pointer", me);
        G4C_REQUIRE(m->plane_ld >= n_nodes, G4C_EINVAL, "%s: plane_ld=%lld < n_nodes=%lld", me, (long long)m->plane_ld, (long long)n_nodes);
    }
    G4C_REQUIRE(nf <= 8, G4C_EUNSUPPORTED, "%s: statistics of nf=%d fields (1 .. 8 are supported)", me, nf);
    if (n_nodes == 0) return G4C_OK;
    g4c::DeviceGuard on_device(step);
    hipStream_t s = (hipStream_t)stream;
    switch (nf) {
        case 1: mom_launch<1>(pred, *m, step, n_nodes, s); break;
        case 2: mom_launch<2>(pred, *m, step, n_nodes, s); break;
        case 3: mom_launch<3>(pred, *m, step, n_nodes, s); break;
        case 4: mom_launch<4>(pred, *m, step, n_nodes, s); break;
        case 5: mom_launch<5>(pred, *m, step, n_nodes, s); break;
        case 6: mom_launch<6>(pred, *m, step, n_nodes, s); break;
        case 7: mom_launch<7>(pred, *m, step, n_nodes, s); break;
        default: mom_launch<8>(pred, *m, step, n_nodes, s); break;
    }
    return g4c::check_launch(me);
}
