// Fourier modes of a rollout at every node (g4c_rollout_spectrum, include/g4c.h): one memory-bound launch per step between the forward
// and the step's closing launch.  It reads the sample of the step (the prediction, or a target's columns of the step) and keeps per
// node and field a pivot (the first sample), the sum of the shifted samples and, for each of K bins, the sums of the shifted samples
// times the two entries of a host-built twiddle table — all fp64, plane-major, one add per accumulator and accumulated step, each
// accumulator owned by one thread: the bits depend on the data and the table alone.  No sin / cos, no LDS, no scratch, nothing
// between workgroups.
#include "g4c_common.h"
#include "step_record.h"

namespace {

constexpr int SPEC_THREADS = g4c::THREADS;          // a launch takes g4c::blocks(n_nodes) workgroups a group of bins (step_record.h)
// bins of one thread: blockIdx.y walks the groups of SPEC_BINS bins (the last one may be shorter), so a 10k-node mesh with K = 32
// still has 160 workgroups, and a thread holds 2 * SPEC_BINS accumulators of one field between its loads and its stores
constexpr int SPEC_BINS = 8;

// The rows of one thread for the KN bins k0 .. k0 + KN - 1.  `lead` (the first bin group) also owns pivot and sum.
template <int KN>
__device__ __forceinline__ void spectrum_rows(const float *__restrict__ x, const g4c_rollout_spectrum_t &s, const double *__restrict__ tw, int nf,
                                              int k0, long long j, long long x_off, bool lead, long long n_nodes) {
    // row j of the table, wave-uniform and read before any store: KN pairs through the scalar cache
    double c[KN], sn[KN];
    const double *row = tw + (j * s.n_bins + k0) * 2;
#pragma unroll
    for (int k = 0; k < KN; ++k) {
        c[k] = row[2 * k];
        sn[k] = row[2 * k + 1];
    }
    const long long ld = s.plane_ld;
    const long long stride = (long long)gridDim.x * SPEC_THREADS;
    for (long long n = (long long)blockIdx.x * SPEC_THREADS + threadIdx.x; n < n_nodes; n += stride) {
        const float *xr = x + n * s.x_ld + x_off;
        for (int f = 0; f < nf; ++f) {
            // (no contraction in this block: d * tw is rounded to fp64 before it is added, so a plain host loop gives the same bits)
#pragma clang fp contract(off)
            const double xf = (double)xr[f];
            double *re = s.re + ((long long)f * s.n_bins + k0) * ld + n;
            double *im = s.im + ((long long)f * s.n_bins + k0) * ld + n;
            if (j == 0) {
                if (lead) {
                    s.pivot[f * ld + n] = xf;
                    s.sum[f * ld + n] = 0.0;
                }
#pragma unroll
                for (int k = 0; k < KN; ++k) {
                    re[k * ld] = 0.0;
                    im[k * ld] = 0.0;
                }
            } else {
                // every load of the field first, then every store (the planes are not declared disjoint: interleaved, each load
                // would wait for the store before it)
                double r[KN], i[KN], sm = 0.0;
                const double d = xf - s.pivot[f * ld + n];
                if (lead) sm = s.sum[f * ld + n];
#pragma unroll
                for (int k = 0; k < KN; ++k) {
                    r[k] = re[k * ld];
                    i[k] = im[k * ld];
                }
                if (lead) s.sum[f * ld + n] = sm + d;
#pragma unroll
                for (int k = 0; k < KN; ++k) {
                    const double pr = d * c[k];
                    const double pi = d * sn[k];
                    re[k * ld] = r[k] + pr;
                    im[k * ld] = i[k] + pi;
                }
            }
        }
    }
}

__global__ __launch_bounds__(SPEC_THREADS) void rollout_spectrum_kernel(const float *__restrict__ x, const g4c_rollout_spectrum_t s,
                                                                       const double *__restrict__ tw, const int *__restrict__ step, int nf,
                                                                       long long n_nodes) {
    const int t = step[0];
    const int origin = s.window[0];
    // every address below is formed from a checked t; an off-window step touches nothing
    if (t < 0 || t >= s.max_steps || t < origin || (t - origin) % s.stride != 0) return;
    const long long j = (t - origin) / s.stride;
    if (j >= s.n_samples) return;
    const int k0 = blockIdx.y * SPEC_BINS;
    const int kn = s.n_bins - k0 < SPEC_BINS ? s.n_bins - k0 : SPEC_BINS;
    const long long x_off = (long long)s.x_step * t;
    const bool lead = blockIdx.y == 0;
    switch (kn) {          // (uniform over the workgroup)
        case 1: spectrum_rows<1>(x, s, tw, nf, k0, j, x_off, lead, n_nodes); break;
        case 2: spectrum_rows<2>(x, s, tw, nf, k0, j, x_off, lead, n_nodes); break;
        case 3: spectrum_rows<3>(x, s, tw, nf, k0, j, x_off, lead, n_nodes); break;
        case 4: spectrum_rows<4>(x, s, tw, nf, k0, j, x_off, lead, n_nodes); break;
        case 5: spectrum_rows<5>(x, s, tw, nf, k0, j, x_off, lead, n_nodes); break;
        case 6: spectrum_rows<6>(x, s, tw, nf, k0, j, x_off, lead, n_nodes); break;
        case 7: spectrum_rows<7>(x, s, tw, nf, k0, j, x_off, lead, n_nodes); break;
        default: spectrum_rows<8>(x, s, tw, nf, k0, j, x_off, lead, n_nodes); break;
    }
    // nothing in the launch reads `last`: no ordering between workgroups is needed
    if (lead && blockIdx.x == 0 && threadIdx.x == 0) s.window[1] = t;
}

}  // namespace

extern "C" int g4c_rollout_spectrum(const float *x, int32_t nf, const g4c_rollout_spectrum_t *s, const int32_t *step, int64_t n_nodes,
                                    void *stream) {
    const char *me = "g4c_rollout_spectrum";
    G4C_REQUIRE(s && step, G4C_EINVAL, "%s: null pointer", me);
    G4C_REQUIRE(nf >= 1 && s->n_bins >= 1 && n_nodes >= 0 && s->max_steps >= 0, G4C_EINVAL, "%s: bad sizes nf=%d n_bins=%d n_nodes=%lld max_steps=%d",
                me, nf, s->n_bins, (long long)n_nodes, s->max_steps);
    G4C_REQUIRE(s->stride >= 1, G4C_EINVAL, "%s: stride=%d (>= 1)", me, s->stride);
    G4C_REQUIRE(s->n_samples >= 1, G4C_EINVAL, "%s: n_samples=%d (>= 1)", me, s->n_samples);
    G4C_REQUIRE(s->window && s->tw, G4C_EINVAL, "%s: null pointer (window, tw)", me);
    G4C_REQUIRE(s->x_ld >= nf, G4C_EINVAL, "%s: x_ld=%d < nf=%d", me, s->x_ld, nf);
    G4C_REQUIRE(s->x_step == 0 || s->x_step == nf, G4C_EINVAL, "%s: x_step=%d (0: the prediction, nf=%d: a target's columns of the step)", me,
                s->x_step, nf);
    if (s->x_step)
        G4C_REQUIRE((long long)s->x_ld >= (long long)nf * s->max_steps, G4C_EINVAL, "%s: x_ld=%d < nf * max_steps = %lld with x_step=%d", me,
                    s->x_ld, (long long)nf * s->max_steps, s->x_step);
    if (n_nodes > 0) {        // (no nodes: x and the accumulators are empty and have no address)
        G4C_REQUIRE(x && s->pivot && s->sum && s->re && s->im, G4C_EINVAL, "%s: null pointer", me);
        G4C_REQUIRE(s->plane_ld >= n_nodes, G4C_EINVAL, "%s: plane_ld=%lld < n_nodes=%lld", me, (long long)s->plane_ld, (long long)n_nodes);
    }
    G4C_REQUIRE(nf <= 8, G4C_EUNSUPPORTED, "%s: spectra of nf=%d fields (1 .. 8 are supported)", me, nf);
    G4C_REQUIRE(s->n_bins <= 64, G4C_EUNSUPPORTED, "%s: n_bins=%d frequencies (1 .. 64 are supported)", me, s->n_bins);
    if (n_nodes == 0) return G4C_OK;
    g4c::DeviceGuard on_device(step);
    const long long b = g4c::blocks(n_nodes);
    const unsigned groups = (unsigned)((s->n_bins + SPEC_BINS - 1) / SPEC_BINS);
    rollout_spectrum_kernel<<<dim3((unsigned)b, groups), dim3(SPEC_THREADS), 0, (hipStream_t)stream>>>(x, *s, s->tw, step, nf, n_nodes);
    return g4c::check_launch(me);
}
