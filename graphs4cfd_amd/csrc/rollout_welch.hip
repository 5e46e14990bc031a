// Segment-averaged spectra of a rollout at every node (g4c_rollout_welch, include/g4c.h): Welch's estimator inside the step.  Two
// memory-bound launches per step between the forward and the step's closing launch.  The first adds the sample of the step to the one
// or two segments it belongs to — per segment the sums of g4c_rollout_spectrum (pivot, sum, re, im), kept in two alternating sets —,
// the second acts only on a step that ends a segment: it removes the segment's mean from its sums and adds the segment's power, and
// its cross-spectrum with a reference, to the averages.  It is a launch of its own because the reference may be another row's sums,
// finished by another workgroup of the first.  All fp64, plane-major, one add per accumulator and event, each accumulator owned by
// one thread: the bits depend on the data and the tables alone.  No sin / cos, no LDS, no scratch, nothing between workgroups.
#include "g4c_common.h"
#include "step_record.h"

// (no contraction anywhere in this file: every product is rounded to fp64 before it is added or subtracted, so a plain host loop gives
// the same bits)
#pragma clang fp contract(off)

namespace {

constexpr int WELCH_THREADS = g4c::THREADS;        // a launch takes g4c::blocks(n_nodes) workgroups a group of bins (step_record.h)
constexpr int WELCH_BINS = 8;                      // bins of one thread: blockIdx.y walks the groups, as in rollout_spectrum.hip
constexpr int WELCH_MAX_TRACK = 1024;

// What each kernel takes of the host's descriptor: the whole of it would sit in scalar registers for the life of the launch.
struct WelchLattice {
    int max_steps, stride, seg_len, hop, n_bins;
    int *window;
};
struct WelchAccumulate {
    WelchLattice on;
    const double *tw;          // (not a __restrict__ parameter of its own: the table's row then stays in vector registers, and no scalar register spills)
    int x_ld, x_step;
    long long plane_ld;
    double *pivot, *sum, *re, *im;
};
struct WelchClose {
    WelchLattice on;
    const double *W;
    double inv_L;
    long long plane_ld;
    const double *sum, *re, *im;
    double *pxx, *cxr_re, *cxr_im;
    const double *ref_sum, *ref_re, *ref_im;
    int ref_row, ref_field, n_track, max_segments;
    const int *track;
    double *seg_power;
};

// The sample index of the step on the lattice origin, origin + stride, ..., or -1 for a step that is off it.
__device__ __forceinline__ long long welch_sample(const WelchLattice &s, const int *__restrict__ step, int &t) {
    t = step[0];
    const int origin = s.window[0];
    if (t < 0 || t >= s.max_steps || t < origin || (t - origin) % s.stride != 0) return -1;
    return (t - origin) / s.stride;
}

// The rows of one thread for the KN bins k0 .. k0 + KN - 1 of the segment kept in `set`, at position q of the segment.  `lead` (the
// first bin group) also owns pivot and sum.
template <int KN>
__device__ __forceinline__ void welch_rows(const float *__restrict__ x, const WelchAccumulate &s, int nf, int k0, int set, long long q,
                                           long long x_off, bool lead, long long n_nodes) {
    // row q of the table, wave-uniform and read before any store
    double c[KN], sn[KN];
    const int K = s.on.n_bins;
    const double *row = s.tw + (q * K + k0) * 2;
#pragma unroll
    for (int k = 0; k < KN; ++k) {
        c[k] = row[2 * k];
        sn[k] = row[2 * k + 1];
    }
    const long long ld = s.plane_ld;
    const long long stride = (long long)gridDim.x * WELCH_THREADS;
    for (long long n = (long long)blockIdx.x * WELCH_THREADS + threadIdx.x; n < n_nodes; n += stride) {
        const float *xr = x + n * s.x_ld + x_off;
        for (int f = 0; f < nf; ++f) {
            const double xf = (double)xr[f];
            const long long pf = (long long)set * nf + f;
            double *re = s.re + (pf * K + k0) * ld + n;
            double *im = s.im + (pf * K + k0) * ld + n;
            if (q == 0) {
                if (lead) {
                    s.pivot[pf * ld + n] = xf;
                    s.sum[pf * ld + n] = 0.0;
                }
#pragma unroll
                for (int k = 0; k < KN; ++k) {
                    re[k * ld] = 0.0;
                    im[k * ld] = 0.0;
                }
            } else {
                // every load of the field first, then every store (the planes are not declared disjoint)
                double r[KN], i[KN], sm = 0.0;
                const double d = xf - s.pivot[pf * ld + n];
                if (lead) sm = s.sum[pf * ld + n];
#pragma unroll
                for (int k = 0; k < KN; ++k) {
                    r[k] = re[k * ld];
                    i[k] = im[k * ld];
                }
                if (lead) s.sum[pf * ld + n] = sm + d;
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

__global__ __launch_bounds__(WELCH_THREADS) void rollout_welch_accumulate_kernel(const float *__restrict__ x, const WelchAccumulate s,
                                                                                const int *__restrict__ step, int nf, long long n_nodes) {
    int t;
    const long long j = welch_sample(s.on, step, t);
    if (j < 0) return;          // every address below is formed from a checked t; a step off the lattice touches nothing
    const long long x_off = (long long)s.x_step * t;
    const int k0 = blockIdx.y * WELCH_BINS;
    const int kn = s.on.n_bins - k0 < WELCH_BINS ? s.on.n_bins - k0 : WELCH_BINS;
    const bool lead = blockIdx.y == 0;
    // sample j is position q of segment seg (q < hop <= seg_len) and, with half-overlapping segments, position q + hop of the one before
    const long long seg = j / s.on.hop, q0 = j - seg * s.on.hop;
    const int passes = (s.on.hop < s.on.seg_len && seg >= 1) ? 2 : 1;
    for (int pass = 0; pass < passes; ++pass) {
        const int set = (int)((seg - pass) & 1);
        const long long q = q0 + (pass ? s.on.hop : 0);
        switch (kn) {          // (uniform over the workgroup)
            case 1: welch_rows<1>(x, s, nf, k0, set, q, x_off, lead, n_nodes); break;
            case 2: welch_rows<2>(x, s, nf, k0, set, q, x_off, lead, n_nodes); break;
            case 3: welch_rows<3>(x, s, nf, k0, set, q, x_off, lead, n_nodes); break;
            case 4: welch_rows<4>(x, s, nf, k0, set, q, x_off, lead, n_nodes); break;
            case 5: welch_rows<5>(x, s, nf, k0, set, q, x_off, lead, n_nodes); break;
            case 6: welch_rows<6>(x, s, nf, k0, set, q, x_off, lead, n_nodes); break;
            case 7: welch_rows<7>(x, s, nf, k0, set, q, x_off, lead, n_nodes); break;
            default: welch_rows<8>(x, s, nf, k0, set, q, x_off, lead, n_nodes); break;
        }
    }
    // nothing in the launch reads `last`: no ordering between workgroups is needed
    if (lead && blockIdx.x == 0 && threadIdx.x == 0) s.on.window[1] = t;
}

// The mode of one field and bin of a finished segment with the segment's mean removed: (re, im) - m (W_k0, W_k1).
__device__ __forceinline__ void welch_mode(double m, double re, double im, double w0, double w1, double &ar, double &ai) {
    const double mr = m * w0;
    const double mi = m * w1;
    ar = re - mr;
    ai = im - mi;
}

__device__ __forceinline__ double welch_power(double ar, double ai) {
    const double p0 = ar * ar;
    const double p1 = ai * ai;
    return p0 + p1;
}

// It runs once per hop, and a thread keeps one bin at a time: plain loops over the fields and the bins of the group.
__global__ __launch_bounds__(WELCH_THREADS) void rollout_welch_close_kernel(const WelchClose s, const int *__restrict__ step, int nf,
                                                                           long long n_nodes) {
    int t;
    const long long j = welch_sample(s.on, step, t);
    // only the last sample of a segment closes it: a last partial segment is never closed
    if (j < s.on.seg_len - 1 || (j - (s.on.seg_len - 1)) % s.on.hop != 0) return;
    const long long seg = (j - (s.on.seg_len - 1)) / s.on.hop;
    const long long set = seg & 1;
    const bool first = seg == 0;          // segment 0 stores the averages, later ones add: no memset is ever needed
    const int K = s.on.n_bins;
    const int k0 = blockIdx.y * WELCH_BINS;
    const int k1 = K - k0 < WELCH_BINS ? K : k0 + WELCH_BINS;
    const long long ld = s.plane_ld;
    const long long stride = (long long)gridDim.x * WELCH_THREADS;
    const bool with_ref = s.ref_sum != nullptr;
    for (long long n = (long long)blockIdx.x * WELCH_THREADS + threadIdx.x; n < n_nodes; n += stride) {
        const long long rn = s.ref_row >= 0 ? (long long)s.ref_row : n;
        for (int f = 0; f < nf; ++f) {
            const long long pf = set * nf + f;
            const long long rf = set * nf + (s.ref_field >= 0 ? s.ref_field : f);
            const double m = s.sum[pf * ld + n] * s.inv_L;
            const double mref = with_ref ? s.ref_sum[rf * ld + rn] * s.inv_L : 0.0;
#pragma nounroll
            for (int k = k0; k < k1; ++k) {
                const double w0 = s.W[2 * k], w1 = s.W[2 * k + 1];          // (wave-uniform)
                double ar, ai;
                welch_mode(m, s.re[(pf * K + k) * ld + n], s.im[(pf * K + k) * ld + n], w0, w1, ar, ai);
                const double p = welch_power(ar, ai);
                const long long at = ((long long)f * K + k) * ld + n;
                s.pxx[at] = first ? p : s.pxx[at] + p;
                if (!with_ref) continue;
                double rr, ri;
                welch_mode(mref, s.ref_re[(rf * K + k) * ld + rn], s.ref_im[(rf * K + k) * ld + rn], w0, w1, rr, ri);
                const double a = ar * rr;          // X conj(R)
                const double b = ai * ri;
                const double c = ai * rr;
                const double d = ar * ri;
                const double cr = a + b;
                const double ci = c - d;
                s.cxr_re[at] = first ? cr : s.cxr_re[at] + cr;
                s.cxr_im[at] = first ? ci : s.cxr_im[at] + ci;
            }
        }
    }
    // the segment's raw power at the tracked rows, formed again from the segment's sums (the same operations: the same bits)
    if (seg < s.max_segments) {
        for (long long p = (long long)blockIdx.x * WELCH_THREADS + threadIdx.x; p < s.n_track; p += stride) {
            const long long n = s.track[p];
            if (n < 0 || n >= n_nodes) continue;          // (refused on the host; never an address)
            double *out = s.seg_power + ((seg * s.n_track + p) * nf) * K;
            for (int f = 0; f < nf; ++f) {
                const long long pf = set * nf + f;
                const double m = s.sum[pf * ld + n] * s.inv_L;
#pragma nounroll
                for (int k = k0; k < k1; ++k) {
                    double ar, ai;
                    welch_mode(m, s.re[(pf * K + k) * ld + n], s.im[(pf * K + k) * ld + n], s.W[2 * k], s.W[2 * k + 1], ar, ai);
                    out[(long long)f * K + k] = welch_power(ar, ai);
                }
            }
        }
    }
    if (blockIdx.y == 0 && blockIdx.x == 0 && threadIdx.x == 0) s.on.window[2] = (int)(seg + 1);
}

}  // namespace

extern "C" int g4c_rollout_welch(const float *x, int32_t nf, const g4c_rollout_welch_t *s, const int32_t *step, int64_t n_nodes, void *stream) {
    const char *me = "g4c_rollout_welch";
    G4C_REQUIRE(s && step, G4C_EINVAL, "%s: null pointer", me);
    G4C_REQUIRE(nf >= 1 && s->n_bins >= 1 && n_nodes >= 0 && s->max_steps >= 0, G4C_EINVAL, "%s: bad sizes nf=%d n_bins=%d n_nodes=%lld max_steps=%d",
                me, nf, s->n_bins, (long long)n_nodes, s->max_steps);
    G4C_REQUIRE(s->stride >= 1, G4C_EINVAL, "%s: stride=%d (>= 1)", me, s->stride);
    G4C_REQUIRE(s->seg_len >= 2, G4C_EINVAL, "%s: seg_len=%d (>= 2)", me, s->seg_len);
    G4C_REQUIRE(s->hop >= 1 && (s->hop == s->seg_len || 2 * s->hop == s->seg_len), G4C_EUNSUPPORTED,
                "%s: hop=%d of segments of seg_len=%d samples (seg_len: no overlap, or seg_len / 2 with an even seg_len)", me, s->hop, s->seg_len);
    G4C_REQUIRE(s->window && s->tw && s->W, G4C_EINVAL, "%s: null pointer (window, tw, W)", me);
    G4C_REQUIRE(s->x_ld >= nf, G4C_EINVAL, "%s: x_ld=%d < nf=%d", me, s->x_ld, nf);
    G4C_REQUIRE(s->x_step == 0 || s->x_step == nf, G4C_EINVAL, "%s: x_step=%d (0: the prediction, nf=%d: a target's columns of the step)", me,
                s->x_step, nf);
    if (s->x_step)
        G4C_REQUIRE((long long)s->x_ld >= (long long)nf * s->max_steps, G4C_EINVAL, "%s: x_ld=%d < nf * max_steps = %lld with x_step=%d", me,
                    s->x_ld, (long long)nf * s->max_steps, s->x_step);
    const bool with_ref = s->ref_sum || s->ref_re || s->ref_im || s->cxr_re || s->cxr_im;
    if (with_ref) {
        G4C_REQUIRE(s->ref_sum && s->ref_re && s->ref_im && s->cxr_re && s->cxr_im, G4C_EINVAL,
                    "%s: a reference needs ref_sum, ref_re, ref_im, cxr_re and cxr_im", me);
        G4C_REQUIRE(s->ref_row < n_nodes || n_nodes == 0, G4C_EINVAL, "%s: ref_row=%d of n_nodes=%lld", me, s->ref_row, (long long)n_nodes);
        G4C_REQUIRE(s->ref_field < nf, G4C_EINVAL, "%s: ref_field=%d of nf=%d", me, s->ref_field, nf);
    }
    G4C_REQUIRE(s->n_track >= 0 && s->max_segments >= 0, G4C_EINVAL, "%s: n_track=%d max_segments=%d", me, s->n_track, s->max_segments);
    G4C_REQUIRE(s->n_track <= WELCH_MAX_TRACK, G4C_EUNSUPPORTED, "%s: n_track=%d tracked rows (at most %d)", me, s->n_track, WELCH_MAX_TRACK);
    if (s->n_track > 0) {
        G4C_REQUIRE(s->track && s->track_host && (s->seg_power || s->max_segments == 0), G4C_EINVAL,
                    "%s: tracked rows need track, track_host and seg_power", me);
        for (int p = 0; p < s->n_track; ++p)
            G4C_REQUIRE(s->track_host[p] >= 0 && s->track_host[p] < n_nodes, G4C_EINVAL, "%s: track[%d]=%d of n_nodes=%lld", me, p,
                        s->track_host[p], (long long)n_nodes);
    }
    if (n_nodes > 0) {        // (no nodes: x and the accumulators are empty and have no address)
        G4C_REQUIRE(x && s->pivot && s->sum && s->re && s->im && s->pxx, G4C_EINVAL, "%s: null pointer", me);
        G4C_REQUIRE(s->plane_ld >= n_nodes, G4C_EINVAL, "%s: plane_ld=%lld < n_nodes=%lld", me, (long long)s->plane_ld, (long long)n_nodes);
    }
    G4C_REQUIRE(nf <= 8, G4C_EUNSUPPORTED, "%s: spectra of nf=%d fields (1 .. 8 are supported)", me, nf);
    G4C_REQUIRE(s->n_bins <= 64, G4C_EUNSUPPORTED, "%s: n_bins=%d frequencies (1 .. 64 are supported)", me, s->n_bins);
    if (n_nodes == 0) return G4C_OK;
    g4c::DeviceGuard on_device(step);
    const long long b = g4c::blocks(n_nodes);
    const unsigned groups = (unsigned)((s->n_bins + WELCH_BINS - 1) / WELCH_BINS);
    const WelchLattice on{s->max_steps, s->stride, s->seg_len, s->hop, s->n_bins, s->window};
    const WelchAccumulate acc{on, s->tw, s->x_ld, s->x_step, s->plane_ld, s->pivot, s->sum, s->re, s->im};
    const WelchClose cl{on,         s->W,      s->inv_L,   s->plane_ld, s->sum,       s->re,      s->im,           s->pxx,   s->cxr_re,   s->cxr_im,
                        s->ref_sum, s->ref_re, s->ref_im,  s->ref_row,  s->ref_field, s->n_track, s->max_segments, s->track, s->seg_power};
    rollout_welch_accumulate_kernel<<<dim3((unsigned)b, groups), dim3(WELCH_THREADS), 0, (hipStream_t)stream>>>(x, acc, step, nf, n_nodes);
    if (int rc = g4c::check_launch(me)) return rc;
    rollout_welch_close_kernel<<<dim3((unsigned)b, groups), dim3(WELCH_THREADS), 0, (hipStream_t)stream>>>(cl, step, nf, n_nodes);
    return g4c::check_launch(me);
}
