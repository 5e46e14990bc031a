// The step-record core under the per-step diagnostic launches of a rollout (records, derived fields, integrals, forces, samples,
// tracers, moments, spectra): the grid they share, the snapshot lattice, the scratch protocol between a launch and the one-workgroup
// launch behind it, and the workgroup reduction whose order is the diagnostics' public promise ("the step-record core").
#pragma once
#include "g4c_common.h"

namespace g4c {

// ------------------------------------------------------------------------------------------------------------------ grid
// Items are dealt to at most MAX_BLOCKS workgroups of THREADS (4 per CU on 256 CUs): beyond 262 144 items a thread takes several
// (gid, gid + grid, ...), and one partial set per workgroup stays a few hundred KB at any mesh size.  The grid — and with it the
// order of every sum — is a function of the item count alone.
constexpr int THREADS = 256;
constexpr int MAX_BLOCKS = 1024;

// (0 for no items: for the callers that return before they launch)
inline long long blocks(long long items) {
    const long long b = (items + THREADS - 1) / THREADS;
    return b > MAX_BLOCKS ? MAX_BLOCKS : b;
}
// (one workgroup for no items: for the callers whose launch has work besides the items, and for the size of their scratch)
inline long long blocks_or_one(long long items) {
    const long long b = blocks(items);
    return b < 1 ? 1 : b;
}

// ------------------------------------------------------------------------------------------------------------------ step clock
// Snapshots are taken on the lattice t = every - 1, 2 every - 1, ...: whether step t is on it and its slot is one of the n_slots.
// every > 0.  Which steps count at all (a range check on t, a buffer that may be absent) is the caller's own predicate.
__device__ __forceinline__ bool snapshot_slot(int t, int every, int n_slots, int &slot) {
    if ((t + 1) % every != 0) return false;
    slot = (t + 1) / every - 1;
    return slot < n_slots;
}

// ------------------------------------------------------------------------------------------------------------------ scratch protocol
// scratch: [0] the step index whose partials follow (-1: none — the step was outside the record), [1 .. 8) unused (the partials start
// on a 64-byte boundary), then [workgroup][n].  ONE thread of the first launch posts the step; the launch behind it on the same
// stream reads it back, and a step outside [0, max_steps) leaves stats untouched.
constexpr int HEADER = 8;

__device__ __forceinline__ double *partials(double *scratch, long long block, int n) { return scratch + HEADER + block * n; }
__device__ __forceinline__ const double *partials(const double *scratch, long long block, int n) { return scratch + HEADER + block * n; }

__device__ __forceinline__ void post_step(double *scratch, bool live, int t) { scratch[0] = live ? (double)t : -1.0; }
__device__ __forceinline__ bool posted_step(const double *scratch, int max_steps, int &t) {
    const double tt = scratch[0];
    if (!(tt >= 0.0 && tt < (double)max_steps)) return false;
    t = (int)tt;
    return true;
}

// ------------------------------------------------------------------------------------------------------------------ reduction
// What a workgroup reduces is a row of sets of NSTAT values (a set per field, column or entry).  Which positions of the row are
// NaN-true maxima (the rest are sums): none, or one of every set.
struct all_sums {
    static constexpr int NSTAT = 1;
    static constexpr bool is_max(int) { return false; }
};
template <int NSTAT_, int AT>
struct max_at {
    static constexpr int NSTAT = NSTAT_;
    static constexpr bool is_max(int j) { return j % NSTAT == AT; }
};

template <class POLICY>
__device__ __forceinline__ double combine(int j, double a, double b) {
    return POLICY::is_max(j) ? nan_max(a, b) : a + b;
}

// The workgroup's THREADS sets of n (<= N) values -> one set at dst.  A 6-level xor butterfly inside each wave (both lanes of a pair
// form the same commutative sum or maximum, so every lane ends with the wave's value), then the four waves in order: the order is
// fixed by the lane and wave numbers, never by arrival.  Everything stays in registers (the loops are unrolled over N and guarded by
// a wave-uniform test, so every index is a compile-time one) and 4 * N * 8 bytes of LDS.  A maximum carries a NaN at any item through
// every stage: nan_max in the caller's loop, between the four waves and over the partials of the workgroups, wave_nan_max in the
// butterfly.  After a NaN every lane of a wave holds the same canonical quiet NaN; of two NaNs of different waves or partials the
// one kept depends on the order of the arguments, which is fixed: two runs give the same bits.
template <class POLICY, int N>
__device__ __forceinline__ void block_reduce(double (&a)[N], int n, double *__restrict__ dst) {
    __shared__ double part[THREADS / 64][N];
#pragma unroll
    for (int j = 0; j < N; ++j) {
        if (j < n) a[j] = POLICY::is_max(j) ? wave_nan_max(a[j]) : wave_sum(a[j]);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int j = 0; j < N; ++j)
            if (j < n) part[wave][j] = a[j];
    }
    __syncthreads();
    if ((int)threadIdx.x < n) {
        const int j = threadIdx.x;
        double x = part[0][j];
#pragma unroll
        for (int w = 1; w < THREADS / 64; ++w) x = combine<POLICY>(j, x, part[w][j]);
        dst[j] = x;
    }
}

// The workgroups' partials -> stats[t], one workgroup, behind the launch that wrote them on the same stream (the launch boundary is
// what makes the partials visible: the alternative — the last workgroup under a fence — puts a write-back of every XCD's L2 into
// each of several hundred workgroups, which rollout_advance_kernel measured at twice this launch).  Thread i takes the partials of
// workgroups i, i + THREADS, ... in order, then block_reduce: the order depends on the number of workgroups alone.  stats[t] is
// overwritten.  The row has n_sets (<= SETS) sets; FULL: it has SETS, and the argument is not read.
template <class POLICY, int SETS, bool FULL>
__global__ __launch_bounds__(THREADS) void partials_kernel(const double *__restrict__ scratch, int n_blocks, int n_sets,
                                                           double *__restrict__ stats, int max_steps) {
    int t;
    if (!posted_step(scratch, max_steps, t)) return;
    constexpr int N = SETS * POLICY::NSTAT;
    const int n = (FULL ? SETS : n_sets) * POLICY::NSTAT;
    double acc[N];
#pragma unroll
    for (int j = 0; j < N; ++j) acc[j] = 0.0;
    for (int b = threadIdx.x; b < n_blocks; b += THREADS) {
        const double *q = partials(scratch, b, n);
#pragma unroll
        for (int j = 0; j < N; ++j)
            if (j < n) acc[j] = combine<POLICY>(j, acc[j], q[j]);
    }
    block_reduce<POLICY>(acc, n, stats + (long long)t * n);
}

}  // namespace g4c
