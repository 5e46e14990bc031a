// The per-point device routines of the periodic searches (knn_periodic.hip, point_sample.hip, tracer.hip), as templates (inlined):
//   wrap_coordinate            the fixed fp32 sequence that brings a query into [o, o + L) (include/g4c.h, g4c_periodic_grid_t);
//   wrapped_offset             t = p − q with connect_knn's rule: t − L if t > L/2, t + L if t < −L/2 (strict), in fp64;
//   periodic_cell              the cell of a coordinate along one axis, clamped as a double before it becomes an integer;
//   knn_ring_search_periodic   the exact ring search in the wrapped metric.  It is NOT folded into knn_ring_search (point_fit.h) or
//                              knn_grid_kernel (knn_grid.hip): those keep their bodies and their registers.
#pragma once
#include "g4c_common.h"

namespace g4c {

// q brought into [o, o + L): f = floorf((q − o) / L), q' = q − f L (the product rounded before the subtraction), then q' + L if
// q' < o, then q' − L if q' >= o + L (o + L rounded to fp32).  Every operation is one fp32 rounding; nothing is contracted.
__device__ __forceinline__ float wrap_coordinate(float q, float o, float L) {
#pragma clang fp contract(off)
    const float rel = q - o;
    const float f = floorf(rel / L);
    const float fl = f * L;
    float w = q - fl;
    if (w < o) w = w + L;
    const float top = o + L;
    if (w >= top) w = w - L;
    // The result is ALWAYS finite: where the sequence gives no finite number (q is not finite, or q − o, (q − o) / L or f L overflows —
    // with L < 1 a finite |q − o| above FLT_MAX L does), the result is o.  A search from a wrapped coordinate therefore has finite
    // distances to every point and returns k candidates whenever the cloud holds k: no index −1 forms an address.  Beyond |q − o| ~
    // 2^24 L the rounded product f L is whole periods away from q and the result, though finite, lies outside [o, o + L): the wrap is
    // exact to the fp32 resolution of (q − o) / L, not beyond.
    if (!(fabsf(w) < __builtin_inff())) w = o;          // (NaN included)
    return w;
}

// Whether the sequence above reaches a finite number by itself (false: wrap_coordinate answers o).  The tracers stop a particle whose
// position does not wrap (G4C_TRACER_NONFINITE) instead of carrying it to the origin.
__device__ __forceinline__ bool wraps_finite(float q, float o, float L) {
#pragma clang fp contract(off)
    const float rel = q - o;
    const float f = floorf(rel / L);
    const float fl = f * L;
    const float w = q - fl;
    return fabsf(w) < __builtin_inff() && fabsf(fl) < __builtin_inff();
}

__device__ __forceinline__ double wrapped_offset(double t, double L) {          // L > 0
    const double half = 0.5 * L;
    if (t > half) t -= L;
    else if (t < -half) t += L;
    return t;
}

__device__ __forceinline__ int periodic_cell(double q, float origin, double cell, int nc) {
    double cc = floor((q - (double)origin) / cell);
    cc = fmin(fmax(cc, 0.0), (double)(nc - 1));          // (a NaN becomes cell 0: no position, however wild, forms an address)
    return (int)cc;
}

// The k nearest points of q in the wrapped metric among the cell-sorted cloud `pos` (cell_start: first sorted point of each cell),
// nearest first, into best_d / best_j[0 .. k − 1] (squared fp64 distances, SORTED indices; −1 where the cloud has fewer than k points).
// Axis a is periodic when per[a] > 0 (its length L_a; the grid tiles it exactly: nc_a cells of h_a = L_a / nc_a from org[a]); another
// axis is searched as knn_ring_search does.  c: the cell of q (periodic_cell).  SELF: q is sorted point `self`, which is skipped.
//
// Ring R scans, along a periodic axis, the min(2R + 1, nc_a) distinct cells c_a − R .. c_a + R modulo nc_a, each once (on the fastest
// axis: one or two contiguous runs of sorted points); along another axis the cells c_a − R .. c_a + R clipped to the grid.
// Why this is exact.  Take the block's own frame: the cells c_a − R .. c_a + R before the modulo.  While 2R + 1 < nc_a, 2R + 2 <= nc_a
// and so (R + 1) h_a <= L_a / 2: a scanned point lies less than (R + 1) h_a from q along the axis in that frame, so its wrapped offset
// (the image with |t| <= L_a / 2) IS its offset in the block's frame, and every image of a point that was not scanned lies outside the
// block, no nearer than the nearest face.  Once 2R + 1 >= nc_a every cell of the axis is scanned, the wrap rule picks each point's
// nearest image, and the axis has nothing behind it.  The loop therefore ends when the k-th distance is inside the nearest face that
// still has cells behind it — for a periodic axis both faces, until the axis is covered — or when every axis is covered.
// Static register indexing only (KM candidate registers, k <= KM).
template <int DIM, bool SELF, int KM>
__device__ __forceinline__ void knn_ring_search_periodic(const float *__restrict__ pos, const int *__restrict__ cell_start,
                                                         const double (&q)[DIM], const int (&c)[3], long long self, const int (&nc)[3],
                                                         const float (&org)[3], const double (&per)[3], const double (&h)[3], int k,
                                                         double (&best_d)[KM], int (&best_j)[KM]) {
    const int nc0 = nc[0], nc1 = nc[1];
    for (int R = 1;; ++R) {
#pragma unroll
        for (int u = 0; u < KM; ++u) { best_d[u] = 1e300; best_j[u] = -1; }
        int first[3] = {0, 0, 0}, count[3] = {1, 1, 1};
        bool whole = true;
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
            if (per[a] > 0.0) {
                if (2 * R + 1 >= nc[a]) {
                    first[a] = 0; count[a] = nc[a];
                } else {
                    first[a] = c[a] - R < 0 ? c[a] - R + nc[a] : c[a] - R;
                    count[a] = 2 * R + 1;
                    whole = false;
                }
            } else {
                const int lo = max(c[a] - R, 0), hi = min(c[a] + R, nc[a] - 1);
                first[a] = lo; count[a] = hi - lo + 1;
                if (lo > 0 || hi < nc[a] - 1) whole = false;
            }
        }
        const int past = first[0] + count[0];          // > nc0: the fastest axis's range passes the seam and splits in two runs
        for (int iz = 0; iz < count[2]; ++iz) {
            int z = first[2] + iz;
            if (z >= nc[2]) z -= nc[2];
            for (int iy = 0; iy < count[1]; ++iy) {
                int y = first[1] + iy;
                if (y >= nc1) y -= nc1;
                const long long line = ((long long)z * nc1 + y) * nc0;
                for (int run = 0; run < 2; ++run) {
                    if (run == 1 && past <= nc0) break;
                    const int beg = cell_start[line + (run == 0 ? first[0] : 0)];
                    const int end = cell_start[line + (run == 0 ? min(past, nc0) : past - nc0)];
                    for (int j = beg; j < end; ++j) {
                        if (SELF && j == self) continue;
                        double d = 0.0;
#pragma unroll
                        for (int a = 0; a < DIM; ++a) {
                            double t = (double)pos[(long long)j * DIM + a] - q[a];
                            if (per[a] > 0.0) t = wrapped_offset(t, per[a]);
                            d += t * t;
                        }
                        int jj = j;
                        // sorted insertion by a swap chain: static register indexing only
#pragma unroll
                        for (int u = 0; u < KM; ++u) {
                            if (u < k && d < best_d[u]) {
                                const double td = best_d[u]; best_d[u] = d; d = td;
                                const int tj = best_j[u]; best_j[u] = jj; jj = tj;
                            }
                        }
                    }
                }
            }
        }
        if (whole) break;   // every axis is covered: the block is the whole grid
        double kth = 1e300;
#pragma unroll
        for (int u = 0; u < KM; ++u)
            if (u == k - 1) kth = best_d[u];
        // distance to the nearest face of the block (in its own frame) with cells behind it, shrunk by a rounding margin
        double safe = 1e300, hmin = 1e300;
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
            const bool wraps = per[a] > 0.0 && 2 * R + 1 < nc[a];
            if (wraps || (!(per[a] > 0.0) && c[a] - R > 0)) safe = fmin(safe, q[a] - ((double)org[a] + (double)(c[a] - R) * h[a]));
            if (wraps || (!(per[a] > 0.0) && c[a] + R < nc[a] - 1))
                safe = fmin(safe, ((double)org[a] + (double)(c[a] + R + 1) * h[a]) - q[a]);
            hmin = fmin(hmin, h[a]);
        }
        safe -= 1e-5 * hmin;
        if (safe > 0.0 && kth <= safe * safe) break;
    }
}

}  // namespace g4c
