// The two per-point device routines of the tracers' stages (tracer.hip), as templates (inlined: no call, no table):
//   knn_ring_search   the exact ring search over a cell grid — a COPY of the body of knn_grid_kernel (knn_grid.hip), statement for
//                     statement, compiled with the default contraction as that kernel is.  It is a copy and not shared because
//                     calling it from knn_grid_kernel cost that kernel registers (2 - 5 VGPRs in its KM = 8 forms, two more SGPR
//                     spills in one KM = 16 form): the kernel keeps its own body.  Whoever changes one changes
//                     the other; tests/test_gpu_tracers.py requires the tracers' neighbours to be g4c_knn_grid_query's.
//   mls_fit           the fp64 coefficients of the linear moving-least-squares fit, shared with sample_weights_kernel
//                     (point_sample.hip), whose body it was — no contraction: every product is rounded before it is added.
#pragma once
#include "g4c_common.h"

namespace g4c {

// The k nearest points of q among the cell-sorted cloud `pos` (cell_start: first sorted point of each cell), nearest first, into
// best_d / best_j[0 .. k − 1] (squared fp64 distances, SORTED indices; −1 where the cloud has fewer than k points).  c: the cell of
// q, clamped into the grid.  SELF: q is sorted point `self`, which is skipped.  Exact: the block of cells within R rings of c is
// scanned again with a larger R until the k-th distance is no larger than the distance to the nearest face of the block that still
// has cells behind it.  Static register indexing only (KM candidate registers, k <= KM).
template <int DIM, bool SELF, int KM>
__device__ __forceinline__ void knn_ring_search(const float *__restrict__ pos, const int *__restrict__ cell_start, const double (&q)[DIM],
                                                const int (&c)[3], long long self, const int (&nc)[3], const float (&org)[3], float h,
                                                int k, double (&best_d)[KM], int (&best_j)[KM]) {
    const int nc0 = nc[0], nc1 = nc[1];
    int max_r = 0;
#pragma unroll
    for (int a = 0; a < DIM; ++a) max_r = max(max_r, max(c[a], nc[a] - 1 - c[a]));

    for (int R = 1;; ++R) {
#pragma unroll
        for (int u = 0; u < KM; ++u) { best_d[u] = 1e300; best_j[u] = -1; }
        int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
#pragma unroll
        for (int a = 0; a < DIM; ++a) { lo[a] = max(c[a] - R, 0); hi[a] = min(c[a] + R, nc[a] - 1); }
        for (int z = lo[2]; z <= hi[2]; ++z)
            for (int y = lo[1]; y <= hi[1]; ++y) {
                // the cells lo[0] .. hi[0] of one grid line are consecutive cell ids: one contiguous run of sorted points
                const long long line = ((long long)z * nc1 + y) * nc0;
                const int beg = cell_start[line + lo[0]], end = cell_start[line + hi[0] + 1];
                for (int j = beg; j < end; ++j) {
                    if (SELF && j == self) continue;
                    double d = 0.0;
#pragma unroll
                    for (int a = 0; a < DIM; ++a) {
                        const double t = (double)pos[(long long)j * DIM + a] - q[a];
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
        double kth = 1e300;
#pragma unroll
        for (int u = 0; u < KM; ++u)
            if (u == k - 1) kth = best_d[u];
        if (R >= max_r) break;   // the block is the whole grid
        // distance to the nearest face of the block with cells behind it (shrunk by a rounding margin)
        double safe = 1e300;
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
            if (c[a] - R > 0) safe = fmin(safe, q[a] - ((double)org[a] + (double)(c[a] - R) * (double)h));
            if (c[a] + R < nc[a] - 1) safe = fmin(safe, ((double)org[a] + (double)(c[a] + R + 1) * (double)h) - q[a]);
        }
        safe -= 1e-5 * (double)h;
        if (safe > 0.0 && kth <= safe * safe) break;
    }
}

// f(j) for j = 0 .. k − 1 ascending.  KM == 0: a loop over j; KM > 0 (k <= KM): unrolled, so that f may index registers with j.
template <int KM, class F>
__device__ __forceinline__ void each_neighbour(int k, F f) {
    if constexpr (KM == 0) {
        for (int j = 0; j < k; ++j) f(j);
    } else {
#pragma unroll
        for (int j = 0; j < KM; ++j)
            if (j < k) f(j);
    }
}

// The coefficients of the linear moving-least-squares fit at one point over its k neighbours (include/g4c.h, g4c_sample_weights, has
// the rule).  nb(j, d) sets d = pos[neighbour j] − q in fp64 and returns Σ_a d_a²; put(j, c) receives coefficient j, rounded to fp32
// once; nearest(r2_0) the squared distance to the nearest neighbour, before anything else.  Returns whether the point is degenerate (Shepard's weights).
template <int DIM, int KM, class NB, class NEAR, class PUT>
__device__ __forceinline__ bool mls_fit(int k, int power, NB nb, NEAR nearest, PUT put) {
#pragma clang fp contract(off)
    auto weight = [&](double r2) -> double { return power == 0 ? 1.0 : (power == 1 ? 1.0 / sqrt(r2) : 1.0 / r2); };
    double d[DIM];
    const double r20 = nb(0, d);
    nearest(r20);
    if (r20 == 0.0) {          // the point is a node: its row, bit for bit
        each_neighbour<KM>(k, [&](int j) { put(j, j == 0 ? 1.f : 0.f); });
        return false;
    }
    // the weighted mean of the neighbours' offsets
    double W = 0.0, dbar[DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a) dbar[a] = 0.0;
    each_neighbour<KM>(k, [&](int j) {
        const double w = weight(nb(j, d));
        W += w;
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
            const double wd = w * d[a];
            dbar[a] += wd;
        }
    });
#pragma unroll
    for (int a = 0; a < DIM; ++a) dbar[a] = dbar[a] / W;
    // the normal matrix of the centred offsets, upper triangle row-major: (0,0), (0,1), .., (1,1), ..
    constexpr int NM = DIM * (DIM + 1) / 2;
    double m[NM];
#pragma unroll
    for (int i = 0; i < NM; ++i) m[i] = 0.0;
    each_neighbour<KM>(k, [&](int j) {
        const double w = weight(nb(j, d));
        double e[DIM];
#pragma unroll
        for (int a = 0; a < DIM; ++a) e[a] = d[a] - dbar[a];
        int i = 0;
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
#pragma unroll
            for (int b = a; b < DIM; ++b, ++i) {
                const double we = w * e[a];
                const double t = we * e[b];
                m[i] += t;
            }
        }
    });
    // adjugate and determinant, as mesh_gradient_weights_kernel forms them
    double adj[NM], det, tr;
    if constexpr (DIM == 2) {
        adj[0] = m[2];
        adj[1] = -m[1];
        adj[2] = m[0];
        const double p0 = m[0] * m[2], p1 = m[1] * m[1];
        det = p0 - p1;
        tr = m[0] + m[2];
    } else {
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
    // the gradient's rule; k <= dim centred offsets span less than the space whatever the rounding made of det
    const bool degen = k <= DIM || !(det > thr);
    // v = adj dbar:  M^-1 dbar = v / det
    double v[DIM];
    if constexpr (DIM == 2) {
        const double a0 = adj[0] * dbar[0], a1 = adj[1] * dbar[1], b0 = adj[1] * dbar[0], b1 = adj[2] * dbar[1];
        v[0] = a0 + a1;
        v[1] = b0 + b1;
    } else {
        const double a0 = adj[0] * dbar[0], a1 = adj[1] * dbar[1], a2 = adj[2] * dbar[2];
        const double b0 = adj[1] * dbar[0], b1 = adj[3] * dbar[1], b2 = adj[4] * dbar[2];
        const double c0 = adj[2] * dbar[0], c1 = adj[4] * dbar[1], c2 = adj[5] * dbar[2];
        v[0] = (a0 + a1) + a2;
        v[1] = (b0 + b1) + b2;
        v[2] = (c0 + c1) + c2;
    }
    const double invW = 1.0 / W;
    each_neighbour<KM>(k, [&](int j) {
        const double w = weight(nb(j, d));
        double c;
        if (degen) {
            c = w / W;                                   // Shepard: exact on constants only
        } else {
            double s = 0.0;
#pragma unroll
            for (int a = 0; a < DIM; ++a) {
                const double ea = d[a] - dbar[a];
                const double t = ea * v[a];
                s += t;
            }
            const double corr = s / det;
            c = w * (invW - corr);
        }
        put(j, (float)c);
    });
    return degen;
}

}  // namespace g4c
