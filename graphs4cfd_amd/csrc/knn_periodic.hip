// k nearest neighbours in the wrapped metric of a domain that is periodic along some of its axes (include/g4c.h,
// g4c_knn_grid_periodic): the search under the periodic PointSampler, MeshJet and Tracers.  This is the project's own metric — the
// offset along a periodic axis is wrapped by connect_knn's rule — not the chord embedding connect_knn ranks by.
//
// MI355X form: as knn_grid.hip — the caller bins the cloud into a cell grid, one lane per query scans the block of cells within R
// rings of its own cell and keeps its k best candidates in registers — with a grid that tiles a periodic axis exactly, cell ranges
// taken modulo the axis's cell count, and a stop rule that counts both faces of a periodic axis until the block covers it
// (knn_periodic.h has the routine and the argument for its exactness).  The queries are wrapped and their cells formed here, on the
// device: a query may lie periods away (exactly, to the fp32 resolution of (q − o) / L; the wrapped value is always finite).
// Distances are fp64 sums of squares of the wrapped offsets of the fp32 coordinates.
#include "g4c_common.h"
#include "knn_periodic.h"

#include <cmath>

namespace {

constexpr int KMAX = 16;   // candidate registers: instantiated for 8 and 16, as knn_grid_kernel

struct grid_arg {          // g4c_periodic_grid_t by value, the period widened once on the host
    int nc[3];
    float org[3];
    float per32[3];
    double per[3], h[3];
};

// SELF: the queries are the cloud's own sorted points (itself excluded, result row = its original index, coordinates as they are);
// otherwise m query points, wrapped into the period first, result row = s.
template <int DIM, bool SELF, int KM>
__global__ __launch_bounds__(256) void knn_periodic_kernel(const float *__restrict__ pos, const int *__restrict__ order,
                                                          const int *__restrict__ cell_start, const float *__restrict__ qpos,
                                                          long long m, const grid_arg g, int k, int64_t *__restrict__ out) {
    const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= m) return;
    const int nc[3] = {g.nc[0], g.nc[1], g.nc[2]};
    const float org[3] = {g.org[0], g.org[1], g.org[2]};
    const double per[3] = {g.per[0], g.per[1], g.per[2]};
    const double h[3] = {g.h[0], g.h[1], g.h[2]};
    double q[DIM];
    int c[3] = {0, 0, 0};
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
        float v = SELF ? pos[s * DIM + a] : qpos[s * DIM + a];
        if (!SELF && g.per32[a] > 0.f) v = g4c::wrap_coordinate(v, org[a], g.per32[a]);
        q[a] = (double)v;
        c[a] = g4c::periodic_cell(q[a], org[a], h[a], nc[a]);
    }
    double best_d[KM];
    int best_j[KM];
    g4c::knn_ring_search_periodic<DIM, SELF, KM>(pos, cell_start, q, c, s, nc, org, per, h, k, best_d, best_j);
    const long long row = SELF ? (long long)order[s] : s;
#pragma unroll
    for (int u = 0; u < KM; ++u)
        if (u < k) out[row * k + u] = best_j[u] >= 0 ? (int64_t)order[best_j[u]] : (int64_t)-1;
}

int check_grid(const char *me, const g4c_periodic_grid_t *grid, int32_t dim, grid_arg &g) {
    G4C_REQUIRE(grid, G4C_EINVAL, "%s: null pointer", me);
    G4C_REQUIRE(dim == 2 || dim == 3, G4C_EINVAL, "%s: dim=%d, must be 2 or 3", me, dim);
    for (int a = 0; a < 3; ++a) {
        const bool live = a < dim;
        g.nc[a] = live ? grid->n_cells[a] : 1;
        g.org[a] = live ? grid->origin[a] : 0.f;
        g.per32[a] = live ? grid->period[a] : 0.f;
        g.per[a] = (double)g.per32[a];
        g.h[a] = live ? grid->cell[a] : 1.0;
        G4C_REQUIRE(grid->n_cells[a] >= 1 && (live || grid->n_cells[a] == 1), G4C_EINVAL, "%s: bad grid %d x %d x %d", me,
                    grid->n_cells[0], grid->n_cells[1], grid->n_cells[2]);
        G4C_REQUIRE(!live || (std::isfinite(g.org[a]) && std::isfinite(g.h[a]) && g.h[a] > 0.0), G4C_EINVAL,
                    "%s: axis %d: origin %g, cell %g", me, a, (double)g.org[a], g.h[a]);
        G4C_REQUIRE(!live || (std::isfinite(g.per32[a]) && g.per32[a] >= 0.f), G4C_EINVAL, "%s: period[%d]=%g (0: not periodic)", me, a,
                    (double)g.per32[a]);
        // a periodic axis is tiled exactly: n_cells · cell is the period, to fp64 rounding
        G4C_REQUIRE(!live || g.per32[a] == 0.f || std::fabs((double)g.nc[a] * g.h[a] - g.per[a]) <= 1e-12 * g.per[a], G4C_EINVAL,
                    "%s: axis %d: %d cells of %g do not tile the period %g", me, a, g.nc[a], g.h[a], g.per[a]);
    }
    G4C_REQUIRE((long long)g.nc[0] * g.nc[1] * g.nc[2] < (1LL << 31), G4C_EINVAL, "%s: bad grid %d x %d x %d", me, g.nc[0], g.nc[1],
                g.nc[2]);
    return G4C_OK;
}

#define G4C_KNNP_LAUNCH(DIM_, SELF_, KM_, ...) knn_periodic_kernel<DIM_, SELF_, KM_><<<grid_dim, block, 0, (hipStream_t)stream>>>(__VA_ARGS__)
#define G4C_KNNP_DISPATCH(SELF_, ...)                                                  \
    do {                                                                               \
        if (dim == 2 && k <= 8) G4C_KNNP_LAUNCH(2, SELF_, 8, __VA_ARGS__);             \
        else if (dim == 2) G4C_KNNP_LAUNCH(2, SELF_, 16, __VA_ARGS__);                 \
        else if (k <= 8) G4C_KNNP_LAUNCH(3, SELF_, 8, __VA_ARGS__);                    \
        else G4C_KNNP_LAUNCH(3, SELF_, 16, __VA_ARGS__);                               \
    } while (0)

}  // namespace

extern "C" int g4c_knn_grid_periodic(const float *pos_sorted, const int32_t *order, const int32_t *cell_start, int64_t n, int32_t dim,
                                     const g4c_periodic_grid_t *grid, int32_t k, int64_t *out, void *stream) {
    const char *me = "g4c_knn_grid_periodic";
    G4C_REQUIRE(pos_sorted && order && cell_start && out, G4C_EINVAL, "%s: null pointer", me);
    grid_arg g;
    if (int rc = check_grid(me, grid, dim, g)) return rc;
    g4c::DeviceGuard on_device(out);
    G4C_REQUIRE(k >= 1 && k <= KMAX, G4C_EINVAL, "%s: k=%d outside [1, %d]", me, k, KMAX);
    G4C_REQUIRE(n > k && n < (1LL << 31), G4C_EINVAL, "%s: n=%lld needs more than k=%d points", me, (long long)n, k);
    const dim3 grid_dim((unsigned)((n + 255) / 256)), block(256);
    G4C_KNNP_DISPATCH(true, pos_sorted, order, cell_start, nullptr, n, g, k, out);
    return g4c::check_launch(me);
}

extern "C" int g4c_knn_grid_query_periodic(const float *pos_sorted, const int32_t *order, const int32_t *cell_start, int64_t n,
                                           int32_t dim, const g4c_periodic_grid_t *grid, const float *q_pos, int64_t m, int32_t k,
                                           int64_t *out, void *stream) {
    const char *me = "g4c_knn_grid_query_periodic";
    G4C_REQUIRE(pos_sorted && order && cell_start && (m == 0 || (q_pos && out)), G4C_EINVAL, "%s: null pointer", me);
    grid_arg g;
    if (int rc = check_grid(me, grid, dim, g)) return rc;
    g4c::DeviceGuard on_device(pos_sorted);
    G4C_REQUIRE(k >= 1 && k <= KMAX, G4C_EINVAL, "%s: k=%d outside [1, %d]", me, k, KMAX);
    G4C_REQUIRE(n >= k && n < (1LL << 31) && m >= 0 && m < (1LL << 31), G4C_EINVAL, "%s: n=%lld points for k=%d neighbours, m=%lld queries",
                me, (long long)n, k, (long long)m);
    if (m == 0) return G4C_OK;
    const dim3 grid_dim((unsigned)((m + 255) / 256)), block(256);
    G4C_KNNP_DISPATCH(false, pos_sorted, order, cell_start, q_pos, m, g, k, out);
    return g4c::check_launch(me);
}
