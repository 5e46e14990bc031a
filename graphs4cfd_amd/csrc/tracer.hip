// Lagrangian tracers (include/g4c.h, g4c_tracer_advance): massless particles carried by a velocity that lives at the mesh nodes.  One
// launch moves every particle one step: per particle and stage the k nearest nodes by the exact ring search over the cloud's cell
// grid, the linear moving-least-squares coefficients over them in fp64, the velocity as their fp32 sum nearest first, and the
// explicit Euler or Heun update of the position — search, fit, interpolation and advance, which before took a host round trip per
// step.  One thread per particle, plain loads and stores, no atomics, no LDS, nothing between workgroups: a particle's bits are a
// function of its own position and of the node data alone.  The search and the fit are the templates of point_fit.h: the fit is shared with
// g4c_sample_weights, the search a statement-for-statement copy of g4c_knn_grid_query's — the same neighbours in the same order, the
// same coefficients.
#include "g4c_common.h"
#include "point_fit.h"
#include "knn_periodic.h"
#include "step_record.h"

#include <cmath>

// No contraction in this file (the search, in point_fit.h, keeps the default it always had): every product is rounded before it is
// added, so the launch equals the composition of g4c_sample_weights, g4c_sample_points and separate fp32 multiplies and adds.
#pragma clang fp contract(off)

namespace {

constexpr int TR_THREADS = g4c::THREADS;          // a launch takes g4c::blocks(n_particles) workgroups (step_record.h)

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) < __builtin_inff(); }          // (false for NaN)

// The physical velocity at r from the node tensor x: v_a = scale_a (Σ_j c_j x[idx_j ld + vcol_a]) + shift_a.  Returns the squared
// distance to the nearest node.  r must be finite.
template <int DIM, int KM>
__device__ __forceinline__ double stage(const g4c_tracer_t &s, const float (&r)[DIM], const float *__restrict__ x, int ld,
                                        float (&v)[DIM]) {
    const int nc[3] = {s.n_cells[0], s.n_cells[1], s.n_cells[2]};
    const float org[3] = {s.origin[0], s.origin[1], s.origin[2]};
    double qd[DIM];
    int c[3] = {0, 0, 0};
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
        qd[a] = (double)r[a];
        // the cell is clamped as a double BEFORE it becomes an integer: no position, however wild, forms an address
        double cc = floor((qd[a] - (double)org[a]) / (double)s.cell_size);
        cc = fmin(fmax(cc, 0.0), (double)(nc[a] - 1));
        c[a] = (int)cc;
    }
    double best_d[KM];
    int best_j[KM];
    g4c::knn_ring_search<DIM, false, KM>(s.pos_sorted, s.cell_start, qd, c, -1, nc, org, s.cell_size, s.k, best_d, best_j);
    float coef[KM];
    auto nb = [&](int j, double (&d)[DIM]) -> double {          // d_j = pos[idx_j] - q, returns r2_j
        const long long i = best_j[j];
        double r2 = 0.0;
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
            d[a] = (double)s.pos_sorted[i * DIM + a] - qd[a];
            const double sq = d[a] * d[a];
            r2 += sq;
        }
        return r2;
    };
    double r20 = 0.0;
    g4c::mls_fit<DIM, KM>(s.k, s.power, nb, [&](double r2) { r20 = r2; }, [&](int j, float cj) { coef[j] = cj; });
    float u[DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a) u[a] = 0.f;
    g4c::each_neighbour<KM>(s.k, [&](int j) {
        const float *row = x + (long long)s.order[best_j[j]] * ld;
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
            const float pr = coef[j] * row[s.vcol[a]];
            u[a] = j == 0 ? pr : u[a] + pr;
        }
    });
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
        const float sc = s.scale[a] * u[a];
        v[a] = sc + s.shift[a];
    }
    return r20;
}

template <int DIM, int KM, int SCHEME>
__global__ __launch_bounds__(TR_THREADS) void tracer_advance_kernel(const g4c_tracer_t s, long long n_particles) {
    const int t = s.step ? s.step[0] : s.t_host;          // read once
    const bool in_range = t >= 0 && t < s.max_steps;
    // the slot address is formed from a checked t
    float *series = nullptr;
    int slot;
    if (s.series && in_range && s.every > 0 && g4c::snapshot_slot(t, s.every, s.n_slots, slot))
        series = s.series + (long long)slot * n_particles * DIM;
    const long long stride = (long long)gridDim.x * TR_THREADS;
    for (long long p = (long long)blockIdx.x * TR_THREADS + threadIdx.x; p < n_particles; p += stride) {
        float q[DIM];
#pragma unroll
        for (int a = 0; a < DIM; ++a) q[a] = s.q[p * DIM + a];
        int st = s.status[p];
        if (in_range && t >= s.release[p] && st < G4C_TRACER_LEFT) {
            st = G4C_TRACER_MOVING;
            bool ok = true;
#pragma unroll
            for (int a = 0; a < DIM; ++a) ok = ok && finite_f(q[a]);
            if (!ok) {
                st = G4C_TRACER_NONFINITE;
            } else {
                float v0[DIM];
                const double r20 = stage<DIM, KM>(s, q, s.x0, s.x0_ld, v0);
                if ((float)sqrt(r20) > s.max_distance) {
                    st = G4C_TRACER_FAR;
                } else {
                    if (s.vel) {
#pragma unroll
                        for (int a = 0; a < DIM; ++a) s.vel[p * DIM + a] = v0[a];
                    }
                    float qn[DIM];
#pragma unroll
                    for (int a = 0; a < DIM; ++a) {
                        const float dv = s.dt * v0[a];
                        qn[a] = q[a] + dv;
                    }
                    if (SCHEME == G4C_TRACER_HEUN) {
#pragma unroll
                        for (int a = 0; a < DIM; ++a) ok = ok && finite_f(qn[a]);
                        if (ok) {
                            float v1[DIM];
                            stage<DIM, KM>(s, qn, s.x1, s.x1_ld, v1);
                            const float half = 0.5f * s.dt;
#pragma unroll
                            for (int a = 0; a < DIM; ++a) {
                                const float sum = v0[a] + v1[a];
                                const float dv = half * sum;
                                qn[a] = q[a] + dv;
                            }
                        } else {
                            st = G4C_TRACER_NONFINITE;
                        }
                    }
                    if (ok) {
                        bool inside = true;
#pragma unroll
                        for (int a = 0; a < DIM; ++a) {
                            q[a] = qn[a];
                            s.q[p * DIM + a] = qn[a];
                            inside = inside && qn[a] >= s.box_lo[a] && qn[a] <= s.box_hi[a];          // (NaN is outside)
                        }
                        if (!inside) st = G4C_TRACER_LEFT;
                    }
                }
            }
            s.status[p] = (unsigned char)st;
            if (st >= G4C_TRACER_LEFT) s.stopped[p] = t;
        }
        if (series) {
#pragma unroll
            for (int a = 0; a < DIM; ++a) series[p * DIM + a] = q[a];
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------ periodic
// The stage and the step in a domain that is periodic along some axes (g4c_tracer_advance_periodic).  Kernels of their own: the forms
// above keep their bodies and their bits.  A stage wraps a copy of its position, searches in the wrapped metric (knn_periodic.h) and
// fits over wrapped offsets, as g4c_knn_grid_query_periodic and g4c_sample_weights_periodic do.
template <int DIM, int KM>
__device__ __forceinline__ double stage_periodic(const g4c_tracer_periodic_t &sp, const float (&r)[DIM], const float *__restrict__ x, int ld,
                                                 float (&v)[DIM]) {
    const g4c_tracer_t &s = sp.base;
    const int nc[3] = {s.n_cells[0], s.n_cells[1], s.n_cells[2]};
    const float org[3] = {s.origin[0], s.origin[1], s.origin[2]};
    const double per[3] = {(double)sp.period[0], (double)sp.period[1], (double)sp.period[2]};
    const double h[3] = {sp.cell[0], sp.cell[1], sp.cell[2]};
    double qd[DIM];
    int c[3] = {0, 0, 0};
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
        float w = r[a];
        if (sp.period[a] > 0.f) w = g4c::wrap_coordinate(w, org[a], sp.period[a]);
        qd[a] = (double)w;
        c[a] = g4c::periodic_cell(qd[a], org[a], h[a], nc[a]);
    }
    double best_d[KM];
    int best_j[KM];
    g4c::knn_ring_search_periodic<DIM, false, KM>(s.pos_sorted, s.cell_start, qd, c, -1, nc, org, per, h, s.k, best_d, best_j);
    float coef[KM];
    auto nb = [&](int j, double (&d)[DIM]) -> double {          // d_j = the wrapped pos[idx_j] - q, returns r2_j
        const long long i = best_j[j];
        double r2 = 0.0;
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
            d[a] = (double)s.pos_sorted[i * DIM + a] - qd[a];
            if (per[a] > 0.0) d[a] = g4c::wrapped_offset(d[a], per[a]);
            const double sq = d[a] * d[a];
            r2 += sq;
        }
        return r2;
    };
    double r20 = 0.0;
    g4c::mls_fit<DIM, KM>(s.k, s.power, nb, [&](double r2) { r20 = r2; }, [&](int j, float cj) { coef[j] = cj; });
    float u[DIM];
#pragma unroll
    for (int a = 0; a < DIM; ++a) u[a] = 0.f;
    g4c::each_neighbour<KM>(s.k, [&](int j) {
        const float *row = x + (long long)s.order[best_j[j]] * ld;
#pragma unroll
        for (int a = 0; a < DIM; ++a) {
            const float pr = coef[j] * row[s.vcol[a]];
            u[a] = j == 0 ? pr : u[a] + pr;
        }
    });
#pragma unroll
    for (int a = 0; a < DIM; ++a) {
        const float sc = s.scale[a] * u[a];
        v[a] = sc + s.shift[a];
    }
    return r20;
}

// Whether coordinate v wraps along axis a (true for an axis that is not periodic): a finite position so large that the wrap sequence
// overflows is treated as one that is not finite — no stage runs on it, so no search starts from a made-up position.
__device__ __forceinline__ bool wraps(const g4c_tracer_periodic_t &sp, float v, int a) {
    return !(sp.period[a] > 0.f) || g4c::wraps_finite(v, sp.base.origin[a], sp.period[a]);
}

template <int DIM, int KM, int SCHEME>
__global__ __launch_bounds__(TR_THREADS) void tracer_advance_periodic_kernel(const g4c_tracer_periodic_t sp, long long n_particles) {
    const g4c_tracer_t &s = sp.base;
    const int t = s.step ? s.step[0] : s.t_host;          // read once
    const bool in_range = t >= 0 && t < s.max_steps;
    // the slot address is formed from a checked t
    float *series = nullptr;
    int slot;
    if (s.series && in_range && s.every > 0 && g4c::snapshot_slot(t, s.every, s.n_slots, slot))
        series = s.series + (long long)slot * n_particles * DIM;
    const long long stride = (long long)gridDim.x * TR_THREADS;
    for (long long p = (long long)blockIdx.x * TR_THREADS + threadIdx.x; p < n_particles; p += stride) {
        float q[DIM];
#pragma unroll
        for (int a = 0; a < DIM; ++a) q[a] = s.q[p * DIM + a];
        int st = s.status[p];
        if (in_range && t >= s.release[p] && st < G4C_TRACER_LEFT) {
            st = G4C_TRACER_MOVING;
            bool ok = true;
#pragma unroll
            for (int a = 0; a < DIM; ++a) ok = ok && finite_f(q[a]) && wraps(sp, q[a], a);
            if (!ok) {
                st = G4C_TRACER_NONFINITE;
            } else {
                float v0[DIM];
                const double r20 = stage_periodic<DIM, KM>(sp, q, s.x0, s.x0_ld, v0);
                if ((float)sqrt(r20) > s.max_distance) {
                    st = G4C_TRACER_FAR;
                } else {
                    if (s.vel) {
#pragma unroll
                        for (int a = 0; a < DIM; ++a) s.vel[p * DIM + a] = v0[a];
                    }
                    float qn[DIM];
#pragma unroll
                    for (int a = 0; a < DIM; ++a) {
                        const float dv = s.dt * v0[a];
                        qn[a] = q[a] + dv;
                    }
                    if (SCHEME == G4C_TRACER_HEUN) {
#pragma unroll
                        for (int a = 0; a < DIM; ++a) ok = ok && finite_f(qn[a]) && wraps(sp, qn[a], a);
                        if (ok) {
                            float v1[DIM];
                            stage_periodic<DIM, KM>(sp, qn, s.x1, s.x1_ld, v1);
                            const float half = 0.5f * s.dt;
#pragma unroll
                            for (int a = 0; a < DIM; ++a) {
                                const float sum = v0[a] + v1[a];
                                const float dv = half * sum;
                                qn[a] = q[a] + dv;
                            }
                        } else {
                            st = G4C_TRACER_NONFINITE;
                        }
                    }
                    // a new position that does not wrap (not finite, or so large that the wrap overflows) is not stored
                    if (ok) {
#pragma unroll
                        for (int a = 0; a < DIM; ++a) ok = ok && wraps(sp, qn[a], a);
                        if (!ok) st = G4C_TRACER_NONFINITE;
                    }
                    if (ok) {
                        bool inside = true;
#pragma unroll
                        for (int a = 0; a < DIM; ++a) {
                            // wrapped before it is stored, tested and written to the series: crossing a periodic face is no leaving
                            if (sp.period[a] > 0.f) qn[a] = g4c::wrap_coordinate(qn[a], s.origin[a], sp.period[a]);
                            q[a] = qn[a];
                            s.q[p * DIM + a] = qn[a];
                            inside = inside && qn[a] >= s.box_lo[a] && qn[a] <= s.box_hi[a];          // (NaN is outside)
                        }
                        if (!inside) st = G4C_TRACER_LEFT;
                    }
                }
            }
            s.status[p] = (unsigned char)st;
            if (st >= G4C_TRACER_LEFT) s.stopped[p] = t;
        }
        if (series) {
#pragma unroll
            for (int a = 0; a < DIM; ++a) series[p * DIM + a] = q[a];
        }
    }
}

// The argument checks of both entry points.
int check_tracer(const char *me, const g4c_tracer_t *tr, int64_t n_nodes, int64_t n_particles, bool periodic) {
    G4C_REQUIRE(n_nodes >= 0 && n_nodes < (1LL << 31) && n_particles >= 0 && tr->k >= 1 && tr->x0_ld >= 0 && tr->x1_ld >= 0 &&
                    tr->max_steps >= 0 && tr->every >= 0 && tr->n_slots >= 0,
                G4C_EINVAL, "%s: bad sizes n_nodes=%lld n_particles=%lld k=%d x0_ld=%d x1_ld=%d max_steps=%d every=%d n_slots=%d", me,
                (long long)n_nodes, (long long)n_particles, tr->k, tr->x0_ld, tr->x1_ld, tr->max_steps, tr->every, tr->n_slots);
    G4C_REQUIRE(tr->dim == 2 || tr->dim == 3, G4C_EUNSUPPORTED, "%s: dim=%d (2 or 3 are supported)", me, tr->dim);
    G4C_REQUIRE(tr->k <= G4C_SAMPLE_MAX_K, G4C_EUNSUPPORTED, "%s: k=%d neighbours (1 .. %d are supported)", me, tr->k, G4C_SAMPLE_MAX_K);
    G4C_REQUIRE(tr->power >= 0 && tr->power <= 2, G4C_EINVAL, "%s: power=%d (0, 1 or 2)", me, tr->power);
    G4C_REQUIRE(tr->scheme == G4C_TRACER_EULER || tr->scheme == G4C_TRACER_HEUN, G4C_EINVAL, "%s: scheme=%d (0 Euler, 1 Heun)", me, tr->scheme);
    const bool heun = tr->scheme == G4C_TRACER_HEUN;
    for (int a = 0; a < tr->dim; ++a) {
        G4C_REQUIRE(tr->vcol[a] >= 0 && tr->vcol[a] < tr->x0_ld && (!heun || tr->vcol[a] < tr->x1_ld), G4C_EINVAL,
                    "%s: vcol[%d]=%d is no column of x0 (ld %d)%s", me, a, tr->vcol[a], tr->x0_ld, heun ? " and x1" : "");
    }
    G4C_REQUIRE((periodic || tr->cell_size > 0.f) && tr->n_cells[0] >= 1 && tr->n_cells[1] >= 1 && tr->n_cells[2] >= 1 &&
                    (tr->dim == 3 || tr->n_cells[2] == 1) && (long long)tr->n_cells[0] * tr->n_cells[1] * tr->n_cells[2] < (1LL << 31),
                G4C_EINVAL, "%s: bad grid %d x %d x %d, cell %g", me, tr->n_cells[0], tr->n_cells[1], tr->n_cells[2], (double)tr->cell_size);
    for (int a = 0; a < tr->dim; ++a)
        G4C_REQUIRE(std::isfinite(tr->origin[a]), G4C_EINVAL, "%s: origin[%d] is not finite", me, a);
    G4C_REQUIRE(tr->every > 0 || !tr->series, G4C_EINVAL, "%s: a series buffer with every=0", me);
    if (n_particles == 0) return G4C_OK;
    G4C_REQUIRE(n_nodes >= tr->k, G4C_EINVAL, "%s: k=%d neighbours of n_nodes=%lld", me, tr->k, (long long)n_nodes);
    G4C_REQUIRE(tr->pos_sorted && tr->order && tr->cell_start && tr->x0 && (!heun || tr->x1) && tr->q && tr->status && tr->stopped &&
                    tr->release,
                G4C_EINVAL, "%s: null pointer", me);
    return G4C_OK;
}

}  // namespace

extern "C" int g4c_tracer_advance_periodic(const g4c_tracer_periodic_t *tr, int64_t n_nodes, int64_t n_particles, void *stream) {
    const char *me = "g4c_tracer_advance_periodic";
    G4C_REQUIRE(tr, G4C_EINVAL, "%s: null pointer", me);
    if (int rc = check_tracer(me, &tr->base, n_nodes, n_particles, true)) return rc;
    for (int a = 0; a < tr->base.dim; ++a) {
        G4C_REQUIRE(std::isfinite(tr->period[a]) && tr->period[a] >= 0.f, G4C_EINVAL, "%s: period[%d]=%g (0: not periodic)", me, a,
                    (double)tr->period[a]);
        G4C_REQUIRE(std::isfinite(tr->cell[a]) && tr->cell[a] > 0.0, G4C_EINVAL, "%s: cell[%d]=%g", me, a, tr->cell[a]);
        G4C_REQUIRE(tr->period[a] == 0.f || std::fabs((double)tr->base.n_cells[a] * tr->cell[a] - (double)tr->period[a]) <=
                                                1e-12 * (double)tr->period[a],
                    G4C_EINVAL, "%s: axis %d: %d cells of %g do not tile the period %g", me, a, tr->base.n_cells[a], tr->cell[a],
                    (double)tr->period[a]);
    }
    if (n_particles == 0) return G4C_OK;
    g4c::DeviceGuard on_device(tr->base.q);
    hipStream_t s = (hipStream_t)stream;
    g4c_tracer_periodic_t d = *tr;
    if (d.base.every == 0 || d.base.n_slots == 0) d.base.series = nullptr;
    for (int a = d.base.dim; a < 3; ++a) { d.period[a] = 0.f; d.cell[a] = 1.0; }
    const bool heun = d.base.scheme == G4C_TRACER_HEUN;
    const dim3 grid((unsigned)g4c::blocks(n_particles)), block(TR_THREADS);
#define G4C_TRACERP_LAUNCH(DIM_, KM_, SCHEME_) tracer_advance_periodic_kernel<DIM_, KM_, SCHEME_><<<grid, block, 0, s>>>(d, (long long)n_particles)
#define G4C_TRACERP_SCHEME(DIM_, KM_)                                    \
    do {                                                                 \
        if (heun) G4C_TRACERP_LAUNCH(DIM_, KM_, G4C_TRACER_HEUN);        \
        else G4C_TRACERP_LAUNCH(DIM_, KM_, G4C_TRACER_EULER);            \
    } while (0)
    if (d.base.dim == 2 && d.base.k <= 8) G4C_TRACERP_SCHEME(2, 8);
    else if (d.base.dim == 2) G4C_TRACERP_SCHEME(2, 16);
    else if (d.base.k <= 8) G4C_TRACERP_SCHEME(3, 8);
    else G4C_TRACERP_SCHEME(3, 16);
    return g4c::check_launch(me);
}

extern "C" int g4c_tracer_advance(const g4c_tracer_t *tr, int64_t n_nodes, int64_t n_particles, void *stream) {
    const char *me = "g4c_tracer_advance";
    G4C_REQUIRE(tr, G4C_EINVAL, "%s: null pointer", me);
    if (int rc = check_tracer(me, tr, n_nodes, n_particles, false)) return rc;
    if (n_particles == 0) return G4C_OK;
    const bool heun = tr->scheme == G4C_TRACER_HEUN;
    g4c::DeviceGuard on_device(tr->q);
    hipStream_t s = (hipStream_t)stream;
    g4c_tracer_t d = *tr;
    if (d.every == 0 || d.n_slots == 0) d.series = nullptr;
    const dim3 grid((unsigned)g4c::blocks(n_particles)), block(TR_THREADS);
#define G4C_TRACER_LAUNCH(DIM_, KM_, SCHEME_) tracer_advance_kernel<DIM_, KM_, SCHEME_><<<grid, block, 0, s>>>(d, (long long)n_particles)
#define G4C_TRACER_SCHEME(DIM_, KM_)                                    \
    do {                                                                \
        if (heun) G4C_TRACER_LAUNCH(DIM_, KM_, G4C_TRACER_HEUN);        \
        else G4C_TRACER_LAUNCH(DIM_, KM_, G4C_TRACER_EULER);            \
    } while (0)
    if (d.dim == 2 && d.k <= 8) G4C_TRACER_SCHEME(2, 8);
    else if (d.dim == 2) G4C_TRACER_SCHEME(2, 16);
    else if (d.k <= 8) G4C_TRACER_SCHEME(3, 8);
    else G4C_TRACER_SCHEME(3, 16);
    return g4c::check_launch(me);
}
