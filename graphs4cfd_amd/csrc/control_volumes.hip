// Node control volumes of a 2-D point cloud and the integrals weighted by them (include/g4c.h):
//   g4c_voronoi_cells       once per mesh: per node the polygon (its Voronoi cell within the cloud) ∩ (a clipping box) ∩ (optionally
//                           one half-plane through the node itself — a wall node's cell must not reach into the body), its area,
//                           centroid, vertex count, flags and the rings of the cell grid it walked;
//   g4c_weighted_integrals  per step: stats[t][e] = sum_i w_i z_i[a_e] z_i[b_e] for up to 8 entries, fp64 in a fixed order — one more
//                           part of the captured step (the step index is read on the device and never written);
//   g4c_weighted_integrals_adjoint  training: gx[i][c] = the derivative of Σ_q Σ_e g[q][e] I[q][e] by x[i][c], fp64 in a fixed order.
// A kNN cloud has no cells: the areas are what turns the node sums of the diagnostics into integrals over the domain.
//
// The construction does not search a fixed k.  One thread per node walks the rings of the caller's cell grid (the binned cloud of
// g4c_knn_grid) outward from the node's own cell and clips its polygon — Sutherland-Hodgman against one half-plane — by the bisector
// with every point it meets, until no unseen point can cut the polygon any more (the security radius: every point of the next ring is
// farther than twice the polygon's farthest vertex) or the next ring lies outside the grid.  The cell is exact for any cloud and any
// density.  The polygon lives in the thread's own LDS column, as mesh_jet_kernel keeps its derivatives: a runtime-indexed private array
// would go to scratch memory.
#include "g4c_common.h"
#include "step_record.h"

// No contraction anywhere in this file: every product is rounded before it is added, so a plain host loop over Python floats
// reproduces the bits.
#pragma clang fp contract(off)

namespace {

// ------------------------------------------------------------------------------------------------------------------ cells
constexpr int VC_THREADS = 64;
constexpr int MAXV = G4C_VORONOI_MAX_VERTS;
// what the edge that LEAVES a vertex lies on
constexpr unsigned char TAG_BOX = 0, TAG_BISECTOR = 1, TAG_WALL = 2;

struct vc_poly_t {
    double x[2][MAXV][VC_THREADS], y[2][MAXV][VC_THREADS];          // two buffers: a clip reads one and writes the other
    unsigned char tag[2][MAXV][VC_THREADS];
};

// The polygon of nv vertices in buffer `cur` (relative to the node), clipped to {v : c - (v_x a + v_y b) >= 0}: the new vertex count, in
// buffer `cur` again (flipped when anything was cut).  A vertex exactly on the line is kept; a polygon wholly inside is not copied.
// -1: the result would have more than MAXV vertices.
__device__ __forceinline__ int vc_clip(vc_poly_t &P, int l, int &cur, int nv, double a, double b, double c, unsigned char tag) {
    bool cut = false;
    for (int j = 0; j < nv; ++j) {
        const double t0 = P.x[cur][j][l] * a, t1 = P.y[cur][j][l] * b;
        const double s = c - (t0 + t1);
        cut = cut || s < 0.0;
    }
    if (!cut) return nv;
    const int nxt = cur ^ 1;
    int m = 0;
    double cx = P.x[cur][0][l], cy = P.y[cur][0][l];
    double cs;
    {
        const double t0 = cx * a, t1 = cy * b;
        cs = c - (t0 + t1);
    }
    for (int j = 0; j < nv; ++j) {
        const int jn = j + 1 < nv ? j + 1 : 0;
        const unsigned char ct = P.tag[cur][j][l];
        const double nx = P.x[cur][jn][l], ny = P.y[cur][jn][l];
        const double t0 = nx * a, t1 = ny * b;
        const double ns = c - (t0 + t1);
        if (cs >= 0.0) {          // the vertex stays; the edge that leaves it runs along the clip line when it sits on the line and leaves
            if (m >= MAXV) return -1;
            P.x[nxt][m][l] = cx;
            P.y[nxt][m][l] = cy;
            P.tag[nxt][m][l] = (cs == 0.0 && ns < 0.0) ? tag : ct;
            ++m;
        }
        // the crossing of the edge (cur -> next), unless it is one of the two vertices themselves
        if ((cs > 0.0 && ns < 0.0) || (cs < 0.0 && ns > 0.0)) {
            if (m >= MAXV) return -1;
            const double t = cs / (cs - ns);
            const double dx = nx - cx, dy = ny - cy;
            const double ux = t * dx, uy = t * dy;
            P.x[nxt][m][l] = cx + ux;
            P.y[nxt][m][l] = cy + uy;
            P.tag[nxt][m][l] = cs > 0.0 ? tag : ct;          // leaving: along the clip line; entering: the rest of the old edge
            ++m;
        }
        cx = nx; cy = ny; cs = ns;
    }
    cur = nxt;
    return m;
}

struct vc_args_t {
    int nc0, nc1;
    double o0, o1, h;
    double lo0, lo1, hi0, hi1;
};

__global__ __launch_bounds__(VC_THREADS) void voronoi_cells_kernel(
    const float *__restrict__ pos,          // [n, 2] the cloud in cell-sorted order
    const int *__restrict__ order,          // [n] node row of each sorted point
    const int *__restrict__ cell_start,     // [nc0 nc1 + 1]
    const double *__restrict__ normals,     // [n, 2] by node row, or NULL
    const vc_args_t g, long long n, double *__restrict__ area, double *__restrict__ centroid, int *__restrict__ nvert,
    unsigned char *__restrict__ flags, int *__restrict__ rings) {
    __shared__ vc_poly_t P;
    const int l = threadIdx.x;
    const long long s = (long long)blockIdx.x * VC_THREADS + l;
    if (s >= n) return;          // (no barrier below: a thread touches its own LDS column only)
    const long long row = order[s];
    const double q0 = (double)pos[2 * s], q1 = (double)pos[2 * s + 1];
    // the node's cell, as the caller's binning forms it: clamped as a double before it becomes an integer
    const double f0 = fmin(fmax(floor((q0 - g.o0) / g.h), 0.0), (double)(g.nc0 - 1));
    const double f1 = fmin(fmax(floor((q1 - g.o1) / g.h), 0.0), (double)(g.nc1 - 1));
    const int c0 = (int)f0, c1 = (int)f1;

    int cur = 0, nv = 4;
    P.x[0][0][l] = g.lo0 - q0; P.y[0][0][l] = g.lo1 - q1;
    P.x[0][1][l] = g.hi0 - q0; P.y[0][1][l] = g.lo1 - q1;
    P.x[0][2][l] = g.hi0 - q0; P.y[0][2][l] = g.hi1 - q1;
    P.x[0][3][l] = g.lo0 - q0; P.y[0][3][l] = g.hi1 - q1;
#pragma unroll
    for (int j = 0; j < 4; ++j) P.tag[0][j][l] = TAG_BOX;

    unsigned fl = 0;
    int walked = 0;
    bool done = false;          // the polygon overflowed or became empty: nothing more to clip
    if (normals) {
        const double n0 = normals[2 * row], n1 = normals[2 * row + 1];
        if (n0 != 0.0 || n1 != 0.0) {
            fl |= G4C_VORONOI_WALL;
            nv = vc_clip(P, l, cur, nv, -n0, -n1, 0.0, TAG_WALL);
            if (nv < 0) { fl |= G4C_VORONOI_OVERFLOW; done = true; }
            else if (nv < 3) { nv = 0; done = true; }
        }
    }

    const int max_r = max(max(c0, g.nc0 - 1 - c0), max(c1, g.nc1 - 1 - c1));
    for (int rho = 0; rho <= max_r && !done; ++rho) {
        if (rho >= 1) {
            double r2 = 0.0;
            for (int j = 0; j < nv; ++j) {
                const double t0 = P.x[cur][j][l] * P.x[cur][j][l], t1 = P.y[cur][j][l] * P.y[cur][j][l];
                r2 = fmax(r2, t0 + t1);
            }
            // no point of ring rho is nearer than the nearest face of the block of rings < rho that has cells behind it
            double lb = 1e300;
            if (c0 - rho + 1 > 0) lb = fmin(lb, q0 - (g.o0 + (double)(c0 - rho + 1) * g.h));
            if (c0 + rho - 1 < g.nc0 - 1) lb = fmin(lb, (g.o0 + (double)(c0 + rho) * g.h) - q0);
            if (c1 - rho + 1 > 0) lb = fmin(lb, q1 - (g.o1 + (double)(c1 - rho + 1) * g.h));
            if (c1 + rho - 1 < g.nc1 - 1) lb = fmin(lb, (g.o1 + (double)(c1 + rho) * g.h) - q1);
            lb -= 1e-5 * g.h;          // (a rounding margin, as in knn_grid_kernel)
            if (lb > 0.0 && lb * lb > 4.0 * r2) break;
        }
        ++walked;
        for (int y = c1 - rho; y <= c1 + rho && !done; ++y) {
            if (y < 0 || y >= g.nc1) continue;
            const bool full = y == c1 - rho || y == c1 + rho;
            // a full row of the ring is one contiguous run of sorted points; any other row holds its two end cells
            for (int part = 0; part < (full ? 1 : 2) && !done; ++part) {
                int x0, x1;
                if (full) { x0 = max(c0 - rho, 0); x1 = min(c0 + rho, g.nc0 - 1); }
                else { x0 = x1 = part == 0 ? c0 - rho : c0 + rho; if (x0 < 0 || x0 >= g.nc0) continue; }
                const long long line = (long long)y * g.nc0;
                const int beg = cell_start[line + x0], end = cell_start[line + x1 + 1];
                for (int j = beg; j < end; ++j) {
                    if (j == s) continue;
                    const double rx = (double)pos[2 * (long long)j] - q0, ry = (double)pos[2 * (long long)j + 1] - q1;
                    const double t0 = rx * rx, t1 = ry * ry;
                    const double d2 = t0 + t1;
                    if (d2 == 0.0) { fl |= G4C_VORONOI_DUPLICATE; continue; }          // a point at zero distance cuts nothing
                    nv = vc_clip(P, l, cur, nv, rx, ry, 0.5 * d2, TAG_BISECTOR);
                    if (nv < 0) { fl |= G4C_VORONOI_OVERFLOW; done = true; break; }
                    if (nv < 3) { nv = 0; done = true; break; }
                }
            }
        }
    }

    // the shoelace sum about the node, in vertex order
    double a2 = 0.0, sx = 0.0, sy = 0.0;
    bool box = false;
    if (nv < 0) nv = 0;
    for (int j = 0; j < nv; ++j) {
        const int jn = j + 1 < nv ? j + 1 : 0;
        const double x = P.x[cur][j][l], y = P.y[cur][j][l], xn = P.x[cur][jn][l], yn = P.y[cur][jn][l];
        const double t0 = x * yn, t1 = xn * y;
        const double cr = t0 - t1;
        a2 += cr;
        const double ux = (x + xn) * cr, uy = (y + yn) * cr;
        sx += ux;
        sy += uy;
        box = box || P.tag[cur][j][l] == TAG_BOX;
    }
    if (box) fl |= G4C_VORONOI_BOX;
    double A = 0.0, g0 = q0, g1 = q1;          // degenerate rows are +0, and their centroid is the node
    if (nv >= 3 && a2 > 0.0) {
        A = 0.5 * a2;
        const double d = 3.0 * a2;
        g0 = q0 + sx / d;
        g1 = q1 + sy / d;
    }
    area[row] = A;
    centroid[2 * row] = g0;
    centroid[2 * row + 1] = g1;
    nvert[row] = nv;
    flags[row] = (unsigned char)fl;
    rings[row] = walked;
}

// ------------------------------------------------------------------------------------------------------------------ integrals
// The grid, the scratch ([workgroup][ne] behind the header) and the reduction are the step-record core's (step_record.h): all sums.
constexpr int WI_THREADS = g4c::THREADS;
constexpr int WI_MAX_ENTRIES = G4C_INTEGRALS_MAX_ENTRIES;

template <int NE>
__global__ __launch_bounds__(WI_THREADS) void weighted_integrals_kernel(
    const float *__restrict__ x, int x_ld, int x_step, const float *__restrict__ sub, int sub_ld, int sub_step,
    const double *__restrict__ w, const g4c_integral_program_t kp, const int *__restrict__ step, int t_host, int max_steps,
    long long n_nodes, double *__restrict__ scratch) {
    // The program is read from LDS, not from the kernel arguments: held in scalar registers over the node loop it spilt them.
    __shared__ g4c_integral_program_t sp;
    if (threadIdx.x == 0) sp = kp;
    __syncthreads();
    const g4c_integral_program_t &p = sp;
    const int t = step ? __builtin_nontemporal_load(step) : t_host;
    const bool live = t >= 0 && t < max_steps;          // every address below is formed from a checked t
    double acc[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) acc[e] = 0.0;
    if (live) {
        const long long stride = (long long)gridDim.x * WI_THREADS;
        for (long long n = (long long)blockIdx.x * WI_THREADS + threadIdx.x; n < n_nodes; n += stride) {
            const double wn = w[n];
            if (wn == 0.0) continue;          // a row of zero weight contributes nothing, whatever it holds
            const float *xr = x + n * x_ld + (long long)x_step * t;
            const float *sr = sub ? sub + n * sub_ld + (long long)sub_step * t : nullptr;
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                const int a = p.a[e], b = p.b[e];
                double za = 1.0, zb = 1.0;
                if (a >= 0) za = sr ? (double)xr[a] - (double)sr[a] : (double)xr[a];
                if (b >= 0) zb = sr ? (double)xr[b] - (double)sr[b] : (double)xr[b];
                const double pr = za * zb;
                const double term = wn * pr;
                acc[e] += term;
            }
        }
    }
    // (`live` is the same in every workgroup: nobody writes the step index before the step's closing launch)
    if (live) g4c::block_reduce<g4c::all_sums>(acc, NE, g4c::partials(scratch, blockIdx.x, NE));
    if (blockIdx.x == 0 && threadIdx.x == 0) g4c::post_step(scratch, live, t);
}

template <int NE>
void wi_launch(const g4c_weighted_integrals_t &wi, const g4c_integral_program_t &p, long long n_nodes, hipStream_t s) {
    const int blocks = (int)g4c::blocks_or_one(n_nodes);
    weighted_integrals_kernel<NE><<<dim3((unsigned)blocks), dim3(WI_THREADS), 0, s>>>(
        wi.x, wi.x_ld, wi.x_step, wi.sub, wi.sub_ld, wi.sub_step, wi.w, p, wi.step, wi.t_host, wi.max_steps, n_nodes, wi.scratch);
    g4c::partials_kernel<g4c::all_sums, NE, true><<<dim3(1), dim3(WI_THREADS), 0, s>>>(wi.scratch, blocks, NE, wi.stats, wi.max_steps);
}

// ------------------------------------------------------------------------------------------------------------------ integrals, transposed
// gx[i][c] = d (Σ_q Σ_e g[q][e] I[q][e]) / d x[i][c].  One thread per (node, column): item n nz + c of the [n_nodes, nz] block, so the lanes
// of a wave store consecutive floats of gx (gx_ld == nz: whole cache lines; a thread per node would store with a stride of nz floats).
// The three or four threads of a node read the same w, group, g and x: one cache line, fetched once.
constexpr int WA_THREADS = g4c::THREADS;

__global__ __launch_bounds__(WA_THREADS) void weighted_integrals_adjoint_kernel(
    const float *__restrict__ x, int x_ld, long long x_off, const float *__restrict__ sub, int sub_ld, long long sub_off, int nz,
    const double *__restrict__ w, const double *__restrict__ g, int n_groups, const int *__restrict__ group,
    const g4c_integral_program_t kp, long long n_nodes, float *__restrict__ gx, int gx_ld) {
    // The program is read from LDS, as in the forward (held in scalar registers over the loops it spilt them there) — once, into the
    // thread's own registers: the loops below are unrolled over the 8 slots, a slot behind the program's end names no column.
    __shared__ g4c_integral_program_t sp;
    if (threadIdx.x == 0) sp = kp;
    __syncthreads();
    const int ne = sp.ne;
    int pa[WI_MAX_ENTRIES], pb[WI_MAX_ENTRIES];
#pragma unroll
    for (int e = 0; e < WI_MAX_ENTRIES; ++e) {
        pa[e] = e < ne ? sp.a[e] : -2;
        pb[e] = e < ne ? sp.b[e] : -2;
    }
    // the workgroup's first item as (node, column), advanced by the grid's stride without a division in the loop
    const long long stride = (long long)gridDim.x * WA_THREADS;
    const long long dq = stride / nz;
    const int dr = (int)(stride - dq * nz);
    long long n0 = ((long long)blockIdx.x * WA_THREADS) / nz;
    int c0 = (int)((long long)blockIdx.x * WA_THREADS - n0 * nz);
    for (; n0 < n_nodes; n0 += dq, c0 += dr) {
        if (c0 >= nz) { c0 -= nz; ++n0; }
        const unsigned l = threadIdx.x + (unsigned)c0;
        const unsigned dn = l / (unsigned)nz;
        const long long n = n0 + dn;
        const int c = (int)(l - dn * (unsigned)nz);
        if (n >= n_nodes) continue;          // (no barrier below)
        const double wn = w[n];
        const int q = group ? group[n] : 0;
        double acc = 0.0;
        // a row of zero weight, or of a group outside [0, n_groups), is +0 whatever it holds: nothing of it is read
        if (wn != 0.0 && q >= 0 && q < n_groups) {
            const float *xr = x + n * x_ld + x_off;
            const float *sr = sub ? sub + n * sub_ld + sub_off : nullptr;
            const double *gq = g + (long long)q * ne;
            // First the loads of all 8 slots, in flight together and without a branch: a slot that does not name column c (or lies
            // behind the program's end) reads a valid address of the same cache lines — g of the last entry, the sample's column 0 —
            // and is then SKIPPED by a select, not multiplied by zero.  Then the sums, in the order of the entries.  The other column
            // of an entry is b when a == c and a when b == c (a == b == c: the same sample twice).
            const float *sq = sr ? sr : xr;
            double ge[WI_MAX_ENTRIES];
            float xo[WI_MAX_ENTRIES], so[WI_MAX_ENTRIES];
#pragma unroll
            for (int e = 0; e < WI_MAX_ENTRIES; ++e) {
                const int o = pa[e] == c ? pb[e] : pa[e];
                const int os = o > 0 ? o : 0;
                ge[e] = gq[e < ne ? e : ne - 1];
                xo[e] = xr[os];
                so[e] = sq[os];
            }
#pragma unroll
            for (int e = 0; e < WI_MAX_ENTRIES; ++e) {
                const bool ha = pa[e] == c, hb = pb[e] == c;
                const int o = ha ? pb[e] : pa[e];
                double z = (double)xo[e];
                if (sr) z = z - (double)so[e];
                z = o >= 0 ? z : 1.0;
                const double gw = ge[e] * wn;
                const double term = gw * z;
                const double one = acc + term;
                acc = ha ? one : acc;
                const double two = acc + term;
                acc = hb ? two : acc;
            }
        }
        gx[n * gx_ld + c] = (float)acc;
    }
}

}  // namespace

extern "C" int g4c_voronoi_cells(const g4c_voronoi_cells_t *vc, int64_t n_nodes, void *stream) {
    const char *me = "g4c_voronoi_cells";
    G4C_REQUIRE(vc, G4C_EINVAL, "%s: null pointer", me);
    G4C_REQUIRE(n_nodes >= 0 && n_nodes < (1LL << 31), G4C_EINVAL, "%s: bad size n_nodes=%lld", me, (long long)n_nodes);
    G4C_REQUIRE(vc->cell_size > 0.f && vc->cell_size <= 3.4028234e38f && vc->n_cells[0] >= 1 && vc->n_cells[1] >= 1 &&
                    (long long)vc->n_cells[0] * vc->n_cells[1] < (1LL << 31),
                G4C_EINVAL, "%s: bad grid %d x %d, cell %g", me, vc->n_cells[0], vc->n_cells[1], (double)vc->cell_size);
    G4C_REQUIRE(vc->origin[0] - vc->origin[0] == 0.f && vc->origin[1] - vc->origin[1] == 0.f, G4C_EINVAL, "%s: an origin that is not finite", me);
    // (a NaN corner fails every comparison)
    G4C_REQUIRE(vc->box_lo[0] < vc->box_hi[0] && vc->box_lo[1] < vc->box_hi[1] && vc->box_lo[0] - vc->box_lo[0] == 0.0 &&
                    vc->box_lo[1] - vc->box_lo[1] == 0.0 && vc->box_hi[0] - vc->box_hi[0] == 0.0 && vc->box_hi[1] - vc->box_hi[1] == 0.0,
                G4C_EINVAL, "%s: the box [%g, %g] x [%g, %g] is empty or not finite", me, vc->box_lo[0], vc->box_hi[0], vc->box_lo[1],
                vc->box_hi[1]);
    if (n_nodes == 0) return G4C_OK;
    G4C_REQUIRE(vc->pos_sorted && vc->order && vc->cell_start && vc->area && vc->centroid && vc->nvert && vc->flags && vc->rings, G4C_EINVAL,
                "%s: null pointer", me);
    g4c::DeviceGuard on_device(vc->pos_sorted);
    const vc_args_t g = {vc->n_cells[0],          vc->n_cells[1], (double)vc->origin[0], (double)vc->origin[1],
                         (double)vc->cell_size, vc->box_lo[0],  vc->box_lo[1],         vc->box_hi[0],
                         vc->box_hi[1]};
    const unsigned blocks = (unsigned)((n_nodes + VC_THREADS - 1) / VC_THREADS);
    voronoi_cells_kernel<<<dim3(blocks), dim3(VC_THREADS), 0, (hipStream_t)stream>>>(vc->pos_sorted, vc->order, vc->cell_start, vc->normals, g,
                                                                                     n_nodes, vc->area, vc->centroid, vc->nvert, vc->flags,
                                                                                     vc->rings);
    return g4c::check_launch(me);
}

extern "C" int64_t g4c_weighted_integrals_scratch_doubles(int64_t n_nodes, int32_t ne) {
    G4C_REQUIRE(n_nodes >= 0 && ne >= 1, G4C_EINVAL, "g4c_weighted_integrals_scratch_doubles: bad sizes n_nodes=%lld ne=%d", (long long)n_nodes, ne);
    G4C_REQUIRE(ne <= WI_MAX_ENTRIES, G4C_EUNSUPPORTED, "g4c_weighted_integrals_scratch_doubles: ne=%d entries (1 .. %d are supported)", ne,
                WI_MAX_ENTRIES);
    return g4c::HEADER + g4c::blocks_or_one(n_nodes) * ne;
}

extern "C" int g4c_weighted_integrals(const g4c_weighted_integrals_t *wi, const g4c_integral_program_t *prog, int64_t n_nodes, void *stream) {
    const char *me = "g4c_weighted_integrals";
    G4C_REQUIRE(wi && prog, G4C_EINVAL, "%s: null pointer", me);
    G4C_REQUIRE(n_nodes >= 0 && wi->nz >= 1 && wi->max_steps >= 0 && prog->ne >= 1, G4C_EINVAL, "%s: bad sizes n_nodes=%lld nz=%d max_steps=%d ne=%d",
                me, (long long)n_nodes, wi->nz, wi->max_steps, prog->ne);
    G4C_REQUIRE(prog->ne <= WI_MAX_ENTRIES, G4C_EUNSUPPORTED, "%s: ne=%d entries (1 .. %d are supported)", me, prog->ne, WI_MAX_ENTRIES);
    for (int e = 0; e < prog->ne; ++e)
        G4C_REQUIRE(prog->a[e] >= -1 && prog->a[e] < wi->nz && prog->b[e] >= -1 && prog->b[e] < wi->nz, G4C_EINVAL,
                    "%s: entry %d = (%d, %d) outside [-1, nz = %d)", me, e, prog->a[e], prog->b[e], wi->nz);
    // a source is [n_nodes, ld] with the step's columns at step_cols * t: step_cols 0 (one step: ld >= nz) or >= nz (every step)
    G4C_REQUIRE(wi->x_step == 0 ? wi->x_ld >= wi->nz : (wi->x_step >= wi->nz && (long long)wi->x_ld >= (long long)wi->x_step * wi->max_steps),
                G4C_EINVAL, "%s: x_ld=%d x_step=%d for nz=%d columns and max_steps=%d", me, wi->x_ld, wi->x_step, wi->nz, wi->max_steps);
    if (wi->sub)
        G4C_REQUIRE(wi->sub_step == 0 ? wi->sub_ld >= wi->nz
                                      : (wi->sub_step >= wi->nz && (long long)wi->sub_ld >= (long long)wi->sub_step * wi->max_steps),
                    G4C_EINVAL, "%s: sub_ld=%d sub_step=%d for nz=%d columns and max_steps=%d", me, wi->sub_ld, wi->sub_step, wi->nz,
                    wi->max_steps);
    G4C_REQUIRE(wi->stats && wi->scratch, G4C_EINVAL, "%s: null pointer", me);
    G4C_REQUIRE(n_nodes == 0 || (wi->x && wi->w), G4C_EINVAL, "%s: null pointer", me);
    g4c::DeviceGuard on_device(wi->stats);
    hipStream_t s = (hipStream_t)stream;
    switch (prog->ne) {
        case 1: wi_launch<1>(*wi, *prog, n_nodes, s); break;
        case 2: wi_launch<2>(*wi, *prog, n_nodes, s); break;
        case 3: wi_launch<3>(*wi, *prog, n_nodes, s); break;
        case 4: wi_launch<4>(*wi, *prog, n_nodes, s); break;
        case 5: wi_launch<5>(*wi, *prog, n_nodes, s); break;
        case 6: wi_launch<6>(*wi, *prog, n_nodes, s); break;
        case 7: wi_launch<7>(*wi, *prog, n_nodes, s); break;
        default: wi_launch<8>(*wi, *prog, n_nodes, s); break;
    }
    return g4c::check_launch(me);
}

extern "C" int g4c_weighted_integrals_adjoint(const g4c_weighted_integrals_adjoint_t *wa, const g4c_integral_program_t *prog, int64_t n_nodes,
                                              void *stream) {
    const char *me = "g4c_weighted_integrals_adjoint";
    G4C_REQUIRE(wa && prog, G4C_EINVAL, "%s: null pointer", me);
    G4C_REQUIRE(n_nodes >= 0 && wa->nz >= 1 && n_nodes <= (1LL << 62) / wa->nz && wa->max_steps >= 0 && prog->ne >= 1 && wa->n_groups >= 1,
                G4C_EINVAL, "%s: bad sizes n_nodes=%lld nz=%d max_steps=%d ne=%d n_groups=%d", me, (long long)n_nodes, wa->nz, wa->max_steps,
                prog->ne, wa->n_groups);
    G4C_REQUIRE(prog->ne <= WI_MAX_ENTRIES, G4C_EUNSUPPORTED, "%s: ne=%d entries (1 .. %d are supported)", me, prog->ne, WI_MAX_ENTRIES);
    for (int e = 0; e < prog->ne; ++e)
        G4C_REQUIRE(prog->a[e] >= -1 && prog->a[e] < wa->nz && prog->b[e] >= -1 && prog->b[e] < wa->nz, G4C_EINVAL,
                    "%s: entry %d = (%d, %d) outside [-1, nz = %d)", me, e, prog->a[e], prog->b[e], wa->nz);
    // the step is the host's: every address of the launch is formed from it, so it is refused here and not skipped on the device
    G4C_REQUIRE(wa->t_host >= 0 && wa->t_host < wa->max_steps, G4C_EINVAL, "%s: step t_host=%d outside [0, max_steps = %d)", me, wa->t_host,
                wa->max_steps);
    G4C_REQUIRE(wa->x_step == 0 ? wa->x_ld >= wa->nz : (wa->x_step >= wa->nz && (long long)wa->x_ld >= (long long)wa->x_step * wa->max_steps),
                G4C_EINVAL, "%s: x_ld=%d x_step=%d for nz=%d columns and max_steps=%d", me, wa->x_ld, wa->x_step, wa->nz, wa->max_steps);
    if (wa->sub)
        G4C_REQUIRE(wa->sub_step == 0 ? wa->sub_ld >= wa->nz
                                      : (wa->sub_step >= wa->nz && (long long)wa->sub_ld >= (long long)wa->sub_step * wa->max_steps),
                    G4C_EINVAL, "%s: sub_ld=%d sub_step=%d for nz=%d columns and max_steps=%d", me, wa->sub_ld, wa->sub_step, wa->nz,
                    wa->max_steps);
    G4C_REQUIRE(wa->gx_ld >= wa->nz, G4C_EINVAL, "%s: gx_ld=%d for nz=%d columns", me, wa->gx_ld, wa->nz);
    if (n_nodes == 0) return G4C_OK;
    G4C_REQUIRE(wa->x && wa->w && wa->g && wa->gx, G4C_EINVAL, "%s: null pointer", me);
    g4c::DeviceGuard on_device(wa->gx);
    const unsigned blocks = (unsigned)g4c::blocks_or_one(n_nodes * wa->nz);
    weighted_integrals_adjoint_kernel<<<dim3(blocks), dim3(WA_THREADS), 0, (hipStream_t)stream>>>(
        wa->x, wa->x_ld, (long long)wa->x_step * wa->t_host, wa->sub, wa->sub_ld, (long long)wa->sub_step * wa->t_host, wa->nz, wa->w, wa->g,
        wa->n_groups, wa->group, *prog, n_nodes, wa->gx, wa->gx_ld);
    return g4c::check_launch(me);
}
