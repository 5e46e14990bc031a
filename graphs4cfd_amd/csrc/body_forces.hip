// The force a flow exerts on the bodies it passes (include/g4c.h): g4c_body_forces, once per step — per wall item the pressure at its
// node and the velocity's least-squares gradient there (the loop of mesh_derived_kernel, mesh_gradient.hip: fp32, the in-edges in CSR
// order), the stress and the two tractions on the item's area vector in fp64, and per body the six sums Fp_x, Fp_y, Fv_x, Fv_y, Mp, Mv.
// A wall is hundreds of items: ONE workgroup of 256 per body takes its items tid, tid + 256, ... into register accumulators, a xor
// butterfly per wave, the four waves in order through LDS (the step-record core's order, step_record.h) — no second launch, no
// atomics, nothing passes between workgroups: the bits are a function of the data alone.
// g4c_body_forces_adjoint, below it, is the transpose of that map's linear part (its backward): two small launches, per item and per node.
#include "g4c_common.h"
#include "step_record.h"

// No contraction anywhere in this file: every product is rounded before it is added, so a plain host loop reproduces the bits.
#pragma clang fp contract(off)

namespace {

constexpr int BF_THREADS = g4c::THREADS;
constexpr int BF_WAVES = BF_THREADS / 64;
constexpr int NSUM = G4C_FORCES_NSUM;

template <bool VISCOUS>
__global__ __launch_bounds__(BF_THREADS) void body_forces_kernel(const g4c_body_forces_t d) {
    const int b = blockIdx.x;
    const int t = d.step ? d.step[0] : d.t0;
    const bool live = t >= 0 && t < d.max_steps;
    // (x_step != 0: the fields are columns x_step t .. of a target, an address only a checked t may form.  Uniform: taken by every
    //  thread of every workgroup or by none.)
    if (d.x_step != 0 && !live) return;
    const float *__restrict__ x = d.x + (long long)d.x_step * (d.x_step != 0 ? t : 0);
    const int w0 = d.body_off[b], w1 = d.body_off[b + 1];

    double acc[NSUM];
#pragma unroll
    for (int j = 0; j < NSUM; ++j) acc[j] = 0.0;

    for (int w = w0 + (int)threadIdx.x; w < w1; w += BF_THREADS) {
        const long long i = d.item[w];
        const float *xr = x + i * d.x_ld;
        float G[2][2] = {{0.f, 0.f}, {0.f, 0.f}};          // G[u or v][axis]
        if constexpr (VISCOUS) {
            const float xu = xr[d.ucol], xv = xr[d.vcol];
            const int e0 = d.off[i], e1 = d.off[i + 1];
            for (int e = e0; e < e1; ++e) {
                const float *xs = x + (long long)d.src[e] * d.x_ld;
                const float g0 = d.g[2ll * e], g1 = d.g[2ll * e + 1];
                const float du = xs[d.ucol] - xu, dv = xs[d.vcol] - xv;
                const float pu0 = g0 * du, pu1 = g1 * du, pv0 = g0 * dv, pv1 = g1 * dv;
                G[0][0] += pu0;
                G[0][1] += pu1;
                G[1][0] += pv0;
                G[1][1] += pv1;
            }
        }
        const double ax = d.area[2ll * w], ay = d.area[2ll * w + 1];
        const double rx = d.arm[2ll * w], ry = d.arm[2ll * w + 1];
        const double ps = d.p_scale * (double)xr[d.pcol];
        const double P = ps + d.p_shift;
        const double pax = P * ax, pay = P * ay;
        const double tpx = -pax, tpy = -pay;
        const double mp0 = rx * tpy, mp1 = ry * tpx;
        acc[G4C_FORCES_FPX] += tpx;
        acc[G4C_FORCES_FPY] += tpy;
        acc[G4C_FORCES_MP] += mp0 - mp1;
        double shear = 0.0;
        if constexpr (VISCOUS) {
            const double ugx = d.u_scale * (double)G[0][0], ugy = d.u_scale * (double)G[0][1];
            const double vgx = d.v_scale * (double)G[1][0], vgy = d.v_scale * (double)G[1][1];
            const double sxx = 2.0 * ugx, sxy = ugy + vgx, syy = 2.0 * vgy;
            const double xa = sxx * ax, xb = sxy * ay, ya = sxy * ax, yb = syy * ay;
            const double tvx = d.mu * (xa + xb), tvy = d.mu * (ya + yb);
            const double mv0 = rx * tvy, mv1 = ry * tvx;
            acc[G4C_FORCES_FVX] += tvx;
            acc[G4C_FORCES_FVY] += tvy;
            acc[G4C_FORCES_MV] += mv0 - mv1;
            const double nx = d.unit[2ll * w], ny = d.unit[2ll * w + 1];
            const double tx = -ny, ty = nx;
            const double c0 = tx * sxx, c1 = ty * sxy, c2 = tx * sxy, c3 = ty * syy;
            const double s0 = (c0 + c1) * nx, s1 = (c2 + c3) * ny;
            shear = d.mu * (s0 + s1);
        }
        if (d.wall) {
            d.wall[2ll * w] = (float)P;
            d.wall[2ll * w + 1] = (float)shear;
        }
    }

    // the step-record core's order (step_record.h): the butterfly per wave, then the four waves in order through LDS — in thread 0
    // alone, which needs all six sums to form `cur`
    __shared__ double part[BF_WAVES][NSUM];
#pragma unroll
    for (int j = 0; j < NSUM; ++j) acc[j] = g4c::wave_sum(acc[j]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int j = 0; j < NSUM; ++j) part[threadIdx.x >> 6][j] = acc[j];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s[NSUM];
#pragma unroll
        for (int j = 0; j < NSUM; ++j) {
            double v = part[0][j];
#pragma unroll
            for (int wv = 1; wv < BF_WAVES; ++wv) v = v + part[wv][j];
            s[j] = v;
        }
        if (d.stats && live) {
            double *st = d.stats + ((long long)t * gridDim.x + b) * NSUM;
#pragma unroll
            for (int j = 0; j < NSUM; ++j) st[j] = s[j];
        }
        float *cur = d.cur + 3ll * b;
        cur[0] = (float)(s[G4C_FORCES_FPX] + s[G4C_FORCES_FVX]);
        cur[1] = (float)(s[G4C_FORCES_FPY] + s[G4C_FORCES_FVY]);
        cur[2] = (float)(s[G4C_FORCES_MP] + s[G4C_FORCES_MV]);
    }
}

}  // namespace

extern "C" int g4c_body_forces(const g4c_body_forces_t *bf, int64_t n_bodies, int64_t n_items, void *stream) {
    const char *me = "g4c_body_forces";
    G4C_REQUIRE(bf, G4C_EINVAL, "%s: null pointer", me);
    G4C_REQUIRE(n_bodies >= 0 && n_items >= 0 && n_bodies <= 0x7fffffffll && n_items <= 0x7fffffffll && bf->x_ld >= 0 && bf->x_step >= 0 &&
                    bf->max_steps >= 0,
                G4C_EINVAL, "%s: bad sizes n_bodies=%lld n_items=%lld x_ld=%d x_step=%d max_steps=%d", me, (long long)n_bodies,
                (long long)n_items, bf->x_ld, bf->x_step, bf->max_steps);
    const bool viscous = bf->mu != 0.0;
    int top = bf->pcol;
    G4C_REQUIRE(bf->pcol >= 0, G4C_EINVAL, "%s: pcol=%d out of range", me, bf->pcol);
    if (viscous) {
        G4C_REQUIRE(bf->ucol >= 0 && bf->vcol >= 0, G4C_EINVAL, "%s: ucol=%d vcol=%d out of range", me, bf->ucol, bf->vcol);
        top = bf->ucol > top ? bf->ucol : top;
        top = bf->vcol > top ? bf->vcol : top;
    }
    G4C_REQUIRE(bf->x_step == 0 || top < bf->x_step, G4C_EINVAL, "%s: column %d out of range (x_step=%d fields a step)", me, top, bf->x_step);
    G4C_REQUIRE(bf->x_step == 0 || bf->max_steps >= 1, G4C_EINVAL, "%s: x_step=%d without max_steps", me, bf->x_step);
    const long long need = (long long)bf->x_step * (bf->x_step ? bf->max_steps - 1 : 0) + top + 1;
    G4C_REQUIRE(bf->x_ld >= need, G4C_EINVAL, "%s: x_ld=%d < %lld, the columns the launch reads", me, bf->x_ld, need);
    G4C_REQUIRE(!viscous || (bf->g && bf->src && bf->off), G4C_EINVAL, "%s: mu != 0 without the gradient's g, src and off", me);
    G4C_REQUIRE(!bf->stats || bf->max_steps >= 1, G4C_EINVAL, "%s: stats without max_steps", me);
    if (n_bodies == 0 || n_items == 0) return G4C_OK;
    G4C_REQUIRE(bf->x && bf->item && bf->body_off && bf->area && bf->unit && bf->arm && bf->cur, G4C_EINVAL, "%s: null pointer", me);
    g4c::DeviceGuard on_device(bf->x);
    hipStream_t s = (hipStream_t)stream;
    if (viscous)
        body_forces_kernel<true><<<dim3((unsigned)n_bodies), dim3(BF_THREADS), 0, s>>>(*bf);
    else
        body_forces_kernel<false><<<dim3((unsigned)n_bodies), dim3(BF_THREADS), 0, s>>>(*bf);
    return g4c::check_launch(me);
}

// ------------------------------------------------------------------------------------------------------------------ adjoint
// g4c_body_forces_adjoint (include/g4c.h has the arithmetic): the scatter from the wall items to their nodes and to the nodes that
// send to them, taken as a gather — the fp64 algebra once per item into hw, then ONE thread per node over its own items and its
// in-list in a fixed order.  Nothing passes between threads.
namespace {

constexpr int HW = 5;                         // hw[w] = (H[u][0], H[u][1], H[v][0], H[v][1], cp)

inline unsigned bfa_blocks(long long n) { return (unsigned)g4c::blocks_or_one(n); }          // as the sibling adjoints

template <bool VISCOUS>
__global__ __launch_bounds__(BF_THREADS) void body_forces_adjoint_items_kernel(const g4c_body_forces_adjoint_t d, long long n_items) {
    const long long stride = (long long)gridDim.x * BF_THREADS;
    for (long long w = (long long)blockIdx.x * BF_THREADS + threadIdx.x; w < n_items; w += stride) {
        const int b = d.item_body[w];
        double gf[NSUM];
#pragma unroll
        for (int j = 0; j < NSUM; ++j) gf[j] = d.gF ? d.gF[(long long)b * NSUM + j] : 0.0;
        const double gp = d.gwall ? (double)d.gwall[2 * w] : 0.0;
        const double ax = d.area[2 * w], ay = d.area[2 * w + 1];
        const double rx = d.arm[2 * w], ry = d.arm[2 * w + 1];
        float h[4] = {0.f, 0.f, 0.f, 0.f};
        if constexpr (VISCOUS) {
            const double gs = d.gwall ? (double)d.gwall[2 * w + 1] : 0.0;
            const double nx = d.unit[2 * w], ny = d.unit[2 * w + 1];
            const double tx = -ny, ty = nx;
            const double m0 = ry * gf[G4C_FORCES_MV], m1 = rx * gf[G4C_FORCES_MV];
            const double A = gf[G4C_FORCES_FVX] - m0, Bc = gf[G4C_FORCES_FVY] + m1;
            const double aax = A * ax, aay = A * ay, bax = Bc * ax, bay = Bc * ay;
            const double txnx = tx * nx, tynx = ty * nx, txny = tx * ny, tyny = ty * ny;
            const double sxx = gs * txnx, sxy = gs * (tynx + txny), syy = gs * tyny;
            const double dxx = d.mu * (aax + sxx);
            const double dxy = d.mu * ((aay + bax) + sxy);
            const double dyy = d.mu * (bay + syy);
            h[0] = (float)(d.u_scale * (2.0 * dxx));
            h[1] = (float)(d.u_scale * dxy);
            h[2] = (float)(d.v_scale * dxy);
            h[3] = (float)(d.v_scale * (2.0 * dyy));
        }
        const double fa = gf[G4C_FORCES_FPX] * ax, fb = gf[G4C_FORCES_FPY] * ay;
        const double c0 = rx * ay, c1 = ry * ax;
        const double mp = gf[G4C_FORCES_MP] * (c0 - c1);
        const float cp = (float)(d.p_scale * (gp - ((fa + fb) + mp)));
        float *o = d.hw + w * HW;
        o[0] = h[0];
        o[1] = h[1];
        o[2] = h[2];
        o[3] = h[3];
        o[4] = cp;
    }
}

// MODE 0: zero-fill (no item, no body, or no gradient at all); 1: the pressure column only (mu == 0); 2: with the viscous part.
template <int MODE>
__global__ __launch_bounds__(BF_THREADS) void body_forces_adjoint_nodes_kernel(const g4c_body_forces_adjoint_t d, long long n_nodes) {
    const float *__restrict__ hw = d.hw;
    const long long stride = (long long)gridDim.x * BF_THREADS;
    for (long long n = (long long)blockIdx.x * BF_THREADS + threadIdx.x; n < n_nodes; n += stride) {
        float p = 0.f, au = 0.f, av = 0.f;
        if constexpr (MODE >= 1) {
            const int k0 = d.own_off[n], k1 = d.own_off[n + 1];
#pragma unroll 4
            for (int k = k0; k < k1; ++k) p += hw[(long long)d.own_item[k] * HW + 4];
            if constexpr (MODE == 2) {
                // the in-list streams its items and weights; only the item's row of hw is a gather (four entries at a time: their
                // loads are in flight together — the adds keep the order)
                const int q0 = d.in_off[n], q1 = d.in_off[n + 1];
#pragma unroll 4
                for (int q = q0; q < q1; ++q) {
                    const float *h = hw + (long long)d.in_item[q] * HW;
                    const float g0 = d.in_g[2ll * q], g1 = d.in_g[2ll * q + 1];
                    const float pu0 = g0 * h[0], pu1 = g1 * h[1], pv0 = g0 * h[2], pv1 = g1 * h[3];
                    au += pu0;
                    au += pu1;
                    av += pv0;
                    av += pv1;
                }
                // the diagonal: for each own item, this node's own in-edges in CSR order
                const int e0 = d.off[n], e1 = d.off[n + 1];
                for (int k = k0; k < k1; ++k) {
                    const float *h = hw + (long long)d.own_item[k] * HW;
                    const float h0 = h[0], h1 = h[1], h2 = h[2], h3 = h[3];
#pragma unroll 4
                    for (int e = e0; e < e1; ++e) {
                        const float g0 = d.g[2ll * e], g1 = d.g[2ll * e + 1];
                        const float pu0 = g0 * h0, pu1 = g1 * h1, pv0 = g0 * h2, pv1 = g1 * h3;
                        au -= pu0;
                        au -= pu1;
                        av -= pv0;
                        av -= pv1;
                    }
                }
            }
        }
        float *row = d.gx + n * d.nf;
        for (int c = 0; c < d.nf; ++c) {
            float v = 0.f;
            if constexpr (MODE >= 1) {
                if (c == d.pcol) v = p;
            }
            if constexpr (MODE == 2) {
                if (c == d.ucol) v = au;
                if (c == d.vcol) v = av;
            }
            row[c] = v;
        }
    }
}

}  // namespace

extern "C" int g4c_body_forces_adjoint(const g4c_body_forces_adjoint_t *a, int64_t n_nodes, int64_t n_bodies, int64_t n_items,
                                       int64_t n_entries, void *stream) {
    const char *me = "g4c_body_forces_adjoint";
    G4C_REQUIRE(a, G4C_EINVAL, "%s: null pointer", me);
    G4C_REQUIRE(n_nodes >= 0 && n_bodies >= 0 && n_items >= 0 && n_entries >= 0 && n_bodies <= 0x7fffffffll && n_items <= 0x7fffffffll &&
                    n_entries <= 0x7fffffffll && a->nf >= 1,
                G4C_EINVAL, "%s: bad sizes n_nodes=%lld n_bodies=%lld n_items=%lld n_entries=%lld nf=%d", me, (long long)n_nodes,
                (long long)n_bodies, (long long)n_items, (long long)n_entries, a->nf);
    const bool viscous = a->mu != 0.0;
    G4C_REQUIRE(a->pcol >= 0 && a->pcol < a->nf, G4C_EINVAL, "%s: pcol=%d out of range (nf=%d)", me, a->pcol, a->nf);
    if (viscous) {
        G4C_REQUIRE(a->ucol >= 0 && a->ucol < a->nf && a->vcol >= 0 && a->vcol < a->nf, G4C_EINVAL, "%s: ucol=%d vcol=%d out of range (nf=%d)",
                    me, a->ucol, a->vcol, a->nf);
        G4C_REQUIRE(a->pcol != a->ucol && a->pcol != a->vcol && a->ucol != a->vcol, G4C_EINVAL, "%s: pcol=%d ucol=%d vcol=%d are not distinct",
                    me, a->pcol, a->ucol, a->vcol);
    }
    if (n_nodes == 0) return G4C_OK;
    G4C_REQUIRE(a->gx, G4C_EINVAL, "%s: null pointer (gx)", me);
    const bool live = n_items > 0 && n_bodies > 0 && (a->gF || a->gwall);
    if (live) {
        G4C_REQUIRE(a->item_body && a->area && a->arm && a->own_off && a->own_item && a->hw && (!viscous || a->unit), G4C_EINVAL,
                    "%s: null pointer", me);
        G4C_REQUIRE(!viscous || (a->g && a->off && a->in_off && (n_entries == 0 || (a->in_item && a->in_g))), G4C_EINVAL,
                    "%s: mu != 0 without the gradient's g and off and the in-tables", me);
        // gx must not share a byte with what the launches read behind it or with the scratch between them
        const char *x0 = (const char *)a->gx, *x1 = x0 + n_nodes * a->nf * 4ll;
        const struct { const void *p; long long bytes; const char *name; } other[] = {
            {a->gF, n_bodies * NSUM * 8ll, "gF"}, {a->gwall, n_items * 2 * 4ll, "gwall"}, {a->hw, n_items * HW * 4ll, "hw"}};
        for (const auto &o : other) {
            const char *p0 = (const char *)o.p;
            G4C_REQUIRE(!p0 || p0 + o.bytes <= x0 || x1 <= p0, G4C_EINVAL, "%s: gx aliases %s", me, o.name);
        }
    }
    g4c::DeviceGuard on_device(a->gx);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(bfa_blocks(n_nodes)), block(BF_THREADS);
    if (!live) {
        body_forces_adjoint_nodes_kernel<0><<<grid, block, 0, s>>>(*a, n_nodes);
    } else if (viscous) {
        body_forces_adjoint_items_kernel<true><<<dim3(bfa_blocks(n_items)), block, 0, s>>>(*a, n_items);
        body_forces_adjoint_nodes_kernel<2><<<grid, block, 0, s>>>(*a, n_nodes);
    } else {
        body_forces_adjoint_items_kernel<false><<<dim3(bfa_blocks(n_items)), block, 0, s>>>(*a, n_items);
        body_forces_adjoint_nodes_kernel<1><<<grid, block, 0, s>>>(*a, n_nodes);
    }
    return g4c::check_launch(me);
}
