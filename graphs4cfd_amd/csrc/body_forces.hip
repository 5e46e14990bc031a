// The force a flow exerts on the bodies it passes (include/g4c.h): g4c_body_forces, once per step — per wall item the pressure at its
// node and the velocity's least-squares gradient there (the loop of mesh_derived_kernel, mesh_gradient.hip: fp32, the in-edges in CSR
// order), the stress and the two tractions on the item's area vector in fp64, and per body the six sums Fp_x, Fp_y, Fv_x, Fv_y, Mp, Mv.
// A wall is hundreds of items: ONE workgroup of 256 per body takes its items tid, tid + 256, ... into register accumulators, a xor
// butterfly per wave, the four waves in order through LDS (the records' rule, rollout_record.hip) — no second launch, no atomics,
// nothing passes between workgroups: the bits are a function of the data alone.
#include "g4c_common.h"

// No contraction anywhere in this file: every product is rounded before it is added, so a plain host loop reproduces the bits.
#pragma clang fp contract(off)

namespace {

constexpr int BF_THREADS = 256;
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

    // the records' reduction: a 6-level xor butterfly per wave, then the four waves in order through LDS
    __shared__ double part[BF_WAVES][NSUM];
#pragma unroll
    for (int j = 0; j < NSUM; ++j) {
        double v = acc[j];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, 64);
        acc[j] = v;
    }
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
