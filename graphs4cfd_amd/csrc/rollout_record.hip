// The recording form of the rollout's bookkeeping launch (g4c_rollout_advance, remus_ops.hip): the same shift of the history window
// and the same bump of the device-side step index, and — for the bytes it moves anyway — strided snapshots of the prediction, the
// prediction's rows at a list of probe nodes, and per-field error sums of the step against a target, all addressed by the step
// index the launch reads on the device (so a captured launch records every replay in its own slot).
#include "g4c_common.h"
#include "step_record.h"

namespace {

constexpr int REC_THREADS = g4c::THREADS;
constexpr int NSTAT = G4C_REC_NSTAT;
// scratch (step_record.h): the header, then [workgroup][nf][G4C_REC_NSTAT]; of every field's set one position is a maximum
using rec_policy = g4c::max_at<NSTAT, G4C_REC_MAX_ABS_ERR>;

// NF > 0: nf == NF, rec.target is given and the statistics are formed (NF * NSTAT fp64 accumulators per thread, in registers);
// NF == 0: any nf, no statistics — the launch of g4c_rollout_advance with the snapshot slot and the probes added.
template <int NF>
__global__ __launch_bounds__(REC_THREADS) void rollout_advance_record_kernel(
    float *__restrict__ field, int field_cols, const float *__restrict__ pred, int nf_any, const g4c_rollout_rec_t rec,
    int *__restrict__ step, long long n_nodes) {
    const int nf = NF ? NF : nf_any;
    const int t = __builtin_nontemporal_load(step);
    // a step index outside [0, max_steps) leaves no record at all: every record address below is formed from a checked t
    const bool live = t >= 0 && t < rec.max_steps;
    float *snap = nullptr;
    int slot;
    if (live && rec.every > 0 && g4c::snapshot_slot(t, rec.every, rec.n_snap, slot)) snap = rec.snap + (long long)slot * n_nodes * nf;
    const bool stats = NF > 0 && live;
    double acc[NF ? NF * NSTAT : 1];
#pragma unroll
    for (int j = 0; j < (NF ? NF * NSTAT : 1); ++j) acc[j] = 0.0;

    const long long stride = (long long)gridDim.x * REC_THREADS;
    const long long gid = (long long)blockIdx.x * REC_THREADS + threadIdx.x;
    for (long long n = gid; n < n_nodes; n += stride) {
        float *fr = field + n * field_cols;
        // roll left by nf, then append pred (row-local, in place, ascending order is safe)
        for (int c = 0; c + nf < field_cols; ++c) fr[c] = fr[c + nf];
        const float *pr = pred + n * nf;
        if constexpr (NF > 0) {
            float y[NF];
#pragma unroll
            for (int c = 0; c < NF; ++c) y[c] = pr[c];
#pragma unroll
            for (int c = 0; c < NF; ++c) fr[field_cols - NF + c] = y[c];
            if (snap) {
#pragma unroll
                for (int c = 0; c < NF; ++c) snap[n * NF + c] = y[c];
            }
            if (stats) {
                const float *tg = rec.target + n * rec.target_ld + (long long)NF * t;
                const bool masked = rec.mask && rec.mask[n] != 0;
#pragma unroll
                for (int c = 0; c < NF; ++c) {
                    const double yt = (double)tg[c];
                    const double d = (double)y[c] - yt, ad = fabs(d);
                    double *a = acc + c * NSTAT;
                    a[G4C_REC_SQ_ERR] += d * d;
                    a[G4C_REC_ABS_ERR] += ad;
                    a[G4C_REC_MAX_ABS_ERR] = g4c::nan_max(a[G4C_REC_MAX_ABS_ERR], ad);
                    a[G4C_REC_TGT_SUM] += yt;
                    a[G4C_REC_TGT_SQ_SUM] += yt * yt;
                    a[G4C_REC_ABS_ERR_MASK] += masked ? ad : 0.0;
                }
            }
        } else {
            for (int c = 0; c < nf; ++c) {
                const float y = pr[c];
                fr[field_cols - nf + c] = y;
                if (snap) snap[n * nf + c] = y;
            }
        }
    }
    if constexpr (NF > 0) {
        // (`stats` is the same in every workgroup: all of them read the step index before anybody bumps it)
        if (stats) g4c::block_reduce<rec_policy>(acc, NF * NSTAT, g4c::partials(rec.scratch, blockIdx.x, NF * NSTAT));
        if (gid == 0) g4c::post_step(rec.scratch, stats, t);
    }
    // probes: pred's rows at the listed nodes (pred is only read by this launch); a row outside the mesh writes nothing
    if (live && rec.n_probe > 0) {
        for (long long p = gid; p < rec.n_probe; p += stride) {
            const long long r = rec.probe_rows[p];
            if (r < 0 || r >= n_nodes) continue;
            float *po = rec.probe_out + ((long long)t * rec.n_probe + p) * nf;
            for (int c = 0; c < nf; ++c) po[c] = pred[r * nf + c];
        }
    }
    // *step = t + 1 by the LAST workgroup to get here, exactly as rollout_advance_kernel does it (remus_ops.hip: a ticket counter in
    // step[1], no fence — only this workgroup's READ of the step index has to have completed)
    __syncthreads();
    if (threadIdx.x == 0) {
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        if (atomicAdd(step + 1, 1) == (int)gridDim.x - 1) { step[1] = 0; step[0] = t + 1; }
    }
}

template <int NF>
void rec_launch(float *field, int field_cols, const float *pred, int nf, const g4c_rollout_rec_t &rec, int *step, long long n_nodes,
                hipStream_t s) {
    const int blocks = (int)g4c::blocks_or_one(n_nodes);
    rollout_advance_record_kernel<NF><<<dim3((unsigned)blocks), dim3(REC_THREADS), 0, s>>>(field, field_cols, pred, nf, rec, step, n_nodes);
    if constexpr (NF > 0)
        g4c::partials_kernel<rec_policy, NF, true><<<dim3(1), dim3(REC_THREADS), 0, s>>>(rec.scratch, blocks, NF, rec.stats, rec.max_steps);
}

}  // namespace

extern "C" int64_t g4c_rollout_record_scratch_doubles(int64_t n_nodes, int32_t nf) {
    G4C_REQUIRE(n_nodes >= 0 && nf >= 1, G4C_EINVAL, "g4c_rollout_record_scratch_doubles: bad sizes n_nodes=%lld nf=%d", (long long)n_nodes, nf);
    G4C_REQUIRE(nf <= 8, G4C_EUNSUPPORTED, "g4c_rollout_record_scratch_doubles: statistics of nf=%d fields (1 .. 8 are supported)", nf);
    return g4c::HEADER + g4c::blocks_or_one(n_nodes) * nf * NSTAT;
}

extern "C" int g4c_rollout_advance_record(float *field, int32_t field_cols, const float *pred, int32_t nf, const g4c_rollout_rec_t *rec,
                                          int32_t *step, int64_t n_nodes, void *stream) {
    const char *me = "g4c_rollout_advance_record";
    G4C_REQUIRE(step && rec, G4C_EINVAL, "%s: null pointer", me);
    G4C_REQUIRE(nf > 0 && field_cols >= nf && n_nodes >= 0, G4C_EINVAL, "%s: bad sizes nf=%d field_cols=%d", me, nf, field_cols);
    G4C_REQUIRE(rec->max_steps >= 0 && rec->every >= 0 && rec->n_snap >= 0 && rec->n_probe >= 0, G4C_EINVAL,
                "%s: negative count max_steps=%d every=%d n_snap=%d n_probe=%d", me, rec->max_steps, rec->every, rec->n_snap, rec->n_probe);
    G4C_REQUIRE(rec->every > 0 || !rec->snap, G4C_EINVAL, "%s: a snapshot buffer with every=0", me);
    G4C_REQUIRE((rec->n_probe > 0) == (rec->probe_rows != nullptr), G4C_EINVAL, "%s: probe_rows does not agree with n_probe=%d", me, rec->n_probe);
    G4C_REQUIRE(rec->target || !rec->mask, G4C_EINVAL, "%s: a mask without a target", me);
    if (rec->target) {
        G4C_REQUIRE((long long)rec->target_ld >= (long long)nf * rec->max_steps, G4C_EINVAL, "%s: target_ld=%d < nf * max_steps = %lld", me,
                    rec->target_ld, (long long)nf * rec->max_steps);
        G4C_REQUIRE(rec->stats && rec->scratch, G4C_EINVAL, "%s: a target without stats or scratch", me);
        G4C_REQUIRE(nf <= 8, G4C_EUNSUPPORTED, "%s: statistics of nf=%d fields (1 .. 8 are supported)", me, nf);
    }
    if (n_nodes > 0) {        // (no nodes: field, pred and the records are empty and have no address; the launch still advances the step index)
        G4C_REQUIRE(field && pred, G4C_EINVAL, "%s: null pointer", me);
        G4C_REQUIRE(rec->every == 0 || rec->n_snap == 0 || rec->snap, G4C_EINVAL, "%s: every=%d, n_snap=%d and no snapshot buffer", me,
                    rec->every, rec->n_snap);
        G4C_REQUIRE(rec->n_probe == 0 || rec->max_steps == 0 || rec->probe_out, G4C_EINVAL, "%s: n_probe=%d and no probe_out", me, rec->n_probe);
    }
    g4c::DeviceGuard on_device(step);
    hipStream_t s = (hipStream_t)stream;
    g4c_rollout_rec_t r = *rec;
    if (n_nodes == 0) r.every = r.n_probe = 0;
    const bool stats = r.target && n_nodes > 0;
    switch (stats ? nf : 0) {
        case 0: rec_launch<0>(field, field_cols, pred, nf, r, step, n_nodes, s); break;
        case 1: rec_launch<1>(field, field_cols, pred, nf, r, step, n_nodes, s); break;
        case 2: rec_launch<2>(field, field_cols, pred, nf, r, step, n_nodes, s); break;
        case 3: rec_launch<3>(field, field_cols, pred, nf, r, step, n_nodes, s); break;
        case 4: rec_launch<4>(field, field_cols, pred, nf, r, step, n_nodes, s); break;
        case 5: rec_launch<5>(field, field_cols, pred, nf, r, step, n_nodes, s); break;
        case 6: rec_launch<6>(field, field_cols, pred, nf, r, step, n_nodes, s); break;
        case 7: rec_launch<7>(field, field_cols, pred, nf, r, step, n_nodes, s); break;
        default: rec_launch<8>(field, field_cols, pred, nf, r, step, n_nodes, s); break;
    }
    return g4c::check_launch(me);
}
