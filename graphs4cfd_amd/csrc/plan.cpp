// Host-side builders of the static mesh plan (run once per mesh, not per step).
//
// The reference recomputes all of this inside every forward, with device->host syncs:
//   * PyG scatter(dim_size=None) -> int(index.max())+1           (call at nn/blocks.py:231)
//   * pool_edge: idx.max().item(), remove_self_loops (mask compaction), coalesce (sort+unique)
//                                                                (nn/blocks.py:63-67)
// Topology is loop-invariant in a rollout, so it is hoisted here.
#include <algorithm>
#include <cstdint>
#include <numeric>
#include <vector>

#include "g4c_common.h"

extern "C" int g4c_plan_csr(const int64_t *keys, int64_t n, int64_t n_seg, int32_t *perm, int32_t *off) {
    G4C_REQUIRE(n >= 0 && n_seg >= 0 && n < (1LL << 31) && n_seg < (1LL << 31), G4C_EINVAL,
                "g4c_plan_csr: sizes out of int32 range (n=%lld n_seg=%lld)", (long long)n, (long long)n_seg);
    G4C_REQUIRE((keys || n == 0) && off && (perm || n == 0), G4C_EINVAL, "g4c_plan_csr: null pointer");
    std::fill(off, off + n_seg + 1, 0);
    for (int64_t p = 0; p < n; ++p) {
        const int64_t k = keys[p];
        G4C_REQUIRE(k >= 0 && k < n_seg, G4C_EINVAL, "g4c_plan_csr: key %lld at %lld outside [0, %lld)",
                    (long long)k, (long long)p, (long long)n_seg);
        off[k + 1]++;
    }
    for (int64_t s = 0; s < n_seg; ++s) off[s + 1] += off[s];
    std::vector<int32_t> cur(off, off + n_seg);
    for (int64_t p = 0; p < n; ++p) perm[cur[keys[p]]++] = (int32_t)p;   // stable
    return G4C_OK;
}

// Tiles of whole segments: tile t covers segments [tile_seg[t], tile_seg[t+1]) = rows [tile_rows[t], tile_rows[t+1]), at
// most max_rows rows (greedy, in order; empty segments ride along).  Lets the edge-MLP kernel reduce the messages of the
// targets it has just computed (g4c_mlp_io_t.agg).  Returns the tile count, -1 if a segment exceeds max_rows (then
// the caller keeps the separate g4c_segment_reduce launch), or a negative G4C_E* code.
extern "C" int64_t g4c_plan_tiles(const int32_t *off, int32_t n_seg, int32_t max_rows, int32_t *tile_rows, int32_t *tile_seg,
                                  int64_t capacity) {
    G4C_REQUIRE(off && tile_rows && tile_seg && n_seg >= 0 && max_rows > 0 && capacity >= 1, G4C_EINVAL, "g4c_plan_tiles: bad arguments");
    int64_t nt = 0;
    int32_t s = 0;
    tile_rows[0] = off[0];
    tile_seg[0] = 0;
    while (s < n_seg) {
        const int32_t r0 = off[s];
        int32_t e = s;
        while (e < n_seg && off[e + 1] - r0 <= max_rows) ++e;
        if (e == s) return -1;                          // one segment alone is larger than a tile
        G4C_REQUIRE(nt + 1 < capacity, G4C_EINVAL, "g4c_plan_tiles: capacity %lld too small", (long long)capacity);
        ++nt;
        tile_rows[nt] = off[e];
        tile_seg[nt] = e;
        s = e;
    }
    return nt;
}

// Row ranges for dense pairs over segments of any length (mlp_ws.hip, ANY): the rows are cut into n_wg contiguous ranges on segment
// boundaries, each of at most cap = 64 P rows, for the smallest P for which that many ranges are enough.  What a launch of persistent
// workgroups pays for is the workgroup with the most pairs, and P is that number: tiles of whole segments leave rows of every tile
// unused, which on a grid of 256 can cost a whole round of pairs.  Among the plans with that P the rows are spread evenly (each range
// ends on the boundary nearest to an even share of what is left, as far as the ranges behind it can still hold the rest): a fused
// layer's node phase is proportional to a workgroup's targets.
extern "C" int64_t g4c_plan_row_ranges(const int32_t *off, int32_t n_seg, int32_t n_wg, int32_t *wg_rows, int32_t *wg_seg,
                                       int32_t *max_seg) {
    G4C_REQUIRE(off && wg_rows && wg_seg && max_seg && n_seg >= 0 && n_wg >= 1 && off[0] == 0, G4C_EINVAL, "g4c_plan_row_ranges: bad arguments");
    for (int32_t s = 0; s < n_seg; ++s)
        G4C_REQUIRE(off[s + 1] >= off[s], G4C_EINVAL, "g4c_plan_row_ranges: offsets decrease at segment %d", s);
    const int64_t rows = off[n_seg];
    *max_seg = 0;
    if (rows == 0) {
        for (int32_t i = 0; i <= n_wg; ++i) { wg_rows[i] = 0; wg_seg[i] = i == 0 ? 0 : n_seg; }
        // (no rows: nothing to launch; the segments, all empty, are range 0's on paper)
        *max_seg = n_seg;
        return 0;
    }
    // need[s]: fewest ranges of at most cap rows that cover segments [s, n_seg) (greedy from s is optimal); -1: a segment is too long
    std::vector<int32_t> nxt((size_t)n_seg + 1), need((size_t)n_seg + 1);
    auto count = [&](int64_t cap) -> int64_t {
        int32_t e = n_seg;
        need[(size_t)n_seg] = 0; nxt[(size_t)n_seg] = n_seg;
        for (int32_t s = n_seg - 1; s >= 0; --s) {
            while ((int64_t)off[e] - off[s] > cap) --e;          // furthest boundary a range that starts at s can reach
            if (e == s) { if (off[s + 1] - off[s] > cap) return -1; }
            // (trailing empty segments ride along with the last rows)
            nxt[(size_t)s] = off[e] == off[n_seg] ? n_seg : e;
            need[(size_t)s] = off[s] == off[n_seg] ? 0 : 1 + need[(size_t)nxt[(size_t)s]];
        }
        return need[0];
    };
    int64_t lo = (rows + 64LL * n_wg - 1) / (64LL * n_wg), hi = (rows + 63) / 64;          // (hi: one range holds everything)
    while (lo < hi) {
        const int64_t mid = (lo + hi) / 2, c = count(64 * mid);
        if (c >= 0 && c <= n_wg) hi = mid; else lo = mid + 1;
    }
    const int64_t P = lo, cap = 64 * P;
    count(cap);
    int32_t s = 0;
    wg_rows[0] = 0; wg_seg[0] = 0;
    for (int32_t i = 0; i < n_wg; ++i) {
        const int32_t left = n_wg - i;
        int32_t e;
        if (off[s] == off[n_seg]) e = n_seg;                      // nothing left (an empty range: s == n_seg already)
        else if (left == 1) e = n_seg;
        else {
            const int64_t want = off[s] + (rows - off[s] + left - 1) / left;
            e = (int32_t)(std::lower_bound(off + s, off + n_seg + 1, (int32_t)want) - off);          // first boundary at or behind the even share
            if (e > s && off[e] > want && want - off[e - 1] <= off[e] - want && off[e - 1] > off[s]) --e;      // the nearer one
            if (e > nxt[(size_t)s]) e = nxt[(size_t)s];
            while (off[e] == off[s] || need[(size_t)e] > left - 1) ++e;          // rows in every range; the rest must still fit (e <= nxt[s] holds)
            if (off[e] == off[n_seg]) e = n_seg;
        }
        wg_rows[i + 1] = off[e]; wg_seg[i + 1] = e;
        *max_seg = std::max(*max_seg, e - s);
        s = e;
    }
    return P;
}

extern "C" int64_t g4c_plan_pool_edge_ordered(const int64_t *idx_hr_to_lr, int64_t n_hr, const int64_t *edge_index,
                                              int64_t n_edges, int32_t target_major, int64_t *coarse_edge_index, int32_t *perm,
                                              int32_t *off, int64_t *n_kept) {
    G4C_REQUIRE(n_hr >= 0 && n_edges >= 0 && n_edges < (1LL << 31), G4C_EINVAL, "g4c_plan_pool_edge: bad sizes");
    G4C_REQUIRE((idx_hr_to_lr || n_hr == 0) && (edge_index || n_edges == 0) && off && n_kept, G4C_EINVAL,
                "g4c_plan_pool_edge: null pointer");
    int64_t n_lr = 0;
    for (int64_t i = 0; i < n_hr; ++i) {
        // (-1 is the 'empty' value of the reference's mask2idx tables: a fine node without a coarse node cannot be pooled)
        G4C_REQUIRE(idx_hr_to_lr[i] >= 0, G4C_EINVAL, "g4c_plan_pool_edge: idx_hr_to_lr[%lld] = %lld is negative", (long long)i,
                    (long long)idx_hr_to_lr[i]);
        n_lr = std::max(n_lr, idx_hr_to_lr[i] + 1);
    }
    G4C_REQUIRE(n_lr < (1LL << 31), G4C_EINVAL, "g4c_plan_pool_edge: %lld coarse nodes do not fit int32", (long long)n_lr);
    // surviving fine edges with their coarse endpoints (remove_self_loops), in fine-edge order
    std::vector<int32_t> cr, cc, id;
    cr.reserve((size_t)n_edges); cc.reserve((size_t)n_edges); id.reserve((size_t)n_edges);
    const int64_t *row = edge_index, *col = edge_index + n_edges;
    for (int64_t e = 0; e < n_edges; ++e) {
        G4C_REQUIRE(row[e] >= 0 && row[e] < n_hr && col[e] >= 0 && col[e] < n_hr, G4C_EINVAL,
                    "g4c_plan_pool_edge: edge %lld endpoint outside [0, %lld)", (long long)e, (long long)n_hr);
        const int64_t r = idx_hr_to_lr[row[e]], c = idx_hr_to_lr[col[e]];
        if (r != c) { cr.push_back((int32_t)r); cc.push_back((int32_t)c); id.push_back((int32_t)e); }
    }
    const int64_t kept = (int64_t)id.size();
    *n_kept = kept;
    // stable two-pass counting sort (minor key, then major key): coalesce order = (row, col), target-major = (col, row);
    // ties keep fine-edge order, as the stable comparison sort on row * n_lr + col did
    const std::vector<int32_t> &major = target_major ? cc : cr, &minor = target_major ? cr : cc;
    std::vector<int32_t> order((size_t)kept), tmp((size_t)kept);
    std::vector<int64_t> cnt((size_t)n_lr + 1);
    auto pass = [&](const std::vector<int32_t> &key, const int32_t *in, int32_t *out) {
        std::fill(cnt.begin(), cnt.end(), 0);
        for (int64_t p = 0; p < kept; ++p) ++cnt[(size_t)key[(size_t)in[p]] + 1];
        for (int64_t b = 0; b < n_lr; ++b) cnt[(size_t)b + 1] += cnt[(size_t)b];
        for (int64_t p = 0; p < kept; ++p) out[cnt[(size_t)key[(size_t)in[p]]]++] = in[p];
    };
    for (int64_t p = 0; p < kept; ++p) tmp[(size_t)p] = (int32_t)p;
    pass(minor, tmp.data(), order.data());
    pass(major, order.data(), tmp.data());          // tmp: positions (into cr / cc / id) in final order
    int64_t n_coarse = 0;
    for (int64_t p = 0; p < kept; ++p) {
        const int32_t q = tmp[(size_t)p];
        if (p == 0 || cr[(size_t)q] != cr[(size_t)tmp[(size_t)p - 1]] || cc[(size_t)q] != cc[(size_t)tmp[(size_t)p - 1]]) ++n_coarse;
    }
    int64_t s = -1;
    for (int64_t p = 0; p < kept; ++p) {
        const int32_t q = tmp[(size_t)p];
        if (p == 0 || cr[(size_t)q] != cr[(size_t)tmp[(size_t)p - 1]] || cc[(size_t)q] != cc[(size_t)tmp[(size_t)p - 1]]) {
            ++s;
            off[s] = (int32_t)p;
            coarse_edge_index[s] = cr[(size_t)q];
            coarse_edge_index[n_coarse + s] = cc[(size_t)q];
        }
        perm[p] = id[(size_t)q];
    }
    off[n_coarse] = (int32_t)kept;
    return n_coarse;
}

extern "C" int64_t g4c_plan_pool_edge(const int64_t *idx_hr_to_lr, int64_t n_hr, const int64_t *edge_index,
                                      int64_t n_edges, int64_t *coarse_edge_index, int32_t *perm, int32_t *off,
                                      int64_t *n_kept) {
    return g4c_plan_pool_edge_ordered(idx_hr_to_lr, n_hr, edge_index, n_edges, 0, coarse_edge_index, perm, off, n_kept);
}
