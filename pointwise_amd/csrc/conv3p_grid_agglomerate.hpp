// conv3p_grid_agglomerate.hpp -- small groups of segments folded into the neighbour they touch most, round after round, on
// the device (conv3p_grid_agglomerate_segments).
//
// include/conv3p_graph.h defines it by the rules H1-H10 and tests/grid_agglomerate_ref.py restates them in numpy.
// Everything is int32 / int64 arithmetic: the result is exact and does not depend on the launch geometry or on thread
// order.  No float arithmetic, no host read.  What a round costs is the E edges of the input graph and the slots of the
// table, not the 26 M taps of the voxel walk: after a merge the new graph is the old one with its endpoints renamed and
// its parallel edges summed.
//
// 15 + 6 R + 6 b launches, R = max_rounds and b the bytes of M - 1 (1 .. 4): fixed by (M, max_rounds), whatever the data.
//
//   agg_init_kernel      every segment its own group: grp[s] = s, W and the label key size << 32 | (0x7fffffff - s) per
//                        segment, best emptied, the log and the graph's rows set to filler, the table emptied, H1 decided
//   R x {
//     agg_contract_kernel  a thread per INPUT edge: (grp[src], grp[dst]) found or claimed in the open-addressed table of
//                          conv3p_grid_adjacency.hpp (the same hash, the same layout of a key and five counters; 64-bit
//                          compare-and-swap on an empty slot, linear probing, the loop bounded by the table's size) and
//                          the contacts and the offset added with int32 adds; an edge inside a group is skipped.  The
//                          combined edges never exceed E <= max_edges, and the table has 2 max_edges + 64 slots: it
//                          cannot fill.
//     agg_choose_kernel    a thread per slot: a combined edge (g, h) with g small and h a candidate (H3) offers H4's
//                          key to best[g] by ONE 64-bit atomicMax -- the degree of a large group serialises no thread
//     agg_count_kernel     the log rows of every tile of kGsegTile segments (a proposal, but of a mutual pair the lower
//                          root's only)
//     agg_scan_kernel      one workgroup: the tiles' exclusive prefix (wg_exscan_inplace); the log's length so far; a
//                          round with no row sets the `done` word
//     agg_log_kernel       the rows behind the tiles' prefix, in ascending root (wg_exscan); gseg_union of every proposer
//                          with its target
//     agg_flatten_kernel   grp[s] = the root of s; W and the label key of a root that was given away move to its new
//                          root (integer add, 64-bit atomicMax) and are zeroed, so that they move once; best and the
//                          table emptied for the next round
//   }                    once `done` is set every kernel of every later round returns at once
//   agg_contract_kernel, agg_choose_kernel   once more on the state after the last round (nothing to do if `done`)
//   agg_census_kernel    the small groups that are left, and those of them that still have a candidate; the table emptied
//   the seven launches of conv3p_grid_merge_segments on (log_a, log_b): H7 holds by construction
//   agg_contract_kernel  the input edges under seg_map: the contracted graph in the result's numbers
//   adj_compact_kernel, 2 b x { adj_sort_hist_kernel, adj_sort_scan_kernel, adj_sort_scatter_kernel }, adj_finish_kernel
//                        conv3p_grid_adjacency.hpp's, through their argument struct, on the result's stats: E4 / E5
//   agg_finish_kernel    voxel_label per voxel; agg_stats
//
// edge_voxels and seg_border[:, 3] are not additive under a merge and are not produced (H8): adj_finish_kernel's
// edge_voxels goes to a column of the workspace.
#pragma once

#include "conv3p_grid_adjacency.hpp"

namespace conv3p {

constexpr int kAggMaxRounds = 32;

struct AggHeader {
    int edges;                                          // E of H1, 0 for an unusable input
    int unusable;
    int done;                                           // a round had no proposal, or the input is unusable
    int rounds, logged, log_base;                       // rounds that had a proposal; log rows so far; before this round
    int small, candidates;                              // agg_stats[4], [5]
};

struct AggArgs {
    const int32_t *seg_size, *seg_rows, *seg_label, *seg_stats;
    const int32_t *edge_src, *edge_dst, *edge_contacts, *edge_offset;
    const long long *adj_stats;
    int M, ntiles, min_size, weight, same_label, min_contacts;
    int32_t *log_a, *log_b, *log_round, *log_contacts;
    const int32_t *seg_map, *segment_out, *label_out, *stats_out;               // the merge's, read behind it
    int32_t *voxel_label;
    long long *agg_stats;
    AdjArgs t;                                          // the table, the sort's buffers and the graph's output arrays
    // the workspace
    AggHeader *hdr;
    int32_t *grp, *weight_of, *tile_count;              // (M), (M), per tile of segments
    unsigned long long *label_key, *best;               // (M) each
};

__device__ __forceinline__ int agg_done(const AggArgs &p)
{
    return __hip_atomic_load(&p.hdr->done, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The table emptied: every key, every counter.
__device__ __forceinline__ void agg_clear_table(const AdjArgs &t, unsigned long long first, unsigned long long step)
{
    for (unsigned long long i = first; i < t.slots; i += step) t.keys[i] = kAdjEmpty;
    for (unsigned long long i = first; i < t.slots * kAdjVals; i += step) t.vals[i] = 0;
}

// H4: the root a key of best[] proposes to.
__device__ __forceinline__ int agg_target(unsigned long long key) { return 0x7fffffff - (int)(key & 0x7fffffffull); }

// H6: whether root s, whose best is `key` (not 0), writes a log row: always, but of a mutual pair only the lower root.
__device__ __forceinline__ bool agg_logs(const AggArgs &p, int s, unsigned long long key)
{
    const int h = agg_target(key);
    const unsigned long long back = p.best[h];
    return !(back != 0ull && agg_target(back) == s) || s < h;
}

__global__ __launch_bounds__(kAdjThreads) void agg_init_kernel(const AggArgs p)
{
    const unsigned long long first = (unsigned long long)blockIdx.x * kAdjThreads + threadIdx.x;
    const unsigned long long step = (unsigned long long)gridDim.x * kAdjThreads;
    const int S = clamped_count(p.seg_stats, p.M);
    agg_clear_table(p.t, first, step);
    for (unsigned long long i = first; i < (unsigned long long)p.M; i += step) {
        const bool in = i < (unsigned long long)S;
        const int size = in ? p.seg_size[i] : 0;
        p.grp[i] = in ? (int)i : -1;
        p.weight_of[i] = in ? (p.weight ? p.seg_rows[i] : size) : 0;
        p.label_key[i] = in ? ((unsigned long long)(unsigned)(size < 0 ? 0 : size) << 32) | (unsigned)(0x7fffffff - (int)i) : 0ull;
        p.best[i] = 0ull;
        p.log_a[i] = -1;
        p.log_b[i] = -1;
        p.log_round[i] = -1;
        p.log_contacts[i] = 0;
    }
    for (unsigned long long i = first; i < (unsigned long long)p.t.max_edges; i += step) {
        p.t.edge_src[i] = -1;
        p.t.edge_dst[i] = -1;
        p.t.edge_twin[i] = -1;
        p.t.edge_contacts[i] = 0;
        p.t.edge_offset[3 * i] = 0;
        p.t.edge_offset[3 * i + 1] = 0;
        p.t.edge_offset[3 * i + 2] = 0;
    }
    for (unsigned long long i = first; i < 2ull * kAdjMaxBytes * kAdjDigits; i += step) p.t.digit_total[i] = 0;
    if (first == 0) {
        const long long E = p.adj_stats[0];
        const int bad = (E < 0 || E > (long long)p.t.max_edges) ? 1 : 0;          // H1
        AdjHeader h;
        h.claimed = h.pairs = h.contacts = 0ull;
        h.overflow = bad;                                // adj_edges() < 0: nothing sorted, start all 0, the rows stay filler
        h.live = h.max_degree = h.max_contacts = 0;
        *p.t.hdr = h;
        AggHeader a;
        a.edges = bad ? 0 : (int)E;
        a.unusable = a.done = bad;
        a.rounds = a.logged = a.log_base = a.small = a.candidates = 0;
        *p.hdr = a;
    }
}

// The input edges under `map` (grp in a round, seg_map behind the merge), parallel edges summed in the table.
__global__ __launch_bounds__(kAdjThreads) void agg_contract_kernel(const AggArgs p, const int32_t *map, int last)
{
    if (!last && agg_done(p)) return;
    const int S = clamped_count(p.seg_stats, p.M), E = p.hdr->edges;
    const AdjArgs &t = p.t;
    for (long long e = (long long)blockIdx.x * kAdjThreads + threadIdx.x; e < E; e += (long long)gridDim.x * kAdjThreads) {
        const int a = p.edge_src[e], b = p.edge_dst[e];
        if (a < 0 || a >= S || b < 0 || b >= S) continue;                       // H1
        const int g = map[a], h = map[b];
        if (g == h || g < 0 || h < 0) continue;
        const unsigned long long key = adj_key(g, h);
        unsigned long long i = adj_slot(key, t.slots);
        for (unsigned long long probe = 0; probe < t.slots; ++probe) {           // bounded: no slot is looked at twice
            unsigned long long cur = __hip_atomic_load(t.keys + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == kAdjEmpty) {
                cur = atomicCAS(t.keys + i, kAdjEmpty, key);
                if (cur == kAdjEmpty) cur = key;
            }
            if (cur == key) {
                int32_t *q = t.vals + i * kAdjVals;
                const int c = p.edge_contacts[e], ox = p.edge_offset[3 * e], oy = p.edge_offset[3 * e + 1], oz = p.edge_offset[3 * e + 2];
                if (c) atomicAdd(q, c);
                if (ox) atomicAdd(q + 2, ox);
                if (oy) atomicAdd(q + 3, oy);
                if (oz) atomicAdd(q + 4, oz);
                break;
            }
            i = i + 1 == t.slots ? 0ull : i + 1;         // another key's slot
        }
    }
}

// H2: the label of the group whose root is g.
__device__ __forceinline__ int agg_label(const AggArgs &p, int g)
{
    return p.seg_label[0x7fffffff - (int)(p.label_key[g] & 0x7fffffffull)];
}

__global__ __launch_bounds__(kAdjThreads) void agg_choose_kernel(const AggArgs p)
{
    if (agg_done(p)) return;
    const AdjArgs &t = p.t;
    const unsigned long long step = (unsigned long long)gridDim.x * kAdjThreads;
    for (unsigned long long i = (unsigned long long)blockIdx.x * kAdjThreads + threadIdx.x; i < t.slots; i += step) {
        const unsigned long long key = t.keys[i];
        if (key == kAdjEmpty) continue;
        const int g = (int)(key >> 32), h = (int)(key & 0xffffffffull);
        const int c = t.vals[i * kAdjVals];
        if (p.weight_of[g] >= p.min_size || c < p.min_contacts) continue;       // H3
        if (p.same_label && agg_label(p, g) != agg_label(p, h)) continue;
        const unsigned long long large = p.weight_of[h] >= p.min_size ? 1ull : 0ull;
        atomicMax(&p.best[g], (large << 62) | ((unsigned long long)(unsigned)c << 31) | (unsigned long long)(unsigned)(0x7fffffff - h));
    }
}

__global__ __launch_bounds__(kGsegThreads) void agg_count_kernel(const AggArgs p)
{
    __shared__ int count_s;
    if (agg_done(p)) return;
    const int tid = threadIdx.x;
    const int S = clamped_count(p.seg_stats, p.M);
    for (int tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
        if (tid == 0) count_s = 0;
        __syncthreads();
        int n = 0;
        for (int j = 0; j < kGsegTileSteps; ++j) {
            const long long s = (long long)tile * kGsegTile + j * kGsegThreads + tid;
            if (s >= S) break;
            const unsigned long long key = p.best[s];
            n += (key != 0ull && agg_logs(p, (int)s, key)) ? 1 : 0;
        }
        if (n) atomicAdd(&count_s, n);
        __syncthreads();
        if (tid == 0) p.tile_count[tile] = count_s;
        __syncthreads();
    }
}

__global__ __launch_bounds__(kGsegScanThreads) void agg_scan_kernel(const AggArgs p)
{
    __shared__ int scan_s[kGsegScanThreads / 64];
    if (agg_done(p)) return;                             // every thread reads it before the barriers below, thread 0 writes behind them
    const int total = wg_exscan_inplace(p.tile_count, p.ntiles, scan_s, (int)threadIdx.x, kGsegScanThreads);
    if (threadIdx.x == 0) {
        AggHeader *h = p.hdr;
        h->log_base = h->logged;
        h->logged += total;
        if (total) ++h->rounds;
        else __hip_atomic_store(&h->done, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(kGsegThreads) void agg_log_kernel(const AggArgs p, int round)
{
    __shared__ int scan_s[kGsegThreads / 64];
    if (agg_done(p)) return;
    const int tid = threadIdx.x;
    const int S = clamped_count(p.seg_stats, p.M), log_base = p.hdr->log_base;
    for (int tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
        int base = log_base + p.tile_count[tile];
        for (int j = 0; j < kGsegTileSteps; ++j) {        // uniform: every thread takes every step
            const long long w = (long long)tile * kGsegTile + j * kGsegThreads + tid;
            const int s = (int)w;
            const unsigned long long key = w < S ? p.best[s] : 0ull;
            const int f = (key != 0ull && agg_logs(p, s, key)) ? 1 : 0;
            int total;
            const int row = base + wg_exscan(f, scan_s, tid, kGsegThreads, &total);
            if (f && row < p.M) {                        // H6: P = S - S' < M
                const int h = agg_target(key);
                p.log_a[row] = s;
                p.log_b[row] = h;
                p.log_round[row] = round;
                p.log_contacts[row] = (int)((key >> 31) & 0x7fffffffull);
                (void)gseg_union<__HIP_MEMORY_SCOPE_AGENT>(p.grp, s, h);
            }
            base += total;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kAdjThreads) void agg_flatten_kernel(const AggArgs p)
{
    if (agg_done(p)) return;
    const unsigned long long first = (unsigned long long)blockIdx.x * kAdjThreads + threadIdx.x;
    const unsigned long long step = (unsigned long long)gridDim.x * kAdjThreads;
    const int S = clamped_count(p.seg_stats, p.M);
    for (unsigned long long w = first; w < (unsigned long long)S; w += step) {
        const int s = (int)w;
        int x = s, q = gseg_load<__HIP_MEMORY_SCOPE_AGENT>(p.grp + x);
        while (q != x) {                                 // strictly decreasing: ends
            x = q;
            q = gseg_load<__HIP_MEMORY_SCOPE_AGENT>(p.grp + x);
        }
        if (x != s) {                                    // s is no root: nobody adds to its words, x's thread leaves x's alone
            __hip_atomic_store(p.grp + s, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const int wt = p.weight_of[s];
            const unsigned long long lk = p.label_key[s];
            if (wt) {
                atomicAdd(&p.weight_of[x], wt);
                p.weight_of[s] = 0;
            }
            if (lk) {
                atomicMax(&p.label_key[x], lk);
                p.label_key[s] = 0ull;
            }
        }
        p.best[s] = 0ull;
    }
    agg_clear_table(p.t, first, step);
}

__global__ __launch_bounds__(kAdjThreads) void agg_census_kernel(const AggArgs p)
{
    __shared__ int sum_s[2];
    const int tid = threadIdx.x;
    if (tid < 2) sum_s[tid] = 0;
    __syncthreads();
    const unsigned long long first = (unsigned long long)blockIdx.x * kAdjThreads + tid;
    const unsigned long long step = (unsigned long long)gridDim.x * kAdjThreads;
    const int S = clamped_count(p.seg_stats, p.M);
    int small = 0, cand = 0;
    for (unsigned long long w = first; w < (unsigned long long)S; w += step) {
        if (p.grp[w] != (int)w || p.weight_of[w] >= p.min_size) continue;
        ++small;
        cand += p.best[w] != 0ull;
    }
    for (int d = 32; d > 0; d >>= 1) {
        small += __shfl_xor(small, d, 64);
        cand += __shfl_xor(cand, d, 64);
    }
    if ((tid & 63) == 0) {
        if (small) atomicAdd(&sum_s[0], small);
        if (cand) atomicAdd(&sum_s[1], cand);
    }
    __syncthreads();
    if (tid == 0 && sum_s[0]) atomicAdd(&p.hdr->small, sum_s[0]);
    if (tid == 1 && sum_s[1]) atomicAdd(&p.hdr->candidates, sum_s[1]);
    agg_clear_table(p.t, first, step);
}

__global__ __launch_bounds__(kGsegThreads) void agg_finish_kernel(const AggArgs p)
{
    const int groups = clamped_count(p.stats_out, p.M);
    for (long long v = (long long)blockIdx.x * kGsegThreads + threadIdx.x; v < p.M; v += (long long)gridDim.x * kGsegThreads) {
        const int g = p.segment_out[v];
        p.voxel_label[v] = (g >= 0 && g < groups) ? p.label_out[g] : -1;        // H7
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const AggHeader h = *p.hdr;
        const int E = adj_edges(p.t);
        long long *o = p.agg_stats;                      // H9
        o[0] = groups;
        o[1] = clamped_count(p.seg_stats, p.M);
        o[2] = h.rounds;
        o[3] = h.logged;
        o[4] = h.small;
        o[5] = h.candidates;
        o[6] = h.unusable;
        o[7] = E < 0 ? 0 : E;
    }
}

}  // namespace conv3p
