// conv3p_grid_match.hpp -- a segmentation scored against ground-truth instances: the overlap table, the one-to-one
// matching at an IoU threshold and the counters of panoptic quality (c3p_grid_match_segments).
//
// include/conv3p_match.h defines the call by the rules M1-M10 and tests/grid_match_ref.py restates them in numpy.
// Everything is int32 / int64 arithmetic: the result is exact and does not depend on the launch geometry or on thread
// order.  No float arithmetic, no host read.
//
// 8 + 9 b launches, b the bytes of max(M, T) - 1 (1 .. 4): fixed by (M, T), whatever the data:
//
//   match_init_kernel    the pair table emptied, the sizes of M3 and class_stats zeroed, every pair row set to filler, the
//                        counters zeroed, and max(S, T) noted for the radix passes
//   match_walk_kernel    a wave takes 64 CONSECUTIVE units, a thread per unit: its (p, t) by M1 / M2 -- the row's voxel and
//                        truth, then the voxel's segment and the instance's class, a wave's 64 of each issued together
//                        before any ballot.  Consecutive lanes with the same (p, t) form a run (ballots alone, as
//                        adj_walk_kernel); the run's first lane finds or claims the key p << 32 | t in the open-addressed
//                        table (adj_slot, 64-bit compare-and-swap on an empty slot, linear probing bounded by the table's
//                        size) and adds the run's length, and adds it to the sizes of M3: one claim and one add per run
//                        and counter, not per unit.  Claims are counted as the adjacency counts them: a count past
//                        max_pairs sets the overflow word, and once it is set no call probes on.  B, the sizes and the
//                        void counts do not go through the table, so they stay exact.
//   adj_compact_kernel, 2 b x { adj_sort_hist_kernel, adj_sort_scan_kernel, adj_sort_scatter_kernel }
//                        conv3p_grid_adjacency.hpp's, as they stand, on the table's keys: P and the keys in ascending (p, t)
//   match_rows_kernel    start by a binary search per segment; per pair its slot found again by the probe that made it:
//                        pair_pred, pair_truth, pair_inter; and the key t << 32 | p into the transpose's buffer
//   b x { adj_sort_hist_kernel, adj_sort_scan_kernel, adj_sort_scatter_kernel }
//                        the passes over the bytes of t alone: they are stable and the input is in ascending p
//   match_transpose_kernel   t_start by a binary search per instance; t_pair by a binary search for p << 32 | t
//   match_pred_kernel    a thread per segment: the best partner among its row (M7), the match (M8), TP / FP (M9).  A row of
//                        more than kMatchShort pairs is left to the whole wave, one such row after another (at most 64),
//                        64 pairs a step, the best by a butterfly of compares.
//   match_truth_kernel   the same per instance through t_pair; FN, the instances and the coverage sums
//   match_stats_kernel   stats
#pragma once

#include "conv3p_grid_adjacency.hpp"

namespace conv3p {

constexpr int kMatchThreads = 256;
constexpr int kMatchMaxGrid = 2048;
constexpr int kMatchShort = 16;                         // pairs of a row a single thread walks
constexpr int kMatchMaxClass = 128;
constexpr int kMatchClassVals = 6;
constexpr int kMatchStats = 16;
constexpr int64_t kMatchMaxUnits = 1 << 24;             // M, N and T: every product of M6 stays below 2^49

struct MatchHeader {
    unsigned long long paired;                          // B
    unsigned long long voids, invalid, missed;
    unsigned long long instances, cover, wcover, tsum;
    int32_t sort_count[8];                              // [0] = max(S, T): what the radix passes size their bytes by
};

struct MatchArgs {
    const int32_t *segment, *seg_stats, *inverse, *grid_stats, *truth, *pred_class, *truth_class;
    int M, T, num_class, rows, num, den, max_pairs;     // rows: 1 a unit is a raw row, 0 a voxel
    long long N;
    int32_t *pred_size, *pred_void, *truth_size, *truth_missed;
    int32_t *pair_pred, *pair_truth, *pair_inter, *start, *t_start, *t_pair;
    int32_t *best_truth, *best_truth_inter, *best_truth_union, *best_pred, *best_pred_inter, *best_pred_union;
    int32_t *pred_match, *truth_match, *pred_iou_q30;
    long long *class_stats, *stats;
    // the workspace
    MatchHeader *hdr;
    int32_t *inter;                                     // (slots): the units of the slot's pair
    AdjArgs t;                                          // the table's keys and the sort by (p, t): hdr, keys, sort_a / b
    AdjArgs u;                                          // the sort by (t, p): its own totals and buffers, t's hdr and hist
};

// A candidate (inter, union, id) against the best so far: a larger IoU by cross-multiplication, the lower id on a tie.
// Products are below 2^49 (M6).  The start is (0, 1, -1), which any pair with inter > 0 beats.
__device__ __forceinline__ void match_better(int ci, int cu, int cid, int &bi, int &bu, int &bid)
{
    const long long l = (long long)ci * bu, r = (long long)bi * cu;
    if (cid >= 0 && (l > r || (l == r && bid >= 0 && cid < bid))) {
        bi = ci;
        bu = cu;
        bid = cid;
    }
}

// The wave's best of the lanes' bests, in every lane.
__device__ __forceinline__ void match_wave_best(int &bi, int &bu, int &bid)
{
    for (int d = 32; d > 0; d >>= 1) {
        const int yi = __shfl_xor(bi, d, 64), yu = __shfl_xor(bu, d, 64), yid = __shfl_xor(bid, d, 64);
        match_better(yi, yu, yid, bi, bu, bid);
    }
}

__device__ __forceinline__ int match_class(const int32_t *cls, int i) { return cls ? cls[i] : 0; }

// M8 on a best partner: the classes agree and are in range, and inter den > num union.
__device__ __forceinline__ bool match_passes(const MatchArgs &p, int cp, int ct, int inter, int uni)
{
    return cp == ct && cp >= 0 && cp < p.num_class && (long long)inter * p.den > (long long)p.num * uni;
}

__device__ __forceinline__ int match_q30(int inter, int uni) { return (int)(((long long)inter << 30) / (long long)uni); }

__global__ __launch_bounds__(kMatchThreads) void match_init_kernel(const MatchArgs p)
{
    const unsigned long long first = (unsigned long long)blockIdx.x * kMatchThreads + threadIdx.x;
    const unsigned long long step = (unsigned long long)gridDim.x * kMatchThreads;
    for (unsigned long long i = first; i < p.t.slots; i += step) {
        p.t.keys[i] = kAdjEmpty;
        p.inter[i] = 0;
    }
    for (unsigned long long i = first; i < (unsigned long long)p.M; i += step) {
        p.pred_size[i] = 0;
        p.pred_void[i] = 0;
    }
    for (unsigned long long i = first; i < (unsigned long long)p.T; i += step) {
        p.truth_size[i] = 0;
        p.truth_missed[i] = 0;
    }
    for (unsigned long long i = first; i < (unsigned long long)p.max_pairs; i += step) {
        p.pair_pred[i] = -1;
        p.pair_truth[i] = -1;
        p.pair_inter[i] = 0;
        p.t_pair[i] = -1;
    }
    for (unsigned long long i = first; i < 2ull * kAdjMaxBytes * kAdjDigits; i += step) {
        p.t.digit_total[i] = 0;
        p.u.digit_total[i] = 0;
    }
    for (unsigned long long i = first; i < (unsigned long long)p.num_class * kMatchClassVals; i += step) p.class_stats[i] = 0;
    if (first == 0) {
        AdjHeader h;
        h.claimed = h.pairs = h.contacts = 0ull;
        h.overflow = h.live = h.max_degree = h.max_contacts = 0;
        *p.t.hdr = h;
        MatchHeader *m = p.hdr;
        m->paired = m->voids = m->invalid = m->missed = m->instances = m->cover = m->wcover = m->tsum = 0ull;
        const int S = clamped_count(p.seg_stats, p.M);
        m->sort_count[0] = S > p.T ? S : p.T;
    }
}

// n units of the pair `key`: found or claimed, then added.  A claim is counted in `mine`, the lane's claims not yet in the
// header; a probe that grows long hands them in and looks at the overflow word every 64 slots, so a table that fills up
// is given up instead of being searched slot by slot.  Once the overflow word is set the pairs are lost whatever is
// added (M5), so the call returns at once.
__device__ __forceinline__ void match_add(const MatchArgs &p, unsigned long long key, int n, int &mine)
{
    const unsigned long long slots = p.t.slots;
    unsigned long long i = adj_slot(key, slots);
    for (unsigned long long probe = 0; probe < slots; ++probe) {       // bounded: no slot is looked at twice
        if ((probe & 63ull) == 0) {
            if (probe && mine) {
                adj_count_claims(p.t, mine);
                mine = 0;
            }
            if (__hip_atomic_load(&p.t.hdr->overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
        }
        unsigned long long cur = __hip_atomic_load(p.t.keys + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == kAdjEmpty) {
            cur = atomicCAS(p.t.keys + i, kAdjEmpty, key);
            if (cur == kAdjEmpty) {
                cur = key;
                ++mine;
            }
        }
        if (cur == key) {
            atomicAdd(p.inter + i, n);
            return;
        }
        i = i + 1 == slots ? 0ull : i + 1;              // another key's slot
    }
    __hip_atomic_store(&p.t.hdr->overflow, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kMatchThreads) void match_walk_kernel(const MatchArgs p)
{
    __shared__ unsigned long long sum_s[4];
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < 4) sum_s[tid] = 0ull;
    __syncthreads();
    const int S = clamped_count(p.seg_stats, p.M);
    const long long units = p.rows ? p.N : (long long)clamped_count(p.grid_stats, p.M);
    unsigned n_paired = 0, n_void = 0, n_invalid = 0, n_missed = 0;           // a thread's counts are far below 2^31
    const long long waves = (long long)gridDim.x * (kMatchThreads / 64);
    for (long long c0 = ((long long)blockIdx.x * (kMatchThreads / 64) + (tid >> 6)) * 64; c0 < units; c0 += waves * 64) {
        const long long w = c0 + lane;                   // c0 is the wave's: all its lanes take every step
        const bool valid = w < units;
        int v = -1, tr = -1;
        if (valid) {                                     // M1: the two loads of the unit, then the two that depend on them
            v = p.rows ? p.inverse[w] : (int)w;
            tr = p.truth[w];
        }
        const bool in_grid = v >= 0 && v < p.M;
        const bool known = tr >= 0 && tr < p.T;
        const int s = in_grid ? p.segment[v] : -1;
        const int c = (known && p.truth_class) ? p.truth_class[tr] : 0;
        const int a = (s >= 0 && s < S) ? s : -1;
        const bool bad = valid && (tr < -1 || tr >= p.T);                     // M2
        const int b = (known && c >= 0 && c < p.num_class) ? tr : -1;
        n_invalid += bad ? 1u : 0u;
        n_void += (valid && b < 0) ? 1u : 0u;

        const int pa = __shfl_up(a, 1, 64), pb = __shfl_up(b, 1, 64);
        const bool head = valid && (lane == 0 || pa != a || pb != b);
        const unsigned long long bound = __ballot(head) | ~__ballot(valid);   // where a run cannot go on
        int mine = 0;
        if (head) {
            const unsigned long long above = lane == 63 ? 0ull : bound >> (lane + 1);
            const int n = (above ? lane + __ffsll((long long)above) : 64) - lane;
            if (a >= 0 && b >= 0) {                      // M3, M4
                n_paired += (unsigned)n;
                atomicAdd(&p.pred_size[a], n);
                atomicAdd(&p.truth_size[b], n);
                match_add(p, adj_key(a, b), n, mine);
            } else if (a >= 0) {
                atomicAdd(&p.pred_void[a], n);
            } else if (b >= 0) {
                n_missed += (unsigned)n;
                atomicAdd(&p.truth_size[b], n);
                atomicAdd(&p.truth_missed[b], n);
            }
        }
        for (int d = 32; d > 0; d >>= 1) mine += __shfl_xor(mine, d, 64);     // the step's claims, one add a wave
        if (lane == 0 && mine) adj_count_claims(p.t, mine);
    }
    for (int d = 32; d > 0; d >>= 1) {
        n_paired += (unsigned)__shfl_xor((int)n_paired, d, 64);
        n_void += (unsigned)__shfl_xor((int)n_void, d, 64);
        n_invalid += (unsigned)__shfl_xor((int)n_invalid, d, 64);
        n_missed += (unsigned)__shfl_xor((int)n_missed, d, 64);
    }
    if (lane == 0) {
        if (n_paired) atomicAdd(&sum_s[0], (unsigned long long)n_paired);
        if (n_void) atomicAdd(&sum_s[1], (unsigned long long)n_void);
        if (n_invalid) atomicAdd(&sum_s[2], (unsigned long long)n_invalid);
        if (n_missed) atomicAdd(&sum_s[3], (unsigned long long)n_missed);
    }
    __syncthreads();
    if (tid == 0 && sum_s[0]) atomicAdd(&p.hdr->paired, sum_s[0]);
    if (tid == 1 && sum_s[1]) atomicAdd(&p.hdr->voids, sum_s[1]);
    if (tid == 2 && sum_s[2]) atomicAdd(&p.hdr->invalid, sum_s[2]);
    if (tid == 3 && sum_s[3]) atomicAdd(&p.hdr->missed, sum_s[3]);
}

__global__ __launch_bounds__(kMatchThreads) void match_rows_kernel(const MatchArgs p)
{
    const int S = clamped_count(p.seg_stats, p.M);
    const int P = adj_edges(p.t), n = P < 0 ? 0 : P;     // on overflow: start all 0, the rows stay filler
    const unsigned long long *keys = p.t.sort_a;
    // the passes over the high half alone are the ordinals nb .. 2 nb - 1 of adj_pass: the first reads sort_b when nb is odd
    const int nb = adj_bytes(clamped_count(p.u.seg_stats, p.u.M));
    unsigned long long *swapped = (nb & 1) ? p.u.sort_b : p.u.sort_a;
    const long long total = (long long)p.M + 1 > (long long)n ? (long long)p.M + 1 : (long long)n;
    for (long long i = (long long)blockIdx.x * kMatchThreads + threadIdx.x; i < total; i += (long long)gridDim.x * kMatchThreads) {
        if (i <= p.M) p.start[i] = i < S ? adj_lower_bound(keys, n, (unsigned long long)i << 32) : n;
        if (i < n) {
            const unsigned long long key = keys[i];
            const int a = (int)(key >> 32), b = (int)(key & 0xffffffffull);
            unsigned long long at = adj_slot(key, p.t.slots);
            bool found = false;
            for (unsigned long long probe = 0; probe < p.t.slots; ++probe) {
                const unsigned long long cur = p.t.keys[at];
                found = cur == key;
                if (found || cur == kAdjEmpty) break;
                at = at + 1 == p.t.slots ? 0ull : at + 1;
            }
            p.pair_pred[i] = a;
            p.pair_truth[i] = b;
            p.pair_inter[i] = found ? p.inter[at] : 0;
            swapped[i] = adj_key(b, a);
        }
    }
}

__global__ __launch_bounds__(kMatchThreads) void match_transpose_kernel(const MatchArgs p)
{
    const int P = adj_edges(p.t), n = P < 0 ? 0 : P;
    const unsigned long long *keys = p.t.sort_a, *tkeys = p.u.sort_a;
    const long long total = (long long)p.T + 1 > (long long)n ? (long long)p.T + 1 : (long long)n;
    for (long long i = (long long)blockIdx.x * kMatchThreads + threadIdx.x; i < total; i += (long long)gridDim.x * kMatchThreads) {
        if (i <= p.T) p.t_start[i] = i < p.T ? adj_lower_bound(tkeys, n, (unsigned long long)i << 32) : n;
        if (i < n) {
            const unsigned long long k = tkeys[i];
            const int r = adj_lower_bound(keys, n, (k << 32) | (k >> 32));
            p.t_pair[i] = r < n ? r : -1;                // there: both buffers hold the same pairs
        }
    }
}

// The class counters of a workgroup, added to class_stats where they are not 0.
__device__ __forceinline__ void match_flush_classes(const MatchArgs &p, const unsigned long long *cls_s, int tid)
{
    for (int i = tid; i < p.num_class * kMatchClassVals; i += kMatchThreads)
        if (cls_s[i]) atomicAdd(reinterpret_cast<unsigned long long *>(p.class_stats) + i, cls_s[i]);
}

__global__ __launch_bounds__(kMatchThreads) void match_pred_kernel(const MatchArgs p)
{
    __shared__ unsigned long long cls_s[kMatchMaxClass * kMatchClassVals];
    const int tid = threadIdx.x, lane = tid & 63;
    for (int i = tid; i < kMatchMaxClass * kMatchClassVals; i += kMatchThreads) cls_s[i] = 0ull;
    __syncthreads();
    const int S = clamped_count(p.seg_stats, p.M);
    const int P = adj_edges(p.t);
    const long long waves = (long long)gridDim.x * (kMatchThreads / 64);
    for (long long c0 = ((long long)blockIdx.x * (kMatchThreads / 64) + (tid >> 6)) * 64; c0 < p.M; c0 += waves * 64) {
        const long long w = c0 + lane;                   // c0 is the wave's
        const int s = (int)w;
        const bool live = w < S && P >= 0;
        const int lo = live ? p.start[s] : 0, hi = live ? p.start[s + 1] : 0;
        const int size = live ? p.pred_size[s] : 0;
        int bi = 0, bu = 1, bt = -1;
        if (hi - lo <= kMatchShort) {
            for (int j = lo; j < hi; ++j) {              // at most kMatchShort steps
                const int t = p.pair_truth[j], in = p.pair_inter[j];
                match_better(in, size + p.truth_size[t] - in, t, bi, bu, bt);
            }
        }
        unsigned long long longs = __ballot(hi - lo > kMatchShort);
        while (longs) {                                  // at most 64 rows, one bit each
            const int src = __ffsll((long long)longs) - 1;
            longs &= longs - 1ull;
            const int rlo = __shfl(lo, src, 64), rhi = __shfl(hi, src, 64), rsize = __shfl(size, src, 64);
            int ci = 0, cu = 1, ct = -1;
            for (int j = rlo + lane; j < rhi; j += 64) {
                const int t = p.pair_truth[j], in = p.pair_inter[j];
                match_better(in, rsize + p.truth_size[t] - in, t, ci, cu, ct);
            }
            match_wave_best(ci, cu, ct);
            if (lane == src) {
                bi = ci;
                bu = cu;
                bt = ct;
            }
        }
        if (w >= p.M) continue;
        int match = -1, q30 = 0;
        if (live) {
            const int cp = match_class(p.pred_class, s);
            if (bt >= 0 && match_passes(p, cp, match_class(p.truth_class, bt), bi, bu)) {
                match = bt;
                q30 = match_q30(bi, bu);
            }
            if (cp >= 0 && cp < p.num_class) {           // M9
                unsigned long long *q = cls_s + cp * kMatchClassVals;
                atomicAdd(q + 5, 1ull);
                if (match >= 0) {
                    atomicAdd(q, 1ull);
                    atomicAdd(q + 3, (unsigned long long)q30);
                } else if (!(p.pred_void[s] > size)) {
                    atomicAdd(q + 1, 1ull);
                }
            }
        }
        p.best_truth[s] = bt;
        p.best_truth_inter[s] = bt >= 0 ? bi : 0;
        p.best_truth_union[s] = bt >= 0 ? bu : 0;
        p.pred_match[s] = match;
        p.pred_iou_q30[s] = q30;
    }
    __syncthreads();
    match_flush_classes(p, cls_s, tid);
}

__global__ __launch_bounds__(kMatchThreads) void match_truth_kernel(const MatchArgs p)
{
    __shared__ unsigned long long cls_s[kMatchMaxClass * kMatchClassVals];
    __shared__ unsigned long long sum_s[4];
    const int tid = threadIdx.x, lane = tid & 63;
    for (int i = tid; i < kMatchMaxClass * kMatchClassVals; i += kMatchThreads) cls_s[i] = 0ull;
    if (tid < 4) sum_s[tid] = 0ull;
    __syncthreads();
    const int P = adj_edges(p.t);
    unsigned long long n_inst = 0, cover = 0, wcover = 0, tsum = 0;
    const long long waves = (long long)gridDim.x * (kMatchThreads / 64);
    for (long long c0 = ((long long)blockIdx.x * (kMatchThreads / 64) + (tid >> 6)) * 64; c0 < p.T; c0 += waves * 64) {
        const long long w = c0 + lane;                   // c0 is the wave's
        const int t = (int)w;
        const bool in = w < p.T, live = in && P >= 0;
        const int lo = live ? p.t_start[t] : 0, hi = live ? p.t_start[t + 1] : 0;
        const int size = in ? p.truth_size[t] : 0;
        int bi = 0, bu = 1, bp = -1;
        if (hi - lo <= kMatchShort) {
            for (int j = lo; j < hi; ++j) {              // at most kMatchShort steps
                const int r = p.t_pair[j];               // a row of the table: match_transpose_kernel found it
                if (r < 0) continue;
                const int s = p.pair_pred[r], n = p.pair_inter[r];
                match_better(n, size + p.pred_size[s] - n, s, bi, bu, bp);
            }
        }
        unsigned long long longs = __ballot(hi - lo > kMatchShort);
        while (longs) {                                  // at most 64 rows, one bit each
            const int src = __ffsll((long long)longs) - 1;
            longs &= longs - 1ull;
            const int rlo = __shfl(lo, src, 64), rhi = __shfl(hi, src, 64), rsize = __shfl(size, src, 64);
            int ci = 0, cu = 1, cp = -1;
            for (int j = rlo + lane; j < rhi; j += 64) {
                const int r = p.t_pair[j];
                if (r < 0) continue;
                const int s = p.pair_pred[r], n = p.pair_inter[r];
                match_better(n, rsize + p.pred_size[s] - n, s, ci, cu, cp);
            }
            match_wave_best(ci, cu, cp);
            if (lane == src) {
                bi = ci;
                bu = cu;
                bp = cp;
            }
        }
        if (!in) continue;
        int match = -1;
        const int ct = match_class(p.truth_class, t);
        if (bp >= 0 && match_passes(p, match_class(p.pred_class, bp), ct, bi, bu)) match = bp;
        if (size > 0) {
            ++n_inst;
            tsum += (unsigned long long)size;
            if (bp >= 0) {                               // M10: the coverage of the best partner
                const unsigned long long q = (unsigned long long)match_q30(bi, bu);
                cover += q;
                wcover += q * (unsigned long long)size;
            }
            if (P >= 0 && ct >= 0 && ct < p.num_class) { // M9; on overflow class_stats stays 0 (M5)
                unsigned long long *q = cls_s + ct * kMatchClassVals;
                atomicAdd(q + 4, 1ull);
                if (match < 0) atomicAdd(q + 2, 1ull);
            }
        }
        p.best_pred[t] = bp;
        p.best_pred_inter[t] = bp >= 0 ? bi : 0;
        p.best_pred_union[t] = bp >= 0 ? bu : 0;
        p.truth_match[t] = match;
    }
    if (n_inst) {
        atomicAdd(&sum_s[0], n_inst);
        atomicAdd(&sum_s[3], tsum);
    }
    if (cover) {
        atomicAdd(&sum_s[1], cover);
        atomicAdd(&sum_s[2], wcover);
    }
    __syncthreads();
    if (tid == 0 && sum_s[0]) atomicAdd(&p.hdr->instances, sum_s[0]);
    if (tid == 1 && sum_s[1]) atomicAdd(&p.hdr->cover, sum_s[1]);
    if (tid == 2 && sum_s[2]) atomicAdd(&p.hdr->wcover, sum_s[2]);
    if (tid == 3 && sum_s[3]) atomicAdd(&p.hdr->tsum, sum_s[3]);
    match_flush_classes(p, cls_s, tid);
}

__global__ __launch_bounds__(64) void match_stats_kernel(const MatchArgs p)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const MatchHeader *h = p.hdr;
    const int P = adj_edges(p.t);
    long long *o = p.stats;                              // M10
    o[0] = P;
    o[1] = (long long)h->paired;
    o[2] = clamped_count(p.seg_stats, p.M);
    o[3] = (long long)h->instances;
    o[4] = (long long)h->voids;
    o[5] = (long long)h->invalid;
    o[6] = (long long)h->missed;
    o[7] = P < 0 ? 1 : 0;
    o[8] = (long long)h->cover;
    o[9] = (long long)h->wcover;
    o[10] = (long long)h->tsum;
    o[11] = o[12] = o[13] = o[14] = o[15] = 0;
}

}  // namespace conv3p
