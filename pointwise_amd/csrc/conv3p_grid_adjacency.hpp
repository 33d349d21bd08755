// conv3p_grid_adjacency.hpp -- which segments touch, and segments merged along chosen pairs
// (conv3p_grid_segment_adjacency, conv3p_grid_merge_segments).
//
// include/conv3p.h defines both by the rules E1-E7 and U1-U5 and tests/grid_adjacency_ref.py restates them in numpy.
// Everything is int32 / int64 arithmetic: the result is exact and does not depend on the launch geometry or on thread
// order.  No float arithmetic, no host read.
//
// conv3p_grid_segment_adjacency, 5 + 6 b launches, b the bytes of M - 1 (1 .. 4): fixed by M, whatever the data:
//
//   adj_init_kernel      the edge table emptied, seg_border zeroed, every edge row set to filler, the counters zeroed
//   adj_walk_kernel      a wave takes 64 CONSECUTIVE voxels, a thread per voxel.  Pass one, unrolled over the 27 taps: the
//                        foreign segment b_t behind every tap (registers, and a column of LDS for pass two), the three
//                        counts of E6, and the set of taps that are the LOWEST tap of the voxel reaching their b (a
//                        triangle of compares on registers).  seg_border: runs of equal a among the wave's voxels are
//                        summed by the segmented shuffle of gseg_assign_kernel; a run whose counts are 0 -- the inside
//                        of a floor -- adds nothing.  Pass two, tap by tap, skipped where no lane of the wave has a
//                        contact at that tap: consecutive lanes with the same (a, b_t) form a run; its length is the
//                        run's contacts, the population count of the "lowest tap" ballot under the run its edge_voxels,
//                        and length times the tap's (dx, dy, dz) its offset -- ballots alone, no shuffle of values.  The
//                        run's first lane finds or claims the key a << 32 | b in an open-addressed table (64-bit
//                        compare-and-swap on an empty slot, linear probing, the loop bounded by the table's size: on
//                        exhaustion it sets the overflow word and goes on; no loop waits for a thread) and adds the five
//                        counters with int32 adds.  A floor against a wall is one set of adds per run, not per contact.
//                        Claims are counted too: a lane notes each claim in its word of LDS, and the wave adds its 64
//                        words to the header after every step of 64 voxels.  A lane whose probe passes 64 slots adds
//                        the whole wave's words at once, since the other lanes may be idle behind it.  A count past
//                        max_edges sets the overflow word as well, and once that word is set no call adds or probes
//                        on.  B, the contacts and seg_border do not go through the table, so they stay exact.
//   adj_compact_kernel   the claimed keys, a wave's at a time behind one add of the wave's count: E, and the keys in SLOT
//                        order, which is not reproducible -- the sort makes it so
//   2 b x { adj_sort_hist_kernel, adj_sort_scan_kernel, adj_sort_scatter_kernel }
//                        the stable 8-bit radix passes of conv3p_workgroup.hpp on the 64-bit keys, b passes over the bytes of
//                        dst, then b over the bytes of src; a pass above the top byte of S - 1 returns at once on the
//                        device, and since both halves skip the same number the sorted keys always end in the first
//                        buffer.  On overflow nothing is sorted.
//   adj_finish_kernel    adj_start[s] = the first sorted key not below s << 32 (a binary search per s: the prefix of the
//                        per-source counts without a second pass over the edges), the largest degree;
//                        per edge its slot found again by the probe that made it, the five counters, and the twin by a
//                        binary search for b << 32 | a; the largest edge_contacts
//   adj_stats_kernel     adj_stats
//
// conv3p_grid_merge_segments, seven launches whatever the data:
//
//   merge_init_kernel    parent[s] = s over the segments, the outputs' "past S'" words, the stats started
//   merge_union_kernel   a thread per pair: gseg_union of the active pairs (lock-free, entries only ever decrease)
//   gseg_flatten_kernel, gseg_scan_kernel                 conv3p_grid_segments.hpp's, on segments in place of voxels
//   merge_number_kernel  the root segments numbered in ascending segment: seg_map[root], root_out
//   merge_assign_kernel  seg_map[s] = seg_map[root]; sizes, rows and member counts by integer adds; the label's key
//                        size << 32 | (0x7fffffff - s) by a 64-bit atomicMax
//   merge_finish_kernel  segment_out per voxel; label_out from the key; the maxima; merge_stats
#pragma once

#include "conv3p_grid_segments.hpp"

namespace conv3p {

constexpr int kAdjThreads = 256;
constexpr int kAdjMaxGrid = 2048;
constexpr int kAdjVals = 5;                             // contacts, voxels, offset x y z
constexpr int kAdjSortTile = 4096;
constexpr int kAdjDigitBits = 8;
constexpr int kAdjDigits = 1 << kAdjDigitBits;
constexpr int kAdjScanThreads = 1024;
constexpr int kAdjMaxBytes = 4;                         // of a segment number
constexpr unsigned long long kAdjEmpty = ~0ull;         // no key: a and b are below 2^31
constexpr unsigned long long kAdjSlack = 64;            // slots = 2 max_edges + kAdjSlack
static_assert(kAdjThreads == kAdjDigits, "a thread per digit in adj_sort_hist_kernel");

struct AdjHeader {
    unsigned long long claimed;                         // slots claimed: E unless the table overflowed
    unsigned long long pairs;                           // B
    unsigned long long contacts;
    int overflow;                                       // more than max_edges keys were claimed, or a probe ran out of slots
    int live;                                           // the claims the walk has counted so far
    int max_degree, max_contacts;
};

struct AdjArgs {
    const int32_t *neigh, *segment, *seg_stats, *grid_stats;
    int M, max_edges;
    unsigned tapmask;
    unsigned long long slots;
    int32_t *adj_start, *edge_src, *edge_dst, *edge_contacts, *edge_voxels, *edge_offset, *edge_twin, *seg_border;
    long long *adj_stats;
    // the workspace
    AdjHeader *hdr;
    int *digit_total;                                   // (2 kAdjMaxBytes, kAdjDigits)
    int *hist;                                          // (kAdjDigits, sort_tiles)
    unsigned long long *keys;                           // (slots)
    int32_t *vals;                                      // (slots, kAdjVals)
    unsigned long long *sort_a, *sort_b;                // (max_edges) each
    int sort_tiles;
};

__device__ __forceinline__ unsigned long long adj_key(int a, int b)
{
    return ((unsigned long long)(unsigned)a << 32) | (unsigned long long)(unsigned)b;
}

// The first slot of a key's probe sequence: a 32-bit mix of both halves, scaled to [0, slots).
__device__ __forceinline__ unsigned long long adj_slot(unsigned long long key, unsigned long long slots)
{
    unsigned h = ((unsigned)(key >> 32) * 0x9E3779B1u) ^ ((unsigned)key * 0x85EBCA77u);
    h ^= h >> 15;
    h *= 0x2C1B3C6Du;
    h ^= h >> 12;
    h *= 0x297A2D39u;
    h ^= h >> 15;
    return __umul64hi((unsigned long long)h << 32, slots);
}

// E, or -1 when the edges do not fit (E7).  Read behind the kernel boundary of adj_compact_kernel.
__device__ __forceinline__ int adj_edges(const AdjArgs &p)
{
    const AdjHeader *h = p.hdr;
    return (h->overflow || h->claimed > (unsigned long long)p.max_edges) ? -1 : (int)h->claimed;
}

// The bytes of S - 1 (at least 1): the radix passes that run per half of the key.
__device__ __forceinline__ int adj_bytes(int S)
{
    const unsigned x = S > 0 ? (unsigned)(S - 1) : 0u;
    int nb = 1;
    while (nb < kAdjMaxBytes && (x >> (8 * nb))) ++nb;
    return nb;
}

// The first i in [0, n) with keys[i] >= key, n if there is none.
__device__ __forceinline__ int adj_lower_bound(const unsigned long long *keys, int n, unsigned long long key)
{
    return lower_bound(0, n, [&](int m) { return keys[m] < key; });
}

__global__ __launch_bounds__(kAdjThreads) void adj_init_kernel(const AdjArgs p)
{
    const unsigned long long first = (unsigned long long)blockIdx.x * kAdjThreads + threadIdx.x;
    const unsigned long long step = (unsigned long long)gridDim.x * kAdjThreads;
    for (unsigned long long i = first; i < p.slots; i += step) p.keys[i] = kAdjEmpty;
    for (unsigned long long i = first; i < p.slots * kAdjVals; i += step) p.vals[i] = 0;
    for (unsigned long long i = first; i < (unsigned long long)p.M * 4; i += step) p.seg_border[i] = 0;
    for (unsigned long long i = first; i < (unsigned long long)p.max_edges; i += step) {
        p.edge_src[i] = -1;
        p.edge_dst[i] = -1;
        p.edge_twin[i] = -1;
        p.edge_contacts[i] = 0;
        p.edge_voxels[i] = 0;
        p.edge_offset[3 * i] = 0;
        p.edge_offset[3 * i + 1] = 0;
        p.edge_offset[3 * i + 2] = 0;
    }
    for (unsigned long long i = first; i < 2ull * kAdjMaxBytes * kAdjDigits; i += step) p.digit_total[i] = 0;
    if (first == 0) {
        AdjHeader h;
        h.claimed = h.pairs = h.contacts = 0ull;
        h.overflow = h.live = h.max_degree = h.max_contacts = 0;
        *p.hdr = h;
    }
}

// n claims counted: every claim is a distinct key, so a count past max_edges is E > max_edges for certain -- the overflow
// of E7.
__device__ __forceinline__ void adj_count_claims(const AdjArgs &p, int n)
{
    const int before = atomicAdd(&p.hdr->live, n);
    if ((long long)before + n > (long long)p.max_edges)
        __hip_atomic_store(&p.hdr->overflow, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// n contacts a -> b at tap t, f of them the lowest tap of their voxel towards b: found or claimed, then added; a claim is
// counted in the lane's word of `claims`, the 64 words in LDS of the wave's claims not yet in the header.  Once the
// overflow word is set the edges are lost whatever is added (E7), so the call returns at once.  A probe that grows long
// -- the table is past max_edges keys, or nearly -- hands in the claims of the WHOLE wave (the other lanes may be idle
// behind this one; an exchange takes each word once, whoever takes it) and looks at the overflow word, every 64 slots:
// every claim reaches the header within a bounded number of steps, so a table that fills up is given up by all threads
// instead of being searched slot by slot by each.
__device__ __forceinline__ void adj_add(const AdjArgs &p, int a, int b, int n, int f, int t, int *claims, int lane)
{
    const unsigned long long key = adj_key(a, b);
    unsigned long long i = adj_slot(key, p.slots);
    for (unsigned long long probe = 0; probe < p.slots; ++probe) {     // bounded: no slot is looked at twice
        if ((probe & 63ull) == 0) {
            if (probe) {
                int sum = 0;
                for (int j = 0; j < 64; ++j) sum += atomicExch(&claims[j], 0);
                if (sum) adj_count_claims(p, sum);
            }
            if (__hip_atomic_load(&p.hdr->overflow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
        }
        unsigned long long cur = __hip_atomic_load(p.keys + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == kAdjEmpty) {
            cur = atomicCAS(p.keys + i, kAdjEmpty, key);
            if (cur == kAdjEmpty) {
                cur = key;
                atomicAdd(&claims[lane], 1);
            }
        }
        if (cur == key) {
            int32_t *q = p.vals + i * kAdjVals;
            const int dx = t / 9 - 1, dy = t / 3 % 3 - 1, dz = t % 3 - 1;
            atomicAdd(q, n);
            if (f) atomicAdd(q + 1, f);
            if (dx) atomicAdd(q + 2, n * dx);
            if (dy) atomicAdd(q + 3, n * dy);
            if (dz) atomicAdd(q + 4, n * dz);
            return;
        }
        i = i + 1 == p.slots ? 0ull : i + 1;            // another key's slot
    }
    __hip_atomic_store(&p.hdr->overflow, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kAdjThreads) void adj_walk_kernel(const AdjArgs p)
{
    __shared__ int b_s[kInterpNeigh][kAdjThreads];      // a column per thread: written and read by that thread alone
    __shared__ unsigned long long sum_s[2];
    __shared__ int claims_s[kAdjThreads];               // a word per lane: its claims not yet counted in the header
    const int tid = threadIdx.x, lane = tid & 63;
    int *claims = claims_s + (tid - lane);
    claims_s[tid] = 0;
    if (tid < 2) sum_s[tid] = 0ull;
    __syncthreads();
    const int ne = clamped_count(p.grid_stats, p.M), S = clamped_count(p.seg_stats, p.M);
    unsigned long long n_pairs = 0, n_contacts = 0;
    const long long waves = (long long)gridDim.x * (kAdjThreads / 64);
    for (long long c0 = ((long long)blockIdx.x * (kAdjThreads / 64) + (tid >> 6)) * 64; c0 < ne; c0 += waves * 64) {
        const long long w = c0 + lane;                   // c0 is the wave's: all its lanes take every step
        const int v = (int)w;
        int a = -1;                                      // E1
        if (w < ne) {
            const int s = p.segment[v];
            if (s >= 0 && s < S) a = s;
        }
        const int32_t *row = p.neigh + (size_t)(a >= 0 ? v : 0) * kInterpNeigh;
        int b[kInterpNeigh];
        int k0 = 0, k1 = 0, k2 = 0;
#pragma unroll
        for (int t = 0; t < kInterpNeigh; ++t) {
            int bt = -1;
            if (a >= 0 && ((p.tapmask >> t) & 1u)) {
                const int u = row[t];
                if (u < 0 || u >= ne) {
                    ++k2;
                } else {
                    const int su = p.segment[u];
                    if (su < 0 || su >= S) {
                        ++k1;
                    } else if (su != a) {                // E2
                        bt = su;
                        ++k0;
                    }
                }
            }
            b[t] = bt;
            b_s[t][tid] = bt;
        }
        unsigned first = 0;                              // the taps that are the lowest of this voxel towards their b
#pragma unroll
        for (int t = 0; t < kInterpNeigh; ++t) {
            bool f = b[t] >= 0;
#pragma unroll
            for (int t2 = 0; t2 < t; ++t2) f = f && b[t2] != b[t];
            if (f) first |= 1u << t;
        }
        n_pairs += (unsigned long long)__popc(first);
        n_contacts += (unsigned long long)k0;

        // E6: runs of equal a among the wave's voxels; the run's first lane gets the run's sums (fields below 2^16)
        {
            int w0 = k0 | (k1 << 16), w1 = k2 | (((k0 | k1 | k2) != 0 ? 1 : 0) << 16);
            const int before = __shfl_up(a, 1, 64);
            const bool head = lane == 0 || before != a;
            const unsigned long long heads = __ballot(head);
            const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
            const int end = above ? lane + __ffsll((long long)above) : 64;
            for (int d = 1; d < 64; d <<= 1) {
                const int y0 = __shfl_down(w0, d, 64), y1 = __shfl_down(w1, d, 64);
                if (lane + d < end) {
                    w0 += y0;
                    w1 += y1;
                }
            }
            if (head && a >= 0) {
                int32_t *q = p.seg_border + (size_t)a * 4;
                if (w0 & 0xffff) atomicAdd(q, w0 & 0xffff);
                if (w0 >> 16) atomicAdd(q + 1, w0 >> 16);
                if (w1 & 0xffff) atomicAdd(q + 2, w1 & 0xffff);
                if (w1 >> 16) atomicAdd(q + 3, w1 >> 16);
            }
        }

        // E4: tap by tap, runs of equal (a, b_t) among the wave's voxels
        for (int t = 0; t < kInterpNeigh; ++t) {
            const int bt = b_s[t][tid];
            const bool valid = bt >= 0;
            const unsigned long long valids = __ballot(valid);
            if (!valids) continue;                       // uniform
            const int pa = __shfl_up(a, 1, 64), pb = __shfl_up(bt, 1, 64);
            const bool head = valid && (lane == 0 || pa != a || pb != bt);
            const unsigned long long bound = __ballot(head) | ~valids;          // where a run cannot go on
            const unsigned long long firsts = __ballot(valid && ((first >> t) & 1u));
            if (head) {
                const unsigned long long above = lane == 63 ? 0ull : bound >> (lane + 1);
                const int end = above ? lane + __ffsll((long long)above) : 64;
                const unsigned long long upto = end == 64 ? ~0ull : (1ull << end) - 1ull;
                const unsigned long long mask = upto & ~((1ull << lane) - 1ull);
                adj_add(p, a, bt, end - lane, __popcll(firsts & mask), t, claims, lane);
            }
        }
        int mine = atomicExch(&claims[lane], 0);         // the step's claims, one add a wave
        for (int d = 32; d > 0; d >>= 1) mine += __shfl_xor(mine, d, 64);
        if (lane == 0 && mine) adj_count_claims(p, mine);
    }
    for (int d = 32; d > 0; d >>= 1) {
        n_pairs += (unsigned long long)__shfl_xor((int)n_pairs, d, 64);         // a thread's counts are far below 2^31
        n_contacts += (unsigned long long)__shfl_xor((int)n_contacts, d, 64);
    }
    if (lane == 0) {
        if (n_pairs) atomicAdd(&sum_s[0], n_pairs);
        if (n_contacts) atomicAdd(&sum_s[1], n_contacts);
    }
    __syncthreads();
    if (tid == 0 && sum_s[0]) atomicAdd(&p.hdr->pairs, sum_s[0]);
    if (tid == 1 && sum_s[1]) atomicAdd(&p.hdr->contacts, sum_s[1]);
}

__global__ __launch_bounds__(kAdjThreads) void adj_compact_kernel(const AdjArgs p)
{
    const int tid = threadIdx.x, lane = tid & 63;
    const unsigned long long step = (unsigned long long)gridDim.x * kAdjThreads;
    for (unsigned long long i0 = (unsigned long long)blockIdx.x * kAdjThreads + (tid - lane); i0 < p.slots; i0 += step) {
        const unsigned long long i = i0 + lane;          // i0 is the wave's
        const unsigned long long key = i < p.slots ? p.keys[i] : kAdjEmpty;
        const bool claimed = key != kAdjEmpty;
        const unsigned long long m = __ballot(claimed);
        if (!m) continue;
        unsigned long long base = 0ull;
        if (lane == 0) base = atomicAdd(&p.hdr->claimed, (unsigned long long)__popcll(m));
        const unsigned lo = (unsigned)__shfl((int)(unsigned)base, 0, 64), hi = (unsigned)__shfl((int)(unsigned)(base >> 32), 0, 64);
        const unsigned long long pos = (((unsigned long long)hi << 32) | lo) + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
        if (claimed && pos < (unsigned long long)p.max_edges) p.sort_a[pos] = key;
    }
}

// What a radix pass works on: pass j of half `half` (0: the bytes of dst, 1: of src).  false: the pass does not run.
struct AdjPass {
    int n, tiles, shift, row;
    const unsigned long long *src;
    unsigned long long *dst;
};
__device__ __forceinline__ bool adj_pass(const AdjArgs &p, int half, int j, AdjPass &q)
{
    const int nb = adj_bytes(clamped_count(p.seg_stats, p.M));
    const int E = adj_edges(p);
    if (j >= nb || E <= 0) return false;
    const int ordinal = half * nb + j;                   // among the passes that run: both halves run nb
    q.n = E;
    q.tiles = (E - 1) / kAdjSortTile + 1;               // E > 0; no sum that could leave int32
    q.shift = half * 32 + j * 8;
    q.row = half * kAdjMaxBytes + j;
    q.src = (ordinal & 1) ? p.sort_b : p.sort_a;
    q.dst = (ordinal & 1) ? p.sort_a : p.sort_b;
    return true;
}

__global__ __launch_bounds__(kAdjThreads) void adj_sort_hist_kernel(const AdjArgs p, int half, int j)
{
    __shared__ int hist_s[kAdjDigits];
    AdjPass q;
    if (!adj_pass(p, half, j, q)) return;
    const int tid = threadIdx.x;
    int mine = 0;                                        // this workgroup's keys of digit tid: kAdjThreads == kAdjDigits
    for (int tile = blockIdx.x; tile < q.tiles; tile += gridDim.x)
        mine += radix_hist_tile<kAdjDigitBits>(q.src, (long long)q.n, tile, kAdjSortTile, q.shift, hist_s, p.hist, p.sort_tiles, tid,
                                               kAdjThreads);
    if (mine) atomicAdd(&p.digit_total[q.row * kAdjDigits + tid], mine);
}

// A workgroup per digit: radix_digit_scan from this pass's totals.
__global__ __launch_bounds__(kAdjScanThreads) void adj_sort_scan_kernel(const AdjArgs p, int half, int j)
{
    __shared__ int scan_s[kAdjScanThreads / 64];
    AdjPass q;
    if (!adj_pass(p, half, j, q)) return;
    const int digit = blockIdx.x;
    radix_digit_scan(p.digit_total + q.row * kAdjDigits, p.hist + (size_t)digit * p.sort_tiles, q.tiles, digit, scan_s,
                     threadIdx.x, kAdjScanThreads);
}

// One wave per sort tile: radix_scatter_tile.  64-bit positions in the loop: n may be within a tile of 2^31.
__global__ __launch_bounds__(64) void adj_sort_scatter_kernel(const AdjArgs p, int half, int j)
{
    __shared__ int run_s[kAdjDigits];
    AdjPass q;
    if (!adj_pass(p, half, j, q)) return;
    for (int tile = blockIdx.x; tile < q.tiles; tile += gridDim.x)
        radix_scatter_tile<kAdjDigitBits, long long>(q.src, q.dst, q.n, tile, kAdjSortTile, q.shift, p.hist, p.sort_tiles, run_s,
                                          threadIdx.x);
}

__global__ __launch_bounds__(kAdjThreads) void adj_finish_kernel(const AdjArgs p)
{
    __shared__ int max_s[2];
    const int tid = threadIdx.x;
    if (tid < 2) max_s[tid] = 0;
    __syncthreads();
    const int S = clamped_count(p.seg_stats, p.M);
    const int E = adj_edges(p), n = E < 0 ? 0 : E;       // on overflow: adj_start all 0, the rows stay filler
    const unsigned long long *keys = p.sort_a;
    int md = 0, mc = 0;
    const long long total = (long long)p.M + 1 > (long long)n ? (long long)p.M + 1 : (long long)n;
    for (long long i = (long long)blockIdx.x * kAdjThreads + tid; i < total; i += (long long)gridDim.x * kAdjThreads) {
        if (i <= p.M) {                                  // E5
            int lo = n;
            if (i < S) {
                lo = adj_lower_bound(keys, n, (unsigned long long)i << 32);
                const int deg = adj_lower_bound(keys + lo, n - lo, (unsigned long long)(i + 1) << 32);
                md = deg > md ? deg : md;
            }
            p.adj_start[i] = lo;
        }
        if (i < n) {                                     // E4
            const unsigned long long key = keys[i];
            const int a = (int)(key >> 32), b = (int)(key & 0xffffffffull);
            unsigned long long at = adj_slot(key, p.slots);
            bool found = false;
            for (unsigned long long probe = 0; probe < p.slots; ++probe) {
                const unsigned long long cur = p.keys[at];
                found = cur == key;
                if (found || cur == kAdjEmpty) break;
                at = at + 1 == p.slots ? 0ull : at + 1;
            }
            const int32_t *q = p.vals + at * kAdjVals;
            const int c = found ? q[0] : 0;
            p.edge_src[i] = a;
            p.edge_dst[i] = b;
            p.edge_contacts[i] = c;
            p.edge_voxels[i] = found ? q[1] : 0;
            p.edge_offset[3 * i] = found ? q[2] : 0;
            p.edge_offset[3 * i + 1] = found ? q[3] : 0;
            p.edge_offset[3 * i + 2] = found ? q[4] : 0;
            const unsigned long long back = adj_key(b, a);
            const int tw = adj_lower_bound(keys, n, back);
            p.edge_twin[i] = (tw < n && keys[tw] == back) ? tw : -1;            // there by E3 on a symmetric table
            mc = c > mc ? c : mc;
        }
    }
    for (int d = 32; d > 0; d >>= 1) {
        const int yd = __shfl_xor(md, d, 64), yc = __shfl_xor(mc, d, 64);
        md = yd > md ? yd : md;
        mc = yc > mc ? yc : mc;
    }
    if ((tid & 63) == 0) {
        if (md) atomicMax(&max_s[0], md);
        if (mc) atomicMax(&max_s[1], mc);
    }
    __syncthreads();
    if (tid == 0 && max_s[0]) atomicMax(&p.hdr->max_degree, max_s[0]);
    if (tid == 1 && max_s[1]) atomicMax(&p.hdr->max_contacts, max_s[1]);
}

__global__ __launch_bounds__(64) void adj_stats_kernel(const AdjArgs p)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const AdjHeader h = *p.hdr;
    const int E = adj_edges(p);
    long long *o = p.adj_stats;                          // E7
    o[0] = E;
    o[1] = (long long)h.pairs;
    o[2] = clamped_count(p.seg_stats, p.M);
    o[3] = (long long)h.contacts;
    o[4] = E < 0 ? 0 : h.max_degree;
    o[5] = E < 0 ? 0 : h.max_contacts;
    o[6] = E < 0 ? 1 : 0;
    o[7] = 0;
}

// -------------------------------------------------------------------------------------------------------------- merge
struct MergeArgs {
    const int32_t *segment, *seg_root, *seg_size, *seg_rows, *seg_label, *seg_stats, *pair_a, *pair_b, *select;
    long long P;
    int M, ntiles;
    int32_t *seg_map, *segment_out, *root_out, *size_out, *rows_out, *label_out, *stats_out, *merge_stats;
    // the workspace
    int32_t *tile_count, *lab, *parent, *members;       // per tile of segments; M words each
    unsigned long long *best;                           // (M): seg_size << 32 | (0x7fffffff - s), the largest wins
};

__global__ __launch_bounds__(kGsegThreads) void merge_init_kernel(const MergeArgs p)
{
    const int S = clamped_count(p.seg_stats, p.M);
    if (blockIdx.x == 0 && threadIdx.x < 8) {
        const int i = threadIdx.x;
        p.stats_out[i] = (i >= 1 && i <= 3) ? p.seg_stats[i] : 0;               // U3
        if (i < 4) p.merge_stats[i] = i == 1 ? S : 0;
    }
    for (long long s = (long long)blockIdx.x * kGsegThreads + threadIdx.x; s < p.M; s += (long long)gridDim.x * kGsegThreads) {
        const bool in = s < S;
        p.lab[s] = in ? 0 : -1;
        p.parent[s] = in ? (int)s : -1;
        p.members[s] = 0;
        p.best[s] = 0ull;
        p.seg_map[s] = -1;
        p.root_out[s] = -1;
        p.size_out[s] = 0;
        p.rows_out[s] = 0;
        p.label_out[s] = -1;
    }
}

__global__ __launch_bounds__(kGsegThreads) void merge_union_kernel(const MergeArgs p)
{
    __shared__ int count_s;
    if (threadIdx.x == 0) count_s = 0;
    __syncthreads();
    const int S = clamped_count(p.seg_stats, p.M);
    int n = 0;
    for (long long i = (long long)blockIdx.x * kGsegThreads + threadIdx.x; i < p.P; i += (long long)gridDim.x * kGsegThreads) {
        if (p.select && p.select[i] == 0) continue;      // U1
        const int a = p.pair_a[i], b = p.pair_b[i];
        if (a < 0 || a >= S || b < 0 || b >= S || a == b) continue;
        ++n;
        (void)gseg_union<__HIP_MEMORY_SCOPE_AGENT>(p.parent, a, b);
    }
    if (n) atomicAdd(&count_s, n);
    __syncthreads();
    if (threadIdx.x == 0 && count_s) atomicAdd(&p.merge_stats[2], count_s);
}

// U2: the root segments numbered in ascending segment, behind the tiles' prefix (as gseg_number_kernel).
__global__ __launch_bounds__(kGsegThreads) void merge_number_kernel(const MergeArgs p)
{
    __shared__ int scan_s[kGsegThreads / 64];
    const int tid = threadIdx.x;
    for (int tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
        int base = p.tile_count[tile];
        for (int j = 0; j < kGsegTileSteps; ++j) {        // uniform: every thread takes every step
            const long long w = (long long)tile * kGsegTile + j * kGsegThreads + tid;
            const int s = (int)w;
            const int f = (w < p.M && p.lab[s] >= 0 && p.parent[s] == s) ? 1 : 0;
            int total;
            const int g = base + wg_exscan(f, scan_s, tid, kGsegThreads, &total);
            if (f) {                                     // g < S' <= S
                p.seg_map[s] = g;
                p.root_out[g] = p.seg_root[s];
            }
            base += total;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kGsegThreads) void merge_assign_kernel(const MergeArgs p)
{
    const int S = clamped_count(p.seg_stats, p.M);
    for (long long w = (long long)blockIdx.x * kGsegThreads + threadIdx.x; w < S; w += (long long)gridDim.x * kGsegThreads) {
        const int s = (int)w;
        const int r = p.parent[s];                       // flattened: the group's root segment
        const int g = p.seg_map[r];                      // a root's word: written by merge_number_kernel, not here
        if (r != s) p.seg_map[s] = g;
        const int size = p.seg_size[s], rows = p.seg_rows[s];
        if (size) atomicAdd(&p.size_out[g], size);
        if (rows) atomicAdd(&p.rows_out[g], rows);
        atomicAdd(&p.members[g], 1);
        atomicMax(&p.best[g], ((unsigned long long)(unsigned)(size < 0 ? 0 : size) << 32) | (unsigned)(0x7fffffff - s));
    }
}

__global__ __launch_bounds__(kGsegThreads) void merge_finish_kernel(const MergeArgs p)
{
    __shared__ int red_s[3];
    const int tid = threadIdx.x;
    if (tid < 3) red_s[tid] = 0;
    __syncthreads();
    const int S = clamped_count(p.seg_stats, p.M), groups = clamped_count(p.stats_out, p.M);
    int a = 0, b = 0, many = 0;
    for (long long w = (long long)blockIdx.x * kGsegThreads + tid; w < p.M; w += (long long)gridDim.x * kGsegThreads) {
        const int s = p.segment[w];
        p.segment_out[w] = (s >= 0 && s < S) ? p.seg_map[s] : -1;               // U3
        if (w < groups) {
            const int s_best = 0x7fffffff - (int)(p.best[w] & 0x7fffffffull);   // every group has a member: its root
            p.label_out[w] = s_best < S ? p.seg_label[s_best] : -1;
            const int n = p.size_out[w], r = p.rows_out[w];
            a = n > a ? n : a;
            b = r > b ? r : b;
            many += p.members[w] > 1;
        }
    }
    for (int d = 32; d > 0; d >>= 1) {
        const int ya = __shfl_xor(a, d, 64), yb = __shfl_xor(b, d, 64);
        a = ya > a ? ya : a;
        b = yb > b ? yb : b;
        many += __shfl_xor(many, d, 64);
    }
    if ((tid & 63) == 0) {
        if (a) atomicMax(&red_s[0], a);
        if (b) atomicMax(&red_s[1], b);
        if (many) atomicAdd(&red_s[2], many);
    }
    __syncthreads();
    if (tid < 2 && red_s[tid]) atomicMax(&p.stats_out[4 + tid], red_s[tid]);
    if (tid == 2 && red_s[2]) atomicAdd(&p.merge_stats[3], red_s[2]);
    if (blockIdx.x == 0 && tid == 0) p.merge_stats[0] = groups;
}

}  // namespace conv3p
