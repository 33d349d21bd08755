// conv3p_grid_segments.hpp -- connected segments of voxel labels over the 27-cell neighbour table, and the one-pass
// clean-up of small segments (conv3p_grid_segments, conv3p_grid_absorb_segments).
//
// include/conv3p.h defines both by the rules S1-S4 and A1-A4 and tests/grid_segments_ref.py restates them in numpy.
// Everything is int32 arithmetic: the result is exact and does not depend on the launch geometry or on thread order.
//
// conv3p_grid_segments, seven launches whatever the data (the first two kernels are gseg_local_body / gseg_link_body with
// the join rule "labels equal"; conv3p_grid_smooth.hpp runs the same bodies under a smoothness rule):
//
//   gseg_local_kernel     a workgroup per tile of 1024 CONSECUTIVE voxels, a thread per voxel: lab[v] by S1 (-1: unlabelled);
//                        the union-find below on a copy of the tile in LDS, over the taps whose neighbour lies in the same
//                        tile (voxels are numbered in ascending cell, so a tile is a few columns or a slab of the lattice
//                        and holds most of its own links along the fastest axes); parent[v] = the root of v within the tile.
//                        The per-segment outputs are set to their "past S" words and seg_stats is started.
//   gseg_link_kernel      the union-find by minimum over the taps that leave the tile.  A thread per voxel walks the taps
//                        t < 13: the table is symmetric below ne, so the taps 14 .. 26 of v are the taps 12 .. 0 of its
//                        neighbours and half the table is enough.  A tap that joins u and v links the larger ROOT under
//                        the smaller by a compare-and-swap; the thread carries its set's root from tap to tap, so a tap
//                        whose voxels are joined already costs two finds and no swap.  What was measured on the way, on a
//                        field of ONE label at 257 000 voxels: a lane per tap on parent[v] = v, 2.4 ms (the 13 lanes of a
//                        voxel contend for one root, every voxel is a node of long chains); a thread per voxel on a forest
//                        pre-linked to the first neighbour below, 1.3 ms (every voxel walks a chain of a hundred voxels
//                        through memory once, all at the same time); the tiles, whose roots are few and are compressed by
//                        the thousands of finds that cross them: the numbers of DESIGN.md 5k.
//
//                        Progress.  parent[x] <= x always, and an entry only ever DECREASES: it starts at or below x, the
//                        CAS replaces a root's own number by a smaller root, and the path halving in gseg_find is an atomic minimum
//                        with an ancestor.  So (a) gseg_find follows a strictly decreasing chain and ends after at most x
//                        steps whatever other threads do, and (b) a CAS on root h fails only when parent[h] != h, that is
//                        when ANOTHER thread's CAS on h has succeeded in between; at most one CAS ever succeeds per voxel,
//                        so all threads together retry fewer times than there are labelled voxels.  No loop waits for a
//                        thread to arrive, reads a flag or needs two workgroups to be resident together; a lane that runs
//                        alone to the end of the kernel finishes its union.  A stale read of parent only shows an older,
//                        larger ancestor: the CAS then fails and hands back the current one.
//   gseg_flatten_kernel   parent[v] = the root of v, behind the kernel boundary, so the forest is final: no atomics on the
//                        links.  In place: a word is read either before or after its own flattening and both are ancestors
//                        on the path to the same root.  Also the roots of every tile of kGsegTile voxels.
//   gseg_scan_kernel      one workgroup: exclusive prefix of the tiles' counts (wg_exscan_inplace); S
//   gseg_number_kernel    roots numbered in ascending voxel number: segment[root], seg_root, seg_label
//   gseg_assign_kernel    segment[v] = segment[root] (roots are only read here), sizes and rows by integer adds: runs of
//                        equal segment among the consecutive voxels of a wave are summed by a segmented shuffle and carried
//                        from step to step first, so a floor that is one segment costs one add per 1024 voxels, not one a
//                        voxel (one add a wave of 64 was measured first: 743 us of adds to one word at 4.1 million voxels
//                        of one label); the labelled / unlabelled counts
//   gseg_max_kernel       the largest size and rows, by integer atomicMax behind a wave and a workgroup maximum
//
// conv3p_grid_absorb_segments, six launches whatever the data:
//
//   absorb_count_kernel  small segments and their voxels per tile of segments (A1); absorb_stats zeroed
//   gseg_scan_kernel      both prefixes; the number of small segments stays on the device
//   absorb_plan_kernel   small_list[k] = s, small_off[k] = cursor[s] = the start of s's members; seg_label_out preset
//   absorb_scatter_kernel  a counting scatter by segment: members of the small segments (any order: votes are counts)
//   absorb_vote_kernel   a wave per small segment, waves looping over the list: 32 lanes a member, lane t < 27 tap t, two
//                        members a step, the members looped over (no cap on a small segment's length); votes into a
//                        histogram of 128 int32 in LDS per wave, then the arg-max with the lowest class winning a tie
//   absorb_labels_kernel labels_out per voxel (A4)
//
// The workspaces are 2 M and 4 M words plus the tiles' counts: O(M), whatever num_class.
#pragma once

#include "conv3p_grid_interp.hpp"

namespace conv3p {

constexpr int kGsegThreads = 256;
constexpr int kGsegMaxGrid = 2048;
constexpr int kGsegTileSteps = 8;
constexpr int kGsegTile = kGsegThreads * kGsegTileSteps;   // voxels (or segments) per tile of the two-level scans
constexpr int kGsegScanThreads = 1024;
constexpr int kGsegLocalTile = 1024;                      // consecutive voxels joined in LDS first, a thread each
constexpr int kGsegHalfTaps = 13;                         // the taps below the voxel's own: the table is symmetric
constexpr int kGsegMaxClass = 128;
constexpr size_t kGsegHeaderBytes = 256;

// The union-find's three steps, on the device's parent array (kScope the agent) or on a tile's copy in LDS (kScope the
// workgroup).
template <int kScope> __device__ __forceinline__ int gseg_load(const int32_t *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, kScope);
}

// The root of x.  Every step goes to a strictly smaller voxel, so the walk ends whatever other threads do.  Path halving:
// x's entry is lowered to its grandparent by an atomic minimum, so entries only ever decrease.
template <int kScope> __device__ __forceinline__ int gseg_find(int32_t *parent, int x)
{
    int p = gseg_load<kScope>(parent + x);
    while (p != x) {
        const int g = gseg_load<kScope>(parent + p);
        if (g != p) (void)__hip_atomic_fetch_min(parent + x, g, __ATOMIC_RELAXED, kScope);
        x = p;
        p = g;
    }
    return x;
}

// Join the sets of a and b -> the root of the joined set as this thread last saw it.  A failed CAS means that another
// thread has linked root h under a smaller voxel in between (see the progress argument at the top); the loop goes on from
// what that thread wrote.
template <int kScope> __device__ __forceinline__ int gseg_union(int32_t *parent, int a, int b)
{
    for (;;) {
        a = gseg_find<kScope>(parent, a);
        b = gseg_find<kScope>(parent, b);
        if (a == b) return a;
        const int h = a > b ? a : b, l = a > b ? b : a;
        int old = h;
        if (__hip_atomic_compare_exchange_strong(parent + h, &old, l, __ATOMIC_RELAXED, __ATOMIC_RELAXED, kScope)) return l;
        a = old;                                         // old < h: the root h was given away by the other thread
        b = l;
    }
}

// S1: the label of voxel v, -1 for an unlabelled one.
__device__ __forceinline__ int gseg_label(const int32_t *voxel_labels, int L, int ne, int num_class, int v)
{
    if (v >= ne) return -1;
    if (!voxel_labels) return 0;
    if (v >= L) return -1;
    const int c = voxel_labels[v];
    return (c >= 0 && c < num_class) ? c : -1;
}

// The join rule of the two union-find kernels is a functor: join(v, u) says whether the neighbours v and u, which carry the
// same label, are joined; enter(v) comes before the taps of a labelled voxel v in either kernel, mark() behind it in the
// local kernel alone (so once a labelled voxel), and done() ends the kernel for every thread.  "Labels equal" is the rule
// of conv3p_grid_segments: it joins every such pair and the four calls compile to nothing.
// conv3p_grid_segments_smooth's rule is in conv3p_grid_smooth.hpp.  Which pairs join does not touch the progress
// argument below: the functor is evaluated before the union and waits for nothing.
struct LabelsJoin {
    __device__ __forceinline__ bool join(int, int) { return true; }
    __device__ __forceinline__ void enter(int) {}
    __device__ __forceinline__ void mark() {}
    __device__ __forceinline__ void done() {}
};

template <typename Join>
__device__ __forceinline__ void gseg_local_body(Join rule, const int32_t *neigh, const int32_t *voxel_labels, int L,
                                                const int32_t *grid_stats, int M, int num_class, unsigned tapmask, int32_t *lab,
                                                int32_t *parent, int32_t *seg_root, int32_t *seg_size, int32_t *seg_rows,
                                                int32_t *seg_label, int32_t *seg_stats)
{
    __shared__ int32_t parent_s[kGsegLocalTile], lab_s[kGsegLocalTile];
    const int ne = clamped_count(grid_stats, M), i = threadIdx.x;
    if (blockIdx.x == 0 && i < 8) seg_stats[i] = i == 3 ? M - ne : 0;
    for (long long base = (long long)blockIdx.x * kGsegLocalTile; base < M; base += (long long)gridDim.x * kGsegLocalTile) {
        const long long w = base + i;
        const int v = (int)w;
        const int c = w < M ? gseg_label(voxel_labels, L, ne, num_class, v) : -1;
        lab_s[i] = c;
        parent_s[i] = i;
        __syncthreads();
        if (c >= 0) {                                    // v < ne
            rule.enter(v);
            rule.mark();
            const int32_t *row = neigh + (size_t)v * kInterpNeigh;
            int r = i;
            for (int t = 0; t < kGsegHalfTaps; ++t) {
                if (!((tapmask >> t) & 1u)) continue;
                const int u = row[t];
                if (u < base || u >= v) continue;        // the tile's own taps: base <= u < v (< ne); the rest is the link's
                if (lab_s[u - (int)base] != c) continue;
                if (!rule.join(v, u)) continue;
                r = gseg_union<__HIP_MEMORY_SCOPE_WORKGROUP>(parent_s, r, u - (int)base);
            }
        }
        __syncthreads();                                 // the tile's forest is final: plain walks
        if (w < M) {
            int x = i;
            while (parent_s[x] != x) x = parent_s[x];
            lab[v] = c;
            parent[v] = c >= 0 ? (int)base + x : -1;
            seg_root[v] = -1;
            seg_size[v] = 0;
            seg_rows[v] = 0;
            seg_label[v] = -1;
        }
        __syncthreads();                                 // before the next tile takes the arrays
    }
    rule.done();
}

__global__ __launch_bounds__(kGsegLocalTile) void gseg_local_kernel(const int32_t *neigh, const int32_t *voxel_labels, int L,
                                                                    const int32_t *grid_stats, int M, int num_class,
                                                                    unsigned tapmask, int32_t *lab, int32_t *parent,
                                                                    int32_t *seg_root, int32_t *seg_size, int32_t *seg_rows,
                                                                    int32_t *seg_label, int32_t *seg_stats)
{
    gseg_local_body(LabelsJoin(), neigh, voxel_labels, L, grid_stats, M, num_class, tapmask, lab, parent, seg_root, seg_size,
                    seg_rows, seg_label, seg_stats);
}

template <typename Join>
__device__ __forceinline__ void gseg_link_body(Join rule, const int32_t *neigh, const int32_t *lab, int32_t *parent,
                                               const int32_t *grid_stats, int M, unsigned tapmask)
{
    const int ne = clamped_count(grid_stats, M);
    for (long long w = (long long)blockIdx.x * kGsegThreads + threadIdx.x; w < ne; w += (long long)gridDim.x * kGsegThreads) {
        const int v = (int)w;
        const int lv = lab[v];
        if (lv < 0) continue;
        rule.enter(v);
        const int32_t *row = neigh + (size_t)v * kInterpNeigh;
        const int base = v / kGsegLocalTile * kGsegLocalTile;
        int r = v;                                       // v's set, followed from link to link: most taps find it joined
        for (int t = 0; t < kGsegHalfTaps; ++t) {
            if (!((tapmask >> t) & 1u)) continue;
            const int u = row[t];
            if (u < 0 || u >= ne || u == v) continue;   // S2
            if (u >= base && u < v) continue;            // joined in the tile already
            if (lab[u] != lv) continue;
            if (!rule.join(v, u)) continue;
            r = gseg_union<__HIP_MEMORY_SCOPE_AGENT>(parent, r, u);
        }
    }
    rule.done();
}

__global__ __launch_bounds__(kGsegThreads) void gseg_link_kernel(const int32_t *neigh, const int32_t *lab, int32_t *parent,
                                                                 const int32_t *grid_stats, int M, unsigned tapmask)
{
    gseg_link_body(LabelsJoin(), neigh, lab, parent, grid_stats, M, tapmask);
}

__global__ __launch_bounds__(kGsegThreads) void gseg_flatten_kernel(const int32_t *lab, int32_t *parent, int M, int ntiles,
                                                                  int32_t *tile_count)
{
    __shared__ int count_s;
    const int tid = threadIdx.x;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        if (tid == 0) count_s = 0;
        __syncthreads();
        int roots = 0;
        for (int j = 0; j < kGsegTileSteps; ++j) {
            const long long w = (long long)tile * kGsegTile + j * kGsegThreads + tid;
            if (w >= M) break;
            const int v = (int)w;
            if (lab[v] < 0) continue;
            int x = v, p = gseg_load<__HIP_MEMORY_SCOPE_AGENT>(parent + x);
            while (p != x) {                             // strictly decreasing: ends
                x = p;
                p = gseg_load<__HIP_MEMORY_SCOPE_AGENT>(parent + x);
            }
            if (x != v) __hip_atomic_store(parent + v, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            roots += x == v;
        }
        if (roots) atomicAdd(&count_s, roots);
        __syncthreads();
        if (tid == 0) tile_count[tile] = count_s;
        __syncthreads();
    }
}

// Exclusive prefixes of a[0 .. n) and, if given, b[0 .. n), in place; the totals go to total_a[0] and total_b[0].
__global__ __launch_bounds__(kGsegScanThreads) void gseg_scan_kernel(int32_t *a, int32_t *b, int n, int32_t *total_a,
                                                                   int32_t *total_b)
{
    __shared__ int scan_s[kGsegScanThreads / 64];
    for (int pass = 0; pass < 2; ++pass) {
        int32_t *x = pass ? b : a;
        if (!x) break;                                   // uniform
        const int total = wg_exscan_inplace(x, n, scan_s, (int)threadIdx.x, kGsegScanThreads);
        if (threadIdx.x == 0) (pass ? total_b : total_a)[0] = total;
    }
}

__global__ __launch_bounds__(kGsegThreads) void gseg_number_kernel(const int32_t *lab, const int32_t *parent, int M, int ntiles,
                                                                 const int32_t *tile_off, int32_t *segment, int32_t *seg_root,
                                                                 int32_t *seg_label)
{
    __shared__ int scan_s[kGsegThreads / 64];
    const int tid = threadIdx.x;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        int base = tile_off[tile];
        for (int j = 0; j < kGsegTileSteps; ++j) {        // uniform: every thread takes every step
            const long long w = (long long)tile * kGsegTile + j * kGsegThreads + tid;
            const int v = (int)w;
            const int c = w < M ? lab[v] : -1;
            const int f = (c >= 0 && parent[v] == v) ? 1 : 0;
            int total;
            const int s = base + wg_exscan(f, scan_s, tid, kGsegThreads, &total);
            if (f) {                                     // s < S <= M
                segment[v] = s;
                seg_root[s] = v;
                seg_label[s] = c;
            }
            base += total;
        }
        __syncthreads();
    }
}

// A wave takes `steps` times 64 CONSECUTIVE voxels at a time.  Within a step, runs of equal segment are summed by a
// segmented shuffle; the run that reaches the step's end is carried in registers into the next step and added to memory
// only when it ends, so a floor that is one segment costs one pair of adds per steps * 64 voxels, not one per voxel.
// Integer adds: the sums do not depend on steps or on the grid.
__global__ __launch_bounds__(kGsegThreads) void gseg_assign_kernel(const int32_t *lab, const int32_t *parent,
                                                                   const int32_t *voxel_count, const int32_t *grid_stats, int M,
                                                                   int steps, int32_t *segment, int32_t *seg_size,
                                                                   int32_t *seg_rows, int32_t *seg_stats)
{
    __shared__ int count_s[2];
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < 2) count_s[tid] = 0;
    __syncthreads();
    const int ne = clamped_count(grid_stats, M);
    int labelled = 0, bare = 0;
    const long long chunk = 64ll * steps, waves = (long long)gridDim.x * (kGsegThreads / 64);
    for (long long c0 = ((long long)blockIdx.x * (kGsegThreads / 64) + (tid >> 6)) * chunk; c0 < M; c0 += waves * chunk) {
        int cs = -1, cn = 0, cr = 0;                     // the carried run: the same in every lane
        for (int j = 0; j < steps; ++j) {
            const long long w = c0 + 64ll * j + lane;    // c0 and j are the wave's: all its lanes take every step
            if (w - lane >= M) break;
            const int v = (int)w;
            int s = -1, n = 0, rows = 0;
            if (w < M) {
                if (lab[v] >= 0) {
                    const int r = parent[v];
                    s = segment[r];                      // a root's word: written by gseg_number_kernel, not written here
                    if (r != v) segment[v] = s;
                    n = 1;
                    rows = voxel_count[v];
                    ++labelled;
                } else {
                    segment[v] = -1;
                    bare += v < ne;
                }
            }
            // runs of equal s among the step's 64 voxels: the run's first lane gets the run's sums
            const int before = __shfl_up(s, 1, 64);
            const bool head = lane == 0 || before != s;
            const unsigned long long heads = __ballot(head);
            const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
            const int end = above ? lane + __ffsll((long long)above) : 64;
            for (int d = 1; d < 64; d <<= 1) {
                const int yn = __shfl_down(n, d, 64), yr = __shfl_down(rows, d, 64);
                if (lane + d < end) {
                    n += yn;
                    rows += yr;
                }
            }
            const int last = 63 - __clzll((long long)heads);         // the head of the step's last run; lane 0 is a head
            const int s0 = __shfl(s, 0, 64), n0 = __shfl(n, 0, 64), r0 = __shfl(rows, 0, 64);
            if (s0 == cs) {                              // the carried run goes on
                cn += n0;
                cr += r0;
            } else {
                if (lane == 0 && cs >= 0) {
                    atomicAdd(&seg_size[cs], cn);
                    atomicAdd(&seg_rows[cs], cr);
                }
                cs = s0; cn = n0; cr = r0;
            }
            if (last != 0) {                             // it ends inside this step: flush it and the runs in between
                if (lane == 0 && cs >= 0) {
                    atomicAdd(&seg_size[cs], cn);
                    atomicAdd(&seg_rows[cs], cr);
                }
                if (head && lane != 0 && lane != last && s >= 0) {
                    atomicAdd(&seg_size[s], n);
                    atomicAdd(&seg_rows[s], rows);
                }
                cs = __shfl(s, last, 64); cn = __shfl(n, last, 64); cr = __shfl(rows, last, 64);
            }
        }
        if (lane == 0 && cs >= 0) {
            atomicAdd(&seg_size[cs], cn);
            atomicAdd(&seg_rows[cs], cr);
        }
    }
    if (labelled) atomicAdd(&count_s[0], labelled);
    if (bare) atomicAdd(&count_s[1], bare);
    __syncthreads();
    if (tid < 2 && count_s[tid]) atomicAdd(&seg_stats[1 + tid], count_s[tid]);
}

__global__ __launch_bounds__(kGsegThreads) void gseg_max_kernel(const int32_t *seg_size, const int32_t *seg_rows, int M,
                                                              int32_t *seg_stats)
{
    __shared__ int max_s[2];
    const int tid = threadIdx.x;
    if (tid < 2) max_s[tid] = 0;
    __syncthreads();
    int S = seg_stats[0];
    S = S < 0 ? 0 : (S > M ? M : S);
    int a = 0, b = 0;
    for (long long w = (long long)blockIdx.x * kGsegThreads + tid; w < S; w += (long long)gridDim.x * kGsegThreads) {
        const int n = seg_size[w], r = seg_rows[w];
        a = n > a ? n : a;
        b = r > b ? r : b;
    }
    for (int d = 32; d > 0; d >>= 1) {
        const int ya = __shfl_xor(a, d, 64), yb = __shfl_xor(b, d, 64);
        a = ya > a ? ya : a;
        b = yb > b ? yb : b;
    }
    if ((tid & 63) == 0) {
        if (a) atomicMax(&max_s[0], a);
        if (b) atomicMax(&max_s[1], b);
    }
    __syncthreads();
    if (tid < 2 && max_s[tid]) atomicMax(&seg_stats[4 + tid], max_s[tid]);
}

// ------------------------------------------------------------------------------------------------------------ absorb
struct AbsorbArgs {
    const int32_t *neigh, *voxel_labels, *segment, *seg_size, *seg_label, *seg_stats, *grid_stats;
    int L, M, num_class, min_size, drop_orphans, ntiles;
    unsigned tapmask;
    int32_t *labels_out, *seg_label_out;
    unsigned long long *stats;
    int32_t *hdr;                                        // hdr[0]: small segments, hdr[1]: their voxels
    int32_t *tile_small, *tile_members;                  // per tile of segments
    int32_t *cursor, *small_list, *small_off, *members;  // M words each
};

// seg_size[s] of a small segment, 0 otherwise (A1); sizes are held to [0, M] so that no sum leaves int32
__device__ __forceinline__ int absorb_small_size(const AbsorbArgs &p, long long s, int S)
{
    if (s >= S) return 0;
    const int n = p.seg_size[s];
    return (n >= 1 && n < p.min_size && n <= p.M) ? n : 0;
}

__global__ __launch_bounds__(kGsegThreads) void absorb_count_kernel(const AbsorbArgs p)
{
    __shared__ int count_s[2];
    const int tid = threadIdx.x;
    const int S = clamped_count(p.seg_stats, p.M);
    if (blockIdx.x == 0 && tid < 4) p.stats[tid] = 0ull;
    for (int tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
        if (tid < 2) count_s[tid] = 0;
        __syncthreads();
        int k = 0, m = 0;
        for (int j = 0; j < kGsegTileSteps; ++j) {
            const int n = absorb_small_size(p, (long long)tile * kGsegTile + j * kGsegThreads + tid, S);
            k += n > 0;
            m += n;
        }
        if (k) {
            atomicAdd(&count_s[0], k);
            atomicAdd(&count_s[1], m);
        }
        __syncthreads();
        if (tid == 0) {
            p.tile_small[tile] = count_s[0];
            p.tile_members[tile] = count_s[1];
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kGsegThreads) void absorb_plan_kernel(const AbsorbArgs p)
{
    __shared__ int scan_s[kGsegThreads / 64];
    const int tid = threadIdx.x;
    const int S = clamped_count(p.seg_stats, p.M);
    for (int tile = blockIdx.x; tile < p.ntiles; tile += gridDim.x) {
        int kbase = p.tile_small[tile], mbase = p.tile_members[tile];
        for (int j = 0; j < kGsegTileSteps; ++j) {        // uniform
            const long long s = (long long)tile * kGsegTile + j * kGsegThreads + tid;
            const int n = absorb_small_size(p, s, S);
            int ktot, mtot;
            const int k = kbase + wg_exscan(n > 0 ? 1 : 0, scan_s, tid, kGsegThreads, &ktot);
            const int off = mbase + wg_exscan(n, scan_s, tid, kGsegThreads, &mtot);
            if (n > 0) {                                 // k < M, off + n <= M: at most M voxels lie in segments
                p.small_list[k] = (int)s;
                p.small_off[k] = off;
                p.cursor[s] = off;
            }
            if (s < p.M) p.seg_label_out[s] = s < S ? p.seg_label[s] : -1;
            kbase += ktot;
            mbase += mtot;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kGsegThreads) void absorb_scatter_kernel(const AbsorbArgs p)
{
    const int S = clamped_count(p.seg_stats, p.M);
    for (long long w = (long long)blockIdx.x * kGsegThreads + threadIdx.x; w < p.M; w += (long long)gridDim.x * kGsegThreads) {
        const int s = p.segment[w];
        if (s < 0 || s >= S) continue;
        const int n = absorb_small_size(p, s, S);
        if (n == 0) continue;
        const int at = atomicAdd(&p.cursor[s], 1);
        if (at >= 0 && at < p.M) p.members[at] = (int)w;  // holds for a consistent segmentation; a guard for any other
    }
}

__global__ __launch_bounds__(kGsegThreads) void absorb_vote_kernel(const AbsorbArgs p)
{
    __shared__ int hist_s[kGsegThreads / 64][kGsegMaxClass];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int S = clamped_count(p.seg_stats, p.M);
    const int ne = clamped_count(p.grid_stats, p.M);
    int small = p.hdr[0];
    small = small < 0 ? 0 : (small > p.M ? p.M : small);
    int *hist = hist_s[wv];
    const int t = lane & 31, half = lane >> 5;
    const bool tap = t < kInterpNeigh && ((p.tapmask >> t) & 1u);
    unsigned long long n_abs = 0, n_orph = 0, n_changed = 0;     // lane 0's
    for (long long k = (long long)blockIdx.x * (kGsegThreads / 64) + wv; k < small; k += (long long)gridDim.x * (kGsegThreads / 64)) {
        const int s = p.small_list[k], off = p.small_off[k];
        int n = p.seg_size[s];
        n = (n < 0 || off < 0 || off > p.M) ? 0 : (n > p.M - off ? p.M - off : n);
        hist[lane] = 0;                                  // a wave's own rows: its lanes run in step, no barrier
        hist[lane + 64] = 0;
        __builtin_amdgcn_wave_barrier();
        for (int i = half; i < n; i += 2) {              // A2: every (member, tap) pair once
            if (!tap) continue;
            const int u = p.members[off + i];
            if (u < 0 || u >= ne) continue;
            const int w = p.neigh[(size_t)u * kInterpNeigh + t];
            if (w < 0 || w >= ne) continue;
            const int sw = p.segment[w];
            if (sw < 0 || sw >= S || sw == s) continue;
            const int nw = p.seg_size[sw];
            if (nw < p.min_size) continue;               // small neighbours do not vote
            const int c = p.seg_label[sw];
            if (c >= 0 && c < p.num_class) atomicAdd(&hist[c], 1);
        }
        __builtin_amdgcn_wave_barrier();
        // A3: most votes, the lowest class of a tie.  key = votes * 256 + (255 - class), the largest key wins.
        const int v0 = hist[lane], v1 = hist[lane + 64];
        long long key = v0 > 0 ? (((long long)v0 << 8) | (255 - lane)) : -1;
        const long long key1 = v1 > 0 ? (((long long)v1 << 8) | (255 - (lane + 64))) : -1;
        key = key1 > key ? key1 : key;
        for (int d = 32; d > 0; d >>= 1) {
            const long long y = __shfl_xor(key, d, 64);
            key = y > key ? y : key;
        }
        __builtin_amdgcn_wave_barrier();                 // the reads above before the next segment's zeroing
        if (lane == 0) {
            const int old = p.seg_label[s];
            int now = old;
            if (key >= 0) {
                now = 255 - (int)(key & 255);
                ++n_abs;
            } else {
                if (p.drop_orphans) now = -1;
                ++n_orph;
            }
            p.seg_label_out[s] = now;
            if (now != old) n_changed += (unsigned long long)n;
        }
    }
    if (lane == 0) {
        if (n_abs) atomicAdd(&p.stats[1], n_abs);
        if (n_orph) atomicAdd(&p.stats[2], n_orph);
        if (n_changed) atomicAdd(&p.stats[3], n_changed);
        if (blockIdx.x == 0 && wv == 0) p.stats[0] = (unsigned long long)small;
    }
}

__global__ __launch_bounds__(kGsegThreads) void absorb_labels_kernel(const AbsorbArgs p)
{
    const int S = clamped_count(p.seg_stats, p.M);
    const int ne = clamped_count(p.grid_stats, p.M);
    const int keep = p.voxel_labels ? (p.L < ne ? p.L : ne) : 0;
    for (long long w = (long long)blockIdx.x * kGsegThreads + threadIdx.x; w < p.M; w += (long long)gridDim.x * kGsegThreads) {
        const int s = p.segment[w];
        int c = -1;                                      // A4
        if (s >= 0 && s < S) c = p.seg_label_out[s];
        else if (w < keep) c = p.voxel_labels[w];
        p.labels_out[w] = c;
    }
}

}  // namespace conv3p
