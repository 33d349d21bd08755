// conv3p_grid_knn.hpp -- the exact k-nearest-voxel search on the grid and its two consumers (conv3p_grid_knn_f32,
// conv3p_grid_interpolate_knn_f32 / _i64, conv3p_grid_normals_knn_f32).
//
// include/conv3p_knn.h defines the results by the rules K1-K8 (and rule 5 / R1-R6 of conv3p.h for the consumers) and
// tests/grid_knn_ref.py restates them in numpy.  The search is four kernels, one launch each, the last only with rings > 1:
//
//   grid_knn_spread_kernel  K5's extremes.  A thread goes over voxels, then over queries, in a grid-stride loop and keeps
//                           the minima and maxima of f_a = x_a - c_a h of the room it is in in registers; a change of
//                           room flushes them.  What is left at the end of a loop is folded over the wave where the
//                           wave's lanes are all in one room (butterfly fmin / fmax on doubles: exact, so the order does
//                           not matter) and flushed by one lane, else by every lane.  A flush is six 64-bit atomicMax on
//                           order-preserving keys of the doubles -- a minimum is kept as the maximum of the complemented
//                           key, so one memset of zeros initialises all twelve words of a room, and a word still 0 says
//                           that nothing was seen.
//   grid_knn_bound_kernel   a thread per room: S[g] from the twelve words, NaN where a word is 0 (no STOP holds there).
//   grid_knn_near_kernel    the plain interpolation's shape: 16 lanes a query, a lane takes entries t and t + 16 of the
//                           27 of neigh[v0], k butterfly minima over the group's 64-bit (d2 bits, voxel) keys; lane j
//                           keeps the j-th, so the rows of the table are written side by side.  The Chebyshev distance
//                           of an entry is 0 for t = 13 and 1 otherwise.  STOP(1) is evaluated once.  With rings == 1 or
//                           STOP(1) the query is finished and written; the others go to a list (a ballot per wave, one
//                           add per wave on the counter, as grid_ring_list_kernel does).
//   grid_knn_ring_kernel    a fixed grid, a wave per listed query, the number of queries read from the scratch and held
//                           to [0, Q].  For r = 1 .. rings the lanes go over the (dx, dy) columns of the shell of ring r
//                           (the whole cube at r = 1) with grid_cell_lower_bound and the run walk of the ring search;
//                           a lane keeps its 16 smallest keys sorted in registers by an unrolled insertion.  After a
//                           ring the wave pops k minima; lane j keeps the j-th and is the only one to put it back, so
//                           the lanes' lists hold the cube's k smallest once each and everything else is dropped.
//                           STOP(r) is wave-uniform, so the branch that ends the search is the wave's.  The ring of the
//                           kept is the maximum over the lanes of the Chebyshev distance of each one's cell.
//
// The consumers: grid_knn_interpolate_kernel is grid_interpolate_kernel with the selection replaced by a read of the
// table (16 lanes a row, entry j loaded by lane j and handed round by shuffles); grid_knn_normals_kernel is
// grid_normals_kernel with at most 16 samples in rank order and the same normals_solve.
//
// The counts are in registers per wave, LDS per workgroup, one 64-bit add per workgroup and count.  Every loop is bounded
// whatever the memory holds: the search halves its range, a walk takes at most 2r + 1 entries, the columns are at most
// 289, the list at most the clamped count, every voxel number used lies in [0, ne), ne <= M.  No candidate list is
// indexed at run time: no private segment.  All shuffles run with the whole wave active.
#pragma once

#include "conv3p_grid_interp_rings.hpp"
#include "conv3p_grid_normals.hpp"

namespace conv3p {

constexpr int kKnnMaxK = 16;
constexpr int kKnnSpreadThreads = 256;
constexpr int kKnnSpreadMaxGrid = 512;
constexpr int kKnnRoomWords = 12;               // Pmax[3], ~Pmin[3], Fmax[3], ~Fmin[3]
constexpr int kKnnStats = 16;
constexpr size_t kKnnHeaderBytes = 256;         // the list's counter

// a finite double as 64 bits that order as it does; never 0 and never ~0 for a finite value
__device__ __forceinline__ unsigned long long knn_key(double x)
{
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double knn_unkey(unsigned long long k)
{
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

struct KnnSpan { double lo[3], hi[3]; int room; };

__device__ __forceinline__ void knn_span_reset(KnnSpan &s, int room)
{
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        s.lo[a] = INFINITY;
        s.hi[a] = -INFINITY;
    }
    s.room = room;
}
// the span's extremes to words [0, 6) of its room's record at `words` (hi as its key, lo as the complement of its key)
__device__ __forceinline__ void knn_span_flush(const KnnSpan &s, unsigned long long *words, int rooms)
{
    if (s.room < 0 || s.room >= rooms || !(s.lo[0] <= s.hi[0])) return;
    unsigned long long *w = words + (size_t)s.room * kKnnRoomWords;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        atomicMax(&w[a], knn_key(s.hi[a]));
        atomicMax(&w[3 + a], ~knn_key(s.lo[a]));
    }
}
__device__ __forceinline__ void knn_span_add(KnnSpan &s, int room, float x, float y, float z, const int32_t *cell, double h,
                                             unsigned long long *words, int rooms)
{
    if (room != s.room) {
        knn_span_flush(s, words, rooms);
        knn_span_reset(s, room);
    }
    const double f[3] = {(double)x - (double)cell[0] * h, (double)y - (double)cell[1] * h, (double)z - (double)cell[2] * h};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        s.lo[a] = fmin(s.lo[a], f[a]);
        s.hi[a] = fmax(s.hi[a], f[a]);
    }
}
// what the lanes of a wave still hold: one flush where they are all in one room, else one a lane.  Every lane calls it.
__device__ __forceinline__ void knn_span_finish(KnnSpan &s, unsigned long long *words, int rooms, int lane)
{
    const bool has = s.room >= 0 && s.lo[0] <= s.hi[0];
    int g = has ? s.room : -1;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int o = __shfl_xor(g, d, 64);
        g = o > g ? o : g;
    }
    if (__ballot(has && s.room != g) == 0ull) {          // the wave's
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                s.lo[a] = fmin(s.lo[a], __shfl_xor(s.lo[a], d, 64));
                s.hi[a] = fmax(s.hi[a], __shfl_xor(s.hi[a], d, 64));
            }
        }
        s.room = g;
        if (lane == 0) knn_span_flush(s, words, rooms);
    } else {
        knn_span_flush(s, words, rooms);
    }
}

__global__ __launch_bounds__(kKnnSpreadThreads) void grid_knn_spread_kernel(const float *query, long long Q, int qs,
                                                                           const int32_t *query_voxel, const float *voxel_data,
                                                                           int Kv, const int32_t *voxel_cell,
                                                                           const int32_t *voxel_room, int num_rooms,
                                                                           const int32_t *grid_stats, int M, float voxel,
                                                                           unsigned long long *words)
{
    const int tid = threadIdx.x, lane = tid & 63;
    const int ne = M > 0 ? clamped_count(grid_stats, M) : 0;
    const int rooms = voxel_room ? num_rooms : 1;
    const double h = (double)voxel;
    const long long first = (long long)blockIdx.x * kKnnSpreadThreads + tid, step = (long long)gridDim.x * kKnnSpreadThreads;
    KnnSpan s;
    knn_span_reset(s, -1);
    for (long long u = first; u < ne; u += step) {       // F: the representatives
        const float *p = voxel_data + (size_t)u * Kv;
        const float x = p[0], y = p[1], z = p[2];
        if (!scene_finite(x, y, z)) continue;
        const int g = voxel_room ? voxel_room[u] : 0;
        if (g < 0 || g >= rooms) continue;
        knn_span_add(s, g, x, y, z, voxel_cell + 3 * (size_t)u, h, words + 6, rooms);
    }
    knn_span_finish(s, words + 6, rooms, lane);
    knn_span_reset(s, -1);
    for (long long i = first; i < Q; i += step) {        // P: the live queries
        const int v0 = query_voxel ? query_voxel[i] : (int)i;
        if (v0 < 0 || v0 >= ne) continue;
        const float *p = query + (size_t)i * qs;
        const float x = p[0], y = p[1], z = p[2];
        if (!scene_finite(x, y, z)) continue;
        const int g = voxel_room ? voxel_room[v0] : 0;
        if (g < 0 || g >= rooms) continue;
        knn_span_add(s, g, x, y, z, voxel_cell + 3 * (size_t)v0, h, words, rooms);
    }
    knn_span_finish(s, words, rooms, lane);
}

__global__ __launch_bounds__(kKnnSpreadThreads) void grid_knn_bound_kernel(const unsigned long long *words, int rooms, double *S)
{
    for (int g = blockIdx.x * kKnnSpreadThreads + threadIdx.x; g < rooms; g += gridDim.x * kKnnSpreadThreads) {
        const unsigned long long *w = words + (size_t)g * kKnnRoomWords;
        double s = -INFINITY;
        bool all = true;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const unsigned long long pmax = w[a], pmin = w[3 + a], fmax_ = w[6 + a], fmin_ = w[9 + a];
            all = all && pmax != 0ull && pmin != 0ull && fmax_ != 0ull && fmin_ != 0ull;
            s = fmax(s, fmax(knn_unkey(pmax) - knn_unkey(~fmin_), knn_unkey(fmax_) - knn_unkey(~pmin)));
        }
        S[g] = all ? s : __longlong_as_double(0x7ff8000000000000ll);
    }
}

// K6 for a query whose room has spread S (NaN: none), n candidates within ring r, d2k the k-th smallest of them
__device__ __forceinline__ bool knn_stop(double S, double h, int r, int n, int k, float d2k)
{
    const double L = (double)(r + 1) * h - S;
    const double least = fmax(0.25 * h, 8.8817841970012523e-16);    // 2^-50
    return n >= k && L >= least && (double)d2k < (L * L) * (1.0 - 9.5367431640625e-07);   // 1 - 2^-20
}

// the range of K2 and the spread of the room of the live query of voxel v0
__device__ __forceinline__ void knn_room(int v0, int ne, const int32_t *voxel_room, const int32_t *voxel_start, int num_rooms,
                                         const double *S, int &lo, int &hi, double &spread)
{
    lo = 0;
    hi = ne;
    int g = 0;
    if (voxel_room) {
        g = voxel_room[v0];
        if (g >= 0 && g < num_rooms) {
            lo = voxel_start[g];
            hi = voxel_start[g + 1];
            lo = lo < 0 ? 0 : lo;
            hi = hi > ne ? ne : hi;
        } else {
            hi = 0;
            g = -1;
        }
    }
    spread = g >= 0 ? S[g] : __longlong_as_double(0x7ff8000000000000ll);
}

struct KnnOut {
    int32_t *index; float *d2; int32_t *count, *ring, *scanned, *certified;
};

constexpr int kKnnNearCounts = 8;               // full, partial, none, not live, certified, finished live, ring 0, ring 1

__global__ __launch_bounds__(kInterpThreads) void grid_knn_near_kernel(const float *query, long long Q, int qs,
                                                                      const int32_t *query_voxel, const float *voxel_data, int Kv,
                                                                      const int32_t *neigh, const int32_t *voxel_room,
                                                                      const int32_t *voxel_start, int num_rooms,
                                                                      const int32_t *grid_stats, int M, const int32_t *valid,
                                                                      float voxel, int k, int rings, int exclude_self,
                                                                      const double *S, int32_t *counter, int32_t *list, KnnOut out,
                                                                      unsigned long long *stats)
{
    __shared__ int count_s[kKnnNearCounts];
    const int tid = threadIdx.x, lane = tid & 63, gl = tid & (kInterpGroup - 1), grp = tid / kInterpGroup;
    const unsigned long long none = ~0ull;
    if (tid < kKnnNearCounts) count_s[tid] = 0;
    const int ne = M > 0 ? clamped_count(grid_stats, M) : 0;
    const double h = (double)voxel;
    int c_full = 0, c_part = 0, c_none = 0, c_dead = 0, c_cert = 0, c_live = 0, c_ring0 = 0, c_ring1 = 0;   // of this wave
    for (long long base = (long long)blockIdx.x * kInterpRows; base < Q; base += (long long)gridDim.x * kInterpRows) {
        const long long i = base + grp;
        const bool in = i < Q;
        int v0 = in ? (query_voxel ? query_voxel[i] : (int)i) : -1;
        if (v0 >= ne) v0 = -1;
        float px = 0.0f, py = 0.0f, pz = 0.0f;
        if (v0 >= 0) {
            const float *p = query + (size_t)i * qs;
            px = p[0]; py = p[1]; pz = p[2];
            if (!scene_finite(px, py, pz)) v0 = -1;      // K1
        }
        int lo = 0, hi = 0;
        double spread = 0.0;
        if (v0 >= 0) knn_room(v0, ne, voxel_room, voxel_start, num_rooms, S, lo, hi, spread);
        unsigned long long key[2];
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int t = gl + half * kInterpGroup;
            key[half] = none;
            if (v0 < 0 || t >= kInterpNeigh) continue;
            const int u = neigh[(size_t)v0 * kInterpNeigh + t];
            if (u < lo || u >= hi) continue;             // K3: inside the range, so inside [0, ne)
            if (exclude_self && u == v0) continue;
            if (valid && valid[u] < 0) continue;
            const float *q = voxel_data + (size_t)u * Kv;
            const float dx = px - q[0], dy = py - q[1], dz = pz - q[2];
            const float d2 = ((dx * dx) + (dy * dy)) + (dz * dz);
            if (!(d2 < INFINITY)) continue;              // NaN or inf
            key[half] = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)u;
        }
        unsigned long long mine = none, last = none;     // lane j's is the j-th kept; the k-th kept, in every lane
        bool far = false;                                // this lane held a kept key of a cell that is not the query's
        int cnt = 0;
#pragma unroll
        for (int j = 0; j < kKnnMaxK; ++j) {
            if (j < k) {                                 // k is the launch's: every lane of the wave is here
                unsigned long long m = key[0] < key[1] ? key[0] : key[1];
#pragma unroll
                for (int d = kInterpGroup / 2; d >= 1; d >>= 1) {
                    const unsigned long long o = __shfl_xor(m, d, 64);
                    m = o < m ? o : m;
                }
                if (m != none) {
                    if (key[0] == m) { key[0] = none; far = far || gl != 13; }      // t = gl: 13 is the query's own cell
                    if (key[1] == m) { key[1] = none; far = true; }                 // t = gl + 16
                    if (gl == j) mine = m;
                    last = m;
                    cnt = j + 1;
                }
            }
        }
        const unsigned long long fars = __ballot(far);
        const int ring = ((fars >> (lane & ~(kInterpGroup - 1))) & 0xffffull) ? 1 : 0;
        const bool live = v0 >= 0;
        const bool stop = live && knn_stop(spread, h, 1, cnt, k, __uint_as_float((unsigned)(last >> 32)));
        const bool finished = in && (!live || rings == 1 || stop);
        const bool lead = gl == 0;
        const bool want = in && !finished && lead;       // to the list
        const unsigned long long mask = __ballot(want);
        const int n = __popcll(mask);
        int at = 0;
        if (n) {                                         // the wave's
            if (lane == 0) at = atomicAdd(counter, n);
            at = __shfl(at, 0, 64);
        }
        if (want) {
            const long long slot = (long long)at + __popcll(mask & ((1ull << lane) - 1ull));
            if (slot >= 0 && slot < Q) list[slot] = (int32_t)i;
        }
        if (finished) {
            if (gl < k) {
                out.index[(size_t)i * k + gl] = mine != none ? (int32_t)(unsigned)(mine & 0xffffffffull) : -1;
                out.d2[(size_t)i * k + gl] = mine != none ? __uint_as_float((unsigned)(mine >> 32)) : INFINITY;
            }
            if (lead) {
                out.count[i] = cnt;
                out.ring[i] = ring;
                out.scanned[i] = live ? 1 : 0;
                out.certified[i] = stop ? 1 : 0;
            }
        }
        const bool fl = finished && lead && live;
        c_full += __popcll(__ballot(fl && cnt == k));
        c_part += __popcll(__ballot(fl && cnt > 0 && cnt < k));
        c_none += __popcll(__ballot(fl && cnt == 0));
        c_dead += __popcll(__ballot(finished && lead && !live));
        c_cert += __popcll(__ballot(fl && stop));
        c_live += __popcll(__ballot(fl));
        c_ring0 += __popcll(__ballot(fl && cnt > 0 && ring == 0));
        c_ring1 += __popcll(__ballot(fl && cnt > 0 && ring == 1));
    }
    __syncthreads();
    if (lane == 0) {
        if (c_full) atomicAdd(&count_s[0], c_full);
        if (c_part) atomicAdd(&count_s[1], c_part);
        if (c_none) atomicAdd(&count_s[2], c_none);
        if (c_dead) atomicAdd(&count_s[3], c_dead);
        if (c_cert) atomicAdd(&count_s[4], c_cert);
        if (c_live) atomicAdd(&count_s[5], c_live);      // scanned is 1 for each of them
        if (c_ring0) atomicAdd(&count_s[6], c_ring0);
        if (c_ring1) atomicAdd(&count_s[7], c_ring1);
    }
    __syncthreads();
    if (tid < kKnnNearCounts && count_s[tid]) atomicAdd(&stats[tid], (unsigned long long)count_s[tid]);   // words 0 .. 7 as K8 has them
}

// one more key into a lane's sixteen smallest, ascending: what falls off the end is dropped
__device__ __forceinline__ void knn_insert(unsigned long long (&b)[kKnnMaxK], unsigned long long x)
{
#pragma unroll
    for (int j = 0; j < kKnnMaxK; ++j) {
        const unsigned long long lo = x < b[j] ? x : b[j], hi = x < b[j] ? b[j] : x;
        b[j] = lo;
        x = hi;
    }
}

constexpr int kKnnRingCounts = 14;              // full, partial, none, certified, sum of scanned, ring 0 .. 8

__global__ __launch_bounds__(kRingThreads) void grid_knn_ring_kernel(const float *query, long long Q, int qs,
                                                                    const int32_t *query_voxel, const float *voxel_data, int Kv,
                                                                    const int32_t *voxel_cell, const int32_t *voxel_room,
                                                                    const int32_t *voxel_start, int num_rooms,
                                                                    const int32_t *grid_stats, int M, const int32_t *valid,
                                                                    float voxel, int k, int rings, int exclude_self,
                                                                    const double *S, const int32_t *counter, const int32_t *list,
                                                                    KnnOut out, unsigned long long *stats)
{
    __shared__ int count_s[kKnnRingCounts];
    long long count = counter[0];
    count = count < 0 ? 0 : (count > Q ? Q : count);
    if ((long long)blockIdx.x * kRingWaves >= count) return;         // the workgroup's: nothing to do
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long none = ~0ull;
    if (tid < kKnnRingCounts) count_s[tid] = 0;
    const int ne = M > 0 ? clamped_count(grid_stats, M) : 0;
    const double h = (double)voxel;
    int tally[kKnnRingCounts];                           // of this wave, the same in all its lanes
#pragma unroll
    for (int q = 0; q < kKnnRingCounts; ++q) tally[q] = 0;
    for (long long at = (long long)blockIdx.x * kRingWaves + wave; at < count; at += (long long)gridDim.x * kRingWaves) {
        const long long i = list[at];
        int v0 = i >= 0 && i < Q ? (query_voxel ? query_voxel[i] : (int)i) : -1;
        if (v0 >= ne) v0 = -1;
        if (v0 < 0) continue;                            // the wave's; never so for a list this call wrote
        const float *p = query + (size_t)i * qs;
        const float px = p[0], py = p[1], pz = p[2];
        if (!scene_finite(px, py, pz)) continue;         // likewise
        int lo, hi;
        double spread;
        knn_room(v0, ne, voxel_room, voxel_start, num_rooms, S, lo, hi, spread);
        const int32_t *own = voxel_cell + 3 * (size_t)v0;
        const int ca = own[0], cb = own[1], cl = own[2];
        unsigned long long best[kKnnMaxK];
#pragma unroll
        for (int j = 0; j < kKnnMaxK; ++j) best[j] = none;
        unsigned long long mine = none, last = none;
        int cnt = 0, scanned = rings;
        bool stop = false;
        for (int r = 1; r <= rings && lo < hi; ++r) {    // rings is the launch's, [lo, hi) the wave's
            const int side = 2 * r + 1;
            for (int col = lane; col < side * side; col += 64) {
                const int dx = col / side - r, dy = col - (col / side) * side - r;
                const int x = ca + dx, y = cb + dy;
                if (x < 0 || y < 0) continue;            // outside the lattice: not found
                const bool outer = r == 1 || dx == r || dx == -r || dy == r || dy == -r;     // ring 1 takes the whole cube
                const int len = outer ? side : 1;
                for (int half = 0; half < (outer ? 1 : 2); ++half) {
                    const int z0 = half ? cl + r : cl - r;
                    int e = grid_cell_lower_bound(voxel_cell, lo, hi, x, y, z0);
                    for (int w = 0; w < len && e < hi; ++w, ++e) {
                        const int32_t *c = voxel_cell + 3 * (size_t)e;
                        if (c[0] != x || c[1] != y || c[2] < z0 || c[2] - z0 >= len) break;
                        if (exclude_self && e == v0) continue;
                        if (valid && valid[e] < 0) continue;
                        const float *q = voxel_data + (size_t)e * Kv;
                        const float ex = px - q[0], ey = py - q[1], ez = pz - q[2];
                        const float d2 = ((ex * ex) + (ey * ey)) + (ez * ez);
                        if (!(d2 < INFINITY)) continue;  // NaN or inf
                        knn_insert(best, ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)e);
                    }
                }
            }
            mine = none;                                 // the cube's k smallest: lane j keeps the j-th
            last = none;
            cnt = 0;
#pragma unroll
            for (int j = 0; j < kKnnMaxK; ++j) {
                if (j < k) {                             // k is the launch's: every lane of the wave is here
                    unsigned long long m = best[0];
#pragma unroll
                    for (int d = 32; d >= 1; d >>= 1) {
                        const unsigned long long o = __shfl_xor(m, d, 64);
                        m = o < m ? o : m;
                    }
                    if (m != none) {
                        if (best[0] == m) {              // a voxel is one candidate of the query: the keys are distinct
#pragma unroll
                            for (int t = 0; t + 1 < kKnnMaxK; ++t) best[t] = best[t + 1];
                            best[kKnnMaxK - 1] = none;
                        }
                        if (lane == j) mine = m;
                        last = m;
                        cnt = j + 1;
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < kKnnMaxK; ++j) best[j] = none;       // what was not popped cannot be kept any more
            best[0] = mine;
            stop = knn_stop(spread, h, r, cnt, k, __uint_as_float((unsigned)(last >> 32)));
            if (stop) {                                  // the wave's
                scanned = r;
                break;
            }
        }
        int ring = 0;                                    // K4: the largest Chebyshev distance among the kept
        if (mine != none) {
            const int32_t *c = voxel_cell + 3 * (size_t)(unsigned)(mine & 0xffffffffull);
            const int a0 = abs(c[0] - ca), a1 = abs(c[1] - cb), a2 = abs(c[2] - cl);
            ring = a0 > a1 ? (a0 > a2 ? a0 : a2) : (a1 > a2 ? a1 : a2);
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const int o = __shfl_xor(ring, d, 64);
            ring = o > ring ? o : ring;
        }
        if (lane < k) {
            out.index[(size_t)i * k + lane] = mine != none ? (int32_t)(unsigned)(mine & 0xffffffffull) : -1;
            out.d2[(size_t)i * k + lane] = mine != none ? __uint_as_float((unsigned)(mine >> 32)) : INFINITY;
        }
        if (lane == 0) {
            out.count[i] = cnt;
            out.ring[i] = ring;
            out.scanned[i] = scanned;
            out.certified[i] = stop ? 1 : 0;
        }
        tally[0] += cnt == k ? 1 : 0;
        tally[1] += cnt > 0 && cnt < k ? 1 : 0;
        tally[2] += cnt == 0 ? 1 : 0;
        tally[3] += stop ? 1 : 0;
        tally[4] += scanned;
#pragma unroll
        for (int q = 0; q <= kRingMax; ++q) tally[5 + q] += cnt > 0 && ring == q ? 1 : 0;
    }
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < kKnnRingCounts; ++q)
            if (tally[q]) atomicAdd(&count_s[q], tally[q]);
    }
    __syncthreads();
    // K8: words 0 .. 2 as they are, certified and the sum of scanned at 4 and 5, the rings from 6
    if (tid < kKnnRingCounts && count_s[tid]) atomicAdd(&stats[tid < 3 ? tid : tid + 1], (unsigned long long)count_s[tid]);
}

// ------------------------------------------------------------------------------------------------- the two consumers
template <typename S>
__global__ __launch_bounds__(kInterpThreads) void grid_knn_interpolate_kernel(const int32_t *knn_index, const float *knn_d2,
                                                                             const int32_t *knn_count, long long Q, int width,
                                                                             int k_use, const S *scores, int M, int C,
                                                                             int32_t *out_labels, float *out_scores,
                                                                             unsigned long long *stats)
{
    __shared__ int count_s[2];
    const int tid = threadIdx.x, gl = tid & (kInterpGroup - 1), grp = tid / kInterpGroup;
    const int head = (tid & 63) & ~(kInterpGroup - 1);   // the group's first lane in the wave
    if (tid < 2) count_s[tid] = 0;
    int done = 0, missed = 0;                            // of this wave, the same in all its lanes
    for (long long base = (long long)blockIdx.x * kInterpRows; base < Q; base += (long long)gridDim.x * kInterpRows) {
        const long long i = base + grp;
        const bool live = i < Q;
        int n = live ? knn_count[i] : 0;
        n = n < 0 ? 0 : (n > k_use ? k_use : n);         // k_use <= width <= 16
        int u = 0;
        float w = 0.0f;
        if (gl < n) {                                    // entry gl is lane gl's
            u = knn_index[(size_t)i * width + gl];
            w = 1.0f / fmaxf(knn_d2[(size_t)i * width + gl], 1e-10f);
        }
        const unsigned long long bad = __ballot(gl < n && (u < 0 || u >= M));
        if ((bad >> head) & 0xffffull) n = 0;            // an entry that is no voxel: the row has no neighbour
        int us[kKnnMaxK];
        float ws[kKnnMaxK];
#pragma unroll
        for (int j = 0; j < kKnnMaxK; ++j) {
            us[j] = __shfl(u, head + j, 64);
            ws[j] = __shfl(w, head + j, 64);
            if (j >= n) {
                us[j] = 0;
                ws[j] = 0.0f;
            }
        }
        float W = ws[0];
#pragma unroll
        for (int j = 1; j < kKnnMaxK; ++j)
            if (j < n) W = W + ws[j];
        float best = -INFINITY;
        int cls = 0x7fffffff;
        bool nan0 = false;
        for (int c0 = 0; c0 < C; c0 += kInterpGroup) {   // C is the launch's
            const int c = c0 + gl;
            if (c >= C) continue;
            float o = 0.0f;
            if (n > 0) {
                float acc = ws[0] * interp_score(scores, (size_t)us[0] * C + c);
#pragma unroll
                for (int j = 1; j < kKnnMaxK; ++j)
                    if (j < n) acc = acc + ws[j] * interp_score(scores, (size_t)us[j] * C + c);
                o = acc / W;
            }
            if (live && out_scores) out_scores[(size_t)i * C + c] = o;
            if (c == 0) nan0 = o != o;
            const float x = o != o ? -INFINITY : o;      // a NaN never wins
            if (cls == 0x7fffffff || x > best) {         // ascending classes: the lowest of a lane's maxima
                best = x;
                cls = c;
            }
        }
#pragma unroll
        for (int d = kInterpGroup / 2; d >= 1; d >>= 1) {
            const float ob = __shfl_xor(best, d, 64);
            const int oc = __shfl_xor(cls, d, 64);
            if (ob > best || (ob == best && oc < cls)) {
                best = ob;
                cls = oc;
            }
        }
        const int nan_first = __shfl(nan0 ? 1 : 0, head, 64);        // class 0 is lane 0's
        const bool lead = live && gl == 0;
        if (lead) out_labels[i] = n > 0 ? (nan_first ? 0 : cls) : -1;
        done += __popcll(__ballot(lead && n > 0));
        missed += __popcll(__ballot(lead && n == 0));
    }
    __syncthreads();
    if ((tid & 63) == 0) {
        if (done) atomicAdd(&count_s[0], done);
        if (missed) atomicAdd(&count_s[1], missed);
    }
    __syncthreads();
    if (tid < 2 && count_s[tid]) atomicAdd(&stats[tid], (unsigned long long)count_s[tid]);   // integers: exact in any order
}

__global__ __launch_bounds__(kNormalsThreads) void grid_knn_normals_kernel(const float *voxel_data, int K, const int32_t *knn_index,
                                                                          const int32_t *knn_count, int width,
                                                                          const int32_t *grid_stats, const int32_t *voxel_room,
                                                                          const float *viewpoint, int V, int M, int min_neighbors,
                                                                          float *normals, float *curvature, int32_t *samples,
                                                                          int32_t *flags, float *moments, int32_t *normal_stats)
{
    __shared__ int count_s[4];
    const int tid = threadIdx.x;
    if (tid < 4) count_s[tid] = 0;
    __syncthreads();
    const int ne = clamped_count(grid_stats, M);
    int c_ok = 0, c_few = 0, c_deg = 0, c_fill = 0;
    for (long long w = (long long)blockIdx.x * kNormalsThreads + tid; w < M; w += (long long)gridDim.x * kNormalsThreads) {
        const int v = (int)w;
        float mx = 0.0f, my = 0.0f, mz = 0.0f, cxx = 0.0f, cxy = 0.0f, cxz = 0.0f, cyy = 0.0f, cyz = 0.0f, czz = 0.0f;
        float px = 0.0f, py = 0.0f, pz = 0.0f;
        int n = 0, fl = -1;                              // R1
        if (v < ne) {
            const float *pv = voxel_data + (size_t)v * K;
            px = pv[0]; py = pv[1]; pz = pv[2];
            const bool own = normals_finite(px) && normals_finite(py) && normals_finite(pz);
            int have = knn_count[v];
            have = have < 0 ? 0 : (have > width ? width : have);     // width <= 16
            const int32_t *row = knn_index + (size_t)v * width;
            float qx[kKnnMaxK], qy[kKnnMaxK], qz[kKnnMaxK];
            unsigned mask = 0;
#pragma unroll
            for (int j = 0; j < kKnnMaxK; ++j) {         // R2': what is no sample reads the voxel's own row
                const int u = j < have ? row[j] : -1;
                const bool in = own && u >= 0 && u < ne;
                const float *pu = voxel_data + (size_t)(in ? u : v) * K;
                const float ax = pu[0], ay = pu[1], az = pu[2];
                const bool ok = in && normals_finite(ax) && normals_finite(ay) && normals_finite(az);
                qx[j] = ax - px; qy[j] = ay - py; qz[j] = az - pz;
                mask |= (ok ? 1u : 0u) << j;
            }
            n = __popc(mask);
            const float fn = (float)(n > 0 ? n : 1);     // n == 0: the sums are 0 and so are the moments
#pragma unroll
            for (int j = 0; j < kKnnMaxK; ++j) {         // R3: the chains in rank order
                const bool ok = (mask >> j) & 1u;
                mx = ok ? mx + qx[j] : mx;
                my = ok ? my + qy[j] : my;
                mz = ok ? mz + qz[j] : mz;
            }
            mx = mx / fn; my = my / fn; mz = mz / fn;
#pragma unroll
            for (int j = 0; j < kKnnMaxK; ++j) {
                const bool ok = (mask >> j) & 1u;
                const float ex = qx[j] - mx, ey = qy[j] - my, ez = qz[j] - mz;
                cxx = ok ? cxx + ex * ex : cxx;
                cxy = ok ? cxy + ex * ey : cxy;
                cxz = ok ? cxz + ex * ez : cxz;
                cyy = ok ? cyy + ey * ey : cyy;
                cyz = ok ? cyz + ey * ez : cyz;
                czz = ok ? czz + ez * ez : czz;
            }
            cxx = cxx / fn; cxy = cxy / fn; cxz = cxz / fn; cyy = cyy / fn; cyz = cyz / fn; czz = czz / fn;
            fl = normals_flag(n, min_neighbors, mx, my, mz, cxx, cxy, cxz, cyy, cyz, czz);   // R4
        }
        float nx = 0.0f, ny = 0.0f, nz = 0.0f, cv = 0.0f;
        if (fl == 0) normals_solve(cxx, cxy, cxz, cyy, cyz, czz, px, py, pz, v, voxel_room, viewpoint, V, nx, ny, nz, cv);   // R5, R6
        normals_store(v, nx, ny, nz, cv, n, fl, mx, my, mz, cxx, cxy, cxz, cyy, cyz, czz, normals, curvature, samples, flags, moments);
        c_ok += fl == 0;
        c_few += fl == 1;
        c_deg += fl == 2;
        c_fill += fl < 0;
    }
    if (c_ok) atomicAdd(&count_s[0], c_ok);
    if (c_few) atomicAdd(&count_s[1], c_few);
    if (c_deg) atomicAdd(&count_s[2], c_deg);
    if (c_fill) atomicAdd(&count_s[3], c_fill);
    __syncthreads();
    if (tid < 4 && count_s[tid]) atomicAdd(&normal_stats[tid], count_s[tid]);   // integers: exact in any order
}

}  // namespace conv3p
