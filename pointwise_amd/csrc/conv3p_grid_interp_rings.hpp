// conv3p_grid_interp_rings.hpp -- the fallback of the interpolated projection: a raw row whose 3 x 3 x 3 cells hold no
// candidate searches ring after ring of cells, up to Chebyshev distance `rings`, until one ring has a candidate
// (conv3p_grid_interpolate_rings_f32 / _i64).
//
// include/conv3p.h defines the result by rules 6-9 behind rules 1-5 of the plain call and tests/grid_interp_rings_ref.py
// restates it in numpy.  The plain pass is grid_interpolate_kernel as it stands (conv3p_grid_interp.hpp); two kernels
// follow it, one launch each, the second only with rings > 1:
//
//   grid_ring_list_kernel   a lane per raw row: the rows with a voxel whose label the plain pass left at -1 go into an
//                           int32 list in the workspace (a ballot per wave, one integer add per wave that has such a row on
//                           the list's counter, the lanes' places by the ballot's prefix); every other row gets its ring
//                           (1 labelled, 0 without a voxel), and the workgroup's counts go to ring_stats[0] and [1].  The
//                           order of the list is whatever the adds make it; no output depends on it.
//   grid_ring_search_kernel a fixed grid, a wave per listed row, the number of rows read from the workspace and held to
//                           [0, N].  For r = 2 .. rings the lanes go over the (dx, dy) columns of the shell of ring r --
//                           the cube of ring r - 1 is known to hold no candidate -- the 8r outer columns taking the cells
//                           l-r .. l+r, the (2r-1)^2 inner ones the two cells l-r and l+r.  A run of cells is one
//                           lower-bound search in the ascending cells of the row's room and a walk over consecutive
//                           entries that compares x, y and z (a lower bound in an empty column lands in the next one; a
//                           cell with a negative coordinate is not found).  A lane keeps its 8 smallest (d2 bits, voxel)
//                           keys sorted in registers by an unrolled insertion.  A ballot ends the ring: empty, the wave
//                           goes on to the next (the branch is the wave's); otherwise k butterfly minima over the lanes'
//                           heads select the voxels, lanes take classes c and c + 64 for the chains of rule 5, and the
//                           label is the wave's (value, class) maximum -- the code of the plain kernel, 64 lanes wide.
//
// The rows of the list are few and a row's work is large and irregular, so a row takes a wave and not a group of 16.  The
// counts: in registers per wave, LDS per workgroup, one 64-bit add per workgroup and count; the rows found move from
// stats[2] to stats[0] by the same adds (integers, exact in any order).  No float atomics.  A listed row's label and score
// row are written again only where a ring found a candidate; out_ring is written once.  Every loop is bounded whatever the
// memory holds: the search halves its range (at most 31 steps), a walk takes at most 2r + 1 entries, the columns are at
// most 17 * 17 = 289, the list at most the clamped count; every voxel number used lies in [0, ne), ne <= M, and a listed
// row outside [0, N) is passed over.  All shuffles run with the whole wave active.
#pragma once

#include "conv3p_grid_interp.hpp"

namespace conv3p {

constexpr int kRingMax = 8;                     // the largest Chebyshev distance: a cube of 17^3 cells
constexpr int kRingListThreads = 256;
constexpr int kRingListMaxGrid = 1024;          // 262 144 rows a pass, the rest is the row loop
constexpr int kRingThreads = 256;               // four waves, four rows of the list
constexpr int kRingWaves = kRingThreads / 64;
constexpr int kRingGrid = 1024;                 // fixed: 4096 rows a pass, the rest is the row loop
constexpr size_t kRingHeaderBytes = 256;        // the list's counter, the list behind it

__global__ __launch_bounds__(kRingListThreads) void grid_ring_list_kernel(const int32_t *inverse, const int32_t *labels, long long N,
                                                                         int M, int rings, int32_t *counter, int32_t *list,
                                                                         int32_t *out_ring, unsigned long long *ring_stats)
{
    __shared__ int count_s[2];
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < 2) count_s[tid] = 0;
    int listed = 0, plain = 0;                           // of this wave, the same in all its lanes
    for (long long base = ((long long)blockIdx.x * kRingListThreads + (tid & ~63)); base < N;
         base += (long long)gridDim.x * kRingListThreads) {
        const long long i = base + lane;
        const bool live = i < N;
        const int v0 = live ? inverse[i] : -1;
        const int lab = live ? labels[i] : 0;
        const bool has = v0 >= 0 && v0 < M;
        const bool want = has && lab == -1;
        const unsigned long long mask = __ballot(want);
        const int n = __popcll(mask);
        int at = 0;
        if (n) {                                         // the wave's
            if (lane == 0) at = atomicAdd(counter, n);
            at = __shfl(at, 0, 64);
        }
        if (want) {
            const long long slot = (long long)at + __popcll(mask & ((1ull << lane) - 1ull));
            if (slot >= 0 && slot < N) list[slot] = (int32_t)i;
        }
        if (live && out_ring && !(want && rings > 1)) out_ring[i] = has && lab >= 0 ? 1 : 0;   // a listed row's is the search's
        listed += n;
        plain += __popcll(__ballot(has && lab >= 0));
    }
    __syncthreads();
    if (lane == 0) {
        if (listed) atomicAdd(&count_s[0], listed);
        if (plain) atomicAdd(&count_s[1], plain);
    }
    __syncthreads();
    if (tid < 2 && count_s[tid]) atomicAdd(&ring_stats[tid], (unsigned long long)count_s[tid]);
}

// one more key into a lane's eight smallest, ascending: what falls off the end is dropped
__device__ __forceinline__ void ring_insert(unsigned long long (&b)[kInterpMaxK], unsigned long long x)
{
#pragma unroll
    for (int j = 0; j < kInterpMaxK; ++j) {
        const unsigned long long lo = x < b[j] ? x : b[j], hi = x < b[j] ? b[j] : x;
        b[j] = lo;
        x = hi;
    }
}

template <typename S>
__global__ __launch_bounds__(kRingThreads) void grid_ring_search_kernel(const float *data, long long N, int K, const int32_t *inverse,
                                                                       const float *voxel_data, int Kv, const int32_t *voxel_cell,
                                                                       const int32_t *voxel_room, const int32_t *voxel_start,
                                                                       int num_rooms, const int32_t *grid_stats, const S *scores,
                                                                       int M, int C, const int32_t *valid, int k, int rings,
                                                                       const int32_t *counter, const int32_t *list,
                                                                       int32_t *out_labels, float *out_scores, int32_t *out_ring,
                                                                       unsigned long long *stats, unsigned long long *ring_stats)
{
    __shared__ int count_s[kRingMax + 1];
    long long count = counter[0];
    count = count < 0 ? 0 : (count > N ? N : count);
    if ((long long)blockIdx.x * kRingWaves >= count) return;         // the workgroup's: nothing to do
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned long long none = ~0ull;
    if (tid <= kRingMax) count_s[tid] = 0;
    int ne = grid_stats[0];
    ne = ne < 0 ? 0 : (ne > M ? M : ne);
    int found[kRingMax + 1];                             // of this wave, the same in all its lanes; [0] is their sum
#pragma unroll
    for (int q = 0; q <= kRingMax; ++q) found[q] = 0;
    for (long long at = (long long)blockIdx.x * kRingWaves + wave; at < count; at += (long long)gridDim.x * kRingWaves) {
        const long long i = list[at];
        int v0 = i >= 0 && i < N ? inverse[i] : -1;
        if (v0 >= M) v0 = -1;
        if (v0 < 0) continue;                            // the wave's; never so for a list this call wrote
        int lo = 0, hi = v0 < ne ? ne : 0;
        if (v0 < ne && voxel_room) {
            const int room = voxel_room[v0];
            if (room >= 0 && room < num_rooms) {
                lo = voxel_start[room];
                hi = voxel_start[room + 1];
                lo = lo < 0 ? 0 : lo;
                hi = hi > ne ? ne : hi;
            } else {
                hi = 0;
            }
        }
        const float *p = data + (size_t)i * K;
        const float px = p[0], py = p[1], pz = p[2];
        const int32_t *own = voxel_cell + 3 * (size_t)v0;
        const int ca = own[0], cb = own[1], cl = own[2];
        unsigned long long best[kInterpMaxK];
#pragma unroll
        for (int j = 0; j < kInterpMaxK; ++j) best[j] = none;
        int ring = 0;
        for (int r = 2; r <= rings && lo < hi; ++r) {    // rings is the launch's, [lo, hi) the wave's
            const int side = 2 * r + 1;
            for (int col = lane; col < side * side; col += 64) {
                const int dx = col / side - r, dy = col - (col / side) * side - r;
                const int x = ca + dx, y = cb + dy;
                if (x < 0 || y < 0) continue;            // outside the lattice: not found
                const bool outer = dx == r || dx == -r || dy == r || dy == -r;
                const int len = outer ? side : 1;
                for (int half = 0; half < (outer ? 1 : 2); ++half) {
                    const int z0 = half ? cl + r : cl - r;
                    int e = grid_cell_lower_bound(voxel_cell, lo, hi, x, y, z0);
                    for (int w = 0; w < len && e < hi; ++w, ++e) {
                        const int32_t *c = voxel_cell + 3 * (size_t)e;
                        if (c[0] != x || c[1] != y || c[2] < z0 || c[2] - z0 >= len) break;
                        if (valid && valid[e] < 0) continue;
                        const float *q = voxel_data + (size_t)e * Kv;
                        const float ex = px - q[0], ey = py - q[1], ez = pz - q[2];
                        const float d2 = ((ex * ex) + (ey * ey)) + (ez * ez);
                        if (!(d2 < INFINITY)) continue;  // NaN or inf
                        ring_insert(best, ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)e);
                    }
                }
            }
            if (__ballot(best[0] != none)) {             // the first ring with a candidate ends the search
                ring = r;
                break;
            }
        }
        if (ring) {                                      // the wave's
            int us[kInterpMaxK];
            float ws[kInterpMaxK];
            int cnt = 0;
#pragma unroll
            for (int j = 0; j < kInterpMaxK; ++j) {
                us[j] = 0;
                ws[j] = 0.0f;
                if (j < k) {                             // k is the launch's: every lane of the wave is here
                    unsigned long long m = best[0];
#pragma unroll
                    for (int d = 32; d >= 1; d >>= 1) {
                        const unsigned long long o = __shfl_xor(m, d, 64);
                        m = o < m ? o : m;
                    }
                    if (m != none) {
                        if (best[0] == m) {              // a voxel is one candidate of the row: the keys are distinct
#pragma unroll
                            for (int t = 0; t + 1 < kInterpMaxK; ++t) best[t] = best[t + 1];
                            best[kInterpMaxK - 1] = none;
                        }
                        us[j] = (int)(unsigned)(m & 0xffffffffull);
                        ws[j] = 1.0f / fmaxf(__uint_as_float((unsigned)(m >> 32)), 1e-10f);
                        cnt = j + 1;
                    }
                }
            }
            float W = ws[0];
#pragma unroll
            for (int j = 1; j < kInterpMaxK; ++j)
                if (j < cnt) W = W + ws[j];
            float top = -INFINITY;
            int cls = 0x7fffffff;
            bool nan0 = false;
            for (int c0 = 0; c0 < C; c0 += 64) {         // C is the launch's
                const int c = c0 + lane;
                if (c >= C) continue;
                float acc = ws[0] * interp_score(scores, (size_t)us[0] * C + c);
#pragma unroll
                for (int j = 1; j < kInterpMaxK; ++j)
                    if (j < cnt) acc = acc + ws[j] * interp_score(scores, (size_t)us[j] * C + c);
                const float o = acc / W;
                if (out_scores) out_scores[(size_t)i * C + c] = o;
                if (c == 0) nan0 = o != o;
                const float x = o != o ? -INFINITY : o;  // a NaN never wins
                if (cls == 0x7fffffff || x > top) {      // ascending classes: the lowest of a lane's maxima
                    top = x;
                    cls = c;
                }
            }
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                const float ob = __shfl_xor(top, d, 64);
                const int oc = __shfl_xor(cls, d, 64);
                if (ob > top || (ob == top && oc < cls)) {
                    top = ob;
                    cls = oc;
                }
            }
            const int nan_first = __shfl(nan0 ? 1 : 0, 0, 64);       // class 0 is lane 0's
            if (lane == 0) out_labels[i] = nan_first ? 0 : cls;
        }
        if (lane == 0 && out_ring) out_ring[i] = ring;
#pragma unroll
        for (int q = 2; q <= kRingMax; ++q) found[q] += ring == q ? 1 : 0;
        found[0] += ring ? 1 : 0;
    }
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q <= kRingMax; ++q)
            if (q != 1 && found[q]) atomicAdd(&count_s[q], found[q]);
    }
    __syncthreads();
    if (tid >= 2 && tid <= kRingMax && count_s[tid]) atomicAdd(&ring_stats[tid], (unsigned long long)count_s[tid]);
    if (tid == 0 && count_s[0]) {                        // the rows found leave "no candidate" for "interpolated"
        atomicAdd(&stats[0], (unsigned long long)count_s[0]);
        atomicAdd(&stats[2], 0ull - (unsigned long long)count_s[0]);
    }
}

}  // namespace conv3p
