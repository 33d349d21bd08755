// conv3p_grid_interp.hpp -- voxel scores interpolated onto every raw row from its nearest voxels (conv3p_grid_neighbors,
// conv3p_grid_interpolate_f32 / _i64).
//
// include/conv3p.h defines the result by numbered rules and tests/grid_interp_ref.py restates it in numpy.  The voxels of
// a cloud are in ascending (i_x, i_y, i_z), so the voxel of a neighbouring cell is found by binary search in voxel_cell;
// inverse gives every raw row its own voxel.  Two kernels, one launch each:
//
//   grid_neighbors_kernel     a lane per (voxel, (dx, dy) column): one lower-bound search for the cell (i+dx, j+dy, l-1)
//                             by lexicographic compare on the triple, then up to three consecutive entries -- 9 searches
//                             a voxel, not 27; the nine lanes of a voxel write its 27 words side by side
//   grid_interpolate_kernel   16 lanes per raw row.  A lane takes candidates t and t + 16 of the voxel's 27 (so a row's
//                             108 bytes of the table are read side by side), forms their d2, and the group picks the k
//                             smallest (d2, voxel) keys by k butterfly minima over 64-bit keys; every lane then holds the
//                             k voxels and weights, and lane c blends classes c, c + 16, ...: the k score rows are read
//                             side by side, straight from global memory (a voxel's row serves all its members, so the
//                             reads hit the cache; staging them in LDS would add a barrier per step of rows and save no traffic),
//                             rows are taken in the order they come.  The label is the group's (value, class) maximum.
//
// The only atomics are integer adds (the three counts: a ballot per wave, LDS per workgroup, one 64-bit add per
// workgroup and count -- adds to one address retire one after the other, about 12 ns each on an MI355X, so the row kernel
// runs as at most 512 workgroups of 1024 threads that loop over the rows: with a workgroup per 16 rows the adds alone took
// 0.8 ms at 2^20 rows); every output word is written once by a plain store; a row's result depends on its own inputs
// alone, so nothing depends on the launch geometry.  All shuffles run with every lane of the wave active: a row past N,
// without a voxel or without a candidate goes through the same code with nothing selected.
#pragma once

#include "conv3p_grid.hpp"

namespace conv3p {

constexpr int kInterpGroup = 16;                // lanes of a raw row
constexpr int kInterpThreads = 1024;            // two workgroups fill a CU: the kernel keeps under 64 registers
constexpr int kInterpRows = kInterpThreads / kInterpGroup;  // rows of a workgroup's step
constexpr int kInterpMaxGrid = 512;             // the resident workgroups of 256 CUs: the rest is the row loop
constexpr int kInterpMaxK = 8;
constexpr int kInterpMaxClass = 128;
constexpr int kInterpNeigh = 27;

// the first position in [a, b) whose cell is not below (x, y, z), cells ascending in (i_x, i_y, i_z)
__device__ __forceinline__ int grid_cell_lower_bound(const int32_t *cell, int a, int b, int x, int y, int z)
{
    while (a < b) {
        const int mid = a + ((b - a) >> 1);
        const int32_t *c = cell + 3 * (size_t)mid;
        const int cx = c[0], cy = c[1], cz = c[2];
        const bool below = cx < x || (cx == x && (cy < y || (cy == y && cz < z)));
        if (below) a = mid + 1; else b = mid;
    }
    return a;
}

__global__ __launch_bounds__(kSceneThreads) void grid_neighbors_kernel(const int32_t *voxel_cell, const int32_t *voxel_room,
                                                                       const int32_t *voxel_start, const int32_t *grid_stats,
                                                                       int max_voxels, int num_rooms, int32_t *neigh)
{
    const int ne = clamped_count(grid_stats, max_voxels);
    const long long total = (long long)max_voxels * 9;
    for (long long w = (long long)blockIdx.x * kSceneThreads + threadIdx.x; w < total; w += (long long)gridDim.x * kSceneThreads) {
        const int v = (int)(w / 9), col = (int)(w - (long long)v * 9);
        int32_t *out = neigh + (size_t)v * kInterpNeigh + 3 * col;
        int a = 0, b = v < ne ? ne : 0;
        if (v < ne && voxel_room) {
            const int r = voxel_room[v];
            if (r >= 0 && r < num_rooms) {
                a = voxel_start[r];
                b = voxel_start[r + 1];
                a = a < 0 ? 0 : a;
                b = b > ne ? ne : b;
            } else {
                b = 0;
            }
        }
        int e = 0, x = 0, y = 0, z = 0;
        if (a < b) {
            const int32_t *c = voxel_cell + 3 * (size_t)v;
            x = c[0] + col / 3 - 1;
            y = c[1] + col % 3 - 1;
            z = c[2] - 1;
            e = grid_cell_lower_bound(voxel_cell, a, b, x, y, z);
        }
#pragma unroll
        for (int dz = 0; dz < 3; ++dz) {                 // distinct ascending cells: the three, if there, follow one another
            int hit = -1;
            if (e < b) {
                const int32_t *c = voxel_cell + 3 * (size_t)e;
                if (c[0] == x && c[1] == y && c[2] == z + dz) hit = e++;
            }
            out[dz] = hit;
        }
    }
}

__device__ __forceinline__ float interp_score(const float *s, size_t at) { return s[at]; }
// an exact fixed-point sum of SceneScores: converted with one rounding to nearest even, then scaled by 2^-30 exactly
__device__ __forceinline__ float interp_score(const long long *s, size_t at) { return (float)s[at] * 9.31322574615478515625e-10f; }

template <typename S>
__global__ __launch_bounds__(kInterpThreads) void grid_interpolate_kernel(const float *data, long long N, int K, const int32_t *inverse,
                                                                         const float *voxel_data, int Kv, const int32_t *neigh,
                                                                         const S *scores, int M, int C, const int32_t *valid,
                                                                         int k, int32_t *out_labels, float *out_scores,
                                                                         unsigned long long *stats)
{
    __shared__ int count_s[3];
    const int tid = threadIdx.x, gl = tid & (kInterpGroup - 1), grp = tid / kInterpGroup;
    const unsigned long long none = ~0ull;
    if (tid < 3) count_s[tid] = 0;
    int done = 0, no_voxel = 0, no_cand = 0;             // of this wave, the same in all its lanes
    for (long long base = (long long)blockIdx.x * kInterpRows; base < N; base += (long long)gridDim.x * kInterpRows) {
        const long long i = base + grp;
        const bool live = i < N;
        int v0 = live ? inverse[i] : -1;
        if (v0 >= M) v0 = -1;
        float px = 0.0f, py = 0.0f, pz = 0.0f;
        if (v0 >= 0) {
            const float *p = data + (size_t)i * K;
            px = p[0]; py = p[1]; pz = p[2];
        }
        unsigned long long key[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int t = gl + h * kInterpGroup;
            key[h] = none;
            if (v0 < 0 || t >= kInterpNeigh) continue;
            const int u = neigh[(size_t)v0 * kInterpNeigh + t];
            if (u < 0 || u >= M) continue;
            if (valid && valid[u] < 0) continue;
            const float *q = voxel_data + (size_t)u * Kv;
            const float dx = px - q[0], dy = py - q[1], dz = pz - q[2];
            const float d2 = ((dx * dx) + (dy * dy)) + (dz * dz);
            if (!(d2 < INFINITY)) continue;              // NaN or inf
            key[h] = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)u;   // d2 >= +0: its bits order as it does
        }
        int us[kInterpMaxK];
        float ws[kInterpMaxK];
        int cnt = 0;
#pragma unroll
        for (int j = 0; j < kInterpMaxK; ++j) {
            us[j] = 0;
            ws[j] = 0.0f;
            if (j < k) {                                 // k is the launch's: every lane of the wave is here
                unsigned long long m = key[0] < key[1] ? key[0] : key[1];
#pragma unroll
                for (int d = kInterpGroup / 2; d >= 1; d >>= 1) {
                    const unsigned long long o = __shfl_xor(m, d, 64);
                    m = o < m ? o : m;
                }
                if (m != none) {
                    if (key[0] == m) key[0] = none;      // a voxel is one candidate of the row: the keys are distinct
                    if (key[1] == m) key[1] = none;
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
        float best = -INFINITY;
        int cls = 0x7fffffff;
        bool nan0 = false;
        for (int c0 = 0; c0 < C; c0 += kInterpGroup) {   // C is the launch's
            const int c = c0 + gl;
            if (c >= C) continue;
            float o = 0.0f;
            if (cnt > 0) {
                float acc = ws[0] * interp_score(scores, (size_t)us[0] * C + c);
#pragma unroll
                for (int j = 1; j < kInterpMaxK; ++j)
                    if (j < cnt) acc = acc + ws[j] * interp_score(scores, (size_t)us[j] * C + c);
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
        const int nan_first = __shfl(nan0 ? 1 : 0, (tid & 63) & ~(kInterpGroup - 1), 64);   // class 0 is lane 0's
        const bool lead = live && gl == 0;
        if (lead) out_labels[i] = cnt > 0 ? (nan_first ? 0 : cls) : -1;
        done += __popcll(__ballot(lead && cnt > 0));
        no_voxel += __popcll(__ballot(lead && v0 < 0));
        no_cand += __popcll(__ballot(lead && v0 >= 0 && cnt == 0));
    }
    __syncthreads();
    if ((tid & 63) == 0) {
        if (done) atomicAdd(&count_s[0], done);
        if (no_voxel) atomicAdd(&count_s[1], no_voxel);
        if (no_cand) atomicAdd(&count_s[2], no_cand);
    }
    __syncthreads();
    if (tid < 3 && count_s[tid]) atomicAdd(&stats[tid], (unsigned long long)count_s[tid]);   // integers: exact in any order
}

}  // namespace conv3p
