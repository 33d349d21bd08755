// conv3p_scene_cover.hpp -- the covering mode of the block partition (conv3p_scene_blocks_cover_f32) and votes by
// summed class probabilities (conv3p_scene_vote_scores_f32, conv3p_scene_score_labels).  include/conv3p.h defines both;
// tests/scene_cover_ref.py restates them in numpy.
//
// Covering mode: a kept cell of n members gives q = ceil(n / P) blocks, part j holding the members of rank
// [floor(j n / q), floor((j + 1) n / q)) of the cell's ascending list, so every row of a kept cell is emitted.  The
// launches, all on one stream; bounds, finish, count, the two fill passes are conv3p_scene.hpp's as they are:
//
//   scene_bounds_kernel, scene_finish_kernel, scene_count_kernel
//   scene_cover_plan_kernel   one workgroup: cells row-major -> kept rank, first block number (a scan over q), and for
//                             the LISTED cells (first block number < max_blocks: a prefix of the kept cells) cell, count,
//                             list offset, first block; stats
//   scene_cover_table_kernel  a lane per emitted block: binary search over the listed cells' first block numbers ->
//                             {cell, list start + a_j, n_j, j * P}; no lane loops over a cell's parts
//   scene_fill_count_kernel, scene_fill_kernel   items (listed cell, row chunk): a member list is built once per cell
//   scene_cover_emit_kernel   scene_emit_body<true>: a workgroup per block, as the plain emit
//
// Votes: a workgroup's waves each stage tiles of 64 rows x C logits in LDS (consecutive words by consecutive lanes, as
// seg_head_kernel), a lane per row takes max, expf, the sum; then the tile's elements, again consecutive lanes on
// consecutive words, are divided, scaled by 2^30, rounded and added with 64-bit integer atomics: exact, so independent
// of order and launch geometry.  No float atomics anywhere in this file.
#pragma once

#include "conv3p_scene.hpp"

namespace conv3p {

constexpr int kScoreMaxClass = 128;
constexpr float kScoreScale = 1073741824.0f;       // 2^30

__global__ __launch_bounds__(kScenePlanThreads) void scene_cover_plan_kernel(const SceneArgs p)
{
    __shared__ int scan_s[kScenePlanThreads / 64];
    const SceneHeader h = *p.hdr;
    const int tid = threadIdx.x, P = p.P;
    const int need = p.min_points < 1 ? 1 : p.min_points;
    int c0, c1;
    wg_chunk(h.ncells, kScenePlanThreads, tid, &c0, &c1);
    int kept = 0, small = 0, parts = 0;                  // sum of q <= kept + 9 N / P < 2^31
    for (int c = c0; c < c1; ++c) {
        const int n = p.count[c];
        kept += n >= need ? 1 : 0;
        small += (n > 0 && n < need) ? 1 : 0;
        parts += n >= need ? (n + P - 1) / P : 0;
    }
    int kept_all, small_all, parts_all, listed_all, dummy;
    const int kbase = wg_exscan(kept, scan_s, tid, kScenePlanThreads, &kept_all);
    (void)wg_exscan(small, scan_s, tid, kScenePlanThreads, &small_all);
    const int pbase = wg_exscan(parts, scan_s, tid, kScenePlanThreads, &parts_all);
    // listed cells: first block number < max_blocks.  The first block numbers ascend with the kept rank, so the listed
    // cells are the kept ranks 0 .. listed_all - 1 (< kSceneMaxCells, as the cells themselves)
    int k = kbase, first = pbase, mine = 0, listed = 0;
    for (int c = c0; c < c1; ++c) {
        const int n = p.count[c];
        if (n < need) continue;
        if (first < p.max_blocks) {
            p.blk_cell[k] = c;
            p.blk_count[k] = n;
            p.blk_first[k] = first;
            mine += n;
            ++listed;
        }
        ++k;
        first += (n + P - 1) / P;
    }
    (void)wg_exscan(listed, scan_s, tid, kScenePlanThreads, &listed_all);
    int off = wg_exscan(mine, scan_s, tid, kScenePlanThreads, &dummy);
    k = kbase;
    first = pbase;
    for (int c = c0; c < c1; ++c) {
        const int n = p.count[c];
        if (n < need) continue;
        if (first < p.max_blocks) {
            p.blk_off[k] = off;
            off += n;
        }
        ++k;
        first += (n + P - 1) / P;
    }
    if (tid == 0) {
        const int ne = parts_all < p.max_blocks ? parts_all : p.max_blocks;
        p.hdr->nb = listed_all;
        p.hdr->ne = ne;
        p.stats[0] = ne;
        p.stats[1] = kept_all;
        p.stats[2] = h.nbx;
        p.stats[3] = h.nby;
        p.stats[4] = h.nonfinite;
        p.stats[5] = small_all;
        p.stats[6] = parts_all;
        p.stats[7] = h.error;
    }
}

__global__ __launch_bounds__(kSceneThreads) void scene_cover_table_kernel(const SceneArgs p)
{
    const SceneHeader h = *p.hdr;
    for (long long w = (long long)blockIdx.x * kSceneThreads + threadIdx.x; w < h.ne; w += (long long)gridDim.x * kSceneThreads) {
        const int b = (int)w;
        int lo = 0, hi = h.nb - 1;                       // the last listed cell whose first block is <= b
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (p.blk_first[mid] <= b) lo = mid; else hi = mid - 1;
        }
        const int n = p.blk_count[lo], j = b - p.blk_first[lo], q = (n + p.P - 1) / p.P;
        const int a0 = (int)((long long)j * n / q), a1 = (int)((long long)(j + 1) * n / q);
        p.table[b] = make_int4(p.blk_cell[lo], p.blk_off[lo] + a0, a1 - a0, j * p.P);
    }
}

__global__ __launch_bounds__(kSceneThreads) void scene_cover_emit_kernel(const SceneArgs p) { scene_emit_body<true>(p); }

// ------------------------------------------------------------------------------------- votes by summed probabilities
__host__ __device__ inline int score_ld(int C) { return C | 1; }
// dynamic LDS of a workgroup of nw waves: the two counters (64 bytes), the tiles, a sum and an index per tile row
inline size_t score_lds_bytes(int nw, int C) { return 64 + (size_t)nw * 64 * ((size_t)score_ld(C) + 2) * 4; }

__global__ __launch_bounds__(256) void scene_vote_scores_kernel(const float *__restrict__ logits,
                                                                const int32_t *__restrict__ index, size_t rows,
                                                                long long N, int C, long long *__restrict__ scores,
                                                                long long *__restrict__ stats)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (int)blockDim.x >> 6;
    const int ld = score_ld(C);
    int *cnt = reinterpret_cast<int *>(smem);                                       // {voted, refused}
    float *xs = reinterpret_cast<float *>(smem + 64) + (size_t)wave * 64 * ld;      // this wave's [64][ld]
    float *sum_s = reinterpret_cast<float *>(smem + 64) + (size_t)nw * 64 * ld + wave * 64;
    int *idx_s = reinterpret_cast<int *>(smem + 64) + (size_t)nw * 64 * (ld + 1) + wave * 64;
    if (threadIdx.x < 2) cnt[threadIdx.x] = 0;
    __syncthreads();

    // element e = lane + 64 k of a tile sits at row e / C, column e % C: advanced without a division per element
    const int q64 = 64 / C, r64 = 64 - q64 * C;
    const int row0 = lane / C, col0 = lane - row0 * C;
    const size_t tiles = (rows + 63) / 64;
    int voted = 0, refused = 0;

    for (size_t tile = (size_t)blockIdx.x * nw + wave; tile < tiles; tile += (size_t)gridDim.x * nw) {
        const size_t r0 = tile * 64;
        const int nrows = rows - r0 < 64 ? (int)(rows - r0) : 64;
        const int n = nrows * C;                                                    // <= 64 * 128
        const float *src = logits + r0 * C;
        {
            int row = row0, col = col0;
            for (int e = lane; e < n; e += 64) {
                xs[row * ld + col] = src[e];
                row += q64;
                col += r64;
                if (col >= C) { col -= C; ++row; }
            }
        }
        __builtin_amdgcn_wave_barrier();   // (LDS operations of a wave complete in order; this pins the program order)
        if (lane < nrows) {
            float *x = xs + lane * ld;
            const int i = index[r0 + lane];
            const bool inside = i >= 0 && (long long)i < N;
            float m = x[0];
            bool fin = isfinite(m);
            for (int c = 1; c < C; ++c) {
                const float v = x[c];
                fin = fin && isfinite(v);
                if (v > m) m = v;
            }
            const bool votes = inside && fin;
            if (votes) {
                float s = 0.0f;
                for (int c = 0; c < C; ++c) {
                    const float e = seg_exp(x[c] - m);
                    x[c] = e;
                    s += e;
                }
                sum_s[lane] = s;
            }
            idx_s[lane] = votes ? i : -1;
            voted += votes ? 1 : 0;
            refused += (inside && !fin) ? 1 : 0;
        }
        __builtin_amdgcn_wave_barrier();
        {
            int row = row0, col = col0;
            for (int e = lane; e < n; e += 64) {
                const int i = idx_s[row];
                if (i >= 0) {
                    const float pc = xs[row * ld + col] / sum_s[row];
                    const long long v = llrintf(pc * kScoreScale);
                    if (v) atomicAdd(reinterpret_cast<unsigned long long *>(scores + (size_t)i * C + col), (unsigned long long)v);
                }
                row += q64;
                col += r64;
                if (col >= C) { col -= C; ++row; }
            }
        }
        __builtin_amdgcn_wave_barrier();   // the next tile's staging overwrites what this pass read
    }
    for (int d = 32; d >= 1; d >>= 1) {
        voted += __shfl_xor(voted, d, 64);
        refused += __shfl_xor(refused, d, 64);
    }
    if (lane == 0) {
        if (voted) atomicAdd(&cnt[0], voted);
        if (refused) atomicAdd(&cnt[1], refused);
    }
    __syncthreads();
    if (threadIdx.x < 2 && cnt[threadIdx.x])
        atomicAdd(reinterpret_cast<unsigned long long *>(stats + threadIdx.x), (unsigned long long)cnt[threadIdx.x]);
}

__global__ __launch_bounds__(kSceneThreads) void scene_score_labels_kernel(const long long *scores, long long N, int C,
                                                                           int32_t *label_out, long long *partial)
{
    __shared__ int voted_s;
    if (threadIdx.x == 0) voted_s = 0;
    __syncthreads();
    int voted = 0;
    for (size_t r = (size_t)blockIdx.x * kSceneThreads + threadIdx.x; r < (size_t)N; r += (size_t)gridDim.x * kSceneThreads) {
        const long long *v = scores + r * C;
        int best = -1;
        long long most = 0;
        for (int c = 0; c < C; ++c) {
            const long long n = v[c];
            if (n > most) {
                most = n;
                best = c;
            }
        }
        label_out[r] = best;
        voted += best >= 0 ? 1 : 0;
    }
    for (int d = 32; d >= 1; d >>= 1) voted += __shfl_xor(voted, d, 64);
    if ((threadIdx.x & 63) == 0 && voted) atomicAdd(&voted_s, voted);
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = voted_s;
}

}  // namespace conv3p
