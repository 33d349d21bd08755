// conv3p_scene.hpp -- a room to model-sized blocks (conv3p_scene_blocks_f32) and block predictions back to a label per
// room row (conv3p_scene_vote, conv3p_scene_vote_labels).
//
// The block partition is PointNet's room2blocks_plus_normalized (indoor3d_util), which made the files the reference
// reads (scene_seg/s3dis_provider.py:9, :62-63); it is not in the reference tree, so include/conv3p.h DEFINES it (the
// ten steps there; tests/scene_ref.py restates them in numpy).  One room per call.  The launches, all on one stream:
//
//   scene_bounds_kernel      grid-stride over the rows: min / max of x, y, z over the finite rows and the number of other
//                            rows, one record per workgroup (butterflies, then the waves' records in wave order)
//   scene_finish_kernel      one workgroup: the records in record order -> lo, lim = max - lo (float32 subtraction is
//                            monotone, so this IS the maximum of v - lo), nbx, nby, the error flag; zeroes the cell counts
//   scene_count_kernel       a row tests its <= 4 x 4 candidate cells with the definition's own comparisons; counts in an
//                            LDS histogram (<= 8192 cells) or straight in global memory -- integer atomics, order-free
//   scene_plan_kernel        one workgroup: cells row-major -> block numbers, member offsets, stats
//   scene_fill_count_kernel  item (emitted block, row chunk): the number of the chunk's rows in the block's cell
//   scene_fill_kernel        the same items: ballot ranks behind the chunks' prefix, so a cell's member list comes out in
//                            ascending room row without a sort
//   scene_emit_kernel        a workgroup per block: slots -> rows (members, or Philox draws), the block minimum through
//                            LDS, then tiles of 256 rows staged in LDS and written as consecutive words by consecutive
//                            lanes, as provider_flat_kernel does; blocks past the emitted ones get the filler
//
// No float atomics; every output word is written once by a plain store.  The two fill passes cost (emitted blocks x
// rows) row tests: what the per-cell masks of the composed path cost, on 8 of a row's bytes.
//
// Draw of slot t of cell c: philox4x32_10(counter (t, 0x80000000 | c, step low, step high), key (seed low, seed
// high)).w[0] -> member (uint64(w) * n) >> 32.  c < 65536, so the counter's second word is >= 2^31 and below
// 0xFFFFFFFF: disjoint from the provider's (s + 1 < 2^31, 0xFFFFFFFF) and the dropout's (0).
#pragma once

#include "conv3p_cls_tail.hpp"
#include "conv3p_workgroup.hpp"

namespace conv3p {

constexpr int kSceneMaxCells = 65536;       // CONV3P_SCENE_MAX_CELLS
constexpr int kSceneMaxN = 1 << 24;
constexpr int kSceneMaxP = 65536;
constexpr int kSceneThreads = 256;
constexpr int kSceneMaxRecords = 1024;      // workgroups of scene_bounds_kernel = threads of scene_finish_kernel
constexpr int kScenePlanThreads = 1024;
constexpr int kSceneHistCells = 8192;       // cells of scene_count_kernel's LDS histogram (32 KB)
constexpr int kSceneMinChunk = 4096;        // rows of a fill chunk, at least
constexpr int kSceneMaxChunks = 256;        // chunks of a room, at most (= threads of scene_fill_kernel)
constexpr int kSceneMaxGrid = 65536;        // workgroups of the item loops, at most

struct SceneHeader {
    float lo[3], lim[3];
    int nbx, nby, ncells, nonfinite, error, nb;
    int ne;                            // the covering mode's emitted blocks (nb is then its listed cells)
};

struct SceneArgs {
    const float *data;                 // (N, K)
    const void *labels;                // (N), label_bytes each; may be NULL
    int N, K, label_bytes, P, min_points, max_blocks;
    float block, stride;
    unsigned seed_lo, seed_hi, step_lo, step_hi;
    float *blocks_out;                 // (max_blocks, P, K + 3)
    int32_t *labels_out, *index_out;   // (max_blocks, P); labels_out may be NULL
    int32_t *block_cell, *block_count; // (max_blocks)
    int32_t *stats;                    // 8 words
    // the workspace
    SceneHeader *hdr;
    float *records;                    // (records, 8): lo[3], hi[3], non-finite rows (an int's bits), -
    int *count;                        // (kSceneMaxCells)
    int *blk_cell, *blk_count, *blk_off;   // (min(max_blocks, kSceneMaxCells))
    int *chunk_count;                  // (emitted blocks, chunks)
    int *members;                      // the member lists, block after block
    int records_n, chunk_rows, chunks;
    // the covering mode only (conv3p_scene_cover.hpp): blk_* are per listed cell there
    int *blk_first;                    // (listed cells): a cell's first block number
    int4 *table;                       // (max_blocks): {cell, list start + a_j, n_j, j * P}
};

// Workgroup reduction of the lanes' ranges -> every thread gets the workgroup's.  red: (nthr / 64) * 7 floats.  min and
// max are exact, so the order does not matter to the bits; it is fixed all the same (butterfly, then wave order).
__device__ __forceinline__ SceneRange scene_reduce(SceneRange r, float *red, int tid, int nthr)
{
    for (int d = 32; d >= 1; d >>= 1) {
        for (int a = 0; a < 3; ++a) {
            r.lo[a] = fminf(r.lo[a], __shfl_xor(r.lo[a], d, 64));
            r.hi[a] = fmaxf(r.hi[a], __shfl_xor(r.hi[a], d, 64));
        }
        r.bad += __shfl_xor(r.bad, d, 64);
    }
    __syncthreads();
    if ((tid & 63) == 0) range_store(r, red + (tid >> 6) * 7);
    __syncthreads();
    SceneRange t;
    range_init(t);
    for (int w = 0; w < nthr / 64; ++w) range_fold(t, red + w * 7);
    return t;
}

__global__ __launch_bounds__(kSceneThreads) void scene_bounds_kernel(const SceneArgs p)
{
    __shared__ float red[(kSceneThreads / 64) * 7];
    const int tid = threadIdx.x;
    SceneRange r;
    range_init(r);
    for (size_t i = (size_t)blockIdx.x * kSceneThreads + tid; i < (size_t)p.N; i += (size_t)gridDim.x * kSceneThreads) {
        const float *v = p.data + i * p.K;
        range_add(r, v[0], v[1], v[2]);
    }
    r = scene_reduce(r, red, tid, kSceneThreads);
    if (tid == 0) {
        float *w = p.records + (size_t)blockIdx.x * 8;
        range_store(r, w);
        w[7] = 0.0f;
    }
}

// Cells along one axis: max(1, (int)ceil((double(lim) - double(block)) / double(stride)) + 1), held at 2^30 (an
// overflowed lim is +inf; anything near it is past kSceneMaxCells and reported as the error).
__host__ __device__ inline int scene_cells_along(float lim, float block, float stride)
{
    double q = ceil(((double)lim - (double)block) / (double)stride) + 1.0;
    if (!(q < 1073741824.0)) q = 1073741824.0;
    return q < 1.0 ? 1 : (int)q;
}

__global__ __launch_bounds__(kSceneMaxRecords) void scene_finish_kernel(const SceneArgs p)
{
    __shared__ float red[(kSceneMaxRecords / 64) * 7];
    __shared__ int ncells_s;
    const int tid = threadIdx.x;
    SceneRange r;
    range_init(r);
    if (tid < p.records_n) {                             // a thread takes one record: loaded over the empty range
        const float *w = p.records + (size_t)tid * 8;
        for (int a = 0; a < 3; ++a) {
            r.lo[a] = w[a];
            r.hi[a] = w[3 + a];
        }
        r.bad = __float_as_int(w[6]);
    }
    r = scene_reduce(r, red, tid, kSceneMaxRecords);
    if (tid == 0) {
        SceneHeader h;
        const bool any = r.bad < p.N;
        for (int a = 0; a < 3; ++a) {
            h.lo[a] = any ? r.lo[a] : 0.0f;
            h.lim[a] = any ? r.hi[a] - r.lo[a] : 0.0f;
        }
        h.nbx = any ? scene_cells_along(h.lim[0], p.block, p.stride) : 0;
        h.nby = any ? scene_cells_along(h.lim[1], p.block, p.stride) : 0;
        const long long cells = (long long)h.nbx * h.nby;
        h.error = cells > kSceneMaxCells ? 1 : 0;
        h.ncells = h.error ? 0 : (int)cells;
        h.nonfinite = r.bad;
        h.nb = 0;
        h.ne = 0;
        *p.hdr = h;
        ncells_s = h.ncells;
    }
    __syncthreads();
    for (int c = tid; c < ncells_s; c += kSceneMaxRecords) p.count[c] = 0;
}

// The candidate cells of a shifted coordinate along one axis: bit d of the result is cell i0 - 2 + d, i0 =
// floor(s / stride) in float32.  With block <= 2 stride a member cell i has i0 - 2 <= i <= i0 + 1 whatever the
// roundings of the quotient and of float(i) * stride; the comparisons are the definition's.
__device__ __forceinline__ unsigned scene_axis_mask(float s, float block, float stride, int ncell, int *first)
{
    const int i0 = (int)floorf(s / stride) - 2;
    unsigned m = 0;
    for (int d = 0; d < 4; ++d) {
        const int i = i0 + d;
        if (i < 0 || i >= ncell) continue;
        const float beg = (float)i * stride, end = beg + block;
        if (beg <= s && s <= end) m |= 1u << d;
    }
    *first = i0;
    return m;
}

__global__ __launch_bounds__(kSceneThreads) void scene_count_kernel(const SceneArgs p)
{
    __shared__ int hist[kSceneHistCells];
    const SceneHeader h = *p.hdr;
    if (h.ncells == 0) return;
    const int tid = threadIdx.x;
    const bool lds = h.ncells <= kSceneHistCells;
    if (lds) {
        for (int c = tid; c < h.ncells; c += kSceneThreads) hist[c] = 0;
        __syncthreads();
    }
    for (size_t i = (size_t)blockIdx.x * kSceneThreads + tid; i < (size_t)p.N; i += (size_t)gridDim.x * kSceneThreads) {
        const float *v = p.data + i * p.K;
        const float x = v[0], y = v[1], z = v[2];
        if (!scene_finite(x, y, z)) continue;
        int i0, j0;
        const unsigned mx = scene_axis_mask(x - h.lo[0], p.block, p.stride, h.nbx, &i0);
        const unsigned my = scene_axis_mask(y - h.lo[1], p.block, p.stride, h.nby, &j0);
        for (int di = 0; di < 4; ++di) {
            if (!((mx >> di) & 1u)) continue;
            for (int dj = 0; dj < 4; ++dj) {
                if (!((my >> dj) & 1u)) continue;
                const int c = (i0 + di) * h.nby + (j0 + dj);
                atomicAdd(lds ? &hist[c] : &p.count[c], 1);
            }
        }
    }
    if (lds) {
        __syncthreads();
        for (int c = tid; c < h.ncells; c += kSceneThreads) {
            const int n = hist[c];
            if (n) atomicAdd(&p.count[c], n);
        }
    }
}

__global__ __launch_bounds__(kScenePlanThreads) void scene_plan_kernel(const SceneArgs p)
{
    __shared__ int scan_s[kScenePlanThreads / 64];
    const SceneHeader h = *p.hdr;
    const int tid = threadIdx.x;
    const int need = p.min_points < 1 ? 1 : p.min_points;
    int c0, c1;
    wg_chunk(h.ncells, kScenePlanThreads, tid, &c0, &c1);
    int kept = 0, small = 0;
    for (int c = c0; c < c1; ++c) {
        const int n = p.count[c];
        kept += n >= need ? 1 : 0;
        small += (n > 0 && n < need) ? 1 : 0;
    }
    int kept_all, small_all, dummy;
    const int kbase = wg_exscan(kept, scan_s, tid, kScenePlanThreads, &kept_all);
    (void)wg_exscan(small, scan_s, tid, kScenePlanThreads, &small_all);
    const int limit = p.max_blocks < kSceneMaxCells ? p.max_blocks : kSceneMaxCells;
    int b = kbase, mine = 0;
    for (int c = c0; c < c1; ++c) {
        const int n = p.count[c];
        if (n < need) continue;
        if (b < limit) {
            p.blk_cell[b] = c;
            p.blk_count[b] = n;
            mine += n;
        }
        ++b;
    }
    int off = wg_exscan(mine, scan_s, tid, kScenePlanThreads, &dummy);
    b = kbase;
    for (int c = c0; c < c1; ++c) {
        const int n = p.count[c];
        if (n < need) continue;
        if (b < limit) {
            p.blk_off[b] = off;
            off += n;
        }
        ++b;
    }
    if (tid == 0) {
        const int nb = kept_all < limit ? kept_all : limit;
        p.hdr->nb = nb;
        p.stats[0] = nb;
        p.stats[1] = kept_all;
        p.stats[2] = h.nbx;
        p.stats[3] = h.nby;
        p.stats[4] = h.nonfinite;
        p.stats[5] = small_all;
        p.stats[6] = 0;
        p.stats[7] = h.error;
    }
}

struct SceneCell { float xbeg, xend, ybeg, yend; };

__device__ __forceinline__ SceneCell scene_cell(const SceneArgs &p, int c, int nby)
{
    const int i = c / nby, j = c - i * nby;
    SceneCell e;
    e.xbeg = (float)i * p.stride;
    e.xend = e.xbeg + p.block;
    e.ybeg = (float)j * p.stride;
    e.yend = e.ybeg + p.block;
    return e;
}

__device__ __forceinline__ bool scene_member(const SceneArgs &p, const SceneHeader &h, const SceneCell &e, int row)
{
    const float *v = p.data + (size_t)row * p.K;
    const float x = v[0], y = v[1], z = v[2];
    if (!scene_finite(x, y, z)) return false;
    const float sx = x - h.lo[0], sy = y - h.lo[1];
    return e.xbeg <= sx && sx <= e.xend && e.ybeg <= sy && sy <= e.yend;
}

__global__ __launch_bounds__(kSceneThreads) void scene_fill_count_kernel(const SceneArgs p)
{
    __shared__ int cnt_s;
    const SceneHeader h = *p.hdr;
    const int tid = threadIdx.x;
    const long long items = (long long)h.nb * p.chunks;
    for (long long w = blockIdx.x; w < items; w += gridDim.x) {
        const int b = (int)(w / p.chunks), ch = (int)(w - (long long)b * p.chunks);
        const SceneCell e = scene_cell(p, p.blk_cell[b], h.nby);
        if (tid == 0) cnt_s = 0;
        __syncthreads();
        const int r0 = ch * p.chunk_rows, r1 = r0 + p.chunk_rows < p.N ? r0 + p.chunk_rows : p.N;
        int n = 0;
        for (int r = r0 + tid; r < r1; r += kSceneThreads) n += scene_member(p, h, e, r) ? 1 : 0;
        for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d, 64);
        if ((tid & 63) == 0 && n) atomicAdd(&cnt_s, n);
        __syncthreads();
        if (tid == 0) p.chunk_count[w] = cnt_s;
        __syncthreads();
    }
}

__global__ __launch_bounds__(kSceneThreads) void scene_fill_kernel(const SceneArgs p)
{
    __shared__ int base_s, wave_s[kSceneThreads / 64];
    const SceneHeader h = *p.hdr;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long long items = (long long)h.nb * p.chunks;
    for (long long w = blockIdx.x; w < items; w += gridDim.x) {
        const int b = (int)(w / p.chunks), ch = (int)(w - (long long)b * p.chunks);
        if (p.chunk_count[w] == 0) continue;             // uniform over the workgroup
        const SceneCell e = scene_cell(p, p.blk_cell[b], h.nby);
        const int n_all = p.blk_count[b];
        int *list = p.members + p.blk_off[b];
        if (tid == 0) base_s = 0;
        __syncthreads();
        if (tid < ch) {                                  // chunks <= kSceneMaxChunks = the workgroup's threads
            const int n = p.chunk_count[(long long)b * p.chunks + tid];
            if (n) atomicAdd(&base_s, n);
        }
        __syncthreads();
        int run = base_s;
        const int r0 = ch * p.chunk_rows, r1 = r0 + p.chunk_rows < p.N ? r0 + p.chunk_rows : p.N;
        for (int t0 = r0; t0 < r1; t0 += kSceneThreads) {
            const int r = t0 + tid;
            const bool m = r < r1 && scene_member(p, h, e, r);
            const unsigned long long bal = __ballot(m);
            if (lane == 0) wave_s[wv] = __popcll(bal);
            __syncthreads();
            int before = 0, all = 0;
            for (int k = 0; k < kSceneThreads / 64; ++k) {
                const int s = wave_s[k];
                if (k < wv) before += s;
                all += s;
            }
            const int pos = run + before + __popcll(bal & ((1ull << lane) - 1ull));
            if (m && pos < n_all) list[pos] = r;         // pos < n_all holds by construction; the guard bounds the store
            run += all;
            __syncthreads();
        }
    }
}

// The emit of both modes.  kCover: block b is part j of its cell, (cell, list start + a_j, n_j, j * P) from the table --
// n_j <= P members, the draws among them, the counter's first word behind j * P.
template <bool kCover> __device__ __forceinline__ void scene_emit_body(const SceneArgs &p)
{
    __shared__ float xyz_s[kSceneThreads * 3], nrm_s[kSceneThreads * 3];
    __shared__ int row_s[kSceneThreads];
    __shared__ float min_s[(kSceneThreads / 64) * 2];
    const SceneHeader h = *p.hdr;
    const int tid = threadIdx.x, P = p.P, K = p.K, K3 = p.K + 3;
    for (int b = blockIdx.x; b < p.max_blocks; b += gridDim.x) {
        float *out = p.blocks_out + (size_t)b * P * K3;
        int32_t *idx = p.index_out + (size_t)b * P;
        int32_t *lab = p.labels_out ? p.labels_out + (size_t)b * P : nullptr;
        if (b >= (kCover ? h.ne : h.nb)) {               // the filler
            for (size_t e = tid; e < (size_t)P * K3; e += kSceneThreads) out[e] = 0.0f;
            for (int t = tid; t < P; t += kSceneThreads) {
                idx[t] = -1;
                if (lab) lab[t] = -1;
            }
            if (tid == 0) {
                p.block_cell[b] = -1;
                p.block_count[b] = 0;
            }
            continue;
        }
        int c, n, off;
        unsigned base = 0;
        if constexpr (kCover) {
            const int4 e = p.table[b];
            c = e.x; off = e.y; n = e.z; base = (unsigned)e.w;
        } else {
            c = p.blk_cell[b]; n = p.blk_count[b]; off = p.blk_off[b];
        }
        const int *list = p.members + off;
        if (tid == 0) {
            p.block_cell[b] = c;
            p.block_count[b] = n;
        }
        float mnx = INFINITY, mny = INFINITY;
        for (int t = tid; t < P; t += kSceneThreads) {
            int m = t;
            if ((!kCover && n > P) || t >= n) {
                const Philox4 w = philox4x32_10(base + (unsigned)t, 0x80000000u | (unsigned)c, p.step_lo, p.step_hi, p.seed_lo,
                                                p.seed_hi);
                m = (int)(((unsigned long long)w.w[0] * (unsigned long long)n) >> 32);
            }
            const int row = list[m];
            idx[t] = row;
            if (lab) lab[t] = row_label(p.labels, p.label_bytes, (size_t)row);
            const float *v = p.data + (size_t)row * K;
            mnx = fminf(mnx, v[0] - h.lo[0]);
            mny = fminf(mny, v[1] - h.lo[1]);
        }
        for (int d = 32; d >= 1; d >>= 1) {
            mnx = fminf(mnx, __shfl_xor(mnx, d, 64));
            mny = fminf(mny, __shfl_xor(mny, d, 64));
        }
        __syncthreads();                                 // the previous block's reads of min_s and the tiles
        if ((tid & 63) == 0) {
            min_s[(tid >> 6) * 2] = mnx;
            min_s[(tid >> 6) * 2 + 1] = mny;
        }
        __syncthreads();
        mnx = min_s[0];
        mny = min_s[1];
        for (int k = 1; k < kSceneThreads / 64; ++k) {
            mnx = fminf(mnx, min_s[2 * k]);
            mny = fminf(mny, min_s[2 * k + 1]);
        }
        const float half = p.block * 0.5f, cx = mnx + half, cy = mny + half;
        for (int t0 = 0; t0 < P; t0 += kSceneThreads) {
            const int t = t0 + tid;
            if (t < P) {
                const int row = idx[t];                  // this thread's own store of the loop above
                const float *v = p.data + (size_t)row * K;
                const float sx = v[0] - h.lo[0], sy = v[1] - h.lo[1], sz = v[2] - h.lo[2];
                row_s[tid] = row;
                xyz_s[3 * tid] = sx - cx;
                xyz_s[3 * tid + 1] = sy - cy;
                xyz_s[3 * tid + 2] = sz;
                nrm_s[3 * tid] = h.lim[0] == 0.0f ? 0.0f : sx / h.lim[0];
                nrm_s[3 * tid + 1] = h.lim[1] == 0.0f ? 0.0f : sy / h.lim[1];
                nrm_s[3 * tid + 2] = h.lim[2] == 0.0f ? 0.0f : sz / h.lim[2];
            }
            __syncthreads();
            const int cnt = P - t0 < kSceneThreads ? P - t0 : kSceneThreads;
            float *dst = out + (size_t)t0 * K3;
            for (int e = tid; e < cnt * K3; e += kSceneThreads) {
                const int r = e / K3, ch = e - r * K3;
                dst[e] = ch < 3 ? xyz_s[3 * r + ch] : (ch < K ? p.data[(size_t)row_s[r] * K + ch] : nrm_s[3 * r + ch - K]);
            }
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(kSceneThreads) void scene_emit_kernel(const SceneArgs p) { scene_emit_body<false>(p); }

// ---------------------------------------------------------------------------------------------- the way back
__global__ __launch_bounds__(kSceneThreads) void scene_vote_kernel(const int32_t *pred, const int32_t *index, size_t rows,
                                                                   long long N, int C, int32_t *votes)
{
    for (size_t r = (size_t)blockIdx.x * kSceneThreads + threadIdx.x; r < rows; r += (size_t)gridDim.x * kSceneThreads) {
        const int i = index[r], c = pred[r];
        if (i >= 0 && (long long)i < N && c >= 0 && c < C) atomicAdd(&votes[(size_t)i * C + c], 1);
    }
}

__global__ __launch_bounds__(kSceneThreads) void scene_vote_labels_kernel(const int32_t *votes, long long N, int C,
                                                                          int32_t *label_out, long long *partial)
{
    __shared__ int voted_s;
    if (threadIdx.x == 0) voted_s = 0;
    __syncthreads();
    int voted = 0;
    for (size_t r = (size_t)blockIdx.x * kSceneThreads + threadIdx.x; r < (size_t)N; r += (size_t)gridDim.x * kSceneThreads) {
        const int32_t *v = votes + r * C;
        int best = -1, most = 0;
        for (int c = 0; c < C; ++c) {
            const int n = v[c];
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

__global__ __launch_bounds__(kSceneMaxRecords) void scene_vote_finish_kernel(const long long *partial, int n, long long N,
                                                                             long long *stats)
{
    __shared__ long long sum_s[kSceneMaxRecords / 64];
    const int tid = threadIdx.x;
    long long v = tid < n ? partial[tid] : 0;
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    if ((tid & 63) == 0) sum_s[tid >> 6] = v;
    __syncthreads();
    if (tid == 0) {
        long long t = 0;
        for (int w = 0; w < kSceneMaxRecords / 64; ++w) t += sum_s[w];
        stats[0] = t;
        stats[1] = N - t;
    }
}

}  // namespace conv3p
