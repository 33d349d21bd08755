// conv3p_grid.hpp -- voxel-grid subsampling of one cloud, labels projected back (conv3p_grid_subsample_f32,
// conv3p_grid_project_labels).
//
// include/conv3p.h defines the result in eight steps and tests/grid_ref.py restates it in numpy.  The rooms call's idea
// on a 3-D lattice: every finite row writes one (cell id, row) pair in row order, a stable least-significant-digit radix
// sort groups the pairs by cell, so a voxel's member list is a run of the sorted pairs in ascending row.  A cell id has
// up to 40 bits and a row 24, so a pair is c << 24 | row in 64 bits and the sort takes 8 bits a pass, five passes at the
// most.  The launches, all on one stream, their number fixed by the arguments:
//
//   grid_bounds_kernel        a workgroup per tile of 1024 rows: one record {min, max of x, y, z over the finite rows,
//                             other rows}
//   grid_frame_kernel         one workgroup: the records -> lo, n_x, n_y, n_z, cells, the error; the prefix of the
//                             tiles' finite rows -> where a tile's pairs start; M pairs, T sort tiles, the passes the
//                             cell ids need (ceil(bits of cells - 1 / 8): the passes above are skipped by this word)
//   grid_pairs_kernel         the same tiles again: the pairs in row order; inverse = -1 for a row without a pair
//   5 x { grid_sort_hist_kernel     per sort tile of 4096 pairs a histogram of 8 bits of the cell id (radix_hist_tile)
//         grid_sort_scan_kernel     a workgroup per digit: prefix over (digit, tile) from the digits' totals
//                                   (radix_digit_scan)
//         grid_sort_scatter_kernel  one WAVE per sort tile, 64 pairs a step in order (radix_scatter_tile): the lanes of
//                                   equal digit from eight ballots, rank = popcount below the lane }
//                             pass p reads buffer p & 1 and writes the other; a skipped pass returns at once, so the
//                             sorted pairs are in buffer passes & 1
//   grid_heads_kernel<0>      per sort tile the pairs whose cell differs from the pair before: the lists' heads
//   grid_heads_scan_kernel    one workgroup: prefix of the tiles' heads (wg_exscan_inplace) -> voxel numbers; occupied
//                             and emitted voxels
//   grid_heads_kernel<1>      the same tiles again: start[v] = the position of voxel v's head; start[V] = M
//   grid_voxel_kernel         eight lanes per voxel: count, cell, inverse of every member; mean: voxel_row and the majority
//                             label by the group's LDS histogram; centre: the representative, its row copied
//   grid_mean_kernel          (mean only) a thread per (voxel, channel): the serial chain over the list, the loads of
//                             eight members issued together, the additions in list order
//   grid_stats_kernel         one workgroup: the largest member count from the voxel kernel's partial maxima; stats
//
// No float atomics (the only atomics are integer adds: the two LDS histograms and a pass's totals per digit); every output word is written once by a
// plain store; the result does not depend on the launch geometry.  The scans, the radix pass and the bounding-box
// records are conv3p_workgroup.hpp's.
#pragma once

#include "conv3p_scene_rooms.hpp"

namespace conv3p {

constexpr int kGridMaxN = 1 << 24;              // a row has 24 bits of a pair
constexpr int kGridMaxAxis = 1 << 20;           // cells along one axis
constexpr long long kGridMaxCells = 1ll << 40;  // cells of the lattice: 40 bits of a pair
constexpr int kGridMaxClass = 128;
constexpr int kGridRowTile = 1024;              // rows of a workgroup of the bounds and pairs kernels: 4 a thread
constexpr int kGridSortTile = 4096;             // pairs of a sort tile: 16 a thread of the heads kernels
constexpr int kGridDigitBits = 8;
constexpr int kGridDigits = 1 << kGridDigitBits;
constexpr int kGridPasses = 5;                  // 5 x 8 bits >= the 40 bits of a cell id
constexpr int kGridRowBits = 24;
constexpr int kGridScanThreads = 1024;
constexpr int kGridGroup = 8;                   // lanes of a voxel in grid_voxel_kernel
constexpr int kGridVoxelGroups = kSceneThreads / kGridGroup;
static_assert(kSceneThreads == kGridDigits, "a thread per digit in grid_sort_hist_kernel");

struct GridHeader {
    float lo[3];
    int n[3];                          // stats[2..4]
    long long cells;                   // 0 with the error or without a finite row
    int error, nonfinite;
    int pairs, sort_tiles, passes;     // M, T = ceil(M / kGridSortTile), the sort passes that run
    int occupied, emitted;             // V, min(V, max_voxels)
};

struct GridArgs {
    const float *data;                 // (N, K)
    const void *labels;                // (N), label_bytes each; may be NULL
    int N, K, label_bytes, mode, num_class, max_voxels;
    float voxel;
    float *out;                        // (max_voxels, K)
    int32_t *labels_out;               // (max_voxels); may be NULL
    int32_t *voxel_row, *voxel_count, *voxel_cell, *inverse, *stats;
    // the workspace
    GridHeader *hdr;
    float *records;                    // (row tiles, 8)
    int *tile_off;                     // (row tiles)
    int *hist;                         // (kGridDigits, sort tiles)
    int *digit_total;                  // (kGridPasses, kGridDigits): a pass's pairs per digit, zeroed by the frame kernel
    int *heads;                        // (sort tiles)
    int *start;                        // (N + 1)
    int *part_max;                     // (workgroups of the voxel kernel)
    unsigned long long *pairs_a, *pairs_b;             // (N) each: c << 24 | row
    int row_tiles, voxel_grid;
};

// i = (int)floorf(s / voxel), one correctly rounded float32 division, held at 2^30 (an overflowed s is +inf; anything
// near the bound is past kGridMaxAxis and reported as the error).
__device__ __forceinline__ int grid_axis_cell(float s, float voxel)
{
    float q = floorf(s / voxel);
    if (!(q < 1073741824.0f)) q = 1073741824.0f;
    return (int)q;
}

__global__ __launch_bounds__(kSceneThreads) void grid_bounds_kernel(const GridArgs p)
{
    __shared__ float red[(kSceneThreads / 64) * 7];
    const int tid = threadIdx.x, tile = blockIdx.x;
    const int t0 = tile * kGridRowTile, t1 = t0 + kGridRowTile < p.N ? t0 + kGridRowTile : p.N;
    SceneRange g;
    range_init(g);
    for (int i = t0 + tid; i < t1; i += kSceneThreads) {
        const float *v = p.data + (size_t)i * p.K;
        range_add(g, v[0], v[1], v[2]);
    }
    g = scene_reduce(g, red, tid, kSceneThreads);
    if (tid == 0) {
        float *w = p.records + (size_t)tile * 8;
        range_store(g, w);
        w[7] = 0.0f;
    }
}

__global__ __launch_bounds__(kGridScanThreads) void grid_frame_kernel(const GridArgs p)
{
    __shared__ float red[(kGridScanThreads / 64) * 7];
    __shared__ int scan_s[kGridScanThreads / 64];
    const int tid = threadIdx.x;
    int a, b;
    wg_chunk(p.row_tiles, kGridScanThreads, tid, &a, &b);
    for (int e = tid; e < kGridPasses * kGridDigits; e += kGridScanThreads) p.digit_total[e] = 0;
    SceneRange g;
    range_init(g);
    int fin = 0;                                         // the finite rows of this thread's tiles
    for (int t = a; t < b; ++t) {
        const float *w = p.records + (size_t)t * 8;
        const int rows = (t + 1) * kGridRowTile <= p.N ? kGridRowTile : p.N - t * kGridRowTile;
        range_fold(g, w);
        fin += rows - __float_as_int(w[6]);
    }
    g = scene_reduce(g, red, tid, kGridScanThreads);
    int total;
    int run = wg_exscan(fin, scan_s, tid, kGridScanThreads, &total);
    for (int t = a; t < b; ++t) {
        const float *w = p.records + (size_t)t * 8;
        const int rows = (t + 1) * kGridRowTile <= p.N ? kGridRowTile : p.N - t * kGridRowTile;
        p.tile_off[t] = run;
        run += rows - __float_as_int(w[6]);
    }
    if (tid == 0) {
        GridHeader h;
        const bool any = g.bad < p.N;
        long long cells = any ? 1 : 0;
        bool over = false;
        for (int e = 0; e < 3; ++e) {
            // a zero minimum has one sign whatever the order of the reduction (see SceneRange).  s and the quotient are
            // monotone in v, so the largest cell along an axis is the cell of the largest coordinate.
            h.lo[e] = any ? g.lo[e] : 0.0f;
            h.n[e] = any ? grid_axis_cell(g.hi[e] - g.lo[e], p.voxel) + 1 : 0;
            if (h.n[e] > kGridMaxAxis) over = true;
        }
        if (!over) cells = (long long)h.n[0] * h.n[1] * h.n[2];      // <= 2^60
        if (!over && cells > kGridMaxCells) over = true;
        h.error = over ? 1 : 0;
        h.cells = over ? 0 : cells;
        h.nonfinite = g.bad;
        h.pairs = over ? 0 : total;
        h.sort_tiles = (h.pairs + kGridSortTile - 1) / kGridSortTile;
        const int bits = h.cells > 1 ? 64 - __clzll(h.cells - 1) : 0;
        h.passes = (bits + kGridDigitBits - 1) / kGridDigitBits;
        h.occupied = 0;
        h.emitted = 0;
        *p.hdr = h;
    }
}

// The pairs in row order: a thread takes 4 consecutive rows, so thread order is row order.
__global__ __launch_bounds__(kSceneThreads) void grid_pairs_kernel(const GridArgs p)
{
    __shared__ int scan_s[kSceneThreads / 64];
    const int tid = threadIdx.x, tile = blockIdx.x;
    const GridHeader h = *p.hdr;
    const int t0 = tile * kGridRowTile, t1 = t0 + kGridRowTile < p.N ? t0 + kGridRowTile : p.N;
    unsigned long long key[4];
    bool has[4];
    int n = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = t0 + 4 * tid + k;
        has[k] = false;
        key[k] = 0ull;
        if (i >= t1) continue;
        const float *v = p.data + (size_t)i * p.K;
        const float x = v[0], y = v[1], z = v[2];
        if (!h.error && scene_finite(x, y, z)) {
            const long long ix = grid_axis_cell(x - h.lo[0], p.voxel), iy = grid_axis_cell(y - h.lo[1], p.voxel),
                            iz = grid_axis_cell(z - h.lo[2], p.voxel);
            const long long c = (ix * h.n[1] + iy) * h.n[2] + iz;                    // < cells <= 2^40
            key[k] = ((unsigned long long)c << kGridRowBits) | (unsigned long long)i;
            has[k] = true;
            ++n;
        } else {
            p.inverse[i] = -1;
        }
    }
    int total;
    int pos = p.tile_off[tile] + wg_exscan(n, scan_s, tid, kSceneThreads, &total);
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (has[k] && pos < h.pairs) p.pairs_a[pos++] = key[k];                     // pos < M <= N: the frame's prefix
}

// ------------------------------------------------------------------------------------------ the radix sort's pass
__global__ __launch_bounds__(kSceneThreads) void grid_sort_hist_kernel(const GridArgs p, int pass)
{
    __shared__ int hist_s[kGridDigits];
    const int tid = threadIdx.x, M = p.hdr->pairs, T = p.hdr->sort_tiles;
    if (pass >= p.hdr->passes) return;
    const unsigned long long *src = (pass & 1) ? p.pairs_b : p.pairs_a;
    const int shift = kGridRowBits + pass * kGridDigitBits;
    int mine = 0;                                        // this workgroup's pairs of digit tid: kSceneThreads == kGridDigits
    for (int tile = blockIdx.x; tile < T; tile += gridDim.x)
        mine += radix_hist_tile<kGridDigitBits>(src, M, tile, kGridSortTile, shift, hist_s, p.hist, T, tid, kSceneThreads);
    if (mine) atomicAdd(&p.digit_total[pass * kGridDigits + tid], mine);   // integers: exact in any order
}

// A workgroup per digit: radix_digit_scan from this pass's totals.
__global__ __launch_bounds__(kGridScanThreads) void grid_sort_scan_kernel(const GridArgs p, int pass)
{
    __shared__ int scan_s[kGridScanThreads / 64];
    const int digit = blockIdx.x, T = p.hdr->sort_tiles;
    if (pass >= p.hdr->passes) return;
    radix_digit_scan(p.digit_total + pass * kGridDigits, p.hist + (size_t)digit * T, T, digit, scan_s, threadIdx.x,
                     kGridScanThreads);
}

__global__ __launch_bounds__(64) void grid_sort_scatter_kernel(const GridArgs p, int pass)
{
    __shared__ int run_s[kGridDigits];
    const int M = p.hdr->pairs, T = p.hdr->sort_tiles;
    if (pass >= p.hdr->passes) return;
    const unsigned long long *src = (pass & 1) ? p.pairs_b : p.pairs_a;
    unsigned long long *dst = (pass & 1) ? p.pairs_a : p.pairs_b;
    const int shift = kGridRowBits + pass * kGridDigitBits;
    for (int tile = blockIdx.x; tile < T; tile += gridDim.x)
        radix_scatter_tile<kGridDigitBits, int>(src, dst, M, tile, kGridSortTile, shift, p.hist, T, run_s, threadIdx.x);
}

// ------------------------------------------------------------------------------------------ lists behind the sort
// A pair is a head if the pair before it is of another cell.  kWrite = false: the tile's heads.  kWrite = true: start[v]
// of the tile's heads, v behind the tiles' prefix.  A thread takes 16 consecutive pairs, so thread order is pair order.
template <bool kWrite> __global__ __launch_bounds__(kSceneThreads) void grid_heads_kernel(const GridArgs p)
{
    __shared__ int scan_s[kSceneThreads / 64];
    const int tid = threadIdx.x;
    const GridHeader h = *p.hdr;
    const int M = h.pairs, T = h.sort_tiles;
    const unsigned long long *sorted = (h.passes & 1) ? p.pairs_b : p.pairs_a;
    if (kWrite && blockIdx.x == 0 && tid == 0) p.start[h.occupied] = M;   // occupied <= M <= N
    for (int tile = blockIdx.x; tile < T; tile += gridDim.x) {
        const int i0 = tile * kGridSortTile + tid * 16;
        const int i1 = i0 + 16 < M ? i0 + 16 : M;
        unsigned long long prev = i0 > 0 && i0 < M ? sorted[i0 - 1] >> kGridRowBits : ~0ull;
        const unsigned long long first = prev;
        int n = 0;
        for (int i = i0; i < i1; ++i) {
            const unsigned long long c = sorted[i] >> kGridRowBits;
            n += (i == 0 || c != prev) ? 1 : 0;
            prev = c;
        }
        int total;
        int v = wg_exscan(n, scan_s, tid, kSceneThreads, &total);
        if (!kWrite) {
            if (tid == 0) p.heads[tile] = total;
        } else {
            v += p.heads[tile];
            prev = first;
            for (int i = i0; i < i1; ++i) {
                const unsigned long long c = sorted[i] >> kGridRowBits;
                if (i == 0 || c != prev) {
                    if (v < p.N) p.start[v] = i;             // v < V <= N
                    ++v;
                }
                prev = c;
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kGridScanThreads) void grid_heads_scan_kernel(const GridArgs p)
{
    __shared__ int scan_s[kGridScanThreads / 64];
    const int tid = threadIdx.x;
    const int total = wg_exscan_inplace(p.heads, p.hdr->sort_tiles, scan_s, tid, kGridScanThreads);
    if (tid == 0) {
        p.hdr->occupied = total;
        p.hdr->emitted = total < p.max_voxels ? total : p.max_voxels;
    }
}

// Is the label of row idx in [0, num_class)?  Compared in the label's own width, so an int64 label is not wrapped first
// -- which is why this is not row_label: 2^32 + 3 is no label, and row_label makes it 3.
__device__ __forceinline__ int grid_valid_label(const GridArgs &p, size_t idx)
{
    long long l;
    if (p.label_bytes == 1) l = (long long) static_cast<const uint8_t *>(p.labels)[idx];
    else if (p.label_bytes == 4) l = (long long) static_cast<const int32_t *>(p.labels)[idx];
    else l = static_cast<const long long *>(p.labels)[idx];
    return l >= 0 && l < (long long)p.num_class ? (int)l : -1;
}

// The frame of one room of conv3p_grid_subsample_rooms_f32 (conv3p_grid_rooms.hpp), and what grid_voxel_body reads of
// the rooms: a voxel's cell id is cell_base[r] + c, c the id in room r's own lattice.
struct GridRoomFrame {
    float lo[3];
    int n[3];                          // room_stats[r][2..4]
    long long cells;                   // 0 with the room's error, without a finite row, and when nothing may be emitted
    int error, nonfinite;
    int pairs, pad;                    // the room's finite rows (0 where cells is 0)
};

struct GridRoomsView {
    const GridRoomFrame *room;         // (R)
    const long long *cell_base;        // (R + 1): the prefix of the rooms' cells
    int32_t *voxel_room;               // (max_voxels)
    int R;
};

// Eight lanes per voxel, v over the occupied voxels and the fillers behind them: short lists dominate, and a list of any
// length is walked eight members a step.  Everything a group does depends on its own voxel alone; the shuffles stay
// inside the group's eight lanes, which are active together.  kRooms: the voxel's room by binary search in cell_base,
// the cell decoded with the room's n, the centre's s formed with the room's lo; the rows are global either way.
template <bool kRooms> __device__ __forceinline__ void grid_voxel_body(const GridArgs &p, const GridRoomsView &rv)
{
    __shared__ int hist_s[kGridVoxelGroups][kGridMaxClass];
    __shared__ int max_s[kSceneThreads / 64];
    const int tid = threadIdx.x, gl = tid & (kGridGroup - 1), grp = tid / kGridGroup;
    const GridHeader h = *p.hdr;
    const unsigned long long *sorted = (h.passes & 1) ? p.pairs_b : p.pairs_a;
    const int V = h.occupied, ne = h.emitted, K = p.K;
    const int bound = V > p.max_voxels ? V : p.max_voxels;
    const bool mean = p.mode == 0;
    const int C = (mean && p.labels) ? p.num_class : 0;  // <= kGridMaxClass
    for (int c = gl; c < C; c += kGridGroup) hist_s[grp][c] = 0;
    int longest = 0;
    for (long long w = (long long)blockIdx.x * kGridVoxelGroups + grp; w < bound; w += (long long)gridDim.x * kGridVoxelGroups) {
        const int v = (int)w;
        if (v >= V) {                                    // a filler: v < max_voxels
            if (gl == 0) {
                p.voxel_row[v] = -1;
                p.voxel_count[v] = 0;
                p.voxel_cell[3 * (size_t)v] = -1;
                p.voxel_cell[3 * (size_t)v + 1] = -1;
                p.voxel_cell[3 * (size_t)v + 2] = -1;
                if (p.labels_out) p.labels_out[v] = -1;
                if (kRooms) rv.voxel_room[v] = -1;
            }
            if (!mean)
                for (int k = gl; k < K; k += kGridGroup) p.out[(size_t)v * K + k] = 0.0f;
            continue;
        }
        const int s0 = p.start[v], n = p.start[v + 1] - s0;
        longest = n > longest ? n : longest;
        const bool emit = v < ne;
        const unsigned long long head = sorted[s0];
        long long c = (long long)(head >> kGridRowBits);
        int room = 0, n1 = h.n[1], n2 = h.n[2];
        float lo0 = h.lo[0], lo1 = h.lo[1], lo2 = h.lo[2];
        if (kRooms) {
            int rl = 0, rh = rv.R - 1;                   // the last room whose cell_base is <= c: the one with cells
            while (rl < rh) {
                const int mid = (rl + rh + 1) >> 1;
                if (rv.cell_base[mid] <= c) rl = mid; else rh = mid - 1;
            }
            const GridRoomFrame *f = rv.room + rl;
            room = rl;
            c -= rv.cell_base[rl];
            n1 = f->n[1] > 0 ? f->n[1] : 1;
            n2 = f->n[2] > 0 ? f->n[2] : 1;
            lo0 = f->lo[0]; lo1 = f->lo[1]; lo2 = f->lo[2];
        }
        const int iz = (int)(c % n2), iy = (int)((c / n2) % n1), ix = (int)(c / ((long long)n2 * n1));
        float best = INFINITY;
        int best_row = 0x7fffffff;
        const float cx = ((float)ix + 0.5f) * p.voxel, cy = ((float)iy + 0.5f) * p.voxel, cz = ((float)iz + 0.5f) * p.voxel;
        for (int j = gl; j < n; j += kGridGroup) {
            const int row = (int)(sorted[s0 + j] & ((1ull << kGridRowBits) - 1ull));
            p.inverse[row] = emit ? v : -1;
            if (!emit) continue;
            if (mean) {
                if (C) {
                    const int l = grid_valid_label(p, (size_t)row);
                    if (l >= 0) atomicAdd(&hist_s[grp][l], 1);
                }
            } else {
                const float *q = p.data + (size_t)row * K;
                const float dx = (q[0] - lo0) - cx, dy = (q[1] - lo1) - cy, dz = (q[2] - lo2) - cz;
                const float d = ((dx * dx) + (dy * dy)) + (dz * dz);
                // a lane's rows ascend, so a strict comparison keeps the lowest row of equal distances; the first
                // member is taken whatever its distance (an overflowed one is +inf)
                if (best_row == 0x7fffffff || d < best) {
                    best = d;
                    best_row = row;
                }
            }
        }
        if (!emit) continue;                             // uniform over the group
        int rep = (int)(head & ((1ull << kGridRowBits) - 1ull));   // mean: the lowest member row
        int label = -1;
        if (mean) {
            if (C) {
                // the group's LDS adds are done: its lanes are of one wave, whose LDS operations complete in order
                __builtin_amdgcn_wave_barrier();
                int cnt = 0, cls = 0;
                for (int k = gl; k < C; k += kGridGroup) {   // ascending classes: a lane keeps the lowest of its maxima
                    const int x = hist_s[grp][k];
                    hist_s[grp][k] = 0;
                    if (x > cnt) {
                        cnt = x;
                        cls = k;
                    }
                }
                for (int d = kGridGroup / 2; d >= 1; d >>= 1) {
                    const int oc = __shfl_xor(cnt, d, 64), ol = __shfl_xor(cls, d, 64);
                    if (oc > cnt || (oc == cnt && ol < cls)) {
                        cnt = oc;
                        cls = ol;
                    }
                }
                label = cnt > 0 ? cls : -1;
                __builtin_amdgcn_wave_barrier();
            }
        } else {
            for (int d = kGridGroup / 2; d >= 1; d >>= 1) {
                const float ob = __shfl_xor(best, d, 64);
                const int orow = __shfl_xor(best_row, d, 64);
                if (orow != 0x7fffffff && (best_row == 0x7fffffff || ob < best || (ob == best && orow < best_row))) {
                    best = ob;
                    best_row = orow;
                }
            }
            rep = best_row;
            if (p.labels) label = row_label(p.labels, p.label_bytes, (size_t)rep);
            const float *q = p.data + (size_t)rep * K;
            for (int k = gl; k < K; k += kGridGroup) p.out[(size_t)v * K + k] = q[k];
        }
        if (gl == 0) {
            p.voxel_row[v] = rep;
            p.voxel_count[v] = n;
            p.voxel_cell[3 * (size_t)v] = ix;
            p.voxel_cell[3 * (size_t)v + 1] = iy;
            p.voxel_cell[3 * (size_t)v + 2] = iz;
            if (p.labels_out) p.labels_out[v] = label;
            if (kRooms) rv.voxel_room[v] = room;
        }
    }
    for (int d = 32; d >= 1; d >>= 1) {                  // the groups are back together
        const int o = __shfl_xor(longest, d, 64);
        longest = o > longest ? o : longest;
    }
    if ((tid & 63) == 0) max_s[tid >> 6] = longest;
    __syncthreads();
    if (tid == 0) {
        int m = max_s[0];
        for (int k = 1; k < kSceneThreads / 64; ++k) m = max_s[k] > m ? max_s[k] : m;
        p.part_max[blockIdx.x] = m;
    }
}

__global__ __launch_bounds__(kSceneThreads) void grid_voxel_kernel(const GridArgs p)
{
    grid_voxel_body<false>(p, GridRoomsView{nullptr, nullptr, nullptr, 0});
}

// mode 0: out[v][k] = (((x[m_0] + x[m_1]) + ...) ) / float(n), a thread per (voxel, channel); the threads of a voxel's
// channels read a member's row together.  The loads of eight members are issued before their additions.
__global__ __launch_bounds__(kSceneThreads) void grid_mean_kernel(const GridArgs p)
{
    const GridHeader h = *p.hdr;
    const unsigned long long *sorted = (h.passes & 1) ? p.pairs_b : p.pairs_a;
    const long long K = p.K, total = (long long)p.max_voxels * K;
    const unsigned long long mask = (1ull << kGridRowBits) - 1ull;
    for (long long w = (long long)blockIdx.x * kSceneThreads + threadIdx.x; w < total; w += (long long)gridDim.x * kSceneThreads) {
        const int v = (int)(w / K), k = (int)(w - (long long)v * K);
        if (v >= h.emitted) {
            p.out[w] = 0.0f;
            continue;
        }
        const int s0 = p.start[v], n = p.start[v + 1] - s0;
        float acc = p.data[(size_t)(sorted[s0] & mask) * K + k];
        int j = 1;
        for (; j + 8 <= n; j += 8) {
            float x[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) x[u] = p.data[(size_t)(sorted[s0 + j + u] & mask) * K + k];
#pragma unroll
            for (int u = 0; u < 8; ++u) acc = acc + x[u];
        }
        for (; j < n; ++j) acc = acc + p.data[(size_t)(sorted[s0 + j] & mask) * K + k];
        p.out[w] = acc / (float)n;
    }
}

__global__ __launch_bounds__(kGridScanThreads) void grid_stats_kernel(const GridArgs p)
{
    __shared__ int red_s[kGridScanThreads / 64];
    const int tid = threadIdx.x;
    int m = 0;
    for (int b = tid; b < p.voxel_grid; b += kGridScanThreads) m = p.part_max[b] > m ? p.part_max[b] : m;
    for (int d = 32; d >= 1; d >>= 1) {
        const int o = __shfl_xor(m, d, 64);
        m = o > m ? o : m;
    }
    if ((tid & 63) == 0) red_s[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < kGridScanThreads / 64; ++k) m = red_s[k] > m ? red_s[k] : m;
        const GridHeader h = *p.hdr;
        p.stats[0] = h.emitted;
        p.stats[1] = h.occupied;
        p.stats[2] = h.n[0];
        p.stats[3] = h.n[1];
        p.stats[4] = h.n[2];
        p.stats[5] = h.nonfinite;
        p.stats[6] = m;
        p.stats[7] = h.error;
    }
}

__global__ __launch_bounds__(kSceneThreads) void grid_project_kernel(const int32_t *voxel_labels, const int32_t *inverse,
                                                                     long long N, long long M, int32_t *out)
{
    for (long long i = (long long)blockIdx.x * kSceneThreads + threadIdx.x; i < N; i += (long long)gridDim.x * kSceneThreads) {
        const int v = inverse[i];
        out[i] = (v >= 0 && (long long)v < M) ? voxel_labels[v] : -1;
    }
}

}  // namespace conv3p
