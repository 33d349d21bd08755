// conv3p_scene_rooms.hpp -- many rooms to model-sized blocks in one call (conv3p_scene_blocks_rooms_f32).
//
// The result is the concatenation of the single-room calls of conv3p_scene.hpp / conv3p_scene_cover.hpp (include/conv3p.h
// defines it; tests/scene_rooms_ref.py restates it on the single-room references).  What differs is how the member lists
// are built: the single-room fill tests every row against every emitted block's cell; here every row writes its (global
// cell id, global row) pairs in row order and a stable least-significant-digit radix sort groups them by cell, so the
// work is proportional to the pairs (<= 9 a row) and a list of any length comes out in ascending row.  A room's cells
// are numbered cell_base[r] + c, cell_base the prefix of the rooms' cell counts; everything behind the per-room frame
// is a pass over all rooms' rows, pairs, cells or blocks.  The launches, all on one stream, their number fixed:
//
//   rooms_check_kernel        one workgroup: room_start well formed?  Everything behind trusts it only if so
//   rooms_bounds_kernel       a workgroup per tile of 1024 global rows; per room that meets the tile one record {min, max
//                             of x, y, z over the finite rows, other rows} at record tile + room -- distinct for distinct
//                             (tile, room), and a room's records are consecutive
//   rooms_finish_kernel       a workgroup per room: its records in record order -> lo, lim, nbx, nby, cells, error
//   rooms_base_kernel         one workgroup: cell_base = prefix of the rooms' cells; the sum's limit; the flags
//   rooms_pairs_kernel<0>     tile of 1024 rows: the rows' member cells by scene_axis_mask's comparisons, counted
//   rooms_tile_scan_kernel    one workgroup: prefix of the tiles' pair counts -> M pairs, T sort tiles
//   rooms_pairs_kernel<1>     the same rows again: the pairs, in row order, behind the tile's prefix
//   3 x { rooms_sort_hist_kernel     per sort tile of 4096 pairs a histogram of 7 bits of the cell id (radix_hist_tile)
//         rooms_sort_scan_kernel     one workgroup: prefix over (digit, tile), the whole histogram as one array
//                                    (wg_exscan_inplace; no totals per digit, unlike the grid's and the adjacency's scan)
//         rooms_sort_scatter_kernel  one WAVE per sort tile, 64 pairs a step in order (radix_scatter_tile): the lanes of
//                                    equal digit from seven ballots, rank = popcount below the lane, a running offset per
//                                    digit in LDS; a pair's destination depends on nothing but the input order, so the
//                                    sort is stable }
//   rooms_segments_kernel     sorted pairs: where the cell id changes, a list starts / ends -> count and offset per cell
//   rooms_plan_kernel         one workgroup: all rooms' cells in order -> kept rank, first block number (scan over the
//                             parts), the listed cells, and the prefixes at the rooms' boundaries
//   rooms_table_kernel        a lane per emitted block: binary searches -> {cell, list start + a_j, n_j, j P}, room
//   rooms_stats_kernel        a lane per room: room_blocks, room_stats; stats
//   rooms_emit_kernel         a workgroup per block, as scene_emit_body; the draws keyed seed + room, rows global
//
// No float atomics (the only atomics are the histogram's LDS integer adds and the check's one LDS atomicOr); every output
// word is written once by a plain
// store; the result does not depend on the launch geometry.  The scans, the radix pass, the bounding-box records and the
// room_start check are conv3p_workgroup.hpp's.
#pragma once

#include "conv3p_scene_cover.hpp"

namespace conv3p {

constexpr int kRoomsMaxRooms = 65536;
constexpr long long kRoomsMaxN = 1ll << 26;
constexpr int kRoomsMaxCells = 1 << 20;         // CONV3P_SCENE_ROOMS_MAX_CELLS
constexpr int kRoomsRowTile = 1024;             // rows of a workgroup of the bounds and pairs kernels: 4 a thread
constexpr int kRoomsSortTile = 4096;            // pairs of a sort tile
constexpr int kRoomsDigitBits = 7;
constexpr int kRoomsDigits = 1 << kRoomsDigitBits;
constexpr int kRoomsPasses = 3;                 // 3 x 7 bits >= the 20 bits of a cell id
constexpr int kRoomsScanThreads = 1024;

struct RoomsHeader {
    int bad;                           // room_start malformed
    int flags;                         // stats[7]
    int cells;                         // cells of all rooms (0 when nothing may be emitted)
    int cells_stat;                    // stats[3]
    int nonfinite;                     // stats[4]
    int pairs, sort_tiles;             // M, T = ceil(M / kRoomsSortTile)
    int listed, ne;                    // listed cells, emitted blocks
};

struct RoomFrame {
    float lo[3], lim[3];
    int nbx, nby, ncells, nonfinite, error, pad;
};

struct RoomsArgs {
    const float *data;                 // (N, K)
    const void *labels;                // (N), label_bytes each; may be NULL
    const int32_t *room_start;         // (R + 1)
    int N, R, K, label_bytes, P, min_points, max_blocks, cover;
    float block, stride;
    unsigned seed_lo, seed_hi, step_lo, step_hi;
    float *blocks_out;                 // (max_blocks, P, K + 3)
    int32_t *labels_out, *index_out;   // (max_blocks, P); labels_out may be NULL
    int32_t *block_cell, *block_count, *block_room;   // (max_blocks)
    int32_t *room_blocks, *room_stats, *stats;        // (R + 1), (R, 8), (8)
    // the workspace
    RoomsHeader *hdr;
    RoomFrame *room;                   // (R)
    int *cell_base;                    // (R + 1)
    int4 *room_pref;                   // (R + 1): {kept, small, parts} summed over the cells before the room's
    float *records;                    // (row tiles + R, 8)
    int *tile_pairs;                   // (row tiles)
    int *seg_start, *seg_end;          // (kRoomsMaxCells)
    int *blk_cell, *blk_count, *blk_off, *blk_first;   // (listed_max)
    int4 *table;                       // (max_blocks)
    int *blk_room;                     // (max_blocks)
    int *hist;                         // (kRoomsDigits, sort tiles)
    unsigned long long *pairs_a, *pairs_b;             // (pairs_max): cell id << 32 | global row
    int row_tiles, listed_max, pairs_max;
};

// The room of global row i: the last r with room_start[r] <= i (so never an empty room); -1 before the first room, R
// behind the last.  Terminates and stays inside room_start[0..R] whatever it holds.
__device__ __forceinline__ int rooms_find(const int32_t *start, int R, int i)
{
    return lower_bound(0, R + 1, [&](int m) { return start[m] <= i; }) - 1;      // the number of entries <= i
}

__global__ __launch_bounds__(kRoomsScanThreads) void rooms_check_kernel(const RoomsArgs p)
{
    __shared__ int bad_s;
    const int bad = room_start_bad(p.room_start, p.R, p.N, kSceneMaxN, &bad_s, threadIdx.x, kRoomsScanThreads);
    if (threadIdx.x == 0) p.hdr->bad = bad;
}

__global__ __launch_bounds__(kSceneThreads) void rooms_bounds_kernel(const RoomsArgs p)
{
    __shared__ float red[(kSceneThreads / 64) * 7];
    if (p.hdr->bad) return;
    const int tid = threadIdx.x, tile = blockIdx.x;
    const int t0 = tile * kRoomsRowTile, t1 = t0 + kRoomsRowTile < p.N ? t0 + kRoomsRowTile : p.N;
    float x[4], y[4], z[4];
    for (int k = 0; k < 4; ++k) {
        const int i = t0 + tid + k * kSceneThreads;
        x[k] = y[k] = z[k] = 0.0f;
        if (i < t1) {
            const float *v = p.data + (size_t)i * p.K;
            x[k] = v[0]; y[k] = v[1]; z[k] = v[2];
        }
    }
    int r0 = rooms_find(p.room_start, p.R, t0), r1 = rooms_find(p.room_start, p.R, t1 - 1);
    if (r0 < 0) r0 = 0;
    if (r1 > p.R - 1) r1 = p.R - 1;
    for (int r = r0; r <= r1; ++r) {                     // uniform over the workgroup
        const int ra = p.room_start[r], rb = p.room_start[r + 1];
        const int a = ra > t0 ? ra : t0, b = rb < t1 ? rb : t1;
        if (a >= b) continue;
        SceneRange g;
        range_init(g);
        for (int k = 0; k < 4; ++k) {
            const int i = t0 + tid + k * kSceneThreads;
            if (i >= a && i < b) range_add(g, x[k], y[k], z[k]);
        }
        g = scene_reduce(g, red, tid, kSceneThreads);
        if (tid == 0) {
            float *w = p.records + (size_t)(tile + r) * 8;
            range_store(g, w);
            w[7] = 0.0f;
        }
    }
}

__global__ __launch_bounds__(kSceneThreads) void rooms_finish_kernel(const RoomsArgs p)
{
    __shared__ float red[(kSceneThreads / 64) * 7];
    const int tid = threadIdx.x;
    const bool bad = p.hdr->bad != 0;
    for (int r = blockIdx.x; r < p.R; r += gridDim.x) {
        const int a = bad ? 0 : p.room_start[r], b = bad ? 0 : p.room_start[r + 1];
        SceneRange g;
        range_init(g);
        if (b > a) {
            const int ta = a / kRoomsRowTile, tb = (b - 1) / kRoomsRowTile;
            for (int t = ta + tid; t <= tb; t += kSceneThreads) range_fold(g, p.records + (size_t)(t + r) * 8);
        }
        g = scene_reduce(g, red, tid, kSceneThreads);
        if (tid == 0) {
            RoomFrame h;
            const bool any = g.bad < b - a;
            for (int e = 0; e < 3; ++e) {
                // a zero minimum has the sign the single-room call gives it, whatever the order (see SceneRange)
                h.lo[e] = any ? g.lo[e] : 0.0f;
                h.lim[e] = any ? g.hi[e] - g.lo[e] : 0.0f;
            }
            h.nbx = any ? scene_cells_along(h.lim[0], p.block, p.stride) : 0;
            h.nby = any ? scene_cells_along(h.lim[1], p.block, p.stride) : 0;
            const long long cells = (long long)h.nbx * h.nby;
            h.error = cells > kSceneMaxCells ? 1 : 0;
            h.ncells = h.error ? 0 : (int)cells;
            h.nonfinite = g.bad;
            h.pad = 0;
            p.room[r] = h;
        }
    }
}

__global__ __launch_bounds__(kRoomsScanThreads) void rooms_base_kernel(const RoomsArgs p)
{
    __shared__ long long scan_s[kRoomsScanThreads / 64];
    const int tid = threadIdx.x;
    int r0, r1;
    wg_chunk(p.R, kRoomsScanThreads, tid, &r0, &r1);
    long long cells = 0, bad_rows = 0, errors = 0;
    for (int r = r0; r < r1; ++r) {
        cells += p.room[r].ncells;
        bad_rows += p.room[r].nonfinite;
        errors += p.room[r].error;
    }
    long long cells_all, bad_all, err_all;
    long long base = wg_exscan(cells, scan_s, tid, kRoomsScanThreads, &cells_all);
    (void)wg_exscan(bad_rows, scan_s, tid, kRoomsScanThreads, &bad_all);
    (void)wg_exscan(errors, scan_s, tid, kRoomsScanThreads, &err_all);
    const bool over = cells_all > (long long)kRoomsMaxCells;
    for (int r = r0; r < r1; ++r) {
        p.cell_base[r] = over ? 0 : (int)base;
        base += p.room[r].ncells;
        if (over) p.room[r].ncells = 0;                  // no row of any room has a member cell then
    }
    if (tid == 0) {
        RoomsHeader *h = p.hdr;
        p.cell_base[p.R] = over ? 0 : (int)cells_all;
        h->flags = (err_all ? 1 : 0) | (h->bad ? 2 : 0) | (over ? 4 : 0);
        h->cells = over ? 0 : (int)cells_all;
        h->cells_stat = cells_all > 2147483647ll ? 2147483647 : (int)cells_all;
        h->nonfinite = (int)bad_all;
        h->pairs = 0;
        h->sort_tiles = 0;
        h->listed = 0;
        h->ne = 0;
    }
}

// The member cells of global row i: the masks of scene_axis_mask over its room's frame; false for a row of no room, a
// non-finite row, a room without cells.  base = the room's first global cell id.
struct RoomsRow { unsigned mx, my; int i0, j0, nby, base; };

__device__ __forceinline__ bool rooms_row(const RoomsArgs &p, int i, RoomsRow *o)
{
    const int r = rooms_find(p.room_start, p.R, i);
    if (r < 0 || r >= p.R) return false;
    const RoomFrame *f = p.room + r;
    if (f->ncells == 0) return false;
    const float *v = p.data + (size_t)i * p.K;
    const float x = v[0], y = v[1], z = v[2];
    if (!scene_finite(x, y, z)) return false;
    o->nby = f->nby;
    o->base = p.cell_base[r];
    o->mx = scene_axis_mask(x - f->lo[0], p.block, p.stride, f->nbx, &o->i0);
    o->my = scene_axis_mask(y - f->lo[1], p.block, p.stride, f->nby, &o->j0);
    return true;
}

// kWrite = false: the tile's number of pairs (and the segment tables zeroed).  kWrite = true: the pairs.  A thread
// takes 4 consecutive rows, so thread order is row order.
template <bool kWrite> __global__ __launch_bounds__(kSceneThreads) void rooms_pairs_kernel(const RoomsArgs p)
{
    __shared__ int scan_s[kSceneThreads / 64];
    const int tid = threadIdx.x, tile = blockIdx.x;
    const RoomsHeader h = *p.hdr;
    if (!kWrite) {
        for (int g = tile * kSceneThreads + tid; g < h.cells; g += (int)gridDim.x * kSceneThreads) {
            p.seg_start[g] = 0;
            p.seg_end[g] = 0;
        }
    }
    const int t0 = tile * kRoomsRowTile, t1 = t0 + kRoomsRowTile < p.N ? t0 + kRoomsRowTile : p.N;
    RoomsRow row[4];
    int n = 0;
    for (int k = 0; k < 4; ++k) {
        const int i = t0 + 4 * tid + k;
        row[k].mx = row[k].my = 0;
        if (i < t1 && !h.bad && rooms_row(p, i, &row[k])) n += __popc(row[k].mx) * __popc(row[k].my);
        else row[k].mx = 0;
    }
    int total;
    int pos = wg_exscan(n, scan_s, tid, kSceneThreads, &total);
    if (!kWrite) {
        if (tid == 0) p.tile_pairs[tile] = total;
        return;
    }
    pos += p.tile_pairs[tile];
    for (int k = 0; k < 4; ++k) {
        if (!row[k].mx) continue;
        const unsigned long long i = (unsigned long long)(t0 + 4 * tid + k);
        for (int di = 0; di < 4; ++di) {
            if (!((row[k].mx >> di) & 1u)) continue;
            for (int dj = 0; dj < 4; ++dj) {
                if (!((row[k].my >> dj) & 1u)) continue;
                const int g = row[k].base + (row[k].i0 + di) * row[k].nby + (row[k].j0 + dj);
                if (pos < p.pairs_max) p.pairs_a[pos] = ((unsigned long long)g << 32) | i;   // else: the tile scan set bit 3
                ++pos;
            }
        }
    }
}

__global__ __launch_bounds__(kRoomsScanThreads) void rooms_tile_scan_kernel(const RoomsArgs p)
{
    __shared__ int scan_s[kRoomsScanThreads / 64];
    const int tid = threadIdx.x;
    const int total = wg_exscan_inplace(p.tile_pairs, p.row_tiles, scan_s, tid, kRoomsScanThreads);
    if (tid == 0) {
        // a row is in at most m x m cells, so total <= pairs_max; should the comparisons ever say otherwise the pairs
        // past the buffers are dropped and stats[7] says so (bit 3) instead of a result that is silently short
        const int pairs = total < p.pairs_max ? total : p.pairs_max;
        if (total > p.pairs_max) p.hdr->flags |= 8;
        p.hdr->pairs = pairs;
        p.hdr->sort_tiles = (pairs + kRoomsSortTile - 1) / kRoomsSortTile;
    }
}

// ------------------------------------------------------------------------------------------ the radix sort's pass
__global__ __launch_bounds__(kSceneThreads) void rooms_sort_hist_kernel(const RoomsArgs p, const unsigned long long *src,
                                                                        int shift)
{
    __shared__ int hist_s[kRoomsDigits];
    const int M = p.hdr->pairs, T = p.hdr->sort_tiles;
    for (int tile = blockIdx.x; tile < T; tile += gridDim.x)
        (void)radix_hist_tile<kRoomsDigitBits>(src, M, tile, kRoomsSortTile, 32 + shift, hist_s, p.hist, T, threadIdx.x,
                                               kSceneThreads);
}

__global__ __launch_bounds__(kRoomsScanThreads) void rooms_sort_scan_kernel(const RoomsArgs p)
{
    __shared__ int scan_s[kRoomsScanThreads / 64];
    (void)wg_exscan_inplace(p.hist, (long long)p.hdr->sort_tiles * kRoomsDigits, scan_s, threadIdx.x, kRoomsScanThreads);
}

__global__ __launch_bounds__(64) void rooms_sort_scatter_kernel(const RoomsArgs p, const unsigned long long *src,
                                                                unsigned long long *dst, int shift)
{
    __shared__ int run_s[kRoomsDigits];
    const int M = p.hdr->pairs, T = p.hdr->sort_tiles;
    for (int tile = blockIdx.x; tile < T; tile += gridDim.x)
        radix_scatter_tile<kRoomsDigitBits, int>(src, dst, M, tile, kRoomsSortTile, 32 + shift, p.hist, T, run_s, threadIdx.x);
}

__global__ __launch_bounds__(kSceneThreads) void rooms_segments_kernel(const RoomsArgs p, const unsigned long long *sorted)
{
    const int M = p.hdr->pairs;
    for (long long w = (long long)blockIdx.x * kSceneThreads + threadIdx.x; w < M; w += (long long)gridDim.x * kSceneThreads) {
        const int i = (int)w;
        const int g = (int)(sorted[i] >> 32);
        if (i == 0 || (int)(sorted[i - 1] >> 32) != g) p.seg_start[g] = i;
        if (i == M - 1 || (int)(sorted[i + 1] >> 32) != g) p.seg_end[g] = i + 1;
    }
}

// All rooms' cells in (room, cell) order.  The block numbers of a room's cells are the single call's behind the blocks
// the earlier rooms need, so one scan and one comparison with max_blocks give every room its cut.
__global__ __launch_bounds__(kRoomsScanThreads) void rooms_plan_kernel(const RoomsArgs p)
{
    __shared__ int scan_s[kRoomsScanThreads / 64];
    const int tid = threadIdx.x, P = p.P, R = p.R;
    const int cells = p.hdr->cells;
    const int need = p.min_points < 1 ? 1 : p.min_points;
    int c0, c1;
    wg_chunk(cells, kRoomsScanThreads, tid, &c0, &c1);
    int kept = 0, small = 0, parts = 0, listed = 0;
    for (int g = c0; g < c1; ++g) {
        const int n = p.seg_end[g] - p.seg_start[g];
        kept += n >= need ? 1 : 0;
        small += (n > 0 && n < need) ? 1 : 0;
        parts += n >= need ? (p.cover ? (n + P - 1) / P : 1) : 0;
    }
    int kept_all, small_all, parts_all, listed_all;
    const int kbase = wg_exscan(kept, scan_s, tid, kRoomsScanThreads, &kept_all);
    const int sbase = wg_exscan(small, scan_s, tid, kRoomsScanThreads, &small_all);
    const int pbase = wg_exscan(parts, scan_s, tid, kRoomsScanThreads, &parts_all);
    int k = kbase, sm = sbase, first = pbase;
    int rp = 0;                                          // the first room whose cell_base is >= c0
    if (c0 < c1) rp = lower_bound(0, R + 1, [&](int m) { return p.cell_base[m] < c0; });
    for (int g = c0; g < c1; ++g) {
        while (rp <= R && p.cell_base[rp] == g) p.room_pref[rp++] = make_int4(k, sm, first, 0);
        const int n = p.seg_end[g] - p.seg_start[g];
        if (n > 0 && n < need) ++sm;
        if (n < need) continue;
        if (first < p.max_blocks && k < p.listed_max) {  // k < listed_max holds: k <= first
            p.blk_cell[k] = g;
            p.blk_count[k] = n;
            p.blk_off[k] = p.seg_start[g];
            p.blk_first[k] = first;
            ++listed;
        }
        ++k;
        first += p.cover ? (n + P - 1) / P : 1;
    }
    (void)wg_exscan(listed, scan_s, tid, kRoomsScanThreads, &listed_all);
    for (int r = tid; r <= R; r += kRoomsScanThreads)    // the rooms behind the last cell
        if (p.cell_base[r] == cells) p.room_pref[r] = make_int4(kept_all, small_all, parts_all, 0);
    if (tid == 0) {
        p.hdr->listed = listed_all;
        p.hdr->ne = parts_all < p.max_blocks ? parts_all : p.max_blocks;
    }
}

__global__ __launch_bounds__(kSceneThreads) void rooms_table_kernel(const RoomsArgs p)
{
    const int ne = p.hdr->ne, listed = p.hdr->listed;
    for (long long w = (long long)blockIdx.x * kSceneThreads + threadIdx.x; w < ne; w += (long long)gridDim.x * kSceneThreads) {
        const int b = (int)w;
        int lo = 0, hi = listed - 1;                     // the last listed cell whose first block is <= b
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (p.blk_first[mid] <= b) lo = mid; else hi = mid - 1;
        }
        const int n = p.blk_count[lo], j = b - p.blk_first[lo], q = p.cover ? (n + p.P - 1) / p.P : 1;
        const int a0 = (int)((long long)j * n / q), a1 = (int)((long long)(j + 1) * n / q);
        const int g = p.blk_cell[lo];
        p.table[b] = make_int4(g, p.blk_off[lo] + a0, a1 - a0, j * p.P);
        int rl = 0, rh = p.R - 1;                        // the last room whose cell_base is <= g: the one with cells
        while (rl < rh) {
            const int mid = (rl + rh + 1) >> 1;
            if (p.cell_base[mid] <= g) rl = mid; else rh = mid - 1;
        }
        p.blk_room[b] = rl;
    }
}

__global__ __launch_bounds__(kSceneThreads) void rooms_stats_kernel(const RoomsArgs p)
{
    const RoomsHeader h = *p.hdr;
    const int mb = p.max_blocks;
    for (int r = blockIdx.x * kSceneThreads + threadIdx.x; r <= p.R; r += (int)gridDim.x * kSceneThreads) {
        const int4 a = p.room_pref[r];
        const int before = a.z < mb ? a.z : mb;
        p.room_blocks[r] = before;
        if (r == p.R) {
            p.stats[0] = before;
            p.stats[1] = a.x;
            p.stats[2] = p.R;
            p.stats[3] = h.cells_stat;
            p.stats[4] = h.nonfinite;
            p.stats[5] = a.y;
            p.stats[6] = p.cover ? a.z : 0;
            p.stats[7] = h.flags;
            continue;
        }
        const int4 e = p.room_pref[r + 1];
        const RoomFrame f = p.room[r];
        int32_t *s = p.room_stats + (size_t)r * 8;
        s[0] = (e.z < mb ? e.z : mb) - before;
        s[1] = e.x - a.x;
        s[2] = f.nbx;
        s[3] = f.nby;
        s[4] = f.nonfinite;
        s[5] = e.y - a.y;
        s[6] = p.cover ? e.z - a.z : 0;
        s[7] = f.error;
    }
}

// scene_emit_body over the table: the block's room gives the frame and the key seed + room; the lists hold global rows.
__global__ __launch_bounds__(kSceneThreads) void rooms_emit_kernel(const RoomsArgs p)
{
    __shared__ float xyz_s[kSceneThreads * 3], nrm_s[kSceneThreads * 3];
    __shared__ int row_s[kSceneThreads];
    __shared__ float min_s[(kSceneThreads / 64) * 2];
    const int ne = p.hdr->ne;
    const unsigned long long *pairs = p.pairs_b;         // three passes: a -> b -> a -> b
    const int tid = threadIdx.x, P = p.P, K = p.K, K3 = p.K + 3;
    for (int b = blockIdx.x; b < p.max_blocks; b += gridDim.x) {
        float *out = p.blocks_out + (size_t)b * P * K3;
        int32_t *idx = p.index_out + (size_t)b * P;
        int32_t *lab = p.labels_out ? p.labels_out + (size_t)b * P : nullptr;
        if (b >= ne) {                                   // the filler
            for (size_t e = tid; e < (size_t)P * K3; e += kSceneThreads) out[e] = 0.0f;
            for (int t = tid; t < P; t += kSceneThreads) {
                idx[t] = -1;
                if (lab) lab[t] = -1;
            }
            if (tid == 0) {
                p.block_cell[b] = -1;
                p.block_count[b] = 0;
                p.block_room[b] = -1;
            }
            continue;
        }
        const int4 e = p.table[b];
        const int r = p.blk_room[b];
        const int c = e.x - p.cell_base[r], off = e.y, n = e.z;
        const unsigned base = (unsigned)e.w;
        const RoomFrame *f = p.room + r;
        const float lox = f->lo[0], loy = f->lo[1], loz = f->lo[2];
        const float limx = f->lim[0], limy = f->lim[1], limz = f->lim[2];
        const unsigned long long seed = (((unsigned long long)p.seed_hi << 32) | p.seed_lo) + (unsigned long long)r;
        const unsigned seed_lo = (unsigned)seed, seed_hi = (unsigned)(seed >> 32);
        if (tid == 0) {
            p.block_cell[b] = c;
            p.block_count[b] = n;
            p.block_room[b] = r;
        }
        float mnx = INFINITY, mny = INFINITY;
        for (int t = tid; t < P; t += kSceneThreads) {
            int m = t;
            if ((!p.cover && n > P) || t >= n) {
                const Philox4 w = philox4x32_10(base + (unsigned)t, 0x80000000u | (unsigned)c, p.step_lo, p.step_hi, seed_lo,
                                                seed_hi);
                m = (int)(((unsigned long long)w.w[0] * (unsigned long long)n) >> 32);
            }
            const int row = (int)(unsigned)pairs[off + m];   // inside the cell's list; the low word is the global row
            idx[t] = row;
            if (lab) lab[t] = row_label(p.labels, p.label_bytes, (size_t)row);
            const float *v = p.data + (size_t)row * K;
            mnx = fminf(mnx, v[0] - lox);
            mny = fminf(mny, v[1] - loy);
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
                const float sx = v[0] - lox, sy = v[1] - loy, sz = v[2] - loz;
                row_s[tid] = row;
                xyz_s[3 * tid] = sx - cx;
                xyz_s[3 * tid + 1] = sy - cy;
                xyz_s[3 * tid + 2] = sz;
                nrm_s[3 * tid] = limx == 0.0f ? 0.0f : sx / limx;
                nrm_s[3 * tid + 1] = limy == 0.0f ? 0.0f : sy / limy;
                nrm_s[3 * tid + 2] = limz == 0.0f ? 0.0f : sz / limz;
            }
            __syncthreads();
            const int cnt = P - t0 < kSceneThreads ? P - t0 : kSceneThreads;
            float *dst = out + (size_t)t0 * K3;
            for (int q = tid; q < cnt * K3; q += kSceneThreads) {
                const int rr = q / K3, ch = q - rr * K3;
                dst[q] = ch < 3 ? xyz_s[3 * rr + ch] : (ch < K ? p.data[(size_t)row_s[rr] * K + ch] : nrm_s[3 * rr + ch - K]);
            }
            __syncthreads();
        }
    }
}

}  // namespace conv3p
