// conv3p_grid_rooms.hpp -- voxel-grid subsampling of many clouds in one call (conv3p_grid_subsample_rooms_f32).
//
// The result is the concatenation of the single-cloud calls of conv3p_grid.hpp (include/conv3p.h defines it;
// tests/grid_rooms_ref.py restates it on the single-cloud reference).  The shape is that of conv3p_scene_rooms.hpp laid on
// the lattice of conv3p_grid.hpp: every room has its own frame (lo, n_x, n_y, n_z), a room's cells are numbered
// cell_base[r] + c, cell_base the 64-bit prefix of the rooms' cell counts, and every finite row of a room with cells
// writes one pair (cell_base[r] + c) << 24 | global row in row order.  One stable radix sort over all rooms' pairs then
// gives the voxels room after room, in ascending cell within a room, their members in ascending row -- the sort, the
// heads and the mean are conv3p_grid.hpp's kernels, launched on a GridArgs that points at this call's workspace.  The
// launches, all on one stream, 28 in mode 0 and 27 in mode 1 whatever R, the rooms' sizes and the data:
//
//   grid_rooms_check_kernel      one workgroup: room_start well formed?  Everything behind trusts it only if so
//   grid_rooms_bounds_kernel     a workgroup per tile of 1024 global rows; per room that meets the tile one record {min,
//                                max of x, y, z over the finite rows, other rows} at record tile + room (the numbering
//                                of rooms_bounds_kernel): distinct for distinct (tile, room), a room's records consecutive
//   grid_rooms_frame_kernel      a workgroup per room: its records -> lo, n, cells, the error, the finite rows; and into
//                                word 7 of every record the room's finite rows in the tiles before it
//   grid_rooms_base_kernel       one workgroup: cell_base (64-bit) and pair_base, the prefixes of the rooms' cells and
//                                pairs; the sum's limit; M pairs, T sort tiles, the passes the GLOBAL cell ids need
//   grid_rooms_pairs_kernel      the row tiles again: a row's room by rooms_find, its pair at pair_base[r] + the record's
//                                word 7 + its rank among the room's pairs of the tile; inverse = -1 for a row without one
//   5 x { grid_sort_hist_kernel, grid_sort_scan_kernel, grid_sort_scatter_kernel }       conv3p_grid.hpp's, unchanged
//   grid_heads_kernel<0>, grid_heads_scan_kernel, grid_heads_kernel<1>                   conv3p_grid.hpp's, unchanged
//   grid_rooms_voxel_kernel      grid_voxel_body<true>: the voxel's room by binary search in cell_base, the cell decoded
//                                with the room's n, the centre's s formed with the room's lo; voxel_room
//   grid_mean_kernel             (mean only) conv3p_grid.hpp's, unchanged: the rows of a list are global
//   grid_rooms_count_max_kernel  per tile of 1024 voxels the largest member count
//   grid_rooms_out_kernel        a wave per room: its voxel range from the voxel numbers at its cell_base boundaries,
//                                the largest count over it (whole tiles by their maxima) -> voxel_start, room_stats
//   grid_rooms_stats_kernel      one workgroup over room_stats: stats, written last
//
// No float atomics (the only atomics are the sort's integer adds and the check's one LDS atomicOr); every output word is
// written once by a plain store; the result does not depend on the launch geometry.
#pragma once

#include "conv3p_grid.hpp"

namespace conv3p {

constexpr int kGridRoomsMaxRooms = 65536;
constexpr int kGridCountTile = 1024;            // voxels of a workgroup of grid_rooms_count_max_kernel: 4 a thread

struct GridRoomsHeader {
    int bad;                           // room_start malformed
    int flags;                         // stats[7]
    int errors;                        // rooms with an error of their own
    int pad;
};

struct GridRoomsArgs {
    GridArgs g;                        // the single call's arguments and workspace words; data, labels, inverse by global
                                       // row; records (row tiles + R, 8); tile_off is not used
    const int32_t *room_start;         // (R + 1)
    int R;
    int32_t *voxel_room, *voxel_start, *room_stats;    // (max_voxels), (R + 1), (R, 8)
    // the workspace
    GridRoomsHeader *xh;
    GridRoomFrame *room;               // (R)
    long long *cell_base;              // (R + 1)
    int *pair_base;                    // (R + 1)
    int *tile_max;                     // (row tiles): voxels <= rows
};

__global__ __launch_bounds__(kGridScanThreads) void grid_rooms_check_kernel(const GridRoomsArgs p)
{
    __shared__ int bad_s;
    // no limit on a room's rows of its own: a well-formed room has at most N
    const int bad = room_start_bad(p.room_start, p.R, p.g.N, 0x7fffffffffffffffll, &bad_s, threadIdx.x, kGridScanThreads);
    if (threadIdx.x == 0) p.xh->bad = bad;
}

__global__ __launch_bounds__(kSceneThreads) void grid_rooms_bounds_kernel(const GridRoomsArgs p)
{
    __shared__ float red[(kSceneThreads / 64) * 7];
    if (p.xh->bad) return;
    const int tid = threadIdx.x, tile = blockIdx.x, N = p.g.N;
    const int t0 = tile * kGridRowTile, t1 = t0 + kGridRowTile < N ? t0 + kGridRowTile : N;
    float x[4], y[4], z[4];
    for (int k = 0; k < 4; ++k) {
        const int i = t0 + tid + k * kSceneThreads;
        x[k] = y[k] = z[k] = 0.0f;
        if (i < t1) {
            const float *v = p.g.data + (size_t)i * p.g.K;
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
        // tile + r < row tiles + R.  Word 7 stays unwritten: grid_rooms_frame_kernel writes it
        if (tid == 0) range_store(g, p.g.records + (size_t)(tile + r) * 8);
    }
}

// A room's frame is grid_frame_kernel's on the room's own rows.  Word 7 of record (t, r) becomes the finite rows of room
// r in the tiles before t, which places the room's pairs of tile t behind pair_base[r].
__global__ __launch_bounds__(kSceneThreads) void grid_rooms_frame_kernel(const GridRoomsArgs p)
{
    __shared__ float red[(kSceneThreads / 64) * 7];
    __shared__ int scan_s[kSceneThreads / 64];
    const int tid = threadIdx.x;
    const bool bad = p.xh->bad != 0;
    for (int r = blockIdx.x; r < p.R; r += gridDim.x) {
        const int a = bad ? 0 : p.room_start[r], b = bad ? 0 : p.room_start[r + 1];
        const int ta = a / kGridRowTile, tb = b > a ? (b - 1) / kGridRowTile : ta - 1;
        SceneRange g;
        range_init(g);
        for (int t = ta + tid; t <= tb; t += kSceneThreads) range_fold(g, p.g.records + (size_t)(t + r) * 8);
        g = scene_reduce(g, red, tid, kSceneThreads);
        int run = 0;
        for (int c0 = ta; c0 <= tb; c0 += kSceneThreads) {       // uniform over the workgroup
            const int t = c0 + tid;
            int fin = 0;
            float *w = p.g.records + (size_t)(t + r) * 8;
            if (t <= tb) {
                const int t0 = t * kGridRowTile, t1 = t0 + kGridRowTile;
                fin = ((b < t1 ? b : t1) - (a > t0 ? a : t0)) - __float_as_int(w[6]);
            }
            int total;
            const int before = wg_exscan(fin, scan_s, tid, kSceneThreads, &total);
            if (t <= tb) w[7] = __int_as_float(run + before);
            run += total;
        }
        if (tid == 0) {
            GridRoomFrame h;
            const bool any = g.bad < b - a;
            bool over = false;
            for (int e = 0; e < 3; ++e) {
                // as in grid_frame_kernel: a zero minimum has the single call's sign
                h.lo[e] = any ? g.lo[e] : 0.0f;
                h.n[e] = any ? grid_axis_cell(g.hi[e] - g.lo[e], p.g.voxel) + 1 : 0;
                if (h.n[e] > kGridMaxAxis) over = true;
            }
            long long cells = 0;
            if (any && !over) cells = (long long)h.n[0] * h.n[1] * h.n[2];   // <= 2^60
            if (cells > kGridMaxCells) over = true;
            h.error = over ? 1 : 0;
            h.cells = over ? 0 : cells;
            h.nonfinite = g.bad;
            h.pairs = over ? 0 : (b - a) - g.bad;
            h.pad = 0;
            p.room[r] = h;
        }
    }
}

__global__ __launch_bounds__(kGridScanThreads) void grid_rooms_base_kernel(const GridRoomsArgs p)
{
    __shared__ long long scan_s[kGridScanThreads / 64];
    __shared__ int scan_i[kGridScanThreads / 64];
    const int tid = threadIdx.x;
    int r0, r1;
    wg_chunk(p.R, kGridScanThreads, tid, &r0, &r1);
    for (int e = tid; e < kGridPasses * kGridDigits; e += kGridScanThreads) p.g.digit_total[e] = 0;
    long long cells = 0;
    int pairs = 0, bad_rows = 0, errors = 0;             // the rooms' rows, summed, are <= N <= 2^24
    for (int r = r0; r < r1; ++r) {
        cells += p.room[r].cells;                        // <= 2^40 each, R <= 2^16
        pairs += p.room[r].pairs;
        bad_rows += p.room[r].nonfinite;
        errors += p.room[r].error;
    }
    long long cells_all;
    int pairs_all, bad_all, err_all;
    long long cbase = wg_exscan(cells, scan_s, tid, kGridScanThreads, &cells_all);
    int pbase = wg_exscan(pairs, scan_i, tid, kGridScanThreads, &pairs_all);
    (void)wg_exscan(bad_rows, scan_i, tid, kGridScanThreads, &bad_all);
    (void)wg_exscan(errors, scan_i, tid, kGridScanThreads, &err_all);
    const bool over = cells_all > kGridMaxCells;         // a global cell id must fit the 40 bits of a pair
    for (int r = r0; r < r1; ++r) {
        p.cell_base[r] = over ? 0 : cbase;
        p.pair_base[r] = over ? 0 : pbase;               // <= the rooms' rows <= N
        cbase += p.room[r].cells;
        pbase += p.room[r].pairs;
        if (over) {                                      // no row of any room has a pair then
            p.room[r].cells = 0;
            p.room[r].pairs = 0;
        }
    }
    if (tid == 0) {
        p.cell_base[p.R] = over ? 0 : cells_all;
        p.pair_base[p.R] = over ? 0 : pairs_all;
        GridRoomsHeader *x = p.xh;
        x->flags = (err_all ? 1 : 0) | (x->bad ? 2 : 0) | (over ? 4 : 0);
        x->errors = err_all;
        x->pad = 0;
        GridHeader h;
        for (int e = 0; e < 3; ++e) {
            h.lo[e] = 0.0f;
            h.n[e] = 0;
        }
        h.cells = over ? 0 : cells_all;
        h.error = 0;
        h.nonfinite = bad_all;
        h.pairs = over ? 0 : pairs_all;
        h.sort_tiles = (h.pairs + kGridSortTile - 1) / kGridSortTile;
        const int bits = h.cells > 1 ? 64 - __clzll(h.cells - 1) : 0;
        h.passes = (bits + kGridDigitBits - 1) / kGridDigitBits;
        h.occupied = 0;
        h.emitted = 0;
        *p.g.hdr = h;
    }
}

// The pairs in global row order: a thread takes 4 consecutive rows.  rank_s[i - t0] = the tile's pairs before row i, so
// a row's rank among its room's pairs of the tile is the difference to the room's first row of the tile.
__global__ __launch_bounds__(kSceneThreads) void grid_rooms_pairs_kernel(const GridRoomsArgs p)
{
    __shared__ int scan_s[kSceneThreads / 64];
    __shared__ int rank_s[kGridRowTile];
    const int tid = threadIdx.x, tile = blockIdx.x, N = p.g.N;
    const int M = p.g.hdr->pairs;
    const bool bad = p.xh->bad != 0;
    const int t0 = tile * kGridRowTile, t1 = t0 + kGridRowTile < N ? t0 + kGridRowTile : N;
    unsigned long long key[4];
    int room[4];
    int n = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = t0 + 4 * tid + k;
        room[k] = -1;
        key[k] = 0ull;
        if (i >= t1) continue;
        if (!bad) {
            const int r = rooms_find(p.room_start, p.R, i);
            if (r >= 0 && r < p.R) {
                const GridRoomFrame *f = p.room + r;
                const float *v = p.g.data + (size_t)i * p.g.K;
                const float x = v[0], y = v[1], z = v[2];
                if (f->cells > 0 && scene_finite(x, y, z)) {
                    const long long ix = grid_axis_cell(x - f->lo[0], p.g.voxel), iy = grid_axis_cell(y - f->lo[1], p.g.voxel),
                                    iz = grid_axis_cell(z - f->lo[2], p.g.voxel);
                    const long long c = p.cell_base[r] + (ix * f->n[1] + iy) * f->n[2] + iz;   // < the rooms' cells <= 2^40
                    key[k] = ((unsigned long long)c << kGridRowBits) | (unsigned long long)i;
                    room[k] = r;
                    ++n;
                }
            }
        }
        if (room[k] < 0) p.g.inverse[i] = -1;
    }
    int total;
    int rank = wg_exscan(n, scan_s, tid, kSceneThreads, &total);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        rank_s[4 * tid + k] = rank;
        rank += room[k] >= 0 ? 1 : 0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int r = room[k];
        if (r < 0) continue;
        const int ra = p.room_start[r], a = ra > t0 ? ra : t0;           // t0 <= a <= the row
        const int before = __float_as_int(p.g.records[(size_t)(tile + r) * 8 + 7]);
        const int pos = p.pair_base[r] + before + rank_s[4 * tid + k] - rank_s[a - t0];
        if (pos >= 0 && pos < M) p.g.pairs_a[pos] = key[k];              // pos < M <= N: the prefixes of the finite rows
    }
}

__global__ __launch_bounds__(kSceneThreads) void grid_rooms_voxel_kernel(const GridRoomsArgs p)
{
    grid_voxel_body<true>(p.g, GridRoomsView{p.room, p.cell_base, p.voxel_room, p.R});
}

__global__ __launch_bounds__(kSceneThreads) void grid_rooms_count_max_kernel(const GridRoomsArgs p)
{
    __shared__ int max_s[kSceneThreads / 64];
    const int tid = threadIdx.x, tile = blockIdx.x, V = p.g.hdr->occupied;
    const int v0 = tile * kGridCountTile;
    if (v0 >= V) return;                                 // uniform; such a tile is never read
    int m = 0;
    for (int k = 0; k < kGridCountTile / kSceneThreads; ++k) {
        const int v = v0 + tid + k * kSceneThreads;
        if (v < V) {                                     // v + 1 <= V <= N: inside start
            const int n = p.g.start[v + 1] - p.g.start[v];
            m = n > m ? n : m;
        }
    }
    for (int d = 32; d >= 1; d >>= 1) {
        const int o = __shfl_xor(m, d, 64);
        m = o > m ? o : m;
    }
    if ((tid & 63) == 0) max_s[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < kSceneThreads / 64; ++k) m = max_s[k] > m ? max_s[k] : m;
        p.tile_max[tile] = m;
    }
}

// A wave per room.  first_r, the occupied voxels of the rooms before r, is the number of voxels whose head's cell id is
// below cell_base[r]: a binary search over the voxels' heads.
__global__ __launch_bounds__(kSceneThreads) void grid_rooms_out_kernel(const GridRoomsArgs p)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = kSceneThreads / 64;
    const GridHeader h = *p.g.hdr;
    const unsigned long long *sorted = (h.passes & 1) ? p.g.pairs_b : p.g.pairs_a;
    const int V = h.occupied, mv = p.g.max_voxels;
    for (int r = blockIdx.x * waves + wave; r < p.R; r += (int)gridDim.x * waves) {
        int f = 0;
        if (lane < 2) {
            const long long base = p.cell_base[r + lane];
            // the voxels whose cell id is below base
            f = lower_bound(0, V, [&](int m) { return (long long)(sorted[p.g.start[m]] >> kGridRowBits) < base; });
        }
        const int f0 = __shfl(f, 0, 64), f1 = __shfl(f, 1, 64);
        const int T0 = (f0 + kGridCountTile - 1) / kGridCountTile, T1 = f1 / kGridCountTile;
        int m = 0;
        const int e0 = T0 < T1 ? T0 * kGridCountTile : f1;       // [f0, e0) and [e1, f1) voxel by voxel
        const int e1 = T0 < T1 ? T1 * kGridCountTile : f1;
        for (int v = f0 + lane; v < e0; v += 64) {
            const int n = p.g.start[v + 1] - p.g.start[v];
            m = n > m ? n : m;
        }
        for (int v = e1 + lane; v < f1; v += 64) {
            const int n = p.g.start[v + 1] - p.g.start[v];
            m = n > m ? n : m;
        }
        for (int t = T0 + lane; t < T1; t += 64) m = p.tile_max[t] > m ? p.tile_max[t] : m;   // whole tiles below V
        for (int d = 32; d >= 1; d >>= 1) {
            const int o = __shfl_xor(m, d, 64);
            m = o > m ? o : m;
        }
        if (lane == 0) {
            const GridRoomFrame fr = p.room[r];
            const int a = f0 < mv ? f0 : mv, b = f1 < mv ? f1 : mv;
            int32_t *s = p.room_stats + (size_t)r * 8;
            s[0] = b - a;
            s[1] = f1 - f0;
            s[2] = fr.n[0];
            s[3] = fr.n[1];
            s[4] = fr.n[2];
            s[5] = fr.nonfinite;
            s[6] = m;
            s[7] = fr.error;
            p.voxel_start[r] = a;
            if (r == p.R - 1) p.voxel_start[p.R] = b;
        }
    }
}

__global__ __launch_bounds__(kGridScanThreads) void grid_rooms_stats_kernel(const GridRoomsArgs p)
{
    __shared__ int scan_s[kGridScanThreads / 64];
    __shared__ int red_s[kGridScanThreads / 64];
    const int tid = threadIdx.x;
    int with = 0, m = 0;
    for (int r = tid; r < p.R; r += kGridScanThreads) {
        const int32_t *s = p.room_stats + (size_t)r * 8;
        with += s[0] > 0 ? 1 : 0;
        m = s[6] > m ? s[6] : m;
    }
    int with_all;
    (void)wg_exscan(with, scan_s, tid, kGridScanThreads, &with_all);
    for (int d = 32; d >= 1; d >>= 1) {
        const int o = __shfl_xor(m, d, 64);
        m = o > m ? o : m;
    }
    if ((tid & 63) == 0) red_s[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < kGridScanThreads / 64; ++k) m = red_s[k] > m ? red_s[k] : m;
        const GridHeader h = *p.g.hdr;
        p.g.stats[0] = h.emitted;
        p.g.stats[1] = h.occupied;
        p.g.stats[2] = p.R;
        p.g.stats[3] = with_all;
        p.g.stats[4] = p.xh->errors;
        p.g.stats[5] = h.nonfinite;
        p.g.stats[6] = m;
        p.g.stats[7] = p.xh->flags;
    }
}

}  // namespace conv3p
