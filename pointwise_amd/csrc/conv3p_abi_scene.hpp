// conv3p_abi_scene.hpp -- host side of scene tiling and voting: blocks (plain, cover, rooms) and the vote / score calls.
// Included by conv3p_abi.hip.
namespace {

// The workspace of conv3p_scene_blocks_f32 (conv3p_scene.hpp): a host-side upper bound from the five arguments.
struct ScenePlan { int records, chunk_rows, chunks, blocks, m; };
bool scene_plan(int64_t N, int num_point, int max_blocks, float block, float stride, ScenePlan &w)
{
    if (N <= 0 || N > kSceneMaxN || num_point < 1 || num_point > kSceneMaxP || max_blocks <= 0) return false;
    if (!std::isfinite(block) || !std::isfinite(stride) || !(block > 0.0f) || !(stride > 0.0f)) return false;
    if (block < stride || block > 2.0f * stride) return false;
    const size_t tiles = ((size_t)N + kSceneThreads - 1) / kSceneThreads;
    w.records = (int)(tiles < (size_t)kSceneMaxRecords ? tiles : (size_t)kSceneMaxRecords);
    const size_t even = (((size_t)N + kSceneMaxChunks - 1) / kSceneMaxChunks + kSceneThreads - 1) / kSceneThreads * kSceneThreads;
    w.chunk_rows = (int)(even > (size_t)kSceneMinChunk ? even : (size_t)kSceneMinChunk);
    w.chunks = (int)(((size_t)N + w.chunk_rows - 1) / w.chunk_rows);
    w.blocks = max_blocks < kSceneMaxCells ? max_blocks : kSceneMaxCells;
    w.m = (int)std::ceil((double)block / (double)stride) + 1;                        // cells a row can be in, an axis
    return true;
}
// The workspace itself.  The covering call (conv3p_scene_cover.hpp) has the plain call's, with its three per-block arrays
// and the chunk counts per LISTED cell (at most min(max_blocks, cells)), then the listed cells' first block numbers and
// the block table.
size_t carve_scene(void *ws, bool cover, const ScenePlan &w, int64_t N, int max_blocks, SceneArgs &a)
{
    Carver cv(ws);
    a.hdr = cv.take<SceneHeader>(1);
    a.records = cv.take<float>((size_t)kSceneMaxRecords * 8);
    a.count = cv.take<int>((size_t)kSceneMaxCells);
    a.blk_cell = cv.take<int>((size_t)w.blocks);
    a.blk_count = cv.take<int>((size_t)w.blocks);
    a.blk_off = cv.take<int>((size_t)w.blocks);
    a.chunk_count = cv.take<int>((size_t)w.blocks * kSceneMaxChunks);
    a.members = cv.take<int>((size_t)N * w.m * w.m);
    a.blk_first = cover ? cv.take<int>((size_t)w.blocks) : nullptr;
    a.table = cover ? cv.take<int4>((size_t)max_blocks) : nullptr;
    return cv.bytes();
}
size_t scene_workspace_bytes(bool cover, int64_t N, int num_point, int max_blocks, float block, float stride)
{
    ScenePlan w;
    SceneArgs a;
    return scene_plan(N, num_point, max_blocks, block, stride, w) ? carve_scene(nullptr, cover, w, N, max_blocks, a) : 0;
}
inline unsigned scene_grid(size_t work)
{
    const size_t g = (work + kSceneThreads - 1) / kSceneThreads;
    return (unsigned)(g < (size_t)kSceneMaxRecords ? (g ? g : 1) : (size_t)kSceneMaxRecords);
}

// Both modes of the partition.  Every status first, in the order include/conv3p.h gives; then the seven launches (the
// covering mode: eight), outside the profile bracket (the table of kinds is pinned), as provider_impl.
int scene_blocks_impl(bool cover, const float *data, const void *labels, int64_t N, int K, int label_bytes, float block,
                      float stride, int num_point, int min_points, int max_blocks, uint64_t seed, uint64_t step,
                      float *blocks_out, int32_t *labels_out, int32_t *index_out, int32_t *block_cell,
                      int32_t *block_count, int32_t *stats, void *workspace, size_t workspace_bytes, void *stream)
{
    if (N < 0 || K < 3 || num_point < 1 || max_blocks < 0) return CONV3P_ERR_INVALID_ARGUMENT;
    if (!std::isfinite(block) || !std::isfinite(stride) || !(block > 0.0f) || !(stride > 0.0f)) return CONV3P_ERR_INVALID_ARGUMENT;
    if ((labels != nullptr) != (labels_out != nullptr)) return CONV3P_ERR_INVALID_ARGUMENT;
    if (labels && label_bytes != 1 && label_bytes != 4 && label_bytes != 8) return CONV3P_ERR_INVALID_ARGUMENT;
    if (N == 0 || max_blocks == 0) return CONV3P_OK;
    if (!data || !blocks_out || !index_out || !block_cell || !block_count || !stats) return CONV3P_ERR_INVALID_ARGUMENT;
    if (N > kSceneMaxN || num_point > kSceneMaxP || K > 65536 || block < stride || block > 2.0f * stride)
        return CONV3P_ERR_UNSUPPORTED;
    ScenePlan w;
    if (!scene_plan(N, num_point, max_blocks, block, stride, w)) return CONV3P_ERR_UNSUPPORTED;
    SceneArgs a;
    TRY(buf_check(workspace, workspace_bytes, carve_scene(workspace, cover, w, N, max_blocks, a)));
    a.data = data; a.labels = labels;
    a.N = (int)N; a.K = K; a.label_bytes = label_bytes; a.P = num_point; a.min_points = min_points; a.max_blocks = max_blocks;
    a.block = block; a.stride = stride;
    a.seed_lo = (unsigned)seed; a.seed_hi = (unsigned)(seed >> 32);
    a.step_lo = (unsigned)step; a.step_hi = (unsigned)(step >> 32);
    a.blocks_out = blocks_out; a.labels_out = labels_out; a.index_out = index_out;
    a.block_cell = block_cell; a.block_count = block_count; a.stats = stats;
    a.records_n = w.records; a.chunk_rows = w.chunk_rows; a.chunks = w.chunks;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t items = (size_t)w.blocks * w.chunks;
    const unsigned igrid = capped_grid(items, kSceneMaxGrid), egrid = capped_grid((size_t)max_blocks, kSceneMaxGrid);
    hipLaunchKernelGGL(scene_bounds_kernel, dim3((unsigned)w.records), dim3(kSceneThreads), 0, s, a);
    hipLaunchKernelGGL(scene_finish_kernel, dim3(1), dim3(kSceneMaxRecords), 0, s, a);
    hipLaunchKernelGGL(scene_count_kernel, dim3((unsigned)w.records), dim3(kSceneThreads), 0, s, a);
    if (cover) {
        hipLaunchKernelGGL(scene_cover_plan_kernel, dim3(1), dim3(kScenePlanThreads), 0, s, a);
        hipLaunchKernelGGL(scene_cover_table_kernel, dim3(scene_grid((size_t)max_blocks)), dim3(kSceneThreads), 0, s, a);
    } else {
        hipLaunchKernelGGL(scene_plan_kernel, dim3(1), dim3(kScenePlanThreads), 0, s, a);
    }
    hipLaunchKernelGGL(scene_fill_count_kernel, dim3(igrid), dim3(kSceneThreads), 0, s, a);
    hipLaunchKernelGGL(scene_fill_kernel, dim3(igrid), dim3(kSceneThreads), 0, s, a);
    if (cover)
        hipLaunchKernelGGL(scene_cover_emit_kernel, dim3(egrid), dim3(kSceneThreads), 0, s, a);
    else
        hipLaunchKernelGGL(scene_emit_kernel, dim3(egrid), dim3(kSceneThreads), 0, s, a);
    return hip_ok();
}

// The workspace of conv3p_scene_blocks_rooms_f32 (conv3p_scene_rooms.hpp): a host-side upper bound from the arguments.
// The two pair buffers dominate it: N * m^2 pairs of 8 bytes each, m = ceil(block / stride) + 1 the cells a row can be
// in along an axis -- at m = 3 that is 144 bytes a row.
struct RoomsPlan {
    int row_tiles, listed_max, pairs_max, sort_tiles;
};
bool rooms_plan(int64_t N, int64_t R, int num_point, int max_blocks, float block, float stride, RoomsPlan &w)
{
    if (N <= 0 || N > kRoomsMaxN || R <= 0 || R > kRoomsMaxRooms || num_point < 1 || num_point > kSceneMaxP || max_blocks <= 0)
        return false;
    if (!std::isfinite(block) || !std::isfinite(stride) || !(block > 0.0f) || !(stride > 0.0f)) return false;
    if (block < stride || block > 2.0f * stride) return false;
    const size_t m = (size_t)std::ceil((double)block / (double)stride) + 1;
    w.row_tiles = (int)((N + kRoomsRowTile - 1) / kRoomsRowTile);
    w.listed_max = max_blocks < kRoomsMaxCells ? max_blocks : kRoomsMaxCells;
    w.pairs_max = (int)((size_t)N * m * m);                                          // <= 9 * 2^26 < 2^31
    w.sort_tiles = (w.pairs_max + kRoomsSortTile - 1) / kRoomsSortTile;
    return true;
}
size_t carve_rooms(void *ws, const RoomsPlan &w, int64_t R, int max_blocks, RoomsArgs &a)
{
    Carver cv(ws);
    a.hdr = cv.take<RoomsHeader>(1);
    a.room = cv.take<RoomFrame>((size_t)R);
    a.cell_base = cv.take<int>((size_t)(R + 1));
    a.room_pref = cv.take<int4>((size_t)(R + 1));
    a.records = cv.take<float>(((size_t)w.row_tiles + (size_t)R) * 8);
    a.tile_pairs = cv.take<int>((size_t)w.row_tiles);
    a.seg_start = cv.take<int>((size_t)kRoomsMaxCells);
    a.seg_end = cv.take<int>((size_t)kRoomsMaxCells);
    a.blk_cell = cv.take<int>((size_t)w.listed_max);
    a.blk_count = cv.take<int>((size_t)w.listed_max);
    a.blk_off = cv.take<int>((size_t)w.listed_max);
    a.blk_first = cv.take<int>((size_t)w.listed_max);
    a.table = cv.take<int4>((size_t)max_blocks);
    a.blk_room = cv.take<int>((size_t)max_blocks);
    a.hist = cv.take<int>((size_t)w.sort_tiles * kRoomsDigits);
    a.pairs_a = cv.take<unsigned long long>((size_t)w.pairs_max);
    a.pairs_b = cv.take<unsigned long long>((size_t)w.pairs_max);
    return cv.bytes();
}

// The label of every room row from its votes (conv3p_scene_vote_labels) or its summed scores (conv3p_scene_score_labels,
// at most kScoreMaxClass classes): the kernel, then scene_vote_finish_kernel over the workgroups' partial counts.
size_t scene_labels_bytes(int64_t N, int num_class, int max_class)
{
    long long *partial;
    if (N <= 0 || N > (int64_t)INT32_MAX || num_class < 1 || num_class > max_class) return 0;
    return carve_one(nullptr, (size_t)kSceneMaxRecords, partial);
}
template <typename V>
int scene_labels_impl(void (*kernel)(const V *, long long, int, int32_t *, long long *), const V *in, int64_t N, int num_class,
                      int max_class, int32_t *label_out, int64_t *stats, void *workspace, size_t workspace_bytes, void *stream)
{
    if (N < 0 || num_class < 1) return CONV3P_ERR_INVALID_ARGUMENT;
    if (N == 0) return CONV3P_OK;
    if (!in || !label_out || !stats) return CONV3P_ERR_INVALID_ARGUMENT;
    if (N > (int64_t)INT32_MAX || num_class > max_class) return CONV3P_ERR_UNSUPPORTED;
    long long *partial;
    TRY(buf_check(workspace, workspace_bytes, carve_one(workspace, (size_t)kSceneMaxRecords, partial)));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned grid = scene_grid((size_t)N);
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kSceneThreads), 0, s, in, (long long)N, num_class, label_out, partial);
    hipLaunchKernelGGL(scene_vote_finish_kernel, dim3(1), dim3(kSceneMaxRecords), 0, s, (const long long *)partial, (int)grid,
                       (long long)N, reinterpret_cast<long long *>(stats));
    return hip_ok();
}

}  // namespace

extern "C" {

size_t conv3p_scene_blocks_workspace_bytes(int64_t N, int num_point, int max_blocks, float block, float stride)
{
    return scene_workspace_bytes(false, N, num_point, max_blocks, block, stride);
}

size_t conv3p_scene_blocks_cover_workspace_bytes(int64_t N, int num_point, int max_blocks, float block, float stride)
{
    return scene_workspace_bytes(true, N, num_point, max_blocks, block, stride);
}

#define SCENE_PARAMS                                                                                                 \
    const float *data, const void *labels, int64_t N, int K, int label_bytes, float block, float stride,             \
        int num_point, int min_points, int max_blocks, uint64_t seed, uint64_t step, float *blocks_out,              \
        int32_t *labels_out, int32_t *index_out, int32_t *block_cell, int32_t *block_count, int32_t *stats,          \
        void *workspace, size_t workspace_bytes, void *stream
#define SCENE_ARGS                                                                                                   \
    data, labels, N, K, label_bytes, block, stride, num_point, min_points, max_blocks, seed, step, blocks_out,       \
        labels_out, index_out, block_cell, block_count, stats, workspace, workspace_bytes, stream
int conv3p_scene_blocks_f32(SCENE_PARAMS) { return scene_blocks_impl(false, SCENE_ARGS); }
int conv3p_scene_blocks_cover_f32(SCENE_PARAMS) { return scene_blocks_impl(true, SCENE_ARGS); }
#undef SCENE_PARAMS
#undef SCENE_ARGS

size_t conv3p_scene_blocks_rooms_workspace_bytes(int64_t N, int64_t R, int num_point, int max_blocks, float block,
                                                 float stride, int cover)
{
    RoomsPlan w;
    RoomsArgs a;
    if (cover != 0 && cover != 1) return 0;
    return rooms_plan(N, R, num_point, max_blocks, block, stride, w) ? carve_rooms(nullptr, w, R, max_blocks, a) : 0;
}

// Every status first, in the order include/conv3p.h gives; then the launches, their number fixed, outside the profile
// bracket as scene_blocks_impl's.
int conv3p_scene_blocks_rooms_f32(const float *data, const void *labels, const int32_t *room_start, int64_t N, int64_t R,
                                  int K, int label_bytes, float block, float stride, int num_point, int min_points,
                                  int max_blocks, int cover, uint64_t seed, uint64_t step, float *blocks_out,
                                  int32_t *labels_out, int32_t *index_out, int32_t *block_cell, int32_t *block_count,
                                  int32_t *block_room, int32_t *room_blocks, int32_t *room_stats, int32_t *stats,
                                  void *workspace, size_t workspace_bytes, void *stream)
{
    if (N < 0 || R < 0 || K < 3 || num_point < 1 || max_blocks < 0 || (cover != 0 && cover != 1)) return CONV3P_ERR_INVALID_ARGUMENT;
    if (!std::isfinite(block) || !std::isfinite(stride) || !(block > 0.0f) || !(stride > 0.0f)) return CONV3P_ERR_INVALID_ARGUMENT;
    if ((labels != nullptr) != (labels_out != nullptr)) return CONV3P_ERR_INVALID_ARGUMENT;
    if (labels && label_bytes != 1 && label_bytes != 4 && label_bytes != 8) return CONV3P_ERR_INVALID_ARGUMENT;
    if (R == 0 || N == 0 || max_blocks == 0) return CONV3P_OK;
    if (!data || !room_start || !blocks_out || !index_out || !block_cell || !block_count || !block_room || !room_blocks ||
        !room_stats || !stats)
        return CONV3P_ERR_INVALID_ARGUMENT;
    if (N > kRoomsMaxN || R > kRoomsMaxRooms || num_point > kSceneMaxP || K > 65536 || block < stride || block > 2.0f * stride)
        return CONV3P_ERR_UNSUPPORTED;
    RoomsPlan w;
    if (!rooms_plan(N, R, num_point, max_blocks, block, stride, w)) return CONV3P_ERR_UNSUPPORTED;
    RoomsArgs a;
    TRY(buf_check(workspace, workspace_bytes, carve_rooms(workspace, w, R, max_blocks, a)));
    a.data = data; a.labels = labels; a.room_start = room_start;
    a.N = (int)N; a.R = (int)R; a.K = K; a.label_bytes = label_bytes; a.P = num_point; a.min_points = min_points;
    a.max_blocks = max_blocks; a.cover = cover;
    a.block = block; a.stride = stride;
    a.seed_lo = (unsigned)seed; a.seed_hi = (unsigned)(seed >> 32);
    a.step_lo = (unsigned)step; a.step_hi = (unsigned)(step >> 32);
    a.blocks_out = blocks_out; a.labels_out = labels_out; a.index_out = index_out;
    a.block_cell = block_cell; a.block_count = block_count; a.block_room = block_room;
    a.room_blocks = room_blocks; a.room_stats = room_stats; a.stats = stats;
    a.row_tiles = w.row_tiles; a.listed_max = w.listed_max; a.pairs_max = w.pairs_max;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned rgrid = capped_grid((size_t)R, kSceneMaxRecords), sgrid = capped_grid((size_t)w.sort_tiles, kSceneMaxGrid);
    const unsigned egrid = capped_grid((size_t)max_blocks, kSceneMaxGrid);
    hipLaunchKernelGGL(rooms_check_kernel, dim3(1), dim3(kRoomsScanThreads), 0, s, a);
    hipLaunchKernelGGL(rooms_bounds_kernel, dim3((unsigned)w.row_tiles), dim3(kSceneThreads), 0, s, a);
    hipLaunchKernelGGL(rooms_finish_kernel, dim3(rgrid), dim3(kSceneThreads), 0, s, a);
    hipLaunchKernelGGL(rooms_base_kernel, dim3(1), dim3(kRoomsScanThreads), 0, s, a);
    hipLaunchKernelGGL(rooms_pairs_kernel<false>, dim3((unsigned)w.row_tiles), dim3(kSceneThreads), 0, s, a);
    hipLaunchKernelGGL(rooms_tile_scan_kernel, dim3(1), dim3(kRoomsScanThreads), 0, s, a);
    hipLaunchKernelGGL(rooms_pairs_kernel<true>, dim3((unsigned)w.row_tiles), dim3(kSceneThreads), 0, s, a);
    unsigned long long *src = a.pairs_a, *dst = a.pairs_b;
    for (int pass = 0; pass < kRoomsPasses; ++pass) {
        const int shift = pass * kRoomsDigitBits;
        hipLaunchKernelGGL(rooms_sort_hist_kernel, dim3(sgrid), dim3(kSceneThreads), 0, s, a, (const unsigned long long *)src, shift);
        hipLaunchKernelGGL(rooms_sort_scan_kernel, dim3(1), dim3(kRoomsScanThreads), 0, s, a);
        hipLaunchKernelGGL(rooms_sort_scatter_kernel, dim3(sgrid), dim3(64), 0, s, a, (const unsigned long long *)src, dst, shift);
        std::swap(src, dst);
    }
    // an odd number of passes: the sorted pairs are in pairs_b (= src after the last swap), where the emit reads them
    hipLaunchKernelGGL(rooms_segments_kernel, dim3(scene_grid((size_t)w.pairs_max)), dim3(kSceneThreads), 0, s, a,
                       (const unsigned long long *)src);
    hipLaunchKernelGGL(rooms_plan_kernel, dim3(1), dim3(kRoomsScanThreads), 0, s, a);
    hipLaunchKernelGGL(rooms_table_kernel, dim3(scene_grid((size_t)max_blocks)), dim3(kSceneThreads), 0, s, a);
    hipLaunchKernelGGL(rooms_stats_kernel, dim3(scene_grid((size_t)R + 1)), dim3(kSceneThreads), 0, s, a);
    hipLaunchKernelGGL(rooms_emit_kernel, dim3(egrid), dim3(kSceneThreads), 0, s, a);
    return hip_ok();
}

int conv3p_scene_vote(const int32_t *pred, const int32_t *index, size_t rows, int64_t N, int num_class, int32_t *votes,
                      void *stream)
{
    if (N < 0 || num_class < 1) return CONV3P_ERR_INVALID_ARGUMENT;
    if (rows == 0 || N == 0) return CONV3P_OK;
    if (!pred || !index || !votes) return CONV3P_ERR_INVALID_ARGUMENT;
    if (N > (int64_t)INT32_MAX) return CONV3P_ERR_UNSUPPORTED;              // index is int32
    hipLaunchKernelGGL(scene_vote_kernel, dim3(scene_grid(rows)), dim3(kSceneThreads), 0, static_cast<hipStream_t>(stream),
                       pred, index, rows, (long long)N, num_class, votes);
    return hip_ok();
}

size_t conv3p_scene_vote_labels_workspace_bytes(int64_t N, int num_class)
{
    return scene_labels_bytes(N, num_class, INT32_MAX);
}

int conv3p_scene_vote_labels(const int32_t *votes, int64_t N, int num_class, int32_t *label_out, int64_t *stats,
                             void *workspace, size_t workspace_bytes, void *stream)
{
    return scene_labels_impl(scene_vote_labels_kernel, votes, N, num_class, INT32_MAX, label_out, stats, workspace,
                             workspace_bytes, stream);
}

// Waves per workgroup of conv3p_scene_vote_scores_f32: four while their tiles fit 48 KB of LDS, then two, then one (128
// classes: 33.6 KB a wave).
int conv3p_scene_vote_scores_f32(const float *logits, const int32_t *index, size_t rows, int64_t N, int num_class,
                                 int64_t *scores, int64_t *stats, void *stream)
{
    if (N < 0 || num_class < 1) return CONV3P_ERR_INVALID_ARGUMENT;
    if (rows == 0 || N == 0) return CONV3P_OK;
    if (!logits || !index || !scores || !stats) return CONV3P_ERR_INVALID_ARGUMENT;
    if (N > (int64_t)INT32_MAX || num_class > kScoreMaxClass) return CONV3P_ERR_UNSUPPORTED;
    const int nw = score_lds_bytes(4, num_class) <= 48 * 1024 ? 4 : score_lds_bytes(2, num_class) <= 48 * 1024 ? 2 : 1;
    const size_t lds = score_lds_bytes(nw, num_class);
    const size_t tiles = (rows + 63) / 64, wgs = (tiles + nw - 1) / nw;
    const unsigned grid = capped_grid(wgs, kSceneMaxRecords);
    hipLaunchKernelGGL(scene_vote_scores_kernel, dim3(grid), dim3(64 * nw), lds, static_cast<hipStream_t>(stream), logits,
                       index, rows, (long long)N, num_class, reinterpret_cast<long long *>(scores),
                       reinterpret_cast<long long *>(stats));
    return hip_ok();
}

size_t conv3p_scene_score_labels_workspace_bytes(int64_t N, int num_class)
{
    return scene_labels_bytes(N, num_class, kScoreMaxClass);
}

int conv3p_scene_score_labels(const int64_t *scores, int64_t N, int num_class, int32_t *label_out, int64_t *stats,
                              void *workspace, size_t workspace_bytes, void *stream)
{
    return scene_labels_impl(scene_score_labels_kernel, reinterpret_cast<const long long *>(scores), N, num_class,
                             kScoreMaxClass, label_out, stats, workspace, workspace_bytes, stream);
}

}  // extern "C"
