// conv3p_abi_grid.hpp -- host side of the voxel grid: subsample (single, rooms), project, neighbours, interpolate (plain,
// rings), normals, segments (by label, smooth), absorb, segment geometry, segment pool, segment adjacency, merge, agglomerate.  Included
// by conv3p_abi.hip.
namespace {

// The workspace of conv3p_grid_subsample_f32 (conv3p_grid.hpp): a host-side bound from the arguments.  The two pair
// buffers dominate it, 16 bytes a row; the list starts add 4.
struct GridPlan { int row_tiles, sort_tiles, voxel_grid; };
bool grid_plan(int64_t N, int max_voxels, GridPlan &w)
{
    if (N <= 0 || N > kGridMaxN || max_voxels <= 0) return false;
    w.row_tiles = (int)((N + kGridRowTile - 1) / kGridRowTile);
    w.sort_tiles = (int)((N + kGridSortTile - 1) / kGridSortTile);
    const int64_t voxels = N > max_voxels ? N : (int64_t)max_voxels;               // occupied voxels and fillers
    const int64_t vg = (voxels + kGridVoxelGroups - 1) / kGridVoxelGroups;
    w.voxel_grid = (int)(vg < kSceneMaxGrid ? vg : kSceneMaxGrid);
    return true;
}
// The sort's and the lists' words, the tail of the single call's workspace and of the rooms call's alike.
void carve_grid_tail(Carver &cv, const GridPlan &w, int64_t N, GridArgs &g)
{
    g.hist = cv.take<int>((size_t)w.sort_tiles * kGridDigits);
    g.digit_total = cv.take<int>((size_t)kGridPasses * kGridDigits);
    g.heads = cv.take<int>((size_t)w.sort_tiles);
    g.start = cv.take<int>((size_t)N + 1);
    g.part_max = cv.take<int>((size_t)kSceneMaxGrid);
    g.pairs_a = cv.take<unsigned long long>((size_t)N);
    g.pairs_b = cv.take<unsigned long long>((size_t)N);
    g.row_tiles = w.row_tiles; g.voxel_grid = w.voxel_grid;
}
size_t carve_grid(void *ws, const GridPlan &w, int64_t N, GridArgs &a)
{
    Carver cv(ws);
    a.hdr = cv.take<GridHeader>(1);
    a.records = cv.take<float>((size_t)w.row_tiles * 8);
    a.tile_off = cv.take<int>((size_t)w.row_tiles);
    carve_grid_tail(cv, w, N, a);
    return cv.bytes();
}
// What the single call and the rooms call are given alike.
void grid_fill(GridArgs &a, const float *data, const void *labels, int64_t N, int K, int label_bytes, float voxel, int mode,
               int num_class, int max_voxels, float *out, int32_t *labels_out, int32_t *voxel_row, int32_t *voxel_count,
               int32_t *voxel_cell, int32_t *inverse, int32_t *stats)
{
    a.data = data; a.labels = labels;
    a.N = (int)N; a.K = K; a.label_bytes = label_bytes; a.mode = mode; a.num_class = num_class; a.max_voxels = max_voxels;
    a.voxel = voxel;
    a.out = out; a.labels_out = labels_out; a.voxel_row = voxel_row; a.voxel_count = voxel_count; a.voxel_cell = voxel_cell;
    a.inverse = inverse; a.stats = stats;
}
// The radix sort of the pairs and the voxels' list heads: 5 x {hist, scan, scatter}, then heads / heads-scan / heads.
void grid_sort_launch(const GridArgs &a, unsigned sgrid, hipStream_t s)
{
    for (int pass = 0; pass < kGridPasses; ++pass) {     // a pass above the cell ids' top bit returns at once
        hipLaunchKernelGGL(grid_sort_hist_kernel, dim3(sgrid), dim3(kSceneThreads), 0, s, a, pass);
        hipLaunchKernelGGL(grid_sort_scan_kernel, dim3(kGridDigits), dim3(kGridScanThreads), 0, s, a, pass);
        hipLaunchKernelGGL(grid_sort_scatter_kernel, dim3(sgrid), dim3(64), 0, s, a, pass);
    }
    hipLaunchKernelGGL(grid_heads_kernel<false>, dim3(sgrid), dim3(kSceneThreads), 0, s, a);
    hipLaunchKernelGGL(grid_heads_scan_kernel, dim3(1), dim3(kGridScanThreads), 0, s, a);
    hipLaunchKernelGGL(grid_heads_kernel<true>, dim3(sgrid), dim3(kSceneThreads), 0, s, a);
}
inline unsigned grid_mean_grid(int max_voxels, int K)
{
    return capped_grid(((size_t)max_voxels * (size_t)K + kSceneThreads - 1) / kSceneThreads, kSceneMaxGrid);
}

template <typename S>
int grid_interpolate(const float *data, int64_t N, int K, const int32_t *inverse, const float *voxel_data, int voxel_K,
                     const int32_t *neigh, const S *voxel_scores, int64_t M, int C, const int32_t *valid_labels, int k,
                     int32_t *out_labels, float *out_scores, int64_t *stats, void *stream)
{
    if (N < 0 || M < 0 || K < 3 || voxel_K < 3 || C < 1 || C > kInterpMaxClass || k < 1 || k > kInterpMaxK)
        return CONV3P_ERR_INVALID_ARGUMENT;
    if (!stats || (N > 0 && (!data || !inverse || !out_labels)) || (N > 0 && M > 0 && (!voxel_data || !neigh || !voxel_scores)))
        return CONV3P_ERR_INVALID_ARGUMENT;
    if (N > (int64_t)INT32_MAX || M > (int64_t)INT32_MAX) return CONV3P_ERR_UNSUPPORTED;   // inverse is int32
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(stats, 0, 3 * sizeof(int64_t), s) != hipSuccess) return CONV3P_ERR_LAUNCH;
    if (N == 0) return hip_ok();
    const size_t work = ((size_t)N + kInterpRows - 1) / kInterpRows;
    hipLaunchKernelGGL((grid_interpolate_kernel<S>), dim3(capped_grid(work, kInterpMaxGrid)), dim3(kInterpThreads), 0, s,
                       data, (long long)N, K, inverse, voxel_data, voxel_K, neigh, voxel_scores, (int)M, C, valid_labels, k,
                       out_labels, out_scores, reinterpret_cast<unsigned long long *>(stats));
    return hip_ok();
}

static_assert(kRingHeaderBytes % kAlign == 0 && kGsegHeaderBytes % kAlign == 0, "the headers keep what follows them aligned");
// The rings' workspace: the list's counter, and a place per row.
size_t carve_rings(void *ws, int64_t N, int32_t *&counter, int32_t *&list)
{
    Carver cv(ws);
    counter = cv.take<int32_t>(kRingHeaderBytes / sizeof(int32_t));
    list = cv.take<int32_t>((size_t)N);
    return cv.bytes();
}

// The plain pass as it stands, then the list of the rows it left without a candidate, then (rings > 1) their ring search.
template <typename S>
int grid_interpolate_rings(const float *data, int64_t N, int K, const int32_t *inverse, const float *voxel_data, int voxel_K,
                           const int32_t *neigh, const int32_t *voxel_cell, const int32_t *voxel_room,
                           const int32_t *voxel_start, int64_t num_rooms, const int32_t *grid_stats, const S *voxel_scores,
                           int64_t M, int C, const int32_t *valid_labels, int k, int rings, int32_t *out_labels,
                           float *out_scores, int32_t *out_ring, int64_t *stats, int64_t *ring_stats, void *workspace,
                           size_t workspace_bytes, void *stream)
{
    if (N < 0 || M < 0 || K < 3 || voxel_K < 3 || C < 1 || C > kInterpMaxClass || k < 1 || k > kInterpMaxK || rings < 1 ||
        rings > kRingMax || num_rooms < 0)
        return CONV3P_ERR_INVALID_ARGUMENT;
    if ((voxel_room == nullptr) != (voxel_start == nullptr)) return CONV3P_ERR_INVALID_ARGUMENT;
    if (!stats || !ring_stats || (N > 0 && (!data || !inverse || !out_labels)) ||
        (N > 0 && M > 0 && (!voxel_data || !neigh || !voxel_scores || !voxel_cell || !grid_stats)))
        return CONV3P_ERR_INVALID_ARGUMENT;
    if (N > (int64_t)INT32_MAX || M > (int64_t)INT32_MAX || num_rooms > kGridRoomsMaxRooms) return CONV3P_ERR_UNSUPPORTED;
    int32_t *counter, *list;
    const size_t need = carve_rings(workspace, N, counter, list);
    if (!workspace || workspace_bytes < need) return CONV3P_ERR_INVALID_ARGUMENT;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(ring_stats, 0, (kRingMax + 1) * sizeof(int64_t), s) != hipSuccess) return CONV3P_ERR_LAUNCH;
    if (hipMemsetAsync(counter, 0, sizeof(int32_t), s) != hipSuccess) return CONV3P_ERR_LAUNCH;
    const int rc = grid_interpolate(data, N, K, inverse, voxel_data, voxel_K, neigh, voxel_scores, M, C, valid_labels, k,
                                    out_labels, out_scores, stats, stream);
    if (rc != CONV3P_OK || N == 0) return rc;
    const size_t work = ((size_t)N + kRingListThreads - 1) / kRingListThreads;
    hipLaunchKernelGGL(grid_ring_list_kernel, dim3(capped_grid(work, kRingListMaxGrid)), dim3(kRingListThreads), 0, s,
                       inverse, out_labels, (long long)N, (int)M, rings, counter, list, out_ring,
                       reinterpret_cast<unsigned long long *>(ring_stats));
    if (rings > 1)
        hipLaunchKernelGGL((grid_ring_search_kernel<S>), dim3(kRingGrid), dim3(kRingThreads), 0, s, data, (long long)N, K, inverse,
                           voxel_data, voxel_K, voxel_cell, voxel_room, voxel_start, (int)num_rooms, grid_stats, voxel_scores,
                           (int)M, C, valid_labels, k, rings, counter, list, out_labels, out_scores, out_ring,
                           reinterpret_cast<unsigned long long *>(stats), reinterpret_cast<unsigned long long *>(ring_stats));
    return hip_ok();
}

// The taps of a connectivity as a mask over t = (dx+1)*9 + (dy+1)*3 + (dz+1); 0 for a connectivity that is none.
unsigned gseg_tapmask(int connectivity)
{
    const int reach = connectivity == 6 ? 1 : (connectivity == 18 ? 2 : (connectivity == 26 ? 3 : 0));
    unsigned mask = 0;
    for (int t = 0; t < kInterpNeigh; ++t) {
        const int d = std::abs(t / 9 - 1) + std::abs(t / 3 % 3 - 1) + std::abs(t % 3 - 1);
        if (d >= 1 && d <= reach) mask |= 1u << t;
    }
    return mask;
}
size_t gseg_tiles(int64_t M) { return ((size_t)M + kGsegTile - 1) / kGsegTile; }
// The consecutive voxels a wave takes in the kernels that reduce runs of equal segment, in steps of 64: more of them where
// there are waves enough to fill the device anyway.
int gseg_steps(int64_t M) { return M >= (1 << 20) ? 16 : (M >= (1 << 16) ? 4 : 1); }
// The segments call's workspace: the tiles' roots, lab, parent.
size_t carve_gseg(void *ws, int64_t M, int32_t *&tile_count, int32_t *&lab, int32_t *&parent)
{
    Carver cv(ws);
    tile_count = cv.take<int32_t>(gseg_tiles(M));
    lab = cv.take<int32_t>((size_t)M);
    parent = cv.take<int32_t>((size_t)M);
    return cv.bytes();
}
// The absorb call's: the two counts, two words per tile of segments, and cursor, small_list, small_off, members.
size_t carve_absorb(void *ws, int64_t M, AbsorbArgs &p)
{
    Carver cv(ws);
    p.hdr = cv.take<int32_t>(kGsegHeaderBytes / sizeof(int32_t));
    p.tile_small = cv.take<int32_t>(gseg_tiles(M));
    p.tile_members = cv.take<int32_t>(gseg_tiles(M));
    p.cursor = cv.take<int32_t>((size_t)M);
    p.small_list = cv.take<int32_t>((size_t)M);
    p.small_off = cv.take<int32_t>((size_t)M);
    p.members = cv.take<int32_t>((size_t)M);
    return cv.bytes();
}
// The adjacency call's: the counters, the radix passes' totals and histograms, the edge table of 2 max_edges + 64 slots (a
// key and five counters each) and the two key buffers of the sort.  A function of max_edges alone: M only bounds it.
void carve_adj_into(Carver &cv, int64_t max_edges, AdjArgs &p)
{
    p.slots = 2ull * (unsigned long long)max_edges + kAdjSlack;
    p.sort_tiles = (int)(((size_t)max_edges + kAdjSortTile - 1) / kAdjSortTile);
    if (p.sort_tiles < 1) p.sort_tiles = 1;
    p.hdr = cv.take<AdjHeader>(1);
    p.digit_total = cv.take<int>((size_t)2 * kAdjMaxBytes * kAdjDigits);
    p.hist = cv.take<int>((size_t)p.sort_tiles * kAdjDigits);
    p.keys = cv.take<unsigned long long>((size_t)p.slots);
    p.vals = cv.take<int32_t>((size_t)p.slots * kAdjVals);
    p.sort_a = cv.take<unsigned long long>((size_t)max_edges);
    p.sort_b = cv.take<unsigned long long>((size_t)max_edges);
}
size_t carve_adj(void *ws, int64_t max_edges, AdjArgs &p)
{
    Carver cv(ws);
    carve_adj_into(cv, max_edges, p);
    return cv.bytes();
}
// The merge call's: the tiles' roots, lab, parent, members, and the 64-bit label keys.
void carve_merge_into(Carver &cv, int64_t M, MergeArgs &p)
{
    p.tile_count = cv.take<int32_t>(gseg_tiles(M));
    p.lab = cv.take<int32_t>((size_t)M);
    p.parent = cv.take<int32_t>((size_t)M);
    p.members = cv.take<int32_t>((size_t)M);
    p.best = cv.take<unsigned long long>((size_t)M);
}
size_t carve_merge(void *ws, int64_t M, MergeArgs &p)
{
    Carver cv(ws);
    carve_merge_into(cv, M, p);
    return cv.bytes();
}
// The agglomeration's: its header, the groups' words (grp, the weights, the tiles' log rows, the label keys, best), a column
// for the edge_voxels adj_finish_kernel writes and H8 does not produce, then the adjacency call's and the merge call's as
// they stand.
size_t carve_agg(void *ws, int64_t M, int64_t max_edges, AggArgs &p, MergeArgs &m)
{
    Carver cv(ws);
    p.hdr = cv.take<AggHeader>(1);
    p.grp = cv.take<int32_t>((size_t)M);
    p.weight_of = cv.take<int32_t>((size_t)M);
    p.tile_count = cv.take<int32_t>(gseg_tiles(M));
    p.label_key = cv.take<unsigned long long>((size_t)M);
    p.best = cv.take<unsigned long long>((size_t)M);
    p.t.edge_voxels = cv.take<int32_t>((size_t)max_edges);
    carve_adj_into(cv, max_edges, p.t);
    carve_merge_into(cv, M, m);
    return cv.bytes();
}
unsigned gseg_grid(size_t work) { return (unsigned)(work < (size_t)kGsegMaxGrid ? (work ? work : 1) : (size_t)kGsegMaxGrid); }

// conv3p_grid_segments (rule NULL: labels equal) and conv3p_grid_segments_smooth (the rule of J2-J4): every status first,
// in the order include/conv3p.h gives; then seven launches whatever the data, the smooth call's behind a memset.
int gseg_run(const SmoothJoin *rule, const int32_t *neigh, const int32_t *voxel_labels, int64_t L, const int32_t *voxel_count,
             const int32_t *grid_stats, int64_t M, int num_class, int connectivity, int32_t *segment, int32_t *seg_root,
             int32_t *seg_size, int32_t *seg_rows, int32_t *seg_label, int32_t *seg_stats, void *workspace,
             size_t workspace_bytes, void *stream)
{
    const unsigned tapmask = gseg_tapmask(connectivity);
    if (M < 0 || (voxel_labels && (L < 0 || L > M)) || num_class < 1 || num_class > kGsegMaxClass || !tapmask)
        return CONV3P_ERR_INVALID_ARGUMENT;
    if (M == 0) return CONV3P_OK;
    if (!neigh || !voxel_count || !grid_stats || !segment || !seg_root || !seg_size || !seg_rows || !seg_label || !seg_stats)
        return CONV3P_ERR_INVALID_ARGUMENT;
    if (M > (int64_t)INT32_MAX) return CONV3P_ERR_UNSUPPORTED;
    int32_t *tile_count, *lab, *parent;
    const size_t need = carve_gseg(workspace, M, tile_count, lab, parent);
    if (!workspace || workspace_bytes < need) return CONV3P_ERR_INVALID_ARGUMENT;
    if (rule) {
        if (!rule->normals && !rule->features) return CONV3P_ERR_INVALID_ARGUMENT;
        if (rule->F < 0 || rule->F > kSmoothMaxFeatures || (rule->features != nullptr) != (rule->F > 0))
            return CONV3P_ERR_INVALID_ARGUMENT;
        if (rule->features && rule->feature_stride < rule->F) return CONV3P_ERR_INVALID_ARGUMENT;
        if (rule->signed_normals != 0 && rule->signed_normals != 1) return CONV3P_ERR_INVALID_ARGUMENT;
        if (std::isnan(rule->min_cos) || std::isnan(rule->max_curvature) || std::isnan(rule->max_difference))
            return CONV3P_ERR_INVALID_ARGUMENT;
        if (!rule->stats) return CONV3P_ERR_INVALID_ARGUMENT;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int m = (int)M, ntiles = (int)gseg_tiles(M), l = voxel_labels ? (int)L : 0, nc = voxel_labels ? num_class : 1;
    const unsigned per_thread = gseg_grid(((size_t)M + kGsegThreads - 1) / kGsegThreads), per_tile = gseg_grid((size_t)ntiles);
    const dim3 local_grid(gseg_grid(((size_t)M + kGsegLocalTile - 1) / kGsegLocalTile));
    if (rule) {
        if (hipMemsetAsync(rule->stats, 0, 8 * sizeof(int64_t), s) != hipSuccess) return CONV3P_ERR_LAUNCH;
        hipLaunchKernelGGL(smooth_local_kernel, local_grid, dim3(kGsegLocalTile), 0, s, *rule, neigh, voxel_labels, l, grid_stats,
                           m, nc, tapmask, lab, parent, seg_root, seg_size, seg_rows, seg_label, seg_stats);
        hipLaunchKernelGGL(smooth_link_kernel, dim3(per_thread), dim3(kGsegThreads), 0, s, *rule, neigh, lab, parent, grid_stats,
                           m, tapmask);
    } else {
        hipLaunchKernelGGL(gseg_local_kernel, local_grid, dim3(kGsegLocalTile), 0, s, neigh, voxel_labels, l, grid_stats, m, nc,
                           tapmask, lab, parent, seg_root, seg_size, seg_rows, seg_label, seg_stats);
        hipLaunchKernelGGL(gseg_link_kernel, dim3(per_thread), dim3(kGsegThreads), 0, s, neigh, lab, parent, grid_stats, m,
                           tapmask);
    }
    hipLaunchKernelGGL(gseg_flatten_kernel, dim3(per_tile), dim3(kGsegThreads), 0, s, lab, parent, m, ntiles, tile_count);
    hipLaunchKernelGGL(gseg_scan_kernel, dim3(1), dim3(kGsegScanThreads), 0, s, tile_count, static_cast<int32_t *>(nullptr),
                       ntiles, seg_stats, static_cast<int32_t *>(nullptr));
    hipLaunchKernelGGL(gseg_number_kernel, dim3(per_tile), dim3(kGsegThreads), 0, s, lab, parent, m, ntiles, tile_count, segment,
                       seg_root, seg_label);
    const int steps = gseg_steps(M);
    const size_t per_wave = (size_t)64 * steps * (kGsegThreads / 64);
    hipLaunchKernelGGL(gseg_assign_kernel, dim3(gseg_grid(((size_t)M + per_wave - 1) / per_wave)), dim3(kGsegThreads), 0, s, lab,
                       parent, voxel_count, grid_stats, m, steps, segment, seg_size, seg_rows, seg_stats);
    hipLaunchKernelGGL(gseg_max_kernel, dim3(per_thread), dim3(kGsegThreads), 0, s, seg_size, seg_rows, m, seg_stats);
    return hip_ok();
}

// The pool's two entries: every status first, in the order include/conv3p.h gives; then three launches, four with
// voxel_label, whatever the data; no workspace (conv3p_grid_smooth.hpp).
template <typename T>
int grid_segment_pool(const T *values, int64_t L, int C, int64_t value_stride, const int32_t *segment, const int32_t *seg_stats,
                      const int32_t *voxel_count, const int32_t *grid_stats, int64_t M, int weight, bool rows_allowed,
                      int64_t *sums, int64_t *weights, double *mean, int32_t *seg_label, int32_t *voxel_label,
                      int64_t *pool_stats, void *stream)
{
    if (M < 0 || L < 0 || L > M || C < 1 || C > kPoolMaxChannels || value_stride < C || (weight != 0 && weight != 1) ||
        (weight == 1 && !rows_allowed))
        return CONV3P_ERR_INVALID_ARGUMENT;
    if (M == 0) return CONV3P_OK;
    if ((L > 0 && !values) || !segment || !seg_stats || !voxel_count || !grid_stats || !sums || !weights || !seg_label ||
        !pool_stats)
        return CONV3P_ERR_INVALID_ARGUMENT;
    if (M > (int64_t)INT32_MAX) return CONV3P_ERR_UNSUPPORTED;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int m = (int)M;
    const unsigned per_thread = gseg_grid(((size_t)M + kGsegThreads - 1) / kGsegThreads);
    const unsigned per_word = gseg_grid(((size_t)M * (size_t)C + kGsegThreads - 1) / kGsegThreads);
    const int steps = gseg_steps(M);
    const size_t per_wave = (size_t)64 * steps * (kGsegThreads / 64);
    unsigned long long *usums = reinterpret_cast<unsigned long long *>(sums);
    unsigned long long *uweights = reinterpret_cast<unsigned long long *>(weights);
    unsigned long long *ustats = reinterpret_cast<unsigned long long *>(pool_stats);
    hipLaunchKernelGGL(pool_init_kernel, dim3(per_word), dim3(kGsegThreads), 0, s, m, C, usums, uweights, ustats);
    hipLaunchKernelGGL((pool_sum_kernel<T>), dim3(gseg_grid(((size_t)M + per_wave - 1) / per_wave)), dim3(kGsegThreads), 0, s,
                       values, (int)L, C, (long long)value_stride, segment, seg_stats, voxel_count, grid_stats, m, weight, steps,
                       usums, uweights, ustats);
    hipLaunchKernelGGL(pool_finish_kernel, dim3(per_thread), dim3(kGsegThreads), 0, s, seg_stats, m, C,
                       reinterpret_cast<const long long *>(sums), reinterpret_cast<const long long *>(weights), mean, seg_label,
                       ustats);
    if (voxel_label)
        hipLaunchKernelGGL(pool_voxel_kernel, dim3(per_thread), dim3(kGsegThreads), 0, s, segment, seg_stats, grid_stats, m,
                           seg_label, voxel_label);
    return hip_ok();
}

// The workspace of conv3p_grid_subsample_rooms_f32 (conv3p_grid_rooms.hpp): the single call's words -- the records grown
// by one per room, the tiles' pair offsets giving way to the voxel tiles' maxima -- and per room a frame and two prefixes.
bool grid_rooms_plan(int64_t N, int64_t R, int max_voxels, GridPlan &w)
{
    return R > 0 && R <= kGridRoomsMaxRooms && grid_plan(N, max_voxels, w);
}
size_t carve_grid_rooms(void *ws, const GridPlan &w, int64_t N, int64_t R, GridRoomsArgs &a)
{
    Carver cv(ws);
    a.g.hdr = cv.take<GridHeader>(1);
    a.xh = cv.take<GridRoomsHeader>(1);
    a.room = cv.take<GridRoomFrame>((size_t)R);
    a.cell_base = cv.take<long long>((size_t)R + 1);
    a.pair_base = cv.take<int>((size_t)R + 1);
    a.g.records = cv.take<float>(((size_t)w.row_tiles + (size_t)R) * 8);
    a.tile_max = cv.take<int>((size_t)w.row_tiles);
    a.g.tile_off = nullptr;
    carve_grid_tail(cv, w, N, a.g);
    return cv.bytes();
}

// The seven launches of conv3p_grid_merge_segments, for it and for the agglomeration.
void merge_launch(const MergeArgs &p, hipStream_t s)
{
    const unsigned per_thread = gseg_grid(((size_t)p.M + kGsegThreads - 1) / kGsegThreads), per_tile = gseg_grid((size_t)p.ntiles);
    hipLaunchKernelGGL(merge_init_kernel, dim3(per_thread), dim3(kGsegThreads), 0, s, p);
    hipLaunchKernelGGL(merge_union_kernel, dim3(gseg_grid(((size_t)p.P + kGsegThreads - 1) / kGsegThreads)), dim3(kGsegThreads), 0,
                       s, p);
    hipLaunchKernelGGL(gseg_flatten_kernel, dim3(per_tile), dim3(kGsegThreads), 0, s, p.lab, p.parent, p.M, p.ntiles,
                       p.tile_count);
    hipLaunchKernelGGL(gseg_scan_kernel, dim3(1), dim3(kGsegScanThreads), 0, s, p.tile_count, static_cast<int32_t *>(nullptr),
                       p.ntiles, p.stats_out, static_cast<int32_t *>(nullptr));
    hipLaunchKernelGGL(merge_number_kernel, dim3(per_tile), dim3(kGsegThreads), 0, s, p);
    hipLaunchKernelGGL(merge_assign_kernel, dim3(per_thread), dim3(kGsegThreads), 0, s, p);
    hipLaunchKernelGGL(merge_finish_kernel, dim3(per_thread), dim3(kGsegThreads), 0, s, p);
}
// The bytes of n - 1 (1 .. 4): the radix passes a half of a key below n can need.
int adj_key_bytes(int64_t n)
{
    int bytes = 1;
    while (bytes < kAdjMaxBytes && ((uint64_t)(n - 1) >> (8 * bytes))) ++bytes;
    return bytes;
}
// The 3 launches of every radix pass over `bytes` bytes of the halves [half0, half1) of p's keys (0: the low words).
void adj_passes_launch(const AdjArgs &p, int half0, int half1, int bytes, hipStream_t s)
{
    const unsigned per_tile = capped_grid((size_t)p.sort_tiles, kAdjMaxGrid);
    for (int half = half0; half < half1; ++half)
        for (int j = 0; j < bytes; ++j) {                // a pass above the top byte of S - 1 returns at once
            hipLaunchKernelGGL(adj_sort_hist_kernel, dim3(per_tile), dim3(kAdjThreads), 0, s, p, half, j);
            hipLaunchKernelGGL(adj_sort_scan_kernel, dim3(kAdjDigits), dim3(kAdjScanThreads), 0, s, p, half, j);
            hipLaunchKernelGGL(adj_sort_scatter_kernel, dim3(per_tile), dim3(64), 0, s, p, half, j);
        }
}
// The compaction and the 6 b launches of the radix passes, b the bytes of M - 1 >= S - 1: the passes a half of the key can
// need.  For the adjacency, the agglomeration and the segment matching.
void adj_sort_launch(const AdjArgs &p, hipStream_t s)
{
    const unsigned per_slot = capped_grid(((size_t)p.slots + kAdjThreads - 1) / kAdjThreads, kAdjMaxGrid);
    hipLaunchKernelGGL(adj_compact_kernel, dim3(per_slot), dim3(kAdjThreads), 0, s, p);
    adj_passes_launch(p, 0, 2, adj_key_bytes(p.M), s);
}
// The sort and the finish of conv3p_grid_segment_adjacency, for it and for the agglomeration.
void adj_order_launch(const AdjArgs &p, hipStream_t s)
{
    const size_t rows = std::max((size_t)p.M + 1, (size_t)p.max_edges);
    adj_sort_launch(p, s);
    hipLaunchKernelGGL(adj_finish_kernel, dim3(capped_grid((rows + kAdjThreads - 1) / kAdjThreads, kAdjMaxGrid)),
                       dim3(kAdjThreads), 0, s, p);
}
}  // namespace

extern "C" {

size_t conv3p_grid_subsample_workspace_bytes(int64_t N, int max_voxels)
{
    GridPlan w;
    GridArgs a;
    return grid_plan(N, max_voxels, w) ? carve_grid(nullptr, w, N, a) : 0;
}

// Every status first, in the order include/conv3p.h gives; then the launches, their number fixed by the arguments.
int conv3p_grid_subsample_f32(const float *data, const void *labels, int64_t N, int K, int label_bytes, float voxel,
                              int mode, int num_class, int max_voxels, float *out, int32_t *labels_out,
                              int32_t *voxel_row, int32_t *voxel_count, int32_t *voxel_cell, int32_t *inverse,
                              int32_t *stats, void *workspace, size_t workspace_bytes, void *stream)
{
    if (N < 0 || K < 3 || max_voxels < 0 || (mode != 0 && mode != 1)) return CONV3P_ERR_INVALID_ARGUMENT;
    if (!std::isfinite(voxel) || !(voxel > 0.0f)) return CONV3P_ERR_INVALID_ARGUMENT;
    if ((labels != nullptr) != (labels_out != nullptr)) return CONV3P_ERR_INVALID_ARGUMENT;
    if (labels && label_bytes != 1 && label_bytes != 4 && label_bytes != 8) return CONV3P_ERR_INVALID_ARGUMENT;
    const bool votes = labels && mode == 0;              // num_class is read by the majority only
    if (votes && num_class < 1) return CONV3P_ERR_INVALID_ARGUMENT;
    if (N == 0 || max_voxels == 0) return CONV3P_OK;
    if (!data || !out || !voxel_row || !voxel_count || !voxel_cell || !inverse || !stats) return CONV3P_ERR_INVALID_ARGUMENT;
    if (N > kGridMaxN || K > 65536 || (votes && num_class > kGridMaxClass)) return CONV3P_ERR_UNSUPPORTED;
    GridPlan w;
    if (!grid_plan(N, max_voxels, w)) return CONV3P_ERR_UNSUPPORTED;
    GridArgs a;
    TRY(buf_check(workspace, workspace_bytes, carve_grid(workspace, w, N, a)));
    grid_fill(a, data, labels, N, K, label_bytes, voxel, mode, num_class, max_voxels, out, labels_out, voxel_row, voxel_count,
              voxel_cell, inverse, stats);
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(grid_bounds_kernel, dim3((unsigned)w.row_tiles), dim3(kSceneThreads), 0, s, a);
    hipLaunchKernelGGL(grid_frame_kernel, dim3(1), dim3(kGridScanThreads), 0, s, a);
    hipLaunchKernelGGL(grid_pairs_kernel, dim3((unsigned)w.row_tiles), dim3(kSceneThreads), 0, s, a);
    grid_sort_launch(a, capped_grid((size_t)w.sort_tiles, kSceneMaxGrid), s);
    hipLaunchKernelGGL(grid_voxel_kernel, dim3((unsigned)w.voxel_grid), dim3(kSceneThreads), 0, s, a);
    if (mode == 0) hipLaunchKernelGGL(grid_mean_kernel, dim3(grid_mean_grid(max_voxels, K)), dim3(kSceneThreads), 0, s, a);
    hipLaunchKernelGGL(grid_stats_kernel, dim3(1), dim3(kGridScanThreads), 0, s, a);
    return hip_ok();
}

int conv3p_grid_project_labels(const int32_t *voxel_labels, const int32_t *inverse, int64_t N, int64_t M, int32_t *out,
                               void *stream)
{
    if (N < 0 || M < 0) return CONV3P_ERR_INVALID_ARGUMENT;
    if (N == 0) return CONV3P_OK;
    if (!inverse || !out || (M > 0 && !voxel_labels)) return CONV3P_ERR_INVALID_ARGUMENT;
    if (N > (int64_t)INT32_MAX || M > (int64_t)INT32_MAX) return CONV3P_ERR_UNSUPPORTED;   // inverse is int32
    const size_t work = ((size_t)N + kSceneThreads - 1) / kSceneThreads;
    hipLaunchKernelGGL(grid_project_kernel, dim3(capped_grid(work, kSceneMaxGrid)), dim3(kSceneThreads), 0,
                       static_cast<hipStream_t>(stream), voxel_labels, inverse, (long long)N, (long long)M, out);
    return hip_ok();
}

int conv3p_grid_neighbors(const int32_t *voxel_cell, const int32_t *voxel_room, const int32_t *voxel_start,
                          const int32_t *grid_stats, int max_voxels, int64_t num_rooms, int32_t *neigh, void *stream)
{
    if (max_voxels < 0 || num_rooms < 0) return CONV3P_ERR_INVALID_ARGUMENT;
    if ((voxel_room == nullptr) != (voxel_start == nullptr)) return CONV3P_ERR_INVALID_ARGUMENT;
    if (max_voxels == 0) return CONV3P_OK;
    if (!voxel_cell || !grid_stats || !neigh) return CONV3P_ERR_INVALID_ARGUMENT;
    if (num_rooms > kGridRoomsMaxRooms) return CONV3P_ERR_UNSUPPORTED;
    const size_t work = ((size_t)max_voxels * 9 + kSceneThreads - 1) / kSceneThreads;
    hipLaunchKernelGGL(grid_neighbors_kernel, dim3(capped_grid(work, kSceneMaxGrid)), dim3(kSceneThreads), 0,
                       static_cast<hipStream_t>(stream), voxel_cell, voxel_room, voxel_start, grid_stats, max_voxels,
                       (int)num_rooms, neigh);
    return hip_ok();
}

int conv3p_grid_interpolate_f32(const float *data, int64_t N, int K, const int32_t *inverse, const float *voxel_data,
                                int voxel_K, const int32_t *neigh, const float *voxel_scores, int64_t M, int C,
                                const int32_t *valid_labels, int k, int32_t *out_labels, float *out_scores, int64_t *stats,
                                void *stream)
{
    return grid_interpolate(data, N, K, inverse, voxel_data, voxel_K, neigh, voxel_scores, M, C, valid_labels, k, out_labels,
                            out_scores, stats, stream);
}

int conv3p_grid_interpolate_i64(const float *data, int64_t N, int K, const int32_t *inverse, const float *voxel_data,
                                int voxel_K, const int32_t *neigh, const int64_t *voxel_scores, int64_t M, int C,
                                const int32_t *valid_labels, int k, int32_t *out_labels, float *out_scores, int64_t *stats,
                                void *stream)
{
    return grid_interpolate(data, N, K, inverse, voxel_data, voxel_K, neigh, reinterpret_cast<const long long *>(voxel_scores),
                            M, C, valid_labels, k, out_labels, out_scores, stats, stream);
}

size_t conv3p_grid_interpolate_rings_workspace_bytes(int64_t N)
{
    int32_t *counter, *list;
    if (N < 0 || N > (int64_t)INT32_MAX) return 0;
    return carve_rings(nullptr, N, counter, list);
}

int conv3p_grid_interpolate_rings_f32(const float *data, int64_t N, int K, const int32_t *inverse, const float *voxel_data,
                                      int voxel_K, const int32_t *neigh, const int32_t *voxel_cell, const int32_t *voxel_room,
                                      const int32_t *voxel_start, int64_t num_rooms, const int32_t *grid_stats,
                                      const float *voxel_scores, int64_t M, int C, const int32_t *valid_labels, int k, int rings,
                                      int32_t *out_labels, float *out_scores, int32_t *out_ring, int64_t *stats,
                                      int64_t *ring_stats, void *workspace, size_t workspace_bytes, void *stream)
{
    return grid_interpolate_rings(data, N, K, inverse, voxel_data, voxel_K, neigh, voxel_cell, voxel_room, voxel_start, num_rooms,
                                  grid_stats, voxel_scores, M, C, valid_labels, k, rings, out_labels, out_scores, out_ring, stats,
                                  ring_stats, workspace, workspace_bytes, stream);
}

int conv3p_grid_interpolate_rings_i64(const float *data, int64_t N, int K, const int32_t *inverse, const float *voxel_data,
                                      int voxel_K, const int32_t *neigh, const int32_t *voxel_cell, const int32_t *voxel_room,
                                      const int32_t *voxel_start, int64_t num_rooms, const int32_t *grid_stats,
                                      const int64_t *voxel_scores, int64_t M, int C, const int32_t *valid_labels, int k, int rings,
                                      int32_t *out_labels, float *out_scores, int32_t *out_ring, int64_t *stats,
                                      int64_t *ring_stats, void *workspace, size_t workspace_bytes, void *stream)
{
    return grid_interpolate_rings(data, N, K, inverse, voxel_data, voxel_K, neigh, voxel_cell, voxel_room, voxel_start, num_rooms,
                                  grid_stats, reinterpret_cast<const long long *>(voxel_scores), M, C, valid_labels, k, rings,
                                  out_labels, out_scores, out_ring, stats, ring_stats, workspace, workspace_bytes, stream);
}

int conv3p_grid_normals_f32(const float *voxel_data, int K, const int32_t *neigh, const int32_t *grid_stats,
                            const int32_t *voxel_room, const float *viewpoint, int64_t V, int64_t M, int min_neighbors,
                            float *normals, float *curvature, int32_t *samples, int32_t *flags, float *moments,
                            int32_t *normal_stats, void *stream)
{
    if (M < 0 || K < 3 || min_neighbors < kNormalsMinNeighbors || min_neighbors > kInterpNeigh) return CONV3P_ERR_INVALID_ARGUMENT;
    if (viewpoint && (V < 1 || (V != 1 && !voxel_room))) return CONV3P_ERR_INVALID_ARGUMENT;
    if (M == 0) return CONV3P_OK;
    if (!voxel_data || !neigh || !grid_stats || !normals || !curvature || !samples || !flags || !normal_stats)
        return CONV3P_ERR_INVALID_ARGUMENT;
    if (M > (int64_t)INT32_MAX || (viewpoint && V > (int64_t)INT32_MAX)) return CONV3P_ERR_UNSUPPORTED;   // neigh is int32
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(normal_stats, 0, 4 * sizeof(int32_t), s) != hipSuccess) return CONV3P_ERR_LAUNCH;
    const size_t work = ((size_t)M + kNormalsThreads - 1) / kNormalsThreads;
    hipLaunchKernelGGL(grid_normals_kernel, dim3(capped_grid(work, kNormalsMaxGrid)), dim3(kNormalsThreads), 0, s,
                       voxel_data, K, neigh, grid_stats, voxel_room, viewpoint, viewpoint ? (int)V : 0, (int)M, min_neighbors, normals, curvature, samples, flags, moments, normal_stats);
    return hip_ok();
}

size_t conv3p_grid_segments_workspace_bytes(int64_t M)
{
    int32_t *tile_count, *lab, *parent;
    if (M <= 0 || M > (int64_t)INT32_MAX) return 0;
    return carve_gseg(nullptr, M, tile_count, lab, parent);
}

int conv3p_grid_segments(const int32_t *neigh, const int32_t *voxel_labels, int64_t L, const int32_t *voxel_count,
                         const int32_t *grid_stats, int64_t M, int num_class, int connectivity, int32_t *segment,
                         int32_t *seg_root, int32_t *seg_size, int32_t *seg_rows, int32_t *seg_label, int32_t *seg_stats,
                         void *workspace, size_t workspace_bytes, void *stream)
{
    return gseg_run(nullptr, neigh, voxel_labels, L, voxel_count, grid_stats, M, num_class, connectivity, segment, seg_root,
                    seg_size, seg_rows, seg_label, seg_stats, workspace, workspace_bytes, stream);
}

int conv3p_grid_segments_smooth(const int32_t *neigh, const int32_t *voxel_labels, int64_t L, const int32_t *voxel_count,
                                const int32_t *grid_stats, int64_t M, int num_class, int connectivity, int32_t *segment,
                                int32_t *seg_root, int32_t *seg_size, int32_t *seg_rows, int32_t *seg_label,
                                int32_t *seg_stats, const float *normals, const int32_t *normal_flags, const float *curvature,
                                float min_cos, int signed_normals, float max_curvature, const float *features, int F,
                                int64_t feature_stride, float max_difference, int64_t *smooth_stats, void *workspace,
                                size_t workspace_bytes, void *stream)
{
    SmoothJoin rule{};                                   // the counters 0
    rule.normals = normals; rule.flags = normal_flags; rule.curvature = curvature; rule.features = features;
    rule.F = F; rule.feature_stride = (long long)feature_stride;
    rule.min_cos = min_cos; rule.max_curvature = max_curvature; rule.max_difference = max_difference;
    rule.signed_normals = signed_normals;
    rule.stats = reinterpret_cast<unsigned long long *>(smooth_stats);
    return gseg_run(&rule, neigh, voxel_labels, L, voxel_count, grid_stats, M, num_class, connectivity, segment, seg_root,
                    seg_size, seg_rows, seg_label, seg_stats, workspace, workspace_bytes, stream);
}

size_t conv3p_grid_absorb_workspace_bytes(int64_t M)
{
    AbsorbArgs p;
    if (M <= 0 || M > (int64_t)INT32_MAX) return 0;
    return carve_absorb(nullptr, M, p);
}

int conv3p_grid_absorb_segments(const int32_t *neigh, const int32_t *voxel_labels, int64_t L, const int32_t *segment,
                                const int32_t *seg_size, const int32_t *seg_label, const int32_t *seg_stats,
                                const int32_t *grid_stats, int64_t M, int num_class, int connectivity, int min_size,
                                int drop_orphans, int32_t *labels_out, int32_t *seg_label_out, int64_t *absorb_stats,
                                void *workspace, size_t workspace_bytes, void *stream)
{
    const unsigned tapmask = gseg_tapmask(connectivity);
    if (M < 0 || (voxel_labels && (L < 0 || L > M)) || num_class < 1 || num_class > kGsegMaxClass || !tapmask || min_size < 1 ||
        (drop_orphans != 0 && drop_orphans != 1))
        return CONV3P_ERR_INVALID_ARGUMENT;
    if (M == 0) return CONV3P_OK;
    if (!neigh || !segment || !seg_size || !seg_label || !seg_stats || !grid_stats || !labels_out || !seg_label_out ||
        !absorb_stats)
        return CONV3P_ERR_INVALID_ARGUMENT;
    if (M > (int64_t)INT32_MAX) return CONV3P_ERR_UNSUPPORTED;
    AbsorbArgs p{};
    const size_t need = carve_absorb(workspace, M, p);
    if (!workspace || workspace_bytes < need) return CONV3P_ERR_INVALID_ARGUMENT;
    hipStream_t s = static_cast<hipStream_t>(stream);
    p.neigh = neigh; p.voxel_labels = voxel_labels; p.segment = segment; p.seg_size = seg_size; p.seg_label = seg_label;
    p.seg_stats = seg_stats; p.grid_stats = grid_stats;
    p.L = voxel_labels ? (int)L : 0; p.M = (int)M; p.num_class = voxel_labels ? num_class : 1; p.min_size = min_size;
    p.drop_orphans = drop_orphans; p.ntiles = (int)gseg_tiles(M); p.tapmask = tapmask;
    p.labels_out = labels_out; p.seg_label_out = seg_label_out;
    p.stats = reinterpret_cast<unsigned long long *>(absorb_stats);
    const unsigned per_thread = gseg_grid(((size_t)M + kGsegThreads - 1) / kGsegThreads), per_tile = gseg_grid((size_t)p.ntiles);
    hipLaunchKernelGGL(absorb_count_kernel, dim3(per_tile), dim3(kGsegThreads), 0, s, p);
    hipLaunchKernelGGL(gseg_scan_kernel, dim3(1), dim3(kGsegScanThreads), 0, s, p.tile_small, p.tile_members, p.ntiles, p.hdr,
                       p.hdr + 1);
    hipLaunchKernelGGL(absorb_plan_kernel, dim3(per_tile), dim3(kGsegThreads), 0, s, p);
    hipLaunchKernelGGL(absorb_scatter_kernel, dim3(per_thread), dim3(kGsegThreads), 0, s, p);
    hipLaunchKernelGGL(absorb_vote_kernel, dim3(gseg_grid(((size_t)M + kGsegThreads / 64 - 1) / (kGsegThreads / 64))),
                       dim3(kGsegThreads), 0, s, p);      // a wave per small segment, and there are at most M
    hipLaunchKernelGGL(absorb_labels_kernel, dim3(per_thread), dim3(kGsegThreads), 0, s, p);
    return hip_ok();
}

// Every status first, in the order include/conv3p.h gives; then six launches whatever the data, and no workspace: the
// accumulators are the output words (conv3p_grid_geometry.hpp).
int conv3p_grid_segment_geometry(const float *voxel_data, int K, const int32_t *voxel_cell, const int32_t *voxel_count,
                                 const int32_t *segment, const int32_t *seg_stats, const int32_t *grid_stats, int64_t M,
                                 int weight, int32_t *cell_box, float *box, int64_t *moments, double *centroid,
                                 double *eigenvalues, double *axes, double *extent, int32_t *geometry_stats, void *stream)
{
    if (M < 0 || K < 3 || (weight != 0 && weight != 1)) return CONV3P_ERR_INVALID_ARGUMENT;
    if (M == 0) return CONV3P_OK;
    if (!voxel_data || !voxel_cell || !voxel_count || !segment || !seg_stats || !grid_stats || !cell_box || !box || !moments ||
        !centroid || !eigenvalues || !axes || !extent || !geometry_stats)
        return CONV3P_ERR_INVALID_ARGUMENT;
    if (M > (int64_t)INT32_MAX || K > 65536) return CONV3P_ERR_UNSUPPORTED;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int m = (int)M;
    const unsigned per_thread = gseg_grid(((size_t)M + kGsegThreads - 1) / kGsegThreads);
    // consecutive voxels a wave, as the segments' size adds take them
    const int steps = M >= (1 << 20) ? 16 : (M >= (1 << 16) ? 4 : 1);
    const size_t per_wave = (size_t)64 * steps * (kGsegThreads / 64);
    const unsigned per_chunk = gseg_grid(((size_t)M + per_wave - 1) / per_wave);
    int32_t *box_key = reinterpret_cast<int32_t *>(box);
    long long *mom = reinterpret_cast<long long *>(moments), *extent_key = reinterpret_cast<long long *>(extent);
    hipLaunchKernelGGL(geom_init_kernel, dim3(per_thread), dim3(kGsegThreads), 0, s, m, cell_box, box_key,
                       reinterpret_cast<unsigned long long *>(moments), extent_key, geometry_stats);
    hipLaunchKernelGGL(geom_box_kernel, dim3(per_chunk), dim3(kGsegThreads), 0, s, voxel_data, K, voxel_cell, segment, seg_stats,
                       grid_stats, m, steps, cell_box, box_key);
    hipLaunchKernelGGL(geom_moments_kernel, dim3(per_chunk), dim3(kGsegThreads), 0, s, voxel_cell, voxel_count, segment,
                       seg_stats, grid_stats, m, weight, steps, cell_box, reinterpret_cast<unsigned long long *>(moments));
    hipLaunchKernelGGL(geom_frame_kernel, dim3(per_thread), dim3(kGsegThreads), 0, s, seg_stats, m, cell_box, mom, centroid,
                       eigenvalues, axes, geometry_stats);
    hipLaunchKernelGGL(geom_extent_kernel, dim3(per_chunk), dim3(kGsegThreads), 0, s, voxel_cell, segment, seg_stats, grid_stats,
                       m, steps, centroid, axes, extent_key);
    hipLaunchKernelGGL(geom_finish_kernel, dim3(per_thread), dim3(kGsegThreads), 0, s, seg_stats, m, cell_box, box_key, mom,
                       extent_key, geometry_stats);
    return hip_ok();
}

int conv3p_grid_segment_pool_f32(const float *values, int64_t L, int C, int64_t value_stride, const int32_t *segment,
                                 const int32_t *seg_stats, const int32_t *voxel_count, const int32_t *grid_stats, int64_t M,
                                 int weight, int64_t *sums, int64_t *weights, double *mean, int32_t *seg_label,
                                 int32_t *voxel_label, int64_t *pool_stats, void *stream)
{
    return grid_segment_pool(values, L, C, value_stride, segment, seg_stats, voxel_count, grid_stats, M, weight, true, sums,
                             weights, mean, seg_label, voxel_label, pool_stats, stream);
}

int conv3p_grid_segment_pool_i64(const int64_t *values, int64_t L, int C, int64_t value_stride, const int32_t *segment,
                                 const int32_t *seg_stats, const int32_t *voxel_count, const int32_t *grid_stats, int64_t M,
                                 int weight, int64_t *sums, int64_t *weights, double *mean, int32_t *seg_label,
                                 int32_t *voxel_label, int64_t *pool_stats, void *stream)
{
    return grid_segment_pool(reinterpret_cast<const long long *>(values), L, C, value_stride, segment, seg_stats, voxel_count,
                             grid_stats, M, weight, false, sums, weights, mean, seg_label, voxel_label, pool_stats, stream);
}

size_t conv3p_grid_adjacency_scratch_bytes(int64_t M, int64_t max_edges)
{
    AdjArgs p;
    if (M <= 0 || M > (int64_t)INT32_MAX || max_edges < 0 || max_edges > (int64_t)INT32_MAX) return 0;
    return carve_adj(nullptr, max_edges, p);
}

// Every status first, in the order include/conv3p.h gives; then 5 + 6 b launches, b the bytes of M - 1: fixed by M.
int conv3p_grid_segment_adjacency(const int32_t *neigh, const int32_t *segment, const int32_t *seg_stats,
                                  const int32_t *grid_stats, int64_t M, int connectivity, int64_t max_edges,
                                  int32_t *adj_start, int32_t *edge_src, int32_t *edge_dst, int32_t *edge_contacts,
                                  int32_t *edge_voxels, int32_t *edge_offset, int32_t *edge_twin, int32_t *seg_border,
                                  int64_t *adj_stats, void *workspace, size_t workspace_bytes, void *stream)
{
    const unsigned tapmask = gseg_tapmask(connectivity);
    if (M < 0 || !tapmask || max_edges < 0) return CONV3P_ERR_INVALID_ARGUMENT;
    if (M == 0) return CONV3P_OK;
    if (!neigh || !segment || !seg_stats || !grid_stats || !adj_start || !seg_border || !adj_stats)
        return CONV3P_ERR_INVALID_ARGUMENT;
    if (max_edges > 0 && (!edge_src || !edge_dst || !edge_contacts || !edge_voxels || !edge_offset || !edge_twin))
        return CONV3P_ERR_INVALID_ARGUMENT;
    if (M > (int64_t)INT32_MAX || max_edges > (int64_t)INT32_MAX) return CONV3P_ERR_UNSUPPORTED;
    AdjArgs p{};
    const size_t need = carve_adj(workspace, max_edges, p);
    if (!workspace || workspace_bytes < need) return CONV3P_ERR_INVALID_ARGUMENT;
    hipStream_t s = static_cast<hipStream_t>(stream);
    p.neigh = neigh; p.segment = segment; p.seg_stats = seg_stats; p.grid_stats = grid_stats;
    p.M = (int)M; p.max_edges = (int)max_edges; p.tapmask = tapmask;
    p.adj_start = adj_start; p.edge_src = edge_src; p.edge_dst = edge_dst; p.edge_contacts = edge_contacts;
    p.edge_voxels = edge_voxels; p.edge_offset = edge_offset; p.edge_twin = edge_twin; p.seg_border = seg_border;
    p.adj_stats = reinterpret_cast<long long *>(adj_stats);
    const size_t cells = std::max((size_t)p.slots * kAdjVals, (size_t)M * 4);
    const unsigned per_cell = capped_grid((cells + kAdjThreads - 1) / kAdjThreads, kAdjMaxGrid);
    const unsigned per_voxel = capped_grid(((size_t)M + kAdjThreads - 1) / kAdjThreads, kAdjMaxGrid);
    hipLaunchKernelGGL(adj_init_kernel, dim3(per_cell), dim3(kAdjThreads), 0, s, p);
    hipLaunchKernelGGL(adj_walk_kernel, dim3(per_voxel), dim3(kAdjThreads), 0, s, p);
    adj_order_launch(p, s);
    hipLaunchKernelGGL(adj_stats_kernel, dim3(1), dim3(64), 0, s, p);
    return hip_ok();
}

size_t conv3p_grid_merge_scratch_bytes(int64_t M)
{
    MergeArgs p;
    if (M <= 0 || M > (int64_t)INT32_MAX) return 0;
    return carve_merge(nullptr, M, p);
}

// Every status first, in the order include/conv3p.h gives; then seven launches whatever the data.
int conv3p_grid_merge_segments(const int32_t *segment, const int32_t *seg_root, const int32_t *seg_size,
                               const int32_t *seg_rows, const int32_t *seg_label, const int32_t *seg_stats,
                               const int32_t *pair_a, const int32_t *pair_b, const int32_t *select, int64_t P, int64_t M,
                               int32_t *seg_map, int32_t *segment_out, int32_t *root_out, int32_t *size_out,
                               int32_t *rows_out, int32_t *label_out, int32_t *stats_out, int32_t *merge_stats,
                               void *workspace, size_t workspace_bytes, void *stream)
{
    if (M < 0 || P < 0) return CONV3P_ERR_INVALID_ARGUMENT;
    if (M == 0) return CONV3P_OK;
    if (!segment || !seg_root || !seg_size || !seg_rows || !seg_label || !seg_stats || !seg_map || !segment_out || !root_out ||
        !size_out || !rows_out || !label_out || !stats_out || !merge_stats || (P > 0 && (!pair_a || !pair_b)))
        return CONV3P_ERR_INVALID_ARGUMENT;
    if (M > (int64_t)INT32_MAX || P > (int64_t)INT32_MAX) return CONV3P_ERR_UNSUPPORTED;
    MergeArgs p{};
    const size_t need = carve_merge(workspace, M, p);
    if (!workspace || workspace_bytes < need) return CONV3P_ERR_INVALID_ARGUMENT;
    hipStream_t s = static_cast<hipStream_t>(stream);
    p.segment = segment; p.seg_root = seg_root; p.seg_size = seg_size; p.seg_rows = seg_rows; p.seg_label = seg_label;
    p.seg_stats = seg_stats; p.pair_a = pair_a; p.pair_b = pair_b; p.select = select; p.P = (long long)P;
    p.M = (int)M; p.ntiles = (int)gseg_tiles(M);
    p.seg_map = seg_map; p.segment_out = segment_out; p.root_out = root_out; p.size_out = size_out; p.rows_out = rows_out;
    p.label_out = label_out; p.stats_out = stats_out; p.merge_stats = merge_stats;
    merge_launch(p, s);
    return hip_ok();
}

size_t conv3p_grid_agglomerate_scratch_bytes(int64_t M, int64_t max_edges)
{
    AggArgs p;
    MergeArgs m;
    if (M <= 0 || M > (int64_t)INT32_MAX || max_edges < 0 || max_edges > (int64_t)INT32_MAX) return 0;
    return carve_agg(nullptr, M, max_edges, p, m);
}

// Every status first, in the order include/conv3p_graph.h gives; then 15 + 6 max_rounds + 6 b launches, b the bytes of
// M - 1: fixed by (M, max_rounds).
int conv3p_grid_agglomerate_segments(const int32_t *segment, const int32_t *seg_root, const int32_t *seg_size,
                                     const int32_t *seg_rows, const int32_t *seg_label, const int32_t *seg_stats,
                                     const int32_t *adj_start, const int32_t *edge_src, const int32_t *edge_dst,
                                     const int32_t *edge_contacts, const int32_t *edge_offset, const int64_t *adj_stats,
                                     int64_t M, int64_t max_edges, int min_size, int weight, int same_label,
                                     int min_contacts, int max_rounds, int32_t *log_a, int32_t *log_b, int32_t *log_round,
                                     int32_t *log_contacts, int32_t *seg_map, int32_t *segment_out, int32_t *root_out,
                                     int32_t *size_out, int32_t *rows_out, int32_t *label_out, int32_t *stats_out,
                                     int32_t *merge_stats, int32_t *voxel_label, int32_t *start_out, int32_t *src_out,
                                     int32_t *dst_out, int32_t *contacts_out, int32_t *offset_out, int32_t *twin_out,
                                     int64_t *agg_stats, void *workspace, size_t workspace_bytes, void *stream)
{
    if (M < 0 || max_edges < 0 || min_size < 1 || (weight != 0 && weight != 1) || (same_label != 0 && same_label != 1) ||
        min_contacts < 1 || max_rounds < 1 || max_rounds > kAggMaxRounds)
        return CONV3P_ERR_INVALID_ARGUMENT;
    if (M == 0) return CONV3P_OK;
    if (!segment || !seg_root || !seg_size || !seg_rows || !seg_label || !seg_stats || !adj_start || !adj_stats || !log_a ||
        !log_b || !log_round || !log_contacts || !seg_map || !segment_out || !root_out || !size_out || !rows_out ||
        !label_out || !stats_out || !merge_stats || !voxel_label || !start_out || !agg_stats)
        return CONV3P_ERR_INVALID_ARGUMENT;
    if (max_edges > 0 && (!edge_src || !edge_dst || !edge_contacts || !edge_offset || !src_out || !dst_out || !contacts_out ||
                          !offset_out || !twin_out))
        return CONV3P_ERR_INVALID_ARGUMENT;
    if (M > (int64_t)INT32_MAX || max_edges > (int64_t)INT32_MAX) return CONV3P_ERR_UNSUPPORTED;
    AggArgs p{};
    MergeArgs m{};
    const size_t need = carve_agg(workspace, M, max_edges, p, m);
    if (!workspace || workspace_bytes < need) return CONV3P_ERR_INVALID_ARGUMENT;
    hipStream_t s = static_cast<hipStream_t>(stream);
    p.seg_size = seg_size; p.seg_rows = seg_rows; p.seg_label = seg_label; p.seg_stats = seg_stats;
    p.edge_src = edge_src; p.edge_dst = edge_dst; p.edge_contacts = edge_contacts; p.edge_offset = edge_offset;
    p.adj_stats = reinterpret_cast<const long long *>(adj_stats);
    p.M = (int)M; p.ntiles = (int)gseg_tiles(M); p.min_size = min_size; p.weight = weight; p.same_label = same_label;
    p.min_contacts = min_contacts;
    p.log_a = log_a; p.log_b = log_b; p.log_round = log_round; p.log_contacts = log_contacts;
    p.seg_map = seg_map; p.segment_out = segment_out; p.label_out = label_out; p.stats_out = stats_out;
    p.voxel_label = voxel_label; p.agg_stats = reinterpret_cast<long long *>(agg_stats);
    p.t.seg_stats = stats_out;                           // the contracted graph is over the result's groups
    p.t.M = (int)M; p.t.max_edges = (int)max_edges;
    p.t.adj_start = start_out; p.t.edge_src = src_out; p.t.edge_dst = dst_out; p.t.edge_contacts = contacts_out;
    p.t.edge_offset = offset_out; p.t.edge_twin = twin_out;
    m.segment = segment; m.seg_root = seg_root; m.seg_size = seg_size; m.seg_rows = seg_rows; m.seg_label = seg_label;
    m.seg_stats = seg_stats; m.pair_a = log_a; m.pair_b = log_b; m.select = nullptr; m.P = (long long)M;
    m.M = (int)M; m.ntiles = p.ntiles;
    m.seg_map = seg_map; m.segment_out = segment_out; m.root_out = root_out; m.size_out = size_out; m.rows_out = rows_out;
    m.label_out = label_out; m.stats_out = stats_out; m.merge_stats = merge_stats;
    const size_t cells = std::max((size_t)p.t.slots * kAdjVals, (size_t)M);
    const dim3 per_cell(capped_grid((cells + kAdjThreads - 1) / kAdjThreads, kAdjMaxGrid)), threads(kAdjThreads);
    const dim3 per_edge(capped_grid(((size_t)std::max<int64_t>(max_edges, 1) + kAdjThreads - 1) / kAdjThreads, kAdjMaxGrid));
    const dim3 per_slot(capped_grid(((size_t)p.t.slots + kAdjThreads - 1) / kAdjThreads, kAdjMaxGrid));
    const dim3 per_tile(gseg_grid((size_t)p.ntiles)), per_voxel(gseg_grid(((size_t)M + kGsegThreads - 1) / kGsegThreads));
    hipLaunchKernelGGL(agg_init_kernel, per_cell, threads, 0, s, p);
    for (int round = 0; round <= max_rounds; ++round) {  // the last one only chooses, for agg_stats[4:6]
        hipLaunchKernelGGL(agg_contract_kernel, per_edge, threads, 0, s, p, static_cast<const int32_t *>(p.grp), 0);
        hipLaunchKernelGGL(agg_choose_kernel, per_slot, threads, 0, s, p);
        if (round == max_rounds) break;
        hipLaunchKernelGGL(agg_count_kernel, per_tile, dim3(kGsegThreads), 0, s, p);
        hipLaunchKernelGGL(agg_scan_kernel, dim3(1), dim3(kGsegScanThreads), 0, s, p);
        hipLaunchKernelGGL(agg_log_kernel, per_tile, dim3(kGsegThreads), 0, s, p, round);
        hipLaunchKernelGGL(agg_flatten_kernel, per_cell, threads, 0, s, p);
    }
    hipLaunchKernelGGL(agg_census_kernel, per_cell, threads, 0, s, p);
    merge_launch(m, s);
    hipLaunchKernelGGL(agg_contract_kernel, per_edge, threads, 0, s, p, static_cast<const int32_t *>(seg_map), 1);
    adj_order_launch(p.t, s);
    hipLaunchKernelGGL(agg_finish_kernel, per_voxel, dim3(kGsegThreads), 0, s, p);
    return hip_ok();
}

size_t conv3p_grid_subsample_rooms_workspace_bytes(int64_t N, int64_t R, int max_voxels)
{
    GridPlan w;
    GridRoomsArgs a;
    return grid_rooms_plan(N, R, max_voxels, w) ? carve_grid_rooms(nullptr, w, N, R, a) : 0;
}

// Every status first, in the order include/conv3p.h gives; then the launches, their number fixed by mode alone.
int conv3p_grid_subsample_rooms_f32(const float *data, const void *labels, const int32_t *room_start, int64_t N, int64_t R,
                                    int K, int label_bytes, float voxel, int mode, int num_class, int max_voxels,
                                    float *out, int32_t *labels_out, int32_t *voxel_row, int32_t *voxel_count,
                                    int32_t *voxel_cell, int32_t *voxel_room, int32_t *voxel_start, int32_t *inverse,
                                    int32_t *room_stats, int32_t *stats, void *workspace, size_t workspace_bytes,
                                    void *stream)
{
    if (N < 0 || R < 0 || K < 3 || max_voxels < 0 || (mode != 0 && mode != 1)) return CONV3P_ERR_INVALID_ARGUMENT;
    if (!std::isfinite(voxel) || !(voxel > 0.0f)) return CONV3P_ERR_INVALID_ARGUMENT;
    if ((labels != nullptr) != (labels_out != nullptr)) return CONV3P_ERR_INVALID_ARGUMENT;
    if (labels && label_bytes != 1 && label_bytes != 4 && label_bytes != 8) return CONV3P_ERR_INVALID_ARGUMENT;
    const bool votes = labels && mode == 0;              // num_class is read by the majority only
    if (votes && num_class < 1) return CONV3P_ERR_INVALID_ARGUMENT;
    if (R == 0 || N == 0 || max_voxels == 0) return CONV3P_OK;
    if (!data || !room_start || !out || !voxel_row || !voxel_count || !voxel_cell || !voxel_room || !voxel_start ||
        !inverse || !room_stats || !stats)
        return CONV3P_ERR_INVALID_ARGUMENT;
    if (N > kGridMaxN || R > kGridRoomsMaxRooms || K > 65536 || (votes && num_class > kGridMaxClass))
        return CONV3P_ERR_UNSUPPORTED;
    GridPlan w;
    if (!grid_rooms_plan(N, R, max_voxels, w)) return CONV3P_ERR_UNSUPPORTED;
    GridRoomsArgs a;
    TRY(buf_check(workspace, workspace_bytes, carve_grid_rooms(workspace, w, N, R, a)));
    const GridArgs &g = a.g;
    grid_fill(a.g, data, labels, N, K, label_bytes, voxel, mode, num_class, max_voxels, out, labels_out, voxel_row, voxel_count,
              voxel_cell, inverse, stats);
    a.room_start = room_start; a.R = (int)R;
    a.voxel_room = voxel_room; a.voxel_start = voxel_start; a.room_stats = room_stats;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const unsigned tgrid = (unsigned)w.row_tiles, rgrid = capped_grid((size_t)R, kSceneMaxGrid);
    hipLaunchKernelGGL(grid_rooms_check_kernel, dim3(1), dim3(kGridScanThreads), 0, s, a);
    hipLaunchKernelGGL(grid_rooms_bounds_kernel, dim3(tgrid), dim3(kSceneThreads), 0, s, a);
    hipLaunchKernelGGL(grid_rooms_frame_kernel, dim3(rgrid), dim3(kSceneThreads), 0, s, a);
    hipLaunchKernelGGL(grid_rooms_base_kernel, dim3(1), dim3(kGridScanThreads), 0, s, a);
    hipLaunchKernelGGL(grid_rooms_pairs_kernel, dim3(tgrid), dim3(kSceneThreads), 0, s, a);
    grid_sort_launch(g, capped_grid((size_t)w.sort_tiles, kSceneMaxGrid), s);
    hipLaunchKernelGGL(grid_rooms_voxel_kernel, dim3((unsigned)w.voxel_grid), dim3(kSceneThreads), 0, s, a);
    if (mode == 0) hipLaunchKernelGGL(grid_mean_kernel, dim3(grid_mean_grid(max_voxels, K)), dim3(kSceneThreads), 0, s, g);
    hipLaunchKernelGGL(grid_rooms_count_max_kernel, dim3(tgrid), dim3(kSceneThreads), 0, s, a);
    hipLaunchKernelGGL(grid_rooms_out_kernel, dim3(capped_grid((size_t)(R + 3) / 4, kSceneMaxGrid)), dim3(kSceneThreads), 0, s, a);
    hipLaunchKernelGGL(grid_rooms_stats_kernel, dim3(1), dim3(kGridScanThreads), 0, s, a);
    return hip_ok();
}

}  // extern "C"
