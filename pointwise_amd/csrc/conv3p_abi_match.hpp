// conv3p_abi_match.hpp -- host side of the segment matching (include/conv3p_match.h).  Included by conv3p_abi.hip behind
// conv3p_abi_grid.hpp, whose launches of the adjacency's sort it uses.
namespace {

// The matching's scratch: its counters, then the table of 2 max_pairs + 64 slots (a key and a count each), the radix
// passes' totals (one set per sort) and histograms, and two key buffers per sort.  A function of max_pairs alone: M, N
// and T only bound it.
size_t carve_match(void *ws, int64_t max_pairs, MatchArgs &p)
{
    Carver cv(ws);
    p.t.slots = p.u.slots = 2ull * (unsigned long long)max_pairs + kAdjSlack;
    p.t.sort_tiles = (int)(((size_t)max_pairs + kAdjSortTile - 1) / kAdjSortTile);
    if (p.t.sort_tiles < 1) p.t.sort_tiles = 1;
    p.u.sort_tiles = p.t.sort_tiles;
    p.hdr = cv.take<MatchHeader>(1);
    p.t.hdr = p.u.hdr = cv.take<AdjHeader>(1);
    p.t.digit_total = cv.take<int>((size_t)2 * kAdjMaxBytes * kAdjDigits);
    p.u.digit_total = cv.take<int>((size_t)2 * kAdjMaxBytes * kAdjDigits);
    p.t.hist = p.u.hist = cv.take<int>((size_t)p.t.sort_tiles * kAdjDigits);
    p.t.keys = p.u.keys = cv.take<unsigned long long>((size_t)p.t.slots);
    p.inter = cv.take<int32_t>((size_t)p.t.slots);
    p.t.sort_a = cv.take<unsigned long long>((size_t)max_pairs);
    p.t.sort_b = cv.take<unsigned long long>((size_t)max_pairs);
    p.u.sort_a = cv.take<unsigned long long>((size_t)max_pairs);
    p.u.sort_b = cv.take<unsigned long long>((size_t)max_pairs);
    return cv.bytes();
}

}  // namespace

extern "C" {

size_t c3p_grid_match_scratch_bytes(int64_t M, int64_t N, int64_t T, int64_t max_pairs)
{
    MatchArgs p{};
    if (M < 1 || M > kMatchMaxUnits || N < 0 || N > kMatchMaxUnits || T < 1 || T > kMatchMaxUnits || max_pairs < 0 ||
        max_pairs > (int64_t)INT32_MAX)
        return 0;
    return carve_match(nullptr, max_pairs, p);
}

// Every status first, in the order include/conv3p_match.h gives; then 8 + 9 b launches, b the bytes of max(M, T) - 1.
int c3p_grid_match_segments(const int32_t *segment, const int32_t *seg_stats, const int32_t *inverse, const int32_t *grid_stats,
                            const int32_t *truth, int64_t M, int64_t N, int64_t T, int weight, const int32_t *pred_class,
                            const int32_t *truth_class, int num_class, int iou_num, int iou_den, int64_t max_pairs,
                            int32_t *pred_size, int32_t *pred_void, int32_t *truth_size, int32_t *truth_missed,
                            int32_t *pair_pred, int32_t *pair_truth, int32_t *pair_inter, int32_t *start, int32_t *t_start,
                            int32_t *t_pair, int32_t *best_truth, int32_t *best_truth_inter, int32_t *best_truth_union,
                            int32_t *best_pred, int32_t *best_pred_inter, int32_t *best_pred_union, int32_t *pred_match,
                            int32_t *truth_match, int32_t *pred_iou_q30, int64_t *class_stats, int64_t *stats, void *workspace,
                            size_t workspace_bytes, void *stream)
{
    if (M < 0 || N < 0 || T < 1 || T > kMatchMaxUnits || (weight != 0 && weight != 1) || num_class < 1 ||
        num_class > kMatchMaxClass || (pred_class == nullptr) != (truth_class == nullptr) || (!pred_class && num_class != 1) ||
        iou_num < 1 || iou_num >= iou_den || iou_den > 32768 || 2 * iou_num < iou_den || max_pairs < 0)
        return CONV3P_ERR_INVALID_ARGUMENT;
    if (M == 0) return CONV3P_OK;
    if (!segment || !seg_stats || !truth || (weight == 0 ? !grid_stats : (N > 0 && !inverse)) || !pred_size || !pred_void ||
        !truth_size || !truth_missed || !start || !t_start || !best_truth || !best_truth_inter || !best_truth_union ||
        !best_pred || !best_pred_inter || !best_pred_union || !pred_match || !truth_match || !pred_iou_q30 || !class_stats ||
        !stats)
        return CONV3P_ERR_INVALID_ARGUMENT;
    if (max_pairs > 0 && (!pair_pred || !pair_truth || !pair_inter || !t_pair)) return CONV3P_ERR_INVALID_ARGUMENT;
    if (M > kMatchMaxUnits || N > kMatchMaxUnits || max_pairs > (int64_t)INT32_MAX) return CONV3P_ERR_UNSUPPORTED;
    MatchArgs p{};
    const size_t need = carve_match(workspace, max_pairs, p);
    if (!workspace || workspace_bytes < need) return CONV3P_ERR_INVALID_ARGUMENT;
    hipStream_t s = static_cast<hipStream_t>(stream);
    p.segment = segment; p.seg_stats = seg_stats; p.inverse = inverse; p.grid_stats = grid_stats; p.truth = truth;
    p.pred_class = pred_class; p.truth_class = truth_class;
    p.M = (int)M; p.N = (long long)N; p.T = (int)T; p.num_class = num_class; p.rows = weight; p.num = iou_num; p.den = iou_den;
    p.max_pairs = (int)max_pairs;
    p.pred_size = pred_size; p.pred_void = pred_void; p.truth_size = truth_size; p.truth_missed = truth_missed;
    p.pair_pred = pair_pred; p.pair_truth = pair_truth; p.pair_inter = pair_inter; p.start = start; p.t_start = t_start;
    p.t_pair = t_pair;
    p.best_truth = best_truth; p.best_truth_inter = best_truth_inter; p.best_truth_union = best_truth_union;
    p.best_pred = best_pred; p.best_pred_inter = best_pred_inter; p.best_pred_union = best_pred_union;
    p.pred_match = pred_match; p.truth_match = truth_match; p.pred_iou_q30 = pred_iou_q30;
    p.class_stats = reinterpret_cast<long long *>(class_stats);
    p.stats = reinterpret_cast<long long *>(stats);
    // the radix passes size their bytes by max(S, T), which match_init_kernel notes behind the counters
    const int64_t most = std::max(M, T);
    p.t.seg_stats = p.u.seg_stats = p.hdr->sort_count;
    p.t.M = p.u.M = (int)most;
    p.t.max_edges = p.u.max_edges = (int)max_pairs;
    const size_t units = weight ? (size_t)N : (size_t)M;
    const size_t cells = std::max(std::max((size_t)p.t.slots, (size_t)most), (size_t)max_pairs);
    auto grid_for = [](size_t work) {                   // at least one workgroup: the walk of no units still launches
        return dim3(capped_grid(std::max((work + kMatchThreads - 1) / kMatchThreads, (size_t)1), kMatchMaxGrid));
    };
    hipLaunchKernelGGL(match_init_kernel, grid_for(cells), dim3(kMatchThreads), 0, s, p);
    hipLaunchKernelGGL(match_walk_kernel, grid_for(units), dim3(kMatchThreads), 0, s, p);
    adj_sort_launch(p.t, s);
    hipLaunchKernelGGL(match_rows_kernel, grid_for(std::max((size_t)M + 1, (size_t)max_pairs)), dim3(kMatchThreads), 0, s, p);
    adj_passes_launch(p.u, 1, 2, adj_key_bytes(most), s);
    hipLaunchKernelGGL(match_transpose_kernel, grid_for(std::max((size_t)T + 1, (size_t)max_pairs)), dim3(kMatchThreads), 0, s, p);
    hipLaunchKernelGGL(match_pred_kernel, grid_for((size_t)M), dim3(kMatchThreads), 0, s, p);
    hipLaunchKernelGGL(match_truth_kernel, grid_for((size_t)T), dim3(kMatchThreads), 0, s, p);
    hipLaunchKernelGGL(match_stats_kernel, dim3(1), dim3(64), 0, s, p);
    return hip_ok();
}

}  // extern "C"
