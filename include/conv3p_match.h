/*
 * conv3p_match.h -- C ABI of the call that scores a segmentation against ground-truth instances (libconv3p_hip.so).  The
 * conventions, the status codes and the ABI version are conv3p.h's; the version stays 5, this header only adds symbols.
 * (A later maintenance change folds it into conv3p.h, together with the symbol table and the case tables of the tests,
 * and renames the two functions to the conv3p_ prefix)
 *
 * c3p_grid_match_segments:  the exact overlap table between predicted segments and true instances, the one-to-one
 *   matching at an IoU threshold, and the counters behind panoptic quality, precision / recall and coverage -- on the
 *   device, in integers, with no host read (pointwise_amd/csrc/conv3p_grid_match.hpp; tests/grid_match_ref.py restates it in
 *   numpy).  Inputs: segment int32 (M) and seg_stats of a segmentation numbered by S3 (conv3p_grid_segments, _smooth,
 *   conv3p_grid_merge_segments or the agglomeration), with S = min(max(seg_stats[0], 0), M) read ON THE DEVICE; the grid's
 *   inverse int32 (N) and grid_stats; truth int32, (N) with weight = 1 and (M) with weight = 0; T = num_truth,
 *   1 <= T <= 2^24; optionally pred_class int32 (M, a row per segment) and truth_class int32 (T) with num_class in
 *   [1, 128] -- both or neither; with neither, num_class must be 1 and every segment and instance has class 0; the
 *   threshold iou_num / iou_den with 1 <= iou_num < iou_den <= 32768 and 2 iou_num >= iou_den.
 *    M1.  UNITS.  weight = 1 (rows): a unit is a raw row r < N; its prediction is p = segment[inverse[r]], -1 when
 *         inverse[r] is outside [0, M) or the segment is outside [0, S); its truth is t = truth[r].  weight = 0 (voxels): a
 *         unit is a voxel v < min(max(grid_stats[0], 0), M); p = segment[v] (-1 outside [0, S)), t = truth[v].
 *    M2.  VOID.  A unit's truth is void when t == -1, when t is outside [-1, T) (counted as INVALID in the stats), or when
 *         truth_class[t] is outside [0, num_class) (an ignored category).  Void units enter no pair and no truth size.
 *    M3.  SIZES, int32, exact whatever happens later: pred_size[p] (M) = the units of p with non-void truth; pred_void[p]
 *         (M) = the units of p with void truth; truth_size[t] (T) = all units with non-void truth t, those with p = -1
 *         included; truth_missed[t] (T) = those of them with p = -1.
 *    M4.  THE TABLE.  One row per pair (p, t) with inter > 0 units, in ascending (p, t): pair_pred, pair_truth, pair_inter
 *         int32 (max_pairs); start int32 (M + 1), the CSR over p (start[p] = P for p >= S).  The transpose: t_start int32
 *         (T + 1) and t_pair int32 (max_pairs), the pair rows in ascending (t, p).  Rows past P hold -1, -1, 0, -1.
 *    M5.  OVERFLOW, as E7.  B = the units with p >= 0 and non-void truth is always computed, and P <= B.  If
 *         P > max_pairs: stats[0] = -1, every pair row is filler, start and t_start are all 0, every match / best output
 *         is -1 / 0, class_stats is 0 and the two coverage sums are 0.  The sizes of M3, B and the other counts of M10
 *         stay exact.  A retry with max_pairs = B always fits.
 *    M6.  union(p, t) = pred_size[p] + truth_size[t] - inter.  IoUs are compared exactly, by cross-multiplication; with
 *         M, N <= 2^24 every product is below 2^49.
 *    M7.  BEST PARTNERS, whatever the classes.  best_truth[p] (M) = the t of the row of p with the largest IoU, the
 *         lowest t on a tie, with best_truth_inter, best_truth_union; best_pred[t] (T) likewise, the lowest p on a tie,
 *         with best_pred_inter, best_pred_union; -1, 0, 0 where there is none.
 *    M8.  MATCHES.  (p, t) MATCH when class(p) == class(t), that class is in [0, num_class), and
 *         inter iou_den > iou_num union.  With 2 iou_num >= iou_den a match has IoU > 1/2, so inter > union / 2; the union
 *         is at least pred_size[p] and at least truth_size[t], so the pair holds more than half of the units of p and more
 *         than half of those of t: no second t can do that for p and no second p for t -- a match is unique on both
 *         sides.  Any other row (p, t') has inter' < pred_size[p] / 2 <= union' / 2, an IoU below 1/2: the match is the
 *         best partner of M7 of p, and by the same argument of t.  So pred_match[p] (M) is best_truth[p] where that pair
 *         passes, else -1; truth_match[t] (T) is best_pred[t] where it passes, else -1; the two agree.
 *         pred_iou_q30[p] int32 (M) = floor(inter 2^30 / union), 0 where unmatched: the 2^-30 fixed point of the scene
 *         scores.
 *    M9.  class_stats int64 (num_class, 6) = {TP, FP, FN, the sum of pred_iou_q30 over the TP, instances with
 *         truth_size > 0, segments with that class}.  A matched segment is a TP of its class.  An unmatched segment p < S
 *         whose class is in range is an FP, unless pred_void[p] > pred_size[p] (mostly on unannotated ground: ignored, the
 *         panoptic-quality rule); column 5 counts TP, FP and ignored.  A segment whose class is out of range is counted
 *         nowhere.  An unmatched instance with truth_size > 0 is an FN of its class.  Integer adds only.
 *    M10. stats int64 (16) = {P or -1, B, S, instances with truth_size > 0, void units, invalid truth ids (among the void),
 *         units with p = -1 and non-void truth, the overflow flag, coverage = the sum over the instances of
 *         floor(best_pred_inter 2^30 / best_pred_union), weighted coverage = the sum of truth_size times that (below
 *         2^54), the sum of truth_size, 0, 0, 0, 0, 0}.
 *   Status, in this order, all before any launch: M < 0, N < 0, T outside [1, 2^24], weight not 0 or 1, num_class outside
 *   [1, 128], exactly one of pred_class and truth_class NULL, both NULL with num_class != 1, iou_num < 1,
 *   iou_num >= iou_den, iou_den > 32768, 2 iou_num < iou_den, max_pairs < 0: CONV3P_ERR_INVALID_ARGUMENT; M == 0: CONV3P_OK,
 *   nothing launched and nothing written; any other pointer NULL (grid_stats may be NULL with weight = 1, inverse with
 *   weight = 0 or N == 0; pair_pred, pair_truth, pair_inter and t_pair with max_pairs == 0): CONV3P_ERR_INVALID_ARGUMENT;
 *   M or N > 2^24 or max_pairs > 2^31 - 1: CONV3P_ERR_UNSUPPORTED; workspace NULL or smaller than
 *   c3p_grid_match_scratch_bytes(M, N, T, max_pairs): CONV3P_ERR_INVALID_ARGUMENT.  With no units (N == 0) the same
 *   launches run: they define every output.
 *   The workspace is 56 bytes per row of max_pairs (the table of 2 max_pairs + 64 slots of a key and a count, and two key
 *   buffers for each of the two sorts) and some KiB: a function of its arguments alone, a multiple of 256, 0 for refused
 *   arguments (M < 1 included).
 *   8 + 9 b launches with b the bytes of max(M, T) - 1 (1 .. 4): fixed by (M, T) whatever the data.  No host read, no
 *   blocking upload, everything ordered on `stream`.  No float arithmetic; the only atomics are the 64-bit CAS that claims
 *   a slot and integer adds, each on its own word.  Every probe loop is bounded by the table's size and none waits for a
 *   thread or a workgroup.  Bitwise reproducible.
 */
#ifndef CONV3P_MATCH_H
#define CONV3P_MATCH_H

#include "conv3p.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t c3p_grid_match_scratch_bytes(int64_t M, int64_t N, int64_t T, int64_t max_pairs);
int c3p_grid_match_segments(const int32_t *segment, const int32_t *seg_stats, const int32_t *inverse,
                            const int32_t *grid_stats, const int32_t *truth, int64_t M, int64_t N, int64_t T, int weight,
                            const int32_t *pred_class, const int32_t *truth_class, int num_class, int iou_num, int iou_den,
                            int64_t max_pairs, int32_t *pred_size, int32_t *pred_void, int32_t *truth_size,
                            int32_t *truth_missed, int32_t *pair_pred, int32_t *pair_truth, int32_t *pair_inter,
                            int32_t *start, int32_t *t_start, int32_t *t_pair, int32_t *best_truth,
                            int32_t *best_truth_inter, int32_t *best_truth_union, int32_t *best_pred,
                            int32_t *best_pred_inter, int32_t *best_pred_union, int32_t *pred_match, int32_t *truth_match,
                            int32_t *pred_iou_q30, int64_t *class_stats, int64_t *stats, void *workspace,
                            size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CONV3P_MATCH_H */
