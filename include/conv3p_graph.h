/*
 * conv3p_graph.h -- C ABI of the segment-graph calls that work on an adjacency instead of on the voxels
 * (libconv3p_hip.so).  The conventions, the status codes and the ABI version are conv3p.h's; the version stays 5, this
 * header only adds symbols.  (A later maintenance change folds it into conv3p.h, together with the symbol table and the
 * case tables of the tests)
 *
 * conv3p_grid_agglomerate_segments:  small groups of segments folded into the neighbour they touch most, round after
 *   round, until nothing small has a neighbour left or max_rounds is reached -- on the device, with no host read and
 *   no second walk over the voxels (pointwise_amd/csrc/conv3p_grid_agglomerate.hpp; tests/grid_agglomerate_ref.py restates
 *   it in numpy).  Inputs: segment, seg_root, seg_size, seg_rows, seg_label, seg_stats of a segmentation numbered by S3
 *   (conv3p_grid_segments, _smooth or conv3p_grid_merge_segments), and adj_start, edge_src, edge_dst, edge_contacts,
 *   edge_offset, adj_stats as conv3p_grid_segment_adjacency wrote them for it, with max_edges rows.  Everything is
 *   int32 / int64 and defined bit for bit.
 *    H1.  S = min(max(seg_stats[0], 0), M) and E = adj_stats[0], both read ON THE DEVICE.  If E < 0 (the adjacency
 *         overflowed, E7) or E > max_edges the input is UNUSABLE: no round runs, the result is the identity of U5, the log
 *         is empty, every row of the contracted graph is filler and start_out is all 0 (as E7 on overflow),
 *         agg_stats[6] = 1, agg_stats[5] = agg_stats[7] = 0.  Edge rows at or past E are not read; rows with src or dst
 *         outside [0, S) are ignored.
 *    H2.  The state is a partition of the segments 0 .. S-1 into GROUPS; at the start every segment is its own group.
 *         The root segment of a group is its lowest number.  W(g) is the sum over the members of seg_size (weight = 0) or
 *         of seg_rows (weight = 1).  L(g) is the seg_label of the member with the largest seg_size, the lowest number on a
 *         tie: U3's rule, on seg_size whatever weight is.  C(g, h) is the sum of edge_contacts over the edges (a, b) with
 *         a in g and b in h; symmetric by E4.
 *    H3.  g is SMALL when W(g) < min_size.  h != g is a CANDIDATE of g when C(g, h) >= min_contacts (min_contacts >= 1)
 *         and, with same_label != 0, L(g) == L(h).
 *    H4.  Every small group with a candidate PROPOSES to the candidate with the largest key, compared left to right:
 *         (h is not small, C(g, h), the lowest root segment wins).  As 64 bits:
 *         flag << 62 | C << 31 | (0x7fffffff - root).
 *    H5.  A ROUND takes all proposals of the state at its start and joins them transitively.  A round with no proposal
 *         ends the rounds: the fixed point.  At most max_rounds rounds run.
 *    H6.  The LOG, int32 (M) each.  Every proposal of round k (from 0) is a row (log_a, log_b, log_round, log_contacts) =
 *         (root(g), root(h), k, C(g, h)), except that of a MUTUAL pair -- h also proposed to g -- which is logged once, by
 *         the lower root.  Rows are in ascending (round, log_a); rows past P hold -1, -1, -1, 0.  Proposal cycles longer
 *         than 2 cannot occur: among small groups the key is symmetric and ties go to the lowest number, and a group that
 *         is not small does not propose.  So the log is a spanning forest and P = S - S' exactly.
 *    H7.  The result segmentation -- seg_map, segment_out, root_out, size_out, rows_out, label_out, stats_out and
 *         merge_stats = {S', S, P, groups of more than one segment} -- is, to the bit, what conv3p_grid_merge_segments
 *         gives on (log_a, log_b).  voxel_label int32 (M): label_out[segment_out[v]], -1 outside every segment.
 *    H8.  The CONTRACTED GRAPH over the result's groups: start_out int32 (M + 1); src_out, dst_out, contacts_out,
 *         twin_out int32 (max_edges), offset_out int32 (max_edges, 3); order and filler as E4 / E5.  Contacts and offsets
 *         are the sums over the input edges that now run between two different groups.  These six arrays equal what
 *         conv3p_grid_segment_adjacency writes for the result at the connectivity of the input adjacency.  edge_voxels
 *         and seg_border[:, 3] are NOT produced: a voxel that touched two segments of one group counts once, so they are
 *         not additive under a merge; run the adjacency call on the result for them
 *         (result.segments.adjacency() in Python).
 *    H9.  agg_stats int64 (8) = {S', S, rounds that had a proposal, P, small groups at the end, of those the ones that
 *         still have a candidate (0: the fixed point was reached), input unusable (H1), E' = the directed edges of the
 *         contracted graph}.
 *    H10. With nothing small (min_size = 1) every output is the identity of U5 and the contracted graph is the input
 *         graph.  A run with max_rounds = k equals conv3p_grid_merge_segments on the rows with log_round < k of any
 *         longer run.
 *   Status, in this order, all before any launch: M < 0, max_edges < 0, min_size < 1, weight not 0 or 1, same_label not 0
 *   or 1, min_contacts < 1, max_rounds outside [1, 32]: CONV3P_ERR_INVALID_ARGUMENT; M == 0: CONV3P_OK, nothing launched;
 *   any pointer NULL (the four input edge arrays and src_out, dst_out, contacts_out, offset_out, twin_out may be NULL
 *   with max_edges == 0): CONV3P_ERR_INVALID_ARGUMENT; M or max_edges > 2^31 - 1: CONV3P_ERR_UNSUPPORTED; workspace NULL or
 *   smaller than conv3p_grid_agglomerate_scratch_bytes(M, max_edges): CONV3P_ERR_INVALID_ARGUMENT.
 *   The workspace is the adjacency call's (18 words per row of max_edges: the table of 2 max_edges + 64 slots and the two
 *   key buffers) plus a word per row of max_edges, the merge call's (5 M words) plus 6 M words of group state, two words
 *   per 2048 segments and a few KiB: a function of (M, max_edges) alone, a multiple of 256, 0 for refused arguments.
 *   15 + 6 max_rounds + 6 b launches with b the bytes of M - 1 (1 .. 4): fixed by (M, max_rounds) whatever the data.  A
 *   `done` word on the device is set by the first round without a proposal; every kernel of every later round returns at
 *   once.  A round costs the E input edges and the table's slots, never the 26 M taps.  No host read; no float
 *   arithmetic; the only atomics are the 64-bit CAS that claims a slot, int32 adds, the int32 CAS / min of the
 *   union-find and 64-bit maxima, each on its own word.  The table cannot fill: the combined edges never exceed
 *   E <= max_edges.  Every probe loop is bounded by the table's size and none waits for a thread or a workgroup.
 *   Bitwise reproducible.
 */
#ifndef CONV3P_GRAPH_H
#define CONV3P_GRAPH_H

#include "conv3p.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t conv3p_grid_agglomerate_scratch_bytes(int64_t M, int64_t max_edges);
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
                                     int64_t *agg_stats, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CONV3P_GRAPH_H */
