/*
 * conv3p_knn.h -- C ABI of the exact k-nearest-voxel search on the voxel grid and of its two consumers
 * (libconv3p_hip.so).  The conventions, the status codes and the ABI version are conv3p.h's; the version stays 5, this
 * header only adds symbols.  (A later maintenance change folds it into conv3p.h, together with the symbol table and the
 * case tables of the tests, as it does conv3p_graph.h.)
 *
 * conv3p_grid_knn_f32:  for every query the k nearest voxel representatives among the cells within Chebyshev distance
 *   `rings` of the query's own cell, in ascending (d2, voxel) -- and a proof, per query, of whether those are the k
 *   nearest of the whole room (pointwise_amd/csrc/conv3p_grid_knn.hpp; tests/grid_knn_ref.py restates it in numpy).  The
 *   ring call of conv3p.h stops at the first cube that is not empty because no floating-point bound on where a
 *   representative can lie was at hand: a float32 mean chain can leave its cell, and a caller may rewrite voxel_data.
 *   This call MEASURES that bound on the device (K5) instead of assuming it, so its stopping test (K6) is conservative
 *   for any voxel_data (K7).
 *   query float32, Q rows, row stride query_stride >= 3 floats, xyz first; query_voxel int32 (Q), the voxel whose cell
 *   the query lies in (a raw row's inverse), or NULL: v0 = i, the voxels query themselves, which needs Q <= M and
 *   query = voxel_data.  voxel_data (>= M, voxel_K), neigh (>= M, 27) as conv3p_grid_neighbors writes it, voxel_cell
 *   (>= M, 3), voxel_room (>= M) and voxel_start (num_rooms + 1) -- both or neither -- and grid_stats are the
 *   subsampling's; ne = min(max(grid_stats[0], 0), M) is read ON THE DEVICE.  valid int32 (M) or NULL.  voxel is the
 *   lattice step h the subsampling was given: a hint, never a correctness input (K7).  k in [1, 16], rings = R in [1, 8],
 *   exclude_self 0 or 1.  Every float32 step is one separately rounded operation (the library is built with
 *   -ffp-contract=off), every float64 step likewise.  For query i, with q = query[i][0..2] and v0 its voxel:
 *    K1. The query is LIVE when 0 <= v0 < ne and q_x, q_y, q_z are finite.  A query that is not live gets count 0, ring 0,
 *        scanned 0, certified 0 and a filler row (K4), and is counted in knn_stats[3].
 *    K2. The RANGE [lo, hi) of a live query is [0, ne); with voxel_room / voxel_start it is [voxel_start[g],
 *        voxel_start[g + 1]), g = voxel_room[v0], with lo held to >= 0 and hi to <= ne as rule 7 / N4 of conv3p.h hold
 *        them; g outside [0, num_rooms) gives an empty range.
 *    K3. The CANDIDATES are the voxels u in [lo, hi) with max_a |cell_a(u) - cell_a(v0)| <= R; valid[u] >= 0 where valid
 *        is given; u != v0 when exclude_self; and d2 finite, d2 = ((p_x-q_x)^2 + (p_y-q_y)^2) + (p_z-q_z)^2 being rule
 *        2's of conv3p.h with p = voxel_data[u][0..2] and the differences taken as q - p: the same float32 operations in
 *        the same order.
 *    K4. The n = min(k, candidates) smallest by the total order (d2, u) are KEPT, in that order: knn_index int32 (Q, k)
 *        and knn_d2 float32 (Q, k), entries j >= n holding -1 and +inf; knn_count[i] = n; knn_ring[i] = the largest
 *        Chebyshev cell distance among the kept, 0 if there is none.  All bit for bit.
 *    K5. The measured SPREAD, in float64, per room g (one cloud is the one room 0).  f_a(x, c) = (double)x_a -
 *        (double)c_a * (double)h: how far a point lies from the lattice position of a cell.  Pmin[g][a], Pmax[g][a] =
 *        minimum and maximum of f_a(q, cell(v0)) over the live queries whose voxel_room[v0] is g; Fmin[g][a], Fmax[g][a]
 *        = those of f_a(p_u, cell(u)) over the voxels u < ne with voxel_room[u] = g and a finite representative, valid
 *        or not; a room outside [0, num_rooms) contributes nothing.  S[g] = max_a max(Pmax[g][a] - Fmin[g][a],
 *        Fmax[g][a] - Pmin[g][a]), and L_r = (double)(r + 1) * (double)h - S[g].  A room without a live query or without
 *        a finite representative has no S, and no STOP of K6 holds in it.  Minima and maxima do not depend on the
 *        order they are taken in (the sign of a zero does not reach L_r), so S is defined to the bit.
 *    K6. STOP(r) holds when at least k candidates lie within Chebyshev distance r, L_r >= max(0.25 * h, 2^-50), and
 *        (double)d2_k(r) < (L_r * L_r) * (1 - 2^-20), d2_k(r) the k-th smallest d2 of those candidates.
 *        knn_scanned[i] = the smallest r in [1, R] with STOP(r), R if there is none; knn_certified[i] = 1 if
 *        STOP(knn_scanned[i]) holds, else 0.  Both bit for bit.
 *    K7. THEOREM.  K4 applied to the cube of knn_scanned[i] equals K4 applied to the cube of R, and the kept set of a
 *        certified query is the k nearest, by (d2, u), of ALL candidates of its room (K3 without the bound R).
 *        Proof.  A voxel u outside the cube of ring r differs from the query's cell by D >= r + 1 cells on some axis a
 *        (up to the sign of the axis).  There q_a - p_a = f_a(q) - f_a(p_u) -/+ D h, so |q_a - p_a| >= (r + 1) h - S
 *        = L_r by K5, for any h > 0 and any voxel_data.  With STOP(r) the k-th kept d2 is below L_r^2 (1 - 2^-20) <=
 *        |q_a - p_a|^2 (1 - 2^-20) < d2(u): the float32 d2 is within 2^-21 relative of the exact sum, which the factor
 *        covers, and the two floors on L_r keep the float64 rounding of L_r and of its square, and float32 underflow,
 *        inside the same factor.  So no voxel outside the cube enters the kept set.
 *        Hence the implementation never scans past knn_scanned[i].  The theorem is promised for consistent tables
 *        (voxel_room[u] = g exactly for u in the range of g), which the library's own always are; a displaced
 *        voxel_data or a wrong `voxel` only makes the search scan further, it never changes K3 / K4.
 *    K8. knn_stats int64 (16), exact, overwritten by every call: [0] live queries with count == k, [1] live queries
 *        with 0 < count < k, [2] live queries with count == 0, [3] queries that are not live, [4] certified queries,
 *        [5] the sum of knn_scanned over the live queries, [6 + r], r = 0 .. 8, the live queries with count > 0 and
 *        knn_ring == r, [15] 0.
 *   Status, in this order, all before any launch: Q < 0, M < 0, query_stride < 3, voxel_K < 3, k outside [1, 16], rings
 *   outside [1, 8], exclude_self not 0 or 1, num_rooms < 0, voxel not finite or not > 0, one of voxel_room / voxel_start
 *   without the other: CONV3P_ERR_INVALID_ARGUMENT; knn_stats NULL; query, knn_index, knn_d2, knn_count, knn_ring,
 *   knn_scanned or knn_certified NULL with Q > 0; voxel_data, neigh, voxel_cell or grid_stats NULL with Q > 0 and M > 0:
 *   CONV3P_ERR_INVALID_ARGUMENT; Q or M > 2^31 - 1, num_rooms > 65536: CONV3P_ERR_UNSUPPORTED; query_voxel NULL with
 *   Q > M: CONV3P_ERR_INVALID_ARGUMENT; scratch NULL or smaller than conv3p_grid_knn_scratch_bytes(Q, num_rooms):
 *   CONV3P_ERR_INVALID_ARGUMENT.  Q == 0 is valid: knn_stats is zeroed and nothing else is written.
 *   conv3p_grid_knn_scratch_bytes is a host-side function of its two arguments: a counter, twelve 64-bit extremes and
 *   an S per room (one room without rooms), and an int32 per query; a multiple of 256; 0 for refused arguments.
 *   The launches depend on nothing but rings > 1: two memsets (knn_stats; the counter and the extremes), the spread
 *   kernel, the bound kernel (S per room), the near kernel -- 16 lanes a query over its row of neigh, STOP(1) once; with
 *   rings > 1 a query without STOP(1) goes to a list -- and with rings > 1 the ring kernel on a fixed grid, a wave per
 *   listed query.  No host read.  No float atomics: the extremes are 64-bit integer maxima on order-preserving keys of
 *   the doubles (a minimum as the maximum of the complemented key), behind a reduction per thread and per wave; the
 *   counts are integer adds, per wave, then per workgroup.  Every loop is bounded whatever the memory holds.  Bitwise
 *   reproducible and independent of the launch geometry and of the order of the list.
 *
 * conv3p_grid_interpolate_knn_f32 / _i64:  rule 5 of conv3p.h on a table this search wrote.  knn_index, knn_d2 (Q,
 *   width) and knn_count (Q); k_use in [1, width], width in [1, 16].  Per query, n = min(k_use, max(knn_count[i], 0)):
 *   rule 5 applies to the first n entries exactly as it stands -- w_j = 1.0f / fmaxf(knn_d2[i][j], 1e-10f), the chains in
 *   rank order, the same label rule.  n == 0, or one of those entries outside [0, M): label -1, score row 0.  stats
 *   int64 (2) = {rows interpolated, rows without a neighbour}, exact, overwritten by every call.  With a table of
 *   rings = 1 and k = k_use the labels and scores are the plain call's, to the bit; with rings = R the labelled rows
 *   are the ring call's.
 *   Status, in this order: Q < 0, M < 0, width outside [1, 16], k_use outside [1, width], C outside [1, 128]:
 *   CONV3P_ERR_INVALID_ARGUMENT; stats NULL; knn_index, knn_d2, knn_count or out_labels NULL with Q > 0; voxel_scores NULL
 *   with Q > 0 and M > 0: CONV3P_ERR_INVALID_ARGUMENT; Q or M > 2^31 - 1: CONV3P_ERR_UNSUPPORTED.  One launch behind a
 *   16-byte memset of stats; 16 lanes a row; the only atomics are the integer adds of the two counts.
 *
 * conv3p_grid_normals_knn_f32:  conv3p_grid_normals_f32 on the neighbours of a table instead of on the 27 cells: a
 *   voxel of a thin or sparsely scanned surface, which has too few samples there, reaches as far as the table does.
 *   Rules R1 and R3-R6 of conv3p_grid_normals_f32 are unchanged; R2 is replaced by
 *    R2'. The table must come from voxel queries (Q = M, query_voxel NULL).  For j = 0 .. min(max(knn_count[v], 0),
 *        width) - 1 ascending, u = knn_index[v][j] is a SAMPLE when 0 <= u < ne and all three of p_u are finite;
 *        samples[v] = n, the number of samples; if p_v is not finite, n = 0.  The chains of R3 run in ascending j.
 *   3 <= min_neighbors <= 16.  samples, flags and moments are bit for bit, normal and curvature to R5's tolerance: the
 *   eigen-solve and the orientation are the same device code.
 *   Status, in this order: M < 0, K < 3, width outside [1, 16], min_neighbors outside [3, 16]:
 *   CONV3P_ERR_INVALID_ARGUMENT; viewpoint given with V < 1, or with V != 1 and voxel_room NULL:
 *   CONV3P_ERR_INVALID_ARGUMENT; M == 0: CONV3P_OK, nothing launched and nothing written; voxel_data, knn_index,
 *   knn_count, grid_stats, normals, curvature, samples, flags or normal_stats NULL: CONV3P_ERR_INVALID_ARGUMENT; M > 2^31
 *   - 1, or V with a viewpoint: CONV3P_ERR_UNSUPPORTED.  One launch behind a 16-byte memset of normal_stats; a thread per
 *   voxel.
 */
#ifndef CONV3P_KNN_H
#define CONV3P_KNN_H

#include "conv3p.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t conv3p_grid_knn_scratch_bytes(int64_t Q, int64_t num_rooms);
int conv3p_grid_knn_f32(const float *query, int64_t Q, int query_stride, const int32_t *query_voxel, const float *voxel_data,
                        int voxel_K, const int32_t *neigh, const int32_t *voxel_cell, const int32_t *voxel_room,
                        const int32_t *voxel_start, int64_t num_rooms, const int32_t *grid_stats, int64_t M,
                        const int32_t *valid, float voxel, int k, int rings, int exclude_self, int32_t *knn_index,
                        float *knn_d2, int32_t *knn_count, int32_t *knn_ring, int32_t *knn_scanned, int32_t *knn_certified,
                        int64_t *knn_stats, void *scratch, size_t scratch_bytes, void *stream);
int conv3p_grid_interpolate_knn_f32(const int32_t *knn_index, const float *knn_d2, const int32_t *knn_count, int64_t Q,
                                    int width, int k_use, const float *voxel_scores, int64_t M, int C, int32_t *out_labels,
                                    float *out_scores, int64_t *stats, void *stream);
int conv3p_grid_interpolate_knn_i64(const int32_t *knn_index, const float *knn_d2, const int32_t *knn_count, int64_t Q,
                                    int width, int k_use, const int64_t *voxel_scores, int64_t M, int C, int32_t *out_labels,
                                    float *out_scores, int64_t *stats, void *stream);
int conv3p_grid_normals_knn_f32(const float *voxel_data, int K, const int32_t *knn_index, const int32_t *knn_count, int width,
                                const int32_t *grid_stats, const int32_t *voxel_room, const float *viewpoint, int64_t V,
                                int64_t M, int min_neighbors, float *normals, float *curvature, int32_t *samples,
                                int32_t *flags, float *moments, int32_t *normal_stats, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CONV3P_KNN_H */
