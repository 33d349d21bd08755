// conv3p_abi_knn.hpp -- host side of the k-nearest-voxel search and of its two consumers (include/conv3p_knn.h).  Included
// by conv3p_abi.hip.
namespace {

static_assert(kKnnHeaderBytes % kAlign == 0, "the header keeps what follows it aligned");
// The search's scratch: the list's counter, twelve extremes and an S per room, a place per query.  The counter and the
// extremes are what one memset zeroes: they follow one another.
struct KnnScratch { int32_t *counter; unsigned long long *words; double *S; int32_t *list; size_t zeroed; };
size_t carve_knn(void *ws, int64_t Q, int64_t rooms, KnnScratch &p)
{
    Carver cv(ws);
    p.counter = cv.take<int32_t>(kKnnHeaderBytes / sizeof(int32_t));
    p.words = cv.take<unsigned long long>((size_t)rooms * kKnnRoomWords);
    p.zeroed = cv.bytes();
    p.S = cv.take<double>((size_t)rooms);
    p.list = cv.take<int32_t>((size_t)Q);
    return cv.bytes();
}
bool knn_sized(int64_t Q, int64_t num_rooms) { return Q >= 0 && Q <= (int64_t)INT32_MAX && num_rooms >= 0 && num_rooms <= kGridRoomsMaxRooms; }

template <typename S>
int grid_interpolate_knn(const int32_t *knn_index, const float *knn_d2, const int32_t *knn_count, int64_t Q, int width, int k_use,
                         const S *voxel_scores, int64_t M, int C, int32_t *out_labels, float *out_scores, int64_t *stats,
                         void *stream)
{
    if (Q < 0 || M < 0 || width < 1 || width > kKnnMaxK || k_use < 1 || k_use > width || C < 1 || C > kInterpMaxClass)
        return CONV3P_ERR_INVALID_ARGUMENT;
    if (!stats || (Q > 0 && (!knn_index || !knn_d2 || !knn_count || !out_labels)) || (Q > 0 && M > 0 && !voxel_scores))
        return CONV3P_ERR_INVALID_ARGUMENT;
    if (Q > (int64_t)INT32_MAX || M > (int64_t)INT32_MAX) return CONV3P_ERR_UNSUPPORTED;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(stats, 0, 2 * sizeof(int64_t), s) != hipSuccess) return CONV3P_ERR_LAUNCH;
    if (Q == 0) return hip_ok();
    const size_t work = ((size_t)Q + kInterpRows - 1) / kInterpRows;
    hipLaunchKernelGGL((grid_knn_interpolate_kernel<S>), dim3(capped_grid(work, kInterpMaxGrid)), dim3(kInterpThreads), 0, s,
                       knn_index, knn_d2, knn_count, (long long)Q, width, k_use, voxel_scores, (int)M, C, out_labels, out_scores,
                       reinterpret_cast<unsigned long long *>(stats));
    return hip_ok();
}

}  // namespace

extern "C" {

size_t conv3p_grid_knn_scratch_bytes(int64_t Q, int64_t num_rooms)
{
    KnnScratch p;
    if (!knn_sized(Q, num_rooms)) return 0;
    return carve_knn(nullptr, Q, num_rooms > 0 ? num_rooms : 1, p);
}

int conv3p_grid_knn_f32(const float *query, int64_t Q, int query_stride, const int32_t *query_voxel, const float *voxel_data,
                        int voxel_K, const int32_t *neigh, const int32_t *voxel_cell, const int32_t *voxel_room,
                        const int32_t *voxel_start, int64_t num_rooms, const int32_t *grid_stats, int64_t M,
                        const int32_t *valid, float voxel, int k, int rings, int exclude_self, int32_t *knn_index,
                        float *knn_d2, int32_t *knn_count, int32_t *knn_ring, int32_t *knn_scanned, int32_t *knn_certified,
                        int64_t *knn_stats, void *scratch, size_t scratch_bytes, void *stream)
{
    if (Q < 0 || M < 0 || query_stride < 3 || voxel_K < 3 || k < 1 || k > kKnnMaxK || rings < 1 || rings > kRingMax ||
        (exclude_self != 0 && exclude_self != 1) || num_rooms < 0 || !(voxel > 0.0f) || !(voxel < INFINITY))
        return CONV3P_ERR_INVALID_ARGUMENT;
    if ((voxel_room == nullptr) != (voxel_start == nullptr)) return CONV3P_ERR_INVALID_ARGUMENT;
    if (!knn_stats || (Q > 0 && (!query || !knn_index || !knn_d2 || !knn_count || !knn_ring || !knn_scanned || !knn_certified)) ||
        (Q > 0 && M > 0 && (!voxel_data || !neigh || !voxel_cell || !grid_stats)))
        return CONV3P_ERR_INVALID_ARGUMENT;
    if (Q > (int64_t)INT32_MAX || M > (int64_t)INT32_MAX || num_rooms > kGridRoomsMaxRooms) return CONV3P_ERR_UNSUPPORTED;
    if (!query_voxel && Q > M) return CONV3P_ERR_INVALID_ARGUMENT;
    KnnScratch p;
    const int rooms = voxel_room ? (int)num_rooms : 1;   // the records the kernels use; the scratch has max(num_rooms, 1)
    const size_t need = carve_knn(scratch, Q, num_rooms > 0 ? num_rooms : 1, p);
    if (!scratch || scratch_bytes < need) return CONV3P_ERR_INVALID_ARGUMENT;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(knn_stats, 0, kKnnStats * sizeof(int64_t), s) != hipSuccess) return CONV3P_ERR_LAUNCH;
    if (Q == 0) return hip_ok();
    if (hipMemsetAsync(scratch, 0, p.zeroed, s) != hipSuccess) return CONV3P_ERR_LAUNCH;
    const size_t most = (size_t)(Q > M ? Q : M);
    hipLaunchKernelGGL(grid_knn_spread_kernel, dim3(capped_grid((most + kKnnSpreadThreads - 1) / kKnnSpreadThreads, kKnnSpreadMaxGrid)),
                       dim3(kKnnSpreadThreads), 0, s, query, (long long)Q, query_stride, query_voxel, voxel_data, voxel_K,
                       voxel_cell, voxel_room, rooms, grid_stats, (int)M, voxel, p.words);
    const size_t rwork = ((size_t)(rooms > 0 ? rooms : 1) + kKnnSpreadThreads - 1) / kKnnSpreadThreads;
    hipLaunchKernelGGL(grid_knn_bound_kernel, dim3((unsigned)rwork), dim3(kKnnSpreadThreads), 0, s, p.words, rooms, p.S);
    const KnnOut out = {knn_index, knn_d2, knn_count, knn_ring, knn_scanned, knn_certified};
    unsigned long long *st = reinterpret_cast<unsigned long long *>(knn_stats);
    const size_t work = ((size_t)Q + kInterpRows - 1) / kInterpRows;
    hipLaunchKernelGGL(grid_knn_near_kernel, dim3(capped_grid(work, kInterpMaxGrid)), dim3(kInterpThreads), 0, s, query, (long long)Q,
                       query_stride, query_voxel, voxel_data, voxel_K, neigh, voxel_room, voxel_start, rooms, grid_stats, (int)M, valid,
                       voxel, k, rings, exclude_self, p.S, p.counter, p.list, out, st);
    if (rings > 1)
        hipLaunchKernelGGL(grid_knn_ring_kernel, dim3(kRingGrid), dim3(kRingThreads), 0, s, query, (long long)Q, query_stride,
                           query_voxel, voxel_data, voxel_K, voxel_cell, voxel_room, voxel_start, rooms, grid_stats, (int)M, valid,
                           voxel, k, rings, exclude_self, p.S, p.counter, p.list, out, st);
    return hip_ok();
}

int conv3p_grid_interpolate_knn_f32(const int32_t *knn_index, const float *knn_d2, const int32_t *knn_count, int64_t Q,
                                    int width, int k_use, const float *voxel_scores, int64_t M, int C, int32_t *out_labels,
                                    float *out_scores, int64_t *stats, void *stream)
{
    return grid_interpolate_knn(knn_index, knn_d2, knn_count, Q, width, k_use, voxel_scores, M, C, out_labels, out_scores, stats,
                                stream);
}

int conv3p_grid_interpolate_knn_i64(const int32_t *knn_index, const float *knn_d2, const int32_t *knn_count, int64_t Q,
                                    int width, int k_use, const int64_t *voxel_scores, int64_t M, int C, int32_t *out_labels,
                                    float *out_scores, int64_t *stats, void *stream)
{
    return grid_interpolate_knn(knn_index, knn_d2, knn_count, Q, width, k_use, reinterpret_cast<const long long *>(voxel_scores), M,
                                C, out_labels, out_scores, stats, stream);
}

int conv3p_grid_normals_knn_f32(const float *voxel_data, int K, const int32_t *knn_index, const int32_t *knn_count, int width,
                                const int32_t *grid_stats, const int32_t *voxel_room, const float *viewpoint, int64_t V,
                                int64_t M, int min_neighbors, float *normals, float *curvature, int32_t *samples,
                                int32_t *flags, float *moments, int32_t *normal_stats, void *stream)
{
    if (M < 0 || K < 3 || width < 1 || width > kKnnMaxK || min_neighbors < kNormalsMinNeighbors || min_neighbors > kKnnMaxK)
        return CONV3P_ERR_INVALID_ARGUMENT;
    if (viewpoint && (V < 1 || (V != 1 && !voxel_room))) return CONV3P_ERR_INVALID_ARGUMENT;
    if (M == 0) return CONV3P_OK;
    if (!voxel_data || !knn_index || !knn_count || !grid_stats || !normals || !curvature || !samples || !flags || !normal_stats)
        return CONV3P_ERR_INVALID_ARGUMENT;
    if (M > (int64_t)INT32_MAX || (viewpoint && V > (int64_t)INT32_MAX)) return CONV3P_ERR_UNSUPPORTED;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (hipMemsetAsync(normal_stats, 0, 4 * sizeof(int32_t), s) != hipSuccess) return CONV3P_ERR_LAUNCH;
    const size_t work = ((size_t)M + kNormalsThreads - 1) / kNormalsThreads;
    hipLaunchKernelGGL(grid_knn_normals_kernel, dim3(capped_grid(work, kNormalsMaxGrid)), dim3(kNormalsThreads), 0, s, voxel_data, K,
                       knn_index, knn_count, width, grid_stats, voxel_room, viewpoint, viewpoint ? (int)V : 0, (int)M, min_neighbors,
                       normals, curvature, samples, flags, moments, normal_stats);
    return hip_ok();
}

}  // extern "C"
