// conv3p_abi_prestep.hpp -- host side of the pre-step: augment, the sorts, gather, the batch provider, the wide sort and
// the wide provider.  Included by conv3p_abi.hip.
namespace {

// Both orders of a cloud: one workgroup per cloud, npad keys of key_bytes in dynamic LDS.
using SortOrderKernel = void (*)(const float *, int, int, int, int32_t *);
int sort_order_launch(SortOrderKernel kernel, size_t key_bytes, const float *data, int B, int N, int row_floats,
                      int32_t *order, void *stream)
{
    if (B < 0 || N < 0 || row_floats < 3) return CONV3P_ERR_INVALID_ARGUMENT;
    if ((size_t)B * N == 0) return CONV3P_OK;
    if (!data || !order) return CONV3P_ERR_INVALID_ARGUMENT;
    if (N > 8192) return CONV3P_ERR_UNSUPPORTED;
    int npad = 64;
    while (npad < N) npad <<= 1;
    const size_t lds = (size_t)npad * key_bytes;
    const int threads = npad / 2 < 1024 ? (npad / 2 < 64 ? 64 : npad / 2) : 1024;
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kernel, dim3((unsigned)B), dim3(threads), lds, static_cast<hipStream_t>(stream), data, N,
                       row_floats, npad, order);
    return hip_ok();
}

// The keys of a cloud in the workspace of the wide sort (conv3p_sort_wide.hpp): npad of them, sorted in chunks.
struct WidePlan { int npad, chunk, tiles; };
bool wide_plan(int B, int N, WidePlan &w)
{
    if (B <= 0 || N <= 0 || N > kWideMaxN) return false;
    w.npad = 64;
    while (w.npad < N) w.npad <<= 1;
    w.chunk = w.npad < kWideChunk ? w.npad : kWideChunk;
    w.tiles = (N + kProviderTile - 1) / kProviderTile;
    return true;
}
// The wide sort's workspace: the keys, then (Morton) the tiles' coordinate ranges.
struct WideSortWs { void *keys; float *ranges; };
void carve_wide_sort(Carver &cv, int B, const WidePlan &w, bool morton, WideSortWs &ws)
{
    const size_t nkeys = (size_t)B * w.npad;
    ws.keys = morton ? static_cast<void *>(cv.take<uint64_t>(nkeys)) : static_cast<void *>(cv.take<SortKey>(nkeys));
    ws.ranges = cv.take<float>(morton ? (size_t)B * w.tiles * 6 : 0);
}
// The wide provider's workspace: the stage (B, N, 3) floats, the order (B, N) int32, then the wide sort's.
struct WideProviderWs { float *stage; int32_t *order; WideSortWs sort; };
size_t carve_wide_provider(void *base, int B, int N, const WidePlan &w, bool morton, WideProviderWs &ws)
{
    Carver cv(base);
    ws.stage = cv.take<float>((size_t)B * N * 3);
    ws.order = cv.take<int32_t>((size_t)B * N);
    carve_wide_sort(cv, B, w, morton, ws.sort);
    return cv.bytes();
}
inline bool wide_grids_ok(int B, const WidePlan &w)
{
    return (size_t)B * (size_t)(w.npad / 2) <= (size_t)INT32_MAX;       // bounds every grid: chunks, pairs, tiles
}

// order[b][r] of B clouds whose rows (xyz first, ld floats a row, cloud_floats a cloud) are on the device: the launches
// of conv3p_sort_wide.hpp, outside the profile bracket as the provider's.  have_ranges: the caller's own pass has written
// the Morton tile ranges.
template <bool MORTON>
void wide_sort_launch(const float *rows, size_t cloud_floats, int ld, int B, int N, const WidePlan &w, const WideSortWs &ws,
                      bool have_ranges, int32_t *order, hipStream_t s)
{
    using Key = typename std::conditional<MORTON, uint64_t, SortKey>::type;
    using Less = typename std::conditional<MORTON, MortonLess, KeyLess>::type;
    Key *keys = static_cast<Key *>(ws.keys);
    float *ranges = ws.ranges;
    if (MORTON && !have_ranges)
        hipLaunchKernelGGL(wide_range_kernel, dim3((unsigned)((size_t)B * w.tiles)), dim3(kProviderTile), 0, s, rows, N, ld,
                           w.tiles, ranges);
    const int chunks = w.npad / w.chunk;
    const unsigned cgrid = (unsigned)((size_t)B * chunks);
    const size_t lds = (size_t)w.chunk * sizeof(Key);
    const int threads = w.chunk / 2 < 1024 ? (w.chunk / 2 < 64 ? 64 : w.chunk / 2) : 1024;
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(wide_chunk_kernel<MORTON>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(wide_chunk_kernel<MORTON>, dim3(cgrid), dim3(threads), lds, s, rows, cloud_floats, ld, N, w.npad,
                       w.chunk, (const float *)ranges, w.tiles, (void *)keys, chunks == 1 ? order : (int32_t *)nullptr);
    if (chunks == 1) return;
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(wide_merge_kernel<Key, Less>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    const unsigned sgrid = (unsigned)((size_t)B * (w.npad / 2 / kWideStageThreads));
    for (int k = 2 * w.chunk; k <= w.npad; k <<= 1) {
        hipLaunchKernelGGL((wide_stage_kernel<Key, Less>), dim3(sgrid), dim3(kWideStageThreads), 0, s, keys, w.npad, k, 0, 1);
        for (int j = k >> 2; j >= w.chunk; j >>= 1)
            hipLaunchKernelGGL((wide_stage_kernel<Key, Less>), dim3(sgrid), dim3(kWideStageThreads), 0, s, keys, w.npad, k, j, 0);
        hipLaunchKernelGGL((wide_merge_kernel<Key, Less>), dim3(cgrid), dim3(threads), lds, s, keys, w.npad, w.chunk, N,
                           k == w.npad ? order : (int32_t *)nullptr);
    }
}

// Every status first; then ONE launch (wide: the launches of conv3p_sort_wide.hpp), outside the profile bracket (the
// table of kinds is pinned), as cls_tail_impl.
int provider_impl(bool wide, const float *data, const void *labels, int S, int Nsrc, int K, int label_bytes,
                  int labels_per_point, const int32_t *perm, int64_t perm_len, int64_t start, int B, int N,
                  int flags, double sigma, double clip, uint64_t seed, uint64_t step, const double *cos_sin,
                  const double *noise, float *points, float *input, int32_t *labels_out, double *cos_sin_out,
                  double *noise_out, int32_t *order_out, int32_t *bad_index, void *workspace,
                  size_t workspace_bytes, void *stream)
{
    const int known = CONV3P_PROVIDER_ROTATE | CONV3P_PROVIDER_JITTER | CONV3P_PROVIDER_SORT | CONV3P_PROVIDER_MORTON;
    if (B < 0 || N < 0 || S < 0 || K < 3 || Nsrc < N || start < 0 || (flags & ~known)) return CONV3P_ERR_INVALID_ARGUMENT;
    if ((flags & CONV3P_PROVIDER_MORTON) && !(flags & CONV3P_PROVIDER_SORT)) return CONV3P_ERR_INVALID_ARGUMENT;   // a qualifier
    if (wide && !(flags & CONV3P_PROVIDER_SORT)) return CONV3P_ERR_INVALID_ARGUMENT;   // the wide entry is the sorting one
    if ((flags & CONV3P_PROVIDER_JITTER) && (!(clip > 0.0) || !(sigma >= 0.0))) return CONV3P_ERR_INVALID_ARGUMENT;
    if ((labels != nullptr) != (labels_out != nullptr)) return CONV3P_ERR_INVALID_ARGUMENT;
    if (labels && label_bytes != 1 && label_bytes != 4 && label_bytes != 8) return CONV3P_ERR_INVALID_ARGUMENT;
    if (perm ? (perm_len < 0 || start > perm_len - B) : start > (int64_t)INT32_MAX) return CONV3P_ERR_INVALID_ARGUMENT;
    if ((size_t)B * N == 0) return CONV3P_OK;
    if (!data || !points || !input || !bad_index) return CONV3P_ERR_INVALID_ARGUMENT;
    const bool sort = (flags & CONV3P_PROVIDER_SORT) != 0;
    if (sort && N > (wide ? kWideMaxN : kProviderMaxSortN)) return CONV3P_ERR_UNSUPPORTED;
    const size_t tiles = ((size_t)N + kProviderTile - 1) / kProviderTile;
    if (K > 65536 || ((!sort || wide) && (size_t)B * tiles > (size_t)INT32_MAX)) return CONV3P_ERR_UNSUPPORTED;
    const bool morton = (flags & CONV3P_PROVIDER_MORTON) != 0;
    WidePlan w;
    if (wide && (!wide_plan(B, N, w) || !wide_grids_ok(B, w))) return CONV3P_ERR_UNSUPPORTED;
    TRY(buf_check(workspace, workspace_bytes,
                  wide ? conv3p_provider_wide_workspace_bytes(B, N, flags) : conv3p_provider_workspace_bytes(B, N, flags)));
    ProviderArgs a;
    a.data = data; a.labels = labels; a.perm = perm;
    a.cos_sin = reinterpret_cast<const double2 *>(cos_sin); a.noise = noise;
    a.start = start;
    a.S = S; a.Nsrc = Nsrc; a.K = K; a.B = B; a.N = N;
    a.label_bytes = label_bytes; a.per_point = labels_per_point != 0;
    a.rotate = (flags & CONV3P_PROVIDER_ROTATE) != 0; a.jitter = (flags & CONV3P_PROVIDER_JITTER) != 0;
    a.sigma = sigma; a.clip = clip;
    a.seed_lo = (unsigned)seed; a.seed_hi = (unsigned)(seed >> 32);
    a.step_lo = (unsigned)step; a.step_hi = (unsigned)(step >> 32);
    a.points = points; a.input = input; a.labels_out = labels_out;
    a.cos_sin_out = reinterpret_cast<double2 *>(cos_sin_out); a.noise_out = noise_out; a.order_out = order_out;
    a.bad_index = bad_index;
    a.stage = static_cast<float *>(workspace);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!sort) {
        hipLaunchKernelGGL(provider_flat_kernel, dim3((unsigned)((size_t)B * tiles)), dim3(kProviderTile), 0, s, a, (int)tiles);
        return hip_ok();
    }
    if (wide) {
        WideProviderWs ws;
        (void)carve_wide_provider(workspace, B, N, w, morton, ws);
        int32_t *order = ws.order;
        const unsigned grid = (unsigned)((size_t)B * tiles);
        if (morton) {
            hipLaunchKernelGGL(provider_wide_stage_kernel<true>, dim3(grid), dim3(kProviderTile), 0, s, a, (int)tiles,
                               ws.sort.ranges);
            wide_sort_launch<true>(a.stage, (size_t)N * 3, 3, B, N, w, ws.sort, true, order, s);
        } else {
            hipLaunchKernelGGL(provider_wide_stage_kernel<false>, dim3(grid), dim3(kProviderTile), 0, s, a, (int)tiles,
                               (float *)nullptr);
            wide_sort_launch<false>(a.stage, (size_t)N * 3, 3, B, N, w, ws.sort, false, order, s);
        }
        hipLaunchKernelGGL(provider_wide_gather_kernel, dim3(grid), dim3(kProviderTile), 0, s, a, (int)tiles,
                           (const int32_t *)order);
        return hip_ok();
    }
    int npad = 64;
    while (npad < N) npad <<= 1;
    const size_t lds = (size_t)npad * (morton ? sizeof(uint64_t) : sizeof(SortKey));
    const int threads = npad / 2 < 1024 ? (npad / 2 < 64 ? 64 : npad / 2) : 1024;
    auto kernel = morton ? provider_sort_kernel<true> : provider_sort_kernel<false>;
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kernel, dim3((unsigned)B), dim3(threads), lds, s, a, npad);
    return hip_ok();
}

}  // namespace

extern "C" {

int conv3p_augment_f32(const float *points_in, const double *cos_sin, const double *noise, double sigma, double clip,
                       int B, int N, float *points_out, void *stream)
{
    if (B < 0 || N < 0 || !(clip > 0.0) || !(sigma >= 0.0)) return CONV3P_ERR_INVALID_ARGUMENT;   // assert(clip > 0), :72
    const size_t total = (size_t)B * N;
    if (total == 0) return CONV3P_OK;
    if (!points_in || !points_out) return CONV3P_ERR_INVALID_ARGUMENT;
    const unsigned grid = (unsigned)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
    hipLaunchKernelGGL(augment_kernel, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), points_in,
                       reinterpret_cast<const double2 *>(cos_sin), noise, sigma, clip, points_out, total, N);
    return hip_ok();
}

int conv3p_sort_xyz_order_f32(const float *data, int B, int N, int row_floats, int32_t *order, void *stream)
{
    return sort_order_launch(sort_xyz_kernel, sizeof(SortKey), data, B, N, row_floats, order, stream);
}

int conv3p_sort_morton_order_f32(const float *data, int B, int N, int row_floats, int32_t *order, void *stream)
{
    return sort_order_launch(sort_morton_kernel, sizeof(uint64_t), data, B, N, row_floats, order, stream);
}

int conv3p_gather_rows(const void *src, const int32_t *order, int B, int N, int row_bytes, void *dst, void *stream)
{
    if (B < 0 || N < 0 || row_bytes < 1) return CONV3P_ERR_INVALID_ARGUMENT;
    const size_t rows = (size_t)B * N;
    if (rows == 0) return CONV3P_OK;
    if (!src || !order || !dst || src == dst) return CONV3P_ERR_INVALID_ARGUMENT;
    const size_t work = rows * (size_t)((row_bytes & 3) == 0 ? row_bytes >> 2 : row_bytes);
    const unsigned grid = (unsigned)((work + 255) / 256 < 4096 ? (work + 255) / 256 : 4096);
    hipLaunchKernelGGL(gather_rows_kernel, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream),
                       static_cast<const char *>(src), order, N, row_bytes, static_cast<char *>(dst), rows);
    return hip_ok();
}

size_t conv3p_provider_workspace_bytes(int B, int N, int flags)
{
    if (B <= 0 || N <= 0 || !(flags & CONV3P_PROVIDER_SORT) || N > kProviderMaxSortN) return 0;
    return up((size_t)B * N * 3 * sizeof(float));
}

size_t conv3p_sort_order_workspace_bytes(int B, int N, int method)
{
    WidePlan w;
    if ((method != CONV3P_SORT_XYZ && method != CONV3P_SORT_MORTON) || !wide_plan(B, N, w)) return 0;
    Carver cv(nullptr);
    WideSortWs ws;
    carve_wide_sort(cv, B, w, method == CONV3P_SORT_MORTON, ws);
    return cv.bytes();
}

int conv3p_sort_order_f32(const float *data, int B, int N, int row_floats, int method, int32_t *order, void *workspace,
                          size_t workspace_bytes, void *stream)
{
    if (B < 0 || N < 0 || row_floats < 3 || (method != CONV3P_SORT_XYZ && method != CONV3P_SORT_MORTON))
        return CONV3P_ERR_INVALID_ARGUMENT;
    if ((size_t)B * N == 0) return CONV3P_OK;
    if (!data || !order) return CONV3P_ERR_INVALID_ARGUMENT;
    if (N > kWideMaxN) return CONV3P_ERR_UNSUPPORTED;
    const bool morton = method == CONV3P_SORT_MORTON;
    WidePlan w;
    wide_plan(B, N, w);
    if (!wide_grids_ok(B, w)) return CONV3P_ERR_UNSUPPORTED;
    Carver cv(workspace);
    WideSortWs ws;
    carve_wide_sort(cv, B, w, morton, ws);
    TRY(buf_check(workspace, workspace_bytes, cv.bytes()));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t cloud = (size_t)N * row_floats;
    if (morton) wide_sort_launch<true>(data, cloud, row_floats, B, N, w, ws, false, order, s);
    else wide_sort_launch<false>(data, cloud, row_floats, B, N, w, ws, false, order, s);
    return hip_ok();
}

size_t conv3p_provider_wide_workspace_bytes(int B, int N, int flags)
{
    WidePlan w;
    if (!(flags & CONV3P_PROVIDER_SORT) || !wide_plan(B, N, w)) return 0;
    WideProviderWs ws;
    return carve_wide_provider(nullptr, B, N, w, (flags & CONV3P_PROVIDER_MORTON) != 0, ws);
}

#define PROVIDER_PARAMS                                                                                              \
    const float *data, const void *labels, int S, int Nsrc, int K, int label_bytes, int labels_per_point,            \
        const int32_t *perm, int64_t perm_len, int64_t start, int B, int N, int flags, double sigma, double clip,    \
        uint64_t seed, uint64_t step, const double *cos_sin, const double *noise, float *points, float *input,       \
        int32_t *labels_out, double *cos_sin_out, double *noise_out, int32_t *order_out, int32_t *bad_index,         \
        void *workspace, size_t workspace_bytes, void *stream
#define PROVIDER_ARGS                                                                                                \
    data, labels, S, Nsrc, K, label_bytes, labels_per_point, perm, perm_len, start, B, N, flags, sigma, clip, seed,  \
        step, cos_sin, noise, points, input, labels_out, cos_sin_out, noise_out, order_out, bad_index, workspace,    \
        workspace_bytes, stream
int conv3p_provider_batch_f32(PROVIDER_PARAMS) { return provider_impl(false, PROVIDER_ARGS); }
int conv3p_provider_batch_wide_f32(PROVIDER_PARAMS) { return provider_impl(true, PROVIDER_ARGS); }
#undef PROVIDER_PARAMS
#undef PROVIDER_ARGS

}  // extern "C"
