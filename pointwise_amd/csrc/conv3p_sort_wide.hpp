// conv3p_sort_wide.hpp -- both orders of the pre-step for clouds of up to 65536 rows, a cloud spread over many
// workgroups (DESIGN.md section 5i').
//
// sort_xyz_kernel, sort_morton_kernel and provider_sort_kernel give a cloud to ONE workgroup and keep every key in LDS:
// N <= 8192, and a batch of few large clouds occupies as many CUs as it has clouds.  Here the keys of a cloud live in the
// workspace, npad = the power of two >= N of them (the padding keys are all ones, as in the kernels above), and are
// sorted by the bitonic network in its ascending-only form:
//
//   wide_range_kernel   (Morton only)  a workgroup owns kProviderTile rows: their MortonRange -> ranges[b][tile].  The
//                                      provider's stage pass does the same for the rows it augments.
//   wide_chunk_kernel   a workgroup owns a chunk of `chunk` keys (a power of two <= 8192): it builds them -- the Morton
//                       keys after joining the cloud's tile ranges into the box by morton_box_reduce: min and max do not
//                       depend on the order they are taken in -- and sorts them ascending in LDS by bitonic_sort_keys.
//   for k = 2 chunk, 4 chunk, .., npad:   runs of k / 2 sorted keys -> runs of k
//     wide_stage_kernel, flip     key i of the run's lower half against key k - 1 - i of the upper half: both halves
//                                 ascend, so this is the network's first half-cleaner and every later stage ascends too
//     wide_stage_kernel, j        for j = k / 4 .. chunk: key i against key i + j; one launch per stage
//     wide_merge_kernel           the stages j = chunk / 2 .. 1 of every chunk in LDS
//   The last launch (wide_chunk_kernel when npad == chunk, else the last wide_merge_kernel) writes order[b][r] = the row
//   of key r, r < N, instead of writing the keys back.
//
// Both orders are strict total orders (the row index breaks every tie), so the result is the one of the one-workgroup
// kernels bit for bit.  A padding key is not "no row": at N = 65536 a non-finite row 65535 HAS the Morton key ~0 and
// there is no padding; nothing here looks at a key's value other than to compare it, and rows are told from padding by
// their place r < N alone.
//
// Phases are ordered by stream order between launches and by nothing else: no workgroup waits for another, there is no
// atomic on global memory, no memset, nothing is read from the workspace that this call has not written, every loop is
// bounded by an argument.  A cloud's keys, and so its order, do not depend on B or on the cloud's place in the batch.
//
//   provider_wide_stage_kernel    provider_flat_kernel's grid (B * ceil(N / 256) workgroups): the augmented xyz of every
//                                 source row -> stage (12 bytes a row), noise_out, cos_sin_out, per-sample labels,
//                                 bad_index; with MORTON the tile's range
//   provider_wide_gather_kernel   the same grid over OUTPUT rows: points, input, per-point labels and order_out of row r
//                                 from stage and source row order[b][r]
#pragma once

#include "conv3p_provider.hpp"

namespace conv3p {

constexpr int kWideMaxN = 65536;
constexpr int kWideStageThreads = 256;      // pairs per workgroup of wide_stage_kernel
#ifndef CONV3P_WIDE_CHUNK                   // developer A/B builds only (tools/provider_time.py --wide)
#define CONV3P_WIDE_CHUNK 2048
#endif
constexpr int kWideChunk = CONV3P_WIDE_CHUNK;
static_assert(kWideChunk >= 2 * kWideStageThreads && kWideChunk <= 8192 && (kWideChunk & (kWideChunk - 1)) == 0,
              "a chunk is a power of two, at least one workgroup of pairs, at most what fits LDS");

__device__ __forceinline__ int32_t wide_key_row(const SortKey &k) { return (int32_t)k.idx; }
__device__ __forceinline__ int32_t wide_key_row(uint64_t k) { return (int32_t)(k & 0xFFFFu); }

__device__ __forceinline__ void wide_pad_key(SortKey &k) { k = SortKey{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}; }
__device__ __forceinline__ void wide_pad_key(uint64_t &k) { k = kMortonPadKey; }

// float_key's inverse on the keys of finite values and infinities.
__device__ __forceinline__ float wide_key_float(uint32_t u)
{
    return __builtin_bit_cast(float, (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u);
}

// The lanes' ranges of one workgroup -> out[0..2] = lo, out[3..5] = hi.  float_key is monotone, so the minimum and the
// maximum are taken on integers in LDS (rng_s: 6 words); no finite row: lo = +inf, hi = -inf, as morton_range_init.
// Every thread of the workgroup calls it.
__device__ __forceinline__ void wide_tile_range(const MortonRange &r, uint32_t *rng_s, int tid, float *out)
{
    if (tid < 3) rng_s[tid] = float_key(__builtin_inff());
    else if (tid < 6) rng_s[tid] = float_key(-__builtin_inff());
    __syncthreads();
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (r.lo[a] <= r.hi[a]) {                 // the lane has seen a finite row
            atomicMin(&rng_s[a], float_key(r.lo[a]));
            atomicMax(&rng_s[3 + a], float_key(r.hi[a]));
        }
    }
    __syncthreads();
    if (tid < 6) out[tid] = wide_key_float(rng_s[tid]);
}

// ranges[b][tile][6] of the rows' xyz; `data` rows have `ld` floats.
__global__ __launch_bounds__(kProviderTile) void wide_range_kernel(const float *__restrict__ data, int N, int ld, int tiles,
                                                                   float *__restrict__ ranges)
{
    __shared__ uint32_t rng_s[6];
    const int tid = threadIdx.x, b = (int)(blockIdx.x / (unsigned)tiles), tile = (int)(blockIdx.x % (unsigned)tiles);
    const int i = tile * kProviderTile + tid;
    MortonRange rg;
    morton_range_init(rg);
    if (i < N) {
        const float *row = data + ((size_t)b * N + i) * ld;
        morton_range_add(rg, row[0], row[1], row[2]);
    }
    wide_tile_range(rg, rng_s, tid, ranges + (size_t)blockIdx.x * 6);
}

// Chunk `ch` of cloud b: keys of rows ch * chunk .. (padding beyond N), sorted ascending.  rows: xyz first, `ld` floats
// a row, `cloud_floats` floats a cloud.  order != NULL (npad == chunk): order[b][r] instead of the keys.
template <bool MORTON>
__global__ __launch_bounds__(1024) void wide_chunk_kernel(const float *__restrict__ rows, size_t cloud_floats, int ld, int N,
                                                          int npad, int chunk, const float *__restrict__ ranges, int tiles,
                                                          void *keys_out, int32_t *order)
{
    using Key = typename std::conditional<MORTON, uint64_t, SortKey>::type;
    using Less = typename std::conditional<MORTON, MortonLess, KeyLess>::type;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    Key *keys = reinterpret_cast<Key *>(smem);
    const int tid = threadIdx.x, nthr = blockDim.x, chunks = npad / chunk;
    const int b = (int)(blockIdx.x / (unsigned)chunks), i0 = (int)(blockIdx.x % (unsigned)chunks) * chunk;
    const float *cloud = rows + (size_t)b * cloud_floats;
    MortonBox box;
    if constexpr (MORTON) {
        __shared__ float box_s[16 * 6];
        MortonRange rg;
        morton_range_init(rg);
        const float *rb = ranges + (size_t)b * tiles * 6;
        for (int t = tid; t < tiles; t += nthr)
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                rg.lo[a] = fminf(rg.lo[a], rb[(size_t)t * 6 + a]);
                rg.hi[a] = fmaxf(rg.hi[a], rb[(size_t)t * 6 + 3 + a]);
            }
        box = morton_box_reduce(rg, box_s, tid, nthr);
    }
    for (int e = tid; e < chunk; e += nthr) {
        const int i = i0 + e;
        Key k;
        wide_pad_key(k);
        if (i < N) {
            const float *row = cloud + (size_t)i * ld;
            if constexpr (MORTON) k = make_morton_key(row[0], row[1], row[2], i, box);
            else k = make_sort_key(row[0], row[1], row[2], i);
        }
        keys[e] = k;
    }
    __syncthreads();
    bitonic_sort_keys<Key, Less>(keys, chunk, tid, nthr);
    if (order) {
        for (int e = tid; e < chunk && i0 + e < N; e += nthr) order[(size_t)b * N + i0 + e] = wide_key_row(keys[e]);
        return;
    }
    Key *out = static_cast<Key *>(keys_out) + (size_t)b * npad + i0;
    for (int e = tid; e < chunk; e += nthr) out[e] = keys[e];
}

// One stage of the network on the keys in the workspace, a pair a thread: B * npad / 2 threads.  flip: key i of every
// run of k against key k - 1 - i; else key i against key i + j (j >= chunk: the stages below j are wide_merge_kernel's).
template <typename Key, typename Less>
__global__ __launch_bounds__(kWideStageThreads) void wide_stage_kernel(Key *keys, int npad, int k, int j, int flip)
{
    const Less less;
    const unsigned per = (unsigned)(npad >> 1) / kWideStageThreads;          // workgroups a cloud
    const int b = (int)(blockIdx.x / per), t = (int)(blockIdx.x % per) * kWideStageThreads + (int)threadIdx.x;
    Key *kc = keys + (size_t)b * npad;
    int i, l;
    if (flip) {
        const int h = k >> 1, o = t & (h - 1);
        i = ((t & ~(h - 1)) << 1) | o;
        l = ((t & ~(h - 1)) << 1) + k - 1 - o;
    } else {
        i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        l = i | j;
    }
    const Key a = kc[i], c = kc[l];
    if (less(c, a)) {
        kc[i] = c;
        kc[l] = a;
    }
}

// The ascending stages j = n / 2 .. 1 over keys[0 .. n) in LDS: what is left of a merge once its pairs are closer than n.
// The keys were stored before a barrier, and the last stage ends in one.
template <typename Key, typename Less>
__device__ __forceinline__ void bitonic_merge_keys(Key *keys, int n, int tid, int nthr)
{
    const Less less;
    for (int j = n >> 1; j > 0; j >>= 1) {
        for (int t = tid; t < (n >> 1); t += nthr) {
            const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
            const int l = i | j;
            const Key a = keys[i], c = keys[l];
            if (less(c, a)) {
                keys[i] = c;
                keys[l] = a;
            }
        }
        __syncthreads();
    }
}

// The stages below `chunk` of one merge level, a workgroup a chunk.  order != NULL (the last level): order[b][r], r < N,
// instead of the keys.
template <typename Key, typename Less>
__global__ __launch_bounds__(1024) void wide_merge_kernel(Key *keys_g, int npad, int chunk, int N, int32_t *order)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    Key *keys = reinterpret_cast<Key *>(smem);
    const int tid = threadIdx.x, nthr = blockDim.x, chunks = npad / chunk;
    const int b = (int)(blockIdx.x / (unsigned)chunks), i0 = (int)(blockIdx.x % (unsigned)chunks) * chunk;
    Key *g = keys_g + (size_t)b * npad + i0;
    for (int e = tid; e < chunk; e += nthr) keys[e] = g[e];
    __syncthreads();
    bitonic_merge_keys<Key, Less>(keys, chunk, tid, nthr);
    if (order) {
        for (int e = tid; e < chunk && i0 + e < N; e += nthr) order[(size_t)b * N + i0 + e] = wide_key_row(keys[e]);
        return;
    }
    for (int e = tid; e < chunk; e += nthr) g[e] = keys[e];
}

// The provider's first pass: provider_flat_kernel's tile of SOURCE rows, augmented into the stage.
template <bool MORTON>
__global__ __launch_bounds__(kProviderTile) void provider_wide_stage_kernel(const ProviderArgs p, int tiles, float *ranges)
{
    __shared__ double2 cs_s;
    __shared__ int bad_s;
    __shared__ uint32_t rng_s[6];
    const int tid = threadIdx.x, b = (int)(blockIdx.x / (unsigned)tiles), tile = (int)(blockIdx.x % (unsigned)tiles);
    const long long s = provider_sample(p, b);
    const bool valid = s >= 0 && s < p.S;
    if (tid == 0) {
        bad_s = 0;
        provider_cloud_head(p, b, s, valid, tile == 0, &cs_s);
    }
    __syncthreads();
    if (blockIdx.x == 0) provider_count_bad(p, &bad_s, tid, kProviderTile);
    const int i = tile * kProviderTile + tid;
    MortonRange rg;
    morton_range_init(rg);
    if (i < p.N) {
        float r[3];
        provider_row(p, b, s, valid, i, cs_s, r);
        float *st = p.stage + ((size_t)b * p.N + i) * 3;
        st[0] = r[0];
        st[1] = r[1];
        st[2] = r[2];
        morton_range_add(rg, r[0], r[1], r[2]);
    }
    if constexpr (MORTON) wide_tile_range(rg, rng_s, tid, ranges + (size_t)blockIdx.x * 6);
}

// The provider's last pass: a tile of OUTPUT rows.  Row r takes xyz from stage row order[b][r], the other channels and
// the per-point label from the source row of that index: provider_sort_kernel's epilogue, the tile's xyz through LDS as
// in provider_flat_kernel so that consecutive lanes store consecutive words.
__global__ __launch_bounds__(kProviderTile) void provider_wide_gather_kernel(const ProviderArgs p, int tiles,
                                                                             const int32_t *__restrict__ order)
{
    __shared__ float xyz_s[kProviderTile * 3];
    __shared__ int32_t idx_s[kProviderTile];
    const int tid = threadIdx.x, b = (int)(blockIdx.x / (unsigned)tiles), tile = (int)(blockIdx.x % (unsigned)tiles);
    const int r0 = tile * kProviderTile, N = p.N, K = p.K;
    const long long s = provider_sample(p, b);
    const bool valid = s >= 0 && s < p.S;
    const int r = r0 + tid;
    if (r < N) {
        const size_t o = (size_t)b * N + r;
        const int i = order[o];
        const float *st = p.stage + ((size_t)b * N + i) * 3;
        idx_s[tid] = i;
        xyz_s[3 * tid] = st[0];
        xyz_s[3 * tid + 1] = st[1];
        xyz_s[3 * tid + 2] = st[2];
        if (p.labels_out && p.per_point) p.labels_out[o] = valid ? row_label(p.labels, p.label_bytes, (size_t)s * p.Nsrc + i) : -1;
        if (p.order_out) p.order_out[o] = i;
    }
    __syncthreads();
    const int cnt = N - r0 < kProviderTile ? N - r0 : kProviderTile;
    float *pts = p.points + ((size_t)b * N + r0) * 3;
    for (int e = tid; e < cnt * 3; e += kProviderTile) pts[e] = xyz_s[e];
    float *inp = p.input + ((size_t)b * N + r0) * K;
    const float *src = valid ? p.data + (size_t)s * p.Nsrc * K : nullptr;
    for (int e = tid; e < cnt * K; e += kProviderTile) {
        const int q = e / K, c = e - q * K;
        inp[e] = c < 3 ? xyz_s[3 * q + c] : (valid ? src[(size_t)idx_s[q] * K + c] : 0.0f);
    }
}

}  // namespace conv3p
