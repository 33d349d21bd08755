// conv3p_provider.hpp -- one batch of the reference's data providers as ONE launch.
//
// What the providers do on the host for every batch, with numpy, per cloud:
//   modelnet_provider.py:171-219   slice the file's clouds to num_points rows, shuffle, then per batch: rotate, jitter,
//                                  optional sort, copy into batch_points / batch_input / batch_label (uint8)
//   scene_seg/s3dis_provider.py:80-118, scene_seg/scenenn_provider.py:67-105
//                                  the epoch's permutation, then per batch: optional sort of rows AND per-point labels,
//                                  points = rows[:, :, 0:3], input = rows, labels
//   util.py:55-109                 sort_point_cloud_xyz / sort_point_cloud_xyz2
// Here the data set is resident on the device; a batch is assembled from it by
//
//   provider_flat_kernel   (no sort)  a workgroup owns 256 consecutive rows of one cloud: B * ceil(N / 256) workgroups,
//                                     so the grid follows the bytes, not the number of clouds.  The augmented xyz of the
//                                     tile is staged in LDS (3 KB) so that points and input are written, and the source's
//                                     further channels read, as consecutive words by consecutive lanes.
//   provider_sort_kernel   (sort)     a workgroup owns a cloud, as sort_xyz_kernel: the augmented xyz of every source row
//                                     goes to the workspace (12 bytes a row) and its key to LDS (16 bytes a row, 128 KB
//                                     at N = 8192: the rows themselves do not fit beside it in 160 KB), the keys are
//                                     sorted by sort_xyz_kernel's network, and row r of the outputs takes xyz from the
//                                     workspace row keys[r].idx -- written by this workgroup before the barrier, so it is
//                                     read back from L2 -- and the other channels and the label from the source.  The
//                                     key is not inverted instead: it has lost -0.0's sign and a NaN's payload.
//                                     provider_sort_kernel<true> is the Morton order (sort_method "morton",
//                                     modelnet_provider.py:202-208): the same passes on make_morton_key's 8-byte keys
//                                     (64 KB at N = 8192), after a pass of their own for the augmented rows' box.
//
// Rotation and jitter are augment_point (conv3p_prestep.hpp), the sort is make_sort_key or make_morton_key and
// bitonic_sort_keys of the same file.  No memset, no atomic on global memory: every output word is written once by a
// plain store.
//
// Sample of cloud b: s = perm[start + b] (perm == NULL: start + b).  s outside [0, S) is never used as an index: the
// cloud's rows are zero, its labels -1 (ignored by both heads), and workgroup 0 counts such clouds into bad_index[0].
//
// Random draws (neither cos_sin nor noise given), Philox4x32-10 under key (seed low, seed high):
//   angle of sample s      counter (s, 0xFFFFFFFF, step low, step high); u = ((w0 >> 5) 2^26 + (w1 >> 6)) 2^-53;
//                          angle = (u * 2) * pi  (np.random.uniform() * 2 * np.pi, modelnet_provider.py:33)
//   jitter of row i of s   counter (i, s + 1, step low, step high); u1 = (w0 + 1) 2^-32, u2 = w1 2^-32,
//                          u3 = (w2 + 1) 2^-32, u4 = w3 2^-32; Box-Muller in double:
//                          n_x = sqrt(-2 log u1) cos(2 pi u2), n_y = sqrt(-2 log u1) sin(2 pi u2),
//                          n_z = sqrt(-2 log u3) cos(2 pi u4)
// Functions of (seed, step, s, i) only -- not of the cloud's place in the batch.  The dropout mask of
// conv3p_cls_tail.hpp uses counters whose second word is 0; here it is s + 1 >= 1 (S <= 2^31) or 0xFFFFFFFF.
#pragma once

#include <type_traits>

#include "conv3p_cls_tail.hpp"
#include "conv3p_prestep.hpp"
#include "conv3p_workgroup.hpp"

namespace conv3p {

constexpr int kProviderTile = 256;          // rows per workgroup of provider_flat_kernel (= its threads)
constexpr int kProviderMaxSortN = 8192;

struct ProviderArgs {
    const float *data;                 // (S, Nsrc, K)
    const void *labels;                // (S) or (S, Nsrc), label_bytes each; may be NULL
    const int32_t *perm;               // may be NULL
    const double2 *cos_sin;            // (B) given; NULL: drawn
    const double *noise;               // (B, N, 3) given; NULL: drawn
    long long start;
    int S, Nsrc, K, B, N;
    int label_bytes, per_point, rotate, jitter;
    double sigma, clip;
    unsigned seed_lo, seed_hi, step_lo, step_hi;
    float *points, *input;
    int32_t *labels_out;               // may be NULL
    double2 *cos_sin_out;              // may be NULL
    double *noise_out;                 // may be NULL, source-row order
    int32_t *order_out;                // may be NULL
    int32_t *bad_index;                // one word
    float *stage;                      // workspace (B, N, 3): provider_sort_kernel only
};

__device__ __forceinline__ long long provider_sample(const ProviderArgs &p, int b)
{
    return p.perm ? (long long)p.perm[p.start + b] : p.start + b;
}

__device__ __forceinline__ double2 provider_draw_cos_sin(const ProviderArgs &p, unsigned s)
{
    const Philox4 w = philox4x32_10(s, 0xFFFFFFFFu, p.step_lo, p.step_hi, p.seed_lo, p.seed_hi);
    const double u = ((double)(w.w[0] >> 5) * 67108864.0 + (double)(w.w[1] >> 6)) * 0x1p-53;
    const double angle = (u * 2.0) * 3.141592653589793;
    return make_double2(cos(angle), sin(angle));
}

__device__ __forceinline__ void provider_draw_normals(const ProviderArgs &p, unsigned s, unsigned i, double n[3])
{
    const Philox4 w = philox4x32_10(i, s + 1u, p.step_lo, p.step_hi, p.seed_lo, p.seed_hi);
    const double u1 = ((double)w.w[0] + 1.0) * 0x1p-32, u2 = (double)w.w[1] * 0x1p-32;
    const double u3 = ((double)w.w[2] + 1.0) * 0x1p-32, u4 = (double)w.w[3] * 0x1p-32;
    const double r = sqrt(-2.0 * log(u1)), a = 6.283185307179586 * u2;
    n[0] = r * cos(a);
    n[1] = r * sin(a);
    n[2] = sqrt(-2.0 * log(u3)) * cos(6.283185307179586 * u4);
}

// Thread 0 of a workgroup of cloud b: {cos, sin} of the cloud -> *cs_s.  `first`: this workgroup also writes the cloud's
// cos_sin_out and, with one label per sample, its label.
__device__ __forceinline__ void provider_cloud_head(const ProviderArgs &p, int b, long long s, bool valid, bool first,
                                                    double2 *cs_s)
{
    double2 t = make_double2(1.0, 0.0);
    if (p.rotate) {
        if (p.cos_sin) t = p.cos_sin[b];
        else if (valid) t = provider_draw_cos_sin(p, (unsigned)s);
    }
    *cs_s = t;
    if (!first) return;
    if (p.cos_sin_out) p.cos_sin_out[b] = t;
    if (p.labels_out && !p.per_point) p.labels_out[b] = valid ? row_label(p.labels, p.label_bytes, (size_t)s) : -1;
}

// Source row i of cloud b (sample s) -> its augmented xyz; noise_out.  An invalid sample reads nothing and gives zeros.
__device__ __forceinline__ void provider_row(const ProviderArgs &p, int b, long long s, bool valid, int i, double2 t,
                                             float r[3])
{
    const size_t o = (size_t)b * p.N + i;
    double n[3] = {0.0, 0.0, 0.0};
    if (p.jitter) {
        if (p.noise) {
            n[0] = p.noise[3 * o];
            n[1] = p.noise[3 * o + 1];
            n[2] = p.noise[3 * o + 2];
        } else if (valid) {
            provider_draw_normals(p, (unsigned)s, (unsigned)i, n);
        }
    }
    if (p.noise_out) {
        p.noise_out[3 * o] = n[0];
        p.noise_out[3 * o + 1] = n[1];
        p.noise_out[3 * o + 2] = n[2];
    }
    r[0] = r[1] = r[2] = 0.0f;
    if (valid) {
        const float *src = p.data + ((size_t)s * p.Nsrc + i) * p.K;
        augment_point(src[0], src[1], src[2], p.rotate != 0, t, p.jitter != 0, n, p.sigma, p.clip, r);
    }
}

// Workgroup 0: how many of the batch's clouds have a sample index outside [0, S) -> bad_index[0].  The sum is of
// integers in LDS; the word is stored once.
__device__ __forceinline__ void provider_count_bad(const ProviderArgs &p, int *bad_s, int tid, int nthr)
{
    int c = 0;
    for (int b = tid; b < p.B; b += nthr) {
        const long long s = provider_sample(p, b);
        c += (s < 0 || s >= p.S) ? 1 : 0;
    }
    if (c) atomicAdd(bad_s, c);
    __syncthreads();
    if (tid == 0) p.bad_index[0] = *bad_s;
}

__global__ __launch_bounds__(kProviderTile) void provider_flat_kernel(const ProviderArgs p, int tiles)
{
    __shared__ float xyz_s[kProviderTile * 3];
    __shared__ double2 cs_s;
    __shared__ int bad_s;
    const int tid = threadIdx.x, b = (int)(blockIdx.x / (unsigned)tiles), tile = (int)(blockIdx.x % (unsigned)tiles);
    const int i0 = tile * kProviderTile, N = p.N, K = p.K;
    const long long s = provider_sample(p, b);
    const bool valid = s >= 0 && s < p.S;
    if (tid == 0) {
        bad_s = 0;
        provider_cloud_head(p, b, s, valid, tile == 0, &cs_s);
    }
    __syncthreads();
    if (blockIdx.x == 0) provider_count_bad(p, &bad_s, tid, kProviderTile);
    const int i = i0 + tid;
    if (i < N) {
        float r[3];
        provider_row(p, b, s, valid, i, cs_s, r);
        xyz_s[3 * tid] = r[0];
        xyz_s[3 * tid + 1] = r[1];
        xyz_s[3 * tid + 2] = r[2];
        const size_t o = (size_t)b * N + i;
        if (p.labels_out && p.per_point) p.labels_out[o] = valid ? row_label(p.labels, p.label_bytes, (size_t)s * p.Nsrc + i) : -1;
        if (p.order_out) p.order_out[o] = i;
    }
    __syncthreads();
    const int cnt = N - i0 < kProviderTile ? N - i0 : kProviderTile;
    float *pts = p.points + ((size_t)b * N + i0) * 3;
    for (int e = tid; e < cnt * 3; e += kProviderTile) pts[e] = xyz_s[e];
    float *inp = p.input + ((size_t)b * N + i0) * K;
    const float *src = valid ? p.data + ((size_t)s * p.Nsrc + i0) * K : nullptr;
    for (int e = tid; e < cnt * K; e += kProviderTile) {
        const int r = e / K, c = e - r * K;
        inp[e] = c < 3 ? xyz_s[3 * r + c] : (valid ? src[e] : 0.0f);
    }
}

// MORTON: the keys are make_morton_key's (8 bytes a row) instead of make_sort_key's (16).  The box of the AUGMENTED
// rows has to be known before the first key, so the pass that stages the rows reduces the box and a second pass, behind
// the barrier, builds the keys from the staged rows -- a lane reads back the rows it wrote itself.  MORTON = false is
// the kernel as it was: none of its statements depends on the parameter.
template <bool MORTON>
__global__ __launch_bounds__(1024) void provider_sort_kernel(const ProviderArgs p, int npad)
{
    using Key = typename std::conditional<MORTON, uint64_t, SortKey>::type;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ double2 cs_s;
    __shared__ int bad_s;
    Key *keys = reinterpret_cast<Key *>(smem);
    const int tid = threadIdx.x, nthr = blockDim.x, b = blockIdx.x, N = p.N, K = p.K;
    const long long s = provider_sample(p, b);
    const bool valid = s >= 0 && s < p.S;
    if (tid == 0) {
        bad_s = 0;
        provider_cloud_head(p, b, s, valid, true, &cs_s);
    }
    __syncthreads();
    if (b == 0) provider_count_bad(p, &bad_s, tid, nthr);
    float *stage = p.stage + (size_t)b * N * 3;
    const double2 t = cs_s;
    if constexpr (MORTON) {
        __shared__ float box_s[16 * 6];
        MortonRange rg;
        morton_range_init(rg);
        for (int i = tid; i < N; i += nthr) {
            float r[3];
            provider_row(p, b, s, valid, i, t, r);
            stage[3 * i] = r[0];
            stage[3 * i + 1] = r[1];
            stage[3 * i + 2] = r[2];
            morton_range_add(rg, r[0], r[1], r[2]);
        }
        __threadfence_block();           // for the epilogue's gather, which reads rows other lanes staged (the key pass
                                         // below reads only the lane's own rows: both loops walk i = tid + k * nthr)
        const MortonBox box = morton_box_reduce(rg, box_s, tid, nthr);
        for (int i = tid; i < npad; i += nthr) {
            uint64_t k = kMortonPadKey;
            if (i < N) k = make_morton_key(stage[3 * i], stage[3 * i + 1], stage[3 * i + 2], i, box);
            keys[i] = k;
        }
        __syncthreads();
        bitonic_sort_keys<uint64_t, MortonLess>(keys, npad, tid, nthr);
    } else {
        for (int i = tid; i < npad; i += nthr) {
            SortKey k{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};   // padding sorts last
            if (i < N) {
                float r[3];
                provider_row(p, b, s, valid, i, t, r);
                stage[3 * i] = r[0];
                stage[3 * i + 1] = r[1];
                stage[3 * i + 2] = r[2];
                k = make_sort_key(r[0], r[1], r[2], i);
            }
            keys[i] = k;
        }
        __threadfence_block();               // the staged rows are read back below by other lanes of this workgroup
        __syncthreads();
        bitonic_sort_keys<SortKey, KeyLess>(keys, npad, tid, nthr);
    }
    auto row_of = [&](int r) -> uint32_t {
        if constexpr (MORTON) return (uint32_t)(keys[r] & 0xFFFFu);
        else return keys[r].idx;
    };
    float *pts = p.points + (size_t)b * N * 3;
    for (int e = tid; e < N * 3; e += nthr) {
        const int r = e / 3, c = e - r * 3;
        pts[e] = stage[3 * (size_t)row_of(r) + c];
    }
    float *inp = p.input + (size_t)b * N * K;
    const float *src = valid ? p.data + (size_t)s * p.Nsrc * K : nullptr;
    for (int e = tid; e < N * K; e += nthr) {
        const int r = e / K, c = e - r * K;
        const size_t i = row_of(r);
        inp[e] = c < 3 ? stage[3 * i + c] : (valid ? src[i * K + c] : 0.0f);
    }
    for (int r = tid; r < N; r += nthr) {
        const int i = (int)row_of(r);
        const size_t o = (size_t)b * N + r;
        if (p.labels_out && p.per_point) p.labels_out[o] = valid ? row_label(p.labels, p.label_bytes, (size_t)s * p.Nsrc + i) : -1;
        if (p.order_out) p.order_out[o] = i;
    }
}

}  // namespace conv3p
