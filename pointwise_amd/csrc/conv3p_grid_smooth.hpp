// conv3p_grid_smooth.hpp -- segments under a smoothness predicate (conv3p_grid_segments_smooth) and exact sums of per-voxel
// values over the segments of any segmentation (conv3p_grid_segment_pool_f32 / _i64).
//
// include/conv3p.h defines both by the rules J1-J5 and P1-P6 and tests/grid_smooth_ref.py restates them in numpy.
//
// conv3p_grid_segments_smooth, seven launches whatever the data behind a 64-byte memset of smooth_stats:
//
//   smooth_local_kernel   gseg_local_body with the rule below: the tile's union-find in LDS over the pairs that pass J2-J4
//   smooth_link_kernel    gseg_link_body with the rule below: the pairs that leave the tile
//   gseg_flatten / scan / number / assign / max            as conv3p_grid_segments launches them
//
//   The two kernels together walk every candidate pair of J1 once (the local one the pairs inside a tile, the link the
//   rest), so the counts of J5 are what their threads saw: seven int32 counters in registers, summed over the wave by
//   shuffles at the kernel's end and added to smooth_stats by lane 0 with 64-bit integer adds.  A voxel's own normal,
//   flag and curvature are read once, in enter(); the neighbour's are read per pair from global memory -- they are rows of
//   12 bytes that the L2 holds, as it holds the labels.  Staging the tile's normals in LDS (12 KB beside the 8 KB of the
//   union-find) was not tried: see DESIGN.md 5k-7.  The predicate is evaluated BEFORE the union and reads no word that a
//   thread of these kernels writes, so the progress argument of conv3p_grid_segments.hpp stands as it is.
//
// conv3p_grid_segment_pool, three launches (four with voxel_label) whatever the data, no workspace:
//
//   pool_init_kernel      sums, weights and pool_stats 0
//   pool_sum_kernel       the shape of geom_moments_kernel.  A wave takes steps * 64 CONSECUTIVE voxels.  First it decides
//                         for each of its voxels whether it contributes (P2: one read of the row), a bit per step; then it
//                         walks the channels in chunks of kPoolChunk: per chunk the runs of equal segment are reduced by
//                         geom_run_step and carried from step to step, and a finished run costs one 64-bit integer atomic
//                         add per channel (and one for the weight, with the first chunk).  Wrapping unsigned arithmetic.
//   pool_finish_kernel    a thread per segment row: P4's mean, P5's label, the two segment counts of P6
//   pool_voxel_kernel     voxel_label (only when it is asked for: seg_label is final behind the kernel boundary)
//
// The only atomics are 64-bit integer adds and the int32 adds through LDS of the counts: no float atomics, nothing depends
// on the launch geometry, on steps or on thread order.
#pragma once

#include "conv3p_grid_geometry.hpp"

namespace conv3p {

constexpr int kSmoothMaxFeatures = 16;
constexpr int kPoolChunk = 8;                            // channels a pass of the runs
constexpr int kPoolMaxChannels = 128;
constexpr double kPoolScale = 1073741824.0;              // 2^30, the fixed point of conv3p_scene_vote_scores_f32

// J2-J5 as the join rule of gseg_local_body / gseg_link_body.
struct SmoothJoin {
    const float *normals;
    const int32_t *flags;
    const float *curvature, *features;
    int F;
    long long feature_stride;
    float min_cos, max_curvature, max_difference;
    int signed_normals;
    unsigned long long *stats;
    // the voxel entered: its normal (has: J2's "has a normal") and whether its curvature passes J3
    float nx, ny, nz;
    bool has, flat;
    int n_pairs, n_joined, n_missing, n_angle, n_curvature, n_features, n_bare;

    __device__ __forceinline__ bool normal_of(int v, float &x, float &y, float &z) const
    {
        x = normals[(size_t)v * 3 + 0];
        y = normals[(size_t)v * 3 + 1];
        z = normals[(size_t)v * 3 + 2];
        const bool flagged = flags && flags[v] != 0;
        return !flagged && isfinite(x) && isfinite(y) && isfinite(z);
    }
    __device__ __forceinline__ void enter(int v)
    {
        nx = ny = nz = 0.0f;
        has = normals ? normal_of(v, nx, ny, nz) : true;
        flat = curvature ? curvature[v] <= max_curvature : true;
    }
    __device__ __forceinline__ void mark() { n_bare += has ? 0 : 1; }
    __device__ __forceinline__ bool join(int v, int u)
    {
        ++n_pairs;                                       // J5: a candidate pair, met once (u < v)
        if (normals) {                                   // J2
            float ux, uy, uz;
            const bool other = normal_of(u, ux, uy, uz);
            if (!has || !other) {
                ++n_missing;
                return false;
            }
            float d = (nx * ux + ny * uy) + nz * uz;
            d = signed_normals ? d : fabsf(d);
            if (!(d >= min_cos)) {
                ++n_angle;
                return false;
            }
        }
        if (curvature && !(flat && curvature[u] <= max_curvature)) {                     // J3
            ++n_curvature;
            return false;
        }
        const float *fv = features + (size_t)v * feature_stride, *fu = features + (size_t)u * feature_stride;
        for (int k = 0; k < F; ++k)                      // J4; F is 0 without features
            if (!(fabsf(fv[k] - fu[k]) <= max_difference)) {
                ++n_features;
                return false;
            }
        ++n_joined;
        return true;
    }
    // Every thread of the kernel, once, at its end: all lanes of a wave arrive together.
    __device__ __forceinline__ void done()
    {
        int n[7] = {n_pairs, n_joined, n_missing, n_angle, n_curvature, n_features, n_bare};
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            for (int d = 32; d > 0; d >>= 1) n[k] += __shfl_xor(n[k], d, 64);
            if ((threadIdx.x & 63) == 0 && n[k])
                (void)__hip_atomic_fetch_add(stats + k, (unsigned long long)n[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
};

__global__ __launch_bounds__(kGsegLocalTile) void smooth_local_kernel(SmoothJoin rule, const int32_t *neigh,
                                                                      const int32_t *voxel_labels, int L,
                                                                      const int32_t *grid_stats, int M, int num_class,
                                                                      unsigned tapmask, int32_t *lab, int32_t *parent,
                                                                      int32_t *seg_root, int32_t *seg_size, int32_t *seg_rows,
                                                                      int32_t *seg_label, int32_t *seg_stats)
{
    gseg_local_body(rule, neigh, voxel_labels, L, grid_stats, M, num_class, tapmask, lab, parent, seg_root, seg_size, seg_rows,
                    seg_label, seg_stats);
}

__global__ __launch_bounds__(kGsegThreads) void smooth_link_kernel(SmoothJoin rule, const int32_t *neigh, const int32_t *lab,
                                                                   int32_t *parent, const int32_t *grid_stats, int M,
                                                                   unsigned tapmask)
{
    gseg_link_body(rule, neigh, lab, parent, grid_stats, M, tapmask);
}

// -------------------------------------------------------------------------------------------------------------- pool
// P2: whether a value may contribute, and its quantum.
__device__ __forceinline__ bool pool_fits(float x) { return fabsf(x) <= 256.0f; }        // false for a NaN and an infinity
__device__ __forceinline__ bool pool_fits(long long) { return true; }
__device__ __forceinline__ unsigned long long pool_quantum(float x)
{
    return (unsigned long long)llrint((double)x * kPoolScale);                            // exact product, to nearest even
}
__device__ __forceinline__ unsigned long long pool_quantum(long long x) { return (unsigned long long)x; }

__global__ __launch_bounds__(kGsegThreads) void pool_init_kernel(int M, int C, unsigned long long *sums,
                                                                 unsigned long long *weights, unsigned long long *pool_stats)
{
    if (blockIdx.x == 0 && threadIdx.x < 4) pool_stats[threadIdx.x] = 0ull;
    const long long words = (long long)M * C;
    for (long long i = (long long)blockIdx.x * kGsegThreads + threadIdx.x; i < words; i += (long long)gridDim.x * kGsegThreads) {
        sums[i] = 0ull;
        if (i < M) weights[i] = 0ull;                    // M <= words
    }
}

template <typename T>
__global__ __launch_bounds__(kGsegThreads) void pool_sum_kernel(const T *values, int L, int C, long long stride,
                                                                const int32_t *segment, const int32_t *seg_stats,
                                                                const int32_t *voxel_count, const int32_t *grid_stats, int M,
                                                                int weight, int steps, unsigned long long *sums,
                                                                unsigned long long *weights, unsigned long long *pool_stats)
{
    using u64 = unsigned long long;
    constexpr int kNV = kPoolChunk + 1;                  // the chunk's channels and the weight
    const int ne = clamped_count(grid_stats, M), S = clamped_count(seg_stats, M);
    const int tid = threadIdx.x, lane = tid & 63;
    const long long chunk = 64ll * steps, waves = (long long)gridDim.x * (kGsegThreads / 64);
    auto op = [](int, u64 a, u64 b) { return a + b; };
    int n_in = 0, n_out = 0;
    for (long long c0 = ((long long)blockIdx.x * (kGsegThreads / 64) + (tid >> 6)) * chunk; c0 < M; c0 += waves * chunk) {
        unsigned contributes = 0;                        // bit j: the lane's voxel of step j (steps <= 16)
        for (int j = 0; j < steps; ++j) {
            const long long w = c0 + 64ll * j + lane;    // c0 and j are the wave's: all its lanes take every step
            if (w - lane >= M) break;
            if (w >= M || geom_member(segment, w, ne, S) < 0) continue;
            bool good = w < L;
            if (good) {
                const T *row = values + (size_t)w * stride;
                for (int c = 0; c < C; ++c) good = good && pool_fits(row[c]);
            }
            contributes |= (good ? 1u : 0u) << j;
            n_in += good ? 1 : 0;
            n_out += good ? 0 : 1;
        }
        for (int cc = 0; cc < C; cc += kPoolChunk) {     // uniform
            auto flush = [=](int s, const u64 (&x)[kNV]) {
#pragma unroll
                for (int k = 0; k < kPoolChunk; ++k)
                    if (cc + k < C && x[k])
                        (void)__hip_atomic_fetch_add(sums + (size_t)s * C + cc + k, x[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (cc == 0 && x[kPoolChunk])
                    (void)__hip_atomic_fetch_add(weights + s, x[kPoolChunk], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            };
            int cs = -1;
            u64 cx[kNV];
#pragma unroll
            for (int k = 0; k < kNV; ++k) cx[k] = 0ull;
            for (int j = 0; j < steps; ++j) {
                const long long w = c0 + 64ll * j + lane;
                if (w - lane >= M) break;
                const int s = ((contributes >> j) & 1u) ? segment[w] : -1;        // a contributor is a member: G1 held
                u64 x[kNV];
#pragma unroll
                for (int k = 0; k < kNV; ++k) x[k] = 0ull;
                if (s >= 0) {
                    const T *row = values + (size_t)w * stride + cc;
                    const u64 wt = weight ? (u64)(long long)voxel_count[w] : 1ull;
#pragma unroll
                    for (int k = 0; k < kPoolChunk; ++k)
                        if (cc + k < C) x[k] = wt * pool_quantum(row[k]);
                    x[kPoolChunk] = wt;
                }
                geom_run_step<kNV>(lane, s, x, cs, cx, op, flush);
            }
            if (lane == 0 && cs >= 0) flush(cs, cx);
        }
    }
    for (int d = 32; d > 0; d >>= 1) {
        n_in += __shfl_xor(n_in, d, 64);
        n_out += __shfl_xor(n_out, d, 64);
    }
    if (lane == 0) {
        if (n_in) (void)__hip_atomic_fetch_add(pool_stats + 0, (u64)n_in, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (n_out) (void)__hip_atomic_fetch_add(pool_stats + 1, (u64)n_out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(kGsegThreads) void pool_finish_kernel(const int32_t *seg_stats, int M, int C, const long long *sums,
                                                                   const long long *weights, double *mean, int32_t *seg_label,
                                                                   unsigned long long *pool_stats)
{
    __shared__ int count_s[2];
    const int tid = threadIdx.x;
    if (tid < 2) count_s[tid] = 0;
    __syncthreads();
    const int S = clamped_count(seg_stats, M);
    int n_with = 0, n_without = 0;
    for (long long s = (long long)blockIdx.x * kGsegThreads + tid; s < M; s += (long long)gridDim.x * kGsegThreads) {
        const long long W = weights[s];
        const long long *row = sums + s * C;
        const double scale = (double)W * kPoolScale;     // exact: a power of two
        int best = 0;
        long long most = row[0];
        bool any = most != 0;
        for (int c = 0; c < C; ++c) {
            const long long n = row[c];
            if (mean) mean[s * C + c] = W != 0 ? (double)n / scale : 0.0;                 // P4
            any = any || n != 0;
            if (n > most) {                              // P5: a later class only when strictly greater
                most = n;
                best = c;
            }
        }
        const int label = (W != 0 && any) ? best : -1;
        seg_label[s] = label;
        if (s < S) {
            n_with += label >= 0 ? 1 : 0;
            n_without += label >= 0 ? 0 : 1;
        }
    }
    if (n_with) atomicAdd(&count_s[0], n_with);
    if (n_without) atomicAdd(&count_s[1], n_without);
    __syncthreads();
    if (tid < 2 && count_s[tid])
        (void)__hip_atomic_fetch_add(pool_stats + 2 + tid, (unsigned long long)count_s[tid], __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kGsegThreads) void pool_voxel_kernel(const int32_t *segment, const int32_t *seg_stats,
                                                                  const int32_t *grid_stats, int M, const int32_t *seg_label,
                                                                  int32_t *voxel_label)
{
    const int ne = clamped_count(grid_stats, M), S = clamped_count(seg_stats, M);
    for (long long w = (long long)blockIdx.x * kGsegThreads + threadIdx.x; w < M; w += (long long)gridDim.x * kGsegThreads) {
        const int s = geom_member(segment, w, ne, S);
        voxel_label[w] = s >= 0 ? seg_label[s] : -1;
    }
}

}  // namespace conv3p
