// conv3p_grid_geometry.hpp -- per-segment geometry of a segmentation of the voxel grid: the box of the members' cells and
// of their representatives, the exact integer moments of the cells, the centroid, the principal axes and the oriented
// extents (conv3p_grid_segment_geometry).
//
// include/conv3p.h defines the result by the rules G1-G8 and tests/grid_geometry_ref.py restates them in numpy.  The call
// has no workspace: every accumulator is the output word it ends up in.  cell_box and moments are accumulated as what they
// are; box and extent are accumulated as ORDERED KEYS -- the float's bits b as a signed integer, b for b >= 0 and
// b ^ 0x7fff... otherwise, whose signed order is the unsigned order of G3's key -- and turned back into floats by the last
// launch (the map is its own inverse).  Six launches whatever the data:
//
//   geom_init_kernel      a thread per segment row: the identities of min / max / add in every accumulator, the stats 0
//   geom_box_kernel       G2, G3.  The shape of gseg_assign_kernel: a wave takes steps * 64 CONSECUTIVE voxels, reduces runs
//                         of equal segment by a segmented shuffle and carries the open run in registers from step to step;
//                         a run is sent to memory when it ends -- 12 integer atomic min / max a run, not a voxel.  Voxels
//                         are numbered in ascending cell, so a floor that is one segment is one run per chunk.
//   geom_moments_kernel   G4, behind the kernel boundary that makes the low corners final: the same runs over ten unsigned
//                         64-bit sums, ten 64-bit integer atomic adds a run
//   geom_frame_kernel     G5-G7, a thread per segment as grid_normals_kernel has one per voxel: the centroid by one division
//                         and one addition, the covariance, kNormalsSweeps cyclic Jacobi sweeps in float64 by
//                         normals_rotate, every rotation taken and every loop unrolled (no array is indexed at run time:
//                         no private segment), the three pairs ordered by selects, each axis normalised and turned; the
//                         two counts of the stats by integer adds through LDS
//   geom_extent_kernel    G8 from the STORED centroid and axes: the runs over six 64-bit keys, six atomic min / max a run
//   geom_finish_kernel    keys -> floats in box and extent, the filler rows, stats[0]
//
// The only atomics are integer min / max on 32- and 64-bit words and 64-bit integer adds: no float atomics, and nothing
// depends on the launch geometry, on steps or on thread order.  The library is built with -ffp-contract=off, so every
// float64 operation of G5, G6 and G8 is one separately rounded operation.
#pragma once

#include "conv3p_grid_normals.hpp"
#include "conv3p_grid_segments.hpp"

namespace conv3p {

constexpr int kGeomBoxWords = 12;      // cell min 3, cell max 3, box key min 3, box key max 3
constexpr int kGeomMoments = 10;
constexpr int kGeomExtentWords = 6;

// The ordered key of a float's bits and back: one map, its own inverse.
__device__ __forceinline__ int geom_key32(int b) { return b >= 0 ? b : b ^ 0x7fffffff; }
__device__ __forceinline__ long long geom_key64(long long b) { return b >= 0 ? b : b ^ 0x7fffffffffffffffll; }

// G1: the segment of voxel w as a member, -1 for a member of nothing.
__device__ __forceinline__ int geom_member(const int32_t *segment, long long w, int ne, int S)
{
    if (w >= ne) return -1;
    const int s = segment[w];
    return (s >= 0 && s < S) ? s : -1;
}

// One step of a wave over 64 consecutive voxels.  s is the lane's segment (-1: none), x its kNV values; op(k, a, b)
// combines two values of component k and flush(s, x) sends a finished run to memory from ONE lane.  Runs of equal s are
// reduced by a segmented shuffle into the run's first lane; (cs, cx) is the run left open by the steps before, the same
// in every lane, and takes the step's first run when that continues it.  Every lane of the wave takes every step.
template <int kNV, typename T, typename Op, typename Flush>
__device__ __forceinline__ void geom_run_step(int lane, int s, T (&x)[kNV], int &cs, T (&cx)[kNV], Op op, Flush flush)
{
    const int before = __shfl_up(s, 1, 64);
    const bool head = lane == 0 || before != s;
    const unsigned long long heads = __ballot(head);
    const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
    const int end = above ? lane + __ffsll((long long)above) : 64;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
#pragma unroll
        for (int k = 0; k < kNV; ++k) {
            const T y = __shfl_down(x[k], d, 64);
            x[k] = lane + d < end ? op(k, x[k], y) : x[k];
        }
    }
    const int last = 63 - __clzll((long long)heads);     // the head of the step's last run; lane 0 is a head
    const int s0 = __shfl(s, 0, 64);
    T x0[kNV];
#pragma unroll
    for (int k = 0; k < kNV; ++k) x0[k] = __shfl(x[k], 0, 64);
    if (s0 == cs) {                                      // the carried run goes on
#pragma unroll
        for (int k = 0; k < kNV; ++k) cx[k] = op(k, cx[k], x0[k]);
    } else {
        if (lane == 0 && cs >= 0) flush(cs, cx);
        cs = s0;
#pragma unroll
        for (int k = 0; k < kNV; ++k) cx[k] = x0[k];
    }
    if (last != 0) {                                     // it ends inside this step: flush it and the runs in between
        if (lane == 0 && cs >= 0) flush(cs, cx);
        if (head && lane != 0 && lane != last && s >= 0) flush(s, x);
        cs = __shfl(s, last, 64);
#pragma unroll
        for (int k = 0; k < kNV; ++k) cx[k] = __shfl(x[k], last, 64);
    }
}

__global__ __launch_bounds__(kGsegThreads) void geom_init_kernel(int M, int32_t *cell_box, int32_t *box_key,
                                                                 unsigned long long *moments, long long *extent_key,
                                                                 int32_t *geometry_stats)
{
    if (blockIdx.x == 0 && threadIdx.x < 4) geometry_stats[threadIdx.x] = 0;
    for (long long s = (long long)blockIdx.x * kGsegThreads + threadIdx.x; s < M; s += (long long)gridDim.x * kGsegThreads) {
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            cell_box[s * 6 + k] = k < 3 ? INT32_MAX : INT32_MIN;
            box_key[s * 6 + k] = k < 3 ? INT32_MAX : INT32_MIN;
            extent_key[s * 6 + k] = k < 3 ? INT64_MAX : INT64_MIN;
        }
#pragma unroll
        for (int k = 0; k < kGeomMoments; ++k) moments[s * kGeomMoments + k] = 0ull;
    }
}

// The chunks of a wave: c0 runs over the starts of the wave's chunks of 64 * steps voxels.
#define GEOM_WAVE_CHUNKS(c0, M, steps)                                                                                       \
    const int tid = threadIdx.x, lane = tid & 63;                                                                            \
    const long long chunk = 64ll * (steps), waves = (long long)gridDim.x * (kGsegThreads / 64);                              \
    for (long long c0 = ((long long)blockIdx.x * (kGsegThreads / 64) + (tid >> 6)) * chunk; c0 < (M); c0 += waves * chunk)

__global__ __launch_bounds__(kGsegThreads) void geom_box_kernel(const float *voxel_data, int K, const int32_t *voxel_cell,
                                                                const int32_t *segment, const int32_t *seg_stats,
                                                                const int32_t *grid_stats, int M, int steps, int32_t *cell_box,
                                                                int32_t *box_key)
{
    const int ne = clamped_count(grid_stats, M), S = clamped_count(seg_stats, M);
    auto op = [](int k, int a, int b) { return (k % 6) < 3 ? (a < b ? a : b) : (a > b ? a : b); };
    auto flush = [=](int s, const int (&x)[kGeomBoxWords]) {
#pragma unroll
        for (int k = 0; k < kGeomBoxWords; ++k) {
            int32_t *p = (k < 6 ? cell_box : box_key) + (size_t)s * 6 + (k % 6);
            if ((k % 6) < 3) (void)__hip_atomic_fetch_min(p, x[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else (void)__hip_atomic_fetch_max(p, x[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    };
    GEOM_WAVE_CHUNKS(c0, M, steps) {
        int cs = -1, cx[kGeomBoxWords];
#pragma unroll
        for (int k = 0; k < kGeomBoxWords; ++k) cx[k] = 0;
        for (int j = 0; j < steps; ++j) {
            const long long w = c0 + 64ll * j + lane;    // c0 and j are the wave's: all its lanes take every step
            if (w - lane >= M) break;
            const int s = w < M ? geom_member(segment, w, ne, S) : -1;
            int x[kGeomBoxWords];
#pragma unroll
            for (int k = 0; k < kGeomBoxWords; ++k) x[k] = 0;
            if (s >= 0) {
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    const int c = voxel_cell[w * 3 + a];
                    const int b = geom_key32(__float_as_int(voxel_data[(size_t)w * K + a]));
                    x[a] = c; x[3 + a] = c; x[6 + a] = b; x[9 + a] = b;
                }
            }
            geom_run_step<kGeomBoxWords>(lane, s, x, cs, cx, op, flush);
        }
        if (lane == 0 && cs >= 0) flush(cs, cx);
    }
}

__global__ __launch_bounds__(kGsegThreads) void geom_moments_kernel(const int32_t *voxel_cell, const int32_t *voxel_count,
                                                                    const int32_t *segment, const int32_t *seg_stats,
                                                                    const int32_t *grid_stats, int M, int weight, int steps,
                                                                    const int32_t *cell_box, unsigned long long *moments)
{
    using u64 = unsigned long long;
    const int ne = clamped_count(grid_stats, M), S = clamped_count(seg_stats, M);
    auto op = [](int, u64 a, u64 b) { return a + b; };
    auto flush = [=](int s, const u64 (&x)[kGeomMoments]) {
#pragma unroll
        for (int k = 0; k < kGeomMoments; ++k)
            (void)__hip_atomic_fetch_add(moments + (size_t)s * kGeomMoments + k, x[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    GEOM_WAVE_CHUNKS(c0, M, steps) {
        int cs = -1;
        u64 cx[kGeomMoments];
#pragma unroll
        for (int k = 0; k < kGeomMoments; ++k) cx[k] = 0ull;
        for (int j = 0; j < steps; ++j) {
            const long long w = c0 + 64ll * j + lane;
            if (w - lane >= M) break;
            const int s = w < M ? geom_member(segment, w, ne, S) : -1;
            u64 x[kGeomMoments];
#pragma unroll
            for (int k = 0; k < kGeomMoments; ++k) x[k] = 0ull;
            if (s >= 0) {                                // the low corner is final: the box pass ended a launch ago
                const int32_t *lo = cell_box + (size_t)s * 6;
                const u64 dx = (u64)((long long)voxel_cell[w * 3 + 0] - (long long)lo[0]);
                const u64 dy = (u64)((long long)voxel_cell[w * 3 + 1] - (long long)lo[1]);
                const u64 dz = (u64)((long long)voxel_cell[w * 3 + 2] - (long long)lo[2]);
                const u64 wt = weight ? (u64)(long long)voxel_count[w] : 1ull;
                x[0] = wt; x[1] = wt * dx; x[2] = wt * dy; x[3] = wt * dz;
                x[4] = x[1] * dx; x[5] = x[1] * dy; x[6] = x[1] * dz; x[7] = x[2] * dy; x[8] = x[2] * dz; x[9] = x[3] * dz;
            }
            geom_run_step<kGeomMoments>(lane, s, x, cs, cx, op, flush);
        }
        if (lane == 0 && cs >= 0) flush(cs, cx);
    }
}

// The pairs (la, column a) and (lb, column b) in descending eigenvalue; equal ones keep their places.
__device__ __forceinline__ void geom_order(double &la, double &lb, double &a0, double &a1, double &a2, double &b0, double &b1,
                                           double &b2)
{
    const bool sw = lb > la;
    const double tl = la, t0 = a0, t1 = a1, t2 = a2;
    la = sw ? lb : la; a0 = sw ? b0 : a0; a1 = sw ? b1 : a1; a2 = sw ? b2 : a2;
    lb = sw ? tl : lb; b0 = sw ? t0 : b0; b1 = sw ? t1 : b1; b2 = sw ? t2 : b2;
}

// G6's unit length and G7's sign on one axis.
__device__ __forceinline__ void geom_axis(double &x, double &y, double &z)
{
    const double len = sqrt((x * x + y * y) + z * z);
    x = x / len; y = y / len; z = z / len;
    const double ax = fabs(x), ay = fabs(y), az = fabs(z);
    const double top = (ax >= ay && ax >= az) ? x : (ay >= az ? y : z);
    if (top < 0.0) { x = -x; y = -y; z = -z; }
}

__global__ __launch_bounds__(kGsegThreads) void geom_frame_kernel(const int32_t *seg_stats, int M, const int32_t *cell_box,
                                                                  const long long *moments, double *centroid,
                                                                  double *eigenvalues, double *axes, int32_t *geometry_stats)
{
    __shared__ int count_s[2];
    const int tid = threadIdx.x;
    if (tid < 2) count_s[tid] = 0;
    __syncthreads();
    const int S = clamped_count(seg_stats, M);
    int n_one = 0, n_flat = 0;
    for (long long s = (long long)blockIdx.x * kGsegThreads + tid; s < M; s += (long long)gridDim.x * kGsegThreads) {
        double c0 = 0.0, c1 = 0.0, c2 = 0.0, l0 = 0.0, l1 = 0.0, l2 = 0.0;
        double v00 = 0.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 0.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 0.0;
        const long long *mo = moments + s * kGeomMoments;
        const long long W = s < S ? mo[0] : 0ll;
        if (W != 0) {
            const int32_t *bx = cell_box + s * 6;
            const double dw = (double)W;
            const double e0 = (double)mo[1] / dw, e1 = (double)mo[2] / dw, e2 = (double)mo[3] / dw;
            c0 = (double)bx[0] + e0; c1 = (double)bx[1] + e1; c2 = (double)bx[2] + e2;                      // G5
            double a00 = (double)mo[4] / dw - e0 * e0, a01 = (double)mo[5] / dw - e0 * e1, a02 = (double)mo[6] / dw - e0 * e2;
            double a11 = (double)mo[7] / dw - e1 * e1, a12 = (double)mo[8] / dw - e1 * e2, a22 = (double)mo[9] / dw - e2 * e2;
            v00 = 1.0; v11 = 1.0; v22 = 1.0;
#pragma unroll
            for (int sweep = 0; sweep < kNormalsSweeps; ++sweep) {                                           // G6
                normals_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
                normals_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
                normals_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
            }
            l0 = a00; l1 = a11; l2 = a22;                // column k of v belongs to l_k
            geom_order(l0, l1, v00, v10, v20, v01, v11, v21);
            geom_order(l1, l2, v01, v11, v21, v02, v12, v22);
            geom_order(l0, l1, v00, v10, v20, v01, v11, v21);
            l0 = l0 < 0.0 ? 0.0 : l0; l1 = l1 < 0.0 ? 0.0 : l1; l2 = l2 < 0.0 ? 0.0 : l2;
            geom_axis(v00, v10, v20);                                                                        // G7
            geom_axis(v01, v11, v21);
            geom_axis(v02, v12, v22);
            n_one += bx[0] == bx[3] && bx[1] == bx[4] && bx[2] == bx[5];
            n_flat += l2 == 0.0;
        }
        centroid[s * 3 + 0] = c0; centroid[s * 3 + 1] = c1; centroid[s * 3 + 2] = c2;
        eigenvalues[s * 3 + 0] = l0; eigenvalues[s * 3 + 1] = l1; eigenvalues[s * 3 + 2] = l2;
        double *ax = axes + s * 9;                       // row k: the eigenvector of l_k, column k of v
        ax[0] = v00; ax[1] = v10; ax[2] = v20;
        ax[3] = v01; ax[4] = v11; ax[5] = v21;
        ax[6] = v02; ax[7] = v12; ax[8] = v22;
    }
    if (n_one) atomicAdd(&count_s[0], n_one);
    if (n_flat) atomicAdd(&count_s[1], n_flat);
    __syncthreads();
    if (tid < 2 && count_s[tid]) atomicAdd(&geometry_stats[1 + tid], count_s[tid]);     // integers: exact in any order
}

__global__ __launch_bounds__(kGsegThreads) void geom_extent_kernel(const int32_t *voxel_cell, const int32_t *segment,
                                                                   const int32_t *seg_stats, const int32_t *grid_stats, int M,
                                                                   int steps, const double *centroid, const double *axes,
                                                                   long long *extent_key)
{
    const int ne = clamped_count(grid_stats, M), S = clamped_count(seg_stats, M);
    auto op = [](int k, long long a, long long b) { return k < 3 ? (a < b ? a : b) : (a > b ? a : b); };
    auto flush = [=](int s, const long long (&x)[kGeomExtentWords]) {
#pragma unroll
        for (int k = 0; k < kGeomExtentWords; ++k) {
            long long *p = extent_key + (size_t)s * 6 + k;
            if (k < 3) (void)__hip_atomic_fetch_min(p, x[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            else (void)__hip_atomic_fetch_max(p, x[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    };
    GEOM_WAVE_CHUNKS(c0, M, steps) {
        int cs = -1;
        long long cx[kGeomExtentWords];
#pragma unroll
        for (int k = 0; k < kGeomExtentWords; ++k) cx[k] = 0ll;
        for (int j = 0; j < steps; ++j) {
            const long long w = c0 + 64ll * j + lane;
            if (w - lane >= M) break;
            const int s = w < M ? geom_member(segment, w, ne, S) : -1;
            long long x[kGeomExtentWords];
#pragma unroll
            for (int k = 0; k < kGeomExtentWords; ++k) x[k] = 0ll;
            if (s >= 0) {                                // G8, on the stored frame
                const double *c = centroid + (size_t)s * 3, *ax = axes + (size_t)s * 9;
                const double qx = (double)voxel_cell[w * 3 + 0] - c[0], qy = (double)voxel_cell[w * 3 + 1] - c[1],
                             qz = (double)voxel_cell[w * 3 + 2] - c[2];
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double p = (qx * ax[3 * k + 0] + qy * ax[3 * k + 1]) + qz * ax[3 * k + 2];
                    x[k] = x[3 + k] = geom_key64(__double_as_longlong(p));
                }
            }
            geom_run_step<kGeomExtentWords>(lane, s, x, cs, cx, op, flush);
        }
        if (lane == 0 && cs >= 0) flush(cs, cx);
    }
}

// box and extent hold keys on entry.  A row past S, or one whose W is 0, is filler.
__global__ __launch_bounds__(kGsegThreads) void geom_finish_kernel(const int32_t *seg_stats, int M, int32_t *cell_box,
                                                                   int32_t *box, long long *moments, long long *extent,
                                                                   int32_t *geometry_stats)
{
    const int S = clamped_count(seg_stats, M);
    if (blockIdx.x == 0 && threadIdx.x == 0) geometry_stats[0] = S;
    for (long long s = (long long)blockIdx.x * kGsegThreads + threadIdx.x; s < M; s += (long long)gridDim.x * kGsegThreads) {
        const bool live = s < S && moments[s * kGeomMoments] != 0ll;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            if (!live) cell_box[s * 6 + k] = k < 3 ? 0 : -1;
            box[s * 6 + k] = live ? geom_key32(box[s * 6 + k]) : 0;
            extent[s * 6 + k] = live ? geom_key64(extent[s * 6 + k]) : 0ll;
        }
        if (!live) {
#pragma unroll
            for (int k = 0; k < kGeomMoments; ++k) moments[s * kGeomMoments + k] = 0ll;
        }
    }
}

#undef GEOM_WAVE_CHUNKS

}  // namespace conv3p
