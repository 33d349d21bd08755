// conv3p_seg_head.hpp -- the per-point loss head of the segmentation model as ONE pass over the logits.
//
//   act (B, N, C) = selu(conv3p(concat, 36 -> num_class))                 (pointcnn_scene_seg_acsd.py:57)
//   loss = mean over all B N points of softmax cross-entropy(act, labels)   (pointcnn_scene_seg_acsd.py:60-71)
// and, after every batch, the statistics of the reference's loops (train_scene_seg_s3dis.py:134-145,
// eval_scene_seg_s3dis.py:88-98): argmax, correct points, per-class seen / correct counts -- there a Python double loop
// over B x N points.  Composed from framework ops this is a dozen launches over the (B N, C) tensor and a host
// synchronisation; here it is
//
//   seg_head_kernel         one read of act, one write of grad_act, pred; one partial record per workgroup
//   seg_head_finish_kernel  the records -> loss_sum (double) and counts (int64), in a fixed order
//
// with no memset, no floating-point atomic and no global atomic: results are bitwise reproducible, and a row's
// gradient and prediction do not depend on the other rows of the call.
//
// Per row r with x = act[r], m = max_c x_c:
//   loss_r = log(sum_c exp(x_c - m)) + m - x_label          (accurate exp / log: no fast-math forms)
//   grad_act[r][c] = (exp(x_c - m) / sum - [c == label]) * grad_scale
//   pred[r] = the FIRST index of the maximum (np.argmax's tie rule): a scan from index 0 that replaces on x > best
// A label outside [0, C) makes an IGNORED row: loss 0, gradient row +0, not counted in seen / correct / predicted,
// counted in `invalid`; the mean's denominator stays B N (that is grad_scale, the caller's).  This is what the
// reference's tf.one_hot of an out-of-range label gives for the loss, and it is how labels are validated here: on the
// device, reported through a counter, without a host synchronisation.
// A row holding a NaN propagates it to loss_sum and to its whole gradient row; its prediction is whatever the x > best
// scan from index 0 leaves (comparisons with NaN are false).  A row whose maximum is +inf yields NaN as well
// (inf - inf); predictions and counters stay exact.
//
// counts[2 + 3 C] = {correct, invalid, seen[C], correct_class[C], predicted[C]}.
//
// Structure.  A wave owns 64 consecutive rows, i.e. 64 C contiguous values (a row of 13 floats is 52 bytes: never
// 16-byte aligned, so rows are not loaded one by one).  The block is copied into LDS with lane-strided, coalesced wave
// loads, into rows of stride ld = C | 1 elements: then lane = row, and the lanes of a half-wave read bank
// (lane * ld + c) mod 32 (fp32; (2 lane ld + 2 c) mod 64 for fp64) -- all different for odd ld.  Pass 1 over the LDS
// row: max and argmax; pass 2: e_c = exp(x_c - m), written back in place, and their sum; pass 3 turns e_c into the
// gradient in place, and the block is stored with the pattern it was loaded with.  The row never lives in registers
// (C is a run-time value: an indexed local array would be a private segment), the counters are LDS integer atomics
// (integer sums do not depend on their order).  A workgroup takes the tiles g, g + gridDim.x, ...; every lane adds its
// rows' losses in that order (double), the wave adds its lanes by a fixed butterfly, the workgroup its waves in wave
// order.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace conv3p {

constexpr int kSegMaxClass = 128;
constexpr int kSegMaxGrid = 1024;      // workgroups (= partial records) of one call at most
constexpr int kSegFinishThreads = 1024;

__host__ __device__ inline int seg_counters(int C) { return 2 + 3 * C; }
// one partial record: {double loss; int32 counters[2 + 3 C]}, padded to 8 bytes
__host__ __device__ inline size_t seg_record_bytes(int C) { return (8 + 4 * (size_t)seg_counters(C) + 7) & ~(size_t)7; }
__host__ __device__ inline int seg_ld(int C) { return C | 1; }
// dynamic LDS of a workgroup of nw waves: wave losses (64 bytes), the tiles, the counters
template <typename T> inline size_t seg_lds_bytes(int nw, int C)
{
    return 64 + (size_t)nw * 64 * seg_ld(C) * sizeof(T) + 4 * (size_t)seg_counters(C);
}

__device__ inline float seg_exp(float x) { return expf(x); }
__device__ inline double seg_exp(double x) { return exp(x); }
__device__ inline float seg_log(float x) { return logf(x); }
__device__ inline double seg_log(double x) { return log(x); }

template <typename T>
__global__ __launch_bounds__(256) void seg_head_kernel(const T *__restrict__ act, const int32_t *__restrict__ labels,
                                                       size_t R, int C, T grad_scale, T *__restrict__ grad_act,
                                                       int32_t *__restrict__ pred, char *__restrict__ partials)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (int)blockDim.x >> 6;
    const int ld = seg_ld(C), nc = seg_counters(C);
    double *wloss = reinterpret_cast<double *>(smem);                               // [nw]
    T *xs = reinterpret_cast<T *>(smem + 64) + (size_t)wave * 64 * ld;              // this wave's [64][ld]
    int *cnt = reinterpret_cast<int *>(smem + 64 + (size_t)nw * 64 * ld * sizeof(T));   // [nc]
    for (int j = threadIdx.x; j < nc; j += (int)blockDim.x) cnt[j] = 0;
    __syncthreads();

    // element e = lane + 64 k of a tile sits at row e / C, column e % C: advanced without a division per element
    const int q64 = 64 / C, r64 = 64 - q64 * C;
    const int row0 = lane / C, col0 = lane - row0 * C;
    const size_t tiles = (R + 63) / 64;
    double lsum = 0.0;
    int ncorrect = 0, ninvalid = 0;

    for (size_t tile = (size_t)blockIdx.x * nw + wave; tile < tiles; tile += (size_t)gridDim.x * nw) {
        const size_t r0 = tile * 64;
        const int nrows = R - r0 < 64 ? (int)(R - r0) : 64;
        const int n = nrows * C;                                                    // <= 64 * 128
        const T *src = act + r0 * C;
        {
            int row = row0, col = col0;
            for (int e = lane; e < n; e += 64) {
                xs[row * ld + col] = src[e];
                row += q64;
                col += r64;
                if (col >= C) { col -= C; ++row; }
            }
        }
        __builtin_amdgcn_wave_barrier();   // (LDS operations of a wave complete in order; this pins the program order)
        if (lane < nrows) {
            T *x = xs + lane * ld;
            const int lab = labels[r0 + lane];
            const bool valid = (unsigned)lab < (unsigned)C;
            T m = x[0];
            int arg = 0;
            for (int c = 1; c < C; ++c) {
                const T v = x[c];
                if (v > m) { m = v; arg = c; }
            }
            if (pred) pred[r0 + lane] = arg;
            if (valid) {
                const T xl = x[lab];
                T s = 0;
                if (grad_act) {
                    for (int c = 0; c < C; ++c) {
                        const T e = seg_exp(x[c] - m);
                        x[c] = e;
                        s += e;
                    }
                    const T inv = T(1) / s;
                    for (int c = 0; c < C; ++c) x[c] = (x[c] * inv - (c == lab ? T(1) : T(0))) * grad_scale;
                } else {
                    for (int c = 0; c < C; ++c) s += seg_exp(x[c] - m);
                }
                lsum += (double)(seg_log(s) + m - xl);
                atomicAdd(&cnt[2 + lab], 1);
                atomicAdd(&cnt[2 + 2 * C + arg], 1);
                if (arg == lab) {
                    atomicAdd(&cnt[2 + C + lab], 1);
                    ++ncorrect;
                }
            } else {
                ++ninvalid;
                if (grad_act)
                    for (int c = 0; c < C; ++c) x[c] = T(0);
            }
        }
        __builtin_amdgcn_wave_barrier();
        if (grad_act) {
            T *dst = grad_act + r0 * C;
            int row = row0, col = col0;
            for (int e = lane; e < n; e += 64) {
                dst[e] = xs[row * ld + col];
                row += q64;
                col += r64;
                if (col >= C) { col -= C; ++row; }
            }
        }
        __builtin_amdgcn_wave_barrier();   // (the next tile's loads overwrite the image)
    }

    // fixed butterfly over the lanes, then the waves in wave order
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) lsum += __shfl_xor(lsum, off, 64);
    if (lane == 0) wloss[wave] = lsum;
    if (ncorrect) atomicAdd(&cnt[0], ncorrect);
    if (ninvalid) atomicAdd(&cnt[1], ninvalid);
    __syncthreads();
    char *rec = partials + (size_t)blockIdx.x * seg_record_bytes(C);
    if (threadIdx.x == 0) {
        double t = wloss[0];
        for (int w = 1; w < nw; ++w) t += wloss[w];
        *reinterpret_cast<double *>(rec) = t;
    }
    int *rc = reinterpret_cast<int *>(rec + 8);
    for (int j = threadIdx.x; j < nc; j += (int)blockDim.x) rc[j] = cnt[j];
}

// loss_sum = the records' losses, counts = the records' counters.  One workgroup of 1024 threads.
// Counters: counter j is summed by S = 1024 / nc threads (records s, s + S, ...: consecutive threads read consecutive
// counters of one record), then over the S slices.  Loss: 256 threads add consecutive runs of records in ascending
// order, 16 threads add 16 consecutive run sums each, thread 0 the 16 results: ascending throughout, one fixed
// association for a given number of records.
__global__ __launch_bounds__(kSegFinishThreads) void seg_head_finish_kernel(const char *__restrict__ partials, int nrec,
                                                                            int C, double *__restrict__ loss_sum,
                                                                            long long *__restrict__ counts)
{
    __shared__ long long red[kSegFinishThreads];
    __shared__ double lred[256 + 16];
    const int t = threadIdx.x, nc = seg_counters(C);
    const size_t rb = seg_record_bytes(C);
    const int S = kSegFinishThreads / nc;                // >= 2 (nc <= 386)
    const int s = t / nc, j = t - s * nc;
    long long a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    if (s < S) {
        const char *p = partials + 8 + 4 * (size_t)j;
        int i = s;
        for (; i + 3 * S < nrec; i += 4 * S) {
            a0 += *reinterpret_cast<const int *>(p + (size_t)i * rb);
            a1 += *reinterpret_cast<const int *>(p + (size_t)(i + S) * rb);
            a2 += *reinterpret_cast<const int *>(p + (size_t)(i + 2 * S) * rb);
            a3 += *reinterpret_cast<const int *>(p + (size_t)(i + 3 * S) * rb);
        }
        for (; i < nrec; i += S) a0 += *reinterpret_cast<const int *>(p + (size_t)i * rb);
    }
    red[t] = (a0 + a1) + (a2 + a3);
    if (t < 256) {
        const int per = (nrec + 255) / 256;
        const int lo = t * per, hi = lo + per < nrec ? lo + per : nrec;
        double v = 0.0;
        for (int i = lo; i < hi; ++i) v += *reinterpret_cast<const double *>(partials + (size_t)i * rb);
        lred[t] = v;
    }
    __syncthreads();
    if (t < nc) {
        long long v = 0;
        for (int k = 0; k < S; ++k) v += red[k * nc + t];
        counts[t] = v;
    }
    if (t < 16) {
        double v = lred[16 * t];
#pragma unroll
        for (int k = 1; k < 16; ++k) v += lred[16 * t + k];
        lred[256 + t] = v;
    }
    __syncthreads();
    if (t == 0) {
        double v = lred[256];
#pragma unroll
        for (int k = 1; k < 16; ++k) v += lred[256 + k];
        *loss_sum = v;
    }
}

}  // namespace conv3p
