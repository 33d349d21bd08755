// conv3p_seg_head_weighted.hpp -- the segmentation loss head with the arguments of the call it replaces:
//
//   tf.losses.softmax_cross_entropy(onehot_labels, logits, weights, label_smoothing, reduction)
//                                                                          (pointcnn_scene_seg_acsd.py:66-67)
//
// conv3p_seg_head.hpp is that call with weights = 1, label_smoothing = 0 and the mean over all points.  Here:
//
//   seg_weight_total_kernel + _finish   labels, weights -> {sum of the row weights, rows with a non-zero weight}
//   seg_head_weighted_kernel            seg_head_kernel with a row weight, a smoothed target and a device denominator
//                                       (its records go through seg_head_finish_kernel, unchanged)
//   seg_confusion_kernel + _finish      labels, pred -> conf[label][pred], int64
//
// Row weight.  w_r = [label in [0, C)] * class_weight[label] * point_weight[r], formed in T; a NULL table is 1.  The
// pre-pass and the head form the same product, so they agree on which rows have w_r != 0.  Weights are not validated:
// a negative, infinite or NaN weight propagates to the total, the loss and that row's gradient (NaN != 0: such a row
// counts as non-zero, as tf.not_equal does).
//
// Weighted head, per valid row with x = act[r], m = max_c x_c, s = sum_c exp(x_c - m), ls = label_smoothing:
//   target    q_c    = (1 - ls) [c == label] + ls / C                       (TensorFlow's rule: the row weight times
//                                                                            the smoothed cross-entropy)
//   loss_r           = w_r (log s + m - (1 - ls) x_label - (ls / C) sum_c x_c)
//                    = w_r (log s + (1 - ls) (m - x_label) + (ls / C) sum_c (m - x_c))      <- the form evaluated: every
//                                                                            term is >= 0, nothing cancels
//   grad_act[r][c]   = (exp(x_c - m) / s - q_c) * (w_r * scale),   scale = grad_scale, or grad_scale / *denominator
//                      (divided in double, rounded to T once), or 0 when *denominator == 0
//   *loss_sum        = sum_r loss_r, double, NOT scaled
// w_r * scale == 0 (a zero weight, a zero denominator): the gradient row is +0, bit for bit.  w_r == 0: no loss term
// either (a NaN in such a row of act reaches nothing).  Both kinds of row still count in seen / correct_class /
// predicted: those are statistics of the predictions, not of the loss.
// A label outside [0, C) is an ignored row exactly as in seg_head_kernel: loss 0, gradient row +0, `invalid` only,
// weight 0.  (TensorFlow differs for such a row under smoothing: tf.one_hot gives a zero row, which label_smoothing
// turns into the uniform target ls / C, so TensorFlow charges it ls * mean_c(-log p_c).  Here an ignored row stays
// ignored.)  The argmax rule, the NaN / inf behaviour of a weighted row and counts[2 + 3 C] are seg_head_kernel's.
// The tile image, lane = row, the LDS counters, the record layout and the fixed summation order are seg_head_kernel's
// too; with no weights, ls == 0 and no denominator the host launches seg_head_kernel itself, so that case is bit-equal
// to conv3p_seg_head_* by construction.
//
// Weight total.  Workgroup b, thread t adds the rows (b * 256 + t) + k * 256 * gridDim.x, k ascending, in double; the
// wave adds its lanes by a fixed butterfly, the workgroup its waves in wave order; the finish (one wave) adds records
// lane, lane + 64, ... ascending, then the same butterfly.  The grid is a function of `rows` alone (one workgroup per
// 1024 rows, at most kSegTotalMaxGrid = 256), so equal inputs give equal bits.
//
// Confusion matrix.  A workgroup histograms its rows into C * C int32 counters in LDS (integer atomics: order does not
// matter) and stores them as one partial; the finish sums the partials into int64.  The grid is capped at
// kSegConfMaxGrid = 64 workgroups (each takes 1024-row chunks g, g + gridDim.x, ...), so the partials are at most
// 64 * 4 C^2 bytes: 43 KB at 13 classes, 4 MB at 128.  Only rows whose label AND prediction are in [0, C) are counted
// (predictions of the head always are).
#pragma once

#include "conv3p_seg_head.hpp"

namespace conv3p {

constexpr int kSegTotalMaxGrid = 256;
constexpr int kSegTotalThreads = 256;
constexpr int kSegTotalRowsPerWg = 1024;
constexpr int kSegConfMaxGrid = 64;
constexpr int kSegConfThreads = 256;
constexpr int kSegConfRowsPerWg = 1024;

struct SegTotalRecord { double sum; long long nonzero; };

template <typename T>
__device__ inline T seg_row_weight(int lab, int C, size_t r, const T *__restrict__ class_weight,
                                   const T *__restrict__ point_weight)
{
    if ((unsigned)lab >= (unsigned)C) return T(0);
    T w = class_weight ? class_weight[lab] : T(1);
    if (point_weight) w = w * point_weight[r];
    return w;
}

__device__ inline double seg_wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ inline long long seg_wave_sum(long long v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

template <typename T>
__global__ __launch_bounds__(kSegTotalThreads) void seg_weight_total_kernel(const int32_t *__restrict__ labels, size_t R,
                                                                            int C, const T *__restrict__ class_weight,
                                                                            const T *__restrict__ point_weight,
                                                                            SegTotalRecord *__restrict__ partials)
{
    __shared__ double wsum[kSegTotalThreads / 64];
    __shared__ long long wcnt[kSegTotalThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double sum = 0.0;
    long long cnt = 0;
    const size_t step = (size_t)gridDim.x * kSegTotalThreads;
    for (size_t r = (size_t)blockIdx.x * kSegTotalThreads + threadIdx.x; r < R; r += step) {
        const T w = seg_row_weight<T>(labels[r], C, r, class_weight, point_weight);
        sum += (double)w;
        cnt += w != T(0) ? 1 : 0;
    }
    sum = seg_wave_sum(sum);
    cnt = seg_wave_sum(cnt);
    if (lane == 0) { wsum[wave] = sum; wcnt[wave] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = wsum[0];
        long long n = wcnt[0];
        for (int w = 1; w < kSegTotalThreads / 64; ++w) { s += wsum[w]; n += wcnt[w]; }
        partials[blockIdx.x].sum = s;
        partials[blockIdx.x].nonzero = n;
    }
}

// total[0] = sum of the row weights, total[1] = rows with a non-zero weight (exact below 2^53).  One wave.
__global__ __launch_bounds__(64) void seg_weight_total_finish_kernel(const SegTotalRecord *__restrict__ partials, int nrec,
                                                                     double *__restrict__ total)
{
    double sum = 0.0;
    long long cnt = 0;
    for (int i = threadIdx.x; i < nrec; i += 64) { sum += partials[i].sum; cnt += partials[i].nonzero; }
    sum = seg_wave_sum(sum);
    cnt = seg_wave_sum(cnt);
    if (threadIdx.x == 0) { total[0] = sum; total[1] = (double)cnt; }
}

// kSmooth: ls != 0 (the host chooses; without it the row loss is seg_head_kernel's expression and no sum of the
// activations is formed, so a -inf in a row stays harmless).
template <typename T, bool kSmooth>
__global__ __launch_bounds__(256) void seg_head_weighted_kernel(const T *__restrict__ act, const int32_t *__restrict__ labels,
                                                                size_t R, int C, const T *__restrict__ class_weight,
                                                                const T *__restrict__ point_weight, T smoothing,
                                                                T grad_scale, const double *__restrict__ denominator,
                                                                T *__restrict__ grad_act, int32_t *__restrict__ pred,
                                                                char *__restrict__ partials)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (int)blockDim.x >> 6;
    const int ld = seg_ld(C), nc = seg_counters(C);
    double *wloss = reinterpret_cast<double *>(smem);                               // [nw]
    T *xs = reinterpret_cast<T *>(smem + 64) + (size_t)wave * 64 * ld;              // this wave's [64][ld]
    int *cnt = reinterpret_cast<int *>(smem + 64 + (size_t)nw * 64 * ld * sizeof(T));   // [nc]
    for (int j = threadIdx.x; j < nc; j += (int)blockDim.x) cnt[j] = 0;
    __syncthreads();

    T scale = grad_scale;
    if (denominator) {
        const double d = *denominator;
        scale = d != 0.0 ? (T)((double)grad_scale / d) : T(0);
    }
    const T on = T(1) - smoothing, off = smoothing / (T)C;                          // q = on [c == label] + off

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
        __builtin_amdgcn_wave_barrier();
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
            const T w = seg_row_weight<T>(lab, C, r0 + lane, class_weight, point_weight);
            const T ws = w * scale;
            const bool want_grad = grad_act && valid && ws != T(0);                 // (a NaN weight is != 0: it propagates)
            if (valid) {
                if (w != T(0)) {
                    const T xl = x[lab];
                    T s = 0, away = 0;                                              // away = sum_c (m - x_c)
                    for (int c = 0; c < C; ++c) {                                   // (written back with or without a
                        const T d = x[c] - m;                                       //  gradient: one loop, and an image
                        const T e = seg_exp(d);                                     //  nobody reads is zeroed or dropped)
                        if (kSmooth) away -= d;
                        x[c] = e;
                        s += e;
                    }
                    if (want_grad) {
                        const T inv = T(1) / s;
                        for (int c = 0; c < C; ++c) x[c] = (x[c] * inv - ((c == lab ? on : T(0)) + off)) * ws;
                    }
                    const T row_loss = kSmooth ? seg_log(s) + (on * (m - xl) + off * away) : seg_log(s) + m - xl;
                    lsum += (double)w * (double)row_loss;
                }
                atomicAdd(&cnt[2 + lab], 1);
                atomicAdd(&cnt[2 + 2 * C + arg], 1);
                if (arg == lab) {
                    atomicAdd(&cnt[2 + C + lab], 1);
                    ++ncorrect;
                }
            } else {
                ++ninvalid;
            }
            if (grad_act && !want_grad)
                for (int c = 0; c < C; ++c) x[c] = T(0);
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

    // the records of seg_head_kernel: fixed butterfly over the lanes, then the waves in wave order
    lsum = seg_wave_sum(lsum);
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

// partial g: int32[C * C], index label * C + pred
__global__ __launch_bounds__(kSegConfThreads) void seg_confusion_kernel(const int32_t *__restrict__ labels,
                                                                        const int32_t *__restrict__ pred, size_t R, int C,
                                                                        int *__restrict__ partials)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int *hist = reinterpret_cast<int *>(smem);
    const int cells = C * C;
    for (int j = threadIdx.x; j < cells; j += kSegConfThreads) hist[j] = 0;
    __syncthreads();
    const size_t chunks = (R + kSegConfRowsPerWg - 1) / kSegConfRowsPerWg;
    for (size_t chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        const size_t base = chunk * kSegConfRowsPerWg;
#pragma unroll
        for (int k = 0; k < kSegConfRowsPerWg / kSegConfThreads; ++k) {
            const size_t r = base + (size_t)k * kSegConfThreads + threadIdx.x;
            if (r < R) {
                const int lab = labels[r], p = pred[r];
                if ((unsigned)lab < (unsigned)C && (unsigned)p < (unsigned)C) atomicAdd(&hist[lab * C + p], 1);
            }
        }
    }
    __syncthreads();
    int *out = partials + (size_t)blockIdx.x * cells;
    for (int j = threadIdx.x; j < cells; j += kSegConfThreads) out[j] = hist[j];
}

__global__ __launch_bounds__(256) void seg_confusion_finish_kernel(const int *__restrict__ partials, int nrec, int cells,
                                                                   long long *__restrict__ conf)
{
    const int j = (int)(blockIdx.x * 256 + threadIdx.x);
    if (j >= cells) return;
    long long v = 0;
    for (int g = 0; g < nrec; ++g) v += partials[(size_t)g * cells + j];
    conf[j] = v;
}

}  // namespace conv3p
