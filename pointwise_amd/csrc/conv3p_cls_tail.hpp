// conv3p_cls_tail.hpp -- the tail of the classification model's training step as TWO launches.
//
//   drop   = dropout_selu(fc1, rate, training)                      (pointcnn2_acsd.py:73, selu.py:35-70)
//   logits = selu(drop . W2 + b2)                                   (pointcnn2_acsd.py:75)
//   loss   = mean sparse softmax cross-entropy(logits, labels)      (pointcnn2_acsd.py:79-90)
//   the batch statistics of train_modelnet40_acsd.py:136-146 (argmax, correct clouds, per-class seen / correct)
//   and the way back: dlogits -> dz -> dW2, db2, dfc1, with minimize()'s update of W2 / b2 when asked for.
// Composed from framework ops and the fc kernels this is about 27 launches on (32, 512) and (32, 40) tensors; the
// arithmetic is 2 M multiply-adds, so its cost is launches and host time.  Here it is
//
//   cls_tail_row_kernel   one workgroup per batch row: dropout (mask given, or drawn with Philox4x32-10), logits, argmax,
//                         row loss, dz, dfc1 (from W2 as it is BEFORE the update); drop, dz, the row's loss and
//                         prediction go to the workspace
//   cls_tail_dw_kernel    one thread per element of W2: dW2[h][c] = sum_m drop[m][h] dz[m][c], rows in ascending order,
//                         stored -- or applied with ApplyMomentum (conv3p_optim.hpp) to W2 and its accumulator in place;
//                         one more workgroup adds the rows' records to loss_sum / counts and makes db2 (or steps b2)
//
// with no memset and no atomic on global memory: bitwise reproducible.  A workgroup of the row kernel sees one row only,
// so logits, pred and dfc1 of a row do not depend on the batch it came in.  What bounds it: launch and L2 latency (W2 is
// 80 KB at the model's size, read twice by each of 32 workgroups, coalesced); there is no arithmetic to speak of.
//
// Row kernel, 1024 threads, H <= 1024, C <= 128:
//   A  thread t < H / 4 loads fc1[m][4 t .. 4 t + 3], makes keep and drop for them (ONE Philox block gives the four
//      words: e = m H + h, H % 4 == 0, so e >> 2 is the block and e & 3 = h & 3 the word) -> LDS, workspace, keep_out
//   B  z[c] = sum_h drop[h] W2[h][c]: S = min(1024 / C, 64) slices; thread (s, c) = s C + c adds the rows h = s, s + S, ...
//      (consecutive threads read consecutive addresses of W2), thread c adds the S slice sums in slice order
//   C  wave 0: max / first argmax by a scan from index 0 (np.argmax's tie rule, as seg_head_kernel), exp and sum by a
//      fixed butterfly, the row loss, dz[c] = (softmax - onehot) grad_scale selu'(logits[c])
//   D  8 lanes per h: dfc1[h] = (sum_c dz[c] W2[h][c]) a keep[h]; a wave reads 8 C consecutive floats of W2
// The sums' associations depend on (H, C) alone.
//
// Philox4x32-10 (Salmon et al., SC'11): key = (seed low, seed high), counter = (e >> 2, 0, step low, step high),
// u = (word >> 8) 2^-24, keep = floorf(keep_prob + u) (selu.py:53-55): a function of (seed, step, m, h) only.
#pragma once

#include "conv3p_optim.hpp"

namespace conv3p {

constexpr int kClsMaxRows = 128;
constexpr int kClsMaxHidden = 1024;
constexpr int kClsMaxClass = 128;
constexpr int kClsRowThreads = 1024;
constexpr int kClsDwThreads = 256;
constexpr int kClsMaxSlices = 64;

struct ClsTailArgs {
    const float *fc1, *W2, *b2;
    const int32_t *labels;
    const float *keep_mask;            // NULL: drawn
    int M, H, C;
    int dropout;                       // training with rate > 0
    int need_grad;
    float keep_prob, a, b, alpha;      // selu.py:40, :59, :61, :36
    unsigned seed_lo, seed_hi, step_lo, step_hi;
    float grad_scale;
    float *logits;
    int32_t *pred;                     // may be NULL
    float *dfc1;
    unsigned char *keep_out;           // may be NULL
    // workspace
    float *drop, *dz;
    double *row_loss;
    int32_t *row_pred;
};

struct Philox4 { unsigned w[4]; };

__host__ __device__ inline Philox4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1)
{
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        c1 = (unsigned)p1;
        c3 = (unsigned)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return Philox4{{c0, c1, c2, c3}};
}

__device__ __forceinline__ float cls_keep(unsigned word, float keep_prob)
{
    return floorf(keep_prob + (float)(word >> 8) * 0x1p-24f);
}

__device__ __forceinline__ float cls_drop(float x, float keep, const ClsTailArgs &p)
{
    return p.a * (x * keep + p.alpha * (1.0f - keep)) + p.b;           // selu.py:56, :62
}

__global__ __launch_bounds__(kClsRowThreads) void cls_tail_row_kernel(const ClsTailArgs p)
{
    __shared__ __attribute__((aligned(16))) float drop_s[kClsMaxHidden];
    __shared__ __attribute__((aligned(16))) float keep_s[kClsMaxHidden];
    __shared__ float part_s[kClsRowThreads];
    __shared__ float x_s[kClsMaxClass];
    __shared__ float dz_s[kClsMaxClass];
    __shared__ int valid_s;
    const int t = threadIdx.x, m = blockIdx.x, H = p.H, C = p.C;

    // A: the row of drop
    if (4 * t < H) {
        const size_t e = (size_t)m * H + 4 * t;
        const float4 x = *reinterpret_cast<const float4 *>(p.fc1 + e);
        float4 d = x, k = make_float4(1.f, 1.f, 1.f, 1.f);
        if (p.dropout) {
            if (p.keep_mask) {
                k = *reinterpret_cast<const float4 *>(p.keep_mask + e);
            } else {
                const Philox4 r = philox4x32_10((unsigned)(e >> 2), 0u, p.step_lo, p.step_hi, p.seed_lo, p.seed_hi);
                k = make_float4(cls_keep(r.w[0], p.keep_prob), cls_keep(r.w[1], p.keep_prob), cls_keep(r.w[2], p.keep_prob),
                                cls_keep(r.w[3], p.keep_prob));
            }
            d = make_float4(cls_drop(x.x, k.x, p), cls_drop(x.y, k.y, p), cls_drop(x.z, k.z, p), cls_drop(x.w, k.w, p));
            if (p.keep_out) {
                unsigned char *ko = p.keep_out + e;
                ko[0] = k.x != 0.0f;
                ko[1] = k.y != 0.0f;
                ko[2] = k.z != 0.0f;
                ko[3] = k.w != 0.0f;
            }
        }
        *reinterpret_cast<float4 *>(drop_s + 4 * t) = d;
        *reinterpret_cast<float4 *>(keep_s + 4 * t) = k;
        if (p.need_grad) *reinterpret_cast<float4 *>(p.drop + e) = d;
    }
    __syncthreads();

    // B: the logits
    const int S = min(kClsRowThreads / C, kClsMaxSlices);
    if (t < S * C) {
        const int s = t / C, c = t - s * C;
        const float *w = p.W2 + c;
        float acc = 0.0f;
        int h = s;
        for (; h + 7 * S < H; h += 8 * S) {
            float wv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) wv[u] = w[(size_t)(h + u * S) * C];
#pragma unroll
            for (int u = 0; u < 8; ++u) acc = fmaf(drop_s[h + u * S], wv[u], acc);
        }
        for (; h < H; h += S) acc = fmaf(drop_s[h], w[(size_t)h * C], acc);
        part_s[t] = acc;
    }
    __syncthreads();
    if (t < C) {
        float z = part_s[t];
        for (int s = 1; s < S; ++s) z += part_s[s * C + t];
        const float x = selu_value(z + p.b2[t]);
        p.logits[(size_t)m * C + t] = x;
        x_s[t] = x;
    }
    __syncthreads();

    // C: wave 0 -- prediction, loss, dz
    if (t < 64) {
        const int lab = p.labels[m];
        const bool valid = (unsigned)lab < (unsigned)C;
        float mx = x_s[0];
        int arg = 0;
        for (int c = 1; c < C; ++c) {
            const float v = x_s[c];
            if (v > mx) { mx = v; arg = c; }
        }
        const float e0 = t < C ? expf(x_s[t] - mx) : 0.0f;
        const float e1 = t + 64 < C ? expf(x_s[t + 64] - mx) : 0.0f;
        float sum = e0 + e1;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) sum += __shfl_xor(sum, off, 64);
        if (t == 0) {
            if (p.pred) p.pred[m] = arg;
            p.row_pred[m] = arg;
            p.row_loss[m] = valid ? (double)(logf(sum) + mx - x_s[lab]) : 0.0;
            valid_s = valid ? 1 : 0;
        }
        if (p.need_grad) {
            const float inv = 1.0f / sum;
            if (t < C) {
                const float g = valid ? (e0 * inv - (t == lab ? 1.0f : 0.0f)) * p.grad_scale * selu_slope(x_s[t]) : 0.0f;
                dz_s[t] = g;
                p.dz[(size_t)m * C + t] = g;
            }
            if (t + 64 < C) {
                const float g = valid ? (e1 * inv - (t + 64 == lab ? 1.0f : 0.0f)) * p.grad_scale * selu_slope(x_s[t + 64]) : 0.0f;
                dz_s[t + 64] = g;
                p.dz[(size_t)m * C + t + 64] = g;
            }
        }
    }
    if (!p.need_grad) return;
    __syncthreads();

    // D: dfc1
    const bool valid = valid_s != 0;
    const int g = t & 7;
    for (int h = t >> 3; h < H; h += kClsRowThreads / 8) {
        const float *w = p.W2 + (size_t)h * C;
        float acc = 0.0f;
        for (int c = g; c < C; c += 8) acc = fmaf(dz_s[c], w[c], acc);
        acc += __shfl_xor(acc, 4, 64);
        acc += __shfl_xor(acc, 2, 64);
        acc += __shfl_xor(acc, 1, 64);
        if (g == 0) {
            const float f = p.dropout ? p.a * keep_s[h] : 1.0f;
            p.dfc1[(size_t)m * H + h] = valid ? acc * f : 0.0f;           // an ignored row is +0 whatever W2 holds
        }
    }
}

// Workgroups 0 .. gridDim.x - 2: one thread per element of W2 (need_grad only); the last workgroup: the statistics, the
// loss and the bias.  W2 / b2 are written only here, after every workgroup of the row kernel has read them.
__global__ __launch_bounds__(kClsDwThreads) void cls_tail_dw_kernel(const float *__restrict__ drop, const float *__restrict__ dz,
                                                                    const double *__restrict__ row_loss,
                                                                    const int32_t *__restrict__ row_pred,
                                                                    const int32_t *__restrict__ labels, int M, int H, int C,
                                                                    int need_grad, float *W2, float *b2, float *accum_W2,
                                                                    float *accum_b2, float lr, float momentum, float *dW2,
                                                                    float *db2, double *__restrict__ loss_sum,
                                                                    long long *__restrict__ counts)
{
    const int t = threadIdx.x;
    if (blockIdx.x + 1 < gridDim.x) {
        const int e = blockIdx.x * kClsDwThreads + t;
        if (e >= H * C) return;
        const int h = e / C, c = e - h * C;
        const float *dp = drop + h, *zp = dz + c;
        float acc = 0.0f;
        int m = 0;
        for (; m + 8 <= M; m += 8) {
            float dv[8], zv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                dv[u] = dp[(size_t)(m + u) * H];
                zv[u] = zp[(size_t)(m + u) * C];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) acc = fmaf(dv[u], zv[u], acc);
        }
        for (; m < M; ++m) acc = fmaf(dp[(size_t)m * H], zp[(size_t)m * C], acc);
        if (accum_W2) {
            float ai = accum_W2[e], wi = W2[e];
            momentum_apply(ai, wi, acc, lr, momentum);
            accum_W2[e] = ai;
            W2[e] = wi;
        } else {
            dW2[e] = acc;
        }
        return;
    }

    __shared__ int cnt[2 + 3 * kClsMaxClass];
    const int nc = 2 + 3 * C;
    for (int j = t; j < nc; j += kClsDwThreads) cnt[j] = 0;
    __syncthreads();
    if (t < M) {
        const int lab = labels[t], arg = row_pred[t];
        if ((unsigned)lab < (unsigned)C) {
            atomicAdd(&cnt[2 + lab], 1);
            atomicAdd(&cnt[2 + 2 * C + arg], 1);
            if (arg == lab) {
                atomicAdd(&cnt[2 + C + lab], 1);
                atomicAdd(&cnt[0], 1);
            }
        } else {
            atomicAdd(&cnt[1], 1);
        }
    }
    if (t == kClsDwThreads - 1) {                      // (a lane of the last wave: the counters and db2 sit in the first)
        double v = 0.0;
        for (int m = 0; m < M; ++m) v += row_loss[m];
        *loss_sum = v;
    }
    if (need_grad && t < C) {
        float s = 0.0f;
        for (int m = 0; m < M; ++m) s += dz[(size_t)m * C + t];
        if (accum_b2) {
            float ai = accum_b2[t], bi = b2[t];
            momentum_apply(ai, bi, s, lr, momentum);
            accum_b2[t] = ai;
            b2[t] = bi;
        } else {
            db2[t] = s;
        }
    }
    __syncthreads();
    for (int j = t; j < nc; j += kClsDwThreads) counts[j] = cnt[j];
}

}  // namespace conv3p
