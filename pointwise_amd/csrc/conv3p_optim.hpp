// conv3p_optim.hpp -- the models' optimizer step: tf.train.MomentumOptimizer (train_modelnet40_acsd.py:81,
// scene_seg/train_scene_seg_s3dis.py:83, train_scene_seg_scenenn.py:86), non-Nesterov ApplyMomentum, in place:
//
//   accum = accum * momentum + grad
//   param = param - accum * lr
//
// Each statement is two separately rounded operations (__fmul_rn / __fadd_rn and the __d forms: never a fused
// multiply-add), so that the result is bit-equal to numpy's `a * m + g` and `w - a * lr` in the element type.
//
//   momentum_step_kernel<T>     up to kOptMaxTensors tensors per launch; the tensor table travels by value in the kernel
//                               arguments (no device-side table, no memset, no atomics).  Bound by HBM: three reads and
//                               two writes of every element.
//   fc_dz_step_kernel           fc_dz_kernel whose thread, holding db[n], updates b[n] and its accumulator instead of
//                               storing db
//   fc_dw_step_kernel<STEPS>    fc_dw_kernel whose lane, holding dW[k][n], updates W[k][n] and its accumulator instead of
//                               storing dW: two reads and two writes of W's size, dW never reaches memory
#pragma once

#include "conv3p_head.hpp"

namespace conv3p {

constexpr int kOptMaxTensors = 16;     // CONV3P_OPT_MAX_TENSORS of include/conv3p.h
constexpr int kOptThreads = 256;
constexpr int kOptChunk = 4096;        // elements per chunk: 4 x 16 bytes per lane and array in fp32, 8 x 16 in fp64
constexpr int kOptMaxGrid = 2048;      // as the other streaming kernels: 8 workgroups per CU, the rest is grid-stride

__device__ __forceinline__ float opt_mul(float a, float b) { return __fmul_rn(a, b); }
__device__ __forceinline__ float opt_add(float a, float b) { return __fadd_rn(a, b); }
__device__ __forceinline__ float opt_sub(float a, float b) { return __fsub_rn(a, b); }
__device__ __forceinline__ double opt_mul(double a, double b) { return __dmul_rn(a, b); }
__device__ __forceinline__ double opt_add(double a, double b) { return __dadd_rn(a, b); }
__device__ __forceinline__ double opt_sub(double a, double b) { return __dsub_rn(a, b); }

// one element of ApplyMomentum: a and w are updated in place
template <typename T> __device__ __forceinline__ void momentum_apply(T &a, T &w, T g, T lr, T momentum)
{
    a = opt_add(opt_mul(a, momentum), g);
    w = opt_sub(w, opt_mul(a, lr));
}

template <typename T> struct OptTable {
    T *param[kOptMaxTensors];
    const T *grad[kOptMaxTensors];
    T *accum[kOptMaxTensors];
    size_t numel[kOptMaxTensors];
    size_t chunk_end[kOptMaxTensors];  // chunks of the tensors 0 .. i together (unused entries: the total)
    size_t chunks;
};

template <typename T> struct OptVec;
template <> struct OptVec<float> { using type = float4; };
template <> struct OptVec<double> { using type = double2; };

// Workgroup g takes the chunks g, g + grid, ...; a chunk is kOptChunk consecutive elements of ONE tensor (the last
// chunk of a tensor is shorter).  Where param, grad and accum sit at the same offset inside a 16-byte line the chunk
// is a head of up to 16 / sizeof(T) - 1 elements, 16-byte vectors, and a tail (kOptChunk * sizeof(T) is a multiple of
// 16, so every chunk of a tensor has the tensor's own head); otherwise every access is one element, coalesced.
// The stack's filter gradients are views into one fused buffer at offsets such as 729 elements: both forms are normal.
template <typename T>
__global__ __launch_bounds__(kOptThreads) void momentum_step_kernel(const OptTable<T> tab, T lr, T momentum)
{
    using V = typename OptVec<T>::type;
    constexpr int kVec = 16 / (int)sizeof(T);
    constexpr int kPer = kOptChunk / kVec / kOptThreads;   // vectors per lane and chunk
    const int tid = threadIdx.x;
    for (size_t c = blockIdx.x; c < tab.chunks; c += gridDim.x) {
        int t = 0;                                         // the tensor that owns chunk c (uniform over the workgroup)
#pragma unroll
        for (int i = 0; i < kOptMaxTensors - 1; ++i) t += c >= tab.chunk_end[i] ? 1 : 0;
        const size_t first = t > 0 ? tab.chunk_end[t - 1] : 0;
        const size_t e0 = (c - first) * (size_t)kOptChunk;
        const size_t left = tab.numel[t] - e0;
        const int len = left < (size_t)kOptChunk ? (int)left : kOptChunk;
        T *w = tab.param[t] + e0;
        const T *g = tab.grad[t] + e0;
        T *a = tab.accum[t] + e0;
        const size_t ow = reinterpret_cast<size_t>(w) & 15;
        int head = len, nvec = 0;
        if (ow == (reinterpret_cast<size_t>(g) & 15) && ow == (reinterpret_cast<size_t>(a) & 15)) {
            head = (int)(((16 - ow) & 15) / sizeof(T));
            if (head > len) head = len;
            nvec = (len - head) / kVec;
        }
        const int tail0 = head + nvec * kVec;
        V av[kPer], wv[kPer], gv[kPer];
#pragma unroll
        for (int u = 0; u < kPer; ++u) {
            const int v = tid + u * kOptThreads;
            if (v < nvec) {
                av[u] = *reinterpret_cast<const V *>(a + head + (size_t)v * kVec);
                gv[u] = *reinterpret_cast<const V *>(g + head + (size_t)v * kVec);
                wv[u] = *reinterpret_cast<const V *>(w + head + (size_t)v * kVec);
            }
        }
#pragma unroll
        for (int u = 0; u < kPer; ++u) {
            const int v = tid + u * kOptThreads;
            if (v < nvec) {
                momentum_apply(av[u].x, wv[u].x, gv[u].x, lr, momentum);
                momentum_apply(av[u].y, wv[u].y, gv[u].y, lr, momentum);
                if constexpr (kVec == 4) {
                    momentum_apply(av[u].z, wv[u].z, gv[u].z, lr, momentum);
                    momentum_apply(av[u].w, wv[u].w, gv[u].w, lr, momentum);
                }
                *reinterpret_cast<V *>(a + head + (size_t)v * kVec) = av[u];
                *reinterpret_cast<V *>(w + head + (size_t)v * kVec) = wv[u];
            }
        }
        // head and tail (or, without a common alignment, the whole chunk: head == len), one element per lane
        for (int e = tid; e < head + (len - tail0); e += kOptThreads) {
            const int i = e < head ? e : tail0 + (e - head);
            T ai = a[i], wi = w[i];
            momentum_apply(ai, wi, g[i], lr, momentum);
            a[i] = ai;
            w[i] = wi;
        }
    }
}

// fc_dz_kernel (conv3p_head.hpp) with the bias update in place of the db store: dz = dy * act'(y), the column sums in
// ascending row order (the same sum, bit for bit), then ApplyMomentum on b[n] / accum_b[n] when there is a bias.
__global__ __launch_bounds__(256) void fc_dz_step_kernel(const float *__restrict__ y, const float *__restrict__ dy, int M,
                                                         int N, int act, float *__restrict__ dz, float *__restrict__ b,
                                                         float *__restrict__ accum_b, float lr, float momentum)
{
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    float s = 0.0f;
    for (int m = 0; m < M; ++m) {
        const size_t i = (size_t)m * N + n;
        const float g = act ? dy[i] * selu_slope(y[i]) : dy[i];
        dz[i] = g;
        s += g;
    }
    if (b) {
        float ai = accum_b[n], bi = b[n];
        momentum_apply(ai, bi, s, lr, momentum);
        accum_b[n] = ai;
        b[n] = bi;
    }
}

// fc_dw_kernel (conv3p_head.hpp: same staging, same MFMA sequence, so the implied dW is bit-identical) with the
// update as its epilogue: the lane that holds dW[k][n] loads accum[k][n] and W[k][n] -- 128 contiguous bytes per row
// and access, all 32 loads of a column block in flight before the first use -- applies the rule and stores both.
// The host launches it AFTER fc_dx_kernel, which needs the old W.
template <int STEPS>
__global__ __launch_bounds__(512) void fc_dw_step_kernel(const float *__restrict__ x, const float *__restrict__ dz, int M,
                                                         int K, int N, float *__restrict__ W, float *__restrict__ accum,
                                                         float lr, float momentum)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int ldz = N + 1;
    float *zs = reinterpret_cast<float *>(smem);                       // [2 STEPS][N + 1], zero rows past M
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, half = lane >> 5, nw = (int)blockDim.x >> 6;
    for (int m = wave; m < 2 * STEPS; m += nw)
        for (int n = lane; n < N; n += 64) zs[m * ldz + n] = m < M ? dz[(size_t)m * N + n] : 0.0f;
    __syncthreads();
    // (wave-uniform, and said so: the epilogue's row addresses are then scalar + one lane offset, not 32 address pairs)
    const int kb = ((int)blockIdx.x * nw + __builtin_amdgcn_readfirstlane(wave)) * 32;
    const int k = min(kb + (lane & 31), K - 1);
    float a[STEPS];
#pragma unroll
    for (int s = 0; s < STEPS; ++s) {
        const int m = 2 * s + half;                                     // unconditional load, clamped to the last row;
        const float v = x[(size_t)min(m, M - 1) * K + k];               // rows past M meet dz == 0 in LDS and are zeroed
        a[s] = m < M ? v : 0.0f;                                        // here as well (0 * Inf)
    }
    float *Wb = W + (size_t)kb * N, *ab = accum + (size_t)kb * N;     // scalar bases; 16 lane offsets below 32 N serve both
    unsigned off[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) off[r] = (unsigned)(((r & 3) + 8 * (r >> 2) + 4 * half) * N + (lane & 31));
    for (int nb = 0; nb < N; nb += 32) {
        const int n = min(nb + (lane & 31), N - 1);
        const bool col_ok = nb + (lane & 31) < N;
        // the epilogue's operands first: they arrive under the LDS reads and the MFMAs
        float av[16], wv[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int kr = kb + (r & 3) + 8 * (r >> 2);
            av[r] = wv[r] = 0.0f;
            if (col_ok && kr + 4 * half < K) {
                av[r] = ab[nb + off[r]];
                wv[r] = Wb[nb + off[r]];
            }
        }
        const float *zb = zs + half * ldz + n;
        float bv[STEPS];
#pragma unroll
        for (int s = 0; s < STEPS; ++s) bv[s] = zb[2 * s * ldz];
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
#pragma unroll
        for (int s = 0; s < STEPS; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], bv[s], acc, 0, 0, 0);
        // vmcnt(0), stated ONCE: the operands were loaded under conditions, so hipcc cannot count them and would
        // otherwise drain the memory queue -- the previous row's stores included -- before each of the 16 updates
        // below and at the head of every block (fused step, model shape: 166 us against 132 us)
        __builtin_amdgcn_s_waitcnt(0x0f70);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int kr = kb + (r & 3) + 8 * (r >> 2);
            if (col_ok && kr + 4 * half < K) {
                momentum_apply(av[r], wv[r], acc[r], lr, momentum);
                ab[nb + off[r]] = av[r];
                Wb[nb + off[r]] = wv[r];
            }
        }
    }
}

}  // namespace conv3p
