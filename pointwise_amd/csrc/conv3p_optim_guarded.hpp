// conv3p_optim_guarded.hpp -- the optimizer step that looks at the gradients before it applies them: the global norm
// of tf.clip_by_global_norm, the use_nesterov argument of tf.train.MomentumOptimizer, and a step that leaves every
// parameter alone when a gradient holds a NaN or an Inf.  Norm, scale and the decision to skip are found and used on
// the device; the host never waits for them.
//
//   grad_sumsq_kernel<T>                    up to kOptMaxTensors gradients per launch with momentum_step_kernel's
//                                           addressing (the table by value, chunks of kOptChunk elements, workgroup g
//                                           takes the chunks g, g + grid, ...): one record {sum of squares of the finite
//                                           elements, number of the others} per workgroup
//   grad_sumsq_finish_kernel                the records -> stats[0] = sum g^2, stats[1] = non-finite elements (doubles)
//   momentum_step_guarded_kernel<T, NEST>   momentum_step_kernel with three wave-uniform additions: return before the
//                                           first load when stats[1] > 0, g' = g * scale, Nesterov's rule
//
// Every sum is formed in double in a fixed order (no memset, no atomic): equal inputs give equal bits.  The longest
// chain of dependent additions behind stats[0] is (chunks per workgroup) * 4 additions per lane and accumulator (fp64:
// 8), 3 to join a lane's accumulators, 6 butterfly steps, 3 over the waves, and at most 8 + 15 + 15 in the finish: about
// 70 for the 40 M elements of the classification model.
#pragma once

#include "conv3p_optim.hpp"

namespace conv3p {

constexpr int kGradFinishThreads = 256;

struct GradNormRecord { double sumsq; int nonfinite; int pad; };

template <typename T> struct GradTable {
    const T *grad[kOptMaxTensors];
    size_t numel[kOptMaxTensors];
    size_t chunk_end[kOptMaxTensors];  // as OptTable
    size_t chunks;
};

__device__ __forceinline__ bool opt_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ bool opt_finite(double v)
{
    return ((unsigned long long)__double_as_longlong(v) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

// s += double(g)^2 for a finite g (an fp32 square is exact in double); anything else adds 0 and is counted
template <typename T> __device__ __forceinline__ void sumsq_add(double &s, int &bad, T g)
{
    const bool ok = opt_finite(g);
    const double d = ok ? (double)g : 0.0;
    s = __dadd_rn(s, __dmul_rn(d, d));
    bad += ok ? 0 : 1;
}

__device__ __forceinline__ double grad_wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = __dadd_rn(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ int grad_wave_sum(int v)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// A lane keeps one accumulator per component of its 16-byte vectors (head and tail elements go to the first), joined
// pairwise at the end; then a butterfly over the wave and the waves' sums in ascending order.
template <typename T>
__global__ __launch_bounds__(kOptThreads) void grad_sumsq_kernel(const GradTable<T> tab, GradNormRecord *__restrict__ partials)
{
    using V = typename OptVec<T>::type;
    constexpr int kVec = 16 / (int)sizeof(T);
    constexpr int kPer = kOptChunk / kVec / kOptThreads;
    constexpr int kWaves = kOptThreads / 64;
    __shared__ double wsum[kWaves];
    __shared__ int wbad[kWaves];
    const int tid = threadIdx.x;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    int bad = 0;
    for (size_t c = blockIdx.x; c < tab.chunks; c += gridDim.x) {
        int t = 0;
#pragma unroll
        for (int i = 0; i < kOptMaxTensors - 1; ++i) t += c >= tab.chunk_end[i] ? 1 : 0;
        const size_t first = t > 0 ? tab.chunk_end[t - 1] : 0;
        const size_t e0 = (c - first) * (size_t)kOptChunk;
        const size_t left = tab.numel[t] - e0;
        const int len = left < (size_t)kOptChunk ? (int)left : kOptChunk;
        const T *g = tab.grad[t] + e0;
        int head = (int)(((16 - (reinterpret_cast<size_t>(g) & 15)) & 15) / sizeof(T));
        if (head > len) head = len;
        const int nvec = (len - head) / kVec;
        const int tail0 = head + nvec * kVec;
        V gv[kPer];
#pragma unroll
        for (int u = 0; u < kPer; ++u) {
            const int v = tid + u * kOptThreads;
            if (v < nvec) gv[u] = *reinterpret_cast<const V *>(g + head + (size_t)v * kVec);
        }
#pragma unroll
        for (int u = 0; u < kPer; ++u) {
            const int v = tid + u * kOptThreads;
            if (v < nvec) {
                sumsq_add(s0, bad, gv[u].x);
                sumsq_add(s1, bad, gv[u].y);
                if constexpr (kVec == 4) {
                    sumsq_add(s2, bad, gv[u].z);
                    sumsq_add(s3, bad, gv[u].w);
                }
            }
        }
        for (int e = tid; e < head + (len - tail0); e += kOptThreads) sumsq_add(s0, bad, g[e < head ? e : tail0 + (e - head)]);
    }
    double s = grad_wave_sum(__dadd_rn(__dadd_rn(s0, s1), __dadd_rn(s2, s3)));
    bad = grad_wave_sum(bad);
    if ((tid & 63) == 0) { wsum[tid >> 6] = s; wbad[tid >> 6] = bad; }
    __syncthreads();
    if (tid == 0) {
        s = wsum[0];
        bad = wbad[0];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) { s = __dadd_rn(s, wsum[w]); bad += wbad[w]; }
        partials[blockIdx.x].sumsq = s;
        partials[blockIdx.x].nonfinite = bad;
    }
}

// One workgroup.  Thread t adds a run of ceil(nrec / 256) consecutive records in ascending order, 16 threads add 16
// consecutive run sums each, thread 0 the 16 results: ascending throughout, one fixed association for a given number of
// records (seg_head_finish_kernel's scheme).  The counts are integers: any order is exact.  accumulate != 0 adds to
// what stats holds.  A sum that is not finite (fp64 squares can overflow) is counted as one more non-finite element,
// so that stats[1] > 0 whenever stats[0] cannot be used.  nrec == 0 is legal (stats = 0, or left as they are).
__global__ __launch_bounds__(kGradFinishThreads) void grad_sumsq_finish_kernel(const GradNormRecord *__restrict__ partials,
                                                                               int nrec, int accumulate,
                                                                               double *__restrict__ stats)
{
    __shared__ double red[kGradFinishThreads + 16];
    __shared__ long long cred[kGradFinishThreads + 16];
    const int t = threadIdx.x;
    const int per = (nrec + kGradFinishThreads - 1) / kGradFinishThreads;
    const int lo = t * per, hi = lo + per < nrec ? lo + per : nrec;
    double v = 0.0;
    long long n = 0;
    for (int i = lo; i < hi; ++i) {
        v = __dadd_rn(v, partials[i].sumsq);
        n += partials[i].nonfinite;
    }
    red[t] = v;
    cred[t] = n;
    __syncthreads();
    if (t < 16) {
        v = red[16 * t];
        n = cred[16 * t];
#pragma unroll
        for (int k = 1; k < 16; ++k) { v = __dadd_rn(v, red[16 * t + k]); n += cred[16 * t + k]; }
        red[kGradFinishThreads + t] = v;
        cred[kGradFinishThreads + t] = n;
    }
    __syncthreads();
    if (t == 0) {
        v = red[kGradFinishThreads];
        n = cred[kGradFinishThreads];
#pragma unroll
        for (int k = 1; k < 16; ++k) { v = __dadd_rn(v, red[kGradFinishThreads + k]); n += cred[kGradFinishThreads + k]; }
        double bad = (double)n;
        if (accumulate) {
            v = __dadd_rn(stats[0], v);
            bad = __dadd_rn(stats[1], bad);
        }
        if (!opt_finite(v)) bad = __dadd_rn(bad, 1.0);
        stats[0] = v;
        stats[1] = bad;
    }
}

// scale = (T)(clip_norm / max(sqrt(sumsq), clip_norm)): sqrt and division correctly rounded in double, one rounding to
// T.  Exactly 1 when the norm is at most clip_norm; 0 when sumsq is not finite.
template <typename T> __device__ __forceinline__ T clip_scale(double sumsq, T clip_norm)
{
    if (!opt_finite(sumsq)) return T(0);
    const double c = (double)clip_norm, norm = __dsqrt_rn(sumsq);
    return (T)__ddiv_rn(c, norm > c ? norm : c);
}

// One element: g' = g * scale (one rounded multiply; scale == 1 leaves every g as it is), then
//   NESTEROV == false   accum = accum * m + g';  param = param - accum * lr                       (momentum_apply)
//   NESTEROV == true    accum = accum * m + g';  param = param - (g' * lr + (accum * m) * lr)     (TensorFlow's
//                       ApplyMomentum with use_nesterov: training_ops.cc, every product and sum rounded on its own)
template <typename T, bool NESTEROV>
__device__ __forceinline__ void momentum_apply_guarded(T &a, T &w, T g, T lr, T momentum, T scale)
{
    g = opt_mul(g, scale);
    if constexpr (NESTEROV) {
        a = opt_add(opt_mul(a, momentum), g);
        w = opt_sub(w, opt_add(opt_mul(g, lr), opt_mul(opt_mul(a, momentum), lr)));
    } else {
        momentum_apply(a, w, g, lr, momentum);
    }
}

// momentum_step_kernel (conv3p_optim.hpp: the same table, chunks, alignment paths and loads) with
//   skip   stats && skip_nonfinite && stats[1] > 0: every workgroup returns before its first load
//   clip   clip_norm > 0: scale from stats[0] (clip_scale), otherwise 1
// Both are uniform over the launch.  The host launches momentum_step_kernel itself when nothing of this is asked for.
template <typename T, bool NESTEROV>
__global__ __launch_bounds__(kOptThreads) void momentum_step_guarded_kernel(const OptTable<T> tab, T lr, T momentum,
                                                                            const double *__restrict__ stats, T clip_norm,
                                                                            int skip_nonfinite)
{
    using V = typename OptVec<T>::type;
    constexpr int kVec = 16 / (int)sizeof(T);
    constexpr int kPer = kOptChunk / kVec / kOptThreads;
    T scale = T(1);
    if (stats) {
        if (skip_nonfinite && stats[1] > 0.0) return;
        if (clip_norm > T(0)) scale = clip_scale<T>(stats[0], clip_norm);
    }
    const int tid = threadIdx.x;
    for (size_t c = blockIdx.x; c < tab.chunks; c += gridDim.x) {
        int t = 0;
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
                momentum_apply_guarded<T, NESTEROV>(av[u].x, wv[u].x, gv[u].x, lr, momentum, scale);
                momentum_apply_guarded<T, NESTEROV>(av[u].y, wv[u].y, gv[u].y, lr, momentum, scale);
                if constexpr (kVec == 4) {
                    momentum_apply_guarded<T, NESTEROV>(av[u].z, wv[u].z, gv[u].z, lr, momentum, scale);
                    momentum_apply_guarded<T, NESTEROV>(av[u].w, wv[u].w, gv[u].w, lr, momentum, scale);
                }
                *reinterpret_cast<V *>(a + head + (size_t)v * kVec) = av[u];
                *reinterpret_cast<V *>(w + head + (size_t)v * kVec) = wv[u];
            }
        }
        for (int e = tid; e < head + (len - tail0); e += kOptThreads) {
            const int i = e < head ? e : tail0 + (e - head);
            T ai = a[i], wi = w[i];
            momentum_apply_guarded<T, NESTEROV>(ai, wi, g[i], lr, momentum, scale);
            a[i] = ai;
            w[i] = wi;
        }
    }
}

}  // namespace conv3p
