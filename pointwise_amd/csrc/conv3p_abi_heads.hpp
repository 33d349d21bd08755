// conv3p_abi_heads.hpp -- host side of the heads and the optimizer: FC, segmentation head (plain, weighted, confusion),
// momentum step (plain, guarded), classification tail.  Included by conv3p_abi.hip.
namespace {

// ----------------------------------------------------------------------------- the segmentation head
// Waves per workgroup and grid of one segmentation-head call.  A (T, C) is supported when four wave tiles and the
// counters fit in the CU's LDS (one wave per SIMD at least: fp32 up to 128 classes, fp64 up to 79); the workgroup is
// four waves while that leaves three or more workgroups per CU (13 classes: 13.5 KB, 41: 42.5 KB), then two, then one.
struct SegPlan { int nw; unsigned grid; size_t lds; };
template <typename T> bool seg_plan(size_t rows, int C, SegPlan &p)
{
    if (C > kSegMaxClass || seg_lds_bytes<T>(4, C) > kMaxLds) return false;
    p.nw = seg_lds_bytes<T>(4, C) <= 48 * 1024 ? 4 : seg_lds_bytes<T>(2, C) <= 48 * 1024 ? 2 : 1;
    p.lds = seg_lds_bytes<T>(p.nw, C);
    const size_t tiles = (rows + 63) / 64, wgs = (tiles + p.nw - 1) / p.nw;
    p.grid = capped_grid(wgs, kSegMaxGrid);
    return true;
}
// The head's workspace: one partial record per workgroup.
inline size_t carve_seg(void *ws, unsigned grid, int C, char *&part) { return carve_one(ws, (size_t)grid * seg_record_bytes(C), part); }
// What conv3p_seg_head_workspace_bytes declares: one-wave workgroups, the most records either element type takes.  A call
// checks its buffer against the size its export declares, not against what this call's plan happens to use, so that a
// caller who allocates less learns it at the first call and not when another shape changes the plan.
inline size_t seg_declared_bytes(size_t rows, int C)
{
    char *part;
    return carve_seg(nullptr, capped_grid((rows + 63) / 64, kSegMaxGrid), C, part);
}

template <typename T>
int seg_head_impl(const T *act, const int32_t *labels, size_t rows, int C, T grad_scale, T *grad_act, int32_t *pred,
                  double *loss_sum, int64_t *counts, void *workspace, size_t workspace_bytes, void *stream,
                  size_t declared = 0)
{
    if (rows == 0 || C < 2 || !act || !labels || !loss_sum || !counts) return CONV3P_ERR_INVALID_ARGUMENT;
    SegPlan p;
    if (rows > ((size_t)1 << 40) || !seg_plan<T>(rows, C, p)) return CONV3P_ERR_UNSUPPORTED;   // (int32 partial counters)
    char *part;
    // declared: bytes the entry point's own export declares (the weighted head's covers this one's)
    TRY(buf_check(workspace, workspace_bytes, std::max({carve_seg(workspace, p.grid, C, part), seg_declared_bytes(rows, C), declared})));
    hipStream_t s = static_cast<hipStream_t>(stream);
    {
        Scope sc(K_SEG_HEAD, s);
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(seg_head_kernel<T>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds);
        hipLaunchKernelGGL(seg_head_kernel<T>, dim3(p.grid), dim3(64 * p.nw), p.lds, s, act, labels, rows, C, grad_scale,
                           grad_act, pred, part);
        hipLaunchKernelGGL(seg_head_finish_kernel, dim3(1), dim3(kSegFinishThreads), 0, s, part, (int)p.grid, C, loss_sum,
                           reinterpret_cast<long long *>(counts));
    }
    return hip_ok();
}

// ----------------------------------------------------------------------------- the weighted segmentation head
// (conv3p_seg_head_weighted.hpp).  All launches are accounted under K_SEG_HEAD.
inline unsigned seg_total_grid(size_t rows)
{
    const size_t wgs = (rows + kSegTotalRowsPerWg - 1) / kSegTotalRowsPerWg;
    return capped_grid(wgs, kSegTotalMaxGrid);
}
inline unsigned seg_conf_grid(size_t rows)
{
    const size_t wgs = (rows + kSegConfRowsPerWg - 1) / kSegConfRowsPerWg;
    return capped_grid(wgs, kSegConfMaxGrid);
}
inline size_t seg_total_bytes(size_t rows) { return up((size_t)seg_total_grid(rows) * sizeof(SegTotalRecord)); }
// What conv3p_seg_head_weighted_workspace_bytes declares: one buffer serves the total and the head.
inline size_t seg_weighted_declared_bytes(size_t rows, int C) { return std::max(seg_declared_bytes(rows, C), seg_total_bytes(rows)); }

template <typename T>
int seg_weight_total_impl(const int32_t *labels, size_t rows, int C, const T *class_weight, const T *point_weight,
                          double *total, void *workspace, size_t workspace_bytes, void *stream)
{
    if (rows == 0 || C < 2 || !labels || !total) return CONV3P_ERR_INVALID_ARGUMENT;
    SegPlan p;
    if (rows > ((size_t)1 << 40) || !seg_plan<T>(rows, C, p)) return CONV3P_ERR_UNSUPPORTED;
    TRY(buf_check(workspace, workspace_bytes, seg_weighted_declared_bytes(rows, C)));
    hipStream_t s = static_cast<hipStream_t>(stream);
    SegTotalRecord *part = static_cast<SegTotalRecord *>(workspace);
    const unsigned grid = seg_total_grid(rows);
    {
        Scope sc(K_SEG_HEAD, s);
        hipLaunchKernelGGL(seg_weight_total_kernel<T>, dim3(grid), dim3(kSegTotalThreads), 0, s, labels, rows, C,
                           class_weight, point_weight, part);
        hipLaunchKernelGGL(seg_weight_total_finish_kernel, dim3(1), dim3(64), 0, s, part, (int)grid, total);
    }
    return hip_ok();
}

template <typename T>
int seg_head_weighted_impl(const T *act, const int32_t *labels, size_t rows, int C, const T *class_weight,
                           const T *point_weight, double smoothing, T grad_scale, const double *denominator, T *grad_act,
                           int32_t *pred, double *loss_sum, int64_t *counts, void *workspace, size_t workspace_bytes,
                           void *stream)
{
    if (rows == 0 || C < 2 || !act || !labels || !loss_sum || !counts) return CONV3P_ERR_INVALID_ARGUMENT;
    if (!(smoothing >= 0.0 && smoothing < 1.0)) return CONV3P_ERR_INVALID_ARGUMENT;   // also rejects NaN
    const T ls = (T)smoothing;                                                         // what the kernel smooths with
    if (!class_weight && !point_weight && ls == T(0) && !denominator)                  // the plain head, bit for bit
        return seg_head_impl<T>(act, labels, rows, C, grad_scale, grad_act, pred, loss_sum, counts, workspace,
                                workspace_bytes, stream, seg_weighted_declared_bytes(rows, C));
    SegPlan p;
    if (rows > ((size_t)1 << 40) || !seg_plan<T>(rows, C, p)) return CONV3P_ERR_UNSUPPORTED;
    char *part;
    TRY(buf_check(workspace, workspace_bytes, std::max(carve_seg(workspace, p.grid, C, part), seg_weighted_declared_bytes(rows, C))));
    hipStream_t s = static_cast<hipStream_t>(stream);
    {
        Scope sc(K_SEG_HEAD, s);
        auto kern = ls != T(0) ? seg_head_weighted_kernel<T, true> : seg_head_weighted_kernel<T, false>;
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds);
        hipLaunchKernelGGL(kern, dim3(p.grid), dim3(64 * p.nw), p.lds, s, act, labels, rows, C, class_weight,
                           point_weight, ls, grad_scale, denominator, grad_act, pred, part);
        hipLaunchKernelGGL(seg_head_finish_kernel, dim3(1), dim3(kSegFinishThreads), 0, s, part, (int)p.grid, C, loss_sum,
                           reinterpret_cast<long long *>(counts));
    }
    return hip_ok();
}

static_assert(kOptMaxTensors == CONV3P_OPT_MAX_TENSORS, "conv3p_optim.hpp and conv3p.h disagree");

// The table of a launch from the host arrays: CONV3P_ERR_INVALID_ARGUMENT for a NULL or misaligned entry with a non-zero
// count; tab.chunks == 0 when there is nothing to do.
template <typename T>
int opt_table(int n, T *const *params, const T *const *grads, T *const *accums, const size_t *numels, OptTable<T> &tab)
{
    size_t chunks = 0;
    for (int i = 0; i < kOptMaxTensors; ++i) {
        const size_t ne = i < n ? numels[i] : 0;
        if (ne != 0) {
            if (!params[i] || !grads[i] || !accums[i]) return CONV3P_ERR_INVALID_ARGUMENT;
            if (((reinterpret_cast<size_t>(params[i]) | reinterpret_cast<size_t>(grads[i]) |
                  reinterpret_cast<size_t>(accums[i])) & (sizeof(T) - 1)) != 0)
                return CONV3P_ERR_INVALID_ARGUMENT;
        }
        tab.param[i] = ne ? params[i] : nullptr;
        tab.grad[i] = ne ? grads[i] : nullptr;
        tab.accum[i] = ne ? accums[i] : nullptr;
        tab.numel[i] = ne;
        chunks += (ne + kOptChunk - 1) / kOptChunk;
        tab.chunk_end[i] = chunks;
    }
    tab.chunks = chunks;
    return CONV3P_OK;
}
inline unsigned opt_grid(size_t chunks) { return capped_grid(chunks, kOptMaxGrid); }

// status first, then (only if there is anything to do) the table by value and one launch
template <typename T>
int momentum_step_impl(int n, T *const *params, const T *const *grads, T *const *accums, const size_t *numels, T lr,
                       T momentum, void *stream)
{
    if (n < 0 || n > kOptMaxTensors) return CONV3P_ERR_INVALID_ARGUMENT;
    if (n == 0) return CONV3P_OK;
    if (!params || !grads || !accums || !numels) return CONV3P_ERR_INVALID_ARGUMENT;
    OptTable<T> tab;
    TRY(opt_table<T>(n, params, grads, accums, numels, tab));
    if (tab.chunks == 0) return CONV3P_OK;
    hipLaunchKernelGGL(momentum_step_kernel<T>, dim3(opt_grid(tab.chunks)), dim3(kOptThreads), 0,
                       static_cast<hipStream_t>(stream), tab, lr, momentum);
    return hip_ok();
}

// The guarded step.  Without Nesterov and without a use for stats this IS momentum_step_impl: the same instantiation
// of momentum_step_kernel, so the defaults cost and compute what they did.
template <typename T>
int momentum_step_guarded_impl(int n, T *const *params, const T *const *grads, T *const *accums, const size_t *numels, T lr,
                               T momentum, int nesterov, T clip_norm, int skip_nonfinite, const double *stats, void *stream)
{
    if (n < 0 || n > kOptMaxTensors) return CONV3P_ERR_INVALID_ARGUMENT;
    if (!std::isfinite((double)clip_norm)) return CONV3P_ERR_INVALID_ARGUMENT;
    const bool clip = clip_norm > T(0), guarded = clip || skip_nonfinite != 0;
    if (guarded && !stats) return CONV3P_ERR_INVALID_ARGUMENT;
    if (!nesterov && !guarded) return momentum_step_impl<T>(n, params, grads, accums, numels, lr, momentum, stream);
    if (n == 0) return CONV3P_OK;
    if (!params || !grads || !accums || !numels) return CONV3P_ERR_INVALID_ARGUMENT;
    OptTable<T> tab;
    TRY(opt_table<T>(n, params, grads, accums, numels, tab));
    if (tab.chunks == 0) return CONV3P_OK;
    auto kern = nesterov ? momentum_step_guarded_kernel<T, true> : momentum_step_guarded_kernel<T, false>;
    hipLaunchKernelGGL(kern, dim3(opt_grid(tab.chunks)), dim3(kOptThreads), 0, static_cast<hipStream_t>(stream), tab, lr,
                       momentum, guarded ? stats : nullptr, clip ? clip_norm : T(0), skip_nonfinite ? 1 : 0);
    return hip_ok();
}

// grad_sumsq_kernel + grad_sumsq_finish_kernel; with nothing to read only the finish runs (stats = 0), and with
// accumulate nothing at all.  Outside the profile bracket, as momentum_step_kernel.
inline size_t grad_norm_bytes() { return up((size_t)kOptMaxGrid * sizeof(GradNormRecord)); }

template <typename T>
int grad_norm_impl(int n, const T *const *grads, const size_t *numels, double *stats, int accumulate, void *workspace,
                   size_t workspace_bytes, void *stream)
{
    if (n < 0 || n > kOptMaxTensors || !stats) return CONV3P_ERR_INVALID_ARGUMENT;
    if (n > 0 && (!grads || !numels)) return CONV3P_ERR_INVALID_ARGUMENT;
    GradTable<T> tab;
    size_t chunks = 0;
    for (int i = 0; i < kOptMaxTensors; ++i) {
        const size_t ne = i < n ? numels[i] : 0;
        if (ne != 0 && (!grads[i] || (reinterpret_cast<size_t>(grads[i]) & (sizeof(T) - 1)) != 0))
            return CONV3P_ERR_INVALID_ARGUMENT;
        tab.grad[i] = ne ? grads[i] : nullptr;
        tab.numel[i] = ne;
        chunks += (ne + kOptChunk - 1) / kOptChunk;
        tab.chunk_end[i] = chunks;
    }
    tab.chunks = chunks;
    if (chunks == 0 && accumulate) return CONV3P_OK;
    if (chunks != 0) TRY(buf_check(workspace, workspace_bytes, grad_norm_bytes()));
    hipStream_t s = static_cast<hipStream_t>(stream);
    GradNormRecord *part = static_cast<GradNormRecord *>(workspace);
    const unsigned grid = opt_grid(chunks);
    if (grid != 0) hipLaunchKernelGGL(grad_sumsq_kernel<T>, dim3(grid), dim3(kOptThreads), 0, s, tab, part);
    hipLaunchKernelGGL(grad_sumsq_finish_kernel, dim3(1), dim3(kGradFinishThreads), 0, s, part, (int)grid,
                       accumulate ? 1 : 0, stats);
    return hip_ok();
}

// ----------------------------------------------------------------------------- the classification tail
bool cls_shape_ok(int M, int H, int C)
{
    return !(M < 1 || M > kClsMaxRows || H < 8 || H % 8 != 0 || H > kClsMaxHidden || C < 2 || C > kClsMaxClass);
}
// The tail's workspace: what cls_tail_row_kernel leaves for cls_tail_dw_kernel.
size_t carve_cls(void *ws, int M, int H, int C, ClsTailArgs &a)
{
    Carver cv(ws);
    a.drop = cv.take<float>((size_t)M * H);
    a.dz = cv.take<float>((size_t)M * C);
    a.row_loss = cv.take<double>((size_t)M);
    a.row_pred = cv.take<int32_t>((size_t)M);
    return cv.bytes();
}

// Every status first; then cls_tail_row_kernel and cls_tail_dw_kernel, outside the profile bracket (the table of
// kinds is pinned), as momentum_step_kernel.  accum_W2 != NULL: the _step entry point.
int cls_tail_impl(const float *fc1, float *W2, float *b2, const int32_t *labels, int M, int H, int C, int training,
                  double rate, const float *keep_mask, uint64_t seed, uint64_t step, float grad_scale, float *logits,
                  int32_t *pred, float *dfc1, float *dW2, float *db2, float *accum_W2, float *accum_b2, float lr,
                  float momentum, uint8_t *keep_out, double *loss_sum, int64_t *counts, void *workspace,
                  size_t workspace_bytes, void *stream)
{
    if (!fc1 || !W2 || !b2 || !labels || !logits || !loss_sum || !counts || M <= 0 || H <= 0 || C < 2)
        return CONV3P_ERR_INVALID_ARGUMENT;
    if (training && !(rate >= 0.0 && rate < 1.0)) return CONV3P_ERR_INVALID_ARGUMENT;
    if (dfc1 && !accum_W2 && (!dW2 || !db2)) return CONV3P_ERR_INVALID_ARGUMENT;
    if (((reinterpret_cast<uintptr_t>(fc1) | reinterpret_cast<uintptr_t>(keep_mask)) & 15) != 0)
        return CONV3P_ERR_INVALID_ARGUMENT;
    if (!cls_shape_ok(M, H, C)) return CONV3P_ERR_UNSUPPORTED;
    ClsTailArgs a;
    TRY(buf_check(workspace, workspace_bytes, carve_cls(workspace, M, H, C, a)));
    a.fc1 = fc1; a.W2 = W2; a.b2 = b2; a.labels = labels; a.keep_mask = keep_mask;
    a.M = M; a.H = H; a.C = C;
    a.dropout = training && rate > 0.0;
    a.need_grad = dfc1 != nullptr;
    // selu.py:36-61 in double, as head.dropout_selu_constants
    const double alpha = -1.7580993408473766, keep = 1.0 - rate;
    const double ca = a.dropout ? std::sqrt(1.0 / (keep * ((1.0 - keep) * alpha * alpha + 1.0))) : 1.0;
    a.keep_prob = (float)keep;
    a.a = (float)ca;
    a.b = a.dropout ? (float)(0.0 - ca * ((1.0 - keep) * alpha)) : 0.0f;
    a.alpha = (float)alpha;
    a.seed_lo = (unsigned)seed; a.seed_hi = (unsigned)(seed >> 32);
    a.step_lo = (unsigned)step; a.step_hi = (unsigned)(step >> 32);
    a.grad_scale = grad_scale;
    a.logits = logits; a.pred = pred; a.dfc1 = dfc1; a.keep_out = keep_out;
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(cls_tail_row_kernel, dim3((unsigned)M), dim3(kClsRowThreads), 0, s, a);
    TRY(hip_ok());
    const unsigned wgs = a.need_grad ? (unsigned)((H * C + kClsDwThreads - 1) / kClsDwThreads) : 0u;
    hipLaunchKernelGGL(cls_tail_dw_kernel, dim3(wgs + 1), dim3(kClsDwThreads), 0, s, a.drop, a.dz, a.row_loss, a.row_pred,
                       labels, M, H, C, a.need_grad, W2, b2, accum_W2, accum_b2, lr, momentum, dW2, db2, loss_sum,
                       reinterpret_cast<long long *>(counts));
    return hip_ok();
}

struct FcPlan { int kc, chunks, mblocks, nblocks; };
bool fc_plan(int M, int K, int N, FcPlan &p)
{
    if (M < 1 || K < 1 || N < 1 || (N % 8) != 0 || N > 1024 || M > 128) return false;
    int kc = (K + 255) / 256;                     // ~256 workgroups along K ...
    kc = (kc + 1) & ~1;
    if (kc < 32) kc = 32;
    if (kc > 480) kc = 480;                       // ... with the x chunk [32][kc + 1] within 64 KiB of LDS
    p.kc = kc;
    p.chunks = (K + kc - 1) / kc;
    p.mblocks = (M + 31) / 32;
    p.nblocks = (N + kFcCols - 1) / kFcCols;
    return true;
}
// The forward's workspace (the K chunks' partial sums) and the backward's (dz): each call has one array.
size_t carve_fc_part(void *ws, const FcPlan &p, int N, float *&part) { return carve_one(ws, (size_t)p.chunks * p.mblocks * 32 * N, part); }
size_t carve_fc_dz(void *ws, int M, int N, float *&dz) { return carve_one(ws, (size_t)M * N, dz); }
// waves per workgroup of the two streaming kernels: 32 rows of W per wave, the whole grid in ONE resident round
// (two workgroups of ~66 KiB of LDS per CU: 512 slots) -- the model's fc1 (73 728 rows): 5 waves, 461 workgroups
inline int fc_waves(int K, size_t lds)
{
    const int tiles = (K + 31) / 32, slots = lds <= 80 * 1024 ? 512 : 256;
    const int nw = (tiles + slots - 1) / slots;
    return nw < 4 ? 4 : (nw > 8 ? 8 : nw);
}
// dx = dz . W^T
void fc_dx_launch(const float *dz, const float *W, int M, int K, int N, int mblocks, float *dx, hipStream_t s)
{
    Scope sc(K_FC_DX, s);
    const int psteps = (N / 8 + 7) / 8 * 8;                            // (fc_dx_kernel's kD)
    size_t lds = (size_t)32 * (8 * psteps + 4) * 4;                   // the dz tile; the transpose tiles reuse it
    const int nw = fc_waves(K, lds);
    if (lds < (size_t)nw * 32 * 33 * 4) lds = (size_t)nw * 32 * 33 * 4;
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(fc_dx_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(fc_dx_kernel, dim3((unsigned)((K + 32 * nw - 1) / (32 * nw)), (unsigned)mblocks), dim3(64 * nw), lds, s, dz, W,
                       M, K, N, dx);
}

}  // namespace

extern "C" {

size_t conv3p_fc_workspace_bytes(int M, int K, int N)
{
    FcPlan p;
    if (!fc_plan(M, K, N, p)) return 0;
    float *unused;
    return std::max(carve_fc_part(nullptr, p, N, unused), carve_fc_dz(nullptr, M, N, unused));
}

int conv3p_fc_forward_f32(const float *x, const float *W, const float *b, int M, int K, int N, int act, float *y,
                          void *workspace, size_t workspace_bytes, void *stream)
{
    if (M < 0 || K < 0 || N < 0 || (act != 0 && act != 1)) return CONV3P_ERR_INVALID_ARGUMENT;
    if ((size_t)M * N == 0) return CONV3P_OK;
    if (!x || !W || !y || K == 0) return CONV3P_ERR_INVALID_ARGUMENT;
    FcPlan p;
    if (!fc_plan(M, K, N, p)) return CONV3P_ERR_UNSUPPORTED;
    float *part;
    TRY(buf_check(workspace, workspace_bytes, carve_fc_part(workspace, p, N, part)));
    hipStream_t s = static_cast<hipStream_t>(stream);
    {
        Scope sc(K_FC_FWD, s);
        const int psteps = ((p.kc + 1) / 2 + kFcDepth - 1) / kFcDepth * kFcDepth;
        const size_t lds = (size_t)32 * (2 * psteps + 1) * 4;
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(fc_forward_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(fc_forward_kernel, dim3((unsigned)p.chunks, (unsigned)p.mblocks, (unsigned)p.nblocks), dim3(256), lds, s,
                           x, W, M, K, N, p.kc, part);
        const size_t n = (size_t)M * N;
        hipLaunchKernelGGL(fc_finish_kernel, dim3((unsigned)((n + 63) / 64)), dim3(1024), 0, s, part, b, M, N, p.chunks,
                           p.mblocks, act, y);
    }
    return hip_ok();
}

int conv3p_fc_backward_f32(const float *x, const float *W, const float *y, const float *dy, int M, int K, int N,
                           int act, float *dx, float *dW, float *db, void *workspace, size_t workspace_bytes,
                           void *stream)
{
    if (M < 0 || K < 0 || N < 0 || (act != 0 && act != 1)) return CONV3P_ERR_INVALID_ARGUMENT;
    if ((size_t)K * N == 0) return CONV3P_OK;
    if (M == 0) {                                                       // empty sums: dW = 0 and db = sum_m dz = 0
        if (!dW) return CONV3P_ERR_INVALID_ARGUMENT;
        TRY(zero_async(dW, (size_t)K * N * 4, static_cast<hipStream_t>(stream)));
        return db ? zero_async(db, (size_t)N * 4, static_cast<hipStream_t>(stream)) : CONV3P_OK;
    }
    if (!x || !W || !dy || !dW || (act && !y)) return CONV3P_ERR_INVALID_ARGUMENT;
    FcPlan p;
    if (!fc_plan(M, K, N, p)) return CONV3P_ERR_UNSUPPORTED;
    float *dz;
    // (against the declared size, which also covers the forward's partials: see seg_declared_bytes)
    TRY(buf_check(workspace, workspace_bytes, std::max(carve_fc_dz(workspace, M, N, dz), conv3p_fc_workspace_bytes(M, K, N))));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int dw_steps = M <= 32 ? 16 : M <= 64 ? 32 : 64;
    if ((size_t)2 * dw_steps * (N + 1) * 4 > kMaxLds) return CONV3P_ERR_UNSUPPORTED;   // before anything is launched
    hipLaunchKernelGGL(fc_dz_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, y, dy, M, N, act, dz, db);
    TRY(hip_ok());
    {
        Scope sc(K_FC_DW, s);
        auto launch = [&](auto kern, int steps) {
            const size_t lds = (size_t)2 * steps * (N + 1) * 4;
            const int nw = fc_waves(K, lds);
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            hipLaunchKernelGGL(kern, dim3((unsigned)((K + 32 * nw - 1) / (32 * nw))), dim3(64 * nw), lds, s, x, dz, M, K, N, dW);
        };
        if (M <= 32) launch(fc_dw_kernel<16>, 16);
        else if (M <= 64) launch(fc_dw_kernel<32>, 32);
        else launch(fc_dw_kernel<64>, 64);
    }
    TRY(hip_ok());
    if (dx != nullptr) fc_dx_launch(dz, W, M, K, N, p.mblocks, dx, s);
    return hip_ok();
}

size_t conv3p_seg_head_workspace_bytes(size_t rows, int num_class)
{
    if (rows == 0 || num_class < 2 || num_class > kSegMaxClass) return 0;
    return seg_declared_bytes(rows, num_class);
}
int conv3p_seg_head_f32(const float *act, const int32_t *labels, size_t rows, int num_class, float grad_scale,
                        float *grad_act, int32_t *pred, double *loss_sum, int64_t *counts, void *workspace,
                        size_t workspace_bytes, void *stream)
{
    return seg_head_impl<float>(act, labels, rows, num_class, grad_scale, grad_act, pred, loss_sum, counts, workspace,
                                workspace_bytes, stream);
}
int conv3p_seg_head_f64(const double *act, const int32_t *labels, size_t rows, int num_class, double grad_scale,
                        double *grad_act, int32_t *pred, double *loss_sum, int64_t *counts, void *workspace,
                        size_t workspace_bytes, void *stream)
{
    return seg_head_impl<double>(act, labels, rows, num_class, grad_scale, grad_act, pred, loss_sum, counts, workspace,
                                 workspace_bytes, stream);
}

size_t conv3p_seg_head_weighted_workspace_bytes(size_t rows, int num_class)
{
    const size_t head = conv3p_seg_head_workspace_bytes(rows, num_class);
    if (head == 0) return 0;
    return seg_weighted_declared_bytes(rows, num_class);
}
int conv3p_seg_weight_total_f32(const int32_t *labels, size_t rows, int num_class, const float *class_weight,
                                const float *point_weight, double *total, void *workspace, size_t workspace_bytes,
                                void *stream)
{
    return seg_weight_total_impl<float>(labels, rows, num_class, class_weight, point_weight, total, workspace,
                                        workspace_bytes, stream);
}
int conv3p_seg_weight_total_f64(const int32_t *labels, size_t rows, int num_class, const double *class_weight,
                                const double *point_weight, double *total, void *workspace, size_t workspace_bytes,
                                void *stream)
{
    return seg_weight_total_impl<double>(labels, rows, num_class, class_weight, point_weight, total, workspace,
                                         workspace_bytes, stream);
}
int conv3p_seg_head_weighted_f32(const float *act, const int32_t *labels, size_t rows, int num_class,
                                 const float *class_weight, const float *point_weight, double label_smoothing,
                                 float grad_scale, const double *denominator, float *grad_act, int32_t *pred,
                                 double *loss_sum, int64_t *counts, void *workspace, size_t workspace_bytes, void *stream)
{
    return seg_head_weighted_impl<float>(act, labels, rows, num_class, class_weight, point_weight, label_smoothing,
                                         grad_scale, denominator, grad_act, pred, loss_sum, counts, workspace,
                                         workspace_bytes, stream);
}
int conv3p_seg_head_weighted_f64(const double *act, const int32_t *labels, size_t rows, int num_class,
                                 const double *class_weight, const double *point_weight, double label_smoothing,
                                 double grad_scale, const double *denominator, double *grad_act, int32_t *pred,
                                 double *loss_sum, int64_t *counts, void *workspace, size_t workspace_bytes, void *stream)
{
    return seg_head_weighted_impl<double>(act, labels, rows, num_class, class_weight, point_weight, label_smoothing,
                                          grad_scale, denominator, grad_act, pred, loss_sum, counts, workspace,
                                          workspace_bytes, stream);
}

size_t conv3p_seg_confusion_workspace_bytes(size_t rows, int num_class)
{
    if (rows == 0 || num_class < 2 || num_class > kSegMaxClass) return 0;
    return up((size_t)seg_conf_grid(rows) * num_class * num_class * sizeof(int));
}
int conv3p_seg_confusion(const int32_t *labels, const int32_t *pred, size_t rows, int num_class, int64_t *confusion,
                         void *workspace, size_t workspace_bytes, void *stream)
{
    if (rows == 0 || num_class < 2 || !labels || !pred || !confusion) return CONV3P_ERR_INVALID_ARGUMENT;
    if (num_class > kSegMaxClass || rows > ((size_t)1 << 36)) return CONV3P_ERR_UNSUPPORTED;   // (int32 partial counters)
    TRY(buf_check(workspace, workspace_bytes, conv3p_seg_confusion_workspace_bytes(rows, num_class)));
    hipStream_t s = static_cast<hipStream_t>(stream);
    int *part = static_cast<int *>(workspace);
    const unsigned grid = seg_conf_grid(rows);
    const int cells = num_class * num_class;
    const size_t lds = (size_t)cells * sizeof(int);
    {
        Scope sc(K_SEG_HEAD, s);
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(seg_confusion_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(seg_confusion_kernel, dim3(grid), dim3(kSegConfThreads), lds, s, labels, pred, rows, num_class,
                           part);
        hipLaunchKernelGGL(seg_confusion_finish_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, part,
                           (int)grid, cells, reinterpret_cast<long long *>(confusion));
    }
    return hip_ok();
}

int conv3p_momentum_step_f32(int n_tensors, float *const *params, const float *const *grads, float *const *accums,
                             const size_t *numels, float lr, float momentum, void *stream)
{
    return momentum_step_impl<float>(n_tensors, params, grads, accums, numels, lr, momentum, stream);
}
int conv3p_momentum_step_f64(int n_tensors, double *const *params, const double *const *grads, double *const *accums,
                             const size_t *numels, double lr, double momentum, void *stream)
{
    return momentum_step_impl<double>(n_tensors, params, grads, accums, numels, lr, momentum, stream);
}

size_t conv3p_grad_norm_workspace_bytes(void) { return grad_norm_bytes(); }
int conv3p_grad_norm_f32(int n_tensors, const float *const *grads, const size_t *numels, double *stats, int accumulate,
                         void *workspace, size_t workspace_bytes, void *stream)
{
    return grad_norm_impl<float>(n_tensors, grads, numels, stats, accumulate, workspace, workspace_bytes, stream);
}
int conv3p_grad_norm_f64(int n_tensors, const double *const *grads, const size_t *numels, double *stats, int accumulate,
                         void *workspace, size_t workspace_bytes, void *stream)
{
    return grad_norm_impl<double>(n_tensors, grads, numels, stats, accumulate, workspace, workspace_bytes, stream);
}
int conv3p_momentum_step_guarded_f32(int n_tensors, float *const *params, const float *const *grads, float *const *accums,
                                     const size_t *numels, float lr, float momentum, int nesterov, float clip_norm,
                                     int skip_nonfinite, const double *stats, void *stream)
{
    return momentum_step_guarded_impl<float>(n_tensors, params, grads, accums, numels, lr, momentum, nesterov, clip_norm,
                                             skip_nonfinite, stats, stream);
}
int conv3p_momentum_step_guarded_f64(int n_tensors, double *const *params, const double *const *grads,
                                     double *const *accums, const size_t *numels, double lr, double momentum, int nesterov,
                                     double clip_norm, int skip_nonfinite, const double *stats, void *stream)
{
    return momentum_step_guarded_impl<double>(n_tensors, params, grads, accums, numels, lr, momentum, nesterov, clip_norm,
                                              skip_nonfinite, stats, stream);
}
int conv3p_fc_backward_step_f32(const float *x, float *W, float *b, const float *y, const float *dy, int M, int K, int N,
                                int act, float *dx, float *accum_W, float *accum_b, float lr, float momentum,
                                void *workspace, size_t workspace_bytes, void *stream)
{
    if (M < 0 || K < 0 || N < 0 || (act != 0 && act != 1)) return CONV3P_ERR_INVALID_ARGUMENT;
    if ((b == nullptr) != (accum_b == nullptr)) return CONV3P_ERR_INVALID_ARGUMENT;
    if ((size_t)K * N == 0) return CONV3P_OK;
    if (M == 0) return CONV3P_ERR_INVALID_ARGUMENT;
    if (!x || !W || !dy || !accum_W || (act && !y)) return CONV3P_ERR_INVALID_ARGUMENT;
    FcPlan p;
    if (!fc_plan(M, K, N, p)) return CONV3P_ERR_UNSUPPORTED;
    float *dz;
    // (against the declared size, which also covers the forward's partials: see seg_declared_bytes)
    TRY(buf_check(workspace, workspace_bytes, std::max(carve_fc_dz(workspace, M, N, dz), conv3p_fc_workspace_bytes(M, K, N))));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int dw_steps = M <= 32 ? 16 : M <= 64 ? 32 : 64;
    if ((size_t)2 * dw_steps * (N + 1) * 4 > kMaxLds) return CONV3P_ERR_UNSUPPORTED;   // before anything is launched
    hipLaunchKernelGGL(fc_dz_step_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, y, dy, M, N, act, dz, b, accum_b,
                       lr, momentum);
    TRY(hip_ok());
    if (dx != nullptr) fc_dx_launch(dz, W, M, K, N, p.mblocks, dx, s);   // FIRST: dx = dz . W^T needs the old W
    TRY(hip_ok());
    {
        Scope sc(K_FC_DW, s);                                              // (no profile kind of its own: the table is pinned)
        auto launch = [&](auto kern, int steps) {
            const size_t lds = (size_t)2 * steps * (N + 1) * 4;
            const int nw = fc_waves(K, lds);
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
            hipLaunchKernelGGL(kern, dim3((unsigned)((K + 32 * nw - 1) / (32 * nw))), dim3(64 * nw), lds, s, x, dz, M, K, N, W,
                               accum_W, lr, momentum);
        };
        if (M <= 32) launch(fc_dw_step_kernel<16>, 16);
        else if (M <= 64) launch(fc_dw_step_kernel<32>, 32);
        else launch(fc_dw_step_kernel<64>, 64);
    }
    return hip_ok();
}

size_t conv3p_cls_tail_workspace_bytes(int M, int H, int C)
{
    ClsTailArgs a;
    return cls_shape_ok(M, H, C) ? carve_cls(nullptr, M, H, C, a) : 0;
}
int conv3p_cls_tail_f32(const float *fc1, const float *W2, const float *b2, const int32_t *labels, int M, int H, int C,
                        int training, double rate, const float *keep_mask, uint64_t seed, uint64_t step, float grad_scale,
                        float *logits, int32_t *pred, float *dfc1, float *dW2, float *db2, uint8_t *keep_out,
                        double *loss_sum, int64_t *counts, void *workspace, size_t workspace_bytes, void *stream)
{
    return cls_tail_impl(fc1, const_cast<float *>(W2), const_cast<float *>(b2), labels, M, H, C, training, rate, keep_mask,
                         seed, step, grad_scale, logits, pred, dfc1, dW2, db2, nullptr, nullptr, 0.0f, 0.0f, keep_out,
                         loss_sum, counts, workspace, workspace_bytes, stream);
}
int conv3p_cls_tail_step_f32(const float *fc1, float *W2, float *b2, const int32_t *labels, int M, int H, int C,
                             int training, double rate, const float *keep_mask, uint64_t seed, uint64_t step,
                             float grad_scale, float *logits, int32_t *pred, float *dfc1, float *accum_W2, float *accum_b2,
                             float lr, float momentum, uint8_t *keep_out, double *loss_sum, int64_t *counts,
                             void *workspace, size_t workspace_bytes, void *stream)
{
    if (!accum_W2 || !accum_b2 || !dfc1) return CONV3P_ERR_INVALID_ARGUMENT;
    return cls_tail_impl(fc1, W2, b2, labels, M, H, C, training, rate, keep_mask, seed, step, grad_scale, logits, pred, dfc1,
                         nullptr, nullptr, accum_W2, accum_b2, lr, momentum, keep_out, loss_sum, counts, workspace,
                         workspace_bytes, stream);
}

}  // extern "C"
