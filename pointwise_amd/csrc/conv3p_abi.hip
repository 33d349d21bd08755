// conv3p_abi.hip -- host side of libconv3p_hip.so: the C ABI declared in include/conv3p.h, include/conv3p_graph.h and
// include/conv3p_knn.h; include/conv3p_match.h declares the segment matching.
//
// Replaces the host glue of the reference's GPU op (tf_conv3p_atrous.cu:541-642, :659-775):
// no blocking D2H copies (stride / voxel arrive by value), no per-call temp allocation
// (caller-provided workspace / cache), no default-stream launches (everything on `stream`),
// status codes instead of OP_REQUIRES / exit().
//
// Pipeline of one op call (all on the caller's stream, no host synchronisation):
//   prep_sort_kernel   hash the clouds; re-sort + re-box only clouds whose content changed
//   search_kernel      per-tap populations + centre-major pair lists   (skipped per cloud when the slot is
//                      current; its last workgroup per cloud commits the slot)
//   forward_kernel / backward_kernel + reduce_partials_kernel          the accumulation (register path), or
//   deep_order / deep_sched / deep_plan + deep_gemm / deep_dw / deep_reduce   (matrix-core path, conv3p_deep.hpp), or
//   the generic forms of forward_kernel / backward_kernel (any channel counts, fp64)
// The stateless entry points run the same kernels on the caller's scratch with force = 1.
//
// One translation unit.  This file holds the single-layer calls (forward, backward, prepare, neighbour count, SELU) and
// their exports; everything they are made of is in host-only headers, one concern each, included in dependency order:
// conv3p_abi_{profile, layout, cache, search, routes, blocks}.hpp before the calls, conv3p_abi_stack.hpp (which composes
// them) after, then the other subsystems (heads, pre-step, scene, grid, the k-nearest-voxel search, the segment matching).  DESIGN.md section 1 has the table.
#include "../../include/conv3p.h"
#include "../../include/conv3p_graph.h"
#include "../../include/conv3p_knn.h"
#include "../../include/conv3p_match.h"
#include "conv3p_host.hpp"
#include "conv3p_kernels.hpp"
#include "conv3p_stack_fused.hpp"
#include "conv3p_prestep.hpp"
#include "conv3p_head.hpp"
#include "conv3p_seg_head.hpp"
#include "conv3p_seg_head_weighted.hpp"
#include "conv3p_optim.hpp"
#include "conv3p_optim_guarded.hpp"
#include "conv3p_cls_tail.hpp"
#include "conv3p_provider.hpp"
#include "conv3p_sort_wide.hpp"
#include "conv3p_scene.hpp"
#include "conv3p_scene_cover.hpp"
#include "conv3p_scene_rooms.hpp"
#include "conv3p_grid.hpp"
#include "conv3p_grid_rooms.hpp"
#include "conv3p_grid_interp.hpp"
#include "conv3p_grid_interp_rings.hpp"
#include "conv3p_grid_normals.hpp"
#include "conv3p_grid_segments.hpp"
#include "conv3p_grid_geometry.hpp"
#include "conv3p_grid_adjacency.hpp"
#include "conv3p_grid_agglomerate.hpp"
#include "conv3p_grid_smooth.hpp"
#include "conv3p_grid_knn.hpp"
#include "conv3p_grid_match.hpp"

#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

using namespace conv3p;

#include "conv3p_abi_profile.hpp"
#include "conv3p_abi_layout.hpp"
#include "conv3p_abi_cache.hpp"
#include "conv3p_abi_search.hpp"
#include "conv3p_abi_routes.hpp"
#include "conv3p_abi_blocks.hpp"

namespace {

template <typename T> int selu_impl(const T *x, T *y, size_t n, void *stream)
{
    if (n == 0) return CONV3P_OK;
    if (!x || !y) return CONV3P_ERR_INVALID_ARGUMENT;
    hipStream_t s = static_cast<hipStream_t>(stream);
    Scope sc(K_SELU, s);
    const unsigned grid = capped_grid((n + 255) / 256, 2048);
    hipLaunchKernelGGL(selu_kernel<T>, dim3(grid), dim3(256), 0, s, x, y, n);
    return hip_ok();
}
// rows x cols values; lds = {ld_y, ld_dy, ld_b, ld_dx} or nullptr for dense operands
template <typename T>
int selu_grad_impl(const T *y, const T *dy, const T *dy_b, T *dx, size_t rows, int cols, const int *lds, void *stream)
{
    const size_t n = rows * (size_t)cols;
    if (n == 0) return CONV3P_OK;
    if (!y || !dy || !dx) return CONV3P_ERR_INVALID_ARGUMENT;
    hipStream_t s = static_cast<hipStream_t>(stream);
    Scope sc(K_SELU_GRAD, s);
    const unsigned grid = capped_grid((n + 255) / 256, 2048);
    hipLaunchKernelGGL(selu_grad_kernel<T>, dim3(grid), dim3(256), 0, s, y, dy, dy_b, dx, rows, cols,
                       lds ? lds[0] : cols, lds ? lds[1] : cols, lds ? lds[2] : cols, lds ? lds[3] : cols);
    return hip_ok();
}

template <typename T>
int forward_impl(const T *points, const T *input, const T *filter, const int32_t *stride, T voxel, int B,
                 int N, int Cin, int Cout, int fz, int fy, int fx, T *output, const Where &wh, void *stream,
                 bool act = false, const RowLd *ldp = nullptr)
{
    Dims d{B, N, Cin, Cout, fz, fy, fx, 0, 0};
    TRY(check(d, stride, (double)voxel, true));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t out_elems = (size_t)B * N * Cout;
    if (out_elems == 0) return CONV3P_OK;
    if (!points || !output || (Cin > 0 && (!input || !filter))) return CONV3P_ERR_INVALID_ARGUMENT;
    if (Cin == 0) return zero_async(output, out_elems * sizeof(T), s);   // empty contraction; selu(0) == 0
    Call<T> c;
    c.act = act;
    set_ld(c, ldp, Cin, Cout);
    const size_t scratch = forward_scratch_bytes(d, (int)sizeof(T), wh.ppp, wh.persistent);
    const Route r = plan_forward<T>(d, make_stencil<T>(d, stride, voxel), plan_args<T>(d, wh, c.strided, scratch));
    if (r.family == Family::Unsupported) return CONV3P_ERR_UNSUPPORTED;   // (before anything is launched or recorded)
    TRY(begin_call<T>(c, d, stride, voxel, scratch, wh, s, r.family == Family::MatrixCore));
    TRY(run_geometry<T>(points, c));
    switch (r.family) {
    case Family::Register:   // (SELU fused into the kernels)
        return register_shape<T>(Cin, Cout)->forward(c, r, input, filter, output);
    case Family::MatrixCore:
        if constexpr (sizeof(T) == 4) TRY(deep_shape(r.cip, r.cop)->forward(c, r, input, filter, output));
        break;
    case Family::Wide:
        if constexpr (sizeof(T) == 4) TRY(wide_forward(c, r, input, filter, output));
        break;
    case Family::F64Blocks:
        if constexpr (sizeof(T) == 8) TRY(f64_blocked_forward(c, r, input, filter, output));
        break;
    default:
        TRY(zero_async(output, out_elems * sizeof(T), s));   // .cpp:451
        TRY((launch_forward<T, 0, 0>(c, r.lds, false, input, filter, output)));
        break;
    }
    return act ? selu_impl<T>(output, output, out_elems, stream) : CONV3P_OK;   // paths without a fused epilogue
}

// geometry only: what a later forward / backward with the same points + stencil will find ready
template <typename T>
int prepare_impl(const T *points, const int32_t *stride, T voxel, int B, int N, int fz, int fy, int fx,
                 const Where &wh, void *stream)
{
    Dims d{B, N, 0, 0, fz, fy, fx, 0, 0};
    TRY(check(d, stride, (double)voxel, false));
    if ((size_t)B * N == 0) return CONV3P_OK;
    if (!points) return CONV3P_ERR_INVALID_ARGUMENT;
    Call<T> c;
    TRY(begin_call<T>(c, d, stride, voxel, 0, wh, static_cast<hipStream_t>(stream)));
    TRY(run_geometry<T>(points, c));
    if constexpr (sizeof(T) == 4) {
        // CONV3P_CACHE_PREPARE_DEEP_ORDERS: also the matrix-core path's two record orders (forward and backward taps),
        // so that the layer's calls on these points find them in the scratch region
        if (wh.persistent && (wh.flags & CONV3P_CACHE_PREPARE_DEEP_ORDERS) != 0) {
            const size_t pair_slots = (size_t)d.B * c.L.pairs_per_cloud;
            if (wh.scratch_cap < deep_order_bytes(c.d, pair_slots)) return CONV3P_ERR_WORKSPACE;
            c.order_ok[0] = c.order_ok[1] = false;
            TRY(launch_deep_order<false>(c, carve_deep(c.d, pair_slots, c.L.partials, 0)));
            TRY(launch_deep_order<true>(c, carve_deep(c.d, pair_slots, c.L.partials, 1)));
        }
    }
    return CONV3P_OK;
}

template <typename T>
int backward_impl(const T *grad_out, const T *points, const T *input, const T *filter,
                  const int32_t *stride, T voxel, int B, int N, int Cin, int Cout, int fz, int fy, int fx,
                  T *grad_input, T *grad_filter, const Where &wh, void *stream, bool act = false,
                  const T *addend = nullptr, const RowLd *ldp = nullptr, DeferredReduce<T> *defer = nullptr)
{
    Dims d{B, N, Cin, Cout, fz, fy, fx, 0, 0};
    TRY(check(d, stride, (double)voxel, true));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t nw = (size_t)d.ntap * Cin * Cout;
    const size_t dx_elems = (size_t)B * N * Cin;
    if ((dx_elems && !grad_input) || (nw && !grad_filter)) return CONV3P_ERR_INVALID_ARGUMENT;
    if (ldp && (dx_elems == 0 || Cout == 0)) return CONV3P_ERR_UNSUPPORTED;
    if (dx_elems == 0 || Cout == 0) {                                    // nothing to accumulate
        TRY(zero_async(grad_input, dx_elems * sizeof(T), s));            // .cpp:580
        TRY(zero_async(grad_filter, nw * sizeof(T), s));                 // .cpp:590
        if (act && dx_elems && addend) {
            if (!input) return CONV3P_ERR_INVALID_ARGUMENT;
            return selu_grad_impl<T>(input, addend, nullptr, grad_input, (size_t)B * N, Cin, nullptr, stream);
        }
        return CONV3P_OK;
    }
    if (!points || !input || !filter || !grad_out) return CONV3P_ERR_INVALID_ARGUMENT;
    Call<T> c;
    c.act = act;
    c.addend = addend;
    set_ld(c, ldp, Cin, Cout);
    const size_t scratch = backward_scratch_bytes(d, (int)sizeof(T), wh.ppp);
    const Route r = plan_backward<T>(d, make_stencil<T>(d, stride, voxel), plan_args<T>(d, wh, c.strided, scratch));
    if (r.family == Family::Unsupported) return CONV3P_ERR_UNSUPPORTED;   // (before anything is launched or recorded)
    TRY(begin_call<T>(c, d, stride, voxel, scratch, wh, s, r.family == Family::MatrixCore));
    TRY(run_geometry<T>(points, c));
    if (defer && defer->ride.nslots > 0 && r.family == Family::Register && rider_fits<T>(r)) {
        c.rider = defer->ride;
        defer->rode = true;
    }
    // the register kernels leave per-workgroup grad_filter partials: in the stack's region when it reduces them later
    T *partials = defer && !r.self_reduces ? defer->region : c.L.partials;
    switch (r.family) {
    case Family::Register:   // (SELU fused into the kernels)
        TRY(register_shape<T>(Cin, Cout)->backward(c, r, grad_out, input, filter, grad_input, partials));
        break;
    case Family::Split36x13:   // (SELU fused into its last pass)
        return backward_split_36_13<T>(c, r, grad_out, input, filter, grad_input, grad_filter);
    case Family::MatrixCore:
        if constexpr (sizeof(T) == 4) TRY(deep_shape(r.cip, r.cop)->backward(c, r, grad_out, input, filter, grad_input, grad_filter));
        break;
    case Family::Wide:
        if constexpr (sizeof(T) == 4) TRY(wide_backward(c, r, grad_out, input, filter, grad_input, grad_filter));
        break;
    case Family::F64Blocks:
        if constexpr (sizeof(T) == 8) TRY(f64_blocked_backward(c, r, grad_out, input, filter, grad_input, grad_filter));
        break;
    default:
        TRY(zero_async(grad_input, dx_elems * sizeof(T), s));
        TRY(zero_async(c.L.partials, nw * (size_t)r.slots * sizeof(T), s));
        TRY((launch_backward<T, 0, 0>(c, r.lds, grad_out, input, filter, grad_input, c.L.partials, nullptr, r.slots)));
        break;
    }
    if (defer && !r.self_reduces) {   // reduced later, together with the stack's other layers
        defer->job = ReduceJob<T>{partials, grad_filter, r.slots, (unsigned)nw};
        return CONV3P_OK;
    }
    if (r.family == Family::Register || r.family == Family::Generic) {
        Scope sc(K_REDUCE, s);
        hipLaunchKernelGGL(reduce_partials_kernel<T>, dim3((unsigned)((nw + kReduceW - 1) / kReduceW)), dim3(1024), 0, s,
                           c.L.partials, r.slots, nw, grad_filter);
        TRY(hip_ok());
    }
    if (act && r.family != Family::Register)   // paths without a fused epilogue
        return selu_grad_impl<T>(input, grad_input, addend, grad_input, (size_t)B * N, Cin, nullptr, stream);
    return CONV3P_OK;
}

template <typename T>
int count_impl(const T *points, const int32_t *stride, T voxel, int B, int N, int fz, int fy, int fx,
               int32_t *count, void *ws, size_t ws_bytes, void *stream)
{
    Dims d{B, N, 0, 0, fz, fy, fx, 0, 0};
    TRY(check(d, stride, (double)voxel, false));
    if ((size_t)B * N == 0) return CONV3P_OK;
    if (!points || !count) return CONV3P_ERR_INVALID_ARGUMENT;
    hipStream_t s = static_cast<hipStream_t>(stream);
    Call<T> c;
    TRY(begin_call<T>(c, d, stride, voxel, 0, populations_only(ws, ws_bytes, d.ntap), s));
    TRY(run_prep<T>(points, c));
    TRY(run_cloud_min<T>(points, c));
    return run_search<T>(c, count, false);
}

}  // namespace

#include "conv3p_abi_stack.hpp"

extern "C" {

#define FWD_ARGS(T)                                                                                            \
    const T *points, const T *input, const T *filter, const int32_t *stride_xyz, T voxel_size, int B, int N,   \
        int Cin, int Cout, int fz, int fy, int fx, T *output
#define FWD_PASS points, input, filter, stride_xyz, voxel_size, B, N, Cin, Cout, fz, fy, fx, output
#define BWD_ARGS(T)                                                                                            \
    const T *grad_out, const T *points, const T *input, const T *filter, const int32_t *stride_xyz,            \
        T voxel_size, int B, int N, int Cin, int Cout, int fz, int fy, int fx, T *grad_input, T *grad_filter
#define BWD_PASS                                                                                               \
    grad_out, points, input, filter, stride_xyz, voxel_size, B, N, Cin, Cout, fz, fy, fx, grad_input, grad_filter

int conv3p_forward_f32(FWD_ARGS(float), void *workspace, size_t workspace_bytes, void *stream)
{
    return forward_impl<float>(FWD_PASS, stateless(workspace, workspace_bytes), stream);
}
int conv3p_forward_f64(FWD_ARGS(double), void *workspace, size_t workspace_bytes, void *stream)
{
    return forward_impl<double>(FWD_PASS, stateless(workspace, workspace_bytes), stream);
}
int conv3p_backward_f32(BWD_ARGS(float), void *workspace, size_t workspace_bytes, void *stream)
{
    return backward_impl<float>(BWD_PASS, stateless(workspace, workspace_bytes), stream);
}
int conv3p_backward_f64(BWD_ARGS(double), void *workspace, size_t workspace_bytes, void *stream)
{
    return backward_impl<double>(BWD_PASS, stateless(workspace, workspace_bytes), stream);
}

#define CACHE_ARGS void *cache, size_t cache_bytes, const conv3p_cache_config *cfg, void *stream
#define CACHE_WHERE(elem)                                                                                      \
    persistent(elem, B, N, cache, cache_bytes, cfg, cfg->flags)
int conv3p_forward_cached_f32(FWD_ARGS(float), CACHE_ARGS)
{
    if (!cache_cfg_ok(cfg)) return CONV3P_ERR_INVALID_ARGUMENT;
    return forward_impl<float>(FWD_PASS, CACHE_WHERE(4), stream);
}
int conv3p_forward_cached_f64(FWD_ARGS(double), CACHE_ARGS)
{
    if (!cache_cfg_ok(cfg)) return CONV3P_ERR_INVALID_ARGUMENT;
    return forward_impl<double>(FWD_PASS, CACHE_WHERE(8), stream);
}
int conv3p_backward_cached_f32(BWD_ARGS(float), CACHE_ARGS)
{
    if (!cache_cfg_ok(cfg)) return CONV3P_ERR_INVALID_ARGUMENT;
    return backward_impl<float>(BWD_PASS, CACHE_WHERE(4), stream);
}
int conv3p_backward_cached_f64(BWD_ARGS(double), CACHE_ARGS)
{
    if (!cache_cfg_ok(cfg)) return CONV3P_ERR_INVALID_ARGUMENT;
    return backward_impl<double>(BWD_PASS, CACHE_WHERE(8), stream);
}

int conv3p_layer_forward_cached_f32(FWD_ARGS(float), CACHE_ARGS)
{
    if (!cache_cfg_ok(cfg)) return CONV3P_ERR_INVALID_ARGUMENT;
    return forward_impl<float>(FWD_PASS, CACHE_WHERE(4), stream, true);
}
int conv3p_layer_forward_cached_f64(FWD_ARGS(double), CACHE_ARGS)
{
    if (!cache_cfg_ok(cfg)) return CONV3P_ERR_INVALID_ARGUMENT;
    return forward_impl<double>(FWD_PASS, CACHE_WHERE(8), stream, true);
}
#define LAYER_BWD_ARGS(T)                                                                                      \
    const T *grad_out, const T *points, const T *input, const T *filter, const int32_t *stride_xyz,            \
        T voxel_size, int B, int N, int Cin, int Cout, int fz, int fy, int fx, const T *grad_addend,           \
        T *grad_input, T *grad_filter
int conv3p_layer_backward_cached_f32(LAYER_BWD_ARGS(float), CACHE_ARGS)
{
    if (!cache_cfg_ok(cfg)) return CONV3P_ERR_INVALID_ARGUMENT;
    return backward_impl<float>(BWD_PASS, CACHE_WHERE(4), stream, true, grad_addend);
}
int conv3p_layer_backward_cached_f64(LAYER_BWD_ARGS(double), CACHE_ARGS)
{
    if (!cache_cfg_ok(cfg)) return CONV3P_ERR_INVALID_ARGUMENT;
    return backward_impl<double>(BWD_PASS, CACHE_WHERE(8), stream, true, grad_addend);
}

int conv3p_cache_prepare_f32(const float *points, const int32_t *stride_xyz, float voxel_size, int B, int N,
                             int fz, int fy, int fx, CACHE_ARGS)
{
    if (!cache_cfg_ok(cfg)) return CONV3P_ERR_INVALID_ARGUMENT;
    return prepare_impl<float>(points, stride_xyz, voxel_size, B, N, fz, fy, fx, CACHE_WHERE(4), stream);
}
int conv3p_cache_prepare_f64(const double *points, const int32_t *stride_xyz, double voxel_size, int B, int N,
                             int fz, int fy, int fx, CACHE_ARGS)
{
    if (!cache_cfg_ok(cfg)) return CONV3P_ERR_INVALID_ARGUMENT;
    return prepare_impl<double>(points, stride_xyz, voxel_size, B, N, fz, fy, fx, CACHE_WHERE(8), stream);
}

int conv3p_cache_prepare_multi_f32(const float *points, const int32_t *strides_xyz, int n_strides,
                                   float voxel_size, int B, int N, int fz, int fy, int fx, CACHE_ARGS)
{
    if (!cache_cfg_ok(cfg)) return CONV3P_ERR_INVALID_ARGUMENT;
    return prepare_multi_impl<float>(points, strides_xyz, n_strides, voxel_size, B, N, fz, fy, fx, CACHE_WHERE(4),
                                     stream);
}
int conv3p_cache_prepare_multi_f64(const double *points, const int32_t *strides_xyz, int n_strides,
                                   double voxel_size, int B, int N, int fz, int fy, int fx, CACHE_ARGS)
{
    if (!cache_cfg_ok(cfg)) return CONV3P_ERR_INVALID_ARGUMENT;
    return prepare_multi_impl<double>(points, strides_xyz, n_strides, voxel_size, B, N, fz, fy, fx, CACHE_WHERE(8),
                                      stream);
}

int conv3p_neighbor_count_f32(const float *points, const int32_t *stride_xyz, float voxel_size, int B,
                              int N, int fz, int fy, int fx, int32_t *count, void *workspace,
                              size_t workspace_bytes, void *stream)
{
    return count_impl<float>(points, stride_xyz, voxel_size, B, N, fz, fy, fx, count, workspace,
                             workspace_bytes, stream);
}
int conv3p_neighbor_count_f64(const double *points, const int32_t *stride_xyz, double voxel_size, int B,
                              int N, int fz, int fy, int fx, int32_t *count, void *workspace,
                              size_t workspace_bytes, void *stream)
{
    return count_impl<double>(points, stride_xyz, voxel_size, B, N, fz, fy, fx, count, workspace,
                              workspace_bytes, stream);
}

int conv3p_selu_f32(const float *x, float *y, size_t n, void *stream) { return selu_impl<float>(x, y, n, stream); }
int conv3p_selu_f64(const double *x, double *y, size_t n, void *stream) { return selu_impl<double>(x, y, n, stream); }
int conv3p_selu_grad_f32(const float *y, const float *dy, float *dx, size_t n, void *stream)
{
    return selu_grad_impl<float>(y, dy, nullptr, dx, n, 1, nullptr, stream);
}
int conv3p_selu_grad_f64(const double *y, const double *dy, double *dx, size_t n, void *stream)
{
    return selu_grad_impl<double>(y, dy, nullptr, dx, n, 1, nullptr, stream);
}
int conv3p_selu_grad_add_f32(const float *y, const float *dy_a, const float *dy_b, float *dx, size_t n,
                             void *stream)
{
    if (n && !dy_b) return CONV3P_ERR_INVALID_ARGUMENT;
    return selu_grad_impl<float>(y, dy_a, dy_b, dx, n, 1, nullptr, stream);
}
int conv3p_selu_grad_add_f64(const double *y, const double *dy_a, const double *dy_b, double *dx, size_t n,
                             void *stream)
{
    if (n && !dy_b) return CONV3P_ERR_INVALID_ARGUMENT;
    return selu_grad_impl<double>(y, dy_a, dy_b, dx, n, 1, nullptr, stream);
}

const char *conv3p_status_string(int status)
{
    switch (status) {
    case CONV3P_OK: return "ok";
    case CONV3P_ERR_INVALID_ARGUMENT: return "invalid argument";
    case CONV3P_ERR_WORKSPACE: return "workspace / cache null, misaligned or too small";
    case CONV3P_ERR_UNSUPPORTED: return "unsupported configuration";
    case CONV3P_ERR_LAUNCH: return "HIP launch error";
    case CONV3P_ERR_NO_DEVICE: return "no HIP device";
    default: return "unknown status";
    }
}
int conv3p_abi_version(void) { return CONV3P_ABI_VERSION; }

}  // extern "C"

#include "conv3p_abi_heads.hpp"
#include "conv3p_abi_prestep.hpp"
#include "conv3p_abi_scene.hpp"
#include "conv3p_abi_grid.hpp"
#include "conv3p_abi_knn.hpp"
#include "conv3p_abi_match.hpp"
