/*
 * conv3p.h -- C ABI of the MI355X-native conv3p operator pair (libconv3p_hip.so).
 *
 * This is the drop-in boundary for the hot path of hkust-vgd/pointwise: the two
 * TensorFlow custom ops `Conv3p` and `Conv3pGrad` of tf_conv3p.so
 *   schema      /root/reference/tf_ops/conv3p/register_op.cpp:44-75   (atrous variant)
 *   CPU kernels /root/reference/tf_ops/conv3p/tf_conv3p_atrous.cpp:401-509, :526-720
 *   GPU kernels /root/reference/tf_ops/conv3p/tf_conv3p_atrous.cu:541-642, :659-775  (replaced)
 *   callers     /root/reference/pointcnn2_acsd.py:10-31,
 *               /root/reference/scene_seg/pointcnn_scene_seg_acsd.py:9-30
 * A TensorFlow OpKernel shim (integration/tf_conv3p_shim.cc) or
 * the Python host mirror (pointwise_amd/conv3p_op.py) binds exactly these symbols.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless
 *     stated otherwise; all tensors dense row-major, dtype float (f32) or double (f64),
 *     the two dtypes the reference registers (register_op.cpp:45).
 *       points  (B, N, 3)            input  (B, N, Cin)
 *       filter  (fz, fy, fx, Cin, Cout)   weight index (f*Cin + k)*Cout + c,
 *                                         tap f = (tz*fy + ty)*fx + tx   (.cpp:290, :490)
 *       output / grad_out (B, N, Cout)    grad_input (B, N, Cin)   grad_filter like filter
 *   - stride_xyz is a HOST pointer to {sx, sy, sz} (the reference's int32[3] `stride`
 *     input, read on the host at .cpp:438-440); voxel_size is passed by value (the
 *     reference's T[1] `voxel_size` input, .cpp:444).  The non-atrous schema
 *     (register_op.cpp:9-38) is the special case stride = {1,1,1}.
 *   - outputs are fully overwritten: the library zero-initialises them itself
 *     (reference: memset at .cpp:451, :580, :590).
 *   - no allocation, no host synchronisation, no stdout in the hot calls: all scratch
 *     comes from the caller's `workspace` (size from conv3p_workspace_bytes), and every
 *     call is ordered on `stream` (a hipStream_t passed as void*; NULL = default stream).
 *   - every function returns a status code (0 = OK); nothing throws or exits.
 *     CONV3P_ERR_INVALID_ARGUMENT corresponds to the reference's
 *     errors::InvalidArgument / OP_REQUIRES failures (.cpp:410-443, :549-585).
 *   - re-entrant and thread-safe for distinct workspaces.
 *   - 64-bit sizes internally: every element offset and byte count is size_t.
 */
#ifndef CONV3P_H
#define CONV3P_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CONV3P_ABI_VERSION 5

/* status codes */
#define CONV3P_OK 0
#define CONV3P_ERR_INVALID_ARGUMENT 1 /* shape / stride / voxel validation failed            */
#define CONV3P_ERR_WORKSPACE 2        /* workspace NULL, misaligned (256 B) or too small     */
#define CONV3P_ERR_UNSUPPORTED 3      /* configuration outside what the kernels handle       */
#define CONV3P_ERR_LAUNCH 4           /* HIP reported an error when launching                */
#define CONV3P_ERR_NO_DEVICE 5        /* no gfx950-class HIP device visible                  */

/* which op the workspace is for */
#define CONV3P_PASS_FORWARD 0
#define CONV3P_PASS_BACKWARD 1
#define CONV3P_PASS_NEIGHBOR_COUNT 2

/* Bytes of scratch the given op needs for these shapes (elem_bytes = 4 or 8).
 * Returns 0 for invalid shapes.  Replaces the reference's per-call
 * OpKernelContext::allocate_temp (tf_conv3p_atrous.cu:97-106, :598-606). */
size_t conv3p_workspace_bytes(int pass, int elem_bytes, int B, int N, int Cin, int Cout, int fz,
                              int fy, int fx);

/* Conv3p forward.  Replaces Conv3pOp<Device,T>::Compute
 * (tf_conv3p_atrous.cpp:401-509 / tf_conv3p_atrous.cu:541-642). */
int conv3p_forward_f32(const float *points, const float *input, const float *filter,
                       const int32_t *stride_xyz, float voxel_size, int B, int N, int Cin,
                       int Cout, int fz, int fy, int fx, float *output, void *workspace,
                       size_t workspace_bytes, void *stream);
int conv3p_forward_f64(const double *points, const double *input, const double *filter,
                       const int32_t *stride_xyz, double voxel_size, int B, int N, int Cin,
                       int Cout, int fz, int fy, int fx, double *output, void *workspace,
                       size_t workspace_bytes, void *stream);

/* Conv3pGrad.  Replaces Conv3pGradOp<Device,T>::Compute
 * (tf_conv3p_atrous.cpp:526-720 / tf_conv3p_atrous.cu:659-775).
 * Input order follows the op schema (register_op.cpp:63-72): grad_from_next first. */
int conv3p_backward_f32(const float *grad_out, const float *points, const float *input,
                        const float *filter, const int32_t *stride_xyz, float voxel_size, int B,
                        int N, int Cin, int Cout, int fz, int fy, int fx, float *grad_input,
                        float *grad_filter, void *workspace, size_t workspace_bytes, void *stream);
int conv3p_backward_f64(const double *grad_out, const double *points, const double *input,
                        const double *filter, const int32_t *stride_xyz, double voxel_size, int B,
                        int N, int Cin, int Cout, int fz, int fy, int fx, double *grad_input,
                        double *grad_filter, void *workspace, size_t workspace_bytes,
                        void *stream);

/* ---------------------------------------------------------------------------------------------
 * Neighbour cache (optional; not in the reference).
 *
 * Everything geometric the ops compute -- curve-sorted point records, per-tap populations and
 * the per-centre neighbour lists with their taps and normalisers -- depends only on `points` and
 * on the stencil (filter extents, stride, voxel_size), not on features, weights or gradients.
 * In the reference's models every layer of a step sees the same `points`, and Conv3pGrad repeats
 * Conv3p's search (pointcnn2_acsd.py:48-66; tf_conv3p_atrous.cu recomputes neighbor_count in both
 * ops).  The *_cached entry points keep that state in a caller-owned, persistent device buffer:
 *
 *   - `cache` must be zero-filled once before its first use and must not be written by the
 *     caller afterwards; one cache serves one (B, N, dtype) at a time (a change of shape simply
 *     invalidates it).  It also holds the per-call scratch, so no separate workspace is needed.
 *   - Validity is decided ON THE DEVICE, per cloud: a 64-bit content hash of the raw coordinates
 *     is recomputed every call (one light kernel) and compared with the hash the lists were built
 *     from; the search / finalise kernels are launched every call and return immediately for
 *     clouds whose lists are current.  There is no host synchronisation and no pointer-identity
 *     assumption: a recycled or overwritten buffer can only cost a rebuild.
 *   - `slots` stencils are kept at once (LRU): 4 for the classification stack, 5 for segmentation.
 *   - Results are bitwise identical to the stateless entry points.
 * The stateless conv3p_forward/backward_* run the very same kernels on `workspace` with the cache
 * logic forced to "rebuild".
 * ------------------------------------------------------------------------------------------- */
typedef struct conv3p_cache_config {
    int slots;           /* stencils cached simultaneously (1..64)                                   */
    int max_taps;        /* largest fz*fy*fx that will be used with this cache (27 for 3x3x3)        */
    int pairs_per_point; /* pair-list capacity per point, averaged over a cloud; 0 = default (256).
                            A cloud that needs more is still handled correctly (slow path).        */
    int max_Cin;         /* largest channel counts of a backward call (sizes the scratch for the   */
    int max_Cout;        /*   per-workgroup grad_filter partials).  Forward calls never need them:  */
                         /*   a forward whose faster variant wants scratch the cache lacks (the     */
                         /*   transform + gather forward of 36 -> 13) runs the plain kernel instead, */
                         /*   same results.  Wide (matrix-core) layers need a cache sized for them. */
    int flags;           /* CONV3P_CACHE_* bits below                                                */
} conv3p_cache_config;

/* Caller's promise for THIS call: `points` holds exactly the bytes it held at the previous *_cached_* call
 * on this cache (e.g. the later layers of a model step, all fed by one points tensor).  The library then
 * skips the content hash and, for a stencil it has already built since the last un-hinted call, the search
 * launches as well.  Without the flag every call re-validates on the device (always safe).  A wrong promise
 * gives results for the previous clouds. */
#define CONV3P_CACHE_POINTS_UNCHANGED 1
/* Which backward kernel serves the dilated narrow layers (9 -> 9 at strides 2-4) depends on the DATA: with short pair
 * lists (surface-sampled objects at N <= 2048: 7-27 neighbours per point) the one that keeps its G matrix for the
 * populated (centre, tap) rows only (37 KiB of LDS instead of 79: four workgroups per CU) is faster (cfg2: -7 % per
 * step); with long ones (S3DIS-like rooms, ~50 neighbours) it is 30 % slower than the dense-G kernel; measured
 * crossover between 27 and 41.  By DEFAULT the library decides on the device: the search leaves, per stencil, a word
 * saying whether the lists it just built are short on average (<= 35 pre-filter hits per point over the batch), the
 * backward launches BOTH kernels and that word lets exactly one of them run -- no host synchronisation, nothing for
 * the caller to know, one empty launch (~5 us) per such backward call.  A caller who knows its data can save that
 * launch with one of the two hints below, valid for the lifetime of the cache (Conv3pStack.tune() measures a sample
 * batch once at set-up and sets one).  Results are the reference's either way (same decisions, tolerance of the op);
 * the two kernels do not give bitwise the same sums, so runs that must reproduce each other bit for bit should fix the
 * choice with a hint or keep the data regime well away from the threshold. */
#define CONV3P_CACHE_SPARSE_NEIGHBOURHOODS 2   /* short lists: the populated-rows kernel alone */
#define CONV3P_CACHE_DENSE_NEIGHBOURHOODS 8    /* long lists: the dense-G kernel alone */
/* conv3p_cache_prepare_f32 only: besides the geometry, also build the two record orders (by forward tap, by backward
 * tap) that the matrix-core path of the wide layers (more than 16 channels on either side, fp32) derives from it -- about
 * 7 % of such a layer's forward+backward.  The next forward / backward on the same points in this cache (called with
 * CONV3P_CACHE_POINTS_UNCHANGED) then finds them in the cache's scratch region; any other use of the cache in between
 * (another stencil's wide layer, a narrow layer) simply rebuilds them.  Needs a cache sized for a wide layer
 * (max_Cin / max_Cout of conv3p_cache_config); CONV3P_ERR_WORKSPACE otherwise.  A performance hint only. */
#define CONV3P_CACHE_PREPARE_DEEP_ORDERS 4
/* conv3p_stack_forward_* / conv3p_stack_backward_* only, OPT-IN: run the hidden layers of a pass as ONE launch with
 * per-cloud barriers between the layers (pointwise_amd/csrc/conv3p_stack_fused.hpp) where the stack, the cache and the
 * device allow it (fp32, in_channels 3 or 9, hidden 9, the whole grid resident at once; the backward also needs
 * CONV3P_CACHE_SPARSE_NEIGHBOURHOODS).  One bit per pass.  Same bits for the activations and grad_input as the per-layer
 * launches; grad_filter sums its partials in another order (tolerance of the op).  Measured (profiles/r06_ab_fused.txt,
 * r06_cfg4_ab.txt): the fused FORWARD is 68 against 86 us on cfg2 and nothing runs beside the forward
 * in a pipelined step, so it is a gain there; the fused BACKWARD holds every slot of the chip while its tiles wait for the
 * slowest tile of their cloud, which keeps the next batch's search out (cfg2: no gain); on the rooms of cfg4, whose tiles
 * differ far more, both lose (1.34 against 1.26 ms).  Hence opt-in; Conv3pStack.tune() sets the forward bit for clouds
 * with short pair lists.  ONE fused launch at a time per device: a waiting tile needs the rest of its cloud resident or
 * dispatchable, and two fused launches issued concurrently (two streams, two processes on one GPU) can hold the slots each
 * other's tiles wait for; every wait is bounded (half a second), a wait that gives up is reported through
 * conv3p_cache_fused_status AND fails the next stack call on that cache with CONV3P_ERR_LAUNCH. */
#define CONV3P_CACHE_FUSED_FORWARD 16
#define CONV3P_CACHE_FUSED_BACKWARD 32
#define CONV3P_CACHE_FUSED_STACK (CONV3P_CACHE_FUSED_FORWARD | CONV3P_CACHE_FUSED_BACKWARD)
/* OPT-IN bf16 precision of the filter contractions of the matrix-core path (fp32 layers with more than 16 channels on a
 * side that have no register-path kernel, including the channel blocks of layers wider than 256) -- torch's
 * set_float32_matmul_precision("medium"): every operand of those contractions (the normalised neighbour sums M_f / G_f',
 * the filter, the X and G rows of the grad_filter product) is rounded once to bf16 (round to nearest even) for
 * v_mfma_f32_32x32x16_bf16, with fp32 accumulation: ~2e-3 relative (max error over max |result|) instead of ~1e-6.
 * The neighbour sums themselves, the grad_filter reduction, the search and the tiles the path hands to the exact generic
 * kernel (non-finite values, pair-buffer overflow) stay fp32.  Without the bit: exact fp32 products, bit for bit the
 * stateless entry points.  Honoured by the *_cached_* forward / backward calls (and conv3p_layer_*) that reach the
 * matrix-core path; ignored, bit for bit, everywhere else: the register-path shapes, fp64, the stateless entry points
 * and the stack entry points.  conv3p_cache_bytes does not depend on it.  (cfg5 shard 128 -> 256, forward + backward:
 * 0.61 x the fp32 time) */
#define CONV3P_CACHE_MATMUL_BF16 64

size_t conv3p_cache_bytes(int elem_bytes, int B, int N, const conv3p_cache_config *cfg);
/* Drop the host-side bookkeeping of a cache buffer (call before freeing it). */
int conv3p_cache_forget(void *cache);
/* Make `cache` (cache_bytes of freshly allocated, possibly RECYCLED device memory) a valid empty cache: zero-fills it on
 * `stream` and drops any host bookkeeping left for that address.  The "zero-filled once" requirement above, as a call:
 * a framework allocator (TensorFlow's BFC) can hand back a region that overlaps a cache freed earlier in the step, whose
 * hashes and slot marks may have survived while its lists were overwritten by temporaries -- content hashes cannot
 * notice that, zero-filling can (integration/tf_conv3p_shim.cc calls this after every allocate_persistent). */
int conv3p_cache_init(void *cache, size_t cache_bytes, void *stream);

int conv3p_forward_cached_f32(const float *points, const float *input, const float *filter,
                              const int32_t *stride_xyz, float voxel_size, int B, int N, int Cin,
                              int Cout, int fz, int fy, int fx, float *output, void *cache,
                              size_t cache_bytes, const conv3p_cache_config *cfg, void *stream);
int conv3p_forward_cached_f64(const double *points, const double *input, const double *filter,
                              const int32_t *stride_xyz, double voxel_size, int B, int N, int Cin,
                              int Cout, int fz, int fy, int fx, double *output, void *cache,
                              size_t cache_bytes, const conv3p_cache_config *cfg, void *stream);
int conv3p_backward_cached_f32(const float *grad_out, const float *points, const float *input,
                               const float *filter, const int32_t *stride_xyz, float voxel_size,
                               int B, int N, int Cin, int Cout, int fz, int fy, int fx,
                               float *grad_input, float *grad_filter, void *cache,
                               size_t cache_bytes, const conv3p_cache_config *cfg, void *stream);
int conv3p_backward_cached_f64(const double *grad_out, const double *points, const double *input,
                               const double *filter, const int32_t *stride_xyz, double voxel_size,
                               int B, int N, int Cin, int Cout, int fz, int fy, int fx,
                               double *grad_input, double *grad_filter, void *cache,
                               size_t cache_bytes, const conv3p_cache_config *cfg, void *stream);

/* Build (or re-validate) the geometry of one stencil without running an op: a later forward / backward
 * with the same points and stencil finds its lists ready.  Lets a caller enqueue the searches of a model's
 * later layers on a second stream while the first layers' accumulation kernels run (the search is
 * VALU-bound, the accumulation gather-latency-bound; they overlap well). */
int conv3p_cache_prepare_f32(const float *points, const int32_t *stride_xyz, float voxel_size, int B,
                             int N, int fz, int fy, int fx, void *cache, size_t cache_bytes,
                             const conv3p_cache_config *cfg, void *stream);
int conv3p_cache_prepare_f64(const double *points, const int32_t *stride_xyz, double voxel_size, int B,
                             int N, int fz, int fy, int fx, void *cache, size_t cache_bytes,
                             const conv3p_cache_config *cfg, void *stream);

/* The same for n_strides stencils that share filter extents, voxel size and points (the layers of the
 * reference's models: strides 1..4, pointcnn2_acsd.py:47-65) with one sort, ONE search launch and ONE
 * normaliser launch: stride_xyz is int32[n_strides][3] on the host, n_strides <= 8 and <= cfg->slots.  A single
 * search launch is one round of workgroups whose duration is set by its slowest tile; batched, the stencils
 * fill each other's tails. */
int conv3p_cache_prepare_multi_f32(const float *points, const int32_t *strides_xyz, int n_strides,
                                   float voxel_size, int B, int N, int fz, int fy, int fx, void *cache,
                                   size_t cache_bytes, const conv3p_cache_config *cfg, void *stream);
int conv3p_cache_prepare_multi_f64(const double *points, const int32_t *strides_xyz, int n_strides,
                                   double voxel_size, int B, int N, int fz, int fy, int fx, void *cache,
                                   size_t cache_bytes, const conv3p_cache_config *cfg, void *stream);

/* Per-point, per-tap neighbour populations, int32 (B, N, fz*fy*fx) on the device.
 * Restates Grid::neighbor_count / kernelBuildNeighborCount
 * (tf_conv3p_atrous.cpp:306-379 / tf_conv3p_atrous.cu:288-343): the intermediate both
 * ops normalise by.  Exported so that neighbour / tap decisions can be checked for
 * exact integer equality against the CPU reference. */
int conv3p_neighbor_count_f32(const float *points, const int32_t *stride_xyz, float voxel_size,
                              int B, int N, int fz, int fy, int fx, int32_t *count,
                              void *workspace, size_t workspace_bytes, void *stream);
int conv3p_neighbor_count_f64(const double *points, const int32_t *stride_xyz, double voxel_size,
                              int B, int N, int fz, int fy, int fx, int32_t *count,
                              void *workspace, size_t workspace_bytes, void *stream);

/* SELU and its derivative, the activation the reference applies after every conv3p
 * (/root/reference/selu.py:22-26; pointcnn2_acsd.py:49-67).  y may alias x.
 * conv3p_selu_grad: dx = dy * selu'(x), expressed through the forward OUTPUT y
 * (selu' = scale for y > 0 [x >= 0 maps to y >= 0], y + scale*alpha otherwise). */
int conv3p_selu_f32(const float *x, float *y, size_t n, void *stream);
int conv3p_selu_grad_f32(const float *y, const float *dy, float *dx, size_t n, void *stream);
int conv3p_selu_f64(const double *x, double *y, size_t n, void *stream);
int conv3p_selu_grad_f64(const double *y, const double *dy, double *dx, size_t n, void *stream);
/* dx = (dy_a + dy_b) * selu'(y): the gradient join where a layer's activation feeds both the
 * next conv3p and the feature concat (pointcnn2_acsd.py:49-69). */
int conv3p_selu_grad_add_f32(const float *y, const float *dy_a, const float *dy_b, float *dx,
                             size_t n, void *stream);
int conv3p_selu_grad_add_f64(const double *y, const double *dy_a, const double *dy_b, double *dx,
                             size_t n, void *stream);

/* The models' layer: conv3p followed by SELU (pointcnn2_acsd.py:48-67:
 *   net = selu(conv3p(points, net, W, stride, voxel))), with the activation fused into the op's kernels.
 * conv3p_layer_forward:   output = selu(Conv3p(points, input, filter, stride, voxel)).
 * conv3p_layer_backward:  for a layer whose `input` is itself the OUTPUT of a SELU (every layer but the
 *   first): grad_filter as Conv3pGrad; grad_input = (dX + grad_addend) * selu'(input), i.e. the gradient
 *   w.r.t. the ARGUMENT of the SELU that produced `input`, where dX is Conv3pGrad's grad_input and
 *   grad_addend (may be NULL) is the gradient arriving at `input` from its other consumer (the feature
 *   concat, pointcnn2_acsd.py:66).  `grad_out` is the gradient w.r.t. this layer's conv3p output (already
 *   through this layer's own SELU).  Results equal the unfused sequence conv3p_*_cached + conv3p_selu* up
 *   to the rounding of one multiply. */
int conv3p_layer_forward_cached_f32(const float *points, const float *input, const float *filter,
                                    const int32_t *stride_xyz, float voxel_size, int B, int N, int Cin,
                                    int Cout, int fz, int fy, int fx, float *output, void *cache,
                                    size_t cache_bytes, const conv3p_cache_config *cfg, void *stream);
int conv3p_layer_forward_cached_f64(const double *points, const double *input, const double *filter,
                                    const int32_t *stride_xyz, double voxel_size, int B, int N, int Cin,
                                    int Cout, int fz, int fy, int fx, double *output, void *cache,
                                    size_t cache_bytes, const conv3p_cache_config *cfg, void *stream);
int conv3p_layer_backward_cached_f32(const float *grad_out, const float *points, const float *input,
                                     const float *filter, const int32_t *stride_xyz, float voxel_size,
                                     int B, int N, int Cin, int Cout, int fz, int fy, int fx,
                                     const float *grad_addend, float *grad_input, float *grad_filter,
                                     void *cache, size_t cache_bytes, const conv3p_cache_config *cfg,
                                     void *stream);
int conv3p_layer_backward_cached_f64(const double *grad_out, const double *points, const double *input,
                                     const double *filter, const int32_t *stride_xyz, double voxel_size,
                                     int B, int N, int Cin, int Cout, int fz, int fy, int fx,
                                     const double *grad_addend, double *grad_input, double *grad_filter,
                                     void *cache, size_t cache_bytes, const conv3p_cache_config *cfg,
                                     void *stream);

/* ---------------------------------------------------------------------------------------------
 * The models' conv3p stack as ONE call per pass (not in the reference, which builds it from op calls in Python:
 * pointcnn2_acsd.py:47-68, scene_seg/pointcnn_scene_seg_acsd.py:51-57).
 *
 *   hidden layer l (l = 0 .. n_hidden-1):  act_l = selu(Conv3p(points, act_{l-1}, filter_l, stride_l, voxel)),
 *       act_{-1} = input (in_channels), every hidden layer has `hidden` output channels;
 *   concat = [act_0 | act_1 | ...]  (B, N, n_hidden*hidden)       -- pointcnn2_acsd.py:68
 *   optional head (num_class > 0):  head = selu(Conv3p(points, concat, filter_head, head_stride, voxel))
 *
 * What the single call buys over 2 x (n_hidden + 1) op calls: one host crossing per pass; the activations are
 * written by the layers' epilogues straight into their column block of `concat` and read from there by the next
 * layer and by the backward (no concat copy, no slice copies); the geometry of all layers is built once per
 * `points` (on `side_stream`, if given, concurrently with the first layers).
 * All layers share the filter extents fz,fy,fx; strides[l] = {sx,sy,sz} of hidden layer l, strides[n_hidden] of the
 * head.  filters / grad_filters are HOST arrays of n_hidden (+1) DEVICE pointers, each tensor laid out as Conv3p's
 * filter.  `cache` as for the *_cached entry points, with slots >= number of distinct strides.
 * Shapes outside the register-resident list return CONV3P_ERR_UNSUPPORTED: compose the stack
 * from the per-op entry points then.  The backward also refuses, before anything is launched, a description whose hidden
 * layers past the first do not fit the register kernels' backward (fp64 9 -> 9 past 28 taps), even where the forward ran.
 * Every layer of a supported description runs on deterministic kernels where its op would.
 * ------------------------------------------------------------------------------------------- */
#define CONV3P_STACK_MAX_LAYERS 8
typedef struct conv3p_stack_desc {
    int n_hidden;      /* hidden layers (4 in both models)                                   */
    int in_channels;   /* channels of `input`                                                */
    int hidden;        /* output channels of every hidden layer (9)                          */
    int num_class;     /* output channels of the head layer, 0 = no head (classification)    */
    int fz, fy, fx;    /* filter extents of every layer                                      */
    int32_t strides[CONV3P_STACK_MAX_LAYERS + 1][3];
} conv3p_stack_desc;

/* bytes of scratch conv3p_stack_backward_* needs (0 for an invalid description) */
size_t conv3p_stack_scratch_bytes(const conv3p_stack_desc *desc, int elem_bytes, int B, int N);

/* Enqueue the geometry (sort + every layer's neighbour search) of `points` into `cache` on `stream`, ordered after
 * everything already enqueued on `after_stream` (the stream that produces `points`; may be NULL).  A later
 * conv3p_stack_forward_* with the same `points` pointer and cache waits for it instead of searching, so the searches
 * of the NEXT batch can run under the current batch's backward.  The caller must not modify `points` in between. */
int conv3p_stack_prefetch_f32(const conv3p_stack_desc *desc, const float *points, float voxel_size, int B, int N,
                              void *cache, size_t cache_bytes, const conv3p_cache_config *cfg, void *stream,
                              void *after_stream);
int conv3p_stack_prefetch_f64(const conv3p_stack_desc *desc, const double *points, double voxel_size, int B, int N,
                              void *cache, size_t cache_bytes, const conv3p_cache_config *cfg, void *stream,
                              void *after_stream);

/* concat (B, N, n_hidden*hidden) receives every hidden activation; head_out (B, N, num_class) or NULL. */
int conv3p_stack_forward_f32(const conv3p_stack_desc *desc, const float *points, const float *input,
                             const float *const *filters, float voxel_size, int B, int N, float *concat,
                             float *head_out, void *cache, size_t cache_bytes, const conv3p_cache_config *cfg,
                             void *stream, void *side_stream);
int conv3p_stack_forward_f64(const conv3p_stack_desc *desc, const double *points, const double *input,
                             const double *const *filters, double voxel_size, int B, int N, double *concat,
                             double *head_out, void *cache, size_t cache_bytes, const conv3p_cache_config *cfg,
                             void *stream, void *side_stream);

/* Backward of the same stack, after conv3p_stack_forward_* on the same cache and points.
 *   grad_concat (B, N, n_hidden*hidden): gradient w.r.t. `concat` from its consumer outside the stack (the dense
 *                head of the classification model); NULL = none.
 *   grad_head   (B, N, num_class): gradient w.r.t. the head activation (num_class > 0).  With a head, grad_concat must
 *                be NULL (neither model of the reference feeds the concat to a second consumer):
 *                CONV3P_ERR_UNSUPPORTED otherwise, before anything is launched.
 *   grad_input  (B, N, in_channels); grad_filters[l] like filters[l] (e.g. views of one fused all-reduce buffer). */
int conv3p_stack_backward_f32(const conv3p_stack_desc *desc, const float *points, const float *input,
                              const float *const *filters, float voxel_size, int B, int N, const float *concat,
                              const float *head_out, const float *grad_concat, const float *grad_head,
                              float *grad_input, float *const *grad_filters, void *scratch, size_t scratch_bytes,
                              void *cache, size_t cache_bytes, const conv3p_cache_config *cfg, void *stream);
int conv3p_stack_backward_f64(const conv3p_stack_desc *desc, const double *points, const double *input,
                              const double *const *filters, double voxel_size, int B, int N, const double *concat,
                              const double *head_out, const double *grad_concat, const double *grad_head,
                              double *grad_input, double *const *grad_filters, void *scratch, size_t scratch_bytes,
                              void *cache, size_t cache_bytes, const conv3p_cache_config *cfg, void *stream);

/* The stack-level passes run the hidden layers as ONE launch per pass where the stack, the cache and the device allow
 * it (pointwise_amd/csrc/conv3p_stack_fused.hpp: per-cloud barriers between the layers).  Diagnostics, SYNCHRONISES the
 * device: how many such launches this cache has seen, and the error bits they left (0 = none; 1: a barrier wait gave up,
 * 2: the tiles of a cloud did not share an XCC).  The reference has no counterpart (one op = one launch sequence there,
 * tf_conv3p_atrous.cu:541-642). */
int conv3p_cache_fused_status(void *cache, unsigned *forward_launches, unsigned *backward_launches, unsigned *error_bits);

/* ---------------------------------------------------------------------------------------------
 * The providers' host pre-step on the device.  The reference prepares every batch with
 * per-cloud numpy loops -- rotate_point_cloud + jitter_point_cloud (/root/reference/modelnet_provider.py:23-75) and
 * sort_point_cloud_xyz / sort_point_cloud_xyz2 (/root/reference/util.py:55-109).  Random numbers stay the caller's.
 *
 * conv3p_augment_f32:  out[b,i,:] = (float)( clip(sigma * noise[b,i,:], +-clip) + (double)(float)(p[b,i,:] . R_b) ),
 *   R_b the rotation about the up (y) axis by the angle whose {cos, sin} is cos_sin[b] (device, double[B][2]; NULL =
 *   no rotation); noise (device, double (B,N,3), e.g. standard normal; NULL = no jitter).  out may alias in.
 * conv3p_sort_xyz_order_f32:  order[b][r] = index of the point that comes r-th in cloud b sorted by x, then y,
 *   then z (what util.py:66-68's three argsorts produce), remaining ties by original index.  data rows have
 *   row_floats floats starting with x, y, z.  N <= 8192 (CONV3P_ERR_UNSUPPORTED beyond).
 * conv3p_sort_morton_order_f32:  the same arguments, status codes and limit; order[b][r] = index of the row that comes
 *   r-th in cloud b by ascending Morton code (sort_method "morton", modelnet_provider.py:100-110 and
 *   :202-208).  The reference computes its code with a third-party library; here the order is DEFINED, per cloud:
 *     1. a row is finite if x, y and z are all finite;
 *     2. lo[a], hi[a] = minimum and maximum of coordinate a over the finite rows, the float values converted to double;
 *     3. e = max_a(hi[a] - lo[a]), subtracted in double;   4. s = 65536.0 / e, one IEEE double division;
 *     5. q[a] = min(65535, floor((double(v[a]) - lo[a]) * s)): one double subtraction, then one double multiplication,
 *        each rounded on its own;                          6. e == 0 (one row, or all finite rows equal): every q = 0;
 *     7. code = the 48-bit interleave, x most significant in every triple: bit 3k+2 of code = bit k of q[x], bit 3k+1 =
 *        bit k of q[y], bit 3k = bit k of q[z], k = 0..15;
 *     8. a row that is not finite is left out of the box and gets code = 2^48 - 1, the code of the far corner cell;
 *     9. ascending code, ties by ascending original index.
 *   Sixteen bits an axis: code << 16 | index is one 64-bit key.  Reproducible bit for bit in numpy (tests/morton_ref.py).
 * conv3p_gather_rows:  dst[b][r] = src[b][order[b][r]] for rows of row_bytes bytes: applies one order to the
 *   points and to every per-point attribute / label array (sort_point_cloud_xyz2).  dst must not alias src.
 * ------------------------------------------------------------------------------------------- */
int conv3p_augment_f32(const float *points_in, const double *cos_sin, const double *noise, double sigma, double clip,
                       int B, int N, float *points_out, void *stream);
int conv3p_sort_xyz_order_f32(const float *data, int B, int N, int row_floats, int32_t *order, void *stream);
int conv3p_sort_morton_order_f32(const float *data, int B, int N, int row_floats, int32_t *order, void *stream);
int conv3p_gather_rows(const void *src, const int32_t *order, int B, int N, int row_bytes, void *dst, void *stream);

/* ---------------------------------------------------------------------------------------------
 * One batch of the reference's data providers as ONE launch (pointwise_amd/csrc/conv3p_provider.hpp): what
 * DataConsumer.get_batch_point_cloud does per batch and load_current_data / next_epoch per file or epoch
 * (modelnet_provider.py:171-219, scene_seg/s3dis_provider.py:80-118, scene_seg/scenenn_provider.py:67-105) with the
 * sort of util.py:55-109, from a data set resident on the device.
 *
 *   data    float (S, Nsrc, K), K >= 3, xyz first; the first N <= Nsrc rows of a sample are used
 *   labels  label_bytes = 1 / 4 / 8 (uint8 / int32 / int64) each; (S) or, labels_per_point != 0, (S, Nsrc).  NULL
 *           together with labels_out: no labels
 *   perm    int32[perm_len] or NULL (identity); cloud b of the batch is sample s = perm[start + b]
 *   flags   CONV3P_PROVIDER_ROTATE | _JITTER | _SORT | _MORTON;  sigma >= 0, clip > 0 (looked at with JITTER).  _MORTON
 *           qualifies _SORT (without it: CONV3P_ERR_INVALID_ARGUMENT): the order of conv3p_sort_morton_order_f32
 *   cos_sin double (B, 2), noise double (B, N, 3): conv3p_augment_f32's, used with ROTATE / JITTER; NULL: drawn with
 *           Philox4x32-10 as a function of (seed, step, s, source row) -- the recipe is in conv3p_provider.hpp
 *
 *   points (B, N, 3); input (B, N, K) = the sample's rows with xyz replaced by the augmented xyz; labels_out int32 (B) or
 *   (B, N).  Optional (NULL: not written): cos_sin_out (B, 2), noise_out (B, N, 3) in source-row order, order_out int32
 *   (B, N): the source row of every output row.  With SORT, rows and per-point labels are in the order of
 *   conv3p_sort_xyz_order_f32 (with MORTON: conv3p_sort_morton_order_f32) applied to the augmented xyz -- the values
 *   written to points; N <= 8192 (CONV3P_ERR_UNSUPPORTED beyond, before any launch).
 *   A sample index outside [0, S) is not read: the cloud's rows are 0, its labels -1, and bad_index[0] (int32, written
 *   by every call that launches) counts such clouds.  B * N == 0: CONV3P_OK, nothing launched, nothing written.
 *   Scratch from conv3p_provider_workspace_bytes (0 without SORT).  Bitwise reproducible; no output depends on a
 *   cloud's position in the batch.
 * ------------------------------------------------------------------------------------------- */
#define CONV3P_PROVIDER_ROTATE 1
#define CONV3P_PROVIDER_JITTER 2
#define CONV3P_PROVIDER_SORT 4
#define CONV3P_PROVIDER_MORTON 8
size_t conv3p_provider_workspace_bytes(int B, int N, int flags);
int conv3p_provider_batch_f32(const float *data, const void *labels, int S, int Nsrc, int K, int label_bytes,
                              int labels_per_point, const int32_t *perm, int64_t perm_len, int64_t start, int B, int N,
                              int flags, double sigma, double clip, uint64_t seed, uint64_t step, const double *cos_sin,
                              const double *noise, float *points, float *input, int32_t *labels_out, double *cos_sin_out,
                              double *noise_out, int32_t *order_out, int32_t *bad_index, void *workspace,
                              size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Both orders for clouds of up to 65536 rows, a cloud spread over many workgroups
 * (pointwise_amd/csrc/conv3p_sort_wide.hpp).  The entry points above keep a cloud's keys in one workgroup's LDS, hence
 * their limit of 8192; these keep them in a workspace and sort them in several launches.  Additions: the entry points
 * above, their limits and their results are what they were.
 *
 * conv3p_sort_order_f32:  method CONV3P_SORT_XYZ: the order of conv3p_sort_xyz_order_f32; CONV3P_SORT_MORTON: the order
 *   of conv3p_sort_morton_order_f32 (the nine steps above) -- both strict total orders, so for N <= 8192 the result is
 *   that of those entry points bit for bit.  1 <= N <= 65536; data, row_floats, order as there.  Status, in this
 *   order: B < 0, N < 0, row_floats < 3 or an unknown method: CONV3P_ERR_INVALID_ARGUMENT; B * N == 0: CONV3P_OK, nothing
 *   launched; data or order NULL: CONV3P_ERR_INVALID_ARGUMENT; N > 65536: CONV3P_ERR_UNSUPPORTED; workspace NULL or
 *   shorter than conv3p_sort_order_workspace_bytes(B, N, method): CONV3P_ERR_WORKSPACE -- all before any launch.
 *   The workspace need not be initialised and nothing is kept in it between calls.
 * conv3p_provider_batch_wide_f32:  conv3p_provider_batch_f32's arguments, meaning, draws and status codes, with two
 *   differences: _SORT is required (CONV3P_ERR_INVALID_ARGUMENT without it) and N <= 65536.  Scratch from
 *   conv3p_provider_wide_workspace_bytes.  Several launches instead of one: the augmented rows into the workspace, the
 *   sort, the gather.  Wherever conv3p_provider_batch_f32 accepts the same call, every output is bit-equal to its.
 * The _bytes functions return a multiple of 256, and 0 for B <= 0, N <= 0, N > 65536, an unknown method, flags
 *   without _SORT.  Bitwise reproducible; a cloud's order does not depend on B or on its place in the batch.
 * ------------------------------------------------------------------------------------------- */
#define CONV3P_SORT_XYZ 0
#define CONV3P_SORT_MORTON 1
size_t conv3p_sort_order_workspace_bytes(int B, int N, int method);
int conv3p_sort_order_f32(const float *data, int B, int N, int row_floats, int method, int32_t *order, void *workspace,
                          size_t workspace_bytes, void *stream);
size_t conv3p_provider_wide_workspace_bytes(int B, int N, int flags);
int conv3p_provider_batch_wide_f32(const float *data, const void *labels, int S, int Nsrc, int K, int label_bytes,
                                   int labels_per_point, const int32_t *perm, int64_t perm_len, int64_t start, int B,
                                   int N, int flags, double sigma, double clip, uint64_t seed, uint64_t step,
                                   const double *cos_sin, const double *noise, float *points, float *input,
                                   int32_t *labels_out, double *cos_sin_out, double *noise_out, int32_t *order_out,
                                   int32_t *bad_index, void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * A room to model-sized blocks and block predictions back to a label per room row
 * (pointwise_amd/csrc/conv3p_scene.hpp).  The segmentation model takes (B, 4096, 9) blocks
 * (scene_seg/s3dis_provider.py:9, :62-63); the partition that made those files is PointNet's
 * room2blocks_plus_normalized (indoor3d_util), which is not in the reference tree, so it is DEFINED here
 * (tests/scene_ref.py restates it in numpy).  One room per call; rows are float32, xyz first, z up.
 *
 * conv3p_scene_blocks_f32:  data (N, K), K >= 3; labels (N) of label_bytes = 1 / 4 / 8 (uint8 / int32 / int64), NULL
 *   together with labels_out: no labels.  P = num_point.
 *    1. A row is finite if x, y and z are finite.  Other rows belong to no cell and are counted in stats[4].
 *    2. lo[a] = minimum of coordinate a over the finite rows; s[a] = v[a] - lo[a], one float32 subtraction, a = x, y,
 *       z; lim[a] = maximum of s[a] over the finite rows.
 *    3. nbx = max(1, (int)ceil((double(lim_x) - double(block)) / double(stride)) + 1), nby alike (PointNet's count with
 *       a floor of one; each held at 2^30).  With no finite row nbx = nby = 0.
 *    4. Cell (i, j) has id c = i * nby + j, edges xbeg = float(i) * stride (one float32 product), xend = xbeg + block
 *       (one float32 sum), y alike.  A finite row is a member iff xbeg <= s_x <= xend and ybeg <= s_y <= yend: both
 *       ends inclusive, so a row on an edge, or under overlapping strides, belongs to several cells.
 *    5. count[c] = number of members.  A cell is kept iff count[c] >= max(1, min_points).  Kept cells get block numbers
 *       in ascending c; blocks numbered >= max_blocks are not emitted.
 *    6. A cell's member list is in ascending room row.
 *    7. Block b of cell c, n = count[c], has P slots.  Slot t takes member t when n <= P and t < n.  Every other slot
 *       (every slot when n > P) is a draw, with replacement as PointNet's sample_data:
 *       w = philox4x32_10(counter (t, 0x80000000 | c, step low, step high), key (seed low, seed high)).w[0],
 *       member (uint64(w) * n) >> 32.  The counter's second word is disjoint from the provider's and the dropout's.
 *    8. index_out[b][t] = the slot's room row; labels_out = that row's label cast to int32.  With bmin_x, bmin_y the
 *       minima of s_x, s_y over the block's P emitted rows and h = block * 0.5f, the output row is
 *       {s_x - (bmin_x + h), s_y - (bmin_y + h), s_z, channels 3..K-1 copied, s_x / lim_x, s_y / lim_y, s_z / lim_z},
 *       each operation a single float32 one; a division by lim == 0 gives 0.
 *    9. Blocks nb..max_blocks-1 (nb = emitted blocks) get data 0, labels -1, index -1, block_cell -1, block_count 0:
 *       both heads and the vote ignore them.  block_cell[b] = c and block_count[b] = n otherwise.
 *   10. stats = {emitted blocks, kept cells, nbx, nby, non-finite rows, cells with 0 < count < min_points, 0, error}.
 *       nbx * nby > CONV3P_SCENE_MAX_CELLS: nothing is emitted (all blocks are step 9's) and stats[7] = 1 -- known
 *       on the device only, so not a status code.
 *   Status, in this order, all before any launch: N < 0, K < 3, num_point < 1, max_blocks < 0, block or stride not
 *   finite or <= 0, labels given without labels_out or the reverse, labels with label_bytes not 1 / 4 / 8:
 *   CONV3P_ERR_INVALID_ARGUMENT; N == 0 or max_blocks == 0: CONV3P_OK, nothing launched, nothing written; data,
 *   blocks_out, index_out, block_cell, block_count or stats NULL: CONV3P_ERR_INVALID_ARGUMENT; N > 2^24, num_point >
 *   65536, K > 65536 or block outside [stride, 2 stride]: CONV3P_ERR_UNSUPPORTED; workspace NULL, misaligned or shorter
 *   than conv3p_scene_blocks_workspace_bytes: CONV3P_ERR_WORKSPACE.  That size is a host-side upper bound from its five
 *   arguments (the cell counts, and member lists of at most N * (ceil(block / stride) + 1)^2 entries), a multiple of
 *   256, 0 for arguments the call refuses or does nothing for; never a data-dependent failure.  The workspace need not
 *   be initialised and nothing is kept in it between calls.  Seven launches; no float atomics; every output word is
 *   written once by a plain store; bitwise reproducible.
 *
 * conv3p_scene_vote:  every row r with 0 <= index[r] < N and 0 <= pred[r] < num_class adds 1 to
 *   votes[index[r]][pred[r]] (int32 (N, num_class), ACCUMULATED into: the caller zeroes it, so several passes -- other
 *   steps, overlapping strides -- add up).  Each emitted row votes, so a room row drawn twice votes twice.  Integer
 *   atomics: exact.  Status: N < 0 or num_class < 1: CONV3P_ERR_INVALID_ARGUMENT; rows == 0 or N == 0: CONV3P_OK,
 *   nothing launched; a NULL pointer: CONV3P_ERR_INVALID_ARGUMENT; N > 2^31 - 1: CONV3P_ERR_UNSUPPORTED.
 * conv3p_scene_vote_labels:  label_out[i] = the class with the most votes of room row i, the lowest class on a tie, -1
 *   for a row without votes; stats = int64 {voted rows, unvoted rows}.  Status as above (N == 0: CONV3P_OK, nothing
 *   written), then CONV3P_ERR_WORKSPACE against conv3p_scene_vote_labels_workspace_bytes.  Two launches.
 *
 * conv3p_scene_blocks_cover_f32:  the COVERING mode of the partition, for evaluation: a crowded cell is not sampled but
 *   split, so every finite row of a kept cell is emitted (pointwise_amd/csrc/conv3p_scene_cover.hpp;
 *   tests/scene_cover_ref.py restates it).  The argument list, the statuses and their order are
 *   conv3p_scene_blocks_f32's, the workspace size is conv3p_scene_blocks_cover_workspace_bytes (the same five arguments,
 *   the same properties).  Steps 1-4, 6, 8 and 9 are as above; the others:
 *    5'. A kept cell c with n = count[c] members gives q = ceil(n / P) blocks, its parts j = 0..q-1 (q = 1 when
 *        n <= P).  Blocks are numbered in ascending (c, j); blocks numbered >= max_blocks are not emitted, so a cell
 *        may be cut between two parts.
 *    7'. Part j holds the members of rank [a_j, a_{j+1}) of the cell's ascending list, a_j = floor(j * n / q) in 64-bit
 *        integers; so n_j = a_{j+1} - a_j <= P, and n_j >= floor(P / 2) whenever q > 1.  Slot t < n_j takes member
 *        a_j + t.  Every other slot is a draw among the part's own members: member a_j + ((uint64(w) * n_j) >> 32),
 *        w = philox4x32_10(counter (j * P + t, 0x80000000 | c, step low, step high), key (seed low, seed high)).w[0];
 *        j * P + t < 2^25.  For j = 0 this is step 7's counter: a cell with n <= P comes out bit for bit as in the
 *        plain mode.
 *    9'. block_cell[b] = c and block_count[b] = n_j: the first block_count[b] slots of a block are distinct members,
 *        the rest are draws; the parts of a cell are consecutive blocks with equal block_cell.
 *   10'. stats[6] = the blocks the room needs (the sum of q over the kept cells); stats[0] < stats[6] tells that
 *        max_blocks cut the room.  The other words keep their meaning (the plain call writes stats[6] = 0).
 *   When nothing is cut, the slots t < block_count[b] over the blocks of a cell are the cell's member list, each row
 *   exactly once, in ascending order.  Eight launches; no float atomics; every output word is written once by a plain
 *   store; bitwise reproducible.
 *
 * conv3p_scene_vote_scores_f32:  votes by summed class probabilities.  logits (rows, num_class) float32, the model's
 *   last activations.  A row r votes iff 0 <= index[r] < N and all its num_class logits are finite; it computes, each
 *   step a single float32 operation and the sum in ascending class, m = max_c x_c, e_c = expf(x_c - m), S = sum_c e_c,
 *   p_c = e_c / S, v_c = llrintf(p_c * 2^30), and adds v_c to scores[index[r]][c] (int64 (N, num_class), ACCUMULATED
 *   into: the caller zeroes it) with a 64-bit integer atomic: fixed point, so exact and independent of the order of
 *   the rows and of the launch geometry.  stats (int64 (2)) is accumulated into as well: stats[0] += rows that voted,
 *   stats[1] += rows with a valid index and a non-finite logit.  Status: N < 0 or num_class < 1:
 *   CONV3P_ERR_INVALID_ARGUMENT; rows == 0 or N == 0: CONV3P_OK, nothing launched; a NULL pointer:
 *   CONV3P_ERR_INVALID_ARGUMENT; N > 2^31 - 1 or num_class > 128: CONV3P_ERR_UNSUPPORTED.  One launch.
 * conv3p_scene_score_labels:  label_out[i] = the class with the largest score of room row i, the lowest class on a
 *   tie, -1 where all scores are 0; stats = int64 {voted rows, unvoted rows}.  Status as conv3p_scene_vote_labels
 *   (num_class > 128: CONV3P_ERR_UNSUPPORTED), then CONV3P_ERR_WORKSPACE against
 *   conv3p_scene_score_labels_workspace_bytes.  Two launches.
 *
 * conv3p_scene_blocks_rooms_f32:  MANY ROOMS in one call (pointwise_amd/csrc/conv3p_scene_rooms.hpp;
 *   tests/scene_rooms_ref.py restates it on the single-room references).  data (N, K) holds the rooms' rows one room
 *   after the other; room_start, int32 (R + 1) ON THE DEVICE, gives room r the rows [room_start[r], room_start[r+1]).
 *   Rows before room_start[0] or from room_start[R] on belong to no room.  cover = 0 / 1 selects the plain or the
 *   covering mode.  The result is the concatenation of the single-room calls:
 *    a. Room r is tiled as by conv3p_scene_blocks_f32 (cover = 0) or conv3p_scene_blocks_cover_f32 (cover = 1) run on
 *       the room's own rows with the same num_point, block, stride, min_points and step, and the Philox key
 *       (seed + r) mod 2^64.  Every step above holds per room; lo, lim, nbx, nby are the room's own.  The minimum of
 *       step 2 takes -0.0 as below +0.0 (IEEE 754-2019 minimum, the device's min instruction), in this call as in the
 *       single-room ones, so lo does not depend on the order of the reduction.
 *    b. Blocks are numbered room after room, within a room as the single call numbers them; first_r = the blocks the
 *       rooms before r need (kept cells; covering: parts).  Blocks numbered >= max_blocks are not emitted: room r
 *       behaves as its single call with max_blocks_r = max(0, max_blocks - first_r).  Blocks past the emitted ones get
 *       step 9's filler and block_room -1.
 *    c. index_out holds the GLOBAL row, room_start[r] + the room row; labels is (N), indexed by global row.  block_cell
 *       is the cell id within the room, block_room (max_blocks) the room.
 *    d. room_blocks int32 (R + 1): the prefix of the emitted blocks per room, room_blocks[R] = stats[0].
 *       room_stats int32 (R, 8): the eight words the single call would write for room r with max_blocks_r -- words 1-7
 *       also when max_blocks_r = 0 (word 0 is then 0); an empty room gives eight zeros.
 *       stats int32 (8) = {emitted blocks, kept cells over all rooms, R, total cells (the sum of nbx nby over the rooms
 *       without an error of their own, held at 2^31 - 1), non-finite rows, small cells, the blocks all rooms need
 *       (covering; 0 plain), error bits}.
 *    e. Errors known on the device only, stats[7]:  bit 0: some room's own tiling has more than CONV3P_SCENE_MAX_CELLS
 *       cells; that room emits nothing and has room_stats[r][7] = 1, the others are unaffected.  bit 1: room_start is
 *       malformed (room_start[0] < 0, a decrease, room_start[R] > N, a room of more than 2^24 rows): nothing is read
 *       through it, nothing is emitted, room_blocks and room_stats are all 0.  bit 2: more than
 *       CONV3P_SCENE_ROOMS_MAX_CELLS cells summed over the rooms without an error of their own: nothing is emitted,
 *       room_blocks is all 0, room_stats keeps words 2, 3, 4 and 7 and has 0 elsewhere.  bit 3: the rows have more
 *       member pairs than N (ceil(block / stride) + 1)^2, which the comparisons of step 4 do not allow -- an internal
 *       error, reported rather than hidden: the pairs past the bound are dropped and the result is not to be used.
 *   Status, in the single call's order: N < 0, R < 0, K < 3, num_point < 1, max_blocks < 0, cover not 0 / 1, block or
 *   stride not finite or <= 0, labels without labels_out or the reverse, label_bytes not 1 / 4 / 8:
 *   CONV3P_ERR_INVALID_ARGUMENT; R == 0, N == 0 or max_blocks == 0: CONV3P_OK, nothing launched, nothing written; a
 *   NULL data, room_start or output: CONV3P_ERR_INVALID_ARGUMENT; N > 2^26 (the member pairs, at most 9 a row, stay
 *   inside 31 bits), R > 65536, num_point > 65536, K > 65536 or block outside [stride, 2 stride]:
 *   CONV3P_ERR_UNSUPPORTED; then CONV3P_ERR_WORKSPACE against conv3p_scene_blocks_rooms_workspace_bytes, a host-side
 *   bound from its arguments (dominated by two buffers of N (ceil(block / stride) + 1)^2 pairs of 8 bytes: up to 144
 *   bytes a row), a multiple of 256, 0 for arguments the call refuses or does nothing for; never a data-dependent
 *   failure.  The workspace need not be initialised and nothing is kept in it.  The member lists are built by a stable
 *   radix sort of (cell, row) pairs: work proportional to the pairs, not to cells x rows, and no limit on a list's
 *   length.  21 launches whatever R, the cells and the blocks; no float atomics; every output word is written once by a
 *   plain store; bitwise reproducible and independent of the launch geometry.
 * ------------------------------------------------------------------------------------------- */
#define CONV3P_SCENE_MAX_CELLS 65536
size_t conv3p_scene_blocks_workspace_bytes(int64_t N, int num_point, int max_blocks, float block, float stride);
int conv3p_scene_blocks_f32(const float *data, const void *labels, int64_t N, int K, int label_bytes, float block,
                            float stride, int num_point, int min_points, int max_blocks, uint64_t seed, uint64_t step,
                            float *blocks_out, int32_t *labels_out, int32_t *index_out, int32_t *block_cell,
                            int32_t *block_count, int32_t *stats, void *workspace, size_t workspace_bytes, void *stream);
int conv3p_scene_vote(const int32_t *pred, const int32_t *index, size_t rows, int64_t N, int num_class, int32_t *votes,
                      void *stream);
size_t conv3p_scene_vote_labels_workspace_bytes(int64_t N, int num_class);
int conv3p_scene_vote_labels(const int32_t *votes, int64_t N, int num_class, int32_t *label_out, int64_t *stats,
                             void *workspace, size_t workspace_bytes, void *stream);
size_t conv3p_scene_blocks_cover_workspace_bytes(int64_t N, int num_point, int max_blocks, float block, float stride);
int conv3p_scene_blocks_cover_f32(const float *data, const void *labels, int64_t N, int K, int label_bytes, float block,
                                  float stride, int num_point, int min_points, int max_blocks, uint64_t seed,
                                  uint64_t step, float *blocks_out, int32_t *labels_out, int32_t *index_out,
                                  int32_t *block_cell, int32_t *block_count, int32_t *stats, void *workspace,
                                  size_t workspace_bytes, void *stream);
#define CONV3P_SCENE_ROOMS_MAX_CELLS 1048576
size_t conv3p_scene_blocks_rooms_workspace_bytes(int64_t N, int64_t R, int num_point, int max_blocks, float block,
                                                 float stride, int cover);
int conv3p_scene_blocks_rooms_f32(const float *data, const void *labels, const int32_t *room_start, int64_t N, int64_t R,
                                  int K, int label_bytes, float block, float stride, int num_point, int min_points,
                                  int max_blocks, int cover, uint64_t seed, uint64_t step, float *blocks_out,
                                  int32_t *labels_out, int32_t *index_out, int32_t *block_cell, int32_t *block_count,
                                  int32_t *block_room, int32_t *room_blocks, int32_t *room_stats, int32_t *stats,
                                  void *workspace, size_t workspace_bytes, void *stream);
int conv3p_scene_vote_scores_f32(const float *logits, const int32_t *index, size_t rows, int64_t N, int num_class,
                                 int64_t *scores, int64_t *stats, void *stream);
size_t conv3p_scene_score_labels_workspace_bytes(int64_t N, int num_class);
int conv3p_scene_score_labels(const int64_t *scores, int64_t N, int num_class, int32_t *label_out, int64_t *stats,
                              void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Voxel-grid subsampling of a cloud, and voxel labels projected back to its rows
 * (pointwise_amd/csrc/conv3p_grid.hpp; tests/grid_ref.py restates it in numpy).  The step in front of the scene calls:
 * a raw room or scan is thinned to one row per occupied voxel, the model runs on those rows, and every raw row gets its
 * voxel's prediction.  One cloud per call, or many with a room_start; rows are float32, xyz first.  Additions: nothing
 * above changes.
 *
 * conv3p_grid_subsample_f32:  data (N, K), K >= 3; labels (N) of label_bytes = 1 / 4 / 8 (uint8 / int32 / int64), NULL
 *   together with labels_out: no labels.  voxel is the lattice step, mode 0 the mean, mode 1 the centre.
 *    1. A row is finite iff x, y and z are finite.  Other rows belong to no voxel and are counted in stats[5].
 *    2. lo[a] = minimum of coordinate a over the finite rows, -0.0 taken as below +0.0 (IEEE 754-2019 minimum, the
 *       device's min instruction, as in conv3p_scene_blocks_rooms_f32), so lo does not depend on the order of the
 *       reduction; s[a] = v[a] - lo[a], one float32 subtraction, a = x, y, z.
 *    3. i_a = (int)floorf(s_a / voxel), one correctly rounded float32 division, the quotient held at 2^30 (an
 *       overflowed s is +inf).  n_a = 1 + the largest i_a over the finite rows; n_a = 0 without a finite row.
 *    4. The row's cell is (i_x, i_y, i_z), its id c = (i_x n_y + i_y) n_z + i_z in 64-bit integers.
 *    5. Voxels are the occupied cells, numbered in ascending c, that is, ascending (i_x, i_y, i_z).  Voxels numbered
 *       >= max_voxels are not emitted.
 *    6. A voxel's member list is in ascending row.
 *    7. mode 0 (mean), n = the members m_0 < m_1 < ...:  out[v][k] = (((x_k[m_0] + x_k[m_1]) + ...) ) / float(n) for
 *       every channel k of the K, on the ORIGINAL values (xyz not shifted), each step a single float32 operation in
 *       list order (n = 1: x / 1.0f).  voxel_row[v] = m_0.  labels_out[v] = the class with the most members among
 *       those whose label l has 0 <= l < num_class (compared in the label's own width), the lowest class on a tie,
 *       -1 with no such member.
 *    8. mode 1 (centre):  the representative is the member that minimises d = ((s_x - c_x)^2 + (s_y - c_y)^2) +
 *       (s_z - c_z)^2 with c_a = (float(i_a) + 0.5f) * voxel, every operation a single float32 one, uncontracted, in
 *       that order; the lowest row on a tie.  out[v] = that row copied, voxel_row[v] = that row, labels_out[v] = its
 *       label cast to int32.  num_class is not read.
 *   Outputs: out float32 (max_voxels, K); labels_out int32 (max_voxels); voxel_row, voxel_count int32 (max_voxels),
 *   the members per voxel; voxel_cell int32 (max_voxels, 3) = (i_x, i_y, i_z); inverse int32 (N), the voxel number of
 *   every row, -1 for a non-finite row and for a row of a voxel that is not emitted; stats int32 (8) = {emitted
 *   voxels, occupied voxels, n_x, n_y, n_z, non-finite rows, the largest member count over the occupied voxels,
 *   error}.  Voxels nv..max_voxels-1 (nv = emitted voxels) get data 0, label -1, row -1, count 0, cell -1.
 *   The error known on the device only: some n_a > 2^20, or n_x n_y n_z > 2^40 (a cell id has 40 bits of a sorted
 *   pair): stats = {0, 0, n_x, n_y, n_z, non-finite rows, 0, 1}, nothing is emitted, inverse is all -1.
 *   Status, in this order, all before any launch: N < 0, K < 3, max_voxels < 0, mode not 0 / 1, voxel not finite or
 *   <= 0, labels given without labels_out or the reverse, labels with label_bytes not 1 / 4 / 8, num_class < 1 where it
 *   is read (mode 0 with labels): CONV3P_ERR_INVALID_ARGUMENT; N == 0 or max_voxels == 0: CONV3P_OK, nothing launched,
 *   nothing written; data, out, voxel_row, voxel_count, voxel_cell, inverse or stats NULL: CONV3P_ERR_INVALID_ARGUMENT;
 *   N > 2^24 (a row has 24 bits of a sorted pair), K > 65536, or num_class > 128 where it is read:
 *   CONV3P_ERR_UNSUPPORTED; workspace NULL, misaligned or shorter than conv3p_grid_subsample_workspace_bytes(N,
 *   max_voxels): CONV3P_ERR_WORKSPACE.  That size is a host-side bound from its two arguments (two buffers of N pairs of
 *   8 bytes and N + 1 list starts dominate: about 21 bytes a row), monotone in N, a multiple of 256, 0 for N <= 0, N >
 *   2^24 or max_voxels <= 0; never a data-dependent failure.  The workspace need not be initialised and nothing is kept
 *   in it.  The member lists come from a stable radix sort of (cell, row) pairs, 8 bits a pass: 24 launches in mode 0,
 *   23 in mode 1, whatever the data (a pass over digits above the top bit of cells - 1 returns at once, by a word the
 *   device wrote); no float atomics; every output word is written once by a plain store; bitwise reproducible and
 *   independent of the launch geometry.
 *
 * conv3p_grid_project_labels:  out[i] = voxel_labels[inverse[i]] where 0 <= inverse[i] < M, otherwise -1; voxel_labels
 *   int32 (M), inverse and out int32 (N).  Status: N < 0 or M < 0: CONV3P_ERR_INVALID_ARGUMENT; N == 0: CONV3P_OK,
 *   nothing launched; inverse or out NULL, or voxel_labels NULL with M > 0: CONV3P_ERR_INVALID_ARGUMENT; N or M > 2^31 -
 *   1: CONV3P_ERR_UNSUPPORTED.  One launch.
 *
 * conv3p_grid_subsample_rooms_f32:  MANY CLOUDS in one call (pointwise_amd/csrc/conv3p_grid_rooms.hpp;
 *   tests/grid_rooms_ref.py restates it on the single-cloud reference).  data (N, K) holds the rooms' rows one room
 *   after the other; room_start, int32 (R + 1) ON THE DEVICE, gives room r the rows [room_start[r], room_start[r+1]).
 *   Rows before room_start[0] or from room_start[R] on belong to no room: their inverse is -1 and they are counted
 *   nowhere.  The result is the concatenation of the single-cloud calls:
 *    a. Room r is subsampled exactly as by conv3p_grid_subsample_f32 run on the room's own rows with the same voxel,
 *       mode and num_class.  Steps 1-8 hold per room; lo, n_x, n_y, n_z and the cell ids are the room's own, so two
 *       rooms that overlap in space never share a voxel.
 *    b. Voxels are numbered room after room, within a room in ascending cell id; first_r = the occupied voxels of the
 *       rooms before r.  Voxels numbered >= max_voxels are not emitted: room r behaves as its single call with
 *       max_voxels_r = max(0, max_voxels - first_r).  Voxels past the emitted ones get the single call's filler and
 *       voxel_room -1.
 *    c. inverse (N) holds the GLOBAL voxel number, voxel_row the GLOBAL row; labels is (N), indexed by global row.
 *       voxel_cell is (i_x, i_y, i_z) in the room's own lattice, voxel_room (max_voxels) the room of each voxel.
 *    d. voxel_start int32 (R + 1): the prefix of the emitted voxels per room, voxel_start[R] = stats[0] -- unchanged and
 *       still on the device, the room_start of conv3p_scene_blocks_rooms_f32 over the rows of out.
 *       room_stats int32 (R, 8): the eight words the single call would write for room r with max_voxels_r -- words 1-7
 *       also when max_voxels_r = 0 (word 0 is then 0); word 6, the largest member count, is taken over the room's
 *       occupied voxels as in the single call; an empty room gives eight zeros.
 *       stats int32 (8) = {emitted voxels, occupied voxels over all rooms without an error of their own, R, rooms with
 *       at least one emitted voxel, rooms with an error of their own, non-finite rows inside the rooms, the largest
 *       member count over all rooms, error bits}.
 *    e. Errors known on the device only, stats[7]:  bit 0: some room's own lattice has an n_a > 2^20 or more than 2^40
 *       cells; that room emits nothing, its room_stats[r] is {0, 0, n_x, n_y, n_z, non-finite rows, 0, 1} and its rows
 *       have inverse -1; every other room is unaffected.  bit 1: room_start is malformed (room_start[0] < 0, a
 *       decrease, room_start[R] > N): nothing is read through it, nothing is emitted, inverse is all -1, voxel_start
 *       and room_stats are all 0 (so stats = {0, 0, R, 0, 0, 0, 0, 2}).  bit 2: the cells, summed over the rooms
 *       without an error of their own, exceed 2^40 -- a global cell id is cell_base[r] + c, cell_base the 64-bit prefix
 *       of the rooms' cell counts, and must fit the 40 bits of a sorted pair: nothing is emitted, voxel_start is all 0,
 *       inverse is all -1, room_stats keeps words 2, 3, 4, 5 and 7 and has 0 elsewhere.
 *   Status, in this order, all before any launch: N < 0, R < 0, K < 3, max_voxels < 0, mode not 0 / 1, voxel not finite
 *   or <= 0, labels given without labels_out or the reverse, labels with label_bytes not 1 / 4 / 8, num_class < 1 where
 *   it is read (mode 0 with labels): CONV3P_ERR_INVALID_ARGUMENT; R == 0, N == 0 or max_voxels == 0: CONV3P_OK, nothing
 *   launched, nothing written; a NULL data, room_start or output (labels_out apart): CONV3P_ERR_INVALID_ARGUMENT;
 *   N > 2^24 summed over all rooms (a GLOBAL row keeps the 24 bits of a sorted pair), R > 65536, K > 65536, or
 *   num_class > 128 where it is read: CONV3P_ERR_UNSUPPORTED; then CONV3P_ERR_WORKSPACE against
 *   conv3p_grid_subsample_rooms_workspace_bytes(N, R, max_voxels), a host-side bound from its three arguments (the
 *   single call's, plus 32 bytes of a bounds record, a frame of 48 bytes and two prefix words per room), monotone in N
 *   and R, a multiple of 256, 0 for arguments the call refuses or does nothing for; never a data-dependent failure.
 *   The workspace need not be initialised and nothing is kept in it.  One stable radix sort orders all rooms' (global
 *   cell, global row) pairs, by the single call's sort, heads and mean kernels: 28 launches in mode 0, 27 in mode 1,
 *   fixed by mode alone whatever R, the rooms' sizes and the data; no float atomics; every output word is written once
 *   by a plain store; bitwise reproducible and independent of the launch geometry.
 *
 * conv3p_grid_neighbors, conv3p_grid_interpolate_f32 / _i64:  voxel SCORES interpolated onto every raw row from the
 *   nearest voxels of the 3 x 3 x 3 cells around its own, with inverse-distance weights
 *   (pointwise_amd/csrc/conv3p_grid_interp.hpp; tests/grid_interp_ref.py restates it in numpy).  conv3p_grid_project_labels
 *   gives a row the label of its own voxel and of no other: a voxel nobody voted for leaves its rows at -1, and class
 *   boundaries follow the lattice.  This is the other ending, for the single-cloud and the many-clouds result alike.
 *
 *   The neighbour table, neigh int32 (max_voxels, 27), from voxel_cell (max_voxels, 3) and the subsampling's stats:
 *    N1. nv = stats[0], the emitted voxels, read ON THE DEVICE (held to [0, max_voxels]); there is no host read.
 *    N2. For an emitted voxel v with cell (i, j, l) and t = (dx+1)*9 + (dy+1)*3 + (dz+1), dx, dy, dz in {-1, 0, 1}:
 *        neigh[v][t] = the number of the emitted voxel whose cell is (i+dx, j+dy, l+dz), -1 if there is none (the cell
 *        is not occupied, lies outside the lattice, or its voxel was cut by max_voxels).  neigh[v][13] = v.
 *    N3. Rows nv..max_voxels-1 are all -1.
 *    N4. With voxel_room (max_voxels) and voxel_start (num_rooms + 1) of conv3p_grid_subsample_rooms_f32 -- both or
 *        neither -- only voxels of the same room are neighbours: cells are compared in the room's own lattice and the
 *        search runs over [voxel_start[r], voxel_start[r+1]), r = voxel_room[v].  Rooms that overlap in space share
 *        nothing.
 *   Status: max_voxels < 0, num_rooms < 0, one of voxel_room / voxel_start without the other:
 *   CONV3P_ERR_INVALID_ARGUMENT; max_voxels == 0: CONV3P_OK, nothing launched; voxel_cell, grid_stats or neigh NULL:
 *   CONV3P_ERR_INVALID_ARGUMENT; num_rooms > 65536: CONV3P_ERR_UNSUPPORTED.  One launch: a lane per (voxel, (dx, dy)),
 *   one binary search for (i+dx, j+dy, l-1) in the ascending cells, then up to three consecutive entries.
 *
 *   The interpolation.  data (N, K) is the raw cloud the subsampling was given, inverse (N) its voxel per row;
 *   voxel_data (>= M, voxel_K) the voxels' rows (xyz first: the mean, or the centre member), neigh (>= M, 27);
 *   voxel_scores (M, C), float32 or the int64 fixed-point sums of conv3p_scene_vote_scores_f32; valid_labels int32 (M) or
 *   NULL; 1 <= k <= 8; 1 <= C <= 128.  Per raw row i, with p = data[i][0..2] and v0 = inverse[i]:
 *    1. v0 < 0 or v0 >= M: label -1, score row all 0; counted in stats[1] ("no voxel").
 *    2. The candidates are the u = neigh[v0][t] with u >= 0, u < M and, with valid_labels, valid_labels[u] >= 0.
 *       q = voxel_data[u][0..2]; d2 = ((p_x-q_x)^2 + (p_y-q_y)^2) + (p_z-q_z)^2, every operation a single float32 one,
 *       uncontracted, in that order.  A candidate whose d2 is NaN or inf is dropped.
 *    3. The min(k, candidates) smallest by the total order (d2, u) are kept, ranked j = 0, 1, ... in that order.
 *    4. None left: label -1, score row 0; counted in stats[2] ("no candidate").
 *    5. Otherwise, counted in stats[0]:  w_j = 1.0f / fmaxf(d2_j, 1e-10f), a correctly rounded division;
 *       W = ((w_0 + w_1) + w_2) + ...; for every class c:  out[c] = (((w_0 s_0c + w_1 s_1c) + w_2 s_2c) + ...) / W,
 *       products and sums rounded separately.  s_jc = voxel_scores[u_j][c] (_f32), or (float)voxel_scores[u_j][c] *
 *       2^-30 (_i64: the conversion rounds to nearest even, the scaling is exact).  The label is class 0 unless a later
 *       class is strictly greater than the best so far: the lowest class wins a tie and a NaN never wins.
 *   Scores are NOT normalised per voxel: a voxel that overlapping blocks voted for twice weighs twice, as it does in
 *   conv3p_scene_score_labels.  out_labels int32 (N); out_scores float32 (N, C) or NULL; stats int64 (3) = {rows
 *   interpolated, rows without a voxel, rows without a candidate}, exact, overwritten by every call.
 *   Status, in this order, all before any launch: N < 0, M < 0, K < 3, voxel_K < 3, C outside [1, 128], k outside [1, 8]:
 *   CONV3P_ERR_INVALID_ARGUMENT; stats NULL; data, inverse or out_labels NULL with N > 0; voxel_data, neigh or voxel_scores
 *   NULL with N > 0 and M > 0: CONV3P_ERR_INVALID_ARGUMENT; N or M > 2^31 - 1: CONV3P_ERR_UNSUPPORTED.  N == 0 and M == 0
 *   are valid: with M == 0 every row has "no voxel".  One kernel launch behind a 24-byte memset of stats; 16 lanes a row;
 *   the only atomics are the integer adds of the three counts; no float atomics; bitwise reproducible and independent of
 *   the launch geometry.
 *
 * conv3p_grid_interpolate_rings_f32 / _i64:  the same, and a row that rule 4 leaves without a candidate searches ring
 *   after ring of cells around its own (pointwise_amd/csrc/conv3p_grid_interp_rings.hpp; tests/grid_interp_rings_ref.py
 *   restates it in numpy).  rings in [1, 8] is the largest Chebyshev distance, in cells, between the row's own cell and a
 *   candidate's: the cube of rings = 8 is 17^3 cells, 32 cm at a 4 cm voxel.  voxel_cell (>= M, 3), voxel_room (>= M) and
 *   voxel_start (num_rooms + 1) -- both or neither -- and grid_stats are the subsampling's; ne = min(max(grid_stats[0], 0),
 *   M) is read ON THE DEVICE.  For a raw row i with v0 = inverse[i] in [0, M) and (a, b, l) = voxel_cell[v0]:
 *    6. Rules 1-5 apply unchanged.  A row that rule 5 interpolates has ring = 1; its label and score row are what the plain
 *       call writes, to the bit, whatever rings is.
 *    7. A row that rule 4 would leave without a candidate takes r = 2, 3, ..., rings in turn.  The candidates of ring r are
 *       the emitted voxels u with u < ne; with voxel_room / voxel_start, u in [voxel_start[p], voxel_start[p+1]), p =
 *       voxel_room[v0], clamped as N4 clamps it (rooms that overlap in space share nothing; v0 >= ne has no candidates,
 *       as its row of neigh has none); max(|i_x(u) - a|, |i_y(u) - b|, |i_z(u) - l|) <= r; valid_labels[u] >= 0 where
 *       valid_labels is given; the d2 of rule 2 finite (the same operations in the same order, uncontracted).  The first r
 *       whose candidate set is not empty ends the search: rules 3 and 5 are applied to that set as they stand -- the min(k,
 *       candidates) smallest by the total order (d2, u), the chains in rank order, the same label rule -- and ring = r.
 *    8. No ring up to rings has a candidate: label -1, score row 0, ring = 0, counted in stats[2].  A row of rule 1 (no
 *       voxel) has ring = 0 too.
 *    9. out_ring int32 (N) or NULL; stats int64 (3) = {rows interpolated at any ring, rows without a voxel, rows without
 *       a candidate within rings}; ring_stats int64 (9): ring_stats[r], r = 1 .. 8, the rows interpolated at ring r,
 *       ring_stats[0] the rows that entered the fallback (no candidate in their 27 cells).  All exact, overwritten by
 *       every call.
 *   This is NOT a k-nearest-neighbour search.  The search stops at the first cube that is not empty, so a nearer voxel
 *   one ring further out is not seen, just as the plain call does not see ring 2; what that buys is that every row the
 *   plain call labels is untouched, and that the stopping test is an integer fact about cells: no floating-point bound
 *   on where a mean representative can lie enters.  The cube of ring r - 1 of a row in the fallback holds no candidate,
 *   so the implementation scans the shell of ring r alone; the set is the same.  rings = 1 gives the plain call's
 *   labels, scores and stats, to the bit, with ring_stats[1] = stats[0].
 *   Status, in this order, all before any launch: N < 0, M < 0, K < 3, voxel_K < 3, C outside [1, 128], k outside [1, 8],
 *   rings outside [1, 8], num_rooms < 0, one of voxel_room / voxel_start without the other: CONV3P_ERR_INVALID_ARGUMENT;
 *   stats or ring_stats NULL; data, inverse or out_labels NULL with N > 0; voxel_data, neigh, voxel_scores, voxel_cell or
 *   grid_stats NULL with N > 0 and M > 0: CONV3P_ERR_INVALID_ARGUMENT; N or M > 2^31 - 1, num_rooms > 65536:
 *   CONV3P_ERR_UNSUPPORTED; workspace NULL or smaller than conv3p_grid_interpolate_rings_workspace_bytes(N) (a counter
 *   and an int32 per row): CONV3P_ERR_INVALID_ARGUMENT.  The launches depend on nothing but rings > 1: the plain call's
 *   memset and kernel, two small memsets, the list kernel, and with rings > 1 the ring kernel on a fixed grid; no host
 *   read; the only atomics are integer adds; a row in the fallback has its label and score row written by the plain pass
 *   and, where a ring finds a candidate, once more; bitwise reproducible and independent of the launch geometry and of
 *   the order of the list.
 *
 * conv3p_grid_normals_f32:  a surface normal and a curvature per voxel, from the representatives of the 3 x 3 x 3 cells
 *   around it (pointwise_amd/csrc/conv3p_grid_normals.hpp; tests/grid_normals_ref.py restates it in numpy).  A raw scan
 *   carries no normals and normals averaged over a voxel are no unit vectors; this is the estimate a model trained on
 *   files with normals is fed.  voxel_data (M, K) with row stride K, xyz first; neigh (M, 27) as conv3p_grid_neighbors
 *   writes it; grid_stats the subsampling's stats, of which grid_stats[0] = nv is read ON THE DEVICE; voxel_room int32 (M)
 *   or NULL; viewpoint float32 (V, 3) ON THE DEVICE or NULL (V is then not read): V = 1 one point for all voxels, V = R
 *   one per room, which needs voxel_room; 3 <= min_neighbors <= 27.  Let p_v = voxel_data[v][0..2] and ne = min(max(nv, 0),
 *   M).  Every float32 step below is one separately rounded operation (the library is built with -ffp-contract=off):
 *    R1. v >= ne (filler): normal 0, curvature 0, samples 0, flags -1, moments 0.
 *    R2. For t = 0 .. 26 ascending, u = neigh[v][t] is a SAMPLE when 0 <= u < ne and all three of p_u are finite (t = 13
 *        is v itself).  samples[v] = n, the number of samples; if p_v is not finite, n = 0.
 *    R3. q_u = p_u - p_v per component (centred on the voxel's own representative: the size of the room's coordinates does
 *        not enter).  m = the chain of float32 additions of q_u in ascending t, from 0, divided by float(n).  e_u = q_u -
 *        m.  C_xx, C_xy, C_xz, C_yy, C_yz, C_zz are each the chain, in ascending t from 0, of the rounded products e_a *
 *        e_b, divided by float(n).  moments[v] = {m_x, m_y, m_z, C_xx, C_xy, C_xz, C_yy, C_yz, C_zz}; all 0 for n = 0.
 *        samples and moments are defined bit for bit.
 *    R4. n < min_neighbors: flags 1.  Otherwise any moment non-finite or (C_xx + C_yy) + C_zz <= 0: flags 2.  Otherwise
 *        flags 0.  For flags != 0 normal and curvature are 0.  flags are bit for bit: they depend on R2 and R3 alone.
 *    R5. flags 0: l0 <= l1 <= l2 the eigenvalues of the symmetric C, n^ a unit eigenvector of l0, curvature = l0 / (l0 +
 *        l1 + l2) held to [0, 1/3].  These two are defined TO A TOLERANCE: against the float64 eigen-decomposition of the
 *        float32 moments, with u = 2^-24, |n^ x n_ref| <= 64 u l2 / (l1 - l0) up to sign where l1 - l0 >= 1e-3 l2,
 *        | |n^| - 1 | <= 1e-6, and the curvature within 64 u.  The solver is a cyclic Jacobi iteration of six sweeps in
 *        float64 on the float32 moments, every rotation taken: deterministic, two calls give the same bits.
 *    R6. Orientation, an exact rule on the float32 n^ about to be stored.  With a viewpoint, w = viewpoint[0], or
 *        viewpoint[voxel_room[v]] when V > 1 (a voxel whose room is outside [0, V) has no viewpoint):
 *        s = ((w_x - p_x) n_x + (w_y - p_y) n_y) + (w_z - p_z) n_z, each difference, product and addition rounded;
 *        s < 0 stores -n^.  Without a viewpoint, or when s == 0 or s is not finite: the component of largest magnitude
 *        is made positive, the lowest axis of a tie.  Negation is exact, so the rule holds on the stored vector.
 *   Outputs: normals float32 (M, 3), curvature float32 (M), samples int32 (M), flags int32 (M), moments float32 (M, 9) or
 *   NULL, normal_stats int32 (4) = {voxels with a normal, too few samples, degenerate, filler}, overwritten by every call.
 *   Status, in this order, all before any launch: M < 0, K < 3, min_neighbors outside [3, 27]: CONV3P_ERR_INVALID_ARGUMENT;
 *   viewpoint given with V < 1, or with V != 1 and voxel_room NULL: CONV3P_ERR_INVALID_ARGUMENT; M == 0: CONV3P_OK, nothing
 *   launched and nothing written; voxel_data, neigh, grid_stats, normals, curvature, samples, flags or normal_stats NULL:
 *   CONV3P_ERR_INVALID_ARGUMENT; M > 2^31 - 1, or V with a viewpoint: CONV3P_ERR_UNSUPPORTED.  One kernel launch behind a
 *   16-byte memset of normal_stats; a thread per voxel; nothing synchronised on; the only atomics are the integer adds
 *   of the four counts; no float atomics; every output word written once; bitwise reproducible and independent of the
 *   launch geometry.
 *
 * conv3p_grid_segments, conv3p_grid_absorb_segments:  the voxel labels as a spatial field -- which voxels form one
 *   connected piece of one class, how large each piece is, and a clean-up that gives small pieces the label around them
 *   (pointwise_amd/csrc/conv3p_grid_segments.hpp; tests/grid_segments_ref.py restates both in numpy).  neigh int32 (M, 27)
 *   as conv3p_grid_neighbors writes it (symmetric below ne: u = neigh[v][t] exactly when v = neigh[u][26 - t]);
 *   voxel_labels int32 (L), L <= M, or NULL (L is then not read); voxel_count int32 (M); grid_stats the subsampling's
 *   stats, of which ne = min(max(grid_stats[0], 0), M) is read ON THE DEVICE; num_class in [1, 128]; connectivity 6, 18
 *   or 26.  Everything is int32 arithmetic: exact, and independent of the launch geometry and of thread order.
 *    S1. Voxel v is LABELLED with c = voxel_labels[v] when v < ne, v < L and 0 <= c < num_class.  With voxel_labels NULL
 *        every v < ne is labelled 0 and num_class is taken as 1: the geometric components.  Every other voxel -- filler
 *        rows, v >= L, negative labels, labels >= num_class -- is unlabelled.
 *    S2. The taps of a connectivity are the t != 13 with |dx| + |dy| + |dz| <= 1 (6), <= 2 (18), <= 3 (26), t = (dx+1)*9 +
 *        (dy+1)*3 + (dz+1).  Labelled voxels u, v are JOINED when u = neigh[v][t] for such a tap, 0 <= u < ne, and both
 *        have the same label.  A segment is an equivalence class of the transitive closure.  The table is per room in the
 *        many-clouds result, so a segment never crosses a room.
 *    S3. The ROOT of a segment is its smallest voxel number; segments are numbered 0 .. S-1 in ascending root.  For one
 *        class that is scipy.ndimage.label's numbering on the dense lattice with generate_binary_structure(3, 1 | 2 | 3),
 *        minus 1.  In the many-clouds result the numbers run room after room; a segment's room is voxel_room[root].
 *    S4. Outputs, int32 (M) each, every word written: segment[v] the segment number, -1 for an unlabelled voxel; for s < S
 *        seg_root[s], seg_size[s] in voxels, seg_rows[s] the sum of voxel_count over the members (at most 2^24),
 *        seg_label[s]; for s >= S root -1, size 0, rows 0, label -1.  seg_stats int32 (8) = {S, labelled voxels,
 *        unlabelled voxels below ne, M - ne, largest seg_size, largest seg_rows, 0, 0}, overwritten by every call.
 *   The absorb is ONE pass over such a segmentation (segment, seg_size, seg_label, seg_stats as written above, the same
 *   neigh, voxel_labels, L, grid_stats, num_class and connectivity), with min_size >= 1 and drop_orphans 0 or 1:
 *    A1. Segment s is SMALL when seg_size[s] < min_size.
 *    A2. For a small s, votes[c] is the number of pairs (u, t), u in s, t a tap of the connectivity, w = neigh[u][t] with
 *        0 <= w < ne, segment[w] >= 0, segment[w] != s, that segment NOT small, seg_label[segment[w]] = c.  A neighbour of
 *        s's own label in another segment cannot exist under the same connectivity, so every vote is for another class.
 *        Small neighbours do not vote.
 *    A3. The new label of s is the class with the most votes, the lowest class of a tie.  With no votes s is an ORPHAN: it
 *        keeps its label, or takes -1 with drop_orphans.  (The geometric segmentation has one class, so every small
 *        segment is an orphan and drop_orphans is outlier removal.)
 *    A4. labels_out int32 (M): a voxel in a segment gets the segment's new or kept label; an unlabelled voxel below
 *        min(L, ne) keeps its input word; everything else -1.  seg_label_out int32 (M): per segment, -1 past S.
 *        absorb_stats int64 (4) = {small segments, absorbed (small with a vote), orphans, voxels whose label changed (the
 *        sizes of the small segments whose new label differs, dropped orphans included)}, overwritten by every call.
 *   With min_size = 1 labels_out is the labelled input to the bit.  The pass is NOT iterated: a small segment surrounded
 *   only by small segments is an orphan, and sizes are not recomputed behind the relabelling.  A caller may segment the
 *   result and run it again.
 *   Status, in this order, all before any launch: M < 0; voxel_labels given with L < 0 or L > M; num_class outside [1, 128];
 *   connectivity not 6, 18 or 26; (absorb) min_size < 1, drop_orphans not 0 or 1: CONV3P_ERR_INVALID_ARGUMENT; M == 0:
 *   CONV3P_OK, nothing launched and nothing written; any other pointer NULL: CONV3P_ERR_INVALID_ARGUMENT; M > 2^31 - 1:
 *   CONV3P_ERR_UNSUPPORTED; workspace NULL or smaller than conv3p_grid_segments_workspace_bytes(M) /
 *   conv3p_grid_absorb_workspace_bytes(M): CONV3P_ERR_INVALID_ARGUMENT.  The workspaces are 2 M and 4 M int32 plus a word
 *   or two per 2048 voxels: a function of M alone, whatever num_class.  Seven launches (segments) and six (absorb) whatever
 *   the data; no host read: ne, S and the number of small segments stay on the device.  The union-find is lock-free: its
 *   entries only ever decrease, so every retry follows another thread's progress and no loop waits for a thread to arrive.
 *   The only atomics are int32 CAS / min / max / add and the int64 adds of absorb_stats; bitwise reproducible.
 *
 * conv3p_grid_segments_smooth:  segments under a join predicate -- region growing over normals, curvature and features
 *   (pointwise_amd/csrc/conv3p_grid_smooth.hpp; tests/grid_smooth_ref.py restates it in numpy).  The arguments of
 *   conv3p_grid_segments, and: normals float32 (M, 3) or NULL; normal_flags int32 (M) or NULL; curvature float32 (M) or
 *   NULL, all as conv3p_grid_normals_f32 writes them; min_cos; signed_normals 0 or 1; max_curvature; features float32, F
 *   channels (0 with features NULL, else 1 .. 16) at a row stride of feature_stride >= F floats, or NULL; max_difference;
 *   smooth_stats int64 (8).  The workspace is that of conv3p_grid_segments_workspace_bytes(M).  The library is built with
 *   -ffp-contract=off: every float operation below is one separately rounded float32 operation.
 *    J1. Labelling is S1 and the taps are S2's.  A pair (v, u) with u = neigh[v][t] for a tap of the connectivity,
 *        0 <= u < ne, both labelled with the same label, is a CANDIDATE pair.  It is JOINED when it also passes J2, J3 and
 *        J4, each for the input that is given; at least one of normals and features must be given.  Segments are the
 *        transitive closure of the joined pairs.  Numbering and the outputs segment, seg_root, seg_size, seg_rows,
 *        seg_label and seg_stats are S3 and S4 unchanged.
 *    J2. Normals.  Voxel v HAS A NORMAL when normal_flags is NULL or normal_flags[v] == 0, and its three components are
 *        finite.  A pair with an endpoint without a normal is not joined: such a voxel is a segment of its own, not
 *        unlabelled.  d = (nx_v * nx_u + ny_v * ny_u) + nz_v * nz_u in that association, which is symmetric in u and v;
 *        with signed_normals == 0, d = fabsf(d).  The pair passes iff d >= min_cos: equality joins, a NaN does not.
 *    J3. Curvature, read only when curvature is given: the pair passes iff curvature[v] <= max_curvature and
 *        curvature[u] <= max_curvature (a NaN fails).
 *    J4. Features: the pair passes iff fabsf(f_v[k] - f_u[k]) <= max_difference for every channel k < F (a NaN fails).
 *    J5. smooth_stats int64 (8), overwritten by every call: [0] candidate pairs with u < v, so each undirected pair once
 *        (for the half taps t < 13 of a table of conv3p_grid_neighbors u < v always holds); [1] pairs joined; [2] pairs
 *        refused for a missing normal; [3] refused by angle; [4] refused by curvature; [5] refused by features; [6]
 *        labelled voxels without a normal (0 without normals); [7] 0.  The first rule that fails, in the order J2, J3, J4,
 *        takes the pair, so [0] = [1] + [2] + [3] + [4] + [5].
 *   Status: those of conv3p_grid_segments in its order (M == 0 is CONV3P_OK there, nothing launched or written); then
 *   normals and features both NULL; F outside [0, 16], or F == 0 with features given, or F > 0 without; features given
 *   with feature_stride < F; signed_normals not 0 or 1; min_cos, max_curvature or max_difference a NaN; smooth_stats NULL:
 *   CONV3P_ERR_INVALID_ARGUMENT.  All before any launch.  Seven launches whatever the data behind a 64-byte memset of
 *   smooth_stats: the two union-find kernels of conv3p_grid_segments with the predicate evaluated behind the label test,
 *   and its other five launches as they are.  The predicate reads nothing the kernels write and is evaluated before the
 *   union, so the progress argument stands: no loop waits for a thread.  J5 is counted in registers, summed over a wave
 *   by shuffles and added with 64-bit integer adds.  The only atomics are integer CAS / min / max / add; no float
 *   atomics; bitwise reproducible and independent of the launch geometry.
 *
 * conv3p_grid_segment_pool_f32, conv3p_grid_segment_pool_i64:  exact sums of a value row per voxel over the segments of
 *   any segmentation: mean normals, mean colours, summed class scores and the class they vote for
 *   (pointwise_amd/csrc/conv3p_grid_smooth.hpp; tests/grid_smooth_ref.py).  values (L, C), L <= M, C in [1, 128], at a row
 *   stride of value_stride >= C elements: float32, or int64 fixed-point sums as conv3p_scene_vote_scores_f32 writes them;
 *   segment and seg_stats as conv3p_grid_segments, _smooth or conv3p_grid_merge_segments write them; voxel_count and
 *   grid_stats the subsampling's; weight 0 (every voxel counts once) or 1 (as its voxel_count raw rows; _f32 only).
 *    P1. Membership is G1: ne and S read on the device, v < ne and 0 <= segment[v] < S.
 *    P2. A member CONTRIBUTES when v < L and, for _f32, all its C values are finite with |x| <= 256.  Its quantum of
 *        channel c is q = llrint((double)x * 2^30) for _f32 (the product is exact, the rounding to nearest even) and
 *        q = values[v][c] for _i64.
 *    P3. sums[s][c] = sum of w_v * q and weights[s] = sum of w_v over the contributors of s, w_v = 1 or voxel_count[v], in
 *        wrapping 64-bit integer arithmetic.  With |x| <= 256 and at most 2^24 rows in all, |sums| <= 2^8 * 2^30 * 2^24 =
 *        2^62: _f32 cannot wrap.
 *    P4. mean[s][c] = (double)sums[s][c] / ((double)weights[s] * 2^30): the conversions round to nearest even, the product
 *        is exact, one division.  0 where weights[s] == 0 (no contributor).
 *    P5. seg_label[s] is class 0 unless a later class is strictly greater: the lowest class of a tie wins (on
 *        non-negative sums the rule of conv3p_scene_score_labels).  -1 when weights[s] == 0 or every sum is 0.
 *        voxel_label[v] = seg_label[segment[v]] for a member, else -1.  Rows s >= S hold sums 0, weights 0, mean 0,
 *        seg_label -1.
 *    P6. pool_stats int64 (4) = {contributors, members that did not contribute, segments s < S with a label, without}.
 *   Outputs, every word written by every call: sums int64 (M, C), weights int64 (M), mean float64 (M, C) or NULL,
 *   seg_label int32 (M), voxel_label int32 (M) or NULL, pool_stats.
 *   Status, in this order, all before any launch: M < 0, L < 0 or L > M, C outside [1, 128], value_stride < C, weight not
 *   0 or 1 (_i64: not 0): CONV3P_ERR_INVALID_ARGUMENT; M == 0: CONV3P_OK, nothing launched and nothing written; values
 *   NULL with L > 0, or any other pointer but mean and voxel_label NULL: CONV3P_ERR_INVALID_ARGUMENT; M > 2^31 - 1:
 *   CONV3P_ERR_UNSUPPORTED.  NO workspace: the outputs are the accumulators.  Three launches, four with voxel_label,
 *   whatever the data (zeroes; the sums -- a wave takes consecutive voxels, reduces runs of equal segment by a segmented
 *   shuffle, carries the open run from step to step, and walks the channels eight at a time: one 64-bit integer atomic add
 *   per channel and finished run; a thread per segment for P4-P6; voxel_label).  No host read; no float atomics; bitwise
 *   reproducible and independent of the launch geometry.
 *
 * conv3p_grid_segment_geometry:  where every segment is, how large it is in space and how it is oriented -- the step from
 *   a segmentation to a list of objects (pointwise_amd/csrc/conv3p_grid_geometry.hpp; tests/grid_geometry_ref.py restates it
 *   in numpy).  voxel_data (M, K) with row stride K, xyz first; voxel_cell int32 (M, 3) and voxel_count int32 (M) as the
 *   subsampling writes them; segment int32 (M) and seg_stats as conv3p_grid_segments writes them; grid_stats the
 *   subsampling's stats; weight 0 (every voxel counts once) or 1 (every voxel counts as its raw rows).  The voxels sit on
 *   an integer lattice that is isotropic: lattice units become metres by one scale, the subsampling's voxel, and one shift,
 *   the cloud's (in the many-clouds result: the room's) minimum corner.
 *    G1. ne = min(max(grid_stats[0], 0), M) and S = min(max(seg_stats[0], 0), M), both read ON THE DEVICE.  The MEMBERS of
 *        segment s < S are the v < ne with segment[v] == s.  A word of segment outside [0, S) makes v a member of nothing.
 *    G2. cell_box int32 (M, 6) = {min i_x, min i_y, min i_z, max i_x, max i_y, max i_z} over the members' voxel_cell.  In the
 *        many-clouds result these are the room's own lattice coordinates, and the room is voxel_room[seg_root[s]].  Every
 *        raw row of a member lies in its voxel's cell, so the cell box bounds the raw rows.
 *    G3. box float32 (M, 6) = the minimum and the maximum of voxel_data[v][0..2] over the members, in the total order on
 *        the BITS b of a float: key(b) = b ^ 0x80000000 for a clear sign bit, ~b otherwise, compared as unsigned.  So -0.0
 *        is below +0.0, and a NaN or an infinity in a representative has a defined place (a NaN with a clear sign bit
 *        above +inf, one with the sign bit set below -inf).  Integer minima and maxima of keys: independent of any order.
 *    G4. moments int64 (M, 10) = {W, sum w dx, sum w dy, sum w dz, sum w dx^2, sum w dx dy, sum w dx dz, sum w dy^2,
 *        sum w dy dz, sum w dz^2} over the members, with d = voxel_cell - (the low corner of cell_box), so 0 <= d_a < 2^20,
 *        and w = 1 (weight 0) or w = voxel_count[v] (weight 1).  The sums are unsigned 64-bit, taken modulo 2^64, and
 *        stored as their bits.  For everything this library produces they are exact: a subsampling has at most 2^24 rows
 *        and as many voxels, so sum w <= 2^24, an axis has at most 2^20 cells, and (2^20 - 1)^2 * 2^24 < 2^64.
 *    G5. centroid float64 (M, 3), in lattice coordinates: c_a = (double)lo_a + (double)m1_a / (double)W -- one division and
 *        one addition, so bit-defined.  The centre of a cell in space is origin_a + (c_a + 0.5) * voxel.
 *    G6. The covariance C_ab = (double)m2_ab / (double)W - ((double)m1_a / (double)W) * ((double)m1_b / (double)W), every
 *        operation one float64 operation.  eigenvalues float64 (M, 3) are the eigenvalues of C in DESCENDING order, negative
 *        round-off held to 0; axes float64 (M, 3, 3): row k is the unit eigenvector of eigenvalues[k].  These two are
 *        defined TO A TOLERANCE, not to the bit: with u = 2^-53, t = 128 u and n = max(trace C, 1), C rebuilt from the
 *        integer moments in exact arithmetic and rounded once:  (i) |A A^T - I| <= t,  (ii) |A^T diag(l) A - C| <= t n,
 *        (iii) l descends and is >= 0,  (iv) |l_k - l_ref,k| <= t n against a float64 eigen-decomposition of C; all four
 *        entrywise and without a condition on a gap, so lines, planes and cubes are covered.  The solver is the cyclic
 *        Jacobi iteration of conv3p_grid_normals_f32, six sweeps, every rotation taken: two calls give the same bits.
 *    G7. Sign, an exact rule on the stored vector: each axis is turned so that its component of largest magnitude is
 *        positive, the lowest index of a tie.  The frame may be left-handed: no axis is turned to make a determinant +1.
 *    G8. extent float64 (M, 6) = {min p_0, min p_1, min p_2, max p_0, max p_1, max p_2} over the members, with
 *        p_k = (((double)i_x - c_x) * a_k0 + ((double)i_y - c_y) * a_k1) + ((double)i_z - c_z) * a_k2 computed from the STORED
 *        centroid and axes, every operation one float64 operation, uncontracted, in that order; minimum and maximum by the
 *        64-bit form of G3's key.  Given the stored frame this is bit-defined.  It is the oriented box of the cell
 *        CENTRES; half a cell of padding is the caller's.
 *   Filler: a row s >= S holds cell_box {0, 0, 0, -1, -1, -1} and 0 everywhere else; so does a row s < S whose W is 0, which
 *   no segmentation of this library has.  geometry_stats int32 (4) = {S, segments of one voxel (cell_box low == high),
 *   segments whose stored eigenvalues[2] is 0 (flat or thinner; filler rows are not counted), 0}, overwritten by every
 *   call.  Every output word is written by every call.
 *   Status, in this order, all before any launch: M < 0, K < 3, weight not 0 or 1: CONV3P_ERR_INVALID_ARGUMENT; M == 0:
 *   CONV3P_OK, nothing launched and nothing written; any pointer NULL: CONV3P_ERR_INVALID_ARGUMENT; M > 2^31 - 1 or
 *   K > 65536: CONV3P_ERR_UNSUPPORTED.  There is NO workspace: the sums, minima and maxima are accumulated in the output
 *   words themselves, box and extent as ordered keys that the last launch turns back into floats.  Six launches whatever
 *   the data (identities; the two boxes; the moments, which need the low corner; a thread per segment for G5-G7; the
 *   extents; keys to floats, filler, stats); no host read; the only atomics are integer min / max on 32- and 64-bit words
 *   and 64-bit integer adds, one set per run of equal segment among the consecutive voxels of a wave; no float atomics;
 *   everything but G6 is bitwise independent of the launch geometry and of thread order, and G6 is a function of the exact
 *   moments alone.
 *
 * conv3p_grid_segment_adjacency:  which segments touch -- the region adjacency graph of a segmentation in CSR form, with
 *   exact integer contact statistics per edge and per segment (pointwise_amd/csrc/conv3p_grid_adjacency.hpp;
 *   tests/grid_adjacency_ref.py restates it in numpy).  neigh int32 (M, 27) as conv3p_grid_neighbors writes it; segment
 *   int32 (M) and seg_stats as conv3p_grid_segments (or conv3p_grid_merge_segments) writes them -- any array with values
 *   in [-1, S) is legal; grid_stats the subsampling's stats; connectivity 6, 18 or 26, independent of the connectivity
 *   that made the segments; max_edges >= 0, the rows of the edge arrays.
 *    E1. ne = min(max(grid_stats[0], 0), M) and S = min(max(seg_stats[0], 0), M), both read ON THE DEVICE.  Voxel v < ne is
 *        a MEMBER of a = segment[v] when 0 <= a < S; any other word makes v a member of nothing.
 *    E2. A CONTACT from a to b is a pair (v, t): v a member of a, t a tap of the connectivity (the taps of S2),
 *        w = neigh[v][t] with 0 <= w < ne, w a member of b, and b != a.
 *    E3. The directed EDGE (a, b) exists when there is at least one contact from a to b.  The table is symmetric below ne,
 *        so (v, t) is a contact a -> b exactly when (w, 26 - t) is a contact b -> a: edges come in pairs and E, the number
 *        of directed edges, is even.
 *    E4. Per edge e, the edges in ascending (a, b), int32 (max_edges) each: edge_src[e] = a; edge_dst[e] = b;
 *        edge_contacts[e] the number of contacts a -> b (the twin's value); edge_voxels[e] the number of distinct v in a
 *        with a contact to b -- the border of a towards b, not symmetric; edge_offset int32 (max_edges, 3) the sum over
 *        the contacts of the tap's (dx, dy, dz), the exact negative of the twin's (a positive dz: b lies above a);
 *        edge_twin[e] the index of edge (b, a).  Contacts are at most 26 * 2^24, so int32 holds every sum.
 *    E5. adj_start int32 (M + 1): adj_start[s] is the number of edges with src < s for s <= S, and E for s > S.  Row s of
 *        the CSR is [adj_start[s], adj_start[s + 1]) and its edge_dst ascends.
 *    E6. seg_border int32 (M, 4), for s < S counts of the (member, tap) pairs of s, 0 for s >= S, whatever max_edges:
 *        {contacts to any other segment; pairs whose neighbour is a voxel below ne that is a member of nothing; pairs with
 *        no neighbour (neigh < 0 or >= ne); members with at least one pair of these three kinds -- the surface voxels}.
 *    E7. B is the number of distinct (member voxel, foreign segment) pairs, the sum of edge_voxels over all edges; it is
 *        always computed and E <= B <= 26 M.  If E <= max_edges: rows e >= E hold src = dst = twin = -1 and 0, and
 *        adj_stats int64 (8) = {E, B, S, total contacts, largest degree, largest edge_contacts, 0, 0}.  Otherwise
 *        (OVERFLOW): every edge row is filler, adj_start is all 0, seg_border is still exact and adj_stats = {-1, B, S,
 *        total contacts, 0, 0, 1, 0}; a caller retries with max_edges = B, which always fits.  Every output word is
 *        written by every call.
 *   Status, in this order, all before any launch: M < 0, connectivity not 6, 18 or 26, max_edges < 0:
 *   CONV3P_ERR_INVALID_ARGUMENT; M == 0: CONV3P_OK, nothing launched and nothing written; any pointer NULL (the six edge
 *   arrays may be NULL with max_edges == 0): CONV3P_ERR_INVALID_ARGUMENT; M or max_edges > 2^31 - 1:
 *   CONV3P_ERR_UNSUPPORTED; workspace NULL or smaller than conv3p_grid_adjacency_scratch_bytes(M, max_edges):
 *   CONV3P_ERR_INVALID_ARGUMENT.  The workspace is 18 words per row of max_edges (an open-addressed table of
 *   2 max_edges + 64 slots, a 64-bit key and five counters each, and the two key buffers of the sort) plus a few KiB and
 *   a histogram of 256 words per 4096 edges: a function of max_edges, nothing per voxel and no record per contact.
 *   5 + 6 b launches with b the bytes of M - 1 (11, 17, 23, 29 for M <= 2^8, 2^16, 2^24, beyond): fixed by M whatever
 *   the data; the radix passes above the top byte of S - 1 return at once.  No host read; no float arithmetic; the only
 *   atomics are the 64-bit CAS that claims a slot, int32 adds and maxima, and the 64-bit adds of three counters.  Every
 *   probe loop is bounded by the table's size and none waits for a thread.  Slot order is not reproducible; the outputs
 *   are: the claimed keys are sorted before anything is written.
 *
 * conv3p_grid_merge_segments:  any set of segment pairs collapsed by union-find into a new segmentation.  segment,
 *   seg_root, seg_size, seg_rows, seg_label, seg_stats of a segmentation numbered by S3; pair_a, pair_b int32 (P), P >= 0;
 *   select int32 (P) or NULL.
 *    U1. Pair p is ACTIVE when select is NULL or select[p] != 0, and 0 <= pair_a[p], pair_b[p] < S.  So the filler rows
 *        of an adjacency (-1) are ignored, one direction of an edge is enough, and a == b joins nothing.
 *    U2. A GROUP is a class of the transitive closure of the active pairs over the segments 0 .. S-1.  Its root segment
 *        is its lowest number; groups are numbered 0 .. S'-1 in ascending root segment -- by S3 in ascending root voxel,
 *        so the result is again numbered by S3.
 *    U3. Outputs, int32 (M) each: seg_map[s] the group of s, -1 for s >= S; segment_out[v] = seg_map[segment[v]] where
 *        0 <= segment[v] < S, -1 otherwise; root_out the seg_root of the root segment; size_out and rows_out the sums over
 *        the group; label_out the seg_label of the member with the largest seg_size, the lowest number on a tie; rows
 *        past S' as S4 fills them.  stats_out int32 (8) has S4's layout: entry 0 is S', 1-3 are copied from seg_stats,
 *        4-5 are the new maxima.
 *    U4. merge_stats int32 (4) = {S', S, active pairs with a != b, groups of more than one segment}.
 *    U5. With no active pair every output equals the input segmentation to the bit and seg_map is the identity.
 *   Status, in this order, all before any launch: M < 0 or P < 0: CONV3P_ERR_INVALID_ARGUMENT; M == 0: CONV3P_OK, nothing
 *   launched; any pointer NULL (select may be; pair_a, pair_b only with P == 0): CONV3P_ERR_INVALID_ARGUMENT; M or
 *   P > 2^31 - 1: CONV3P_ERR_UNSUPPORTED; workspace NULL or smaller than conv3p_grid_merge_scratch_bytes(M):
 *   CONV3P_ERR_INVALID_ARGUMENT.  The workspace is 5 M words plus a word per 2048 segments: a function of M alone.  Seven
 *   launches whatever the data; no host read; the union-find is that of conv3p_grid_segments (lock-free, entries only
 *   ever decrease); the only atomics are int32 CAS / min / max / add and the 64-bit maximum of size << 32 |
 *   (0x7fffffff - s) that picks the label; bitwise reproducible.
 * ------------------------------------------------------------------------------------------- */
#define CONV3P_GRID_MEAN 0
#define CONV3P_GRID_CENTER 1
size_t conv3p_grid_subsample_workspace_bytes(int64_t N, int max_voxels);
int conv3p_grid_subsample_f32(const float *data, const void *labels, int64_t N, int K, int label_bytes, float voxel,
                              int mode, int num_class, int max_voxels, float *out, int32_t *labels_out,
                              int32_t *voxel_row, int32_t *voxel_count, int32_t *voxel_cell, int32_t *inverse,
                              int32_t *stats, void *workspace, size_t workspace_bytes, void *stream);
int conv3p_grid_project_labels(const int32_t *voxel_labels, const int32_t *inverse, int64_t N, int64_t M, int32_t *out,
                               void *stream);
size_t conv3p_grid_subsample_rooms_workspace_bytes(int64_t N, int64_t R, int max_voxels);
int conv3p_grid_subsample_rooms_f32(const float *data, const void *labels, const int32_t *room_start, int64_t N, int64_t R,
                                    int K, int label_bytes, float voxel, int mode, int num_class, int max_voxels,
                                    float *out, int32_t *labels_out, int32_t *voxel_row, int32_t *voxel_count,
                                    int32_t *voxel_cell, int32_t *voxel_room, int32_t *voxel_start, int32_t *inverse,
                                    int32_t *room_stats, int32_t *stats, void *workspace, size_t workspace_bytes,
                                    void *stream);
int conv3p_grid_neighbors(const int32_t *voxel_cell, const int32_t *voxel_room, const int32_t *voxel_start,
                          const int32_t *grid_stats, int max_voxels, int64_t num_rooms, int32_t *neigh, void *stream);
int conv3p_grid_interpolate_f32(const float *data, int64_t N, int K, const int32_t *inverse, const float *voxel_data,
                                int voxel_K, const int32_t *neigh, const float *voxel_scores, int64_t M, int C,
                                const int32_t *valid_labels, int k, int32_t *out_labels, float *out_scores, int64_t *stats,
                                void *stream);
int conv3p_grid_interpolate_i64(const float *data, int64_t N, int K, const int32_t *inverse, const float *voxel_data,
                                int voxel_K, const int32_t *neigh, const int64_t *voxel_scores, int64_t M, int C,
                                const int32_t *valid_labels, int k, int32_t *out_labels, float *out_scores, int64_t *stats,
                                void *stream);
size_t conv3p_grid_interpolate_rings_workspace_bytes(int64_t N);
int conv3p_grid_interpolate_rings_f32(const float *data, int64_t N, int K, const int32_t *inverse, const float *voxel_data,
                                      int voxel_K, const int32_t *neigh, const int32_t *voxel_cell, const int32_t *voxel_room,
                                      const int32_t *voxel_start, int64_t num_rooms, const int32_t *grid_stats,
                                      const float *voxel_scores, int64_t M, int C, const int32_t *valid_labels, int k, int rings,
                                      int32_t *out_labels, float *out_scores, int32_t *out_ring, int64_t *stats,
                                      int64_t *ring_stats, void *workspace, size_t workspace_bytes, void *stream);
int conv3p_grid_interpolate_rings_i64(const float *data, int64_t N, int K, const int32_t *inverse, const float *voxel_data,
                                      int voxel_K, const int32_t *neigh, const int32_t *voxel_cell, const int32_t *voxel_room,
                                      const int32_t *voxel_start, int64_t num_rooms, const int32_t *grid_stats,
                                      const int64_t *voxel_scores, int64_t M, int C, const int32_t *valid_labels, int k, int rings,
                                      int32_t *out_labels, float *out_scores, int32_t *out_ring, int64_t *stats,
                                      int64_t *ring_stats, void *workspace, size_t workspace_bytes, void *stream);
int conv3p_grid_normals_f32(const float *voxel_data, int K, const int32_t *neigh, const int32_t *grid_stats,
                            const int32_t *voxel_room, const float *viewpoint, int64_t V, int64_t M, int min_neighbors,
                            float *normals, float *curvature, int32_t *samples, int32_t *flags, float *moments,
                            int32_t *normal_stats, void *stream);
size_t conv3p_grid_segments_workspace_bytes(int64_t M);
int conv3p_grid_segments(const int32_t *neigh, const int32_t *voxel_labels, int64_t L, const int32_t *voxel_count,
                         const int32_t *grid_stats, int64_t M, int num_class, int connectivity, int32_t *segment,
                         int32_t *seg_root, int32_t *seg_size, int32_t *seg_rows, int32_t *seg_label, int32_t *seg_stats,
                         void *workspace, size_t workspace_bytes, void *stream);
int conv3p_grid_segments_smooth(const int32_t *neigh, const int32_t *voxel_labels, int64_t L, const int32_t *voxel_count,
                                const int32_t *grid_stats, int64_t M, int num_class, int connectivity, int32_t *segment,
                                int32_t *seg_root, int32_t *seg_size, int32_t *seg_rows, int32_t *seg_label,
                                int32_t *seg_stats, const float *normals, const int32_t *normal_flags, const float *curvature,
                                float min_cos, int signed_normals, float max_curvature, const float *features, int F,
                                int64_t feature_stride, float max_difference, int64_t *smooth_stats, void *workspace,
                                size_t workspace_bytes, void *stream);
int conv3p_grid_segment_pool_f32(const float *values, int64_t L, int C, int64_t value_stride, const int32_t *segment,
                                 const int32_t *seg_stats, const int32_t *voxel_count, const int32_t *grid_stats, int64_t M,
                                 int weight, int64_t *sums, int64_t *weights, double *mean, int32_t *seg_label,
                                 int32_t *voxel_label, int64_t *pool_stats, void *stream);
int conv3p_grid_segment_pool_i64(const int64_t *values, int64_t L, int C, int64_t value_stride, const int32_t *segment,
                                 const int32_t *seg_stats, const int32_t *voxel_count, const int32_t *grid_stats, int64_t M,
                                 int weight, int64_t *sums, int64_t *weights, double *mean, int32_t *seg_label,
                                 int32_t *voxel_label, int64_t *pool_stats, void *stream);
size_t conv3p_grid_absorb_workspace_bytes(int64_t M);
int conv3p_grid_absorb_segments(const int32_t *neigh, const int32_t *voxel_labels, int64_t L, const int32_t *segment,
                                const int32_t *seg_size, const int32_t *seg_label, const int32_t *seg_stats,
                                const int32_t *grid_stats, int64_t M, int num_class, int connectivity, int min_size,
                                int drop_orphans, int32_t *labels_out, int32_t *seg_label_out, int64_t *absorb_stats,
                                void *workspace, size_t workspace_bytes, void *stream);
int conv3p_grid_segment_geometry(const float *voxel_data, int K, const int32_t *voxel_cell, const int32_t *voxel_count,
                                 const int32_t *segment, const int32_t *seg_stats, const int32_t *grid_stats,
                                 int64_t M, int weight,
                                 int32_t *cell_box, float *box, int64_t *moments,
                                 double *centroid, double *eigenvalues, double *axes, double *extent,
                                 int32_t *geometry_stats, void *stream);
size_t conv3p_grid_adjacency_scratch_bytes(int64_t M, int64_t max_edges);
int conv3p_grid_segment_adjacency(const int32_t *neigh, const int32_t *segment, const int32_t *seg_stats,
                                  const int32_t *grid_stats, int64_t M, int connectivity, int64_t max_edges,
                                  int32_t *adj_start, int32_t *edge_src, int32_t *edge_dst, int32_t *edge_contacts,
                                  int32_t *edge_voxels, int32_t *edge_offset, int32_t *edge_twin, int32_t *seg_border,
                                  int64_t *adj_stats, void *workspace, size_t workspace_bytes, void *stream);
size_t conv3p_grid_merge_scratch_bytes(int64_t M);
int conv3p_grid_merge_segments(const int32_t *segment, const int32_t *seg_root, const int32_t *seg_size,
                               const int32_t *seg_rows, const int32_t *seg_label, const int32_t *seg_stats,
                               const int32_t *pair_a, const int32_t *pair_b, const int32_t *select, int64_t P, int64_t M,
                               int32_t *seg_map, int32_t *segment_out, int32_t *root_out, int32_t *size_out,
                               int32_t *rows_out, int32_t *label_out, int32_t *stats_out, int32_t *merge_stats,
                               void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * The dense head of the classification model (/root/reference/pointcnn2_acsd.py:69-75:
 * view (B, N*36) -> fully_connected 512, selu -> dropout_selu -> fully_connected num_class, selu).
 * tf.contrib.layers.fully_connected is y = activation(x . W + b) with W of shape (K, N).
 *
 * conv3p_fc_forward_f32   y (M, N) = act(x (M, K) . W (K, N) + b (N));  act: 0 = identity, 1 = SELU; b may be NULL.
 * conv3p_fc_backward_f32  given y (the forward OUTPUT) and dy = dL/dy:  dW (K, N) = x^T . dz,  db (N) = sum_m dz,
 *                         dx (M, K) = dz . W^T  with dz = dy * act'(y);  dx and db may be NULL.
 * W is streamed exactly once per pass (it is the 151 MB object of the model); products are exact fp32 on the
 * matrix cores; results are bitwise reproducible.  Constraints: N % 8 == 0, N <= 1024, M <= 128
 * (CONV3P_ERR_UNSUPPORTED otherwise).  The backward (and conv3p_fc_backward_step_f32) keeps all of dz in LDS for the dW
 * pass, 2 STEPS rows of N + 1 floats within 160 KiB with STEPS = 16, 32, 64 for M <= 32, <= 64, <= 128, and so also
 * refuses (CONV3P_ERR_UNSUPPORTED, before anything is launched)
 *     33 <= M <= 64   with N > 632
 *     65 <= M <= 128  with N > 312
 * which the forward serves.  Scratch from conv3p_fc_workspace_bytes: 0 where the FORWARD's constraints fail; it does
 * not reflect the backward's two regions (it is non-zero there).
 * One size serves the forward, the backward and conv3p_fc_backward_step_f32, and each of them checks its buffer against
 * that size (CONV3P_ERR_WORKSPACE), whichever part of it the call itself uses.
 * A non-finite input reaches exactly the outputs whose sums it enters (padded rows, columns and K-steps are zero on
 * both operands: no 0 * Inf).  M == 0: nothing forward; the backward writes dW = 0 and, when given, db = 0.
 * ------------------------------------------------------------------------------------------- */
size_t conv3p_fc_workspace_bytes(int M, int K, int N);
int conv3p_fc_forward_f32(const float *x, const float *W, const float *b, int M, int K, int N, int act, float *y,
                          void *workspace, size_t workspace_bytes, void *stream);
int conv3p_fc_backward_f32(const float *x, const float *W, const float *y, const float *dy, int M, int K, int N,
                           int act, float *dx, float *dW, float *db, void *workspace, size_t workspace_bytes,
                           void *stream);

/* ---------------------------------------------------------------------------------------------
 * The per-point loss head of the segmentation model as one fused pass
 * (/root/reference/scene_seg/pointcnn_scene_seg_acsd.py:60-71: softmax cross-entropy over every point, mean over all
 * B*N points) together with the statistics the reference's loops compute after every batch with a Python double loop
 * (/root/reference/scene_seg/train_scene_seg_s3dis.py:134-145, eval_scene_seg_s3dis.py:88-98).
 *
 * act (rows, num_class) row-major: the SELU'd output of the last layer, rows = B*N, 2 <= num_class <= 128;
 * labels int32[rows].  Per row, with m = max_c act[r][c]:
 *   row loss      = log(sum_c exp(act[r][c] - m)) + m - act[r][label]
 *   grad_act[r]   = (softmax(act[r]) - onehot(label)) * grad_scale       (NULL: evaluation, no gradient)
 *   pred[r]       = first index of the maximum, as np.argmax             (may be NULL)
 *   *loss_sum     = sum of the row losses (double, device), NOT scaled: the mean is *loss_sum * grad_scale
 *   counts        = int64[2 + 3 * num_class] (device): {correct, invalid, seen[C], correct_class[C], predicted[C]}
 * grad_scale = 1 / (number of points the mean runs over; those of all ranks in data-parallel runs).
 * A label outside [0, num_class) makes an ignored row: loss 0 (what tf.one_hot gives), gradient row 0, counted in
 * `invalid` only; the denominator is the caller's.  Labels are thereby validated on the device without a host
 * synchronisation.  A NaN in a row reaches *loss_sum and that row's gradient.
 * Two launches on `stream`, no memset, no atomics on global memory: bitwise reproducible; grad_act and pred of a row
 * do not depend on the other rows.  Scratch from conv3p_seg_head_workspace_bytes (either element type).
 * Status: CONV3P_ERR_INVALID_ARGUMENT for rows == 0, num_class < 2 or NULL act / labels / loss_sum / counts;
 * CONV3P_ERR_UNSUPPORTED when four 64-row tiles of (num_class | 1) elements do not fit in the CU's LDS (fp32: up to
 * 128 classes; fp64: up to 79, so 64 works and 128 does not); CONV3P_ERR_WORKSPACE; nothing is launched on an error.
 * ------------------------------------------------------------------------------------------- */
size_t conv3p_seg_head_workspace_bytes(size_t rows, int num_class);
int conv3p_seg_head_f32(const float *act, const int32_t *labels, size_t rows, int num_class, float grad_scale,
                        float *grad_act, int32_t *pred, double *loss_sum, int64_t *counts, void *workspace,
                        size_t workspace_bytes, void *stream);
int conv3p_seg_head_f64(const double *act, const int32_t *labels, size_t rows, int num_class, double grad_scale,
                        double *grad_act, int32_t *pred, double *loss_sum, int64_t *counts, void *workspace,
                        size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * The same head with the other arguments of the call it replaces,
 * tf.losses.softmax_cross_entropy(onehot_labels, logits, weights, label_smoothing, reduction)
 * (scene_seg/pointcnn_scene_seg_acsd.py:66-67), and the confusion matrix of an evaluation.  Kernels and the exact
 * arithmetic: csrc/conv3p_seg_head_weighted.hpp.
 *
 * Row weight  w_r = [label in [0, num_class)] * class_weight[label] * point_weight[r]; class_weight (num_class) and
 * point_weight (rows) are device arrays of the element type, either may be NULL (= 1).  Weights are NOT validated: a
 * negative, infinite or NaN weight propagates to the total, *loss_sum and that row's gradient.
 *
 * conv3p_seg_weight_total_f32 / _f64   (pointcnn_scene_seg_acsd.py:66-67: the denominator of the `reduction`)
 *   total = double[2] (device): {sum_r w_r, number of rows with w_r != 0}; reads labels and the weights only.  Two
 *   launches, fixed summation order: equal inputs give equal bits.  total[0] is the denominator of torch's weighted
 *   mean, total[1] that of TensorFlow's SUM_BY_NONZERO_WEIGHTS; a data-parallel caller all-reduces `total` first.
 *
 * conv3p_seg_head_weighted_f32 / _f64  (pointcnn_scene_seg_acsd.py:66-67: the loss itself)
 *   conv3p_seg_head_* with, per valid row and ls = label_smoothing in [0, 1):
 *     target q_c     = (1 - ls) [c == label] + ls / num_class       (TensorFlow's rule, not torch's class-weighted one)
 *     row loss       = w_r * (logsumexp(act[r]) - (1 - ls) act[r][label] - (ls / num_class) sum_c act[r][c])
 *     grad_act[r][c] = w_r * (softmax(act[r])_c - q_c) * scale
 *     scale          = grad_scale, or with denominator != NULL (a device double, e.g. total + 0 or total + 1)
 *                      grad_scale / *denominator, and 0 when *denominator == 0 (gradient all +0)
 *     *loss_sum      = sum of the row losses (double, device), NOT scaled
 *   A row with w_r == 0 has no loss and a +0 gradient row but still counts in seen / correct_class / predicted.  A
 *   label outside [0, num_class) is an ignored row as in conv3p_seg_head_* (TensorFlow would charge such a row the
 *   uniform part of a smoothed target; here it stays ignored).  pred, counts, the NaN / inf behaviour and the
 *   reproducibility are those of conv3p_seg_head_*; with class_weight == point_weight == denominator == NULL and
 *   label_smoothing == 0 every output is bit-equal to it.  No host synchronisation: the denominator is read on the
 *   device.
 *
 * conv3p_seg_confusion                 (the evaluation of a model trained with pointcnn_scene_seg_acsd.py:66-67)
 *   confusion = int64[num_class][num_class] (device): confusion[label][pred] over the rows whose label and pred are
 *   both in [0, num_class); exact.  Two launches.
 *
 * Scratch: conv3p_seg_head_weighted_workspace_bytes covers conv3p_seg_weight_total_* and conv3p_seg_head_weighted_*
 * (one buffer may serve both calls on one stream; each checks for the whole of it, as conv3p_seg_head_* check for the
 * whole of conv3p_seg_head_workspace_bytes), conv3p_seg_confusion_workspace_bytes the matrix; 0 for a refused
 * shape.  Status, decided before any launch: CONV3P_ERR_INVALID_ARGUMENT for rows == 0, num_class < 2, a NULL act /
 * labels / loss_sum / counts (total; pred / confusion), label_smoothing outside [0, 1) or NaN; CONV3P_ERR_UNSUPPORTED
 * above the class limit of conv3p_seg_head_* (fp32 and the confusion matrix 128, fp64 79); CONV3P_ERR_WORKSPACE.
 * ------------------------------------------------------------------------------------------- */
size_t conv3p_seg_head_weighted_workspace_bytes(size_t rows, int num_class);
int conv3p_seg_weight_total_f32(const int32_t *labels, size_t rows, int num_class, const float *class_weight,
                                const float *point_weight, double *total, void *workspace, size_t workspace_bytes,
                                void *stream);
int conv3p_seg_weight_total_f64(const int32_t *labels, size_t rows, int num_class, const double *class_weight,
                                const double *point_weight, double *total, void *workspace, size_t workspace_bytes,
                                void *stream);
int conv3p_seg_head_weighted_f32(const float *act, const int32_t *labels, size_t rows, int num_class,
                                 const float *class_weight, const float *point_weight, double label_smoothing,
                                 float grad_scale, const double *denominator, float *grad_act, int32_t *pred,
                                 double *loss_sum, int64_t *counts, void *workspace, size_t workspace_bytes, void *stream);
int conv3p_seg_head_weighted_f64(const double *act, const int32_t *labels, size_t rows, int num_class,
                                 const double *class_weight, const double *point_weight, double label_smoothing,
                                 double grad_scale, const double *denominator, double *grad_act, int32_t *pred,
                                 double *loss_sum, int64_t *counts, void *workspace, size_t workspace_bytes, void *stream);
size_t conv3p_seg_confusion_workspace_bytes(size_t rows, int num_class);
int conv3p_seg_confusion(const int32_t *labels, const int32_t *pred, size_t rows, int num_class, int64_t *confusion,
                         void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * The optimizer step of all three training drivers: tf.train.MomentumOptimizer(learning_rate, momentum)
 * (train_modelnet40_acsd.py:81, scene_seg/train_scene_seg_s3dis.py:83, train_scene_seg_scenenn.py:86),
 * i.e. TensorFlow's non-Nesterov ApplyMomentum, in place, per element:
 *   accum = accum * momentum + grad
 *   param = param - accum * lr
 * Each statement is two separately rounded operations (no fused multiply-add): bit-equal to numpy's `a * m + g` and
 * `w - a * lr` in the element type.  A NaN or Inf in grad propagates to that element, as in TensorFlow.  lr is the
 * value of the schedule (train_modelnet40_acsd.py:78-79, a host computation) for this step.
 *
 * conv3p_momentum_step_f32 / _f64   n_tensors <= CONV3P_OPT_MAX_TENSORS tensors in ONE launch on `stream`.  params,
 *   grads, accums, numels are HOST arrays of n_tensors entries (as the tables of conv3p_stack_*), read before the call
 *   returns; the pointers in them are device pointers aligned to the element size (16-byte accesses are used wherever
 *   the three pointers of a tensor share their offset inside a 16-byte line).  A tensor of 0 elements is legal and
 *   its pointers may be NULL.  The result does not depend on how tensors are grouped into calls.
 *   Status, decided before any launch: n_tensors < 0 or > CONV3P_OPT_MAX_TENSORS, a NULL array (n_tensors > 0), a NULL
 *   or misaligned entry with a non-zero count -> CONV3P_ERR_INVALID_ARGUMENT; n_tensors == 0 or all counts zero ->
 *   CONV3P_OK, nothing launched.
 *
 * conv3p_fc_backward_step_f32   conv3p_fc_backward_f32 (pointcnn2_acsd.py:71, the minimize() of
 *   train_modelnet40_acsd.py:82 on its weights) with the update in the epilogue of the dW pass: W, b and their
 *   accumulators are updated in place, dW and db never reach memory (two reads and two writes of W's size instead of
 *   one write, three reads and two writes).  dx (may be NULL) is computed from W as it was BEFORE the call.  W, accum_W,
 *   b, accum_b afterwards are bit-equal to conv3p_fc_backward_f32 followed by conv3p_momentum_step_f32.
 *   b and accum_b may both be NULL (one without the other: CONV3P_ERR_INVALID_ARGUMENT).  Constraints, scratch and
 *   status codes of conv3p_fc_backward_f32, except M == 0 with K * N > 0: CONV3P_ERR_INVALID_ARGUMENT (no batch, no
 *   gradient to step with).
 * ------------------------------------------------------------------------------------------- */
#define CONV3P_OPT_MAX_TENSORS 16
int conv3p_momentum_step_f32(int n_tensors, float *const *params, const float *const *grads, float *const *accums,
                             const size_t *numels, float lr, float momentum, void *stream);
int conv3p_momentum_step_f64(int n_tensors, double *const *params, const double *const *grads, double *const *accums,
                             const size_t *numels, double lr, double momentum, void *stream);
int conv3p_fc_backward_step_f32(const float *x, float *W, float *b, const float *y, const float *dy, int M, int K, int N,
                                int act, float *dx, float *accum_W, float *accum_b, float lr, float momentum,
                                void *workspace, size_t workspace_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * The same step with the rest of the call it replaces: the use_nesterov argument of tf.train.MomentumOptimizer, the
 * tf.clip_by_global_norm a TF1 driver puts between compute_gradients and apply_gradients, and a step that is not
 * taken when a gradient holds a NaN or an Inf.  The norm is found on the device and used on the device: no host
 * synchronisation.  Kernels and the exact arithmetic: csrc/conv3p_optim_guarded.hpp.
 *
 * conv3p_grad_norm_f32 / _f64   stats = double[2] (device): {sum over all elements of grad^2, number of elements that
 *   are NaN or +-Inf}.  grads and numels are HOST arrays of n_tensors <= CONV3P_OPT_MAX_TENSORS entries as in
 *   conv3p_momentum_step_*; a tensor of 0 elements is legal and its pointer may be NULL.  Squares and sums are double
 *   (an fp32 square is exact), a non-finite element contributes 0 to stats[0] and 1 to stats[1]; when stats[0] itself
 *   is not finite (fp64 squares can overflow) stats[1] is one larger, so stats[1] > 0 whenever stats[0] is unusable.
 *   accumulate != 0 adds to what stats holds: more than 16 tensors, both element types or several calls chain in
 *   stream order, e.g. f32(.., accumulate 0), f64(.., accumulate 1).  Two launches, no memset, no atomic, a grid that
 *   depends on the element counts alone: equal arguments give equal bits (the result does depend on how tensors are
 *   grouped into calls and on their alignment, within the rounding of a double sum of non-negative terms).
 *   Nothing to read (n_tensors == 0 or all counts zero): accumulate == 0 writes {0, 0} (one launch), accumulate != 0
 *   launches nothing.  Scratch: conv3p_grad_norm_workspace_bytes(), needed only when there is something to read.
 *   Status, decided before any launch: n_tensors out of range, NULL stats, a NULL array (n_tensors > 0), a NULL or
 *   misaligned entry with a non-zero count -> CONV3P_ERR_INVALID_ARGUMENT; CONV3P_ERR_WORKSPACE.
 *
 * conv3p_momentum_step_guarded_f32 / _f64   conv3p_momentum_step_* with, uniformly over the call:
 *   skip   skip_nonfinite != 0 and stats[1] > 0: nothing is read or written, params and accums keep their bits
 *   clip   clip_norm > 0: grad' = grad * scale (one rounded multiply), scale = (T)(clip_norm / max(sqrt(stats[0]),
 *          clip_norm)) with sqrt and division correctly rounded in double and one rounding to the element type;
 *          exactly 1 (the step is bit-equal to the unclipped one) when the norm is at most clip_norm, 0 when stats[0]
 *          is not finite.  clip_norm <= 0: no clipping
 *   rule   nesterov == 0: the rule above.  nesterov != 0: TensorFlow's ApplyMomentum with use_nesterov,
 *            accum = accum * momentum + grad'
 *            param = param - (grad' * lr + (accum * momentum) * lr)
 *          every product and sum separately rounded: bit-equal to numpy evaluating these statements in the element type
 *   stats is the device double[2] of conv3p_grad_norm_* (or those of all ranks, summed); it is read only when clipping
 *   or skipping is asked for and may be NULL otherwise.  With nesterov == 0, clip_norm <= 0 and skip_nonfinite == 0 the
 *   call is conv3p_momentum_step_*: the same kernel, the same bits.  Without skipping, a NaN or Inf in grad reaches
 *   its element as before (it is not part of the norm).  One launch.
 *   Status, decided before any launch: those of conv3p_momentum_step_*; a NaN or infinite clip_norm, or stats == NULL
 *   with clip_norm > 0 or skip_nonfinite != 0 -> CONV3P_ERR_INVALID_ARGUMENT.
 * ------------------------------------------------------------------------------------------- */
size_t conv3p_grad_norm_workspace_bytes(void);
int conv3p_grad_norm_f32(int n_tensors, const float *const *grads, const size_t *numels, double *stats, int accumulate,
                         void *workspace, size_t workspace_bytes, void *stream);
int conv3p_grad_norm_f64(int n_tensors, const double *const *grads, const size_t *numels, double *stats, int accumulate,
                         void *workspace, size_t workspace_bytes, void *stream);
int conv3p_momentum_step_guarded_f32(int n_tensors, float *const *params, const float *const *grads, float *const *accums,
                                     const size_t *numels, float lr, float momentum, int nesterov, float clip_norm,
                                     int skip_nonfinite, const double *stats, void *stream);
int conv3p_momentum_step_guarded_f64(int n_tensors, double *const *params, const double *const *grads,
                                     double *const *accums, const size_t *numels, double lr, double momentum, int nesterov,
                                     double clip_norm, int skip_nonfinite, const double *stats, void *stream);

/* ---------------------------------------------------------------------------------------------
 * The tail of the classification model's training step as two launches: everything between fc1's output and fc1's
 * backward (/root/reference/pointcnn2_acsd.py:73-90: dropout_selu, fully_connected num_class selu, mean sparse softmax
 * cross-entropy; /root/reference/selu.py:35-70), the statistics of /root/reference/train_modelnet40_acsd.py:136-146
 * (argmax, correct clouds, per-class seen / correct) and, in the _step form, minimize()'s update of W2 / b2
 * (train_modelnet40_acsd.py:82).  fp32.
 *
 * fc1 (M, H): the SELU'd output of fc1, 16-byte aligned; W2 (H, C); b2 (C); labels int32[M].  Per row m:
 *   drop[m]     = training && rate > 0 ? a * (fc1[m] * keep + alpha' * (1 - keep)) + b : fc1[m]      (selu.py:56-62; a, b,
 *                 alpha' of selu.py:36-61 for keep_prob = 1 - rate, computed in double, used in fp32)
 *   logits[m]   = selu(drop[m] . W2 + b2)                                 (M, C), required
 *   pred[m]     = first index of the row maximum, as np.argmax           (may be NULL)
 *   row loss    = log(sum_c exp(logits - max)) + max - logits[label]
 *   dz[m]       = (softmax(logits[m]) - onehot(label)) * grad_scale * selu'(logits[m])   (through the output, as fc_backward)
 *   dfc1[m]     = (dz[m] . W2^T) * (dropout ? a * keep : 1)              (M, H): the dy of conv3p_fc_backward_f32 for fc1
 * and across rows, in ascending row order with a fixed association:
 *   dW2 (H, C)  = drop^T . dz,   db2 (C) = sum_m dz[m]
 *   *loss_sum   = sum of the row losses (double, device), NOT scaled
 *   counts      = int64[2 + 3 C] (device): {correct, invalid, seen[C], correct_class[C], predicted[C]}, the layout of
 *                 conv3p_seg_head_*
 * A label outside [0, C) makes an ignored row: loss 0, dz and dfc1 rows +0, counted in `invalid` only; no host
 * synchronisation.  A NaN in a row of fc1 reaches *loss_sum and that row of dfc1 (and dW2, db2), no other row.
 *
 * keep: keep_mask (M, H) float 0 / 1, 16-byte aligned; or keep_mask == NULL: drawn with Philox4x32-10, key = (low, high
 * 32 bits of seed), counter = (e >> 2, 0, low, high 32 bits of step) with e = m * H + h, output word e & 3,
 * u = (word >> 8) * 2^-24, keep = floorf((float)(1 - rate) + u) (selu.py:53-55): a function of (seed, step, m, h) alone.
 * keep_out (uint8 (M, H), may be NULL) receives the mask whenever dropout is applied, from either source.
 *
 * dfc1 == NULL: evaluation -- no gradient work, dW2 / db2 are not touched; logits, pred, *loss_sum and counts are
 * produced.  training == 0 switches the dropout off (drop = fc1) with or without gradients.
 * conv3p_cls_tail_step_f32: accum_W2 (H, C) and accum_b2 (C) in place of dW2 / db2: the second launch applies
 * ApplyMomentum (see conv3p_momentum_step_f32) to W2, b2 and the accumulators in place; dW2 / db2 are never written,
 * dfc1 comes from W2 as it was BEFORE the call; W2, b2 and the accumulators afterwards are bit-equal to
 * conv3p_cls_tail_f32 followed by conv3p_momentum_step_f32.
 * Two launches on `stream`, no memset, no atomic on global memory: bitwise reproducible; logits, pred and dfc1 of a row
 * do not depend on the other rows of the call.  Scratch from conv3p_cls_tail_workspace_bytes (0 for a refused shape).
 * Status, decided before any launch: CONV3P_ERR_INVALID_ARGUMENT for NULL fc1 / W2 / b2 / labels / logits / loss_sum /
 * counts, M <= 0, H <= 0, C < 2, rate outside [0, 1) when training, dfc1 without dW2 and db2, misaligned fc1 /
 * keep_mask, and in the _step form a NULL dfc1 or accumulator; CONV3P_ERR_UNSUPPORTED unless M <= 128, H % 8 == 0,
 * H <= 1024, C <= 128 (C need not be a multiple of 8); CONV3P_ERR_WORKSPACE.
 * ------------------------------------------------------------------------------------------- */
size_t conv3p_cls_tail_workspace_bytes(int M, int H, int C);
int conv3p_cls_tail_f32(const float *fc1, const float *W2, const float *b2, const int32_t *labels, int M, int H, int C,
                        int training, double rate, const float *keep_mask, uint64_t seed, uint64_t step, float grad_scale,
                        float *logits, int32_t *pred, float *dfc1, float *dW2, float *db2, uint8_t *keep_out,
                        double *loss_sum, int64_t *counts, void *workspace, size_t workspace_bytes, void *stream);
int conv3p_cls_tail_step_f32(const float *fc1, float *W2, float *b2, const int32_t *labels, int M, int H, int C,
                             int training, double rate, const float *keep_mask, uint64_t seed, uint64_t step,
                             float grad_scale, float *logits, int32_t *pred, float *dfc1, float *accum_W2, float *accum_b2,
                             float lr, float momentum, uint8_t *keep_out, double *loss_sum, int64_t *counts,
                             void *workspace, size_t workspace_bytes, void *stream);

/* Kernel-level timing with HIP events recorded on the caller's stream (bench.py uses it
 * to derive the roofline of the dominant kernel).  Off by default; when enabled every
 * kernel launch of this library is bracketed by an event pair.  read() synchronises the
 * recorded events and returns the number of distinct kernel ids; per id: launches and
 * total milliseconds.  name() gives the kernel-id's label. */
int conv3p_profile_enable(int on);
int conv3p_profile_reset(void);
int conv3p_profile_kinds(void);
const char *conv3p_profile_name(int kind);
int conv3p_profile_read(int kind, uint64_t *launches, double *total_ms);

const char *conv3p_status_string(int status);
int conv3p_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* CONV3P_H */
