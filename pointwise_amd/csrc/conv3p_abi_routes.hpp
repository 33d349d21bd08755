// conv3p_abi_routes.hpp -- the kernel families and the planners that choose among them: Route, the LDS formulas, the
// scratch carves, the register and matrix-core launchers with their shape tables, plan_forward / plan_backward and the
// scratch sizes that follow from them.  Included by conv3p_abi.hip.
namespace {

// ----------------------------------------------------------------------------- routes
// (Cin, Cout) pairs with register-resident rows: the layers of the reference's two models
// (pointcnn2_acsd.py:48-66: Cin->9, 9->9; pointcnn_scene_seg_acsd.py:51-57: +36->num_class,
// 13 classes for S3DIS) plus a few neighbours.  Everything else takes the generic path.
#define CONV3P_SMALL_SHAPES(X) X(3, 9) X(6, 9) X(9, 9) X(12, 9) X(36, 13) X(3, 3) X(9, 3)

// The kernel family that serves one pass of a call and what it needs.  plan_forward / plan_backward (below) are the one
// place that chooses it, from the call's dtype, channels, stencil, strides, hints and precision, before anything is
// launched; the workspace and cache sizes are the same planners applied to the undilated stencil.
enum class Family { Register, Split36x13, MatrixCore, Wide, F64Blocks, Generic, Unsupported };
struct Route {
    Family family = Family::Generic;
    int cip = 0, cop = 0;       // MatrixCore: the padded (instantiated) channel class
    int co = 0;                 // F64Blocks backward: output channels per block (8, 4 or 2)
    int cap = 0;                // Register, fp32 backward: rows of the populated-rows G (0: the dense-G kernel only)
    bool regime = false;        // ... and the dense-G kernel after it, the slot's regime word letting exactly one of them run
    bool tap = false;           // Register, fp32 forward: transform + gather
    size_t lds = 0;             // dynamic LDS of the route's kernel (Split36x13: its 5-column pass; MatrixCore, Wide: unused)
    size_t lds4 = 0;            // Split36x13: its 4-column passes
    size_t sparse_lds = 0;      // Register, fp32 backward: the populated-rows kernel
    size_t generic_lds = 0;     // the generic kernel (also over the tiles the matrix-core kernels flag)
    int slots = 1;              // Register, Generic backward: grad_filter partials
    size_t scratch = 0;         // bytes of per-call scratch the route uses (backward: at least the generic fallback's)
    size_t mandatory = 0;       // ... of them, what the call cannot run without (the rest only lets it take this route)
    bool self_reduces = true;   // backward: writes grad_filter itself (Register leaves per-workgroup partials instead)
};
// What a route depends on besides the dtype, Dims and stencil.  have: bytes of scratch of the buffer (SIZE_MAX when
// sizing one); pair_slots, ngroups: the buffer's pair storage and search groups (scratch of the matrix-core path).
struct PlanArgs {
    bool strided = false;       // some tensor is a column block of a wider buffer (register kernels only)
    bool sparse_hint = false, dense_hint = false;
    int prec = kPrecF32;
    size_t pair_slots = 0;
    int ngroups = 1;
    size_t have = SIZE_MAX;
};

// Generic backward: every pair adds Cin*Cout products to grad_filter with global atomics.  One shared copy
// serialises them all on the same few addresses (cfg2-sized 5->7: 67 ms); the workgroups therefore spread over
// `slots` partial copies (workgroup % slots), at most one per workgroup and at most 64 MiB in total, summed by
// reduce_partials_kernel.
inline int generic_slots(const Dims &d, int elem)
{
    const size_t nw = (size_t)d.ntap * d.Cin * d.Cout;
    const size_t grid = (size_t)grid_of(make_blockmap(d));
    size_t s = nw ? ((size_t)64 << 20) / (nw * (size_t)elem) : 1;
    if (s > grid) s = grid;
    return s < 1 ? 1 : (int)s;
}

// ----------------------------------------------------------------------------- deep-channel path
// Channel shapes served by the matrix-core kernels of conv3p_deep.hpp (fp32 only): every layer with up to 128
// channels on either side, padded to the instantiated sizes {32, 64, 128}, plus the 128 -> 256 layer of BASELINE
// config 5.  (Cin, Cout) below are the PADDED sizes.
#define CONV3P_DEEP_SHAPES(X) X(128, 256) X(256, 256) X(256, 128) X(32, 32) X(32, 64) X(32, 128) X(64, 32) X(64, 64) X(64, 128) X(128, 32) X(128, 64) X(128, 128)

inline int deep_pad(int c) { return c <= 32 ? 32 : c <= 64 ? 64 : c <= 128 ? 128 : c <= 256 ? 256 : 0; }

constexpr int kDwItems = 1024;        // target number of deep_dw_kernel work items (2 rounds at 2 per CU)
struct DeepScratch {   // carved from the per-call scratch region
    float *wt;             // zero-padded (and, for grad_input, transposed) filter [F][Kpad][Npad]
    uint2 *tap_meta;       // per pair slot, tap-major inside a tile: {neighbour, centre lane | population << 8}
    uint32_t *tap_off;     // [tiles][F+1]
    uint8_t *tile_flag;    // [tiles]
    unsigned long long *pop_mask;   // [tiles] bit f: the tile has records of backward tap f (deep_order -> deep_plan)
    uint4 *tap_split;      // [tiles][F] quarter points of every (tile, tap) run (deep_order -> deep_gemm stage 1)
    unsigned long long *tap_cmask;   // [tiles][F] centres with records of the backward tap: the rows of G_f' that exist
    uint32_t *sched;       // [8][sched_cap] launch order of the tiles per XCD (deep_sched_kernel)
    int sched_cap;
    uint2 *dsegs;          // [tiles] {first slot in tap_meta, records} of every tile (deep_order; all search groups together)
    uint32_t *meta_cursor; // [B] slot allocator of tap_meta for tiles searched in several groups (N > 8192)
    uint32_t *tap_total;   // [64] pairs per backward tap, then [1] number of work items  (deep_plan_kernel)
    uint2 *tap_rng;        // [64] partial slots of each tap
    uint4 *items;          // [kDwItems + 64] deep_dw_kernel work items
    float *partials;       // [kDwItems + 64][Cin*Cout] item partials, then [F*Cin*Cout] the generic kernel's share
    float *gbuf;           // [tiles][F][64][Coutpad]: G_f' of every (tile, backward tap), grad_input -> grad_filter pass
    size_t bytes;
};

// The record orders (deep_order_kernel) come FIRST and twice -- forward taps and backward taps -- at offsets that do not
// depend on the channel counts: a geometry prefetch (CONV3P_CACHE_PREPARE_DEEP_ORDERS) builds both ahead of the
// layer's calls, which then find them in place.  `which`: 0 = the forward's set, 1 = the backward's.
DeepScratch carve_deep(const Dims &d, size_t pair_slots, void *base, int which, size_t *order_bytes = nullptr, size_t *forward_bytes = nullptr)
{
    DeepScratch s{};
    Carver cv(base);
    const size_t nw = (size_t)d.ntap * d.Cin * d.Cout;
    const size_t cip = (size_t)deep_pad(d.Cin), cop = (size_t)deep_pad(d.Cout);
    const size_t tiles = (size_t)d.B * d.ntiles;
    s.sched_cap = ((d.B + 7) / 8) * d.ntiles;
    for (int w = 0; w < 2; ++w) {
        uint2 *tap_meta = cv.take<uint2>(pair_slots);
        uint32_t *tap_off = cv.take<uint32_t>(tiles * (d.ntap + 1));
        uint8_t *tile_flag = cv.take<uint8_t>(tiles);
        uint4 *tap_split = cv.take<uint4>(tiles * d.ntap);
        uint32_t *sched = cv.take<uint32_t>((size_t)8 * s.sched_cap);
        uint2 *dsegs = cv.take<uint2>(tiles);
        uint32_t *meta_cursor = cv.take<uint32_t>((size_t)d.B);
        if (w == which) {
            s.tap_meta = tap_meta; s.tap_off = tap_off; s.tile_flag = tile_flag; s.tap_split = tap_split;
            s.sched = sched; s.dsegs = dsegs; s.meta_cursor = meta_cursor;
        }
    }
    // backward only
    s.pop_mask = cv.take<unsigned long long>(tiles);
    s.tap_cmask = cv.take<unsigned long long>(tiles * d.ntap);
    s.tap_total = cv.take<uint32_t>(65);
    s.tap_rng = cv.take<uint2>(64);
    s.items = cv.take<uint4>((size_t)(kDwItems + 64));
    if (order_bytes) *order_bytes = cv.bytes();
    s.wt = cv.take<float>((size_t)d.ntap * cip * cop);
    if (forward_bytes) *forward_bytes = cv.bytes();   // everything below is the backward's (work-item partials, the G tiles)
    s.partials = cv.take<float>((size_t)(kDwItems + 64) * cip * cop + nw);
    s.gbuf = cv.take<float>(tiles * d.ntap * 64 * cop);
    s.bytes = cv.bytes();
    return s;
}

size_t deep_scratch_bytes(const Dims &d, size_t pair_slots) { return carve_deep(d, pair_slots, nullptr, 0).bytes; }
// what a FORWARD call of the matrix-core path touches: the record orders and the padded filter -- not the backward's G tiles
// (B x tiles x taps x 64 x Cout floats: 3.6 GB for the cfg5 shard) nor its partials
size_t deep_forward_bytes(const Dims &d, size_t pair_slots)
{
    size_t b = 0;
    (void)carve_deep(d, pair_slots, nullptr, 0, nullptr, &b);
    return b;
}
// the part of it the record orders take (the same for every channel shape)
size_t deep_order_bytes(const Dims &d, size_t pair_slots)
{
    size_t b = 0;
    (void)carve_deep(d, pair_slots, nullptr, 0, &b);
    return b;
}

// fp32 layers with more than 256 channels on a side (round 4): column blocks of at most 256 x 256 channels on the
// matrix-core kernels -- the op is linear in the input-channel blocks and independent over the output-channel blocks
// -- instead of the global-atomics kernels.  Scratch: the matrix-core path's own for a 256 x 256 block, then packed
// copies of the block's rows (input / grad_out / result: 3 x [B N][256]) and of its filter block and grad_filter block.
constexpr int kWideBlk = 256;
inline bool wide_shape(int elem, int cin, int cout)
{
    return elem == 4 && cin >= 1 && cout >= 1 && (cin > kWideBlk || cout > kWideBlk);
}
struct WideScratch {
    float *xp, *yp, *zp;   // [B N][256] packed rows: block input, block grad_out (backward), block result
    float *wp, *dwp;       // [ntap][256][256] packed filter block, its grad_filter block
};
// forward_part: the packs follow the forward's part of the block scratch only
inline size_t carve_wide_scratch(const Dims &d, size_t pair_slots, bool forward_part, void *base, WideScratch &w)
{
    Dims db = d;
    db.Cin = kWideBlk;    // (blocks are padded to 128 or 256 channels: sized for the largest)
    db.Cout = kWideBlk;
    const size_t rows = (size_t)d.B * d.N;
    Carver cv(base);
    (void)cv.take<char>(forward_part ? deep_forward_bytes(db, pair_slots) : deep_scratch_bytes(db, pair_slots));
    w.xp = cv.take<float>(rows * kWideBlk);
    w.yp = cv.take<float>(rows * kWideBlk);
    w.zp = cv.take<float>(rows * kWideBlk);
    w.wp = cv.take<float>((size_t)d.ntap * kWideBlk * kWideBlk);
    w.dwp = cv.take<float>((size_t)d.ntap * kWideBlk * kWideBlk);
    return cv.bytes();
}
inline size_t wide_scratch_bytes(const Dims &d, size_t pair_slots, bool forward_only = false)
{
    WideScratch w;
    return carve_wide_scratch(d, pair_slots, forward_only, nullptr, w);
}

// fp64 layers outside the register-path shapes (round 4): blocks of 16 input x 8 output channels, zero-padded, on the
// register-path kernels <double, 16, 8> (their G matrix, 27 x 8 rows of 65 doubles = 112 KB, and transposed filter fit LDS
// in double) -- the op is linear in the input-channel blocks and independent over the output-channel blocks -- instead
// of the global-atomics kernels.  Block sizes measured in round 6 (profiles/r06_f64_blocks.txt; 32 -> 64 at the cfg2
// size): 16 x 4 1.36 / 3.81 ms, 16 x 8 0.91 / 3.41, 16 x 16 forward 1.21, 32 x 16 forward 0.90, 32 x 4 backward 3.77.
// Scratch: the block kernel's grad_filter partials, packed rows (input [B N][16], grad_out / result [B N][8] and
// [B N][16]) and the packed filter block and its grad_filter block.
#ifndef CONV3P_F64_FWD_KI
#define CONV3P_F64_FWD_KI 16
#define CONV3P_F64_FWD_CO 8
#endif
#ifndef CONV3P_F64_BWD_KI
#define CONV3P_F64_BWD_KI 16
#define CONV3P_F64_BWD_CO 8
#endif
constexpr int kF64FwdKi = CONV3P_F64_FWD_KI, kF64FwdCo = CONV3P_F64_FWD_CO;   // block of the forward pass
constexpr int kF64BwdKi = CONV3P_F64_BWD_KI, kF64BwdCo = CONV3P_F64_BWD_CO;   // block of the backward pass
constexpr int kF64Ki = kF64FwdKi > kF64BwdKi ? kF64FwdKi : kF64BwdKi;         // (scratch: sized for the larger of the two)
constexpr int kF64Co = kF64FwdCo > kF64BwdCo ? kF64FwdCo : kF64BwdCo;
constexpr int kF64Row = kF64Ki > kF64Co ? kF64Ki : kF64Co;
struct F64Scratch {
    double *parts;          // the block kernel's grad_filter partials
    double *xp, *yp, *zp;   // packed rows: input block [B N][16], grad_out block / forward result [B N][8], grad_input block [B N][16]
    double *wp, *dwp;       // [ntap][16][8] filter block, its grad_filter block
};
inline size_t carve_f64_scratch(const Dims &d, void *base, F64Scratch &w)
{
    const size_t rows = (size_t)d.B * d.N, nwb = (size_t)d.ntap * kF64Ki * kF64Co;
    Carver cv(base);
    w.parts = cv.take<double>((size_t)grid_of(make_blockmap(d)) * nwb);
    w.xp = cv.take<double>(rows * kF64Row);
    w.yp = cv.take<double>(rows * kF64Row);
    w.zp = cv.take<double>(rows * kF64Row);
    w.wp = cv.take<double>(nwb);
    w.dwp = cv.take<double>(nwb);
    return cv.bytes();
}
inline size_t f64_blocked_bytes(const Dims &d)
{
    F64Scratch w;
    return carve_f64_scratch(d, nullptr, w);
}

// The transform + gather forward's scratch (conv3p_forward_taps.hpp): Z [B N][ntap][16] floats.
inline size_t tap_forward_bytes(const Dims &d) { return (size_t)d.B * d.N * (size_t)d.ntap * kZRow * 4; }

inline int wide_pad(int n) { return n <= 128 ? 128 : 256; }

// lds: the route's (plan_forward); tap: the transform + gather forward (fp32 Cin >= 16, Cout <= 16 register shapes)
template <typename T, int CI, int CO>
int launch_forward(const Call<T> &c, size_t lds, bool tap, const T *input, const T *filter, T *output,
                   const uint8_t *only_flagged = nullptr)
{
    const Dims &d = c.d;
    const Stencil<T> &st = c.st;
    const auto &S = c.L.slot[c.slot];
    if constexpr (sizeof(T) == 4 && CI >= 16 && CI % 4 == 0 && CO <= 16) {
        // transform + gather (conv3p_forward_taps.hpp): Z = X . W[f] for every point and tap, then 64 bytes per pair
        if (tap) {
            float *z = c.L.partials;
            const size_t rows = (size_t)d.B * d.N;
            const BlockMap bm = make_blockmap(d);
#ifdef CONV3P_DEV_WALK_STATS
            dev_walk_stats(c, "tap_gather_kernel", CI, CO);
#endif
            Scope sc(K_FORWARD, c.s);
            hipLaunchKernelGGL((tap_transform_kernel<CI, CO>), dim3((unsigned)((rows + 127) / 128)), dim3(256), 0, c.s, input,
                               filter, z, rows, st.ntap, c.ld.in);
            launch_lds(tap_gather_kernel<CO>, dim3(grid_of(bm)), dim3(256), lds, c.s, c.L.pts, c.L.boxes, S.count, S.pairs, S.segs,
                       S.qsegs, z, st, d.N, d.ntiles, c.L.ngroups, bm, output, c.act ? 1 : 0, st.window ? c.L.cmin : nullptr,
                       S.tcount, c.ld, sched_of(S));
            return hip_ok();
        }
    }
    const BlockMap bm = make_blockmap(d);
#ifdef CONV3P_DEV_WALK_STATS
    if (CI > 0) dev_walk_stats(c, "forward_kernel", CI, CO);
#endif
    // (the generic form over a whole call has a kind of its own; over the tiles another path flagged, forward_kernel's)
    Scope sc(CI == 0 && only_flagged == nullptr ? K_GENERIC_FWD : K_FORWARD, c.s);
    launch_lds(forward_kernel<T, CI, CO>, dim3(grid_of(bm)), dim3(256), lds, c.s, c.L.pts, c.L.boxes, S.count, S.pairs, S.segs,
               S.qsegs, input, filter, st, d.N, d.ntiles, c.L.ngroups, d.Cin, d.Cout, bm, output, only_flagged,
               (CI > 0 && c.act) ? 1 : 0, st.window ? c.L.cmin : nullptr, S.tcount, c.ld, sched_of(S));
    return hip_ok();
}

// LDS of forward_kernel<T, cin, cout> (cin == 0: its generic form)
template <typename T> size_t forward_lds(const Stencil<T> &st, int cin, int cout)
{
    return lds_common(st) + (cin > 0 ? a16((size_t)st.ntap * fwd_wstr<T>(cin, cout) * sizeof(T)) : 0) +
           a16((size_t)st.ntap * kCntStride * sizeof(T)) + 256 + a16((size_t)kWavesPerBlock * 192 * 4) +
           (cin > 0 ? a16((size_t)kWavesPerBlock * cout * 64 * sizeof(T)) : 0);
}
// LDS of tap_gather_kernel<cout>
inline size_t tap_gather_lds(const Stencil<float> &st, int cout)
{
    return lds_common(st) + a16((size_t)st.ntap * kCntStride * 4) + 256 + a16((size_t)kWavesPerBlock * 192 * 4) +
           a16((size_t)kWavesPerBlock * cout * 64 * 4);
}
// LDS of backward_kernel<T, cin, cout>, the dense-G kernel (cin == 0: its generic form); its reduce buffer [4][cin][64]
// aliases { Wt | X tile | SoA }
template <typename T> size_t dense_backward_lds(const Stencil<T> &st, int cin, int cout)
{
    const size_t nw = (size_t)st.ntap * cin * cout;
    size_t tail = (cin > 0 ? a16(nw * sizeof(T)) + a16((size_t)64 * cin * sizeof(T)) : 0) + a16((size_t)kWavesPerBlock * 192 * 4);
    const size_t red = cin > 0 ? a16((size_t)kWavesPerBlock * cin * 64 * sizeof(T)) : 0;
    if (tail < red) tail = red;
    return lds_common(st) + (cin > 0 ? a16((size_t)st.ntap * cout * kCntStride * sizeof(T)) + a16(256 * sizeof(T)) : 0) + 256 + tail;
}
// Rows of the populated-rows G matrix (conv3p_backward_sparse.hpp) that fit LDS next to the kernel's other arrays with
// four (else three, else two) workgroups per CU; 0: use backward_kernel's dense G.
template <typename T> int sparse_cap(const Stencil<T> &st, int cin, int cout, size_t &lds)
{
    // (phase B holds the output channels in one 16-wide block; 33 .. 64 taps: the narrow layers' 64-bit tap sets, 65 .. 128:
    // 128-bit ones -- round 6: a 5 x 5 x 5 filter stays on the deterministic kernels)
    if (st.ntap > 128 || (st.ntap > 32 && cin >= 16) || cin < 1 || cout < 1 || cout > 16) return 0;
    // Undilated stencils populate a third of a centre's taps and more (adjacent cells: 9 of 27 on the ModelNet-shaped
    // clouds, 650-850 rows per tile): their tiles would take two rounds, each walking the pair lists again
    // (measured: 3 -> 9 stride 1 at the cfg2 size 63.8 us against 49.5 us dense).  Dilated ones: 210-450 rows.
    // (Unless the dense G does not fit LDS at all -- filters of many taps: then the rounds are the only register path.)
#ifndef CONV3P_DEV_SPARSE_UNDILATED   // developer A/B build: the populated-rows kernel for undilated narrow layers too
    if (cin < 16 && st.step[0] * st.step[1] * st.step[2] == 1 && dense_backward_lds<T>(st, cin, cout) <= kMaxLds) return 0;
#endif
    const size_t fixed = sparse_fixed_lds<T>(st.maxfull, st.ntap, cin, cout) + 64;
    const size_t budgets[3] = {40960, 54608, 81920};
    for (size_t bud : budgets) {
        if (cin >= 16 && bud < 81920) continue;   // wide rows: 2 waves per SIMD for the registers (dX rows of Cin values)
        if (bud <= fixed) continue;
        long long cap = (long long)((bud - fixed) / ((size_t)cout * sizeof(T)));
        if (cap > 64LL * st.ntap) cap = 64LL * st.ntap;
        if (cap < (long long)sparse_min_rows<T>(cin, cout)) continue;
        if (cap >= 256 || cap == 64LL * st.ntap) {
            lds = fixed + (size_t)cap * cout * sizeof(T);
            return (int)cap;
        }
    }
    return 0;
}
template <typename T> Stencil<T> undilated_stencil(const Dims &d)
{
    const int32_t one[3] = {1, 1, 1};
    return make_stencil<T>(d, one, (T)1);
}

// workgroups a launch appends for its reduction rider (reduce_rider, conv3p_kernels.hpp)
template <typename T> inline unsigned rider_grid(const ReduceJob<T> &rider)
{
    return rider.nslots > 0 ? rider_blocks(rider.nw) : 0u;
}
// the first backward launch of a Register route can carry a rider: its dynamic LDS holds the rider's [16][kRiderW] sums
template <typename T> inline bool rider_fits(const Route &r)
{
    return (r.cap > 0 ? r.sparse_lds : r.lds) >= (size_t)16 * kRiderW * sizeof(T);
}

// The populated-rows kernel: narrow dilated layers when the pair lists are short, layers of >= 16 inputs always (their
// dense G plus the transposed filter take 151 KiB of LDS, one workgroup per CU; the populated rows fit two), and filters
// whose dense G does not fit LDS at all.  regime: launched for the short-lists case only -- the dense-G kernel follows and
// the slot's regime word (tile_sched_kernel, from the lists just built) lets exactly one of them run: the choice needs
// neither the caller nor a host synchronisation, at the price of one empty launch (~5 us).
template <typename T, int CI, int CO>
int launch_backward_sparse(const Call<T> &c, const Route &r, const T *grad_out, const T *input, const T *filter,
                           T *grad_input, T *partials)
{
    if constexpr (CI > 0 && CO <= 16 && sizeof(T) == 4) {
        const Dims &d = c.d;
        const Stencil<T> &st = c.st;
        const auto &S = c.L.slot[c.slot];
        const BlockMap bm = make_blockmap(d);
        Scope sc(K_BACKWARD, c.s);
        auto go = [&](auto kern) {
            launch_lds(kern, dim3(grid_of(bm) + rider_grid(c.rider)), dim3(256), r.sparse_lds, c.s, c.L.pts, c.L.boxes, S.count, S.pairs,
                       S.segs, S.qsegs, S.qbm, S.qbm_hi, grad_out, input, filter, st, d.N, d.ntiles, c.L.ngroups, bm, grad_input,
                       partials, (c.act ? 1 : 0) | (c.accum ? 2 : 0), c.addend, st.window ? c.L.cmin : nullptr, c.ld, r.cap,
                       sched_of(S), r.regime ? S.regime : static_cast<const uint32_t *>(nullptr), c.rider, grid_of(bm));
        };
        if constexpr (CI < 16) {
            if (st.ntap > 64) go(backward_sparse_kernel<T, CI, CO, 2>);        // 128-bit tap sets
            else if (st.ntap > 32) go(backward_sparse_kernel<T, CI, CO, 1>);   // 64-bit tap sets
            else go(backward_sparse_kernel<T, CI, CO, 0>);
        } else {
            go(backward_sparse_kernel<T, CI, CO, 0>);
        }
        return hip_ok();
    } else {
        return CONV3P_ERR_UNSUPPORTED;   // (never planned: fp64 and wide outputs have no populated-rows kernel)
    }
}

// The dense-G kernel (CI == 0: its generic form).  lds: the route's (plan_backward); regime: see launch_backward_sparse.
template <typename T, int CI, int CO>
int launch_backward(const Call<T> &c, size_t lds, const T *grad_out, const T *input, const T *filter, T *grad_input,
                    T *partials, const uint8_t *only_flagged = nullptr, int gen_slots = 1, const uint32_t *regime = nullptr,
                    const ReduceJob<T> &rider = ReduceJob<T>{})
{
    const Dims &d = c.d;
    const Stencil<T> &st = c.st;
    const auto &S = c.L.slot[c.slot];
    const BlockMap bm = make_blockmap(d);
    Scope sc(CI == 0 && only_flagged == nullptr ? K_GENERIC_BWD : K_BACKWARD, c.s);
    launch_lds(backward_kernel<T, CI, CO>, dim3(grid_of(bm) + rider_grid(rider)), dim3(256), lds, c.s, c.L.pts, c.L.boxes, S.count,
               S.pairs, S.segs, S.qsegs, grad_out, input, filter, st, d.N, d.ntiles, c.L.ngroups, d.Cin, d.Cout, bm, grad_input,
               partials, only_flagged, ((CI > 0 && c.act) ? 1 : 0) | ((CI > 0 && c.accum) ? 2 : 0), c.addend, gen_slots,
               st.window ? c.L.cmin : nullptr, c.ld, sched_of(S), regime, rider, grid_of(bm));
    return hip_ok();
}

// A register-path shape's pass as the route says (the table of instantiations below)
template <typename T, int CI, int CO>
int register_forward(const Call<T> &c, const Route &r, const T *input, const T *filter, T *output)
{
    return launch_forward<T, CI, CO>(c, r.lds, r.tap, input, filter, output);
}
template <typename T, int CI, int CO>
int register_backward(const Call<T> &c, const Route &r, const T *grad_out, const T *input, const T *filter, T *grad_input,
                      T *partials)
{
    if (r.cap > 0) TRY((launch_backward_sparse<T, CI, CO>(c, r, grad_out, input, filter, grad_input, partials)));
    if (r.cap > 0 && !r.regime) return CONV3P_OK;
    // (a rider goes with the call's FIRST launch: the populated-rows kernel's when there is one)
    return launch_backward<T, CI, CO>(c, r.lds, grad_out, input, filter, grad_input, partials, nullptr, 1,
                                      r.cap > 0 ? c.L.slot[c.slot].regime : nullptr, r.cap > 0 ? ReduceJob<T>{} : c.rider);
}
template <typename T> struct RegisterShape {
    int cin, cout;
    int (*forward)(const Call<T> &, const Route &, const T *, const T *, T *);
    int (*backward)(const Call<T> &, const Route &, const T *, const T *, const T *, T *, T *);
};
template <typename T> const RegisterShape<T> kRegisterShapes[] = {
#define X(ci, co) {ci, co, register_forward<T, ci, co>, register_backward<T, ci, co>},
    CONV3P_SMALL_SHAPES(X)
#undef X
};
template <typename T> const RegisterShape<T> *register_shape(int cin, int cout)
{
    for (const RegisterShape<T> &e : kRegisterShapes<T>)
        if (e.cin == cin && e.cout == cout) return &e;
    return nullptr;
}
inline bool small_shape(int elem, int cin, int cout)
{
#ifdef CONV3P_DEV_SKIP_SMALL   // developer build only (-DCONV3P_DEV_SKIP_SMALL): time the other paths on the models' shapes
    return false;
#endif
    (void)elem;   // fp32 and fp64 (the kernels are templates on T; the planner sends shapes whose LDS does not fit elsewhere)
    return register_shape<float>(cin, cout) != nullptr;
}

// LDS of deep_order_kernel (ngroups: search groups of the layout)
inline size_t deep_order_lds(int ntap, int ngroups) { return (size_t)(2 + 4 * kOrderR + 64) * ntap * 4 + 256 + (size_t)(2 * 64 * ngroups + 1 + 8) * 4; }
// LDS of deep_dw_kernel<ci, co, prec> (nh: its column parts; bf16: 2-byte images of X and G)
inline size_t deep_dw_lds(int ci, int co, int nh, int prec)
{
    return prec == kPrecF32 ? (size_t)DEEP_DW_ROWS * (ci + 1) * 4 + (size_t)DEEP_DW_ROWS * (co / nh + 1) * 4 + 256
                            : (size_t)DEEP_DW_ROWS * (ci + co / nh) * 2 + 256;
}

template <bool BWD> int launch_deep_order(const Call<float> &c, const DeepScratch &ds)
{
    const Dims &d = c.d;
    if (d.ntap > 64) return CONV3P_ERR_UNSUPPORTED;
    if (c.order_ok[BWD ? 1 : 0]) return CONV3P_OK;   // built for this geometry by an earlier call, scratch untouched since
    const auto &S = c.L.slot[c.slot];
    const int ng = c.L.ngroups;
    const size_t lds = deep_order_lds(d.ntap, ng);
    if (lds > kMaxLds) return CONV3P_ERR_UNSUPPORTED;
    Scope sc(K_DEEP_ORDER, c.s);
    if (BWD) TRY(zero_async(ds.tap_total, 65 * 4, c.s));
    if (ng > 1) TRY(zero_async(ds.meta_cursor, (size_t)d.B * 4, c.s));
    launch_lds(deep_order_kernel<BWD>, dim3((unsigned)(d.B * d.ntiles)), dim3(256), lds, c.s, c.L.pts, S.count, S.pairs, S.segs, d.N,
               d.ntiles, d.ntap, ng, S.qsegs, ds.dsegs, ds.meta_cursor, c.L.pairs_per_cloud, ds.tap_meta, ds.tap_off, ds.tile_flag,
               BWD ? ds.tap_total : nullptr, BWD ? ds.pop_mask : nullptr, ds.tap_split, BWD ? ds.tap_cmask : nullptr);
    hipLaunchKernelGGL(deep_sched_kernel, dim3(8), dim3(1024), 0, c.s, ds.dsegs, d.B, d.ntiles, ds.sched_cap, ds.sched);
    if (BWD)
        hipLaunchKernelGGL(deep_plan_kernel, dim3(1), dim3(1024), (size_t)(d.B * d.ntiles <= kPlanTiles ? d.B * d.ntiles : 0) * 8, c.s,
                           ds.tap_total, ds.pop_mask, d.ntap, d.B * d.ntiles, kDwItems,
                           ds.items, ds.tap_rng, ds.tap_total + 64);
    note_deep_order(c, BWD ? 1 : 0);
    return hip_ok();
}

template <int KD, int ND, bool BWD>
int launch_deep_gemm(const Call<float> &c, const float *src, const float *Bm, float *out, const DeepScratch &ds,
                     int kreal, int nreal, float *gbuf = nullptr, const float *xin = nullptr)
{
    const Dims &d = c.d;
    const auto &S = c.L.slot[c.slot];
    const size_t lds = a16((size_t)(KD < 256 ? 256 / KD : 1) * 64 * (KD + 4) * 4) + 68 * 4 + 256 + 4096 + 512;
    if (lds > kMaxLds) return CONV3P_ERR_UNSUPPORTED;
    if ((size_t)d.N * (size_t)kreal * 4 > 0xFFFFFFFFull) return CONV3P_ERR_UNSUPPORTED;   // (stage 1 addresses rows by 32-bit offsets)
    const BlockMap bm = make_blockmap(d);
    Scope sc(c.prec != kPrecF32 ? K_DEEP_GEMM_BF16 : K_DEEP_GEMM, c.s);
    auto go = [&](auto kern) {
        launch_lds(kern, dim3(grid_of(bm)), dim3(256), lds, c.s, c.L.pts, S.pairs, ds.dsegs, src, Bm, d.N, d.ntiles, d.ntap, ds.sched,
                   ds.sched_cap, out, ds.tap_meta, ds.tap_off, ds.tile_flag, kreal, nreal, gbuf, xin, ds.tap_split, ds.tap_cmask);
    };
    // rows shorter than 4 floats (only possible in the 32-column class) take the variant with scalar row loads
    auto go_prec = [&](auto wide_c) {
        constexpr bool kWide = decltype(wide_c)::value;
        if (c.prec == kPrecBf16) go(deep_gemm_kernel<KD, ND, BWD, kWide, kPrecBf16>);
        else go(deep_gemm_kernel<KD, ND, BWD, kWide, kPrecF32>);
    };
    if constexpr (KD == 32) {
        if (kreal < 4) {
            go_prec(std::false_type{});
            return hip_ok();
        }
    }
    go_prec(std::true_type{});
    return hip_ok();
}

int launch_pad_filter(const Call<float> &c, const float *filter, int kp, int np, int transpose, float *wp)
{
    const size_t n = (size_t)c.d.ntap * kp * np;
    Scope sc(K_TRANSPOSE, c.s);
    hipLaunchKernelGGL(pad_filter_kernel, dim3(capped_grid((n + 255) / 256, 1024)), dim3(256), 0,
                       c.s, filter, c.d.ntap, c.d.Cin, c.d.Cout, kp, np, transpose, wp);
    return hip_ok();
}
// bf16: the B operand of the bf16 deep_gemm_kernel, in (half) the bytes of the fp32 copy
int launch_pack_filter_bf16(const Call<float> &c, const float *filter, int kp, int np, int transpose, float *wp)
{
    const size_t n = (size_t)c.d.ntap * kp * np;
    Scope sc(K_TRANSPOSE, c.s);
    hipLaunchKernelGGL(pack_filter_bf16_kernel, dim3(capped_grid((n + 255) / 256, 1024)), dim3(256), 0,
                       c.s, filter, c.d.ntap, c.d.Cin, c.d.Cout, kp, np, transpose, reinterpret_cast<__bf16 *>(wp));
    return hip_ok();
}

// CI, CO: the padded instantiation; c.d.Cin / c.d.Cout: the layer's real channel counts
template <int CI, int CO>
int deep_forward(const Call<float> &c, const Route &r, const float *input, const float *filter, float *output)
{
    const Dims &d = c.d;
    const DeepScratch ds = carve_deep(d, (size_t)d.B * c.L.pairs_per_cloud, c.L.partials, 0);
    for (int w = 0; w < 2; ++w)
        if (c.order_ok[w]) note_deep_order(c, w);   // this path leaves both orders in place
    TRY(launch_deep_order<false>(c, ds));
    const float *Bm = filter;
    if (c.prec != kPrecF32) {
        TRY(launch_pack_filter_bf16(c, filter, CI, CO, 0, ds.wt));
        Bm = ds.wt;
    } else if (d.Cin != CI || d.Cout != CO) {
        TRY(launch_pad_filter(c, filter, CI, CO, 0, ds.wt));
        Bm = ds.wt;
    }
    TRY((launch_deep_gemm<CI, CO, false>(c, input, Bm, output, ds, d.Cin, d.Cout)));
    // tiles the deep kernels could not take (pair buffer overflow, non-finite rows): generic kernel, flagged tiles
    return launch_forward<float, 0, 0>(c, r.generic_lds, false, input, filter, output, ds.tile_flag);
}

template <int CI, int CO>
int deep_backward(const Call<float> &c, const Route &r, const float *grad_out, const float *input, const float *filter,
                  float *grad_input, float *grad_filter)
{
    const Dims &d = c.d;
    const size_t nw = (size_t)d.ntap * d.Cin * d.Cout;
    const DeepScratch ds = carve_deep(d, (size_t)d.B * c.L.pairs_per_cloud, c.L.partials, 1);
    for (int w = 0; w < 2; ++w)
        if (c.order_ok[w]) note_deep_order(c, w);   // this path leaves both orders in place
    TRY(launch_deep_order<true>(c, ds));
    if (c.prec != kPrecF32) TRY(launch_pack_filter_bf16(c, filter, CO, CI, 1, ds.wt));
    else TRY(launch_pad_filter(c, filter, CO, CI, 1, ds.wt));
    // dX = sum_f' G_f' . W[f']^T  (K = Cout, N = Cin)
    TRY((launch_deep_gemm<CO, CI, true>(c, grad_out, ds.wt, grad_input, ds, d.Cout, d.Cin, ds.gbuf, input)));
    {
        constexpr int NH = deep_dw_parts<CI, CO>();
        const size_t lds = deep_dw_lds(CI, CO, NH, c.prec);
        Scope sc(c.prec != kPrecF32 ? K_DEEP_DW_BF16 : K_DEEP_DW, c.s);
        auto go = [&](auto kern) {
            launch_lds(kern, dim3(kDwItems + 64, NH), dim3(256), lds, c.s, c.L.pts, ds.tap_off, ds.gbuf, input, d.N, d.ntiles, d.ntap,
                       ds.tile_flag, ds.items, ds.tap_total + 64, ds.partials, d.Cin, ds.tap_cmask);
        };
        if (c.prec == kPrecBf16) go(deep_dw_kernel<CI, CO, kPrecBf16>);
        else go(deep_dw_kernel<CI, CO, kPrecF32>);
    }
    TRY(hip_ok());
    // flagged tiles: generic kernel adds into the zeroed rows / into its own grad_filter-shaped buffer
    float *extra = ds.partials + (size_t)(kDwItems + 64) * CI * CO;
    TRY(zero_async(extra, nw * 4, c.s));
    TRY((launch_backward<float, 0, 0>(c, r.generic_lds, grad_out, input, filter, grad_input, extra, ds.tile_flag)));
    {
        Scope sc(K_REDUCE, c.s);
        hipLaunchKernelGGL(deep_reduce_kernel, dim3((unsigned)((d.Cin * d.Cout + 255) / 256), (unsigned)d.ntap), dim3(256), 0,
                           c.s, ds.partials, ds.tap_rng, extra, CI * CO, CO, d.Cin, d.Cout, grad_filter);
    }
    return hip_ok();
}

// The matrix-core path's instantiations, by padded (Cin, Cout)
struct DeepShape {
    int cip, cop;
    int dw_parts;   // deep_dw_kernel's column parts
    int (*forward)(const Call<float> &, const Route &, const float *, const float *, float *);
    int (*backward)(const Call<float> &, const Route &, const float *, const float *, const float *, float *, float *);
};
const DeepShape kDeepShapes[] = {
#define X(ci, co) {ci, co, deep_dw_parts<ci, co>(), deep_forward<ci, co>, deep_backward<ci, co>},
    CONV3P_DEEP_SHAPES(X)
#undef X
};
inline const DeepShape *deep_shape(int cip, int cop)
{
    for (const DeepShape &e : kDeepShapes)
        if (e.cip == cip && e.cop == cop) return &e;
    return nullptr;
}
// padded (Cin, Cout) of a layer the matrix-core path takes (fp32; 129 .. 256 channels on either side: the 128 -> 256,
// 256 -> 256 and 256 -> 128 classes), or false
inline bool deep_class(int elem, int cin, int cout, int &cip, int &cop)
{
    if (elem != 4 || cin < 1 || cout < 1) return false;
    cip = deep_pad(cin);
    cop = deep_pad(cout);
    return cip != 0 && cop != 0 && deep_shape(cip, cop) != nullptr;
}

// ----------------------------------------------------------------------------- the planners
// Can the matrix-core kernels take (cip x cop) blocks of this call?  kreal: real width of deep_gemm's A rows (stage 1
// addresses them by 32-bit offsets)
inline bool deep_fits(const Dims &d, const PlanArgs &a, int cip, int cop, int kreal, bool backward)
{
    if (d.ntap > 64 || deep_order_lds(d.ntap, a.ngroups) > kMaxLds) return false;   // (64-bit tap sets)
    if ((size_t)d.N * (size_t)kreal * 4 > 0xFFFFFFFFull) return false;
    return !backward || deep_dw_lds(cip, cop, deep_shape(cip, cop)->dw_parts, a.prec) <= kMaxLds;
}
// ... every block of a layer of more than 256 channels (wide_forward / wide_backward)
inline bool wide_fits(const Dims &d, const PlanArgs &a, bool backward)
{
    for (int k0 = 0; k0 < d.Cin; k0 += kWideBlk)
        for (int c0 = 0; c0 < d.Cout; c0 += kWideBlk) {
            const int kwp = wide_pad(std::min(kWideBlk, d.Cin - k0)), cwp = wide_pad(std::min(kWideBlk, d.Cout - c0));
            if (!deep_fits(d, a, kwp, cwp, backward ? cwp : kwp, backward)) return false;
        }
    return true;
}

// The forward's route.  Register shapes: forward_kernel while its filter copy fits LDS (fp32 shapes of >= 16 inputs and
// <= 16 outputs: transform + gather where the buffer has room for Z, which is optional); past that fp32 takes the
// matrix-core kernels (up to 64 taps) and fp64 its channel blocks.  Other shapes: fp32 on the matrix-core kernels, in
// blocks above 256 channels; fp64 in channel blocks.  A family whose kernels do not fit, or whose scratch the buffer
// does not have, leaves the call to the generic kernels; strided tensors only the register kernels take.
template <typename T> Route plan_forward(const Dims &d, const Stencil<T> &st, const PlanArgs &a)
{
    constexpr int elem = (int)sizeof(T);
    Route g;
    g.lds = g.generic_lds = forward_lds<T>(st, 0, 0);
    if (g.lds > kMaxLds) g.family = Family::Unsupported;
    Route un = g;
    un.family = Family::Unsupported;
    Route r = g;
    int cip = 0, cop = 0;
    const bool small = small_shape(elem, d.Cin, d.Cout);
    if (small) {
        r.family = Family::Register;
        if constexpr (elem == 4) {
#ifndef CONV3P_DEV_NO_TAP_FORWARD   // developer A/B build
            if (d.Cin >= 16 && d.Cin % 4 == 0 && d.Cout <= 16 && tap_forward_bytes(d) <= a.have) {
                r.tap = true;
                r.lds = tap_gather_lds(st, d.Cout);
                r.scratch = tap_forward_bytes(d);
                return r;
            }
#endif
        }
        r.lds = forward_lds<T>(st, d.Cin, d.Cout);
        if (r.lds <= kMaxLds) return r;
        if (a.strided) return un;
        if (elem == 4 && d.ntap > 64) return g;
    } else if (a.strided) {
        return un;
    }
    r = g;
    if (deep_class(elem, d.Cin, d.Cout, cip, cop)) {
        r.family = deep_fits(d, a, cip, cop, d.Cin, false) ? Family::MatrixCore : g.family;
        r.cip = cip;
        r.cop = cop;
        r.scratch = deep_forward_bytes(d, a.pair_slots);
        r.mandatory = small ? 0 : r.scratch;
    } else if (wide_shape(elem, d.Cin, d.Cout)) {
        r.family = wide_fits(d, a, false) ? Family::Wide : g.family;
        r.scratch = wide_scratch_bytes(d, a.pair_slots, true);
    } else if (elem == 8 && d.Cin >= 1 && d.Cout >= 1) {
        const size_t lds = forward_lds<T>(st, kF64FwdKi, kF64FwdCo);
        if (lds <= kMaxLds) {
            r.family = Family::F64Blocks;
            r.lds = lds;
        }
        r.scratch = f64_blocked_bytes(d);
    }
    if (r.scratch > a.have) r.family = g.family, r.lds = g.lds;
    return r;
}

// The backward's route.  Register shapes: their register kernels while the dense G or the populated rows fit LDS (the fp64
// 36 -> 13 head in three column passes of them after that); past that fp32 takes the matrix-core kernels (up to 64
// taps) and fp64 its channel blocks.  Other shapes as in the forward.  Scratch: at least the grad_filter partials of the
// generic kernels, the fallback of every family (register shapes: one per workgroup, as their register kernels take).
template <typename T> Route plan_backward(const Dims &d, const Stencil<T> &st, const PlanArgs &a)
{
    constexpr int elem = (int)sizeof(T);
    const bool small = small_shape(elem, d.Cin, d.Cout);
    const int grid = (int)grid_of(make_blockmap(d));
    Route g;
    g.lds = g.generic_lds = dense_backward_lds<T>(st, 0, 0);
    if (g.lds > kMaxLds) g.family = Family::Unsupported;
    g.slots = generic_slots(d, elem);
    g.scratch = (size_t)d.ntap * d.Cin * d.Cout * (size_t)(small ? grid : g.slots) * elem;
    if (small) g.slots = std::min(g.slots, grid);
    Route un = g;
    un.family = Family::Unsupported;
    Route r = g;
    int cip = 0, cop = 0;
    if (small) {
        const size_t dense = dense_backward_lds<T>(st, d.Cin, d.Cout);
        size_t slds = 0;
        int cap = 0;
#ifndef CONV3P_DEV_DENSE_BACKWARD   // developer A/B build: always the dense-G kernel
        if (elem == 4) cap = sparse_cap<T>(st, d.Cin, d.Cout, slds);
#endif
        if (dense <= kMaxLds || cap > 0) {
            r.family = Family::Register;
            r.lds = dense;
            r.slots = grid;
            r.self_reduces = false;
            // Populated rows: layers of >= 16 inputs, and filters whose dense G does not fit, always.  Narrow dilated
            // layers: on the caller's SPARSE hint alone; on neither hint the regime word picks one of the two kernels on
            // the device; on the DENSE hint the dense G.
            if (cap > 0 && !(d.Cin < 16 && a.dense_hint && dense <= kMaxLds)) {
                r.cap = cap;
                r.sparse_lds = slds;
                r.regime = d.Cin < 16 && !a.sparse_hint && dense <= kMaxLds;
            }
            return r;
        }
        // (fp64 36 -> 13: the dense G of 5 output channels fits up to 33 taps)
        if (elem == 8 && d.Cin == 36 && d.Cout == 13 && dense_backward_lds<T>(st, 36, 5) <= kMaxLds) {
            r.family = Family::Split36x13;
            r.lds = dense_backward_lds<T>(st, 36, 5);
            r.lds4 = dense_backward_lds<T>(st, 36, 4);
            return r;
        }
        if (a.strided) return un;
        if (elem == 4 && d.ntap > 64) return g;
    } else if (a.strided) {
        return un;
    }
    if (deep_class(elem, d.Cin, d.Cout, cip, cop)) {
        r.family = deep_fits(d, a, cip, cop, d.Cout, true) ? Family::MatrixCore : g.family;
        r.cip = cip;
        r.cop = cop;
        r.scratch = std::max(g.scratch, deep_scratch_bytes(d, a.pair_slots));
    } else if (wide_shape(elem, d.Cin, d.Cout)) {
        r.family = wide_fits(d, a, true) ? Family::Wide : g.family;
        r.scratch = std::max(g.scratch, wide_scratch_bytes(d, a.pair_slots));
    } else if (elem == 8 && d.Cin >= 1 && d.Cout >= 1) {
        // blocks of kF64BwdCo output channels, else 4, else 2: the widest whose dense G fits (16 x 8 up to 28 taps, 16 x 4
        // up to 57, 16 x 2 up to 115)
        for (int co : {kF64BwdCo, 4, 2})
            if (co <= kF64BwdCo && dense_backward_lds<T>(st, kF64BwdKi, co) <= kMaxLds) {
                r.family = Family::F64Blocks;
                r.co = co;
                r.lds = dense_backward_lds<T>(st, kF64BwdKi, co);
                break;
            }
        r.scratch = std::max(g.scratch, f64_blocked_bytes(d));
    }
    if (r.scratch > a.have) r.family = g.family, r.lds = g.lds;
    return r;
}

// Workspace sizes: the planners on the undilated stencil of the call's extents -- what the workspace query (no stride
// argument) and the call itself both know -- with no hints and room for everything.  ppp: pair slots per point of the
// buffer (a cache may be configured with fewer than the default).  (A dilation large enough to tip a register shape past
// its fit on its own finds the scratch of the next family only in a cache: a stateless call takes the generic kernels.)
size_t backward_scratch_bytes(const Dims &d, int elem, int ppp = kDefaultPairsPerPoint)
{
    PlanArgs a;
    a.pair_slots = (size_t)d.B * d.N * (size_t)ppp;
    return elem == 4 ? plan_backward<float>(d, undilated_stencil<float>(d), a).scratch
                     : plan_backward<double>(d, undilated_stencil<double>(d), a).scratch;
}
// mandatory_only: what the forward cannot run without (a persistent cache sized for narrower layers is not refused for
// the optional rest)
size_t forward_scratch_bytes(const Dims &d, int elem, int ppp = kDefaultPairsPerPoint, bool mandatory_only = false)
{
    PlanArgs a;
    a.pair_slots = (size_t)d.B * d.N * (size_t)ppp;
    const Route r = elem == 4 ? plan_forward<float>(d, undilated_stencil<float>(d), a)
                              : plan_forward<double>(d, undilated_stencil<double>(d), a);
    return mandatory_only ? r.mandatory : r.scratch;
}

// What a call's route depends on besides its shape and stencil.  scratch: bytes of per-call scratch of a stateless call
template <typename T> PlanArgs plan_args(const Dims &d, const Where &wh, bool strided, size_t scratch)
{
    const Layout<T> L = carve<T>(d.B, d.N, d.ntiles, wh.persistent ? wh.ntap_max : d.ntap, 1, wh.ppp, 0, nullptr);
    PlanArgs a;
    a.strided = strided;
    a.sparse_hint = wh.persistent && (wh.flags & CONV3P_CACHE_SPARSE_NEIGHBOURHOODS) != 0;
    a.dense_hint = wh.persistent && !a.sparse_hint && (wh.flags & CONV3P_CACHE_DENSE_NEIGHBOURHOODS) != 0;
    a.prec = call_prec(wh);
    a.pair_slots = (size_t)d.B * L.pairs_per_cloud;
    a.ngroups = L.ngroups;
    a.have = wh.persistent ? wh.scratch_cap : scratch;
    return a;
}

size_t cache_scratch_bytes(int elem, int B, int N, int max_taps, int max_Cin, int max_Cout, int ppp)
{
    // the largest need of any (Cin <= max_Cin, Cout <= max_Cout, taps <= max_taps) call: the routes of the largest shape
    // and of the register-path shapes, both passes; the matrix-core classes the smaller fp32 shapes pad to; and any fp64
    // shape outside the register-path list (the blocked path's scratch does not depend on the channels)
    const int ntiles = (N + kTile - 1) / kTile;
    size_t b = 0;
    auto take = [&](int cin, int cout) {
        const Dims d{B, N, cin, cout, 1, 1, max_taps, max_taps, ntiles};
        b = std::max({b, backward_scratch_bytes(d, elem, ppp), forward_scratch_bytes(d, elem, ppp)});
    };
    take(max_Cin, max_Cout);
    for (const RegisterShape<float> &e : kRegisterShapes<float>)
        if (e.cin <= max_Cin && e.cout <= max_Cout) take(e.cin, e.cout);
    for (const DeepShape &e : kDeepShapes)
        if (elem == 4 && max_Cin > 0 && max_Cout > 0 && e.cip <= deep_pad(max_Cin) && e.cop <= deep_pad(max_Cout))
            b = std::max(b, deep_scratch_bytes(Dims{B, N, e.cip, e.cop, 1, 1, max_taps, max_taps, ntiles}, (size_t)B * N * (size_t)ppp));
    if (elem == 8) b = std::max(b, f64_blocked_bytes(Dims{B, N, max_Cin, max_Cout, 1, 1, max_taps, max_taps, ntiles}));
    return b;
}

}  // namespace

extern "C" {

size_t conv3p_workspace_bytes(int pass, int elem_bytes, int B, int N, int Cin, int Cout, int fz, int fy,
                              int fx)
{
    if (pass < 0 || pass > 2 || (elem_bytes != 4 && elem_bytes != 8)) return 0;
    Dims d{B, N, Cin, Cout, fz, fy, fx, 0, 0};
    const int32_t one[3] = {1, 1, 1};
    if (check(d, one, 1.0, pass != CONV3P_PASS_NEIGHBOR_COUNT) != CONV3P_OK) return 0;
    const int ppp = pass == CONV3P_PASS_NEIGHBOR_COUNT ? 0 : kDefaultPairsPerPoint;
    const size_t scratch = pass == CONV3P_PASS_BACKWARD ? backward_scratch_bytes(d, elem_bytes)
                           : pass == CONV3P_PASS_FORWARD ? forward_scratch_bytes(d, elem_bytes) : 0;
    const size_t b = layout_bytes(elem_bytes, B, N, d.ntap, 1, ppp, scratch);
    return b ? b : kAlign;
}

}  // extern "C"
