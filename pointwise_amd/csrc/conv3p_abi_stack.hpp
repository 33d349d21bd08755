// conv3p_abi_stack.hpp -- the models' layer stack in one call: geometry prefetch, the per-layer passes, the fused stack
// launches.  Included by conv3p_abi.hip after the single-layer calls it composes.
namespace {

// ----------------------------------------------------------------------------- the models' stack in one call
bool stack_desc_ok(const conv3p_stack_desc *sd)
{
    if (!sd || sd->n_hidden < 1 || sd->n_hidden > CONV3P_STACK_MAX_LAYERS || sd->in_channels < 1 || sd->hidden < 1 ||
        sd->num_class < 0 || sd->fz < 1 || sd->fy < 1 || sd->fx < 1)
        return false;
    for (int l = 0; l < sd->n_hidden + (sd->num_class > 0 ? 1 : 0); ++l)
        for (int a = 0; a < 3; ++a)
            if (sd->strides[l][a] < 1) return false;
    return true;
}
inline int stack_layers(const conv3p_stack_desc *sd) { return sd->n_hidden + (sd->num_class > 0 ? 1 : 0); }

// One stack call, described once.  Hidden layer l maps its Cin channels (in_channels for l == 0, else hidden) to `hidden`,
// from `input` / column block l - 1 of `concat` into column block l; the head (l == n_hidden, when num_class > 0) maps
// the whole concat row to num_class channels.
template <typename T> struct StackCall {
    const conv3p_stack_desc *sd;
    int B, N;
    void *cache;
    size_t cache_bytes;
    const conv3p_cache_config *cfg;

    int layers() const { return stack_layers(sd); }
    size_t rows() const { return (size_t)B * N; }
    int row() const { return sd->n_hidden * sd->hidden; }               // channels of a concat row
    size_t col(int l) const { return (size_t)sd->hidden * l; }          // first column of hidden layer l's block in it
    bool head(int l) const { return l == sd->n_hidden; }
    int cin(int l) const { return head(l) ? row() : l == 0 ? sd->in_channels : sd->hidden; }
    int cout(int l) const { return head(l) ? sd->num_class : sd->hidden; }
    // layer l's input and output inside the call's tensors, and the row strides they have there
    const T *in(int l, const T *input, const T *concat) const { return head(l) ? concat : l == 0 ? input : concat + col(l - 1); }
    T *out(int l, T *concat, T *head_out) const { return head(l) ? head_out : concat + col(l); }
    int ld_in(int l) const { return l == 0 ? sd->in_channels : row(); }
    int ld_out(int l) const { return head(l) ? sd->num_class : row(); }
    Dims dims(int l) const
    {
        return Dims{B, N, cin(l), cout(l), sd->fz, sd->fy, sd->fx, sd->fz * sd->fy * sd->fx, (N + kTile - 1) / kTile};
    }
    // where the layers' calls live: the stack's cache, under the CONV3P_CACHE_* flags of one call
    Where where(int flags) const { return persistent((int)sizeof(T), B, N, cache, cache_bytes, cfg, flags); }
};

// geometry of every layer on `s`, ordered after `after`; one event per layer in the cache's host record
template <typename T>
int stack_geometry(const StackCall<T> &x, const T *points, T voxel, hipStream_t s, hipStream_t after, bool differs, bool one_launch)
{
    const conv3p_stack_desc *sd = x.sd;
    const int nl = x.layers();
    std::vector<hipEvent_t> ev;
    {
        const CacheRef h = find_or_create_cache(x.cache);
        while ((int)h->ready.size() < nl + 1) {
            hipEvent_t e = nullptr;
            if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return CONV3P_ERR_LAUNCH;
            h->ready.push_back(e);
        }
        ev = h->ready;
    }
    if (differs) {   // `points` is produced on another stream
        if (hipEventRecord(ev[nl], after) != hipSuccess || hipStreamWaitEvent(s, ev[nl], 0) != hipSuccess)
            return CONV3P_ERR_LAUNCH;
    }
    // one_launch (prefetch of the NEXT batch: nobody waits for the first layer's lists): all strides in ONE search
    // launch, whose light tiles fill in behind another stride's heavy ones (0.534 -> 0.527 ms/step on cfg2);
    // otherwise one launch and one event per layer, so that layer 0 can start as soon as its lists exist
#ifdef CONV3P_DEV_STACK_NO_MULTI   // developer A/B build only (-DCONV3P_DEV_STACK_NO_MULTI)
    const bool no_batch = true;
#else
    const bool no_batch = false;
#endif
    if (one_launch && !no_batch && nl <= kMaxJobs) {
        int32_t strides[kMaxJobs * 3];
        int k = 0;
        for (int l = 0; l < nl; ++l) {
            bool dup = false;
            for (int m = 0; m < k; ++m)
                dup |= strides[3 * m] == sd->strides[l][0] && strides[3 * m + 1] == sd->strides[l][1] && strides[3 * m + 2] == sd->strides[l][2];
            if (!dup) { strides[3 * k] = sd->strides[l][0]; strides[3 * k + 1] = sd->strides[l][1]; strides[3 * k + 2] = sd->strides[l][2]; ++k; }
        }
        TRY(prepare_multi_impl<T>(points, strides, k, voxel, x.B, x.N, sd->fz, sd->fy, sd->fx, x.where(0), s));
        for (int l = 0; l < nl; ++l)
            if (hipEventRecord(ev[l], s) != hipSuccess) return CONV3P_ERR_LAUNCH;
    } else
    for (int l = 0; l < nl; ++l) {
        const int flags = (l > 0 ? CONV3P_CACHE_POINTS_UNCHANGED : 0) | hints(x.cfg);
        TRY(prepare_impl<T>(points, sd->strides[l], voxel, x.B, x.N, sd->fz, sd->fy, sd->fx, x.where(flags), s));
        if (hipEventRecord(ev[l], s) != hipSuccess) return CONV3P_ERR_LAUNCH;
    }
    const CacheRef h = find_or_create_cache(x.cache);
    h->pending_points = points;
    h->pending_layers = nl;
    return CONV3P_OK;
}


// ----------------------------------------------------------------------------- fused stack launches (conv3p_stack_fused.hpp)
// Per device, once: the placement census (is workgroup b of a 2048-workgroup grid on the same XCC for every b of one
// residue mod 8?) and the CU count.  One host synchronisation, at the first stack call of the process.
struct FusedDevice {
    bool ok = false;
    uint32_t xcc_of[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int cus = 0;
};
const FusedDevice &fused_device()
{
    static std::mutex mu;
    static std::map<int, FusedDevice> devs;
    std::lock_guard<std::mutex> lk(mu);
    int dev = 0;
    (void)hipGetDevice(&dev);
    auto it = devs.find(dev);
    if (it != devs.end()) return it->second;
    FusedDevice fd;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) == hipSuccess) {
        fd.cus = prop.multiProcessorCount;
        constexpr int kCensus = 2048;
        uint32_t *d = nullptr;
        std::vector<uint32_t> h(kCensus, 0xFFFFFFFFu);
        if (hipMalloc(&d, sizeof(uint32_t) * kCensus) == hipSuccess) {
            hipLaunchKernelGGL(xcc_census_kernel, dim3(kCensus), dim3(256), 0, nullptr, d);
            if (hipMemcpy(h.data(), d, sizeof(uint32_t) * kCensus, hipMemcpyDeviceToHost) == hipSuccess) {
                fd.ok = true;
                for (int i = 0; i < 8; ++i) fd.xcc_of[i] = h[i];
                for (int b = 0; b < kCensus; ++b) fd.ok &= h[b] == fd.xcc_of[b & 7];
            }
            (void)hipFree(d);
        }
        (void)hipGetLastError();
    }
    return devs.emplace(dev, fd).first->second;
}
// workgroups of `kern` (256 threads, `lds` bytes of dynamic LDS) the device holds at once
int fused_capacity(const void *kern, size_t lds, int cus)
{
    static std::mutex mu;
    static std::map<std::pair<const void *, size_t>, int> memo;
    std::lock_guard<std::mutex> lk(mu);
    auto key = std::make_pair(kern, lds);
    auto it = memo.find(key);
    if (it != memo.end()) return it->second * cus;
    int nb = 0;
    if (hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess ||
        hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kern, 256, lds) != hipSuccess)
        nb = 0;
    (void)hipGetLastError();
    memo[key] = nb;
    return nb * cus;
}
// the cache's arrival counters (created at the first fused launch on it; zero-filled once, never reset: the host tracks
// their value)
uint32_t *fused_sync(void *cache, int B, int kind, uint32_t arrivals, uint32_t &base, int *status)
{
    const CacheRef ref = find_or_create_cache(cache);
    CacheHost &h = *ref;
    *status = CONV3P_ERR_LAUNCH;
    // an earlier fused launch on this cache reported an error (a barrier wait that gave up: e.g. two fused launches on one
    // device at the same time, each holding the slots the other's tiles wait for; or a cloud whose tiles did not share an
    // XCC): its results were wrong -- fail loudly now, once
    if (h.host_err != nullptr && *reinterpret_cast<volatile uint32_t *>(h.host_err) != 0u) {
        *reinterpret_cast<volatile uint32_t *>(h.host_err) = 0u;
        return nullptr;
    }
    if (h.sync != nullptr && h.sync_clouds < B) {
        (void)hipFree(h.sync);   // (synchronises: nothing can still be using it)
        h.sync = nullptr;
    }
    if (h.sync == nullptr) {
        const size_t words = (size_t)2 * B * kSyncLineWords;
        if (h.host_err == nullptr) {
            if (hipHostMalloc(reinterpret_cast<void **>(&h.host_err), sizeof(uint32_t), hipHostMallocMapped) != hipSuccess) {
                (void)hipGetLastError();
                h.host_err = nullptr;
                return nullptr;
            }
            *h.host_err = 0u;
        }
        void *dev_err = nullptr;
        std::vector<uint32_t> init(words, 0u);
        if (hipHostGetDevicePointer(&dev_err, h.host_err, 0) != hipSuccess) dev_err = nullptr;
        for (size_t l = 0; l < words; l += kSyncLineWords) {   // words 4-5 of every line: where an error is also reported
            init[l + 4] = (uint32_t)(reinterpret_cast<uintptr_t>(dev_err) & 0xFFFFFFFFu);
            init[l + 5] = (uint32_t)((unsigned long long)reinterpret_cast<uintptr_t>(dev_err) >> 32);
        }
        if (hipMalloc(&h.sync, words * sizeof(uint32_t)) != hipSuccess ||
            hipMemcpy(h.sync, init.data(), words * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipGetLastError();
            h.sync = nullptr;
            return nullptr;
        }
        h.sync_clouds = B;
        h.sync_base[0] = h.sync_base[1] = 0u;
    }
    base = h.sync_base[kind];
    h.sync_base[kind] += arrivals;
    h.fused_launches[kind] += 1u;
    *status = CONV3P_OK;
    return h.sync + (size_t)kind * h.sync_clouds * kSyncLineWords;
}

// Can the hidden layers of this stack run as fused launches on this cache?  Decided from the description alone, BEFORE any
// call touches the cache's host record.  (fp32; in_channels 3 or 9 -> 9 -> 9 ...; odd dilated extents; one search group;
// enough slots for the strides not to evict each other; the whole grid resident at once; census passed.)
template <typename T> bool stack_fusable(const StackCall<T> &x, T voxel, size_t scratch_cap_needed, size_t scratch_cap)
{
    if constexpr (sizeof(T) != 4) {
        return false;
    } else {
        const conv3p_stack_desc *sd = x.sd;
        const conv3p_cache_config *cfg = x.cfg;
        if ((cfg->flags & CONV3P_CACHE_FUSED_STACK) == 0) return false;   // opt-in, one bit per pass (include/conv3p.h; the callers test theirs)
        if (sd->hidden != 9 || (sd->in_channels != 3 && sd->in_channels != 9) || sd->n_hidden < 2 || sd->n_hidden > kStackMaxFused) return false;
        if (sd->fz * sd->fy * sd->fx > 32 || x.N <= kTile || x.N > kFusedMaxPoints) return false;
        if (scratch_cap_needed > scratch_cap) return false;
        int distinct = 0;
        for (int l = 0; l < x.layers(); ++l) {
            bool dup = false;
            for (int m = 0; m < l; ++m) dup |= sd->strides[m][0] == sd->strides[l][0] && sd->strides[m][1] == sd->strides[l][1] && sd->strides[m][2] == sd->strides[l][2];
            distinct += dup ? 0 : 1;
        }
        if (cfg->slots < distinct) return false;
        if (carve<T>(x.B, x.N, x.dims(0).ntiles, cfg->max_taps, 1, pairs_per_point(cfg), 0, nullptr).ngroups != 1) return false;
        for (int l = 0; l < sd->n_hidden; ++l) {
            Dims d = x.dims(l);
            if (check(d, sd->strides[l], (double)voxel, true) != CONV3P_OK) return false;
            if (make_stencil<T>(d, sd->strides[l], voxel).window) return false;
        }
        return fused_device().ok;
    }
}

// The fused forward's hand-off buffers in the cache's scratch: hand[l], l < n_hidden - 1, the dense copy of hidden layer
// l's activation that layer l + 1 gathers (a buffer of its own: no stale L1 line)
template <typename T> size_t carve_handoff(const conv3p_stack_desc *sd, size_t rows, void *base, T **hand)
{
    Carver cv(base);
    for (int l = 0; l + 1 < sd->n_hidden; ++l) hand[l] = cv.take<T>(rows * (size_t)sd->hidden);
    return cv.bytes();
}

// forward of the hidden layers in ONE launch.  CONV3P_ERR_UNSUPPORTED (nothing enqueued, nothing recorded): take the per-layer path.
template <typename T>
int stack_forward_fused(const StackCall<T> &x, const T *points, const T *input, const T *const *filters, T voxel, T *concat,
                        hipStream_t s, bool geometry_enqueued)
{
    if constexpr (sizeof(T) != 4) {
        return CONV3P_ERR_UNSUPPORTED;
    } else {
        const conv3p_stack_desc *sd = x.sd;
        const int nh = sd->n_hidden, H = sd->hidden;
        T *hand[CONV3P_STACK_MAX_LAYERS];
        const size_t handoff = carve_handoff<T>(sd, x.rows(), nullptr, hand);
        if ((x.cfg->flags & CONV3P_CACHE_FUSED_FORWARD) == 0 || !stack_fusable<T>(x, voxel, handoff, x.where(0).scratch_cap))
            return CONV3P_ERR_UNSUPPORTED;
        const FusedDevice &fd = fused_device();
        const BlockMap bm = make_blockmap(x.dims(0));
        size_t lds = 0;
        for (int l = 0; l < nh; ++l) {   // (the layers' register routes: their forward_kernel's LDS)
            const Dims d = x.dims(l);
            PlanArgs pa;
            pa.strided = true;
            const Route r = plan_forward<T>(d, make_stencil<T>(d, sd->strides[l], voxel), pa);
            if (r.family != Family::Register) return CONV3P_ERR_UNSUPPORTED;
            lds = std::max(lds, r.lds);
        }
        const void *kern = sd->in_channels == 3 ? reinterpret_cast<const void *>(stack_forward_kernel<T, 3, 9>)
                                                : reinterpret_cast<const void *>(stack_forward_kernel<T, 9, 9>);
        if (lds > kMaxLds || (int)grid_of(bm) > fused_capacity(kern, lds, fd.cus)) return CONV3P_ERR_UNSUPPORTED;
        for (int l = 0; l < nh; ++l)
            if (!filters[l]) return CONV3P_ERR_INVALID_ARGUMENT;
        // from here on the cache's host record is touched exactly as the per-layer calls would touch it
        StackFwdArgs<T> a{};
        for (int l = 0; l < nh; ++l) {
            const int flags = ((l > 0 || geometry_enqueued) ? CONV3P_CACHE_POINTS_UNCHANGED : 0) | hints(x.cfg);
            const Dims d = x.dims(l);
            Call<T> c;
            TRY(begin_call<T>(c, d, sd->strides[l], voxel, handoff, x.where(flags), s));
            TRY(run_geometry<T>(points, c));
            const auto &S = c.L.slot[c.slot];
            StackFwdLayer<T> &L = a.layer[l];
            L.st = c.st;
            L.count = S.count; L.tcount = S.tcount; L.pairs = S.pairs; L.segs = S.segs; L.qsegs = S.qsegs;
            (void)carve_handoff<T>(sd, x.rows(), c.L.partials, hand);
            L.input = l == 0 ? input : hand[l - 1];   // (the dense copy, not the concat's column block)
            L.filter = filters[l];
            L.output = x.out(l, concat, nullptr);
            L.out2 = l + 1 < nh ? hand[l] : nullptr;
            L.ld_out2 = H;
            L.ld = RowLd{d.Cin, x.ld_out(l), H, d.Cin, d.Cin};
            if (l == 0) {
                a.pts = c.L.pts; a.boxes = c.L.boxes; a.cmin = nullptr;
            }
        }
        a.N = x.N; a.ntiles = x.dims(0).ntiles; a.nl = nh; a.bm = bm;
        int srcs = CONV3P_OK;
        a.sync = fused_sync(x.cache, x.B, 0, (uint32_t)(a.ntiles * (nh - 1)), a.base, &srcs);
        if (a.sync == nullptr) return srcs;
        Scope sc(K_FORWARD, s);
        // A plain launch: the kernel's dynamic-LDS limit is the one fused_capacity() set for this (kernel, lds) when it first
        // measured it, not re-set here (ADVICE.md reports this; changing it is a behaviour fix of its own).
        if (sd->in_channels == 3) hipLaunchKernelGGL((stack_forward_kernel<T, 3, 9>), dim3(grid_of(bm)), dim3(256), lds, s, a);
        else hipLaunchKernelGGL((stack_forward_kernel<T, 9, 9>), dim3(grid_of(bm)), dim3(256), lds, s, a);
        return hip_ok();
    }
}

template <typename T>
int stack_prefetch_impl(const conv3p_stack_desc *sd, const T *points, T voxel, int B, int N, void *cache,
                        size_t cache_bytes, const conv3p_cache_config *cfg, void *stream, void *after_stream)
{
    if (!stack_desc_ok(sd) || !cache_cfg_ok(cfg)) return CONV3P_ERR_INVALID_ARGUMENT;
    if ((size_t)B * N == 0) return CONV3P_OK;
    if (!points) return CONV3P_ERR_INVALID_ARGUMENT;
    const StackCall<T> x{sd, B, N, cache, cache_bytes, cfg};
    return stack_geometry<T>(x, points, voxel, static_cast<hipStream_t>(stream), static_cast<hipStream_t>(after_stream),
                             after_stream != stream, /*one_launch=*/true);
}

template <typename T>
int stack_forward_impl(const conv3p_stack_desc *sd, const T *points, const T *input, const T *const *filters, T voxel,
                       int B, int N, T *concat, T *head_out, void *cache, size_t cache_bytes,
                       const conv3p_cache_config *cfg, void *stream, void *side_stream)
{
    if (!stack_desc_ok(sd) || !cache_cfg_ok(cfg) || !filters) return CONV3P_ERR_INVALID_ARGUMENT;
    if ((size_t)B * N == 0) return CONV3P_OK;
    if (!points || !input || !concat || (sd->num_class > 0 && !head_out)) return CONV3P_ERR_INVALID_ARGUMENT;
    const StackCall<T> x{sd, B, N, cache, cache_bytes, cfg};
    const int nl = x.layers();
    hipStream_t main = static_cast<hipStream_t>(stream);
    // geometry: already enqueued by conv3p_stack_prefetch_* for these points, or enqueued now on the side stream
    // (each layer's search then runs while the previous layers accumulate), or built inline by the op calls
    bool events = false, prefetched = false;
    std::vector<hipEvent_t> ev;   // with `events`: the cache's per-layer events
    if (const CacheRef h = find_cache(cache)) {
        if (h->pending_points == points && h->pending_layers == nl) {
            events = prefetched = true;
            ev = h->ready;
        }
        h->pending_points = nullptr;
    }
    if (!events && side_stream != nullptr && side_stream != stream) {
        TRY(stack_geometry<T>(x, points, voxel, static_cast<hipStream_t>(side_stream), main, true, /*one_launch=*/false));
        const CacheRef h = find_or_create_cache(cache);
        h->pending_points = nullptr;
        ev = h->ready;
        events = true;
    }
    // prefetched geometry (normally finished long ago, under the previous batch's backward): ONE wait on the last
    // layer's event covers them all; geometry enqueued just now: per-layer waits, so that layer 0 starts early
    if (prefetched && hipStreamWaitEvent(main, ev[nl - 1], 0) != hipSuccess) return CONV3P_ERR_LAUNCH;
    // the hidden layers as ONE launch (conv3p_stack_fused.hpp) where the stack, the cache and the device allow it
    int first = 0;
    {
        T *hand[CONV3P_STACK_MAX_LAYERS];
        if ((cfg->flags & CONV3P_CACHE_FUSED_FORWARD) != 0 &&
            stack_fusable<T>(x, voxel, carve_handoff<T>(sd, x.rows(), nullptr, hand), x.where(0).scratch_cap)) {
            if (events && !prefetched && hipStreamWaitEvent(main, ev[sd->n_hidden - 1], 0) != hipSuccess) return CONV3P_ERR_LAUNCH;
            const int rc = stack_forward_fused<T>(x, points, input, filters, voxel, concat, main, events);
            if (rc == CONV3P_OK) first = sd->n_hidden;
            else if (rc != CONV3P_ERR_UNSUPPORTED) return rc;
        }
    }
    for (int l = first; l < nl; ++l) {
        if (events && !prefetched && hipStreamWaitEvent(main, ev[l], 0) != hipSuccess) return CONV3P_ERR_LAUNCH;
        const int flags = ((l > 0 || events) ? CONV3P_CACHE_POINTS_UNCHANGED : 0) | hints(cfg);   // the first call of a step re-validates
        const RowLd ld{x.ld_in(l), x.ld_out(l), 0, 0, 0};
        const Where wh = x.where(flags);
        if (!filters[l]) return CONV3P_ERR_INVALID_ARGUMENT;
        TRY(forward_impl<T>(points, x.in(l, input, concat), filters[l], sd->strides[l], voxel, B, N, x.cin(l), x.cout(l), sd->fz,
                            sd->fy, sd->fx, x.out(l, concat, head_out), wh, stream, /*act=*/true, &ld));
    }
    return CONV3P_OK;
}

// values of layer l's grad_filter partials (one copy per backward workgroup)
template <typename T> size_t stack_region_elems(const StackCall<T> &x, int l)
{
    const Dims d = x.dims(l);
    return (size_t)d.ntap * d.Cin * d.Cout * (size_t)grid_of(make_blockmap(d));
}

// The stack backward's scratch.
template <typename T> struct StackScratch {
    T *ga, *gb;                                  // two ping-pong gradient buffers
    T *dconcat;                                  // the head's gradient w.r.t. the concat
    T *region[CONV3P_STACK_MAX_LAYERS + 1];      // every layer's grad_filter partials
    T *G[CONV3P_STACK_MAX_LAYERS];               // the fused launch's gradient hand-off buffers, one per hidden layer
                                                 // (conv3p_stack_fused.hpp: every layer's rows in a buffer of their own)
};
template <typename T> size_t carve_stack(const StackCall<T> &x, void *base, StackScratch<T> &w)
{
    const conv3p_stack_desc *sd = x.sd;
    const size_t wide = (size_t)(sd->hidden > sd->num_class ? sd->hidden : sd->num_class);
    Carver cv(base);
    w.ga = cv.take<T>(x.rows() * wide);
    w.gb = cv.take<T>(x.rows() * wide);
    w.dconcat = cv.take<T>(x.rows() * (size_t)x.row());
    for (int l = 0; l < x.layers(); ++l) w.region[l] = cv.take<T>(stack_region_elems(x, l));
    for (int l = 0; l < sd->n_hidden; ++l) w.G[l] = cv.take<T>(x.rows() * (size_t)sd->hidden);
    return cv.bytes();
}
// (the scratch does not depend on the cache)
template <typename T> size_t stack_scratch_bytes(const conv3p_stack_desc *sd, int B, int N)
{
    StackScratch<T> w;
    return carve_stack<T>(StackCall<T>{sd, B, N, nullptr, 0, nullptr}, nullptr, w);
}


// backward of the hidden layers nh-1 .. 1 in ONE launch (populated-rows kernel; needs the caller's SPARSE hint: the fused
// launch cannot pick the kernel per layer on the device).  G[l] = gradient w.r.t. the conv output of hidden layer l, dense
// [B][N][H], each in a buffer of its own.  CONV3P_ERR_UNSUPPORTED (nothing enqueued): take the per-layer path.
template <typename T>
int stack_backward_fused(const StackCall<T> &x, const T *points, const T *const *filters, T voxel, const T *concat, const T *ext,
                         int ld_ext, T *const *G, DeferredReduce<T> *red, T *const *grad_filters, hipStream_t s)
{
    if constexpr (sizeof(T) != 4) {
        return CONV3P_ERR_UNSUPPORTED;
    } else {
        const conv3p_stack_desc *sd = x.sd;
        const conv3p_cache_config *cfg = x.cfg;
        const int nh = sd->n_hidden, H = sd->hidden;
        if ((cfg->flags & CONV3P_CACHE_SPARSE_NEIGHBOURHOODS) == 0 || (cfg->flags & CONV3P_CACHE_FUSED_BACKWARD) == 0) return CONV3P_ERR_UNSUPPORTED;
        if (!stack_fusable<T>(x, voxel, 0, x.where(0).scratch_cap)) return CONV3P_ERR_UNSUPPORTED;
        const FusedDevice &fd = fused_device();
        const Dims d = x.dims(1);   // (the hidden layers past the first share one shape)
        const BlockMap bm = make_blockmap(d);
        size_t lds = 0;
        int caps[kStackMaxFused];
        for (int l = nh - 1; l >= 1; --l) {   // (the layers' register routes on the SPARSE hint: their populated rows)
            PlanArgs pa;
            pa.strided = pa.sparse_hint = true;
            const Route r = plan_backward<T>(d, make_stencil<T>(d, sd->strides[l], voxel), pa);
            caps[l] = r.family == Family::Register ? r.cap : 0;
            if (caps[l] <= 0 || r.sparse_lds > 40960) return CONV3P_ERR_UNSUPPORTED;   // (undilated layers: dense G; four workgroups per CU)
            lds = std::max(lds, r.sparse_lds);
        }
        const void *kern = reinterpret_cast<const void *>(stack_backward_kernel<T, 9>);
        if ((int)grid_of(bm) > fused_capacity(kern, lds, fd.cus)) return CONV3P_ERR_UNSUPPORTED;
        StackBwdArgs<T> a{};
        int k = 0;
        for (int l = nh - 1; l >= 1; --l, ++k) {
            const Where wh = x.where(CONV3P_CACHE_POINTS_UNCHANGED | hints(cfg));
            Call<T> c;
            TRY(begin_call<T>(c, d, sd->strides[l], voxel, backward_scratch_bytes(d, (int)sizeof(T), wh.ppp), wh, s));
            TRY(run_geometry<T>(points, c));
            const auto &S = c.L.slot[c.slot];
            StackBwdLayer<T> &L = a.layer[k];
            L.st = c.st;
            L.count = S.count; L.pairs = S.pairs; L.segs = S.segs; L.qsegs = S.qsegs; L.qbm = S.qbm;
            L.grad_out = G[l];
            L.input = x.in(l, nullptr, concat);
            L.filter = filters[l];
            L.addend = ext + x.col(l - 1);
            L.grad_input = G[l - 1];
            L.partials = red[l].region;
            L.ld = RowLd{x.ld_in(l), H, H, H, ld_ext};
            L.cap = caps[l];
            red[l].job = ReduceJob<T>{red[l].region, grad_filters[l], (int)grid_of(bm), (unsigned)((size_t)d.ntap * H * H)};
            if (k == 0) {
                a.pts = c.L.pts; a.boxes = c.L.boxes; a.cmin = nullptr;
            }
        }
        a.N = x.N; a.ntiles = d.ntiles; a.nl = k; a.bm = bm;
        a.nw = (size_t)d.ntap * H * H;
        a.top_act = concat + x.col(nh - 1);
        a.top_ext = ext + x.col(nh - 1);
        a.top_g = G[nh - 1];
        a.ld_act = x.row();
        a.ld_ext = ld_ext;
        int srcs = CONV3P_OK;
        a.sync = fused_sync(x.cache, x.B, 1, (uint32_t)(d.ntiles * k), a.base, &srcs);
        if (a.sync == nullptr) return srcs;
        Scope sc(K_BACKWARD, s);
        launch_lds(stack_backward_kernel<T, 9>, dim3(grid_of(bm)), dim3(256), lds, s, a);
        return hip_ok();
    }
}

// The hidden layers past the first read and write column blocks of `concat` (row strides), which only the register kernels
// take: each must plan to them.  Checked before anything is launched, so that a description the backward cannot serve
// (fp64 9 -> 9 past 28 taps, hidden widths outside the list) returns CONV3P_ERR_UNSUPPORTED with every output untouched.
template <typename T> int stack_backward_fits(const StackCall<T> &x, T voxel)
{
    for (int l = 1; l < x.sd->n_hidden; ++l) {
        Dims d = x.dims(l);
        TRY(check(d, x.sd->strides[l], (double)voxel, true));
        PlanArgs pa;
        pa.strided = true;
        if (plan_backward<T>(d, make_stencil<T>(d, x.sd->strides[l], voxel), pa).family != Family::Register)
            return CONV3P_ERR_UNSUPPORTED;
    }
    return CONV3P_OK;
}

template <typename T>
int stack_backward_impl(const conv3p_stack_desc *sd, const T *points, const T *input, const T *const *filters, T voxel,
                        int B, int N, const T *concat, const T *head_out, const T *grad_concat, const T *grad_head,
                        T *grad_input, T *const *grad_filters, void *scratch, size_t scratch_bytes, void *cache,
                        size_t cache_bytes, const conv3p_cache_config *cfg, void *stream)
{
    if (!stack_desc_ok(sd) || !cache_cfg_ok(cfg) || !filters || !grad_filters) return CONV3P_ERR_INVALID_ARGUMENT;
    if ((size_t)B * N == 0) return CONV3P_OK;   // (grad_filters of an empty batch are the caller's zeros)
    const bool has_head = sd->num_class > 0;
    if (!points || !input || !concat || !grad_input || (has_head && (!head_out || !grad_head)) ||
        (!has_head && !grad_concat))
        return CONV3P_ERR_INVALID_ARGUMENT;
    if (has_head && grad_concat) return CONV3P_ERR_UNSUPPORTED;   // (see conv3p.h: not needed by either model) -- before any launch
    const StackCall<T> x{sd, B, N, cache, cache_bytes, cfg};
    TRY(stack_backward_fits<T>(x, voxel));
    StackScratch<T> ws;
    TRY(buf_check(scratch, scratch_bytes, carve_stack<T>(x, scratch, ws)));
    const size_t rows = x.rows();
    const int H = sd->hidden, CW = x.row(), nh = sd->n_hidden;
    T *ga = ws.ga, *gb = ws.gb, *dconcat = ws.dconcat;
    // every layer leaves its grad_filter partials in its own region.  The per-layer path: a layer's partials are summed by
    // rider workgroups of the NEXT layer's launch (reduce_rider: stream order makes them complete and visible there), and
    // one closing launch reduces what no launch carried -- the first layer's, and those of layers on other kernels; so the
    // chain of dependent backward kernels is not interleaved with reductions
    DeferredReduce<T> red[CONV3P_STACK_MAX_LAYERS + 1];
    for (int l = 0; l < stack_layers(sd); ++l) red[l].region = ws.region[l];
    auto reduce_all = [&]() -> int {
        ReduceJobs<T> jobs{};
        int nj = 0;
        unsigned gx = 0;
        for (int l = 0; l < stack_layers(sd); ++l)
            if (red[l].job.nslots > 0) {
                jobs.job[nj++] = red[l].job;
                const unsigned g = (red[l].job.nw + (unsigned)kReduceMultiW - 1u) / (unsigned)kReduceMultiW;
                gx = g > gx ? g : gx;
            }
        if (nj == 0) return CONV3P_OK;
        hipStream_t s = static_cast<hipStream_t>(stream);
        Scope sc(K_REDUCE, s);
        // one layer left (the riders took the others): 16 weights per workgroup -- a few MB are bound by the chain of
        // dependent loads, which is a quarter as long there (same summation order, same bits: reduce_slots)
        if (nj == 1)
            hipLaunchKernelGGL(reduce_partials_kernel<T>, dim3((jobs.job[0].nw + kReduceW - 1) / kReduceW), dim3(1024), 0, s,
                               jobs.job[0].partials, jobs.job[0].nslots, (size_t)jobs.job[0].nw, jobs.job[0].grad_filter);
        else
            hipLaunchKernelGGL(reduce_multi_kernel<T>, dim3(gx, (unsigned)nj), dim3(1024), 0, s, jobs);
        return hip_ok();
    };
    // layer l's backward call: grad_out -> dx (and the layer's partials, deferred); on the forward's points, so hinted
    auto layer_backward = [&](int l, const T *grad_out, T *dx, bool act, const T *addend, const RowLd *ld) -> int {
        return backward_impl<T>(grad_out, points, x.in(l, input, concat), filters[l], sd->strides[l], voxel, B, N, x.cin(l), x.cout(l),
                                sd->fz, sd->fy, sd->fx, dx, grad_filters[l], x.where(CONV3P_CACHE_POINTS_UNCHANGED | hints(cfg)),
                                stream, act, addend, ld, &red[l]);
    };
    int pending = -1;   // the layer whose partials wait for a launch to ride in
    auto ride = [&](int l) {
        red[l].ride = pending >= 0 ? red[pending].job : ReduceJob<T>{};
        red[l].rode = false;
    };
    auto rode = [&](int l) {
        if (red[l].rode) red[pending].job.nslots = 0;   // (summed inside layer l's launch: nothing left for reduce_all)
        pending = red[l].job.nslots > 0 ? l : -1;
    };
    // external gradient of the concat's column blocks: the caller's, the head's, or their sum
    const T *ext = grad_concat;
    int ld_ext = CW;
    if (has_head) {
        // g = dL/d(head conv output) = grad_head * selu'(head_out)
        TRY(selu_grad_impl<T>(head_out, grad_head, nullptr, ga, rows, sd->num_class, nullptr, stream));
        TRY(layer_backward(nh, ga, dconcat, false, nullptr, nullptr));
        pending = red[nh].job.nslots > 0 ? nh : -1;
        ext = dconcat;
    }
    // the hidden layers nh-1 .. 1 as ONE launch (conv3p_stack_fused.hpp) where the stack, the cache and the device allow it
    {
        T *const *G = ws.G;
        const int rc = stack_backward_fused<T>(x, points, filters, voxel, concat, ext, ld_ext, G, red, grad_filters,
                                               static_cast<hipStream_t>(stream));
        if (rc == CONV3P_OK) {
            TRY(layer_backward(0, G[0], grad_input, false, nullptr, nullptr));
            return reduce_all();
        }
        if (rc != CONV3P_ERR_UNSUPPORTED) return rc;
    }
    // g_l = dL/d(conv output of hidden layer l).  Last hidden layer: only the external gradient reaches its activation.
    T *g = has_head ? gb : ga, *gn = has_head ? ga : gb;
    {
        const int lds[4] = {CW, ld_ext, 0, H};
        TRY(selu_grad_impl<T>(concat + x.col(nh - 1), ext + x.col(nh - 1), nullptr, g, rows, H, lds, stream));
    }
    for (int l = nh - 1; l >= 1; --l) {
        // grad wrt the argument of the SELU that produced act_{l-1}: (dX + ext_{l-1}) * selu'(act_{l-1})
        const RowLd ld{x.ld_in(l), 0, H, H, ld_ext};
        ride(l);
        TRY(layer_backward(l, g, gn, /*act=*/true, ext + x.col(l - 1), &ld));
        rode(l);
        T *t = g; g = gn; gn = t;
    }
    ride(0);
    TRY(layer_backward(0, g, grad_input, false, nullptr, nullptr));
    rode(0);
    return reduce_all();
}

}  // namespace

extern "C" {

size_t conv3p_stack_scratch_bytes(const conv3p_stack_desc *desc, int elem_bytes, int B, int N)
{
    if (!stack_desc_ok(desc) || B < 0 || N < 0 || (elem_bytes != 4 && elem_bytes != 8)) return 0;
    const size_t b = elem_bytes == 4 ? stack_scratch_bytes<float>(desc, B, N) : stack_scratch_bytes<double>(desc, B, N);
    return b ? b : kAlign;
}
#define STACK_ENTRY(SFX, T)                                                                                         \
    int conv3p_stack_prefetch_##SFX(const conv3p_stack_desc *desc, const T *points, T voxel_size, int B, int N,     \
                                    void *cache, size_t cache_bytes, const conv3p_cache_config *cfg, void *stream,  \
                                    void *after_stream)                                                             \
    {                                                                                                               \
        return stack_prefetch_impl<T>(desc, points, voxel_size, B, N, cache, cache_bytes, cfg, stream,              \
                                      after_stream);                                                                \
    }                                                                                                               \
    int conv3p_stack_forward_##SFX(const conv3p_stack_desc *desc, const T *points, const T *input,                  \
                                   const T *const *filters, T voxel_size, int B, int N, T *concat, T *head_out,     \
                                   void *cache, size_t cache_bytes, const conv3p_cache_config *cfg, void *stream,   \
                                   void *side_stream)                                                               \
    {                                                                                                               \
        return stack_forward_impl<T>(desc, points, input, filters, voxel_size, B, N, concat, head_out, cache,       \
                                     cache_bytes, cfg, stream, side_stream);                                        \
    }                                                                                                               \
    int conv3p_stack_backward_##SFX(const conv3p_stack_desc *desc, const T *points, const T *input,                 \
                                    const T *const *filters, T voxel_size, int B, int N, const T *concat,           \
                                    const T *head_out, const T *grad_concat, const T *grad_head, T *grad_input,     \
                                    T *const *grad_filters, void *scratch, size_t scratch_bytes, void *cache,       \
                                    size_t cache_bytes, const conv3p_cache_config *cfg, void *stream)               \
    {                                                                                                               \
        return stack_backward_impl<T>(desc, points, input, filters, voxel_size, B, N, concat, head_out,             \
                                      grad_concat, grad_head, grad_input, grad_filters, scratch, scratch_bytes,     \
                                      cache, cache_bytes, cfg, stream);                                             \
    }
STACK_ENTRY(f32, float)
STACK_ENTRY(f64, double)

}  // extern "C"
