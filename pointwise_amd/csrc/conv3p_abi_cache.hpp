// conv3p_abi_cache.hpp -- where a call's state lives: the host record of a persistent neighbour cache, the Where of a
// call, and begin_call, which turns both into the call's slot and control block.  Included by conv3p_abi.hip.
namespace {

// ----------------------------------------------------------------------------- cache (host side)
// What the host remembers about a cache buffer: only which stencil tag lives in which slot
// (LRU) and a call counter.  Validity itself is decided on the device (CacheCtl).
//
// CacheShaped: everything that holds for ONE shape (B, N, elem, ntap_max, nslots, ppp) of the buffer.  A call with another
// shape re-shapes the record: it assigns a fresh CacheShaped, so a field added here starts over with the rest.
struct CacheShaped {
    int B = -1, N = -1, elem = 0, ntap_max = 0, nslots = 0, ppp = 0;
    std::vector<unsigned long long> tags;
    std::vector<uint64_t> stamp;
    std::vector<uint64_t> built_gen;   // generation in which the slot's search was last enqueued
    struct SlotDesc { int fz = 0, fy = 0, fx = 0; int32_t stride[3] = {0, 0, 0}; double voxel = 0.0; };
    std::vector<SlotDesc> desc;        // what stencil the slot's tag stands for (un-hinted calls rebuild them all together)
    uint64_t clock = 0;
    uint64_t gen = 0;                  // bumped by every call that does not carry CONV3P_CACHE_POINTS_UNCHANGED
    uint32_t epoch = 0;
    // record orders of the matrix-core path left in the scratch region: for which slot, built in which generation
    // (0: none).  Any call that uses the scratch for something else clears them.
    int order_slot[2] = {-1, -1};
    uint64_t order_gen[2] = {0, 0};
    // conv3p_stack_prefetch_*: geometry of `pending_points` enqueued on another stream
    const void *pending_points = nullptr;
    int pending_layers = 0;

    CacheShaped() = default;
    CacheShaped(int B_, int N_, int elem_, int ntap_max_, int nslots_, int ppp_)
        : B(B_), N(N_), elem(elem_), ntap_max(ntap_max_), nslots(nslots_), ppp(ppp_), tags(nslots_, 0ull), stamp(nslots_, 0ull),
          built_gen(nslots_, 0ull), desc(nslots_)
    {
    }
    bool shaped(int B_, int N_, int elem_, int ntap_max_, int nslots_, int ppp_) const
    {
        return B == B_ && N == N_ && elem == elem_ && ntap_max == ntap_max_ && nslots == nslots_ && ppp == ppp_;
    }
};
// ... and what lives as long as the record (until conv3p_cache_forget), whatever shapes the buffer is used with.
struct CacheHost : CacheShaped {
    std::vector<hipEvent_t> ready;     // the stack-level entry points' events: ready[l] fires when layer l's lists are complete
    // fused stack launches (conv3p_stack_fused.hpp): the per-cloud arrival counters -- a small device allocation of the
    // library's own (the caller's cache bytes may be garbage; a counter must not be), [kind][clouds][kSyncLineWords]: a
    // cloud's line = {counter, placement word, error bits} -- and the value every counter of a kind holds between launches
    uint32_t *sync = nullptr;
    int sync_clouds = 0;
    uint32_t sync_base[2] = {0u, 0u};
    uint32_t fused_launches[2] = {0u, 0u};
    uint32_t *host_err = nullptr;      // one word of host-mapped memory the fused kernels set on an error (looked at before every launch)
};

// The records by cache address, behind one mutex.  A CacheRef holds the mutex while it lives and is empty (false) when the
// cache has no record.
std::mutex g_cache_mu;
std::map<void *, CacheHost> g_caches;
struct CacheRef {
    std::unique_lock<std::mutex> lk;
    CacheHost *h;
    explicit operator bool() const { return h != nullptr; }
    CacheHost &operator*() const { return *h; }
    CacheHost *operator->() const { return h; }
};
inline CacheRef find_cache(void *cache)
{
    std::unique_lock<std::mutex> lk(g_cache_mu);
    auto it = g_caches.find(cache);
    return CacheRef{std::move(lk), it != g_caches.end() ? &it->second : nullptr};
}
// ... a cache's first call creates its record
inline CacheRef find_or_create_cache(void *cache)
{
    std::unique_lock<std::mutex> lk(g_cache_mu);
    CacheHost *h = &g_caches[cache];
    return CacheRef{std::move(lk), h};
}

void note_deep_order(const Call<float> &c, int which)
{
    if (c.cache_key == nullptr) return;   // per-call workspace: nothing outlives the call
    const CacheRef h = find_cache(c.cache_key);
    if (!h) return;
    h->order_slot[which] = c.slot;
    h->order_gen[which] = c.gen;
}

// Describes where a call's state lives: a persistent cache or per-call scratch.
struct Where {
    void *buf;
    size_t bytes;
    bool persistent;
    int nslots, ntap_max, ppp;
    size_t scratch_cap;   // persistent: bytes of scratch the layout was sized with
    int flags;            // CONV3P_CACHE_* of this call
};
inline int call_prec(const Where &wh) { return wh.persistent && (wh.flags & CONV3P_CACHE_MATMUL_BF16) != 0 ? kPrecBf16 : kPrecF32; }

// The routes' scratch sizes (conv3p_abi_routes.hpp, which needs this file's note_deep_order)
size_t deep_scratch_bytes(const Dims &d, size_t pair_slots);
size_t cache_scratch_bytes(int elem, int B, int N, int max_taps, int max_Cin, int max_Cout, int ppp);

// keep_orders: the route may find the matrix-core path's record orders left in the scratch region
template <typename T>
int begin_call(Call<T> &c, const Dims &d, const int32_t *stride, T voxel, size_t scratch, const Where &wh,
               hipStream_t s, bool keep_orders = false)
{
    c.d = d;
    c.st = make_stencil<T>(d, stride, voxel);
    c.s = s;
    // (read by deep_forward / deep_backward only: every other path ignores the bit)
    c.prec = call_prec(wh);
    const int ntap_max = wh.persistent ? wh.ntap_max : d.ntap;
    if (d.ntap > ntap_max) return CONV3P_ERR_WORKSPACE;
    if (wh.persistent && scratch > wh.scratch_cap) return CONV3P_ERR_WORKSPACE;
    c.scratch = wh.persistent ? wh.scratch_cap : scratch;
    c.L = carve<T>(d.B, d.N, d.ntiles, ntap_max, wh.nslots, wh.ppp, c.scratch, wh.buf);
    TRY(buf_check(wh.buf, wh.bytes, c.L.bytes));
    // (a forward's route needs only part of the matrix-core scratch: the orders count only where all of it is there)
    keep_orders = keep_orders && c.scratch >= deep_scratch_bytes(d, (size_t)d.B * c.L.pairs_per_cloud);
    const unsigned long long tag = stencil_tag(d, stride, (double)voxel, (int)sizeof(T));
    if (!wh.persistent) {
        c.slot = 0;
        c.cc = make_ctl(c.L, 0, tag, 1u, /*force=*/1);
        return CONV3P_OK;
    }
    const CacheRef ref = find_or_create_cache(wh.buf);
    CacheHost &h = *ref;
    // (the events and the fused launches' counters outlive a re-shape: they are not part of CacheShaped)
    if (!h.shaped(d.B, d.N, (int)sizeof(T), ntap_max, wh.nslots, wh.ppp))
        static_cast<CacheShaped &>(h) = CacheShaped(d.B, d.N, (int)sizeof(T), ntap_max, wh.nslots, wh.ppp);
    const bool hinted = (wh.flags & CONV3P_CACHE_POINTS_UNCHANGED) != 0 && h.gen != 0;
    if (!hinted) h.gen += 1;
    int slot = -1;
    for (int i = 0; i < h.nslots; ++i)
        if (h.tags[i] == tag) slot = i;
    if (slot < 0) {   // least recently used slot; the device-side tag check forces its rebuild
        slot = 0;
        for (int i = 1; i < h.nslots; ++i)
            if (h.stamp[i] < h.stamp[slot]) slot = i;
        h.tags[slot] = tag;
        h.built_gen[slot] = 0;
    }
    {
        CacheHost::SlotDesc &sd = h.desc[slot];
        sd.fz = d.fz; sd.fy = d.fy; sd.fx = d.fx;
        sd.stride[0] = stride[0]; sd.stride[1] = stride[1]; sd.stride[2] = stride[2];
        sd.voxel = (double)voxel;
    }
    c.skip_prep = hinted;
    c.evicted_hinted = hinted && h.built_gen[slot] == 0 && c.L.slot[slot].cursor != nullptr;
    c.skip_search = hinted && h.built_gen[slot] == h.gen;
    h.built_gen[slot] = h.gen;
    c.cache_key = wh.buf;
    c.gen = h.gen;
    for (int w = 0; w < 2; ++w)
        c.order_ok[w] = c.skip_search && keep_orders && h.order_slot[w] == slot && h.order_gen[w] == h.gen && h.gen != 0;
    // a call with channels may use the scratch region for anything (partials, Z, ...): the orders count as gone unless
    // the matrix-core path, which leaves them in place, says otherwise (deep_forward / deep_backward re-note them)
    if (d.Cin > 0) h.order_gen[0] = h.order_gen[1] = 0;
    h.stamp[slot] = ++h.clock;
    h.epoch += 1;
    if (h.epoch == 0) h.epoch = 1;
    c.slot = slot;
    c.cc = make_ctl(c.L, slot, tag, h.epoch, /*force=*/0);
    return CONV3P_OK;
}

bool cache_cfg_ok(const conv3p_cache_config *cfg)
{
    return cfg && cfg->slots > 0 && cfg->slots <= 64 && cfg->max_taps > 0 && cfg->max_taps < (int)kNoTap &&
           cfg->max_Cin >= 0 && cfg->max_Cout >= 0;
}

// A per-call workspace (its taps are the call's: begin_call)
Where stateless(void *ws, size_t bytes) { return Where{ws, bytes, false, 1, 0, kDefaultPairsPerPoint, 0, 0}; }
// ... of conv3p_neighbor_count_*: populations only, no pair storage
Where populations_only(void *ws, size_t bytes, int ntap) { return Where{ws, bytes, false, 1, ntap, 0, 0, 0}; }

// the caller's hints about the lists' lengths: what the stack's calls pass on of cfg->flags
inline int hints(const conv3p_cache_config *cfg)
{
    return cfg->flags & (CONV3P_CACHE_SPARSE_NEIGHBOURHOODS | CONV3P_CACHE_DENSE_NEIGHBOURHOODS);
}
// pair slots per point of a cache of this configuration
inline int pairs_per_point(const conv3p_cache_config *cfg)
{
    return cfg->pairs_per_point > 0 ? cfg->pairs_per_point : kDefaultPairsPerPoint;
}
// flags: CONV3P_CACHE_* of this call (cfg->flags is the caller's to pass on or not)
Where persistent(int elem, int B, int N, void *cache, size_t bytes, const conv3p_cache_config *cfg, int flags)
{
    const int ppp = pairs_per_point(cfg);
    return Where{cache, bytes, true, cfg->slots, cfg->max_taps, ppp,
                 cache_scratch_bytes(elem, B, N, cfg->max_taps, cfg->max_Cin, cfg->max_Cout, ppp), flags};
}

}  // namespace

extern "C" {

size_t conv3p_cache_bytes(int elem_bytes, int B, int N, const conv3p_cache_config *cfg)
{
    if ((elem_bytes != 4 && elem_bytes != 8) || B < 0 || N < 0 || !cache_cfg_ok(cfg)) return 0;
    const int ppp = pairs_per_point(cfg);
    return layout_bytes(elem_bytes, B, N, cfg->max_taps, cfg->slots, ppp,
                        cache_scratch_bytes(elem_bytes, B, N, cfg->max_taps, cfg->max_Cin, cfg->max_Cout, ppp));
}

int conv3p_cache_forget(void *cache)
{
    std::lock_guard<std::mutex> lk(g_cache_mu);
    auto it = g_caches.find(cache);
    if (it != g_caches.end()) {
        for (hipEvent_t e : it->second.ready) (void)hipEventDestroy(e);
        if (it->second.sync != nullptr) (void)hipFree(it->second.sync);
        if (it->second.host_err != nullptr) (void)hipHostFree(it->second.host_err);
        g_caches.erase(it);
    }
    return CONV3P_OK;
}

int conv3p_cache_fused_status(void *cache, unsigned *forward_launches, unsigned *backward_launches, unsigned *error_bits)
{
    uint32_t *sync = nullptr;
    int clouds = 0;
    {
        std::lock_guard<std::mutex> lk(g_cache_mu);
        auto it = g_caches.find(cache);
        if (forward_launches) *forward_launches = it != g_caches.end() ? it->second.fused_launches[0] : 0u;
        if (backward_launches) *backward_launches = it != g_caches.end() ? it->second.fused_launches[1] : 0u;
        if (it != g_caches.end()) { sync = it->second.sync; clouds = it->second.sync_clouds; }
    }
    if (error_bits) {
        *error_bits = 0u;
        if (sync != nullptr) {
            std::vector<uint32_t> h((size_t)2 * clouds * kSyncLineWords);
            if (hipMemcpy(h.data(), sync, h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) {
                (void)hipGetLastError();
                return CONV3P_ERR_LAUNCH;
            }
            for (size_t l = 0; l < h.size(); l += kSyncLineWords) *error_bits |= h[l + 2];
        }
    }
    return CONV3P_OK;
}

int conv3p_cache_init(void *cache, size_t cache_bytes, void *stream)
{
    if (cache == nullptr) return cache_bytes == 0 ? CONV3P_OK : CONV3P_ERR_INVALID_ARGUMENT;
    (void)conv3p_cache_forget(cache);
    if (hipMemsetAsync(cache, 0, cache_bytes, static_cast<hipStream_t>(stream)) != hipSuccess) {
        (void)hipGetLastError();
        return CONV3P_ERR_LAUNCH;
    }
    return CONV3P_OK;
}

}  // extern "C"
