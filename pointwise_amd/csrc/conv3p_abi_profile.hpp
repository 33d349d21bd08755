// conv3p_abi_profile.hpp -- the profile calls: host-side launch scopes per kind, timed by events.  Included by
// conv3p_abi.hip.
namespace {

// ----------------------------------------------------------------------------- profiling
enum Kind { K_PREP = 0, K_SEARCH, K_FORWARD, K_BACKWARD, K_REDUCE, K_SELU, K_SELU_GRAD, K_MEMSET,
            K_DEEP_GEMM, K_DEEP_DW, K_TRANSPOSE, K_DEEP_ORDER, K_FC_FWD, K_FC_DX, K_FC_DW, K_DEEP_GEMM_BF16, K_DEEP_DW_BF16,
            K_GENERIC_FWD, K_GENERIC_BWD,   // the thread-per-pair kernels (global float atomics) over a whole call
            K_SEG_HEAD,                     // seg_head_kernel + seg_head_finish_kernel (conv3p_seg_head.hpp)
            K_NKINDS };
constexpr int kNoKind = -1;                 // a Scope of no kind counts nothing
const char *const kKindName[K_NKINDS] = {"prep_kernel", "search_kernel", "forward_kernel",
                                         "backward_kernel", "reduce_partials_kernel", "selu_kernel",
                                         "selu_grad_kernel", "memset", "deep_gemm_kernel", "deep_dw_kernel",
                                         "transpose_filter_kernel", "deep_order_kernel", "fc_forward_kernel",
                                         "fc_dx_kernel", "fc_dw_kernel", "deep_gemm_bf16_kernel", "deep_dw_bf16_kernel",
                                         "generic_forward_kernel", "generic_backward_kernel", "seg_head_kernel"};
struct Prof {
    std::mutex mu;
    bool on = false;
    struct Rec { int kind; hipEvent_t a, b; };
    std::vector<Rec> recs;
    std::vector<hipEvent_t> pool;
    hipEvent_t get()
    {
        if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
        hipEvent_t e = nullptr;
        (void)hipEventCreate(&e);
        return e;
    }
} g_prof;

struct Scope {
    hipStream_t s;
    hipEvent_t b = nullptr;
    bool on;
    Scope(int kind, hipStream_t stream) : s(stream), on(false)
    {
        if (kind == kNoKind) return;
        std::lock_guard<std::mutex> lk(g_prof.mu);
        on = g_prof.on;
        if (!on) return;
        hipEvent_t a = g_prof.get();
        b = g_prof.get();
        (void)hipEventRecord(a, s);
        g_prof.recs.push_back({kind, a, b});
    }
    ~Scope()
    {
        if (on) (void)hipEventRecord(b, s);
    }
};

// a zero-fill on the call's stream, counted as a launch of its own kind
int zero_async(void *p, size_t bytes, hipStream_t s)
{
    if (bytes == 0) return CONV3P_OK;
    Scope sc(K_MEMSET, s);
    return hipMemsetAsync(p, 0, bytes, s) == hipSuccess ? CONV3P_OK : CONV3P_ERR_LAUNCH;
}

}  // namespace

extern "C" {

int conv3p_profile_enable(int on)
{
    std::lock_guard<std::mutex> lk(g_prof.mu);
    g_prof.on = on != 0;
    return CONV3P_OK;
}
int conv3p_profile_reset(void)
{
    std::lock_guard<std::mutex> lk(g_prof.mu);
    for (auto &r : g_prof.recs) {
        g_prof.pool.push_back(r.a);
        g_prof.pool.push_back(r.b);
    }
    g_prof.recs.clear();
    return CONV3P_OK;
}
int conv3p_profile_kinds(void) { return K_NKINDS; }
const char *conv3p_profile_name(int kind) { return kind >= 0 && kind < K_NKINDS ? kKindName[kind] : ""; }
int conv3p_profile_read(int kind, uint64_t *launches, double *total_ms)
{
    std::lock_guard<std::mutex> lk(g_prof.mu);
    uint64_t n = 0;
    double ms = 0.0;
    for (auto &r : g_prof.recs) {
        if (r.kind != kind) continue;
        if (hipEventSynchronize(r.b) != hipSuccess) return CONV3P_ERR_LAUNCH;
        float t = 0.f;
        if (hipEventElapsedTime(&t, r.a, r.b) != hipSuccess) return CONV3P_ERR_LAUNCH;
        ms += t;
        ++n;
    }
    if (launches) *launches = n;
    if (total_ms) *total_ms = ms;
    return CONV3P_OK;
}

}  // extern "C"
