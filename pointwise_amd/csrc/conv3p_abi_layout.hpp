// conv3p_abi_layout.hpp -- what a conv3p call is made of: its checked dimensions and stencil, the one buffer layout of
// workspaces and caches, and the Call record every launcher reads.  Included by conv3p_abi.hip.
namespace {

// ----------------------------------------------------------------------------- validation
struct Dims {
    int B, N, Cin, Cout, fz, fy, fx;
    int ntap, ntiles;
};

int check(Dims &d, const int32_t *stride, double voxel, bool need_channels)
{
    // mirrors the reference's OP_REQUIRES checks as far as a flat C signature can
    // (ranks and matching batch sizes are the host mirror's job, .cpp:410-443)
    if (d.B < 0 || d.N < 0) return CONV3P_ERR_INVALID_ARGUMENT;
    if (d.fz <= 0 || d.fy <= 0 || d.fx <= 0) return CONV3P_ERR_INVALID_ARGUMENT;
    if (need_channels && (d.Cin < 0 || d.Cout < 0)) return CONV3P_ERR_INVALID_ARGUMENT;
    if (!stride || stride[0] <= 0 || stride[1] <= 0 || stride[2] <= 0) return CONV3P_ERR_INVALID_ARGUMENT;
    if (!(voxel > 0.0)) return CONV3P_ERR_INVALID_ARGUMENT;   // also rejects NaN
    const long long ntap = (long long)d.fz * d.fy * d.fx;
    if (ntap >= (long long)kNoTap) return CONV3P_ERR_UNSUPPORTED;   // taps are 12-bit fields of the pair code
    d.ntap = (int)ntap;
    d.ntiles = (d.N + kTile - 1) / kTile;
    const int ext[3] = {d.fx, d.fy, d.fz};
    for (int a = 0; a < 3; ++a) {
        const long long full = (long long)(ext[a] - 1) * stride[a] + 1;
        if (full > 4096) return CONV3P_ERR_UNSUPPORTED;
    }
    return CONV3P_OK;
}

template <typename T> Stencil<T> make_stencil(const Dims &d, const int32_t *stride, T voxel)
{
    Stencil<T> st;
    st.ext[0] = d.fx; st.ext[1] = d.fy; st.ext[2] = d.fz;
    st.maxfull = 1;
    for (int a = 0; a < 3; ++a) {
        st.step[a] = stride[a];
        st.full[a] = (st.ext[a] - 1) * st.step[a] + 1;
        st.half[a] = ((double)st.full[a] * 0.5) * (double)voxel;   // .cpp:240, evaluated in double
        if (st.full[a] > st.maxfull) st.maxfull = st.full[a];
        st.inv[a] = (float)(1.0 / ((double)st.step[a] * (double)voxel));
        st.shift[a] = (float)((1.0 - 1.0 / (double)st.step[a]) * 0.5 - 0.5);
        st.halfw[a] = (float)(0.5 / (double)st.step[a]);
        st.mmax[a] = (float)(st.ext[a] - 1);
        st.reach[a] = (int)((st.full[a] + 1) * 0.5);              // .cpp:247-249
    }
    st.window = ((st.full[0] & 1) == 0 || (st.full[1] & 1) == 0 || (st.full[2] & 1) == 0) ? 1 : 0;
    st.ntap = d.ntap;
    st.voxel = voxel;
    return st;
}

// 64-bit tag of a stencil: what a cache slot was built for
unsigned long long stencil_tag(const Dims &d, const int32_t *stride, double voxel, int elem)
{
    unsigned long long h = 0xcbf29ce484222325ull;
    auto mix = [&](unsigned long long v) {
        h ^= v;
        h *= 0x100000001b3ull;
        h ^= h >> 29;
    };
    unsigned long long vb;
    std::memcpy(&vb, &voxel, 8);
    mix((unsigned long long)d.fz); mix((unsigned long long)d.fy); mix((unsigned long long)d.fx);
    mix((unsigned long long)stride[0]); mix((unsigned long long)stride[1]); mix((unsigned long long)stride[2]);
    mix(vb); mix((unsigned long long)elem); mix((unsigned long long)d.B); mix((unsigned long long)d.N);
    return h | 1ull;
}

BlockMap make_blockmap(const Dims &d)
{
    BlockMap m;
    m.blocks_per_cloud = d.ntiles;   // one workgroup per query tile
    m.clouds = d.B;
    m.rounds = (d.B + 7) / 8;
    return m;
}
inline unsigned grid_of(const BlockMap &m) { return 8u * (unsigned)m.rounds * (unsigned)m.blocks_per_cloud; }
// (Tried and dropped: two consecutive query tiles per backward workgroup -- half the grad_filter partials, one resident
// round of 512 workgroups -- 0.247 -> 0.306 ms/step: the kernel is latency-bound per workgroup and wants as many tiles
// in flight as fit; and handling the taps in 2-3 ranges to shrink G and fit a third workgroup per CU -- 0.247 -> 0.385.)

// ----------------------------------------------------------------------------- buffer layout
// One layout serves both the per-call workspace (1 slot, rebuilt every call) and the persistent
// neighbour cache (several slots).  Everything a slot holds depends only on (points, stencil).
constexpr int kGroupTiles = 128;      // candidate tiles per search group (64 KiB of hit masks in LDS)
constexpr int kFusedMaxPoints = 16384;   // clouds the prep kernel sorts: only their tiles are compact enough for the window tables
constexpr int kDefaultPairsPerPoint = 256;   // 16-B records; room-like clouds reach ~170 neighbours/point

template <typename T> struct Layout {
    // per cloud, independent of the stencil
    unsigned long long *hash;
    uint32_t *version;
    PointRec<T> *pts;
    T *boxes;
    T *cmin;   // [B][3] origin of the reference's uniform grid (stencils with an even dilated extent only)
    unsigned long long *ftab;   // [B][ntiles][kFTableU64] per-tile window tables of the fused search (sorted clouds only)
    uint32_t *tab_version, *tab_ticket;   // [B] version of the cloud its tables were built from / tiles done (tile_tables_kernel)
    uint32_t *tab_inv;                    // [B] bits of the inv16 (= 16 / voxel) the tables were built with
    // per slot
    struct Slot {
        uint32_t *built_version, *cursor, *ticket;
        unsigned long long *built_tag;
        int32_t *count, *tcount;   // populations: original-index order (B,N,F) / tile-major [tile][F][64]
        uint2 *segs, *qsegs;
        uint32_t *qbm;             // [B][ntiles][64] backward taps each centre's list holds (bit f' of taps 0 .. 31)
        uint32_t *qbm_hi;          // ... taps 32 .. 63 (caches / workspaces for filters of more than 32 taps; else nullptr)
        uint32_t *sched;           // [8][ceil(B / 8) * ntiles] launch order of the tiles per XCD (tile_sched_kernel)
        uint32_t *regime;          // [1] 1: short pair lists on average (tile_sched_kernel), see SchedJob
        PairEntry *pairs;
    };
    std::vector<Slot> slot;
    uint32_t *cursor_all;   // [nslots][2][B]: pair allocator and completion ticket of every slot
    int nclouds;
    uint32_t pairs_per_cloud;
    int gtiles, ngroups;
    // per-call scratch
    T *partials;
    size_t bytes;
};

// ntap_max: taps the slots must be able to hold; scratch_bytes: bytes of per-call scratch
template <typename T>
Layout<T> carve(int B, int N, int ntiles, int ntap_max, int nslots, int pairs_per_point, size_t scratch_bytes,
                void *base)
{
    Layout<T> L;
    Carver cv(base);
    const size_t tiles = (size_t)B * ntiles;
    // hit masks take 512 B per candidate tile of a group; leave room for the [taps][65] populations
    int gmax = kGroupTiles;
    {
        const size_t fixed = (size_t)ntap_max * kCntStride * 4 + 16 * 1024;
        const size_t room = fixed < 150 * 1024 ? 150 * 1024 - fixed : 0;
        const int fit = (int)(room / 516);
        if (fit < gmax) gmax = fit < 4 ? 4 : fit;
    }
    L.gtiles = ntiles < gmax ? (ntiles > 0 ? ntiles : 1) : gmax;
    L.ngroups = ntiles > 0 ? (ntiles + L.gtiles - 1) / L.gtiles : 1;
    L.hash = cv.take<unsigned long long>((size_t)B);
    L.version = cv.take<uint32_t>((size_t)B);
    L.pts = cv.take<PointRec<T>>(tiles * kTile);
    L.boxes = cv.take<T>(tiles * 6);
    L.cmin = cv.take<T>((size_t)B * 3);
    L.ftab = N <= kFusedMaxPoints ? cv.take<unsigned long long>(tiles * kFTableU64) : nullptr;
    L.tab_version = cv.take<uint32_t>((size_t)B);
    L.tab_ticket = cv.take<uint32_t>((size_t)B);
    L.tab_inv = cv.take<uint32_t>((size_t)B);
    size_t ppc = (size_t)N * (size_t)pairs_per_point;
    if ((size_t)B * ppc > 0xFFFFFFF0ull) ppc = B ? 0xFFFFFFF0ull / (size_t)B : 0;
    if (ppc > 0x7FFFFFFFull) ppc = 0x7FFFFFFFull;   // headroom for the allocator's transient overshoot (search_tile P2)
    L.pairs_per_cloud = (uint32_t)ppc;
    L.slot.resize(nslots);
    L.nclouds = B;
    L.cursor_all = cv.take<uint32_t>((size_t)B * nslots * 2);
    for (int s = 0; s < nslots; ++s) {
        auto &S = L.slot[s];
        S.built_version = cv.take<uint32_t>((size_t)B);
        S.cursor = L.cursor_all ? L.cursor_all + (size_t)(2 * s) * B : nullptr;
        S.ticket = L.cursor_all ? L.cursor_all + (size_t)(2 * s + 1) * B : nullptr;
        S.built_tag = cv.take<unsigned long long>((size_t)B);
        S.count = cv.take<int32_t>((size_t)B * N * ntap_max);
        S.tcount = cv.take<int32_t>(tiles * kTile * ntap_max);
        S.segs = cv.take<uint2>(tiles * L.ngroups);
        S.qsegs = cv.take<uint2>(tiles * L.ngroups * 64);
        S.qbm = cv.take<uint32_t>(tiles * 64 * (ntap_max > 64 ? 4 : ntap_max > 32 ? 2 : 1));   // one plane per 32 taps (up to 128)
        S.qbm_hi = ntap_max > 32 && S.qbm != nullptr ? S.qbm + tiles * 64 : nullptr;
        S.sched = cv.take<uint32_t>(8 * (size_t)((B + 7) / 8) * ntiles);
        S.regime = cv.take<uint32_t>(1);
        S.pairs = cv.take<PairEntry>((size_t)B * ppc);
    }
    L.partials = reinterpret_cast<T *>(cv.take<char>(scratch_bytes));
    L.bytes = cv.bytes();
    return L;
}

template <typename T> size_t lds_common(const Stencil<T> &st) { return (3 * (size_t)st.maxfull * 2 + 15) & ~(size_t)15; }
inline size_t a16(size_t x) { return (x + 15) & ~(size_t)15; }
constexpr size_t kMaxLds = 160 * 1024;
// A launch of 256-thread (or `block`) workgroups with `lds` bytes of dynamic LDS: the kernel's limit is raised to the
// request before every launch -- the attribute belongs to the kernel, not to the launch.
template <typename Kern, typename... Args>
inline void launch_lds(Kern kern, dim3 grid, dim3 block, size_t lds, hipStream_t s, const Args &...args)
{
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kern, grid, block, lds, s, args...);
}

// Everything one call needs.
template <typename T> struct Call {
    Dims d;
    Stencil<T> st;
    Layout<T> L;
    int slot;
    CacheCtl cc;
    hipStream_t s;
    size_t scratch = 0;            // bytes of the scratch region (L.partials)
    bool order_ok[2] = {false, false};   // the deep path's forward / backward record order of this geometry is in the scratch
    int prec = kPrecF32;           // filter contractions of the matrix-core path: kPrecBf16 = CONV3P_CACHE_MATMUL_BF16
    void *cache_key = nullptr;     // persistent cache the call runs in (host bookkeeping of the record orders)
    uint64_t gen = 0;
    bool evicted_hinted = false;   // slot re-assigned to a new stencil while prep is skipped: reset its allocators
    bool skip_prep = false;     // caller promised unchanged points
    bool skip_search = false;   // ... and this slot's lists were already enqueued for them
    // conv3p_layer_*: SELU fused into the op (pointcnn2_acsd.py:48-49).  forward: output = selu(conv);
    // backward: grad_input = (dX + addend) * selu'(input)
    bool act = false;
    bool accum = false;            // backward: add to the grad_input already there (column-split passes)
    const T *addend = nullptr;
    RowLd ld{0, 0, 0, 0, 0};       // row strides of the feature tensors; filled with the dense values by set_ld()
    bool strided = false;          // some tensor is a column block of a wider buffer (register-path shapes only)
    ReduceJob<T> rider{};          // stack backward, register kernels: partials of the layer above, summed by workgroups
                                   // appended to this call's first backward launch (reduce_rider); nslots == 0: none
};

template <typename T> void set_ld(Call<T> &c, const RowLd *ld, int Cin, int Cout)
{
    c.ld = RowLd{Cin, Cout, Cout, Cin, Cin};
    if (ld) {
        if (ld->in > 0) c.ld.in = ld->in;
        if (ld->out > 0) c.ld.out = ld->out;
        if (ld->dy > 0) c.ld.dy = ld->dy;
        if (ld->dx > 0) c.ld.dx = ld->dx;
        if (ld->add > 0) c.ld.add = ld->add;
    }
    c.strided = c.ld.in != Cin || c.ld.out != Cout || c.ld.dy != Cout || c.ld.dx != Cin || c.ld.add != Cin;
}

template <typename T> CacheCtl make_ctl(const Layout<T> &L, int slot, unsigned long long tag, uint32_t epoch, int force)
{
    CacheCtl cc;
    cc.hash = L.hash;
    cc.version = L.version;
    cc.built_version = L.slot[slot].built_version;
    cc.built_tag = L.slot[slot].built_tag;
    cc.cursor = L.slot[slot].cursor;
    cc.ticket = L.slot[slot].ticket;
    cc.cursor_all = L.cursor_all;
    cc.tab_version = L.tab_version;
    cc.tab_ticket = L.tab_ticket;
    cc.nslots = (int)L.slot.size();
    cc.nclouds = L.nclouds;
    cc.tag = tag;
    cc.epoch = epoch;
    cc.pairs_per_cloud = L.pairs_per_cloud;
    cc.force = force;
    return cc;
}

// Stack-level backward: a layer's grad_filter partials stay in the caller's region and are reduced later -- by the rider
// workgroups of the next layer's launch, or by the stack's closing reduction.
template <typename T> struct DeferredReduce {
    T *region = nullptr;      // in: where this layer's partials go (>= reduce_region_bytes)
    ReduceJob<T> job{};       // out: what to reduce (nslots == 0: the layer reduced its grad_filter itself)
    ReduceJob<T> ride{};      // in: partials of the layer above, complete when this layer's launches start (nslots == 0: none)
    bool rode = false;        // out: this layer's first launch sums `ride` (register kernels; else it stays the caller's)
};

size_t layout_bytes(int elem, int B, int N, int ntap, int nslots, int ppp, size_t scratch)
{
    const int ntiles = (N + kTile - 1) / kTile;
    return elem == 4 ? carve<float>(B, N, ntiles, ntap, nslots, ppp, scratch, nullptr).bytes
                     : carve<double>(B, N, ntiles, ntap, nslots, ppp, scratch, nullptr).bytes;
}

}  // namespace
