// conv3p_abi_search.hpp -- the geometry of a call: prep, the cloud origins, the fused and the tile-pair search, the
// companion stencils a cached search takes along, and the batched search of several strides.  Included by conv3p_abi.hip.
namespace {

template <typename T> int run_prep(const T *points, const Call<T> &c)
{
    if (c.skip_prep) {
        if (c.evicted_hinted)   // prep_sort_kernel would have done this for an un-hinted call
            return hipMemsetAsync(c.L.slot[c.slot].cursor, 0, sizeof(uint32_t) * 2 * (size_t)c.d.B, c.s) == hipSuccess
                       ? CONV3P_OK : CONV3P_ERR_LAUNCH;
        return CONV3P_OK;
    }
    const Dims &d = c.d;
    Scope sc(K_PREP, c.s);
    if (d.N <= 16384 && d.N > kTile) {
        int npad = 128;
        while (npad < d.N) npad <<= 1;
        const int threads = npad / 2 < 1024 ? (npad / 2 < 64 ? 64 : npad / 2) : 1024;
        const size_t lds = (size_t)npad * 8 + 256;
        auto launch = [&](auto kern) {
            launch_lds(kern, dim3(d.B), dim3(threads), lds, c.s, points, d.N, d.ntiles, npad, c.L.pts, c.L.boxes, c.cc);
        };
        switch (npad / threads) {   // keys per thread
        case 2: launch(prep_sort_kernel<T, 2>); break;
        case 4: launch(prep_sort_kernel<T, 4>); break;
        case 8: launch(prep_sort_kernel<T, 8>); break;
        default: launch(prep_sort_kernel<T, 16>); break;
        }
        return hip_ok();
    }
    dim3 grid((d.ntiles + kWavesPerBlock - 1) / kWavesPerBlock, d.B);
    hipLaunchKernelGGL(prep_kernel<T>, grid, dim3(256), 0, c.s, points, d.N, d.ntiles, c.L.pts, c.L.boxes, c.cc);
    return hip_ok();
}

template <typename T> size_t search_lds_bytes(const Stencil<T> &st, int gtiles)
{
    // (+ 1024: search_tile's static array of the centres' backward-tap sets -- it counts against the 160 KiB like the dynamic part)
    return lds_common(st) + a16((size_t)st.ntap * kCntStride * 4) + a16(sizeof(CentreRec<T>) * 64) + 64 * 3 * 4 +
           a16((size_t)gtiles * 64 * 8) + a16((size_t)gtiles * 4) + 32 + kWavesPerBlock * 64 * 4 +
           a16((size_t)kWavesPerBlock * 192 * 4) + a16((size_t)kWavesPerBlock * 256 * 4) + 1024;
}

// grid origin of every cloud, for stencils whose candidate window can decide (even dilated extents)
template <typename T> int run_cloud_min(const T *points, const Call<T> &c)
{
    if (!c.st.window) return CONV3P_OK;
    hipLaunchKernelGGL(cloud_min_kernel<T>, dim3((unsigned)c.d.B), dim3(256), 0, c.s, points, c.d.N, c.L.cmin);
    return hip_ok();
}

// launch order of a slot's tiles for the list-walking kernels
template <typename SlotT> inline const uint32_t *sched_of(const SlotT &S)
{
#ifdef CONV3P_DEV_NO_SCHED   // developer A/B build: BlockMap order
    return nullptr;
#else
    return S.sched;
#endif
}

// mean pre-filter hits per point below which a slot's lists count as SHORT (populated-rows backward for the dilated narrow
// layers): Conv3pStack.tune()'s threshold of 32 neighbours per point plus the pre-filter's ~10 % of false positives
// The regime word only matters for DILATED narrow layers (undilated ones never take the populated-rows kernel).  Of a
// dilated stencil's hits the window tables of the fused search let through 1.24 per neighbour (measured, see
// fused_compacts), the tile-pair pre-filter of search_tile ~1.1: the same 32 neighbours per point are
// kFHitsOf32Neighbours = 40 hits there and 35 here.
constexpr unsigned long long kShortListsPerPoint = 35, kShortListsPerPointFused = kFHitsOf32Neighbours;
template <typename T> SchedJob make_sched_job(const Call<T> &c, int slot, bool fused)
{
    const auto &S = c.L.slot[slot];
    return SchedJob{S.segs, S.sched, S.cursor, S.regime,
                    (fused ? kShortListsPerPointFused : kShortListsPerPoint) * (unsigned long long)c.d.B * (unsigned long long)c.d.N};
}

// ----------------------------------------------------------------------------- fused search (conv3p_search_fused.hpp)
#ifndef CONV3P_DEV_FUSED_M
#define CONV3P_DEV_FUSED_M 6     // candidate tiles per wave whose hit masks stay in LDS between the passes
#endif
template <typename T> bool fused_ok(const Call<T> &c)
{
#ifdef CONV3P_DEV_NO_FUSED_SEARCH   // developer A/B build: the tile-pair pre-filter of search_tile for everything
    return false;
#endif
    const Stencil<T> &st = c.st;
    if (c.L.ftab == nullptr || st.window) return false;
    for (int a = 0; a < 3; ++a)
        if (st.ext[a] > kFMaxExt) return false;
    return true;
}
template <typename T> FusedJob<T> make_fused_job(const Call<T> &c)
{
    const auto &S = c.L.slot[c.slot];
    FusedJob<T> j;
    j.st = c.st;
    j.cc = c.cc;
    j.count = S.count;
    j.tcount = S.tcount;
    j.pairs = S.pairs;
    j.segs = S.segs;
    j.qsegs = S.qsegs;
    j.qbm = S.qbm;
    j.qbm_hi = S.qbm_hi;
    for (int a = 0; a < 3; ++a)
        for (int k = 0; k < kFMaxExt; ++k)
            j.clo[a][k] = (float)(((double)k * c.st.step[a] - (double)c.st.full[a] * 0.5) * (double)kFR);
    return j;
}
// tables of every tile + ONE search launch for `njobs` stencils over the same points + the launch order of the tiles
// hit masks of a wave's first candidate tiles kept in LDS between the passes: as many as fit 40 KiB (0: not even one fits
// the LDS at all)
inline int fused_mask_depth(int elem, int ntiles, int ntap_max, int maxfull_max)
{
    const int mmax = (ntiles + kWavesPerBlock - 1) / kWavesPerBlock;
    int M = std::min(mmax, (int)CONV3P_DEV_FUSED_M);
    // small clouds (<= 32 tiles: a wave meets two or three candidate tiles): ONE stored mask -- 31 KiB instead of 41, a
    // fifth workgroup per CU; recomputing the others in pass 2 costs less than the occupancy gives (cfg2 search alone
    // 111 -> 106 us, under the backward 141 -> 123; on the rooms' 64 tiles per cloud the step does not move)
    if (ntiles <= 32) M = 1;
    if (M < 1) M = 1;
    while (M > 1 && fused_lds(ntap_max, maxfull_max, elem, M).total > 40 * 1024) --M;   // large filters: fewer stored masks
    return fused_lds(ntap_max, maxfull_max, elem, M).total > kMaxLds ? 0 : M;
}
template <typename T> int launch_fused(const Call<T> &c, const FusedJobs<T> &jobs, const SchedJobs &sjobs, int njobs, bool schedule = true)
{
    const Dims &d = c.d;
    const BlockMap bm = make_blockmap(d);
    int ntap_max = 1, maxfull_max = 1;
    for (int k = 0; k < njobs; ++k) {
        ntap_max = std::max(ntap_max, jobs.job[k].st.ntap);
        maxfull_max = std::max(maxfull_max, jobs.job[k].st.maxfull);
    }
    const int M = fused_mask_depth((int)sizeof(T), d.ntiles, ntap_max, maxfull_max);
    if (M == 0) return CONV3P_ERR_UNSUPPORTED;   // (callers test fused_fits() first and take the tile-pair search instead)
#ifdef CONV3P_DEV_FUSED_LDS_KB   // developer: pad the LDS request (fewer workgroups per CU) to see how the kernel scales with occupancy
    const size_t lds = std::max(fused_lds(ntap_max, maxfull_max, (int)sizeof(T), M).total, (size_t)CONV3P_DEV_FUSED_LDS_KB * 1024);
#else
    const size_t lds = fused_lds(ntap_max, maxfull_max, (int)sizeof(T), M).total;
#endif
    if (lds > kMaxLds) return CONV3P_ERR_UNSUPPORTED;
    const float inv16 = (float)((double)kFR / (double)c.st.voxel);
    Scope sc(K_SEARCH, c.s);
    hipLaunchKernelGGL(tile_tables_kernel<T>, dim3((d.ntiles + kWavesPerBlock - 1) / kWavesPerBlock, d.B), dim3(256), 0, c.s,
                       c.L.pts, d.ntiles, inv16, c.L.ftab, c.cc.version, c.L.tab_version, c.L.tab_ticket, c.L.tab_inv, c.cc.force);
    bool ext3 = true;
    for (int k = 0; k < njobs; ++k)
        for (int a = 0; a < 3; ++a) ext3 &= jobs.job[k].st.ext[a] == 3;
    auto launch = [&](auto kern) {
        launch_lds(kern, dim3(grid_of(bm), njobs), dim3(256), lds, c.s, c.L.pts, c.L.boxes, c.L.ftab, d.N, d.ntiles, c.L.ngroups, bm,
                   jobs, M, inv16);
    };
    if (ext3) launch(search_fused_kernel<T, true>);
    else launch(search_fused_kernel<T, false>);
#ifndef CONV3P_DEV_NO_SCHED   // developer A/B build: no launch order at all (BlockMap order; needs a hint: no regime word either)
    if (schedule)
        hipLaunchKernelGGL(tile_sched_kernel, dim3(8, njobs), dim3(1024), 0, c.s, sjobs, d.B, d.ntiles, c.L.ngroups, bm.rounds * d.ntiles);
#endif
    return hip_ok();
}

// An un-hinted call on a persistent cache re-validates the points; if they changed, EVERY stencil the cache holds is
// stale, and the caller (a framework executing a model op by op: 4 strides forward, the same 4 backward) is about to ask
// for each of them in turn.  The call therefore takes the cache's other stencils along as jobs of its own search launch
// (one launch for all strides: 115 us instead of 4 x 42 + launch overheads on cfg2); for clouds whose lists are current
// the extra jobs' workgroups exit at once, as the requested one's do.  Host bookkeeping only: what is rebuilt is still
// decided on the device.
template <typename T> int add_companions(const Call<T> &c, FusedJobs<T> &fj, SchedJobs &sj, int n)
{
    if (c.cache_key == nullptr || c.skip_prep) return n;   // per-call workspace, or the caller vouches for the points
    const CacheRef ref = find_cache(c.cache_key);
    if (!ref) return n;
    CacheHost &h = *ref;
    for (int sl = 0; sl < h.nslots && n < kFusedMaxJobs; ++sl) {
        if (sl == c.slot || h.tags[sl] == 0ull) continue;
        const CacheHost::SlotDesc &sd = h.desc[sl];
        if (sd.voxel != (double)c.st.voxel) continue;                 // the window tables are built for ONE voxel size
        Dims d2 = c.d;
        d2.fz = sd.fz; d2.fy = sd.fy; d2.fx = sd.fx;
        d2.ntap = sd.fz * sd.fy * sd.fx;
        Call<T> c2;
        c2.d = d2;
        c2.st = make_stencil<T>(d2, sd.stride, c.st.voxel);
        c2.L = c.L;
        c2.slot = sl;
        c2.s = c.s;
        c2.cc = make_ctl(c.L, sl, h.tags[sl], c.cc.epoch, /*force=*/0);
        if (!fused_ok(c2)) continue;
        // the launch's LDS request and the number M of hit masks a wave keeps follow the LARGEST filter among its jobs: a
        // companion must not cost the requested stencil its masks, let alone push the launch past the LDS limit
        if (fused_mask_depth((int)sizeof(T), c.d.ntiles, std::max(c.st.ntap, c2.st.ntap), std::max(c.st.maxfull, c2.st.maxfull)) <
            fused_mask_depth((int)sizeof(T), c.d.ntiles, c.st.ntap, c.st.maxfull))
            continue;
        fj.job[n] = make_fused_job(c2);
        sj.job[n] = make_sched_job(c, sl, true);
        ++n;
    }
    return n;
}
// ... and, once the launch that carries them has been issued without error: a hinted call for one of them later in
// this generation skips its search
template <typename T> void note_companions_built(const Call<T> &c, const FusedJobs<T> &fj, int n)
{
    if (c.cache_key == nullptr || n <= 1) return;
    const CacheRef ref = find_cache(c.cache_key);
    if (!ref) return;
    CacheHost &h = *ref;
    for (int k = 1; k < n; ++k)
        for (int sl = 0; sl < h.nslots; ++sl)
            if (sl != c.slot && h.tags[sl] == fj.job[k].cc.tag) h.built_gen[sl] = h.gen;
}

// search.  count: where the populations go.
template <typename T> int run_search(const Call<T> &c, int32_t *count, bool with_pairs)
{
    if (c.skip_search && with_pairs) return CONV3P_OK;
    const Dims &d = c.d;
    const Stencil<T> &st = c.st;
    const auto &S = c.L.slot[c.slot];
    if (fused_ok(c) && fused_mask_depth((int)sizeof(T), d.ntiles, st.ntap, st.maxfull) > 0 && (!with_pairs || count == S.count)) {
        FusedJobs<T> fj;
        SchedJobs sj;
        fj.job[0] = make_fused_job(c);
        sj.job[0] = make_sched_job(c, c.slot, true);
        if (!with_pairs) {   // populations only (conv3p_neighbor_count_*): into the caller's tensor, nothing else kept
            FusedJob<T> &j = fj.job[0];
            j.count = count;
            j.tcount = nullptr;
            j.pairs = nullptr;
            j.segs = nullptr;
            j.qsegs = nullptr;
            j.qbm = nullptr;
            j.qbm_hi = nullptr;
            return launch_fused<T>(c, fj, sj, 1, /*schedule=*/false);
        }
        const int nj = add_companions<T>(c, fj, sj, 1);
        TRY(launch_fused<T>(c, fj, sj, nj));
        note_companions_built<T>(c, fj, nj);
        return CONV3P_OK;
    }
    const size_t lds = search_lds_bytes(st, c.L.gtiles);
    if (lds > kMaxLds) return CONV3P_ERR_UNSUPPORTED;   // very large filters (> ~570 taps): populations alone exceed LDS
    const BlockMap bm = make_blockmap(d);
    {
        Scope sc(K_SEARCH, c.s);
        auto launch = [&](auto kern, const T *cmin) {
            launch_lds(kern, dim3(grid_of(bm)), dim3(256), lds, c.s, c.L.pts, c.L.boxes, st, d.N, d.ntiles, c.L.gtiles, c.L.ngroups,
                       bm, count, with_pairs ? S.pairs : nullptr, c.cc, S.segs, S.qsegs, cmin, with_pairs ? S.tcount : nullptr,
                       with_pairs ? S.qbm : nullptr, with_pairs ? S.qbm_hi : nullptr);
        };
        if (st.window) launch(search_kernel<T, true>, c.L.cmin);
        else launch(search_kernel<T, false>, static_cast<const T *>(nullptr));
        if (with_pairs) {
            SchedJobs sj;
            sj.job[0] = make_sched_job(c, c.slot, false);
            hipLaunchKernelGGL(tile_sched_kernel, dim3(8, 1), dim3(1024), 0, c.s, sj, d.B, d.ntiles, c.L.ngroups, bm.rounds * d.ntiles);
        }
    }
    return hip_ok();
}

// The geometry of a call, after begin_call: sorted points and boxes, the clouds' grid origins, and the lists and
// populations of the call's slot (each skipped where begin_call found it current).
template <typename T> int run_geometry(const T *points, const Call<T> &c)
{
    TRY(run_prep<T>(points, c));
    TRY(run_cloud_min<T>(points, c));
    return run_search<T>(c, c.L.slot[c.slot].count, true);
}

#ifdef CONV3P_DEV_WALK_STATS
// developer instrumentation build only (-DCONV3P_DEV_WALK_STATS, tools/walk_stats.py): how well the list-walking kernels'
// lane mapping uses a wave.  Per query tile, from the per-centre segment table: records, steps of the shipped mapping
// (wave = 16 centres x 4 sub-lanes: ceil(longest list / 4)), steps with the lanes of a wave dealt to its centres in
// proportion to their lists, the same over the whole workgroup, and the bound ceil(records / 64).
__global__ void walk_stats_kernel(const uint2 *qsegs, const PairEntry *pairs, int ntiles_all, unsigned long long *out)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ntiles_all) return;
    uint32_t len[64];
    unsigned long long recs = 0, live = 0;
    for (int c = 0; c < 64; ++c) {
        const uint2 sg = qsegs[(size_t)t * 64 + c];
        len[c] = sg.y == kSegOverflow ? 0u : sg.y;
        recs += len[c];
        for (uint32_t i = 0; i < len[c]; ++i) live += code_fwd(pairs[sg.x + i].code) != kNoTap ? 1u : 0u;
    }
    unsigned long long cur = 0, pslw = 0, ideal = 0, curmax = 0, pslmax = 0, idealmax = 0;
    for (int w = 0; w < 4; ++w) {
        uint32_t mx = 0, sum = 0;
        for (int c = 0; c < 16; ++c) { mx = max(mx, len[16 * w + c]); sum += len[16 * w + c]; }
        const unsigned long long a = (mx + 3) / 4;
        uint32_t S = max(1u, (sum + 63) / 64);
        for (;; ++S) {
            uint32_t need = 0;
            for (int c = 0; c < 16; ++c) need += (len[16 * w + c] + S - 1) / S;
            if (need <= 64) break;
        }
        const unsigned long long idl = (sum + 63) / 64;
        cur += a; pslw += S; ideal += idl;
        curmax = max(curmax, a); pslmax = max(pslmax, (unsigned long long)S); idealmax = max(idealmax, idl);
    }
    uint32_t St = max(1u, (uint32_t)((recs + 255) / 256));
    for (;; ++St) {
        uint32_t need = 0;
        for (int c = 0; c < 64; ++c) need += (len[c] + St - 1) / St;
        if (need <= 256) break;
    }
    atomicAdd(&out[0], recs); atomicAdd(&out[1], live); atomicAdd(&out[2], cur); atomicAdd(&out[3], pslw);
    atomicAdd(&out[4], 4ull * St); atomicAdd(&out[5], ideal);
    atomicMax(&out[6], curmax); atomicMax(&out[7], pslmax); atomicMax(&out[8], (unsigned long long)St); atomicMax(&out[9], idealmax);
}
template <typename T> void dev_walk_stats(const Call<T> &c, const char *what, int ci, int co)
{
    const auto &S = c.L.slot[c.slot];
    if (c.L.ngroups != 1) return;
    unsigned long long *d = nullptr, h[10];
    if (hipMalloc(&d, sizeof(h)) != hipSuccess) return;
    (void)hipMemsetAsync(d, 0, sizeof(h), c.s);
    const int nt = c.d.B * c.d.ntiles;
    hipLaunchKernelGGL(walk_stats_kernel, dim3((nt + 63) / 64), dim3(64), 0, c.s, S.qsegs, S.pairs, nt, d);
    (void)hipStreamSynchronize(c.s);
    (void)hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    const double r = (double)h[0];
    fprintf(stderr, "walk_stats %s<%d,%d> stride %d B=%d N=%d: records/point %.2f (true pairs %.2f) | lane use: shipped %.3f (true-pair %.3f), "
            "per-wave proportional %.3f, per-workgroup proportional %.3f, bound %.3f | steps of the slowest wave: shipped %llu, "
            "per-wave prop. %llu, per-wg prop. %llu, bound %llu | mean steps per wave: %.2f / %.2f / %.2f / %.2f\n",
            what, ci, co, c.st.step[0], c.d.B, c.d.N, r / ((double)c.d.B * c.d.N), (double)h[1] / ((double)c.d.B * c.d.N),
            r / (64.0 * h[2]), (double)h[1] / (64.0 * h[2]), r / (64.0 * h[3]), r / (64.0 * h[4]), r / (64.0 * h[5]),
            h[6], h[7], h[8], h[9], h[2] / (4.0 * nt), h[3] / (4.0 * nt), h[4] / (4.0 * nt), h[5] / (4.0 * nt));
}
#endif

// geometry of K stencils (same filter extents, K strides) over the same points: one prep, ONE search launch and
// nothing else
template <typename T>
int prepare_multi_impl(const T *points, const int32_t *strides, int K, T voxel, int B, int N, int fz, int fy,
                       int fx, Where wh, void *stream)
{
    if (K <= 0 || K > kMaxJobs || !strides) return CONV3P_ERR_INVALID_ARGUMENT;
    Dims d{B, N, 0, 0, fz, fy, fx, 0, 0};
    for (int k = 0; k < K; ++k) TRY(check(d, strides + 3 * k, (double)voxel, false));
    if ((size_t)B * N == 0) return CONV3P_OK;
    if (!points) return CONV3P_ERR_INVALID_ARGUMENT;
    if (K > wh.nslots) return CONV3P_ERR_WORKSPACE;     // the stencils would evict each other
    hipStream_t s = static_cast<hipStream_t>(stream);
    // Every stencil takes the search a single prepare would give it (run_search): the fused search where it fits, the
    // tile-pair search otherwise.  The two build their pair lists in different orders, so a stencil batched into the other
    // search would give sums of other bits (e.g. the odd stencils of a stack whose other strides make an even, windowed one).
    SearchJobs<T> jobs;
    FusedJobs<T> fjobs;
    SchedJobs sjobs, fsjobs;
    int njobs = 0, nfused = 0;
    size_t lds = 0;
    bool any_window = false;
    Call<T> c;
    for (int k = 0; k < K; ++k) {
        TRY(begin_call<T>(c, d, strides + 3 * k, voxel, 0, wh, s));
        TRY(run_prep<T>(points, c));
        wh.flags |= CONV3P_CACHE_POINTS_UNCHANGED;      // the other stencils see the same points
        if (c.skip_search) continue;
        const Stencil<T> &st = c.st;
        const auto &S = c.L.slot[c.slot];
        TRY(run_cloud_min<T>(points, c));
        if (fused_ok(c) && fused_mask_depth((int)sizeof(T), c.d.ntiles, c.st.ntap, c.st.maxfull) > 0) {
            fjobs.job[nfused] = make_fused_job(c);
            fsjobs.job[nfused++] = make_sched_job(c, c.slot, true);
            continue;
        }
        any_window |= st.window != 0;
        const size_t l = search_lds_bytes(st, c.L.gtiles);
        if (l > kMaxLds) return CONV3P_ERR_UNSUPPORTED;
        lds = l > lds ? l : lds;
        SearchJob<T> &j = jobs.job[njobs++];
        j.st = st;
        j.cc = c.cc;
        j.count = S.count;
        j.tcount = S.tcount;
        j.pairs = S.pairs;
        j.segs = S.segs;
        j.qsegs = S.qsegs;
        j.qbm = S.qbm;
        j.qbm_hi = S.qbm_hi;
        sjobs.job[njobs - 1] = make_sched_job(c, c.slot, true);
    }
    if (nfused > 0) TRY(launch_fused<T>(c, fjobs, fsjobs, nfused));
    if (njobs == 0) return CONV3P_OK;
    for (int k = 0; k < njobs; ++k)   // (the tile-pair search lets fewer false positives through: its own threshold)
        sjobs.job[k].limit = kShortListsPerPoint * (unsigned long long)c.d.B * (unsigned long long)c.d.N;
#ifndef CONV3P_DEV_JOBS_IN_ORDER
    // widest stencil first (blockIdx.y ascending is the dispatch order): its boxes meet the most candidate tiles, its
    // workgroups run longest -- started last they would be the launch's tail
    for (int a = 1; a < njobs; ++a)
        for (int b2 = a; b2 > 0; --b2) {
            auto vol = [](const SearchJob<T> &j) { return (long long)j.st.step[0] * j.st.step[1] * j.st.step[2]; };
            if (vol(jobs.job[b2]) <= vol(jobs.job[b2 - 1])) break;
            std::swap(jobs.job[b2], jobs.job[b2 - 1]);
            std::swap(sjobs.job[b2], sjobs.job[b2 - 1]);
        }
#endif
    const BlockMap bm = make_blockmap(c.d);
    {
        Scope sc(K_SEARCH, s);
        auto launch = [&](auto kern) {
            launch_lds(kern, dim3(grid_of(bm), njobs), dim3(256), lds, s, c.L.pts, c.L.boxes, c.d.N, c.d.ntiles, c.L.gtiles,
                       c.L.ngroups, bm, jobs, c.L.cmin);
        };
        if (any_window) launch(search_multi_kernel<T, true>);    // window replication is a no-op for odd extents
        else launch(search_multi_kernel<T, false>);
        hipLaunchKernelGGL(tile_sched_kernel, dim3(8, njobs), dim3(1024), 0, s, sjobs, c.d.B, c.d.ntiles, c.L.ngroups,
                           bm.rounds * c.d.ntiles);
    }
    return hip_ok();
}

}  // namespace
