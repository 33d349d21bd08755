// conv3p_workgroup.hpp -- the workgroup primitives of the scene and grid family, each stated once.
//
// conv3p_scene*.hpp, conv3p_grid*.hpp and conv3p_provider.hpp build their kernels from these.  Every function is
// __device__ __forceinline__ and keeps no state; its comment is its contract: the LDS words it needs, the barriers it
// executes (a function that executes a barrier must be called by every thread of the workgroup, with the arguments the
// contract calls uniform equal in all of them), and the integer ranges it assumes.  A wave is 64 lanes and nthr, the
// workgroup's threads, is a multiple of 64 throughout.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace conv3p {

// ------------------------------------------------------------------------------------------------------------ scans
// Exclusive prefix of v over the workgroup's threads in thread order, and the total, to every thread.  lds: nthr / 64
// words of T, free to reuse once the call has returned in every thread.  Two barriers; the first one is also what lets
// a call follow another on the same lds.  tid, nthr uniform in meaning (tid the thread's own).  The sums must fit T.
template <typename T> __device__ __forceinline__ T wg_exscan(T v, T *lds, int tid, int nthr, T *total)
{
    const int lane = tid & 63, wv = tid >> 6;
    T x = v;
    for (int d = 1; d < 64; d <<= 1) {
        const T y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    __syncthreads();
    if (lane == 63) lds[wv] = x;
    __syncthreads();
    T base = 0, tot = 0;
    for (int w = 0; w < nthr / 64; ++w) {
        const T s = lds[w];
        if (w < wv) base += s;
        tot += s;
    }
    *total = tot;
    return base + x - v;
}

// Thread tid's share [*a, *b) of the elements [0, n) when every thread takes ceil(n / nthr) consecutive ones, so
// thread order is element order; empty behind the last element.  No LDS, no barrier.  0 <= n, and n + nthr and
// nthr * ceil(n / nthr) fit Index.
template <typename Index> __device__ __forceinline__ void wg_chunk(Index n, int nthr, int tid, Index *a, Index *b)
{
    const Index per = (n + nthr - 1) / nthr;
    *a = tid * per < n ? tid * per : n;
    *b = *a + per < n ? *a + per : n;
}

// x[0 .. n) -> its exclusive prefix, in place, by one workgroup over wg_chunk's shares; returns the total to every
// thread.  lds and the barriers are wg_exscan's; n uniform.  No thread reads another's share, so nothing else is needed
// between the two passes over x.
template <typename Index, typename T>
__device__ __forceinline__ T wg_exscan_inplace(T *x, Index n, T *lds, int tid, int nthr)
{
    Index a, b;
    wg_chunk(n, nthr, tid, &a, &b);
    T mine = 0;
    for (Index e = a; e < b; ++e) mine += x[e];
    T total;
    T run = wg_exscan(mine, lds, tid, nthr, &total);
    for (Index e = a; e < b; ++e) {
        const T v = x[e];
        x[e] = run;
        run += v;
    }
    return total;
}

// ------------------------------------------------------------------------------------- the stable LSD radix sort's pass
// A pass sorts 64-bit keys by the kBits bits above `shift`.  The keys are cut into sort tiles; hist is (digits, T) ints,
// T the tiles: hist[d * T + t] first holds tile t's keys of digit d, then, after the scan, the position of the first of
// them.  The three functions are the three launches of a pass; which pass runs, its buffers, shift and tile size are
// the kernel's.  Tile t is the keys [t * tile_size, min((t + 1) * tile_size, n)).  Index is the type of a key's position
// in the loops (long long where n may be within a tile of 2^31); the positions a key is sent to, like the histogram,
// are int: 0 <= n < 2^31.

// Tile `tile` counted into hist_s and the counts written to the tile's column of hist.  Returns the count of digit tid
// (0 for tid >= digits).  hist_s: 1 << kBits ints; nthr >= 1 << kBits; three barriers, the last one before hist_s may
// be used again.  All arguments but tid uniform.
template <int kBits, typename Index>
__device__ __forceinline__ int radix_hist_tile(const unsigned long long *src, Index n, int tile, int tile_size, int shift,
                                               int *hist_s, int *hist, int T, int tid, int nthr)
{
    constexpr int kDigits = 1 << kBits;
    const bool has_digit = nthr == kDigits || tid < kDigits;    // nthr is a constant at every call: no test where they are equal
    if (has_digit) hist_s[tid] = 0;
    __syncthreads();
    const Index i0 = (Index)tile * tile_size, i1 = i0 + tile_size < n ? i0 + tile_size : n;
    for (Index i = i0 + tid; i < i1; i += nthr) atomicAdd(&hist_s[(int)(src[i] >> shift) & (kDigits - 1)], 1);
    __syncthreads();
    const int count = has_digit ? hist_s[tid] : 0;
    if (has_digit) hist[(size_t)tid * T + tile] = count;
    __syncthreads();
    return count;
}

// The scan of the sorts that keep a pass's totals per digit: workgroup `digit` turns its row of the histogram (row =
// hist + digit * T) into the exclusive prefix over (digit, tile) -- the digit's first position is the sum of the totals
// of the digits below it, and the row, a tile a thread, is scanned behind that, every load coalesced.  lds: nthr / 64
// ints; nthr >= the digits; barriers: wg_exscan's, 1 + ceil(T / nthr) times; digit, T uniform.
__device__ __forceinline__ void radix_digit_scan(const int *digit_total, int *row, int T, int digit, int *lds, int tid,
                                                 int nthr)
{
    int run;
    (void)wg_exscan(tid < digit ? digit_total[tid] : 0, lds, tid, nthr, &run);
    for (int t0 = 0; t0 < T; t0 += nthr) {
        const int t = t0 + tid;
        int total;
        const int before = wg_exscan(t < T ? row[t] : 0, lds, tid, nthr, &total);
        if (t < T) row[t] = run + before;
        run += total;
    }
}

// Tile `tile` scattered by ONE WAVE (the workgroup is 64 threads), 64 keys a step in order: the lanes of equal digit
// from kBits ballots, rank = popcount below the lane, a running offset per digit in run_s, started from the tile's
// column of the scanned hist.  A key's destination depends on nothing but the input order, so the pass is stable.
// run_s: 1 << kBits ints.  Two barriers at entry (the first lets a call follow another on the same run_s) and two a step.
// All arguments but lane uniform.  Every position is a prefix of the n keys' histogram, so 0 <= pos < n holds by
// construction; the guard bounds the store all the same, on both sides in one unsigned comparison (0 <= n).
template <int kBits, typename Index>
__device__ __forceinline__ void radix_scatter_tile(const unsigned long long *src, unsigned long long *dst, int n, int tile,
                                                   int tile_size, int shift, const int *hist, int T, int *run_s, int lane)
{
    constexpr int kDigits = 1 << kBits;
    __syncthreads();
    for (int d = lane; d < kDigits; d += 64) run_s[d] = hist[(size_t)d * T + tile];
    __syncthreads();
    const Index i0 = (Index)tile * tile_size, i1 = i0 + tile_size < n ? i0 + tile_size : n;
    for (Index c0 = i0; c0 < i1; c0 += 64) {
        const Index i = c0 + lane;
        const bool valid = i < i1;
        const unsigned long long v = valid ? src[i] : 0ull;
        const int digit = (int)(v >> shift) & (kDigits - 1);
        unsigned long long peer = __ballot(valid);
        for (int bit = 0; bit < kBits; ++bit) {
            const bool one = (digit >> bit) & 1;
            const unsigned long long m = __ballot(valid && one);
            peer &= one ? m : ~m;
        }
        const int rank = __popcll(peer & ((1ull << lane) - 1ull));
        const int pos = valid ? run_s[digit] + rank : 0;
        __syncthreads();
        if (valid && rank == 0) run_s[digit] += __popcll(peer);     // one lane per digit
        __syncthreads();
        if (valid && (unsigned)pos < (unsigned)n) dst[pos] = v;
    }
}

// ----------------------------------------------------------------------------------------------- a cloud's bounding box
__device__ __forceinline__ bool scene_finite(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// min and max of x, y, z over the finite rows seen, and the number of other rows.  A record is the same in 8 words of
// global memory (7 in scene_reduce's LDS): lo[3], hi[3], bad as an int's bits; word 7 is the caller's.  min and max are
// exact and the counts integers, so folding in any order gives the same bits -- fminf is the device's min instruction,
// which takes -0.0 as below +0.0, so even a zero minimum has one sign.  No LDS, no barrier.
struct SceneRange { float lo[3], hi[3]; int bad; };

__device__ __forceinline__ void range_init(SceneRange &r)
{
    for (int a = 0; a < 3; ++a) {
        r.lo[a] = INFINITY;
        r.hi[a] = -INFINITY;
    }
    r.bad = 0;
}

__device__ __forceinline__ void range_add(SceneRange &r, float x, float y, float z)
{
    if (scene_finite(x, y, z)) {
        r.lo[0] = fminf(r.lo[0], x); r.hi[0] = fmaxf(r.hi[0], x);
        r.lo[1] = fminf(r.lo[1], y); r.hi[1] = fmaxf(r.hi[1], y);
        r.lo[2] = fminf(r.lo[2], z); r.hi[2] = fmaxf(r.hi[2], z);
    } else {
        r.bad += 1;
    }
}

__device__ __forceinline__ void range_store(const SceneRange &r, float *w)
{
    for (int a = 0; a < 3; ++a) {
        w[a] = r.lo[a];
        w[3 + a] = r.hi[a];
    }
    w[6] = __int_as_float(r.bad);
}

__device__ __forceinline__ void range_fold(SceneRange &r, const float *w)
{
    for (int a = 0; a < 3; ++a) {
        r.lo[a] = fminf(r.lo[a], w[a]);
        r.hi[a] = fmaxf(r.hi[a], w[3 + a]);
    }
    r.bad += __float_as_int(w[6]);
}

// --------------------------------------------------------------------------------------------------------- small reads
// The label of row idx, 1, 4 or 8 bytes wide, as an int32 (an int64 label keeps its low word).
__device__ __forceinline__ int32_t row_label(const void *labels, int label_bytes, size_t idx)
{
    if (label_bytes == 1) return (int32_t) static_cast<const uint8_t *>(labels)[idx];
    if (label_bytes == 4) return static_cast<const int32_t *>(labels)[idx];
    return (int32_t) static_cast<const long long *>(labels)[idx];
}

// A count that an earlier call left in stats[0] (emitted voxels, segments), held to [0, M]: whatever the word holds, an
// index below the result is inside an array of M.
__device__ __forceinline__ int clamped_count(const int32_t *stats, int M)
{
    const int n = stats[0];
    return n < 0 ? 0 : (n > M ? M : n);
}

// The first i in [lo, hi) for which below(i) is false, hi if there is none; below must be true on a prefix of the range
// and false behind it.  Terminates and calls below inside [lo, hi) only, whatever it answers.  hi - lo fits Index.
template <typename Index, typename Pred> __device__ __forceinline__ Index lower_bound(Index lo, Index hi, Pred below)
{
    while (lo < hi) {
        const Index mid = lo + ((hi - lo) >> 1);
        if (below(mid)) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// Is room_start[0 .. R] malformed?  Well formed: 0 <= room_start[0], ascending, room_start[R] <= N, and no room of more
// than max_rows rows.  One workgroup; every thread gets the answer (0 or 1).  bad_s: one int of LDS; two barriers;
// R, N, max_rows uniform.
__device__ __forceinline__ int room_start_bad(const int32_t *room_start, int R, int N, long long max_rows, int *bad_s, int tid,
                                              int nthr)
{
    if (tid == 0) *bad_s = 0;
    __syncthreads();
    bool bad = false;
    for (int i = tid; i <= R; i += nthr) {
        const int a = room_start[i];
        if (i == 0 && a < 0) bad = true;
        if (i == R && a > N) bad = true;
        if (i < R) {
            const int b = room_start[i + 1];
            if (b < a || (long long)b - (long long)a > max_rows) bad = true;
        }
    }
    if (bad) atomicOr(bad_s, 1);
    __syncthreads();
    return *bad_s;
}

}  // namespace conv3p
