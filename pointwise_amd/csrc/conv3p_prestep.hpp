// conv3p_prestep.hpp -- the host pre-step of the reference's data providers, as gfx950 kernels.
//
// The reference prepares every batch on the host with per-cloud Python loops:
//   rotate_point_cloud / jitter_point_cloud   /root/reference/modelnet_provider.py:23-75   (training augmentation)
//   sort_point_cloud_xyz / sort_point_cloud_xyz2   /root/reference/util.py:55-109          (optional cloud ordering)
//   sort_point_cloud_morton                        /root/reference/modelnet_provider.py:100-110   (the other sort_method)
// Once the op itself takes well under a millisecond per step these loops are the feed-side bottleneck, so the same
// transformations are provided on the device, operating on the batch where it already lives.  Random numbers stay
// the caller's (rotation angles on the host, Gaussian noise as a device tensor): the kernels are deterministic
// functions of their inputs, which is what makes them checkable against the reference functions.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace conv3p {

// out[b,i,:] = (float)( clip(sigma * noise[b,i,:], -clip, +clip) + (double)(float)(p[b,i,:] . R_b) )
//   R_b = [[c,0,s],[0,1,0],[-s,0,c]] (rotation about the up axis, modelnet_provider.py:34-39); the product is
//   evaluated in double and stored as float32 (rotated_data is a float32 array, :32), the jitter is added in
//   double (np.random.randn is float64, :73-74) and the sum becomes float32 when the batch is fed.
//   cs[b] = {cos, sin} (host-computed, device array); cs == nullptr: no rotation; noise == nullptr: no jitter.
// One point of it: r = the point (x, y, z), rotated when `rot` (t = {cos, sin}), plus the clipped jitter when `jit`
// (n = the point's three standard-normal samples).  The one statement of this arithmetic: augment_kernel and the
// batch provider (conv3p_provider.hpp) both call it.
__device__ __forceinline__ void augment_point(float x, float y, float z, bool rot, double2 t, bool jit, const double n[3],
                                              double sigma, double clip, float out[3])
{
    float r[3] = {x, y, z};
    if (rot) {
        // row vector times matrix, terms added in index order (np.dot on an (N,3) x (3,3) product)
        r[0] = (float)(((double)x * t.x + (double)y * 0.0) + (double)z * -t.y);
        r[1] = (float)(((double)x * 0.0 + (double)y * 1.0) + (double)z * 0.0);
        r[2] = (float)(((double)x * t.y + (double)y * 0.0) + (double)z * t.x);
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        double v = (double)r[a];
        if (jit) {
            double j = sigma * n[a];
            j = j < -clip ? -clip : (j > clip ? clip : j);          // np.clip
            v = j + v;
        }
        out[a] = (float)v;
    }
}

__global__ __launch_bounds__(256) void augment_kernel(const float *in, const double2 *__restrict__ cs,
                                                      const double *__restrict__ noise, double sigma, double clip,
                                                      float *out,   // may alias `in` (a thread reads its point before it writes it)
                                                      size_t total, int N)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const float x = in[3 * i], y = in[3 * i + 1], z = in[3 * i + 2];
        double2 t = make_double2(1.0, 0.0);
        if (cs != nullptr) t = cs[i / (size_t)N];
        double n[3] = {0.0, 0.0, 0.0};
        if (noise != nullptr) {
            n[0] = noise[3 * i];
            n[1] = noise[3 * i + 1];
            n[2] = noise[3 * i + 2];
        }
        float r[3];
        augment_point(x, y, z, cs != nullptr, t, noise != nullptr, n, sigma, clip, r);
        out[3 * i] = r[0];
        out[3 * i + 1] = r[1];
        out[3 * i + 2] = r[2];
    }
}

// Total order of float keys as unsigned integers (negative values reversed, -0 < +0, NaN after +inf like numpy's sort).
__device__ __forceinline__ uint32_t float_key(float v)
{
    const uint32_t b = __builtin_bit_cast(uint32_t, v);
    if ((b & 0x7FFFFFFFu) > 0x7F800000u) return 0xFFFFFFFEu;   // every NaN (either sign) sorts last, as numpy.argsort puts it
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

struct SortKey {
    uint32_t x, y, z, idx;
};
__device__ __forceinline__ bool key_less(const SortKey &a, const SortKey &b)
{
    if (a.x != b.x) return a.x < b.x;
    if (a.y != b.y) return a.y < b.y;
    if (a.z != b.z) return a.z < b.z;
    return a.idx < b.idx;
}

// The key of a point: numpy compares values, -0.0 == +0.0 (adding +0.0 turns -0.0 into +0.0 and changes nothing else).
__device__ __forceinline__ SortKey make_sort_key(float x, float y, float z, int i)
{
    return SortKey{float_key(x + 0.0f), float_key(y + 0.0f), float_key(z + 0.0f), (uint32_t)i};
}

// Bitonic network over keys[0 .. npad) in LDS (npad a power of two), by the whole workgroup; the keys were stored
// before a barrier, and the last stage ends in one.  Key: the element moved, Less: its strict order -- SortKey with
// KeyLess (16 bytes, up to four compares) for the xyz order, uint64_t with MortonLess (8 bytes, one compare) for the
// Morton order.
struct KeyLess {
    __device__ __forceinline__ bool operator()(const SortKey &a, const SortKey &b) const { return key_less(a, b); }
};
struct MortonLess {
    __device__ __forceinline__ bool operator()(uint64_t a, uint64_t b) const { return a < b; }
};
template <typename Key, typename Less>
__device__ __forceinline__ void bitonic_sort_keys(Key *keys, int npad, int tid, int nthr)
{
    const Less less;
    for (int k = 2; k <= npad; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (npad >> 1); t += nthr) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int l = i | j;
                const Key a = keys[i], c = keys[l];
                const bool up = (i & k) == 0;
                if (less(c, a) == up) {
                    keys[i] = c;
                    keys[l] = a;
                }
            }
            __syncthreads();
        }
}

// order[b][r] = index of the point of cloud b that comes r-th when the cloud is sorted by x, ties by y, ties by z
// (util.py:66-68: argsort by z, then STABLE argsort by y, then by x), remaining ties by original index.  One
// workgroup per cloud, bitonic network on 16-byte keys in LDS: npad (power of two >= N) * 16 bytes, N <= 8192.
// `data` rows have `ld` floats, the first three being x, y, z.  -0.0 sorts with +0.0 as in numpy (equal keys).
__global__ __launch_bounds__(1024) void sort_xyz_kernel(const float *__restrict__ data, int N, int ld, int npad,
                                                        int32_t *__restrict__ order)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    SortKey *keys = reinterpret_cast<SortKey *>(smem);
    const int b = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
    const float *cloud = data + (size_t)b * N * ld;
    for (int i = tid; i < npad; i += nthr) {
        SortKey k{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};   // padding sorts last
        if (i < N) k = make_sort_key(cloud[(size_t)i * ld + 0], cloud[(size_t)i * ld + 1], cloud[(size_t)i * ld + 2], i);
        keys[i] = k;
    }
    __syncthreads();
    bitonic_sort_keys<SortKey, KeyLess>(keys, npad, tid, nthr);
    for (int i = tid; i < N; i += nthr) order[(size_t)b * N + i] = (int32_t)keys[i].idx;
}

// ---------------------------------------------------------------------------------------------------------------
// The Morton order of a cloud (sort_method "morton" of the reference's providers, modelnet_provider.py:100-110; the
// reference calls a third-party library whose cell size is not documented, so the order is DEFINED here -- the same
// words as include/conv3p.h and DESIGN.md section 5d):
//   a row is finite if x, y and z are; lo[a], hi[a] = min, max of coordinate a over the finite rows, as double;
//   e = max_a(hi[a] - lo[a]);  s = 65536.0 / e;  q[a] = min(65535, floor((double(v[a]) - lo[a]) * s)), every
//   operation an IEEE double operation rounded on its own; e == 0: q = 0;
//   code = the 48-bit interleave, bit 3k+2 = bit k of q[x], 3k+1 of q[y], 3k of q[z]; a row that is not finite:
//   code = 2^48 - 1;  order by ascending code, ties by ascending original index.
// Sixteen bits an axis, so that code << 16 | index is ONE 64-bit key for every N <= 65536.

constexpr uint64_t kMortonPadKey = ~0ull;                     // sorts strictly last: index < N <= 8192 < 0xFFFF
constexpr uint64_t kMortonFarCode = (1ull << 48) - 1;

__device__ __forceinline__ bool morton_finite(float x, float y, float z)
{
    const uint32_t m = 0x7F800000u;
    return (__builtin_bit_cast(uint32_t, x) & m) != m && (__builtin_bit_cast(uint32_t, y) & m) != m &&
           (__builtin_bit_cast(uint32_t, z) & m) != m;
}

// The box of a cloud, as every lane of the workgroup holds it after morton_box_reduce: lo[a] and the one scale.
struct MortonBox {
    double lo[3];
    double s;              // 65536 / e; 0 when e == 0 or no row is finite (every q is 0 then)
};

// bits 0..15 of q -> bits 0, 3, 6, .., 45
__device__ __forceinline__ uint64_t morton_spread16(uint32_t q)
{
    uint64_t v = q & 0xFFFFu;
    v = (v | (v << 16)) & 0x0000FF0000FFull;
    v = (v | (v << 8)) & 0x00F00F00F00Full;
    v = (v | (v << 4)) & 0x0C30C30C30C3ull;
    v = (v | (v << 2)) & 0x249249249249ull;
    return v;
}

__device__ __forceinline__ uint64_t morton_code(float x, float y, float z, const MortonBox &box)
{
    if (!morton_finite(x, y, z)) return kMortonFarCode;
    const float v[3] = {x, y, z};
    uint32_t q[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double c = floor(__dmul_rn(__dsub_rn((double)v[a], box.lo[a]), box.s));   // >= 0: v[a] >= lo[a]
        q[a] = c < 65535.0 ? (uint32_t)c : 65535u;
    }
    return (morton_spread16(q[0]) << 2) | (morton_spread16(q[1]) << 1) | morton_spread16(q[2]);
}

__device__ __forceinline__ uint64_t make_morton_key(float x, float y, float z, int i, const MortonBox &box)
{
    return (morton_code(x, y, z, box) << 16) | (uint64_t)(uint32_t)i;
}

// A lane's running box: lo = +inf, hi = -inf before the first finite row.
struct MortonRange {
    float lo[3], hi[3];
};
__device__ __forceinline__ void morton_range_init(MortonRange &r)
{
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        r.lo[a] = __builtin_inff();
        r.hi[a] = -__builtin_inff();
    }
}
__device__ __forceinline__ void morton_range_add(MortonRange &r, float x, float y, float z)
{
    if (!morton_finite(x, y, z)) return;
    const float v[3] = {x, y, z};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        r.lo[a] = fminf(r.lo[a], v[a]);
        r.hi[a] = fmaxf(r.hi[a], v[a]);
    }
}

// The lanes' ranges -> the cloud's box, in every lane: a butterfly inside each wave, then across the (at most 16)
// waves through LDS (box_s: 16 x 6 floats).  Min and max do not depend on the order they are taken in, so the box is
// exact; nothing goes through global memory.  Every thread of the workgroup calls it; it ends behind a barrier.
__device__ __forceinline__ MortonBox morton_box_reduce(MortonRange r, float *box_s, int tid, int nthr)
{
#pragma unroll
    for (int a = 0; a < 3; ++a)
        for (int m = 32; m > 0; m >>= 1) {
            r.lo[a] = fminf(r.lo[a], __shfl_xor(r.lo[a], m, 64));
            r.hi[a] = fmaxf(r.hi[a], __shfl_xor(r.hi[a], m, 64));
        }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            box_s[(tid >> 6) * 6 + a] = r.lo[a];
            box_s[(tid >> 6) * 6 + 3 + a] = r.hi[a];
        }
    }
    __syncthreads();
    const int waves = (nthr + 63) >> 6;
    MortonBox box;
    double e = 0.0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float lo = box_s[a], hi = box_s[3 + a];
        for (int w = 1; w < waves; ++w) {
            lo = fminf(lo, box_s[w * 6 + a]);
            hi = fmaxf(hi, box_s[w * 6 + 3 + a]);
        }
        box.lo[a] = (double)lo;
        const double d = __dsub_rn((double)hi, (double)lo);     // -inf when no row is finite
        e = d > e ? d : e;
    }
    box.s = e > 0.0 ? __ddiv_rn(65536.0, e) : 0.0;
    return box;
}

// order[b][r] = index of the row of cloud b that comes r-th in the Morton order defined above.  One workgroup per
// cloud, the structure of sort_xyz_kernel: the box pass, the key pass, the network on 8-byte keys in LDS (npad * 8
// bytes, 64 KB at N = 8192), `order` last.  `data` rows have `ld` floats, the first three being x, y, z.
__global__ __launch_bounds__(1024) void sort_morton_kernel(const float *__restrict__ data, int N, int ld, int npad,
                                                           int32_t *__restrict__ order)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ float box_s[16 * 6];
    uint64_t *keys = reinterpret_cast<uint64_t *>(smem);
    const int b = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
    const float *cloud = data + (size_t)b * N * ld;
    MortonRange rg;
    morton_range_init(rg);
    for (int i = tid; i < N; i += nthr)
        morton_range_add(rg, cloud[(size_t)i * ld + 0], cloud[(size_t)i * ld + 1], cloud[(size_t)i * ld + 2]);
    const MortonBox box = morton_box_reduce(rg, box_s, tid, nthr);
    for (int i = tid; i < npad; i += nthr) {
        uint64_t k = kMortonPadKey;
        if (i < N) {
            const float *row = cloud + (size_t)i * ld;
            k = make_morton_key(row[0], row[1], row[2], i, box);
        }
        keys[i] = k;
    }
    __syncthreads();
    bitonic_sort_keys<uint64_t, MortonLess>(keys, npad, tid, nthr);
    for (int i = tid; i < N; i += nthr) order[(size_t)b * N + i] = (int32_t)(keys[i] & 0xFFFFu);
}

// dst[b][r][:] = src[b][order[b][r]][:], rows of `row_bytes` bytes (any element type: points, labels, attributes)
__global__ __launch_bounds__(256) void gather_rows_kernel(const char *__restrict__ src, const int32_t *__restrict__ order,
                                                          int N, int row_bytes, char *__restrict__ dst, size_t rows)
{
    const size_t total = rows * (size_t)row_bytes;
    if ((row_bytes & 3) == 0) {
        const int rw = row_bytes >> 2;
        const size_t tw = rows * (size_t)rw;
        const uint32_t *s = reinterpret_cast<const uint32_t *>(src);
        uint32_t *d = reinterpret_cast<uint32_t *>(dst);
        for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < tw; e += (size_t)gridDim.x * blockDim.x) {
            const size_t r = e / (size_t)rw;
            const size_t b = r / (size_t)N;
            d[e] = s[(b * N + (size_t)order[r]) * rw + (e - r * rw)];
        }
        return;
    }
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const size_t r = e / (size_t)row_bytes;
        const size_t b = r / (size_t)N;
        dst[e] = src[(b * N + (size_t)order[r]) * row_bytes + (e - r * row_bytes)];
    }
}

}  // namespace conv3p
