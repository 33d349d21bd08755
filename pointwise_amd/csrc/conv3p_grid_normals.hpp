// conv3p_grid_normals.hpp -- per-voxel surface normals and curvature from the voxel grid (conv3p_grid_normals_f32).
//
// include/conv3p.h defines the result by the rules R1-R6 and tests/grid_normals_ref.py restates it in numpy.  One kernel,
// one launch:
//
//   grid_normals_kernel   a thread per voxel, workgroups looping over the voxels.  The thread reads the 27 words of its row
//                         of the neighbour table, clamps every word that is no sample to its own number (so the 27 x 3
//                         gathers are unconditional, in bounds, and all in flight at once), and keeps the 81 differences
//                         q_u = p_u - p_v in registers for the two passes of R3: the chain of the mean, then the chains of
//                         the six products.  R3's chains run in ascending t, so they are serial whatever gathers: with a
//                         lane per candidate every addition would be a cross-lane move plus an add in every lane of the
//                         group (about 240 wave instructions for two voxels); with a thread per voxel they are about 570
//                         lane operations, 9 wave instructions a voxel.  Every loop over t is fully unrolled and a sample is
//                         a bit of one mask word, so no array is indexed at run time: no private segment.
//
//                         R5 is a cyclic Jacobi iteration of kNormalsSweeps sweeps IN FLOAT64 on the float32 moments: the
//                         moments are exact inputs (R3 defines them to the bit), and rotations in float64 leave the
//                         eigenvector with the rounding of its conversion to float32 and nothing else -- an angle error of
//                         order 2^-24 against R5's bound of 64 * 2^-24 * l2 / (l1 - l0), which a float32 solver meets only
//                         by a constant.  Per voxel that is 18 rotations, three divisions or roots each; the gathers, not
//                         these, set the time.  The sweep count is fixed, every rotation is taken (one whose off-diagonal
//                         entry is 0 is the identity by a select), so two calls give the same bits.
//
// R4, R5 / R6 and the stores are functions (normals_flag, normals_solve, normals_store): grid_knn_normals_kernel of
// conv3p_grid_knn.hpp, the same rules on the neighbours of a k-NN table, calls them too.
//
// The only atomics are the integer adds of the four counts (per thread into LDS after its loop, then one add per workgroup
// and count); every output word is written once by a plain store; a voxel's result depends on its own inputs alone, so
// nothing depends on the launch geometry.
#pragma once

#include "conv3p_grid_interp.hpp"

namespace conv3p {

constexpr int kNormalsThreads = 256;
constexpr int kNormalsMaxGrid = 2048;           // eight workgroups a CU: the rest is the voxel loop
constexpr int kNormalsSweeps = 6;               // off-diagonal mass falls quadratically: 1e-16 of the trace well before
constexpr int kNormalsMinNeighbors = 3;

__device__ __forceinline__ bool normals_finite(float x) { return fabsf(x) < INFINITY; }   // false for a NaN too

// One Jacobi rotation in the (p, q) plane of a symmetric 3 x 3 matrix, r the third index: a_pq becomes 0.  vNp, vNq are
// the columns p and q of the accumulated eigenvectors.
__device__ __forceinline__ void normals_rotate(double &app, double &aqq, double &apq, double &arp, double &arq, double &v0p,
                                               double &v0q, double &v1p, double &v1q, double &v2p, double &v2q)
{
    const double theta = (aqq - app) / (2.0 * apq);      // apq == 0: never used
    const double t = apq != 0.0 ? copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0)) : 0.0;   // theta inf: 0
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    app = app - t * apq;
    aqq = aqq + t * apq;
    apq = 0.0;
    const double rp = c * arp - s * arq, rq = s * arp + c * arq;
    arp = rp;
    arq = rq;
    const double a0 = c * v0p - s * v0q, b0 = s * v0p + c * v0q;
    const double a1 = c * v1p - s * v1q, b1 = s * v1p + c * v1q;
    const double a2 = c * v2p - s * v2q, b2 = s * v2p + c * v2q;
    v0p = a0; v0q = b0; v1p = a1; v1q = b1; v2p = a2; v2q = b2;
}

// R5 and R6 for a voxel with flags 0: the unit eigenvector of the smallest eigenvalue of the moments' covariance, oriented,
// and the curvature.  p is the voxel's representative.
__device__ __forceinline__ void normals_solve(float cxx, float cxy, float cxz, float cyy, float cyz, float czz, float px, float py,
                                              float pz, int v, const int32_t *voxel_room, const float *viewpoint, int V,
                                              float &nx, float &ny, float &nz, float &cv)
{
    double a00 = cxx, a01 = cxy, a02 = cxz, a11 = cyy, a12 = cyz, a22 = czz;
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
#pragma unroll
    for (int sweep = 0; sweep < kNormalsSweeps; ++sweep) {
        normals_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
        normals_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
        normals_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
    }
    const int k = (a00 <= a11 && a00 <= a22) ? 0 : (a11 <= a22 ? 1 : 2);     // the lowest of equal eigenvalues
    const double l0 = k == 0 ? a00 : (k == 1 ? a11 : a22);
    const double ex = k == 0 ? v00 : (k == 1 ? v01 : v02);
    const double ey = k == 0 ? v10 : (k == 1 ? v11 : v12);
    const double ez = k == 0 ? v20 : (k == 1 ? v21 : v22);
    const double len = sqrt((ex * ex + ey * ey) + ez * ez);
    nx = (float)(ex / len); ny = (float)(ey / len); nz = (float)(ez / len);
    cv = (float)(l0 / ((a00 + a11) + a22));
    cv = fminf(fmaxf(cv, 0.0f), 1.0f / 3.0f);
    float s = 0.0f;                              // R6, on the float32 vector about to be stored
    bool have = false;
    if (viewpoint) {
        int r = 0;
        if (V > 1) r = voxel_room ? voxel_room[v] : -1;
        if (r >= 0 && r < V) {
            const float *wv = viewpoint + (size_t)r * 3;
            s = ((wv[0] - px) * nx + (wv[1] - py) * ny) + (wv[2] - pz) * nz;
            have = normals_finite(s) && s != 0.0f;
        }
    }
    bool flip;
    if (have) {
        flip = s < 0.0f;
    } else {                                     // the largest magnitude positive, the lowest axis of a tie
        const float ax = fabsf(nx), ay = fabsf(ny), az = fabsf(nz);
        const float top = (ax >= ay && ax >= az) ? nx : (ay >= az ? ny : nz);
        flip = top < 0.0f;
    }
    if (flip) { nx = -nx; ny = -ny; nz = -nz; }
}

// R4 from the sample count and the moments
__device__ __forceinline__ int normals_flag(int n, int min_neighbors, float mx, float my, float mz, float cxx, float cxy, float cxz,
                                            float cyy, float cyz, float czz)
{
    const bool fin = normals_finite(mx) && normals_finite(my) && normals_finite(mz) && normals_finite(cxx) &&
                     normals_finite(cxy) && normals_finite(cxz) && normals_finite(cyy) && normals_finite(cyz) &&
                     normals_finite(czz);
    const float tr = (cxx + cyy) + czz;
    return n < min_neighbors ? 1 : ((!fin || !(tr > 0.0f)) ? 2 : 0);
}

// a voxel's outputs, every word written once
__device__ __forceinline__ void normals_store(int v, float nx, float ny, float nz, float cv, int n, int fl, float mx, float my,
                                              float mz, float cxx, float cxy, float cxz, float cyy, float cyz, float czz,
                                              float *normals, float *curvature, int32_t *samples, int32_t *flags, float *moments)
{
    normals[(size_t)v * 3 + 0] = nx;
    normals[(size_t)v * 3 + 1] = ny;
    normals[(size_t)v * 3 + 2] = nz;
    curvature[v] = cv;
    samples[v] = n;
    flags[v] = fl;
    if (moments) {
        float *mo = moments + (size_t)v * 9;
        mo[0] = mx; mo[1] = my; mo[2] = mz; mo[3] = cxx; mo[4] = cxy; mo[5] = cxz; mo[6] = cyy; mo[7] = cyz; mo[8] = czz;
    }
}

__global__ __launch_bounds__(kNormalsThreads) void grid_normals_kernel(const float *voxel_data, int K, const int32_t *neigh,
                                                                       const int32_t *grid_stats, const int32_t *voxel_room,
                                                                       const float *viewpoint, int V, int M, int min_neighbors,
                                                                       float *normals, float *curvature, int32_t *samples,
                                                                       int32_t *flags, float *moments, int32_t *normal_stats)
{
    __shared__ int count_s[4];
    const int tid = threadIdx.x;
    if (tid < 4) count_s[tid] = 0;
    __syncthreads();
    int ne = grid_stats[0];
    ne = ne < 0 ? 0 : (ne > M ? M : ne);
    int c_ok = 0, c_few = 0, c_deg = 0, c_fill = 0;
    for (long long w = (long long)blockIdx.x * kNormalsThreads + tid; w < M; w += (long long)gridDim.x * kNormalsThreads) {
        const int v = (int)w;
        float mx = 0.0f, my = 0.0f, mz = 0.0f, cxx = 0.0f, cxy = 0.0f, cxz = 0.0f, cyy = 0.0f, cyz = 0.0f, czz = 0.0f;
        float nx = 0.0f, ny = 0.0f, nz = 0.0f, cv = 0.0f, px = 0.0f, py = 0.0f, pz = 0.0f;
        int n = 0, fl = -1;                              // R1
        if (v < ne) {
            const float *pv = voxel_data + (size_t)v * K;
            px = pv[0]; py = pv[1]; pz = pv[2];
            const bool own = normals_finite(px) && normals_finite(py) && normals_finite(pz);
            const int32_t *row = neigh + (size_t)v * kInterpNeigh;
            int u[kInterpNeigh];
#pragma unroll
            for (int t = 0; t < kInterpNeigh; ++t) u[t] = row[t];
            float qx[kInterpNeigh], qy[kInterpNeigh], qz[kInterpNeigh];
            unsigned mask = 0;
#pragma unroll
            for (int t = 0; t < kInterpNeigh; ++t) {     // R2: what is no sample reads the voxel's own row
                const bool in = own && u[t] >= 0 && u[t] < ne;
                const float *pu = voxel_data + (size_t)(in ? u[t] : v) * K;
                const float ax = pu[0], ay = pu[1], az = pu[2];
                const bool ok = in && normals_finite(ax) && normals_finite(ay) && normals_finite(az);
                qx[t] = ax - px; qy[t] = ay - py; qz[t] = az - pz;
                mask |= (ok ? 1u : 0u) << t;
            }
            n = __popc(mask);
            const float fn = (float)(n > 0 ? n : 1);     // n == 0: the sums are 0 and so are the moments
#pragma unroll
            for (int t = 0; t < kInterpNeigh; ++t) {     // R3: the chains in ascending t
                const bool ok = (mask >> t) & 1u;
                mx = ok ? mx + qx[t] : mx;
                my = ok ? my + qy[t] : my;
                mz = ok ? mz + qz[t] : mz;
            }
            mx = mx / fn; my = my / fn; mz = mz / fn;
#pragma unroll
            for (int t = 0; t < kInterpNeigh; ++t) {
                const bool ok = (mask >> t) & 1u;
                const float ex = qx[t] - mx, ey = qy[t] - my, ez = qz[t] - mz;
                cxx = ok ? cxx + ex * ex : cxx;
                cxy = ok ? cxy + ex * ey : cxy;
                cxz = ok ? cxz + ex * ez : cxz;
                cyy = ok ? cyy + ey * ey : cyy;
                cyz = ok ? cyz + ey * ez : cyz;
                czz = ok ? czz + ez * ez : czz;
            }
            cxx = cxx / fn; cxy = cxy / fn; cxz = cxz / fn; cyy = cyy / fn; cyz = cyz / fn; czz = czz / fn;
            fl = normals_flag(n, min_neighbors, mx, my, mz, cxx, cxy, cxz, cyy, cyz, czz);   // R4
        }
        if (fl == 0) normals_solve(cxx, cxy, cxz, cyy, cyz, czz, px, py, pz, v, voxel_room, viewpoint, V, nx, ny, nz, cv);   // R5, R6
        normals_store(v, nx, ny, nz, cv, n, fl, mx, my, mz, cxx, cxy, cxz, cyy, cyz, czz, normals, curvature, samples, flags, moments);
        c_ok += fl == 0;
        c_few += fl == 1;
        c_deg += fl == 2;
        c_fill += fl < 0;
    }
    if (c_ok) atomicAdd(&count_s[0], c_ok);
    if (c_few) atomicAdd(&count_s[1], c_few);
    if (c_deg) atomicAdd(&count_s[2], c_deg);
    if (c_fill) atomicAdd(&count_s[3], c_fill);
    __syncthreads();
    if (tid < 4 && count_s[tid]) atomicAdd(&normal_stats[tid], count_s[tid]);   // integers: exact in any order
}

}  // namespace conv3p
