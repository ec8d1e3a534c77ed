// The atomic-free reduction and the 6 x 6 Gauss-Newton step shared by frame-to-model tracking (hv_track.hip) and map-to-map
// registration (hv_register.hip).  One text for both, so a sum associates and a step rounds the same way in either.
//
// A linearise kernel keeps NACC float64 sums per thread - H upper triangle [0, 21) row by row, g [21, 27), the squared error [27],
// the inlier count [28], then whatever else the caller counts - and hands them to hv_gn_block_reduce: wave butterfly, LDS, one slab
// row per workgroup.  A one-workgroup solve kernel of HV_GN_SUM_THREADS threads adds the slab rows in a fixed order
// (hv_gn_slab_sum) and its thread 0 runs hv_gn_step: Cholesky, exp, the state update.  No float atomics anywhere.
#pragma once
#include "hv_common.h"

#ifdef __HIPCC__
constexpr int HV_GN_SUM_PARTS = 32; // solve workgroup: 32 parts x 32 components
constexpr int HV_GN_SUM_THREADS = HV_GN_SUM_PARTS * 32;

// The workgroup's sums of acc[0, NACC) -> row[0, NACC).  All BLOCK threads; red is LDS.
template <int NACC, int BLOCK>
__device__ __forceinline__ void hv_gn_block_reduce(const double *acc, double (*red)[NACC], double *__restrict__ row) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NACC; ++k) {
        const double s = hv_wave_sum(acc[k]);
        if (lane == 0) red[wave][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < NACC) {
        double s = red[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < BLOCK / 64; ++w) s += red[w][threadIdx.x];
        row[threadIdx.x] = s;
    }
}

// The slab's `rows` rows of NACC (<= 32) sums -> tot[0, NACC): part k adds rows k, k + 32, ..., then the parts are added in
// order.  All HV_GN_SUM_THREADS threads; part and tot are LDS; tot is complete after the caller's next barrier.
template <int NACC>
__device__ __forceinline__ void hv_gn_slab_sum(const double *__restrict__ slab, int rows, double (*part)[32], double *tot) {
    static_assert(NACC <= 32, "one component per thread of a part");
    const int c = threadIdx.x & 31, k = threadIdx.x >> 5;
    double s = 0.0;
    if (c < NACC)
        for (int r = k; r < rows; r += HV_GN_SUM_PARTS) s += slab[(int64_t)r * NACC + c];
    part[k][c] = s;
    __syncthreads();
    if (threadIdx.x < NACC) {
        double t = part[0][threadIdx.x];
        for (int q = 1; q < HV_GN_SUM_PARTS; ++q) t += part[q][threadIdx.x];
        tot[threadIdx.x] = t;
    }
}

// One step from the summed system tot (layout above; tot[28] = inliers): Cholesky H = L L^T, L y = -g, L^T xi = y.  DEGENERATE
// (-> 2, xi = 0, A untouched) below min_inliers inliers or at a pivot <= pivot_rel trace(H).  Otherwise A := exp(xi) A with
// exp(xi) = [Rodrigues(omega), t]; -> 1 when |omega| + |t| < converged, else 0.  A0 = the state before the step, g = tot[21, 27).
// One thread.  (Every loop has constant bounds and is unrolled: the 6 x 6 arrays stay in registers.)
__device__ __forceinline__ int hv_gn_step(const double *tot, double min_inliers, double pivot_rel, double converged, double *A, double *A0,
                                          double *g, double *xi) {
    double H[6][6];
    {
        int q = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = a; b < 6; ++b) H[a][b] = H[b][a] = tot[q++];
#pragma unroll
        for (int a = 0; a < 6; ++a) g[a] = tot[21 + a];
    }
    const double inliers = tot[28];
    double trH = 0.0;
#pragma unroll
    for (int a = 0; a < 6; ++a) trH += H[a][a];
    // (the values of a degenerate factorisation are not used)
    bool degenerate = inliers < min_inliers;
    double Lm[6][6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double d = H[j][j];
#pragma unroll
        for (int q = 0; q < j; ++q) d -= Lm[j][q] * Lm[j][q];
        if (!(d > pivot_rel * trH)) degenerate = true;
        Lm[j][j] = sqrt(d);
#pragma unroll
        for (int i = j + 1; i < 6; ++i) {
            double e = H[i][j];
#pragma unroll
            for (int q = 0; q < j; ++q) e -= Lm[i][q] * Lm[j][q];
            Lm[i][j] = e / Lm[j][j];
        }
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) A0[i] = A[i];
    int status = degenerate ? 2 : 0;
    {
        double y[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            double e = -g[i];
#pragma unroll
            for (int q = 0; q < i; ++q) e -= Lm[i][q] * y[q];
            y[i] = e / Lm[i][i];
        }
#pragma unroll
        for (int i = 5; i >= 0; --i) {
            double e = y[i];
#pragma unroll
            for (int q = i + 1; q < 6; ++q) e -= Lm[q][i] * xi[q];
            xi[i] = e / Lm[i][i];
        }
    }
    if (degenerate) {
#pragma unroll
        for (int i = 0; i < 6; ++i) xi[i] = 0.0;
    } else {
        const double w0 = xi[0], w1 = xi[1], w2 = xi[2];
        const double th = sqrt(w0 * w0 + w1 * w1 + w2 * w2);
        const double sa = th < 1e-8 ? 1.0 : sin(th) / th, sb = th < 1e-8 ? 0.5 : (1.0 - cos(th)) / (th * th);
        const double K[9] = {0.0, -w2, w1, w2, 0.0, -w0, -w1, w0, 0.0};
        double E[12];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const double kk = K[i * 3] * K[j] + K[i * 3 + 1] * K[3 + j] + K[i * 3 + 2] * K[6 + j];
                E[i * 4 + j] = (i == j ? 1.0 : 0.0) + sa * K[i * 3 + j] + sb * kk;
            }
            E[i * 4 + 3] = xi[3 + i];
        }
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                A[i * 4 + j] = E[i * 4] * A0[j] + E[i * 4 + 1] * A0[4 + j] + E[i * 4 + 2] * A0[8 + j] + E[i * 4 + 3] * A0[12 + j];
        const double tn = sqrt(xi[3] * xi[3] + xi[4] * xi[4] + xi[5] * xi[5]);
        if (th + tn < converged) status = 1;
    }
    return status;
}
#endif // __HIPCC__
