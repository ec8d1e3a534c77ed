// libpyslam_hipvol.so — bundle adjustment (hv_bundle_adjust, hv_bundle_linearise; contract B1-B8 in include/hipvol.h).
//
// Levenberg-Marquardt over camera poses and points (hv_lm.h: the pose graph's state, decision, pose update and CG scalars) with the
// Schur complement on the points as the inner system, never formed.  What an observation keeps between a linearisation and the CG's
// products is q = R p + t (3 doubles) and A = w s J^T J (upper triangle, 6 doubles), J = d r / d q: struct-of-arrays, 72 bytes.  Both
// Jacobians follow from them and the camera's rotation, J_camera = J [-[q]x, I] and J_point = J R, so E_o = [-[q]x, I]^T A R and a
// product never needs more than q, A and R.  Storing the two Jacobians instead would stream 27 doubles per observation and pass, three
// times as many, against some twenty multiply-adds here; the poses a pass gathers (128 bytes per camera) stay in L2.
//   pass 1 (k_bd_schur_points)  one lane per point down its list:  y_j = (C_j + lambda I)^-1 sum_o R^T A (p_t + p_w x q)
//   pass 2 (k_bd_schur_cams)    one wave per camera, lanes stride its list by 64: (S p)_i = (B_i + lambda I) p_i - sum_o [-[q]x, I]^T A R y_j
// A camera's sum is lanes by butterfly (hv_wave_sum); lane l holds the entries l, l + 64, ... of the list in order, so the order of
// the additions is a function of the list alone.  No float atomics; every sum over workgroups is taken in order by one thread.
#include <algorithm>
#include <cmath>
#include <vector>

#include "hv_common.h"
#include "hv_lm.h"

namespace {
constexpr int BD_CAMS_PER_BLOCK = PG_BLOCK / HV_WAVE; // one wave per camera

struct BdModel {
    double fx, fy, cx, cy, bf, delta2_mono, delta2_stereo, min_depth;
    int32_t huber;
};

__device__ __forceinline__ int bd_sym3(int a, int b) { return a <= b ? a * 3 - (a * (a - 1)) / 2 + (b - a) : b * 3 - (b * (b - 1)) / 2 + (a - b); }

// W = [-[q]x, I] (3 x 6): d q / d (omega, t) of q := exp(d) q
__device__ __forceinline__ void bd_W(const double *q, double *W) {
    W[0] = 0.0, W[1] = q[2], W[2] = -q[1], W[3] = 1.0, W[4] = 0.0, W[5] = 0.0;
    W[6] = -q[2], W[7] = 0.0, W[8] = q[0], W[9] = 0.0, W[10] = 1.0, W[11] = 0.0;
    W[12] = q[1], W[13] = -q[0], W[14] = 0.0, W[15] = 0.0, W[16] = 0.0, W[17] = 1.0;
}
// out = A v for the symmetric A[6]
__device__ __forceinline__ void bd_sym3_mul(const double *A, const double *v, double *out) {
#pragma unroll
    for (int i = 0; i < 3; ++i) out[i] = (A[bd_sym3(i, 0)] * v[0] + A[bd_sym3(i, 1)] * v[1]) + A[bd_sym3(i, 2)] * v[2];
}
// out = R v / R^T v for the rotation rows of a 4 x 4 pose
__device__ __forceinline__ void bd_rot(const double *T, const double *v, double *out) {
#pragma unroll
    for (int i = 0; i < 3; ++i) out[i] = (T[i * 4] * v[0] + T[i * 4 + 1] * v[1]) + T[i * 4 + 2] * v[2];
}
__device__ __forceinline__ void bd_rot_t(const double *T, const double *v, double *out) {
#pragma unroll
    for (int i = 0; i < 3; ++i) out[i] = (T[i] * v[0] + T[4 + i] * v[1]) + T[8 + i] * v[2];
}
// acc[a] += sum_i W[i][a] h[i]
__device__ __forceinline__ void bd_Wt_add(const double *W, const double *h, double *acc) {
#pragma unroll
    for (int a = 0; a < 6; ++a) acc[a] += (W[a] * h[0] + W[6 + a] * h[1]) + W[12 + a] * h[2];
}
// acc[pg_tri(a, b)] += (W^T G W)(a, b), a <= b, for the symmetric G[6]
__device__ __forceinline__ void bd_WtGW_add(const double *W, const double *G, double *acc) {
    double GW[18];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int b = 0; b < 6; ++b) GW[i * 6 + b] = (G[bd_sym3(i, 0)] * W[b] + G[bd_sym3(i, 1)] * W[6 + b]) + G[bd_sym3(i, 2)] * W[12 + b];
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = a; b < 6; ++b) acc[pg_tri(a, b)] += (W[a] * GW[b] + W[6 + a] * GW[6 + b]) + W[12 + a] * GW[12 + b];
}

// the four waves' values of lane 0 in order -> thread 0 (sum or max).  All PG_BLOCK threads.
__device__ __forceinline__ double bd_waves_sum(double x, double *red) {
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    const double s = ((red[0] + red[1]) + red[2]) + red[3];
    __syncthreads();
    return s;
}
__device__ __forceinline__ double bd_waves_max(double x, double *red) {
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    const double s = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    __syncthreads();
    return s;
}

// One observation at the state (T, P): q, r, chi2, the weight, rho and - where asked for - A and g_q = w s J^T r.  One lane per
// observation.  first: an active observation with q_z <= min_depth is switched off and marked in `behind` (B4); later such an
// observation makes the workgroup's sum not-a-number.  part_F[workgroup] = the workgroup's sum of rho.
__global__ __launch_bounds__(PG_BLOCK) void k_bd_linearise(const double *__restrict__ T, const double *__restrict__ P,
                                                            const int32_t *__restrict__ idx, const double *__restrict__ meas,
                                                            uint8_t *__restrict__ act, uint8_t *__restrict__ behind, int first, int O, BdModel K,
                                                            double *__restrict__ q_out, double *__restrict__ A_out, double *__restrict__ g_out,
                                                            double *__restrict__ chi_out, double *__restrict__ r_out, double *__restrict__ w_out,
                                                            double *__restrict__ part_F) {
    __shared__ double red[4];
    const int o = blockIdx.x * PG_BLOCK + threadIdx.x;
    double cost = 0.0;
    if (o < O) {
        bool on = act[o] != 0;
        double q[3] = {0.0, 0.0, 0.0}, A[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, g[3] = {0.0, 0.0, 0.0}, r[3] = {0.0, 0.0, 0.0};
        double chi = 0.0, w = 0.0;
        if (on) {
            const double *Tc = T + (size_t)idx[2 * o] * 16, *p = P + (size_t)idx[2 * o + 1] * 3;
#pragma unroll
            for (int i = 0; i < 3; ++i) q[i] = ((Tc[i * 4] * p[0] + Tc[i * 4 + 1] * p[1]) + Tc[i * 4 + 2] * p[2]) + Tc[i * 4 + 3];
            if (!(q[2] > K.min_depth)) {
                on = false;
                q[0] = 0.0, q[1] = 0.0, q[2] = 0.0;
                if (first)
                    act[o] = 0, behind[o] = 1;
                else
                    cost = nan("");
            }
        }
        if (on) {
            const double u = meas[4 * (size_t)o], vv = meas[4 * (size_t)o + 1], ur = meas[4 * (size_t)o + 2], s = meas[4 * (size_t)o + 3];
            const bool stereo = isfinite(ur);
            const double iz = 1.0 / q[2], xz = q[0] * iz, yz = q[1] * iz;
            const double pu = K.fx * xz + K.cx;
            r[0] = u - pu;
            r[1] = vv - (K.fy * yz + K.cy);
            r[2] = stereo ? ur - (pu - K.bf * iz) : 0.0;
            chi = s * ((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]);
            const double d2 = stereo ? K.delta2_stereo : K.delta2_mono;
            w = 1.0, cost = chi;
            if (K.huber && chi > d2) {
                const double sq = sqrt(chi), d = sqrt(d2);
                w = d / sq;
                cost = 2.0 * d * sq - d2;
            }
            // J = d r / d q, rows u, v, u_r
            const double J[9] = {-K.fx * iz, 0.0, K.fx * xz * iz, 0.0, -K.fy * iz, K.fy * yz * iz,
                                 stereo ? -K.fx * iz : 0.0, 0.0, stereo ? (K.fx * xz - K.bf * iz) * iz : 0.0};
            const double ws = w * s;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
#pragma unroll
                for (int b = a; b < 3; ++b) A[bd_sym3(a, b)] = ws * ((J[a] * J[b] + J[3 + a] * J[3 + b]) + J[6 + a] * J[6 + b]);
                g[a] = ws * ((J[a] * r[0] + J[3 + a] * r[1]) + J[6 + a] * r[2]);
            }
        }
        if (q_out != nullptr) {
#pragma unroll
            for (int a = 0; a < 3; ++a) q_out[(size_t)a * O + o] = q[a], g_out[(size_t)a * O + o] = g[a];
#pragma unroll
            for (int a = 0; a < 6; ++a) A_out[(size_t)a * O + o] = A[a];
        }
        if (chi_out != nullptr) chi_out[o] = chi;
        if (w_out != nullptr) w_out[o] = w;
        if (r_out != nullptr)
#pragma unroll
            for (int a = 0; a < 3; ++a) r_out[(size_t)a * O + o] = r[a];
    }
    const double tot = pg_block_sum(cost, red);
    if (threadIdx.x == 0 && part_F != nullptr) part_F[blockIdx.x] = tot;
}

// One lane per point down its list: C_j = sum R^T A R (upper triangle) and b_j = sum R^T g_q.  With the points fixed both are
// zero.  part_maxd / part_grad[workgroup]: the largest diagonal entry of C and the largest |b| of the workgroup's points.
__global__ __launch_bounds__(PG_BLOCK) void k_bd_gather_points(const int32_t *__restrict__ row, const int32_t *__restrict__ ent,
                                                                const int32_t *__restrict__ idx, const double *__restrict__ T,
                                                                const double *__restrict__ A6, const double *__restrict__ gq, int M, int O,
                                                                int points_free, double *__restrict__ C6, double *__restrict__ bp,
                                                                double *__restrict__ part_maxd, double *__restrict__ part_grad) {
    __shared__ double red[4];
    const int j = blockIdx.x * PG_BLOCK + threadIdx.x;
    double maxd = 0.0, maxg = 0.0;
    if (j < M) {
        double C[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, b[3] = {0.0, 0.0, 0.0};
        if (points_free) {
            for (int k = row[j]; k < row[j + 1]; ++k) {
                const int o = ent[k];
                const double *R = T + (size_t)idx[2 * o] * 16;
                double A[6], g[3], h[3], AR[9];
#pragma unroll
                for (int a = 0; a < 6; ++a) A[a] = A6[(size_t)a * O + o];
#pragma unroll
                for (int a = 0; a < 3; ++a) g[a] = gq[(size_t)a * O + o];
#pragma unroll
                for (int i = 0; i < 3; ++i)
#pragma unroll
                    for (int l = 0; l < 3; ++l)
                        AR[i * 3 + l] = (A[bd_sym3(i, 0)] * R[l] + A[bd_sym3(i, 1)] * R[4 + l]) + A[bd_sym3(i, 2)] * R[8 + l];
#pragma unroll
                for (int a = 0; a < 3; ++a)
#pragma unroll
                    for (int c = a; c < 3; ++c) C[bd_sym3(a, c)] += (R[a] * AR[c] + R[4 + a] * AR[3 + c]) + R[8 + a] * AR[6 + c];
                bd_rot_t(R, g, h);
#pragma unroll
                for (int a = 0; a < 3; ++a) b[a] += h[a];
            }
        }
#pragma unroll
        for (int a = 0; a < 6; ++a) C6[(size_t)a * M + j] = C[a];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            bp[(size_t)a * M + j] = b[a];
            maxg = fmax(maxg, fabs(b[a]));
            maxd = fmax(maxd, C[bd_sym3(a, a)]);
        }
    }
    const double md = pg_block_max(maxd, red), mg = pg_block_max(maxg, red);
    if (threadIdx.x == 0) part_maxd[blockIdx.x] = md, part_grad[blockIdx.x] = mg;
}

// One wave per camera, lanes stride its list: B_i = sum W^T A W (upper triangle) and b_i = sum W^T g_q; a fixed camera gets b = 0.
__global__ __launch_bounds__(PG_BLOCK) void k_bd_gather_cams(const int32_t *__restrict__ row, const int32_t *__restrict__ ent,
                                                              const double *__restrict__ q3, const double *__restrict__ A6,
                                                              const double *__restrict__ gq, const uint8_t *__restrict__ cam_fixed, int N, int O,
                                                              double *__restrict__ B21, double *__restrict__ bc, double *__restrict__ part_maxd,
                                                              double *__restrict__ part_grad) {
    __shared__ double red[4];
    const int lane = threadIdx.x & 63, i = blockIdx.x * BD_CAMS_PER_BLOCK + (threadIdx.x >> 6);
    double maxd = 0.0, maxg = 0.0;
    if (i < N) { // wave-uniform
        double B[21], b[6];
#pragma unroll
        for (int a = 0; a < 21; ++a) B[a] = 0.0;
#pragma unroll
        for (int a = 0; a < 6; ++a) b[a] = 0.0;
        for (int k = row[i] + lane; k < row[i + 1]; k += HV_WAVE) {
            const int o = ent[k];
            double q[3], A[6], g[3], W[18];
#pragma unroll
            for (int a = 0; a < 3; ++a) q[a] = q3[(size_t)a * O + o], g[a] = gq[(size_t)a * O + o];
#pragma unroll
            for (int a = 0; a < 6; ++a) A[a] = A6[(size_t)a * O + o];
            bd_W(q, W);
            bd_WtGW_add(W, A, B);
            bd_Wt_add(W, g, b);
        }
#pragma unroll
        for (int a = 0; a < 21; ++a) B[a] = hv_wave_sum(B[a]);
#pragma unroll
        for (int a = 0; a < 6; ++a) b[a] = hv_wave_sum(b[a]);
        if (lane == 0) {
            const bool fixed = cam_fixed[i] != 0;
#pragma unroll
            for (int a = 0; a < 21; ++a) B21[(size_t)a * N + i] = B[a];
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                const double v = fixed ? 0.0 : b[a];
                bc[(size_t)a * N + i] = v;
                maxg = fmax(maxg, fabs(v));
                if (!fixed) maxd = fmax(maxd, B[pg_tri(a, a)]);
            }
        }
    }
    const double md = bd_waves_max(maxd, red), mg = bd_waves_max(maxg, red);
    if (threadIdx.x == 0) part_maxd[blockIdx.x] = md, part_grad[blockIdx.x] = mg;
}

// One thread: lambda_0 = lambda_scale max diag H at the call's first iteration, and max |b|, over the n parts of cameras and points.
// grad_out[0] receives the maximum (the rest of that array stays zero: k_pg_decide takes its maximum).
__global__ void k_bd_lambda(PgState *__restrict__ S, const double *__restrict__ part_maxd, const double *__restrict__ part_grad, int n,
                            double lambda_scale, double *__restrict__ grad_out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double m = 0.0, g = 0.0;
    for (int k = 0; k < n; ++k) m = fmax(m, part_maxd[k]), g = fmax(g, part_grad[k]);
    if (S->iter == 0) S->lambda = lambda_scale * m;
    grad_out[0] = g;
}

// One lane per point: (C_j + lambda I)^-1 through its Cholesky factor, and w_j = that times b_j.  Fixed points: both zero.
__global__ __launch_bounds__(PG_BLOCK) void k_bd_invert_points(PgState *__restrict__ S, const double *__restrict__ C6,
                                                                const double *__restrict__ bp, int M, int points_free,
                                                                double *__restrict__ Ci6, double *__restrict__ wp) {
    const int j = blockIdx.x * PG_BLOCK + threadIdx.x;
    if (j >= M) return;
    double Ci[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, w[3] = {0.0, 0.0, 0.0};
    if (points_free) {
        const double lambda = S->lambda;
        const double a00 = C6[j] + lambda, a01 = C6[(size_t)M + j], a02 = C6[2 * (size_t)M + j];
        const double a11 = C6[3 * (size_t)M + j] + lambda, a12 = C6[4 * (size_t)M + j], a22 = C6[5 * (size_t)M + j] + lambda;
        bool bad = !(a00 > 0.0);
        const double l00 = sqrt(bad ? 1.0 : a00), l10 = a01 / l00, l20 = a02 / l00;
        double d = a11 - l10 * l10;
        if (!(d > 0.0)) bad = true, d = 1.0;
        const double l11 = sqrt(d), l21 = (a12 - l20 * l10) / l11;
        d = (a22 - l20 * l20) - l21 * l21;
        if (!(d > 0.0)) bad = true, d = 1.0;
        const double l22 = sqrt(d);
        const double i00 = 1.0 / l00, i11 = 1.0 / l11, i22 = 1.0 / l22;
        const double i10 = -(l10 * i00) * i11, i21 = -(l21 * i11) * i22, i20 = -(l20 * i00 + l21 * i10) * i22;
        if (bad) {
            atomicOr(&S->bad, 1);
        } else {
            Ci[0] = (i00 * i00 + i10 * i10) + i20 * i20, Ci[1] = i10 * i11 + i20 * i21, Ci[2] = i20 * i22;
            Ci[3] = i11 * i11 + i21 * i21, Ci[4] = i21 * i22, Ci[5] = i22 * i22;
            const double b[3] = {bp[j], bp[(size_t)M + j], bp[2 * (size_t)M + j]};
            bd_sym3_mul(Ci, b, w);
        }
    }
#pragma unroll
    for (int a = 0; a < 6; ++a) Ci6[(size_t)a * M + j] = Ci[a];
#pragma unroll
    for (int a = 0; a < 3; ++a) wp[(size_t)a * M + j] = w[a];
}

// One wave per camera: its block of S, (B_i + lambda I) - sum_o E_o (C_j + lambda I)^-1 E_o^T, factored; and the reduced right-hand
// side r_i = -(b_i - sum_o E_o w_j).  E_o = W^T A R.  A fixed camera gets the unit factor and r = 0.
__global__ __launch_bounds__(PG_BLOCK) void k_bd_factor_cams(PgState *__restrict__ S, const int32_t *__restrict__ row,
                                                              const int32_t *__restrict__ ent, const int32_t *__restrict__ idx,
                                                              const double *__restrict__ T, const double *__restrict__ q3,
                                                              const double *__restrict__ A6, const double *__restrict__ Ci6,
                                                              const double *__restrict__ wp, const double *__restrict__ B21,
                                                              const double *__restrict__ bc, const uint8_t *__restrict__ cam_fixed, int N, int M,
                                                              int O, double *__restrict__ L21, double *__restrict__ rr) {
    const int lane = threadIdx.x & 63, i = blockIdx.x * BD_CAMS_PER_BLOCK + (threadIdx.x >> 6);
    if (i >= N) return;
    const double *R = T + (size_t)i * 16;
    double acc[21], ew[6];
#pragma unroll
    for (int a = 0; a < 21; ++a) acc[a] = 0.0;
#pragma unroll
    for (int a = 0; a < 6; ++a) ew[a] = 0.0;
    for (int k = row[i] + lane; k < row[i + 1]; k += HV_WAVE) {
        const int o = ent[k], j = idx[2 * o + 1];
        double q[3], A[6], Ci[6], w[3], W[18];
#pragma unroll
        for (int a = 0; a < 3; ++a) q[a] = q3[(size_t)a * O + o], w[a] = wp[(size_t)a * M + j];
#pragma unroll
        for (int a = 0; a < 6; ++a) A[a] = A6[(size_t)a * O + o], Ci[a] = Ci6[(size_t)a * M + j];
        // X = R Ci, RC = X R^T (symmetric), Y = A RC, G = Y A (symmetric)
        double X[9], RC[6], Y[9], G[6];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) X[r * 3 + c] = (R[r * 4] * Ci[bd_sym3(0, c)] + R[r * 4 + 1] * Ci[bd_sym3(1, c)]) + R[r * 4 + 2] * Ci[bd_sym3(2, c)];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = r; c < 3; ++c) RC[bd_sym3(r, c)] = (X[r * 3] * R[c * 4] + X[r * 3 + 1] * R[c * 4 + 1]) + X[r * 3 + 2] * R[c * 4 + 2];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = 0; c < 3; ++c) Y[r * 3 + c] = (A[bd_sym3(r, 0)] * RC[bd_sym3(0, c)] + A[bd_sym3(r, 1)] * RC[bd_sym3(1, c)]) + A[bd_sym3(r, 2)] * RC[bd_sym3(2, c)];
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
            for (int c = r; c < 3; ++c) G[bd_sym3(r, c)] = (Y[r * 3] * A[bd_sym3(0, c)] + Y[r * 3 + 1] * A[bd_sym3(1, c)]) + Y[r * 3 + 2] * A[bd_sym3(2, c)];
        bd_W(q, W);
        bd_WtGW_add(W, G, acc);
        double rw[3], h[3];
        bd_rot(R, w, rw);
        bd_sym3_mul(A, rw, h);
        bd_Wt_add(W, h, ew);
    }
#pragma unroll
    for (int a = 0; a < 21; ++a) acc[a] = hv_wave_sum(acc[a]);
#pragma unroll
    for (int a = 0; a < 6; ++a) ew[a] = hv_wave_sum(ew[a]);
    if (lane != 0) return;
    double Sii[21], L[21];
#pragma unroll
    for (int a = 0; a < 21; ++a) Sii[a] = B21[(size_t)a * N + i] - acc[a];
    const bool fixed = cam_fixed[i] != 0;
    bool bad = pg_chol6(Sii, S->lambda, L);
    if (fixed) {
        bad = false;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int c = a; c < 6; ++c) L[pg_tri(a, c)] = a == c ? 1.0 : 0.0;
    }
    if (bad) atomicOr(&S->bad, 1);
#pragma unroll
    for (int a = 0; a < 21; ++a) L21[(size_t)a * N + i] = L[a];
#pragma unroll
    for (int a = 0; a < 6; ++a) rr[(size_t)a * N + i] = fixed ? 0.0 : -(bc[(size_t)a * N + i] - ew[a]);
}

// One lane per camera: the start of the CG, x = 0, z = P^-1 r, part_rz
__global__ __launch_bounds__(PG_BLOCK) void k_bd_cg_start(const double *__restrict__ L21, const double *__restrict__ rr, int N,
                                                           double *__restrict__ x, double *__restrict__ z, double *__restrict__ part_rz) {
    __shared__ double red[4];
    const int i = blockIdx.x * PG_BLOCK + threadIdx.x;
    double rz = 0.0;
    if (i < N) {
        double L[21], r6[6], z6[6];
#pragma unroll
        for (int a = 0; a < 21; ++a) L[a] = L21[(size_t)a * N + i];
#pragma unroll
        for (int a = 0; a < 6; ++a) r6[a] = rr[(size_t)a * N + i];
        pg_precond(L, r6, z6);
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            x[(size_t)a * N + i] = 0.0;
            z[(size_t)a * N + i] = z6[a];
            rz += r6[a] * z6[a];
        }
    }
    const double tot = pg_block_sum(rz, red);
    if (threadIdx.x == 0) part_rz[blockIdx.x] = tot;
}

// Pass 1, one lane per point down its list: y_j = (C_j + lambda I)^-1 sum_o R^T A (p_t + p_w x q) for the camera vector p.
// j >= 0: CG iteration j (a no-op once the CG is done), y is written.  j < 0: the back-substitution with p = the CG's x:
// d_j = -(w_j + y_j), Pn = P + d, part_dd = sum d.d, part_pred = sum d.(lambda d - b).
__global__ __launch_bounds__(PG_BLOCK) void k_bd_schur_points(const PgState *__restrict__ S, int j_cg, const int32_t *__restrict__ row,
                                                               const int32_t *__restrict__ ent, const int32_t *__restrict__ idx,
                                                               const double *__restrict__ T, const double *__restrict__ q3,
                                                               const double *__restrict__ A6, const double *__restrict__ Ci6,
                                                               const double *__restrict__ p, int N, int M, int O, double *__restrict__ y,
                                                               const double *__restrict__ wp, const double *__restrict__ bp,
                                                               const double *__restrict__ P, double *__restrict__ Pn,
                                                               double *__restrict__ part_dd, double *__restrict__ part_pred) {
    __shared__ double red[4];
    if (j_cg >= 0 && S->done[j_cg & 1]) return;
    const int j = blockIdx.x * PG_BLOCK + threadIdx.x;
    double dd = 0.0, pred = 0.0;
    if (j < M) {
        double t[3] = {0.0, 0.0, 0.0};
        for (int k = row[j]; k < row[j + 1]; ++k) {
            const int o = ent[k], c = idx[2 * o];
            const double *R = T + (size_t)c * 16;
            double q[3], A[6], pc[6], e[3], f[3], h[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) q[a] = q3[(size_t)a * O + o];
#pragma unroll
            for (int a = 0; a < 6; ++a) A[a] = A6[(size_t)a * O + o], pc[a] = p[(size_t)a * N + c];
            e[0] = pc[3] + (pc[1] * q[2] - pc[2] * q[1]);
            e[1] = pc[4] + (pc[2] * q[0] - pc[0] * q[2]);
            e[2] = pc[5] + (pc[0] * q[1] - pc[1] * q[0]);
            bd_sym3_mul(A, e, f);
            bd_rot_t(R, f, h);
#pragma unroll
            for (int a = 0; a < 3; ++a) t[a] += h[a];
        }
        double Ci[6], yj[3];
#pragma unroll
        for (int a = 0; a < 6; ++a) Ci[a] = Ci6[(size_t)a * M + j];
        bd_sym3_mul(Ci, t, yj);
        if (j_cg >= 0) {
#pragma unroll
            for (int a = 0; a < 3; ++a) y[(size_t)a * M + j] = yj[a];
        } else {
            const double lambda = S->lambda;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const double d = -(wp[(size_t)a * M + j] + yj[a]);
                Pn[(size_t)j * 3 + a] = P[(size_t)j * 3 + a] + d;
                dd += d * d;
                pred += d * (lambda * d - bp[(size_t)a * M + j]);
            }
        }
    }
    if (j_cg < 0) {
        const double sdd = pg_block_sum(dd, red), sp = pg_block_sum(pred, red);
        if (threadIdx.x == 0) part_dd[blockIdx.x] = sdd, part_pred[blockIdx.x] = sp;
    }
}

// Pass 2, one wave per camera: (S p)_i = (B_i + lambda I) p_i - sum_o W^T A R y_j (0 for a fixed camera), part_pq
__global__ __launch_bounds__(PG_BLOCK) void k_bd_schur_cams(const PgState *__restrict__ S, int j_cg, const int32_t *__restrict__ row,
                                                             const int32_t *__restrict__ ent, const int32_t *__restrict__ idx,
                                                             const double *__restrict__ T, const double *__restrict__ q3,
                                                             const double *__restrict__ A6, const double *__restrict__ y,
                                                             const double *__restrict__ B21, const uint8_t *__restrict__ cam_fixed,
                                                             const double *__restrict__ p, int N, int M, int O, double *__restrict__ qv,
                                                             double *__restrict__ part_pq) {
    __shared__ double red[4];
    if (S->done[j_cg & 1]) return;
    const int lane = threadIdx.x & 63, i = blockIdx.x * BD_CAMS_PER_BLOCK + (threadIdx.x >> 6);
    double pq = 0.0;
    if (i < N) { // wave-uniform
        const double *R = T + (size_t)i * 16;
        double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int k = row[i] + lane; k < row[i + 1]; k += HV_WAVE) {
            const int o = ent[k], j = idx[2 * o + 1];
            double q[3], A[6], yj[3], ry[3], h[3], W[18];
#pragma unroll
            for (int a = 0; a < 3; ++a) q[a] = q3[(size_t)a * O + o], yj[a] = y[(size_t)a * M + j];
#pragma unroll
            for (int a = 0; a < 6; ++a) A[a] = A6[(size_t)a * O + o];
            bd_rot(R, yj, ry);
            bd_sym3_mul(A, ry, h);
            bd_W(q, W);
            bd_Wt_add(W, h, acc);
        }
#pragma unroll
        for (int a = 0; a < 6; ++a) acc[a] = hv_wave_sum(acc[a]);
        if (lane == 0) {
            const double lambda = S->lambda;
            const bool fixed = cam_fixed[i] != 0;
            double B[21], pi[6];
#pragma unroll
            for (int a = 0; a < 21; ++a) B[a] = B21[(size_t)a * N + i];
#pragma unroll
            for (int a = 0; a < 6; ++a) pi[a] = p[(size_t)a * N + i];
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                double s = lambda * pi[a];
#pragma unroll
                for (int c = 0; c < 6; ++c) s += B[a <= c ? pg_tri(a, c) : pg_tri(c, a)] * pi[c];
                const double v = fixed ? 0.0 : s - acc[a];
                qv[(size_t)a * N + i] = v;
                pq += pi[a] * v;
            }
        }
    }
    const double tot = bd_waves_sum(pq, red);
    if (threadIdx.x == 0) part_pq[blockIdx.x] = tot;
}

// the operands on the host, for the checks and the incidence lists: the caller's arrays (HV_HOST) or copies (HV_DEVICE; one wait)
struct BdHostView {
    std::vector<double> cams, pts, meas;
    std::vector<int32_t> idx;
    std::vector<uint8_t> fixed, active;
    const double *p_cams, *p_pts, *p_meas;
    const int32_t *p_idx;
    const uint8_t *p_fixed, *p_active;
};
int bd_host_view(hv_volume *v, BdHostView &h, const double *cams, int64_t N, const double *pts, int64_t M, const uint8_t *fixed,
                 const int32_t *idx, const double *meas, const uint8_t *active, int64_t O, int32_t loc) {
    h.p_cams = cams, h.p_pts = pts, h.p_fixed = fixed, h.p_idx = idx, h.p_meas = meas, h.p_active = active;
    if (loc == HV_HOST) return HV_OK;
    h.cams.resize((size_t)N * 16), h.pts.resize((size_t)M * 3), h.idx.resize((size_t)O * 2), h.meas.resize((size_t)O * 4);
    if (N > 0) HV_HIP(hipMemcpyAsync(h.cams.data(), cams, 128 * (size_t)N, hipMemcpyDeviceToHost, v->stream));
    if (M > 0) HV_HIP(hipMemcpyAsync(h.pts.data(), pts, 24 * (size_t)M, hipMemcpyDeviceToHost, v->stream));
    if (fixed != nullptr && N > 0) {
        h.fixed.resize((size_t)N);
        HV_HIP(hipMemcpyAsync(h.fixed.data(), fixed, (size_t)N, hipMemcpyDeviceToHost, v->stream));
    }
    if (O > 0) {
        HV_HIP(hipMemcpyAsync(h.idx.data(), idx, 8 * (size_t)O, hipMemcpyDeviceToHost, v->stream));
        HV_HIP(hipMemcpyAsync(h.meas.data(), meas, 32 * (size_t)O, hipMemcpyDeviceToHost, v->stream));
        if (active != nullptr) {
            h.active.resize((size_t)O);
            HV_HIP(hipMemcpyAsync(h.active.data(), active, (size_t)O, hipMemcpyDeviceToHost, v->stream));
        }
    }
    HV_HIP(hipStreamSynchronize(v->stream));
    h.p_cams = h.cams.data(), h.p_pts = h.pts.data(), h.p_idx = h.idx.data(), h.p_meas = h.meas.data();
    h.p_fixed = fixed != nullptr ? h.fixed.data() : nullptr;
    h.p_active = active != nullptr ? h.active.data() : nullptr;
    return HV_OK;
}

// The host's checks of the problem, before any launch.  solve: also that a camera is fixed while the points are free.
int bd_check(const char *fn, const BdHostView &h, int64_t N, int64_t M, int64_t O, bool points_free, bool solve) {
    bool any_fixed = false;
    for (int64_t i = 0; i < N; ++i) {
        const double *T = h.p_cams + i * 16;
        bool ok = T[12] == 0.0 && T[13] == 0.0 && T[14] == 0.0 && T[15] == 1.0;
        for (int k = 0; k < 16; ++k) ok = ok && std::isfinite(T[k]);
        HV_REQUIRE(ok, HV_ERR_INVALID, "%s: camera %lld is not finite or its bottom row is not 0 0 0 1", fn, (long long)i);
        any_fixed = any_fixed || (h.p_fixed != nullptr && h.p_fixed[i] != 0);
    }
    for (int64_t j = 0; j < 3 * M; ++j) HV_REQUIRE(std::isfinite(h.p_pts[j]), HV_ERR_INVALID, "%s: point %lld is not finite", fn, (long long)(j / 3));
    for (int64_t o = 0; o < O; ++o) {
        const int c = h.p_idx[2 * o], j = h.p_idx[2 * o + 1];
        HV_REQUIRE(c >= 0 && c < N && j >= 0 && j < M, HV_ERR_INVALID, "%s: observation %lld names camera %d and point %d, outside 0..%lld and 0..%lld",
                   fn, (long long)o, c, j, (long long)N - 1, (long long)M - 1);
        const double *m = h.p_meas + o * 4;
        HV_REQUIRE(std::isfinite(m[0]) && std::isfinite(m[1]), HV_ERR_INVALID, "%s: observation %lld has a pixel that is not finite", fn, (long long)o);
        HV_REQUIRE(std::isfinite(m[3]) && m[3] > 0.0, HV_ERR_INVALID, "%s: observation %lld has an inv_sigma2 that is not positive and finite", fn,
                   (long long)o);
    }
    HV_REQUIRE(!solve || !points_free || any_fixed || O == 0, HV_ERR_INVALID,
               "%s: no camera is fixed while the points are free: the gauge is open (fix a camera, or pass fixed_points)", fn);
    return HV_OK;
}

// rowc [N + 1], entc [O], rowp [M + 1], entp [O]: the observations of a camera / a point in the order of the observation index
void bd_incidence(const int32_t *idx, int64_t N, int64_t M, int64_t O, std::vector<int32_t> &csr) {
    csr.assign((size_t)(N + 1 + O + M + 1 + O), 0);
    int32_t *rowc = csr.data(), *entc = rowc + N + 1, *rowp = entc + O, *entp = rowp + M + 1;
    for (int64_t o = 0; o < O; ++o) rowc[idx[2 * o] + 1]++, rowp[idx[2 * o + 1] + 1]++;
    for (int64_t i = 0; i < N; ++i) rowc[i + 1] += rowc[i];
    for (int64_t j = 0; j < M; ++j) rowp[j + 1] += rowp[j];
    std::vector<int32_t> ac(rowc, rowc + N), ap(rowp, rowp + M);
    for (int64_t o = 0; o < O; ++o) {
        entc[ac[(size_t)idx[2 * o]]++] = (int32_t)o;
        entp[ap[(size_t)idx[2 * o + 1]]++] = (int32_t)o;
    }
}

int bd_check_model(const char *fn, const hv_bundle_params *prm) {
    HV_REQUIRE(std::isfinite(prm->fx) && prm->fx > 0.0 && std::isfinite(prm->fy) && prm->fy > 0.0 && std::isfinite(prm->bf) && prm->bf > 0.0,
               HV_ERR_INVALID, "%s: fx, fy and bf must be positive and finite", fn);
    HV_REQUIRE(std::isfinite(prm->cx) && std::isfinite(prm->cy), HV_ERR_INVALID, "%s: cx and cy must be finite", fn);
    HV_REQUIRE(std::isfinite(prm->huber_delta2_mono) && prm->huber_delta2_mono > 0.0 && std::isfinite(prm->huber_delta2_stereo) &&
                   prm->huber_delta2_stereo > 0.0,
               HV_ERR_INVALID, "%s: the Huber thresholds must be positive and finite", fn);
    HV_REQUIRE(std::isfinite(prm->min_depth) && prm->min_depth >= 0.0, HV_ERR_INVALID, "%s: min_depth must be finite and not negative", fn);
    return HV_OK;
}

// a caller's array (at loc) into the call's scratch, queued on the volume's stream
int bd_put(hv_volume *v, void *dst, const void *src, size_t bytes, int32_t loc) {
    if (loc == HV_HOST) return hv_h2d(v, dst, src, bytes);
    HV_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, v->stream));
    return HV_OK;
}

BdModel bd_model(const hv_bundle_params *prm) {
    return BdModel{prm->fx, prm->fy, prm->cx, prm->cy, prm->bf, prm->huber_delta2_mono, prm->huber_delta2_stereo, prm->min_depth, prm->huber ? 1 : 0};
}

constexpr int64_t BD_MAX_CAMERAS = 1 << 20, BD_MAX_POINTS = 1 << 24, BD_MAX_OBS = 1 << 26;
} // namespace

extern "C" void hv_bundle_default_params(hv_bundle_params *p) {
    if (p == nullptr) return;
    memset(p, 0, sizeof(*p));
    p->fx = 1.0, p->fy = 1.0, p->bf = 1.0;
    p->huber_delta2_mono = 5.991;
    p->huber_delta2_stereo = 7.815;
    p->min_depth = 1.0e-6;
    p->lambda_scale = 1.0e-5;
    p->gradient_tolerance = 1.0e-6;
    p->step_tolerance = 1.0e-6;
    p->decrease_tolerance = 1.0e-6;
    p->residual_tolerance = 1.0e-6;
    p->cg_tolerance = 1.0e-8;
    p->max_iterations = 100;
    p->cg_max_iterations = 100;
    p->huber = 1;
}

extern "C" int hv_bundle_adjust(hv_volume *v, double *cameras, int64_t n_cameras, double *points, int64_t n_points,
                                const uint8_t *camera_fixed, const int32_t *obs_index, const double *obs_meas, const uint8_t *obs_active,
                                int64_t n_obs, const hv_bundle_params *prm, double *chi2_out, uint8_t *behind_out, hv_bundle_result *res,
                                double *trace, double *trace_cameras, double *trace_points, int64_t trace_cap, int64_t *trace_rows,
                                int32_t loc) {
    const char *fn = "hv_bundle_adjust";
    HV_REQUIRE(v != nullptr && prm != nullptr && res != nullptr, HV_ERR_INVALID, "%s: null argument", fn);
    HV_REQUIRE(loc == HV_HOST || loc == HV_DEVICE, HV_ERR_INVALID, "%s: bad loc %d", fn, (int)loc);
    const int64_t N = n_cameras, M = n_points, O = n_obs;
    HV_REQUIRE(N >= 0 && N <= BD_MAX_CAMERAS && M >= 0 && M <= BD_MAX_POINTS && O >= 0 && O <= BD_MAX_OBS, HV_ERR_INVALID,
               "%s: need 0 .. %lld cameras, 0 .. %lld points and 0 .. %lld observations, got %lld, %lld, %lld", fn, (long long)BD_MAX_CAMERAS,
               (long long)BD_MAX_POINTS, (long long)BD_MAX_OBS, (long long)N, (long long)M, (long long)O);
    HV_REQUIRE(O == 0 || (N >= 1 && M >= 1), HV_ERR_INVALID, "%s: %lld observations need at least one camera and one point, got %lld and %lld", fn,
               (long long)O, (long long)N, (long long)M);
    HV_REQUIRE((N == 0 || cameras != nullptr) && (M == 0 || points != nullptr) && (O == 0 || (obs_index != nullptr && obs_meas != nullptr)),
               HV_ERR_INVALID, "%s: null cameras, points or observation arrays", fn);
    int rc = bd_check_model(fn, prm);
    if (rc != HV_OK) return rc;
    HV_REQUIRE(std::isfinite(prm->lambda_scale) && prm->lambda_scale > 0.0, HV_ERR_INVALID, "%s: lambda_scale must be positive and finite", fn);
    HV_REQUIRE(prm->gradient_tolerance >= 0.0 && prm->step_tolerance >= 0.0 && prm->decrease_tolerance >= 0.0 && prm->residual_tolerance >= 0.0 &&
                   prm->cg_tolerance >= 0.0 && prm->cg_tolerance < 1.0,
               HV_ERR_INVALID, "%s: a tolerance is negative (or cg_tolerance is not below 1)", fn);
    HV_REQUIRE(prm->max_iterations >= 1 && prm->max_iterations <= 10000 && prm->cg_max_iterations >= 1 && prm->cg_max_iterations <= 10000,
               HV_ERR_INVALID, "%s: max_iterations and cg_max_iterations must be in 1..10000", fn);
    HV_REQUIRE(trace == nullptr || trace_cap >= 0, HV_ERR_INVALID, "%s: negative trace_cap", fn);
    HV_REQUIRE(!prm->trace_state || (trace != nullptr && trace_cameras != nullptr && trace_points != nullptr), HV_ERR_INVALID,
               "%s: trace_state needs trace, trace_cameras and trace_points", fn);
    HV_HIP(hipSetDevice(v->device));
    const bool points_free = prm->fixed_points == 0;

    BdHostView h;
    rc = bd_host_view(v, h, cameras, N, points, M, camera_fixed, obs_index, obs_meas, obs_active, O, loc);
    if (rc != HV_OK) return rc;
    rc = bd_check(fn, h, N, M, O, points_free, true);
    if (rc != HV_OK) return rc;
    if (trace_rows) *trace_rows = 0;
    memset(res, 0, sizeof(*res));
    bool any_active = false;
    for (int64_t o = 0; o < O && !any_active; ++o) any_active = h.p_active == nullptr || h.p_active[o] != 0;
    if (!any_active) { // nothing was measured: nothing moves
        res->success = 1;
        res->converged = HV_POSE_GRAPH_RESIDUAL;
        return HV_OK;
    }
    std::vector<int32_t> csr;
    bd_incidence(h.p_idx, N, M, O, csr);

    const int nbO = (int)((O + PG_BLOCK - 1) / PG_BLOCK), nbN = (int)((N + PG_BLOCK - 1) / PG_BLOCK), nbM = (int)((M + PG_BLOCK - 1) / PG_BLOCK);
    const int nbW = (int)((N + BD_CAMS_PER_BLOCK - 1) / BD_CAMS_PER_BLOCK);
    const int cap = trace != nullptr ? (int)std::min<int64_t>(trace_cap, prm->max_iterations) : 0;
    const int cap_state = prm->trace_state ? cap : 0;
    PgLayout lay;
    const size_t o_state = lay.take(sizeof(PgState));
    const size_t o_T = lay.take(128 * (size_t)N), o_Tn = lay.take(128 * (size_t)N), o_P = lay.take(24 * (size_t)M), o_Pn = lay.take(24 * (size_t)M);
    const size_t o_csr = lay.take(4 * csr.size());
    const size_t o_act = lay.take((size_t)O), o_beh = lay.take((size_t)O), o_fix = lay.take((size_t)N);
    const size_t o_q = lay.take(24 * (size_t)O), o_A = lay.take(48 * (size_t)O), o_g = lay.take(24 * (size_t)O), o_chi = lay.take(8 * (size_t)O);
    const size_t o_C = lay.take(48 * (size_t)M), o_Ci = lay.take(48 * (size_t)M);
    size_t o_pv[3]; // bp, wp, y
    for (size_t &o : o_pv) o = lay.take(24 * (size_t)M);
    const size_t o_B = lay.take(8 * 21 * (size_t)N), o_L = lay.take(8 * 21 * (size_t)N);
    size_t o_vec[6]; // bc, x, r, z, p, q
    for (size_t &o : o_vec) o = lay.take(48 * (size_t)N);
    const int nMax = nbW + nbM, nStep = nbN + nbM;
    const size_t o_pmaxd = lay.take(8 * (size_t)nMax), o_pgrad = lay.take(8 * (size_t)nMax), o_grad = lay.take(8 * (size_t)nStep);
    const size_t o_prz = lay.take(8 * (size_t)std::max(nbN, nbW)), o_ppq = lay.take(8 * (size_t)nbW);
    const size_t o_pdd = lay.take(8 * (size_t)nStep), o_ppred = lay.take(8 * (size_t)nStep);
    const size_t o_pF = lay.take(8 * (size_t)nbO), o_pFn = lay.take(8 * (size_t)nbO);
    const size_t o_trace = lay.take(8 * HV_POSE_GRAPH_TRACE_STRIDE * (size_t)std::max(cap, 1));
    const size_t o_tcam = lay.take(128 * (size_t)N * (size_t)cap_state), o_tpt = lay.take(24 * (size_t)M * (size_t)cap_state);
    rc = hv_ensure_buffer(v, &v->track_buf, &v->track_buf_bytes, lay.off);
    if (rc != HV_OK) return rc;
    char *base = (char *)v->track_buf;
    PgState *S = (PgState *)(base + o_state);
    double *T = (double *)(base + o_T), *Tn = (double *)(base + o_Tn), *P = (double *)(base + o_P), *Pn = (double *)(base + o_Pn);
    int32_t *d_rowc = (int32_t *)(base + o_csr), *d_entc = d_rowc + N + 1, *d_rowp = d_entc + O, *d_entp = d_rowp + M + 1;
    uint8_t *d_act = (uint8_t *)(base + o_act), *d_beh = (uint8_t *)(base + o_beh), *d_fix = (uint8_t *)(base + o_fix);
    double *q3 = (double *)(base + o_q), *A6 = (double *)(base + o_A), *gq = (double *)(base + o_g), *d_chi = (double *)(base + o_chi);
    double *C6 = (double *)(base + o_C), *Ci6 = (double *)(base + o_Ci);
    double *bp = (double *)(base + o_pv[0]), *wp = (double *)(base + o_pv[1]), *y = (double *)(base + o_pv[2]);
    double *B21 = (double *)(base + o_B), *L21 = (double *)(base + o_L);
    double *bc = (double *)(base + o_vec[0]), *x = (double *)(base + o_vec[1]), *rr = (double *)(base + o_vec[2]);
    double *z = (double *)(base + o_vec[3]), *p = (double *)(base + o_vec[4]), *qv = (double *)(base + o_vec[5]);
    double *p_maxd = (double *)(base + o_pmaxd), *p_grad = (double *)(base + o_pgrad), *d_grad = (double *)(base + o_grad);
    double *p_rz = (double *)(base + o_prz), *p_pq = (double *)(base + o_ppq), *p_dd = (double *)(base + o_pdd), *p_pred = (double *)(base + o_ppred);
    double *p_F = (double *)(base + o_pF), *p_Fn = (double *)(base + o_pFn);
    double *d_trace = (double *)(base + o_trace), *d_tcam = (double *)(base + o_tcam), *d_tpt = (double *)(base + o_tpt);

    HvStage st(v, loc);
    // the state and the flags go straight into the call's scratch (bd_put below); what the kernels read in place is staged
    const int i_idx = st.in(obs_index, 8 * (size_t)O), i_meas = st.in(obs_meas, 32 * (size_t)O);
    const int i_cout = st.out(cameras, 128 * (size_t)N), i_pout = st.out(points, 24 * (size_t)M);
    const int i_chi = st.out(chi2_out, 8 * (size_t)O), i_beh = st.out(behind_out, (size_t)O);
    rc = st.commit(&v->stage, &v->stage_bytes);
    if (rc != HV_OK) return rc;
    const int32_t *d_idx = st.dev<const int32_t>(i_idx);
    const double *d_meas = st.dev<const double>(i_meas);
    v->pipe_armed = false; // as hv_pose_graph_optimize: the next batch starts a fresh chain behind this call

    PgState h0{};
    h0.nu = 2.0;
    HV_HIP(hipMemcpyAsync(S, &h0, sizeof(PgState), hipMemcpyHostToDevice, v->stream));
    HV_HIP(hipMemcpyAsync(d_rowc, csr.data(), 4 * csr.size(), hipMemcpyHostToDevice, v->stream));
    if ((rc = bd_put(v, T, cameras, 128 * (size_t)N, loc)) != HV_OK || (rc = bd_put(v, P, points, 24 * (size_t)M, loc)) != HV_OK) return rc;
    if (camera_fixed != nullptr) {
        if ((rc = bd_put(v, d_fix, camera_fixed, (size_t)N, loc)) != HV_OK) return rc;
    } else {
        HV_HIP(hipMemsetAsync(d_fix, 0, (size_t)N, v->stream));
    }
    if (obs_active != nullptr) {
        if ((rc = bd_put(v, d_act, obs_active, (size_t)O, loc)) != HV_OK) return rc;
    } else {
        HV_HIP(hipMemsetAsync(d_act, 1, (size_t)O, v->stream));
    }
    HV_HIP(hipMemsetAsync(d_beh, 0, (size_t)O, v->stream));
    HV_HIP(hipMemsetAsync(d_grad, 0, 8 * (size_t)nStep, v->stream));
    HV_HIP(hipStreamSynchronize(v->stream)); // h0 and csr are host memory of this frame

    const BdModel K = bd_model(prm);
    const double tol2 = prm->cg_tolerance * prm->cg_tolerance;
    const PgRules rules{prm->gradient_tolerance, prm->step_tolerance, prm->decrease_tolerance, prm->residual_tolerance, prm->max_iterations};
    const dim3 gO((unsigned)nbO), gN((unsigned)nbN), gM((unsigned)nbM), gW((unsigned)nbW), blk(PG_BLOCK);
    const int pf = points_free ? 1 : 0;
    const int64_t n16 = 16 * N, m3 = 3 * M;
    double *const nul = nullptr;
    PgState hs{};
    for (int it = 0; it < prm->max_iterations; ++it) {
        if (it < cap_state) {
            HV_HIP(hipMemcpyAsync(d_tcam + (size_t)it * 16 * (size_t)N, T, 128 * (size_t)N, hipMemcpyDeviceToDevice, v->stream));
            HV_HIP(hipMemcpyAsync(d_tpt + (size_t)it * 3 * (size_t)M, P, 24 * (size_t)M, hipMemcpyDeviceToDevice, v->stream));
        }
        hv_profile_begin(v);
        hipLaunchKernelGGL(k_bd_linearise, gO, blk, 0, v->stream, (const double *)T, (const double *)P, d_idx, d_meas, d_act, d_beh, it == 0 ? 1 : 0,
                           (int)O, K, q3, A6, gq, nul, nul, nul, p_F);
        hipLaunchKernelGGL(k_bd_gather_points, gM, blk, 0, v->stream, (const int32_t *)d_rowp, (const int32_t *)d_entp, d_idx, (const double *)T,
                           (const double *)A6, (const double *)gq, (int)M, (int)O, pf, C6, bp, p_maxd + nbW, p_grad + nbW);
        hipLaunchKernelGGL(k_bd_gather_cams, gW, blk, 0, v->stream, (const int32_t *)d_rowc, (const int32_t *)d_entc, (const double *)q3,
                           (const double *)A6, (const double *)gq, (const uint8_t *)d_fix, (int)N, (int)O, B21, bc, p_maxd, p_grad);
        hipLaunchKernelGGL(k_bd_lambda, dim3(1), dim3(64), 0, v->stream, S, (const double *)p_maxd, (const double *)p_grad, nMax, prm->lambda_scale,
                           d_grad);
        hipLaunchKernelGGL(k_bd_invert_points, gM, blk, 0, v->stream, S, (const double *)C6, (const double *)bp, (int)M, pf, Ci6, wp);
        hipLaunchKernelGGL(k_bd_factor_cams, gW, blk, 0, v->stream, S, (const int32_t *)d_rowc, (const int32_t *)d_entc, d_idx, (const double *)T,
                           (const double *)q3, (const double *)A6, (const double *)Ci6, (const double *)wp, (const double *)B21, (const double *)bc,
                           (const uint8_t *)d_fix, (int)N, (int)M, (int)O, L21, rr);
        hipLaunchKernelGGL(k_bd_cg_start, gN, blk, 0, v->stream, (const double *)L21, (const double *)rr, (int)N, x, z, p_rz);
        for (int j = 0; j < prm->cg_max_iterations; ++j) {
            hipLaunchKernelGGL(k_pg_cg_direction, gN, blk, 0, v->stream, S, j, (const double *)p_rz, nbN, tol2, (int)N, (const double *)z, p);
            hipLaunchKernelGGL(k_bd_schur_points, gM, blk, 0, v->stream, (const PgState *)S, j, (const int32_t *)d_rowp, (const int32_t *)d_entp, d_idx,
                               (const double *)T, (const double *)q3, (const double *)A6, (const double *)Ci6, (const double *)p, (int)N, (int)M,
                               (int)O, y, (const double *)nullptr, (const double *)nullptr, (const double *)nullptr, nul, nul, nul);
            hipLaunchKernelGGL(k_bd_schur_cams, gW, blk, 0, v->stream, (const PgState *)S, j, (const int32_t *)d_rowc, (const int32_t *)d_entc, d_idx,
                               (const double *)T, (const double *)q3, (const double *)A6, (const double *)y, (const double *)B21,
                               (const uint8_t *)d_fix, (const double *)p, (int)N, (int)M, (int)O, qv, p_pq);
            hipLaunchKernelGGL(k_pg_cg_update, gN, blk, 0, v->stream, (const PgState *)S, j, (const double *)p_pq, nbW, (const double *)L21, (int)N,
                               (const double *)p, (const double *)qv, x, rr, z, p_rz);
        }
        hipLaunchKernelGGL(k_pg_trial, gN, blk, 0, v->stream, (const PgState *)S, (const double *)T, (const double *)x, (const double *)bc, (int)N, Tn,
                           p_dd, p_pred);
        hipLaunchKernelGGL(k_bd_schur_points, gM, blk, 0, v->stream, (const PgState *)S, -1, (const int32_t *)d_rowp, (const int32_t *)d_entp, d_idx,
                           (const double *)T, (const double *)q3, (const double *)A6, (const double *)Ci6, (const double *)x, (int)N, (int)M, (int)O,
                           nul, (const double *)wp, (const double *)bp, (const double *)P, Pn, p_dd + nbN, p_pred + nbN);
        hipLaunchKernelGGL(k_bd_linearise, gO, blk, 0, v->stream, (const double *)Tn, (const double *)Pn, d_idx, d_meas, d_act, d_beh, 0, (int)O, K, nul,
                           nul, nul, nul, nul, nul, p_Fn);
        hipLaunchKernelGGL(k_pg_decide, dim3(1), dim3(64), 0, v->stream, S, (const double *)p_F, (const double *)p_Fn, nbO, (const double *)p_dd,
                           (const double *)p_pred, (const double *)d_grad, nStep, rules, cap > 0 ? d_trace : nul, cap);
        hipLaunchKernelGGL(k_pg_commit, dim3((unsigned)((n16 + PG_BLOCK - 1) / PG_BLOCK)), blk, 0, v->stream, (const PgState *)S, (const double *)Tn,
                           n16, T);
        hipLaunchKernelGGL(k_pg_commit, dim3((unsigned)((m3 + PG_BLOCK - 1) / PG_BLOCK)), blk, 0, v->stream, (const PgState *)S, (const double *)Pn,
                           m3, P);
        hv_profile_end(v, 0);
        HV_HIP(hipGetLastError());
        // the iteration's one host wait
        HV_HIP(hipMemcpyAsync(&hs, S, sizeof(PgState), hipMemcpyDeviceToHost, v->stream));
        HV_HIP(hipStreamSynchronize(v->stream));
        if (hs.stop) break;
    }
    // chi2 per observation at the final state, and the state to where the caller reads it
    double *d_chi_out = st.dev<double>(i_chi) != nullptr ? st.dev<double>(i_chi) : d_chi;
    hv_profile_begin(v);
    hipLaunchKernelGGL(k_bd_linearise, gO, blk, 0, v->stream, (const double *)T, (const double *)P, d_idx, d_meas, d_act, d_beh, 0, (int)O, K, nul, nul,
                       nul, d_chi_out, nul, nul, nul);
    hv_profile_end(v, 0);
    HV_HIP(hipGetLastError());
    HV_HIP(hipMemcpyAsync(st.dev<double>(i_cout), T, 128 * (size_t)N, hipMemcpyDeviceToDevice, v->stream));
    HV_HIP(hipMemcpyAsync(st.dev<double>(i_pout), P, 24 * (size_t)M, hipMemcpyDeviceToDevice, v->stream));
    if (st.dev<uint8_t>(i_beh) != nullptr) HV_HIP(hipMemcpyAsync(st.dev<uint8_t>(i_beh), d_beh, (size_t)O, hipMemcpyDeviceToDevice, v->stream));
    rc = st.finish(&hs, sizeof(PgState), S);
    if (rc != HV_OK) return rc;
    const int64_t rows = std::min<int64_t>(hs.iter, cap);
    if (rows > 0) {
        HV_HIP(hipMemcpy(trace, d_trace, 8 * HV_POSE_GRAPH_TRACE_STRIDE * (size_t)rows, hipMemcpyDeviceToHost));
        if (cap_state > 0) {
            HV_HIP(hipMemcpy(trace_cameras, d_tcam, 128 * (size_t)N * (size_t)rows, hipMemcpyDeviceToHost));
            HV_HIP(hipMemcpy(trace_points, d_tpt, 24 * (size_t)M * (size_t)rows, hipMemcpyDeviceToHost));
        }
    }
    if (trace_rows) *trace_rows = rows;
    res->chi2_initial = hs.chi2_initial;
    res->chi2_final = hs.chi2_final;
    res->lambda = hs.lambda;
    res->iterations = hs.iter;
    res->cg_iterations_total = hs.cg_total;
    res->converged = hs.converged;
    res->success = (hs.converged != 0 && hs.bad == 0 && std::isfinite(hs.chi2_final)) ? 1 : 0;
    return HV_OK;
}

extern "C" int hv_bundle_linearise(hv_volume *v, const double *cameras, int64_t n_cameras, const double *points, int64_t n_points,
                                   const int32_t *obs_index, const double *obs_meas, const uint8_t *obs_active, int64_t n_obs,
                                   const hv_bundle_params *prm, double *r_out, double *chi2_out, double *w_out, uint8_t *behind_out,
                                   double *B_out, double *bc_out, double *C_out, double *bp_out, double *F_out, int32_t loc) {
    const char *fn = "hv_bundle_linearise";
    HV_REQUIRE(v != nullptr && prm != nullptr && cameras != nullptr && points != nullptr && obs_index != nullptr && obs_meas != nullptr,
               HV_ERR_INVALID, "%s: null argument", fn);
    HV_REQUIRE(loc == HV_HOST || loc == HV_DEVICE, HV_ERR_INVALID, "%s: bad loc %d", fn, (int)loc);
    const int64_t N = n_cameras, M = n_points, O = n_obs;
    HV_REQUIRE(N >= 1 && N <= BD_MAX_CAMERAS && M >= 1 && M <= BD_MAX_POINTS && O >= 1 && O <= BD_MAX_OBS, HV_ERR_INVALID,
               "%s: bad problem size %lld cameras, %lld points, %lld observations", fn, (long long)N, (long long)M, (long long)O);
    int rc = bd_check_model(fn, prm);
    if (rc != HV_OK) return rc;
    HV_HIP(hipSetDevice(v->device));
    BdHostView h;
    rc = bd_host_view(v, h, cameras, N, points, M, nullptr, obs_index, obs_meas, obs_active, O, loc);
    if (rc != HV_OK) return rc;
    rc = bd_check(fn, h, N, M, O, true, false);
    if (rc != HV_OK) return rc;
    std::vector<int32_t> csr;
    bd_incidence(h.p_idx, N, M, O, csr);
    const int nbO = (int)((O + PG_BLOCK - 1) / PG_BLOCK), nbM = (int)((M + PG_BLOCK - 1) / PG_BLOCK);
    const int nbW = (int)((N + BD_CAMS_PER_BLOCK - 1) / BD_CAMS_PER_BLOCK);
    PgLayout lay;
    const size_t o_csr = lay.take(4 * csr.size()), o_act = lay.take((size_t)O), o_beh = lay.take((size_t)O), o_fix = lay.take((size_t)N);
    const size_t o_q = lay.take(24 * (size_t)O), o_A = lay.take(48 * (size_t)O), o_g = lay.take(24 * (size_t)O), o_r = lay.take(24 * (size_t)O);
    const size_t o_chi = lay.take(8 * (size_t)O), o_w = lay.take(8 * (size_t)O);
    const size_t o_C = lay.take(48 * (size_t)M), o_bp = lay.take(24 * (size_t)M), o_B = lay.take(8 * 21 * (size_t)N), o_bc = lay.take(48 * (size_t)N);
    const size_t o_p0 = lay.take(8 * (size_t)(nbW + nbM)), o_p1 = lay.take(8 * (size_t)(nbW + nbM)), o_pF = lay.take(8 * (size_t)nbO);
    rc = hv_ensure_buffer(v, &v->track_buf, &v->track_buf_bytes, lay.off);
    if (rc != HV_OK) return rc;
    char *base = (char *)v->track_buf;
    int32_t *d_rowc = (int32_t *)(base + o_csr), *d_entc = d_rowc + N + 1, *d_rowp = d_entc + O, *d_entp = d_rowp + M + 1;
    uint8_t *d_act = (uint8_t *)(base + o_act), *d_beh = (uint8_t *)(base + o_beh), *d_fix = (uint8_t *)(base + o_fix);
    double *q3 = (double *)(base + o_q), *A6 = (double *)(base + o_A), *gq = (double *)(base + o_g), *r3 = (double *)(base + o_r);
    double *chi = (double *)(base + o_chi), *w = (double *)(base + o_w), *C6 = (double *)(base + o_C), *bp = (double *)(base + o_bp);
    double *B21 = (double *)(base + o_B), *bc = (double *)(base + o_bc), *p_F = (double *)(base + o_pF);
    HvStage st(v, loc);
    const int i_cin = st.in(cameras, 128 * (size_t)N), i_pin = st.in(points, 24 * (size_t)M), i_idx = st.in(obs_index, 8 * (size_t)O);
    const int i_meas = st.in(obs_meas, 32 * (size_t)O), i_act = st.in(obs_active, (size_t)O);
    rc = st.commit(&v->stage, &v->stage_bytes);
    if (rc != HV_OK) return rc;
    v->pipe_armed = false;
    const double *T = st.dev<const double>(i_cin), *P = st.dev<const double>(i_pin);
    const int32_t *d_idx = st.dev<const int32_t>(i_idx);
    HV_HIP(hipMemcpyAsync(d_rowc, csr.data(), 4 * csr.size(), hipMemcpyHostToDevice, v->stream));
    if (obs_active != nullptr)
        HV_HIP(hipMemcpyAsync(d_act, st.dev<const uint8_t>(i_act), (size_t)O, hipMemcpyDeviceToDevice, v->stream));
    else
        HV_HIP(hipMemsetAsync(d_act, 1, (size_t)O, v->stream));
    HV_HIP(hipMemsetAsync(d_beh, 0, (size_t)O, v->stream));
    HV_HIP(hipMemsetAsync(d_fix, 0, (size_t)N, v->stream));
    const dim3 blk(PG_BLOCK);
    hipLaunchKernelGGL(k_bd_linearise, dim3((unsigned)nbO), blk, 0, v->stream, T, P, d_idx, st.dev<const double>(i_meas), d_act, d_beh, 1, (int)O,
                       bd_model(prm), q3, A6, gq, chi, r3, w, p_F);
    hipLaunchKernelGGL(k_bd_gather_points, dim3((unsigned)nbM), blk, 0, v->stream, (const int32_t *)d_rowp, (const int32_t *)d_entp, d_idx, T,
                       (const double *)A6, (const double *)gq, (int)M, (int)O, 1, C6, bp, (double *)(base + o_p0) + nbW, (double *)(base + o_p1) + nbW);
    hipLaunchKernelGGL(k_bd_gather_cams, dim3((unsigned)nbW), blk, 0, v->stream, (const int32_t *)d_rowc, (const int32_t *)d_entc, (const double *)q3,
                       (const double *)A6, (const double *)gq, (const uint8_t *)d_fix, (int)N, (int)O, B21, bc, (double *)(base + o_p0),
                       (double *)(base + o_p1));
    HV_HIP(hipGetLastError());
    // struct-of-arrays on the device, row-major records for the caller (host memory)
    std::vector<double> hr(3 * (size_t)O), hC(6 * (size_t)M), hbp(3 * (size_t)M), hB(21 * (size_t)N), hbc(6 * (size_t)N), hF((size_t)nbO);
    HV_HIP(hipMemcpyAsync(hr.data(), r3, 8 * hr.size(), hipMemcpyDeviceToHost, v->stream));
    HV_HIP(hipMemcpyAsync(hC.data(), C6, 8 * hC.size(), hipMemcpyDeviceToHost, v->stream));
    HV_HIP(hipMemcpyAsync(hbp.data(), bp, 8 * hbp.size(), hipMemcpyDeviceToHost, v->stream));
    HV_HIP(hipMemcpyAsync(hB.data(), B21, 8 * hB.size(), hipMemcpyDeviceToHost, v->stream));
    HV_HIP(hipMemcpyAsync(hbc.data(), bc, 8 * hbc.size(), hipMemcpyDeviceToHost, v->stream));
    HV_HIP(hipMemcpyAsync(hF.data(), p_F, 8 * hF.size(), hipMemcpyDeviceToHost, v->stream));
    if (chi2_out != nullptr) HV_HIP(hipMemcpyAsync(chi2_out, chi, 8 * (size_t)O, hipMemcpyDeviceToHost, v->stream));
    if (w_out != nullptr) HV_HIP(hipMemcpyAsync(w_out, w, 8 * (size_t)O, hipMemcpyDeviceToHost, v->stream));
    if (behind_out != nullptr) HV_HIP(hipMemcpyAsync(behind_out, d_beh, (size_t)O, hipMemcpyDeviceToHost, v->stream));
    HV_HIP(hipStreamSynchronize(v->stream));
    if (r_out != nullptr)
        for (int64_t o = 0; o < O; ++o)
            for (int a = 0; a < 3; ++a) r_out[o * 3 + a] = hr[(size_t)a * O + o];
    for (int64_t j = 0; j < M; ++j)
        for (int a = 0; a < 3; ++a) {
            if (bp_out != nullptr) bp_out[j * 3 + a] = hbp[(size_t)a * M + j];
            if (C_out != nullptr)
                for (int c = 0; c < 3; ++c) {
                    const int lo = std::min(a, c), hi = std::max(a, c);
                    C_out[j * 9 + a * 3 + c] = hC[(size_t)(lo * 3 - (lo * (lo - 1)) / 2 + (hi - lo)) * M + j];
                }
        }
    for (int64_t i = 0; i < N; ++i)
        for (int a = 0; a < 6; ++a) {
            if (bc_out != nullptr) bc_out[i * 6 + a] = hbc[(size_t)a * N + i];
            if (B_out != nullptr)
                for (int c = 0; c < 6; ++c) {
                    const int lo = std::min(a, c), hi = std::max(a, c);
                    B_out[i * 36 + a * 6 + c] = hB[(size_t)(lo * 6 - (lo * (lo - 1)) / 2 + (hi - lo)) * N + i];
                }
        }
    if (F_out != nullptr) {
        double F = 0.0;
        for (double f : hF) F += f;
        *F_out = F;
    }
    return HV_OK;
}
