// Levenberg-Marquardt with a block-Jacobi preconditioned conjugate-gradient inner solve over 6-vectors, one per pose: what
// hv_pose_graph.hip and hv_bundle.hip share (contract in include/hipvol.h, the pose-graph section).  The state and the CG scalars on the
// device (PgState), the fixed-order sums, Log of a rotation, the pose update T := exp(d) T (k_pg_trial), the preconditioner solve, the
// two CG kernels that touch only per-pose vectors, the decision of an outer iteration and the commit of an accepted step.  The product
// H p between k_pg_cg_direction and k_pg_cg_update is the including file's own.  Kernels live in the including file's unnamed namespace.
#pragma once
#include <cmath>

#include "hv_common.h"

namespace {
constexpr int PG_BLOCK = 256;
constexpr double PG_SMALL = 1.0e-8;       // Log / exp: below it sin(th) / th = 1
constexpr double PG_NEAR_PI_COS = -0.99;  // Log: cos(th) below it takes the axis from R + R^T
constexpr double PG_JINV_SERIES = 0.05;   // Jl^-1: below it the coefficient is its series

struct PgState {
    double lambda, nu, F, Fnew, rho, pred, gradnorm, stepnorm, cg_res, chi2_initial, chi2_final, rz0;
    double rz[2];
    int32_t done[2];
    int32_t iter, stop, converged, accepted, cg_iters, cg_total, kept, bad;
};

__device__ __forceinline__ int pg_tri(int a, int b) { return a * 6 - (a * (a - 1)) / 2 + (b - a); } // a <= b

// the workgroup's sum: lanes by butterfly, then the four waves in order.  All PG_BLOCK threads.
__device__ __forceinline__ double pg_block_sum(double x, double *red) {
    x = hv_wave_sum(x);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    const double s = ((red[0] + red[1]) + red[2]) + red[3];
    __syncthreads();
    return s;
}
__device__ __forceinline__ double pg_block_max(double x, double *red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x = fmax(x, __shfl_xor(x, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    const double s = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    __syncthreads();
    return s;
}
// the second stage: the n workgroup sums in order, by one thread, handed to all
__device__ __forceinline__ double pg_sum_parts(const double *__restrict__ part, int n, double *sh) {
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int k = 0; k < n; ++k) s += part[k];
        *sh = s;
    }
    __syncthreads();
    const double s = *sh;
    __syncthreads();
    return s;
}

// Log of a rotation (row-major R[9]) -> w[3]
__device__ __forceinline__ void pg_log_rot(const double *R, double *w) {
    const double v0 = 0.5 * (R[7] - R[5]), v1 = 0.5 * (R[2] - R[6]), v2 = 0.5 * (R[3] - R[1]);
    const double s = sqrt((v0 * v0 + v1 * v1) + v2 * v2);
    const double c = 0.5 * (((R[0] + R[4]) + R[8]) - 1.0);
    const double th = atan2(s, c);
    if (c < PG_NEAR_PI_COS) {
        const double den = 1.0 - c;
        const double m00 = (R[0] - c) / den, m11 = (R[4] - c) / den, m22 = (R[8] - c) / den;
        const double m01 = 0.5 * (R[1] + R[3]) / den, m02 = 0.5 * (R[2] + R[6]) / den, m12 = 0.5 * (R[5] + R[7]) / den;
        const int k = (m11 > m00) ? ((m22 > m11) ? 2 : 1) : ((m22 > m00) ? 2 : 0);
        const double dk = sqrt(k == 0 ? m00 : (k == 1 ? m11 : m22));
        double a0 = (k == 0 ? m00 : (k == 1 ? m01 : m02)) / dk;
        double a1 = (k == 0 ? m01 : (k == 1 ? m11 : m12)) / dk;
        double a2 = (k == 0 ? m02 : (k == 1 ? m12 : m22)) / dk;
        const double n = sqrt((a0 * a0 + a1 * a1) + a2 * a2);
        const double sg = ((a0 * v0 + a1 * v1) + a2 * v2) < 0.0 ? -1.0 : 1.0;
        const double f = sg * th / n;
        w[0] = f * a0, w[1] = f * a1, w[2] = f * a2;
    } else {
        const double f = s < PG_SMALL ? 1.0 : th / s;
        w[0] = f * v0, w[1] = f * v1, w[2] = f * v2;
    }
}

// The Cholesky factor of A + lambda I for one 6 x 6 block (upper triangle A[pg_tri]); L[pg_tri(c, r)] = L(r, c), c <= r.  A pivot
// that is not positive is replaced by 1 and reported: returns true.
__device__ __forceinline__ bool pg_chol6(const double *A, double lambda, double *L) {
    bool bad = false;
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        double d = A[pg_tri(j, j)] + lambda;
#pragma unroll
        for (int q = 0; q < j; ++q) d -= L[pg_tri(q, j)] * L[pg_tri(q, j)];
        if (!(d > 0.0)) bad = true, d = 1.0;
        const double p = sqrt(d);
        L[pg_tri(j, j)] = p;
#pragma unroll
        for (int r = j + 1; r < 6; ++r) {
            double e = A[pg_tri(j, r)];
#pragma unroll
            for (int q = 0; q < j; ++q) e -= L[pg_tri(q, r)] * L[pg_tri(q, j)];
            L[pg_tri(j, r)] = e / p;
        }
    }
    return bad;
}

// z = (L L^T)^-1 r with one node's factor in registers: L[pg_tri(c, r)] = L(r, c), c <= r
__device__ __forceinline__ void pg_precond(const double *L, const double *r, double *z) {
    double y[6];
#pragma unroll
    for (int a = 0; a < 6; ++a) {
        double e = r[a];
#pragma unroll
        for (int q = 0; q < a; ++q) e -= L[pg_tri(q, a)] * y[q];
        y[a] = e / L[pg_tri(a, a)];
    }
#pragma unroll
    for (int a = 5; a >= 0; --a) {
        double e = y[a];
#pragma unroll
        for (int q = a + 1; q < 6; ++q) e -= L[pg_tri(a, q)] * z[q];
        z[a] = e / L[pg_tri(a, a)];
    }
}

// CG iteration j, first of four: rz = sum part_rz, the stopping test, beta, p = z + beta p.  Reads the scalars of parity j - 1,
// writes those of parity j.
__global__ __launch_bounds__(PG_BLOCK) void k_pg_cg_direction(PgState *__restrict__ S, int j, const double *__restrict__ part_rz, int nbN,
                                                               double tol2, int N, const double *__restrict__ z, double *__restrict__ p) {
    __shared__ double sh;
    const int cur = j & 1, prev = cur ^ 1;
    const bool first = blockIdx.x == 0 && threadIdx.x == 0;
    if (j > 0 && S->done[prev]) {
        if (first) S->done[cur] = 1, S->rz[cur] = S->rz[prev];
        return;
    }
    const double rz = pg_sum_parts(part_rz, nbN, &sh);
    const double rz0 = j == 0 ? rz : S->rz0;
    const bool done = !(rz > tol2 * rz0);
    const double beta = j == 0 ? 0.0 : rz / S->rz[prev];
    if (first) {
        S->rz[cur] = rz;
        S->done[cur] = done ? 1 : 0;
        if (j == 0) S->rz0 = rz, S->cg_iters = 0;
        S->cg_res = rz0 > 0.0 ? sqrt(rz / rz0) : 0.0;
        if (!done) S->cg_iters = j + 1;
    }
    if (done) return;
    const int i = blockIdx.x * PG_BLOCK + threadIdx.x;
    if (i < N) {
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            const size_t k = (size_t)a * N + i;
            p[k] = j == 0 ? z[k] : z[k] + beta * p[k];
        }
    }
}

// fourth: alpha = rz / sum part_pq, x += alpha p, r -= alpha q, z = P^-1 r, part_rz
__global__ __launch_bounds__(PG_BLOCK) void k_pg_cg_update(const PgState *__restrict__ S, int j, const double *__restrict__ part_pq, int nbN,
                                                            const double *__restrict__ L21, int N, const double *__restrict__ p,
                                                            const double *__restrict__ qv, double *__restrict__ x, double *__restrict__ rr,
                                                            double *__restrict__ z, double *__restrict__ part_rz) {
    __shared__ double red[4];
    __shared__ double sh;
    if (S->done[j & 1]) return;
    const double pq = pg_sum_parts(part_pq, nbN, &sh);
    const double alpha = pq > 0.0 ? S->rz[j & 1] / pq : 0.0;
    const int i = blockIdx.x * PG_BLOCK + threadIdx.x;
    double rz = 0.0;
    if (i < N) {
        double r6[6], z6[6];
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            const size_t k = (size_t)a * N + i;
            x[k] += alpha * p[k];
            r6[a] = rr[k] - alpha * qv[k];
            rr[k] = r6[a];
        }
        double L[21];
#pragma unroll
        for (int q = 0; q < 21; ++q) L[q] = L21[(size_t)q * N + i];
        pg_precond(L, r6, z6);
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            z[(size_t)a * N + i] = z6[a];
            rz += r6[a] * z6[a];
        }
    }
    const double tot = pg_block_sum(rz, red);
    if (threadIdx.x == 0) part_rz[blockIdx.x] = tot;
}

// The trial state T' = exp(d_i) T_i with d = the CG's x; part_dd = sum d.d, part_pred = sum d.(lambda d - b)
__global__ __launch_bounds__(PG_BLOCK) void k_pg_trial(const PgState *__restrict__ S, const double *__restrict__ T, const double *__restrict__ x,
                                                        const double *__restrict__ b, int N, double *__restrict__ Tn,
                                                        double *__restrict__ part_dd, double *__restrict__ part_pred) {
    __shared__ double red[4];
    const double lambda = S->lambda;
    const int i = blockIdx.x * PG_BLOCK + threadIdx.x;
    double dd = 0.0, pred = 0.0;
    if (i < N) {
        double xi[6];
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            xi[a] = x[(size_t)a * N + i];
            dd += xi[a] * xi[a];
            pred += xi[a] * (lambda * xi[a] - b[(size_t)a * N + i]);
        }
        const double w0 = xi[0], w1 = xi[1], w2 = xi[2];
        const double th = sqrt((w0 * w0 + w1 * w1) + w2 * w2);
        const double sa = th < PG_SMALL ? 1.0 : sin(th) / th, sb = th < PG_SMALL ? 0.5 : (1.0 - cos(th)) / (th * th);
        const double K[9] = {0.0, -w2, w1, w2, 0.0, -w0, -w1, w0, 0.0};
        const double *A0 = T + (size_t)i * 16;
        double *A = Tn + (size_t)i * 16;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            double Er[4];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const double kk = (K[r * 3] * K[c] + K[r * 3 + 1] * K[3 + c]) + K[r * 3 + 2] * K[6 + c];
                Er[c] = ((r == c ? 1.0 : 0.0) + sa * K[r * 3 + c]) + sb * kk;
            }
            Er[3] = xi[3 + r];
#pragma unroll
            for (int c = 0; c < 4; ++c) A[r * 4 + c] = ((Er[0] * A0[c] + Er[1] * A0[4 + c]) + Er[2] * A0[8 + c]) + Er[3] * A0[12 + c];
        }
        A[12] = 0.0, A[13] = 0.0, A[14] = 0.0, A[15] = 1.0;
    }
    const double sdd = pg_block_sum(dd, red), sp = pg_block_sum(pred, red);
    if (threadIdx.x == 0) part_dd[blockIdx.x] = sdd, part_pred[blockIdx.x] = sp;
}

struct PgRules {
    double gradient_tolerance, step_tolerance, decrease_tolerance, residual_tolerance;
    int32_t max_iterations;
};

// One thread: the second stage of the iteration's sums, the gain ratio, Nielsen's rule, the stopping rules, the trace row.
__global__ void k_pg_decide(PgState *__restrict__ S, const double *__restrict__ part_F, const double *__restrict__ part_Fn, int nbE,
                            const double *__restrict__ part_dd, const double *__restrict__ part_pred, const double *__restrict__ part_grad,
                            int nbN, PgRules R, double *__restrict__ trace, int trace_cap) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double F = 0.0, Fn = 0.0, dd = 0.0, pred = 0.0, grad = 0.0;
    for (int k = 0; k < nbE; ++k) F += part_F[k];
    for (int k = 0; k < nbE; ++k) Fn += part_Fn[k];
    for (int k = 0; k < nbN; ++k) dd += part_dd[k];
    for (int k = 0; k < nbN; ++k) pred += part_pred[k];
    for (int k = 0; k < nbN; ++k) grad = fmax(grad, part_grad[k]);
    const double lambda = S->lambda, step = sqrt(dd);
    const double rho = (pred > 0.0 && Fn == Fn) ? (F - Fn) / pred : 0.0;
    int conv = 0, accepted = 0;
    double ln = lambda;
    if (F <= R.residual_tolerance) {
        conv = HV_POSE_GRAPH_RESIDUAL;
    } else if (grad <= R.gradient_tolerance) {
        conv = HV_POSE_GRAPH_GRADIENT;
    } else {
        accepted = rho > 0.0 ? 1 : 0;
        if (accepted) {
            const double q = 2.0 * rho - 1.0;
            ln = lambda * fmax(1.0 / 3.0, 1.0 - q * q * q);
            S->nu = 2.0;
        } else {
            ln = lambda * S->nu;
            S->nu = 2.0 * S->nu;
        }
        if (step <= R.step_tolerance)
            conv = HV_POSE_GRAPH_STEP;
        else if (accepted && (F - Fn) <= R.decrease_tolerance * F)
            conv = HV_POSE_GRAPH_DECREASE;
    }
    const int it = S->iter;
    if (it == 0) S->chi2_initial = F;
    S->chi2_final = accepted ? Fn : F;
    if (trace != nullptr && it < trace_cap) {
        double *row = trace + (size_t)it * HV_POSE_GRAPH_TRACE_STRIDE;
        row[0] = it, row[1] = lambda, row[2] = F, row[3] = Fn, row[4] = rho, row[5] = accepted, row[6] = S->cg_iters, row[7] = S->cg_res;
        row[8] = step, row[9] = grad, row[10] = ln, row[11] = conv;
    }
    S->F = F, S->Fnew = Fn, S->rho = rho, S->pred = pred, S->gradnorm = grad, S->stepnorm = step;
    S->lambda = ln;
    S->accepted = accepted;
    S->converged = conv;
    S->cg_total += S->cg_iters;
    S->iter = it + 1;
    S->stop = (conv != 0 || it + 1 >= R.max_iterations) ? 1 : 0;
}

__global__ __launch_bounds__(PG_BLOCK) void k_pg_commit(const PgState *__restrict__ S, const double *__restrict__ Tn, int64_t n,
                                                         double *__restrict__ T) {
    if (!S->accepted) return;
    const int64_t k = (int64_t)blockIdx.x * PG_BLOCK + threadIdx.x;
    if (k < n) T[k] = Tn[k];
}

struct PgLayout { // the call's scratch, every piece 256-byte aligned
    size_t off = 0;
    size_t take(size_t bytes) {
        const size_t at = off;
        off += (bytes + 255) & ~(size_t)255;
        return at;
    }
};
} // namespace
