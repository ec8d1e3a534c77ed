// hv_tsdf_register_volume: align one TSDF volume to another on the signed distance fields themselves (include/hipvol.h states the
// contract; tests/register_reference.py restates it in numpy).  Both volumes are only read.
//
//   collect    once per call, one workgroup per source unit in pool order: a voxel with weight > weight_threshold and |tsdf| <=
//              tsdf_band is a candidate.  A counting launch, a one-workgroup exclusive scan of the per-unit counts, the host reads
//              the total (0: nothing to align), then a filling launch writes {global voxel index, tsdf} - 16 bytes - at
//              offset[unit] + (ballot prefix inside the unit): a fixed order without an atomic append     k_reg_collect, k_reg_scan
//   linearise  per iteration, one thread per candidate (grid-stride): the point goes through the state A into the destination
//              lattice, eight gathers give the trilinear value and its analytic gradient, the 30 sums are reduced as tracking
//              reduces them (hv_gauss_newton.h) into one slab row per workgroup                                   k_reg_linearise
//   solve      one workgroup: the slab rows summed in a fixed order, Cholesky, A update, trace row, flag          k_reg_solve
// Every iteration is queued up front; a step of a finished call reads the flag and returns; the host waits once for the result.
// Iterations touch only the near-surface band of the source (the candidate list), not every allocated voxel; neighbours in the
// list fall into the same destination units, so the one-entry unit cache answers most of the eight unit look-ups (hv_tsdf_cell.h:
// the cell, its eight voxels, the trilinear value and gradient).
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "hv_common.h"
#include "hv_gauss_newton.h"
#include "hv_tsdf_cell.h"

namespace {

constexpr int RG_NACC = 30;         // H upper triangle [21], g [6], e, inliers, candidates
constexpr int RG_BLOCK = 256;       // linearise workgroup (4 waves)
constexpr int RG_MAX_BLOCKS = 1024; // linearise grid cap = slab rows

struct RgCand { // 16 bytes
    int32_t gx, gy, gz; // global voxel index, 16 key + xyz
    float tsdf;
};
static_assert(sizeof(RgCand) == 16, "a candidate is one 16-byte record");

struct RgState {
    double A[16];         // the state, row-major; identity at the start
    double last[RG_NACC]; // sums of the last linearisation
    int32_t done;         // 0 running, 1 converged, 2 degenerate
    int32_t iters;        // linearisations run
    int32_t rows;         // trace rows written
    int32_t pad;
};

struct RgXf {
    double R0[9];  // rotation of T_init, row-major
    double cs[3];  // anchor in the source frame
    double c[3];   // anchor in the destination frame, T_init cs
    double voxel_length, sdf_trunc;
    double grad_scale; // sdf_trunc / voxel_length
    double weight_threshold, residual_trunc, huber_delta;
};

__global__ __launch_bounds__(64) void k_reg_init(RgState *st) {
    const int t = threadIdx.x;
    if (t < 16) st->A[t] = (t % 5 == 0) ? 1.0 : 0.0;
    if (t < RG_NACC) st->last[t] = 0.0;
    if (t == 0) st->done = st->iters = st->rows = st->pad = 0;
}

// One workgroup per source unit.  A step covers the 256 words of one z plane (lane -> word: 1 KiB per plane and wave instruction).
// FILL = false: counts[unit] = candidates of the unit.  FILL = true: counts holds the exclusive scan; the unit's candidates go to
// list[counts[unit] ...] in word order (z, x, y).
template <bool FILL>
__global__ __launch_bounds__(256) void k_reg_collect(const unsigned long long *__restrict__ keys, const char *__restrict__ pool,
                                                     double weight_threshold, double tsdf_band, int64_t *__restrict__ counts,
                                                     RgCand *__restrict__ list) {
    __shared__ int32_t s_wave[4];
    const int32_t unit = (int32_t)blockIdx.x;
    const float *t = (const float *)(pool + (int64_t)unit * HV_TSDF_UNIT_BYTES);
    const uint32_t *w = (const uint32_t *)(pool + (int64_t)unit * HV_TSDF_UNIT_BYTES + HV_TSDF_PLANE_BYTES);
    const int tid = (int)threadIdx.x, lane = hv_lane_id(), wave = tid >> 6;
    int32_t kx = 0, ky = 0, kz = 0;
    int64_t at = 0;
    if (FILL) {
        hv_unpack_key(keys[unit], kx, ky, kz);
        at = counts[unit];
    }
    int32_t n = 0;
    for (int z = 0; z < HV_TSDF_R; ++z) {
        const int word = z * HV_TSDF_RR + tid;
        const float tv = t[word];
        const bool is = (double)w[word] > weight_threshold && fabs((double)tv) <= tsdf_band;
        if (FILL) {
            const unsigned long long m = __ballot(is);
            if (lane == 0) s_wave[wave] = (int32_t)__popcll(m);
            __syncthreads();
            int32_t before = 0, total = 0;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                before += v < wave ? s_wave[v] : 0;
                total += s_wave[v];
            }
            if (is) {
                const unsigned long long lower = lane == 0 ? 0ull : (~0ull >> (64 - lane));
                list[at + before + (int32_t)__popcll(m & lower)] = RgCand{kx * HV_TSDF_R + (tid >> 4), ky * HV_TSDF_R + (tid & 15), kz * HV_TSDF_R + z, tv};
            }
            at += total;
            __syncthreads();
        } else {
            n += is ? 1 : 0;
        }
    }
    if (!FILL) {
        n = hv_wave_sum(n);
        if (lane == 0) s_wave[wave] = n;
        __syncthreads();
        if (tid == 0) counts[unit] = (int64_t)((s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]));
    }
}

// counts[0, n) -> its exclusive scan in place, counts[n] = the total.  One workgroup of 1024 threads, a run of units per thread.
__global__ __launch_bounds__(1024) void k_reg_scan(int64_t *__restrict__ counts, int32_t n) {
    __shared__ int64_t s_sum[1024];
    const int tid = (int)threadIdx.x;
    const int64_t per = ((int64_t)n + 1023) / 1024;
    const int32_t lo = (int32_t)(tid * per < n ? tid * per : n), hi = (int32_t)(lo + per < n ? lo + per : n);
    int64_t s = 0;
    for (int32_t i = lo; i < hi; ++i) s += counts[i];
    s_sum[tid] = s;
    __syncthreads();
    if (tid == 0) {
        int64_t run = 0;
        for (int i = 0; i < 1024; ++i) {
            const int64_t c = s_sum[i];
            s_sum[i] = run;
            run += c;
        }
        counts[n] = run;
    }
    __syncthreads();
    int64_t run = s_sum[tid];
    for (int32_t i = lo; i < hi; ++i) {
        const int64_t c = counts[i];
        counts[i] = run;
        run += c;
    }
}

// One step's linearisation: per workgroup the 30 sums of its candidates -> slab[blockIdx.x].
__global__ __launch_bounds__(RG_BLOCK) void k_reg_linearise(const RgCand *__restrict__ list, int64_t n, HvTable dst, const char *__restrict__ pool,
                                                            RgXf X, const RgState *__restrict__ st, double *__restrict__ slab) {
    if (st->done != 0) return; // (uniform: every thread reads the same flag)
    double A[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) A[k] = st->A[k];
    double acc[RG_NACC];
#pragma unroll
    for (int k = 0; k < RG_NACC; ++k) acc[k] = 0.0;
    unsigned long long ck = HV_EMPTY_KEY;
    int32_t ci = -1;

    for (int64_t i = (int64_t)blockIdx.x * RG_BLOCK + threadIdx.x; i < n; i += (int64_t)gridDim.x * RG_BLOCK) {
        const RgCand cand = list[i];
        acc[29] += 1.0;
        const double d0 = ((double)cand.gx + 0.5) * X.voxel_length - X.cs[0];
        const double d1 = ((double)cand.gy + 0.5) * X.voxel_length - X.cs[1];
        const double d2 = ((double)cand.gz + 0.5) * X.voxel_length - X.cs[2];
        const double q0 = (X.R0[0] * d0 + X.R0[1] * d1) + X.R0[2] * d2;
        const double q1 = (X.R0[3] * d0 + X.R0[4] * d1) + X.R0[5] * d2;
        const double q2 = (X.R0[6] * d0 + X.R0[7] * d1) + X.R0[8] * d2;
        const double y[3] = {((A[0] * q0 + A[1] * q1) + A[2] * q2) + A[3], ((A[4] * q0 + A[5] * q1) + A[6] * q2) + A[7],
                             ((A[8] * q0 + A[9] * q1) + A[10] * q2) + A[11]};
        const double p[3] = {X.c[0] + y[0], X.c[1] + y[1], X.c[2] + y[2]};
        int32_t g0[3];
        double r[3];
        if (!hv_cell_locate(p, X.voxel_length, g0, r)) continue;
        int64_t at[8];
        if (hv_tsdf_cell_gather(dst, g0, ck, ci, at) != 0xffu) continue;
        bool all = true;
#pragma unroll
        for (int c = 0; c < 8; ++c) all = all && (double)((const uint32_t *)pool)[at[c] + HV_TSDF_RRR] > X.weight_threshold;
        if (!all) continue;
        double f[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) f[c] = (double)((const float *)pool)[at[c]];
        double phi, e[3];
        hv_cell_lerp_grad(r, f, phi, e);
        const double rho = X.sdf_trunc * (phi - (double)cand.tsdf);
        if (!(fabs(rho) <= X.residual_trunc)) continue;
        const double n0 = X.grad_scale * e[0], n1 = X.grad_scale * e[1], n2 = X.grad_scale * e[2];
        const double J[6] = {y[1] * n2 - y[2] * n1, y[2] * n0 - y[0] * n2, y[0] * n1 - y[1] * n0, n0, n1, n2};
        const double w = fabs(rho) <= X.huber_delta ? 1.0 : X.huber_delta / fabs(rho);
        int k = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            const double wa = w * J[a];
#pragma unroll
            for (int b = a; b < 6; ++b) acc[k++] += wa * J[b];
            acc[21 + a] += wa * rho;
        }
        acc[27] += rho * rho;
        acc[28] += 1.0;
    }

    __shared__ double red[RG_BLOCK / 64][RG_NACC];
    hv_gn_block_reduce<RG_NACC, RG_BLOCK>(acc, red, slab + (int64_t)blockIdx.x * RG_NACC);
}

// one step's solve: the slab summed in a fixed order, then (thread 0) the Gauss-Newton step, trace row, flag
__global__ __launch_bounds__(HV_GN_SUM_THREADS) void k_reg_solve(RgState *__restrict__ st, const double *__restrict__ slab, int rows, int iteration,
                                                                 double *__restrict__ trace, int trace_cap) {
    if (st->done != 0) return;
    __shared__ double part[HV_GN_SUM_PARTS][32];
    __shared__ double tot[RG_NACC];
    hv_gn_slab_sum<RG_NACC>(slab, rows, part, tot);
    if (threadIdx.x < RG_NACC) st->last[threadIdx.x] = tot[threadIdx.x];
    __syncthreads();
    if (threadIdx.x != 0) return;

    double A0[16], g[6], xi[6];
    const int status = hv_gn_step(tot, (double)HV_REGISTER_MIN_INLIERS, HV_REGISTER_PIVOT_REL, HV_REGISTER_CONVERGED, st->A, A0, g, xi);
    const int row = st->rows;
    if (trace != nullptr && row < trace_cap) {
        double *o = trace + (int64_t)row * HV_REGISTER_TRACE_STRIDE;
        o[0] = iteration;
        o[1] = status;
        o[2] = tot[28];
        o[3] = tot[29];
        o[4] = tot[27];
        for (int i = 0; i < 16; ++i) o[5 + i] = A0[i];
        for (int i = 0; i < 21; ++i) o[21 + i] = tot[i];
        for (int i = 0; i < 6; ++i) o[42 + i] = g[i];
        for (int i = 0; i < 6; ++i) o[48 + i] = xi[i];
    }
    st->rows = row + 1;
    st->iters += 1;
    if (status != 0) st->done = status;
}

// linearise grid: one thread per candidate up to RG_MAX_BLOCKS workgroups.  HV_REGISTER_GRID_BLOCKS (1 .. RG_MAX_BLOCKS) lowers the
// cap, so that a test reaches the grid-stride remainder with a map of a few units
int register_grid_cap() {
    const char *e = std::getenv("HV_REGISTER_GRID_BLOCKS");
    if (e == nullptr || *e == 0) return RG_MAX_BLOCKS;
    const long v = std::strtol(e, nullptr, 10);
    return (int)std::min<long>(std::max<long>(v, 1), RG_MAX_BLOCKS);
}

} // namespace

extern "C" int hv_tsdf_register_volume(hv_volume *dst, hv_volume *src, const double *T, const hv_register_params *prm, hv_register_result *res,
                                       double *trace, int64_t trace_cap, int64_t *trace_rows) {
    HV_REQUIRE(dst != nullptr && src != nullptr && T != nullptr && prm != nullptr && res != nullptr, HV_ERR_INVALID,
               "hv_tsdf_register_volume: null argument");
    const char *fn = "hv_tsdf_register_volume";
    int rc = hv_tsdf_require_whole_map(dst, fn, "the destination");
    if (rc != HV_OK) return rc;
    rc = hv_tsdf_require_whole_map(src, fn, "the source");
    if (rc != HV_OK) return rc;
    HV_REQUIRE(dst != src, HV_ERR_INVALID, "hv_tsdf_register_volume: source and destination are the same volume");
    HV_REQUIRE(dst->cfg.voxel_size == src->cfg.voxel_size && dst->cfg.sdf_trunc == src->cfg.sdf_trunc && dst->cfg.block_size == src->cfg.block_size,
               HV_ERR_INVALID, "hv_tsdf_register_volume: the volumes differ in voxel_length (%g / %g), sdf_trunc (%g / %g) or unit resolution (%d / %d)",
               dst->cfg.voxel_size, src->cfg.voxel_size, dst->cfg.sdf_trunc, src->cfg.sdf_trunc, (int)dst->cfg.block_size, (int)src->cfg.block_size);
    HV_REQUIRE(dst->device == src->device, HV_ERR_INVALID, "hv_tsdf_register_volume: the volumes live on different devices (%d / %d)", dst->device,
               src->device);
    for (int i = 0; i < 16; ++i) HV_REQUIRE(std::isfinite(T[i]), HV_ERR_INVALID, "hv_tsdf_register_volume: the initial transformation is not finite");
    HV_REQUIRE(T[12] == 0.0 && T[13] == 0.0 && T[14] == 0.0 && T[15] == 1.0, HV_ERR_INVALID,
               "hv_tsdf_register_volume: the initial transformation's bottom row is not (0, 0, 0, 1)");
    RgXf X{};
    double ortho = 0.0;
    for (int a = 0; a < 3; ++a) {
        double row = 0.0;
        for (int b = 0; b < 3; ++b) {
            double s = 0.0;
            for (int k = 0; k < 3; ++k) s += T[k * 4 + a] * T[k * 4 + b];
            row += std::fabs(s - (a == b ? 1.0 : 0.0));
            X.R0[a * 3 + b] = T[a * 4 + b];
        }
        ortho = std::max(ortho, row);
    }
    const double det = T[0] * (T[5] * T[10] - T[6] * T[9]) - T[1] * (T[4] * T[10] - T[6] * T[8]) + T[2] * (T[4] * T[9] - T[5] * T[8]);
    HV_REQUIRE(ortho <= 1.0e-6 && det >= 0.0, HV_ERR_INVALID,
               "hv_tsdf_register_volume: the initial transformation is not rigid (|R^T R - I|_inf = %.3g, det = %.3g)", ortho, det);
    HV_REQUIRE(prm->max_iterations >= 1 && prm->max_iterations <= 10000, HV_ERR_INVALID, "hv_tsdf_register_volume: bad max_iterations %d (1 .. 10000)",
               (int)prm->max_iterations);
    HV_REQUIRE(std::isfinite(prm->weight_threshold) && prm->weight_threshold >= 0.0, HV_ERR_INVALID,
               "hv_tsdf_register_volume: weight_threshold must be finite and >= 0");
    HV_REQUIRE(prm->tsdf_band > 0.0 && prm->tsdf_band <= 1.0, HV_ERR_INVALID, "hv_tsdf_register_volume: tsdf_band %g is outside (0, 1]", prm->tsdf_band);
    HV_REQUIRE(std::isfinite(prm->residual_trunc) && prm->residual_trunc > 0.0 && std::isfinite(prm->huber_delta) && prm->huber_delta > 0.0,
               HV_ERR_INVALID, "hv_tsdf_register_volume: residual_trunc and huber_delta must be positive");
    HV_REQUIRE(trace == nullptr || trace_cap >= 0, HV_ERR_INVALID, "hv_tsdf_register_volume: negative trace_cap");

    // what a call that finds nothing to align returns
    *res = hv_register_result{};
    for (int i = 0; i < 16; ++i) res->T_dst_src[i] = T[i];
    if (trace_rows) *trace_rows = 0;

    // drain both batch pipelines; the source's pending work is done before the destination's stream reads it
    int64_t src_used = 0;
    rc = hv_tsdf_drain(src, fn, false, &src_used);
    if (rc == HV_OK) rc = hv_tsdf_drain(dst, fn, false, nullptr);
    if (rc != HV_OK) return rc;
    HV_REQUIRE(src->h_counters[HV_CNT_OVERFLOW] == 0 && !src->overflow_latched, HV_ERR_CAPACITY,
               "%s: the source's block pool overflowed earlier (hv_reserve_blocks or hv_reset it first)", fn);
    if (src_used == 0) return HV_OK;

    // anchor: the centre of the bounding box of the source's unit keys, and where T_init puts it
    {
        std::vector<unsigned long long> keys((size_t)src_used);
        HV_HIP(hipMemcpy(keys.data(), src->table.block_keys, sizeof(unsigned long long) * (size_t)src_used, hipMemcpyDeviceToHost));
        int32_t lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
        for (unsigned long long key : keys) {
            int32_t k[3];
            hv_unpack_key(key, k[0], k[1], k[2]);
            for (int a = 0; a < 3; ++a) {
                lo[a] = std::min(lo[a], k[a]);
                hi[a] = std::max(hi[a], k[a]);
            }
        }
        X.voxel_length = dst->cfg.voxel_size;
        X.sdf_trunc = dst->cfg.sdf_trunc;
        for (int a = 0; a < 3; ++a) X.cs[a] = ((double)((int64_t)lo[a] + hi[a] + 1) * 0.5) * ((double)HV_TSDF_R * X.voxel_length);
        for (int a = 0; a < 3; ++a) {
            X.c[a] = ((T[a * 4] * X.cs[0] + T[a * 4 + 1] * X.cs[1]) + T[a * 4 + 2] * X.cs[2]) + T[a * 4 + 3];
            res->anchor[a] = X.c[a];
        }
    }
    X.grad_scale = X.sdf_trunc / X.voxel_length;
    X.weight_threshold = prm->weight_threshold;
    X.residual_trunc = prm->residual_trunc;
    X.huber_delta = prm->huber_delta;

    // scratch, freed on return: [state][slab][trace][per-unit counts / offsets, src_used + 1 int64], then the candidate list
    const int steps = prm->max_iterations;
    size_t off = 0;
    auto take = [&off](size_t bytes) { // -> the offset of the next bytes, every piece 256-byte aligned
        const size_t at = off;
        off += (bytes + 255) & ~(size_t)255;
        return at;
    };
    const size_t o_state = take(sizeof(RgState));
    const size_t o_slab = take(sizeof(double) * RG_NACC * RG_MAX_BLOCKS);
    const size_t o_trace = take(sizeof(double) * HV_REGISTER_TRACE_STRIDE * (size_t)steps);
    const size_t o_counts = take(sizeof(int64_t) * (size_t)(src_used + 1));
    HvScratch S;
    char *base = nullptr;
    RgCand *list = nullptr;
    HV_HIP(S.get(&base, off));
    auto fail = [&](const char *what, hipError_t e) {
        hv_set_error("hv_tsdf_register_volume: %s failed: %s", what, hipGetErrorString(e));
        return HV_ERR_DEVICE;
    };
    RgState *st = (RgState *)(base + o_state);
    double *slab = (double *)(base + o_slab);
    double *d_trace = (double *)(base + o_trace);
    int64_t *d_counts = (int64_t *)(base + o_counts);
    hipStream_t s = dst->stream;

    hipLaunchKernelGGL(k_reg_collect<false>, dim3((unsigned)src_used), dim3(256), 0, s, (const unsigned long long *)src->table.block_keys,
                       (const char *)src->pool, prm->weight_threshold, prm->tsdf_band, d_counts, (RgCand *)nullptr);
    hipLaunchKernelGGL(k_reg_scan, dim3(1), dim3(1024), 0, s, d_counts, (int32_t)src_used);
    int64_t n_cand = 0;
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(&n_cand, d_counts + src_used, sizeof(int64_t), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail("the candidate count", e);
    if (n_cand <= 0) return HV_OK; // no near-surface voxel in the source
    e = S.get(&list, (size_t)n_cand);
    if (e != hipSuccess) return fail("allocating the candidate list", e);

    hipLaunchKernelGGL(k_reg_collect<true>, dim3((unsigned)src_used), dim3(256), 0, s, (const unsigned long long *)src->table.block_keys,
                       (const char *)src->pool, prm->weight_threshold, prm->tsdf_band, d_counts, list);
    hipLaunchKernelGGL(k_reg_init, dim3(1), dim3(64), 0, s, st);
    const int blocks = (int)std::min<int64_t>((n_cand + RG_BLOCK - 1) / RG_BLOCK, register_grid_cap());
    for (int it = 0; it < steps; ++it) {
        hipLaunchKernelGGL(k_reg_linearise, dim3((unsigned)blocks), dim3(RG_BLOCK), 0, s, (const RgCand *)list, n_cand, dst->table,
                           (const char *)dst->pool, X, (const RgState *)st, slab);
        hipLaunchKernelGGL(k_reg_solve, dim3(1), dim3(HV_GN_SUM_THREADS), 0, s, st, (const double *)slab, blocks, it,
                           trace ? d_trace : (double *)nullptr, steps);
    }
    RgState h{};
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(&h, st, sizeof(RgState), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail("the iterations", e);
    if (trace != nullptr) {
        const int64_t n = std::min<int64_t>(h.rows, trace_cap);
        if (n > 0) {
            e = hipMemcpy(trace, d_trace, sizeof(double) * HV_REGISTER_TRACE_STRIDE * (size_t)n, hipMemcpyDeviceToHost);
            if (e != hipSuccess) return fail("reading the trace", e);
        }
        if (trace_rows) *trace_rows = n;
    }

    // T = Tr(c) A Tr(-c) T_init: M = [R_A, (c + t_A) - R_A c], T = M T_init.  A state that never moved returns T_init as it came.
    bool moved = false;
    for (int i = 0; i < 16; ++i) moved = moved || h.A[i] != ((i % 5 == 0) ? 1.0 : 0.0);
    if (moved) {
        double M[16] = {};
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) M[r * 4 + c] = h.A[r * 4 + c];
            M[r * 4 + 3] = (X.c[r] + h.A[r * 4 + 3]) - ((h.A[r * 4] * X.c[0] + h.A[r * 4 + 1] * X.c[1]) + h.A[r * 4 + 2] * X.c[2]);
        }
        M[15] = 1.0;
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c)
                res->T_dst_src[r * 4 + c] = M[r * 4] * T[c] + M[r * 4 + 1] * T[4 + c] + M[r * 4 + 2] * T[8 + c] + M[r * 4 + 3] * T[12 + c];
    }
    {
        int q = 0;
        for (int a = 0; a < 6; ++a)
            for (int b = a; b < 6; ++b) res->information[a * 6 + b] = res->information[b * 6 + a] = h.last[q++];
    }
    const double err = h.last[27], inl = h.last[28], cand = h.last[29];
    res->inliers = (int64_t)inl;
    res->candidates = (int64_t)cand;
    res->fitness = cand > 0.0 ? inl / cand : 0.0;
    res->inlier_rmse = inl > 0.0 ? std::sqrt(err / inl) : 0.0;
    res->iterations = h.iters;
    res->success = (h.done != 2 && inl >= (double)HV_REGISTER_MIN_INLIERS) ? 1 : 0;
    return HV_OK;
}
