// libpyslam_hipvol.so — frame-to-model tracking against the fused TSDF map on gfx950: point-to-plane (hv_tsdf_track) and hybrid,
// point-to-plane plus a photometric term on the map's colour (hv_tsdf_track_color).  The contracts (pyramid, model, association,
// linearisation, solve, stopping, outputs) are written once in include/hipvol.h; tests/track_reference.py and
// tests/track_color_reference.py restate them in numpy.
//
// Per call, all on the volume's stream and queued up front: one launch per source pyramid level, one ray cast per level (the
// model, k_tsdf_ray_cast through hv_ray_cast_launch), then for every iteration of every level a linearise launch (one thread per
// source pixel, grid-stride; wave butterfly + LDS reduction of the 30 sums in double into one slab row per workgroup) and a
// one-workgroup solve launch (the slab summed in a fixed order, Cholesky, A update, trace row, level flag).  A step of a level that
// has converged or gone degenerate reads the flag and returns.  No float atomics anywhere: results are bitwise reproducible.  The
// reduction, the slab sum and the 6 x 6 step are hv_gauss_newton.h's, shared with map-to-map registration (hv_register.hip).
//
// The hybrid call runs the same schedule with the same kernels, instantiated with the hybrid part that sits under `if constexpr`:
// k_track_source<true> / k_track_down<true> also produce the source intensity of the level, the casts also render colour, one
// model-preparation launch per level packs {I_m, g_x, g_y, has-gradient} into a 16-byte record per model pixel, and
// k_track_linearise<32> adds the photometric rank-1 update and two more sums (32 instead of 30).  The geometric body, workgroup
// size, grid rule and reduction are one text for both instantiations - so with intensity_weight = 0 every float64 sum associates
// as in the depth-only call and the two agree bit for bit.
#include <cmath>

#include "hv_common.h"
#include "hv_gauss_newton.h"

namespace {

constexpr int TK_NACC = 30;          // H upper triangle [21], g [6], e, inliers, valid
constexpr int TK_NACC_COLOR = 32;    // ... photometric inliers, sum r_I^2
constexpr int TK_BLOCK = 256;        // linearise workgroup (4 waves)
constexpr int TK_MAX_BLOCKS = 1024;  // linearise grid cap = slab rows
constexpr int TK_SUM_PARTS = HV_GN_SUM_PARTS;
constexpr int TK_SUM_THREADS = HV_GN_SUM_THREADS;

template <int NACC>
struct TkStateT {
    double A[16];                          // current camera -> anchor, row-major
    double last[NACC];                     // sums of the last level-0 linearisation
    int32_t done[HV_TRACK_MAX_LEVELS];     // 0 running, 1 converged, 2 degenerate
    int32_t iters[HV_TRACK_MAX_LEVELS];    // linearisations run
    int32_t rows;                          // trace rows written
    int32_t pad;
};
using TkState = TkStateT<TK_NACC>;
using TkStateColor = TkStateT<TK_NACC_COLOR>;

struct TkLevel {
    const float *src;        // source depth of the level, metres, 0 = invalid
    const float *mdepth;     // model (cast) depth
    const float *mnormal;    // model normal, world frame [H,W,3]
    const uint8_t *mmask;    // model hit mask
    int32_t height, width;
    double fx, fy, cx, cy;
};

struct TkParams {
    double R0[9];  // R_cw_init: world normal -> anchor frame
    double trunc, delta;
};

struct TkColor {
    const float4 *mrec;  // model record of the level: {I_m, g_x, g_y, has-gradient (1 or 0)}
    const float *isrc;   // source intensity of the level
    double lambda, delta;
};

template <int NACC>
__global__ __launch_bounds__(64) void k_track_init(TkStateT<NACC> *st) {
    const int t = threadIdx.x;
    if (t < 16) st->A[t] = (t % 5 == 0) ? 1.0 : 0.0;
    if (t < NACC) st->last[t] = 0.0;
    if (t < HV_TRACK_MAX_LEVELS) {
        st->done[t] = 0;
        st->iters[t] = 0;
    }
    if (t == 0) st->rows = 0;
}

// level 0: depth / depth_scale in float32; valid iff finite and in (depth_min, depth_max] (double compares), else 0.  HYBRID: also
// the intensity ((0.299f R + 0.587f G) + 0.114f B) / 255f of every pixel (depth only: rgb and iout are null and not read)
template <bool HYBRID>
__global__ __launch_bounds__(256) void k_track_source(const void *__restrict__ raw, int is_u16, const uint8_t *__restrict__ rgb, int bgr,
                                                      int64_t npx, float scale, double dmin, double dmax, float *__restrict__ out,
                                                      float *__restrict__ iout) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npx) return;
    float d = is_u16 ? (float)((const uint16_t *)raw)[i] : ((const float *)raw)[i];
    d = d / scale;
    out[i] = (isfinite(d) && (double)d > dmin && (double)d <= dmax) ? d : 0.0f;
    if constexpr (HYBRID) {
        const uint8_t *c = rgb + 3 * i;
        const float r = (float)c[bgr ? 2 : 0], g = (float)c[1], b = (float)c[bgr ? 0 : 2];
        iout[i] = ((0.299f * r + 0.587f * g) + 0.114f * b) / 255.0f;
    }
}

// level l -> l + 1: float32 mean of the valid 2x2 children (fixed order), valid iff max - min <= trunc.  HYBRID: also the float32
// mean of all four children's intensities, same child order (depth only: iin and iout are null and not read)
template <bool HYBRID>
__global__ __launch_bounds__(256) void k_track_down(const float *__restrict__ in, const float *__restrict__ iin, int32_t w_in,
                                                    float *__restrict__ out, float *__restrict__ iout, int32_t h_out, int32_t w_out,
                                                    double trunc) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)h_out * w_out) return;
    const int u = (int)(i % w_out), v = (int)(i / w_out);
    const int64_t o0 = (int64_t)(2 * v) * w_in + 2 * u;
    const float *r0 = in + o0, *r1 = r0 + w_in;
    const float c[4] = {r0[0], r0[1], r1[0], r1[1]};
    float sum = 0.0f, mx = -INFINITY, mn = INFINITY;
    int n = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (c[k] > 0.0f) {
            sum = sum + c[k];
            mx = fmaxf(mx, c[k]);
            mn = fminf(mn, c[k]);
            ++n;
        }
    }
    out[i] = (n > 0 && (double)(mx - mn) <= trunc) ? sum / (float)n : 0.0f;
    if constexpr (HYBRID) {
        const float *i0 = iin + o0, *i1 = i0 + w_in;
        iout[i] = (((i0[0] + i0[1]) + i1[0]) + i1[1]) * 0.25f;
    }
}

__device__ __forceinline__ float tk_model_intensity(const float *__restrict__ color, int64_t m) {
    return (0.299f * color[3 * m] + 0.587f * color[3 * m + 1]) + 0.114f * color[3 * m + 2];
}

// hybrid, per level: the cast's colour, depth and mask -> one record {I_m, g_x, g_y, has-gradient} per model pixel.  A pixel has a
// gradient iff it is off the border, the mask is set at it and its four neighbours, and no neighbour's depth is further than trunc
// from its own (difference and compare in double); g_x = g_y = 0 where it has none.
__global__ __launch_bounds__(256) void k_track_model_prep(const float *__restrict__ color, const float *__restrict__ depth,
                                                          const uint8_t *__restrict__ mask, int32_t height, int32_t width, double trunc,
                                                          float4 *__restrict__ rec) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)height * width) return;
    const int u = (int)(i % width), v = (int)(i / width);
    float4 o = make_float4(tk_model_intensity(color, i), 0.0f, 0.0f, 0.0f);
    if (u >= 1 && v >= 1 && u + 1 < width && v + 1 < height && mask[i]) {
        const int64_t nb[4] = {i + 1, i - 1, i + width, i - width};
        const double z = (double)depth[i];
        bool ok = true;
#pragma unroll
        for (int k = 0; k < 4; ++k) ok = ok && mask[nb[k]] && fabs((double)depth[nb[k]] - z) <= trunc;
        if (ok) {
            o.y = 0.5f * (tk_model_intensity(color, nb[0]) - tk_model_intensity(color, nb[1]));
            o.z = 0.5f * (tk_model_intensity(color, nb[2]) - tk_model_intensity(color, nb[3]));
            o.w = 1.0f;
        }
    }
    rec[i] = o;
}


// one step's linearisation: per workgroup the NACC sums of its pixels -> slab[blockIdx.x].  NACC = 30 is the depth-only call (C is
// not read); NACC = 32 the hybrid one: for an inlier whose model pixel has a gradient also the photometric products into the same
// accumulators, and two more sums.  The geometric part and the reduction are this one text for both, which is what makes the
// hybrid call with intensity_weight = 0 associate every float64 sum as the depth-only call does.
template <int NACC>
__global__ __launch_bounds__(TK_BLOCK) void k_track_linearise(TkLevel L, TkParams P, TkColor C, const TkStateT<NACC> *__restrict__ st,
                                                              int level, double *__restrict__ slab) {
    constexpr bool HYBRID = NACC == TK_NACC_COLOR;
    static_assert(HYBRID || NACC == TK_NACC, "30 sums (depth only) or 32 (hybrid)");
    if (st->done[level] != 0) return; // (uniform: every thread reads the same flag)
    double A[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) A[k] = st->A[k];
    double acc[NACC];
#pragma unroll
    for (int k = 0; k < NACC; ++k) acc[k] = 0.0;

    const int64_t npx = (int64_t)L.height * L.width;
    for (int64_t pix = (int64_t)blockIdx.x * TK_BLOCK + threadIdx.x; pix < npx; pix += (int64_t)gridDim.x * TK_BLOCK) {
        const float ds = L.src[pix];
        if (!(ds > 0.0f)) continue;
        acc[29] += 1.0;
        const int u = (int)(pix % L.width), v = (int)(pix / L.width);
        const double d = (double)ds;
        const double pc0 = d * (((double)u - L.cx) / L.fx), pc1 = d * (((double)v - L.cy) / L.fy), pc2 = d;
        const double p0 = A[0] * pc0 + A[1] * pc1 + A[2] * pc2 + A[3];
        const double p1 = A[4] * pc0 + A[5] * pc1 + A[6] * pc2 + A[7];
        const double p2 = A[8] * pc0 + A[9] * pc1 + A[10] * pc2 + A[11];
        if (!(p2 > 0.0)) continue;
        const double xf = L.fx * p0 / p2 + L.cx, yf = L.fy * p1 / p2 + L.cy;
        const double uf = floor(xf + 0.5), vf = floor(yf + 0.5);
        if (!(uf >= 0.0 && uf < (double)L.width && vf >= 0.0 && vf < (double)L.height)) continue;
        const int64_t m = (int64_t)vf * L.width + (int64_t)uf;
        if (!L.mmask[m]) continue;
        const double z = (double)L.mdepth[m];
        const double q0 = z * ((uf - L.cx) / L.fx), q1 = z * ((vf - L.cy) / L.fy), q2 = z;
        const double nw0 = (double)L.mnormal[3 * m], nw1 = (double)L.mnormal[3 * m + 1], nw2 = (double)L.mnormal[3 * m + 2];
        const double n0 = P.R0[0] * nw0 + P.R0[1] * nw1 + P.R0[2] * nw2;
        const double n1 = P.R0[3] * nw0 + P.R0[4] * nw1 + P.R0[5] * nw2;
        const double n2 = P.R0[6] * nw0 + P.R0[7] * nw1 + P.R0[8] * nw2;
        const double e0 = p0 - q0, e1 = p1 - q1, e2 = p2 - q2;
        if (!(sqrt(e0 * e0 + e1 * e1 + e2 * e2) <= P.trunc)) continue;
        const double r = n0 * e0 + n1 * e1 + n2 * e2;
        const double J[6] = {p1 * n2 - p2 * n1, p2 * n0 - p0 * n2, p0 * n1 - p1 * n0, n0, n1, n2};
        const double w = fabs(r) <= P.delta ? 1.0 : P.delta / fabs(r);
        int k = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a) {
            const double wa = w * J[a];
#pragma unroll
            for (int b = a; b < 6; ++b) acc[k++] += wa * J[b];
            acc[21 + a] += wa * r;
        }
        acc[27] += r * r;
        acc[28] += 1.0;

        if constexpr (HYBRID) {
            const float4 rec = C.mrec[m];
            if (rec.w == 0.0f) continue;
            const double gx = (double)rec.y, gy = (double)rec.z;
            const double ri = (((double)rec.x + gx * (xf - uf)) + gy * (yf - vf)) - (double)C.isrc[pix];
            const double ga = gx * L.fx / p2, gb = gy * L.fy / p2;
            const double gc = -(ga * p0 + gb * p1) / p2;
            const double JI[6] = {p1 * gc - p2 * gb, p2 * ga - p0 * gc, p0 * gb - p1 * ga, ga, gb, gc};
            const double wi = C.lambda * (fabs(ri) <= C.delta ? 1.0 : C.delta / fabs(ri));
            k = 0;
#pragma unroll
            for (int a = 0; a < 6; ++a) {
                const double wa = wi * JI[a];
#pragma unroll
                for (int b = a; b < 6; ++b) acc[k++] += wa * JI[b];
                acc[21 + a] += wa * ri;
            }
            acc[30] += 1.0;
            acc[31] += ri * ri;
        }
    }

    __shared__ double red[TK_BLOCK / 64][NACC];
    hv_gn_block_reduce<NACC, TK_BLOCK>(acc, red, slab + (int64_t)blockIdx.x * NACC);
}

// one step's solve: the slab summed in a fixed order, then (thread 0) Cholesky, exp, A update, trace row, flag
// (NACC sums per slab row, at most 32; a trace row of STRIDE doubles: the sums past the depth-only 30 follow its 56 fields)
template <int NACC, int STRIDE>
__global__ __launch_bounds__(TK_SUM_THREADS) void k_track_solve(TkStateT<NACC> *__restrict__ st, const double *__restrict__ slab, int rows,
                                                                int level, int iteration, double *__restrict__ trace, int trace_cap) {
    static_assert(NACC >= TK_NACC && NACC <= 32 && STRIDE == 56 + NACC - TK_NACC, "slab row / trace row layout");
    if (st->done[level] != 0) return;
    __shared__ double part[TK_SUM_PARTS][32];
    __shared__ double tot[NACC];
    hv_gn_slab_sum<NACC>(slab, rows, part, tot);
    if (threadIdx.x < NACC && level == 0) st->last[threadIdx.x] = tot[threadIdx.x];
    __syncthreads();
    if (threadIdx.x != 0) return;

    double A0[16], g[6], xi[6];
    const int status = hv_gn_step(tot, (double)HV_TRACK_MIN_INLIERS, HV_TRACK_PIVOT_REL, HV_TRACK_CONVERGED, st->A, A0, g, xi);
    const double inliers = tot[28];
    const int row = st->rows;
    if (trace != nullptr && row < trace_cap) {
        double *o = trace + (int64_t)row * STRIDE;
        o[0] = level;
        o[1] = iteration;
        o[2] = status;
        o[3] = inliers;
        o[4] = tot[29];
        o[5] = tot[27];
        for (int i = 0; i < 16; ++i) o[6 + i] = A0[i];
        for (int i = 0; i < 21; ++i) o[22 + i] = tot[i];
        for (int i = 0; i < 6; ++i) o[43 + i] = g[i];
        for (int i = 0; i < 6; ++i) o[49 + i] = xi[i];
        o[55] = 0.0;
        for (int i = TK_NACC; i < NACC; ++i) o[56 + i - TK_NACC] = tot[i];
    }
    st->rows = row + 1;
    st->iters[level] += 1;
    if (status != 0) st->done[level] = status;
}

// Both entry points: HYBRID = false is hv_tsdf_track (color, cprm and cres unused), true is hv_tsdf_track_color.  The depth-only
// call queues exactly the launches it always did, with null colour / intensity operands.
template <bool HYBRID>
int tk_run(const char *fn, hv_volume *v, const void *depth, int32_t depth_dtype, const uint8_t *color, int32_t height, int32_t width,
           const double *intr, const double *T_cw_init, const hv_track_params *prm, const hv_track_color_params *cprm,
           hv_track_result *res, hv_track_color_result *cres, double *trace, int64_t trace_cap, int64_t *trace_rows, int32_t loc) {
    constexpr int NACC = HYBRID ? TK_NACC_COLOR : TK_NACC;
    constexpr int STRIDE = HYBRID ? HV_TRACK_COLOR_TRACE_STRIDE : HV_TRACK_TRACE_STRIDE;
    using State = TkStateT<NACC>;
    HV_REQUIRE(v != nullptr && depth != nullptr && intr != nullptr && T_cw_init != nullptr && prm != nullptr && res != nullptr &&
                   (!HYBRID || color != nullptr),
               HV_ERR_INVALID, "%s: null argument", fn);
    HV_REQUIRE(v->cfg.mode == HV_MODE_TSDF, HV_ERR_MODE, "%s: volume is not in TSDF mode", fn);
    HV_REQUIRE(v->owner_world <= 1, HV_ERR_MODE, "%s: tracking needs the whole volume (owner-sharded: merge or gather first)", fn);
    HV_REQUIRE(depth_dtype == HV_DEPTH_F32 || depth_dtype == HV_DEPTH_U16, HV_ERR_INVALID, "%s: bad depth dtype %d", fn,
               (int)depth_dtype);
    HV_REQUIRE(loc == HV_HOST || loc == HV_DEVICE, HV_ERR_INVALID, "%s: bad loc %d", fn, (int)loc);
    const int nl = prm->n_levels;
    HV_REQUIRE(nl >= 1 && nl <= HV_TRACK_MAX_LEVELS, HV_ERR_INVALID, "%s: need 1 to %d pyramid levels, got %d", fn,
               HV_TRACK_MAX_LEVELS, nl);
    HV_REQUIRE(height > 0 && width > 0 && height <= 65535 && width <= 65535 && (height >> (nl - 1)) >= 1 && (width >> (nl - 1)) >= 1,
               HV_ERR_INVALID, "%s: bad image size %d x %d for %d levels", fn, (int)height, (int)width, nl);
    HV_REQUIRE(std::isfinite(prm->depth_min) && std::isfinite(prm->depth_max) && prm->depth_min >= 0.0 && prm->depth_min < prm->depth_max,
               HV_ERR_INVALID, "%s: bad depth range [%g, %g)", fn, prm->depth_min, prm->depth_max);
    HV_REQUIRE(std::isfinite(intr[0]) && std::isfinite(intr[1]) && std::isfinite(intr[2]) && std::isfinite(intr[3]) && intr[0] != 0.0 &&
                   intr[1] != 0.0 && std::isfinite(prm->weight_threshold) && std::isfinite(prm->depth_scale) && prm->depth_scale != 0.0,
               HV_ERR_INVALID, "%s: bad intrinsics / threshold / scale", fn);
    HV_REQUIRE(std::isfinite(prm->depth_outlier_trunc) && prm->depth_outlier_trunc > 0.0 && std::isfinite(prm->depth_huber_delta) &&
                   prm->depth_huber_delta > 0.0,
               HV_ERR_INVALID, "%s: depth_outlier_trunc and depth_huber_delta must be positive", fn);
    if (HYBRID) {
        HV_REQUIRE(std::isfinite(cprm->intensity_weight) && cprm->intensity_weight >= 0.0, HV_ERR_INVALID,
                   "%s: intensity_weight must be finite and >= 0", fn);
        HV_REQUIRE(std::isfinite(cprm->intensity_huber_delta) && cprm->intensity_huber_delta > 0.0, HV_ERR_INVALID,
                   "%s: intensity_huber_delta must be positive", fn);
    }
    int64_t steps = 0;
    for (int l = 0; l < nl; ++l) {
        HV_REQUIRE(prm->iterations[l] >= 0 && prm->iterations[l] <= 10000, HV_ERR_INVALID, "%s: bad iteration count %d at level %d", fn,
                   (int)prm->iterations[l], l);
        steps += prm->iterations[l];
    }
    HV_REQUIRE(prm->iterations[0] >= 1, HV_ERR_INVALID, "%s: level 0 needs at least one iteration", fn);
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c)
            HV_REQUIRE(std::isfinite(T_cw_init[r * 4 + c]), HV_ERR_INVALID, "%s: T_cw_init is not finite", fn);
    HV_HIP(hipSetDevice(v->device));

    // scratch: [state][slab][trace][per level: source, model depth, model normal, model mask; hybrid: model colour, model
    // record, source intensity]
    size_t off = 0;
    auto take = [&off](size_t bytes) { // -> the offset of the next bytes, every piece 256-byte aligned
        const size_t at = off;
        off += (bytes + 255) & ~(size_t)255;
        return at;
    };
    const size_t o_state = take(sizeof(State));
    const size_t o_slab = take(sizeof(double) * NACC * TK_MAX_BLOCKS);
    const size_t o_trace = take(sizeof(double) * STRIDE * (size_t)steps);
    size_t o_src[HV_TRACK_MAX_LEVELS], o_md[HV_TRACK_MAX_LEVELS], o_mn[HV_TRACK_MAX_LEVELS], o_mm[HV_TRACK_MAX_LEVELS];
    size_t o_mc[HV_TRACK_MAX_LEVELS] = {}, o_rec[HV_TRACK_MAX_LEVELS] = {}, o_int[HV_TRACK_MAX_LEVELS] = {};
    for (int l = 0; l < nl; ++l) {
        const size_t n = (size_t)(height >> l) * (size_t)(width >> l);
        o_src[l] = take(4 * n);
        o_md[l] = take(4 * n);
        o_mn[l] = take(12 * n);
        o_mm[l] = take(n);
        if (HYBRID) {
            o_mc[l] = take(12 * n);
            o_rec[l] = take(16 * n);
            o_int[l] = take(4 * n);
        }
    }
    int rc = hv_ensure_buffer(v, &v->track_buf, &v->track_buf_bytes, off);
    if (rc != HV_OK) return rc;
    char *base = (char *)v->track_buf;
    // the source intensity of a level; null in the depth-only call, whose kernels do not read it
    auto intensity = [&](int l) { return HYBRID ? (float *)(base + o_int[l]) : (float *)nullptr; };
    State *st = (State *)(base + o_state);
    double *slab = (double *)(base + o_slab);
    double *d_trace = (double *)(base + o_trace);

    const void *d_depth = nullptr;
    const uint8_t *d_color = nullptr;
    const size_t npx0 = (size_t)height * (size_t)width;
    rc = hv_stage_frame(v, depth, depth_dtype, HYBRID ? color : nullptr, npx0, loc, &d_depth, &d_color);
    if (rc != HV_OK) return rc;
    // reads only, as hv_tsdf_ray_cast: the next batch starts a fresh touch + pack chain behind this call
    v->pipe_armed = false;

    hipLaunchKernelGGL(k_track_init<NACC>, dim3(1), dim3(64), 0, v->stream, st);
    hv_profile_begin(v);
    hipLaunchKernelGGL(k_track_source<HYBRID>, dim3((unsigned)((npx0 + 255) / 256)), dim3(256), 0, v->stream, d_depth,
                       depth_dtype == HV_DEPTH_U16 ? 1 : 0, d_color, v->color_bgr, (int64_t)npx0, (float)prm->depth_scale,
                       prm->depth_min, prm->depth_max, (float *)(base + o_src[0]), intensity(0));
    hv_profile_end(v, 0);
    for (int l = 1; l < nl; ++l) {
        const int ho = height >> l, wo = width >> l;
        hv_profile_begin(v);
        hipLaunchKernelGGL(k_track_down<HYBRID>, dim3((unsigned)(((size_t)ho * wo + 255) / 256)), dim3(256), 0, v->stream,
                           (const float *)(base + o_src[l - 1]), (const float *)intensity(l - 1), width >> (l - 1),
                           (float *)(base + o_src[l]), intensity(l), ho, wo, prm->depth_outlier_trunc);
        hv_profile_end(v, 0);
    }
    HV_HIP(hipGetLastError());

    TkLevel lv[HV_TRACK_MAX_LEVELS];
    for (int l = 0; l < nl; ++l) {
        const double s = (double)(1 << l);
        const double li[4] = {intr[0] / s, intr[1] / s, (intr[2] + 0.5) / s - 0.5, (intr[3] + 0.5) / s - 0.5};
        lv[l] = TkLevel{(const float *)(base + o_src[l]), (const float *)(base + o_md[l]), (const float *)(base + o_mn[l]),
                        (const uint8_t *)(base + o_mm[l]), height >> l, width >> l, li[0], li[1], li[2], li[3]};
        if (prm->iterations[l] == 0) continue;
        rc = hv_ray_cast_launch(v, height >> l, width >> l, li, T_cw_init, prm->depth_min, prm->depth_max, prm->weight_threshold, 1.0,
                                (float *)(base + o_md[l]), nullptr, (float *)(base + o_mn[l]),
                                HYBRID ? (float *)(base + o_mc[l]) : (float *)nullptr, (uint8_t *)(base + o_mm[l]));
        if (rc != HV_OK) return rc;
        if (HYBRID) {
            const size_t n = (size_t)lv[l].height * (size_t)lv[l].width;
            hv_profile_begin(v);
            hipLaunchKernelGGL(k_track_model_prep, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, v->stream,
                               (const float *)(base + o_mc[l]), (const float *)(base + o_md[l]), (const uint8_t *)(base + o_mm[l]),
                               lv[l].height, lv[l].width, prm->depth_outlier_trunc, (float4 *)(base + o_rec[l]));
            hv_profile_end(v, 0);
        }
    }

    TkParams P{};
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) P.R0[r * 3 + c] = T_cw_init[r * 4 + c];
    P.trunc = prm->depth_outlier_trunc;
    P.delta = prm->depth_huber_delta;
    for (int l = nl - 1; l >= 0; --l) {
        const int64_t npx = (int64_t)lv[l].height * lv[l].width;
        const int blocks = (int)std::min<int64_t>((npx + TK_BLOCK - 1) / TK_BLOCK, TK_MAX_BLOCKS);
        TkColor C{}; // depth only: zero, and not read
        if constexpr (HYBRID) C = TkColor{(const float4 *)(base + o_rec[l]), intensity(l), cprm->intensity_weight, cprm->intensity_huber_delta};
        for (int it = 0; it < prm->iterations[l]; ++it) {
            hv_profile_begin(v);
            hipLaunchKernelGGL(k_track_linearise<NACC>, dim3((unsigned)blocks), dim3(TK_BLOCK), 0, v->stream, lv[l], P, C,
                               (const State *)st, l, slab);
            hv_profile_end(v, 0);
            hv_profile_begin(v);
            hipLaunchKernelGGL((k_track_solve<NACC, STRIDE>), dim3(1), dim3(TK_SUM_THREADS), 0, v->stream, st, (const double *)slab, blocks, l, it,
                               trace ? d_trace : (double *)nullptr, (int)steps);
            hv_profile_end(v, 0);
        }
    }
    HV_HIP(hipGetLastError());

    State h{};
    HV_HIP(hipMemcpyAsync(&h, st, sizeof(State), hipMemcpyDeviceToHost, v->stream));
    HV_HIP(hipStreamSynchronize(v->stream));
    if (trace != nullptr) {
        const int64_t n = std::min<int64_t>(h.rows, trace_cap);
        if (n > 0) HV_HIP(hipMemcpy(trace, d_trace, sizeof(double) * STRIDE * (size_t)n, hipMemcpyDeviceToHost));
        if (trace_rows) *trace_rows = n;
    } else if (trace_rows) {
        *trace_rows = 0;
    }

    // T_cw = inverse(A) T_cw_init, A rigid: inverse(A) = [R^T, -R^T t]
    double Ai[16] = {};
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) Ai[r * 4 + c] = h.A[c * 4 + r];
        Ai[r * 4 + 3] = -(h.A[r] * h.A[3] + h.A[4 + r] * h.A[7] + h.A[8 + r] * h.A[11]);
    }
    Ai[15] = 1.0;
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c)
            res->T_cw[r * 4 + c] = Ai[r * 4] * T_cw_init[c] + Ai[r * 4 + 1] * T_cw_init[4 + c] + Ai[r * 4 + 2] * T_cw_init[8 + c] +
                                   Ai[r * 4 + 3] * T_cw_init[12 + c];
    {
        int q = 0;
        for (int a = 0; a < 6; ++a)
            for (int b = a; b < 6; ++b) {
                res->information[a * 6 + b] = res->information[b * 6 + a] = h.last[q++];
            }
    }
    const double e = h.last[27], inl = h.last[28], val = h.last[29];
    res->inliers = (int64_t)inl;
    res->valid = (int64_t)val;
    res->fitness = val > 0.0 ? inl / val : 0.0;
    res->inlier_rmse = inl > 0.0 ? std::sqrt(e / inl) : 0.0;
    res->degenerate = 0;
    for (int l = 0; l < HV_TRACK_MAX_LEVELS; ++l) {
        res->iterations[l] = l < nl ? h.iters[l] : 0;
        if (l < nl && h.done[l] == 2) res->degenerate |= 1 << l;
    }
    res->success = (h.done[0] != 2 && inl >= (double)HV_TRACK_MIN_INLIERS) ? 1 : 0;
    if constexpr (HYBRID) {
        const double pin = h.last[30], pe = h.last[31];
        cres->photometric_inliers = (int64_t)pin;
        cres->intensity_rmse = pin > 0.0 ? std::sqrt(pe / pin) : 0.0;
    }
    return HV_OK;
}

} // namespace

extern "C" int hv_tsdf_track(hv_volume *v, const void *depth, int32_t depth_dtype, int32_t height, int32_t width, const double *intr,
                             const double *T_cw_init, const hv_track_params *prm, hv_track_result *res, double *trace, int64_t trace_cap,
                             int64_t *trace_rows, int32_t loc) {
    return tk_run<false>("hv_tsdf_track", v, depth, depth_dtype, nullptr, height, width, intr, T_cw_init, prm, nullptr, res, nullptr, trace,
                         trace_cap, trace_rows, loc);
}

extern "C" int hv_tsdf_track_color(hv_volume *v, const void *depth, int32_t depth_dtype, const uint8_t *color, int32_t height,
                                   int32_t width, const double *intr, const double *T_cw_init, const hv_track_color_params *prm,
                                   hv_track_color_result *res, double *trace, int64_t trace_cap, int64_t *trace_rows, int32_t loc) {
    HV_REQUIRE(prm != nullptr && res != nullptr, HV_ERR_INVALID, "hv_tsdf_track_color: null argument");
    return tk_run<true>("hv_tsdf_track_color", v, depth, depth_dtype, color, height, width, intr, T_cw_init, &prm->base, prm, &res->base,
                        res, trace, trace_cap, trace_rows, loc);
}
