// libpyslam_hipvol.so — frame-to-model tracking against the fused TSDF map on gfx950: point-to-plane (hv_tsdf_track) and hybrid,
// point-to-plane plus a photometric term on the map's colour (hv_tsdf_track_color); and the same schedule against a second RGB-D
// frame instead of the map, frame-to-frame odometry (hv_rgbd_odometry, last paragraph).  The contracts (pyramid, model,
// association, linearisation, solve, stopping, outputs) are written once in include/hipvol.h; tests/track_reference.py and
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
//
// Frame-to-frame odometry is tk_run with another model provider: where the tracker queues a ray cast (and k_track_model_prep) per
// level, TkFrameModel queues the target frame's pyramid (the source pyramid's two kernels) and one k_odometry_model launch per level,
// which turns the level's depth (and intensity) into normal, mask (and record); the state starts at T_init, the normals need no
// rotation (R0 = identity), and the result pose is the state A itself.  tests/odometry_reference.py restates it.
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
    const float *mdepth;     // model depth (the map cast at T_cw_init, or the target frame)
    const float *mnormal;    // model normal [H,W,3]: world frame (cast) or anchor frame already (target frame, R0 = identity)
    const uint8_t *mmask;    // model mask
    int32_t height, width;
    double fx, fy, cx, cy;
};

struct TkParams {
    double R0[9];  // model normal -> anchor frame: R_cw_init for the cast's world normals, the identity for a target frame's
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

// frame-to-frame: the state of k_track_init with A = A0 (T_init) instead of the identity
struct TkPose {
    double m[16];
};
template <int NACC>
__global__ __launch_bounds__(64) void k_track_init_at(TkStateT<NACC> *st, TkPose A0) {
    const int t = threadIdx.x;
    if (t < 16) st->A[t] = A0.m[t];
    if (t < NACC) st->last[t] = 0.0;
    if (t < HV_TRACK_MAX_LEVELS) {
        st->done[t] = 0;
        st->iters[t] = 0;
    }
    if (t == 0) st->rows = 0;
}

// frame-to-frame, per level: the target frame's depth z (and intensity it) of the level -> the model the linearisation reads: normal
// and mask, HYBRID also the record {I_t, g_x, g_y, has-gradient}.  One thread per target pixel, a 5-point stencil on plain loads
// (a row's neighbours are the same cache lines, the rows above and below were just read by the neighbouring workgroups).
// mask = 1 iff the pixel is off the border, z > 0 at it and its four neighbours, no neighbour's depth is further than trunc from its
// own (double), and c = dy x dx of the back-projected central differences has a finite length > 0; normal = c / |c|, turned to face
// the camera, rounded to float32; 0 where mask = 0.  All geometry in double, one IEEE operation per step (tests/odometry_reference.py
// restates it bit for bit).
template <bool HYBRID>
__global__ __launch_bounds__(256) void k_odometry_model(const float *__restrict__ z, const float *__restrict__ it, int32_t height, int32_t width,
                                                        double fx, double fy, double cx, double cy, double trunc, float *__restrict__ normal,
                                                        uint8_t *__restrict__ mask, float4 *__restrict__ rec) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)height * width) return;
    const int u = (int)(i % width), v = (int)(i / width);
    float n[3] = {0.0f, 0.0f, 0.0f};
    bool ok = false;
    const bool inner = u >= 1 && v >= 1 && u + 1 < width && v + 1 < height;
    const int64_t nb[4] = {i + 1, i - 1, i + width, i - width}; // (read only when inner)
    if (inner) {
        const float zc = z[i];
        const float zn[4] = {z[nb[0]], z[nb[1]], z[nb[2]], z[nb[3]]};
        ok = zc > 0.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k) ok = ok && zn[k] > 0.0f && fabs((double)zn[k] - (double)zc) <= trunc;
        if (ok) {
            const double xm = ((double)(u - 1) - cx) / fx, x0 = ((double)u - cx) / fx, xp = ((double)(u + 1) - cx) / fx;
            const double ym = ((double)(v - 1) - cy) / fy, y0 = ((double)v - cy) / fy, yp = ((double)(v + 1) - cy) / fy;
            const double zr = (double)zn[0], zl = (double)zn[1], zd = (double)zn[2], zu = (double)zn[3], zz = (double)zc;
            const double dx[3] = {zr * xp - zl * xm, zr * y0 - zl * y0, zr - zl};
            const double dy[3] = {zd * x0 - zu * x0, zd * yp - zu * ym, zd - zu};
            const double c[3] = {dy[1] * dx[2] - dy[2] * dx[1], dy[2] * dx[0] - dy[0] * dx[2], dy[0] * dx[1] - dy[1] * dx[0]};
            const double len = sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
            ok = isfinite(len) && len > 0.0;
            if (ok) {
                double m[3] = {c[0] / len, c[1] / len, c[2] / len};
                const bool away = (m[0] * (zz * x0) + m[1] * (zz * y0)) + m[2] * zz > 0.0;
#pragma unroll
                for (int k = 0; k < 3; ++k) n[k] = (float)(away ? -m[k] : m[k]);
            }
        }
    }
    normal[3 * i] = n[0];
    normal[3 * i + 1] = n[1];
    normal[3 * i + 2] = n[2];
    mask[i] = ok ? 1 : 0;
    if constexpr (HYBRID) {
        float4 o = make_float4(it[i], 0.0f, 0.0f, 0.0f);
        if (ok) {
            o.y = 0.5f * (it[nb[0]] - it[nb[1]]);
            o.z = 0.5f * (it[nb[2]] - it[nb[3]]);
            o.w = 1.0f;
        }
        rec[i] = o;
    }
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

// ---- the schedule, once (tk_run), and the two things a kind of call supplies to it ------------------------------------------------
// What every call shares: the schedule's numbers, checked by tk_run before any launch.
struct TkSchedule {
    double depth_scale, depth_min, depth_max, trunc, delta;
    double lambda, idelta;  // hybrid only
    int32_t n_levels;
    const int32_t *iterations;
};

// One level's model maps in the call's scratch, as tk_run hands them to the provider that fills them.
struct TkModelMaps {
    float *depth, *normal;
    uint8_t *mask;
    float *aux;   // hybrid: the provider's own plane of AUX_BYTES per pixel (cast colour / target intensity)
    float4 *rec;  // hybrid: {I_m, g_x, g_y, has-gradient}
    int32_t height, width;
    double K[4];
};

// What tk_run leaves behind: the final state and the outputs of the last level-0 linearisation.  The caller forms its pose from A.
struct TkOutcome {
    double A[16];
    double information[36];
    double fitness, inlier_rmse, intensity_rmse;
    int64_t inliers, valid, photometric_inliers;
    int32_t iterations[HV_TRACK_MAX_LEVELS];
    int32_t degenerate, success;
    bool level0_started;  // a level-0 linearisation left the level running (false: A holds coarser levels' steps at most)
};

template <class Result>
void tk_copy_result(const TkOutcome &o, Result *res) {
    for (int i = 0; i < 36; ++i) res->information[i] = o.information[i];
    res->fitness = o.fitness;
    res->inlier_rmse = o.inlier_rmse;
    res->inliers = o.inliers;
    res->valid = o.valid;
    for (int l = 0; l < HV_TRACK_MAX_LEVELS; ++l) res->iterations[l] = o.iterations[l];
    res->degenerate = o.degenerate;
    res->success = o.success;
}

// A model provider says where the per-level model comes from.  tk_run calls, in this order: check() (before any launch), stage()
// (the call's frames -> device pointers of the SOURCE frame), start() (queues the state's initialisation), after the source pyramid
// prepare() (what the levels' models need first) and per level with iterations level() (queues the model of that level into its
// maps); R0() is the rotation the linearisation applies to the model's normals.

// Frame-to-model: the map cast at T_cw_init, hybrid also k_track_model_prep on the cast's colour (hv_tsdf_track[_color]).
struct TkMapModel {
    static constexpr size_t AUX_BYTES = 12;  // the cast's colour
    hv_volume *v;
    const char *fn;
    const void *depth;
    int32_t depth_dtype;
    const uint8_t *color;
    const double *T0;
    double depth_min, depth_max, weight_threshold, trunc;

    int check() const {
        HV_REQUIRE(v->cfg.mode == HV_MODE_TSDF, HV_ERR_MODE, "%s: volume is not in TSDF mode", fn);
        HV_REQUIRE(v->owner_world <= 1, HV_ERR_MODE, "%s: tracking needs the whole volume (owner-sharded: merge or gather first)", fn);
        HV_REQUIRE(std::isfinite(weight_threshold), HV_ERR_INVALID, "%s: bad intrinsics / threshold / scale", fn);
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) HV_REQUIRE(std::isfinite(T0[r * 4 + c]), HV_ERR_INVALID, "%s: T_cw_init is not finite", fn);
        return HV_OK;
    }
    int stage(size_t npx, int32_t loc, const void **d_depth, const uint8_t **d_color) {
        return hv_stage_frame(v, depth, depth_dtype, color, npx, loc, d_depth, d_color);
    }
    template <int NACC>
    void start(TkStateT<NACC> *st) const {
        hipLaunchKernelGGL(k_track_init<NACC>, dim3(1), dim3(64), 0, v->stream, st);
    }
    template <bool HYBRID>
    int prepare(const TkModelMaps *, int) const {
        return HV_OK;
    }
    template <bool HYBRID>
    int level(const TkModelMaps &m) const {
        const int rc = hv_ray_cast_launch(v, m.height, m.width, m.K, T0, depth_min, depth_max, weight_threshold, 1.0, m.depth, nullptr, m.normal,
                                          HYBRID ? m.aux : (float *)nullptr, m.mask);
        if (rc != HV_OK) return rc;
        if (HYBRID) {
            const size_t n = (size_t)m.height * (size_t)m.width;
            hv_profile_begin(v);
            hipLaunchKernelGGL(k_track_model_prep, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, v->stream, (const float *)m.aux,
                               (const float *)m.depth, (const uint8_t *)m.mask, m.height, m.width, trunc, m.rec);
            hv_profile_end(v, 0);
        }
        return HV_OK;
    }
    void R0(double *R) const {
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) R[r * 3 + c] = T0[r * 4 + c];
    }
};

// Frame-to-frame: the model is a second RGB-D frame (hv_rgbd_odometry): its pyramid through the source's two kernels straight into
// the levels' model depth (and, hybrid, the aux plane = target intensity), then k_odometry_model per level.
struct TkFrameModel {
    static constexpr size_t AUX_BYTES = 4;  // the target intensity of the level
    hv_volume *v;
    const char *fn;
    const void *source_depth, *target_depth;
    int32_t depth_dtype;
    const uint8_t *source_color, *target_color;
    double T0[16];
    double depth_scale, depth_min, depth_max, trunc;
    const void *d_target_depth = nullptr;
    const uint8_t *d_target_color = nullptr;

    int check() const {
        for (int i = 0; i < 16; ++i) HV_REQUIRE(std::isfinite(T0[i]), HV_ERR_INVALID, "%s: T_init is not finite", fn);
        HV_REQUIRE(T0[12] == 0.0 && T0[13] == 0.0 && T0[14] == 0.0 && T0[15] == 1.0, HV_ERR_INVALID, "%s: T_init's bottom row must be 0 0 0 1", fn);
        return HV_OK;
    }
    int stage(size_t npx, int32_t loc, const void **d_depth, const uint8_t **d_color) {
        HvStage st(v, loc);
        const size_t depth_bytes = npx * (depth_dtype == HV_DEPTH_U16 ? 2 : 4);
        const int i_sd = st.in(source_depth, depth_bytes), i_td = st.in(target_depth, depth_bytes);
        const int i_sc = st.in(source_color, npx * 3), i_tc = st.in(target_color, npx * 3);
        const int rc = st.commit(&v->stage, &v->stage_bytes);
        *d_depth = st.dev<const void>(i_sd);
        *d_color = st.dev<const uint8_t>(i_sc);
        d_target_depth = st.dev<const void>(i_td);
        d_target_color = st.dev<const uint8_t>(i_tc);
        return rc;
    }
    template <int NACC>
    void start(TkStateT<NACC> *st) const {
        TkPose A0;
        for (int i = 0; i < 16; ++i) A0.m[i] = T0[i];
        hipLaunchKernelGGL(k_track_init_at<NACC>, dim3(1), dim3(64), 0, v->stream, st, A0);
    }
    // the target pyramid, levels 0 .. nl - 1 (maps[l].depth, hybrid maps[l].aux)
    template <bool HYBRID>
    int prepare(const TkModelMaps *maps, int nl) const {
        const size_t npx0 = (size_t)maps[0].height * (size_t)maps[0].width;
        hv_profile_begin(v);
        hipLaunchKernelGGL(k_track_source<HYBRID>, dim3((unsigned)((npx0 + 255) / 256)), dim3(256), 0, v->stream, d_target_depth,
                           depth_dtype == HV_DEPTH_U16 ? 1 : 0, d_target_color, v->color_bgr, (int64_t)npx0, (float)depth_scale, depth_min,
                           depth_max, maps[0].depth, HYBRID ? maps[0].aux : (float *)nullptr);
        hv_profile_end(v, 0);
        for (int l = 1; l < nl; ++l) {
            const size_t n = (size_t)maps[l].height * (size_t)maps[l].width;
            hv_profile_begin(v);
            hipLaunchKernelGGL(k_track_down<HYBRID>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, v->stream, (const float *)maps[l - 1].depth,
                               HYBRID ? (const float *)maps[l - 1].aux : (const float *)nullptr, maps[l - 1].width, maps[l].depth,
                               HYBRID ? maps[l].aux : (float *)nullptr, maps[l].height, maps[l].width, trunc);
            hv_profile_end(v, 0);
        }
        HV_HIP(hipGetLastError());
        return HV_OK;
    }
    template <bool HYBRID>
    int level(const TkModelMaps &m) const {
        const size_t n = (size_t)m.height * (size_t)m.width;
        hv_profile_begin(v);
        hipLaunchKernelGGL(k_odometry_model<HYBRID>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, v->stream, (const float *)m.depth,
                           HYBRID ? (const float *)m.aux : (const float *)nullptr, m.height, m.width, m.K[0], m.K[1], m.K[2], m.K[3], trunc,
                           m.normal, m.mask, HYBRID ? m.rec : (float4 *)nullptr);
        hv_profile_end(v, (int64_t)n);
        return HV_OK;
    }
    void R0(double *R) const {
        for (int i = 0; i < 9; ++i) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
    }
};

// What hv_tsdf_track states for sizes, depth range, intrinsics, scale, thresholds and iterations, for every kind of call
int tk_check_schedule(const char *fn, const TkSchedule &S, bool hybrid, int32_t height, int32_t width, const double *intr, int64_t *steps) {
    const int nl = S.n_levels;
    HV_REQUIRE(nl >= 1 && nl <= HV_TRACK_MAX_LEVELS, HV_ERR_INVALID, "%s: need 1 to %d pyramid levels, got %d", fn, HV_TRACK_MAX_LEVELS, nl);
    HV_REQUIRE(height > 0 && width > 0 && height <= 65535 && width <= 65535 && (height >> (nl - 1)) >= 1 && (width >> (nl - 1)) >= 1,
               HV_ERR_INVALID, "%s: bad image size %d x %d for %d levels", fn, (int)height, (int)width, nl);
    HV_REQUIRE(std::isfinite(S.depth_min) && std::isfinite(S.depth_max) && S.depth_min >= 0.0 && S.depth_min < S.depth_max, HV_ERR_INVALID,
               "%s: bad depth range [%g, %g)", fn, S.depth_min, S.depth_max);
    HV_REQUIRE(std::isfinite(intr[0]) && std::isfinite(intr[1]) && std::isfinite(intr[2]) && std::isfinite(intr[3]) && intr[0] != 0.0 &&
                   intr[1] != 0.0 && std::isfinite(S.depth_scale) && S.depth_scale != 0.0,
               HV_ERR_INVALID, "%s: bad intrinsics / threshold / scale", fn);
    HV_REQUIRE(std::isfinite(S.trunc) && S.trunc > 0.0 && std::isfinite(S.delta) && S.delta > 0.0, HV_ERR_INVALID,
               "%s: depth_outlier_trunc and depth_huber_delta must be positive", fn);
    if (hybrid) {
        HV_REQUIRE(std::isfinite(S.lambda) && S.lambda >= 0.0, HV_ERR_INVALID, "%s: intensity_weight must be finite and >= 0", fn);
        HV_REQUIRE(std::isfinite(S.idelta) && S.idelta > 0.0, HV_ERR_INVALID, "%s: intensity_huber_delta must be positive", fn);
    }
    *steps = 0;
    for (int l = 0; l < nl; ++l) {
        HV_REQUIRE(S.iterations[l] >= 0 && S.iterations[l] <= 10000, HV_ERR_INVALID, "%s: bad iteration count %d at level %d", fn,
                   (int)S.iterations[l], l);
        *steps += S.iterations[l];
    }
    HV_REQUIRE(S.iterations[0] >= 1, HV_ERR_INVALID, "%s: level 0 needs at least one iteration", fn);
    return HV_OK;
}

// Every entry point: state init, source pyramid, per-level model (the provider's), the linearise / solve steps, fetch, outcome.
// HYBRID = false is the depth-only call (30 sums; colour operands null and not read), true the hybrid one (32 sums).  With
// TkMapModel it queues exactly the launches hv_tsdf_track / hv_tsdf_track_color always queued.
template <bool HYBRID, class Model>
int tk_run(const char *fn, hv_volume *v, Model &model, const TkSchedule &S, int32_t depth_dtype, int32_t height, int32_t width,
           const double *intr, TkOutcome *out, double *trace, int64_t trace_cap, int64_t *trace_rows, int32_t loc) {
    constexpr int NACC = HYBRID ? TK_NACC_COLOR : TK_NACC;
    constexpr int STRIDE = HYBRID ? HV_TRACK_COLOR_TRACE_STRIDE : HV_TRACK_TRACE_STRIDE;
    using State = TkStateT<NACC>;
    HV_REQUIRE(depth_dtype == HV_DEPTH_F32 || depth_dtype == HV_DEPTH_U16, HV_ERR_INVALID, "%s: bad depth dtype %d", fn, (int)depth_dtype);
    HV_REQUIRE(loc == HV_HOST || loc == HV_DEVICE, HV_ERR_INVALID, "%s: bad loc %d", fn, (int)loc);
    int rc = model.check();
    if (rc != HV_OK) return rc;
    int64_t steps = 0;
    rc = tk_check_schedule(fn, S, HYBRID, height, width, intr, &steps);
    if (rc != HV_OK) return rc;
    const int nl = S.n_levels;
    HV_HIP(hipSetDevice(v->device));

    // scratch: [state][slab][trace][per level: source, model depth, model normal, model mask; hybrid: the provider's plane, model
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
    size_t o_aux[HV_TRACK_MAX_LEVELS] = {}, o_rec[HV_TRACK_MAX_LEVELS] = {}, o_int[HV_TRACK_MAX_LEVELS] = {};
    for (int l = 0; l < nl; ++l) {
        const size_t n = (size_t)(height >> l) * (size_t)(width >> l);
        o_src[l] = take(4 * n);
        o_md[l] = take(4 * n);
        o_mn[l] = take(12 * n);
        o_mm[l] = take(n);
        if (HYBRID) {
            o_aux[l] = take(Model::AUX_BYTES * n);
            o_rec[l] = take(16 * n);
            o_int[l] = take(4 * n);
        }
    }
    rc = hv_ensure_buffer(v, &v->track_buf, &v->track_buf_bytes, off);
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
    rc = model.stage(npx0, loc, &d_depth, &d_color);
    if (rc != HV_OK) return rc;
    // reads only, as hv_tsdf_ray_cast: the next batch starts a fresh touch + pack chain behind this call
    v->pipe_armed = false;

    model.template start<NACC>(st);
    hv_profile_begin(v);
    hipLaunchKernelGGL(k_track_source<HYBRID>, dim3((unsigned)((npx0 + 255) / 256)), dim3(256), 0, v->stream, d_depth,
                       depth_dtype == HV_DEPTH_U16 ? 1 : 0, d_color, v->color_bgr, (int64_t)npx0, (float)S.depth_scale, S.depth_min,
                       S.depth_max, (float *)(base + o_src[0]), intensity(0));
    hv_profile_end(v, 0);
    for (int l = 1; l < nl; ++l) {
        const int ho = height >> l, wo = width >> l;
        hv_profile_begin(v);
        hipLaunchKernelGGL(k_track_down<HYBRID>, dim3((unsigned)(((size_t)ho * wo + 255) / 256)), dim3(256), 0, v->stream,
                           (const float *)(base + o_src[l - 1]), (const float *)intensity(l - 1), width >> (l - 1),
                           (float *)(base + o_src[l]), intensity(l), ho, wo, S.trunc);
        hv_profile_end(v, 0);
    }
    HV_HIP(hipGetLastError());

    TkLevel lv[HV_TRACK_MAX_LEVELS];
    TkModelMaps maps[HV_TRACK_MAX_LEVELS];
    for (int l = 0; l < nl; ++l) {
        const double s = (double)(1 << l);
        maps[l] = TkModelMaps{(float *)(base + o_md[l]), (float *)(base + o_mn[l]), (uint8_t *)(base + o_mm[l]),
                              HYBRID ? (float *)(base + o_aux[l]) : (float *)nullptr, HYBRID ? (float4 *)(base + o_rec[l]) : (float4 *)nullptr,
                              height >> l, width >> l, {intr[0] / s, intr[1] / s, (intr[2] + 0.5) / s - 0.5, (intr[3] + 0.5) / s - 0.5}};
        lv[l] = TkLevel{(const float *)(base + o_src[l]), maps[l].depth, maps[l].normal, maps[l].mask, height >> l, width >> l,
                        maps[l].K[0], maps[l].K[1], maps[l].K[2], maps[l].K[3]};
    }
    rc = model.template prepare<HYBRID>(maps, nl);
    if (rc != HV_OK) return rc;
    for (int l = 0; l < nl; ++l) {
        if (S.iterations[l] == 0) continue;
        rc = model.template level<HYBRID>(maps[l]);
        if (rc != HV_OK) return rc;
    }

    TkParams P{};
    model.R0(P.R0);
    P.trunc = S.trunc;
    P.delta = S.delta;
    for (int l = nl - 1; l >= 0; --l) {
        const int64_t npx = (int64_t)lv[l].height * lv[l].width;
        const int blocks = (int)std::min<int64_t>((npx + TK_BLOCK - 1) / TK_BLOCK, TK_MAX_BLOCKS);
        TkColor C{}; // depth only: zero, and not read
        if constexpr (HYBRID) C = TkColor{(const float4 *)maps[l].rec, intensity(l), S.lambda, S.idelta};
        for (int it = 0; it < S.iterations[l]; ++it) {
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

    for (int i = 0; i < 16; ++i) out->A[i] = h.A[i];
    {
        int q = 0;
        for (int a = 0; a < 6; ++a)
            for (int b = a; b < 6; ++b) {
                out->information[a * 6 + b] = out->information[b * 6 + a] = h.last[q++];
            }
    }
    const double e = h.last[27], inl = h.last[28], val = h.last[29];
    out->inliers = (int64_t)inl;
    out->valid = (int64_t)val;
    out->fitness = val > 0.0 ? inl / val : 0.0;
    out->inlier_rmse = inl > 0.0 ? std::sqrt(e / inl) : 0.0;
    out->degenerate = 0;
    for (int l = 0; l < HV_TRACK_MAX_LEVELS; ++l) {
        out->iterations[l] = l < nl ? h.iters[l] : 0;
        if (l < nl && h.done[l] == 2) out->degenerate |= 1 << l;
    }
    out->success = (h.done[0] != 2 && inl >= (double)HV_TRACK_MIN_INLIERS) ? 1 : 0;
    out->level0_started = !(h.done[0] == 2 && h.iters[0] <= 1);
    out->photometric_inliers = 0;
    out->intensity_rmse = 0.0;
    if constexpr (HYBRID) {
        const double pin = h.last[30], pe = h.last[31];
        out->photometric_inliers = (int64_t)pin;
        out->intensity_rmse = pin > 0.0 ? std::sqrt(pe / pin) : 0.0;
    }
    return HV_OK;
}

// hv_tsdf_track / hv_tsdf_track_color: the map as the model, T_cw = inverse(A) T_cw_init
template <bool HYBRID>
int tk_track(const char *fn, hv_volume *v, const void *depth, int32_t depth_dtype, const uint8_t *color, int32_t height, int32_t width,
             const double *intr, const double *T_cw_init, const hv_track_params *prm, const hv_track_color_params *cprm,
             hv_track_result *res, hv_track_color_result *cres, double *trace, int64_t trace_cap, int64_t *trace_rows, int32_t loc) {
    HV_REQUIRE(v != nullptr && depth != nullptr && intr != nullptr && T_cw_init != nullptr && prm != nullptr && res != nullptr &&
                   (!HYBRID || color != nullptr),
               HV_ERR_INVALID, "%s: null argument", fn);
    TkMapModel model{v, fn, depth, depth_dtype, HYBRID ? color : nullptr, T_cw_init, prm->depth_min, prm->depth_max, prm->weight_threshold,
                     prm->depth_outlier_trunc};
    const TkSchedule S{prm->depth_scale, prm->depth_min, prm->depth_max, prm->depth_outlier_trunc, prm->depth_huber_delta,
                       HYBRID ? cprm->intensity_weight : 0.0, HYBRID ? cprm->intensity_huber_delta : 0.0, prm->n_levels, prm->iterations};
    TkOutcome o{};
    const int rc = tk_run<HYBRID>(fn, v, model, S, depth_dtype, height, width, intr, &o, trace, trace_cap, trace_rows, loc);
    if (rc != HV_OK) return rc;
    // T_cw = inverse(A) T_cw_init, A rigid: inverse(A) = [R^T, -R^T t]
    double Ai[16] = {};
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) Ai[r * 4 + c] = o.A[c * 4 + r];
        Ai[r * 4 + 3] = -(o.A[r] * o.A[3] + o.A[4 + r] * o.A[7] + o.A[8 + r] * o.A[11]);
    }
    Ai[15] = 1.0;
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c)
            res->T_cw[r * 4 + c] = Ai[r * 4] * T_cw_init[c] + Ai[r * 4 + 1] * T_cw_init[4 + c] + Ai[r * 4 + 2] * T_cw_init[8 + c] +
                                   Ai[r * 4 + 3] * T_cw_init[12 + c];
    tk_copy_result(o, res);
    if constexpr (HYBRID) {
        cres->photometric_inliers = o.photometric_inliers;
        cres->intensity_rmse = o.intensity_rmse;
    }
    return HV_OK;
}

// the provider of the two odometry entry points (T_init null: the identity)
TkFrameModel od_frame_model(const char *fn, hv_volume *v, const void *source_depth, const void *target_depth, int32_t depth_dtype,
                            const uint8_t *source_color, const uint8_t *target_color, const double *T_init, const hv_odometry_params *prm) {
    TkFrameModel model{v, fn, source_depth, target_depth, depth_dtype, source_color, target_color, {}, prm->depth_scale, prm->depth_min,
                       prm->depth_max, prm->depth_outlier_trunc};
    for (int i = 0; i < 16; ++i) model.T0[i] = T_init != nullptr ? T_init[i] : ((i % 5 == 0) ? 1.0 : 0.0);
    return model;
}

} // namespace

extern "C" int hv_tsdf_track(hv_volume *v, const void *depth, int32_t depth_dtype, int32_t height, int32_t width, const double *intr,
                             const double *T_cw_init, const hv_track_params *prm, hv_track_result *res, double *trace, int64_t trace_cap,
                             int64_t *trace_rows, int32_t loc) {
    return tk_track<false>("hv_tsdf_track", v, depth, depth_dtype, nullptr, height, width, intr, T_cw_init, prm, nullptr, res, nullptr, trace,
                           trace_cap, trace_rows, loc);
}

extern "C" int hv_tsdf_track_color(hv_volume *v, const void *depth, int32_t depth_dtype, const uint8_t *color, int32_t height,
                                   int32_t width, const double *intr, const double *T_cw_init, const hv_track_color_params *prm,
                                   hv_track_color_result *res, double *trace, int64_t trace_cap, int64_t *trace_rows, int32_t loc) {
    HV_REQUIRE(prm != nullptr && res != nullptr, HV_ERR_INVALID, "hv_tsdf_track_color: null argument");
    return tk_track<true>("hv_tsdf_track_color", v, depth, depth_dtype, color, height, width, intr, T_cw_init, &prm->base, prm, &res->base,
                          res, trace, trace_cap, trace_rows, loc);
}

extern "C" int hv_rgbd_odometry(hv_volume *v, const void *source_depth, const void *target_depth, int32_t depth_dtype,
                                const uint8_t *source_color, const uint8_t *target_color, int32_t height, int32_t width, const double *intr,
                                const double *T_init, const hv_odometry_params *prm, hv_odometry_result *res, double *trace,
                                int64_t trace_cap, int64_t *trace_rows, int32_t loc) {
    const char *fn = "hv_rgbd_odometry";
    HV_REQUIRE(v != nullptr && source_depth != nullptr && target_depth != nullptr && intr != nullptr && prm != nullptr && res != nullptr,
               HV_ERR_INVALID, "%s: null argument", fn);
    HV_REQUIRE((source_color == nullptr) == (target_color == nullptr), HV_ERR_INVALID,
               "%s: give both colour images (hybrid) or neither (depth only)", fn);
    const bool hybrid = source_color != nullptr;
    TkFrameModel model = od_frame_model(fn, v, source_depth, target_depth, depth_dtype, source_color, target_color, T_init, prm);
    const TkSchedule S{prm->depth_scale, prm->depth_min, prm->depth_max, prm->depth_outlier_trunc, prm->depth_huber_delta,
                       prm->intensity_weight, prm->intensity_huber_delta, prm->n_levels, prm->iterations};
    TkOutcome o{};
    const int rc = hybrid ? tk_run<true>(fn, v, model, S, depth_dtype, height, width, intr, &o, trace, trace_cap, trace_rows, loc)
                          : tk_run<false>(fn, v, model, S, depth_dtype, height, width, intr, &o, trace, trace_cap, trace_rows, loc);
    if (rc != HV_OK) return rc;
    // transformation = A itself; T_init when level 0 never got going (A then holds the steps of coarser levels at most)
    for (int i = 0; i < 16; ++i) res->transformation[i] = o.level0_started ? o.A[i] : model.T0[i];
    tk_copy_result(o, res);
    res->photometric_inliers = o.photometric_inliers;
    res->intensity_rmse = o.intensity_rmse;
    return HV_OK;
}

extern "C" int hv_rgbd_odometry_model(hv_volume *v, const void *depth, int32_t depth_dtype, const uint8_t *color, int32_t height,
                                      int32_t width, const double *intr, const hv_odometry_params *prm, int32_t level, float *out_depth,
                                      float *out_normal, uint8_t *out_mask, float *out_record, int32_t loc) {
    const char *fn = "hv_rgbd_odometry_model";
    HV_REQUIRE(v != nullptr && depth != nullptr && intr != nullptr && prm != nullptr, HV_ERR_INVALID, "%s: null argument", fn);
    HV_REQUIRE(depth_dtype == HV_DEPTH_F32 || depth_dtype == HV_DEPTH_U16, HV_ERR_INVALID, "%s: bad depth dtype %d", fn, (int)depth_dtype);
    HV_REQUIRE(loc == HV_HOST || loc == HV_DEVICE, HV_ERR_INVALID, "%s: bad loc %d", fn, (int)loc);
    HV_REQUIRE(level >= 0 && level < HV_TRACK_MAX_LEVELS, HV_ERR_INVALID, "%s: level must be in 0..%d", fn, HV_TRACK_MAX_LEVELS - 1);
    HV_REQUIRE(out_record == nullptr || color != nullptr, HV_ERR_INVALID, "%s: the record needs a colour image", fn);
    // the schedule's checks at n_levels = level + 1, one linearisation at level 0 (nothing is linearised here)
    const int32_t one[HV_TRACK_MAX_LEVELS] = {1, 0, 0, 0, 0, 0, 0, 0};
    const int nl = level + 1;
    const TkSchedule S{prm->depth_scale, prm->depth_min, prm->depth_max, prm->depth_outlier_trunc, 1.0, 0.0, 1.0, nl, one};
    int64_t steps = 0;
    int rc = tk_check_schedule(fn, S, false, height, width, intr, &steps);
    if (rc != HV_OK) return rc;
    const bool hybrid = color != nullptr;
    TkFrameModel model = od_frame_model(fn, v, depth, depth, depth_dtype, color, color, nullptr, prm);
    HV_HIP(hipSetDevice(v->device));

    // scratch: per level the depth (hybrid: and intensity) of the pyramid; for `level` also normal, mask and, hybrid, the record
    size_t off = 0;
    auto take = [&off](size_t bytes) {
        const size_t at = off;
        off += (bytes + 255) & ~(size_t)255;
        return at;
    };
    size_t o_d[HV_TRACK_MAX_LEVELS], o_i[HV_TRACK_MAX_LEVELS] = {};
    for (int l = 0; l < nl; ++l) {
        const size_t n = (size_t)(height >> l) * (size_t)(width >> l);
        o_d[l] = take(4 * n);
        if (hybrid) o_i[l] = take(4 * n);
    }
    const size_t n = (size_t)(height >> level) * (size_t)(width >> level);
    const size_t o_n = take(12 * n), o_m = take(n), o_r = hybrid ? take(16 * n) : 0;
    rc = hv_ensure_buffer(v, &v->track_buf, &v->track_buf_bytes, off);
    if (rc != HV_OK) return rc;
    char *base = (char *)v->track_buf;
    TkModelMaps maps[HV_TRACK_MAX_LEVELS];
    for (int l = 0; l < nl; ++l) {
        const double s = (double)(1 << l);
        maps[l] = TkModelMaps{(float *)(base + o_d[l]), nullptr, nullptr, hybrid ? (float *)(base + o_i[l]) : (float *)nullptr, nullptr,
                              height >> l, width >> l, {intr[0] / s, intr[1] / s, (intr[2] + 0.5) / s - 0.5, (intr[3] + 0.5) / s - 0.5}};
    }
    maps[level].normal = (float *)(base + o_n);
    maps[level].mask = (uint8_t *)(base + o_m);
    maps[level].rec = hybrid ? (float4 *)(base + o_r) : (float4 *)nullptr;

    // the one frame is the provider's target: staged once (its source slots are the same pointers)
    const void *d_depth = nullptr;
    const uint8_t *d_color = nullptr;
    rc = hv_stage_frame(v, depth, depth_dtype, color, (size_t)height * (size_t)width, loc, &d_depth, &d_color);
    if (rc != HV_OK) return rc;
    model.d_target_depth = d_depth;
    model.d_target_color = d_color;
    v->pipe_armed = false;
    rc = hybrid ? model.prepare<true>(maps, nl) : model.prepare<false>(maps, nl);
    if (rc != HV_OK) return rc;
    rc = hybrid ? model.level<true>(maps[level]) : model.level<false>(maps[level]);
    if (rc != HV_OK) return rc;
    HV_HIP(hipGetLastError());
    const hipMemcpyKind kind = loc == HV_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (out_depth) HV_HIP(hipMemcpyAsync(out_depth, maps[level].depth, 4 * n, kind, v->stream));
    if (out_normal) HV_HIP(hipMemcpyAsync(out_normal, maps[level].normal, 12 * n, kind, v->stream));
    if (out_mask) HV_HIP(hipMemcpyAsync(out_mask, maps[level].mask, n, kind, v->stream));
    if (out_record) HV_HIP(hipMemcpyAsync(out_record, maps[level].rec, 16 * n, kind, v->stream));
    HV_HIP(hipStreamSynchronize(v->stream));
    return HV_OK;
}

