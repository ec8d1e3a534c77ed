// libpyslam_hipvol.so — point queries of the TSDF map on gfx950 (hv_tsdf_sample_points, hv_tsdf_check_frame): signed distance,
// gradient, colour and observation count at given points, and the per-pixel verdict of a depth frame against the map.  The contract
// (locate, value, class) is written once in include/hipvol.h; tests/sample_reference.py restates it in numpy.
//
// One template, instantiated by front end (a point list, or the pixels of a depth image) and by output set (colour, gradient).  One
// lane per point; every lane takes the cell, its eight voxels and the trilinear form from hv_tsdf_cell.h, reads the eight weights,
// then the tsdf values, then - only in the instantiation that outputs colour - the colour sums.  In the image form a wave covers an
// 8 x 8 pixel tile (a workgroup of four waves 16 x 16 pixels, as the ray cast): the back-projected points of a tile fall into fewer
// units and fewer 64-byte lines than 64 pixels of a row.  No LDS, no float atomics, no scratch; the class counters are integer
// atomics, one per wave and class after a ballot.  The kernels read the table and the pool only.
#include <algorithm>
#include <cmath>

#include "hv_common.h"
#include "hv_tsdf_cell.h"
#include "hv_unproject.h"

namespace {

struct HvSampleParams {
    double voxel_length, sdf_trunc, grad_scale, weight_threshold;
    // image front end
    double fx, fy, cx, cy;
    double Rwc[9], twc[3];
    double depth_min, depth_max, tolerance;
    float depth_scale_f;
    int32_t height, width, depth_is_u16;
};

struct HvSampleOut {
    float *sdf, *gradient, *color, *weight;
    uint8_t *status; // the class in the image form
    unsigned long long *count; // [5] image form, or nullptr
};

// The contract's locate + value at p.  Outputs the caller did not ask for (COLOR / GRAD false) are not computed; every output is 0
// for HV_SAMPLE_OUTSIDE and HV_SAMPLE_UNOBSERVED.
template <bool COLOR, bool GRAD>
__device__ __forceinline__ int sp_sample(const HvTable &table, const char *__restrict__ pool, const HvSampleParams &P, const double *p,
                                         float &sdf, float *grad, float *col, float &weight) {
    sdf = 0.0f;
    weight = 0.0f;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (GRAD) grad[a] = 0.0f;
        if (COLOR) col[a] = 0.0f;
    }
    int32_t g0[3];
    double r[3];
    if (!hv_cell_locate(p, P.voxel_length, g0, r)) return HV_SAMPLE_OUTSIDE;
    const int nx = r[0] >= 0.5, ny = r[1] >= 0.5, nz = r[2] >= 0.5;
    unsigned long long ck = HV_EMPTY_KEY;
    int32_t ci = -1;
    int64_t at[8];
    const uint32_t held = hv_tsdf_cell_gather(table, g0, ck, ci, at);
    int64_t near_at = 0;
    bool near_held = false;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        int sx, sy, sz;
        hv_cell_corner(c, sx, sy, sz);
        const bool is_near = sx == nx && sy == ny && sz == nz;
        near_at = is_near ? at[c] : near_at;
        near_held = is_near ? (held >> c) & 1u : near_held;
    }
    if (!near_held) return HV_SAMPLE_OUTSIDE;
    // the eight weights first, the tsdf values after them
    const uint32_t *words = (const uint32_t *)pool;
    uint32_t w[8], wn = 0u;
    bool all = true;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        int sx, sy, sz;
        hv_cell_corner(c, sx, sy, sz);
        const bool has = (held >> c) & 1u;
        w[c] = has ? words[at[c] + HV_TSDF_RRR] : 0u;
        all = all && has && (double)w[c] > P.weight_threshold;
        wn = (sx == nx && sy == ny && sz == nz) ? w[c] : wn;
    }
    if (!((double)wn > P.weight_threshold)) return HV_SAMPLE_UNOBSERVED;
    weight = (float)wn;
    if (!all) {
        sdf = (float)(P.sdf_trunc * (double)((const float *)pool)[near_at]);
        if (COLOR) {
#pragma unroll
            for (int k = 0; k < 3; ++k) col[k] = (float)(((double)words[near_at + (2 + k) * HV_TSDF_RRR] / (double)wn) / 255.0);
        }
        return HV_SAMPLE_NEAREST;
    }
    double f[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) f[c] = (double)((const float *)pool)[at[c]];
    if (GRAD) {
        double phi, e[3];
        hv_cell_lerp_grad(r, f, phi, e);
        sdf = (float)(P.sdf_trunc * phi);
#pragma unroll
        for (int a = 0; a < 3; ++a) grad[a] = (float)(P.grad_scale * e[a]);
    } else {
        sdf = (float)(P.sdf_trunc * hv_cell_lerp(r, f));
    }
    if (COLOR) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
#pragma unroll
            for (int c = 0; c < 8; ++c) f[c] = (double)words[at[c] + (2 + k) * HV_TSDF_RRR] / (double)w[c];
            col[k] = (float)(hv_cell_lerp(r, f) / 255.0);
        }
    }
    return HV_SAMPLE_TRILINEAR;
}

// IMAGE = false: `in` is the point list [n,3] (float64 when F64, else float32), one lane per point.
// IMAGE = true: `in` is the depth image; a wave covers an 8 x 8 pixel tile, O.status takes the class, O.count the class counts.
template <bool IMAGE, bool F64, bool COLOR, bool GRAD>
__global__ __launch_bounds__(256) void k_tsdf_sample(HvTable table, const char *__restrict__ pool, const void *__restrict__ in, int64_t n,
                                                     HvSampleParams P, HvSampleOut O) {
    if constexpr (IMAGE) {
        const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
        const int u = (int)blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
        const int v = (int)blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
        const bool inside = u < P.width && v < P.height; // partial tiles at the right and bottom edges: such a lane reads and writes nothing
        const int64_t pix = (int64_t)v * P.width + u;
        int cls = -1;
        float sdf = 0.0f;
        if (inside) {
            float d = P.depth_is_u16 ? (float)((const uint16_t *)in)[pix] : ((const float *)in)[pix];
            d = d / P.depth_scale_f;
            cls = HV_CHECK_INVALID;
            if (isfinite(d) && (double)d > P.depth_min && (double)d <= P.depth_max) {
                const double z = (double)d;
                const double a = ((double)u - P.cx) / P.fx, x = a * z;
                const double b = ((double)v - P.cy) / P.fy, y = b * z;
                double p[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) p[k] = ((P.Rwc[k * 3 + 0] * x + P.Rwc[k * 3 + 1] * y) + P.Rwc[k * 3 + 2] * z) + P.twc[k];
                float weight;
                const int status = sp_sample<false, false>(table, pool, P, p, sdf, nullptr, nullptr, weight);
                if (status == HV_SAMPLE_OUTSIDE || status == HV_SAMPLE_UNOBSERVED) cls = HV_CHECK_UNKNOWN;
                else if ((double)sdf > P.tolerance) cls = HV_CHECK_IN_FRONT;
                else if ((double)sdf < -P.tolerance) cls = HV_CHECK_BEHIND;
                else cls = HV_CHECK_CONSISTENT;
            }
            if (O.sdf) O.sdf[pix] = sdf;
            if (O.status) O.status[pix] = (uint8_t)cls;
        }
        if (O.count != nullptr) { // exact integer counts: one atomic per wave and class
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                const unsigned long long m = __ballot(cls == k);
                if (m != 0ull && lane == __ffsll((long long)m) - 1) atomicAdd(&O.count[k], (unsigned long long)__popcll(m));
            }
        }
    } else {
        const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
        if (i >= n) return;
        double p[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) p[a] = F64 ? ((const double *)in)[i * 3 + a] : (double)((const float *)in)[i * 3 + a];
        float sdf, weight, grad[3], col[3];
        const int status = sp_sample<COLOR, GRAD>(table, pool, P, p, sdf, grad, col, weight);
        if (O.sdf) O.sdf[i] = sdf;
        if (O.weight) O.weight[i] = weight;
        if (O.status) O.status[i] = (uint8_t)status;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (GRAD) O.gradient[i * 3 + a] = grad[a];
            if (COLOR) O.color[i * 3 + a] = col[a];
        }
    }
}

HvSampleParams sample_params(const hv_volume *v, double weight_threshold) {
    HvSampleParams P{};
    P.voxel_length = v->cfg.voxel_size;
    P.sdf_trunc = v->cfg.sdf_trunc;
    P.grad_scale = v->cfg.sdf_trunc / v->cfg.voxel_size;
    P.weight_threshold = weight_threshold;
    return P;
}

} // namespace

extern "C" int hv_tsdf_sample_points(hv_volume *v, const void *points, int32_t point_dtype, int64_t n, double weight_threshold, float *sdf,
                                     float *gradient, float *color, float *weight, uint8_t *status, int32_t loc) {
    const char *fn = "hv_tsdf_sample_points";
    HV_REQUIRE(v != nullptr, HV_ERR_INVALID, "%s: null argument", fn);
    int rc = hv_tsdf_require_whole_map(v, fn, "the volume");
    if (rc != HV_OK) return rc;
    HV_REQUIRE(n >= 0 && n <= (1ll << 36), HV_ERR_INVALID, "%s: bad point count %lld", fn, (long long)n);
    HV_REQUIRE(points != nullptr || n == 0, HV_ERR_INVALID, "%s: null points", fn);
    HV_REQUIRE(point_dtype == HV_F32 || point_dtype == HV_F64, HV_ERR_INVALID, "%s: points must be float32 or float64", fn);
    HV_REQUIRE(std::isfinite(weight_threshold) && weight_threshold >= 0.0, HV_ERR_INVALID, "%s: weight_threshold must be finite and >= 0", fn);
    HV_REQUIRE(loc == HV_HOST || loc == HV_DEVICE, HV_ERR_INVALID, "%s: bad loc %d", fn, (int)loc);
    if (n == 0) return HV_OK;
    HV_HIP(hipSetDevice(v->device));

    const size_t un = (size_t)n;
    HvStage st(v, loc);
    const int i_points = st.in(points, un * 3 * (point_dtype == HV_F64 ? 8 : 4));
    const int o_sdf = st.out(sdf, 4 * un), o_grad = st.out(gradient, 12 * un), o_color = st.out(color, 12 * un), o_weight = st.out(weight, 4 * un),
              o_status = st.out(status, un);
    rc = st.commit(&v->stage, &v->stage_bytes);
    if (rc != HV_OK) return rc;
    const void *d_points = st.dev<const void>(i_points);
    // reads only, as hv_tsdf_ray_cast: the next batch starts a fresh touch + pack chain behind this call
    v->pipe_armed = false;

    const HvSampleParams P = sample_params(v, weight_threshold);
    const HvSampleOut O{st.dev<float>(o_sdf), st.dev<float>(o_grad), st.dev<float>(o_color), st.dev<float>(o_weight), st.dev<uint8_t>(o_status), nullptr};
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    const bool f64 = point_dtype == HV_F64, c = color != nullptr, g = gradient != nullptr;
    hv_profile_begin(v);
#define HV_SAMPLE_LAUNCH(F, C, G) \
    hipLaunchKernelGGL((k_tsdf_sample<false, F, C, G>), grid, block, 0, v->stream, v->table, (const char *)v->pool, d_points, n, P, O)
#define HV_SAMPLE_PICK(F)                                                                                                                 \
    do {                                                                                                                                  \
        if (c && g) HV_SAMPLE_LAUNCH(F, true, true);                                                                                      \
        else if (c) HV_SAMPLE_LAUNCH(F, true, false);                                                                                     \
        else if (g) HV_SAMPLE_LAUNCH(F, false, true);                                                                                     \
        else HV_SAMPLE_LAUNCH(F, false, false);                                                                                           \
    } while (0)
    if (f64) HV_SAMPLE_PICK(true);
    else HV_SAMPLE_PICK(false);
#undef HV_SAMPLE_PICK
#undef HV_SAMPLE_LAUNCH
    hv_profile_end(v, 0);
    HV_HIP(hipGetLastError());
    return st.finish();
}

extern "C" int hv_tsdf_check_frame(hv_volume *v, const void *depth, int32_t depth_dtype, int32_t height, int32_t width, const double *intr,
                                   const double *T_cw, const hv_check_params *params, float *sdf, uint8_t *cls, hv_check_stats *stats,
                                   int32_t loc) {
    const char *fn = "hv_tsdf_check_frame";
    HV_REQUIRE(v != nullptr && depth != nullptr && intr != nullptr && T_cw != nullptr && params != nullptr, HV_ERR_INVALID, "%s: null argument", fn);
    int rc = hv_tsdf_require_whole_map(v, fn, "the volume");
    if (rc != HV_OK) return rc;
    HV_REQUIRE(depth_dtype == HV_DEPTH_F32 || depth_dtype == HV_DEPTH_U16, HV_ERR_INVALID, "%s: bad depth dtype %d", fn, (int)depth_dtype);
    HV_REQUIRE(loc == HV_HOST || loc == HV_DEVICE, HV_ERR_INVALID, "%s: bad loc %d", fn, (int)loc);
    HV_REQUIRE(height > 0 && width > 0 && height <= 65535 && width <= 65535, HV_ERR_INVALID, "%s: bad image size %d x %d", fn, (int)height,
               (int)width);
    HV_REQUIRE(std::isfinite(params->depth_min) && std::isfinite(params->depth_max) && params->depth_min >= 0.0 &&
                   params->depth_min < params->depth_max,
               HV_ERR_INVALID, "%s: bad depth range [%g, %g)", fn, params->depth_min, params->depth_max);
    HV_REQUIRE(std::isfinite(intr[0]) && std::isfinite(intr[1]) && std::isfinite(intr[2]) && std::isfinite(intr[3]) && intr[0] != 0.0 &&
                   intr[1] != 0.0 && std::isfinite(params->depth_scale) && params->depth_scale != 0.0,
               HV_ERR_INVALID, "%s: bad intrinsics / scale", fn);
    HV_REQUIRE(std::isfinite(params->weight_threshold) && params->weight_threshold >= 0.0, HV_ERR_INVALID,
               "%s: weight_threshold must be finite and >= 0", fn);
    HV_REQUIRE(std::isfinite(params->tolerance) && params->tolerance > 0.0, HV_ERR_INVALID, "%s: tolerance must be positive and finite", fn);
    // T_cw is inverted as a rigid transform (hv_unproject.h): refuse what is not one, by hv_tsdf_integrate_volume's rule
    for (int i = 0; i < 16; ++i) HV_REQUIRE(std::isfinite(T_cw[i]), HV_ERR_INVALID, "%s: T_cw is not finite", fn);
    HV_REQUIRE(T_cw[12] == 0.0 && T_cw[13] == 0.0 && T_cw[14] == 0.0 && T_cw[15] == 1.0, HV_ERR_INVALID, "%s: T_cw's bottom row is not (0, 0, 0, 1)", fn);
    double ortho = 0.0;
    for (int a = 0; a < 3; ++a) {
        double row = 0.0;
        for (int b = 0; b < 3; ++b) {
            double s = 0.0;
            for (int k = 0; k < 3; ++k) s += T_cw[k * 4 + a] * T_cw[k * 4 + b];
            row += std::fabs(s - (a == b ? 1.0 : 0.0));
        }
        ortho = std::max(ortho, row);
    }
    const double det = T_cw[0] * (T_cw[5] * T_cw[10] - T_cw[6] * T_cw[9]) - T_cw[1] * (T_cw[4] * T_cw[10] - T_cw[6] * T_cw[8]) +
                       T_cw[2] * (T_cw[4] * T_cw[9] - T_cw[5] * T_cw[8]);
    HV_REQUIRE(ortho <= 1.0e-6 && det >= 0.0, HV_ERR_INVALID, "%s: T_cw is not rigid (|R^T R - I|_inf = %.3g, det = %.3g)", fn, ortho, det);
    HV_HIP(hipSetDevice(v->device));

    // head: the 5 class counters
    const size_t npx = (size_t)height * (size_t)width;
    HvStage st(v, loc);
    st.head(stats != nullptr ? 256 : 0);
    const int i_depth = st.in(depth, npx * (depth_dtype == HV_DEPTH_U16 ? 2 : 4));
    const int o_sdf = st.out(sdf, 4 * npx), o_cls = st.out(cls, npx);
    rc = st.commit(&v->stage, &v->stage_bytes);
    if (rc != HV_OK) return rc;
    const void *d_depth = st.dev<const void>(i_depth);
    v->pipe_armed = false; // reads only, as hv_tsdf_ray_cast

    HvSampleParams P = sample_params(v, params->weight_threshold);
    const HvUnprojectParams U = unproject_params(depth_dtype, params->depth_scale, height, width, intr, T_cw, params->depth_min, params->depth_max);
    P.fx = intr[0];
    P.fy = intr[1];
    P.cx = intr[2];
    P.cy = intr[3];
    for (int i = 0; i < 9; ++i) P.Rwc[i] = U.Rwc[i];
    for (int i = 0; i < 3; ++i) P.twc[i] = U.twc[i];
    P.depth_min = params->depth_min;
    P.depth_max = params->depth_max;
    P.tolerance = params->tolerance;
    P.depth_scale_f = (float)params->depth_scale;
    P.height = height;
    P.width = width;
    P.depth_is_u16 = depth_dtype == HV_DEPTH_U16;
    unsigned long long *d_count = (unsigned long long *)st.head_dev;
    if (d_count != nullptr) HV_HIP(hipMemsetAsync(d_count, 0, 5 * sizeof(unsigned long long), v->stream));
    const HvSampleOut O{st.dev<float>(o_sdf), nullptr, nullptr, nullptr, st.dev<uint8_t>(o_cls), d_count};
    hv_profile_begin(v);
    hipLaunchKernelGGL((k_tsdf_sample<true, false, false, false>), dim3((unsigned)((width + 15) / 16), (unsigned)((height + 15) / 16)), dim3(256),
                       0, v->stream, v->table, (const char *)v->pool, d_depth, (int64_t)npx, P, O);
    hv_profile_end(v, 0);
    HV_HIP(hipGetLastError());
    unsigned long long h_count[5];
    rc = st.finish(stats != nullptr ? h_count : nullptr, sizeof(h_count));
    if (rc != HV_OK) return rc;
    if (stats != nullptr)
        for (int k = 0; k < 5; ++k) stats->count[k] = (int64_t)h_count[k];
    return HV_OK;
}
