// libpyslam_hipvol.so — ray casting of the TSDF map on gfx950 (hv_tsdf_ray_cast): depth, vertex, normal, colour and hit mask as
// the fused map predicts them from a pinhole camera at pose T_cw.  The contract (march, bracket, refinement, outputs) is written
// once in include/hipvol.h; tests/raycast_reference.py restates it in numpy.
//
// One thread per ray, one wave per 8 x 8 pixel tile (a workgroup of four waves covers 16 x 16 pixels), so that the rays of a wave
// walk the same units and read neighbouring voxels.  Each lane caches its last unit key -> pool index (hv_tsdf_cell.h).  The march
// and the refinement run in float32; the normal is GetNormalAt (hv_tsdf_gradient, double), as the point-cloud normals.
// The kernel reads the table and the pool only.
#include <cmath>

#include "hv_common.h"
#include "hv_tsdf_sample.h"

namespace {

struct HvRayParams {
    float rot[9];  // R_wc, row-major
    float orig[3]; // camera centre in the world (T_wc * 0)
    float fx, fy, cx, cy;
    float voxel_length, sdf_trunc, unit_eps;
    float depth_min, depth_max, weight_threshold, depth_scale;
    int32_t height, width, max_steps;
    double voxel_length_d, unit_length_d;
};

struct HvRayOut {
    float *depth, *vertex, *normal, *color;
    uint8_t *mask;
};

// the cell of p in float, by the ray caster's own formula (the corner order and the trilinear form are hv_tsdf_cell.h's)
__device__ __forceinline__ void rc_cell(const float *p, float vl, int32_t *g0, float *r) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float g = (p[a] - 0.5f * vl) / vl;
        const float fl = floorf(g);
        g0[a] = (int32_t)fl;
        r[a] = g - fl;
    }
}

// Trilinear tsdf at p; false unless all 8 voxels are observed (weight > threshold)
__device__ inline bool rc_tsdf_tri(const HvTable &table, const char *__restrict__ pool, const HvRayParams &P, const float *p,
                                   unsigned long long &ck, int32_t &ci, float &out) {
    int32_t g0[3];
    float r[3], f[8];
    rc_cell(p, P.voxel_length, g0, r);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        int sx, sy, sz, word;
        hv_cell_corner(i, sx, sy, sz);
        const int32_t idx = hv_tsdf_voxel_at(table, g0[0] + sx, g0[1] + sy, g0[2] + sz, ck, ci, word);
        if (idx < 0) return false;
        const char *u = pool + (int64_t)idx * HV_TSDF_UNIT_BYTES;
        const uint32_t w = ((const uint32_t *)(u + HV_TSDF_PLANE_BYTES))[word];
        if (!((float)w > P.weight_threshold)) return false;
        f[i] = ((const float *)u)[word];
    }
    out = hv_cell_lerp(r, f);
    return true;
}

// Colour at p in [0, 1]: the trilinear mean colour when all 8 voxels are observed, else the nearest voxel's mean (0 if none)
__device__ inline void rc_color(const HvTable &table, const char *__restrict__ pool, const HvRayParams &P, const float *p,
                                unsigned long long &ck, int32_t &ci, float *rgb) {
    int32_t g0[3];
    float r[3], c[3][8];
    rc_cell(p, P.voxel_length, g0, r);
    bool valid = true;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        int sx, sy, sz, word;
        hv_cell_corner(i, sx, sy, sz);
        const int32_t idx = valid ? hv_tsdf_voxel_at(table, g0[0] + sx, g0[1] + sy, g0[2] + sz, ck, ci, word) : -1;
        if (idx < 0) {
            valid = false;
            continue;
        }
        const char *u = pool + (int64_t)idx * HV_TSDF_UNIT_BYTES;
        const uint32_t w = ((const uint32_t *)(u + HV_TSDF_PLANE_BYTES))[word];
        valid = valid && (float)w > P.weight_threshold;
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k][i] = valid ? (float)((const uint32_t *)(u + (2 + k) * HV_TSDF_PLANE_BYTES))[word] / (float)w : 0.0f;
    }
    if (valid) {
#pragma unroll
        for (int k = 0; k < 3; ++k) rgb[k] = hv_cell_lerp(r, c[k]) / 255.0f;
        return;
    }
    int word;
    const int32_t idx = hv_tsdf_voxel_at(table, (int32_t)floorf(p[0] / P.voxel_length), (int32_t)floorf(p[1] / P.voxel_length),
                                  (int32_t)floorf(p[2] / P.voxel_length), ck, ci, word);
    const char *u = pool + (int64_t)(idx < 0 ? 0 : idx) * HV_TSDF_UNIT_BYTES;
    const uint32_t w = idx < 0 ? 0u : ((const uint32_t *)(u + HV_TSDF_PLANE_BYTES))[word];
#pragma unroll
    for (int k = 0; k < 3; ++k) rgb[k] = w > 0 ? (float)((const uint32_t *)(u + (2 + k) * HV_TSDF_PLANE_BYTES))[word] / (float)w / 255.0f : 0.0f;
}

__global__ __launch_bounds__(256) void k_tsdf_ray_cast(HvTable table, const char *__restrict__ pool, HvRayParams P, HvRayOut O) {
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const int u = (int)blockIdx.x * 16 + (wave & 1) * 8 + (lane & 7);
    const int v = (int)blockIdx.y * 16 + (wave >> 1) * 8 + (lane >> 3);
    if (u >= P.width || v >= P.height) return;
    const int64_t pix = (int64_t)v * P.width + u;

    const float dc0 = ((float)u - P.cx) / P.fx, dc1 = ((float)v - P.cy) / P.fy;
    float d[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) d[a] = P.rot[a * 3] * dc0 + P.rot[a * 3 + 1] * dc1 + P.rot[a * 3 + 2];
    const float vl = P.voxel_length;

    unsigned long long ck = HV_EMPTY_KEY;
    int32_t ci = -1;
    // march: the ray parameter is camera z
    float z = P.depth_min, z_prev = 0.0f, f_prev = 0.0f, f = 0.0f;
    bool have_prev = false, hit = false;
    for (int it = 0; it < P.max_steps && z < P.depth_max; ++it) {
        float p[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) p[a] = P.orig[a] + z * d[a];
        int32_t gv[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) gv[a] = (int32_t)floorf(p[a] / vl);
        int word;
        const int32_t idx = hv_tsdf_voxel_at(table, gv[0], gv[1], gv[2], ck, ci, word);
        if (idx < 0) { // no unit here: to where the ray leaves the unit's box
            float t = INFINITY;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const int32_t ub = gv[a] >> 4;
                if (d[a] > 0.0f) t = fminf(t, ((float)((ub + 1) * HV_TSDF_R) * vl - P.orig[a]) / d[a]);
                else if (d[a] < 0.0f) t = fminf(t, ((float)(ub * HV_TSDF_R) * vl - P.orig[a]) / d[a]);
            }
            z = fmaxf(t, z) + P.unit_eps;
            have_prev = false;
            continue;
        }
        const char *unit = pool + (int64_t)idx * HV_TSDF_UNIT_BYTES;
        const uint32_t w = ((const uint32_t *)(unit + HV_TSDF_PLANE_BYTES))[word];
        if (!((float)w > P.weight_threshold)) {
            z += vl;
            have_prev = false;
            continue;
        }
        f = ((const float *)unit)[word];
        if (have_prev && f_prev > 0.0f && f <= 0.0f) {
            hit = true;
            break;
        }
        have_prev = true;
        z_prev = z;
        f_prev = f;
        z += f > 0.0f ? fmaxf(vl, HV_RAYCAST_STEP_FRAC * f * P.sdf_trunc) : vl;
    }
    if (!hit) {
        if (O.depth) O.depth[pix] = 0.0f;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (O.vertex) O.vertex[pix * 3 + a] = 0.0f;
            if (O.normal) O.normal[pix * 3 + a] = 0.0f;
            if (O.color) O.color[pix * 3 + a] = 0.0f;
        }
        if (O.mask) O.mask[pix] = 0;
        return;
    }

    // refine: regula falsi (Illinois) on the trilinear field.  The nearest samples bracket the root of the nearest field, which
    // can lie up to about a voxel away from the trilinear one: each end moves one voxel outwards where the trilinear sample there is
    // valid and of its sign, else stays (trilinear value if valid and of its sign, else the nearest value)
    float za = z_prev, fa = f_prev, zb = z, fb = f, zs = z;
    {
        const float za_out = fmaxf(z_prev - vl, P.depth_min), zb_out = fminf(z + vl, P.depth_max);
        float p[3], t;
#pragma unroll
        for (int a = 0; a < 3; ++a) p[a] = P.orig[a] + za_out * d[a];
        if (rc_tsdf_tri(table, pool, P, p, ck, ci, t) && t > 0.0f) {
            za = za_out;
            fa = t;
        } else {
#pragma unroll
            for (int a = 0; a < 3; ++a) p[a] = P.orig[a] + za * d[a];
            if (rc_tsdf_tri(table, pool, P, p, ck, ci, t) && t > 0.0f) fa = t;
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) p[a] = P.orig[a] + zb_out * d[a];
        if (rc_tsdf_tri(table, pool, P, p, ck, ci, t) && t <= 0.0f) {
            zb = zb_out;
            fb = t;
        } else {
#pragma unroll
            for (int a = 0; a < 3; ++a) p[a] = P.orig[a] + zb * d[a];
            if (rc_tsdf_tri(table, pool, P, p, ck, ci, t) && t <= 0.0f) fb = t;
        }
    }
    int side = 0;
    for (int k = 0; k < HV_RAYCAST_REFINE_ITERS; ++k) {
        zs = za + fa * (zb - za) / (fa - fb);
        float p[3], fs;
#pragma unroll
        for (int a = 0; a < 3; ++a) p[a] = P.orig[a] + zs * d[a];
        if (!rc_tsdf_tri(table, pool, P, p, ck, ci, fs)) break;
        if (fs > 0.0f) {
            za = zs;
            fa = fs;
            if (side == 1) fb *= 0.5f;
            side = 1;
        } else {
            zb = zs;
            fb = fs;
            if (side == -1) fa *= 0.5f;
            side = -1;
        }
    }

    float p[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) p[a] = P.orig[a] + zs * d[a];
    if (O.depth) O.depth[pix] = zs * P.depth_scale;
    if (O.vertex) {
#pragma unroll
        for (int a = 0; a < 3; ++a) O.vertex[pix * 3 + a] = p[a];
    }
    if (O.normal) {
        const double pd[3] = {(double)p[0], (double)p[1], (double)p[2]};
        double nn[3];
        hv_tsdf_gradient(table, pool, P.voxel_length_d, P.unit_length_d, pd, ck, ci, nn);
        const double q = nn[0] * nn[0] + nn[1] * nn[1] + nn[2] * nn[2];
        const double s = sqrt(q);
#pragma unroll
        for (int a = 0; a < 3; ++a) O.normal[pix * 3 + a] = (float)(q > 0.0 ? nn[a] / s : nn[a]);
    }
    if (O.color) {
        float rgb[3];
        rc_color(table, pool, P, p, ck, ci, rgb);
#pragma unroll
        for (int a = 0; a < 3; ++a) O.color[pix * 3 + a] = rgb[a];
    }
    if (O.mask) O.mask[pix] = 1;
}

} // namespace

// Queue one cast on the volume's stream into device arrays (any may be NULL); bracketed for hv_profile_read.  The caller has checked
// the arguments and set pipe_armed = false.  (hv_tsdf_track renders its model with it.)
int hv_ray_cast_launch(hv_volume *v, int32_t height, int32_t width, const double *intr, const double *T_cw, double depth_min,
                       double depth_max, double weight_threshold, double depth_scale, float *depth, float *vertex, float *normal,
                       float *color, uint8_t *mask) {
    HvRayParams P{};
    double T_wc[16];
    hv_invert4x4(T_cw, T_wc);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) P.rot[r * 3 + c] = (float)T_wc[r * 4 + c];
        P.orig[r] = (float)T_wc[r * 4 + 3];
    }
    P.fx = (float)intr[0];
    P.fy = (float)intr[1];
    P.cx = (float)intr[2];
    P.cy = (float)intr[3];
    P.voxel_length = (float)v->cfg.voxel_size;
    P.sdf_trunc = (float)v->cfg.sdf_trunc;
    P.unit_eps = HV_RAYCAST_UNIT_EPS * P.voxel_length;
    P.depth_min = (float)depth_min;
    P.depth_max = (float)depth_max;
    P.weight_threshold = (float)weight_threshold;
    P.depth_scale = (float)depth_scale;
    P.height = height;
    P.width = width;
    const double steps = std::ceil(4.0 * (depth_max - depth_min) / v->cfg.voxel_size);
    P.max_steps = (int32_t)std::min(steps, 1.0e8);
    P.voxel_length_d = v->cfg.voxel_size;
    P.unit_length_d = v->cfg.voxel_size * (double)HV_TSDF_R;
    HvRayOut O{depth, vertex, normal, color, mask};
    hv_profile_begin(v);
    hipLaunchKernelGGL(k_tsdf_ray_cast, dim3((unsigned)((width + 15) / 16), (unsigned)((height + 15) / 16)), dim3(256), 0, v->stream, v->table,
                       (const char *)v->pool, P, O);
    hv_profile_end(v, 0);
    HV_HIP(hipGetLastError());
    return HV_OK;
}

extern "C" int hv_tsdf_ray_cast(hv_volume *v, int32_t height, int32_t width, const double *intr, const double *T_cw, double depth_min,
                                double depth_max, double weight_threshold, double depth_scale, float *depth, float *vertex,
                                float *normal, float *color, uint8_t *mask, int32_t loc) {
    HV_REQUIRE(v != nullptr && intr != nullptr && T_cw != nullptr, HV_ERR_INVALID, "hv_tsdf_ray_cast: null argument");
    HV_REQUIRE(v->cfg.mode == HV_MODE_TSDF, HV_ERR_MODE, "hv_tsdf_ray_cast: volume is not in TSDF mode");
    HV_REQUIRE(v->owner_world <= 1, HV_ERR_MODE, "hv_tsdf_ray_cast: ray_cast needs the whole volume (owner-sharded: merge or gather first)");
    HV_REQUIRE(height > 0 && width > 0 && height <= 65535 && width <= 65535, HV_ERR_INVALID, "hv_tsdf_ray_cast: bad image size %d x %d",
               (int)height, (int)width);
    HV_REQUIRE(std::isfinite(depth_min) && std::isfinite(depth_max) && depth_min >= 0.0 && depth_min < depth_max, HV_ERR_INVALID,
               "hv_tsdf_ray_cast: bad depth range [%g, %g)", depth_min, depth_max);
    HV_REQUIRE(intr[0] != 0.0 && intr[1] != 0.0 && std::isfinite(weight_threshold) && std::isfinite(depth_scale), HV_ERR_INVALID,
               "hv_tsdf_ray_cast: bad intrinsics / threshold / scale");
    HV_REQUIRE(loc == HV_HOST || loc == HV_DEVICE, HV_ERR_INVALID, "hv_tsdf_ray_cast: bad loc %d", (int)loc);
    HV_HIP(hipSetDevice(v->device));

    // outputs: in place (HV_DEVICE) or in the volume's staging buffer, copied back before returning (HV_HOST)
    const size_t npx = (size_t)height * (size_t)width;
    HvStage st(v, loc);
    const int o_depth = st.out(depth, 4 * npx), o_vertex = st.out(vertex, 12 * npx), o_normal = st.out(normal, 12 * npx), o_color = st.out(color, 12 * npx),
              o_mask = st.out(mask, npx);
    int rc = st.commit(&v->stage, &v->stage_bytes);
    if (rc != HV_OK) return rc;
    // a batch issued after this call must not start claiming units (its touch + pack launch on the auxiliary stream) while the
    // cast still reads the table: the next hv_tsdf_integrate_batch starts a fresh chain behind it
    v->pipe_armed = false;
    rc = hv_ray_cast_launch(v, height, width, intr, T_cw, depth_min, depth_max, weight_threshold, depth_scale, st.dev<float>(o_depth),
                            st.dev<float>(o_vertex), st.dev<float>(o_normal), st.dev<float>(o_color), st.dev<uint8_t>(o_mask));
    if (rc != HV_OK) return rc;
    return st.finish();
}
