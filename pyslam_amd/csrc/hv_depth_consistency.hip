// libpyslam_hipvol.so — hv_depth_consistency: the geometric consistency check between a depth map and the depth maps of 1..4 posed
// neighbours, with fusion of the agreeing depths.  A reference pixel is projected with its depth into a source view (rule M3, the
// device functions of the plane sweep), the source's depth is read there and projected back: the view agrees when the pixel lands
// where it started at the depth it started with.  The rules C1 - C7 are stated in include/hipvol.h and restated in numpy in
// tests/depth_consistency_reference.py, which this file is held to bit for bit.
//
// One kernel on the volume's stream, one lane per reference pixel.  A workgroup is a 64 x 4 pixel tile, a wave one row of 64 pixels:
// neighbouring pixels project to neighbouring source pixels, so a wave's gather falls on a few source rows.  The matrices and the
// source pointers travel by value (scalar registers).  The gathers of all views are issued before the first backward projection.
#include <cmath>

#include "hv_mvs_project.h"

struct DcViews {
    float m[MVS_MAX_VIEWS][12];     // [A | b]: reference pixel -> source s
    float back[MVS_MAX_VIEWS][12];  // [A' | b']: pixel of source s -> reference
    const float *depth[MVS_MAX_VIEWS];
    int n;
};

struct DcRule {
    float max_e2;  // max_reproj_error squared, formed once on the host
    float inv_depth_tol, rel_depth_tol;
    int min_consistent, max_violations, fuse;
};

static constexpr int DC_TILE_W = 64, DC_TILE_H = 4;
// the counters of the stats: DC_STAT_SETS sets of three, a cache line apart, a workgroup adding to the set of its index - 5640 waves
// adding to ONE set queue up behind each other at one L2 channel (measured: 75 us at 752 x 480 against 9 us for the kernel itself).
// The host adds the sets up: integers, so the sums do not depend on the order
static constexpr int DC_STAT_SETS = 64, DC_STAT_STRIDE = 16;  // (16 uint64 = 128 bytes)

__device__ __forceinline__ bool dc_is_depth(float z) { return z > 0.0f && z < INFINITY; }  // (a NaN fails both)

__global__ __launch_bounds__(256) void k_depth_consistency(const DcViews V, const DcRule R, const float *__restrict__ depth, int H, int W,
                                                            float *__restrict__ depth_out, uint32_t *__restrict__ counts_out,
                                                            unsigned long long *__restrict__ stat) {
    const int lane = threadIdx.x & 63;
    const int x = blockIdx.x * DC_TILE_W + lane, y = blockIdx.y * DC_TILE_H + (threadIdx.x >> 6);
    const bool inside = x < W && y < H;  // (no early return: the wave's counts are taken with every lane present)
    const int64_t p = (int64_t)y * W + x;
    // C1
    const float z = inside ? depth[p] : 0.0f;
    const bool valid = dc_is_depth(z);
    const float w = 1.0f / z;
    // C2 for every view, and all the gathers in flight before anything is worked out from them
    int q[MVS_MAX_VIEWS];
    float zs[MVS_MAX_VIEWS], d[MVS_MAX_VIEWS];
#pragma unroll
    for (int s = 0; s < MVS_MAX_VIEWS; ++s) {
        q[s] = -1;
        zs[s] = 0.0f;
        d[s] = 0.0f;
        if (s < V.n) {
            float a[3];
            mvs_ray(V.m[s], x, y, a);
            if (valid) q[s] = mvs_source_pixel(a, V.m[s], w, H, W);
            zs[s] = z * (a[2] + w * V.m[s][11]);  // z q2, with the q2 of rule M3
            if (q[s] >= 0) d[s] = V.depth[s][q[s]];
        }
    }
    int agree = 0, occluded = 0, violated = 0, seen = 0;
    float acc = z;
    const float fx = (float)x, fy = (float)y;
    const float tol = R.inv_depth_tol + R.rel_depth_tol * w;
#pragma unroll
    for (int s = 0; s < MVS_MAX_VIEWS; ++s) {
        if (s < V.n && q[s] >= 0) {
            seen += 1;
            if (dc_is_depth(d[s])) {
                // C3
                const float *__restrict__ m = V.back[s];
                const int vi = q[s] / W;
                const float vr = (float)vi, ur = (float)(q[s] - vi * W);
                const float ws = 1.0f / d[s];
                const float q0 = ((m[0] * ur + m[1] * vr) + m[2]) + ws * m[3];
                const float q1 = ((m[4] * ur + m[5] * vr) + m[6]) + ws * m[7];
                const float q2 = ((m[8] * ur + m[9] * vr) + m[10]) + ws * m[11];
                const float xb = q0 / q2, yb = q1 / q2, zb = d[s] * q2;
                const float ex = xb - fx, ey = yb - fy;
                const float e2 = ex * ex + ey * ey;
                const float wb = 1.0f / zb;
                // C4, C5
                if (q2 > 0.0f && e2 <= R.max_e2 && fabsf(wb - w) <= tol) {
                    agree += 1;
                    acc = acc + zb;
                } else if (d[s] < zs[s]) {
                    occluded += 1;
                } else {
                    violated += 1;
                }
            }
        }
    }
    // C6, C7
    const bool kept = valid && agree >= R.min_consistent && violated <= R.max_violations;
    if (inside) {
        if (depth_out != nullptr) depth_out[p] = !kept ? 0.0f : (R.fuse != 0 ? acc / (float)(agree + 1) : z);
        if (counts_out != nullptr)
            counts_out[p] = (uint32_t)agree | (uint32_t)occluded << 8 | (uint32_t)violated << 16 | (uint32_t)seen << 24;
    }
    if (stat != nullptr) {  // exact integer counts of the wave, added by its first three lanes in one atomic instruction
        const unsigned long long n_valid = __popcll(__ballot(valid)), n_kept = __popcll(__ballot(kept));
        const unsigned long long n_agree = (unsigned long long)__popcll(__ballot((agree & 1) != 0)) +
                                           2ull * __popcll(__ballot((agree & 2) != 0)) + 4ull * __popcll(__ballot((agree & 4) != 0));
        const unsigned set = (blockIdx.y * gridDim.x + blockIdx.x) % DC_STAT_SETS;
        if (lane < 3 && n_valid != 0ull) atomicAdd(&stat[set * DC_STAT_STRIDE + lane], lane == 0 ? n_valid : (lane == 1 ? n_kept : n_agree));
    }
}

extern "C" {

int hv_depth_consistency(hv_volume *v, const float *depth, const float *source_depths, int32_t n_sources, int32_t height, int32_t width,
                         const float *views, const float *back_views, const hv_consistency_params *params, float *depth_out,
                         uint8_t *counts_out, hv_consistency_stats *stats, int32_t loc) {
    HV_REQUIRE(v != nullptr && depth != nullptr && source_depths != nullptr && views != nullptr && back_views != nullptr && params != nullptr,
               HV_ERR_INVALID, "hv_depth_consistency: null argument");
    HV_REQUIRE(depth_out != nullptr || counts_out != nullptr, HV_ERR_INVALID, "hv_depth_consistency: no output asked for");
    HV_REQUIRE(height >= 1 && width >= 1 && height <= 32768 && width <= 32768 && (int64_t)height * width < (int64_t)1 << 30, HV_ERR_INVALID,
               "hv_depth_consistency: bad image size");
    HV_REQUIRE(n_sources >= 1 && n_sources <= MVS_MAX_VIEWS, HV_ERR_INVALID, "hv_depth_consistency: n_sources must be in 1..4");
    const hv_consistency_params P = *params;
    const int N = n_sources;
    for (int i = 0; i < 12 * N; ++i)
        HV_REQUIRE(std::isfinite(views[i]) && std::isfinite(back_views[i]), HV_ERR_INVALID, "hv_depth_consistency: a view matrix entry is not finite");
    HV_REQUIRE(std::isfinite(P.max_reproj_error) && P.max_reproj_error >= 0.0f, HV_ERR_INVALID,
               "hv_depth_consistency: max_reproj_error must be finite and not negative");
    HV_REQUIRE(std::isfinite(P.inv_depth_tol) && P.inv_depth_tol >= 0.0f && std::isfinite(P.rel_depth_tol) && P.rel_depth_tol >= 0.0f,
               HV_ERR_INVALID, "hv_depth_consistency: the depth tolerances must be finite and not negative");
    HV_REQUIRE(P.inv_depth_tol > 0.0f || P.rel_depth_tol > 0.0f, HV_ERR_INVALID, "hv_depth_consistency: one of the depth tolerances must be positive");
    HV_REQUIRE(P.min_consistent >= 0 && P.min_consistent <= N, HV_ERR_INVALID, "hv_depth_consistency: min_consistent must be in 0..n_sources");
    HV_REQUIRE(P.max_violations >= 0 && P.max_violations <= N, HV_ERR_INVALID, "hv_depth_consistency: max_violations must be in 0..n_sources");
    HV_HIP(hipSetDevice(v->device));
    const size_t npx = (size_t)height * (size_t)width;

    // head: the sets of three counters
    constexpr size_t stat_bytes = sizeof(unsigned long long) * DC_STAT_SETS * DC_STAT_STRIDE;
    HvStage st(v, loc);
    st.head(stats != nullptr ? stat_bytes : 0);
    const int i_depth = st.in(depth, sizeof(float) * npx), i_src = st.in(source_depths, sizeof(float) * npx * N);
    const int o_depth = st.out(depth_out, sizeof(float) * npx), o_counts = st.out(counts_out, 4 * npx);
    int rc = st.commit(&v->stage, &v->stage_bytes);
    if (rc != HV_OK) return rc;

    DcViews dv = {};
    dv.n = N;
    for (int k = 0; k < N; ++k) {
        dv.depth[k] = st.dev<const float>(i_src) + npx * k;
        for (int i = 0; i < 12; ++i) {
            dv.m[k][i] = views[12 * k + i];
            dv.back[k][i] = back_views[12 * k + i];
        }
    }
    const DcRule rule = {P.max_reproj_error * P.max_reproj_error, P.inv_depth_tol, P.rel_depth_tol, P.min_consistent, P.max_violations, P.fuse};
    unsigned long long *d_stat = (unsigned long long *)st.head_dev;
    if (d_stat != nullptr) HV_HIP(hipMemsetAsync(d_stat, 0, stat_bytes, v->stream));
    hv_profile_begin(v);
    hipLaunchKernelGGL(k_depth_consistency, dim3((unsigned)((width + DC_TILE_W - 1) / DC_TILE_W), (unsigned)((height + DC_TILE_H - 1) / DC_TILE_H)),
                       dim3(256), 0, v->stream, dv, rule, st.dev<const float>(i_depth), height, width, st.dev<float>(o_depth),
                       st.dev<uint32_t>(o_counts), d_stat);
    hv_profile_end(v, (int64_t)npx);
    HV_HIP(hipGetLastError());
    unsigned long long h[DC_STAT_SETS * DC_STAT_STRIDE] = {};
    rc = st.finish(stats != nullptr ? h : nullptr, sizeof h);  // (stats: waits for the stream, for either loc)
    if (rc != HV_OK) return rc;
    if (stats != nullptr) {
        int64_t sum[3] = {0, 0, 0};
        for (int k = 0; k < DC_STAT_SETS; ++k)
            for (int i = 0; i < 3; ++i) sum[i] += (int64_t)h[k * DC_STAT_STRIDE + i];
        *stats = hv_consistency_stats{sum[0], sum[1], sum[2]};
    }
    return HV_OK;
}

} // extern "C"
