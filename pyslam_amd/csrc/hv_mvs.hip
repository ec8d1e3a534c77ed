// libpyslam_hipvol.so — hv_mvs_sgm: plane-sweep depth for a posed reference image and 1..4 source views.  Fronto-parallel planes at
// evenly spaced inverse depths in the reference camera, each reference pixel looked up in the source views through the per-view 3x4
// matrix, census Hamming cost, then the semi-global stages of hv_stereo_sgm.  The rules M1 - M10 are stated in include/hipvol.h and
// restated in numpy in tests/mvs_reference.py, which this file is held to bit for bit.
//
// Stages on the volume's stream (census, paths and winner are the kernels of hv_sgm.h, shared with hv_stereo_sgm):
//   census   the reference and the source images in one launch
//   cost     k_mvs_cost: the uint8 volume C[(y W + x) D + k].  A lane takes 4 consecutive planes of one pixel and stores one dword, so
//            a wave writes 256 consecutive bytes of C; a = A p is computed once per lane and view, and the census words that the four
//            planes gather lie on neighbouring source pixels (the projections of one reference pixel move along the epipolar line)
//   paths    k_sgm_path with the cost read from C, VPL bytes per lane and step
//   winner   k_sgm_winner without the right image's votes
//   finish   k_mvs_finish: rule M6 (the views that see the winner, by the device function the cost kernel uses), M7 and M9
#include <algorithm>
#include <cmath>

#include "hv_mvs_project.h"  // rule M3: mvs_ray, mvs_source_pixel
#include "hv_sgm.h"

struct MvsViews {
    float m[MVS_MAX_VIEWS][12];  // [A | b] of each view, row-major 3x4
    const uint64_t *census[MVS_MAX_VIEWS];
    int n;
};

// Rule M2: the inverse depth of index k16 (in sixteenths of a plane; plane k is k16 = 16 k): one multiply, one add
__device__ __forceinline__ float mvs_inverse_depth(float w0, float step16, int k16) { return w0 + (float)k16 * step16; }

// Rule M4 for the planes k0 .. k0 + 3 of one pixel per lane.
__global__ __launch_bounds__(256) void k_mvs_cost(const MvsViews views, const uint64_t *__restrict__ census_ref, int H, int W, int D, float w0,
                                                   float step16, int min_views, uint32_t *__restrict__ C4) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int per_px = D >> 2;
    const int64_t p = t / per_px;
    if (p >= (int64_t)H * W) return;
    const int k0 = (int)(t - p * per_px) * 4;
    const int x = (int)(p % W), y = (int)(p / W);
    const uint64_t cref = census_ref[p];
    int sum[4] = {0, 0, 0, 0}, n[4] = {0, 0, 0, 0};
    for (int s = 0; s < views.n; ++s) {
        const float *m = views.m[s];
        float a[3];
        mvs_ray(m, x, y, a);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int q = mvs_source_pixel(a, m, mvs_inverse_depth(w0, step16, 16 * (k0 + j)), H, W);
            if (q >= 0) {
                sum[j] += __popcll(cref ^ views.census[s][q]);
                n[j] += 1;
            }
        }
    }
    uint32_t packed = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = n[j] >= min_views ? (2 * sum[j] + n[j]) / (2 * n[j]) : 64;  // (min_views >= 1: n = 0 never divides)
        packed |= (uint32_t)c << (8 * j);
    }
    C4[t] = packed;  // t = (p D + k0) / 4
}

// Rules M6, M7 and M9.
__global__ __launch_bounds__(256) void k_mvs_finish(const MvsViews views, const uint16_t *__restrict__ S, const int16_t *__restrict__ d_left, int H,
                                                     int W, int D, float w0, float step16, int min_views, int16_t *__restrict__ index,
                                                     float *__restrict__ depth) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)H * W) return;
    const int k = d_left[i];
    bool valid = k >= 0;
    if (valid) {
        const int x = (int)(i % W), y = (int)(i / W);
        const float w = mvs_inverse_depth(w0, step16, 16 * k);
        int n = 0;
        for (int s = 0; s < views.n; ++s) {
            float a[3];
            mvs_ray(views.m[s], x, y, a);
            n += mvs_source_pixel(a, views.m[s], w, H, W) >= 0;
        }
        valid = n >= min_views;
    }
    const int k16 = valid ? st_subpixel16(S + i * D, k, D) : -16;
    if (index != nullptr) index[i] = (int16_t)k16;
    if (depth != nullptr) {
        float z = 0.0f;
        if (valid) {
            const float wv = mvs_inverse_depth(w0, step16, k16);
            if (!(wv <= 0.0f)) z = 1.0f / wv;
        }
        depth[i] = z;
    }
}

extern "C" {

int hv_mvs_sgm(hv_volume *v, const uint8_t *ref, const uint8_t *sources, int32_t n_sources, int32_t height, int32_t width, int32_t channels,
               const float *views, const hv_mvs_params *params, int16_t *index_out, float *depth_out, hv_speckle_stats *stats, int32_t loc) {
    HV_REQUIRE(v != nullptr && ref != nullptr && sources != nullptr && views != nullptr && params != nullptr, HV_ERR_INVALID,
               "hv_mvs_sgm: null argument");
    HV_REQUIRE(index_out != nullptr || depth_out != nullptr, HV_ERR_INVALID, "hv_mvs_sgm: no output asked for");
    HV_REQUIRE(channels == 1 || channels == 3, HV_ERR_INVALID, "hv_mvs_sgm: channels must be 1 or 3");
    HV_REQUIRE(height >= 1 && width >= 1 && height <= 32768 && width <= 32768 && (int64_t)height * width < (int64_t)1 << 30, HV_ERR_INVALID,
               "hv_mvs_sgm: bad image size");
    HV_REQUIRE(n_sources >= 1 && n_sources <= MVS_MAX_VIEWS, HV_ERR_INVALID, "hv_mvs_sgm: n_sources must be in 1..4");
    const hv_mvs_params P = *params;
    const int D = P.num_planes, N = n_sources;
    HV_REQUIRE(P.min_views >= 1 && P.min_views <= N, HV_ERR_INVALID, "hv_mvs_sgm: min_views must be in 1..n_sources");
    HV_REQUIRE(D >= 16 && D <= 256 && D % 16 == 0, HV_ERR_INVALID, "hv_mvs_sgm: num_planes must be a multiple of 16 in 16..256");
    HV_REQUIRE(P.p1 > 0 && P.p1 <= P.p2 && P.p2 <= 1023, HV_ERR_INVALID, "hv_mvs_sgm: need 0 < p1 <= p2 <= 1023");
    HV_REQUIRE(P.uniqueness_ratio >= 0 && P.uniqueness_ratio <= 99, HV_ERR_INVALID, "hv_mvs_sgm: uniqueness_ratio must be in 0..99");
    HV_REQUIRE(P.paths == 4 || P.paths == 8, HV_ERR_INVALID, "hv_mvs_sgm: paths must be 4 or 8");
    HV_REQUIRE(std::isfinite(P.min_depth) && P.min_depth > 0.0, HV_ERR_INVALID, "hv_mvs_sgm: min_depth must be finite and positive");
    HV_REQUIRE(P.max_depth > P.min_depth, HV_ERR_INVALID, "hv_mvs_sgm: need max_depth > min_depth");  // (false for a NaN)
    for (int i = 0; i < 12 * N; ++i) HV_REQUIRE(std::isfinite(views[i]), HV_ERR_INVALID, "hv_mvs_sgm: a view matrix entry is not finite");
    HV_REQUIRE(P.speckle_window_size >= 0 && P.speckle_window_size <= 1 << 30, HV_ERR_INVALID,
               "hv_mvs_sgm: speckle_window_size must be in 0..2^30");
    HV_REQUIRE(P.speckle_window_size == 0 || (P.speckle_range >= 0 && P.speckle_range <= 4095), HV_ERR_INVALID,
               "hv_mvs_sgm: speckle_range must be in 0..4095");
    // rule M2, in double with exactly these operations, rounded once
    const double inv_far = std::isinf(P.max_depth) ? 0.0 : 1.0 / P.max_depth;
    const float w0 = (float)inv_far;
    const float step16 = (float)((1.0 / P.min_depth - inv_far) / (16.0 * (double)(D - 1)));
    HV_REQUIRE(std::isfinite(step16), HV_ERR_INVALID, "hv_mvs_sgm: min_depth is too small: the plane step overflows float32");
    HV_HIP(hipSetDevice(v->device));
    const int64_t npx = (int64_t)height * width;
    const int window = P.speckle_window_size;
    // scratch of the handle: [S npx D u16][C npx D u8][census of the reference and the N sources, npx u64 each][winners npx i16]
    const size_t s_bytes = st_align((size_t)npx * D * 2), v_bytes = st_align((size_t)npx * D), c_bytes = st_align((size_t)npx * 8),
                 d_bytes = st_align((size_t)npx * 2);
    const size_t x_bytes = window > 0 && index_out == nullptr ? d_bytes : 0;
    int rc = st_scratch(v, s_bytes + v_bytes + (size_t)(1 + N) * c_bytes + d_bytes + x_bytes, "hv_mvs_sgm", height, width, D);
    if (rc != HV_OK) return rc;
    char *base = (char *)v->stereo_buf;
    uint16_t *S = (uint16_t *)base;
    uint8_t *C = (uint8_t *)(base + s_bytes);
    char *census = base + s_bytes + v_bytes;
    int16_t *dl = (int16_t *)(census + (size_t)(1 + N) * c_bytes);

    HvStage st(v, loc);
    if (window > 0 && stats != nullptr) st.head(sizeof(unsigned long long) * 5);
    const size_t img_bytes = (size_t)npx * channels;
    const int i_ref = st.in(ref, img_bytes), i_src = st.in(sources, img_bytes * N);
    const int o_index = st.out(index_out, sizeof(int16_t) * npx), o_depth = st.out(depth_out, sizeof(float) * npx);
    rc = st.commit(&v->stage, &v->stage_bytes);
    if (rc != HV_OK) return rc;

    hipStream_t s = v->stream;
    StCensusList list = {};
    MvsViews mv = {};
    mv.n = N;
    list.img[0] = st.dev<const uint8_t>(i_ref);
    list.out[0] = (uint64_t *)census;
    for (int k = 0; k < N; ++k) {
        list.img[1 + k] = st.dev<const uint8_t>(i_src) + img_bytes * k;
        list.out[1 + k] = (uint64_t *)(census + (size_t)(1 + k) * c_bytes);
        mv.census[k] = list.out[1 + k];
        for (int i = 0; i < 12; ++i) mv.m[k][i] = views[12 * k + i];
    }
    hv_profile_begin(v);
    st_launch_census(s, list, 1 + N, height, width, channels);
    hv_profile_end(v, 0);
    hv_profile_begin(v);
    hipLaunchKernelGGL(k_mvs_cost, dim3((unsigned)((npx * (D / 4) + 255) / 256)), dim3(256), 0, s, mv, (const uint64_t *)census, height, width, D, w0,
                       step16, P.min_views, (uint32_t *)C);
    hv_profile_end(v, 0);
    hv_profile_begin(v);
    st_launch_paths(s, StCostVolume{C}, height, width, D, P.paths, P.p1, P.p2, S);
    hv_profile_end(v, 0);
    hv_profile_begin(v);
    st_launch_winner<false>(s, S, height, width, D, P.uniqueness_ratio, dl, nullptr);
    hv_profile_end(v, 0);
    hv_profile_begin(v);
    // (the filter needs the index on the device: in scratch of the handle when the caller asks for depth alone)
    int16_t *index = st.dev<int16_t>(o_index);
    if (window > 0 && index == nullptr) index = (int16_t *)((char *)dl + d_bytes);
    hipLaunchKernelGGL(k_mvs_finish, dim3((unsigned)((npx + 255) / 256)), dim3(256), 0, s, mv, S, dl, height, width, D, w0, step16, P.min_views, index,
                       st.dev<float>(o_depth));
    hv_profile_end(v, npx);
    HV_HIP(hipGetLastError());
    if (window <= 0) return st.finish();
    // rule M8, exactly as hv_stereo_sgm_speckle does it: in place on the device, the depth zeroed where a pixel went
    rc = hv_speckle_launch(v, "hv_mvs_sgm", index, HV_SPECKLE_I16, height, width, -16.0, window, 16.0 * P.speckle_range, index, st.dev<float>(o_depth),
                           nullptr, (unsigned long long *)st.head_dev);
    if (rc != HV_OK) return rc;
    unsigned long long h[5] = {0, 0, 0, 0, 0};
    rc = st.finish(stats != nullptr ? h : nullptr, sizeof h);  // (stats: waits for the stream, for either loc)
    if (rc != HV_OK) return rc;
    if (stats != nullptr) *stats = hv_speckle_stats{(int64_t)h[0], (int64_t)h[1], (int64_t)h[2], (int64_t)h[3], (int64_t)h[4]};
    return HV_OK;
}

} // extern "C"
