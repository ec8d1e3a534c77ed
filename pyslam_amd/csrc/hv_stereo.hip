// libpyslam_hipvol.so — hv_stereo_sgm: census semi-global stereo matching, rectified uint8 pair -> int16 disparity in sixteenths
// and float32 metric depth.  The rules (grey, 9x7 census, Hamming cost, 4 or 8 paths, winner, uniqueness, left-right check,
// sub-pixel, depth) are stated in include/hipvol.h and restated in numpy in tests/stereo_reference.py, which this file is held to
// bit for bit.  Integer arithmetic only before the depth division.
//
// Four stages on the volume's stream (the first three live in hv_sgm.h, shared with hv_mvs_sgm):
//   census   both images in one launch, the grey conversion fused in: a 32x8 tile and its halo staged through LDS
//   paths    one launch per direction, one wave per scan line / column / diagonal start.  The lanes hold the D values of L(q,.)
//            in registers (VPL = 1, 2 or 4 consecutive disparities per lane), M(q) is a DPP reduction inside the rows of 16 lanes
//            and three scalar minima across them, d-1 / d+1 come from the neighbouring lane.  The cost is recomputed from the two
//            census images (8 B per pixel); S is a uint16 volume that the first direction writes and the others add to
//   winner   16 lanes per pixel: the smallest best d, the uniqueness rule, and the right image's disparity from the same read of S
//            (votes in LDS per tile of a row, merged with one atomic per right pixel and tile)
//   finish   left-right check, sub-pixel step, disparity and depth out
#include <algorithm>
#include <cmath>

#include "hv_sgm.h"

// Rules 1 and 2.  blockIdx.z picks the image of the list.
__global__ __launch_bounds__(256) void k_sgm_census(const StCensusList list, int H, int W, int C) {
    constexpr int TW = ST_TILE_W + 2 * ST_RX, TH = ST_TILE_H + 2 * ST_RY;
    __shared__ uint8_t tile[TH][TW];
    const uint8_t *__restrict__ img = list.img[blockIdx.z];
    uint64_t *__restrict__ out = list.out[blockIdx.z];
    const int x0 = blockIdx.x * ST_TILE_W, y0 = blockIdx.y * ST_TILE_H;
    for (int k = threadIdx.x; k < TW * TH; k += 256) {
        const int ty = k / TW, tx = k % TW;
        const int yy = min(max(y0 + ty - ST_RY, 0), H - 1), xx = min(max(x0 + tx - ST_RX, 0), W - 1);  // replicate
        tile[ty][tx] = (uint8_t)st_grey(img, C, (int64_t)yy * W + xx);
    }
    __syncthreads();
    const int lx = threadIdx.x % ST_TILE_W, ly = threadIdx.x / ST_TILE_W;
    const int x = x0 + lx, y = y0 + ly;
    if (x >= W || y >= H) return;
    const int c = tile[ly + ST_RY][lx + ST_RX];
    uint64_t bits = 0;
#pragma unroll
    for (int dy = -ST_RY; dy <= ST_RY; ++dy)
#pragma unroll
        for (int dx = -ST_RX; dx <= ST_RX; ++dx) {
            if (dy == 0 && dx == 0) continue;
            bits = (bits << 1) | (uint64_t)((int)tile[ly + ST_RY + dy][lx + ST_RX + dx] < c);
        }
    out[(int64_t)y * W + x] = bits;
}

void st_launch_census(hipStream_t s, const StCensusList &list, int n, int H, int W, int C) {
    hipLaunchKernelGGL(k_sgm_census, dim3((unsigned)((W + ST_TILE_W - 1) / ST_TILE_W), (unsigned)((H + ST_TILE_H - 1) / ST_TILE_H), (unsigned)n),
                       dim3(256), 0, s, list, H, W, C);
}

int st_scratch(hv_volume *v, size_t want, const char *fn, int height, int width, int D) {
    if (v->stereo_buf != nullptr && v->stereo_buf_bytes >= want) return HV_OK;
    if (v->stereo_buf != nullptr) {
        HV_HIP(hipStreamSynchronize(v->stream));
        HV_HIP(hipFree(v->stereo_buf));
        v->stereo_buf = nullptr;
        v->stereo_buf_bytes = 0;
    }
    if (hipMalloc(&v->stereo_buf, want) != hipSuccess) {
        (void)hipGetLastError();
        v->stereo_buf = nullptr;
        hv_set_error("%s: cannot allocate %zu bytes of scratch (%d x %d, %d disparities)", fn, want, height, width, D);
        return HV_ERR_CAPACITY;
    }
    v->stereo_buf_bytes = want;
    return HV_OK;
}

// Rules 7 to 10.
__global__ __launch_bounds__(256) void k_stereo_finish(const uint16_t *__restrict__ S, const int16_t *__restrict__ d_left,
                                                        const uint32_t *__restrict__ r_keys, int H, int W, int D, int max_diff, float bf,
                                                        float min_depth, float max_depth, int16_t *__restrict__ disparity,
                                                        float *__restrict__ depth) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)H * W) return;
    const int x = (int)(i % W);
    const int d = d_left[i];
    bool valid = d >= 0;
    if (valid && max_diff >= 0) {
        valid = x - d >= 0;
        if (valid) {
            const int diff = (int)(r_keys[i - d] & 0xffu) - d;  // (the left pixel itself voted for it: never ST_NO_KEY)
            valid = (diff < 0 ? -diff : diff) <= max_diff;
        }
    }
    const int d16 = valid ? st_subpixel16(S + i * D, d, D) : -16;
    if (disparity != nullptr) disparity[i] = (int16_t)d16;
    if (depth != nullptr) {
        float z = 0.0f;
        if (d16 > 0) {
            z = (bf * 16.0f) / (float)d16;
            if (z < min_depth || (max_depth < INFINITY && z > max_depth)) z = 0.0f;
        }
        depth[i] = z;
    }
}

// The body of both entry points.  speckle_window 0: hv_stereo_sgm, launch for launch.  Positive: the disparity of rule 9 is filtered
// where it lies on the device (hv_speckle_launch, in place) and rule 10's depth is zeroed where a pixel went.
static int st_run(hv_volume *v, const uint8_t *left, const uint8_t *right, int32_t height, int32_t width, int32_t channels,
                  const hv_stereo_params *params, int32_t speckle_window, int32_t speckle_range, int16_t *disparity_out, float *depth_out,
                  hv_speckle_stats *stats, int32_t loc) {
    HV_REQUIRE(v != nullptr && left != nullptr && right != nullptr && params != nullptr, HV_ERR_INVALID, "hv_stereo_sgm: null argument");
    HV_REQUIRE(disparity_out != nullptr || depth_out != nullptr, HV_ERR_INVALID, "hv_stereo_sgm: no output asked for");
    HV_REQUIRE(channels == 1 || channels == 3, HV_ERR_INVALID, "hv_stereo_sgm: channels must be 1 or 3");
    HV_REQUIRE(height >= 1 && width >= 1 && height <= 32768 && width <= 32768 && (int64_t)height * width < (int64_t)1 << 30, HV_ERR_INVALID,
               "hv_stereo_sgm: bad image size");
    const hv_stereo_params P = *params;
    const int D = P.num_disparities;
    HV_REQUIRE(D >= 16 && D <= 256 && D % 16 == 0, HV_ERR_INVALID, "hv_stereo_sgm: num_disparities must be a multiple of 16 in 16..256");
    HV_REQUIRE(P.p1 > 0 && P.p1 <= P.p2 && P.p2 <= 1023, HV_ERR_INVALID, "hv_stereo_sgm: need 0 < p1 <= p2 <= 1023");
    HV_REQUIRE(P.uniqueness_ratio >= 0 && P.uniqueness_ratio <= 99, HV_ERR_INVALID, "hv_stereo_sgm: uniqueness_ratio must be in 0..99");
    HV_REQUIRE(P.paths == 4 || P.paths == 8, HV_ERR_INVALID, "hv_stereo_sgm: paths must be 4 or 8");
    HV_REQUIRE(depth_out == nullptr || (std::isfinite(P.bf) && P.bf > 0.0f), HV_ERR_INVALID,
               "hv_stereo_sgm: bf must be finite and positive when depth is asked for");
    HV_HIP(hipSetDevice(v->device));
    const int64_t npx = (int64_t)height * width;
    // scratch of the handle: [S npx D u16][census left npx u64][census right npx u64][d_left npx i16][right keys npx u32]
    const size_t s_bytes = st_align((size_t)npx * D * 2), c_bytes = st_align((size_t)npx * 8), d_bytes = st_align((size_t)npx * 2),
                 r_bytes = st_align((size_t)npx * 4);
    const size_t x_bytes = speckle_window > 0 && disparity_out == nullptr ? d_bytes : 0;
    int rc = st_scratch(v, s_bytes + 2 * c_bytes + d_bytes + r_bytes + x_bytes, "hv_stereo_sgm", height, width, D);
    if (rc != HV_OK) return rc;
    char *base = (char *)v->stereo_buf;
    uint16_t *S = (uint16_t *)base;
    uint64_t *cl = (uint64_t *)(base + s_bytes), *cr = (uint64_t *)(base + s_bytes + c_bytes);
    int16_t *dl = (int16_t *)(base + s_bytes + 2 * c_bytes);
    uint32_t *rk = (uint32_t *)(base + s_bytes + 2 * c_bytes + d_bytes);

    HvStage st(v, loc);
    if (speckle_window > 0 && stats != nullptr) st.head(sizeof(unsigned long long) * 5);
    const int i_left = st.in(left, (size_t)npx * channels), i_right = st.in(right, (size_t)npx * channels);
    const int o_disp = st.out(disparity_out, sizeof(int16_t) * npx), o_depth = st.out(depth_out, sizeof(float) * npx);
    rc = st.commit(&v->stage, &v->stage_bytes);
    if (rc != HV_OK) return rc;

    hipStream_t s = v->stream;
    hv_profile_begin(v);
    StCensusList list = {};
    list.img[0] = st.dev<const uint8_t>(i_left), list.img[1] = st.dev<const uint8_t>(i_right);
    list.out[0] = cl, list.out[1] = cr;
    st_launch_census(s, list, 2, height, width, channels);
    hv_profile_end(v, 0);
    hv_profile_begin(v);
    st_launch_paths(s, StCostCensus{cl, cr}, height, width, D, P.paths, P.p1, P.p2, S);
    hv_profile_end(v, 0);
    const unsigned px_grid = (unsigned)((npx + 255) / 256);
    hv_profile_begin(v);
    HV_HIP(hipMemsetAsync(rk, 0xff, sizeof(uint32_t) * npx, s));  // ST_NO_KEY
    st_launch_winner<true>(s, S, height, width, D, P.uniqueness_ratio, dl, rk);
    hv_profile_end(v, 0);
    hv_profile_begin(v);
    // (the filter needs rule 9's disparity on the device: in scratch of the handle when the caller asks for depth alone)
    int16_t *disp = st.dev<int16_t>(o_disp);
    if (speckle_window > 0 && disp == nullptr) disp = (int16_t *)(base + s_bytes + 2 * c_bytes + d_bytes + r_bytes);
    hipLaunchKernelGGL(k_stereo_finish, dim3(px_grid), dim3(256), 0, s, S, dl, rk, height, width, D, P.max_diff, P.bf, P.min_depth, P.max_depth,
                       disp, st.dev<float>(o_depth));
    hv_profile_end(v, npx);
    HV_HIP(hipGetLastError());
    // host images: copied back and complete on return; device images: queued on the volume's stream like every other launch
    if (speckle_window <= 0) return st.finish();
    rc = hv_speckle_launch(v, "hv_stereo_sgm_speckle", disp, HV_SPECKLE_I16, height, width, -16.0, speckle_window, 16.0 * speckle_range, disp,
                           st.dev<float>(o_depth), nullptr, (unsigned long long *)st.head_dev);
    if (rc != HV_OK) return rc;
    unsigned long long h[5] = {0, 0, 0, 0, 0};
    rc = st.finish(stats != nullptr ? h : nullptr, sizeof h);  // (stats: waits for the stream, for either loc)
    if (rc != HV_OK) return rc;
    if (stats != nullptr) *stats = hv_speckle_stats{(int64_t)h[0], (int64_t)h[1], (int64_t)h[2], (int64_t)h[3], (int64_t)h[4]};
    return HV_OK;
}

extern "C" {

int hv_stereo_sgm(hv_volume *v, const uint8_t *left, const uint8_t *right, int32_t height, int32_t width, int32_t channels,
                  const hv_stereo_params *params, int16_t *disparity_out, float *depth_out, int32_t loc) {
    return st_run(v, left, right, height, width, channels, params, 0, 0, disparity_out, depth_out, nullptr, loc);
}

int hv_stereo_sgm_speckle(hv_volume *v, const uint8_t *left, const uint8_t *right, int32_t height, int32_t width, int32_t channels,
                          const hv_stereo_params *params, int32_t speckle_window_size, int32_t speckle_range, int16_t *disparity_out,
                          float *depth_out, hv_speckle_stats *stats, int32_t loc) {
    HV_REQUIRE(speckle_window_size >= 1 && speckle_window_size <= 1 << 30, HV_ERR_INVALID,
               "hv_stereo_sgm_speckle: speckle_window_size must be in 1..2^30 (hv_stereo_sgm is the call without the filter)");
    HV_REQUIRE(speckle_range >= 0 && speckle_range <= 4095, HV_ERR_INVALID, "hv_stereo_sgm_speckle: speckle_range must be in 0..4095");
    return st_run(v, left, right, height, width, channels, params, speckle_window_size, speckle_range, disparity_out, depth_out, stats, loc);
}

} // extern "C"
