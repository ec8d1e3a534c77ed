// libpyslam_hipvol.so — per-frame image preparation on the GPU: cv2.remap as pySLAM uses it for
// undistortion (pyslam/dense/volumetric_integrator_base.py:1017-1043): colour INTER_LINEAR, depth and
// label images INTER_NEAREST, float32 maps, BORDER_CONSTANT 0.
//
// OpenCV semantics restated (OpenCV is not available in this image: parity with cv2 is UNPINNED):
//   nearest : src(cvRound(map_y), cvRound(map_x)), cvRound = round-half-to-even
//   linear  : fixed-point bilinear, INTER_BITS = 5: sx = cvRound(map_x * 32), ix = sx >> 5, fx = sx & 31;
//             8-bit images use integer weights (32-fx)(32-fy)*32 ... summing to 2^15 and
//             (sum + 2^14) >> 15; float images use the same 1/32-quantised weights in float.
//
// ... and filter_shadow_points (pyslam/utilities/depth.py:103-146), the depth image's other per-keyframe preparation (below).
#include <algorithm>
#include <climits>

#include "hv_common.h"

enum { HV_IMG_U8 = 0, HV_IMG_F32 = 1, HV_IMG_I32 = 2 };

// cvRound of a map coordinate (nearest), or of 32 times it (linear): round-half-to-even.  A coordinate that is NaN or +-inf, or whose
// rounded value does not fit int32, is OUTSIDE the image: INT_MIN here, like x86's cvRound, so that neither it nor the tap next to
// it (ix + 1) can land in [0, W).  v_cvt_i32_f32 alone gives 0 for NaN: row / column 0 of the source.  Every finite value below
// 2^31 in magnitude rounds exactly as before.
__device__ __forceinline__ int hv_map_round(float v) { return fabsf(v) < 2147483648.0f ? __float2int_rn(v) : INT_MIN; }

template <typename T> __device__ __forceinline__ T px_or_zero(const T *src, int H, int W, int C, int y, int x, int c) {
    return (x >= 0 && x < W && y >= 0 && y < H) ? src[((int64_t)y * W + x) * C + c] : (T)0;
}

template <typename T>
__global__ __launch_bounds__(256) void k_remap_nearest(const T *__restrict__ src, int H, int W, int C,
                                                        const float *__restrict__ mx, const float *__restrict__ my,
                                                        T *__restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)H * W) return;
    const int sx = hv_map_round(mx[i]), sy = hv_map_round(my[i]);
    for (int c = 0; c < C; ++c) dst[i * C + c] = px_or_zero(src, H, W, C, sy, sx, c);
}

__global__ __launch_bounds__(256) void k_remap_linear_u8(const uint8_t *__restrict__ src, int H, int W, int C,
                                                          const float *__restrict__ mx, const float *__restrict__ my,
                                                          uint8_t *__restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)H * W) return;
    const int sx = hv_map_round(mx[i] * 32.0f), sy = hv_map_round(my[i] * 32.0f);
    const int ix = sx >> 5, iy = sy >> 5, fx = sx & 31, fy = sy & 31;
    const int w00 = (32 - fx) * (32 - fy) * 32, w01 = fx * (32 - fy) * 32, w10 = (32 - fx) * fy * 32, w11 = fx * fy * 32;
    for (int c = 0; c < C; ++c) {
        const int s = (int)px_or_zero(src, H, W, C, iy, ix, c) * w00 + (int)px_or_zero(src, H, W, C, iy, ix + 1, c) * w01 +
                      (int)px_or_zero(src, H, W, C, iy + 1, ix, c) * w10 + (int)px_or_zero(src, H, W, C, iy + 1, ix + 1, c) * w11;
        const int r = (s + (1 << 14)) >> 15;
        dst[i * C + c] = (uint8_t)(r < 0 ? 0 : (r > 255 ? 255 : r));
    }
}

__global__ __launch_bounds__(256) void k_remap_linear_f32(const float *__restrict__ src, int H, int W, int C,
                                                           const float *__restrict__ mx, const float *__restrict__ my,
                                                           float *__restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)H * W) return;
    const int sx = hv_map_round(mx[i] * 32.0f), sy = hv_map_round(my[i] * 32.0f);
    const int ix = sx >> 5, iy = sy >> 5;
    const float fx = (float)(sx & 31) * (1.0f / 32.0f), fy = (float)(sy & 31) * (1.0f / 32.0f);
    for (int c = 0; c < C; ++c) {
        dst[i * C + c] = px_or_zero(src, H, W, C, iy, ix, c) * ((1.0f - fx) * (1.0f - fy)) +
                         px_or_zero(src, H, W, C, iy, ix + 1, c) * (fx * (1.0f - fy)) +
                         px_or_zero(src, H, W, C, iy + 1, ix, c) * ((1.0f - fx) * fy) +
                         px_or_zero(src, H, W, C, iy + 1, ix + 1, c) * (fx * fy);
    }
}

// The reference's per-keyframe pair of remaps (colour INTER_LINEAR, depth INTER_NEAREST: volumetric_integrator_base.py:1017-1043) for
// a whole batch of device-resident frames in ONE launch: a thread owns an output pixel, reads its map entry once and samples every
// frame of the batch with it.  Depth keeps its storage type (float32, or the sensor's uint16: the nearest-neighbour pick commutes with
// the later conversion to metres), so a TUM-style keyframe stays 5 bytes per pixel on its way through the GPU.
template <typename D>
__global__ __launch_bounds__(256) void k_rectify_frames(const D *__restrict__ depth, const uint8_t *__restrict__ rgb, int n_frames, int H, int W,
                                                         const float *__restrict__ mx, const float *__restrict__ my,
                                                         D *__restrict__ depth_out, uint8_t *__restrict__ rgb_out) {
    const int64_t npx = (int64_t)H * W;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npx) return;
    const float fxm = mx[i], fym = my[i];
    const int nx = hv_map_round(fxm), ny = hv_map_round(fym);
    const int sx = hv_map_round(fxm * 32.0f), sy = hv_map_round(fym * 32.0f);
    const int ix = sx >> 5, iy = sy >> 5, fx = sx & 31, fy = sy & 31;
    const int w00 = (32 - fx) * (32 - fy) * 32, w01 = fx * (32 - fy) * 32, w10 = (32 - fx) * fy * 32, w11 = fx * fy * 32;
    for (int f = 0; f < n_frames; ++f) {
        const D *df = depth + (int64_t)f * npx;
        const uint8_t *cf = rgb + (int64_t)f * npx * 3;
        depth_out[(int64_t)f * npx + i] = px_or_zero(df, H, W, 1, ny, nx, 0);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int s = (int)px_or_zero(cf, H, W, 3, iy, ix, c) * w00 + (int)px_or_zero(cf, H, W, 3, iy, ix + 1, c) * w01 +
                          (int)px_or_zero(cf, H, W, 3, iy + 1, ix, c) * w10 + (int)px_or_zero(cf, H, W, 3, iy + 1, ix + 1, c) * w11;
            const int r = (s + (1 << 14)) >> 15;
            rgb_out[((int64_t)f * npx + i) * 3 + c] = (uint8_t)(r < 0 ? 0 : (r > 255 ? 255 : r));
        }
    }
}

// (hv_tsdf.hip: queued on `s`, nothing waits)
int hv_rectify_frames_device(hv_volume *v, hipStream_t s, const void *d_depth, int32_t depth_dtype, const uint8_t *d_rgb, int n_frames,
                             int height, int width, void *d_depth_out, uint8_t *d_rgb_out) {
    const int64_t npx = (int64_t)height * width;
    const dim3 grid((unsigned)((npx + 255) / 256)), block(256);
    if (depth_dtype == HV_DEPTH_U16)
        hipLaunchKernelGGL(k_rectify_frames<uint16_t>, grid, block, 0, s, (const uint16_t *)d_depth, d_rgb, n_frames, height, width,
                           (const float *)v->rect_map_x, (const float *)v->rect_map_y, (uint16_t *)d_depth_out, d_rgb_out);
    else
        hipLaunchKernelGGL(k_rectify_frames<float>, grid, block, 0, s, (const float *)d_depth, d_rgb, n_frames, height, width,
                           (const float *)v->rect_map_x, (const float *)v->rect_map_y, (float *)d_depth_out, d_rgb_out);
    HV_HIP(hipGetLastError());
    return HV_OK;
}

extern "C" int hv_tsdf_set_rectify_maps(hv_volume *v, const float *map_x, const float *map_y, int32_t height, int32_t width, int32_t loc) {
    HV_REQUIRE(v != nullptr, HV_ERR_INVALID, "hv_tsdf_set_rectify_maps: null volume");
    HV_REQUIRE(v->cfg.mode == HV_MODE_TSDF, HV_ERR_MODE, "hv_tsdf_set_rectify_maps: volume is not in TSDF mode");
    HV_HIP(hipSetDevice(v->device));
    if (v->stream_aux) HV_HIP(hipStreamSynchronize(v->stream_aux));
    HV_HIP(hipStreamSynchronize(v->stream));
    if (map_x == nullptr || map_y == nullptr) { // frames are fused as they come again
        v->rect_W = v->rect_H = 0;
        return HV_OK;
    }
    HV_REQUIRE(height > 0 && width > 0, HV_ERR_INVALID, "hv_tsdf_set_rectify_maps: bad image size");
    const size_t bytes = sizeof(float) * (size_t)height * width;
    void *mxb = v->rect_map_x, *myb = v->rect_map_y;
    int rc = hv_ensure_buffer(v, &mxb, &v->rect_map_x_bytes, bytes);
    if (rc != HV_OK) return rc;
    v->rect_map_x = (float *)mxb;
    rc = hv_ensure_buffer(v, &myb, &v->rect_map_y_bytes, bytes);
    if (rc != HV_OK) return rc;
    v->rect_map_y = (float *)myb;
    HV_HIP(hipMemcpy(v->rect_map_x, map_x, bytes, loc == HV_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    HV_HIP(hipMemcpy(v->rect_map_y, map_y, bytes, loc == HV_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    v->rect_W = width;
    v->rect_H = height;
    return HV_OK;
}

extern "C" int hv_remap(hv_volume *v, const void *src, int32_t src_kind, int32_t channels, int32_t height, int32_t width,
                        const float *map_x, const float *map_y, int32_t linear, void *dst, int32_t loc) {
    HV_REQUIRE(v != nullptr && src != nullptr && map_x != nullptr && map_y != nullptr && dst != nullptr, HV_ERR_INVALID,
               "hv_remap: null argument");
    HV_REQUIRE(height > 0 && width > 0 && channels >= 1 && channels <= 4, HV_ERR_INVALID, "hv_remap: bad image shape");
    HV_REQUIRE(src_kind == HV_IMG_U8 || src_kind == HV_IMG_F32 || src_kind == HV_IMG_I32, HV_ERR_INVALID,
               "hv_remap: unsupported image dtype");
    HV_REQUIRE(!(linear && src_kind == HV_IMG_I32), HV_ERR_INVALID, "hv_remap: label images are remapped with INTER_NEAREST");
    HV_HIP(hipSetDevice(v->device));
    const int64_t npx = (int64_t)height * width;
    const size_t esz = src_kind == HV_IMG_U8 ? 1 : 4;
    const size_t img_bytes = esz * channels * npx, map_bytes = sizeof(float) * npx;
    HvStage st(v, loc);
    const int i_mx = st.in(map_x, map_bytes), i_my = st.in(map_y, map_bytes), i_src = st.in(src, img_bytes), o_dst = st.out(dst, img_bytes);
    int rc = st.commit(&v->stage, &v->stage_bytes);
    if (rc != HV_OK) return rc;
    const void *d_src = st.dev<const void>(i_src);
    const float *d_mx = st.dev<const float>(i_mx), *d_my = st.dev<const float>(i_my);
    void *d_dst = st.dev<void>(o_dst);
    const dim3 grid((unsigned)((npx + 255) / 256)), block(256);
    if (!linear) {
        if (src_kind == HV_IMG_U8)
            hipLaunchKernelGGL(k_remap_nearest<uint8_t>, grid, block, 0, v->stream, (const uint8_t *)d_src, height, width, channels, d_mx, d_my, (uint8_t *)d_dst);
        else if (src_kind == HV_IMG_F32)
            hipLaunchKernelGGL(k_remap_nearest<float>, grid, block, 0, v->stream, (const float *)d_src, height, width, channels, d_mx, d_my, (float *)d_dst);
        else
            hipLaunchKernelGGL(k_remap_nearest<int32_t>, grid, block, 0, v->stream, (const int32_t *)d_src, height, width, channels, d_mx, d_my, (int32_t *)d_dst);
    } else if (src_kind == HV_IMG_U8) {
        hipLaunchKernelGGL(k_remap_linear_u8, grid, block, 0, v->stream, (const uint8_t *)d_src, height, width, channels, d_mx, d_my, (uint8_t *)d_dst);
    } else {
        hipLaunchKernelGGL(k_remap_linear_f32, grid, block, 0, v->stream, (const float *)d_src, height, width, channels, d_mx, d_my, (float *)d_dst);
    }
    HV_HIP(hipGetLastError());
    if ((rc = st.finish()) != HV_OK) return rc;
    HV_HIP(hipStreamSynchronize(v->stream)); // (device images too: this call has always been complete on return)
    return HV_OK;
}


// ---- filter_shadow_points (pyslam/utilities/depth.py:103-146) -----------------------------------
// |d(r,c) - d(r-dy,c)| and |d(r,c) - d(r,c-dx)|; threshold = 3 * 1.4826 * median(positive deltas)
// (float32 arithmetic, as numpy evaluates it for a float32 image); both endpoints of a large jump
// are replaced by fill_value.  The global median is an exact radix SELECT on the deltas' bit patterns (order-preserving for
// positive floats): three histogram passes over the image (12 + 12 + 8 bits), each followed by a one-workgroup pick of the
// bin(s) that hold the two middle ranks; the deltas are recomputed in every pass (two subtractions) instead of being stored,
// and the threshold stays in device memory for the mask kernel - no sort, no host round trip.  (Round 2: the deltas were
// written out, radix-sorted (19 launches) and the middle elements copied to the host - 0.33 ms of a 1.2 ms semantic keyframe,
// profiles/r03/kernel_stats_semantic.csv.)
// state words: [0] number of positive deltas, [1] [2] remaining ranks of the two middle elements, [3] [4] their key prefixes,
// [5] the threshold (float bits)
enum { HV_SH_N = 0, HV_SH_RANK0 = 1, HV_SH_RANK1 = 2, HV_SH_PRE0 = 3, HV_SH_PRE1 = 4, HV_SH_THR = 5, HV_SH_TICKET = 8 /* + pass */, HV_SH_WORDS = 16 };
static constexpr int HV_SH_BINS01 = 4096, HV_SH_BINS2 = 256;
static constexpr int HV_SH_GRID = 256; // workgroups of a histogram pass
static constexpr int HV_SH_HIST_WORDS = HV_SH_BINS01 + 2 * HV_SH_BINS01 + 2 * HV_SH_BINS2;

// one workgroup: the bin holding each of the two ranks, the rank inside it.  (Round 5 tried the pick as the tail of the histogram
// launch - run by its last workgroup to finish, the histogram read back with L2-level loads -: three launches less per keyframe and
// 18 us MORE, 69.6 us for the three passes against 51.5: the 4096 bypassing loads of one workgroup cost more than a 5 us launch.)
template <int PASS>
__device__ __forceinline__ void hv_shadow_pick(const uint32_t *__restrict__ hist, uint32_t *__restrict__ state) {
    constexpr int BINS = PASS == 2 ? HV_SH_BINS2 : HV_SH_BINS01;
    constexpr int PER = BINS / 256;
    constexpr int BITS = PASS == 2 ? 8 : 12;
    __shared__ uint32_t s_scan[256];
    __shared__ uint32_t s_rank[2];
    const int t = threadIdx.x;
    for (int target = 0; target < 2; ++target) {
        const uint32_t *h = hist + (PASS == 0 ? 0 : target * BINS);
        uint32_t local[PER], sum = 0u;
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            local[k] = h[t * PER + k];
            sum += local[k];
        }
        s_scan[t] = sum;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) { // Hillis-Steele inclusive scan
            const uint32_t addv = t >= off ? s_scan[t - off] : 0u;
            __syncthreads();
            s_scan[t] += addv;
            __syncthreads();
        }
        if (PASS == 0 && t == 0) {
            const uint32_t n = s_scan[255];
            if (target == 0) state[HV_SH_N] = n;
            s_rank[target] = n ? (target == 0 ? (n - 1u) / 2u : n / 2u) : 0u; // ranks of np.median's two middle elements
        }
        if (PASS > 0 && t == 0) s_rank[target] = state[HV_SH_RANK0 + target];
        __syncthreads();
        const uint32_t rank = s_rank[target];
        const uint32_t incl = s_scan[t];
        uint32_t before = incl - sum;
        if (rank >= before && rank < incl) { // exactly one thread when the rank exists
#pragma unroll
            for (int k = 0; k < PER; ++k) {
                if (rank < before + local[k]) {
                    const uint32_t prefix = PASS == 0 ? 0u : state[HV_SH_PRE0 + target];
                    state[HV_SH_PRE0 + target] = (prefix << BITS) | (uint32_t)(t * PER + k);
                    state[HV_SH_RANK0 + target] = rank - before;
                    break;
                }
                before += local[k];
            }
        }
        __syncthreads();
    }
    if (PASS == 2 && t == 0) {
        float thr = __uint_as_float(0x7fc00000u); // np.median of an empty array -> nan -> nothing is masked
        if (state[HV_SH_N]) {
            const float a = __uint_as_float(state[HV_SH_PRE0]), b = __uint_as_float(state[HV_SH_PRE1]);
            const float mad = state[HV_SH_PRE0] == state[HV_SH_PRE1] ? a : (a + b) * 0.5f; // np.median -> np.mean of the two middle float32
            const float sigma = 1.4826f * mad;
            thr = 3.0f * sigma;
        }
        state[HV_SH_THR] = __float_as_uint(thr);
    }
}

template <int PASS>
__global__ __launch_bounds__(256) void k_shadow_hist(const float *__restrict__ depth, int H, int W, int dx, int dy,
                                                      uint32_t *__restrict__ state, uint32_t *__restrict__ hist) {
    constexpr int BINS = PASS == 2 ? HV_SH_BINS2 : HV_SH_BINS01;
    constexpr int NB = (PASS == 0 ? 1 : 2) * BINS;
    __shared__ uint32_t s_h[NB];
    for (int i = threadIdx.x; i < NB; i += 256) s_h[i] = 0u;
    __syncthreads();
    const uint32_t p0 = PASS > 0 ? state[HV_SH_PRE0] : 0u, p1 = PASS > 0 ? state[HV_SH_PRE1] : 0u;
    auto add = [&](float v) {
        if (!(v > 0.0f)) return; // NaN compares false, like numpy's `delta_values > 0`
        const uint32_t key = __float_as_uint(v);
        if (PASS == 0) {
            atomicAdd(&s_h[key >> 20], 1u);
        } else if (PASS == 1) {
            if ((key >> 20) == p0) atomicAdd(&s_h[(key >> 8) & 0xfffu], 1u);
            if ((key >> 20) == p1) atomicAdd(&s_h[BINS + ((key >> 8) & 0xfffu)], 1u);
        } else {
            if ((key >> 8) == p0) atomicAdd(&s_h[key & 0xffu], 1u);
            if ((key >> 8) == p1) atomicAdd(&s_h[BINS + (key & 0xffu)], 1u);
        }
    };
    const int npx = H * W;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < npx; i += gridDim.x * 256) {
        const int r = i / W, c = i - r * W;
        const float d = depth[i];
        if (dy > 0 && r >= dy) add(fabsf(d - depth[i - dy * W]));
        if (dx > 0 && c >= dx) add(fabsf(d - depth[i - dx]));
    }
    __syncthreads();
    for (int i = threadIdx.x; i < NB; i += 256)
        if (s_h[i]) atomicAdd(&hist[i], s_h[i]);
}

template <int PASS>
__global__ __launch_bounds__(256) void k_shadow_pick(const uint32_t *__restrict__ hist, uint32_t *__restrict__ state) {
    hv_shadow_pick<PASS>(hist, state);
}

__global__ __launch_bounds__(256) void k_shadow_mask(const float *__restrict__ depth, int H, int W, int dx, int dy,
                                                      const uint32_t *__restrict__ state, float fill, float *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)H * W) return;
    const float thr = __uint_as_float(state[HV_SH_THR]);
    const int r = (int)(i / W), c = (int)(i % W);
    const float d = depth[i];
    bool m = false;
    if (dy > 0) {
        if (r >= dy) m |= fabsf(d - depth[i - (int64_t)dy * W]) > thr;
        if (r + dy < H) m |= fabsf(depth[i + (int64_t)dy * W] - d) > thr;
    }
    if (dx > 0) {
        if (c >= dx) m |= fabsf(d - depth[i - dx]) > thr;
        if (c + dx < W) m |= fabsf(depth[i + dx] - d) > thr;
    }
    out[i] = m ? fill : d;
}

extern "C" {

// the seven launches of the filter on `st`: head = [histograms][state] (zeroed here), dd -> d_out (device images)
static int shadow_filter_launch(const float *dd, int32_t height, int32_t width, int32_t delta_x, int32_t delta_y, float fill_value,
                                float *d_out, uint32_t *head, hipStream_t st) {
    const int64_t npx = (int64_t)height * width;
    uint32_t *hist0 = head, *hist1 = hist0 + HV_SH_BINS01, *hist2 = hist1 + 2 * HV_SH_BINS01;
    uint32_t *state = hist0 + HV_SH_HIST_WORDS;
    HV_HIP(hipMemsetAsync(hist0, 0, sizeof(uint32_t) * (HV_SH_HIST_WORDS + HV_SH_WORDS), st));
    // one workgroup per CU (1024 measured the same, round 6: the passes are bound by the LDS atomics of a few dozen hot bins)
    const unsigned hist_grid = (unsigned)std::min<int64_t>((npx + 255) / 256, HV_SH_GRID);
    hipLaunchKernelGGL(k_shadow_hist<0>, dim3(hist_grid), dim3(256), 0, st, dd, height, width, delta_x, delta_y, state, hist0);
    hipLaunchKernelGGL(k_shadow_pick<0>, dim3(1), dim3(256), 0, st, hist0, state);
    hipLaunchKernelGGL(k_shadow_hist<1>, dim3(hist_grid), dim3(256), 0, st, dd, height, width, delta_x, delta_y, state, hist1);
    hipLaunchKernelGGL(k_shadow_pick<1>, dim3(1), dim3(256), 0, st, hist1, state);
    hipLaunchKernelGGL(k_shadow_hist<2>, dim3(hist_grid), dim3(256), 0, st, dd, height, width, delta_x, delta_y, state, hist2);
    hipLaunchKernelGGL(k_shadow_pick<2>, dim3(1), dim3(256), 0, st, hist2, state);
    hipLaunchKernelGGL(k_shadow_mask, dim3((unsigned)((npx + 255) / 256)), dim3(256), 0, st, dd, height, width, delta_x, delta_y, state, fill_value, d_out);
    HV_HIP(hipGetLastError());
    return HV_OK;
}

int hv_filter_shadow_points(hv_volume *v, const float *depth, int32_t height, int32_t width, int32_t delta_x,
                            int32_t delta_y, float fill_value, float *out, int32_t loc) {
    HV_REQUIRE(v != nullptr && depth != nullptr && out != nullptr, HV_ERR_INVALID, "hv_filter_shadow_points: null argument");
    HV_REQUIRE(height > 0 && width > 0 && delta_x >= 0 && delta_y >= 0 && delta_x < width && delta_y < height,
               HV_ERR_INVALID, "hv_filter_shadow_points: bad image size or deltas");
    HV_HIP(hipSetDevice(v->device));
    const int64_t npx = (int64_t)height * width;
    HV_REQUIRE(npx < (int64_t)1 << 30, HV_ERR_INVALID, "hv_filter_shadow_points: image too large");
    // head: [histograms][state]
    HvStage st(v, loc);
    st.head(sizeof(uint32_t) * (HV_SH_HIST_WORDS + HV_SH_WORDS));
    const int i_depth = st.in(depth, sizeof(float) * npx), o_out = st.out(out, sizeof(float) * npx);
    int rc = st.commit(&v->stage, &v->stage_bytes);
    if (rc != HV_OK) return rc;
    rc = shadow_filter_launch(st.dev<const float>(i_depth), height, width, delta_x, delta_y, fill_value, st.dev<float>(o_out), (uint32_t *)st.head_dev,
                              v->stream);
    if (rc != HV_OK) return rc;
    // host images: copied back and complete on return; device images: queued on the volume's stream like every other launch
    return st.finish();
}

int hv_filter_shadow_points_on_stream(hv_volume *v, const float *depth, int32_t height, int32_t width, int32_t delta_x,
                                      int32_t delta_y, float fill_value, float *out, void *stream) {
    HV_REQUIRE(v != nullptr && depth != nullptr && out != nullptr, HV_ERR_INVALID, "hv_filter_shadow_points_on_stream: null argument");
    HV_REQUIRE(height > 0 && width > 0 && delta_x >= 0 && delta_y >= 0 && delta_x < width && delta_y < height,
               HV_ERR_INVALID, "hv_filter_shadow_points_on_stream: bad image size or deltas");
    HV_REQUIRE((int64_t)height * width < (int64_t)1 << 30, HV_ERR_INVALID, "hv_filter_shadow_points_on_stream: image too large");
    HV_HIP(hipSetDevice(v->device));
    // the filter touches nothing of the volume: it may run beside the volume's own launches (a keyframe's depth is filtered on the
    // upload side while the previous keyframe is fused).  Histograms and state of its own, four sets used in turn.
    constexpr int SETS = 4;
    const size_t head = sizeof(uint32_t) * (HV_SH_HIST_WORDS + HV_SH_WORDS);
    if (v->shadow_ring == nullptr) HV_HIP(hipMalloc(&v->shadow_ring, head * SETS));
    uint32_t *scratch = (uint32_t *)((char *)v->shadow_ring + head * (size_t)v->shadow_ring_next);
    v->shadow_ring_next = (v->shadow_ring_next + 1) % SETS;
    return shadow_filter_launch(depth, height, width, delta_x, delta_y, fill_value, out, scratch, (hipStream_t)stream);
}

} // extern "C"
