// libpyslam_hipvol.so — hv_stereo_sgm: census semi-global stereo matching, rectified uint8 pair -> int16 disparity in sixteenths
// and float32 metric depth.  The rules (grey, 9x7 census, Hamming cost, 4 or 8 paths, winner, uniqueness, left-right check,
// sub-pixel, depth) are stated in include/hipvol.h and restated in numpy in tests/stereo_reference.py, which this file is held to
// bit for bit.  Integer arithmetic only before the depth division.
//
// Four stages on the volume's stream:
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

#include "hv_common.h"

static constexpr int ST_INF = 1 << 20;  // an absent L: larger than any L + P2, small enough to add penalties to
static constexpr int ST_TILE_W = 32, ST_TILE_H = 8, ST_RX = 4, ST_RY = 3;

__device__ __forceinline__ int st_grey(const uint8_t *__restrict__ img, int C, int64_t i) {
    if (C == 1) return img[i];
    const uint8_t *p = img + 3 * i;
    return ((int)p[0] + 2 * (int)p[1] + (int)p[2] + 2) >> 2;
}

__global__ __launch_bounds__(256) void k_stereo_census(const uint8_t *__restrict__ left, const uint8_t *__restrict__ right, int H, int W,
                                                        int C, uint64_t *__restrict__ census_l, uint64_t *__restrict__ census_r) {
    constexpr int TW = ST_TILE_W + 2 * ST_RX, TH = ST_TILE_H + 2 * ST_RY;
    __shared__ uint8_t tile[TH][TW];
    const uint8_t *img = blockIdx.z ? right : left;
    uint64_t *out = blockIdx.z ? census_r : census_l;
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

// min over the wave, the same value in every lane's copy (scalar).  Every lane of the wave must be active.
__device__ __forceinline__ int st_wave_min(int v) {
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xF, 0xF, false));   // quad_perm [1,0,3,2]
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xF, 0xF, false));   // quad_perm [2,3,0,1]
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x141, 0xF, 0xF, false));  // row_half_mirror: the other quad of each 8
    v = min(v, __builtin_amdgcn_update_dpp(v, v, 0x140, 0xF, 0xF, false));  // row_mirror: the other half of each 16
    return min(min(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
               min(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}

template <int N> struct alignas(2 * N) StPack {
    uint16_t v[N];
};

// what one step of a path reads from memory: the left census word, the right ones of the lane's disparities, the lane's part of S
template <int VPL> struct StFetch {
    uint64_t cl;
    uint64_t cr[VPL];
    StPack<VPL> s;
};

template <int VPL>
__device__ __forceinline__ void st_fetch(StFetch<VPL> &f, const uint64_t *__restrict__ census_l, const uint64_t *__restrict__ census_r,
                                         const uint16_t *S, int W, int D, int x, int y, int d0, bool read_s) {
    const int64_t p = (int64_t)y * W + x;
    f.cl = census_l[p];
#pragma unroll
    for (int j = 0; j < VPL; ++j) f.cr[j] = x - (d0 + j) >= 0 ? census_r[p - (d0 + j)] : 0;  // p - d stays inside row y
    if (read_s && d0 < D) f.s = *(const StPack<VPL> *)(S + p * D + d0);
}

// One direction (dx, dy) of rule 4.  Wave w of the launch walks the path that starts at the w-th pixel whose predecessor lies outside
// the image: with dx != 0 the H pixels of the column x0 the direction leaves from, with dy != 0 the pixels of row y0 (without column
// x0 when it is counted already).  Lane l holds the disparities l VPL .. l VPL + VPL - 1; D is a multiple of VPL, so a lane is
// either wholly inside [0, D) or wholly outside (its L stays ST_INF and it writes nothing).
template <int VPL>
__global__ __launch_bounds__(256) void k_stereo_path(const uint64_t *__restrict__ census_l, const uint64_t *__restrict__ census_r, int H,
                                                      int W, int D, int dx, int dy, int p1, int p2, int first, uint16_t *S) {
    const int lane = threadIdx.x & 63;
    const int start = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    const int n_side = dx != 0 ? H : 0;
    const int n_total = n_side + (dy != 0 ? (dx != 0 ? W - 1 : W) : 0);
    if (start >= n_total) return;
    int x, y;
    if (start < n_side) {
        x = dx > 0 ? 0 : W - 1;
        y = start;
    } else {
        const int k = start - n_side;
        y = dy > 0 ? 0 : H - 1;
        x = dx > 0 ? k + 1 : k;  // dx > 0: column 0 is counted above; dx < 0: column W-1 is; dx == 0: every column
    }
    const int d0 = lane * VPL;
    const bool active = d0 < D;
    int Lq[VPL];
    bool has_q = false;
    StFetch<VPL> cur, nxt;
    st_fetch<VPL>(cur, census_l, census_r, S, W, D, x, y, d0, !first);
    for (;;) {
        const int xn = x + dx, yn = y + dy;
        const bool more = xn >= 0 && xn < W && yn >= 0 && yn < H;  // the same in every lane
        if (more) st_fetch<VPL>(nxt, census_l, census_r, S, W, D, xn, yn, d0, !first);  // in flight while this pixel is worked out
        int L[VPL];
#pragma unroll
        for (int j = 0; j < VPL; ++j) L[j] = x - (d0 + j) >= 0 ? __popcll(cur.cl ^ cur.cr[j]) : 64;
        if (has_q) {
            int m = Lq[0];
#pragma unroll
            for (int j = 1; j < VPL; ++j) m = min(m, Lq[j]);
            const int M = st_wave_min(m);
            int below = __shfl_up(Lq[VPL - 1], 1, 64), above = __shfl_down(Lq[0], 1, 64);
            if (lane == 0) below = ST_INF;   // d - 1 < 0: absent
            if (lane == 63) above = ST_INF;  // d + 1 >= 64 VPL >= D: absent (below that, the lane above holds ST_INF)
#pragma unroll
            for (int j = 0; j < VPL; ++j) {
                const int lo = j == 0 ? below : Lq[j - 1], hi = j == VPL - 1 ? above : Lq[j + 1];
                L[j] += min(min(Lq[j], lo + p1), min(hi + p1, M + p2)) - M;
            }
        }
#pragma unroll
        for (int j = 0; j < VPL; ++j) Lq[j] = active ? L[j] : ST_INF;
        has_q = true;
        if (active) {
            StPack<VPL> s;
#pragma unroll
            for (int j = 0; j < VPL; ++j) s.v[j] = (uint16_t)(first ? L[j] : (int)cur.s.v[j] + L[j]);
            *(StPack<VPL> *)(S + ((int64_t)y * W + x) * D + d0) = s;
        }
        if (!more) break;
        cur = nxt;
        x = xn;
        y = yn;
    }
}

// min over each row of 16 lanes, in every lane of the row.  Every lane of the wave must be active.
__device__ __forceinline__ uint32_t st_row16_min(uint32_t v) {
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0xB1, 0xF, 0xF, false));
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x4E, 0xF, 0xF, false));
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x141, 0xF, 0xF, false));
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x140, 0xF, 0xF, false));
    return v;
}

static constexpr int ST_WIN_TILE = 256;       // left pixels of one row per workgroup
static constexpr uint32_t ST_NO_KEY = ~0u;    // a right pixel nothing has voted for yet

// Rules 5 and 6 for the left image and rule 7's right disparity.  A workgroup takes ST_WIN_TILE consecutive pixels of one row; 16
// lanes share a pixel, lane j of them reads the disparities j, j + 16, ...: S is read in whole rows.  A value is ranked by the key
// (S << 8) | d, whose minimum is the smallest S and among equals the smallest d.  The same keys vote for the right image: S(y,x,d)
// belongs to the right pixel x - d, whose minimum is kept in LDS for the tile's span of right pixels and merged into r_keys
// (set to ST_NO_KEY beforehand) with one atomic per right pixel and tile.  d_left = d*, or -1 where d* is not unique.
__global__ __launch_bounds__(256) void k_stereo_winner(const uint16_t *__restrict__ S, int W, int D, int uniqueness,
                                                        int16_t *__restrict__ d_left, uint32_t *__restrict__ r_keys) {
    __shared__ uint32_t votes[ST_WIN_TILE + 256];  // right pixels x0 - (D - 1) .. x0 + ST_WIN_TILE - 1
    const int y = blockIdx.y, x0 = blockIdx.x * ST_WIN_TILE, r0 = x0 - (D - 1);
    for (int k = threadIdx.x; k < ST_WIN_TILE + 256; k += 256) votes[k] = ST_NO_KEY;
    __syncthreads();
    const int j = threadIdx.x & 15, group = threadIdx.x >> 4;
    const int scale = 100 - uniqueness;
    for (int it = 0; it < 16; ++it) {
        const int x = x0 + group * 16 + it;  // the four pixels of a wave lie 16 apart: their votes go to different right pixels
        const bool ok = x < W;
        const uint16_t *row = S + ((int64_t)y * W + (ok ? x : 0)) * D;
        uint32_t best = ST_NO_KEY;
        if (ok)
            for (int d = j; d < D; d += 16) {
                const uint32_t key = ((uint32_t)row[d] << 8) | (uint32_t)d;
                best = min(best, key);
                if (x - d >= 0) atomicMin(&votes[x - d - r0], key);
            }
        best = st_row16_min(best);
        const int bd = (int)(best & 0xffu), bound = (int)(best >> 8) * 100;
        uint32_t clear = 1;  // 0: this lane saw a rival
        if (ok)
            for (int d = j; d < D; d += 16)
                if ((d < bd - 1 || d > bd + 1) && (int)row[d] * scale < bound) clear = 0;
        clear = st_row16_min(clear);
        if (ok && j == 0) d_left[(int64_t)y * W + x] = (int16_t)(clear ? bd : -1);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < ST_WIN_TILE + D - 1; k += 256) {
        const int xr = r0 + k;
        if (xr >= 0 && xr < W && votes[k] != ST_NO_KEY) atomicMin(&r_keys[(int64_t)y * W + xr], votes[k]);
    }
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
    int d16 = -16;
    if (valid) {
        d16 = 16 * d;
        if (d > 0 && d < D - 1) {
            const uint16_t *s = S + i * D + d;
            const int sm = s[-1], s0 = s[0], sp = s[1];
            const int den = max(sm + sp - 2 * s0, 1);
            d16 += ((sm - sp) * 16 + den) / (2 * den);  // C division: toward zero
        }
    }
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

template <int VPL>
static void st_launch_path(hipStream_t s, const uint64_t *cl, const uint64_t *cr, int H, int W, int D, int dx, int dy, int p1, int p2,
                           int first, uint16_t *S) {
    const int n = (dx != 0 ? H : 0) + (dy != 0 ? (dx != 0 ? W - 1 : W) : 0);
    if (n <= 0) return;  // (a diagonal of a one-column image: the H starts of the side are all there is, n = H)
    hipLaunchKernelGGL(k_stereo_path<VPL>, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, cl, cr, H, W, D, dx, dy, p1, p2, first, S);
}

static size_t st_align(size_t n) { return (n + 255) & ~(size_t)255; }

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
    const size_t want = s_bytes + 2 * c_bytes + d_bytes + r_bytes + x_bytes;
    if (v->stereo_buf == nullptr || v->stereo_buf_bytes < want) {
        if (v->stereo_buf != nullptr) {
            HV_HIP(hipStreamSynchronize(v->stream));
            HV_HIP(hipFree(v->stereo_buf));
            v->stereo_buf = nullptr;
            v->stereo_buf_bytes = 0;
        }
        if (hipMalloc(&v->stereo_buf, want) != hipSuccess) {
            (void)hipGetLastError();
            v->stereo_buf = nullptr;
            hv_set_error("hv_stereo_sgm: cannot allocate %zu bytes of scratch (%d x %d, %d disparities)", want, height, width, D);
            return HV_ERR_CAPACITY;
        }
        v->stereo_buf_bytes = want;
    }
    char *base = (char *)v->stereo_buf;
    uint16_t *S = (uint16_t *)base;
    uint64_t *cl = (uint64_t *)(base + s_bytes), *cr = (uint64_t *)(base + s_bytes + c_bytes);
    int16_t *dl = (int16_t *)(base + s_bytes + 2 * c_bytes);
    uint32_t *rk = (uint32_t *)(base + s_bytes + 2 * c_bytes + d_bytes);

    HvStage st(v, loc);
    if (speckle_window > 0 && stats != nullptr) st.head(sizeof(unsigned long long) * 5);
    const int i_left = st.in(left, (size_t)npx * channels), i_right = st.in(right, (size_t)npx * channels);
    const int o_disp = st.out(disparity_out, sizeof(int16_t) * npx), o_depth = st.out(depth_out, sizeof(float) * npx);
    int rc = st.commit(&v->stage, &v->stage_bytes);
    if (rc != HV_OK) return rc;

    hipStream_t s = v->stream;
    hv_profile_begin(v);
    hipLaunchKernelGGL(k_stereo_census, dim3((unsigned)((width + ST_TILE_W - 1) / ST_TILE_W), (unsigned)((height + ST_TILE_H - 1) / ST_TILE_H), 2),
                       dim3(256), 0, s, st.dev<const uint8_t>(i_left), st.dev<const uint8_t>(i_right), height, width, channels, cl, cr);
    hv_profile_end(v, 0);
    // q -> p steps: the four axis directions, then the four diagonals (the order of tests/stereo_reference.py; the sum does not
    // depend on it)
    static const int dirs[8][2] = {{1, 0}, {-1, 0}, {0, 1}, {0, -1}, {1, 1}, {-1, -1}, {1, -1}, {-1, 1}};
    hv_profile_begin(v);
    for (int k = 0; k < P.paths; ++k) {
        const int dx = dirs[k][0], dy = dirs[k][1], first = k == 0;
        if (D <= 64)
            st_launch_path<1>(s, cl, cr, height, width, D, dx, dy, P.p1, P.p2, first, S);
        else if (D <= 128)
            st_launch_path<2>(s, cl, cr, height, width, D, dx, dy, P.p1, P.p2, first, S);
        else
            st_launch_path<4>(s, cl, cr, height, width, D, dx, dy, P.p1, P.p2, first, S);
    }
    hv_profile_end(v, 0);
    const unsigned px_grid = (unsigned)((npx + 255) / 256);
    hv_profile_begin(v);
    HV_HIP(hipMemsetAsync(rk, 0xff, sizeof(uint32_t) * npx, s));  // ST_NO_KEY
    hipLaunchKernelGGL(k_stereo_winner, dim3((unsigned)((width + ST_WIN_TILE - 1) / ST_WIN_TILE), (unsigned)height), dim3(256), 0, s, S, width, D,
                       P.uniqueness_ratio, dl, rk);
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
