// libpyslam_hipvol.so — hv_orb_detect and hv_match_descriptors: oriented binary keypoints and their Hamming matching.  The rules
// (F1 - F11, M1 - M5) are stated in include/hipvol.h and restated in numpy in tests/orb_reference.py, which this file is held to bit
// for bit.  Integer arithmetic only.
//
// hv_orb_detect, on the volume's stream:
//   grey / down  rule F1 at level 0, rule F2 for every further level that yields keypoints
//   fast         per level: a 32x8 tile and its 3-pixel halo in LDS; the two 16-bit ring masks, the 9-contiguous test as shift-and-AND
//                on the mask doubled to 32 bits, the score V as a uint16 map (F3, F4)
//   select       one wave per 32x32 cell: the cell's V and a 1-pixel halo in LDS, 16 pixels per lane, non-maximum suppression (F5),
//                then per_cell rounds of a wave-wide max over the key V << 10 | (1023 - local index) (F6): no sort, no atomic
//   scan         the cells' counts of all levels -> their first output row (F7) and the total
//   describe     one wave per (cell, rank): the 31x31 patch in LDS, the disc moments through a wave reduction (F8), the 5x5 box sums
//                of the patch (F9), then each lane evaluates bits k, k + 64, k + 128, k + 192 and four ballots give the 32 bytes (F11)
// hv_match_descriptors:
//   best         each lane holds one query in 8 registers; a tile of 128 train descriptors sits in LDS and is read at a wave-uniform
//                address; 8 xor and 8 popcounts per pair; (d1, j1, d2) stay in registers; a segment is a pair of loop bounds (M1, M2)
//   owner        the same kernel with the roles swapped and one segment: for every train descriptor the smallest query index attaining
//                its minimum (M4) - independent of the order of execution
//   accept       M3, M4, M5: the index or -1, and one integer atomic per wave for the segment's count
#include <algorithm>

#define HV_ORB_TABLE static __device__ const
#include "orb_pattern.h"

#include "hv_sgm.h"

static constexpr int ORB_BORDER = 16, ORB_CELL = 32, ORB_MIN_SIDE = 33, ORB_MAX_LEVELS = 8;
static constexpr int ORB_PATCH = 31, ORB_BOX = 27;  // the disc of radius 15; the box-sum centres of radius 13

// the levels that yield keypoints (F2), and where each one's pixels and cells start in the arrays that hold all levels
struct OrbLevels {
    int n;
    int H[ORB_MAX_LEVELS], W[ORB_MAX_LEVELS], cells_x[ORB_MAX_LEVELS];
    int cell_base[ORB_MAX_LEVELS + 1];
    int64_t px_base[ORB_MAX_LEVELS + 1];
};

static OrbLevels orb_levels(int H, int W, int levels) {
    OrbLevels L = {};
    L.cell_base[0] = 0, L.px_base[0] = 0;
    for (int l = 0; l < levels && H >= ORB_MIN_SIDE && W >= ORB_MIN_SIDE; ++l) {
        L.H[l] = H, L.W[l] = W, L.cells_x[l] = (W + ORB_CELL - 1) / ORB_CELL;
        L.cell_base[l + 1] = L.cell_base[l] + L.cells_x[l] * ((H + ORB_CELL - 1) / ORB_CELL);
        L.px_base[l + 1] = L.px_base[l] + (int64_t)st_align((size_t)H * W);
        L.n = l + 1;
        H /= 2, W /= 2;
    }
    return L;
}

__device__ __forceinline__ int orb_wave_max(int v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = max(v, __shfl_xor(v, off));
    return v;
}
__device__ __forceinline__ int orb_wave_sum(int v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// F1
__global__ __launch_bounds__(256) void k_orb_grey(const uint8_t *__restrict__ img, int C, int64_t npx, uint8_t *__restrict__ g) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npx; i += (int64_t)gridDim.x * 256) g[i] = (uint8_t)st_grey(img, C, i);
}

// F2: dst [Hd,Wd] from src of width Ws
__global__ __launch_bounds__(256) void k_orb_down(const uint8_t *__restrict__ src, int Ws, uint8_t *__restrict__ dst, int Hd, int Wd) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= Wd || y >= Hd) return;
    const uint8_t *p = src + (int64_t)(2 * y) * Ws + 2 * x;
    dst[(int64_t)y * Wd + x] = (uint8_t)(((int)p[0] + (int)p[1] + (int)p[Ws] + (int)p[Ws + 1] + 2) >> 2);
}

// at least 9 circularly contiguous bits of the 16-bit mask
__device__ __forceinline__ bool orb_arc9(uint32_t m) {
    const uint32_t m2 = m | (m << 16);
    uint32_t r = m2 & (m2 >> 1);  // runs of 2
    r &= r >> 2;                  // 4
    r &= r >> 4;                  // 8
    r &= m2 >> 8;                 // 9
    return (r & 0xffffu) != 0;
}

// F3, F4: V [H,W], 0 for a non-corner and outside the candidate region
__global__ __launch_bounds__(256) void k_orb_fast(const uint8_t *__restrict__ g, int H, int W, int t, uint16_t *__restrict__ V) {
    constexpr int TW = 32 + 6, TH = 8 + 6;
    __shared__ uint8_t tile[TH][TW + 2];
    const int x0 = blockIdx.x * 32, y0 = blockIdx.y * 8;
    for (int k = threadIdx.x; k < TW * TH; k += 256) {
        const int ty = k / TW, tx = k % TW;
        const int yy = min(max(y0 + ty - 3, 0), H - 1), xx = min(max(x0 + tx - 3, 0), W - 1);  // (never a candidate's ring: in bounds only)
        tile[ty][tx] = g[(int64_t)yy * W + xx];
    }
    __syncthreads();
    const int lx = threadIdx.x & 31, ly = threadIdx.x >> 5;
    const int x = x0 + lx, y = y0 + ly;
    if (x >= W || y >= H) return;
    int v = 0;
    if (x >= ORB_BORDER && x < W - ORB_BORDER && y >= ORB_BORDER && y < H - ORB_BORDER) {
        constexpr int RX[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
        constexpr int RY[16] = {-3, -3, -2, -1, 0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3};
        const int c = tile[ly + 3][lx + 3];
        uint32_t bm = 0, dm = 0;
        int bs = 0, ds = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int d = (int)tile[ly + 3 + RY[i]][lx + 3 + RX[i]] - c;
            if (d > t) bm |= 1u << i, bs += d - t;
            if (-d > t) dm |= 1u << i, ds += -d - t;
        }
        if (orb_arc9(bm) || orb_arc9(dm)) v = max(bs, ds);
    }
    V[(int64_t)y * W + x] = (uint16_t)v;
}

// F5, F6: one wave per cell.  kp [cells][per_cell][3] = x, y, V in rank order; cnt [cells]
__global__ __launch_bounds__(64) void k_orb_select(const uint16_t *__restrict__ V, int H, int W, int cells_x, int per_cell, int cell_base,
                                                   int32_t *__restrict__ cnt, int32_t *__restrict__ kp) {
    constexpr int T = ORB_CELL + 2;
    __shared__ uint16_t tile[T][T];
    const int lane = threadIdx.x;
    const int cx0 = (blockIdx.x % cells_x) * ORB_CELL, cy0 = (blockIdx.x / cells_x) * ORB_CELL;
    for (int k = lane; k < T * T; k += 64) {
        const int ty = k / T, tx = k % T;
        const int gy = cy0 + ty - 1, gx = cx0 + tx - 1;
        tile[ty][tx] = (gy >= 0 && gy < H && gx >= 0 && gx < W) ? V[(int64_t)gy * W + gx] : (uint16_t)0;
    }
    __syncthreads();
    int key[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int local = lane + 64 * k, ly = (local >> 5) + 1, lx = (local & 31) + 1;
        const int v = tile[ly][lx];
        bool keep = v > 0;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                if (dy == 0 && dx == 0) continue;
                const int n = tile[ly + dy][lx + dx];
                const bool later = dy > 0 || (dy == 0 && dx > 0);
                keep = keep && (v > n || (later && v == n));
            }
        key[k] = keep ? (v << 10 | (1023 - local)) : 0;
    }
    const int cell = cell_base + blockIdx.x;
    int n = 0;
    for (; n < per_cell; ++n) {
        int m = 0;
#pragma unroll
        for (int k = 0; k < 16; ++k) m = max(m, key[k]);
        m = orb_wave_max(m);
        if (m == 0) break;
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (key[k] == m) key[k] = 0;
        if (lane == 0) {
            const int local = 1023 - (m & 1023);
            int32_t *o = kp + ((int64_t)cell * per_cell + n) * 3;
            o[0] = cx0 + (local & 31), o[1] = cy0 + (local >> 5), o[2] = m >> 10;
        }
    }
    if (lane == 0) cnt[cell] = n;
}

// F7: off[c] = the counts before cell c; total[0] = their sum.  One workgroup.
__global__ __launch_bounds__(256) void k_orb_scan(const int32_t *__restrict__ cnt, int n, int32_t *__restrict__ off, int32_t *__restrict__ total) {
    __shared__ int sh[256];
    __shared__ int carry;
    const int tid = threadIdx.x;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < n; base += 256) {
        const int i = base + tid;
        const int v = i < n ? cnt[i] : 0;
        sh[tid] = v;
        __syncthreads();
        for (int d = 1; d < 256; d <<= 1) {
            const int add = tid >= d ? sh[tid - d] : 0;
            __syncthreads();
            sh[tid] += add;
            __syncthreads();
        }
        const int incl = sh[tid], c = carry;
        if (i < n) off[i] = c + incl - v;
        __syncthreads();
        if (tid == 255) carry = c + incl;
        __syncthreads();
    }
    if (tid == 0) total[0] = carry;
}

// F8 - F11: one wave per (cell, rank)
__global__ __launch_bounds__(64) void k_orb_describe(const uint8_t *__restrict__ pyr, const OrbLevels L, int per_cell, const int32_t *__restrict__ cnt,
                                                     const int32_t *__restrict__ off, const int32_t *__restrict__ kp,
                                                     int32_t *__restrict__ keypoints, uint8_t *__restrict__ descriptors) {
    __shared__ uint8_t patch[ORB_PATCH][ORB_PATCH + 1];
    __shared__ uint16_t hs[ORB_PATCH][ORB_BOX + 1];
    __shared__ uint16_t box[ORB_BOX][ORB_BOX + 1];
    const int lane = threadIdx.x;
    const int cell = blockIdx.x / per_cell, rank = blockIdx.x % per_cell;
    if (rank >= cnt[cell]) return;  // (the same for the whole wave)
    int level = 0;
    while (level + 1 < L.n && cell >= L.cell_base[level + 1]) ++level;
    const int32_t *k3 = kp + (int64_t)blockIdx.x * 3;
    const int x = k3[0], y = k3[1], score = k3[2];
    const int W = L.W[level];
    const uint8_t *g = pyr + L.px_base[level];
    int m10 = 0, m01 = 0;
    for (int k = lane; k < ORB_PATCH * ORB_PATCH; k += 64) {
        const int py = k / ORB_PATCH, px = k % ORB_PATCH;
        const int gv = g[(int64_t)(y - 15 + py) * W + (x - 15 + px)];
        patch[py][px] = (uint8_t)gv;
        const int dx = px - 15, dy = py - 15;
        if (dx * dx + dy * dy <= 225) m10 += dx * gv, m01 += dy * gv;
    }
    m10 = orb_wave_sum(m10), m01 = orb_wave_sum(m01);
    int bin = 0;
    int64_t best = (int64_t)m10 * hv_orb_cx[0] + (int64_t)m01 * hv_orb_cy[0];
    for (int b = 1; b < 32; ++b) {
        const int64_t sc = (int64_t)m10 * hv_orb_cx[b] + (int64_t)m01 * hv_orb_cy[b];
        if (sc > best) best = sc, bin = b;  // (strictly: the smallest bin of a tie stays)
    }
    __syncthreads();
    for (int k = lane; k < ORB_PATCH * ORB_BOX; k += 64) {
        const int r = k / ORB_BOX, c = k % ORB_BOX;
        hs[r][c] = (uint16_t)((int)patch[r][c] + patch[r][c + 1] + patch[r][c + 2] + patch[r][c + 3] + patch[r][c + 4]);
    }
    __syncthreads();
    for (int k = lane; k < ORB_BOX * ORB_BOX; k += 64) {
        const int r = k / ORB_BOX, c = k % ORB_BOX;
        box[r][c] = (uint16_t)((int)hs[r][c] + hs[r + 1][c] + hs[r + 2][c] + hs[r + 3][c] + hs[r + 4][c]);  // s(y + r - 13, x + c - 13)
    }
    __syncthreads();
    unsigned long long bal[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int8_t *p = hv_orb_pattern_rotated[bin][lane + 64 * j];
        bal[j] = __ballot(box[13 + p[1]][13 + p[0]] < box[13 + p[3]][13 + p[2]]);
    }
    const int64_t o = (int64_t)off[cell] + rank;
    if (lane < 32) {
        const int w = lane >> 3;
        const unsigned long long word = w == 0 ? bal[0] : w == 1 ? bal[1] : w == 2 ? bal[2] : bal[3];
        descriptors[o * 32 + lane] = (uint8_t)(word >> (8 * (lane & 7)));
    } else if (lane < 37) {
        const int f = lane - 32;
        keypoints[o * 5 + f] = f == 0 ? x : f == 1 ? y : f == 2 ? level : f == 3 ? score : bin;
    }
}

// M1, M2 for segment s = blockIdx.x / nblk and 256 queries.  offsets == nullptr: one segment, all of t.  Descriptors 4-byte aligned.
template <bool WITH_D>
__global__ __launch_bounds__(256) void k_hamming_best(const uint32_t *__restrict__ q, int nq, const uint32_t *__restrict__ t, int nt,
                                                      const int32_t *__restrict__ offsets, int nblk, int32_t *__restrict__ j1_out,
                                                      uint16_t *__restrict__ d1_out, uint16_t *__restrict__ d2_out) {
    constexpr int TILE = 128;
    __shared__ uint32_t tile[TILE][8];
    uint32_t *flat = &tile[0][0];
    const int s = blockIdx.x / nblk, i = (blockIdx.x % nblk) * 256 + threadIdx.x;
    const int lo = offsets != nullptr ? offsets[s] : 0, hi = offsets != nullptr ? offsets[s + 1] : nt;
    uint32_t qw[8];
#pragma unroll
    for (int w = 0; w < 8; ++w) qw[w] = i < nq ? q[(int64_t)i * 8 + w] : 0u;
    int d1 = 65535, d2 = 65535, j1 = -1;
    for (int base = lo; base < hi; base += TILE) {
        const int n = min(TILE, hi - base);
        __syncthreads();
        for (int k = threadIdx.x; k < n * 8; k += 256) flat[k] = t[(int64_t)base * 8 + k];
        __syncthreads();
        for (int j = 0; j < n; ++j) {
            int d = 0;
#pragma unroll
            for (int w = 0; w < 8; ++w) d += __popc(qw[w] ^ tile[j][w]);
            if (d < d1) {
                d2 = d1, d1 = d, j1 = base + j;
            } else if (d < d2) {
                d2 = d;
            }
        }
    }
    if (i >= nq) return;
    const int64_t o = (int64_t)s * nq + i;
    j1_out[o] = j1;
    if (WITH_D) d1_out[o] = (uint16_t)d1, d2_out[o] = (uint16_t)d2;
}

// M3 - M5: index holds j1 on entry
__global__ __launch_bounds__(256) void k_match_accept(int32_t *__restrict__ index, const uint16_t *__restrict__ d1, const uint16_t *__restrict__ d2,
                                                      const int32_t *__restrict__ owner, int nq, int nblk, int max_distance, int ratio_percent,
                                                      int cross_check, int32_t *__restrict__ counts) {
    const int s = blockIdx.x / nblk, i = (blockIdx.x % nblk) * 256 + threadIdx.x;
    bool ok = false;
    if (i < nq) {
        const int64_t o = (int64_t)s * nq + i;
        const int j1 = index[o], a = d1[o], b = d2[o];
        ok = j1 >= 0 && a <= max_distance && (ratio_percent == 0 || 100 * a < ratio_percent * b);
        if (ok && cross_check) ok = owner[j1] == i;
        index[o] = ok ? j1 : -1;
    }
    const int n = __popcll(__ballot(ok));
    if (counts != nullptr && n > 0 && (threadIdx.x & 63) == 0) atomicAdd(counts + s, n);
}

extern "C" {

int hv_orb_detect(hv_volume *v, const uint8_t *image, int32_t height, int32_t width, int32_t channels, const hv_feature_params *params,
                  int32_t *keypoints_out, uint8_t *descriptors_out, int64_t capacity, int32_t *count_out, int32_t loc) {
    HV_REQUIRE(v != nullptr && image != nullptr && params != nullptr && keypoints_out != nullptr && descriptors_out != nullptr && count_out != nullptr,
               HV_ERR_INVALID, "hv_orb_detect: null argument");
    HV_REQUIRE(channels == 1 || channels == 3, HV_ERR_INVALID, "hv_orb_detect: channels must be 1 or 3");
    HV_REQUIRE(height >= 1 && width >= 1 && height <= 32768 && width <= 32768, HV_ERR_INVALID, "hv_orb_detect: bad image size");
    const hv_feature_params P = *params;
    HV_REQUIRE(P.levels >= 1 && P.levels <= ORB_MAX_LEVELS, HV_ERR_INVALID, "hv_orb_detect: levels must be in 1..8");
    HV_REQUIRE(P.threshold >= 1 && P.threshold <= 254, HV_ERR_INVALID, "hv_orb_detect: threshold must be in 1..254");
    HV_REQUIRE(P.per_cell >= 1 && P.per_cell <= 16, HV_ERR_INVALID, "hv_orb_detect: per_cell must be in 1..16");
    const OrbLevels L = orb_levels(height, width, P.levels);
    const int cells = L.cell_base[L.n];
    const int64_t bound = (int64_t)cells * P.per_cell;
    HV_REQUIRE(capacity >= bound, HV_ERR_INVALID, "hv_orb_detect: the outputs hold %lld keypoints, the bound is %lld", (long long)capacity,
               (long long)bound);
    if (L.n == 0) {  // F2: no level yields anything
        *count_out = 0;
        return HV_OK;
    }
    HV_HIP(hipSetDevice(v->device));
    // scratch of the handle: [grey pyramid u8][V u16, the same layout][cell counts i32][cell offsets i32][x, y, V per (cell, rank) i32]
    const size_t pyr_bytes = (size_t)L.px_base[L.n], v_bytes = 2 * pyr_bytes, c_bytes = st_align(sizeof(int32_t) * cells),
                 k_bytes = st_align(sizeof(int32_t) * 3 * (size_t)bound);
    int rc = hv_ensure_buffer(v, &v->stereo_buf, &v->stereo_buf_bytes, pyr_bytes + v_bytes + 2 * c_bytes + k_bytes);
    if (rc != HV_OK) return rc;
    uint8_t *pyr = (uint8_t *)v->stereo_buf;
    uint16_t *V = (uint16_t *)(pyr + pyr_bytes);
    int32_t *cnt = (int32_t *)(pyr + pyr_bytes + v_bytes), *off = (int32_t *)(pyr + pyr_bytes + v_bytes + c_bytes);
    int32_t *kp = (int32_t *)(pyr + pyr_bytes + v_bytes + 2 * c_bytes);

    const int64_t npx = (int64_t)height * width;
    HvStage st(v, loc);
    st.head(sizeof(int32_t));
    const int i_img = st.in(image, (size_t)npx * channels);
    const int o_kp = st.out(keypoints_out, sizeof(int32_t) * 5 * (size_t)bound, sizeof(int32_t) * 5);
    const int o_desc = st.out(descriptors_out, (size_t)32 * bound, 32);
    rc = st.commit(&v->stage, &v->stage_bytes);
    if (rc != HV_OK) return rc;

    hipStream_t s = v->stream;
    hv_profile_begin(v);
    hipLaunchKernelGGL(k_orb_grey, dim3((unsigned)std::min<int64_t>((npx + 255) / 256, 2048)), dim3(256), 0, s, st.dev<const uint8_t>(i_img), channels,
                       npx, pyr);
    for (int l = 1; l < L.n; ++l)
        hipLaunchKernelGGL(k_orb_down, dim3((unsigned)((L.W[l] + 63) / 64), (unsigned)((L.H[l] + 3) / 4)), dim3(256), 0, s, pyr + L.px_base[l - 1],
                           L.W[l - 1], pyr + L.px_base[l], L.H[l], L.W[l]);
    hv_profile_end(v, 0);
    hv_profile_begin(v);
    for (int l = 0; l < L.n; ++l)
        hipLaunchKernelGGL(k_orb_fast, dim3((unsigned)((L.W[l] + 31) / 32), (unsigned)((L.H[l] + 7) / 8)), dim3(256), 0, s, pyr + L.px_base[l], L.H[l],
                           L.W[l], P.threshold, V + L.px_base[l]);
    hv_profile_end(v, 0);
    hv_profile_begin(v);
    for (int l = 0; l < L.n; ++l)
        hipLaunchKernelGGL(k_orb_select, dim3((unsigned)(L.cell_base[l + 1] - L.cell_base[l])), dim3(64), 0, s, V + L.px_base[l], L.H[l], L.W[l],
                           L.cells_x[l], P.per_cell, L.cell_base[l], cnt, kp);
    hipLaunchKernelGGL(k_orb_scan, dim3(1), dim3(256), 0, s, cnt, cells, off, (int32_t *)st.head_dev);
    hv_profile_end(v, 0);
    hv_profile_begin(v);
    hipLaunchKernelGGL(k_orb_describe, dim3((unsigned)bound), dim3(64), 0, s, pyr, L, P.per_cell, cnt, off, kp, st.dev<int32_t>(o_kp),
                       st.dev<uint8_t>(o_desc));
    hv_profile_end(v, npx);
    HV_HIP(hipGetLastError());
    // the count goes back to the host: the call waits for the stream, for either loc
    int32_t count = 0;
    HV_HIP(hipMemcpyAsync(&count, st.head_dev, sizeof count, hipMemcpyDeviceToHost, s));
    HV_HIP(hipStreamSynchronize(s));
    st.rows(count);
    rc = st.finish();
    if (rc != HV_OK) return rc;
    *count_out = count;
    return HV_OK;
}

int hv_match_descriptors(hv_volume *v, const uint8_t *query, int32_t n_query, const uint8_t *train, int32_t n_train,
                         const int32_t *segment_offsets, int32_t n_segments, const hv_match_params *params, int32_t *index_out,
                         uint16_t *distance_out, uint16_t *second_out, int32_t *counts_out, int32_t loc) {
    HV_REQUIRE(v != nullptr && query != nullptr && segment_offsets != nullptr && params != nullptr && index_out != nullptr, HV_ERR_INVALID,
               "hv_match_descriptors: null argument");
    HV_REQUIRE(n_query >= 1 && n_query <= 65536, HV_ERR_INVALID, "hv_match_descriptors: n_query must be in 1..65536");
    HV_REQUIRE(n_train >= 0 && n_train < (1 << 24), HV_ERR_INVALID, "hv_match_descriptors: n_train must be in 0..2^24 - 1");
    HV_REQUIRE(train != nullptr || n_train == 0, HV_ERR_INVALID, "hv_match_descriptors: null argument");
    HV_REQUIRE(n_segments >= 1 && (int64_t)n_segments * n_query < ((int64_t)1 << 27), HV_ERR_INVALID,
               "hv_match_descriptors: need 1 <= n_segments and n_segments n_query < 2^27");
    const hv_match_params P = *params;
    HV_REQUIRE(P.max_distance >= 0 && P.max_distance <= 256, HV_ERR_INVALID, "hv_match_descriptors: max_distance must be in 0..256");
    HV_REQUIRE(P.ratio_percent >= 0 && P.ratio_percent <= 100, HV_ERR_INVALID, "hv_match_descriptors: ratio_percent must be in 0..100");
    HV_REQUIRE(P.cross_check == 0 || P.cross_check == 1, HV_ERR_INVALID, "hv_match_descriptors: cross_check must be 0 or 1");
    HV_REQUIRE(segment_offsets[0] == 0 && segment_offsets[n_segments] == n_train, HV_ERR_INVALID,
               "hv_match_descriptors: segment_offsets must start at 0 and end at n_train");
    for (int32_t k = 0; k < n_segments; ++k)
        HV_REQUIRE(segment_offsets[k] <= segment_offsets[k + 1], HV_ERR_INVALID, "hv_match_descriptors: segment_offsets must not decrease");
    HV_REQUIRE(loc != HV_DEVICE || (((uintptr_t)query | (uintptr_t)train) & 3) == 0, HV_ERR_INVALID,
               "hv_match_descriptors: device descriptors must be 4-byte aligned");
    HV_HIP(hipSetDevice(v->device));
    const int64_t rows = (int64_t)n_segments * n_query;
    // scratch of the handle: [owner i32 n_train][d1 u16 rows][d2 u16 rows] (the last two only where the caller passes no array)
    const size_t w_bytes = st_align(sizeof(int32_t) * (size_t)std::max(n_train, 1)), d_bytes = st_align(sizeof(uint16_t) * (size_t)rows);
    int rc = hv_ensure_buffer(v, &v->stereo_buf, &v->stereo_buf_bytes, w_bytes + 2 * d_bytes);
    if (rc != HV_OK) return rc;
    char *base = (char *)v->stereo_buf;
    int32_t *owner = (int32_t *)base;

    HvStage st(v, loc);
    const int i_q = st.in(query, (size_t)32 * n_query), i_t = st.in(train, (size_t)32 * n_train);
    const int i_off = st.in(segment_offsets, sizeof(int32_t) * ((size_t)n_segments + 1), HV_HOST);
    const int o_idx = st.out(index_out, sizeof(int32_t) * rows), o_d1 = st.out(distance_out, sizeof(uint16_t) * rows),
              o_d2 = st.out(second_out, sizeof(uint16_t) * rows), o_cnt = st.out(counts_out, sizeof(int32_t) * (size_t)n_segments);
    rc = st.commit(&v->stage, &v->stage_bytes);
    if (rc != HV_OK) return rc;
    uint16_t *d1 = distance_out != nullptr ? st.dev<uint16_t>(o_d1) : (uint16_t *)(base + w_bytes);
    uint16_t *d2 = second_out != nullptr ? st.dev<uint16_t>(o_d2) : (uint16_t *)(base + w_bytes + d_bytes);
    const uint32_t *q = st.dev<const uint32_t>(i_q), *t = st.dev<const uint32_t>(i_t);

    hipStream_t s = v->stream;
    const int nblk = (n_query + 255) / 256;
    hv_profile_begin(v);
    hipLaunchKernelGGL(k_hamming_best<true>, dim3((unsigned)(nblk * n_segments)), dim3(256), 0, s, q, n_query, t, n_train,
                       st.dev<const int32_t>(i_off), nblk, st.dev<int32_t>(o_idx), d1, d2);
    if (P.cross_check && n_train > 0)
        hipLaunchKernelGGL(k_hamming_best<false>, dim3((unsigned)((n_train + 255) / 256)), dim3(256), 0, s, t, n_train, q, n_query,
                           (const int32_t *)nullptr, (n_train + 255) / 256, owner, (uint16_t *)nullptr, (uint16_t *)nullptr);
    if (counts_out != nullptr) HV_HIP(hipMemsetAsync(st.dev<int32_t>(o_cnt), 0, sizeof(int32_t) * (size_t)n_segments, s));
    hipLaunchKernelGGL(k_match_accept, dim3((unsigned)(nblk * n_segments)), dim3(256), 0, s, st.dev<int32_t>(o_idx), d1, d2, owner, n_query, nblk,
                       P.max_distance, P.ratio_percent, P.cross_check, st.dev<int32_t>(o_cnt));
    hv_profile_end(v, rows);
    HV_HIP(hipGetLastError());
    return st.finish();
}

} // extern "C"
