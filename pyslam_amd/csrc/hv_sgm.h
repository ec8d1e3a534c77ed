// The semi-global matching stages that hv_stereo_sgm (hv_stereo.hip) and hv_mvs_sgm (hv_mvs.hip) share: the grey conversion and the
// 9x7 census, the register-resident path kernel, the winner and uniqueness kernel and the sub-pixel step (rules 1, 2, 4, 5, 6 and 8
// of the stereo matcher in include/hipvol.h, which the multi-view rules M1, M5 and M7 refer to).  One copy of each rule; the two
// callers differ in where the matching cost comes from and in whether the winner kernel also collects the right image's votes:
//   StCostCensus  C(y,x,d) recomputed at every step of a path from two census images (stereo rule 3)
//   StCostVolume  C read from a uint8 volume [H,W,D], VPL bytes per lane and step (the plane sweep of hv_mvs_sgm, rule M4)
#pragma once
#include "hv_common.h"

static constexpr int ST_INF = 1 << 20;  // an absent L: larger than any L + P2, small enough to add penalties to
static constexpr int ST_TILE_W = 32, ST_TILE_H = 8, ST_RX = 4, ST_RY = 3;
static constexpr int ST_MAX_IMAGES = 5;  // a stereo pair; a reference image and up to four source views

// the images of one census launch and where each one's census words go
struct StCensusList {
    const uint8_t *img[ST_MAX_IMAGES];
    uint64_t *out[ST_MAX_IMAGES];
};
// rules 1 and 2 for the first n images of the list, all [H,W] with C channels, in one launch on s (hv_stereo.hip)
void st_launch_census(hipStream_t s, const StCensusList &list, int n, int H, int W, int C);

__device__ __forceinline__ int st_grey(const uint8_t *__restrict__ img, int C, int64_t i) {
    if (C == 1) return img[i];
    const uint8_t *p = img + 3 * i;
    return ((int)p[0] + 2 * (int)p[1] + (int)p[2] + 2) >> 2;
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
template <int N> struct alignas(N) StBytes {
    uint8_t v[N];
};

// Where the cost of a path step comes from.  fetch() issues the loads of one pixel for the lane's disparities d0 .. d0 + VPL - 1,
// cost() turns what they brought into C(y,x,d0 + j).
struct StCostCensus {
    const uint64_t *__restrict__ census_l;
    const uint64_t *__restrict__ census_r;
    template <int VPL> struct Regs {
        uint64_t cl;
        uint64_t cr[VPL];
    };
    template <int VPL> __device__ __forceinline__ void fetch(Regs<VPL> &r, int W, int D, int x, int y, int d0) const {
        const int64_t p = (int64_t)y * W + x;
        r.cl = census_l[p];
#pragma unroll
        for (int j = 0; j < VPL; ++j) r.cr[j] = x - (d0 + j) >= 0 ? census_r[p - (d0 + j)] : 0;  // p - d stays inside row y
    }
    template <int VPL> __device__ __forceinline__ void cost(const Regs<VPL> &r, int x, int d0, int (&L)[VPL]) const {
#pragma unroll
        for (int j = 0; j < VPL; ++j) L[j] = x - (d0 + j) >= 0 ? __popcll(r.cl ^ r.cr[j]) : 64;
    }
};
struct StCostVolume {
    const uint8_t *__restrict__ C;  // [H,W,D]
    template <int VPL> struct Regs {
        StBytes<VPL> c;
    };
    template <int VPL> __device__ __forceinline__ void fetch(Regs<VPL> &r, int W, int D, int x, int y, int d0) const {
        if (d0 < D) r.c = *(const StBytes<VPL> *)(C + ((int64_t)y * W + x) * D + d0);  // (a lane outside [0, D) reads nothing)
    }
    template <int VPL> __device__ __forceinline__ void cost(const Regs<VPL> &r, int x, int d0, int (&L)[VPL]) const {
#pragma unroll
        for (int j = 0; j < VPL; ++j) L[j] = r.c.v[j];
    }
};

// what one step of a path reads from memory: the cost's operands and the lane's part of S
template <int VPL, typename Cost> struct StFetch {
    typename Cost::template Regs<VPL> c;
    StPack<VPL> s;
};

template <int VPL, typename Cost>
__device__ __forceinline__ void st_fetch(StFetch<VPL, Cost> &f, const Cost &cost, const uint16_t *S, int W, int D, int x, int y, int d0,
                                         bool read_s) {
    cost.template fetch<VPL>(f.c, W, D, x, y, d0);
    if (read_s && d0 < D) f.s = *(const StPack<VPL> *)(S + ((int64_t)y * W + x) * D + d0);
}

// One direction (dx, dy) of rule 4.  Wave w of the launch walks the path that starts at the w-th pixel whose predecessor lies outside
// the image: with dx != 0 the H pixels of the column x0 the direction leaves from, with dy != 0 the pixels of row y0 (without column
// x0 when it is counted already).  Lane l holds the disparities l VPL .. l VPL + VPL - 1; D is a multiple of VPL, so a lane is
// either wholly inside [0, D) or wholly outside (its L stays ST_INF and it writes nothing).
template <int VPL, typename Cost>
__global__ __launch_bounds__(256) void k_sgm_path(const Cost cost, int H, int W, int D, int dx, int dy, int p1, int p2, int first, uint16_t *S) {
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
    StFetch<VPL, Cost> cur, nxt;
    st_fetch<VPL, Cost>(cur, cost, S, W, D, x, y, d0, !first);
    for (;;) {
        const int xn = x + dx, yn = y + dy;
        const bool more = xn >= 0 && xn < W && yn >= 0 && yn < H;  // the same in every lane
        if (more) st_fetch<VPL, Cost>(nxt, cost, S, W, D, xn, yn, d0, !first);  // in flight while this pixel is worked out
        int L[VPL];
        cost.template cost<VPL>(cur.c, x, d0, L);
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

template <int VPL, typename Cost>
static void st_launch_path(hipStream_t s, const Cost &cost, int H, int W, int D, int dx, int dy, int p1, int p2, int first, uint16_t *S) {
    const int n = (dx != 0 ? H : 0) + (dy != 0 ? (dx != 0 ? W - 1 : W) : 0);
    if (n <= 0) return;  // (a diagonal of a one-column image: the H starts of the side are all there is, n = H)
    hipLaunchKernelGGL((k_sgm_path<VPL, Cost>), dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, cost, H, W, D, dx, dy, p1, p2, first, S);
}

// Rule 4: S = the sum of L over the first `paths` directions, one launch each.  q -> p steps: the four axis directions, then the four
// diagonals (the order of tests/stereo_reference.py; the sum does not depend on it).
template <typename Cost> static void st_launch_paths(hipStream_t s, const Cost &cost, int H, int W, int D, int paths, int p1, int p2, uint16_t *S) {
    static const int dirs[8][2] = {{1, 0}, {-1, 0}, {0, 1}, {0, -1}, {1, 1}, {-1, -1}, {1, -1}, {-1, 1}};
    for (int k = 0; k < paths; ++k) {
        const int dx = dirs[k][0], dy = dirs[k][1], first = k == 0;
        if (D <= 64)
            st_launch_path<1, Cost>(s, cost, H, W, D, dx, dy, p1, p2, first, S);
        else if (D <= 128)
            st_launch_path<2, Cost>(s, cost, H, W, D, dx, dy, p1, p2, first, S);
        else
            st_launch_path<4, Cost>(s, cost, H, W, D, dx, dy, p1, p2, first, S);
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

// Rules 5 and 6 for the left image and, with VOTES, rule 7's right disparity.  A workgroup takes ST_WIN_TILE consecutive pixels of one
// row; 16 lanes share a pixel, lane j of them reads the disparities j, j + 16, ...: S is read in whole rows.  A value is ranked by the
// key (S << 8) | d, whose minimum is the smallest S and among equals the smallest d.  VOTES: the same keys vote for the right image:
// S(y,x,d) belongs to the right pixel x - d, whose minimum is kept in LDS for the tile's span of right pixels and merged into r_keys
// (set to ST_NO_KEY beforehand) with one atomic per right pixel and tile; without VOTES r_keys is not touched.  d_left = d*, or -1
// where d* is not unique.
template <bool VOTES>
__global__ __launch_bounds__(256) void k_sgm_winner(const uint16_t *__restrict__ S, int W, int D, int uniqueness, int16_t *__restrict__ d_left,
                                                     uint32_t *__restrict__ r_keys) {
    __shared__ uint32_t votes[VOTES ? ST_WIN_TILE + 256 : 1];  // right pixels x0 - (D - 1) .. x0 + ST_WIN_TILE - 1
    const int y = blockIdx.y, x0 = blockIdx.x * ST_WIN_TILE, r0 = x0 - (D - 1);
    if constexpr (VOTES) {
        for (int k = threadIdx.x; k < ST_WIN_TILE + 256; k += 256) votes[k] = ST_NO_KEY;
        __syncthreads();
    }
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
                if constexpr (VOTES)
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
    if constexpr (VOTES) {
        __syncthreads();
        for (int k = threadIdx.x; k < ST_WIN_TILE + D - 1; k += 256) {
            const int xr = r0 + k;
            if (xr >= 0 && xr < W && votes[k] != ST_NO_KEY) atomicMin(&r_keys[(int64_t)y * W + xr], votes[k]);
        }
    }
}

template <bool VOTES> static void st_launch_winner(hipStream_t s, const uint16_t *S, int H, int W, int D, int uniqueness, int16_t *d_left, uint32_t *r_keys) {
    hipLaunchKernelGGL(k_sgm_winner<VOTES>, dim3((unsigned)((W + ST_WIN_TILE - 1) / ST_WIN_TILE), (unsigned)H), dim3(256), 0, s, S, W, D, uniqueness,
                       d_left, r_keys);
}

// Rule 8: the winner d of a pixel in sixteenths, with the parabola offset for 0 < d < D - 1.  s: the pixel's D values of S.
__device__ __forceinline__ int st_subpixel16(const uint16_t *__restrict__ s, int d, int D) {
    int d16 = 16 * d;
    if (d > 0 && d < D - 1) {
        const int sm = s[d - 1], s0 = s[d], sp = s[d + 1];
        const int den = max(sm + sp - 2 * s0, 1);
        d16 += ((sm - sp) * 16 + den) / (2 * den);  // C division: toward zero
    }
    return d16;
}

static inline size_t st_align(size_t n) { return (n + 255) & ~(size_t)255; }

// The handle's stereo scratch, grown on demand to `want` bytes (the stream is drained before a smaller one is freed).
// -> HV_OK, or HV_ERR_CAPACITY with the message `fn: cannot allocate ...`
int st_scratch(hv_volume *v, size_t want, const char *fn, int height, int width, int D);
