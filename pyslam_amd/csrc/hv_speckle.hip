// libpyslam_hipvol.so — hv_filter_speckles: connected components of an image under "4-neighbours link when both are valid and differ
// by at most max_diff", and the removal of the small ones (cv2.filterSpeckles' rule).  The contract (S1 - S7) is written once in
// include/hipvol.h; tests/speckle_reference.py restates it in numpy, and this file is held to that restatement bit for bit.
//
// The idiom is hv_components.hip's, on a dense 2-D lattice: union-find with parent[i] <= i, links by atomicMin towards the smaller
// index, so that a component's root is its smallest row-major index - the label of S4.  Two int32 per pixel of scratch: parent[]
// (SP_NONE for an invalid pixel) and size[] (meaningful at roots).
//   k_sp_local    one workgroup per SP_TILE_W x SP_TILE_H tile: values and parents in LDS; a pixel links to its left and upper
//                 neighbour only (every edge once, from its larger end); flattened, parent[] written as global pixel indices;
//                 size[] zeroed
//   k_sp_cross    one workgroup per tile: its bottom row against the row below, its right column against the column to the right,
//                 the same union on the global parent[]
//   k_sp_flatten  one lane per pixel: parent[i] = root; sizes by one atomic per run of equal roots among the 1024 consecutive pixels
//                 of a workgroup (an all-equal image makes H W / 1024 atomics on its one root, not H W)
//   k_sp_apply    one lane per pixel: out, depth, labels; the five counts by wave reductions and one atomic per wave and count
// Every link loop strictly lowers the larger of its two indices, so it ends; no wave waits for another; there is no loop over
// propagation rounds on the host at all.
#include <cmath>

#include "hv_common.h"

namespace {

constexpr int SP_TILE_W = 64, SP_TILE_H = 16;  // tests/speckle_reference.py repeats them (TILE_W, TILE_H)
constexpr int SP_TILE = SP_TILE_W * SP_TILE_H;
constexpr int SP_PER_THREAD = SP_TILE / 256;   // a thread's pixels lie SP_TILE_H / SP_PER_THREAD rows apart
constexpr int SP_FLAT = 1024;                  // pixels (threads) of a workgroup of k_sp_flatten
constexpr uint32_t SP_NONE = 0xffffffffu;      // parent of an invalid pixel: -1 as int32, S4's label
enum { SP_S_VALID = 0, SP_S_COMPONENTS = 1, SP_S_LARGEST = 2, SP_S_COMP_REMOVED = 3, SP_S_PIX_REMOVED = 4, SP_S_WORDS = 5 };

// What the kernels know of the pixel type: KIND 0 = int16 (held sign-extended in 32 bits), 1 = float32 (held as its bits).
template <int KIND> struct SpRule {
    uint32_t new_bits;  // int16: the value sign-extended; float32: the bits of (float)new_val
    uint32_t diff_bits; // int16: max_diff as an integer in 0..65535; float32: the bits of (float)max_diff
    __device__ __forceinline__ uint32_t load(const void *img, int64_t i) const {
        if (KIND == 0) return (uint32_t)(int32_t)((const int16_t *)img)[i];
        return ((const uint32_t *)img)[i];
    }
    // S1
    __device__ __forceinline__ bool valid(uint32_t a) const {
        if (KIND == 0) return a != new_bits;
        return __uint_as_float(a) != __uint_as_float(new_bits);  // IEEE: NaN is valid, -0.0 equals 0.0
    }
    // S2 for two valid pixels
    __device__ __forceinline__ bool near(uint32_t a, uint32_t b) const {
        if (KIND == 0) {
            const int32_t d = (int32_t)a - (int32_t)b;  // |d| <= 65535: no wrap
            return (uint32_t)(d < 0 ? -d : d) <= diff_bits;
        }
        return fabsf(__uint_as_float(a) - __uint_as_float(b)) <= __uint_as_float(diff_bits);  // false for NaN
    }
};

// ---- union-find: parent[i] <= i always, links go to the smaller index, a root has parent[i] == i --------------------------------
// find with path halving: a non-root's parent is lowered to its grandparent (atomicMin: an ancestor, never above what is there).
template <bool GLOBAL>
__device__ __forceinline__ uint32_t sp_load(uint32_t *p, uint32_t a) {
    if (GLOBAL) return __hip_atomic_load(&p[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // past this CU's L1
    return __hip_atomic_load(&p[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
template <bool GLOBAL>
__device__ __forceinline__ uint32_t sp_find(uint32_t *p, uint32_t a) {
    for (;;) {
        const uint32_t up = sp_load<GLOBAL>(p, a);
        if (up == a) return a;
        const uint32_t up2 = sp_load<GLOBAL>(p, up);
        if (up2 != up) atomicMin(&p[a], up2);
        a = up2;  // < a
    }
}
// Every turn either ends or replaces the larger index by a smaller one: at most a + b turns.
template <bool GLOBAL>
__device__ __forceinline__ void sp_union(uint32_t *p, uint32_t a, uint32_t b) {
    for (;;) {
        a = sp_find<GLOBAL>(p, a);
        b = sp_find<GLOBAL>(p, b);
        if (a == b) return;
        if (a < b) {
            const uint32_t s = a;
            a = b;
            b = s;
        }
        const uint32_t old = atomicMin(&p[a], b);
        if (old == a) return;  // a was a root: linked
        a = old;               // a had been linked meanwhile (to old < a): old and b still have to meet
    }
}

template <int KIND>
__global__ __launch_bounds__(256) void k_sp_local(const void *image, int H, int W, SpRule<KIND> rule, uint32_t *__restrict__ parent,
                                                  uint32_t *__restrict__ size) {
    __shared__ uint32_t val[SP_TILE];
    __shared__ uint32_t par[SP_TILE];
    const int t = (int)threadIdx.x;
    const int x0 = (int)blockIdx.x * SP_TILE_W, y0 = (int)blockIdx.y * SP_TILE_H;
    const int lx = t % SP_TILE_W, ly0 = t / SP_TILE_W;
    constexpr int STEP = 256 / SP_TILE_W;  // rows between two pixels of a thread
    const int x = x0 + lx;
#pragma unroll
    for (int k = 0; k < SP_PER_THREAD; ++k) {
        const int ly = ly0 + k * STEP, y = y0 + ly, l = ly * SP_TILE_W + lx;
        const bool in = x < W && y < H;
        const uint32_t a = in ? rule.load(image, (int64_t)y * W + x) : 0u;
        val[l] = a;
        par[l] = in && rule.valid(a) ? (uint32_t)l : SP_NONE;
    }
    __syncthreads();
    // (a parent is SP_NONE from the start or never: the test below reads validity, whatever the links have done since)
#pragma unroll
    for (int k = 0; k < SP_PER_THREAD; ++k) {
        const int ly = ly0 + k * STEP, l = ly * SP_TILE_W + lx;
        if (sp_load<false>(par, (uint32_t)l) == SP_NONE) continue;
        const uint32_t a = val[l];
        if (lx > 0 && sp_load<false>(par, (uint32_t)(l - 1)) != SP_NONE && rule.near(a, val[l - 1])) sp_union<false>(par, (uint32_t)l, (uint32_t)(l - 1));
        if (ly > 0 && sp_load<false>(par, (uint32_t)(l - SP_TILE_W)) != SP_NONE && rule.near(a, val[l - SP_TILE_W]))
            sp_union<false>(par, (uint32_t)l, (uint32_t)(l - SP_TILE_W));
    }
    __syncthreads();
    // the order of l inside the tile is the order of y W + x: the smallest l of a component is its smallest pixel index
#pragma unroll
    for (int k = 0; k < SP_PER_THREAD; ++k) {
        const int ly = ly0 + k * STEP, y = y0 + ly, l = ly * SP_TILE_W + lx;
        if (x >= W || y >= H) continue;
        const int64_t i = (int64_t)y * W + x;
        uint32_t r = SP_NONE;
        if (sp_load<false>(par, (uint32_t)l) != SP_NONE) {
            const uint32_t root = sp_find<false>(par, (uint32_t)l);
            r = (uint32_t)((y0 + (int)(root / SP_TILE_W)) * W + x0 + (int)(root % SP_TILE_W));
        }
        parent[i] = r;
        size[i] = 0u;
    }
}

// 128 threads per tile: lane t < SP_TILE_W takes the bottom row's pixel (x0 + t, y0 + SP_TILE_H - 1) and the one below it, lane
// SP_TILE_W + k the right column's pixel (x0 + SP_TILE_W - 1, y0 + k) and the one to its right.
template <int KIND>
__global__ __launch_bounds__(128) void k_sp_cross(const void *image, int H, int W, SpRule<KIND> rule, uint32_t *parent) {
    static_assert(SP_TILE_W + SP_TILE_H <= 128, "one lane per seam pixel");
    const int t = (int)threadIdx.x;
    const int x0 = (int)blockIdx.x * SP_TILE_W, y0 = (int)blockIdx.y * SP_TILE_H;
    int x, y, x2, y2;
    if (t < SP_TILE_W) {
        x = x2 = x0 + t;
        y = y0 + SP_TILE_H - 1;
        y2 = y + 1;
    } else if (t < SP_TILE_W + SP_TILE_H) {
        y = y2 = y0 + t - SP_TILE_W;
        x = x0 + SP_TILE_W - 1;
        x2 = x + 1;
    } else {
        return;
    }
    if (x2 >= W || y2 >= H) return;  // (x <= x2 and y <= y2: both pixels are inside the image)
    const int64_t i = (int64_t)y * W + x, j = (int64_t)y2 * W + x2;
    const uint32_t a = rule.load(image, i), b = rule.load(image, j);
    if (!rule.valid(a) || !rule.valid(b) || !rule.near(a, b)) return;
    sp_union<true>(parent, (uint32_t)j, (uint32_t)i);
}

// parent[i] = the root of i.  Roots do not change here, and a parent read while another lane shortens it is an ancestor either way.
__global__ __launch_bounds__(SP_FLAT) void k_sp_flatten(uint32_t *parent, uint32_t n, uint32_t *size) {
    __shared__ uint32_t s_root[SP_FLAT];
    __shared__ unsigned long long s_heads[SP_FLAT / 64];
    const int t = (int)threadIdx.x;
    const uint32_t i = blockIdx.x * (uint32_t)SP_FLAT + threadIdx.x;  // n < 2^30: the grid's last index stays below 2^31
    // Plain loads, through this CU's L1: nothing links here, the only stores put a pixel's root into its own word, so whatever copy
    // of a word a lane reads - the one the kernel started with or the new one - names an ancestor, and a root's word never changes.
    uint32_t r = i < n ? parent[i] : SP_NONE;
    if (r != SP_NONE) {
        const uint32_t up0 = r;
        for (;;) {
            const uint32_t up = parent[r];
            if (up == r) break;
            r = up;
        }
        if (r != up0) parent[i] = r;
    }
    // runs of equal roots over the workgroup's SP_FLAT pixels: a run's first lane adds its length.  (Atomics on one address take
    // their turns, about 12 ns each: per wave they were half of the filter's time on an image that is mostly one region.)
    s_root[t] = r;
    __syncthreads();
    const int lane = hv_lane_id(), wave = t >> 6;
    const bool head = t == 0 || s_root[t - 1] != r;
    const unsigned long long heads = __ballot(head);
    if (lane == 0) s_heads[wave] = heads;
    __syncthreads();
    if (head && r != SP_NONE) {
        const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
        int len;
        if (above != 0ull) {
            len = __ffsll((long long)above);
        } else {
            len = 64 - lane;
            for (int w = wave + 1; w < SP_FLAT / 64; ++w) {
                const unsigned long long m = s_heads[w];
                if (m != 0ull) {
                    len += __ffsll((long long)m) - 1;
                    break;
                }
                len += 64;
            }
        }
        atomicAdd(&size[r], (uint32_t)len);
    }
}

__device__ __forceinline__ uint32_t sp_wave_max(uint32_t v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o));
    return v;
}

// S6, S7, the labels and the counts.  out may be image (each lane reads its pixel before it writes it).
template <int KIND>
__global__ __launch_bounds__(256) void k_sp_apply(const void *image, uint32_t n, SpRule<KIND> rule, uint32_t max_size,
                                                  const uint32_t *__restrict__ parent, const uint32_t *__restrict__ size, void *out,
                                                  float *depth, int32_t *labels, unsigned long long *stats) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const bool live = i < n;
    const uint32_t r = live ? parent[i] : SP_NONE;
    const bool valid = r != SP_NONE;
    const uint32_t sz = valid ? size[r] : 0u;
    const bool gone = valid && sz <= max_size;
    if (live) {
        const uint32_t a = rule.load(image, i);
        const uint32_t o = gone ? rule.new_bits : a;
        if (KIND == 0)
            ((int16_t *)out)[i] = (int16_t)(int32_t)o;
        else
            ((uint32_t *)out)[i] = o;
        if (depth != nullptr && gone) depth[i] = 0.0f;
        if (labels != nullptr) labels[i] = (int32_t)r;
    }
    if (stats == nullptr) return;
    const bool root = valid && r == i;
    const unsigned long long m_valid = __ballot(valid), m_root = __ballot(root), m_comp_gone = __ballot(root && gone), m_gone = __ballot(gone);
    const uint32_t largest = sp_wave_max(root ? sz : 0u);
    if (hv_lane_id() == 0 && m_valid != 0ull) {
        atomicAdd(&stats[SP_S_VALID], (unsigned long long)__popcll(m_valid));
        if (m_root != 0ull) {
            atomicAdd(&stats[SP_S_COMPONENTS], (unsigned long long)__popcll(m_root));
            atomicMax(&stats[SP_S_LARGEST], (unsigned long long)largest);
        }
        if (m_comp_gone != 0ull) atomicAdd(&stats[SP_S_COMP_REMOVED], (unsigned long long)__popcll(m_comp_gone));
        if (m_gone != 0ull) atomicAdd(&stats[SP_S_PIX_REMOVED], (unsigned long long)__popcll(m_gone));
    }
}

template <int KIND>
void sp_launch(hv_volume *v, const void *image, int H, int W, SpRule<KIND> rule, uint32_t max_size, uint32_t *parent, uint32_t *size,
               void *out, float *depth, int32_t *labels, unsigned long long *d_stats) {
    hipStream_t s = v->stream;
    const uint32_t n = (uint32_t)((int64_t)H * W);
    const dim3 tiles((unsigned)((W + SP_TILE_W - 1) / SP_TILE_W), (unsigned)((H + SP_TILE_H - 1) / SP_TILE_H));
    const unsigned px_grid = (unsigned)((n + 255u) / 256u);
    hv_profile_begin(v);
    hipLaunchKernelGGL(k_sp_local<KIND>, tiles, dim3(256), 0, s, image, H, W, rule, parent, size);
    hv_profile_end(v, 0);
    hv_profile_begin(v);
    hipLaunchKernelGGL(k_sp_cross<KIND>, tiles, dim3(128), 0, s, image, H, W, rule, parent);
    hv_profile_end(v, 0);
    hv_profile_begin(v);
    hipLaunchKernelGGL(k_sp_flatten, dim3((unsigned)((n + SP_FLAT - 1u) / SP_FLAT)), dim3(SP_FLAT), 0, s, parent, n, size);
    hv_profile_end(v, 0);
    hv_profile_begin(v);
    hipLaunchKernelGGL(k_sp_apply<KIND>, dim3(px_grid), dim3(256), 0, s, image, n, rule, max_size, parent, size, out, depth, labels, d_stats);
    hv_profile_end(v, (int64_t)n);
}

uint32_t sp_float_bits(float f) {
    uint32_t u;
    memcpy(&u, &f, sizeof u);
    return u;
}

// [a, a + na) and [b, b + nb) share a byte (either may be absent)
bool sp_overlap(const void *a, size_t na, const void *b, size_t nb) {
    if (a == nullptr || b == nullptr) return false;
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + nb && b0 < a0 + na;
}

} // namespace

int hv_speckle_launch(hv_volume *v, const char *fn, const void *image, int32_t kind, int32_t height, int32_t width, double new_val,
                      int64_t max_speckle_size, double max_diff, void *out, float *depth, int32_t *labels, unsigned long long *d_stats) {
    const int64_t npx = (int64_t)height * width;
    const size_t want = sizeof(uint32_t) * 2 * (size_t)npx;
    if (v->speckle_buf == nullptr || v->speckle_buf_bytes < want) {
        if (v->speckle_buf != nullptr) {
            HV_HIP(hipStreamSynchronize(v->stream));
            HV_HIP(hipFree(v->speckle_buf));
            v->speckle_buf = nullptr;
            v->speckle_buf_bytes = 0;
        }
        if (hipMalloc(&v->speckle_buf, want) != hipSuccess) {
            (void)hipGetLastError();
            v->speckle_buf = nullptr;
            hv_set_error("%s: cannot allocate %zu bytes of scratch (%d x %d)", fn, want, height, width);
            return HV_ERR_CAPACITY;
        }
        v->speckle_buf_bytes = want;
    }
    uint32_t *parent = (uint32_t *)v->speckle_buf, *size = parent + npx;
    if (d_stats != nullptr) HV_HIP(hipMemsetAsync(d_stats, 0, sizeof(unsigned long long) * SP_S_WORDS, v->stream));
    const uint32_t max_size = (uint32_t)std::min<int64_t>(max_speckle_size, (int64_t)1 << 30);  // sizes stay below 2^30
    if (kind == HV_SPECKLE_I16) {
        SpRule<0> rule{(uint32_t)(int32_t)new_val, (uint32_t)std::min(std::floor(max_diff), 65535.0)};
        sp_launch<0>(v, image, height, width, rule, max_size, parent, size, out, depth, labels, d_stats);
    } else {
        SpRule<1> rule{sp_float_bits((float)new_val), sp_float_bits((float)max_diff)};
        sp_launch<1>(v, image, height, width, rule, max_size, parent, size, out, depth, labels, d_stats);
    }
    HV_HIP(hipGetLastError());
    return HV_OK;
}

extern "C" {

int hv_filter_speckles(hv_volume *v, const void *image, int32_t kind, int32_t height, int32_t width, double new_val, int64_t max_speckle_size,
                       double max_diff, void *out, float *depth_inout, int32_t *labels_out, hv_speckle_stats *stats, int32_t loc) {
    HV_REQUIRE(v != nullptr && image != nullptr && out != nullptr, HV_ERR_INVALID, "hv_filter_speckles: null argument");
    HV_REQUIRE(kind == HV_SPECKLE_I16 || kind == HV_SPECKLE_F32, HV_ERR_INVALID, "hv_filter_speckles: kind must be HV_SPECKLE_I16 or HV_SPECKLE_F32");
    HV_REQUIRE(height >= 1 && width >= 1 && height <= 32768 && width <= 32768 && (int64_t)height * width < (int64_t)1 << 30, HV_ERR_INVALID,
               "hv_filter_speckles: bad image size");
    HV_REQUIRE(max_speckle_size >= 0, HV_ERR_INVALID, "hv_filter_speckles: max_speckle_size must not be negative");
    HV_REQUIRE(std::isfinite(max_diff) && max_diff >= 0.0 && (kind != HV_SPECKLE_I16 || max_diff <= 65535.0), HV_ERR_INVALID,
               "hv_filter_speckles: max_diff must be finite and not negative (int16: at most 65535)");
    HV_REQUIRE(kind != HV_SPECKLE_I16 || (new_val >= -32768.0 && new_val <= 32767.0 && new_val == std::floor(new_val)), HV_ERR_INVALID,
               "hv_filter_speckles: new_val of an int16 image must be an integer in -32768..32767");
    const int64_t npx = (int64_t)height * width;
    const size_t img_bytes = (size_t)npx * (kind == HV_SPECKLE_I16 ? 2 : 4);
    HV_REQUIRE((out == image || !sp_overlap(image, img_bytes, out, img_bytes)) && !sp_overlap(image, img_bytes, depth_inout, sizeof(float) * npx) &&
                   !sp_overlap(image, img_bytes, labels_out, sizeof(int32_t) * npx),
               HV_ERR_INVALID, "hv_filter_speckles: out, depth and labels must not overlap image (out may be image itself)");
    HV_HIP(hipSetDevice(v->device));
    HvStage st(v, loc);
    if (stats != nullptr) st.head(sizeof(unsigned long long) * SP_S_WORDS);
    const int i_img = st.in(image, img_bytes), i_depth = st.in(depth_inout, sizeof(float) * npx);
    const int o_out = st.out(out, img_bytes), o_depth = st.out(depth_inout, sizeof(float) * npx), o_labels = st.out(labels_out, sizeof(int32_t) * npx);
    int rc = st.commit(&v->stage, &v->stage_bytes);
    if (rc != HV_OK) return rc;
    // depth is read and written: staged once as an input, the same bytes copied back
    float *d_depth = st.dev<float>(i_depth);
    if (loc == HV_HOST && depth_inout != nullptr) st.piece[o_depth].dev = d_depth;
    unsigned long long *d_stats = (unsigned long long *)st.head_dev;
    rc = hv_speckle_launch(v, "hv_filter_speckles", st.dev<const void>(i_img), kind, height, width, new_val, max_speckle_size, max_diff,
                           st.dev<void>(o_out), d_depth, st.dev<int32_t>(o_labels), d_stats);
    if (rc != HV_OK) return rc;
    unsigned long long h[SP_S_WORDS] = {0, 0, 0, 0, 0};
    rc = st.finish(stats != nullptr ? h : nullptr, sizeof h);
    if (rc != HV_OK) return rc;
    if (stats != nullptr) *stats = hv_speckle_stats{(int64_t)h[0], (int64_t)h[1], (int64_t)h[2], (int64_t)h[3], (int64_t)h[4]};
    return HV_OK;
}

} // extern "C"
