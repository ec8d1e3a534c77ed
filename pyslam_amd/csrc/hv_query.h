// Shared by the VOXEL_GRID and the semantic payloads: grid parameters, and the bbox / camera-frustum
// query description with its host-side setup (reference: camera_frustrum.cpp:175-264,
// voxel_block_grid.hpp:827-835, 1339-1349).
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>
#include <initializer_list>
#include <numeric>
#include <vector>

#include "hv_common.h"

struct HvGridParams {
    float inv_voxel_size; // 1.0f / voxel_size  (voxel_block_grid.hpp:6)
    int32_t bs;           // block_size
    int32_t nvox;         // bs^3
    int32_t local_bits;
    int32_t bs_shift;     // log2(bs) when bs is a power of two (the default 8 and 16), else -1
    int32_t owner_rank, owner_world; // multi-GPU block ownership (hv_set_owner): this GPU fuses block b iff hv_owner_of(b) % world == rank
};

// Block-ownership sharding of the grid modes (SURVEY 8e "zero reduce" form): a point whose block another GPU owns is skipped
// here - it is neither fused nor counted as dropped.
__host__ __device__ inline bool hv_block_is_foreign(const HvGridParams &G, uint64_t packed_block_key) {
    return G.owner_world > 1 && hv_owner_of(packed_block_key, G.owner_world) != G.owner_rank;
}

// floor_div, voxel_hashing.h:139-142
__host__ __device__ inline int32_t hv_floor_div(int32_t a, int32_t b) {
    const int64_t aa = a, bb = b;
    return (int32_t)((aa >= 0) ? (aa / bb) : ((aa - bb + 1) / bb));
}

static inline HvGridParams grid_params(const hv_volume *v) {
    HvGridParams G;
    const float vs = (float)v->cfg.voxel_size; // pybind narrows the Python double to float first
    G.inv_voxel_size = 1.0f / vs;
    G.bs = v->cfg.block_size;
    G.nvox = G.bs * G.bs * G.bs;
    G.local_bits = v->local_bits;
    G.bs_shift = -1;
    for (int sh = 0; sh <= 4; ++sh)
        if ((1 << sh) == G.bs) G.bs_shift = sh;
    G.owner_rank = v->owner_rank;
    G.owner_world = v->owner_world;
    return G;
}

// ---- a point's voxel: what the integrate (hv_voxel_grid.hip) and the point lookup (hv_lookup.hip) share ----
struct HvPointKey {
    int32_t v[3], b[3], l[3];
};
#ifdef __HIPCC__
// get_voxel_key_inv<Tp,float> + get_block_key + get_local_voxel_key.  Tp = float: floorf(x * inv) in float; Tp = double (the
// binding's py::array_t<double> overload, volumetric_grid_module.h:738-741): the float inverse voxel size is promoted and the
// product and floor are double - a float64 point near a cell border keeps its own cell instead of its float32 neighbour's.
template <typename Tp>
__device__ __forceinline__ HvPointKey hv_point_key(Tp x, Tp y, Tp z, const HvGridParams &G) {
    HvPointKey k;
    const Tp inv = (Tp)G.inv_voxel_size;
    const Tp f[3] = {floor(x * inv), floor(y * inv), floor(z * inv)};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        k.v[a] = (int32_t)f[a];
        // floor_div (voxel_hashing.h:139-142) without the 64-bit division (3 per point: most of the key kernel's time): an
        // arithmetic shift for power-of-two blocks, else floor(v * (1 / bs) + 2^-10) in double - exact for |v| < 2^31 and
        // bs <= 16: a non-integer v / bs is at least 1/16 away from an integer, the product's error is below 2^-20
        k.b[a] = G.bs_shift >= 0 ? (k.v[a] >> G.bs_shift) : (int32_t)floor(fma((double)k.v[a], 1.0 / (double)G.bs, 0x1p-10));
        k.l[a] = k.v[a] - k.b[a] * G.bs; // in [0, bs): no overflow (|b * bs| <= |v| + bs)
    }
    return k;
}
// the point is finite and its voxel index fits the 32-bit key
template <typename Tp>
__device__ __forceinline__ bool hv_point_keyable(Tp x, Tp y, Tp z, const HvGridParams &G) {
    const Tp inv = (Tp)G.inv_voxel_size, lim = (Tp)1.0e9;
    return isfinite(x) && isfinite(y) && isfinite(z) && fabs(x * inv) < lim && fabs(y * inv) < lim && fabs(z * inv) < lim;
}
#endif

// ---- scans over all allocated voxels -----------------------------------------------------------
struct HvQuery {
    int32_t kind; // 0: all, 1: bbox, 2: frustum, 3: carve
    int32_t min_count;
    int32_t vmin[3], vmax[3], bmin[3], bmax[3];
    double bb[6];
    // frustum (CameraFrustrum, camera_frustrum.h:108-121)
    float fx, fy, cx, cy, depth_max, depth_min;
    int32_t width, height;
    double R[9], t[3];
    float carve_threshold;
};

// CameraFrustrum::contains<T>, camera_frustrum.cpp:175-196 (the point is cast to double first)
__device__ __forceinline__ bool hv_frustum_contains_d(const HvQuery &Q, double p0, double p1, double p2, float *uvd) {
    double pc[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) pc[r] = (Q.R[r * 3 + 0] * p0 + Q.R[r * 3 + 1] * p1 + Q.R[r * 3 + 2] * p2) + Q.t[r];
    const float depth = (float)pc[2];
    if (!(depth >= Q.depth_min && depth <= Q.depth_max)) return false;
    const float u = (float)((double)Q.fx * (pc[0] / pc[2]) + (double)Q.cx);
    const float v = (float)((double)Q.fy * (pc[1] / pc[2]) + (double)Q.cy);
    uvd[0] = u;
    uvd[1] = v;
    uvd[2] = depth;
    return u >= 0.0f && u < (float)Q.width && v >= 0.0f && v < (float)Q.height;
}
__device__ __forceinline__ bool hv_frustum_contains(const HvQuery &Q, float xw, float yw, float zw, float *uvd) {
    return hv_frustum_contains_d(Q, (double)xw, (double)yw, (double)zw, uvd);
}

static inline void fill_frustum_query(HvQuery &Q, const float *intr, int width, int height, const double *T_cw, float depth_max,
                                      float depth_min) {
    Q.fx = intr[0];
    Q.fy = intr[1];
    Q.cx = intr[2];
    Q.cy = intr[3];
    Q.width = width;
    Q.height = height;
    Q.depth_max = depth_max;
    Q.depth_min = depth_min;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) Q.R[r * 3 + c] = T_cw[r * 4 + c];
        Q.t[r] = T_cw[r * 4 + 3];
    }
    // compute_frustum_corners_world_ + compute_bbox_, camera_frustrum.cpp:209-264
    double Rwc[9], twc[3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) Rwc[r * 3 + c] = Q.R[c * 3 + r];
    for (int r = 0; r < 3; ++r) twc[r] = -(Rwc[r * 3 + 0] * Q.t[0] + Rwc[r * 3 + 1] * Q.t[1] + Rwc[r * 3 + 2] * Q.t[2]);
    const double cu[4] = {0.0, (double)width, (double)width, 0.0};
    const double cv[4] = {0.0, 0.0, (double)height, (double)height};
    for (int k = 0; k < 3; ++k) {
        Q.bb[k] = 1.7976931348623157e308;
        Q.bb[3 + k] = -1.7976931348623157e308;
    }
    for (int i = 0; i < 4; ++i) {
        const double xn = (cu[i] - (double)Q.cx) / (double)Q.fx;
        const double yn = (cv[i] - (double)Q.cy) / (double)Q.fy;
        const double ds[2] = {(double)depth_min, (double)depth_max};
        for (int j = 0; j < 2; ++j) {
            const double pc[3] = {xn * ds[j], yn * ds[j], ds[j]};
            for (int r = 0; r < 3; ++r) {
                const double w = (Rwc[r * 3 + 0] * pc[0] + Rwc[r * 3 + 1] * pc[1] + Rwc[r * 3 + 2] * pc[2]) + twc[r];
                if (w < Q.bb[r]) Q.bb[r] = w;
                if (w > Q.bb[3 + r]) Q.bb[3 + r] = w;
            }
        }
    }
}

// bbox -> voxel/block key range, voxel_block_grid.hpp:827-835: get_voxel_key_inv<double,double>
// with the float inv_voxel_size_ promoted to double.
static inline void fill_key_range(HvQuery &Q, const hv_volume *v) {
    const HvGridParams G = grid_params(v); // (voxel size and block size: the same in every grid mode)
    for (int k = 0; k < 3; ++k) {
        Q.vmin[k] = (int32_t)std::floor(Q.bb[k] * (double)G.inv_voxel_size);
        Q.vmax[k] = (int32_t)std::floor(Q.bb[3 + k] * (double)G.inv_voxel_size);
        Q.bmin[k] = hv_floor_div(Q.vmin[k], G.bs);
        Q.bmax[k] = hv_floor_div(Q.vmax[k], G.bs);
    }
}

// The three queries of get_voxels / get_voxels_in_bb / get_voxels_in_camera_frustrum (and, as kind 3, carve), ready for a kernel.
static inline HvQuery hv_query_all(int32_t min_count) {
    HvQuery Q;
    memset(&Q, 0, sizeof(Q));
    Q.min_count = min_count;
    return Q;
}
static inline HvQuery hv_query_in_bb(const hv_volume *v, const double *bbox, int32_t min_count) {
    HvQuery Q = hv_query_all(min_count);
    Q.kind = 1;
    for (int k = 0; k < 6; ++k) Q.bb[k] = bbox[k];
    fill_key_range(Q, v);
    return Q;
}
static inline HvQuery hv_query_in_frustum(const hv_volume *v, const float *intr, int width, int height, const double *T_cw, float depth_max,
                                          float depth_min, int32_t min_count, int32_t kind = 2) {
    HvQuery Q = hv_query_all(min_count);
    Q.kind = kind;
    fill_frustum_query(Q, intr, width, height, T_cw, depth_max, depth_min);
    fill_key_range(Q, v);
    return Q;
}

// ---- host halves the VOXEL_GRID and the semantic scans share --------------------------------------
// a wave per block of the pool, grid-stride: workgroups of 256
static inline unsigned hv_wave_per_block_grid(int64_t nb) { return (unsigned)std::min<int64_t>((nb + 3) / 4, 8192); }

// the prologue of a scan over the allocated blocks: the volume's device, the number of blocks (0: an empty map, nothing to launch)
static inline int hv_scan_begin(hv_volume *v, int64_t *nb) {
    HV_HIP(hipSetDevice(v->device));
    return hv_num_blocks(v, nb);
}

// A collecting scan: `launch()` queues the kernel that counts its rows in HV_CNT_OUT (and writes the first `cap` of them to device
// arrays); *n receives the count, and min(*n, cap) rows of every {host, device, bytes per row} triple in `back` are copied back.
struct HvRowsBack {
    void *host;
    const void *dev;
    size_t row_bytes;
};
template <typename Launch>
static int hv_collect_rows(hv_volume *v, int64_t cap, int64_t *n, Launch launch, std::initializer_list<HvRowsBack> back) {
    HV_HIP(hipMemsetAsync(&v->table.counters[HV_CNT_OUT], 0, sizeof(int32_t), v->stream));
    launch();
    HV_HIP(hipGetLastError());
    const int rc = hv_read_counters(v);
    if (rc != HV_OK) return rc;
    *n = v->h_counters[HV_CNT_OUT];
    const int64_t m = std::min(*n, cap);
    if (m <= 0 || back.size() == 0) return HV_OK;
    for (const HvRowsBack &b : back) HV_HIP(hipMemcpyAsync(b.host, b.dev, b.row_bytes * (size_t)m, hipMemcpyDeviceToHost, v->stream));
    HV_HIP(hipStreamSynchronize(v->stream));
    return HV_OK;
}

// The map's blocks in ascending (x, y, z) key order, as the dumps list them: xyz[i] = key of pool block i, order[o] = the pool block
// at place o.
static inline int hv_blocks_in_key_order(hv_volume *v, int64_t nb, std::vector<std::array<int32_t, 3>> &xyz, std::vector<int64_t> &order) {
    std::vector<uint64_t> bkeys((size_t)nb);
    HV_HIP(hipMemcpy(bkeys.data(), v->table.block_keys, sizeof(uint64_t) * nb, hipMemcpyDeviceToHost));
    xyz.resize((size_t)nb);
    for (int64_t i = 0; i < nb; ++i) hv_unpack_key(bkeys[i], xyz[i][0], xyz[i][1], xyz[i][2]);
    order.resize((size_t)nb);
    std::iota(order.begin(), order.end(), 0);
    std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return xyz[a] < xyz[b]; });
    return HV_OK;
}

// semantic-payload implementations behind the mode-independent entry points (hv_semantic_ops.hip)
int hv_sem_carve(hv_volume *v, const HvQuery &Q, const float *d_depth, int64_t n_blocks);
int hv_sem_segment_op(hv_volume *v, int op, int32_t a, int32_t b, float fa);
int hv_sem_size(hv_volume *v, int64_t *n);
int hv_unproject_frame(hv_volume *v, const void *depth, int32_t depth_dtype, double depth_scale, const uint8_t *rgb,
                       int32_t height, int32_t width, const double *intr, const double *T_cw, double min_depth,
                       double max_depth, int32_t loc, const void **d_depth_out); // hv_voxel_grid.hip
