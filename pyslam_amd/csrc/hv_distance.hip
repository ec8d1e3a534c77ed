// libpyslam_hipvol.so — the distance field of the TSDF map on gfx950 (hv_tsdf_distance_field): a dense signed Euclidean distance over a
// box of the map's own voxel lattice, out to a radius of R voxels, beyond the truncation band.  The contract (state, site, the three
// windowed passes, cap, square root and sign) is written once in include/hipvol.h; tests/distance_reference.py restates it in numpy.
//
// Four launches over a grid of nx x ny x nz cells (z fastest), all integer until the last instruction:
//   k_dist_classify   one workgroup per 16^3 brick of the box, aligned to the map's units: the classification halo of hv_tsdf_sites.h
//                     (seven hash probes, the unit's planes, the six neighbour faces, the states in an 18^3 LDS halo); clips to the
//                     box and writes the class byte and the seed (0 at a site, DF_INF elsewhere).  A brick whose unit is not held
//                     writes UNKNOWN / DF_INF and reads nothing of the pool.
//   k_dist_scan_x     one lane per (y, z) column: a forward and a backward scan along x (distance to the last site seen), no window
//                     walk; for a fixed x the lanes of a wave read and write consecutive words.
//   k_dist_pass_y     one workgroup per (x, group of ZT consecutive z): the whole ny x ZT slab staged in LDS (ZT * 4 bytes contiguous
//                     per row), then every cell walks outward k = 0, 1, ... along y until k^2 >= its best; written back in place.
//   k_dist_pass_z     one workgroup per group of LT whole z lines (contiguous memory): the same walk along z, fused with the cap, the
//                     square root, the sign and the counts (one integer atomic per wave and counter, after ballots).
// No float atomics, no atomics on values, no scratch memory per lane.  The kernels read the table and the pool only.
#include <algorithm>
#include <cmath>

#include "hv_common.h"
#include "hv_tsdf_device.h"
#include "hv_tsdf_sites.h"

namespace {

constexpr uint32_t DF_INF = 0x3fffffffu; // "no site within the window": above every sum of three squares <= 3 * 1024^2, and + 1024^2 fits
constexpr int DF_LINE_WORDS = 8192;      // LDS words a pass aims to stage per workgroup (32 KiB: several workgroups per CU)
constexpr int DF_LINE_WORDS_MAX = 16384; // ... and never exceeds (a 4096-cell line times the narrowest slab, 64 KiB)
enum { DF_N_UNKNOWN = 0, DF_N_FREE = 1, DF_N_INSIDE = 2, DF_N_SITES = 3, DF_N_FAR = 4, DF_N_COUNT = 5 };

struct HvDistGrid {
    int32_t o[3]; // voxel index of cell (0, 0, 0)
    int32_t n[3]; // cells per axis
    int32_t u[3]; // unit index of brick (0, 0, 0)
    int32_t R;
};

__global__ __launch_bounds__(256) void k_dist_classify(HvTable table, const char *__restrict__ pool, HvDistGrid G, double thr,
                                                       uint8_t *__restrict__ cls, uint32_t *__restrict__ seed) {
    __shared__ uint8_t st[HV_SITE_HALO_CELLS];
    __shared__ int32_t unit_idx[7]; // the brick's unit, then its -x +x -y +y -z +z neighbours
    const int t = (int)threadIdx.x;
    const int32_t ux = G.u[0] + (int32_t)blockIdx.x, uy = G.u[1] + (int32_t)blockIdx.y, uz = G.u[2] + (int32_t)blockIdx.z;
    hv_site_halo_units(table, ux, uy, uz, INT32_MAX, -1, unit_idx);
    __syncthreads();
    const int32_t self = unit_idx[0];
    // cells of this thread: one (y, z) of the brick, all x - a wave writes runs of 16 consecutive z
    const int lz = t & 15, ly = t >> 4;
    const int32_t j = uy * HV_TSDF_R + ly - G.o[1], k = uz * HV_TSDF_R + lz - G.o[2];
    const bool in_yz = j >= 0 && j < G.n[1] && k >= 0 && k < G.n[2];
    const int32_t i0 = ux * HV_TSDF_R - G.o[0];
    if (self >= 0) hv_site_halo_load(pool, unit_idx, thr, st);
    __syncthreads();
    if (!in_yz) return;
#pragma unroll 4
    for (int lx = 0; lx < HV_TSDF_R; ++lx) {
        const int32_t i = i0 + lx;
        if (i < 0 || i >= G.n[0]) continue;
        uint32_t c = HV_DIST_UNKNOWN;
        if (self >= 0) {
            const int at = hv_site_halo_at(lx, ly, lz);
            c = st[at] | (hv_site_is_site(st, at) ? (uint32_t)HV_DIST_SITE : 0u);
        }
        const int64_t cell = ((int64_t)i * G.n[1] + j) * G.n[2] + k;
        cls[cell] = (uint8_t)c;
        if (seed != nullptr) seed[cell] = (c & HV_DIST_SITE) ? 0u : DF_INF;
    }
}

// g: seeds in, g1 out.  plane = ny * nz; lane = one column, so the accesses of a wave at a fixed x are consecutive.
__global__ __launch_bounds__(256) void k_dist_scan_x(uint32_t *__restrict__ g, int32_t nx, int64_t plane, int32_t R) {
    const int64_t col = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (col >= plane) return;
    uint32_t d = DF_INF; // cells since the last site, saturating
    for (int32_t x = 0; x < nx; ++x) {
        uint32_t *p = g + (int64_t)x * plane + col;
        d = *p == 0u ? 0u : min(d + 1u, DF_INF);
        *p = d;
    }
    d = DF_INF;
    for (int32_t x = nx - 1; x >= 0; --x) {
        uint32_t *p = g + (int64_t)x * plane + col;
        const uint32_t fwd = *p;
        d = fwd == 0u ? 0u : min(d + 1u, DF_INF);
        const uint32_t m = min(fwd, d);
        *p = m <= (uint32_t)R ? m * m : DF_INF;
    }
}

// min over |k| <= R of line[(pos + k) * stride] + k^2, walking outward: a later k cannot improve a best <= k^2.
__device__ __forceinline__ uint32_t df_walk(const uint32_t *line, int pos, int len, int stride, int R) {
    uint32_t best = line[pos * stride];
    const int reach = min(R, max(pos, len - 1 - pos));
    for (int k = 1; k <= reach; ++k) {
        const uint32_t kk = (uint32_t)(k * k);
        if (kk >= best) break;
        if (pos - k >= 0) best = min(best, line[(pos - k) * stride] + kk);
        if (pos + k < len) best = min(best, line[(pos + k) * stride] + kk);
    }
    return best;
}

// g1 -> g2 in place.  blockIdx.y = x, blockIdx.x = the group of zt consecutive z; LDS [ny][zt].
__global__ __launch_bounds__(256) void k_dist_pass_y(uint32_t *__restrict__ g, int32_t ny, int32_t nz, int32_t zt, int32_t R) {
    extern __shared__ uint32_t df_line[];
    const int z0 = (int)blockIdx.x * zt;
    uint32_t *base = g + (int64_t)blockIdx.y * ny * nz;
    const int total = ny * zt;
    for (int e = (int)threadIdx.x; e < total; e += 256) {
        const int y = e / zt, z = z0 + (e - y * zt);
        df_line[e] = z < nz ? base[(int64_t)y * nz + z] : DF_INF;
    }
    __syncthreads();
    // the slab is this workgroup's alone and staged whole: results go straight back to memory
    for (int e = (int)threadIdx.x; e < total; e += 256) {
        const int y = e / zt, zz = e - y * zt, z = z0 + zz;
        if (z < nz) base[(int64_t)y * nz + z] = df_walk(df_line + zz, y, ny, zt, R);
    }
}

// g2 -> dist2, distance, counts.  One workgroup per lt whole z lines, contiguous in memory; LDS [lt][nz].
__global__ __launch_bounds__(256) void k_dist_pass_z(uint32_t *__restrict__ g, const uint8_t *__restrict__ cls, int64_t lines, int32_t nz,
                                                     int32_t lt, int32_t R, float voxel_length, int write_dist2,
                                                     float *__restrict__ distance, unsigned long long *__restrict__ count) {
    extern __shared__ uint32_t df_line[];
    const int64_t l0 = (int64_t)blockIdx.x * lt;
    const int nl = lines - l0 < (int64_t)lt ? (int)(lines - l0) : lt;
    const int64_t base = l0 * nz;
    const int total = nl * nz;
    for (int e = (int)threadIdx.x; e < total; e += 256) df_line[e] = g[base + e];
    __syncthreads();
    const uint32_t cap = (uint32_t)R * (uint32_t)R;
    uint32_t n[DF_N_COUNT] = {0u, 0u, 0u, 0u, 0u}; // wave-uniform
    for (int e0 = 0; e0 < total; e0 += 256) {
        const int e = e0 + (int)threadIdx.x;
        const bool live = e < total;
        uint32_t c = 0u, d2 = 0u;
        if (live) {
            const int l = e / nz, z = e - l * nz;
            d2 = min(df_walk(df_line + l * nz, z, nz, 1, R), cap);
            c = cls[base + e];
            if (write_dist2) g[base + e] = d2;
            if (distance != nullptr) {
                const float root = d2 == 0u ? 0.0f : hv_sqrt_ge1((float)d2);
                distance[base + e] = ((c & 3u) == HV_DIST_INSIDE ? -1.0f : 1.0f) * (root * voxel_length);
            }
        }
        if (count != nullptr) {
            n[DF_N_UNKNOWN] += (uint32_t)__popcll(__ballot(live && (c & 3u) == HV_DIST_UNKNOWN));
            n[DF_N_FREE] += (uint32_t)__popcll(__ballot(live && (c & 3u) == HV_DIST_FREE));
            n[DF_N_INSIDE] += (uint32_t)__popcll(__ballot(live && (c & 3u) == HV_DIST_INSIDE));
            n[DF_N_SITES] += (uint32_t)__popcll(__ballot(live && (c & HV_DIST_SITE) != 0u));
            n[DF_N_FAR] += (uint32_t)__popcll(__ballot(live && d2 == cap));
        }
    }
    if (count != nullptr && hv_lane_id() == 0) {
#pragma unroll
        for (int q = 0; q < DF_N_COUNT; ++q)
            if (n[q] != 0u) atomicAdd(&count[q], (unsigned long long)n[q]);
    }
}

} // namespace

extern "C" int hv_tsdf_distance_field(hv_volume *v, const hv_distance_params *p, float *distance, uint32_t *dist2, uint8_t *cls,
                                      hv_distance_stats *stats, int32_t loc) {
    const char *fn = "hv_tsdf_distance_field";
    HV_REQUIRE(v != nullptr, HV_ERR_INVALID, "%s: null argument", fn);
    {
        const int rc = hv_tsdf_require_whole_map(v, fn, "the volume");
        if (rc != HV_OK) return rc;
    }
    HV_REQUIRE(p != nullptr, HV_ERR_INVALID, "%s: null params", fn);
    for (int a = 0; a < 3; ++a) {
        HV_REQUIRE(p->shape[a] >= 1 && p->shape[a] <= HV_DIST_MAX_SHAPE, HV_ERR_INVALID, "%s: shape[%d] = %d is outside 1..%d", fn, a,
                   (int)p->shape[a], HV_DIST_MAX_SHAPE);
        HV_REQUIRE(p->origin[a] >= -(1 << 30) && p->origin[a] <= (1 << 30), HV_ERR_INVALID, "%s: origin[%d] = %d is outside +-2^30", fn, a,
                   (int)p->origin[a]);
    }
    const int64_t cells = (int64_t)p->shape[0] * p->shape[1] * p->shape[2];
    HV_REQUIRE(cells <= (int64_t)INT32_MAX, HV_ERR_INVALID, "%s: %lld cells exceed 2^31 - 1", fn, (long long)cells);
    HV_REQUIRE(p->radius >= 1 && p->radius <= HV_DIST_MAX_RADIUS, HV_ERR_INVALID, "%s: radius %d is outside 1..%d", fn, (int)p->radius,
               HV_DIST_MAX_RADIUS);
    HV_REQUIRE(std::isfinite(p->weight_threshold) && p->weight_threshold >= 0.0, HV_ERR_INVALID,
               "%s: weight_threshold must be finite and >= 0", fn);
    HV_REQUIRE(loc == HV_HOST || loc == HV_DEVICE, HV_ERR_INVALID, "%s: bad loc %d", fn, (int)loc);
    HV_HIP(hipSetDevice(v->device));

    // the transform runs when something needs it; a call for the classes alone stops after the classification
    const bool passes = distance != nullptr || dist2 != nullptr || stats != nullptr;
    // head: [5 counters, 256 B][grid u32, unless the caller's dist2 takes it][classes, unless the caller's cls does]; an output the
    // caller asked for is the caller's own array (HV_DEVICE) or a staged piece (HV_HOST)
    const size_t n = (size_t)cells, pad = 255;
    const size_t off_grid = 256, off_cls = off_grid + (passes && dist2 == nullptr ? (4 * n + pad) & ~pad : 0);
    HvStage st(v, loc);
    st.head(off_cls + (cls == nullptr ? (n + pad) & ~pad : 0));
    const int o_dist = st.out(distance, 4 * n), o_grid = st.out(dist2, 4 * n), o_cls = st.out(cls, n);
    int rc = st.commit(&v->dist_buf, &v->dist_buf_bytes);
    if (rc != HV_OK) return rc;
    char *buf = (char *)st.head_dev;
    unsigned long long *d_count = stats != nullptr ? (unsigned long long *)buf : nullptr;
    uint32_t *d_grid = !passes ? nullptr : (dist2 != nullptr ? st.dev<uint32_t>(o_grid) : (uint32_t *)(buf + off_grid));
    uint8_t *d_cls = cls != nullptr ? st.dev<uint8_t>(o_cls) : (uint8_t *)(buf + off_cls);
    float *d_dist = st.dev<float>(o_dist);
    // reads only, as hv_tsdf_ray_cast: the next batch starts a fresh touch + pack chain behind this call
    v->pipe_armed = false;

    HvDistGrid G{};
    int32_t bricks[3];
    for (int a = 0; a < 3; ++a) {
        G.o[a] = p->origin[a];
        G.n[a] = p->shape[a];
        G.u[a] = p->origin[a] >> 4;
        bricks[a] = ((p->origin[a] + p->shape[a] - 1) >> 4) - G.u[a] + 1;
    }
    G.R = p->radius;
    const int32_t nx = G.n[0], ny = G.n[1], nz = G.n[2];
    if (d_count != nullptr) HV_HIP(hipMemsetAsync(d_count, 0, DF_N_COUNT * sizeof(unsigned long long), v->stream));
    hv_profile_begin(v);
    hipLaunchKernelGGL(k_dist_classify, dim3((unsigned)bricks[0], (unsigned)bricks[1], (unsigned)bricks[2]), dim3(256), 0, v->stream, v->table,
                       (const char *)v->pool, G, p->weight_threshold, d_cls, d_grid);
    hv_profile_end(v, 0);
    if (passes) {
        const int64_t plane = (int64_t)ny * nz;
        hv_profile_begin(v);
        hipLaunchKernelGGL(k_dist_scan_x, dim3((unsigned)((plane + 255) / 256)), dim3(256), 0, v->stream, d_grid, nx, plane, G.R);
        hv_profile_end(v, 0);
        // z per slab of the y pass: as many as DF_LINE_WORDS hold, at least 4 (16 contiguous bytes per row), no more than nz needs
        int zt = 64;
        while (zt > 4 && (int64_t)ny * zt > DF_LINE_WORDS) zt >>= 1;
        while (zt > 1 && zt / 2 >= nz) zt >>= 1;
        static_assert(4 * HV_DIST_MAX_SHAPE <= DF_LINE_WORDS_MAX, "the narrowest slab of the longest line fits");
        hv_profile_begin(v);
        hipLaunchKernelGGL(k_dist_pass_y, dim3((unsigned)((nz + zt - 1) / zt), (unsigned)nx), dim3(256), (size_t)ny * zt * 4, v->stream, d_grid,
                           ny, nz, zt, G.R);
        hv_profile_end(v, 0);
        const int64_t lines = (int64_t)nx * ny;
        const int lt = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(64, lines), DF_LINE_WORDS / nz));
        hv_profile_begin(v);
        hipLaunchKernelGGL(k_dist_pass_z, dim3((unsigned)((lines + lt - 1) / lt)), dim3(256), (size_t)lt * nz * 4, v->stream, d_grid,
                           (const uint8_t *)d_cls, lines, nz, lt, G.R, (float)v->cfg.voxel_size, dist2 != nullptr ? 1 : 0, d_dist, d_count);
        hv_profile_end(v, 0);
    }
    HV_HIP(hipGetLastError());
    unsigned long long h[DF_N_COUNT];
    rc = st.finish(stats != nullptr ? h : nullptr, sizeof(h));
    if (rc != HV_OK) return rc;
    if (stats != nullptr) {
        stats->unknown = (int64_t)h[DF_N_UNKNOWN];
        stats->free = (int64_t)h[DF_N_FREE];
        stats->inside = (int64_t)h[DF_N_INSIDE];
        stats->sites = (int64_t)h[DF_N_SITES];
        stats->far = (int64_t)h[DF_N_FAR];
    }
    return HV_OK;
}
