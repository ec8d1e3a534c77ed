// The cell of the TSDF contract (include/hipvol.h), written once: where a point falls in the voxel lattice, the order of the eight
// voxels around it, the trilinear value and its gradient, and - on the device - where those voxels lie in the pool.  Every query
// that samples the map (hv_sample.hip, hv_register.hip, hv_merge.hip, hv_raycast.hip, hv_tsdf_sample.h) takes these from here; the
// numpy restatements under tests/ are compared with them for equality, so an operation or its order changes here or nowhere.
//
// The arithmetic part needs <cmath> and <cstdint> only: a host program includes this header without HIP
// (tests/test_tsdf_cell_cpu.py does).  The library is built with -ffp-contract=off: every product and sum below is one IEEE operation.
#pragma once
#include <cmath>
#include <cstdint>

#ifdef __HIPCC__
#define HV_HD __host__ __device__ __forceinline__
#else
#define HV_HD inline
#endif

static constexpr double HV_CELL_LIMIT = 1.0e9; // lattice coordinates of this magnitude and beyond name no voxel

// Point p -> its cell: g = p / voxel_length - 0.5 per axis, g0 = floor(g), r = g - g0 in [0, 1).  false: p lies outside every
// representable voxel (|g| >= 1e9 or not finite); g0 is 0 from the first such axis on and r means nothing.
HV_HD bool hv_cell_locate(const double *p, double voxel_length, int32_t *g0, double *r) {
    bool ok = true;
#ifdef __HIPCC__
#pragma unroll
#endif
    for (int a = 0; a < 3; ++a) {
        const double g = p[a] / voxel_length - 0.5;
        ok = ok && fabs(g) < HV_CELL_LIMIT;
        const double f = floor(g);
        g0[a] = ok ? (int32_t)f : 0;
        r[a] = g - f;
    }
    return ok;
}

// Corner c of a cell is voxel g0 + (sx, sy, sz): Open3D's order, x + (c in {1,2,5,6}), y + (c in {2,3,6,7}), z + (c >= 4).
HV_HD void hv_cell_corner(int c, int &sx, int &sy, int &sz) {
    sx = (c == 1 || c == 2 || c == 5 || c == 6);
    sy = (c == 2 || c == 3 || c == 6 || c == 7);
    sz = c >= 4;
}

// Trilinear value of the eight corner values f at r: along z, then y, then x (T = double, or float for the ray caster).
template <typename T>
HV_HD T hv_cell_lerp(const T *r, const T *f) {
    const T u0 = 1 - r[0], u1 = 1 - r[1], u2 = 1 - r[2];
    const T c00 = u2 * f[0] + r[2] * f[4], c01 = u2 * f[3] + r[2] * f[7];
    const T c10 = u2 * f[1] + r[2] * f[5], c11 = u2 * f[2] + r[2] * f[6];
    const T b0 = u1 * c00 + r[1] * c01, b1 = u1 * c10 + r[1] * c11;
    return u0 * b0 + r[0] * b1;
}

// ... and with its gradient e = d phi / d r (per voxel: the caller scales it)
HV_HD void hv_cell_lerp_grad(const double *r, const double *f, double &phi, double *e) {
    const double u0 = 1 - r[0], u1 = 1 - r[1], u2 = 1 - r[2];
    const double c00 = u2 * f[0] + r[2] * f[4], c01 = u2 * f[3] + r[2] * f[7];
    const double c10 = u2 * f[1] + r[2] * f[5], c11 = u2 * f[2] + r[2] * f[6];
    const double b0 = u1 * c00 + r[1] * c01, b1 = u1 * c10 + r[1] * c11;
    phi = u0 * b0 + r[0] * b1;
    e[0] = b1 - b0;
    e[1] = u0 * (c01 - c00) + r[0] * (c11 - c10);
    e[2] = u0 * (u1 * (f[4] - f[0]) + r[1] * (f[7] - f[3])) + r[0] * (u1 * (f[5] - f[1]) + r[1] * (f[6] - f[2]));
}

#ifdef __HIPCC__
#include "hv_common.h"

// pool index of unit (kx, ky, kz), -1 if the map does not hold it - or holds it at an index >= used (INT32_MAX: no such bound)
__device__ __forceinline__ int32_t hv_tsdf_unit_index(const HvTable &table, int32_t kx, int32_t ky, int32_t kz, int32_t used) {
    if (!hv_key_in_range(kx, ky, kz)) return -1;
    const int32_t slot = hv_table_find(table, hv_pack_key(kx, ky, kz));
    const int32_t idx = slot >= 0 ? table.vals[slot] : -1;
    return idx >= 0 && idx < used ? idx : -1;
}

// ... for a lane that asks for one voxel after another: the last key looked up and its index are cached in (cached_key, cached_idx)
__device__ __forceinline__ int32_t hv_tsdf_unit(const HvTable &table, int32_t ux, int32_t uy, int32_t uz, unsigned long long &cached_key,
                                                int32_t &cached_idx) {
    if (!hv_key_in_range(ux, uy, uz)) return -1;
    const unsigned long long key = hv_pack_key(ux, uy, uz);
    if (key != cached_key) {
        const int32_t slot = hv_table_find(table, key);
        cached_key = key;
        cached_idx = slot >= 0 ? table.vals[slot] : -1;
    }
    return cached_idx;
}

// voxel (gx, gy, gz) in global voxel indices: pool index of its unit (or -1) and its word inside the unit's planes
__device__ __forceinline__ int32_t hv_tsdf_voxel_at(const HvTable &table, int32_t gx, int32_t gy, int32_t gz, unsigned long long &ck,
                                                    int32_t &ci, int &word) {
    word = hv_tsdf_word(gx & (HV_TSDF_R - 1), gy & (HV_TSDF_R - 1), gz & (HV_TSDF_R - 1));
    return hv_tsdf_unit(table, gx >> 4, gy >> 4, gz >> 4, ck, ci);
}

// The eight voxels of cell g0: at[c] = word offset of corner c's tsdf from the pool's start (its weight lies HV_TSDF_RRR words on,
// the colour sums behind that); bit c of the result = the map holds corner c's unit (at[c] of an absent unit points into unit 0).
__device__ __forceinline__ uint32_t hv_tsdf_cell_gather(const HvTable &table, const int32_t *g0, unsigned long long &ck, int32_t &ci,
                                                        int64_t *at) {
    uint32_t held = 0u;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        int sx, sy, sz, word;
        hv_cell_corner(c, sx, sy, sz);
        const int32_t idx = hv_tsdf_voxel_at(table, g0[0] + sx, g0[1] + sy, g0[2] + sz, ck, ci, word);
        at[c] = (int64_t)(idx < 0 ? 0 : idx) * (HV_TSDF_UNIT_BYTES / 4) + word;
        held |= idx >= 0 ? 1u << c : 0u;
    }
    return held;
}
#endif // __HIPCC__
