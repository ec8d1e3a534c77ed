// Point samplers of the TSDF field, shared by surface extraction (hv_extract.hip) and ray casting (hv_raycast.hip).
//
// hv_tsdf_at is Open3D's ScalableTSDFVolume::GetTSDFAt: the trilinear interpolation of the eight voxels around a position.  It
// does not look at weights (a voxel never observed holds its initial tsdf 0) and a missing unit contributes 0.  The unit of the
// previous fetch is remembered by the caller (ck / ci: most of the fetches of one point fall into one or two units); the
// arithmetic is Open3D's, in double.  hv_tsdf_gradient is GetNormalAt before normalisation: central differences, at +/- 0.99
// voxel along each axis, of GetTSDFAt.
#pragma once
#include "hv_common.h"

#ifdef __HIPCC__
// pool index of unit (ux, uy, uz), -1 if absent; the last key looked up and its index are cached in (cached_key, cached_idx)
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

__device__ __forceinline__ float hv_tsdf_voxel(const HvTable &table, const char *__restrict__ pool, int32_t ux, int32_t uy, int32_t uz,
                                               int x, int y, int z, unsigned long long &cached_key, int32_t &cached_idx) {
    const int32_t idx = hv_tsdf_unit(table, ux, uy, uz, cached_key, cached_idx);
    if (idx < 0) return 0.0f;
    return ((const float *)(pool + (int64_t)idx * HV_TSDF_UNIT_BYTES))[hv_tsdf_word(x, y, z)];
}

__device__ inline double hv_tsdf_at(const HvTable &table, const char *__restrict__ pool, double voxel_length, double unit_length,
                                    const double *p, unsigned long long &ck, int32_t &ci) {
    int32_t index0[3];
    int idx0[3];
    double r[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double p_locate = p[i] - 0.5 * voxel_length;
        index0[i] = (int32_t)floor(p_locate / unit_length);
        const double p_grid = (p_locate - (double)index0[i] * unit_length) / voxel_length;
        int q = (int)floor(p_grid);
        q = q < 0 ? 0 : (q >= HV_TSDF_R ? HV_TSDF_R - 1 : q);
        idx0[i] = q;
        r[i] = p_grid - (double)q;
    }
    {   // the unit of p itself decides "no such unit -> 0" (GetTSDFAt returns before looking at neighbours)
        unsigned long long k0 = HV_EMPTY_KEY;
        int32_t i0 = -1;
        (void)hv_tsdf_voxel(table, pool, index0[0], index0[1], index0[2], 0, 0, 0, k0, i0);
        if (i0 < 0) return 0.0;
        ck = k0;
        ci = i0;
    }
    float f[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int sx = (i == 1 || i == 2 || i == 5 || i == 6), sy = (i == 2 || i == 3 || i == 6 || i == 7), sz = i >= 4;
        int x = idx0[0] + sx, y = idx0[1] + sy, z = idx0[2] + sz;
        const int32_t ux = index0[0] + (x >= HV_TSDF_R), uy = index0[1] + (y >= HV_TSDF_R), uz = index0[2] + (z >= HV_TSDF_R);
        f[i] = hv_tsdf_voxel(table, pool, ux, uy, uz, x & (HV_TSDF_R - 1), y & (HV_TSDF_R - 1), z & (HV_TSDF_R - 1), ck, ci);
    }
    return (1 - r[0]) * ((1 - r[1]) * ((1 - r[2]) * f[0] + r[2] * f[4]) + r[1] * ((1 - r[2]) * f[3] + r[2] * f[7])) +
           r[0] * ((1 - r[1]) * ((1 - r[2]) * f[1] + r[2] * f[5]) + r[1] * ((1 - r[2]) * f[2] + r[2] * f[6]));
}

// GetNormalAt's unnormalised gradient at p (nn[i] = tsdf(p + 0.99 vl e_i) - tsdf(p - 0.99 vl e_i))
__device__ inline void hv_tsdf_gradient(const HvTable &table, const char *__restrict__ pool, double voxel_length, double unit_length,
                                        const double *p, unsigned long long &ck, int32_t &ci, double *nn) {
    const double half_gap = 0.99 * voxel_length;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        double p0[3] = {p[0], p[1], p[2]}, p1[3] = {p[0], p[1], p[2]};
        p0[i] -= half_gap;
        p1[i] += half_gap;
        nn[i] = hv_tsdf_at(table, pool, voxel_length, unit_length, p1, ck, ci) - hv_tsdf_at(table, pool, voxel_length, unit_length, p0, ck, ci);
    }
}
#endif // __HIPCC__
