// Point samplers of the TSDF field, shared by surface extraction (hv_extract.hip) and ray casting (hv_raycast.hip).
//
// hv_tsdf_at is Open3D's ScalableTSDFVolume::GetTSDFAt: the trilinear interpolation of the eight voxels around a position.  It
// does not look at weights (a voxel never observed holds its initial tsdf 0) and a missing unit contributes 0.  The unit of the
// previous fetch is remembered by the caller (ck / ci: most of the fetches of one point fall into one or two units); the
// locate is Open3D's, in double; the corner order and the trilinear form are the contract's (hv_tsdf_cell.h).  hv_tsdf_gradient
// is GetNormalAt before normalisation: central differences, at +/- 0.99 voxel along each axis, of GetTSDFAt.
#pragma once
#include "hv_common.h"
#include "hv_tsdf_cell.h"

#ifdef __HIPCC__
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
    double f[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        int sx, sy, sz;
        hv_cell_corner(i, sx, sy, sz);
        int x = idx0[0] + sx, y = idx0[1] + sy, z = idx0[2] + sz;
        const int32_t ux = index0[0] + (x >= HV_TSDF_R), uy = index0[1] + (y >= HV_TSDF_R), uz = index0[2] + (z >= HV_TSDF_R);
        f[i] = (double)hv_tsdf_voxel(table, pool, ux, uy, uz, x & (HV_TSDF_R - 1), y & (HV_TSDF_R - 1), z & (HV_TSDF_R - 1), ck, ci);
    }
    return hv_cell_lerp(r, f);
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
