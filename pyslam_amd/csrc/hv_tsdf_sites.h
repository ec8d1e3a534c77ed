// The surface sites of the TSDF contract (include/hipvol.h: state, site), written once for the kernels that walk them
// (k_dist_classify in hv_distance.hip, k_cc_sites in hv_components.hip): a workgroup of 256 threads classifies the 16^3 voxels of
// one unit and the faces of its six neighbours into an 18^3 halo of states in LDS, and a voxel is a site when a face neighbour
// holds the opposite state.  tests/distance_reference.py restates the rule in numpy.
//
// The caller owns the LDS (uint8_t st[HV_SITE_HALO_CELLS], int32_t unit_idx[7]) and the two barriers: one between
// hv_site_halo_units and hv_site_halo_load, one between hv_site_halo_load and the first hv_site_is_site.
#pragma once
#include "hv_tsdf_cell.h"

#ifdef __HIPCC__
constexpr int HV_SITE_H = HV_TSDF_R + 2; // side of the state halo
constexpr int HV_SITE_HALO_CELLS = HV_SITE_H * HV_SITE_H * HV_SITE_H;

__device__ __forceinline__ uint32_t hv_site_state(uint32_t w, float f, double thr) {
    return (double)w > thr ? (f <= 0.0f ? (uint32_t)HV_DIST_INSIDE : (uint32_t)HV_DIST_FREE) : (uint32_t)HV_DIST_UNKNOWN;
}
// halo cell of voxel (x, y, z) of the unit, each in -1 .. 16
__device__ __forceinline__ int hv_site_halo_at(int x, int y, int z) { return ((x + 1) * HV_SITE_H + (y + 1)) * HV_SITE_H + (z + 1); }

// unit_idx[0 .. 6] = pool index (-1: absent, or at an index >= used) of unit (ux, uy, uz), then of its -x +x -y +y -z +z neighbours:
// one hash probe each by threads 0 .. 6.  self >= 0: the caller knows the unit's own index, entry 0 is not probed.
__device__ __forceinline__ void hv_site_halo_units(const HvTable &table, int32_t ux, int32_t uy, int32_t uz, int32_t used, int32_t self,
                                                   int32_t *unit_idx) {
    const int t = (int)threadIdx.x;
    if (t < 7)
        unit_idx[t] = t == 0 && self >= 0
                          ? self
                          : hv_tsdf_unit_index(table, ux + (t == 2) - (t == 1), uy + (t == 4) - (t == 3), uz + (t == 6) - (t == 5), used);
}

// The states of unit unit_idx[0] (held) and of the facing voxels of its neighbours (UNKNOWN where absent) into st.  All 256 threads:
// the unit's weight plane, then its tsdf plane, as four 16-byte loads each; then the six face weights, then the six face tsdf values.
// The halo's edges and corners are never read and stay unwritten.
__device__ __forceinline__ void hv_site_halo_load(const char *__restrict__ pool, const int32_t *unit_idx, double thr, uint8_t *st) {
    const int t = (int)threadIdx.x;
    const char *unit = pool + (size_t)unit_idx[0] * HV_TSDF_UNIT_BYTES;
    uint4 w[4];
    float4 f[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) w[q] = ((const uint4 *)(unit + HV_TSDF_PLANE_BYTES))[q * 256 + t];
#pragma unroll
    for (int q = 0; q < 4; ++q) f[q] = ((const float4 *)unit)[q * 256 + t];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int word = (q * 256 + t) * 4; // z * 256 + x * 16 + y: four consecutive y
        const int at = hv_site_halo_at((word >> 4) & 15, word & 15, word >> 8);
        st[at] = (uint8_t)hv_site_state(w[q].x, f[q].x, thr);
        st[at + HV_SITE_H] = (uint8_t)hv_site_state(w[q].y, f[q].y, thr);
        st[at + 2 * HV_SITE_H] = (uint8_t)hv_site_state(w[q].z, f[q].z, thr);
        st[at + 3 * HV_SITE_H] = (uint8_t)hv_site_state(w[q].w, f[q].w, thr);
    }
    // the six faces: 256 voxels each, one per thread (a = t >> 4, b = t & 15)
    const int a = t >> 4, b = t & 15;
    const int word[6] = {hv_tsdf_word(15, b, a), hv_tsdf_word(0, b, a), hv_tsdf_word(b, 15, a),
                         hv_tsdf_word(b, 0, a),  hv_tsdf_word(a, b, 15), hv_tsdf_word(a, b, 0)};
    uint32_t fw[6];
    float ff[6];
#pragma unroll
    for (int s = 0; s < 6; ++s) {
        const int32_t nb = unit_idx[1 + s];
        fw[s] = nb >= 0 ? ((const uint32_t *)(pool + (size_t)nb * HV_TSDF_UNIT_BYTES + HV_TSDF_PLANE_BYTES))[word[s]] : 0u;
    }
#pragma unroll
    for (int s = 0; s < 6; ++s) {
        const int32_t nb = unit_idx[1 + s];
        ff[s] = nb >= 0 ? ((const float *)(pool + (size_t)nb * HV_TSDF_UNIT_BYTES))[word[s]] : 0.0f;
    }
    st[hv_site_halo_at(-1, b, a)] = (uint8_t)hv_site_state(fw[0], ff[0], thr);
    st[hv_site_halo_at(16, b, a)] = (uint8_t)hv_site_state(fw[1], ff[1], thr);
    st[hv_site_halo_at(b, -1, a)] = (uint8_t)hv_site_state(fw[2], ff[2], thr);
    st[hv_site_halo_at(b, 16, a)] = (uint8_t)hv_site_state(fw[3], ff[3], thr);
    st[hv_site_halo_at(a, b, -1)] = (uint8_t)hv_site_state(fw[4], ff[4], thr);
    st[hv_site_halo_at(a, b, 16)] = (uint8_t)hv_site_state(fw[5], ff[5], thr);
}

// Is the voxel at halo cell `at` (of the unit itself) a site: FREE or INSIDE with a face neighbour of the other state?
__device__ __forceinline__ bool hv_site_is_site(const uint8_t *st, int at) {
    const uint32_t s = st[at], other = s ^ 3u; // FREE <-> INSIDE; UNKNOWN gives 3, which no voxel holds
    return st[at - HV_SITE_H * HV_SITE_H] == other || st[at + HV_SITE_H * HV_SITE_H] == other || st[at - HV_SITE_H] == other ||
           st[at + HV_SITE_H] == other || st[at - 1] == other || st[at + 1] == other;
}
#endif // __HIPCC__
