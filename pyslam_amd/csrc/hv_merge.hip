// hv_tsdf_integrate_volume: fuse one TSDF volume into another through a rigid transform (include/hipvol.h states the contract).
//
// Every destination voxel centre is carried into the source's frame and the source field is sampled there (trilinear where all
// eight voxels around the point are observed, else the nearest voxel); the sample enters the destination as w_s observations.
//   candidates  one wave per source unit: hv_tsdf_unit_has_weight; a unit that holds a weight names the destination
//               units its transformed box can reach (at most 3 per axis) into a scratch key set                k_merge_candidates
//   probe       one workgroup per candidate: does ANY of its voxels have an observed nearest source voxel?  Leaves at the first
//               plane group that has one; such a unit goes onto the keep list                                  k_merge_probe
//   (the host reads the count: nothing kept = the destination is left exactly as it was)
//   claim       the kept keys enter the destination's table (hv_table_insert); the pool grows as for integrate  k_merge_claim
//   sweep       one workgroup per kept unit, lane -> (x, 4 y's), a wave per z plane: sample, update, stamp     k_merge_sweep
// Probe and sweep resolve the 3 x 3 x 3 source units a destination unit can reach into LDS once (27 hash probes); a voxel fetch is
// then integer arithmetic and loads; the cell rule, the corner order and the trilinear form are hv_tsdf_cell.h's.  Probe and sweep
// evaluate the same predicate with the same instructions (hv_merge_locate / hv_merge_nearest), so every kept unit gets at least
// one voxel and no other unit is claimed.
#include <algorithm>
#include <cmath>

#include "hv_common.h"
#include "hv_tsdf_cell.h"

namespace {

enum { HV_MERGE_N_SOURCE = 0, HV_MERGE_N_CAND = 1, HV_MERGE_N_KEEP = 2, HV_MERGE_TRILINEAR = 3, HV_MERGE_NEAREST = 4, HV_MERGE_SET_FULL = 5,
       HV_MERGE_WORDS = 8 };
constexpr size_t HV_MERGE_HDR = 256;

struct HvMergeXf {
    double rt[9];  // R^T, row-major: p = R^T (c - t)
    double t[3];
    double fwd[9]; // R, row-major (candidates: source box -> destination frame)
    double voxel_length;
};

// Destination voxel (global index gv) -> its cell in the source lattice (hv_cell_locate).  false: the point lies outside every
// representable source voxel - no source voxel there is observed.
__device__ __forceinline__ bool hv_merge_locate(const HvMergeXf &X, int32_t gx, int32_t gy, int32_t gz, int32_t *g0, double *r) {
    const double d0 = ((double)gx + 0.5) * X.voxel_length - X.t[0];
    const double d1 = ((double)gy + 0.5) * X.voxel_length - X.t[1];
    const double d2 = ((double)gz + 0.5) * X.voxel_length - X.t[2];
    double p[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) p[a] = (X.rt[a * 3 + 0] * d0 + X.rt[a * 3 + 1] * d1) + X.rt[a * 3 + 2] * d2;
    return hv_cell_locate(p, X.voxel_length, g0, r);
}

// The source units around a destination unit: pool indices of units base + {0,1,2}^3 (-1 = absent) in LDS.
struct HvMergeSrc {
    const int32_t *tab; // LDS [27]
    int32_t bx, by, bz;
    const HvTable *table;
    const char *pool;
};

__device__ __forceinline__ int32_t hv_merge_unit(const HvMergeSrc &S, int32_t ux, int32_t uy, int32_t uz) {
    const uint32_t rx = (uint32_t)ux - (uint32_t)S.bx, ry = (uint32_t)uy - (uint32_t)S.by, rz = (uint32_t)uz - (uint32_t)S.bz;
    if (rx < 3u && ry < 3u && rz < 3u) return S.tab[(rz * 3 + ry) * 3 + rx];
    // beyond the table (the corner estimate of the base was off by a rounding): the hash itself
    unsigned long long ck = HV_EMPTY_KEY;
    int32_t ci = -1;
    return hv_tsdf_unit(*S.table, ux, uy, uz, ck, ci);
}

// pool index and word of source voxel (vx, vy, vz); idx < 0: no such unit
__device__ __forceinline__ void hv_merge_voxel(const HvMergeSrc &S, int32_t vx, int32_t vy, int32_t vz, int32_t &idx, int &word) {
    idx = hv_merge_unit(S, vx >> 4, vy >> 4, vz >> 4);
    word = hv_tsdf_word(vx & (HV_TSDF_R - 1), vy & (HV_TSDF_R - 1), vz & (HV_TSDF_R - 1));
}

__device__ __forceinline__ uint32_t hv_merge_weight(const HvMergeSrc &S, int32_t idx, int word) {
    return idx < 0 ? 0u : ((const uint32_t *)(S.pool + (int64_t)idx * HV_TSDF_UNIT_BYTES + HV_TSDF_PLANE_BYTES))[word];
}

// weight of the nearest source voxel (0: unobserved); its pool index and word
__device__ __forceinline__ uint32_t hv_merge_nearest(const HvMergeSrc &S, const int32_t *g0, const double *r, int32_t &idx, int &word) {
    hv_merge_voxel(S, g0[0] + (r[0] >= 0.5), g0[1] + (r[1] >= 0.5), g0[2] + (r[2] >= 0.5), idx, word);
    return hv_merge_weight(S, idx, word);
}

// Fill the LDS table for destination unit (kx, ky, kz).  All threads of the workgroup; ends with a barrier.
__device__ __forceinline__ void hv_merge_resolve(const HvMergeXf &X, const HvTable &src, int32_t kx, int32_t ky, int32_t kz, int32_t *s_tab,
                                                 int32_t *s_base) {
    const int t = (int)threadIdx.x;
    if (t < 3) s_base[t] = INT32_MAX;
    __syncthreads();
    if (t < 8) { // the eight corner voxels: g is affine in the voxel index, its minimum is at a corner
        int32_t g0[3];
        double r[3];
        const bool ok = hv_merge_locate(X, kx * HV_TSDF_R + ((t & 1) ? HV_TSDF_R - 1 : 0), ky * HV_TSDF_R + ((t & 2) ? HV_TSDF_R - 1 : 0), kz * HV_TSDF_R + ((t & 4) ? HV_TSDF_R - 1 : 0), g0, r);
        if (ok)
            for (int a = 0; a < 3; ++a) atomicMin(&s_base[a], g0[a] >> 4);
    }
    __syncthreads();
    if (t < 27) {
        const int32_t bx = s_base[0], by = s_base[1], bz = s_base[2];
        int32_t idx = -1;
        if (bx != INT32_MAX) {
            unsigned long long ck = HV_EMPTY_KEY;
            int32_t ci = -1;
            idx = hv_tsdf_unit(src, bx + t % 3, by + (t / 3) % 3, bz + t / 9, ck, ci);
        }
        s_tab[t] = idx;
    }
    __syncthreads();
}

// One wave per source unit.  Emptiness: hv_tsdf_unit_has_weight.
// A unit with a weight: the eight corners of its box [k L, (k + 1) L) go to the destination frame; every destination unit with a
// voxel centre inside their bounding box (padded by 1e-3 voxel against the rounding of the per-voxel arithmetic) is a candidate.
// A destination voxel whose nearest source voxel lies in this unit has its centre's pre-image inside the box, so no unit is missed.
__global__ __launch_bounds__(256) void k_merge_candidates(const unsigned long long *__restrict__ src_keys, const char *__restrict__ src_pool,
                                                          int32_t used, HvMergeXf X, unsigned long long *__restrict__ set, uint32_t set_mask,
                                                          unsigned long long *__restrict__ cand, int32_t cand_cap, int32_t *__restrict__ cnt) {
    const int32_t unit = (int32_t)blockIdx.x * 4 + (int32_t)(threadIdx.x >> 6); // wave-uniform
    if (unit >= used) return;
    const int lane = hv_lane_id();
    if (!hv_tsdf_unit_has_weight(src_pool, unit, lane)) return;
    if (lane == 0) atomicAdd(&cnt[HV_MERGE_N_SOURCE], 1);
    int32_t kx, ky, kz;
    hv_unpack_key(src_keys[unit], kx, ky, kz);
    const double L = X.voxel_length * (double)HV_TSDF_R;
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const double p0 = (double)(kx + (c & 1)) * L, p1 = (double)(ky + ((c >> 1) & 1)) * L, p2 = (double)(kz + (c >> 2)) * L;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double q = ((X.fwd[a * 3 + 0] * p0 + X.fwd[a * 3 + 1] * p1) + X.fwd[a * 3 + 2] * p2) + X.t[a];
            lo[a] = fmin(lo[a], q);
            hi[a] = fmax(hi[a], q);
        }
    }
    int32_t ulo[3], n[3];
    bool ok = true;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double glo = lo[a] / X.voxel_length - 0.5 - 1.0e-3, ghi = hi[a] / X.voxel_length - 0.5 + 1.0e-3;
        ok = ok && fabs(glo) < HV_CELL_LIMIT && fabs(ghi) < HV_CELL_LIMIT;
        const double a0 = floor(ceil(glo) / (double)HV_TSDF_R), a1 = floor(floor(ghi) / (double)HV_TSDF_R); // units of the first / last voxel centre inside
        ulo[a] = ok ? (int32_t)a0 : 0;
        n[a] = ok ? (int32_t)(a1 - a0) + 1 : 0; // <= 3: the box spans 16 sqrt(3) + 0.002 < 32 voxels
    }
    if (!ok || lane >= 27) return;
    const int i = lane % 3, j = (lane / 3) % 3, k = lane / 9;
    if (i >= n[0] || j >= n[1] || k >= n[2]) return;
    const int32_t ux = ulo[0] + i, uy = ulo[1] + j, uz = ulo[2] + k;
    if (!hv_key_in_range(ux, uy, uz)) return;
    const unsigned long long key = hv_pack_key(ux, uy, uz);
    bool is_new;
    if (hv_keyset_insert(set, set_mask, key, &is_new) < 0) {
        atomicAdd(&cnt[HV_MERGE_SET_FULL], 1);
    } else if (is_new) {
        const int32_t at = atomicAdd(&cnt[HV_MERGE_N_CAND], 1);
        if (at < cand_cap) cand[at] = key;
    }
}

// One workgroup per candidate: a wave per z plane, lane -> (x, 4 y's); the workgroup leaves after the first group of four planes
// in which some voxel's nearest source voxel is observed, and thread 0 puts the key onto the keep list.
__global__ __launch_bounds__(256) void k_merge_probe(const unsigned long long *__restrict__ cand, HvTable src, const char *__restrict__ src_pool,
                                                     HvMergeXf X, unsigned long long *__restrict__ keep, int32_t *__restrict__ cnt) {
    __shared__ int32_t s_tab[27];
    __shared__ int32_t s_base[3];
    const unsigned long long key = cand[blockIdx.x];
    int32_t kx, ky, kz;
    hv_unpack_key(key, kx, ky, kz);
    hv_merge_resolve(X, src, kx, ky, kz, s_tab, s_base);
    const HvMergeSrc S{s_tab, s_base[0], s_base[1], s_base[2], &src, src_pool};
    const int lane = hv_lane_id(), wave = (int)(threadIdx.x >> 6);
    const int x = lane >> 2, y0 = (lane & 3) * 4;
    for (int zb = 0; zb < HV_TSDF_R; zb += 4) {
        const int z = zb + wave;
        int hit = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            int32_t g0[3], idx;
            double r[3];
            int word;
            if (hv_merge_locate(X, kx * HV_TSDF_R + x, ky * HV_TSDF_R + y0 + q, kz * HV_TSDF_R + z, g0, r)) hit |= hv_merge_nearest(S, g0, r, idx, word) != 0u;
        }
        if (__syncthreads_or(hit)) {
            if (threadIdx.x == 0) keep[atomicAdd(&cnt[HV_MERGE_N_KEEP], 1)] = key;
            return;
        }
    }
}

__global__ __launch_bounds__(256) void k_merge_claim(HvTable dst, const unsigned long long *__restrict__ keep, int32_t n) {
    const int32_t i = (int32_t)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < n) hv_table_insert(dst, keep[i]);
}

// One workgroup per kept destination unit.  A wave owns the planes z = wave, wave + 4, ...; a lane owns (x, y0 .. y0 + 3), so the
// destination's five planes are read and written in 1 KiB bursts of 16-byte accesses - and only where one of the lane's four voxels
// is updated (most voxels of a unit lie off the observed band).  Source fetches are gathers: neighbours along the source's y are
// adjacent words, the rest is served by L2.
__global__ __launch_bounds__(256) void k_merge_sweep(const unsigned long long *__restrict__ keep, HvTable dst, char *__restrict__ dst_pool,
                                                     int32_t *__restrict__ dst_stamp, int32_t stamp, HvTable src,
                                                     const char *__restrict__ src_pool, HvMergeXf X, unsigned long long *__restrict__ cnt64) {
    __shared__ int32_t s_tab[27];
    __shared__ int32_t s_base[3];
    __shared__ int32_t s_unit;
    const unsigned long long key = keep[blockIdx.x];
    int32_t kx, ky, kz;
    hv_unpack_key(key, kx, ky, kz);
    if (threadIdx.x == 0) {
        const int32_t slot = hv_table_find(dst, key);
        const int32_t idx = slot >= 0 ? dst.vals[slot] : -1;
        if (idx >= 0) dst_stamp[slot] = stamp;
        s_unit = idx;
    }
    hv_merge_resolve(X, src, kx, ky, kz, s_tab, s_base); // (its barriers publish s_unit)
    if (s_unit < 0) return;                              // (claimed without a block: the host has refused the call already)
    char *unit = dst_pool + (int64_t)s_unit * HV_TSDF_UNIT_BYTES;
    const HvMergeSrc S{s_tab, s_base[0], s_base[1], s_base[2], &src, src_pool};
    const int lane = hv_lane_id(), wave = (int)(threadIdx.x >> 6);
    const int x = lane >> 2, y0 = (lane & 3) * 4;
    int n_tri = 0, n_near = 0;
    for (int z = wave; z < HV_TSDF_R; z += 4) {
        uint32_t ws[4];     // the sample's weight (0: the voxel is not touched)
        double ts[4];       // tsdf_s
        uint32_t gain[4][3];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            ws[q] = 0u;
            ts[q] = 0.0;
            gain[q][0] = gain[q][1] = gain[q][2] = 0u;
            int32_t g0[3], nidx;
            double r[3];
            int nword;
            if (!hv_merge_locate(X, kx * HV_TSDF_R + x, ky * HV_TSDF_R + y0 + q, kz * HV_TSDF_R + z, g0, r)) continue;
            const uint32_t wn = hv_merge_nearest(S, g0, r, nidx, nword);
            if (wn == 0u) continue;
            int32_t cidx[8];
            int cword[8];
            uint32_t cw[8];
            bool all = true;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                int sx, sy, sz;
                hv_cell_corner(i, sx, sy, sz);
                hv_merge_voxel(S, g0[0] + sx, g0[1] + sy, g0[2] + sz, cidx[i], cword[i]);
                cw[i] = hv_merge_weight(S, cidx[i], cword[i]);
                all = all && cw[i] != 0u;
            }
            double mean[3];
            if (all) {
                double f[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) f[i] = (double)((const float *)(src_pool + (int64_t)cidx[i] * HV_TSDF_UNIT_BYTES))[cword[i]];
                ts[q] = hv_cell_lerp(r, f);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
#pragma unroll
                    for (int i = 0; i < 8; ++i)
                        f[i] = (double)((const uint32_t *)(src_pool + (int64_t)cidx[i] * HV_TSDF_UNIT_BYTES + (2 + c) * HV_TSDF_PLANE_BYTES))[cword[i]] / (double)cw[i];
                    mean[c] = hv_cell_lerp(r, f);
                }
                n_tri += 1;
            } else {
                const char *u = src_pool + (int64_t)nidx * HV_TSDF_UNIT_BYTES;
                ts[q] = (double)((const float *)u)[nword];
#pragma unroll
                for (int c = 0; c < 3; ++c) mean[c] = (double)((const uint32_t *)(u + (2 + c) * HV_TSDF_PLANE_BYTES))[nword] / (double)wn;
                n_near += 1;
            }
            ws[q] = wn;
#pragma unroll
            for (int c = 0; c < 3; ++c) gain[q][c] = (uint32_t)floor(mean[c] * (double)wn + 0.5);
        }
        if ((ws[0] | ws[1] | ws[2] | ws[3]) == 0u) continue;
        const int v4 = hv_tsdf_word(x, y0, z) >> 2;
        float4 vt = ((const float4 *)unit)[v4];
        uint4 vw = ((const uint4 *)(unit + HV_TSDF_PLANE_BYTES))[v4];
        uint4 vr = ((const uint4 *)(unit + 2 * HV_TSDF_PLANE_BYTES))[v4];
        uint4 vg = ((const uint4 *)(unit + 3 * HV_TSDF_PLANE_BYTES))[v4];
        uint4 vb = ((const uint4 *)(unit + 4 * HV_TSDF_PLANE_BYTES))[v4];
#define HV_MERGE_APPLY(q, m)                                                                                                         \
    if (ws[q] != 0u) {                                                                                                               \
        const uint32_t w1 = vw.m + ws[q];                                                                                            \
        vt.m = (float)(((double)vt.m * (double)vw.m + ts[q] * (double)ws[q]) / (double)w1);                                          \
        vw.m = w1;                                                                                                                   \
        vr.m += gain[q][0];                                                                                                          \
        vg.m += gain[q][1];                                                                                                          \
        vb.m += gain[q][2];                                                                                                          \
    }
        HV_MERGE_APPLY(0, x)
        HV_MERGE_APPLY(1, y)
        HV_MERGE_APPLY(2, z)
        HV_MERGE_APPLY(3, w)
#undef HV_MERGE_APPLY
        ((float4 *)unit)[v4] = vt;
        ((uint4 *)(unit + HV_TSDF_PLANE_BYTES))[v4] = vw;
        ((uint4 *)(unit + 2 * HV_TSDF_PLANE_BYTES))[v4] = vr;
        ((uint4 *)(unit + 3 * HV_TSDF_PLANE_BYTES))[v4] = vg;
        ((uint4 *)(unit + 4 * HV_TSDF_PLANE_BYTES))[v4] = vb;
    }
    n_tri = hv_wave_sum(n_tri);
    n_near = hv_wave_sum(n_near);
    if (lane == 0) {
        if (n_tri) atomicAdd(&cnt64[0], (unsigned long long)n_tri);
        if (n_near) atomicAdd(&cnt64[1], (unsigned long long)n_near);
    }
}

} // namespace

extern "C" int hv_tsdf_integrate_volume(hv_volume *dst, hv_volume *src, const double *T, hv_merge_stats *stats) {
    HV_REQUIRE(dst != nullptr && src != nullptr && T != nullptr, HV_ERR_INVALID, "hv_tsdf_integrate_volume: null argument");
    const char *fn = "hv_tsdf_integrate_volume";
    int rc = hv_tsdf_require_whole_map(dst, fn, "the destination");
    if (rc != HV_OK) return rc;
    rc = hv_tsdf_require_whole_map(src, fn, "the source");
    if (rc != HV_OK) return rc;
    HV_REQUIRE(dst != src, HV_ERR_INVALID, "hv_tsdf_integrate_volume: source and destination are the same volume");
    HV_REQUIRE(dst->cfg.voxel_size == src->cfg.voxel_size && dst->cfg.sdf_trunc == src->cfg.sdf_trunc && dst->cfg.block_size == src->cfg.block_size,
               HV_ERR_INVALID, "hv_tsdf_integrate_volume: the volumes differ in voxel_length (%g / %g), sdf_trunc (%g / %g) or unit resolution (%d / %d)",
               dst->cfg.voxel_size, src->cfg.voxel_size, dst->cfg.sdf_trunc, src->cfg.sdf_trunc, (int)dst->cfg.block_size, (int)src->cfg.block_size);
    HV_REQUIRE(dst->device == src->device, HV_ERR_INVALID, "hv_tsdf_integrate_volume: the volumes live on different devices (%d / %d)", dst->device,
               src->device);
    for (int i = 0; i < 16; ++i) HV_REQUIRE(std::isfinite(T[i]), HV_ERR_INVALID, "hv_tsdf_integrate_volume: the transformation is not finite");
    HV_REQUIRE(T[12] == 0.0 && T[13] == 0.0 && T[14] == 0.0 && T[15] == 1.0, HV_ERR_INVALID,
               "hv_tsdf_integrate_volume: the transformation's bottom row is not (0, 0, 0, 1)");
    HvMergeXf X{};
    double ortho = 0.0;
    for (int a = 0; a < 3; ++a) {
        double row = 0.0;
        for (int b = 0; b < 3; ++b) {
            double s = 0.0;
            for (int k = 0; k < 3; ++k) s += T[k * 4 + a] * T[k * 4 + b];
            row += std::fabs(s - (a == b ? 1.0 : 0.0));
            X.rt[a * 3 + b] = T[b * 4 + a];
            X.fwd[a * 3 + b] = T[a * 4 + b];
        }
        ortho = std::max(ortho, row);
        X.t[a] = T[a * 4 + 3];
    }
    const double det = T[0] * (T[5] * T[10] - T[6] * T[9]) - T[1] * (T[4] * T[10] - T[6] * T[8]) + T[2] * (T[4] * T[9] - T[5] * T[8]);
    HV_REQUIRE(ortho <= 1.0e-6 && det >= 0.0, HV_ERR_INVALID,
               "hv_tsdf_integrate_volume: the transformation is not rigid (|R^T R - I|_inf = %.3g, det = %.3g)", ortho, det);
    X.voxel_length = dst->cfg.voxel_size;

    // drain both batch pipelines; the source's pending work is done before the destination's stream reads it
    int64_t src_used = 0, dst_before = 0;
    rc = hv_tsdf_drain(src, fn, false, &src_used);
    if (rc == HV_OK) rc = hv_tsdf_drain(dst, fn, false, &dst_before);
    if (rc != HV_OK) return rc;
    HV_REQUIRE(src->h_counters[HV_CNT_OVERFLOW] == 0 && !src->overflow_latched, HV_ERR_CAPACITY,
               "%s: the source's block pool overflowed earlier (hv_reserve_blocks or hv_reset it first)", fn);
    if (stats != nullptr) *stats = hv_merge_stats{0, 0, 0, 0, 0};
    if (src_used == 0) return HV_OK;

    // scratch: [counters 256 B][candidate keys cap u64][kept keys cap u64][key set set_cap u64]; cap = 27 per source unit (every
    // one of them distinct would be the worst case), the set at most half full
    const int64_t cap = 27 * src_used;
    HV_REQUIRE(cap < (1ll << 30), HV_ERR_CAPACITY, "hv_tsdf_integrate_volume: %lld source units are too many", (long long)src_used);
    uint64_t set_cap = 1024;
    while (set_cap < 2 * (uint64_t)cap) set_cap <<= 1;
    HvScratch S; // (every return below has waited for the stream, or follows a device error)
    char *scratch = nullptr;
    HV_HIP(S.get(&scratch, HV_MERGE_HDR + 8 * (size_t)(2 * cap + (int64_t)set_cap)));
    int32_t *d_cnt = (int32_t *)scratch;
    unsigned long long *d_cnt64 = (unsigned long long *)(scratch + 128);
    unsigned long long *d_cand = (unsigned long long *)(scratch + HV_MERGE_HDR);
    unsigned long long *d_keep = d_cand + cap;
    unsigned long long *d_set = d_keep + cap;
    int32_t h_cnt[HV_MERGE_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
    auto fail = [&](const char *what, hipError_t e) {
        hv_set_error("hv_tsdf_integrate_volume: %s failed: %s", what, hipGetErrorString(e));
        return HV_ERR_DEVICE;
    };
    auto read_counts = [&]() {
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(h_cnt, d_cnt, sizeof(h_cnt), hipMemcpyDeviceToHost, dst->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(dst->stream);
        return e;
    };
    hipStream_t s = dst->stream;
    hipError_t e = hipMemsetAsync(scratch, 0, HV_MERGE_HDR, s);
    if (e == hipSuccess) e = hipMemsetAsync(d_set, 0xFF, 8 * (size_t)set_cap, s);
    if (e != hipSuccess) return fail("clearing the scratch", e);
    hipLaunchKernelGGL(k_merge_candidates, dim3((unsigned)((src_used + 3) / 4)), dim3(256), 0, s, (const unsigned long long *)src->table.block_keys,
                       (const char *)src->pool, (int32_t)src_used, X, d_set, (uint32_t)(set_cap - 1), d_cand, (int32_t)cap, d_cnt);
    if ((e = read_counts()) != hipSuccess) return fail("the candidate pass", e);
    const int64_t n_cand = h_cnt[HV_MERGE_N_CAND];
    HV_REQUIRE(h_cnt[HV_MERGE_SET_FULL] == 0 && n_cand <= cap, HV_ERR_CAPACITY,
               "hv_tsdf_integrate_volume: the candidate set overflowed (%lld candidates, room for %lld)", (long long)n_cand, (long long)cap);
    if (stats != nullptr) stats->units_source = h_cnt[HV_MERGE_N_SOURCE];
    int64_t n_keep = 0;
    if (n_cand > 0) {
        hipLaunchKernelGGL(k_merge_probe, dim3((unsigned)n_cand), dim3(256), 0, s, (const unsigned long long *)d_cand, src->table,
                           (const char *)src->pool, X, d_keep, d_cnt);
        if ((e = read_counts()) != hipSuccess) return fail("the probe pass", e);
        n_keep = h_cnt[HV_MERGE_N_KEEP];
    }
    if (n_keep == 0) return HV_OK; // no destination voxel has an observed source voxel nearest: the destination is left exactly as it was
    // claim the kept units.  The gate refuses a latched overflow and grows a pool that is more than half full; whether it asks
    // for a checked claim does not matter here: the claim is ALWAYS verified (hv_claims_fit - this call waits for the GPU anyway),
    // so a pool that is too small grows before a voxel is written
    bool checked_unused = false;
    rc = hv_capacity_gate(dst, &checked_unused);
    for (int attempt = 0; rc == HV_OK; ++attempt) {
        hipLaunchKernelGGL(k_merge_claim, dim3((unsigned)((n_keep + 255) / 256)), dim3(256), 0, dst->stream, dst->table,
                           (const unsigned long long *)d_keep, (int32_t)n_keep);
        rc = hv_claims_fit(dst);
        if (rc == HV_OK) break;
        if (rc == HV_RETRY_CLAIM && attempt < 8) rc = HV_OK;
        else if (rc == HV_RETRY_CLAIM) rc = HV_ERR_CAPACITY;
    }
    if (rc != HV_OK) return rc;
    const int64_t dst_after = std::min<int64_t>(dst->h_counters[HV_CNT_BLOCKS], dst->cfg.max_blocks);
    // voxels change from here on: cached extraction results are void, the written units carry a new stamp (the per-unit extraction
    // caches and hv_tsdf_dirty_keys see them)
    dst->content_version += 1;
    dst->frame_counter += 1;
    hv_profile_begin(dst);
    hipLaunchKernelGGL(k_merge_sweep, dim3((unsigned)n_keep), dim3(256), 0, dst->stream, (const unsigned long long *)d_keep, dst->table,
                       (char *)dst->pool, dst->touched_stamp, dst->frame_counter, src->table, (const char *)src->pool, X, d_cnt64);
    hv_profile_end(dst, n_keep);
    hv_launch_publish_status(dst);
    unsigned long long h_cnt64[2] = {0, 0};
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(h_cnt64, d_cnt64, sizeof(h_cnt64), hipMemcpyDeviceToHost, dst->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(dst->stream);
    if (e != hipSuccess) // (a device fault: the claimed units are in dst, written or not - the contract's error paragraph says so)
        return fail("the sweep (the destination holds the claimed units, possibly unwritten; hv_tsdf_prune releases the empty ones)", e);
    if (stats != nullptr) {
        stats->units_claimed = dst_after - dst_before;
        stats->voxels_trilinear = (int64_t)h_cnt64[0];
        stats->voxels_nearest = (int64_t)h_cnt64[1];
        stats->voxels_updated = stats->voxels_trilinear + stats->voxels_nearest;
    }
    return HV_OK;
}
