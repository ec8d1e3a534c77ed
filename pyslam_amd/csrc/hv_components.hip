// libpyslam_hipvol.so — connected components of the surface sites of the TSDF map on gfx950 (hv_tsdf_surface_components,
// hv_tsdf_remove_components).  The contract (site, adjacency, canonical numbering, the removal rule) is written once in
// include/hipvol.h; tests/components_reference.py restates it in numpy.
//
// Nothing here holds a word per pool voxel.  Per unit: a 4096-bit site mask in dump bit order (bit x * 256 + y * 16 + z, i.e. 256
// rows of 16 z bits), the exclusive popcount prefix of its rows, its count and its base.  The units are ranked by key on the host
// (hv_tsdf_key_order, the order of hv_tsdf_dump and hv_tsdf_pack), the bases are the prefix sum of the counts in that order, and
//   index(site) = base[unit] + rowpre[row] + popcount(row bits below z)
// numbers the sites in the order of the site list: the parent array and the list come from the same masks.
//   k_cc_sites    one workgroup per unit: the classification halo of hv_tsdf_sites.h (18^3 states in LDS, six hash probes), the
//                 row masks, their prefix, the count
//   k_cc_scan     one workgroup: bases in key order, the number of sites
//   k_cc_local    one workgroup per unit: union-find over the unit's 4096 voxels in LDS (atomicMin towards the smaller index, 13
//                 forward neighbours per site), flattened into parent[]
//   k_cc_cross    one workgroup per unit: every border site against the sites of the 26 neighbour units' masks, union-find on
//                 parent[] with global atomicMin; an edge is linked from its larger end only
//   k_cc_flatten  one lane per site: parent[i] = root; roots take a component slot (one atomic per wave)
//   k_cc_stats    one workgroup per unit, a lane per row: sizes and boxes (phase 0), then the seed's y (phase 1) and z (phase 2) -
//                 integer atomics, one per wave where the wave's rows belong to one component, else one per row run
//   rocprim       three stable radix sorts of the component slots by seed z, y, x: the canonical order
//   k_cc_table / k_cc_list   the table in that order; site_index / site_label
//   k_cc_small / k_cc_reset  removal: the mask of the sites of small components per unit; then per unit the two box dilations
//                 (SMALL, KEPT) of the 3 x 3 x 3 units' masks - shifts and ORs of the 48-bit z rows, then ORs of 16-bit rows along y,
//                 then along x - and the reset of whole quads of the five planes
// Every link loop strictly lowers the larger of its two indices, so it ends; no wave waits for another; there is no loop over
// propagation rounds on the host at all.
#include <algorithm>
#include <cmath>
#include <vector>

#include <rocprim/device/device_radix_sort.hpp>

#include "hv_common.h"
#include "hv_tsdf_sites.h"

namespace {

constexpr int CC_ROWS = HV_TSDF_RR;   // 16-bit z rows of a unit, row = x * 16 + y
constexpr int CC_W = 3 * HV_TSDF_R;   // side of the 3 x 3 x 3 unit neighbourhood in voxels
enum { CC_R_SITES = 0, CC_R_COMPONENTS = 1, CC_R_LARGEST = 2, CC_R_COMP_REMOVED = 3, CC_R_SITES_REMOVED = 4, CC_R_VOXELS_RESET = 5,
       CC_R_UNITS_CHANGED = 6, CC_R_UNITS_EMPTIED = 7, CC_R_WORDS = 8 };
enum { CC_LO = 0, CC_HI = 3, CC_SY = 6, CC_SZ = 7, CC_BOX_ROWS = 8 }; // rows of the per-component int32 table [8][C]

__device__ __forceinline__ uint32_t cc_below(uint32_t row, int z) { return (uint32_t)__popc(row & ((1u << z) - 1u)); }

// exclusive prefix of v over the 256 threads of the workgroup; *total = the sum.  s_w: 4 ints of LDS, used once per kernel.
__device__ __forceinline__ int cc_block_scan(int v, int *s_w, int *total) {
    const int lane = hv_lane_id(), wave = (int)threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int o = 1; o < HV_WAVE; o <<= 1) {
        const int up = __shfl_up(incl, o);
        if (lane >= o) incl += up;
    }
    if (lane == HV_WAVE - 1) s_w[wave] = incl;
    __syncthreads();
    int off = 0, sum = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        off += w < wave ? s_w[w] : 0;
        sum += s_w[w];
    }
    *total = sum;
    return off + incl - v;
}

__global__ __launch_bounds__(256) void k_cc_sites(HvTable table, const char *__restrict__ pool, int32_t used, double thr,
                                                  uint16_t *__restrict__ mask, uint16_t *__restrict__ rowpre, uint32_t *__restrict__ count) {
    __shared__ uint8_t st[HV_SITE_HALO_CELLS];
    __shared__ int32_t unit_idx[7]; // the unit, then its -x +x -y +y -z +z neighbours
    __shared__ int s_w[4];
    const int t = (int)threadIdx.x;
    const int32_t self = (int32_t)blockIdx.x;
    int32_t ux, uy, uz;
    hv_unpack_key(table.block_keys[self], ux, uy, uz);
    hv_site_halo_units(table, ux, uy, uz, used, self, unit_idx);
    __syncthreads();
    hv_site_halo_load(pool, unit_idx, thr, st);
    __syncthreads();
    const int x = t >> 4, y = t & 15;
    uint32_t row = 0u;
#pragma unroll 4
    for (int z = 0; z < HV_TSDF_R; ++z) row |= hv_site_is_site(st, hv_site_halo_at(x, y, z)) ? 1u << z : 0u;
    int total;
    const int pre = cc_block_scan(__popc(row), s_w, &total);
    mask[(size_t)self * CC_ROWS + t] = (uint16_t)row;
    rowpre[(size_t)self * CC_ROWS + t] = (uint16_t)pre; // < 4096: the last row's prefix is at most 4080
    if (t == 0) count[self] = (uint32_t)total;
}

// One workgroup: base[order[r]] = sites of the units ranked below r; result[CC_R_SITES] = all of them.
__global__ __launch_bounds__(1024) void k_cc_scan(const uint32_t *__restrict__ count, const int32_t *__restrict__ order, int32_t used,
                                                  uint32_t *__restrict__ base, unsigned long long *__restrict__ result) {
    __shared__ unsigned long long s_scan[1024];
    const int t = (int)threadIdx.x;
    const int64_t per = ((int64_t)used + 1023) / 1024;
    const int64_t b0 = t * per, b1 = b0 + per;
    const int32_t i0 = (int32_t)(b0 < used ? b0 : used), i1 = (int32_t)(b1 < used ? b1 : used);
    unsigned long long mine = 0;
    for (int32_t r = i0; r < i1; ++r) mine += count[order[r]];
    s_scan[t] = mine;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const unsigned long long below = t >= d ? s_scan[t - d] : 0ull;
        __syncthreads();
        s_scan[t] += below;
        __syncthreads();
    }
    unsigned long long run = s_scan[t] - mine;
    for (int32_t r = i0; r < i1; ++r) {
        const int32_t u = order[r];
        base[u] = (uint32_t)run; // (meaningful only while the total stays below 2^31: the host refuses more)
        run += count[u];
    }
    if (t == 1023) result[CC_R_SITES] = s_scan[1023];
}

// ---- union-find: parent[i] <= i always, links go to the smaller index, a root has parent[i] == i --------------------------------
__device__ __forceinline__ uint32_t cc_find_lds(uint32_t *l, uint32_t a) {
    for (;;) {
        const uint32_t p = __hip_atomic_load(&l[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (p == a) return a;
        a = p;
    }
}
// Every turn either ends or replaces the larger index by a smaller one: at most a + b turns.
__device__ __forceinline__ void cc_union_lds(uint32_t *l, uint32_t a, uint32_t b) {
    for (;;) {
        a = cc_find_lds(l, a);
        b = cc_find_lds(l, b);
        if (a == b) return;
        if (a < b) {
            const uint32_t s = a;
            a = b;
            b = s;
        }
        const uint32_t old = atomicMin(&l[a], b);
        if (old == a) return; // a was a root: linked
        a = old;              // a had been linked meanwhile (to old < a): old and b still have to meet
    }
}
__device__ __forceinline__ uint32_t cc_find(uint32_t *parent, uint32_t a) {
    for (;;) {
        const uint32_t p = __hip_atomic_load(&parent[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); // past this CU's L1
        if (p == a) return a;
        a = p;
    }
}
__device__ __forceinline__ void cc_union(uint32_t *parent, uint32_t a, uint32_t b) {
    for (;;) {
        a = cc_find(parent, a);
        b = cc_find(parent, b);
        if (a == b) return;
        if (a < b) {
            const uint32_t s = a;
            a = b;
            b = s;
        }
        const uint32_t old = atomicMin(&parent[a], b);
        if (old == a) return;
        a = old;
    }
}

__global__ __launch_bounds__(256) void k_cc_local(const uint16_t *__restrict__ mask, const uint16_t *__restrict__ rowpre,
                                                  const uint32_t *__restrict__ count, const uint32_t *__restrict__ base,
                                                  uint32_t *__restrict__ parent) {
    __shared__ uint32_t lbl[HV_TSDF_RRR];
    __shared__ uint16_t rows[CC_ROWS], pre[CC_ROWS];
    const int t = (int)threadIdx.x;
    const size_t u = blockIdx.x;
    if (count[u] == 0u) return; // (the whole workgroup)
    const uint32_t mine = mask[u * CC_ROWS + t];
    rows[t] = (uint16_t)mine;
    pre[t] = rowpre[u * CC_ROWS + t];
#pragma unroll
    for (int z = 0; z < HV_TSDF_R; ++z) lbl[t * HV_TSDF_R + z] = (uint32_t)(t * HV_TSDF_R + z);
    __syncthreads();
    const int x = t >> 4, y = t & 15;
    for (uint32_t m = mine; m != 0u; m &= m - 1u) {
        const int z = __ffs((int)m) - 1;
        const uint32_t d = (uint32_t)(t * HV_TSDF_R + z);
        const uint32_t zwin = ((7u << z) >> 1) & 0xffffu; // z - 1, z, z + 1 inside the row
        if ((mine >> (z + 1)) & 1u) cc_union_lds(lbl, d, d + 1u);
        for (int dx = 0; dx <= 1; ++dx)
            for (int dy = -1; dy <= 1; ++dy) {
                if (dx == 0 && dy <= 0) continue; // the 13 neighbours after d in (x, y, z) order: each pair once
                const int X = x + dx, Y = y + dy;
                if (X > 15 || Y < 0 || Y > 15) continue;
                const int r2 = X * HV_TSDF_R + Y;
                for (uint32_t c = rows[r2] & zwin; c != 0u; c &= c - 1u) cc_union_lds(lbl, d, (uint32_t)(r2 * HV_TSDF_R + __ffs((int)c) - 1));
            }
    }
    __syncthreads();
    const uint32_t b = base[u];
    for (uint32_t m = mine; m != 0u; m &= m - 1u) {
        const int z = __ffs((int)m) - 1;
        const uint32_t root = cc_find_lds(lbl, (uint32_t)(t * HV_TSDF_R + z));
        const uint32_t rr = root >> 4;
        parent[b + pre[t] + cc_below(mine, z)] = b + pre[rr] + cc_below(rows[rr], (int)(root & 15u));
    }
}

__global__ __launch_bounds__(256) void k_cc_cross(HvTable table, int32_t used, const uint16_t *__restrict__ mask,
                                                  const uint16_t *__restrict__ rowpre, const uint32_t *__restrict__ base,
                                                  uint32_t *__restrict__ parent) {
    __shared__ int32_t nb[27];
    const int t = (int)threadIdx.x;
    const int32_t self = (int32_t)blockIdx.x;
    if (t < 27) {
        int32_t ux, uy, uz;
        hv_unpack_key(table.block_keys[self], ux, uy, uz);
        nb[t] = t == 13 ? self : hv_tsdf_unit_index(table, ux + t / 9 - 1, uy + (t / 3) % 3 - 1, uz + t % 3 - 1, used);
    }
    __syncthreads();
    const uint32_t mine = mask[(size_t)self * CC_ROWS + t];
    if (mine == 0u) return;
    const int x = t >> 4, y = t & 15;
    const uint32_t at = base[self] + rowpre[(size_t)self * CC_ROWS + t];
    const bool xy_edge = x == 0 || x == 15 || y == 0 || y == 15;
    // A site that is not a root keeps the parent k_cc_local gave it (links only ever rewrite roots), and a root's parent is an
    // ancestor whenever it is read: parent[i] and parent[j] stand for i and j.  Neighbouring border sites mostly repeat the same
    // pair of them, so the lane remembers the last four partners it linked its current representative to and skips those.
    uint32_t rep = 0xffffffffu, seen0 = 0xffffffffu, seen1 = 0xffffffffu, seen2 = 0xffffffffu, seen3 = 0xffffffffu;
    for (uint32_t m = xy_edge ? mine : mine & 0x8001u; m != 0u; m &= m - 1u) {
        const int z = __ffs((int)m) - 1;
        const uint32_t i = at + cc_below(mine, z);
        const uint32_t li = parent[i];
        if (li != rep) {
            rep = li;
            seen0 = seen1 = seen2 = seen3 = 0xffffffffu;
        }
        for (int dx = -1; dx <= 1; ++dx)
            for (int dy = -1; dy <= 1; ++dy) {
                const int X = x + dx, Y = y + dy;
                const int ox = X < 0 ? 0 : (X > 15 ? 2 : 1), oy = Y < 0 ? 0 : (Y > 15 ? 2 : 1);
                const int r2 = ((X & 15) << 4) | (Y & 15);
                for (int dz = -1; dz <= 1; ++dz) {
                    const int Z = z + dz;
                    const int oz = Z < 0 ? 0 : (Z > 15 ? 2 : 1);
                    const int n = ox * 9 + oy * 3 + oz;
                    if (n == 13) continue; // inside this unit: k_cc_local's
                    const int32_t nu = nb[n];
                    if (nu < 0) continue;
                    const uint32_t row2 = mask[(size_t)nu * CC_ROWS + r2];
                    if (!((row2 >> (Z & 15)) & 1u)) continue;
                    const uint32_t j = base[nu] + rowpre[(size_t)nu * CC_ROWS + r2] + cc_below(row2, Z & 15);
                    if (j >= i) continue; // (the other end sees its j < i and links the edge)
                    const uint32_t lj = parent[j];
                    if (lj == seen0 || lj == seen1 || lj == seen2 || lj == seen3) continue;
                    cc_union(parent, li, lj);
                    seen3 = seen2, seen2 = seen1, seen1 = seen0, seen0 = lj;
                }
            }
    }
}

// parent[i] = the root of i; a root takes component slot aux[i].  Roots do not change here, and a parent read while another lane
// shortens it is an ancestor either way.
__global__ __launch_bounds__(256) void k_cc_flatten(uint32_t *__restrict__ parent, uint32_t n, uint32_t *__restrict__ aux, int32_t *__restrict__ slots) {
    const uint64_t i64 = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const bool live = i64 < n;
    const uint32_t i = (uint32_t)i64;
    uint32_t r = 0u;
    if (live) {
        r = cc_find(parent, i);
        parent[i] = r;
    }
    const bool root = live && r == i;
    const int32_t slot = hv_wave_append(slots, root);
    if (root) aux[i] = (uint32_t)slot;
}

__global__ __launch_bounds__(256) void k_cc_comp_init(uint32_t *__restrict__ cnt, int32_t *__restrict__ box, uint32_t c) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j >= c) return;
    cnt[j] = 0u;
#pragma unroll
    for (int r = 0; r < CC_BOX_ROWS; ++r) box[(size_t)r * c + j] = r >= CC_HI && r < CC_HI + 3 ? INT32_MIN : INT32_MAX;
}

// One component's contribution from a lane (n sites, all of row (gx, gy), z in [z0, z1]) into the table.  PHASE 0: size and box;
// 1: the seed's y (rows at the smallest x); 2: the seed's z (rows at the smallest x and, there, the smallest y); 3: size only.
template <int PHASE>
__device__ __forceinline__ void cc_flush(uint32_t *cnt, int32_t *box, uint32_t c, uint32_t cid, uint32_t n, int32_t v0, int32_t v1, int32_t v2,
                                         int32_t w0, int32_t w1, int32_t w2) {
    if (PHASE == 0 || PHASE == 3) atomicAdd(&cnt[cid], n);
    if (PHASE == 0) {
        atomicMin(&box[(size_t)(CC_LO + 0) * c + cid], v0);
        atomicMin(&box[(size_t)(CC_LO + 1) * c + cid], v1);
        atomicMin(&box[(size_t)(CC_LO + 2) * c + cid], v2);
        atomicMax(&box[(size_t)(CC_HI + 0) * c + cid], w0);
        atomicMax(&box[(size_t)(CC_HI + 1) * c + cid], w1);
        atomicMax(&box[(size_t)(CC_HI + 2) * c + cid], w2);
    }
    if (PHASE == 1 && v0 != INT32_MAX) atomicMin(&box[(size_t)CC_SY * c + cid], v0);
    if (PHASE == 2 && v0 != INT32_MAX) atomicMin(&box[(size_t)CC_SZ * c + cid], v0);
}

template <int PHASE>
__global__ __launch_bounds__(256) void k_cc_stats(const unsigned long long *__restrict__ block_keys, const uint16_t *__restrict__ mask,
                                                  const uint16_t *__restrict__ rowpre, const uint32_t *__restrict__ count,
                                                  const uint32_t *__restrict__ base, const uint32_t *__restrict__ parent,
                                                  const uint32_t *__restrict__ aux, uint32_t *__restrict__ cnt, int32_t *__restrict__ box, uint32_t c) {
    const int t = (int)threadIdx.x;
    const size_t u = blockIdx.x;
    if (count[u] == 0u) return;
    int32_t kx, ky, kz;
    hv_unpack_key(block_keys[u], kx, ky, kz);
    const uint32_t mine = mask[u * CC_ROWS + t];
    const int32_t gx = kx * HV_TSDF_R + (t >> 4), gy = ky * HV_TSDF_R + (t & 15), gz0 = kz * HV_TSDF_R;
    const uint32_t at = base[u] + rowpre[u * CC_ROWS + t];
    // runs of one component along the row; all but the last are flushed at once, the last may be shared with the wave
    uint32_t cid = 0u, n = 0u;
    int z0 = 0, z1 = 0, k = 0;
    auto value = [&](int32_t &v0, int32_t &v1, int32_t &v2, int32_t &w0, int32_t &w1, int32_t &w2) {
        v0 = gx, v1 = gy, v2 = gz0 + z0, w0 = gx, w1 = gy, w2 = gz0 + z1;
        if (PHASE == 1) v0 = gx == box[(size_t)CC_LO * c + cid] ? gy : INT32_MAX;
        if (PHASE == 2) v0 = gx == box[(size_t)CC_LO * c + cid] && gy == box[(size_t)CC_SY * c + cid] ? gz0 + z0 : INT32_MAX;
    };
    for (uint32_t m = mine; m != 0u; m &= m - 1u, ++k) {
        const int z = __ffs((int)m) - 1;
        const uint32_t id = aux[parent[at + (uint32_t)k]];
        if (n != 0u && id != cid) {
            int32_t v0, v1, v2, w0, w1, w2;
            value(v0, v1, v2, w0, w1, w2);
            cc_flush<PHASE>(cnt, box, c, cid, n, v0, v1, v2, w0, w1, w2);
            n = 0u;
        }
        if (n == 0u) cid = id, z0 = z;
        z1 = z;
        n += 1u;
    }
    const bool has = n != 0u;
    const unsigned long long any = __ballot(has);
    if (any == 0ull) return;
    int32_t v0 = INT32_MAX, v1 = INT32_MAX, v2 = INT32_MAX, w0 = INT32_MIN, w1 = INT32_MIN, w2 = INT32_MIN;
    if (has) value(v0, v1, v2, w0, w1, w2);
    const int first = __ffsll((long long)any) - 1;
    const uint32_t c0 = __shfl(cid, first);
    if (__ballot(has && cid == c0) == any) { // one component in the whole wave: one atomic per field
        const uint32_t ns = hv_wave_sum(n);
        v0 = hv_wave_min(v0);
        if (PHASE == 0) {
            v1 = hv_wave_min(v1), v2 = hv_wave_min(v2);
            w0 = hv_wave_max(w0), w1 = hv_wave_max(w1), w2 = hv_wave_max(w2);
        }
        if (hv_lane_id() == first) cc_flush<PHASE>(cnt, box, c, c0, ns, v0, v1, v2, w0, w1, w2);
    } else if (has) {
        cc_flush<PHASE>(cnt, box, c, cid, n, v0, v1, v2, w0, w1, w2);
    }
}

// sort key of one radix pass: the coordinate of the slots in their current order, biased to unsigned
__global__ __launch_bounds__(256) void k_cc_sort_key(const int32_t *__restrict__ coord, const uint32_t *__restrict__ perm, uint32_t c,
                                                     uint32_t *__restrict__ key, uint32_t *__restrict__ iota) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (j >= c) return;
    const uint32_t slot = perm != nullptr ? perm[j] : (uint32_t)j;
    key[j] = (uint32_t)coord[slot] ^ 0x80000000u;
    if (iota != nullptr) iota[j] = (uint32_t)j;
}

// Row j of the table = slot perm[j] (perm == nullptr: slot j, no table wanted); rank[slot] = j; the largest size; for the removal
// (min_sites > 0) the components and sites that go.
__global__ __launch_bounds__(256) void k_cc_table(const uint32_t *__restrict__ perm, const uint32_t *__restrict__ cnt, const int32_t *__restrict__ box,
                                                  uint32_t c, uint32_t *__restrict__ rank, int32_t *__restrict__ seed, int64_t *__restrict__ sites,
                                                  int32_t *__restrict__ lo, int32_t *__restrict__ hi, int64_t min_sites,
                                                  unsigned long long *__restrict__ result) {
    const uint64_t j = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const bool live = j < c;
    uint32_t n = 0u;
    if (live) {
        const uint32_t slot = perm != nullptr ? perm[j] : (uint32_t)j;
        n = cnt[slot];
        if (rank != nullptr) rank[slot] = (uint32_t)j;
        if (seed != nullptr) {
            seed[j * 3 + 0] = box[(size_t)CC_LO * c + slot];
            seed[j * 3 + 1] = box[(size_t)CC_SY * c + slot];
            seed[j * 3 + 2] = box[(size_t)CC_SZ * c + slot];
        }
        if (sites != nullptr) sites[j] = (int64_t)n;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            if (lo != nullptr) lo[j * 3 + a] = box[(size_t)(CC_LO + a) * c + slot];
            if (hi != nullptr) hi[j * 3 + a] = box[(size_t)(CC_HI + a) * c + slot];
        }
    }
    const uint32_t largest = hv_wave_max(n);
    const bool small = live && (int64_t)n < min_sites;
    const unsigned long long gone = (unsigned long long)__popcll(__ballot(small));
    const unsigned long long gone_sites = hv_wave_sum<unsigned long long>(small ? n : 0u);
    if (hv_lane_id() == 0) {
        if (largest != 0u) atomicMax(&result[CC_R_LARGEST], (unsigned long long)largest);
        if (gone != 0ull) {
            atomicAdd(&result[CC_R_COMP_REMOVED], gone);
            atomicAdd(&result[CC_R_SITES_REMOVED], gone_sites);
        }
    }
}

__global__ __launch_bounds__(256) void k_cc_list(const unsigned long long *__restrict__ block_keys, const uint16_t *__restrict__ mask,
                                                 const uint16_t *__restrict__ rowpre, const uint32_t *__restrict__ count,
                                                 const uint32_t *__restrict__ base, const uint32_t *__restrict__ parent,
                                                 const uint32_t *__restrict__ aux, const uint32_t *__restrict__ rank,
                                                 int32_t *__restrict__ site_index, int32_t *__restrict__ site_label) {
    const int t = (int)threadIdx.x;
    const size_t u = blockIdx.x;
    if (count[u] == 0u) return;
    int32_t kx, ky, kz;
    hv_unpack_key(block_keys[u], kx, ky, kz);
    const uint32_t mine = mask[u * CC_ROWS + t];
    const size_t at = (size_t)base[u] + rowpre[u * CC_ROWS + t];
    int k = 0;
    for (uint32_t m = mine; m != 0u; m &= m - 1u, ++k) {
        const size_t i = at + (size_t)k;
        if (site_index != nullptr) {
            site_index[i * 3 + 0] = kx * HV_TSDF_R + (t >> 4);
            site_index[i * 3 + 1] = ky * HV_TSDF_R + (t & 15);
            site_index[i * 3 + 2] = kz * HV_TSDF_R + __ffs((int)m) - 1;
        }
        if (site_label != nullptr) site_label[i] = (int32_t)rank[aux[parent[i]]];
    }
}

// small[u][row] = the sites of the row whose component has fewer than min_sites sites; small_count[u] = how many in the unit
__global__ __launch_bounds__(256) void k_cc_small(const uint16_t *__restrict__ mask, const uint16_t *__restrict__ rowpre,
                                                  const uint32_t *__restrict__ base, const uint32_t *__restrict__ parent,
                                                  const uint32_t *__restrict__ aux, const uint32_t *__restrict__ cnt, int64_t min_sites,
                                                  uint16_t *__restrict__ small, uint32_t *__restrict__ small_count) {
    __shared__ int s_w[4];
    const int t = (int)threadIdx.x;
    const size_t u = blockIdx.x;
    const uint32_t mine = mask[u * CC_ROWS + t];
    const uint32_t at = base[u] + rowpre[u * CC_ROWS + t];
    uint32_t row = 0u;
    int k = 0;
    for (uint32_t m = mine; m != 0u; m &= m - 1u, ++k)
        if ((int64_t)cnt[aux[parent[at + (uint32_t)k]]] < min_sites) row |= m & (0u - m);
    small[u * CC_ROWS + t] = (uint16_t)row;
    int total;
    (void)cc_block_scan(__popc(row), s_w, &total);
    if (t == 0) small_count[u] = (uint32_t)total;
}

// One workgroup per unit.  S = the box dilation by `margin` of the SMALL sites, K = that of the KEPT ones (mask & ~small), over the
// 3 x 3 x 3 units around this one; a voxel with a weight is reset when it is a SMALL site, or in S and not in K.  The dilation is
// separable and the order of the axes does not matter: z first, inside the 48-bit rows of three units, leaves 16-bit rows.
__global__ __launch_bounds__(256) void k_cc_reset(HvTable table, char *__restrict__ pool, int32_t used, const uint16_t *__restrict__ mask,
                                                  const uint16_t *__restrict__ small, const uint32_t *__restrict__ small_count, int32_t margin,
                                                  int32_t *__restrict__ stamp, int32_t new_stamp, unsigned long long *__restrict__ result) {
    __shared__ int32_t nb[27];
    __shared__ uint16_t a_s[CC_W * CC_W], a_k[CC_W * CC_W]; // [X][Y], z dilated, this unit's 16 z
    __shared__ uint16_t b_s[CC_W * HV_TSDF_R], b_k[CC_W * HV_TSDF_R]; // [X][y], y dilated
    __shared__ uint16_t cand[CC_ROWS];
    __shared__ uint32_t s_cnt[2];
    const int t = (int)threadIdx.x;
    const int32_t self = (int32_t)blockIdx.x;
    const unsigned long long key = table.block_keys[self];
    if (t < 27) {
        int32_t ux, uy, uz;
        hv_unpack_key(key, ux, uy, uz);
        int32_t idx = t == 13 ? self : hv_tsdf_unit_index(table, ux + t / 9 - 1, uy + (t / 3) % 3 - 1, uz + t % 3 - 1, used);
        if (idx >= 0 && t != 13 && margin == 0) idx = -1; // margin 0: the neighbours do not reach in
        nb[t] = idx;
    }
    if (t < 2) s_cnt[t] = 0u;
    __syncthreads();
    bool near = false; // does a unit of the neighbourhood hold a SMALL site at all?
    if (t < 27 && nb[t] >= 0) near = small_count[nb[t]] != 0u;
    if (!__syncthreads_or(near ? 1 : 0)) return;
    const int lo = HV_TSDF_R - margin, hi = 2 * HV_TSDF_R - 1 + margin; // rows that can reach this unit
    for (int e = t; e < CC_W * CC_W; e += 256) {
        const int X = e / CC_W, Y = e - X * CC_W;
        uint32_t rs = 0u, rk = 0u;
        if (X >= lo && X <= hi && Y >= lo && Y <= hi) {
            unsigned long long s48 = 0ull, k48 = 0ull;
            const int r = ((X & 15) << 4) | (Y & 15);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int32_t nu = nb[(X >> 4) * 9 + (Y >> 4) * 3 + k];
                if (nu < 0) continue;
                const uint32_t sm = small[(size_t)nu * CC_ROWS + r], all = mask[(size_t)nu * CC_ROWS + r];
                s48 |= (unsigned long long)sm << (16 * k);
                k48 |= (unsigned long long)(all & ~sm) << (16 * k);
            }
            unsigned long long ds = s48, dk = k48;
            for (int s = 1; s <= margin; ++s) {
                ds |= (s48 << s) | (s48 >> s);
                dk |= (k48 << s) | (k48 >> s);
            }
            rs = (uint32_t)(ds >> 16) & 0xffffu;
            rk = (uint32_t)(dk >> 16) & 0xffffu;
        }
        a_s[e] = (uint16_t)rs;
        a_k[e] = (uint16_t)rk;
    }
    __syncthreads();
    for (int e = t; e < CC_W * HV_TSDF_R; e += 256) {
        const int X = e >> 4, y = e & 15;
        uint32_t rs = 0u, rk = 0u;
        for (int Y = HV_TSDF_R + y - margin; Y <= HV_TSDF_R + y + margin; ++Y) {
            rs |= a_s[X * CC_W + Y];
            rk |= a_k[X * CC_W + Y];
        }
        b_s[e] = (uint16_t)rs;
        b_k[e] = (uint16_t)rk;
    }
    __syncthreads();
    {
        const int x = t >> 4, y = t & 15;
        uint32_t rs = 0u, rk = 0u;
        for (int X = HV_TSDF_R + x - margin; X <= HV_TSDF_R + x + margin; ++X) {
            rs |= b_s[X * HV_TSDF_R + y];
            rk |= b_k[X * HV_TSDF_R + y];
        }
        const uint32_t c = (uint32_t)small[(size_t)self * CC_ROWS + t] | (rs & ~rk);
        cand[t] = (uint16_t)c;
        if (!__syncthreads_or(c != 0u ? 1 : 0)) return;
    }
    // quads of four consecutive y (16 bytes of a plane): thread t owns quads t, t + 256, t + 512, t + 768 - the whole weight plane
    char *unit = pool + (size_t)self * HV_TSDF_UNIT_BYTES;
    uint32_t n_reset = 0u, n_left = 0u;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int quad = q * 256 + t, word = quad * 4;
        const int z = word >> 8, row = word & 255; // word = z * 256 + x * 16 + y: row = x * 16 + y of the quad's first voxel
        const uint4 w = ((const uint4 *)(unit + HV_TSDF_PLANE_BYTES))[quad];
        const bool r0 = ((cand[row] >> z) & 1u) && w.x != 0u, r1 = ((cand[row + 1] >> z) & 1u) && w.y != 0u;
        const bool r2 = ((cand[row + 2] >> z) & 1u) && w.z != 0u, r3 = ((cand[row + 3] >> z) & 1u) && w.w != 0u;
        n_reset += (uint32_t)r0 + (uint32_t)r1 + (uint32_t)r2 + (uint32_t)r3;
        n_left += (uint32_t)(w.x != 0u && !r0) + (uint32_t)(w.y != 0u && !r1) + (uint32_t)(w.z != 0u && !r2) + (uint32_t)(w.w != 0u && !r3);
        if (r0 || r1 || r2 || r3) {
#pragma unroll
            for (int p = 0; p < HV_TSDF_PLANES; ++p) { // the fresh state in all five planes, each quad one 16-byte store
                uint4 *at = (uint4 *)(unit + (size_t)p * HV_TSDF_PLANE_BYTES) + quad;
                uint4 v = p == 1 ? w : *at;
                v.x = r0 ? 0u : v.x;
                v.y = r1 ? 0u : v.y;
                v.z = r2 ? 0u : v.z;
                v.w = r3 ? 0u : v.w;
                *at = v;
            }
        }
    }
    n_reset = hv_wave_sum(n_reset);
    n_left = hv_wave_sum(n_left);
    if (hv_lane_id() == 0) {
        if (n_reset) atomicAdd(&s_cnt[0], n_reset);
        if (n_left) atomicAdd(&s_cnt[1], n_left);
    }
    __syncthreads();
    if (t == 0 && s_cnt[0] != 0u) {
        atomicAdd(&result[CC_R_VOXELS_RESET], (unsigned long long)s_cnt[0]);
        atomicAdd(&result[CC_R_UNITS_CHANGED], 1ull);
        if (s_cnt[1] == 0u) atomicAdd(&result[CC_R_UNITS_EMPTIED], 1ull);
        const int32_t slot = hv_table_find(table, key);
        if (slot >= 0) stamp[slot] = new_stamp;
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
struct CcLabels {
    int64_t units = 0, sites = 0, components = 0;
    uint16_t *mask = nullptr, *rowpre = nullptr;
    uint32_t *count = nullptr, *base = nullptr, *parent = nullptr, *aux = nullptr, *cnt = nullptr;
    int32_t *order = nullptr, *box = nullptr;
    unsigned long long *result = nullptr; // [CC_R_WORDS], device
};

int cc_check(hv_volume *v, double weight_threshold, const char *fn) {
    HV_REQUIRE(v != nullptr, HV_ERR_INVALID, "%s: null volume", fn);
    const int rc = hv_tsdf_require_whole_map(v, fn, "the volume");
    if (rc != HV_OK) return rc;
    HV_REQUIRE(std::isfinite(weight_threshold) && weight_threshold >= 0.0, HV_ERR_INVALID, "%s: weight_threshold must be finite and >= 0", fn);
    return HV_OK;
}

template <int PHASE>
void cc_launch_stats(hv_volume *v, const CcLabels &L) {
    hv_profile_begin(v);
    hipLaunchKernelGGL(k_cc_stats<PHASE>, dim3((unsigned)L.units), dim3(256), 0, v->stream, (const unsigned long long *)v->table.block_keys,
                       (const uint16_t *)L.mask, (const uint16_t *)L.rowpre, (const uint32_t *)L.count, (const uint32_t *)L.base,
                       (const uint32_t *)L.parent, (const uint32_t *)L.aux, L.cnt, L.box, (uint32_t)L.components);
    hv_profile_end(v, L.units);
}

// Sites, union-find, component slots, sizes (and boxes and seeds when `seeds`).  Drains the pipeline and waits for the GPU.
int cc_label(hv_volume *v, double thr, bool seeds, HvScratch &S, CcLabels &L, const char *fn) {
    int64_t used = 0;
    int rc = hv_tsdf_drain(v, fn, false, &used);
    if (rc != HV_OK) return rc;
    L.units = used;
    HV_HIP(S.get(&L.result, CC_R_WORDS));
    HV_HIP(hipMemsetAsync(L.result, 0, CC_R_WORDS * sizeof(unsigned long long), v->stream));
    if (used == 0) return HV_OK;
    // rank the units by key: 8 bytes per unit to the host, 4 back
    std::vector<int32_t> order;
    rc = hv_tsdf_key_order(v, used, order, nullptr);
    if (rc != HV_OK) return rc;
    HV_HIP(S.get(&L.mask, (size_t)used * CC_ROWS));
    HV_HIP(S.get(&L.rowpre, (size_t)used * CC_ROWS));
    HV_HIP(S.get(&L.count, (size_t)used));
    HV_HIP(S.get(&L.base, (size_t)used));
    HV_HIP(S.get(&L.order, (size_t)used));
    rc = hv_h2d(v, L.order, order.data(), 4 * (size_t)used);
    if (rc != HV_OK) return rc;
    hv_profile_begin(v);
    hipLaunchKernelGGL(k_cc_sites, dim3((unsigned)used), dim3(256), 0, v->stream, v->table, (const char *)v->pool, (int32_t)used, thr, L.mask,
                       L.rowpre, L.count);
    hv_profile_end(v, used);
    hv_profile_begin(v);
    hipLaunchKernelGGL(k_cc_scan, dim3(1), dim3(1024), 0, v->stream, (const uint32_t *)L.count, (const int32_t *)L.order, (int32_t)used, L.base,
                       L.result);
    hv_profile_end(v, 0);
    HV_HIP(hipGetLastError());
    unsigned long long h[CC_R_WORDS];
    HV_HIP(hipMemcpyAsync(h, L.result, sizeof(h), hipMemcpyDeviceToHost, v->stream));
    HV_HIP(hipStreamSynchronize(v->stream));
    HV_REQUIRE(h[CC_R_SITES] <= (unsigned long long)INT32_MAX, HV_ERR_INVALID, "%s: %llu sites exceed 2^31 - 1", fn, h[CC_R_SITES]);
    L.sites = (int64_t)h[CC_R_SITES];
    if (L.sites == 0) return HV_OK;
    HV_HIP(S.get(&L.parent, (size_t)L.sites));
    HV_HIP(S.get(&L.aux, (size_t)L.sites));
    int32_t *d_slots = nullptr; // hv_wave_append's counter
    HV_HIP(S.get(&d_slots, 1));
    HV_HIP(hipMemsetAsync(d_slots, 0, sizeof(int32_t), v->stream));
    hv_profile_begin(v);
    hipLaunchKernelGGL(k_cc_local, dim3((unsigned)used), dim3(256), 0, v->stream, (const uint16_t *)L.mask, (const uint16_t *)L.rowpre,
                       (const uint32_t *)L.count, (const uint32_t *)L.base, L.parent);
    hv_profile_end(v, used);
    hv_profile_begin(v);
    hipLaunchKernelGGL(k_cc_cross, dim3((unsigned)used), dim3(256), 0, v->stream, v->table, (int32_t)used, (const uint16_t *)L.mask,
                       (const uint16_t *)L.rowpre, (const uint32_t *)L.base, L.parent);
    hv_profile_end(v, used);
    hv_profile_begin(v);
    hipLaunchKernelGGL(k_cc_flatten, dim3((unsigned)((L.sites + 255) / 256)), dim3(256), 0, v->stream, L.parent, (uint32_t)L.sites, L.aux, d_slots);
    hv_profile_end(v, 0);
    HV_HIP(hipGetLastError());
    int32_t slots = 0;
    HV_HIP(hipMemcpyAsync(&slots, d_slots, sizeof(slots), hipMemcpyDeviceToHost, v->stream));
    HV_HIP(hipStreamSynchronize(v->stream));
    L.components = slots;
    const size_t c = (size_t)L.components;
    HV_HIP(S.get(&L.cnt, c));
    HV_HIP(S.get(&L.box, c * CC_BOX_ROWS));
    hv_profile_begin(v);
    hipLaunchKernelGGL(k_cc_comp_init, dim3((unsigned)((c + 255) / 256)), dim3(256), 0, v->stream, L.cnt, L.box, (uint32_t)c);
    hv_profile_end(v, 0);
    if (seeds) {
        cc_launch_stats<0>(v, L);
        cc_launch_stats<1>(v, L);
        cc_launch_stats<2>(v, L);
    } else {
        cc_launch_stats<3>(v, L);
    }
    HV_HIP(hipGetLastError());
    return HV_OK;
}

} // namespace

extern "C" int hv_tsdf_surface_components(hv_volume *v, double weight_threshold, int32_t *seed, int64_t *sites, int32_t *lo, int32_t *hi,
                                          int64_t component_cap, int32_t *site_index, int32_t *site_label, int64_t site_cap,
                                          int64_t *n_components, int64_t *n_sites, hv_components_stats *stats, int32_t loc) {
    const char *fn = "hv_tsdf_surface_components";
    int rc = cc_check(v, weight_threshold, fn);
    if (rc != HV_OK) return rc;
    HV_REQUIRE(loc == HV_HOST || loc == HV_DEVICE, HV_ERR_INVALID, "%s: bad loc %d", fn, (int)loc);
    const bool want_table = seed != nullptr || sites != nullptr || lo != nullptr || hi != nullptr;
    const bool want_list = site_index != nullptr || site_label != nullptr;
    HV_REQUIRE((!want_table || component_cap >= 0) && (!want_list || site_cap >= 0), HV_ERR_INVALID, "%s: negative capacity", fn);
    HvScratch S;
    CcLabels L;
    rc = cc_label(v, weight_threshold, want_table || site_label != nullptr, S, L, fn);
    if (rc != HV_OK) return rc;
    if (n_components != nullptr) *n_components = L.components;
    if (n_sites != nullptr) *n_sites = L.sites;
    HV_REQUIRE(!want_table || component_cap >= L.components, HV_ERR_INVALID, "%s: %lld components, room for %lld", fn, (long long)L.components,
               (long long)component_cap);
    HV_REQUIRE(!want_list || site_cap >= L.sites, HV_ERR_INVALID, "%s: %lld sites, room for %lld", fn, (long long)L.sites, (long long)site_cap);
    // (the sizes are known only now, after the labelling: an empty map has no outputs)
    const size_t c = (size_t)L.components, n = (size_t)L.sites;
    HvStage st(v, loc);
    const int o_seed = st.out(seed, 12 * c), o_sites = st.out(sites, 8 * c), o_lo = st.out(lo, 12 * c), o_hi = st.out(hi, 12 * c);
    const int o_index = st.out(site_index, 12 * n), o_label = st.out(site_label, 4 * n);
    rc = st.commit(&v->stage, &v->stage_bytes);
    if (rc != HV_OK) return rc;
    if (c > 0) {
        uint32_t *perm = nullptr, *rank = nullptr;
        if (want_table || site_label != nullptr) {
            // the canonical order: three stable radix sorts of the slots, by seed z, then y, then x
            uint32_t *key_a = nullptr, *key_b = nullptr, *perm_a = nullptr, *perm_b = nullptr;
            HV_HIP(S.get(&key_a, c));
            HV_HIP(S.get(&key_b, c));
            HV_HIP(S.get(&perm_a, c));
            HV_HIP(S.get(&perm_b, c));
            HV_HIP(S.get(&rank, c));
            size_t tmp_bytes = 0;
            HV_HIP(rocprim::radix_sort_pairs(nullptr, tmp_bytes, key_a, key_b, perm_a, perm_b, c, 0, 32, v->stream));
            char *tmp = nullptr;
            HV_HIP(S.get(&tmp, tmp_bytes));
            const int32_t *coord[3] = {L.box + (size_t)CC_SZ * c, L.box + (size_t)CC_SY * c, L.box + (size_t)CC_LO * c};
            hv_profile_begin(v); // (one bracket around the three sorts)
            for (int pass = 0; pass < 3; ++pass) {
                hipLaunchKernelGGL(k_cc_sort_key, dim3((unsigned)((c + 255) / 256)), dim3(256), 0, v->stream, coord[pass],
                                   pass == 0 ? (const uint32_t *)nullptr : (const uint32_t *)perm_a, (uint32_t)c, key_a, pass == 0 ? perm_a : nullptr);
                HV_HIP(rocprim::radix_sort_pairs(tmp, tmp_bytes, key_a, key_b, perm_a, perm_b, c, 0, 32, v->stream));
                std::swap(perm_a, perm_b);
            }
            hv_profile_end(v, 0);
            perm = perm_a;
        }
        hv_profile_begin(v);
        hipLaunchKernelGGL(k_cc_table, dim3((unsigned)((c + 255) / 256)), dim3(256), 0, v->stream, (const uint32_t *)perm, (const uint32_t *)L.cnt,
                           (const int32_t *)L.box, (uint32_t)c, rank, st.dev<int32_t>(o_seed), st.dev<int64_t>(o_sites), st.dev<int32_t>(o_lo),
                           st.dev<int32_t>(o_hi), (int64_t)0, L.result);
        hv_profile_end(v, 0);
        if (want_list) {
            hv_profile_begin(v);
            hipLaunchKernelGGL(k_cc_list, dim3((unsigned)L.units), dim3(256), 0, v->stream, (const unsigned long long *)v->table.block_keys,
                               (const uint16_t *)L.mask, (const uint16_t *)L.rowpre, (const uint32_t *)L.count, (const uint32_t *)L.base,
                               (const uint32_t *)L.parent, (const uint32_t *)L.aux, (const uint32_t *)rank, st.dev<int32_t>(o_index),
                               st.dev<int32_t>(o_label));
            hv_profile_end(v, L.units);
        }
        HV_HIP(hipGetLastError());
    }
    unsigned long long h[CC_R_WORDS];
    rc = st.finish(h, sizeof(h), L.result); // (always waits: the scratch is freed on return, everything queued has run)
    if (rc != HV_OK) return rc;
    if (stats != nullptr) {
        stats->units = L.units;
        stats->sites = L.sites;
        stats->components = L.components;
        stats->largest = (int64_t)h[CC_R_LARGEST];
    }
    return HV_OK;
}

extern "C" int hv_tsdf_remove_components(hv_volume *v, double weight_threshold, int64_t min_sites, int32_t margin, hv_remove_components_stats *stats) {
    const char *fn = "hv_tsdf_remove_components";
    int rc = cc_check(v, weight_threshold, fn);
    if (rc != HV_OK) return rc;
    HV_REQUIRE(min_sites >= 1, HV_ERR_INVALID, "%s: min_sites must be >= 1, got %lld", fn, (long long)min_sites);
    HV_REQUIRE(margin >= 0 && margin <= HV_COMPONENTS_MAX_MARGIN, HV_ERR_INVALID, "%s: margin %d is outside 0..%d", fn, (int)margin,
               HV_COMPONENTS_MAX_MARGIN);
    HvScratch S;
    CcLabels L;
    rc = cc_label(v, weight_threshold, false, S, L, fn);
    if (rc != HV_OK) return rc;
    unsigned long long h[CC_R_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (L.components > 0) {
        const size_t c = (size_t)L.components;
        uint16_t *small = nullptr;
        uint32_t *small_count = nullptr;
        HV_HIP(S.get(&small, (size_t)L.units * CC_ROWS));
        HV_HIP(S.get(&small_count, (size_t)L.units));
        hv_profile_begin(v);
        hipLaunchKernelGGL(k_cc_table, dim3((unsigned)((c + 255) / 256)), dim3(256), 0, v->stream, (const uint32_t *)nullptr, (const uint32_t *)L.cnt,
                           (const int32_t *)L.box, (uint32_t)c, (uint32_t *)nullptr, (int32_t *)nullptr, (int64_t *)nullptr, (int32_t *)nullptr,
                           (int32_t *)nullptr, min_sites, L.result);
        hv_profile_end(v, 0);
        hv_profile_begin(v);
        hipLaunchKernelGGL(k_cc_small, dim3((unsigned)L.units), dim3(256), 0, v->stream, (const uint16_t *)L.mask, (const uint16_t *)L.rowpre,
                           (const uint32_t *)L.base, (const uint32_t *)L.parent, (const uint32_t *)L.aux, (const uint32_t *)L.cnt, min_sites, small,
                           small_count);
        hv_profile_end(v, L.units);
        // a changed unit is stamped with the NEXT frame id; the host commits that id only if a voxel was reset
        hv_profile_begin(v);
        hipLaunchKernelGGL(k_cc_reset, dim3((unsigned)L.units), dim3(256), 0, v->stream, v->table, (char *)v->pool, (int32_t)L.units,
                           (const uint16_t *)L.mask, (const uint16_t *)small, (const uint32_t *)small_count, margin, v->touched_stamp,
                           v->frame_counter + 1, L.result);
        hv_profile_end(v, L.units);
        HV_HIP(hipGetLastError());
        HV_HIP(hipMemcpyAsync(h, L.result, sizeof(h), hipMemcpyDeviceToHost, v->stream));
        HV_HIP(hipStreamSynchronize(v->stream));
        if (h[CC_R_VOXELS_RESET] != 0ull) {
            // voxels changed: cached extraction results are void, the changed units carry the new stamp (the per-unit extraction
            // caches and hv_tsdf_dirty_keys see them), as after hv_tsdf_deintegrate
            v->content_version += 1;
            v->frame_counter += 1;
        }
    }
    if (stats != nullptr) {
        stats->components = L.components;
        stats->components_removed = (int64_t)h[CC_R_COMP_REMOVED];
        stats->sites = L.sites;
        stats->sites_removed = (int64_t)h[CC_R_SITES_REMOVED];
        stats->voxels_reset = (int64_t)h[CC_R_VOXELS_RESET];
        stats->units_changed = (int64_t)h[CC_R_UNITS_CHANGED];
        stats->units_emptied = (int64_t)h[CC_R_UNITS_EMPTIED];
    }
    return HV_OK;
}
