// libpyslam_hipvol.so - the exchange of TSDF units between GPUs: numerators export / import (a gather onto one rank) and the halo
// merge of image-tile-sharded volumes (include/hipvol.h "halo merge", pyslam_amd/distributed.py::merge_halo).
//
// The library packs and unpacks on the device (k_tsdf_export / k_tsdf_halo_unpack: a unit travels as five float numerators per
// voxel, tsdf * w, w and the colour sums, so that an all-reduce adds observations); the caller runs the collectives with whatever
// transport it has - torch.distributed over RCCL in pyslam_amd/distributed.py.
//
// Each rule stands once: the plan rule in hv_halo_plan.h (hv_halo_run_rule: the host plans and k_halo_decide walk the runs of equal
// keys with it); the unit <-> payload codec in hv_voxel_numerators / hv_voxel_from_numerators, with one export and one unpack launch
// (an import is an unpack that keeps every unit) behind the staged and the _planned entry points; the dirty lister k_halo_lists
// behind hv_tsdf_dirty_keys and hv_merge_halo_lists_device; the claim-until-it-fits loop in hv_claim_keys.
//
// The halo merge needs every rank's list of units written since its last merge and its list of units held, and from the
// all-gathered lists the plan: the keys some rank updated that two ranks or more hold, with this rank's action.  Two forms:
//   host    hv_tsdf_dirty_keys + hv_merge_halo_plan / _plan_held (a std::sort of the entries) + hv_merge_halo_pack / _unpack;
//   device  (round 6) the lists are written as packed 64-bit keys into DEVICE buffers of the caller (torch
//           tensors: what RCCL's all_gather_into_tensor takes), the plan is a device radix sort + two small kernels, and the shared
//           keys / actions stay in the volume for hv_merge_halo_pack_planned / _unpack_planned.  What still crosses to the host is
//           three integers per merge: the two list lengths (they size the gather) and the number of shared units (it sizes the
//           payload).  Same plan as the host function, in packed-key order instead of (x, y, z) order - every rank of a group takes
//           the same path, and tests/test_gpu_distributed.py holds the two to each other.
#include <algorithm>
#include <array>
#include <cstring>
#include <vector>

#include "hv_common.h"
#include "hv_halo_plan.h"
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

// dirty units (stamp later than the last merge) and held units (every allocated unit) of one volume, as packed keys
__global__ __launch_bounds__(256) void k_halo_lists(HvTable table, const int32_t *__restrict__ stamp, int32_t merge_stamp, int32_t n_blocks,
                                                     unsigned long long *__restrict__ dirty, int64_t dirty_cap, unsigned long long *__restrict__ held,
                                                     int64_t held_cap) {
    const int32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    bool is_dirty = false;
    unsigned long long key = 0ull;
    if (idx < n_blocks) {
        key = table.block_keys[idx];
        const int32_t slot = hv_table_find(table, key);
        is_dirty = slot >= 0 && stamp[slot] > merge_stamp;
        if (idx < held_cap) held[idx] = key;
    }
    const int32_t at = hv_wave_append(&table.counters[HV_CNT_OUT], is_dirty);
    if (is_dirty && at < dirty_cap) dirty[at] = key;
}

struct HvHaloSpans {
    int32_t world;
    int64_t dirty_off[65], held_off[65]; // exclusive prefixes of the ranks' counts (world <= 64)
};
// the gathered, padded lists [world][stride] -> one entry array: every dirty entry (by rank), then every held entry (by rank);
// value = rank << 1 | held
__global__ __launch_bounds__(256) void k_halo_entries(HvHaloSpans S, const unsigned long long *__restrict__ dirty, int64_t dirty_stride,
                                                       const unsigned long long *__restrict__ held, int64_t held_stride,
                                                       unsigned long long *__restrict__ keys, int32_t *__restrict__ vals) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nd = S.dirty_off[S.world], nh = S.held_off[S.world];
    if (i >= nd + nh) return;
    const bool is_held = i >= nd;
    const int64_t j = is_held ? i - nd : i;
    const int64_t *off = is_held ? S.held_off : S.dirty_off;
    int r = 0;
    while (r + 1 < S.world && off[r + 1] <= j) ++r;
    const int64_t k = j - off[r];
    keys[i] = is_held ? held[(int64_t)r * held_stride + k] : dirty[(int64_t)r * dirty_stride + k];
    vals[i] = (r << 1) | (is_held ? 1 : 0);
}
// sorted by key (stable: a key's dirty entries come first, then its holders by ascending rank): the head of a key's run decides
__global__ __launch_bounds__(256) void k_halo_decide(const unsigned long long *__restrict__ keys, const int32_t *__restrict__ vals, int64_t n, int32_t rank,
                                                      int32_t all_dirty_kept, int32_t *__restrict__ flag, uint8_t *__restrict__ act) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int32_t f = 0;
    uint8_t a = 0;
    const unsigned long long key = keys[i];
    if (i == 0 || keys[i - 1] != key) {
        int64_t m = 1;
        while (i + m < n && keys[i + m] == key) ++m;
        f = hv_halo_run_rule(vals + i, m, rank, all_dirty_kept != 0, &a) ? 1 : 0;
    }
    flag[i] = f;
    act[i] = a;
}
__global__ __launch_bounds__(256) void k_halo_emit(const unsigned long long *__restrict__ keys, const int32_t *__restrict__ flag, const int32_t *__restrict__ pos,
                                                    const uint8_t *__restrict__ act, int64_t n, int32_t *__restrict__ out_keys, uint8_t *__restrict__ out_act) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !flag[i]) return;
    const int32_t at = pos[i];
    int32_t x, y, z;
    hv_unpack_key(keys[i], x, y, z);
    out_keys[at * 3 + 0] = x;
    out_keys[at * 3 + 1] = y;
    out_keys[at * 3 + 2] = z;
    out_act[at] = act[i];
}

// ---- the unit <-> payload codec: a voxel travels as five float numerators {tsdf * w, w, sum r, sum g, sum b} ----
__device__ __forceinline__ void hv_voxel_numerators(const char *unit, int word, float *out) {
    const float tsdf = ((const float *)unit)[word];
    const uint32_t w = ((const uint32_t *)(unit + HV_TSDF_PLANE_BYTES))[word];
    out[0] = tsdf * (float)w;
    out[1] = (float)w;
#pragma unroll
    for (int c = 2; c < 5; ++c) out[c] = (float)((const uint32_t *)(unit + c * HV_TSDF_PLANE_BYTES))[word];
}
// ... and back: the voxel's state := the numerators n, or zero where n is null.  A weight of 0 gives tsdf 0 whatever the numerator.
__device__ __forceinline__ void hv_voxel_from_numerators(char *unit, int word, const float *n) {
    float tsdf = 0.f;
    uint32_t p[5] = {0u, 0u, 0u, 0u, 0u};
    if (n != nullptr) {
        tsdf = n[1] > 0.f ? n[0] / n[1] : 0.f;
#pragma unroll
        for (int c = 1; c < 5; ++c) p[c] = (uint32_t)n[c];
    }
    ((float *)unit)[word] = tsdf;
#pragma unroll
    for (int c = 1; c < 5; ++c) ((uint32_t *)(unit + c * HV_TSDF_PLANE_BYTES))[word] = p[c];
}
// entry ui of a key list [k,3] -> the pool index of its unit, or -1 (key out of range, or no such unit in this volume)
__device__ __forceinline__ int32_t hv_keyed_unit(const HvTable &table, const int32_t *__restrict__ keys, int64_t ui) {
    const int32_t kx = keys[ui * 3], ky = keys[ui * 3 + 1], kz = keys[ui * 3 + 2];
    if (!hv_key_in_range(kx, ky, kz)) return -1;
    const int32_t slot = hv_table_find(table, hv_pack_key(kx, ky, kz));
    return slot >= 0 ? table.vals[slot] : -1;
}

// one thread per voxel of every listed unit; zeros for a unit this volume does not hold
__global__ void k_tsdf_export(HvTable table, const char *__restrict__ pool, const int32_t *__restrict__ keys,
                              int64_t k, float *__restrict__ payload) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= k * HV_TSDF_RRR) return;
    float out[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    const int32_t idx = hv_keyed_unit(table, keys, gid / HV_TSDF_RRR);
    if (idx >= 0) hv_voxel_numerators(pool + (int64_t)idx * HV_TSDF_UNIT_BYTES, (int)(gid % HV_TSDF_RRR), out);
    float *dst = payload + gid * 5;
#pragma unroll
    for (int c = 0; c < 5; ++c) dst[c] = out[c];
}

__global__ void k_tsdf_import_claim(HvTable table, const int32_t *__restrict__ keys, int64_t k) {
    const int64_t ui = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (ui >= k) return;
    const int32_t kx = keys[ui * 3], ky = keys[ui * 3 + 1], kz = keys[ui * 3 + 2];
    if (!hv_key_in_range(kx, ky, kz)) {
        atomicAdd(&table.counters[HV_CNT_DROPPED], 1);
        return;
    }
    hv_table_insert(table, hv_pack_key(kx, ky, kz));
}

// action[u]: 0 = leave the unit alone (this GPU does not hold it), 1 = replace its state by the reduced numerators (this GPU
// keeps the unit), 2 = zero it (another GPU keeps it; this one goes on fusing deltas into an empty unit).  A null action: 1 for
// every unit (hv_tsdf_import_numerators).  A unit this volume does not hold is left out.
__global__ void k_tsdf_halo_unpack(HvTable table, char *__restrict__ pool, const int32_t *__restrict__ keys, int64_t k,
                                   const float *__restrict__ payload, const uint8_t *__restrict__ action) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= k * HV_TSDF_RRR) return;
    const int64_t ui = gid / HV_TSDF_RRR;
    const int act = action != nullptr ? action[ui] : 1;
    if (act == 0) return;
    const int32_t idx = hv_keyed_unit(table, keys, ui);
    if (idx < 0) return;
    hv_voxel_from_numerators(pool + (int64_t)idx * HV_TSDF_UNIT_BYTES, (int)(gid % HV_TSDF_RRR), act == 1 ? payload + gid * 5 : nullptr);
}

// ---- the launches the staged and the _planned entry points share: k keys [k,3] and the payload in device memory, queued on the
// volume's stream ----
static int halo_launch_export(hv_volume *v, const int32_t *d_keys, int64_t k, float *d_payload) {
    hipLaunchKernelGGL(k_tsdf_export, dim3((unsigned)((k * HV_TSDF_RRR + 255) / 256)), dim3(256), 0, v->stream, v->table, (const char *)v->pool, d_keys, k,
                       d_payload);
    HV_HIP(hipGetLastError());
    return HV_OK;
}
static int halo_launch_unpack(hv_volume *v, const int32_t *d_keys, int64_t k, const float *d_payload, const uint8_t *d_action) {
    hipLaunchKernelGGL(k_tsdf_halo_unpack, dim3((unsigned)((k * HV_TSDF_RRR + 255) / 256)), dim3(256), 0, v->stream, v->table, (char *)v->pool, d_keys, k,
                       d_payload, d_action);
    HV_HIP(hipGetLastError());
    return HV_OK;
}
// the dirty list (and the held list, where `held` is given) of the volume's nb units as packed keys; waits for the one number the
// caller sizes its next step by: *n_dirty is the true count, also above dirty_cap
static int halo_launch_lists(hv_volume *v, int64_t nb, unsigned long long *dirty, int64_t dirty_cap, unsigned long long *held, int64_t held_cap,
                             int64_t *n_dirty) {
    HV_HIP(hipMemsetAsync(&v->table.counters[HV_CNT_OUT], 0, sizeof(int32_t), v->stream));
    hipLaunchKernelGGL(k_halo_lists, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, v->stream, v->table, (const int32_t *)v->touched_stamp,
                       v->merge_stamp, (int32_t)nb, dirty, dirty_cap, held, held_cap);
    HV_HIP(hipGetLastError());
    const int rc = hv_read_counters(v); // (synchronises)
    if (rc != HV_OK) return rc;
    *n_dirty = v->h_counters[HV_CNT_OUT];
    return HV_OK;
}

// the claim pass of the calls that are handed keys (hv_tsdf_import_numerators here, the unpacks of hv_pack.hip / hv_grid_pack.hip)
// - always verified, these calls wait for the GPU anyway: a pool that is too small grows before anything is written, or the call
// fails with the volume unchanged (a gather onto a root whose pool was sized like every other rank's)
int hv_claim_keys(hv_volume *v, const int32_t *d_keys, int64_t k) {
    bool checked_unused = false;
    int rc = hv_capacity_gate(v, &checked_unused);
    for (int attempt = 0; rc == HV_OK; ++attempt) {
        hipLaunchKernelGGL(k_tsdf_import_claim, dim3((unsigned)((k + 255) / 256)), dim3(256), 0, v->stream, v->table, d_keys, k);
        rc = hv_claims_fit(v);
        if (rc != HV_RETRY_CLAIM) break;
        rc = attempt < 8 ? HV_OK : HV_ERR_CAPACITY;
    }
    return rc;
}

// the argument checks of the two host plans, then the one plan (hv_halo_plan.h)
static int halo_plan_checked(const char *fn, const int32_t *dirty_keys, const int64_t *dirty_counts, const int32_t *held_keys,
                             const int64_t *held_counts, int32_t world_size, int32_t rank, int32_t *shared_keys, uint8_t *action, int64_t cap,
                             int64_t *n_shared) {
    HV_REQUIRE(dirty_counts != nullptr && held_counts != nullptr && n_shared != nullptr && world_size >= 1 && rank >= 0 && rank < world_size,
               HV_ERR_INVALID, "%s: bad argument", fn);
    int64_t nd = 0, nh = 0;
    for (int r = 0; r < world_size; ++r) {
        nd += dirty_counts[r];
        nh += held_counts[r];
    }
    HV_REQUIRE((nd == 0 || dirty_keys != nullptr) && (nh == 0 || held_keys != nullptr), HV_ERR_INVALID, "%s: null key list", fn);
    *n_shared = hv_halo_plan_host(dirty_keys, dirty_counts, held_keys, held_counts, world_size, rank, shared_keys, action, cap);
    return HV_OK;
}

extern "C" {

int hv_merge_halo_lists_device(hv_volume *v, int64_t *d_dirty_keys, int64_t dirty_cap, int64_t *d_held_keys, int64_t held_cap, int64_t *n_dirty,
                               int64_t *n_held) {
    HV_REQUIRE(v != nullptr && n_dirty != nullptr && n_held != nullptr, HV_ERR_INVALID, "hv_merge_halo_lists_device: null argument");
    HV_REQUIRE(v->cfg.mode == HV_MODE_TSDF, HV_ERR_MODE, "hv_merge_halo_lists_device: not a TSDF volume");
    HV_HIP(hipSetDevice(v->device));
    int64_t nb = 0;
    int rc = hv_num_blocks(v, &nb);
    if (rc != HV_OK) return rc;
    *n_dirty = 0;
    *n_held = nb;
    if (nb == 0 || d_dirty_keys == nullptr || d_held_keys == nullptr) return HV_OK; // (size query: an upper bound of both lists is nb)
    return halo_launch_lists(v, nb, (unsigned long long *)d_dirty_keys, dirty_cap, (unsigned long long *)d_held_keys, held_cap, n_dirty);
}

int hv_merge_halo_plan_device(hv_volume *v, const int64_t *d_dirty_all, const int64_t *dirty_counts, int64_t dirty_stride, const int64_t *d_held_all,
                              const int64_t *held_counts, int64_t held_stride, int32_t world_size, int32_t rank, int32_t all_dirty_kept,
                              int64_t *n_shared) {
    HV_REQUIRE(v != nullptr && dirty_counts != nullptr && held_counts != nullptr && n_shared != nullptr, HV_ERR_INVALID,
               "hv_merge_halo_plan_device: null argument");
    v->halo_plan_n = 0; // (before the checks below: a refused call leaves no plan of earlier lists behind)
    *n_shared = 0;
    HV_REQUIRE(world_size >= 1 && world_size <= 64 && rank >= 0 && rank < world_size, HV_ERR_INVALID, "hv_merge_halo_plan_device: bad rank / world size");
    HV_REQUIRE(v->cfg.mode == HV_MODE_TSDF, HV_ERR_MODE, "hv_merge_halo_plan_device: not a TSDF volume");
    HV_HIP(hipSetDevice(v->device));
    HvHaloSpans S;
    S.world = world_size;
    S.dirty_off[0] = S.held_off[0] = 0;
    for (int r = 0; r < world_size; ++r) {
        HV_REQUIRE(dirty_counts[r] >= 0 && dirty_counts[r] <= dirty_stride && held_counts[r] >= 0 && held_counts[r] <= held_stride, HV_ERR_INVALID,
                   "hv_merge_halo_plan_device: a list is longer than its stride");
        S.dirty_off[r + 1] = S.dirty_off[r] + dirty_counts[r];
        S.held_off[r + 1] = S.held_off[r] + held_counts[r];
    }
    const int64_t n = S.dirty_off[world_size] + S.held_off[world_size];
    if (n == 0) return HV_OK;
    HV_REQUIRE(n < (1ll << 31) && d_dirty_all != nullptr && d_held_all != nullptr, HV_ERR_INVALID, "hv_merge_halo_plan_device: bad lists");
    // scratch: [keys in n u64][keys out n u64][vals in n i32][vals out n i32][flag n i32][pos n + 1 i32][act n u8] + the sort's own
    const size_t a8 = sizeof(uint64_t) * (size_t)n, a4 = sizeof(int32_t) * (size_t)(n + 1);
    int rc = hv_ensure_buffer(v, &v->out_c, &v->out_c_bytes, 2 * a8 + 4 * a4 + (size_t)n + 64);
    if (rc != HV_OK) return rc;
    char *p = (char *)v->out_c;
    unsigned long long *k_in = (unsigned long long *)p, *k_out = (unsigned long long *)(p + a8);
    int32_t *v_in = (int32_t *)(p + 2 * a8), *v_out = (int32_t *)(p + 2 * a8 + a4), *flag = (int32_t *)(p + 2 * a8 + 2 * a4),
            *pos = (int32_t *)(p + 2 * a8 + 3 * a4);
    uint8_t *act = (uint8_t *)(p + 2 * a8 + 4 * a4);
    const unsigned grid = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(k_halo_entries, dim3(grid), dim3(256), 0, v->stream, S, (const unsigned long long *)d_dirty_all, dirty_stride,
                       (const unsigned long long *)d_held_all, held_stride, k_in, v_in);
    size_t tmp = 0;
    HV_HIP(rocprim::radix_sort_pairs(nullptr, tmp, k_in, k_out, v_in, v_out, (size_t)n, 0, 64, v->stream));
    rc = hv_ensure_buffer(v, &v->sort_tmp, &v->sort_tmp_bytes, tmp);
    if (rc != HV_OK) return rc;
    tmp = v->sort_tmp_bytes;
    HV_HIP(rocprim::radix_sort_pairs(v->sort_tmp, tmp, k_in, k_out, v_in, v_out, (size_t)n, 0, 64, v->stream)); // (stable: LSD radix)
    hipLaunchKernelGGL(k_halo_decide, dim3(grid), dim3(256), 0, v->stream, k_out, v_out, n, rank, all_dirty_kept, flag, act);
    HV_HIP(hipMemsetAsync(flag + n, 0, sizeof(int32_t), v->stream)); // the scan's extra element: its output there is the total
    size_t tmp2 = 0;
    HV_HIP(rocprim::exclusive_scan(nullptr, tmp2, flag, pos, 0, (size_t)(n + 1), rocprim::plus<int32_t>(), v->stream));
    rc = hv_ensure_buffer(v, &v->sort_tmp, &v->sort_tmp_bytes, tmp2);
    if (rc != HV_OK) return rc;
    tmp2 = v->sort_tmp_bytes;
    HV_HIP(rocprim::exclusive_scan(v->sort_tmp, tmp2, flag, pos, 0, (size_t)(n + 1), rocprim::plus<int32_t>(), v->stream));
    int32_t total = 0;
    HV_HIP(hipMemcpyAsync(&total, pos + n, sizeof(int32_t), hipMemcpyDeviceToHost, v->stream));
    HV_HIP(hipStreamSynchronize(v->stream)); // (the one number the payload's size depends on)
    if (total > 0) {
        rc = hv_ensure_buffer(v, &v->halo_plan, &v->halo_plan_bytes, (size_t)total * 13 + 64);
        if (rc != HV_OK) return rc;
        hipLaunchKernelGGL(k_halo_emit, dim3(grid), dim3(256), 0, v->stream, k_out, flag, pos, act, n, (int32_t *)v->halo_plan,
                           (uint8_t *)v->halo_plan + (size_t)total * 12);
        HV_HIP(hipGetLastError());
    }
    v->halo_plan_n = total;
    *n_shared = total;
    return HV_OK;
}

// the plan as host arrays (inspection, tests): shared_keys [n, 3] i32, action [n] u8
int hv_merge_halo_plan_fetch(hv_volume *v, int32_t *shared_keys, uint8_t *action, int64_t cap, int64_t *n_shared) {
    HV_REQUIRE(v != nullptr && n_shared != nullptr, HV_ERR_INVALID, "hv_merge_halo_plan_fetch: null argument");
    *n_shared = v->halo_plan_n;
    const int64_t m = std::min<int64_t>(v->halo_plan_n, cap);
    if (shared_keys == nullptr || action == nullptr || m <= 0) return HV_OK;
    HV_HIP(hipSetDevice(v->device));
    HV_HIP(hipMemcpyAsync(shared_keys, v->halo_plan, sizeof(int32_t) * 3 * (size_t)m, hipMemcpyDeviceToHost, v->stream));
    HV_HIP(hipMemcpyAsync(action, (const uint8_t *)v->halo_plan + (size_t)v->halo_plan_n * 12, (size_t)m, hipMemcpyDeviceToHost, v->stream));
    HV_HIP(hipStreamSynchronize(v->stream));
    return HV_OK;
}

int hv_tsdf_export_numerators(hv_volume *v, const int32_t *keys, int64_t k, float *payload, int32_t loc) {
    HV_REQUIRE(v != nullptr && (k == 0 || (keys != nullptr && payload != nullptr)), HV_ERR_INVALID,
               "hv_tsdf_export_numerators: null argument");
    HV_REQUIRE(v->cfg.mode == HV_MODE_TSDF, HV_ERR_MODE, "hv_tsdf_export_numerators: not a TSDF volume");
    if (k == 0) return HV_OK;
    HV_HIP(hipSetDevice(v->device));
    HvStage st(v, loc); // (the keys are host memory by contract)
    const int i_keys = st.in(keys, sizeof(int32_t) * 3 * (size_t)k, HV_HOST), o_payload = st.out(payload, sizeof(float) * 5 * HV_TSDF_RRR * (size_t)k);
    int rc = st.commit(&v->stage, &v->stage_bytes);
    if (rc != HV_OK) return rc;
    if ((rc = halo_launch_export(v, st.dev<const int32_t>(i_keys), k, st.dev<float>(o_payload))) != HV_OK) return rc;
    if ((rc = st.finish()) != HV_OK) return rc;
    HV_HIP(hipStreamSynchronize(v->stream)); // (a device payload too: this call has always been complete on return)
    return HV_OK;
}

int hv_tsdf_import_numerators(hv_volume *v, const int32_t *keys, int64_t k, const float *payload, int32_t loc) {
    HV_REQUIRE(v != nullptr && (k == 0 || (keys != nullptr && payload != nullptr)), HV_ERR_INVALID,
               "hv_tsdf_import_numerators: null argument");
    HV_REQUIRE(v->cfg.mode == HV_MODE_TSDF, HV_ERR_MODE, "hv_tsdf_import_numerators: not a TSDF volume");
    if (k == 0) return HV_OK;
    v->content_version += 1;
    v->extract_epoch += 1; // (writes voxels without stamping their units)
    HV_HIP(hipSetDevice(v->device));
    HvStage st(v, loc); // (the keys are host memory by contract)
    const int i_keys = st.in(keys, sizeof(int32_t) * 3 * (size_t)k, HV_HOST), i_payload = st.in(payload, sizeof(float) * 5 * HV_TSDF_RRR * (size_t)k);
    int rc = st.commit(&v->stage, &v->stage_bytes);
    if (rc != HV_OK) return rc;
    const int32_t *d_keys = st.dev<const int32_t>(i_keys);
    if ((rc = hv_claim_keys(v, d_keys, k)) != HV_OK) return rc; // the imported units are claimed first: nothing is written unless they fit
    if ((rc = halo_launch_unpack(v, d_keys, k, st.dev<const float>(i_payload), nullptr)) != HV_OK) return rc; // (no actions: every unit is kept)
    hv_launch_publish_status(v); // the imported units are part of the published occupancy (a later rollback keeps them)
    HV_HIP(hipStreamSynchronize(v->stream));
    return HV_OK;
}

// ---- halo merge entry points (SURVEY 8b hv_merge_halo, 8e): the library packs / unpacks on the device, the caller runs
// the two collectives (all-gather of key lists, all-reduce of the dense buffer) with whatever transport it has -
// torch.distributed over RCCL in pyslam_amd/distributed.py ----
int hv_tsdf_dirty_keys(hv_volume *v, int32_t *keys, int64_t cap, int64_t *n) {
    HV_REQUIRE(v != nullptr && n != nullptr, HV_ERR_INVALID, "hv_tsdf_dirty_keys: null argument");
    HV_REQUIRE(v->cfg.mode == HV_MODE_TSDF, HV_ERR_MODE, "hv_tsdf_dirty_keys: not a TSDF volume");
    HV_HIP(hipSetDevice(v->device));
    int64_t nb = 0;
    int rc = hv_num_blocks(v, &nb);
    if (rc != HV_OK) return rc;
    *n = 0;
    if (nb == 0) return HV_OK;
    v->mesh_cache_version = v->points_cache_version = 0; // out_a is reused below
    rc = hv_ensure_buffer(v, &v->out_a, &v->out_a_bytes, sizeof(uint64_t) * (size_t)nb);
    if (rc != HV_OK) return rc;
    int64_t nd = 0;
    rc = halo_launch_lists(v, nb, (unsigned long long *)v->out_a, nb, nullptr, 0, &nd);
    if (rc != HV_OK) return rc;
    *n = nd;
    if (keys == nullptr || nd == 0) return HV_OK;
    std::vector<uint64_t> packed((size_t)nd);
    HV_HIP(hipMemcpy(packed.data(), v->out_a, sizeof(uint64_t) * (size_t)nd, hipMemcpyDeviceToHost));
    std::vector<std::array<int32_t, 3>> out((size_t)nd);
    for (int64_t i = 0; i < nd; ++i) hv_unpack_key(packed[i], out[i][0], out[i][1], out[i][2]);
    std::sort(out.begin(), out.end());
    const int64_t m = std::min(nd, cap);
    for (int64_t i = 0; i < m; ++i) memcpy(keys + i * 3, out[i].data(), 12);
    return HV_OK;
}

int hv_tsdf_mark_merged(hv_volume *v) {
    HV_REQUIRE(v != nullptr, HV_ERR_INVALID, "hv_tsdf_mark_merged: null volume");
    HV_REQUIRE(v->cfg.mode == HV_MODE_TSDF, HV_ERR_MODE, "hv_tsdf_mark_merged: not a TSDF volume");
    v->merge_stamp = v->frame_counter;
    return HV_OK;
}

// the plan from the dirty lists alone: the held plan with every lister taken as a holder (a rank lists a key once, so the lowest
// lister is the lowest holder)
int hv_merge_halo_plan(const int32_t *gathered_keys, const int64_t *counts, int32_t world_size, int32_t rank,
                       int32_t *shared_keys, uint8_t *action, int64_t cap, int64_t *n_shared) {
    return halo_plan_checked("hv_merge_halo_plan", gathered_keys, counts, gathered_keys, counts, world_size, rank, shared_keys, action, cap, n_shared);
}

int hv_merge_halo_plan_held(const int32_t *dirty_keys, const int64_t *dirty_counts, const int32_t *held_keys,
                            const int64_t *held_counts, int32_t world_size, int32_t rank, int32_t *shared_keys, uint8_t *action,
                            int64_t cap, int64_t *n_shared) {
    return halo_plan_checked("hv_merge_halo_plan_held", dirty_keys, dirty_counts, held_keys, held_counts, world_size, rank, shared_keys, action, cap,
                             n_shared);
}

int hv_merge_halo_pack(hv_volume *v, const int32_t *shared_keys, int64_t k, float *payload, int32_t loc) {
    return hv_tsdf_export_numerators(v, shared_keys, k, payload, loc);
}

int hv_merge_halo_unpack(hv_volume *v, const int32_t *shared_keys, int64_t k, const float *payload, const uint8_t *action,
                         int32_t loc) {
    HV_REQUIRE(v != nullptr && (k == 0 || (shared_keys != nullptr && payload != nullptr && action != nullptr)), HV_ERR_INVALID,
               "hv_merge_halo_unpack: null argument");
    HV_REQUIRE(v->cfg.mode == HV_MODE_TSDF, HV_ERR_MODE, "hv_merge_halo_unpack: not a TSDF volume");
    if (k == 0) return HV_OK;
    v->content_version += 1;
    v->extract_epoch += 1; // (writes voxels without stamping their units)
    HV_HIP(hipSetDevice(v->device));
    HvStage st(v, loc); // (the keys and the actions are host memory by contract)
    const int i_keys = st.in(shared_keys, (size_t)k * 12, HV_HOST), i_action = st.in(action, (size_t)k, HV_HOST),
              i_payload = st.in(payload, sizeof(float) * 5 * HV_TSDF_RRR * (size_t)k);
    int rc = st.commit(&v->stage, &v->stage_bytes);
    if (rc != HV_OK) return rc;
    rc = halo_launch_unpack(v, st.dev<const int32_t>(i_keys), k, st.dev<const float>(i_payload), st.dev<const uint8_t>(i_action));
    if (rc != HV_OK) return rc;
    HV_HIP(hipStreamSynchronize(v->stream)); // (this call has always been complete on return)
    return HV_OK;
}

// ... with the plan hv_merge_halo_plan_device left in the volume: units [first, first + count) of it, device payload,
// nothing staged, nothing waited for - the caller orders its collective against the volume's stream
int hv_merge_halo_pack_planned(hv_volume *v, int64_t first, int64_t count, float *d_payload) {
    HV_REQUIRE(v != nullptr && (count == 0 || d_payload != nullptr), HV_ERR_INVALID, "hv_merge_halo_pack_planned: null argument");
    HV_REQUIRE(v->cfg.mode == HV_MODE_TSDF, HV_ERR_MODE, "hv_merge_halo_pack_planned: not a TSDF volume");
    HV_REQUIRE(first >= 0 && count >= 0 && first + count <= v->halo_plan_n, HV_ERR_INVALID, "hv_merge_halo_pack_planned: range outside the plan");
    if (count == 0) return HV_OK;
    HV_HIP(hipSetDevice(v->device));
    return halo_launch_export(v, (const int32_t *)v->halo_plan + 3 * first, count, d_payload);
}

int hv_merge_halo_unpack_planned(hv_volume *v, int64_t first, int64_t count, const float *d_payload) {
    HV_REQUIRE(v != nullptr && (count == 0 || d_payload != nullptr), HV_ERR_INVALID, "hv_merge_halo_unpack_planned: null argument");
    HV_REQUIRE(v->cfg.mode == HV_MODE_TSDF, HV_ERR_MODE, "hv_merge_halo_unpack_planned: not a TSDF volume");
    HV_REQUIRE(first >= 0 && count >= 0 && first + count <= v->halo_plan_n, HV_ERR_INVALID, "hv_merge_halo_unpack_planned: range outside the plan");
    if (count == 0) return HV_OK;
    v->content_version += 1;
    v->extract_epoch += 1; // (writes voxels without stamping their units)
    HV_HIP(hipSetDevice(v->device));
    return halo_launch_unpack(v, (const int32_t *)v->halo_plan + 3 * first, count, d_payload,
                              (const uint8_t *)v->halo_plan + (size_t)v->halo_plan_n * 12 + first);
}

} // extern "C"
