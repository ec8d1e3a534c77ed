// hv_tsdf_prune: give units of the TSDF mode back to the pool (include/hipvol.h states the contract).
//
// The pool is a bump allocator: units in use are the prefix [0, HV_CNT_BLOCKS) and a claim pass hands out the next index without
// clearing it.  Releasing units therefore means making the survivors a prefix again, in place:
//   scan     one wave per unit decides keep / outside the box / empty (all R^3 weights zero)           k_prune_scan
//   plan     exclusive scan of the keep flags, the counts, and the move list: with `kept` survivors,    k_prune_plan
//            the j-th survivor at an index >= kept goes into the j-th hole below kept
//   (the host reads the four counts: nothing released = nothing else happens, the volume is left as it was)
//   move     sources (>= kept) and destinations (< kept) are disjoint: one launch, one workgroup a unit  k_prune_move
//   zero     [kept, used) - every slot a later claim pass can hand out is all zero again
//   re-key   hv_rekey_in_place (hv_core.hip): table, stamps, touched state, counters - the sequence a rolled-back claim pass runs
// Extra device memory: 13 bytes per unit in use plus the re-key's copy of the table (20 bytes per slot); never a second pool.
#include <algorithm>

#include "hv_common.h"

namespace {

constexpr int UNIT_VEC = HV_TSDF_UNIT_BYTES / 16; // 16-byte words of a unit
static_assert(UNIT_VEC % (256 * 5) == 0, "k_prune_move copies a unit in rounds of 5 x 256 16-byte words");

enum : uint8_t { HV_PRUNE_KEEP = 0, HV_PRUNE_OUTSIDE = 1, HV_PRUNE_EMPTY = 2 };
enum { HV_PRUNE_KEPT = 0, HV_PRUNE_N_OUTSIDE = 1, HV_PRUNE_N_EMPTY = 2, HV_PRUNE_N_MOVES = 3, HV_PRUNE_RESULT_WORDS = 4 };

struct HvPruneBox {
    int32_t lo[3], hi[3]; // inclusive unit range
    int32_t bounded;      // 0: no box
    int32_t release_empty;
};

// One wave per unit.  The box test is arithmetic on the key; a unit it releases is not read.  The emptiness test is
// hv_tsdf_unit_has_weight.
__global__ __launch_bounds__(256) void k_prune_scan(const unsigned long long *__restrict__ block_keys, const char *__restrict__ pool, int32_t used,
                                                    HvPruneBox box, uint8_t *__restrict__ flags) {
    const int32_t unit = (int32_t)blockIdx.x * 4 + (int32_t)(threadIdx.x >> 6); // wave-uniform
    if (unit >= used) return;
    const int lane = hv_lane_id();
    uint8_t f = HV_PRUNE_KEEP;
    if (box.bounded) {
        int32_t x, y, z;
        hv_unpack_key(block_keys[unit], x, y, z);
        if (x < box.lo[0] || x > box.hi[0] || y < box.lo[1] || y > box.hi[1] || z < box.lo[2] || z > box.hi[2]) f = HV_PRUNE_OUTSIDE;
    }
    if (f == HV_PRUNE_KEEP && box.release_empty) {
        if (!hv_tsdf_unit_has_weight(pool, unit, lane)) f = HV_PRUNE_EMPTY;
    }
    if (lane == 0) flags[unit] = f;
}

// One workgroup: thread t owns the contiguous range of ceil(used / 1024) flags.  prefix[i] = survivors below i; result = {kept,
// outside, empty, moves}; move_src[j] / move_dst[j] = the j-th survivor at or above `kept` / the j-th hole below it (both in index
// order; there are as many of one as of the other: kept - prefix[kept]).
__global__ __launch_bounds__(1024) void k_prune_plan(const uint8_t *__restrict__ flags, int32_t used, int32_t *__restrict__ prefix,
                                                     int32_t *__restrict__ move_src, int32_t *__restrict__ move_dst, int32_t *__restrict__ result) {
    __shared__ int32_t s_scan[1024];
    __shared__ int32_t s_released[2];
    const int t = (int)threadIdx.x;
    const int64_t per = ((int64_t)used + 1023) / 1024;
    const int64_t b0 = t * per, b1 = b0 + per;
    const int32_t i0 = (int32_t)(b0 < used ? b0 : used), i1 = (int32_t)(b1 < used ? b1 : used);
    int32_t kept = 0, outside = 0, empty = 0;
    for (int32_t i = i0; i < i1; ++i) {
        const uint8_t f = flags[i];
        kept += f == HV_PRUNE_KEEP;
        outside += f == HV_PRUNE_OUTSIDE;
        empty += f == HV_PRUNE_EMPTY;
    }
    if (t < 2) s_released[t] = 0;
    s_scan[t] = kept;
    __syncthreads();
    if (outside) atomicAdd(&s_released[0], outside);
    if (empty) atomicAdd(&s_released[1], empty);
    for (int d = 1; d < 1024; d <<= 1) { // inclusive scan of the threads' counts
        const int32_t below = t >= d ? s_scan[t - d] : 0;
        __syncthreads();
        s_scan[t] += below;
        __syncthreads();
    }
    const int32_t total = s_scan[1023];
    int32_t run = s_scan[t] - kept;
    for (int32_t i = i0; i < i1; ++i) {
        prefix[i] = run;
        run += flags[i] == HV_PRUNE_KEEP;
    }
    __syncthreads(); // prefix[total] is another thread's
    const int32_t below_kept = total < used ? prefix[total] : total;
    for (int32_t i = i0; i < i1; ++i) {
        const bool keep = flags[i] == HV_PRUNE_KEEP;
        const int32_t p = prefix[i];
        if (i >= total && keep) move_src[p - below_kept] = i;
        if (i < total && !keep) move_dst[i - p] = i;
    }
    if (t == 0) {
        result[HV_PRUNE_KEPT] = total;
        result[HV_PRUNE_N_OUTSIDE] = s_released[0];
        result[HV_PRUNE_N_EMPTY] = s_released[1];
        result[HV_PRUNE_N_MOVES] = total - below_kept;
    }
}

// One workgroup per move: the unit's 80 KiB in 16-byte accesses, five loads in flight per lane, and its key.
__global__ __launch_bounds__(256) void k_prune_move(char *__restrict__ pool, unsigned long long *__restrict__ block_keys,
                                                    const int32_t *__restrict__ move_src, const int32_t *__restrict__ move_dst) {
    const int32_t from = move_src[blockIdx.x], to = move_dst[blockIdx.x];
    const uint4 *s = (const uint4 *)(pool + (size_t)from * HV_TSDF_UNIT_BYTES);
    uint4 *d = (uint4 *)(pool + (size_t)to * HV_TSDF_UNIT_BYTES);
    const int t = (int)threadIdx.x;
    for (int base = 0; base < UNIT_VEC; base += 256 * 5) {
        uint4 x[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) x[k] = s[base + k * 256 + t];
#pragma unroll
        for (int k = 0; k < 5; ++k) d[base + k * 256 + t] = x[k];
    }
    if (t == 0) block_keys[to] = block_keys[from];
}

} // namespace

extern "C" int hv_tsdf_prune(hv_volume *v, int32_t release_empty, const int32_t *unit_lo, const int32_t *unit_hi, hv_prune_stats *stats) {
    HV_REQUIRE(v != nullptr, HV_ERR_INVALID, "hv_tsdf_prune: null volume");
    HV_REQUIRE(v->cfg.mode == HV_MODE_TSDF, HV_ERR_MODE, "hv_tsdf_prune: volume is not in TSDF mode");
    HV_REQUIRE(v->tile[0] == 0 && v->tile[1] == 0 && v->tile[2] == 0 && v->tile[3] == 0, HV_ERR_MODE,
               "hv_tsdf_prune: not supported on a tile-sharded volume (its ranks must agree on the unit set)");
    HV_REQUIRE((unit_lo == nullptr) == (unit_hi == nullptr), HV_ERR_INVALID, "hv_tsdf_prune: unit_lo and unit_hi go together");
    HvPruneBox box{};
    box.release_empty = release_empty != 0;
    if (unit_lo != nullptr) {
        box.bounded = 1;
        for (int a = 0; a < 3; ++a) {
            HV_REQUIRE(unit_lo[a] <= unit_hi[a], HV_ERR_INVALID, "hv_tsdf_prune: empty unit range on axis %d: [%d, %d]", a, (int)unit_lo[a],
                       (int)unit_hi[a]);
            box.lo[a] = unit_lo[a];
            box.hi[a] = unit_hi[a];
        }
    }
    // drain the batch pipeline: nothing claims units or reads the table on the second stream while slots move (a later batch
    // starts a fresh chain on the main stream)
    int64_t used = 0;
    int rc = hv_tsdf_drain(v, "hv_tsdf_prune", false, &used);
    if (rc != HV_OK) return rc;
    if (!box.bounded && !box.release_empty) { // nothing to release by: a no-op
        if (stats != nullptr) *stats = hv_prune_stats{used, 0, 0, used};
        return HV_OK;
    }
    // keys without a block (an earlier claim pass overflowed) leave with the re-key, as in hv_reserve_blocks
    const bool repair = v->h_counters[HV_CNT_OVERFLOW] != 0 || v->overflow_latched;
    int32_t result[HV_PRUNE_RESULT_WORDS] = {(int32_t)used, 0, 0, 0};
    void *scratch = nullptr;
    int32_t *d_src = nullptr, *d_dst = nullptr;
    if (used > 0) {
        // [result 256 B][prefix used i32][move_src used i32][move_dst used i32][flags used u8]
        HV_HIP(hipMalloc(&scratch, 256 + 13 * (size_t)used));
        int32_t *d_result = (int32_t *)scratch;
        int32_t *d_prefix = (int32_t *)((char *)scratch + 256);
        d_src = d_prefix + used;
        d_dst = d_src + used;
        uint8_t *d_flags = (uint8_t *)(d_dst + used);
        hv_profile_begin(v);
        hipLaunchKernelGGL(k_prune_scan, dim3((unsigned)((used + 3) / 4)), dim3(256), 0, v->stream, (const unsigned long long *)v->table.block_keys,
                           (const char *)v->pool, (int32_t)used, box, d_flags);
        hv_profile_end(v, used);
        hipLaunchKernelGGL(k_prune_plan, dim3(1), dim3(1024), 0, v->stream, (const uint8_t *)d_flags, (int32_t)used, d_prefix, d_src, d_dst, d_result);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(result, d_result, sizeof(result), hipMemcpyDeviceToHost, v->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(v->stream);
        if (e != hipSuccess) {
            (void)hipFree(scratch);
            hv_set_error("hv_tsdf_prune: the scan failed: %s", hipGetErrorString(e));
            return HV_ERR_DEVICE;
        }
    }
    const int64_t kept = result[HV_PRUNE_KEPT], released = used - kept, moves = result[HV_PRUNE_N_MOVES];
    if (stats != nullptr) {
        stats->units_before = used;
        stats->units_outside = result[HV_PRUNE_N_OUTSIDE];
        stats->units_empty = result[HV_PRUNE_N_EMPTY];
        stats->units_after = kept;
    }
    if (released == 0 && !repair) { // the volume is left exactly as it was, caches included
        if (scratch) HV_HIP(hipFree(scratch));
        return HV_OK;
    }
    hipError_t e = hipSuccess;
    if (moves > 0) {
        hipLaunchKernelGGL(k_prune_move, dim3((unsigned)moves), dim3(256), 0, v->stream, (char *)v->pool, v->table.block_keys, (const int32_t *)d_src,
                           (const int32_t *)d_dst);
        e = hipGetLastError();
    }
    if (e == hipSuccess && released > 0)
        e = hipMemsetAsync((char *)v->pool + (size_t)kept * HV_TSDF_UNIT_BYTES, 0, (size_t)released * HV_TSDF_UNIT_BYTES, v->stream);
    // pool slots moved: the per-unit extraction caches (hv_rekey_in_place bumps extract_epoch), cached extraction results and a stored
    // halo plan describe a volume that no longer exists
    v->content_version += 1;
    v->halo_plan_n = 0;
    rc = e == hipSuccess ? hv_rekey_in_place(v, kept) : HV_ERR_DEVICE; // synchronises the stream
    if (e != hipSuccess) hv_set_error("hv_tsdf_prune: compacting the pool failed: %s", hipGetErrorString(e));
    if (scratch) (void)hipFree(scratch);
    return rc;
}
