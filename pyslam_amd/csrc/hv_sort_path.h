// The device-wide radix-sort path of the VOXEL_GRID integrate (hv_voxel_grid.hip) and the semantic grids' (hv_semantic.hip): the only
// path for calls beyond the bin path's limits (hv_bins.h) and for the batched replay, and the reference the tests hold the bin path to.
//   keys      1 thread / point: the block is claimed in the hash, sort key = (table slot << local_bits) | local voxel index,
//             HV_SORT_SENTINEL for a point that is not fused; value = point index
//   sort      rocPRIM LSD pairs sort (stable): points grouped per voxel, point-index order kept inside every voxel
//   reduce    the first thread of every voxel run folds its points in point order
// The two grids differ in the keys and reduce kernels only; the host sequence around them is here.
#pragma once
#include <algorithm>

#include "hv_common.h"
#include <rocprim/device/device_radix_sort.hpp>

static constexpr uint32_t HV_SORT_SENTINEL = 0xFFFFFFFFu;

// the key's width follows the table: slot bits + local voxel bits, and one more for the sentinel
static inline int hv_sort_bits(const hv_volume *v) {
    int slot_bits = 0;
    while ((1ull << slot_bits) < v->table_capacity) slot_bits++;
    return std::min(32, slot_bits + v->local_bits + 1);
}

static inline int hv_sort_pairs(hv_volume *v, void *tmp, size_t &bytes, int64_t n) {
    HV_HIP(rocprim::radix_sort_pairs(tmp, bytes, v->sort_keys_in, v->sort_keys_out, v->sort_vals_in, v->sort_vals_out, (size_t)n, 0,
                                     hv_sort_bits(v), v->stream));
    return HV_OK;
}

// `keys()` launches the caller's key kernel into v->sort_keys_in / sort_vals_in, `reduce()` its reduce over v->sort_keys_out /
// sort_vals_out.  `checked`: the capacity gate could not vouch for the call - the claims are looked at synchronously, and blocks
// that did not fit make the pool grow and the keys run again (sort keys embed table slots; the sort's width and temporary follow).
template <typename Keys, typename Reduce>
static int hv_sort_path(hv_volume *v, int64_t n, bool checked, Keys keys, Reduce reduce) {
    for (int attempt = 0;; ++attempt) {
        size_t bytes = 0;
        int rc = hv_sort_pairs(v, nullptr, bytes, n); // size query
        if (rc == HV_OK) rc = hv_ensure_buffer(v, &v->sort_tmp, &v->sort_tmp_bytes, bytes);
        if (rc != HV_OK) return rc;
        keys();
        if (!checked) break;
        rc = hv_claims_fit(v);
        if (rc == HV_OK) break;
        if (rc != HV_RETRY_CLAIM || attempt >= 8) return rc == HV_RETRY_CLAIM ? HV_ERR_CAPACITY : rc;
    }
    size_t bytes = v->sort_tmp_bytes;
    const int rc = hv_sort_pairs(v, v->sort_tmp, bytes, n);
    if (rc != HV_OK) return rc;
    reduce();
    hv_launch_publish_status(v); // pool occupancy for the next call's hv_capacity_gate
    HV_HIP(hipGetLastError());
    v->frame_counter += 1;
    return HV_OK;
}
