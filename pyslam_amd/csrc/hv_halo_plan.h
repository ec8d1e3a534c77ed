// The plan rule of the halo merge (include/hipvol.h "halo merge"), written once: which unit keys are shared and what a rank does
// with each.  The device plan (k_halo_decide in hv_halo.hip, on radix-sorted packed keys) and the host plans (hv_merge_halo_plan /
// _plan_held, through hv_halo_plan_host below) both walk the runs of equal keys with hv_halo_run_rule.
//
// Needs the C++ standard library only: a host program includes this header without HIP (tools/host_check/halo_plan_check.cpp does).
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstring>
#include <vector>

#ifdef __HIPCC__
#define HV_HALO_HD __host__ __device__ inline
#else
#define HV_HALO_HD inline
#endif

// One key's run of m entries, each rank << 1 | held: the dirty entries first, then the holders by ascending rank.  -> is the key
// shared, and *action of `rank` for it: 1 = keeps the unit (the lowest holding rank), 2 = zeroes its copy (a no-op where it has
// none), 0 where the key is not shared.  Shared: some rank lists the key dirty AND two ranks or more hold it - a rank counts as a
// holder once, however often it lists the key.  all_dirty_kept (one rank taking its own dirty units through the collective path,
// force_collectives): every dirty key is shared and kept.
HV_HALO_HD bool hv_halo_run_rule(const int32_t *run, int64_t m, int32_t rank, bool all_dirty_kept, uint8_t *action) {
    bool any_dirty = false;
    int32_t holders = 0, keeper = -1, last_holder = -1;
    for (int64_t j = 0; j < m; ++j) {
        const int32_t r = run[j] >> 1;
        if (!(run[j] & 1)) {
            any_dirty = true;
        } else if (r != last_holder) {
            last_holder = r;
            if (keeper < 0) keeper = r;
            ++holders;
        }
    }
    const bool shared = all_dirty_kept ? any_dirty : any_dirty && holders >= 2;
    *action = !shared ? 0 : all_dirty_kept || keeper == rank ? 1 : 2;
    return shared;
}

// The host plan: the ranks' dirty lists and held lists back to back ([sum counts, 3] int32 each) -> the number of shared keys; the
// first `cap` of them go to shared_keys / action (both may be null) in (x, y, z) order.  EVERY holder but the keeper zeroes - also
// one that did not update the unit in this window: the pack step exports whatever a rank holds, so a holder that kept its copy
// would be counted twice.
inline int64_t hv_halo_plan_host(const int32_t *dirty_keys, const int64_t *dirty_counts, const int32_t *held_keys, const int64_t *held_counts,
                                 int32_t world_size, int32_t rank, int32_t *shared_keys, uint8_t *action, int64_t cap) {
    struct Entry {
        std::array<int32_t, 3> key;
        int32_t val; // rank << 1 | held
    };
    std::vector<Entry> all;
    for (int held = 0; held < 2; ++held) {
        const int32_t *src = held ? held_keys : dirty_keys;
        const int64_t *counts = held ? held_counts : dirty_counts;
        for (int32_t r = 0; r < world_size; ++r)
            for (int64_t i = 0; i < counts[r]; ++i, src += 3) all.push_back({{src[0], src[1], src[2]}, (r << 1) | held});
    }
    // by key, then in the order the run rule takes: dirty before held, ascending rank
    std::sort(all.begin(), all.end(), [](const Entry &a, const Entry &b) {
        if (a.key != b.key) return a.key < b.key;
        return (a.val & 1) != (b.val & 1) ? (a.val & 1) < (b.val & 1) : a.val < b.val;
    });
    std::vector<int32_t> vals(all.size());
    for (size_t i = 0; i < all.size(); ++i) vals[i] = all[i].val;
    int64_t ns = 0;
    for (size_t i = 0, j; i < all.size(); i = j) {
        for (j = i + 1; j < all.size() && all[j].key == all[i].key;) ++j;
        uint8_t act = 0;
        if (!hv_halo_run_rule(vals.data() + i, (int64_t)(j - i), rank, false, &act)) continue;
        if (shared_keys != nullptr && action != nullptr && ns < cap) {
            memcpy(shared_keys + ns * 3, all[i].key.data(), 12);
            action[ns] = act;
        }
        ++ns;
    }
    return ns;
}
