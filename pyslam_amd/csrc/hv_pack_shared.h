// What the two packed formats of include/hipvol.h share ("Packed maps": hv_pack.hip, "Packed grids": hv_grid_pack.hip): sections on
// 64-byte boundaries, a validator that reads a caller's buffer at any alignment, unit / block keys in ascending order with uint64
// record offsets, and the scan behind those offsets.
#pragma once
#include <cstring>

#include "hv_common.h"
#include <rocprim/device/device_scan.hpp>

inline uint64_t pack_align(uint64_t x) { return (x + 63) & ~(uint64_t)63; }

template <typename T>
inline T rd(const void *p) { // (a caller's buffer need not be aligned)
    T x;
    memcpy(&x, p, sizeof(T));
    return x;
}

// the layout the packers write: the sections in the header's order behind it, each on the next 64-byte boundary -> total bytes
inline int64_t pack_place_sections(int n, uint64_t header_bytes, const uint64_t *size, uint64_t *off) {
    uint64_t cur = header_bytes;
    for (int s = 0; s < n; ++s) {
        off[s] = cur;
        cur = pack_align(cur + size[s]);
    }
    return (int64_t)cur;
}

// the section rules of both validators, in this order: every offset 64-byte aligned; every section behind the header and inside the
// buffer with its size; no two sections overlap
inline int pack_check_sections(const char *fn, int n, const char *const *names, const uint64_t *off, const uint64_t *size, uint64_t header_bytes,
                               int64_t bytes) {
    for (int s = 0; s < n; ++s)
        HV_REQUIRE((off[s] & 63) == 0, HV_ERR_INVALID, "%s: section %s offset %llu is not 64-byte aligned", fn, names[s], (unsigned long long)off[s]);
    for (int s = 0; s < n; ++s)
        HV_REQUIRE(off[s] >= header_bytes && off[s] <= (uint64_t)bytes && size[s] <= (uint64_t)bytes - off[s], HV_ERR_INVALID,
                   "%s: section %s (offset %llu, %llu bytes) lies outside the buffer", fn, names[s], (unsigned long long)off[s],
                   (unsigned long long)size[s]);
    for (int a = 0; a < n; ++a)
        for (int b = a + 1; b < n; ++b)
            HV_REQUIRE(size[a] == 0 || size[b] == 0 || off[a] + size[a] <= off[b] || off[b] + size[b] <= off[a], HV_ERR_INVALID,
                       "%s: sections %s and %s overlap", fn, names[a], names[b]);
    return HV_OK;
}

// the rules on the keys and offsets sections (host copies, any alignment), in this order: keys in [-2^20, 2^20); strictly ascending by
// (x, y, z); offsets[0] == 0; offsets non-decreasing; offsets[U] == N.  `what` / `letter` name a unit ("unit", 'U') or a block.
inline int pack_check_keys_offsets(const char *fn, const char *what, char letter, const unsigned char *keys, const unsigned char *offsets, int64_t U,
                                   int64_t N) {
    for (int64_t u = 0; u < U; ++u) {
        const int32_t x = rd<int32_t>(keys + 12 * u), y = rd<int32_t>(keys + 12 * u + 4), z = rd<int32_t>(keys + 12 * u + 8);
        HV_REQUIRE(hv_key_in_range(x, y, z), HV_ERR_INVALID, "%s: key %lld (%d, %d, %d) is out of range [-2^20, 2^20)", fn, (long long)u, x, y, z);
    }
    for (int64_t u = 1; u < U; ++u) {
        bool less = false;
        for (int a = 0; a < 3; ++a) {
            const int32_t p = rd<int32_t>(keys + 12 * (u - 1) + 4 * a), q = rd<int32_t>(keys + 12 * u + 4 * a);
            if (p != q) {
                less = p < q;
                break;
            }
        }
        HV_REQUIRE(less, HV_ERR_INVALID, "%s: keys are not strictly ascending at %s %lld", fn, what, (long long)u);
    }
    HV_REQUIRE(rd<uint64_t>(offsets) == 0, HV_ERR_INVALID, "%s: offsets[0] is %llu, not 0", fn, (unsigned long long)rd<uint64_t>(offsets));
    for (int64_t u = 0; u < U; ++u)
        HV_REQUIRE(rd<uint64_t>(offsets + 8 * (u + 1)) >= rd<uint64_t>(offsets + 8 * u), HV_ERR_INVALID, "%s: offsets decrease at %s %lld", fn, what,
                   (long long)u);
    HV_REQUIRE(rd<uint64_t>(offsets + 8 * U) == (uint64_t)N, HV_ERR_INVALID, "%s: offsets[%c] (%llu) differs from voxels (%lld)", fn, letter,
               (unsigned long long)rd<uint64_t>(offsets + 8 * U), (long long)N);
    return HV_OK;
}

// exclusive sum of n values into out (unsigned long long; `in` any iterator rocPRIM reads), queued on the volume's stream; the temporary
// storage is the volume's sort_tmp
template <typename In>
inline int pack_exclusive_scan(hv_volume *v, In in, unsigned long long *out, size_t n) {
    size_t tmp = 0;
    HV_HIP(rocprim::exclusive_scan(nullptr, tmp, in, out, 0ull, n, rocprim::plus<unsigned long long>(), v->stream));
    const int rc = hv_ensure_buffer(v, &v->sort_tmp, &v->sort_tmp_bytes, tmp);
    if (rc != HV_OK) return rc;
    tmp = v->sort_tmp_bytes;
    HV_HIP(rocprim::exclusive_scan(v->sort_tmp, tmp, in, out, 0ull, n, rocprim::plus<unsigned long long>(), v->stream));
    return HV_OK;
}

// ---- what the two unpacks share ----
// A packed buffer in DEVICE memory, first step: its header to the host (on the volume's stream: a caller orders the buffer's producers
// against that stream).  Waits for the copy.
inline int unpack_fetch_header(hv_volume *v, const void *d_src, unsigned char *header, size_t header_bytes) {
    HV_HIP(hipMemcpyAsync(header, d_src, header_bytes, hipMemcpyDeviceToHost, v->stream));
    HV_HIP(hipStreamSynchronize(v->stream));
    return HV_OK;
}
// ... second step, once the header rules hold: the metadata sections which[0 .. n) (never the records) to the host, meta[i] holding at
// least 8 readable bytes.  Waits for the copies.
inline int unpack_fetch_sections(hv_volume *v, const void *d_src, const uint64_t *off, const uint64_t *size, const int *which, int n,
                                 std::vector<unsigned char> *meta) {
    for (int i = 0; i < n; ++i) {
        const uint64_t bytes = size[which[i]];
        meta[i].resize((size_t)(bytes > 8 ? bytes : 8));
        if (bytes > 0) HV_HIP(hipMemcpyAsync(meta[i].data(), (const char *)d_src + off[which[i]], (size_t)bytes, hipMemcpyDeviceToHost, v->stream));
    }
    HV_HIP(hipStreamSynchronize(v->stream));
    return HV_OK;
}
// Claim the n keys [n,3] (device memory) of a validated buffer and verify the claims: a pool that is too small grows before anything is
// written, or the claim pass is rolled back, the volume is what it was and the call fails with HV_ERR_CAPACITY.  What the capacity gate
// has learnt about the growth per integrate call is kept: an unpack says nothing about that.
inline int unpack_claim_keys(hv_volume *v, const int32_t *d_keys, int64_t n) {
    const int64_t max_new = v->max_new_per_call;
    const double avg_new = v->avg_new_per_call;
    const int rc = hv_claim_keys(v, d_keys, n);
    v->max_new_per_call = max_new;
    v->avg_new_per_call = avg_new;
    return rc;
}
// After the scatter and its publishing kernel have been waited for: the stream is idle and the volume holds exactly n units / blocks -
// the gate knows the occupancy exactly, as after a growth.
inline void unpack_occupancy_exact(hv_volume *v, int64_t n) {
    v->known_blocks = n;
    v->status_seq_seen = v->status_seq_issued;
    v->status_exact = true;
}

// Drain + key order of a pack: *U = units / blocks held; order[r] = pool index of the r-th key, keys = [U,3] in that order (host).
inline int pack_key_order(hv_volume *v, const char *fn, int64_t *U, std::vector<int32_t> &order, std::vector<int32_t> &keys) {
    int rc = hv_tsdf_drain(v, fn, true, U);
    if (rc != HV_OK || *U == 0) return rc;
    return hv_tsdf_key_order(v, *U, order, &keys);
}
