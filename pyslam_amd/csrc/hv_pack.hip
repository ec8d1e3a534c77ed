// libpyslam_hipvol.so - packed TSDF maps (include/hipvol.h "Packed maps"): a compact, bit-exact form of a map for files, other
// processes and other GPUs.  A unit travels as a 4096-bit mask of its stored voxels (any of the five words non-zero) and five
// contiguous record streams, instead of its 80 KiB.
//
//   pack    k_pack_mask (one workgroup per unit, in key order: the five planes in word order, a wave's ballot = two mask words)
//           -> rocPRIM exclusive scan of the counts -> k_pack_emit (rank of a stored voxel = popcount of the mask bits below it)
//   unpack  hv_tsdf_packed_check on the host (the whole buffer, or the header + the three metadata sections of a device buffer)
//           -> claim (k_tsdf_import_claim, verified) -> k_unpack_scatter (all 4096 voxels of all five planes of every unit)
//
// The validator is the only way into the unpack kernels: they index the record streams with offsets[u] + rank, and rank < the
// unit's count = popcount(masks[u]) is what the validator established, so every index lies inside [0, N).
#include <algorithm>
#include <cstring>
#include <vector>

#include "hv_common.h"
#include "hv_pack_shared.h"

namespace {

constexpr int HV_PACK_SECTIONS = 8;
constexpr int HV_PACK_MASK_WORDS = HV_TSDF_RRR / 32; // 128
const char *const HV_PACK_SECTION_NAMES[HV_PACK_SECTIONS] = {"keys", "offsets", "masks", "tsdf", "weight", "sum_r", "sum_g", "sum_b"};
const char HV_PACK_MAGIC[8] = {'H', 'V', 'T', 'S', 'D', 'F', 'P', 'K'};

void pack_section_sizes(int64_t U, int64_t N, uint64_t size[HV_PACK_SECTIONS]) {
    size[0] = 12ull * (uint64_t)U;
    size[1] = 8ull * (uint64_t)(U + 1);
    size[2] = 4ull * HV_PACK_MASK_WORDS * (uint64_t)U;
    for (int s = 3; s < HV_PACK_SECTIONS; ++s) size[s] = 4ull * (uint64_t)N;
}

struct PackLayout {
    uint64_t off[HV_PACK_SECTIONS], size[HV_PACK_SECTIONS];
    int64_t total;
};
// the layout hv_tsdf_pack writes: the sections in the header's order, each on the next 64-byte boundary
PackLayout pack_layout(int64_t U, int64_t N) {
    PackLayout L;
    pack_section_sizes(U, N, L.size);
    L.total = pack_place_sections(HV_PACK_SECTIONS, HV_PACK_HEADER_BYTES, L.size, L.off);
    return L;
}

struct PackHeader {
    double voxel_length, sdf_trunc;
    int64_t U, N, total;
    uint64_t off[HV_PACK_SECTIONS], size[HV_PACK_SECTIONS];
};

// the rules that need the header alone (h: HV_PACK_HEADER_BYTES readable bytes; bytes: the size of the whole buffer)
int pack_check_header(const unsigned char *h, int64_t bytes, PackHeader *H, hv_packed_header *out) {
    HV_REQUIRE(memcmp(h, HV_PACK_MAGIC, 8) == 0, HV_ERR_INVALID, "hv_tsdf_packed_check: bad magic (not a packed TSDF map)");
    const uint32_t version = rd<uint32_t>(h + 8), header_bytes = rd<uint32_t>(h + 12);
    HV_REQUIRE(version == HV_PACK_VERSION, HV_ERR_INVALID, "hv_tsdf_packed_check: unsupported version %u (this library reads version %d)", version,
               HV_PACK_VERSION);
    HV_REQUIRE(header_bytes == HV_PACK_HEADER_BYTES, HV_ERR_INVALID, "hv_tsdf_packed_check: header_bytes is %u, not %d", header_bytes,
               HV_PACK_HEADER_BYTES);
    const int32_t resolution = rd<int32_t>(h + 32);
    HV_REQUIRE(resolution == HV_TSDF_R, HV_ERR_INVALID, "hv_tsdf_packed_check: resolution is %d, not %d", resolution, HV_TSDF_R);
    H->voxel_length = rd<double>(h + 16);
    H->sdf_trunc = rd<double>(h + 24);
    H->U = rd<int64_t>(h + 40);
    H->N = rd<int64_t>(h + 48);
    H->total = rd<int64_t>(h + 56);
    HV_REQUIRE(H->U >= 0 && H->N >= 0, HV_ERR_INVALID, "hv_tsdf_packed_check: negative units (%lld) or voxels (%lld)", (long long)H->U,
               (long long)H->N);
    HV_REQUIRE(H->U <= bytes / 12 && H->N <= bytes / 4, HV_ERR_INVALID,
               "hv_tsdf_packed_check: units (%lld) or voxels (%lld) exceed what a buffer of %lld bytes could hold", (long long)H->U, (long long)H->N,
               (long long)bytes);
    HV_REQUIRE(H->total == bytes, HV_ERR_INVALID, "hv_tsdf_packed_check: total_bytes (%lld) differs from the buffer's size (%lld)",
               (long long)H->total, (long long)bytes);
    pack_section_sizes(H->U, H->N, H->size);
    for (int s = 0; s < HV_PACK_SECTIONS; ++s) H->off[s] = rd<uint64_t>(h + 64 + 8 * s);
    const int rc = pack_check_sections("hv_tsdf_packed_check", HV_PACK_SECTIONS, HV_PACK_SECTION_NAMES, H->off, H->size, HV_PACK_HEADER_BYTES, bytes);
    if (rc != HV_OK) return rc;
    if (out != nullptr) {
        out->voxel_length = H->voxel_length;
        out->sdf_trunc = H->sdf_trunc;
        out->resolution = resolution;
        out->version = (int32_t)version;
        out->units = H->U;
        out->voxels = H->N;
        out->bytes = H->total;
    }
    return HV_OK;
}

// the rules on the three metadata sections (host copies, any alignment)
int pack_check_meta(const unsigned char *keys, const unsigned char *offsets, const unsigned char *masks, int64_t U, int64_t N) {
    const int rc = pack_check_keys_offsets("hv_tsdf_packed_check", "unit", 'U', keys, offsets, U, N);
    if (rc != HV_OK) return rc;
    for (int64_t u = 0; u < U; ++u) {
        int pop = 0;
        for (int w = 0; w < HV_PACK_MASK_WORDS; ++w) pop += __builtin_popcount(rd<uint32_t>(masks + 4 * (HV_PACK_MASK_WORDS * u + w)));
        const uint64_t count = rd<uint64_t>(offsets + 8 * (u + 1)) - rd<uint64_t>(offsets + 8 * u);
        HV_REQUIRE((uint64_t)pop == count, HV_ERR_INVALID, "hv_tsdf_packed_check: unit %lld: mask popcount %d differs from its record count %llu",
                   (long long)u, pop, (unsigned long long)count);
    }
    return HV_OK;
}

// ---- kernels -----------------------------------------------------------------------------------------------------------------
// A unit's mask words and the exclusive prefix of their popcounts into LDS (all 256 threads call; ends with a barrier).
__device__ __forceinline__ void pack_load_masks(const uint32_t *__restrict__ masks, uint32_t *s_mask, uint32_t *s_pre, uint32_t *s_tot) {
    const int tid = (int)threadIdx.x, lane = hv_lane_id();
    uint32_t m = 0;
    if (tid < HV_PACK_MASK_WORDS) {
        m = masks[tid];
        s_mask[tid] = m;
    }
    const uint32_t c = (uint32_t)__popc(m);
    uint32_t inc = c;
#pragma unroll
    for (int o = 1; o < HV_WAVE; o <<= 1) {
        const uint32_t t = __shfl_up(inc, o, HV_WAVE);
        if (lane >= o) inc += t;
    }
    if (tid == HV_WAVE - 1) *s_tot = inc;
    __syncthreads();
    if (tid < HV_PACK_MASK_WORDS) s_pre[tid] = inc - c + (tid >= HV_WAVE ? *s_tot : 0u);
    __syncthreads();
}

// pool unit order[u] -> masks[u][128], counts[u]: voxel word k is stored when any of its five words is non-zero
__global__ __launch_bounds__(256) void k_pack_mask(const char *__restrict__ pool, const int32_t *__restrict__ order, uint32_t *__restrict__ masks,
                                                    unsigned long long *__restrict__ counts) {
    const int64_t u = blockIdx.x;
    const uint32_t *unit = (const uint32_t *)(pool + (size_t)order[u] * HV_TSDF_UNIT_BYTES);
    const int tid = (int)threadIdx.x, lane = hv_lane_id(), wave = tid >> 6;
    __shared__ uint32_t s_cnt[4];
    uint32_t cnt = 0;
#pragma unroll 4
    for (int i = 0; i < HV_TSDF_RRR / 256; ++i) {
        const int k = i * 256 + tid;
        const uint32_t any = unit[k] | unit[k + HV_TSDF_RRR] | unit[k + 2 * HV_TSDF_RRR] | unit[k + 3 * HV_TSDF_RRR] | unit[k + 4 * HV_TSDF_RRR];
        const unsigned long long m = __ballot(any != 0u);
        if (lane == 0) { // words k .. k + 63 of the unit = mask words k >> 5 and (k >> 5) + 1
            *(uint2 *)(masks + u * HV_PACK_MASK_WORDS + (k >> 5)) = make_uint2((uint32_t)m, (uint32_t)(m >> 32));
            cnt += (uint32_t)__popcll(m);
        }
    }
    if (lane == 0) s_cnt[wave] = cnt;
    __syncthreads();
    if (tid == 0) counts[u] = (unsigned long long)(s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3]);
}

// the stored voxels of pool unit order[u] -> records [offsets[u], offsets[u + 1]) of the five streams, by ascending word
__global__ __launch_bounds__(256) void k_pack_emit(const char *__restrict__ pool, const int32_t *__restrict__ order, const uint32_t *__restrict__ masks,
                                                    const unsigned long long *__restrict__ offsets, uint32_t *__restrict__ out_t,
                                                    uint32_t *__restrict__ out_w, uint32_t *__restrict__ out_r, uint32_t *__restrict__ out_g,
                                                    uint32_t *__restrict__ out_b) {
    __shared__ uint32_t s_mask[HV_PACK_MASK_WORDS], s_pre[HV_PACK_MASK_WORDS], s_tot;
    const int64_t u = blockIdx.x;
    pack_load_masks(masks + u * HV_PACK_MASK_WORDS, s_mask, s_pre, &s_tot);
    const uint32_t *unit = (const uint32_t *)(pool + (size_t)order[u] * HV_TSDF_UNIT_BYTES);
    const unsigned long long base = offsets[u];
    const int tid = (int)threadIdx.x;
#pragma unroll 4
    for (int i = 0; i < HV_TSDF_RRR / 256; ++i) {
        const int k = i * 256 + tid;
        const uint32_t m = s_mask[k >> 5], bit = 1u << (k & 31);
        if (m & bit) {
            const unsigned long long o = base + s_pre[k >> 5] + (uint32_t)__popc(m & (bit - 1u));
            out_t[o] = unit[k];
            out_w[o] = unit[k + HV_TSDF_RRR];
            out_r[o] = unit[k + 2 * HV_TSDF_RRR];
            out_g[o] = unit[k + 3 * HV_TSDF_RRR];
            out_b[o] = unit[k + 4 * HV_TSDF_RRR];
        }
    }
}

// unit u of a validated packed map -> its claimed pool unit: all 4096 voxels of all five planes (the record where the bit is set,
// zero where it is not), and the unit's stamp.  n_records bounds every record index once more (the validator already did).
__global__ __launch_bounds__(256) void k_unpack_scatter(HvTable table, char *__restrict__ pool, int32_t *__restrict__ stamp, int32_t frame_id,
                                                         const int32_t *__restrict__ keys, const unsigned long long *__restrict__ offsets,
                                                         const uint32_t *__restrict__ masks, unsigned long long n_records,
                                                         const uint32_t *__restrict__ in_t, const uint32_t *__restrict__ in_w,
                                                         const uint32_t *__restrict__ in_r, const uint32_t *__restrict__ in_g,
                                                         const uint32_t *__restrict__ in_b) {
    __shared__ uint32_t s_mask[HV_PACK_MASK_WORDS], s_pre[HV_PACK_MASK_WORDS], s_tot;
    const int64_t u = blockIdx.x;
    const int32_t kx = keys[u * 3], ky = keys[u * 3 + 1], kz = keys[u * 3 + 2];
    if (!hv_key_in_range(kx, ky, kz)) return;
    const int32_t slot = hv_table_find(table, hv_pack_key(kx, ky, kz));
    const int32_t idx = slot >= 0 ? table.vals[slot] : -1;
    if (idx < 0 || idx >= table.max_blocks) return; // (uniform over the workgroup; the claims were verified, so it does not happen)
    pack_load_masks(masks + u * HV_PACK_MASK_WORDS, s_mask, s_pre, &s_tot);
    uint32_t *unit = (uint32_t *)(pool + (size_t)idx * HV_TSDF_UNIT_BYTES);
    const unsigned long long base = offsets[u];
    const int tid = (int)threadIdx.x;
    if (tid == 0) stamp[slot] = frame_id;
#pragma unroll 4
    for (int i = 0; i < HV_TSDF_RRR / 256; ++i) {
        const int k = i * 256 + tid;
        const uint32_t m = s_mask[k >> 5], bit = 1u << (k & 31);
        const unsigned long long o = base + s_pre[k >> 5] + (uint32_t)__popc(m & (bit - 1u));
        uint32_t t = 0u, w = 0u, r = 0u, g = 0u, b = 0u;
        if ((m & bit) && o < n_records) {
            t = in_t[o];
            w = in_w[o];
            r = in_r[o];
            g = in_g[o];
            b = in_b[o];
        }
        unit[k] = t;
        unit[k + HV_TSDF_RRR] = w;
        unit[k + 2 * HV_TSDF_RRR] = r;
        unit[k + 3 * HV_TSDF_RRR] = g;
        unit[k + 4 * HV_TSDF_RRR] = b;
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
// device scratch of one pack call, released when it goes out of scope
struct PackScratch {
    HvScratch device; // the masks / counts block, and the assembled map of a host destination
    int32_t *order = nullptr;
    uint32_t *masks = nullptr;
    unsigned long long *counts = nullptr, *offsets = nullptr;
    std::vector<int32_t> keys; // [U,3] in key order (host)
    int64_t U = 0, N = 0;
};

// The first two steps of a pack: key order (hv_tsdf_key_order), masks + counts, scan.  Reads the volume only; touches
// none of its output buffers (the cached extraction results live there).  Waits for the GPU.
int pack_prepare(hv_volume *v, const char *fn, PackScratch &S) {
    int rc = hv_tsdf_require_whole_map(v, fn, "the volume");
    if (rc != HV_OK) return rc;
    int64_t U = 0;
    std::vector<int32_t> order;
    rc = pack_key_order(v, fn, &U, order, S.keys);
    if (rc != HV_OK) return rc;
    S.U = U;
    S.N = 0;
    if (U == 0) return HV_OK;
    // [order U i32][masks U*128 u32][counts U+1 u64][offsets U+1 u64], each part on a 256-byte boundary
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t b_order = up(sizeof(int32_t) * (size_t)U), b_masks = up(sizeof(uint32_t) * HV_PACK_MASK_WORDS * (size_t)U),
                 b_cnt = up(sizeof(uint64_t) * (size_t)(U + 1));
    char *mem = nullptr;
    HV_HIP(S.device.get(&mem, b_order + b_masks + 2 * b_cnt));
    S.order = (int32_t *)mem;
    S.masks = (uint32_t *)(mem + b_order);
    S.counts = (unsigned long long *)(mem + b_order + b_masks);
    S.offsets = (unsigned long long *)(mem + b_order + b_masks + b_cnt);
    HV_HIP(hipMemcpyAsync(S.order, order.data(), sizeof(int32_t) * (size_t)U, hipMemcpyHostToDevice, v->stream));
    HV_HIP(hipMemsetAsync(S.counts + U, 0, sizeof(uint64_t), v->stream)); // the scan's extra element: its output there is N
    hipLaunchKernelGGL(k_pack_mask, dim3((unsigned)U), dim3(256), 0, v->stream, (const char *)v->pool, (const int32_t *)S.order, S.masks, S.counts);
    HV_HIP(hipGetLastError());
    rc = pack_exclusive_scan(v, S.counts, S.offsets, (size_t)(U + 1));
    if (rc != HV_OK) return rc;
    unsigned long long n = 0;
    HV_HIP(hipMemcpyAsync(&n, S.offsets + U, sizeof(n), hipMemcpyDeviceToHost, v->stream));
    HV_HIP(hipStreamSynchronize(v->stream));
    S.N = (int64_t)n;
    return HV_OK;
}

} // namespace

extern "C" {

int hv_tsdf_packed_check(const void *host_src, int64_t bytes, hv_packed_header *out) {
    HV_REQUIRE(host_src != nullptr, HV_ERR_INVALID, "hv_tsdf_packed_check: null buffer");
    HV_REQUIRE(bytes >= HV_PACK_HEADER_BYTES, HV_ERR_INVALID, "hv_tsdf_packed_check: %lld bytes are fewer than the %d-byte header", (long long)bytes,
               HV_PACK_HEADER_BYTES);
    const unsigned char *p = (const unsigned char *)host_src;
    PackHeader H;
    const int rc = pack_check_header(p, bytes, &H, out);
    if (rc != HV_OK) return rc;
    return pack_check_meta(p + H.off[0], p + H.off[1], p + H.off[2], H.U, H.N);
}

int hv_tsdf_pack_size(hv_volume *v, hv_pack_info *info) {
    HV_REQUIRE(v != nullptr && info != nullptr, HV_ERR_INVALID, "hv_tsdf_pack_size: null argument");
    PackScratch S;
    const int rc = pack_prepare(v, "hv_tsdf_pack_size", S);
    if (rc != HV_OK) return rc;
    *info = hv_pack_info{S.U, S.N, pack_layout(S.U, S.N).total};
    return HV_OK;
}

int hv_tsdf_pack(hv_volume *v, void *dst, int64_t cap, int32_t loc, hv_pack_info *info) {
    HV_REQUIRE(v != nullptr && (dst != nullptr || cap <= 0), HV_ERR_INVALID, "hv_tsdf_pack: null argument");
    HV_REQUIRE(loc == HV_HOST || loc == HV_DEVICE, HV_ERR_INVALID, "hv_tsdf_pack: loc must be HV_HOST or HV_DEVICE");
    PackScratch S;
    int rc = pack_prepare(v, "hv_tsdf_pack", S);
    if (rc != HV_OK) return rc;
    const PackLayout L = pack_layout(S.U, S.N);
    if (info != nullptr) *info = hv_pack_info{S.U, S.N, L.total};
    HV_REQUIRE(cap >= L.total, HV_ERR_CAPACITY, "hv_tsdf_pack: the destination holds %lld bytes, the packed map needs %lld", (long long)cap,
               (long long)L.total);
    unsigned char header[HV_PACK_HEADER_BYTES];
    memset(header, 0, sizeof(header));
    memcpy(header, HV_PACK_MAGIC, 8);
    const uint32_t version = HV_PACK_VERSION, header_bytes = HV_PACK_HEADER_BYTES;
    const int32_t resolution = HV_TSDF_R;
    memcpy(header + 8, &version, 4);
    memcpy(header + 12, &header_bytes, 4);
    memcpy(header + 16, &v->cfg.voxel_size, 8);
    memcpy(header + 24, &v->cfg.sdf_trunc, 8);
    memcpy(header + 32, &resolution, 4);
    memcpy(header + 40, &S.U, 8);
    memcpy(header + 48, &S.N, 8);
    memcpy(header + 56, &L.total, 8);
    memcpy(header + 64, L.off, 8 * HV_PACK_SECTIONS);

    char *tmp = nullptr; // a host destination is assembled in device memory and crosses PCIe once
    if (loc == HV_HOST) HV_HIP(S.device.get(&tmp, (size_t)L.total));
    char *d = loc == HV_HOST ? tmp : (char *)dst;
    hipStream_t s = v->stream;
    hipError_t e = hipMemcpyAsync(d, header, sizeof(header), hipMemcpyHostToDevice, s);
    if (e == hipSuccess && S.U > 0) e = hipMemcpyAsync(d + L.off[0], S.keys.data(), L.size[0], hipMemcpyHostToDevice, s);
    if (e == hipSuccess && S.U > 0) e = hipMemcpyAsync(d + L.off[1], S.offsets, L.size[1], hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess && S.U == 0) e = hipMemsetAsync(d + L.off[1], 0, L.size[1], s); // offsets[0] = 0 = N
    if (e == hipSuccess && S.U > 0) e = hipMemcpyAsync(d + L.off[2], S.masks, L.size[2], hipMemcpyDeviceToDevice, s);
    for (int i = 0; i < HV_PACK_SECTIONS && e == hipSuccess; ++i) { // the padding behind every section
        const uint64_t end = L.off[i] + L.size[i], next = i + 1 < HV_PACK_SECTIONS ? L.off[i + 1] : (uint64_t)L.total;
        if (next > end) e = hipMemsetAsync(d + end, 0, (size_t)(next - end), s);
    }
    if (e == hipSuccess && S.N > 0) {
        hipLaunchKernelGGL(k_pack_emit, dim3((unsigned)S.U), dim3(256), 0, s, (const char *)v->pool, (const int32_t *)S.order, (const uint32_t *)S.masks,
                           (const unsigned long long *)S.offsets, (uint32_t *)(d + L.off[3]), (uint32_t *)(d + L.off[4]), (uint32_t *)(d + L.off[5]),
                           (uint32_t *)(d + L.off[6]), (uint32_t *)(d + L.off[7]));
        e = hipGetLastError();
    }
    if (e == hipSuccess && loc == HV_HOST) e = hipMemcpyAsync(dst, d, (size_t)L.total, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        hv_set_error("hv_tsdf_pack: writing the packed map failed: %s", hipGetErrorString(e));
        return HV_ERR_DEVICE;
    }
    return HV_OK;
}

int hv_tsdf_unpack(hv_volume *v, const void *src, int64_t bytes, int32_t loc, hv_pack_info *info) {
    HV_REQUIRE(v != nullptr && src != nullptr, HV_ERR_INVALID, "hv_tsdf_unpack: null argument");
    HV_REQUIRE(loc == HV_HOST || loc == HV_DEVICE, HV_ERR_INVALID, "hv_tsdf_unpack: loc must be HV_HOST or HV_DEVICE");
    int rc = hv_tsdf_require_whole_map(v, "hv_tsdf_unpack", "the volume");
    if (rc != HV_OK) return rc;
    HV_REQUIRE(bytes >= HV_PACK_HEADER_BYTES, HV_ERR_INVALID, "hv_tsdf_packed_check: %lld bytes are fewer than the %d-byte header", (long long)bytes,
               HV_PACK_HEADER_BYTES);
    int64_t used = 0;
    rc = hv_tsdf_drain(v, "hv_tsdf_unpack", true, &used);
    if (rc != HV_OK) return rc;
    // nothing reaches a kernel before the validator has passed it: a host buffer as it lies, of a device buffer the header and then
    // the three metadata sections (the records are only ever indexed through them)
    PackHeader H;
    if (loc == HV_HOST) {
        rc = hv_tsdf_packed_check(src, bytes, nullptr);
        if (rc != HV_OK) return rc;
        rc = pack_check_header((const unsigned char *)src, bytes, &H, nullptr);
        if (rc != HV_OK) return rc;
    } else {
        unsigned char header[HV_PACK_HEADER_BYTES];
        rc = unpack_fetch_header(v, src, header, sizeof(header));
        if (rc != HV_OK) return rc;
        rc = pack_check_header(header, bytes, &H, nullptr);
        if (rc != HV_OK) return rc;
        const int which[3] = {0, 1, 2};
        std::vector<unsigned char> meta[3];
        rc = unpack_fetch_sections(v, src, H.off, H.size, which, 3, meta);
        if (rc != HV_OK) return rc;
        rc = pack_check_meta(meta[0].data(), meta[1].data(), meta[2].data(), H.U, H.N);
        if (rc != HV_OK) return rc;
    }
    HV_REQUIRE(memcmp(&H.voxel_length, &v->cfg.voxel_size, 8) == 0 && memcmp(&H.sdf_trunc, &v->cfg.sdf_trunc, 8) == 0, HV_ERR_INVALID,
               "hv_tsdf_unpack: the packed map has voxel_length %.17g and sdf_trunc %.17g, the volume %.17g and %.17g (they must be bitwise equal)",
               H.voxel_length, H.sdf_trunc, v->cfg.voxel_size, v->cfg.sdf_trunc);
    HV_REQUIRE(used == 0, HV_ERR_INVALID,
               "hv_tsdf_unpack: the volume holds %lld units; a packed map is unpacked into an EMPTY volume (to merge it into this one, unpack "
               "it into a fresh volume and call hv_tsdf_integrate_volume)",
               (long long)used);
    HV_REQUIRE(H.U < (1ll << 30), HV_ERR_CAPACITY, "hv_tsdf_unpack: %lld units are too many", (long long)H.U);
    if (info != nullptr) *info = hv_pack_info{H.U, H.N, H.total};
    if (H.U == 0) return HV_OK;

    HvScratch S;
    char *tmp = nullptr;
    if (loc == HV_HOST) {
        HV_HIP(S.get(&tmp, (size_t)bytes));
        rc = hv_h2d(v, tmp, src, (size_t)bytes);
        if (rc != HV_OK) return rc;
    }
    const char *d = loc == HV_HOST ? (const char *)tmp : (const char *)src;
    // claim first, and verify (this call waits for the GPU anyway): a pool that is too small grows before a voxel is written, or the
    // claim pass is rolled back and the volume is what it was
    rc = unpack_claim_keys(v, (const int32_t *)(d + H.off[0]), H.U);
    if (rc != HV_OK) return rc;
    v->content_version += 1;
    v->extract_epoch += 1;
    v->frame_counter += 1;
    hipStream_t s = v->stream;
    hv_profile_begin(v);
    hipLaunchKernelGGL(k_unpack_scatter, dim3((unsigned)H.U), dim3(256), 0, s, v->table, (char *)v->pool, v->touched_stamp, v->frame_counter,
                       (const int32_t *)(d + H.off[0]), (const unsigned long long *)(d + H.off[1]), (const uint32_t *)(d + H.off[2]),
                       (unsigned long long)H.N, (const uint32_t *)(d + H.off[3]), (const uint32_t *)(d + H.off[4]), (const uint32_t *)(d + H.off[5]),
                       (const uint32_t *)(d + H.off[6]), (const uint32_t *)(d + H.off[7]));
    hv_profile_end(v, H.U);
    hipError_t e = hipGetLastError();
    // hv_tsdf_touched lists the units of the last integrate: none of this volume's
    if (e == hipSuccess) e = hipMemsetAsync(&v->table.counters[HV_CNT_TOUCH0], 0, HV_CNT_TOUCH_SPAN_BYTES, s);
    v->touch_counters_clean = true;
    v->last_touch_parity = 0;
    hv_launch_publish_status(v); // the unpacked units are part of the published occupancy
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        hv_set_error("hv_tsdf_unpack: the scatter failed: %s (the volume holds the claimed units, possibly unwritten: hv_reset it)", hipGetErrorString(e));
        return HV_ERR_DEVICE;
    }
    unpack_occupancy_exact(v, H.U);
    return HV_OK;
}

} // extern "C"
