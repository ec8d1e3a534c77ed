// libpyslam_hipvol.so - packed block grids (include/hipvol.h "Packed grids"): VoxelBlockGrid and the four semantic grids as one bit-exact,
// sparse buffer.  A block travels as a bs^3-bit mask of its stored voxels and their records back to back; the label pairs beyond a
// record's six inline ones follow in three streams.
//
//   pack    k_grid_mask (one workgroup per block, in key order: a wave's ballot = one mask word; the occupancy bits spare the records of
//           voxels that never took a point) -> scans of the per-block counts -> k_grid_emit (rank of a stored voxel = popcount of the
//           mask bits below it; record_bytes / 16 lanes move one record) -> scan of the extras -> k_grid_emit_pairs (chain walk)
//   unpack  hv_grid_packed_check on the host (the whole buffer, or the header + the four metadata sections of a device buffer)
//           -> k_grid_check_records (label maps: meta against extras, read-only) -> claim (verified) -> k_grid_scatter (all bs^3
//           records and the occupancy words of every block) -> k_grid_chains
//
// The validator and the record pass are the only way into the writing kernels: they index the records with offsets[b] + rank < N, the
// pair streams with the scanned extras < P and the node pool with the scanned node counts < the total the host checked against the
// pool - and bound each index once more.
#include <algorithm>
#include <cstring>
#include <vector>

#include "hv_common.h"
#include "hv_pack_shared.h"
#include "hv_semantic.h"
#include <rocprim/iterator/transform_iterator.hpp>

namespace {

constexpr int HV_GP_SECTIONS = 8;
constexpr int HV_GP_MAX_EXTRA = HV_PROB_MAX - HV_PROB_K; // 248
const char *const HV_GP_SECTION_NAMES[HV_GP_SECTIONS] = {"keys", "offsets", "masks", "records", "extras", "extra_obj", "extra_cls", "extra_logp"};
const char HV_GP_MAGIC[8] = {'H', 'V', 'G', 'R', 'I', 'D', 'P', 'K'};
const char *const GP_CHECK = "hv_grid_packed_check";

inline bool gp_mode_ok(int32_t mode) { return mode == HV_MODE_VOXEL_GRID || hv_mode_is_semantic(mode); }
inline int32_t gp_record_bytes(int32_t mode) { return mode == HV_MODE_VOXEL_GRID ? 32 : hv_mode_has_label_maps(mode) ? 128 : 64; }
// the 32-bit words of a record that are content (bit j = word j): everything but the padding and the chain link
inline uint32_t gp_keep_words(int32_t mode) {
    return mode == HV_MODE_VOXEL_GRID ? 0x7fu : mode == HV_MODE_VOXEL_SEMANTIC_GRID ? 0x1fffu : mode == HV_MODE_VOXEL_SEMANTIC_GRID2 ? 0x3fffu : 0x1fffffffu;
}
static_assert(offsetof(HvVoxel, pad) == 28 && offsetof(HvSemVoxel, pad) == 52 && offsetof(HvSem2Voxel, pad) == 56, "record padding moved");
static_assert(offsetof(HvProbVoxel, meta) == 4 && offsetof(HvProbVoxel, next) == 116 && offsetof(HvProbVoxel, pad) == 120, "HvProbVoxel layout moved");

struct GridHeader {
    double voxel_size;
    int32_t mode, bs, record_bytes, next_object_id, nvox, W;
    float depth_threshold, depth_decay_rate;
    int64_t B, N, P, total;
    uint64_t off[HV_GP_SECTIONS], size[HV_GP_SECTIONS];
};

void gp_section_sizes(int64_t B, int64_t N, int64_t P, int W, int32_t record_bytes, bool maps, uint64_t size[HV_GP_SECTIONS]) {
    size[0] = 12ull * (uint64_t)B;
    size[1] = 8ull * (uint64_t)(B + 1);
    size[2] = 8ull * (uint64_t)W * (uint64_t)B;
    size[3] = (uint64_t)record_bytes * (uint64_t)N;
    size[4] = maps ? (uint64_t)N : 0;
    size[5] = size[6] = size[7] = 4ull * (uint64_t)P;
}

// the rules that need the header alone (h: HV_GRID_PACK_HEADER_BYTES readable bytes; bytes: the size of the whole buffer)
int gp_check_header(const unsigned char *h, int64_t bytes, GridHeader *H, hv_grid_packed_header *out) {
    HV_REQUIRE(memcmp(h, HV_GP_MAGIC, 8) == 0, HV_ERR_INVALID, "%s: bad magic (not a packed grid)", GP_CHECK);
    const uint32_t version = rd<uint32_t>(h + 8), header_bytes = rd<uint32_t>(h + 12);
    HV_REQUIRE(version == HV_GRID_PACK_VERSION, HV_ERR_INVALID, "%s: unsupported version %u (this library reads version %d)", GP_CHECK, version,
               HV_GRID_PACK_VERSION);
    HV_REQUIRE(header_bytes == HV_GRID_PACK_HEADER_BYTES, HV_ERR_INVALID, "%s: header_bytes is %u, not %d", GP_CHECK, header_bytes,
               HV_GRID_PACK_HEADER_BYTES);
    H->voxel_size = rd<double>(h + 16);
    H->mode = rd<int32_t>(h + 24);
    H->bs = rd<int32_t>(h + 28);
    H->record_bytes = rd<int32_t>(h + 32);
    H->next_object_id = rd<int32_t>(h + 36);
    H->depth_threshold = rd<float>(h + 40);
    H->depth_decay_rate = rd<float>(h + 44);
    H->B = rd<int64_t>(h + 48);
    H->N = rd<int64_t>(h + 56);
    H->P = rd<int64_t>(h + 64);
    H->total = rd<int64_t>(h + 72);
    HV_REQUIRE(gp_mode_ok(H->mode), HV_ERR_INVALID, "%s: mode is %d, not one of the five grid modes", GP_CHECK, H->mode);
    HV_REQUIRE(H->bs >= 1 && H->bs <= 16, HV_ERR_INVALID, "%s: block_size is %d, not in [1,16]", GP_CHECK, H->bs);
    HV_REQUIRE(H->record_bytes == gp_record_bytes(H->mode), HV_ERR_INVALID, "%s: record_bytes is %d, mode %d has %d", GP_CHECK, H->record_bytes,
               H->mode, gp_record_bytes(H->mode));
    H->nvox = H->bs * H->bs * H->bs;
    H->W = (H->nvox + 63) / 64;
    const bool maps = hv_mode_has_label_maps(H->mode);
    HV_REQUIRE(H->B >= 0 && H->N >= 0 && H->P >= 0, HV_ERR_INVALID, "%s: negative blocks (%lld), voxels (%lld) or extra_pairs (%lld)", GP_CHECK,
               (long long)H->B, (long long)H->N, (long long)H->P);
    HV_REQUIRE(maps || H->P == 0, HV_ERR_INVALID, "%s: extra_pairs is %lld in mode %d, which has no label maps", GP_CHECK, (long long)H->P, H->mode);
    HV_REQUIRE(H->B <= bytes / 12 && H->N <= bytes / H->record_bytes && H->P <= bytes / 12, HV_ERR_INVALID,
               "%s: blocks (%lld), voxels (%lld) or extra_pairs (%lld) exceed what a buffer of %lld bytes could hold", GP_CHECK, (long long)H->B,
               (long long)H->N, (long long)H->P, (long long)bytes);
    HV_REQUIRE(H->total == bytes, HV_ERR_INVALID, "%s: total_bytes (%lld) differs from the buffer's size (%lld)", GP_CHECK, (long long)H->total,
               (long long)bytes);
    gp_section_sizes(H->B, H->N, H->P, H->W, H->record_bytes, maps, H->size);
    for (int s = 0; s < HV_GP_SECTIONS; ++s) H->off[s] = rd<uint64_t>(h + 80 + 8 * s);
    const int rc = pack_check_sections(GP_CHECK, HV_GP_SECTIONS, HV_GP_SECTION_NAMES, H->off, H->size, HV_GRID_PACK_HEADER_BYTES, bytes);
    if (rc != HV_OK) return rc;
    if (out != nullptr) {
        *out = hv_grid_packed_header{H->voxel_size, H->mode, H->bs, H->record_bytes, (int32_t)version, H->next_object_id, H->depth_threshold,
                                     H->depth_decay_rate, 0, H->B, H->N, H->P, H->total, 0};
    }
    return HV_OK;
}

// the rules on the four metadata sections (host copies, any alignment); *nodes = sum ceil(extras / HV_PROB_NK)
int gp_check_meta(const GridHeader &H, const unsigned char *keys, const unsigned char *offsets, const unsigned char *masks, const unsigned char *extras,
                  int64_t *nodes) {
    const int rc = pack_check_keys_offsets(GP_CHECK, "block", 'B', keys, offsets, H.B, H.N);
    if (rc != HV_OK) return rc;
    for (int64_t b = 0; b < H.B; ++b) {
        int pop = 0;
        for (int w = 0; w < H.W; ++w) pop += __builtin_popcountll(rd<uint64_t>(masks + 8 * (H.W * b + w)));
        const uint64_t count = rd<uint64_t>(offsets + 8 * (b + 1)) - rd<uint64_t>(offsets + 8 * b);
        HV_REQUIRE((uint64_t)pop == count, HV_ERR_INVALID, "%s: block %lld: mask popcount %d differs from its record count %llu", GP_CHECK, (long long)b,
                   pop, (unsigned long long)count);
    }
    if (H.nvox & 63) {
        const uint64_t high = ~0ull << (H.nvox & 63);
        for (int64_t b = 0; b < H.B; ++b)
            HV_REQUIRE((rd<uint64_t>(masks + 8 * (H.W * b + H.W - 1)) & high) == 0, HV_ERR_INVALID,
                       "%s: block %lld: a mask bit at or above block_size^3 = %d is set", GP_CHECK, (long long)b, H.nvox);
    }
    int64_t pairs = 0, nn = 0;
    if (H.size[4] > 0) {
        for (int64_t i = 0; i < H.N; ++i)
            HV_REQUIRE(extras[i] <= HV_GP_MAX_EXTRA, HV_ERR_INVALID, "%s: extras[%lld] is %d, more than %d", GP_CHECK, (long long)i, (int)extras[i],
                       HV_GP_MAX_EXTRA);
        for (int64_t i = 0; i < H.N; ++i) {
            pairs += extras[i];
            nn += (extras[i] + HV_PROB_NK - 1) / HV_PROB_NK;
        }
    }
    HV_REQUIRE(pairs == H.P, HV_ERR_INVALID, "%s: the sum of extras (%lld) differs from extra_pairs (%lld)", GP_CHECK, (long long)pairs, (long long)H.P);
    if (nodes != nullptr) *nodes = nn;
    return HV_OK;
}

// what a label-map record must say beside its extras entry: 0 fine, 1 the label count disagrees, 2 a cached best index exceeds it
__host__ __device__ inline int gp_record_rule(uint32_t meta, uint32_t extra, bool prob2) {
    const uint32_t n = meta & 0xffu;
    if (n > (uint32_t)HV_PROB_MAX || extra != (n > (uint32_t)HV_PROB_K ? n - HV_PROB_K : 0u)) return 1;
    if (((meta >> 8) & 0xffu) > n || (prob2 && ((meta >> 16) & 0xffu) > n)) return 2;
    return 0;
}

// ---- kernels -----------------------------------------------------------------------------------------------------------------
struct GpPairCount { // extras entry -> the pairs it stands for
    __host__ __device__ unsigned long long operator()(uint8_t e) const { return e; }
};
struct GpNodeCount { // ... -> the overflow nodes they fill
    __host__ __device__ unsigned long long operator()(uint8_t e) const { return (e + HV_PROB_NK - 1) / HV_PROB_NK; }
};

// word j of a record, or zero when it is padding / the chain link
__device__ __forceinline__ uint4 gp_keep(uint4 x, uint32_t keep, int part) {
    const uint32_t kp = keep >> (part * 4);
    x.x = (kp & 1u) ? x.x : 0u;
    x.y = (kp & 2u) ? x.y : 0u;
    x.z = (kp & 4u) ? x.z : 0u;
    x.w = (kp & 8u) ? x.w : 0u;
    return x;
}

// A block's W <= 64 mask words and the exclusive prefix of their popcounts into LDS (all 256 threads call; ends with a barrier).
__device__ __forceinline__ void gp_load_masks(const unsigned long long *__restrict__ masks, int W, unsigned long long *s_mask, uint32_t *s_pre) {
    const int tid = (int)threadIdx.x;
    if (tid < HV_WAVE) { // wave 0, whole
        const unsigned long long m = tid < W ? masks[tid] : 0ull;
        const uint32_t c = (uint32_t)__popcll(m);
        uint32_t inc = c;
#pragma unroll
        for (int o = 1; o < HV_WAVE; o <<= 1) {
            const uint32_t t = __shfl_up(inc, o, HV_WAVE);
            if (tid >= o) inc += t;
        }
        s_mask[tid] = m;
        s_pre[tid] = inc - c;
    }
    __syncthreads();
}

// pool block order[b] -> masks[b][W], counts[b], ecounts[b] (label maps: the block's pairs beyond the inline ones).  A wave takes 64
// voxels at a time; a lane reads its record only when its occupancy bit is set (occ == nullptr: VoxelBlockGrid, every record).
template <int RB>
__global__ __launch_bounds__(256) void k_grid_mask(const char *__restrict__ pool, const int32_t *__restrict__ order,
                                                    const unsigned long long *__restrict__ occ, int nvox, int W, uint32_t keep, bool maps,
                                                    unsigned long long *__restrict__ masks, unsigned long long *__restrict__ counts,
                                                    unsigned long long *__restrict__ ecounts) {
    constexpr int L = RB / 16;
    const int64_t b = blockIdx.x, idx = order[b];
    const uint4 *blk = (const uint4 *)(pool + (size_t)idx * (size_t)nvox * RB);
    const int tid = (int)threadIdx.x, lane = hv_lane_id(), wave = tid >> 6;
    __shared__ uint32_t s_cnt[4], s_ext[4];
    uint32_t cnt = 0, ext = 0;
    for (int w = wave; w < W; w += 4) { // (wave-uniform)
        const int k = w * 64 + lane;
        bool stored = false;
        uint32_t e = 0;
        if (k < nvox && sem_maybe_occupied(occ, idx * nvox + k)) {
            uint32_t any = 0, meta = 0;
#pragma unroll
            for (int q = 0; q < L; ++q) {
                const uint4 x = gp_keep(blk[(size_t)k * L + q], keep, q);
                any |= x.x | x.y | x.z | x.w;
                if (q == 0) meta = x.y;
            }
            stored = any != 0u;
            if (maps && stored) {
                const uint32_t n = min(meta & 0xffu, (uint32_t)HV_PROB_MAX);
                e = n > (uint32_t)HV_PROB_K ? n - HV_PROB_K : 0u;
            }
        }
        const unsigned long long m = __ballot(stored);
        const uint32_t esum = hv_wave_sum(e);
        if (lane == 0) {
            masks[b * W + w] = m;
            cnt += (uint32_t)__popcll(m);
            ext += esum;
        }
    }
    if (lane == 0) {
        s_cnt[wave] = cnt;
        s_ext[wave] = ext;
    }
    __syncthreads();
    if (tid == 0) {
        counts[b] = (unsigned long long)(s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3]);
        if (ecounts != nullptr) ecounts[b] = (unsigned long long)(s_ext[0] + s_ext[1] + s_ext[2] + s_ext[3]);
    }
}

// the stored voxels of pool block order[b] -> records [offsets[b], offsets[b + 1]): RB / 16 lanes move one record in 16-byte pieces, so
// consecutive lanes write consecutive bytes.  Label maps: the extras entry, and the chain link (zeroed in the record) for k_grid_emit_pairs.
template <int RB>
__global__ __launch_bounds__(256) void k_grid_emit(const char *__restrict__ pool, const int32_t *__restrict__ order, int nvox, int W, uint32_t keep,
                                                    bool maps, const unsigned long long *__restrict__ masks,
                                                    const unsigned long long *__restrict__ offsets, uint4 *__restrict__ out_rec,
                                                    uint8_t *__restrict__ out_extras, uint32_t *__restrict__ chain_head) {
    constexpr int L = RB / 16;
    __shared__ unsigned long long s_mask[HV_WAVE];
    __shared__ uint32_t s_pre[HV_WAVE];
    const int64_t b = blockIdx.x;
    gp_load_masks(masks + b * W, W, s_mask, s_pre);
    const uint4 *blk = (const uint4 *)(pool + (size_t)order[b] * (size_t)nvox * RB);
    const unsigned long long base = offsets[b];
    const uint32_t total = s_pre[W - 1] + (uint32_t)__popcll(s_mask[W - 1]);
    for (uint32_t t = threadIdx.x; t < total * L; t += 256) {
        const uint32_t r = t / L;
        const int part = (int)(t % L);
        int lo = 0, hi = W - 1; // the last word whose prefix is <= r holds the r-th stored voxel
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (s_pre[mid] <= r) lo = mid;
            else hi = mid - 1;
        }
        const int k = lo * 64 + sem_select_bit(s_mask[lo], (int)(r - s_pre[lo]));
        const uint4 raw = blk[(size_t)k * L + part];
        out_rec[(base + r) * L + part] = gp_keep(raw, keep, part);
        if (maps) {
            if (part == 0) {
                const uint32_t n = min(raw.y & 0xffu, (uint32_t)HV_PROB_MAX);
                out_extras[base + r] = (uint8_t)(n > (uint32_t)HV_PROB_K ? n - HV_PROB_K : 0u);
            }
            if (part == 7) chain_head[base + r] = raw.y; // word 29
        }
    }
}

// one lane per stored voxel with extras: its chain's pairs, in order, to [pair_off[i], pair_off[i] + extras[i])
__global__ __launch_bounds__(256) void k_grid_emit_pairs(const HvProbNode *__restrict__ nodes, int32_t node_cap, const uint8_t *__restrict__ extras,
                                                          const uint32_t *__restrict__ chain_head, const unsigned long long *__restrict__ pair_off,
                                                          int64_t N, unsigned long long P, int32_t *__restrict__ out_obj,
                                                          int32_t *__restrict__ out_cls, float *__restrict__ out_logp) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const uint32_t e = extras[i];
    if (e == 0u) return;
    const unsigned long long po = pair_off[i];
    uint32_t n = chain_head[i];
    for (uint32_t j = 0; j < e && n != 0u && n <= (uint32_t)node_cap; n = nodes[n - 1].next) {
        const HvProbNode *nd = &nodes[n - 1];
        for (int s = 0; s < HV_PROB_NK && j < e; ++s, ++j) {
            if (po + j >= P) return;
            out_obj[po + j] = nd->obj[s];
            out_cls[po + j] = nd->cls[s];
            out_logp[po + j] = nd->logp[s];
        }
    }
}

// label maps, read-only: the first record (lowest index) whose meta breaks gp_record_rule
__global__ __launch_bounds__(256) void k_grid_check_records(const uint4 *__restrict__ rec, const uint8_t *__restrict__ extras, int64_t N, bool prob2,
                                                             unsigned long long *__restrict__ first_bad) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    if (gp_record_rule(rec[i * 8].y, extras[i], prob2) != 0) atomicMin(first_bad, (unsigned long long)i);
}

// block b of a validated packed grid -> its claimed pool block: all bs^3 records (the packed one where the bit is set, zero where it is
// not; a label-map record gets its chain link from the node scan) and the block's occupancy bits.  n_records bounds every record index
// once more (the validator already did).
template <int RB>
__global__ __launch_bounds__(256) void k_grid_scatter(HvTable table, char *__restrict__ pool, unsigned long long *__restrict__ occ, int nvox, int W,
                                                       uint32_t keep, bool maps, const int32_t *__restrict__ keys,
                                                       const unsigned long long *__restrict__ offsets, const unsigned long long *__restrict__ masks,
                                                       unsigned long long n_records, const uint4 *__restrict__ rec, const uint8_t *__restrict__ extras,
                                                       const unsigned long long *__restrict__ node_off) {
    constexpr int L = RB / 16;
    __shared__ unsigned long long s_mask[HV_WAVE];
    __shared__ uint32_t s_pre[HV_WAVE];
    const int64_t b = blockIdx.x;
    const int32_t kx = keys[b * 3], ky = keys[b * 3 + 1], kz = keys[b * 3 + 2];
    if (!hv_key_in_range(kx, ky, kz)) return;
    const int32_t slot = hv_table_find(table, hv_pack_key(kx, ky, kz));
    const int32_t idx = slot >= 0 ? table.vals[slot] : -1;
    if (idx < 0 || idx >= table.max_blocks) return; // (uniform over the workgroup; the claims were verified, so it does not happen)
    gp_load_masks(masks + b * W, W, s_mask, s_pre);
    uint4 *blk = (uint4 *)(pool + (size_t)idx * (size_t)nvox * RB);
    const unsigned long long base = offsets[b];
    const int tid = (int)threadIdx.x;
    for (int t = tid; t < nvox * L; t += 256) {
        const int k = t / L, part = t % L;
        const unsigned long long m = s_mask[k >> 6], bit = 1ull << (k & 63);
        uint4 x = make_uint4(0u, 0u, 0u, 0u);
        const unsigned long long i = base + s_pre[k >> 6] + (uint32_t)__popcll(m & (bit - 1ull));
        if ((m & bit) && i < n_records) {
            x = gp_keep(rec[i * L + part], keep, part);
            if (maps && part == 7) x.y = extras[i] > 0 ? (uint32_t)node_off[i] + 1u : 0u;
        }
        blk[(size_t)k * L + part] = x;
    }
    if (occ != nullptr && tid < W) {
        const unsigned long long m = s_mask[tid];
        if ((nvox & 63) == 0) {
            occ[(size_t)idx * W + tid] = m;
        } else if (m != 0ull) { // the block's bits straddle words it shares with its neighbours (all zero in the empty target)
            const unsigned long long pos = (unsigned long long)idx * (unsigned long long)nvox + (unsigned long long)tid * 64ull;
            const int sh = (int)(pos & 63ull);
            atomicOr(&occ[pos >> 6], m << sh);
            if (sh != 0 && (m >> (64 - sh)) != 0ull) atomicOr(&occ[(pos >> 6) + 1], m >> (64 - sh));
        }
    }
}

// one lane per stored voxel with extras: nodes [node_off[i], node_off[i] + ceil(extras[i] / NK)) filled in order and linked
__global__ __launch_bounds__(256) void k_grid_chains(HvProbNode *__restrict__ nodes, int32_t node_cap, const uint8_t *__restrict__ extras,
                                                      const unsigned long long *__restrict__ node_off, const unsigned long long *__restrict__ pair_off,
                                                      int64_t N, unsigned long long P, const int32_t *__restrict__ in_obj,
                                                      const int32_t *__restrict__ in_cls, const float *__restrict__ in_logp) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const uint32_t e = extras[i];
    if (e == 0u) return;
    const uint32_t nn = (e + HV_PROB_NK - 1) / HV_PROB_NK;
    const unsigned long long first = node_off[i], po = pair_off[i];
    if (first + nn > (unsigned long long)node_cap || po + e > P) return; // (the host checked both totals)
    for (uint32_t j = 0; j < nn; ++j) {
        HvProbNode *nd = &nodes[first + j];
        for (int s = 0; s < HV_PROB_NK; ++s) {
            const uint32_t p = j * HV_PROB_NK + s;
            const bool has = p < e;
            nd->obj[s] = has ? in_obj[po + p] : 0;
            nd->cls[s] = has ? in_cls[po + p] : 0;
            nd->logp[s] = has ? in_logp[po + p] : 0.0f;
        }
        nd->next = j + 1 < nn ? (uint32_t)(first + j) + 2u : 0u;
        nd->pad = 0u;
    }
}

// the kernel template instantiated for the volume's record size
#define HV_GP_BY_RECORD(rb, ...)                                                                                                           \
    switch (rb) {                                                                                                                          \
    case 32: { constexpr int RB = 32; __VA_ARGS__; } break;                                                                                \
    case 64: { constexpr int RB = 64; __VA_ARGS__; } break;                                                                                \
    default: { constexpr int RB = 128; __VA_ARGS__; } break;                                                                               \
    }

// ---- host side ---------------------------------------------------------------------------------------------------------------
int gp_require_whole_grid(const hv_volume *v, const char *fn) {
    HV_REQUIRE(gp_mode_ok(v->cfg.mode), HV_ERR_MODE, "%s: the volume is not a voxel block grid (TSDF maps: hv_tsdf_pack / hv_tsdf_unpack)", fn);
    HV_REQUIRE(v->owner_world <= 1, HV_ERR_MODE, "%s: the grid is owner-sharded (it holds a part of the map's blocks)", fn);
    return HV_OK;
}

// device scratch of one pack call, released when it goes out of scope
struct GridPackScratch {
    HvScratch device;
    int32_t *order = nullptr;
    unsigned long long *masks = nullptr, *counts = nullptr, *offsets = nullptr, *ecounts = nullptr, *eoffsets = nullptr;
    std::vector<int32_t> keys; // [B,3] in key order (host)
    int64_t B = 0, N = 0, P = 0;
    int nvox = 0, W = 0, record_bytes = 0;
    uint32_t keep = 0;
    bool maps = false;
};

// The first steps of a pack: key order, masks + counts, scans.  Reads the volume only.  Waits for the GPU.
int gp_prepare(hv_volume *v, const char *fn, GridPackScratch &S) {
    int rc = gp_require_whole_grid(v, fn);
    if (rc != HV_OK) return rc;
    S.nvox = v->cfg.block_size * v->cfg.block_size * v->cfg.block_size;
    S.W = (S.nvox + 63) / 64;
    S.record_bytes = gp_record_bytes(v->cfg.mode);
    S.keep = gp_keep_words(v->cfg.mode);
    S.maps = hv_mode_has_label_maps(v->cfg.mode);
    int64_t B = 0;
    std::vector<int32_t> order;
    rc = pack_key_order(v, fn, &B, order, S.keys);
    if (rc != HV_OK) return rc;
    S.B = B;
    if (B == 0) return HV_OK;
    // [order B i32][masks B*W u64][counts, offsets, ecounts, eoffsets B+1 u64 each], each part on a 256-byte boundary
    auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t b_order = up(sizeof(int32_t) * (size_t)B), b_masks = up(8 * (size_t)S.W * (size_t)B), b_cnt = up(8 * (size_t)(B + 1));
    char *mem = nullptr;
    HV_HIP(S.device.get(&mem, b_order + b_masks + 4 * b_cnt));
    S.order = (int32_t *)mem;
    S.masks = (unsigned long long *)(mem + b_order);
    S.counts = (unsigned long long *)(mem + b_order + b_masks);
    S.offsets = (unsigned long long *)(mem + b_order + b_masks + b_cnt);
    S.ecounts = (unsigned long long *)(mem + b_order + b_masks + 2 * b_cnt);
    S.eoffsets = (unsigned long long *)(mem + b_order + b_masks + 3 * b_cnt);
    hipStream_t s = v->stream;
    HV_HIP(hipMemcpyAsync(S.order, order.data(), sizeof(int32_t) * (size_t)B, hipMemcpyHostToDevice, s));
    HV_HIP(hipMemsetAsync(S.counts + B, 0, 8, s)); // the scans' extra element: their output there is N / P
    HV_HIP(hipMemsetAsync(S.ecounts + B, 0, 8, s));
    HV_GP_BY_RECORD(S.record_bytes, hipLaunchKernelGGL(k_grid_mask<RB>, dim3((unsigned)B), dim3(256), 0, s, (const char *)v->pool, (const int32_t *)S.order,
                                                       (const unsigned long long *)v->occ, S.nvox, S.W, S.keep, S.maps, S.masks, S.counts,
                                                       S.maps ? S.ecounts : nullptr));
    HV_HIP(hipGetLastError());
    rc = pack_exclusive_scan(v, S.counts, S.offsets, (size_t)(B + 1));
    if (rc != HV_OK) return rc;
    if (S.maps) {
        rc = pack_exclusive_scan(v, S.ecounts, S.eoffsets, (size_t)(B + 1));
        if (rc != HV_OK) return rc;
    }
    unsigned long long n = 0, p = 0;
    HV_HIP(hipMemcpyAsync(&n, S.offsets + B, 8, hipMemcpyDeviceToHost, s));
    if (S.maps) HV_HIP(hipMemcpyAsync(&p, S.eoffsets + B, 8, hipMemcpyDeviceToHost, s));
    HV_HIP(hipStreamSynchronize(s));
    S.N = (int64_t)n;
    S.P = (int64_t)p;
    return HV_OK;
}

struct GridLayout {
    uint64_t off[HV_GP_SECTIONS], size[HV_GP_SECTIONS];
    int64_t total;
};
GridLayout gp_layout(const GridPackScratch &S) {
    GridLayout L;
    gp_section_sizes(S.B, S.N, S.P, S.W, S.record_bytes, S.maps, L.size);
    L.total = pack_place_sections(HV_GP_SECTIONS, HV_GRID_PACK_HEADER_BYTES, L.size, L.off);
    return L;
}

} // namespace

extern "C" {

int hv_grid_packed_check(const void *host_src, int64_t bytes, hv_grid_packed_header *out) {
    HV_REQUIRE(host_src != nullptr, HV_ERR_INVALID, "%s: null buffer", GP_CHECK);
    HV_REQUIRE(bytes >= HV_GRID_PACK_HEADER_BYTES, HV_ERR_INVALID, "%s: %lld bytes are fewer than the %d-byte header", GP_CHECK, (long long)bytes,
               HV_GRID_PACK_HEADER_BYTES);
    const unsigned char *p = (const unsigned char *)host_src;
    GridHeader H;
    const int rc = gp_check_header(p, bytes, &H, out);
    if (rc != HV_OK) return rc;
    int64_t nodes = 0;
    const int rm = gp_check_meta(H, p + H.off[0], p + H.off[1], p + H.off[2], p + H.off[4], &nodes);
    if (rm == HV_OK && out != nullptr) out->chain_nodes = nodes;
    return rm;
}

int hv_grid_pack_size(hv_volume *v, hv_grid_pack_info *info) {
    HV_REQUIRE(v != nullptr && info != nullptr, HV_ERR_INVALID, "hv_grid_pack_size: null argument");
    GridPackScratch S;
    const int rc = gp_prepare(v, "hv_grid_pack_size", S);
    if (rc != HV_OK) return rc;
    *info = hv_grid_pack_info{S.B, S.N, S.P, gp_layout(S).total};
    return HV_OK;
}

int hv_grid_pack(hv_volume *v, void *dst, int64_t cap, int32_t loc, hv_grid_pack_info *info) {
    HV_REQUIRE(v != nullptr && (dst != nullptr || cap <= 0), HV_ERR_INVALID, "hv_grid_pack: null argument");
    HV_REQUIRE(loc == HV_HOST || loc == HV_DEVICE, HV_ERR_INVALID, "hv_grid_pack: loc must be HV_HOST or HV_DEVICE");
    GridPackScratch S;
    int rc = gp_prepare(v, "hv_grid_pack", S);
    if (rc != HV_OK) return rc;
    const GridLayout L = gp_layout(S);
    if (info != nullptr) *info = hv_grid_pack_info{S.B, S.N, S.P, L.total};
    HV_REQUIRE(cap >= L.total, HV_ERR_CAPACITY, "hv_grid_pack: the destination holds %lld bytes, the packed grid needs %lld", (long long)cap,
               (long long)L.total);
    const int32_t next_id = hv_is_semantic(v) ? hv_peek_next_object_id() : 1; // (reads the counter; waits for the device)
    HV_HIP(hipSetDevice(v->device));
    unsigned char header[HV_GRID_PACK_HEADER_BYTES];
    memset(header, 0, sizeof(header));
    memcpy(header, HV_GP_MAGIC, 8);
    const uint32_t version = HV_GRID_PACK_VERSION, header_bytes = HV_GRID_PACK_HEADER_BYTES;
    const int32_t mode = v->cfg.mode, bs = v->cfg.block_size, rb = S.record_bytes;
    memcpy(header + 8, &version, 4);
    memcpy(header + 12, &header_bytes, 4);
    memcpy(header + 16, &v->cfg.voxel_size, 8);
    memcpy(header + 24, &mode, 4);
    memcpy(header + 28, &bs, 4);
    memcpy(header + 32, &rb, 4);
    memcpy(header + 36, &next_id, 4);
    memcpy(header + 40, &v->sem_depth_threshold, 4);
    memcpy(header + 44, &v->sem_depth_decay_rate, 4);
    memcpy(header + 48, &S.B, 8);
    memcpy(header + 56, &S.N, 8);
    memcpy(header + 64, &S.P, 8);
    memcpy(header + 72, &L.total, 8);
    memcpy(header + 80, L.off, 8 * HV_GP_SECTIONS);

    char *tmp = nullptr; // a host destination is assembled in device memory and crosses PCIe once
    if (loc == HV_HOST) HV_HIP(S.device.get(&tmp, (size_t)L.total));
    char *d = loc == HV_HOST ? tmp : (char *)dst;
    uint32_t *chain_head = nullptr;
    unsigned long long *pair_off = nullptr;
    if (S.maps && S.N > 0) {
        HV_HIP(S.device.get(&chain_head, (size_t)S.N));
        HV_HIP(S.device.get(&pair_off, (size_t)S.N));
    }
    hipStream_t s = v->stream;
    hipError_t e = hipMemcpyAsync(d, header, sizeof(header), hipMemcpyHostToDevice, s);
    if (e == hipSuccess && S.B > 0) e = hipMemcpyAsync(d + L.off[0], S.keys.data(), L.size[0], hipMemcpyHostToDevice, s);
    if (e == hipSuccess && S.B > 0) e = hipMemcpyAsync(d + L.off[1], S.offsets, L.size[1], hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess && S.B == 0) e = hipMemsetAsync(d + L.off[1], 0, L.size[1], s); // offsets[0] = 0 = N
    if (e == hipSuccess && S.B > 0) e = hipMemcpyAsync(d + L.off[2], S.masks, L.size[2], hipMemcpyDeviceToDevice, s);
    for (int i = 0; i < HV_GP_SECTIONS && e == hipSuccess; ++i) { // the padding behind every section
        const uint64_t end = L.off[i] + L.size[i], next = i + 1 < HV_GP_SECTIONS ? L.off[i + 1] : (uint64_t)L.total;
        if (next > end) e = hipMemsetAsync(d + end, 0, (size_t)(next - end), s);
    }
    if (e == hipSuccess && S.N > 0) {
        HV_GP_BY_RECORD(S.record_bytes, hipLaunchKernelGGL(k_grid_emit<RB>, dim3((unsigned)S.B), dim3(256), 0, s, (const char *)v->pool,
                                                           (const int32_t *)S.order, S.nvox, S.W, S.keep, S.maps, (const unsigned long long *)S.masks,
                                                           (const unsigned long long *)S.offsets, (uint4 *)(d + L.off[3]), (uint8_t *)(d + L.off[4]),
                                                           chain_head));
        e = hipGetLastError();
    }
    if (e == hipSuccess && S.P > 0) {
        for (int i = 5; i < HV_GP_SECTIONS && e == hipSuccess; ++i) e = hipMemsetAsync(d + L.off[i], 0, L.size[i], s);
        if (e == hipSuccess) {
            rc = pack_exclusive_scan(v, rocprim::make_transform_iterator((const uint8_t *)(d + L.off[4]), GpPairCount()), pair_off, (size_t)S.N);
            if (rc != HV_OK) return rc;
            hipLaunchKernelGGL(k_grid_emit_pairs, dim3((unsigned)((S.N + 255) / 256)), dim3(256), 0, s, (const HvProbNode *)v->table.prob_nodes,
                               v->table.prob_node_cap, (const uint8_t *)(d + L.off[4]), (const uint32_t *)chain_head, (const unsigned long long *)pair_off,
                               S.N, (unsigned long long)S.P, (int32_t *)(d + L.off[5]), (int32_t *)(d + L.off[6]), (float *)(d + L.off[7]));
            e = hipGetLastError();
        }
    }
    if (e == hipSuccess && loc == HV_HOST) e = hipMemcpyAsync(dst, d, (size_t)L.total, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        hv_set_error("hv_grid_pack: writing the packed grid failed: %s", hipGetErrorString(e));
        return HV_ERR_DEVICE;
    }
    return HV_OK;
}

int hv_grid_unpack(hv_volume *v, const void *src, int64_t bytes, int32_t loc, hv_grid_pack_info *info) {
    const char *fn = "hv_grid_unpack";
    HV_REQUIRE(v != nullptr && src != nullptr, HV_ERR_INVALID, "%s: null argument", fn);
    HV_REQUIRE(loc == HV_HOST || loc == HV_DEVICE, HV_ERR_INVALID, "%s: loc must be HV_HOST or HV_DEVICE", fn);
    int rc = gp_require_whole_grid(v, fn);
    if (rc != HV_OK) return rc;
    HV_REQUIRE(bytes >= HV_GRID_PACK_HEADER_BYTES, HV_ERR_INVALID, "%s: %lld bytes are fewer than the %d-byte header", GP_CHECK, (long long)bytes,
               HV_GRID_PACK_HEADER_BYTES);
    int64_t used = 0;
    rc = hv_tsdf_drain(v, fn, true, &used);
    if (rc != HV_OK) return rc;
    // nothing reaches a kernel before the validator has passed it: a host buffer as it lies, of a device buffer the header and then the
    // four metadata sections (the records and pairs are only ever indexed through them)
    GridHeader H;
    int64_t nodes_needed = 0;
    if (loc == HV_HOST) {
        const unsigned char *p = (const unsigned char *)src;
        rc = gp_check_header(p, bytes, &H, nullptr);
        if (rc != HV_OK) return rc;
        rc = gp_check_meta(H, p + H.off[0], p + H.off[1], p + H.off[2], p + H.off[4], &nodes_needed);
        if (rc != HV_OK) return rc;
    } else {
        unsigned char header[HV_GRID_PACK_HEADER_BYTES];
        rc = unpack_fetch_header(v, src, header, sizeof(header));
        if (rc != HV_OK) return rc;
        rc = gp_check_header(header, bytes, &H, nullptr);
        if (rc != HV_OK) return rc;
        const int which[4] = {0, 1, 2, 4};
        std::vector<unsigned char> meta[4];
        rc = unpack_fetch_sections(v, src, H.off, H.size, which, 4, meta);
        if (rc != HV_OK) return rc;
        rc = gp_check_meta(H, meta[0].data(), meta[1].data(), meta[2].data(), meta[3].data(), &nodes_needed);
        if (rc != HV_OK) return rc;
    }
    HV_REQUIRE(H.mode == v->cfg.mode && H.bs == v->cfg.block_size, HV_ERR_INVALID,
               "%s: the packed grid has mode %d and block_size %d, the volume mode %d and block_size %d", fn, H.mode, H.bs, v->cfg.mode,
               v->cfg.block_size);
    HV_REQUIRE(memcmp(&H.voxel_size, &v->cfg.voxel_size, 8) == 0, HV_ERR_INVALID,
               "%s: the packed grid has voxel_size %.17g, the volume %.17g (they must be bitwise equal)", fn, H.voxel_size, v->cfg.voxel_size);
    HV_REQUIRE(used == 0, HV_ERR_INVALID, "%s: the volume holds %lld blocks; a packed grid is unpacked into an EMPTY grid", fn, (long long)used);
    HV_REQUIRE(H.B < (1ll << 30), HV_ERR_CAPACITY, "%s: %lld blocks are too many", fn, (long long)H.B);
    const bool maps = hv_mode_has_label_maps(H.mode);
    const uint32_t keep = gp_keep_words(H.mode);
    hipStream_t s = v->stream;

    HvScratch S;
    char *tmp = nullptr;
    if (loc == HV_HOST && H.B > 0) {
        HV_HIP(S.get(&tmp, (size_t)bytes));
        rc = hv_h2d(v, tmp, src, (size_t)bytes);
        if (rc != HV_OK) return rc;
    }
    const char *d = loc == HV_HOST ? (const char *)tmp : (const char *)src;
    unsigned long long *node_off = nullptr, *pair_off = nullptr;
    if (maps && H.N > 0) {
        // what the metadata cannot establish: every record's meta against its extras entry (read-only, before anything is claimed)
        unsigned long long *first_bad = nullptr, bad = ~0ull;
        HV_HIP(S.get(&first_bad, 1));
        HV_HIP(hipMemsetAsync(first_bad, 0xFF, 8, s));
        hipLaunchKernelGGL(k_grid_check_records, dim3((unsigned)((H.N + 255) / 256)), dim3(256), 0, s, (const uint4 *)(d + H.off[3]),
                           (const uint8_t *)(d + H.off[4]), H.N, H.mode == HV_MODE_VOXEL_SEMANTIC_PROBABILISTIC_GRID2, first_bad);
        HV_HIP(hipGetLastError());
        HV_HIP(hipMemcpyAsync(&bad, first_bad, 8, hipMemcpyDeviceToHost, s));
        HV_HIP(hipStreamSynchronize(s));
        if (bad != ~0ull) {
            uint32_t meta = 0;
            uint8_t extra = 0;
            HV_HIP(hipMemcpy(&meta, d + H.off[3] + bad * 128 + 4, 4, hipMemcpyDeviceToHost));
            HV_HIP(hipMemcpy(&extra, d + H.off[4] + bad, 1, hipMemcpyDeviceToHost));
            const int rule = gp_record_rule(meta, extra, H.mode == HV_MODE_VOXEL_SEMANTIC_PROBABILISTIC_GRID2);
            HV_REQUIRE(rule != 1, HV_ERR_INVALID, "%s: record %llu: meta names %u label pairs, extras[%llu] is %d (it must be max(pairs - %d, 0), pairs <= %d)",
                       fn, bad, meta & 0xffu, bad, (int)extra, HV_PROB_K, HV_PROB_MAX);
            HV_REQUIRE(false, HV_ERR_INVALID, "%s: record %llu: a cached best index of meta 0x%08x exceeds its %u label pairs", fn, bad, meta, meta & 0xffu);
        }
        HV_REQUIRE(nodes_needed <= (int64_t)v->table.prob_node_cap, HV_ERR_CAPACITY,
                   "%s: the label maps need %lld overflow nodes, the volume's node pool holds %d (create the grid with a larger max_blocks: 4 nodes per "
                   "block, at least 65536)",
                   fn, (long long)nodes_needed, v->table.prob_node_cap);
        if (H.P > 0) {
            HV_HIP(S.get(&node_off, (size_t)H.N));
            HV_HIP(S.get(&pair_off, (size_t)H.N));
        }
    }
    if (info != nullptr) *info = hv_grid_pack_info{H.B, H.N, H.P, H.total};
    if (H.B > 0) {
        // claim first, and verify (this call waits for the GPU anyway)
        rc = unpack_claim_keys(v, (const int32_t *)(d + H.off[0]), H.B);
        if (rc != HV_OK) return rc;
    }
    v->content_version += 1;
    v->assoc_state = 0;
    hv_segments_cache_free(v->segments_cache);
    v->segments_cache = nullptr;
    hipError_t e = hipSuccess;
    if (H.B > 0) {
        if (node_off != nullptr) {
            rc = pack_exclusive_scan(v, rocprim::make_transform_iterator((const uint8_t *)(d + H.off[4]), GpNodeCount()), node_off, (size_t)H.N);
            if (rc == HV_OK) rc = pack_exclusive_scan(v, rocprim::make_transform_iterator((const uint8_t *)(d + H.off[4]), GpPairCount()), pair_off, (size_t)H.N);
            if (rc != HV_OK) {
                (void)hv_reset(v); // the claimed blocks were never written
                return rc;
            }
        }
        hv_profile_begin(v);
        HV_GP_BY_RECORD(H.record_bytes, hipLaunchKernelGGL(k_grid_scatter<RB>, dim3((unsigned)H.B), dim3(256), 0, s, v->table, (char *)v->pool, v->occ, H.nvox,
                                                           H.W, keep, maps, (const int32_t *)(d + H.off[0]), (const unsigned long long *)(d + H.off[1]),
                                                           (const unsigned long long *)(d + H.off[2]), (unsigned long long)H.N,
                                                           (const uint4 *)(d + H.off[3]), (const uint8_t *)(d + H.off[4]),
                                                           (const unsigned long long *)node_off));
        hv_profile_end(v, H.B);
        e = hipGetLastError();
        if (e == hipSuccess && node_off != nullptr) {
            hipLaunchKernelGGL(k_grid_chains, dim3((unsigned)((H.N + 255) / 256)), dim3(256), 0, s, (HvProbNode *)v->table.prob_nodes, v->table.prob_node_cap,
                               (const uint8_t *)(d + H.off[4]), (const unsigned long long *)node_off, (const unsigned long long *)pair_off, H.N,
                               (unsigned long long)H.P, (const int32_t *)(d + H.off[5]), (const int32_t *)(d + H.off[6]), (const float *)(d + H.off[7]));
            e = hipGetLastError();
        }
        const int32_t nodes_used = (int32_t)nodes_needed;
        if (e == hipSuccess && maps) e = hipMemcpyAsync(&v->table.counters[HV_CNT_PROB_NODES], &nodes_used, sizeof(int32_t), hipMemcpyHostToDevice, s);
        hv_launch_publish_status(v); // the unpacked blocks are part of the published occupancy
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            hv_set_error("%s: the scatter failed: %s (the grid holds the claimed blocks, possibly unwritten: hv_reset it)", fn, hipGetErrorString(e));
            return HV_ERR_DEVICE;
        }
        unpack_occupancy_exact(v, H.B);
    }
    if (hv_is_semantic(v) && hv_peek_next_object_id() < H.next_object_id) hv_set_next_object_id(H.next_object_id);
    HV_HIP(hipSetDevice(v->device));
    return HV_OK;
}

} // extern "C"
