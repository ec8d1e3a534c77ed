// libpyslam_hipvol.so — point lookup on the block grids (hv_lookup_points) on gfx950: what does the plain VoxelBlockGrid or one of the
// four semantic grids hold at given points - count, mean position, mean colour, class id, object id and confidence of the voxel the
// point falls into or, with radius >= 1, of the qualifying voxel around it whose mean position is nearest.  The grids' counterpart of
// hv_tsdf_sample_points; the contract is written once in include/hipvol.h, tests/lookup_reference.py restates it in numpy.
//
// One template over the voxel record (HvVoxel and the four semantic payloads), the point dtype and NEAR (radius >= 1).
//   own voxel   one lane per point: the point's voxel by the integrate's own key functions (hv_query.h / hv_semantic.h), one table probe,
//               one record read.  radius == 0 ends here: the neighbourhood code is not in that instantiation.
//   near        mesh vertices of a surface fused into both maps mostly find their own voxel, so the neighbourhood is searched only for
//               the points the first step left open, one after the other by the whole wave: the blocks the (2r+1)^3 voxels span (at
//               most 8 at block sizes >= 2r+1) are probed once, by one lane each, into the wave's LDS window; a lane per candidate
//               then tests the occupancy bit and the count before it touches the rest of the record, and forms d2 to the mean position;
//               a wave min over (d2, offset index) picks the winner, whose lane alone reads the record for the outputs and hands them
//               to the point's lane.
//   outputs     every lane holds its point's row; the [n,3] rows pass through the wave's LDS window so that each store instruction
//               of the wave writes consecutive addresses.
// No atomics on outputs (the four status counters are integer atomics, one per wave and status after a ballot), no scratch; the
// kernels read the table, the pool, the occupancy words and the label nodes only.
#include <algorithm>
#include <climits>
#include <cmath>
#include <type_traits>

#include "hv_common.h"
#include "hv_query.h"
#include "hv_semantic.h"

namespace {

struct HvLookupArgs {
    HvGridParams G;  // the lattice (and the plain grid's key)
    HvSemParams S;   // the semantic grids' key
    int32_t min_count; // max(min_count, 1)
    float min_confidence;
    int32_t radius;
    const unsigned long long *occ; // semantic grids: "may be occupied" bits, pool order
    uint8_t *status;
    int32_t *count;
    double *position;
    float *color;
    int32_t *class_id, *object_id;
    float *confidence;
    unsigned long long *stat; // [4] status counts, or nullptr
};

struct HvLookupRow {
    int32_t status, count;
    double m[3];
    float col[3];
    int32_t cls, obj;
    float conf;
};

template <typename VOX>
constexpr bool lk_plain = std::is_same<VOX, HvVoxel>::value;

// The voxel `integrate` puts the point in (the integrate's own functions, per mode and point dtype); false: LOOKUP_INVALID.
template <typename VOX, typename PT>
__device__ __forceinline__ bool lk_own_voxel(const HvLookupArgs &A, PT x, PT y, PT z, int32_t *v) {
    if constexpr (lk_plain<VOX>) {
        if (!hv_point_keyable(x, y, z, A.G)) return false;
        const HvPointKey k = hv_point_key(x, y, z, A.G);
        if (!hv_key_in_range(k.b[0], k.b[1], k.b[2])) return false;
#pragma unroll
        for (int a = 0; a < 3; ++a) v[a] = k.v[a];
        return true;
    } else {
        unsigned long long bkey = 0ull;
        uint32_t lidx = 0u;
        bool foreign = false;
        // (another rank's block is a voxel like any other: the table does not hold it)
        if (!sem_point_block(A.S, (double)x, (double)y, (double)z, sizeof(PT) == 8, bkey, lidx, foreign) && !foreign) return false;
        int32_t b[3];
        hv_unpack_key(bkey, b[0], b[1], b[2]);
        const int32_t bs = A.S.bs;
        v[0] = b[0] * bs + (int32_t)(lidx % (uint32_t)bs);
        v[1] = b[1] * bs + (int32_t)((lidx / (uint32_t)bs) % (uint32_t)bs);
        v[2] = b[2] * bs + (int32_t)(lidx / (uint32_t)(bs * bs));
        return true;
    }
}

// hv_floor_div(c, bs): an arithmetic shift where the block size is a power of two
__device__ __forceinline__ int32_t lk_block_of(const HvGridParams &G, int32_t c) { return G.bs_shift >= 0 ? (c >> G.bs_shift) : hv_floor_div(c, G.bs); }

// pool index of block (bx, by, bz), -1: not held (or its key is out of range)
__device__ __forceinline__ int32_t lk_block_index(const HvTable &table, int32_t bx, int32_t by, int32_t bz) {
    if (!hv_key_in_range(bx, by, bz)) return -1;
    const int32_t slot = hv_table_find(table, hv_pack_key(bx, by, bz));
    return slot < 0 ? -1 : table.vals[slot];
}

// The contract's "qualifies" for the voxel at pool position gid: the occupancy bit and the count before anything else of the record.
template <typename VOX>
__device__ __forceinline__ bool lk_qualifies(const HvLookupArgs &A, const HvTable &table, const VOX *__restrict__ pool, int64_t gid, int32_t &count) {
    if constexpr (!lk_plain<VOX>) {
        if (!sem_maybe_occupied(A.occ, gid)) return false;
    }
    count = pool[gid].count;
    if (count < A.min_count) return false;
    if constexpr (lk_plain<VOX>) return true;
    else return sem_confidence(pool + gid, table.prob_nodes) >= A.min_confidence; // hv_get_voxels_semantic's test
}

// the mean position get_voxels lists: float64 sums / (double)count (semantic), float32 sums / (float)count widened (plain)
template <typename VOX>
__device__ __forceinline__ void lk_mean(const VOX *rec, int32_t count, double *m) {
    if constexpr (lk_plain<VOX>) {
        const float c = (float)count;
#pragma unroll
        for (int k = 0; k < 3; ++k) m[k] = (double)(rec->pos[k] / c);
    } else {
        const double c = (double)count;
#pragma unroll
        for (int k = 0; k < 3; ++k) m[k] = rec->pos[k] / c;
    }
}

template <typename VOX>
__device__ __forceinline__ void lk_fill(const HvLookupArgs &A, const HvTable &table, const VOX *rec, int32_t count, int status, HvLookupRow &o) {
    o.status = status;
    o.count = count;
    lk_mean(rec, count, o.m);
    const float cf = (float)count;
#pragma unroll
    for (int k = 0; k < 3; ++k) o.col[k] = rec->col[k] / cf;
    if constexpr (!lk_plain<VOX>) {
        if (A.class_id) o.cls = sem_class_id(rec, table.prob_nodes);
        if (A.object_id) o.obj = sem_object_id(rec, table.prob_nodes);
        if (A.confidence) o.conf = sem_confidence(rec, table.prob_nodes);
    }
}

template <typename VOX, typename PT, bool NEAR>
__global__ __launch_bounds__(256) void k_lookup(HvTable table, const VOX *__restrict__ pool, const PT *__restrict__ pts, int64_t n, HvLookupArgs A) {
    __shared__ double s_rows[4][HV_WAVE * 3];                 // per wave: the [64,3] rows on their way out
    __shared__ int32_t s_blk[NEAR ? 4 : 1][NEAR ? 128 : 1];   // per wave: pool indices of the blocks one neighbourhood spans (<= 5^3)
    const int lane = hv_lane_id(), wave = (int)(threadIdx.x >> 6);
    const int64_t base = ((int64_t)blockIdx.x * 4 + wave) * HV_WAVE; // the wave's first point
    if (base >= n) return;                                            // (the whole wave)
    const int64_t i = base + lane;
    const bool live = i < n;
    const int32_t bs = A.G.bs;

    HvLookupRow o;
    o.status = HV_LOOKUP_MISSING;
    o.count = 0;
    o.cls = o.obj = -1;
    o.conf = 0.0f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        o.m[k] = 0.0;
        o.col[k] = 0.0f;
    }
    int32_t v[3] = {0, 0, 0};
    double p[3] = {0.0, 0.0, 0.0};
    bool open = false; // own voxel does not qualify: the neighbourhood decides
    if (live) {
        const PT x = pts[i * 3 + 0], y = pts[i * 3 + 1], z = pts[i * 3 + 2];
        p[0] = (double)x;
        p[1] = (double)y;
        p[2] = (double)z;
        if (!lk_own_voxel<VOX>(A, x, y, z, v)) {
            o.status = HV_LOOKUP_INVALID;
        } else {
            const int32_t b[3] = {lk_block_of(A.G, v[0]), lk_block_of(A.G, v[1]), lk_block_of(A.G, v[2])};
            const int32_t idx = lk_block_index(table, b[0], b[1], b[2]);
            int32_t cnt = 0;
            bool own = false;
            int64_t gid = 0;
            if (idx >= 0) {
                gid = (int64_t)idx * A.G.nvox + ((v[0] - b[0] * bs) + (v[1] - b[1] * bs) * bs + (v[2] - b[2] * bs) * bs * bs);
                own = lk_qualifies(A, table, pool, gid, cnt);
            }
            if (own) lk_fill(A, table, pool + gid, cnt, HV_LOOKUP_OWN, o);
            else open = NEAR;
        }
    }

    if constexpr (NEAR) {
        int32_t *blk = s_blk[wave];
        const int r = A.radius, w = 2 * r + 1, nc = w * w * w;
        unsigned long long todo = __ballot(open);
        while (todo != 0ull) { // wave-uniform
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1ull;
            const int32_t v0[3] = {__shfl(v[0], src), __shfl(v[1], src), __shfl(v[2], src)};
            const double q[3] = {__shfl(p[0], src), __shfl(p[1], src), __shfl(p[2], src)};
            // the blocks the neighbourhood spans, resolved once (|v0| < 1e9: no overflow)
            int32_t blo[3], nb[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                blo[a] = lk_block_of(A.G, v0[a] - r);
                nb[a] = lk_block_of(A.G, v0[a] + r) - blo[a] + 1; // <= 2 for bs >= 2r+1, <= 5 at bs == 1
            }
            const int nblk = nb[0] * nb[1] * nb[2];
            hv_wave_lds_sync(); // the previous point's window is no longer read
            for (int j = lane; j < nblk; j += HV_WAVE)
                blk[j] = lk_block_index(table, blo[0] + j % nb[0], blo[1] + (j / nb[0]) % nb[1], blo[2] + j / (nb[0] * nb[1]));
            hv_wave_lds_sync();
            // a lane per candidate (two turns at radius 2); a lane keeps the best of its turns - offsets ascend, so an equal d2 keeps the earlier
            unsigned long long best_bits = ~0ull;
            int best_c = INT_MAX;
            int64_t best_gid = 0;
            int32_t best_count = 0;
            for (int c = lane; c < nc; c += HV_WAVE) {
                const int32_t cv[3] = {v0[0] + (c % w - r), v0[1] + ((c / w) % w - r), v0[2] + (c / (w * w) - r)};
                const int32_t cb[3] = {lk_block_of(A.G, cv[0]), lk_block_of(A.G, cv[1]), lk_block_of(A.G, cv[2])};
                const int32_t idx = blk[(cb[0] - blo[0]) + (cb[1] - blo[1]) * nb[0] + (cb[2] - blo[2]) * nb[0] * nb[1]];
                if (idx < 0) continue;
                const int64_t gid = (int64_t)idx * A.G.nvox + ((cv[0] - cb[0] * bs) + (cv[1] - cb[1] * bs) * bs + (cv[2] - cb[2] * bs) * bs * bs);
                int32_t cnt = 0;
                if (!lk_qualifies(A, table, pool, gid, cnt)) continue;
                double m[3];
                lk_mean(pool + gid, cnt, m);
                const double e0 = m[0] - q[0], e1 = m[1] - q[1], e2 = m[2] - q[2];
                const double d2 = (e0 * e0 + e1 * e1) + e2 * e2;
                const unsigned long long bits = (unsigned long long)__double_as_longlong(d2); // d2 >= 0: its bits order as its value
                if (bits < best_bits) {
                    best_bits = bits;
                    best_c = c;
                    best_gid = gid;
                    best_count = cnt;
                }
            }
            const unsigned long long win_bits = hv_wave_min(best_bits);
            const int win_c = hv_wave_min((best_c != INT_MAX && best_bits == win_bits) ? best_c : INT_MAX);
            if (win_c == INT_MAX) continue; // nothing qualifies: MISSING (wave-uniform)
            const int win = win_c & (HV_WAVE - 1);
            HvLookupRow f = o;
            if (lane == win) lk_fill(A, table, pool + best_gid, best_count, HV_LOOKUP_NEAR, f);
            // the winner's row goes to the point's lane
            const bool mine = lane == src;
            const int32_t t_status = __shfl(f.status, win), t_count = __shfl(f.count, win), t_cls = __shfl(f.cls, win), t_obj = __shfl(f.obj, win);
            const float t_conf = __shfl(f.conf, win);
            o.status = mine ? t_status : o.status;
            o.count = mine ? t_count : o.count;
            o.cls = mine ? t_cls : o.cls;
            o.obj = mine ? t_obj : o.obj;
            o.conf = mine ? t_conf : o.conf;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double t_m = __shfl(f.m[k], win);
                const float t_col = __shfl(f.col[k], win);
                o.m[k] = mine ? t_m : o.m[k];
                o.col[k] = mine ? t_col : o.col[k];
            }
        }
    }

    if (live) {
        if (A.status) A.status[i] = (uint8_t)o.status;
        if (A.count) A.count[i] = o.count;
        if (A.class_id) A.class_id[i] = o.cls;
        if (A.object_id) A.object_id[i] = o.obj;
        if (A.confidence) A.confidence[i] = o.conf;
    }
    const int rows3 = (n - base < HV_WAVE ? (int)(n - base) : HV_WAVE) * 3;
    if (A.position) {
        double *t = s_rows[wave];
        hv_wave_lds_sync();
#pragma unroll
        for (int k = 0; k < 3; ++k) t[lane * 3 + k] = o.m[k];
        hv_wave_lds_sync();
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int j = k * HV_WAVE + lane;
            if (j < rows3) A.position[base * 3 + j] = t[j];
        }
    }
    if (A.color) {
        float *t = (float *)s_rows[wave];
        hv_wave_lds_sync();
#pragma unroll
        for (int k = 0; k < 3; ++k) t[lane * 3 + k] = o.col[k];
        hv_wave_lds_sync();
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int j = k * HV_WAVE + lane;
            if (j < rows3) A.color[base * 3 + j] = t[j];
        }
    }
    if (A.stat != nullptr) { // exact integer counts: one atomic per wave and status
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const unsigned long long m = __ballot(live && o.status == k);
            if (m != 0ull && lane == __ffsll((long long)m) - 1) atomicAdd(&A.stat[k], (unsigned long long)__popcll(m));
        }
    }
}

template <typename VOX>
void lookup_launch(hv_volume *v, const void *d_points, bool f64, int64_t n, const HvLookupArgs &A) {
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    const VOX *pool = (const VOX *)v->pool;
#define HV_LOOKUP_LAUNCH(PT, NEAR) hipLaunchKernelGGL((k_lookup<VOX, PT, NEAR>), grid, block, 0, v->stream, v->table, pool, (const PT *)d_points, n, A)
    if (A.radius > 0) {
        if (f64) HV_LOOKUP_LAUNCH(double, true);
        else HV_LOOKUP_LAUNCH(float, true);
    } else {
        if (f64) HV_LOOKUP_LAUNCH(double, false);
        else HV_LOOKUP_LAUNCH(float, false);
    }
#undef HV_LOOKUP_LAUNCH
}

} // namespace

extern "C" int hv_lookup_points(hv_volume *v, const void *points, int32_t point_dtype, int64_t n, const hv_lookup_params *p, uint8_t *status,
                                int32_t *count, double *position, float *color, int32_t *class_id, int32_t *object_id, float *confidence,
                                hv_lookup_stats *stats, int32_t loc) {
    const char *fn = "hv_lookup_points";
    HV_REQUIRE(v != nullptr && p != nullptr, HV_ERR_INVALID, "%s: null argument", fn);
    const bool plain = v->cfg.mode == HV_MODE_VOXEL_GRID;
    HV_REQUIRE(plain || hv_is_semantic(v), HV_ERR_MODE, "%s: the volume is not a voxel block grid", fn);
    HV_REQUIRE(n >= 0 && n <= (1ll << 36), HV_ERR_INVALID, "%s: bad point count %lld", fn, (long long)n);
    HV_REQUIRE(points != nullptr || n == 0, HV_ERR_INVALID, "%s: null points", fn);
    HV_REQUIRE(point_dtype == HV_F32 || point_dtype == HV_F64, HV_ERR_INVALID, "%s: points must be float32 or float64", fn);
    HV_REQUIRE(loc == HV_HOST || loc == HV_DEVICE, HV_ERR_INVALID, "%s: bad loc %d", fn, (int)loc);
    HV_REQUIRE(p->radius >= 0 && p->radius <= 2, HV_ERR_INVALID, "%s: radius must be 0, 1 or 2, got %d", fn, (int)p->radius);
    HV_REQUIRE(!plain || (class_id == nullptr && object_id == nullptr && confidence == nullptr), HV_ERR_INVALID,
               "%s: a plain voxel grid holds no class id, object id or confidence", fn);
    if (stats != nullptr) *stats = hv_lookup_stats{0, 0, 0, 0, 0};
    if (n == 0) return HV_OK;
    HV_HIP(hipSetDevice(v->device));

    // head: the 4 status counters
    const size_t un = (size_t)n;
    HvStage st(v, loc);
    st.head(stats != nullptr ? 256 : 0);
    const int i_points = st.in(points, un * 3 * (point_dtype == HV_F64 ? 8 : 4));
    const int o_status = st.out(status, un), o_count = st.out(count, 4 * un), o_position = st.out(position, 24 * un), o_color = st.out(color, 12 * un),
              o_class = st.out(class_id, 4 * un), o_object = st.out(object_id, 4 * un), o_conf = st.out(confidence, 4 * un);
    int rc = st.commit(&v->stage, &v->stage_bytes);
    if (rc != HV_OK) return rc;
    const void *d_points = st.dev<const void>(i_points);

    HvLookupArgs A{};
    A.G = grid_params(v);
    A.S = sem_params(v);
    A.min_count = std::max(p->min_count, 1);
    A.min_confidence = p->min_confidence;
    A.radius = p->radius;
    A.occ = plain ? nullptr : v->occ;
    A.status = st.dev<uint8_t>(o_status);
    A.count = st.dev<int32_t>(o_count);
    A.position = st.dev<double>(o_position);
    A.color = st.dev<float>(o_color);
    A.class_id = st.dev<int32_t>(o_class);
    A.object_id = st.dev<int32_t>(o_object);
    A.confidence = st.dev<float>(o_conf);
    A.stat = (unsigned long long *)st.head_dev;
    if (A.stat != nullptr) HV_HIP(hipMemsetAsync(A.stat, 0, 4 * sizeof(unsigned long long), v->stream));
    const bool f64 = point_dtype == HV_F64;
    hv_profile_begin(v);
    if (plain) {
        lookup_launch<HvVoxel>(v, d_points, f64, n, A);
    } else {
        HV_SEM_DISPATCH(v, lookup_launch<VOX>(v, d_points, f64, n, A));
    }
    hv_profile_end(v, 0);
    HV_HIP(hipGetLastError());
    unsigned long long h_count[4];
    rc = st.finish(stats != nullptr ? h_count : nullptr, sizeof(h_count));
    if (rc != HV_OK) return rc;
    if (stats != nullptr) {
        stats->points = n;
        stats->missing = (int64_t)h_count[HV_LOOKUP_MISSING];
        stats->own = (int64_t)h_count[HV_LOOKUP_OWN];
        stats->near = (int64_t)h_count[HV_LOOKUP_NEAR];
        stats->invalid = (int64_t)h_count[HV_LOOKUP_INVALID];
    }
    return HV_OK;
}
