// libpyslam_hipvol.so — TSDF de-integration (BundleFusion's correction of a map whose poses moved): take the observations
// a posed frame added back out of the voxels it updated, so that a frame can be re-integrated at a corrected pose without a
// rebuild.  Contract: include/hipvol.h, hv_tsdf_deintegrate.
//
// Per chunk of <= 64 frames, all on the volume's stream:
//   k_tsdf_deint_touch  one launch, two block roles as k_tsdf_prep_touch_batch: pack blocks write every frame's 8-byte
//                       {depth, colour} records (hv_pack_px4, the integrate path's own conversion); touch blocks run the integrate
//                       touch pass (hv_touch_patch) with a hash LOOKUP instead of a claim: a unit the volume holds gets bit f of
//                       its frame mask and, at its first touch in the chunk, a stamp and its place in the union list; a unit it
//                       does not hold is skipped (and, when the caller wants stats, counted once per frame through a scratch
//                       key set).
//   k_tsdf_deint_sweep  one workgroup per listed unit, the online sweep's lane layout (wave w: z in [4w, 4w + 4), lane: x and
//                       4 y's).  A lane walks the unit's frame bits in ascending order and accumulates, per voxel, the number
//                       of frames that sample it, their tsdf samples (double, frame order) and colour bytes - the projection
//                       and predicate are hv_tsdf_eval_fast, the function the fuse kernels use.  The unit's planes are then
//                       read and written once.
//   k_tsdf_deint_finish clears the chunk's frame masks and list counter.
#include <algorithm>
#include <cstring>
#include <vector>

#include "hv_tsdf_device.h"

enum { HV_DEINT_LISTED = 0, HV_DEINT_MISSING = 1, HV_DEINT_REMOVED = 2, HV_DEINT_UNDERFLOW = 3, HV_DEINT_MISS_FULL = 4 };
static constexpr size_t HV_DEINT_HDR = 256; // counter block at the head of deint_buf

__global__ __launch_bounds__(256) void k_tsdf_deint_touch(HvTable table, int32_t *__restrict__ stamp,
                                                           unsigned long long *__restrict__ frame_mask, int32_t *__restrict__ list,
                                                           int batch_stamp, const char *__restrict__ depth_raw, int64_t depth_stride,
                                                           const uint8_t *__restrict__ rgb, uint2 *__restrict__ frame_px,
                                                           const HvFrameParams *__restrict__ Ps, int n_prep_blocks, int n_touch_blocks,
                                                           int n_frames, unsigned long long *__restrict__ cnt,
                                                           unsigned long long *__restrict__ miss_keys,
                                                           unsigned long long *__restrict__ miss_mask, uint32_t miss_cap_mask) {
    int f, bx;
    const bool touch_role = (int)blockIdx.x < n_touch_blocks * n_frames;
    if (touch_role) {
        f = (int)blockIdx.x / n_touch_blocks;
        bx = (int)blockIdx.x % n_touch_blocks;
    } else {
        const int b = (int)blockIdx.x - n_touch_blocks * n_frames;
        f = b / n_prep_blocks;
        bx = b % n_prep_blocks;
    }
    const HvFrameParams &P = Ps[f];
    const int64_t npx = (int64_t)P.H * P.W;
    const void *depth_f = depth_raw + (int64_t)f * depth_stride;
    if (!touch_role) {
        hv_pack_px4(P, f, ((int64_t)bx * blockDim.x + threadIdx.x) * 4, depth_f, rgb + (int64_t)f * npx * 3, frame_px, nullptr);
        return;
    }
    __shared__ HvTouchScratch scratch[4];
    const int patch = bx * 4 + (int)(threadIdx.x / HV_WAVE);
    if (patch >= hv_touch_patches(P)) return; // (whole waves: a patch is one wave)
    const unsigned long long fbit = 1ull << f;
    unsigned long long listed = 0, missing = 0, full = 0;
    hv_touch_patch(table, P, depth_f, patch, scratch[threadIdx.x / HV_WAVE], [&](unsigned long long key, int32_t, int32_t, int32_t) {
        const int32_t slot = hv_table_find(table, key);
        const int32_t idx = slot >= 0 ? table.vals[slot] : -1;
        if (idx >= 0) {
            // this frame's bit: the unit is counted by the lane whose atomicOr set it
            const unsigned long long seen = __hip_atomic_load(&frame_mask[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (!(seen & fbit) && !(atomicOr(&frame_mask[slot], fbit) & fbit)) listed += 1;
            if (__hip_atomic_load(&stamp[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != batch_stamp &&
                atomicExch(&stamp[slot], batch_stamp) != batch_stamp) {
                const int32_t at = atomicAdd(&table.counters[HV_CNT_TOUCH(0)], 1);
                if (at < table.max_blocks) list[at] = slot;
            }
        } else if (miss_keys != nullptr) {
            bool is_new; // (not needed: the frame bit below says whether this frame counted the unit)
            const int32_t ms = hv_keyset_insert(miss_keys, miss_cap_mask, key, &is_new);
            if (ms < 0) {
                full += 1;
            } else if (!(atomicOr(&miss_mask[ms], fbit) & fbit)) {
                listed += 1;
                missing += 1;
            }
        }
    });
    // (hv_touch_patch returns with the whole wave: one atomic per counter and wave)
    listed = hv_wave_sum(listed);
    missing = hv_wave_sum(missing);
    full = hv_wave_sum(full);
    if (hv_lane_id() == 0) {
        if (listed) atomicAdd(&cnt[HV_DEINT_LISTED], listed);
        if (missing) atomicAdd(&cnt[HV_DEINT_MISSING], missing);
        if (full) atomicAdd(&cnt[HV_DEINT_MISS_FULL], full);
    }
}

// One voxel: n frames sampled it with tsdf samples summing to s (double, frame order) and colour bytes rg = r | g << 16,
// bn = b | n << 16.  The update rule of include/hipvol.h.
__device__ __forceinline__ void hv_deint_apply(double s, uint32_t rg, uint32_t bn, float &tsdf, uint32_t &w, uint32_t &sr, uint32_t &sg,
                                               uint32_t &sb, uint32_t &removed, uint32_t &underflow) {
    const uint32_t n = bn >> 16;
    if (n == 0) return;
    if (w < n) {
        underflow += 1;
        return;
    }
    removed += n;
    if (w == n) { // back to the state of a freshly claimed voxel (the pool is zero-initialised)
        tsdf = 0.0f;
        w = sr = sg = sb = 0u;
        return;
    }
    const uint32_t w1 = w - n;
    tsdf = (float)(((double)tsdf * (double)w - s) / (double)w1);
    w = w1;
    // each sum stays in [0, 255 * w]: the clamp acts only when a frame that was never fused into the voxel is removed from it
    const uint32_t top = 255u * w1;
    const uint32_t r = rg & 0xffffu, g = rg >> 16, b = bn & 0xffffu;
    sr = sr > r ? std::min(sr - r, top) : 0u;
    sg = sg > g ? std::min(sg - g, top) : 0u;
    sb = sb > b ? std::min(sb - b, top) : 0u;
}

// One frame's samples of a lane's 4 x 4 voxels added to its accumulators: n and colour bytes packed (rg = r | g << 16, bn = b | n << 16:
// <= 64 frames x 255 fit in 16 bits), the tsdf samples summed in double in frame order.
__device__ __forceinline__ void hv_deint_frame(const HvFrameParams &P, const uint2 *__restrict__ px, const float *__restrict__ mult,
                                               float (&pc)[4][3], float inc0, float inc1, float inc2, double (&st)[4][4],
                                               uint32_t (&rg)[4][4], uint32_t (&bn)[4][4]) {
#pragma unroll
    for (int zz = 0; zz < 4; ++zz) {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float tv;
            uint32_t cv;
            const bool ok = hv_tsdf_eval_fast<true, true>(P, px, mult, pc[c][0], pc[c][1], pc[c][2], tv, cv);
            st[zz][c] += ok ? (double)tv : 0.0; // (+0.0 leaves a sum that started at +0.0 unchanged, bit for bit)
            const uint32_t cm = ok ? cv : 0u;
            rg[zz][c] += (cm & 255u) | (((cm >> 8) & 255u) << 16);
            bn[zz][c] += ok ? (((cm >> 16) & 255u) | (1u << 16)) : 0u;
            pc[c][0] += inc0;
            pc[c][1] += inc1;
            pc[c][2] += inc2;
        }
    }
}

__global__ __launch_bounds__(256) void k_tsdf_deint_sweep(HvTable table, const int32_t *__restrict__ list,
                                                           const unsigned long long *__restrict__ frame_mask, char *__restrict__ pool,
                                                           const uint2 *__restrict__ frame_px, const float *__restrict__ mult,
                                                           const HvFrameParams *__restrict__ Ps, unsigned long long *__restrict__ cnt) {
    int n_units = table.counters[HV_CNT_TOUCH(0)];
    if (n_units > table.max_blocks) n_units = table.max_blocks;
    const int wave = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    const int x = lane >> 2;
    const int y0 = (lane & 3) << 2;
    const int z0 = wave * 4;
    const int64_t npx = (int64_t)Ps[0].H * Ps[0].W;
    uint32_t removed = 0, underflow = 0;
    for (int t = blockIdx.x; t < n_units; t += gridDim.x) {
        const int32_t slot = list[t];
        const int32_t idx = table.vals[slot];
        if (idx < 0) continue;
        int32_t ux, uy, uz;
        hv_unpack_key(table.keys[slot], ux, uy, uz);
        const double o0 = (double)ux * Ps[0].unit_length;
        const double o1 = (double)uy * Ps[0].unit_length;
        const double o2 = (double)uz * Ps[0].unit_length;
        double st[4][4];
        uint32_t rg[4][4], bn[4][4];
#pragma unroll
        for (int zz = 0; zz < 4; ++zz)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                st[zz][c] = 0.0;
                rg[zz][c] = 0u;
                bn[zz][c] = 0u;
            }
        // the unit's frames in ascending (= call) order; the mask is uniform across the workgroup
        for (unsigned long long fm = frame_mask[slot]; fm != 0ull; fm &= fm - 1ull) {
            const int f = __ffsll((long long)fm) - 1;
            const HvFrameParams &P = Ps[f];
            const uint2 *px = frame_px + (int64_t)f * npx;
            const float *mf = mult;
            // voxel centres in camera space exactly as k_tsdf_integrate forms them (float, z advanced by repeated additions)
            const float inc0 = P.ext_scaled_col2[0], inc1 = P.ext_scaled_col2[1], inc2 = P.ext_scaled_col2[2];
            const float p0 = (float)((double)(P.half_voxel_length_f + P.voxel_length_f * (float)x) + o0);
            const float p2 = (float)((double)P.half_voxel_length_f + o2);
            float pc[4][3];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const float p1 = (float)((double)(P.half_voxel_length_f + P.voxel_length_f * (float)(y0 + c)) + o1);
#pragma unroll
                for (int r = 0; r < 3; ++r) pc[c][r] = ((P.ext[r * 4 + 0] * p0 + P.ext[r * 4 + 1] * p1) + P.ext[r * 4 + 2] * p2) + P.ext[r * 4 + 3];
            }
            for (int s = 0; s < z0; ++s) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    pc[c][0] += inc0;
                    pc[c][1] += inc1;
                    pc[c][2] += inc2;
                }
            }
            // the EXACT division form throughout (IEEE division wherever the short chain's band does not hold): measured faster here than
            // choosing the form per wave as hv_tsdf_slabs does (the second copy of the loop costs occupancy: 169 VGPRs, 2 waves per
            // SIMD, 3.9 against 3.5 ms for 64 frames).  Both give the IEEE quotients, so the samples are integrate's either way
            // (whole-image frames only: tile-sharded volumes are refused).
            hv_deint_frame(P, px, mf, pc, inc0, inc1, inc2, st, rg, bn);
        }
        char *unit = pool + (int64_t)idx * HV_TSDF_UNIT_BYTES;
#pragma unroll
        for (int zz = 0; zz < 4; ++zz) {
            if (((bn[zz][0] | bn[zz][1] | bn[zz][2] | bn[zz][3]) >> 16) == 0u) continue;
            const int q = hv_tsdf_word(x, y0, z0 + zz) >> 2;
            float4 vt = ((const float4 *)(unit + 0 * HV_TSDF_PLANE_BYTES))[q];
            uint4 vw = ((const uint4 *)(unit + 1 * HV_TSDF_PLANE_BYTES))[q];
            uint4 vr = ((const uint4 *)(unit + 2 * HV_TSDF_PLANE_BYTES))[q];
            uint4 vg = ((const uint4 *)(unit + 3 * HV_TSDF_PLANE_BYTES))[q];
            uint4 vb = ((const uint4 *)(unit + 4 * HV_TSDF_PLANE_BYTES))[q];
            hv_deint_apply(st[zz][0], rg[zz][0], bn[zz][0], vt.x, vw.x, vr.x, vg.x, vb.x, removed, underflow);
            hv_deint_apply(st[zz][1], rg[zz][1], bn[zz][1], vt.y, vw.y, vr.y, vg.y, vb.y, removed, underflow);
            hv_deint_apply(st[zz][2], rg[zz][2], bn[zz][2], vt.z, vw.z, vr.z, vg.z, vb.z, removed, underflow);
            hv_deint_apply(st[zz][3], rg[zz][3], bn[zz][3], vt.w, vw.w, vr.w, vg.w, vb.w, removed, underflow);
            ((float4 *)(unit + 0 * HV_TSDF_PLANE_BYTES))[q] = vt;
            ((uint4 *)(unit + 1 * HV_TSDF_PLANE_BYTES))[q] = vw;
            ((uint4 *)(unit + 2 * HV_TSDF_PLANE_BYTES))[q] = vr;
            ((uint4 *)(unit + 3 * HV_TSDF_PLANE_BYTES))[q] = vg;
            ((uint4 *)(unit + 4 * HV_TSDF_PLANE_BYTES))[q] = vb;
        }
    }
    const unsigned long long rs = hv_wave_sum<unsigned long long>(removed), us = hv_wave_sum<unsigned long long>(underflow);
    if (lane == 0) {
        if (rs) atomicAdd(&cnt[HV_DEINT_REMOVED], rs);
        if (us) atomicAdd(&cnt[HV_DEINT_UNDERFLOW], us);
    }
}

// After the sweep (one workgroup): clear the chunk's frame masks and its list counter (as k_tsdf_batch_finish).
__global__ __launch_bounds__(1024) void k_tsdf_deint_finish(HvTable table, const int32_t *__restrict__ list,
                                                            unsigned long long *__restrict__ frame_mask) {
    int n_units = table.counters[HV_CNT_TOUCH(0)];
    if (n_units > table.max_blocks) n_units = table.max_blocks;
    __syncthreads(); // every thread holds n_units before the counter is reset
    for (int t = threadIdx.x; t < n_units; t += blockDim.x) frame_mask[list[t]] = 0ull;
    if (threadIdx.x == 0) table.counters[HV_CNT_TOUCH(0)] = 0;
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
static int check_deint_args(hv_volume *v, const void *depth, const uint8_t *rgb, int H, int W, const double *intr, const double *T_cw,
                            int frames) {
    int rc = check_tsdf_args(v, depth, rgb, H, W, intr, T_cw, frames);
    if (rc != HV_OK) return rc;
    HV_REQUIRE(v->tile[0] == 0 && v->tile[1] == 0 && v->tile[2] == 0 && v->tile[3] == 0, HV_ERR_MODE,
               "hv_tsdf_deintegrate: not supported on a tile-sharded volume (its ranks hold partial sums of a voxel)");
    return HV_OK;
}

// F device-resident frames (already rectified when rectify == false), chunks of HV_BATCH_MAX, queued on the volume's stream.
// count_missing: count the touch sets' absent units (the stats' units_missing / units_listed need it).
static int tsdf_deintegrate_device(hv_volume *v, const void *d_depth, int32_t depth_dtype, const uint8_t *d_rgb, int32_t n_frames, int32_t H,
                                   int32_t W, const double *intr, const double *T_cw, double depth_scale, double depth_trunc, bool rectify,
                                   bool count_missing) {
    const size_t npx = (size_t)H * W;
    const size_t dsz = depth_dtype == HV_DEPTH_U16 ? 2 : 4;
    const uint64_t miss_cap = count_missing ? v->table_capacity : 0;
    int rc = hv_ensure_buffer(v, &v->deint_buf, &v->deint_buf_bytes, HV_DEINT_HDR + 16 * (size_t)miss_cap);
    if (rc != HV_OK) return rc;
    unsigned long long *cnt = (unsigned long long *)v->deint_buf;
    unsigned long long *miss_keys = (unsigned long long *)((char *)v->deint_buf + HV_DEINT_HDR);
    unsigned long long *miss_mask = miss_keys + miss_cap;
    HV_HIP(hipMemsetAsync(cnt, 0, HV_DEINT_HDR, v->stream));
    // nothing of an integrate call still runs on its second stream: the main stream waited for each of its launches.  A later
    // integrate call finds content_version moved and starts a fresh chain on the main stream.
    v->content_version += 1;
    std::vector<HvFrameParams> params(HV_BATCH_MAX);
    for (int f0 = 0; f0 < n_frames; f0 += HV_BATCH_MAX) {
        const int B = std::min(HV_BATCH_MAX, n_frames - f0);
        v->frame_counter += 1; // the chunk's stamp: the extraction caches and hv_tsdf_dirty_keys see every unit it wrote
        const int batch_stamp = v->frame_counter;
        for (int f = 0; f < B; ++f) {
            make_frame_params(v, H, W, intr, T_cw + 16 * (size_t)(f0 + f), depth_scale, depth_trunc, depth_dtype, &params[f]);
            params[f].frame_id = batch_stamp;
        }
        rc = tsdf_multiplier_table(v, params[0]);
        if (rc != HV_OK) return rc;
        size_t params_off = 0;
        const size_t want = tsdf_batch_scratch(8, npx, B, &params_off);
        if (v->batch_buf_bytes < want && v->stream_aux) HV_HIP(hipStreamSynchronize(v->stream_aux));
        rc = hv_ensure_buffer(v, &v->batch_buf, &v->batch_buf_bytes, want);
        if (rc != HV_OK) return rc;
        uint2 *d_px = (uint2 *)v->batch_buf;
        HvFrameParams *d_params = (HvFrameParams *)((char *)v->batch_buf + params_off);
        rc = hv_h2d(v, d_params, params.data(), sizeof(HvFrameParams) * (size_t)B); // (pageable: read before it returns)
        if (rc != HV_OK) return rc;
        if (count_missing) {
            HV_HIP(hipMemsetAsync(miss_keys, 0xFF, sizeof(uint64_t) * miss_cap, v->stream));
            HV_HIP(hipMemsetAsync(miss_mask, 0, sizeof(uint64_t) * miss_cap, v->stream));
        }
        const void *c_depth = (const char *)d_depth + npx * dsz * (size_t)f0;
        const uint8_t *c_rgb = d_rgb + npx * 3 * (size_t)f0;
        if (rectify) {
            rc = tsdf_rectify(v, v->stream, &c_depth, depth_dtype, &c_rgb, B, H, W);
            if (rc != HV_OK) return rc;
        }
        // scratch set 0 of the batch path: union list, frame masks (zero between batches) and the list counter
        if (!v->touch_counters_clean) HV_HIP(hipMemsetAsync(&v->table.counters[HV_CNT_TOUCH0], 0, HV_CNT_TOUCH_SPAN_BYTES, v->stream));
        v->touch_counters_clean = true;
        int32_t *d_list = v->touched_list;
        unsigned long long *d_mask = (unsigned long long *)v->touched_mask;
        const int n_prep_blocks = (int)((npx + 1023) / 1024); // 4 pixels per thread
        const int n_touch_blocks = (hv_touch_patches(W, H, v->cfg.depth_sampling_stride) + 3) / 4;
        hipLaunchKernelGGL(k_tsdf_deint_touch, dim3((n_prep_blocks + n_touch_blocks) * B), dim3(256), 0, v->stream, v->table, v->touched_stamp,
                           d_mask, d_list, batch_stamp, (const char *)c_depth, (int64_t)(npx * dsz), c_rgb, d_px,
                           (const HvFrameParams *)d_params, n_prep_blocks, n_touch_blocks, B, cnt, count_missing ? miss_keys : nullptr,
                           miss_mask, (uint32_t)(miss_cap ? miss_cap - 1 : 0));
        hv_profile_begin(v);
        hipLaunchKernelGGL(k_tsdf_deint_sweep, dim3(8192), dim3(256), 0, v->stream, v->table, (const int32_t *)d_list,
                           (const unsigned long long *)d_mask, (char *)v->pool, (const uint2 *)d_px, (const float *)v->mult_table,
                           (const HvFrameParams *)d_params, cnt);
        hv_profile_end(v, B);
        hipLaunchKernelGGL(k_tsdf_deint_finish, dim3(1), dim3(1024), 0, v->stream, v->table, (const int32_t *)d_list, d_mask);
        HV_HIP(hipGetLastError());
    }
    return HV_OK;
}

static int deint_read_stats(hv_volume *v, hv_deintegrate_stats *stats) {
    unsigned long long c[5] = {0, 0, 0, 0, 0};
    HV_HIP(hipMemcpyAsync(c, v->deint_buf, sizeof(c), hipMemcpyDeviceToHost, v->stream));
    HV_HIP(hipStreamSynchronize(v->stream));
    HV_REQUIRE(c[HV_DEINT_MISS_FULL] == 0, HV_ERR_CAPACITY,
               "hv_tsdf_deintegrate: more absent units than the table holds: the voxels were updated, units_missing is incomplete");
    stats->units_listed = (int64_t)c[HV_DEINT_LISTED];
    stats->units_missing = (int64_t)c[HV_DEINT_MISSING];
    stats->voxels_removed = (int64_t)c[HV_DEINT_REMOVED];
    stats->voxels_underflow = (int64_t)c[HV_DEINT_UNDERFLOW];
    return HV_OK;
}

extern "C" {

int hv_tsdf_deintegrate_batch(hv_volume *v, const void *depth, int32_t depth_dtype, const uint8_t *rgb, int32_t n_frames, int32_t height,
                              int32_t width, const double *intr, const double *T_cw, double depth_scale, double depth_trunc, int32_t loc,
                              hv_deintegrate_stats *stats) {
    int rc = check_deint_args(v, depth, rgb, height, width, intr, T_cw, n_frames);
    if (rc != HV_OK) return rc;
    HV_HIP(hipSetDevice(v->device));
    const void *d_depth = nullptr;
    const uint8_t *d_rgb = nullptr;
    rc = hv_stage_frame(v, depth, depth_dtype, rgb, (size_t)height * width * (size_t)n_frames, loc, &d_depth, &d_rgb);
    if (rc != HV_OK) return rc;
    rc = tsdf_deintegrate_device(v, d_depth, depth_dtype, d_rgb, n_frames, height, width, intr, T_cw, depth_scale, depth_trunc, true,
                                 stats != nullptr);
    if (rc != HV_OK || stats == nullptr) return rc;
    return deint_read_stats(v, stats);
}

int hv_tsdf_deintegrate(hv_volume *v, const void *depth, int32_t depth_dtype, const uint8_t *rgb, int32_t height, int32_t width,
                        const double *intr, const double *T_cw, double depth_scale, double depth_trunc, int32_t loc,
                        hv_deintegrate_stats *stats) {
    return hv_tsdf_deintegrate_batch(v, depth, depth_dtype, rgb, 1, height, width, intr, T_cw, depth_scale, depth_trunc, loc, stats);
}

int hv_tsdf_reintegrate_batch(hv_volume *v, const void *depth, int32_t depth_dtype, const uint8_t *rgb, int32_t n_frames, int32_t height,
                              int32_t width, const double *intr, const double *T_cw_old, const double *T_cw_new, double depth_scale,
                              double depth_trunc, int32_t loc, hv_deintegrate_stats *stats) {
    int rc = check_deint_args(v, depth, rgb, height, width, intr, T_cw_old, n_frames);
    if (rc != HV_OK) return rc;
    HV_REQUIRE(T_cw_new != nullptr, HV_ERR_INVALID, "[ScalableTSDFVolume::Integrate] Unsupported image format.");
    HV_HIP(hipSetDevice(v->device));
    const void *d_depth = nullptr;
    const uint8_t *d_rgb = nullptr;
    rc = hv_stage_frame(v, depth, depth_dtype, rgb, (size_t)height * width * (size_t)n_frames, loc, &d_depth, &d_rgb);
    if (rc != HV_OK) return rc;
    // the frames go through the camera's rectify maps once, for both halves (rect_buf holds all of them)
    rc = tsdf_rectify(v, v->stream, &d_depth, depth_dtype, &d_rgb, n_frames, height, width);
    if (rc != HV_OK) return rc;
    rc = tsdf_deintegrate_device(v, d_depth, depth_dtype, d_rgb, n_frames, height, width, intr, T_cw_old, depth_scale, depth_trunc, false,
                                 stats != nullptr);
    if (rc != HV_OK) return rc;
    // the integrate half: hv_tsdf_integrate_batch on the prepared device frames, with the maps switched off for the call
    const int32_t rect_W = v->rect_W;
    v->rect_W = 0;
    rc = tsdf_integrate_batch_impl(v, d_depth, nullptr, depth_dtype, d_rgb, nullptr, n_frames, height, width, intr, T_cw_new, depth_scale,
                                   depth_trunc, HV_DEVICE);
    v->rect_W = rect_W;
    if (rc != HV_OK || stats == nullptr) return rc;
    return deint_read_stats(v, stats);
}

} // extern "C"
