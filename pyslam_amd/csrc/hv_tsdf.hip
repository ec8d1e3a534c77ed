// libpyslam_hipvol.so — TSDF fusion kernels (Open3D ScalableTSDFVolume semantics) for gfx950.
//
// Online path, per frame (reference call site pyslam/dense/volumetric_integrator_tsdf.py:215-223):
//   k_tsdf_prep_touch   one launch, two block roles:
//       prep  blocks: depth -> float metres with depth_scale/depth_trunc applied
//                     (Image::ConvertDepthToFloatImage), RGB u8x3 packed: one 8-byte
//                     {depth, rgb} record per pixel (the sweep's per-voxel gather);
//       touch blocks: every `stride`-th pixel is back-projected in f64 and the volume units within
//                     +/- sdf_trunc are claimed in the block hash (ScalableTSDFVolume::Integrate
//                     front half), de-duplicated per wave; the first toucher of a unit this frame
//                     appends it to the touched list.
//   k_tsdf_integrate    one workgroup (4 waves) per touched unit; wave w owns z in [4w, 4w+4); lane
//                       (x, 4 y's).  Each z-slab of each plane is one contiguous 1 KiB dwordx4
//                       burst per wave.  Arithmetic follows UniformTSDFVolume::
//                       IntegrateWithDepthToCameraDistanceMultiplier operation by operation
//                       (compiled with -ffp-contract=off; IEEE div/sqrt) so tsdf and weight are
//                       bit-identical to the CPU restatement in oracle/tsdf_oracle.c.
//   HBM-bound: algorithmic bytes per touched unit = 4096 voxels * 20 B read (+ 20 B per updated
//   voxel written); no reuse of voxel data within a frame.  Frame gathers are served by L1/L2 (a
//   640x480 frame = 2.4 MB packed, resident in every XCD's 4 MiB L2).
// Multi-frame sweep (hv_tsdf_integrate_batch): k_tsdf_prep_touch_batch + k_tsdf_sweep_column (or k_tsdf_sweep, the bitwise form)
// further down — a unit's voxels stay in registers across up to 64 frames.
// Multi-GPU hooks: image-tile restriction (hv_tsdf_set_tile) and unit ownership (hv_tsdf_set_owner); the exchange of units between
// GPUs (numerators export / import, halo merge) is hv_halo.hip.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>
#include <numeric>

#include "hv_tsdf_device.h"

// The depth-to-camera-distance multiplier depends on the pixel and the intrinsics only: one table per (intrinsics,
// image size), rebuilt when they change, lets the multi-frame sweep replace ~20 VALU instructions (two conversions, the
// normalisation, a correctly rounded sqrt) per voxel visit by a 4-byte gather at the pixel index it already has.
__global__ __launch_bounds__(256) void k_tsdf_multiplier_table(HvFrameParams P, float *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.H * P.W) return;
    out[i] = hv_multiplier(P, i % P.W, i / P.W);
}


__global__ __launch_bounds__(256) void k_tsdf_prep_touch(HvTable table, int32_t *__restrict__ stamp,
                                                          int32_t *__restrict__ list, int parity,
                                                          const void *__restrict__ depth_raw,
                                                          const uint8_t *__restrict__ rgb,
                                                          uint2 *__restrict__ frame_px, HvFrameParams P,
                                                          int n_touch_blocks) {
    const int64_t npx = (int64_t)P.H * P.W;
    if ((int)blockIdx.x >= n_touch_blocks) { // touch blocks (latency chains) are dispatched first, the streaming prep blocks fill in
        // prep role: one 8-byte {depth f32, rgb packed} record per pixel so that the per-voxel
        // gather of the integrate kernel is a single dwordx2 load
        const int64_t i = (int64_t)((int)blockIdx.x - n_touch_blocks) * blockDim.x + threadIdx.x;
        if (i >= npx) return;
        const uint8_t *c = rgb + i * 3;
        uint2 rec;
        rec.x = __float_as_uint(hv_convert_depth(P, depth_raw, i));
        rec.y = hv_colour_order((uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16), P.bgr);
        frame_px[i] = rec;
        return;
    }
    // ---- touch role, online form: the launch is as long as its longest wave (a single frame has only ~300 patches:
    // nothing to hide a patch's chains behind), so the samples are fanned out instead - HV_TOUCH_FAN lanes per sample,
    // lane (sample, k0) handles the sample's units k0, k0 + FAN, ...: the (usually 8) hash inserts of one sample run in
    // parallel, every wave is ONE short chain, and 8 neighbouring samples are de-duplicated by ballot.  (Measured: 15 us
    // per frame against 28 us for the patch form, whose discontinuity patches walk several chains back to back; over
    // the 32 frames of a batch the patch form is the faster one: 83 vs 128 us.) ----
    const int ns_w = (P.W + P.stride - 1) / P.stride;
    const int ns_h = (P.H + P.stride - 1) / P.stride;
    const int tid = (int)blockIdx.x * blockDim.x + threadIdx.x;
    const int s = tid / HV_TOUCH_FAN;
    const int k0 = tid % HV_TOUCH_FAN;
    int32_t lo[3] = {0, 0, 0}, hi[3] = {-1, -1, -1}; // empty range for lanes without a valid sample
    if (s < ns_w * ns_h) {
        const int i = (s / ns_w) * P.stride;
        const int j = (s % ns_w) * P.stride;
        const float p = hv_convert_depth(P, depth_raw, (int64_t)i * P.W + j);
        if (p > 0.0f) {
            const double z = (double)p;
            const double x = ((double)j - P.cx_d) * z / P.fx_d;
            const double y = ((double)i - P.cy_d) * z / P.fy_d;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const double pw = ((P.pose[r * 4 + 0] * x + P.pose[r * 4 + 1] * y) + P.pose[r * 4 + 2] * z) + P.pose[r * 4 + 3];
                lo[r] = (int32_t)floor((pw - P.sdf_trunc_d) / P.unit_length);
                hi[r] = (int32_t)floor((pw + P.sdf_trunc_d) / P.unit_length);
            }
        }
    }
    const int64_t nx = (int64_t)hi[0] - lo[0] + 1, ny = (int64_t)hi[1] - lo[1] + 1, nz = (int64_t)hi[2] - lo[2] + 1;
    const int64_t count = (nx > 0 && ny > 0 && nz > 0) ? nx * ny * nz : 0;
    const int lane = hv_lane_id();
    for (int64_t k = k0; __any(k < count); k += HV_TOUCH_FAN) {
        unsigned long long key = HV_EMPTY_KEY;
        int32_t ux = 0, uy = 0, uz = 0;
        if (k < count) {
            ux = lo[0] + (int32_t)(k / (ny * nz));
            uy = lo[1] + (int32_t)((k / nz) % ny);
            uz = lo[2] + (int32_t)(k % nz);
            if (hv_key_in_range(ux, uy, uz)) {
                key = hv_pack_key(ux, uy, uz);
                // unit-ownership sharding: another GPU fuses (and stores) this unit
                if (P.owner_world > 1 && hv_owner_of(key, P.owner_world) != P.owner_rank) key = HV_EMPTY_KEY;
            } else {
                atomicAdd(&table.counters[HV_CNT_DROPPED], 1);
            }
        }
        // wave-level de-duplication: neighbouring samples hit the same units; only one lane per distinct key goes to
        // the hash (ballot + shuffle, no memory traffic)
        bool leader = false;
        unsigned long long remaining = __ballot(key != HV_EMPTY_KEY);
        while (remaining) {
            const int first = __ffsll((long long)remaining) - 1;
            const unsigned long long fkey = __shfl(key, first);
            const unsigned long long same = __ballot(key == fkey);
            if (lane == first) leader = true;
            remaining &= ~same;
        }
        // image-tile sharding: a unit none of whose voxels can project into this GPU's tile is neither allocated nor
        // stamped here (whole-image tile: always true) - so "stamped since the last merge" == "may hold updates"
        if (leader && hv_unit_hits_tile(P, ux, uy, uz)) {
            const int32_t slot = hv_table_insert(table, key);
            if (slot >= 0) {
                // L1-bypassing pre-check: most units were already stamped by another wave this frame
                if (__hip_atomic_load(&stamp[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != P.frame_id) {
                    const int32_t old = atomicExch(&stamp[slot], P.frame_id);
                    if (old != P.frame_id) {
                        const int32_t at = atomicAdd(&table.counters[HV_CNT_TOUCH(parity)], 1);
                        if (at < table.max_blocks) list[at] = slot;
                    }
                }
            }
        }
    }
}

// ZB z-slabs of one lane (ZB x 4 voxels).  Phase 1 evaluates every voxel (ZB*4 independent 8-byte
// gathers in flight, no voxel-plane traffic; predicated, the multiplier computed per visit: this kernel waits on memory, the table's
// extra gather costs more than the VALU work it saves - 8.5 k frames/s against 7.9 k, 6.2-7.2 k with a branching evaluation); phase 2
// read-modify-writes only the 16-byte pieces that hold an updated voxel.  pc[][] is advanced by ZB z-steps.
template <int ZB>
__device__ __forceinline__ void hv_tsdf_slabs(const HvFrameParams &P, const uint2 *__restrict__ frame_px, char *__restrict__ unit, int wordb,
                                              float (&pc)[4][3], float inc0, float inc1, float inc2) {
    float tv[ZB][4];
    uint32_t cv[ZB][4];
    unsigned mask = 0;
    // wave-uniform choice of the division form: columns that come within 1 mm of the camera plane on these ZB steps
    // (and tile-sharded frames) take the EXACT form
    bool near_plane = false;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const float e = pc[c][2] + (float)ZB * inc2;
        near_plane |= (int)(fminf(pc[c][2], e) < 0x1p-10f) & (int)(fmaxf(pc[c][2], e) > -0x1p-10f);
    }
    if (P.tiled || __any(near_plane)) {
#pragma unroll
        for (int zz = 0; zz < ZB; ++zz) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (hv_tsdf_eval_fast<true, false>(P, frame_px, nullptr, pc[c][0], pc[c][1], pc[c][2], tv[zz][c], cv[zz][c]))
                    mask |= 1u << (zz * 4 + c);
                pc[c][0] += inc0;
                pc[c][1] += inc1;
                pc[c][2] += inc2;
            }
        }
    } else {
#pragma unroll
        for (int zz = 0; zz < ZB; ++zz) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (hv_tsdf_eval_fast<false, false>(P, frame_px, nullptr, pc[c][0], pc[c][1], pc[c][2], tv[zz][c], cv[zz][c]))
                    mask |= 1u << (zz * 4 + c);
                pc[c][0] += inc0;
                pc[c][1] += inc1;
                pc[c][2] += inc2;
            }
        }
    }
    float4 vt[ZB];
    uint4 vw[ZB], vr[ZB], vg[ZB], vb[ZB];
#pragma unroll
    for (int zz = 0; zz < ZB; ++zz) {
        if ((mask >> (zz * 4)) & 15u) {
            const int q = (wordb + zz * HV_TSDF_RR) >> 2;
            vt[zz] = ((const float4 *)(unit + 0 * HV_TSDF_PLANE_BYTES))[q];
            vw[zz] = ((const uint4 *)(unit + 1 * HV_TSDF_PLANE_BYTES))[q];
            vr[zz] = ((const uint4 *)(unit + 2 * HV_TSDF_PLANE_BYTES))[q];
            vg[zz] = ((const uint4 *)(unit + 3 * HV_TSDF_PLANE_BYTES))[q];
            vb[zz] = ((const uint4 *)(unit + 4 * HV_TSDF_PLANE_BYTES))[q];
        }
    }
#pragma unroll
    for (int zz = 0; zz < ZB; ++zz) {
        const unsigned m = (mask >> (zz * 4)) & 15u;
        if (m) {
            hv_tsdf_apply(m & 1u, tv[zz][0], cv[zz][0], vt[zz].x, vw[zz].x, vr[zz].x, vg[zz].x, vb[zz].x);
            hv_tsdf_apply(m & 2u, tv[zz][1], cv[zz][1], vt[zz].y, vw[zz].y, vr[zz].y, vg[zz].y, vb[zz].y);
            hv_tsdf_apply(m & 4u, tv[zz][2], cv[zz][2], vt[zz].z, vw[zz].z, vr[zz].z, vg[zz].z, vb[zz].z);
            hv_tsdf_apply(m & 8u, tv[zz][3], cv[zz][3], vt[zz].w, vw[zz].w, vr[zz].w, vg[zz].w, vb[zz].w);
            const int q = (wordb + zz * HV_TSDF_RR) >> 2;
            ((float4 *)(unit + 0 * HV_TSDF_PLANE_BYTES))[q] = vt[zz];
            ((uint4 *)(unit + 1 * HV_TSDF_PLANE_BYTES))[q] = vw[zz];
            ((uint4 *)(unit + 2 * HV_TSDF_PLANE_BYTES))[q] = vr[zz];
            ((uint4 *)(unit + 3 * HV_TSDF_PLANE_BYTES))[q] = vg[zz];
            ((uint4 *)(unit + 4 * HV_TSDF_PLANE_BYTES))[q] = vb[zz];
        }
    }
}

// The online sweep: evaluate first - predicated, all gathers of a lane in flight -, then fetch only the pieces that are updated.
// (The roofline ablations of rounds 1-2 - no plane traffic / plane traffic only - are recorded in profiles/r01, r02.)
__global__ __launch_bounds__(256) void k_tsdf_integrate(HvTable table, const int32_t *__restrict__ list,
                                                         int parity, char *__restrict__ pool,
                                                         const uint2 *__restrict__ frame_px, HvFrameParams P,
                                                         HvStatus *status, int32_t status_seq) {
    int n_touched = table.counters[HV_CNT_TOUCH(parity)];
    if (n_touched > table.max_blocks) n_touched = table.max_blocks;
    // the next frame's touch pass appends to the other parity's counter: zero it here (stream order); the pool occupancy
    // this frame's touch pass left goes to the host-visible status word (hv_capacity_gate reads it before the next call)
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        table.counters[HV_CNT_TOUCH(parity ^ 1)] = 0;
        hv_publish_status(table, status, status_seq);
    }
    const int wave = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    const int x = lane >> 2;
    const int y0 = (lane & 3) << 2;
    const int z0 = wave * 4;
    const float inc0 = P.ext_scaled_col2[0], inc1 = P.ext_scaled_col2[1], inc2 = P.ext_scaled_col2[2];

    for (int t = blockIdx.x; t < n_touched; t += gridDim.x) {
        const int32_t slot = list[t];
        const int32_t idx = table.vals[slot];
        if (idx < 0) continue;
        int32_t ux, uy, uz;
        hv_unpack_key(table.keys[slot], ux, uy, uz);
        const double o0 = (double)ux * P.unit_length;
        const double o1 = (double)uy * P.unit_length;
        const double o2 = (double)uz * P.unit_length;
        const float p0 = (float)((double)(P.half_voxel_length_f + P.voxel_length_f * (float)x) + o0);
        const float p2 = (float)((double)P.half_voxel_length_f + o2);
        float pc[4][3];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const float p1 = (float)((double)(P.half_voxel_length_f + P.voxel_length_f * (float)(y0 + c)) + o1);
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                pc[c][r] = ((P.ext[r * 4 + 0] * p0 + P.ext[r * 4 + 1] * p1) + P.ext[r * 4 + 2] * p2) + P.ext[r * 4 + 3];
            }
        }
        // the reference advances pt_camera by repeated float additions along z: replay them so the
        // wave that starts at z0 holds bit-identical values
        for (int s = 0; s < z0; ++s) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                pc[c][0] += inc0;
                pc[c][1] += inc1;
                pc[c][2] += inc2;
            }
        }
        char *unit = pool + (int64_t)idx * HV_TSDF_UNIT_BYTES;
        // 2 z-slabs evaluated per batch: (107 VGPRs, 4 waves/SIMD) measured 7269 frames/s vs 6342 for 4
        // (180 VGPRs, 2 waves/SIMD) on the headline config
        constexpr int ZB = 2;
#pragma unroll
        for (int zb = 0; zb < 4; zb += ZB) hv_tsdf_slabs<ZB>(P, frame_px, unit, hv_tsdf_word(x, y0, z0 + zb), pc, inc0, inc1, inc2);
    }
}

// Touch role of the multi-frame path: one wave = one 8x8 patch of frame f's depth samples; every distinct unit the patch opens gets
// bit f of its frame mask and - at its first touch in the batch - its place in the batch's union list.
__device__ __forceinline__ void hv_touch_batch_patch(const HvTable &table, const HvFrameParams &P, const void *depth_f, const int patch,
                                                     HvTouchScratch &scratch, const int f, unsigned long long *__restrict__ frame_mask,
                                                     int32_t *__restrict__ stamp, int32_t *__restrict__ list, const int batch_stamp,
                                                     const int parity) {
    const unsigned long long fbit = 1ull << f;
    hv_touch_patch(table, P, depth_f, patch, scratch,
                   [&](unsigned long long key, int32_t ux, int32_t uy, int32_t uz) {
                       // image-tile sharding: units that cannot project into this GPU's tile are not allocated here
                       if (!hv_unit_hits_tile(P, ux, uy, uz)) return;
                       const int32_t slot = hv_table_insert(table, key);
                       if (slot < 0) return;
                       // both L1-bypassing pre-checks in flight together
                       const unsigned long long seen = __hip_atomic_load(&frame_mask[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                       const int32_t stamped = __hip_atomic_load(&stamp[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                       // frame bit (skip the atomic when another wave of this frame already set it)
                       if (!(seen & fbit)) atomicOr(&frame_mask[slot], fbit);
                       if (stamped != batch_stamp) {
                           const int32_t old = atomicExch(&stamp[slot], batch_stamp);
                           if (old != batch_stamp) {
                               const int32_t at = atomicAdd(&table.counters[HV_CNT_TOUCH(parity)], 1);
                               if (at < table.max_blocks) list[at] = slot;
                           }
                       }
                   });
}

// ================================================================================================
// Multi-frame sweep (hv_tsdf_integrate_batch; the rebuild()/offline-replay use case,
// volumetric_integrator_base.py:1242-1318).  B <= 64 posed frames are resident in HBM:
//   k_tsdf_prep_touch_batch  one launch for all B frames: packs every frame (a pack thread writes the records of its 4
//                            pixels for HV_PACK_FRAMES consecutive frames, all of their loads in flight before the first
//                            wait: hv_pack_px4_frames) and ORs bit f into the 64-bit frame mask of each unit frame f
//                            touches (one wave per 8x8 sample patch, hv_touch_patch); the first toucher of a unit in the
//                            batch appends it to the union list
//   sweep                    per union unit: a lane's voxels are folded over every frame bit in ascending (= chronological) order
//                            in registers and stored once - k_tsdf_sweep_column (production) or k_tsdf_sweep (bitwise)
//   k_tsdf_batch_finish      clears the batch's frame masks and list counter
// Identical results to B successive hv_tsdf_integrate calls: a unit is updated by frame f iff frame
// f touched it, and its frames are applied in order.  Plane traffic per frame drops by ~B x (the
// union of 32 consecutive frames' units is ~1.6x one frame's); what remains is the per-voxel math
// and the frame gathers.
// (Rounds 2-5 also carried a first column form, a 4-voxels-per-lane fold form, a launch fused with the next batch's touch + pack pass,
// a longest-task-first list order, a third scratch set and an image-coherent ownership plan; each measured slower than or equal to
// what is kept - profiles/r02 .. r05, sweep_forms.jsonl, pipeline_experiments.md, simulate_ranks_coherent.jsonl - and taken out in
// round 6.)
// ================================================================================================
__global__ __launch_bounds__(256) void k_tsdf_prep_touch_batch(HvTable table, int32_t *__restrict__ stamp,
                                                                unsigned long long *__restrict__ frame_mask,
                                                                int32_t *__restrict__ list, int batch_stamp,
                                                                const char *__restrict__ depth_raw, int64_t depth_stride,
                                                                const uint8_t *__restrict__ rgb,
                                                                uint2 *__restrict__ frame_px,
                                                                const HvFrameParams *__restrict__ Ps, int n_prep_blocks,
                                                                int n_touch_blocks, int n_frames, int parity,
                                                                const float *__restrict__ mult12) {
    // block order: the touch blocks of ALL frames first, then the pack blocks.  A touch wave is one chain of dependent
    // memory round trips (depth -> hash probe -> mask / stamp -> atomics; a patch on a long depth discontinuity walks
    // several such chains), the pack blocks are pure streaming: dispatched last they fill the machine while the touch
    // chains drain, instead of the launch ending on the chains of the last frame.
    __shared__ __attribute__((aligned(16))) HvTouchScratch scratch[4]; // per wave: the touch role's bitmap and list, the pack role's stage
    static_assert(sizeof(HvTouchScratch) >= HV_WAVE * 48, "a wave stages 64 x 4 records of 12 bytes");
    if ((int)blockIdx.x >= n_touch_blocks * n_frames) {
        // ---- pack role: a thread packs the same pixel quads of the HV_PACK_FRAMES consecutive frames of its group ----
        // (everything the pack reads from a frame's constants - image size, depth type and scale, colour order, tile - is the
        // same for every frame of a batch: the group's first frame stands for all of them)
        const int b = (int)blockIdx.x - n_touch_blocks * n_frames;
        const int f0 = (b / n_prep_blocks) * HV_PACK_FRAMES;
        const int nf = min(HV_PACK_FRAMES, n_frames - f0);
        const HvFrameParams &P = Ps[f0];
        const int64_t npx = (int64_t)P.H * P.W;
        const int64_t i0 = ((int64_t)(b % n_prep_blocks) * blockDim.x + threadIdx.x) * 4; // (prep blocks cover 1024 pixels each)
        if (mult12 != nullptr && (npx & 3) == 0 && nf == HV_PACK_FRAMES && i0 < npx) {
            if (P.tiled && (P.W & 3) == 0) { // as hv_pack_px4: only the tile's rows and columns (+ 4 pixels) are packed
                const int u = (int)(i0 % P.W), v = (int)(i0 / P.W);
                if (u + 3 < P.tile_u0 - 4 || u >= P.tile_u1 + 4 || v < P.tile_v0 - 4 || v >= P.tile_v1 + 4) return;
            }
            // every choice a wave makes as one is made here, outside the load sequence
            uint4 *stage = (uint4 *)&scratch[threadIdx.x / HV_WAVE];
            const bool whole_wave = __ballot(1) == ~0ull;
            if (P.depth_is_u16) {
                if (whole_wave) hv_pack_px4_frames<true, true>(P, f0, i0, depth_raw, depth_stride, rgb, frame_px, mult12, stage);
                else hv_pack_px4_frames<true, false>(P, f0, i0, depth_raw, depth_stride, rgb, frame_px, mult12, nullptr);
            } else {
                if (whole_wave) hv_pack_px4_frames<false, true>(P, f0, i0, depth_raw, depth_stride, rgb, frame_px, mult12, stage);
                else hv_pack_px4_frames<false, false>(P, f0, i0, depth_raw, depth_stride, rgb, frame_px, mult12, nullptr);
            }
            return;
        }
        // the ragged last group of a batch, 8-byte records, an image that is no whole number of quads: frame by frame
        for (int k = 0; k < nf; ++k)
            hv_pack_px4(P, f0 + k, i0, depth_raw + (int64_t)(f0 + k) * depth_stride, rgb + (int64_t)(f0 + k) * npx * 3, frame_px, mult12);
        return;
    }
    const int f = (int)blockIdx.x / n_touch_blocks;
    const int bx = (int)blockIdx.x % n_touch_blocks;
    const HvFrameParams &P = Ps[f];
    const void *depth_f = depth_raw + (int64_t)f * depth_stride;
    // ---- touch role: one wave per 8x8 sample patch (hv_touch_patch) ----
    const int patch = bx * 4 + (int)(threadIdx.x / HV_WAVE);
    if (patch < hv_touch_patches(P))
        hv_touch_batch_patch(table, P, depth_f, patch, scratch[threadIdx.x / HV_WAVE], f, frame_mask, stamp, list, batch_stamp, parity);
}

// ================================================================================================
// Sweep, BITWISE form (HV_TSDF_SWEEP=2; the production form further down folds a batch per voxel and is not bitwise).  Lane = one
// voxel column, wave = 64 columns x 4 z, frames applied in order in registers with the reference's running mean after every frame:
// tsdf, weight and colour bit-identical to B successive online frames and to the oracle.  What the form does about instructions:
//  * the (u, v) projection chain is written on float2 values of ONE voxel ((pc0, pc1) walk, (a0, a1) / pc2 with the
//    refined reciprocal broadcast): v_pk_* instructions;
//  * gathers go through raw buffer descriptors (out-of-range offsets return 0: garbage lanes need no select), the pixel
//    index is a 24-bit mad;
//  * what does not depend on the frame (intrinsics, image size, truncation) is read once per work item, the 16 dwords
//    that do (extrinsics and the z step) are fetched one frame AHEAD into scalar registers;
//  * the near-camera-plane regime is detected once per work item (lane f tests frame f) and routes the whole item to the EXACT loop;
//  * the running mean of a voxel pair is skipped when no lane of the wave updates either voxel;
//  * colour is accumulated in two packed registers per voxel (16-bit r and b fields, g in bits 8..23: <= 64 frames x 255
//    fit) and the three colour planes are only loaded for the final add of voxels that were updated.
// Measured (profiles/r02): 31.4 k frames/s at 128 VGPRs / 4 waves per SIMD.
// ================================================================================================
typedef float hv_f2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ hv_f2 hv_fma2(hv_f2 a, hv_f2 b, hv_f2 c) { return __builtin_elementwise_fma(a, b, c); }
__device__ __forceinline__ hv_f2 hv_splat(float x) { return hv_f2{x, x}; }

struct HvSweepFrameK { // HvFrameParams::sweep_k in registers (plain members: the two prefetch sets must live in scalar registers)
    hv_f2 e04, e15, e26, e37;
    float e8, e11;
    hv_f2 e9_10, i01;
    float i2;
};
__device__ __forceinline__ HvSweepFrameK hv_sweep_frame_k(const HvFrameParams *__restrict__ Ps, int f) {
    const float *k = Ps[f].sweep_k;
    return HvSweepFrameK{hv_f2{k[0], k[1]}, hv_f2{k[2], k[3]}, hv_f2{k[4], k[5]}, hv_f2{k[6], k[7]}, k[8], k[9], hv_f2{k[10], k[11]}, hv_f2{k[12], k[13]}, k[14]};
}

// Work items -> workgroups, for both sweep kernels.  A unit is `parts` work items (one workgroup each).  Workgroup b runs on XCD
// b % 8 and every XCD has its own L2; the union list is in touch order, i.e. roughly in image raster order of the first frames.  The
// parts of a unit (which read the same depth pixels in every frame) and G consecutive list entries stay on one XCD: item i -> XCD
// i & 7, and within that XCD entries (8 g + xcd) G .. + G - 1 of the list for g = 0, 1, ... - the XCD's L2 holds one band of the
// frame records instead of every XCD pulling every frame whole (profiles/r02/baseline: 2.0x the algorithmic traffic).  G small
// enough that a heavy stretch of the list is spread over all XCDs: G = 2 measured best, +2.5 %, FETCH_SIZE halves; one contiguous
// eighth of the list per XCD halves the traffic too but is 28 % slower, the dispatcher waits for the heaviest XCD.
// hv_sweep_items: the number of work items (the list is run in whole rounds of 8 G entries); hv_sweep_item: item -> list entry t
// and part of it.  t >= n_units: a padding item of the last round, nothing to run.
static constexpr unsigned HV_SWEEP_XCD_GROUP = 2; // G
__device__ __forceinline__ int hv_sweep_items(const int n_units, const int parts) {
    constexpr int G = HV_SWEEP_XCD_GROUP;
    return (n_units + 8 * G - 1) / (8 * G) * 8 * G * parts;
}
__device__ __forceinline__ void hv_sweep_item(const unsigned item, const unsigned parts, int &t, int &part) {
    constexpr unsigned G = HV_SWEEP_XCD_GROUP; // (unsigned throughout: G and parts are powers of two, the mapping is shifts and masks)
    const unsigned xcd = item & 7u, j = item >> 3;
    const unsigned g = j / (G * parts), within = j % (G * parts);
    t = (int)((g * 8 + xcd) * G + within / parts);
    part = (int)(within % parts);
}

// Epilogue of a sweep item: the plane words of a lane's updated voxels, read-modify-written in PASSES of ZB voxels along z.
// A pass first issues every plane load of its updated voxels (TW: tsdf and weight too, else only the three colour sums), waits for
// them ONCE, and then runs voxel by voxel: `finish(z, w)` turns the loaded words into the words to store, the five stores follow in
// plane order with no wait between them.  A wave so pays about one memory round trip per pass; written voxel by voxel (`+=` on
// the colour planes inside each voxel's block) it paid one per voxel, the loads of voxel k + 1 counted behind the stores of voxel
// k (gfx9: one vmcnt for both), plus one per four voxels for tsdf and weight.  `updated(z)` is the lane's own condition, the same in both halves
// of a pass: a lane with nothing to add touches no word, and a z plane no lane updates is skipped by the execz branch - no traffic
// is added.  The wait is explicit because the compiler cannot see that the two halves run under the same condition: left to place
// the waits itself it puts one in front of every store ("the load into this register may still be pending"), which counts the
// stores before it too.
// (Compiled and dropped, profiles/sweep_epilogue: passes of 8 voxels - whole columns keep 128 registers with 1 spilled outside the
// frame loop and measure the same as passes of 4, z halves spill 36; passes of 16 - 181 spilled; the loads of pass p + 1 issued
// before the stores of pass p, two word sets alternating - 28 spilled and a longer frame loop.)
static constexpr int HV_WAIT_VMCNT0 = 0x0f70; // s_waitcnt vmcnt(0), expcnt and lgkmcnt left at their maxima (gfx9 encoding)
struct HvPlaneWords {
    float vt;
    uint32_t vw, r, g, b;
};
template <int ZH, int ZB, bool TW, typename Updated, typename Finish>
__device__ __forceinline__ void hv_sweep_epilogue(char *__restrict__ unit, const int wordb, Updated updated, Finish finish) {
    constexpr int NP = ZH / ZB;
    static_assert(ZH % ZB == 0, "whole passes");
    auto load = [&](const int p, HvPlaneWords (&w)[ZB]) __attribute__((always_inline)) {
#pragma unroll
        for (int k = 0; k < ZB; ++k) {
            const int z = p * ZB + k;
            if (updated(z)) {
                const int q = wordb + z * HV_TSDF_RR;
                if (TW) {
                    w[k].vt = ((const float *)(unit + 0 * HV_TSDF_PLANE_BYTES))[q];
                    w[k].vw = ((const uint32_t *)(unit + 1 * HV_TSDF_PLANE_BYTES))[q];
                }
                w[k].r = ((const uint32_t *)(unit + 2 * HV_TSDF_PLANE_BYTES))[q];
                w[k].g = ((const uint32_t *)(unit + 3 * HV_TSDF_PLANE_BYTES))[q];
                w[k].b = ((const uint32_t *)(unit + 4 * HV_TSDF_PLANE_BYTES))[q];
            }
        }
    };
    auto store = [&](const int p, const HvPlaneWords (&w)[ZB]) __attribute__((always_inline)) {
#pragma unroll
        for (int k = 0; k < ZB; ++k) {
            const int z = p * ZB + k;
            if (updated(z)) {
                const int q = wordb + z * HV_TSDF_RR;
                HvPlaneWords o = w[k];
                finish(z, o);
                ((float *)(unit + 0 * HV_TSDF_PLANE_BYTES))[q] = o.vt;
                ((uint32_t *)(unit + 1 * HV_TSDF_PLANE_BYTES))[q] = o.vw;
                ((uint32_t *)(unit + 2 * HV_TSDF_PLANE_BYTES))[q] = o.r;
                ((uint32_t *)(unit + 3 * HV_TSDF_PLANE_BYTES))[q] = o.g;
                ((uint32_t *)(unit + 4 * HV_TSDF_PLANE_BYTES))[q] = o.b;
            }
        }
    };
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        HvPlaneWords w[ZB];
        load(p, w);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_waitcnt(HV_WAIT_VMCNT0);
        store(p, w);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// the bitwise form's shape: a lane owns ZH voxels along z, a wave 64 columns x ZH z = one of a unit's 64 / ZH tasks
static constexpr int HV_SWEEP_ZH = 4;
static constexpr int HV_SWEEP_SPLIT = 8; // workgroups per unit
static constexpr int HV_SWEEP_WAVES = 64 / HV_SWEEP_ZH / HV_SWEEP_SPLIT; // waves per workgroup
static constexpr int HV_SWEEP_WPE = 4;   // waves per SIMD the kernel is compiled for
static_assert(HV_SWEEP_ZH % 2 == 0, "voxels are folded in pairs");

struct HvSweepGather { // what a frame's evaluation leaves for its fold: the gathered records, multipliers, depths along z, tests
    uint2 rec[HV_SWEEP_ZH];
    float mm[HV_SWEEP_ZH], zk[HV_SWEEP_ZH];
    bool ok[HV_SWEEP_ZH];
};

__global__ __launch_bounds__(64 * HV_SWEEP_WAVES, HV_SWEEP_WPE) void k_tsdf_sweep(
    HvTable table, const int32_t *__restrict__ list, const unsigned long long *__restrict__ frame_mask,
    char *__restrict__ pool, const uint2 *__restrict__ frame_px, const HvFrameParams *__restrict__ Ps, int n_frames,
    int general, const float *__restrict__ mult, int parity) {
    constexpr int ZH = HV_SWEEP_ZH, SPLIT = HV_SWEEP_SPLIT, WAVES = HV_SWEEP_WAVES;
    int n_units = table.counters[HV_CNT_TOUCH(parity)];
    if (n_units > table.max_blocks) n_units = table.max_blocks;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    // frame-independent constants (one camera and one volume per batch)
    const HvFrameParams &P0 = Ps[0];
    const float vl = P0.voxel_length_f, hl = P0.half_voxel_length_f;
    const double unit_length = P0.unit_length;
    const bool tiled = P0.tiled != 0;
    const int npx = P0.H * P0.W;
    const hv_f2 F = {P0.fx, P0.fy}, C = {P0.cx, P0.cy};
    const uint32_t lo = __float_as_uint(0.0001f);
    const uint32_t wlim = __float_as_uint(P0.safe_width_f) - lo, hlim = __float_as_uint(P0.safe_height_f) - lo;
    const uint32_t W24 = (uint32_t)P0.W;
    const float ntrunc = -P0.sdf_trunc_f, tinv = P0.sdf_trunc_inv_f;
    const __amdgpu_buffer_rsrc_t rs_m = __builtin_amdgcn_make_buffer_rsrc((void *)mult, 0, npx * 4, 0x00020000);
    const int n_items = hv_sweep_items(n_units, SPLIT);
    for (int item = blockIdx.x; item < n_items; item += gridDim.x) {
        int t, part;
        hv_sweep_item(item, SPLIT, t, part);
        if (t >= n_units) continue;
        const int task = part * WAVES + wave;
        const int cg = task & 3;            // column group: x in [4 cg, 4 cg + 4)
        const int z0 = (task >> 2) * ZH;
        const int x = cg * 4 + (lane >> 4);
        const int y = lane & 15;
        const int32_t slot = list[t];
        const int32_t idx = table.vals[slot];
        unsigned long long mask = frame_mask[slot];
        if (idx < 0 || mask == 0ull) continue;
        int32_t ux, uy, uz;
        hv_unpack_key(table.keys[slot], ux, uy, uz);
        const double o0 = (double)ux * unit_length, o1 = (double)uy * unit_length, o2 = (double)uz * unit_length;
        // lane f <-> frame f: does the box of this wave's voxel centres come within 3 cm of frame f's camera plane?  Then a
        // voxel may leave the band the short division chain is verified for (pc2 >= 2^-20 where pc2 > 0) and the whole
        // item takes the EXACT loop (rare: a frame only has a unit in its mask when it sees a surface within sdf_trunc of it)
        bool near = false;
        if (lane < n_frames && ((mask >> lane) & 1ull)) {
            const HvFrameParams &Pl = Ps[lane];
            const float bx = (float)((double)(hl + vl * (float)(cg * 4)) + o0), by = (float)((double)hl + o1),
                        bz = (float)((double)(hl + vl * (float)z0) + o2);
            const float zmin = (Pl.ext[8] * bx + Pl.ext[9] * by + Pl.ext[10] * bz + Pl.ext[11]) + fminf(Pl.ext[8] * (3.0f * vl), 0.f) +
                               fminf(Pl.ext[9] * (15.0f * vl), 0.f) + fminf(Pl.ext[10] * ((float)(ZH - 1) * vl), 0.f);
            near = !(zmin > 0.03f);
        }
        const bool near_any = __any(near);
        char *unit = pool + (int64_t)idx * HV_TSDF_UNIT_BYTES;
        const int wordb = z0 * HV_TSDF_RR + cg * 64 + lane;
        float vt[ZH];
        uint32_t vw[ZH];
#pragma unroll
        for (int zz = 0; zz < ZH; ++zz) {
            const int q = wordb + zz * HV_TSDF_RR;
            vt[zz] = ((const float *)(unit + 0 * HV_TSDF_PLANE_BYTES))[q];
            vw[zz] = ((const uint32_t *)(unit + 1 * HV_TSDF_PLANE_BYTES))[q];
        }
        // the voxel centre of (x, y, z = 0) does not depend on the frame
        const float p0 = (float)((double)(hl + vl * (float)x) + o0);
        const float p1 = (float)((double)(hl + vl * (float)y) + o1);
        const float p2 = (float)((double)hl + o2);
        bool heavy = false; // a voxel near 2^24 observations: float weights would stop being exact
#pragma unroll
        for (int zz = 0; zz < ZH; ++zz) heavy |= vw[zz] >= (1u << 24) - 64u;
        unsigned dirty = 0;
        if (general || tiled || near_any || __any(heavy)) {
            // rare regimes: EXACT evaluation with integer weights, frame by frame (the first form's code)
            uint32_t vr[ZH], vg[ZH], vb[ZH];
#pragma unroll
            for (int zz = 0; zz < ZH; ++zz) {
                const int q = wordb + zz * HV_TSDF_RR;
                vr[zz] = ((const uint32_t *)(unit + 2 * HV_TSDF_PLANE_BYTES))[q];
                vg[zz] = ((const uint32_t *)(unit + 3 * HV_TSDF_PLANE_BYTES))[q];
                vb[zz] = ((const uint32_t *)(unit + 4 * HV_TSDF_PLANE_BYTES))[q];
            }
            while (mask) {
                const int f = __ffsll((long long)mask) - 1;
                mask &= mask - 1;
                const HvFrameParams &P = Ps[f];
                const uint2 *px = frame_px + (int64_t)f * npx;
                const float inc0 = P.ext_scaled_col2[0], inc1 = P.ext_scaled_col2[1], inc2 = P.ext_scaled_col2[2];
                float pc0 = ((P.ext[0] * p0 + P.ext[1] * p1) + P.ext[2] * p2) + P.ext[3];
                float pc1 = ((P.ext[4] * p0 + P.ext[5] * p1) + P.ext[6] * p2) + P.ext[7];
                float pc2 = ((P.ext[8] * p0 + P.ext[9] * p1) + P.ext[10] * p2) + P.ext[11];
                for (int s = 0; s < z0; ++s) { // the reference's repeated float additions along z, replayed
                    pc0 += inc0;
                    pc1 += inc1;
                    pc2 += inc2;
                }
#pragma unroll
                for (int zz = 0; zz < ZH; ++zz) {
                    float tv;
                    uint32_t cv;
                    const bool ok = hv_tsdf_eval_fast<true, true>(P, px, mult, pc0, pc1, pc2, tv, cv);
                    pc0 += inc0;
                    pc1 += inc1;
                    pc2 += inc2;
                    hv_tsdf_apply(ok, tv, cv, vt[zz], vw[zz], vr[zz], vg[zz], vb[zz]);
                    if (ok) dirty |= 1u << zz;
                }
            }
#pragma unroll
            for (int zz = 0; zz < ZH; ++zz) {
                if (dirty & (1u << zz)) {
                    const int q = wordb + zz * HV_TSDF_RR;
                    ((float *)(unit + 0 * HV_TSDF_PLANE_BYTES))[q] = vt[zz];
                    ((uint32_t *)(unit + 1 * HV_TSDF_PLANE_BYTES))[q] = vw[zz];
                    ((uint32_t *)(unit + 2 * HV_TSDF_PLANE_BYTES))[q] = vr[zz];
                    ((uint32_t *)(unit + 3 * HV_TSDF_PLANE_BYTES))[q] = vg[zz];
                    ((uint32_t *)(unit + 4 * HV_TSDF_PLANE_BYTES))[q] = vb[zz];
                }
            }
            continue;
        }
        hv_f2 VT[ZH / 2], WF[ZH / 2];
        uint32_t arb[ZH], ag[ZH]; // colour of the batch: r | b << 16 and g << 8
#pragma unroll
        for (int zp = 0; zp < ZH / 2; ++zp) {
            VT[zp] = hv_f2{vt[2 * zp], vt[2 * zp + 1]};
            WF[zp] = hv_f2{(float)vw[2 * zp], (float)vw[2 * zp + 1]};
            arb[2 * zp] = arb[2 * zp + 1] = ag[2 * zp] = ag[2 * zp + 1] = 0u;
        }
        // One frame folded into the registers; K = the frame's 16 constant dwords, already in scalar registers.
        auto project_frame = [&](const HvSweepFrameK K, const int f, HvSweepFrameK &Knext, const unsigned long long rest,
                                 HvSweepGather &g) __attribute__((always_inline)) {
            const __amdgpu_buffer_rsrc_t rs_px = __builtin_amdgcn_make_buffer_rsrc((void *)(frame_px + (int64_t)f * npx), 0, npx * 8, 0x00020000);
            const hv_f2 INC = K.i01;
            const float inc2 = K.i2;
            // pc = ((e0 p0 + e1 p1) + e2 p2) + e3, rows 0 and 1 as one float2 (same IEEE ops as the reference)
            hv_f2 XY = ((K.e04 * p0 + K.e15 * p1) + K.e26 * p2) + K.e37;
            const hv_f2 Z12 = K.e9_10 * hv_f2{p1, p2};
            float Z = ((K.e8 * p0 + Z12.x) + Z12.y) + K.e11;
            // K is consumed (the wait for its scalar loads sits above): only now issue the loads of the next frame's constants,
            // so that wait does not include them (scalar loads return out of order: there is only "wait for all")
            __builtin_amdgcn_sched_barrier(0);
            Knext = hv_sweep_frame_k(Ps, rest ? __ffsll((long long)rest) - 1 : f); // (the last frame re-reads itself: no branch, the order above holds)
            __builtin_amdgcn_sched_barrier(0);
            for (int s = 0; s < z0; ++s) { // the reference's repeated float additions along z, replayed
                XY += INC;
                Z += inc2;
            }
            // ---- evaluation of the ZH voxels: all 2 ZH gathers in flight ----
#pragma unroll
            for (int k = 0; k < ZH; ++k) {
                // (a0, a1) / pc2, correctly rounded, sharing one refined reciprocal (hv_div2's chain on a float2)
                float r = __builtin_amdgcn_rcpf(Z);
                const float e = fmaf(-Z, r, 1.0f);
                r = fmaf(e, r, r);
                const hv_f2 A = XY * F;
                const hv_f2 R = hv_splat(r), NZ = hv_splat(-Z);
                hv_f2 Q = A * R;
                hv_f2 REM = hv_fma2(NZ, Q, A);
                Q = hv_fma2(REM, R, Q);
                REM = hv_fma2(NZ, Q, A);
                Q = hv_fma2(REM, R, Q);
                const hv_f2 UV = (Q + C) + hv_splat(0.5f);
                // u_f in [0.0001, safe_width) as ONE unsigned compare (bit patterns of non-negative floats order like the values)
                const bool in_u = (__float_as_uint(UV.x) - lo) < wlim;
                const bool in_v = (__float_as_uint(UV.y) - lo) < hlim;
                g.ok[k] = (int)(Z > 0.0f) & (int)in_u & (int)in_v;
                const uint32_t u = (uint32_t)(int)UV.x, v = (uint32_t)(int)UV.y; // saturating conversions: garbage lanes stay defined
                const uint32_t off = __umul24(v, W24) + u; // exact for every in-image pixel; a garbage lane reads 0 or some pixel, unused
                g.rec[k] = __builtin_bit_cast(uint2, __builtin_amdgcn_raw_buffer_load_b64(rs_px, (int)(off << 3), 0, 0));
                g.mm[k] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_m, (int)(off << 2), 0, 0));
                g.zk[k] = Z;
                XY += INC;
                Z += inc2;
            }
        };
        // ---- fold of an evaluated frame, two voxels at a time ----
        auto apply_frame = [&](const HvSweepGather &g) __attribute__((always_inline)) {
#pragma unroll
            for (int zp = 0; zp < ZH / 2; ++zp) {
                const int k0 = 2 * zp, k1 = 2 * zp + 1;
                const float da = __uint_as_float(g.rec[k0].x), db = __uint_as_float(g.rec[k1].x);
                const float sa = (da - g.zk[k0]) * g.mm[k0], sb = (db - g.zk[k1]) * g.mm[k1];
                const bool oka = (int)g.ok[k0] & (int)(da > 0.0f) & (int)(sa > ntrunc);
                const bool okb = (int)g.ok[k1] & (int)(db > 0.0f) & (int)(sb > ntrunc);
                if (!__any((int)oka | (int)okb)) continue; // no lane of the wave updates either voxel
                const hv_f2 T = {fminf(sa * tinv, 1.0f), fminf(sb * tinv, 1.0f)}; // == `if (t > 1) t = 1` for the non-NaN t of an accepted voxel
                // running mean (tsdf * w + t) / (w + 1) with float weights (exact below 2^24), hv_div1's chain on a float2
                const hv_f2 W1 = WF[zp] + hv_splat(1.0f);
                const hv_f2 NUM = VT[zp] * WF[zp] + T;
                hv_f2 R = {__builtin_amdgcn_rcpf(W1.x), __builtin_amdgcn_rcpf(W1.y)};
                const hv_f2 E = hv_fma2(-W1, R, hv_splat(1.0f));
                R = hv_fma2(E, R, R);
                hv_f2 Q = NUM * R;
                hv_f2 REM = hv_fma2(-W1, Q, NUM);
                Q = hv_fma2(REM, R, Q);
                REM = hv_fma2(-W1, Q, NUM);
                Q = hv_fma2(REM, R, Q);
                VT[zp].x = oka ? Q.x : VT[zp].x;
                VT[zp].y = okb ? Q.y : VT[zp].y;
                WF[zp].x = oka ? W1.x : WF[zp].x;
                WF[zp].y = okb ? W1.y : WF[zp].y;
                const uint32_t ca = oka ? g.rec[k0].y : 0u, cb = okb ? g.rec[k1].y : 0u;
                arb[k0] += ca & 0x00ff00ffu; ag[k0] += ca & 0x0000ff00u;
                arb[k1] += cb & 0x00ff00ffu; ag[k1] += cb & 0x0000ff00u;
            }
        };
        // Frame constants are fetched one frame AHEAD, alternating between two scalar register sets (a copy between sets
        // would make the wave wait for the load at once): the scalar-load latency of frame n+1 hides behind frame n's fold.
        HvSweepFrameK ka = hv_sweep_frame_k(Ps, __ffsll((long long)mask) - 1), kb = ka;
        // (Measured dead end: issuing frame n+1's evaluation - projection + gathers - BEFORE folding frame n, two gather sets
        // in flight at 126 VGPRs: 32.0 k frames/s against 32.7 k.  The wave does not wait for its gathers.)
        HvSweepGather g;
        while (true) {
            const int fa = __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            project_frame(ka, fa, kb, mask, g);
            apply_frame(g);
            if (!mask) break;
            const int fb = __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            project_frame(kb, fb, ka, mask, g);
            apply_frame(g);
            if (!mask) break;
        }
        // updated by at least one frame: fold the batch's colour into the planes (hv_sweep_epilogue: the colour loads of the pass first)
        auto new_weight = [&](const int zz) __attribute__((always_inline)) { return (uint32_t)((zz & 1) ? WF[zz / 2].y : WF[zz / 2].x); };
        hv_sweep_epilogue<ZH, ZH, false>(
            unit, wordb, [&](const int zz) __attribute__((always_inline)) { return new_weight(zz) != vw[zz]; },
            [&](const int zz, HvPlaneWords &w) __attribute__((always_inline)) {
                w.vt = (zz & 1) ? VT[zz / 2].y : VT[zz / 2].x;
                w.vw = new_weight(zz);
                w.r += arb[zz] & 0xffffu;
                w.g += ag[zz] >> 8;
                w.b += arb[zz] >> 16;
            });
    }
}

// ================================================================================================
// Sweep, production form: the batch is FOLDED per voxel, on WHOLE voxel columns.  The contract asks for bit-exact unit keys and
// weights and 1e-4 on tsdf / colour (BASELINE.json north_star); the running mean (tsdf w + t) / (w + 1) applied once per accepted
// frame is, in real numbers, (tsdf w0 + sum t) / (w0 + n) - so a lane keeps `sum t` and n per voxel in registers over the batch's
// frames and divides ONCE when the item is done (measured against the oracle's per-frame float chain: <= 3e-7).  What decides
// WHETHER a frame updates a voxel - the projection, the pixel it lands in, the truncation test - is still evaluated with the
// reference's IEEE operations in the reference's order, so weights and colour sums stay exact integers.  Against the bitwise form a
// voxel visit loses the correctly rounded running-mean division, the float weight carry, and three tests the item-level regime test
// already implies:
//  * `pc2 > 0`: an item only takes this path when every voxel of the wave's box lies beyond `near_z` of every frame in its mask;
//  * `depth > 0`: with near_z >= 1.25 sdf_trunc and a multiplier >= 1, a record with depth <= 0 (invalid, truncated, or
//    the zero an out-of-range buffer load returns) gives sdf <= -pc2 < -sdf_trunc and fails the truncation test by itself;
//  * the image-tile test of the tile-sharded mode folds into the image-range compare (the range constants become the tile's).
// The observation count rides in byte 3 of the packed colour word (HV_REC_ONE, set by the pack role): one masked add accumulates
// green and the count.  tsdf / weight planes are only read when the item is done, and only by lanes with n > 0: the epilogue
// (hv_sweep_epilogue) reads and writes the five planes of a column in passes of 4 voxels, one memory round trip per pass.
// A lane owns one (x, y) column of the unit and all 16 z of it, a wave 64 columns (one column group), a unit is 4 wave tasks:
//  * the z-walk starts at z = 0 for every lane: no replay of the reference's repeated float additions, and the per-frame set-up (the
//    rigid transform of the column's base point, the frame's buffer descriptor, the prefetch of the next frame's constants) is paid
//    once per 16 voxels: ~27 VALU instructions per voxel visit;
//  * the voxels of a column are evaluated 4 at a time; the gathers of group g+1 are issued BEFORE group g is folded, so a wave always
//    has 4 gathers in flight behind 4 voxels' worth of arithmetic;
//  * the accumulation runs under the EXEC mask of the accepting lanes (no selects; the compiler's execz branch skips a step no lane
//    accepts).
// 12-byte frame records ({depth, colour | 1 << 24, multiplier}: one gather per voxel visit).  Registers: 3 x 16 accumulators (sum t,
// r | b << 16, g << 8 | n << 24) + two gather groups: AT the 128 registers of 4 waves per SIMD.
// (Measured and dropped, rounds 3-5 - profiles/r03 .. r05: gather groups of 1 / 2 / 8 voxels, gathers pipelined across frames, the
// select form of the accumulation, 1 / 2 workgroups per unit, register caps of 120 / 112 / 5-6 waves per SIMD, 16-byte records.)
// Correction rounds of the projection's shared-reciprocal division: hv_div2 (online path, bitwise form) runs two, this kernel ONE.
// With the reciprocal refined by one Newton step the first round already returns the correctly rounded quotient on every operand
// pair tried: tools/divtest.hip, round 4 - 0 mismatches against IEEE division in 3.4e12 pairs each of the kernel's operand ranges,
// wide random exponents and divisors whose mantissa ends in runs of ones / zeros.  Two packed FMAs less per voxel visit.
// The kernel is a grid-stride loop over the work items of the batch's union list (hv_sweep_item), one wave per workgroup.  ZS = 2 (z
// halves, 8 one-wave tasks per unit) is the default for a GPU that shares the volume with 3 or more others.
// ================================================================================================
template <int ZS>
__global__ __launch_bounds__(64, 4) void k_tsdf_sweep_column(
    HvTable table, const int32_t *__restrict__ list, const unsigned long long *__restrict__ frame_mask,
    char *__restrict__ pool, const uint2 *__restrict__ frame_px, const HvFrameParams *__restrict__ Ps, int n_frames,
    int general, const float *__restrict__ mult, int parity) {
    constexpr int GV = 4;          // voxels per gather group
    // ZS = 2: a column is split into two z halves = 8 wave tasks per unit (a GPU that owns few units - multi-GPU sharding - has
    // ~3 000 column tasks of very different lengths for 4 096 wave slots: nothing evens them out; twice as many, half as long
    // tasks do).  The upper half replays the reference's 8 repeated float additions along z per frame.
    static_assert(ZS == 1 || ZS == 2, "whole columns or z halves");
    constexpr int ZH = 16 / ZS;
    constexpr int NG = ZH / GV;
    constexpr int PARTS = 4 * ZS;  // work items per unit: its 4 column groups x ZS z ranges
    constexpr int ZB = 4;          // voxels per epilogue pass (hv_sweep_epilogue)
    typedef uint32_t hv_u3 __attribute__((ext_vector_type(3)));
    int n_units = table.counters[HV_CNT_TOUCH(parity)];
    if (n_units > table.max_blocks) n_units = table.max_blocks;
    const int lane = threadIdx.x & 63;
    const HvFrameParams &P0 = Ps[0];
    const float vl = P0.voxel_length_f, hl = P0.half_voxel_length_f;
    const double unit_length = P0.unit_length;
    const int npx = P0.H * P0.W;
    const hv_f2 F = {P0.fx, P0.fy}, C = {P0.cx, P0.cy};
    const float lo_uf = fmaxf(0.0001f, (float)P0.tile_u0), lo_vf = fmaxf(0.0001f, (float)P0.tile_v0);
    const float hi_uf = fminf(P0.safe_width_f, (float)P0.tile_u1), hi_vf = fminf(P0.safe_height_f, (float)P0.tile_v1);
    const uint32_t lo_u = __float_as_uint(lo_uf), lo_v = __float_as_uint(lo_vf);
    const uint32_t lim_u = hi_uf > lo_uf ? __float_as_uint(hi_uf) - lo_u : 0u, lim_v = hi_vf > lo_vf ? __float_as_uint(hi_vf) - lo_v : 0u;
    const uint32_t W24 = (uint32_t)P0.W;
    const float ntrunc = -P0.sdf_trunc_f, tinv = P0.sdf_trunc_inv_f;
    const float near_z = fmaxf(0.03f, 1.25f * P0.sdf_trunc_f);
    const int n_items = hv_sweep_items(n_units, PARTS);
    for (int item = blockIdx.x; item < n_items; item += gridDim.x) {
        int t, part;
        hv_sweep_item(item, PARTS, t, part);
        if (t >= n_units) continue;
        const int z0 = ZS == 1 ? 0 : (part >> 2) * ZH; // first z of this task
        const int32_t slot = list[t];
        const int cg = part & 3; // column group: x in [4 cg, 4 cg + 4)
        const int x = cg * 4 + (lane >> 4);
        const int y = lane & 15;
        const int32_t idx = table.vals[slot];
        unsigned long long mask = frame_mask[slot];
        if (idx < 0 || mask == 0ull) continue;
        int32_t ux, uy, uz;
        hv_unpack_key(table.keys[slot], ux, uy, uz);
        const double o0 = (double)ux * unit_length, o1 = (double)uy * unit_length, o2 = (double)uz * unit_length;
        // lane f <-> frame f: does the box of this wave's voxel centres come within near_z of frame f's camera plane?
        bool near = false;
        // ... and: does the box project at least 2 pixels inside the image (the GPU's tile) in frame f?  Then every voxel
        // of the item does - a perspective projection maps the box into the hull of its projected corners - and the frame's visits skip the
        // image-range test: two v_sub + two v_cmp of ~30 instructions per visit, for ~70 % of the (item, frame) pairs of the bench's stream.
        bool interior = false;
        if (lane < n_frames && ((mask >> lane) & 1ull)) {
            const HvFrameParams &Pl = Ps[lane];
            const float bx = (float)((double)(hl + vl * (float)(cg * 4)) + o0), by = (float)((double)hl + o1),
                        bz = (float)((double)(hl + vl * (float)z0) + o2);
            const float zmin = (Pl.ext[8] * bx + Pl.ext[9] * by + Pl.ext[10] * bz + Pl.ext[11]) + fminf(Pl.ext[8] * (3.0f * vl), 0.f) +
                               fminf(Pl.ext[9] * (15.0f * vl), 0.f) + fminf(Pl.ext[10] * ((float)(ZH - 1) * vl), 0.f);
            near = !(zmin > near_z);
            if (!near) {
                float umin = 3.0e38f, umax = -3.0e38f, vmin = 3.0e38f, vmax = -3.0e38f;
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const float qx = bx + ((c & 1) ? 3.0f * vl : 0.0f), qy = by + ((c & 2) ? 15.0f * vl : 0.0f), qz = bz + ((c & 4) ? (float)(ZH - 1) * vl : 0.0f);
                    const float c2 = Pl.ext[8] * qx + Pl.ext[9] * qy + Pl.ext[10] * qz + Pl.ext[11];
                    const float rz = 1.0f / c2; // (c2 >= zmin > near_z)
                    const float cu = (Pl.ext[0] * qx + Pl.ext[1] * qy + Pl.ext[2] * qz + Pl.ext[3]) * F.x * rz + C.x + 0.5f;
                    const float cv = (Pl.ext[4] * qx + Pl.ext[5] * qy + Pl.ext[6] * qz + Pl.ext[7]) * F.y * rz + C.y + 0.5f;
                    umin = fminf(umin, cu); umax = fmaxf(umax, cu);
                    vmin = fminf(vmin, cv); vmax = fmaxf(vmax, cv);
                }
                interior = umin >= lo_uf + 2.0f && umax <= hi_uf - 2.0f && vmin >= lo_vf + 2.0f && vmax <= hi_vf - 2.0f;
            }
        }
        const unsigned long long interior_mask = __ballot(interior);
        const bool near_any = __any(near);
        char *unit = pool + (int64_t)idx * HV_TSDF_UNIT_BYTES;
        const int wordb = z0 * HV_TSDF_RR + cg * 64 + lane;
        const float p0 = (float)((double)(hl + vl * (float)x) + o0);
        const float p1 = (float)((double)(hl + vl * (float)y) + o1);
        const float p2 = (float)((double)hl + o2);
        if (general || near_any) {
            // rare regime: the reference's evaluation frame by frame with integer weights, one voxel at a time
#pragma unroll 1
            for (int zz = 0; zz < ZH; ++zz) {
                const int q = wordb + zz * HV_TSDF_RR;
                float vt = ((const float *)(unit + 0 * HV_TSDF_PLANE_BYTES))[q];
                uint32_t vw = ((const uint32_t *)(unit + 1 * HV_TSDF_PLANE_BYTES))[q];
                uint32_t vr = ((const uint32_t *)(unit + 2 * HV_TSDF_PLANE_BYTES))[q];
                uint32_t vg = ((const uint32_t *)(unit + 3 * HV_TSDF_PLANE_BYTES))[q];
                uint32_t vb = ((const uint32_t *)(unit + 4 * HV_TSDF_PLANE_BYTES))[q];
                bool dirty = false;
                unsigned long long m = mask;
#pragma unroll 1
                while (m) {
                    const int f = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    const HvFrameParams &P = Ps[f];
                    const float inc0 = P.ext_scaled_col2[0], inc1 = P.ext_scaled_col2[1], inc2 = P.ext_scaled_col2[2];
                    float pc0 = ((P.ext[0] * p0 + P.ext[1] * p1) + P.ext[2] * p2) + P.ext[3];
                    float pc1 = ((P.ext[4] * p0 + P.ext[5] * p1) + P.ext[6] * p2) + P.ext[7];
                    float pc2 = ((P.ext[8] * p0 + P.ext[9] * p1) + P.ext[10] * p2) + P.ext[11];
#pragma unroll 1
                    for (int s = 0; s < z0 + zz; ++s) { // the reference's repeated float additions along z, replayed
                        pc0 += inc0;
                        pc1 += inc1;
                        pc2 += inc2;
                    }
                    float tv;
                    uint32_t cv;
                    const uint2 *px_f = (const uint2 *)((const uint32_t *)frame_px + (int64_t)f * npx * 3);
                    const bool ok = hv_tsdf_eval_fast<true, true, true>(P, px_f, mult, pc0, pc1, pc2, tv, cv);
                    hv_tsdf_apply(ok, tv, cv, vt, vw, vr, vg, vb);
                    dirty |= ok;
                }
                if (dirty) {
                    ((float *)(unit + 0 * HV_TSDF_PLANE_BYTES))[q] = vt;
                    ((uint32_t *)(unit + 1 * HV_TSDF_PLANE_BYTES))[q] = vw;
                    ((uint32_t *)(unit + 2 * HV_TSDF_PLANE_BYTES))[q] = vr;
                    ((uint32_t *)(unit + 3 * HV_TSDF_PLANE_BYTES))[q] = vg;
                    ((uint32_t *)(unit + 4 * HV_TSDF_PLANE_BYTES))[q] = vb;
                }
            }
            continue;
        }
        float S[ZH];               // sum of the accepted frames' t
        uint32_t arb[ZH], agn[ZH]; // r | b << 16 and g << 8 | n << 24 of the accepted frames
#pragma unroll
        for (int k = 0; k < ZH; ++k) {
            S[k] = 0.0f;
            arb[k] = agn[k] = 0u;
        }
        struct Group { // GV voxels between their gather and their fold
            hv_u3 rec[GV];
            float zk[GV];
            bool inimg[GV];
        };
        // the frame whose voxels are being projected
        hv_f2 XY, INC;
        float Z, inc2;
        __amdgpu_buffer_rsrc_t rs_px;
        auto begin_frame = [&](const HvSweepFrameK K, const int f, HvSweepFrameK &Knext, const unsigned long long rest) __attribute__((always_inline)) {
            rs_px = __builtin_amdgcn_make_buffer_rsrc((void *)((const uint32_t *)frame_px + (int64_t)f * npx * 3), 0, npx * 12, 0x00020000);
            INC = K.i01;
            inc2 = K.i2;
            // pc = ((e0 p0 + e1 p1) + e2 p2) + e3 at z = 0, rows 0 and 1 as one float2 (same IEEE ops as the reference)
            XY = ((K.e04 * p0 + K.e15 * p1) + K.e26 * p2) + K.e37;
            const hv_f2 Z12 = K.e9_10 * hv_f2{p1, p2};
            Z = ((K.e8 * p0 + Z12.x) + Z12.y) + K.e11;
            if (ZS == 2 && z0 != 0) { // (wave-uniform) the reference's repeated additions up to this task's first voxel
#pragma unroll
                for (int sidx = 0; sidx < ZH; ++sidx) {
                    XY += INC;
                    Z += inc2;
                }
            }
            // K is consumed: only now issue the scalar loads of the next frame's constants (scalar loads return out of order, a
            // wait is always "for all"), so that their latency hides behind this frame's arithmetic
            __builtin_amdgcn_sched_barrier(0);
            Knext = hv_sweep_frame_k(Ps, rest ? __ffsll((long long)rest) - 1 : f);
            __builtin_amdgcn_sched_barrier(0);
        };
        bool frame_checked = true; // (wave-uniform) false: the frame is interior for this item, no voxel can leave the image
        auto project = [&](Group &g) __attribute__((always_inline)) {
#pragma unroll
            for (int k = 0; k < GV; ++k) {
                // (a0, a1) / pc2, correctly rounded, sharing one refined reciprocal (hv_div2's chain on a float2, ONE correction round)
                float r = __builtin_amdgcn_rcpf(Z);
                const float e = fmaf(-Z, r, 1.0f);
                r = fmaf(e, r, r);
                const hv_f2 A = XY * F;
                const hv_f2 R = hv_splat(r), NZ = hv_splat(-Z);
                hv_f2 Q = A * R;
                hv_f2 REM = hv_fma2(NZ, Q, A);
                Q = hv_fma2(REM, R, Q);
                const hv_f2 UV = (Q + C) + hv_splat(0.5f);
                bool in = true;
                // a scalar branch around four vector instructions, kept a branch by the empty asm.  (The same choice per gather group - two
                // copies of this loop - costs two more spilled registers and 5 % of the sweep; per frame - two copies of the frame body - 171.)
                if (frame_checked) {
                    asm volatile("" ::: "memory");
                    const bool in_u = (__float_as_uint(UV.x) - lo_u) < lim_u;
                    const bool in_v = (__float_as_uint(UV.y) - lo_v) < lim_v;
                    in = (int)in_u & (int)in_v;
                }
                g.inimg[k] = in;
                const uint32_t u = (uint32_t)(int)UV.x, v = (uint32_t)(int)UV.y; // saturating conversions: garbage lanes stay defined
                const uint32_t off = __umul24(v, W24) + u; // exact for every in-image pixel; a garbage lane reads 0 or some pixel, unused
                g.rec[k] = __builtin_bit_cast(hv_u3, __builtin_amdgcn_raw_buffer_load_b96(rs_px, (int)__umul24(off, 12u), 0, 0));
                g.zk[k] = Z;
                XY += INC;
                Z += inc2;
            }
        };
        auto fold = [&](const Group &g, const int gi) __attribute__((always_inline)) {
#pragma unroll
            for (int k = 0; k < GV; ++k) {
                const int z = gi * GV + k;
                const float sdf = (__uint_as_float(g.rec[k].x) - g.zk[k]) * __uint_as_float(g.rec[k].z);
                const bool ok = (int)g.inimg[k] & (int)(sdf > ntrunc);
                if (ok) { // the accumulation runs under the EXEC mask of the accepting lanes
                    asm volatile("" ::: "memory"); // keeps the branch: if-converted, the body is the select form again
                    S[z] += fminf(sdf * tinv, 1.0f); // == `if (t > 1) t = 1` for the non-NaN t of an accepted voxel
                    arb[z] += g.rec[k].y & 0x00ff00ffu;
                    agn[z] += g.rec[k].y & 0xff00ff00u;
                }
            }
        };
        HvSweepFrameK ka = hv_sweep_frame_k(Ps, __ffsll((long long)mask) - 1), kb = ka;
        auto fold_frame = [&](const HvSweepFrameK K, const int f, HvSweepFrameK &Knext, const unsigned long long rest) __attribute__((always_inline)) {
            begin_frame(K, f, Knext, rest);
            frame_checked = !((interior_mask >> f) & 1ull);
            // the gathers of group g+1 are issued before group g is folded; the pipeline drains at the end of a frame
            Group ga, gb;
            project(ga);
#pragma unroll
            for (int gi = 0; gi < NG; gi += 2) {
                project(gb);
                __builtin_amdgcn_sched_barrier(0);
                fold(ga, gi);
                __builtin_amdgcn_sched_barrier(0);
                if (gi + 2 < NG) project(ga);
                __builtin_amdgcn_sched_barrier(0);
                fold(gb, gi + 1);
                __builtin_amdgcn_sched_barrier(0);
            }
        };
        while (true) {
            const int fa = __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            fold_frame(ka, fa, kb, mask);
            if (!mask) break;
            const int fb = __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            fold_frame(kb, fb, ka, mask);
            if (!mask) break;
        }
        // one running-mean step per voxel for the whole batch, in passes over the column (hv_sweep_epilogue)
        hv_sweep_epilogue<ZH, ZB, true>(
            unit, wordb, [&](const int z) __attribute__((always_inline)) { return (agn[z] >> 24) != 0u; },
            [&](const int z, HvPlaneWords &w) __attribute__((always_inline)) {
                const uint32_t nw = w.vw + (agn[z] >> 24);
                w.vt = (w.vt * (float)w.vw + S[z]) / (float)nw;
                w.vw = nw;
                w.r += arb[z] & 0xffffu;
                w.g += (agn[z] >> 8) & 0xffffu;
                w.b += arb[z] >> 16;
            });
    }
}

// n16 16-byte words from device-visible host memory to device memory, one workgroup (see hv_tsdf_integrate_batch: frame constants).
__global__ __launch_bounds__(256) void k_upload_words(const uint4 *__restrict__ src, uint4 *__restrict__ dst, int n16) {
    for (int i = threadIdx.x; i < n16; i += 256) dst[i] = src[i]; // (one workgroup: 3-4 PCIe round trips for a 32-frame batch)
}

// After the sweep (one workgroup): clear the frame masks of the batch's units and zero the batch's touched-list counter, so
// that the next batch / online frame starts clean without a memset launch per counter.
__global__ __launch_bounds__(1024) void k_tsdf_batch_finish(HvTable table, const int32_t *__restrict__ list,
                                                             unsigned long long *__restrict__ frame_mask, int parity,
                                                             HvStatus *status, int32_t status_seq) {
    int n_units = table.counters[HV_CNT_TOUCH(parity)];
    if (n_units > table.max_blocks) n_units = table.max_blocks;
    __syncthreads(); // every thread holds n_units before the counters are reset
    // 8 independent list loads in flight per thread, then the 8 stores: two memory latencies per 8192 units instead
    // of two per 1024
    for (int base = 0; base < n_units; base += 8 * (int)blockDim.x) {
        int32_t slot[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int t = base + k * (int)blockDim.x + (int)threadIdx.x;
            slot[k] = t < n_units ? list[t] : -1;
        }
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (slot[k] >= 0) frame_mask[slot[k]] = 0ull;
    }
    if (threadIdx.x == 0) {
        table.counters[HV_CNT_TOUCH(parity)] = 0; // (the other set's counter may be filling: the next batch's touch pass)
        hv_publish_status(table, status, status_seq); // pool occupancy after this batch, for hv_capacity_gate
    }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
int make_frame_params(hv_volume *v, int H, int W, const double *intr, const double *T_cw,
                             double depth_scale, double depth_trunc, int depth_dtype, HvFrameParams *P) {
    memset(P, 0, sizeof(*P));
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) P->ext[r * 4 + c] = (float)T_cw[r * 4 + c];
    P->voxel_length_f = (float)v->cfg.voxel_size;
    P->half_voxel_length_f = P->voxel_length_f * 0.5f;
    for (int r = 0; r < 3; ++r) P->ext_scaled_col2[r] = P->ext[r * 4 + 2] * P->voxel_length_f;
    for (int c = 0; c < 4; ++c) {
        P->sweep_k[2 * c] = P->ext[c];
        P->sweep_k[2 * c + 1] = P->ext[4 + c];
    }
    P->sweep_k[8] = P->ext[8];
    P->sweep_k[9] = P->ext[11];
    P->sweep_k[10] = P->ext[9];
    P->sweep_k[11] = P->ext[10];
    for (int r = 0; r < 3; ++r) P->sweep_k[12 + r] = P->ext_scaled_col2[r];
    P->fx = (float)intr[0];
    P->fy = (float)intr[1];
    P->cx = (float)intr[2];
    P->cy = (float)intr[3];
    P->ffl_inv_x = 1.0f / (float)intr[0];
    P->ffl_inv_y = 1.0f / (float)intr[1];
    P->sdf_trunc_f = (float)v->cfg.sdf_trunc;
    P->sdf_trunc_inv_f = 1.0f / P->sdf_trunc_f;
    P->safe_width_f = (float)W - 0.0001f;
    P->safe_height_f = (float)H - 0.0001f;
    P->unit_length = v->cfg.voxel_size * (double)v->cfg.block_size;
    double pose[16];
    hv_invert4x4(T_cw, pose);
    for (int i = 0; i < 12; ++i) P->pose[i] = pose[i];
    P->fx_d = intr[0];
    P->fy_d = intr[1];
    P->cx_d = intr[2];
    P->cy_d = intr[3];
    P->sdf_trunc_d = v->cfg.sdf_trunc;
    P->depth_scale_f = (float)depth_scale;
    P->depth_trunc_d = depth_trunc;
    P->H = H;
    P->W = W;
    P->stride = v->cfg.depth_sampling_stride;
    P->touch_box_bits = v->touch_box_bits;
    P->bgr = v->color_bgr;
    P->depth_is_u16 = depth_dtype == HV_DEPTH_U16;
    const bool whole = v->tile[0] == 0 && v->tile[1] == 0 && v->tile[2] == 0 && v->tile[3] == 0;
    P->tile_u0 = whole ? 0 : v->tile[0];
    P->tile_v0 = whole ? 0 : v->tile[1];
    P->tile_u1 = whole ? W : v->tile[2];
    P->tile_v1 = whole ? H : v->tile[3];
    P->tiled = whole ? 0 : 1;
    P->owner_rank = v->owner_rank;
    P->owner_world = v->owner_world;
    return HV_OK;
}

// First half of a frame: convert/pack the frame, claim and list the touched units.  (This parity's
// touched counter was zeroed by the previous frame's sweep kernel.)
static int tsdf_launch_touch(hv_volume *v, hipStream_t s, const HvFrameParams &P, int parity, const void *d_depth,
                             const uint8_t *d_rgb) {
    const int64_t npx = (int64_t)P.H * P.W;
    const int n_prep_blocks = (int)((npx + 255) / 256);
    const int ns = ((P.W + P.stride - 1) / P.stride) * ((P.H + P.stride - 1) / P.stride);
    const int n_touch_blocks = (ns * HV_TOUCH_FAN + 255) / 256;
    // Per-frame scratch (frame_px, touched_list) is single-buffered: the two halves of a frame run back to back on one stream.
    // Measured alternative, rejected: prep+touch of frame f+1 on a second stream overlapping the sweep of frame f (double-buffered
    // scratch, event hand-offs) ran 6955 vs 7280 frames/s - the cross-stream waits and the contention on the sweep cost more than
    // the 16 us they hide.
    hipLaunchKernelGGL(k_tsdf_prep_touch, dim3(n_prep_blocks + n_touch_blocks), dim3(256), 0, s, v->table,
                       v->touched_stamp, v->touched_list, parity, d_depth, d_rgb, (uint2 *)v->frame_px, P, n_touch_blocks);
    return HV_OK;
}

// Second half on the volume's stream: sweep the touched units.  Grid: enough workgroups to fill
// 256 CUs; grid-stride over the device-side touched count (no host round trip between launches).
// (Re)build the per-pixel multiplier table when the intrinsics or the image size changed (stream-ordered).
int tsdf_multiplier_table(hv_volume *v, const HvFrameParams &P) {
    const float key[4] = {P.cx, P.cy, P.ffl_inv_x, P.ffl_inv_y};
    if (v->mult_table != nullptr && v->mult_W == P.W && v->mult_H == P.H && memcmp(key, v->mult_key, sizeof(key)) == 0)
        return HV_OK;
    const size_t npx = (size_t)P.W * P.H;
    void *buf = v->mult_table;
    int rc = hv_ensure_buffer(v, &buf, &v->mult_table_bytes, npx * sizeof(float));
    if (rc != HV_OK) return rc;
    v->mult_table = (float *)buf;
    hipLaunchKernelGGL(k_tsdf_multiplier_table, dim3((unsigned)((npx + 255) / 256)), dim3(256), 0, v->stream, P,
                       v->mult_table);
    HV_HIP(hipGetLastError());
    memcpy(v->mult_key, key, sizeof(key));
    v->mult_W = P.W;
    v->mult_H = P.H;
    return HV_OK;
}

static int tsdf_launch_integrate(hv_volume *v, const HvFrameParams &P, int parity) {
    const dim3 grid(8192), block(256); // > touched units of a frame: no second pass per block
    hv_profile_begin(v);
    hipLaunchKernelGGL(k_tsdf_integrate, grid, block, 0, v->stream, v->table, (const int32_t *)v->touched_list, parity, (char *)v->pool,
                       (const uint2 *)v->frame_px, P, v->d_status, hv_next_status_seq(v));
    hv_profile_end(v, 0);
    HV_HIP(hipGetLastError());
    return HV_OK;
}

static void tsdf_next_frame(hv_volume *v, HvFrameParams &P, int &parity) {
    v->content_version += 1;
    v->frame_counter += 1;
    P.frame_id = v->frame_counter;
    parity = v->frame_counter & 1;
    v->last_touch_parity = parity;
    v->touch_counters_clean = false; // this parity's counter keeps the frame's touched count until the next frame's sweep
}

// hv_tsdf_set_rectify_maps: B device-resident frames through the camera's undistort / rectify maps on stream `s` (one launch), into
// the volume's rect_buf; depth / rgb then point at the rectified copies.  The buffer is single: the launch that reads it (touch + pack
// of the same batch) follows on the same stream, and the next batch's rectify launch follows that one (same stream) or the event the
// aux stream waits for (ev_presweep, recorded on the main stream behind it).
int tsdf_rectify(hv_volume *v, hipStream_t s, const void **depth, int depth_dtype, const uint8_t **rgb, int B, int H, int W) {
    if (v->rect_W == 0) return HV_OK;
    HV_REQUIRE(v->rect_W == W && v->rect_H == H, HV_ERR_INVALID, "hv_tsdf_integrate: frames are %dx%d, the rectify maps %dx%d", W, H, v->rect_W, v->rect_H);
    const size_t npx = (size_t)H * W, dsz = depth_dtype == HV_DEPTH_U16 ? 2 : 4;
    const size_t depth_bytes = (npx * dsz * (size_t)B + 255) & ~(size_t)255;
    const size_t want = depth_bytes + npx * 3 * (size_t)B;
    if (v->rect_buf_bytes < want && v->stream_aux) HV_HIP(hipStreamSynchronize(v->stream_aux)); // (a launch on the aux stream may still read the old buffer)
    int rc = hv_ensure_buffer(v, &v->rect_buf, &v->rect_buf_bytes, want);
    if (rc != HV_OK) return rc;
    rc = hv_rectify_frames_device(v, s, *depth, depth_dtype, *rgb, B, H, W, v->rect_buf, (uint8_t *)v->rect_buf + depth_bytes);
    if (rc != HV_OK) return rc;
    *depth = v->rect_buf;
    *rgb = (const uint8_t *)v->rect_buf + depth_bytes;
    return HV_OK;
}

// Online path: both halves back to back on the volume's stream.  In checked mode (hv_capacity_gate: the pool's headroom is
// not known to cover this frame) the claims of the touch pass are verified before anything is fused: if some did not fit
// the pool grows and the touch pass runs again under a fresh stamp.
static int tsdf_integrate_one(hv_volume *v, const void *d_depth, int depth_dtype, const uint8_t *d_rgb,
                              int H, int W, const double *intr, const double *T_cw, double depth_scale,
                              double depth_trunc) {
    bool checked = false;
    int rc = hv_capacity_gate(v, &checked);
    if (rc != HV_OK) return rc;
    rc = tsdf_rectify(v, v->stream, &d_depth, depth_dtype, &d_rgb, 1, H, W);
    if (rc != HV_OK) return rc;
    HvFrameParams P;
    make_frame_params(v, H, W, intr, T_cw, depth_scale, depth_trunc, depth_dtype, &P);
    int parity = 0;
    for (int attempt = 0;; ++attempt) {
        tsdf_next_frame(v, P, parity);
        if (attempt > 0) HV_HIP(hipMemsetAsync(&v->table.counters[HV_CNT_TOUCH0], 0, HV_CNT_TOUCH_SPAN_BYTES, v->stream));
        rc = tsdf_launch_touch(v, v->stream, P, parity, d_depth, d_rgb);
        if (rc != HV_OK) return rc;
        if (!checked) break;
        rc = hv_claims_fit(v);
        if (rc == HV_OK) break;
        if (rc != HV_RETRY_CLAIM || attempt >= 8) return rc == HV_RETRY_CLAIM ? HV_ERR_CAPACITY : rc;
        make_frame_params(v, H, W, intr, T_cw, depth_scale, depth_trunc, depth_dtype, &P); // (touch_box_bits etc. unchanged; cheap)
    }
    return tsdf_launch_integrate(v, P, parity);
}

int check_tsdf_args(hv_volume *v, const void *depth, const uint8_t *rgb, int H, int W,
                           const double *intr, const double *T_cw, int frames) {
    HV_REQUIRE(v != nullptr, HV_ERR_INVALID, "hv_tsdf_integrate: null volume");
    HV_REQUIRE(v->cfg.mode == HV_MODE_TSDF, HV_ERR_MODE, "hv_tsdf_integrate: volume is not in TSDF mode");
    HV_REQUIRE(depth != nullptr && rgb != nullptr && intr != nullptr && T_cw != nullptr, HV_ERR_INVALID,
               "[ScalableTSDFVolume::Integrate] Unsupported image format.");
    HV_REQUIRE(H > 0 && W > 0 && frames > 0, HV_ERR_INVALID, "hv_tsdf_integrate: empty image");
    HV_REQUIRE((int64_t)H * W <= v->cfg.max_points, HV_ERR_CAPACITY,
               "hv_tsdf_integrate: image %dx%d exceeds max_points=%lld", W, H, (long long)v->cfg.max_points);
    return HV_OK;
}

extern "C" {

int hv_tsdf_integrate(hv_volume *v, const void *depth, int32_t depth_dtype, const uint8_t *rgb,
                      int32_t height, int32_t width, const double *intr, const double *T_cw,
                      double depth_scale, double depth_trunc, int32_t loc) {
    int rc = check_tsdf_args(v, depth, rgb, height, width, intr, T_cw, 1);
    if (rc != HV_OK) return rc;
    HV_HIP(hipSetDevice(v->device));
    const size_t npx = (size_t)height * width;
    const void *d_depth = nullptr;
    const uint8_t *d_rgb = nullptr;
    rc = hv_stage_frame(v, depth, depth_dtype, rgb, npx, loc, &d_depth, &d_rgb);
    if (rc != HV_OK) return rc;
    return tsdf_integrate_one(v, d_depth, depth_dtype, d_rgb, height, width, intr, T_cw,
                              depth_scale, depth_trunc);
}

} // extern "C"

// Scratch of a multi-frame call: [B frame records of rec_bytes each per pixel][pad to 256][B HvFrameParams].  Returns the bytes to
// ask for; *params_offset = where the frame constants start.
size_t tsdf_batch_scratch(size_t rec_bytes, size_t npx, int B, size_t *params_offset) {
    const size_t px_bytes = rec_bytes * npx * (size_t)B;
    *params_offset = (px_bytes + 255) & ~(size_t)255;
    return px_bytes + 256 + sizeof(HvFrameParams) * (size_t)B;
}

// depth_ptrs / rgb_ptrs != nullptr: host-resident frames given one pointer per frame (hv_tsdf_integrate_frames); else `depth`
// / `rgb` hold the frames contiguously at `loc`.
int tsdf_integrate_batch_impl(hv_volume *v, const void *depth, const void *const *depth_ptrs, int32_t depth_dtype,
                                     const uint8_t *rgb, const void *const *rgb_ptrs, int32_t n_frames, int32_t height,
                                     int32_t width, const double *intr, const double *T_cw, double depth_scale,
                                     double depth_trunc, int32_t loc) {
    int rc = HV_OK;
    HV_HIP(hipSetDevice(v->device));
    const size_t npx = (size_t)height * width;
    const size_t dsz = depth_dtype == HV_DEPTH_U16 ? 2 : 4;
    const void *d_depth = nullptr, *d_rgb = nullptr;
    int host_set = -1; // device staging set of host-resident frames (hv_stage_frames)
    if (loc == HV_HOST) {
        // pageable caller memory -> page-locked slots -> DMA on the copy stream, two device sets: the frames of this call
        // cross PCIe while the previous batch is still being swept
        rc = hv_stage_frames(v, depth_ptrs, depth, npx * dsz, rgb_ptrs, rgb, npx * 3, n_frames, &d_depth, &d_rgb, &host_set);
        if (rc != HV_OK) return rc;
    } else {
        d_depth = depth;
        d_rgb = rgb;
    }
    if (n_frames == 1) { // trivial batch: the online path
        if (host_set >= 0) HV_HIP(hipStreamWaitEvent(v->stream, v->hs_dev_ready[host_set], 0));
        rc = tsdf_integrate_one(v, d_depth, depth_dtype, (const uint8_t *)d_rgb, height, width, intr, T_cw, depth_scale, depth_trunc);
        if (rc != HV_OK) return rc;
        if (host_set >= 0) return hv_stage_frames_consumed(v, host_set, v->stream);
        return HV_OK;
    }
    // multi-frame sweeps of up to 64 frames (one bit per frame in the per-unit mask)
    //
    // Batch pipeline.  A batch is [touch + pack launch: HBM streaming and hash-insert latency chains] -> [sweep: VALU-bound]
    // -> [finish].  When batches follow each other with nothing else done to the volume in between (a replay / rebuild loop),
    // the touch + pack launch of batch k+1 goes to a second stream and runs WHILE batch k is swept: it only inserts units and
    // fills its own scratch set (frame records, union list, frame masks, list counter: two sets, alternating), the sweep of
    // batch k reads none of that.  Hand-offs: the aux stream waits for the event recorded on the main stream just before the
    // PREVIOUS sweep (everything older than that sweep is done - in particular the batch that last used this scratch set);
    // the main stream waits for this batch's touch + pack before its own sweep.  Every other entry point works on the main
    // stream behind those waits and never meets the aux stream; a call that finds the volume touched by anything else since
    // the previous batch (content_version), the checked capacity mode or HV_TSDF_PIPELINE=0 runs everything on the main stream.
    const bool pipeline_on = !(getenv("HV_TSDF_PIPELINE") && atoi(getenv("HV_TSDF_PIPELINE")) == 0);
    // sweep form: 4 = k_tsdf_sweep_column (production: the batch folded per voxel, a lane walks a whole voxel column, tsdf within
    // 5e-6 of the per-frame chain), 2 = k_tsdf_sweep (the reference's running mean frame by frame: tsdf bit-identical to it).
    // The switches are read per call: the parity tests flip them inside one process.
    const int sweep_form = getenv("HV_TSDF_SWEEP") && atoi(getenv("HV_TSDF_SWEEP")) == 2 ? 2 : 4;
    const bool rec12 = sweep_form == 4; // 12-byte frame records {depth, colour, multiplier}; the bitwise form: 8-byte records + the table
    const size_t rec_bytes = rec12 ? 12 : 8;
    // 1: run the EXACT evaluation with integer weights everywhere (parity checks of the rare-regime code)
    const int general = getenv("HV_TSDF_BATCH_GENERAL") ? atoi(getenv("HV_TSDF_BATCH_GENERAL")) : 0;
    // z halves (8 tasks per unit) when this GPU shares the volume with 3 or more others: DESIGN section 4
    const int zs = getenv("HV_TSDF_SWEEP_ZS") ? atoi(getenv("HV_TSDF_SWEEP_ZS")) : (v->owner_world >= 4 ? 2 : 1);
    const int sweep_grid = 65536; // one work item each up to 16 384 units per batch, grid-stride beyond (measured: 29.6 k frames/s vs 28.2 k at 8192)
    bool chain_ok = v->pipe_armed && v->pipe_version == v->content_version; // nothing but batches since ev_presweep was recorded
    v->content_version += 1;
    const int BMAX = HV_BATCH_MAX;
    for (int f0 = 0; f0 < n_frames; f0 += BMAX) {
        const int B = std::min(BMAX, n_frames - f0);
        // pool headroom (grows here when more than half is known to be used; see hv_capacity_gate)
        bool checked = false;
        const int64_t max_before = v->cfg.max_blocks;
        rc = hv_capacity_gate(v, &checked);
        if (rc != HV_OK) return rc;
        if (v->cfg.max_blocks != max_before) chain_ok = false; // the pool grew: the stream was drained, start a fresh chain
        const bool overlap = pipeline_on && chain_ok && !checked;
        if (v->stream_aux == nullptr) {
            HV_HIP(hipStreamCreateWithFlags(&v->stream_aux, hipStreamNonBlocking)); // (queue priorities, CU masks: measured, no gain - profiles/r04, r05)
            HV_HIP(hipEventCreateWithFlags(&v->ev_prep, hipEventDisableTiming));
            HV_HIP(hipEventCreateWithFlags(&v->ev_presweep, hipEventDisableTiming));
        }
        hipStream_t ps = overlap ? v->stream_aux : v->stream; // where this batch's touch + pack launch goes
        bool overlap_this = overlap;
        // scratch set (two, alternating)
        const int parity = v->batch_parity & 1;
        v->batch_parity = parity ^ 1;
        int32_t *d_list = v->touched_list + (size_t)parity * (size_t)v->cfg.max_blocks;
        unsigned long long *d_mask_rw = (unsigned long long *)v->touched_mask + (size_t)parity * (size_t)v->table_capacity;
        // what this batch's touch + pack launch waits for: the batch that last used its scratch set is swept and finished =
        // the main stream up to just before the previous sweep
        if (overlap) HV_HIP(hipStreamWaitEvent(v->stream_aux, v->ev_presweep, 0));
        if (host_set >= 0) HV_HIP(hipStreamWaitEvent(ps, v->hs_dev_ready[host_set], 0)); // the frames have arrived
        // per-frame constants go through a ring of 4 pinned host buffers: a slot is only rewritten after the upload that last
        // used it has completed, so consecutive calls queue up on the stream without a host synchronisation
        const int ri = v->params_idx;
        v->params_idx = (ri + 1) & 3;
        if (v->pinned_params[ri] == nullptr) {
            HV_HIP(hipHostMalloc(&v->pinned_params[ri], sizeof(HvFrameParams) * BMAX));
            HV_HIP(hipEventCreateWithFlags(&v->params_ev[ri], hipEventDisableTiming));
        } else {
            HV_HIP(hipEventSynchronize(v->params_ev[ri]));
        }
        HvFrameParams *params = (HvFrameParams *)v->pinned_params[ri];
        for (int f = 0; f < B; ++f) {
            make_frame_params(v, height, width, intr, T_cw + 16 * (size_t)(f0 + f), depth_scale, depth_trunc, depth_dtype,
                              &params[f]);
            v->frame_counter += 1;
            params[f].frame_id = v->frame_counter;
        }
        int batch_stamp = v->frame_counter;
        v->last_touch_parity = parity;
        {
            // (the pack role copies the multipliers into the 12-byte records: when the table has to be rebuilt - first call, other
            // intrinsics - it is rebuilt on the main stream and this batch's touch + pack launch follows it there)
            const float *before = v->mult_table;
            const int mw = v->mult_W, mh = v->mult_H;
            float key_before[4];
            memcpy(key_before, v->mult_key, sizeof(key_before));
            rc = tsdf_multiplier_table(v, params[0]);
            if (rc != HV_OK) return rc;
            if (before != v->mult_table || mw != v->mult_W || mh != v->mult_H || memcmp(key_before, v->mult_key, sizeof(key_before)) != 0) {
                if (ps != v->stream) HV_HIP(hipStreamSynchronize(v->stream_aux)); // nothing of an older batch still reads the old table there
                ps = v->stream;
                overlap_this = false;
                if (host_set >= 0) HV_HIP(hipStreamWaitEvent(ps, v->hs_dev_ready[host_set], 0));
            }
        }
        const float *d_mult = v->mult_table;
        size_t params_off = 0;
        const size_t want = tsdf_batch_scratch(rec_bytes, npx, B, &params_off);
        void **bb = parity ? &v->batch_buf2 : &v->batch_buf;
        size_t *bb_bytes = parity ? &v->batch_buf2_bytes : &v->batch_buf_bytes;
        if (*bb_bytes < want && v->stream_aux) HV_HIP(hipStreamSynchronize(v->stream_aux)); // (a launch two batches back may still write the old buffer)
        rc = hv_ensure_buffer(v, bb, bb_bytes, want); // (re-allocation drains the main stream, and with it every batch whose touch pass it waited for)
        if (rc != HV_OK) return rc;
        uint2 *d_px = (uint2 *)*bb;
        HvFrameParams *d_params = (HvFrameParams *)((char *)*bb + params_off);
        // The 12 KB of frame constants go up with a ONE-WORKGROUP kernel that reads the page-locked ring slot in place (hipHostMalloc
        // memory is device-visible).  hipMemcpyAsync turns a small pinned copy into the runtime's blit kernel, whose workgroups wait
        // for wave slots behind the sweep that is running on the other queue: 100-420 us per batch in profiles/r03/
        // pipeline_timeline.txt (first version), which delayed the touch + pack launch to the end of the sweep it should hide in.
        {
            const int n16 = (int)((sizeof(HvFrameParams) * (size_t)B + 15) / 16);
            hipLaunchKernelGGL(k_upload_words, dim3(1), dim3(256), 0, ps, (const uint4 *)params, (uint4 *)d_params, n16);
        }
        HV_HIP(hipEventRecord(v->params_ev[ri], ps));
        const int n_prep_blocks = (int)((npx + 1023) / 1024); // 4 pixels per thread
        const int n_pack_groups = (B + HV_PACK_FRAMES - 1) / HV_PACK_FRAMES; // a pack thread handles its pixels in a whole group of frames
        const int n_touch_blocks = (hv_touch_patches(width, height, v->cfg.depth_sampling_stride) + 3) / 4;
        // this chunk's frames (through the camera's rectify maps first, when the volume has them: hv_tsdf_set_rectify_maps)
        const void *c_depth = (const char *)d_depth + npx * dsz * (size_t)f0;
        const uint8_t *c_rgb = (const uint8_t *)d_rgb + npx * 3 * (size_t)f0;
        rc = tsdf_rectify(v, ps, &c_depth, depth_dtype, &c_rgb, B, height, width);
        if (rc != HV_OK) return rc;
        for (int attempt = 0;; ++attempt) {
            // the touched-list counters are zero after hv_reset and k_tsdf_batch_finish; an online frame or an aborted claim pass
            // leaves its own parity's count behind (never while a chain runs)
            if (!v->touch_counters_clean) HV_HIP(hipMemsetAsync(&v->table.counters[HV_CNT_TOUCH0], 0, HV_CNT_TOUCH_SPAN_BYTES, v->stream));
            v->touch_counters_clean = true;
            hipLaunchKernelGGL(k_tsdf_prep_touch_batch, dim3(n_touch_blocks * B + n_prep_blocks * n_pack_groups), dim3(256), 0, ps,
                               v->table, v->touched_stamp, d_mask_rw, d_list, batch_stamp,
                               (const char *)c_depth, (int64_t)(npx * dsz), c_rgb, d_px, (const HvFrameParams *)d_params, n_prep_blocks, n_touch_blocks, B, parity,
                               rec12 ? d_mult : (const float *)nullptr);
            if (!checked) break;
            // checked mode: nothing is fused before every unit of the batch has its pool slot; if some claims did not fit, the
            // pool has grown (table rebuilt without them, stamps kept) and the touch pass runs again under a fresh stamp
            rc = hv_claims_fit(v);
            if (rc == HV_OK) break;
            if (rc != HV_RETRY_CLAIM || attempt >= 8) return rc == HV_RETRY_CLAIM ? HV_ERR_CAPACITY : rc;
            v->frame_counter += 1;
            batch_stamp = v->frame_counter;
            v->touch_counters_clean = false;
            // the tables were rebuilt: the scratch set's arrays moved
            d_list = v->touched_list + (size_t)parity * (size_t)v->cfg.max_blocks;
            d_mask_rw = (unsigned long long *)v->touched_mask + (size_t)parity * (size_t)v->table_capacity;
        }
        // What the NEXT batch's touch + pack launch waits for: everything the main stream holds up to here, i.e. the finish of the
        // batch that last used the next batch's scratch set.  Recorded BEFORE the main stream waits for this batch's own touch + pack
        // launch: the aux stream is in order, so the next launch follows this batch's there anyway, and recorded after it every touch +
        // pack launch also waited for the cross-queue hand-off into the sweep before it (profiles/r04/rank8_timeline.txt).
        HV_HIP(hipEventRecord(v->ev_presweep, v->stream));
        if (overlap_this) {
            HV_HIP(hipEventRecord(v->ev_prep, v->stream_aux));
            HV_HIP(hipStreamWaitEvent(v->stream, v->ev_prep, 0));
        }
        chain_ok = true; // (the next chunk of this call may follow this one directly)
        hv_profile_begin(v);
        const unsigned long long *d_mask = d_mask_rw;
        if (sweep_form == 2)
            hipLaunchKernelGGL(k_tsdf_sweep, dim3(sweep_grid), dim3(64 * HV_SWEEP_WAVES), 0, v->stream, v->table, (const int32_t *)d_list, d_mask,
                               (char *)v->pool, (const uint2 *)d_px, (const HvFrameParams *)d_params, B, general, d_mult, parity);
        else if (zs == 2)
            hipLaunchKernelGGL(k_tsdf_sweep_column<2>, dim3(sweep_grid), dim3(64), 0, v->stream, v->table, (const int32_t *)d_list, d_mask,
                               (char *)v->pool, (const uint2 *)d_px, (const HvFrameParams *)d_params, B, general, d_mult, parity);
        else
            hipLaunchKernelGGL(k_tsdf_sweep_column<1>, dim3(sweep_grid), dim3(64), 0, v->stream, v->table, (const int32_t *)d_list, d_mask,
                               (char *)v->pool, (const uint2 *)d_px, (const HvFrameParams *)d_params, B, general, d_mult, parity);
        hv_profile_end(v, B);
        hipLaunchKernelGGL(k_tsdf_batch_finish, dim3(1), dim3(1024), 0, v->stream, v->table, (const int32_t *)d_list, d_mask_rw, parity, v->d_status,
                           hv_next_status_seq(v));
        HV_HIP(hipGetLastError());
    }
    v->pipe_armed = true;
    v->pipe_version = v->content_version;
    // (every touch + pack launch of this call precedes the point the main stream has reached: it waited for each of them)
    if (host_set >= 0) return hv_stage_frames_consumed(v, host_set, v->stream);
    return HV_OK;
}

extern "C" {

int hv_tsdf_integrate_batch(hv_volume *v, const void *depth, int32_t depth_dtype, const uint8_t *rgb,
                            int32_t n_frames, int32_t height, int32_t width, const double *intr,
                            const double *T_cw, double depth_scale, double depth_trunc, int32_t loc) {
    int rc = check_tsdf_args(v, depth, rgb, height, width, intr, T_cw, n_frames);
    if (rc != HV_OK) return rc;
    return tsdf_integrate_batch_impl(v, depth, nullptr, depth_dtype, rgb, nullptr, n_frames, height, width, intr, T_cw, depth_scale,
                                     depth_trunc, loc);
}

int hv_tsdf_integrate_frames(hv_volume *v, const void *const *depth_frames, int32_t depth_dtype, const uint8_t *const *rgb_frames,
                             int32_t n_frames, int32_t height, int32_t width, const double *intr, const double *T_cw,
                             double depth_scale, double depth_trunc) {
    HV_REQUIRE(depth_frames != nullptr && rgb_frames != nullptr && n_frames >= 1, HV_ERR_INVALID, "hv_tsdf_integrate_frames: null argument");
    for (int f = 0; f < n_frames; ++f)
        HV_REQUIRE(depth_frames[f] != nullptr && rgb_frames[f] != nullptr, HV_ERR_INVALID, "hv_tsdf_integrate_frames: null frame %d", f);
    int rc = check_tsdf_args(v, depth_frames[0], rgb_frames[0], height, width, intr, T_cw, n_frames);
    if (rc != HV_OK) return rc;
    return tsdf_integrate_batch_impl(v, nullptr, depth_frames, depth_dtype, nullptr, (const void *const *)rgb_frames, n_frames, height,
                                     width, intr, T_cw, depth_scale, depth_trunc, HV_HOST);
}

int hv_tsdf_set_tile(hv_volume *v, int32_t u0, int32_t v0, int32_t u1, int32_t v1) {
    HV_REQUIRE(v != nullptr, HV_ERR_INVALID, "hv_tsdf_set_tile: null volume");
    HV_REQUIRE(v->cfg.mode == HV_MODE_TSDF, HV_ERR_MODE, "hv_tsdf_set_tile: volume is not in TSDF mode");
    HV_REQUIRE((u0 == 0 && v0 == 0 && u1 == 0 && v1 == 0) || (u0 >= 0 && v0 >= 0 && u1 > u0 && v1 > v0), HV_ERR_INVALID,
               "hv_tsdf_set_tile: empty tile");
    v->tile[0] = u0;
    v->tile[1] = v0;
    v->tile[2] = u1;
    v->tile[3] = v1;
    return HV_OK;
}

int hv_tsdf_set_color_order(hv_volume *v, int32_t bgr) {
    HV_REQUIRE(v != nullptr, HV_ERR_INVALID, "hv_tsdf_set_color_order: null volume");
    HV_REQUIRE(v->cfg.mode == HV_MODE_TSDF, HV_ERR_MODE, "hv_tsdf_set_color_order: volume is not in TSDF mode");
    v->color_bgr = bgr ? 1 : 0;
    return HV_OK;
}

int hv_tsdf_set_owner(hv_volume *v, int32_t rank, int32_t world_size) {
    HV_REQUIRE(v != nullptr, HV_ERR_INVALID, "hv_tsdf_set_owner: null volume");
    HV_REQUIRE(v->cfg.mode == HV_MODE_TSDF, HV_ERR_MODE, "hv_tsdf_set_owner: volume is not in TSDF mode");
    HV_REQUIRE(world_size >= 1 && rank >= 0 && rank < world_size, HV_ERR_INVALID, "hv_tsdf_set_owner: bad rank/world");
    v->owner_rank = rank;
    v->owner_world = world_size;
    return HV_OK;
}

int hv_tsdf_dump(hv_volume *v, int32_t *keys, float *tsdf, float *weight, double *color, int64_t *n_units) {
    HV_REQUIRE(v != nullptr && n_units != nullptr, HV_ERR_INVALID, "hv_tsdf_dump: null argument");
    HV_REQUIRE(v->cfg.mode == HV_MODE_TSDF, HV_ERR_MODE, "hv_tsdf_dump: volume is not in TSDF mode");
    int64_t nb = 0;
    int rc = hv_num_blocks(v, &nb);
    if (rc != HV_OK) return rc;
    *n_units = nb;
    if (nb == 0 || (keys == nullptr && tsdf == nullptr && weight == nullptr && color == nullptr)) return HV_OK;
    std::vector<int32_t> order, xyz; // the units and their keys by ascending (x, y, z)
    rc = hv_tsdf_key_order(v, nb, order, &xyz);
    if (rc != HV_OK) return rc;
    std::vector<char> unit((size_t)HV_TSDF_UNIT_BYTES);
    for (int64_t o = 0; o < nb; ++o) {
        const int64_t i = order[o];
        if (keys) memcpy(keys + o * 3, &xyz[o * 3], 12);
        if (!(tsdf || weight || color)) continue;
        HV_HIP(hipMemcpy(unit.data(), (char *)v->pool + i * unit.size(), unit.size(), hipMemcpyDeviceToHost));
        const float *pt = (const float *)unit.data();
        const uint32_t *pw = (const uint32_t *)(unit.data() + HV_TSDF_PLANE_BYTES);
        const uint32_t *pr = (const uint32_t *)(unit.data() + 2 * HV_TSDF_PLANE_BYTES);
        const uint32_t *pg = (const uint32_t *)(unit.data() + 3 * HV_TSDF_PLANE_BYTES);
        const uint32_t *pb = (const uint32_t *)(unit.data() + 4 * HV_TSDF_PLANE_BYTES);
        for (int x = 0; x < HV_TSDF_R; ++x)
            for (int y = 0; y < HV_TSDF_R; ++y)
                for (int z = 0; z < HV_TSDF_R; ++z) {
                    const int src = hv_tsdf_word(x, y, z);
                    const int64_t dst = o * HV_TSDF_RRR + (x * HV_TSDF_R + y) * HV_TSDF_R + z;
                    if (tsdf) tsdf[dst] = pt[src];
                    if (weight) weight[dst] = (float)pw[src];
                    if (color) {
                        const double w = (double)pw[src];
                        color[dst * 3 + 0] = w > 0 ? (double)pr[src] / w : 0.0;
                        color[dst * 3 + 1] = w > 0 ? (double)pg[src] / w : 0.0;
                        color[dst * 3 + 2] = w > 0 ? (double)pb[src] / w : 0.0;
                    }
                }
    }
    return HV_OK;
}

int hv_tsdf_touched(hv_volume *v, int32_t *keys, int64_t cap, int64_t *n) {
    HV_REQUIRE(v != nullptr && n != nullptr, HV_ERR_INVALID, "hv_tsdf_touched: null argument");
    HV_REQUIRE(v->cfg.mode == HV_MODE_TSDF, HV_ERR_MODE, "hv_tsdf_touched: volume is not in TSDF mode");
    int rc = hv_read_counters(v);
    if (rc != HV_OK) return rc;
    int64_t nt = v->h_counters[HV_CNT_TOUCH(v->last_touch_parity)];
    if (nt > v->cfg.max_blocks) nt = v->cfg.max_blocks;
    *n = nt;
    if (keys == nullptr || nt == 0) return HV_OK;
    std::vector<int32_t> slots((size_t)nt);
    HV_HIP(hipMemcpy(slots.data(), v->touched_list, sizeof(int32_t) * nt, hipMemcpyDeviceToHost));
    std::vector<uint64_t> tkeys((size_t)v->table_capacity);
    HV_HIP(hipMemcpy(tkeys.data(), v->table.keys, sizeof(uint64_t) * v->table_capacity, hipMemcpyDeviceToHost));
    std::vector<std::array<int32_t, 3>> out((size_t)nt);
    for (int64_t i = 0; i < nt; ++i) hv_unpack_key(tkeys[slots[i]], out[i][0], out[i][1], out[i][2]);
    std::sort(out.begin(), out.end());
    const int64_t m = std::min(nt, cap);
    for (int64_t i = 0; i < m; ++i) memcpy(keys + i * 3, out[i].data(), 12);
    return HV_OK;
}

int hv_tsdf_unit_keys(hv_volume *v, int32_t *keys, int64_t cap, int64_t *n) {
    HV_REQUIRE(v != nullptr && n != nullptr, HV_ERR_INVALID, "hv_tsdf_unit_keys: null argument");
    int64_t nb = 0;
    int rc = hv_num_blocks(v, &nb);
    if (rc != HV_OK) return rc;
    *n = nb;
    if (keys == nullptr || nb == 0) return HV_OK;
    std::vector<uint64_t> bkeys((size_t)nb);
    HV_HIP(hipMemcpy(bkeys.data(), v->table.block_keys, sizeof(uint64_t) * nb, hipMemcpyDeviceToHost));
    const int64_t m = std::min(nb, cap);
    for (int64_t i = 0; i < m; ++i) hv_unpack_key(bkeys[i], keys[i * 3], keys[i * 3 + 1], keys[i * 3 + 2]);
    return HV_OK;
}

} // extern "C"
