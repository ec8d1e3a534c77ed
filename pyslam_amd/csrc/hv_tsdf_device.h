// Device code shared by the TSDF fuse kernels (hv_tsdf.hip) and the de-integration kernels (hv_deintegrate.hip): the frame
// conversion, the touch pass over an 8x8 sample patch, the per-voxel projection + predicate and the batch pack role.  One
// definition, so that a frame handed to hv_tsdf_deintegrate* is sampled exactly as hv_tsdf_integrate* sampled it.
#pragma once
#include "hv_common.h"

static constexpr int HV_TOUCH_FAN = 8; // lanes per depth sample in the online touch pass
static constexpr uint32_t HV_REC_ONE = 1u << 24; // observation count byte of a batch frame record's colour word

// packed colour word {byte0 = R, byte1 = G, byte2 = B}: a B, G, R source swaps bytes 0 and 2 (one v_perm_b32)
__device__ __forceinline__ uint32_t hv_colour_order(uint32_t c, int bgr) {
    return bgr ? __builtin_amdgcn_perm(0u, c, 0x03000102u) : c;
}

// Image::CreateDepthToCameraDistanceMultiplierFloatImage, evaluated per gather instead of tabulated.
__device__ __forceinline__ float hv_multiplier(const HvFrameParams &P, int u, int v) {
    const float xx = ((float)u - P.cx) * P.ffl_inv_x;
    const float yy = ((float)v - P.cy) * P.ffl_inv_y;
    return sqrtf(xx * xx + yy * yy + 1.0f);
}

__device__ __forceinline__ float hv_convert_depth(const HvFrameParams &P, const void *depth_raw, int64_t i) {
    float p = P.depth_is_u16 ? (float)((const uint16_t *)depth_raw)[i] : ((const float *)depth_raw)[i];
    p = p / P.depth_scale_f;
    if ((double)p >= P.depth_trunc_d) p = 0.0f;
    return p;
}

// Conservative test: can any voxel centre of unit (ux,uy,uz) project into this GPU's image tile?
// (Only used to skip units when the frame is tile-sharded across GPUs; with the default whole-image
// tile every touched unit is kept, exactly as in ScalableTSDFVolume::Integrate.)
__device__ inline bool hv_unit_hits_tile(const HvFrameParams &P, int32_t ux, int32_t uy, int32_t uz) {
    if (P.tile_u0 <= 0 && P.tile_v0 <= 0 && P.tile_u1 >= P.W && P.tile_v1 >= P.H) return true;
    const float len = (float)P.unit_length;
    const float o[3] = {(float)((double)ux * P.unit_length), (float)((double)uy * P.unit_length),
                        (float)((double)uz * P.unit_length)};
    float umin = 3.0e38f, umax = -3.0e38f, vmin = 3.0e38f, vmax = -3.0e38f;
    for (int c = 0; c < 8; ++c) {
        const float x = o[0] + ((c & 1) ? len : 0.0f), y = o[1] + ((c & 2) ? len : 0.0f), z = o[2] + ((c & 4) ? len : 0.0f);
        const float pz = P.ext[8] * x + P.ext[9] * y + P.ext[10] * z + P.ext[11];
        if (pz <= 1.0e-3f) return true; // straddles the camera plane: keep
        const float px = P.ext[0] * x + P.ext[1] * y + P.ext[2] * z + P.ext[3];
        const float py = P.ext[4] * x + P.ext[5] * y + P.ext[6] * z + P.ext[7];
        const float u = px * P.fx / pz + P.cx + 0.5f, v = py * P.fy / pz + P.cy + 0.5f;
        umin = fminf(umin, u); umax = fmaxf(umax, u);
        vmin = fminf(vmin, v); vmax = fmaxf(vmax, v);
    }
    // tiles on the image border extend outwards without bound: a touched unit that projects entirely outside the image (it
    // only has a sample's +/- sdf_trunc box in view) still belongs to exactly the ranks it is nearest to, so the union of the
    // ranks' units stays Open3D's set of opened units
    const bool u_ok = (P.tile_u0 <= 0 || umax + 2.0f >= (float)P.tile_u0) && (P.tile_u1 >= P.W || umin - 2.0f < (float)P.tile_u1);
    const bool v_ok = (P.tile_v0 <= 0 || vmax + 2.0f >= (float)P.tile_v0) && (P.tile_v1 >= P.H || vmin - 2.0f < (float)P.tile_v1);
    return u_ok && v_ok;
}

// ---- touch pass: PointCloud::CreateFromDepthImage(stride) + unit enumeration, all f64 -------------------------------
// One wave = one 8x8 patch of depth samples (32x32 pixels at stride 4), one lane = one sample: the f64 back-projection
// runs once per sample.  Neighbouring samples open the same few volume units, so the wave first reduces its samples'
// unit ranges to their bounding box, marks every unit some sample's range covers in a per-wave LDS bitmap of the box
// (ScalableTSDFVolume::Integrate opens exactly those), compacts the set bits and hands ONE lane per distinct unit to
// `visit(key, ux, uy, uz)`: all hash probes of a patch are in flight together and a unit is probed once per patch, not
// once per sample.  Boxes larger than HV_TOUCH_BOX_BITS units (a patch straddling a long depth discontinuity) take the
// per-sample loop with ballot de-duplication instead; P.touch_box_bits = 0 forces that path (tests).
static constexpr int HV_TOUCH_PATCH = 8;                   // samples per patch side
static constexpr int HV_TOUCH_BOX_BITS = 2048;             // units in the largest bitmap-enumerated box
static constexpr int HV_TOUCH_BOX_WORDS = HV_TOUCH_BOX_BITS / 32;
static_assert(HV_TOUCH_BOX_WORDS == HV_WAVE, "one bitmap word per lane");

struct HvTouchScratch { // per wave
    uint32_t bits[HV_TOUCH_BOX_WORDS];
    uint16_t list[HV_TOUCH_BOX_BITS];
};

__host__ __device__ inline int hv_touch_patches_1d(int extent, int stride) {
    return ((extent + stride - 1) / stride + HV_TOUCH_PATCH - 1) / HV_TOUCH_PATCH;
}
__host__ __device__ inline int hv_touch_patches(int W, int H, int stride) {
    return hv_touch_patches_1d(W, stride) * hv_touch_patches_1d(H, stride);
}
__host__ __device__ inline int hv_touch_patches(const HvFrameParams &P) { return hv_touch_patches(P.W, P.H, P.stride); }

template <typename Visit>
__device__ __forceinline__ void hv_touch_patch(const HvTable &table, const HvFrameParams &P, const void *depth_f, int patch,
                                               HvTouchScratch &scratch, Visit visit) {
    const int ns_w = (P.W + P.stride - 1) / P.stride;
    const int ns_h = (P.H + P.stride - 1) / P.stride;
    const int pw = hv_touch_patches_1d(P.W, P.stride);
    const int lane = hv_lane_id();
    const int sj = (patch % pw) * HV_TOUCH_PATCH + (lane & (HV_TOUCH_PATCH - 1));
    const int si = (patch / pw) * HV_TOUCH_PATCH + lane / HV_TOUCH_PATCH;
    int32_t lo[3] = {0, 0, 0}, hi[3] = {-1, -1, -1}; // empty range for lanes without a valid sample
    bool has = false;
    if (sj < ns_w && si < ns_h) {
        const int i = si * P.stride;
        const int j = sj * P.stride;
        float p = hv_convert_depth(P, depth_f, (int64_t)i * P.W + j);
        if (P.tiled && p > 0.0f) {
            // Tile-sharded volume: a sample far outside this GPU's image tile cannot open a unit that projects into the tile
            // (hv_unit_hits_tile would refuse every one of them) - leave before the double-precision back-projection.  The
            // sample opens units over an L-infinity box of +/- sdf_trunc per axis, so a corner / voxel centre of an opened unit lies
            // within rad = sqrt(3) (unit_length + sdf_trunc) of its point; for a point q that close, with camera
            // depth >= zn = p - rad > 0, |u_q - u_s| <= (rad / zn) (fx + |u_s - cx|) (same for v).  Border tiles extend
            // outwards without bound, as in hv_unit_hits_tile.
            const float rad = (float)((P.unit_length + P.sdf_trunc_d) * 1.7320508075688772) * 1.001f;
            const float zn = p - rad;
            if (zn > 0.05f) {
                const float k = rad / zn;
                const float mu = k * (P.fx + fabsf((float)j - P.cx)) + 4.0f, mv = k * (P.fy + fabsf((float)i - P.cy)) + 4.0f;
                const bool out_u = (P.tile_u0 > 0 && (float)j + mu < (float)P.tile_u0) || (P.tile_u1 < P.W && (float)j - mu >= (float)P.tile_u1);
                const bool out_v = (P.tile_v0 > 0 && (float)i + mv < (float)P.tile_v0) || (P.tile_v1 < P.H && (float)i - mv >= (float)P.tile_v1);
                if (out_u || out_v) p = 0.0f;
            }
        }
        if (p > 0.0f) {
            const double z = (double)p;
            const double x = ((double)j - P.cx_d) * z / P.fx_d;
            const double y = ((double)i - P.cy_d) * z / P.fy_d;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const double pw_r = ((P.pose[r * 4 + 0] * x + P.pose[r * 4 + 1] * y) + P.pose[r * 4 + 2] * z) + P.pose[r * 4 + 3];
                lo[r] = (int32_t)floor((pw_r - P.sdf_trunc_d) / P.unit_length);
                hi[r] = (int32_t)floor((pw_r + P.sdf_trunc_d) / P.unit_length);
            }
            has = hi[0] >= lo[0] && hi[1] >= lo[1] && hi[2] >= lo[2];
        }
    }
    if (!__any(has)) return;
    // bounding box of the patch's unit ranges
    int32_t blo[3], bhi[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        blo[r] = hv_wave_min(has ? lo[r] : INT32_MAX);
        bhi[r] = hv_wave_max(has ? hi[r] : INT32_MIN);
    }
    const int64_t d0 = (int64_t)bhi[0] - blo[0] + 1, d1 = (int64_t)bhi[1] - blo[1] + 1, d2 = (int64_t)bhi[2] - blo[2] + 1;
    const bool boxed = d0 <= P.touch_box_bits && d1 <= P.touch_box_bits && d2 <= P.touch_box_bits &&
                       d0 * d1 * d2 <= (int64_t)P.touch_box_bits;
    if (boxed) {
        const int e1 = (int)d1, e2 = (int)d2;
        scratch.bits[lane] = 0u;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (has) {
            for (int32_t x = lo[0]; x <= hi[0]; ++x)
                for (int32_t y = lo[1]; y <= hi[1]; ++y)
                    for (int32_t z = lo[2]; z <= hi[2]; ++z) {
                        const int c = ((x - blo[0]) * e1 + (y - blo[1])) * e2 + (z - blo[2]);
                        atomicOr(&scratch.bits[c >> 5], 1u << (c & 31));
                    }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // compact the set bits: lane l owns word l; its units go to list[prefix(l) ...]
        uint32_t word = scratch.bits[lane];
        const int cnt = __popc(word);
        int incl = cnt;
#pragma unroll
        for (int o = 1; o < HV_WAVE; o <<= 1) {
            const int up = __shfl_up(incl, o);
            if (lane >= o) incl += up;
        }
        const int total = __shfl(incl, HV_WAVE - 1);
        int at = incl - cnt;
        while (word) {
            const int b = __ffs((int)word) - 1;
            scratch.list[at++] = (uint16_t)(lane * 32 + b);
            word &= word - 1u;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        for (int n = lane; n < total; n += HV_WAVE) {
            const int c = scratch.list[n];
            const int32_t ux = blo[0] + c / (e1 * e2);
            const int32_t uy = blo[1] + (c / e2) % e1;
            const int32_t uz = blo[2] + c % e2;
            if (hv_key_in_range(ux, uy, uz)) {
                const unsigned long long key = hv_pack_key(ux, uy, uz);
                // unit-ownership sharding: another GPU fuses (and stores) this unit
                if (!(P.owner_world > 1 && hv_owner_of(key, P.owner_world) != P.owner_rank)) visit(key, ux, uy, uz);
            } else {
                atomicAdd(&table.counters[HV_CNT_DROPPED], 1);
            }
        }
        // the next patch of this wave (none today) would reuse the scratch: keep the phases ordered
        __builtin_amdgcn_wave_barrier();
        return;
    }
    // general path: every lane walks its own sample's units; per step the wave's distinct keys are visited once
    const int64_t n0 = (int64_t)hi[0] - lo[0] + 1, n1 = (int64_t)hi[1] - lo[1] + 1, n2 = (int64_t)hi[2] - lo[2] + 1;
    const int64_t count = has ? n0 * n1 * n2 : 0;
    for (int64_t k = 0; __any(k < count); ++k) {
        unsigned long long key = HV_EMPTY_KEY;
        int32_t ux = 0, uy = 0, uz = 0;
        if (k < count) {
            ux = lo[0] + (int32_t)(k / (n1 * n2));
            uy = lo[1] + (int32_t)((k / n2) % n1);
            uz = lo[2] + (int32_t)(k % n2);
            if (hv_key_in_range(ux, uy, uz)) {
                key = hv_pack_key(ux, uy, uz);
                if (P.owner_world > 1 && hv_owner_of(key, P.owner_world) != P.owner_rank) key = HV_EMPTY_KEY;
            } else {
                atomicAdd(&table.counters[HV_CNT_DROPPED], 1);
            }
        }
        // wave-level de-duplication (ballot + shuffle, no memory traffic)
        bool leader = false;
        unsigned long long remaining = __ballot(key != HV_EMPTY_KEY);
        while (remaining) {
            const int first = __ffsll((long long)remaining) - 1;
            const unsigned long long fkey = __shfl(key, first);
            const unsigned long long same = __ballot(key == fkey);
            if (lane == first) leader = true;
            remaining &= ~same;
        }
        if (leader) visit(key, ux, uy, uz);
    }
}

// One voxel update (UniformTSDFVolume::IntegrateWithDepthToCameraDistanceMultiplier's inner body) in two phases: the evaluation
// (hv_tsdf_eval_fast) decides whether the voxel is updated and with what - it needs only the frame -, hv_tsdf_apply folds it into the
// voxel state.  Splitting them lets the kernels fetch voxel planes only for lanes that really update something.
// a0 / b and a1 / b, both correctly rounded (bit-identical to the IEEE divisions the reference performs), sharing one
// refined reciprocal: v_rcp_f32 + one Newton step, then the quotient / residual / correction chain the compiler itself
// emits for an f32 division, minus v_div_scale / v_div_fixup, which are no-ops while the operands stay clear of the
// overflow / denormal bands.  Verified exhaustively-at-random on gfx950: 0 mismatches in 1.4e11 divisions with
// operands in 2^-60 .. 2^60 (tools/divtest.hip); callers guarantee b >= 2^-20 and |a| < 2^60.
__device__ __forceinline__ void hv_div2(float a0, float a1, float b, float &q0, float &q1) {
    float r = __builtin_amdgcn_rcpf(b);
    const float e = fmaf(-b, r, 1.0f);
    r = fmaf(e, r, r);
    float q = a0 * r;
    float rem = fmaf(-b, q, a0);
    q = fmaf(rem, r, q);
    rem = fmaf(-b, q, a0);
    q0 = fmaf(rem, r, q);
    q = a1 * r;
    rem = fmaf(-b, q, a1);
    q = fmaf(rem, r, q);
    rem = fmaf(-b, q, a1);
    q1 = fmaf(rem, r, q);
}

// a / b correctly rounded for operands clear of the overflow / denormal bands (same chain as hv_div2).
__device__ __forceinline__ float hv_div1(float a, float b) {
    float r = __builtin_amdgcn_rcpf(b);
    const float e = fmaf(-b, r, 1.0f);
    r = fmaf(e, r, r);
    float q = a * r;
    float rem = fmaf(-b, q, a);
    q = fmaf(rem, r, q);
    rem = fmaf(-b, q, a);
    return fmaf(rem, r, q);
}

__device__ __forceinline__ void hv_tsdf_apply(bool valid, float t, uint32_t c, float &tsdf, uint32_t &w, uint32_t &sr,
                                              uint32_t &sg, uint32_t &sb) {
    if (!valid) return;
    const float wf = (float)w;
    // |tsdf * wf + t| <= 2^24 + 1 and 1 <= wf + 1 <= 2^24 for w < 2^24: inside hv_div1's verified band; beyond
    // (a voxel observed 16.7 M times) fall back to the plain division
    const float num = tsdf * wf + t;
    tsdf = (w < (1u << 24)) ? hv_div1(num, wf + 1.0f) : num / (wf + 1.0f);
    w += 1u;
    sr += c & 255u;
    sg += (c >> 8) & 255u;
    sb += (c >> 16) & 255u;
}

// ---- Predicated ("fast") forms for the multi-frame sweep -------------------------------------------------------------
// Same arithmetic, no divergent control flow: every lane runs the whole chain and a single predicate selects the
// result, so the compiler can interleave the ZH voxels of a lane (ZH gathers in flight) and does not spend VALU slots on
// re-materialising phi values.  The two rare regimes the short division chains do not cover are picked out by
// wave-uniform tests in the caller, which then runs the EXACT forms: a voxel column that comes within 1 mm of the camera
// plane (hv_div2 wants pc2 >= 2^-20 when pc2 > 0) and voxels observed more than 2^24 - 64 times (integer weights).

// sqrtf(x), correctly rounded, for x >= 2^-96 (here: x >= 1): v_sqrt_f32 (1 ulp) + the compiler's own neighbour test,
// minus the denormal pre-scaling and the zero / infinity class fix-up it has to add for arbitrary operands.
__device__ __forceinline__ float hv_sqrt_ge1(float x) {
    const float s = __builtin_amdgcn_sqrtf(x);
    const float sd = __uint_as_float(__float_as_uint(s) - 1u);
    const float su = __uint_as_float(__float_as_uint(s) + 1u);
    const float vp = fmaf(-sd, s, x);
    const float vs = fmaf(-su, s, x);
    float r = (vp <= 0.0f) ? sd : s;
    r = (vs > 0.0f) ? su : r;
    return r;
}

// EXACT = false: operands inside hv_div2's band (the caller's wave-uniform test), whole-image frames.
// EXACT = true: any operands (IEEE division where pc2 < 2^-20) and the image-tile test of the tile-sharded mode.
// MT: take the multiplier from the per-pixel table instead of computing it.
// REC12: frame_px points at 12-byte {depth, colour, multiplier} records (the fold form's batch layout) instead of 8-byte
// {depth, colour} records beside the multiplier table.
template <bool EXACT, bool MT, bool REC12 = false>
__device__ __forceinline__ bool hv_tsdf_eval_fast(const HvFrameParams &P, const uint2 *__restrict__ frame_px,
                                                  const float *__restrict__ mult, float pc0, float pc1, float pc2,
                                                  float &t, uint32_t &rgb) {
    const float a0 = pc0 * P.fx, a1 = pc1 * P.fy;
    float q0, q1;
    hv_div2(a0, a1, pc2, q0, q1); // pc2 <= 0: inf / NaN / a mirrored pixel, rejected by the pc2 > 0 term below
    if (EXACT) {
        const bool tiny = !(pc2 >= 0x1p-20f);
        const float e0 = a0 / pc2, e1 = a1 / pc2;
        q0 = tiny ? e0 : q0;
        q1 = tiny ? e1 : q1;
    }
    const float u_f = q0 + P.cx + 0.5f;
    const float v_f = q1 + P.cy + 0.5f;
    // u_f in [0.0001, safe_width) as ONE unsigned compare: for non-negative floats the bit patterns order like the
    // values, and a negative / NaN operand has a pattern above every finite positive one
    const uint32_t lo = __float_as_uint(0.0001f);
    const bool in_u = (__float_as_uint(u_f) - lo) < (__float_as_uint(P.safe_width_f) - lo);
    const bool in_v = (__float_as_uint(v_f) - lo) < (__float_as_uint(P.safe_height_f) - lo);
    bool ok = (int)(pc2 > 0.0f) & (int)in_u & (int)in_v;
    const int u = (int)u_f; // saturating conversions: garbage lanes stay defined
    const int v = (int)v_f;
    if (EXACT && P.tiled) {
        const bool in_tile_u = (int)(u >= P.tile_u0) & (int)(u < P.tile_u1);
        const bool in_tile_v = (int)(v >= P.tile_v0) & (int)(v < P.tile_v1);
        ok = (int)ok & (int)in_tile_u & (int)in_tile_v;
    }
    const uint32_t off = ok ? (uint32_t)v * (uint32_t)P.W + (uint32_t)u : 0u;
    uint2 rec;
    float m;
    if (REC12) {
        const uint32_t *r3 = (const uint32_t *)frame_px + (size_t)off * 3;
        rec = make_uint2(r3[0], r3[1]);
        m = __uint_as_float(r3[2]);
    } else {
        rec = frame_px[off];
    }
    const float d = __uint_as_float(rec.x);
    if (REC12) {
    } else if (MT) {
        m = mult[off];
    } else {
        const float xx = ((float)u - P.cx) * P.ffl_inv_x;
        const float yy = ((float)v - P.cy) * P.ffl_inv_y;
        m = hv_sqrt_ge1(xx * xx + yy * yy + 1.0f);
    }
    const float sdf = (d - pc2) * m;
    ok = (int)ok & (int)(d > 0.0f) & (int)(sdf > -P.sdf_trunc_f);
    t = fminf(sdf * P.sdf_trunc_inv_f, 1.0f); // == `if (t > 1) t = 1` for the non-NaN t of an accepted voxel
    rgb = rec.y;
    return ok;
}

// Running mean with the weight carried as a float (exact below 2^24): no int->float conversion and one add less per
// update; the caller converts back once per unit.
__device__ __forceinline__ void hv_tsdf_apply_fast(bool ok, float t, uint32_t rgb, float &tsdf, float &wf, uint32_t &sr,
                                                   uint32_t &sg, uint32_t &sb) {
    const float wf1 = wf + 1.0f;
    const float nt = hv_div1(tsdf * wf + t, wf1);
    tsdf = ok ? nt : tsdf;
    wf = ok ? wf1 : wf;
    const uint32_t c = ok ? rgb : 0u;
    sr += c & 255u;
    sg += (c >> 8) & 255u;
    sb += (c >> 16) & 255u;
}

// Pack role of the multi-frame path: pixels [i0, i0 + 4) of frame f -> frame records (4 pixels per thread: one 16-byte depth load -
// 8 for uint16 -, three dwords of RGB, two / three 16-byte record stores).
__device__ __forceinline__ void hv_pack_px4(const HvFrameParams &P, const int f, const int64_t i0, const void *depth_f,
                                            const uint8_t *rgb_f, uint2 *__restrict__ frame_px, const float *__restrict__ mult12) {
    const int64_t npx = (int64_t)P.H * P.W;
    if (i0 >= npx) return;
    if (P.tiled && (P.W & 3) == 0) {
        // tile-sharded volume: only voxels that project into this GPU's tile gather a record (the sweep's image-range test
        // uses the tile's bounds), so only the tile's columns and rows are packed (+ 4 pixels: a garbage lane may read
        // outside, its value is never used)
        const int u = (int)(i0 % P.W), v = (int)(i0 / P.W);
        if (u + 3 < P.tile_u0 - 4 || u >= P.tile_u1 + 4 || v < P.tile_v0 - 4 || v >= P.tile_v1 + 4) return;
    }
    uint2 *dst = frame_px + (int64_t)f * npx + i0;
    // mult12 != nullptr: 12-byte records {depth, colour, multiplier} (the column sweep gathers a voxel's pixel with ONE load; the
    // multiplier comes from the per-pixel table, which is built before this launch); else 8-byte {depth, colour} records beside the
    // table (the bitwise sweep form)
    uint32_t *dst12 = (uint32_t *)frame_px + ((int64_t)f * npx + i0) * 3;
    if (i0 + 4 <= npx && (npx & 3) == 0) {
        const uint32_t *c4 = (const uint32_t *)(rgb_f + i0 * 3); // i0 % 4 == 0 -> 12-byte multiple: dword aligned
        const uint32_t w0 = c4[0], w1 = c4[1], w2 = c4[2];
        // byte 3 of a batch record's colour word is 1: the fold form of the sweep adds accepted records' words into packed
        // accumulators and that byte counts the observations (every other consumer masks the colour bytes out)
        const uint32_t col[4] = {hv_colour_order(w0 & 0xffffffu, P.bgr) | HV_REC_ONE,
                                 hv_colour_order((w0 >> 24) | ((w1 & 0xffffu) << 8), P.bgr) | HV_REC_ONE,
                                 hv_colour_order((w1 >> 16) | ((w2 & 0xffu) << 16), P.bgr) | HV_REC_ONE,
                                 hv_colour_order(w2 >> 8, P.bgr) | HV_REC_ONE};
        float d[4];
        if (P.depth_is_u16) {
            const uint2 raw = *(const uint2 *)((const uint16_t *)depth_f + i0);
            d[0] = (float)(raw.x & 0xffffu); d[1] = (float)(raw.x >> 16);
            d[2] = (float)(raw.y & 0xffffu); d[3] = (float)(raw.y >> 16);
        } else {
            const float4 raw = *(const float4 *)((const float *)depth_f + i0);
            d[0] = raw.x; d[1] = raw.y; d[2] = raw.z; d[3] = raw.w;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) { // hv_convert_depth
            d[k] = d[k] / P.depth_scale_f;
            if ((double)d[k] >= P.depth_trunc_d) d[k] = 0.0f;
        }
        if (mult12 != nullptr) {
            const float4 m4 = *(const float4 *)(mult12 + i0);
            ((uint4 *)dst12)[0] = make_uint4(__float_as_uint(d[0]), col[0], __float_as_uint(m4.x), __float_as_uint(d[1]));
            ((uint4 *)dst12)[1] = make_uint4(col[1], __float_as_uint(m4.y), __float_as_uint(d[2]), col[2]);
            ((uint4 *)dst12)[2] = make_uint4(__float_as_uint(m4.z), __float_as_uint(d[3]), col[3], __float_as_uint(m4.w));
        } else {
            ((uint4 *)dst)[0] = make_uint4(__float_as_uint(d[0]), col[0], __float_as_uint(d[1]), col[1]);
            ((uint4 *)dst)[1] = make_uint4(__float_as_uint(d[2]), col[2], __float_as_uint(d[3]), col[3]);
        }
    } else {
        for (int64_t i = i0; i < npx && i < i0 + 4; ++i) {
            const uint8_t *c = rgb_f + i * 3;
            uint2 rec;
            rec.x = __float_as_uint(hv_convert_depth(P, depth_f, i));
            rec.y = hv_colour_order((uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16), P.bgr) | HV_REC_ONE;
            if (mult12 != nullptr) {
                uint32_t *r3 = (uint32_t *)frame_px + ((int64_t)f * npx + i) * 3;
                r3[0] = rec.x;
                r3[1] = rec.y;
                r3[2] = __float_as_uint(mult12[i]);
            } else {
                frame_px[(int64_t)f * npx + i] = rec;
            }
        }
    }
}

// Frame-grouped pack role of the batch path's 12-byte records: pixels [i0, i0 + 4) of the HV_PACK_FRAMES consecutive frames from f0 (a
// wave's lanes hold consecutive quads, so every wave access is one frame's contiguous 1 KB of depth, 768 B of RGB or 3 KB of records).
// The multiplier quad is loaded once, then every frame's depth quad and three RGB dwords are issued before the first of them is waited
// for.  The group size and the depth type are compile-time so that the loads stand in one straight block (a frame count or a depth type
// only known at run time puts a branch and a full wait between the frames).  The caller guarantees a whole quad inside the image.
// The records are byte for byte hv_pack_px4's: hv_convert_depth's operations, the same colour order and count byte.
// STAGE (every lane of the wave is here): the wave's 3 KB of records of a frame go through `stage` (3 KB of LDS of the wave's own), so
// that each of the three store instructions writes 1 KB contiguously; straight from the registers a lane's 16 bytes lie 48 bytes apart
// and every instruction touches all 24 lines.  Alone the launch of a 64-frame batch takes 129 us with it, 145 us without
// (profiles/pack_groups).
static constexpr int HV_PACK_FRAMES = 2; // frames per pack thread (4: one more register granule and slower, profiles/pack_groups)

template <bool U16, bool STAGE>
__device__ __forceinline__ void hv_pack_px4_frames(const HvFrameParams &P, const int f0, const int64_t i0, const char *depth_raw,
                                                   const int64_t depth_stride, const uint8_t *rgb, uint2 *__restrict__ frame_px,
                                                   const float *__restrict__ mult12, uint4 *stage) {
    constexpr int NF = HV_PACK_FRAMES;
    const int64_t npx = (int64_t)P.H * P.W;
    const float4 m = *(const float4 *)(mult12 + i0);
    uint4 raw[NF]; // depth as loaded: four floats, or four uint16 in .x and .y
    uint32_t w[NF][3];
#pragma unroll
    for (int k = 0; k < NF; ++k) {
        const char *depth_f = depth_raw + (int64_t)(f0 + k) * depth_stride;
        if (U16) {
            const uint2 r2 = *(const uint2 *)((const uint16_t *)depth_f + i0);
            raw[k] = make_uint4(r2.x, r2.y, 0u, 0u);
        } else {
            raw[k] = *(const uint4 *)((const float *)depth_f + i0);
        }
        const uint32_t *c4 = (const uint32_t *)(rgb + ((int64_t)(f0 + k) * npx + i0) * 3); // a multiple of 12 bytes: dword aligned
        w[k][0] = c4[0]; w[k][1] = c4[1]; w[k][2] = c4[2];
    }
#pragma unroll
    for (int k = 0; k < NF; ++k) {
        float d[4];
        if (U16) {
            d[0] = (float)(raw[k].x & 0xffffu); d[1] = (float)(raw[k].x >> 16);
            d[2] = (float)(raw[k].y & 0xffffu); d[3] = (float)(raw[k].y >> 16);
        } else {
            d[0] = __uint_as_float(raw[k].x); d[1] = __uint_as_float(raw[k].y);
            d[2] = __uint_as_float(raw[k].z); d[3] = __uint_as_float(raw[k].w);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) { // hv_convert_depth
            d[j] = d[j] / P.depth_scale_f;
            if ((double)d[j] >= P.depth_trunc_d) d[j] = 0.0f;
        }
        const uint32_t w0 = w[k][0], w1 = w[k][1], w2 = w[k][2];
        const uint32_t col[4] = {hv_colour_order(w0 & 0xffffffu, P.bgr) | HV_REC_ONE,
                                 hv_colour_order((w0 >> 24) | ((w1 & 0xffffu) << 8), P.bgr) | HV_REC_ONE,
                                 hv_colour_order((w1 >> 16) | ((w2 & 0xffu) << 16), P.bgr) | HV_REC_ONE,
                                 hv_colour_order(w2 >> 8, P.bgr) | HV_REC_ONE};
        const uint4 r0 = make_uint4(__float_as_uint(d[0]), col[0], __float_as_uint(m.x), __float_as_uint(d[1]));
        const uint4 r1 = make_uint4(col[1], __float_as_uint(m.y), __float_as_uint(d[2]), col[2]);
        const uint4 r2 = make_uint4(__float_as_uint(m.z), __float_as_uint(d[3]), col[3], __float_as_uint(m.w));
        uint4 *dst12 = (uint4 *)((uint32_t *)frame_px + ((int64_t)(f0 + k) * npx + i0) * 3);
        if (STAGE) {
            const int lane = hv_lane_id();
            stage[lane * 3 + 0] = r0; stage[lane * 3 + 1] = r1; stage[lane * 3 + 2] = r2;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const uint4 a = stage[lane], b = stage[HV_WAVE + lane], c = stage[2 * HV_WAVE + lane];
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier(); // (the next frame's records overwrite the stage)
            uint4 *base = dst12 - lane * 3; // lane 0's records: the wave's 192 uint4 follow each other
            base[lane] = a; base[HV_WAVE + lane] = b; base[2 * HV_WAVE + lane] = c;
        } else {
            dst12[0] = r0; dst12[1] = r1; dst12[2] = r2;
        }
    }
}

// ---- host side (hv_tsdf.hip), shared with hv_deintegrate.hip ----
static constexpr int HV_BATCH_MAX = 64; // frames per sweep (one bit per frame in a unit's mask)
int make_frame_params(hv_volume *v, int H, int W, const double *intr, const double *T_cw, double depth_scale, double depth_trunc,
                      int depth_dtype, HvFrameParams *P);
int tsdf_multiplier_table(hv_volume *v, const HvFrameParams &P); // v->mult_table for P's intrinsics and image size
int tsdf_rectify(hv_volume *v, hipStream_t s, const void **depth, int depth_dtype, const uint8_t **rgb, int B, int H, int W);
int check_tsdf_args(hv_volume *v, const void *depth, const uint8_t *rgb, int H, int W, const double *intr, const double *T_cw,
                    int frames);
size_t tsdf_batch_scratch(size_t rec_bytes, size_t npx, int B, size_t *params_offset); // bytes of a multi-frame call's scratch
int tsdf_integrate_batch_impl(hv_volume *v, const void *depth, const void *const *depth_ptrs, int32_t depth_dtype, const uint8_t *rgb,
                              const void *const *rgb_ptrs, int32_t n_frames, int32_t height, int32_t width, const double *intr,
                              const double *T_cw, double depth_scale, double depth_trunc, int32_t loc);
