/*
 * hipvol.h — C ABI of libpyslam_hipvol.so, the MI355X-native (gfx950) volumetric fusion library.
 *
 * This is the drop-in boundary for pySLAM's dense-mapping hot path.  Each entry point states the
 * reference interface it replaces (paths relative to the pySLAM tree):
 *
 *   VOXEL_GRID mode  == the `volumetric` pybind11 module's VoxelBlockGrid
 *                       (cpp/volumetric/volumetric_grid_module.h:732-935, voxel_block_grid.h:61-234)
 *   TSDF mode        == open3d.pipelines.integration.ScalableTSDFVolume as pySLAM drives it
 *                       (pyslam/dense/volumetric_integrator_tsdf.py:104-108, 215-223, 239-267)
 *
 * Conventions
 *   - plain C types only; all pointers are borrowed for the duration of the call;
 *   - every function returns HV_OK (0) or a negative hv_status; hv_last_error() gives the message
 *     of the last failure on the calling thread (mirrors the std::runtime_error text the pybind
 *     module would raise, e.g. "points must be a contiguous Nx3 array");
 *   - `loc` says where the *input/output arrays* live: HV_HOST (the library stages them through
 *     HBM itself) or HV_DEVICE (already resident in HBM on the volume's device; zero-copy);
 *   - a volume is owned by one host thread at a time (pySLAM runs all volume access on the single
 *     thread of its VolumetricIntegratorProcess, volumetric_integrator_base.py:789-967);
 *   - all GPU work is enqueued on the volume's HIP stream; calls that return data to the host
 *     synchronise that stream, the integrate calls do not.
 *   - there is NO CPU fallback: hv_create fails if no gfx950 device is usable.
 */
#ifndef PYSLAM_HIPVOL_H
#define PYSLAM_HIPVOL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hv_volume hv_volume;

typedef enum hv_status {
    HV_OK = 0,
    HV_ERR_INVALID = -1,   /* bad argument (message mirrors the pybind module's) */
    HV_ERR_DEVICE = -2,    /* HIP runtime failure / no gfx950 device */
    HV_ERR_CAPACITY = -3,  /* block pool, hash table or scratch capacity exceeded */
    HV_ERR_MODE = -4       /* call not valid for this volume's mode */
} hv_status;

/* Values match pySLAM's VolumetricIntegratorType (pyslam/dense/volumetric_integrator_types.py:8-21). */
typedef enum hv_mode {
    HV_MODE_VOXEL_GRID = 0,
    HV_MODE_VOXEL_SEMANTIC_GRID = 1,               /* voting payload */
    HV_MODE_VOXEL_SEMANTIC_PROBABILISTIC_GRID = 2, /* log-probability payload */
    HV_MODE_TSDF = 3,
    /* the two "*2" payload variants the reference's module also binds (volumetric_grid_module.h:1014-1032,
     * voxel_block_semantic_grid.h:120-123); pySLAM's VolumetricIntegratorType has no entry for them (4 is GAUSSIAN_SPLATTING) */
    HV_MODE_VOXEL_SEMANTIC_GRID2 = 11,               /* separate object / class counters, voxel_data_semantic2.h:46-196 */
    HV_MODE_VOXEL_SEMANTIC_PROBABILISTIC_GRID2 = 12  /* marginal object / class label maps, voxel_data_semantic2.h:256-787 */
} hv_mode;
typedef enum hv_loc { HV_HOST = 0, HV_DEVICE = 1 } hv_loc;
typedef enum hv_color_dtype { HV_COLOR_NONE = 0, HV_COLOR_U8 = 1, HV_COLOR_F32 = 2 } hv_color_dtype;
typedef enum hv_depth_dtype { HV_DEPTH_F32 = 0, HV_DEPTH_U16 = 1 } hv_depth_dtype;

typedef struct hv_config {
    int32_t mode;          /* hv_mode */
    int32_t device;        /* HIP device ordinal */
    /* VOXEL_GRID: VoxelBlockGrid(voxel_size: float, block_size=8) — voxel_block_grid.hpp:4-9.
     * TSDF: ScalableTSDFVolume(voxel_length, sdf_trunc, RGB8, volume_unit_resolution=16,
     *       depth_sampling_stride=4) — volumetric_integrator_tsdf.py:104-108. */
    double voxel_size;     /* metres (narrowed to float in VOXEL_GRID mode, as pybind does) */
    double sdf_trunc;      /* TSDF only */
    int32_t block_size;    /* voxels per block side: 8 (VOXEL_GRID) / 16 (TSDF unit resolution) */
    int32_t depth_sampling_stride; /* TSDF only (Open3D default 4) */
    int64_t max_blocks;    /* block/unit pool capacity (HBM = max_blocks * bytes_per_block) */
    int64_t max_points;    /* largest point batch / H*W accepted by one integrate call */
} hv_config;

/* Camera: pinhole intrinsics {fx, fy, cx, cy} as doubles and T_cw (world->camera) as a row-major
 * 4x4 double — exactly what pySLAM hands over (keyframe.pose(), volumetric_integrator_base.py:116). */

const char *hv_last_error(void);
int hv_device_count(void);                       /* usable gfx950 devices, or negative hv_status */
void hv_default_config(int32_t mode, hv_config *cfg);

int hv_create(const hv_config *cfg, hv_volume **out);
void hv_destroy(hv_volume *v);
int hv_reset(hv_volume *v);                      /* VoxelBlockGrid.clear()/reset(), ScalableTSDFVolume.reset() */
int hv_synchronize(hv_volume *v);
int hv_set_stream(hv_volume *v, void *hip_stream); /* adopt a caller-owned hipStream_t (e.g. a torch stream) */
void *hv_get_stream(hv_volume *v);

/* ---- common introspection (volumetric_grid_module.h:761-812) ---------------------------------- */
int hv_num_blocks(hv_volume *v, int64_t *n);     /* num_blocks() / number of TSDF volume units */
int hv_block_size(hv_volume *v, int32_t *bs);    /* get_block_size() */
/* Grow the block pool + hash to new_max_blocks, keeping the contents (no-op when not larger).  The library also
 * doubles the pool by itself whenever a data-returning call finds it more than half full and the larger pool fits
 * into free HBM (HV_AUTO_GROW=0 disables this); the reference's containers grow without bound, so must the map. */
int hv_reserve_blocks(hv_volume *v, int64_t new_max_blocks);
int hv_max_blocks(hv_volume *v, int64_t *n);
int hv_bytes_per_block(hv_volume *v, int64_t *bytes);
int hv_dropped_points(hv_volume *v, int64_t *n); /* points/pixels rejected because their block key fell
                                                    outside the +/-2^20 packed range (never for sane maps) */

/* ---- VOXEL_GRID mode ---------------------------------------------------------------------------
 * hv_integrate_points == VoxelBlockGrid.integrate(points f32 [N,3], colors u8|f32 [N,3] | None)
 *   (volumetric_grid_module.h:743-749 -> integrate_raw, voxel_block_grid.hpp:115-136).
 *   Result is bit-identical to the reference's sequential (point-index-order) accumulation. */
int hv_integrate_points(hv_volume *v, const float *points, int64_t n, const void *colors,
                        int32_t color_dtype, int32_t loc);
/* The binding's float64 overload (volumetric_grid_module.h:738-741 -> integrate_raw<double, ...>): voxel keys come from the
 * doubles (floor(x * (double)inv_voxel_size)), the voxel sums take static_cast<float>(x) (voxel_data.h:54-56). */
int hv_integrate_points_f64(hv_volume *v, const double *points, int64_t n, const void *colors,
                            int32_t color_dtype, int32_t loc);

/* Fused L3 prep + integrate for one posed RGB-D frame: depth2pointcloud (pyslam/utilities/depth.py:
 * 45-85) + world transform (volumetric_integrator_voxel_grid.py:262-281) + integrate, without the
 * host round trip.  rgb is H*W*3 u8 (already RGB), depth H*W f32 metres (or u16 * depth_scale^-1).
 * Pixels with depth <= min_depth or >= max_depth are skipped (depth.py:64). */
int hv_integrate_rgbd_points(hv_volume *v, const void *depth, int32_t depth_dtype, double depth_scale,
                             const uint8_t *rgb, int32_t height, int32_t width, const double *intr,
                             const double *T_cw, double min_depth, double max_depth, int32_t loc);

/* Batched replay of F posed frames (rebuild(), offline reconstruction): depth F*H*W, rgb F*H*W*3, T_cw F*16 (host).
 * Bit-identical to F hv_integrate_rgbd_points calls; one sort + reduce per chunk of max_points / (H*W) frames. */
int hv_integrate_rgbd_points_batch(hv_volume *v, const void *depth, int32_t depth_dtype, double depth_scale,
                                   const uint8_t *rgb, int32_t n_frames, int32_t height, int32_t width, const double *intr,
                                   const double *T_cw, double min_depth, double max_depth, int32_t loc);

/* cv2.remap(src, map_x, map_y, INTER_LINEAR | INTER_NEAREST, BORDER_CONSTANT 0) as pySLAM's undistortion
 * uses it (volumetric_integrator_base.py:1017-1043).  src_kind 0: uint8 (channels interleaved), 1: float32,
 * 2: int32 (nearest only); maps float32 [H,W] - the image's own height and width, the caller checks that; all arrays live at
 * `loc`.  OpenCV semantics restated, unpinned (tests/remap_reference.py states them once more, tests/test_gpu_remap_planted.py):
 *   coordinates  r = round-half-to-even of the float32 map entry (nearest) or of 32 times it, multiplied in float32 (linear).  An
 *                entry that is NaN or +-inf, or whose r does not fit int32, is OUTSIDE the image.
 *   border       constant 0 (0.0 for float32) for every tap outside [0,H) x [0,W).
 *   nearest      dst = src[r(map_y), r(map_x)]; values are copied, never converted.
 *   linear       sx = r(32 map_x): ix = sx >> 5, fx = sx & 31 (arithmetic shift, two's-complement mask), the same in y; uint8: integer
 *                weights (32-fx)(32-fy)32 ... summing to 2^15, (sum + 2^14) >> 15; float32: the weights (1-fx/32)(1-fy/32) ...,
 *                four products added in float32 in the order (0,0) (0,1) (1,0) (1,1) (a zero weight times inf is NaN). */
int hv_remap(hv_volume *v, const void *src, int32_t src_kind, int32_t channels, int32_t height, int32_t width,
             const float *map_x, const float *map_y, int32_t linear, void *dst, int32_t loc);

/* filter_shadow_points(depth, delta_depth=None, delta_x=2, delta_y=2, fill_value=-1)
 * (pyslam/utilities/depth.py:103-146): MAD-thresholded depth-discontinuity filter, bit-identical to
 * the numpy reference for float32 depth.  Works on any volume (uses its stream and scratch).  Host images (loc =
 * HV_HOST) are complete on return; with HV_DEVICE the launches are queued on the volume's stream (hv_get_stream) and the
 * call returns without waiting, like the integrate entry points. */
int hv_filter_shadow_points(hv_volume *v, const float *depth, int32_t height, int32_t width, int32_t delta_x,
                            int32_t delta_y, float fill_value, float *out, int32_t loc);
/* The same filter on DEVICE images, queued on the caller's HIP stream (`stream` = a hipStream_t) instead of the volume's, with
 * scratch of its own: the filter reads nothing of the volume, so a front can run it on its upload side - keyframe k + 1's depth is
 * filtered while keyframe k is fused (pyslam_amd/dense/device_pipeline.py).  The caller orders `out` against its consumers (an
 * event on `stream`).  Same reference: pyslam/utilities/depth.py filter_shadow_points, as called at
 * pyslam/dense/volumetric_integrator_voxel_grid.py:235 / volumetric_integrator_voxel_semantic_grid.py:334. */
int hv_filter_shadow_points_on_stream(hv_volume *v, const float *depth, int32_t height, int32_t width, int32_t delta_x,
                                      int32_t delta_y, float fill_value, float *out, void *stream);

/* ---- census semi-global stereo matching ------------------------------------------------------------
 * hv_stereo_sgm: a rectified uint8 pair -> disparity (int16, sixteenths of a pixel, -16 = invalid: the format of
 * cv2.StereoSGBM.compute, so disparity / 16 works as in pyslam/depth_estimation/depth_estimator_base.py:69-131
 * DepthEstimatorSgbm) and metric depth (float32, 0 = none).  The weight-free stereo estimator of the package: OpenCV is not a
 * dependency and parity with its SGBM is not claimed; the algorithm is fixed by the rules below, restated in numpy in
 * tests/stereo_reference.py, and the library is held to that restatement bit for bit.  Integer arithmetic except rule 10;
 * D = num_disparities, the minimum disparity is 0.
 *   1 grey        one channel as is; three channels g = (c0 + 2 c1 + c2 + 2) >> 2 (the same for RGB and BGR)
 *   2 census      window 9 wide x 7 high, centred, centre excluded (62 bits); bit = neighbour < centre; pixels outside the image
 *                 take the nearest edge pixel
 *   3 cost        C(y,x,d) = popcount(censusL(y,x) ^ censusR(y,x-d)) for x - d >= 0, else 64
 *   4 paths       4: left->right, right->left, top->bottom, bottom->top; 8: and the four diagonals.  With q the pixel before p on
 *                 the path and M(q) = min_k L(q,k):  L(p,d) = C(p,d) + min(L(q,d), L(q,d-1) + P1, L(q,d+1) + P1, M(q) + P2) - M(q),
 *                 the d-1 / d+1 terms absent outside [0,D);  L(p,d) = C(p,d) where q lies outside the image.  S = the sum of L over
 *                 the paths (0 < P1 <= P2 <= 1023: S <= 8 (64 + P2) fits uint16)
 *   5 winner      d* = the smallest d attaining min_d S(p,d)
 *   6 uniqueness  invalid if some d with |d - d*| > 1 has S(p,d) (100 - uniqueness_ratio) < S(p,d*) 100
 *   7 left-right  (max_diff >= 0; a negative value disables the rule)  dR(y,xr) = the smallest d attaining the minimum of
 *                 S(y,xr+d,d) over xr + d < W;  invalid if x - d* < 0 or |dR(y,x-d*) - d*| > max_diff
 *   8 sub-pixel   for 0 < d* < D-1: den = max(S(d*-1) + S(d*+1) - 2 S(d*), 1), d16 = 16 d* + ((S(d*-1) - S(d*+1)) 16 + den) / (2 den)
 *                 with C division (toward zero); otherwise d16 = 16 d*
 *   9 disparity   d16 for valid pixels, -16 for invalid ones
 *  10 depth       (bf * 16f) / float(d16): one float32 multiply, one correctly rounded divide; 0 where d16 <= 0, where the result is
 *                 < min_depth, or > max_depth when max_depth is finite
 * The speckle filter of cv2.StereoSGBM (speckleWindowSize, speckleRange) is a step of its own: hv_stereo_sgm_speckle runs it on the
 * disparity of rule 9 before anything leaves the device, hv_filter_speckles on any image (both below).
 * left / right: [height,width] (channels 1) or [height,width,3] uint8, both outputs [height,width]; either output may be NULL, not
 * both.  `loc` as in hv_filter_shadow_points: host arrays are complete on return, a device call is queued on the volume's stream
 * and returns.  Works on a volume of any mode and reads nothing of it.  Scratch is owned by the handle, grown on demand and freed by
 * hv_destroy: height width (2 num_disparities + 22) bytes (S uint16, two census images, the left winners and the right image's
 * best keys), each part rounded up to 256 bytes.
 * HV_ERR_INVALID before anything is launched or written: a NULL image or params, both outputs NULL, channels not 1 or 3, height or
 * width < 1 (or > 32768, or 2^30 pixels and more), num_disparities not a multiple of 16 in 16..256, not 0 < p1 <= p2 <= 1023,
 * uniqueness_ratio outside 0..99, paths not 4 or 8, bf not finite and positive while depth_out is given.  HV_ERR_CAPACITY when the
 * scratch cannot be allocated. */
typedef struct hv_stereo_params {
    int32_t num_disparities;  /* 128 */
    int32_t p1, p2;           /* 10, 120 */
    int32_t uniqueness_ratio; /* 15 */
    int32_t max_diff;         /* 1 */
    int32_t paths;            /* 8 */
    float bf;                 /* baseline times focal length, metres x pixels (read only when depth_out is given) */
    float min_depth, max_depth; /* 0, +inf */
} hv_stereo_params;
int hv_stereo_sgm(hv_volume *v, const uint8_t *left, const uint8_t *right, int32_t height, int32_t width, int32_t channels,
                  const hv_stereo_params *params, int16_t *disparity_out /* may be NULL */, float *depth_out /* may be NULL */,
                  int32_t loc);

/* ---- speckle filter: small connected regions of a disparity or depth image ------------------------------
 * hv_filter_speckles: the rule of cv2.filterSpeckles(img, newVal, maxSpeckleSize, maxDiff), as cv2.StereoSGBM.compute applies it
 * to its disparity (pyslam/depth_estimation/depth_estimator_base.py:97-108 sets speckleWindowSize = 50, speckleRange = 1).  OpenCV
 * is not a dependency: parity is by rule, restated in numpy in tests/speckle_reference.py, and the library is held to that
 * restatement bit for bit (tests/golden/speckle_opencv.npz pins it to OpenCV wherever tools/make_golden_speckle.py has run).
 * image: [height,width] of kind HV_SPECKLE_I16 (disparity in sixteenths) or HV_SPECKLE_F32 (depth).
 *   S1 valid      a pixel is valid iff value != new_val: an integer compare for int16, the IEEE compare for float32 (NaN is valid;
 *                 -0.0 is invalid when new_val is 0.0).  new_val is converted to the image's type: for int16 it must be an integer in
 *                 -32768..32767, for float32 it is rounded to float32
 *   S2 link       two 4-neighbours link iff both are valid and |a - b| <= max_diff.  int16: the difference is taken in int32 (-32768
 *                 against 32767 is 65535, no wrap) and compared with floor(max_diff); float32: fabsf(a - b) <= (float)max_diff in
 *                 float32 (NaN and inf - inf never link).  The comparison is between ADJACENT pixels, not against a seed
 *   S3 component  the classes of the transitive closure of S2 over the valid pixels
 *   S4 label      the smallest row-major index y width + x in the component; -1 for an invalid pixel
 *   S5 size       the component's pixel count (int32; height width < 2^30)
 *   S6 removal    every pixel of a component with size <= max_speckle_size is set to new_val; every other pixel is copied bit for
 *                 bit.  max_speckle_size = 0 removes nothing; labels and stats are produced all the same
 *   S7 depth      depth_inout (optional, float32 [height,width]) gets 0.0f where S6 removed the pixel, every other pixel keeps its bits
 * stats (all exact, independent of the order of execution): valid_pixels, components, largest (the largest size, 0 without a valid
 * pixel), removed_components, removed_pixels.
 * out: [height,width] of the image's kind, may be image itself (in place); labels_out: int32 [height,width].  `loc` as in
 * hv_filter_shadow_points: host arrays are staged by the library and complete on return; a device call is queued on the volume's
 * stream and returns - unless stats is given: the call then waits for the stream.  Works on a volume of any mode and reads nothing
 * of the map.  Scratch (a parent and a size array, 8 bytes per pixel) is owned by the handle, grown on demand and freed by
 * hv_destroy.
 * HV_ERR_INVALID before anything is launched or written: a NULL handle, image or out; a kind other than the two; height or width
 * < 1 or > 32768, or 2^30 pixels and more; max_speckle_size < 0; max_diff negative, NaN or infinite (int16: above 65535); an int16
 * new_val that is no integer of the type; an out, labels_out or depth_inout that overlaps image other than out == image exactly.
 * HV_ERR_CAPACITY when the scratch cannot be allocated.
 *
 * hv_stereo_sgm_speckle: hv_stereo_sgm followed, on the device, by the filter on the disparity of rule 9 with new_val = -16,
 * max_speckle_size = speckle_window_size and max_diff = 16 speckle_range (cv2.StereoSGBM's own call); depth_out (rule 10) is zeroed
 * by S7.  With host images the disparity does not visit the host between the two steps.  speckle_window_size in 1..2^30 (0 is
 * refused: hv_stereo_sgm is that call), speckle_range in 0..4095; everything else as hv_stereo_sgm.  stats (may be NULL, host
 * memory) are the filter's; when given, the call waits for the stream. */
typedef enum hv_speckle_kind { HV_SPECKLE_I16 = 0, HV_SPECKLE_F32 = 1 } hv_speckle_kind;
typedef struct hv_speckle_stats {
    int64_t valid_pixels, components, largest, removed_components, removed_pixels;
} hv_speckle_stats;
int hv_filter_speckles(hv_volume *v, const void *image, int32_t kind /* HV_SPECKLE_I16 | HV_SPECKLE_F32 */, int32_t height, int32_t width,
                       double new_val, int64_t max_speckle_size, double max_diff, void *out, float *depth_inout /* may be NULL */,
                       int32_t *labels_out /* may be NULL */, hv_speckle_stats *stats /* may be NULL, host */, int32_t loc);
int hv_stereo_sgm_speckle(hv_volume *v, const uint8_t *left, const uint8_t *right, int32_t height, int32_t width, int32_t channels,
                          const hv_stereo_params *params, int32_t speckle_window_size, int32_t speckle_range,
                          int16_t *disparity_out /* may be NULL */, float *depth_out /* may be NULL */,
                          hv_speckle_stats *stats /* may be NULL, host */, int32_t loc);

/* ---- plane-sweep depth for posed monocular keyframes ----------------------------------------------------
 * hv_mvs_sgm: a uint8 reference image and 1..4 source images of the same shape, each with a 3x4 matrix that takes the reference
 * pixel and an inverse depth to the source pixel -> the winning plane per reference pixel (int16, sixteenths of a plane, -16 =
 * invalid: the format of the stereo disparity, so hv_filter_speckles and every consumer of one take it as is) and metric z-depth in
 * the reference camera (float32, 0 = none).  The weight-free counterpart of the reference's multi-view estimators
 * (pyslam/depth_estimation/depth_estimator_mvdust3r.py, depth_estimator_mast3r.py) for a posed single-camera stream; parity with
 * a network is not claimed.  The algorithm is fixed by the rules below, restated in numpy in tests/mvs_reference.py, and the library
 * is held to that restatement bit for bit.  D = num_planes, N = n_sources; "stereo rule n" is rule n of hv_stereo_sgm above.
 *   M1 grey, census  stereo rules 1 and 2, unchanged, for the reference image and every source image
 *   M2 planes        the inverse depth of plane k is w_k = w0 + float(16 k) * step16 in float32: one multiply, one add.
 *                    w0 = float32(1 / max_depth), 0 for an infinite max_depth; step16 = float32((1 / min_depth - 1 / max_depth) /
 *                    (16 (D - 1))), both computed in double on the host with exactly these operations and rounded once.  Plane 0 is
 *                    the farthest
 *   M3 projection    source view s is a float32 3x4 matrix [A_s | b_s], row-major (for a pinhole pair A = K_s R_sr K_r^-1 and
 *                    b = K_s t_sr).  For the reference pixel (x, y), in float32 and in this order, ONE multiply and ONE add per
 *                    term (no fused multiply-add, no fast reciprocal or divide):
 *                      a_i = (A_i0 * float(x) + A_i1 * float(y)) + A_i2        q_i = a_i + w_k * b_i
 *                      u = q_0 / q_2, v = q_1 / q_2 (IEEE division)             ur = rintf(u), vr = rintf(v) (ties to even)
 *                    The view SEES (x, y, k) iff q_2 > 0, 0 <= ur <= W-1 and 0 <= vr <= H-1 all hold as float comparisons (a NaN
 *                    fails); the source pixel is then (int ur, int vr)
 *   M4 cost          n = the views that see (x, y, k), sum = the sum of popcount(census_ref(x,y) ^ census_s(ur,vr)) over them:
 *                    C = (2 sum + n) / (2 n) with C division if n >= min_views, else 64
 *   M5 paths, winner, uniqueness   stereo rules 4, 5 and 6 on this C.  There is no left-right check
 *   M6 seen          invalid if fewer than min_views views see (x, y, k*)
 *   M7 sub-pixel     stereo rule 8 on S gives k16; an invalid pixel gets -16
 *   M8 speckles      speckle_window_size > 0: hv_filter_speckles on k16 with max_speckle_size = speckle_window_size, max_diff =
 *                    16 speckle_range and new_val = -16, on the device, exactly as hv_stereo_sgm_speckle does it
 *   M9 depth         wv = w0 + float(k16) * step16, depth = 1.0f / wv; 0 where the pixel is invalid (after M8) or wv <= 0
 *  M10 outputs       index_out int16 [height,width] and depth_out float32 [height,width]; either may be NULL, not both
 * ref: [height,width] (channels 1) or [height,width,3]; sources: n_sources such images behind each other; both at `loc`, as are the
 * outputs (`loc` as in hv_stereo_sgm, staged by the library for HV_HOST).  views: float[n_sources][12], HOST memory for either loc.
 * stats (may be NULL, host memory) are the filter's; read only with a filter, and the call then waits for the stream.  Works on a
 * volume of any mode and reads nothing of it.  Scratch is the handle's stereo scratch, grown on demand: height width (3 D + 8 (1 + N)
 * + 2) bytes (S uint16, C uint8, 1 + N census images, the winners), each part rounded up to 256 bytes, plus 2 bytes per pixel when a
 * filter runs and index_out is NULL, plus the filter's own scratch.
 * HV_ERR_INVALID before anything is launched or written: a NULL image, views or params; both outputs NULL; channels not 1 or 3;
 * n_sources outside 1..4; min_views outside 1..n_sources; num_planes not a multiple of 16 in 16..256; not 0 < p1 <= p2 <= 1023;
 * uniqueness_ratio outside 0..99; paths not 4 or 8; min_depth not finite and positive (or so small that step16 is not finite);
 * max_depth <= min_depth or NaN; a matrix entry that is not finite; the image-size limits of hv_stereo_sgm; speckle_window_size
 * outside 0..2^30 or, with a filter, speckle_range outside 0..4095.  HV_ERR_CAPACITY when the scratch cannot be allocated. */
typedef struct hv_mvs_params {
    int32_t num_planes;          /* 128 */
    int32_t p1, p2;              /* 10, 120 */
    int32_t uniqueness_ratio;    /* 15 */
    int32_t min_views;           /* 1 */
    int32_t paths;               /* 8 */
    double min_depth, max_depth; /* metres; max_depth may be +inf */
    int32_t speckle_window_size; /* 0: no filter */
    int32_t speckle_range;       /* 1 */
} hv_mvs_params;
int hv_mvs_sgm(hv_volume *v, const uint8_t *ref, const uint8_t *sources, int32_t n_sources, int32_t height, int32_t width,
               int32_t channels, const float *views /* float[n_sources][12], host */, const hv_mvs_params *params,
               int16_t *index_out /* may be NULL */, float *depth_out /* may be NULL */,
               hv_speckle_stats *stats /* may be NULL, host */, int32_t loc);

/* ---- cross-view consistency check and fusion of posed depth maps ----------------------------------------
 * hv_depth_consistency: a float32 depth map and the depth maps of 1..4 posed neighbours of the same shape -> the depth map with
 * the pixels removed that the neighbours do not confirm (0 = none), the confirmed ones optionally averaged with the neighbours'
 * depths, and per pixel the number of views that agree, are occluded, are violated and see the pixel at all.  The geometric
 * consistency check of multi-view stereo, for the depth of hv_mvs_sgm (which has no left-right check of its own) and for any other
 * posed depth stream: stereo depth of consecutive keyframes, a network's or a sensor's depth before fusion.  The algorithm is
 * fixed by the rules below, restated in numpy in tests/depth_consistency_reference.py, and the library is held to that restatement
 * bit for bit.  N = n_sources.  Every arithmetic line is ONE IEEE float32 operation per written operator, in the written order (no
 * fused multiply-add, no fast reciprocal or divide); every comparison is a float comparison, so a NaN fails it.
 *   C1 valid input   z = depth[y,x] is valid iff z > 0 and z < inf.  Otherwise the output depth is 0 and all four counts are 0.
 *                    w = 1.0f / z
 *   C2 forward       rule M3 with views[s] and w gives q, ur, vr and the seen test (q_2 > 0, 0 <= ur <= W-1, 0 <= vr <= H-1).  A
 *                    view that does not see the pixel contributes nothing.  Otherwise seen += 1, the predicted source depth is
 *                    zs = z * q_2 and d = source_depths[s][vr,ur] (ur, vr from here on: the integer pixel as floats, +0.0 for 0).
 *                    If not (d > 0 and d < inf) the view contributes nothing more
 *   C3 backward      with back_views[s] = [A' | b'], in this order:
 *                      ws = 1.0f / d
 *                      a'_i = (A'_i0 * ur + A'_i1 * vr) + A'_i2                  q'_i = a'_i + ws * b'_i
 *                      xb = q'_0 / q'_2, yb = q'_1 / q'_2, zb = d * q'_2
 *                      ex = xb - float(x), ey = yb - float(y), e2 = ex * ex + ey * ey
 *                      wb = 1.0f / zb
 *   C4 agreement     view s AGREES iff q'_2 > 0 and e2 <= max_reproj_error * max_reproj_error (the product formed once in float32
 *                    on the host) and fabsf(wb - w) <= inv_depth_tol + rel_depth_tol * w.  inv_depth_tol is an absolute tolerance
 *                    in inverse metres (the unit of a plane sweep: one plane step is (1 / min_depth - 1 / max_depth) / (D - 1)),
 *                    rel_depth_tol a relative depth difference; either may be 0, not both
 *   C5 otherwise     a view that has a depth and does not agree is OCCLUDED if d < zs (the source sees something nearer), else
 *                    VIOLATED (the source sees through the point; d == zs and a NaN zs count here)
 *   C6 keep          a valid pixel is kept iff agree >= min_consistent and violated <= max_violations
 *   C7 output        depth_out: 0 if not kept; z if kept and fuse == 0; else acc / float(agree + 1) with acc = z and then
 *                    acc = acc + zb for the agreeing views in ascending s.  counts_out (agree, occluded, violated, seen) is written
 *                    for every pixel, kept or not
 * depth: float32 [height,width]; source_depths: n_sources such images behind each other; depth_out: float32 [height,width];
 * counts_out: uint8 [height,width,4], 4-byte aligned (one 32-bit store per pixel); all at `loc` (as in hv_mvs_sgm, staged by the
 * library for HV_HOST).  Either output may be NULL, not both.  views, back_views: float[n_sources][12], HOST memory for either loc:
 * 3x4 matrices [A | b] in the convention of rule M3, views[s] from a reference pixel to source s, back_views[s] from a pixel of
 * source s to the reference.  stats (may be NULL, host memory): the pixels valid on input (C1), the pixels kept (C6) and the sum of
 * the agree counts over all pixels, all exact; when given, the call waits for the stream.  A device call is otherwise queued on
 * the volume's stream and returns.  Works on a volume of any mode and reads nothing of it.  No scratch beyond the staging of host
 * arguments (with stats 8 KB more of it, for the counters).
 * HV_ERR_INVALID before anything is launched or written: a NULL image, matrix set or params; both outputs NULL; n_sources
 * outside 1..4; the image-size limits of hv_mvs_sgm; a matrix entry that is not finite; max_reproj_error, inv_depth_tol or
 * rel_depth_tol negative or not finite; both tolerances 0; min_consistent or max_violations outside 0..n_sources. */
typedef struct hv_consistency_params {
    float max_reproj_error;  /* 1.0, pixels */
    float inv_depth_tol;     /* 0.0, 1 / metres */
    float rel_depth_tol;     /* 0.01 */
    int32_t min_consistent;  /* 1 */
    int32_t max_violations;  /* 0 */
    int32_t fuse;            /* 1 */
} hv_consistency_params;
typedef struct hv_consistency_stats {
    int64_t valid_pixels, kept_pixels, agree_sum;
} hv_consistency_stats;
int hv_depth_consistency(hv_volume *v, const float *depth, const float *source_depths, int32_t n_sources, int32_t height, int32_t width,
                         const float *views /* float[n_sources][12], host */, const float *back_views /* float[n_sources][12], host */,
                         const hv_consistency_params *params, float *depth_out /* may be NULL */, uint8_t *counts_out /* may be NULL */,
                         hv_consistency_stats *stats /* may be NULL, host */, int32_t loc);

/* get_voxels(min_count, min_confidence) (voxel_block_grid.hpp:717-819): rows = sum / count.
 * Pass points == NULL to query *n only.  At most `cap` rows are written; *n is the full count. */
int hv_get_voxels(hv_volume *v, int32_t min_count, float min_confidence, float *points,
                  float *colors, int64_t cap, int64_t *n, int32_t loc);
/* get_voxels_in_bb (voxel_block_grid.hpp:822-1016); bbox = {min x,y,z, max x,y,z}. */
int hv_get_voxels_in_bb(hv_volume *v, const double *bbox, int32_t min_count, float min_confidence,
                        float *points, float *colors, int64_t cap, int64_t *n, int32_t loc);
/* get_voxels_in_camera_frustrum (voxel_block_grid.hpp:1019-1195); CameraFrustrum(fx,fy,cx,cy f32,
 * width, height, T_cw, depth_max, depth_min) (camera_frustrum.h:37-130). */
int hv_get_voxels_in_frustum(hv_volume *v, const float *intr_f32, int32_t width, int32_t height,
                             const double *T_cw, float depth_max, float depth_min, int32_t min_count,
                             float min_confidence, float *points, float *colors, int64_t cap,
                             int64_t *n, int32_t loc);
/* carve(camera_frustrum, depth_image f32 HxW, depth_threshold) (voxel_grid_carving.h:47-79); VOXEL_GRID and both
 * semantic modes. */
int hv_carve(hv_volume *v, const float *intr_f32, int32_t width, int32_t height, const double *T_cw,
             float depth_max, float depth_min, const float *depth, float depth_threshold, int32_t loc);
int hv_remove_low_count_voxels(hv_volume *v, int32_t min_count); /* voxel_block_grid.hpp:625-646 */
int hv_size(hv_volume *v, int64_t *n);           /* size()/get_total_voxel_count(): voxels with count>0 */

/* Parity/debug export: all blocks sorted by (x,y,z) key.  keys [B,3] i32; hashes [B] u64 =
 * BlockKeyHash (voxel_hashing.h:106-113); counts [B,bs^3] i32; sums [B,bs^3,6] f32 (position_sum,
 * color_sum); voxel order inside a block = lx + ly*bs + lz*bs^2 (voxel_block.h:67-70).  Host
 * pointers; any may be NULL.  *n_blocks receives B. */
int hv_dump_blocks(hv_volume *v, int32_t *keys, uint64_t *hashes, int32_t *counts, float *sums,
                   int64_t *n_blocks);
/* K2 parity probe: key arithmetic of voxel_hashing.h:69-75,139-161 for N f32 points (host arrays). */
int hv_keys_from_points(hv_volume *v, const float *points, int64_t n, int32_t *voxel_keys,
                        int32_t *block_keys, int32_t *local_keys, uint64_t *block_hashes);

/* ---- semantic block grids ------------------------------------------------------------------------
 * HV_MODE_VOXEL_SEMANTIC_GRID               == volumetric.VoxelBlockSemanticGrid (voting payload,
 *                                              VoxelSemanticData, voxel_data_semantic.h:106-202)
 * HV_MODE_VOXEL_SEMANTIC_PROBABILISTIC_GRID == volumetric.VoxelBlockSemanticProbabilisticGrid (log-probability
 *                                              payload, VoxelSemanticDataProbabilistic, voxel_data_semantic.h:249-672)
 * HV_MODE_VOXEL_SEMANTIC_GRID2               == volumetric.VoxelBlockSemanticGrid2 (VoxelSemanticData2: one confidence counter
 *                                              for the object id and one for the class id, voxel_data_semantic2.h:46-196)
 * HV_MODE_VOXEL_SEMANTIC_PROBABILISTIC_GRID2 == volumetric.VoxelBlockSemanticProbabilisticGrid2 (VoxelSemanticDataProbabilistic2:
 *                                              one log-probability map per object id and one per class id, half of every
 *                                              observation's log-probability to each, voxel_data_semantic2.h:256-787)
 * (bindings: cpp/volumetric/volumetric_grid_module.h:939-1033; class: voxel_block_semantic_grid.h:57-123).  Every entry point of
 * this section takes the four modes; the reference itself documents the two *2 payloads as the inferior variants
 * (voxel_data_semantic.h:52-100) and nothing under pyslam/dense instantiates them.
 *
 * hv_integrate_points_semantic == .integrate(points f32|f64 [N,3], colors u8|f32, class_ids i32 [N] | None,
 *   instance_ids i32 [N] | None, depths f32 [N] | None)
 *   (volumetric_grid_module.h:131-467 -> integrate_raw -> update_voxel_direct, voxel_block_grid.hpp:524-614).
 *   point_dtype: 0 float32, 1 float64 (keys follow get_voxel_key_inv<Tpos,Tpos>).  Labels, confidence
 *   counters / log-probabilities, counts and float64 position sums are bit-identical to the reference's
 *   sequential (point-index) order.  The probabilistic payload's per-voxel label map (std::map in the reference) holds
 *   6 pairs in the voxel record and chains 10-pair nodes from a per-volume pool beyond them; a pair is dropped, and
 *   counted (hv_label_overflows), only past 254 pairs in one voxel or when the node pool is exhausted. */
int hv_integrate_points_semantic(hv_volume *v, const void *points, int32_t point_dtype, int64_t n, const void *colors,
                                 int32_t color_dtype, const int32_t *class_ids, const int32_t *instance_ids,
                                 const float *depths, int32_t loc);
/* Fused L3 prep + integrate for one posed RGB-D frame with label images (the per-keyframe body of
 * VolumetricIntegratorVoxelSemanticGrid, pyslam/dense/volumetric_integrator_voxel_semantic_grid.py:402-461):
 * depth2pointcloud(depth, rgb, ..., semantic_image, object_ids_image) + world transform + float32 casts +
 * integrate(points, colors, class_ids, instance_ids, depths = camera z when use_depths).  depth f32 metres HxW, rgb
 * u8 HxWx3, label images i32 HxW or NULL. */
int hv_integrate_rgbd_semantic(hv_volume *v, const float *depth, const uint8_t *rgb, const int32_t *class_ids_image,
                               const int32_t *object_ids_image, int32_t height, int32_t width, const double *intr,
                               const double *T_cw, double min_depth, double max_depth, int32_t use_depths, int32_t loc);
/* get_voxels(min_count, min_confidence) for semantic voxels: rows with count >= min_count and
 * confidence >= min_confidence; points f64 [M,3], colors f32 [M,3], class_ids/object_ids i32 [M],
 * confidences f32 [M] (host).  points == NULL: size query. */
int hv_get_voxels_semantic(hv_volume *v, int32_t min_count, float min_confidence, double *points, float *colors,
                           int32_t *class_ids, int32_t *object_ids, float *confidences, int64_t cap, int64_t *n);
/* get_voxels_in_bb / get_voxels_in_camera_frustrum for semantic voxels (voxel_block_grid.hpp:822-1016, 1019-1195; the
 * label / confidence outputs are what IncludeSemantics=true adds).  Same output conventions as hv_get_voxels_semantic. */
int hv_get_voxels_semantic_in_bb(hv_volume *v, const double *bbox, int32_t min_count, float min_confidence, double *points,
                                 float *colors, int32_t *class_ids, int32_t *object_ids, float *confidences, int64_t cap,
                                 int64_t *n);
int hv_get_voxels_semantic_in_frustum(hv_volume *v, const float *intr_f32, int32_t width, int32_t height, const double *T_cw,
                                      float depth_max, float depth_min, int32_t min_count, float min_confidence, double *points,
                                      float *colors, int32_t *class_ids, int32_t *object_ids, float *confidences, int64_t cap,
                                      int64_t *n);
/* set_depth_threshold() (voxel_block_semantic_grid.hpp:24-30): voting: observations with depth >= threshold do
 * not vote (voxel_data_semantic.h:168-198); probabilistic: beyond it the evidence decays (:337-352).  Defaults
 * 10 m / 5 m.  The reference keeps these as process-wide statics; here they are per volume. */
int hv_set_depth_threshold(hv_volume *v, float depth_threshold);
/* set_depth_decay_rate() (voxel_block_semantic_grid.hpp:32-37), probabilistic payload; default 0.07 1/m. */
int hv_set_depth_decay_rate(hv_volume *v, float depth_decay_rate);
/* Label observations the probabilistic payload could not store (a voxel's map past 254 pairs, or the overflow-node pool exhausted):
 * 0 in every test and bench run; never silent. */
int hv_label_overflows(hv_volume *v, int64_t *n);
/* Overflow nodes of the probabilistic label maps handed out so far (of the pool's 4 per block; HV_PROB_NODE_CAP overrides).  A voxel
 * that is reset (carve, remove_low_*, remove_segment) keeps its chain and grows its next map into it, so the count is bounded by the
 * longest map every voxel ever held - it does not grow with the number of carve / re-observe cycles. */
int hv_prob_nodes_used(hv_volume *v, int64_t *n);
/* assign_object_ids_to_instance_ids(camera_frustrum, class_ids_image i32 HxW, semantic_instances_image i32 HxW,
 * depth_image f32 HxW | NULL, depth_threshold, do_carving, min_vote_ratio, min_votes)
 * (voxel_semantic_data_association.h:70-373).  Returns the instance -> object map sorted by instance id in
 * map_inst / map_obj (host, at most cap entries; *n_map = full size).  Mutates the volume (carving, object ids of
 * voxels that had none) exactly once per call: there is no size-query mode, pass cap >= the number of distinct
 * instance ids in the image.  New object ids come from a process-wide counter (hv_peek/set_next_object_id). */
int hv_assign_object_ids_to_instance_ids(hv_volume *v, const float *intr_f32, int32_t width, int32_t height, const double *T_cw,
                                         float depth_max, float depth_min, const int32_t *class_ids_image,
                                         const int32_t *instance_ids_image, const float *depth_image, float depth_threshold,
                                         int32_t do_carving, float min_vote_ratio, int32_t min_votes, int32_t *map_inst,
                                         int32_t *map_obj, int64_t cap, int64_t *n_map, int32_t loc);
/* The same association in stages, none of which waits for the GPU unless it hands data to the host (pySLAM's per-keyframe flow -
 * assign -> remap -> integrate, volumetric_integrator_voxel_semantic_grid.py:326-461 - then runs without a host round trip):
 *   hv_assoc_vote      per-voxel votes + the image's instance ids -> (instance << 32 | object, votes) pairs in device memory
 *   hv_assoc_decide    the reference's winner / min_votes / min_vote_ratio rules on the pairs (voxel_semantic_data_association.h:
 *                      268-361), new object ids from the process-wide counter (kept in device memory), deferred set_object_id
 *   hv_assoc_map_fetch the instance -> object map, sorted by instance id (synchronises; reports capacity overflows of the stages)
 *   hv_remap_instance_ids_last  remap_instance_ids (image_utils.h:69-163) with that map, read where it lies
 * Multi-GPU (block ownership, hv_set_owner): every GPU votes with its own voxels, hv_assoc_pairs_fetch -> all-gather of the pair
 * lists -> hv_assoc_pairs_set(concatenation) on every GPU -> hv_assoc_decide: identical maps and object ids everywhere. */
int hv_assoc_vote(hv_volume *v, const float *intr_f32, int32_t width, int32_t height, const double *T_cw, float depth_max,
                  float depth_min, const int32_t *class_ids_image, const int32_t *instance_ids_image, const float *depth_image,
                  float depth_threshold, int32_t do_carving, int32_t loc);
int hv_assoc_pairs_fetch(hv_volume *v, uint64_t *pair_keys, int32_t *pair_counts, int64_t cap, int64_t *n_pairs);
int hv_assoc_pairs_set(hv_volume *v, const uint64_t *pair_keys, const int32_t *pair_counts, int64_t n_pairs);
/* Multi-GPU exchange with the pair lists staying in device memory (no host round trip per keyframe): d_msg / d_msgs are DEVICE
 * buffers of the caller (torch tensors), int64 words: one GPU's message = [n, keys[cap], votes[cap]] (1 + 2 cap words, cap <= 4096);
 * hv_assoc_pairs_import takes `world` messages back to back - the output of an all-gather - and adds equal pairs up.  Both are
 * queued on the volume's stream and return at once. */
int hv_assoc_pairs_export(hv_volume *v, int64_t *d_msg, int64_t cap);
int hv_assoc_pairs_import(hv_volume *v, const int64_t *d_msgs, int32_t world, int64_t cap);
int hv_assoc_decide(hv_volume *v, float min_vote_ratio, int32_t min_votes);
int hv_assoc_map_fetch(hv_volume *v, int32_t *map_inst, int32_t *map_obj, int64_t cap, int64_t *n_map);
int hv_remap_instance_ids_last(hv_volume *v, const int32_t *instance_ids, int32_t height, int32_t width, int32_t *out, int32_t loc);
/* One semantic keyframe in one call, on DEVICE images, queued on the volume's stream (nothing waits): the per-keyframe body of
 * VolumetricIntegratorVoxelSemanticGrid (pyslam/dense/volumetric_integrator_voxel_semantic_grid.py:326-461) - filter_shadow_points
 * (:334, when filter_shadow_points != 0) -> assign_object_ids_to_instance_ids + remap_instance_ids (:340-372, when use_instance_ids
 * != 0 and instance_ids_image != NULL; a NULL class image gives the reference's empty map: every object id -1) or carve (:373-380,
 * when do_carving != 0) -> depth2pointcloud + world transform + integrate (:402-461).  The stages are the entry points above, in that
 * order; the filtered depth and the object-id image live in scratch of the volume.  frustum_*: the CameraFrustrum of the
 * association / carve (float32 intrinsics, camera_frustrum.h:37-130); intr: the float64 intrinsics of depth2pointcloud. */
int hv_semantic_fuse_keyframe(hv_volume *v, const float *depth, const uint8_t *rgb, const int32_t *class_ids_image,
                              const int32_t *instance_ids_image, int32_t height, int32_t width, const float *frustum_intr_f32,
                              float frustum_depth_max, float frustum_depth_min, const double *intr, const double *T_cw,
                              int32_t filter_shadow_points, int32_t use_instance_ids, float assoc_depth_threshold, int32_t do_carving,
                              float min_vote_ratio, int32_t min_votes, double min_depth, double max_depth, int32_t use_depths);
int32_t hv_peek_next_object_id(void); /* VoxelSemanticSharedData::next_object_id, voxel_semantic_shared_data.h:26-34 */
void hv_set_next_object_id(int32_t id);
/* volumetric.remap_instance_ids(instance_ids i32 HxW, map) (binding image_utils_module.h:49-94 over image_utils.h:69-163): ids
 * absent from the map become -1; an EMPTY map returns the image unchanged (the binding's early return, :52-58). */
int hv_remap_instance_ids(hv_volume *v, const int32_t *instance_ids, int32_t height, int32_t width, const int32_t *map_inst,
                          const int32_t *map_obj, int64_t n_map, int32_t *out, int32_t loc);
/* get_object_segments(min_count, min_confidence) (voxel_block_semantic_grid.hpp:217-267): voxels with
 * count > min_count (strict, as the reference), confidence >= min_confidence and object id >= 0, grouped by object
 * id.  _compute runs the query and caches the result on the host; _fetch copies it out: points f64 [R,3] and
 * colors f32 [R,3] grouped by ascending object id, row_object_ids i32 [R]; per object: object_ids i32 [O,3] =
 * {object_id, class_id, n_points}, confidences f32 [O,2] = {min, max}, obbs f64 [O,10] = {center xyz, quaternion
 * wxyz, size xyz} = OrientedBoundingBox3D::compute_from_points(PCA) (bounding_boxes_3d.cpp:373-553).  Any pointer
 * may be NULL. */
int hv_object_segments_compute(hv_volume *v, int32_t min_count, float min_confidence, int64_t *n_rows, int64_t *n_objects);
int hv_object_segments_fetch(hv_volume *v, double *points, float *colors, int32_t *row_object_ids, int32_t *object_ids,
                             float *confidences, double *obbs);
int hv_compute_obb_pca(const double *points, int64_t n, double *obb);
/* merge_segments / remove_segment / remove_low_confidence_segments (voxel_block_semantic_grid.hpp:119-196) and
 * remove_low_confidence_voxels (voxel_block_grid.hpp:650-676; a no-op on non-semantic volumes). */
int hv_merge_segments(hv_volume *v, int32_t instance_id1, int32_t instance_id2);
int hv_remove_segment(hv_volume *v, int32_t object_id);
int hv_remove_low_confidence_segments(hv_volume *v, int32_t min_confidence);
int hv_remove_low_confidence_voxels(hv_volume *v, float min_confidence);
/* Parity/debug export, key-sorted: keys [B,3]; ints [B,bs^3,4] {count, object_id, class_id, confidence_counter};
 * pos_sums [B,bs^3,3] f64; col_sums [B,bs^3,3] f32.  The second form adds conf [B,bs^3] f32 and, for the
 * probabilistic payload, label_counts [B,bs^3] (the size of each voxel's label map), labels [B,bs^3,max_labels,2]
 * {object, class} and log_probs [B,bs^3,max_labels]: each map's first max_labels pairs in insertion order. */
int hv_dump_blocks_semantic(hv_volume *v, int32_t *keys, int32_t *ints, double *pos_sums, float *col_sums,
                            int64_t *n_blocks);
int hv_dump_blocks_semantic2(hv_volume *v, int32_t *keys, int32_t *ints, float *conf, double *pos_sums, float *col_sums,
                             int32_t *label_counts, int32_t *labels, float *log_probs, int32_t max_labels,
                             int64_t *n_blocks);
/* The marginal confidences of the two "*2" payloads, [B,bs^3] f32 each in the dumps' order: get_object_confidence() /
 * get_class_confidence() (voxel_data_semantic2.h:60-76, 528-560); -1 everywhere for the other two payloads, which have none.
 * For HV_MODE_VOXEL_SEMANTIC_PROBABILISTIC_GRID2 the labels of hv_dump_blocks_semantic2 are the entries of the voxel's two maps,
 * {id, which map (0 object, 1 class)}, in insertion order. */
int hv_dump_marginals_semantic(hv_volume *v, float *object_confidences, float *class_confidences, int64_t *n_blocks);

/* ---- TSDF mode ---------------------------------------------------------------------------------
 * hv_tsdf_integrate == RGBDImage.create_from_color_and_depth(color, depth, depth_scale,
 *   depth_trunc, convert_rgb_to_intensity=False) + volume.integrate(rgbd, intrinsic, T_cw)
 *   (volumetric_integrator_tsdf.py:215-223). */
int hv_tsdf_integrate(hv_volume *v, const void *depth, int32_t depth_dtype, const uint8_t *rgb,
                      int32_t height, int32_t width, const double *intr, const double *T_cw,
                      double depth_scale, double depth_trunc, int32_t loc);

/* Batched replay of F posed frames resident in HBM (rebuild(), volumetric_integrator_base.py:
 * 1242-1318): identical results to F successive hv_tsdf_integrate calls.  depth: F*H*W, rgb:
 * F*H*W*3, T_cw: F*16 (host array). */
int hv_tsdf_integrate_batch(hv_volume *v, const void *depth, int32_t depth_dtype, const uint8_t *rgb,
                            int32_t n_frames, int32_t height, int32_t width, const double *intr,
                            const double *T_cw, double depth_scale, double depth_trunc, int32_t loc);

/* The same for HOST-resident frames given one pointer per frame - what pySLAM's worker holds after draining its queue of
 * INTEGRATE tasks (volumetric_integrator_base.py:101-137: every keyframe carries its own pageable numpy arrays).  The frames
 * are copied to page-locked slots by worker threads and cross PCIe on a copy stream while the previous batch is swept; the
 * caller's memory has been read completely when the call returns.  depth_frames[f]: H*W of depth_dtype, rgb_frames[f]:
 * H*W*3 uint8, T_cw: F*16. */
int hv_tsdf_integrate_frames(hv_volume *v, const void *const *depth_frames, int32_t depth_dtype, const uint8_t *const *rgb_frames,
                             int32_t n_frames, int32_t height, int32_t width, const double *intr, const double *T_cw,
                             double depth_scale, double depth_trunc);

/* De-integration and re-integration (BundleFusion's map correction after a loop closure: take a frame out at the pose it was
 * fused with, put it back at the corrected one; Open3D's legacy ScalableTSDFVolume has none).  This project's own contract, not
 * Open3D-pinned:
 *   prep       depth conversion (dtype, depth_scale, depth_trunc, NaN / inf / negative), the volume's rectify maps and colour order
 *              exactly as in hv_tsdf_integrate*: a frame handed here is sampled exactly as integrate sampled it.
 *   touch set  the units integrate's touch pass would claim for the frame and pose (the volume's stride, +/- sdf_trunc; owned units
 *              only when owner-sharded).  They are only LOOKED UP: nothing is claimed or grown; absent units are skipped.
 *   predicate  within the touch set a voxel is updated under integrate's predicate (projection, valid depth, sdf >= -trunc) with
 *              integrate's per-frame sample t (float32) and colour c.
 *   update     a call of F frames acts as consecutive chunks of at most HV_TSDF_DEINTEGRATE_MAX_FRAMES frames, in call order.  Per
 *              voxel and chunk, n = the chunk's frames that sample it, w0 / tsdf0 / sums its state before the chunk:
 *                w0 < n   unchanged in all five planes, counted once in voxels_underflow;
 *                w0 == n  the state of a freshly claimed voxel: weight 0, colour sums 0, tsdf 0 (what hv_tsdf_dump shows for a voxel
 *                         no frame has touched);
 *                else     w = w0 - n, each colour sum becomes min(max(sum - bytes, 0), 255 * w) with `bytes` the frames' colour bytes
 *                         (exact integers), and
 *                         tsdf = (float)(((double)tsdf0 * w0 - sum_f (double)t_f) / (double)(w0 - n)), the sum in frame order, in
 *                         double, without contraction (one double and one float rounding).
 *              Weights and colour sums come back bit for bit; the tsdf mean carries the ~half-ulp rounding of every stored mean,
 *              scaled by about w0 / w by the removal (63 of 64 observations removed: ~64 x 3e-8).  The clamp of the colour sums
 *              never acts when the removed frames were fused into the voxel (the bytes that remain sum to at most 255 * w); it
 *              keeps sum / w in [0, 255] when a frame that was never fused into the voxel is removed while w0 > n (a second
 *              removal, a wrong pose, a merged map).  The tsdf is NOT clamped: after such a removal it can leave [-1, 1].
 *   stamping   every unit of the touch set that the volume holds is stamped with a new frame counter value (the incremental
 *              extractions recompute it, hv_tsdf_dirty_keys reports it).
 *   reintegrate  hv_tsdf_deintegrate_batch at T_cw_old, then hv_tsdf_integrate_batch at T_cw_new (both F*16), over frames
 *              uploaded and rectified once: bitwise the result of the two calls, the integrate side's pool growth included.
 *   stats      may be NULL: the call is then asynchronous on the volume's stream, like integrate.  Otherwise the call waits once
 *              and fills them (of the de-integration side).
 *   errors     HV_ERR_MODE for a non-TSDF or tile-sharded volume (hv_tsdf_set_tile: a rank holds partial sums of a voxel that halo
 *              merges move between ranks); owner-sharded volumes are supported (each rank removes from its own units).
 *              HV_ERR_INVALID for bad sizes or arguments, as integrate. */
#define HV_TSDF_DEINTEGRATE_MAX_FRAMES 64
typedef struct hv_deintegrate_stats {
    int64_t units_listed;     /* sum over frames of the units the frame's touch set names (owned units only when owner-sharded) */
    int64_t units_missing;    /* ... of those, absent from the volume: skipped */
    int64_t voxels_removed;   /* voxel observations removed */
    int64_t voxels_underflow; /* voxels left unchanged because they hold fewer observations than were to be removed */
} hv_deintegrate_stats;
int hv_tsdf_deintegrate(hv_volume *v, const void *depth, int32_t depth_dtype, const uint8_t *rgb, int32_t height, int32_t width,
                        const double *intr, const double *T_cw, double depth_scale, double depth_trunc, int32_t loc,
                        hv_deintegrate_stats *stats);
int hv_tsdf_deintegrate_batch(hv_volume *v, const void *depth, int32_t depth_dtype, const uint8_t *rgb, int32_t n_frames,
                              int32_t height, int32_t width, const double *intr, const double *T_cw, double depth_scale,
                              double depth_trunc, int32_t loc, hv_deintegrate_stats *stats);
int hv_tsdf_reintegrate_batch(hv_volume *v, const void *depth, int32_t depth_dtype, const uint8_t *rgb, int32_t n_frames,
                              int32_t height, int32_t width, const double *intr, const double *T_cw_old, const double *T_cw_new,
                              double depth_scale, double depth_trunc, int32_t loc, hv_deintegrate_stats *stats);

/* Undistort / rectify on the device.  The reference remaps every keyframe on the host before it is fused
 * (estimate_depth_if_needed_and_rectify, volumetric_integrator_base.py:1017-1043: cv2.remap colour INTER_LINEAR, depth INTER_NEAREST,
 * maps from cv2.initUndistortRectifyMap, :758-786).  With maps set (float32 [H,W], at `loc`; copied), every frame handed to
 * hv_tsdf_integrate / _batch / _frames goes through them first - one launch per batch, beside the batch's touch + pack launch, the
 * depth in its own storage type (float32 or uint16: 5 bytes per pixel for a TUM-style keyframe end to end) - and the caller passes
 * the RECTIFIED intrinsics.  map_x == NULL clears them.  OpenCV's remap semantics restated (hv_remap): unpinned.  The rules are
 * hv_remap's, coordinate for coordinate: a NaN or +-inf map entry, or one whose rounded value does not fit int32, is outside the
 * image - depth 0 (nothing is fused there) and colour 0.  Frames of another size than the maps' are refused (HV_ERR_INVALID);
 * HV_ERR_MODE for a volume that is not a TSDF volume. */
int hv_tsdf_set_rectify_maps(hv_volume *v, const float *map_x, const float *map_y, int32_t height, int32_t width, int32_t loc);

/* Channel order of the colour frames handed to hv_tsdf_integrate*: 0 = R, G, B (Open3D's RGBDImage, the default), 1 = B, G, R -
 * pySLAM's keyframe.img as OpenCV loads it; the reference converts every keyframe on the host with cv2.cvtColor
 * (volumetric_integrator_base.py:1054), here the pack kernel swaps the bytes of the record it writes anyway. */
int hv_tsdf_set_color_order(hv_volume *v, int32_t bgr);

/* Page-lock caller memory for the H2D DMA of hv_tsdf_integrate_frames / hv_integrate_*(HV_HOST): pySLAM's front hands keyframes
 * over in a shared-memory ring (volumetric_integrator_base.py:401-410 carries them pickled through a Manager queue); once the
 * ring is registered, frames that lie inside it are DMA'd in place - no staging copy - and the call returns when the DMA has
 * read them.  This holds for EVERY entry point that takes HV_HOST arrays: a page-locked source (registered here, or any other
 * pinned allocation) is read by the DMA engine when the stream gets to the copy, so those calls wait for their copies before they
 * return (hv_core.hip: hv_h2d); the kernels behind the copies stay asynchronous.  Process-wide (any volume of the process sees the
 * range); unregister before the memory is unmapped. */
int hv_host_register(void *ptr, int64_t bytes);
int hv_host_unregister(void *ptr);

/* Multi-GPU image-tile sharding (north-star form): this volume fuses only voxels whose
 * projection lands in pixel tile [u0,u1) x [v0,v1); units that cannot project into the tile are
 * allocated (so all GPUs agree on the unit set) but not swept.  All zeros = whole image (default). */
int hv_tsdf_set_tile(hv_volume *v, int32_t u0, int32_t v0, int32_t u1, int32_t v1);

/* The same for the VOXEL_GRID mode: owner(block) = hash(block key) mod world_size; a point whose block another GPU owns is
 * skipped (not counted as dropped).  The GPUs' voxel sets are disjoint and their union is the single-GPU grid bit for bit
 * (cpp/volumetric/voxel_block_grid.hpp:371-456 already treats blocks as independent).  hv_block_owner evaluates the ownership
 * function on the host for block keys [n,3] (-1 for keys outside the supported range). */
int hv_set_owner(hv_volume *v, int32_t rank, int32_t world_size);
int hv_block_owner(const int32_t *block_keys, int64_t n, int32_t world_size, int32_t *owner);

/* Multi-GPU unit-ownership sharding (SURVEY §8e "zero reduce" form): every GPU sees every frame but
 * claims, stores and fuses only the units with owner(unit index) == rank (a fixed hash of the
 * index modulo world_size).  Per-frame work and HBM footprint divide by world_size, results are
 * bit-identical to a single GPU, and no collective is needed while fusing.  (1 GPU: rank 0 of 1.) */
int hv_tsdf_set_owner(hv_volume *v, int32_t rank, int32_t world_size);

/* extract_triangle_mesh() (volumetric_integrator_tsdf.py:239,260).  vertices/vertex_colors f64
 * [V,3] (colours in [0,1]); triangles i32 [T,3].  NULL arrays = size query.  The destination arrays may be host memory
 * (pySLAM's viewer / PLY writer) or device memory of the volume's GPU (a GPU consumer: the 272 MB device-to-host copy of a
 * 32 k-unit mesh is the whole wall time of an output tick); the same holds for hv_tsdf_extract_points / _point_normals. */
int hv_tsdf_extract_mesh(hv_volume *v, double *vertices, double *vertex_colors, int64_t cap_vertices,
                         int32_t *triangles, int64_t cap_triangles, int64_t *n_vertices,
                         int64_t *n_triangles);
/* The same mesh with float32 vertices / vertex_colors: the float64 values of hv_tsdf_extract_mesh rounded once on the device
 * (numpy's astype(float32) of its arrays, bit for bit).  pySLAM's viewer and dense-map consumers take float32
 * (Parameters.kDenseMappingDtypeVertices / kDenseMappingDtypeColors, pyslam/config_parameters.py:290-291; the viewer casts,
 * pyslam/viz/viewer3D.py:1335-1342): a third fewer bytes across PCIe per output tick and half the vertex bytes written.
 * Opt-in: Open3D's arrays (and the reference's VolumetricIntegrationMesh, volumetric_integrator_base.py:209-214) are float64. */
int hv_tsdf_extract_mesh_f32(hv_volume *v, float *vertices, float *vertex_colors, int64_t cap_vertices,
                             int32_t *triangles, int64_t cap_triangles, int64_t *n_vertices,
                             int64_t *n_triangles);
/* A simplified mesh by vertex clustering (Open3D users reach for simplify_vertex_clustering on the host; here the full mesh never
 * leaves the device, nor is it written).  This project's own contract.  Let FULL be the mesh hv_tsdf_extract_mesh returns for the
 * volume as it is now: V vertices and T triangles, float64, in that call's order.
 *   Owner and cell.  Every full vertex v lies on the edge from its OWNER voxel g(v) to g(v) + e_axis; g is the global integer voxel
 *     index, unit key * 16 + (x, y, z), its centre at (g + 0.5) * voxel_length.  With cell = k voxels, k in {2, 4, 8, 16}:
 *     cell(v) = floor_div(g(v), k) per component (towards -inf: unit keys are negative too).  No floating-point value takes part.
 *     A CLUSTER is the set of full vertices with the same cell; it lies inside one unit.
 *   Vertices.  One per non-empty cluster (also one no kept triangle references).  Clusters of the unit that comes first in FULL come
 *     first (FULL's vertices are grouped by unit); inside a unit they ascend by (cx, cy, cz), x-major.  Position and colour are each
 *     (the members' float64 values, FULL's bit for bit, added one by one in ascending full vertex index starting from the first
 *     member) / (double)count, per component; _f32 rounds that double once, as hv_tsdf_extract_mesh_f32 does.
 *   Triangles.  A full triangle (a, b, c) maps to the cluster numbers (A, B, C); it is DROPPED when two of them are equal, otherwise
 *     rotated so that its smallest number comes first (orientation kept).  The output is the set of DISTINCT rotated triples, sorted
 *     lexicographically; (A, B, C) and (A, C, B) are different triangles and both stay, as in Open3D's clustering.
 *   vertex_cluster i32 [V], optional (NULL): for every full vertex the number of its simplified vertex - to carry per-vertex data
 *     (hv_lookup_points labels, ...) from one mesh to the other.
 *   Normals are not part of the result: sample the map at the simplified vertices (hv_tsdf_sample_points with gradients).
 * Reads only: no growth, stamp or claim; the cached full mesh / point cloud stand (results and scratch are separate), and two calls
 * give bitwise equal outputs.  The result depends on pool order only through FULL's unit order.  An empty map, or one without a
 * surface, gives 0 / 0 and is not an error.
 * Count-then-fill, as hv_tsdf_extract_mesh: *n_vertices, *n_triangles and *n_full_vertices (= V) are always written; with vertices
 * or vertex_colors NULL the call is a size query.  triangles may be NULL on its own (a result with vertices and no triangle, whose
 * zero-row array has no address): the other arrays are still filled.  The result is kept under (contents, cell, type), so the pair computes
 * once.  At most cap_* rows of each array are written; destinations may be host or device memory.
 * Errors: HV_ERR_MODE as hv_tsdf_extract_mesh; HV_ERR_INVALID for a cell outside {2, 4, 8, 16}, a unit resolution other than 16,
 * or a null count pointer. */
int hv_tsdf_extract_mesh_clustered(hv_volume *v, int32_t cell, double *vertices, double *vertex_colors, int64_t cap_vertices,
                                   int32_t *triangles, int64_t cap_triangles, int32_t *vertex_cluster, int64_t cap_full_vertices,
                                   int64_t *n_vertices, int64_t *n_triangles, int64_t *n_full_vertices);
int hv_tsdf_extract_mesh_clustered_f32(hv_volume *v, int32_t cell, float *vertices, float *vertex_colors, int64_t cap_vertices,
                                       int32_t *triangles, int64_t cap_triangles, int32_t *vertex_cluster, int64_t cap_full_vertices,
                                       int64_t *n_vertices, int64_t *n_triangles, int64_t *n_full_vertices);
/* extract_point_cloud() (volumetric_integrator_tsdf.py:246,267): points/colors f64 [N,3]. */
int hv_tsdf_extract_points(hv_volume *v, double *points, double *colors, int64_t cap, int64_t *n);
/* ... with float32 points / colors (the float64 rows rounded once, as hv_tsdf_extract_mesh_f32). */
int hv_tsdf_extract_points_f32(hv_volume *v, float *points, float *colors, int64_t cap, int64_t *n);
/* The normals Open3D's extract_point_cloud() attaches to those points (ScalableTSDFVolume::GetNormalAt: central differences of
 * the trilinearly interpolated tsdf at +/- 0.99 voxel, normalised); o3d.io.write_point_cloud stores them in dense_map.ply
 * (volumetric_integrator_tsdf.py:246-247).  normals f64 [N,3] in the order of hv_tsdf_extract_points; NULL to query *n. */
int hv_tsdf_extract_point_normals(hv_volume *v, double *normals, int64_t cap, int64_t *n);

/* Ray casting (KinectFusion's second TSDF operation; Open3D's tensor VoxelBlockGrid.ray_cast has one, the legacy
 * ScalableTSDFVolume does not): what depth, world vertex, normal and colour the fused map predicts at pixel (u, v) of a pinhole
 * camera intr = {fx, fy, cx, cy} at pose T_cw (row-major 4x4 double, as integrate).  This project's own contract, not Open3D-pinned:
 *   ray       d_c = ((u - cx) / fx, (v - cy) / fy, 1) for integer u, v, so the ray parameter z IS camera z; in the world
 *             o = T_wc * 0, d = R_wc * d_c (T_wc = inverse(T_cw)).  Everything below runs in float32 except the normal.
 *   observed  a voxel with weight > weight_threshold.  Colour = sum / weight / 255.
 *   nearest   the voxel floor(p / voxel_length), unit floor(voxel / 16); a missing unit is empty.
 *   trilinear the 8 voxels around p - 0.5 voxel_length (hv_tsdf_at's cell), across units; valid only if all 8 are observed.
 *   march     z from depth_min while z < depth_max, at most ceil(4 (depth_max - depth_min) / voxel_length) steps:
 *               unit missing    z := max(exit of the unit's box, z) + HV_RAYCAST_UNIT_EPS * voxel_length; forget the previous sample
 *               not observed    z += voxel_length; forget the previous sample
 *               else            nearest f; previous observed sample f_prev > 0 and f <= 0: hit, bracket [z_prev, z] (front faces only)
 *                               otherwise z += max(voxel_length, HV_RAYCAST_STEP_FRAC * f * sdf_trunc) for f > 0, voxel_length else
 *   refine    HV_RAYCAST_REFINE_ITERS steps of regula falsi (Illinois) on the trilinear field.  The bracket [z_prev, z] of the
 *             nearest field may miss the trilinear root by up to about a voxel, so each end first moves one voxel outwards
 *             (max(z_prev - voxel_length, depth_min), min(z + voxel_length, depth_max)) where the trilinear sample there is valid and
 *             of its sign (> 0 before, <= 0 behind); otherwise it stays, with its trilinear value if valid and of its sign, else
 *             its nearest value.  A step whose trilinear sample is invalid ends the refinement.  z* = the last estimate.
 *   hit       depth = z* * depth_scale; vertex = o + z* d (world); normal = GetNormalAt there (hv_tsdf_extract_point_normals' central
 *             differences of the trilinear tsdf at +/- 0.99 voxel, double, normalised; world frame); colour in [0, 1] = trilinear
 *             mean colour if valid, else the nearest voxel's (0 if it has no weight); mask = 1.
 *   miss      every output 0, mask = 0.
 * Outputs: depth [H,W] f32, vertex / normal / color [H,W,3] f32, mask [H,W] u8; any may be NULL (not computed).  loc = HV_DEVICE:
 * device pointers, written asynchronously on the volume's stream; HV_HOST: staged by the library and copied back before returning.
 * Reads only: no growth, reset or stamp; the extraction caches stay valid.  HV_ERR_MODE for a non-TSDF or owner-sharded volume
 * (hv_tsdf_set_owner with world_size > 1: ray casting needs the whole volume), HV_ERR_INVALID for bad sizes or depth range. */
#define HV_RAYCAST_STEP_FRAC 0.8f
#define HV_RAYCAST_REFINE_ITERS 4
#define HV_RAYCAST_UNIT_EPS 0.01f
int hv_tsdf_ray_cast(hv_volume *v, int32_t height, int32_t width, const double *intr, const double *T_cw, double depth_min,
                     double depth_max, double weight_threshold, double depth_scale, float *depth, float *vertex, float *normal,
                     float *color, uint8_t *mask, int32_t loc);

/* Frame-to-model tracking (KinectFusion's other half; names and defaults follow Open3D's tensor odometry, point-to-plane): where
 * was a depth frame taken, aligned against the fused map rendered at an initial pose, and how well does it fit.  This project's
 * own contract, not Open3D-pinned:
 *   source    depth [H,W] (depth_dtype, at loc) -> float32 metres d = depth / (float)depth_scale (both dtypes, as integrate).
 *             Level 0 valid: finite and depth_min < d <= depth_max (compared in double).  Level l+1 [H >> (l+1), W >> (l+1)]:
 *             the valid ones of the 2x2 children (2u, 2v), (2u+1, 2v), (2u, 2v+1), (2u+1, 2v+1), summed in that order in float32
 *             and divided by their count; valid iff >= 1 child is valid and max - min of the valid children <= depth_outlier_trunc.
 *             Invalid is stored as 0.
 *   levels    l = 0 .. n_levels - 1 (0 = full resolution), run from n_levels - 1 down to 0; intrinsics fx / 2^l, fy / 2^l,
 *             (cx + 0.5) / 2^l - 0.5, (cy + 0.5) / 2^l - 0.5.
 *   model     per level one hv_tsdf_ray_cast at T_cw_init with that level's intrinsics (depth_min, depth_max, weight_threshold,
 *             depth_scale 1; depth, normal and mask only).  Everything below is double, in the ANCHOR frame = the T_cw_init
 *             camera: model vertex q(u, v) = z* ((u - cx) / fx, (v - cy) / fy, 1) from the cast depth z*, normal
 *             n = R_cw_init n_world (the world vertex is not used: the precision does not depend on where the world origin is).
 *   state     A = T_cw_init T_wc (current camera -> anchor), identity at the start, kept on the device.
 *   linearise every valid source pixel (u, v): p_c = d ((u - cx) / fx, (v - cy) / fy, 1), p = R_A p_c + t_A,
 *             (u', v') = (floor(fx p_x / p_z + cx + 0.5), floor(fy p_y / p_z + cy + 0.5)); an INLIER iff p_z > 0, (u', v') lies
 *             in the level's image, the model mask is set there and |p - q| <= depth_outlier_trunc.  For an inlier
 *             r = n . (p - q), J = [p x n, n] (omega, t), Huber weight w = 1 if |r| <= depth_huber_delta else delta / |r|;
 *             H = sum w J^T J, g = sum w J^T r, e = sum r^2 (unweighted), counts of inliers and of valid source pixels.
 *   solve     H xi = -g by Cholesky; DEGENERATE if fewer than HV_TRACK_MIN_INLIERS inliers or a pivot <= HV_TRACK_PIVOT_REL
 *             trace(H): A stays, the level ends and is marked degenerate.  Otherwise A := exp(xi) A with
 *             exp(xi) = [Rodrigues(omega), t] (the translation as it is), and the level ends when |omega| + |t| <
 *             HV_TRACK_CONVERGED or after its iterations[l] linearisations.
 *   result    T_cw = inverse(A) T_cw_init; of the LAST level-0 linearisation: fitness = inliers / valid (0 if none), inlier_rmse
 *             = sqrt(e / inliers) (0 if none), information = H (6x6, row-major, anchor frame, order (omega, t)); iterations =
 *             linearisations run per level; degenerate = bit l set when level l ended on a degenerate step; success = level 0 did
 *             not and had >= HV_TRACK_MIN_INLIERS inliers.  An empty map is not an error: success = 0, T_cw = T_cw_init.
 * trace (may be NULL): one row of HV_TRACK_TRACE_STRIDE doubles per linearisation run, in order: {level, iteration, status
 * (0 stepped, 1 converged, 2 degenerate), inliers, valid, e, A [16] (the state it linearised at), H [21] (upper triangle, row by
 * row), g [6], xi [6]}; *trace_rows = rows written (at most trace_cap).
 * All steps are queued at once on the volume's stream; a step of a finished level returns at once (a device flag), and the host
 * waits once, for the result.  No float atomics: the reduction order is fixed, results are bitwise reproducible.  Reads only (as
 * hv_tsdf_ray_cast).  HV_ERR_MODE for a non-TSDF or owner-sharded volume, HV_ERR_INVALID for bad sizes, depth range, intrinsics,
 * thresholds or iterations (1 <= n_levels <= HV_TRACK_MAX_LEVELS, every entry >= 0, level 0's >= 1, H >> (n_levels - 1) >= 1). */
#define HV_TRACK_MAX_LEVELS 8
#define HV_TRACK_MIN_INLIERS 6
#define HV_TRACK_PIVOT_REL 1e-10
#define HV_TRACK_CONVERGED 1e-6
#define HV_TRACK_TRACE_STRIDE 56
typedef struct hv_track_params {
    double depth_scale, depth_min, depth_max, weight_threshold;
    double depth_outlier_trunc; /* Open3D default 0.07 m */
    double depth_huber_delta;   /* Open3D default 0.05 m */
    int32_t n_levels;
    int32_t iterations[HV_TRACK_MAX_LEVELS]; /* per level, level 0 first (Open3D default {10, 5, 4}) */
} hv_track_params;
typedef struct hv_track_result {
    double T_cw[16];
    double information[36];
    double fitness, inlier_rmse;
    int64_t inliers, valid;
    int32_t iterations[HV_TRACK_MAX_LEVELS];
    int32_t degenerate;
    int32_t success;
} hv_track_result;
int hv_tsdf_track(hv_volume *v, const void *depth, int32_t depth_dtype, int32_t height, int32_t width, const double *intr,
                  const double *T_cw_init, const hv_track_params *params, hv_track_result *result, double *trace, int64_t trace_cap,
                  int64_t *trace_rows, int32_t loc);

/* Hybrid frame-to-model tracking (Open3D's tensor odometry "Hybrid": point-to-plane plus intensity): hv_tsdf_track with a
 * photometric term on the colour the map already holds, for scenes whose geometry leaves motions free (a wall, a floor, a table
 * top).  This project's own contract.  EVERYTHING of hv_tsdf_track holds unchanged - source depth pyramid, level intrinsics, the
 * model cast per level at T_cw_init, anchor frame, state A, association (u', v'), the inlier test, r, J, its Huber weight, the
 * solve, the degenerate rule, the stopping rule, the outputs - with these additions:
 *   source I  color [H,W,3] uint8 at loc, channel order as integrate takes it (hv_tsdf_set_color_order).  Level 0, float32:
 *             I_s = ((0.299f R + 0.587f G) + 0.114f B) / 255f.  Level l+1: (((c0 + c1) + c2) + c3) * 0.25f over the four children in
 *             the depth pyramid's child order, all four whatever their depth.
 *   model I   the per-level cast also renders colour (r, g, b) in [0, 1] (no second cast).  Per model pixel, float32:
 *             I_m = (0.299f r + 0.587f g) + 0.114f b; g_x = 0.5f (I_m(u+1, v) - I_m(u-1, v)), g_y = 0.5f (I_m(u, v+1) - I_m(u, v-1)).
 *             The pixel HAS A GRADIENT iff 1 <= u <= W-2 and 1 <= v <= H-2, the mask is set at it and at its four neighbours, and
 *             |z*(neighbour) - z*(u, v)| <= depth_outlier_trunc for each of them (the float32 cast depths subtracted and compared
 *             in double: no gradient across a depth edge).  A level narrower or lower than 3 pixels has no photometric term.
 *   photometric  double, for every inlier of hv_tsdf_track's test whose model pixel (u', v') has a gradient: with the unrounded
 *             x' = fx p_x / p_z + cx, y' = fy p_y / p_z + cy (u' = floor(x' + 0.5), v' likewise),
 *             r_I = ((I_m + g_x (x' - u')) + g_y (y' - v')) - I_s(u, v)   (I_m, g_x, g_y of (u', v'); I_s of the source pixel);
 *             a = g_x fx / p_z, b = g_y fy / p_z, c = -(a p_x + b p_y) / p_z, g3 = (a, b, c), J_I = [p x g3, g3] (omega, t);
 *             w_I = intensity_weight * (1 if |r_I| <= intensity_huber_delta else intensity_huber_delta / |r_I|).
 *             The first-order expansion about the associated pixel stands in for a bilinear sample: one record per inlier.
 *   sums      H = sum w J^T J + sum w_I J_I^T J_I and g = sum w J^T r + sum w_I J_I^T r_I: per pixel the products (w J_a) J_b, (w J_a) r,
 *             then (w_I J_I,a) J_I,b, (w_I J_I,a) r_I, are added into the same float64 sums; e, inliers and valid as before; new: the
 *             count of photometric inliers and e_I = sum r_I^2 (unweighted).  The degenerate test, information and the trace's H, g
 *             are those of the combined system.  The sums are reduced in hv_tsdf_track's order, so intensity_weight = 0 (every
 *             photometric product is then 0) gives, bit for bit, hv_tsdf_track's T_cw, information, fitness, inlier_rmse, counts,
 *             iterations and flags on the same inputs.
 *   result    base as hv_tsdf_track; of the LAST level-0 linearisation: photometric_inliers, intensity_rmse = sqrt(e_I /
 *             photometric_inliers) (0 if none).
 * trace: rows of HV_TRACK_COLOR_TRACE_STRIDE doubles: hv_tsdf_track's 56 fields in their order, then photometric inliers, e_I.
 * Depth and colour are both at loc.  Errors as hv_tsdf_track, plus HV_ERR_INVALID for a NULL color, an intensity_weight that is
 * negative or not finite, an intensity_huber_delta that is not positive and finite.  Reads only, all steps queued at once, one
 * host wait, no float atomics, bitwise reproducible: as hv_tsdf_track. */
#define HV_TRACK_COLOR_TRACE_STRIDE 58
typedef struct hv_track_color_params {
    hv_track_params base;         /* everything hv_tsdf_track takes, same meaning */
    double intensity_weight;      /* lambda >= 0: factor on the photometric normal equations */
    double intensity_huber_delta; /* > 0, in intensity units (image range [0, 1]) */
} hv_track_color_params;
typedef struct hv_track_color_result {
    hv_track_result base;
    int64_t photometric_inliers; /* of the last level-0 linearisation */
    double intensity_rmse;       /* sqrt(sum r_I^2 / photometric_inliers), unweighted, 0 if none */
} hv_track_color_result;
int hv_tsdf_track_color(hv_volume *v, const void *depth, int32_t depth_dtype, const uint8_t *color, int32_t height, int32_t width,
                        const double *intr, const double *T_cw_init, const hv_track_color_params *params, hv_track_color_result *result,
                        double *trace, int64_t trace_cap, int64_t *trace_rows, int32_t loc);

/* Frame-to-frame RGB-D odometry (the place of Open3D's rgbd_odometry_multi_scale, methods PointToPlane and Hybrid): how did the
 * camera move between two RGB-D frames - the first keyframes of a session, when the map is still empty; a relative-pose check of a
 * loop-closure candidate; a start pose for hv_tsdf_track after a fast motion.  It is hv_tsdf_track / hv_tsdf_track_color with the
 * model built from a second frame instead of a cast of the map.  This project's own contract.  The volume is context only (stream,
 * scratch, staging; any mode): nothing of the map is read or changed.  Both colours NULL: the depth-only call (hv_tsdf_track's 30
 * sums, trace rows of HV_TRACK_TRACE_STRIDE); both given: hybrid (hv_tsdf_track_color's 32 sums, HV_TRACK_COLOR_TRACE_STRIDE);
 * exactly one NULL: HV_ERR_INVALID.  EVERYTHING not listed here stays as hv_tsdf_track / hv_tsdf_track_color state it - level
 * intrinsics, source pyramid (depth and intensity, of the SOURCE frame), association, inlier test, residual, Jacobian, Huber weights,
 * the photometric expansion, the sums and their order, the solve, the degenerate and stopping rules, the trace row layout and the
 * outputs of the last level-0 linearisation:
 *   frames    ANCHOR = the target camera.  transformation = T_target_source maps a point in source-camera coordinates into
 *             target-camera coordinates; with world poses T_cw(target) inverse(T_cw(source)).  The state A starts at T_init (NULL:
 *             the identity; else finite with bottom row 0 0 0 1), A := exp(xi) A, and transformation is A itself.
 *   target    the source pyramid's rules applied to the target frame: depth z (float32, 0 = invalid) and, hybrid, intensity I_t of
 *             every level.
 *   model     per level with iterations[l] > 0, per target pixel (u, v), with P(u, v) = z ((u - cx) / fx, (v - cy) / fy, 1) in double
 *             at the level's intrinsics: mask = 1 iff 1 <= u <= W-2 and 1 <= v <= H-2, z > 0 at the pixel and its four neighbours,
 *             |z(neighbour) - z(u, v)| <= depth_outlier_trunc for each (the float32 depths subtracted and compared in double), and
 *             c = dy x dx, dx = P(u+1, v) - P(u-1, v), dy = P(u, v+1) - P(u, v-1), has a finite length sqrt((c_x c_x + c_y c_y) + c_z c_z)
 *             > 0.  normal = c / |c|, negated when (n_x P_x + n_y P_y) + n_z P_z > 0 at (u, v) (it faces the camera), each component
 *             rounded to float32; 0 where mask = 0.  The model depth is z, the vertex q = P.  The normals are in the anchor frame
 *             already: the linearisation's R0 is the identity.
 *   record    hybrid, per target pixel: I_m = I_t(u, v); where mask = 1, g_x = 0.5f (I_t(u+1, v) - I_t(u-1, v)), g_y = 0.5f
 *             (I_t(u, v+1) - I_t(u, v-1)) and has-gradient = 1, elsewhere g = 0 and has-gradient = 0: every inlier carries a
 *             photometric term, photometric_inliers == inliers.  A level narrower or lower than 3 pixels has an empty mask and ends
 *             degenerate (fewer than HV_TRACK_MIN_INLIERS inliers).
 *   result    as hv_tsdf_track; photometric_inliers and intensity_rmse are 0 in the depth-only call.  When the FIRST level-0
 *             linearisation is degenerate (empty frames are not an error), success = 0 and transformation = T_init.
 * intensity_weight and intensity_huber_delta are read (and checked) by the hybrid call only; with intensity_weight = 0 it gives the
 * depth-only call's transformation, information, fitness, inlier_rmse, counts, iterations and flags bit for bit.  Depths and colours
 * are all at loc; colour channel order as hv_tsdf_set_color_order.  Errors as hv_tsdf_track (sizes against n_levels, depth range,
 * scale, thresholds, iterations), checked before any launch.  All launches are queued at once on the volume's stream, one host
 * wait, no float atomics, bitwise reproducible.
 * hv_rgbd_odometry_model: what the call builds from its target frame, for tests and for users who want the maps - the pyramid of
 * one frame down to `level` (0 .. HV_TRACK_MAX_LEVELS - 1, H >> level >= 1), then the model of that level: depth [h,w] float32,
 * normal [h,w,3] float32, mask [h,w] uint8, record [h,w,4] float32 {I_m, g_x, g_y, has-gradient}, at loc; any may be NULL; a record
 * needs a colour.  Of params it reads depth_scale, depth_min, depth_max and depth_outlier_trunc. */
typedef struct hv_odometry_params {
    double depth_scale, depth_min, depth_max;
    double depth_outlier_trunc;   /* Open3D default 0.07 m */
    double depth_huber_delta;     /* Open3D default 0.05 m */
    double intensity_weight;      /* hybrid: lambda >= 0 */
    double intensity_huber_delta; /* hybrid: > 0, image range [0, 1] */
    int32_t n_levels;
    int32_t iterations[HV_TRACK_MAX_LEVELS]; /* per level, level 0 first */
} hv_odometry_params;
typedef struct hv_odometry_result {
    double transformation[16]; /* T_target_source, row-major */
    double information[36];
    double fitness, inlier_rmse;
    int64_t inliers, valid;
    int32_t iterations[HV_TRACK_MAX_LEVELS];
    int32_t degenerate;
    int32_t success;
    int64_t photometric_inliers;
    double intensity_rmse;
} hv_odometry_result;
int hv_rgbd_odometry(hv_volume *v, const void *source_depth, const void *target_depth, int32_t depth_dtype,
                     const uint8_t *source_color, const uint8_t *target_color, int32_t height, int32_t width, const double *intr,
                     const double *T_init, const hv_odometry_params *params, hv_odometry_result *result, double *trace,
                     int64_t trace_cap, int64_t *trace_rows, int32_t loc);
int hv_rgbd_odometry_model(hv_volume *v, const void *depth, int32_t depth_dtype, const uint8_t *color, int32_t height, int32_t width,
                           const double *intr, const hv_odometry_params *params, int32_t level, float *out_depth, float *out_normal,
                           uint8_t *out_mask, float *out_record, int32_t loc);

/* Pose-graph optimisation (the place of Open3D's pipelines::registration::GlobalOptimization with the Levenberg-Marquardt method and
 * its line process): given node poses, relative poses between pairs of them with their information matrices, and which of those are
 * trusted (odometry) and which are not (loop closures), the node poses that fit them best, with the weight of every untrusted edge.
 * This project's own contract.  The volume is context only, as for hv_rgbd_odometry (stream, scratch, staging; any mode): nothing of
 * the map is read or changed.
 *   operands  all at loc (HV_HOST arrays are staged by the library and the results copied back before the call returns).
 *             poses [N,16] float64 row-major T_wc (camera-to-world), in and out; edge_nodes [E,2] int32 {source, target}; edge_T
 *             [E,16] float64 Z = T_target_source - exactly hv_rgbd_odometry's transformation for that pair and
 *             hv_tsdf_register_volume's T_self_source; edge_info [E,36] float64, the 6 x 6 information in the order (omega, t) that
 *             xi has everywhere in this project; edge_uncertain [E] uint8 (non-zero = uncertain) or NULL = all certain;
 *             params->fixed: the node that does not move.  Rotation blocks are taken as orthonormal: every inverse is [R^T, -R^T t].
 *             Duplicate edges and edges with source > target are legal.
 *   exp, Log  exp(xi) = [Rodrigues(omega), t], hv_gauss_newton.h's: R = I + a K + b K K, K = [omega]x, th = |omega|, a = sin th / th,
 *             b = (1 - cos th) / th^2 (a = 1, b = 1/2 for th < 1e-8); the translation part is t itself.  Log(T) = (Log R, t) inverts it:
 *             v = (R21 - R12, R02 - R20, R10 - R01) / 2, s = |v|, c = (trace R - 1) / 2, th = atan2(s, c);
 *               c >= -0.99, s >= 1e-8   omega = v th / s
 *               c >= -0.99, s <  1e-8   omega = v                               (small angle)
 *               c <  -0.99              near pi, where v vanishes: A = ((R + R^T) / 2 - c I) / (1 - c) = a a^T for the axis a; k = the
 *                                       first largest diagonal entry of A, a = A[k, :] / sqrt(A[k, k]), normalised, negated when
 *                                       a . v < 0; omega = th a.
 *   residual  per edge X = inv(T_t) T_s inv(Z), r = Log(X) = (omega, t).  edge_info is used as the odometry returns it: its
 *             information is about a left perturbation exp(xi) T_target_source, and Log(P inv(Z)) is that xi.
 *   update    T_i := exp(d_i) T_i.  With it J_t = -J_s and J_s = Jl^-1(r) Ad(inv(T_t)), where for inv(T_t) = [Ra, ta]
 *               Ad = [[Ra, 0], [[ta]x Ra, Ra]]                              ((omega, t) order; first order of A exp(d) inv(A))
 *               Jl^-1(r) = [[Jw(omega), 0], [-[t]x, I]]                     (closed form: the left Jacobian of THIS exp, rotation and
 *                                                                            translation uncoupled except through exp(d) acting on t)
 *               Jw = I - K / 2 + c2 K K, c2 = 1 / th^2 - cos(th / 2) / (2 th sin(th / 2)), finite up to th = pi; for th < 0.05 its
 *                    series 1/12 + th^2 / 720 + th^4 / 30240 (the closed form cancels there; the series' next term is below 2e-17)
 *             so J_s = [[Jw Ra, 0], [[ta - t]x Ra, Ra]].
 *   edge      M_e = l_e J_s^T Omega_e J_s goes to the blocks (s,s) and (t,t) and -M_e to (s,t) and (t,s); g_e = l_e J_s^T Omega_e r
 *             goes to s and -g_e to t.  The optimiser keeps M_e (its upper triangle) and g_e per edge and nothing else.
 *   objective F = sum_e l_e chi2_e + sum_uncertain mu (sqrt(l_e) - 1)^2, chi2_e = r^T Omega_e r; l_e = 1 for a certain edge, l_e =
 *             (mu / (mu + chi2_e))^2 for an uncertain one, recomputed from the state at EVERY evaluation (linearisation and trial).
 *             mu = line_process_weight, default 1.  An uncertain edge is switched off (l < 1/4) when chi2_e > mu, so mu is the chi2
 *             of the worst loop edge the caller still wants to keep: about (the largest acceptable residual)^2 times the typical
 *             diagonal of the loop edges' information (Open3D derives it from preference_loop_closure and the mean information; this
 *             call takes the number).  edge_weight_out [E] at loc (may be NULL): the final l_e; kept = l_e >= edge_prune_threshold
 *             (default 0.25); the call marks edges and never removes one.
 *   outer     Levenberg-Marquardt on (H + lambda I) d = -b, b = the sum of +-g_e, lambda_0 = lambda_scale max diag H (default 1e-5,
 *             Open3D's tau) over the free nodes.  Gain ratio rho = (F - F_trial) / (d . (lambda d - b)), which is the model's decrease
 *             for every CG iterate started at 0; rho is 0 when the denominator is not positive or F_trial is not a number.  Accepted
 *             iff rho > 0: lambda *= max(1/3, 1 - (2 rho - 1)^3), nu = 2; else lambda *= nu, nu *= 2 (Nielsen).  An iteration stops
 *             the call, rules tested in this order: F <= residual_tolerance (HV_POSE_GRAPH_RESIDUAL, no step taken); max |b| <=
 *             gradient_tolerance (HV_POSE_GRAPH_GRADIENT, no step taken); |d|_2 <= step_tolerance (HV_POSE_GRAPH_STEP, the step taken
 *             if accepted); accepted and F - F_trial <= decrease_tolerance F (HV_POSE_GRAPH_DECREASE); max_iterations reached
 *             (converged = 0).  Defaults 1e-6 each and 100 iterations, Open3D's GlobalOptimizationConvergenceCriteria.
 *   inner     block-Jacobi preconditioned conjugate gradients from x = 0 over the free nodes (the fixed node's rows and columns are
 *             dropped); the preconditioner is the Cholesky factor of each node's 6 x 6 block D_i + lambda I.  It ends when
 *             sqrt(r.z / r0.z0) <= cg_tolerance (default 1e-8) or after cg_max_iterations (default 100): a truncated solve is still a
 *             descent step with the rho above.  The matrix is never formed: a product is one pass over the edges, u_e = M_e (x_s -
 *             x_t), and one over the nodes, which add +u_e / -u_e in the order of their incidence list (a CSR built once per call on
 *             the host, sorted by edge index).  Dot products, F and the norms are two-stage sums in a fixed order; no float atomics;
 *             bitwise reproducible run to run.  alpha, beta and the "done" flag live on the device: a finished CG turns the rest of
 *             its queued launches into no-ops, and there is no host wait inside the CG loop.  An outer iteration queues 7 + 4
 *             cg_max_iterations launches and costs ONE host wait (the read of its decision).  The call adds one wait for its start,
 *             one for its results and, with loc = HV_DEVICE, one to fetch the operands for the checks below.
 *   result    chi2_initial / chi2_final: F at the first linearisation / at the final state; lambda: the last; iterations: outer
 *             iterations run; cg_iterations_total; edges_kept: edges with l_e >= edge_prune_threshold (certain ones included);
 *             converged: the rule that stopped the call (HV_POSE_GRAPH_*, 0 = max_iterations); success = converged != 0, every
 *             block factorisation had positive pivots and chi2_final is finite.
 *   trace     (host memory for either loc, may be NULL) one row of HV_POSE_GRAPH_TRACE_STRIDE doubles per outer iteration, at most
 *             trace_cap: {iteration, lambda, F before, F of the trial, rho, accepted, CG iterations, CG residual sqrt(r.z / r0.z0),
 *             |d|_2, max |b|, the new lambda, the rule that fired or 0}.  With params->trace_state, trace_poses [trace_cap, N, 16]
 *             (host) receives the poses each iteration STARTED from, so that a restatement can be fed the same state.
 *   errors    HV_ERR_INVALID, all checked on the host before any launch, poses untouched: N < 1; fixed outside 0..N-1; a node index
 *             outside 0..N-1; a self edge; a pose or Z that is not finite or whose bottom row is not 0 0 0 1; an information matrix
 *             that is not finite or not symmetric BITWISE (Omega[a][b] == Omega[b][a]); a node that is not connected to `fixed`
 *             through CERTAIN edges (union-find on the host; the message says so) - the line process could cut it loose; parameters
 *             out of range.  E == 0 with N == 1 is a no-op with success = 1.
 * hv_pose_graph_linearise: what one linearisation of the call computes at the given poses, for tests: per edge r [E,6], chi2 [E],
 * l [E], M_e [E,36] (full, symmetric), g_e [E,6] and the gradient b [N,6] (no node fixed), outputs in HOST memory for either loc, any
 * may be NULL; the same kernels, the same checks except connectivity. */
#define HV_POSE_GRAPH_TRACE_STRIDE 12
#define HV_POSE_GRAPH_GRADIENT 1
#define HV_POSE_GRAPH_STEP 2
#define HV_POSE_GRAPH_DECREASE 3
#define HV_POSE_GRAPH_RESIDUAL 4
typedef struct hv_pose_graph_params {
    double line_process_weight;  /* mu > 0, default 1 */
    double edge_prune_threshold; /* default 0.25 */
    double lambda_scale;         /* default 1e-5 */
    double gradient_tolerance;   /* max |b|, default 1e-6 (Open3D min_right_term) */
    double step_tolerance;       /* |d|_2, default 1e-6 (Open3D min_relative_increment, here absolute) */
    double decrease_tolerance;   /* (F - F_trial) / F, default 1e-6 (Open3D min_relative_residual_increment) */
    double residual_tolerance;   /* F, default 1e-6 (Open3D min_residual) */
    double cg_tolerance;         /* default 1e-8 */
    int32_t max_iterations;      /* default 100 (Open3D max_iteration) */
    int32_t cg_max_iterations;   /* default 100 */
    int32_t fixed;               /* default 0 */
    int32_t trace_state;
} hv_pose_graph_params;
typedef struct hv_pose_graph_result {
    double chi2_initial, chi2_final, lambda;
    int32_t iterations, cg_iterations_total, edges_kept, converged, success;
} hv_pose_graph_result;
void hv_pose_graph_default_params(hv_pose_graph_params *params);
int hv_pose_graph_optimize(hv_volume *v, double *poses, int64_t n_nodes, const int32_t *edge_nodes, const double *edge_T,
                           const double *edge_info, const uint8_t *edge_uncertain, int64_t n_edges, const hv_pose_graph_params *params,
                           double *edge_weight_out, hv_pose_graph_result *result, double *trace, double *trace_poses, int64_t trace_cap,
                           int64_t *trace_rows, int32_t loc);
int hv_pose_graph_linearise(hv_volume *v, const double *poses, int64_t n_nodes, const int32_t *edge_nodes, const double *edge_T,
                            const double *edge_info, const uint8_t *edge_uncertain, int64_t n_edges, double line_process_weight,
                            double *r_out, double *chi2_out, double *l_out, double *M_out, double *g_out, double *gradient_out,
                            int32_t loc);

/* ---- bundle adjustment ---------------------------------------------------------------------------------------
 * hv_bundle_adjust: Levenberg-Marquardt over camera poses AND points against pixel measurements, with the Schur complement on the
 * points as the inner system.  It takes the place of the reference's bundle_adjustment / global_bundle_adjustment /
 * local_bundle_adjustment / pose_optimization (pyslam/slam/optimizer_g2o.py, g2o's EdgeSE3ProjectXYZ and EdgeStereoSE3ProjectXYZ with
 * a Huber kernel); g2o's solver is not reproduced - the algorithm is fixed by the rules below, restated in numpy in
 * tests/bundle_reference.py.  The volume is context only, as for hv_pose_graph_optimize (stream, scratch, staging; any mode).
 *   B1 state     cameras [N,16] float64 row-major T_cw (world to camera: the reference's Tcw, this project's extrinsics), in and
 *                out; points [M,3] float64 in the world, in and out; camera_fixed [N] uint8 (non-zero = does not move) or NULL = none;
 *                params->fixed_points: no point moves (pose-only, the reference's pose_optimization); one pinhole per call, params->
 *                fx, fy, cx, cy, bf (bf = baseline times fx; it must be positive even when no observation is stereo).
 *   B2 observation  obs_index [O,2] int32 {camera, point}; obs_meas [O,4] float64 {u, v, u_r, inv_sigma2}; obs_active [O] uint8 or
 *                NULL = all.  With q = R p + t, pi(q) = (fx q_x / q_z + cx, fy q_y / q_z + cy): u_r not finite = monocular, r = (u, v)
 *                - pi(q); else stereo / RGB-D, r = (u, v, u_r) - (pi(q), pi_u(q) - bf / q_z).  Information inv_sigma2 I, so chi2 =
 *                inv_sigma2 r.r.  Duplicate (camera, point) pairs are legal: each observation is a term of its own.
 *   B3 kernel    params->huber: rho = chi2 when chi2 <= delta2, else 2 delta sqrt(chi2) - delta2; the weight w = rho' = 1, else
 *                delta / sqrt(chi2); delta2 = huber_delta2_mono (5.991) / huber_delta2_stereo (7.815).  Without it rho = chi2, w = 1.
 *                F = sum of rho over the active observations.  The normal equations take w as a constant (g2o's robustified
 *                information): with J = d r / d q, A_o = w inv_sigma2 J^T J and g_o = w inv_sigma2 J^T r.
 *   B4 depth     an active observation with q_z <= min_depth (default 1e-6) at the call's FIRST linearisation is switched off for
 *                the whole call and reported in behind_out [O] uint8.  A trial state in which a still-active observation has q_z <=
 *                min_depth has F_trial = not-a-number: rho_gain = 0 and the step is rejected.  So every accepted state keeps every
 *                active observation in front of its camera and F is continuous along the call.
 *   B5 update    camera T := exp(d) T, exp as in the pose-graph section, (omega, t) order, translation uncoupled: d q / d d =
 *                W(q) = [-[q]x, I].  Point p := p + d: d q / d d = R.  So an observation adds W^T A W to its camera's block B_i, R^T A R
 *                to its point's block C_j, E_o = W^T A R between them, W^T g to the camera's gradient and R^T g to the point's.
 *   B6 outer     the pose graph's Levenberg-Marquardt to the letter: (H + lambda I) d = -b with lambda I on camera and point blocks,
 *                lambda_0 = lambda_scale max diag H over the free variables; gain ratio (F - F_trial) / (d . (lambda d - b)); Nielsen's
 *                update; the four stopping rules in the pose graph's order with its codes (HV_POSE_GRAPH_*); its trace row layout.
 *   B7 inner     H = [[B, E], [E^T, C]], C block-diagonal.  Preconditioned CG from x = 0 on S x = -(b_c - E (C + lambda I)^-1 b_p),
 *                S = (B + lambda I) - E (C + lambda I)^-1 E^T over the free cameras, never formed: a product is one pass cameras ->
 *                observations -> points, y_j = (C_j + lambda I)^-1 sum_o E_o^T x, and one pass back, (B_i + lambda I) x_i - sum_o E_o
 *                y_j.  Then d_j = -(C_j + lambda I)^-1 (b_j + sum_o E_o^T x).  (C_j + lambda I)^-1 is formed once per linearisation
 *                through its Cholesky factor.  Preconditioner: the Cholesky factor of (B_i + lambda I) - sum_o E_o (C_j + lambda I)^-1
 *                E_o^T, the sum over the camera's observations one by one.  Stopping as in the pose graph (cg_tolerance,
 *                cg_max_iterations).  With fixed_points E and the points' gradient are taken as zero in the same code: S is block-
 *                diagonal and the CG ends after one iteration.  A fixed camera has x = 0 and the unit factor.
 *   B8 sums      no float atomics.  Two incidence lists are built once per call on the host (the observations of a camera, of a
 *                point), each sorted by observation index and holding inactive observations too (they add zeros).  A point's sums run
 *                down its list in order.  A camera's sums: lane l of 64 adds the list's entries l, l + 64, ... in order, the 64 lanes
 *                are added by xor butterfly (offsets 32, 16, ..., 1).  Sums over observations, cameras and points for F, the dot
 *                products and the norms: 256 consecutive items by butterfly per 64 and the four sixty-fours in order, then the groups
 *                in order.  Bitwise reproducible run to run.
 *   result       as hv_pose_graph_result; chi2_out [O] float64 at loc (may be NULL): chi2 at the final state, 0 for an observation that
 *                is inactive or behind; behind_out [O] uint8 at loc (may be NULL).  trace as for the pose graph; with params->
 *                trace_state, trace_cameras [trace_cap,N,16] and trace_points [trace_cap,M,3] (host) receive the state each iteration
 *                STARTED from.
 *   errors       HV_ERR_INVALID, all checked on the host before any launch, operands untouched: N or M < 1 with observations
 *                present; an index out of range; a camera, point, u or v that is not finite; a bottom row not 0 0 0 1; inv_sigma2 not
 *                positive and finite; no fixed camera while the points are free; fx, fy or bf not positive; parameters out of range.
 *                Not errors: no observation, or none active (a no-op with success = 1, converged = HV_POSE_GRAPH_RESIDUAL); every camera fixed
 *                with the points free (points only).
 * hv_bundle_linearise: one linearisation at the given state, for tests: per observation r [O,3] (third entry 0 for a monocular one),
 * chi2 [O], w [O], behind [O]; per camera B [N,36] and b [N,6] (no camera fixed); per point C [M,9] and b [M,3]; F.  Outputs in HOST
 * memory for either loc, any may be NULL; the same kernels, the same checks except the fixed camera. */
typedef struct hv_bundle_params {
    double fx, fy, cx, cy, bf;
    double huber_delta2_mono;   /* default 5.991 */
    double huber_delta2_stereo; /* default 7.815 */
    double min_depth;           /* default 1e-6 */
    double lambda_scale;        /* default 1e-5 */
    double gradient_tolerance, step_tolerance, decrease_tolerance, residual_tolerance; /* default 1e-6 each */
    double cg_tolerance;        /* default 1e-8 */
    int32_t max_iterations;     /* default 100 */
    int32_t cg_max_iterations;  /* default 100 */
    int32_t huber;              /* default 1 */
    int32_t fixed_points;       /* default 0 */
    int32_t trace_state;
    int32_t reserved;
} hv_bundle_params;
typedef struct hv_bundle_result {
    double chi2_initial, chi2_final, lambda;
    int32_t iterations, cg_iterations_total, converged, success;
} hv_bundle_result;
void hv_bundle_default_params(hv_bundle_params *params);
int hv_bundle_adjust(hv_volume *v, double *cameras, int64_t n_cameras, double *points, int64_t n_points, const uint8_t *camera_fixed,
                     const int32_t *obs_index, const double *obs_meas, const uint8_t *obs_active, int64_t n_obs,
                     const hv_bundle_params *params, double *chi2_out, uint8_t *behind_out, hv_bundle_result *result, double *trace,
                     double *trace_cameras, double *trace_points, int64_t trace_cap, int64_t *trace_rows, int32_t loc);
int hv_bundle_linearise(hv_volume *v, const double *cameras, int64_t n_cameras, const double *points, int64_t n_points,
                        const int32_t *obs_index, const double *obs_meas, const uint8_t *obs_active, int64_t n_obs,
                        const hv_bundle_params *params, double *r_out, double *chi2_out, double *w_out, uint8_t *behind_out, double *B_out,
                        double *bc_out, double *C_out, double *bp_out, double *F_out, int32_t loc);

/* ---- oriented binary keypoints and Hamming matching ---------------------------------------------------------
 * hv_orb_detect: a uint8 image -> keypoints of a FAST-9 segment test on a factor-2 pyramid, each with an orientation bin and a
 * 256-bit binary descriptor steered to that bin; hv_match_descriptors: brute-force Hamming matching of such descriptors against one
 * or many sets.  Together with pyslam_amd/features.py they are what the reference's loop closing does by appearance
 * (pyslam/local_features/feature_matcher.py:76-136,371-396, cpp/hamming/, pyslam/loop_closing/loop_closing.py:266-365).  OpenCV is
 * not a dependency; compatibility with cv2.ORB descriptors or a DBoW vocabulary is not claimed, and the descriptor pattern is not
 * the learned ORB pattern: it is generated (F10).  The algorithm is fixed by the rules below, restated in numpy in
 * tests/orb_reference.py, and the library is held to that restatement bit for bit.  Integer arithmetic only.
 *   F1 grey         stereo rule 1
 *   F2 pyramid      level 0 is the grey image [H_0,W_0]; level l+1 is [H_l / 2, W_l / 2] (integer division), each pixel
 *                   (a + b + c + d + 2) >> 2 of its 2x2 block.  A level with H_l < 33 or W_l < 33 yields nothing, and neither does
 *                   any level after it
 *   F3 segment test the 16 ring offsets (dx,dy) start at (0,-3) and go clockwise: (0,-3) (1,-3) (2,-2) (3,-1) (3,0) (3,1) (2,2) (1,3)
 *                   (0,3) (-1,3) (-2,2) (-3,1) (-3,0) (-3,-1) (-2,-2) (-1,-3).  With c the centre and t = threshold, a ring pixel r is
 *                   brighter iff r - c > t, darker iff c - r > t.  A pixel is a corner iff at least 9 circularly contiguous ring
 *                   pixels are brighter, or at least 9 are darker.  Candidates only at 16 <= x < W_l - 16, 16 <= y < H_l - 16
 *   F4 score        V = max(sum over the brighter ring pixels of r - c - t, sum over the darker ones of c - r - t), over all 16 ring
 *                   pixels; 0 for a non-corner
 *   F5 suppression  a corner survives iff for each of its 8 neighbours n: V > V_n, or V == V_n and n comes later in row-major order;
 *                   pixels outside the candidate region count as 0
 *   F6 selection    cells are 32x32, aligned to the level's origin; each keeps its per_cell survivors of largest V, ties to the smaller
 *                   row-major index
 *   F7 order        level ascending, then cell in row-major order, then rank in the cell (V descending, index ascending)
 *   F8 orientation  over the disc dx^2 + dy^2 <= 225 on the level's grey g: m10 = sum dx g, m01 = sum dy g.  The bin is the SMALLEST
 *                   b in 0..31 that maximises m10 CX[b] + m01 CY[b] in int64; CX[b] = round(1024 cos(2 pi b / 32)),
 *                   CY[b] = round(1024 sin(2 pi b / 32)), literal tables (m10 = m01 = 0 takes bin 0)
 *   F9 smoothing    s(y,x) = the 5x5 box sum of the level's grey centred on the pixel (the border keeps every read inside the image)
 *   F10 pattern     256 point pairs (A[k], B[k]) with integer coordinates in the disc of radius 13, drawn by this generator:
 *                   x <- (1103515245 x + 12345) mod 2^31 starting from x = 1 (HV_ORB_PATTERN_SEED); one draw is ((x >> 16) mod 27) - 13;
 *                   a point is two draws (px, py), both redrawn while px^2 + py^2 > 169; pair k is a point A, then a point B redrawn
 *                   while B == A, k = 0..255 in the order drawn.  For bin b, with c = cos(2 pi b / 32), s = sin(2 pi b / 32) in
 *                   float64: A_b[k] = (floor(c ax - s ay + 0.5), floor(s ax + c ay + 0.5)), B_b[k] alike.  tools/gen_orb_pattern.py
 *                   writes the pattern, its 32 rotations and CX / CY into pyslam_amd/csrc/orb_pattern.h as literal arrays
 *   F11 bit k       s(p + A_b[k]) < s(p + B_b[k]), stored in byte k >> 3, bit k & 7
 * image: [height,width] (channels 1) or [height,width,3] uint8.  keypoints_out: int32 [capacity,5] = x, y (at the keypoint's level),
 * level, score V, orientation bin; the level-0 position of a keypoint is ((x + 0.5) 2^level - 0.5, (y + 0.5) 2^level - 0.5).
 * descriptors_out: uint8 [capacity,32].  Rows 0 .. *count_out - 1 are written, in the F7 order; capacity (rows of both arrays) must
 * be at least the bound: per_cell times the 32x32 cells (partial ones included) of every level that yields - the library never
 * truncates.  count_out is HOST memory.  `loc` as in hv_stereo_sgm for the image and the two arrays; the call waits for the stream
 * for either loc, because it returns the count.  Works on a volume of any mode and reads nothing of it; scratch (the grey pyramid,
 * a uint16 score map of the same layout, 8 bytes per cell and 12 per cell and rank) is owned by the handle.
 * HV_ERR_INVALID before anything is launched or written: a NULL pointer, channels not 1 or 3, height or width < 1 or > 32768,
 * levels outside 1..8, threshold outside 1..254, per_cell outside 1..16, capacity below the bound. */
typedef struct hv_feature_params {
    int32_t levels;    /* 3 */
    int32_t threshold; /* 20 */
    int32_t per_cell;  /* 8 */
} hv_feature_params;
int hv_orb_detect(hv_volume *v, const uint8_t *image, int32_t height, int32_t width, int32_t channels, const hv_feature_params *params,
                  int32_t *keypoints_out, uint8_t *descriptors_out, int64_t capacity, int32_t *count_out /* host */, int32_t loc);
/* hv_match_descriptors: query uint8 [n_query,32] against train uint8 [n_train,32], which segment_offsets (int32 [n_segments + 1],
 * HOST memory for either loc: non-decreasing, first 0, last n_train) cuts into segments - one keyframe's descriptors each;
 * n_segments = 1 is plain two-set matching.  Per segment s and query i:
 *   M1 distance     popcount of the 256-bit xor
 *   M2 best, second j1 = the smallest train index in the segment attaining the minimum distance d1; d2 = the minimum over the segment
 *                   without j1 (65535 when the segment has one descriptor); d1 = 65535 and j1 = -1 when the segment is empty
 *   M3 acceptance   d1 <= max_distance and 100 d1 < ratio_percent d2; ratio_percent 0 skips the second half
 *   M4 cross-check  (cross_check 1) among all n_query queries, the smallest query index attaining the minimum distance to train j1 is i
 *   M5 outputs      index int32 [n_segments,n_query]: the global train index j1 of an accepted match, else -1; distance and second
 *                   uint16 [n_segments,n_query]: d1 and d2, accepted or not; counts int32 [n_segments]: the number accepted.  Any
 *                   output but index may be NULL
 * Every result is independent of the order of execution.  `loc` as in hv_stereo_sgm (device descriptors 4-byte aligned).  Scratch
 * (4 bytes per train descriptor, 4 per segment and query) is owned by the handle.
 * HV_ERR_INVALID before anything is launched or written: a NULL query, offsets, params or index (train may be NULL when n_train is 0);
 * n_query outside 1..65536; n_train outside 0..2^24 - 1; n_segments < 1 or n_segments n_query >= 2^27; max_distance outside 0..256;
 * ratio_percent outside 0..100; cross_check not 0 or 1; offsets that decrease, do not start at 0 or do not end at n_train. */
typedef struct hv_match_params {
    int32_t max_distance;  /* 64 */
    int32_t ratio_percent; /* 80; 0 disables the ratio half of M3 */
    int32_t cross_check;   /* 1 */
} hv_match_params;
int hv_match_descriptors(hv_volume *v, const uint8_t *query, int32_t n_query, const uint8_t *train, int32_t n_train,
                         const int32_t *segment_offsets /* host */, int32_t n_segments, const hv_match_params *params, int32_t *index_out,
                         uint16_t *distance_out /* may be NULL */, uint16_t *second_out /* may be NULL */,
                         int32_t *counts_out /* may be NULL */, int32_t loc);

/* Pruning: give units back to the pool. Fusion only ever claims units - the touch pass claims every unit within sdf_trunc of a
 * sampled depth point, whether or not a voxel of it is then updated, and de-integration leaves the units it emptied allocated - so
 * a long session holds units that carry nothing, and units far from where the camera now is.  This project's own contract (Open3D's
 * ScalableTSDFVolume never frees a unit):
 *   empty     release_empty != 0: a unit goes when all R^3 weights are 0.  (A voxel of weight 0 is in the fresh state in all five
 *             planes - integrate's initial state and de-integration's w0 == n rule - so the weight plane alone decides.)
 *   outside   unit_lo / unit_hi ([3] each, both or neither): a unit goes when its index lies outside the INCLUSIVE range
 *             [unit_lo, unit_hi] on some axis, observed voxels and all.  The caller converts metres to unit indices
 *             (floor(x / (voxel_size * 16)) per axis keeps every unit whose half-open box meets the closed box in metres).
 *   stats     units_before = units held at the call; units_outside; units_empty (a unit that is both counts as outside only - it is
 *             not read); units_after = units_before - units_outside - units_empty.  Neither criterion: a no-op, {n, 0, 0, n}.
 *   after     hv_tsdf_dump = the dump before with the released units' rows removed, bit for bit; hv_num_blocks, hv_tsdf_unit_keys
 *             and the dump agree on units_after; hv_max_blocks is unchanged (the allocation does not shrink: the released blocks can
 *             be claimed again, and are all zero like every block never handed out).  Units in use are blocks [0, units_after) again
 *             - survivors from the tail move into the holes, at most min(released, kept) of them - and the table holds exactly the
 *             surviving keys: keys claimed without a block by an overflowed call are gone and the latched overflow is cleared, as
 *             after hv_reserve_blocks.  The "dirty since the last merge" stamps follow their units (hv_tsdf_dirty_keys = before
 *             minus the released keys); hv_tsdf_touched lists nothing until the next integrate; a stored device halo plan is
 *             dropped; cached extraction results and the per-unit extraction caches are recomputed.  If NOTHING is released the
 *             volume is left exactly as it was, caches included.
 * The batch pipeline is drained first; the call waits for the GPU.  Device work: one wave per unit streams the weight plane (16 KiB,
 * 16 bytes per lane, leaving at the first weight it sees; a unit outside the range is not read), a one-workgroup scan plans the moves,
 * the host reads the four counts, then one launch moves the tail's survivors (sources and destinations are disjoint), the freed tail
 * is zeroed and the table re-keyed in place.  Extra device memory: 13 bytes per unit plus 20 bytes per table slot, never a second
 * pool.  HV_ERR_MODE for a non-TSDF volume and for a tile-sharded one (hv_tsdf_set_tile: its ranks must agree on the unit set; an
 * owner-sharded volume prunes the units it owns), HV_ERR_INVALID for one of unit_lo / unit_hi alone or unit_lo > unit_hi. */
typedef struct hv_prune_stats {
    int64_t units_before, units_outside, units_empty, units_after;
} hv_prune_stats;
int hv_tsdf_prune(hv_volume *v, int32_t release_empty, const int32_t *unit_lo /* [3] or NULL */,
                  const int32_t *unit_hi /* [3] or NULL */, hv_prune_stats *stats /* may be NULL */);

/* Volume-to-volume fusion: the observations of `src` enter `dst` through a rigid transform, p_dst = T_dst_src p_src (row-major 4x4
 * double, R = its upper 3x3, t = its last column).  For joining submaps whose relative pose is known, for moving a map to another
 * frame (one merge into an empty volume), for adding maps whose voxel lattices do not coincide.  This project's own contract
 * (Open3D has no such call).  src is only read.  For EVERY voxel of the destination lattice, with global index i = 16 key + xyz per
 * axis, all arithmetic float64, one IEEE operation per step in the order written, no contraction:
 *   locate    d_a = ((double)i_a + 0.5) * voxel_length - t_a;   p_a = (R_0a d_0 + R_1a d_1) + R_2a d_2   (R^-1 is taken as R^T);
 *             g_a = p_a / voxel_length - 0.5;  g0_a = floor(g_a);  r_a = g_a - g0_a.  The eight source voxels are g0 + {0,1}^3 in
 *             hv_tsdf_at's corner order; the NEAREST is g0_a + (r_a >= 0.5 ? 1 : 0) per axis.  A source voxel is OBSERVED when its
 *             unit exists and its weight is > 0.  A point with some |g_a| >= 1e9 (or not finite) has no observed voxel around it.
 *   sample    nearest unobserved: the destination voxel is not touched.  All eight observed: tsdf_s = the trilinear interpolation
 *             of the eight tsdf values (float32 widened), (1-r0)((1-r1)((1-r2) f0 + r2 f4) + r1((1-r2) f3 + r2 f7)) +
 *             r0((1-r1)((1-r2) f1 + r2 f5) + r1((1-r2) f2 + r2 f6)), and mean_s per channel the same expression of the eight mean
 *             colours (double)sum / (double)weight.  Otherwise tsdf_s and mean_s are the nearest voxel's.  In both cases w_s is the
 *             nearest voxel's weight: weights stay integer observation counts.
 *   update    with the destination voxel's tsdf0, w0 and sums:  weight = w0 + w_s;
 *             tsdf = (float)(((double)tsdf0 * (double)w0 + tsdf_s * (double)w_s) / (double)(w0 + w_s));
 *             each colour sum gains (uint32) floor(mean_s * (double)w_s + 0.5).
 *   units     afterwards dst holds its former units plus exactly the units (inside the key range) in which at least one voxel was
 *             updated - no all-zero unit is left behind.  The pool grows as for integrate (HV_ERR_CAPACITY, dst unchanged, if it
 *             cannot).  Updated units get a new stamp: incremental extraction and hv_tsdf_dirty_keys see them; cached extraction
 *             results are dropped.  If no voxel is updated (src holds no observed voxel) dst is left exactly as it was, caches
 *             included.
 *   stats     units_source = source units that hold a weight; units_claimed = units new in dst; voxels_trilinear / voxels_nearest
 *             = voxels updated from an interpolated / a nearest sample; voxels_updated = their sum.
 * No float atomics; every destination voxel is written by one lane from values only it computes: two calls on equal inputs give
 * bitwise equal dumps.  Both volumes' batch pipelines are drained, src's pending work is waited for, the device work is queued on
 * dst's stream and the call waits for it.  Device work: one wave per source unit (emptiness as hv_tsdf_prune) names candidate
 * units through a scratch key set; one workgroup per candidate evaluates only the nearest-observed predicate and leaves at the first
 * hit; the host reads the count; claim; one workgroup per kept unit resolves the 3 x 3 x 3 source units it can reach into LDS and
 * sweeps its voxels.  Extra device memory, freed before the call returns: with c = 27 x (units src holds), 8 c bytes of candidate
 * keys, 8 c of kept keys and a key set of 8 x (the power of two >= max(1024, 2 c)) bytes - under 108 keys per unit - plus 256 bytes.
 * NOT given: frames fused into src cannot later be de-integrated from dst exactly (their contribution was resampled); every merge
 * resamples once, so chained merges accumulate interpolation error - to move a map, merge it ONCE into an empty volume.
 * NOT given either: weights of 2^24 and more.  Weights and colour sums are uint32 counters that the merge adds without a check:
 * hv_tsdf_dump reports weights as float32 (exact below 2^24 only) and a colour sum wraps past 2^32, i.e. near 1.68e7
 * observations of a voxel at full brightness.
 * HV_ERR_MODE when either volume is not TSDF or is tile- or owner-sharded; HV_ERR_INVALID for dst == src, volumes that differ in
 * voxel_length, sdf_trunc, unit resolution or device, a non-finite T, |R^T R - I|_inf > 1e-6 (largest absolute row sum) or
 * det R < 0, a bottom row other than (0, 0, 0, 1).  HV_ERR_CAPACITY, dst unchanged, when src's pool overflowed in an earlier call
 * (hv_reserve_blocks or hv_reset it first), when the scratch key set overflows (it cannot, by the bound above), or when dst's pool
 * cannot grow.  HV_ERR_DEVICE from the sweep itself (a device fault after the claim) is the one path on which dst may be left with
 * claimed units that were not written, under a new content version: hv_tsdf_prune releases them. */
typedef struct hv_merge_stats {
    int64_t units_source, units_claimed, voxels_updated, voxels_trilinear, voxels_nearest;
} hv_merge_stats;
int hv_tsdf_integrate_volume(hv_volume *dst, hv_volume *src, const double *T_dst_src /* [16] */, hv_merge_stats *stats /* may be NULL */);

/* Map-to-map registration: refine the rigid transform p_dst = T p_src between two TSDF volumes on their signed distance fields
 * (SDF-2-SDF, voxgraph's submap constraints), for maps whose frames are gone - the transform hv_tsdf_integrate_volume takes as
 * given.  A REFINEMENT, not a global search: the field knows distances only inside the truncation band, so T_init must be good to
 * roughly (1 - tsdf_band) * sdf_trunc.  This project's own contract.  Both volumes are only read.  All geometry float64, one IEEE
 * operation per step in the order written, no contraction:
 *   candidates  fixed for the call: every source voxel with (double)weight > weight_threshold and |(double)tsdf_s| <= tsdf_band (a
 *             saturated voxel carries no distance), in pool order of the units and word order (z, x, y) inside a unit.  Its point
 *             is the voxel centre x_a = ((double)i_a + 0.5) * voxel_length, i = 16 key + xyz.
 *   anchor    cs_a = ((double)(kmin_a + kmax_a + 1) * 0.5) * (16.0 * voxel_length): the centre of the bounding box of the source's
 *             unit keys (all units it holds), computed on the host; c_a = ((T_a0 cs_0 + T_a1 cs_1) + T_a2 cs_2) + T_a3 with T =
 *             T_init.  State A (4x4) = identity at the start, kept on the device.  With R = T_init's rotation:
 *             d_a = x_a - cs_a;  q_a = (R_a0 d_0 + R_a1 d_1) + R_a2 d_2   (= T_init x - c, taken as R (x - cs) so that two far-away
 *             points are never subtracted);  y_a = ((A_a0 q_0 + A_a1 q_1) + A_a2 q_2) + A_a3;  p_a = c_a + y_a, the point in the
 *             destination frame.  H and g are those of motions about c: they do not degrade far from the world origin.
 *   sample    p is located in the destination lattice as hv_tsdf_integrate_volume locates a point in the source lattice:
 *             g_a = p_a / voxel_length - 0.5, g0_a = floor(g_a), r_a = g_a - g0_a; some |g_a| >= 1e9 (or not finite): invalid.  The
 *             eight voxels f0..f7 are g0 + {0,1}^3 in hv_tsdf_at's corner order ((0,0,0) (1,0,0) (1,1,0) (0,1,0) (0,0,1) (1,0,1)
 *             (1,1,1) (0,1,1)).  VALID iff all eight exist (unit held, key in range) and have (double)weight > weight_threshold.
 *             With u_a = 1 - r_a and the float32 values widened:
 *               c00 = u2 f0 + r2 f4,  c01 = u2 f3 + r2 f7,  c10 = u2 f1 + r2 f5,  c11 = u2 f2 + r2 f6,
 *               b0 = u1 c00 + r1 c01,  b1 = u1 c10 + r1 c11,  phi_d = u0 b0 + r0 b1      (the merge contract's trilinear expression)
 *             and its analytic derivative (eight gathers per candidate, not hv_tsdf_extract_point_normals' 48):
 *               dphi/dr0 = b1 - b0
 *               dphi/dr1 = u0 (c01 - c00) + r0 (c11 - c10)
 *               dphi/dr2 = u0 (u1 (f4 - f0) + r1 (f7 - f3)) + r0 (u1 (f5 - f1) + r1 (f6 - f2))
 *             grad_a = (sdf_trunc / voxel_length) * dphi/dr_a, metres per metre.
 *   residual  rho = sdf_trunc * (phi_d - (double)tsdf_s), metres.  INLIER iff the sample is valid and |rho| <= residual_trunc.
 *             J = [y x grad, grad] (omega, t); Huber weight w = 1 if |rho| <= huber_delta else huber_delta / |rho|.
 *             H = sum w J^T J (products (w J_a) J_b), g = sum w J^T rho ((w J_a) rho), e = sum rho^2 (unweighted), counts of
 *             inliers and of candidates.
 *   solve     as hv_tsdf_track: H xi = -g by Cholesky; DEGENERATE below HV_REGISTER_MIN_INLIERS inliers or at a pivot <=
 *             HV_REGISTER_PIVOT_REL trace(H): A stays and the call ends with success = 0.  Otherwise A := exp(xi) A with exp(xi) =
 *             [Rodrigues(omega), t]; the call ends when |omega| + |t| < HV_REGISTER_CONVERGED or after max_iterations
 *             linearisations (1 .. 10000).
 *   result    T_dst_src = Tr(c) A Tr(-c) T_init, evaluated as [R_A, (c + t_A) - R_A c] T_init (T_init itself, bit for bit, when A
 *             never moved): pass it to hv_tsdf_integrate_volume.  Of the LAST linearisation: fitness = inliers / candidates,
 *             inlier_rmse = sqrt(e / inliers) (0 if none), information = H (6x6, row-major, order (omega, t), motions about
 *             anchor = c, which is returned: an edge of a submap pose graph).  success = the last step was not degenerate and had
 *             >= HV_REGISTER_MIN_INLIERS inliers.  An empty src, an empty dst, no candidate or no overlap is not an error:
 *             success = 0, T_dst_src = T_init.
 * trace (may be NULL): one row of HV_REGISTER_TRACE_STRIDE doubles per linearisation run: {iteration, status (0 stepped, 1
 * converged, 2 degenerate), inliers, candidates, e, A [16] (the state it linearised at), H [21] (upper triangle, row by row), g [6],
 * xi [6]}; *trace_rows = rows written (at most trace_cap).
 * No float atomics, a fixed reduction order (hv_tsdf_track's): two calls on the same two volumes are bitwise equal.  Both batch
 * pipelines are drained and src's pending work is waited for, as hv_tsdf_integrate_volume does; the host reads the candidate count,
 * then every iteration is queued at once on dst's stream - a step of a finished call returns on a device flag - and the host waits
 * once for the result.  Device work: one workgroup per source unit counts, a scan, one workgroup per unit writes the 16-byte
 * candidates {index, tsdf_s} in their fixed order (ballot prefix, no atomic append); per iteration one thread per candidate
 * linearises (the iterations read the near-surface band only, not every allocated voxel) and one workgroup solves.  Extra device
 * memory, freed before the call returns: 16 bytes per candidate, 8 bytes per source unit, 240 KiB of reduction slab, 432 bytes per
 * iteration of trace and under 1 KiB of state.  Nothing of either volume is written, stamped, grown or claimed: dumps stay bit
 * for bit, extraction caches stay valid.
 * HV_ERR_MODE / HV_ERR_INVALID for the volumes and T_init exactly as hv_tsdf_integrate_volume (mode, sharding, dst == src, differing
 * voxel_length / sdf_trunc / unit resolution / device, a T_init that is not finite, rigid or has a bad bottom row); HV_ERR_INVALID
 * for max_iterations outside 1 .. 10000, a weight_threshold that is negative or not finite, tsdf_band outside (0, 1],
 * residual_trunc or huber_delta not positive and finite; HV_ERR_CAPACITY when src's pool overflowed in an earlier call. */
#define HV_REGISTER_MIN_INLIERS 6
#define HV_REGISTER_PIVOT_REL 1e-10
#define HV_REGISTER_CONVERGED 1e-6
#define HV_REGISTER_TRACE_STRIDE 54
typedef struct hv_register_params {
    double weight_threshold; /* a voxel counts when its weight is > this (source candidates and destination samples) */
    double tsdf_band;        /* candidates have |tsdf| <= this, in (0, 1] */
    double residual_trunc;   /* metres; customary 0.5 sdf_trunc */
    double huber_delta;      /* metres; customary 0.25 sdf_trunc */
    int32_t max_iterations;
    int32_t reserved;
} hv_register_params;
typedef struct hv_register_result {
    double T_dst_src[16];
    double information[36];
    double anchor[3]; /* c: the point of the destination frame the motions (omega, t) of `information` turn about */
    double fitness, inlier_rmse;
    int64_t inliers, candidates;
    int32_t iterations;
    int32_t success;
} hv_register_result;
int hv_tsdf_register_volume(hv_volume *dst, hv_volume *src, const double *T_init /* [16] */, const hv_register_params *params,
                            hv_register_result *result, double *trace, int64_t trace_cap, int64_t *trace_rows);

/* Point queries: what does the map hold at given points - signed distance, its gradient, colour and observation count - for
 * collision and clearance checks, for external optimisers, and as the core of hv_tsdf_check_frame below.  This project's own
 * contract, not Open3D-pinned.  The volume is only read.  points [n,3] of point_dtype (HV_F32 | HV_F64: the values
 * hv_integrate_points_semantic's point_dtype takes; float32 points are widened first) at loc.  For every point p all geometry is
 * float64, one IEEE operation per step in the order written, no contraction:
 *   locate    as hv_tsdf_integrate_volume locates a point in the source lattice: g_a = p_a / voxel_length - 0.5, g0_a = floor(g_a),
 *             r_a = g_a - g0_a.  The eight voxels are g0 + {0,1}^3 in hv_tsdf_at's corner order ((0,0,0) (1,0,0) (1,1,0) (0,1,0)
 *             (0,0,1) (1,0,1) (1,1,1) (0,1,1)); the NEAREST is g0_a + (r_a >= 0.5 ? 1 : 0) per axis; the unit of a voxel is its
 *             index >> 4.  A voxel is OBSERVED when its unit is held, its key is in range and (double)weight > weight_threshold.
 *   status    HV_SAMPLE_OUTSIDE     the point is not finite, some |g_a| >= 1e9, or the nearest voxel's unit is not held (or its key is
 *                                   out of range)
 *             HV_SAMPLE_UNOBSERVED  the nearest voxel's unit is held, the nearest voxel is not observed
 *             HV_SAMPLE_NEAREST     the nearest voxel is observed, not all eight are
 *             HV_SAMPLE_TRILINEAR   all eight are observed
 *   value     TRILINEAR: with u_a = 1 - r_a and the eight float32 tsdf values f0..f7 widened,
 *               c00 = u2 f0 + r2 f4,  c01 = u2 f3 + r2 f7,  c10 = u2 f1 + r2 f5,  c11 = u2 f2 + r2 f6,
 *               b0 = u1 c00 + r1 c01,  b1 = u1 c10 + r1 c11,  phi = u0 b0 + r0 b1     (the merge contract's trilinear expression)
 *               dphi/dr0 = b1 - b0
 *               dphi/dr1 = u0 (c01 - c00) + r0 (c11 - c10)
 *               dphi/dr2 = u0 (u1 (f4 - f0) + r1 (f7 - f3)) + r0 (u1 (f5 - f1) + r1 (f6 - f2))   (the registration contract's derivative)
 *             sdf = (float)(sdf_trunc * phi), metres; gradient_a = (float)((sdf_trunc / voxel_length) * dphi/dr_a), metres per metre,
 *             not normalised; color_c = (float)(tri(mean_c) / 255.0), tri = the expression of phi on the eight mean colours
 *             mean = (double)sum / (double)weight.
 *             NEAREST: sdf = (float)(sdf_trunc * (double)tsdf) of the nearest voxel, gradient 0, color_c = (float)(mean_c / 255.0) of
 *             the nearest voxel.  In both cases weight = (float) the nearest voxel's weight.
 *             OUTSIDE and UNOBSERVED: every output 0.
 * Outputs: sdf [n], gradient [n,3], color [n,3], weight [n] f32, status [n] u8; any may be NULL, and a NULL output is not computed - a
 * call that asks for neither colour nor gradient reads the weight and tsdf planes only.  loc = HV_DEVICE: device pointers, the call is
 * queued on the volume's stream and returns without waiting; HV_HOST: staged by the library and copied back before returning, as
 * hv_tsdf_ray_cast.  Reads only: no growth, no stamp, no claim - dumps stay bit for bit, extraction caches stay valid; the batch
 * pipeline is drained first, as hv_tsdf_ray_cast does.  Every point is written by one lane from values only that lane computes: two
 * calls give bitwise equal outputs, whatever the pool order.
 * HV_ERR_MODE for a volume that is not TSDF or is tile- or owner-sharded; HV_ERR_INVALID for n < 0 (or n > 2^36), NULL points with
 * n > 0, a bad dtype, a weight_threshold that is negative or not finite.  n == 0 is a no-op. */
typedef enum hv_point_dtype { HV_F32 = 0, HV_F64 = 1 } hv_point_dtype;
#define HV_SAMPLE_OUTSIDE 0
#define HV_SAMPLE_UNOBSERVED 1
#define HV_SAMPLE_NEAREST 2
#define HV_SAMPLE_TRILINEAR 3
int hv_tsdf_sample_points(hv_volume *v, const void *points /* [n,3] */, int32_t point_dtype, int64_t n, double weight_threshold,
                          float *sdf /* [n] */, float *gradient /* [n,3] */, float *color /* [n,3] */, float *weight /* [n] */,
                          uint8_t *status /* [n] */, int32_t loc);

/* Does a depth frame agree with the map?  Every pixel's back-projected point is sampled as above and classified: a point that floats
 * where the map has SEEN free space belongs to something that was not there before (zero such pixels - depth 0 is invalid everywhere
 * in this library - before hv_tsdf_integrate or hv_tsdf_track), and the five counts say whether keyframes still agree with a
 * corrected or merged map.  This project's own contract.  The volume is only read.
 *   depth     hv_tsdf_track's level 0: d = depth / (float)depth_scale in float32 (both dtypes); valid iff finite and
 *             depth_min < d <= depth_max, compared in double.
 *   point     float64 for integer u, v:  a = ((double)u - cx) / fx;  x = a * d;  b = ((double)v - cy) / fy;  y = b * d;  z = d;
 *             P_r = ((Rwc_r0 x + Rwc_r1 y) + Rwc_r2 z) + twc_r with Rwc = R_cw^T, twc_r = -((Rwc_r0 t_0 + Rwc_r1 t_1) + Rwc_r2 t_2)
 *             (t = T_cw's last column), computed on the host.  P is sampled by hv_tsdf_sample_points' rule with params->weight_threshold.
 *   class     HV_CHECK_INVALID     no valid depth
 *             HV_CHECK_UNKNOWN     sample status OUTSIDE or UNOBSERVED: the map knows nothing here
 *             HV_CHECK_CONSISTENT  |sdf| <= tolerance
 *             HV_CHECK_IN_FRONT    sdf > tolerance: the point floats in space the map saw as free
 *             HV_CHECK_BEHIND      sdf < -tolerance: the point lies behind the map's surface
 *             decided on the float32 sdf of the sample, widened and compared with tolerance in double.  sdf is 0 where the class is
 *             INVALID or UNKNOWN.
 *   stats     count[c] = pixels of class c, exact (integer atomics, at most one per wave and class).
 * Outputs: sdf [H,W] f32, cls [H,W] u8, stats; any may be NULL.  depth and the two arrays live at loc; HV_HOST is staged and copied
 * back.  With stats != NULL the call waits for the GPU; with stats == NULL and loc = HV_DEVICE it is queued on the volume's stream
 * and returns without waiting.  Reads only, as hv_tsdf_sample_points.  One lane per pixel, a wave per 8 x 8 pixel tile.
 * HV_ERR_MODE as hv_tsdf_sample_points; HV_ERR_INVALID for sizes, intrinsics, depth_scale and the depth range as hv_tsdf_track, a
 * tolerance that is not positive and finite, a weight_threshold that is negative or not finite, a T_cw that is not finite, has a
 * bottom row other than (0, 0, 0, 1) or is not rigid by hv_tsdf_integrate_volume's rule (T_cw is inverted as a rigid transform).  An
 * empty map is not an error: every valid pixel is UNKNOWN. */
#define HV_CHECK_INVALID 0
#define HV_CHECK_UNKNOWN 1
#define HV_CHECK_CONSISTENT 2
#define HV_CHECK_IN_FRONT 3
#define HV_CHECK_BEHIND 4
typedef struct hv_check_params {
    double depth_scale, depth_min, depth_max, weight_threshold, tolerance;
} hv_check_params;
typedef struct hv_check_stats {
    int64_t count[5]; /* pixels per class, indexed by HV_CHECK_* */
} hv_check_stats;
int hv_tsdf_check_frame(hv_volume *v, const void *depth, int32_t depth_dtype, int32_t height, int32_t width, const double *intr,
                        const double *T_cw, const hv_check_params *params, float *sdf /* [H,W] or NULL */,
                        uint8_t *cls /* [H,W] or NULL */, hv_check_stats *stats /* or NULL */, int32_t loc);

/* Point lookup on the block grids: what does the grid hold at given points - the grids' counterpart of hv_tsdf_sample_points, and the
 * bridge from the TSDF map's surfaces (mesh vertices, ray-cast vertex images, point clouds) to the semantic grids' labels.  This
 * project's own contract.  Modes: HV_MODE_VOXEL_GRID and the four semantic grids.  The volume is only read.  points [n,3] of point_dtype
 * (HV_F32 | HV_F64) at loc.  For every point p:
 *   own voxel  the voxel hv_integrate_points / hv_integrate_points_f64 / hv_integrate_points_semantic would put p in, by the very
 *              functions those calls key their points with: a float32 point is keyed in float32 (floorf(p_a * inv) with inv =
 *              1.0f / (float)voxel_size), a float64 point in float64 (floor(p_a * (double)inv)), so a point that was integrated finds
 *              the voxel it went to.  p has NO voxel - status HV_LOOKUP_INVALID - when a coordinate is not finite, when some
 *              |p_a * inv| >= 1e9 (evaluated as the mode's integrate does), or when the voxel's block key leaves [-2^20, 2^20).
 *   qualifies  a voxel qualifies when its block is held by this volume, its count >= max(min_count, 1) and - semantic modes only -
 *              confidence >= min_confidence, the predicate of hv_get_voxels_semantic through the same accessors (a NaN confidence or a
 *              NaN min_confidence never passes; min_confidence <= 0 passes every other voxel).  On the plain grid min_confidence is
 *              ignored.  A voxel is found by a lookup exactly when hv_get_voxels / hv_get_voxels_semantic (min_count, min_confidence)
 *              lists it.
 *   choice     the own voxel, if it qualifies: HV_LOOKUP_OWN.  Otherwise, with r = radius in {0, 1, 2}, the candidates are the voxels
 *              at the integer offsets (dx, dy, dz) in [-r, r]^3 from the own voxel's coordinate; a candidate's block is floor_div(
 *              coordinate, block_size) per axis, and a candidate whose block key leaves the key range is skipped.  Among the
 *              qualifying candidates the answer is the one whose MEAN POSITION m - the row hv_get_voxels* lists: the float64
 *              position_sum / (double)count of a semantic voxel, the float32 position_sum / (float)count of a plain one, widened - is
 *              nearest p, with p widened to float64 exactly and d2 = ((m0 - p0)^2 + (m1 - p1)^2) + (m2 - p2)^2 in float64, one IEEE
 *              operation per step in that order, no contraction; equal d2: the smallest offset index (dz + r)(2r + 1)^2 +
 *              (dy + r)(2r + 1) + (dx + r).  HV_LOOKUP_NEAR.  No qualifying candidate (always so for r = 0): HV_LOOKUP_MISSING.
 *   outputs    for a found voxel: count; position = m; color = color_sum / (float)count, class_id, object_id, confidence as
 *              hv_get_voxels / hv_get_voxels_semantic write them.  MISSING and INVALID: count 0, position and colour 0, ids -1,
 *              confidence 0.
 *   stats      points = n and the number of points per status, exact (integer atomics, at most one per wave and status).
 * Outputs: status [n] u8, count [n] i32, position [n,3] f64, color [n,3] f32, class_id [n] i32, object_id [n] i32, confidence [n] f32,
 * stats; any may be NULL, and a NULL output is not computed.  On HV_MODE_VOXEL_GRID class_id, object_id and confidence must be NULL.
 * points and the arrays live at loc; HV_HOST is staged by the library and copied back before returning.  With stats != NULL the call
 * waits for the GPU; with stats == NULL and loc = HV_DEVICE nothing is read back: the call is queued on the volume's stream, behind
 * every integrate call made before it, and returns without waiting.  Reads only: no claim, no growth, no counter - dumps before and
 * after are bitwise equal; it writes only the input staging and its output buffers, so caches, the touched lists, the point bins and
 * the association state stay as they are.  One point's outputs are written by lanes that computed them from that point alone, no atomics on outputs: two calls on
 * equal inputs give bitwise equal outputs, whatever the pool order.  On an owner-sharded grid (hv_set_owner) the lookup sees the blocks
 * this rank holds and everything else is MISSING; there is no collective inside the call.
 * Device work (hv_lookup.hip): one lane per point for the own voxel - one table probe, one record read; radius 0 is only that.  For
 * radius >= 1 the wave then takes the points still open one by one: the blocks of the neighbourhood are probed once, a lane per
 * candidate tests the occupancy bit and the count before anything else of the record, a wave min over (d2, offset index) picks the
 * winner and only its record is read for the outputs.
 * HV_ERR_MODE for a TSDF volume; HV_ERR_INVALID for a radius outside 0..2, n < 0 (or n > 2^36), NULL points with n > 0, a bad dtype or
 * loc, a label output on the plain grid.  n == 0 is a successful no-op (stats all 0). */
#define HV_LOOKUP_MISSING 0
#define HV_LOOKUP_OWN 1
#define HV_LOOKUP_NEAR 2
#define HV_LOOKUP_INVALID 3
typedef struct hv_lookup_params {
    int32_t min_count;
    float min_confidence;
    int32_t radius;
} hv_lookup_params;
typedef struct hv_lookup_stats {
    int64_t points, own, near, missing, invalid;
} hv_lookup_stats;
int hv_lookup_points(hv_volume *v, const void *points /* [n,3] */, int32_t point_dtype /* HV_F32 | HV_F64 */, int64_t n,
                     const hv_lookup_params *p, uint8_t *status /* [n] */, int32_t *count /* [n] */, double *position /* [n,3] */,
                     float *color /* [n,3] */, int32_t *class_id /* [n] */, int32_t *object_id /* [n] */, float *confidence /* [n] */,
                     hv_lookup_stats *stats /* may be NULL */, int32_t loc);

/* Distance field: how far is every cell of a box from the nearest surface of the map - beyond the truncation band, where the map
 * itself holds no value and, in open space, no unit.  A dense signed Euclidean distance over a box of the map's OWN voxel lattice, out
 * to a radius of R voxels, for planners, collision checks and camera-to-surface guards.  This project's own contract.  The volume is
 * only read.  Everything up to the final square root is integer arithmetic on squared voxel distances: there are no fragile points.
 *   cell      (i, j, k), 0 <= i < nx ..., is voxel q = origin + (i, j, k) of the map's lattice (centre (q + 0.5) * voxel_length); its
 *             unit is q >> 4 per axis (arithmetic shift: negative indices work), its local index q & 15.
 *   observed  hv_tsdf_sample_points' rule: the unit is held, its key is in range, (double)weight > weight_threshold.
 *   state     HV_DIST_INSIDE  observed and tsdf <= 0;  HV_DIST_FREE  observed and tsdf > 0 (a NaN tsdf is FREE);  HV_DIST_UNKNOWN
 *             otherwise.
 *   site      an observed voxel with at least one of its six axis neighbours IN THE MAP (inside the box or not) observed and of the
 *             other state (FREE against INSIDE): both voxels of every sign-changing lattice edge.  An UNKNOWN voxel is never a site
 *             and never makes one.  cls = state, with HV_DIST_SITE OR-ed on at a site.
 *   dist2     min(R * R, min over the sites s INSIDE THE BOX of |c - s|^2) in integer voxel units, evaluated as three separable
 *             passes with a window of +-R per axis, along x, then y, then z:
 *               g1(i, j, k) = min over |i' - i| <= R of (site(i', j, k) ? (i - i')^2 : INF)
 *               g2(i, j, k) = min over |j' - j| <= R of g1(i, j', k) + (j - j')^2
 *               g3(i, j, k) = min over |k' - k| <= R of g2(i, j, k') + (k - k')^2,     dist2 = min(g3, R * R)
 *             (a site within Euclidean distance R has every axis offset <= R, so the windows lose nothing below the cap).  A cell is
 *             FAR when dist2 == R * R: no site of the box lies nearer than R voxels.
 *   distance  s * (sqrtf((float)dist2) * (float)voxel_length): one correctly rounded float32 square root, then one float32 product;
 *             s = -1.0f for INSIDE cells (an inside site is -0.0f), +1.0f for FREE and UNKNOWN ones.  Metres.
 *   stats     unknown + free + inside = cells; sites = cells with the SITE bit; far = FAR cells.  Exact (integer atomics, at most one
 *             per wave and counter, after ballots).  They count the box of the call.
 * What the number means: `distance` is the distance to the nearest site CENTRE.  Every site centre lies within one voxel length of
 * a zero crossing on a lattice edge, so against the true surface it under-reports by at most one voxel length; for a planar surface
 * it over-reports by at most sqrt(3) voxel lengths.  A surface just outside the box is not seen: grow the box by R cells per side (the
 * Python front does, pad=True) where that matters.  Inside the truncation band hv_tsdf_sample_points remains the precise value.
 * Unknown space is not an obstacle here: cls tells known free from unknown, the caller decides.
 * Outputs: distance f32, dist2 u32, cls u8, each [nx,ny,nz] C-ordered (z fastest); any may be NULL, and a NULL output is neither
 * computed nor staged (a call for cls alone stops after the classification).  loc = HV_DEVICE: device pointers, queued on the
 * volume's stream; HV_HOST: staged by the library and copied back before returning, as hv_tsdf_sample_points.  With stats != NULL
 * the call waits for the GPU.  Reads only: no growth, no stamp, no claim - dumps stay bit for bit, extraction caches,
 * hv_tsdf_dirty_keys and hv_tsdf_touched are what they were; the batch pipeline is drained first, as hv_tsdf_ray_cast does.  Every
 * cell is written from values that depend on the map's content alone: two calls give bitwise equal outputs, whatever the pool order.
 * HV_ERR_MODE for a volume that is not TSDF or is tile- or owner-sharded; HV_ERR_INVALID for NULL params, a shape outside
 * 1..HV_DIST_MAX_SHAPE or with more than 2^31 - 1 cells, an |origin| above 2^30 (origin + shape stays inside int32), a radius outside
 * 1..HV_DIST_MAX_RADIUS, a weight_threshold that is negative or not finite, a bad loc.  An empty map is not an error: every cell is
 * UNKNOWN and FAR. */
#define HV_DIST_UNKNOWN 0
#define HV_DIST_FREE 1
#define HV_DIST_INSIDE 2
#define HV_DIST_SITE 4 /* OR-ed onto FREE or INSIDE */
#define HV_DIST_MAX_SHAPE 4096
#define HV_DIST_MAX_RADIUS 1024
typedef struct hv_distance_params {
    int32_t origin[3];        /* voxel index of cell (0,0,0); voxel q has its centre at (q + 0.5) * voxel_length */
    int32_t shape[3];         /* nx, ny, nz cells, each 1..4096; nx*ny*nz <= 2^31 - 1 */
    int32_t radius;           /* R, in voxels, 1..1024 */
    double weight_threshold;  /* >= 0, finite */
} hv_distance_params;
typedef struct hv_distance_stats {
    int64_t unknown, free, inside, sites, far;
} hv_distance_stats;
int hv_tsdf_distance_field(hv_volume *v, const hv_distance_params *p, float *distance /* [nx,ny,nz] */, uint32_t *dist2 /* [nx,ny,nz] */,
                           uint8_t *cls /* [nx,ny,nz] */, hv_distance_stats *stats, int32_t loc);

/* Surface components: the connected pieces of the map's surface, found in the sparse unit hash itself, and the removal of the small
 * ones in place - the floaters that noisy depth, depth edges and moving objects leave in every real map, which show up in
 * hv_tsdf_extract_mesh, become obstacles in hv_tsdf_distance_field and pull on hv_tsdf_register_volume.  This project's own
 * contract (Open3D clusters the triangles of an extracted, welded mesh on the host and leaves the map dirty).  Every definition is
 * integer: the whole contract is bit-exact, there is no fragile point.
 *   observed, state, site   exactly hv_tsdf_distance_field's rules: a voxel is OBSERVED when its unit is held, its key is in range
 *             and (double)weight > weight_threshold; its state is INSIDE when tsdf <= 0, else FREE (a NaN tsdf is FREE); a SITE is an
 *             observed voxel with at least one of its six axis neighbours observed and of the other state.
 *   adjacent  two sites whose global voxel indices (16 * key + local) differ by at most 1 on every axis: the 26-neighbourhood, across
 *             unit borders, edges and corners.  Both ends of every sign-changing lattice edge are sites and adjacent; a one-voxel-
 *             thick oblique sheet stays one piece (under the 6-neighbourhood it may not).
 *   component a class of the transitive closure of "adjacent".  Its SEED is its smallest site in lexicographic (x, y, z) order of the
 *             global voxel index; components are numbered 0 .. C-1 by increasing seed.  The numbering depends on the map's content
 *             alone - not on pool order, table order or launch order.
 * hv_tsdf_surface_components (reads only).  Per component, in its number's order: seed [C,3] i32, sites [C] i64 (how many), lo and
 * hi [C,3] i32 (the inclusive bounding box in global voxel indices).  The site list: site_index [N,3] i32 (global voxel index) and
 * site_label [N] i32 (component number), rows sorted by unit key (x, y, z), then by dump order x * 256 + y * 16 + z inside the unit.
 * Count-then-fill, as hv_tsdf_extract_mesh: *n_components = C and *n_sites = N are always written; every buffer may be NULL and a
 * NULL buffer is neither computed nor staged (with no table and no label the seeds are not computed nor sorted); a call with all
 * six NULL returns the counts.  A table buffer needs component_cap >= C, a list buffer site_cap >= N.  Buffers live at loc: HV_DEVICE
 * = device pointers, HV_HOST = staged by the library and copied back.  stats (may be NULL): units = units held, sites = N,
 * components = C, largest = the most sites in one component.  The call waits for the GPU.  Nothing of the volume changes: dumps stay
 * bit for bit, extraction caches, hv_tsdf_dirty_keys and hv_tsdf_touched are what they were; the batch pipeline is drained first.
 * An empty map or a map without a site is not an error: C = N = 0.  The two calls of a count-then-fill pair each label the map.
 * hv_tsdf_remove_components (rewrites the map).  With SMALL = the sites of components that have fewer than min_sites sites and KEPT =
 * all other sites, a voxel v of a held unit with weight > 0 (as an integer: any observation, whatever weight_threshold) is RESET when
 *   v is in SMALL, or some site of SMALL lies within Chebyshev distance `margin` of v and no site of KEPT does.
 * Reset = the fresh state in all five planes: what a never-written voxel holds and what hv_tsdf_deintegrate leaves behind.
 *   why this is safe   A voxel that is not a site has no observed axis neighbour of the other state, so making voxels unobserved
 *             never creates a sign-changing edge: no new site, no new surface.  Every cube that marching cubes triangulates for a
 *             kept component has a sign change, hence a KEPT site, among its corners, so all its corners lie within Chebyshev
 *             distance 1 of a KEPT site: with margin >= 1 the kept mesh is untouched (margin 0 resets SMALL sites only - and with them
 *             the triangles of kept cubes that have a SMALL corner).  After the call no SMALL site is observed any more and every KEPT
 *             site still is a site (its other-state neighbour is a site of its own component, so KEPT, so not reset): a second
 *             identical call finds exactly the KEPT components, none of them small, and resets nothing - the call is idempotent.
 *   after     units in which a voxel changed get a new stamp, as after hv_tsdf_deintegrate: incremental extraction and
 *             hv_tsdf_dirty_keys see them, cached extraction results are dropped; other units keep their stamp.  No unit is released
 *             (hv_tsdf_prune does that; units_emptied says how many now hold no weight).  If NOTHING is reset the volume is left
 *             exactly as it was, caches included.
 *   stats     components, sites = as hv_tsdf_surface_components before the call; components_removed, sites_removed = those of SMALL;
 *             voxels_reset; units_changed; units_emptied = changed units left without a weight.
 * Device work (hv_components.hip): one workgroup per unit classifies as hv_tsdf_distance_field does and writes the unit's 4096-bit
 * site mask; the host ranks the unit keys (hv_tsdf_dump's sort; 12 bytes per unit cross PCIe) and a scan gives every site its index in
 * the site list's order; union-find with atomicMin towards the smaller index, inside a unit in LDS, across units through the 26
 * neighbour units' masks - every link loop strictly lowers an index, no wave waits for another, nothing loops over rounds; a flatten
 * pass; sizes, boxes and seeds by integer atomics (one per wave where a wave's rows share a component); the canonical order by three
 * stable device radix sorts of the C seeds; the removal's two box dilations as shifts and ORs of 16-bit rows of the 3 x 3 x 3 units'
 * masks in LDS, the reset as 16-byte stores.  The site list never visits the host (HV_HOST copies the finished rows).  Extra device
 * memory, freed before the call returns, never a word per pool voxel: 1036 bytes per unit (site mask 512, row prefix 512, count,
 * base, rank) - 1552 for the removal (+ the SMALL mask and its count) -, 8 bytes per site (parent, component slot), 36 bytes per
 * component plus, where the table or the labels are asked for, 20 bytes per component and the radix sort's own scratch, 64 bytes of
 * counters, and with HV_HOST the outputs.
 * HV_ERR_MODE for a volume that is not TSDF or is tile- or owner-sharded (components cross ranks); HV_ERR_INVALID for a
 * weight_threshold that is negative or not finite, a bad loc, a capacity that is too small (the counts are still written), more than
 * 2^31 - 1 sites, min_sites < 1, a margin outside 0..HV_COMPONENTS_MAX_MARGIN (one unit: only the 26 neighbour units reach in). */
#define HV_COMPONENTS_MAX_MARGIN 16
typedef struct hv_components_stats {
    int64_t units, sites, components, largest;
} hv_components_stats;
typedef struct hv_remove_components_stats {
    int64_t components, components_removed, sites, sites_removed, voxels_reset, units_changed, units_emptied;
} hv_remove_components_stats;
int hv_tsdf_surface_components(hv_volume *v, double weight_threshold, int32_t *seed /* [C,3] */, int64_t *sites /* [C] */,
                               int32_t *lo /* [C,3] */, int32_t *hi /* [C,3] */, int64_t component_cap, int32_t *site_index /* [N,3] */,
                               int32_t *site_label /* [N] */, int64_t site_cap, int64_t *n_components, int64_t *n_sites,
                               hv_components_stats *stats, int32_t loc);
int hv_tsdf_remove_components(hv_volume *v, double weight_threshold, int64_t min_sites, int32_t margin, hv_remove_components_stats *stats);

/* Parity/debug export, units sorted by (x,y,z) index: keys [U,3] i32; tsdf, weight [U,R^3] f32;
 * color [U,R^3,3] f64 = running-mean RGB on the 0..255 scale; voxel order = Open3D's IndexOf
 * x*R^2 + y*R + z.  Host pointers; any may be NULL. */
int hv_tsdf_dump(hv_volume *v, int32_t *keys, float *tsdf, float *weight, double *color,
                 int64_t *n_units);
/* Unit indices touched by the most recent hv_tsdf_integrate, sorted; keys may be NULL. */
int hv_tsdf_touched(hv_volume *v, int32_t *keys, int64_t cap, int64_t *n);

/* Multi-GPU merge support: export/import additive numerators of the listed units.
 * keys [K,3] i32 host; payload [K, R^3, 5] f32 = {sum_tsdf_w, weight, sum_r, sum_g, sum_b}; units
 * absent from the volume export zeros; import REPLACES the unit's state from merged numerators
 * (allocating the unit if needed).  payload lives at `loc`. */
int hv_tsdf_export_numerators(hv_volume *v, const int32_t *keys, int64_t k, float *payload, int32_t loc);
int hv_tsdf_import_numerators(hv_volume *v, const int32_t *keys, int64_t k, const float *payload, int32_t loc);
/* All allocated unit keys (unsorted) for the key all-gather; keys may be NULL. */
int hv_tsdf_unit_keys(hv_volume *v, int32_t *keys, int64_t cap, int64_t *n);

/* Packed maps: a compact, BIT-EXACT form of a TSDF map, made and consumed on the GPU - for keeping a map across sessions, handing it
 * to another process or GPU, checkpointing it before a correction.  This project's own format; this comment is its contract.
 * One flat little-endian byte buffer.  Every section starts on a 64-byte boundary, padding bytes are zero, and the buffer ends on
 * one: total_bytes = the end of the last section rounded up to 64.
 *   header, 128 bytes
 *     off  type        field
 *       0  8 bytes     magic "HVTSDFPK"
 *       8  uint32      version = HV_PACK_VERSION (1)
 *      12  uint32      header_bytes = 128
 *      16  float64     voxel_length
 *      24  float64     sdf_trunc
 *      32  int32       resolution = 16
 *      36  int32       reserved = 0
 *      40  int64       units  U
 *      48  int64       voxels N (stored voxel records)
 *      56  int64       total_bytes
 *      64  8 x uint64  byte offsets of the eight sections below, in this order
 *   keys     int32  [U,3]    unit indices, strictly ascending by (x, then y, then z) - the order of hv_tsdf_dump: the same map gives
 *                            the same bytes whatever its pool order
 *   offsets  uint64 [U+1]    offsets[0] = 0, offsets[U] = N; unit u's records are [offsets[u], offsets[u+1])
 *   masks    uint32 [U,128]  bit (k & 31) of word (k >> 5) is set when voxel word k of the unit is STORED; k = z * 256 + x * 16 + y,
 *                            the library's voxel word (the order hv_tsdf_export_numerators exposes)
 *   tsdf     float32 [N]     records, unit after unit, within a unit by ascending k
 *   weight   uint32 [N]      same order
 *   sum_r, sum_g, sum_b  uint32 [N] each, same order
 * A voxel is STORED when any of its five 32-bit words is non-zero as a bit pattern (a tsdf of -0.0 counts, and so does a voxel of
 * weight 0 that still carries a colour sum): the round trip is bit-exact without relying on "weight 0 implies the fresh state".
 * EVERY allocated unit is stored, all-zero ones included (count 0, mask 0): hv_num_blocks and hv_tsdf_unit_keys survive the trip
 * (hv_tsdf_prune first drops empty units).  NOT stored, NOT restored: rectify maps, colour order, tile and owner settings, pool
 * size - settings of a volume, not content of a map.
 *   hv_tsdf_packed_check  host only, no GPU.  Checks, in this order, and names the first rule that fails (HV_ERR_INVALID): at least
 *              128 bytes; magic; version; header_bytes; resolution == 16; units, voxels >= 0 and no more than the buffer could hold;
 *              total_bytes == bytes; every section offset 64-byte aligned; every section behind the header and inside the buffer
 *              with the size U and N imply; no two sections overlap; keys in the library's range [-2^20, 2^20) and strictly
 *              ascending; offsets[0] == 0, offsets non-decreasing, offsets[U] == N; offsets[u+1] - offsets[u] == popcount(masks[u]).
 *              Fills *out (may be NULL) with the header fields once the header rules hold.
 *   hv_tsdf_pack_size     waits; info = {U, N, exact buffer size}.
 *   hv_tsdf_pack          dst (cap bytes) at loc = HV_HOST or HV_DEVICE (the volume's GPU).  cap too small: HV_ERR_CAPACITY, info
 *              filled in, nothing written.  Only READS the volume: dumps, extraction caches, hv_tsdf_dirty_keys and hv_tsdf_touched
 *              are what they were.  An empty volume packs to a valid buffer with U = N = 0.  Device work: one workgroup per unit
 *              reads the five planes in word order and writes the unit's 128 mask words (a wave's ballot = two of them) and its
 *              count; a scan of the counts; one workgroup per unit ranks each stored voxel by the popcount of the mask bits below it
 *              and writes the five record streams.  The key order is a host sort of the unit keys, as hv_tsdf_dump's.
 *   hv_tsdf_unpack        src (bytes) at loc.  Runs hv_tsdf_packed_check BEFORE it launches anything - on a host buffer itself; of a
 *              device buffer it copies the header, then the keys / offsets / masks sections (about 532 bytes per unit, never the
 *              records) to the host - so nothing a caller passes reaches a kernel unvalidated and the kernels cannot index outside
 *              the buffer.  Requires a TSDF volume with hv_num_blocks == 0 whose voxel_length and sdf_trunc are BITWISE equal to the
 *              header's (merging a packed map into a non-empty volume is hv_tsdf_integrate_volume's job, after unpacking into a
 *              fresh volume).  Then: the keys are claimed and the claims verified (a pool that is too small grows before anything is
 *              written, or the call fails with HV_ERR_CAPACITY); one workgroup per unit writes ALL 4096 voxels of all five planes,
 *              the record where the bit is set and zero where it is not; every unpacked unit is stamped with one new frame id
 *              (hv_tsdf_dirty_keys lists them, incremental extraction sees them; hv_tsdf_touched lists nothing); the content and
 *              extraction versions are bumped and the occupancy is published, as hv_tsdf_import_numerators does.
 *              On ANY error the volume is unchanged.
 * Both hv_tsdf_pack and hv_tsdf_unpack drain the batch pipeline and wait for the GPU; HV_ERR_MODE for a non-TSDF volume and for a
 * tile- or owner-sharded one (it holds partial sums, or a part of the map's units), as hv_tsdf_integrate_volume. */
#define HV_PACK_VERSION 1
#define HV_PACK_HEADER_BYTES 128
typedef struct hv_pack_info {
    int64_t units, voxels, bytes;
} hv_pack_info;
typedef struct hv_packed_header {
    double voxel_length, sdf_trunc;
    int32_t resolution, version;
    int64_t units, voxels, bytes;
} hv_packed_header;
int hv_tsdf_pack_size(hv_volume *v, hv_pack_info *info);
int hv_tsdf_pack(hv_volume *v, void *dst, int64_t cap, int32_t loc, hv_pack_info *info);
int hv_tsdf_unpack(hv_volume *v, const void *src, int64_t bytes, int32_t loc, hv_pack_info *info);
int hv_tsdf_packed_check(const void *host_src, int64_t bytes, hv_packed_header *out);

/* Packed grids: the same for HV_MODE_VOXEL_GRID and the four semantic block grids - a compact, BIT-EXACT form of the whole map (counts,
 * position and colour sums, object and class ids, both confidence counters, the per-voxel label maps in insertion order, the next
 * object id), made and consumed on the GPU.  This project's own format; this comment is its contract.
 * One flat little-endian byte buffer.  Every section starts on a 64-byte boundary, padding bytes are zero, and the buffer ends on
 * one: total_bytes = the end of the last section rounded up to 64.
 *   header, 192 bytes
 *     off  type        field
 *       0  8 bytes     magic "HVGRIDPK"
 *       8  uint32      version = HV_GRID_PACK_VERSION (1)
 *      12  uint32      header_bytes = 192
 *      16  float64     voxel_size
 *      24  int32       mode (the HV_MODE_* value: 0, 1, 2, 11 or 12)
 *      28  int32       block_size bs, 1..16
 *      32  int32       record_bytes: 32 (mode 0), 64 (modes 1, 11), 128 (modes 2, 12)
 *      36  int32       next_object_id: the process-wide counter (hv_peek_next_object_id) at pack time
 *      40  float32     depth_threshold  (hv_set_depth_threshold)
 *      44  float32     depth_decay_rate (hv_set_depth_decay_rate)
 *      48  int64       blocks B
 *      56  int64       voxels N (stored records)
 *      64  int64       extra_pairs P
 *      72  int64       total_bytes
 *      80  8 x uint64  byte offsets of the eight sections below, in this order
 *     144  48 bytes    reserved = 0
 *   keys        int32  [B,3]   block keys, strictly ascending by (x, then y, then z) - the order of hv_dump_blocks: the same map gives the
 *                              same bytes whatever its pool order
 *   offsets     uint64 [B+1]   offsets[0] = 0, offsets[B] = N; block b's records are [offsets[b], offsets[b+1])
 *   masks       uint64 [B,W]   W = ceil(bs^3 / 64); bit (k & 63) of word (k >> 6) is set when local voxel k = lx + ly * bs + lz * bs^2 is
 *                              STORED; bits at or above bs^3 are zero
 *   records     N x record_bytes   block after block, within a block by ascending k.  A record is the pool record bit for bit - HvVoxel,
 *                              HvSemVoxel, HvSem2Voxel, HvProbVoxel or HvProb2Voxel, as 32-bit words:
 *                                mode 0        0 count, 1-3 position sums f32, 4-6 colour sums f32, 7 padding
 *                                modes 1, 11   0 count, 1 object id + 1, 2 class id + 1, 3 (object) confidence counter, 4-9 position sums f64,
 *                                              10-12 colour sums f32, 13 class confidence counter (mode 11; padding in mode 1), 14-15 padding
 *                                modes 2, 12   0 count, 1 meta, 2-7 position sums f64, 8-10 colour sums f32, 11-16 the ids of the 6 inline
 *                                              label pairs, 17-22 their class ids (mode 12: which map, 0 object / 1 class), 23-28 their
 *                                              log-probabilities f32, 29 chain link, 30-31 padding
 *                              meta = n | (b1 << 8) | (b2 << 16): n = pairs of the label map (0..254), b1 = 1 + index of the cached most
 *                              likely pair (mode 12: object entry) or 0, b2 (mode 12 only) = 1 + index of the cached most likely class
 *                              entry or 0.  Padding words and the chain link are written as ZERO.
 *   extras      uint8  [N]     modes 2, 12 (size 0 otherwise): max(n - 6, 0) = the pairs of the voxel's map beyond the 6 inline ones, 0..248
 *   extra_obj, extra_cls  int32 [P] each   P = sum of extras: the extra pairs of every voxel in record order, within a voxel in insertion
 *                              order (pair 6, 7, ...)
 *   extra_logp  float32 [P]    same order
 * A voxel is STORED when any word of its record other than padding and the chain link is non-zero as a bit pattern.  A reset
 * probabilistic voxel that only kept its overflow chain is NOT stored (the chain is capacity, not content).  EVERY allocated block is
 * stored, also with mask 0 (hv_num_blocks survives the trip).  NOT stored, NOT restored: pool size, owner settings, streams, the
 * association's scratch (votes, the decided map), hv_dropped_points, hv_label_overflows, the segments cache.
 *   hv_grid_packed_check  host only, no GPU.  Checks, in this order, and names the first rule that fails (HV_ERR_INVALID): at least 192
 *              bytes; magic; version; header_bytes; mode one of the five; block_size in [1,16]; record_bytes matches the mode; blocks, voxels,
 *              extra_pairs >= 0; extra_pairs == 0 for a mode without label maps; blocks, voxels and extra_pairs no more than the buffer could
 *              hold (12, record_bytes and 12 bytes apiece); total_bytes == bytes; every section offset 64-byte aligned; every section behind
 *              the header and inside the buffer with the size B, N and P imply; no two sections overlap; keys in [-2^20, 2^20); keys
 *              strictly ascending; offsets[0] == 0; offsets non-decreasing; offsets[B] == N; offsets[b+1] - offsets[b] ==
 *              popcount(masks[b]); no mask bit at or above bs^3; every extras entry <= 248; sum of extras == P.
 *              Fills *out (may be NULL) with the header fields once the header rules hold, and its chain_nodes once every rule holds.
 *   hv_grid_pack_size     waits; info = {B, N, P, exact buffer size}.
 *   hv_grid_pack          dst (cap bytes) at loc = HV_HOST or HV_DEVICE (the volume's GPU).  cap too small: HV_ERR_CAPACITY, info filled
 *              in, nothing written.  Only READS the volume: the dumps, hv_lookup_points, the association state (an unfetched map included)
 *              are what they were.  An empty grid packs to a valid buffer with B = N = P = 0.
 *   hv_grid_unpack        src (bytes) at loc.  Runs hv_grid_packed_check BEFORE it launches anything - on a host buffer as it lies; of a
 *              device buffer it copies the header, then the keys / offsets / masks / extras sections to the host, never the records.
 *              Requires a grid of the header's mode and block_size whose voxel_size is BITWISE equal to the header's (HV_ERR_INVALID),
 *              hv_num_blocks == 0 (HV_ERR_INVALID) and no owner sharding (HV_ERR_MODE, as for a TSDF volume).  For modes 2 and 12 a
 *              read-only pass over the records (indices inside [0, N) only) then checks what the metadata cannot: n <= 254, extras ==
 *              max(n - 6, 0), b1 <= n and (mode 12) b2 <= n (HV_ERR_INVALID).  Then: the overflow-node pool must hold
 *              sum ceil(extras / 10) nodes (HV_ERR_CAPACITY, the need named); the keys are claimed and the claims verified (a pool that is
 *              too small grows before anything is written, or HV_ERR_CAPACITY); ALL bs^3 records of every block are written, the
 *              packed record where the bit is set and zero where it is not, and the block's occupancy bits = its mask; the chains are
 *              rebuilt (voxel i gets ceil(extras[i] / 10) consecutive nodes, filled in order, the unused slots of the last one zero).
 *              On ANY error the volume is unchanged.  Afterwards the node counter (hv_prob_nodes_used) = nodes rebuilt, no association is
 *              pending, the segments cache is dropped, the content version is bumped, and the process-wide next object id is
 *              max(its value, the header's) - never lowered.  depth_threshold and depth_decay_rate are settings: the volume keeps its own.
 * All of them drain pending work and wait for the GPU; HV_ERR_MODE for a TSDF volume and for an owner-sharded grid (hv_set_owner with
 * world_size > 1: it holds a part of the map's blocks). */
#define HV_GRID_PACK_VERSION 1
#define HV_GRID_PACK_HEADER_BYTES 192
typedef struct hv_grid_pack_info {
    int64_t blocks, voxels, extra_pairs, bytes;
} hv_grid_pack_info;
typedef struct hv_grid_packed_header {
    double voxel_size;
    int32_t mode, block_size, record_bytes, version, next_object_id;
    float depth_threshold, depth_decay_rate;
    int32_t reserved;
    int64_t blocks, voxels, extra_pairs, bytes;
    int64_t chain_nodes; /* sum of ceil(extras / 10): the overflow nodes hv_grid_unpack rebuilds */
} hv_grid_packed_header;
int hv_grid_pack_size(hv_volume *v, hv_grid_pack_info *info);
int hv_grid_pack(hv_volume *v, void *dst, int64_t cap, int32_t loc, hv_grid_pack_info *info);
int hv_grid_unpack(hv_volume *v, const void *src, int64_t bytes, int32_t loc, hv_grid_pack_info *info);
int hv_grid_packed_check(const void *host_src, int64_t bytes, hv_grid_packed_header *out);

/* ---- halo merge of image-tile-sharded volumes (SURVEY 8b `hv_merge_halo`, 8e; north-star "RCCL all-reduce of
 * overlapping-block TSDF/weight").  pySLAM has no multi-GPU path (no NCCL/MPI/torch.distributed call anywhere in the
 * reference): these are new.  With hv_tsdf_set_tile each GPU fuses the voxels that project into its image tile, so units
 * on tile borders (and revisits from other viewpoints) hold PARTIAL running means on several GPUs.  A merge:
 *   1. hv_tsdf_dirty_keys      every rank: the units it stamped since its last merge (sorted, 12 B per key)
 *   2. (caller) all-gather of the key lists
 *   3. hv_merge_halo_plan_held every rank, same input -> same output: the keys that some rank updated since its last merge
 *                              AND that two ranks or more hold (second all-gather: hv_tsdf_unit_keys), in sorted order, and
 *                              what THIS rank does with each: 1 = keeps it (the lowest holding rank), 2 = zeroes its copy (a
 *                              no-op where the rank has none).  A rank counts as a holder ONCE, however often its held list
 *                              names the key - on the host and in the device plan below (one rule: csrc/hv_halo_plan.h).
 *                              (hv_merge_halo_plan: the same from the dirty lists alone - keys listed by >= 2 ranks, lowest
 *                              listing rank keeps, EVERY other rank zeroes: a unit that is updated by one rank per window is
 *                              never consolidated by it.  It IS hv_merge_halo_plan_held(keys, counts, keys, counts): every
 *                              lister taken as a holder; a rank lists a key once, so the lowest lister is the lowest holder.)
 *   4. hv_merge_halo_pack      additive numerators {sum w*tsdf, w, sum r, sum g, sum b} of the shared units only, dense
 *                              [K, 16^3, 5] f32 in plan order (zeros where the rank does not hold a unit)
 *   5. (caller) all-reduce(sum) of that buffer - message size = shared units x 81 920 B, not the whole volume
 *   6. hv_merge_halo_unpack    keeper: state := reduced numerators; other holders: unit zeroed (they go on fusing deltas)
 *                              (hv_tsdf_import_numerators is the same write with every unit kept, after claiming the units)
 *   7. hv_tsdf_mark_merged
 * Afterwards the sum over ranks of every unit's numerators is still the single-GPU total, and every unit that went through
 * the merge is complete on exactly one rank (with the _held plan: every unit two ranks hold).  The library does the device work; the caller owns the transport (pyslam_amd/distributed.py:
 * torch.distributed, backend nccl = RCCL over xGMI). */
int hv_tsdf_dirty_keys(hv_volume *v, int32_t *keys /* [cap,3] host, may be NULL */, int64_t cap, int64_t *n);
int hv_tsdf_mark_merged(hv_volume *v);
/* Host-only.  gathered_keys = the ranks' lists back to back ([sum counts, 3]); shared_keys/action may be NULL to query *n_shared. */
int hv_merge_halo_plan(const int32_t *gathered_keys, const int64_t *counts, int32_t world_size, int32_t rank,
                       int32_t *shared_keys, uint8_t *action, int64_t cap, int64_t *n_shared);
int hv_merge_halo_plan_held(const int32_t *dirty_keys, const int64_t *dirty_counts, const int32_t *held_keys,
                            const int64_t *held_counts, int32_t world_size, int32_t rank, int32_t *shared_keys, uint8_t *action,
                            int64_t cap, int64_t *n_shared);
int hv_merge_halo_pack(hv_volume *v, const int32_t *shared_keys, int64_t k, float *payload, int32_t loc);
int hv_merge_halo_unpack(hv_volume *v, const int32_t *shared_keys, int64_t k, const float *payload, const uint8_t *action,
                         int32_t loc);
/* The same merge with the key lists and the plan staying in DEVICE memory (round 6: the transport is RCCL, which gathers device
 * buffers; rounds 3-5 took the lists through the host twice per merge).  Keys are packed 64-bit words (the library's block key) in
 * int64 device buffers of the caller (torch tensors):
 *   1. hv_merge_halo_lists_device   this rank's dirty list and held list into d_dirty_keys / d_held_keys (NULL buffers: *n_held = an
 *                                   upper bound of both lengths, to size them); the two lengths come back to the host (they size the
 *                                   all-gather)
 *   2. (caller) all-gather of the counts and of the padded lists -> [world][stride] device buffers
 *   3. hv_merge_halo_plan_device    radix sort of (key, rank, held) + two small kernels: the plan of hv_merge_halo_plan_held (the
 *                                   same rule on every run of equal keys), in packed-key order, left IN THE VOLUME; *n_shared comes back to the host (it sizes the payload).
 *                                   all_dirty_kept != 0: one rank takes every dirty unit through the path as its own keeper.
 *   4. hv_merge_halo_pack_planned / 6. _unpack_planned   units [first, first + count) of the stored plan, device payload, queued on the
 *                                   volume's stream (the caller orders its all-reduce against that stream)
 *   hv_merge_halo_plan_fetch        the stored plan as host arrays (inspection, tests). */
int hv_merge_halo_lists_device(hv_volume *v, int64_t *d_dirty_keys, int64_t dirty_cap, int64_t *d_held_keys, int64_t held_cap,
                               int64_t *n_dirty, int64_t *n_held);
int hv_merge_halo_plan_device(hv_volume *v, const int64_t *d_dirty_all, const int64_t *dirty_counts /* host [world] */, int64_t dirty_stride,
                              const int64_t *d_held_all, const int64_t *held_counts /* host [world] */, int64_t held_stride,
                              int32_t world_size, int32_t rank, int32_t all_dirty_kept, int64_t *n_shared);
int hv_merge_halo_plan_fetch(hv_volume *v, int32_t *shared_keys, uint8_t *action, int64_t cap, int64_t *n_shared);
int hv_merge_halo_pack_planned(hv_volume *v, int64_t first, int64_t count, float *d_payload);
int hv_merge_halo_unpack_planned(hv_volume *v, int64_t first, int64_t count, const float *d_payload);

/* ---- measurement hooks (bench.py) ---------------------------------------------------------------
 * When enabled, the dominant kernel of each integrate call is bracketed by HIP events on the
 * volume's stream; hv_profile_read synchronises and returns the summed device time. */
int hv_profile_enable(hv_volume *v, int32_t on);
int hv_profile_read(hv_volume *v, double *kernel_ms_total, int64_t *kernel_launches,
                    int64_t *units_processed);
/* The same measurement launch by launch: durations (ms) of the bracketed launches since hv_profile_enable / the last
 * read, in issue order, into launch_ms[0 .. min(*n, cap)); *n = launches recorded.  Does not reset (hv_profile_read does). */
int hv_profile_read_launches(hv_volume *v, float *launch_ms, int64_t cap, int64_t *n);

#ifdef __cplusplus
}
#endif
#endif /* PYSLAM_HIPVOL_H */
