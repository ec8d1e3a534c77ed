"""Host-side mirror of the two volume objects pySLAM's dense integrators drive.

* :class:`VoxelBlockGrid`, :class:`CameraFrustrum`, :class:`BoundingBox3D`, :class:`VoxelGridData`
  mirror the ``volumetric`` pybind11 module (reference: cpp/volumetric/volumetric_grid_module.h:
  732-935, camera_frustrum_module.h:41-130) — same method names, argument meaning, defaults and
  error messages — over the HIP library's VOXEL_GRID mode.
* :class:`ScalableTSDFVolume`, :class:`PinholeCameraIntrinsic`, :class:`TriangleMesh`,
  :class:`PointCloud` mirror the slice of ``open3d`` that pyslam/dense/volumetric_integrator_tsdf.py
  uses (:104-119, 215-223, 239-267) over the library's TSDF mode.

All compute happens in libpyslam_hipvol.so on the GPU; nothing here falls back to the CPU.
Arrays may be numpy (host) or torch CUDA tensors (zero-copy, already resident in HBM).
"""
import contextlib
import ctypes
import functools
import typing

import numpy as np

from . import _lib as L


def _result_array(shape, dtype):
    """Host array a large device result is copied into.  Page-locked when torch can provide it (hipHostMalloc behind torch's
    caching host allocator: the block is reused from one output tick to the next) - the D2H copy of a 270 MB mesh then runs
    as one DMA at PCIe speed instead of through the runtime's pageable staging; plain numpy otherwise or with
    PYSLAM_AMD_PINNED_RESULTS=0.  Either way the caller gets an ordinary writable numpy array."""
    import os

    n = int(np.prod(shape))
    if n * np.dtype(dtype).itemsize >= (1 << 20) and os.environ.get("PYSLAM_AMD_PINNED_RESULTS", "1") != "0":
        try:
            import torch

            if torch.cuda.is_available():
                return torch.empty(tuple(shape), dtype=getattr(torch, np.dtype(dtype).name), pin_memory=True).numpy()
        except Exception:  # no torch / no pinned memory left: the pageable copy is still correct
            pass
    return np.empty(shape, dtype)


def _is_torch(a):
    """A torch tensor, on either device (numpy arrays, lists and bytes-like objects are not)."""
    return hasattr(a, "data_ptr") and not isinstance(a, np.ndarray)


def _check_map_shapes(map_x, map_y, H, W):
    """hv_remap takes one height and width for image and maps: smaller maps would be read past their end."""
    for name, m in (("map_x", map_x), ("map_y", map_y)):
        if tuple(np.shape(m)) != (H, W):
            raise RuntimeError(f"remap: {name} has shape {tuple(np.shape(m))}, the image is {H}x{W} (maps are [H, W])")


def _stats(cls, struct):
    """A *Stats result (a _Stats subclass or a named tuple) from the ctypes struct the library filled, field by field name."""
    return cls(*[getattr(struct, name) for name in getattr(cls, "_fields", cls.__slots__)])


def _as_f64_4x4(T):
    T = np.ascontiguousarray(np.asarray(T, dtype=np.float64))
    if T.shape != (4, 4):
        raise RuntimeError("T_cw must be a 4x4 matrix")
    return T


_UNSUPPORTED_IMAGE = "[ScalableTSDFVolume::Integrate] Unsupported image format."


def _pose_rows(T, frames):
    """The poses of `frames` frames ([F,4,4], [F,16] or flat) as the library reads them: contiguous float64 [F,16]."""
    T = np.asarray(T, dtype=np.float64)
    if T.size != 16 * frames or (T.ndim > 1 and T.shape[0] != frames):
        raise RuntimeError(_UNSUPPORTED_IMAGE)
    return np.ascontiguousarray(T.reshape(frames, 16))


def _rigid_operand(source, T, who, what):
    """The operands of a volume-to-volume call: `source` must be a volume, T (None: identity) a 4x4 -> contiguous float64 [4,4]."""
    if getattr(source, "_h", None) is None:
        raise TypeError(f"{who}: source must be a volume")
    T = np.eye(4) if T is None else np.asarray(T, dtype=np.float64)
    if T.shape != (4, 4):
        raise ValueError(f"{who}: {what} must be a 4x4 matrix")
    return np.ascontiguousarray(T, dtype=np.float64)


def _points_operand(points, torch_ok=False):
    """points [N,3] of a grid's integrate -> (operand, wide, N): contiguous float64 when they are float64, else float32 (the
    binding's two overloads).  torch_ok: a torch tensor stays one (either device); else everything becomes a host array."""
    pts = points if torch_ok and _is_torch(points) else np.asarray(points)
    if len(pts.shape) != 2 or pts.shape[1] != 3:
        raise RuntimeError("points must be a contiguous Nx3 array")
    wide = str(pts.dtype) in ("float64", "torch.float64")
    if _is_torch(pts):
        pts = pts.contiguous() if wide else pts.contiguous().float()
    else:
        pts = np.ascontiguousarray(pts, dtype=np.float64 if wide else np.float32)
    return pts, wide, pts.shape[0]


def _colors_operand(colors, n, torch_ok=False):
    """colors [N,3] uint8 | float32 | None of a grid's integrate -> (contiguous operand, HV_COLOR_*); torch_ok as _points_operand."""
    if colors is None:
        return None, L.HV_COLOR_NONE
    cols = colors.contiguous() if torch_ok and _is_torch(colors) else np.ascontiguousarray(colors)
    if len(cols.shape) != 2 or cols.shape[1] != 3:
        raise RuntimeError("colors must be a contiguous Nx3 array")
    if cols.shape[0] != n:
        raise RuntimeError("points and colors must have the same size")
    kind = {"uint8": L.HV_COLOR_U8, "float32": L.HV_COLOR_F32}.get(str(cols.dtype).replace("torch.", ""))
    if kind is None:
        raise RuntimeError(f"Colors must be uint8 or float32, got dtype with {cols.dtype}")
    return cols, kind


def _tsdf_operands(depth, color, intrinsic, frames=None, depth_only=False):
    """The depth / colour operands of ScalableTSDFVolume.integrate* in the layout the library reads from a bare pointer, as
    Open3D's Image would hold them: depth uint16 as it is, any other real dtype as float32; colour uint8 [..., H, W, 3]; both
    contiguous.  numpy arrays and torch tensors on either device alike; a conversion runs on the operand's own device, and an
    operand that already has the layout is returned as it is (no copy).  frames=None: one [H, W] frame, else [frames, H, W].
    -> (depth, color, depth kind, converted) - converted: a new CUDA tensor was made (torch's stream produces it).
    Anything else - colour that is not uint8 of the depth's shape + (3,), an intrinsic of another size, depth and colour on
    different devices - raises before any library call.  depth_only=True: the depth operand alone, color is ignored (and
    returned as None)."""
    is_torch = _is_torch
    if not depth_only and is_torch(depth) != is_torch(color):
        # one host array and one torch tensor: only together when the tensor lives on the host
        if L.location(depth) != L.HV_HOST or L.location(color) != L.HV_HOST:
            raise RuntimeError(_UNSUPPORTED_IMAGE)
    converted = False
    if is_torch(depth):
        import torch

        if not depth_only and (L.location(depth) != L.location(color) or (depth.is_cuda and depth.device != color.device)):
            raise RuntimeError(_UNSUPPORTED_IMAGE)
        if depth.dtype == torch.bool or depth.dtype.is_complex:
            raise RuntimeError(_UNSUPPORTED_IMAGE)
        d = depth if depth.dtype == torch.uint16 else depth.to(torch.float32)
        d = d.contiguous()
        dkind = L.HV_DEPTH_U16 if d.dtype == torch.uint16 else L.HV_DEPTH_F32
        converted = d is not depth and d.is_cuda
    else:
        d = np.asarray(depth)
        if not (np.issubdtype(d.dtype, np.integer) or np.issubdtype(d.dtype, np.floating)):
            raise RuntimeError(_UNSUPPORTED_IMAGE)
        d = np.ascontiguousarray(d, dtype=np.uint16 if d.dtype == np.uint16 else np.float32)
        dkind = L.HV_DEPTH_U16 if d.dtype == np.uint16 else L.HV_DEPTH_F32
    if depth_only:
        c = None
    elif is_torch(color):
        import torch

        if color.dtype != torch.uint8:
            raise RuntimeError(_UNSUPPORTED_IMAGE)
        c = color.contiguous()
        converted = converted or (c is not color and c.is_cuda)
    else:
        c = np.asarray(color)
        if c.dtype != np.uint8:
            raise RuntimeError(_UNSUPPORTED_IMAGE)
        c = np.ascontiguousarray(c)
    shape = tuple(int(s) for s in d.shape)
    if len(shape) != (2 if frames is None else 3) or (frames is not None and shape[0] != frames):
        raise RuntimeError(_UNSUPPORTED_IMAGE)
    if not depth_only and tuple(int(s) for s in c.shape) != shape + (3,):
        raise RuntimeError(_UNSUPPORTED_IMAGE)
    if int(intrinsic.width) != shape[-1] or int(intrinsic.height) != shape[-2]:
        raise RuntimeError(_UNSUPPORTED_IMAGE)
    return d, c, dkind, converted


class PoseGraphResult:
    """What optimize_pose_graph returns (hv_pose_graph_result and the call's arrays): poses [N,4,4] float64 T_wc after the
    optimisation; line_process [E] float64, the final weight l_e of every edge (1 for a certain one); kept [E] bool = l_e >=
    edge_prune_threshold; chi2_initial / chi2_final, the objective at the first linearisation and at the final state; lambda_, the
    last damping; iterations (outer), cg_iterations_total, edges_kept; converged: the rule that stopped the call ("gradient",
    "step", "decrease", "residual" or "max_iterations"); success; trace = None, or one dict per outer iteration (iteration, lambda_,
    chi2, chi2_trial, gain_ratio, accepted, cg_iterations, cg_residual, step_norm, gradient_norm, lambda_new, converged, and poses
    [N,4,4] - the state the iteration started from)."""
    __slots__ = ("poses", "line_process", "kept", "chi2_initial", "chi2_final", "lambda_", "iterations", "cg_iterations_total", "edges_kept",
                 "converged", "success", "trace")

    def __init__(self, *values):
        for name, value in zip(self.__slots__, values):
            setattr(self, name, value)


_POSE_GRAPH_TRACE = (("iteration", int), ("lambda_", float), ("chi2", float), ("chi2_trial", float), ("gain_ratio", float), ("accepted", bool),
                     ("cg_iterations", int), ("cg_residual", float), ("step_norm", float), ("gradient_norm", float), ("lambda_new", float),
                     ("converged", int))


class BundleResult:
    """What bundle_adjust returns (hv_bundle_result and the call's arrays): cameras [N,4,4] float64 T_cw and points [M,3] float64 after
    the adjustment; chi2 [O] float64, every observation's chi2 at the final state (0 where inactive or behind); behind [O] bool, the
    observations switched off at the first linearisation because their point lay behind the camera; inlier [O] bool = active, not
    behind and chi2 <= the gate (huber_delta2_mono / huber_delta2_stereo by the kind of the observation); chi2_initial / chi2_final,
    the objective at the first linearisation and at the final state; lambda_; iterations (outer), cg_iterations_total; converged
    ("gradient", "step", "decrease", "residual" or "max_iterations"); success; trace = None, or one dict per outer iteration (the
    fields of a pose-graph trace row, and cameras [N,4,4] / points [M,3] - the state the iteration started from)."""
    __slots__ = ("cameras", "points", "chi2", "behind", "inlier", "chi2_initial", "chi2_final", "lambda_", "iterations", "cg_iterations_total",
                 "converged", "success", "trace")

    def __init__(self, *values):
        for name, value in zip(self.__slots__, values):
            setattr(self, name, value)


class OdometryResult:
    """What ScalableTSDFVolume.track_frame_to_model and rgbd_odometry return (the fields of Open3D's tensor odometry result, plus the
    rest of hv_track_result / hv_odometry_result):  transformation 4x4 float64, T_cw after tracking, T_target_source after
    rgbd_odometry; fitness = inliers / valid source pixels and inlier_rmse (metres) of the
    last full-resolution linearisation; information 6x6 float64 (its Gauss-Newton matrix H, anchor frame, order (omega, t));
    success; iterations run per pyramid level (level 0 first); degenerate = bit l set when level l ended on a degenerate step;
    inliers / valid counts; trace = None, or one dict per linearisation (level, iteration, status, inliers, valid, sq_error,
    A 4x4, H 6x6, g 6, xi 6) when asked for.  A call with colour (hv_track_color_result) also fills photometric_inliers and
    intensity_rmse (image range [0, 1]) of that linearisation, and its trace rows carry photometric_inliers and sq_intensity_error;
    both are None after a depth-only call."""

    def __init__(self, transformation, fitness, inlier_rmse, information, success, iterations, degenerate, inliers, valid,
                 trace=None, photometric_inliers=None, intensity_rmse=None):
        self.transformation = transformation
        self.fitness = fitness
        self.inlier_rmse = inlier_rmse
        self.information = information
        self.success = success
        self.iterations = iterations
        self.degenerate = degenerate
        self.inliers = inliers
        self.valid = valid
        self.trace = trace
        self.photometric_inliers = photometric_inliers
        self.intensity_rmse = intensity_rmse

    def __repr__(self):
        return (f"OdometryResult(success={self.success}, fitness={self.fitness:.4f}, inlier_rmse={self.inlier_rmse:.6f}, "
                f"iterations={self.iterations})")


class RegistrationResult:
    """What ScalableTSDFVolume.register_volume returns (hv_register_result): transformation 4x4 float64, the refined T_dst_src
    (p_dst = T p_src) - pass it straight to integrate_volume; of the last linearisation: fitness = inliers / candidates,
    inlier_rmse (metres, unweighted SDF residual of the inliers), information 6x6 float64 (its Gauss-Newton matrix H, order
    (omega, t), motions about `anchor`, a point [3] of the destination frame: an edge of a submap pose graph), inliers and
    candidates; success; iterations = linearisations run; trace = None, or one dict per linearisation (iteration, status, inliers,
    candidates, sq_error, A 4x4, H 6x6, g 6, xi 6) when asked for."""

    def __init__(self, transformation, fitness, inlier_rmse, information, success, iterations, inliers, candidates, anchor, trace=None):
        self.transformation = transformation
        self.fitness = fitness
        self.inlier_rmse = inlier_rmse
        self.information = information
        self.success = success
        self.iterations = iterations
        self.inliers = inliers
        self.candidates = candidates
        self.anchor = anchor
        self.trace = trace

    def __repr__(self):
        return (f"RegistrationResult(success={self.success}, fitness={self.fitness:.4f}, inlier_rmse={self.inlier_rmse:.6f}, "
                f"iterations={self.iterations})")


class _Stats:
    """Base of the *Stats results below: integer fields, named (and ordered) by the subclass's __slots__, each defaulting to 0."""

    __slots__ = ()

    def __init__(self, *args, **kwargs):
        names = self.__slots__
        if len(args) > len(names):
            raise TypeError(f"{type(self).__name__}() takes at most {len(names)} arguments ({len(args)} given)")
        values = dict(zip(names, args))
        for name, value in kwargs.items():
            if name not in names or name in values:
                raise TypeError(f"{type(self).__name__}() got an unexpected or repeated argument '{name}'")
            values[name] = value
        for name in names:
            setattr(self, name, int(values.get(name, 0)))

    def as_tuple(self):
        return tuple(getattr(self, name) for name in self.__slots__)

    def __eq__(self, other):
        return isinstance(other, type(self)) and self.as_tuple() == other.as_tuple()

    def __repr__(self):
        return f"{type(self).__name__}({', '.join(f'{name}={getattr(self, name)}' for name in self.__slots__)})"


class DeintegrationStats(_Stats):
    """What ScalableTSDFVolume.deintegrate* / reintegrate_batch return (hv_deintegrate_stats): units_listed = units the frames'
    touch sets name, summed over frames; units_missing = of those, absent from the volume (skipped); voxels_removed = voxel
    observations taken out; voxels_underflow = voxels left unchanged because they held fewer observations than were to go."""

    __slots__ = ("units_listed", "units_missing", "voxels_removed", "voxels_underflow")


class PruneStats(_Stats):
    """What ScalableTSDFVolume.prune returns (hv_prune_stats): units_before = units held at the call; units_outside = released
    because their index lies outside the bounds; units_empty = released because all their weights are 0 (a unit that is both
    counts as outside); units_after = units_before - units_outside - units_empty."""

    __slots__ = ("units_before", "units_outside", "units_empty", "units_after")


class MergeStats(_Stats):
    """What ScalableTSDFVolume.integrate_volume returns (hv_merge_stats): units_source = source units that hold a weight;
    units_claimed = units new in the destination; voxels_trilinear / voxels_nearest = voxels updated from an interpolated / a
    nearest sample; voxels_updated = their sum."""

    __slots__ = ("units_source", "units_claimed", "voxels_updated", "voxels_trilinear", "voxels_nearest")


class PackStats(_Stats):
    """What ScalableTSDFVolume.unpack / save return (hv_pack_info): units = units of the packed map, all-zero ones included;
    voxels = stored voxel records (a voxel is stored when any of its five words is non-zero); bytes = size of the packed buffer."""

    __slots__ = ("units", "voxels", "bytes")


class GridPackStats(_Stats):
    """What the block grids' unpack / save return (hv_grid_pack_info): blocks = blocks of the packed grid, empty ones included;
    voxels = stored voxel records; extra_pairs = label pairs beyond the six a record holds inline (the two probabilistic
    payloads; 0 otherwise); bytes = size of the packed buffer."""

    __slots__ = ("blocks", "voxels", "extra_pairs", "bytes")


# hv_tsdf_sample_points' status and hv_tsdf_check_frame's class values (include/hipvol.h)
SAMPLE_OUTSIDE, SAMPLE_UNOBSERVED, SAMPLE_NEAREST, SAMPLE_TRILINEAR = (L.HV_SAMPLE_OUTSIDE, L.HV_SAMPLE_UNOBSERVED, L.HV_SAMPLE_NEAREST,
                                                                      L.HV_SAMPLE_TRILINEAR)
CHECK_INVALID, CHECK_UNKNOWN, CHECK_CONSISTENT, CHECK_IN_FRONT, CHECK_BEHIND = (L.HV_CHECK_INVALID, L.HV_CHECK_UNKNOWN, L.HV_CHECK_CONSISTENT,
                                                                                L.HV_CHECK_IN_FRONT, L.HV_CHECK_BEHIND)


class SampleResult:
    """What ScalableTSDFVolume.sample_points returns, one row per point: sdf [n] float32 (metres), gradient [n,3] float32 (metres
    per metre, not normalised) or None, color [n,3] float32 in [0, 1] or None, weight [n] float32 (the nearest voxel's observation
    count), status [n] uint8 (SAMPLE_OUTSIDE / SAMPLE_UNOBSERVED / SAMPLE_NEAREST / SAMPLE_TRILINEAR).  Every value is 0 where the
    status is SAMPLE_OUTSIDE or SAMPLE_UNOBSERVED."""

    def __init__(self, sdf, gradient, color, weight, status):
        self.sdf = sdf
        self.gradient = gradient
        self.color = color
        self.weight = weight
        self.status = status

    def __repr__(self):
        return f"SampleResult(n={len(self.sdf)}, gradient={self.gradient is not None}, color={self.color is not None})"


class FrameCheckStats(_Stats):
    """Pixels per class of one ScalableTSDFVolume.check_frame (hv_check_stats, in the order of the CHECK_* values)."""

    __slots__ = ("invalid", "unknown", "consistent", "in_front", "behind")


class FrameCheck:
    """What ScalableTSDFVolume.check_frame returns: sdf [H,W] float32 (the map's signed distance at the pixel's point, 0 where the
    class is CHECK_INVALID or CHECK_UNKNOWN), cls [H,W] uint8 (CHECK_*), stats (FrameCheckStats) and its five counts as attributes:
    invalid, unknown, consistent, in_front, behind."""

    def __init__(self, sdf, cls, stats):
        self.sdf = sdf
        self.cls = cls
        self.stats = stats

    invalid = property(lambda self: self.stats.invalid)
    unknown = property(lambda self: self.stats.unknown)
    consistent = property(lambda self: self.stats.consistent)
    in_front = property(lambda self: self.stats.in_front)
    behind = property(lambda self: self.stats.behind)

    def __repr__(self):
        return f"FrameCheck({', '.join(f'{name}={getattr(self.stats, name)}' for name in self.stats.__slots__)})"


# hv_lookup_points' status values (include/hipvol.h)
LOOKUP_MISSING, LOOKUP_OWN, LOOKUP_NEAR, LOOKUP_INVALID = L.HV_LOOKUP_MISSING, L.HV_LOOKUP_OWN, L.HV_LOOKUP_NEAR, L.HV_LOOKUP_INVALID


class LookupStats(_Stats):
    """Points per status of one lookup_points call (hv_lookup_stats): points = own + near + missing + invalid."""

    __slots__ = ("points", "own", "near", "missing", "invalid")


class VoxelLookup:
    """What lookup_points of a block grid returns, one row per point: status [n] uint8 (LOOKUP_MISSING / LOOKUP_OWN / LOOKUP_NEAR /
    LOOKUP_INVALID), count [n] int32, position [n,3] float64 (the found voxel's mean position, the row get_voxels lists), color [n,3]
    float32, class_id / object_id [n] int32 and confidence [n] float32 (None on the plain VoxelBlockGrid / VoxelGrid), stats
    (LookupStats, or None when not asked for).  MISSING and INVALID rows hold count 0, position and colour 0, ids -1, confidence 0."""

    def __init__(self, status, count, position, color, class_id, object_id, confidence, stats):
        self.status = status
        self.count = count
        self.position = position
        self.color = color
        self.class_id = class_id
        self.object_id = object_id
        self.confidence = confidence
        self.stats = stats

    def __repr__(self):
        return f"VoxelLookup(n={len(self.status)}, labels={self.class_id is not None}, stats={self.stats})"


class SpeckleStats(_Stats):
    """What one speckle filter found (hv_speckle_stats): valid_pixels = pixels that differ from new_val, components = connected
    regions among them, largest = the largest region's pixel count, removed_components / removed_pixels = what the size rule took."""

    __slots__ = ("valid_pixels", "components", "largest", "removed_components", "removed_pixels")


class ConsistencyStats(_Stats):
    """What one filter_depth_consistency found (hv_consistency_stats): valid_pixels = pixels with a depth on input, kept_pixels =
    pixels the check kept, agree_sum = the sum over all pixels of the views that agree."""

    __slots__ = ("valid_pixels", "kept_pixels", "agree_sum")


class SpeckleResult:
    """What filter_speckles returns when more than the image is asked for: image (the filtered image), depth (the companion depth
    with 0 where a pixel was removed, or None), labels (int32 [H,W]: the smallest row-major index of the pixel's region, -1 for an
    invalid pixel, or None), stats (SpeckleStats or None)."""

    def __init__(self, image, depth, labels, stats):
        self.image = image
        self.depth = depth
        self.labels = labels
        self.stats = stats

    def __repr__(self):
        return f"SpeckleResult(shape={tuple(self.image.shape)}, depth={self.depth is not None}, labels={self.labels is not None}, stats={self.stats})"


class Features(typing.NamedTuple):
    """What detect_features returns: keypoints int32 [N,5] = x, y (at the keypoint's level), level, score, orientation bin, in the
    order of rule F7; xy float32 [N,2], the level-0 position ((x + 0.5) 2^level - 0.5, (y + 0.5) 2^level - 0.5); descriptors uint8
    [N,32]."""

    keypoints: typing.Any
    xy: typing.Any
    descriptors: typing.Any


class MatchResult(typing.NamedTuple):
    """What match_features returns: index int32 [S,Nq], the global train index of each accepted match or -1; distance / second
    uint16 [S,Nq], the best and second-best Hamming distance in the segment, accepted or not; counts int32 [S], the accepted matches
    per segment."""

    index: typing.Any
    distance: typing.Any
    second: typing.Any
    counts: typing.Any


def feature_capacity(height, width, levels, per_cell):
    """The rows hv_orb_detect wants its outputs to have: per_cell times the 32x32 cells of every pyramid level that yields."""
    n = 0
    for _ in range(int(levels)):
        if height < 33 or width < 33:
            break
        n += ((height + 31) // 32) * ((width + 31) // 32) * int(per_cell)
        height, width = height // 2, width // 2
    return n


# hv_tsdf_distance_field's cell classes (include/hipvol.h): DIST_SITE is OR-ed onto DIST_FREE or DIST_INSIDE
DIST_UNKNOWN, DIST_FREE, DIST_INSIDE, DIST_SITE = L.HV_DIST_UNKNOWN, L.HV_DIST_FREE, L.HV_DIST_INSIDE, L.HV_DIST_SITE


class DistanceFieldStats(_Stats):
    """Cells per kind of one ScalableTSDFVolume.distance_field (hv_distance_stats), over the box the call computed (the padded one
    with pad=True): unknown + free + inside = cells; sites = cells at a sign change of the map; far = cells with no site of the box
    nearer than max_distance."""

    __slots__ = ("unknown", "free", "inside", "sites", "far")


class DistanceField:
    """What ScalableTSDFVolume.distance_field returns: a dense grid over a box of the map's voxel lattice, cell (i, j, k) being voxel
    origin + (i, j, k), centred at (origin + (i, j, k) + 0.5) * voxel_length.  distance [nx,ny,nz] float32: metres to the nearest
    surface site, negative inside a surface, capped at max_distance; dist2 [nx,ny,nz] uint32: the same in squared voxels, capped at
    R^2; cls [nx,ny,nz] uint8: DIST_UNKNOWN / DIST_FREE / DIST_INSIDE, with DIST_SITE OR-ed on at a sign change.  An output that was
    not asked for is None.  origin [3] int64, shape (nx, ny, nz), voxel_length, radius = R, max_distance = R * voxel_length, stats
    (DistanceFieldStats of the computed box)."""

    def __init__(self, distance, dist2, cls, origin, shape, voxel_length, radius, stats):
        self.distance = distance
        self.dist2 = dist2
        self.cls = cls
        self.origin = np.asarray(origin, np.int64).reshape(3)
        self.shape = tuple(int(n) for n in shape)
        self.voxel_length = float(voxel_length)
        self.radius = int(radius)
        self.max_distance = float(self.radius * np.float64(voxel_length))
        self.stats = stats

    def cell_of(self, points):
        """points [n,3] world metres -> (idx [n,3] int64 = floor(p / voxel_length) - origin, inside [n] bool: the cell is in the box).
        Not finite: outside."""
        p = np.asarray(points, np.float64).reshape(-1, 3)
        with np.errstate(invalid="ignore"):
            q = np.floor(p / np.float64(self.voxel_length))
            ok = np.isfinite(q).all(axis=1) & (np.abs(q) < 2.0 ** 62).all(axis=1)
        idx = np.where(ok[:, None], q, 0.0).astype(np.int64) - self.origin
        inside = ok & ((idx >= 0) & (idx < np.asarray(self.shape, np.int64))).all(axis=1)
        return idx, inside

    def lookup(self, points):
        """distance at the cell that contains each of points [n,3] (float32 [n], numpy); max_distance where the point is outside
        the box - as float32(R) * float32(voxel_length), the very value a far cell holds."""
        if self.distance is None:
            raise ValueError("DistanceField.lookup: the field was computed without 'distance'")
        idx, inside = self.cell_of(points)
        out = np.full(len(idx), np.float32(self.radius) * np.float32(self.voxel_length), np.float32)
        i = idx[inside]
        if _is_torch(self.distance):
            import torch

            t = torch.from_numpy(i).to(self.distance.device)
            out[inside] = self.distance[t[:, 0], t[:, 1], t[:, 2]].cpu().numpy()
        else:
            out[inside] = self.distance[i[:, 0], i[:, 1], i[:, 2]]
        return out

    def __repr__(self):
        return f"DistanceField(origin={self.origin.tolist()}, shape={self.shape}, max_distance={self.max_distance:g})"


class SurfaceComponentsStats(_Stats):
    """Counts of one ScalableTSDFVolume.surface_components (hv_components_stats): units = units held; sites = surface sites;
    components = connected components of the sites; largest = the most sites in one component."""

    __slots__ = ("units", "sites", "components", "largest")


class SurfaceComponents:
    """What ScalableTSDFVolume.surface_components returns.  Per component, numbered 0 .. C-1 by increasing seed: seed [C,3] int32
    (its smallest site in (x, y, z) order of the global voxel index), sites [C] int64 (how many), lo, hi [C,3] int32 (its inclusive
    bounding box in global voxel indices; voxel q has its centre at (q + 0.5) * voxel_length).  With sites=True the site list:
    site_index [N,3] int32 and site_label [N] int32 (the component number), rows sorted by unit key, then by x * 256 + y * 16 + z
    inside the unit; else both None.  stats (SurfaceComponentsStats), voxel_length."""

    def __init__(self, seed, sites, lo, hi, site_index, site_label, stats, voxel_length):
        self.seed = seed
        self.sites = sites
        self.lo = lo
        self.hi = hi
        self.site_index = site_index
        self.site_label = site_label
        self.stats = stats
        self.voxel_length = float(voxel_length)

    def __len__(self):
        return int(self.stats.components)

    def __repr__(self):
        return f"SurfaceComponents(components={self.stats.components}, sites={self.stats.sites}, largest={self.stats.largest})"


class ComponentRemovalStats(typing.NamedTuple):
    """What ScalableTSDFVolume.remove_small_components returns (hv_remove_components_stats): components, sites = what
    surface_components counts before the call; components_removed, sites_removed = those with fewer than min_sites sites;
    voxels_reset = voxels put back into the fresh state; units_changed = units holding one of them; units_emptied = changed units
    left without a weight (prune(empty=True) releases them)."""

    components: int
    components_removed: int
    sites: int
    sites_removed: int
    voxels_reset: int
    units_changed: int
    units_emptied: int


def _packed_operand(buf):
    """A packed map as the C ABI takes it: numpy array, bytes-like object or torch tensor (either device) -> contiguous 1-D uint8,
    numpy for host memory, torch for a GPU."""
    if _is_torch(buf):
        import torch

        if buf.dtype != torch.uint8 or buf.dim() != 1:
            raise ValueError(f"a packed map is a 1-D uint8 buffer, got {buf.dtype} with shape {tuple(buf.shape)}")
        return buf.contiguous() if buf.is_cuda else buf.contiguous().numpy()
    a = buf if isinstance(buf, np.ndarray) else np.frombuffer(buf, dtype=np.uint8)
    if a.dtype != np.uint8 or a.ndim != 1:
        raise ValueError(f"a packed map is a 1-D uint8 buffer, got {a.dtype} with shape {a.shape}")
    return np.ascontiguousarray(a)


def _packed_info(abi, path_or_buffer):
    """The header of a packed map or grid as a dict, after the library's validator (abi = a class's _PACKED) has passed the WHOLE
    buffer: a file path, or a buffer as unpack() takes it.  Needs no GPU.  ValueError with the validator's message."""
    import os

    prefix, _, Header, _, fields = abi
    if isinstance(path_or_buffer, (str, os.PathLike)):
        op = np.fromfile(path_or_buffer, dtype=np.uint8)
    else:
        op = _packed_operand(path_or_buffer)
        if _is_torch(op):
            op = op.cpu().numpy()
    lib = L.load()
    hdr = Header()
    if getattr(lib, prefix + "packed_check")(L.ptr(op), int(op.size), ctypes.byref(hdr)) != L.HV_OK:
        raise ValueError((lib.hv_last_error() or (prefix + "packed_check failed").encode()).decode())
    return {name: getattr(hdr, name) for name in fields}


_UNIT_KEY_BIAS = 1 << 20  # the library packs a unit index into 21 bits per axis: [-2^20, 2^20)


def unit_range_of_bounds(bounds, voxel_length, resolution=16):
    """(min_xyz, max_xyz) in world metres -> (lo[3], hi[3]) int32, the inclusive range of unit indices ScalableTSDFVolume.prune
    keeps: lo = floor(min / L), hi = floor(max / L) per axis with L = voxel_length * resolution, in float64.  Unit k covers the
    half-open box [k L, (k + 1) L), so these are exactly the units that meet the closed box.  ValueError on min > max, non-finite
    values or a range outside the library's unit keys."""
    try:
        lo_m, hi_m = bounds
        lo_m = np.asarray(lo_m, dtype=np.float64).reshape(-1)
        hi_m = np.asarray(hi_m, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError) as e:
        raise ValueError(f"bounds must be (min_xyz, max_xyz): {e}") from None
    if lo_m.shape != (3,) or hi_m.shape != (3,):
        raise ValueError("bounds must be (min_xyz, max_xyz) with three coordinates each")
    L_unit = np.float64(voxel_length) * np.float64(resolution)
    if not (np.isfinite(L_unit) and L_unit > 0.0):
        raise ValueError(f"bad unit length {L_unit}")
    if not (np.all(np.isfinite(lo_m)) and np.all(np.isfinite(hi_m))):
        raise ValueError("bounds must be finite")
    if np.any(lo_m > hi_m):
        raise ValueError(f"bounds: min {lo_m.tolist()} exceeds max {hi_m.tolist()}")
    lo, hi = np.floor(lo_m / L_unit), np.floor(hi_m / L_unit)
    if np.any(lo < -_UNIT_KEY_BIAS) or np.any(hi >= _UNIT_KEY_BIAS):
        raise ValueError(f"bounds reach beyond the unit keys [-2^20, 2^20): units {lo.tolist()} .. {hi.tolist()}")
    return lo.astype(np.int32), hi.astype(np.int32)


_TRACK_HEAD = (("level", int), ("iteration", int), ("status", int), ("inliers", int), ("valid", int), ("sq_error", float))
_REGISTER_HEAD = (("iteration", int), ("status", int), ("inliers", int), ("candidates", int), ("sq_error", float))


def _trace_rows(rows, head=_TRACK_HEAD):
    """The per-linearisation record of tracking / registration, rows [n, stride] float64 -> one dict per row: the leading scalars
    that `head` names, then A 4x4, H 6x6 (stored as its upper triangle), g 6, xi 6; a hybrid tracking row holds two more columns."""
    out = []
    iu = np.triu_indices(6)
    k = len(head)
    for r in rows:
        H = np.zeros((6, 6))
        H[iu] = r[k + 16:k + 37]
        H = H + np.triu(H, 1).T
        out.append({name: kind(r[i]) for i, (name, kind) in enumerate(head)})
        out[-1].update(A=r[k:k + 16].reshape(4, 4).copy(), H=H, g=r[k + 37:k + 43].copy(), xi=r[k + 43:k + 49].copy())
        if len(r) > L.HV_TRACK_TRACE_STRIDE:  # a hybrid call's row
            out[-1].update(photometric_inliers=int(r[56]), sq_intensity_error=float(r[57]))
    return out


_NOTHING_TO_ORDER = contextlib.nullcontext()  # what _Volume._ordered() returns for host operands


class _Volume:
    """Owns one hv_volume handle."""

    def __init__(self, mode, voxel_size, sdf_trunc, block_size, stride, device, max_blocks, max_points):
        lib = L.load()
        cfg = L.HvConfig()
        lib.hv_default_config(mode, ctypes.byref(cfg))
        cfg.device = int(device)
        cfg.voxel_size = float(voxel_size)
        cfg.sdf_trunc = float(sdf_trunc)
        cfg.block_size = int(block_size)
        cfg.depth_sampling_stride = int(stride)
        if max_blocks is not None:
            cfg.max_blocks = int(max_blocks)
        if max_points is not None:
            cfg.max_points = int(max_points)
        self._lib = lib
        self._cfg = cfg
        handle = ctypes.c_void_p()
        L.check(lib.hv_create(ctypes.byref(cfg), ctypes.byref(handle)))
        self._h = handle

    def close(self):
        if getattr(self, "_h", None):
            self._lib.hv_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- the steps every method is made of ------------------------------------------------------------
    def _int64(self, fn, *args):
        """fn(handle, *args, &n) -> n: the library's single-integer getters."""
        n = ctypes.c_int64()
        L.check(fn(self._h, *args, ctypes.byref(n)))
        return n.value

    def _sized_fetch(self, call, *specs):
        """The two-call fetch: call(*pointers, capacity, &count) with null pointers and capacity 0 asks for the count; unless that
        is 0 the second call fills zeroed host arrays [count, *row shape], one per spec = (row shape, dtype).  -> the arrays."""
        n = ctypes.c_int64()
        L.check(call(*(None,) * len(specs), 0, ctypes.byref(n)))
        out = [np.zeros((n.value,) + tuple(row), dtype) for row, dtype in specs]
        if n.value:
            L.check(call(*(L.ptr(a) for a in out), n.value, ctypes.byref(n)))
        return out

    def _device(self):
        """The volume's GPU as a torch.device (made on first use: no host-only path comes here)."""
        if getattr(self, "_torch_device", None) is None:
            import torch

            self._torch_device = torch.device("cuda", int(self._cfg.device))
        return self._torch_device

    def _results(self, spec, device, pinned=True, synchronize=True):
        """The buffers one call writes its results to: spec {name: (shape, numpy dtype) or None} -> {name: array or None}.  On the
        host numpy arrays, page-locked when large (_result_array; pinned=False: plain np.empty).  With `device` torch tensors on
        the volume's GPU (torch has no uint32 arithmetic: such a result is an int32 tensor with the same bits); synchronize: then
        wait for torch's current stream - the allocator may hand out blocks with work pending on that stream, which a launch
        outside _ordered() does not wait for."""
        if not device:
            make = _result_array if pinned else np.empty
            return {name: None if s is None else make(s[0], s[1]) for name, s in spec.items()}
        import torch

        dev = self._device()
        out = {name: None if s is None else torch.empty(tuple(s[0]), dtype=getattr(torch, np.dtype(s[1]).name.replace("uint32", "int32")),
                                                        device=dev) for name, s in spec.items()}
        if synchronize:
            torch.cuda.current_stream(dev).synchronize()
        return out

    # -- shared introspection -------------------------------------------------------------------
    def num_blocks(self):
        return self._int64(self._lib.hv_num_blocks)

    def max_blocks(self):
        return self._int64(self._lib.hv_max_blocks)

    def reserve_blocks(self, new_max_blocks):
        """Grow the block pool / hash, keeping the contents (also happens automatically when more than half full)."""
        L.check(self._lib.hv_reserve_blocks(self._h, int(new_max_blocks)))

    def synchronize(self):
        L.check(self._lib.hv_synchronize(self._h))

    def set_stream(self, stream_handle):
        """Adopt a caller-owned hipStream_t (e.g. ``torch.cuda.Stream().cuda_stream``)."""
        L.check(self._lib.hv_set_stream(self._h, ctypes.c_void_p(int(stream_handle))))

    def register_host_memory(self, address, nbytes):
        """Page-lock [address, address + nbytes) (hv_host_register): host frames inside it are DMA'd in place."""
        L.check(self._lib.hv_host_register(ctypes.c_void_p(int(address)), int(nbytes)))

    def unregister_host_memory(self, address):
        L.check(self._lib.hv_host_unregister(ctypes.c_void_p(int(address))))

    # -- torch CUDA tensors handed to / returned by the C ABI ------------------------------------------
    def _torch_stream(self, device):
        """The volume's hipStream_t as a torch stream (for event ordering against torch's streams and the caching allocator)."""
        import torch

        h = int(self._lib.hv_get_stream(self._h) or 0)
        if getattr(self, "_ts_key", None) != (h, device):
            self._ts = torch.cuda.ExternalStream(h, device=device) if h else torch.cuda.default_stream(device)
            self._ts_key = (h, device)
        return self._ts

    def adopt_torch_stream(self):
        """Run this volume's launches on a torch stream of its own device and hand that stream back: inside
        ``with torch.cuda.stream(s)`` torch ops (uploads, allocations) and the volume's kernels are ordered by the one queue, and
        _torch_in / _torch_out need no cross-stream event waits (eight per semantic keyframe otherwise)."""
        import torch

        if getattr(self, "_adopted", None) is None:
            self._adopted = torch.cuda.Stream(self._device())
            self.set_stream(self._adopted.cuda_stream)
        return self._adopted

    def _torch_in(self, *tensors):
        """Before a launch that reads / writes torch CUDA tensors on the volume's stream: that stream waits for what torch's
        current stream has queued (the producers).  No host synchronisation.  -> the volume's torch stream, or None when no
        tensor is on a GPU.  Always paired with _torch_out() after the launch."""
        import torch

        for t in tensors:
            if t is not None and getattr(t, "is_cuda", False):
                cur = torch.cuda.current_stream(t.device)
                if int(cur.cuda_stream) == int(self._lib.hv_get_stream(self._h) or 0) and int(cur.cuda_stream) != 0:
                    return None  # the volume runs on torch's current stream (adopt_torch_stream): already ordered
                ts = self._torch_stream(t.device)
                ts.wait_stream(cur)
                return ts
        return None

    def _torch_out(self, ts, device):
        """After such a launch: torch's current stream waits for the volume's.  Torch ops on the results are ordered after
        the launch, and so is everything the caching allocator may later place in a block the caller drops (a block freed
        on torch's stream is only reused by work queued on that stream), so tensors may be released right after the call.
        (record_stream() on the volume's stream would say the same to the allocator, but leaves it holding events on a stream
        that hv_destroy() may already have destroyed when the tensor is finally freed.)"""
        import torch

        if ts is not None:
            torch.cuda.current_stream(device).wait_stream(ts)

    def _ordered(self, *tensors):
        """``with self._ordered(operands and results):`` around a launch that reads / writes torch tensors: _torch_in() before,
        _torch_out() after, also when the launch raises.  Host arrays and None take no part; with nothing on a GPU it does nothing."""
        for t in tensors:
            if t is not None and getattr(t, "is_cuda", False):
                return self._ordered_on(t)
        return _NOTHING_TO_ORDER

    @contextlib.contextmanager
    def _ordered_on(self, tensor):
        ts = self._torch_in(tensor)
        try:
            yield
        finally:
            if ts is not None:
                self._torch_out(ts, tensor.device)

    def _publish(self, dev):
        """After a launch that only WRITES torch tensors (allocated by _results): torch's current stream waits for the volume's."""
        self._torch_out(self._torch_stream(dev), dev)

    def _query_place(self, a, device):
        """Where a query runs: -> (operand at that place, torch device or None).  device=None: where the operand lives (a torch CUDA
        tensor stays on its GPU, anything else is host memory); True / False: the volume's GPU / the host, the operand moved there."""
        on_gpu = L.location(a) == L.HV_DEVICE
        if device is None:
            device = on_gpu
        if not device:
            return (a.cpu().numpy() if _is_torch(a) else a), None
        import torch

        dev = self._device()
        if on_gpu and a.device != dev:
            raise ValueError(f"the operand lives on {a.device}, the volume on {dev}")
        return (a if on_gpu else torch.as_tensor(a).to(dev)), dev

    def dropped_points(self):
        return self._int64(self._lib.hv_dropped_points)

    def profile_enable(self, on=True):
        L.check(self._lib.hv_profile_enable(self._h, 1 if on else 0))

    def profile_read(self):
        ms, launches, units = ctypes.c_double(), ctypes.c_int64(), ctypes.c_int64()
        L.check(self._lib.hv_profile_read(self._h, ctypes.byref(ms), ctypes.byref(launches), ctypes.byref(units)))
        return ms.value, launches.value, units.value

    def profile_launches(self):
        """Durations (ms) of the bracketed launches since profile_enable / the last profile_read, in issue order."""
        return self._sized_fetch(functools.partial(self._lib.hv_profile_read_launches, self._h), ((), np.float32))[0]

    def filter_shadow_points(self, depth, delta_x=2, delta_y=2, fill_value=-1.0, stream=None):
        """pyslam.utilities.depth.filter_shadow_points(depth, delta_depth=None, ...) on the GPU.
        stream: a torch.cuda.Stream - the launches of a CUDA tensor's filter go to THAT stream (which must be torch's current one:
        the result is allocated on it) instead of the volume's; the filter reads nothing of the volume, so it may run beside the
        volume's kernels (device_pipeline.KeyframeUploader: the next keyframe's depth is filtered while this one is fused)."""
        if stream is not None or _is_torch(depth):
            import torch

            d = depth.contiguous().float()
            out = torch.empty_like(d)
        else:
            d = np.ascontiguousarray(depth, dtype=np.float32)
            out = np.empty_like(d)
        args = (self._h, L.ptr(d), int(d.shape[0]), int(d.shape[1]), int(delta_x), int(delta_y), float(fill_value), L.ptr(out))
        if stream is not None:
            L.check(self._lib.hv_filter_shadow_points_on_stream(*args, int(stream.cuda_stream)))
        else:
            with self._ordered(d, out):
                L.check(self._lib.hv_filter_shadow_points(*args, L.location(d)))
        return out

    def filter_speckles(self, image, max_speckle_size, max_diff, new_val=None, depth=None, labels=False, stats=False):
        """cv2.filterSpeckles(image, new_val, max_speckle_size, max_diff) on the GPU (hv_filter_speckles, rules S1 - S7 in
        include/hipvol.h): the pixels of every 4-connected region of at most max_speckle_size pixels - neighbours belong together
        when both differ from new_val and from each other by at most max_diff - are set to new_val.  image: [H,W] int16 (disparity in
        sixteenths; new_val defaults to -16) or float32 (depth; new_val defaults to 0.0).  numpy in, numpy out; a torch CUDA tensor
        on the volume's GPU in, tensors on that GPU out, queued on the volume's stream.  The inputs are never written.
        -> the filtered image; with depth= (a float32 [H,W] companion that gets 0 where a pixel is removed), labels=True or
        stats=True a SpeckleResult (stats=True waits for the GPU).  Works on a volume of any mode and reads nothing of it."""
        on_gpu = L.location(image) == L.HV_DEVICE
        if on_gpu:
            import torch

            kinds = {torch.int16: L.HV_SPECKLE_I16, torch.float32: L.HV_SPECKLE_F32}
            if image.device != self._device():
                raise ValueError(f"filter_speckles: the image lives on {image.device}, the volume on {self._device()}")
            a = image.contiguous()
        else:
            a = image.cpu().numpy() if _is_torch(image) else np.asarray(image)
            kinds = {np.dtype(np.int16): L.HV_SPECKLE_I16, np.dtype(np.float32): L.HV_SPECKLE_F32}
            a = np.ascontiguousarray(a)
        if a.dtype not in kinds:
            raise ValueError(f"filter_speckles: the image must be int16 or float32, got {a.dtype}")
        kind = kinds[a.dtype]
        if a.ndim != 2:
            raise ValueError(f"filter_speckles: the image must be [H, W], got {tuple(a.shape)}")
        H, W = int(a.shape[0]), int(a.shape[1])
        # what hv_filter_speckles answers with HV_ERR_INVALID, refused here before anything is allocated
        if H < 1 or W < 1 or H > 32768 or W > 32768 or H * W >= 1 << 30:
            raise ValueError(f"filter_speckles: bad image size {tuple(a.shape)}")
        if int(max_speckle_size) != max_speckle_size or int(max_speckle_size) < 0:
            raise ValueError(f"filter_speckles: max_speckle_size must be an integer >= 0, got {max_speckle_size}")
        md = float(max_diff)
        if not (0.0 <= md < np.inf) or (kind == L.HV_SPECKLE_I16 and md > 65535.0):
            raise ValueError(f"filter_speckles: max_diff must be finite and not negative (int16: at most 65535), got {max_diff}")
        nv = float(new_val) if new_val is not None else (-16.0 if kind == L.HV_SPECKLE_I16 else 0.0)
        if kind == L.HV_SPECKLE_I16 and not (-32768.0 <= nv <= 32767.0 and nv == np.floor(nv)):
            raise ValueError(f"filter_speckles: new_val of an int16 image must be an integer in -32768..32767, got {new_val}")
        d = None
        if depth is not None:
            if (L.location(depth) == L.HV_DEVICE) != on_gpu:
                raise ValueError("filter_speckles: image and depth must live in the same place")
            if on_gpu:
                if depth.dtype != torch.float32 or depth.device != self._device():
                    raise ValueError(f"filter_speckles: depth must be a float32 tensor on {self._device()}")
                d = depth.clone(memory_format=torch.contiguous_format)  # (the library writes it in place: the caller's stays)
            else:
                d = depth.cpu().numpy() if _is_torch(depth) else np.asarray(depth)
                if d.dtype != np.float32:
                    raise ValueError(f"filter_speckles: depth must be float32, got {d.dtype}")
                d = np.array(d, dtype=np.float32, order="C", copy=True)
            if tuple(d.shape) != (H, W):
                raise ValueError(f"filter_speckles: depth {tuple(d.shape)} must have the image's shape {(H, W)}")
        out = self._results({"image": ((H, W), np.int16 if kind == L.HV_SPECKLE_I16 else np.float32),
                             "labels": ((H, W), np.int32) if labels else None}, on_gpu, pinned=False, synchronize=False)
        st = L.HvSpeckleStats() if stats else None
        with self._ordered(a, d, out["image"], out["labels"]):
            L.check(self._lib.hv_filter_speckles(self._h, L.ptr(a), kind, H, W, nv, int(max_speckle_size), md, L.ptr(out["image"]), L.ptr(d),
                                                 L.ptr(out["labels"]), ctypes.byref(st) if stats else None, L.location(a)))
        if depth is None and not labels and not stats:
            return out["image"]
        return SpeckleResult(out["image"], d, out["labels"], _stats(SpeckleStats, st) if stats else None)

    def stereo_sgm(self, left, right, num_disparities=128, p1=10, p2=120, uniqueness_ratio=15, max_diff=1, paths=8, bf=None,
                   min_depth=0.0, max_depth=np.inf, speckle_window_size=0, speckle_range=1):
        """Census semi-global stereo matching of a rectified uint8 pair, [H,W] or [H,W,3] (hv_stereo_sgm, the rules in
        include/hipvol.h) -> (disparity int16 [H,W] in sixteenths of a pixel, -16 = invalid; depth float32 [H,W] metres = bf 16 /
        disparity, 0 = none - or None when bf is None).  numpy arrays in, numpy arrays out; torch CUDA tensors in, tensors on the
        same GPU out, queued on the volume's stream.  Works on a volume of any mode and reads nothing of it.
        speckle_window_size > 0 (cv2.StereoSGBM's speckleWindowSize; the reference sets 50) removes, on the device, the connected
        regions of at most that many pixels whose neighbouring disparities differ by at most speckle_range pixels
        (hv_stereo_sgm_speckle; filter_speckles is the step on its own): disparity -16 and depth 0 there.  0: no filter."""
        on_gpu = L.location(left) == L.HV_DEVICE
        if on_gpu != (L.location(right) == L.HV_DEVICE):
            raise ValueError("stereo_sgm: left and right must live in the same place")
        if on_gpu:
            import torch

            if left.dtype != torch.uint8 or right.dtype != torch.uint8:
                raise ValueError("stereo_sgm: the images must be uint8")
            if left.device != self._device() or right.device != self._device():
                raise ValueError(f"stereo_sgm: the images live on {left.device} / {right.device}, the volume on {self._device()}")
            a, b = left.contiguous(), right.contiguous()
        else:
            a, b = (x.cpu().numpy() if _is_torch(x) else np.asarray(x) for x in (left, right))
            if a.dtype != np.uint8 or b.dtype != np.uint8:
                raise ValueError("stereo_sgm: the images must be uint8")
            a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        if tuple(a.shape) != tuple(b.shape) or a.ndim not in (2, 3):
            raise ValueError(f"stereo_sgm: left {tuple(a.shape)} and right {tuple(b.shape)} must be two images of one shape")
        H, W = int(a.shape[0]), int(a.shape[1])
        channels = 1 if a.ndim == 2 else int(a.shape[2])
        # what hv_stereo_sgm answers with HV_ERR_INVALID, refused here before anything is allocated
        if channels not in (1, 3):
            raise ValueError(f"stereo_sgm: images must have 1 or 3 channels, got {channels}")
        if H < 1 or W < 1:
            raise ValueError(f"stereo_sgm: empty image {tuple(a.shape)}")
        if not (16 <= int(num_disparities) <= 256 and int(num_disparities) % 16 == 0):
            raise ValueError(f"stereo_sgm: num_disparities must be a multiple of 16 in 16..256, got {num_disparities}")
        if not 0 < int(p1) <= int(p2) <= 1023:
            raise ValueError(f"stereo_sgm: need 0 < p1 <= p2 <= 1023, got p1 = {p1}, p2 = {p2}")
        if not 0 <= int(uniqueness_ratio) <= 99:
            raise ValueError(f"stereo_sgm: uniqueness_ratio must be in 0..99, got {uniqueness_ratio}")
        if int(paths) not in (4, 8):
            raise ValueError(f"stereo_sgm: paths must be 4 or 8, got {paths}")
        if bf is not None and not 0.0 < float(bf) <= float(np.finfo(np.float32).max):  # (the library reads a float32)
            raise ValueError(f"stereo_sgm: bf must be finite and positive, got {bf}")
        if int(speckle_window_size) != speckle_window_size or not 0 <= int(speckle_window_size) <= 1 << 30:
            raise ValueError(f"stereo_sgm: speckle_window_size must be an integer in 0..2^30, got {speckle_window_size}")
        if int(speckle_range) != speckle_range or not 0 <= int(speckle_range) <= 4095:
            raise ValueError(f"stereo_sgm: speckle_range must be an integer in 0..4095, got {speckle_range}")
        prm = L.HvStereoParams(int(num_disparities), int(p1), int(p2), int(uniqueness_ratio), int(max_diff), int(paths),
                               float(bf) if bf is not None else 0.0, float(min_depth), float(max_depth))
        out = self._results({"disparity": ((H, W), np.int16), "depth": ((H, W), np.float32) if bf is not None else None}, on_gpu,
                            pinned=False, synchronize=False)
        with self._ordered(a, b, out["disparity"], out["depth"]):
            if int(speckle_window_size) == 0:
                L.check(self._lib.hv_stereo_sgm(self._h, L.ptr(a), L.ptr(b), H, W, channels, ctypes.byref(prm), L.ptr(out["disparity"]),
                                                L.ptr(out["depth"]), L.location(a)))
            else:
                L.check(self._lib.hv_stereo_sgm_speckle(self._h, L.ptr(a), L.ptr(b), H, W, channels, ctypes.byref(prm), int(speckle_window_size),
                                                        int(speckle_range), L.ptr(out["disparity"]), L.ptr(out["depth"]), None, L.location(a)))
        return out["disparity"], out["depth"]

    def detect_features(self, image, levels=3, threshold=20, per_cell=8):
        """Oriented binary keypoints of a uint8 image, [H,W] or [H,W,3] (hv_orb_detect, the rules F1 - F11 in include/hipvol.h):
        FAST-9 corners on a factor-2 pyramid, non-maximum suppression, the per_cell strongest of every 32x32 cell, an orientation
        bin and a steered 256-bit descriptor each.  -> Features(keypoints, xy, descriptors).  A numpy array in, numpy arrays out;
        a torch CUDA tensor on the volume's GPU in, tensors out.  The call waits for the GPU (it returns the count).  Works on a
        volume of any mode and reads nothing of it."""
        on_gpu = L.location(image) == L.HV_DEVICE
        if on_gpu:
            import torch

            if image.dtype != torch.uint8:
                raise ValueError("detect_features: the image must be uint8")
            if image.device != self._device():
                raise ValueError(f"detect_features: the image lives on {image.device}, the volume on {self._device()}")
            a = image.contiguous()
        else:
            a = image.cpu().numpy() if _is_torch(image) else np.asarray(image)
            if a.dtype != np.uint8:
                raise ValueError("detect_features: the image must be uint8")
            a = np.ascontiguousarray(a)
        if a.ndim not in (2, 3):
            raise ValueError(f"detect_features: the image must be [H,W] or [H,W,3], got {tuple(a.shape)}")
        H, W = int(a.shape[0]), int(a.shape[1])
        channels = 1 if a.ndim == 2 else int(a.shape[2])
        # what hv_orb_detect answers with HV_ERR_INVALID, refused here before anything is allocated
        if channels not in (1, 3):
            raise ValueError(f"detect_features: images must have 1 or 3 channels, got {channels}")
        if H < 1 or W < 1 or H > 32768 or W > 32768:
            raise ValueError(f"detect_features: height and width must be in 1..32768, got {tuple(a.shape)}")
        for name, value, lo, hi in (("levels", levels, 1, 8), ("threshold", threshold, 1, 254), ("per_cell", per_cell, 1, 16)):
            if int(value) != value or not lo <= int(value) <= hi:
                raise ValueError(f"detect_features: {name} must be an integer in {lo}..{hi}, got {value}")
        bound = feature_capacity(H, W, levels, per_cell)
        cap = max(bound, 1)
        prm = L.HvFeatureParams(int(levels), int(threshold), int(per_cell))
        out = self._results({"keypoints": ((cap, 5), np.int32), "descriptors": ((cap, 32), np.uint8)}, on_gpu, pinned=False, synchronize=False)
        count = ctypes.c_int32(0)
        with self._ordered(a, out["keypoints"], out["descriptors"]):
            L.check(self._lib.hv_orb_detect(self._h, L.ptr(a), H, W, channels, ctypes.byref(prm), L.ptr(out["keypoints"]), L.ptr(out["descriptors"]),
                                            cap, ctypes.byref(count), L.location(a)))
        n = int(count.value)
        kp, desc = out["keypoints"][:n], out["descriptors"][:n]
        if on_gpu:
            import torch

            scale = torch.pow(2.0, kp[:, 2:3].clamp(0, 7).to(torch.float32))
            xy = (kp[:, 0:2].to(torch.float32) + 0.5) * scale - 0.5
        else:
            scale = (1 << np.clip(kp[:, 2:3], 0, 7)).astype(np.float32)
            xy = ((kp[:, 0:2].astype(np.float32) + np.float32(0.5)) * scale - np.float32(0.5)).astype(np.float32)
        return Features(kp, xy, desc)

    def match_features(self, query, train, segments=None, max_distance=64, ratio=0.8, cross_check=True):
        """Brute-force Hamming matching of 256-bit descriptors, query uint8 [Nq,32] against train uint8 [Nt,32]
        (hv_match_descriptors, the rules M1 - M5 in include/hipvol.h).  segments: int32 [S+1] offsets into train (non-decreasing, first
        0, last Nt), one segment per keyframe - None: one segment, all of train.  A match is accepted when its distance is at most
        max_distance, 100 d1 < round(100 ratio) d2 (ratio=None: no ratio test) and, with cross_check, the query is the best one of its
        train descriptor among all queries.  -> MatchResult(index [S,Nq], distance, second, counts [S]).  numpy arrays in, numpy
        arrays out; torch CUDA tensors on the volume's GPU in, tensors out, queued on the volume's stream.  Works on a volume of any
        mode and reads nothing of it."""
        on_gpu = L.location(query) == L.HV_DEVICE
        if on_gpu != (L.location(train) == L.HV_DEVICE):
            raise ValueError("match_features: query and train must live in the same place")
        if on_gpu:
            import torch

            if query.dtype != torch.uint8 or train.dtype != torch.uint8:
                raise ValueError("match_features: the descriptors must be uint8")
            if query.device != self._device() or train.device != self._device():
                raise ValueError(f"match_features: the descriptors live on {query.device} / {train.device}, the volume on {self._device()}")
            q, t = query.contiguous(), train.contiguous()
        else:
            q, t = (x.cpu().numpy() if _is_torch(x) else np.asarray(x) for x in (query, train))
            if q.dtype != np.uint8 or t.dtype != np.uint8:
                raise ValueError("match_features: the descriptors must be uint8")
            q, t = np.ascontiguousarray(q), np.ascontiguousarray(t)
        if q.ndim != 2 or t.ndim != 2 or q.shape[1] != 32 or t.shape[1] != 32:
            raise ValueError(f"match_features: query {tuple(q.shape)} and train {tuple(t.shape)} must be [N,32]")
        Nq, Nt = int(q.shape[0]), int(t.shape[0])
        seg = np.array([0, Nt], np.int32) if segments is None else np.ascontiguousarray(
            segments.cpu().numpy() if _is_torch(segments) else np.asarray(segments))
        if seg.ndim != 1 or seg.shape[0] < 2 or not np.issubdtype(seg.dtype, np.integer):
            raise ValueError("match_features: segments must be a 1-D integer array of at least two offsets")
        seg = seg.astype(np.int64)
        if seg[0] != 0 or seg[-1] != Nt or (np.diff(seg) < 0).any():
            raise ValueError(f"match_features: segments must not decrease, start at 0 and end at {Nt}")
        seg = np.ascontiguousarray(seg, dtype=np.int32)
        S = int(seg.shape[0]) - 1
        # what hv_match_descriptors answers with HV_ERR_INVALID, refused here before anything is allocated
        if not 1 <= Nq <= 65536:
            raise ValueError(f"match_features: need 1..65536 query descriptors, got {Nq}")
        if Nt >= 1 << 24:
            raise ValueError(f"match_features: at most 2^24 - 1 train descriptors, got {Nt}")
        if S * Nq >= 1 << 27:
            raise ValueError(f"match_features: segments times queries must stay below 2^27, got {S} x {Nq}")
        if int(max_distance) != max_distance or not 0 <= int(max_distance) <= 256:
            raise ValueError(f"match_features: max_distance must be an integer in 0..256, got {max_distance}")
        ratio_percent = 0 if ratio is None else int(round(100.0 * float(ratio)))
        if ratio is not None and not 0 <= ratio_percent <= 100:
            raise ValueError(f"match_features: ratio must be in 0..1 or None, got {ratio}")
        prm = L.HvMatchParams(int(max_distance), ratio_percent, 1 if cross_check else 0)
        out = self._results({"index": ((S, Nq), np.int32), "distance": ((S, Nq), np.uint16), "second": ((S, Nq), np.uint16),
                             "counts": ((S,), np.int32)}, on_gpu, pinned=False, synchronize=False)
        with self._ordered(q, t, out["index"], out["distance"], out["second"], out["counts"]):
            L.check(self._lib.hv_match_descriptors(self._h, L.ptr(q), Nq, L.ptr(t) if Nt else None, Nt, L.ptr(seg), S, ctypes.byref(prm),
                                                   L.ptr(out["index"]), L.ptr(out["distance"]), L.ptr(out["second"]), L.ptr(out["counts"]),
                                                   L.location(q)))
        return MatchResult(out["index"], out["distance"], out["second"], out["counts"])

    def multiview_sgm(self, ref, sources, views=None, *, intrinsic=None, T_ref=None, T_sources=None, min_depth, max_depth=np.inf,
                      num_planes=128, p1=10, p2=120, uniqueness_ratio=15, min_views=1, paths=8, speckle_window_size=0, speckle_range=1,
                      index=True, depth=True):
        """Plane-sweep depth for a posed reference image and 1..4 source images of the same shape, uint8 [H,W] or [H,W,3]
        (hv_mvs_sgm, the rules M1 - M10 in include/hipvol.h): num_planes fronto-parallel planes of the reference camera at evenly
        spaced inverse depths from 1 / max_depth (plane 0) to 1 / min_depth, census cost through the per-view 3x4 matrices, then the
        semi-global stages of stereo_sgm.  -> (index int16 [H,W] in sixteenths of a plane, -16 = invalid: the format of a disparity;
        depth float32 [H,W], z-depth in the reference camera in metres, 0 = none); index=False / depth=False leaves that one out
        (None in its place).  sources: a list of images or one [N,H,W(,3)] array.  Pass views, [N,3,4] float32 (A p + w b is the
        source pixel of the point at depth 1 / w along p), or intrinsic (a PinholeCameraIntrinsic, 3x3 or (fx, fy, cx, cy)) with the
        world-to-camera poses T_ref [4,4] and T_sources [N,4,4], which prep.plane_sweep_views turns into the matrices.  numpy arrays
        in, numpy arrays out; torch CUDA tensors on the volume's GPU in, tensors out, queued on the volume's stream.  min_views: the
        views that must see a plane of a pixel for its cost to count.  speckle_window_size > 0 filters the index as stereo_sgm does
        its disparity.  Works on a volume of any mode and reads nothing of it."""
        on_gpu = L.location(ref) == L.HV_DEVICE
        is_list = isinstance(sources, (list, tuple))
        src_list = list(sources) if is_list else [sources]
        if not src_list or any((L.location(s) == L.HV_DEVICE) != on_gpu for s in src_list):
            raise ValueError("multiview_sgm: ref and sources must live in the same place")
        if on_gpu:
            import torch

            if ref.dtype != torch.uint8 or any(s.dtype != torch.uint8 for s in src_list):
                raise ValueError("multiview_sgm: the images must be uint8")
            if any(t.device != self._device() for t in [ref] + src_list):
                raise ValueError(f"multiview_sgm: the images must live on the volume's GPU {self._device()}")
            a, stack = ref.contiguous(), torch.stack
        else:
            a = ref.cpu().numpy() if _is_torch(ref) else np.asarray(ref)
            src_list = [s.cpu().numpy() if _is_torch(s) else np.asarray(s) for s in src_list]
            if a.dtype != np.uint8 or any(s.dtype != np.uint8 for s in src_list):
                raise ValueError("multiview_sgm: the images must be uint8")
            a, stack = np.ascontiguousarray(a), np.stack
        # a list of images of the reference's shape becomes one block; an array or tensor must be [N] + that shape already
        want = tuple(a.shape) if is_list else (int(src_list[0].shape[0]),) + tuple(a.shape) if src_list[0].ndim else None
        if a.ndim not in (2, 3) or any(tuple(s.shape) != want for s in src_list):
            raise ValueError(f"multiview_sgm: the sources must be 1..4 images of the reference's shape {tuple(a.shape)}")
        b = stack(src_list) if is_list else src_list[0].contiguous() if on_gpu else np.ascontiguousarray(src_list[0])
        N, H, W = int(b.shape[0]), int(a.shape[0]), int(a.shape[1])
        channels = 1 if a.ndim == 2 else int(a.shape[2])
        # what hv_mvs_sgm answers with HV_ERR_INVALID, refused here before anything is allocated
        if channels not in (1, 3):
            raise ValueError(f"multiview_sgm: images must have 1 or 3 channels, got {channels}")
        if H < 1 or W < 1 or H > 32768 or W > 32768 or H * W >= 1 << 30:
            raise ValueError(f"multiview_sgm: bad image size {tuple(a.shape)}")
        if not 1 <= N <= 4:
            raise ValueError(f"multiview_sgm: need 1..4 source views, got {N}")
        if not index and not depth:
            raise ValueError("multiview_sgm: no output asked for")
        if int(min_views) != min_views or not 1 <= int(min_views) <= N:
            raise ValueError(f"multiview_sgm: min_views must be in 1..{N}, got {min_views}")
        if not (16 <= int(num_planes) <= 256 and int(num_planes) % 16 == 0):
            raise ValueError(f"multiview_sgm: num_planes must be a multiple of 16 in 16..256, got {num_planes}")
        if not 0 < int(p1) <= int(p2) <= 1023:
            raise ValueError(f"multiview_sgm: need 0 < p1 <= p2 <= 1023, got p1 = {p1}, p2 = {p2}")
        if not 0 <= int(uniqueness_ratio) <= 99:
            raise ValueError(f"multiview_sgm: uniqueness_ratio must be in 0..99, got {uniqueness_ratio}")
        if int(paths) not in (4, 8):
            raise ValueError(f"multiview_sgm: paths must be 4 or 8, got {paths}")
        lo, hi = float(min_depth), float(max_depth)
        if not 0.0 < lo < np.inf:
            raise ValueError(f"multiview_sgm: min_depth must be finite and positive, got {min_depth}")
        if not hi > lo:
            raise ValueError(f"multiview_sgm: need max_depth > min_depth, got {max_depth} and {min_depth}")
        if (1.0 / lo - (0.0 if np.isinf(hi) else 1.0 / hi)) / (16.0 * (int(num_planes) - 1)) > float(np.finfo(np.float32).max):
            raise ValueError(f"multiview_sgm: min_depth {min_depth} is too small: the plane step overflows float32")
        if int(speckle_window_size) != speckle_window_size or not 0 <= int(speckle_window_size) <= 1 << 30:
            raise ValueError(f"multiview_sgm: speckle_window_size must be an integer in 0..2^30, got {speckle_window_size}")
        if int(speckle_range) != speckle_range or not 0 <= int(speckle_range) <= 4095:
            raise ValueError(f"multiview_sgm: speckle_range must be an integer in 0..4095, got {speckle_range}")
        if (views is None) == (intrinsic is None):
            raise ValueError("multiview_sgm: pass either views or intrinsic with T_ref and T_sources")
        if views is None:
            if T_ref is None or T_sources is None:
                raise ValueError("multiview_sgm: intrinsic needs the poses T_ref and T_sources")
            from .prep import plane_sweep_views

            m = plane_sweep_views(intrinsic, T_ref, intrinsic, T_sources)
        else:
            if T_ref is not None or T_sources is not None:
                raise ValueError("multiview_sgm: pass either views or intrinsic with T_ref and T_sources")
            m = np.ascontiguousarray(views.cpu().numpy() if _is_torch(views) else views, dtype=np.float32)
        if m.size != 12 * N or tuple(m.shape[-2:]) != (3, 4):
            raise ValueError(f"multiview_sgm: views must be [{N}, 3, 4], got {tuple(m.shape)}")
        if not np.isfinite(m).all():
            raise ValueError("multiview_sgm: a view matrix entry is not finite")
        prm = L.HvMvsParams(int(num_planes), int(p1), int(p2), int(uniqueness_ratio), int(min_views), int(paths), lo, hi,
                            int(speckle_window_size), int(speckle_range))
        out = self._results({"index": ((H, W), np.int16) if index else None, "depth": ((H, W), np.float32) if depth else None}, on_gpu,
                            pinned=False, synchronize=False)
        with self._ordered(a, b, out["index"], out["depth"]):
            L.check(self._lib.hv_mvs_sgm(self._h, L.ptr(a), L.ptr(b), N, H, W, channels, L.ptr(m), ctypes.byref(prm), L.ptr(out["index"]),
                                         L.ptr(out["depth"]), None, L.location(a)))
        return out["index"], out["depth"]

    def filter_depth_consistency(self, depth, source_depths, views=None, back_views=None, *, intrinsic=None, T_ref=None, T_sources=None,
                                 max_reproj_error=1.0, inv_depth_tol=0.0, rel_depth_tol=0.01, min_consistent=1, max_violations=0, fuse=True,
                                 counts=False, stats=False):
        """The cross-view consistency check of a float32 depth map [H,W] against the depth maps of 1..4 posed neighbours of the same
        shape (hv_depth_consistency, the rules C1 - C7 in include/hipvol.h): a pixel is projected with its depth into each
        neighbour, the neighbour's depth is read there and projected back; the view agrees when the pixel lands within
        max_reproj_error pixels of where it started and its inverse depth within inv_depth_tol + rel_depth_tol / depth of what it
        started with.  A view that has a depth there and does not agree is occluded (it sees something nearer) or violated (it sees
        through the point).  A pixel is kept iff at least min_consistent views agree and at most max_violations are violated.
        -> (depth float32 [H,W]: 0 where a pixel went, the mean of its own and the agreeing views' depths with fuse, its own
        depth without; counts uint8 [H,W,4]: agree, occluded, violated, seen - or None without counts=True) and, with stats=True,
        a ConsistencyStats as a third item (the call then waits for the stream).  source_depths: a list of images or one [N,H,W]
        array.  Pass views and back_views, [N,3,4] float32 each (reference pixel -> source s, pixel of source s -> reference, in
        the convention of multiview_sgm), or intrinsic with the world-to-camera poses T_ref [4,4] and T_sources [N,4,4], which
        prep.consistency_views turns into both.  inv_depth_tol is absolute, in 1 / metres: one plane step for the depth of a
        plane sweep; rel_depth_tol is relative: for metric sensors; one of them must be positive.  numpy arrays in, numpy arrays
        out; torch CUDA tensors on the volume's GPU in, tensors out, queued on the volume's stream.  Works on a volume of any
        mode and reads nothing of it."""
        on_gpu = L.location(depth) == L.HV_DEVICE
        is_list = isinstance(source_depths, (list, tuple))
        src_list = list(source_depths) if is_list else [source_depths]
        if not src_list or any((L.location(s) == L.HV_DEVICE) != on_gpu for s in src_list):
            raise ValueError("filter_depth_consistency: depth and source_depths must live in the same place")
        if on_gpu:
            import torch

            if depth.dtype != torch.float32 or any(s.dtype != torch.float32 for s in src_list):
                raise ValueError("filter_depth_consistency: the depth maps must be float32")
            if any(t.device != self._device() for t in [depth] + src_list):
                raise ValueError(f"filter_depth_consistency: the depth maps must live on the volume's GPU {self._device()}")
            a, stack = depth.contiguous(), torch.stack
        else:
            a = depth.cpu().numpy() if _is_torch(depth) else np.asarray(depth)
            src_list = [s.cpu().numpy() if _is_torch(s) else np.asarray(s) for s in src_list]
            if a.dtype != np.float32 or any(s.dtype != np.float32 for s in src_list):
                raise ValueError("filter_depth_consistency: the depth maps must be float32")
            a, stack = np.ascontiguousarray(a), np.stack
        # a list of maps of the reference's shape becomes one block; an array or tensor must be [N] + that shape already
        want = tuple(a.shape) if is_list else (int(src_list[0].shape[0]),) + tuple(a.shape) if src_list[0].ndim else None
        if a.ndim != 2 or any(tuple(s.shape) != want for s in src_list):
            raise ValueError(f"filter_depth_consistency: the sources must be 1..4 depth maps of the reference's shape {tuple(a.shape)}")
        b = stack(src_list) if is_list else src_list[0].contiguous() if on_gpu else np.ascontiguousarray(src_list[0])
        N, H, W = int(b.shape[0]), int(a.shape[0]), int(a.shape[1])
        # what hv_depth_consistency answers with HV_ERR_INVALID, refused here before anything is allocated
        if H < 1 or W < 1 or H > 32768 or W > 32768 or H * W >= 1 << 30:
            raise ValueError(f"filter_depth_consistency: bad image size {tuple(a.shape)}")
        if not 1 <= N <= 4:
            raise ValueError(f"filter_depth_consistency: need 1..4 source views, got {N}")
        f32_max = float(np.finfo(np.float32).max)  # (the library reads float32)
        if not 0.0 <= float(max_reproj_error) <= f32_max:
            raise ValueError(f"filter_depth_consistency: max_reproj_error must be finite and not negative, got {max_reproj_error}")
        if not (0.0 <= float(inv_depth_tol) <= f32_max and 0.0 <= float(rel_depth_tol) <= f32_max):
            raise ValueError(f"filter_depth_consistency: the depth tolerances must be finite and not negative, got {inv_depth_tol} and {rel_depth_tol}")
        if not (np.float32(inv_depth_tol) > 0 or np.float32(rel_depth_tol) > 0):
            raise ValueError("filter_depth_consistency: one of inv_depth_tol and rel_depth_tol must be positive")
        if int(min_consistent) != min_consistent or not 0 <= int(min_consistent) <= N:
            raise ValueError(f"filter_depth_consistency: min_consistent must be in 0..{N}, got {min_consistent}")
        if int(max_violations) != max_violations or not 0 <= int(max_violations) <= N:
            raise ValueError(f"filter_depth_consistency: max_violations must be in 0..{N}, got {max_violations}")
        if (views is None) != (back_views is None) or (views is None) == (intrinsic is None):
            raise ValueError("filter_depth_consistency: pass either views and back_views or intrinsic with T_ref and T_sources")
        if views is None:
            if T_ref is None or T_sources is None:
                raise ValueError("filter_depth_consistency: intrinsic needs the poses T_ref and T_sources")
            from .prep import consistency_views

            m, mb = consistency_views(intrinsic, T_ref, intrinsic, T_sources)
        else:
            if T_ref is not None or T_sources is not None:
                raise ValueError("filter_depth_consistency: pass either views and back_views or intrinsic with T_ref and T_sources")
            m, mb = (np.ascontiguousarray(x.cpu().numpy() if _is_torch(x) else x, dtype=np.float32) for x in (views, back_views))
        for name, x in (("views", m), ("back_views", mb)):
            if x.size != 12 * N or tuple(x.shape[-2:]) != (3, 4):
                raise ValueError(f"filter_depth_consistency: {name} must be [{N}, 3, 4], got {tuple(x.shape)}")
            if not np.isfinite(x).all():
                raise ValueError("filter_depth_consistency: a view matrix entry is not finite")
        prm = L.HvConsistencyParams(float(max_reproj_error), float(inv_depth_tol), float(rel_depth_tol), int(min_consistent), int(max_violations),
                                    1 if fuse else 0)
        out = self._results({"depth": ((H, W), np.float32), "counts": ((H, W, 4), np.uint8) if counts else None}, on_gpu, pinned=False,
                            synchronize=False)
        st = L.HvConsistencyStats() if stats else None
        with self._ordered(a, b, out["depth"], out["counts"]):
            L.check(self._lib.hv_depth_consistency(self._h, L.ptr(a), L.ptr(b), N, H, W, L.ptr(m), L.ptr(mb), ctypes.byref(prm), L.ptr(out["depth"]),
                                                   L.ptr(out["counts"]), ctypes.byref(st) if stats else None, L.location(a)))
        if stats:
            return out["depth"], out["counts"], _stats(ConsistencyStats, st)
        return out["depth"], out["counts"]

    @staticmethod
    def _odometry_params(depth_scale, depth_min, depth_max, iterations, depth_outlier_trunc, depth_huber_delta, intensity_weight=0.0,
                         intensity_huber_delta=1.0):
        """-> (hv_odometry_params, the iteration counts as ints)"""
        iters = [int(i) for i in iterations]
        prm = L.HvOdometryParams()
        prm.depth_scale, prm.depth_min, prm.depth_max = float(depth_scale), float(depth_min), float(depth_max)
        prm.depth_outlier_trunc, prm.depth_huber_delta = float(depth_outlier_trunc), float(depth_huber_delta)
        prm.intensity_weight, prm.intensity_huber_delta = float(intensity_weight), float(intensity_huber_delta)
        prm.n_levels = len(iters)
        for i, n in enumerate(iters[:L.HV_TRACK_MAX_LEVELS]):
            prm.iterations[i] = n
        return prm, iters

    def rgbd_odometry(self, source_depth, target_depth, intrinsic, init=None, source_color=None, target_color=None, depth_scale=1.0,
                      depth_min=0.1, depth_max=3.0, iterations=(10, 5, 4), depth_outlier_trunc=0.07, depth_huber_delta=0.05,
                      intensity_weight=0.01, intensity_huber_delta=0.1, trace=False):
        """How the camera moved between two RGB-D frames (hv_rgbd_odometry; the place of Open3D's rgbd_odometry_multi_scale): ->
        OdometryResult whose transformation is T_target_source - it maps a point in source-camera coordinates into target-camera
        coordinates; with world poses T_cw(target) @ inv(T_cw(source)).  The volume is context only (its stream and scratch, any
        mode): the map is neither read nor changed.  It is track_frame_to_model's alignment with the model built from the target
        frame instead of the map; parameters and result fields mean what they mean there.
        source_depth, target_depth [H,W]: numpy or torch (either device), uint16 or any real dtype (as float32), divided by
        depth_scale; H, W = intrinsic.height, intrinsic.width.  Both frames must share place, dtype and shape.  init: the 4x4 start
        of T_target_source (None: identity).  source_color and target_color [H,W,3] uint8, both or neither: hybrid (point-to-plane
        plus a photometric term weighted by intensity_weight; 0 is the depth-only result bit for bit) or depth only.  When the
        frames cannot be aligned (empty, or geometry that leaves a motion free and no colour) success is False and transformation
        is init.  CUDA tensors are read after the work queued on torch's current stream.  trace=True: the per-linearisation record."""
        who = "rgbd_odometry"
        if (source_color is None) != (target_color is None):
            raise ValueError(f"{who}: give both source_color and target_color (hybrid) or neither (depth only)")
        hybrid = source_color is not None
        shapes = [tuple(int(s) for s in np.shape(a)) for a in (source_depth, target_depth)]
        if shapes[0] != shapes[1]:
            raise ValueError(f"{who}: source_depth is {shapes[0]}, target_depth is {shapes[1]}: the two frames must have the same shape")
        sd, sc, skind, _ = _tsdf_operands(source_depth, source_color, intrinsic, depth_only=not hybrid)
        td, tc, tkind, _ = _tsdf_operands(target_depth, target_color, intrinsic, depth_only=not hybrid)
        if skind != tkind:
            raise ValueError(f"{who}: source_depth is {sd.dtype}, target_depth is {td.dtype}: the two frames must have the same dtype")
        places = [str(a.device) if L.location(a) == L.HV_DEVICE else "the host" for a in (sd, td)]
        if places[0] != places[1]:
            raise ValueError(f"{who}: source_depth lives on {places[0]}, target_depth on {places[1]}: the two frames must live in the same place")
        T0 = None
        if init is not None:
            T0 = _as_f64_4x4(init)
            if not np.isfinite(T0).all() or not np.array_equal(T0[3], (0.0, 0.0, 0.0, 1.0)):
                raise ValueError(f"{who}: init must be a finite rigid 4x4 with bottom row 0 0 0 1")
        H, W = int(sd.shape[0]), int(sd.shape[1])
        prm, iters = self._odometry_params(depth_scale, depth_min, depth_max, iterations, depth_outlier_trunc, depth_huber_delta,
                                           intensity_weight, intensity_huber_delta)
        res = L.HvOdometryResult()
        intr = intrinsic.as_array()
        steps = max(sum(iters), 1)
        rows = np.zeros((steps, L.HV_TRACK_COLOR_TRACE_STRIDE if hybrid else L.HV_TRACK_TRACE_STRIDE), np.float64) if trace else None
        n_rows = ctypes.c_int64()
        with self._ordered(sd, td, sc, tc):
            L.check(self._lib.hv_rgbd_odometry(self._h, L.ptr(sd), L.ptr(td), skind, L.ptr(sc), L.ptr(tc), H, W, L.ptr(intr), L.ptr(T0),
                                               ctypes.byref(prm), ctypes.byref(res), L.ptr(rows), steps if trace else 0, ctypes.byref(n_rows),
                                               L.location(sd)))
        n_levels = min(len(iters), L.HV_TRACK_MAX_LEVELS)
        return OdometryResult(np.array(res.transformation, np.float64).reshape(4, 4), float(res.fitness), float(res.inlier_rmse),
                              np.array(res.information, np.float64).reshape(6, 6), bool(res.success),
                              tuple(int(res.iterations[i]) for i in range(n_levels)), int(res.degenerate), int(res.inliers),
                              int(res.valid), _trace_rows(rows[:n_rows.value]) if trace else None,
                              int(res.photometric_inliers) if hybrid else None, float(res.intensity_rmse) if hybrid else None)

    def rgbd_odometry_model(self, depth, intrinsic, color=None, level=0, depth_scale=1.0, depth_min=0.1, depth_max=3.0,
                            depth_outlier_trunc=0.07, device=False):
        """The model rgbd_odometry builds from its target frame at pyramid `level` (hv_rgbd_odometry_model): a dict with depth [h,w]
        float32 (metres, 0 = invalid), normal [h,w,3] float32 (camera frame, facing the camera, 0 where the mask is not set), mask
        [h,w] bool and record [h,w,4] float32 {intensity, g_x, g_y, has-gradient} (None without color); h, w = H >> level, W >> level.
        depth and color as rgbd_odometry takes a frame.  device=False: numpy arrays; True: torch CUDA tensors on the volume's GPU,
        ordered before later work on torch's current stream; the operands are moved to that side first."""
        d, c, dkind, _ = _tsdf_operands(depth, color, intrinsic, depth_only=color is None)
        H, W = int(d.shape[0]), int(d.shape[1])
        level = int(level)
        if not 0 <= level < L.HV_TRACK_MAX_LEVELS or min(H >> level, W >> level) < 1:
            raise ValueError(f"rgbd_odometry_model: a {H}x{W} frame has no pyramid level {level}")
        d, dev = self._query_place(d, bool(device))
        if c is not None:
            c, _ = self._query_place(c, bool(device))
        prm, _ = self._odometry_params(depth_scale, depth_min, depth_max, (1,), depth_outlier_trunc, 1.0)
        h, w = H >> level, W >> level
        out = self._results({"depth": ((h, w), np.float32), "normal": ((h, w, 3), np.float32), "mask": ((h, w), np.bool_),
                             "record": None if c is None else ((h, w, 4), np.float32)}, bool(device), pinned=False)
        intr = intrinsic.as_array()
        with self._ordered(d, c):
            L.check(self._lib.hv_rgbd_odometry_model(self._h, L.ptr(d), dkind, L.ptr(c), H, W, L.ptr(intr), ctypes.byref(prm), level,
                                                     L.ptr(out["depth"]), L.ptr(out["normal"]), L.ptr(out["mask"]), L.ptr(out["record"]),
                                                     L.HV_DEVICE if device else L.HV_HOST))
        return out

    def _pose_graph_operands(self, who, poses, edges, transformations, informations, uncertain):
        """The graph's arrays where the call reads them: all on the volume's GPU when `poses` is a CUDA tensor, else all on the host;
        float64 / int32 / uint8, C-contiguous.  -> (poses [N,4,4], edges [E,2], Z [E,4,4], info [E,6,6], uncertain [E] or None, on_gpu, N, E)"""
        on_gpu = L.location(poses) == L.HV_DEVICE
        if on_gpu:
            import torch

            dev = self._device()
            if poses.device != dev:
                raise ValueError(f"{who}: poses live on {poses.device}, the volume on {dev}")

            def place(a, dtype):
                t = a if _is_torch(a) else torch.as_tensor(np.asarray(a))
                return t.to(device=dev, dtype=getattr(torch, dtype)).contiguous()
        else:
            def place(a, dtype):
                return np.ascontiguousarray(a.cpu().numpy() if _is_torch(a) else np.asarray(a), dtype=dtype)

        P = place(poses, "float64")
        if P.ndim != 3 or tuple(P.shape[1:]) != (4, 4) or P.shape[0] < 1:
            raise ValueError(f"{who}: poses must be [N,4,4] with N >= 1, got {tuple(P.shape)}")
        N = int(P.shape[0])
        Ed = place(edges, "int32").reshape(-1, 2)
        E = int(Ed.shape[0])
        Z, Om = place(transformations, "float64"), place(informations, "float64")
        if int(np.prod(Z.shape)) != 16 * E or (E > 0 and tuple(Z.shape[-2:]) != (4, 4)):
            raise ValueError(f"{who}: transformations must be [{E},4,4] for {E} edges, got {tuple(Z.shape)}")
        if int(np.prod(Om.shape)) != 36 * E or (E > 0 and tuple(Om.shape[-2:]) != (6, 6)):
            raise ValueError(f"{who}: informations must be [{E},6,6] for {E} edges, got {tuple(Om.shape)}")
        Z, Om = Z.reshape(E, 4, 4), Om.reshape(E, 6, 6)
        U = None
        if uncertain is not None:
            U = place(uncertain, "bool")
            U = U.to(torch.uint8) if on_gpu else U.astype(np.uint8)
            if tuple(U.shape) != (E,):
                raise ValueError(f"{who}: uncertain must be [{E}], got {tuple(U.shape)}")
        return P, Ed, Z, Om, U, on_gpu, N, E

    def optimize_pose_graph(self, poses, edges, transformations, informations, uncertain=None, fixed=0, line_process_weight=1.0,
                            edge_prune_threshold=0.25, max_iterations=100, lambda_scale=1e-5, gradient_tolerance=1e-6, step_tolerance=1e-6,
                            decrease_tolerance=1e-6, residual_tolerance=1e-6, cg_max_iterations=100, cg_tolerance=1e-8, trace=False):
        """Pose-graph optimisation on the GPU (hv_pose_graph_optimize; the place of Open3D's global_optimization with
        Levenberg-Marquardt and the line process): -> PoseGraphResult.  poses [N,4,4] T_wc (camera-to-world) of the nodes; edges
        [E,2] {source, target}; transformations [E,4,4] T_target_source of each edge - what rgbd_odometry returns for (source,
        target) and register_volume returns as T_self_source; informations [E,6,6], as those calls return them, order (omega, t);
        uncertain [E] bool: loop closures, which the line process may switch off (None: all certain); fixed: the node that does
        not move.  Every node must reach `fixed` through certain edges.  line_process_weight is the chi2 above which an uncertain
        edge is switched off: about (the largest residual still accepted)^2 times the information's diagonal.  The operands are
        not changed.  numpy or torch on either device: with `poses` a CUDA tensor on the volume's GPU everything is read there and
        poses, line_process and kept come back as tensors ordered on torch's current stream; else numpy arrays.  The volume is
        context only (its stream and scratch, any mode): the map is neither read nor changed.  trace=True: one dict per outer
        iteration with the poses it started from."""
        who = "optimize_pose_graph"
        P, Ed, Z, Om, U, on_gpu, N, E = self._pose_graph_operands(who, poses, edges, transformations, informations, uncertain)
        if int(fixed) != fixed or not 0 <= int(fixed) < N:
            raise ValueError(f"{who}: fixed must be a node index in 0..{N - 1}, got {fixed}")
        if not (np.isfinite(line_process_weight) and line_process_weight > 0):
            raise ValueError(f"{who}: line_process_weight must be positive and finite, got {line_process_weight}")
        if not 0.0 <= edge_prune_threshold <= 1.0:
            raise ValueError(f"{who}: edge_prune_threshold must be in 0..1, got {edge_prune_threshold}")
        if not (1 <= int(max_iterations) <= 10000 and 1 <= int(cg_max_iterations) <= 10000):
            raise ValueError(f"{who}: max_iterations and cg_max_iterations must be in 1..10000")
        prm = L.HvPoseGraphParams(float(line_process_weight), float(edge_prune_threshold), float(lambda_scale), float(gradient_tolerance),
                                  float(step_tolerance), float(decrease_tolerance), float(residual_tolerance), float(cg_tolerance),
                                  int(max_iterations), int(cg_max_iterations), int(fixed), 1 if trace else 0)
        out = self._results({"poses": ((N, 4, 4), np.float64), "line_process": ((E,), np.float64)}, on_gpu, pinned=False, synchronize=False)
        if on_gpu:
            out["poses"].copy_(P)
        else:
            out["poses"][...] = P
        cap = int(max_iterations) if trace else 0
        rows = np.zeros((cap, L.HV_POSE_GRAPH_TRACE_STRIDE), np.float64) if trace else None
        states = np.zeros((cap, N, 4, 4), np.float64) if trace else None
        n_rows = ctypes.c_int64()
        res = L.HvPoseGraphResult()
        with self._ordered(P, Ed, Z, Om, U, out["poses"], out["line_process"]):
            L.check(self._lib.hv_pose_graph_optimize(self._h, L.ptr(out["poses"]), N, L.ptr(Ed), L.ptr(Z), L.ptr(Om), L.ptr(U), E, ctypes.byref(prm),
                                                     L.ptr(out["line_process"]), ctypes.byref(res), L.ptr(rows), L.ptr(states), cap,
                                                     ctypes.byref(n_rows), L.location(P)))
        lp = out["line_process"]
        if E == 0:
            lp = lp[:0]
        tr = None
        if trace:
            tr = [dict({name: kind(r[i]) for i, (name, kind) in enumerate(_POSE_GRAPH_TRACE)}, poses=states[k].copy())
                  for k, r in enumerate(rows[:n_rows.value])]
        return PoseGraphResult(out["poses"], lp, lp >= float(edge_prune_threshold), float(res.chi2_initial), float(res.chi2_final),
                               float(res.lambda_), int(res.iterations), int(res.cg_iterations_total), int(res.edges_kept),
                               L.HV_POSE_GRAPH_RULES.get(int(res.converged), str(int(res.converged))), bool(res.success), tr)

    def pose_graph_linearise(self, poses, edges, transformations, informations, uncertain=None, line_process_weight=1.0):
        """One linearisation of optimize_pose_graph at `poses`, for tests (hv_pose_graph_linearise): a dict of numpy arrays r [E,6],
        chi2 [E], l [E], M [E,6,6], g [E,6] per edge and the gradient b [N,6] with no node fixed.  Operands as optimize_pose_graph."""
        who = "pose_graph_linearise"
        P, Ed, Z, Om, U, on_gpu, N, E = self._pose_graph_operands(who, poses, edges, transformations, informations, uncertain)
        if E < 1:
            raise ValueError(f"{who}: the graph has no edge")
        out = {"r": np.zeros((E, 6)), "chi2": np.zeros(E), "l": np.zeros(E), "M": np.zeros((E, 6, 6)), "g": np.zeros((E, 6)), "b": np.zeros((N, 6))}
        with self._ordered(P, Ed, Z, Om, U):
            L.check(self._lib.hv_pose_graph_linearise(self._h, L.ptr(P), N, L.ptr(Ed), L.ptr(Z), L.ptr(Om), L.ptr(U), E, float(line_process_weight),
                                                      L.ptr(out["r"]), L.ptr(out["chi2"]), L.ptr(out["l"]), L.ptr(out["M"]), L.ptr(out["g"]),
                                                      L.ptr(out["b"]), L.location(P)))
        return out

    def _bundle_operands(self, who, cameras, points, observations, measurements, inv_sigma2, active, camera_fixed):
        """The problem's arrays where the call reads them: all on the volume's GPU when `cameras` is a CUDA tensor, else all on the
        host; float64 / int32 / uint8, C-contiguous.  -> (cameras [N,4,4], points [M,3], index [O,2], meas [O,4], active [O] or None,
        fixed [N] or None, on_gpu, N, M, O)"""
        on_gpu = L.location(cameras) == L.HV_DEVICE
        if on_gpu:
            import torch

            dev = self._device()
            if cameras.device != dev:
                raise ValueError(f"{who}: cameras live on {cameras.device}, the volume on {dev}")

            def place(a, dtype):
                t = a if _is_torch(a) else torch.as_tensor(np.asarray(a))
                return t.to(device=dev, dtype=getattr(torch, dtype)).contiguous()
        else:
            def place(a, dtype):
                return np.ascontiguousarray(a.cpu().numpy() if _is_torch(a) else np.asarray(a), dtype=dtype)

        T = place(cameras, "float64")
        if T.ndim != 3 or tuple(T.shape[1:]) != (4, 4):
            raise ValueError(f"{who}: cameras must be [N,4,4], got {tuple(T.shape)}")
        X = place(points, "float64")
        if X.ndim != 2 or X.shape[1] != 3:
            raise ValueError(f"{who}: points must be [M,3], got {tuple(X.shape)}")
        N, M = int(T.shape[0]), int(X.shape[0])
        idx = place(observations, "int32").reshape(-1, 2)
        O = int(idx.shape[0])
        Z = place(measurements, "float64")
        if Z.ndim != 2 or int(Z.shape[0]) != O or int(Z.shape[1]) not in (2, 3):
            raise ValueError(f"{who}: measurements must be [{O},2] (u, v) or [{O},3] (u, v, u_r) for {O} observations, got {tuple(Z.shape)}")
        if np.ndim(inv_sigma2) == 0:
            inv_sigma2 = np.full(O, float(inv_sigma2))
        s2 = place(inv_sigma2, "float64")
        if tuple(s2.shape) != (O,):
            raise ValueError(f"{who}: inv_sigma2 must be a number or [{O}], got {tuple(s2.shape)}")
        if on_gpu:
            meas = torch.full((O, 4), float("nan"), dtype=torch.float64, device=dev)
        else:
            meas = np.full((O, 4), np.nan)
        meas[:, :int(Z.shape[1])] = Z
        meas[:, 3] = s2

        def flags(a, n, name):
            if a is None:
                return None
            f = place(a, "bool")
            f = f.to(torch.uint8) if on_gpu else f.astype(np.uint8)
            if tuple(f.shape) != (n,):
                raise ValueError(f"{who}: {name} must be [{n}], got {tuple(f.shape)}")
            return f

        return T, X, idx, meas, flags(active, O, "active"), flags(camera_fixed, N, "camera_fixed"), on_gpu, N, M, O

    @staticmethod
    def _bundle_params(who, intrinsic, bf, huber, fixed_points, trace, kw):
        prm = L.HvBundleParams()
        names = [n for n, _ in L.HvBundleParams._fields_[5:16]]
        bad = sorted(set(kw) - set(names))
        if bad:
            raise TypeError(f"{who}: unknown parameter {bad[0]} (known: {', '.join(names)})")
        values = dict(huber_delta2_mono=5.991, huber_delta2_stereo=7.815, min_depth=1e-6, lambda_scale=1e-5, gradient_tolerance=1e-6,
                      step_tolerance=1e-6, decrease_tolerance=1e-6, residual_tolerance=1e-6, cg_tolerance=1e-8, max_iterations=100,
                      cg_max_iterations=100)
        values.update(kw)
        if not (1 <= int(values["max_iterations"]) <= 10000 and 1 <= int(values["cg_max_iterations"]) <= 10000):
            raise ValueError(f"{who}: max_iterations and cg_max_iterations must be in 1..10000")
        if not (np.isfinite(bf) and bf > 0):
            raise ValueError(f"{who}: bf must be positive and finite, got {bf}")
        prm.fx, prm.fy, prm.cx, prm.cy, prm.bf = float(intrinsic.fx), float(intrinsic.fy), float(intrinsic.cx), float(intrinsic.cy), float(bf)
        for name, value in values.items():
            setattr(prm, name, int(value) if name.endswith("iterations") else float(value))
        prm.huber, prm.fixed_points, prm.trace_state = int(bool(huber)), int(bool(fixed_points)), int(bool(trace))
        return prm

    def bundle_adjust(self, cameras, points, observations, measurements, intrinsic, bf=1.0, inv_sigma2=1.0, active=None, camera_fixed=None,
                      fixed_points=False, huber=True, trace=False, **params):
        """Bundle adjustment on the GPU (hv_bundle_adjust; the place of the reference's bundle_adjustment, local_bundle_adjustment
        and, with fixed_points, pose_optimization): -> BundleResult.  cameras [N,4,4] T_cw (world to camera, this project's
        extrinsics); points [M,3] in the world; observations [O,2] {camera, point}; measurements [O,2] (u, v) or [O,3] (u, v, u_r),
        a u_r that is not finite marking a monocular observation; intrinsic: fx, fy, cx, cy of the one pinhole; bf = baseline x
        fx; inv_sigma2: a number or [O], 4^-level for a keypoint of this project's pyramid; active [O] bool (None: all);
        camera_fixed [N] bool (None: none; with free points one camera must be fixed); huber: the robust kernel.  **params: the
        remaining fields of hv_bundle_params (max_iterations, cg_tolerance, huber_delta2_mono, ...).  The operands are not changed.
        numpy or torch on either device: with `cameras` a CUDA tensor on the volume's GPU everything is read there and the arrays
        come back as tensors ordered on torch's current stream; else numpy arrays.  The volume is context only (any mode): the map
        is neither read nor changed.  trace=True: one dict per outer iteration with the state it started from."""
        who = "bundle_adjust"
        T, X, idx, meas, act, fix, on_gpu, N, M, O = self._bundle_operands(who, cameras, points, observations, measurements, inv_sigma2, active,
                                                                           camera_fixed)
        prm = self._bundle_params(who, intrinsic, bf, huber, fixed_points, trace, params)
        out = self._results({"cameras": ((N, 4, 4), np.float64), "points": ((M, 3), np.float64), "chi2": ((O,), np.float64),
                             "behind": ((O,), np.uint8)}, on_gpu, pinned=False, synchronize=False)
        if on_gpu:
            out["cameras"].copy_(T), out["points"].copy_(X), out["chi2"].zero_(), out["behind"].zero_()
        else:
            out["cameras"][...], out["points"][...], out["chi2"][...], out["behind"][...] = T, X, 0.0, 0
        cap = int(prm.max_iterations) if trace else 0
        rows = np.zeros((cap, L.HV_POSE_GRAPH_TRACE_STRIDE), np.float64) if trace else None
        tc, tp = (np.zeros((cap, N, 4, 4), np.float64), np.zeros((cap, M, 3), np.float64)) if trace else (None, None)
        n_rows = ctypes.c_int64()
        res = L.HvBundleResult()
        with self._ordered(T, X, idx, meas, act, fix, out["cameras"], out["points"], out["chi2"], out["behind"]):
            L.check(self._lib.hv_bundle_adjust(self._h, L.ptr(out["cameras"]), N, L.ptr(out["points"]), M, L.ptr(fix), L.ptr(idx), L.ptr(meas),
                                               L.ptr(act), O, ctypes.byref(prm), L.ptr(out["chi2"]), L.ptr(out["behind"]), ctypes.byref(res),
                                               L.ptr(rows), L.ptr(tc), L.ptr(tp), cap, ctypes.byref(n_rows), L.location(T)))
        chi2, behind = out["chi2"], out["behind"] != 0
        stereo = meas[:, 2] == meas[:, 2]
        stereo = stereo & (abs(meas[:, 2]) != float("inf"))
        gate = stereo * float(prm.huber_delta2_stereo) + ~stereo * float(prm.huber_delta2_mono)
        inlier = (chi2 <= gate) & ~behind
        if act is not None:
            inlier = inlier & (act != 0)
        tr = None
        if trace:
            tr = [dict({name: kind(r[i]) for i, (name, kind) in enumerate(_POSE_GRAPH_TRACE)}, cameras=tc[k].copy(), points=tp[k].copy())
                  for k, r in enumerate(rows[:n_rows.value])]
        return BundleResult(out["cameras"], out["points"], chi2, behind, inlier, float(res.chi2_initial), float(res.chi2_final), float(res.lambda_),
                            int(res.iterations), int(res.cg_iterations_total), L.HV_POSE_GRAPH_RULES.get(int(res.converged), str(int(res.converged))),
                            bool(res.success), tr)

    def bundle_linearise(self, cameras, points, observations, measurements, intrinsic, bf=1.0, inv_sigma2=1.0, active=None, huber=True, **params):
        """One linearisation of bundle_adjust at the given state, for tests (hv_bundle_linearise): a dict of numpy arrays r [O,3],
        chi2 [O], w [O], behind [O] bool per observation, B [N,6,6] and bc [N,6] per camera (none fixed), C [M,3,3] and bp [M,3] per
        point, and F.  Operands as bundle_adjust."""
        who = "bundle_linearise"
        T, X, idx, meas, act, _, on_gpu, N, M, O = self._bundle_operands(who, cameras, points, observations, measurements, inv_sigma2, active, None)
        if min(N, M, O) < 1:
            raise ValueError(f"{who}: needs a camera, a point and an observation, got {N}, {M}, {O}")
        prm = self._bundle_params(who, intrinsic, bf, huber, False, False, params)
        out = {"r": np.zeros((O, 3)), "chi2": np.zeros(O), "w": np.zeros(O), "behind": np.zeros(O, np.uint8), "B": np.zeros((N, 6, 6)),
               "bc": np.zeros((N, 6)), "C": np.zeros((M, 3, 3)), "bp": np.zeros((M, 3)), "F": np.zeros(1)}
        with self._ordered(T, X, idx, meas, act):
            L.check(self._lib.hv_bundle_linearise(self._h, L.ptr(T), N, L.ptr(X), M, L.ptr(idx), L.ptr(meas), L.ptr(act), O, ctypes.byref(prm),
                                                  L.ptr(out["r"]), L.ptr(out["chi2"]), L.ptr(out["w"]), L.ptr(out["behind"]), L.ptr(out["B"]),
                                                  L.ptr(out["bc"]), L.ptr(out["C"]), L.ptr(out["bp"]), L.ptr(out["F"]), L.location(T)))
        out["behind"] = out["behind"] != 0
        out["F"] = float(out["F"][0])
        return out

    def remap(self, img, map_x, map_y, linear=False):
        """cv2.remap(img, map_x, map_y, INTER_LINEAR if linear else INTER_NEAREST) on the GPU; the maps are [H, W] like the image.
        Host arrays, or a torch CUDA tensor: the image never leaves the device, and maps that are float32 CUDA tensors are read
        where they lie (prep.RectifyMaps keeps such a pair across frames); host maps are uploaded by this call.  The result depends
        on this call's arguments alone: nothing is cached here."""
        if _is_torch(img) and img.is_cuda:
            import torch

            src = img.contiguous()
            kind = {torch.uint8: 0, torch.float32: 1, torch.int32: 2}.get(src.dtype)
            if kind is None:
                raise RuntimeError(f"remap: unsupported image dtype {src.dtype}")
            H, W = int(src.shape[0]), int(src.shape[1])
            _check_map_shapes(map_x, map_y, H, W)
            mx, my = (m.to(device=src.device, dtype=torch.float32).contiguous() for m in
                      (m if _is_torch(m) else torch.tensor(np.asarray(m, dtype=np.float32)) for m in (map_x, map_y)))
            C = 1 if src.dim() == 2 else int(src.shape[2])
            out = torch.empty_like(src)
            torch.cuda.current_stream(src.device).synchronize()  # producers ran on torch's stream, hv_remap on the volume's
            L.check(self._lib.hv_remap(self._h, L.ptr(src), kind, C, H, W, L.ptr(mx), L.ptr(my), 1 if linear else 0, L.ptr(out),
                                       L.HV_DEVICE))
            self.synchronize()
            return out
        img = np.ascontiguousarray(img)
        kind = {np.dtype(np.uint8): 0, np.dtype(np.float32): 1, np.dtype(np.int32): 2}.get(img.dtype)
        if kind is None:
            raise RuntimeError(f"remap: unsupported image dtype {img.dtype}")
        H, W = img.shape[:2]
        C = 1 if img.ndim == 2 else img.shape[2]
        _check_map_shapes(map_x, map_y, H, W)
        mx = np.ascontiguousarray(map_x, dtype=np.float32)
        my = np.ascontiguousarray(map_y, dtype=np.float32)
        out = np.empty_like(img)
        L.check(self._lib.hv_remap(self._h, L.ptr(img), kind, C, H, W, L.ptr(mx), L.ptr(my), 1 if linear else 0, L.ptr(out), L.HV_HOST))
        return out

    # -- packed maps: what ScalableTSDFVolume and the block grids share (the class names its C ABI in _PACKED) ----------------------
    _PACKED = None  # (function prefix, info struct, header struct, stats class, header fields)

    def _pack(self, device):
        prefix, Info, _, Stats, _ = self._PACKED
        info = Info()
        L.check(getattr(self._lib, prefix + "pack_size")(self._h, ctypes.byref(info)))
        out = self._results({"map": ((info.bytes,), np.uint8)}, device, synchronize=False)["map"]
        with self._ordered(out):
            L.check(getattr(self._lib, prefix + "pack")(self._h, L.ptr(out), info.bytes, L.location(out), ctypes.byref(info)))
        return out, _stats(Stats, info)

    def _unpack(self, buf):
        prefix, Info, _, Stats, _ = self._PACKED
        op = _packed_operand(buf)
        info = Info()
        with self._ordered(op):
            L.check(getattr(self._lib, prefix + "unpack")(self._h, L.ptr(op), int(op.numel() if _is_torch(op) else op.size), L.location(op),
                                                          ctypes.byref(info)))
        return _stats(Stats, info)

    def _save(self, path):
        import os
        import tempfile

        buf, stats = self._pack(False)
        path = os.fspath(path)
        fd, tmp = tempfile.mkstemp(prefix=os.path.basename(path) + ".", suffix=".tmp", dir=os.path.dirname(os.path.abspath(path)))
        try:
            with os.fdopen(fd, "wb") as f:
                f.write(memoryview(buf))
            os.replace(tmp, path)
        except BaseException:
            if os.path.exists(tmp):
                os.unlink(tmp)
            raise
        return stats

    @staticmethod
    def _read_packed(path):
        import os

        size = os.path.getsize(path)
        buf = _result_array((size,), np.uint8)  # page-locked when large: the upload is one DMA
        with open(path, "rb") as f:
            got = f.readinto(memoryview(buf))
        if got != size:
            raise ValueError(f"{path}: read {got} of {size} bytes")
        return buf

    def bytes_per_block(self):
        return self._int64(self._lib.hv_bytes_per_block)


class _BlockGrid(_Volume):
    """What VoxelBlockGrid and the semantic block grids share: a grid of voxel_size with block_size^3 voxels per block."""

    def __init__(self, mode, voxel_size, block_size, device, max_blocks, max_points):
        voxel_size = float(np.float32(voxel_size))  # pybind narrows to float (py::init<float,int>)
        super().__init__(mode, voxel_size, 0.0, block_size, 1, device, max_blocks, max_points)
        self.voxel_size = voxel_size
        self.block_size = int(block_size)

    def set_owner(self, rank, world_size):
        """Multi-GPU block ownership (hv_set_owner): fuse and store only the blocks with hash(block key) % world_size == rank (no
        collective while fusing)."""
        L.check(self._lib.hv_set_owner(self._h, int(rank), int(world_size)))

    def carve(self, camera_frustrum, depth_image, depth_threshold=1e-2):
        """carve(camera_frustrum, depth f32 HxW, threshold) of every grid type (voxel_grid_carving.h:47-79).  Host array or
        torch CUDA tensor (used in place, ordered against torch's stream)."""
        f = camera_frustrum
        if _is_torch(depth_image):
            depth = depth_image.contiguous().float()
        else:
            depth = np.ascontiguousarray(depth_image, dtype=np.float32)
        if depth.ndim != 2 or depth.shape[0] * depth.shape[1] == 0 or depth.shape[0] != f.height or depth.shape[1] != f.width:
            return  # "Depth image is empty" / check_image_size(): the reference prints a message and returns
        with self._ordered(depth):
            L.check(self._lib.hv_carve(self._h, L.ptr(f.intr), f.width, f.height, L.ptr(f.T_cw), f.depth_max, f.depth_min, L.ptr(depth),
                                       float(depth_threshold), L.location(depth)))

    def remove_low_count_voxels(self, min_count):
        L.check(self._lib.hv_remove_low_count_voxels(self._h, int(min_count)))

    _HAS_LABELS = False  # the semantic grids: lookup_points fills class_id, object_id and confidence

    def lookup_points(self, points, min_count=1, min_confidence=0.0, radius=0, stats=False, device=None):
        """What the grid holds at `points` [n,3] (float32 or float64; numpy or torch, either device): -> VoxelLookup.  A point's own
        voxel is the one integrate() would put it in (float32 points keyed in float32, float64 in float64); it is the answer
        (LOOKUP_OWN) when it qualifies - its block exists, count >= max(min_count, 1) and, on the semantic grids, confidence >=
        min_confidence: exactly the voxels get_voxels(min_count, min_confidence) lists.  Otherwise, with radius 1 or 2, the qualifying
        voxel of the (2 radius + 1)^3 around it whose mean position is nearest the point (LOOKUP_NEAR), else LOOKUP_MISSING; a point
        that has no voxel (not finite, out of the key range) is LOOKUP_INVALID (include/hipvol.h, hv_lookup_points).  Reads the grid
        only.  stats=True also counts the statuses (LookupStats) and waits for the GPU.  device as ScalableTSDFVolume.sample_points:
        None gives results where the input lives - a torch CUDA tensor gives torch CUDA tensors, queued behind torch's current stream
        and ordered before its later work; True / False: torch CUDA tensors on the grid's GPU / numpy arrays."""
        if _is_torch(points):
            import torch

            if points.dtype not in (torch.float32, torch.float64):
                raise ValueError(f"lookup_points: points must be float32 or float64, got {points.dtype}")
            p = points.contiguous()
        else:
            p = np.asarray(points)
            if p.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
                raise ValueError(f"lookup_points: points must be float32 or float64, got {p.dtype}")
            p = np.ascontiguousarray(p)
        if len(p.shape) != 2 or int(p.shape[1]) != 3:
            raise ValueError(f"lookup_points: points must have shape [n, 3], got {tuple(p.shape)}")
        p, dev = self._query_place(p, device)
        n = int(p.shape[0])
        f64 = str(p.dtype).endswith("float64")
        i32, f32 = np.int32, np.float32
        lab = self._HAS_LABELS
        out = self._results({"status": ((n,), np.uint8), "count": ((n,), i32), "position": ((n, 3), np.float64), "color": ((n, 3), f32),
                             "class_id": ((n,), i32) if lab else None, "object_id": ((n,), i32) if lab else None,
                             "confidence": ((n,), f32) if lab else None}, dev is not None, pinned=False, synchronize=False)
        prm = L.HvLookupParams(int(min_count), float(min_confidence), int(radius))
        st = L.HvLookupStats() if stats else None
        with self._ordered(p):
            L.check(self._lib.hv_lookup_points(self._h, L.ptr(p), L.HV_F64 if f64 else L.HV_F32, n, ctypes.byref(prm), L.ptr(out["status"]),
                                               L.ptr(out["count"]), L.ptr(out["position"]), L.ptr(out["color"]), L.ptr(out["class_id"]),
                                               L.ptr(out["object_id"]), L.ptr(out["confidence"]), ctypes.byref(st) if stats else None,
                                               L.HV_DEVICE if dev is not None else L.HV_HOST))
        return VoxelLookup(out["status"], out["count"], out["position"], out["color"], out["class_id"], out["object_id"], out["confidence"],
                           LookupStats(st.points, st.own, st.near, st.missing, st.invalid) if stats else None)

    def clear(self):
        L.check(self._lib.hv_reset(self._h))

    reset = clear

    # -- packed grids: keeping and moving a map (include/hipvol.h "Packed grids"; hv_grid_pack.hip) ---------------------------------
    _PACKED = ("hv_grid_", L.HvGridPackInfo, L.HvGridPackedHeader, GridPackStats,
               ("voxel_size", "mode", "block_size", "record_bytes", "version", "next_object_id", "depth_threshold", "depth_decay_rate",
                "blocks", "voxels", "extra_pairs", "bytes", "chain_nodes"))
    _MODE = None  # the HV_MODE_* value of the concrete grid class
    _NODES_PER_BLOCK, _MIN_NODES = 4, 1 << 16  # the overflow-node pool hv_create gives a probabilistic grid
    _ALIAS_BLOCK_SIZE = None  # the direct-hash aliases: the block size their constructors fix

    @classmethod
    def _load_blocks(cls, hdr, max_blocks=None):
        """The pool load() asks for: max_blocks or max(1024, 2 * blocks), raised to ceil(chain_nodes / 4) when the node pool that
        comes with it (4 nodes per block, at least 65536) would not hold the map's chains."""
        blocks = int(max_blocks or max(1024, 2 * hdr["blocks"]))
        if hdr["chain_nodes"] > max(cls._MIN_NODES, cls._NODES_PER_BLOCK * blocks):
            blocks = -(-hdr["chain_nodes"] // cls._NODES_PER_BLOCK)
        return blocks

    def pack(self, device=False):
        """The whole grid as one packed buffer, bit for bit (include/hipvol.h "Packed grids"): every allocated block, of each the
        voxels that hold anything - counts, position and colour sums, ids, both confidence counters, the label maps in insertion
        order - and the process's next object id.  -> 1-D uint8, a numpy array, or with device=True a torch CUDA tensor on the
        grid's GPU (nothing crosses PCIe).  Only reads the grid; waits for the GPU.  Pool size, owner settings, association
        scratch, dropped_points() and label_overflows() are not part of a map."""
        return self._pack(device)[0]

    def unpack(self, buf):
        """Fill this EMPTY grid (num_blocks() == 0; same class, block_size and voxel_size, bit for bit) from a packed buffer: numpy,
        bytes-like or a torch uint8 tensor on either device.  The buffer is validated before a kernel writes anything; a corrupt or
        foreign buffer, a non-empty or owner-sharded grid, a pool that cannot hold the map raise HipVolError with the library's
        message and leave the grid unchanged.  Afterwards the grid holds the map that was packed, bit for bit, and every call
        that is a function of the map answers as before; the POOL order is not part of a map (blocks are claimed in key order),
        so what depends on it may differ: the row order of get_voxels(), and the class id of an object segment whose voxels
        carry several classes (it is that of the segment's first voxel in pool order).  The
        process's next object id is raised to the map's if it was lower.  The grid keeps its own depth threshold and decay rate
        (load() applies the map's).  Waits for the GPU and returns GridPackStats."""
        keep = getattr(self, "_keep_unread_map", None)  # (semantic grids: the id map of an association before a clear())
        if keep is not None:
            keep()
        return self._unpack(buf)

    def save(self, path):
        """pack() into the file `path`: written to a temporary file in the same directory, then moved into place (os.replace), so
        a reader never sees half a map.  -> GridPackStats."""
        return self._save(path)

    @classmethod
    def load(cls, path, device=0, max_blocks=None, max_points=None):
        """A new grid of this class holding the map save() wrote to `path`: voxel_size and block_size from the file's header, the
        pool sized max_blocks or max(1024, 2 * blocks) - and large enough that the overflow-node pool (4 nodes per block, at least
        65536) holds the map's chains; an explicit max_blocks that is too small for them is raised as well (_load_blocks) - and the
        header's depth threshold and decay rate applied.  The grid is made by the class's own constructor.  ValueError when the
        file holds a grid of another mode than this class's, or a block_size a direct-hash alias does not have."""
        buf = cls._read_packed(path)
        hdr = cls.packed_info(buf)
        if cls._MODE is None or hdr["mode"] != cls._MODE:
            raise ValueError(f"{path}: a packed grid of mode {hdr['mode']} cannot be loaded as {cls.__name__} (mode {cls._MODE})")
        kw = dict(device=device, max_blocks=cls._load_blocks(hdr, max_blocks), max_points=max_points)
        if cls._ALIAS_BLOCK_SIZE is None:
            vol = cls(hdr["voxel_size"], hdr["block_size"], **kw)
        elif hdr["block_size"] == cls._ALIAS_BLOCK_SIZE:
            vol = cls(hdr["voxel_size"], **kw)
        else:
            raise ValueError(f"{path}: a packed grid of block_size {hdr['block_size']} cannot be loaded as {cls.__name__}, whose "
                             f"blocks have {cls._ALIAS_BLOCK_SIZE}^3 voxels")
        if hdr["mode"] != L.HV_MODE_VOXEL_GRID:
            vol.set_depth_threshold(hdr["depth_threshold"])
            vol.set_depth_decay_rate(hdr["depth_decay_rate"])
        vol.unpack(buf)
        return vol

    @staticmethod
    def packed_info(path_or_buffer):
        """The header of a packed grid - {voxel_size, mode, block_size, record_bytes, version, next_object_id, depth_threshold,
        depth_decay_rate, blocks, voxels, extra_pairs, bytes, chain_nodes} - after the library's validator (hv_grid_packed_check)
        has passed the WHOLE buffer: a file path, or a buffer as unpack() takes it.  Needs no GPU.  ValueError with the validator's
        message, which names the first rule that failed."""
        return _packed_info(_BlockGrid._PACKED, path_or_buffer)

    def size(self):
        return self._int64(self._lib.hv_size)

    get_total_voxel_count = size

    def empty(self):
        return self.num_blocks() == 0

    def get_block_size(self):
        return self.block_size


# ================================================================================================
# `volumetric` module mirror
# ================================================================================================
class BoundingBox3D:
    """Axis-aligned box: cpp/volumetric/bounding_boxes_3d.h:39-80, bounding_boxes_3d.cpp:174-247, bindings
    bounding_boxes_module.h:49-93.  BoundingBox3D(), BoundingBox3D(min_point, max_point) or the six scalars."""

    def __init__(self, *args):
        if len(args) == 0:
            vals = (0.0,) * 6
        elif len(args) == 2:
            vals = tuple(float(x) for x in args[0]) + tuple(float(x) for x in args[1])
        elif len(args) == 6:
            vals = tuple(float(x) for x in args)
        else:
            raise TypeError("BoundingBox3D(), BoundingBox3D(min_point, max_point) or BoundingBox3D(min_x, min_y, min_z, max_x, max_y, max_z)")
        self.min_x, self.min_y, self.min_z, self.max_x, self.max_y, self.max_z = vals

    def as_array(self):
        return np.array([self.min_x, self.min_y, self.min_z, self.max_x, self.max_y, self.max_z], np.float64)

    def get_min_point(self):
        return np.array([self.min_x, self.min_y, self.min_z], np.float64)

    def get_max_point(self):
        return np.array([self.max_x, self.max_y, self.max_z], np.float64)

    def get_center(self):
        return (self.get_min_point() + self.get_max_point()) / 2.0

    def get_size(self):
        return self.get_max_point() - self.get_min_point()

    def get_volume(self):
        sx, sy, sz = self.get_size()
        return float(sx * sy * sz)

    def get_surface_area(self):
        sx, sy, sz = self.get_size()
        return float(2.0 * (sx * sy + sx * sz + sy * sz))

    def get_diagonal_length(self):
        sx, sy, sz = self.get_size()
        return float(np.sqrt(sx * sx + sy * sy + sz * sz))

    def contains(self, points):
        """One point [3] -> bool; several [N,3] -> list of bool (the binding's two overloads).  Closed box."""
        p = np.asarray(points, np.float64)
        m = np.all((p >= self.get_min_point()) & (p <= self.get_max_point()), axis=-1)
        return bool(m) if p.ndim == 1 else [bool(x) for x in m]

    def intersects(self, other):
        return bool(np.all((self.get_min_point() <= other.get_max_point()) & (self.get_max_point() >= other.get_min_point())))

    @staticmethod
    def compute_from_points(points):
        p = np.asarray(points, np.float64).reshape(-1, 3)
        if len(p) == 0:
            return BoundingBox3D()
        return BoundingBox3D(p.min(axis=0), p.max(axis=0))


class ImagePoint:
    """``volumetric.ImagePoint`` (camera_frustrum.h:31-35, camera_frustrum_module.h:41-47): pixel coordinates and depth as float32."""

    def __init__(self, u=0.0, v=0.0, depth=0.0):
        self.u, self.v, self.depth = float(np.float32(u)), float(np.float32(v)), float(np.float32(depth))

    def __repr__(self):
        return f"ImagePoint(u={self.u}, v={self.v}, depth={self.depth})"


class Quaterniond:
    """``volumetric.Quaterniond`` (eigen_module.h:36-96): Eigen::Quaterniond as the module exposes it - Quaterniond() identity,
    Quaterniond(w, x, y, z), Quaterniond([w, x, y, z]); w() x() y() z(), coeffs() -> [w, x, y, z], normalized(), normalize(),
    conjugate(), inverse(), toRotationMatrix(); picklable."""

    def __init__(self, *args):
        if len(args) == 0:
            c = (1.0, 0.0, 0.0, 0.0)
        elif len(args) == 4:
            c = args
        elif len(args) == 1 and np.size(args[0]) == 4:
            c = np.asarray(args[0], np.float64).reshape(4)
        else:
            raise RuntimeError("Quaternion array must have exactly 4 elements [w, x, y, z]")
        self._c = np.array([float(v) for v in c], np.float64)  # w, x, y, z

    def w(self):
        return float(self._c[0])

    def x(self):
        return float(self._c[1])

    def y(self):
        return float(self._c[2])

    def z(self):
        return float(self._c[3])

    def coeffs(self):
        return self._c.copy()

    def normalized(self):
        return Quaterniond(self._c / np.sqrt(np.sum(self._c * self._c)))

    def normalize(self):
        self._c = self._c / np.sqrt(np.sum(self._c * self._c))

    def conjugate(self):
        return Quaterniond(self._c[0], -self._c[1], -self._c[2], -self._c[3])

    def inverse(self):
        n2 = float(np.sum(self._c * self._c))
        return Quaterniond(self.conjugate()._c / n2) if n2 > 0.0 else Quaterniond(0.0, 0.0, 0.0, 0.0)

    def toRotationMatrix(self):
        w, x, y, z = self._c  # (Eigen does not normalise here)
        tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
        twx, twy, twz = tx * w, ty * w, tz * w
        txx, txy, txz = tx * x, ty * x, tz * x
        tyy, tyz, tzz = ty * y, tz * y, tz * z
        return np.array([[1.0 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1.0 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1.0 - (txx + tyy)]])

    def __repr__(self):
        return "Quaterniond(w=%f, x=%f, y=%f, z=%f)" % tuple(self._c)

    def __reduce__(self):
        return (Quaterniond, tuple(float(v) for v in self._c))


def _quat_from_matrix(m):
    """Eigen::Quaterniond(Matrix3d) (Eigen/src/Geometry/Quaternion.h, quaternionbase_assign_impl<Other, 3, 3>) -> (w, x, y, z)."""
    t = m[0, 0] + m[1, 1] + m[2, 2]
    q = np.zeros(4, np.float64)  # x, y, z, w
    if t > 0.0:
        t = np.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0], q[1], q[2] = (m[2, 1] - m[1, 2]) * t, (m[0, 2] - m[2, 0]) * t, (m[1, 0] - m[0, 1]) * t
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (m[k, j] - m[j, k]) * t
        q[j] = (m[j, i] + m[i, j]) * t
        q[k] = (m[k, i] + m[i, k]) * t
    return np.array([q[3], q[0], q[1], q[2]])


def _matrix_from_quat(wxyz):
    """Eigen::Quaterniond::normalized().toRotationMatrix()."""
    w, x, y, z = np.asarray(wxyz, np.float64) / np.sqrt(np.sum(np.asarray(wxyz, np.float64) ** 2))
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1.0 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1.0 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1.0 - (txx + tyy)]])


def _mat3_vec(R, v):
    """R v in Eigen's coefficient order ((r0 v0 + r1 v1) + r2 v2 per row): the same float64 bits as the reference's products."""
    return R[:, 0] * v[0] + R[:, 1] * v[1] + R[:, 2] * v[2]


class CameraFrustrum:
    """``volumetric.CameraFrustrum`` (cpp/volumetric/camera_frustrum.h:37-130, camera_frustrum.cpp, bindings camera_frustrum_module.h:50-130).
    The binding's three constructors: ``CameraFrustrum(fx, fy, cx, cy, width, height, T_cw, depth_max, depth_min)``,
    ``CameraFrustrum(K, width, height, T_cw, depth_max, depth_min)`` and ``CameraFrustrum(fx, fy, cx, cy, width, height, orientation,
    translation, depth_max, depth_min)`` (orientation: quaternion (w, x, y, z) or an object with .w() .. .z()); keywords as there.
    Intrinsics and depth limits are float32 members, the pose float64.  Corners, boxes and the point tests are the host-side
    geometry of the reference class; the grids take the frustum as a query (hv_query.h)."""

    def __init__(self, *args, **kw):
        names9 = ("fx", "fy", "cx", "cy", "width", "height", "T_cw", "depth_max", "depth_min")
        names6 = ("K", "width", "height", "T_cw", "depth_max", "depth_min")
        names10 = ("fx", "fy", "cx", "cy", "width", "height", "orientation", "translation", "depth_max", "depth_min")
        if "K" in kw or (args and np.ndim(args[0]) == 2):
            a = dict(zip(names6, args), **kw)
            K = np.asarray(a["K"], np.float64)
            a.update(fx=K[0, 0], fy=K[1, 1], cx=K[0, 2], cy=K[1, 2])
        elif "orientation" in kw or len(args) == 10:
            a = dict(zip(names10, args), **kw)
        else:
            a = dict(zip(names9, args), **kw)
        self.intr = np.array([a["fx"], a["fy"], a["cx"], a["cy"]], dtype=np.float32)
        self.width = int(a["width"])
        self.height = int(a["height"])
        self.depth_max = float(np.float32(a.get("depth_max", 10.0)))
        self.depth_min = float(np.float32(a.get("depth_min", 1e-2)))
        self._cache = None
        if "orientation" in a:
            self.set_T_cw(a["orientation"], a["translation"])
        else:
            self.set_T_cw(np.eye(4) if a.get("T_cw") is None else a["T_cw"])

    # ---- setters (each drops the cached corners / boxes, camera_frustrum.cpp:64-121) ----
    def set_T_cw(self, T_cw, translation=None):
        """set_T_cw(T_cw 4x4) or set_T_cw(orientation, translation)."""
        if translation is not None:
            q = T_cw
            wxyz = np.array([q.w(), q.x(), q.y(), q.z()], np.float64) if hasattr(q, "w") and callable(q.w) else np.asarray(q, np.float64)
            T = np.eye(4)
            T[:3, :3] = _matrix_from_quat(wxyz)
            T[:3, 3] = np.asarray(translation, np.float64)
            T_cw = T
        self.T_cw = _as_f64_4x4(T_cw)
        self._cache = None

    def set_width(self, width):
        self.width = int(width)
        self._cache = None

    def set_height(self, height):
        self.height = int(height)
        self._cache = None

    def set_depth_max(self, depth_max):
        self.depth_max = float(np.float32(depth_max))
        self._cache = None

    def set_depth_min(self, depth_min):
        self.depth_min = float(np.float32(depth_min))
        self._cache = None

    def set_intrinsics(self, *args, **kw):
        """set_intrinsics(K) or set_intrinsics(fx, fy, cx, cy)."""
        if "K" in kw or len(args) == 1:
            K = np.asarray(kw.get("K", args[0] if args else None), np.float64)
            vals = (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
        else:
            vals = tuple(dict(zip(("fx", "fy", "cx", "cy"), args), **kw)[k] for k in ("fx", "fy", "cx", "cy"))
        self.intr = np.array(vals, dtype=np.float32)
        self._cache = None

    # ---- getters ----
    def get_width(self):
        return self.width

    def get_height(self):
        return self.height

    def get_fx(self):
        return float(self.intr[0])

    def get_fy(self):
        return float(self.intr[1])

    def get_cx(self):
        return float(self.intr[2])

    def get_cy(self):
        return float(self.intr[3])

    def get_K(self):
        fx, fy, cx, cy = (float(x) for x in self.intr)
        return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])

    def get_T_cw(self):
        T = np.eye(4)
        T[:3, :] = self.T_cw[:3, :]
        return T

    def get_R_cw(self):
        return self.T_cw[:3, :3].copy()

    def get_t_cw(self):
        return self.T_cw[:3, 3].copy()

    def get_orientation_cw(self):
        """-> Quaterniond of R_cw (Eigen::Quaterniond(R_cw_), camera_frustrum.cpp:152-154)."""
        return Quaterniond(_quat_from_matrix(self.T_cw[:3, :3]))

    def is_cache_valid(self):
        return self._cache is not None

    def _update_cache(self):
        if self._cache is not None:
            return self._cache
        fx, fy, cx, cy = (float(x) for x in self.intr)
        R_cw, t_cw = self.T_cw[:3, :3], self.T_cw[:3, 3]
        R_wc = R_cw.T
        t_wc = _mat3_vec(-R_wc, t_cw)
        corners = []  # camera_frustrum.cpp:209-245: near and far point of top-left, top-right, bottom-right, bottom-left
        for u, v in ((0.0, 0.0), (float(self.width), 0.0), (float(self.width), float(self.height)), (0.0, float(self.height))):
            xn, yn = (u - cx) / fx, (v - cy) / fy
            for d in (self.depth_min, self.depth_max):
                corners.append(_mat3_vec(R_wc, np.array([xn * d, yn * d, d])) + t_wc)
        corners = np.array(corners)
        bbox = BoundingBox3D(corners.min(axis=0), corners.max(axis=0))  # :247-264
        cam = np.array([_mat3_vec(R_cw, c) + t_cw for c in corners])  # :266-301: the box of the corners in the camera frame
        lo, hi = cam.min(axis=0), cam.max(axis=0)
        center_w = _mat3_vec(R_wc, (lo + hi) / 2.0) + t_wc
        self._cache = (corners, bbox, (center_w, _quat_from_matrix(R_wc), hi - lo))
        return self._cache

    def get_corners(self):
        return [c.copy() for c in self._update_cache()[0]]

    def get_bbox(self):
        return self._update_cache()[1]

    def get_obb(self):
        from .volumetric_semantic import OrientedBoundingBox3D

        return OrientedBoundingBox3D(*self._update_cache()[2])

    def is_in_bbox(self, point_w):
        return self.get_bbox().contains(np.asarray(point_w, np.float64))

    def is_in_obb(self, point_w):
        return self.get_obb().contains(np.asarray(point_w, np.float64))

    def contains(self, point_w):
        """-> (inside, ImagePoint): camera_frustrum.cpp:175-196 (the depth test first - ImagePoint(-1, -1, -1) when it fails -, then
        the projection in float64 narrowed to float32 pixel coordinates, then the image bounds)."""
        p = np.asarray(point_w, np.float64)
        pc = _mat3_vec(self.T_cw[:3, :3], p) + self.T_cw[:3, 3]
        depth = np.float32(pc[2])
        if not (depth >= np.float32(self.depth_min) and depth <= np.float32(self.depth_max)):
            return False, ImagePoint(-1.0, -1.0, -1.0)
        fx, fy, cx, cy = (float(x) for x in self.intr)
        with np.errstate(divide="ignore", invalid="ignore"):
            u = np.float32(fx * (pc[0] / pc[2]) + cx)
            v = np.float32(fy * (pc[1] / pc[2]) + cy)
        inside = bool(u >= np.float32(0.0) and u < np.float32(self.width) and v >= np.float32(0.0) and v < np.float32(self.height))
        return inside, ImagePoint(u, v, depth)


class VoxelGridData:
    """cpp/volumetric/voxel_grid_data.h:36-50: .points/.colors (+ empty semantic fields); default-constructible like the binding's."""

    def __init__(self, points=None, colors=None):
        self.points = np.zeros((0, 3), np.float32) if points is None else points
        self.colors = np.zeros((0, 3), np.float32) if colors is None else colors
        self.class_ids = np.zeros((0,), np.int32)
        self.object_ids = np.zeros((0,), np.int32)
        self.confidences = np.zeros((0,), np.float32)


class VoxelData:
    """``volumetric.VoxelData`` (volumetric_grid_module.h:943-947; cpp/volumetric/voxel_data.h:118-139): the value type of one voxel as
    the module hands it to Python - ``count`` (read / write), ``get_position()``, ``get_color()`` = sum / count in float32 (0 / 0 = nan for
    an empty voxel: the release build has no zero-count check, voxel_data.h:31-37).  A host-side value class as in the reference; the
    grids keep their voxels in HBM (HvVoxel) and return rows, not objects."""

    _pos_dtype = np.float32

    def __init__(self):
        self.count = 0
        self.position_sum = np.zeros(3, self._pos_dtype)
        self.color_sum = np.zeros(3, np.float32)

    def get_position(self):
        with np.errstate(invalid="ignore", divide="ignore"):
            return list(self.position_sum / self._pos_dtype(self.count))

    def get_color(self):
        with np.errstate(invalid="ignore", divide="ignore"):
            return list(self.color_sum / np.float32(self.count))


class VoxelBlockGrid(_BlockGrid):
    """``volumetric.VoxelBlockGrid(voxel_size, block_size=8)`` on the GPU.

    integrate() results (count, position_sum, color_sum per voxel) are bit-identical to the
    reference's sequential accumulation; row order of get_voxels() differs (the reference's is its
    unordered_map iteration order), so compare outputs as sets.
    """

    _MODE = L.HV_MODE_VOXEL_GRID

    def __init__(self, voxel_size, block_size=8, device=0, max_blocks=None, max_points=None):
        super().__init__(L.HV_MODE_VOXEL_GRID, voxel_size, block_size, device, max_blocks, max_points)

    # -- integrate -------------------------------------------------------------------------------
    def integrate(self, points, colors=None):
        """points: [N,3] float32 or float64 (the binding's two overloads, volumetric_grid_module.h:738-749: float64 points
        are keyed in double, anything else goes through float32); colors: [N,3] uint8|float32|None."""
        pts, wide, n = _points_operand(points, torch_ok=True)
        if n == 0:
            return
        cols, kind = _colors_operand(colors, n, torch_ok=True)
        if cols is not None and L.location(cols) != L.location(pts):
            raise RuntimeError("points and colors must live on the same device")
        fn = self._lib.hv_integrate_points_f64 if wide else self._lib.hv_integrate_points
        L.check(fn(self._h, L.ptr(pts), n, L.ptr(cols), kind, L.location(pts)))

    def integrate_rgbd(self, depth, rgb, fx, fy, cx, cy, T_cw, max_depth=np.inf, min_depth=0.0, depth_scale=1.0):
        """Fused depth2pointcloud + world transform + integrate for one posed RGB-D frame
        (pyslam/utilities/depth.py:45-85, volumetric_integrator_voxel_grid.py:251-300)."""
        dkind = L.HV_DEPTH_U16 if str(depth.dtype) in ("uint16", "torch.uint16") else L.HV_DEPTH_F32
        if _is_torch(depth):  # torch: the kernels read packed f32 / u16 depth and packed u8 colour
            if str(depth.dtype) not in ("torch.float32", "torch.uint16") or not depth.is_contiguous() or not rgb.is_contiguous() \
                    or str(rgb.dtype) != "torch.uint8":
                raise RuntimeError("integrate_rgbd: device inputs must be contiguous float32|uint16 depth and uint8 colour")
        else:  # host arrays: float64 / strided inputs are converted, not silently misread
            depth = np.ascontiguousarray(depth, dtype=np.uint16 if dkind == L.HV_DEPTH_U16 else np.float32)
            rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
        H, W = int(depth.shape[0]), int(depth.shape[1])
        if tuple(rgb.shape) != (H, W, 3):
            raise RuntimeError(f"integrate_rgbd: colour image {tuple(rgb.shape)} does not match depth {(H, W)}")
        intr = np.array([fx, fy, cx, cy], dtype=np.float64)
        T = _as_f64_4x4(T_cw)
        maxd = float(min(max_depth, 3.0e38))
        L.check(
            self._lib.hv_integrate_rgbd_points(
                self._h, L.ptr(depth), dkind, float(depth_scale), L.ptr(rgb), H, W, L.ptr(intr), L.ptr(T),
                float(min_depth), maxd, L.location(depth)
            )
        )

    def integrate_rgbd_batch(self, depth, rgb, fx, fy, cx, cy, T_cw, max_depth=np.inf, min_depth=0.0, depth_scale=1.0):
        """Replay F posed frames ([F,H,W] depth, [F,H,W,3] rgb, [F,4,4] T_cw): bit-identical to F integrate_rgbd()
        calls, with one device sort per max_points / (H*W) frames (create the grid with a large max_points)."""
        dkind = L.HV_DEPTH_U16 if str(depth.dtype) in ("uint16", "torch.uint16") else L.HV_DEPTH_F32
        F, H, W = (int(x) for x in depth.shape)
        if not _is_torch(depth):
            depth = np.ascontiguousarray(depth, dtype=np.uint16 if dkind == L.HV_DEPTH_U16 else np.float32)
            rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
        intr = np.array([fx, fy, cx, cy], dtype=np.float64)
        T = np.ascontiguousarray(np.asarray(T_cw, dtype=np.float64).reshape(F, 16))
        L.check(self._lib.hv_integrate_rgbd_points_batch(self._h, L.ptr(depth), dkind, float(depth_scale), L.ptr(rgb), F, H, W,
                                                         L.ptr(intr), L.ptr(T), float(min_depth), float(min(max_depth, 3.0e38)),
                                                         L.location(depth)))

    # -- queries ---------------------------------------------------------------------------------
    def _collect(self, call):
        return VoxelGridData(*self._sized_fetch(call, ((3,), np.float32), ((3,), np.float32)))

    def get_voxels(self, min_count=1, min_confidence=0.0):
        return self._collect(
            lambda p, c, cap, n: self._lib.hv_get_voxels(self._h, int(min_count), float(min_confidence), p, c, cap, n, L.HV_HOST)
        )

    def get_points(self):
        return self.get_voxels(1, 0.0).points

    def get_colors(self):
        return self.get_voxels(1, 0.0).colors

    def get_voxels_in_bb(self, bbox, min_count=1, min_confidence=0.0, include_semantics=False):
        bb = bbox.as_array() if isinstance(bbox, BoundingBox3D) else np.ascontiguousarray(bbox, dtype=np.float64)
        return self._collect(
            lambda p, c, cap, n: self._lib.hv_get_voxels_in_bb(
                self._h, L.ptr(bb), int(min_count), float(min_confidence), p, c, cap, n, L.HV_HOST
            )
        )

    def get_voxels_in_camera_frustrum(self, camera_frustrum, min_count=1, min_confidence=0.0, include_semantics=False):
        f = camera_frustrum
        return self._collect(
            lambda p, c, cap, n: self._lib.hv_get_voxels_in_frustum(
                self._h, L.ptr(f.intr), f.width, f.height, L.ptr(f.T_cw), f.depth_max, f.depth_min,
                int(min_count), float(min_confidence), p, c, cap, n, L.HV_HOST
            )
        )

    def remove_low_confidence_voxels(self, min_confidence):
        return  # no-op for non-semantic voxels (voxel_block_grid.hpp:650-676)

    # -- parity/debug ----------------------------------------------------------------------------
    def dump(self):
        """-> keys [B,3] i32, hashes [B] u64, counts [B,bs^3] i32, sums [B,bs^3,6] f32, key-sorted."""
        nb = self.num_blocks()
        nv = self.block_size ** 3
        keys = np.zeros((nb, 3), np.int32)
        hashes = np.zeros(nb, np.uint64)
        counts = np.zeros((nb, nv), np.int32)
        sums = np.zeros((nb, nv, 6), np.float32)
        self._int64(self._lib.hv_dump_blocks, L.ptr(keys), L.ptr(hashes), L.ptr(counts), L.ptr(sums))
        return keys, hashes, counts, sums

    def keys_from_points(self, points):
        pts = np.ascontiguousarray(points, dtype=np.float32)
        n = pts.shape[0]
        vk = np.zeros((n, 3), np.int32)
        bk = np.zeros((n, 3), np.int32)
        lk = np.zeros((n, 3), np.int32)
        h = np.zeros(n, np.uint64)
        L.check(self._lib.hv_keys_from_points(self._h, L.ptr(pts), n, L.ptr(vk), L.ptr(bk), L.ptr(lk), L.ptr(h)))
        return vk, bk, lk, h


class VoxelGrid(VoxelBlockGrid):
    """``volumetric.VoxelGrid(voxel_size)`` — the reference's *direct* voxel hash (cpp/volumetric/voxel_grid.h:83-245;
    selected only with kVolumetricIntegrationUseVoxelBlocks=False).  Its observable results (per-voxel sums in
    point-index order, get_voxels / queries / carve) are those of the block grid, so on the GPU it is the block hash
    behind the direct grid's constructor.  Two reference quirks of this non-default path: uint8 colours are dropped
    by its scalar branch (HasColors = is_same<Tc, float>, voxel_grid.hpp:493-498) — mirrored here; with float32
    points + float32 colours an AVX2/SSE build accumulates batches of 4 in double (voxel_grid_simd.hpp) — not
    mirrored (the non-SIMD build, which is what the oracle compiles, matches bit for bit)."""

    _ALIAS_BLOCK_SIZE = 8

    def __init__(self, voxel_size=0.05, device=0, max_blocks=None, max_points=None):
        super().__init__(voxel_size, 8, device=device, max_blocks=max_blocks, max_points=max_points)

    def integrate(self, points, colors=None):
        if colors is not None and getattr(colors, "dtype", None) == np.uint8:
            colors = None
        return super().integrate(points, colors)


class TBBUtils:
    """`volumetric.TBBUtils` exists only so callers' thread-cap call keeps working; the GPU path has
    no CPU worker threads (cpp/volumetric/tbb_utils.h:29-58)."""

    _max_threads = None  # what the caller set last (nothing on the GPU path depends on it)

    @staticmethod
    def set_max_threads(num_threads):
        """-> the number of threads set (tbb_utils.h:37-48: a value <= 0 asks for the default, all hardware threads)."""
        import os

        TBBUtils._max_threads = int(num_threads) if int(num_threads) > 0 else (os.cpu_count() or 1)
        return TBBUtils._max_threads

    @staticmethod
    def get_max_threads():
        """tbb_utils.h:51-53: the cap in force (the host's hardware threads until one is set)."""
        import os

        return TBBUtils._max_threads if TBBUtils._max_threads is not None else (os.cpu_count() or 1)


# ================================================================================================
# open3d slice mirror (TSDF)
# ================================================================================================
class PinholeCameraIntrinsic:
    """o3d.camera.PinholeCameraIntrinsic(width, height, fx, fy, cx, cy)."""

    def __init__(self, width, height, fx, fy, cx, cy):
        self.width = int(width)
        self.height = int(height)
        self.fx, self.fy, self.cx, self.cy = float(fx), float(fy), float(cx), float(cy)

    def as_array(self):
        return np.array([self.fx, self.fy, self.cx, self.cy], dtype=np.float64)


class RGBDImage:
    """o3d.geometry.RGBDImage.create_from_color_and_depth(color, depth, depth_scale, depth_trunc,
    convert_rgb_to_intensity=False): the scale/trunc conversion itself runs on the GPU inside
    integrate(); this object only carries the operands."""

    def __init__(self, color, depth, depth_scale=1000.0, depth_trunc=3.0):
        self.color = color
        self.depth = depth
        self.depth_scale = float(depth_scale)
        self.depth_trunc = float(depth_trunc)

    @staticmethod
    def create_from_color_and_depth(color, depth, depth_scale=1000.0, depth_trunc=3.0, convert_rgb_to_intensity=True):
        if convert_rgb_to_intensity:
            raise RuntimeError("[ScalableTSDFVolume::Integrate] Unsupported image format.")
        return RGBDImage(color, depth, depth_scale, depth_trunc)


class TriangleMesh:
    def __init__(self, vertices, triangles, vertex_colors, vertex_cluster=None):
        self.vertices = vertices
        self.triangles = triangles
        self.vertex_colors = vertex_colors
        if vertex_cluster is not None:  # extract_simplified_mesh(vertex_map=True): int32 [V], full vertex -> simplified vertex
            self.vertex_cluster = vertex_cluster
        self.vertex_normals = np.zeros((0, 3), np.float64)  # compute_vertex_normals() is not called by pySLAM


class PointCloud:
    def __init__(self, points, colors, normals=None):
        self.points = points
        self.colors = colors
        self.normals = normals  # [N,3] f64 when asked for (Open3D's point cloud always carries them), else None

    def has_normals(self):
        return self.normals is not None and len(self.normals) == len(self.points)


class ScalableTSDFVolume(_Volume):
    """o3d.pipelines.integration.ScalableTSDFVolume(voxel_length, sdf_trunc, color_type=RGB8) on
    the GPU (volume_unit_resolution=16, depth_sampling_stride=4 as in Open3D)."""

    def __init__(self, voxel_length, sdf_trunc, color_type=None, volume_unit_resolution=16,
                 depth_sampling_stride=4, device=0, max_blocks=None, max_points=None):
        super().__init__(L.HV_MODE_TSDF, voxel_length, sdf_trunc, volume_unit_resolution, depth_sampling_stride,
                         device, max_blocks, max_points)
        self.voxel_length = float(voxel_length)
        self.sdf_trunc = float(sdf_trunc)
        self.res = int(volume_unit_resolution)

    def reset(self):
        L.check(self._lib.hv_reset(self._h))

    def integrate(self, image, intrinsic, extrinsic):
        """image: RGBDImage (color HxWx3 uint8 RGB, depth HxW uint16 or any real dtype, read as float32); extrinsic = T_cw."""
        self._frame_call(self._lib.hv_tsdf_integrate, image.depth, image.color, intrinsic, [extrinsic], image.depth_scale, image.depth_trunc)

    def integrate_batch(self, depth, color, intrinsic, extrinsics, depth_scale=1.0, depth_trunc=4.0):
        """Replay F posed frames ([F,H,W] depth, [F,H,W,3] colour, [F,4,4] T_cw); same result as F
        integrate() calls (the rebuild() use case, volumetric_integrator_base.py:1242-1318)."""
        self._frame_call(self._lib.hv_tsdf_integrate_batch, depth, color, intrinsic, [extrinsics], float(depth_scale), float(depth_trunc),
                         batch=True)

    def _batch_operands(self, depth, color, intrinsic, *extrinsics):
        F = int(depth.shape[0]) if len(depth.shape) == 3 else -1
        depth, color, dkind, converted = _tsdf_operands(depth, color, intrinsic, frames=F)
        return F, depth, color, dkind, converted, [_pose_rows(T, F) for T in extrinsics]

    def _frame_call(self, fn, depth, color, intrinsic, poses, depth_scale, depth_trunc, batch=False, stats=False):
        """The one path of integrate / deintegrate / reintegrate, of one frame (poses: 4x4 each) or, batch=True, of F frames (poses:
        F each): the operands in the library's layout (_tsdf_operands), the pose check, fn(handle, depth, kind, colour, [F,] H, W,
        intrinsics, pose(s), depth_scale, depth_trunc, location[, stats]) through _launch_tsdf.  stats: fn fills a
        hv_deintegrate_stats -> DeintegrationStats, else None.  Zero frames: no call, and the stats stay 0."""
        if batch:
            F, depth, color, dkind, converted, poses = self._batch_operands(depth, color, intrinsic, *poses)
            dims = (F, int(depth.shape[1]), int(depth.shape[2]))
        else:
            depth, color, dkind, converted = _tsdf_operands(depth, color, intrinsic)
            dims = (int(depth.shape[0]), int(depth.shape[1]))
            poses = [_as_f64_4x4(T) for T in poses]
        st = L.HvDeintegrateStats() if stats else None
        if not (batch and dims[0] == 0):
            intr = intrinsic.as_array()
            tail = (depth_scale, depth_trunc, L.location(depth)) + ((ctypes.byref(st),) if stats else ())
            self._launch_tsdf(depth, color, converted, lambda: fn(
                self._h, L.ptr(depth), dkind, L.ptr(color), *dims, L.ptr(intr), *[L.ptr(T) for T in poses], *tail))
        return _stats(DeintegrationStats, st) if stats else None

    def _launch_tsdf(self, depth, color, converted, call):
        """The kernels gather from the operands asynchronously on the volume's stream: keep them alive until the next call (by
        then the stream has consumed them or they are still referenced here).  Operands converted on the device come from
        torch's current stream: the volume's stream waits for it, and torch's waits for the launch before it may reuse them."""
        self._inflight = (getattr(self, "_inflight_prev", None), depth, color)
        self._inflight_prev = (depth, color)
        ts = self._torch_in(depth) if converted else None
        try:
            L.check(call())
        finally:
            if ts is not None:
                self._torch_out(ts, depth.device)

    def deintegrate(self, image, intrinsic, extrinsic):
        """Take the observations integrate(image, intrinsic, extrinsic) added back out of the map (include/hipvol.h,
        hv_tsdf_deintegrate): image and extrinsic must be what that frame was fused with.  Where they are not, and the voxel holds
        more observations than are removed, each colour sum is clamped to [0, 255 * weight] (colours stay in 0..255); the tsdf is
        not clamped.  Waits for the GPU and returns DeintegrationStats."""
        return self._frame_call(self._lib.hv_tsdf_deintegrate, image.depth, image.color, intrinsic, [extrinsic], image.depth_scale,
                                image.depth_trunc, stats=True)

    def deintegrate_batch(self, depth, color, intrinsic, extrinsics, depth_scale=1.0, depth_trunc=4.0):
        """Take F frames ([F,H,W] depth, [F,H,W,3] colour, [F,4,4] T_cw they were fused with) back out of the map, in chunks of 64
        frames in order (colour sums clamped as in deintegrate).  Waits for the GPU and returns DeintegrationStats; zero frames is a
        no-op."""
        return self._frame_call(self._lib.hv_tsdf_deintegrate_batch, depth, color, intrinsic, [extrinsics], float(depth_scale),
                                float(depth_trunc), batch=True, stats=True)

    def reintegrate_batch(self, depth, color, intrinsic, old_extrinsics, new_extrinsics, depth_scale=1.0, depth_trunc=4.0):
        """Move F fused frames from the poses they were fused with (old_extrinsics) to corrected ones (new_extrinsics): the
        result of deintegrate_batch(old) followed by integrate_batch(new), bit for bit, with the frames uploaded once.  Waits for
        the GPU and returns the de-integration's DeintegrationStats; zero frames is a no-op."""
        return self._frame_call(self._lib.hv_tsdf_reintegrate_batch, depth, color, intrinsic, [old_extrinsics, new_extrinsics],
                                float(depth_scale), float(depth_trunc), batch=True, stats=True)

    def prune(self, empty=True, bounds=None):
        """Give units back to the pool (include/hipvol.h, hv_tsdf_prune).  empty: release every unit whose weights are all 0 -
        what de-integration emptied and what the touch pass claimed without ever updating.  bounds = (min_xyz, max_xyz) in world
        metres or None: release every unit outside unit_range_of_bounds(bounds, ...), observed voxels and all (a window that
        follows the camera).  num_blocks() shrinks, max_blocks() does not: the released blocks are claimed again by later
        frames.  Waits for the GPU and returns PruneStats; with neither criterion, or nothing to release, the volume is untouched."""
        lo = hi = None
        if bounds is not None:
            lo, hi = unit_range_of_bounds(bounds, self.voxel_length, self.res)
            lo, hi = np.ascontiguousarray(lo, dtype=np.int32), np.ascontiguousarray(hi, dtype=np.int32)
        st = L.HvPruneStats()
        L.check(self._lib.hv_tsdf_prune(self._h, 1 if empty else 0, None if lo is None else lo.ctypes.data_as(L._pi32),
                                        None if hi is None else hi.ctypes.data_as(L._pi32), ctypes.byref(st)))
        return _stats(PruneStats, st)

    def integrate_volume(self, source, transformation=None):
        """Fuse another TSDF volume into this one (include/hipvol.h, hv_tsdf_integrate_volume): p_self = transformation @ p_source,
        a rigid float64 [4,4] (default: identity).  Every voxel of this volume whose centre falls onto observed voxels of `source`
        takes the source field sampled there (trilinear, or the nearest voxel at the edge of what was observed) as that many
        observations; units are claimed exactly where a voxel is updated.  `source` is only read and must have the same
        voxel_length, sdf_trunc and unit resolution.  To move a map to another frame, merge it ONCE into an empty volume: every merge
        resamples.  Waits for the GPU and returns MergeStats; a source without observed voxels leaves this volume untouched."""
        T = _rigid_operand(source, transformation, "integrate_volume", "transformation")
        st = L.HvMergeStats()
        L.check(self._lib.hv_tsdf_integrate_volume(self._h, source._h, L.ptr(T), ctypes.byref(st)))
        return _stats(MergeStats, st)

    def register_volume(self, source, init=None, max_iterations=30, weight_threshold=3.0, tsdf_band=0.5, residual_trunc=None,
                        huber_delta=None, trace=False):
        """Align another TSDF volume to this one on the two signed distance fields (include/hipvol.h, hv_tsdf_register_volume): ->
        RegistrationResult whose transformation is the refined T_self_source (p_self = T p_source), ready for integrate_volume.
        init: the guess, a rigid float64 [4,4] (default: identity), checked as integrate_volume checks its transform.  A REFINEMENT,
        not a global search: the fields know distances only inside the truncation band, so init must be good to roughly
        (1 - tsdf_band) * sdf_trunc.  Source voxels with weight > weight_threshold and |tsdf| <= tsdf_band are sampled in this volume
        (all eight voxels around them observed above the same threshold); residuals beyond residual_trunc (default 0.5 sdf_trunc)
        are outliers, beyond huber_delta (default 0.25 sdf_trunc) down-weighted.  Both volumes are only read and must agree in
        voxel_length, sdf_trunc and unit resolution.  Empty maps or no overlap: success False, transformation == init.  Waits for
        the GPU.  trace=True: the per-linearisation record (tests)."""
        T = _rigid_operand(source, init, "register_volume", "init")
        prm = L.HvRegisterParams()
        prm.weight_threshold, prm.tsdf_band = float(weight_threshold), float(tsdf_band)
        sdf_trunc = float(getattr(self, "sdf_trunc", 0.0))  # (a volume without one is refused by the library for its mode)
        prm.residual_trunc = 0.5 * sdf_trunc if residual_trunc is None else float(residual_trunc)
        prm.huber_delta = 0.25 * sdf_trunc if huber_delta is None else float(huber_delta)
        prm.max_iterations = int(max_iterations)
        res = L.HvRegisterResult()
        steps = max(int(max_iterations), 1)
        rows = np.zeros((steps, L.HV_REGISTER_TRACE_STRIDE), np.float64) if trace else None
        n_rows = ctypes.c_int64()
        L.check(self._lib.hv_tsdf_register_volume(self._h, source._h, L.ptr(T), ctypes.byref(prm), ctypes.byref(res), L.ptr(rows),
                                                  steps if trace else 0, ctypes.byref(n_rows)))
        return RegistrationResult(np.array(res.T_dst_src, np.float64).reshape(4, 4), float(res.fitness), float(res.inlier_rmse),
                                  np.array(res.information, np.float64).reshape(6, 6), bool(res.success), int(res.iterations),
                                  int(res.inliers), int(res.candidates), np.array(res.anchor, np.float64),
                                  _trace_rows(rows[:n_rows.value], _REGISTER_HEAD) if trace else None)

    def integrate_frames(self, depths, colors, intrinsic, extrinsics, depth_scale=1.0, depth_trunc=4.0):
        """integrate_batch for HOST frames held one numpy array per frame (what the integrator worker has after draining
        its queue): no np.stack - the library copies every frame straight into page-locked staging slots and sends them
        over PCIe on a copy stream while the previous batch is swept.  Same result as len(depths) integrate() calls."""
        F = len(depths)
        if len(colors) != F:
            raise RuntimeError(_UNSUPPORTED_IMAGE)
        T = _pose_rows(extrinsics, F)
        if F == 0:
            return
        ops = [_tsdf_operands(d, c, intrinsic) for d, c in zip(depths, colors)]
        if any(L.location(o[0]) != L.HV_HOST for o in ops) or len({o[2] for o in ops}) != 1:
            raise RuntimeError(_UNSUPPORTED_IMAGE)  # host frames of one depth type
        dkind = ops[0][2]
        depths = [np.asarray(o[0]) for o in ops]  # (host torch tensors: numpy views of the same memory)
        colors = [np.asarray(o[1]) for o in ops]
        H, W = (int(x) for x in depths[0].shape)
        intr = intrinsic.as_array()
        dp = (ctypes.c_void_p * F)(*[d.ctypes.data for d in depths])
        cp = (ctypes.c_void_p * F)(*[c.ctypes.data for c in colors])
        L.check(self._lib.hv_tsdf_integrate_frames(self._h, dp, dkind, cp, F, H, W, L.ptr(intr), L.ptr(T), float(depth_scale),
                                                   float(depth_trunc)))

    def set_color_order(self, bgr=False):
        """Colour frames handed to integrate* are R, G, B (Open3D's order, default) or B, G, R (OpenCV's: pySLAM's keyframe.img)."""
        L.check(self._lib.hv_tsdf_set_color_order(self._h, 1 if bgr else 0))

    def set_tile(self, u0, v0, u1, v1):
        """Restrict fusion to the image tile [u0,u1) x [v0,v1) (multi-GPU sharding); zeros = whole image."""
        L.check(self._lib.hv_tsdf_set_tile(self._h, int(u0), int(v0), int(u1), int(v1)))

    def set_rectify_maps(self, map_x, map_y):
        """Undistort / rectify on the device: every frame handed to integrate / integrate_batch / integrate_frames afterwards goes
        through the maps first (colour bilinear, depth nearest - the reference's per-keyframe cv2.remap pair,
        volumetric_integrator_base.py:1017-1043), one launch per batch; the caller passes the RECTIFIED intrinsics.  None clears."""
        if map_x is None or map_y is None:
            L.check(self._lib.hv_tsdf_set_rectify_maps(self._h, None, None, 0, 0, L.HV_HOST))
            return
        mx, my = np.ascontiguousarray(map_x, dtype=np.float32), np.ascontiguousarray(map_y, dtype=np.float32)
        assert mx.ndim == 2 and mx.shape == my.shape
        L.check(self._lib.hv_tsdf_set_rectify_maps(self._h, L.ptr(mx), L.ptr(my), int(mx.shape[0]), int(mx.shape[1]), L.HV_HOST))

    def set_owner(self, rank, world_size):
        """Fuse/store only the units owned by `rank` of `world_size` (multi-GPU unit-ownership sharding)."""
        L.check(self._lib.hv_tsdf_set_owner(self._h, int(rank), int(world_size)))

    @staticmethod
    def _out_dtype(dtype):
        dt = np.dtype(np.float64 if dtype is None else dtype)
        if dt not in (np.dtype(np.float64), np.dtype(np.float32)):
            raise TypeError(f"extraction dtype must be float64 (Open3D's) or float32, got {dt}")
        return dt

    def extract_triangle_mesh(self, device=False, dtype=None):
        """o3d's extract_triangle_mesh().  device=True: vertices / vertex_colors / triangles are torch CUDA tensors on the volume's GPU
        (nothing crosses PCIe: for consumers that render or post-process on the GPU); default: host arrays like Open3D's.
        dtype=np.float32: vertices / vertex_colors as float32 - Open3D's float64 values rounded once on the device (what
        Parameters.kDenseMappingDtypeVertices / Colors name and pySLAM's viewer casts to, config_parameters.py:290-291): a third fewer
        bytes per output tick.  Default float64 = Open3D's arrays."""
        dt = self._out_dtype(dtype)
        fn = self._lib.hv_tsdf_extract_mesh if dt == np.float64 else self._lib.hv_tsdf_extract_mesh_f32
        nv, nt = ctypes.c_int64(), ctypes.c_int64()
        L.check(fn(self._h, None, None, 0, None, 0, ctypes.byref(nv), ctypes.byref(nt)))
        out = self._results({"verts": ((nv.value, 3), dt), "cols": ((nv.value, 3), dt), "tris": ((nt.value, 3), np.int32)}, device)
        verts, cols, tris = out["verts"], out["cols"], out["tris"]
        if nv.value or nt.value:
            L.check(fn(self._h, L.ptr(verts), L.ptr(cols), nv.value, L.ptr(tris), nt.value, ctypes.byref(nv), ctypes.byref(nt)))
        return TriangleMesh(verts, tris, cols)

    SIMPLIFIED_MESH_CELLS = (2, 4, 8, 16)

    def extract_simplified_mesh(self, cell=4, device=False, dtype=None, vertex_map=False):
        """The mesh of extract_triangle_mesh() simplified by vertex clustering on the device (include/hipvol.h,
        hv_tsdf_extract_mesh_clustered): one vertex per cube of `cell` voxels (2, 4, 8 or 16) that holds full-mesh vertices - the mean
        of their positions and colours - and the distinct non-degenerate triangles between those, sorted.  For viewers, links and
        files that do not want millimetre triangles: the full mesh is neither written nor copied.  device and dtype as in
        extract_triangle_mesh.  vertex_map=True: the mesh also carries .vertex_cluster, int32 [V] - for every vertex of
        extract_triangle_mesh() the number of its simplified vertex (to carry per-vertex data such as label_mesh results over).
        Normals are not part of the result: sample_points(mesh.vertices, gradient=True) gives them.  The map is only read."""
        if isinstance(cell, bool) or not isinstance(cell, (int, np.integer)) or int(cell) not in self.SIMPLIFIED_MESH_CELLS:
            raise ValueError(f"extract_simplified_mesh: cell must be one of {self.SIMPLIFIED_MESH_CELLS} voxels, got {cell!r}")
        cell = int(cell)
        dt = self._out_dtype(dtype)
        fn = self._lib.hv_tsdf_extract_mesh_clustered if dt == np.float64 else self._lib.hv_tsdf_extract_mesh_clustered_f32
        nv, nt, nf = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        L.check(fn(self._h, cell, None, None, 0, None, 0, None, 0, ctypes.byref(nv), ctypes.byref(nt), ctypes.byref(nf)))
        out = self._results({"verts": ((nv.value, 3), dt), "cols": ((nv.value, 3), dt), "tris": ((nt.value, 3), np.int32),
                             "map": ((nf.value,), np.int32) if vertex_map else None}, device)
        verts, cols, tris, vmap = out["verts"], out["cols"], out["tris"], out["map"]
        if nv.value or nt.value:
            L.check(fn(self._h, cell, L.ptr(verts), L.ptr(cols), nv.value, L.ptr(tris), nt.value, L.ptr(vmap), nf.value if vertex_map else 0,
                       ctypes.byref(nv), ctypes.byref(nt), ctypes.byref(nf)))
        return TriangleMesh(verts, tris, cols, vertex_cluster=vmap)

    def extract_point_cloud(self, normals=False, device=False, dtype=None):
        """o3d's extract_point_cloud().  normals=True also computes the per-point normals Open3D attaches (GetNormalAt: the
        gradient of the trilinearly interpolated tsdf) - pySLAM's viewer path does not read them, its save path writes them.
        device=True: torch CUDA tensors on the volume's GPU instead of host arrays.  dtype=np.float32: points / colors as float32
        (see extract_triangle_mesh; the normals stay float64, taken at the float64 points)."""
        dt = self._out_dtype(dtype)
        fn = self._lib.hv_tsdf_extract_points if dt == np.float64 else self._lib.hv_tsdf_extract_points_f32
        n = ctypes.c_int64()
        L.check(fn(self._h, None, None, 0, ctypes.byref(n)))
        out = self._results({"pts": ((n.value, 3), dt), "cols": ((n.value, 3), dt)}, device)
        pts, cols = out["pts"], out["cols"]
        nrm = None
        if n.value:
            L.check(fn(self._h, L.ptr(pts), L.ptr(cols), n.value, ctypes.byref(n)))
        if normals:
            if device:
                import torch

                nrm = torch.zeros((n.value, 3), dtype=torch.float64, device=self._device())
            else:
                nrm = np.zeros((n.value, 3), np.float64)
            if n.value:
                L.check(self._lib.hv_tsdf_extract_point_normals(self._h, L.ptr(nrm), n.value, ctypes.byref(n)))
        return PointCloud(pts, cols, nrm)

    RAY_CAST_ATTRIBUTES = ("depth", "vertex", "normal", "color", "mask")

    def ray_cast(self, intrinsic, extrinsic, depth_min=0.1, depth_max=3.0, weight_threshold=3.0, depth_scale=1.0,
                 render_attributes=RAY_CAST_ATTRIBUTES, device=False):
        """What the fused map looks like from a pinhole camera at extrinsic = T_cw: a dict with the requested attributes,
        depth [H,W] float32 (camera z * depth_scale, metres by default), vertex [H,W,3] float32 (world), normal [H,W,3] float32
        (world, unit length), color [H,W,3] float32 in [0, 1], mask [H,W] bool (the ray hit a surface); 0 where it did not.
        H, W = intrinsic.height, intrinsic.width.  Names and defaults follow Open3D's tensor VoxelBlockGrid.ray_cast; the
        contract (include/hipvol.h, hv_tsdf_ray_cast) is this project's own.  Only the requested attributes are computed.
        device=True: torch CUDA tensors on the volume's GPU, ordered before later work on torch's current stream."""
        attrs = tuple(render_attributes)
        bad = [a for a in attrs if a not in self.RAY_CAST_ATTRIBUTES]
        if bad:
            raise ValueError(f"ray_cast: unknown render attribute(s) {bad}; choose from {self.RAY_CAST_ATTRIBUTES}")
        H, W = int(intrinsic.height), int(intrinsic.width)
        shapes = {"depth": (H, W), "vertex": (H, W, 3), "normal": (H, W, 3), "color": (H, W, 3), "mask": (H, W)}
        intr = intrinsic.as_array()
        T = _as_f64_4x4(extrinsic)
        out = self._results({a: (shapes[a], np.bool_ if a == "mask" else np.float32) for a in attrs}, device)
        p = {a: (L.ptr(out[a]) if a in out else None) for a in self.RAY_CAST_ATTRIBUTES}
        L.check(self._lib.hv_tsdf_ray_cast(self._h, H, W, L.ptr(intr), L.ptr(T), float(depth_min), float(depth_max),
                                           float(weight_threshold), float(depth_scale), p["depth"], p["vertex"], p["normal"],
                                           p["color"], p["mask"], L.HV_DEVICE if device else L.HV_HOST))
        if device:
            self._publish(self._device())
        return out

    def track_frame_to_model(self, depth, intrinsic, extrinsic, depth_scale=1.0, depth_min=0.1, depth_max=3.0, weight_threshold=3.0,
                             iterations=(10, 5, 4), depth_outlier_trunc=0.07, depth_huber_delta=0.05, trace=False, color=None,
                             intensity_weight=0.01, intensity_huber_delta=0.1):
        """Point-to-plane alignment of one depth frame against the fused map rendered at extrinsic = T_cw_init: -> OdometryResult
        whose transformation is the refined T_cw.  depth [H,W]: numpy or torch (either device), uint16 or any real dtype (as
        float32), divided by depth_scale; H, W = intrinsic.height, intrinsic.width.  iterations: the cap per pyramid level, level 0
        (full resolution) first; levels run coarse to fine.  Names and defaults follow Open3D's tensor odometry; the contract
        (include/hipvol.h, hv_tsdf_track) is this project's own.  Reads the volume only.  A CUDA depth tensor is read after the
        work queued on torch's current stream.  trace=True: the per-linearisation record (tests).
        color [H,W,3] uint8 (the frame's image, as integrate takes it, same place as depth): hybrid tracking (hv_tsdf_track_color) -
        a photometric term on the map's colour, weighted by intensity_weight (>= 0; 0 is the depth-only result bit for bit) with
        Huber threshold intensity_huber_delta (image range [0, 1]), constrains the motions that geometry leaves free (a wall, a
        floor); the result then carries photometric_inliers and intensity_rmse.  color=None: depth only."""
        if color is None:
            d, c, dkind, _ = _tsdf_operands(depth, None, intrinsic, depth_only=True)
        else:
            d, c, dkind, _ = _tsdf_operands(depth, color, intrinsic)
        H, W = int(d.shape[0]), int(d.shape[1])
        iters = [int(i) for i in iterations]
        cprm = L.HvTrackColorParams()
        cprm.intensity_weight, cprm.intensity_huber_delta = float(intensity_weight), float(intensity_huber_delta)
        prm = cprm.base
        prm.depth_scale, prm.depth_min, prm.depth_max = float(depth_scale), float(depth_min), float(depth_max)
        prm.weight_threshold = float(weight_threshold)
        prm.depth_outlier_trunc, prm.depth_huber_delta = float(depth_outlier_trunc), float(depth_huber_delta)
        prm.n_levels = len(iters)
        for i, n in enumerate(iters[:L.HV_TRACK_MAX_LEVELS]):
            prm.iterations[i] = n
        cres = L.HvTrackColorResult()
        res = cres.base
        intr = intrinsic.as_array()
        T0 = _as_f64_4x4(extrinsic)
        steps = max(sum(iters), 1)
        stride = L.HV_TRACK_TRACE_STRIDE if c is None else L.HV_TRACK_COLOR_TRACE_STRIDE
        rows = np.zeros((steps, stride), np.float64) if trace else None
        n_rows = ctypes.c_int64()
        loc = L.location(d)
        with self._ordered(d):
            if c is None:
                L.check(self._lib.hv_tsdf_track(self._h, L.ptr(d), dkind, H, W, L.ptr(intr), L.ptr(T0), ctypes.byref(prm),
                                                ctypes.byref(res), L.ptr(rows), steps if trace else 0, ctypes.byref(n_rows), loc))
            else:
                L.check(self._lib.hv_tsdf_track_color(self._h, L.ptr(d), dkind, L.ptr(c), H, W, L.ptr(intr), L.ptr(T0),
                                                      ctypes.byref(cprm), ctypes.byref(cres), L.ptr(rows), steps if trace else 0,
                                                      ctypes.byref(n_rows), loc))
        n_levels = min(len(iters), L.HV_TRACK_MAX_LEVELS)
        return OdometryResult(np.array(res.T_cw, np.float64).reshape(4, 4), float(res.fitness), float(res.inlier_rmse),
                              np.array(res.information, np.float64).reshape(6, 6), bool(res.success),
                              tuple(int(res.iterations[i]) for i in range(n_levels)), int(res.degenerate), int(res.inliers),
                              int(res.valid), _trace_rows(rows[:n_rows.value]) if trace else None,
                              None if c is None else int(cres.photometric_inliers), None if c is None else float(cres.intensity_rmse))

    def sample_points(self, points, weight_threshold=0.0, gradient=True, color=False, device=None):
        """What the map holds at `points` [n,3] (float32 or float64; numpy or torch, either device): -> SampleResult with the signed
        distance (metres), its gradient (metres per metre, not normalised; gradient=False: None), the colour in [0, 1] (color=True,
        else None), the nearest voxel's observation count and a status per point.  Trilinear where all eight voxels around the point
        have weight > weight_threshold, the nearest voxel where only it has, 0 elsewhere (include/hipvol.h, hv_tsdf_sample_points).
        Reads the volume only.  device=None: results where the input lives - a torch CUDA tensor gives torch CUDA tensors, queued behind
        torch's current stream and ordered before its later work, nothing crosses PCIe; anything else gives numpy arrays.
        device=True / False: torch CUDA tensors on the volume's GPU / numpy arrays, wherever the input lives."""
        if _is_torch(points):
            import torch

            if points.dtype not in (torch.float32, torch.float64):
                raise ValueError(f"sample_points: points must be float32 or float64, got {points.dtype}")
            p = points.contiguous()
        else:
            p = np.asarray(points)
            if p.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
                raise ValueError(f"sample_points: points must be float32 or float64, got {p.dtype}")
            p = np.ascontiguousarray(p)
        if len(p.shape) != 2 or int(p.shape[1]) != 3:
            raise ValueError(f"sample_points: points must have shape [n, 3], got {tuple(p.shape)}")
        p, dev = self._query_place(p, device)
        n = int(p.shape[0])
        f64 = str(p.dtype).endswith("float64")
        f32 = np.float32
        out = self._results({"sdf": ((n,), f32), "gradient": ((n, 3), f32) if gradient else None, "color": ((n, 3), f32) if color else None,
                             "weight": ((n,), f32), "status": ((n,), np.uint8)}, dev is not None, pinned=False, synchronize=False)
        with self._ordered(p):
            L.check(self._lib.hv_tsdf_sample_points(self._h, L.ptr(p), L.HV_F64 if f64 else L.HV_F32, n, float(weight_threshold),
                                                    L.ptr(out["sdf"]), L.ptr(out["gradient"]), L.ptr(out["color"]), L.ptr(out["weight"]),
                                                    L.ptr(out["status"]), L.HV_DEVICE if dev is not None else L.HV_HOST))
        return SampleResult(out["sdf"], out["gradient"], out["color"], out["weight"], out["status"])

    def check_frame(self, depth, intrinsic, extrinsic, depth_scale=1.0, depth_min=0.1, depth_max=3.0, weight_threshold=0.0,
                    tolerance=None, device=None):
        """Does a depth frame taken at extrinsic = T_cw agree with the map?  -> FrameCheck: per pixel the map's signed distance at the
        back-projected point and a class - CHECK_INVALID (no valid depth), CHECK_UNKNOWN (the map knows nothing there),
        CHECK_CONSISTENT (|sdf| <= tolerance), CHECK_IN_FRONT (sdf > tolerance: the point floats in space the map saw as free -
        something that was not there before), CHECK_BEHIND (sdf < -tolerance) - and the five pixel counts (include/hipvol.h,
        hv_tsdf_check_frame).  depth [H,W] as track_frame_to_model takes it: numpy or torch (either device), uint16 or any real dtype
        (as float32), divided by depth_scale, valid in (depth_min, depth_max].  tolerance=None: 0.5 sdf_trunc (register_volume's
        default residual_trunc).  Reads the volume only; waits for the GPU (the counts).  device as sample_points."""
        d, _, dkind, _ = _tsdf_operands(depth, None, intrinsic, depth_only=True)
        H, W = int(d.shape[0]), int(d.shape[1])
        d, dev = self._query_place(d, device)
        prm = L.HvCheckParams()
        prm.depth_scale, prm.depth_min, prm.depth_max = float(depth_scale), float(depth_min), float(depth_max)
        prm.weight_threshold = float(weight_threshold)
        prm.tolerance = 0.5 * float(getattr(self, "sdf_trunc", 0.0)) if tolerance is None else float(tolerance)
        intr = intrinsic.as_array()
        T = _as_f64_4x4(extrinsic)
        out = self._results({"sdf": ((H, W), np.float32), "cls": ((H, W), np.uint8)}, dev is not None, pinned=False, synchronize=False)
        sdf, cls = out["sdf"], out["cls"]
        st = L.HvCheckStats()
        with self._ordered(d):
            L.check(self._lib.hv_tsdf_check_frame(self._h, L.ptr(d), dkind, H, W, L.ptr(intr), L.ptr(T), ctypes.byref(prm), L.ptr(sdf),
                                                  L.ptr(cls), ctypes.byref(st), L.HV_DEVICE if dev is not None else L.HV_HOST))
        return FrameCheck(sdf, cls, FrameCheckStats(*st.count))

    DISTANCE_FIELD_OUTPUTS = ("distance", "dist2", "cls")

    def distance_field(self, bounds, max_distance, weight_threshold=0.0, pad=True, outputs=("distance", "cls"), device=False):
        """Signed Euclidean distance to the map's nearest surface at every voxel of a box, out to max_distance - beyond the
        truncation band, in open space where the map holds no unit: -> DistanceField.  bounds = (lo, hi) in world metres; the box is
        the voxels floor(lo / voxel_length) .. floor(hi / voxel_length) of the map's own lattice (float64), R = ceil(max_distance /
        voxel_length) voxels.  A voxel is observed when weight > weight_threshold, INSIDE when its tsdf <= 0, else FREE; a SITE is an
        observed voxel with an observed axis neighbour of the other sign; distance = +-sqrt(dist2) * voxel_length to the nearest site
        of the computed box, capped at R * voxel_length (include/hipvol.h, hv_tsdf_distance_field).  pad=True computes the box grown by
        R cells per side, so that surfaces just outside `bounds` are seen, and returns views cropped back to it; pad=False computes
        `bounds` as given.  No axis of the computed box may exceed 4096 cells.  outputs: which of "distance", "dist2", "cls" to
        compute.  Reads the volume only; waits for the GPU (the counts).  device=True: torch CUDA tensors on the volume's GPU, ordered
        before later work on torch's current stream."""
        names = tuple(outputs)
        bad = [a for a in names if a not in self.DISTANCE_FIELD_OUTPUTS]
        if bad:
            raise ValueError(f"distance_field: unknown output(s) {bad}; choose from {self.DISTANCE_FIELD_OUTPUTS}")
        try:
            lo_m, hi_m = bounds
            lo_m = np.asarray(lo_m, dtype=np.float64).reshape(-1)
            hi_m = np.asarray(hi_m, dtype=np.float64).reshape(-1)
        except (TypeError, ValueError) as e:
            raise ValueError(f"distance_field: bounds must be (lo_xyz, hi_xyz): {e}") from None
        if lo_m.shape != (3,) or hi_m.shape != (3,) or not (np.all(np.isfinite(lo_m)) and np.all(np.isfinite(hi_m))) or np.any(lo_m > hi_m):
            raise ValueError("distance_field: bounds must be (lo_xyz, hi_xyz), finite, lo <= hi")
        vl = np.float64(self.voxel_length)
        if not (np.isfinite(max_distance) and max_distance > 0.0):
            raise ValueError(f"distance_field: max_distance must be positive and finite, got {max_distance}")
        R = int(np.ceil(np.float64(max_distance) / vl))
        if not 1 <= R <= L.HV_DIST_MAX_RADIUS:
            raise ValueError(f"distance_field: max_distance {max_distance} is {R} voxels; the radius is limited to {L.HV_DIST_MAX_RADIUS}")
        first, last = np.floor(lo_m / vl), np.floor(hi_m / vl)
        if np.any(np.abs(first) > 2.0 ** 30) or np.any(np.abs(last) > 2.0 ** 30):
            raise ValueError("distance_field: bounds reach beyond voxel index +-2^30")
        origin = first.astype(np.int64)
        shape = last.astype(np.int64) - origin + 1
        grow = R if pad else 0
        full_origin, full_shape = origin - grow, shape + 2 * grow
        if np.any(full_shape > L.HV_DIST_MAX_SHAPE):
            raise ValueError(f"distance_field: the box is {shape.tolist()} cells" + (f", {full_shape.tolist()} with {R} cells of padding per side" if pad else "")
                             + f"; the limit is {L.HV_DIST_MAX_SHAPE} per axis (a smaller box, a smaller max_distance or pad=False)")
        prm = L.HvDistanceParams()
        for a in range(3):
            prm.origin[a], prm.shape[a] = int(full_origin[a]), int(full_shape[a])
        prm.radius, prm.weight_threshold = R, float(weight_threshold)
        dtypes = {"distance": np.float32, "dist2": np.uint32, "cls": np.uint8}
        full = tuple(int(n) for n in full_shape)
        out = self._results({a: (full, dtypes[a]) for a in names}, device)  # (device: dist2 int32, the same bits, values <= 2^20)
        st = L.HvDistanceStats()
        L.check(self._lib.hv_tsdf_distance_field(self._h, ctypes.byref(prm), L.ptr(out.get("distance")), L.ptr(out.get("dist2")),
                                                 L.ptr(out.get("cls")), ctypes.byref(st), L.HV_DEVICE if device else L.HV_HOST))
        if device:
            self._publish(self._device())
        crop = tuple(slice(grow, grow + int(n)) for n in shape)
        view = {a: (out[a][crop] if a in out else None) for a in self.DISTANCE_FIELD_OUTPUTS}
        return DistanceField(view["distance"], view["dist2"], view["cls"], origin, shape, float(vl), R,
                             _stats(DistanceFieldStats, st))

    def surface_components(self, weight_threshold=0.0, sites=False, device=False):
        """The connected pieces of the map's surface, labelled in the sparse unit hash on the GPU: -> SurfaceComponents.  A voxel is
        observed when weight > weight_threshold, INSIDE when its tsdf <= 0, else FREE; a SITE is an observed voxel with an observed
        axis neighbour of the other sign (distance_field's rule); two sites are adjacent when their voxel indices differ by at most 1
        on every axis, across unit borders, edges and corners; a component is a class of the closure of that.  Components are
        numbered by their smallest site in (x, y, z) order, whatever the pool order (include/hipvol.h, hv_tsdf_surface_components).
        Per component: seed, sites (the count), lo, hi.  sites=True adds the site list, site_index [N,3] and site_label [N] - to
        colour a mesh by component, look its vertices' voxels up there.  Reads the volume only; waits for the GPU; labels the map
        twice (once for the sizes of the results, once to fill them).  device=True: torch CUDA tensors on the volume's GPU, ordered
        before later work on torch's current stream.  An empty map gives zero components."""
        st = L.HvComponentsStats()
        nc, ns = ctypes.c_int64(), ctypes.c_int64()
        call = self._lib.hv_tsdf_surface_components
        L.check(call(self._h, float(weight_threshold), None, None, None, None, 0, None, None, 0, ctypes.byref(nc), ctypes.byref(ns),
                     ctypes.byref(st), L.HV_HOST))
        C, N = int(nc.value), int(ns.value)
        shapes = {"seed": ((C, 3), np.int32), "sites": ((C,), np.int64), "lo": ((C, 3), np.int32), "hi": ((C, 3), np.int32)}
        if sites:
            shapes.update({"site_index": ((N, 3), np.int32), "site_label": ((N,), np.int32)})
        out = self._results(shapes, device)
        if C > 0:
            L.check(call(self._h, float(weight_threshold), L.ptr(out["seed"]), L.ptr(out["sites"]), L.ptr(out["lo"]), L.ptr(out["hi"]), C,
                         L.ptr(out.get("site_index")), L.ptr(out.get("site_label")), N, ctypes.byref(nc), ctypes.byref(ns), ctypes.byref(st),
                         L.HV_DEVICE if device else L.HV_HOST))
            if device:
                self._publish(self._device())
        return SurfaceComponents(out["seed"], out["sites"], out["lo"], out["hi"], out.get("site_index"), out.get("site_label"),
                                 _stats(SurfaceComponentsStats, st), self.voxel_length)

    def remove_small_components(self, min_sites, weight_threshold=0.0, margin=None):
        """Clean the map: reset, in place, every surface component with fewer than min_sites sites - the floaters that noisy depth,
        depth edges and moving objects leave behind - together with the observed voxels within `margin` voxels (Chebyshev) of them
        that are not that close to a kept component (include/hipvol.h, hv_tsdf_remove_components).  margin=None: min(16,
        ceil(sdf_trunc / voxel_length)), the truncation band's half width - a floater's band goes with it; margin >= 1 leaves the
        kept surface's mesh untouched.  Reset voxels are in the fresh state, as after deintegrate; changed units are stamped
        (incremental extraction and dirty_keys() see them); no unit is released - follow with prune(empty=True).  Waits for the GPU
        and returns ComponentRemovalStats; with nothing to remove the volume is untouched, caches included."""
        if margin is None:
            margin = min(L.HV_COMPONENTS_MAX_MARGIN, int(np.ceil(np.float64(self.sdf_trunc) / np.float64(self.voxel_length))))
        st = L.HvRemoveComponentsStats()
        L.check(self._lib.hv_tsdf_remove_components(self._h, float(weight_threshold), int(min_sites), int(margin), ctypes.byref(st)))
        return _stats(ComponentRemovalStats, st)

    # -- parity/debug + multi-GPU ------------------------------------------------------------------
    def dump(self):
        """-> keys [U,3], tsdf [U,R^3] f32, weight [U,R^3] f32, color [U,R^3,3] f64 (0..255), key-sorted,
        voxel order x*R^2 + y*R + z (Open3D IndexOf)."""
        nu = self.num_blocks()
        nv = self.res ** 3
        keys = np.zeros((nu, 3), np.int32)
        tsdf = np.zeros((nu, nv), np.float32)
        weight = np.zeros((nu, nv), np.float32)
        color = np.zeros((nu, nv, 3), np.float64)
        self._int64(self._lib.hv_tsdf_dump, L.ptr(keys), L.ptr(tsdf), L.ptr(weight), L.ptr(color))
        return keys, tsdf, weight, color

    def _keys(self, fn):
        return self._sized_fetch(functools.partial(fn, self._h), ((3,), np.int32))[0]

    def touched_keys(self):
        return self._keys(self._lib.hv_tsdf_touched)

    def unit_keys(self):
        return self._keys(self._lib.hv_tsdf_unit_keys)

    def dirty_keys(self):
        """Units this GPU stamped (i.e. may have updated) since the last mark_merged(), sorted [K,3] int32."""
        return self._keys(self._lib.hv_tsdf_dirty_keys)

    def mark_merged(self):
        L.check(self._lib.hv_tsdf_mark_merged(self._h))

    # -- the halo merge with lists and plan in device memory (hv_halo.hip; distributed.ShardedTSDF._merge_halo_device) ------------
    def halo_lists_device(self, dirty, held):
        """This volume's dirty and held unit keys (packed 64-bit words) into the torch CUDA int64 tensors `dirty` / `held`
        (each at least num_blocks() long).  -> (n_dirty, n_held)."""
        nd, nh = ctypes.c_int64(), ctypes.c_int64()
        L.check(self._lib.hv_merge_halo_lists_device(self._h, L.ptr(dirty), int(dirty.numel()), L.ptr(held), int(held.numel()),
                                                     ctypes.byref(nd), ctypes.byref(nh)))
        return nd.value, nh.value

    def halo_plan_device(self, dirty_all, dirty_counts, held_all, held_counts, world_size, rank, all_dirty_kept=False):
        """The gathered lists ([world, stride] CUDA int64 tensors; counts: host int64 [world]) -> the merge plan, left in the volume.
        -> number of shared units."""
        dc, hc = np.ascontiguousarray(dirty_counts, dtype=np.int64), np.ascontiguousarray(held_counts, dtype=np.int64)
        return self._int64(self._lib.hv_merge_halo_plan_device, L.ptr(dirty_all), L.ptr(dc), int(dirty_all.shape[1]), L.ptr(held_all), L.ptr(hc),
                           int(held_all.shape[1]), int(world_size), int(rank), int(bool(all_dirty_kept)))

    def halo_plan_fetch(self):
        """-> (shared_keys [K,3] int32, action [K] uint8) of the stored plan (host arrays; inspection and tests)."""
        keys, action = self._sized_fetch(functools.partial(self._lib.hv_merge_halo_plan_fetch, self._h), ((3,), np.int32), ((), np.uint8))
        return keys, action

    def halo_pack_planned(self, first, count, payload):
        L.check(self._lib.hv_merge_halo_pack_planned(self._h, int(first), int(count), L.ptr(payload)))

    def halo_unpack_planned(self, first, count, payload):
        L.check(self._lib.hv_merge_halo_unpack_planned(self._h, int(first), int(count), L.ptr(payload)))

    def halo_unpack(self, keys, payload, action):
        """hv_merge_halo_unpack: action[k] 0 = not held here, 1 = keep (state := payload), 2 = zero the unit."""
        keys = np.ascontiguousarray(keys, dtype=np.int32)
        action = np.ascontiguousarray(action, dtype=np.uint8)
        L.check(self._lib.hv_merge_halo_unpack(self._h, L.ptr(keys), keys.shape[0], L.ptr(payload), L.ptr(action), L.location(payload)))

    def export_numerators(self, keys, out=None):
        """keys [K,3] int32 -> payload [K, R^3, 5] float32 {sum tsdf*w, w, sum r, sum g, sum b}."""
        keys = np.ascontiguousarray(keys, dtype=np.int32)
        k = keys.shape[0]
        if out is None:
            out = np.zeros((k, self.res ** 3, 5), np.float32)
        L.check(self._lib.hv_tsdf_export_numerators(self._h, L.ptr(keys), k, L.ptr(out), L.location(out)))
        return out

    def import_numerators(self, keys, payload):
        keys = np.ascontiguousarray(keys, dtype=np.int32)
        L.check(self._lib.hv_tsdf_import_numerators(self._h, L.ptr(keys), keys.shape[0], L.ptr(payload), L.location(payload)))

    # -- packed maps: keeping and moving a map (include/hipvol.h "Packed maps"; hv_pack.hip) ---------------------------------------
    _PACKED = ("hv_tsdf_", L.HvPackInfo, L.HvPackedHeader, PackStats,
               ("voxel_length", "sdf_trunc", "resolution", "version", "units", "voxels", "bytes"))

    def pack(self, device=False):
        """The map as one packed buffer, bit for bit (include/hipvol.h "Packed maps"): every allocated unit, and of each the voxels
        that hold anything.  -> 1-D uint8, a numpy array (page-locked like the extraction results), or with device=True a torch CUDA
        tensor on the volume's GPU (nothing crosses PCIe: for handing the map to another rank).  Only reads the volume; waits for
        the GPU.  Settings of the volume (rectify maps, colour order, sharding, pool size) are not part of a map."""
        return self._pack(device)[0]

    def unpack(self, buf):
        """Fill this EMPTY volume (num_blocks() == 0, same voxel_length and sdf_trunc as the packed map, bit for bit) from a packed
        buffer: numpy, bytes-like or a torch uint8 tensor on either device.  The buffer is validated on the host before a kernel
        sees it; a corrupt or foreign buffer, a non-empty or sharded volume raise HipVolError with the library's message and leave
        the volume unchanged.  Afterwards the volume behaves, call for call, like the one that was packed; every unit counts as
        dirty (dirty_keys()).  To merge a packed map into a map that already holds something, unpack it into a fresh volume and
        integrate_volume that.  Waits for the GPU and returns PackStats."""
        return self._unpack(buf)

    def save(self, path):
        """pack() into the file `path`: written to a temporary file in the same directory, then moved into place (os.replace), so
        a reader never sees half a map.  -> PackStats."""
        return self._save(path)

    @classmethod
    def load(cls, path, device=0, max_blocks=None):
        """A new volume holding the map save() wrote to `path`: voxel_length and sdf_trunc from the file's header, the pool sized
        max_blocks or max(1024, 2 * units) so that the first integrate() after a load does not have to grow it."""
        buf = cls._read_packed(path)
        hdr = cls.packed_info(buf)
        vol = cls(hdr["voxel_length"], hdr["sdf_trunc"], device=device, max_blocks=max_blocks or max(1024, 2 * hdr["units"]))
        vol.unpack(buf)
        return vol

    @staticmethod
    def packed_info(path_or_buffer):
        """The header of a packed map - {voxel_length, sdf_trunc, resolution, version, units, voxels, bytes} - after the library's
        validator (hv_tsdf_packed_check) has passed the WHOLE buffer: a file path, or a buffer as unpack() takes it.  Needs no GPU.
        ValueError with the validator's message, which names the first rule that failed."""
        return _packed_info(ScalableTSDFVolume._PACKED, path_or_buffer)
