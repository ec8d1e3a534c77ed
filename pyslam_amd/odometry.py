"""Frame-to-frame RGB-D visual odometry on the GPU: the place of the reference's VisualOdometryRgbdTensor
(pyslam/slam/visual_odometry_rgbd.py, Open3D's rgbd_odometry_multi_scale with methods Hybrid and PointToPlane, three levels, the
previous frame as the other operand) over _Volume.rgbd_odometry (hv_rgbd_odometry).  A plain previous-frame chain: no keyframes,
no drift bound (INTEGRATION.md section 21 has the measured limits)."""
import numpy as np

METHODS = ("hybrid", "point_to_plane")


class VisualOdometryRgbd:
    """track(color, depth) -> T_wc (4x4 float64, camera-to-world) of the frame.

    The first frame has the pose T_wc0 (the identity unless given).  Each later frame is aligned as the SOURCE against the previous
    frame as the TARGET from an identity start, and T_wc := T_wc(previous) @ T_target_source.  When the alignment fails (success is
    False) the pose stays, `lost` is True for that frame, and the frame still becomes the next target.  last_result is the
    OdometryResult of the last alignment (None after the first frame); frames counts the frames seen.

    volume: any volume of this package (context only: its stream and scratch; the map is neither read nor changed).  camera: fx, fy,
    cx, cy, width, height.  method "hybrid" uses the colour image, "point_to_plane" depth alone (color may then be None).
    keep_on_device: each frame is uploaded once and stays on the volume's GPU as the next call's target; False keeps host arrays.
    odometry_params: what rgbd_odometry takes (depth_scale, depth_min, depth_max, iterations, depth_outlier_trunc,
    depth_huber_delta, intensity_weight, intensity_huber_delta)."""

    def __init__(self, volume, camera, method="hybrid", keep_on_device=True, T_wc0=None, **odometry_params):
        if method not in METHODS:
            raise ValueError(f"VisualOdometryRgbd: method must be one of {METHODS}, got {method!r}")
        from .volumetric import PinholeCameraIntrinsic

        self.volume = volume
        self.camera = camera
        self.method = method
        self.keep_on_device = keep_on_device
        self.odometry_params = dict(odometry_params)
        self.intrinsic = PinholeCameraIntrinsic(int(camera.width), int(camera.height), float(camera.fx), float(camera.fy), float(camera.cx),
                                                float(camera.cy))
        self.T_wc = np.eye(4) if T_wc0 is None else np.array(T_wc0, dtype=np.float64).reshape(4, 4)
        self.previous = None  # (depth, color or None) of the last frame, where rgbd_odometry reads them
        self.last_result = None
        self.lost = False
        self.frames = 0

    def _place(self, a):
        a = np.ascontiguousarray(a)
        if not self.keep_on_device:
            return a
        import torch

        return torch.from_numpy(a).to(self.volume._device())

    def track(self, color, depth):
        hybrid = self.method == "hybrid"
        if hybrid and color is None:
            raise ValueError("VisualOdometryRgbd: the hybrid method needs the colour image")
        frame = (self._place(depth), self._place(color) if hybrid else None)
        self.frames += 1
        if self.previous is None:
            self.previous = frame
            self.lost = False
            return self.T_wc.copy()
        target, self.previous = self.previous, frame
        res = self.volume.rgbd_odometry(frame[0], target[0], self.intrinsic, source_color=frame[1], target_color=target[1],
                                        **self.odometry_params)
        self.last_result = res
        self.lost = not res.success
        if res.success:
            self.T_wc = self.T_wc @ res.transformation
        return self.T_wc.copy()
