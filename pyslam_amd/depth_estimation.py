"""Depth-estimator hand-off without a host round trip (reference
pyslam/depth_estimation/depth_estimator_raft_stereo.py:143-177 and volumetric_integrator_base.py:989-1004).

pySLAM's stereo back-end runs a PyTorch network (RAFT-Stereo by default) on the rectified pair, copies the
disparity to the host, converts it with ``depth = bf / |disparity|`` in numpy and hands a numpy depth image to
the integrator, which uploads it again.  Here the network's output stays a CUDA tensor: the disparity -> depth
conversion is a couple of torch ops on the same device (PyTorch-ROCm as plumbing), and the fused integrate calls
of libpyslam_hipvol take the tensor's device pointer (HV_DEVICE).

No network weights are available offline, so the module is injected: any ``torch.nn.Module`` mapping
(left, right) float tensors [1,3,H,W] to a disparity [1,1,H,W] or [H,W] works; ``StubStereoNet`` is a tiny
deterministic stand-in used by the tests (RAFT-Stereo itself is out of this package's scope); its disparity has nothing to
do with the scene.  ``DepthEstimatorSgm`` needs no weights: census semi-global matching on the GPU (hv_stereo_sgm), depth
in the same place, selected in the dense front by kVolumetricIntegrationDepthEstimatorType = "DEPTH_SGM_HIP".
``DepthEstimatorMvs`` needs none either, and no second camera: plane-sweep matching of a posed keyframe against earlier keyframes
(hv_mvs_sgm), selected by "DEPTH_MVS_HIP"."""
import numpy as np


class DepthEstimatorStereoTorch:
    """infer(image, image_right) -> (depth, None); depth is a float32 CUDA tensor when `keep_on_device`."""

    def __init__(self, module, camera, device="cuda", keep_on_device=True, min_depth=0.0, max_depth=np.inf):
        import torch

        self.torch = torch
        self.module = module.to(device).eval()
        self.camera = camera
        self.device = torch.device(device)
        self.keep_on_device = keep_on_device
        self.min_depth, self.max_depth = float(min_depth), float(max_depth)
        self.disparity_map = None

    def infer(self, image, image_right=None):
        if image_right is None:
            raise ValueError("Image right is None. Are you using a stereo dataset? If not, you cant use a stereo depth estimator here.")
        torch = self.torch
        with torch.no_grad():
            left = torch.from_numpy(np.ascontiguousarray(image)).to(self.device).permute(2, 0, 1).float()[None]
            right = torch.from_numpy(np.ascontiguousarray(image_right)).to(self.device).permute(2, 0, 1).float()[None]
            disparity = self.module(left, right)
            if isinstance(disparity, (tuple, list)):
                disparity = disparity[-1]  # RAFT-Stereo returns (low-res flow, up-sampled flow)
            disparity = disparity.squeeze()
            self.disparity_map = disparity
            bf = float(getattr(self.camera, "bf", 1.0) or 1.0)
            a = disparity.abs()
            depth = torch.where(a > 0, bf / a.clamp_min(1e-30), torch.zeros_like(a)).float()  # raft_stereo.py:170-174
            if np.isfinite(self.max_depth):
                depth = torch.where(depth > self.max_depth, torch.zeros_like(depth), depth)
            if self.min_depth > 0:
                depth = torch.where(depth < self.min_depth, torch.zeros_like(depth), depth)
            depth = depth.contiguous()
        if self.keep_on_device:
            torch.cuda.current_stream(self.device).synchronize()  # the volume's HIP stream consumes it next
            return depth, None
        return depth.cpu().numpy(), None


class DepthEstimatorSgm:
    """The weight-free stereo estimator: census semi-global matching on the GPU (_Volume.stereo_sgm, hv_stereo_sgm), in the
    place of the reference's DepthEstimatorSgbm (pyslam/depth_estimation/depth_estimator_base.py:69-131, a cv2.StereoSGBM).
    infer(image, image_right) -> (depth, None): the pair is uploaded once and the depth stays a float32 CUDA tensor when
    `keep_on_device`, a numpy array otherwise; disparity_map is the int16 disparity in sixteenths (-16 = invalid), in the same
    place.  An invalid pixel has depth 0 (the reference wrapper's bf is not reproduced).  sgm_params: num_disparities, p1, p2,
    uniqueness_ratio, max_diff, paths, speckle_window_size, speckle_range (the reference's speckle filter is
    speckle_window_size=50, speckle_range=1; the default 0 runs none)."""

    def __init__(self, volume, camera, keep_on_device=True, min_depth=0.0, max_depth=np.inf, **sgm_params):
        self.volume = volume
        self.camera = camera
        self.keep_on_device = keep_on_device
        self.min_depth, self.max_depth = float(min_depth), float(max_depth)
        self.sgm_params = dict(sgm_params)
        self.disparity_map = None

    def infer(self, image, image_right=None):
        if image_right is None:
            raise ValueError("Image right is None. Are you using a stereo dataset? If not, you cant use a stereo depth estimator here.")
        bf = float(getattr(self.camera, "bf", 1.0) or 1.0)
        left, right = np.ascontiguousarray(image), np.ascontiguousarray(image_right)
        if self.keep_on_device:
            import torch

            dev = self.volume._device()
            left, right = torch.from_numpy(left).to(dev), torch.from_numpy(right).to(dev)
        self.disparity_map, depth = self.volume.stereo_sgm(left, right, bf=bf, min_depth=self.min_depth, max_depth=self.max_depth,
                                                           **self.sgm_params)
        return depth, None


class DepthEstimatorMvs:
    """The weight-free estimator for a posed single-camera stream: plane-sweep semi-global matching of a keyframe against earlier
    keyframes on the GPU (_Volume.multiview_sgm, hv_mvs_sgm), in the place the reference gives its multi-view networks
    (pyslam/depth_estimation/depth_estimator_mvdust3r.py, depth_estimator_mast3r.py).  Selected in the dense front by
    kVolumetricIntegrationDepthEstimatorType = "DEPTH_MVS_HIP".  The camera is a pinhole (fx, fy, cx, cy): undistort first.

    infer_posed(image, T_cw) -> (depth, None): T_cw is the keyframe's world-to-camera pose.  The estimator keeps a ring of the last
    `ring_size` keyframes (image and pose; with keep_on_device the uploaded image) and matches the new one against the most recent
    ones, at most max_sources, whose camera centres lie between min_baseline and max_baseline metres from its own.  While fewer
    than min_views (an mvs_param, 1 by default) qualify it returns (None, None): the front skips such a keyframe.  depth is z-depth
    in metres, a float32 CUDA tensor with keep_on_device and a numpy array otherwise, 0 = none; index_map is the int16 plane index
    in sixteenths (-16 = invalid) in the same place, sources_used the ring positions of the chosen keyframes (0 = the last one).
    mvs_params: num_planes, p1, p2, uniqueness_ratio, min_views, paths, speckle_window_size, speckle_range.

    consistency_min_views > 0 adds the cross-view check (_Volume.filter_depth_consistency, hv_depth_consistency): the ring also keeps
    each keyframe's RAW depth - the matcher's output before any check, None for a keyframe that produced none, so that one
    keyframe's verdict does not cascade into the next - and the freshly matched depth is checked against those chosen sources that
    carry one, fused with the agreeing ones.  A pixel needs consistency_min_views agreeing views and at most
    consistency_max_violations violated ones (capped at the number of sources checked against); the inverse-depth tolerance is
    consistency_inv_depth_steps plane steps of this estimator's own sweep, the reprojection tolerance consistency_max_reproj
    pixels.  While fewer than consistency_min_views of the chosen sources carry a depth the keyframe returns (None, None) like
    one without sources; it enters the ring with its raw depth all the same.  counts_map is the uint8 [H,W,4] of the check (agree,
    occluded, violated, seen), None without one; index_map stays the matcher's own.  The default 0 runs no check."""

    def __init__(self, volume, camera, keep_on_device=True, *, min_depth, max_depth=np.inf, max_sources=2, min_baseline,
                 max_baseline=np.inf, ring_size=8, consistency_min_views=0, consistency_inv_depth_steps=1.0, consistency_max_reproj=1.0,
                 consistency_max_violations=0, **mvs_params):
        if not 1 <= int(max_sources) <= 4:
            raise ValueError(f"DepthEstimatorMvs: max_sources must be in 1..4, got {max_sources}")
        if not 0.0 <= float(min_baseline) <= float(max_baseline):
            raise ValueError(f"DepthEstimatorMvs: need 0 <= min_baseline <= max_baseline, got {min_baseline} and {max_baseline}")
        if int(ring_size) < int(max_sources):
            raise ValueError(f"DepthEstimatorMvs: ring_size {ring_size} cannot hold max_sources = {max_sources} keyframes")
        self.volume = volume
        self.camera = camera
        self.keep_on_device = keep_on_device
        self.min_depth, self.max_depth = float(min_depth), float(max_depth)
        self.max_sources, self.ring_size = int(max_sources), int(ring_size)
        self.min_baseline, self.max_baseline = float(min_baseline), float(max_baseline)
        if int(consistency_min_views) != consistency_min_views or not 0 <= int(consistency_min_views) <= int(max_sources):
            raise ValueError(f"DepthEstimatorMvs: consistency_min_views must be in 0..max_sources, got {consistency_min_views}")
        if int(consistency_max_violations) != consistency_max_violations or int(consistency_max_violations) < 0:
            raise ValueError(f"DepthEstimatorMvs: consistency_max_violations must be an integer >= 0, got {consistency_max_violations}")
        if not (0.0 < float(consistency_inv_depth_steps) < np.inf and 0.0 <= float(consistency_max_reproj) < np.inf):
            raise ValueError("DepthEstimatorMvs: need consistency_inv_depth_steps > 0 and consistency_max_reproj >= 0, both finite, got "
                             f"{consistency_inv_depth_steps} and {consistency_max_reproj}")
        self.mvs_params = dict(mvs_params)
        self.consistency_min_views, self.consistency_max_violations = int(consistency_min_views), int(consistency_max_violations)
        self.consistency_inv_depth_steps, self.consistency_max_reproj = float(consistency_inv_depth_steps), float(consistency_max_reproj)
        self.ring = []  # [(image, T_cw, camera centre, raw depth or None)], the last keyframe first
        self.index_map = None
        self.counts_map = None
        self.sources_used = ()

    def infer(self, image, image_right=None):
        raise ValueError("DepthEstimatorMvs matches a keyframe against earlier keyframes: call infer_posed(image, T_cw) "
                         "(a stereo pair goes to DepthEstimatorSgm)")

    def infer_posed(self, image, T_cw):
        T = np.array(T_cw, dtype=np.float64).reshape(4, 4)
        centre = -T[:3, :3].T @ T[:3, 3]
        ref = np.ascontiguousarray(image)
        if self.keep_on_device:
            import torch

            ref = torch.from_numpy(ref).to(self.volume._device())
        chosen = []
        for k, (_, _, c, _) in enumerate(self.ring):
            if len(chosen) < self.max_sources and self.min_baseline <= float(np.linalg.norm(c - centre)) <= self.max_baseline:
                chosen.append(k)
        earlier = [self.ring[k] for k in chosen]
        self.sources_used = tuple(chosen)
        self.index_map = self.counts_map = None
        index = raw = None
        K = tuple(float(getattr(self.camera, a)) for a in ("fx", "fy", "cx", "cy"))
        if len(chosen) >= max(int(self.mvs_params.get("min_views", 1)), 1):
            index, raw = self.volume.multiview_sgm(ref, [e[0] for e in earlier], intrinsic=K, T_ref=T, T_sources=np.stack([e[1] for e in earlier]),
                                                   min_depth=self.min_depth, max_depth=self.max_depth, **self.mvs_params)
        self.ring = ([(ref, T, centre, raw)] + self.ring)[:self.ring_size]
        if raw is None:
            return None, None
        if self.consistency_min_views == 0:
            self.index_map = index
            return raw, None
        checked = [e for e in earlier if e[3] is not None]
        if len(checked) < self.consistency_min_views:
            return None, None
        self.index_map = index
        depth, self.counts_map = self.volume.filter_depth_consistency(
            raw, [e[3] for e in checked], intrinsic=K, T_ref=T, T_sources=np.stack([e[1] for e in checked]),
            max_reproj_error=self.consistency_max_reproj, inv_depth_tol=self.consistency_inv_depth_steps * self.plane_step(), rel_depth_tol=0.0,
            min_consistent=self.consistency_min_views, max_violations=min(self.consistency_max_violations, len(checked)), fuse=True, counts=True)
        return depth, None

    def plane_step(self):
        """One plane step of this estimator's sweep in inverse metres: (1 / min_depth - 1 / max_depth) / (num_planes - 1)"""
        far = 0.0 if np.isinf(self.max_depth) else 1.0 / self.max_depth
        return (1.0 / self.min_depth - far) / (int(self.mvs_params.get("num_planes", 128)) - 1)


def make_stub_stereo_net(seed=0):
    """A tiny deterministic conv net with a strictly positive disparity output (tests / examples only)."""
    import torch

    class StubStereoNet(torch.nn.Module):
        def __init__(self):
            super().__init__()
            g = torch.Generator().manual_seed(seed)
            self.conv = torch.nn.Conv2d(6, 1, 5, padding=2, bias=True)
            with torch.no_grad():
                self.conv.weight.copy_(torch.randn(self.conv.weight.shape, generator=g) * 0.002)
                self.conv.bias.fill_(0.0)

        def forward(self, left, right):
            x = torch.cat([left, right], dim=1) / 255.0
            return 20.0 + 30.0 * torch.sigmoid(self.conv(x))  # disparity in (20, 50) px

    return StubStereoNet()
