"""A pose graph and a keyframe graph for RGB-D sessions over _Volume.optimize_pose_graph (hv_pose_graph_optimize): the piece
between odometry and integration that Open3D's reconstruction system calls the pose graph and global_optimization.  Conventions
(INTEGRATION.md section 22): a node is T_wc, camera-to-world; an edge (source, target) carries T_target_source - what
rgbd_odometry(source frame, target frame) returns - and its 6 x 6 information, order (omega, t); odometry edges are certain, loop
closures uncertain: the optimiser's line process may switch those off."""
import numpy as np

from .odometry import METHODS


def _rigid_inverse(T):
    T = np.asarray(T, np.float64)
    out = np.zeros_like(T)
    Rt = np.swapaxes(T[..., :3, :3], -1, -2)
    out[..., :3, :3] = Rt
    out[..., :3, 3] = -(Rt @ T[..., :3, 3:])[..., 0]
    out[..., 3, 3] = 1.0
    return out


def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _torch_cat(parts):
    import torch

    return torch.cat(parts)


class PoseGraph:
    """Nodes and edges as plain arrays: poses [N,4,4] float64, edges [E,2] int32, transformations [E,4,4], informations [E,6,6],
    uncertain [E] bool (properties; the lists behind them grow by add_node / add_edge)."""

    def __init__(self):
        self._poses, self._edges, self._T, self._info, self._uncertain = [], [], [], [], []
        self.last_result = None

    def add_node(self, T_wc):
        """-> the node's index"""
        T = np.array(T_wc, dtype=np.float64)
        if T.shape != (4, 4):
            raise ValueError(f"PoseGraph.add_node: T_wc must be 4x4, got {T.shape}")
        self._poses.append(T)
        return len(self._poses) - 1

    def add_edge(self, source, target, transformation, information, uncertain=False):
        """transformation = T_target_source, information 6x6 (order (omega, t)); -> the edge's index"""
        n = len(self._poses)
        if not (0 <= int(source) < n and 0 <= int(target) < n) or int(source) == int(target):
            raise ValueError(f"PoseGraph.add_edge: bad node pair ({source}, {target}) for {n} nodes")
        T, info = np.array(transformation, dtype=np.float64), np.array(information, dtype=np.float64)
        if T.shape != (4, 4) or info.shape != (6, 6):
            raise ValueError(f"PoseGraph.add_edge: transformation must be 4x4 and information 6x6, got {T.shape} and {info.shape}")
        self._edges.append((int(source), int(target)))
        self._T.append(T)
        self._info.append((info + info.T) / 2)  # the call wants a bitwise symmetric matrix
        self._uncertain.append(bool(uncertain))
        return len(self._edges) - 1

    poses = property(lambda self: np.array(self._poses, np.float64).reshape(-1, 4, 4))
    edges = property(lambda self: np.array(self._edges, np.int32).reshape(-1, 2))
    transformations = property(lambda self: np.array(self._T, np.float64).reshape(-1, 4, 4))
    informations = property(lambda self: np.array(self._info, np.float64).reshape(-1, 6, 6))
    uncertain = property(lambda self: np.array(self._uncertain, bool))

    def line_process_weight(self, max_translation):
        """A line_process_weight for optimize(): the chi2 of an uncertain edge that is max_translation metres off, by the mean
        diagonal of the uncertain edges' translation blocks - max_translation^2 times it.  Loop edges further off than that end
        with a weight below 1/4 and are marked not kept.  1.0 when the graph has no uncertain edge."""
        unc = self.uncertain
        if not unc.any():
            return 1.0
        info = self.informations[unc]
        return float(max_translation) ** 2 * float(np.mean([np.diag(m)[3:].mean() for m in info]))

    def optimize(self, volume, **params):
        """volume.optimize_pose_graph on the graph; the node poses become the optimised ones when the call succeeds.  -> its
        PoseGraphResult (also kept as last_result).  params: what optimize_pose_graph takes (fixed, line_process_weight, ...)."""
        res = volume.optimize_pose_graph(self.poses, self.edges, self.transformations, self.informations, self.uncertain, **params)
        self.last_result = res
        if res.success:
            self._poses = [np.array(T, np.float64) for T in np.asarray(res.poses)]
        return res

    def extrinsics(self):
        """[N,4,4] T_cw = inv(T_wc) of the nodes, ready for integrate / reintegrate_batch."""
        return _rigid_inverse(self.poses)


class KeyframeGraphRgbd:
    """A keyframe pose graph built with rgbd_odometry.

    add_frame(color, depth): every keyframe_every-th frame becomes a keyframe (the others are dropped: -> None).  The first
    keyframe is node 0 at T_wc0.  A later one is aligned as the SOURCE against the previous keyframe as the TARGET; it becomes a node
    at T_wc(previous) @ T_target_source with a certain edge (new, previous) carrying the result's transformation and information.
    When the alignment fails the node is placed at the previous keyframe's pose and joined to it by a certain edge with the identity
    and lost_information times the identity, so that the graph stays connected, and `lost` is True (lost_nodes lists them).
    -> the node's index.

    close_loops(max_distance, max_angle, min_gap): for each keyframe j and each earlier keyframe i <= j - min_gap whose current
    estimate D = inv(T_wc_i) T_wc_j has |translation| <= max_distance (metres) and rotation angle <= max_angle (radians),
    rgbd_odometry(source j, target i, init=D); a success with fitness >= min_fitness becomes an UNCERTAIN edge (j, i).  -> the new
    edges' indices.

    features: a dict of detect_features parameters ({} for the defaults).  add_frame then also detects and keeps each keyframe's
    Features - it needs `color` for that, for the depth-only method too - and close_loops_by_appearance(min_gap, min_inliers,
    inlier_threshold, max_candidates, min_fitness, **match_params) finds loops the pose estimates cannot: for each keyframe j, ONE
    segmented match_features call against the descriptors of all keyframes i <= j - min_gap; the up to max_candidates keyframes with
    the most accepted matches (at least 3; ties to the earlier one) are verified with features.backproject and
    features.rigid_from_matches(threshold = inlier_threshold metres); with min_inliers inliers or more, rgbd_odometry(source j, target
    i, init = the RANSAC pose), and a success with fitness >= min_fitness becomes an UNCERTAIN edge (j, i), as in close_loops.  Pairs
    that already share an edge are skipped.  -> the new edges' indices; appearance_log lists every verified pair
    (j, i, matches, inliers, T_ransac, edge index or None).

    The keyframes' images are kept where VisualOdometryRgbd keeps its previous frame: on the volume's GPU with keep_on_device,
    else as host arrays.  volume: context only.  odometry_params: what rgbd_odometry takes."""

    def __init__(self, volume, camera, method="hybrid", keyframe_every=1, keep_on_device=True, T_wc0=None, lost_information=1.0,
                 features=None, **odometry_params):
        if method not in METHODS:
            raise ValueError(f"KeyframeGraphRgbd: method must be one of {METHODS}, got {method!r}")
        if int(keyframe_every) < 1:
            raise ValueError(f"KeyframeGraphRgbd: keyframe_every must be at least 1, got {keyframe_every}")
        from .volumetric import PinholeCameraIntrinsic

        self.volume = volume
        self.method = method
        self.keyframe_every = int(keyframe_every)
        self.keep_on_device = keep_on_device
        self.lost_information = float(lost_information)
        self.odometry_params = dict(odometry_params)
        self.intrinsic = PinholeCameraIntrinsic(int(camera.width), int(camera.height), float(camera.fx), float(camera.fy), float(camera.cx),
                                                float(camera.cy))
        self.T_wc0 = np.eye(4) if T_wc0 is None else np.array(T_wc0, dtype=np.float64).reshape(4, 4)
        self.graph = PoseGraph()
        self.keyframes = []  # (depth, color or None) per node, where rgbd_odometry reads them
        self.feature_params = None if features is None else dict(features)
        self.features = []  # Features per node (with feature_params), where match_features reads them
        self.appearance_log = []
        self.lost_nodes = []
        self.last_result = None
        self.lost = False
        self.frames = 0

    def _place(self, a):
        a = np.ascontiguousarray(a)
        if not self.keep_on_device:
            return a
        import torch

        return torch.from_numpy(a).to(self.volume._device())

    def _align(self, source, target, init=None):
        return self.volume.rgbd_odometry(source[0], target[0], self.intrinsic, init=init, source_color=source[1], target_color=target[1],
                                         **self.odometry_params)

    def add_frame(self, color, depth):
        hybrid = self.method == "hybrid"
        if hybrid and color is None:
            raise ValueError("KeyframeGraphRgbd: the hybrid method needs the colour image")
        if self.feature_params is not None and color is None:
            raise ValueError("KeyframeGraphRgbd: features need the colour image")
        self.frames += 1
        if (self.frames - 1) % self.keyframe_every != 0:
            return None
        frame = (self._place(depth), self._place(color) if hybrid else None)
        if self.feature_params is not None:
            self.features.append(self.volume.detect_features(frame[1] if hybrid else self._place(color), **self.feature_params))
        if not self.keyframes:
            self.keyframes.append(frame)
            self.lost = False
            return self.graph.add_node(self.T_wc0)
        prev = len(self.keyframes) - 1
        res = self._align(frame, self.keyframes[prev])
        self.last_result = res
        self.lost = not res.success
        T_prev = self.graph._poses[prev]
        self.keyframes.append(frame)
        if res.success:
            node = self.graph.add_node(T_prev @ res.transformation)
            self.graph.add_edge(node, prev, res.transformation, res.information)
        else:
            node = self.graph.add_node(T_prev)
            self.graph.add_edge(node, prev, np.eye(4), self.lost_information * np.eye(6))
            self.lost_nodes.append(node)
        return node

    def candidates(self, max_distance, max_angle, min_gap):
        """The (j, i, D) close_loops tries, in the order it tries them."""
        poses = self.graph.poses
        out = []
        for j in range(len(poses)):
            for i in range(0, j - int(min_gap) + 1):
                D = _rigid_inverse(poses[i]) @ poses[j]
                angle = np.arccos(np.clip((np.trace(D[:3, :3]) - 1.0) / 2.0, -1.0, 1.0))
                if np.linalg.norm(D[:3, 3]) <= max_distance and angle <= max_angle:
                    out.append((j, i, D))
        return out

    def close_loops(self, max_distance=0.3, max_angle=0.5, min_gap=10, min_fitness=0.0):
        if int(min_gap) < 1:
            raise ValueError(f"KeyframeGraphRgbd.close_loops: min_gap must be at least 1, got {min_gap}")
        added = []
        for j, i, D in self.candidates(max_distance, max_angle, min_gap):
            res = self._align(self.keyframes[j], self.keyframes[i], init=D)
            if res.success and res.fitness >= min_fitness:
                added.append(self.graph.add_edge(j, i, res.transformation, res.information, uncertain=True))
        return added

    def close_loops_by_appearance(self, min_gap=10, min_inliers=8, inlier_threshold=0.05, max_candidates=3, min_fitness=0.0, **match_params):
        from .features import backproject, rigid_from_matches

        if self.feature_params is None:
            raise ValueError("KeyframeGraphRgbd.close_loops_by_appearance: the graph was made without features")
        if int(min_gap) < 1:
            raise ValueError(f"KeyframeGraphRgbd.close_loops_by_appearance: min_gap must be at least 1, got {min_gap}")
        host = _host
        depth_scale = float(self.odometry_params.get("depth_scale", 1.0))
        joined = {frozenset(e) for e in self.graph._edges}
        sizes = [int(f.descriptors.shape[0]) for f in self.features]
        added = []
        for j in range(len(self.features)):
            last = j - int(min_gap)
            if last < 0 or sizes[j] == 0:
                continue
            offsets = np.concatenate([[0], np.cumsum(sizes[:last + 1])]).astype(np.int32)
            if offsets[-1] == 0:
                continue
            parts = [self.features[i].descriptors for i in range(last + 1)]
            train = np.concatenate(parts) if isinstance(parts[0], np.ndarray) else _torch_cat(parts)
            res = self.volume.match_features(self.features[j].descriptors, train, segments=offsets, **match_params)
            counts, index = host(res.counts), host(res.index)
            ranked = [int(i) for i in np.argsort(-counts, kind="stable")[:int(max_candidates)] if counts[i] >= 3]
            xy_j, depth_j = host(self.features[j].xy), None
            for i in ranked:
                if frozenset((j, i)) in joined:
                    continue
                if depth_j is None:
                    depth_j = host(self.keyframes[j][0])
                hit = index[i] >= 0
                P, ok_p = backproject(xy_j[hit], depth_j, self.intrinsic, depth_scale)
                Q, ok_q = backproject(host(self.features[i].xy)[index[i][hit] - offsets[i]], host(self.keyframes[i][0]), self.intrinsic, depth_scale)
                ok = ok_p & ok_q
                T, inliers = rigid_from_matches(P[ok], Q[ok], inlier_threshold)
                entry = [j, i, int(hit.sum()), int(inliers.sum()), T, None]
                self.appearance_log.append(entry)
                if T is None or inliers.sum() < min_inliers:
                    continue
                out = self._align(self.keyframes[j], self.keyframes[i], init=T)
                if out.success and out.fitness >= min_fitness:
                    entry[5] = self.graph.add_edge(j, i, out.transformation, out.information, uncertain=True)
                    joined.add(frozenset((j, i)))
                    added.append(entry[5])
        return added

    def optimize(self, **params):
        return self.graph.optimize(self.volume, **params)

    def feature_matches(self, **match_params):
        """The accepted matches of every keyframe against its predecessors along the graph's edges: for each keyframe j ONE segmented
        match_features call against the descriptors of the keyframes i < j it shares an edge with.  -> [(i, j, matches [K,2] of
        (keypoint in i, keypoint in j))] in the order (j, i)."""
        if self.feature_params is None:
            raise ValueError("KeyframeGraphRgbd.feature_matches: the graph was made without features")
        sizes = [int(f.descriptors.shape[0]) for f in self.features]
        before = [sorted({min(e) for e in self.graph._edges if max(e) == j}) for j in range(len(self.features))]
        pairs = []
        for j, prev in enumerate(before):
            prev = [i for i in prev if sizes[i] > 0]
            if not prev or sizes[j] == 0:
                continue
            offsets = np.concatenate([[0], np.cumsum([sizes[i] for i in prev])]).astype(np.int32)
            parts = [self.features[i].descriptors for i in prev]
            train = np.concatenate(parts) if isinstance(parts[0], np.ndarray) else _torch_cat(parts)
            index = _host(self.volume.match_features(self.features[j].descriptors, train, segments=offsets, **match_params).index)
            for s, i in enumerate(prev):
                hit = np.flatnonzero(index[s] >= 0)
                pairs.append((i, j, np.stack([index[s][hit] - offsets[s], hit], -1).astype(np.int64)))
        return pairs

    def bundle_adjust(self, bf, min_length=2, rounds=10, match_params=None, **params):
        """Bundle adjustment of the keyframe poses and the points their features saw (bundle.bundle_adjust_two_phase over
        _Volume.bundle_adjust, node 0 fixed): feature_matches(**match_params), bundle.build_tracks(min_length), bundle.initial_points
        from the keyframes' depth, then the two phases of `rounds` outer iterations.  bf = baseline x fx of the depth the RGB-D
        observations are turned into (the reference's Camera.bf).  On success the poses go back into the graph, so that extrinsics()
        feeds reintegrate_batch unchanged.  -> (BundleResult, mean chi2 over the observations of the second phase); bundle_log keeps
        the tracks, the observation arrays and the active flags."""
        from . import bundle

        pairs = self.feature_matches(**(match_params or {}))
        tracks = bundle.build_tracks(pairs, min_length)
        depth_scale = float(self.odometry_params.get("depth_scale", 1.0))
        cameras = self.graph.extrinsics()
        points, index, meas, s2, keep = bundle.initial_points(tracks, self.features, [k[0] for k in self.keyframes], cameras, self.intrinsic, bf,
                                                              depth_scale)
        fixed = np.zeros(len(cameras), bool)
        fixed[0] = True
        result, active, mean = bundle.bundle_adjust_two_phase(self.volume, cameras, points, index, meas, self.intrinsic, bf, inv_sigma2=s2,
                                                              camera_fixed=fixed, rounds=rounds, **params)
        self.bundle_log = dict(tracks=[t for t, k in zip(tracks, keep) if k], points=points, index=index, measurements=meas, inv_sigma2=s2,
                               active=_host(active), cameras=cameras)
        if result.success:
            self.graph._poses = [np.array(T, np.float64) for T in _rigid_inverse(_host(result.cameras))]
        return result, mean

    def extrinsics(self):
        return self.graph.extrinsics()
