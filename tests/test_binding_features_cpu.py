"""What detect_features and match_features send over the C ABI, pinned against the recording stand-in for the library
(tests/recording_lib.py; no GPU), in the manner of tests/test_binding_stereo_cpu.py, whose list of exercised public methods these
tests extend; and the feature bookkeeping of KeyframeGraphRgbd that needs no library."""
import ctypes
import types

import numpy as np
import pytest

from pyslam_amd import _lib as L
from pyslam_amd import volumetric as V
from pyslam_amd import volumetric_semantic as S
from tests.recording_lib import ref, volume
from tests.test_binding_calls_cpu import ANY, P, REF, covers, expect, host, refused, shaped, tsdf  # noqa: F401 (host: a fixture)

H, W = 40, 70  # 2 x 3 cells at level 0; level 1 is 20 x 35: it yields nothing
I32 = ctypes.c_int32


def image(channels=3, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (H, W) if channels == 1 else (H, W, channels), dtype=np.uint8)


def fields(struct):
    return {name: getattr(struct, name) for name, _ in struct._fields_}


def test_structs_mirror_the_header():
    assert [n for n, _ in L.HvFeatureParams._fields_] == ["levels", "threshold", "per_cell"] and ctypes.sizeof(L.HvFeatureParams) == 12
    assert [n for n, _ in L.HvMatchParams._fields_] == ["max_distance", "ratio_percent", "cross_check"] and ctypes.sizeof(L.HvMatchParams) == 12


def test_feature_capacity_counts_the_cells_of_the_yielding_levels():
    assert V.feature_capacity(33, 33, 3, 8) == 4 * 8 and V.feature_capacity(32, 200, 3, 8) == 0
    assert V.feature_capacity(66, 66, 8, 2) == (9 + 4) * 2 and V.feature_capacity(65, 66, 8, 2) == 9 * 2
    assert V.feature_capacity(480, 640, 3, 8) == (300 + 80 + 20) * 8 and V.feature_capacity(480, 640, 1, 16) == 300 * 16


@pytest.mark.parametrize("channels", [1, 3])
@covers("detect_features")
def test_detect_features_defaults_and_result_kinds(channels):
    img = image(channels)
    for vol in (tsdf(), volume(V.VoxelBlockGrid, voxel_size=0.05, block_size=8), volume(S.VoxelBlockSemanticGrid, voxel_size=0.05, block_size=8)):
        vol._lib.script("hv_orb_detect", 3)
        out = vol.detect_features(img)
        call, = expect(vol, ("hv_orb_detect", P(img), H, W, channels, REF(L.HvFeatureParams), P(out.keypoints), P(out.descriptors), 48, REF(I32),
                             L.HV_HOST))
        assert isinstance(out, V.Features) and fields(ref(call[1][5])) == dict(levels=3, threshold=20, per_cell=8)
        shaped(out.keypoints, (3, 5), np.int32), shaped(out.descriptors, (3, 32), np.uint8), shaped(out.xy, (3, 2), np.float32)
        assert out.keypoints.base.shape == (48, 5) and out.descriptors.base.shape == (48, 32)  # sized to the bound, cut to the count


@covers("detect_features")
def test_detect_features_marshals_every_argument(host):
    img = image()
    vol = tsdf()
    out = vol.detect_features(host(img), levels=np.int64(1), threshold=7, per_cell=np.int32(16))
    call, = expect(vol, ("hv_orb_detect", P(img), H, W, 3, REF(L.HvFeatureParams), P(out.keypoints.base), P(out.descriptors.base), 96, REF(I32),
                         L.HV_HOST))
    assert fields(ref(call[1][5])) == dict(levels=1, threshold=7, per_cell=16) and all(type(x) is int for x in call[1][2:5] + (call[1][8],))
    shaped(out.keypoints, (0, 5), np.int32), shaped(out.xy, (0, 2), np.float32)  # the stand-in counts nothing
    # a strided view is made contiguous for the call; an image too small for any level still gets arrays of one row
    wide = np.zeros((H, 2 * W), np.uint8)
    vol.detect_features(wide[:, ::2])
    expect(vol, ("hv_orb_detect", ANY, H, W, 1, REF(L.HvFeatureParams), ANY, ANY, 48, REF(I32), L.HV_HOST))
    vol.detect_features(np.zeros((20, 90), np.uint8))
    expect(vol, ("hv_orb_detect", ANY, 20, 90, 1, REF(L.HvFeatureParams), ANY, ANY, 1, REF(I32), L.HV_HOST))
    # the level-0 position: ((x + 0.5) 2^level - 0.5, (y + 0.5) 2^level - 0.5)
    kp = np.array([[16, 17, 0, 9, 0], [16, 17, 1, 9, 3], [20, 30, 2, 9, 31]], np.int32)
    assert ((kp[:, :2] + 0.5) * 2.0 ** kp[:, 2:3] - 0.5).tolist() == [[16.0, 17.0], [32.5, 34.5], [81.5, 121.5]]


@covers("detect_features")
def test_detect_features_refusals_come_before_any_call():
    img = image()
    vol = tsdf()
    for bad in (0, 9, -1, 2.5):
        refused(vol, ValueError, "detect_features: levels must be an integer in 1..8", vol.detect_features, img, levels=bad)
    for bad in (0, 255):
        refused(vol, ValueError, "detect_features: threshold must be an integer in 1..254", vol.detect_features, img, threshold=bad)
    for bad in (0, 17):
        refused(vol, ValueError, "detect_features: per_cell must be an integer in 1..16", vol.detect_features, img, per_cell=bad)
    refused(vol, ValueError, "detect_features: images must have 1 or 3 channels, got 2", vol.detect_features, img[..., :2])
    refused(vol, ValueError, "detect_features: height and width must be in 1..32768", vol.detect_features, img[:0])
    refused(vol, ValueError, "detect_features: height and width must be in 1..32768", vol.detect_features, np.zeros((1, 32769), np.uint8))
    refused(vol, ValueError, "detect_features: the image must be [H,W] or [H,W,3]", vol.detect_features, img.ravel())
    refused(vol, ValueError, "detect_features: the image must be uint8", vol.detect_features, img.astype(np.float32))


def sets(nq=5, nt=9, seed=0):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (nq, 32), dtype=np.uint8), rng.integers(0, 256, (nt, 32), dtype=np.uint8)


@covers("match_features")
def test_match_features_defaults_and_result_kinds():
    q, t = sets()
    for vol in (tsdf(), volume(V.VoxelBlockGrid, voxel_size=0.05, block_size=8), volume(S.VoxelBlockSemanticGrid, voxel_size=0.05, block_size=8)):
        vol._lib.script("hv_match_descriptors", peek={5: (np.int32, 2)})
        out = vol.match_features(q, t)
        call, = expect(vol, ("hv_match_descriptors", P(q), 5, P(t), 9, ANY, 1, REF(L.HvMatchParams), P(out.index), P(out.distance), P(out.second),
                             P(out.counts), L.HV_HOST))
        assert isinstance(out, V.MatchResult) and fields(ref(call[1][7])) == dict(max_distance=64, ratio_percent=80, cross_check=1)
        assert vol._lib.peeked[-1][5].tolist() == [0, 9]  # no segments: one, all of train
        shaped(out.index, (1, 5), np.int32), shaped(out.distance, (1, 5), np.uint16), shaped(out.second, (1, 5), np.uint16)
        shaped(out.counts, (1,), np.int32)


@covers("match_features")
def test_match_features_marshals_every_argument(host):
    q, t = sets()
    vol = tsdf()
    vol._lib.script("hv_match_descriptors", peek={5: (np.int32, 4)})
    out = vol.match_features(host(q), host(t), segments=[0, 4, 4, 9], max_distance=np.int64(256), ratio=None, cross_check=False)
    call, = expect(vol, ("hv_match_descriptors", P(q), 5, P(t), 9, ANY, 3, REF(L.HvMatchParams), P(out.index), P(out.distance), P(out.second),
                         P(out.counts), L.HV_HOST))
    assert fields(ref(call[1][7])) == dict(max_distance=256, ratio_percent=0, cross_check=0) and vol._lib.peeked[-1][5].tolist() == [0, 4, 4, 9]
    shaped(out.index, (3, 5), np.int32), shaped(out.counts, (3,), np.int32)
    for ratio, percent in ((0.7, 70), (1.0, 100), (0.0, 0), (0.754, 75)):
        vol.match_features(q, t, segments=np.array([0, 9], np.int64), ratio=ratio)
        call, = expect(vol, ("hv_match_descriptors", P(q), 5, P(t), 9, ANY, 1, REF(L.HvMatchParams), ANY, ANY, ANY, ANY, L.HV_HOST))
        assert fields(ref(call[1][7]))["ratio_percent"] == percent
    # no train descriptor at all: a null pointer and one empty segment
    vol.match_features(q, t[:0])
    expect(vol, ("hv_match_descriptors", P(q), 5, None, 0, ANY, 1, REF(L.HvMatchParams), ANY, ANY, ANY, ANY, L.HV_HOST))


@covers("match_features")
def test_match_features_refusals_come_before_any_call():
    q, t = sets()
    vol = tsdf()
    refused(vol, ValueError, "match_features: the descriptors must be uint8", vol.match_features, q.astype(np.int32), t)
    refused(vol, ValueError, "must be [N,32]", vol.match_features, q[:, :31], t)
    refused(vol, ValueError, "must be [N,32]", vol.match_features, q, t.ravel())
    refused(vol, ValueError, "match_features: need 1..65536 query descriptors, got 0", vol.match_features, q[:0], t)
    refused(vol, ValueError, "match_features: need 1..65536 query descriptors", vol.match_features, np.zeros((65537, 32), np.uint8), t)
    for bad in ([1, 9], [0, 8], [0, 5, 4, 9], [0, 10]):
        refused(vol, ValueError, "match_features: segments must not decrease, start at 0 and end at 9", vol.match_features, q, t, segments=bad)
    refused(vol, ValueError, "match_features: segments must be a 1-D integer array", vol.match_features, q, t, segments=[9])
    refused(vol, ValueError, "match_features: segments must be a 1-D integer array", vol.match_features, q, t, segments=[0.0, 9.0])
    refused(vol, ValueError, "match_features: segments times queries must stay below 2^27", vol.match_features, np.zeros((4096, 32), np.uint8), t[:0],
            segments=np.zeros((1 << 15) + 1, np.int32))
    for bad in (-1, 257, 1.5):
        refused(vol, ValueError, "match_features: max_distance must be an integer in 0..256", vol.match_features, q, t, max_distance=bad)
    for bad in (-0.1, 1.01):
        refused(vol, ValueError, "match_features: ratio must be in 0..1 or None", vol.match_features, q, t, ratio=bad)


def test_keyframe_graph_keeps_features_only_when_asked():
    from pyslam_amd.pose_graph import KeyframeGraphRgbd

    cam = types.SimpleNamespace(fx=30.0, fy=31.0, cx=34.5, cy=19.5, width=W, height=H)
    depth, color = np.ones((H, W), np.float32), image()
    vol = tsdf()
    plain = KeyframeGraphRgbd(vol, cam, method="point_to_plane", keep_on_device=False)
    assert plain.add_frame(None, depth) == 0 and plain.features == [] and vol._lib.calls == []
    with pytest.raises(ValueError, match="made without features"):
        plain.close_loops_by_appearance()
    kg = KeyframeGraphRgbd(vol, cam, method="point_to_plane", keep_on_device=False, features=dict(per_cell=4))
    with pytest.raises(ValueError, match="features need the colour image"):
        kg.add_frame(None, depth)
    vol._lib.script("hv_orb_detect", 2)
    assert kg.add_frame(color, depth) == 0
    call, = expect(vol, ("hv_orb_detect", ANY, H, W, 3, REF(L.HvFeatureParams), ANY, ANY, 24, REF(I32), L.HV_HOST))
    assert fields(ref(call[1][5]))["per_cell"] == 4 and len(kg.features) == 1 and kg.features[0].descriptors.shape == (2, 32)
    assert kg.close_loops_by_appearance(min_gap=1) == [] and vol._lib.calls == []  # one keyframe: nothing to match against
