"""GPU: _Volume.detect_features (hv_orb_detect) and match_features (hv_match_descriptors) against the numpy restatement
(tests/orb_reference.py), bit for bit, at the shapes and planted inputs where the kernels change path (tests/orb_cases.py), and
every HV_ERR_INVALID case of the two entry points with untouched outputs."""
import ctypes

import numpy as np
import pytest

from pyslam_amd import _lib as L
from tests import orb_cases as oc
from tests import orb_reference as R

pytestmark = pytest.mark.gpu

HV_ERR_INVALID = -1  # include/hipvol.h, hv_status


@pytest.fixture(scope="module")
def vol():
    from pyslam_amd.volumetric import ScalableTSDFVolume

    v = ScalableTSDFVolume(0.02, 0.08, max_blocks=1 << 10)
    yield v
    v.close()


def _detect_same(vol, image, **kw):
    got = vol.detect_features(image, **kw)
    kp, desc = R.detect(image, **kw)
    assert got.keypoints.dtype == np.int32 and got.descriptors.dtype == np.uint8 and got.xy.dtype == np.float32
    np.testing.assert_array_equal(got.keypoints, kp)
    np.testing.assert_array_equal(got.descriptors, desc)
    np.testing.assert_array_equal(got.xy, R.level0_xy(kp).reshape(-1, 2))
    return kp, desc


@pytest.mark.parametrize("shape", oc.SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_detection_matches_the_restatement_at_every_shape(vol, shape):
    H, W, C = shape
    kp, _ = _detect_same(vol, oc.shaped(H, W, C, seed=H * 1000 + W))
    assert len(kp) > 0
    if (H, W) == (33, 33):
        assert kp[:, :3].tolist() == [[16, 16, 0]]  # the one candidate pixel
    if (H, W) == (65, 66):
        assert (kp[:, 2] == 0).all()  # level 1 is 32x33: nothing
    if (H, W) == (66, 66):
        assert kp[kp[:, 2] == 1][:, :2].tolist() == [[16, 16]]  # level 1 is 33x33: its one candidate


@pytest.mark.parametrize("kw", [dict(per_cell=1), dict(per_cell=16), dict(threshold=1), dict(threshold=254), dict(levels=1), dict(levels=8)],
                         ids=lambda kw: "%s%d" % next(iter(kw.items())))
def test_detection_parameters(vol, kw):
    img = oc.shaped(97, 131, 3, seed=7)
    if kw.get("threshold") == 254:
        img[37:44, 47:54] = 0
        img[40, 50] = 255  # one corner the largest threshold still finds: 255 - 0 > 254
    kp, _ = _detect_same(vol, img, **kw)
    if kw.get("threshold") == 254:
        assert [40, 50] in kp[:, 1::-1].tolist()


def test_planted_images(vol):
    kp, _ = _detect_same(vol, oc.dot())
    assert kp.tolist() == [[20, 17, 0, 16 * (100 - 20), 0]]  # a lone dot: found at its pixel, m10 = m01 = 0 takes bin 0
    kp, _ = _detect_same(vol, np.full((50, 70), 90, np.uint8))
    assert len(kp) == 0  # the constant image
    kp, _ = _detect_same(vol, oc.periodic(), levels=1)
    inner = kp[(kp[:, 0] // 32 == 1) & (kp[:, 1] // 32 == 1)]  # the cell wholly inside the candidate region: 16 equal scores
    assert len(set(kp[:, 3].tolist())) == 1 and inner[:, :2].tolist() == [[x, y] for y in (36, 44) for x in (36, 44, 52, 60)]
    kp, _ = _detect_same(vol, oc.adjacent_pair(), levels=1)
    assert kp[:, :2].tolist() == [[22, 20]]  # the F5 tie: the earlier of the two
    kp, _ = _detect_same(vol, oc.orientation_tie(), levels=1)
    y, x = oc.TIE_CENTRE
    centre = kp[(kp[:, 0] == x) & (kp[:, 1] == y)]
    assert len(centre) == 1 and centre[0, 4] == 0  # the F8 tie: the smaller bin


def test_device_tensors_agree_with_host_arrays(vol):
    import torch

    img = oc.shaped(97, 131, 3, seed=3)
    host = vol.detect_features(img)
    dev = vol.detect_features(torch.from_numpy(img).cuda())
    assert dev.keypoints.is_cuda and dev.descriptors.is_cuda and dev.xy.is_cuda
    for a, b in zip(dev, host):
        np.testing.assert_array_equal(a.cpu().numpy(), b)
    q, t = oc.descriptor_sets(65, 257, seed=2)
    seg = np.array([0, 1, 1, 130, 257], np.int32)
    host = vol.match_features(q, t, segments=seg)
    dev = vol.match_features(torch.from_numpy(q).cuda(), torch.from_numpy(t).cuda(), segments=seg)
    for a, b in zip(dev, host):
        assert a.is_cuda
        np.testing.assert_array_equal(a.cpu().numpy().astype(b.dtype), b)


def _match_same(vol, q, t, segments=None, max_distance=64, ratio=0.8, cross_check=True):
    got = vol.match_features(q, t, segments=segments, max_distance=max_distance, ratio=ratio, cross_check=cross_check)
    want = R.match(q, t, segments, max_distance, 0 if ratio is None else int(round(100 * ratio)), int(cross_check))
    assert got.index.dtype == np.int32 and got.distance.dtype == np.uint16 and got.second.dtype == np.uint16 and got.counts.dtype == np.int32
    for a, b, name in zip(got, want, ("index", "distance", "second", "counts")):
        np.testing.assert_array_equal(a, b, err_msg=name)
    return got


@pytest.mark.parametrize("sizes", [(1, 1), (65, 257), (300, 1000)], ids=lambda s: "%dx%d" % s)
def test_matching_matches_the_restatement(vol, sizes):
    q, t = oc.descriptor_sets(*sizes, seed=sum(sizes))
    got = _match_same(vol, q, t)
    if sizes[0] > 1:
        assert got.counts[0] > 0


def test_matching_segments(vol):
    q, t = oc.descriptor_sets(65, 257, seed=5)
    got = _match_same(vol, q, t, segments=np.array([0, 1, 1, 130, 257], np.int32))  # one descriptor, none, boundaries off the tile
    assert (got.second[0] == 65535).all() and (got.distance[1] == 65535).all() and (got.index[1] == -1).all() and got.counts[1] == 0
    q, t = oc.descriptor_sets(300, 64 * 37, seed=6)
    _match_same(vol, q, t, segments=np.arange(65, dtype=np.int32) * 37)  # S = 64


@pytest.mark.parametrize("kw", [dict(max_distance=0), dict(max_distance=256), dict(ratio=None), dict(ratio=1.0), dict(cross_check=False),
                                dict(max_distance=256, ratio=None, cross_check=False)],
                         ids=["max0", "max256", "ratio0", "ratio100", "no_cross_check", "everything_off"])
def test_matching_rule_switches(vol, kw):
    q, t = oc.descriptor_sets(130, 300, seed=8)
    _match_same(vol, q, t, segments=np.array([0, 100, 300], np.int32), **kw)


def test_matching_planted_ties(vol):
    q, t = oc.descriptor_sets(40, 50, seed=9)
    # duplicate train descriptors: the smallest index wins, and d2 == d1 rejects under the ratio
    t[30] = t[7] = q[3]
    got = _match_same(vol, q, t)
    assert got.distance[0, 3] == 0 and got.second[0, 3] == 0 and got.index[0, 3] == -1
    got = _match_same(vol, q, t, ratio=None)
    assert got.index[0, 3] == 7
    # duplicate queries: the M4 tie goes to the smaller query index
    q[11] = q[3]
    got = _match_same(vol, q, t, ratio=None)
    assert got.index[0, 3] == 7 and got.index[0, 11] == -1 and got.distance[0, 11] == 0
    # all-zero against all-ones: distance 256
    got = _match_same(vol, np.zeros((2, 32), np.uint8), np.full((3, 32), 255, np.uint8), max_distance=256, ratio=None)
    assert (got.distance == 256).all() and (got.second == 256).all() and got.index[0].tolist() == [0, -1]


# ---- refusals of the C entry points: HV_ERR_INVALID, outputs untouched ------------------------------------------------------------

def _detect_raw(vol, img, H, W, C, prm, kp, desc, cap, count, null=()):
    p = lambda name, a: None if name in null else L.ptr(a)  # noqa: E731
    return vol._lib.hv_orb_detect(vol._h, p("image", img), H, W, C, None if "params" in null else ctypes.byref(prm), p("keypoints", kp),
                                  p("descriptors", desc), cap, None if "count" in null else ctypes.byref(count), L.HV_HOST)


def test_detect_refusals_touch_nothing(vol):
    img = oc.shaped(64, 64, 1)
    cap = R.capacity(64, 64, 3, 8)
    assert cap == 4 * 8  # (level 1 is 32x32: it yields nothing)

    def attempt(H=64, W=64, C=1, levels=3, threshold=20, per_cell=8, capacity=cap, null=()):
        kp, desc, count = np.full((cap, 5), -7, np.int32), np.full((cap, 32), 0xA5, np.uint8), ctypes.c_int32(-7)
        rc = _detect_raw(vol, img, H, W, C, L.HvFeatureParams(levels, threshold, per_cell), kp, desc, capacity, count, null)
        assert rc == HV_ERR_INVALID, (rc, H, W, C, levels, threshold, per_cell, capacity, null)
        assert (kp == -7).all() and (desc == 0xA5).all() and count.value == -7

    for name in ("image", "params", "keypoints", "descriptors", "count"):
        attempt(null=(name,))
    for C in (0, 2, 4):
        attempt(C=C)
    for H, W in ((0, 64), (64, 0), (-1, 64), (32769, 64), (64, 32769)):
        attempt(H=H, W=W)
    for levels in (0, 9):
        attempt(levels=levels)
    for threshold in (0, 255):
        attempt(threshold=threshold)
    for per_cell in (0, 17):
        attempt(per_cell=per_cell)
    attempt(capacity=cap - 1)
    kp, desc, count = np.full((cap, 5), -7, np.int32), np.full((cap, 32), 0xA5, np.uint8), ctypes.c_int32(-7)
    assert _detect_raw(vol, img, 64, 64, 1, L.HvFeatureParams(3, 20, 8), kp, desc, cap, count) == L.HV_OK and count.value > 0


def test_match_refusals_touch_nothing(vol):
    q, t = oc.descriptor_sets(5, 9, seed=1)
    good = np.array([0, 4, 9], np.int32)

    def attempt(nq=5, nt=9, seg=good, S=2, prm=(64, 80, 1), null=(), ok=False):
        idx, d1, d2, cnt = np.full((2, 5), -7, np.int32), np.full((2, 5), 7, np.uint16), np.full((2, 5), 7, np.uint16), np.full(2, -7, np.int32)
        p = lambda name, a: None if name in null else L.ptr(a)  # noqa: E731
        rc = vol._lib.hv_match_descriptors(vol._h, p("query", q), nq, p("train", t), nt, p("offsets", seg), S,
                                           None if "params" in null else ctypes.byref(L.HvMatchParams(*prm)), p("index", idx), L.ptr(d1),
                                           L.ptr(d2), L.ptr(cnt), L.HV_HOST)
        if ok:
            assert rc == L.HV_OK and (idx != -7).all() and (cnt >= 0).all()
            return
        assert rc == HV_ERR_INVALID, (rc, nq, nt, seg, S, prm, null)
        assert (idx == -7).all() and (d1 == 7).all() and (d2 == 7).all() and (cnt == -7).all()

    for name in ("query", "train", "offsets", "params", "index"):
        attempt(null=(name,))
    for nq in (0, -1, 65537):
        attempt(nq=nq)
    for nt in (-1, 1 << 24):
        attempt(nt=nt)
    attempt(S=0)
    attempt(nq=65536, S=2048, seg=np.zeros(2049, np.int32), nt=0)  # S Nq = 2^27
    for prm in ((-1, 80, 1), (257, 80, 1), (64, -1, 1), (64, 101, 1), (64, 80, 2), (64, 80, -1)):
        attempt(prm=prm)
    for seg in ([1, 4, 9], [0, 4, 8], [0, 4, 10], [0, 10, 9]):
        attempt(seg=np.array(seg, np.int32))
    attempt(ok=True)
