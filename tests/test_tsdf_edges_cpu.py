"""CPU side of the TSDF edge cases (tests/test_gpu_tsdf_edges.py holds the GPU side).

* The operand normalisation of ScalableTSDFVolume.integrate / integrate_batch / integrate_frames (volumetric._tsdf_operands):
  what reaches the library is Open3D's Image layout - contiguous float32 or uint16 depth, contiguous uint8 RGB - for numpy
  arrays and host torch tensors alike, without a copy when the operand already has it; everything else is refused before
  any library call.  The entry points run here against a recording stand-in for the library (no GPU).
* oracle/tsdf_oracle.c held to the closed-form evaluator (tests/tsdf_closed_form.py) at an odd image size with an off-centre
  principal point and fx != fy, at depth sampling strides 1 and 3: the GPU edge tests trust the oracle at such cameras.
"""
import ctypes
import os

import numpy as np
import pytest

import oracle
from pyslam_amd import _lib as L
from pyslam_amd.volumetric import PinholeCameraIntrinsic, RGBDImage, ScalableTSDFVolume, _tsdf_operands
from tests import tsdf_closed_form as cf
from tests.recording_lib import RecordingLib

H, W = 7, 9
K = PinholeCameraIntrinsic(W, H, 8.0, 7.0, 3.3, 4.1)
UNSUPPORTED = "Unsupported image format"


def _frames(F=None, seed=0):
    rng = np.random.default_rng(seed)
    lead = () if F is None else (F,)
    depth = (0.5 + 3.0 * rng.random(lead + (H, W))).astype(np.float32)
    color = rng.integers(0, 256, lead + (H, W, 3)).astype(np.uint8)
    return depth, color


def _addr(a):
    return a.data_ptr() if hasattr(a, "data_ptr") and not isinstance(a, np.ndarray) else a.ctypes.data


# ---- the helper -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [None, 3])
def test_operands_in_the_library_layout_are_passed_through_without_a_copy(F):
    torch = pytest.importorskip("torch")
    depth, color = _frames(F)
    for d, c in ((depth, color), (depth.astype(np.uint16), color), (torch.from_numpy(depth), torch.from_numpy(color)),
                 (torch.from_numpy(depth.astype(np.uint16)), torch.from_numpy(color))):
        od, oc, kind, converted = _tsdf_operands(d, c, K, frames=F)
        assert od is d and oc is c and not converted
        assert kind == (L.HV_DEPTH_U16 if str(d.dtype) in ("uint16", "torch.uint16") else L.HV_DEPTH_F32)


@pytest.mark.parametrize("F", [None, 2])
def test_wrong_layouts_become_the_canonical_arrays(F):
    """A cropped view of a larger depth map, an RGBA buffer sliced to RGB, float64 / integer depth: converted on the host into
    exactly the canonical float32 / uint8 arrays (uint16 depth stays uint16)."""
    depth, color = _frames(F)
    lead = () if F is None else (F,)
    big = np.zeros(lead + (H + 3, W + 5), np.float32)
    big[..., 1:1 + H, 2:2 + W] = depth
    rgba = np.full(lead + (H, W, 4), 77, np.uint8)
    rgba[..., :3] = color
    cases = [(big[..., 1:1 + H, 2:2 + W], rgba[..., :3], depth, L.HV_DEPTH_F32),
             (depth.astype(np.float64), color, depth.astype(np.float64).astype(np.float32), L.HV_DEPTH_F32),
             (np.rint(depth * 1000).astype(np.int32), color, np.rint(depth * 1000).astype(np.float32), L.HV_DEPTH_F32),
             (np.rint(depth * 1000).astype(np.uint16)[..., ::-1][..., ::-1], color[..., ::1, :], np.rint(depth * 1000).astype(np.uint16),
              L.HV_DEPTH_U16),
             (np.asfortranarray(depth), np.asfortranarray(color), depth, L.HV_DEPTH_F32)]
    for d, c, want, kind in cases:
        od, oc, k, converted = _tsdf_operands(d, c, K, frames=F)
        assert isinstance(od, np.ndarray) and od.flags.c_contiguous and oc.flags.c_contiguous and not converted
        assert k == kind and od.dtype == want.dtype and oc.dtype == np.uint8
        np.testing.assert_array_equal(od, want)
        np.testing.assert_array_equal(oc, color)


def test_host_torch_tensors_are_normalised_like_numpy():
    torch = pytest.importorskip("torch")
    depth, color = _frames(2)
    td = torch.from_numpy(depth.astype(np.float64))
    rgba = torch.zeros((2, H, W, 4), dtype=torch.uint8)
    rgba[..., :3] = torch.from_numpy(color)
    big = torch.zeros((2, H + 2, W + 3), dtype=torch.float32)
    big[:, 2:, 3:] = torch.from_numpy(depth)
    for d, c in ((td, rgba[..., :3]), (big[:, 2:, 3:], torch.from_numpy(color)), (torch.from_numpy(depth).half(), rgba[..., :3])):
        od, oc, kind, converted = _tsdf_operands(d, c, K, frames=2)
        assert od.dtype == torch.float32 and oc.dtype == torch.uint8 and kind == L.HV_DEPTH_F32 and not converted
        assert od.is_contiguous() and oc.is_contiguous() and od.device.type == "cpu"
        np.testing.assert_array_equal(od.numpy(), d.to(torch.float32).numpy())
        np.testing.assert_array_equal(oc.numpy(), color)
    # a host tensor beside a numpy array is accepted (both are host memory)
    od, oc, _, _ = _tsdf_operands(torch.from_numpy(depth), color, K, frames=2)
    assert _addr(od) == _addr(torch.from_numpy(depth)) or np.array_equal(od.numpy(), depth)


def test_operands_that_do_not_fit_are_refused():
    torch = pytest.importorskip("torch")
    depth, color = _frames(2)
    rgba = np.zeros((2, H, W, 4), np.uint8)
    bad = [
        (depth, rgba, K, 2),                                        # 4 channels
        (depth, color[:, :, :-1], K, 2),                            # colour of another size
        (depth, color.astype(np.float32), K, 2),                    # colour not uint8
        (depth, color[..., 0], K, 2),                               # grey
        (depth, color, PinholeCameraIntrinsic(W + 1, H, 8.0, 7.0, 3.3, 4.1), 2),
        (depth, color, PinholeCameraIntrinsic(W, H - 1, 8.0, 7.0, 3.3, 4.1), 2),
        (depth, color, K, 3),                                       # frame count
        (depth[0], color[0], K, 2),                                 # a single frame where a batch is expected
        (depth, color, K, None),                                    # a batch where a frame is expected
        (depth.astype(bool), color, K, 2),
        (depth.astype(np.complex64), color, K, 2),
        (torch.from_numpy(depth).to(torch.complex64), torch.from_numpy(color), K, 2),
        (torch.from_numpy(depth), torch.from_numpy(color).float(), K, 2),
        (torch.from_numpy(depth) > 1, torch.from_numpy(color), K, 2),
    ]
    for d, c, k, F in bad:
        with pytest.raises(RuntimeError, match=UNSUPPORTED):
            _tsdf_operands(d, c, k, frames=F)


# ---- the entry points against a recording stand-in for the library -------------------------------------------------------
def _volume():
    vol = ScalableTSDFVolume.__new__(ScalableTSDFVolume)  # no hv_create: nothing here needs a device
    vol._lib = RecordingLib()
    vol._h = None
    return vol


def _p(arg):
    return arg.value if isinstance(arg, ctypes.c_void_p) else arg


def test_integrate_hands_the_library_the_normalised_operands():
    depth, color = _frames()
    vol = _volume()
    big = np.zeros((H + 1, W + 2), np.float64)
    big[:H, :W] = depth
    rgba = np.zeros((H, W, 4), np.uint8)
    rgba[..., :3] = color
    vol.integrate(RGBDImage(rgba[..., :3], big[:H, :W], 1.0, 4.0), K, np.eye(4))
    (name, args), = vol._lib.calls
    assert name == "hv_tsdf_integrate" and args[2] == L.HV_DEPTH_F32 and args[4:6] == (H, W)
    kept_depth, kept_color = vol._inflight[1:]
    assert _p(args[1]) == kept_depth.ctypes.data and _p(args[3]) == kept_color.ctypes.data
    np.testing.assert_array_equal(kept_depth, depth)
    np.testing.assert_array_equal(kept_color, color)
    # canonical operands: the caller's own buffers
    vol.integrate(RGBDImage(color, depth, 1.0, 4.0), K, np.eye(4))
    assert _p(vol._lib.calls[-1][1][1]) == depth.ctypes.data and _p(vol._lib.calls[-1][1][3]) == color.ctypes.data


def test_integrate_batch_and_frames_normalise_and_refuse_before_the_library():
    depth, color = _frames(3)
    T = np.tile(np.eye(4), (3, 1, 1))
    vol = _volume()
    vol.integrate_batch(depth.astype(np.float64), color, K, T, depth_scale=1.0, depth_trunc=4.0)
    (name, args), = vol._lib.calls
    assert name == "hv_tsdf_integrate_batch" and args[2] == L.HV_DEPTH_F32 and args[4:7] == (3, H, W)
    assert _p(args[1]) == vol._inflight[1].ctypes.data and vol._inflight[1].dtype == np.float32
    vol.integrate_batch(depth, color, K, T)
    assert _p(vol._lib.calls[-1][1][1]) == depth.ctypes.data  # no copy of a canonical batch
    # zero frames: no call at all
    vol.integrate_batch(depth[:0], color[:0], K, T[:0])
    vol.integrate_frames([], [], K, T[:0])
    assert len(vol._lib.calls) == 2
    for args in ((depth, color, K, T[:2]), (depth, color, K, np.tile(np.eye(4), (4, 1, 1))), (depth, color[:2], K, T),
                 (depth, np.zeros((3, H, W, 4), np.uint8), K, T), (depth, color, PinholeCameraIntrinsic(W, H + 1, 1, 1, 0, 0), T),
                 (depth[0], color[0], K, T[0])):
        with pytest.raises(RuntimeError, match=UNSUPPORTED):
            vol.integrate_batch(*args)
        with pytest.raises(RuntimeError, match=UNSUPPORTED):
            vol.integrate_frames(list(args[0]) if args[0].ndim == 3 else [args[0]], list(args[1]) if args[1].ndim == 4 else [args[1]],
                                 args[2], args[3])
    with pytest.raises(RuntimeError, match=UNSUPPORTED):  # mixed depth types in one call
        vol.integrate_frames([depth[0], depth[1].astype(np.uint16)], [color[0], color[1]], K, T[:2])
    with pytest.raises(RuntimeError, match=UNSUPPORTED):
        vol.integrate(RGBDImage(color[0][:, :-1], depth[0], 1.0, 4.0), K, np.eye(4))
    assert len(vol._lib.calls) == 2
    # integrate_frames: every frame normalised on its own, pointers to the normalised arrays
    rgba = np.zeros((3, H, W, 4), np.uint8)
    rgba[..., :3] = color
    vol.integrate_frames([d.astype(np.float64) for d in depth], [c for c in rgba[..., :3]], K, T)
    name, args = vol._lib.calls[-1]
    assert name == "hv_tsdf_integrate_frames" and args[2] == L.HV_DEPTH_F32 and args[4:7] == (3, H, W)
    for f, (d, c) in enumerate(vol._lib.frames):
        np.testing.assert_array_equal(d, depth[f])
        np.testing.assert_array_equal(c, color[f])


# ---- the oracle held to the closed form at an odd camera -----------------------------------------------------------------
ODD_W, ODD_H = 161, 119
ODD_K = (525.0 * ODD_W / 640 * 1.03, 525.0 * ODD_W / 640 * 0.97, 0.37 * ODD_W, 0.61 * ODD_H)


@pytest.mark.parametrize("stride", [1, 3])
def test_oracle_equals_the_closed_form_at_an_odd_camera(stride):
    cam = cf.camera(ODD_W, ODD_H, ODD_K, stride)
    fr = cf.frames(cam)
    assert all(d.shape == (ODD_H, ODD_W) and (d > 0).mean() > 0.9 for d, _, _ in fr)
    ref = cf.evaluate(fr, cam=cam)
    vol = oracle.PortTsdf(cf.VOXEL, cf.TRUNC, depth_sampling_stride=stride, threads=min(16, os.cpu_count() or 1))
    for d, c, T in fr:
        vol.integrate(d, c, np.asarray(ODD_K), T, 1.0, cf.DEPTH_TRUNC)
    stats = cf.compare(vol.dump(), ref, f"oracle/tsdf_oracle.c {ODD_W}x{ODD_H} stride {stride}")
    assert stats["units"] > 2000 and stats["max_weight"] == 3 and stats["updated"] > 5_000_000
    assert stats["fragile_frac"] < 0.05
