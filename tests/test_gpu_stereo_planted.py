"""GPU: _Volume.stereo_sgm (hv_stereo_sgm) on the planted pairs of tests/stereo_cases.py (PLANTED) against the numpy restatement
(tests/stereo_reference.py), bit for bit - the int16 disparity with assert_array_equal, the depth as uint32 views.  The pairs reach
what the shapes of tests/test_gpu_stereo.py do not: winners and path minima in every row of 16 lanes and every slot of a lane, rows
of two and three tiles of the winner kernel, every residue of the number of path starts, rule 6 at equality, a winner left of the
image, depth cuts met exactly (tests/test_stereo_planted_cpu.py counts all of that and proves which wrong reading each pair tells
from the right one).  One volume serves every case, in the order of the list: its scratch buffer grows and is reused.

The device form runs on non-contiguous CUDA tensors made by a torch operation queued just before the call, on torch's default
stream, inside ``with torch.cuda.stream(side)`` behind pending work, and on the stream adopt_torch_stream() hands back; the results
are consumed by .clone() right after the call.  As tests/test_gpu_binding_streams.py says: a stream-ordering mistake is a race,
these tests can catch one, they cannot prove there is none.  Each runs once per setting."""
import contextlib
import ctypes
import functools

import numpy as np
import pytest

from pyslam_amd import _lib as L
from tests import stereo_cases as sc
from tests import stereo_reference as sr

pytestmark = pytest.mark.gpu

SETTINGS = ("default", "side", "adopted")
DEVICE_CASES = ("wide_3x513_D256", "stair_D64_rgb")
FARTHEST = "stair_D256"  # the case with the largest disparities


def runs():
    """(name, paths): every case with its own parameters, and with the other number of paths where its events survive that."""
    out = []
    for name, _, _, params in sc.PLANTED:
        out.append((name, params["paths"]))
        if name not in sc.OWN_PATHS:
            out.append((name, 12 - params["paths"]))
    return out


@functools.lru_cache(maxsize=None)
def restated(name, paths):
    """The restatement's (disparity, depth) of a case, computed once and read-only."""
    left, right, params = sc.planted(name)
    want = sr.stereo_sgm(left, right, **{**params, "paths": paths})
    for a in want:
        a.setflags(write=False)
    return want


@pytest.fixture(scope="module")
def vol():
    from pyslam_amd.volumetric import ScalableTSDFVolume

    v = ScalableTSDFVolume(0.02, 0.08, max_blocks=1 << 10)
    yield v
    v.close()


@pytest.fixture(scope="module")
def adopted():
    from pyslam_amd.volumetric import ScalableTSDFVolume

    v = ScalableTSDFVolume(0.02, 0.08, max_blocks=1 << 10)
    v.adopt_torch_stream()
    yield v
    v.close()


@pytest.fixture(scope="module")
def side():
    import torch

    return torch.cuda.Stream(torch.device("cuda", 0))


@pytest.fixture(scope="module")
def filler():
    import torch

    return torch.ones((2048, 2048), device=torch.device("cuda", 0))


def _same(got, want):
    (disp, depth), (rdisp, rdepth) = got, want
    assert disp.dtype == np.int16 and disp.shape == rdisp.shape
    np.testing.assert_array_equal(disp, rdisp)
    assert depth.dtype == np.float32 and depth.shape == rdepth.shape
    np.testing.assert_array_equal(depth.view(np.uint32), rdepth.view(np.uint32))


@pytest.mark.parametrize("name,paths", runs(), ids=lambda v: str(v))
def test_planted_case_matches_the_restatement(vol, name, paths):
    left, right, params = sc.planted(name)
    _same(vol.stereo_sgm(left, right, **{**params, "paths": paths}), restated(name, paths))


@contextlib.contextmanager
def setting(name, volume, side, filler):
    """Torch's current stream for one comparison; the side and adopted streams have work pending when the matcher is called."""
    import torch

    if name == "default":
        yield
    else:
        with torch.cuda.stream(side if name == "side" else volume.adopt_torch_stream()):
            a = filler
            for _ in range(8):
                a = a @ filler * 0.0 + 1.0
            yield
    torch.cuda.synchronize()


def strided(image, device):
    """The image as a non-contiguous CUDA tensor that a torch operation has just produced: a column slice of a wider tensor for one
    channel, [..., :3] of a four-channel tensor for three."""
    import torch

    if image.ndim == 2:
        wide = np.full((image.shape[0], image.shape[1] + 7), 0xA5, np.uint8)
        wide[:, 3:3 + image.shape[1]] = image
        view = (torch.from_numpy(wide).to(device) + 0)[:, 3:3 + image.shape[1]]
    else:
        wide = np.concatenate([image, np.full(image.shape[:2] + (1,), 0xA5, np.uint8)], axis=2)
        view = (torch.from_numpy(wide).to(device) + 0)[..., :3]
    assert not view.is_contiguous() and view.dtype == torch.uint8
    return view


@pytest.mark.parametrize("case", DEVICE_CASES)
@pytest.mark.parametrize("name", SETTINGS)
def test_device_form_on_strided_tensors_and_streams(vol, adopted, side, filler, name, case):
    import torch

    left, right, params = sc.planted(case)
    volume = adopted if name == "adopted" else vol
    host = volume.stereo_sgm(left, right, **params)
    _same(host, restated(case, params["paths"]))
    dev = torch.device("cuda", 0)
    with setting(name, volume, side, filler):
        got = volume.stereo_sgm(strided(left, dev), strided(right, dev), **params)
        got = tuple(t.clone() for t in got)
    assert all(t.is_cuda for t in got) and got[0].dtype == torch.int16 and got[1].dtype == torch.float32
    _same(tuple(t.cpu().numpy() for t in got), host)


def test_each_output_alone_through_the_raw_call(vol):
    """disparity_out = NULL and depth_out = NULL are both legal: the other output is written as if both were asked for, the
    buffer that was not passed is not touched."""
    left, right, params = sc.planted(FARTHEST)
    want = restated(FARTHEST, params["paths"])
    assert int(want[0].max()) >= 16 * 250  # the far end of the range is there
    H, W = left.shape
    prm = L.HvStereoParams(*(int(params[k]) for k in ("num_disparities", "p1", "p2", "uniqueness_ratio", "max_diff", "paths")),
                           float(params["bf"]), float(params["min_depth"]), float(params["max_depth"]))
    disp = np.full((H, W), 0x5A5A, np.int16)
    depth = np.full((H, W), -77.0, np.float32)

    def call(d, z):
        return vol._lib.hv_stereo_sgm(vol._h, L.ptr(left), L.ptr(right), H, W, 1, ctypes.byref(prm), L.ptr(d), L.ptr(z), L.HV_HOST)

    assert call(disp, None) == 0
    np.testing.assert_array_equal(disp, want[0])
    assert (depth == -77.0).all()
    disp[:] = 0x5A5A
    assert call(None, depth) == 0
    np.testing.assert_array_equal(depth.view(np.uint32), want[1].view(np.uint32))
    assert (disp == 0x5A5A).all()
