"""GPU: the epilogue of the multi-frame sweep - the read-modify-write of a column's plane words in passes of voxels
(hv_sweep_epilogue in pyslam_amd/csrc/hv_tsdf.hip) - against oracle.PortTsdf on tiny_160x120_2cm (2 cm voxels, sdf_trunc 0.08, a
few dozen units).

Bars (tests/conftest.py): unit keys, weights and colour sums exact; tsdf within FOLD_TSDF_TOL on the fold form, bitwise under
HV_TSDF_SWEEP=2.  Forms: whole columns (HV_TSDF_SWEEP_ZS=1, four passes per column), z halves (ZS=2, two passes), the general
regime (HV_TSDF_BATCH_GENERAL=1) and the bitwise form.  Batches of 1, 5 and 64 frames; a second batch into the same volume, so
that the epilogue adds to non-zero weights and colour sums; and a second batch whose depth is zero over the left half of every
image: the voxels it does not update must keep every word bit for bit (the skipped lanes and skipped z planes of a pass), in
columns that are updated on both sides of a pass boundary (z = 3 / 4).
"""
import functools

import numpy as np
import pytest

import oracle
from tests.conftest import assert_tsdf_parity
from tests.test_gpu_tsdf_edges import cuda, intrinsic, oracle_of, stack, tiny_frames, volume

pytestmark = pytest.mark.gpu

VOXEL, TRUNC = 0.02, 0.08
FORMS = {  # environment of a call (read per integrate_batch call)
    "columns": {"HV_TSDF_SWEEP": "4", "HV_TSDF_SWEEP_ZS": "1"},
    "z_halves": {"HV_TSDF_SWEEP": "4", "HV_TSDF_SWEEP_ZS": "2"},
    "general": {"HV_TSDF_SWEEP": "4", "HV_TSDF_BATCH_GENERAL": "1"},
    "bitwise": {"HV_TSDF_SWEEP": "2"},
}


@pytest.fixture(params=list(FORMS))
def form(request, monkeypatch):
    for k, v in FORMS[request.param].items():
        monkeypatch.setenv(k, v)
    return request.param


def half_invalid(frames):
    """The frames with depth zero (= invalid) over the left half of every image."""
    out = []
    for d, c, T in frames:
        d = d.copy()
        d[:, : d.shape[1] // 2] = 0
        out.append((d, c, T))
    return out


@functools.lru_cache(maxsize=None)
def frame_set(name):
    """-> (stream, list of batches); every batch a list of (depth, colour, T_cw)."""
    if name.startswith("one_batch_"):
        s, fr = tiny_frames(0, int(name.rsplit("_", 1)[1]))
        return s, [fr]
    if name == "two_batches":
        s, fr = tiny_frames(0, 10)
        return s, [fr[:5], fr[5:]]
    assert name == "second_half_invalid"
    s, fr = tiny_frames(0, 69)
    return s, [fr[:5], half_invalid(fr[5:])]


@functools.lru_cache(maxsize=None)
def oracle_dump(name):
    """The oracle's volume after every frame of the set, computed once and shared (read-only) by the forms."""
    s, batches = frame_set(name)
    cpu = oracle.PortTsdf(VOXEL, TRUNC, threads=8)
    for b in batches:
        oracle_of(s, b, VOXEL, TRUNC, cpu=cpu)
    assert cpu.num_units() > 0
    dump = cpu.dump()
    for a in dump:
        a.setflags(write=False)
    return dump


def assert_matches_oracle(gpu, name):
    """Keys, weights and colour SUMS exact, tsdf per assert_tsdf_parity.  The planes hold integer colour sums; the oracle keeps the
    colour as a running mean in double precision, whose product with the weight is within 1e-10 of the integer sum it stands for."""
    kb, tb, wb, cb = oracle_dump(name)
    ka, ta, wa, _ = gpu.dump()
    np.testing.assert_array_equal(ka, kb)
    np.testing.assert_array_equal(wa, wb)
    assert_tsdf_parity(ta, tb, swept=True)
    sums = cb * wb[..., None]
    assert np.abs(sums - np.rint(sums)).max() < 1e-6
    np.testing.assert_array_equal(numerators(gpu, ka)[..., 2:5].reshape(sums.shape), np.rint(sums).astype(np.float32))


def numerators(gpu, keys):
    """export_numerators in the order of dump(): [unit, x, y, z, {tsdf w, w, sum r, sum g, sum b}].  (The payload is in the
    planes' word order, z * 256 + x * 16 + y.)"""
    return np.ascontiguousarray(gpu.export_numerators(keys).reshape(len(keys), 16, 16, 16, 5).transpose(0, 2, 3, 1, 4))


def integrate(gpu, s, batch):
    d, c, T = stack(batch)
    gpu.integrate_batch(*cuda(d, c), intrinsic(s), T, depth_scale=1.0, depth_trunc=4.0)


@pytest.mark.parametrize("F", [1, 5, 64])
def test_one_batch_matches_the_oracle(F, form):
    s, (batch,) = frame_set(f"one_batch_{F}")
    gpu = volume(VOXEL, TRUNC)
    integrate(gpu, s, batch)
    assert_matches_oracle(gpu, f"one_batch_{F}")


def test_second_batch_adds_to_nonzero_weights_and_colour_sums(form):
    s, (first, second) = frame_set("two_batches")
    gpu = volume(VOXEL, TRUNC)
    integrate(gpu, s, first)
    keys = gpu.dump()[0]
    w0 = numerators(gpu, keys)[..., 1]
    integrate(gpu, s, second)
    w1 = numerators(gpu, keys)[..., 1]
    assert ((w0 > 0) & (w1 > w0)).any()  # the second epilogue did add to words the first one wrote
    assert_matches_oracle(gpu, "two_batches")


def test_voxels_a_batch_does_not_update_keep_every_word(form):
    s, (first, second) = frame_set("second_half_invalid")
    gpu = volume(VOXEL, TRUNC)
    integrate(gpu, s, first)
    keys = gpu.dump()[0]
    before = numerators(gpu, keys)  # [unit, x, y, z, {tsdf w, w, r, g, b}]
    integrate(gpu, s, second)
    after = numerators(gpu, keys)
    assert_matches_oracle(gpu, "second_half_invalid")
    changed = after[..., 1] != before[..., 1]
    assert changed.any() and (~changed).any()  # both kinds of voxel occur
    assert (~changed & (before[..., 1] > 0)).any()  # ... and some of the untouched ones held data
    np.testing.assert_array_equal(after.view(np.uint32)[~changed], before.view(np.uint32)[~changed])
    # columns (unit, x, y) updated on both sides of the pass boundary z = 3 / 4 that also hold a z the batch left alone: the
    # skipped lanes of a pass next to its updated ones
    straddle = changed[..., 3] & changed[..., 4] & ~changed.all(axis=-1)
    assert straddle.any()
    np.testing.assert_array_equal(after.view(np.uint32)[straddle][~changed[straddle]],
                                  before.view(np.uint32)[straddle][~changed[straddle]])
    # ... and whole z planes of a column group (x in [4 g, 4 g + 4), every y) that no lane updates, beside planes some lane does
    planes = changed.reshape(len(keys), 4, 4, 16, 16).any(axis=(2, 3))  # [unit, column group, z]
    assert (planes.any(axis=-1) & ~planes.all(axis=-1)).any()
