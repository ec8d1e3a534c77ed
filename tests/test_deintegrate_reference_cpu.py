"""CPU: the numpy restatement of TSDF de-integration (tests/deintegrate_reference.py) on hand-built volumes - the zero-weight
reset, underflow, the clamp of the colour sums, chunking at 64 frames and the tsdf error a removal leaves."""
import numpy as np

from tests.deintegrate_reference import MAX_FRAMES, FrameSamples, deintegrate_reference

R3 = 16 ** 3


def one_unit(tsdf, weight, colour):
    """A one-unit dump whose voxel 0 holds (tsdf, weight, mean colour); every other voxel is fresh."""
    keys = np.array([[1, -2, 3]], np.int32)
    t = np.zeros((1, R3), np.float32)
    w = np.zeros((1, R3), np.float32)
    c = np.zeros((1, R3, 3), np.float64)
    t[0, 0], w[0, 0], c[0, 0] = tsdf, weight, colour
    return keys, t, w, c


def sample(t, colour, key=(1, -2, 3), sampled=True):
    ts = np.zeros((1, R3), np.float32)
    sm = np.zeros((1, R3), bool)
    cs = np.zeros((1, R3, 3), np.int64)
    ts[0, 0], sm[0, 0], cs[0, 0] = t, sampled, colour
    return FrameSamples(np.array([key], np.int32), ts, sm, cs)


def running_mean(ts):
    """The fuse kernels' running mean in float32 over the samples ts."""
    tsdf, w = np.float32(0.0), 0
    for t in ts:
        tsdf = np.float32((tsdf * np.float32(w) + np.float32(t)) / np.float32(w + 1))
        w += 1
    return tsdf, w


def test_removing_every_observation_gives_the_fresh_voxel():
    ts = [0.25, -0.5, 0.75]
    mean, w = running_mean(ts)
    dump = one_unit(mean, w, (10.0, 20.0, 30.0))
    (keys, t, wt, c), stats = deintegrate_reference(dump, [sample(x, (10, 20, 30)) for x in ts])
    assert t[0, 0] == 0.0 and wt[0, 0] == 0.0 and np.all(c[0, 0] == 0.0)
    assert stats == (3, 0, 3, 0)
    # the rest of the unit is untouched
    assert np.all(t[0, 1:] == 0.0) and np.all(wt[0, 1:] == 0.0)


def test_partial_removal_is_exact_on_weights_and_colour_sums():
    dump = one_unit(np.float32(0.5), 4, (100.0, 50.0, 25.0))  # sums 400, 200, 100
    (_, t, w, c), stats = deintegrate_reference(dump, [sample(0.25, (40, 20, 10)), sample(-0.25, (60, 30, 15))])
    assert w[0, 0] == 2.0
    np.testing.assert_array_equal(c[0, 0], [150.0, 75.0, 37.5])  # (400 - 100) / 2, (200 - 50) / 2, (100 - 25) / 2
    assert t[0, 0] == np.float32((0.5 * 4.0 - (0.25 + -0.25)) / 2.0)
    assert stats == (2, 0, 2, 0)


def test_colour_sums_are_clamped_when_a_frame_that_was_never_fused_is_removed():
    # sums 30, 1500, 400 at weight 6; a foreign frame of colour (200, 0, 100) leaves weight 5 and
    #   r: 30 - 200 < 0 -> 0 (the low end);  g: 1500 - 0 > 255 * 5 -> 1275 (the high end);  b: 400 - 100 = 300, inside
    dump = one_unit(np.float32(0.5), 6, (5.0, 250.0, 400.0 / 6.0))
    (_, t, w, c), stats = deintegrate_reference(dump, [sample(0.25, (200, 0, 100))])
    assert w[0, 0] == 5.0 and stats == (1, 0, 1, 0)
    np.testing.assert_array_equal(c[0, 0], [0.0, 255.0, 60.0])
    assert t[0, 0] == np.float32((0.5 * 6.0 - 0.25) / 5.0)  # the tsdf rule is untouched by the clamp
    # a removal of frames that WERE fused never reaches the clamp: the extreme bytes on both sides
    dump = one_unit(np.float32(0.0), 3, (170.0, 85.0, 255.0))  # sums 510 = 255 + 255 + 0, 255 = 0 + 0 + 255, 765
    (_, _, w, c), _ = deintegrate_reference(dump, [sample(0.0, (0, 255, 255))])
    assert w[0, 0] == 2.0
    np.testing.assert_array_equal(c[0, 0], [255.0, 0.0, 255.0])


def test_underflow_leaves_the_voxel_unchanged_and_counts_it_once():
    dump = one_unit(np.float32(0.125), 1, (7.0, 8.0, 9.0))
    after, stats = deintegrate_reference(dump, [sample(0.125, (7, 8, 9)), sample(0.5, (1, 2, 3))])
    for a, b in zip(after[1:], dump[1:]):
        np.testing.assert_array_equal(a, b)
    assert stats == (2, 0, 0, 1)


def test_unsampled_voxels_and_missing_units():
    dump = one_unit(np.float32(0.5), 2, (1.0, 1.0, 1.0))
    frames = [sample(0.9, (5, 5, 5), sampled=False), sample(0.3, (5, 5, 5), key=(9, 9, 9))]
    after, stats = deintegrate_reference(dump, frames)
    for a, b in zip(after[1:], dump[1:]):
        np.testing.assert_array_equal(a, b)
    assert stats == (2, 1, 0, 0)


def test_frames_act_in_chunks_of_64():
    # 65 frames sample a voxel that holds 64 observations: the first chunk empties it, the 65th frame then underflows
    # (one call over all 65 at once would underflow the voxel and leave it as it was)
    ts = [((k % 7) - 3) / 4.0 for k in range(MAX_FRAMES)]
    mean, w = running_mean(ts)
    dump = one_unit(mean, w, (3.0, 2.0, 1.0))
    frames = [sample(x, (3, 2, 1)) for x in ts] + [sample(0.5, (3, 2, 1))]
    (_, t, wt, c), stats = deintegrate_reference(dump, frames)
    assert wt[0, 0] == 0.0 and t[0, 0] == 0.0
    assert stats == (65, 0, 64, 1)
    (_, t1, w1, _), stats1 = deintegrate_reference(dump, frames, max_frames=65)
    assert w1[0, 0] == 64.0 and t1[0, 0] == mean and stats1 == (65, 0, 0, 1)


def test_tsdf_error_after_removal_stays_within_the_bound():
    # 64 observations fused by the float32 running mean, 63 of them removed: the stored mean's rounding is scaled by ~w0 / w
    rng = np.random.default_rng(7)
    worst = 0.0
    for _ in range(200):
        ts = rng.uniform(-1.0, 1.0, MAX_FRAMES).astype(np.float32)
        mean, w = running_mean(ts)
        dump = one_unit(mean, w, (0.0, 0.0, 0.0))
        (_, t, wt, _), _ = deintegrate_reference(dump, [sample(x, (0, 0, 0)) for x in ts[1:]])
        assert wt[0, 0] == 1.0
        worst = max(worst, abs(float(t[0, 0]) - float(ts[0])))
    # each stored mean carries up to ~half an ulp of |mean| <= 1 per update (a few times 6e-8 after 64 of them); the removal
    # multiplies by w0 / w = 64
    print(f"max |tsdf - t| after removing 63 of 64: {worst:.3g}")
    assert worst <= 64 * 64 * 6e-8
    assert worst <= 1e-4
