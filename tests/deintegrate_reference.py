"""numpy restatement of TSDF de-integration (include/hipvol.h, hv_tsdf_deintegrate): from an hv_tsdf_dump taken before the call
and every frame's exact samples, the dump after it and the call's stats.

A frame's samples come from the oracle: a fresh PortTsdf integrates the frame once, so every unit it holds afterwards is in the
frame's touch set, a voxel with weight 1 holds exactly the frame's tsdf sample t (0 * 0 + t, divided by 1) and its colour is
exactly the frame's colour bytes."""
import numpy as np

MAX_FRAMES = 64


class FrameSamples:
    """One frame's touch set and per-voxel samples: keys [k,3] i32, t [k,R^3] f32, sampled [k,R^3] bool, colour [k,R^3,3] i64
    (voxel order of hv_tsdf_dump)."""

    def __init__(self, keys, t, sampled, colour):
        self.keys, self.t, self.sampled, self.colour = keys, t, sampled, colour


def frame_samples(voxel, trunc, depth, rgb, K, T, depth_scale=1.0, depth_trunc=4.0, stride=4):
    import oracle

    cpu = oracle.PortTsdf(voxel, trunc, depth_sampling_stride=stride)
    cpu.integrate(depth, rgb, K, T, depth_scale, depth_trunc)
    keys, t, w, c = cpu.dump()
    assert len(keys) == cpu.num_touched()
    sampled = w == 1.0
    assert np.all((w == 0.0) | sampled)
    return FrameSamples(keys, t, sampled, np.rint(c).astype(np.int64))


def deintegrate_reference(dump, samples, max_frames=MAX_FRAMES):
    """dump = (keys, tsdf, weight, colour) of hv_tsdf_dump before the call; samples = [FrameSamples] in call order.
    -> (dump after the call, (units_listed, units_missing, voxels_removed, voxels_underflow))."""
    keys, tsdf, weight, colour = dump
    tsdf = np.array(tsdf, np.float32, copy=True)
    w = np.asarray(weight).astype(np.int64)
    sums = np.rint(np.asarray(colour, np.float64) * np.asarray(weight, np.float64)[..., None]).astype(np.int64)
    index = {tuple(int(x) for x in k): i for i, k in enumerate(keys)}
    listed = missing = removed = underflow = 0
    for c0 in range(0, len(samples), max_frames):
        n = np.zeros(w.shape, np.int64)
        s = np.zeros(w.shape, np.float64)
        csum = np.zeros(sums.shape, np.int64)
        for fs in samples[c0:c0 + max_frames]:
            listed += len(fs.keys)
            for j, k in enumerate(fs.keys):
                i = index.get(tuple(int(x) for x in k))
                if i is None:
                    missing += 1
                    continue
                m = fs.sampled[j]
                n[i] += m
                s[i] = np.where(m, s[i] + fs.t[j].astype(np.float64), s[i])  # frame order, one double rounding per frame
                csum[i] += fs.colour[j] * m[:, None]
        upd = n > 0
        under = upd & (w < n)
        fresh = upd & (w == n)
        rest = upd & (w > n)
        underflow += int(under.sum())
        removed += int(n[fresh | rest].sum())
        tsdf[fresh] = 0.0
        w[fresh] = 0
        sums[fresh] = 0
        tsdf[rest] = ((tsdf[rest].astype(np.float64) * w[rest].astype(np.float64) - s[rest]) /
                      (w[rest] - n[rest]).astype(np.float64)).astype(np.float32)
        w[rest] -= n[rest]
        # each sum stays in [0, 255 w]: acts only when a frame that was never fused into the voxel is removed from it
        sums[rest] = np.minimum(np.maximum(sums[rest] - csum[rest], 0), 255 * w[rest][:, None])
    wf = w.astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        col = np.where(wf[..., None] > 0, sums / wf[..., None], 0.0)
    return (np.asarray(keys), tsdf, w.astype(np.float32), col), (listed, missing, removed, underflow)
