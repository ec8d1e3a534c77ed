"""The multi-GPU exchange on its own, on one GPU: the library calls behind ShardedTSDF.merge / merge_halo (hv_halo.hip) on a volume of
1 024 planted units, every one of them dirty.  A one-GPU bench.py run has no exchange leg; this is the yardstick for changes to that
file.  Each figure is the median wall time of REPS calls after WARM warm-up calls, the clock stopped after the volume's stream has
been waited for.  Reported, not asserted.  Uses nothing but long-standing methods of ScalableTSDFVolume, so the same file times an
older checkout.

Prints one JSON line, times in microseconds:
  export_us        export_numerators of all units into a device payload (80 MiB)
  halo_unpack_us   halo_unpack of that payload, every unit kept
  import_us        import_numerators of it into an EMPTY volume (claim + write; the reset is outside the clock)
  lists_us         halo_lists_device (dirty and held lists as packed keys, two integers back)
  plan_us          halo_plan_device on the gathered lists of 8 ranks, `plan_entries` entries, `plan_shared` shared keys
  dirty_keys_us    dirty_keys() (sorted host array)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from pyslam_amd.volumetric import ScalableTSDFVolume  # noqa: E402

UNITS, REPS, WARM, WORLD = 1024, 200, 10, 8
BIAS = 1 << 20


def planted(rng):
    """1 024 unit keys around the origin and their numerators: weights 0 .. 7 (a third of the voxels unobserved), tsdf in (-1, 1),
    colour sums up to 255 w - integers float32 holds exactly."""
    keys = np.array([(x, y, z) for x in range(-8, 8) for y in range(-4, 4) for z in range(-4, 4)], np.int32)
    w = rng.integers(0, 8, (UNITS, 4096)).astype(np.float32) * (rng.random((UNITS, 4096)) > 0.33)
    payload = np.empty((UNITS, 4096, 5), np.float32)
    payload[..., 0] = rng.uniform(-1, 1, w.shape).astype(np.float32) * w
    payload[..., 1] = w
    payload[..., 2:] = rng.integers(0, 256, w.shape + (3,)).astype(np.float32) * w[..., None]
    return keys, payload


def gathered_lists(keys, rng):
    """World-8 lists over the planted keys as halo_plan_device takes them: a rank holds 30 % of the keys and lists 7 % dirty."""
    packed = ((keys[:, 0] + BIAS).astype(np.int64) | (keys[:, 1] + BIAS).astype(np.int64) << 21 | (keys[:, 2] + BIAS).astype(np.int64) << 42)
    out = []
    for share in (0.07, 0.30):
        lists = [packed[rng.random(UNITS) < share] for _ in range(WORLD)]
        counts = np.array([len(x) for x in lists], np.int64)
        padded = np.zeros((WORLD, int(counts.max())), np.int64)
        for r, x in enumerate(lists):
            padded[r, :len(x)] = x
        out += [torch.from_numpy(padded).cuda(), counts]
    return out


def main():
    assert torch.cuda.is_available(), "bench_exchange needs a GPU"
    rng = np.random.default_rng(5)
    keys, payload_host = planted(rng)
    new_volume = lambda: ScalableTSDFVolume(0.01, 0.04, max_blocks=2 * UNITS)
    src, vol, dst = new_volume(), new_volume(), new_volume()
    src.import_numerators(keys, payload_host)
    vol.unpack(src.pack(device=True))  # (an unpacked unit is dirty, an imported one is not)
    payload = torch.empty((UNITS, 4096, 5), dtype=torch.float32, device="cuda")
    dirty, held = (torch.empty(UNITS, dtype=torch.int64, device="cuda") for _ in range(2))
    dirty_all, dirty_counts, held_all, held_counts = gathered_lists(keys, rng)
    keep = np.ones(UNITS, np.uint8)
    torch.cuda.synchronize()
    assert vol.num_blocks() == UNITS and len(vol.dirty_keys()) == UNITS

    def median_us(volume, fn, prepare=None):
        times = []
        for i in range(WARM + REPS):
            if prepare:
                prepare()
            volume.synchronize()
            t0 = time.perf_counter()
            fn()
            volume.synchronize()
            if i >= WARM:
                times.append((time.perf_counter() - t0) * 1e6)
        return round(float(np.median(times)), 1)

    out = {"tool": "bench_exchange", "units": UNITS, "reps": REPS, "plan_entries": int(dirty_counts.sum() + held_counts.sum())}
    out["export_us"] = median_us(vol, lambda: vol.export_numerators(keys, out=payload))
    out["halo_unpack_us"] = median_us(vol, lambda: vol.halo_unpack(keys, payload, keep))
    out["import_us"] = median_us(dst, lambda: dst.import_numerators(keys, payload), prepare=dst.reset)
    out["lists_us"] = median_us(vol, lambda: vol.halo_lists_device(dirty, held))
    plan = lambda: vol.halo_plan_device(dirty_all, dirty_counts, held_all, held_counts, WORLD, 3)
    out["plan_us"] = median_us(vol, plan)
    out["plan_shared"] = int(plan())
    out["dirty_keys_us"] = median_us(vol, vol.dirty_keys)
    assert dst.num_blocks() == UNITS and vol.halo_lists_device(dirty, held) == (UNITS, UNITS)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
