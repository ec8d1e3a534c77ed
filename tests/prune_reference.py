"""numpy restatement of TSDF pruning (include/hipvol.h, hv_tsdf_prune): from an hv_tsdf_dump taken before the call, the dump after
it and the call's stats.

A unit is released when its index lies outside the inclusive range [unit_lo, unit_hi] on some axis (counted as outside), else, with
`empty`, when all its weights are 0 (counted as empty).  The rows that stay are untouched and keep their (sorted) order."""
import numpy as np


def prune_reference(dump, empty=True, unit_lo=None, unit_hi=None):
    """dump = (keys, tsdf, weight, colour) of hv_tsdf_dump; unit_lo / unit_hi = [3] unit indices or None (both or neither).
    -> (dump after the call, (units_before, units_outside, units_empty, units_after))."""
    keys, tsdf, weight, colour = (np.asarray(x) for x in dump)
    assert (unit_lo is None) == (unit_hi is None)
    n = len(keys)
    outside = np.zeros(n, bool)
    if unit_lo is not None:
        lo, hi = np.asarray(unit_lo, np.int64).reshape(3), np.asarray(unit_hi, np.int64).reshape(3)
        k = keys.reshape(n, 3).astype(np.int64)
        outside = np.any((k < lo) | (k > hi), axis=1)
    hollow = np.zeros(n, bool)
    if empty:
        hollow = ~outside & np.all(weight == 0, axis=tuple(range(1, weight.ndim)))
    keep = ~(outside | hollow)
    stats = (n, int(outside.sum()), int(hollow.sum()), int(keep.sum()))
    return (keys[keep], tsdf[keep], weight[keep], colour[keep]), stats
