"""Scripts over one long-lived TSDF map: fixed lists of mixed operations, each followed by a TICK that says which readers run after
it - test infrastructure, no GPU.  tests/test_lifetime_reference_cpu.py runs them through the numpy / oracle restatements alone and
holds the conditions that keep the GPU tests from passing vacuously; tests/test_gpu_lifetime.py runs them on a ScalableTSDFVolume
and holds every step, and the state the volume carries from one call into the next, to the same restatements.

Voxel 0.02, sdf_trunc 0.08, the (keys, tsdf, weight, colour) dump format of tests/planted_states.py throughout.

A STEP is Step(op, arg, tick, nothing):
    fuse                online integrate, one call per frame          arg = Frames
    fuse_batch          integrate_batch                               arg = Frames
    deintegrate_batch                                                 arg = Frames
    reintegrate_batch   from the frames' poses to poses moved by MOVE arg = Frames
    prune               arg = (empty, unit_lo, unit_hi)  (unit indices, inclusive, or None)
    merge               integrate_volume                              arg = (name in SOURCES, name in TRANSFORMS)
    remove_small        remove_small_components                       arg = (min_sites, margin)
    repack              pack, reset, unpack into the same volume
    mark_merged
    read_mesh, ray_cast, sample_points     readers as steps of their own (the "other operation" of the pipeline scripts)
tick: a tuple out of "mesh", "points", "normals" (points with normals), "mesh32"; () puts two operations between two extractions.
nothing: the step must leave the dump bit-identical (a reader, a removal below every component's size, a merge of a hollow source,
a prune with nothing to release).  repack and mark_merged leave it identical by definition and are not marked.

Frames come from tests/test_gpu_tsdf_edges.py's tiny_160x120_2cm stream with the depth masked to a pixel window, so that no state
exceeds the size guide of about 150 units.  Units held, measured with the restatements (start / maximum over the script):
    slots_move 32 / 85    pool_grows 0 / 132    pipeline_readers 0 / 54    pipeline_no_ops 1 / 47    pipeline_writers 0 / 62
    gather_a 27 / 49      gather_b 33 / 49      chain_a 27 / 72           chain_b 27 / 67
    chain_c 34 / 101      chain_d 34 / 110      chain_e 33 / 55           chain_f 33 / 70
pool_grows crosses its pool of 64 blocks with all three per-unit caches warm; growing past the 1024-unit cache layout
(unit_caches_ensure) conflicts with the size guide and is left to test_incremental_extraction_equals_a_full_pass_at_every_tick.

The issue's gather script, mark_merged behind every writer, would have sixteen steps; it is split into gather_a (the frame writers) and
gather_b (merge, removal, both prune forms, repack).  Its pipeline script is split by the kind of operation between the batches.

Pair coverage (pair_coverage(), asserted in tests/test_lifetime_reference_cpu.py) is counted over the nine writer OPS - fuse, fuse_batch,
deintegrate_batch, reintegrate_batch, prune by emptiness, prune by bounds, merge, remove_small, repack - whose carried state differs:
72 ordered pairs, each present with an empty tick between the two.  The named scripts cannot hold them in 8-14 steps each; chain_a to
chain_f carry the rest.
"""
import collections
import functools

import numpy as np

from tests import components_cases as cc
from tests import planted_states as ps
from tests import sample_cases as sc

VOX, TRUNC = ps.VOX, ps.TRUNC
Step = collections.namedtuple("Step", "op arg tick nothing", defaults=((), False))
Frames = collections.namedtuple("Frames", "camera first count window", defaults=("small",))
Script = collections.namedtuple("Script", "name max_blocks start steps")

WINDOWS = {"small": (56, 104, 40, 80), "wide": (40, 120, 30, 90)}  # u0, u1, v0, v1: depth outside is set to 0 (no sample)
OTHER_CAMERA = dict(width=160, height=120, fx=140.0, fy=127.3125, cx=70.25, cy=73.2, voxel=0.02)  # same shape, other intrinsics
MOVE = ps.with_translation(ps.IDENTITY, metres=(0.013, -0.007, 0.021))  # reintegrate_batch: T_new = T_old @ MOVE
WRITER_STEPS = ("fuse", "fuse_batch", "deintegrate_batch", "reintegrate_batch", "prune", "merge", "remove_small", "repack")
READER_STEPS = ("read_mesh", "ray_cast", "sample_points")
MESH_TICKS, POINT_TICKS = ("mesh", "mesh32"), ("points", "normals")
EVERYTHING = (False, (-1000, -1000, -1000), (1000, 1000, 1000))  # a prune that releases nothing


# ---- frames --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def frames_for(spec):
    """-> (camera, [(depth, colour, T_cw)]) of a Frames spec, the depth masked to the spec's window.  Shared: never written to."""
    from tests.test_gpu_tsdf_edges import frames_of, tiny_frames

    s, frames = tiny_frames(spec.first, spec.count) if spec.camera == "tiny" else frames_of(OTHER_CAMERA, spec.first, spec.count)
    u0, u1, v0, v1 = WINDOWS[spec.window]
    out = []
    for d, c, T in frames:
        masked = np.zeros_like(d)
        masked[v0:v1, u0:u1] = d[v0:v1, u0:u1]
        out.append((masked, c, T))
    return s, out


@functools.lru_cache(maxsize=None)
def samples_for(spec, moved=False):
    """The FrameSamples of tests/deintegrate_reference.py for the frames of `spec` (moved: at T_cw @ MOVE)."""
    from tests.deintegrate_reference import frame_samples
    from tests.test_gpu_tsdf_edges import intrinsic

    s, frames = frames_for(spec)
    K = intrinsic(s).as_array()
    return [frame_samples(VOX, TRUNC, d, c, K, T @ MOVE if moved else T, 1.0, 4.0, 4) for d, c, T in frames]


def tiny(first, count, window="small"):
    return Frames("tiny", first, count, window)


# ---- planted starts and merge sources --------------------------------------------------------------------------------------------
SHIFT = np.array([4, 1, 3], np.int32)   # carries planted_states' cluster (units -2..0) to where the tiny camera looks
HOLES = ((3, 0, 2), (4, 0, 2), (3, -2, 2), (3, 2, 4), (4, -2, 3))  # all-zero units, in the middle of the (x, y, z) order
FLOATER_UNIT = (9, 0, 1)


def shifted(states, by):
    return (np.asarray(states[0], np.int32) + np.asarray(by, np.int32),) + tuple(states[1:])


@functools.lru_cache(maxsize=None)
def cluster():
    """planted_states' sphere-and-plane cluster (special values, weights 0..7) in front of the camera."""
    return shifted(ps.sparse_source(), SHIFT)


@functools.lru_cache(maxsize=None)
def floater():
    """components_cases' small sphere (radius 3 voxels, one component inside one unit) in a unit apart from everything."""
    ball = cc._band(lambda p: np.linalg.norm(p - np.array(cc.SMALL_CENTRE) * VOX, axis=-1) - cc.SMALL_RADIUS * VOX, [(2, 0, 0)])
    return shifted(ball, np.array(FLOATER_UNIT) - np.array([2, 0, 0]))


@functools.lru_cache(maxsize=None)
def holes():
    return ps.empty_units(np.array(HOLES, np.int64))


LINE_X, FAR_LO = 12, (-50, -50, -50)


def line(count):
    """`count` units at (LINE_X + i, 0, 1), beyond everything the camera sees, one observed voxel each (no site, not empty): a prune
    by bounds with hi x = LINE_X + i - 1 releases those from i on, whatever else the map holds."""
    return sc.concat(*(ps.single_voxel((LINE_X + i, 0, 1), (8, 8, 8), tsdf=0.25, weight=5) for i in range(count)))


def _rigid(axis, degrees, t):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    th = np.radians(degrees)
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * Kx + (1.0 - np.cos(th)) * (Kx @ Kx)
    T[:3, 3] = t
    return T


# p_map = T p_source.  "into view": the source (units -1..0 around the origin) lands on and beside the units the camera fills.
TRANSFORMS = {"identity": np.eye(4), "into view": _rigid((0.3, 1.0, 0.2), 23.0, (1.37, 0.41, 0.93)),
              "beside": _rigid((1.0, -0.4, 0.5), -17.0, (1.13, -0.29, 1.22)), "shift": ps.with_translation(ps.IDENTITY, (67, 5, 52))}


@functools.lru_cache(maxsize=None)
def source(name):
    """Merge sources, planted states: "blob" a sphere-and-plane piece over six units, "other blob" the same with another seed,
    "hollow" units that hold no observed voxel (a merge of it updates nothing)."""
    keys = np.array([(-1, -1, -1), (-1, 0, -1), (0, -1, -1), (0, 0, -1), (-1, -1, 0), (0, 0, 0)], np.int64)
    if name == "blob":
        return ps.sphere_and_plane(keys, seed=3, special=False)
    if name == "other blob":
        return ps.sphere_and_plane(keys[1:], seed=4, special=True)
    assert name == "hollow"
    return ps.empty_units(keys[:3])


SOURCES = ("blob", "other blob", "hollow")


def concat(parts):
    return sc.concat(*parts) if parts else empty_dump()


def empty_dump():
    return (np.zeros((0, 3), np.int32), np.zeros((0, ps.NV), np.float32), np.zeros((0, ps.NV), np.float32), np.zeros((0, ps.NV, 3)))


def start_dump(script):
    """The dump of a volume the script's start states were planted into."""
    return ps.as_dump(concat([part() for part in script.start])) if script.start else empty_dump()


# ---- the scripts -----------------------------------------------------------------------------------------------------------------
WARM = ("mesh", "points")
ALL = ("mesh", "normals", "mesh32")
BIG_BLOCKS = 1 << 12


def _pipeline(name, start, others, odd_batch=None):
    """fuse_batch, fuse_batch (chained), one other operation, fuse_batch - once per entry of `others`, the last batch of one
    round being the first of the next.  Every batch is two consecutive frames; odd_batch: the index of the batch taken with
    OTHER_CAMERA (the sweep's multiplier table is rebuilt in the middle of the chain)."""
    steps, at = [], [0]

    def batch(tick=()):
        n = len([s for s in steps if s.op == "fuse_batch"])
        spec = Frames("other" if n == odd_batch else "tiny", at[0], 2, "small")
        at[0] += 2
        steps.append(Step("fuse_batch", spec, tick))

    batch()
    for k, other in enumerate(others):
        batch()
        steps.append(other)
        batch(WARM if k == 0 else ())
    steps[-1] = steps[-1]._replace(tick=ALL)
    return Script(name, BIG_BLOCKS, start, tuple(steps))


def _scripts():
    out = []
    # slots_move: all-zero units planted FIRST take the low pool slots; releasing them moves the cluster's units into the holes
    batch, later = tiny(0, 2), tiny(20, 1)
    out.append(Script("slots_move", BIG_BLOCKS, (holes, cluster, floater), (
        Step("mark_merged", None, ALL),
        Step("prune", (True, None, None)),
        Step("fuse_batch", batch),
        Step("remove_small", (40, 1)),
        Step("prune", (False, (2, -1, 1), (9, 7, 4))),          # releases the isolated unit (8, 6, 0); the floater, which the first
        Step("deintegrate_batch", batch, WARM),                 # prune moved and nothing writes afterwards, stays
        Step("merge", ("blob", "into view")),
        Step("repack", None),
        Step("fuse", later),
        Step("merge", ("other blob", "beside")),
        Step("deintegrate_batch", later, ALL))))
    # pool_grows: a pool of 64 blocks that is rebuilt under warm caches
    first, wide = tiny(0, 3), tiny(8, 3, "wide")
    out.append(Script("pool_grows", 1 << 6, (), (
        Step("fuse_batch", first, ALL),
        Step("fuse_batch", wide, WARM),                       # crosses 64 units: the pool is rebuilt, every cache warm
        Step("merge", ("blob", "into view")),
        Step("prune", (True, None, None)),
        Step("remove_small", (2100, 1)),                      # the merged piece is the smaller of two components
        Step("repack", None, ("mesh32", "points")),
        Step("deintegrate_batch", first),
        Step("repack", None),
        Step("prune", (False, (2, -1, 1), (6, 4, 3))),
        Step("merge", ("other blob", "beside")),
        Step("remove_small", (30, 4)),
        Step("fuse", tiny(30, 1)),
        Step("deintegrate_batch", tiny(30, 1)),
        Step("fuse_batch", tiny(40, 2, "wide"), ALL))))
    # pipeline: what stands between two integrate_batch calls of a running chain
    out.append(_pipeline("pipeline_readers", (), (Step("read_mesh", None, (), True), Step("ray_cast", tiny(1, 1), (), True),
                                                  Step("sample_points", 500, (), True)), odd_batch=4))
    out.append(_pipeline("pipeline_no_ops", (floater,), (Step("remove_small", (1, 1), (), True), Step("remove_small", (201, 1)),
                                                         Step("merge", ("hollow", "identity"), (), True))))
    out.append(_pipeline("pipeline_writers", (), (Step("deintegrate_batch", tiny(0, 2)), Step("fuse", tiny(30, 1)),
                                                  Step("prune", EVERYTHING, (), True))))
    # gather_a, gather_b: mark_merged between all writers (sixteen steps in one script: split, each writer op in one of the two)
    gb = tiny(4, 2)
    mm = Step("mark_merged", None)
    out.append(Script("gather_a", BIG_BLOCKS, (cluster, floater), (
        Step("fuse", tiny(0, 1)), mm,
        Step("fuse_batch", gb, WARM), mm,
        Step("deintegrate_batch", tiny(0, 1)), mm,
        Step("reintegrate_batch", gb), Step("mark_merged", None, ALL))))
    out.append(Script("gather_b", BIG_BLOCKS, (holes, cluster, floater, functools.partial(line, 1)), (
        Step("merge", ("blob", "into view"), WARM), mm,
        Step("remove_small", (40, 4)), Step("mark_merged", None, ("points",)),
        Step("prune", (True, None, None)), mm,
        Step("prune", (False, FAR_LO, (LINE_X - 1, 50, 50))), mm,
        Step("repack", None), Step("mark_merged", None, ALL))))
    # chain_a, chain_b: the ordered writer pairs the scripts above leave
    out.append(Script("chain_a", BIG_BLOCKS, (cluster, floater), (
        Step("mark_merged", None, WARM),
        Step("remove_small", (40, 1)),
        Step("deintegrate_batch", tiny(10, 1)),
        Step("prune", (True, (2, -1, 1), (8, 7, 4))),
        Step("repack", None),
        Step("merge", ("blob", "into view")),
        Step("fuse_batch", tiny(10, 2)),
        Step("repack", None),
        Step("deintegrate_batch", tiny(10, 2)),
        Step("merge", ("other blob", "beside"), ALL))))
    out.append(Script("chain_b", BIG_BLOCKS, (cluster, floater), (
        Step("mark_merged", None, WARM),
        Step("repack", None),
        Step("remove_small", (40, 1)),
        Step("merge", ("blob", "into view"), WARM),
        Step("fuse", tiny(16, 1)),
        Step("prune", (True, (2, -1, 1), (8, 7, 4)), ("mesh32",)),
        Step("deintegrate_batch", tiny(16, 1)),
        Step("remove_small", (60, 4), ALL))))
    # chain_c .. chain_f: the ordered pairs of writer OPS (fuse and fuse_batch, de- and re-integration, the two prune forms apart)
    # that are left; every prune by bounds releases one unit of the planted line, so that each one moves something
    out.append(Script("chain_c", BIG_BLOCKS, (holes, cluster, floater, functools.partial(line, 2)), (
        Step("mark_merged", None, WARM),
        Step("deintegrate_batch", tiny(0, 1)),
        Step("reintegrate_batch", tiny(2, 1)),
        Step("prune", (True, None, None)),
        Step("reintegrate_batch", tiny(4, 1)),
        Step("prune", (False, FAR_LO, (LINE_X, 50, 50))),
        Step("reintegrate_batch", tiny(6, 1)),
        Step("fuse", tiny(8, 1)),
        Step("prune", (True, None, None)),
        Step("prune", (False, FAR_LO, (LINE_X - 1, 50, 50))),
        Step("fuse", tiny(10, 1)),
        Step("reintegrate_batch", tiny(10, 1)),
        Step("fuse_batch", tiny(12, 2, "wide")),
        Step("prune", (True, None, None), ALL))))
    out.append(Script("chain_d", BIG_BLOCKS, (holes, cluster, floater, functools.partial(line, 2)), (
        Step("mark_merged", None, WARM),
        Step("fuse_batch", tiny(0, 2)),
        Step("reintegrate_batch", tiny(0, 2)),
        Step("deintegrate_batch", tiny(3, 1)),
        Step("prune", (True, None, None)),
        Step("fuse", tiny(5, 1, "wide")),
        Step("prune", (False, FAR_LO, (LINE_X, 50, 50))),
        Step("repack", None),
        Step("prune", (True, None, None)),
        Step("merge", ("blob", "into view")),
        Step("reintegrate_batch", tiny(5, 1)),
        Step("merge", ("other blob", "beside")),
        Step("prune", (False, FAR_LO, (LINE_X - 1, 50, 50))),
        Step("prune", (True, None, None), ALL))))
    out.append(Script("chain_e", BIG_BLOCKS, (holes, cluster, floater, functools.partial(line, 1)), (
        Step("mark_merged", None, WARM),
        Step("deintegrate_batch", tiny(0, 1)),
        Step("fuse", tiny(2, 1)),
        Step("remove_small", (40, 1)),
        Step("reintegrate_batch", tiny(2, 1)),
        Step("repack", None),
        Step("fuse_batch", tiny(4, 2)),
        Step("prune", (False, FAR_LO, (LINE_X - 1, 50, 50))),
        Step("remove_small", (250, 1)),
        Step("prune", (True, None, None)),
        Step("repack", None),
        Step("reintegrate_batch", tiny(4, 2)),
        Step("remove_small", (600, 1), ALL))))
    out.append(Script("chain_f", BIG_BLOCKS, (holes, cluster, floater, functools.partial(line, 1)), (
        Step("mark_merged", None, WARM),
        Step("prune", (True, None, None)),
        Step("deintegrate_batch", tiny(0, 1)),
        Step("prune", (False, FAR_LO, (LINE_X - 1, 50, 50))),
        Step("fuse_batch", tiny(2, 2)),
        Step("merge", ("blob", "into view")),
        Step("fuse", tiny(5, 1)),
        Step("repack", None, ALL))))
    return {s.name: s for s in out}


SCRIPTS = _scripts()
# units held at the start / at most, as the module docstring states them (tests/test_lifetime_reference_cpu.py measures them)
UNITS = {"slots_move": (32, 85), "pool_grows": (0, 132), "pipeline_readers": (0, 54), "pipeline_no_ops": (1, 47), "pipeline_writers": (0, 62),
         "gather_a": (27, 49), "gather_b": (33, 49), "chain_a": (27, 72), "chain_b": (27, 67), "chain_c": (34, 101), "chain_d": (34, 110),
         "chain_e": (33, 55), "chain_f": (33, 70)}
NAMED = ("slots_move", "pool_grows", "gather_a", "gather_b")                      # the issue's scripts of 8-14 steps ...
PIPELINE = ("pipeline_readers", "pipeline_no_ops", "pipeline_writers")  # ... and its pipeline script, split by kind of operation


# ---- coverage, computed from the lists ---------------------------------------------------------------------------------------------
def writer_op(step):
    """The writer a step is, or None: the step's op, with prune split by form ("prune_empty", "prune_bounds"; a prune by both
    criteria in one call is "prune_both" and counts for neither)."""
    if step.op not in WRITER_STEPS or step.nothing:
        return None
    if step.op == "prune":
        empty, lo, _ = step.arg
        return "prune_both" if empty and lo is not None else "prune_empty" if empty else "prune_bounds"
    return step.op


WRITER_OPS = ("fuse", "fuse_batch", "deintegrate_batch", "reintegrate_batch", "prune_empty", "prune_bounds", "merge", "remove_small", "repack")


def pair_coverage(scripts=None):
    """Ordered pairs (writer op, next writer op) that follow each other directly with an empty tick between them."""
    pairs = set()
    for script in (SCRIPTS.values() if scripts is None else scripts):
        for a, b in zip(script.steps[:-1], script.steps[1:]):
            if writer_op(a) and writer_op(b) and a.tick == ():
                pairs.add((writer_op(a), writer_op(b)))
    return pairs


def warm_coverage(scripts=None):
    """writer op -> (a warm mesh extraction precedes some step of it, a warm point extraction does): an extraction earlier in the
    same script, on the same volume."""
    out = {op: [False, False] for op in WRITER_OPS}
    for script in (SCRIPTS.values() if scripts is None else scripts):
        mesh = points = False
        for step in script.steps:
            if writer_op(step) in out:
                out[writer_op(step)][0] |= mesh
                out[writer_op(step)][1] |= points
            mesh |= any(t in MESH_TICKS for t in step.tick) or step.op == "read_mesh"
            points |= any(t in POINT_TICKS for t in step.tick)
    return {k: tuple(v) for k, v in out.items()}


# ---- one step through the restatements ---------------------------------------------------------------------------------------------
def oracle_of(dump):
    import oracle

    return ps.to_oracle(dump) if len(dump[0]) else oracle.PortTsdf(VOX, TRUNC)


def as_held(dump):
    """An oracle dump as a ScalableTSDFVolume holds it: the oracle keeps Open3D's double running mean of the colours, the library
    integer sums, so the colour it dumps is sum / weight (the last bit can differ)."""
    keys, tsdf, weight, colour = dump
    w = np.asarray(weight, np.float64)[..., None]
    with np.errstate(invalid="ignore", divide="ignore"):
        return keys, tsdf, weight, np.where(w > 0, np.rint(np.asarray(colour, np.float64) * w) / w, 0.0)


def fuse_reference(dump, spec, moved=False):
    """-> the oracle.PortTsdf that holds `dump` with the frames of `spec` fused on top."""
    from tests.test_gpu_tsdf_edges import intrinsic

    s, frames = frames_for(spec)
    cpu = oracle_of(dump)
    K = intrinsic(s).as_array()
    for d, c, T in frames:
        cpu.integrate(d, c, K, T @ MOVE if moved else T, 1.0, 4.0)
    return cpu


def pack_state(dump):
    """A dump as tests/pack_reference.py's state (word order, integer weights and colour sums)."""
    from tests import pack_reference as pr

    keys, tsdf, weight, colour = dump
    w = pr.to_word_order(weight)
    return (np.asarray(keys, np.int32), pr.to_word_order(np.asarray(tsdf, np.float32)).view(np.uint32), w.astype(np.uint32),
            np.rint(pr.to_word_order(colour) * w[..., None]).astype(np.uint32))


def repack_reference(dump):
    """pack_reference, check_reference, unpack_reference: -> (the dump that comes back, (units, voxels, bytes))."""
    from tests import pack_reference as pr

    buf = pr.pack_reference(*pack_state(dump), voxel_length=VOX, sdf_trunc=TRUNC)
    h = pr.check_reference(buf)
    keys, tsdf_bits, weight, sums = pr.unpack_reference(buf)
    U = len(keys)
    back = lambda a: a.reshape((U, 16, 16, 16) + a.shape[2:]).transpose((0, 2, 3, 1) + tuple(range(4, 2 + a.ndim))).reshape(a.shape)
    w = back(weight).astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        colour = np.where(w[..., None] > 0, back(sums).astype(np.float64) / w[..., None].astype(np.float64), 0.0)
    return (keys, np.ascontiguousarray(back(tsdf_bits)).view(np.float32), w, colour), (h["units"], h["voxels"], h["bytes"])


def reference_step(dump, step, sources=None):
    """One step applied to `dump` by its restatement.  -> (dump afterwards, the stats the call must return or None, extra) with
    extra = {"oracle": PortTsdf} after a fuse, {"components": ...} for a removal.  sources: name -> dump of the merge sources
    (default: the planted states' as_dump)."""
    from tests import components_reference as cr
    from tests.deintegrate_reference import deintegrate_reference
    from tests.merge_reference import merge_reference
    from tests.prune_reference import prune_reference

    op, arg = step.op, step.arg
    if op in ("fuse", "fuse_batch"):
        cpu = fuse_reference(dump, arg)
        return as_held(cpu.dump()), None, {"oracle": cpu}
    if op == "deintegrate_batch":
        after, stats = deintegrate_reference(dump, samples_for(arg))
        return after, stats, {}
    if op == "reintegrate_batch":
        mid, stats = deintegrate_reference(dump, samples_for(arg))
        cpu = fuse_reference(mid, arg, moved=True)
        return as_held(cpu.dump()), stats, {"oracle": cpu, "removed": mid}
    if op == "prune":
        after, stats = prune_reference(dump, *arg)
        return after, stats, {}
    if op == "merge":
        src = ps.as_dump(source(arg[0])) if sources is None else sources[arg[0]]
        after, stats = merge_reference(dump, src, TRANSFORMS[arg[1]], VOX)
        return after, stats, {"source": src}
    if op == "remove_small":
        ref = cr.components(dump)
        after, stats = cr.remove_components(dump, arg[0], arg[1], ref=ref)
        return after, stats, {"components": ref}
    if op == "repack":
        after, stats = repack_reference(dump)
        return after, stats, {}
    assert op == "mark_merged" or op in READER_STEPS, op
    return dump, None, {}


def same_bits(a, b):
    return all(x.shape == y.shape and np.array_equal(x.view(np.uint8) if x.dtype == np.float32 else x, y.view(np.uint8) if y.dtype == np.float32 else y)
               for x, y in zip(a, b))


def sign_changes(dump):
    """A cheap fingerprint of the surface: (sign changes between observed axis neighbours inside the units, observed voxels)."""
    t, w = np.asarray(dump[1]).reshape(-1, 16, 16, 16), np.asarray(dump[2]).reshape(-1, 16, 16, 16)
    inside, seen = t <= 0, w > 0
    n = 0
    for axis in (1, 2, 3):
        a, b = [slice(None)] * 4, [slice(None)] * 4
        a[axis], b[axis] = slice(0, 15), slice(1, 16)
        a, b = tuple(a), tuple(b)
        n += int((seen[a] & seen[b] & (inside[a] != inside[b])).sum())
    return n, int(seen.sum())


def sample_positions(dump, n, seed=7):
    """n float64 points in the bounding box of the dump's units, grown by a quarter unit."""
    keys = np.asarray(dump[0], np.float64).reshape(-1, 3)
    lo, hi = (keys.min(axis=0) - 0.25) * ps.UNIT, (keys.max(axis=0) + 1.25) * ps.UNIT
    return np.random.default_rng(seed).uniform(lo, hi, (n, 3))
