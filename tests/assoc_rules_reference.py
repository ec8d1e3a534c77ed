"""TEST INFRASTRUCTURE ONLY - the voting rules of assign_object_ids_to_instance_ids (voxel_semantic_data_association.h:268-361)
restated with dictionaries.  Input: the (instance, object, votes) pairs of one keyframe as the staged interface carries them
(hv_assoc_pairs_fetch / hv_assoc_pairs_set): a vote of a voxel that waits for a new object id has the object PENDING, an instance id
that merely occurs in the image (with a valid class) has the marker SEEN.  Shares nothing with the rules kernel (no sort, no packed
keys) and nothing with oracle/semantic2_oracle.c (which counts while it visits and never sees markers)."""
import numpy as np

PENDING = -(2 ** 31)      # INT32_MIN
SEEN = -(2 ** 31) + 1     # INT32_MIN + 1


def decide(pairs, min_vote_ratio, min_votes, next_object_id):
    """-> ({instance: object}, next object id afterwards)."""
    votes, pending, seen = {}, {}, set()
    for inst, obj, n in pairs:
        inst, obj, n = int(inst), int(obj), int(n)
        if obj == SEEN:
            seen.add(inst)
        elif obj == PENDING:
            pending[inst] = pending.get(inst, 0) + n
        else:  # equal pairs (several GPUs' lists) add up
            per = votes.setdefault(inst, {})
            per[obj] = per.get(obj, 0) + n
    # instances whose voxels wait for an id get new ones in ascending instance order; the waiting votes are votes for that id
    next_id = int(next_object_id)
    for inst in sorted(pending):
        if pending[inst] <= 0:
            continue
        per = votes.setdefault(inst, {})
        per[next_id] = per.get(next_id, 0) + pending[inst]
        next_id += 1
    out = {}
    for inst, per in votes.items():
        best, winner, total = 0, -1, 0
        for obj in sorted(per):  # ascending object id; the first strict maximum wins
            total += per[obj]
            if per[obj] > best:
                best, winner = per[obj], obj
        if total < int(min_votes):
            out[inst] = -1
        elif np.float32(best) / np.float32(total) < np.float32(min_vote_ratio):
            out[inst] = -1
        else:
            out[inst] = winner
    for inst in seen:
        if inst == 0:
            out[0] = 0
        elif inst not in out:
            out[inst] = -1
    return out, next_id


def pack_pairs(pairs):
    """-> (keys u64 = instance << 32 | object (two's complement), votes i32) for assoc_set_pairs."""
    keys = np.array([((int(i) & 0xFFFFFFFF) << 32) | (int(o) & 0xFFFFFFFF) for i, o, _ in pairs], np.uint64)
    return keys, np.array([int(n) for _, _, n in pairs], np.int32)


def unpack_pairs(keys, counts):
    """The inverse: -> sorted list of (instance, object, votes)."""
    out = []
    for k, n in zip(np.asarray(keys, np.uint64).tolist(), np.asarray(counts).tolist()):
        inst, obj = k >> 32, k & 0xFFFFFFFF
        out.append((inst - (1 << 32) if inst >= 1 << 31 else inst, obj - (1 << 32) if obj >= 1 << 31 else obj, int(n)))
    return sorted(out)
