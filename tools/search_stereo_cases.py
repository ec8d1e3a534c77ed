"""The searches behind the seeded cases of tests/stereo_cases.py (PLANTED), on the CPU with tests/stereo_reference.py - run it again
after a change of the generators and carry what it prints into that file and into tests/test_stereo_planted_cpu.py.

    python tools/search_stereo_cases.py seeds      the rule 6 equality seeds, the left-of-image settings, the max_diff = 3 seed
    python tools/search_stereo_cases.py events     events() of every planted case, and the table of the CPU test's docstring
    python tools/search_stereo_cases.py kills      pixels in which every wrong reading differs from the right one, per planted case
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import stereo_cases as sc  # noqa: E402
from tests import stereo_reference as sr  # noqa: E402
from tests.test_stereo_planted_cpu import AFTER_S, pixels_apart  # noqa: E402


def apart(left, right, variant, **params):
    S = sr.volume(left, right, **params)
    Sv = S if variant in AFTER_S else sr.volume(left, right, variant=variant, **params)
    return pixels_apart(sr.finish(S, **params), sr.finish(Sv, variant=variant, **params))


def seeds():
    bf = dict(bf=sc.BF_24)
    for u in (0, 20, 50):  # a valid pixel that rule 6 keeps by its strictness alone, S(d*) > 0
        for seed in range(3000):
            left, right = sc.shifted_noise(6, 24, 5, seed)
            params = dict(num_disparities=16, uniqueness_ratio=u, **bf)
            if apart(left, right, "unique_le", **params) and sr.events(left, right, **params)["unique_equality"]:
                print(f"equality u = {u}: seed {seed}")
                break
    left, right = sc.left_of_image_pair()
    for paths in (4, 8):  # a unique winner with x - d* < 0
        for p1 in (10, 60, 100, 200):
            for p2 in (120, 1023):
                params = dict(num_disparities=16, paths=paths, p1=p1, p2=p2, uniqueness_ratio=0, max_diff=1, **bf)
                n = sr.events(left, right, **params)["winner_left_of_image"]
                if p1 <= p2 and n:
                    print(f"left of image: paths {paths}, p1 {p1}, p2 {p2}: {n} pixels, lr_clamped differs in {apart(left, right, 'lr_clamped', **params)}")
    for seed in range(100):  # |dR - d*| = 3 and = 4 in one small pair
        left, right = sc.textured_pair(9, 40, 1, seed)
        ev = sr.events(left, right, num_disparities=16, max_diff=3)
        if ev["lr_diff_eq_max"] and ev["lr_diff_eq_max_plus_1"]:
            print(f"max_diff 3: seed {seed}")
            break


def events():
    counts = {name: sr.events(left, right, **params) for name, left, right, params in sc.PLANTED}
    for name, ev in counts.items():
        print(name, {k: v for k, v in ev.items() if v})
    for e in sr.EVENTS:
        reach = {name: ev[e] for name, ev in counts.items() if ev[e]}
        best = max(reach, key=reach.get) if reach else "UNREACHED"
        print(f"    {e:28s}{best:25s}{reach.get(best, 0):7d}{len(reach):8d}{sum(reach.values()):10d}")


def kills():
    for v in sr.VARIANTS:
        row = {}
        for name, left, right, params in sc.PLANTED:
            if not (v.startswith("grey") and left.ndim == 2):
                row[name] = apart(left, right, v, **params)
        print(v, {k: n for k, n in row.items() if n})


if __name__ == "__main__":
    {"seeds": seeds, "events": events, "kills": kills}[sys.argv[1] if len(sys.argv) > 1 else "events"]()
