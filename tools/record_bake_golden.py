#!/usr/bin/env python3
"""Writes tests/golden/host_route_bake.npz: the device arrays (nnbvh_scene_read / nnbvh_kd_scene_read) and the
*_scene_info numbers of the scenes of tests/bake_golden_scenes.py, created through the host-tree calls.  Run ONCE, on a
GPU, from the last commit whose host-tree two-level and kd calls baked on the host (the parent of the commit that
moved them to the device bakers): the file is what that independent writer of the layout produced, and
tests/test_bake_golden.py holds every later baker to it.  Data only.

Scenes are stored whole, smallest first, while the raw bytes stay under --budget; of the rest every array is stored as
its SHA-256 and its length ("<scene>/<array>/sha256", "<scene>/<array>/len")."""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import bake_golden_scenes as bg
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "host_route_bake.npz"))
    ap.add_argument("--budget", type=int, default=860 << 10, help="raw bytes of the scenes stored whole")
    a = ap.parse_args()
    shots = {}
    for name, make in bg.scenes().items():
        family, agg, _ = make()
        try:
            shots[name] = bg.snapshot(family, agg)
        finally:
            agg.close()
    out, used = {}, 0
    for name in sorted(shots, key=lambda n: sum(x.nbytes for x in shots[n].values())):
        size = sum(x.nbytes for x in shots[name].values())
        whole = used + size <= a.budget
        used += size if whole else 0
        for array, x in shots[name].items():
            if whole or array == "info":
                out[f"{name}/{array}"] = x
            else:
                out[f"{name}/{array}/sha256"] = np.frombuffer(hashlib.sha256(x.tobytes()).digest(), np.uint8)
                out[f"{name}/{array}/len"] = np.array(x.nbytes, np.int64)
        print(f"{name}: {size} bytes, {'whole' if whole else 'hashed'}")
    np.savez_compressed(a.out, **out)
    print(f"{a.out}: {os.path.getsize(a.out)} bytes, {len(shots)} scenes, {used} raw bytes stored whole")


if __name__ == "__main__":
    main()
