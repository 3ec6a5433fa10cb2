"""The baked device layout against recorded bytes.  tests/golden/host_route_bake.npz holds what the host-tree creation
calls put on the device when two-level and kd-tree scenes were still baked by host code of their own (written by
tools/record_bake_golden.py from that commit): interior records, primitive stream and animation table of the BVH
scenes; nodes, indices, primitive records and attribute slots of the kd scenes; the *_scene_info numbers of both.  The
same calls bake on the device now, with the baker the device-built routes use, so the "host route == device route"
tests no longer compare two writers of the layout.  This file does: one of them is the recording."""
import hashlib
import os

import numpy as np
import pytest

import bake_golden_scenes as bg

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "host_route_bake.npz")
SCENES = bg.scenes()


def first_difference(family, array, got, exp, kinds):
    """the first 16-byte slot that differs, and the kind of the primitive it belongs to where the array has primitives"""
    n = min(len(got), len(exp))
    bad = np.nonzero(got[:n] != exp[:n])[0]
    if len(bad) == 0:
        return f"{len(got)} bytes against the recorded {len(exp)}"
    slot = int(bad[0]) // 16
    words = f"slot {slot} (byte {int(bad[0])}): {got[16 * slot:16 * slot + 16].view(np.uint32)} against the recorded " \
            f"{exp[16 * slot:16 * slot + 16].view(np.uint32)}"
    prim = None
    if family == "bvh" and array == "stream":
        prim = int(np.searchsorted(np.cumsum(bg.stream_slots(kinds)), slot, side="right"))
    elif family == "kd" and array in ("records", "extras"):
        prim = slot // (4 if array == "records" else 6)
    if prim is not None and prim < len(kinds):
        words += f", primitive {prim} of kind {int(kinds[prim])}"
    return words


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


def test_the_fixture_has_every_scene_and_only_data(golden):
    arrays = {"bvh": set(bg.BVH_ARRAYS) | {"info"}, "kd": set(bg.KD_ARRAYS) | {"info"}}
    seen = {}
    for key in golden.files:
        assert golden[key].dtype in (np.uint8, np.int64), key
        for name in SCENES:
            if key.startswith(name + "/"):
                seen.setdefault(name, set()).add(key[len(name) + 1:].split("/")[0])
    assert set(seen) == set(SCENES)
    assert all(got in (arrays["bvh"], arrays["kd"]) for got in seen.values()), seen
    assert os.path.getsize(GOLDEN) < 1 << 20
    # whole scenes of both families, the two-level ones with every kind among them
    assert all(f"{n}/stream" in golden.files for n in ("flat", "two_level_alpha_texture/static", "edge_shape/unnamed object"))
    assert any(k.startswith("kd_") and k.endswith("/extras") and len(golden[k]) for k in golden.files)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENES))
def test_host_tree_routes_bake_the_recorded_bytes(golden, name):
    family, agg, kinds = SCENES[name]()
    try:
        got = bg.snapshot(family, agg)
    finally:
        agg.close()
    assert np.array_equal(got.pop("info"), golden[f"{name}/info"]), (name, "scene_info")
    for array, x in got.items():
        key = f"{name}/{array}"
        if key in golden.files:
            exp = golden[key]
            assert x.tobytes() == exp.tobytes(), f"{name}, {array}: " + first_difference(family, array, x, exp, kinds)
        else:
            assert len(x) == int(golden[key + "/len"]), (name, array, len(x))
            assert hashlib.sha256(x.tobytes()).digest() == golden[key + "/sha256"].tobytes(), \
                f"{name}, {array}: SHA-256 differs from the recorded one (the scene is too large to be stored whole)"
