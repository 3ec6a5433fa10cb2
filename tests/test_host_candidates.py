"""Host-only primitives returned as candidates instead of voiding the ray (include/nnbvh.h
nnbvh_host_candidates): the device hit plus the list of host-only primitives a ray reached, merged by the
caller with the reference's order of acceptance (aggregates.cpp:529-624).  CPU: the merge rule against a
sequential replay, the ABI's argument checks.  GPU: scenes whose host-declared primitives are triangles, so
that the resolved answer can be held bit for bit to the oracle on the same scene with them as triangles."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle_binding as ob
import scenes_small as ss
from ledger_cases import BVH, bvh, reaches
from nn_bvh_amd import (BVHAggregate, _lib, build_tree, candidates_dtype, instancing, resolve_host_candidates,
                        resolve_host_candidates_any, scene)
from nn_bvh_amd._lib import HIT_DTYPE, RAY_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 1
# case -> (kernel family, the instances its device calls launch), asserted by `reaches` (tests/ledger_cases.py): the
# candidate twins <0/2,8,INST,1,0,0,1> of the two-level forms; the static case also makes the plain Intersect call
LEDGER = {
    "test_two_level_static_closest_and_any_hit": (BVH, bvh((0, 2), inst=1, hostc=1) | bvh((0,), inst=1)),
    "test_two_level_animated_closest_and_any_hit": (BVH, bvh((0, 2), inst=2, hostc=1)),
}


# ---- the merge rule, CPU ---------------------------------------------------------------------------------
def replay(tmax, events):
    """The reference's loop in traversal order: each primitive is tested against the running tMax and a hit
    replaces the result.  events: list of (name, t, kind) with kind "tri" (accept t <= tMax, the equal-t case of
    Triangle::Intersect) or "patch" (accept t < tMax) or "miss"."""
    best = None
    for name, t, kind in events:
        if kind == "miss":
            continue
        if (kind == "tri" and t <= tmax) or (kind == "patch" and t < tmax):
            best, tmax = name, t
    return best, tmax


def run_case(tmax, host, before, device, device_kind="tri"):
    """host: list of (t or None) in traversal order; the device hit (t or None) sits after `before` of them."""
    k = max(len(host), 1)
    rays = np.zeros(1, RAY_DTYPE)
    rays["tmax"] = tmax
    hits = np.zeros(1, HIT_DTYPE)
    hits["prim"] = -1 if device is None else 100
    hits["t"] = tmax if device is None else device
    hits["b0"], hits["nodes_visited"], hits["prim_tests"] = 0.25, 7, 3
    cands = np.zeros(1, candidates_dtype(k))
    cands["count"], cands["before"] = len(host), before
    cands["prim"][0, :len(host)] = np.arange(len(host))
    ht = np.array([np.nan if t is None else t for t in host] + [np.nan] * (k - len(host)), np.float32)

    def cb(idx, prim, inst, tm):  # a host triangle at ht[prim]: accepted iff t <= tMax
        t = ht[prim]
        hit = ~np.isnan(t) & (t <= tm)
        return hit, t, np.full(len(idx), 0.5, np.float32), np.zeros(len(idx), np.float32), np.zeros(len(idx), np.float32)

    kind = np.zeros(101, np.int32)
    kind[100] = 1 if device_kind == "patch" else 0
    res = resolve_host_candidates(rays, hits, cands, cb, kind=kind)
    events = [(j, t, "miss" if t is None else "tri") for j, t in enumerate(host[:before])]
    if device is not None:
        events.append(("dev", device, device_kind))
    events += [(j, t, "miss" if t is None else "tri") for j, t in enumerate(host[before:], before)]
    best, t_end = replay(np.float32(tmax), events)
    return res[0], best, t_end


@pytest.mark.parametrize("tmax,host,before,device,device_kind", [
    (np.inf, [2.0], 1, 5.0, "tri"),          # host hit before the device hit, nearer: host wins
    (np.inf, [7.0], 1, 5.0, "tri"),          # ... farther: the device hit replaces it
    (np.inf, [5.0], 1, 5.0, "tri"),          # tie, host first: a triangle accepts an equal t
    (np.inf, [5.0], 1, 5.0, "patch"),        # tie, host first: a patch rejects an equal t
    (np.inf, [5.0], 0, 5.0, "tri"),          # tie, device first: the host test (t <= tMax) decides
    (np.inf, [2.0], 0, 5.0, "tri"),          # host after the device hit, nearer
    (np.inf, [7.0], 0, 5.0, "tri"),          # host after the device hit, farther
    (np.inf, [9.0, 3.0, 4.0], 3, 5.0, "tri"),  # before = count
    (np.inf, [9.0, 3.0, 1.0], 0, 5.0, "tri"),  # before = 0
    (np.inf, [9.0, None, 2.5, 6.0], 2, 4.0, "tri"),
    (np.inf, [None, 3.0], 1, 5.0, "tri"),    # a host miss before, a hit after
    (np.inf, [3.0, 2.0], 0, None, "tri"),    # a miss on the device, candidates only
    (np.inf, [None, None], 0, None, "tri"),  # a miss everywhere
    (4.0, [4.5, 3.5], 0, None, "tri"),       # the ray's tmax bounds the candidates
])
def test_merge_rule_equals_sequential_replay(tmax, host, before, device, device_kind):
    r, best, t_end = run_case(tmax, host, before, device, device_kind)
    if best is None:
        assert r["prim"] == -1 and r["t"] == np.float32(tmax)
    elif best == "dev":
        assert r["prim"] == 100 and r["t"] == np.float32(device) and r["b0"] == np.float32(0.25)
    else:
        assert r["prim"] == best and r["t"] == np.float32(host[best]) and r["b0"] == np.float32(0.5)
    assert r["nodes_visited"] == 7 and r["prim_tests"] == 3 and r["instance"] == 0


def test_merge_rule_void_rays_and_any_hit():
    rays = np.zeros(4, RAY_DTYPE)
    rays["tmax"] = [np.inf, np.inf, 3.0, np.inf]
    hits = np.zeros(4, HIT_DTYPE)
    hits["prim"], hits["instance"] = [-1, 5, -1, -1], [-1, -1, 0, 0]
    cands = np.zeros(4, candidates_dtype(2))
    cands["count"] = [-1, -2, 2, 1]
    cands["prim"][2] = [0, 1]
    cands["prim"][3] = [1, -1]
    calls = []

    def cb(idx, prim, inst, tm):
        calls.append(idx.copy())
        t = np.array([4.0, 2.0], np.float32)[prim]
        return t <= tm, t, np.zeros(len(idx)), np.zeros(len(idx)), np.zeros(len(idx))

    res = resolve_host_candidates(rays, hits, cands, cb)
    assert res[:2].tobytes() == hits[:2].tobytes()  # void rays are left as they came
    assert res["prim"][2] == 1 and res["t"][2] == 2.0 and res["prim"][3] == 1
    assert all((c >= 2).all() for c in calls)  # count < 0 is never handed to the callback
    occ = np.array([2, 2, 2, 1], np.uint8)
    cands["count"][3] = 0
    rays["tmax"][2] = 1.5  # neither candidate of ray 2 within tmax: not occluded
    got = resolve_host_candidates_any(rays, occ, cands, cb)
    assert list(got) == [2, 2, 0, 1]
    rays["tmax"][2] = 2.5
    assert list(resolve_host_candidates_any(rays, occ, cands, cb)) == [2, 2, 1, 1]


C_PROBE = r"""
#include <stdio.h>
#include "nnbvh.h"
int main(void) {
    int32_t count[1], before[1], prim[4], inst[4];
    nnbvh_host_candidates c = {4, count, before, prim, inst};
    nnbvh_ray r = {{0, 0, 0}, 1.0f, {0, 0, 1}, 0.0f};
    nnbvh_hit h;
    uint8_t occ;
    printf("%d %d %d %d\n", nnbvh_intersect_closest_candidates(NULL, &r, 1, &h, &c),
           nnbvh_intersect_any_candidates(NULL, &r, 1, &occ, &c),
           nnbvh_intersect_closest_candidates_device(NULL, &r, 1, &h, &c, NULL),
           nnbvh_intersect_any_candidates_device(NULL, &r, 1, &occ, &c, NULL));
    return 0;
}
"""


def test_candidate_abi_exports_compiles_as_c11_and_rejects_a_null_scene(nnbvh_lib, tmp_path):
    for s in ("nnbvh_intersect_closest_candidates", "nnbvh_intersect_any_candidates",
              "nnbvh_intersect_closest_candidates_device", "nnbvh_intersect_any_candidates_device"):
        assert s in _lib.EXPORTS and hasattr(nnbvh_lib, s)
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(C_PROBE)
    libdir = os.path.join(ROOT, "nn_bvh_amd")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(exe), "-L", libdir, "-l:libnnbvh_hip.so", f"-Wl,-rpath,{libdir}",
                    "-Wl,-rpath-link,/opt/rocm/lib"], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.split() == [str(ERR_ARG)] * 4
    rays = np.zeros(1, RAY_DTYPE)
    hits = np.zeros(1, HIT_DTYPE)
    cnt, bef, pr, ins = (np.zeros(8, np.int32) for _ in range(4))
    c = _lib.HostCandidates(8, cnt.ctypes.data, bef.ctypes.data, pr.ctypes.data, ins.ctypes.data)
    assert nnbvh_lib.nnbvh_intersect_closest_candidates(None, _lib.ptr(rays), 1, _lib.ptr(hits),
                                                        ctypes.byref(c)) == ERR_ARG


# ---- GPU ------------------------------------------------------------------------------------------------
def tri_callback(rays, verts, tri_by_id, minv=None):
    """host_intersect backed by the oracle's pinned triangle test (shapes.cpp:172-273).  tri_by_id[id] = the
    triangle's three vertex indices; minv(ray_idx, k) -> prim_from_render rows [n, 12] of instance k, applied
    with the reference's ApplyInverse (TransformedPrimitive::Intersect, primitive.cpp:112-126)."""
    def cb(idx, prim, inst, tmax):
        o, d, tm = rays["o"][idx].copy(), rays["d"][idx].copy(), np.asarray(tmax, np.float32).copy()
        m = inst > 0
        if m.any():
            x = ob.apply_inverse_ray(minv(idx[m], inst[m] - 1), o[m], d[m], tm[m])
            o[m], d[m], tm[m] = x[:, :3], x[:, 3:6], x[:, 6]
        p9 = verts[tri_by_id[prim]].reshape(-1, 9)
        hit, out = ob.leaf_batch("tri", np.concatenate([o, d, tm[:, None], p9], 1))
        return hit.astype(bool), out[:, 3], out[:, 0], out[:, 1], out[:, 2]
    return cb


def tri_table(prims):
    t = np.zeros((prims["id"].max() + 1, 3), np.int64)
    t[prims["id"]] = prims["v"][:, :3]
    return t


def assert_same_but_instance(a, b):
    """Byte-equal records in every field but instance."""
    for f in HIT_DTYPE.names:
        if f != "instance":
            assert np.array_equal(a[f].view(np.uint32), b[f].view(np.uint32)), f


def assert_resolved_equal(res, exp, what):
    for f in ("prim", "instance"):
        bad = np.nonzero(res[f] != exp[f])[0]
        assert len(bad) == 0, f"{what}: {f} differs on {len(bad)} rays, first {bad[:5]}"
    for f in ("t", "b0", "b1", "b2"):
        bad = np.nonzero(res[f].view(np.uint32) != exp[f].view(np.uint32))[0]
        assert len(bad) == 0, f"{what}: {f} not bit-equal on {len(bad)} rays, first {bad[:5]}"


def flat_host_scene(seed=0, n=1500):
    """tests/test_instancing.py host_prim_scene: every 7th triangle declared host-only with its exact bounds;
    and the same soup as triangles."""
    verts, prims = ss.random_soup(n, 0, seed)
    host = np.arange(len(prims)) % 7 == 3
    tri = verts[prims["v"][:, :3]]
    bounds = np.concatenate([tri.min(1), tri.max(1)], 1).astype(np.float32)
    hp = prims.copy()
    hp["kind"][host] = 3
    tree_h = build_tree(hp, verts, prim_bounds=bounds)
    tree_t = build_tree(prims, verts)
    return verts, prims, host, tree_h, tree_t


@pytest.mark.gpu
def test_flat_scene_closest_resolves_bit_exact_to_the_oracle():
    verts, prims, host, tree_h, tree_t = flat_host_scene(0)
    assert tree_h.nodes.tobytes() == tree_t.nodes.tobytes()
    assert np.array_equal(tree_h.ordered_prims["id"], tree_t.ordered_prims["id"])
    rays = np.concatenate([scene.random_rays(20000, verts.min(0), verts.max(0), 3),
                           scene.random_rays(4000, verts.min(0), verts.max(0), 4, tmax=np.float32(0.6))])
    agg = BVHAggregate.from_tree(tree_h.nodes, tree_h.ordered_prims, verts)
    hits, cands = agg.intersect_with_host_candidates(rays, capacity=16)
    plain = agg.Intersect(rays)
    agg.close()
    cnt = cands["count"]
    assert (cnt > 0).mean() > 0.05 and (cnt >= 0).mean() > 0.99
    # records unchanged: every field but instance; instance -1 today exactly where a candidate was met
    assert_same_but_instance(hits, plain)
    assert np.array_equal(plain["instance"] == -1, cnt != 0)
    assert np.array_equal(hits["instance"], np.where(cnt < 0, -1, 0))
    cb = tri_callback(rays, verts, tri_table(prims))
    res = resolve_host_candidates(rays, hits, cands, cb, kind=np.zeros(len(prims), np.int32))
    exp = ob.closest(tree_t.nodes, tree_t.ordered_prims, verts, rays, 4)
    ok = cnt >= 0
    assert_resolved_equal(res[ok], exp[ok], "flat closest")
    won_by_host = (res["prim"] >= 0) & host[np.maximum(res["prim"], 0)]
    assert won_by_host.sum() > 50
    # step 3 exercised: a device hit that comes after a candidate the ray hits
    two = np.nonzero((cands["before"] > 0) & (hits["prim"] >= 0))[0]
    h0 = cb(two, cands["prim"][two, 0], cands["instance"][two, 0], rays["tmax"][two])[0]
    assert h0.sum() > 5


@pytest.mark.gpu
def test_flat_scene_any_hit_resolves_to_the_oracle():
    verts, prims, host, tree_h, tree_t = flat_host_scene(1)
    lo, hi = verts.min(0), verts.max(0)
    rays = np.concatenate([scene.random_rays(15000, lo, hi, 5),
                           scene.random_rays(15000, lo, hi, 6, tmax=np.float32(0.5))])
    agg = BVHAggregate.from_tree(tree_h.nodes, tree_h.ordered_prims, verts)
    occ, cands = agg.intersect_p_with_host_candidates(rays, capacity=16)
    plain = agg.IntersectP(rays)
    agg.close()
    assert np.array_equal(occ, plain)  # the occlusion flags are today's
    # an occluder ends the walk (its list may be partial); otherwise occluded 2 exactly where candidates were met
    assert (cands["before"] == 0).all() and np.array_equal(occ == 2, (cands["count"] != 0) & (occ != 1))
    assert (occ == 2).sum() > 500 and (cands["count"] >= 0).mean() > 0.99
    res = resolve_host_candidates_any(rays, occ, cands, tri_callback(rays, verts, tri_table(prims)))
    exp = ob.any_hit(tree_t.nodes, tree_t.ordered_prims, verts, rays, 4)[0]
    assert np.array_equal(res == 2, (occ == 2) & (cands["count"] < 0))
    for finite in (False, True):
        m = (np.isfinite(rays["tmax"]) == finite) & (res != 2)
        assert np.array_equal(res[m], exp[m])
    assert ((occ == 2) & (res == 1)).sum() > 50 and ((occ == 2) & (res == 0)).sum() > 50


@pytest.mark.gpu
def test_ties_of_duplicated_triangles_in_both_leaf_orders():
    """Each triangle twice (same three vertices): one copy host-only, one on the device; for half of the pairs
    the host copy comes first in its leaf.  An equal t is where the comparison on t stands in for the
    triangle's own test (include/nnbvh.h): re-testing the device primitive gives the oracle exactly; the
    comparison accepts every equal t, and differs from the oracle only on host-first ties the reference's
    tScaled test rejects."""
    verts, base = ss.random_soup(600, 0, 7, extent=6.0, size=1.0)
    n = len(base)
    dup = np.concatenate([base, base])
    dup["id"] = np.arange(2 * n)
    tree = build_tree(dup, verts)
    op = tree.ordered_prims.copy()
    pos = np.empty(2 * n, np.int64)
    pos[op["id"]] = np.arange(2 * n)
    first = np.where(pos[:n] < pos[n:], np.arange(n), np.arange(n) + n)  # the pair's first copy in leaf order
    second = np.where(first < n, first + n, first - n)
    host_first = np.arange(n) % 2 == 0
    host_ids = np.where(host_first, first, second)
    is_host = np.zeros(2 * n, bool)
    is_host[host_ids] = True
    op["kind"][is_host[op["id"]]] = 3
    rays = scene.random_rays(30000, verts.min(0), verts.max(0), 8)
    agg = BVHAggregate.from_tree(tree.nodes, op, verts)
    hits, cands = agg.intersect_with_host_candidates(rays, capacity=16)
    agg.close()
    ok = cands["count"] >= 0
    assert ok.mean() > 0.9
    rays, hits, cands = rays[ok], hits[ok], cands[ok]
    exp = ob.closest(tree.nodes, tree.ordered_prims, verts, rays, 4)
    cb = tri_callback(rays, verts, tri_table(dup))
    exact = resolve_host_candidates(rays, hits, cands, cb, device_intersect=cb)
    assert_resolved_equal(exact, exp, "ties, device primitive re-tested")
    by_t = resolve_host_candidates(rays, hits, cands, cb, kind=np.zeros(2 * n, np.int32))
    pair = np.maximum(exp["prim"], 0) % n
    hit = exp["prim"] >= 0
    assert (hit & host_first[pair]).sum() > 500 and (hit & ~host_first[pair]).sum() > 500
    # device-first pairs: the host copy is tested by the reference's own test after the device hit
    dev_first = hit & ~host_first[pair]
    assert np.array_equal(by_t["prim"][dev_first], exp["prim"][dev_first])
    # host-first pairs: an equal t is accepted, so the device copy stands wherever the device hit that pair
    hf = hit & host_first[pair] & (hits["prim"] >= 0) & (hits["prim"] % n == pair)
    assert (by_t["prim"][hf] == hits["prim"][hf]).all()
    differ = by_t["prim"] != exp["prim"]
    assert (differ <= hf).all() and (exp["prim"][differ] == host_ids[pair[differ]]).all()
    assert differ.sum() < 0.25 * hf.sum()
    for f in ("t", "b0", "b1", "b2"):  # the copies are the same triangle: the hit itself is the oracle's
        assert np.array_equal(by_t[f].view(np.uint32), exp[f].view(np.uint32))


def unique_id_two_level(seed=0, n_place=40):
    """Two object definitions and top-level triangles with ids unique across the scene (so that a candidate's id
    names its triangle), all triangles."""
    from test_oracle_vs_reference_live import random_affine
    rng = np.random.default_rng(seed)
    va, pa = ss.grid_mesh(12, seed)
    vb, pb = ss.random_soup(150, 0, seed + 1, extent=1.0, size=0.2)
    vt, pt = ss.random_soup(60, 0, seed + 2, extent=30.0, size=2.0)
    pb, pt = pb.copy(), pt.copy()
    pb["v"][:, :3] += len(va)
    pt["v"][:, :3] += len(va) + len(vb)
    pb["id"] += len(pa)
    pt["id"] += len(pa) + len(pb)
    verts = np.concatenate([va, vb, vt]).astype(np.float32)
    M, _ = random_affine(rng, n_place)
    M[:, :3, 3] = rng.uniform(-25, 25, size=(n_place, 3))
    M[:, :3, :3] *= (0.3 / np.abs(M[:, :3, :3]).max((1, 2)))[:, None, None] * rng.uniform(1, 6, (n_place, 1, 1))
    Mi = np.linalg.inv(M.astype(np.float64)).astype(np.float32)
    placements = [(int(rng.integers(0, 2)), M[j, :3].reshape(12), Mi[j, :3].reshape(12)) for j in range(n_place)]
    nodes, prims, instances, n_top = instancing.assemble_two_level(pt, verts, [pa, pb], placements)
    return verts, nodes, prims, instances, n_top, np.concatenate([pa, pb, pt]), placements, (pa, pb)


def declare_host(prims, every, offset):
    """Flip every `every`-th triangle to host-only in the baked order (the tree does not change: host-only
    primitives' bounds are their triangles' bounds)."""
    hp = prims.copy()
    tri = np.nonzero(hp["kind"] == 0)[0]
    hp["kind"][tri[offset::every]] = 3
    return hp


def check_instances_entered(cands, placements, objects, top_level=True):
    """Every candidate inside instance k is a triangle of the object placed as instance k."""
    k = cands["prim"].shape[1]
    j = np.arange(k)[None, :] < np.maximum(cands["count"], 0)[:, None]
    inst, prim = cands["instance"][j], cands["prim"][j]
    assert (inst > 0).sum() > 100 and (not top_level or (inst == 0).sum() > 5)
    obj = np.array([p[0] for p in placements])
    for o, op in enumerate(objects):
        m = (inst > 0) & (obj[np.maximum(inst - 1, 0)] == o)
        assert np.isin(prim[m], op["id"]).all()


@pytest.mark.gpu
def test_two_level_static_closest_and_any_hit():
    verts, nodes, prims, instances, n_top, all_tris, placements, objects = unique_id_two_level(2, 50)
    hp = declare_host(prims, 5, 2)
    lo = np.array([-30, -30, -30.0])
    rays = np.concatenate([scene.random_rays(25000, lo, -lo, 21),
                           scene.random_rays(5000, lo, -lo, 22, tmax=np.float32(0.5))])
    with reaches(LEDGER, "test_two_level_static_closest_and_any_hit"):
        agg = BVHAggregate.from_tree(nodes, hp, verts, instances=instances, n_top_nodes=n_top)
        hits, cands = agg.intersect_with_host_candidates(rays, capacity=16)
        plain = agg.Intersect(rays)
        occ, acands = agg.intersect_p_with_host_candidates(rays, capacity=16)
        agg.close()
    assert (cands["count"] >= 0).mean() > 0.99 and (cands["count"] > 0).mean() > 0.02
    assert_same_but_instance(hits, plain)
    assert np.array_equal(plain["instance"] == -1, cands["count"] != 0)
    check_instances_entered(cands, placements, objects)
    minv = lambda idx, k: instances["prim_from_render"][k]  # noqa: E731
    cb = tri_callback(rays, verts, tri_table(all_tris), minv)
    res = resolve_host_candidates(rays, hits, cands, cb, kind=np.zeros(len(all_tris), np.int32))
    exp = ob.closest_inst(nodes, prims, verts, instances, rays, 4)
    ok = cands["count"] >= 0
    assert_resolved_equal(res[ok], exp[ok], "two-level closest")
    is_host = np.zeros(len(all_tris), bool)
    is_host[hp["id"][hp["kind"] == 3]] = True
    assert ((res["instance"] > 0) & is_host[np.maximum(res["prim"], 0)] & (res["prim"] >= 0)).sum() > 20
    got = resolve_host_candidates_any(rays, occ, acands, cb)
    settled = got != 2
    assert settled.mean() > 0.99
    assert np.array_equal(got[settled], ob.any_hit_inst(nodes, prims, verts, instances, rays, 4)[0][settled])


@pytest.mark.gpu
def test_two_level_animated_closest_and_any_hit():
    from test_animated import animated_scene, rebuild_with_motion_bounds
    verts, prims0, _, _, _, _, anims, oa, placements = animated_scene(4, 30)
    nodes, aprims, instances, n_top = rebuild_with_motion_bounds(verts, prims0, placements, anims, oa)
    hp = declare_host(aprims, 4, 1)
    n = 20000
    rays = scene.random_rays(n, [-25, -25, -25], [25, 25, 25], 5)
    rays["time"] = np.random.default_rng(6).uniform(-0.2, 1.2, n).astype(np.float32)
    with reaches(LEDGER, "test_two_level_animated_closest_and_any_hit"):
        agg = BVHAggregate.from_tree(nodes, hp, verts, instances=instances, n_top_nodes=n_top, animated=anims)
        hits, cands = agg.intersect_with_host_candidates(rays, capacity=16)
        occ, acands = agg.intersect_p_with_host_candidates(rays, capacity=16)
        agg.close()
    assert (cands["count"] >= 0).mean() > 0.99 and (cands["count"] > 0).mean() > 0.02
    check_instances_entered(cands, placements, [prims0], top_level=False)

    def minv(idx, k):
        rows = instances["prim_from_render"][k].copy()
        a = anims["actually_animated"][k] != 0
        if a.any():
            rows[a] = ob.anim_interpolate(oa[k[a]], rays["time"][idx[a]])[:, 16:28]
        return rows

    try:
        ob.set_sin_mode(1)  # the device's Slerp sine (test_animated.py: the documented exception)
        cb = tri_callback(rays, verts, tri_table(prims0), minv)
        res = resolve_host_candidates(rays, hits, cands, cb, kind=np.zeros(len(prims0), np.int32))
        exp = ob.closest_anim(nodes, aprims, verts, instances, oa, rays, 4)
        got = resolve_host_candidates_any(rays, occ, acands, cb)
        eocc = ob.any_hit_anim(nodes, aprims, verts, instances, oa, rays, 4)[0]
    finally:
        ob.set_sin_mode(0)
    ok, settled = cands["count"] >= 0, got != 2
    assert settled.mean() > 0.99
    assert_resolved_equal(res[ok], exp[ok], "animated closest")
    assert np.array_equal(got[settled], eocc[settled])
    moved = anims["actually_animated"][np.maximum(res["instance"] - 1, 0)] != 0
    assert ((res["instance"] > 0) & moved).sum() > 100


@pytest.mark.gpu
def test_overflow_voids_the_ray_as_today():
    verts, prims, host, tree_h, tree_t = flat_host_scene(0)
    rays = scene.random_rays(20000, verts.min(0), verts.max(0), 3)
    agg = BVHAggregate.from_tree(tree_h.nodes, tree_h.ordered_prims, verts)
    h16, c16 = agg.intersect_with_host_candidates(rays, capacity=16)
    h1, c1 = agg.intersect_with_host_candidates(rays, capacity=1)
    occ1, a1 = agg.intersect_p_with_host_candidates(rays, capacity=1)
    plain_occ = agg.IntersectP(rays)
    agg.close()
    c16["count"][c16["count"] < 0] = 17  # more than 16
    many = c16["count"] > 1
    assert many.sum() > 20
    assert np.array_equal(c1["count"] == -1, many)
    assert (h1["instance"][many] == -1).all() and (h1["instance"][~many] == 0).all()
    assert np.array_equal(c1["count"][~many], c16["count"][~many])
    assert np.array_equal(c1["prim"][:, 0][c1["count"] == 1], c16["prim"][:, 0][c1["count"] == 1])
    assert_same_but_instance(h1, h16)
    assert np.array_equal(occ1, plain_occ) and np.array_equal(occ1 == 2, (a1["count"] != 0) & (occ1 != 1))
    assert ((a1["count"] == -1) & (occ1 == 2)).sum() > 10


@pytest.mark.gpu
def test_alpha_retrace_voids_get_count_minus_two():
    from test_alpha import alpha_scene
    verts, prims, alpha, kinds = alpha_scene(9, 800)
    tree = build_tree(prims, verts)
    rng = np.random.default_rng(3)
    rays = scene.random_rays(6000, verts.min(0) - 1, verts.max(0) + 1, 11)
    special = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1e-30], np.float32)
    for f in ("o", "d"):
        v = rays[f].copy()
        m = rng.random(v.shape) < 0.15
        v[m] = rng.choice(special, int(m.sum()))
        rays[f] = v
    agg = BVHAggregate.from_tree(tree.nodes, tree.ordered_prims, verts)
    plain = agg.Intersect(rays)
    hits, cands = agg.intersect_with_host_candidates(rays, capacity=4)
    plain_occ = agg.IntersectP(rays)
    occ, acands = agg.intersect_p_with_host_candidates(rays, capacity=4)
    agg.close()
    void = plain["instance"] == -1
    assert void.sum() > 0
    assert np.array_equal(cands["count"], np.where(void, -2, 0))
    assert hits.tobytes() == plain.tobytes()
    assert np.array_equal(occ, plain_occ) and (occ == 2).sum() > 0
    assert np.array_equal(acands["count"][occ != 1] == -2, occ[occ != 1] == 2)
    assert (acands["count"][occ == 0] == 0).all()


@pytest.mark.gpu
def test_scene_without_host_primitives_runs_the_plain_kernels():
    verts, prims = ss.random_soup(3000, 0, 11)
    tree = build_tree(prims, verts)
    rays = scene.random_rays(20000, verts.min(0), verts.max(0), 12)
    agg = BVHAggregate.from_tree(tree.nodes, tree.ordered_prims, verts)
    hits, cands = agg.intersect_with_host_candidates(rays)
    occ, acands = agg.intersect_p_with_host_candidates(rays)
    assert hits.tobytes() == agg.Intersect(rays).tobytes()
    assert np.array_equal(occ, agg.IntersectP(rays))
    agg.close()
    assert (cands["count"] == 0).all() and (cands["before"] == 0).all() and (acands["count"] == 0).all()


@pytest.mark.gpu
def test_device_forms_equal_host_forms_and_bad_arguments_launch_nothing():
    import torch
    verts, prims, host, tree_h, tree_t = flat_host_scene(2)
    rays = scene.random_rays(8000, verts.min(0), verts.max(0), 13)
    agg = BVHAggregate.from_tree(tree_h.nodes, tree_h.ordered_prims, verts)
    hits, cands = agg.intersect_with_host_candidates(rays, capacity=8)
    occ, acands = agg.intersect_p_with_host_candidates(rays, capacity=8)
    n, k = len(rays), 8
    dev = torch.device("cuda", 0)
    d_rays = torch.from_numpy(rays.view(np.uint8).copy()).to(dev)
    d_hits = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
    d_occ = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_cnt = torch.full((n,), 77, dtype=torch.int32, device=dev)
    d_bef = torch.full((n,), 77, dtype=torch.int32, device=dev)
    d_prim = torch.full((n * k,), -1, dtype=torch.int32, device=dev)
    d_inst = torch.full((n * k,), -1, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    agg.intersect_candidates_device(d_rays.data_ptr(), d_hits.data_ptr(), n, k, d_cnt.data_ptr(), d_bef.data_ptr(),
                                    d_prim.data_ptr(), d_inst.data_ptr(), stream)
    torch.cuda.synchronize(dev)
    assert d_hits.cpu().numpy().tobytes() == hits.tobytes()
    assert np.array_equal(d_cnt.cpu().numpy(), cands["count"]) and np.array_equal(d_bef.cpu().numpy(), cands["before"])
    j = np.arange(k)[None, :] < cands["count"][:, None]
    assert np.array_equal(d_prim.cpu().numpy().reshape(n, k)[j], cands["prim"][j])
    assert np.array_equal(d_inst.cpu().numpy().reshape(n, k)[j], cands["instance"][j])
    d_cnt.fill_(77)
    agg.intersect_p_candidates_device(d_rays.data_ptr(), d_occ.data_ptr(), n, k, d_cnt.data_ptr(), d_prim.data_ptr(),
                                      d_inst.data_ptr(), stream)
    torch.cuda.synchronize(dev)
    assert np.array_equal(d_occ.cpu().numpy(), occ) and np.array_equal(d_cnt.cpu().numpy(), acands["count"])
    # bad arguments: NNBVH_ERR_ARG and nothing launched (the count array keeps its sentinel)
    L = _lib.lib()
    d_cnt.fill_(77)
    torch.cuda.synchronize(dev)
    p = lambda t: t.data_ptr()  # noqa: E731
    bad = [_lib.HostCandidates(0, p(d_cnt), p(d_bef), p(d_prim), p(d_inst)),
           _lib.HostCandidates(17, p(d_cnt), p(d_bef), p(d_prim), p(d_inst)),
           _lib.HostCandidates(8, None, p(d_bef), p(d_prim), p(d_inst)),
           _lib.HostCandidates(8, p(d_cnt), None, p(d_prim), p(d_inst))]
    for i, c in enumerate(bad):
        assert L.nnbvh_intersect_closest_candidates_device(agg._h, p(d_rays), n, p(d_hits), ctypes.byref(c),
                                                           stream) == ERR_ARG
        if i < 3:
            assert L.nnbvh_intersect_any_candidates_device(agg._h, p(d_rays), n, p(d_occ), ctypes.byref(c),
                                                           stream) == ERR_ARG
    torch.cuda.synchronize(dev)
    assert (d_cnt.cpu().numpy() == 77).all()
    agg.close()


@pytest.mark.gpu
def test_cpp_adapter_candidate_overloads(nnbvh_lib):
    src = os.path.join(ROOT, "tests", "cpp", "host_candidates_check.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "host_candidates_check")
    libdir = os.path.join(ROOT, "nn_bvh_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    src, "-o", exe, "-pthread", "-L", libdir, "-l:libnnbvh_hip.so", f"-Wl,-rpath,{libdir}",
                    "-Wl,-rpath-link,/opt/rocm/lib"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "host candidates ok" in out.stdout
