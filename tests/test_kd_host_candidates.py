"""Host-only primitives as candidates on kd-tree scenes (include/nnbvh.h "kd-tree scenes: host-only primitives as
candidates").  CPU: a Python restatement of the kd walk that skips host-only primitives and lists
them, pinned to the oracle; the premise of the GPU tests on the soup they use; the ABI's argument checks.  GPU: the
device's lists, counts and `before` against that walker exactly, the records against the plain kd calls, the resolved
answers against the oracle on the same soup with the host-declared primitives as triangles."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle_binding as ob
import scenes_small as ss
from nn_bvh_amd import _lib, candidates_dtype, resolve_host_candidates, resolve_host_candidates_any, scene
from nn_bvh_amd._lib import HIT_DTYPE, RAY_DTYPE
from nn_bvh_amd.kdtree import KdTreeAggregate, build_kd_tree
from test_host_candidates import assert_resolved_equal, assert_same_but_instance, tri_callback, tri_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 1
KD_CANDIDATE_CALLS = ("nnbvh_kd_intersect_closest_candidates", "nnbvh_kd_intersect_any_candidates",
                      "nnbvh_kd_intersect_closest_candidates_device", "nnbvh_kd_intersect_any_candidates_device",
                      "nnbvh_kd_trace_batches_candidates_device", "nnbvh_kd_wavefront_intersect_closest_items_candidates",
                      "nnbvh_kd_wavefront_intersect_shadow_candidates",
                      "nnbvh_kd_wavefront_intersect_closest_and_shadow_items_candidates")
RAW_CAP = 96  # raw (every reach) host ids kept per ray; the raw COUNT is exact beyond it


# ---- the reference walker -----------------------------------------------------------------------------------
def kd_walk(tree, prims, verts, rays, closest=True):
    """KdTreeAggregate::Intersect / IntersectP (aggregates.cpp:973-1150) over all rays in lockstep, with host-only
    primitives (kind 3) skipped and listed.  Built from the pinned pieces ob.bounds_t0t1 (root interval) and
    ob.leaf_batch (Triangle / BilinearPatch tests); every other operation is the float32 arithmetic of the reference
    line by line.  Kinds 0 (triangle), 1 (bilinear patch) and 3 only.
    Returns a dict: hits (HIT_DTYPE, instance 0 everywhere) or occluded (uint8 0 / 1) with visited / tests; raw_count,
    raw (every reach of a host primitive, in order, the first RAW_CAP ids); count / list (the repeat rule: first
    positions only, never truncated below RAW_CAP); before (closest: len(list) at the accepted hit that stands)."""
    nodes, idx = tree.nodes, tree.prim_indices
    n = len(rays)
    o, d = rays["o"].astype(np.float32), rays["d"].astype(np.float32)
    ray_tmax = rays["tmax"].astype(np.float32).copy()
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = (np.float32(1) / d).astype(np.float32)
    inside, t01 = ob.bounds_t0t1(np.tile(np.asarray(tree.bounds, np.float32), (n, 1)), o, d, ray_tmax)
    t_min, t_max = t01[:, 0].copy(), t01[:, 1].copy()
    cur = np.where(inside != 0, 0, -1).astype(np.int64)  # node index; -1 finished
    leaf_left = np.zeros(n, np.int64)   # > 0: inside a leaf, primitives still to test
    leaf_pos = np.zeros(n, np.int64)    # where the next index sits (primitiveIndices) or the one primitive's id
    leaf_one = np.zeros(n, bool)
    stack = np.zeros((n, 64, 3), np.float32)
    stack_node = np.zeros((n, 64), np.int64)
    sp = np.zeros(n, np.int64)
    hits = np.zeros(n, HIT_DTYPE)
    hits["prim"], hits["t"] = -1, ray_tmax
    visited, tests = np.zeros(n, np.int32), np.zeros(n, np.int32)
    found = np.zeros(n, bool)
    raw_count, count, before = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    raw = np.full((n, RAW_CAP), -1, np.int32)
    lst = np.full((n, RAW_CAP), -1, np.int32)
    kind, pid, pv = prims["kind"], prims["id"], prims["v"]
    flags, word = nodes["flags"].astype(np.int64), nodes["split_or_index"]
    split = word.view(np.float32)

    def pop(r):
        has = sp[r] > 0
        a, b = r[has], r[~has]
        sp[a] -= 1
        cur[a] = stack_node[a, sp[a]]
        t_min[a], t_max[a] = stack[a, sp[a], 0], stack[a, sp[a], 1]
        cur[b] = -1

    while True:
        act = np.nonzero(cur >= 0)[0]
        if len(act) == 0:
            break
        in_leaf = leaf_left[act] > 0
        # ---- one primitive of the leaf
        r = act[in_leaf]
        if len(r):
            p = np.where(leaf_one[r], leaf_pos[r], idx[np.minimum(leaf_pos[r], max(len(idx) - 1, 0))] if len(idx) else 0)
            k = kind[p]
            h = r[k == 3]
            if len(h):
                hid = pid[p[k == 3]]
                rc = raw_count[h]
                keep = rc < RAW_CAP
                raw[h[keep], rc[keep]] = hid[keep]
                raw_count[h] += 1
                new = ~(lst[h] == hid[:, None]).any(1)
                assert (count[h[new]] < RAW_CAP).all()
                lst[h[new], count[h[new]]] = hid[new]
                count[h[new]] += 1
            for code, mode, nv in ((0, "tri", 3), (1, "blp", 4)):
                m = k == code
                if not m.any():
                    continue
                rr, pp = r[m], p[m]
                tests[rr] += 1
                rec = np.concatenate([o[rr], d[rr], ray_tmax[rr, None], verts[pv[pp, :nv]].reshape(len(rr), 3 * nv)], 1)
                hit, out = ob.leaf_batch(mode, rec)
                w, ow = rr[hit != 0], out[hit != 0]
                if closest:
                    hits["prim"][w] = pid[pp[hit != 0]]
                    hits["b0"][w], hits["b1"][w] = ow[:, 0], ow[:, 1]
                    hits["b2"][w] = ow[:, 2] if mode == "tri" else 0
                    hits["t"][w] = ray_tmax[w] = ow[:, -1]
                    before[w] = count[w]
                else:
                    found[w] = True
            assert np.isin(k, (0, 1, 3)).all()
            leaf_left[r] -= 1
            leaf_pos[r] += 1
            done = r[found[r]]
            cur[done], leaf_left[done] = -1, 0
            fin = r[(leaf_left[r] == 0) & ~found[r]]
            pop(fin)
        # ---- one node step
        r = act[~in_leaf]
        if len(r):
            if closest:  # :992 a hit closer than this node
                out = ray_tmax[r] < t_min[r]
                cur[r[out]] = -1
                r = r[~out]
            visited[r] += 1
            c = cur[r]
            f = flags[c]
            leaf = (f & 3) == 3
            a, ca = r[~leaf], c[~leaf]
            if len(a):
                axis = f[~leaf] & 3
                sa = split[ca]
                oa, ia, da = o[a, axis], inv[a, axis], d[a, axis]
                with np.errstate(invalid="ignore", over="ignore"):
                    t_split = ((sa - oa).astype(np.float32) * ia).astype(np.float32)
                below_first = (oa < sa) | ((oa == sa) & (da <= 0))
                above = f[~leaf] >> 2
                first = np.where(below_first, ca + 1, above)
                second = np.where(below_first, above, ca + 1)
                go_first = (t_split > t_max[a]) | (t_split <= 0)
                go_second = ~go_first & (t_split < t_min[a])
                push = ~go_first & ~go_second
                cur[a] = np.where(go_second, second, first)
                q = a[push]
                stack_node[q, sp[q]] = second[push]
                stack[q, sp[q], 0], stack[q, sp[q], 1] = t_split[push], t_max[q]
                sp[q] += 1
                t_max[q] = t_split[push]
            b, cb = r[leaf], c[leaf]
            if len(b):
                npr = f[leaf] >> 2
                empty = npr == 0
                pop(b[empty])
                e, ce, ne = b[~empty], cb[~empty], npr[~empty]
                leaf_left[e] = ne
                leaf_one[e] = ne == 1
                leaf_pos[e] = word[ce].view(np.int32)
    hits["nodes_visited"], hits["prim_tests"] = visited, tests
    res = {"raw_count": raw_count, "raw": raw, "count": count, "list": lst, "before": before, "visited": visited,
           "tests": tests}
    if closest:
        res["hits"] = hits
    else:
        res["occluded"] = found.astype(np.uint8)
    return res


def walker_cands(w, k=16):
    """The walker's de-duplicated lists as a candidates_dtype(k) array; count -1 where a list is longer than k."""
    c = np.zeros(len(w["count"]), candidates_dtype(k))
    c["count"] = np.where(w["count"] > k, -1, w["count"])
    c["before"] = w["before"]
    c["prim"] = w["list"][:, :k]
    c["instance"] = np.where(c["prim"] >= 0, 0, -1)
    return c


# ---- scenes ---------------------------------------------------------------------------------------------------
class Soup:
    """ss.random_soup(1500, 0, seed) with every 7th triangle host-only (kind 3, its exact bounds as prim_bounds), the
    kd-tree over it and over the all-triangle soup, and the rays of the GPU tests: 18 000 with infinite and 6 000 with
    finite tmax, as tests/test_host_candidates.py mixes them.  Both bounds of test_soup_keeps_the_gpu_tests_honest hold
    for these sizes."""

    def __init__(self, seed, max_prims, n_patches=0):
        self.verts, self.prims = ss.random_soup(1500, n_patches, seed)
        tri = self.prims["kind"] == 0
        self.host = tri & (np.arange(len(self.prims)) % 7 == 3)
        v = self.verts[self.prims["v"][:, :3]]
        self.bounds = np.concatenate([v.min(1), v.max(1)], 1).astype(np.float32)
        self.hp = self.prims.copy()
        self.hp["kind"][self.host] = 3
        self.tree_h = build_kd_tree(self.hp, self.verts, prim_bounds=self.bounds, max_prims=max_prims)
        self.tree_t = build_kd_tree(self.prims, self.verts, max_prims=max_prims)
        lo, hi = self.verts.min(0), self.verts.max(0)
        self.rays = np.concatenate([scene.random_rays(18000, lo, hi, seed + 3),
                                    scene.random_rays(6000, lo, hi, seed + 4, tmax=np.float32(0.6))])

    def aggregate(self):
        return KdTreeAggregate.from_tree(self.tree_h.nodes, self.tree_h.prim_indices, self.hp, self.verts, self.tree_h.bounds)

    def callback(self, rays=None):
        return tri_callback(self.rays if rays is None else rays, self.verts, tri_table(self.prims))


_SOUPS, _WALKS = {}, {}


def soup(seed, max_prims, n_patches=0):
    key = (seed, max_prims, n_patches)
    if key not in _SOUPS:
        _SOUPS[key] = Soup(*key)
    return _SOUPS[key]


def walk(s, closest):
    key = (id(s), closest)
    if key not in _WALKS:
        _WALKS[key] = kd_walk(s.tree_h, s.hp, s.verts, s.rays, closest)
    return _WALKS[key]


class OpaqueAttrScene:
    """The scene of the ATTR kernel twin that the walker can restate: triangles of kinds 0 / 4 .. 7 and bilinear patches
    of kinds 1 / 8 .. 15 (tests/test_alpha.py alpha_patch_scene, half of the alpha triangles smooth) with alpha = 1 on
    every primitive.  The per-vertex normals, uvs and per-primitive alpha are handed over, so the scene runs the
    attribute-reading instance, and an alpha of 1 accepts every hit (cpu/primitive.cpp:57-58), so the walk is the
    plain one: the walker sees kinds 0 / 1.  Every 5th triangle (of any triangle kind) is host-only with its exact
    bounds; `prims` is the twin with them on the device."""

    def __init__(self):
        from test_alpha import alpha_patch_scene, patch_uvs
        verts, prims, normals, _, kinds = alpha_patch_scene(43, 1500, 700)
        rng = np.random.default_rng(4)
        prims = prims.copy()
        smooth = ((kinds == 4) | (kinds == 5)) & (rng.random(len(prims)) < 0.5)
        prims["kind"] = np.where(smooth, kinds + 2, kinds)
        one = np.ones(len(prims), np.float32)
        tri = np.isin(prims["kind"], (0, 4, 5, 6, 7))
        prims["v"][tri & (prims["kind"] != 0), 3] = one[:1].view(np.int32)[0]
        self.verts, self.prims, self.normals, self.uvs, self.alpha = verts, prims, normals, patch_uvs(verts), one
        self.host = tri & (np.cumsum(tri) % 5 == 2)
        self.hp = prims.copy()
        self.hp["kind"][self.host] = 3
        v = verts[prims["v"][:, :3]]
        pb = np.concatenate([v.min(1), v.max(1)], 1).astype(np.float32)
        self.tree_h = build_kd_tree(self.hp, verts, prim_bounds=pb, max_prims=2)
        self.tree_t = build_kd_tree(prims, verts, max_prims=2)
        self.walk_prims = self.hp.copy()  # what the walker tests: the same primitives as plain triangles / patches
        self.walk_prims["kind"] = np.where(self.hp["kind"] == 3, 3, np.where(tri, 0, 1))
        self.rays = np.concatenate([scene.random_rays(12000, verts.min(0), verts.max(0), 21),
                                    scene.random_rays(4000, verts.min(0), verts.max(0), 22, tmax=np.float32(0.6))])
        self._walks = {}

    def walk(self, closest):
        if closest not in self._walks:
            self._walks[closest] = kd_walk(self.tree_h, self.walk_prims, self.verts, self.rays, closest)
        return self._walks[closest]

    def oracle(self, fn, tree, prims):
        try:
            ob.set_vertex_normals(self.normals)
            ob.set_vertex_uvs(self.uvs)
            ob.set_prim_alpha(self.alpha)
            return fn(tree.nodes, tree.prim_indices, prims, self.verts, tree.bounds, self.rays, 4)
        finally:
            ob.set_vertex_normals(None)
            ob.set_vertex_uvs(None)
            ob.set_prim_alpha(None)


_OPAQUE = []


def opaque_attr_scene():
    if not _OPAQUE:
        _OPAQUE.append(OpaqueAttrScene())
    return _OPAQUE[0]


def box_scene():
    """The soup with one host-declared box of about half the scene's extent in its middle: it sits in many leaves."""
    verts, prims = ss.random_soup(1500, 0, 5)
    lo, hi = verts.min(0), verts.max(0)
    box = np.zeros(1, prims.dtype)
    box["kind"], box["id"] = 3, len(prims)
    allp = np.concatenate([prims, box])
    v = verts[prims["v"][:, :3]]
    mid, half = (lo + hi) / 2, (hi - lo) / 4
    pb = np.concatenate([np.concatenate([v.min(1), v.max(1)], 1), np.concatenate([mid - half, mid + half])[None]]).astype(np.float32)
    tree = build_kd_tree(allp, verts, prim_bounds=pb)
    rays = scene.random_rays(8000, lo, hi, 6)
    return verts, allp, tree, rays


# ---- CPU ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_prims", [1, 4])
def test_walker_equals_the_oracle_on_the_host_declared_soup(max_prims):
    s = soup(0, max_prims)
    w = walk(s, True)
    exp = ob.kd_closest(s.tree_h.nodes, s.tree_h.prim_indices, s.hp, s.verts, s.tree_h.bounds, s.rays, 4)
    for f in ("prim", "t", "b0", "b1", "b2", "nodes_visited", "prim_tests"):
        assert np.array_equal(w["hits"][f].view(np.uint32), exp[f].view(np.uint32)), f
    assert np.array_equal(exp["instance"] == -1, w["raw_count"] > 0)
    a = walk(s, False)
    eo, ev, et = ob.kd_any_hit(s.tree_h.nodes, s.tree_h.prim_indices, s.hp, s.verts, s.tree_h.bounds, s.rays, 4)
    assert np.array_equal(a["visited"], ev) and np.array_equal(a["tests"], et)
    assert np.array_equal(eo == 1, a["occluded"] == 1)
    assert np.array_equal(eo == 2, (a["occluded"] == 0) & (a["raw_count"] > 0))
    assert (w["raw_count"] >= w["count"]).all() and (w["raw_count"] > w["count"]).any()


@pytest.mark.parametrize("max_prims", [1, 4])
def test_walker_with_patches_equals_the_oracle(max_prims):
    s = soup(2, max_prims, 300)
    w = walk(s, True)
    exp = ob.kd_closest(s.tree_h.nodes, s.tree_h.prim_indices, s.hp, s.verts, s.tree_h.bounds, s.rays, 4)
    for f in ("prim", "t", "b0", "b1", "b2", "nodes_visited", "prim_tests"):
        assert np.array_equal(w["hits"][f].view(np.uint32), exp[f].view(np.uint32)), f
    assert np.array_equal(exp["instance"] == -1, w["raw_count"] > 0)


def test_walker_equals_the_oracle_on_the_opaque_attribute_scene():
    """The oracle walks the real kinds (4 .. 15 with alpha 1), the walker the same primitives as kinds 0 / 1."""
    s = opaque_attr_scene()
    assert s.tree_h.nodes.tobytes() == s.tree_t.nodes.tobytes()
    assert s.tree_h.prim_indices.tobytes() == s.tree_t.prim_indices.tobytes()
    assert len(np.unique(s.hp["kind"])) >= 12 and s.host.sum() > 200
    w = s.walk(True)
    exp = s.oracle(ob.kd_closest, s.tree_h, s.hp)
    for f in ("prim", "t", "b0", "b1", "b2", "nodes_visited", "prim_tests"):
        assert np.array_equal(w["hits"][f].view(np.uint32), exp[f].view(np.uint32)), f
    assert np.array_equal(exp["instance"] == -1, w["raw_count"] > 0)
    a = s.walk(False)
    eo, ev, et = s.oracle(ob.kd_any_hit, s.tree_h, s.hp)
    assert np.array_equal(a["visited"], ev) and np.array_equal(a["tests"], et)
    assert np.array_equal(eo == 1, a["occluded"] == 1)
    assert np.array_equal(eo == 2, (a["occluded"] == 0) & (a["raw_count"] > 0))
    assert (w["count"] > 16).mean() <= 0.01 and (w["count"] > 0).mean() > 0.05


@pytest.mark.parametrize("max_prims", [1, 4])
def test_soup_keeps_the_gpu_tests_honest(max_prims):
    """The premise of the GPU tests: the tree does not change when triangles are declared host-only, the walker's lists
    resolve to the oracle on the all-triangle tree, at most 1 % of the lists are longer than 16 and more than 5 % of
    the rays have a candidate."""
    s = soup(0, max_prims)
    assert s.tree_h.nodes.tobytes() == s.tree_t.nodes.tobytes()
    assert s.tree_h.prim_indices.tobytes() == s.tree_t.prim_indices.tobytes()
    w = walk(s, True)
    assert (w["count"] > 16).mean() <= 0.01 and (w["count"] > 0).mean() > 0.05
    kind = np.zeros(len(s.prims), np.int32)
    cands = walker_cands(w)
    res = resolve_host_candidates(s.rays, w["hits"], cands, s.callback(), kind=kind)
    exp = ob.kd_closest(s.tree_t.nodes, s.tree_t.prim_indices, s.prims, s.verts, s.tree_t.bounds, s.rays, 4)
    ok = cands["count"] >= 0
    assert_resolved_equal(res[ok], exp[ok], "walker closest")
    a = walk(s, False)
    acands = walker_cands(a)
    occ = np.where(a["occluded"] == 1, 1, np.where(a["count"] != 0, 2, 0)).astype(np.uint8)
    got = resolve_host_candidates_any(s.rays, occ, acands, s.callback())
    eocc = ob.kd_any_hit(s.tree_t.nodes, s.tree_t.prim_indices, s.prims, s.verts, s.tree_t.bounds, s.rays, 4)[0]
    settled = got != 2
    assert settled.mean() > 0.99 and np.array_equal(got[settled], eocc[settled])


def test_a_large_host_box_exercises_the_repeat_rule():
    verts, allp, tree, rays = box_scene()
    w = kd_walk(tree, allp, verts, rays, True)
    assert (w["raw_count"] > 16).sum() > 50
    assert w["count"].max() == 1 and ((w["raw_count"] > 16) & (w["count"] == 1)).sum() > 50


C_PROBE = r"""
#include <stdio.h>
#include "nnbvh.h"
int main(void) {
    int32_t count[1], before[1], prim[4], inst[4];
    nnbvh_host_candidates c = {4, count, before, prim, inst};
    nnbvh_ray r = {{0, 0, 0}, 1.0f, {0, 0, 1}, 0.0f};
    nnbvh_hit h;
    uint8_t occ;
    nnbvh_batch b = {NNBVH_BATCH_CLOSEST, 0, &r, 1, &h, NULL, NULL};
    printf("%d %d %d %d %d\n", nnbvh_kd_intersect_closest_candidates(NULL, &r, 1, &h, &c),
           nnbvh_kd_intersect_any_candidates(NULL, &r, 1, &occ, &c),
           nnbvh_kd_intersect_closest_candidates_device(NULL, &r, 1, &h, &c, NULL),
           nnbvh_kd_intersect_any_candidates_device(NULL, &r, 1, &occ, &c, NULL),
           nnbvh_kd_trace_batches_candidates_device(NULL, &b, 1, &c, NULL));
    return 0;
}
"""


def test_kd_candidate_abi_exports_and_compiles_as_c11(nnbvh_lib, tmp_path):
    for s in KD_CANDIDATE_CALLS:
        assert s in _lib.EXPORTS and hasattr(nnbvh_lib, s), s
        assert getattr(nnbvh_lib, s).argtypes == getattr(nnbvh_lib, s.replace("nnbvh_kd_", "nnbvh_")).argtypes, s
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(C_PROBE)
    libdir = os.path.join(ROOT, "nn_bvh_amd")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(exe), "-L", libdir, "-l:libnnbvh_hip.so", f"-Wl,-rpath,{libdir}",
                    "-Wl,-rpath-link,/opt/rocm/lib"], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.split() == [str(ERR_ARG)] * 5


def test_kd_candidate_calls_reject_bad_arguments_before_any_device_work(nnbvh_lib):
    L = nnbvh_lib
    fake = ctypes.c_void_p(8)  # a non-NULL "scene" that must never be dereferenced: the checks below come first
    p = _lib.ptr
    rays, hits, occ = np.zeros(16, RAY_DTYPE), np.zeros(16, HIT_DTYPE), np.zeros(16, np.uint8)
    cnt, bef, pr, ins = (np.zeros(16 * 16, np.int32) for _ in range(4))
    a = lambda x: x.ctypes.data  # noqa: E731
    good = _lib.HostCandidates(8, a(cnt), a(bef), a(pr), a(ins))
    faults = {"capacity 17": _lib.HostCandidates(17, a(cnt), a(bef), a(pr), a(ins)),
              "capacity -1": _lib.HostCandidates(-1, a(cnt), a(bef), a(pr), a(ins)),
              "no count": _lib.HostCandidates(8, None, a(bef), a(pr), a(ins)),
              "no prim": _lib.HostCandidates(8, a(cnt), a(bef), None, a(ins)),
              "no instance": _lib.HostCandidates(8, a(cnt), a(bef), a(pr), None),
              "no before": _lib.HostCandidates(8, a(cnt), None, a(pr), a(ins))}

    def flat(scene_h, c, n=16):
        return [("kd_intersect_closest_candidates", True, lambda: L.nnbvh_kd_intersect_closest_candidates(scene_h, p(rays), n, p(hits), ctypes.byref(c))),
                ("kd_intersect_any_candidates", False, lambda: L.nnbvh_kd_intersect_any_candidates(scene_h, p(rays), n, p(occ), ctypes.byref(c))),
                ("kd_intersect_closest_candidates_device", True, lambda: L.nnbvh_kd_intersect_closest_candidates_device(scene_h, p(rays), n, p(hits), ctypes.byref(c), None)),
                ("kd_intersect_any_candidates_device", False, lambda: L.nnbvh_kd_intersect_any_candidates_device(scene_h, p(rays), n, p(occ), ctypes.byref(c), None))]

    def batches(scene_h, c, kind=0, n=16, counts=False):
        b = np.zeros(2, _lib.BATCH_DTYPE)
        b["kind"], b["n"], b["d_rays"], b["d_out"] = [0, kind], [8, n], 64, 64
        if counts:
            b["d_nodes_visited"][1] = 64
        cs = (_lib.HostCandidates * 2)(good, c)
        return L.nnbvh_kd_trace_batches_candidates_device(scene_h, p(b), 2, cs, None)

    def queues(scene_h, c, sc, max_rays=8, max_shadow=8):
        rec = np.zeros(1, _lib.RAY_SOA_DTYPE)
        buf = np.zeros((6, 16), np.float32)
        for k, name in enumerate(("ox", "oy", "oz", "dx", "dy", "dz")):
            rec[name] = buf[k].ctypes.data
        qrec, irec = np.zeros(1, _lib.CLOSEST_QUEUES_DTYPE), np.zeros(1, _lib.CLOSEST_ITEMS_DTYPE)
        f, px = np.zeros((16, 4), np.float32), np.zeros(16, np.int32)
        mesh = ctypes.c_void_p(1)
        shadow = (max_shadow, p(rec), None, p(f), p(f), p(f), p(px), p(f), 16, p(occ))
        keep = (rec, buf, qrec, irec, f, px)
        return keep, [
            ("kd_wavefront_intersect_closest_items_candidates", lambda: L.nnbvh_kd_wavefront_intersect_closest_items_candidates(
                scene_h, mesh, max_rays, p(rec), None, None, 0, p(hits), p(qrec), p(irec), ctypes.byref(c), None)),
            ("kd_wavefront_intersect_shadow_candidates", lambda: L.nnbvh_kd_wavefront_intersect_shadow_candidates(
                scene_h, *shadow, ctypes.byref(sc), None)),
            ("kd_wavefront_intersect_closest_and_shadow_items_candidates", lambda: L.nnbvh_kd_wavefront_intersect_closest_and_shadow_items_candidates(
                scene_h, mesh, max_rays, p(rec), None, None, 0, p(hits), p(qrec), p(irec), ctypes.byref(c), *shadow, ctypes.byref(sc), None))]

    # a NULL scene: every call, under its own name
    for name, _, call in flat(None, good):
        assert call() == ERR_ARG and name in _lib.last_error(), name
    assert batches(None, good) == ERR_ARG and "kd_trace_batches_candidates_device" in _lib.last_error()
    keep, calls = queues(None, good, good)
    for name, call in calls:
        assert call() == ERR_ARG and name in _lib.last_error(), name
    # the candidate-argument faults, on a scene that would crash if it were looked at
    for what, c in faults.items():
        for name, closest, call in flat(fake, c):
            if what == "no before" and not closest:
                continue  # before is not an output of any hit
            assert call() == ERR_ARG and name in _lib.last_error(), (what, name)
        assert batches(fake, c) == ERR_ARG and "kd_trace_batches_candidates_device" in _lib.last_error(), what
        keep, calls = queues(fake, c, good)
        assert calls[0][1]() == ERR_ARG and calls[0][0] in _lib.last_error(), what
        assert calls[2][1]() == ERR_ARG and calls[2][0] in _lib.last_error(), what
        if what != "no before":
            keep, calls = queues(fake, good, c)
            assert calls[1][1]() == ERR_ARG and calls[1][0] in _lib.last_error(), what
            assert calls[2][1]() == ERR_ARG and calls[2][0] in _lib.last_error(), what
    # capacity 0 is a plain batch only in the batches call
    zero = _lib.HostCandidates(0, None, None, None, None)
    for name, _, call in flat(fake, zero):
        assert call() == ERR_ARG, name
    # an any-hit batch with exact counts and candidates; batches and queues of 2^28 rays or more
    assert batches(fake, good, kind=1, counts=True) == ERR_ARG and "not both" in _lib.last_error()
    assert batches(fake, good, n=1 << 28) == ERR_ARG
    for name, _, call in flat(fake, good, n=1 << 28):
        assert call() == ERR_ARG and name in _lib.last_error(), name
    for mr, ms in ((1 << 28, 8), (8, 1 << 28), (-1, 8), (8, -1)):
        keep, calls = queues(fake, good, good, mr, ms)
        for k, (name, call) in enumerate(calls):
            if (k == 0 and mr == 8) or (k == 1 and ms == 8):
                continue  # the call has no such argument
            assert call() == ERR_ARG and name in _lib.last_error(), (name, mr, ms)
    # a NULL candidates array
    b = np.zeros(1, _lib.BATCH_DTYPE)
    b["n"], b["d_rays"], b["d_out"] = 8, 64, 64
    assert L.nnbvh_kd_trace_batches_candidates_device(fake, p(b), 1, None, None) == ERR_ARG


def test_wavefront_aggregate_binds_the_kd_candidate_calls(monkeypatch):
    """The three *WithCandidates methods of a WavefrontAggregate over a scene-less KdTreeAggregate reach the kd entry
    points: the library refuses the NULL scene under the kd call's own name (no device is touched before that check,
    so host tensors stand in for the queues).  IntersectShadowTr / IntersectOneRandom stay refused by the class."""
    torch = pytest.importorskip("torch")
    import types
    from nn_bvh_amd import NNBVHError
    from nn_bvh_amd.wavefront import HostCandidateArrays, RayQueue, WavefrontAggregate, WorkQueue
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: types.SimpleNamespace(cuda_stream=0))
    wf = WavefrontAggregate(KdTreeAggregate(None, np.zeros(6, np.float32)))
    n = 8
    rays = np.zeros(n, RAY_DTYPE)
    rq, sq = RayQueue.from_records(rays, "cpu"), RayQueue.from_records(rays, "cpu", shadow=True)
    c, sc = HostCandidateArrays(n, 4, "cpu"), HostCandidateArrays(n, 4, "cpu")
    hits, occ = torch.zeros((n, 32), dtype=torch.uint8), torch.zeros(n, dtype=torch.uint8)
    f4, px = torch.zeros((n, 4), dtype=torch.float32), torch.zeros(n, dtype=torch.int32)
    mesh = types.SimpleNamespace(_h=None)
    nh = WorkQueue(n, "cpu")
    calls = {
        "intersect_closest_items_candidates":
            lambda: wf.IntersectClosestItemsWithCandidates(n, rq, mesh, c, hits, needs_host=nh),
        "intersect_shadow_candidates":
            lambda: wf.IntersectShadowWithCandidates(n, sq, f4, f4, f4, px, f4.clone(), occ, sc),
        "intersect_closest_and_shadow_items_candidates":
            lambda: wf.IntersectClosestAndShadowItemsWithCandidates(n, rq, mesh, c, hits, n, sq, f4, f4, f4, px, f4.clone(),
                                                                    occ, sc, needs_host=nh)}
    for call, run in calls.items():
        assert wf._name(call) == "nnbvh_kd_wavefront_" + call
        with pytest.raises(NNBVHError) as err:
            run()
        assert "status 1" in str(err.value) and "kd_wavefront_" + call in str(err.value), str(err.value)
        assert "not offered" not in str(err.value)
    with pytest.raises(NNBVHError, match="not offered for kd-tree"):
        wf.IntersectShadowTr(0, None, None, None, None, None, None, None)
    with pytest.raises(NNBVHError, match="not offered for kd-tree"):
        wf.IntersectOneRandom(0, None, None, None, None)


# ---- GPU ------------------------------------------------------------------------------------------------------
def _dev():
    import torch
    return torch.device("cuda", 0)


def _stream():
    import torch
    return torch.cuda.current_stream(_dev()).cuda_stream


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(_dev())


class DevCands:
    """Device arrays of one batch's nnbvh_host_candidates, with sentinels where the kernel must not write."""

    def __init__(self, n, k):
        import torch
        self.n, self.k = n, max(k, 1)
        self.count = torch.full((max(n, 1),), 77, dtype=torch.int32, device=_dev())
        self.before = torch.full((max(n, 1),), 77, dtype=torch.int32, device=_dev())
        self.prim = torch.full((max(n, 1) * self.k,), -1, dtype=torch.int32, device=_dev())
        self.inst = torch.full((max(n, 1) * self.k,), -1, dtype=torch.int32, device=_dev())

    def tuple(self, k, closest):
        return (k, self.count.data_ptr(), self.before.data_ptr() if closest else None, self.prim.data_ptr(),
                self.inst.data_ptr())

    def numpy(self):
        c = np.zeros(self.n, candidates_dtype(self.k))
        c["count"], c["before"] = self.count.cpu().numpy()[:self.n], self.before.cpu().numpy()[:self.n]
        c["prim"] = self.prim.cpu().numpy().reshape(-1, self.k)[:self.n]
        c["instance"] = self.inst.cpu().numpy().reshape(-1, self.k)[:self.n]
        return c


def assert_lists_equal(got, exp, closest=True, where=None):
    """count, before and the entries below count; instance 0 in every entry."""
    m = np.ones(len(exp), bool) if where is None else where
    assert np.array_equal(got["count"][m], exp["count"][m])
    if closest:  # (a void ray's `before` says nothing: the list it counts into was given up)
        settled = m & (exp["count"] >= 0)
        assert np.array_equal(got["before"][settled], exp["before"][settled])
    k = got["prim"].shape[1]
    j = (np.arange(k)[None, :] < np.maximum(exp["count"], 0)[:, None]) & m[:, None]
    assert np.array_equal(got["prim"][j], exp["prim"][:, :k][j])
    assert (got["instance"][j] == 0).all()
    # (an overflowed ray's K entries were written before it was given up)
    assert (got["prim"][~j & (m & (exp["count"] >= 0))[:, None]] == -1).all(), "entries beyond count were written"


@pytest.mark.gpu
@pytest.mark.parametrize("max_prims", [1, 4])
def test_gpu_closest_lists_records_and_resolved_hits(max_prims):
    s = soup(0, max_prims)
    w = walk(s, True)
    agg = s.aggregate()
    hits, cands = agg.intersect_with_host_candidates(s.rays, capacity=16)
    plain = agg.Intersect(s.rays)
    agg.close()
    assert_lists_equal(cands, walker_cands(w))
    assert_same_but_instance(hits, plain)
    assert hits[cands["count"] >= 0].tobytes() == w["hits"][cands["count"] >= 0].tobytes()
    assert np.array_equal(plain["instance"] == -1, cands["count"] != 0)
    assert np.array_equal(hits["instance"], np.where(cands["count"] < 0, -1, 0))
    cb = s.callback()
    res = resolve_host_candidates(s.rays, hits, cands, cb, kind=np.zeros(len(s.prims), np.int32))
    exp = ob.kd_closest(s.tree_t.nodes, s.tree_t.prim_indices, s.prims, s.verts, s.tree_t.bounds, s.rays, 4)
    ok = cands["count"] >= 0
    assert ok.mean() >= 0.99
    assert_resolved_equal(res[ok], exp[ok], "kd closest")
    assert ((res["prim"] >= 0) & s.host[np.maximum(res["prim"], 0)])[ok].sum() > 50
    two = np.nonzero((cands["before"] > 0) & (hits["prim"] >= 0) & ok)[0]  # step 3 of the merge rule
    assert cb(two, cands["prim"][two, 0], cands["instance"][two, 0], s.rays["tmax"][two])[0].sum() > 5


@pytest.mark.gpu
@pytest.mark.parametrize("max_prims", [1, 4])
def test_gpu_any_hit_lists_flags_and_resolved_flags(max_prims):
    s = soup(0, max_prims)
    a = walk(s, False)
    agg = s.aggregate()
    occ, cands = agg.intersect_p_with_host_candidates(s.rays, capacity=16)
    plain = agg.IntersectP(s.rays)
    agg.close()
    assert_lists_equal(cands, walker_cands(a), closest=False)
    assert (cands["before"] == 0).all()
    assert np.array_equal(occ, plain)
    assert np.array_equal(occ == 1, a["occluded"] == 1)
    assert np.array_equal(occ == 2, (cands["count"] != 0) & (occ != 1)) and (occ == 2).sum() > 300
    got = resolve_host_candidates_any(s.rays, occ, cands, s.callback())
    eocc = ob.kd_any_hit(s.tree_t.nodes, s.tree_t.prim_indices, s.prims, s.verts, s.tree_t.bounds, s.rays, 4)[0]
    settled = got != 2
    assert np.array_equal(~settled, (occ == 2) & (cands["count"] < 0))
    assert np.array_equal(got[settled], eocc[settled])
    assert ((occ == 2) & (got == 1)).sum() > 50 and ((occ == 2) & (got == 0)).sum() > 50


@pytest.mark.gpu
def test_gpu_patch_instance_lists_and_resolved_hits():
    """The PATCH twin: a soup with bilinear patches, every 7th triangle host-only."""
    s = soup(2, 4, 300)
    w, a = walk(s, True), walk(s, False)
    agg = s.aggregate()
    hits, cands = agg.intersect_with_host_candidates(s.rays, capacity=16)
    occ, acands = agg.intersect_p_with_host_candidates(s.rays, capacity=16)
    plain = agg.Intersect(s.rays)
    agg.close()
    assert_lists_equal(cands, walker_cands(w))
    assert_lists_equal(acands, walker_cands(a), closest=False)
    assert_same_but_instance(hits, plain)
    assert np.array_equal(plain["instance"] == -1, cands["count"] != 0) and (cands["count"] > 0).mean() > 0.03
    res = resolve_host_candidates(s.rays, hits, cands, s.callback(), kind=s.prims["kind"])
    exp = ob.kd_closest(s.tree_t.nodes, s.tree_t.prim_indices, s.prims, s.verts, s.tree_t.bounds, s.rays, 4)
    ok = cands["count"] >= 0
    assert_resolved_equal(res[ok], exp[ok], "kd closest, patches")
    assert (s.prims["kind"][np.maximum(res["prim"], 0)][res["prim"] >= 0] == 1).sum() > 100


@pytest.mark.gpu
def test_gpu_attribute_instance_and_alpha_retrace_voids():
    """The ATTR twin (nnbvh_kd_scene_create_with_attributes): attribute-reading alpha kinds with every 7th plain
    triangle host-only.  Records equal the plain call's but for instance, and the rays resolve to the oracle on the
    scene with those triangles on the device.  Ordinary rays never void by a re-trace here (three re-traces are enough
    for a surface a line meets twice at most), so a family of degenerate rays (NaN / inf / zero components, the rays
    of tests/test_alpha.py) follows: on them an alpha re-trace voids, and count is -2 as the oracle's void record
    says."""
    from test_alpha import alpha_patch_scene, patch_uvs
    verts, prims, normals, alpha, kinds = alpha_patch_scene(43, 1500, 2500)
    rng = np.random.default_rng(4)
    prims = prims.copy()
    smooth = ((kinds == 4) | (kinds == 5)) & (rng.random(len(prims)) < 0.5)
    prims["kind"] = np.where(smooth, kinds + 2, kinds)
    uvs = patch_uvs(verts)
    host = (prims["kind"] == 0) & (np.cumsum(prims["kind"] == 0) % 7 == 3)
    assert host.sum() > 20
    hp = prims.copy()
    hp["kind"][host] = 3
    v = verts[prims["v"][:, :3]]
    pb = np.concatenate([v.min(1), v.max(1)], 1).astype(np.float32)
    tree = build_kd_tree(hp, verts, prim_bounds=pb, max_prims=2)
    tree_t = build_kd_tree(prims, verts, max_prims=2)
    assert tree.nodes.tobytes() == tree_t.nodes.tobytes()
    rays = np.concatenate([scene.random_rays(12000, verts.min(0) - 1, verts.max(0) + 1, 21),
                           scene.random_rays(4000, verts.min(0), verts.max(0), 22, tmax=0.6)])
    odd = scene.random_rays(6000, verts.min(0) - 1, verts.max(0) + 1, 11)
    rng = np.random.default_rng(3)
    special = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1e-30], np.float32)
    for f in ("o", "d"):
        x = odd[f].copy()
        m = rng.random(x.shape) < 0.15
        x[m] = rng.choice(special, int(m.sum()))
        odd[f] = x
    agg = KdTreeAggregate.from_tree(tree.nodes, tree.prim_indices, hp, verts, tree.bounds, normals=normals, uvs=uvs,
                                    prim_alpha=alpha)
    hits, cands = agg.intersect_with_host_candidates(rays, capacity=16)
    occ, acands = agg.intersect_p_with_host_candidates(rays, capacity=16)
    plain, plain_occ = agg.Intersect(rays), agg.IntersectP(rays)
    odd_hits, odd_cands = agg.intersect_with_host_candidates(odd, capacity=16)
    odd_plain = agg.Intersect(odd)
    agg.close()
    # the same scene with every primitive on the device: whatever voids is an alpha re-trace
    agg_t = KdTreeAggregate.from_tree(tree_t.nodes, tree_t.prim_indices, prims, verts, tree_t.bounds, normals=normals,
                                      uvs=uvs, prim_alpha=alpha)
    t_hits, t_cands = agg_t.intersect_with_host_candidates(odd, capacity=16)
    t_occ, t_acands = agg_t.intersect_p_with_host_candidates(odd, capacity=16)
    t_plain, t_plain_occ = agg_t.Intersect(odd), agg_t.IntersectP(odd)
    agg_t.close()
    try:
        ob.set_vertex_normals(normals)
        ob.set_vertex_uvs(uvs)
        ob.set_prim_alpha(alpha)
        exp = ob.kd_closest(tree_t.nodes, tree_t.prim_indices, prims, verts, tree_t.bounds, rays, 4)
        exp_h = ob.kd_closest(tree.nodes, tree.prim_indices, hp, verts, tree.bounds, rays, 4)
        odd_exp = ob.kd_closest(tree_t.nodes, tree_t.prim_indices, prims, verts, tree_t.bounds, odd, 4)
    finally:
        ob.set_vertex_normals(None)
        ob.set_vertex_uvs(None)
        ob.set_prim_alpha(None)
    cnt = cands["count"]
    assert_same_but_instance(hits, plain)
    assert plain.tobytes() == exp_h.tobytes()  # the oracle's void records are the plain call's
    assert np.array_equal(plain["instance"] == -1, cnt != 0)
    assert np.array_equal(hits["instance"], np.where(cnt < 0, -1, 0))
    assert (cnt > 0).sum() > 200 and (cnt >= 0).mean() > 0.99
    # the degenerate family: count -2 exactly where the oracle's record is void, the records the oracle's
    void = odd_exp["instance"] == -1
    assert void.sum() > 100
    assert t_hits.tobytes() == t_plain.tobytes()  # (bytes against the device: a NaN's sign is not pinned by the oracle)
    for f in ("prim", "nodes_visited", "prim_tests", "instance"):
        assert np.array_equal(t_hits[f], odd_exp[f]), f
    assert np.array_equal(t_cands["count"], np.where(void, -2, 0)) and (t_cands["before"] == 0).all()
    assert np.array_equal(t_occ, t_plain_occ) and (t_occ == 2).sum() > 0
    assert np.array_equal(t_acands["count"][t_occ != 1] == -2, t_occ[t_occ != 1] == 2)
    assert (t_acands["count"][t_occ == 0] == 0).all()
    # ... and with the host-declared triangles in the scene the void of a re-trace wins over a list
    assert_same_but_instance(odd_hits, odd_plain)
    assert np.array_equal(odd_plain["instance"] == -1, odd_cands["count"] != 0)
    assert (odd_cands["count"] == -2).sum() > 100 and (odd_cands["count"] > 0).sum() > 100
    assert np.array_equal(occ, plain_occ) and np.array_equal(occ == 2, (acands["count"] != 0) & (occ != 1))
    assert (cands["instance"][np.arange(16)[None, :] < np.maximum(cnt, 0)[:, None]] == 0).all()
    res = resolve_host_candidates(rays, hits, cands, tri_callback(rays, verts, tri_table(prims)), kind=prims["kind"])
    ok = (cnt >= 0) & (exp["instance"] != -1)
    assert ((exp["instance"] == -1) <= (cnt == -2)).all()  # the reference's own voids are among the device's
    assert_resolved_equal(res[ok], exp[ok], "kd closest, attributes")
    # ... and the any-hit lists, wherever neither side voids
    try:
        ob.set_vertex_normals(normals)
        ob.set_vertex_uvs(uvs)
        ob.set_prim_alpha(alpha)
        eocc = ob.kd_any_hit(tree_t.nodes, tree_t.prim_indices, prims, verts, tree_t.bounds, rays, 4)[0]
    finally:
        ob.set_vertex_normals(None)
        ob.set_vertex_uvs(None)
        ob.set_prim_alpha(None)
    got = resolve_host_candidates_any(rays, occ, acands, tri_callback(rays, verts, tri_table(prims)))
    settled = (got != 2) & (eocc != 2)
    assert settled.mean() > 0.99 and np.array_equal(got[settled], eocc[settled])
    assert ((occ == 2) & (got == 1)).sum() > 10 and ((occ == 2) & (got == 0)).sum() > 10


@pytest.mark.gpu
def test_gpu_attribute_instance_lists_equal_the_walker():
    """The same check as on the lean and the PATCH twin, on the ATTR twin <2,1,8,O32,1,1>: count, before and the list
    entries equal the walker's exactly, closest and any hit, on the attribute scene whose walk the walker restates
    (OpaqueAttrScene); records, resolved hits, host wins and step 3 of the merge rule as there."""
    s = opaque_attr_scene()
    w, a = s.walk(True), s.walk(False)
    agg = KdTreeAggregate.from_tree(s.tree_h.nodes, s.tree_h.prim_indices, s.hp, s.verts, s.tree_h.bounds,
                                    normals=s.normals, uvs=s.uvs, prim_alpha=s.alpha)
    hits, cands = agg.intersect_with_host_candidates(s.rays, capacity=16)
    occ, acands = agg.intersect_p_with_host_candidates(s.rays, capacity=16)
    plain, plain_occ = agg.Intersect(s.rays), agg.IntersectP(s.rays)
    agg.close()
    assert_lists_equal(cands, walker_cands(w))
    assert_lists_equal(acands, walker_cands(a), closest=False)
    assert (acands["before"] == 0).all()
    ok = cands["count"] >= 0
    assert ok.mean() >= 0.99 and (cands["count"] > 0).mean() > 0.05
    assert_same_but_instance(hits, plain)
    assert hits[ok].tobytes() == w["hits"][ok].tobytes()
    assert np.array_equal(plain["instance"] == -1, cands["count"] != 0)
    assert np.array_equal(hits["instance"], np.where(cands["count"] < 0, -1, 0))
    assert np.array_equal(occ, plain_occ) and np.array_equal(occ == 1, a["occluded"] == 1)
    assert np.array_equal(occ == 2, (acands["count"] != 0) & (occ != 1))
    cb = tri_callback(s.rays, s.verts, tri_table(s.prims))
    res = resolve_host_candidates(s.rays, hits, cands, cb, kind=s.prims["kind"])
    exp = s.oracle(ob.kd_closest, s.tree_t, s.prims)
    assert (exp["instance"] == 0).all()
    assert_resolved_equal(res[ok], exp[ok], "kd closest, opaque attributes")
    assert ((res["prim"] >= 0) & s.host[np.maximum(res["prim"], 0)])[ok].sum() > 50
    two = np.nonzero((cands["before"] > 0) & (hits["prim"] >= 0) & ok)[0]  # step 3 of the merge rule
    assert cb(two, cands["prim"][two, 0], cands["instance"][two, 0], s.rays["tmax"][two])[0].sum() > 5
    hit_kind = s.prims["kind"][np.maximum(res["prim"], 0)][(res["prim"] >= 0) & ok]
    assert (hit_kind >= 8).sum() > 100 and np.isin(hit_kind, (6, 7)).sum() > 50  # the attribute-reading kinds are hit
    got = resolve_host_candidates_any(s.rays, occ, acands, cb)
    eocc = s.oracle(ob.kd_any_hit, s.tree_t, s.prims)[0]
    settled = got != 2
    assert np.array_equal(~settled, (occ == 2) & (acands["count"] < 0))
    assert np.array_equal(got[settled], eocc[settled])
    assert ((occ == 2) & (got == 1)).sum() > 20 and ((occ == 2) & (got == 0)).sum() > 20


@pytest.mark.gpu
def test_gpu_large_host_box_is_listed_once():
    verts, allp, tree, rays = box_scene()
    w = kd_walk(tree, allp, verts, rays, True)
    agg = KdTreeAggregate.from_tree(tree.nodes, tree.prim_indices, allp, verts, tree.bounds)
    hits, cands = agg.intersect_with_host_candidates(rays, capacity=16)
    agg.close()
    assert_lists_equal(cands, walker_cands(w))
    many = w["raw_count"] > 16
    assert many.sum() > 50 and (cands["count"][many] == 1).all() and (cands["prim"][many, 0] == len(allp) - 1).all()
    assert hits.tobytes() == w["hits"].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 2])
def test_gpu_overflow_voids_the_ray_as_today(k):
    s = soup(0, 4)
    w, a = walk(s, True), walk(s, False)
    agg = s.aggregate()
    hits, cands = agg.intersect_with_host_candidates(s.rays, capacity=k)
    occ, acands = agg.intersect_p_with_host_candidates(s.rays, capacity=k)
    plain, plain_occ = agg.Intersect(s.rays), agg.IntersectP(s.rays)
    agg.close()
    over = w["count"] > k
    assert over.sum() > 20
    assert_lists_equal(cands, walker_cands(w, k))
    assert np.array_equal(cands["count"] == -1, over)
    assert hits[over].tobytes() == plain[over].tobytes() and (hits["instance"][over] == -1).all()
    assert_same_but_instance(hits, plain)
    assert_lists_equal(acands, walker_cands(a, k), closest=False, where=occ != 1)
    assert np.array_equal(occ, plain_occ) and ((acands["count"] == -1) & (occ == 2)).sum() > 10


@pytest.mark.gpu
def test_gpu_one_launch_batches_equal_the_single_batch_calls():
    """Four batches in one launch: closest with candidates, any hit with capacity 0 (a plain batch), an empty one, any
    hit with candidates.  (nnbvh_batch carries host sizes only: device-resident sizes are the queue calls', below.)"""
    import torch
    s = soup(0, 4)
    agg = s.aggregate()
    r0, r1, r3 = s.rays[:9000], s.rays[9000:13000], s.rays[12000:24000]
    hits, cands = agg.intersect_with_host_candidates(r0, capacity=8)
    occ3, cands3 = agg.intersect_p_with_host_candidates(r3, capacity=16)
    d = [_t(r0), _t(r1), torch.zeros(32, dtype=torch.uint8, device=_dev()), _t(r3)]
    out = [torch.full((len(r0) * 32,), 0xAB, dtype=torch.uint8, device=_dev()),
           torch.full((len(r1),), 9, dtype=torch.uint8, device=_dev()),
           torch.full((32,), 0xAB, dtype=torch.uint8, device=_dev()),
           torch.full((len(r3),), 9, dtype=torch.uint8, device=_dev())]
    c0, c3 = DevCands(len(r0), 8), DevCands(len(r3), 16)
    batches = [("closest", d[0].data_ptr(), len(r0), out[0].data_ptr()), ("any", d[1].data_ptr(), len(r1), out[1].data_ptr()),
               ("closest", d[2].data_ptr(), 0, out[2].data_ptr()), ("any", d[3].data_ptr(), len(r3), out[3].data_ptr())]
    agg.trace_batches_candidates_device(batches, [c0.tuple(8, True), None, None, c3.tuple(16, False)], _stream())
    plain1 = torch.full((len(r1),), 9, dtype=torch.uint8, device=_dev())
    agg.trace_batches_device([("any", d[1].data_ptr(), len(r1), plain1.data_ptr())], _stream())
    torch.cuda.synchronize()
    assert out[0].cpu().numpy().tobytes() == hits.tobytes()
    g0 = c0.numpy()
    assert_lists_equal(g0, cands)
    assert torch.equal(out[1], plain1) and (plain1 == 2).any()
    assert (out[2] == 0xAB).all()
    assert np.array_equal(out[3].cpu().numpy(), occ3)
    assert_lists_equal(c3.numpy(), cands3, closest=False)
    assert (c3.before == 77).all()  # not an output of any hit
    agg.close()


@pytest.mark.gpu
def test_gpu_deep_tree_spill_path_and_candidate_sites_coexist():
    import collections
    ch = ss.kd_chain(64, 1)
    verts, prims = ch.verts, ch.prims
    tree = collections.namedtuple("Tree", "nodes prim_indices bounds")(ch.nodes, ch.prim_indices, ch.bounds)
    rays = ss.kd_chain_rays(2000, 2)
    hp = prims.copy()
    hp["kind"][np.arange(len(hp)) % 5 == 2] = 3
    for closest in (True, False):
        w = kd_walk(tree, hp, verts, rays, closest)
        agg = KdTreeAggregate.from_tree(tree.nodes, tree.prim_indices, hp, verts, tree.bounds)
        if closest:
            hits, cands = agg.intersect_with_host_candidates(rays, capacity=16)
            ok = cands["count"] >= 0
            assert hits[ok].tobytes() == w["hits"][ok].tobytes() and hits["nodes_visited"].max() > 60
        else:
            occ, cands = agg.intersect_p_with_host_candidates(rays, capacity=16)
            assert np.array_equal(occ == 1, w["occluded"] == 1)
        agg.close()
        assert_lists_equal(cands, walker_cands(w), closest=closest, where=None if closest else occ != 1)
        assert not closest or (cands["count"] > 0).sum() > 10


@pytest.mark.gpu
def test_gpu_device_call_is_hip_graph_capturable():
    import torch
    s = soup(0, 4)
    agg = s.aggregate()
    rays = s.rays[:8000]
    hits, cands = agg.intersect_with_host_candidates(rays, capacity=8)
    n, k = len(rays), 8
    d_rays, d_hits, c = _t(rays), torch.zeros(n * 32, dtype=torch.uint8, device=_dev()), DevCands(n, k)
    side = torch.cuda.Stream(_dev())

    def call():
        agg.intersect_candidates_device(d_rays.data_ptr(), d_hits.data_ptr(), n, k, c.count.data_ptr(),
                                        c.before.data_ptr(), c.prim.data_ptr(), c.inst.data_ptr(), side.cuda_stream)

    with torch.cuda.stream(side):
        call()  # warm-up: creates this stream's workspace (allocation is not capturable)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        call()
    for _ in range(2):
        d_hits.zero_()
        c.count.fill_(77)
        c.before.fill_(77)
        c.prim.fill_(-1)
        torch.cuda.synchronize()
        graph.replay()
        torch.cuda.synchronize()
        assert d_hits.cpu().numpy().tobytes() == hits.tobytes()
        assert_lists_equal(c.numpy(), cands)
    agg.close()


@pytest.mark.gpu
def test_gpu_scene_without_host_primitives_runs_the_plain_kernels():
    s = soup(0, 4)
    agg = KdTreeAggregate.from_tree(s.tree_t.nodes, s.tree_t.prim_indices, s.prims, s.verts, s.tree_t.bounds)
    hits, cands = agg.intersect_with_host_candidates(s.rays)
    occ, acands = agg.intersect_p_with_host_candidates(s.rays)
    assert hits.tobytes() == agg.Intersect(s.rays).tobytes() and np.array_equal(occ, agg.IntersectP(s.rays))
    agg.close()
    assert (cands["count"] == 0).all() and (cands["before"] == 0).all() and (acands["count"] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("pair_one_launch", [0, 1])
def test_gpu_queue_calls_route_resolve_and_record(pair_one_launch):
    """The three queue calls over SOA queues with device-side sizes: rays without candidates are routed and their items
    written as by the plain kd items call, rays with candidates go to needs_host only; after the host resolves them
    and the indexed second enqueue the queues are those of the all-triangle scene, and after the second record_shadow
    pass the radiance is ob.record_shadow's on the all-triangle scene."""
    import torch
    from test_kd_wavefront import QUEUES, _items_by_index, _shadow_rays
    from test_wavefront import shadow_inputs
    from test_wavefront_items import full_items, ray_queue
    from nn_bvh_amd.interaction import ShadingMesh
    from nn_bvh_amd.wavefront import (HostCandidateArrays, RayQueue, WavefrontAggregate, WorkQueue, enqueue_closest_items,
                                      record_shadow)
    s = soup(0, 4)
    dev = _dev()
    n, nq, max_shadow, ns, n_pixels = 7000, 6500, 5000, 4600, 6000
    rays = s.rays[:n].copy()
    rays["tmax"] = np.inf
    srays = _shadow_rays(s.verts, max_shadow, 9)
    srays["time"] = 0
    mesh = ShadingMesh(s.verts, s.prims["v"][:, :3].copy())
    rng = np.random.default_rng(2)
    prim_class = rng.choice(np.array([0, 1, 2, 4, 5, 6], np.uint8), len(s.prims))
    has_medium = (rng.random(n) < 0.15).astype(np.uint8)
    Ld, r_u, r_l, px, L = shadow_inputs(max_shadow, n_pixels, 7)
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731

    def run(agg, candidates, pair):
        agg.set_option("pair_one_launch", pair_one_launch)
        wf = WavefrontAggregate(agg, prim_class)
        rq, sq = ray_queue(rays, dev, has_medium), RayQueue.from_records(srays, dev, shadow=True)
        rq.size.fill_(nq)
        sq.size.fill_(ns)
        o = {"queues": {k: WorkQueue(n, dev) for k in QUEUES}, "items": full_items(n, dev), "nh": WorkQueue(n, dev),
             "hits": torch.full((n, 32), 0xAB, dtype=torch.uint8, device=dev), "L": t(L), "rq": rq, "sq": sq,
             "occ": torch.full((max_shadow,), 9, dtype=torch.uint8, device=dev), "wf": wf,
             "c": HostCandidateArrays(n, 16, dev), "sc": HostCandidateArrays(max_shadow, 16, dev)}
        sh = (max_shadow, sq, t(Ld), t(r_u), t(r_l), t(px), o["L"])
        if candidates and pair:
            wf.IntersectClosestAndShadowItemsWithCandidates(n, rq, mesh, o["c"], o["hits"], *sh, o["occ"], o["sc"],
                                                            items=o["items"], needs_host=o["nh"], **o["queues"])
        elif candidates:
            wf.IntersectShadowWithCandidates(*sh, o["occ"], o["sc"])
            wf.IntersectClosestItemsWithCandidates(n, rq, mesh, o["c"], o["hits"], items=o["items"], needs_host=o["nh"],
                                                   **o["queues"])
        else:
            wf.IntersectClosestAndShadowItems(n, rq, mesh, *sh, items=o["items"], needs_host=o["nh"], hits=o["hits"],
                                              occluded=o["occ"], **o["queues"])
        torch.cuda.synchronize()
        return o

    agg_h = s.aggregate()
    agg_t = KdTreeAggregate.from_tree(s.tree_t.nodes, s.tree_t.prim_indices, s.prims, s.verts, s.tree_t.bounds)
    flat_hits, flat_c = agg_h.intersect_with_host_candidates(rays[:nq], capacity=16)
    flat_occ, flat_sc = agg_h.intersect_p_with_host_candidates(srays[:ns], capacity=16)
    plain_h = run(agg_h, False, True)   # today's call on the host-declared scene: voids go to needs_host
    plain_t = run(agg_t, False, True)   # ... and on the all-triangle scene: the goal
    for pair in (False, True):
        o = run(agg_h, True, pair)
        cands, scands = o["c"].numpy()[:nq], o["sc"].numpy()[:ns]
        hits = o["hits"].cpu().numpy().view(HIT_DTYPE).reshape(-1)
        assert hits[:nq].tobytes() == flat_hits.tobytes() and (o["hits"][nq:] == 0xAB).all()
        assert_lists_equal(cands, flat_c)
        assert np.array_equal(o["occ"].cpu().numpy()[:ns], flat_occ) and (o["occ"][ns:] == 9).all()
        assert_lists_equal(scands, flat_sc, closest=False)
        # rays with candidates: needs_host only; the others: routed and written as by the plain call
        with_c = np.nonzero(cands["count"] != 0)[0]
        assert len(with_c) > 300
        assert np.array_equal(np.sort(o["nh"].indices().cpu().numpy()), np.sort(plain_h["nh"].indices().cpu().numpy()))
        assert np.isin(with_c, o["nh"].indices().cpu().numpy()).all()
        for k in QUEUES:
            assert o["queues"][k].Size() == plain_h["queues"][k].Size(), k
            assert not np.isin(o["queues"][k].indices().cpu().numpy(), with_c).any(), k
            if k in o["items"]:
                a, b = _items_by_index(o["queues"][k], o["items"][k]), _items_by_index(plain_h["queues"][k], plain_h["items"][k])
                assert np.array_equal(a["index"], b["index"]), k
                surf = hits["prim"][a["index"]] >= 0
                for f in a:
                    assert a[f][..., surf].tobytes() == b[f][..., surf].tobytes(), (k, f)
        # shadow side, first pass: exactly the unoccluded rays without candidates have added their radiance
        exp1 = ob.record_shadow(np.where(flat_occ == 0, 0, 1).astype(np.uint8), Ld[:ns], r_u[:ns], r_l[:ns], px[:ns], L)
        assert np.array_equal(o["L"].cpu().numpy().view(np.uint32), exp1.view(np.uint32))
        # the host resolves, writes the merged records back and enqueues the needs_host rays
        res = resolve_host_candidates(rays[:nq], hits[:nq], cands, s.callback(rays), kind=np.zeros(len(s.prims), np.int32))
        assert (cands["count"] >= 0).all()
        o["hits"][:nq] = _t(res).reshape(nq, 32)
        nh2 = WorkQueue(n, dev)
        enqueue_closest_items(mesh, n, o["rq"], o["hits"], prim_class=o["wf"].prim_class, items=o["items"], needs_host=nh2,
                              index=o["nh"], **o["queues"])
        torch.cuda.synchronize()
        assert nh2.Size() == plain_t["nh"].Size() == 0
        # (the node / test counts of a ray with candidates are the device walk's, include/nnbvh.h)
        assert_resolved_equal(res, plain_t["hits"].cpu().numpy().view(HIT_DTYPE).reshape(-1)[:nq], "queue records")
        for k in QUEUES:
            assert o["queues"][k].Size() == plain_t["queues"][k].Size(), k
            if k in o["items"]:
                a, b = _items_by_index(o["queues"][k], o["items"][k]), _items_by_index(plain_t["queues"][k], plain_t["items"][k])
                assert np.array_equal(a["index"], b["index"]), k
                surf = res["prim"][a["index"]] >= 0
                for f in a:
                    assert a[f][..., surf].tobytes() == b[f][..., surf].tobytes(), (k, f)
            else:
                assert np.array_equal(np.sort(o["queues"][k].indices().cpu().numpy()),
                                      np.sort(plain_t["queues"][k].indices().cpu().numpy())), k
        got = resolve_host_candidates_any(srays[:ns], flat_occ, scands, s.callback(srays))
        assert (got != 2).all() and ((flat_occ == 2) & (got == 0)).sum() > 20
        second = np.where((flat_occ == 2) & (got == 0), 0, 1).astype(np.uint8)
        record_shadow(max_shadow, o["sq"], t(second), t(Ld), t(r_u), t(r_l), t(px), o["L"])
        torch.cuda.synchronize()
        eocc = ob.kd_any_hit(s.tree_t.nodes, s.tree_t.prim_indices, s.prims, s.verts, s.tree_t.bounds, srays[:ns], 4)[0]
        assert np.array_equal(got, eocc)
        expL = ob.record_shadow(eocc, Ld[:ns], r_u[:ns], r_l[:ns], px[:ns], L)
        assert np.array_equal(o["L"].cpu().numpy().view(np.uint32), expL.view(np.uint32))
        assert np.array_equal(plain_t["L"].cpu().numpy().view(np.uint32), expL.view(np.uint32))
    agg_h.close()
    agg_t.close()
    mesh.close()
