"""IntersectShadowTr / IntersectOneRandom on kd-tree scenes, walked inside ONE trace launch
(nnbvh_kd_wavefront_walk_shadow_tr / _one_random, WavefrontAggregate.WalkShadowTr / WalkOneRandom).

An item is finished iff the reference loop (wavefront/intersect.h:183-256, aggregate.cpp:100-108) makes at most
max_surfaces calls of Intersect for it.  The reference is composed here as in test_wavefront_tr.py — every piece pinned
to the compiled reference — with the oracle's KdTreeAggregate::Intersect (ob.kd_closest) as the closest hit and a count
of the Intersect calls per item.  Scenes the composed oracle does not cover (bilinear patches, host-only primitives)
take their expected values from a loop in the test over calls that exist without the walk: KdTreeAggregate.Intersect,
the interaction post-pass and ob.offset_batch.

The module's name sorts it behind the existing test modules on purpose: its capture test adds a side stream and a
captured graph to the process, and the GPU tests that were here before keep the process state they have always run
in."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import oracle_binding as ob
import scenes_small as ss
from nn_bvh_amd import HIT_DTYPE, RAY_DTYPE, NNBVHError, _lib, build_tree, scene
from nn_bvh_amd.kdtree import KdTreeAggregate, build_kd_tree
from test_wavefront_bounded import SENTINEL, host_prim_scene, one_random_numpy, patch_scene, shadow_radiance
from test_wavefront_tr import layered_scene, oracle_interactions, oracle_shadow_tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WALKS = ("nnbvh_kd_wavefront_walk_shadow_tr", "nnbvh_kd_wavefront_walk_one_random")
ERR_ARG = 1
UNCAPPED = 65536
FINISHED = (1, 3)  # NNBVH_INTERACTION_TRIANGLE, NNBVH_INTERACTION_PATCH: all fields of the interaction valid


# ---- the composed reference, over any closest-hit function ------------------------------------------------------------
def shadow_walk(closest, verts, tris, rays, prim_class):
    """oracle_shadow_tr's loop -> (state per ray, Intersect calls per ray)."""
    n = len(rays)
    state, calls = np.zeros(n, np.uint8), np.zeros(n, np.int64)
    p_light = (rays["o"] + rays["d"] * rays["tmax"][:, None]).astype(np.float32)
    cur, idx = rays.copy(), np.arange(n)
    while len(idx):
        live = (cur["d"] != 0).any(1)  # while (ray.d != Vector3f(0, 0, 0)), intersect.h:183
        cur, idx = cur[live], idx[live]
        if not len(idx):
            break
        calls[idx] += 1
        h = closest(cur)
        hit = h["prim"] >= 0
        iface = hit & ((prim_class[np.maximum(h["prim"], 0)] & 2) != 0)
        state[idx[hit & ~iface]] = 1
        cur, idx, h = cur[iface], idx[iface], h[iface]
        if not len(idx):
            break
        lo, hi, nn = oracle_interactions(verts, tris, cur, h)
        sp = ob.offset_batch(np.concatenate([lo, hi, nn, p_light[idx]], 1))
        cur = cur.copy()
        cur["o"], cur["d"] = sp[:, 3:6], sp[:, 6:9]
    return state, calls


def one_random_walk(closest, verts, tris, p0, p1, material, prim_material):
    """oracle_one_random's loop -> (selected hits, their segment rays, pdf, weight sum, Intersect calls per item)."""
    n = len(p0)
    sel_hit = np.zeros(n, HIT_DTYPE)
    sel_hit["prim"] = -1
    sel_ray = np.zeros(n, RAY_DTYPE)
    calls = np.zeros(n, np.int64)
    matches = [[] for _ in range(n)]
    lo, hi, nn = p0.copy(), p0.copy(), np.zeros_like(p0)
    idx = np.arange(n)
    while len(idx):
        sp = ob.offset_batch(np.concatenate([lo, hi, nn, p1[idx]], 1))
        rays = np.zeros(len(idx), RAY_DTYPE)
        rays["o"], rays["d"], rays["tmax"] = sp[:, 3:6], sp[:, 6:9], 1.0
        live = (rays["d"] != 0).any(1)
        rays, idx = rays[live], idx[live]
        if not len(idx):
            break
        calls[idx] += 1
        h = closest(rays)
        hit = h["prim"] >= 0
        rays, idx, h = rays[hit], idx[hit], h[hit]
        if not len(idx):
            break
        lo, hi, nn = oracle_interactions(verts, tris, rays, h)
        for j, i in enumerate(idx):
            if prim_material[h["prim"][j]] == material[i]:
                matches[i].append((h[j].copy(), rays[j].copy()))
    pdf, wsum = np.zeros(n, np.float32), np.zeros(n, np.float32)
    for i in range(n):
        k = len(matches[i])
        sel, out = ob.wrs_batch(np.concatenate([p0[i], p1[i], [k]]).astype(np.float32)[None])
        pdf[i], wsum[i] = out[0]
        if k:
            sel_hit[i], sel_ray[i] = matches[i][sel[0]]
    return sel_hit, sel_ray, pdf, wsum, calls


class Case:
    pass


@functools.lru_cache(maxsize=None)
def layered_case():
    """layered_scene(3) as a kd tree, the ray set of test_device_shadow_tr_equals_oracle and one-random segments."""
    c = Case()
    c.verts, c.tris = layered_scene(3)
    c.prims = ss.make_prims(c.tris)
    c.kd = build_kd_tree(c.prims, c.verts)
    c.closest = lambda rays: ob.kd_closest(c.kd.nodes, c.kd.prim_indices, c.prims, c.verts, c.kd.bounds, rays, 4)
    rng = np.random.default_rng(8)
    n = c.n = 6000
    c.rays = scene.random_rays(n, [-3.5, -3.5, -5], [3.5, 3.5, 5], 9, tmax=1 - 1e-4)
    c.rays["d"][::97] = 0
    c.rays["time"] = rng.random(n).astype(np.float32)
    c.cls = rng.choice(np.array([0, 1, 2, 2, 2, 6], np.uint8), len(c.tris))
    c.Ld = (rng.random((n, 4), np.float32) * 2).astype(np.float32)
    c.ru = (rng.random((n, 4), np.float32) + 0.5).astype(np.float32)
    c.rl = (rng.random((n, 4), np.float32) + 0.5).astype(np.float32)
    c.pixel = rng.permutation(n).astype(np.int32)
    c.L0 = rng.random((n, 4), np.float32).astype(np.float32)
    c.state, c.calls = shadow_walk(c.closest, c.verts, c.tris, c.rays, c.cls)
    return c


@functools.lru_cache(maxsize=None)
def one_random_case():
    s = layered_case()
    c = Case()
    c.verts, c.tris, c.prims, c.kd, c.closest = s.verts, s.tris, s.prims, s.kd, s.closest
    rng = np.random.default_rng(10)
    n = c.n = 3000
    c.p0 = rng.uniform([-3, -3, -4.5], [3, 3, 4.5], (n, 3)).astype(np.float32)
    c.p1 = rng.uniform([-3, -3, -4.5], [3, 3, 4.5], (n, 3)).astype(np.float32)
    c.p1[::50] = c.p0[::50]
    c.prim_material = rng.integers(0, 3, len(c.tris)).astype(np.int32)
    c.material = rng.integers(0, 3, n).astype(np.int32)
    c.hits, c.rays, c.pdf, c.wsum, c.calls = one_random_walk(c.closest, c.verts, c.tris, c.p0, c.p1, c.material,
                                                             c.prim_material)
    return c


@functools.lru_cache(maxsize=None)
def all_interface_case():
    """The layered scene with every class set to interface: every ray walks to its light."""
    s = layered_case()
    c = Case()
    c.verts, c.tris, c.prims, c.kd, c.closest = s.verts, s.tris, s.prims, s.kd, s.closest
    c.n = 257
    c.rays = s.rays[1:1 + c.n].copy()  # ray 0 of the set has a zero direction; these start with a live one
    c.cls = np.full(len(c.tris), 2, np.uint8)
    c.Ld, c.ru, c.rl, c.L0 = s.Ld[:c.n], s.ru[:c.n], s.rl[:c.n], s.L0[:c.n]
    c.pixel = np.arange(c.n, dtype=np.int32)  # (every prefix of it stays inside its own L)
    c.state, c.calls = shadow_walk(c.closest, c.verts, c.tris, c.rays, c.cls)
    return c


def shadow_expected(c, cap, size=None, n=None, order=None):
    """(state, L) the walk call must leave for the first `size` of the case's first n rays taken in `order`."""
    n = c.n if n is None else n
    order = np.arange(n) if order is None else order
    size = n if size is None else size
    state = np.where(c.calls > cap, 2, c.state).astype(np.uint8)[order]
    full = np.full(n, SENTINEL, np.uint8)
    full[:size] = state[:size]
    live = np.full(n, 1, np.uint8)  # anything but 0: rays beyond the size add nothing
    live[:size] = state[:size]
    return full, shadow_radiance(live, c.Ld[order], c.ru[order], c.rl[order], c.pixel[:n], c.L0[:n])


# ---- CPU ----------------------------------------------------------------------------------------------------------
def test_walk_calls_are_exported_prototyped_and_declared(nnbvh_lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nnbvh.h")).read(), flags=re.S)
    for name, twin in zip(WALKS, ("nnbvh_wavefront_intersect_shadow_tr_bounded",
                                  "nnbvh_wavefront_intersect_one_random_bounded")):
        assert name in _lib.EXPORTS and hasattr(nnbvh_lib, name), name
        fn = getattr(nnbvh_lib, name)
        assert fn.restype == ctypes.c_int32 and fn.argtypes == getattr(nnbvh_lib, twin).argtypes, name
        assert re.search(r"\b" + name + r"\s*\(", header), name
        decl = header[header.index(name):]
        decl = re.sub(r"\s+", " ", decl[:decl.index(";")])
        assert decl.startswith(name + "(nnbvh_kd_scene *s, const nnbvh_shading_mesh *m, int32_t max_")
        assert "int32_t max_surfaces, int32_t *d_unfinished, void *stream)" in decl
    adapter = open(os.path.join(ROOT, "include", "nnbvh_aggregate.hpp")).read()
    kd = adapter[adapter.index("class HipKdTreeAggregate"):]
    assert "void WalkShadowTr(" in kd and "void WalkOneRandom(" in kd
    assert "nnbvh_kd_wavefront_walk_shadow_tr(" in kd and "nnbvh_kd_wavefront_walk_one_random(" in kd


# where the refusals that read a handle find their fields: `int device` opens both structs; the mesh's instance table
# follows two ints, eight pointers and two ints; the scene's attribute array follows nine ints, six floats (padded to 8)
# and three pointers
MESH_INSTANCES_AT, SCENE_EXTRAS_AT = 8 + 8 * 8 + 8, 64 + 3 * 8


def test_walk_calls_reject_bad_arguments_before_any_device_work(nnbvh_lib):
    """NNBVH_ERR_ARG with a message that names the call.  Zeroed stand-ins serve where a handle must be non-NULL (the
    checks read `device`, the mesh's instance table and the scene's attribute array from them): nothing reaches a
    device."""
    fake_scene, fake_mesh = ctypes.create_string_buffer(1 << 16), ctypes.create_string_buffer(1 << 16)
    S, M = ctypes.addressof(fake_scene), ctypes.addressof(fake_mesh)
    soa = np.zeros(1, _lib.RAY_SOA_DTYPE)
    for k in ("ox", "oy", "oz", "dx", "dy", "dz", "tmax"):
        soa[k] = 64  # non-NULL, never read
    Q, A = soa.ctypes.data, 64

    def shadow(s=S, m=M, n=8, q=Q, npc=0, arrays=(A, A, A, A, A), npx=8, cap=4):
        return nnbvh_lib.nnbvh_kd_wavefront_walk_shadow_tr(s, m, n, q, None, None, npc, *arrays, npx, None, cap, None,
                                                           None)

    def one_random(s=S, m=M, n=8, arrays=(A, A, A), npm=0, outs=(A, A, A), cap=4):
        return nnbvh_lib.nnbvh_kd_wavefront_walk_one_random(s, m, n, *arrays, None, None, npm, *outs, None, cap, None,
                                                            None)

    for call, name in ((shadow, "kd_wavefront_walk_shadow_tr"), (one_random, "kd_wavefront_walk_one_random")):
        bad = [dict(s=None), dict(m=None), dict(cap=0), dict(cap=65537), dict(cap=-1), dict(n=-1), dict(n=1 << 28),
               dict(n=(1 << 31) - 1)]
        if call is shadow:
            bad += [dict(npc=-1), dict(npx=-1), dict(q=None)]
            bad += [dict(arrays=tuple(None if j == k else A for j in range(5))) for k in range(5)]
            nosoa = soa.copy()
            nosoa["dx"] = 0
            bad.append(dict(q=nosoa.ctypes.data))
        else:
            bad += [dict(npm=-1)]
            bad += [dict(arrays=tuple(None if j == k else A for j in range(3))) for k in range(3)]
            bad += [dict(outs=tuple(None if j == k else A for j in range(3))) for k in range(3)]
        for kw in bad:
            assert call(**kw) == ERR_ARG, (name, kw)
            assert _lib.last_error().startswith(name + ":"), (_lib.last_error(), kw)
        # what the checks read from the handles, each refusal with the words that tell the caller what to change
        for buf, at, value, words in ((fake_mesh, 0, 1, "different devices"),
                                      (fake_mesh, MESH_INSTANCES_AT, 64, "instance table"),
                                      (fake_scene, SCENE_EXTRAS_AT, 64, "ATTR")):
            ctypes.memmove(ctypes.addressof(buf) + at, ctypes.byref(ctypes.c_int64(value)), 8)
            assert call() == ERR_ARG, (name, words)
            assert _lib.last_error().startswith(name + ":") and words in _lib.last_error(), _lib.last_error()
            ctypes.memset(ctypes.addressof(buf) + at, 0, 8)


def test_wavefront_aggregate_offers_the_walks_for_kd_scenes_only():
    pytest.importorskip("torch")
    from nn_bvh_amd.wavefront import WavefrontAggregate

    class Handle:  # what WavefrontAggregate reads of a BVH aggregate before it refuses
        device = 0
        _h = None

    wf = WavefrontAggregate(Handle())
    with pytest.raises(NNBVHError, match="not offered for BVH scenes"):
        wf.WalkShadowTr(0, None, None, None, None, None, None, None)
    with pytest.raises(NNBVHError, match="not offered for BVH scenes"):
        wf.WalkOneRandom(0, None, None, None, None)
    kd = WavefrontAggregate(KdTreeAggregate(None, np.zeros(6, np.float32)))
    with pytest.raises(NNBVHError, match="not offered for kd-tree.*WalkShadowTr"):
        kd.IntersectShadowTr(0, None, None, None, None, None, None, None)
    with pytest.raises(NNBVHError, match="not offered for kd-tree.*WalkOneRandom"):
        kd.IntersectOneRandom(0, None, None, None, None)


def test_inputs_make_both_sides_of_every_cap_non_empty():
    """The preconditions of the GPU tests, from the composed reference alone."""
    s, r, a = layered_case(), one_random_case(), all_interface_case()
    assert len(s.tris) == 1127 and len(s.kd.nodes) == 5841
    assert np.array_equal(np.bincount(s.calls), [62, 2587, 1696, 905, 469, 183, 77, 20, 1])
    assert ((s.state == 0).sum(), (s.state == 1).sum()) == (2942, 3058)
    assert np.array_equal(np.bincount(r.calls), [60, 484, 674, 589, 500, 323, 223, 115, 32])
    for c in (s, r):
        assert c.calls.max() == 8
        for cap in (1, 2, 3, 7):
            assert 0 < (c.calls > cap).sum() < c.n
    assert (r.hits["prim"] >= 0).mean() > 0.3
    # the BVH reference of the same scene gives the same verdicts, and the pinned loop agrees with the counted one
    tree = build_tree(s.prims, s.verts)
    bvh_state, bvh_calls = shadow_walk(lambda rays: ob.closest(tree.nodes, tree.ordered_prims, s.verts, rays, 4), s.verts,
                                       s.tris, s.rays, s.cls)
    assert (bvh_state != s.state).sum() == 0
    L = s.L0.copy()
    state, passes = oracle_shadow_tr(tree, s.verts, s.tris, s.rays, s.cls, s.Ld, s.ru, s.rl, s.pixel, L)
    assert np.array_equal(state, bvh_state) and passes == bvh_calls.max() == 8
    assert L.tobytes() == shadow_radiance(bvh_state, s.Ld, s.ru, s.rl, s.pixel, s.L0).tobytes()
    # the small shapes: ray 0 walks through at least four surfaces, and nothing is blocked
    assert a.calls[0] >= 4 and (a.state == 0).all() and a.calls.max() >= 6


# ---- GPU ----------------------------------------------------------------------------------------------------------
class ShadowDevice:
    """A shadow case on the device: kd scene, mesh, queue and per-ray arrays."""

    def __init__(self, c, n=None, cls=None):
        import torch
        from nn_bvh_amd.interaction import ShadingMesh
        from nn_bvh_amd.wavefront import RayQueue, WavefrontAggregate
        self.c, self.dev, self.n = c, torch.device("cuda", 0), c.n if n is None else n
        self.agg = KdTreeAggregate.from_tree(c.kd.nodes, c.kd.prim_indices, c.prims, c.verts, c.kd.bounds)
        self.mesh = ShadingMesh(c.verts, c.tris)
        self.wf = WavefrontAggregate(self.agg, c.cls if cls is None else cls)
        self.t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        rays = c.rays[:self.n]
        self.q = RayQueue.from_records(rays, self.dev, shadow=True)
        self.q.time = self.t(rays["time"])
        self.Ld, self.ru, self.rl = self.t(c.Ld[:self.n]), self.t(c.ru[:self.n]), self.t(c.rl[:self.n])
        self.pixel = self.t(c.pixel[:self.n])
        self.unfinished = torch.full((1,), -3, dtype=torch.int32, device=self.dev)

    def set_rays(self, rays, order):
        c = self.c
        self.q.o.copy_(self.t(rays["o"].T))
        self.q.d.copy_(self.t(rays["d"].T))
        self.q.tmax.copy_(self.t(rays["tmax"]))
        self.q.time.copy_(self.t(rays["time"]))
        for dst, src in ((self.Ld, c.Ld), (self.ru, c.ru), (self.rl, c.rl)):
            dst.copy_(self.t(src[order]))

    def run(self, cap, L=None, state=None):
        import torch
        L = self.t(self.c.L0[:self.n]) if L is None else L
        state = torch.full((self.n,), SENTINEL, dtype=torch.uint8, device=self.dev) if state is None else state
        self.wf.WalkShadowTr(self.n, self.q, self.mesh, self.Ld, self.ru, self.rl, self.pixel, L, state,
                             max_surfaces=cap, unfinished=self.unfinished)
        torch.cuda.synchronize()
        return state.cpu().numpy(), L.cpu().numpy(), int(self.unfinished.item())

    def close(self):
        self.agg.close()
        self.mesh.close()


class OneRandomDevice:
    def __init__(self, c):
        import torch
        from nn_bvh_amd.interaction import ShadingMesh
        from nn_bvh_amd.wavefront import WavefrontAggregate
        self.c, self.dev = c, torch.device("cuda", 0)
        self.agg = KdTreeAggregate.from_tree(c.kd.nodes, c.kd.prim_indices, c.prims, c.verts, c.kd.bounds)
        self.mesh = ShadingMesh(c.verts, c.tris)
        self.wf = WavefrontAggregate(self.agg)
        self.t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        self.p0, self.p1, self.material = self.t(c.p0), self.t(c.p1), self.t(c.material)
        self.prim_material = self.t(c.prim_material)
        self.size = torch.full((1,), c.n, dtype=torch.int32, device=self.dev)
        self.unfinished = torch.full((1,), -3, dtype=torch.int32, device=self.dev)

    def call(self, cap):
        return self.wf.WalkOneRandom(self.c.n, self.p0, self.p1, self.material, self.mesh, self.prim_material,
                                     size=self.size, max_surfaces=cap, unfinished=self.unfinished)

    def run(self, cap):
        import torch
        out = self.call(cap)
        torch.cuda.synchronize()
        return one_random_numpy(out) + (int(self.unfinished.item()),)

    def close(self):
        self.agg.close()
        self.mesh.close()


def check_one_random(c, got, cap, size=None, order=None):
    """Finished items hold the reference's outputs bit for bit, unfinished ones instance = -1; returns their number."""
    gh, gr, pdf, wsum = got[:4]
    order = np.arange(c.n) if order is None else order
    size = c.n if size is None else size
    rows = np.arange(size)
    fin = c.calls[order][rows] <= cap
    f, src = rows[fin], order[rows][fin]
    assert (gh["instance"][rows[~fin]] == -1).all()
    assert np.array_equal(gh["prim"][f], c.hits["prim"][src]) and (gh["instance"][f] != -1).all()
    assert np.array_equal(wsum[f].view(np.uint32), c.wsum[src].view(np.uint32))
    assert np.array_equal(pdf[f].view(np.uint32), c.pdf[src].view(np.uint32))
    sel = c.hits["prim"][src] >= 0
    assert gh[f][sel].tobytes() == c.hits[src][sel].tobytes() and gr[f][sel].tobytes() == c.rays[src][sel].tobytes()
    assert not pdf[size:].any() and not wsum[size:].any()  # beyond the size: the zero fill, untouched
    return int((~fin).sum())


@pytest.mark.gpu
def test_gpu_shadow_walk_equals_the_composed_kd_reference():
    import torch
    c = layered_case()
    d = ShadowDevice(c)
    state, L, unfinished = d.run(UNCAPPED)
    exp_state, exp_L = shadow_expected(c, UNCAPPED)
    print(f"states {np.bincount(state, minlength=3)[:3]} (reference {np.bincount(exp_state, minlength=3)[:3]}), "
          f"unfinished {unfinished}")
    assert np.array_equal(state, exp_state)
    assert L.tobytes() == exp_L.tobytes()
    assert unfinished == 0
    # the device-side size at n / 2: items beyond it are untouched
    d.q.size.fill_(c.n // 2)
    state, L, unfinished = d.run(UNCAPPED)
    exp_state, exp_L = shadow_expected(c, UNCAPPED, c.n // 2)
    assert (state[c.n // 2:] == SENTINEL).all() and np.array_equal(state, exp_state)
    assert L.tobytes() == exp_L.tobytes() and unfinished == 0
    d.q.size.fill_(c.n)
    # without interface surfaces the live rays' verdict is IntersectP's
    wf0 = type(d.wf)(d.agg, np.zeros(len(c.tris), np.uint8))
    st0 = torch.full((c.n,), SENTINEL, dtype=torch.uint8, device=d.dev)
    wf0.WalkShadowTr(c.n, d.q, d.mesh, d.Ld, d.ru, d.rl, d.pixel, d.t(c.L0), st0, unfinished=d.unfinished)
    torch.cuda.synchronize()
    live = (c.rays["d"] != 0).any(1)
    occ = d.agg.IntersectP(c.rays)
    assert np.array_equal(st0.cpu().numpy()[live], occ[live]) and 0.05 < occ[live].mean() < 0.95
    assert (st0.cpu().numpy()[~live] == 0).all() and int(d.unfinished.item()) == 0
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [1, 2, 3, 7, 8])
def test_gpu_shadow_walk_stops_at_max_surfaces(cap):
    c = layered_case()
    d = ShadowDevice(c)
    state, L, unfinished = d.run(cap)
    exp_state, exp_L = shadow_expected(c, cap)
    left = int((c.calls > cap).sum())
    print(f"max_surfaces {cap}: unfinished {unfinished} (reference {left}), states "
          f"{np.bincount(state, minlength=3)[:3]} (reference {np.bincount(exp_state, minlength=3)[:3]})")
    assert (left == 0) == (cap == 8)
    assert np.array_equal(state, exp_state)
    assert L.tobytes() == exp_L.tobytes()
    assert unfinished == left
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [UNCAPPED, 1, 3])
def test_gpu_one_random_walk_equals_the_composed_kd_reference(cap):
    c = one_random_case()
    d = OneRandomDevice(c)
    got = d.run(cap)
    left = check_one_random(c, got, cap)
    print(f"max_surfaces {cap}: unfinished {got[4]} (reference {left})")
    assert left == int((c.calls > cap).sum()) and (left == 0) == (cap == UNCAPPED)
    assert got[4] == left
    if cap == UNCAPPED:  # ... and under a device-side size
        d.size.fill_(c.n // 2)
        got = d.run(cap)
        assert check_one_random(c, got, cap, c.n // 2) == 0 and got[4] == 0
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n,size", [(1, None), (63, None), (64, None), (65, None), (257, 130)])
def test_gpu_shadow_walk_small_shapes(n, size):
    """The smallest shapes at which the in-lane continuation can go wrong: one continuing lane beside 63 idle ones on
    an exhausted queue, a full wave, a second wave with one lane, and a device-side size inside a wave."""
    c = all_interface_case()
    d = ShadowDevice(c, n)
    if size is not None:
        d.q.size.fill_(size)
    for cap in (UNCAPPED, 2):
        state, L, unfinished = d.run(cap)
        exp_state, exp_L = shadow_expected(c, cap, size, n)
        assert np.array_equal(state, exp_state), (n, cap)
        assert L.tobytes() == exp_L.tobytes(), (n, cap)
        assert unfinished == int((c.calls[:n if size is None else size] > cap).sum()), (n, cap)
    d.close()


@pytest.mark.gpu
def test_gpu_walk_calls_are_hip_graph_capturable():
    """Both walk calls in ONE captured graph (a linear chain of kernel nodes); between the replays the queue contents
    and the device-side sizes are rewritten in place, and each replay equals the reference for the inputs it saw."""
    import torch
    c, r = layered_case(), one_random_case()
    d, e = ShadowDevice(c), OneRandomDevice(r)
    L0 = d.t(c.L0)
    L = L0.clone()
    state = torch.full((c.n,), SENTINEL, dtype=torch.uint8, device=d.dev)
    side = torch.cuda.Stream(d.dev)
    torch.cuda.synchronize()

    def step():
        d.wf.WalkShadowTr(c.n, d.q, d.mesh, d.Ld, d.ru, d.rl, d.pixel, L, state, max_surfaces=UNCAPPED,
                          unfinished=d.unfinished)
        return e.call(7)

    with torch.cuda.stream(side):
        step()  # warm-up: the stream's workspace gets its size (allocation is not capturable)
    torch.cuda.synchronize()
    L.copy_(L0)
    state.fill_(SENTINEL)
    d.unfinished.fill_(-3)
    e.unfinished.fill_(-3)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = step()
    torch.cuda.synchronize()
    assert (state == SENTINEL).all() and torch.equal(L, L0), "capture must not execute the work"
    assert int(d.unfinished.item()) == -3 and int(e.unfinished.item()) == -3
    graph.replay()
    torch.cuda.synchronize()
    exp_state, exp_L = shadow_expected(c, UNCAPPED)
    assert np.array_equal(state.cpu().numpy(), exp_state) and L.cpu().numpy().tobytes() == exp_L.tobytes()
    assert int(d.unfinished.item()) == 0
    assert check_one_random(r, one_random_numpy(out), 7) == 32 == int(e.unfinished.item())
    # replay 2: every queue reversed in place and cut to half by its device-side size
    so, ro = np.arange(c.n)[::-1].copy(), np.arange(r.n)[::-1].copy()
    d.set_rays(c.rays[so], so)
    d.q.size.fill_(c.n // 2)
    e.p0.copy_(e.t(r.p0[ro]))
    e.p1.copy_(e.t(r.p1[ro]))
    e.material.copy_(e.t(r.material[ro]))
    e.size.fill_(r.n // 2)
    L.copy_(L0)
    state.fill_(SENTINEL)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    exp_state, exp_L = shadow_expected(c, UNCAPPED, c.n // 2, order=so)
    assert np.array_equal(state.cpu().numpy(), exp_state) and L.cpu().numpy().tobytes() == exp_L.tobytes()
    assert int(d.unfinished.item()) == 0
    left = check_one_random(r, one_random_numpy(out), 7, r.n // 2, ro)
    assert left == int((r.calls[ro][: r.n // 2] > 7).sum()) == int(e.unfinished.item())
    del graph
    d.close()
    e.close()


# ---- beyond flat triangles: expected values from calls that exist without the walk ----------------------------------
def device_shadow_walk(agg, mesh, rays, prim_class):
    """shadow_walk over KdTreeAggregate.Intersect and the interaction post-pass -> (state, calls)."""
    n = len(rays)
    state, calls = np.zeros(n, np.uint8), np.zeros(n, np.int64)
    p_light = (rays["o"] + rays["d"] * rays["tmax"][:, None]).astype(np.float32)
    cur, idx = rays.copy(), np.arange(n)
    while len(idx):
        live = (cur["d"] != 0).any(1)
        cur, idx = cur[live], idx[live]
        if not len(idx):
            break
        calls[idx] += 1
        h = agg.Intersect(cur)
        void = h["instance"] == -1
        state[idx[void]] = 2
        hit = ~void & (h["prim"] >= 0)
        iface = hit & ((prim_class[np.maximum(h["prim"], 0)] & 2) != 0)
        state[idx[hit & ~iface]] = 1
        cur, idx, h = cur[iface], idx[iface], h[iface]
        if not len(idx):
            break
        it = mesh.interactions(cur, h)
        ok = np.isin(it["status"], FINISHED)
        state[idx[~ok]] = 2
        cur, idx, it = cur[ok], idx[ok], it[ok]
        if not len(idx):
            break
        sp = ob.offset_batch(np.concatenate([it["pi_lo"], it["pi_hi"], it["n"], p_light[idx]], 1))
        cur = cur.copy()
        cur["o"], cur["d"] = sp[:, 3:6], sp[:, 6:9]
    return state, calls


def device_one_random_walk(agg, mesh, p0, p1, material, prim_material):
    """one_random_walk over KdTreeAggregate.Intersect and the interaction post-pass; `host`: the caller's items."""
    n = len(p0)
    sel_hit = np.zeros(n, HIT_DTYPE)
    sel_hit["prim"] = -1
    sel_ray = np.zeros(n, RAY_DTYPE)
    calls, host = np.zeros(n, np.int64), np.zeros(n, bool)
    matches = [[] for _ in range(n)]
    lo, hi, nn = p0.copy(), p0.copy(), np.zeros_like(p0)
    idx = np.arange(n)
    while len(idx):
        sp = ob.offset_batch(np.concatenate([lo, hi, nn, p1[idx]], 1))
        rays = np.zeros(len(idx), RAY_DTYPE)
        rays["o"], rays["d"], rays["tmax"] = sp[:, 3:6], sp[:, 6:9], 1.0
        live = (rays["d"] != 0).any(1)
        rays, idx = rays[live], idx[live]
        if not len(idx):
            break
        calls[idx] += 1
        h = agg.Intersect(rays)
        void = h["instance"] == -1
        host[idx[void]] = True
        hit = ~void & (h["prim"] >= 0)
        rays, idx, h = rays[hit], idx[hit], h[hit]
        if not len(idx):
            break
        it = mesh.interactions(rays, h)
        ok = np.isin(it["status"], FINISHED)
        host[idx[~ok]] = True
        rays, idx, h, it = rays[ok], idx[ok], h[ok], it[ok]
        if not len(idx):
            break
        lo, hi, nn = it["pi_lo"], it["pi_hi"], it["n"]
        for j, i in enumerate(idx):
            if prim_material[h["prim"][j]] == material[i]:
                matches[i].append((h[j].copy(), rays[j].copy()))
    pdf, wsum = np.zeros(n, np.float32), np.zeros(n, np.float32)
    for i in range(n):
        k = len(matches[i])
        sel, out = ob.wrs_batch(np.concatenate([p0[i], p1[i], [k]]).astype(np.float32)[None])
        pdf[i], wsum[i] = out[0]
        if k:
            sel_hit[i], sel_ray[i] = matches[i][sel[0]]
    return sel_hit, sel_ray, pdf, wsum, calls, host


@pytest.mark.gpu
@pytest.mark.parametrize("make", [patch_scene, host_prim_scene])
def test_gpu_walks_beyond_flat_triangles(make):
    import torch
    from nn_bvh_amd.interaction import ShadingMesh
    from nn_bvh_amd.wavefront import RayQueue, WavefrontAggregate
    s = make()
    _, prims, verts = s["tree"]
    prims = np.sort(prims, order="id")  # the caller's order: the tree's ordered_prims carry every primitive once
    assert np.array_equal(prims["id"], np.arange(s["n_ids"]))
    if make is host_prim_scene:
        rng = np.random.default_rng(23)
        lo = rng.uniform(-2.5, 2.5, (len(prims), 3)).astype(np.float32)
        pb = np.concatenate([lo, lo + rng.uniform(0.3, 0.8, (len(prims), 3)).astype(np.float32)], 1)
        kd = build_kd_tree(prims, verts, prim_bounds=pb)
    else:
        kd = build_kd_tree(prims, verts)
    agg = KdTreeAggregate.from_tree(kd.nodes, kd.prim_indices, prims, verts, kd.bounds)
    mesh = ShadingMesh(verts, **s["mesh"])
    info = agg.info()
    assert info["has_patches"] == (make is patch_scene) and info["has_host_prims"] == (make is host_prim_scene)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    rng = np.random.default_rng(31)
    n, box = 2001, s["box"]
    cls = rng.choice(np.array([0, 2, 2, 2, 2, 6], np.uint8), s["n_ids"])
    wf = WavefrontAggregate(agg, cls)
    rays = scene.random_rays(n, [-box] * 3, [box] * 3, 32, tmax=1 - 1e-4)
    rays["d"][::97] = 0
    rays["time"] = rng.random(n).astype(np.float32)
    q = RayQueue.from_records(rays, dev, shadow=True)
    q.time = t(rays["time"])
    Ld, ru, rl = ((rng.random((n, 4), np.float32) + 0.5).astype(np.float32) for _ in range(3))
    pixel = rng.permutation(n).astype(np.int32)
    L0 = rng.random((n, 4), np.float32).astype(np.float32)
    unfinished = torch.full((1,), -3, dtype=torch.int32, device=dev)
    ref_state, calls = device_shadow_walk(agg, mesh, rays, cls)
    assert min((ref_state == 0).sum(), (ref_state == 1).sum()) > 20 and (calls > 1).sum() > 20
    if make is host_prim_scene:
        assert (ref_state == 2).sum() > 20

    def shadow(cap):
        L, state = t(L0), torch.full((n,), SENTINEL, dtype=torch.uint8, device=dev)
        wf.WalkShadowTr(n, q, mesh, t(Ld), t(ru), t(rl), t(pixel), L, state, max_surfaces=cap, unfinished=unfinished)
        torch.cuda.synchronize()
        return state.cpu().numpy(), L.cpu().numpy(), int(unfinished.item())

    state, L, left = shadow(UNCAPPED)
    assert np.array_equal(state, ref_state) and left == 0
    assert L.tobytes() == shadow_radiance(ref_state, Ld, ru, rl, pixel, L0).tobytes()
    one_state, one_L, left = shadow(1)
    exp_one = np.where(calls > 1, 2, ref_state).astype(np.uint8)
    assert np.array_equal(one_state, exp_one) and left == (calls > 1).sum()
    assert one_L.tobytes() == shadow_radiance(exp_one, Ld, ru, rl, pixel, L0).tobytes()

    m = 1501
    p0 = rng.uniform(-box, box, (m, 3)).astype(np.float32)
    p1 = rng.uniform(-box, box, (m, 3)).astype(np.float32)
    p1[::50] = p0[::50]
    material = rng.integers(0, 3, m).astype(np.int32)
    prim_material = rng.integers(0, 3, s["n_ids"]).astype(np.int32)
    eh, er, epdf, ewsum, ecalls, host = device_one_random_walk(agg, mesh, p0, p1, material, prim_material)
    assert (eh["prim"][~host] >= 0).sum() > 20 and (ecalls > 1).sum() > 20
    if make is host_prim_scene:
        assert host.sum() > 20

    def one_random(cap):
        out = wf.WalkOneRandom(m, t(p0), t(p1), t(material), mesh, t(prim_material), max_surfaces=cap,
                               unfinished=unfinished)
        torch.cuda.synchronize()
        return one_random_numpy(out), int(unfinished.item())

    def check(got, own):
        """own: the items the device finishes itself; the others carry instance = -1"""
        gh, gr, pdf, wsum = got
        assert np.array_equal(gh["instance"] == -1, ~own)
        assert np.array_equal(gh["prim"][own], eh["prim"][own])
        assert np.array_equal(pdf[own].view(np.uint32), epdf[own].view(np.uint32))
        assert np.array_equal(wsum[own].view(np.uint32), ewsum[own].view(np.uint32))
        sel = own & (eh["prim"] >= 0)
        assert gh[sel].tobytes() == eh[sel].tobytes() and gr[sel].tobytes() == er[sel].tobytes()

    got, left = one_random(UNCAPPED)
    assert left == 0
    check(got, ~host)
    got, left = one_random(1)
    # an item the first call already hands to the caller (a host-only primitive) is marked, not counted
    assert left == (ecalls > 1).sum()
    check(got, ~host & (ecalls <= 1))
    agg.close()
    mesh.close()
