"""IntersectShadowTr / IntersectOneRandom on BVH scenes, walked inside ONE trace launch
(nnbvh_wavefront_walk_shadow_tr / _one_random, WavefrontAggregate.IntersectShadowTr / IntersectOneRandom with
max_surfaces).

An item is finished iff the reference loop (wavefront/intersect.h:183-256, aggregate.cpp:100-108) makes at most
max_surfaces calls of Intersect for it.  The cases, the composed reference and the checks are those of
test_wavefront_walk_kd.py with the oracle's BVHAggregate::Intersect (ob.closest) as the closest hit; the scenes the
composed oracle does not cover are those of test_wavefront_bounded.py, where the walk must equal the bounded and the
unbounded calls and, at cap 1, a loop in the test over calls that exist without the walk.

The module's name sorts it behind the existing test modules on purpose: its capture test adds a side stream and a
captured graph to the process."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import oracle_binding as ob
import scenes_small as ss
from ledger_cases import BVH, assert_reached, bvh, ledger_start
from nn_bvh_amd import NNBVHError, _lib, build_tree, scene
from test_wavefront_bounded import (SENTINEL, host_prim_scene, one_random_numpy, patch_scene, shadow_radiance,
                                    two_level_case)
from test_wavefront_bounded import shadow_walk as tree_shadow_walk
from test_wavefront_walk_kd import (UNCAPPED, Case, all_interface_case, check_one_random, device_one_random_walk,
                                    device_shadow_walk, layered_case, one_random_case, one_random_walk, shadow_expected,
                                    shadow_walk)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WALKS = ("nnbvh_wavefront_walk_shadow_tr", "nnbvh_wavefront_walk_one_random")
TWINS = ("nnbvh_wavefront_intersect_shadow_tr_bounded", "nnbvh_wavefront_intersect_one_random_bounded")
ERR_ARG = 1


# ---- the kd test's cases over the BVH of the same scene -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bvh_tree():
    s = layered_case()
    return build_tree(s.prims, s.verts)


def bvh_closest(rays):
    tree = bvh_tree()
    return ob.closest(tree.nodes, tree.ordered_prims, layered_case().verts, rays, 4)


def _on_bvh(kd_case):
    c = Case()
    c.__dict__.update(kd_case.__dict__)
    c.tree, c.closest = bvh_tree(), bvh_closest
    return c


@functools.lru_cache(maxsize=None)
def bvh_layered_case():
    c = _on_bvh(layered_case())
    c.state, c.calls = shadow_walk(bvh_closest, c.verts, c.tris, c.rays, c.cls)
    return c


@functools.lru_cache(maxsize=None)
def bvh_one_random_case():
    c = _on_bvh(one_random_case())
    c.hits, c.rays, c.pdf, c.wsum, c.calls = one_random_walk(bvh_closest, c.verts, c.tris, c.p0, c.p1, c.material,
                                                             c.prim_material)
    return c


@functools.lru_cache(maxsize=None)
def bvh_all_interface_case():
    c = _on_bvh(all_interface_case())
    c.state, c.calls = shadow_walk(bvh_closest, c.verts, c.tris, c.rays, c.cls)
    return c


@functools.lru_cache(maxsize=None)
def spill_case():
    """A tube chain that keeps 64 entries pending, every class interface: the first Intersect call of a ray goes through
    the HBM spill of the 8-entry window, and the ray re-enters the tree from the surface it met."""
    c = Case()
    ch = ss.chain_tree(64, np.random.default_rng(11), tube=True, leaves="tri", extras=True)
    c.verts, c.prims, c.nodes = ch.verts, ch.prims, ch.nodes
    c.tris = ch.prims["v"][:, :3].copy()
    x_far = float(ch.leaf_hi[:, 0].max())
    n = c.n = 321
    c.rays = ss.chain_rays(x_far, n, 12, tmax_share=0.0)
    c.rays["tmax"] = np.float32(x_far + 17.0)  # the light lies 5 beyond the chain's near end
    c.rays["time"] = 0
    with ob.pending_depth(n) as dc:
        ob.closest(c.nodes, c.prims, c.verts, c.rays)
    c.depth = dc.depth[:, 0].copy()
    c.cls = np.full(len(c.prims), 2, np.uint8)
    tree = Case()
    tree.nodes, tree.ordered_prims = c.nodes, c.prims
    c.state, c.calls = tree_shadow_walk(tree, c.verts, c.tris, c.rays, c.cls)
    rng = np.random.default_rng(13)
    c.Ld = (rng.random((n, 4), np.float32) * 2).astype(np.float32)
    c.ru = (rng.random((n, 4), np.float32) + 0.5).astype(np.float32)
    c.rl = (rng.random((n, 4), np.float32) + 0.5).astype(np.float32)
    c.pixel = rng.permutation(n).astype(np.int32)
    c.L0 = rng.random((n, 4), np.float32).astype(np.float32)
    return c


# ---- CPU ----------------------------------------------------------------------------------------------------------
def test_walk_calls_are_exported_prototyped_and_declared(nnbvh_lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nnbvh.h")).read(), flags=re.S)
    for name, twin in zip(WALKS, TWINS):
        assert name in _lib.EXPORTS and hasattr(nnbvh_lib, name), name
        fn = getattr(nnbvh_lib, name)
        assert fn.restype == ctypes.c_int32 and fn.argtypes == getattr(nnbvh_lib, twin).argtypes, name
        assert re.search(r"\b" + name + r"\s*\(", header), name
        decl = header[re.search(r"\b" + name + r"\s*\(", header).start():]
        decl = re.sub(r"\s+", " ", decl[:decl.index(";")])
        assert decl.startswith(name + "(nnbvh_scene *s, const nnbvh_shading_mesh *m, int32_t max_")
        assert "int32_t max_surfaces, int32_t *d_unfinished, void *stream)" in decl
        twin_decl = header[re.search(r"\b" + twin + r"\s*\(", header).start():]
        twin_decl = re.sub(r"\s+", " ", twin_decl[:twin_decl.index(";")])
        squeeze = lambda text: re.sub(r"\s+", "", text)  # noqa: E731
        assert squeeze(decl[len(name):]).replace("max_surfaces", "max_passes") == squeeze(twin_decl[len(twin):])
    adapter = open(os.path.join(ROOT, "include", "nnbvh_aggregate.hpp")).read()
    bvh = adapter[adapter.index("class HipBVHAggregate"):adapter.index("class HipKdTreeAggregate")]
    assert "void WalkShadowTr(" in bvh and "void WalkOneRandom(" in bvh
    assert "nnbvh_wavefront_walk_shadow_tr(" in bvh and "nnbvh_wavefront_walk_one_random(" in bvh


# where the refusals that read a handle find their fields: `int device` opens both structs; in the scene the animation
# table follows three ints (padded), a 64-bit count, an int, six floats, an int (padded) and two pointers, `instanced`
# follows it after an int (padded), a size, five ints (padded) and a pointer, and has_alpha is the third int behind that
SCENE_ANIM_AT, SCENE_INSTANCED_AT, SCENE_ALPHA_AT = 72, 128, 140


def test_walk_calls_reject_bad_arguments_before_any_device_work(nnbvh_lib):
    """NNBVH_ERR_ARG with a message that names the call.  Zeroed stand-ins serve where a handle must be non-NULL (the
    checks read `device` from both and the instancing, animation and alpha fields from the scene): nothing reaches a
    device."""
    fake_scene, fake_mesh = ctypes.create_string_buffer(1 << 16), ctypes.create_string_buffer(1 << 16)
    S, M = ctypes.addressof(fake_scene), ctypes.addressof(fake_mesh)
    soa = np.zeros(1, _lib.RAY_SOA_DTYPE)
    for k in ("ox", "oy", "oz", "dx", "dy", "dz", "tmax"):
        soa[k] = 64  # non-NULL, never read
    Q, A = soa.ctypes.data, 64

    def shadow(s=S, m=M, n=8, q=Q, npc=0, arrays=(A, A, A, A, A), npx=8, cap=4):
        return nnbvh_lib.nnbvh_wavefront_walk_shadow_tr(s, m, n, q, None, None, npc, *arrays, npx, None, cap, None, None)

    def one_random(s=S, m=M, n=8, arrays=(A, A, A), npm=0, outs=(A, A, A), cap=4):
        return nnbvh_lib.nnbvh_wavefront_walk_one_random(s, m, n, *arrays, None, None, npm, *outs, None, cap, None, None)

    for call, name in ((shadow, "wavefront_walk_shadow_tr"), (one_random, "wavefront_walk_one_random")):
        bad = [dict(s=None), dict(m=None), dict(cap=0), dict(cap=65537), dict(cap=-1), dict(n=-1)]
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
        # (empty queues: the refusals come before the size is looked at)
        for buf, fields, words in ((fake_mesh, ((0, 1),), "different devices"),
                                   (fake_scene, ((SCENE_INSTANCED_AT, 1), (SCENE_ANIM_AT, 64)), "AnimatedPrimitive"),
                                   (fake_scene, ((SCENE_ALPHA_AT, 1),), "alpha-tested"),
                                   (fake_scene, ((SCENE_ALPHA_AT, 2),), "alpha-tested")):
            for at, value in fields:
                ctypes.memmove(ctypes.addressof(buf) + at, ctypes.byref(ctypes.c_int64(value)), 8 if at % 8 == 0 else 4)
            assert call(n=0) == ERR_ARG, (name, words)
            assert _lib.last_error().startswith(name + ":") and words in _lib.last_error(), _lib.last_error()
            for at, _ in fields:
                ctypes.memset(ctypes.addressof(buf) + at, 0, 8 if at % 8 == 0 else 4)


def test_walk_calls_of_both_trees_refuse_common_bad_arguments_in_the_same_words(nnbvh_lib):
    """The bad arguments that need no per-type field: the BVH call and the kd-tree call of the same walk return
    NNBVH_ERR_ARG and set the same text behind their own name.  Zeroed stand-in handles: nothing reaches a device."""
    fake_scene, fake_mesh = ctypes.create_string_buffer(1 << 16), ctypes.create_string_buffer(1 << 16)
    S, M = ctypes.addressof(fake_scene), ctypes.addressof(fake_mesh)
    soa = np.zeros(1, _lib.RAY_SOA_DTYPE)
    for k in ("ox", "oy", "oz", "dx", "dy", "dz", "tmax"):
        soa[k] = 64  # non-NULL, never read
    nosoa = soa.copy()
    nosoa["dx"] = 0
    Q, A = soa.ctypes.data, 64

    def shadow(prefix, s=S, m=M, n=8, q=Q, npc=0, arrays=(A, A, A, A, A), npx=8, cap=4):
        fn = getattr(nnbvh_lib, f"nnbvh_{prefix}wavefront_walk_shadow_tr")
        return fn(s, m, n, q, None, None, npc, *arrays, npx, None, cap, None, None)

    def one_random(prefix, s=S, m=M, n=8, arrays=(A, A, A), npm=0, outs=(A, A, A), cap=4):
        fn = getattr(nnbvh_lib, f"nnbvh_{prefix}wavefront_walk_one_random")
        return fn(s, m, n, *arrays, None, None, npm, *outs, None, cap, None, None)

    common = [dict(s=None), dict(m=None), dict(cap=0), dict(cap=65537), dict(cap=-1), dict(n=-1)]
    cases = {shadow: common + [dict(npc=-1), dict(npx=-1), dict(q=None), dict(q=nosoa.ctypes.data)] +
             [dict(arrays=tuple(None if j == k else A for j in range(5))) for k in range(5)],
             one_random: common + [dict(npm=-1)] +
             [dict(arrays=tuple(None if j == k else A for j in range(3))) for k in range(3)] +
             [dict(outs=tuple(None if j == k else A for j in range(3))) for k in range(3)]}
    for call, walk in ((shadow, "wavefront_walk_shadow_tr"), (one_random, "wavefront_walk_one_random")):
        def refusal(prefix, **kw):
            assert call(prefix, **kw) == ERR_ARG, (prefix + walk, kw)
            name, _, text = _lib.last_error().partition(": ")
            assert name == prefix + walk and text, (_lib.last_error(), kw)
            return text

        texts = set()
        for kw in cases[call]:
            bvh, kd = refusal("", **kw), refusal("kd_", **kw)
            assert bvh == kd, (walk, kw, bvh, kd)
            texts.add(bvh)
        assert len(texts) == 5, texts  # no scene, no mesh, the cap, a negative size, a null array
        ctypes.memmove(ctypes.addressof(fake_mesh), ctypes.byref(ctypes.c_int32(1)), 4)  # the mesh on another device
        try:
            bvh, kd = refusal("", n=0), refusal("kd_", n=0)
        finally:
            ctypes.memset(ctypes.addressof(fake_mesh), 0, 4)
        assert bvh == kd and "different devices" in bvh and bvh not in texts


def test_max_surfaces_selects_the_walk_on_bvh_aggregates_only():
    pytest.importorskip("torch")
    from nn_bvh_amd.kdtree import KdTreeAggregate
    from nn_bvh_amd.wavefront import WavefrontAggregate

    class Handle:  # what WavefrontAggregate reads of a BVH aggregate before it refuses
        device = 0
        _h = None

    wf = WavefrontAggregate(Handle())
    with pytest.raises(NNBVHError, match="max_passes.*max_surfaces"):
        wf.IntersectShadowTr(0, None, None, None, None, None, None, None, max_passes=4, max_surfaces=4)
    with pytest.raises(NNBVHError, match="max_passes.*max_surfaces"):
        wf.IntersectOneRandom(0, None, None, None, None, max_passes=4, max_surfaces=4)
    with pytest.raises(NNBVHError, match="not offered for BVH scenes.*max_surfaces"):
        wf.WalkShadowTr(0, None, None, None, None, None, None, None)
    with pytest.raises(NNBVHError, match="not offered for BVH scenes.*max_surfaces"):
        wf.WalkOneRandom(0, None, None, None, None)
    kd = WavefrontAggregate(KdTreeAggregate(None, np.zeros(6, np.float32)))
    with pytest.raises(NNBVHError, match="not offered for kd-tree"):
        kd.IntersectShadowTr(0, None, None, None, None, None, None, None, max_surfaces=4)
    with pytest.raises(NNBVHError, match="not offered for kd-tree"):
        kd.IntersectOneRandom(0, None, None, None, None, max_surfaces=4)


def test_inputs_make_both_sides_of_every_cap_non_empty():
    """The preconditions of the GPU tests, from the composed reference alone."""
    s, r, a = bvh_layered_case(), bvh_one_random_case(), bvh_all_interface_case()
    tree = bvh_tree()
    assert len(tree.nodes) == 2099 and len(s.tris) == 1127
    assert np.array_equal(np.bincount(s.calls), [62, 2587, 1696, 905, 469, 183, 77, 20, 1])
    assert ((s.state == 0).sum(), (s.state == 1).sum()) == (2942, 3058)
    assert np.array_equal(np.bincount(r.calls), [60, 484, 674, 589, 500, 323, 223, 115, 32])
    assert abs((r.hits["prim"] >= 0).mean() - 0.496) < 0.001
    # per item identical to the kd tree's
    ks, kr, ka = layered_case(), one_random_case(), all_interface_case()
    assert np.array_equal(s.state, ks.state) and np.array_equal(s.calls, ks.calls)
    assert np.array_equal(r.calls, kr.calls) and np.array_equal(r.hits["prim"], kr.hits["prim"])
    assert np.array_equal(a.state, ka.state) and np.array_equal(a.calls, ka.calls)
    for c in (s, r):
        assert c.calls.max() == 8
        for cap in (1, 2, 3, 7):
            assert 0 < (c.calls > cap).sum() < c.n
        assert (c.calls > 8).sum() == 0
    # the small shapes
    assert a.calls[0] == 6 and a.calls.max() == 8 and (a.state == 0).all()
    assert [int((a.calls[:k] > 2).sum()) for k in (1, 63, 64, 65, 130, 257)] == [1, 39, 40, 40, 84, 164]


def test_spill_case_reenters_after_the_stack_went_through_the_spill():
    c = spill_case()
    both = (c.depth == 64) & (c.calls >= 2)
    print(f"depth 64: {(c.depth == 64).sum()} of {c.n}, calls histogram {np.bincount(c.calls)}, both {both.sum()}")
    assert both.sum() > 20 and c.calls.max() <= 64 and c.n % 64 != 0
    assert (c.state == 0).all()  # every class is interface: nothing blocks


# ---- GPU ----------------------------------------------------------------------------------------------------------
class ShadowDevice:
    """A shadow case on the device: BVH scene, mesh, queue and per-ray arrays."""

    def __init__(self, c, n=None, cls=None, tree=None):
        import torch
        from nn_bvh_amd import BVHAggregate
        from nn_bvh_amd.interaction import ShadingMesh
        from nn_bvh_amd.wavefront import RayQueue, WavefrontAggregate
        self.c, self.dev, self.n = c, torch.device("cuda", 0), c.n if n is None else n
        nodes, prims = tree if tree is not None else (c.tree.nodes, c.tree.ordered_prims)
        self.agg = BVHAggregate.from_tree(nodes, prims, c.verts)
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

    def run(self, cap=None, passes=None, L=None, state=None):
        import torch
        L = self.t(self.c.L0[:self.n]) if L is None else L
        state = torch.full((self.n,), SENTINEL, dtype=torch.uint8, device=self.dev) if state is None else state
        self.unfinished.fill_(-3)
        self.wf.IntersectShadowTr(self.n, self.q, self.mesh, self.Ld, self.ru, self.rl, self.pixel, L, state,
                                  max_surfaces=cap, max_passes=passes, unfinished=self.unfinished)
        torch.cuda.synchronize()
        return state.cpu().numpy(), L.cpu().numpy(), int(self.unfinished.item())

    def close(self):
        self.agg.close()
        self.mesh.close()


class OneRandomDevice:
    def __init__(self, c):
        import torch
        from nn_bvh_amd import BVHAggregate
        from nn_bvh_amd.interaction import ShadingMesh
        from nn_bvh_amd.wavefront import WavefrontAggregate
        self.c, self.dev = c, torch.device("cuda", 0)
        self.agg = BVHAggregate.from_tree(c.tree.nodes, c.tree.ordered_prims, c.verts)
        self.mesh = ShadingMesh(c.verts, c.tris)
        self.wf = WavefrontAggregate(self.agg)
        self.t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        self.p0, self.p1, self.material = self.t(c.p0), self.t(c.p1), self.t(c.material)
        self.prim_material = self.t(c.prim_material)
        self.size = torch.full((1,), c.n, dtype=torch.int32, device=self.dev)
        self.unfinished = torch.full((1,), -3, dtype=torch.int32, device=self.dev)

    def call(self, cap=None, passes=None):
        return self.wf.IntersectOneRandom(self.c.n, self.p0, self.p1, self.material, self.mesh, self.prim_material,
                                          size=self.size, max_surfaces=cap, max_passes=passes,
                                          unfinished=self.unfinished)

    def run(self, cap=None, passes=None):
        import torch
        self.unfinished.fill_(-3)
        out = self.call(cap, passes)
        torch.cuda.synchronize()
        return one_random_numpy(out) + (int(self.unfinished.item()),)

    def close(self):
        self.agg.close()
        self.mesh.close()


@pytest.mark.gpu
def test_gpu_shadow_walk_equals_the_composed_bvh_reference():
    import torch
    c = bvh_layered_case()
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
    wf0.IntersectShadowTr(c.n, d.q, d.mesh, d.Ld, d.ru, d.rl, d.pixel, d.t(c.L0), st0, max_surfaces=UNCAPPED,
                          unfinished=d.unfinished)
    torch.cuda.synchronize()
    live = (c.rays["d"] != 0).any(1)
    occ = d.agg.IntersectP(c.rays)
    assert np.array_equal(st0.cpu().numpy()[live], occ[live]) and 0.05 < occ[live].mean() < 0.95
    assert (st0.cpu().numpy()[~live] == 0).all() and int(d.unfinished.item()) == 0
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [1, 2, 3, 7, 8])
def test_gpu_shadow_walk_stops_at_max_surfaces(cap):
    c = bvh_layered_case()
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
    # ... and the bounded pass form of the same scene leaves the same outputs
    b_state, b_L, b_unfinished = d.run(passes=cap)
    assert np.array_equal(state, b_state) and L.tobytes() == b_L.tobytes() and unfinished == b_unfinished
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [UNCAPPED, 1, 3])
def test_gpu_one_random_walk_equals_the_composed_bvh_reference(cap):
    c = bvh_one_random_case()
    d = OneRandomDevice(c)
    got = d.run(cap)
    left = check_one_random(c, got, cap)
    print(f"max_surfaces {cap}: unfinished {got[4]} (reference {left})")
    assert left == int((c.calls > cap).sum()) and (left == 0) == (cap == UNCAPPED)
    assert got[4] == left
    if cap <= 64:  # the bounded pass form: the same marks, and the same outputs for the items it finishes
        ref = d.run(passes=cap)
        assert check_one_random(c, ref, cap) == left == ref[4]
        fin = c.calls <= cap
        assert np.array_equal(got[0]["instance"] == -1, ref[0]["instance"] == -1)
        for a, b in zip(got[:4], ref[:4]):
            assert a[fin].tobytes() == b[fin].tobytes()
    else:  # ... and under a device-side size
        d.size.fill_(c.n // 2)
        got = d.run(cap)
        assert check_one_random(c, got, cap, c.n // 2) == 0 and got[4] == 0
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n,size", [(1, None), (63, None), (64, None), (65, None), (257, 130)])
def test_gpu_shadow_walk_small_shapes(n, size):
    """The smallest shapes at which the in-lane continuation can go wrong: one continuing lane beside 63 idle ones on
    an exhausted queue, a full wave, a second wave with one lane, and a device-side size inside a wave."""
    c = bvh_all_interface_case()
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
def test_gpu_walk_reenters_the_tree_after_a_stack_spill():
    c = spill_case()
    d = ShadowDevice(c, tree=(c.nodes, c.prims))
    ref_state, ref_L, ref_left = d.run(passes=64)
    exp_L = shadow_radiance(c.state, c.Ld, c.ru, c.rl, c.pixel, c.L0)
    assert np.array_equal(ref_state, c.state) and ref_L.tobytes() == exp_L.tobytes() and ref_left == 0
    state, L, left = d.run(UNCAPPED)
    assert np.array_equal(state, ref_state) and L.tobytes() == ref_L.tobytes() and left == 0
    for cap in (1, 2):
        ref_state, ref_L, ref_left = d.run(passes=cap)
        state, L, left = d.run(cap)
        assert np.array_equal(state, ref_state) and L.tobytes() == ref_L.tobytes(), cap
        assert left == ref_left == int((c.calls > cap).sum()), cap
    d.close()


@pytest.mark.gpu
def test_gpu_walk_calls_are_hip_graph_capturable():
    """Both walk calls in ONE captured graph (a linear chain of kernel nodes); between the replays the queue contents
    and the device-side sizes are rewritten in place, and each replay equals the reference for the inputs it saw."""
    import torch
    c, r = bvh_layered_case(), bvh_one_random_case()
    d, e = ShadowDevice(c), OneRandomDevice(r)
    L0 = d.t(c.L0)
    L = L0.clone()
    state = torch.full((c.n,), SENTINEL, dtype=torch.uint8, device=d.dev)
    side = torch.cuda.Stream(d.dev)
    torch.cuda.synchronize()

    def step():
        d.wf.IntersectShadowTr(c.n, d.q, d.mesh, d.Ld, d.ru, d.rl, d.pixel, L, state, max_surfaces=UNCAPPED,
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
# (device_shadow_walk / device_one_random_walk of the kd test: host loops over the aggregate's Intersect, the
# interaction post-pass and ob.offset_batch; a BVHAggregate serves them as a KdTreeAggregate does)
# case -> (kernel family, the instances its device calls launch), asserted with the launch ledger (tests/ledger_cases.py).
# pick_walk_instance gives the walks <4,8,INST,1> / <5,8,INST,1> (form 1, or 2 in the two-level scene); the unbounded
# and bounded calls and the host loops over Intersect that compose the expected values run the closest-hit form of
# the same scene, <0,8,INST,1>
LEDGER = {
    "test_gpu_walks_beyond_flat_triangles[patch_scene]": (BVH, bvh((0, 4, 5))),
    "test_gpu_walks_beyond_flat_triangles[host_prim_scene]": (BVH, bvh((0, 4, 5))),
    "test_gpu_walks_beyond_flat_triangles[two_level_case]": (BVH, bvh((0, 4, 5), inst=1)),
}


@pytest.mark.gpu
@pytest.mark.parametrize("make", [patch_scene, host_prim_scene, two_level_case])
def test_gpu_walks_beyond_flat_triangles(make):
    import torch
    from nn_bvh_amd import BVHAggregate
    from nn_bvh_amd.interaction import ShadingMesh
    from nn_bvh_amd.wavefront import RayQueue, WavefrontAggregate
    s = make()
    start = ledger_start(LEDGER, f"test_gpu_walks_beyond_flat_triangles[{make.__name__}]")
    nodes, prims, verts = s["tree"]
    mesh = ShadingMesh(verts, **s["mesh"])
    if "instances" in s:
        mesh.set_instances(s["instances"])
        agg = BVHAggregate.from_tree(nodes, prims, verts, instances=s["instances"], n_top_nodes=s["n_top"])
    else:
        agg = BVHAggregate.from_tree(nodes, prims, verts)
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

    def shadow(cap=None, passes=None):
        L, state = t(L0), torch.full((n,), SENTINEL, dtype=torch.uint8, device=dev)
        unfinished.fill_(-3)
        wf.IntersectShadowTr(n, q, mesh, t(Ld), t(ru), t(rl), t(pixel), L, state, max_surfaces=cap, max_passes=passes,
                             unfinished=None if cap is None and passes is None else unfinished)
        torch.cuda.synchronize()
        return state.cpu().numpy(), L.cpu().numpy(), int(unfinished.item())

    ref_state, ref_L, _ = shadow()
    assert min((ref_state == 0).sum(), (ref_state == 1).sum()) > 20
    if make is host_prim_scene:
        assert (ref_state == 2).sum() > 20
    for got in (shadow(passes=16), shadow(UNCAPPED)):
        assert np.array_equal(got[0], ref_state) and got[1].tobytes() == ref_L.tobytes() and got[2] == 0
    host_state, calls = device_shadow_walk(agg, mesh, rays, cls)
    assert np.array_equal(host_state, ref_state) and (calls > 1).sum() > 20
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
    args = (m, t(p0), t(p1), t(material), mesh, t(prim_material))

    def one_random(cap=None, passes=None):
        unfinished.fill_(-3)
        out = wf.IntersectOneRandom(*args, max_surfaces=cap, max_passes=passes,
                                    unfinished=None if cap is None and passes is None else unfinished)
        torch.cuda.synchronize()
        return one_random_numpy(out), int(unfinished.item())

    ref, _ = one_random()
    own = ref[0]["instance"] != -1  # the others: a host-only primitive lies on the segment
    assert (ref[0]["prim"][own] >= 0).sum() > 20
    if make is host_prim_scene:
        assert (~own).sum() > 20
    if make is two_level_case:
        assert (ref[0]["instance"][own & (ref[0]["prim"] >= 0)] > 0).sum() > 20  # selected hits inside instances
    for got, left in (one_random(passes=16), one_random(UNCAPPED)):
        assert left == 0
        for a, b in zip(got, ref):
            assert a.tobytes() == b.tobytes()
    eh, er, epdf, ewsum, ecalls, host = device_one_random_walk(agg, mesh, p0, p1, material, prim_material)
    assert np.array_equal(host, ~own) and (ecalls > 1).sum() > 20
    sel = own & (eh["prim"] >= 0)
    assert np.array_equal(ref[0]["prim"][own], eh["prim"][own])
    assert ref[0][sel].tobytes() == eh[sel].tobytes() and ref[1][sel].tobytes() == er[sel].tobytes()
    assert np.array_equal(ref[2][own].view(np.uint32), epdf[own].view(np.uint32))
    assert np.array_equal(ref[3][own].view(np.uint32), ewsum[own].view(np.uint32))
    got, left = one_random(1)
    # an item the first call already hands to the caller (a host-only primitive) is marked, not counted
    assert left == (ecalls > 1).sum()
    fin = own & (ecalls <= 1)
    assert np.array_equal(got[0]["instance"] == -1, ~fin)
    for a, b in zip(got, ref):
        assert a[fin].tobytes() == b[fin].tobytes()
    agg.close()
    mesh.close()
    assert_reached(LEDGER, f"test_gpu_walks_beyond_flat_triangles[{make.__name__}]", start)
