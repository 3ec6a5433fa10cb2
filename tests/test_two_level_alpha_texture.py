"""Image-textured alpha (primitive kinds 16 .. 19) in two-level scenes: nnbvh_scene_create_instanced_with_alpha_textures
(host-built trees) and nnbvh_scene_create_instanced_gpu_build_with_alpha_textures (every tree built on the device),
their argument checks, the premise of the oracle's construction (tests/two_level_alpha_oracle.py) and the device
kernels against it.  Every result comparison is bytes against the oracle: hit records, occluded, nodes visited and
primitive tests, no ray left out."""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import alpha_texture_oracle as ato
import oracle_binding as ob
import scenes_small as ss
import two_level_alpha_oracle as tlo
from ledger_cases import BVH, assert_reached, ledger_start
from nn_bvh_amd import AlphaTexture, BVHAggregate, NNBVHError, _lib, build_tree, scene
from nn_bvh_amd._lib import ptr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_CALLS = ("nnbvh_scene_create_instanced_with_alpha_textures", "nnbvh_scene_create_instanced_gpu_build_with_alpha_textures")
NO_DEVICE = 1 << 20  # a device index no machine has: a well-formed call gets as far as the device check
F = np.float32
N_RAYS = 3000


# ---- the scene -----------------------------------------------------------------------------------------------------------
def rigid_scaled(rng, shift, scale=(0.7, 1.3)):
    """(render_from_prim 3x4, prim_from_render 3x4): a random rotation, a scale per axis, a translation within +-shift"""
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    m = np.eye(4)
    m[:3, :3] = q * rng.uniform(*scale, 3)[None, :]
    m[:3, 3] = rng.uniform(-shift, shift, 3)
    return m[:3].astype(F).reshape(12), np.linalg.inv(m)[:3].astype(F).reshape(12)


def parts(seed=11):
    """Object 0: 48 triangles of kinds 0, 4 .. 7 and 16 .. 19; object 1: 16 plain triangles and six alpha-tested patches
    (kinds 8 / 12); six textured triangles for the top-level list.  Ids are unique over the scene."""
    rng = np.random.default_rng(seed)
    v0, p0 = ss.random_soup(48, 0, seed, extent=1.5, size=1.0)
    v1, p1 = ss.random_soup(16, 6, seed + 1, extent=1.5, size=0.7)
    v2, p2 = ss.random_soup(6, 0, seed + 2, extent=4.0, size=3.0)
    p0, p1, p2 = p0.copy(), p1.copy(), p2.copy()
    kinds = np.array([0, 4, 5, 6, 7, 16, 17, 18, 19])[np.arange(len(p0)) % 9]
    p0["kind"] = kinds
    const = (kinds >= 4) & (kinds <= 7)
    p0["v"][:, 3] = np.where(const, ss.ALPHAS[np.arange(len(p0)) % len(ss.ALPHAS)].view(np.int32),
                             np.where(kinds >= 16, (np.arange(len(p0)) // 9) % 3, 0))
    quads = np.nonzero(p1["kind"] == 1)[0]
    p1["kind"][quads] = np.array([8, 12])[np.arange(len(quads)) % 2]
    p1["v"][p1["kind"] == 0, 3] = 0
    p1["v"] += len(v0)
    p1["id"] += len(p0)
    p2["kind"] = 16 + np.arange(len(p2)) % 4
    p2["v"][:, 3] = np.arange(len(p2)) % 3
    p2["v"][:, :3] += len(v0) + len(v1)
    p2["id"] += len(p0) + len(p1)
    verts = np.concatenate([v0, v1, v2]).astype(F)
    normals = rng.normal(size=(len(verts), 3)).astype(F)
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    uvs = rng.uniform(-0.5, 1.5, (len(verts), 2)).astype(F)
    alpha_by_id = rng.choice(ss.ALPHAS, len(p0) + len(p1) + len(p2)).astype(F)
    return verts, p0, p1, p2, normals, uvs, alpha_by_id


@functools.lru_cache(None)
def static_scene(with_uvs=True, max_prims=4, split="sah"):
    """five placements of object 0 that overlap in space (translations within +-0.6 of an object 3 wide), two of
    object 1"""
    verts, p0, p1, p2, normals, uvs, alpha_by_id = parts()
    if not with_uvs:  # a scene without (u, v) cannot hold the patches that read them
        p1 = p1.copy()
        p1["kind"][p1["kind"] == 12] = 8
    rng = np.random.default_rng(5)
    placements = [(0,) + rigid_scaled(rng, 0.6) for _ in range(5)] + [(1,) + rigid_scaled(rng, 2.0) for _ in range(2)]
    return tlo.Scene(p2, verts, [p0, p1], placements, normals, uvs if with_uvs else None, ato.scene_textures(0),
                     alpha_by_id, max_prims, split, None, None, None)


def hand_made_animation(rng, shift):
    """An AnimatedTransform whose decomposition is exact by construction: M(t) = T(t) R(t) S with S a diagonal scale,
    R from the identity to a turn of 0.2 .. 0.6 rad about a random axis, T moving by up to 0.5.  Returns the
    _lib.ANIMATED_DTYPE record (time range 0 .. 1)."""
    def compose(t, q, s):
        x, y, z, w = q
        r = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                      [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        m = np.eye(4)
        m[:3, :3] = r @ np.diag(s)
        m[:3, 3] = t
        return m
    a = np.zeros(1, _lib.ANIMATED_DTYPE)[0]
    s = rng.uniform(0.7, 1.3, 3)
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    half = rng.uniform(0.1, 0.3)
    q0, q1 = np.array([0, 0, 0, 1.0]), np.concatenate([axis * np.sin(half), [np.cos(half)]])
    t0 = rng.uniform(-shift, shift, 3)
    t1 = t0 + rng.uniform(-0.5, 0.5, 3)
    m0, m1 = compose(t0, q0, s), compose(t1, q1, s)
    a["start_from"], a["end_from"] = m0.astype(F).reshape(16), m1.astype(F).reshape(16)
    a["start_inv"], a["end_inv"] = np.linalg.inv(m0).astype(F).reshape(16), np.linalg.inv(m1).astype(F).reshape(16)
    a["T"], a["R"] = np.stack([t0, t1]).astype(F), np.stack([q0, q1]).astype(F)
    sm = np.eye(4)
    sm[:3, :3] = np.diag(s)
    a["S"] = np.stack([sm, sm]).astype(F).reshape(2, 16)
    a["start_time"], a["end_time"], a["actually_animated"] = 0.0, 1.0, 1
    return a


def oracle_anims(anims):
    oa = np.zeros(len(anims), ob.ANIM_DTYPE)
    for f_o, f_p in (("start_m", "start_from"), ("start_minv", "start_inv"), ("end_m", "end_from"), ("end_minv", "end_inv")):
        oa[f_o] = anims[f_p]
    for f in ("T", "R", "S", "start_time", "end_time", "actually_animated"):
        oa[f] = anims[f]
    return oa


@functools.lru_cache(None)
def animated_scene():
    """five placements of object 0, three of them actually animated; the instance entries of those take bounds that
    cover the motion (the union of the transformed root box at 33 times, padded: MotionBounds stay the caller's)"""
    verts, p0, p1, p2, normals, uvs, alpha_by_id = parts()
    rng = np.random.default_rng(8)
    anims = np.zeros(5, _lib.ANIMATED_DTYPE)
    placements = []
    for j in range(5):
        anims[j] = hand_made_animation(rng, 0.6)
        anims[j]["actually_animated"] = int(j in (0, 2, 3))
        placements.append((0, anims[j]["start_from"][:12].copy(), anims[j]["start_inv"][:12].copy()))
    oa = oracle_anims(anims)
    root = build_tree(p0, verts, 4).nodes[0]
    box = np.concatenate([root["pmin"], root["pmax"]])
    motion = np.zeros((5, 6), F)
    for j in range(5):
        if not anims[j]["actually_animated"]:
            continue
        lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
        for t in np.linspace(0, 1, 33):
            m = ob.anim_interpolate(oa[j:j + 1], [t])[0, :16].reshape(4, 4)
            b = tlo.instancing.transform_bounds(m[:3].reshape(12), box)
            lo, hi = np.minimum(lo, b[:3]), np.maximum(hi, b[3:])
        pad = 0.05 * (hi - lo) + 1e-3
        motion[j] = np.concatenate([lo - pad, hi + pad])
    return tlo.Scene(p2, verts, [p0], placements, normals, uvs, ato.scene_textures(0), alpha_by_id, 4, "sah", anims, oa,
                     motion)


def scene_rays(seed=21, n=N_RAYS, times=False):
    rays = np.concatenate([scene.random_rays(n - n // 6, [-3, -3, -3], [3, 3, 3], seed),
                           scene.random_rays(n // 6, [-3, -3, -3], [3, 3, 3], seed + 1, tmax=F(0.6))])
    if times:  # below, inside and above the time range 0 .. 1
        rays["time"] = np.random.default_rng(seed + 2).uniform(-0.3, 1.3, n).astype(F)
    return rays


class Case:
    """a scene, its rays, and the oracle's answers, computed once"""

    def __init__(self, s, rays):
        self.s, self.rays = s, rays
        self.oracle = tlo.TwoLevelOracle(s, rays)
        self.closest = self.oracle.closest()
        self.any_hit = self.oracle.any_hit()
        self.opaque = self.oracle.closest(self.oracle.mid_opaque())
        self.kind_of_id = np.zeros(len(s.alpha_by_id), np.int32)
        for p in [s.top] + list(s.objects):
            self.kind_of_id[p["id"]] = p["kind"]

    # the conditions on the inputs, from the oracle alone
    def hit_kind(self):
        return np.where(self.closest["prim"] >= 0, self.kind_of_id[np.maximum(self.closest["prim"], 0)], -1)

    def rejected_by_hash(self):
        """rays on which a textured hit with 0 < a < 1 was rejected: the record (its prim_tests at least) differs from
        the one with those alphas turned 1"""
        return np.array([self.closest[i].tobytes() != self.opaque[i].tobytes() for i in range(len(self.rays))])

    def accepted_behind_rejected(self):
        """an accepted textured hit at a larger t than a rejected one: with the mid alphas opaque the ray stops earlier"""
        return (self.hit_kind() >= 16) & (self.opaque["prim"] >= 0) & (self.opaque["t"] < self.closest["t"])

    def two_placements(self):
        """rays whose line meets the same object triangle through two placements with different alpha"""
        o = self.oracle
        out = np.zeros(len(self.rays), bool)
        for src in np.unique(o.src[o.seg >= 0]):
            cols = np.nonzero((o.src == src) & (o.seg >= 0))[0]
            for x in range(len(cols)):
                for y in range(x + 1, len(cols)):
                    a, b = cols[x], cols[y]
                    out |= o.met[:, a] & o.met[:, b] & (o.alpha[:, a] != o.alpha[:, b])
        return out


@functools.lru_cache(None)
def case(name, with_uvs=True, max_prims=4, split="sah"):
    if name == "animated":
        return Case(animated_scene(), scene_rays(31, times=True))
    return Case(static_scene(with_uvs, max_prims, split), scene_rays())


# ---- CPU: the oracle's premise -------------------------------------------------------------------------------------------
def constant_alpha(s):
    """the scene with its textured kinds rewritten to constant ones (16 .. 19 -> 4 .. 7, alpha by id)"""
    def const(p):
        p = p.copy()
        t = ato.is_textured(p["kind"])
        p["kind"][t] -= 12
        p["v"][t, 3] = np.asarray(s.alpha_by_id, F)[p["id"][t]].view(np.int32)
        return p
    return s._replace(top=const(s.top), objects=[const(o) for o in s.objects])


@pytest.mark.parametrize("name", ["static", "animated"])
def test_one_copy_per_placement_gives_the_shared_forms_bytes(name):
    """the premise of tests/two_level_alpha_oracle.py: on a constant-alpha scene the oracle's closest hits, occlusion
    flags and both counters are the same bytes for the shared object and for one copy of it per placement"""
    s = constant_alpha(static_scene() if name == "static" else animated_scene())
    rays = scene_rays(41, times=name == "animated")
    shared, copied = tlo.shared_form(s), tlo.copied_form(s)
    assert len(copied[0]) > len(shared[0]) and len(copied[1]) > len(shared[1])  # the forms do differ
    n_top = shared[3]
    assert copied[3] == n_top and copied[0][:n_top].tobytes() == shared[0][:n_top].tobytes()  # the same top-level tree
    if name == "static":  # ... and assemble is instancing.assemble_two_level
        ref = tlo.instancing.assemble_two_level(s.top, s.verts, s.objects, s.placements, s.max_prims, s.split)
        assert all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(shared[:4], ref))
    out = []
    for nodes, prims, instances, _, _ in (shared, copied):
        try:
            ob.set_vertex_normals(s.normals)
            ob.set_vertex_uvs(s.uvs)
            ob.set_prim_alpha(tlo.ordered_alpha(s, prims))
            ob.set_sin_mode(1)
            if name == "static":
                out.append((ob.closest_inst(nodes, prims, s.verts, instances, rays),
                            ob.any_hit_inst(nodes, prims, s.verts, instances, rays)))
            else:
                out.append((ob.closest_anim(nodes, prims, s.verts, instances, s.oa, rays),
                            ob.any_hit_anim(nodes, prims, s.verts, instances, s.oa, rays)))
        finally:
            ob.set_sin_mode(0)
            ob.set_vertex_normals(None)
            ob.set_vertex_uvs(None)
            ob.set_prim_alpha(None)
    (h0, a0), (h1, a1) = out
    assert h0.tobytes() == h1.tobytes()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a0, a1))
    assert (h0["instance"] > 0).sum() > 500 and len(np.unique(h0["instance"])) >= len(s.placements)
    assert (a0[0] == 1).sum() > 500 and (a0[0] == 0).sum() > 100


def test_the_oracle_alone_meets_the_conditions_on_the_inputs():
    c = case("static")
    kinds, inside = c.hit_kind(), c.closest["instance"] > 0
    counts = {k: int((inside & (kinds == k)).sum()) for k in (16, 17, 18, 19)}
    rejected, two, behind = c.rejected_by_hash().sum(), c.two_placements().sum(), c.accepted_behind_rejected().sum()
    print("accepted inside an instance", counts, "rejected by the hash", rejected, "two placements", two,
          "accepted behind a rejected one", behind, "top-level textured hits", int((~inside & (kinds >= 16)).sum()))
    assert min(counts.values()) > 20 and rejected > 20 and two > 20 and behind > 20
    assert (~inside & (kinds >= 16)).sum() > 5 and (kinds == 8).sum() + (kinds == 12).sum() > 5
    c = case("animated")
    an = c.s.anims
    moving = (c.closest["instance"] > 0) & (an["actually_animated"][np.maximum(c.closest["instance"] - 1, 0)] != 0)
    within = (c.rays["time"] > 0) & (c.rays["time"] < 1)
    n = int((c.accepted_behind_rejected() & moving & within).sum())
    print("animated: accepted behind a rejected one, inside a moving placement at a time inside its range", n)
    assert n > 20 and (c.rays["time"] < 0).sum() > 100 and (c.rays["time"] > 1).sum() > 100


# ---- CPU: exports, argument faults, refusals ---------------------------------------------------------------------------
def test_calls_are_exported_prototyped_and_declared(nnbvh_lib):
    header = open(os.path.join(ROOT, "include", "nnbvh.h")).read()
    for name in NEW_CALLS:
        assert name in _lib.EXPORTS and hasattr(nnbvh_lib, name)
        assert re.search(r"nnbvh_scene \*" + name + r"\(", header), name
        assert getattr(nnbvh_lib, name).restype is ctypes.c_void_p
    assert len(nnbvh_lib.nnbvh_scene_create_instanced_with_alpha_textures.argtypes) == 16
    assert len(nnbvh_lib.nnbvh_scene_create_instanced_gpu_build_with_alpha_textures.argtypes) == 19
    assert "flat scenes only" not in header.lower()
    adapter = open(os.path.join(ROOT, "include", "nnbvh_aggregate.hpp")).read()
    assert all(name in adapter for name in NEW_CALLS)


def raw_create(L, route, s, top=None, objects=None, textures="scene", n_textures=None, normals="scene", device=NO_DEVICE):
    top = s.top if top is None else top
    objects = s.objects if objects is None else objects
    s = s._replace(top=top, objects=objects)
    table, n = _lib.alpha_texture_table(s.textures) if isinstance(textures, str) else (
        (None, 0) if textures is None else _lib.alpha_texture_table(textures))
    n = n if n_textures is None else n_textures
    nrm = s.normals if isinstance(normals, str) else normals
    opt = lambda a: ptr(a) if a is not None else None  # noqa: E731
    if route == "host_tree":
        nodes, prims, instances, n_top, _ = tlo.shared_form(s)
        alpha = tlo.ordered_alpha(s, prims)
        return L.nnbvh_scene_create_instanced_with_alpha_textures(
            ptr(nodes), len(nodes), n_top, ptr(prims), len(prims), ptr(s.verts), len(s.verts), ptr(instances),
            len(instances), None, opt(nrm), opt(s.uvs), ptr(alpha), device, table, n)
    entries, n_top, first = BVHAggregate.two_level_entries(s.top, s.objects, s.placements)
    pl = np.zeros(len(s.placements), _lib.PLACEMENT_DTYPE)
    for j, (k, m, mi) in enumerate(s.placements):
        pl[j]["render_from_prim"], pl[j]["prim_from_render"], pl[j]["object"] = m, mi, k
    alpha = np.ascontiguousarray(np.asarray(s.alpha_by_id, F)[entries["id"]])
    return L.nnbvh_scene_create_instanced_gpu_build_with_alpha_textures(
        ptr(entries), len(entries), n_top, ptr(first), len(s.objects), ptr(s.verts), len(s.verts), opt(nrm), opt(s.uvs),
        ptr(alpha), None, ptr(pl), len(pl), None, 4, 0, device, table, n)


@pytest.mark.parametrize("route", ["host_tree", "device_build"])
def test_argument_faults_name_the_call_before_any_device_work(nnbvh_lib, route):
    L = nnbvh_lib
    call = NEW_CALLS[0 if route == "host_tree" else 1]
    s = static_scene()
    good = list(s.textures)

    def refused(words, **kw):
        assert not raw_create(L, route, s, **kw), words
        err = _lib.last_error()
        assert call in err and words in err, (words, err)

    # a well-formed call (textured triangles in an object and in the top-level list, alpha-tested patches beside them)
    # gets as far as the device check
    assert not raw_create(L, route, s) and "no usable HIP device" in _lib.last_error()
    refused("need the alpha-texture table", textures=None)
    refused("null alpha-texture table", n_textures=2, textures=None)
    for where in ("object", "top"):
        for bad_index in (3, -1):
            top, obj = s.top.copy(), s.objects[0].copy()
            target = obj if where == "object" else top
            target["v"][np.nonzero(ato.is_textured(target["kind"]))[0][0], 3] = bad_index
            refused("alpha-texture index out of range", top=top, objects=[obj, s.objects[1]])
    bad = AlphaTexture(np.ones((2, 3), F))
    bad.texels = None
    refused("null texels", textures=[good[0], good[1], bad])
    for w, h in ((0, 1), (1, 0), (-3, 2), ((1 << 24) + 1, 1), (1, (1 << 24) + 1)):
        bad = AlphaTexture(np.ones((2, 3), F))
        bad.width, bad.height = w, h
        refused("width and height must be 1 .. 2^24", textures=[bad, good[1], good[2]])
    for wrap in (3, -1, 7):
        refused("unknown wrap mode", textures=[good[0], good[1], AlphaTexture(np.ones((2, 3), F), wrap=wrap)])
    refused("need the vertex normals", normals=None)  # kinds 18 / 19 are in the scene


def test_the_other_instanced_calls_keep_refusing_the_textured_kinds(nnbvh_lib):
    L = nnbvh_lib
    s = static_scene()
    nodes, prims, instances, n_top, _ = tlo.shared_form(s)
    alpha = tlo.ordered_alpha(s, prims)
    two_level_calls = " / ".join(NEW_CALLS)
    flat_calls = "nnbvh_scene_create_with_alpha_textures / nnbvh_scene_create_gpu_build_with_alpha_textures"
    kd_calls = "nnbvh_kd_scene_create_with_alpha_textures / nnbvh_kd_scene_create_gpu_build_with_alpha_textures"
    head = (ptr(nodes), len(nodes), n_top, ptr(prims), len(prims), ptr(s.verts), len(s.verts), ptr(instances), len(instances))
    assert not L.nnbvh_scene_create_instanced(*head, NO_DEVICE)
    err = _lib.last_error()
    assert "unknown primitive kind" in err and two_level_calls in err and flat_calls in err and kd_calls in err
    assert not L.nnbvh_scene_create_instanced_animated(*head, None, NO_DEVICE)
    assert two_level_calls in _lib.last_error()
    assert not L.nnbvh_scene_create_instanced_with_attributes(*head, None, ptr(s.normals), ptr(s.uvs), ptr(alpha), NO_DEVICE)
    assert two_level_calls in _lib.last_error()
    with pytest.raises(NNBVHError, match="nnbvh_scene_create_instanced_gpu_build_with_alpha_textures"):
        BVHAggregate.build_two_level_on_device(s.top, s.verts, s.objects, s.placements, normals=s.normals, uvs=s.uvs,
                                               prim_alpha=entries_alpha(s), device=NO_DEVICE)
    with pytest.raises(NNBVHError, match="unknown primitive kind"):
        BVHAggregate.from_tree(nodes, prims, s.verts, instances=instances, n_top_nodes=n_top, normals=s.normals, uvs=s.uvs,
                               prim_alpha=alpha, device=NO_DEVICE)
    # the new host-tree call is for two-level scenes; flat scenes keep refusing the mix with alpha-tested patches
    assert not L.nnbvh_scene_create_instanced_with_alpha_textures(*head[:7], None, 0, None, ptr(s.normals), ptr(s.uvs),
                                                                  ptr(alpha), NO_DEVICE, *_lib.alpha_texture_table(s.textures))
    assert NEW_CALLS[0] in _lib.last_error() and "instance table" in _lib.last_error()
    mixed = np.concatenate([s.objects[0], s.objects[1]])
    with pytest.raises(NNBVHError, match="alpha-tested patches"):
        BVHAggregate.build_on_device(mixed, s.verts, normals=s.normals, uvs=s.uvs, prim_alpha=np.ones(len(mixed), F),
                                     alpha_textures=s.textures, device=NO_DEVICE)


def entries_alpha(s):
    entries, _, _ = BVHAggregate.two_level_entries(s.top, s.objects, s.placements)
    return np.ascontiguousarray(np.asarray(s.alpha_by_id, F)[entries["id"]])


def make_aggregate(s, route, device=0, **over):
    kw = dict(normals=s.normals, uvs=s.uvs, alpha_textures=s.textures, animated=s.anims, device=device)
    if route == "host_tree":
        nodes, prims, instances, n_top, _ = tlo.shared_form(s)
        kw.update(prim_alpha=tlo.ordered_alpha(s, prims), instances=instances, n_top_nodes=n_top)
        kw.update(over)
        return BVHAggregate.from_tree(nodes, prims, s.verts, **kw)
    bounds = None
    if s.anims is not None:
        n_top, n_all = len(s.top), len(s.top) + len(s.placements) + sum(len(o) for o in s.objects)
        bounds = np.zeros((n_all, 6), F)
        bounds[n_top:n_top + len(s.placements)] = s.motion
    kw.update(prim_alpha=entries_alpha(s), prim_bounds=bounds)
    kw.update(over)
    return BVHAggregate.build_two_level_on_device(s.top, s.verts, s.objects, s.placements, s.max_prims, s.split, **kw)


@pytest.mark.parametrize("route", ["host_tree", "device_build"])
def test_python_front_end_checks_its_arguments(route):
    s = static_scene()
    with pytest.raises(NNBVHError, match="no usable HIP device"):
        make_aggregate(s, route, NO_DEVICE)
    with pytest.raises(NNBVHError, match="sequence of nn_bvh_amd.AlphaTexture"):
        make_aggregate(s, route, NO_DEVICE, alpha_textures=[np.ones((2, 2), F)])
    for name, short in (("normals", s.normals[:-1]), ("uvs", s.uvs[:-1]), ("prim_alpha", np.ones(3, F)),
                        ("animated", np.zeros(len(s.placements) - 1, _lib.ANIMATED_DTYPE))):
        with pytest.raises(NNBVHError, match=name + " has"):
            make_aggregate(s, route, NO_DEVICE, **{name: short})


ADAPTER_EXE = os.path.join(ROOT, "tests", "cpp", "two_level_alpha_texture_adapter_check")


def build_adapter_check(nnbvh_lib):
    libdir = os.path.join(ROOT, "nn_bvh_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), ADAPTER_EXE + ".cpp",
                    "-o", ADAPTER_EXE, "-pthread", "-L", libdir, "-l:libnnbvh_hip.so", f"-Wl,-rpath,{libdir}",
                    "-Wl,-rpath-link,/opt/rocm/lib"], check=True)
    return ADAPTER_EXE


def test_cpp_front_end_compiles_and_hands_its_arguments_over(nnbvh_lib):
    out = subprocess.run([build_adapter_check(nnbvh_lib)], capture_output=True, text=True)
    assert out.returncode == 0 and "two-level alpha texture adapter ok (arguments)" in out.stdout, out.stdout + out.stderr


# ---- GPU -----------------------------------------------------------------------------------------------------------------
def first_bad(got, exp):
    return [i for i in range(len(exp)) if got[i].tobytes() != exp[i].tobytes()][:5]


def alpha_rows(inst, hostc_modes=()):
    """the trace_kernel instances a two-level alpha scene may launch: {mode, 8, inst, 1, 2, 0, hostc}"""
    return {(m, 8, inst, 1, 2, 0, 0) for m in (0, 1, 2)} | {(m, 8, inst, 1, 2, 0, 1) for m in hostc_modes}


CASES = [(True, 4, "sah"), (True, 1, "sah"), (False, 4, "sah"), (True, 4, "hlbvh"), (True, 1, "hlbvh")]
# case -> (kernel family, the instances ALL its device calls launch), asserted by ledger_start / assert_reached
# (tests/ledger_cases.py) around the whole case; the LaunchLedger blocks inside the tests assert the same per call
LEDGER = {f"test_device_equals_the_per_ray_oracle[{with_uvs}-{max_prims}-{split}-{route}]": (BVH, alpha_rows(1))
          for with_uvs, max_prims, split in CASES for route in ("host_tree", "device_build")}
LEDGER.update({
    "test_animated_placements_equal_the_per_ray_oracle": (BVH, alpha_rows(2)),
    # the two candidate calls and the plain Intersect
    "test_candidate_calls_with_host_only_triangles[static]":
        (BVH, {(0, 8, 1, 1, 2, 0, 1), (2, 8, 1, 1, 2, 0, 1), (0, 8, 1, 1, 2, 0, 0)}),
    "test_candidate_calls_with_host_only_triangles[animated]":
        (BVH, {(0, 8, 2, 1, 2, 0, 1), (2, 8, 2, 1, 2, 0, 1), (0, 8, 2, 1, 2, 0, 0)}),
    # an alpha scene has no mode-3 form: the batches and the gathered queues run as modes 0 and 2
    "test_batches_call_and_wavefront_queues": (BVH, {(0, 8, 1, 1, 2, 0, 0), (2, 8, 1, 1, 2, 0, 0)}),
})


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["host_tree", "device_build"])
@pytest.mark.parametrize("with_uvs,max_prims,split", CASES)
def test_device_equals_the_per_ray_oracle(with_uvs, max_prims, split, route):
    """closest (prim, t, b, both counters, instance), any hit with counts (mode 1) and without (mode 2), whole batches
    and batches of 1, 63, 64, 65 and 257; the INST = 1 x ALPHA = 2 instances are the ones launched"""
    c = case("static", with_uvs, max_prims, split)
    key = f"test_device_equals_the_per_ray_oracle[{with_uvs}-{max_prims}-{split}-{route}]"
    start = ledger_start(LEDGER, key)
    agg = make_aggregate(c.s, route)
    try:
        with _lib.LaunchLedger(_lib.FAMILY_BVH) as led:
            got = agg.Intersect(c.rays)
            occ, vis, tst = agg.IntersectP(c.rays, counts=True)
            occ2 = agg.IntersectP(c.rays)
        assert set(led.launched) == alpha_rows(1), led.launched
        assert got.tobytes() == c.closest.tobytes(), first_bad(got, c.closest)
        eo, ev, et = c.any_hit
        assert np.array_equal(occ, eo) and np.array_equal(vis, ev) and np.array_equal(tst, et)
        assert np.array_equal(occ2, eo)
        for k in (1, 63, 64, 65, 257):
            assert agg.Intersect(c.rays[:k]).tobytes() == c.closest[:k].tobytes(), k
            assert np.array_equal(agg.IntersectP(c.rays[:k]), eo[:k]), k
            o2, v2, t2 = agg.IntersectP(c.rays[-k:], counts=True)
            assert np.array_equal(o2, eo[-k:]) and np.array_equal(v2, ev[-k:]) and np.array_equal(t2, et[-k:]), k
    finally:
        agg.close()
    assert_reached(LEDGER, key, start)
    kinds, inside = c.hit_kind(), c.closest["instance"] > 0
    assert all((inside & (kinds == k)).sum() > 20 for k in (16, 17, 18, 19))
    assert c.rejected_by_hash().sum() > 20 and c.two_placements().sum() > 20 and c.accepted_behind_rejected().sum() > 20


@pytest.mark.gpu
@pytest.mark.parametrize("name,split", [("static", "sah"), ("static", "hlbvh"), ("animated", "sah")])
def test_creation_routes_make_the_same_bytes(name, split):
    c = case(name, True, 4, split)
    a, b = make_aggregate(c.s, "host_tree"), make_aggregate(c.s, "device_build")
    try:
        for what in (0, 1, 2, 3, 4):
            x, y = a.read(what), b.read(what)
            assert (x is None) == (y is None) == (what == 2 and name == "static"), what
            assert x is None or (x.shape == y.shape and x.tobytes() == y.tobytes()), what
        assert all(np.array_equal(x, y) for x, y in zip(a.Bounds(), b.Bounds()))
        assert a.info == b.info
        pool = np.concatenate([t.image.reshape(-1) for t in c.s.textures])
        assert a.read(4).tobytes() == pool.tobytes()
        assert [int(r[2]) for r in a.read(3)] == [t.width for t in c.s.textures]
        # the table and the pool are counted: records (256-B aligned), slots + 64 B, the animation table is not
        records = (max(a.info["interior_records"], 1) * 64 + 255) & ~255
        assert a.info["device_bytes"] == records + a.info["prim_slots"] * 16 + 64 + 48 * len(c.s.textures) + 4 * len(pool)
        kinds = np.concatenate([c.s.top] + list(c.s.objects))["kind"]
        slots = (3 * (kinds < 8).sum() + 3 * np.isin(kinds, (6, 7)).sum() + 4 * (kinds == 8).sum() + 6 * (kinds == 12).sum() +
                 5 * (kinds >= 16).sum() + 3 * (kinds >= 18).sum() + 6 * len(c.s.placements))
        assert a.info["prim_slots"] == slots
    finally:
        a.close()
        b.close()


@pytest.mark.gpu
def test_animated_placements_equal_the_per_ray_oracle():
    """five placements, three actually animated, ray times below, inside and above the range: the INST = 2 x ALPHA = 2
    instances"""
    c = case("animated")
    start = ledger_start(LEDGER, "test_animated_placements_equal_the_per_ray_oracle")
    for route in ("host_tree", "device_build"):
        agg = make_aggregate(c.s, route)
        try:
            with _lib.LaunchLedger(_lib.FAMILY_BVH) as led:
                got = agg.Intersect(c.rays)
                occ, vis, tst = agg.IntersectP(c.rays, counts=True)
                occ2 = agg.IntersectP(c.rays)
            assert set(led.launched) == alpha_rows(2), led.launched
            assert got.tobytes() == c.closest.tobytes(), (route, first_bad(got, c.closest))
            eo, ev, et = c.any_hit
            assert np.array_equal(occ, eo) and np.array_equal(vis, ev) and np.array_equal(tst, et)
            assert np.array_equal(occ2, eo)
        finally:
            agg.close()
    assert_reached(LEDGER, "test_animated_placements_equal_the_per_ray_oracle", start)
    an = c.s.anims
    moving = (c.closest["instance"] > 0) & (an["actually_animated"][np.maximum(c.closest["instance"] - 1, 0)] != 0)
    within = (c.rays["time"] > 0) & (c.rays["time"] < 1)
    assert (c.accepted_behind_rejected() & moving & within).sum() > 20


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["static", "animated"])
def test_candidate_calls_with_host_only_triangles(name):
    """every second plain triangle (kind 0, in both objects) declared host-only in the baked order: the candidate
    calls (the HOSTC twins), resolved with the oracle's triangle test, equal the per-ray oracle of the scene with
    them as triangles"""
    from nn_bvh_amd import resolve_host_candidates, resolve_host_candidates_any
    from test_host_candidates import assert_resolved_equal, tri_callback, tri_table
    c = case(name)
    s = c.s
    nodes, prims, instances, n_top, _ = tlo.shared_form(s)
    hp = prims.copy()
    plain = np.nonzero(hp["kind"] == 0)[0]
    hp["kind"][plain[::2]] = 3
    start = ledger_start(LEDGER, f"test_candidate_calls_with_host_only_triangles[{name}]")
    agg = BVHAggregate.from_tree(nodes, hp, s.verts, instances=instances, n_top_nodes=n_top, animated=s.anims,
                                 normals=s.normals, uvs=s.uvs, prim_alpha=tlo.ordered_alpha(s, prims),
                                 alpha_textures=s.textures)
    inst = 1 if name == "static" else 2
    try:
        with _lib.LaunchLedger(_lib.FAMILY_BVH) as led:
            hits, cands = agg.intersect_with_host_candidates(c.rays, capacity=16)
            occ, cands_any = agg.intersect_p_with_host_candidates(c.rays, capacity=16)
        assert set(led.launched) == {(0, 8, inst, 1, 2, 0, 1), (2, 8, inst, 1, 2, 0, 1)}, led.launched
        with _lib.LaunchLedger(_lib.FAMILY_BVH) as led:
            void = agg.Intersect(c.rays)
        assert set(led.launched) == {(0, 8, inst, 1, 2, 0, 0)}, led.launched
    finally:
        agg.close()
    assert_reached(LEDGER, f"test_candidate_calls_with_host_only_triangles[{name}]", start)
    cnt = cands["count"]
    assert (cnt > 0).sum() > 100 and (cnt >= 0).all()
    assert np.array_equal(void["instance"] == -1, cnt != 0)
    all_prims = np.concatenate([s.top] + list(s.objects))

    def minv(idx, k):
        rows = instances["prim_from_render"][k].copy()
        if s.anims is not None:
            a = s.anims["actually_animated"][k] != 0
            if a.any():
                rows[a] = ob.anim_interpolate(s.oa[k[a]], c.rays["time"][idx[a]])[:, 16:28]
        return rows

    try:
        ob.set_sin_mode(1)
        cb = tri_callback(c.rays, s.verts, tri_table(all_prims), minv)
        res = resolve_host_candidates(c.rays, hits, cands, cb, kind=c.kind_of_id)
        res_any = resolve_host_candidates_any(c.rays, occ, cands_any, cb)
    finally:
        ob.set_sin_mode(0)
    assert_resolved_equal(res, c.closest, "two-level textured alpha with host-only triangles, closest")
    assert np.array_equal(res_any, c.any_hit[0])
    is_host = np.zeros(len(c.kind_of_id), bool)
    is_host[hp["id"][hp["kind"] == 3]] = True
    assert ((res["prim"] >= 0) & is_host[np.maximum(res["prim"], 0)]).sum() > 20
    assert ((occ == 2) & (res_any == 1)).sum() > 5 and ((occ == 2) & (res_any == 0)).sum() > 5


@pytest.mark.gpu
def test_batches_call_and_wavefront_queues():
    """nnbvh_trace_batches_device (a closest and an any-hit batch: separate launches for an alpha scene) and
    nnbvh_wavefront_intersect_closest_and_shadow (the closest queue's rays carry tMax = Infinity; queue calls gather
    records for an INST scene)"""
    import torch
    from nn_bvh_amd.wavefront import RayQueue, WavefrontAggregate, WorkQueue
    from test_wavefront import QUEUES, shadow_inputs
    c = case("static")
    dev = torch.device("cuda", 0)
    start = ledger_start(LEDGER, "test_batches_call_and_wavefront_queues")
    agg = make_aggregate(c.s, "device_build")
    try:
        n = len(c.rays)
        d_rays = torch.from_numpy(c.rays.view(np.uint8).reshape(n, 32)).to(dev)
        d_hits = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
        d_occ = torch.full((n,), 9, dtype=torch.uint8, device=dev)
        with _lib.LaunchLedger(_lib.FAMILY_BVH) as led:
            agg.trace_batches_device([("closest", d_rays.data_ptr(), n, d_hits.data_ptr()),
                                      ("any", d_rays.data_ptr(), n, d_occ.data_ptr())])
            torch.cuda.synchronize()
        assert led.launched and set(led.launched) <= alpha_rows(1), led.launched
        got = d_hits.cpu().numpy().view(_lib.HIT_DTYPE).reshape(-1)
        assert got.tobytes() == c.closest.tobytes(), first_bad(got, c.closest)
        assert np.array_equal(d_occ.cpu().numpy(), c.any_hit[0])
        far = c.rays.copy()
        far["tmax"] = np.inf
        exp_far = c.oracle.closest(rays=far)  # alpha does not depend on tMax
        Ld, r_u, r_l, px, L = shadow_inputs(n, n + 100, 7)
        t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
        rq, sq = RayQueue.from_records(far, dev), RayQueue.from_records(c.rays, dev, shadow=True)
        wf = WavefrontAggregate(agg)
        queues = {k: WorkQueue(n, dev) for k in QUEUES}
        hits_t = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
        L_t, occ_t = t(L), torch.full((n,), 9, dtype=torch.uint8, device=dev)
        with _lib.LaunchLedger(_lib.FAMILY_BVH) as led:
            wf.IntersectClosestAndShadow(n, rq, n, sq, t(Ld), t(r_u), t(r_l), t(px), L_t, hits=hits_t, occluded=occ_t, **queues)
            torch.cuda.synchronize()
        assert led.launched and set(led.launched) <= alpha_rows(1), led.launched
        got = hits_t.cpu().numpy().view(_lib.HIT_DTYPE).reshape(-1)
        assert got.tobytes() == exp_far.tobytes(), first_bad(got, exp_far)
        assert np.array_equal(occ_t.cpu().numpy(), c.any_hit[0])
        expL = ob.record_shadow(c.any_hit[0], Ld, r_u, r_l, px, L)
        assert np.array_equal(L_t.cpu().numpy().view(np.uint32), expL.view(np.uint32))
    finally:
        agg.close()
    assert_reached(LEDGER, "test_batches_call_and_wavefront_queues", start)


@pytest.mark.gpu
def test_cpp_front_end_traces_through_both_routes(nnbvh_lib):
    out = subprocess.run([build_adapter_check(nnbvh_lib), "gpu"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "two-level alpha texture adapter ok" in out.stdout, out.stdout + out.stderr
