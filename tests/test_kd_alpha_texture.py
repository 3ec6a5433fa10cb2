"""Image-textured alpha on triangles (primitive kinds 16 .. 19) in kd-tree scenes: the two creation calls
(nnbvh_kd_scene_create_with_alpha_textures / nnbvh_kd_scene_create_gpu_build_with_alpha_textures), the three kd builders
on such primitives, and the ATTR = 2 instances of kd_trace_kernel against the per-ray oracle.

The oracle is the construction of tests/alpha_texture_oracle.py on the kd walk: ato.per_ray_alpha gives alpha[i][j] of
every textured triangle j for ray i (prims in the caller's order, which is the order kd scenes keep), and the C oracle's
KdTreeAggregate (ob.kd_closest / ob.kd_any_hit) runs on ray i alone with kinds 16 .. 19 rewritten to 4 .. 7 and v[3] =
bits(alpha[i][j]).  Everything is compared bit for bit; no expected value comes from the device."""
import collections
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
from nn_bvh_amd import AlphaTexture, NNBVHError, _lib
from nn_bvh_amd._lib import HIT_DTYPE, ptr
from nn_bvh_amd.kdtree import KdTreeAggregate, build_kd_tree, prim_bounds_of
from test_alpha_texture import grid_scene, mixed_soup, scene_rays, small_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_CALLS = ("nnbvh_kd_scene_create_with_alpha_textures", "nnbvh_kd_scene_create_gpu_build_with_alpha_textures")
NO_DEVICE = 1 << 20  # a device index no machine has: a well-formed call gets as far as the device check
F = np.float32
ADAPTER_EXE = os.path.join(ROOT, "tests", "cpp", "kd_alpha_texture_adapter_check")


# ---- the kd per-ray oracle ----------------------------------------------------------------------------------------
class KdPerRayOracle:
    """closest / any hit of a kd scene with textured triangles: the C oracle's kd walk on each ray alone.  prims in the
    caller's order; tree: anything with nodes / prim_indices / bounds; alpha / tex: ato.per_ray_alpha's (they depend
    on neither the tree nor tMax, so cases share them)."""

    def __init__(self, tree, prims, verts, rays, normals, alpha, tex):
        self.tree, self.prims, self.verts, self.rays = tree, np.ascontiguousarray(prims), verts, rays
        self.normals, self.alpha, self.tex = normals, alpha, tex

    def _each(self, fn):
        work = self.prims.copy()
        work["kind"][self.tex] -= 12
        t = self.tree
        try:
            ob.set_vertex_normals(self.normals)
            for i in range(len(self.rays)):
                work["v"][self.tex, 3] = self.alpha[i].view(np.int32)
                fn(i, (t.nodes, t.prim_indices, work, self.verts, t.bounds, self.rays[i:i + 1]))
        finally:
            ob.set_vertex_normals(None)

    def closest(self):
        hits = np.zeros(len(self.rays), HIT_DTYPE)

        def one(i, args):
            hits[i] = ob.kd_closest(*args)[0]
        self._each(one)
        return hits

    def any_hit(self):
        n = len(self.rays)
        occ, vis, tst = np.zeros(n, np.uint8), np.zeros(n, np.int32), np.zeros(n, np.int32)

        def one(i, args):
            o, v, t = ob.kd_any_hit(*args)
            occ[i], vis[i], tst[i] = o[0], v[0], t[0]
        self._each(one)
        return occ, vis, tst


Scene = collections.namedtuple("Scene", "verts prims normals uvs textures rays")
Case = collections.namedtuple("Case", "verts prims normals uvs textures rays tree closest any_hit alpha tex")


@functools.lru_cache(None)
def scene_of(name):
    verts, prims, normals, uvs = mixed_soup() if name == "soup" else grid_scene()
    return Scene(verts, prims, normals, uvs, ato.scene_textures(0), scene_rays(verts, prims, 7 if name == "soup" else 11))


@functools.lru_cache(None)
def alpha_of(name, with_uvs):
    s = scene_of(name)
    return ato.per_ray_alpha(s.prims, s.verts, s.uvs if with_uvs else None, s.textures, s.rays)


@functools.lru_cache(None)
def tree_of(name, max_prims, where):
    s = scene_of(name)
    return build_kd_tree(s.prims, s.verts, max_prims=max_prims, where=where)


@functools.lru_cache(None)
def case(name, max_prims, with_uvs=True, where="host"):
    """where: "host" for from_tree / build, "host_stable" for build_on_device (the device's leaf order)"""
    s = scene_of(name)
    alpha, tex = alpha_of(name, with_uvs)
    tree = tree_of(name, max_prims, where)
    per = KdPerRayOracle(tree, s.prims, s.verts, s.rays, s.normals, alpha, tex)
    return Case(s.verts, s.prims, s.normals, s.uvs if with_uvs else None, s.textures, s.rays, tree, per.closest(),
                per.any_hit(), alpha, tex)


def first_bad(got, exp):
    return [i for i in range(len(exp)) if got[i].tobytes() != exp[i].tobytes()][:5]


# ---- 1: exports -------------------------------------------------------------------------------------------------------
def test_calls_are_exported_prototyped_and_declared(nnbvh_lib):
    header = open(os.path.join(ROOT, "include", "nnbvh.h")).read()
    for name, twin in zip(NEW_CALLS, ("nnbvh_kd_scene_create_with_attributes",
                                      "nnbvh_kd_scene_create_gpu_build_with_attributes")):
        assert name in _lib.EXPORTS and hasattr(nnbvh_lib, name), name
        assert re.search(r"nnbvh_kd_scene \*" + name + r"\(", header), name
        fn = getattr(nnbvh_lib, name)
        assert fn.restype is ctypes.c_void_p
        assert list(fn.argtypes) == list(getattr(nnbvh_lib, twin).argtypes) + [ctypes.c_void_p, ctypes.c_int]
        decl = re.sub(r"\s+", " ", header[header.index("*" + name + "("):].split(";")[0])
        assert decl.endswith("const nnbvh_alpha_texture *textures, int n_textures)"), decl
    assert "flat scenes only" not in header.lower()


# ---- 2: a textured triangle is a triangle for the builders ------------------------------------------------------------
def as_plain(prims):
    out = prims.copy()
    tex = ato.is_textured(out["kind"])
    out["kind"][tex], out["v"][tex, 3] = 0, 0
    return out


def assert_same_tree(a, b, what):
    assert a.nodes.tobytes() == b.nodes.tobytes(), what
    assert a.prim_indices.tobytes() == b.prim_indices.tobytes(), what
    assert a.bounds.tobytes() == b.bounds.tobytes() and a.depth == b.depth, what


@pytest.mark.parametrize("name", ["soup", "grid"])
@pytest.mark.parametrize("max_prims", [1, 4])
def test_host_builders_take_textured_triangles_as_triangles(name, max_prims):
    s = scene_of(name)
    assert ato.is_textured(s.prims["kind"]).mean() > 0.25
    plain = as_plain(s.prims)
    for where in ("host", "host_stable"):
        assert_same_tree(tree_of(name, max_prims, where), build_kd_tree(plain, s.verts, max_prims=max_prims, where=where),
                         (name, max_prims, where))
    # the stable order is the same tree but for the order inside multi-primitive leaves
    assert tree_of(name, max_prims, "host").nodes.tobytes() == tree_of(name, max_prims, "host_stable").nodes.tobytes()
    # v[3] of a textured triangle (0 .. 2 here: valid vertex numbers) is no vertex index
    for got, exp in zip(prim_bounds_of(s.prims, s.verts), prim_bounds_of(plain, s.verts)):
        assert got.tobytes() == exp.tobytes()
    # ... nor is it for any other triangle kind: kinds 4 .. 7 keep the bits of an alpha there
    tri = s.verts[s.prims["v"][:, :3]]
    lo, hi = prim_bounds_of(s.prims, s.verts)
    assert np.array_equal(lo, tri.min(1)) and np.array_equal(hi, tri.max(1))
    assert all((s.prims["kind"] == k).any() for k in (4, 5, 6, 7))


# ---- 3: argument faults -----------------------------------------------------------------------------------------------
def raw_create(L, route, tree, prims, verts, textures, n_textures=None, normals=None, uvs=None, device=NO_DEVICE):
    table, n = _lib.alpha_texture_table(textures) if textures is not None else (None, 0)
    n = n if n_textures is None else n_textures
    opt = lambda a: ptr(a) if a is not None else None  # noqa: E731
    if route == "host_tree":
        idx = tree.prim_indices
        return L.nnbvh_kd_scene_create_with_alpha_textures(
            ptr(tree.nodes), len(tree.nodes), ptr(idx) if len(idx) else None, len(idx), ptr(prims), len(prims), ptr(verts),
            len(verts), ptr(tree.bounds), opt(normals), opt(uvs), None, device, table, n)
    return L.nnbvh_kd_scene_create_gpu_build_with_alpha_textures(
        ptr(prims), len(prims), ptr(verts), len(verts), None, opt(normals), opt(uvs), None, 5, 1, ctypes.c_float(0.5), 1, -1,
        device, table, n)


@pytest.mark.parametrize("route", ["host_tree", "device_build"])
def test_argument_faults_name_the_call_before_any_device_work(nnbvh_lib, route):
    """the refusal list of test_alpha_texture.py's test of the same name, for the two kd calls"""
    L = nnbvh_lib
    call = NEW_CALLS[0 if route == "host_tree" else 1]
    verts, prims = small_scene()
    good = [AlphaTexture(np.ones((2, 3), F)), AlphaTexture(np.zeros((1, 1), F), wrap="black")]
    tree = build_kd_tree(as_plain(prims), verts)  # (the refusals below must not depend on the builder)

    def refused(words, prims=prims, textures=good, **kw):
        assert not raw_create(L, route, tree, prims, verts, textures, **kw), words
        err = _lib.last_error()
        assert call in err and words in err, (words, err)

    # a well-formed call gets as far as the device check
    assert not raw_create(L, route, tree, prims, verts, good) and "no usable HIP device" in _lib.last_error()
    assert not raw_create(L, route, tree, prims, verts, good, uvs=np.zeros((len(verts), 2), F))
    assert "no usable HIP device" in _lib.last_error()
    refused("need the alpha-texture table", textures=None)
    refused("null alpha-texture table", n_textures=2, textures=None)
    p = prims.copy()
    p["v"][0, 3] = 2
    refused("alpha-texture index out of range", prims=p)
    p["v"][0, 3] = -1
    refused("alpha-texture index out of range", prims=p)
    bad = AlphaTexture(np.ones((2, 3), F))
    bad.texels = None
    refused("null texels", textures=[good[0], bad])
    for w, h in ((0, 1), (1, 0), (-3, 2), ((1 << 24) + 1, 1), (1, (1 << 24) + 1)):
        bad = AlphaTexture(np.ones((2, 3), F))
        bad.width, bad.height = w, h
        refused("width and height must be 1 .. 2^24", textures=[bad, good[1]])
    for wrap in (3, -1, 7):
        bad = AlphaTexture(np.ones((2, 3), F), wrap=wrap)
        refused("unknown wrap mode", textures=[good[0], bad])
    for kind in (18, 19):
        v2, p2 = small_scene(kind)
        refused("need the vertex normals", prims=p2)
    p = prims.copy()  # a scene that also holds alpha-tested patches
    p["kind"][1] = 8
    refused("alpha-tested patches", prims=p)
    # ... which a table alone does not forbid: without a textured triangle the call is the one without textures
    p["kind"][p["kind"] == 16], p["v"][:, 3] = 0, 0
    assert not raw_create(L, route, tree, p, verts, good) and "no usable HIP device" in _lib.last_error()


def test_the_kd_calls_without_a_table_still_refuse_kind_16(nnbvh_lib):
    L = nnbvh_lib
    verts, prims = small_scene()
    tree = build_kd_tree(as_plain(prims), verts)
    idx, nv, half = tree.prim_indices, len(verts), ctypes.c_float(0.5)
    head = (ptr(tree.nodes), len(tree.nodes), ptr(idx) if len(idx) else None, len(idx), ptr(prims), len(prims), ptr(verts),
            nv, ptr(tree.bounds))
    calls = [lambda: L.nnbvh_kd_scene_create(*head, NO_DEVICE),
             lambda: L.nnbvh_kd_scene_create_with_attributes(*head, None, None, None, NO_DEVICE),
             lambda: L.nnbvh_kd_scene_create_gpu_build(ptr(prims), len(prims), ptr(verts), nv, None, 5, 1, half, 1, -1,
                                                       NO_DEVICE),
             lambda: L.nnbvh_kd_scene_create_gpu_build_with_attributes(ptr(prims), len(prims), ptr(verts), nv, None, None,
                                                                       None, None, 5, 1, half, 1, -1, NO_DEVICE)]
    for call in calls:
        assert not call()
        err = _lib.last_error()
        assert "unknown primitive kind" in err and " / ".join(NEW_CALLS) in err, err
        assert "nnbvh_scene_create_with_alpha_textures / nnbvh_scene_create_gpu_build_with_alpha_textures" in err


# ---- 4, 5: the oracle alone ----------------------------------------------------------------------------------------------
def alpha_test_shares(c):
    """of the rays: the record differs from the all-opaque scene's / a textured hit was accepted after evaluating
    0 < a < 1 / the closest hit is a textured triangle.  From the oracle alone (kd prims are in the caller's order: id
    k is row k)."""
    assert np.array_equal(c.prims["id"], np.arange(len(c.prims)))
    col_of_prim = np.full(len(c.prims), -1)
    col_of_prim[c.tex] = np.arange(len(c.tex))
    hit = c.closest["prim"] >= 0
    col = col_of_prim[np.maximum(c.closest["prim"], 0)]
    a_hit = c.alpha[np.arange(len(c.rays)), np.maximum(col, 0)]
    accepted_mid = hit & (col >= 0) & (a_hit > 0) & (a_hit < 1)
    opaque = ato.constant_prims(c.prims, c.tex, np.ones(len(c.tex), F))
    try:
        ob.set_vertex_normals(c.normals)
        h0 = ob.kd_closest(c.tree.nodes, c.tree.prim_indices, opaque, c.verts, c.tree.bounds, c.rays)
    finally:
        ob.set_vertex_normals(None)
    differs = np.array([c.closest[i].tobytes() != h0[i].tobytes() for i in range(len(c.rays))])
    return differs.mean(), accepted_mid.mean(), (hit & (col >= 0)).mean()


@pytest.mark.parametrize("name", ["soup", "grid"])
@pytest.mark.parametrize("max_prims", [1, 4])
def test_the_oracle_alone_rejects_and_accepts_enough(name, max_prims):
    c = case(name, max_prims)
    differs, accepted_mid, textured = alpha_test_shares(c)
    print(name, max_prims, "differs from opaque", differs, "accepted with 0 < a < 1", accepted_mid, "textured closest hit",
          textured)
    assert differs >= 0.10 and accepted_mid >= 0.10 and textured > 0.10
    assert not (c.closest["instance"] == -1).any() and not (c.any_hit[0] == 2).any()  # no record is void


def test_per_ray_oracle_with_constant_zero_textures_is_the_kind_4_oracle():
    """a constant 0 gives exactly 0 through the bilinear sum: the construction must then agree with the kd oracle's own
    constant-alpha path on the whole batch"""
    s = scene_of("soup")
    zero = [AlphaTexture(np.zeros(sh, F), wrap=w, point_filter=p) for sh, w, p in (((5, 3), "repeat", False),
                                                                                  ((1, 1), "clamp", False),
                                                                                  ((7, 9), "black", True))]
    tree = tree_of("soup", 4, "host")
    rays = scene_rays(s.verts, s.prims, 3, 512)
    alpha, tex = ato.per_ray_alpha(s.prims, s.verts, s.uvs, zero, rays)
    assert (alpha == 0).all() and not np.signbit(alpha).any()
    per = KdPerRayOracle(tree, s.prims, s.verts, rays, s.normals, alpha, tex)
    const = ato.constant_prims(s.prims, tex, np.zeros(len(tex), F))
    try:
        ob.set_vertex_normals(s.normals)
        exp = ob.kd_closest(tree.nodes, tree.prim_indices, const, s.verts, tree.bounds, rays)
        eo, ev, et = ob.kd_any_hit(tree.nodes, tree.prim_indices, const, s.verts, tree.bounds, rays)
    finally:
        ob.set_vertex_normals(None)
    assert per.closest().tobytes() == exp.tobytes()
    occ, vis, tst = per.any_hit()
    assert np.array_equal(occ, eo) and np.array_equal(vis, ev) and np.array_equal(tst, et)
    assert not ato.is_textured(s.prims["kind"])[np.maximum(exp["prim"], 0)][exp["prim"] >= 0].any()  # alpha 0: never hit
    assert (exp["prim"] >= 0).mean() > 0.3


# ---- 6, 7: the front ends ----------------------------------------------------------------------------------------------
def test_python_front_end_checks_its_arguments():
    verts, prims = small_scene()
    tree = build_kd_tree(as_plain(prims), verts)
    two = [AlphaTexture(np.ones((2, 2), F))] * 2
    with pytest.raises(NNBVHError, match="sequence of nn_bvh_amd.AlphaTexture"):
        KdTreeAggregate.from_tree(tree.nodes, tree.prim_indices, prims, verts, tree.bounds, device=NO_DEVICE,
                                  alpha_textures=[np.ones((2, 2), F)])
    with pytest.raises(NNBVHError, match="sequence of nn_bvh_amd.AlphaTexture"):
        KdTreeAggregate.build_on_device(prims, verts, device=NO_DEVICE, alpha_textures=[np.ones((2, 2), F)])
    short = np.zeros((len(verts) - 1, 2), F)
    with pytest.raises(ValueError):
        KdTreeAggregate.from_tree(tree.nodes, tree.prim_indices, prims, verts, tree.bounds, device=NO_DEVICE, uvs=short,
                                  alpha_textures=two)
    with pytest.raises(ValueError):
        KdTreeAggregate.build(prims, verts, device=NO_DEVICE, uvs=short, alpha_textures=two)
    with pytest.raises(ValueError):
        KdTreeAggregate.build_on_device(prims, verts, device=NO_DEVICE, uvs=short, alpha_textures=two)
    # well-formed calls get as far as the device check, through the new calls
    for make in (lambda: KdTreeAggregate.build(prims, verts, device=NO_DEVICE, alpha_textures=two),
                 lambda: KdTreeAggregate.build_on_device(prims, verts, device=NO_DEVICE, alpha_textures=two)):
        with pytest.raises(NNBVHError, match="no usable HIP device"):
            make()
    with pytest.raises(NNBVHError, match="unknown primitive kind"):  # without a table: the existing calls, unchanged
        KdTreeAggregate.build(prims, verts, device=NO_DEVICE)


def build_adapter_check(nnbvh_lib):
    libdir = os.path.join(ROOT, "nn_bvh_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), ADAPTER_EXE + ".cpp",
                    "-o", ADAPTER_EXE, "-pthread", "-L", libdir, "-l:libnnbvh_hip.so", f"-Wl,-rpath,{libdir}",
                    "-Wl,-rpath-link,/opt/rocm/lib"], check=True)
    return ADAPTER_EXE


def test_cpp_front_end_compiles_and_hands_its_arguments_over(nnbvh_lib):
    out = subprocess.run([build_adapter_check(nnbvh_lib)], capture_output=True, text=True)
    assert out.returncode == 0 and "kd alpha texture adapter ok (arguments)" in out.stdout, out.stdout + out.stderr


# ---- GPU: the kernels against the per-ray oracle ---------------------------------------------------------------------------
def make_aggregate(c, route, max_prims):
    if route == "from_tree":
        return KdTreeAggregate.from_tree(c.tree.nodes, c.tree.prim_indices, c.prims, c.verts, c.tree.bounds,
                                         normals=c.normals, uvs=c.uvs, alpha_textures=c.textures)
    return KdTreeAggregate.build_on_device(c.prims, c.verts, normals=c.normals, uvs=c.uvs, max_prims=max_prims,
                                           alpha_textures=c.textures)


def assert_device_equals(agg, rays, exp, any_exp, ks=()):
    """closest (prim, t, b, both counters, void mark), any hit with counts and without; then the first and last k rays"""
    eo, ev, et = any_exp
    got = agg.Intersect(rays)
    assert got.tobytes() == exp.tobytes(), first_bad(got, exp)
    occ, vis, tst = agg.IntersectP(rays, counts=True)
    assert np.array_equal(occ, eo) and np.array_equal(vis, ev) and np.array_equal(tst, et)
    assert np.array_equal(agg.IntersectP(rays), eo)
    for k in ks:  # batches below, at and above one wavefront, and above one block
        assert agg.Intersect(rays[:k]).tobytes() == exp[:k].tobytes(), k
        assert np.array_equal(agg.IntersectP(rays[:k]), eo[:k]), k
        o2, v2, t2 = agg.IntersectP(rays[-k:], counts=True)
        assert np.array_equal(o2, eo[-k:]) and np.array_equal(v2, ev[-k:]) and np.array_equal(t2, et[-k:]), k
        assert agg.Intersect(rays[-k:]).tobytes() == exp[-k:].tobytes(), k


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["from_tree", "build_on_device"])
@pytest.mark.parametrize("with_uvs", [True, False])
@pytest.mark.parametrize("max_prims", [1, 4])
@pytest.mark.parametrize("name", ["soup", "grid"])
def test_device_equals_the_per_ray_oracle(name, max_prims, with_uvs, route):
    c = case(name, max_prims, with_uvs, "host" if route == "from_tree" else "host_stable")
    agg = make_aggregate(c, route, max_prims)
    try:
        assert_device_equals(agg, c.rays, c.closest, c.any_hit, (1, 63, 64, 65, 257))
    finally:
        agg.close()
    textured = ato.is_textured(c.prims["kind"])
    assert (textured[np.maximum(c.closest["prim"], 0)] & (c.closest["prim"] >= 0)).mean() > 0.1


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["from_tree", "build_on_device"])
def test_a_table_without_textured_triangles_changes_nothing(route):
    """alpha-tested patches (kinds 8 .. 15) and smooth alpha-tested triangles with a texture table but no textured
    triangle: both calls accept the scene, keep the table, and trace it as the calls without textures do — against the
    kd oracle's own alpha-patch path (the recursion after a rejected hit included), which needs no per-ray construction"""
    from nn_bvh_amd import scene
    from test_alpha import alpha_patch_scene, patch_uvs
    verts, prims, normals, alpha, kinds = alpha_patch_scene(43, 300, 500)
    rng = np.random.default_rng(4)
    prims = prims.copy()
    smooth = ((kinds == 4) | (kinds == 5)) & (rng.random(len(prims)) < 0.5)
    prims["kind"] = np.where(smooth, kinds + 2, kinds)
    kinds = prims["kind"]
    assert not ato.is_textured(kinds).any() and (kinds >= 8).mean() > 0.3
    uvs = patch_uvs(verts)
    textures = ato.scene_textures(0)
    tree = build_kd_tree(prims, verts, max_prims=2, where="host" if route == "from_tree" else "host_stable")
    rays = np.concatenate([scene.random_rays(6000, verts.min(0) - 1, verts.max(0) + 1, 21),
                           scene.random_rays(2000, verts.min(0), verts.max(0), 22, tmax=0.6)])
    try:
        ob.set_vertex_normals(normals)
        ob.set_vertex_uvs(uvs)
        ob.set_prim_alpha(alpha)
        exp = ob.kd_closest(tree.nodes, tree.prim_indices, prims, verts, tree.bounds, rays)
        any_exp = ob.kd_any_hit(tree.nodes, tree.prim_indices, prims, verts, tree.bounds, rays)
    finally:
        ob.set_vertex_normals(None)
        ob.set_vertex_uvs(None)
        ob.set_prim_alpha(None)
    hit_kind = kinds[np.maximum(exp["prim"], 0)]
    for k in range(8, 16):  # every alpha-tested patch kind stands as a closest hit, and some rays are voided or re-traced
        assert ((hit_kind == k) & (exp["prim"] >= 0)).sum() > 10, k
    opaque = alpha.copy()
    opaque[kinds >= 8] = 1.0
    try:
        ob.set_vertex_normals(normals)
        ob.set_vertex_uvs(uvs)
        ob.set_prim_alpha(opaque)
        as_opaque = ob.kd_closest(tree.nodes, tree.prim_indices, prims, verts, tree.bounds, rays)
    finally:
        ob.set_vertex_normals(None)
        ob.set_vertex_uvs(None)
        ob.set_prim_alpha(None)
    assert np.mean([exp[i].tobytes() != as_opaque[i].tobytes() for i in range(len(rays))]) > 0.05  # opaque patches: seen
    if route == "from_tree":
        agg = KdTreeAggregate.from_tree(tree.nodes, tree.prim_indices, prims, verts, tree.bounds, normals=normals, uvs=uvs,
                                        prim_alpha=alpha, alpha_textures=textures)
    else:
        agg = KdTreeAggregate.build_on_device(prims, verts, normals=normals, uvs=uvs, prim_alpha=alpha, max_prims=2,
                                              alpha_textures=textures)
    try:
        assert_device_equals(agg, rays, exp, any_exp, (65,))
        pool = np.concatenate([t.image.reshape(-1) for t in textures])
        assert agg.read(5).tobytes() == pool.tobytes() and len(agg.read(4)) == len(textures)  # the table is kept
    finally:
        agg.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["soup", "grid"])
@pytest.mark.parametrize("max_prims", [1, 4])
def test_gpu_builder_takes_textured_triangles_as_triangles(name, max_prims):
    s = scene_of(name)
    got = build_kd_tree(s.prims, s.verts, max_prims=max_prims, where="gpu")
    assert_same_tree(got, tree_of(name, max_prims, "host_stable"), "gpu against host_stable")
    assert_same_tree(got, build_kd_tree(as_plain(s.prims), s.verts, max_prims=max_prims, where="gpu"), "gpu, kind 0")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["soup", "grid"])
def test_creation_routes_make_the_same_bytes(name):
    c = case(name, 4, True, "host_stable")
    a, b = make_aggregate(c, "from_tree", 4), make_aggregate(c, "build_on_device", 4)
    try:
        for what in range(6):
            assert a.read(what).tobytes() == b.read(what).tobytes(), what
        assert all(np.array_equal(x, y) for x, y in zip(a.Bounds(), b.Bounds()))
        assert a.info() == b.info()
        info = a.info()
        n = len(c.prims)
        # the table is the descriptors in order, the pool the images one after another; both count as device bytes
        pool = np.concatenate([t.image.reshape(-1) for t in c.textures])
        assert a.read(5).tobytes() == pool.tobytes()
        table = a.read(4)
        assert [int(r[2]) for r in table] == [t.width for t in c.textures] and list(table[:, 0]) == [0, 15, 15 + 256]
        assert info["has_attribute_slots"] == 1 and info["has_patches"] == 1 and info["has_host_prims"] == 1
        assert info["device_bytes"] == (8 * info["n_nodes"] + 4 * max(info["n_indices"], 1) + 64 * n + 96 * n +
                                        48 * len(c.textures) + 4 * len(pool))
        # a textured triangle's record: the texture index where kind 4 keeps alpha, the flags, its (u, v) in slots 4 / 5
        rec, ex = a.read(2), a.read(3)
        tex = ato.is_textured(c.prims["kind"])
        assert np.array_equal(rec[tex, 11].view(np.int32), c.prims["v"][tex, 3])
        flags = rec[:, 7].view(np.uint32)
        assert ((flags[tex] & (32 | 1024)) == (32 | 1024)).all() and not (flags[~tex] & 1024).any()
        assert np.array_equal((flags[tex] & 256) != 0, c.prims["kind"][tex] >= 18)
        assert np.array_equal((flags[tex] & 64) != 0, (c.prims["kind"][tex] & 1) == 1)
        assert ex[tex, 16:22].tobytes() == c.uvs[c.prims["v"][tex, :3]].reshape(-1, 6).tobytes()
        assert not ex[tex, 22:].any() and not ex[~tex, 16:].any()
        smooth = np.isin(c.prims["kind"], (6, 7, 18, 19))
        assert ex[smooth][:, [0, 1, 2, 4, 5, 6, 8, 9, 10]].tobytes() == c.normals[c.prims["v"][smooth, :3]].reshape(-1, 9).tobytes()
    finally:
        a.close()
        b.close()
    # without uvs: the default corners
    d = case(name, 4, False, "host_stable")
    a, b = make_aggregate(d, "from_tree", 4), make_aggregate(d, "build_on_device", 4)
    try:
        ex = a.read(3)
        assert ex.tobytes() == b.read(3).tobytes()
        assert (ex[ato.is_textured(d.prims["kind"]), 16:22] == ato.DEFAULT_UV).all()
    finally:
        a.close()
        b.close()


@pytest.mark.gpu
def test_batches_call_and_wavefront_queues():
    """nnbvh_kd_trace_batches_device (a closest and an any-hit batch in one launch), the queue call
    nnbvh_kd_wavefront_intersect_closest_and_shadow (the closest queue's rays carry tMax = Infinity), and the walk
    calls' refusal"""
    import torch
    from nn_bvh_amd.interaction import ShadingMesh
    from nn_bvh_amd.wavefront import RayQueue, WavefrontAggregate, WorkQueue
    from test_wavefront import QUEUES, shadow_inputs
    c = case("soup", 4, True)
    dev = torch.device("cuda", 0)
    agg = make_aggregate(c, "from_tree", 4)
    mesh = None
    try:
        n = len(c.rays)
        d_rays = torch.from_numpy(c.rays.view(np.uint8).reshape(n, 32)).to(dev)
        d_hits = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
        d_occ = torch.full((n,), 9, dtype=torch.uint8, device=dev)
        d_vis = torch.full((n,), -7, dtype=torch.int32, device=dev)
        d_tst = torch.full((n,), -7, dtype=torch.int32, device=dev)
        agg.trace_batches_device([("closest", d_rays.data_ptr(), n, d_hits.data_ptr()),
                                  ("any", d_rays.data_ptr(), n, d_occ.data_ptr(), d_vis.data_ptr(), d_tst.data_ptr())])
        torch.cuda.synchronize()
        got = d_hits.cpu().numpy().view(HIT_DTYPE).reshape(-1)
        assert got.tobytes() == c.closest.tobytes(), first_bad(got, c.closest)
        assert np.array_equal(d_occ.cpu().numpy(), c.any_hit[0])
        assert np.array_equal(d_vis.cpu().numpy(), c.any_hit[1]) and np.array_equal(d_tst.cpu().numpy(), c.any_hit[2])
        # the wavefront call: the same rays without their tMax in the closest queue, with it in the shadow queue
        far = c.rays.copy()
        far["tmax"] = np.inf
        exp_far = KdPerRayOracle(c.tree, c.prims, c.verts, far, c.normals, c.alpha, c.tex).closest()  # alpha: not tMax's
        Ld, r_u, r_l, px, L = shadow_inputs(n, n + 100, 7)
        t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
        rq, sq = RayQueue.from_records(far, dev), RayQueue.from_records(c.rays, dev, shadow=True)
        wf = WavefrontAggregate(agg)
        queues = {k: WorkQueue(n, dev) for k in QUEUES}
        hits_t = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
        L_t, occ_t = t(L), torch.full((n,), 9, dtype=torch.uint8, device=dev)
        wf.IntersectClosestAndShadow(n, rq, n, sq, t(Ld), t(r_u), t(r_l), t(px), L_t, hits=hits_t, occluded=occ_t, **queues)
        torch.cuda.synchronize()
        got = hits_t.cpu().numpy().view(HIT_DTYPE).reshape(-1)
        assert got.tobytes() == exp_far.tobytes(), first_bad(got, exp_far)
        assert np.array_equal(occ_t.cpu().numpy(), c.any_hit[0])
        expL = ob.record_shadow(c.any_hit[0], Ld, r_u, r_l, px, L)
        assert np.array_equal(L_t.cpu().numpy().view(np.uint32), expL.view(np.uint32))
        # the walk calls refuse the scene as they refuse every scene with attribute slots, before any device work
        mesh = ShadingMesh(c.verts, c.prims["v"][:, :3].astype(np.int32))
        state = torch.full((n,), 9, dtype=torch.uint8, device=dev)
        with pytest.raises(NNBVHError, match="kd_wavefront_walk_shadow_tr.*no walk instances"):
            wf.WalkShadowTr(n, sq, mesh, t(Ld), t(r_u), t(r_l), t(px), L_t, state)
        torch.cuda.synchronize()
        assert (state.cpu().numpy() == 9).all()
    finally:
        agg.close()
        if mesh is not None:
            mesh.close()


@pytest.mark.gpu
def test_mixed_with_host_only_primitives_through_candidates():
    """every third plain triangle declared host-only with its exact bounds: the candidate calls (the HOSTC twin),
    resolved with the oracle's triangle test, equal the per-ray oracle of the scene with them as triangles"""
    from nn_bvh_amd import resolve_host_candidates, resolve_host_candidates_any
    from test_host_candidates import assert_resolved_equal, tri_callback, tri_table
    c = case("soup", 4, True)
    host = (c.prims["kind"] == 0) & (np.arange(len(c.prims)) % 3 == 0)
    tri = c.verts[c.prims["v"][:, :3]]
    bounds = np.concatenate([tri.min(1), tri.max(1)], 1).astype(F)
    hp = c.prims.copy()
    hp["kind"][host] = 3
    assert_same_tree(build_kd_tree(hp, c.verts, prim_bounds=bounds, max_prims=4), c.tree, "host-only, exact bounds")
    agg = KdTreeAggregate.from_tree(c.tree.nodes, c.tree.prim_indices, hp, c.verts, c.tree.bounds, normals=c.normals,
                                    uvs=c.uvs, alpha_textures=c.textures)
    try:
        hits, cands = agg.intersect_with_host_candidates(c.rays, capacity=16)
        occ, cands_any = agg.intersect_p_with_host_candidates(c.rays, capacity=16)
        plain = agg.Intersect(c.rays)
    finally:
        agg.close()
    cnt = cands["count"]
    assert (cnt > 0).mean() > 0.05 and (cnt >= 0).mean() > 0.99
    assert np.array_equal(plain["instance"] == -1, cnt != 0)
    cb = tri_callback(c.rays, c.verts, tri_table(c.prims))
    res = resolve_host_candidates(c.rays, hits, cands, cb, kind=np.zeros(len(c.prims), np.int32))
    ok = cnt >= 0
    assert_resolved_equal(res[ok], c.closest[ok], "textured alpha with host-only primitives, kd closest")
    assert ((res["prim"] >= 0) & host[np.maximum(res["prim"], 0)]).sum() > 20
    res_any = resolve_host_candidates_any(c.rays, occ, cands_any, cb)
    m = res_any != 2
    assert m.mean() > 0.99 and np.array_equal(res_any[m], c.any_hit[0][m])
    assert ((occ == 2) & (res_any == 1)).sum() > 5 and ((occ == 2) & (res_any == 0)).sum() > 5


@pytest.mark.gpu
def test_stack_spill_with_textured_leaves():
    """ss.kd_chain, 64 deep, with its tube triangles turned plain / constant alpha / textured: the new instances through
    the spill of the 8-entry window of the to-visit list"""
    k = ss.kd_chain(64, 44, "lean")
    n = len(k.prims)
    assert n == 65 and (k.prims["kind"] == 0).all()
    rng = np.random.default_rng(144)
    which = rng.integers(0, 4, n)
    sub = rng.integers(0, 4, n)
    prims = k.prims.copy()
    prims["kind"] = np.where(which == 0, 0, np.where(which == 1, 4 + sub, 16 + sub))
    alpha_const = rng.choice(np.array([0, .3, .7, 1], F), n)
    prims["v"][:, 3] = np.where(which == 0, 0, np.where(which == 1, alpha_const.view(np.int32), rng.integers(0, 3, n)))
    textures = ato.scene_textures(3)
    rays = ss.kd_chain_rays(1024, 5)
    with ob.pending_depth(len(rays)) as pd:
        ob.kd_closest(k.nodes, k.prim_indices, k.prims, k.verts, k.bounds, rays)
    assert pd.depth[:, 0].max() == 64 and (pd.depth[:, 0] > 8).mean() > 0.5  # the walks outgrow the window
    alpha, tex = ato.per_ray_alpha(prims, k.verts, k.uvs, textures, rays)
    per = KdPerRayOracle(k, prims, k.verts, rays, k.normals, alpha, tex)
    exp, any_exp = per.closest(), per.any_hit()
    share = ((exp["prim"] >= 0) & ato.is_textured(prims["kind"])[np.maximum(exp["prim"], 0)]).mean()
    print("textured closest hits", share, "above 8 pending", (pd.depth[:, 0] > 8).mean())
    assert share >= 0.25
    agg = KdTreeAggregate.from_tree(k.nodes, k.prim_indices, prims, k.verts, k.bounds, normals=k.normals, uvs=k.uvs,
                                    alpha_textures=textures)
    try:
        assert_device_equals(agg, rays, exp, any_exp)
    finally:
        agg.close()


@pytest.mark.gpu
def test_cpp_front_end_traces_through_both_routes(nnbvh_lib):
    out = subprocess.run([build_adapter_check(nnbvh_lib), "gpu"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "kd alpha texture adapter ok" in out.stdout, out.stdout + out.stderr
