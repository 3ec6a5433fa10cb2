"""Image-textured alpha on triangles (primitive kinds 16 .. 19, include/nnbvh.h): the C ABI's argument checks, the
arithmetic of nn_bvh_amd/csrc/alpha_texture_math.h against the numpy restatement of tests/alpha_texture_oracle.py
(host program here, one record per lane on the device), the per-ray oracle construction, and the device kernels
against it.  Everything is bit for bit; the only rule beside equality is that a NaN equals a NaN."""
import collections
import ctypes
import functools
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import alpha_texture_oracle as ato
import oracle_binding as ob
import scenes_small as ss
from ledger_cases import BVH, bvh, reaches
from nn_bvh_amd import AlphaTexture, BVHAggregate, NNBVHError, _lib, build, build_tree, scene
from nn_bvh_amd._lib import ptr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_SRC = os.path.join(ROOT, "tests", "cpp", "alpha_texture_check.cpp")
HOST_EXE = os.path.join(ROOT, "tests", "cpp", "alpha_texture_check")
DEV_SRC = os.path.join(ROOT, "tests", "hip", "alpha_texture_check.hip")
DEV_EXE = os.path.join(ROOT, "tests", "hip", "alpha_texture_check")
HEADER = os.path.join(build.CSRC, "alpha_texture_math.h")
NEW_CALLS = ("nnbvh_scene_create_with_alpha_textures", "nnbvh_scene_create_gpu_build_with_alpha_textures")
NO_DEVICE = 1 << 20  # a device index no machine has: a well-formed call gets as far as the device check
F = np.float32


def same_bits(a, b):
    """bit equality of float32 arrays, a NaN equal to a NaN"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


# ---- exports and refusals (CPU) -----------------------------------------------------------------------------------------
def test_calls_are_exported_prototyped_and_declared(nnbvh_lib):
    header = open(os.path.join(ROOT, "include", "nnbvh.h")).read()
    for name in NEW_CALLS:
        assert name in _lib.EXPORTS and hasattr(nnbvh_lib, name)
        assert re.search(r"nnbvh_scene \*" + name + r"\(", header), name
        assert getattr(nnbvh_lib, name).restype is ctypes.c_void_p and len(getattr(nnbvh_lib, name).argtypes) >= 12
    for k, name in enumerate(("", "_FLIPPED", "_SMOOTH", "_SMOOTH_FLIPPED")):
        assert re.search(rf"#define NNBVH_PRIM_ALPHATEX_TRIANGLE{name} {16 + k}\b", header)
    assert ctypes.sizeof(AlphaTexture) == 48  # the struct of the header, field for field
    fields = re.search(r"typedef struct nnbvh_alpha_texture \{(.*?)\} nnbvh_alpha_texture;", header, re.S).group(1)
    fields = re.sub(r"/\*.*?\*/", "", fields, flags=re.S)
    names = re.findall(r"(\w+)\s*[,;]", fields)
    assert names == [f[0] for f in AlphaTexture._fields_]


def small_scene(kind=16, n=12):
    verts, prims = ss.random_soup(n, 0, 3)
    prims = prims.copy()
    prims["kind"][::2] = kind
    prims["v"][::2, 3] = np.arange(len(prims[::2])) % 2
    return verts, prims


def raw_create(L, route, tree, prims, verts, textures, n_textures=None, normals=None, uvs=None, device=NO_DEVICE):
    table, n = _lib.alpha_texture_table(textures) if textures is not None else (None, 0)
    n = n if n_textures is None else n_textures
    opt = lambda a: ptr(a) if a is not None else None  # noqa: E731
    if route == "host_tree":
        return L.nnbvh_scene_create_with_alpha_textures(ptr(tree.nodes), len(tree.nodes), ptr(tree.ordered_prims),
                                                        len(prims), ptr(verts), opt(normals), opt(uvs), None, len(verts),
                                                        device, table, n)
    return L.nnbvh_scene_create_gpu_build_with_alpha_textures(ptr(prims), len(prims), ptr(verts), len(verts), None,
                                                              opt(normals), opt(uvs), None, 4, 0, device, table, n)


@pytest.mark.parametrize("route", ["host_tree", "device_build"])
def test_argument_faults_name_the_call_before_any_device_work(nnbvh_lib, route):
    L = nnbvh_lib
    call = NEW_CALLS[0 if route == "host_tree" else 1]
    verts, prims = small_scene()
    good = [AlphaTexture(np.ones((2, 3), F)), AlphaTexture(np.zeros((1, 1), F), wrap="black")]

    def refused(words, prims=prims, textures=good, **kw):
        tree = build_tree(prims, verts)
        assert not raw_create(L, route, tree, prims, verts, textures, **kw), words
        err = _lib.last_error()
        assert call in err and words in err, (words, err)

    # a well-formed call gets as far as the device check
    tree = build_tree(prims, verts)
    assert not raw_create(L, route, tree, prims, verts, good) and "no usable HIP device" in _lib.last_error()
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


def test_the_other_creation_calls_refuse_kind_16(nnbvh_lib):
    L = nnbvh_lib
    verts, prims = small_scene()
    tree = build_tree(prims, verts)  # a textured triangle is a triangle for the builders
    plain = prims.copy()
    plain["kind"] = 0
    assert build_tree(plain, verts).nodes.tobytes() == tree.nodes.tobytes()
    flat_calls = "nnbvh_scene_create_with_alpha_textures / nnbvh_scene_create_gpu_build_with_alpha_textures"
    op, n, nv = tree.ordered_prims, len(tree.nodes), len(verts)
    assert not L.nnbvh_scene_create(ptr(tree.nodes), n, ptr(op), len(op), ptr(verts), nv, NO_DEVICE)
    assert "unknown primitive kind" in _lib.last_error()
    assert not L.nnbvh_scene_create_with_attributes(ptr(tree.nodes), n, ptr(op), len(op), ptr(verts), None, None, None, nv,
                                                    NO_DEVICE)
    assert "unknown primitive kind" in _lib.last_error()
    assert not L.nnbvh_scene_create_gpu_build_with_attributes(ptr(prims), len(prims), ptr(verts), nv, None, None, None,
                                                              None, 4, 0, NO_DEVICE)
    assert "unknown primitive kind" in _lib.last_error()
    # two-level scenes: host-built trees and the device build
    assert not L.nnbvh_scene_create_instanced(ptr(tree.nodes), n, n, ptr(op), len(op), ptr(verts), nv, None, 0, NO_DEVICE)
    assert flat_calls in _lib.last_error()
    with pytest.raises(NNBVHError, match="alpha_textures / nnbvh_scene_create_gpu_build_with_alpha_textures"):
        BVHAggregate.build_two_level_on_device(prims[:0], verts, [prims], [(0, np.eye(4)[:3], np.eye(4)[:3])],
                                               device=NO_DEVICE)
    # kd scenes
    kd_nodes = np.zeros(1, _lib.KD_NODE_DTYPE)
    kd_nodes["flags"] = 3 | (1 << 2)
    bounds = np.concatenate([verts.min(0), verts.max(0)]).astype(F)
    assert not L.nnbvh_kd_scene_create(ptr(kd_nodes), 1, None, 0, ptr(prims), len(prims), ptr(verts), nv, ptr(bounds),
                                       NO_DEVICE)
    assert flat_calls in _lib.last_error()
    assert not L.nnbvh_kd_scene_create_gpu_build(ptr(prims), len(prims), ptr(verts), nv, None, 80, 1, 0.5, 1, -1, NO_DEVICE)
    assert flat_calls in _lib.last_error()


def test_python_front_end_checks_its_arguments():
    verts, prims = small_scene()
    tree = build_tree(prims, verts)
    with pytest.raises(NNBVHError, match="sequence of nn_bvh_amd.AlphaTexture"):
        BVHAggregate.from_tree(tree.nodes, tree.ordered_prims, verts, alpha_textures=[np.ones((2, 2), F)], device=NO_DEVICE)
    with pytest.raises(NNBVHError, match=r"\[height, width\]"):
        AlphaTexture(np.ones(4, F))
    with pytest.raises((AssertionError, ValueError)):
        BVHAggregate.from_tree(tree.nodes, tree.ordered_prims, verts, uvs=np.zeros((len(verts) - 1, 2), F),
                               alpha_textures=[AlphaTexture(np.ones((2, 2), F))] * 2, device=NO_DEVICE)
    with pytest.raises(ValueError):
        BVHAggregate.build_on_device(prims, verts, uvs=np.zeros((len(verts) - 1, 2), F),
                                     alpha_textures=[AlphaTexture(np.ones((2, 2), F))] * 2, device=NO_DEVICE)


ADAPTER_EXE = os.path.join(ROOT, "tests", "cpp", "alpha_texture_adapter_check")


def build_adapter_check(nnbvh_lib):
    libdir = os.path.join(ROOT, "nn_bvh_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), ADAPTER_EXE + ".cpp",
                    "-o", ADAPTER_EXE, "-pthread", "-L", libdir, "-l:libnnbvh_hip.so", f"-Wl,-rpath,{libdir}",
                    "-Wl,-rpath-link,/opt/rocm/lib"], check=True)
    return ADAPTER_EXE


def test_cpp_front_end_compiles_and_hands_its_arguments_over(nnbvh_lib):
    out = subprocess.run([build_adapter_check(nnbvh_lib)], capture_output=True, text=True)
    assert out.returncode == 0 and "alpha texture adapter ok (arguments)" in out.stdout, out.stdout + out.stderr


# ---- the header against the lookup ----------------------------------------------------------------------------------------
@functools.lru_cache(None)
def check_inputs():
    textures = ato.check_textures(0)
    ti, b, uv6 = ato.check_records(textures, 1)
    return textures, ti, b, uv6


def build_host_check():
    deps = [HOST_SRC, HEADER]
    if not (os.path.exists(HOST_EXE) and os.path.getmtime(HOST_EXE) >= max(os.path.getmtime(d) for d in deps)):
        flags = [f for f in build.CFLAGS if f != "-fPIC"]
        subprocess.run([build._hipcc()] + flags + ["-I", build.CSRC, HOST_SRC, "-o", HOST_EXE], check=True)
    return HOST_EXE


def run_check(exe, timeout=60):
    textures, ti, b, uv6 = check_inputs()
    with tempfile.TemporaryDirectory() as td:
        fi, fo = os.path.join(td, "i.bin"), os.path.join(td, "o.bin")
        ato.write_records(fi, textures, ti, b, uv6)
        out = subprocess.run([exe, fi, fo], capture_output=True, text=True, timeout=timeout)
        assert out.returncode == 0, f"{exe}: exit status {out.returncode}\n{out.stderr}"
        return np.fromfile(fo, np.uint32).view(F)


def test_header_equals_the_numpy_lookup_on_the_host():
    assert "-ffp-contract=off" in build.CFLAGS
    textures, ti, b, uv6 = check_inputs()
    got = run_check(build_host_check())
    exp = ato.lookup(textures, ti, b, uv6)
    bad = np.nonzero(~((got.view(np.uint32) == exp.view(np.uint32)) | (np.isnan(got) & np.isnan(exp))))[0]
    assert len(bad) == 0, (len(bad), [(int(ti[i]), b[i], uv6[i], got[i], exp[i]) for i in bad[:3]])
    bad_file = subprocess.run([HOST_EXE, os.devnull, os.devnull], capture_output=True, text=True)
    assert bad_file.returncode == 4 and "not a record file" in bad_file.stderr


def test_the_records_take_every_branch():
    textures, ti, b, uv6 = check_inputs()
    shapes = {(t.height, t.width) for t in textures}
    assert shapes == {(1, 1), (7, 1), (3, 5), (64, 64)}
    assert {t.wrap for t in textures} == {0, 1, 2} and {t.point_filter for t in textures} == {0, 1}
    assert {t.invert for t in textures} == {0, 1} and {t.scale for t in textures} == {0.5, 1.0, 2.0}
    assert {round(t.su, 4) for t in textures} == {1.0, 3.7, -2.0} == {round(t.sv, 4) for t in textures}
    assert any(t.du != 0 and t.dv != 0 for t in textures)
    shares = ato.branch_shares(textures, ti, b, uv6)
    print(shares)
    for name, share in shares.items():
        assert share > 0.01, (name, share)
    # the placements: exactly 0 and 1, texel centres (dx = 0), an ulp either side of an edge, the default corners
    u = (b[:, 0] * uv6[:, 0] + b[:, 1] * uv6[:, 2]) + b[:, 2] * uv6[:, 4]
    v = (b[:, 0] * uv6[:, 1] + b[:, 1] * uv6[:, 3]) + b[:, 2] * uv6[:, 5]
    assert ((u == 0) & (v == 0)).any() and ((u == 1) & (v == 1)).any() and ((u == 0) & (v == 1)).any()
    assert (uv6 == ato.DEFAULT_UV).all(1).mean() > 0.1
    on_centre = on_edge = below = above = 0
    for k, t in enumerate(textures):
        if t.point_filter:
            continue
        m = ti == k
        s, tt = ato.uv_to_st(t, u[m], v[m])
        x = s * F(t.width) - F(0.5)
        on_centre += int((x == np.floor(x)).sum())
        e = s * F(t.width)
        r = np.round(e)
        on_edge += int((e == r).sum())
        below += int(((e < r) & (r - e < 1e-5 * np.maximum(np.abs(r), 1))).sum())
        above += int(((e > r) & (e - r < 1e-5 * np.maximum(np.abs(r), 1))).sum())
    assert min(on_centre, on_edge, below, above) > 20, (on_centre, on_edge, below, above)


# ---- the oracle construction itself -----------------------------------------------------------------------------------------
def mixed_soup(seed=5, n=600, uv_seed=None):
    """a third each plain, constant alpha (kinds 4 .. 7 over ss.ALPHAS) and textured (kinds 16 .. 19)"""
    verts, prims = ss.random_soup(n, 0, seed, extent=4.0, size=1.5)
    rng = np.random.default_rng(seed + 1)
    prims = prims.copy()
    which = rng.integers(0, 3, len(prims))
    sub = rng.integers(0, 4, len(prims))
    prims["kind"] = np.where(which == 0, 0, np.where(which == 1, 4 + sub, 16 + sub))
    alpha = rng.choice(ss.ALPHAS, len(prims))
    prims["v"][:, 3] = np.where(which == 1, alpha.view(np.int32), np.where(which == 2, rng.integers(0, 3, len(prims)), 0))
    normals = rng.normal(size=(len(verts), 3)).astype(F)
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    uvs = rng.uniform(-0.5, 1.5, (len(verts), 2)).astype(F)
    return verts, prims, normals, uvs


def grid_scene(seed=2):
    """ss.grid_mesh(24) with shared-vertex (u, v): two thirds of the triangles textured, the rest plain / constant"""
    verts, prims = ss.grid_mesh(24, seed)
    rng = np.random.default_rng(seed + 9)
    prims = prims.copy()
    which = rng.integers(0, 6, len(prims))
    sub = rng.integers(0, 4, len(prims))
    prims["kind"] = np.where(which == 0, 0, np.where(which == 1, 4 + sub, 16 + sub))
    alpha = rng.choice(ss.ALPHAS, len(prims))
    prims["v"][:, 3] = np.where(which == 1, alpha.view(np.int32), np.where(which >= 2, rng.integers(0, 3, len(prims)), 0))
    normals = rng.normal(size=(len(verts), 3)).astype(F) + np.array([0, 2, 0], F)
    normals /= np.linalg.norm(normals, axis=1, keepdims=True)
    uvs = ((verts[:, [0, 2]] + 5) / 10).astype(F)  # the height field's own parametrisation
    return verts, prims, normals, uvs


def scene_rays(verts, prims, seed, n_random=1024):
    return np.concatenate([ss.edge_case_rays(verts, prims, seed, 2048),
                           scene.random_rays(n_random, verts.min(0) - 1, verts.max(0) + 1, seed + 1)])


def test_per_ray_oracle_with_constant_zero_textures_is_the_kind_4_oracle():
    """a constant 0 gives exactly 0 through the bilinear sum: the construction must then agree with the oracle's own
    constant-alpha path on the whole batch"""
    verts, prims, normals, uvs = mixed_soup()
    zero = [AlphaTexture(np.zeros(s, F), wrap=w, point_filter=p) for s, w, p in (((5, 3), "repeat", False),
                                                                                 ((1, 1), "clamp", False),
                                                                                 ((7, 9), "black", True))]
    tree = build_tree(prims, verts, 4)
    rays = scene_rays(verts, prims, 3, 512)
    per = ato.PerRayOracle(tree.nodes, tree.ordered_prims, verts, uvs, zero, rays, normals)
    assert (per.alpha == 0).all() and not np.signbit(per.alpha).any()
    const = ato.constant_prims(tree.ordered_prims, per.tex, np.zeros(len(per.tex), F))
    try:
        ob.set_vertex_normals(normals)
        exp = ob.closest(tree.nodes, const, verts, rays)
        eo, ev, et = ob.any_hit(tree.nodes, const, verts, rays)
    finally:
        ob.set_vertex_normals(None)
    assert per.closest().tobytes() == exp.tobytes()
    occ, vis, tst = per.any_hit()
    assert np.array_equal(occ, eo) and np.array_equal(vis, ev) and np.array_equal(tst, et)
    textured = ato.is_textured(prims["kind"])
    assert not textured[np.maximum(exp["prim"], 0)][exp["prim"] >= 0].any()  # alpha 0: never hit


# ---- the expected results of the GPU tests, computed once ---------------------------------------------------------------
Case = collections.namedtuple("Case", "verts prims normals uvs textures tree rays closest any_hit alpha tex")


@functools.lru_cache(None)
def case(name, max_prims, with_uvs=True):
    verts, prims, normals, uvs = mixed_soup() if name == "soup" else grid_scene()
    textures = ato.scene_textures(0)
    tree = build_tree(prims, verts, max_prims)
    rays = scene_rays(verts, prims, 7 if name == "soup" else 11)
    uv = uvs if with_uvs else None
    per = ato.PerRayOracle(tree.nodes, tree.ordered_prims, verts, uv, textures, rays, normals)
    return Case(verts, prims, normals, uv, textures, tree, rays, per.closest(), per.any_hit(), per.alpha, per.tex)


def alpha_test_shares(c):
    """of the rays: the alpha test of a textured triangle rejected a hit / accepted one after evaluating 0 < a < 1.
    From the oracle alone: the alpha of the hit that stands is a[i][j]."""
    op = c.tree.ordered_prims
    pos_of_id = np.full(op["id"].max() + 1, -1)
    pos_of_id[op["id"]] = np.arange(len(op))
    col_of_pos = np.full(len(op), -1)
    col_of_pos[c.tex] = np.arange(len(c.tex))
    hit = c.closest["prim"] >= 0
    col = col_of_pos[pos_of_id[np.maximum(c.closest["prim"], 0)]]
    a_hit = c.alpha[np.arange(len(c.rays)), np.maximum(col, 0)]
    accepted_mid = hit & (col >= 0) & (a_hit > 0) & (a_hit < 1)
    # rejected: the record differs from the one the same scene gives with every textured triangle opaque (alpha 1);
    # the two walks are the same until the first textured hit that the alpha test rejects
    opaque = ato.constant_prims(op, c.tex, np.ones(len(c.tex), F))
    try:
        ob.set_vertex_normals(c.normals)
        h0 = ob.closest(c.tree.nodes, opaque, c.verts, c.rays)
    finally:
        ob.set_vertex_normals(None)
    rejected = np.array([c.closest[i].tobytes() != h0[i].tobytes() for i in range(len(c.rays))])
    return rejected.mean(), accepted_mid.mean()


@pytest.mark.parametrize("name", ["soup", "grid"])
def test_the_oracle_alone_rejects_and_accepts_enough(name):
    rejected, accepted_mid = alpha_test_shares(case(name, 4))
    print(name, "rejected", rejected, "accepted with 0 < a < 1", accepted_mid)
    assert rejected >= 0.10 and accepted_mid >= 0.10


# ---- GPU: the kernels against the per-ray oracle ---------------------------------------------------------------------------
CASES = [("soup", 4, True), ("soup", 1, True), ("soup", 4, False), ("grid", 4, True), ("grid", 1, True), ("grid", 4, False)]
# case -> (kernel family, the instances its device calls launch), asserted by `reaches` (tests/ledger_cases.py): the
# ALPHA = 3 instances <M,8,0,1,3> and, beside host-only primitives, their HOSTC twins <0/2,8,0,1,3,0,1>
LEDGER = {f"test_device_equals_the_per_ray_oracle[{name}-{max_prims}-{with_uvs}-{route}]": (BVH, bvh((0, 1, 2), alpha=3))
          for name, max_prims, with_uvs in CASES for route in ("host_tree", "device_build")}
LEDGER.update({
    # an alpha scene has no mode-3 form: the batches and the gathered queues run as modes 0 and 2
    "test_batches_call_and_wavefront_queues": (BVH, bvh((0, 2), alpha=3)),
    # the plain Intersect beside the two candidate calls
    "test_mixed_with_host_only_primitives_through_candidates": (BVH, bvh((0, 2), alpha=3, hostc=1) | bvh((0,), alpha=3)),
})


def make_aggregate(c, route, max_prims):
    if route == "host_tree":
        return BVHAggregate.from_tree(c.tree.nodes, c.tree.ordered_prims, c.verts, normals=c.normals, uvs=c.uvs,
                                      alpha_textures=c.textures)
    return BVHAggregate.build_on_device(c.prims, c.verts, max_prims, "sah", normals=c.normals, uvs=c.uvs,
                                        alpha_textures=c.textures)


def first_bad(got, exp):
    return [i for i in range(len(exp)) if got[i].tobytes() != exp[i].tobytes()][:5]


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["host_tree", "device_build"])
@pytest.mark.parametrize("name,max_prims,with_uvs", CASES)
def test_device_equals_the_per_ray_oracle(name, max_prims, with_uvs, route):
    """closest (prim, t, b, both counters, void mark), any hit with counts (mode 1) and without (mode 2)"""
    c = case(name, max_prims, with_uvs)
    with reaches(LEDGER, f"test_device_equals_the_per_ray_oracle[{name}-{max_prims}-{with_uvs}-{route}]"):
        agg = make_aggregate(c, route, max_prims)
        try:
            got = agg.Intersect(c.rays)
            assert got.tobytes() == c.closest.tobytes(), first_bad(got, c.closest)
            eo, ev, et = c.any_hit
            occ, vis, tst = agg.IntersectP(c.rays, counts=True)
            assert np.array_equal(occ, eo) and np.array_equal(vis, ev) and np.array_equal(tst, et)
            assert np.array_equal(agg.IntersectP(c.rays), eo)
            for k in (1, 63, 64, 65, 257):  # batches below, at and above one wavefront, and above one block
                assert agg.Intersect(c.rays[:k]).tobytes() == c.closest[:k].tobytes(), k
                assert np.array_equal(agg.IntersectP(c.rays[:k]), eo[:k]), k
                o2, v2, t2 = agg.IntersectP(c.rays[-k:], counts=True)
                assert np.array_equal(o2, eo[-k:]) and np.array_equal(v2, ev[-k:]) and np.array_equal(t2, et[-k:]), k
        finally:
            agg.close()
    textured = ato.is_textured(c.prims["kind"])
    assert (textured[np.maximum(c.closest["prim"], 0)] & (c.closest["prim"] >= 0)).mean() > 0.1


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["soup", "grid"])
def test_creation_routes_make_the_same_bytes(name):
    c = case(name, 4, True)
    a, b = make_aggregate(c, "host_tree", 4), make_aggregate(c, "device_build", 4)
    try:
        for what in (0, 1, 3, 4):
            assert a.read(what).tobytes() == b.read(what).tobytes(), what
        assert all(np.array_equal(x, y) for x, y in zip(a.Bounds(), b.Bounds()))
        assert a.info == b.info
        # the table is the descriptors in order, the pool the images one after another
        pool = np.concatenate([t.image.reshape(-1) for t in c.textures])
        assert a.read(4).tobytes() == pool.tobytes()
        table = a.read(3)
        assert [int(r[2]) for r in table] == [t.width for t in c.textures] and list(table[:, 0]) == [0, 15, 15 + 256]
        # a textured triangle takes 5 slots (8 with normals) where a constant-alpha one takes 3 (6)
        kinds = c.prims["kind"]
        slots = 3 * len(kinds) + 3 * (np.isin(kinds, (6, 7, 18, 19))).sum() + 2 * ato.is_textured(kinds).sum()
        assert a.info["prim_slots"] == slots
    finally:
        a.close()
        b.close()


@pytest.mark.gpu
def test_batches_call_and_wavefront_queues():
    """nnbvh_trace_batches_device (a closest and an any-hit batch: separate launches for an alpha scene) and
    nnbvh_wavefront_intersect_closest_and_shadow (the closest queue's rays carry tMax = Infinity)"""
    import torch
    from nn_bvh_amd.wavefront import RayQueue, WavefrontAggregate, WorkQueue
    from test_wavefront import QUEUES, shadow_inputs
    c = case("soup", 4, True)
    dev = torch.device("cuda", 0)
    with reaches(LEDGER, "test_batches_call_and_wavefront_queues"):
        agg = make_aggregate(c, "host_tree", 4)
        try:
            n = len(c.rays)
            d_rays = torch.from_numpy(c.rays.view(np.uint8).reshape(n, 32)).to(dev)
            d_hits = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
            d_occ = torch.full((n,), 9, dtype=torch.uint8, device=dev)
            agg.trace_batches_device([("closest", d_rays.data_ptr(), n, d_hits.data_ptr()),
                                      ("any", d_rays.data_ptr(), n, d_occ.data_ptr())])
            torch.cuda.synchronize()
            got = d_hits.cpu().numpy().view(_lib.HIT_DTYPE).reshape(-1)
            assert got.tobytes() == c.closest.tobytes(), first_bad(got, c.closest)
            assert np.array_equal(d_occ.cpu().numpy(), c.any_hit[0])
            # the wavefront call: the same rays without their tMax in the closest queue, with it in the shadow queue
            far = c.rays.copy()
            far["tmax"] = np.inf
            per = ato.PerRayOracle.__new__(ato.PerRayOracle)
            per.nodes, per.prims, per.verts, per.rays = c.tree.nodes, np.ascontiguousarray(c.tree.ordered_prims), c.verts, far
            per.normals, per.alpha, per.tex = c.normals, c.alpha, c.tex  # alpha does not depend on tMax
            exp_far = per.closest()
            Ld, r_u, r_l, px, L = shadow_inputs(n, n + 100, 7)
            t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
            rq, sq = RayQueue.from_records(far, dev), RayQueue.from_records(c.rays, dev, shadow=True)
            wf = WavefrontAggregate(agg)
            queues = {k: WorkQueue(n, dev) for k in QUEUES}
            hits_t = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
            L_t, occ_t = t(L), torch.full((n,), 9, dtype=torch.uint8, device=dev)
            wf.IntersectClosestAndShadow(n, rq, n, sq, t(Ld), t(r_u), t(r_l), t(px), L_t, hits=hits_t, occluded=occ_t, **queues)
            torch.cuda.synchronize()
            got = hits_t.cpu().numpy().view(_lib.HIT_DTYPE).reshape(-1)
            assert got.tobytes() == exp_far.tobytes(), first_bad(got, exp_far)
            assert np.array_equal(occ_t.cpu().numpy(), c.any_hit[0])
            expL = ob.record_shadow(c.any_hit[0], Ld, r_u, r_l, px, L)
            assert np.array_equal(L_t.cpu().numpy().view(np.uint32), expL.view(np.uint32))
        finally:
            agg.close()


@pytest.mark.gpu
def test_mixed_with_host_only_primitives_through_candidates():
    """every third plain triangle declared host-only with its exact bounds: the candidate calls (the HOSTC twins),
    resolved with the oracle's triangle test, equal the per-ray oracle of the scene with them as triangles"""
    from nn_bvh_amd import resolve_host_candidates, resolve_host_candidates_any
    from test_host_candidates import assert_resolved_equal, tri_callback, tri_table
    c = case("soup", 4, True)
    host = (c.prims["kind"] == 0) & (np.arange(len(c.prims)) % 3 == 0)
    tri = c.verts[c.prims["v"][:, :3]]
    bounds = np.concatenate([tri.min(1), tri.max(1)], 1).astype(F)
    hp = c.prims.copy()
    hp["kind"][host] = 3
    tree_h = build_tree(hp, c.verts, 4, prim_bounds=bounds)
    assert tree_h.nodes.tobytes() == c.tree.nodes.tobytes()
    assert np.array_equal(tree_h.ordered_prims["id"], c.tree.ordered_prims["id"])
    agg = BVHAggregate.from_tree(tree_h.nodes, tree_h.ordered_prims, c.verts, normals=c.normals, uvs=c.uvs,
                                 alpha_textures=c.textures)
    try:
        with reaches(LEDGER, "test_mixed_with_host_only_primitives_through_candidates"):
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
    assert_resolved_equal(res[ok], c.closest[ok], "textured alpha with host-only primitives, closest")
    assert ((res["prim"] >= 0) & host[np.maximum(res["prim"], 0)]).sum() > 20
    res_any = resolve_host_candidates_any(c.rays, occ, cands_any, cb)
    m = res_any != 2
    assert m.mean() > 0.99 and np.array_equal(res_any[m], c.any_hit[0][m])
    assert ((occ == 2) & (res_any == 1)).sum() > 5 and ((occ == 2) & (res_any == 0)).sum() > 5


@pytest.mark.gpu
def test_device_arithmetic_one_record_per_lane(nnbvh_lib):
    """tests/hip/alpha_texture_check.hip: the CPU test's record file through the header on the device, in a fresh child
    process with a time limit of its own; its output equals the host program's"""
    deps = [DEV_SRC, HEADER]
    if not (os.path.exists(DEV_EXE) and os.path.getmtime(DEV_EXE) >= max(os.path.getmtime(d) for d in deps)):
        subprocess.run([build._hipcc()] + [f for f in build.CFLAGS if f != "-fPIC"] + ["-I", build.CSRC, DEV_SRC, "-o", DEV_EXE],
                       check=True)
    host = run_check(build_host_check())
    device = run_check(DEV_EXE, timeout=40)
    assert same_bits(device, host), np.nonzero(device.view(np.uint32) != host.view(np.uint32))[0][:5]


@pytest.mark.gpu
def test_cpp_front_end_traces_through_both_routes(nnbvh_lib):
    out = subprocess.run([build_adapter_check(nnbvh_lib), "gpu"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "alpha texture adapter ok" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_stack_spill_with_textured_leaves():
    """ss.chain_tree's alpha-triangle chain, 64 deep, with the leaves' alpha-tested triangles turned textured: the new
    instances through the spill of the 8-entry stack window"""
    rng = np.random.default_rng(43)  # (a seed whose chain puts textured triangles on the axis: most rays meet one)
    ch = ss.chain_tree(64, rng, tube=True, leaves="alpha_tri", extras=True)
    prims = ch.prims.copy()
    was_alpha = prims["kind"] >= 4
    prims["kind"][was_alpha] += 12
    prims["v"][was_alpha, 3] = rng.integers(0, 3, was_alpha.sum())
    textures = ato.scene_textures(3)
    rays = ss.chain_rays(float(ch.verts[:, 0].max()), 1024, 5)
    with ob.pending_depth(len(rays)) as pd:
        plain = prims.copy()
        plain["kind"], plain["v"][:, 3] = 0, 0
        ob.closest(ch.nodes, plain, ch.verts, rays)
    assert pd.depth[:, 0].max() == 64 and (pd.depth[:, 0] > 8).mean() > 0.5  # the walks outgrow the window
    per = ato.PerRayOracle(ch.nodes, prims, ch.verts, ch.uvs, textures, rays, ch.normals)
    exp, (eo, ev, et) = per.closest(), per.any_hit()
    agg = BVHAggregate.from_tree(ch.nodes, prims, ch.verts, normals=ch.normals, uvs=ch.uvs, alpha_textures=textures)
    try:
        got = agg.Intersect(rays)
        assert got.tobytes() == exp.tobytes(), first_bad(got, exp)
        occ, vis, tst = agg.IntersectP(rays, counts=True)
        assert np.array_equal(occ, eo) and np.array_equal(vis, ev) and np.array_equal(tst, et)
        assert np.array_equal(agg.IntersectP(rays), eo)
    finally:
        agg.close()
    assert ((exp["prim"] >= 0) & ato.is_textured(prims["kind"])[np.maximum(exp["prim"], 0)]).mean() > 0.25
    assert (exp["prim_tests"] > 65).mean() > 0.1  # rejected hits: each is re-tested
