"""Hits inside instances -> SurfaceInteraction, every attribute mix, against the composed oracle.

surface_interaction<FULL = true> (csrc/interaction_math.h) is the branch every instanced, animated or
patch-carrying scene goes through.  Here it gets synthetic hits — one private triangle or patch per golden-style
input record, hits["prim"] = arange(n), hits["instance"] = k + 1 — so that all 16 flag mixes, the degenerate
parameterisations, zero normals, slivers and the other rare branches of tests/golden/interaction_cases.py run
inside rigid, scaled, mirrored and far-away instances and inside AnimatedPrimitives.  Expected values:
test_interaction.instance_oracle, the composition of pieces that are each pinned to the compiled reference
(ob.triangle_ / patch_ / transform_interaction_batch, ob.anim_interpolate).  Every device comparison is bit for
bit; the one float64 comparison (CPU) guards the composition itself."""
import functools
import os

import numpy as np
import pytest

import oracle_binding as ob
import test_animated as ta
from interaction_cases import cases, patch_cases
from test_interaction import (GOLDEN, HERE, assert_interaction_fields, assert_records_equal, instance_oracle,
                              mesh_from_records)

XF_KINDS = ("identity", "rigid", "scale", "mirror1", "mirror3", "far")
PATCH_FLAGS = (0, 1, 2, 3, 8, 9, 10, 11)


# ---------------------------------------------------------------------------------------- inputs
def _rot(axis, ang):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) * np.cos(ang) + np.sin(ang) * K + (1 - np.cos(ang)) * np.outer(a, a)


@functools.lru_cache(None)
def instance_transforms():
    """(m, mi), float32 [6, 3, 4] each, in the order of XF_KINDS: renderFromPrimitive and the float64 inverse of
    the float32 matrix, rounded.  The mirrored ones have a negative determinant (asserted in float64)."""
    r1, r2 = _rot([1, 2, 3], 0.7), _rot([-2, 1, 0.5], 2.1)
    parts = {"identity": (np.eye(3), [0, 0, 0]),
             "rigid": (r1, [3, -2, 5]),
             "scale": (r2 @ np.diag([0.25, 3.0, 1.5]), [-4, 1, 2]),
             "mirror1": (r1 @ np.diag([-1.5, 1.0, 0.5]), [1, 2, -3]),
             "mirror3": (r2 @ np.diag([-1.0, -2.0, -0.4]), [-2, 4, 1]),
             "far": (r2, [1200, -900, 1500])}
    m = np.zeros((len(XF_KINDS), 3, 4), np.float32)
    mi = np.zeros_like(m)
    for k, name in enumerate(XF_KINDS):
        m[k, :, :3], m[k, :, 3] = parts[name]
        m44 = np.eye(4)
        m44[:3] = m[k].astype(np.float64)
        mi[k] = np.linalg.inv(m44)[:3]
        det = np.linalg.det(m[k, :, :3].astype(np.float64))
        assert (det < 0) == name.startswith("mirror"), (name, det)
    return m, mi


def instance_table(m, mi):
    from nn_bvh_amd import _lib
    inst = np.zeros(len(m), _lib.INSTANCE_DTYPE)
    inst["render_from_prim"], inst["prim_from_render"] = m.reshape(-1, 12), mi.reshape(-1, 12)
    return inst


@functools.lru_cache(None)
def tri_records():
    """All committed triangle inputs + one further seed of the generator."""
    return np.concatenate([np.load(GOLDEN)["inputs"], cases(2048, 31)])


@functools.lru_cache(None)
def patch_records():
    return np.concatenate([np.load(os.path.join(HERE, "golden", "blp_interaction.npz"))["inputs"],
                           patch_cases(2048, 32)])


@functools.lru_cache(None)
def animated_table():
    """(anims, oa, instances): three AnimatedTransforms of each kind of golden/make_anim_golden.py's generator
    (general, translation only, small rotation, rotation beyond 90 degrees, not animated, rigid), decomposed by
    the reference's constructor, with the time ranges they were drawn with; the instance table holds the start
    transforms, as a scene's does."""
    from nn_bvh_amd import _lib
    g = np.load(os.path.join(HERE, "golden", "anim_interpolate.npz"))
    a_all = ta.anims_from_reference_output(g["inputs"], g["outputs"])
    oa = a_all[np.arange(18)].copy()  # the generator's kind is the record number modulo 6
    anims = np.zeros(len(oa), _lib.ANIMATED_DTYPE)
    for f_o, f_p in (("start_m", "start_from"), ("start_minv", "start_inv"), ("end_m", "end_from"), ("end_minv", "end_inv")):
        anims[f_p] = oa[f_o]
    for f in ("T", "R", "S", "start_time", "end_time", "actually_animated"):
        anims[f] = oa[f]
    same_r = (oa["R"][:, 0] == oa["R"][:, 1]).all(1)
    animated = oa["actually_animated"] != 0
    assert (~animated).any(), "an entry that is not actually animated"
    assert (animated & same_r & (oa["T"][:, 0] != oa["T"][:, 1]).any(1)).any(), "a translation-only entry"
    assert (animated & ~same_r).any(), "a rotating entry"
    inst = instance_table(oa["start_m"].reshape(-1, 4, 4)[:, :3], oa["start_minv"].reshape(-1, 4, 4)[:, :3])
    return anims, oa, inst


def interpolated(oa, k, times):
    """Interpolate(time) of entries oa[k] as the device evaluates it: m, mi [n, 3, 4]."""
    try:
        ob.set_sin_mode(1)  # the path's one documented exception: the two Slerp sines in fp64, rounded once
        mm = ob.anim_interpolate(oa[k], times)
    finally:
        ob.set_sin_mode(0)
    return mm[:, :16].reshape(-1, 4, 4)[:, :3, :], mm[:, 16:].reshape(-1, 4, 4)[:, :3, :]


def times_around_ranges(oa, n, seed):
    """Entry and ray time per row: every entry sees times below, exactly at, strictly inside (four rows of
    eight), exactly at the other end of and above its time range."""
    k = (np.arange(n) // 8) % len(oa)
    cat = np.arange(n) % 8
    t0, t1 = oa["start_time"][k], oa["end_time"][k]
    f = np.random.default_rng(seed).uniform(0.05, 0.95, n).astype(np.float32)
    t = (t0 + f * (t1 - t0)).astype(np.float32)
    t = np.where(cat == 0, t0 - np.float32(0.25), t)
    t = np.where(cat == 1, t0, t)
    t = np.where(cat == 2, t1, t)
    t = np.where(cat == 3, t1 + np.float32(0.25), t).astype(np.float32)
    inside = (t > t0) & (t < t1)
    assert (inside == (cat >= 4)).all()
    for c in range(8):
        assert len(np.unique(k[cat == c])) == len(oa)
    return k, t, inside & (oa["actually_animated"][k] != 0)


def patch_mesh_from_records(rec):
    """One bilinear patch with four private vertices per record; attributes as BilinearPatchMesh stores them."""
    from nn_bvh_amd import _lib
    n = len(rec)
    flags_in = rec[:, 18].astype(np.int32)
    normals = rec[:, 27:39].reshape(-1, 3).copy()
    normals[np.repeat((flags_in & 8) != 0, 4)] *= -1  # util/mesh.cpp:216-223
    tri_flags = (((flags_in & 1) != 0) * _lib.TRI_HAS_UV + ((flags_in & 2) != 0) * _lib.TRI_HAS_N +
                 ((flags_in & 8) != 0) * _lib.TRI_FLIP_NORMAL).astype(np.uint8)
    return dict(verts=rec[:, 0:12].reshape(-1, 3), tri_vertices=np.full((n, 3), -1, np.int32), normals=normals,
                uvs=rec[:, 19:27].reshape(-1, 2), face_indices=7 + np.arange(n, dtype=np.int32),
                tri_flags=tri_flags, patch_vertices=np.arange(4 * n, dtype=np.int32).reshape(n, 4))


def synthetic_hits(kind, rec, instance):
    """Hit record i = primitive i struck where record i says, inside instance `instance` - 1 (0: top level)."""
    from nn_bvh_amd import HIT_DTYPE
    hits = np.zeros(len(rec), HIT_DTYPE)
    hits["prim"] = np.arange(len(rec))
    if kind == 0:
        hits["b0"], hits["b1"], hits["b2"] = rec[:, 9], rec[:, 10], rec[:, 11]
    else:
        hits["b0"], hits["b1"] = rec[:, 12], rec[:, 13]
    hits["t"] = 1.0
    hits["instance"] = instance
    return hits


def render_rays(kind, rec, m=None, time=None):
    """Rays whose direction is the record's -wo carried to render space by m ([n, 3, 4]; None: top level)."""
    from nn_bvh_amd import RAY_DTYPE
    rays = np.zeros(len(rec), RAY_DTYPE)
    d = -(rec[:, 12:15] if kind == 0 else rec[:, 14:17])
    if m is not None:
        d = np.stack([(m[:, i, 0] * d[:, 0] + m[:, i, 1] * d[:, 1]) + m[:, i, 2] * d[:, 2] for i in range(3)], 1)
    rays["d"] = d
    rays["time"] = (rec[:, 18] if kind == 0 else rec[:, 17]) if time is None else time
    return rays


def run_device(mesh, rays, hits, soa_size=None):
    """nnbvh_triangle_interactions_device into records pre-filled with 0x5A; rays as records, or (soa_size
    given) as an SOA queue whose device-side size is soa_size.  Returns the output's bytes [n, 192]."""
    import torch
    from nn_bvh_amd.wavefront import RayQueue
    dev = torch.device("cuda", 0)
    n = len(hits)
    hits_t = torch.from_numpy(np.ascontiguousarray(hits).view(np.uint8).reshape(n, 32)).to(dev)
    out = torch.full((n * 192,), 0x5A, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    if soa_size is None:
        rays_t = torch.from_numpy(np.ascontiguousarray(rays).view(np.uint8).reshape(n, 32)).to(dev)
        mesh.interactions_device(hits_t.data_ptr(), n, out.data_ptr(), d_rays=rays_t.data_ptr(), stream=stream)
    else:
        rq = RayQueue.from_records(rays, dev)
        rq.time = torch.from_numpy(np.ascontiguousarray(rays["time"])).to(dev)
        rq.size.fill_(soa_size)
        mesh.interactions_device(hits_t.data_ptr(), n, out.data_ptr(), ray_queue=rq, d_size=rq.size.data_ptr(),
                                 stream=stream)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(n, 192)


def as_records(raw):
    from nn_bvh_amd import _lib
    return np.ascontiguousarray(raw).reshape(-1).view(_lib.INTERACTION_DTYPE)


def assert_all_pairs(flags, kidx, flag_set, n_kinds):
    seen = set(zip(flags.astype(int).tolist(), kidx.tolist()))
    missing = [(f, k) for f in flag_set for k in range(n_kinds) if (f, k) not in seen]
    assert not missing, f"(flag, transform kind) pairs without a record: {missing}"


def mesh_of(kind, rec):
    return mesh_from_records(rec) if kind == 0 else patch_mesh_from_records(rec)


def flags_of(kind, rec):
    return rec[:, 19 if kind == 0 else 18].astype(np.int32)


# ------------------------------------------------------------------- CPU: the composition itself
# Worst relative deviation of the composed float32 oracle from the float64 computation below, measured over the
# seeded inputs of the guard (cases(600, 77) without the excluded kinds, patch_cases(300, 78), six transforms):
# 2.16e-7, the sine between a triangle's n and the normal of the transformed vertices; every other field stays
# below 1.5e-7.  The bound is 4 x the measured value: the inputs are fixed.  A column mix-up in instance_oracle's
# mapping shows as a deviation of order 1.
F64_MEASURED = 2.16e-7
F64_BOUND = 4 * F64_MEASURED


def excluded_from_the_guard(rec, kind):
    """Slivers (kind 12: the normal of the transformed vertices is ill-conditioned) and the degenerate
    parameterisations (kinds 3 and 14: one uv for all three vertices) where the mesh's uv are in use: left out of
    the float64 guard, and only of it.  The collinear, tiny and stretched parameterisations stay in."""
    return (kind == 12) | (np.isin(kind, (3, 14)) & ((rec[:, 19].astype(np.int32) & 1) != 0))


def f64_deviation(kind, rec):
    """Worst relative deviation per field of instance_oracle from float64, rows cycling through XF_KINDS."""
    n = len(rec)
    m_all, mi_all = instance_transforms()
    kidx = np.arange(n) % len(XF_KINDS)
    m, mi = m_all[kidx], mi_all[kidx]
    rays = render_rays(kind, rec, m)
    exp = instance_oracle(kind, rec, m, mi, rays["d"], rays["time"])
    d = rays["d"]
    d_in = np.stack([(mi[:, i, 0] * d[:, 0] + mi[:, i, 1] * d[:, 1]) + mi[:, i, 2] * d[:, 2] for i in range(3)], 1)
    local = instance_oracle(kind, rec, None, None, d_in, rays["time"])   # the shape's own interaction
    for name in ("uv", "time", "face_index"):
        assert np.array_equal(exp[name], local[name]), name
    assert np.array_equal(exp["time"], rays["time"]) and np.array_equal(exp["face_index"], 7 + np.arange(n))
    M, Mi = m.astype(np.float64), mi.astype(np.float64)
    fwd = lambda v: np.einsum("nij,nj->ni", M[:, :, :3], v.astype(np.float64))          # noqa: E731
    nrm = lambda v: np.einsum("nji,nj->ni", Mi[:, :, :3], v.astype(np.float64))         # noqa: E731
    unit = lambda v: v / np.linalg.norm(v, axis=1, keepdims=True)                        # noqa: E731
    sine = lambda a, b64: np.linalg.norm(np.cross(a.astype(np.float64), b64), axis=1)    # noqa: E731
    dev = {}
    if kind == 0:
        P = rec[:, 0:9].reshape(n, 3, 3).astype(np.float64)
        b = rec[:, 9:12].astype(np.float64)
        p64 = fwd(np.einsum("ni,nij->nj", b, P)) + M[:, :, 3]
        V = np.einsum("nij,nvj->nvi", M[:, :, :3], P) + M[:, None, :, 3]   # the explicitly transformed vertices
        dev["n"] = sine(exp["n"], unit(np.cross(V[:, 0] - V[:, 2], V[:, 1] - V[:, 2])))
        assert not exp["dndu"].any() and not exp["dndv"].any()  # Normal3f() stays zero
    else:
        P = rec[:, 0:12].reshape(n, 4, 3).astype(np.float64)
        u, v = rec[:, 12:13].astype(np.float64), rec[:, 13:14].astype(np.float64)
        p64 = fwd((1 - u) * ((1 - v) * P[:, 0] + v * P[:, 2]) + u * ((1 - v) * P[:, 1] + v * P[:, 3])) + M[:, :, 3]
        dev["n"] = sine(exp["n"], unit(nrm(local["n"])))
    widen = np.abs(p64) * 2.0 ** -24  # the rounding of the float64 point to float32
    assert (exp["pi_lo"] - widen <= p64).all() and (p64 <= exp["pi_hi"] + widen).all()
    assert (exp["pi_lo"] <= exp["pi_hi"]).all()
    dev["ns"] = sine(exp["ns"], unit(nrm(local["ns"])))
    dev["wo"] = np.linalg.norm(exp["wo"] - unit(-d.astype(np.float64)), axis=1)
    for name, f in (("dpdu", fwd), ("dpdv", fwd), ("dpdus", fwd), ("dpdvs", fwd), ("dndus", nrm), ("dndvs", nrm),
                    ("dndu", nrm), ("dndv", nrm)):
        ref = f(local[name])
        size = np.linalg.norm(ref, axis=1)
        diff = np.linalg.norm(exp[name] - ref, axis=1)
        assert (diff[size == 0] == 0).all(), name
        dev[name] = np.where(size > 0, diff / np.where(size > 0, size, 1), 0)
    for name in ("n", "ns", "wo"):  # unit vectors after the transform
        dev[name + " length"] = np.abs(np.linalg.norm(exp[name].astype(np.float64), axis=1) - 1)
    return {k: float(x.max()) for k, x in dev.items()}


def test_composed_oracle_agrees_with_float64_on_transformed_vertices():
    """instance_oracle against float64: the hit point M p lies in [pi_lo, pi_hi] (widened by the rounding of
    the float64 point to float32), a triangle's n is parallel to the normal of the explicitly transformed
    vertices, wo to -ray.d, dpdu / dpdv / the shading frame equal M applied to the shape's own (local) ones,
    the normals and normal derivatives the inverse transpose applied to them; uv, time and faceIndex pass
    through.  Bound: see F64_BOUND."""
    for n, seed in ((600, 77), (2048, 31)):  # this guard's records, and the generator at the GPU tests' seed
        rec, kind = cases(n, seed, return_kind=True)
        assert excluded_from_the_guard(rec, kind).mean() <= 0.15
    rec, kind = cases(600, 77, return_kind=True)
    worst = f64_deviation(0, rec[~excluded_from_the_guard(rec, kind)])
    print("triangles, worst relative deviation per field:", worst)
    assert max(worst.values()) <= F64_BOUND, worst
    worst = f64_deviation(1, patch_cases(300, 78))
    print("patches, worst relative deviation per field:", worst)
    assert max(worst.values()) <= F64_BOUND, worst


# ------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("force", ["empty_patch_table", "unused_instance_table"])
def test_gpu_full_kernel_at_top_level_matches_oracle_on_reference_vectors(force):
    """The reference vectors through k_triangle_interactions<true>: a mesh with a patch table that is all -1,
    or with an instance table that no hit refers to."""
    from nn_bvh_amd.interaction import ShadingMesh
    rec = tri_records()
    n = len(rec)
    exp = ob.triangle_interaction_batch(rec)
    kw = mesh_from_records(rec)
    if force == "empty_patch_table":
        kw["patch_vertices"] = np.full((n, 4), -1, np.int32)
    mesh = ShadingMesh(**kw)
    if force == "unused_instance_table":
        mesh.set_instances(instance_table(*instance_transforms()))
    hits = synthetic_hits(0, rec, 0)
    got = mesh.interactions(render_rays(0, rec), hits)
    assert (got["status"] == 1).all() and np.array_equal(got["prim"], hits["prim"])
    assert_records_equal(got, exp, np.arange(n), f"golden inputs, {force}")
    assert not got["dndu"].any() and not got["dndv"].any()
    mesh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,per_prim_flags", [(0, True), (0, False), (1, True)])
def test_gpu_every_flag_mix_inside_static_instances(kind, per_prim_flags):
    """Triangles (flags 0..15) and patches (flags 0 1 2 3 8 9 10 11) with uv, normals, tangents and faceIndices
    inside identity, rigid, scaled, mirrored and far-away instances; per_prim_flags = False drops the tri_flags
    array so that the mesh's defaultFlags (uv | n | s, no flip) decide."""
    from nn_bvh_amd.interaction import ShadingMesh
    rec = (tri_records() if kind == 0 else patch_records()).copy()
    if not per_prim_flags:
        rec[:, 19] = 7
    n = len(rec)
    m_all, mi_all = instance_transforms()
    kidx = np.arange(n) % len(XF_KINDS)
    flags = flags_of(kind, rec)
    if per_prim_flags:
        assert_all_pairs(flags, kidx, range(16) if kind == 0 else PATCH_FLAGS, len(XF_KINDS))
    kw = mesh_of(kind, rec)
    if not per_prim_flags:
        kw["tri_flags"] = None
    mesh = ShadingMesh(**kw)
    mesh.set_instances(instance_table(m_all, mi_all))
    rays = render_rays(kind, rec, m_all[kidx])
    hits = synthetic_hits(kind, rec, kidx + 1)
    got = mesh.interactions(rays, hits)
    assert (got["status"] == (1, 3)[kind]).all() and np.array_equal(got["prim"], hits["prim"])
    exp = instance_oracle(kind, rec, m_all[kidx], mi_all[kidx], rays["d"], rays["time"])
    assert_interaction_fields(got, exp, f"kind {kind} inside static instances", flags=flags,
                              xf_kind=np.array(XF_KINDS)[kidx])
    mesh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [0, 1])
def test_gpu_every_flag_mix_inside_animated_instances(kind):
    """The same records inside AnimatedPrimitives (cpu/primitive.cpp:143-153), ray times below, at the ends of,
    inside and above each entry's time range; ob.anim_interpolate runs with the device's sine."""
    from nn_bvh_amd.interaction import ShadingMesh
    rec = tri_records() if kind == 0 else patch_records()
    n = len(rec)
    anims, oa, inst = animated_table()
    k, t, moving = times_around_ranges(oa, n, 3)
    assert moving.mean() >= 0.25, moving.mean()
    flags = flags_of(kind, rec)
    for f in (range(16) if kind == 0 else PATCH_FLAGS):
        assert (moving & (flags == f)).any(), f
    m, mi = interpolated(oa, k, t)
    mesh = ShadingMesh(**mesh_of(kind, rec))
    mesh.set_instances(inst, animated=anims)
    rays = render_rays(kind, rec, m, time=t)
    hits = synthetic_hits(kind, rec, k + 1)
    got = mesh.interactions(rays, hits)
    assert (got["status"] == (1, 3)[kind]).all()
    exp = instance_oracle(kind, rec, m, mi, rays["d"], rays["time"])
    assert_interaction_fields(got, exp, f"kind {kind} inside animated instances", flags=flags,
                              xf_kind=np.where(moving, "moving", "at rest"))
    mesh.close()


@pytest.mark.gpu
def test_gpu_guarded_boundaries_leave_the_record_to_the_host():
    """interaction_status's bounds checks: instance == nInstances is the last valid entry; instance beyond the
    table, a negative instance and prim == nTris give status HOST, a miss status MISS, and these write only the
    record's last 16 bytes."""
    from nn_bvh_amd.interaction import ShadingMesh
    rec = tri_records()[:64]
    n = len(rec)
    m_all, mi_all = instance_transforms()
    n_inst = len(m_all)
    mesh = ShadingMesh(**mesh_from_records(rec))
    mesh.set_instances(instance_table(m_all, mi_all))
    inst = np.full(n, n_inst, np.int32)       # the last entry
    inst[1::8] = n_inst + 1
    inst[2::8] = -1
    inst[3::8] = -2 ** 31
    inst[4::8] = 2 ** 31 - 1
    hits = synthetic_hits(0, rec, inst)
    hits["prim"][5::8] = n                    # one past the last primitive, inside a valid instance
    hits["prim"][6::8] = -1                   # a miss
    hits["instance"][7::8] = 0
    hits["prim"][7::8] = n                    # ... and at top level
    kidx = np.full(n, n_inst - 1)
    rays = render_rays(0, rec, m_all[kidx])
    raw = run_device(mesh, rays, hits)
    got = as_records(raw)
    valid = np.nonzero(np.arange(n) % 8 == 0)[0]
    assert (got["status"][valid] == 1).all()
    exp = instance_oracle(0, rec[valid], m_all[kidx[valid]], mi_all[kidx[valid]], rays["d"][valid],
                          rays["time"][valid], face_index=7 + valid)
    assert_interaction_fields(got[valid], exp, "instance == nInstances", flags=rec[valid, 19],
                              xf_kind=np.array(XF_KINDS)[kidx[valid]])
    for r in range(1, 8):
        rows = np.arange(r, n, 8)
        assert (got["status"][rows] == (0 if r == 6 else 2)).all(), r
        assert np.array_equal(got["prim"][rows], hits["prim"][rows]), r
        assert (raw[rows, :176] == 0x5A).all(), f"case {r}: a record left to the host was written"
        assert (raw[rows, 184:] == 0).all(), r
    mesh.close()


@pytest.mark.gpu
def test_gpu_soa_rays_inside_instances_respect_the_device_side_size():
    from nn_bvh_amd.interaction import ShadingMesh
    rec = tri_records()[:3000]
    n = len(rec)
    size = n - 123
    m_all, mi_all = instance_transforms()
    kidx = np.arange(n) % len(XF_KINDS)
    mesh = ShadingMesh(**mesh_from_records(rec))
    mesh.set_instances(instance_table(m_all, mi_all))
    rays = render_rays(0, rec, m_all[kidx])
    raw = run_device(mesh, rays, synthetic_hits(0, rec, kidx + 1), soa_size=size)
    assert (raw[size:] == 0x5A).all(), "records beyond the queue size were written"
    got = as_records(raw[:size])
    assert (got["status"] == 1).all()
    exp = instance_oracle(0, rec[:size], m_all[kidx[:size]], mi_all[kidx[:size]], rays["d"][:size],
                          rays["time"][:size])
    assert_interaction_fields(got, exp, "SOA rays inside static instances", flags=rec[:size, 19],
                              xf_kind=np.array(XF_KINDS)[kidx[:size]])
    mesh.close()


# -------------------------------------------------------------- replacing the instance table
def static_table(n_entries):
    m_all, mi_all = instance_transforms()
    idx = (np.arange(n_entries) + 1) % len(XF_KINDS)
    return m_all[idx], mi_all[idx], np.array(XF_KINDS)[idx]


@pytest.mark.gpu
@pytest.mark.parametrize("length", ["same", "shorter", "larger"])
def test_gpu_static_table_replaces_an_animated_one(length):
    """set_instances(instances, animated=anims), then set_instances(static table): the new table's hits go
    through the new table's matrices, whatever its length — the animation tables of the earlier call are gone.
    (While set_instances kept them, the same-length case failed with "pi_lo differs on 1200 of 1440 records": the
    15 of 18 entries that are animated went through the old interpolated transforms; a larger table read past
    the old animation table.)"""
    from nn_bvh_amd.interaction import ShadingMesh
    rec = tri_records()[:1440]
    n = len(rec)
    anims, oa, inst = animated_table()
    n_static = {"same": len(oa), "shorter": 6, "larger": len(oa) + 6}[length]
    sm, smi, names = static_table(n_static)
    k = np.arange(n) % n_static
    old = np.minimum(k, len(oa) - 1)          # the entry a stale animation table would be read at
    f = np.random.default_rng(4).uniform(0.05, 0.95, n).astype(np.float32)
    t = (oa["start_time"][old] + f * (oa["end_time"][old] - oa["start_time"][old])).astype(np.float32)
    assert ((t > oa["start_time"][old]) & (t < oa["end_time"][old])).all()
    # the test shows something only where the stale, interpolated matrices differ from the new static ones
    im, _ = interpolated(oa, old, t)
    stale = (k < len(oa)) & (oa["actually_animated"][old] != 0) & (im != sm[k]).any((1, 2))
    assert stale.mean() > 0.5, stale.mean()
    mesh = ShadingMesh(**mesh_from_records(rec))
    mesh.set_instances(inst, animated=anims)
    mesh.set_instances(instance_table(sm, smi))
    rays = render_rays(0, rec, sm[k], time=t)
    got = mesh.interactions(rays, synthetic_hits(0, rec, k + 1))
    assert (got["status"] == 1).all()
    exp = instance_oracle(0, rec, sm[k], smi[k], rays["d"], rays["time"])
    assert_interaction_fields(got, exp, f"static table ({length} length) after an animated one", flags=rec[:, 19],
                              xf_kind=names[k])
    mesh.close()


@pytest.mark.gpu
def test_gpu_animated_table_replaces_a_static_one_and_an_empty_one_clears_it():
    from nn_bvh_amd import _lib
    from nn_bvh_amd.interaction import ShadingMesh
    rec = tri_records()[:1440]
    n = len(rec)
    anims, oa, inst = animated_table()
    k, t, moving = times_around_ranges(oa, n, 5)
    assert moving.mean() >= 0.25
    m, mi = interpolated(oa, k, t)
    mesh = ShadingMesh(**mesh_from_records(rec))
    sm, smi, _ = static_table(len(oa) + 6)
    mesh.set_instances(instance_table(sm, smi))
    mesh.set_instances(inst, animated=anims)
    rays = render_rays(0, rec, m, time=t)
    hits = synthetic_hits(0, rec, k + 1)
    got = mesh.interactions(rays, hits)
    assert (got["status"] == 1).all()
    exp = instance_oracle(0, rec, m, mi, rays["d"], rays["time"])
    assert_interaction_fields(got, exp, "animated table after a static one", flags=rec[:, 19],
                              xf_kind=np.where(moving, "moving", "at rest"))
    # no table at all: hits inside instances are the host's again, hits at top level still finished here
    mesh.set_instances(np.zeros(0, _lib.INSTANCE_DTYPE))
    hits["instance"][::2] = 0
    rays["d"][::2] = -rec[::2, 12:15]
    got = mesh.interactions(rays, hits)
    assert (got["status"][1::2] == 2).all() and (got["status"][::2] == 1).all()
    assert np.array_equal(got["prim"], hits["prim"])
    top = instance_oracle(0, rec[::2], None, None, rays["d"][::2], rays["time"][::2], face_index=7 + np.arange(0, n, 2))
    assert_interaction_fields(got[::2], top, "top level after the table was cleared", flags=rec[::2, 19])
    mesh.close()
