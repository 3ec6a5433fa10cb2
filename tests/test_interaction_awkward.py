"""The SurfaceInteraction arithmetic (csrc/interaction_math.h) on zeros, -0, denormals and extreme magnitudes.

Inputs: tests/awkward_cases.py's cases_tri_ / cases_blp_ / cases_xf_interaction, the generators of
tests/golden/interaction_cases.py made awkward (every flag mix and rare-branch kind stays).

CPU: what the families reach (on the oracle alone), how many records carry a NaN, the oracle against the compiled
reference — live where the harness exists, and on recorded vectors everywhere (tests/golden/awkward_*_interaction.npz).
The reference harness builds its mesh through an identity Transform, which normalises the sign of zeros
(awkward_cases.as_the_reference_mesh_stores); the oracle is held to it on records normalised the same way.

GPU: the post-pass (lean and FULL, at top level, inside static and inside animated instances) and the fused enqueue of
work items against the oracle on the RAW records, -0 as stored.  Every word is equal as uint32, or is a NaN on both
sides: x86 and gfx950 differ in the sign of the default NaN, and that is the only tolerance."""
import functools
import os
import subprocess
import tempfile
import types

import numpy as np
import pytest

import awkward_cases as ac
import oracle_binding as ob
from test_device_math import MIN_DENORMAL_SHARE, denormal
from test_interaction import HERE, REF, assert_interaction_fields, instance_oracle, mesh_from_records, words_differ
from test_interaction_instances import (animated_table, flags_of, instance_table, interpolated, mesh_of, render_rays,
                                        synthetic_hits, times_around_ranges)

SEEDS = {"tri": 101, "blp": 102, "xf": 103}          # the live comparison, the reach tests and the GPU tests alike
N_LIVE, N_GPU = 20000, 4096                          # the GPU tests take the first N_GPU records of the N_LIVE drawn
N_PARTS = -(-N_LIVE // N_GPU)
FAMILY = {"tri": ac.cases_tri_interaction, "blp": ac.cases_blp_interaction, "xf": ac.cases_xf_interaction}
ORACLE = {"tri": ob.triangle_interaction_batch, "blp": ob.patch_interaction_batch,
          "xf": ob.transform_interaction_batch}
FLOAT_COLUMNS = {"tri": np.r_[0:15, 20:35, 36:45], "blp": np.r_[0:17, 19:39], "xf": np.r_[0:71]}  # not time, flags
WO = {"tri": slice(12, 15), "blp": slice(14, 17)}
P_AND_N = {"tri": np.r_[0:9, 26:35], "blp": np.r_[0:12, 27:39]}
NOUT = {"tri": 44, "blp": 50, "xf": 40}
MAX_NAN_SHARE = 0.10                                 # of the records of any comparison: "NaN equals NaN" stays rare
live = pytest.mark.skipif(not (os.path.exists(REF) and os.path.isdir("/root/reference")),
                          reason="compiled reference harness only exists in the build container")


@functools.lru_cache(None)
def family(name):
    rec = FAMILY[name](SEEDS[name], N_LIVE)
    rec.setflags(write=False)
    return rec


def gpu_records(name, part=0):
    """The records of one GPU call: part 0 everywhere, parts 1 .. N_PARTS - 1 (the rest of the family, so that the
    device sees every record the live comparison pins) in the two plain top-level tests."""
    return family(name)[part * N_GPU:(part + 1) * N_GPU]


@functools.lru_cache(None)
def oracle_out(name):
    out = ORACLE[name](family(name))
    out.setflags(write=False)
    return out


def len2_wo(name, rec):
    w = rec[:, WO[name]]
    with np.errstate(over="ignore", under="ignore"):
        return (w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2]  # vecmath.h:948-950, in float32


def negative_zero(x):
    return (x == 0) & np.signbit(x)


def nan_share(fields):
    """share of the records with a NaN in any word of {name: array [n, ...]} or of an array [n, k]"""
    arrays = fields.values() if isinstance(fields, dict) else [fields]
    arrays = [np.asarray(a) for a in arrays]
    return np.any([np.isnan(a.reshape(len(a), -1)).any(1) for a in arrays if a.dtype == np.float32], 0).mean()


# ------------------------------------------------------------------------------------------ CPU: reach
@pytest.mark.parametrize("name", ["tri", "blp", "xf"])
def test_families_hold_denormals_and_stay_finite(name):
    for rec, what in ((family(name), "all"), (gpu_records(name), "the GPU tests' records")):
        share = denormal(rec[:, FLOAT_COLUMNS[name]]).any(1).mean()
        print(f"{name}, {what}: {len(rec)} records, {share:.1%} hold a denormal input")
        assert share >= MIN_DENORMAL_SHARE, (name, what, share)
        assert np.isfinite(rec).all()
    assert len(gpu_records(name)) == N_GPU and (N_PARTS - 1) * N_GPU < len(family(name)) <= N_LIVE
    if name == "tri":
        assert not ac.zero_area(family(name)).any()
    if name == "xf":
        rec = family(name)
        assert (rec[:, 32:35] <= rec[:, 35:38]).all()
        exact = (rec[:, 32:35] == rec[:, 35:38]).all(1)
        one_ulp = (rec[:, 35:38] == np.nextafter(rec[:, 32:35], np.float32(np.inf))).all(1)
        denormal_wide = denormal(rec[:, 35:38] - rec[:, 32:35]).all(1)
        print(f"xf: pi exact on {exact.sum()}, one ulp wide on {one_ulp.sum()}, a denormal wide on {denormal_wide.sum()}")
        assert min(exact.sum(), one_ulp.sum(), denormal_wide.sum()) >= 1000
        m = rec[:, 0:16].reshape(-1, 4, 4).astype(np.float64)
        assert (np.abs(np.linalg.det(m)) > 0).all(), "a singular matrix"
        assert (np.linalg.det(m[:, :3, :3]) < 0).sum() >= 1000, "mirrored transforms"
        assert denormal(rec[:, np.r_[0:12, 16:28]]).any(1).sum() >= 500, "denormals among the matrix entries"


@pytest.mark.parametrize("name", ["tri", "blp"])
def test_families_reach_every_branch_and_every_class_of_wo_length(name):
    """Every rare-branch counter of the oracle, LengthSquared(wo) as a denormal, as zero and as infinity, -0 among
    positions and normals: at least 100 records of each class and 500 with a -0 in the whole family, and the share of
    that (4096 / 20000, rounded down: 20 and 102) among the first records, which every GPU test takes."""
    branches = ob.interaction_branches if name == "tri" else ob.patch_branches
    for rec, want_class, want_neg0 in ((family(name), 100, 500), (gpu_records(name), 20, 102)):
        branches(reset=True)
        ORACLE[name](rec)
        counts = branches(reset=True)
        l2 = len2_wo(name, rec)
        classes = {"denormal": int(denormal(l2).sum()), "zero": int((l2 == 0).sum()), "infinite": int(np.isinf(l2).sum())}
        neg0 = int(negative_zero(rec[:, P_AND_N[name]]).any(1).sum())
        print(f"{name}, {len(rec)} records: branches {counts}, LengthSquared(wo) {classes}, "
              f"{neg0} records with a -0 among positions or normals")
        assert min(counts) > 0, counts
        assert min(classes.values()) >= want_class, classes
        assert neg0 >= want_neg0, neg0


@pytest.mark.parametrize("name", ["tri", "blp", "xf"])
def test_nan_records_stay_rare(name):
    """A condition on the families, not a filter: records with NaNs stay in every comparison; the cap only limits how
    many words are compared as "NaN equals NaN"."""
    calls = [(oracle_out(name)[part * N_GPU:(part + 1) * N_GPU], f"GPU call {part}") for part in range(N_PARTS)]
    for out, what in [(oracle_out(name), "all")] + calls:
        share = nan_share(out)
        print(f"{name}, {what}: {share:.2%} of the records hold a NaN in an oracle output word")
        assert share <= MAX_NAN_SHARE, (name, what, share)


# ------------------------------------------------------- CPU: the oracle against the compiled reference
def run_ref(rec, mode):
    with tempfile.TemporaryDirectory() as td:
        fi, fo = os.path.join(td, "in.bin"), os.path.join(td, "out.bin")
        with open(fi, "wb") as f:
            f.write(np.int32(len(rec)).tobytes())
            f.write(np.ascontiguousarray(rec, np.float32).tobytes())
        subprocess.run([REF, mode, fi, fo], check=True)
        return np.fromfile(fo, dtype=np.uint32).reshape(len(rec), NOUT[mode])


def oracle_as_the_reference_sees(name, rec):
    if name != "xf":
        rec = ac.as_the_reference_mesh_stores(rec, ("tri", "blp").index(name))
    return ORACLE[name](rec).view(np.uint32)


def assert_bits_equal(got, exp, what):
    bad = np.nonzero(got != exp)
    assert len(bad[0]) == 0, (f"{what}: {len(bad[0])} words on {len(np.unique(bad[0]))} records differ, "
                              f"first rows {bad[0][:5]} columns {bad[1][:5]}")


@pytest.mark.parametrize("name", ["tri", "blp"])
def test_the_reference_mesh_changes_only_signs_of_zeros(name):
    rec = family(name)
    stored = ac.as_the_reference_mesh_stores(rec, ("tri", "blp").index(name))
    changed = rec.view(np.uint32) != stored.view(np.uint32)
    print(f"{name}: {changed.sum()} words on {changed.any(1).sum()} of {len(rec)} records change")
    assert changed.any(), "the family holds no -0 the identity transform would touch"
    assert (rec[changed] == 0).all() and (stored[changed] == 0).all()
    assert negative_zero(rec[changed]).all() and not np.signbit(stored[changed]).any()
    # positions: every -0 becomes +0; normals and tangents: a -0 stays next to two components with the sign bit set
    n_pos = 9 if name == "tri" else 12
    assert not negative_zero(stored[:, :n_pos]).any()
    kept = negative_zero(stored[:, P_AND_N[name][n_pos:]]).reshape(-1, 3)
    assert kept.any() and np.signbit(stored[:, P_AND_N[name][n_pos:]].reshape(-1, 3)[kept.any(1)]).all()


@live
@pytest.mark.parametrize("name", ["tri", "blp"])
def test_reference_gives_the_same_bytes_for_raw_and_stored_records(name):
    rec = family(name)
    stored = ac.as_the_reference_mesh_stores(rec, ("tri", "blp").index(name))
    assert run_ref(rec, name).tobytes() == run_ref(stored, name).tobytes()


@live
@pytest.mark.parametrize("name", ["tri", "blp", "xf"])
def test_oracle_equals_reference_live_on_awkward_records(name):
    """20 000 records at the seed of the GPU tests (which take the first 4 096): every output word, NaNs included."""
    rec = family(name)
    ref = run_ref(rec, name)
    raw = (ORACLE[name](rec).view(np.uint32) != ref).any(1).sum()
    print(f"{name}: the oracle on the RAW records differs from the reference on {raw} of {len(rec)} records "
          "(signs of zeros the reference's mesh normalised)")
    assert_bits_equal(oracle_as_the_reference_sees(name, rec), ref, f"{name}, seed {SEEDS[name]}")


@pytest.mark.parametrize("name", ["tri", "blp", "xf"])
def test_oracle_matches_recorded_reference_bits_on_awkward_records(name):
    """tests/golden/awkward_*_interaction.npz (make_awkward_interaction_golden.py): RAW inputs, the reference's bits."""
    g = np.load(os.path.join(HERE, "golden", f"awkward_{name}_interaction.npz"))
    rec = g["inputs"]
    assert len(rec) >= 2000 and denormal(rec[:, FLOAT_COLUMNS[name]]).any(1).mean() >= MIN_DENORMAL_SHARE
    assert_bits_equal(oracle_as_the_reference_sees(name, rec), g["outputs"], f"{name} fixture")


# ------------------------------------------------------------------------------------------------- GPU
def quiet(f, *a, **kw):
    """numpy restating the device's float32 products on extreme inputs: overflow is the point, not a warning"""
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return f(*a, **kw)


def compare(got, exp, what, kind, rec, xf_kind=None):
    share = nan_share(exp)
    print(f"{what}: {share:.2%} of {len(rec)} records hold a NaN in an oracle word")
    assert share <= MAX_NAN_SHARE, (what, share)
    assert (got["status"] == (1, 3)[kind]).all() and np.array_equal(got["prim"], np.arange(len(rec))), what
    assert_interaction_fields(got, exp, what, flags=flags_of(kind, rec), xf_kind=xf_kind, nan_equal=True)


@functools.lru_cache(None)
def awkward_instances():
    """256 entries of ac.random_affine (rigid, scaled 1e-2 .. 1e2, mirrored, translated up to 1e3 and untranslated);
    about 15 % of them with a denormal among the elements of the matrix or of its inverse: m, mi float32 [256, 3, 4]."""
    M, Mi = ac.random_affine(np.random.default_rng(7), 256)
    flat = np.concatenate([M[:, :3].reshape(-1, 12), Mi[:, :3].reshape(-1, 12)], 1)
    flat = ac.with_denormals(flat, np.r_[0:24], [7, 1], share=0.15)
    m, mi = flat[:, :12].reshape(-1, 3, 4), flat[:, 12:].reshape(-1, 3, 4)
    holds = denormal(flat).any(1)
    mirrored = np.linalg.det(m[:, :, :3].astype(np.float64)) < 0
    assert 20 <= holds.sum() <= 64 and mirrored.sum() >= 20 and (~mirrored).sum() >= 100, (holds.sum(), mirrored.sum())
    assert (m[:, :, 3] == 0).all(1).sum() >= 20 and denormal(flat[:, :12]).any() and denormal(flat[:, 12:]).any()
    names = np.where(holds, "denormal ", "") + np.where(mirrored, "mirrored", "not mirrored")
    return m, mi, names


@pytest.mark.gpu
@pytest.mark.parametrize("force,part", [(None, part) for part in range(N_PARTS)] +
                         [("empty_patch_table", 0), ("unused_instance_table", 0)])
def test_gpu_awkward_triangles_at_top_level(force, part):
    """k_triangle_interactions<false> on the whole family, 4 096 records a call, and <true> forced by a patch table
    that is all -1 or by an instance table no hit refers to."""
    from nn_bvh_amd.interaction import ShadingMesh
    rec = gpu_records("tri", part)
    rays, hits = render_rays(0, rec), synthetic_hits(0, rec, 0)
    exp = instance_oracle(0, rec, None, None, rays["d"], rays["time"])
    kw = mesh_from_records(rec)
    if force == "empty_patch_table":
        kw["patch_vertices"] = np.full((len(rec), 4), -1, np.int32)
    mesh = ShadingMesh(**kw)
    if force == "unused_instance_table":
        m, mi, _ = awkward_instances()
        mesh.set_instances(instance_table(m, mi))
    got = mesh.interactions(rays, hits)
    compare(got, exp, f"awkward triangles at top level, {force}, part {part}", 0, rec)
    assert not got["dndu"].any() and not got["dndv"].any()
    mesh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("part", range(N_PARTS))
def test_gpu_awkward_patches_at_top_level(part):
    from nn_bvh_amd.interaction import ShadingMesh
    rec = gpu_records("blp", part)
    rays, hits = render_rays(1, rec), synthetic_hits(1, rec, 0)
    exp = instance_oracle(1, rec, None, None, rays["d"], rays["time"])
    mesh = ShadingMesh(**mesh_of(1, rec))
    compare(mesh.interactions(rays, hits), exp, f"awkward patches at top level, part {part}", 1, rec)
    mesh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [0, 1])
def test_gpu_awkward_records_inside_static_instances(kind):
    from nn_bvh_amd.interaction import ShadingMesh
    rec = gpu_records(("tri", "blp")[kind])
    m, mi, names = awkward_instances()
    k = np.arange(len(rec)) % len(m)
    rays, hits = quiet(render_rays, kind, rec, m[k]), synthetic_hits(kind, rec, k + 1)
    exp = quiet(instance_oracle, kind, rec, m[k], mi[k], rays["d"], rays["time"])
    mesh = ShadingMesh(**mesh_of(kind, rec))
    mesh.set_instances(instance_table(m, mi))
    compare(mesh.interactions(rays, hits), exp, f"awkward kind {kind} inside static instances", kind, rec, names[k])
    mesh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [0, 1])
def test_gpu_awkward_records_inside_animated_instances(kind):
    """Inside the entries of animated_table(), ray times below, at the ends of, inside and above each entry's time
    range; the oracle's Interpolate runs with the device's sine (the path's documented exception)."""
    from nn_bvh_amd.interaction import ShadingMesh
    rec = gpu_records(("tri", "blp")[kind])
    anims, oa, inst = animated_table()
    k, t, moving = times_around_ranges(oa, len(rec), 3)
    assert moving.mean() >= 0.25, moving.mean()
    m, mi = interpolated(oa, k, t)
    rays, hits = quiet(render_rays, kind, rec, m, time=t), synthetic_hits(kind, rec, k + 1)
    exp = quiet(instance_oracle, kind, rec, m, mi, rays["d"], rays["time"])
    mesh = ShadingMesh(**mesh_of(kind, rec))
    mesh.set_instances(inst, animated=anims)
    compare(mesh.interactions(rays, hits), exp, f"awkward kind {kind} inside animated instances", kind, rec,
            np.where(moving, "moving", "at rest"))
    mesh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("inside", [False, True])
def test_gpu_fused_enqueue_of_awkward_triangles(inside):
    """nnbvh_wavefront_enqueue_closest_items_device on synthetic hits on the awkward triangles, a prim_class table
    that feeds every item queue, all slices: each slice equals the post-pass record of the same hit (itself held to
    the oracle here), p is the interval's midpoint, next_ray.ray_o the oracle's OffsetRayOrigin."""
    import torch
    import test_wavefront_items as twi
    from nn_bvh_amd import _lib
    from nn_bvh_amd.interaction import ShadingMesh
    from nn_bvh_amd.wavefront import WorkQueue, enqueue_closest_items
    rec = gpu_records("tri")
    n = len(rec)
    mesh = ShadingMesh(**mesh_from_records(rec))
    if inside:
        m, mi, names = awkward_instances()
        k = np.arange(n) % len(m)
        mesh.set_instances(instance_table(m, mi))
        rays, hits = quiet(render_rays, 0, rec, m[k]), synthetic_hits(0, rec, k + 1)
        exp = quiet(instance_oracle, 0, rec, m[k], mi[k], rays["d"], rays["time"])
    else:
        rays, hits = render_rays(0, rec), synthetic_hits(0, rec, 0)
        exp = instance_oracle(0, rec, None, None, rays["d"], rays["time"])
    rng = np.random.default_rng(5)
    prim_class = rng.choice(np.array([0, 1, 2, 4, 5, 6], np.uint8), n)
    has_medium = (rng.random(n) < 0.15).astype(np.uint8)
    dev = torch.device("cuda", 0)
    rq = twi.ray_queue(rays, dev, has_medium)
    hits_t = torch.from_numpy(np.ascontiguousarray(hits).view(np.uint8).reshape(n, 32)).to(dev)
    queues = {q: WorkQueue(n, dev) for q in twi.QUEUES}
    items = twi.full_items(n, dev)
    enqueue_closest_items(mesh, n, rq, hits_t, prim_class=torch.from_numpy(prim_class).to(dev), items=items, **queues)
    torch.cuda.synchronize()
    intr = twi.reference_records(mesh, hits_t, rq, n, dev)
    compare(intr, exp, f"post-pass records of the enqueue's hits, inside = {inside}", 0, rec)
    expect = dict(zip(twi.QUEUES, ob.wavefront_enqueue_closest(hits, has_medium, prim_class)))
    d = np.ascontiguousarray(rays["d"])
    for q in _lib.ITEM_QUEUES:
        assert queues[q].Size() > 100, q
        but_ray_o = types.SimpleNamespace(fields={f: t for f, t in items[q].fields.items() if f != "ray_o"})
        with np.errstate(over="ignore", invalid="ignore"):  # p = (lo + hi) / 2 of huge or infinite ends
            rows = twi.check_slices(q, queues[q], but_ray_o, intr, hits, d, expect[q], nan_equal=True)
        assert len(rows) == queues[q].Size()
    # next_ray.ray_o: equal on the rows whose pi, n and d are finite, NaN for NaN on the few others
    q = queues["next_ray"]
    idx = q.items[:q.Size()].cpu().numpy()
    order = np.argsort(idx)
    rows = idx[order]
    got = items["next_ray"].fields["ray_o"].cpu().numpy()[:, :len(idx)][:, order]
    want = twi.expected_field("ray_o", "next_ray", rows, intr, hits, d)
    r = intr[rows]
    finite = np.isfinite(np.concatenate([r["pi_lo"], r["pi_hi"], r["n"], d[rows]], 1)).all(1)
    print(f"next_ray: {1 - finite.mean():.2%} of {len(rows)} items have a non-finite pi, n or d")
    assert 1 - finite.mean() <= MAX_NAN_SHARE
    assert not words_differ(got[:, finite], want[:, finite]).any(), "ray_o on finite rows"
    assert not words_differ(got[:, ~finite], want[:, ~finite], nan_equal=True).any(), "ray_o on the other rows"
    mesh.close()
