"""The device's own arithmetic (nn_bvh_amd/csrc/trace_math.h, spawn_math.h, anim_math.h) evaluated directly, one
record per lane, by tests/hip/device_math_check.hip, a stand-alone program that includes the product headers:

  a. on the golden vectors of tests/golden/ (raw output bits of the REFERENCE's compiled functions), bit for bit;
  b. on the awkward-input families of tests/awkward_cases.py (about 13 % of the leaf records hold a denormal), against
     the oracle, which tests/test_oracle_vs_reference_live.py and tests/test_aux_oracle.py hold to the compiled
     reference on the same families;
  c. all pairs through the real kernels: scenes whose root is ONE leaf holding the golden triangles (and patches),
     traced with the golden rays: every ray against every primitive at every scale of the fixtures.

The CPU tests compile the program and check, on the oracle alone, that the inputs reach what they are meant to reach.
Every GPU run of the program is a fresh child process with a time limit of its own; a non-zero exit status fails the
test with the child's stderr before any output is read."""
import functools
import os
import subprocess
import tempfile
import time

import numpy as np
import pytest

import awkward_cases as ac
import oracle_binding as ob
from test_animated import anims_from_reference_output

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SRC = os.path.join(ROOT, "tests", "hip", "device_math_check.hip")
EXE = os.path.join(ROOT, "tests", "hip", "device_math_check")

# One run = process start, HIP initialisation, one kernel of at most 20 000 lanes, two small copies.  Measured on an
# MI355X: 0.16 .. 0.37 s per run in every mode, at 3 000 and at 20 000 records alike (the kernel itself is
# microseconds), so one limit serves all modes: a hundred times the slowest run.  A run that reaches it has hung.
HARNESS_SECONDS_MEASURED = 0.37
HARNESS_TIMEOUT = 100 * HARNESS_SECONDS_MEASURED

NOUT = {"tri": 4, "tri_masks": 4, "blp": 3, "slab": 2, "slab2": 2, "xfray": 7, "hash": 2, "offset": 9, "wrs": 2,
        "anim": 24}


def _build(nnbvh_lib, force=False):
    """Compile the harness with the product's flags when it is missing or older than its source, a product header or
    the product library it links (fill_anim_entry): the library the package loads, _lib.LIB_PATH."""
    from nn_bvh_amd import _lib, build
    deps = [SRC, _lib.LIB_PATH] + [os.path.join(build.CSRC, h) for h in build.HEADERS]
    if not force and os.path.exists(EXE) and os.path.getmtime(EXE) >= max(os.path.getmtime(d) for d in deps):
        return EXE
    libdir, libname = os.path.split(_lib.LIB_PATH)
    subprocess.run([build._hipcc()] + build.CFLAGS + ["-I", build.CSRC, SRC, "-o", EXE, "-L", libdir,
                    f"-l:{libname}", "-Wl,-rpath,$ORIGIN/../../nn_bvh_amd"], check=True)
    return EXE


def run_device(nnbvh_lib, mode, recs):
    """One fresh child process: raw uint32 [n, 1 + NOUT[mode]]."""
    exe = _build(nnbvh_lib)
    recs = np.ascontiguousarray(recs, np.float32)
    with tempfile.TemporaryDirectory() as td:
        fi, fo = os.path.join(td, "i.bin"), os.path.join(td, "o.bin")
        with open(fi, "wb") as f:
            f.write(np.int32(len(recs)).tobytes())
            f.write(recs.tobytes())
        t0 = time.perf_counter()
        out = subprocess.run([exe, mode, fi, fo], capture_output=True, text=True, timeout=HARNESS_TIMEOUT)
        print(f"device_math_check {mode}: {len(recs)} records in {time.perf_counter() - t0:.2f} s")
        assert out.returncode == 0, f"device_math_check {mode}: exit status {out.returncode}\n{out.stderr}"
        return np.fromfile(fo, np.uint32).reshape(len(recs), 1 + NOUT[mode])


def first_rows(a, k=5):
    return np.nonzero(a)[0][:k]


def denormal(x):
    ax = np.abs(np.asarray(x, np.float32))
    return (ax > 0) & (ax < np.finfo(np.float32).tiny)


# ---- the harness itself ---------------------------------------------------------------------------------------------
def test_harness_cross_compiles_with_the_product_flags(nnbvh_lib):
    from nn_bvh_amd import build
    assert "-ffp-contract=off" in build.CFLAGS and "-O3" in build.CFLAGS
    _build(nnbvh_lib, force=True)
    assert os.path.exists(EXE)
    bad = subprocess.run([EXE, "no_such_mode", "a", "b"], capture_output=True, text=True, timeout=HARNESS_TIMEOUT)  # no GPU call
    assert bad.returncode == 2 and "usage" in bad.stderr
    with tempfile.TemporaryDirectory() as td:  # an empty batch and a truncated one: decided before any GPU call too
        fi, fo = os.path.join(td, "i.bin"), os.path.join(td, "o.bin")
        with open(fi, "wb") as f:
            f.write(np.int32(0).tobytes())
        empty = subprocess.run([EXE, "tri", fi, fo], capture_output=True, timeout=HARNESS_TIMEOUT)
        assert empty.returncode == 0 and os.path.getsize(fo) == 0
        with open(fi, "wb") as f:
            f.write(np.int32(2).tobytes() + np.zeros(16, np.float32).tobytes())
        short = subprocess.run([EXE, "tri", fi, fo], capture_output=True, text=True, timeout=HARNESS_TIMEOUT)
        assert short.returncode == 4 and "16 float32" in short.stderr


# ---- a. golden vectors: the reference's bits -------------------------------------------------------------------------
@functools.lru_cache(None)
def golden(mode):
    """(records, first word or None, out_bits) of the fixture `mode` is checked on"""
    if mode == "anim":
        g = np.load(os.path.join(GOLD, "anim_interpolate.npz"))
        return g["inputs"], None, g["outputs"]
    leaf = {"tri": "leaf_tri", "tri_masks": "leaf_tri", "blp": "leaf_blp", "slab": "leaf_slab", "xfray": "leaf_xfray"}
    if mode in leaf:
        g = np.load(os.path.join(GOLD, leaf[mode] + ".npz"))
        return g["inputs"], g["hit"].astype(np.uint32), g["out_bits"]
    g = np.load(os.path.join(GOLD, f"aux_{mode}.npz"))
    return g["inputs"], g["first"], g["out_bits"]


def anim_records():
    """The anim fixture as harness records: the C ABI's nnbvh_animated_transform (what the reference object holds after
    construction), then the time; and the same transforms as the oracle's records."""
    from nn_bvh_amd import _lib
    rec, _, out = golden("anim")
    a = anims_from_reference_output(rec, out)
    p = np.zeros(len(rec), _lib.ANIMATED_DTYPE)
    for src, dst in (("start_m", "start_from"), ("start_minv", "start_inv"), ("end_m", "end_from"), ("end_minv", "end_inv"),
                     ("T", "T"), ("R", "R"), ("S", "S"), ("start_time", "start_time"), ("end_time", "end_time"),
                     ("actually_animated", "actually_animated")):
        p[dst] = a[src]
    words = p.view(np.float32).reshape(len(rec), -1)
    assert words.shape[1] == 114
    return np.concatenate([words, rec[:, 34:35]], 1), a


ROWS = np.r_[0:12, 16:28]  # rows 0..2 of m and of mInv among the 32 words {m, mInv}


def anim_oracle_with_device_sine():
    _, a = anim_records()
    try:
        ob.set_sin_mode(1)
        return ob.anim_interpolate(a, golden("anim")[0][:, 34]).view(np.uint32)
    finally:
        ob.set_sin_mode(0)


def test_golden_fixtures_reach_the_hard_branches_and_hold_no_nan_or_denormal():
    """test_oracle.py's reachability conditions on the fixtures used here, and what makes `bit for bit, no exception`
    the right rule for them: no NaN and no denormal anywhere (the awkward families of part b bring those)."""
    r, hit, bits = golden("tri")
    bary = bits[:256, :3].view(np.float32)
    assert ((bary == 0).any(1) & (hit[:256] == 1)).sum() > 20       # hits with a barycentric of exactly 0
    p = r[:, 7:].reshape(-1, 3, 3)
    assert ((p[:, 1] == p[:, 2]).all(1)).sum() > 100                # degenerate triangles
    assert ((r[:, 3:6] == 0).sum(1) == 2).sum() > 100               # axis-aligned directions
    assert ((golden("slab")[0][:, 3:6] == 0).any(1)).sum() > 500    # +-inf inverse directions
    for mode in ("tri", "blp", "slab", "xfray", "slab2", "hash", "offset", "wrs"):
        x, first, out = golden(mode)
        assert not np.isnan(x).any() and not denormal(x).any(), mode
        if mode != "hash":  # (a hash's high word is an integer)
            f = out.view(np.float32)
            assert not np.isnan(f).any() and not denormal(f).any(), mode
    x, _, out = golden("anim")
    assert not np.isnan(x).any() and not np.isnan(np.ascontiguousarray(out).view(np.float32)).any()
    for mode in ("tri", "blp", "slab", "slab2"):
        assert 0.2 < golden(mode)[1].mean() < 0.9, mode              # both verdicts


def test_anim_exception_on_the_oracle():
    """The oracle with the device's sine differs from the reference on some records of the fixture (the documented Slerp
    exception), never in the rows the device does not produce (row 3 of m and of mInv), and by low-order
    bits only."""
    exp = np.ascontiguousarray(golden("anim")[2][:, 80:112]).view(np.uint32)
    got = anim_oracle_with_device_sine()
    differs = (got != exp).any(1)
    assert differs.any() and differs.mean() < 0.05
    other = np.setdiff1d(np.arange(32), ROWS)
    assert np.array_equal(got[:, other], exp[:, other])
    e = exp.view(np.float32).astype(np.float64)
    rel = np.abs(got.view(np.float32) - e) / np.maximum(np.abs(e), 1e-30)
    print(f"anim: the oracle with the device's sine differs from the reference on {int(differs.sum())} of {len(exp)} "
          f"records, max relative difference {rel.max():.1e}")
    assert rel.max() < 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["tri", "tri_masks", "blp", "slab2"])
def test_golden_verdicts_and_hit_outputs_are_the_references_bits(nnbvh_lib, mode):
    x, first, bits = golden(mode)
    raw = run_device(nnbvh_lib, mode, x)
    bad = raw[:, 0] != first
    assert not bad.any(), f"{mode}: verdict differs on {bad.sum()} records, first {first_rows(bad)}"
    h = first.astype(bool)
    bad = (raw[:, 1:] != bits).any(1) & h
    assert not bad.any(), f"{mode}: output bits differ on {bad.sum()} hits, first {first_rows(bad)}: " \
                          f"{raw[first_rows(bad, 1), 1:]} vs {bits[first_rows(bad, 1)]}"


@pytest.mark.gpu
def test_golden_triangle_test_with_and_without_masks_agree_everywhere(nnbvh_lib):
    x = golden("tri")[0]
    a, b = run_device(nnbvh_lib, "tri", x), run_device(nnbvh_lib, "tri_masks", x)
    bad = (a != b).any(1)
    assert not bad.any(), f"triangle_test with masks differs on {bad.sum()} records, first {first_rows(bad)}"


@pytest.mark.gpu
def test_golden_three_slab_forms_give_the_references_verdict(nnbvh_lib):
    x, hit, _ = golden("slab")
    raw = run_device(nnbvh_lib, "slab", x)
    for k, form in enumerate(("slab_partial", "slab_entry_key", "slab_entry_key with masks")):
        bad = raw[:, k] != hit
        assert not bad.any(), f"{form}: verdict differs on {bad.sum()} records, first {first_rows(bad)}"


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["xfray", "hash", "offset", "wrs"])
def test_golden_every_output_word_is_the_references(nnbvh_lib, mode):
    x, first, bits = golden(mode)
    raw = run_device(nnbvh_lib, mode, x)
    if mode == "xfray":
        first = np.ones(len(x), np.uint32)
    elif mode == "offset":
        first = np.ones(len(x), np.uint32)
    bad = (raw[:, 0] != first) | (raw[:, 1:] != bits).any(1)
    assert not bad.any(), f"{mode}: {bad.sum()} records differ, first {first_rows(bad)}: " \
                          f"{raw[first_rows(bad, 1)]} vs {first[first_rows(bad, 1)]} {bits[first_rows(bad, 1)]}"


@pytest.mark.gpu
def test_golden_anim_rows_equal_the_oracle_with_the_device_sine_and_the_exception_is_exact(nnbvh_lib):
    """anim_rows<true> on table entries made by the product's fill_anim_entry: bit-equal to the oracle evaluated with the
    device's sine on every record; against the reference's own bits the records that differ are exactly the records on
    which that oracle differs — the Slerp exception, no more and no less."""
    recs, _ = anim_records()
    raw = run_device(nnbvh_lib, "anim", recs)
    assert (raw[:, 0] == 1).all()
    exp = anim_oracle_with_device_sine()[:, ROWS]
    bad = (raw[:, 1:] != exp).any(1)
    assert not bad.any(), f"anim: differs from the oracle with the device's sine on {bad.sum()} records, first {first_rows(bad)}"
    ref = np.ascontiguousarray(golden("anim")[2][:, 80:112]).view(np.uint32)[:, ROWS]
    dev_differs, orc_differs = (raw[:, 1:] != ref).any(1), (exp != ref).any(1)
    assert np.array_equal(dev_differs, orc_differs)
    print(f"anim: {int(dev_differs.sum())} of {len(recs)} records differ from the reference's bits")


# ---- b. awkward inputs: the oracle's bits ----------------------------------------------------------------------------
# mode -> (generator, seed).  The seeds are this file's own (the live comparisons with the reference use 1, 2, 11 .. 42).
# The leaf families hold a denormal in 11 - 17 % of their records as they are; the others are drawn with further
# denormal operands (awkward_cases.with_denormals), so that every mode meets the same 10 %.
AWKWARD = {"tri": (ac.cases_tri, 101), "blp": (ac.cases_blp, 102), "slab": (ac.cases_slab, 103),
           "xfray": (ac.cases_xfray_denormal, 104), "hash": (ac.cases_hash_denormal, 105),
           "offset": (ac.cases_offset_denormal, 106), "wrs": (ac.cases_wrs_denormal, 107),
           "slab2": (ac.cases_slab2_denormal, 108)}
N_AWKWARD = 20000
HAS_VERDICT = ("tri", "blp", "slab", "slab2", "wrs")
MIN_DENORMAL_SHARE = 0.10  # of the records of every mode hold a denormal input


@functools.lru_cache(None)
def awkward(mode):
    """(records, the oracle's first word uint32 [n], the oracle's outputs uint32 [n, k], float columns of them)"""
    gen, seed = AWKWARD[mode]
    x = gen(seed, N_AWKWARD)
    if mode in ("tri", "blp", "slab"):
        hit, out = ob.leaf_batch(mode, x)
        return x, hit.astype(np.uint32), out.view(np.uint32).reshape(len(x), -1), slice(None)
    if mode == "xfray":
        out = ob.apply_inverse_ray(x[:, 23:35], x[:, 0:3], x[:, 3:6], x[:, 6])
        return x, np.ones(len(x), np.uint32), out.view(np.uint32), slice(None)
    if mode == "hash":
        lo, hi, hf = ob.hash_batch(x)
        return x, lo, np.stack([hf.view(np.uint32), hi], 1), slice(0, 1)
    if mode == "offset":
        return x, np.ones(len(x), np.uint32), ob.offset_batch(x).view(np.uint32), slice(None)
    if mode == "wrs":
        sel, out = ob.wrs_batch(x)
        return x, sel.view(np.uint32), out.view(np.uint32), slice(None)
    hit, tt = ob.bounds_t0t1(x[:, 7:13], x[:, 0:3], x[:, 3:6], x[:, 6])
    return x, hit.astype(np.uint32), tt.view(np.uint32), slice(None)


def awkward_hits(mode):
    x, first, out, _ = awkward(mode)
    if mode == "wrs":
        return first.view(np.int32) >= 0
    return first.astype(bool) if mode in HAS_VERDICT else np.ones(len(x), bool)


@pytest.mark.parametrize("mode", list(AWKWARD))
def test_awkward_families_reach_hits_denormals_and_few_nans_on_the_oracle(mode):
    x, first, out, fcols = awkward(mode)
    assert len(x) >= 0.99 * N_AWKWARD
    hits = awkward_hits(mode)
    den = denormal(x).any(1)
    f = out[:, fcols].view(np.float32)
    nan_hits = hits & np.isnan(f).any(1) if f.shape[1] else np.zeros(len(x), bool)
    print(f"{mode}: {len(x)} records, {int(hits.sum())} hits, {int(den.sum())} with a denormal input, "
          f"{int((hits & den).sum())} hits among those, {int(nan_hits.sum())} hits with a NaN output")
    if mode in HAS_VERDICT:  # (xfray, hash and offset have no verdict: every record counts as a hit, nothing to assert)
        assert hits.sum() >= 1000
        if mode != "wrs":
            assert (~hits).sum() >= 1000  # and misses
            assert (hits & den).sum() >= 100 and (~hits & den).sum() >= 100
    assert den.mean() >= MIN_DENORMAL_SHARE
    if mode in ("tri", "blp"):
        assert (hits & den).sum() >= 500
    assert nan_hits.sum() <= 0.001 * hits.sum()


REF = os.path.join(ROOT, "oracle", "_ref", "ref_leaf")


@pytest.mark.skipif(not os.path.exists(REF), reason="oracle/_ref/ref_leaf not built")
@pytest.mark.parametrize("mode", ["xfray", "hash", "offset", "wrs", "slab2"])
def test_oracle_equals_the_compiled_reference_on_the_families_with_more_denormals(mode):
    """The plain families are held to the reference by the live tests; the device is compared with the oracle on their
    denser variants, so the oracle is held to the reference on exactly those records too (CPU only)."""
    from test_aux_oracle import run_ref_raw
    x, first, out, fcols = awkward(mode)
    rfirst, rbits = run_ref_raw(mode, x, out.shape[1])
    hits = awkward_hits(mode)
    assert np.array_equal(first, rfirst.astype(np.uint32) if mode == "slab2" else rfirst)
    assert np.array_equal(out[hits], rbits[hits])


def assert_device_equals_oracle(mode, raw, first, out, fcols, hits):
    bad = raw[:, 0] != first
    assert not bad.any(), f"{mode}: first word (verdict) differs on {bad.sum()} records, first {first_rows(bad)}"
    got = raw[:, 1:1 + out.shape[1]]
    same = got == out
    both_nan = np.zeros_like(same)
    both_nan[:, fcols] = np.isnan(got[:, fcols].view(np.float32)) & np.isnan(out[:, fcols].view(np.float32))
    bad = ~(same | both_nan).all(1) & hits
    assert not bad.any(), f"{mode}: outputs differ on {bad.sum()} records, first {first_rows(bad)}: " \
                          f"{got[first_rows(bad, 1)]} vs {out[first_rows(bad, 1)]}"


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["tri", "tri_masks", "blp", "xfray", "hash", "offset", "wrs", "slab2"])
def test_awkward_inputs_device_equals_oracle(nnbvh_lib, mode):
    """Verdicts equal everywhere; outputs bit-equal wherever both are numbers, a NaN equal to a NaN (x86 and gfx950
    differ in the default NaN's sign)."""
    family = "tri" if mode == "tri_masks" else mode
    x, first, out, fcols = awkward(family)
    raw = run_device(nnbvh_lib, mode, x)
    assert_device_equals_oracle(mode, raw, first, out, fcols, awkward_hits(family))


@pytest.mark.gpu
def test_awkward_inputs_three_slab_forms_equal_the_oracle(nnbvh_lib):
    x, first, _, _ = awkward("slab")
    raw = run_device(nnbvh_lib, "slab", x)
    for k, form in enumerate(("slab_partial", "slab_entry_key", "slab_entry_key with masks")):
        bad = raw[:, k] != first
        assert not bad.any(), f"{form}: verdict differs on {bad.sum()} records, first {first_rows(bad)}"


# ---- c. all pairs through the real kernels ---------------------------------------------------------------------------
N_PAIRS = 4096


@functools.lru_cache(None)
def one_leaf_scene(which):
    """`tri`: the triangles of the first 4 096 leaf_tri records, private vertices, in one leaf, and their 4 096 rays with
    their golden tMax.  `mixed`: the first 2 048 triangles and the patches of the first 2 048 leaf_blp records in one
    leaf, with both ray sets.  Returns what the BVH and the kd-tree forms of the scene and the checks need."""
    from nn_bvh_amd import _lib, make_prims, make_rays
    t, thit, tbits = golden("tri")
    nt = N_PAIRS if which == "tri" else N_PAIRS // 2
    verts = t[:nt, 7:16].reshape(-1, 3)
    tris = np.arange(3 * nt, dtype=np.int32).reshape(nt, 3)
    recs, hit, t_gold = t[:nt], thit[:nt].astype(bool), tbits[:nt, 3].view(np.float32)
    patches = None
    if which == "mixed":
        b, bhit, bbits = golden("blp")
        nb = N_PAIRS - nt
        verts = np.concatenate([verts, b[:nb, 7:19].reshape(-1, 3)])
        patches = 3 * nt + np.arange(4 * nb, dtype=np.int32).reshape(nb, 4)
        recs = np.concatenate([recs[:, :7], b[:nb, :7]])
        hit = np.concatenate([hit, bhit[:nb].astype(bool)])
        t_gold = np.concatenate([t_gold, bbits[:nb, 2].view(np.float32)])
    verts = np.ascontiguousarray(verts, np.float32)
    prims = make_prims(tris, patches)
    rays = make_rays(recs[:, 0:3], recs[:, 3:6], recs[:, 6])
    bounds = np.concatenate([verts.min(0), verts.max(0)]).astype(np.float32)
    nodes = np.zeros(1, _lib.NODE_DTYPE)  # LinearBVHNode: a leaf of all the primitives, from offset 0
    nodes["pmin"], nodes["pmax"], nodes["nprims"] = bounds[:3], bounds[3:], len(prims)
    kd_nodes = np.zeros(1, _lib.KD_NODE_DTYPE)  # KdTreeNode::InitLeaf: flags = 3 | n << 2, offset 0 into the indices
    kd_nodes["flags"] = 3 | (len(prims) << 2)
    kd_idx = np.arange(len(prims), dtype=np.int32)
    return dict(verts=verts, prims=prims, rays=rays, bounds=bounds, nodes=nodes, kd_nodes=kd_nodes, kd_idx=kd_idx,
                gold_hit=hit, gold_t=t_gold)


@functools.lru_cache(None)
def one_leaf_oracle(which, tree):
    s = one_leaf_scene(which)
    nt = min(8, os.cpu_count() or 1)
    if tree == "bvh":
        return (ob.closest(s["nodes"], s["prims"], s["verts"], s["rays"], nt),
                ob.any_hit(s["nodes"], s["prims"], s["verts"], s["rays"], nt))
    return (ob.kd_closest(s["kd_nodes"], s["kd_idx"], s["prims"], s["verts"], s["bounds"], s["rays"], nt),
            ob.kd_any_hit(s["kd_nodes"], s["kd_idx"], s["prims"], s["verts"], s["bounds"], s["rays"], nt))


def closest_is_no_farther_than_the_golden_hit(s, hits):
    """wherever record i's golden verdict is `hit at t_i` and ray i reaches the leaf, the closest t is <= t_i"""
    m = s["gold_hit"] & (hits["prim_tests"] > 0)
    return m, (hits["prim"][m] >= 0) & (hits["t"][m] <= s["gold_t"][m])


@pytest.mark.parametrize("tree", ["bvh", "kd"])
def test_all_pairs_scene_reaches_its_leaf_on_the_oracle(tree):
    s = one_leaf_scene("tri")
    exp, _ = one_leaf_oracle("tri", tree)
    reached, hit = exp["prim_tests"] > 0, exp["prim"] >= 0
    print(f"{tree}: {reached.mean():.3%} of the rays reach the leaf, {hit.mean():.3%} hit something")
    assert reached.mean() >= 0.95 and hit.mean() > 0.90
    assert (exp["prim_tests"][reached] == N_PAIRS).all()  # closest hit: every primitive of the leaf is tested
    m, ok = closest_is_no_farther_than_the_golden_hit(s, exp)
    assert m.sum() > 1000 and ok.all()


@pytest.mark.parametrize("tree", ["bvh", "kd"])
def test_mixed_all_pairs_scene_reaches_its_leaf_on_the_oracle(tree):
    s = one_leaf_scene("mixed")
    exp, _ = one_leaf_oracle("mixed", tree)
    reached, hit = exp["prim_tests"] > 0, exp["prim"] >= 0
    is_patch = s["prims"]["kind"][np.maximum(exp["prim"], 0)] == 1
    print(f"{tree}: {reached.mean():.3%} of the rays reach the leaf, {hit.mean():.3%} hit something, "
          f"{(hit & is_patch).sum()} closest hits on a patch")
    assert reached.mean() >= 0.95 and hit.mean() > 0.90
    assert (hit & is_patch).sum() > 500 and (hit & ~is_patch).sum() > 500
    m, ok = closest_is_no_farther_than_the_golden_hit(s, exp)
    assert m.sum() > 1000 and ok.all()


def assert_records_equal(got, exp, what):
    """test_gpu_parity.assert_hits_equal's rules, a NaN equal to a NaN"""
    for f in ("prim", "nodes_visited", "prim_tests"):
        bad = got[f] != exp[f]
        assert not bad.any(), f"{what}: {f} differs on {bad.sum()} rays, first {first_rows(bad)}: " \
                              f"{got[f][first_rows(bad)]} vs {exp[f][first_rows(bad)]}"
    for f in ("t", "b0", "b1", "b2"):
        bad = (got[f].view(np.uint32) != exp[f].view(np.uint32)) & ~(np.isnan(got[f]) & np.isnan(exp[f]))
        assert not bad.any(), f"{what}: {f} not bit-equal on {bad.sum()} rays, first {first_rows(bad)}"


@pytest.mark.gpu
@pytest.mark.parametrize("tree", ["bvh", "kd"])
@pytest.mark.parametrize("which", ["tri", "mixed"])
def test_all_pairs_through_the_trace_kernels(nnbvh_lib, which, tree):
    """`tri` runs the lean kernel instances (triangle_test with the wave's masks), `mixed` the PATCH instances
    (triangle_test without masks, patch_test)."""
    from nn_bvh_amd import BVHAggregate
    from nn_bvh_amd.kdtree import KdTreeAggregate
    s = one_leaf_scene(which)
    exp, (eocc, evis, etst) = one_leaf_oracle(which, tree)
    if tree == "bvh":
        agg = BVHAggregate.from_tree(s["nodes"], s["prims"], s["verts"])
    else:
        agg = KdTreeAggregate.from_tree(s["kd_nodes"], s["kd_idx"], s["prims"], s["verts"], s["bounds"])
    try:
        got = agg.Intersect(s["rays"])
        occ, vis, tst = agg.IntersectP(s["rays"], counts=True)
    finally:
        agg.close()
    assert_records_equal(got, exp, f"{which} {tree} closest")
    assert np.array_equal(occ, eocc), f"{which} {tree} any: occluded differs on rays {first_rows(occ != eocc)}"
    assert np.array_equal(vis, evis) and np.array_equal(tst, etst), f"{which} {tree} any: counts differ"
    m, ok = closest_is_no_farther_than_the_golden_hit(s, got)
    assert ok.all(), f"{which} {tree}: closest hit beyond the golden hit on rays {np.nonzero(m)[0][~ok][:5]}"
