"""The trace kernels that address the scene through 64-bit offsets, run on small scenes and held to the oracle; and which
kernel instance every case here reaches, asserted with the launch ledger.

kd_trace.hip compiles every instance twice: O32 = 1 fetches nodes, primitive records and indices through 32-bit byte
offsets from a scalar base, O32 = 0 through 64-bit addressing.  kd_fits32 (kd_trace.h) picks O32 = 0 only for scenes of
2^26 - 1 primitive records, 2^29 nodes or 2^30 indices and more, which no test scene comes near.  The scene option
"offsets32" 0 (nnbvh_kd_scene_set_option, nnbvh_scene_set_option) makes a scene behave as if it did not fit 32-bit
offsets; 1 restores the width its sizes give.  On BVH scenes the same key turns scene_fits32 off: never the lean
instances, no LDS top table, wavefront queues gathered into records, walk form 1 instead of form 0.

nnbvh_instance_launches (the launch ledger; _lib.LaunchLedger) counts the launches of every kernel instance, so each
GPU case below asserts (c) WHICH instance its calls reached beside (a) the bytes against the oracle, (b) the bytes
against the same call at the other width and (d) the premise that makes the case worth running, taken from the
oracle's output.  Every case runs narrow, wide, narrow on ONE scene object: what the scene caches per width
(blocks_per_cu of a kd scene, walk_blocks_per_cu of a BVH scene) is dropped by the toggle, not by a second scene.

Scenes and oracles are those of the narrow tests, cut to at most about 2 000 primitives and 8 000 rays; a count the
narrow test asks of more rays is asked here as the same share of the rays (the helper `share`).  Where the narrow test
composes its expected values from device calls that exist without the walk (the walks on a scene with patches:
tests/test_wavefront_walk_kd.py), those calls are made at the narrow width, outside the ledger's block.

The census at the end computes, from the expected-instance tables here and the LEDGER tables of the modules that
tests/ledger_cases.py names, which of the 75 + 42 instances a ledger-asserted oracle comparison reaches: all of them."""
import contextlib
import ctypes
import functools
import math
import os

import numpy as np
import pytest

import oracle_binding as ob
from nn_bvh_amd import HIT_DTYPE, BVHAggregate, _lib, scene
from nn_bvh_amd.kdtree import KdTreeAggregate, build_kd_tree

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KD, BVH = _lib.FAMILY_KD, _lib.FAMILY_BVH
ERR_ARG = 1
MAX_RAYS, MAX_PRIMS = 8000, 2300  # "at most about 2 000 primitives" (the opaque attribute scene has 2 200)

# ---- the case tables ----------------------------------------------------------------------------------------------
# kd instances are (mode, patch, o32, attr, hostc) of kd_trace_kernel; a case id is "<scene form>-<call>"
KD_CASES = [
    ("lean-closest", (0, 0, 0, 0, 0)), ("lean-any", (1, 0, 0, 0, 0)), ("lean-batches", (2, 0, 0, 0, 0)),
    ("lean-queues", (3, 0, 0, 0, 0)), ("lean-candidates", (2, 0, 0, 0, 1)), ("lean-walk_shadow", (4, 0, 0, 0, 0)),
    ("lean-walk_one_random", (5, 0, 0, 0, 0)),
    ("patch-closest", (0, 1, 0, 0, 0)), ("patch-any", (1, 1, 0, 0, 0)), ("patch-batches", (2, 1, 0, 0, 0)),
    ("patch-candidates", (2, 1, 0, 0, 1)), ("patch-walk_shadow", (4, 1, 0, 0, 0)),
    ("patch-walk_one_random", (5, 1, 0, 0, 0)),
    ("attr-closest", (0, 1, 0, 1, 0)), ("attr-any", (1, 1, 0, 1, 0)), ("attr-batches", (2, 1, 0, 1, 0)),
    ("attr-candidates", (2, 1, 0, 1, 1)),
    ("tex-closest", (0, 1, 0, 2, 0)), ("tex-any", (1, 1, 0, 2, 0)), ("tex-batches", (2, 1, 0, 2, 0)),
    ("tex-candidates", (2, 1, 0, 2, 1)),
]
# BVH instances are (mode, window, inst, patch, alpha, soa, hostc) of trace_kernel.  Per case: what the calls reach on
# a triangle-only flat scene with offsets32 0 (the general instances), and with offsets32 1 (the lean ones)
G = lambda mode: (mode, 8, 0, 1, 0, 0, 0)  # noqa: E731
LEAN = lambda mode, soa=0: (mode, 8, 0, 0, 0, soa, 0)  # noqa: E731
BVH_CASES = [
    # Intersect, IntersectP with counts, IntersectP, trace_batches_device (closest + any)
    ("flat_calls", {G(0), G(1), G(2), G(3)}, {LEAN(0), LEAN(1), LEAN(2), LEAN(3)}),
    # IntersectClosest, IntersectShadow, IntersectClosestAndShadow on queues: gathered (wide) / read as SOA slices
    ("queue_calls", {G(0), G(2), G(3)}, {LEAN(0, 1), LEAN(2, 1), LEAN(3, 1)}),
    ("walk_shadow", {G(4)}, {LEAN(4)}),
    ("walk_one_random", {G(5)}, {LEAN(5)}),
]


def narrow_twin(instance):
    return instance[:2] + (1,) + instance[3:]


def share(count, of, n):
    """the count the narrow test asks of `of` rays, as the same share of n rays"""
    return math.ceil(count * n / of)


# ---- CPU: the ledger, the option's argument checks, the case table ------------------------------------------------------
def test_ledger_lists_the_75_bvh_instances_of_the_table(tmp_path, nnbvh_lib):
    from test_trace_instance import run_check
    lines = run_check(tmp_path / "trace_instance_check", [])
    table = {tuple(int(x) for x in ln[len("table <"):-1].split(",")) for ln in lines if ln.startswith("table ")}
    ledger = _lib.instance_launches(BVH)
    assert len(ledger) == len(table) == 75
    assert set(ledger) == table


def test_ledger_lists_42_kd_instances_closed_under_flipping_o32(nnbvh_lib):
    ledger = _lib.instance_launches(KD)
    assert len(ledger) == 42
    assert all(len(k) == 5 and k[2] in (0, 1) for k in ledger)
    flipped = {k[:2] + (1 - k[2],) + k[3:] for k in ledger}
    assert flipped == set(ledger), "an instance exists at one offset width only"
    assert sum(1 for k in ledger if k[2] == 0) == 21


def test_ledger_call_checks_its_arguments_and_needs_no_device(nnbvh_lib):
    L = nnbvh_lib
    assert L.nnbvh_instance_launches(0, None, None, 0, 0) == 75
    assert L.nnbvh_instance_launches(1, None, None, 0, 0) == 42
    for family in (-1, 2):
        assert L.nnbvh_instance_launches(family, None, None, 0, 0) == -ERR_ARG
        assert "instance_launches" in _lib.last_error()
    assert L.nnbvh_instance_launches(0, None, None, -1, 0) == -ERR_ARG
    assert L.nnbvh_instance_launches(0, None, None, 4, 0) == -ERR_ARG  # rows asked for, nowhere to put them
    # a short capacity fills that many rows and still returns the number of instances
    desc, counts = np.full((3, 7), -9, np.int32), np.full(3, 99, np.uint64)
    assert L.nnbvh_instance_launches(1, _lib.ptr(desc), _lib.ptr(counts), 2, 0) == 42
    assert (desc[2] == -9).all() and counts[2] == 99 and (desc[:2, 5:] == 0).all() and (desc[:2, :5] >= 0).all()
    # nothing launches on this side of a device: a ledger block sees no launch, reset or not
    with _lib.LaunchLedger(KD) as led:
        _lib.instance_launches(KD, reset=False)
    assert led.launched == {}


def test_offsets32_refuses_other_values_before_the_scene_is_looked_at(nnbvh_lib):
    L = nnbvh_lib
    for fn, words in ((L.nnbvh_scene_set_option, "set_option: offsets32 must be 0 or 1"),
                      (L.nnbvh_kd_scene_set_option, "kd_scene_set_option: offsets32 must be 0 or 1")):
        for bad in (2, -1, 32, 1 << 30):
            assert fn(None, b"offsets32", bad) == ERR_ARG
            assert _lib.last_error() == words, (bad, _lib.last_error())
        for good in (0, 1):  # the value is fine: the null scene is what is refused
            assert fn(None, b"offsets32", good) == ERR_ARG
            assert "null argument" in _lib.last_error()
        assert fn(None, None, 2) == ERR_ARG and "null argument" in _lib.last_error()
    header = open(os.path.join(ROOT, "include", "nnbvh.h")).read()
    assert header.count('"offsets32"') >= 2 and "nnbvh_instance_launches(" in header
    assert "nnbvh_instance_launches" in _lib.EXPORTS
    assert L.nnbvh_instance_launches.restype is ctypes.c_int


def test_case_table_names_every_wide_kd_instance_once(nnbvh_lib):
    wide = {k for k in _lib.instance_launches(KD) if k[2] == 0}
    named = [inst for _, inst in KD_CASES]
    assert len(named) == len(set(named)) == 21, "an instance named twice"
    assert set(named) == wide
    assert len({cid for cid, _ in KD_CASES}) == 21
    for cid, inst in KD_CASES:
        form, call = cid.split("-", 1)
        assert form in KD_FORMS and call in KD_CALLS, cid
        # the table is consistent with what the form and the call mean
        assert inst[1] == (0 if form == "lean" else 1) and inst[3] == {"lean": 0, "patch": 0, "attr": 1, "tex": 2}[form]
        assert inst[4] == (1 if call == "candidates" else 0)
        assert inst[0] == {"closest": 0, "any": 1, "batches": 2, "queues": 3, "candidates": 2, "walk_shadow": 4,
                           "walk_one_random": 5}[call]
    for _, wide_set, narrow_set in BVH_CASES:
        ledger = _lib.instance_launches(BVH)
        assert wide_set <= set(ledger) and narrow_set <= set(ledger) and not (wide_set & narrow_set)


# ---- device helpers ---------------------------------------------------------------------------------------------------
def _dev():
    import torch
    return torch.device("cuda", 0)


def _bytes(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(_dev())


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def batches_call(agg, rays):
    """trace_batches_device: a closest batch and an any-hit batch with counts over the rays reversed, ONE launch"""
    import torch
    n = len(rays)
    rev = rays[::-1].copy()
    dc, da = _bytes(rays), _bytes(rev)
    oc = torch.full((n * 32,), 0x5A, dtype=torch.uint8, device=_dev())
    oa = torch.full((n,), 0x5A, dtype=torch.uint8, device=_dev())
    ov = torch.full((n,), -7, dtype=torch.int32, device=_dev())
    ot = torch.full((n,), -7, dtype=torch.int32, device=_dev())
    if isinstance(agg, KdTreeAggregate):
        any_batch = ("any", da.data_ptr(), n, oa.data_ptr(), ov.data_ptr(), ot.data_ptr())
    else:  # (a BVH batch with counts is not fusable: occlusion only)
        any_batch = ("any", da.data_ptr(), n, oa.data_ptr())
    agg.trace_batches_device([("closest", dc.data_ptr(), n, oc.data_ptr()), any_batch],
                             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return {"batch_hits": oc.cpu().numpy().view(HIT_DTYPE), "batch_occ": oa.cpu().numpy()[::-1].copy(),
            "batch_visited": ov.cpu().numpy()[::-1].copy(), "batch_tests": ot.cpu().numpy()[::-1].copy()}


QUEUE_SHORT = 137  # the queues' device-side size lies this far below their capacity


def queue_calls(agg, rays):
    """IntersectClosest, IntersectShadow and IntersectClosestAndShadow on RayQueues (tests/test_stack_limits.py
    check_queue_calls): hit records, occlusion flags and radiance of the single calls and of the pair call"""
    import torch
    from nn_bvh_amd.wavefront import RayQueue, WavefrontAggregate
    from test_wavefront import shadow_inputs
    cap = len(rays)
    n = cap - QUEUE_SHORT
    Ld, r_u, r_l, px, L = shadow_inputs(cap, cap + 500, 7)
    wf = WavefrontAggregate(agg)
    rq, sq = RayQueue.from_records(rays, _dev()), RayQueue.from_records(rays, _dev(), shadow=True)
    rq.size.fill_(n)
    sq.size.fill_(n)
    res = {}
    for call in ("single", "pair"):
        hits_t = torch.full((cap, 32), 0xAB, dtype=torch.uint8, device=_dev())
        l_t, occ_t = _t(L), torch.full((cap,), 9, dtype=torch.uint8, device=_dev())
        if call == "single":
            wf.IntersectClosest(cap, rq, hits=hits_t)
            wf.IntersectShadow(cap, sq, _t(Ld), _t(r_u), _t(r_l), _t(px), l_t, occluded=occ_t)
        else:
            wf.IntersectClosestAndShadow(cap, rq, cap, sq, _t(Ld), _t(r_u), _t(r_l), _t(px), l_t, hits=hits_t,
                                         occluded=occ_t)
        torch.cuda.synchronize()
        res[call + "_hits"], res[call + "_occ"] = hits_t.cpu().numpy(), occ_t.cpu().numpy()
        res[call + "_L"] = l_t.cpu().numpy()
    return res


def check_queue_results(res, exp_far, eocc, cap, what):
    """exp_far: the oracle's closest records of the first n rays with tMax = Infinity (a closest queue carries none);
    eocc: its any-hit flags of the first n rays as they are"""
    from test_wavefront import shadow_inputs
    n = cap - QUEUE_SHORT
    Ld, r_u, r_l, px, L = shadow_inputs(cap, cap + 500, 7)
    exp_l = ob.record_shadow(eocc, Ld[:n], r_u[:n], r_l[:n], px[:n], L)
    for call in ("single", "pair"):
        hits, occ = res[call + "_hits"], res[call + "_occ"]
        assert hits[:n].tobytes() == exp_far.tobytes(), f"{what} {call}: hit records"
        assert (hits[n:] == 0xAB).all() and (occ[n:] == 9).all(), f"{what} {call}: wrote beyond the size"
        assert np.array_equal(occ[:n], eocc), f"{what} {call}: occlusion flags"
        assert np.array_equal(res[call + "_L"].view(np.uint32), exp_l.view(np.uint32)), f"{what} {call}: radiance"


def assert_same_bytes(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), f"{what}: {k} differs"


def narrow_wide_narrow(job, family, wide, narrow, what):
    """job.agg through offsets32 1, 0, 1 with job.run() under the ledger at each width: (c) exactly `wide` / `narrow`
    launch, (a) job.check at each width, (b) the same bytes at all three"""
    results = []
    for width, want in ((1, narrow), (0, wide), (1, narrow)):
        job.agg.set_option("offsets32", width)
        with _lib.LaunchLedger(family) as led:
            res = job.run()
        assert set(led.launched) == set(want), \
            f"{what}, offsets32 {width}: launched {sorted(led.launched.items())}, expected {sorted(want)}"
        assert all(v >= 1 for v in led.launched.values())
        job.check(res, f"{what}, offsets32 {width}")
        results.append(res)
    assert_same_bytes(results[1], results[0], f"{what}: wide against narrow")
    assert_same_bytes(results[2], results[0], f"{what}: narrow again after wide")


# ---- kd scene forms -----------------------------------------------------------------------------------------------------
class Form:
    """A kd scene of one form: `plain` (tree, prims) for the plain calls, `host` (tree, prims with host-only primitives)
    for the candidate calls; the oracle's attribute arrays; the rays."""
    attrs = (None, None, None)  # normals, uvs, prim_alpha
    kw = {}                     # what from_tree takes beside the tree

    @contextlib.contextmanager
    def oracle_attributes(self):
        normals, uvs, alpha = self.attrs
        try:
            ob.set_vertex_normals(normals)
            ob.set_vertex_uvs(uvs)
            ob.set_prim_alpha(alpha)
            yield
        finally:
            ob.set_vertex_normals(None)
            ob.set_vertex_uvs(None)
            ob.set_prim_alpha(None)

    def aggregate(self, which="plain"):
        tree, prims = getattr(self, which)
        return KdTreeAggregate.from_tree(tree.nodes, tree.prim_indices, prims, self.verts, tree.bounds, **self.kw)

    def oracle(self, fn, which="plain", rays=None):
        tree, prims = getattr(self, which)
        with self.oracle_attributes():
            return fn(tree.nodes, tree.prim_indices, prims, self.verts, tree.bounds, self.rays if rays is None else rays, 4)

    @functools.lru_cache(None)
    def closest(self, which="plain"):
        return self.oracle(ob.kd_closest, which)

    @functools.lru_cache(None)
    def any_hit(self, which="plain"):
        return self.oracle(ob.kd_any_hit, which)

    def n_prims(self):
        return max(len(self.plain[1]), len(self.host[1]))


class SoupForm(Form):
    """tests/test_kd_host_candidates.py Soup: 1 500 triangles (+ 300 bilinear patches: the patch form), every 7th
    triangle host-only in the `host` scene; every third of its rays (6 000 with infinite, 2 000 with finite tMax)"""

    def __init__(self, seed, n_patches):
        import test_kd_host_candidates as khc
        self.khc = khc
        s = self.soup = khc.soup(seed, 4, n_patches)
        self.verts, self.rays = s.verts, s.rays[::3].copy()
        self.plain, self.host = (s.tree_t, s.prims), (s.tree_h, s.hp)
        self.walk_prims, self.tri_prims, self.host_mask = s.hp, s.prims, s.host
        self.host_wins = (50, 24000)  # the narrow test: more than 50 of its 24 000 rays

    @functools.lru_cache(None)
    def walker(self, closest):
        return self.khc.kd_walk(self.host[0], self.walk_prims, self.verts, self.rays, closest)

    def premise(self):
        exp, (occ, _, _) = self.closest(), self.any_hit()
        n = len(self.rays)
        assert (exp["prim"] >= 0).mean() > 0.2 and exp["nodes_visited"].max() > 20  # tests/test_kd_wavefront.py
        assert 0.05 < (occ == 1).mean() < 0.95
        if len(self.tri_prims) > 1500:  # tests/test_kd_host_candidates.py: more than 100 of 24 000 rays hit a patch
            hit_kind = self.tri_prims["kind"][np.maximum(exp["prim"], 0)][exp["prim"] >= 0]
            assert (hit_kind == 1).sum() > share(100, 24000, n)

    def candidates_premise(self):
        w = self.walker(True)
        assert (w["count"] > 16).mean() <= 0.01 and (w["count"] > 0).mean() > 0.05


class AttrForm(Form):
    """The scene of test_device_kd_traversal_with_attribute_reading_alpha_kinds (tests/test_kdtree.py) at half its
    size: 750 triangles (plain, constant alpha, half of those smooth) and 1 250 twisted patches of kinds 1, 8 .. 15;
    8 000 of its rays in the same 5 : 1 mix.  `host`: tests/test_kd_host_candidates.py OpaqueAttrScene, the
    attribute scene whose walk the list walker restates (alpha 1 everywhere), every second of its rays."""
    N_NARROW = 48000

    def __init__(self):
        import test_kd_host_candidates as khc
        from test_alpha import alpha_patch_scene, patch_uvs
        self.khc = khc
        verts, prims, normals, alpha, kinds = alpha_patch_scene(43, 750, 1250)
        rng = np.random.default_rng(4)
        prims = prims.copy()
        smooth = ((kinds == 4) | (kinds == 5)) & (rng.random(len(prims)) < 0.5)
        prims["kind"] = np.where(smooth, kinds + 2, kinds)
        uvs = patch_uvs(verts)
        self.verts, self.attrs = verts, (normals, uvs, alpha)
        self.kw = dict(normals=normals, uvs=uvs, prim_alpha=alpha)
        self.plain = (build_kd_tree(prims, verts, max_prims=2), prims)
        self.rays = np.concatenate([scene.random_rays(6667, verts.min(0) - 1, verts.max(0) + 1, 21),
                                    scene.random_rays(1333, verts.min(0), verts.max(0), 22, tmax=0.6)])
        self.host = self.plain  # (n_prims; the candidates case has a form of its own: opaque())

    def premise(self):
        exp = self.closest()
        prims = self.plain[1]
        hit_kind = prims["kind"][np.maximum(exp["prim"], 0)]
        for k in (6, 7, 8, 9, 10, 11, 12, 13, 14, 15):  # the narrow test: more than 50 of 48 000 rays, each kind
            assert ((hit_kind == k) & (exp["prim"] >= 0)).sum() > share(50, self.N_NARROW, len(self.rays)), k
        # alpha rejections: the record differs from the walk of the same primitives with every alpha at 1
        opaque = prims.copy()
        tri_alpha = np.isin(prims["kind"], (4, 5, 6, 7))
        opaque["v"][tri_alpha, 3] = np.ones(1, np.float32).view(np.int32)[0]
        normals, uvs, alpha = self.attrs
        tree = self.plain[0]
        try:
            ob.set_vertex_normals(normals)
            ob.set_vertex_uvs(uvs)
            ob.set_prim_alpha(np.ones_like(alpha))
            base = ob.kd_closest(tree.nodes, tree.prim_indices, opaque, self.verts, tree.bounds, self.rays, 4)
        finally:
            ob.set_vertex_normals(None)
            ob.set_vertex_uvs(None)
            ob.set_prim_alpha(None)
        rejected = (exp["prim"] != base["prim"]) | (exp["prim_tests"] != base["prim_tests"])
        assert rejected.mean() > 0.1, "rays whose walk differs from the walk without alpha: a hit was rejected"


class OpaqueAttrForm(Form):
    def __init__(self):
        import test_kd_host_candidates as khc
        self.khc = khc
        s = self.scene = khc.opaque_attr_scene()
        self.verts, self.rays = s.verts, s.rays[::2].copy()
        self.attrs = (s.normals, s.uvs, s.alpha)
        self.kw = dict(normals=s.normals, uvs=s.uvs, prim_alpha=s.alpha)
        self.plain, self.host = (s.tree_t, s.prims), (s.tree_h, s.hp)
        self.walk_prims, self.tri_prims, self.host_mask = s.walk_prims, s.prims, s.host
        self.host_wins = (50, 16000)

    @functools.lru_cache(None)
    def walker(self, closest):
        return self.khc.kd_walk(self.host[0], self.walk_prims, self.verts, self.rays, closest)

    def candidates_premise(self):
        w = self.walker(True)
        assert (w["count"] > 16).mean() <= 0.01 and (w["count"] > 0).mean() > 0.05
        exp = self.closest("plain")  # the attribute-reading kinds are hit (narrow: 100 and 50 of 16 000 rays)
        hit_kind = self.tri_prims["kind"][np.maximum(exp["prim"], 0)][exp["prim"] >= 0]
        assert (hit_kind >= 8).sum() > share(100, 16000, len(self.rays))
        assert np.isin(hit_kind, (6, 7)).sum() > share(50, 16000, len(self.rays))


class TexForm(Form):
    """tests/test_kd_alpha_texture.py case("soup", 4): 600 triangles, a third each plain, constant alpha and image-
    textured (kinds 16 .. 19), 3 072 rays, the per-ray oracle.  `host`: every third plain triangle host-only, as
    test_mixed_with_host_only_primitives_through_candidates declares them."""

    def __init__(self):
        import test_kd_alpha_texture as kat
        self.kat = kat
        c = self.case = kat.case("soup", 4, True)
        self.verts, self.rays = c.verts, c.rays
        self.kw = dict(normals=c.normals, uvs=c.uvs, alpha_textures=c.textures)
        self.host_mask = (c.prims["kind"] == 0) & (np.arange(len(c.prims)) % 3 == 0)
        hp = c.prims.copy()
        hp["kind"][self.host_mask] = 3
        self.plain, self.host = (c.tree, c.prims), (c.tree, hp)
        self.tri_prims = c.prims
        self.host_wins = (20, 3072)

    @functools.lru_cache(None)
    def closest(self, which="plain"):
        c = self.case
        if which == "plain":
            return c.closest
        return self.kat.KdPerRayOracle(c.tree, self.host[1], c.verts, c.rays, c.normals, c.alpha, c.tex).closest()

    @functools.lru_cache(None)
    def any_hit(self, which="plain"):
        c = self.case
        if which == "plain":
            return c.any_hit
        return self.kat.KdPerRayOracle(c.tree, self.host[1], c.verts, c.rays, c.normals, c.alpha, c.tex).any_hit()

    def premise(self):
        differs, accepted_mid, textured = self.kat.alpha_test_shares(self.case)
        assert differs >= 0.10 and accepted_mid >= 0.10 and textured > 0.10

    def candidates_premise(self):
        self.premise()
        tri = self.verts[self.case.prims["v"][:, :3]]
        bounds = np.concatenate([tri.min(1), tri.max(1)], 1).astype(np.float32)
        self.kat.assert_same_tree(build_kd_tree(self.host[1], self.verts, prim_bounds=bounds, max_prims=4),
                                  self.case.tree, "host-only, exact bounds")
        void = self.closest("host")["instance"] == -1  # the rays that reach a host-only primitive
        assert void.mean() > 0.05


@functools.lru_cache(None)
def lean_form():
    return SoupForm(0, 0)


@functools.lru_cache(None)
def patch_form():
    return SoupForm(2, 300)


@functools.lru_cache(None)
def attr_form():
    return AttrForm()


@functools.lru_cache(None)
def opaque_attr_form():
    return OpaqueAttrForm()


@functools.lru_cache(None)
def tex_form():
    return TexForm()


KD_FORMS = {"lean": lean_form, "patch": patch_form, "attr": attr_form, "tex": tex_form}


# ---- kd calls: a job has .agg, .run() -> {name: array}, .check(result, what), .close() -------------------------------------
class PlainJob:
    """closest: Intersect; any: IntersectP with counts; batches: both in one launch of the batch-mode instance"""

    def __init__(self, form, call):
        form.premise()
        self.form, self.call, self.agg = form, call, form.aggregate()

    def run(self):
        rays = self.form.rays
        if self.call == "closest":
            return {"hits": self.agg.Intersect(rays)}
        if self.call == "any":
            occ, vis, tst = self.agg.IntersectP(rays, counts=True)
            return {"occ": occ, "visited": vis, "tests": tst, "occ_only": self.agg.IntersectP(rays)}
        return batches_call(self.agg, rays)

    def check(self, res, what):
        exp, (eo, ev, et) = self.form.closest(), self.form.any_hit()
        if self.call == "closest":
            assert res["hits"].tobytes() == exp.tobytes(), f"{what}: closest-hit records"
        elif self.call == "any":
            assert np.array_equal(res["occ"], eo) and np.array_equal(res["visited"], ev), f"{what}: any hit"
            assert np.array_equal(res["tests"], et) and np.array_equal(res["occ_only"], eo), f"{what}: any hit"
        else:
            assert res["batch_hits"].tobytes() == exp.tobytes(), f"{what}: closest batch"
            assert np.array_equal(res["batch_occ"], eo) and np.array_equal(res["batch_visited"], ev), f"{what}: any batch"
            assert np.array_equal(res["batch_tests"], et), f"{what}: any batch"

    def close(self):
        self.agg.close()


class QueuesJob:
    """lean scenes, read_soa 1: the three queue calls run the SOA form of the batch-mode instance (mode 3)"""

    def __init__(self, form, call):
        form.premise()
        self.form, self.agg = form, form.aggregate()
        self.agg.set_option("read_soa", 1)

    def run(self):
        return queue_calls(self.agg, self.form.rays)

    def check(self, res, what):
        n = len(self.form.rays) - QUEUE_SHORT
        far = self.form.rays[:n].copy()
        far["tmax"] = np.inf
        exp_far = self.form.oracle(ob.kd_closest, rays=far)
        assert (exp_far["prim"] >= 0).mean() > 0.2
        check_queue_results(res, exp_far, self.form.any_hit()[0][:n], len(self.form.rays), what)

    def close(self):
        self.agg.close()


class CandidatesJob:
    """The candidate twin: the single-batch closest and any-hit calls with candidates on the `host` scene.  Lean, patch
    and (opaque) attribute scenes: lists, counts and `before` against the list walker exactly, the records against the
    oracle on the host scene but for `instance`.  Textured scene (no walker restates it): the records against the
    per-ray oracle on the host scene, the resolved answers against it on the scene with every triangle on the device."""

    def __init__(self, form, call):
        self.form = opaque_attr_form() if isinstance(form, AttrForm) else form
        self.form.candidates_premise()
        self.agg = self.form.aggregate("host")

    def run(self):
        hits, cands = self.agg.intersect_with_host_candidates(self.form.rays, capacity=16)
        occ, acands = self.agg.intersect_p_with_host_candidates(self.form.rays, capacity=16)
        return {"hits": hits, "cands": cands, "occ": occ, "any_cands": acands}

    def check(self, res, what):
        from nn_bvh_amd import resolve_host_candidates, resolve_host_candidates_any
        from test_host_candidates import assert_resolved_equal, assert_same_but_instance, tri_callback, tri_table
        f = self.form
        hits, cands, occ, acands = res["hits"], res["cands"], res["occ"], res["any_cands"]
        exp_h, (eo_h, _, _) = f.closest("host"), f.any_hit("host")
        cnt = cands["count"]
        assert_same_but_instance(hits, exp_h)
        assert np.array_equal(exp_h["instance"] == -1, cnt != 0), what
        assert np.array_equal(hits["instance"], np.where(cnt < 0, -1, 0)), what
        assert np.array_equal(occ, eo_h) and np.array_equal(occ == 2, (acands["count"] != 0) & (occ != 1)), what
        assert (acands["before"] == 0).all()
        ok = cnt >= 0
        assert ok.mean() >= 0.99
        cb = tri_callback(f.rays, f.verts, tri_table(f.tri_prims))
        kind = f.tri_prims["kind"] if not isinstance(f, TexForm) else np.zeros(len(f.tri_prims), np.int32)
        resolved = resolve_host_candidates(f.rays, hits, cands, cb, kind=kind)
        assert_resolved_equal(resolved[ok], f.closest("plain")[ok], what)
        won = (resolved["prim"] >= 0) & f.host_mask[np.maximum(resolved["prim"], 0)]
        assert won[ok].sum() > share(*f.host_wins, len(f.rays)), what  # a host-only primitive is the closest hit
        got = resolve_host_candidates_any(f.rays, occ, acands, cb)
        settled = got != 2
        assert settled.mean() > 0.99 and np.array_equal(got[settled], f.any_hit("plain")[0][settled]), what
        if not isinstance(f, TexForm):
            w, a = f.walker(True), f.walker(False)
            f.khc.assert_lists_equal(cands, f.khc.walker_cands(w))
            f.khc.assert_lists_equal(acands, f.khc.walker_cands(a), closest=False)
            assert hits[ok].tobytes() == w["hits"][ok].tobytes(), what
            assert np.array_equal(occ == 1, a["occluded"] == 1), what

    def close(self):
        self.agg.close()


class LeanWalkJob:
    """tests/test_wavefront_walk_kd.py: the layered scene, the composed reference, ShadowDevice / OneRandomDevice"""

    def __init__(self, form, call):
        import test_wavefront_walk_kd as wk
        self.wk, self.shadow = wk, call == "walk_shadow"
        self.c = wk.layered_case() if self.shadow else wk.one_random_case()
        c = self.c
        assert len(c.prims) <= MAX_PRIMS and c.n <= MAX_RAYS
        assert (c.calls > 1).sum() > 20, "items that walk through more than one surface"
        if self.shadow:
            assert min((c.state == 0).sum(), (c.state == 1).sum()) > 20
        else:
            assert (c.hits["prim"] >= 0).sum() > 20
        self.d = wk.ShadowDevice(c) if self.shadow else wk.OneRandomDevice(c)
        self.agg = self.d.agg

    def run(self):
        if self.shadow:
            state, L, unfinished = self.d.run(self.wk.UNCAPPED)
            return {"state": state, "L": L, "unfinished": np.array([unfinished])}
        gh, gr, pdf, wsum, unfinished = self.d.run(self.wk.UNCAPPED)
        return {"sel_hits": gh, "sel_rays": gr, "pdf": pdf, "wsum": wsum, "unfinished": np.array([unfinished])}

    def check(self, res, what):
        wk = self.wk
        assert res["unfinished"][0] == 0, what
        if self.shadow:
            exp_state, exp_L = wk.shadow_expected(self.c, wk.UNCAPPED)
            assert np.array_equal(res["state"], exp_state) and res["L"].tobytes() == exp_L.tobytes(), what
        else:
            got = (res["sel_hits"], res["sel_rays"], res["pdf"], res["wsum"])
            assert wk.check_one_random(self.c, got, wk.UNCAPPED) == 0, what

    def close(self):
        self.d.close()


class PatchWalkJob:
    """test_gpu_walks_beyond_flat_triangles of tests/test_wavefront_walk_kd.py on its patch scene (300 triangles, 100
    patches): the FULL walk instances.  As there, the expected values are the reference loop over calls that exist
    without the walk — KdTreeAggregate.Intersect, the interaction post-pass, ob.offset_batch — made here at the narrow
    width before the ledger's blocks; the closest-hit call of that loop is itself held to the oracle first."""

    def __init__(self, form, call):
        import torch
        import test_wavefront_walk_kd as wk
        from nn_bvh_amd.interaction import ShadingMesh
        from nn_bvh_amd.wavefront import RayQueue, WavefrontAggregate
        from test_wavefront_bounded import patch_scene
        self.wk, self.shadow = wk, call == "walk_shadow"
        s = patch_scene()
        _, prims, verts = s["tree"]
        prims = np.sort(prims, order="id")
        kd = build_kd_tree(prims, verts)
        self.agg = agg = KdTreeAggregate.from_tree(kd.nodes, kd.prim_indices, prims, verts, kd.bounds)
        self.mesh = mesh = ShadingMesh(verts, **s["mesh"])
        assert agg.info()["has_patches"] and len(prims) <= MAX_PRIMS
        rng = np.random.default_rng(31)
        box = s["box"]
        if self.shadow:
            n = self.n = 2001
            cls = rng.choice(np.array([0, 2, 2, 2, 2, 6], np.uint8), s["n_ids"])
            self.wf = WavefrontAggregate(agg, cls)
            rays = scene.random_rays(n, [-box] * 3, [box] * 3, 32, tmax=1 - 1e-4)
            rays["d"][::97] = 0
            rays["time"] = rng.random(n).astype(np.float32)
            exp = ob.kd_closest(kd.nodes, kd.prim_indices, prims, verts, kd.bounds, rays, 4)
            assert agg.Intersect(rays).tobytes() == exp.tobytes()
            self.q = RayQueue.from_records(rays, _dev(), shadow=True)
            self.q.time = _t(rays["time"])
            self.Ld, self.ru, self.rl = ((rng.random((n, 4), np.float32) + 0.5).astype(np.float32) for _ in range(3))
            self.pixel = rng.permutation(n).astype(np.int32)
            self.L0 = rng.random((n, 4), np.float32).astype(np.float32)
            self.ref_state, calls = wk.device_shadow_walk(agg, mesh, rays, cls)
            assert min((self.ref_state == 0).sum(), (self.ref_state == 1).sum()) > 20 and (calls > 1).sum() > 20
        else:
            m = self.n = 1501
            rng = np.random.default_rng(33)
            self.wf = WavefrontAggregate(agg)
            self.p0 = rng.uniform(-box, box, (m, 3)).astype(np.float32)
            self.p1 = rng.uniform(-box, box, (m, 3)).astype(np.float32)
            self.p1[::50] = self.p0[::50]
            self.material = rng.integers(0, 3, m).astype(np.int32)
            self.prim_material = rng.integers(0, 3, s["n_ids"]).astype(np.int32)
            self.exp = wk.device_one_random_walk(agg, mesh, self.p0, self.p1, self.material, self.prim_material)
            eh, _, _, _, ecalls, host = self.exp
            assert not host.any() and (eh["prim"] >= 0).sum() > 20 and (ecalls > 1).sum() > 20
        self.unfinished = torch.full((1,), -3, dtype=torch.int32, device=_dev())

    def run(self):
        import torch
        from test_wavefront_bounded import SENTINEL, one_random_numpy
        wk = self.wk
        if self.shadow:
            L, state = _t(self.L0), torch.full((self.n,), SENTINEL, dtype=torch.uint8, device=_dev())
            self.wf.WalkShadowTr(self.n, self.q, self.mesh, _t(self.Ld), _t(self.ru), _t(self.rl), _t(self.pixel), L,
                                 state, max_surfaces=wk.UNCAPPED, unfinished=self.unfinished)
            torch.cuda.synchronize()
            return {"state": state.cpu().numpy(), "L": L.cpu().numpy(),
                    "unfinished": np.array([int(self.unfinished.item())])}
        out = self.wf.WalkOneRandom(self.n, _t(self.p0), _t(self.p1), _t(self.material), self.mesh,
                                    _t(self.prim_material), max_surfaces=wk.UNCAPPED, unfinished=self.unfinished)
        torch.cuda.synchronize()
        gh, gr, pdf, wsum = one_random_numpy(out)
        return {"sel_hits": gh, "sel_rays": gr, "pdf": pdf, "wsum": wsum,
                "unfinished": np.array([int(self.unfinished.item())])}

    def check(self, res, what):
        from test_wavefront_bounded import shadow_radiance
        assert res["unfinished"][0] == 0, what
        if self.shadow:
            assert np.array_equal(res["state"], self.ref_state), what
            exp_L = shadow_radiance(self.ref_state, self.Ld, self.ru, self.rl, self.pixel, self.L0)
            assert res["L"].tobytes() == exp_L.tobytes(), what
        else:
            eh, er, epdf, ewsum, _, _ = self.exp
            gh, gr = res["sel_hits"], res["sel_rays"]
            assert (gh["instance"] != -1).all() and np.array_equal(gh["prim"], eh["prim"]), what
            assert np.array_equal(res["pdf"].view(np.uint32), epdf.view(np.uint32)), what
            assert np.array_equal(res["wsum"].view(np.uint32), ewsum.view(np.uint32)), what
            sel = eh["prim"] >= 0
            assert gh[sel].tobytes() == eh[sel].tobytes() and gr[sel].tobytes() == er[sel].tobytes(), what

    def close(self):
        self.agg.close()
        self.mesh.close()


def walk_job(form, call):
    return (LeanWalkJob if form is lean_form() else PatchWalkJob)(form, call)


KD_CALLS = {"closest": PlainJob, "any": PlainJob, "batches": PlainJob, "queues": QueuesJob, "candidates": CandidatesJob,
            "walk_shadow": walk_job, "walk_one_random": walk_job}


def test_kd_scenes_are_small_and_their_premises_hold():
    """(d) of every plain and candidate case, on the CPU: the GPU cases assert the same from the same cached oracle
    outputs.  (The walk cases' premises need their scenes' reference loops: asserted where the jobs are made.)"""
    for name, make in list(KD_FORMS.items()) + [("opaque attr", opaque_attr_form)]:
        form = make()
        assert len(form.rays) <= MAX_RAYS and form.n_prims() <= MAX_PRIMS, name
        if hasattr(form, "premise"):
            form.premise()
        if hasattr(form, "candidates_premise"):
            form.candidates_premise()


# ---- GPU: one case per wide kd instance ---------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("case_id,instance", KD_CASES, ids=[c for c, _ in KD_CASES])
def test_kd_wide_instance(case_id, instance):
    form_name, call = case_id.split("-", 1)
    job = KD_CALLS[call](KD_FORMS[form_name](), call)
    try:
        narrow_wide_narrow(job, KD, {instance}, {narrow_twin(instance)}, case_id)
    finally:
        job.close()


# ---- GPU: a triangle-only flat BVH scene with offsets32 0 -------------------------------------------------------------
@functools.lru_cache(None)
def flat_scene():
    """the golden mesh of smoke(): 4 K triangles, 8 K rays, and the oracle's answers"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "traversal_small.npz"))
    nodes, prims, verts, rays = g["nodes"], g["ordered_prims"], g["verts"], g["rays"][:MAX_RAYS]
    exp = ob.closest(nodes, prims, verts, rays)
    eany = ob.any_hit(nodes, prims, verts, rays)
    n = len(rays) - QUEUE_SHORT
    far = rays[:n].copy()
    far["tmax"] = np.inf
    return nodes, prims, verts, rays, exp, eany, ob.closest(nodes, prims, verts, far)


class BvhFlatJob:
    def __init__(self, queues):
        nodes, prims, verts, self.rays, self.exp, self.eany, self.exp_far = flat_scene()
        assert (prims["kind"] == 0).all(), "a triangle-only scene: lean at the narrow width"
        assert 0.2 < (self.exp["prim"] >= 0).mean() and 0.05 < (self.eany[0] == 1).mean() < 0.95
        self.queues = queues
        self.agg = BVHAggregate.from_tree(nodes, prims, verts)

    def run(self):
        if self.queues:
            return queue_calls(self.agg, self.rays)
        res = {"hits": self.agg.Intersect(self.rays), "occ_only": self.agg.IntersectP(self.rays)}
        res["occ"], res["visited"], res["tests"] = self.agg.IntersectP(self.rays, counts=True)
        b = batches_call(self.agg, self.rays)
        res["batch_hits"], res["batch_occ"] = b["batch_hits"], b["batch_occ"]
        return res

    def check(self, res, what):
        eo, ev, et = self.eany
        if self.queues:
            n = len(self.rays) - QUEUE_SHORT
            return check_queue_results(res, self.exp_far, eo[:n], len(self.rays), what)
        assert res["hits"].tobytes() == self.exp.tobytes(), f"{what}: closest-hit records"
        assert np.array_equal(res["occ"], eo) and np.array_equal(res["visited"], ev), f"{what}: any hit with counts"
        assert np.array_equal(res["tests"], et) and np.array_equal(res["occ_only"], eo), f"{what}: any hit"
        assert res["batch_hits"].tobytes() == self.exp.tobytes(), f"{what}: closest batch of the one-launch form"
        assert np.array_equal(res["batch_occ"], eo), f"{what}: any batch of the one-launch form"

    def close(self):
        self.agg.close()


class BvhWalkJob:
    """tests/test_wavefront_walk_on_bvh.py: the layered scene as a BVH, max_surfaces selects the walk instances"""

    def __init__(self, shadow):
        import test_wavefront_walk_on_bvh as wb
        self.wb, self.shadow = wb, shadow
        c = self.c = wb.bvh_layered_case() if shadow else wb.bvh_one_random_case()
        assert (c.calls > 1).sum() > 20 and c.n <= MAX_RAYS
        self.d = wb.ShadowDevice(c) if shadow else wb.OneRandomDevice(c)
        self.agg = self.d.agg

    def run(self):
        cap = self.wb.UNCAPPED
        if self.shadow:
            state, L, unfinished = self.d.run(cap)
            return {"state": state, "L": L, "unfinished": np.array([unfinished])}
        gh, gr, pdf, wsum, unfinished = self.d.run(cap)
        return {"sel_hits": gh, "sel_rays": gr, "pdf": pdf, "wsum": wsum, "unfinished": np.array([unfinished])}

    def check(self, res, what):
        wb = self.wb
        assert res["unfinished"][0] == 0, what
        if self.shadow:
            exp_state, exp_L = wb.shadow_expected(self.c, wb.UNCAPPED)
            assert np.array_equal(res["state"], exp_state) and res["L"].tobytes() == exp_L.tobytes(), what
        else:
            got = (res["sel_hits"], res["sel_rays"], res["pdf"], res["wsum"])
            assert wb.check_one_random(self.c, got, wb.UNCAPPED) == 0, what

    def close(self):
        self.d.close()


BVH_JOBS = {"flat_calls": lambda: BvhFlatJob(False), "queue_calls": lambda: BvhFlatJob(True),
            "walk_shadow": lambda: BvhWalkJob(True), "walk_one_random": lambda: BvhWalkJob(False)}


@gpu
@pytest.mark.parametrize("case_id,wide,narrow", BVH_CASES, ids=[c[0] for c in BVH_CASES])
def test_bvh_wide_offsets(case_id, wide, narrow):
    job = BVH_JOBS[case_id]()
    try:
        narrow_wide_narrow(job, BVH, wide, narrow, "bvh " + case_id)
        # the top table sits in lean instances only: on or off, the wide results are the same bytes from the same instances
        job.agg.set_option("offsets32", 0)
        per_table = []
        for top in (0, 1):
            job.agg.set_option("top_table", top)
            with _lib.LaunchLedger(BVH) as led:
                per_table.append(job.run())
            assert set(led.launched) == wide, f"bvh {case_id}, top_table {top}: launched {sorted(led.launched)}"
            job.check(per_table[-1], f"bvh {case_id}, wide, top_table {top}")
        assert_same_bytes(per_table[0], per_table[1], f"bvh {case_id}: top_table 0 against 1 at the wide width")
    finally:
        job.close()


# ---- the census ---------------------------------------------------------------------------------------------------------
# Instances no ledger-asserted oracle comparison reaches: the LEDGER tables of the modules ledger_cases.MODULES names
# and the tables above leave none.  (Until tests/test_alpha_candidates.py the BVH list held 37)
BVH_NOT_LEDGER_ASSERTED = set()
KD_NOT_LEDGER_ASSERTED = set()


def ledger_tables():
    """{module name: its LEDGER table}, the modules listed by name in tests/ledger_cases.py"""
    import importlib

    import ledger_cases
    return {name: importlib.import_module(name).LEDGER for name in ledger_cases.MODULES}


def test_every_ledger_key_names_a_gpu_test_of_its_module():
    import importlib
    for name, table in ledger_tables().items():
        module = importlib.import_module(name)
        assert table, name
        for key, (family, instances) in table.items():
            fn = getattr(module, key.split("[")[0], None)
            assert callable(fn) and fn.__name__.startswith("test_"), f"{name}: {key} names no test function"
            marks = {m.name for m in getattr(fn, "pytestmark", [])}
            assert "gpu" in marks, f"{name}: {key} is not marked gpu"
            assert family in (BVH, KD) and instances, f"{name}: {key}"
            assert all(len(i) == (7 if family == BVH else 5) for i in instances), f"{name}: {key}"


def test_census_of_ledger_asserted_instances(nnbvh_lib):
    covered = {BVH: set(), KD: set()}
    for _, inst in KD_CASES:
        covered[KD] |= {inst, narrow_twin(inst)}
    for _, wide, narrow in BVH_CASES:
        covered[BVH] |= wide | narrow
    for table in ledger_tables().values():
        for family, instances in table.values():
            covered[family] |= set(instances)
    all_bvh, all_kd = set(_lib.instance_launches(BVH)), set(_lib.instance_launches(KD))
    assert covered[BVH] <= all_bvh and covered[KD] <= all_kd, "a table names an instance the library does not hold"
    assert {k for k in all_kd if k[2] == 0} <= {inst for _, inst in KD_CASES}, \
        "a wide kd instance without a ledger-asserted case of its own"
    rest_bvh, rest_kd = all_bvh - covered[BVH], all_kd - covered[KD]
    print(f"ledger-asserted: {len(covered[BVH])} of 75 BVH and {len(covered[KD])} of 42 kd instances")
    print("BVH rest:", sorted(rest_bvh))
    print("kd rest:", sorted(rest_kd))
    assert len(covered[BVH]) == 75 and len(covered[KD]) == 42
    assert rest_bvh == BVH_NOT_LEDGER_ASSERTED and rest_kd == KD_NOT_LEDGER_ASSERTED
