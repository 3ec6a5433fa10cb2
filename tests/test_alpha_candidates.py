"""Host-only candidates beside alpha-tested primitives, and constant-alpha triangles inside instances: the trace_kernel
instances no test had launched, each against the oracle bit for bit and asserted with the launch ledger.

Six scenes: flat, static two-level and animated two-level, each with constant-alpha triangles alone (kinds 4 .. 7:
ALPHA = 1) and with constant-alpha patches beside them (kinds 8 .. 15, per-primitive alpha, normals, uvs: ALPHA = 2).
An object has at most 800 primitives, a case at most 20 000 rays, the oracle runs with 4 threads.

A few kind-0 triangles are declared host-only in the baked order (the tree does not change).  Three forms of every
scene go to the oracle:
  tri     the declared triangles as plain triangles: what the resolved candidate lists must give
  clear   the declared triangles as kind 4 with alpha 0: never accepted, never shrinking tMax, which is the device's
          walk (it skips them).  Its void records are exactly the rays whose alpha re-trace hit again, so
          count == -2 is PREDICTED from it, not tolerated.  The prediction is "none" in all six scenes: a line meets
          a triangle once and a bilinear patch (a quadric) twice at most, so the reference's re-traces never find a
          surface a third time on a finite ray, however twisted the patch.  Only rays with NaN components get the
          -2 mark; for those `clear` is no prediction, since a NaN ray can "hit" the declared triangle itself
  skipped the declared triangles as degenerate triangles (three times the same vertex), which the reference's test
          rejects before it looks at the ray: the device's walk for ANY ray.  On the six ray sets it predicts what
          `clear` predicts (a CPU test); test_degenerate_rays_get_count_minus_two_where_the_oracle_predicts runs the
          flat scenes on rays with NaN, infinite and zero components, where it predicts 79 and 85 voids of 4 000 rays
  opaque  `tri` with every alpha forced to 1: where its answer differs, an alpha rejection changed the result
Overflow (count == -1) is impossible by construction: (declared triangles per object) x (placements) <= 16 = capacity.

Random rays seldom meet 2 .. 16 triangles, so every case adds rays AIMED at random points of the declared triangles
and of the alpha-tested primitives, mapped through the placement at the ray's time.  The CPU tests
prove on the oracle alone that the cases bite; the GPU tests add the premises only the device's lists can show."""
import functools

import numpy as np
import pytest

import oracle_binding as ob
from ledger_cases import BVH, bvh, reaches
from nn_bvh_amd import build_tree, instancing, resolve_host_candidates, resolve_host_candidates_any, scene
from nn_bvh_amd._lib import RAY_DTYPE
from test_alpha import alpha_patch_scene, alpha_scene, patch_uvs
from test_host_candidates import (assert_resolved_equal, assert_same_but_instance, check_instances_entered, tri_callback,
                                  tri_table)

gpu = pytest.mark.gpu
CAPACITY = 16
FORMS = ("flat", "static", "animated")
INST = {"flat": 0, "static": 1, "animated": 2}
CASES = [(form, alpha) for form in FORMS for alpha in (1, 2)]
N_PLACE = 8                  # two-level: 2 declared triangles per object x 8 placements = 16
N_HOST = {"flat": 16, "static": 2, "animated": 2}

# case -> (kernel family, the instances its device calls launch), asserted by `reaches` (tests/ledger_cases.py)
LEDGER = {f"test_candidates_beside_alpha_resolve_to_the_oracle[{form}-{alpha}]":
          (BVH, bvh((0, 2), inst=INST[form], alpha=alpha, hostc=1) | bvh((0, 2), inst=INST[form], alpha=alpha))
          for form, alpha in CASES}
LEDGER.update({f"test_alpha_triangles_inside_instances[{form}]": (BVH, bvh((0, 1, 2), inst=INST[form], alpha=1))
               for form in ("static", "animated")})
LEDGER.update({f"test_degenerate_rays_get_count_minus_two_where_the_oracle_predicts[{alpha}]":
               (BVH, bvh((0, 2), alpha=alpha, hostc=1) | bvh((0, 2), alpha=alpha)) for alpha in (1, 2)})


def alpha_object(alpha_form, seed):
    """(verts, prims, normals, uvs, alpha by id): alpha_scene with about half of the alpha triangles smooth (no patch:
    the scene reports has_alpha 1), or alpha_patch_scene likewise (has_alpha 2)"""
    rng = np.random.default_rng(seed + 7)
    if alpha_form == 1:
        verts, prims, alpha, kinds = alpha_scene(seed, 800)
        normals = rng.normal(size=(len(verts), 3)).astype(np.float32)
        normals /= np.linalg.norm(normals, axis=1, keepdims=True)
        normals[rng.random(len(verts)) < 0.02] = 0
        uvs = alpha = None
    else:
        verts, prims, normals, alpha, kinds = alpha_patch_scene(seed, 350, 450)
        uvs = patch_uvs(verts)
    prims = prims.copy()
    smooth = ((kinds == 4) | (kinds == 5)) & (rng.random(len(prims)) < 0.5)
    prims["kind"] = np.where(smooth, kinds + 2, kinds)   # 4 -> 6, 5 -> 7
    assert np.array_equal(prims["id"], np.arange(len(prims))) and len(prims) <= 800
    return verts, prims, normals, uvs, alpha


def aimed_rays(rng, verts, prims, targets, n, transforms=None):
    """n rays through random points of the primitives `targets` (the triangle of their first three vertices), from
    random origins 0.2 .. 8 object units away; transforms: [n, 4, 4] render-from-object, one per ray.  The point lies
    at t = 1 / s, s in 0.7 .. 3; one ray in five ends at tMax = 1"""
    tri = verts[prims["v"][rng.choice(targets, n), :3]].astype(np.float64)
    p = (rng.dirichlet([1, 1, 1], n)[:, :, None] * tri).sum(1)
    away = rng.normal(size=(n, 3))
    o = p - away / np.linalg.norm(away, axis=1, keepdims=True) * rng.uniform(0.2, 8.0, (n, 1))
    if transforms is not None:
        m = transforms.astype(np.float64)
        p = np.einsum("nij,nj->ni", m[:, :3, :3], p) + m[:, :3, 3]
        o = np.einsum("nij,nj->ni", m[:, :3, :3], o) + m[:, :3, 3]
    rays = np.zeros(n, RAY_DTYPE)
    rays["o"], rays["d"] = o.astype(np.float32), ((p - o) * rng.uniform(0.7, 3.0, (n, 1))).astype(np.float32)
    rays["tmax"] = np.where(rng.random(n) < 0.2, np.float32(1.0), np.float32(np.inf))
    return rays


class Case:
    def __init__(self, form, alpha_form):
        self.form, self.alpha_form = form, alpha_form
        seed = 50 + 10 * FORMS.index(form) + alpha_form
        rng = np.random.default_rng(seed)
        verts, prims, normals, uvs, alpha = alpha_object(alpha_form, seed)
        self.verts, self.prims, self.normals, self.uvs = verts, prims, normals, uvs
        self.kind_by_id = prims["kind"].copy()
        self.host_ids = np.sort(rng.choice(np.nonzero(prims["kind"] == 0)[0], N_HOST[form], replace=False))
        self.anims = self.oa = self.instances = self.n_top = self.placements = None
        if form == "flat":
            tree = build_tree(prims, verts)
            self.nodes, self.baked = tree.nodes, np.ascontiguousarray(tree.ordered_prims)
        elif form == "static":
            from test_oracle_vs_reference_live import random_affine
            M, _ = random_affine(rng, N_PLACE)
            M[:, :3, 3] = rng.uniform(-15, 15, size=(N_PLACE, 3))
            Mi = np.linalg.inv(M.astype(np.float64)).astype(np.float32)
            self.placements = [(0, M[j, :3].reshape(12), Mi[j, :3].reshape(12)) for j in range(N_PLACE)]
            self.nodes, self.baked, self.instances, self.n_top = instancing.assemble_two_level(
                prims[:0], verts, [prims], self.placements)
        else:
            import test_animated as ta
            _, _, _, _, _, _, self.anims, self.oa, self.placements = ta.animated_scene(seed, N_PLACE)
            self.nodes, self.baked, self.instances, self.n_top = ta.rebuild_with_motion_bounds(
                verts, prims, self.placements, self.anims, self.oa)
        n_place = 1 if form == "flat" else len(self.placements)
        assert len(self.host_ids) * n_place <= CAPACITY  # a ray cannot reach more declared triangles than fit its list
        obj = self.baked["kind"] != 2
        assert np.array_equal(self.baked["kind"][obj], prims["kind"][self.baked["id"][obj]])
        self.a_ord = None
        if alpha is not None:
            self.a_ord = np.zeros(len(self.baked), np.float32)
            self.a_ord[obj] = alpha[self.baked["id"][obj]]
        declared = obj & np.isin(self.baked["id"], self.host_ids)
        assert declared.sum() == len(self.host_ids) and (self.baked["kind"][declared] == 0).all()
        self.host_prims = self.baked.copy()      # what the device gets
        self.host_prims["kind"][declared] = 3
        self.clear_prims = self.baked.copy()     # the device's walk, for the oracle
        self.clear_prims["kind"][declared] = 4
        self.clear_prims["v"][declared, 3] = np.float32(0.0).view(np.int32)
        self.skipped_prims = self.baked.copy()   # the same walk for ANY ray: a degenerate triangle is never hit
        self.skipped_prims["v"][declared, 1] = self.skipped_prims["v"][declared, 2] = self.baked["v"][declared, 0]
        self.opaque_prims = self.baked.copy()
        tri_alpha = obj & (self.baked["kind"] >= 4) & (self.baked["kind"] <= 7)
        self.opaque_prims["v"][tri_alpha, 3] = np.float32(1.0).view(np.int32)
        self.rays = self._rays(rng)
        assert len(self.rays) <= 20000

    def _rays(self, rng):
        verts, prims = self.verts, self.prims
        # the alpha-tested primitives of the form: the triangles, or the patches (a ray through a twisted patch is
        # the one that can cross it twice)
        tested = np.nonzero(prims["kind"] >= (4 if self.alpha_form == 1 else 8))[0]
        if self.form == "flat":
            lo, hi = verts.min(0), verts.max(0)
            return np.concatenate([scene.random_rays(5000, lo - 1, hi + 1, int(rng.integers(1 << 30))),
                                   scene.random_rays(2000, lo, hi, int(rng.integers(1 << 30)), tmax=0.6),
                                   aimed_rays(rng, verts, prims, tested, 5000),
                                   aimed_rays(rng, verts, prims, self.host_ids, 7000)])
        n_box, n_obj, n_host = 3000, 8000, 8000
        n = n_obj + n_host
        time = rng.uniform(-0.2, 1.2, n).astype(np.float32) if self.form == "animated" else np.zeros(n, np.float32)
        k = rng.integers(0, len(self.placements), n)
        if self.form == "animated":
            m = ob.anim_interpolate(self.oa[k], time)[:, :16].reshape(n, 4, 4)
        else:
            m = np.zeros((n, 4, 4), np.float32)
            m[:, :3] = self.instances["render_from_prim"][k].reshape(n, 3, 4)
        aimed = np.concatenate([aimed_rays(rng, verts, prims, tested, n_obj, m[:n_obj]),
                                aimed_rays(rng, verts, prims, self.host_ids, n_host, m[n_obj:])])
        aimed["time"] = time
        box = scene.random_rays(n_box, [-25, -25, -25], [25, 25, 25], int(rng.integers(1 << 30)))
        if self.form == "animated":
            box["time"] = rng.uniform(-0.2, 1.2, n_box).astype(np.float32)
        return np.concatenate([box, aimed])

    # ---- the oracle ----
    def _oracle(self, prims, alpha_ord, any_hit, rays=None):
        a = (self.nodes, prims, self.verts)
        rays = self.rays if rays is None else rays
        try:
            ob.set_vertex_normals(self.normals)
            ob.set_vertex_uvs(self.uvs)
            ob.set_prim_alpha(alpha_ord)
            if self.form == "flat":
                return (ob.any_hit if any_hit else ob.closest)(*a, rays, 4)
            if self.form == "static":
                return (ob.any_hit_inst if any_hit else ob.closest_inst)(*a, self.instances, rays, 4)
            ob.set_sin_mode(1)  # the device's Slerp sine (tests/test_animated.py: the path's documented exception)
            return (ob.any_hit_anim if any_hit else ob.closest_anim)(*a, self.instances, self.oa, rays, 4)
        finally:
            ob.set_sin_mode(0)
            ob.set_vertex_normals(None)
            ob.set_vertex_uvs(None)
            ob.set_prim_alpha(None)

    @functools.cached_property
    def tri_closest(self):
        return self._oracle(self.baked, self.a_ord, False)

    @functools.cached_property
    def tri_any(self):
        return self._oracle(self.baked, self.a_ord, True)

    @functools.cached_property
    def clear_void(self):
        """rays the device's closest walk voids: an alpha re-trace hit again"""
        return self._oracle(self.clear_prims, self.a_ord, False)["instance"] == -1

    @functools.cached_property
    def clear_any(self):
        """the device's any-hit walk: 1 an occluder, 2 an alpha re-trace hit again and no occluder"""
        return self._oracle(self.clear_prims, self.a_ord, True)[0]

    @functools.cached_property
    def host_void(self):
        """rays the plain call voids: a declared triangle's leaf entry reached, or an alpha re-trace hit again"""
        return self._oracle(self.host_prims, self.a_ord, False)["instance"] == -1

    @functools.cached_property
    def opaque_closest(self):
        return self._oracle(self.opaque_prims, None if self.a_ord is None else np.ones_like(self.a_ord), False)

    # ---- the host's side of the candidate calls ----
    def callback(self):
        minv = None
        if self.form == "static":
            minv = lambda idx, k: self.instances["prim_from_render"][k]  # noqa: E731
        elif self.form == "animated":
            def minv(idx, k):
                rows = self.instances["prim_from_render"][k].copy()
                a = self.anims["actually_animated"][k] != 0
                if a.any():
                    rows[a] = ob.anim_interpolate(self.oa[k[a]], self.rays["time"][idx[a]])[:, 16:28]
                return rows
        return tri_callback(self.rays, self.verts, tri_table(self.prims), minv)

    def aggregate(self, prims):
        from nn_bvh_amd import BVHAggregate
        kw = dict(normals=self.normals)
        if self.alpha_form == 2:
            kw.update(uvs=self.uvs, prim_alpha=self.a_ord)
        if self.form != "flat":
            kw.update(instances=self.instances, n_top_nodes=self.n_top, animated=self.anims)
        return BVHAggregate.from_tree(self.nodes, prims, self.verts, **kw)


@functools.lru_cache(None)
def case(form, alpha_form):
    return Case(form, alpha_form)


@functools.lru_cache(None)
def degenerate_rays(alpha_form, n=4000):
    """rays through the flat scene's box with NaN, infinite, zero and tiny components (tests/test_alpha.py); the
    oracle on the `skipped` and the `tri` form and the scene as the device gets it: (rays, skipped closest, skipped any
    hit, tri closest, tri any hit, voided by the plain call)"""
    c = case("flat", alpha_form)
    rng = np.random.default_rng(3)
    rays = scene.random_rays(n, c.verts.min(0) - 1, c.verts.max(0) + 1, 11)
    special = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, 1e-30], np.float32)
    for f in ("o", "d"):
        v = rays[f].copy()
        m = rng.random(v.shape) < 0.15
        v[m] = rng.choice(special, int(m.sum()))
        rays[f] = v
    return (rays, c._oracle(c.skipped_prims, c.a_ord, False, rays), c._oracle(c.skipped_prims, c.a_ord, True, rays)[0],
            c._oracle(c.baked, c.a_ord, False, rays), c._oracle(c.baked, c.a_ord, True, rays)[0],
            c._oracle(c.host_prims, c.a_ord, False, rays)["instance"] == -1)


def hit_of(hits, mask_by_id):
    return (hits["prim"] >= 0) & mask_by_id[np.maximum(hits["prim"], 0)]


# ---- CPU: the cases bite, on the oracle alone --------------------------------------------------------------------------
@pytest.mark.parametrize("form,alpha_form", CASES)
def test_the_oracle_alone_shows_that_the_case_bites(form, alpha_form):
    c = case(form, alpha_form)
    exp = c.tri_closest
    is_host = np.zeros(len(c.prims), bool)
    is_host[c.host_ids] = True
    inside = exp["instance"] > 0 if form != "flat" else np.ones(len(exp), bool)
    on_host = hit_of(exp, is_host)
    on_alpha = hit_of(exp, c.kind_by_id >= 4) & inside
    opaque = c.opaque_closest
    changed = (opaque["prim"] != exp["prim"]) | (opaque["instance"] != exp["instance"])
    void_c, void_a = c.clear_void.mean(), (c.clear_any == 2).mean()
    print(f"{form}-{alpha_form}: {len(c.rays)} rays, closest hit a declared triangle {on_host.sum()}, an alpha kind"
          f"{' inside an instance' if form != 'flat' else ''} {on_alpha.sum()}, changed by an alpha rejection "
          f"{changed.sum()}, predicted void share closest {void_c:.5f} any hit {void_a:.5f}")
    assert on_host.sum() >= 100 and on_alpha.sum() >= 100 and changed.sum() >= 50
    assert void_c < 0.01 and void_a < 0.01
    if alpha_form == 1:
        assert c.clear_void.sum() == 0  # a planar triangle is never met again by its re-trace
    else:
        hit_kind = c.kind_by_id[np.maximum(exp["prim"], 0)]
        assert all(((hit_kind == k) & (exp["prim"] >= 0)).sum() > 20 for k in range(8, 16))
        # every rejected patch hit is re-traced; and the sample holds the re-trace that FINDS the patch again: rejected
        # at its first crossing, accepted at its second (rare among aimed rays: a handful shows the accumulated tHit;
        # tests/test_alpha.py test_device_alpha_patches_equal_oracle holds that path at full size)
        second = (exp["prim"] >= 0) & (exp["prim"] == opaque["prim"]) & (exp["instance"] == opaque["instance"]) & \
            (hit_kind >= 8) & (exp["t"] > opaque["t"] * 1.0001)
        print(f"{form}-{alpha_form}: a patch accepted at its second crossing on {second.sum()} rays")
        assert second.sum() >= 5
    # what is compared is never void on the reference's side
    assert (exp["instance"][~c.clear_void] >= 0).all()
    if form == "animated":
        moved = c.anims["actually_animated"][np.maximum(exp["instance"] - 1, 0)] != 0
        within = (c.rays["time"] > 0) & (c.rays["time"] < 1)
        assert ((exp["instance"] > 0) & moved & within).sum() >= 100
        assert (on_host & moved & within).sum() >= 20


@pytest.mark.parametrize("form,alpha_form", CASES)
def test_both_forms_of_the_devices_walk_predict_the_same_voids(form, alpha_form):
    c = case(form, alpha_form)
    assert np.array_equal(c._oracle(c.skipped_prims, c.a_ord, False)["instance"] == -1, c.clear_void)
    assert np.array_equal(c._oracle(c.skipped_prims, c.a_ord, True)[0], c.clear_any)


@pytest.mark.parametrize("alpha_form", [1, 2])
def test_degenerate_rays_are_voided_by_an_alpha_retrace_often_enough(alpha_form):
    rays, skipped, skipped_any, tri, _, host_void = degenerate_rays(alpha_form)
    void = skipped["instance"] == -1
    assert (void <= host_void).all() and (host_void & ~void).sum() >= 150  # rays that keep a list
    print(f"flat-{alpha_form}, degenerate rays: {void.sum()} of {len(rays)} voided by an alpha re-trace, "
          f"{(skipped_any == 2).sum()} in the any-hit walk")
    assert 50 <= void.sum() < 0.05 * len(rays)
    assert ((tri["instance"] == -1) <= void).all()  # a declared triangle as a triangle only ends walks sooner


def test_the_object_without_patches_holds_every_alpha_triangle_kind():
    for form in FORMS:
        c = case(form, 1)
        assert set(np.unique(c.kind_by_id)) == {0, 4, 5, 6, 7}
        exp = c.tri_closest
        hit_kind = c.kind_by_id[np.maximum(exp["prim"], 0)]
        assert all(((hit_kind == k) & (exp["prim"] >= 0)).sum() > 50 for k in (4, 5, 6, 7))


# ---- GPU ----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("form", ["static", "animated"])
def test_alpha_triangles_inside_instances(form):
    """constant-alpha triangles (kinds 4 .. 7, no patch: has_alpha 1) inside TransformedPrimitive / AnimatedPrimitive
    instances: the alpha hash and the re-trace on the instance-space ray, after the animated ENTER step"""
    c = case(form, 1)
    with reaches(LEDGER, f"test_alpha_triangles_inside_instances[{form}]"):
        agg = c.aggregate(c.baked)
        got = agg.Intersect(c.rays)
        occ, vis, tst = agg.IntersectP(c.rays, counts=True)
        occ2 = agg.IntersectP(c.rays)
        agg.close()
    exp, (eo, ev, et) = c.tri_closest, c.tri_any
    assert (exp["instance"] == -1).sum() == 0
    assert got.tobytes() == exp.tobytes()
    assert np.array_equal(occ, eo) and np.array_equal(vis, ev) and np.array_equal(tst, et)
    assert np.array_equal(occ2, eo)


@gpu
@pytest.mark.parametrize("form,alpha_form", CASES)
def test_candidates_beside_alpha_resolve_to_the_oracle(form, alpha_form):
    c = case(form, alpha_form)
    rays = c.rays
    with reaches(LEDGER, f"test_candidates_beside_alpha_resolve_to_the_oracle[{form}-{alpha_form}]"):
        agg = c.aggregate(c.host_prims)
        hits, cands = agg.intersect_with_host_candidates(rays, capacity=CAPACITY)
        occ, acands = agg.intersect_p_with_host_candidates(rays, capacity=CAPACITY)
        plain = agg.Intersect(rays)
        plain_occ = agg.IntersectP(rays)
        agg.close()
    cnt, acnt = cands["count"], acands["count"]
    listed = np.arange(CAPACITY)[None, :] < np.maximum(cnt, 0)[:, None]
    print(f"{form}-{alpha_form}: {len(rays)} rays, count > 0 on {(cnt > 0).sum()}, count == -2 on {(cnt == -2).sum()} "
          f"(any hit: {(acnt > 0).sum()}, {(acnt == -2).sum()}), {listed.sum()} candidates, longest list {cnt.max()}")
    # -- the lists: no overflow, the voids are the predicted ones, only declared triangles are named
    assert (cnt == -1).sum() == 0 and (acnt == -1).sum() == 0
    assert np.array_equal(cnt == -2, c.clear_void)
    assert np.array_equal(cnt != 0, c.host_void)  # a list exactly where the reference's walk reaches a declared triangle
    assert (cnt > 0).sum() >= 200
    assert np.isin(cands["prim"][listed], c.host_ids).all()
    if form != "flat":
        assert (cands["instance"][listed] > 0).all()
        check_instances_entered(cands, c.placements, [c.prims], top_level=False)
    # -- the plain calls: records equal in every field but instance, void exactly where count != 0
    assert_same_but_instance(hits, plain)
    assert np.array_equal(plain["instance"] == -1, cnt != 0)
    assert np.array_equal(hits["instance"] == -1, cnt < 0)
    # -- closest: every ray but the predicted voids, resolved, is the oracle's record on the all-triangle scene
    cb = c.callback()
    try:
        ob.set_sin_mode(1 if form == "animated" else 0)
        res = resolve_host_candidates(rays, hits, cands, cb, kind=c.kind_by_id)
        two = np.nonzero((cands["before"] > 0) & (hits["prim"] >= 0) & (cnt > 0))[0]
        first_taken = cb(two, cands["prim"][two, 0], cands["instance"][two, 0], rays["tmax"][two])[0]
        got_any = resolve_host_candidates_any(rays, occ, acands, cb)
    finally:
        ob.set_sin_mode(0)
    ok = ~c.clear_void
    assert_resolved_equal(res[ok], c.tri_closest[ok], f"{form}-{alpha_form} closest")
    assert first_taken.sum() >= 5  # merge step 3: a device hit that comes after a candidate the ray hits
    # -- any hit: the flags are the plain call's and the device walk's; the voids are the predicted ones
    assert np.array_equal(occ, plain_occ) and (acands["before"] == 0).all()
    assert np.array_equal(occ == 2, (acnt != 0) & (occ != 1))
    assert np.array_equal(occ == 1, c.clear_any == 1)
    assert np.array_equal(acnt[occ != 1] == -2, c.clear_any[occ != 1] == 2)
    assert np.array_equal(got_any == 2, c.clear_any == 2)
    settled = got_any != 2
    assert np.array_equal(got_any[settled], c.tri_any[0][settled])
    assert ((occ == 2) & (got_any == 1)).sum() >= 20 and ((occ == 2) & (got_any == 0)).sum() >= 20


def same_records(a, b):
    """records equal bit for bit, a NaN equal to a NaN (x86 and gfx950 differ in the sign of the default NaN:
    tests/test_alpha.py test_device_alpha_patches_equal_oracle)"""
    for f in ("prim", "instance", "nodes_visited", "prim_tests"):
        if not np.array_equal(a[f], b[f]):
            return False
    return all((((a[f].view(np.uint32) == b[f].view(np.uint32)) | (np.isnan(a[f]) & np.isnan(b[f]))).all())
               for f in ("t", "b0", "b1", "b2"))


@gpu
@pytest.mark.parametrize("alpha_form", [1, 2])
def test_degenerate_rays_get_count_minus_two_where_the_oracle_predicts(alpha_form):
    """cold[kColdHost] holds the candidate count, the -1 overflow and the -2 alpha void: on rays with NaN, infinite and
    zero components the re-trace does hit again, beside declared triangles that the same rays reach.  count == -2
    exactly where the oracle on the `skipped` form voids the ray; the lists of such rays are not resolved (the merge
    rule compares on t, and these rays carry NaN t), a ray without a list has the oracle's record"""
    c = case("flat", alpha_form)
    rays, skipped, skipped_any, tri, tri_any, host_void = degenerate_rays(alpha_form)
    with reaches(LEDGER, f"test_degenerate_rays_get_count_minus_two_where_the_oracle_predicts[{alpha_form}]"):
        agg = c.aggregate(c.host_prims)
        hits, cands = agg.intersect_with_host_candidates(rays, capacity=CAPACITY)
        occ, acands = agg.intersect_p_with_host_candidates(rays, capacity=CAPACITY)
        plain = agg.Intersect(rays)
        plain_occ = agg.IntersectP(rays)
        agg.close()
    cnt, acnt = cands["count"], acands["count"]
    void = skipped["instance"] == -1
    print(f"flat-{alpha_form}, degenerate rays: count == -2 on {(cnt == -2).sum()} (predicted {void.sum()}), count > 0 on "
          f"{(cnt > 0).sum()}, any hit: count == -2 on {(acnt == -2).sum()}")
    assert (cnt == -1).sum() == 0 and (acnt == -1).sum() == 0
    assert np.array_equal(cnt == -2, void)
    assert np.array_equal(cnt > 0, host_void & ~void)  # at least 150 rays (the CPU test): the lists are not lost
    listed = np.arange(CAPACITY)[None, :] < np.maximum(cnt, 0)[:, None]
    assert np.isin(cands["prim"][listed], c.host_ids).all()
    assert_same_but_instance(hits, plain)
    assert np.array_equal(plain["instance"] == -1, cnt != 0)
    assert np.array_equal(hits["instance"] == -1, cnt < 0)
    alone = cnt == 0   # no declared triangle reached: the walk is the all-triangle scene's
    assert alone.sum() >= 1000 and same_records(hits[alone], tri[alone])
    assert np.array_equal(occ, plain_occ) and (acands["before"] == 0).all()
    assert np.array_equal(occ == 2, (acnt != 0) & (occ != 1))
    assert np.array_equal(occ == 1, skipped_any == 1)
    assert np.array_equal(acnt[occ != 1] == -2, skipped_any[occ != 1] == 2)
    assert np.array_equal(occ[acnt == 0], tri_any[acnt == 0])
