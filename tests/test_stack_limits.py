"""Every traversal kernel family at the 64-entry stack limit and through its spill.

Each ray keeps its pending nodes in a per-lane LDS ring window (BVH kernels: 4, 8 or 16 entries, bvh_trace.hip; kd
kernels: kKdWLean = 4 or kKdW = 8, kd_trace.h); the oldest entry spills to an HBM array whose size is computed
exactly (workspace_for in bvh_capi.cpp, kd_workspace_for in capi_kd.cpp).  The scenes here (scenes_small: chain_tree
tube form, two_level_chain, kd_chain) make every "deep" ray hold 64 pending entries (63 = a + b in the two-level
scene, see below), which the CPU tests in this file PROVE with the oracle's pending-depth output and a float64
margin check — never with the device's own counters.  Every GPU case compares bit for bit with the oracle and
asserts that at least half of its deep rays exceeded the instance's window by 2 or more.

Which template instance a case reaches (trace_kernel<MODE, W, INST, PATCH, ALPHA, SOA, HOSTC>; pick_trace_instance of
trace_instance.h picks it from the scene's content, the "stack_window" option and the call).  The table LEDGER below
states the same per case as data, and every GPU case asserts it with the launch ledger (nnbvh_instance_launches): its
device calls launch exactly the instances listed for it, each at least once, and no other instance of the family:

  test_bvh_single_level[lean-8]      triangles only, window 8: the lean instances <0,8,0,0>, <1,8,0,0>, <2,8,0,0>
                                     for Intersect / IntersectP(counts) / IntersectP and <3,8,0,0> for the
                                     one-launch trace_batches_device (closest + any)
  test_bvh_single_level[lean-4|16]   triangles only, window 4 / 16: no lean instance exists at these windows, the
                                     general <M,4,0,1> / <M,16,0,1> run; mode 3 exists at window 8 only, so
                                     trace_batches_device runs its batches as modes 0 and 2 on its side streams
                                     (each stream has its own spill array)
  test_bvh_single_level[general-W]   patch leaves force PATCH = 1: <M,W,0,1> for W = 4, 8, 16; <3,8,0,1> at W = 8
  test_bvh_alpha[tri]                kinds 4 .. 7: <M,8,0,1,1>, M = 0, 1, 2 (alpha scenes never run mode 3)
  test_bvh_alpha[patch]              kinds 8 .. 15: <M,8,0,1,2>, M = 0, 1, 2
  test_bvh_wavefront_soa             triangles only, WavefrontAggregate.IntersectClosest / IntersectShadow on RayQueues
                                     whose device-side size is below the capacity: the lean SOA instances
                                     <0,8,0,0,0,1> / <2,8,0,0,0,1>, and <3,8,0,0,0,1> for IntersectClosestAndShadow
  test_bvh_host_only_chain           kind-3 leaves at several levels: the general <M,8,0,1> with hasHostPrims (plain
                                     calls: void rays); the HOSTC twins <0,8,0,1,0,0,1> / <2,8,0,1,0,0,1> through the
                                     single-batch *_candidates calls; <3,8,0,1,0,0,1> through
                                     trace_batches_candidates_device (fused_batches 1; 0: the twins on side streams);
                                     the wavefront calls IntersectClosestItemsWithCandidates and
                                     IntersectShadowWithCandidates, which gather their queue into records and run
                                     the twins of modes 0 / 2 with a device-side size.  Every list is resolved with
                                     the host's triangle test and compared with the oracle on the all-triangle scene
  test_two_level_chain               INST = 1: <M,8,1,1>, M = 0, 1, 2, and <3,8,1,1> in one launch
  test_animated_two_level_chain      INST = 2: <M,8,2,1>, M = 0, 1, 2, and <3,8,2,1> in one launch, ray times inside,
                                     at and outside the time range
  test_kd_chain[lean|patch|attr]     kd_trace_kernel<MODE, PATCH, W, O32, ATTR>: lean <M,0,4,1>, patch <M,1,8,1>,
                                     attr <M,1,8,1,1> for M = 0 (Intersect), 1 (IntersectP, both forms) and the
                                     batch mode 2 through nnbvh_kd_trace_batches_device (O32 = 1: these scenes fit
                                     32-bit offsets); the queue calls IntersectClosest / IntersectShadow /
                                     IntersectClosestAndShadow with read_soa 1 (lean: batch mode 3, the kernel reads
                                     the SOA slices; patch / attr: always gathered) and read_soa 0 (gathered into
                                     records: batch mode 2), pair_one_launch 1 and 0
  test_kd_chain[*-wide]              the same three scenes with the option "offsets32" 0: the O32 = 0 twins of those
                                     instances (64-bit addressing; tests/test_wide_offsets.py), through the same spill
  test_full_grid_*                   lean <1,8,0,0> with blocks_per_cu 8 and kd lean <0,0,4,1>: one deep ray per
                                     lane of the largest grid the library launches, which addresses the END of the
                                     spill arrays

Windows other than 8 can be selected for the single-level general instances only ("stack_window"); every other BVH
instance is compiled at 8, and the kd windows are fixed per form.

The two-level sum: bvh_scene_create bounds (outer depth) + (child depth + 1) by 64.  The reference's walk holds at most
(outer depth) + (child depth) entries at once, one fewer than that bound counts, so the a + b + 1 == 64 scene reaches 63
pending entries (a = 31 outer ones at the deepest instance's entry, b = 32 more inside it), and a + b + 1 == 65 is
refused.

The animated scene writes its own AnimatedTransforms (a turn about the chain axis and a slide along it): the committed
golden ones are arbitrary affine maps, which take a ray off the child's axis, and then no depth could be proved.
"""
import numpy as np
import pytest

import oracle_binding as ob
import scenes_small as ss
from ledger_cases import assert_reached, ledger_start, reaches
from nn_bvh_amd import HIT_DTYPE, BVHAggregate, NNBVHError, _lib, scene
from nn_bvh_amd.kdtree import KdTreeAggregate

gpu = pytest.mark.gpu
BVH, KD = _lib.FAMILY_BVH, _lib.FAMILY_KD


def _bvh(modes, window=8, inst=0, patch=1, alpha=0, soa=0, hostc=0):
    return {(m, window, inst, patch, alpha, soa, hostc) for m in modes}


def _kd(modes, patch, o32, attr=0):
    return {(m, patch, o32, attr, 0) for m in modes}


# case -> (kernel family, the instances its device calls launch): BVH (mode, window, inst, patch, alpha, soa, hostc), kd
# (mode, patch, o32, attr, hostc).  Asserted by `reaches` (tests/ledger_cases.py); tests/test_wide_offsets.py takes
# its census from it.
LEDGER = {
    "test_bvh_single_level[lean-8]": (BVH, _bvh((0, 1, 2, 3), patch=0)),
    "test_bvh_single_level[lean-4]": (BVH, _bvh((0, 1, 2), window=4)),
    "test_bvh_single_level[lean-16]": (BVH, _bvh((0, 1, 2), window=16)),
    "test_bvh_single_level[general-4]": (BVH, _bvh((0, 1, 2), window=4)),
    "test_bvh_single_level[general-8]": (BVH, _bvh((0, 1, 2, 3))),
    "test_bvh_single_level[general-16]": (BVH, _bvh((0, 1, 2), window=16)),
    "test_bvh_wavefront_soa": (BVH, _bvh((0, 2, 3), patch=0, soa=1)),
    "test_bvh_alpha[tri]": (BVH, _bvh((0, 1, 2), alpha=1)),
    "test_bvh_alpha[patch]": (BVH, _bvh((0, 1, 2), alpha=2)),
    "test_bvh_host_only_chain": (BVH, _bvh((0, 1, 2, 3)) | _bvh((0, 2, 3), hostc=1)),
    "test_two_level_chain": (BVH, _bvh((0, 1, 2, 3), inst=1)),
    "test_animated_two_level_chain": (BVH, _bvh((0, 1, 2, 3), inst=2)),
    "test_kd_chain[lean]": (KD, _kd((0, 1, 2, 3), 0, 1)),
    "test_kd_chain[patch]": (KD, _kd((0, 1, 2), 1, 1)),
    "test_kd_chain[attr]": (KD, _kd((0, 1, 2), 1, 1, attr=1)),
    "test_kd_chain[lean-wide]": (KD, _kd((0, 1, 2, 3), 0, 0)),
    "test_kd_chain[patch-wide]": (KD, _kd((0, 1, 2), 1, 0)),
    "test_kd_chain[attr-wide]": (KD, _kd((0, 1, 2), 1, 0, attr=1)),
    "test_full_grid_bvh_any_hit_with_counts": (BVH, _bvh((1,), patch=0)),
    "test_full_grid_kd_closest": (KD, _kd((0,), 0, 1)),
    "test_deep_results_independent_of_tuning_and_order[two_level]": (BVH, _bvh((0, 1, 2), inst=1)),
    "test_deep_results_independent_of_tuning_and_order[alpha]": (BVH, _bvh((0, 1, 2), alpha=2)),
}


N_DEEP, N_RANDOM = 1500, 500
# share of chain_rays / kd_chain_rays that are "deep": all BVH chain rays (every box is crossed whatever tMax is);
# the kd rays with an infinite tMax (a finite one ends the interval before the far split planes)
KD_TMAX_SHARE = 0.25


class attributes:
    """The oracle's per-vertex / per-primitive attribute arrays, for the duration of a block."""

    def __init__(self, ch):
        self.ch = ch

    def __enter__(self):
        ob.set_vertex_normals(self.ch.normals)
        ob.set_vertex_uvs(self.ch.uvs)
        ob.set_prim_alpha(self.ch.prim_alpha)

    def __exit__(self, *exc):
        ob.set_vertex_normals(None)
        ob.set_vertex_uvs(None)
        ob.set_prim_alpha(None)
        return False


def bvh_ray_set(lo, hi, seed, n_deep=N_DEEP, n_random=N_RANDOM):
    """n_deep chain rays (the deep set: the first n_deep) + random rays through the scene's box."""
    rays = np.concatenate([ss.chain_rays(float(hi[:, 0].max()), n_deep, seed),
                           scene.random_rays(n_random, lo.min(0) - 1, hi.max(0) + 1, seed + 1)])
    return rays, np.arange(len(rays)) < n_deep


def oracle_single(ch, rays):
    """closest records, any-hit triple and the pending depths of both walks"""
    with attributes(ch):
        with ob.pending_depth(len(rays)) as dc:
            exp = ob.closest(ch.nodes, ch.prims, ch.verts, rays)
        with ob.pending_depth(len(rays)) as da:
            eany = ob.any_hit(ch.nodes, ch.prims, ch.verts, rays)
    return exp, eany, dc.depth[:, 0], da.depth[:, 0]


def assert_exceeds_window(depth, deep, window, what):
    share = (depth[deep] >= window + 2).mean()
    assert share >= 0.5, f"{what}: only {share:.2f} of the deep rays exceed the {window}-entry window by 2"


def upload(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def one_launch(agg, rays_closest, rays_any):
    """trace_batches_device with a closest and an any batch -> (records, flags)"""
    import torch
    dc, da = upload(rays_closest), upload(rays_any)
    oc = torch.full((len(rays_closest) * 32,), 0x5A, dtype=torch.uint8, device="cuda")
    oa = torch.full((len(rays_any),), 0x5A, dtype=torch.uint8, device="cuda")
    agg.trace_batches_device([("closest", dc.data_ptr(), len(rays_closest), oc.data_ptr()),
                              ("any", da.data_ptr(), len(rays_any), oa.data_ptr())],
                             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return oc.cpu().numpy().view(HIT_DTYPE), oa.cpu().numpy()


def check_all_modes(agg, rays, exp, eany, what, batches=True):
    assert agg.Intersect(rays).tobytes() == exp.tobytes(), f"{what}: closest-hit records"
    occ, vis, tst = agg.IntersectP(rays, counts=True)
    assert np.array_equal(occ, eany[0]) and np.array_equal(vis, eany[1]) and np.array_equal(tst, eany[2]), \
        f"{what}: any hit with counts"
    assert np.array_equal(agg.IntersectP(rays), eany[0]), f"{what}: occlusion only"
    if batches:
        hits, flags = one_launch(agg, rays, rays[::-1].copy())
        assert hits.tobytes() == exp.tobytes(), f"{what}: closest batch of the one-launch form"
        assert np.array_equal(flags, eany[0][::-1]), f"{what}: any batch of the one-launch form"


def check_queue_calls(agg, walk, rays, deep, window, what):
    """IntersectClosest, IntersectShadow and IntersectClosestAndShadow on RayQueues whose device-side size is below the
    capacity.  walk(kind, rays) -> (the oracle's result, pending depths).  A closest queue carries no tMax (Infinity)."""
    import torch
    from nn_bvh_amd.wavefront import RayQueue, WavefrontAggregate
    from test_wavefront import shadow_inputs
    cap = len(rays)
    n = cap - 137
    dev = torch.device("cuda", 0)
    q = rays[:n].copy()
    q["tmax"] = np.inf
    exp, dc = walk("closest", q)
    (eocc, _, _), da = walk("any", rays[:n])
    assert_exceeds_window(dc, deep[:n], window, what + " closest queue")
    assert_exceeds_window(da, deep[:n], window, what + " shadow queue")
    Ld, r_u, r_l, px, L = shadow_inputs(cap, cap + 500, 7)
    exp_l = ob.record_shadow(eocc, Ld[:n], r_u[:n], r_l[:n], px[:n], L)
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    wf = WavefrontAggregate(agg)
    rq, sq = RayQueue.from_records(rays, dev), RayQueue.from_records(rays, dev, shadow=True)
    rq.size.fill_(n)
    sq.size.fill_(n)

    def outputs():
        return (torch.full((cap, 32), 0xAB, dtype=torch.uint8, device=dev), t(L),
                torch.full((cap,), 9, dtype=torch.uint8, device=dev))

    def check(hits_t, l_t, occ_t, call):
        torch.cuda.synchronize()
        hits = hits_t.cpu().numpy()
        assert hits[:n].tobytes() == exp.tobytes(), f"{what} {call}: hit records"
        assert (hits[n:] == 0xAB).all() and (occ_t.cpu().numpy()[n:] == 9).all(), f"{what} {call}: wrote beyond the size"
        assert np.array_equal(occ_t.cpu().numpy()[:n], eocc), f"{what} {call}: occlusion flags"
        assert np.array_equal(l_t.cpu().numpy().view(np.uint32), exp_l.view(np.uint32)), f"{what} {call}: radiance"

    hits_t, l_t, occ_t = outputs()
    wf.IntersectClosest(cap, rq, hits=hits_t)
    wf.IntersectShadow(cap, sq, t(Ld), t(r_u), t(r_l), t(px), l_t, occluded=occ_t)
    check(hits_t, l_t, occ_t, "single calls")
    hits_t, l_t, occ_t = outputs()
    wf.IntersectClosestAndShadow(cap, rq, cap, sq, t(Ld), t(r_u), t(r_l), t(px), l_t, hits=hits_t, occluded=occ_t)
    check(hits_t, l_t, occ_t, "pair call")


# ---- CPU: the builders' claims -----------------------------------------------------------------------------------
@pytest.mark.parametrize("leaves", sorted(ss.LEAF_MIXES))
def test_cpu_tube_chain_keeps_64_entries_pending(leaves):
    """Every chain ray (share 1.0 of the deep set) reaches exactly 64 pending entries in the reference's closest and
    any walks, and its LINE stays 0.05 or more inside every leaf box's cross-section: a far child is then pushed by
    the device (whose modes 0 / 2 / 3 skip a box the ray misses whatever tMax is) exactly where the reference does."""
    ch = ss.chain_tree(64, np.random.default_rng(11), tube=True, leaves=leaves, extras=True)
    rays, deep = bvh_ray_set(ch.leaf_lo, ch.leaf_hi, 12)
    exp, eany, dc, da = oracle_single(ch, rays)
    assert deep.mean() == N_DEEP / (N_DEEP + N_RANDOM)
    assert (dc[deep] == 64).all() and (da[deep] == 64).all() and dc.max() == 64
    assert ss.line_box_margin(rays[deep], ch.leaf_lo, ch.leaf_hi).min() >= 0.05
    # the rays meet some primitives and miss others: hits, misses and (any hit) walks of many lengths
    assert 0.3 < (exp["prim"] >= 0)[deep].mean() and (eany[0][deep] != 1).mean() > 0.02
    assert len(np.unique(eany[1][deep])) > 3  # ... at least: an early hit, later ones, none
    if leaves.startswith("host"):
        assert (exp["instance"][deep] == -1).sum() > 50


def test_cpu_legacy_chain_is_unchanged_by_the_move():
    """chain_tree's default form (what test_gpu_parity's depth tests build): same arrays as ever for a seed."""
    verts, prims, nodes = ss.chain_tree(64, np.random.default_rng(3))
    assert len(nodes) == 129 and len(prims) == 65 and verts.shape == (195, 3)
    assert nodes["nprims"][0] == 0 and nodes["offset"][0] == 2 and nodes["nprims"][-1] == 1
    rng = np.random.default_rng(3)
    x = np.arange(65, dtype=np.float32) * 2.0
    c = np.stack([x, np.zeros_like(x), np.zeros_like(x)], 1)[:, None, :]
    assert np.array_equal(verts, (c + rng.uniform(-0.7, 0.7, size=(65, 3, 3))).reshape(-1, 3).astype(np.float32))


@pytest.mark.parametrize("a,b", [(31, 32), (32, 32)])
def test_cpu_two_level_chain_pending_depth_is_the_sum(a, b):
    """Outer entries pending at the deepest instance's entry: a; the child walk's own maximum: b; at once: a + b
    (the library bounds a + b + 1).  Every chain ray is deep (share 1.0); its line crosses every outer leaf box and, in
    each instance's space, every child leaf box by 0.05 or more."""
    t = ss.two_level_chain(a, b, 5)
    rays, deep = bvh_ray_set(t.outer_lo, t.outer_hi, 6)
    with ob.pending_depth(len(rays)) as dc:
        exp = ob.closest_inst(t.nodes, t.prims, t.verts, t.instances, rays)
    with ob.pending_depth(len(rays)) as da:
        ob.any_hit_inst(t.nodes, t.prims, t.verts, t.instances, rays)
    for d in (dc.depth, da.depth):
        assert (d[deep, 0] == a + b).all() and d[:, 0].max() == a + b
        assert (d[deep, 1] == a).all() and (d[deep, 2] == b).all()
    assert ss.line_box_margin(rays[deep], t.outer_lo, t.outer_hi).min() >= 0.05
    for inst in t.instances:
        assert not np.allclose(inst["prim_from_render"][[5, 6]], 0)  # a real rotation: the transformed ray is used
        assert ss.line_box_margin(rays[deep], t.child_lo, t.child_hi, inst["prim_from_render"]).min() >= 0.05
    inside = np.bincount(exp["instance"][deep] + 1, minlength=len(t.instances) + 2)
    assert (inside[2:] > 0).all(), "hits inside every instance"


ANIM_TIMES = np.array([-0.3, 0.0, 0.2, 0.5, 0.8, 1.0, 1.4], np.float32)  # outside, at and inside the range [0, 1]


def anim_ray_set(t, seed):
    rays, deep = bvh_ray_set(t.outer_lo, t.outer_hi, seed)
    rng = np.random.default_rng(seed + 7)
    rays["time"] = np.where(rng.random(len(rays)) < 0.5, rng.choice(ANIM_TIMES, len(rays)),
                            rng.uniform(-0.2, 1.2, len(rays))).astype(np.float32)
    return rays, deep


def oracle_anim(t, oa, rays, sin_mode):
    try:
        ob.set_sin_mode(sin_mode)
        with ob.pending_depth(len(rays)) as dc:
            exp = ob.closest_anim(t.nodes, t.prims, t.verts, t.instances, oa, rays)
        with ob.pending_depth(len(rays)) as da:
            eany = ob.any_hit_anim(t.nodes, t.prims, t.verts, t.instances, oa, rays)
    finally:
        ob.set_sin_mode(0)
    return exp, eany, dc.depth, da.depth


@pytest.mark.parametrize("a,b", [(31, 32), (32, 32)])
def test_cpu_animated_two_level_chain_pending_depth_is_the_sum(a, b):
    """The animated form of the two-level chain: at every ray time (inside, at and outside the time range) every chain
    ray (share 1.0) holds a outer entries at the deepest instance's entry and b more inside: a + b at once, with the
    reference's sine and with the device's.  In float64: the line crosses every outer box (the motion bounds) and, under
    the interpolated transform of each instance at a spread of times, every child leaf box by 0.05 or more."""
    t, anims, oa = ss.animated_two_level_chain(a, b, 5)
    rays, deep = anim_ray_set(t, 6)
    assert oa["actually_animated"][-1] == 1 and 0 < oa["actually_animated"].sum() < len(oa)
    inside = (rays["time"] > 0) & (rays["time"] < 1)
    assert (inside & deep).sum() > 400 and (~inside & deep).sum() > 400 and (rays["time"][deep] == 1).sum() > 50
    for sin_mode in (0, 1):
        exp, _, dc, da = oracle_anim(t, oa, rays, sin_mode)
        for d in (dc, da):
            assert (d[deep, 0] == a + b).all() and d[:, 0].max() == a + b
            assert (d[deep, 1] == a).all() and (d[deep, 2] == b).all()
    assert ss.line_box_margin(rays[deep], t.outer_lo, t.outer_hi).min() >= 0.05
    for time in np.linspace(-0.5, 1.5, 21, dtype=np.float32):
        m = ob.anim_interpolate(oa, np.full(len(oa), time, np.float32))
        for j in range(len(oa)):
            assert ss.line_box_margin(rays[deep], t.child_lo, t.child_hi, m[j, 16:28]).min() >= 0.05
    still = ob.closest_inst(t.nodes, t.prims, t.verts, t.instances, rays)
    moved = (exp["prim"] != still["prim"]) | (exp["t"] != still["t"])
    assert (moved & deep & inside).sum() > 100, "the interpolated transform, not the start one, decides hits"
    inside_inst = np.bincount(exp["instance"][deep] + 1, minlength=len(oa) + 2)
    assert (inside_inst[2:] > 0).all(), "hits inside every instance"


@pytest.mark.parametrize("form", ["lean", "patch", "attr"])
def test_cpu_kd_chain_keeps_64_entries_pending(form):
    """Rays with an infinite tMax (the deep set: share 1 - KD_TMAX_SHARE of the chain rays, all of which are deep)
    push one entry per level: todoPos reaches exactly 64.  In float64: every split plane is crossed strictly inside
    the ray's interval in the tree's bounds, by a margin of 0.05 in t."""
    k = ss.kd_chain(64, 7, form)
    rays = ss.kd_chain_rays(2000, 8, KD_TMAX_SHARE)
    deep = np.isinf(rays["tmax"])
    assert abs(deep.mean() - (1 - KD_TMAX_SHARE)) < 0.05
    with attributes(k):
        with ob.pending_depth(len(rays)) as dc:
            exp = ob.kd_closest(k.nodes, k.prim_indices, k.prims, k.verts, k.bounds, rays)
        with ob.pending_depth(len(rays)) as da:
            ob.kd_any_hit(k.nodes, k.prim_indices, k.prims, k.verts, k.bounds, rays)
    assert (dc.depth[deep, 0] == 64).all() and (da.depth[deep, 0] == 64).all() and dc.depth[:, 0].max() == 64
    assert (dc.depth[~deep, 0] < 64).all()
    o, d = rays["o"][deep].astype(np.float64), rays["d"][deep].astype(np.float64)
    t_split = (k.splits[None, :].astype(np.float64) - o[:, :1]) / d[:, :1]
    t_in = (float(k.bounds[0]) - o[:, 0]) / d[:, 0]
    t_out = (float(k.bounds[3]) - o[:, 0]) / d[:, 0]
    assert (t_split.min(1) - t_in >= 0.05).all() and (t_out - t_split.max(1) >= 0.05).all() and (t_in > 0).all()
    for ax in (1, 2):  # ... and the rays leave the bounds through the far x face, not sideways
        p = o[:, ax:ax + 1] + np.stack([t_in, t_out], 1) * d[:, ax:ax + 1]
        assert (np.abs(p) <= 0.95).all()
    assert 0.3 < (exp["prim"] >= 0)[deep].mean() and len(np.unique(exp["nodes_visited"][deep])) > 3


def test_cpu_pending_depth_output_changes_no_result():
    ch = ss.chain_tree(40, np.random.default_rng(1), tube=True, leaves="patch", extras=True)
    rays, _ = bvh_ray_set(ch.leaf_lo, ch.leaf_hi, 2, 300, 300)
    plain = ob.closest(ch.nodes, ch.prims, ch.verts, rays)
    with ob.pending_depth(len(rays)) as d1:
        with_out = ob.closest(ch.nodes, ch.prims, ch.verts, rays, nthreads=4)
    assert plain.tobytes() == with_out.tobytes() and d1.depth[:, 0].max() == 40
    with ob.pending_depth(len(rays)) as d2:
        ob.closest(ch.nodes, ch.prims, ch.verts, rays)
    assert np.array_equal(d1.depth, d2.depth), "threaded and serial runs record the same depths"


# ---- GPU: single-level BVH ---------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("leaves,window", [("tri", 8), ("tri", 4), ("tri", 16), ("patch", 4), ("patch", 8), ("patch", 16)],
                         ids=["lean-8", "lean-4", "lean-16", "general-4", "general-8", "general-16"])
def test_bvh_single_level(leaves, window):
    ch = ss.chain_tree(64, np.random.default_rng(21), tube=True, leaves=leaves, extras=True)
    rays, deep = bvh_ray_set(ch.leaf_lo, ch.leaf_hi, 22)
    exp, eany, dc, da = oracle_single(ch, rays)
    assert_exceeds_window(dc, deep, window, "closest")
    assert_exceeds_window(da, deep, window, "any")
    agg = BVHAggregate.from_tree(ch.nodes, ch.prims, ch.verts)
    assert agg.info["depth"] == 64
    agg.set_option("stack_window", window)
    with reaches(LEDGER, f"test_bvh_single_level[{'lean' if leaves == 'tri' else 'general'}-{window}]"):
        check_all_modes(agg, rays, exp, eany, f"{leaves} window {window}")
    agg.close()


@gpu
def test_bvh_wavefront_soa():
    """The lean SOA instances: the kernel fetches its rays from the queue's slices (an LDS layout of their own around
    the same push / spill / pop code).  Device-side queue size 137 below the capacity."""
    ch = ss.chain_tree(64, np.random.default_rng(21), tube=True, leaves="tri", extras=True)
    rays, deep = bvh_ray_set(ch.leaf_lo, ch.leaf_hi, 23)

    def walk(kind, r):
        with ob.pending_depth(len(r)) as d:
            res = (ob.closest if kind == "closest" else ob.any_hit)(ch.nodes, ch.prims, ch.verts, r)
        return res, d.depth[:, 0]
    agg = BVHAggregate.from_tree(ch.nodes, ch.prims, ch.verts)
    with reaches(LEDGER, "test_bvh_wavefront_soa"):
        check_queue_calls(agg, walk, rays, deep, 8, "lean SOA")
    agg.close()


@gpu
@pytest.mark.parametrize("leaves", ["alpha_tri", "alpha_patch"], ids=["tri", "patch"])
def test_bvh_alpha(leaves):
    """Alpha values 0, 1 and between: hits are rejected (and re-traced) while entries are spilled.  The count of
    rejected hits is by proxy: a deep ray whose record or test count differs from the walk of the same scene without
    alpha had a hit rejected somewhere.  That it happened WHILE entries were spilled follows from the scene, not from
    the count: the walk reaches leaf 64 first with 64 entries pending and pops one per leaf, so at leaf k it holds k
    entries, of which k - 8 are spilled for every k > 8; the rejecting leaf of each counted ray is required to be
    one of those (its index, from the oracle's record without alpha, is above 8)."""
    ch = ss.chain_tree(64, np.random.default_rng(31), tube=True, leaves=leaves, extras=True)
    rays, deep = bvh_ray_set(ch.leaf_lo, ch.leaf_hi, 32)
    exp, eany, dc, da = oracle_single(ch, rays)
    assert_exceeds_window(dc, deep, 8, "closest")
    assert_exceeds_window(da, deep, 8, "any")
    # one primitive per leaf: a walk that visited v nodes of this chain tested at most (v - 64) leaves' primitives
    # without a re-trace; with alpha 0 leaves in the chain, the rays that meet one re-test it
    plain = ch.prims.copy()
    plain["kind"] = np.where(np.isin(plain["kind"], ss.TRI_KINDS), 0, 1)
    plain["v"][plain["kind"] == 0, 3] = 0
    base = ob.closest(ch.nodes, plain, ch.verts, rays)
    rejected = deep & ((exp["prim"] != base["prim"]) | (exp["prim_tests"] != base["prim_tests"]))
    # the first hit of the walk without alpha is the first rejected one (ids are leaf indices): it lies above leaf 8
    rejected &= base["prim"] > 8
    assert rejected.sum() >= 200, "rays whose walk differs from the walk without alpha: a hit was rejected"
    kw = dict(normals=ch.normals, prim_alpha=ch.prim_alpha, uvs=ch.uvs)
    agg = BVHAggregate.from_tree(ch.nodes, ch.prims, ch.verts, **kw)
    with reaches(LEDGER, f"test_bvh_alpha[{'tri' if leaves == 'alpha_tri' else 'patch'}]"):
        check_all_modes(agg, rays, exp, eany, leaves, batches=False)
    agg.close()


@gpu
def test_bvh_host_only_chain():
    """Host-declared leaves at several levels of the chain (13 of 65, within the capacity of 16); they keep their triangles, so that the same
    arrays with kind 0 are the scene the resolved answers are held to, as tests/test_host_candidates.py does.  Plain
    calls: the rays that reach one are void, as the oracle says.  Candidate calls, in the single-batch, one-launch
    and wavefront forms: records, lists and `before` counts resolved with the host's triangle test equal the oracle on
    the all-triangle scene for EVERY ray.  The chain also fixes the lists themselves: a deep ray meets leaf 64 first
    and then every lower leaf (ids are leaf indices; leaves are 2 apart and 0.6 long), so its candidates are the host
    ids in descending order, and a device hit at leaf p comes after exactly the listed ids above p: before == count ==
    the number of host ids above p when tMax is infinite."""
    import torch
    from test_host_candidates import assert_resolved_equal, tri_callback, tri_table
    from test_wavefront_candidates import DevCands, Outputs, assert_cands_equal, gathered, ray_queue
    from nn_bvh_amd import resolve_host_candidates, resolve_host_candidates_any
    from nn_bvh_amd.interaction import ShadingMesh
    from nn_bvh_amd.wavefront import HostCandidateArrays, WavefrontAggregate
    from test_wavefront import shadow_inputs
    ch = ss.chain_tree(64, np.random.default_rng(44), tube=True, leaves="host_tri", extras=True)
    tris = ch.prims.copy()
    tris["kind"] = 0
    rays, deep = bvh_ray_set(ch.leaf_lo, ch.leaf_hi, 42)
    exp, eany, dc, da = oracle_single(ch, rays)
    assert_exceeds_window(dc, deep, 8, "closest")
    assert_exceeds_window(da, deep, 8, "any")
    assert (exp["instance"][deep] == -1).sum() > 50 and (eany[0][deep] == 2).sum() > 20
    agg = BVHAggregate.from_tree(ch.nodes, ch.prims, ch.verts)
    start = ledger_start(LEDGER, "test_bvh_host_only_chain")
    check_all_modes(agg, rays, exp, eany, "host-only chain")
    host_ids = np.sort(ch.prims["id"][ch.prims["kind"] == 3])[::-1]
    assert len(host_ids) == 13 and host_ids.min() < 8 and host_ids.max() > 56
    in_order = np.full(16, -1)
    in_order[:13] = host_ids
    kind0 = np.zeros(len(tris), np.int32)
    k16 = np.arange(16)[None, :]

    def check_closest(r, hits, cands, what):
        """records + lists of a closest call on rays r (deep: the first N_DEEP), resolved, against the oracle"""
        with ob.pending_depth(len(r)) as d:
            want = ob.closest(ch.nodes, tris, ch.verts, r)
        assert (d.depth[:N_DEEP, 0] == 64).all()
        cnt = cands["count"]
        assert (cnt >= 0).all() and (hits["instance"] == 0).all(), what
        res = resolve_host_candidates(r, hits, cands, tri_callback(r, ch.verts, tri_table(tris)), kind=kind0)
        assert_resolved_equal(res, want, what)
        for f in ("nodes_visited", "prim_tests"):
            assert np.array_equal(hits[f], exp_counts(r)[f]), f"{what}: {f}"
        won_by_host = (res["prim"] >= 0) & np.isin(res["prim"], host_ids)
        assert won_by_host[:N_DEEP].sum() > 50, what
        # the lists themselves, for the deep rays: a prefix of the descending host ids; with a device hit at leaf p
        # every listed id is above p and all of them were recorded before it
        dcnt, dprim, dbef = cnt[:N_DEEP], cands["prim"][:N_DEEP], cands["before"][:N_DEEP]
        listed = k16 < dcnt[:, None]
        assert (dprim[listed] == np.broadcast_to(in_order, dprim.shape)[listed]).all(), what
        p = hits["prim"][:N_DEEP]
        above = (host_ids[None, :] > p[:, None]).sum(1)
        dev_hit = p >= 0
        assert (dbef[dev_hit] == dcnt[dev_hit]).all() and (dbef[~dev_hit] == 0).all(), what + ": before"
        inf = np.isinf(r["tmax"][:N_DEEP])
        assert (dcnt[dev_hit & inf] == above[dev_hit & inf]).all(), what + ": count of the rays with a device hit"
        assert (dev_hit & inf & (dcnt > 0) & (p > 8)).sum() > 100, "candidates recorded before a hit, entries spilled"

    def exp_counts(r):
        return ob.closest(ch.nodes, ch.prims, ch.verts, r)  # the counters are the plain walk's

    def check_any(r, occ, cands, what):
        want = ob.any_hit(ch.nodes, tris, ch.verts, r)[0]
        assert np.array_equal(occ, ob.any_hit(ch.nodes, ch.prims, ch.verts, r)[0]), what
        assert (cands["before"] == 0).all() and np.array_equal(occ == 2, (cands["count"] != 0) & (occ != 1)), what
        assert (cands["count"] >= 0).all()
        got = resolve_host_candidates_any(r, occ, cands, tri_callback(r, ch.verts, tri_table(tris)))
        assert np.array_equal(got, want), what
        assert ((occ == 2) & (got == 1)).sum() > 20 and ((occ == 2) & (got == 0)).sum() > 20, what
        listed = k16 < cands["count"][:N_DEEP, None]
        assert (cands["prim"][:N_DEEP][listed] == np.broadcast_to(in_order, listed.shape)[listed]).all(), what

    # -- the single-batch calls (HOSTC twins of modes 0 and 2)
    hits, cands = agg.intersect_with_host_candidates(rays, capacity=16)
    check_closest(rays, hits, cands, "single-batch closest")
    for f in HIT_DTYPE.names:
        if f != "instance":
            assert np.array_equal(hits[f].view(np.uint32), exp[f].view(np.uint32)), f
    assert np.array_equal(exp["instance"] == -1, cands["count"] != 0)
    occ, acands = agg.intersect_p_with_host_candidates(rays, capacity=16)
    check_any(rays, occ, acands, "single-batch any")

    # -- one launch: a closest and an any batch with candidates (mode 3 HOSTC; fused_batches 0: the twins)
    from nn_bvh_amd import candidates_dtype
    rev = rays[::-1].copy()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    n = len(rays)

    def as_cands(count, before, prim, inst):
        c = np.zeros(len(count), candidates_dtype(16))
        c["count"], c["before"], c["prim"], c["instance"] = count, before, prim, inst
        return c
    for fused in (1, 0):
        agg.set_option("fused_batches", fused)
        d_c, d_a = upload(rays), upload(rev)
        o_c = torch.full((n * 32,), 0x5A, dtype=torch.uint8, device=dev)
        o_a = torch.full((n,), 0x5A, dtype=torch.uint8, device=dev)
        c_c, c_a = DevCands(n), DevCands(n)
        agg.trace_batches_candidates_device([("closest", d_c.data_ptr(), n, o_c.data_ptr()),
                                             ("any", d_a.data_ptr(), n, o_a.data_ptr())],
                                            [c_c.tup(True), c_a.tup(False)], stream)
        torch.cuda.synchronize()
        check_closest(rays, o_c.cpu().numpy().view(HIT_DTYPE), as_cands(*c_c.host()), f"one launch (fused {fused})")
        assert_cands_equal(c_c.host(), (cands["count"], cands["before"], cands["prim"], cands["instance"]), True,
                           f"one launch (fused {fused}) against the single batch")
        cnt, _, prim, inst = c_a.host()
        ac = as_cands(cnt[::-1], 0, prim[::-1], inst[::-1])
        check_any(rays, o_a.cpu().numpy()[::-1], ac, f"one launch any (fused {fused})")
    agg.set_option("fused_batches", 1)

    # -- the wavefront calls with candidates (a closest queue carries no tMax), device-side sizes below the capacity
    m = n - 137
    mesh = ShadingMesh(ch.verts, tri_table(tris))
    wf = WavefrontAggregate(agg)
    rq, sq = ray_queue(rays), ray_queue(rays, shadow=True)
    rq.size.fill_(m)
    sq.size.fill_(m)
    out = Outputs(n)
    wf.IntersectClosestItemsWithCandidates(n, rq, mesh, out.cands, out.hits, items=out.items,
                                           needs_host=out.needs_host, **out.queues)
    Ld, r_u, r_l, px, L = shadow_inputs(n, n + 500, 7)
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    d_l = t(L)
    socc = torch.full((n,), 9, dtype=torch.uint8, device=dev)
    sc = HostCandidateArrays(n, 16, dev)
    wf.IntersectShadowWithCandidates(n, sq, t(Ld), t(r_u), t(r_l), t(px), d_l, socc, sc)
    torch.cuda.synchronize()
    check_closest(gathered(rays)[:m], out.hit_records()[:m], out.cands.numpy()[:m], "wavefront closest")
    assert np.array_equal(np.sort(out.needs_host.indices().cpu().numpy()),
                          np.nonzero(out.cands.numpy()["count"][:m] != 0)[0])
    h_occ = socc.cpu().numpy()
    assert (h_occ[m:] == 9).all()
    check_any(rays[:m], h_occ[:m], sc.numpy()[:m], "wavefront shadow")
    first = ob.record_shadow(np.where(h_occ[:m] == 0, 0, 1).astype(np.uint8), Ld[:m], r_u[:m], r_l[:m], px[:m], L)
    assert np.array_equal(d_l.cpu().numpy().view(np.uint32), first.view(np.uint32))
    assert_reached(LEDGER, "test_bvh_host_only_chain", start)
    mesh.close()
    agg.close()


# ---- GPU: two-level scenes -----------------------------------------------------------------------------------------
@gpu
def test_two_level_chain():
    """a + b + 1 == 64 is accepted and exact in modes 0 / 1 / 2 and in one launch; the child walk spills OUTER entries
    (31 pending at the deepest instance's entry, 32 more inside) and kReturn pops back below `base`."""
    t = ss.two_level_chain(31, 32, 5)
    rays, deep = bvh_ray_set(t.outer_lo, t.outer_hi, 6)
    with ob.pending_depth(len(rays)) as dc:
        exp = ob.closest_inst(t.nodes, t.prims, t.verts, t.instances, rays)
    with ob.pending_depth(len(rays)) as da:
        eany = ob.any_hit_inst(t.nodes, t.prims, t.verts, t.instances, rays)
    for d in (dc.depth, da.depth):
        assert_exceeds_window(d[:, 0], deep, 8, "two-level")
        both = deep & (d[:, 1] > 8) & (d[:, 2] > 8)
        assert both.sum() >= N_DEEP, "every deep ray enters an instance with > 8 outer entries and goes > 8 deep in it"
    agg = BVHAggregate.from_tree(t.nodes, t.prims, t.verts, instances=t.instances, n_top_nodes=t.n_top)
    assert agg.info["depth"] == 64
    with reaches(LEDGER, "test_two_level_chain"):
        check_all_modes(agg, rays, exp, eany, "two-level chain")
    assert (exp["instance"][deep] > 0).sum() > 500
    agg.close()


def test_two_level_chain_of_65_is_refused(nnbvh_lib):  # (refused on the host, before any device work)
    t = ss.two_level_chain(32, 32, 5)
    with pytest.raises(NNBVHError, match="deeper than the 64-entry"):
        BVHAggregate.from_tree(t.nodes, t.prims, t.verts, instances=t.instances, n_top_nodes=t.n_top)


@gpu
def test_animated_two_level_chain():
    """INST = 2 at a + b + 1 == 64, against the oracle with the device's sine (tests/test_animated.py: the documented
    exception), ray times inside, at and outside the time range.  The child walk spills outer entries as in the
    static scene; the transform it runs under is interpolated per ray."""
    t, anims, oa = ss.animated_two_level_chain(31, 32, 5)
    rays, deep = anim_ray_set(t, 6)
    exp, eany, dc, da = oracle_anim(t, oa, rays, 1)
    for d in (dc, da):
        assert_exceeds_window(d[:, 0], deep, 8, "animated two-level")
        both = deep & (d[:, 1] > 8) & (d[:, 2] > 8)
        assert both.sum() >= N_DEEP, "every deep ray enters an instance with > 8 outer entries and goes > 8 deep in it"
    tm = rays["time"][deep]
    assert ((tm > 0) & (tm < 1)).sum() > 400 and (tm == 0).sum() > 50 and (tm == 1).sum() > 50
    assert (tm < 0).sum() > 50 and (tm > 1).sum() > 50
    agg = BVHAggregate.from_tree(t.nodes, t.prims, t.verts, instances=t.instances, n_top_nodes=t.n_top, animated=anims)
    assert agg.info["depth"] == 64
    with reaches(LEDGER, "test_animated_two_level_chain"):
        check_all_modes(agg, rays, exp, eany, "animated two-level chain")
    moving = oa["actually_animated"][np.maximum(exp["instance"] - 1, 0)] != 0
    assert ((exp["instance"] > 0) & moving & deep & (rays["time"] > 0) & (rays["time"] < 1)).sum() > 100
    agg.close()


def test_animated_two_level_chain_of_65_is_refused(nnbvh_lib):
    t, anims, oa = ss.animated_two_level_chain(32, 32, 5)
    with pytest.raises(NNBVHError, match="deeper than the 64-entry"):
        BVHAggregate.from_tree(t.nodes, t.prims, t.verts, instances=t.instances, n_top_nodes=t.n_top, animated=anims)


# ---- GPU: kd-trees ---------------------------------------------------------------------------------------------------
def kd_ray_set(k, seed, n_deep=N_DEEP, n_random=N_RANDOM):
    rays = np.concatenate([ss.kd_chain_rays(n_deep, seed, KD_TMAX_SHARE),
                           scene.random_rays(n_random, k.bounds[:3] - 1, k.bounds[3:] + 1, seed + 1)])
    return rays, (np.arange(len(rays)) < n_deep) & np.isinf(rays["tmax"])


def kd_oracle(k, rays):
    with attributes(k):
        with ob.pending_depth(len(rays)) as dc:
            exp = ob.kd_closest(k.nodes, k.prim_indices, k.prims, k.verts, k.bounds, rays)
        with ob.pending_depth(len(rays)) as da:
            eany = ob.kd_any_hit(k.nodes, k.prim_indices, k.prims, k.verts, k.bounds, rays)
    return exp, eany, dc.depth[:, 0], da.depth[:, 0]


@gpu
@pytest.mark.parametrize("form,window,offsets32",
                         [("lean", 4, 1), ("patch", 8, 1), ("attr", 8, 1), ("lean", 4, 0), ("patch", 8, 0), ("attr", 8, 0)],
                         ids=["lean", "patch", "attr", "lean-wide", "patch-wide", "attr-wide"])
def test_kd_chain(form, window, offsets32):
    """offsets32 0 (the *-wide cases): the same scene, calls and assertions through the O32 = 0 instances — the HBM
    spill and the 64-bit addressing, the two rarely-run mechanisms, in one walk."""
    import torch
    k = ss.kd_chain(64, 7, form)
    rays, deep = kd_ray_set(k, 9)
    exp, eany, dc, da = kd_oracle(k, rays)
    assert_exceeds_window(dc, deep, window, "kd closest")
    assert_exceeds_window(da, deep, window, "kd any")
    agg = KdTreeAggregate.from_tree(k.nodes, k.prim_indices, k.prims, k.verts, k.bounds, normals=k.normals, uvs=k.uvs,
                                    prim_alpha=k.prim_alpha)
    agg.set_option("offsets32", offsets32)
    start = ledger_start(LEDGER, f"test_kd_chain[{form}{'' if offsets32 else '-wide'}]")
    assert agg.Intersect(rays).tobytes() == exp.tobytes()
    occ, vis, tst = agg.IntersectP(rays, counts=True)
    assert np.array_equal(occ, eany[0]) and np.array_equal(vis, eany[1]) and np.array_equal(tst, eany[2])
    assert np.array_equal(agg.IntersectP(rays), eany[0])
    # one launch: a closest and an any batch (with counts) from ray records: the batch-mode instance
    rev = rays[::-1].copy()
    dcl, dan = upload(rays), upload(rev)
    oc = torch.full((len(rays) * 32,), 0x5A, dtype=torch.uint8, device="cuda")
    oa = torch.full((len(rays),), 0x5A, dtype=torch.uint8, device="cuda")
    ov = torch.zeros(len(rays), dtype=torch.int32, device="cuda")
    ot = torch.zeros(len(rays), dtype=torch.int32, device="cuda")
    agg.trace_batches_device([("closest", dcl.data_ptr(), len(rays), oc.data_ptr()),
                              ("any", dan.data_ptr(), len(rays), oa.data_ptr(), ov.data_ptr(), ot.data_ptr())],
                             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert oc.cpu().numpy().view(HIT_DTYPE).tobytes() == exp.tobytes()
    assert np.array_equal(oa.cpu().numpy(), eany[0][::-1]) and np.array_equal(ov.cpu().numpy(), eany[1][::-1])
    assert np.array_equal(ot.cpu().numpy(), eany[2][::-1])

    # the queue calls: SOA slices read by the kernel (lean, read_soa 1: batch mode 3) and gathered into records
    def walk(kind, r):
        with attributes(k):
            with ob.pending_depth(len(r)) as d:
                res = (ob.kd_closest if kind == "closest" else ob.kd_any_hit)(k.nodes, k.prim_indices, k.prims,
                                                                              k.verts, k.bounds, r)
        return res, d.depth[:, 0]
    for read_soa, pair in ((1, 1), (0, 1), (1, 0)):
        agg.set_option("read_soa", read_soa)
        agg.set_option("pair_one_launch", pair)
        check_queue_calls(agg, walk, rays, deep, window, f"kd {form} read_soa {read_soa} pair_one_launch {pair}")
    assert_reached(LEDGER, f"test_kd_chain[{form}{'' if offsets32 else '-wide'}]", start)
    agg.close()


def test_kd_chain_of_65_is_refused(nnbvh_lib):
    k = ss.kd_chain(65, 7, "lean")
    with pytest.raises(NNBVHError, match="deeper than the traversal stack"):
        KdTreeAggregate.from_tree(k.nodes, k.prim_indices, k.prims, k.verts, k.bounds)


# ---- GPU: one deep ray in every lane of the largest grid ----------------------------------------------------------------
# kBlockThreads = 256 (bvh_trace.h) and kKdBlock = 256 (kd_trace.h); both libraries launch at most 8 blocks per CU
BLOCK_THREADS = 256
N_DISTINCT = 4096


def full_grid_count():
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = int(1.25 * cus * 8 * BLOCK_THREADS) + 1
    return (n + N_DISTINCT - 1) // N_DISTINCT * N_DISTINCT  # whole tiles of the distinct rays


def two_streams(call, d_rays, n, out_bytes):
    """the same batch on two streams at once (each stream has its own workspace) -> the two output buffers"""
    import torch
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = [torch.full((n * out_bytes,), 0x5A, dtype=torch.uint8, device="cuda") for _ in streams]
    torch.cuda.synchronize()
    for st, o in zip(streams, outs):
        call(d_rays.data_ptr(), o.data_ptr(), n, st.cuda_stream)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs]


@gpu
def test_full_grid_bvh_any_hit_with_counts():
    """Lean window-8 instance, mode 1 (every far child is pushed), blocks_per_cu 8: 1.25 deep rays per lane of the
    largest grid, so every lane holds a deep ray at once and the last lane reaches the last level of the spill array
    (max(depth - 2, 1) levels of n_cus * 8 * 256 lanes).  The rays are 4096 distinct deep rays tiled."""
    ch = ss.chain_tree(64, np.random.default_rng(51), tube=True, leaves="tri", extras=True)
    distinct = ss.chain_rays(float(ch.leaf_hi[:, 0].max()), N_DISTINCT, 52, tmax_share=0.0)
    with ob.pending_depth(N_DISTINCT) as da:
        eocc, evis, etst = ob.any_hit(ch.nodes, ch.prims, ch.verts, distinct, 8)
    assert (da.depth[:, 0] == 64).all()
    n = full_grid_count()
    rays = np.tile(distinct, n // N_DISTINCT)
    agg = BVHAggregate.from_tree(ch.nodes, ch.prims, ch.verts)
    agg.set_option("blocks_per_cu", 8)
    start = ledger_start(LEDGER, "test_full_grid_bvh_any_hit_with_counts")
    occ, vis, tst = agg.IntersectP(rays, counts=True)
    idx = np.random.default_rng(53).choice(n, 60000, replace=False)
    assert np.array_equal(occ[idx], eocc[idx % N_DISTINCT]) and np.array_equal(vis[idx], evis[idx % N_DISTINCT])
    assert np.array_equal(tst[idx], etst[idx % N_DISTINCT])
    for got, one in ((occ, eocc), (vis, evis), (tst, etst)):  # every copy equals its original
        assert (got.reshape(-1, N_DISTINCT) == one[None, :]).all()
    d_rays = upload(rays)

    import torch
    # the counting call (mode 1) on both streams: its counters, per stream.  They are zeroed here, ahead of
    # two_streams' synchronize: a fill on the default stream is not ordered against a launch on another stream
    counts = [[torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2)] for _ in range(2)]
    unused = iter(counts)

    def call(r, o, m, st):
        v, c = next(unused)
        agg.intersect_p_device(r, o, m, v.data_ptr(), c.data_ptr(), stream=st)
    for flags, (v, c) in zip(two_streams(call, d_rays, n, 1), counts):
        assert (flags.reshape(-1, N_DISTINCT) == eocc[None, :]).all()
        assert (v.cpu().numpy().reshape(-1, N_DISTINCT) == evis[None, :]).all()
        assert (c.cpu().numpy().reshape(-1, N_DISTINCT) == etst[None, :]).all()
    assert_reached(LEDGER, "test_full_grid_bvh_any_hit_with_counts", start)
    agg.close()


@gpu
def test_full_grid_kd_closest():
    """Lean kd instance (window 4), closest hit: 1.25 deep rays per lane of n_cus * 8 * 256 lanes, the size of the kd
    spill array's levels (depth + 1 - 4 of them)."""
    k = ss.kd_chain(64, 7, "lean")
    distinct = ss.kd_chain_rays(N_DISTINCT, 54, tmax_share=0.0)
    with ob.pending_depth(N_DISTINCT) as dc:
        exp = ob.kd_closest(k.nodes, k.prim_indices, k.prims, k.verts, k.bounds, distinct, 8)
    assert (dc.depth[:, 0] == 64).all()
    n = full_grid_count()
    rays = np.tile(distinct, n // N_DISTINCT)
    agg = KdTreeAggregate.from_tree(k.nodes, k.prim_indices, k.prims, k.verts, k.bounds)
    start = ledger_start(LEDGER, "test_full_grid_kd_closest")
    got = agg.Intersect(rays)
    idx = np.random.default_rng(55).choice(n, 60000, replace=False)
    assert got[idx].tobytes() == exp[idx % N_DISTINCT].tobytes()
    one = exp.view(np.uint8).reshape(1, -1)  # every copy equals its original, byte for byte
    assert (got.view(np.uint8).reshape(n // N_DISTINCT, -1) == one).all()
    d_rays = upload(rays)
    for rec in two_streams(agg.intersect_device, d_rays, n, 32):
        assert (rec.reshape(n // N_DISTINCT, -1) == one).all()
    assert_reached(LEDGER, "test_full_grid_kd_closest", start)
    agg.close()


# ---- GPU: scheduling must not change a byte on deep scenes -----------------------------------------------------------
TUNING = (("xcd_queues", 0), ("refill_weight", 1), ("refill_weight", 64), ("prim_weight", 1), ("prim_weight", 64),
          ("int_repeat", 1), ("int_repeat", 5), ("prim_repeat", 1), ("prim_repeat", 4))


@gpu
@pytest.mark.parametrize("which", ["two_level", "alpha"])
def test_deep_results_independent_of_tuning_and_order(which):
    if which == "two_level":
        t = ss.two_level_chain(31, 32, 5)
        rays, _ = bvh_ray_set(t.outer_lo, t.outer_hi, 61)
        agg = BVHAggregate.from_tree(t.nodes, t.prims, t.verts, instances=t.instances, n_top_nodes=t.n_top)
    else:
        ch = ss.chain_tree(64, np.random.default_rng(62), tube=True, leaves="alpha_patch", extras=True)
        rays, _ = bvh_ray_set(ch.leaf_lo, ch.leaf_hi, 63)
        agg = BVHAggregate.from_tree(ch.nodes, ch.prims, ch.verts, normals=ch.normals, prim_alpha=ch.prim_alpha,
                                     uvs=ch.uvs)

    def run(r):
        occ, vis, tst = agg.IntersectP(r, counts=True)
        return agg.Intersect(r), occ, vis, tst, agg.IntersectP(r)
    start = ledger_start(LEDGER, f"test_deep_results_independent_of_tuning_and_order[{which}]")
    base = run(rays)
    perm = np.random.default_rng(0).permutation(len(rays))
    for a, b in zip(run(rays[perm]), base):
        assert a.tobytes() == b[perm].tobytes(), "ray order changed a result"
    for key, val in TUNING:
        agg.set_option(key, val)
        for a, b in zip(run(rays), base):
            assert a.tobytes() == b.tobytes(), f"{key}={val} changed a result"
    assert_reached(LEDGER, f"test_deep_results_independent_of_tuning_and_order[{which}]", start)
    agg.close()
