"""Host-only candidates through the one-launch batches and the wavefront queue entry points (include/nnbvh.h:
nnbvh_trace_batches_candidates_device, nnbvh_wavefront_*_candidates, nnbvh_wavefront_enqueue_closest_items_
indexed_device).  Everything is held bit for bit to paths that are pinned already: the single-batch candidate calls,
the plain wavefront calls, and the oracle on the same scene with the host-declared primitives as triangles.
CPU: exports and the C ABI's argument checks.  GPU: the scenes of tests/test_host_candidates.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import oracle_binding as ob
from ledger_cases import BVH, assert_reached, bvh, ledger_start
from nn_bvh_amd import (BVHAggregate, _lib, candidates_dtype, resolve_host_candidates, resolve_host_candidates_any,
                        scene)
from nn_bvh_amd._lib import HIT_DTYPE, RAY_DTYPE
from test_host_candidates import (assert_resolved_equal, declare_host, flat_host_scene, tri_callback, tri_table,
                                  unique_id_two_level)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = 1
QUEUES = _lib.CLOSEST_QUEUES
NEW_SYMBOLS = ("nnbvh_trace_batches_candidates_device", "nnbvh_wavefront_intersect_closest_items_candidates",
               "nnbvh_wavefront_enqueue_closest_items_indexed_device", "nnbvh_wavefront_intersect_shadow_candidates",
               "nnbvh_wavefront_intersect_closest_and_shadow_items_candidates")

# ---------------------------------------------------------------------------------------------------- CPU
C_PROBE = r"""
#include <stdio.h>
#include "nnbvh.h"
int main(void) {
    int32_t count[1], before[1], prim[4], inst[4], index[1] = {0}, size[1] = {1}, px[1] = {0};
    nnbvh_host_candidates c = {4, count, before, prim, inst};
    nnbvh_ray r = {{0, 0, 0}, 1.0f, {0, 0, 1}, 0.0f};
    nnbvh_hit h;
    uint8_t occ;
    float f[4] = {0, 0, 0, 0};
    nnbvh_batch b = {NNBVH_BATCH_CLOSEST, 0, &r, 1, &h, NULL, NULL};
    nnbvh_ray_soa q = {f, f, f, f, f, f, NULL, f, NULL};
    nnbvh_closest_queues out = {{NULL, NULL, 0, 0}, {NULL, NULL, 0, 0}, {NULL, NULL, 0, 0}, {NULL, NULL, 0, 0},
                                {NULL, NULL, 0, 0}, {NULL, NULL, 0, 0}};
    static nnbvh_closest_items items;
    printf("%d %d %d %d %d\n", nnbvh_trace_batches_candidates_device(NULL, &b, 1, &c, NULL),
           nnbvh_wavefront_intersect_closest_items_candidates(NULL, NULL, 1, &q, size, NULL, 0, &h, &out, &items, &c, NULL),
           nnbvh_wavefront_enqueue_closest_items_indexed_device(NULL, 1, &q, index, size, 1, &h, NULL, 0, &out, &items,
                                                                NULL),
           nnbvh_wavefront_intersect_shadow_candidates(NULL, 1, &q, size, f, f, f, px, f, 1, &occ, &c, NULL),
           nnbvh_wavefront_intersect_closest_and_shadow_items_candidates(NULL, NULL, 1, &q, size, NULL, 0, &h, &out,
                                                                         &items, &c, 1, &q, size, f, f, f, px, f, 1,
                                                                         &occ, &c, NULL));
    return 0;
}
"""


def test_new_symbols_are_exported(nnbvh_lib):
    for s in NEW_SYMBOLS:
        assert s in _lib.EXPORTS and hasattr(nnbvh_lib, s), s


def test_c11_probe_gets_err_arg_for_a_null_scene(nnbvh_lib, tmp_path):
    src, exe = tmp_path / "probe.c", tmp_path / "probe"
    src.write_text(C_PROBE)
    libdir = os.path.join(ROOT, "nn_bvh_amd")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                    "-o", str(exe), "-L", libdir, "-l:libnnbvh_hip.so", f"-Wl,-rpath,{libdir}",
                    "-Wl,-rpath-link,/opt/rocm/lib"], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.split() == [str(ERR_ARG)] * 5


def test_python_layer_has_the_new_calls():
    from nn_bvh_amd import wavefront
    assert hasattr(BVHAggregate, "trace_batches_candidates_device")
    for name in ("IntersectClosestItemsWithCandidates", "IntersectShadowWithCandidates",
                 "IntersectClosestAndShadowItemsWithCandidates"):
        assert hasattr(wavefront.WavefrontAggregate, name), name
    import inspect
    assert "index" in inspect.signature(wavefront.enqueue_closest_items).parameters


# ---------------------------------------------------------------------------------------------------- GPU
K = 16
SCENES = ("flat", "two_level", "animated")
BATCHES_TEST = "test_batches_equal_the_single_batch_candidate_calls"
# case and part of the case -> (kernel family, the instances its device calls launch), asserted with the launch ledger
# (tests/ledger_cases.py); a key is the pytest id followed by the part.  Per scene form INST = 0 / 1 / 2: the
# single-batch candidate calls run the twins of modes 0 / 2; with "fused_batches" 1 the candidate batches and the plain
# batches beside them run in ONE launch each, the mode-3 twin and the plain mode-3 form; with 0 every batch runs alone
# on a side stream as mode 0 or 2, twin or plain
LEDGER = {}
for _name, _inst in zip(SCENES, (0, 1, 2)):
    LEDGER.update({
        f"{BATCHES_TEST}[{_name}] single calls": (BVH, bvh((0, 2), inst=_inst, hostc=1)),
        f"{BATCHES_TEST}[{_name}] fused_batches 1": (BVH, bvh((3,), inst=_inst, hostc=1) | bvh((3,), inst=_inst)),
        f"{BATCHES_TEST}[{_name}] fused_batches 0": (BVH, bvh((0, 2), inst=_inst, hostc=1) | bvh((0, 2), inst=_inst)),
    })


class Case:
    """One scene with host-declared triangles: its aggregate, the same scene with every primitive a triangle (the
    oracle's and a second aggregate's), a shading mesh that holds every triangle, rays, and the host callback."""

    # the ray sets of tests/test_host_candidates.py (same generators, seeds and sizes)
    N_RAYS = {"flat": 20000, "two_level": 25000, "animated": 20000}

    def __init__(self, name, n_rays=None):
        n_rays = n_rays or self.N_RAYS[name]
        from nn_bvh_amd.interaction import ShadingMesh
        self.name = name
        self.sin_mode = 0
        if name == "flat":
            verts, prims, host, tree_h, tree_t = flat_host_scene(0)
            self.rays = scene.random_rays(n_rays, verts.min(0), verts.max(0), 3)
            self.all_tris = prims
            self.host_args = dict(nodes=tree_h.nodes, ordered_prims=tree_h.ordered_prims, verts=verts)
            self.tri_args = dict(nodes=tree_t.nodes, ordered_prims=tree_t.ordered_prims, verts=verts)
            self.oracle_closest = lambda r: ob.closest(tree_t.nodes, tree_t.ordered_prims, verts, r, 4)
            self.oracle_any = lambda r: ob.any_hit(tree_t.nodes, tree_t.ordered_prims, verts, r, 4)[0]
            self.minv, instances, anims = None, None, None
        elif name == "two_level":
            verts, nodes, prims, instances, n_top, all_tris, placements, objects = unique_id_two_level(2, 50)
            hp = declare_host(prims, 5, 2)
            lo = np.array([-30, -30, -30.0])
            self.rays = scene.random_rays(n_rays, lo, -lo, 21)
            self.all_tris = all_tris
            self.host_args = dict(nodes=nodes, ordered_prims=hp, verts=verts, instances=instances, n_top_nodes=n_top)
            self.tri_args = dict(nodes=nodes, ordered_prims=prims, verts=verts, instances=instances, n_top_nodes=n_top)
            self.oracle_closest = lambda r: ob.closest_inst(nodes, prims, verts, instances, r, 4)
            self.oracle_any = lambda r: ob.any_hit_inst(nodes, prims, verts, instances, r, 4)[0]
            self.minv = lambda idx, k: instances["prim_from_render"][k]
            anims = None
        else:
            from test_animated import animated_scene, rebuild_with_motion_bounds
            verts, prims0, _, _, _, _, anims, oa, placements = animated_scene(4, 30)
            nodes, aprims, instances, n_top = rebuild_with_motion_bounds(verts, prims0, placements, anims, oa)
            hp = declare_host(aprims, 4, 1)
            self.rays = scene.random_rays(n_rays, [-25, -25, -25], [25, 25, 25], 5)
            self.rays["time"] = np.random.default_rng(6).uniform(-0.2, 1.2, n_rays).astype(np.float32)
            self.all_tris = prims0
            self.host_args = dict(nodes=nodes, ordered_prims=hp, verts=verts, instances=instances, n_top_nodes=n_top,
                                  animated=anims)
            self.tri_args = dict(nodes=nodes, ordered_prims=aprims, verts=verts, instances=instances,
                                 n_top_nodes=n_top, animated=anims)
            self.oracle_closest = lambda r: ob.closest_anim(nodes, aprims, verts, instances, oa, r, 4)
            self.oracle_any = lambda r: ob.any_hit_anim(nodes, aprims, verts, instances, oa, r, 4)[0]
            self.sin_mode = 1  # the device's Slerp sine (test_animated.py: the documented exception)

            def minv(idx, k, rays=None):
                rows = instances["prim_from_render"][k].copy()
                a = anims["actually_animated"][k] != 0
                if a.any():
                    rows[a] = ob.anim_interpolate(oa[k[a]], self._cb_rays["time"][idx[a]])[:, 16:28]
                return rows
            self.minv = minv
        self.verts = verts
        self.agg = BVHAggregate.from_tree(**self.host_args)
        self.mesh = ShadingMesh(verts, tri_table(self.all_tris))
        if instances is not None:
            self.mesh.set_instances(instances, anims)
        is_host = np.zeros(len(tri_table(self.all_tris)), bool)
        hp_ = self.host_args["ordered_prims"]
        is_host[hp_["id"][hp_["kind"] == 3]] = True
        self.is_host = is_host

    def callback(self, rays):
        self._cb_rays = rays
        return tri_callback(rays, self.verts, tri_table(self.all_tris), self.minv)

    def oracle(self, fn, *a):
        try:
            ob.set_sin_mode(self.sin_mode)
            return fn(*a)
        finally:
            ob.set_sin_mode(0)

    def close(self):
        self.agg.close()
        self.mesh.close()


def dev0():
    import torch
    return torch.device("cuda", 0)


def stream0():
    import torch
    return torch.cuda.current_stream(dev0()).cuda_stream


class DevCands:
    """Sentinel-filled device candidate arrays for n rays."""

    def __init__(self, n, k=K, sentinel=77):
        import torch
        dev = dev0()
        self.n, self.k = n, k
        self.count = torch.full((n,), sentinel, dtype=torch.int32, device=dev)
        self.before = torch.full((n,), sentinel, dtype=torch.int32, device=dev)
        self.prim = torch.full((n, k), -1, dtype=torch.int32, device=dev)
        self.instance = torch.full((n, k), -1, dtype=torch.int32, device=dev)

    def tup(self, closest=True):
        return (self.k, self.count.data_ptr(), self.before.data_ptr() if closest else None, self.prim.data_ptr(),
                self.instance.data_ptr())

    def host(self):
        return tuple(t.cpu().numpy() for t in (self.count, self.before, self.prim, self.instance))


def assert_cands_equal(a, b, closest, what):
    ca, ba, pa, ia = a
    cb, bb, pb, ib = b
    assert np.array_equal(ca, cb), what + ": count"
    if closest:
        assert np.array_equal(ba, bb), what + ": before"
    j = np.arange(pa.shape[1])[None, :] < ca[:, None]
    assert np.array_equal(pa[j], pb[j]) and np.array_equal(ia[j], ib[j]), what + ": prim / instance"


def upload(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(len(a), -1).copy()).to(dev0())


def single_batch_reference(agg, rays, kind):
    """nnbvh_intersect_{closest,any}_candidates_device on `rays`: (output bytes, candidate arrays)."""
    import torch
    n = len(rays)
    d_rays = upload(rays)
    c = DevCands(n)
    if kind == "closest":
        out = torch.zeros((n, 32), dtype=torch.uint8, device=dev0())
        agg.intersect_candidates_device(d_rays.data_ptr(), out.data_ptr(), n, K, c.count.data_ptr(),
                                        c.before.data_ptr(), c.prim.data_ptr(), c.instance.data_ptr(), stream0())
    else:
        out = torch.zeros(n, dtype=torch.uint8, device=dev0())
        agg.intersect_p_candidates_device(d_rays.data_ptr(), out.data_ptr(), n, K, c.count.data_ptr(),
                                          c.prim.data_ptr(), c.instance.data_ptr(), stream0())
    torch.cuda.synchronize()
    return out.cpu().numpy(), c.host()


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_batches_equal_the_single_batch_candidate_calls(name):
    import torch
    case = Case(name, 9000)
    agg, rays = case.agg, case.rays
    parts = [("closest", rays[:4000]), ("any", rays[4000:7000].copy()), ("closest", rays[7000:])]
    parts[1][1]["tmax"] = np.float32(0.7)
    start = ledger_start(LEDGER, f"{BATCHES_TEST}[{name}] single calls")
    refs = [single_batch_reference(agg, r, kind) for kind, r in parts]
    assert_reached(LEDGER, f"{BATCHES_TEST}[{name}] single calls", start)
    oracle = [case.oracle(case.oracle_closest if kind == "closest" else case.oracle_any, r) for kind, r in parts]
    assert (refs[0][1][0] > 0).any() and (refs[1][1][0] > 0).any() and (refs[2][1][1] > 0).any()  # the paths are exercised
    for fused in (1, 0):
        start = ledger_start(LEDGER, f"{BATCHES_TEST}[{name}] fused_batches {fused}")
        agg.set_option("fused_batches", fused)
        d_rays = [upload(r) for _, r in parts]
        outs = [torch.zeros((len(r), 32) if kind == "closest" else (len(r),), dtype=torch.uint8, device=dev0())
                for kind, r in parts]
        cs = [DevCands(len(r)) for _, r in parts]
        batches = [(kind, d.data_ptr(), len(r), o.data_ptr()) for (kind, r), d, o in zip(parts, d_rays, outs)]
        agg.trace_batches_candidates_device(batches, [c.tup(kind == "closest") for c, (kind, _) in zip(cs, parts)],
                                            stream0())
        torch.cuda.synchronize()
        for b, ((kind, r), o, c, ref) in enumerate(zip(parts, outs, cs, refs)):
            what = f"{name} fused={fused} batch {b} ({kind})"
            assert o.cpu().numpy().tobytes() == ref[0].tobytes(), what + ": output"
            assert_cands_equal(c.host(), ref[1], kind == "closest", what)
            # ... and, resolved with the host's triangle test, the oracle on the all-triangle scene
            packed = np.zeros(len(r), candidates_dtype(K))
            packed["count"], packed["before"], packed["prim"], packed["instance"] = c.host()
            ok = packed["count"] >= 0
            if kind == "closest":
                res = case.oracle(resolve_host_candidates, r, o.cpu().numpy().view(HIT_DTYPE).reshape(-1), packed,
                                  case.callback(r), np.zeros(len(case.is_host), np.int32))
                assert_resolved_equal(res[ok], oracle[b][ok], what + " against the oracle")
            else:
                res = case.oracle(resolve_host_candidates_any, r, o.cpu().numpy(), packed, case.callback(r))
                assert np.array_equal(res[res != 2], oracle[b][res != 2]), what + " against the oracle"
        # a batch with capacity 0 is a plain batch: nnbvh_trace_batches_device's output, arrays untouched
        plain = [torch.zeros_like(o) for o in outs]
        agg.trace_batches_device([(kind, d.data_ptr(), len(r), o.data_ptr())
                                  for (kind, r), d, o in zip(parts, d_rays, plain)], stream0())
        outs2 = [torch.zeros_like(o) for o in outs]
        cs2 = [DevCands(len(r)) for _, r in parts]
        batches2 = [(kind, d.data_ptr(), len(r), o.data_ptr()) for (kind, r), d, o in zip(parts, d_rays, outs2)]
        agg.trace_batches_candidates_device(batches2, [None, cs2[1].tup(False), None], stream0())
        torch.cuda.synchronize()
        for b in (0, 2):
            assert torch.equal(outs2[b], plain[b]), f"{name} fused={fused}: plain batch {b}"
            assert (cs2[b].count == 77).all()
        assert outs2[1].cpu().numpy().tobytes() == refs[1][0].tobytes()
        assert_cands_equal(cs2[1].host(), refs[1][1], False, f"{name} fused={fused}: mixed call")
        assert_reached(LEDGER, f"{BATCHES_TEST}[{name}] fused_batches {fused}", start)
    case.close()


@pytest.mark.gpu
def test_batches_bad_arguments_launch_nothing():
    import torch
    case = Case("flat", 3000)
    agg, rays = case.agg, case.rays
    n = len(rays)
    d_rays = upload(rays)
    hits = torch.full((n, 32), 0x5a, dtype=torch.uint8, device=dev0())
    occ = torch.full((n,), 0x5a, dtype=torch.uint8, device=dev0())
    vis = torch.zeros(n, dtype=torch.int32, device=dev0())
    c = DevCands(n)
    L = _lib.lib()
    p = lambda t: t.data_ptr()  # noqa: E731

    def call(kind, out, cand, vis_ptr=0):
        arr = np.zeros(1, _lib.BATCH_DTYPE)
        arr["kind"], arr["d_rays"], arr["n"], arr["d_out"], arr["d_nodes_visited"] = kind, p(d_rays), n, p(out), vis_ptr
        cs = (_lib.HostCandidates * 1)(cand)
        return L.nnbvh_trace_batches_candidates_device(agg._h, _lib.ptr(arr), 1, cs, stream0())

    HC = _lib.HostCandidates
    bad_closest = [HC(-1, p(c.count), p(c.before), p(c.prim), p(c.instance)),
                   HC(17, p(c.count), p(c.before), p(c.prim), p(c.instance)),
                   HC(8, None, p(c.before), p(c.prim), p(c.instance)),
                   HC(8, p(c.count), p(c.before), None, p(c.instance)),
                   HC(8, p(c.count), p(c.before), p(c.prim), None),
                   HC(8, p(c.count), None, p(c.prim), p(c.instance))]
    for cand in bad_closest:
        assert call(0, hits, cand) == ERR_ARG
    for cand in bad_closest[:5]:
        assert call(1, occ, cand) == ERR_ARG
    # an any-hit batch asks for exact counts or for candidates, not both
    assert call(1, occ, HC(8, p(c.count), None, p(c.prim), p(c.instance)), p(vis)) == ERR_ARG
    arr = np.zeros(1, _lib.BATCH_DTYPE)
    arr["d_rays"], arr["n"], arr["d_out"] = p(d_rays), n, p(hits)
    assert L.nnbvh_trace_batches_candidates_device(agg._h, _lib.ptr(arr), 1, None, stream0()) == ERR_ARG
    torch.cuda.synchronize()
    assert (hits == 0x5a).all() and (occ == 0x5a).all()
    assert (c.count == 77).all() and (c.before == 77).all() and (c.prim == -1).all() and (c.instance == -1).all()
    case.close()


# ---- wavefront ---------------------------------------------------------------------------------------------
def ray_queue(rays, shadow=False):
    import torch
    from nn_bvh_amd.wavefront import RayQueue
    rq = RayQueue.from_records(rays, dev0(), shadow=shadow)
    rq.time = torch.from_numpy(np.ascontiguousarray(rays["time"])).to(dev0())
    return rq


def gathered(rays, shadow=False):
    """The nnbvh_ray records the wavefront calls trace for a queue: tmax = Infinity unless a shadow queue."""
    r = rays.copy()
    if not shadow:
        r["tmax"] = np.inf
    return r


class Outputs:
    def __init__(self, n):
        import torch
        from test_wavefront_items import full_items
        from nn_bvh_amd.wavefront import HostCandidateArrays, WorkQueue
        dev = dev0()
        self.queues = {k: WorkQueue(n, dev) for k in QUEUES}
        self.items = full_items(n, dev)
        self.needs_host = WorkQueue(n, dev)
        self.hits = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
        self.cands = HostCandidateArrays(n, K, dev)

    def sets(self):
        return {k: np.sort(q.indices().cpu().numpy()) for k, q in self.queues.items()}

    def hit_records(self):
        return self.hits.cpu().numpy().view(HIT_DTYPE).reshape(-1)

    def slices_by_ray(self, name):
        """{ray index: slot} of queue `name` and its slice tensors on the host."""
        q = self.queues[name]
        k = min(q.Size(), q.capacity)
        idx = q.items[:k].cpu().numpy()
        return idx, {f: t.cpu().numpy()[..., :k] for f, t in self.items[name].fields.items()}


def assert_slices_equal(a, b, name, rows, what):
    """Queue `name` of Outputs a and b carries bit-equal item slices for the rays `rows` (present in both)."""
    ia, fa = a.slices_by_ray(name)
    ib, fb = b.slices_by_ray(name)
    sa, sb = np.argsort(ia), np.argsort(ib)
    pa = sa[np.searchsorted(ia[sa], rows)]
    pb = sb[np.searchsorted(ib[sb], rows)]
    assert np.array_equal(ia[pa], rows) and np.array_equal(ib[pb], rows), f"{what}: {name} lacks some of the rays"
    for f in fa:
        x, y = fa[f][..., pa], fb[f][..., pb]
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), f"{what}: {name}.{f}"


def class_table(n_ids, seed=5):
    return np.random.default_rng(seed).choice(np.array([0, 1, 2, 4, 5, 6], np.uint8), n_ids)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_wavefront_routing_and_closest_end_to_end(name):
    import torch
    from nn_bvh_amd.wavefront import WavefrontAggregate, WorkQueue, enqueue_closest_items
    case = Case(name)
    rays, n = case.rays, len(case.rays)
    prim_class = class_table(len(case.is_host))
    wf = WavefrontAggregate(case.agg, prim_class)
    rq = ray_queue(rays)
    plain = Outputs(n)
    wf.IntersectClosestItems(n, rq, case.mesh, items=plain.items, needs_host=plain.needs_host, hits=plain.hits,
                             **plain.queues)
    got = Outputs(n)
    wf.IntersectClosestItemsWithCandidates(n, rq, case.mesh, got.cands, got.hits, items=got.items,
                                           needs_host=got.needs_host, **got.queues)
    torch.cuda.synchronize()
    # -- routing: the six queues as sets, needs_host, records and candidate arrays
    cands = got.cands.numpy()
    cnt = cands["count"]
    print(f"{name}: count > 0 on {(cnt > 0).mean():.4f} of the rays, count < 0 on {(cnt < 0).mean():.5f}")
    assert (cnt < 0).mean() <= 0.01 and (cnt > 0).mean() > 0.05
    ps, gs = plain.sets(), got.sets()
    for k in QUEUES:
        assert np.array_equal(ps[k], gs[k]), k
    assert np.array_equal(np.sort(got.needs_host.indices().cpu().numpy()), np.nonzero(cnt != 0)[0])
    assert np.array_equal(plain.hit_records()["instance"] == -1, cnt != 0)
    ref_hits, ref_c = single_batch_reference(case.agg, gathered(rays), "closest")
    assert got.hits.cpu().numpy().tobytes() == ref_hits.tobytes()
    assert_cands_equal((cnt, cands["before"], cands["prim"], cands["instance"]), ref_c, True, name)
    for k in _lib.ITEM_QUEUES:
        assert_slices_equal(got, plain, k, gs[k], f"{name} count == 0 rays")
    # -- end to end: resolve needs_host, write the merged records back, enqueue those rays only
    hits = got.hit_records()
    todo = got.needs_host.indices().cpu().numpy()
    res = case.oracle(resolve_host_candidates, gathered(rays), hits, cands, case.callback(gathered(rays)),
                      np.zeros(len(case.is_host), np.int32))
    merged = hits.copy()
    merged[todo] = res[todo]
    got.hits.copy_(upload(merged))
    fresh = WorkQueue(n, dev0())
    enqueue_closest_items(case.mesh, n, rq, got.hits, prim_class=wf.prim_class, items=got.items, needs_host=fresh,
                          index=got.needs_host, **got.queues)
    torch.cuda.synchronize()
    ok = cnt >= 0
    exp_hits = case.oracle(case.oracle_closest, gathered(rays))
    exp_q = ob.wavefront_enqueue_closest(exp_hits, None, prim_class)
    union = got.sets()
    for k, e in zip(QUEUES, exp_q):
        assert np.array_equal(union[k], np.sort(e[ok[e]])), f"{name}: union of both enqueues, {k}"
    assert np.array_equal(np.sort(fresh.indices().cpu().numpy()), np.nonzero(~ok)[0])
    # the items of host-declared triangles: what the plain call gives on the all-triangle scene
    tri_agg = BVHAggregate.from_tree(**case.tri_args)
    tri = Outputs(n)
    WavefrontAggregate(tri_agg, prim_class).IntersectClosestItems(n, rq, case.mesh, items=tri.items,
                                                                  needs_host=tri.needs_host, hits=tri.hits,
                                                                  **tri.queues)
    torch.cuda.synchronize()
    assert tri.needs_host.Size() == 0
    won_by_host = (res["prim"] >= 0) & case.is_host[np.maximum(res["prim"], 0)] & ok
    assert won_by_host.any()
    for k in _lib.ITEM_QUEUES:
        assert_slices_equal(got, tri, k, union[k], f"{name} after the indexed enqueue")
    in_items = np.concatenate([union[k] for k in _lib.ITEM_QUEUES])
    assert np.isin(np.nonzero(won_by_host)[0], in_items).any()  # host-declared triangles do carry items
    tri_agg.close()
    case.close()


def shadow_setup(case):
    from test_wavefront import shadow_inputs
    srays = case.rays.copy()
    srays["tmax"] = np.float32(1 - 1e-4)
    n = len(srays)
    Ld, r_u, r_l, px, L = shadow_inputs(n, n + 5000, 7)
    assert len(np.unique(px)) == n  # distinct pixel indices
    return srays, Ld, r_u, r_l, px, L


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_wavefront_shadow_end_to_end(name):
    import torch
    from nn_bvh_amd.wavefront import HostCandidateArrays, WavefrontAggregate, record_shadow
    case = Case(name)
    srays, Ld, r_u, r_l, px, L = shadow_setup(case)
    n = len(srays)
    t = lambda a: torch.from_numpy(a).to(dev0())  # noqa: E731
    wf = WavefrontAggregate(case.agg)
    sq = ray_queue(srays, shadow=True)
    d_Ld, d_ru, d_rl, d_px, d_L = t(Ld), t(r_u), t(r_l), t(px), t(L)
    occ = torch.full((n,), 9, dtype=torch.uint8, device=dev0())
    sc = HostCandidateArrays(n, K, dev0())
    wf.IntersectShadowWithCandidates(n, sq, d_Ld, d_ru, d_rl, d_px, d_L, occ, sc)
    torch.cuda.synchronize()
    ref_occ, ref_c = single_batch_reference(case.agg, srays, "any")
    h_occ, cands = occ.cpu().numpy(), sc.numpy()
    assert np.array_equal(h_occ, ref_occ)
    assert_cands_equal((cands["count"], None, cands["prim"], cands["instance"]), ref_c, False, name)
    assert (cands["before"] == 0).all()
    # so far exactly the rays with occluded 0 have been recorded
    first = ob.record_shadow(np.where(h_occ == 0, 0, 1), Ld, r_u, r_l, px, L)
    assert np.array_equal(d_L.cpu().numpy().view(np.uint32), first.view(np.uint32))
    res = case.oracle(resolve_host_candidates_any, srays, h_occ, cands, case.callback(srays))
    assert ((h_occ == 2) & (res == 0)).any() and ((h_occ == 2) & (res == 1)).any()  # both outcomes occur
    second = np.where((h_occ == 2) & (res == 0), 0, 1).astype(np.uint8)
    record_shadow(n, sq, t(second), d_Ld, d_ru, d_rl, d_px, d_L)
    torch.cuda.synchronize()
    exp_occ = case.oracle(case.oracle_any, srays)
    void = res == 2
    assert void.mean() <= 0.01
    expected = ob.record_shadow(np.where(void, 1, exp_occ), Ld, r_u, r_l, px, L)  # void rays: removed from both sides
    assert np.array_equal(d_L.cpu().numpy().view(np.uint32), expected.view(np.uint32))
    case.close()


def one_launch_against_two_calls(agg, mesh, rays, srays, prim_class, what):
    import torch
    from test_wavefront import shadow_inputs
    from nn_bvh_amd.wavefront import HostCandidateArrays, WavefrontAggregate
    n, ns = len(rays), len(srays)
    Ld, r_u, r_l, px, L = shadow_inputs(ns, ns + 500, 7)
    t = lambda a: torch.from_numpy(a).to(dev0())  # noqa: E731
    wf = WavefrontAggregate(agg, prim_class)
    rq, sq = ray_queue(rays), ray_queue(srays, shadow=True)
    two, L2 = Outputs(n), t(L)
    occ2 = torch.full((ns,), 9, dtype=torch.uint8, device=dev0())
    sc2 = HostCandidateArrays(ns, K, dev0())
    wf.IntersectShadowWithCandidates(ns, sq, t(Ld), t(r_u), t(r_l), t(px), L2, occ2, sc2)
    wf.IntersectClosestItemsWithCandidates(n, rq, mesh, two.cands, two.hits, items=two.items,
                                           needs_host=two.needs_host, **two.queues)
    one, L1 = Outputs(n), t(L)
    occ1 = torch.full((ns,), 9, dtype=torch.uint8, device=dev0())
    sc1 = HostCandidateArrays(ns, K, dev0())
    wf.IntersectClosestAndShadowItemsWithCandidates(n, rq, mesh, one.cands, one.hits, ns, sq, t(Ld), t(r_u), t(r_l),
                                                    t(px), L1, occ1, sc1, items=one.items,
                                                    needs_host=one.needs_host, **one.queues)
    torch.cuda.synchronize()
    assert torch.equal(one.hits, two.hits) and torch.equal(occ1, occ2), what
    assert np.array_equal(L1.cpu().numpy().view(np.uint32), L2.cpu().numpy().view(np.uint32)), what
    for a, b, closest in ((one.cands.numpy(), two.cands.numpy(), True), (sc1.numpy(), sc2.numpy(), False)):
        assert_cands_equal((a["count"], a["before"], a["prim"], a["instance"]),
                           (b["count"], b["before"], b["prim"], b["instance"]), closest, what)
    s1, s2 = one.sets(), two.sets()
    for k in QUEUES:
        assert np.array_equal(s1[k], s2[k]), (what, k)
    assert np.array_equal(np.sort(one.needs_host.indices().cpu().numpy()),
                          np.sort(two.needs_host.indices().cpu().numpy())), what
    for k in _lib.ITEM_QUEUES:
        assert_slices_equal(one, two, k, s1[k], what)
    return one, occ1.cpu().numpy(), sc1.numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", SCENES)
def test_one_launch_equals_the_two_candidate_calls(name):
    case = Case(name, 9000)
    srays = case.rays[:6000].copy()
    srays["tmax"] = np.float32(1 - 1e-4)
    one, occ, sc = one_launch_against_two_calls(case.agg, case.mesh, case.rays, srays, class_table(len(case.is_host)),
                                                name)
    assert (one.cands.numpy()["count"] > 0).any() and (occ == 2).any()
    case.close()


@pytest.mark.gpu
def test_one_launch_falls_back_on_an_alpha_tested_scene():
    from nn_bvh_amd import build_tree
    from nn_bvh_amd.interaction import ShadingMesh
    from test_alpha import alpha_scene
    verts, prims, alpha, kinds = alpha_scene(9, 800)
    tree = build_tree(prims, verts)
    agg = BVHAggregate.from_tree(tree.nodes, tree.ordered_prims, verts)
    mesh = ShadingMesh(verts, tri_table(prims))
    rays = scene.random_rays(6000, verts.min(0) - 1, verts.max(0) + 1, 11)
    srays = scene.random_rays(5000, verts.min(0) - 1, verts.max(0) + 1, 12, tmax=np.float32(1 - 1e-4))
    one, occ, sc = one_launch_against_two_calls(agg, mesh, rays, srays, class_table(len(prims)), "alpha")
    cnt = one.cands.numpy()["count"]
    assert np.isin(cnt, (0, -2)).all() and np.isin(sc["count"], (0, -2)).all()
    plain = agg.Intersect(gathered(rays))
    assert one.hit_records().tobytes() == plain.tobytes()  # no host-only primitives: the plain records
    agg.close()
    mesh.close()


@pytest.mark.gpu
def test_scene_without_host_primitives_runs_the_plain_calls():
    import torch
    from test_wavefront_items import soup_setup
    from test_wavefront import shadow_inputs
    from nn_bvh_amd.wavefront import HostCandidateArrays, WavefrontAggregate
    n, ns = 7001, 6000
    verts, prims, mesh, agg, rays = soup_setup(51, n)
    srays = scene.random_rays(ns, verts.min(0) - 3, verts.max(0) + 3, 77, tmax=np.float32(1 - 1e-4))
    srays["d"] *= np.float32(12.0)
    prim_class = class_table(len(prims))
    Ld, r_u, r_l, px, L = shadow_inputs(ns, 9000, 7)
    t = lambda a: torch.from_numpy(a).to(dev0())  # noqa: E731
    wf = WavefrontAggregate(agg, prim_class)
    rq, sq = ray_queue(rays), ray_queue(srays, shadow=True)
    plain, Lp = Outputs(n), t(L)
    occp = torch.full((ns,), 9, dtype=torch.uint8, device=dev0())
    wf.IntersectClosestAndShadowItems(n, rq, mesh, ns, sq, t(Ld), t(r_u), t(r_l), t(px), Lp, items=plain.items,
                                      needs_host=plain.needs_host, hits=plain.hits, occluded=occp, **plain.queues)
    for form in ("one", "two"):
        got, Lg = Outputs(n), t(L)
        got.cands.count.fill_(55)
        got.cands.before.fill_(55)
        occg = torch.full((ns,), 9, dtype=torch.uint8, device=dev0())
        sc = HostCandidateArrays(ns, K, dev0())
        sc.count.fill_(55)
        if form == "one":
            wf.IntersectClosestAndShadowItemsWithCandidates(n, rq, mesh, got.cands, got.hits, ns, sq, t(Ld), t(r_u),
                                                            t(r_l), t(px), Lg, occg, sc, items=got.items,
                                                            needs_host=got.needs_host, **got.queues)
        else:
            wf.IntersectShadowWithCandidates(ns, sq, t(Ld), t(r_u), t(r_l), t(px), Lg, occg, sc)
            wf.IntersectClosestItemsWithCandidates(n, rq, mesh, got.cands, got.hits, items=got.items,
                                                   needs_host=got.needs_host, **got.queues)
        torch.cuda.synchronize()
        assert torch.equal(got.hits, plain.hits) and torch.equal(occg, occp) and torch.equal(Lg, Lp), form
        assert (got.cands.count == 0).all() and (got.cands.before == 0).all() and (sc.count == 0).all(), form
        gs, ps = got.sets(), plain.sets()
        for k in QUEUES:
            assert np.array_equal(gs[k], ps[k]), (form, k)
        assert got.needs_host.Size() == plain.needs_host.Size() == 0
        for k in _lib.ITEM_QUEUES:
            assert_slices_equal(got, plain, k, gs[k], form)
    # batches: the plain call's bytes and zero counts
    d_rays, d_srays = upload(gathered(rays)), upload(srays)
    h1 = torch.zeros((n, 32), dtype=torch.uint8, device=dev0())
    o1 = torch.zeros(ns, dtype=torch.uint8, device=dev0())
    c1, c2 = DevCands(n), DevCands(ns)
    agg.trace_batches_candidates_device([("closest", d_rays.data_ptr(), n, h1.data_ptr()),
                                         ("any", d_srays.data_ptr(), ns, o1.data_ptr())],
                                        [c1.tup(True), c2.tup(False)], stream0())
    torch.cuda.synchronize()
    assert torch.equal(h1, plain.hits) and torch.equal(o1, occp)
    assert (c1.count == 0).all() and (c1.before == 0).all() and (c2.count == 0).all()
    agg.close()
    mesh.close()


@pytest.mark.gpu
def test_wavefront_bad_arguments_launch_nothing():
    import torch
    from nn_bvh_amd.wavefront import HostCandidateArrays, WavefrontAggregate, _items_record, _queues_record
    case = Case("flat", 2000)
    n = len(case.rays)
    rq, sq = ray_queue(case.rays), ray_queue(case.rays, shadow=True)
    out = Outputs(n)
    out.hits.fill_(0x5a)
    out.cands.count.fill_(77)
    soa, ssoa = rq._wire(), sq._wire()
    qrec, irec = _queues_record(out.queues), _items_record(out.items, out.needs_host)
    L = _lib.lib()
    ptr, st = _lib.ptr, stream0()
    good = out.cands._wire()
    no_before = _lib.HostCandidates(K, good.count, None, good.prim, good.instance)
    zero_cap = _lib.HostCandidates(0, good.count, good.before, good.prim, good.instance)
    f4 = torch.zeros((n, 4), dtype=torch.float32, device=dev0())
    px = torch.arange(n, dtype=torch.int32, device=dev0())
    occ = torch.full((n,), 9, dtype=torch.uint8, device=dev0())
    h = case.agg._h

    def closest(hits_ptr, c):
        return L.nnbvh_wavefront_intersect_closest_items_candidates(
            h, case.mesh._h, n, ptr(soa), rq.size.data_ptr(), None, 0, hits_ptr, ptr(qrec), ptr(irec),
            ctypes.byref(c) if c is not None else None, st)

    def shadow(occ_ptr, c):
        return L.nnbvh_wavefront_intersect_shadow_candidates(
            h, n, ptr(ssoa), sq.size.data_ptr(), f4.data_ptr(), f4.data_ptr(), f4.data_ptr(), px.data_ptr(),
            f4.data_ptr(), n, occ_ptr, ctypes.byref(c) if c is not None else None, st)

    assert closest(None, good) == ERR_ARG and closest(out.hits.data_ptr(), None) == ERR_ARG
    assert closest(out.hits.data_ptr(), no_before) == ERR_ARG and closest(out.hits.data_ptr(), zero_cap) == ERR_ARG
    assert shadow(None, good) == ERR_ARG and shadow(occ.data_ptr(), zero_cap) == ERR_ARG
    assert L.nnbvh_wavefront_intersect_closest_and_shadow_items_candidates(
        h, case.mesh._h, n, ptr(soa), rq.size.data_ptr(), None, 0, out.hits.data_ptr(), ptr(qrec), ptr(irec),
        ctypes.byref(good), n, ptr(ssoa), sq.size.data_ptr(), f4.data_ptr(), f4.data_ptr(), f4.data_ptr(),
        px.data_ptr(), f4.data_ptr(), n, None, ctypes.byref(good), st) == ERR_ARG
    assert L.nnbvh_wavefront_enqueue_closest_items_indexed_device(
        case.mesh._h, n, ptr(soa), None, None, n, out.hits.data_ptr(), None, 0, ptr(qrec), ptr(irec), st) == ERR_ARG
    torch.cuda.synchronize()
    assert (out.hits == 0x5a).all() and (out.cands.count == 77).all() and (occ == 9).all() and (f4 == 0).all()
    assert all(q.Size() == 0 for q in out.queues.values()) and out.needs_host.Size() == 0
    # index entries outside [0, max_rays) are skipped; all item slices NULL gives index queues only
    WavefrontAggregate(case.agg).IntersectClosestItemsWithCandidates(n, rq, case.mesh, out.cands, out.hits,
                                                                      needs_host=out.needs_host, **out.queues)
    torch.cuda.synchronize()
    total = sum(q.Size() for q in out.queues.values()) + out.needs_host.Size()
    assert total >= n and (out.cands.count != 77).all()
    case.close()


@pytest.mark.gpu
def test_cpp_adapter_wavefront_candidates(nnbvh_lib):
    src = os.path.join(ROOT, "tests", "cpp", "wavefront_candidates_check.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "wavefront_candidates_check")
    libdir = os.path.join(ROOT, "nn_bvh_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    "-I", "/opt/rocm/include", "-D__HIP_PLATFORM_AMD__", src, "-o", exe, "-pthread", "-L", libdir,
                    "-l:libnnbvh_hip.so", f"-Wl,-rpath,{libdir}", "-L", "/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath,/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "wavefront candidates ok" in out.stdout
