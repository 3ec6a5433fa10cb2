"""The top table of a lean scene: the first 63 interior records, breadth-first from the root, which the lean one-launch
kernels (trace_kernel<3, 8, 0, 0> and its SOA twin, bvh_trace.hip) copy into LDS and read instead of the baked array.

Inside the copies a reference to another copied record is tagged (bit 30 | table slot, nn_bvh_amd/csrc/top_table.h); the
walk enters at the tagged root, and tagged references pass through the LDS stack window and its HBM spill unchanged.
The copies are byte copies, so every result must stay what it was: each GPU case compares the one-launch call bit for
bit with the oracle (records with their counts, occlusion flags), with the separate mode-0 and mode-2 launches of the
same rays, which read the baked array only, and with the one-launch call with the table switched off
(option "top_table" 0).  The CPU case runs the table builder on hand-made trees (tests/cpp/top_table_check.cpp)."""
import os
import subprocess

import numpy as np
import pytest

import oracle_binding as ob
import scenes_small as ss
from nn_bvh_amd import HIT_DTYPE, RAY_DTYPE, BVHAggregate, build_tree, scene

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 63  # kTopRecords


def ray_mix(lo, hi, n, seed):
    """Seeded rays for a scene with bounds [lo, hi]: incoherent rays between points of the slightly larger box (most
    start inside the root's box, hence inside the boxes of the top records), rays from inside with a finite tMax, and
    rays that miss the root (they start beyond `hi` and point away)."""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    n_in, n_miss = n // 6, n // 8
    through = scene.random_rays(n - n_in - n_miss, lo - 1, hi + 1, seed + 1)
    inside = np.zeros(n_in, RAY_DTYPE)
    inside["o"] = (lo + rng.random((n_in, 3)) * (hi - lo)).astype(np.float32)
    inside["d"] = rng.standard_normal((n_in, 3)).astype(np.float32)
    inside["tmax"] = rng.uniform(0.5, 8.0, n_in).astype(np.float32)
    miss = np.zeros(n_miss, RAY_DTYPE)
    miss["o"] = (hi + 1 + 4 * rng.random((n_miss, 3))).astype(np.float32)
    miss["d"] = (0.1 + rng.random((n_miss, 3))).astype(np.float32)
    miss["tmax"] = np.inf
    rays = np.concatenate([through, inside, miss])
    return rays[rng.permutation(len(rays))]


def upload(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def one_launch(agg, any_rays, closest_batches):
    """One trace_batches_device call: an any-hit batch, then the closest-hit batches -> (flags, [records, ...])"""
    import torch
    d_any = upload(any_rays)
    o_any = torch.full((len(any_rays),), 0x5A, dtype=torch.uint8, device="cuda")
    d_cl = [upload(r) for r in closest_batches]
    o_cl = [torch.full((len(r) * 32,), 0x5A, dtype=torch.uint8, device="cuda") for r in closest_batches]
    agg.trace_batches_device([("any", d_any.data_ptr(), len(any_rays), o_any.data_ptr())] +
                             [("closest", d.data_ptr(), len(r), o.data_ptr()) for d, r, o in zip(d_cl, closest_batches, o_cl)],
                             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return o_any.cpu().numpy(), [o.cpu().numpy().view(HIT_DTYPE) for o in o_cl]


def check_scene(tree, verts, any_rays, closest_batches, what, n_table):
    """The four-batch launch against the oracle, the separate launches and the launch without the table."""
    exp_any = ob.any_hit(tree.nodes, tree.ordered_prims, verts, any_rays)[0]
    exp = [ob.closest(tree.nodes, tree.ordered_prims, verts, r) for r in closest_batches]
    agg = BVHAggregate.from_tree(tree.nodes, tree.ordered_prims, verts)
    try:
        # the scene holds its table: the baked arrays and n_table records more
        info = agg.info
        assert info["device_bytes"] == max(info["interior_records"], 1) * 64 + max(info["prim_slots"], 1) * 16 + n_table * 64, \
            f"{what}: the scene's top table should hold {n_table} records"
        for table in (1, 0):
            agg.set_option("top_table", table)
            flags, recs = one_launch(agg, any_rays, closest_batches)
            assert np.array_equal(flags, exp_any), f"{what}: any batch, top_table {table}"
            for b, (got, want) in enumerate(zip(recs, exp)):
                assert got.tobytes() == want.tobytes(), f"{what}: closest batch {b}, top_table {table}"
        agg.set_option("top_table", 1)
        # the mode-0 and mode-2 lean launches read the baked array only
        for b, (r, want) in enumerate(zip(closest_batches, exp)):
            assert agg.Intersect(r).tobytes() == want.tobytes(), f"{what}: mode-0 launch of batch {b}"
        assert np.array_equal(agg.IntersectP(any_rays), exp_any), f"{what}: mode-2 launch"
    finally:
        agg.close()


@gpu
@pytest.mark.parametrize("n_tris,max_prims,interior", [(50, 4, "below"), (72, 4, "above"), (1, 4, "none"), (2, 1, "one")],
                         ids=["below-K", "above-K", "one-leaf", "two-triangles"])
def test_interior_count_on_either_side_of_k(n_tris, max_prims, interior):
    """Fewer interior records than K: the whole tree is in LDS.  A few more: copied records have leaf, copied and
    not-copied children.  A root that is a leaf has no table; two leaves under one record have a table of one."""
    verts, prims = ss.random_soup(n_tris, seed=31)
    tree = build_tree(prims, verts, max_prims_in_node=max_prims)
    n_int = int((tree.nodes["nprims"] == 0).sum())
    assert {"below": 30 < n_int < K, "above": K < n_int <= K + 12, "none": n_int == 0, "one": n_int == 1}[interior], n_int
    lo, hi = verts.min(0), verts.max(0)
    rays = [ray_mix(lo, hi, 3000, 40 + k) for k in range(4)]
    check_scene(tree, verts, rays[0], rays[1:], f"{n_tris} triangles", min(n_int, K))


@gpu
def test_mixed_launch():
    """About 20 000 seeded rays per batch through one four-batch launch (any, closest, closest, closest) on a soup of
    10 000 triangles: rays that start inside the top boxes, rays that miss the root."""
    verts, prims = ss.random_soup(10000, seed=32)
    tree = build_tree(prims, verts)
    lo, hi = verts.min(0), verts.max(0)
    rays = [ray_mix(lo, hi, 20000 + 37 * k, 50 + k) for k in range(4)]
    check_scene(tree, verts, rays[0], rays[1:], "10 000 triangles", K)


@gpu
def test_spilled_tagged_references():
    """The deep-chain scene of test_stack_limits: every deep ray holds 64 pending entries, so references of the chain's
    first 63 records (all of them in the table, hence tagged) are spilled to the HBM array and popped back."""
    from test_stack_limits import assert_exceeds_window, bvh_ray_set, oracle_single
    ch = ss.chain_tree(64, np.random.default_rng(21), tube=True, leaves="tri", extras=True)
    rays, deep = bvh_ray_set(ch.leaf_lo, ch.leaf_hi, 24)
    exp, eany, dc, da = oracle_single(ch, rays)
    assert_exceeds_window(dc, deep, 8, "closest")
    assert_exceeds_window(da, deep, 8, "any")
    agg = BVHAggregate.from_tree(ch.nodes, ch.prims, ch.verts)
    try:
        assert agg.info["depth"] == 64 and agg.info["interior_records"] >= K
        flags, (recs, recs2) = one_launch(agg, rays[::-1].copy(), [rays, rays[::2].copy()])
        assert recs.tobytes() == exp.tobytes(), "closest batch against the oracle"
        assert recs2.tobytes() == exp[::2].tobytes(), "second closest batch against the oracle"
        assert np.array_equal(flags, eany[0][::-1]), "any batch against the oracle"
        assert agg.Intersect(rays).tobytes() == recs.tobytes(), "the mode-0 launch"
        assert np.array_equal(agg.IntersectP(rays), eany[0]), "the mode-2 launch"
    finally:
        agg.close()


@gpu
def test_soa_twin():
    """IntersectClosestAndShadow on queues: the SOA twin <3, 8, 0, 0, 0, 1> reads the slices itself and walks from the
    same table.  Device-side queue sizes below the capacity."""
    import torch
    from nn_bvh_amd.wavefront import RayQueue, WavefrontAggregate
    from test_wavefront import shadow_inputs
    verts, prims = ss.random_soup(72, seed=31)
    tree = build_tree(prims, verts)
    rays = ray_mix(verts.min(0), verts.max(0), 4000, 60)
    cap, n = len(rays), len(rays) - 137
    q = rays[:n].copy()
    q["tmax"] = np.inf  # a closest queue carries no tMax
    exp = ob.closest(tree.nodes, tree.ordered_prims, verts, q)
    eocc = ob.any_hit(tree.nodes, tree.ordered_prims, verts, rays[:n])[0]
    Ld, r_u, r_l, px, L = shadow_inputs(cap, cap + 500, 7)
    exp_l = ob.record_shadow(eocc, Ld[:n], r_u[:n], r_l[:n], px[:n], L)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    agg = BVHAggregate.from_tree(tree.nodes, tree.ordered_prims, verts)
    try:
        wf = WavefrontAggregate(agg)
        rq, sq = RayQueue.from_records(rays, dev), RayQueue.from_records(rays, dev, shadow=True)
        rq.size.fill_(n)
        sq.size.fill_(n)
        for table in (1, 0):
            agg.set_option("top_table", table)
            hits_t = torch.full((cap, 32), 0xAB, dtype=torch.uint8, device=dev)
            occ_t = torch.full((cap,), 9, dtype=torch.uint8, device=dev)
            l_t = t(L)
            wf.IntersectClosestAndShadow(cap, rq, cap, sq, t(Ld), t(r_u), t(r_l), t(px), l_t, hits=hits_t, occluded=occ_t)
            torch.cuda.synchronize()
            hits, occ = hits_t.cpu().numpy(), occ_t.cpu().numpy()
            assert hits[:n].tobytes() == exp.tobytes(), f"hit records, top_table {table}"
            assert (hits[n:] == 0xAB).all() and (occ[n:] == 9).all(), f"wrote beyond the size, top_table {table}"
            assert np.array_equal(occ[:n], eocc), f"occlusion flags, top_table {table}"
            assert np.array_equal(l_t.cpu().numpy().view(np.uint32), exp_l.view(np.uint32)), f"radiance, top_table {table}"
    finally:
        agg.close()


# ---- CPU: the table builder -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [[], ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan-ubsan"])
def test_table_builder_on_hand_made_trees(tmp_path, flags):
    """Every tagged slot holds the byte copy of the record it replaces; no reference in `wide` changed; the slots are the
    first records breadth-first; exactly the references to copied records are tagged."""
    exe = tmp_path / "top_table_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + flags +
                   [os.path.join(ROOT, "tests", "cpp", "top_table_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and not out.stderr, out.stdout[-2000:] + out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert len(lines) == 12 and not any("FAILED" in ln for ln in lines), out.stdout
    assert lines[0] == "leaf root: records 0 slots 0 tagged 0 leaf 0 outside 0"
    assert lines[1] == "one record: records 1 slots 1 tagged 0 leaf 2 outside 0"
    assert lines[3] == "full 63: records 63 slots 63 tagged 62 leaf 64 outside 0"
    assert all(" slots 63 tagged 62 " in ln and " outside 0" not in ln for ln in lines[4:10])
