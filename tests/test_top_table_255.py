"""The LDS top table of the lean one-launch kernels at 1024 threads per block: each block copies the scene's 63 records
and extends its copy to 255 from the baked array itself, generation by generation (nn_bvh_amd/csrc/top_extend.h).

CPU: the slot assignment the prologue runs, on hand-made trees (tests/cpp/top_extend_check.cpp), plain and under
ASan/UBSan.  GPU: the table a block really holds (a debug kernel that runs the prologue alone) against the host's run of
the same assignment, byte for byte; the results of the one-launch call, which no table may change, bit for bit against
the oracle, the separate launches and the call without a table (check_scene of test_top_table) at top_burst 1, 24 and 65;
batch sizes around the wave and the block, grids of 1, 4 and 8 units of 256 lanes per CU, the SOA twin; and the spill
array under the largest grid of 1024-thread blocks."""
import ctypes
import functools
import os
import subprocess
import types

import numpy as np
import pytest

import oracle_binding as ob
import scenes_small as ss
import test_top_table
from nn_bvh_amd import BVHAggregate, _lib, build_tree
from test_top_table import K, check_scene, one_launch, ray_mix

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPACITY = 255  # top_lds_records(1024)
NODE = np.dtype([("q", "<f4", 12), ("ref", "<i4", 2), ("axis", "<i4"), ("pad", "<i4")])  # WideNode
TAG = 1 << 30


# ---- CPU: the slot assignment ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [[], ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan-ubsan"])
def test_extension_on_hand_made_trees(tmp_path, flags):
    """Parent-closed, byte copies behind every tagged reference, nothing fetched through a tagged reference, the first
    records breadth-first up to the capacity: checked by the program, which prints one line per case."""
    exe = tmp_path / "top_extend_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + flags +
                   [os.path.join(ROOT, "tests", "cpp", "top_extend_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and not out.stderr, out.stdout[-2000:] + out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert len(lines) == 37 and not any("FAILED" in ln for ln in lines), out.stdout
    by_name = {ln.split(":")[0]: ln.split(": ")[1] for ln in lines}
    assert by_name["random 50, capacity 255"] == "records 50 slots 50 tagged 49 leaf 51 outside 0"
    assert by_name["balanced 64..75, capacity 255"] == "records 75 slots 75 tagged 74 leaf 76 outside 0"  # (the last of them)
    assert by_name["balanced 150, capacity 255"] == "records 150 slots 150 tagged 149 leaf 151 outside 0"
    assert by_name["balanced 300, capacity 255"] == "records 300 slots 255 tagged 254 leaf 211 outside 45"
    assert by_name["balanced 300, capacity 127"] == "records 300 slots 127 tagged 126 leaf 0 outside 128"
    assert by_name["chain 200, capacity 255"] == "records 200 slots 200 tagged 199 leaf 201 outside 0"
    assert by_name["chain 300, capacity 255"] == "records 300 slots 255 tagged 254 leaf 255 outside 1"
    assert by_name["random 600, capacity 10"].startswith("records 600 slots 63 ")  # never below the scene's table
    assert " slots 255 tagged 254 " in by_name["leaf children at level 5, capacity 255"]


# ---- GPU scenes -----------------------------------------------------------------------------------------------------
SCENES = ("soup-72", "soup-150", "soup-300", "soup-10000", "chain-64")


@functools.lru_cache(maxsize=None)
def scene_case(name):
    """(tree with .nodes / .ordered_prims, verts, interior records, four batches of about 3 000 rays)"""
    kind, n = name.split("-")
    if kind == "soup":
        verts, prims = ss.random_soup(int(n), seed=31 if n == "72" else 33)
        tree = build_tree(prims, verts, max_prims_in_node=4)
        rays = [ray_mix(verts.min(0), verts.max(0), 3000, 70 + k) for k in range(4)]
    else:
        from test_stack_limits import bvh_ray_set
        ch = ss.chain_tree(int(n), np.random.default_rng(21), tube=True, leaves="tri", extras=True)
        tree, verts = types.SimpleNamespace(nodes=ch.nodes, ordered_prims=ch.prims), ch.verts
        # deep chain rays (64 pending entries: tagged references of all 64 records go through the spill) and random ones
        rays = [bvh_ray_set(ch.leaf_lo, ch.leaf_hi, 80 + k, n_deep=1500, n_random=1500)[0] for k in range(4)]
    return tree, verts, int((tree.nodes["nprims"] == 0).sum()), rays


def debug_tables(agg, blocks):
    """nnbvh_debug_top_table (bvh_capi.cpp, not in the public header) -> (per-block tables, per-block counts, the host's
    table)"""
    fn = _lib.lib().nnbvh_debug_top_table
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 5
    dev = np.full((blocks, CAPACITY), 0x5A, np.uint8).repeat(64, 1).view(NODE)
    counts = np.full(blocks, -1, np.int32)
    host = np.zeros(CAPACITY, NODE)
    n_host, cap = ctypes.c_int32(-1), ctypes.c_int32(-1)
    _lib.check(fn(agg._h, blocks, _lib.ptr(dev), _lib.ptr(counts), _lib.ptr(host), ctypes.byref(n_host),
                  ctypes.byref(cap)), "nnbvh_debug_top_table")
    assert cap.value == CAPACITY
    return dev, counts, host[:n_host.value]


@gpu
@pytest.mark.parametrize("name", SCENES)
def test_block_table_is_the_host_table(name):
    """Every block of a small grid holds, byte for byte, the table the host's run of the slot assignment gives: all the
    scene's interior records up to 255 of them, every one a byte copy of its record of the baked array but for tagged
    references, each of which names the slot of the record it replaced."""
    tree, verts, n_int, _ = scene_case(name)
    agg = BVHAggregate.from_tree(tree.nodes, tree.ordered_prims, verts)
    try:
        dev, counts, host = debug_tables(agg, 5)
        assert len(host) == min(n_int, CAPACITY) and len(host) > K, f"{n_int} interior records: the extension is missing"
        assert (counts == len(host)).all(), counts
        for b in range(len(counts)):
            assert dev[b, :len(host)].tobytes() == host.tobytes(), f"block {b}"
        # ... and that table against the baked array itself, read back from the device
        wide = np.zeros(n_int, NODE)
        _lib.check(_lib.lib().nnbvh_scene_read(agg._h, 0, _lib.ptr(wide), wide.nbytes), "nnbvh_scene_read")
        assert not ((wide["ref"] >= 0) & (wide["ref"] & TAG != 0)).any()
        record_of = np.full(len(host), -1)
        record_of[0] = 0  # the root is the bake's first record
        for k in range(len(host)):  # parents come before their children
            assert record_of[k] >= 0, f"slot {k} is named by no tagged reference"
            w = wide[record_of[k]]
            assert host[k]["q"].tobytes() == w["q"].tobytes() and host[k]["axis"] == w["axis"], f"slot {k} is no copy"
            for c in range(2):
                ref = int(host[k]["ref"][c])
                if ref >= 0 and ref & TAG:
                    slot = ref & (TAG - 1)
                    assert k < slot < len(host) and record_of[slot] < 0, f"slot {k} child {c}"
                    record_of[slot] = int(w["ref"][c])
                else:
                    assert ref == int(w["ref"][c]), f"slot {k} child {c} changed"
        assert len(set(record_of.tolist())) == len(host)
    finally:
        agg.close()


class AggregateAtBurst:
    """BVHAggregate for check_scene: every scene it creates runs at a given top_burst"""
    burst = 24

    @classmethod
    def from_tree(cls, *args, **kwargs):
        agg = BVHAggregate.from_tree(*args, **kwargs)
        agg.set_option("top_burst", cls.burst)
        return agg


@gpu
@pytest.mark.parametrize("burst", (1, 24, 65))
@pytest.mark.parametrize("name", SCENES)
def test_results_with_the_extended_table(name, burst, monkeypatch):
    """One four-batch launch (any + three closest) bit for bit against the oracle, the mode-0 / mode-2 launches and the
    launch with top_table 0, with table steps for a single tagged lane (1), as shipped (24) and never (65)."""
    tree, verts, n_int, rays = scene_case(name)
    monkeypatch.setattr(AggregateAtBurst, "burst", burst)
    monkeypatch.setattr(test_top_table, "BVHAggregate", AggregateAtBurst)
    check_scene(tree, verts, rays[0], rays[1:], f"{name}, top_burst {burst}", min(n_int, K))


@functools.lru_cache(maxsize=None)
def edge_case():
    """soup-300 (255 of its records in LDS, the others not) with the oracle's results for its four batches"""
    tree, verts, _, _ = scene_case("soup-300")
    rays = [ray_mix(verts.min(0), verts.max(0), 1100, 90 + k) for k in range(4)]
    exp_any = ob.any_hit(tree.nodes, tree.ordered_prims, verts, rays[0])[0]
    exp = [ob.closest(tree.nodes, tree.ordered_prims, verts, r) for r in rays[1:]]
    return tree, verts, rays, exp_any, exp


@gpu
@pytest.mark.parametrize("per_cu", (1, 4, 8))
def test_batch_and_block_boundaries(per_cu):
    """Batches of 1, 63, 64, 65, 1023, 1024 and 1025 rays (a lane, a wave and a 1024-thread block, one less and one more;
    the grid is clamped to the rays) on 1, 4 and 8 units of 256 lanes per CU: 1 / 4 block per CU, 1 block, 2 blocks."""
    from test_top_table_steps import check_launch
    tree, verts, rays, exp_any, exp = edge_case()
    agg = BVHAggregate.from_tree(tree.nodes, tree.ordered_prims, verts)
    try:
        agg.set_option("blocks_per_cu", per_cu)
        for n in (1, 63, 64, 65, 1023, 1024, 1025):
            check_launch(agg, 24, rays[0][:n].copy(), [r[:n].copy() for r in rays[1:]], exp_any[:n], [e[:n] for e in exp],
                         f"batches of {n}, blocks_per_cu {per_cu}")
        sizes = (1025, 1, 1024, 63)
        check_launch(agg, 24, rays[0][:sizes[0]].copy(), [r[:m].copy() for r, m in zip(rays[1:], sizes[1:])],
                     exp_any[:sizes[0]], [e[:m] for e, m in zip(exp, sizes[1:])], f"batches of {sizes}")
    finally:
        agg.close()


@gpu
@pytest.mark.parametrize("burst", (1, 24, 65))
def test_soa_twin_with_the_extended_table(burst):
    """IntersectClosestAndShadow on queues, as test_top_table_steps.test_soa_twin but on soup-300: the instance
    <3, 8, 0, 0, 0, 1> builds the same table in its 1024-thread blocks."""
    import torch
    from nn_bvh_amd.wavefront import RayQueue, WavefrontAggregate
    from test_wavefront import shadow_inputs
    tree, verts, rays4, exp_any, exp_cl = edge_case()
    rays = rays4[0]
    cap, n = len(rays), len(rays) - 37  # 1 063 of 1 100: a full block and a wave with idle lanes
    q = rays[:n].copy()
    q["tmax"] = np.inf  # a closest queue carries no tMax
    exp = ob.closest(tree.nodes, tree.ordered_prims, verts, q)
    eocc = exp_any[:n]
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
        agg.set_option("top_burst", burst)
        for table in (1, 0):
            agg.set_option("top_table", table)
            hits_t = torch.full((cap, 32), 0xAB, dtype=torch.uint8, device=dev)
            occ_t = torch.full((cap,), 9, dtype=torch.uint8, device=dev)
            l_t = t(L.copy())
            wf.IntersectClosestAndShadow(cap, rq, cap, sq, t(Ld), t(r_u), t(r_l), t(px), l_t, hits=hits_t, occluded=occ_t)
            torch.cuda.synchronize()
            hits, occ = hits_t.cpu().numpy(), occ_t.cpu().numpy()
            what = f"top_burst {burst}, top_table {table}"
            assert hits[:n].tobytes() == exp.tobytes(), f"hit records, {what}"
            assert (hits[n:] == 0xAB).all() and (occ[n:] == 9).all(), f"wrote beyond the size, {what}"
            assert np.array_equal(occ[:n], eocc), f"occlusion flags, {what}"
            assert np.array_equal(l_t.cpu().numpy().view(np.uint32), exp_l.view(np.uint32)), f"radiance, {what}"
    finally:
        agg.close()


@gpu
def test_full_grid_spill_at_1024_threads():
    """The 64-deep chain, closest hit through the one-launch call at blocks_per_cu 8 (two 1024-thread blocks per CU):
    1.25 deep rays per lane of the largest grid, 4 096 distinct rays tiled, so every lane of every block holds a deep ray
    at once and the last lane of the last block reaches the last level of the spill array, which is sized by lanes
    (n_cus * 8 * 256) whatever the block size."""
    import torch
    from test_stack_limits import N_DISTINCT, full_grid_count, upload
    ch = ss.chain_tree(64, np.random.default_rng(51), tube=True, leaves="tri", extras=True)
    distinct = ss.chain_rays(float(ch.leaf_hi[:, 0].max()), N_DISTINCT, 52, tmax_share=0.0)
    with ob.pending_depth(N_DISTINCT) as dc:
        exp = ob.closest(ch.nodes, ch.prims, ch.verts, distinct)
    assert (dc.depth[:, 0] == 64).all()
    n = full_grid_count()
    d_rays = upload(np.tile(distinct, n // N_DISTINCT))
    out = torch.full((n * 32,), 0x5A, dtype=torch.uint8, device="cuda")
    agg = BVHAggregate.from_tree(ch.nodes, ch.prims, ch.verts)
    try:
        agg.set_option("blocks_per_cu", 8)
        agg.trace_batches_device([("closest", d_rays.data_ptr(), n, out.data_ptr())],
                                 torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got = out.cpu().numpy().reshape(n // N_DISTINCT, N_DISTINCT * 32)
        want = np.frombuffer(exp.tobytes(), np.uint8)
        for tile in range(len(got)):
            assert np.array_equal(got[tile], want), f"tile {tile}"
    finally:
        agg.close()
