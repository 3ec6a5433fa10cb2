"""Table steps of the lean one-launch kernels (trace_kernel<3, 8, 0, 0> and its SOA twin, bvh_trace.hip): a wave with at
least `top_burst` lanes at a record of the LDS top table advances those lanes in a step of their own, which loads nothing
from memory; fewer ride along in the ordinary interior step.  Which wave trip carries a ray's step is all that changes, so
every case compares the one-launch call bit for bit with the oracle (records with both counts, occlusion flags) and with
the same call with the table switched off (option "top_table" 0), at top_burst 1 (a single tagged lane takes a table
step), 8, 64 (only a full wave of tagged lanes does: straight after a full refill) and 65 (never)."""
import functools

import numpy as np
import pytest

import oracle_binding as ob
import scenes_small as ss
from nn_bvh_amd import BVHAggregate, NNBVHError, build_tree
from test_top_table import K, one_launch, ray_mix

gpu = pytest.mark.gpu
BURSTS = (1, 8, 64, 65)


@functools.lru_cache(maxsize=None)
def soup(n_tris, max_prims):
    """A seeded soup, its tree, four batches of 3 000 ray_mix rays and the oracle's results for them (computed once)."""
    verts, prims = ss.random_soup(n_tris, seed=31)
    tree = build_tree(prims, verts, max_prims_in_node=max_prims)
    lo, hi = verts.min(0), verts.max(0)
    rays = [ray_mix(lo, hi, 3000, 40 + k) for k in range(4)]
    exp_any = ob.any_hit(tree.nodes, tree.ordered_prims, verts, rays[0])[0]
    exp = [ob.closest(tree.nodes, tree.ordered_prims, verts, r) for r in rays[1:]]
    return tree, verts, rays, exp_any, exp


def check_launch(agg, burst, any_rays, closest_batches, exp_any, exp, what):
    """The one-launch call at `burst` and at top_table 0 against the oracle, hence against each other."""
    agg.set_option("top_burst", burst)
    try:
        for table in (1, 0):
            agg.set_option("top_table", table)
            flags, recs = one_launch(agg, any_rays, closest_batches)
            assert np.array_equal(flags, exp_any), f"{what}: any batch, top_burst {burst}, top_table {table}"
            for b, (got, want) in enumerate(zip(recs, exp)):
                assert got.tobytes() == want.tobytes(), f"{what}: closest batch {b}, top_burst {burst}, top_table {table}"
    finally:
        agg.set_option("top_table", 1)


@gpu
@pytest.mark.parametrize("burst", BURSTS)
@pytest.mark.parametrize("n_tris,max_prims,interior", [(72, 4, "above"), (50, 4, "below"), (1, 4, "none"), (2, 1, "one")],
                         ids=["above-K", "below-K", "one-leaf", "two-triangles"])
def test_soups(n_tris, max_prims, interior, burst):
    """Above K: table steps hand lanes over to global records, leaves and pops.  Below K: the whole tree is in LDS, rays
    reach leaves, pop and finish from inside table steps.  A table of 0 / 1 records: nothing to step on, nothing hangs."""
    tree, verts, rays, exp_any, exp = soup(n_tris, max_prims)
    n_int = int((tree.nodes["nprims"] == 0).sum())
    assert {"below": 30 < n_int < K, "above": K < n_int <= K + 12, "none": n_int == 0, "one": n_int == 1}[interior], n_int
    agg = BVHAggregate.from_tree(tree.nodes, tree.ordered_prims, verts)
    try:
        check_launch(agg, burst, rays[0], rays[1:], exp_any, exp, f"{n_tris} triangles")
    finally:
        agg.close()


@gpu
def test_top_burst_range():
    tree, verts, *_ = soup(2, 1)
    agg = BVHAggregate.from_tree(tree.nodes, tree.ordered_prims, verts)
    try:
        for bad in (0, 66, -1):
            with pytest.raises(NNBVHError):
                agg.set_option("top_burst", bad)
        for good in (1, 65):
            agg.set_option("top_burst", good)
    finally:
        agg.close()


@functools.lru_cache(maxsize=None)
def chain():
    """The deep-chain scene of test_top_table.test_spilled_tagged_references with its rays and the oracle's results."""
    from test_stack_limits import assert_exceeds_window, bvh_ray_set, oracle_single
    ch = ss.chain_tree(64, np.random.default_rng(21), tube=True, leaves="tri", extras=True)
    rays, deep = bvh_ray_set(ch.leaf_lo, ch.leaf_hi, 24)
    exp, eany, dc, da = oracle_single(ch, rays)
    assert_exceeds_window(dc, deep, 8, "closest")
    assert_exceeds_window(da, deep, 8, "any")
    return ch, rays, exp, eany[0]


@gpu
@pytest.mark.parametrize("burst", BURSTS)
def test_chain_spills(burst):
    """Every deep ray holds 64 pending entries and the chain's first 63 records are all in the table: a table step pushes
    with a full window (the spill store), and a table step's pop re-loads a spilled tagged reference."""
    ch, rays, exp, eany = chain()
    agg = BVHAggregate.from_tree(ch.nodes, ch.prims, ch.verts)
    try:
        assert agg.info["depth"] == 64 and agg.info["interior_records"] >= K
        check_launch(agg, burst, rays[::-1].copy(), [rays, rays[::2].copy()], eany[::-1], [exp, exp[::2]], "chain")
    finally:
        agg.close()


@gpu
@pytest.mark.parametrize("burst", BURSTS)
def test_batch_edges(burst):
    """Batches of 1, 63, 64 and 65 rays, any first then closest: a refill straight into a table step with few lanes, the
    switch from one batch to the next between table steps, a last wave with idle lanes."""
    tree, verts, rays, exp_any, exp = soup(72, 4)
    agg = BVHAggregate.from_tree(tree.nodes, tree.ordered_prims, verts)
    try:
        for n in (1, 63, 64, 65):
            # (the oracle's results are per ray: the first n of a batch are the results of its first n rays)
            check_launch(agg, burst, rays[0][:n].copy(), [r[:n].copy() for r in rays[1:]], exp_any[:n],
                         [e[:n] for e in exp], f"batches of {n}")
        # ... and of different sizes in one launch
        sizes = (65, 1, 64, 63)
        check_launch(agg, burst, rays[0][:sizes[0]].copy(), [r[:m].copy() for r, m in zip(rays[1:], sizes[1:])],
                     exp_any[:sizes[0]], [e[:m] for e, m in zip(exp, sizes[1:])], "batches of 65, 1, 64, 63")
    finally:
        agg.close()


@functools.lru_cache(maxsize=None)
def soa_case():
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
    return tree, verts, rays, n, exp, eocc, (Ld, r_u, r_l, px, L), exp_l


@gpu
@pytest.mark.parametrize("burst", BURSTS)
def test_soa_twin(burst):
    """IntersectClosestAndShadow on queues, as test_top_table.test_soa_twin: the <3, 8, 0, 0, 0, 1> instance."""
    import torch
    from nn_bvh_amd.wavefront import RayQueue, WavefrontAggregate
    tree, verts, rays, n, exp, eocc, (Ld, r_u, r_l, px, L), exp_l = soa_case()
    cap = len(rays)
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
