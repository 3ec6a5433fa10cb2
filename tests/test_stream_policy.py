"""The loads and stores of once-used data in the trace and film kernels: ray fetch (records and SOA slices), the
retire stores of every mode (hit records, occlusion bytes, counts), the stack spill store and re-load, the film
stage's sample inputs.  A cache policy on these accesses may change where bytes live, never what they are: every
result here equals the oracle's byte for byte, every byte inside [0, n) of an output is written (two different
sentinels), and no byte of a guard region behind n is touched.

Shapes: 3 * 64 + 5 rays per class, so that a wavefront refills part of its lanes and the last grant of the queue is a
partial one; a chain 11 deep, just past the 8-entry stack window, so that the spill store and the re-load run."""
import numpy as np
import pytest

import oracle_binding as ob
import scenes_small as ss
from nn_bvh_amd import HIT_DTYPE, BVHAggregate, build_tree, scene
from test_stack_limits import assert_exceeds_window, bvh_ray_set, oracle_single

pytestmark = pytest.mark.gpu
N = 3 * 64 + 5
GUARD = 64  # records / flags behind n that must keep the sentinel
SENTINELS = (0x5A, 0xA5)


@pytest.fixture(scope="module")
def soup():
    """A few hundred random triangles, their SAH tree, three ray classes and the oracle's answers (computed once)."""
    verts, prims = ss.random_soup(n_tris=300, seed=11)
    tree = build_tree(prims, verts)
    lo, hi = verts.min(0) - 1, verts.max(0) + 1
    rays = [scene.random_rays(n, lo, hi, seed=40 + k) for k, n in enumerate((N, N - 64, N + 3))]
    rays[1]["tmax"][::3] = 4.0
    exp = [ob.closest(tree.nodes, tree.ordered_prims, verts, r) for r in rays]
    eany = [ob.any_hit(tree.nodes, tree.ordered_prims, verts, r) for r in rays]
    assert (exp[0]["prim"] >= 0).any() and (exp[0]["prim"] < 0).any() and eany[0][0].any() and not eany[0][0].all()
    return dict(verts=verts, nodes=tree.nodes, prims=tree.ordered_prims, rays=rays, exp=exp, eany=eany)


@pytest.fixture(scope="module")
def soup_agg(soup):
    agg = BVHAggregate.from_tree(soup["nodes"], soup["prims"], soup["verts"])
    yield agg
    agg.close()


def upload(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def filled(n_bytes, sentinel):
    import torch
    return torch.full((n_bytes,), sentinel, dtype=torch.uint8, device="cuda")


def check_out(buf, exp_bytes, sentinel, what):
    """buf: device bytes; [0, len(exp_bytes)) must be the oracle's, the rest the untouched sentinel"""
    got = buf.cpu().numpy()
    n = len(exp_bytes)
    assert got[:n].tobytes() == exp_bytes, f"{what}: differs from the oracle"
    assert (got[n:] == sentinel).all(), f"{what}: wrote behind n"


@pytest.mark.parametrize("sentinel", SENTINELS)
def test_single_calls_write_exactly_their_range(soup, soup_agg, sentinel):
    import torch
    s = torch.cuda.current_stream().cuda_stream
    rays, exp, (eocc, evis, etst) = soup["rays"][0], soup["exp"][0], soup["eany"][0]
    d = upload(rays)
    hits = filled((N + GUARD) * 32, sentinel)
    soup_agg.intersect_device(d.data_ptr(), hits.data_ptr(), N, s)
    occ = filled(N + GUARD, sentinel)
    soup_agg.intersect_p_device(d.data_ptr(), occ.data_ptr(), N, stream=s)
    occ_c, vis, tst = filled(N + GUARD, sentinel), filled((N + GUARD) * 4, sentinel), filled((N + GUARD) * 4, sentinel)
    soup_agg.intersect_p_device(d.data_ptr(), occ_c.data_ptr(), N, vis.data_ptr(), tst.data_ptr(), stream=s)
    torch.cuda.synchronize()
    check_out(hits, exp.tobytes(), sentinel, "closest hit records")
    check_out(occ, eocc.astype(np.uint8).tobytes(), sentinel, "occlusion flags")
    check_out(occ_c, eocc.astype(np.uint8).tobytes(), sentinel, "occlusion flags of the counting call")
    check_out(vis, evis.astype(np.int32).tobytes(), sentinel, "nodes visited")
    check_out(tst, etst.astype(np.int32).tobytes(), sentinel, "primitive tests")


@pytest.mark.parametrize("sentinel", SENTINELS)
def test_one_launch_batches_write_exactly_their_ranges(soup, soup_agg, sentinel):
    """one any-hit and two closest batches of unequal sizes, and an empty one between them"""
    import torch
    s = torch.cuda.current_stream().cuda_stream
    ra, rb, rc = soup["rays"]
    da, db, dc = upload(ra), upload(rb), upload(rc)
    oa = filled(len(ra) + GUARD, sentinel)
    ob_, oc = filled((len(rb) + GUARD) * 32, sentinel), filled((len(rc) + GUARD) * 32, sentinel)
    oe = filled(GUARD * 32, sentinel)
    soup_agg.trace_batches_device([("any", da.data_ptr(), len(ra), oa.data_ptr()),
                                   ("closest", db.data_ptr(), len(rb), ob_.data_ptr()),
                                   ("closest", dc.data_ptr(), 0, oe.data_ptr()),
                                   ("closest", dc.data_ptr(), len(rc), oc.data_ptr())], s)
    torch.cuda.synchronize()
    check_out(oa, soup["eany"][0][0].astype(np.uint8).tobytes(), sentinel, "any batch")
    check_out(ob_, soup["exp"][1].tobytes(), sentinel, "first closest batch")
    check_out(oe, b"", sentinel, "empty batch")
    check_out(oc, soup["exp"][2].tobytes(), sentinel, "second closest batch")


def test_spill_store_and_reload():
    """11 pending entries per deep ray against a window of 8: the oldest entries go to the spill array and come back"""
    ch = ss.chain_tree(11, np.random.default_rng(5), tube=True, leaves="tri", extras=True)
    rays, deep = bvh_ray_set(ch.leaf_lo, ch.leaf_hi, 6, n_deep=N - 40, n_random=40)
    exp, eany, dc, da = oracle_single(ch, rays)
    assert_exceeds_window(dc, deep, 8, "closest")
    assert_exceeds_window(da, deep, 8, "any")
    agg = BVHAggregate.from_tree(ch.nodes, ch.prims, ch.verts)
    hits = agg.Intersect(rays)
    assert np.array_equal(hits["nodes_visited"], exp["nodes_visited"])
    assert hits.tobytes() == exp.tobytes()
    occ, vis, tst = agg.IntersectP(rays, counts=True)
    assert np.array_equal(occ, eany[0]) and np.array_equal(vis, eany[1]) and np.array_equal(tst, eany[2])
    assert np.array_equal(agg.IntersectP(rays), eany[0])
    agg.close()


@pytest.mark.parametrize("sentinel", SENTINELS)
def test_queue_slices_feed_the_kernel(soup, soup_agg, sentinel):
    """WavefrontAggregate.IntersectClosest on a RayQueue: the kernel reads the SOA slices itself"""
    import torch
    from nn_bvh_amd.wavefront import RayQueue, WavefrontAggregate
    dev = torch.device("cuda", 0)
    rays = np.concatenate([soup["rays"][0], soup["rays"][2][:GUARD]])  # capacity N + GUARD, device-side size N
    rays["tmax"] = np.inf  # a closest queue carries no tMax
    exp = ob.closest(soup["nodes"], soup["prims"], soup["verts"], rays[:N])
    rq = RayQueue.from_records(rays, dev)
    rq.size.fill_(N)
    hits = torch.full((N + GUARD, 32), sentinel, dtype=torch.uint8, device=dev)
    WavefrontAggregate(soup_agg).IntersectClosest(N + GUARD, rq, hits=hits)
    torch.cuda.synchronize()
    check_out(hits.reshape(-1), exp.tobytes(), sentinel, "queue-fed closest hit records")
    assert exp.dtype == HIT_DTYPE


def test_film_samples():
    """7 x 5 film, 3 passes, one slot outside the bounds: float product, double sum, in sample order"""
    import torch
    from nn_bvh_amd.film import Film
    xres, yres, passes = 7, 5, 3
    rng = np.random.default_rng(9)
    lin = rng.permutation(xres * yres)[:20]
    px, py = (lin % xres).astype(np.int32), (lin // xres).astype(np.int32)
    px[4] = xres  # outside: skipped
    n = len(px)
    rgb = (rng.random((n * passes, 3), np.float32) * np.float32(3.0)).astype(np.float32)
    w = (rng.random(n * passes, np.float32) + np.float32(0.25)).astype(np.float32)
    film = Film(xres, yres, float("inf"))
    d = [torch.from_numpy(a).cuda() for a in (px, py, rgb, w)]
    film.add_samples_device(d[0], d[1], d[2], d[3], n, passes, rgb_stride=3,
                            stream=torch.cuda.current_stream().cuda_stream)
    got = film.read()
    exp = np.zeros((xres * yres, 4), np.float64)
    for p in range(passes):
        for i in range(n):
            if 0 <= px[i] < xres and 0 <= py[i] < yres:
                k = p * n + i
                for c in range(3):
                    exp[py[i] * xres + px[i], c] += float(np.float32(w[k] * rgb[k, c]))
                exp[py[i] * xres + px[i], 3] += float(w[k])
    assert got.tobytes() == exp.tobytes()
    assert (got[:, 3] > 0).sum() == n - 1
