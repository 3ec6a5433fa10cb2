"""The bounded, graph-capturable forms of IntersectShadowTr / IntersectOneRandom
(nnbvh_wavefront_intersect_shadow_tr_bounded / _one_random_bounded): exactly max_passes passes, kernel launches only.

An item is finished iff the reference loop (wavefront/intersect.h:183-256, aggregate.cpp:100-108) makes at most
max_passes calls of Intersect for it.  The composed oracle of test_wavefront_tr.py, with a counter of those calls per
item, gives what finished items must hold bit for bit and which items must carry the "caller's to finish" mark
(state 2 / instance = -1).  The unbounded entry points run the same pass (the trace and one fused step) under a
host-driven driver, so they are no independent reference: on scenes the composed oracle does not cover (bilinear
patches, host-only primitives, instances) both forms are held to the loops of test_wavefront_walk_kd.py
(device_shadow_walk / device_one_random_walk) over calls that exist without either: the flat closest-hit call, the
public interaction post-pass and the oracle's SpawnRayTo.  The last test runs the unbounded driver past the 64 passes
the bounded form stops at."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import oracle_binding as ob
import scenes_small as ss
from nn_bvh_amd import HIT_DTYPE, RAY_DTYPE, _lib, build_tree, scene
from test_wavefront_tr import layered_scene, oracle_interactions, oracle_one_random

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDED = ("nnbvh_wavefront_intersect_shadow_tr_bounded", "nnbvh_wavefront_intersect_one_random_bounded")
SENTINEL = 77


# ---- the composed oracle with a per-item count of Intersect calls -------------------------------------------------
def shadow_walk(tree, verts, tris, rays, prim_class):
    """oracle_shadow_tr's loop -> (state per ray, Intersect calls per ray)."""
    n = len(rays)
    state, calls = np.zeros(n, np.uint8), np.zeros(n, np.int64)
    p_light = (rays["o"] + rays["d"] * rays["tmax"][:, None]).astype(np.float32)
    cur, idx = rays.copy(), np.arange(n)
    while len(idx):
        live = (cur["d"] != 0).any(1)  # while (ray.d != Vector3f(0, 0, 0)), intersect.h:183
        cur, idx = cur[live], idx[live]
        if not len(idx):
            break
        calls[idx] += 1
        h = ob.closest(tree.nodes, tree.ordered_prims, verts, cur)
        hit = h["prim"] >= 0
        iface = hit & ((prim_class[np.maximum(h["prim"], 0)] & 2) != 0)
        state[idx[hit & ~iface]] = 1
        cur, idx, h = cur[iface], idx[iface], h[iface]
        if not len(idx):
            break
        lo, hi, nn = oracle_interactions(verts, tris, cur, h)
        sp = ob.offset_batch(np.concatenate([lo, hi, nn, p_light[idx]], 1))
        cur = cur.copy()
        cur["o"], cur["d"] = sp[:, 3:6], sp[:, 6:9]
    return state, calls


def shadow_radiance(state, Ld, ru, rl, pixel, L0):
    """intersect.h:258-273 with T_ray = r_u = r_l = 1 for the rays of state 0, in item order."""
    L = L0.copy()
    for i in np.nonzero(state == 0)[0]:
        s = ru[i] * np.float32(1) + rl[i] * np.float32(1)
        acc = s[0]
        for k in (1, 2, 3):
            acc = np.float32(acc + s[k])
        kk = np.float32(1) / np.float32(acc / np.float32(4))
        L[pixel[i]] = L[pixel[i]] + Ld[i] * kk
    return L


def one_random_calls(tree, verts, tris, p0, p1):
    """Intersect calls per item of oracle_one_random's loop (aggregate.cpp:100-108)."""
    n = len(p0)
    calls = np.zeros(n, np.int64)
    lo, hi, nn = p0.copy(), p0.copy(), np.zeros_like(p0)
    idx = np.arange(n)
    while len(idx):
        sp = ob.offset_batch(np.concatenate([lo, hi, nn, p1[idx]], 1))
        rays = np.zeros(len(idx), RAY_DTYPE)
        rays["o"], rays["d"], rays["tmax"] = sp[:, 3:6], sp[:, 6:9], 1.0
        live = (rays["d"] != 0).any(1)
        rays, idx = rays[live], idx[live]
        if not len(idx):
            break
        calls[idx] += 1
        h = ob.closest(tree.nodes, tree.ordered_prims, verts, rays)
        hit = h["prim"] >= 0
        rays, idx, h = rays[hit], idx[hit], h[hit]
        if not len(idx):
            break
        lo, hi, nn = oracle_interactions(verts, tris, rays, h)
    return calls


class Case:
    pass


@functools.lru_cache(maxsize=None)
def shadow_case():
    c = Case()
    c.verts, c.tris = layered_scene(3)
    c.tree = build_tree(ss.make_prims(c.tris), c.verts)
    rng = np.random.default_rng(8)
    c.cls = rng.choice(np.array([0, 1, 2, 2, 2, 6], np.uint8), len(c.tris))
    n = c.n = 1999
    c.rays = scene.random_rays(n, [-3.5, -3.5, -5], [3.5, 3.5, 5], 9, tmax=1 - 1e-4)
    c.rays["d"][::97] = 0
    c.rays["time"] = rng.random(n).astype(np.float32)
    c.Ld = (rng.random((n, 4), np.float32) * 2).astype(np.float32)
    c.ru = (rng.random((n, 4), np.float32) + 0.5).astype(np.float32)
    c.rl = (rng.random((n, 4), np.float32) + 0.5).astype(np.float32)
    c.pixel = rng.permutation(n).astype(np.int32)
    c.L0 = rng.random((n, 4), np.float32).astype(np.float32)
    c.state, c.calls = shadow_walk(c.tree, c.verts, c.tris, c.rays, c.cls)
    return c


@functools.lru_cache(maxsize=None)
def one_random_case():
    c = Case()
    c.verts, c.tris = layered_scene(5)
    c.tree = build_tree(ss.make_prims(c.tris), c.verts)
    rng = np.random.default_rng(10)
    n = c.n = 1499
    c.p0 = rng.uniform([-3, -3, -4.5], [3, 3, 4.5], (n, 3)).astype(np.float32)
    c.p1 = rng.uniform([-3, -3, -4.5], [3, 3, 4.5], (n, 3)).astype(np.float32)
    c.p1[::50] = c.p0[::50]
    c.prim_material = rng.integers(0, 3, len(c.tris)).astype(np.int32)
    c.material = rng.integers(0, 3, n).astype(np.int32)
    c.hits, c.rays, c.pdf, c.wsum, _ = oracle_one_random(c.tree, c.verts, c.tris, c.p0, c.p1, c.material,
                                                         c.prim_material)
    c.calls = one_random_calls(c.tree, c.verts, c.tris, c.p0, c.p1)
    return c


def shadow_expected(c, max_passes, size=None, order=None):
    """(state, L) the bounded call must leave for the first `size` rays of the case taken in `order`."""
    order = np.arange(c.n) if order is None else order
    size = c.n if size is None else size
    state = np.where(c.calls > max_passes, 2, c.state).astype(np.uint8)[order]
    full = np.full(c.n, SENTINEL, np.uint8)
    full[:size] = state[:size]
    live = np.full(c.n, 1, np.uint8)  # anything but 0: rays beyond the size add nothing
    live[:size] = state[:size]
    return full, shadow_radiance(live, c.Ld[order], c.ru[order], c.rl[order], c.pixel, c.L0)


# ---- CPU ----------------------------------------------------------------------------------------------------------
def test_bounded_calls_are_exported_prototyped_and_declared(nnbvh_lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nnbvh.h")).read(), flags=re.S)
    for name in BOUNDED:
        assert name in _lib.EXPORTS and hasattr(nnbvh_lib, name), name
        fn = getattr(nnbvh_lib, name)
        assert fn.restype == ctypes.c_int32 and fn.argtypes is not None, name
        assert re.search(r"\b" + name + r"\s*\(", header), name
        decl = header[header.index(name):]
        assert "int32_t max_passes, int32_t *d_unfinished, void *stream)" in re.sub(r"\s+", " ", decl[:decl.index(";")])
    assert len(nnbvh_lib.nnbvh_wavefront_intersect_shadow_tr_bounded.argtypes) == 17
    assert len(nnbvh_lib.nnbvh_wavefront_intersect_one_random_bounded.argtypes) == 16
    adapter = open(os.path.join(ROOT, "include", "nnbvh_aggregate.hpp")).read()
    assert "IntersectShadowTrBounded" in adapter and "IntersectOneRandomBounded" in adapter


def test_bounded_calls_reject_bad_arguments_before_any_device_work(nnbvh_lib):
    """NNBVH_ERR_ARG with a message that names the call.  The handles are opaque to the check that rejects the
    other arguments, so zeroed stand-ins serve where a handle must be non-NULL: nothing below reaches a device."""
    ERR_ARG = 1
    fake_scene, fake_mesh = ctypes.create_string_buffer(1 << 16), ctypes.create_string_buffer(1 << 16)
    S, M = ctypes.addressof(fake_scene), ctypes.addressof(fake_mesh)
    soa = np.zeros(1, _lib.RAY_SOA_DTYPE)
    for k in ("ox", "oy", "oz", "dx", "dy", "dz", "tmax"):
        soa[k] = 64  # non-NULL, never read
    Q, A = soa.ctypes.data, 64

    def shadow(s=S, m=M, n=8, q=Q, npc=0, arrays=(A, A, A, A, A), npx=8, passes=4):
        return nnbvh_lib.nnbvh_wavefront_intersect_shadow_tr_bounded(s, m, n, q, None, None, npc, *arrays, npx, None,
                                                                     passes, None, None)

    def one_random(s=S, m=M, n=8, arrays=(A, A, A), npm=0, outs=(A, A, A), passes=4):
        return nnbvh_lib.nnbvh_wavefront_intersect_one_random_bounded(s, m, n, *arrays, None, None, npm, *outs, None,
                                                                      passes, None, None)

    for call, name in ((shadow, "wavefront_intersect_shadow_tr_bounded"),
                       (one_random, "wavefront_intersect_one_random_bounded")):
        bad = [dict(s=None), dict(m=None), dict(passes=0), dict(passes=65), dict(passes=-1), dict(n=-1)]
        if call is shadow:
            bad += [dict(npc=-1), dict(npx=-1), dict(q=None)]
            bad += [dict(arrays=tuple(None if j == k else A for j in range(5))) for k in range(5)]
            nosoa = soa.copy()
            nosoa["dx"] = 0
            bad.append(dict(q=nosoa.ctypes.data))
        else:
            bad += [dict(npm=-1)]
            bad += [dict(arrays=tuple(None if j == k else A for j in range(3))) for k in range(3)]
            bad += [dict(outs=tuple(None if j == k else A for j in range(3))) for k in range(3)]
        for kw in bad:
            assert call(**kw) == ERR_ARG, (name, kw)
            assert _lib.last_error().startswith(name + ":"), (_lib.last_error(), kw)


def test_inputs_make_both_sides_of_every_truncation_non_empty():
    """The preconditions of the truncation tests, from the composed oracle alone."""
    s, r = shadow_case(), one_random_case()
    assert np.array_equal(np.bincount(s.calls), [21, 892, 536, 314, 148, 53, 29, 4, 2])
    assert np.array_equal(np.bincount(r.calls), [30, 223, 365, 308, 225, 149, 113, 65, 21])
    for c in (s, r):
        assert c.calls.max() == 8 and c.n % 64 != 0
        assert 0.05 < (c.calls > 2).mean() < 0.95
    # the verdicts are not one-sided either
    assert min((s.state == 0).sum(), (s.state == 1).sum()) > 100 and (r.hits["prim"] >= 0).mean() > 0.3
    # oracle_shadow_tr itself (the pinned loop) agrees with the counted copy of it
    from test_wavefront_tr import oracle_shadow_tr
    L = s.L0.copy()
    state, passes = oracle_shadow_tr(s.tree, s.verts, s.tris, s.rays, s.cls, s.Ld, s.ru, s.rl, s.pixel, L)
    assert np.array_equal(state, s.state) and passes == 8
    assert L.tobytes() == shadow_radiance(s.state, s.Ld, s.ru, s.rl, s.pixel, s.L0).tobytes()


# ---- GPU ----------------------------------------------------------------------------------------------------------
class ShadowDevice:
    """The shadow case on the device: scene, mesh, queue and per-ray arrays."""

    def __init__(self, c, order=None):
        import torch
        from nn_bvh_amd import BVHAggregate
        from nn_bvh_amd.interaction import ShadingMesh
        from nn_bvh_amd.wavefront import RayQueue, WavefrontAggregate
        self.c, self.dev = c, torch.device("cuda", 0)
        self.agg = BVHAggregate.from_tree(c.tree.nodes, c.tree.ordered_prims, c.verts)
        self.mesh = ShadingMesh(c.verts, c.tris)
        self.wf = WavefrontAggregate(self.agg, c.cls)
        self.t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        rays = c.rays if order is None else c.rays[order]
        self.q = RayQueue.from_records(rays, self.dev, shadow=True)
        self.q.time = self.t(rays["time"])
        sel = slice(None) if order is None else order
        self.Ld, self.ru, self.rl, self.pixel = self.t(c.Ld[sel]), self.t(c.ru[sel]), self.t(c.rl[sel]), self.t(c.pixel)
        self.unfinished = torch.full((1,), -3, dtype=torch.int32, device=self.dev)

    def set_rays(self, rays, order):
        """Rewrites the queue and the per-ray arrays in place (the addresses a captured graph holds stay valid)."""
        c = self.c
        self.q.o.copy_(self.t(rays["o"].T))
        self.q.d.copy_(self.t(rays["d"].T))
        self.q.tmax.copy_(self.t(rays["tmax"]))
        self.q.time.copy_(self.t(rays["time"]))
        for dst, src in ((self.Ld, c.Ld), (self.ru, c.ru), (self.rl, c.rl)):
            dst.copy_(self.t(src[order]))

    def run(self, max_passes, max_rays=None, L=None, state=None):
        import torch
        c = self.c
        L = self.t(c.L0) if L is None else L
        state = torch.full((c.n,), SENTINEL, dtype=torch.uint8, device=self.dev) if state is None else state
        self.wf.IntersectShadowTr(c.n if max_rays is None else max_rays, self.q, self.mesh, self.Ld, self.ru, self.rl,
                                  self.pixel, L, state, max_passes=max_passes,
                                  unfinished=None if max_passes is None else self.unfinished)
        torch.cuda.synchronize()
        return state.cpu().numpy(), L.cpu().numpy(), int(self.unfinished.item())

    def close(self):
        self.agg.close()
        self.mesh.close()


class OneRandomDevice:
    def __init__(self, c):
        import torch
        from nn_bvh_amd import BVHAggregate
        from nn_bvh_amd.interaction import ShadingMesh
        from nn_bvh_amd.wavefront import WavefrontAggregate
        self.c, self.dev = c, torch.device("cuda", 0)
        self.agg = BVHAggregate.from_tree(c.tree.nodes, c.tree.ordered_prims, c.verts)
        self.mesh = ShadingMesh(c.verts, c.tris)
        self.wf = WavefrontAggregate(self.agg)
        self.t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        self.p0, self.p1, self.material = self.t(c.p0), self.t(c.p1), self.t(c.material)
        self.prim_material = self.t(c.prim_material)
        self.size = torch.full((1,), c.n, dtype=torch.int32, device=self.dev)
        self.unfinished = torch.full((1,), -3, dtype=torch.int32, device=self.dev)

    def call(self, max_passes, max_items=None):
        return self.wf.IntersectOneRandom(self.c.n if max_items is None else max_items, self.p0, self.p1, self.material,
                                          self.mesh, self.prim_material, size=self.size, max_passes=max_passes,
                                          unfinished=None if max_passes is None else self.unfinished)

    def run(self, max_passes, max_items=None):
        import torch
        out = self.call(max_passes, max_items)
        torch.cuda.synchronize()
        return one_random_numpy(out) + (int(self.unfinished.item()),)

    def close(self):
        self.agg.close()
        self.mesh.close()


def one_random_numpy(out):
    sh, sr, pdf, wsum = out
    return (sh.cpu().numpy().view(HIT_DTYPE).reshape(-1), sr.cpu().numpy().view(RAY_DTYPE).reshape(-1),
            pdf.cpu().numpy(), wsum.cpu().numpy())


def check_one_random(c, got, max_passes, size=None, order=None):
    """Finished items hold the oracle's outputs bit for bit, unfinished ones instance = -1; returns their number."""
    gh, gr, pdf, wsum = got[:4]
    order = np.arange(c.n) if order is None else order
    size = c.n if size is None else size
    rows = np.arange(size)
    fin = c.calls[order][rows] <= max_passes
    f, src = rows[fin], order[rows][fin]
    assert (gh["instance"][rows[~fin]] == -1).all()
    assert np.array_equal(gh["prim"][f], c.hits["prim"][src]) and (gh["instance"][f] != -1).all()
    assert np.array_equal(wsum[f].view(np.uint32), c.wsum[src].view(np.uint32))
    assert np.array_equal(pdf[f].view(np.uint32), c.pdf[src].view(np.uint32))
    sel = c.hits["prim"][src] >= 0
    assert gh[f][sel].tobytes() == c.hits[src][sel].tobytes() and gr[f][sel].tobytes() == c.rays[src][sel].tobytes()
    assert not pdf[size:].any() and not wsum[size:].any()  # beyond the size: the zero fill, untouched
    return int((~fin).sum())


@pytest.mark.gpu
@pytest.mark.parametrize("max_passes", [8, 7, 2])
def test_gpu_bounded_shadow_tr_equals_oracle(max_passes):
    c = shadow_case()
    d = ShadowDevice(c)
    state, L, unfinished = d.run(max_passes)
    exp_state, exp_L = shadow_expected(c, max_passes)
    left = int((c.calls > max_passes).sum())
    print(f"max_passes {max_passes}: unfinished {unfinished} (oracle {left}), states "
          f"{np.bincount(state, minlength=3)[:3]} (oracle {np.bincount(exp_state, minlength=3)[:3]})")
    assert left == {8: 0, 7: 2, 2: int((c.calls > 2).sum())}[max_passes]
    assert np.array_equal(state, exp_state)
    assert L.tobytes() == exp_L.tobytes()
    assert unfinished == left
    if max_passes == 8:  # ... and the unbounded entry point's, on the same inputs
        ref_state, ref_L, _ = d.run(None)
        assert np.array_equal(state, ref_state) and L.tobytes() == ref_L.tobytes()
    d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("max_passes", [8, 7, 2])
def test_gpu_bounded_one_random_equals_oracle(max_passes):
    c = one_random_case()
    d = OneRandomDevice(c)
    got = d.run(max_passes)
    left = check_one_random(c, got, max_passes)
    print(f"max_passes {max_passes}: unfinished {got[4]} (oracle {left})")
    assert left == {8: 0, 7: 21, 2: int((c.calls > 2).sum())}[max_passes]
    assert got[4] == left
    if max_passes == 8:
        ref = d.run(None)
        for a, b in zip(got[:4], ref[:4]):
            assert a.tobytes() == b.tobytes()
    d.close()


@pytest.mark.gpu
def test_gpu_bounded_calls_take_their_size_from_the_device():
    import torch
    c, r = shadow_case(), one_random_case()
    d, e = ShadowDevice(c), OneRandomDevice(r)
    for value, size in ((c.n // 2, c.n // 2), (0, 0), (c.n + 1000, c.n), (-5, 0)):
        d.q.size.fill_(value)
        state, L, unfinished = d.run(8)
        exp_state, exp_L = shadow_expected(c, 8, size)
        assert np.array_equal(state, exp_state) and L.tobytes() == exp_L.tobytes() and unfinished == 0, value
    d.q.size.fill_(c.n // 2)  # a truncated walk counts the unfinished rays of the live part only
    assert d.run(2)[2] == int((c.calls[: c.n // 2] > 2).sum())
    d.q.size.fill_(c.n)
    for max_rays in (0, 1, 64, 65):
        state, L, unfinished = d.run(3, max_rays)
        exp_state, exp_L = shadow_expected(c, 3, max_rays)
        assert np.array_equal(state, exp_state) and L.tobytes() == exp_L.tobytes(), max_rays
        assert unfinished == int((c.calls[:max_rays] > 3).sum()), max_rays
    for value, size in ((r.n // 2, r.n // 2), (0, 0), (r.n + 1000, r.n), (-5, 0)):
        e.size.fill_(value)
        got = e.run(8)
        assert check_one_random(r, got, 8, size) == 0 and got[4] == 0, value
    e.size.fill_(r.n)
    for max_items in (0, 1, 64, 65):
        got = e.run(3, max_items)
        assert check_one_random(r, got, 3, max_items) == got[4], max_items
    torch.cuda.synchronize()
    d.close()
    e.close()


@pytest.mark.gpu
def test_gpu_bounded_calls_are_hip_graph_capturable():
    """Both bounded calls in ONE captured graph; between the replays the queue contents and the device-side sizes are
    rewritten in place, and each replay equals the oracle for the inputs it saw."""
    import torch
    c, r = shadow_case(), one_random_case()
    d, e = ShadowDevice(c), OneRandomDevice(r)
    L0 = d.t(c.L0)
    L = L0.clone()
    state = torch.full((c.n,), SENTINEL, dtype=torch.uint8, device=d.dev)
    side = torch.cuda.Stream(d.dev)
    torch.cuda.synchronize()

    def step():
        d.wf.IntersectShadowTr(c.n, d.q, d.mesh, d.Ld, d.ru, d.rl, d.pixel, L, state, max_passes=8,
                               unfinished=d.unfinished)
        return e.call(7)

    with torch.cuda.stream(side):
        step()  # warm-up: the stream's workspace gets its size (allocation is not capturable)
    torch.cuda.synchronize()
    L.copy_(L0)
    state.fill_(SENTINEL)
    d.unfinished.fill_(-3)
    e.unfinished.fill_(-3)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out = step()
    torch.cuda.synchronize()
    assert (state == SENTINEL).all() and torch.equal(L, L0), "capture must not execute the work"
    assert int(d.unfinished.item()) == -3 and int(e.unfinished.item()) == -3
    # replay 1: the inputs as they are
    graph.replay()
    torch.cuda.synchronize()
    exp_state, exp_L = shadow_expected(c, 8)
    assert np.array_equal(state.cpu().numpy(), exp_state) and L.cpu().numpy().tobytes() == exp_L.tobytes()
    assert int(d.unfinished.item()) == 0
    assert check_one_random(r, one_random_numpy(out), 7) == 21 == int(e.unfinished.item())
    # replay 2: every queue reversed in place and cut to half by its device-side size
    so, ro = np.arange(c.n)[::-1].copy(), np.arange(r.n)[::-1].copy()
    d.set_rays(c.rays[so], so)
    d.q.size.fill_(c.n // 2)
    e.p0.copy_(e.t(r.p0[ro]))
    e.p1.copy_(e.t(r.p1[ro]))
    e.material.copy_(e.t(r.material[ro]))
    e.size.fill_(r.n // 2)
    L.copy_(L0)
    state.fill_(SENTINEL)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    exp_state, exp_L = shadow_expected(c, 8, c.n // 2, so)
    assert np.array_equal(state.cpu().numpy(), exp_state) and L.cpu().numpy().tobytes() == exp_L.tobytes()
    assert int(d.unfinished.item()) == 0
    left = check_one_random(r, one_random_numpy(out), 7, r.n // 2, ro)
    assert left == int((r.calls[ro][: r.n // 2] > 7).sum()) == int(e.unfinished.item())
    del graph
    d.close()
    e.close()


def patch_scene():
    """Bilinear patches and triangles in one flat tree."""
    verts, prims = ss.random_soup(300, 100, 21, extent=3.0, size=0.8)
    tree = build_tree(prims, verts)
    tri = np.full((len(prims), 3), -1, np.int32)
    patch = np.full((len(prims), 4), -1, np.int32)
    tri[prims["kind"] == 0] = prims["v"][prims["kind"] == 0][:, :3]
    patch[prims["kind"] == 1] = prims["v"][prims["kind"] == 1]
    return dict(tree=(tree.nodes, tree.ordered_prims, verts), mesh=dict(tri_vertices=tri, patch_vertices=patch),
                n_ids=len(prims), box=3.5)


def host_prim_scene():
    """NNBVH_PRIM_HOST boxes among interface surfaces: the walk hands such rays / items to the caller."""
    verts, prims = ss.random_soup(400, 0, 22, extent=3.0, size=0.8)
    rng = np.random.default_rng(23)
    extra = np.zeros(15, prims.dtype)
    extra["kind"] = 3
    extra["id"] = len(prims) + np.arange(len(extra))
    allp = np.concatenate([prims, extra])
    lo = rng.uniform(-2.5, 2.5, (len(allp), 3)).astype(np.float32)
    pb = np.concatenate([lo, lo + rng.uniform(0.3, 0.8, (len(allp), 3)).astype(np.float32)], 1)
    tree = build_tree(allp, verts, prim_bounds=pb)
    return dict(tree=(tree.nodes, tree.ordered_prims, verts), mesh=dict(tri_vertices=prims["v"][:, :3].copy()),
                n_ids=len(allp), box=3.5)


def two_level_case():
    """A two-level scene whose shading mesh has the instance table: hits inside instances are finished on the device."""
    from test_instancing import two_level_scene
    verts, nodes, prims, instances, n_top, _ = two_level_scene(3, 50)
    prims = prims.copy()
    prims["id"] = np.arange(len(prims))
    tri = np.full((len(prims), 3), -1, np.int32)
    patch = np.full((len(prims), 4), -1, np.int32)
    tri[prims["kind"] == 0] = prims["v"][prims["kind"] == 0][:, :3]
    patch[prims["kind"] == 1] = prims["v"][prims["kind"] == 1]
    return dict(tree=(nodes, prims, verts), mesh=dict(tri_vertices=tri, patch_vertices=patch), n_ids=len(prims),
                box=28.0, instances=instances, n_top=n_top)


@pytest.mark.gpu
@pytest.mark.parametrize("make", [patch_scene, host_prim_scene, two_level_case])
def test_gpu_bounded_calls_equal_the_unbounded_ones_beyond_flat_triangles(make):
    import torch
    from nn_bvh_amd import BVHAggregate
    from nn_bvh_amd.interaction import ShadingMesh
    from nn_bvh_amd.wavefront import RayQueue, WavefrontAggregate
    from test_wavefront_walk_kd import device_one_random_walk, device_shadow_walk  # (that module imports this one)
    s = make()
    nodes, prims, verts = s["tree"]
    mesh = ShadingMesh(verts, **s["mesh"])
    if "instances" in s:
        mesh.set_instances(s["instances"])
        agg = BVHAggregate.from_tree(nodes, prims, verts, instances=s["instances"], n_top_nodes=s["n_top"])
    else:
        agg = BVHAggregate.from_tree(nodes, prims, verts)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    rng = np.random.default_rng(31)
    n, box = 2001, s["box"]
    cls = rng.choice(np.array([0, 2, 2, 2, 2, 6], np.uint8), s["n_ids"])
    wf = WavefrontAggregate(agg, cls)
    rays = scene.random_rays(n, [-box] * 3, [box] * 3, 32, tmax=1 - 1e-4)
    rays["d"][::97] = 0
    rays["time"] = rng.random(n).astype(np.float32)
    q = RayQueue.from_records(rays, dev, shadow=True)
    q.time = t(rays["time"])
    Ld_h, ru_h, rl_h = ((rng.random((n, 4), np.float32) + 0.5).astype(np.float32) for _ in range(3))
    pixel_h = rng.permutation(n).astype(np.int32)
    Ld, ru, rl, pixel = t(Ld_h), t(ru_h), t(rl_h), t(pixel_h)
    L0 = rng.random((n, 4), np.float32).astype(np.float32)
    unfinished = torch.full((1,), -3, dtype=torch.int32, device=dev)

    def shadow(max_passes):
        L, state = t(L0), torch.full((n,), SENTINEL, dtype=torch.uint8, device=dev)
        wf.IntersectShadowTr(n, q, mesh, Ld, ru, rl, pixel, L, state, max_passes=max_passes,
                             unfinished=None if max_passes is None else unfinished)
        torch.cuda.synchronize()
        return state.cpu().numpy(), L.cpu().numpy()

    ref_state, ref_L = shadow(None)
    # the unbounded call against the loop over the flat closest-hit call, the interaction post-pass and SpawnRayTo
    walk_state, walk_calls = device_shadow_walk(agg, mesh, rays, cls)
    assert np.array_equal(ref_state, walk_state) and 1 < walk_calls.max() <= 16
    assert ref_L.tobytes() == shadow_radiance(ref_state, Ld_h, ru_h, rl_h, pixel_h, L0).tobytes()
    state, L = shadow(16)
    assert np.array_equal(state, ref_state) and L.tobytes() == ref_L.tobytes() and int(unfinished.item()) == 0
    one_state, _ = shadow(1)
    # walks of several passes; a ray that a later pass hands to the caller anyway is unfinished after one pass too
    assert 20 < ((one_state == 2) & (ref_state != 2)).sum() <= int(unfinished.item()) <= (one_state == 2).sum()
    if make is not host_prim_scene:
        assert int(unfinished.item()) == (one_state == 2).sum()
    assert ((one_state == ref_state) | (one_state == 2)).all()
    assert min((ref_state == 0).sum(), (ref_state == 1).sum()) > 20
    if make is host_prim_scene:
        assert (ref_state == 2).sum() > 20

    m = 1501
    p0 = rng.uniform(-box, box, (m, 3)).astype(np.float32)
    p1 = rng.uniform(-box, box, (m, 3)).astype(np.float32)
    p1[::50] = p0[::50]
    material = rng.integers(0, 3, m).astype(np.int32)
    prim_material = rng.integers(0, 3, s["n_ids"]).astype(np.int32)
    args = (m, t(p0), t(p1), t(material), mesh, t(prim_material))

    def one_random(max_passes):
        out = wf.IntersectOneRandom(*args, max_passes=max_passes, unfinished=None if max_passes is None else unfinished)
        torch.cuda.synchronize()
        return one_random_numpy(out)

    ref = one_random(None)
    # the unbounded call against the test-side loop, on the items that are not the caller's
    eh, er, epdf, ewsum, ecalls, host = device_one_random_walk(agg, mesh, p0, p1, material, prim_material)
    assert ecalls.max() <= 16
    gh, gr, pdf, wsum = ref
    assert np.array_equal(gh["instance"] == -1, host)
    assert np.array_equal(gh["prim"][~host], eh["prim"][~host])
    assert np.array_equal(pdf[~host].view(np.uint32), epdf[~host].view(np.uint32))
    assert np.array_equal(wsum[~host].view(np.uint32), ewsum[~host].view(np.uint32))
    sel = ~host & (eh["prim"] >= 0)
    assert gh[sel].tobytes() == eh[sel].tobytes() and gr[sel].tobytes() == er[sel].tobytes()
    got = one_random(16)
    assert int(unfinished.item()) == 0
    for a, b in zip(got, ref):
        assert a.tobytes() == b.tobytes()
    own = ref[0]["instance"] != -1  # the others: a host-only primitive lies on the segment
    assert (ref[0]["prim"][own] >= 0).sum() > 20
    one = one_random(1)
    assert 20 < ((one[0]["instance"] == -1) & own).sum() <= int(unfinished.item()) <= (one[0]["instance"] == -1).sum()
    if make is not host_prim_scene:
        assert int(unfinished.item()) == (one[0]["instance"] == -1).sum()
    if make is host_prim_scene:
        assert (~own).sum() > 20
    if make is two_level_case:
        assert (ref[0]["instance"][own & (ref[0]["prim"] >= 0)] > 0).sum() > 20  # selected hits inside instances
    agg.close()
    mesh.close()


@functools.lru_cache(maxsize=None)
def sheets_case():
    """70 parallel interface quads and 65 rays / segments across all of them (one full wavefront and one lane)."""
    from test_wavefront_walk_kd import one_random_walk
    from test_wavefront_walk_kd import shadow_walk as walk
    c = Case()
    k, c.n, c.capacity = 70, 65, 128
    z = (0.1 * np.arange(k)).astype(np.float32)
    quad = np.array([[-1, -1], [1, -1], [1, 1], [-1, 1]], np.float32)
    c.verts = np.concatenate([np.concatenate([quad, np.full((4, 1), zz, np.float32)], 1) for zz in z])
    c.tris = np.concatenate([4 * i + np.array([[0, 1, 2], [0, 2, 3]], np.int32) for i in range(k)]).astype(np.int32)
    c.tree = build_tree(ss.make_prims(c.tris), c.verts)
    c.cls = np.full(len(c.tris), 2, np.uint8)  # NNBVH_CLASS_INTERFACE
    closest = lambda rays: ob.closest(c.tree.nodes, c.tree.ordered_prims, c.verts, rays)  # noqa: E731
    rng = np.random.default_rng(70)
    c.p0 = np.concatenate([rng.uniform(-0.8, 0.8, (c.n, 2)), np.full((c.n, 1), -1.0)], 1).astype(np.float32)
    c.p1 = np.concatenate([rng.uniform(-0.8, 0.8, (c.n, 2)), np.full((c.n, 1), 8.0)], 1).astype(np.float32)
    c.rays = np.zeros(c.capacity, RAY_DTYPE)  # the queue's allocation; the device-resident size says 65
    c.rays["o"][:c.n], c.rays["d"][:c.n], c.rays["tmax"] = c.p0, c.p1 - c.p0, 1 - 1e-4
    c.rays["d"][c.n:] = (0, 0, 1)  # beyond the size: never read
    c.zero = 33
    c.rays["d"][c.zero] = 0
    c.rays["time"] = rng.random(c.capacity).astype(np.float32)
    c.Ld, c.ru, c.rl = ((rng.random((c.capacity, 4), np.float32) + 0.5).astype(np.float32) for _ in range(3))
    c.pixel = rng.permutation(c.capacity).astype(np.int32)
    c.L0 = rng.random((c.capacity, 4), np.float32).astype(np.float32)
    c.state, c.calls = walk(closest, c.verts, c.tris, c.rays[:c.n], c.cls)
    # every ray arrives; the crossing ones after 70 hits and the miss behind the last sheet
    assert (c.state == 0).all() and c.calls[c.zero] == 0 and (np.delete(c.calls, c.zero) == k + 1).all()
    c.material, c.prim_material = np.zeros(c.n, np.int32), np.zeros(len(c.tris), np.int32)
    c.hits, c.sel_rays, c.pdf, c.wsum, c.or_calls = one_random_walk(closest, c.verts, c.tris, c.p0, c.p1, c.material,
                                                                    c.prim_material)
    assert (c.or_calls == k + 1).all() and (c.wsum == k).all() and (c.hits["prim"] >= 0).all()
    return c


@pytest.mark.gpu
def test_gpu_unbounded_calls_walk_past_the_64_passes_of_the_bounded_forms():
    """71 passes of the host-driven driver: its two alternating counters and its host-sized grids, on the only walks
    that need it.  Expected values: the composed reference of test_wavefront_walk_kd.py over the oracle's closest
    hit, bit for bit."""
    import torch
    from nn_bvh_amd import BVHAggregate
    from nn_bvh_amd.interaction import ShadingMesh
    from nn_bvh_amd.wavefront import RayQueue, WavefrontAggregate
    c = sheets_case()
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    agg = BVHAggregate.from_tree(c.tree.nodes, c.tree.ordered_prims, c.verts)
    mesh = ShadingMesh(c.verts, c.tris)
    wf = WavefrontAggregate(agg, c.cls)
    q = RayQueue.from_records(c.rays, dev, shadow=True)
    q.time = t(c.rays["time"])
    q.size.fill_(c.n)
    L, state = t(c.L0), torch.full((c.capacity,), SENTINEL, dtype=torch.uint8, device=dev)
    wf.IntersectShadowTr(c.capacity, q, mesh, t(c.Ld), t(c.ru), t(c.rl), t(c.pixel), L, state)
    torch.cuda.synchronize()
    state = state.cpu().numpy()
    assert np.array_equal(state[:c.n], c.state) and (state[c.n:] == SENTINEL).all()
    live = np.concatenate([c.state, np.ones(c.capacity - c.n, np.uint8)])  # rays beyond the size add nothing
    assert L.cpu().numpy().tobytes() == shadow_radiance(live, c.Ld, c.ru, c.rl, c.pixel, c.L0).tobytes()
    # the bounded form at its limit leaves every crossing ray to the caller
    unfinished = torch.full((1,), -3, dtype=torch.int32, device=dev)
    st64 = torch.full((c.capacity,), SENTINEL, dtype=torch.uint8, device=dev)
    wf.IntersectShadowTr(c.capacity, q, mesh, t(c.Ld), t(c.ru), t(c.rl), t(c.pixel), t(c.L0), st64, max_passes=64,
                         unfinished=unfinished)
    torch.cuda.synchronize()
    assert int(unfinished.item()) == c.n - 1 and (np.delete(st64.cpu().numpy()[:c.n], c.zero) == 2).all()

    gh, gr, pdf, wsum = one_random_numpy(wf.IntersectOneRandom(c.n, t(c.p0), t(c.p1), t(c.material), mesh,
                                                               t(c.prim_material)))
    assert gh.tobytes() == c.hits.tobytes() and gr.tobytes() == c.sel_rays.tobytes()
    assert np.array_equal(pdf.view(np.uint32), c.pdf.view(np.uint32))
    assert np.array_equal(wsum.view(np.uint32), c.wsum.view(np.uint32)) and (wsum == 70).all()
    agg.close()
    mesh.close()
