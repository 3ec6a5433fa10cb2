"""Host-side mirror of the reference's batched caller interface, WavefrontAggregate
(/root/reference/src/pbrt/wavefront/integrator.h:32-54; CPU implementation
wavefront/aggregate.cpp:34-68), over include/nnbvh.h's nnbvh_wavefront_* entry points.

Queues are device-resident (torch tensors are buffers + the current stream only).  A ray queue is
the reference's SOA<Ray> (workitems.soa:40-50): six float arrays plus the queue's device-side
size; the output queues hold indices into the input queue, pushed by the device with the
reference's rules (wavefront/intersect.h:16-156).  IntersectShadowTr / IntersectOneRandom come in
their media-free form (see include/nnbvh.h)."""
import ctypes

import numpy as np
import torch

from . import _lib
from ._lib import CLOSEST_QUEUES, check, ptr
from .kdtree import KdTreeAggregate


class WorkQueue:
    """WorkQueue<T> (wavefront/workqueue.h:36-113) of int32 work-item indices on the device."""

    def __init__(self, capacity, device):
        self.capacity = int(capacity)
        self.items = torch.empty(max(self.capacity, 1), dtype=torch.int32, device=device)
        self.size = torch.zeros(1, dtype=torch.int32, device=device)

    def Reset(self):
        self.size.zero_()

    def Size(self):
        """Host read of the device counter (synchronises the current stream)."""
        return int(self.size.item())

    def indices(self):
        return self.items[:min(self.Size(), self.capacity)]

    def _wire(self, rec):
        rec["items"], rec["size"], rec["capacity"] = self.items.data_ptr(), self.size.data_ptr(), self.capacity


class RayQueue:
    """SOA ray queue: RayQueue (tmax None, has_medium optional) or ShadowRayQueue (tmax set)."""

    def __init__(self, o, d, tmax=None, time=None, has_medium=None, size=None):
        """o, d: float32 device tensors [3, capacity] (SOA: row k is the k-th coordinate array)."""
        self.o = o.contiguous()
        self.d = d.contiguous()
        assert self.o.dtype == torch.float32 and self.o.shape == self.d.shape and self.o.shape[0] == 3
        self.capacity = int(self.o.shape[1])
        self.tmax, self.time, self.has_medium = tmax, time, has_medium
        dev = self.o.device
        self.size = size if size is not None else torch.full((1,), self.capacity, dtype=torch.int32,
                                                             device=dev)

    @classmethod
    def from_records(cls, rays, device, shadow=False):
        """From a host RAY_DTYPE batch (the AoS wire format of the plain entry points)."""
        o = torch.from_numpy(np.ascontiguousarray(rays["o"].T)).to(device)
        d = torch.from_numpy(np.ascontiguousarray(rays["d"].T)).to(device)
        tmax = torch.from_numpy(np.ascontiguousarray(rays["tmax"])).to(device) if shadow else None
        return cls(o, d, tmax=tmax)

    def _wire(self):
        rec = np.zeros(1, _lib.RAY_SOA_DTYPE)
        for k, name in enumerate("xyz"):
            rec["o" + name] = self.o[k].data_ptr()
            rec["d" + name] = self.d[k].data_ptr()
        for key in ("time", "tmax", "has_medium"):
            t = getattr(self, key)
            rec[key] = t.data_ptr() if t is not None else 0
        return rec


class ItemSlices:
    """SOA slices of one work-item queue (nnbvh_item_slices): a device tensor per requested field, with
    `capacity` rows (slot k belongs to the queue's items[k]).  fields: names of _lib.ITEM_FIELDS; "prim" and
    "face_index" are int32 [capacity], the others float32 [components, capacity] (component c = slice c)."""

    def __init__(self, capacity, fields, device):
        self.capacity = int(capacity)
        self.fields = {}
        for name in fields:
            comps = _lib.ITEM_FIELDS[name]
            dtype = torch.int32 if name in ("prim", "face_index") else torch.float32
            shape = (max(self.capacity, 1),) if comps == 1 else (comps, max(self.capacity, 1))
            self.fields[name] = torch.empty(shape, dtype=dtype, device=device)

    def __getitem__(self, name):
        return self.fields[name]

    def _wire(self, rec):
        for name, t in self.fields.items():
            if _lib.ITEM_FIELDS[name] == 1:
                rec[name] = t.data_ptr()
            else:
                rec[name] = [t[c].data_ptr() for c in range(t.shape[0])]


def _items_record(items, needs_host):
    rec = np.zeros(1, _lib.CLOSEST_ITEMS_DTYPE)
    for name, sl in (items or {}).items():
        assert name in _lib.ITEM_QUEUES, f"no work-item slices for queue {name}"
        sl._wire(rec[name][0:1])
    if needs_host is not None:
        needs_host._wire(rec["needs_host"][0:1])
    return rec


def _check_shadow_args(shadow_queue, Ld, r_u, r_l, pixel_index, L):
    assert shadow_queue.tmax is not None, "a shadow queue carries tMax per item"
    for t in (Ld, r_u, r_l, L):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.shape[-1] == 4
    assert pixel_index.dtype == torch.int32 and pixel_index.is_contiguous()


def _ptr_count(t):
    """The (pointer, element count) argument pair of an optional per-primitive device tensor."""
    return (None, 0) if t is None else (t.data_ptr(), t.numel())


def _unfinished_ptr(t):
    if t is None:
        return None
    assert t.dtype == torch.int32 and t.numel() >= 1 and t.is_contiguous()
    return t.data_ptr()


def _one_bound(method, max_passes, max_surfaces):
    if max_passes is not None and max_surfaces is not None:
        raise _lib.NNBVHError(f"WavefrontAggregate.{method}: max_passes (the bounded pass form) and max_surfaces (the "
                              "walk inside one trace launch) are two forms of the call: pass one of them")


def _queues_record(queues):
    qrec = np.zeros(1, _lib.CLOSEST_QUEUES_DTYPE)
    for name, q in queues.items():
        assert name in CLOSEST_QUEUES, name
        if q is not None:
            q._wire(qrec[name][0:1])
    return qrec


class HostCandidateArrays:
    """Device arrays of nnbvh_host_candidates for a queue of `n` rays: count / before int32 [n], prim / instance
    int32 [n, capacity] (entries beyond count keep their -1)."""

    def __init__(self, n, capacity, device):
        self.capacity = int(capacity)
        n = max(int(n), 1)
        self.count = torch.zeros(n, dtype=torch.int32, device=device)
        self.before = torch.zeros(n, dtype=torch.int32, device=device)
        self.prim = torch.full((n, self.capacity), -1, dtype=torch.int32, device=device)
        self.instance = torch.full((n, self.capacity), -1, dtype=torch.int32, device=device)

    def _wire(self):
        return _lib.HostCandidates(self.capacity, self.count.data_ptr(), self.before.data_ptr(),
                                   self.prim.data_ptr(), self.instance.data_ptr())

    def numpy(self):
        """Host copy as a candidates_dtype(capacity) array (synchronises)."""
        from .aggregate import _pack_candidates
        return _pack_candidates(self.count.cpu().numpy(), self.before.cpu().numpy(), self.prim.cpu().numpy(),
                                self.instance.cpu().numpy())


def enqueue_closest_items(shading_mesh, max_rays, ray_queue, hits, prim_class=None, items=None, needs_host=None,
                          index=None, **queues):
    """nnbvh_wavefront_enqueue_closest_items_device: IntersectClosest's enqueue with the work items for hit
    records from any source (hits: device tensor of HIT_DTYPE rows).  queues: WorkQueues by
    _lib.CLOSEST_QUEUES name; items: ItemSlices by _lib.ITEM_QUEUES name; needs_host: WorkQueue or None.
    index: a WorkQueue of ray indices: only those rays are enqueued, appended to the queues
    (nnbvh_wavefront_enqueue_closest_items_indexed_device; the second pass of the host-candidates loop)."""
    dev = ray_queue.o.device
    pc = prim_class
    # the records must outlive the call: ptr() does not keep its array alive
    soa, qrec, irec = ray_queue._wire(), _queues_record(queues), _items_record(items, needs_host)
    if index is not None:
        check(_lib.lib().nnbvh_wavefront_enqueue_closest_items_indexed_device(
            shading_mesh._h, int(max_rays), ptr(soa), index.items.data_ptr(), index.size.data_ptr(),
            int(index.capacity), hits.data_ptr(), *_ptr_count(pc), ptr(qrec), ptr(irec),
            torch.cuda.current_stream(dev).cuda_stream),
            "nnbvh_wavefront_enqueue_closest_items_indexed_device")
        return
    check(_lib.lib().nnbvh_wavefront_enqueue_closest_items_device(
        shading_mesh._h, int(max_rays), ptr(soa), ray_queue.size.data_ptr(), hits.data_ptr(), *_ptr_count(pc),
        ptr(qrec), ptr(irec), torch.cuda.current_stream(dev).cuda_stream),
        "nnbvh_wavefront_enqueue_closest_items_device")


def record_shadow(max_rays, shadow_queue, occluded, Ld, r_u, r_l, pixel_index, L):
    """nnbvh_wavefront_record_shadow_device: RecordShadowRayResult for a per-ray uint8 `occluded` array (entries
    that are not 0 add nothing).  In the host-candidates loop: 1 everywhere but 0 on the rays the caller resolved
    as unoccluded."""
    dev = L.device
    check(_lib.lib().nnbvh_wavefront_record_shadow_device(
        occluded.data_ptr(), int(max_rays), shadow_queue.size.data_ptr(), Ld.data_ptr(), r_u.data_ptr(),
        r_l.data_ptr(), pixel_index.data_ptr(), L.data_ptr(), L.shape[0], dev.index or 0,
        torch.cuda.current_stream(dev).cuda_stream), "nnbvh_wavefront_record_shadow_device")


class WavefrontAggregate:
    """IntersectClosest / IntersectShadow of wavefront/integrator.h:32-54 on one BVHAggregate or KdTreeAggregate
    (a kd scene offers the five queue calls, the three *WithCandidates ones and WalkShadowTr / WalkOneRandom;
    IntersectShadowTr and IntersectOneRandom raise NNBVHError for it, WalkShadowTr / WalkOneRandom for a BVH scene).

    prim_class: optional uint8 per primitive id (nn_bvh_amd._lib.CLASS_*), what the reference
    reads off the hit's SurfaceInteraction when it decides the destination queues."""

    def __init__(self, aggregate, prim_class=None):
        self.aggregate = aggregate
        # a KdTreeAggregate binds the nnbvh_kd_wavefront_* entry points: the same argument lists on a kd scene
        self._prefix = "nnbvh_kd_wavefront_" if isinstance(aggregate, KdTreeAggregate) else "nnbvh_wavefront_"
        self.device = torch.device("cuda", aggregate.device)
        self.prim_class = None
        if prim_class is not None:
            self.prim_class = torch.from_numpy(np.ascontiguousarray(prim_class, np.uint8)).to(self.device)

    def Bounds(self):
        return self.aggregate.Bounds()

    def _name(self, call):
        return self._prefix + call

    def _entry(self, call):
        return getattr(_lib.lib(), self._prefix + call)

    def _bvh_only(self, method):
        if self._prefix != "nnbvh_wavefront_":
            raise _lib.NNBVHError(f"WavefrontAggregate.{method} is not offered for kd-tree scenes (DESIGN.md §8): "
                                  f"call Walk{method[len('Intersect'):]} (the walk inside one trace launch), or bind "
                                  "a BVH aggregate")

    def _kd_only(self, method):
        if self._prefix != "nnbvh_kd_wavefront_":
            raise _lib.NNBVHError(f"WavefrontAggregate.{method} is not offered for BVH scenes (DESIGN.md §8): call "
                                  f"Intersect{method[len('Walk'):]} with max_surfaces (the walk inside one BVH trace "
                                  "launch) or with max_passes")

    def IntersectClosest(self, max_rays, ray_queue, escaped=None, hit_area_light=None,
                         basic_eval_material=None, universal_eval_material=None, medium_sample=None,
                         next_ray=None, hits=None):
        """Traces ray_queue[0 : min(max_rays, size)] and pushes each item's index to the queues
        the reference would (a None queue drops its pushes).  Returns the device hit records
        (HIT_DTYPE rows as a uint8 tensor [max_rays, 32]); asynchronous on the current stream."""
        if hits is None:
            hits = torch.empty((max(int(max_rays), 1), 32), dtype=torch.uint8, device=self.device)
        qrec = _queues_record(dict(zip(CLOSEST_QUEUES, (escaped, hit_area_light, basic_eval_material,
                                                        universal_eval_material, medium_sample, next_ray))))
        soa = ray_queue._wire()
        pc = self.prim_class
        check(self._entry("intersect_closest")(
            self.aggregate._h, int(max_rays), ptr(soa), ray_queue.size.data_ptr(), *_ptr_count(pc),
            hits.data_ptr(), ptr(qrec), torch.cuda.current_stream(self.device).cuda_stream),
            self._name("intersect_closest"))
        return hits

    def IntersectShadow(self, max_rays, shadow_queue, Ld, r_u, r_l, pixel_index, L, occluded=None):
        """Traces the shadow queue and adds Ld / (r_u + r_l).Average() to L[pixel_index] for the
        unoccluded rays (RecordShadowRayResult, wavefront/intersect.h:32-47).  Ld, r_u, r_l:
        float32 [capacity, 4]; L: float32 [n_pixels, 4]; all device tensors."""
        _check_shadow_args(shadow_queue, Ld, r_u, r_l, pixel_index, L)
        soa = shadow_queue._wire()
        check(self._entry("intersect_shadow")(
            self.aggregate._h, int(max_rays), ptr(soa), shadow_queue.size.data_ptr(), Ld.data_ptr(),
            r_u.data_ptr(), r_l.data_ptr(), pixel_index.data_ptr(), L.data_ptr(), L.shape[0],
            occluded.data_ptr() if occluded is not None else None,
            torch.cuda.current_stream(self.device).cuda_stream),
            self._name("intersect_shadow"))

    def IntersectClosestAndShadow(self, max_rays, ray_queue, max_shadow_rays, shadow_queue, Ld, r_u, r_l, pixel_index,
                                  L, escaped=None, hit_area_light=None, basic_eval_material=None,
                                  universal_eval_material=None, medium_sample=None, next_ray=None, hits=None,
                                  occluded=None):
        """IntersectShadow(max_shadow_rays, shadow_queue, ...) of one depth and IntersectClosest(max_rays, ray_queue,
        ...) of the next in ONE launch of the traversal kernel (both queues come out of the same shading pass and
        neither reads what the other writes: wavefront/integrator.cpp's render loop).  Same results as the two calls.
        Returns the hit records."""
        _check_shadow_args(shadow_queue, Ld, r_u, r_l, pixel_index, L)
        if hits is None:
            hits = torch.empty((max(int(max_rays), 1), 32), dtype=torch.uint8, device=self.device)
        qrec = _queues_record(dict(zip(CLOSEST_QUEUES, (escaped, hit_area_light, basic_eval_material,
                                                        universal_eval_material, medium_sample, next_ray))))
        soa, ssoa = ray_queue._wire(), shadow_queue._wire()
        pc = self.prim_class
        check(self._entry("intersect_closest_and_shadow")(
            self.aggregate._h, int(max_rays), ptr(soa), ray_queue.size.data_ptr(), *_ptr_count(pc), hits.data_ptr(),
            ptr(qrec), int(max_shadow_rays), ptr(ssoa), shadow_queue.size.data_ptr(), Ld.data_ptr(), r_u.data_ptr(),
            r_l.data_ptr(), pixel_index.data_ptr(), L.data_ptr(), L.shape[0],
            occluded.data_ptr() if occluded is not None else None,
            torch.cuda.current_stream(self.device).cuda_stream), self._name("intersect_closest_and_shadow"))
        return hits

    def IntersectClosestItems(self, max_rays, ray_queue, shading_mesh, items=None, needs_host=None, hits=None,
                              **queues):
        """IntersectClosest with the work items themselves (nnbvh_wavefront_intersect_closest_items): the index
        queues as IntersectClosest fills them (keyword arguments by _lib.CLOSEST_QUEUES name), and for the queues
        in `items` (ItemSlices by _lib.ITEM_QUEUES name) the SOA payload of each pushed item, computed from
        shading_mesh.  Voided records and hits the mesh cannot finish go to needs_host (a WorkQueue, or None to
        drop them).  hits: optional device tensor for the hit records (else a library workspace holds them).
        Returns hits."""
        pc = self.prim_class
        soa, qrec, irec = ray_queue._wire(), _queues_record(queues), _items_record(items, needs_host)
        check(self._entry("intersect_closest_items")(
            self.aggregate._h, shading_mesh._h, int(max_rays), ptr(soa), ray_queue.size.data_ptr(),
            *_ptr_count(pc), hits.data_ptr() if hits is not None else None, ptr(qrec), ptr(irec),
            torch.cuda.current_stream(self.device).cuda_stream),
            self._name("intersect_closest_items"))
        return hits

    def IntersectClosestAndShadowItems(self, max_rays, ray_queue, shading_mesh, max_shadow_rays, shadow_queue, Ld,
                                       r_u, r_l, pixel_index, L, items=None, needs_host=None, hits=None,
                                       occluded=None, **queues):
        """IntersectClosestAndShadow with the closest side's work items (see IntersectClosestItems)."""
        _check_shadow_args(shadow_queue, Ld, r_u, r_l, pixel_index, L)
        pc = self.prim_class
        soa, ssoa = ray_queue._wire(), shadow_queue._wire()
        qrec, irec = _queues_record(queues), _items_record(items, needs_host)
        check(self._entry("intersect_closest_and_shadow_items")(
            self.aggregate._h, shading_mesh._h, int(max_rays), ptr(soa), ray_queue.size.data_ptr(),
            *_ptr_count(pc), hits.data_ptr() if hits is not None else None, ptr(qrec), ptr(irec),
            int(max_shadow_rays), ptr(ssoa),
            shadow_queue.size.data_ptr(), Ld.data_ptr(), r_u.data_ptr(), r_l.data_ptr(), pixel_index.data_ptr(),
            L.data_ptr(), L.shape[0], occluded.data_ptr() if occluded is not None else None,
            torch.cuda.current_stream(self.device).cuda_stream), self._name("intersect_closest_and_shadow_items"))
        return hits

    def IntersectClosestItemsWithCandidates(self, max_rays, ray_queue, shading_mesh, candidates, hits, items=None,
                                            needs_host=None, **queues):
        """IntersectClosestItems that lists the host-only primitives a ray reached instead of voiding it
        (nnbvh_wavefront_intersect_closest_items_candidates).  candidates: HostCandidateArrays of the queue's
        capacity; hits (required): device tensor of HIT_DTYPE rows.  Rays with count 0 are routed as
        IntersectClosestItems routes them; the others go to needs_host only, their candidate-mode record in hits:
        resolve them (resolve_host_candidates), write the merged records back and enqueue them with
        enqueue_closest_items(index=needs_host)."""
        pc = self.prim_class
        soa, qrec, irec = ray_queue._wire(), _queues_record(queues), _items_record(items, needs_host)
        c = candidates._wire()
        check(self._entry("intersect_closest_items_candidates")(
            self.aggregate._h, shading_mesh._h, int(max_rays), ptr(soa), ray_queue.size.data_ptr(),
            *_ptr_count(pc), hits.data_ptr(), ptr(qrec),
            ptr(irec), ctypes.byref(c), torch.cuda.current_stream(self.device).cuda_stream),
            self._name("intersect_closest_items_candidates"))
        return hits

    def IntersectShadowWithCandidates(self, max_rays, shadow_queue, Ld, r_u, r_l, pixel_index, L, occluded,
                                      candidates):
        """IntersectShadow with host candidates (nnbvh_wavefront_intersect_shadow_candidates): occluded (required,
        uint8 [capacity]) gets 0 / 1 / 2; rays with 0 add to L, rays with 2 and count > 0 are the caller's to test
        (resolve_host_candidates_any) and to record with record_shadow."""
        _check_shadow_args(shadow_queue, Ld, r_u, r_l, pixel_index, L)
        soa, c = shadow_queue._wire(), candidates._wire()
        check(self._entry("intersect_shadow_candidates")(
            self.aggregate._h, int(max_rays), ptr(soa), shadow_queue.size.data_ptr(), Ld.data_ptr(), r_u.data_ptr(),
            r_l.data_ptr(), pixel_index.data_ptr(), L.data_ptr(), L.shape[0], occluded.data_ptr(), ctypes.byref(c),
            torch.cuda.current_stream(self.device).cuda_stream), self._name("intersect_shadow_candidates"))

    def IntersectClosestAndShadowItemsWithCandidates(self, max_rays, ray_queue, shading_mesh, candidates, hits,
                                                     max_shadow_rays, shadow_queue, Ld, r_u, r_l, pixel_index, L,
                                                     occluded, shadow_candidates, items=None, needs_host=None,
                                                     **queues):
        """IntersectClosestItemsWithCandidates and IntersectShadowWithCandidates in ONE launch of the traversal
        kernel (nnbvh_wavefront_intersect_closest_and_shadow_items_candidates); same results as the two calls."""
        _check_shadow_args(shadow_queue, Ld, r_u, r_l, pixel_index, L)
        pc = self.prim_class
        soa, ssoa = ray_queue._wire(), shadow_queue._wire()
        qrec, irec = _queues_record(queues), _items_record(items, needs_host)
        c, sc = candidates._wire(), shadow_candidates._wire()
        check(self._entry("intersect_closest_and_shadow_items_candidates")(
            self.aggregate._h, shading_mesh._h, int(max_rays), ptr(soa), ray_queue.size.data_ptr(),
            *_ptr_count(pc), hits.data_ptr(), ptr(qrec),
            ptr(irec), ctypes.byref(c), int(max_shadow_rays), ptr(ssoa), shadow_queue.size.data_ptr(), Ld.data_ptr(),
            r_u.data_ptr(), r_l.data_ptr(), pixel_index.data_ptr(), L.data_ptr(), L.shape[0], occluded.data_ptr(),
            ctypes.byref(sc), torch.cuda.current_stream(self.device).cuda_stream),
            self._name("intersect_closest_and_shadow_items_candidates"))
        return hits

    def _shadow_tr_args(self, max_rays, shadow_queue, shading_mesh, Ld, r_u, r_l, pixel_index, L, state):
        """The arguments every IntersectShadowTr entry point starts with (scene to d_state), and the queue's wire
        record, which the caller keeps alive over the call."""
        _check_shadow_args(shadow_queue, Ld, r_u, r_l, pixel_index, L)
        soa = shadow_queue._wire()
        return (self.aggregate._h, shading_mesh._h, int(max_rays), ptr(soa), shadow_queue.size.data_ptr(),
                *_ptr_count(self.prim_class), Ld.data_ptr(), r_u.data_ptr(), r_l.data_ptr(), pixel_index.data_ptr(),
                L.data_ptr(), L.shape[0], state.data_ptr() if state is not None else None), soa

    def _one_random_args(self, max_items, p0, p1, material, shading_mesh, prim_material, size):
        """IntersectOneRandom's inputs checked, its four result tensors, and the arguments every one of its entry
        points starts with (scene to d_weight_sum)."""
        for t in (p0, p1):
            assert t.dtype == torch.float32 and t.is_contiguous() and t.shape[-1] == 3
        assert material.dtype == torch.int32 and material.is_contiguous()
        n = int(max_items)
        sel_hits = torch.empty((max(n, 1), 32), dtype=torch.uint8, device=self.device)
        sel_rays = torch.empty((max(n, 1), 32), dtype=torch.uint8, device=self.device)
        pdf = torch.zeros(max(n, 1), dtype=torch.float32, device=self.device)
        wsum = torch.zeros(max(n, 1), dtype=torch.float32, device=self.device)
        args = (self.aggregate._h, shading_mesh._h, n, p0.data_ptr(), p1.data_ptr(), material.data_ptr(),
                size.data_ptr() if size is not None else None, *_ptr_count(prim_material), sel_hits.data_ptr(),
                sel_rays.data_ptr(), pdf.data_ptr(), wsum.data_ptr())
        return (sel_hits, sel_rays, pdf, wsum), args

    def IntersectShadowTr(self, max_rays, shadow_queue, shading_mesh, Ld, r_u, r_l, pixel_index, L, state=None,
                          max_passes=None, unfinished=None, max_surfaces=None):
        """IntersectShadowTr (wavefront/aggregate.cpp:70-88, TraceTransmittance of wavefront/intersect.h:
        164-274) without media: shadow rays pass through interface surfaces (CLASS_INTERFACE) and are
        blocked by the first surface with a material; arriving rays add Ld * (1 / (r_u + r_l).Average())
        to L[pixel_index].  state: optional uint8 [capacity] out (0 arrived, 1 blocked, 2 host).

        max_passes None: the host-driven loop (reads a count per pass; not graph-capturable).  max_passes 1..64:
        nnbvh_wavefront_intersect_shadow_tr_bounded — exactly that many passes, kernel launches only (capturable
        after one warm-up call); a ray whose walk needs more Intersect calls gets state 2 and adds nothing.
        unfinished: optional int32 [1] device tensor, receives the number of such rays.
        max_surfaces 1..65536 (not together with max_passes): nnbvh_wavefront_walk_shadow_tr — the walk inside ONE
        trace launch, five kernel launches whatever the bound (capturable after one warm-up call); a ray whose walk
        would start one more Intersect call gets state 2, adds nothing and is counted in unfinished."""
        self._bvh_only("IntersectShadowTr")
        _one_bound("IntersectShadowTr", max_passes, max_surfaces)
        args, _soa = self._shadow_tr_args(max_rays, shadow_queue, shading_mesh, Ld, r_u, r_l, pixel_index, L, state)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        if max_surfaces is not None:
            check(_lib.lib().nnbvh_wavefront_walk_shadow_tr(
                *args, int(max_surfaces), _unfinished_ptr(unfinished), stream), "nnbvh_wavefront_walk_shadow_tr")
        elif max_passes is None:
            assert unfinished is None, "unfinished belongs to the bounded form: pass max_passes"
            check(_lib.lib().nnbvh_wavefront_intersect_shadow_tr(*args, stream), "nnbvh_wavefront_intersect_shadow_tr")
        else:
            check(_lib.lib().nnbvh_wavefront_intersect_shadow_tr_bounded(
                *args, int(max_passes), _unfinished_ptr(unfinished), stream),
                "nnbvh_wavefront_intersect_shadow_tr_bounded")

    def IntersectOneRandom(self, max_items, p0, p1, material, shading_mesh, prim_material=None, size=None,
                           max_passes=None, unfinished=None, max_surfaces=None):
        """IntersectOneRandom (wavefront/aggregate.cpp:90-116): p0, p1 float32 [n, 3], material int32 [n]
        device tensors; prim_material int32 per primitive id.  Returns (selected hit records uint8
        [n, 32], their segment rays uint8 [n, 32], reservoir pdf float32 [n], weight sum float32 [n]).

        max_passes None: the host-driven loop.  max_passes 1..64: nnbvh_wavefront_intersect_one_random_bounded —
        exactly that many passes, kernel launches only; an item whose segment needs more Intersect calls gets
        instance = -1 in its selected hit record (its pdf, weight sum and ray are then unspecified).
        unfinished: optional int32 [1] device tensor, receives the number of such items.
        max_surfaces 1..65536 (not together with max_passes): nnbvh_wavefront_walk_one_random — the walk inside ONE
        trace launch; an item whose segment would start one more Intersect call gets instance = -1 and is counted."""
        self._bvh_only("IntersectOneRandom")
        _one_bound("IntersectOneRandom", max_passes, max_surfaces)
        results, args = self._one_random_args(max_items, p0, p1, material, shading_mesh, prim_material, size)
        stream = torch.cuda.current_stream(self.device).cuda_stream
        if max_surfaces is not None:
            check(_lib.lib().nnbvh_wavefront_walk_one_random(
                *args, int(max_surfaces), _unfinished_ptr(unfinished), stream), "nnbvh_wavefront_walk_one_random")
        elif max_passes is None:
            assert unfinished is None, "unfinished belongs to the bounded form: pass max_passes"
            check(_lib.lib().nnbvh_wavefront_intersect_one_random(*args, stream), "nnbvh_wavefront_intersect_one_random")
        else:
            check(_lib.lib().nnbvh_wavefront_intersect_one_random_bounded(
                *args, int(max_passes), _unfinished_ptr(unfinished), stream),
                "nnbvh_wavefront_intersect_one_random_bounded")
        return results

    def WalkShadowTr(self, max_rays, shadow_queue, shading_mesh, Ld, r_u, r_l, pixel_index, L, state=None,
                     max_surfaces=65536, unfinished=None):
        """IntersectShadowTr on a KdTreeAggregate, walked inside ONE trace launch (nnbvh_kd_wavefront_walk_shadow_tr):
        the arguments and results of IntersectShadowTr(max_passes=...), with max_surfaces (1..65536) Intersect calls
        per ray in the place of the passes.  A ray whose walk would start one more call gets state 2, adds nothing
        and is counted in unfinished (optional int32 [1] device tensor).  Kernel launches only: capturable after one
        warm-up call with the same max_rays."""
        self._kd_only("WalkShadowTr")
        args, _soa = self._shadow_tr_args(max_rays, shadow_queue, shading_mesh, Ld, r_u, r_l, pixel_index, L, state)
        check(_lib.lib().nnbvh_kd_wavefront_walk_shadow_tr(
            *args, int(max_surfaces), _unfinished_ptr(unfinished), torch.cuda.current_stream(self.device).cuda_stream),
            "nnbvh_kd_wavefront_walk_shadow_tr")

    def WalkOneRandom(self, max_items, p0, p1, material, shading_mesh, prim_material=None, size=None,
                      max_surfaces=65536, unfinished=None):
        """IntersectOneRandom on a KdTreeAggregate, walked inside ONE trace launch
        (nnbvh_kd_wavefront_walk_one_random): the arguments and the four returned tensors of
        IntersectOneRandom(max_passes=...), with max_surfaces (1..65536) Intersect calls per item in the place of the
        passes.  An item whose segment would start one more call gets instance = -1 in its selected hit record and
        is counted in unfinished."""
        self._kd_only("WalkOneRandom")
        results, args = self._one_random_args(max_items, p0, p1, material, shading_mesh, prim_material, size)
        check(_lib.lib().nnbvh_kd_wavefront_walk_one_random(
            *args, int(max_surfaces), _unfinished_ptr(unfinished), torch.cuda.current_stream(self.device).cuda_stream),
            "nnbvh_kd_wavefront_walk_one_random")
        return results
