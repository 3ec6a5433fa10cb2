"""Image-textured alpha (primitive kinds 16 .. 19) in two-level scenes — TEST INFRASTRUCTURE ONLY.

tests/alpha_texture_oracle.py gives each ray its own constant alphas and runs the C oracle on that ray alone with the
kinds 16 .. 19 rewritten to 4 .. 7.  In a two-level scene a triangle's alpha also depends on the placement the ray met
it through: the barycentrics are those of the instance-space ray (TransformedPrimitive / AnimatedPrimitive::Intersect
hand the transformed ray to the child aggregate, cpu/primitive.cpp:112-158), so one object shared by several placements
cannot carry one constant per triangle.  The oracle's scene therefore holds ONE COPY OF THE OBJECT PER PLACEMENT,
placement j pointing at copy j: the child trees, the instance bounds, the top-level tree and the ids are those of the
shared form, hence the results and both counters too (tests/test_two_level_alpha_texture.py proves that premise on
constant-alpha scenes, byte for byte).

Per ray i and placement j the instance-space ray is ob.apply_inverse_ray(m_inv_j, o, d, tmax)[:6] (origin and direction
do not depend on tmax); for an actually-animated placement m_inv_j is the first twelve floats of mInv from
ob.anim_interpolate at the ray's time under ob.set_sin_mode(1), which is what instance_minv does in the oracle.
Top-level textured triangles use the ray as given.  Alpha then comes from the pieces of ato.per_ray_alpha: the oracle's
batched triangle test, its triangle interaction (uvHit) and the numpy texture lookup."""
import collections

import numpy as np

import alpha_texture_oracle as ato
import oracle_binding as ob
from nn_bvh_amd import HIT_DTYPE, build_tree, instancing
from nn_bvh_amd._lib import INSTANCE_DTYPE, NODE_DTYPE, PRIM_DTYPE

F = np.float32

# top: the top-level list; objects: one primitive array per object definition; placements: (object, render_from_prim
# 3x4, prim_from_render 3x4); alpha_by_id: the constant alpha of the patches (kinds 8 .. 15) by primitive id (ids are
# unique over the scene); anims / oa: the placements' AnimatedTransforms as _lib.ANIMATED_DTYPE / ob.ANIM_DTYPE or
# None; motion: the caller's bounds [n_placements, 6] of the actually-animated placements' instance entries
Scene = collections.namedtuple("Scene", "top verts objects placements normals uvs textures alpha_by_id max_prims split "
                                        "anims oa motion")


def assemble(top_prims, verts, objects, placements, max_prims=4, split="sah", anim_flags=None, motion=None):
    """instancing.assemble_two_level (the same arrays, byte for byte, without anim_flags) where the instance entry of an
    actually-animated placement takes the caller's bounds motion[j] instead of the transformed root box.  Also returns
    the first primitive of every object's copy in the primitive array."""
    verts = np.ascontiguousarray(verts, F).reshape(-1, 3)
    children = [build_tree(o, verts, max_prims, split) for o in objects]
    n_top = len(top_prims)
    inst_prims = np.zeros(len(placements), PRIM_DTYPE)
    inst_prims["kind"] = 2
    inst_prims["v"][:, 0] = np.arange(len(placements))
    inst_prims["id"] = n_top + np.arange(len(placements))
    all_top = np.concatenate([np.asarray(top_prims, PRIM_DTYPE), inst_prims])
    bounds = np.zeros((len(all_top), 6), F)
    for j, (k, m, _) in enumerate(placements):
        if anim_flags is not None and anim_flags[j]:
            bounds[n_top + j] = motion[j]
        else:
            root = children[k].nodes[0]
            bounds[n_top + j] = instancing.transform_bounds(m, np.concatenate([root["pmin"], root["pmax"]]))
    top = build_tree(all_top, verts, max_prims, split, prim_bounds=bounds)
    nodes, prims, node_base, prim_base = [top.nodes], [top.ordered_prims], [], []
    nb, pb = len(top.nodes), len(top.ordered_prims)
    for c in children:
        node_base.append(nb)
        prim_base.append(pb)
        cn = c.nodes.copy()
        interior = cn["nprims"] == 0
        cn["offset"][interior] += nb
        cn["offset"][~interior] += pb
        nodes.append(cn)
        prims.append(c.ordered_prims)
        nb += len(cn)
        pb += len(c.ordered_prims)
    instances = np.zeros(len(placements), INSTANCE_DTYPE)
    for j, (k, m, mi) in enumerate(placements):
        instances[j]["render_from_prim"] = np.asarray(m, F).reshape(12)
        instances[j]["prim_from_render"] = np.asarray(mi, F).reshape(12)
        instances[j]["root"] = node_base[k]
        instances[j]["n_nodes"] = len(children[k].nodes)
    return (np.concatenate(nodes).astype(NODE_DTYPE), np.concatenate(prims).astype(PRIM_DTYPE), instances,
            len(top.nodes), np.array(prim_base + [pb]))


def anim_flags(s):
    return None if s.anims is None else s.anims["actually_animated"] != 0


def shared_form(s):
    """(nodes, prims, instances, n_top_nodes, first primitive per object): what the device is given"""
    return assemble(s.top, s.verts, s.objects, s.placements, s.max_prims, s.split, anim_flags(s), s.motion)


def copied_form(s):
    """... and with one copy of the object per placement, placement j pointing at copy j: what the oracle is given"""
    objects = [s.objects[k] for k, _, _ in s.placements]
    placements = [(j, m, mi) for j, (_, m, mi) in enumerate(s.placements)]
    return assemble(s.top, s.verts, objects, placements, s.max_prims, s.split, anim_flags(s), s.motion)


def ordered_alpha(s, prims):
    """the patches' constant alpha per entry of an assembled primitive array"""
    if s.alpha_by_id is None:
        return None
    return np.asarray(s.alpha_by_id, F)[prims["id"]]  # (read for the kinds 8 .. 15 only)


def instance_space_rays(s, j, rays):
    """(o, d) [n, 3] of every ray in the space of placement j"""
    n = len(rays)
    mi = np.tile(np.asarray(s.placements[j][2], F).reshape(1, 12), (n, 1))
    if s.anims is not None and s.anims[j]["actually_animated"]:
        try:
            ob.set_sin_mode(1)  # the device's Slerp sine (tests/test_animated.py: the path's documented exception)
            mi = ob.anim_interpolate(np.repeat(s.oa[j:j + 1], n), rays["time"])[:, 16:28]
        finally:
            ob.set_sin_mode(0)
    x = ob.apply_inverse_ray(mi, rays["o"], rays["d"], rays["tmax"])
    return x[:, 0:3], x[:, 3:6]


def segment_alpha(prims, verts, uvs, textures, o, d):
    """ato.per_ray_alpha on rays given as (o, d): alpha [n, T] of the T textured triangles of `prims` where ray i's line
    meets triangle j (0 elsewhere), that `met` mask, and the triangles' positions in `prims`"""
    verts = np.asarray(verts, F)
    tex = np.nonzero(ato.is_textured(prims["kind"]))[0]
    n = len(o)
    a, met = np.zeros((n, len(tex)), F), np.zeros((n, len(tex)), bool)
    if not len(tex) or not n:
        return a, met, tex
    p9 = verts[prims["v"][tex][:, :3]].reshape(len(tex), 9)
    uv6 = ato.triangle_uvs(prims[tex], uvs)
    ti = prims["v"][tex][:, 3]
    rec = np.zeros((n, len(tex), 16), F)
    rec[:, :, 0:3] = np.asarray(o, F)[:, None, :]
    rec[:, :, 3:6] = np.asarray(d, F)[:, None, :]
    rec[:, :, 6] = np.inf  # barycentrics do not depend on tMax
    rec[:, :, 7:16] = p9[None]
    hit, out = ob.leaf_batch("tri", rec.reshape(-1, 16))
    h = np.nonzero(hit)[0]
    if not len(h):
        return a, met, tex
    jj = h % len(tex)
    irec = np.zeros((len(h), 45), F)  # oracle/ref_interaction.cpp's record, as ato.per_ray_alpha fills it
    irec[:, 0:9] = p9[jj]
    irec[:, 9:12] = out[h, 0:3]
    irec[:, 12:15] = (0, 0, 1)
    irec[:, 19] = 1
    irec[:, 20:26] = uv6[jj]
    uv_hit = ob.triangle_interaction_batch(irec)[:, 6:8]
    alpha = np.zeros(len(h), F)
    for k, t in enumerate(textures):
        m = ti[jj] == k
        if m.any():
            alpha[m] = ato.lookup_uv(t, uv_hit[m, 0], uv_hit[m, 1])
    a.reshape(-1)[h] = alpha
    met.reshape(-1)[h] = True
    return a, met, tex


class TwoLevelOracle:
    """closest / any hit of a two-level scene with textured triangles: the C oracle on each ray alone, on the copied
    form.  alpha / met [n_rays, T] and tex (positions in the copied form's primitive array) cover the top-level
    list's textured triangles first, then copy 0's, copy 1's, ...; seg[c] names the copy (-1: top level) and
    src[c] the triangle's id."""

    def __init__(self, s, rays):
        self.s, self.rays = s, np.ascontiguousarray(rays)
        self.nodes, self.prims, self.instances, self.n_top, base = copied_form(s)
        n_head = len(s.top) + len(s.placements)
        a, met, tex = segment_alpha(self.prims[:n_head], s.verts, s.uvs, s.textures, rays["o"], rays["d"])
        alphas, mets, texs, segs = [a], [met], [tex], [np.full(len(tex), -1)]
        for j in range(len(s.placements)):
            o, d = instance_space_rays(s, j, self.rays)
            a, met, tex = segment_alpha(self.prims[base[j]:base[j + 1]], s.verts, s.uvs, s.textures, o, d)
            alphas.append(a)
            mets.append(met)
            texs.append(tex + base[j])
            segs.append(np.full(len(tex), j))
        self.alpha, self.met = np.concatenate(alphas, 1), np.concatenate(mets, 1)
        self.tex, self.seg = np.concatenate(texs), np.concatenate(segs)
        self.src = self.prims["id"][self.tex]
        self.a_ord = ordered_alpha(s, self.prims)

    def _each(self, fn, alpha, rays):
        work = self.prims.copy()
        work["kind"][self.tex] -= 12
        try:
            ob.set_vertex_normals(self.s.normals)
            ob.set_vertex_uvs(self.s.uvs)
            ob.set_prim_alpha(self.a_ord)
            ob.set_sin_mode(1)
            for i in range(len(rays)):
                work["v"][self.tex, 3] = alpha[i].view(np.int32)
                fn(i, work, rays[i:i + 1])
        finally:
            ob.set_sin_mode(0)
            ob.set_vertex_normals(None)
            ob.set_vertex_uvs(None)
            ob.set_prim_alpha(None)

    def closest(self, alpha=None, rays=None):
        """rays: the same rays with another tMax (alpha does not depend on it)"""
        rays = self.rays if rays is None else np.ascontiguousarray(rays)
        hits = np.zeros(len(rays), HIT_DTYPE)
        s = self.s

        def one(i, prims, ray):
            if s.anims is None:
                hits[i] = ob.closest_inst(self.nodes, prims, s.verts, self.instances, ray)[0]
            else:
                hits[i] = ob.closest_anim(self.nodes, prims, s.verts, self.instances, s.oa, ray)[0]
        self._each(one, self.alpha if alpha is None else alpha, rays)
        return hits

    def any_hit(self, alpha=None):
        n = len(self.rays)
        occ, vis, tst = np.zeros(n, np.uint8), np.zeros(n, np.int32), np.zeros(n, np.int32)
        s = self.s

        def one(i, prims, ray):
            if s.anims is None:
                o, v, t = ob.any_hit_inst(self.nodes, prims, s.verts, self.instances, ray)
            else:
                o, v, t = ob.any_hit_anim(self.nodes, prims, s.verts, self.instances, s.oa, ray)
            occ[i], vis[i], tst[i] = o[0], v[0], t[0]
        self._each(one, self.alpha if alpha is None else alpha, self.rays)
        return occ, vis, tst

    def mid_opaque(self):
        """the alphas with every 0 < a < 1 turned 1: the walk of a ray differs from the real one exactly from the first
        textured hit the hash rejected (a rejected hit is re-tested, so even a ray whose result stands has another
        prim_tests count)"""
        return np.where((self.alpha > 0) & (self.alpha < 1), F(1), self.alpha)
