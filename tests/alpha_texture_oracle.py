"""Image-textured alpha on triangles (primitive kinds 16 .. 19) — TEST INFRASTRUCTURE ONLY.

The oracle needs no new traversal code.  A textured triangle's alpha depends only on the ray as given and on the
triangle (the barycentrics of a hit do not depend on tMax, and the re-traced ray never evaluates alpha again), so for
ray i the alpha a[i][j] of every textured triangle j is computed here, outside the oracle:

  * barycentrics from the oracle's batched triangle test (ob.leaf_batch, pinned to the compiled reference);
  * uvHit from ob.triangle_interaction_batch (pinned to oracle/ref_interaction.cpp);
  * the texture lookup by `lookup` below: a numpy float32 restatement of FloatImageTexture::Evaluate with zero
    differentials (textures.h:579-590, util/mipmap.cpp:229-284, util/image.h:96-146, 279-292), the fifteen operations of
    nn_bvh_amd/csrc/alpha_texture_math.h.  It is the one piece with no compiled reference behind it.

Then the C oracle runs on ray i alone with kinds 16 .. 19 rewritten to 4 .. 7 and v[3] = bits(a[i][j])."""
import numpy as np

import oracle_binding as ob
from nn_bvh_amd import HIT_DTYPE, AlphaTexture

F = np.float32
REPEAT, CLAMP, BLACK = 0, 1, 2


def is_textured(kinds):
    return (kinds >= 16) & (kinds <= 19)


# ---- the lookup --------------------------------------------------------------------------------------------------------
def _to_int(f):
    """int(floor(x)) / int(round(x)), saturating as alpha_texture_math.h's atex_to_int does"""
    f = np.where(np.isnan(f), F(0), f)
    return np.clip(f.astype(np.float64), -2147483648.0, 2147483646.0).astype(np.int64)


def _round_half_away(x):
    r = np.trunc(x)
    return np.where(np.abs(x - r) >= F(0.5), r + np.copysign(F(1), x), r).astype(F)  # x - trunc(x) is exact


def _remap(p, res, wrap):
    """RemapPixelCoords on one coordinate: (index, inside)"""
    if wrap == REPEAT:
        q = np.abs(p) // res * np.sign(p)  # C's truncating division
        r = p - q * res
        return np.where(r < 0, r + res, r), np.ones(p.shape, bool)
    if wrap == CLAMP:
        return np.clip(p, 0, res - 1), np.ones(p.shape, bool)
    inside = (p >= 0) & (p < res)
    return np.where(inside, p, 0), inside


def _texel(t, x, y):
    xi, okx = _remap(x, t.width, t.wrap)
    yi, oky = _remap(y, t.height, t.wrap)
    return np.where(okx & oky, t.image[yi, xi], F(0)).astype(F)


def taps(t, st_s, st_t):
    """the (x, y) tap coordinates before remapping, int64 [n, k, 2] (k = 1 point filter, 4 bilinear)"""
    if t.point_filter:
        xi = _to_int(_round_half_away(st_s * F(t.width) - F(0.5)))
        yi = _to_int(_round_half_away(st_t * F(t.height) - F(0.5)))
        return np.stack([xi, yi], -1)[:, None, :]
    xi = _to_int(np.floor(st_s * F(t.width) - F(0.5)))
    yi = _to_int(np.floor(st_t * F(t.height) - F(0.5)))
    return np.stack([np.stack([xi, yi], -1), np.stack([xi + 1, yi], -1), np.stack([xi, yi + 1], -1),
                     np.stack([xi + 1, yi + 1], -1)], 1)


def st_of(t, b, uv6):
    b, uv6 = np.asarray(b, F), np.asarray(uv6, F)
    u = (b[:, 0] * uv6[:, 0] + b[:, 1] * uv6[:, 2]) + b[:, 2] * uv6[:, 4]
    v = (b[:, 0] * uv6[:, 1] + b[:, 1] * uv6[:, 3]) + b[:, 2] * uv6[:, 5]
    return uv_to_st(t, u, v)


def uv_to_st(t, u, v):
    s = F(t.su) * u + F(t.du)
    tt = F(t.sv) * v + F(t.dv)
    return s.astype(F), (F(1) - tt).astype(F)


def lookup_uv(t, u, v):
    """FloatImageTexture::Evaluate at uvHit = (u, v), float32 in and out"""
    with np.errstate(all="ignore"):
        s, tt = uv_to_st(t, np.asarray(u, F), np.asarray(v, F))
        if t.point_filter:
            xy = taps(t, s, tt)
            val = _texel(t, xy[:, 0, 0], xy[:, 0, 1])
        else:
            x, y = s * F(t.width) - F(0.5), tt * F(t.height) - F(0.5)
            xi, yi = _to_int(np.floor(x)), _to_int(np.floor(y))
            dx, dy = x - xi.astype(F), y - yi.astype(F)
            t00, t10 = _texel(t, xi, yi), _texel(t, xi + 1, yi)
            t01, t11 = _texel(t, xi, yi + 1), _texel(t, xi + 1, yi + 1)
            one = F(1)
            val = (((one - dx) * (one - dy) * t00 + dx * (one - dy) * t10) + (one - dx) * dy * t01) + dx * dy * t11
        val = (F(t.scale) * val).astype(F)
        if t.invert:
            w = F(1) - val
            val = np.where(F(0) < w, w, F(0))
        return val.astype(F)


def lookup(textures, tex_index, b, uv6):
    """alpha of records (barycentrics [n, 3], the triangle's (u, v) pairs [n, 6], texture index [n])"""
    b, uv6 = np.asarray(b, F), np.asarray(uv6, F)
    out = np.zeros(len(b), F)
    with np.errstate(all="ignore"):
        u = (b[:, 0] * uv6[:, 0] + b[:, 1] * uv6[:, 2]) + b[:, 2] * uv6[:, 4]
        v = (b[:, 0] * uv6[:, 1] + b[:, 1] * uv6[:, 3]) + b[:, 2] * uv6[:, 5]
    for k, t in enumerate(textures):
        m = tex_index == k
        if m.any():
            out[m] = lookup_uv(t, u[m], v[m])
    return out


# ---- record files of the stand-alone header checks (tests/cpp/alpha_texture_check.cpp, tests/hip/...) -------------------
def write_records(path, textures, tex_index, b, uv6):
    """int32 n_textures, n_records; per texture 10 words (width, height, wrap, point_filter as int32; su, sv, du, dv,
    scale as float32; invert as int32); the texels of all textures; per record 10 float32 (b, uv6, texture index)"""
    with open(path, "wb") as f:
        f.write(np.array([len(textures), len(b)], np.int32).tobytes())
        for t in textures:
            f.write(np.array([t.width, t.height, t.wrap, t.point_filter], np.int32).tobytes())
            f.write(np.array([t.su, t.sv, t.du, t.dv, t.scale], F).tobytes())
            f.write(np.array([t.invert], np.int32).tobytes())
        for t in textures:
            f.write(t.image.tobytes())
        rec = np.concatenate([np.asarray(b, F), np.asarray(uv6, F), np.asarray(tex_index, F)[:, None]], 1)
        f.write(np.ascontiguousarray(rec, F).tobytes())


DEFAULT_UV = np.array([0, 0, 1, 0, 1, 1], F)


def check_textures(shape_seed=0):
    """the header tests' textures: 1x1, 1x7 (one column), 5x3 and 64x64 images of random values, a 0/1 checker and a
    ramp, over all three wraps, the point filter, invert, scale 0.5 / 1 / 2, su / sv of 1, 3.7 and -2, nonzero du / dv"""
    rng = np.random.default_rng(shape_seed)
    out = []
    shapes = [(1, 1), (7, 1), (3, 5), (64, 64)]  # (height, width)
    k = 0
    for h, w in shapes:
        yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
        images = [rng.random((h, w)).astype(F), ((xx + yy) % 2).astype(F), ((xx + w * yy) / F(max(w * h - 1, 1))).astype(F)]
        for img in images:
            for wrap in (REPEAT, CLAMP, BLACK):
                su, sv = [(1.0, 1.0), (3.7, -2.0), (-2.0, 3.7)][k % 3]
                du, dv = [(0.0, 0.0), (0.25, -0.6), (-1.3, 0.1)][(k // 3) % 3]
                out.append(AlphaTexture(img, wrap=wrap, point_filter=(k % 4 == 3), su=su, sv=sv, du=du, dv=dv,
                                        scale=[1.0, 0.5, 2.0][(k // 2) % 3], invert=(k % 5 == 2)))
                k += 1
    return out


def check_records(textures, seed=1, per_texture=96):
    """(tex_index, b, uv6) families: uvHit exactly 0 and 1, on texel centres (dx = 0), one ulp either side of a texel
    edge, anywhere in [-3, 4], and random barycentrics over random and the default corner triples"""
    rng = np.random.default_rng(seed)
    ti, bs, uvs = [], [], []
    for k, t in enumerate(textures):
        n = per_texture
        # families 0 .. 3 fix uvHit through b = (1, 0, 0) and uv0 = the wanted (u, v)
        u, v = np.zeros(n, F), np.zeros(n, F)
        fam = np.arange(n) % 6
        u[:], v[:] = rng.uniform(-3, 4, n), rng.uniform(-3, 4, n)
        m = fam == 0
        u[m], v[m] = rng.choice([0.0, 1.0], m.sum()), rng.choice([0.0, 1.0], m.sum())
        # texel centres and edges in st, mapped back through the UVMapping (approximately: the family only has to land
        # near them; exact landings come from the identity mappings)
        cx = (rng.integers(-t.width, 2 * t.width, n) + 0.5) / t.width
        cy = (rng.integers(-t.height, 2 * t.height, n) + 0.5) / t.height
        ex = rng.integers(-t.width, 2 * t.width + 1, n) / t.width
        ey = rng.integers(-t.height, 2 * t.height + 1, n) / t.height
        for mask, sx, sy in ((fam == 1, cx, cy), (fam == 2, ex, ey)):
            uu = ((sx - t.du) / t.su).astype(F)
            vv = (((1 - sy) - t.dv) / t.sv).astype(F)
            u[mask], v[mask] = uu[mask], vv[mask]
        m = fam == 2  # one ulp either side of the edge
        step = rng.integers(-1, 2, n)
        u[m] = np.where(step[m] < 0, np.nextafter(u[m], F(-np.inf)), np.where(step[m] > 0, np.nextafter(u[m], F(np.inf)), u[m]))
        v[m] = np.where(step[m] > 0, np.nextafter(v[m], F(-np.inf)), np.where(step[m] < 0, np.nextafter(v[m], F(np.inf)), v[m]))
        b = np.zeros((n, 3), F)
        b[:, 0] = 1
        uv6 = np.zeros((n, 6), F)
        uv6[:, 0], uv6[:, 1] = u, v
        uv6[:, 2:] = rng.uniform(-3, 4, (n, 4))
        # families 4 / 5: random barycentrics (as the triangle test makes them: b2 is not 1 - b0 - b1 exactly) over a
        # random triple / the default corners
        m = fam >= 4
        bb = rng.dirichlet([1, 1, 1], n).astype(F)
        b[m] = bb[m]
        uv6[fam == 5] = DEFAULT_UV
        ti.append(np.full(n, k, np.int32))
        bs.append(b)
        uvs.append(uv6)
    return np.concatenate(ti), np.concatenate(bs), np.concatenate(uvs)


def branch_shares(textures, tex_index, b, uv6):
    """share of the records on which each branch of the lookup is taken (the CPU test asserts every one is > 0)"""
    n = len(b)
    neg = np.zeros(n, bool)
    past = {REPEAT: np.zeros(n, bool), CLAMP: np.zeros(n, bool), BLACK: np.zeros(n, bool)}
    for k, t in enumerate(textures):
        m = np.nonzero(tex_index == k)[0]
        if not len(m):
            continue
        s, tt = st_of(t, b[m], uv6[m])
        xy = taps(t, s, tt)
        neg[m] = (xy < 0).any((1, 2))
        past[t.wrap][m] = (xy[:, :, 0] >= t.width).any(1) | (xy[:, :, 1] >= t.height).any(1)
    a = lookup(textures, tex_index, b, uv6)
    return {"negative tap": neg.mean(), "past the edge, repeat": past[REPEAT].mean(),
            "past the edge, clamp": past[CLAMP].mean(), "past the edge, black": past[BLACK].mean(),
            "a <= 0": (a <= 0).mean(), "0 < a < 1": ((a > 0) & (a < 1)).mean(), "a >= 1": (a >= 1).mean()}


# ---- the per-ray oracle -------------------------------------------------------------------------------------------------
def triangle_uvs(prims, uvs):
    """the three (u, v) pairs of every primitive [n, 6]: the mesh's, or the reference's default corners"""
    if uvs is None:
        return np.tile(DEFAULT_UV, (len(prims), 1))
    return np.asarray(uvs, F)[prims["v"][:, :3]].reshape(len(prims), 6)


def per_ray_alpha(prims, verts, uvs, textures, rays, chunk=512):
    """a[i][j]: alpha of textured triangle j (position in `prims`) for ray i where the ray's line meets it (any value
    elsewhere: 0), float32 [n_rays, n_textured]; and the positions of the textured triangles"""
    verts = np.asarray(verts, F)
    tex = np.nonzero(is_textured(prims["kind"]))[0]
    a = np.zeros((len(rays), len(tex)), F)
    if not len(tex):
        return a, tex
    p9 = verts[prims["v"][tex][:, :3]].reshape(len(tex), 9)
    uv6 = triangle_uvs(prims[tex], uvs)
    ti = prims["v"][tex][:, 3]
    for lo in range(0, len(rays), chunk):
        r = rays[lo:lo + chunk]
        n = len(r)
        rec = np.zeros((n, len(tex), 16), F)
        rec[:, :, 0:3] = r["o"][:, None, :]
        rec[:, :, 3:6] = r["d"][:, None, :]
        rec[:, :, 6] = np.inf  # barycentrics do not depend on tMax
        rec[:, :, 7:16] = p9[None]
        hit, out = ob.leaf_batch("tri", rec.reshape(-1, 16))
        h = np.nonzero(hit)[0]
        if not len(h):
            continue
        jj = h % len(tex)
        irec = np.zeros((len(h), 45), F)  # oracle/ref_interaction.cpp's record: p9, b, wo, ..., time, flags, uv6 at 20
        irec[:, 0:9] = p9[jj]
        irec[:, 9:12] = out[h, 0:3]
        irec[:, 12:15] = (0, 0, 1)
        irec[:, 19] = 1  # the mesh has (u, v): the default corners are passed explicitly
        irec[:, 20:26] = uv6[jj]
        uv_hit = ob.triangle_interaction_batch(irec)[:, 6:8]
        alpha = np.zeros(len(h), F)
        for k, t in enumerate(textures):
            m = ti[jj] == k
            if m.any():
                alpha[m] = lookup_uv(t, uv_hit[m, 0], uv_hit[m, 1])
        a.reshape(-1)[lo * len(tex) + h] = alpha
    return a, tex


def constant_prims(prims, tex, alpha_row):
    """prims with the textured kinds rewritten to the constant-alpha ones (16 .. 19 -> 4 .. 7), v[3] = bits(alpha)"""
    out = prims.copy()
    out["kind"][tex] -= 12
    out["v"][tex, 3] = np.asarray(alpha_row, F).view(np.int32)
    return out


class PerRayOracle:
    """closest / any hit of a scene with textured triangles: the C oracle on each ray alone.  ordered_prims in the
    tree's leaf order; normals for the smooth kinds."""

    def __init__(self, nodes, ordered_prims, verts, uvs, textures, rays, normals=None):
        self.nodes, self.prims, self.verts, self.rays = nodes, np.ascontiguousarray(ordered_prims), verts, rays
        self.normals = normals
        self.alpha, self.tex = per_ray_alpha(self.prims, verts, uvs, textures, rays)

    def _each(self, fn):
        work = self.prims.copy()
        work["kind"][self.tex] -= 12
        try:
            ob.set_vertex_normals(self.normals)
            for i in range(len(self.rays)):
                work["v"][self.tex, 3] = self.alpha[i].view(np.int32)
                fn(i, work)
        finally:
            ob.set_vertex_normals(None)

    def closest(self):
        hits = np.zeros(len(self.rays), HIT_DTYPE)

        def one(i, prims):
            hits[i] = ob.closest(self.nodes, prims, self.verts, self.rays[i:i + 1])[0]
        self._each(one)
        return hits

    def any_hit(self):
        n = len(self.rays)
        occ, vis, tst = np.zeros(n, np.uint8), np.zeros(n, np.int32), np.zeros(n, np.int32)

        def one(i, prims):
            o, v, t = ob.any_hit(self.nodes, prims, self.verts, self.rays[i:i + 1])
            occ[i], vis[i], tst[i] = o[0], v[0], t[0]
        self._each(one)
        return occ, vis, tst


def scene_textures(seed=0):
    """three textures of different shape, wrap and mapping for the parity scenes: alphas spread over [0, 1.2] so that the
    test rejects, accepts after hashing and accepts outright"""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
    return [AlphaTexture((rng.random((5, 3)) * 1.2).astype(F), wrap="repeat", su=3.7, sv=-2.0, du=0.25, dv=-0.6),
            AlphaTexture((((xx // 2 + yy // 2) % 2) * 0.75).astype(F), wrap="clamp", su=2.0, sv=2.0, du=-0.5, dv=-0.5),
            AlphaTexture(rng.random((7, 9)).astype(F), wrap="black", point_filter=True, su=1.3, sv=1.3, du=-0.1, dv=-0.2,
                         scale=1.5, invert=True)]
