"""Seeded record generators for the awkward-input families: values biased towards exact zeros, +-0, denormals
(1e-40), huge and tiny magnitudes, rays aimed at the primitive so that hits stay common.

cases_<mode>(seed, n) returns float32 records in the layout oracle/ref_leaf.cpp documents for <mode>.  The live
comparisons of the oracle with the compiled reference (tests/test_oracle_vs_reference_live.py,
tests/test_aux_oracle.py) and the comparison of the device arithmetic with the oracle (tests/test_device_math.py)
draw from the same families with seeds of their own.  `seed` may be a numpy Generator: the draws then continue its
stream (test_aux_oracle.py draws its four families from one stream).  TEST INFRASTRUCTURE ONLY."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import interaction_cases as ic  # noqa: E402


def specials(rng, shape):
    """float32 values biased towards the awkward: exact zeros, +-0, tiny, huge, equal pairs."""
    v = rng.normal(size=shape) * 10.0 ** rng.integers(-6, 6, size=shape)
    pick = rng.random(shape)
    v = np.where(pick < 0.05, 0.0, v)
    v = np.where((pick >= 0.05) & (pick < 0.07), -0.0, v)
    v = np.where((pick >= 0.07) & (pick < 0.09), np.round(v), v)
    v = np.where((pick >= 0.09) & (pick < 0.10), 1e-40, v)
    return v.astype(np.float32)


def cases_tri(seed, n):
    """o[3] d[3] tmax p0[3] p1[3] p2[3]"""
    rng = np.random.default_rng(seed)
    recs = specials(rng, (n, 16))
    # half of the cases: aim the ray at a point of the triangle so that hits are common
    p = recs[:, 7:].reshape(n, 3, 3).astype(np.float64)
    b = rng.dirichlet([1, 1, 1], n)
    b[: n // 8, 0] = 0  # on an edge
    b /= b.sum(1, keepdims=True)
    tgt = np.einsum("nk,nkc->nc", b, p)
    aim = rng.random(n) < 0.6
    recs[aim, 3:6] = (tgt[aim] - recs[aim, 0:3].astype(np.float64)).astype(np.float32)
    recs[:, 6] = np.where(rng.random(n) < 0.7, np.inf, np.abs(recs[:, 6]))
    return recs


def cases_blp(seed, n):
    """o[3] d[3] tmax p00[3] p10[3] p01[3] p11[3]"""
    rng = np.random.default_rng(seed)
    recs = specials(rng, (n, 19))
    p = recs[:, 7:].reshape(n, 4, 3).astype(np.float64)
    u, v = rng.random((n, 1)), rng.random((n, 1))
    tgt = (1 - u) * (1 - v) * p[:, 0] + u * (1 - v) * p[:, 1] + (1 - u) * v * p[:, 2] + u * v * p[:, 3]
    aim = rng.random(n) < 0.7
    recs[aim, 3:6] = (tgt[aim] - recs[aim, 0:3].astype(np.float64)).astype(np.float32)
    recs[:, 6] = np.where(rng.random(n) < 0.7, np.inf, np.abs(recs[:, 6]))
    return recs


def cases_slab(seed, n):
    """o[3] d[3] tmax pmin[3] pmax[3]"""
    rng = np.random.default_rng(seed)
    recs = specials(rng, (n, 13))
    lo = np.minimum(recs[:, 7:10], recs[:, 10:13])
    hi = np.maximum(recs[:, 7:10], recs[:, 10:13])
    recs[:, 7:10], recs[:, 10:13] = lo, hi
    inside = rng.random(n) < 0.3
    recs[inside, 0:3] = (lo[inside] + (hi[inside] - lo[inside]) * rng.random((inside.sum(), 3))).astype(np.float32)
    onface = rng.random(n) < 0.1   # origin exactly on a face: the 0 * inf = NaN cases when d is 0 there
    recs[onface, 0] = lo[onface, 0]
    recs[:, 6] = np.where(rng.random(n) < 0.6, np.inf, np.abs(recs[:, 6]))
    return recs


def random_affine(rng, n):
    """Rotation * non-uniform scale (some negative) + translation in float64; both the matrix
    and its float64 inverse are then rounded to float32, like a pbrt Transform's m / mInv pair."""
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w),
                  2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w),
                  2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], 1).reshape(n, 3, 3)
    S = 10.0 ** rng.uniform(-2, 2, size=(n, 3)) * rng.choice([-1, 1], size=(n, 3), p=[0.1, 0.9])
    kind = rng.integers(0, 5, n)
    R[kind == 0] = np.eye(3)            # pure scale + translate
    S[kind == 1] = 1.0                  # rigid
    M = np.zeros((n, 4, 4))
    M[:, :3, :3] = R * S[:, None, :]
    M[:, :3, 3] = rng.normal(size=(n, 3)) * 10.0 ** rng.uniform(-1, 3, size=(n, 1))
    M[kind == 2, :3, 3] = 0             # no translation
    M[:, 3, 3] = 1
    Mi = np.linalg.inv(M)
    return M.astype(np.float32), Mi.astype(np.float32)


def cases_xfray(seed, n):
    """o[3] d[3] tmax m[16] mInv[16] (row-major)"""
    rng = np.random.default_rng(seed)
    M, Mi = random_affine(rng, n)
    o = specials(rng, (n, 3))
    d = specials(rng, (n, 3))
    t = np.where(rng.random(n) < 0.5, np.inf, np.abs(specials(rng, n))).astype(np.float32)
    return np.concatenate([o, d, t[:, None], M.reshape(n, 16), Mi.reshape(n, 16)], 1)


def cases_hash(seed, n):
    """a[3] b[3]"""
    rng = np.random.default_rng(seed)
    return specials(rng, (n, 6))


def cases_offset(seed, n):
    """pi_lo[3] pi_hi[3] n[3] w[3]; records with a non-finite value are left out (at most n come back)"""
    rng = np.random.default_rng(seed)
    p = specials(rng, (n, 3))
    err = np.abs(specials(rng, (n, 3))) * np.float32(1e-6)
    nn = rng.normal(size=(n, 3)).astype(np.float32)
    nn[rng.random(n) < 0.1] = 0
    lo = (p - err).astype(np.float32)
    y = np.concatenate([lo, np.where(err == 0, lo, p + err), nn, specials(rng, (n, 3))], 1).astype(np.float32)
    return y[np.isfinite(y).all(1)]


def cases_wrs(seed, n):
    """p0[3] p1[3] nAdds"""
    rng = np.random.default_rng(seed)
    return np.concatenate([specials(rng, (n, 6)), rng.integers(0, 30, (n, 1))], 1).astype(np.float32)


def cases_slab2(seed, n):
    """o[3] d[3] tmax pmin[3] pmax[3]"""
    rng = np.random.default_rng(seed)
    b = np.sort(rng.uniform(-5, 5, (n, 2, 3)), axis=1).reshape(n, 6)
    o = rng.uniform(-8, 8, (n, 3))
    d = (b[:, :3] + rng.uniform(-2, 6, (n, 3)) - o)
    d[::7, 1] = 0
    return np.concatenate([o, d, np.where(rng.random(n) < 0.5, np.inf, rng.uniform(0, 4, n))[:, None], b], 1).astype(np.float32)


# ---- the same families with more denormals ---------------------------------------------------------------------------
# specials() makes 1 % of its values 1e-40: a family that keeps 6 or 7 of them per record holds a denormal in 6 - 7 %
# of its records, cases_offset in 3 % (its points are moved by their error bounds) and cases_slab2, uniform in a box,
# in none.  The comparison of the device with the oracle wants at least 10 % everywhere, so it draws these families
# through with_denormals: further operands of about 15 % of the records become denormals of either sign, from the
# smallest to the largest.  The live comparisons with the compiled reference on the seeds of old keep the plain
# generators (byte-identical inputs); tests/test_device_math.py holds the oracle to the reference on these too.
DENORMALS = np.array([1e-40, -1e-40, 1.4e-45, -1.4e-45, 1.1e-38, -1.1e-38], np.float32)


def with_denormals(recs, columns, seed, share=0.15):
    """a copy of recs in which one or two of `columns` of about `share` of the records hold a denormal"""
    rng = np.random.default_rng(seed)
    x = np.array(recs, np.float32)
    rows = np.nonzero(rng.random(len(x)) < share)[0]
    for _ in range(2):
        x[rows, rng.choice(columns, len(rows))] = rng.choice(DENORMALS, len(rows))
        rows = rows[rng.random(len(rows)) < 0.5]
    return x


def cases_xfray_denormal(seed, n):
    """cases_xfray with denormals among o, d, tmax and rows 0..2 of mInv (what ApplyInverse reads)"""
    return with_denormals(cases_xfray(seed, n), np.r_[0:7, 23:35], [seed, 1])


def cases_hash_denormal(seed, n):
    return with_denormals(cases_hash(seed, n), np.r_[0:6], [seed, 1])


def cases_wrs_denormal(seed, n):
    return with_denormals(cases_wrs(seed, n), np.r_[0:6], [seed, 1])


def cases_offset_denormal(seed, n):
    """cases_offset with denormals among the interval's ends, n and w; the ends stay ordered"""
    x = with_denormals(cases_offset(seed, n), np.r_[0:12], [seed, 1])
    lo, hi = np.minimum(x[:, 0:3], x[:, 3:6]), np.maximum(x[:, 0:3], x[:, 3:6])
    x[:, 0:3], x[:, 3:6] = lo, hi
    return x


def cases_slab2_denormal(seed, n):
    """cases_slab2 with denormals among o, d, tmax and the box's corners; pmin <= pmax stays"""
    x = with_denormals(cases_slab2(seed, n), np.r_[0:13], [seed, 1])
    lo, hi = np.minimum(x[:, 7:10], x[:, 10:13]), np.maximum(x[:, 7:10], x[:, 10:13])
    x[:, 7:10], x[:, 10:13] = lo, hi
    x[:, 6] = np.abs(x[:, 6])
    return x


# ---- the interaction families ----------------------------------------------------------------------------------------
# Inputs of Triangle:: / BilinearPatch::InteractionFromIntersection and of Transform::operator()(SurfaceInteraction) in
# the record layouts of tests/golden/interaction_cases.py.  They start from that file's generators, so every flag mix
# and every rare-branch kind stays, and then become awkward: in about half of the records some of the positions, wo,
# uv, normals and tangents are specials() (exact zeros, -0, 1e-40, whole numbers, 1e-6 .. 1e6 magnitudes next to each
# other, normals that are not unit vectors), about 20 % of the records get one or two denormals of either sign, and two
# extreme kinds scale the geometry or wo by 1e-24 .. 1e-17 or 1e15 .. 1.5e19: LengthSquared then underflows to a
# denormal or to zero, or overflows to infinity, and Normalize divides by it.  The inputs themselves stay finite.
# tests/test_interaction_awkward.py holds the oracle to the compiled reference on them and the device to the oracle.
TRI_GROUPS = (np.r_[0:9], np.r_[12:15], np.r_[20:26], np.r_[26:35], np.r_[36:45])  # p, wo, uv, n, s
BLP_GROUPS = (np.r_[0:12], np.r_[14:17], np.r_[19:27], np.r_[27:39])               # p, wo, uv, n
XF_VECTORS = tuple(np.r_[38 + 3 * k:41 + 3 * k] for k in range(11))


def _specials_into(rng, rec, groups, share=0.5):
    """about `share` of the records: each group with probability 1/2, and of a chosen group each column with
    probability 1/2, becomes a draw of specials()"""
    n = len(rec)
    awkward = rng.random(n) < share
    for g in groups:
        take = (awkward & (rng.random(n) < 0.5))[:, None] & (rng.random((n, len(g))) < 0.5)
        rec[:, g] = np.where(take, specials(rng, (n, len(g))), rec[:, g])


def _extreme_scales(rng, n):
    """10 ** uniform over 1e-24 .. 1e-17 (one half) or 1e15 .. 1.5e19 (the other half), float32 [n, 1]"""
    small = rng.uniform(-24, -17, n)
    large = rng.uniform(15, np.log10(1.5e19), n)
    return (10.0 ** np.where(rng.random(n) < 0.5, small, large)).astype(np.float32)[:, None]


def _extremes(rng, rec, geometry, wo, share_geometry, share_wo):
    pick = rng.random(len(rec))
    for cols, rows in ((geometry, pick < share_geometry),
                       (wo, (pick >= share_geometry) & (pick < share_geometry + share_wo))):
        with np.errstate(over="ignore", under="ignore"):
            rec[:, cols] = np.where(rows[:, None], rec[:, cols] * _extreme_scales(rng, len(rec)), rec[:, cols])
    rec[~np.isfinite(rec)] = 0


def zero_area(rec):
    """The triangles the reference refuses (CHECK_NE(LengthSquared(ng), 0), shapes.h:916-919): the edges p2 - p0 and
    p1 - p0 in float32, their cross product in float64 rounded to float32, and the float32 LengthSquared of that is 0."""
    p = np.asarray(rec, np.float32)
    v, w = (p[:, 6:9] - p[:, 0:3]).astype(np.float64), (p[:, 3:6] - p[:, 0:3]).astype(np.float64)
    with np.errstate(over="ignore", under="ignore"):
        c = np.stack([v[:, 1] * w[:, 2] - v[:, 2] * w[:, 1], v[:, 2] * w[:, 0] - v[:, 0] * w[:, 2],
                      v[:, 0] * w[:, 1] - v[:, 1] * w[:, 0]], 1).astype(np.float32)
        return (c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2] == 0


def cases_tri_interaction(seed, n, share_geometry=0.1, share_wo=0.1):
    """45 columns, interaction_cases.cases' layout and kinds; specials among p, wo, uv, n and s; denormals among every
    float column but time and flags; 10 % of the records with p scaled by 1e-24 .. 1e-17 or 1e15 .. 1.5e19 and 10 % with
    wo scaled so.  Zero-area triangles are left out (at most n records come back): the rule is zero_area()'s, the
    reference's own test, applied to every record whether or not it would reach that test.  The bake flags such
    triangles degenerate and no hit on them is ever reported; the small half of the geometry extremes falls under it."""
    rng = np.random.default_rng([seed, 2])
    rec = ic.cases(n, seed)
    _specials_into(rng, rec, TRI_GROUPS)
    rec = with_denormals(rec, np.r_[0:15, 20:35, 36:45], [seed, 3], share=0.2)
    _extremes(rng, rec, np.r_[0:9], np.r_[12:15], share_geometry, share_wo)
    return rec[~zero_area(rec)]


def cases_blp_interaction(seed, n, share_geometry=0.04, share_wo=0.1):
    """40 columns, interaction_cases.patch_cases' layout and kinds; specials among p, wo, uv and n; denormals among
    every float column but time and flags; the two extreme kinds as in cases_tri_interaction, the geometry at 4 %: a patch
    whose dpdu x dpdv underflows or overflows has a NaN normal, and the comparisons want few NaN records."""
    rng = np.random.default_rng([seed, 2])
    rec = ic.patch_cases(n, seed)
    _specials_into(rng, rec, BLP_GROUPS)
    rec = with_denormals(rec, np.r_[0:17, 19:39], [seed, 3], share=0.2)
    _extremes(rng, rec, np.r_[0:12], np.r_[14:17], share_geometry, share_wo)
    return rec


def cases_xf_interaction(seed, n):
    """72 columns, interaction_cases.transform_cases' layout, kinds and (invertible) matrices; denormals among rows
    0..2 of m and mInv and among the vectors; specials among the eleven vectors; pi intervals that are exact, one ulp or
    a denormal wide, or specials at both ends, with lo <= hi restored."""
    rng = np.random.default_rng([seed, 2])
    rec = ic.transform_cases(n, seed)
    _specials_into(rng, rec, XF_VECTORS)
    kind = rng.integers(0, 8, n)
    p = np.where((kind == 0)[:, None], specials(rng, (n, 3)), rec[:, 32:35])
    k = kind <= 1                                       # exact points, awkward coordinates among them
    rec[k, 32:35] = rec[k, 35:38] = p[k]
    k = kind == 2                                       # one ulp wide
    rec[k, 35:38] = np.nextafter(rec[k, 32:35], np.float32(np.inf))
    k = kind == 3                                       # points at zero or a denormal, the interval a denormal wide
    rec[k, 32:35] = rng.choice(np.r_[DENORMALS, np.float32([0.0, -0.0])], (int(k.sum()), 3))
    rec[k, 35:38] = rec[k, 32:35] + np.float32(1e-40)
    k = kind == 4                                       # both ends awkward
    rec[k, 32:38] = specials(rng, (int(k.sum()), 6))
    rec = with_denormals(rec, np.r_[0:12, 16:28, 32:71], [seed, 3], share=0.2)
    lo, hi = np.minimum(rec[:, 32:35], rec[:, 35:38]), np.maximum(rec[:, 32:35], rec[:, 35:38])
    rec[:, 32:35], rec[:, 35:38] = lo, hi
    return rec


def _identity(rows, translation):
    """x' = m[i][0] * x + m[i][1] * y + m[i][2] * z (+ m[i][3]) with m the identity, summed left to right in float32"""
    one, zero = np.float32(1), np.float32(0)
    x, y, z = rows[:, 0], rows[:, 1], rows[:, 2]
    out = [(one * x + zero * y) + zero * z, (zero * x + one * y) + zero * z, (zero * x + zero * y) + one * z]
    return np.stack([c + zero for c in out] if translation else out, 1).astype(np.float32)


def as_the_reference_mesh_stores(rec, kind):
    """Triangle (kind 0) or patch (kind 1) records as oracle/ref_interaction.cpp's mesh holds them.  That harness builds
    its mesh with Transform(), and the reference's mesh constructors send every position (util/mesh.cpp:37-38, 207-208),
    normal (:51-52, :218-219) and tangent (:60-61) through that identity transform: Transform::operator()(Point3)
    (util/transform.h:310-319: three products and the translation, summed left to right; w is 1, so no division),
    (Vector3) (:322-326) and (Normal3) (:329-334, the columns of mInv).  Multiplying by 0 and 1 is exact, so only signs
    of zeros move: (0 * x + 1 * y) + 0 * z + 0 makes a -0 coordinate +0, and a -0 component of a normal or tangent
    survives only next to two negative ones.  The product never does this: it takes the caller's arrays as they are."""
    out = np.array(rec, np.float32)
    n_vert, c_n = (3, 26) if kind == 0 else (4, 27)
    groups = [(0, True), (c_n, False)] + ([(36, False)] if kind == 0 else [])
    for at, translation in groups:
        cols = slice(at, at + 3 * n_vert)
        out[:, cols] = _identity(out[:, cols].reshape(-1, 3), translation).reshape(len(out), -1)
    return out
