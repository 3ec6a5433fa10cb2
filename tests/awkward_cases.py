"""Seeded record generators for the awkward-input families: values biased towards exact zeros, +-0, denormals
(1e-40), huge and tiny magnitudes, rays aimed at the primitive so that hits stay common.

cases_<mode>(seed, n) returns float32 records in the layout oracle/ref_leaf.cpp documents for <mode>.  The live
comparisons of the oracle with the compiled reference (tests/test_oracle_vs_reference_live.py,
tests/test_aux_oracle.py) and the comparison of the device arithmetic with the oracle (tests/test_device_math.py)
draw from the same families with seeds of their own.  `seed` may be a numpy Generator: the draws then continue its
stream (test_aux_oracle.py draws its four families from one stream).  TEST INFRASTRUCTURE ONLY."""
import numpy as np


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
