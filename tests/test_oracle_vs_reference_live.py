"""Live cross-check of the oracle's leaf functions against the REFERENCE's own compiled code
(oracle/_ref/ref_leaf, built by oracle/Makefile from /root/reference sources) on fresh random
inputs every run-seed — beyond the fixed golden vectors.  Skipped where the binary is absent
(it is git-ignored; it exists in the build container and travels to the GPU box)."""
import os
import subprocess
import tempfile

import numpy as np
import pytest

import oracle_binding as ob
from awkward_cases import cases_blp, cases_slab, cases_tri, cases_xfray, random_affine, specials  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.path.join(ROOT, "oracle", "_ref", "ref_leaf")

pytestmark = pytest.mark.skipif(not os.path.exists(REF), reason="oracle/_ref/ref_leaf not built")


def run_ref(mode, recs, nout):
    recs = np.ascontiguousarray(recs, np.float32)
    with tempfile.TemporaryDirectory() as td:
        fi, fo = os.path.join(td, "i.bin"), os.path.join(td, "o.bin")
        with open(fi, "wb") as f:
            f.write(np.int32(len(recs)).tobytes())
            f.write(recs.tobytes())
        subprocess.run([REF, mode, fi, fo], check=True)
        raw = np.fromfile(fo, np.uint32).reshape(len(recs), 1 + nout)
    return raw[:, 0].astype(np.uint8), raw[:, 1:]


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_triangle_oracle_equals_reference_on_random_inputs(seed):
    recs = cases_tri(seed, 20000)
    eh, eb = run_ref("tri", recs, 4)
    gh, go = ob.leaf_batch("tri", recs)
    assert (gh == eh).all()
    m = eh.astype(bool)
    assert (go.view(np.uint32)[m] == eb[m]).all()
    assert m.sum() > 1000


@pytest.mark.parametrize("seed", [21, 22])
def test_patch_oracle_equals_reference_on_random_inputs(seed):
    recs = cases_blp(seed, 20000)
    eh, eb = run_ref("blp", recs, 3)
    gh, go = ob.leaf_batch("blp", recs)
    assert (gh == eh).all()
    m = eh.astype(bool)
    assert (go.view(np.uint32)[m] == eb[m]).all()
    assert m.sum() > 1000


@pytest.mark.parametrize("seed", [31, 32])
def test_slab_oracle_equals_reference_on_random_inputs(seed):
    recs = cases_slab(seed, 40000)
    eh, _ = run_ref("slab", recs, 0)
    gh, _ = ob.leaf_batch("slab", recs)
    assert (gh == eh).all()
    assert 0.05 < eh.mean() < 0.95


@pytest.mark.parametrize("seed", [41, 42])
def test_ray_inverse_transform_equals_reference(seed):
    """Transform::ApplyInverse(Ray, tMax) with its interval arithmetic (transform.h:416-429)."""
    recs = cases_xfray(seed, 20000)
    eh, eb = run_ref("xfray", recs, 7)
    got = ob.apply_inverse_ray(recs[:, 23:35], recs[:, 0:3], recs[:, 3:6], recs[:, 6])
    assert (got.view(np.uint32) == eb).all()
