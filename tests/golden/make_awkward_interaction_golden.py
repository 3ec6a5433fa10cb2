#!/usr/bin/env python3
"""Generate tests/golden/awkward_{tri,blp,xf}_interaction.npz: the awkward-input families of tests/awkward_cases.py
(cases_tri_ / cases_blp_ / cases_xf_interaction) and what the REFERENCE's own functions make of them
(oracle/_ref/ref_interaction, built by oracle/Makefile).  Build-container only; the .npz files hold data only: seeded
inputs, RAW (signed zeros as drawn), and the reference's outputs as float32 bit patterns.  The record counts keep each
file below 1 MiB."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import awkward_cases as ac  # noqa: E402
from make_interaction_golden import run_ref  # noqa: E402

FIXTURES = (("tri", ac.cases_tri_interaction, 20241001, 3000),
            ("blp", ac.cases_blp_interaction, 20241002, 3000),
            ("xf", ac.cases_xf_interaction, 20241003, 2400))

if __name__ == "__main__":
    for mode, family, seed, n in FIXTURES:
        rec = family(seed, n)
        out = run_ref(rec, mode)
        path = os.path.join(HERE, f"awkward_{mode}_interaction.npz")
        np.savez_compressed(path, inputs=rec, outputs=out)
        print(os.path.basename(path), rec.shape, out.shape, os.path.getsize(path), "bytes")
