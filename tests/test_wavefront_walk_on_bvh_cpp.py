"""A C++ caller of HipBVHAggregate::WalkShadowTr / WalkOneRandom (include/nnbvh_aggregate.hpp): compiles with a plain
host compiler (CPU check); on a GPU the walks equal IntersectShadowTrBounded / IntersectOneRandomBounded of the same
aggregate where they finish, and mark what they do not (gpu check)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "bvh_walk_check")
ROCM_LIB = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")


def _build(nnbvh_lib):
    src = os.path.join(ROOT, "tests", "cpp", "bvh_walk_check.cpp")
    libdir = os.path.join(ROOT, "nn_bvh_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    src, "-o", EXE, "-pthread", "-L", libdir, "-l:libnnbvh_hip.so", f"-Wl,-rpath,{libdir}",
                    "-L", ROCM_LIB, "-lamdhip64", f"-Wl,-rpath,{ROCM_LIB}"], check=True)


def test_bvh_walk_caller_compiles_with_host_compiler_only(nnbvh_lib):
    _build(nnbvh_lib)
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_bvh_walk_adapter_equals_the_bounded_calls(nnbvh_lib):
    _build(nnbvh_lib)
    out = subprocess.run([EXE], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "bvh walk ok" in out.stdout
