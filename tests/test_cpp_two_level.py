"""HipBVHAggregate::BuildTwoLevelOnDevice (include/nnbvh_aggregate.hpp): compiles with a plain host compiler (CPU
check); on a GPU its scene is the scene of host-built trees, array for array and hit for hit (gpu check)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "two_level_check")


def _build(nnbvh_lib):
    src = os.path.join(ROOT, "tests", "cpp", "two_level_check.cpp")
    libdir = os.path.join(ROOT, "nn_bvh_amd")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    src, "-o", EXE, "-pthread", "-L", libdir, "-l:libnnbvh_hip.so", f"-Wl,-rpath,{libdir}",
                    "-Wl,-rpath-link,/opt/rocm/lib"], check=True)


def test_two_level_adapter_compiles_with_host_compiler_only(nnbvh_lib):
    _build(nnbvh_lib)
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_two_level_adapter_scene_is_the_host_built_one(nnbvh_lib):
    _build(nnbvh_lib)
    out = subprocess.run([EXE], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "two-level adapter ok" in out.stdout
