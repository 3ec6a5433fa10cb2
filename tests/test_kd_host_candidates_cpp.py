"""tests/cpp/kd_candidates_check.cpp: HipKdTreeAggregate's host-candidate overloads as an embedder calls them,
resolved with the oracle's triangle test and held to the all-triangle kd scene."""
import os
import subprocess

import pytest

import oracle_binding as ob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "kd_candidates_check")


def _build(nnbvh_lib):
    src = os.path.join(ROOT, "tests", "cpp", "kd_candidates_check.cpp")
    libdir, oracle_dir = os.path.join(ROOT, "nn_bvh_amd"), os.path.join(ROOT, "oracle")
    ob.lib()  # builds oracle/libnnbvh_oracle.so where it is missing
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    src, "-o", EXE, "-pthread", "-L", libdir, "-l:libnnbvh_hip.so", f"-Wl,-rpath,{libdir}",
                    "-L", oracle_dir, "-l:libnnbvh_oracle.so", f"-Wl,-rpath,{oracle_dir}",
                    "-Wl,-rpath-link,/opt/rocm/lib"], check=True)


def test_kd_candidate_caller_compiles_with_host_compiler_only(nnbvh_lib):
    _build(nnbvh_lib)
    assert os.path.exists(EXE)


@pytest.mark.gpu
def test_gpu_cpp_kd_candidate_overloads_resolve_to_the_all_triangle_scene(nnbvh_lib):
    _build(nnbvh_lib)
    out = subprocess.run([EXE], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "kd host candidates ok" in out.stdout
