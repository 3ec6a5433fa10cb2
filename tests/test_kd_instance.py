"""Which kd_trace_kernel instance a call on a kd-tree scene runs (nn_bvh_amd/csrc/kd_instance.h), pinned without a GPU.

tests/golden/kd_instance_choice.txt holds the decision of the dispatch the pickers replaced (scene_instance,
kd_scene_reads_soa, kd_scene_fits32 and the inline choices of kd_launch_batches and launch_walk at the commit its first
line names, recorded by a host-only copy of them) for the whole cross product of its inputs: the eight scene traits times
the ten calls.  tests/cpp/kd_instance_check.cpp prints the same table from the three pickers, and then the library's
instance list, which kd_trace.hip compiles its kernels from.  (The ORDER of that list is the order of the kernels in the
compiled file; tools/isa_diff.py compares that, this test does not.)"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "kd_instance_check.cpp")
FIXTURE = os.path.join(ROOT, "tests", "golden", "kd_instance_choice.txt")


def run_check(exe, flags):
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror"] + flags + [SRC, "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert not out.stderr, out.stderr[-2000:]
    return out.stdout.splitlines()


@pytest.fixture(scope="module")
def expected():
    return [ln for ln in open(FIXTURE).read().splitlines() if not ln.startswith("#")]


def test_choice_matches_the_recorded_dispatch(tmp_path, expected):
    lines = run_check(tmp_path / "kd_instance_check", [])
    choice = [ln for ln in lines if not ln.startswith("table ")]
    # single 0 / 1; batch x {all SOA} x {candidates}; walk x {kind 1, 2} x {mesh has patches}; each over 2^8 trait bits
    assert len(expected) == (2 + 2 * 2 + 2 * 2) * 256
    assert len(choice) == len(expected)
    for got, want in zip(choice, expected):
        assert got == want
    # the library's table: every instance the fixture names, and none it never names
    table = [ln[len("table "):] for ln in lines if ln.startswith("table ")]
    named = set()
    for ln in expected:
        (instance,) = [w for w in ln.split() if w.startswith("<") and w.endswith(">")]
        named.add(instance)
    assert len(table) == len(set(table)) == 42
    assert named - set(table) == set()
    assert set(table) - named == set()


def test_choice_under_asan_ubsan(tmp_path, expected):
    lines = run_check(tmp_path / "kd_instance_check_san",
                      ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert [ln for ln in lines if not ln.startswith("table ")] == expected
