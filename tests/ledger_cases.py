"""One way to state and assert "this case runs these kernel instances" (the launch ledger).

A test module that asserts with the ledger holds a module-level dict

    LEDGER = {pytest id of the GPU case: (kernel family, set of instances)}

BVH instances are (mode, window, inst, patch, alpha, soa, hostc) of trace_kernel, kd instances (mode, patch, o32, attr,
hostc) of kd_trace_kernel.  Where a case states the sets of its parts separately (one per option value, say), a key
is the pytest id followed by the part's name.  The GPU test wraps ALL device calls of the case in `with reaches(LEDGER, case):`; the block
asserts that the calls launched exactly the instances listed, each at least once, and no other instance of the family.
The census (tests/test_wide_offsets.py) takes the union over the modules named in MODULES."""
import contextlib

from nn_bvh_amd import _lib

BVH, KD = _lib.FAMILY_BVH, _lib.FAMILY_KD

# every test module with a LEDGER table; the census and the key check import them by name
MODULES = ("test_stack_limits", "test_alpha", "test_alpha_texture", "test_two_level_alpha_texture",
           "test_host_candidates", "test_wavefront_candidates", "test_wavefront_walk_on_bvh", "test_alpha_candidates")


def bvh(modes, window=8, inst=0, patch=1, alpha=0, soa=0, hostc=0):
    """{<m, window, inst, patch, alpha, soa, hostc> for m in modes}"""
    return {(m, window, inst, patch, alpha, soa, hostc) for m in modes}


def ledger_start(table, case):
    return _lib.instance_launches(table[case][0])


def assert_reached(table, case, start):
    """the device calls since ledger_start(table, case) launched exactly the instances the table lists for `case`"""
    family, want = table[case]
    launched = {k: v - start[k] for k, v in _lib.instance_launches(family).items() if v != start[k]}
    assert set(launched) == set(want), f"{case}: launched {sorted(launched.items())}, LEDGER says {sorted(want)}"


@contextlib.contextmanager
def reaches(table, case):
    start = ledger_start(table, case)
    yield
    assert_reached(table, case, start)
