"""The fleet host (include/smpc_host.h sortham_fleet_*, include/smpc.h smpc_group_optimize_some)
without a GPU: the new symbols are declared and exported, null arguments are refused before anything
touches a device, and the ABI number of the ctypes mirror is the header's."""
import ctypes as C
import os
import re

import pytest

from mpcholonavigation_amd import _abi as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLEET = ["sortham_fleet_create", "sortham_fleet_destroy", "sortham_fleet_last_error", "sortham_fleet_eval_control",
         "sortham_fleet_stats", "sortham_fleet_run_rounds"]


def header(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


@pytest.fixture(scope="module")
def libs():
    import __graft_entry__ as ge
    ge.build()
    from mpcholonavigation_amd import host_optimizer
    from mpcholonavigation_amd.optimizer import load_library
    return load_library(), host_optimizer.load_fleet_library()


def test_the_new_symbols_are_declared_and_exported(libs):
    smpc, host = libs
    from mpcholonavigation_amd import host_optimizer
    assert re.search(r"\bint\s+smpc_group_optimize_some\s*\(", header("smpc.h"))
    assert "smpc_group_optimize_some" in A.PROTOTYPES
    f = smpc.smpc_group_optimize_some
    assert f.restype is C.c_int and len(f.argtypes) == 5
    h = header("smpc_host.h")
    assert sorted(host_optimizer.FLEET_PROTOTYPES) == sorted(FLEET)
    for name in FLEET:
        assert re.search(r"\b%s\s*\(" % name, h), name
        assert hasattr(host, name), name
    assert re.search(r"#define\s+SORTHAM_FLEET_NOT_TAKEN\s+1\b", h)
    assert host_optimizer.SORTHAM_FLEET_NOT_TAKEN == 1


def test_the_abi_number_is_the_headers(libs):
    smpc, _ = libs
    m = re.search(r"#define\s+SMPC_ABI_VERSION\s+(\d+)", header("smpc.h"))
    assert m and int(m.group(1)) == A.SMPC_ABI_VERSION == smpc.smpc_abi_version()


def test_create_refuses_null_arguments(libs):
    _, host = libs
    h = C.c_void_p(0x1234)
    assert host.sortham_fleet_create(None, 3, C.byref(h)) == A.SMPC_ERR_INVALID
    assert not h.value                       # (cleared: nothing was made)
    one = (C.c_void_p * 1)(None)
    assert host.sortham_fleet_create(one, 0, C.byref(h)) == A.SMPC_ERR_INVALID
    assert host.sortham_fleet_create(one, 1, None) == A.SMPC_ERR_INVALID
    assert host.sortham_fleet_create(one, 1, C.byref(h)) == A.SMPC_ERR_INVALID
    assert not h.value
    assert b"member 0 is null" in host.sortham_fleet_last_error(None)


def test_a_null_fleet_is_invalid(libs):
    _, host = libs
    ins = (A.SmpcTickIn * 1)()
    tw = (C.c_double * 3)()
    st = (C.c_int32 * 1)(77)
    assert host.sortham_fleet_eval_control(None, ins, None, tw, None, st) == A.SMPC_ERR_INVALID
    done = C.c_uint32(9)
    assert host.sortham_fleet_run_rounds(None, ins, None, 4, 0, tw, None, st, C.byref(done)) == A.SMPC_ERR_INVALID
    assert host.sortham_fleet_run_rounds(None, ins, None, 4, 1, tw, None, st, C.byref(done)) == A.SMPC_ERR_INVALID
    assert done.value == 0 and st[0] == 77
    assert host.sortham_fleet_stats(None, None, None, None) == A.SMPC_ERR_INVALID
    host.sortham_fleet_destroy(None)         # (a no-op, like free)


def test_a_null_group_is_invalid_for_the_subset_call(libs):
    smpc, _ = libs
    assert smpc.smpc_group_optimize_some(None, None, None, None, None) == A.SMPC_ERR_INVALID


def test_the_python_faces_have_it():
    import inspect
    from mpcholonavigation_amd.host_optimizer import FleetOptimizer
    from mpcholonavigation_amd.optimizer import SmpcGroup
    assert "take" in inspect.signature(SmpcGroup.optimize).parameters
    assert callable(FleetOptimizer.eval_control) and callable(FleetOptimizer.run_rounds)
