"""smpc_group_stats (include/smpc.h, ABI 3) without a GPU: the symbol is exported and bound, and a
NULL group is refused — nothing here creates a context."""
import ctypes as C

import pytest

from mpcholonavigation_amd import _abi as A


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge
    ge.build()
    from mpcholonavigation_amd.optimizer import load_library
    return load_library()


def test_the_symbol_is_exported_and_bound(lib):
    assert "smpc_group_stats" in A.PROTOTYPES
    f = lib.smpc_group_stats
    assert f.restype is C.c_int and len(f.argtypes) == 3
    assert A.SMPC_ABI_VERSION == 3 and lib.smpc_abi_version() == 3


def test_a_null_group_is_invalid(lib):
    launches, singles = C.c_uint64(7), C.c_uint64(9)
    assert lib.smpc_group_stats(None, C.byref(launches), C.byref(singles)) == A.SMPC_ERR_INVALID
    assert (launches.value, singles.value) == (7, 9)        # nothing written
    assert lib.smpc_group_stats(None, None, None) == A.SMPC_ERR_INVALID


def test_the_python_face_has_it():
    from mpcholonavigation_amd.optimizer import SmpcGroup
    assert callable(SmpcGroup.stats)
