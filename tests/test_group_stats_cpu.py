"""smpc_group_stats (include/smpc.h, ABI 3) without a GPU: the symbol is exported and bound, and a
NULL group is refused — nothing here creates a context."""
import ctypes as C


from mpcholonavigation_amd import _abi as A
from tests.harness import lib  # noqa: F401


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
