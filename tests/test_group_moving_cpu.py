"""Grouped moving obstacles, the parts that need no GPU: the two new entry points refuse a NULL
group, and the Python wrapper checks the shape of its arguments before it calls the library."""
import ctypes as C

import pytest

from mpcholonavigation_amd import _abi as A
from tests.harness import lib  # noqa: F401


def test_the_group_setter_refuses_a_null_group(lib):
    n_discs = (C.c_uint32 * 1)(0)
    assert lib.smpc_group_set_moving_obstacles(None, None, None, None, n_discs, None) == A.SMPC_ERR_INVALID
    assert lib.smpc_group_set_moving_obstacles(None, None, None, None, None, None) == A.SMPC_ERR_INVALID


def test_the_launch_counter_refuses_a_null_group(lib):
    a, b = C.c_uint64(7), C.c_uint64(7)
    assert lib.smpc_debug_group_moving_launches(None, C.byref(a), C.byref(b)) == A.SMPC_ERR_INVALID
    assert (a.value, b.value) == (7, 7)


def test_the_per_member_switch_refuses_a_null_group(lib):
    assert lib.smpc_debug_group_moving_per_member(None, 1) == A.SMPC_ERR_INVALID


class _NoLibrary:
    """Stands where the library would: any call through it fails the test."""

    def __getattr__(self, name):
        raise AssertionError(f"the wrapper called {name} before it checked its arguments")


def _group_of(n):
    from mpcholonavigation_amd.optimizer import SmpcGroup
    import types
    g = SmpcGroup.__new__(SmpcGroup)
    g.members = [types.SimpleNamespace(T=30, B=100) for _ in range(n)]
    g.lib = _NoLibrary()
    g.h = None     # (close() and __del__ then do nothing)
    return g


def test_the_wrapper_refuses_a_tables_list_of_the_wrong_length():
    g = _group_of(3)
    with pytest.raises(ValueError, match="one table"):
        g.set_moving_obstacles([None, None])
    with pytest.raises(ValueError, match="one table"):
        g.set_moving_obstacles([None] * 4)
    with pytest.raises(ValueError, match="one take"):
        g.set_moving_obstacles([None] * 3, take=[1, 0])
