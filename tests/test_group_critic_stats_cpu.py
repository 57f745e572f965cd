"""No-GPU checks of smpc_group_critic_breakdown and smpc_group_breakdown_counts (include/smpc.h) and of
the fleet's host face (include/smpc_host.h): declared, exported, bound with the header's signature,
and null arguments refused before anything is touched."""
import ctypes as C
import os
import re


from mpcholonavigation_amd import _abi as A
from tests.harness import lib  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("smpc_group_critic_breakdown", "smpc_group_breakdown_counts")


def header(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def declared(src, fn):
    """(return type, [parameter types]) of the prototype of `fn`, spaces and names stripped."""
    m = re.search(r"(\w[\w\s\*]*?)\b%s\s*\(([^)]*)\)\s*;" % fn, src)
    assert m, f"{fn} is not declared"
    params = []
    for p in m.group(2).split(","):
        p = re.sub(r"\b[a-z_0-9]+\s*$", "", p.strip())     # the parameter's name
        params.append(re.sub(r"\s+", "", p))
    return m.group(1).strip(), params


# what a parameter type of the header is bound as
CTYPE = {
    "smpc_group*": A._ctx, "constsmpc_group*": A._ctx,
    "constsmpc_tick_in*": C.POINTER(A.SmpcTickIn),
    "constfloat*const*": C.POINTER(C.c_void_p), "float*const*": C.POINTER(C.c_void_p),
    "constuint8_t*": C.c_void_p,
    "smpc_critic_stats*": C.POINTER(A.SmpcCriticStats),
    "int32_t*": C.POINTER(C.c_int32), "uint64_t*": C.POINTER(C.c_uint64),
}


def test_the_new_symbols_are_declared_exported_and_bound(lib):
    src = header("smpc.h")
    for fn in NEW:
        ret, params = declared(src, fn)
        assert ret == "int"
        assert hasattr(lib, fn), f"{fn} declared in smpc.h but not exported"
        restype, argtypes = A.PROTOTYPES[fn]
        assert restype is C.c_int
        assert [CTYPE[p] for p in params] == list(argtypes), (fn, params, argtypes)
        assert getattr(lib, fn).argtypes == list(argtypes) or tuple(getattr(lib, fn).argtypes) == tuple(argtypes)
    assert declared(src, NEW[0])[1] == ["smpc_group*", "constsmpc_tick_in*", "constfloat*const*", "constuint8_t*",
                                        "smpc_critic_stats*", "float*const*", "int32_t*"]
    assert declared(src, NEW[1])[1] == ["constsmpc_group*", "uint64_t*", "uint64_t*"]
    # an addition under the current ABI version
    assert A.SMPC_ABI_VERSION == 3 and lib.smpc_abi_version() == 3


def test_null_arguments_are_refused_before_anything_is_touched(lib):
    n = 2
    ins = (A.SmpcTickIn * n)()
    us = (C.c_void_p * n)()
    st = (A.SmpcCriticStats * n)()
    C.memset(st, 0xAB, C.sizeof(st))
    status = (C.c_int32 * n)(-77, -77)
    f = lib.smpc_group_critic_breakdown
    assert f(None, ins, us, None, st, None, status) == A.SMPC_ERR_INVALID
    assert lib.smpc_last_error(None) == b"null argument"
    # a group pointer that must never be followed: the null arrays are seen first
    never = C.create_string_buffer(4096)
    group = C.cast(never, C.c_void_p)
    for args in ((group, None, us, None, st, None, status), (group, ins, None, None, st, None, status),
                 (group, ins, us, None, None, None, status), (group, ins, us, None, st, None, None)):
        assert f(*args) == A.SMPC_ERR_INVALID
        assert lib.smpc_last_error(None) == b"null argument"
    assert bytes(st) == b"\xab" * C.sizeof(st) and list(status) == [-77, -77]
    b, s = C.c_uint64(5), C.c_uint64(6)
    assert lib.smpc_group_breakdown_counts(None, C.byref(b), C.byref(s)) == A.SMPC_ERR_INVALID
    assert (b.value, s.value) == (5, 6)


def test_the_fleets_host_face_is_declared_exported_and_bound(lib):
    from mpcholonavigation_amd import host_optimizer
    src = header("smpc_host.h")
    assert re.search(r"\bsortham_fleet_critic_stats\s*\(", src)
    host = host_optimizer.load_fleet_library()
    assert hasattr(host, "sortham_fleet_critic_stats")
    assert list(host.sortham_fleet_critic_stats.argtypes) == host_optimizer.FLEET_STATS_PROTOTYPES["sortham_fleet_critic_stats"][1]
    assert "sortham_fleet_critic_stats" in host_optimizer.FLEET_STATS_PROTOTYPES
    ret, params = declared(src, "sortham_fleet_critic_stats")
    assert ret == "int" and len(params) == len(host_optimizer.FLEET_STATS_PROTOTYPES["sortham_fleet_critic_stats"][1])
    assert host.sortham_fleet_critic_stats(None, None, None, None, None, None) == A.SMPC_ERR_INVALID
