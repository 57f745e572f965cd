"""No-GPU checks of the critic statistics' ABI (include/smpc.h: smpc_critic_name,
smpc_critic_stats, smpc_critic_breakdown; include/smpc_host.h: sortham_optimizer_critic_stats)."""
import ctypes as C
import os
import re
import subprocess
import tempfile


from mpcholonavigation_amd import _abi as A
from tests.harness import lib  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = ("sum", "min", "max", "weighted", "at_best")


def header(name="smpc.h"):
    return open(os.path.join(ROOT, "include", name)).read()


def test_symbols_exist_and_are_bound(lib):
    from mpcholonavigation_amd import host_optimizer
    for name in ("smpc_critic_name", "smpc_critic_breakdown"):
        assert hasattr(lib, name), name
        assert name in A.PROTOTYPES, name
    assert hasattr(host_optimizer.load_library(), "sortham_optimizer_critic_stats")
    assert "sortham_optimizer_critic_stats" in host_optimizer.PROTOTYPES
    assert "sortham_optimizer_critic_stats" in header("smpc_host.h")
    from mpcholonavigation_amd.optimizer import Smpc
    assert callable(Smpc.critic_stats) and callable(host_optimizer.Optimizer.critic_stats)


def test_constants_match_the_header():
    h = header()
    defs = dict(re.findall(r"#define\s+(SMPC_(?:N_CRITICS|CRITIC_[A-Z_]+|STATS_[A-Z]+))\s+(\d+)", h))
    assert len(defs) == 15
    for name, value in defs.items():
        assert getattr(A, name) == int(value), name
    assert A.SMPC_N_CRITICS == 12 and A.SMPC_STATS_CONTROL == 12 and A.SMPC_STATS_ROWS == 13


def test_struct_layout_matches_header():
    """sizeof/offsetof of the ctypes mirror against a tiny C program compiled from smpc.h."""
    fields = [n for n, _ in A.SmpcCriticStats._fields_]
    offs = ", ".join(f"offsetof(smpc_critic_stats, {n})" for n in fields)
    prog = ('#include <stdio.h>\n#include <stddef.h>\n#include "smpc.h"\nint main(void) {\n'
            '  size_t v[] = {sizeof(smpc_critic_stats), sizeof(((smpc_critic_stats*)0)->sum), %s};\n'
            '  for (unsigned i = 0; i < sizeof(v) / sizeof(v[0]); ++i) printf("%%zu ", v[i]);\n  return 0;\n}\n' % offs)
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write(prog)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", exe, src], check=True)
        out = [int(x) for x in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert out[0] == C.sizeof(A.SmpcCriticStats)
    assert out[1] == 13 * 4 == A.SmpcCriticStats.sum.size
    assert out[2:] == [getattr(A.SmpcCriticStats, n).offset for n in fields]
    assert fields == ["scored_mask", "fail_flag", "batch", "best_rollout", "best_cost", "effective_samples", *ROWS]


def scoring_order():
    """The critics in the fixed scoring order, from the comment in smpc.h above smpc_critic_params."""
    m = re.search(r"/\* Scoring order.*?\):\s*(.*?)\.\s+A[\s*]+different YAML order", header(), flags=re.S)
    assert m, "smpc.h no longer states the scoring order"
    names = [n.strip() for n in re.sub(r"[\s*]+", " ", m.group(1)).split(",")]
    assert len(names) == 12
    return names


def test_critic_names(lib):
    names = [lib.smpc_critic_name(k) for k in range(A.SMPC_N_CRITICS)]
    assert all(n is not None for n in names)
    names = [n.decode() for n in names]
    # the scoring order of smpc.h, which names the critics without the "Critic" suffix
    assert [n[:-len("Critic")] for n in names] == scoring_order()
    assert all(n.endswith("Critic") for n in names)
    # the ids follow it
    ids = ["CONSTRAINT", "COST", "OBSTACLES", "PATH_ALIGN", "PATH_ALIGN_LEGACY", "PATH_FOLLOW", "GOAL_ANGLE",
           "PREFER_FORWARD", "GOAL", "PATH_ANGLE", "TWIRLING", "VELOCITY_DEADBAND"]
    for k, (i, n) in enumerate(zip(ids, names)):
        assert getattr(A, "SMPC_CRITIC_" + i) == k
        assert n == "".join(w.capitalize() for w in i.split("_")) + "Critic"
    # the class names nav2_plugin/critics.xml registers
    xml = open(os.path.join(ROOT, "nav2_plugin", "critics.xml")).read()
    registered = re.findall(r'<class type="sortham::critics::(\w+)"', xml)
    assert len(registered) == 12 and sorted(registered) == sorted(names)


def test_control_row_and_out_of_range(lib):
    assert lib.smpc_critic_name(A.SMPC_STATS_CONTROL) == b"ControlCost"
    assert lib.smpc_critic_name(13) is None
    assert lib.smpc_critic_name(0xFFFFFFFF) is None


def test_null_arguments_without_a_device(lib):
    """SMPC_ERR_INVALID before anything touches a device: no context is needed to find out."""
    st = A.SmpcCriticStats()
    tick = A.SmpcTickIn()
    u = (C.c_float * 3)()
    f = lib.smpc_critic_breakdown
    assert f(None, C.byref(tick), u, C.byref(st), None) == A.SMPC_ERR_INVALID
    assert f(None, None, None, None, None) == A.SMPC_ERR_INVALID
    from mpcholonavigation_amd import host_optimizer
    host = host_optimizer.load_library()
    assert host.sortham_optimizer_critic_stats(None, C.byref(tick), C.byref(st), None) == A.SMPC_ERR_INVALID
