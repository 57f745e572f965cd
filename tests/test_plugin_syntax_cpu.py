"""The Nav2 adaptor sources (nav2_plugin/src/*.cpp, nav2_plugin/include/) through a compiler.

There is no ROS 2 / Nav2 / xtensor / pluginlib in this image, so the adaptor cannot be built.
This is the next best thing: `g++ -std=c++17 -fsyntax-only` against the
declaration-only stand-ins under tests/nav2_stubs/ — the 503 lines are well-formed C++ and
type-check against the interfaces they name.  It proves nothing about Nav2's behaviour.  The
second test checks that the stand-ins of the reference's OWN headers declare only names those
headers really have, against the names recorded from them in tests/golden/reference_header_names.json
(tests/golden/make_header_names.py)."""
import json
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUBS = os.path.join(ROOT, "tests", "nav2_stubs")
SOURCES = ["nav2_plugin/src/optimizer.cpp", "nav2_plugin/src/fused_critics.cpp"]
REF_NAMES = os.path.join(ROOT, "tests", "golden", "reference_header_names.json")


@pytest.mark.parametrize("src", SOURCES)
def test_adaptor_source_is_well_formed(src):
    cmd = ["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror=return-type",
           "-I", STUBS, "-I", os.path.join(ROOT, "nav2_plugin", "include"), "-I", os.path.join(ROOT, "include"),
           "-I", os.path.join(ROOT, "mpcholonavigation_amd"), os.path.join(ROOT, src)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_stand_ins_of_the_reference_headers_declare_real_names():
    """Every identifier followed by '(' or ';' that a stand-in of a reference header declares
    inside a class body appears in the header it stands for (as recorded in the golden names)."""
    with open(REF_NAMES) as f:
        ref_names = json.load(f)
    pairs = {"tools/parameters_handler.hpp": ["ParameterType", "Dynamic", "Static", "ParametersHandler", "getParamGetter",
                                              "addPostCallback", "getLock", "getParam"],
             "critic_function.hpp": ["CriticFunction", "on_configure", "score", "initialize", "getName", "enabled_",
                                     "name_", "parent_name_", "parent_", "costmap_ros_", "costmap_",
                                     "parameters_handler_", "logger_"],
             "critic_manager.hpp": ["CriticManager", "on_configure", "evalTrajectoriesScores"],
             "models/trajectories.hpp": ["Trajectories", "reset", "yaws"]}
    for rel, names in pairs.items():
        ref = set(ref_names[rel])
        mine = open(os.path.join(STUBS, "nav2_sortham_controller", rel)).read()
        for n in names:
            assert re.search(r"\b" + re.escape(n) + r"\b", mine), (rel, n, "not in the stand-in")
            assert n in ref, (rel, n, "not in the reference header")
