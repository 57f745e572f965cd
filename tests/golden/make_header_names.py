#!/usr/bin/env python3
"""Generates tests/golden/reference_header_names.json: for each stand-in under
tests/nav2_stubs/nav2_sortham_controller/ that stands for one of the reference's own headers,
the identifiers that appear both in the stand-in and in the header it stands for.

The fixture is data only (names the stand-ins already spell, confirmed against the real
headers), so tests/test_plugin_syntax_cpu.py checks the stand-ins without the reference.
Regenerate with:  python tests/golden/make_header_names.py <reference include/nav2_sortham_controller>
"""
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
STUBS = os.path.join(os.path.dirname(HERE), "nav2_stubs", "nav2_sortham_controller")
OUT = os.path.join(HERE, "reference_header_names.json")
HEADERS = ["tools/parameters_handler.hpp", "critic_function.hpp", "critic_manager.hpp", "models/trajectories.hpp"]


def identifiers(text):
    """The identifiers of the code (comments and preprocessor lines dropped)."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^\s*#[^\n]*", " ", text, flags=re.M)
    return set(re.findall(r"\b[A-Za-z_]\w*\b", text))


def main(ref_inc):
    names = {}
    for rel in HEADERS:
        with open(os.path.join(ref_inc, rel)) as f:
            ref = identifiers(f.read())
        with open(os.path.join(STUBS, rel)) as f:
            mine = identifiers(f.read())
        names[rel] = sorted(ref & mine)
    with open(OUT, "w") as f:
        json.dump(names, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
