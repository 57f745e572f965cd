#!/usr/bin/env python3
"""Developer tool: one line per kernel from the output of `make -C mpcholonavigation_amd/csrc resource-usage`.

    make -C mpcholonavigation_amd/csrc resource-usage 2> usage.txt
    tools/resource_usage_table.py usage.txt [NAME-PART]      (e.g. smpc_pass_lane)

The remarks of -Rpass-analysis=kernel-resource-usage carry source line numbers, so two builds do not
diff; these lines (demangled name, registers, scratch, LDS, occupancy, spill counts) do."""
import re
import subprocess
import sys

FIELDS = (("VGPRs", "VGPRs"), ("AGPRs", "AGPRs"), ("SGPRs", "TotalSGPRs"), ("ScratchSize", "ScratchSize [bytes/lane]"),
          ("LDS", "LDS Size [bytes/block]"), ("Occupancy", "Occupancy [waves/SIMD]"), ("VGPR spills", "VGPRs Spill"),
          ("SGPR spills", "SGPRs Spill"))


def main():
    part = sys.argv[2] if len(sys.argv) > 2 else ""
    rows, cur = {}, None
    for line in open(sys.argv[1]):
        m = re.search(r"remark:\s+(.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        text = m.group(1)
        if text.startswith("Function Name:"):
            cur = text.split(": ", 1)[1]
            rows[cur] = {}
        elif cur and ":" in text:
            k, v = text.split(":", 1)
            rows[cur][k.strip()] = v.strip()
    names = list(rows)
    plain = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.splitlines()
    for mangled, name in zip(names, plain):
        name = name.split("(")[0].replace("void ", "")
        if part in name:
            print(name + ": " + ", ".join(f"{label} {rows[mangled].get(key)}" for label, key in FIELDS))


if __name__ == "__main__":
    main()
