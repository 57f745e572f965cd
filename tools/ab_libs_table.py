#!/usr/bin/env python3
"""Developer tool: the table of tools/ab_libs.sh.   tools/ab_libs_table.py OUTDIR

Per round the scoring pass's average duration under the kernel trace (a), the smpc_reduce_partials
average, and the plain bench line's ms_per_step (b), for parent / new / parent again; then the means, the
gain, and the call's own noise s = max - min over ALL parent runs (c), for (a) and for (b)."""
import csv, glob, json, os, re, sys

out = sys.argv[1]


def stats(path):
    p = r = None
    for row in csv.DictReader(open(path)):
        n, avg = row["Name"], float(row["AverageNs"]) / 1e3
        if n.startswith("smpc_pass_lane") or n.startswith("void smpc_pass_lane"):
            p = avg if p is None else max(p, avg)
        if "smpc_reduce_partials" in n:
            r = avg
    return p, r


def line(path):
    return 1e3 * json.loads(open(path).read().strip().splitlines()[-1])["ms_per_step"]


rounds = sorted({int(re.search(r"kernel_stats_(\d+)_", f).group(1)) for f in glob.glob(os.path.join(out, "kernel_stats_*_*.csv"))})
acc = {k: {"pass": [], "reduce": [], "tick": []} for k in ("parent", "new", "parent2")}
print("round  who      pass us (a)  reduce us  tick us (b)")
for r in rounds:
    for who in ("parent", "new", "parent2"):
        p, red = stats(os.path.join(out, f"kernel_stats_{r}_{who}.csv"))
        t = line(os.path.join(out, f"bench_{r}_{who}.json"))
        acc[who]["pass"].append(p); acc[who]["reduce"].append(red); acc[who]["tick"].append(t)
        print(f"{r:5d}  {who:8s} {p:11.2f} {red:10.2f} {t:12.2f}")
for key, label in (("pass", "(a) pass average under the kernel trace"), ("tick", "(b) bench line ms_per_step")):
    par = acc["parent"][key] + acc["parent2"][key]
    new = acc["new"][key]
    mp, mn = sum(par) / len(par), sum(new) / len(new)
    s = max(par) - min(par)
    print(f"{label}: parent {mp:.2f} us (n={len(par)}, min {min(par):.2f}, max {max(par):.2f}), new {mn:.2f} us "
          f"(n={len(new)}, min {min(new):.2f}, max {max(new):.2f}); gain {mp - mn:.2f} us = {100 * (mp - mn) / mp:.2f} %; "
          f"noise s = {s:.2f} us; gain / s = {(mp - mn) / s if s else float('inf'):.2f}")
