#!/usr/bin/env python3
"""Developer tool: the table of tools/fleet_tick.py runs of two builds.   fleet_tick_table.py FILE.jsonl ...

Each file holds the JSON lines of alternating processes labelled `parent` and `new` (fleet_tick.py
--label) on one scene.  Per member count: every process's median round time, the median and the
spread (max - min) over ALL blocks of a build, the gain, the gain in units of the larger spread, the
new build's round over N single ticks, and the group's counters of the last `new` process."""
import collections
import json
import sys

import numpy as np

for path in sys.argv[1:]:
    rows = collections.defaultdict(list)
    for text in open(path):
        d = json.loads(text)
        rows[(d["members"], d["label"])].append(d)
    first = next(iter(rows.values()))[0]
    print(f"{path}: scene {first['scene']}, {first['B']} x {first['T']}; round time in us; blocks of {first['rounds_per_block']} rounds")
    print("  N | parent: process medians, median and spread over all blocks | new: the same | gain us, gain / spread | "
          "new round / (N x single tick) | batched launches / single ticks, passes, non-colliding (last new process)")
    for N in sorted({k[0] for k in rows}):
        stat = {}
        for who in ("parent", "new"):
            ds = rows[(N, who)]
            blocks = [b for d in ds for b in d["round_us_blocks"]]
            stat[who] = (float(np.median(blocks)), max(blocks) - min(blocks), [d["round_us_median"] for d in ds], ds)
        p, n = stat["parent"], stat["new"]
        gain, spread = p[0] - n[0], max(p[1], n[1])
        single = float(np.median([b for d in n[3] for b in d["single_tick_us_blocks"]]))
        last = n[3][-1]
        print(f"{N:3d} | {' '.join(f'{m:7.1f}' for m in p[2])}  median {p[0]:7.1f} spread {p[1]:5.1f} | "
              f"{' '.join(f'{m:7.1f}' for m in n[2])}  median {n[0]:7.1f} spread {n[1]:5.1f} | {gain:7.1f} {gain / spread:6.1f} | "
              f"{n[0] / (N * single):.3f} (single tick {single:.1f}) | {last.get('batched_launches')} / {last.get('single_ticks')}, "
              f"passes {sorted(set(last['passes']))}, non-colliding {last['non_colliding'][0]}")
    print()
