"""Tables of the alternating timing runs in speed/: per tool and figure (every
*_ms_median key the tool prints) the three values of each commit, the medians,
the parent's own spread (max - min of its three runs) and whether the new
median lies within that spread of the parent's.

    python speed_table.py speed > speed_tables.md
"""
import glob
import json
import os
import statistics
import sys

d = sys.argv[1]
for tool in ("plan_bench", "align_bench", "trial_bench"):
    runs = {b: [json.load(open(f)) for f in sorted(glob.glob(os.path.join(d, f"{tool}_{b}_*.json")))]
            for b in ("parent", "new")}
    if not runs["parent"] or not runs["new"]:
        continue
    print(f"\n## tools/{tool}.py ({len(runs['parent'])} parent runs, {len(runs['new'])} new runs, ms)\n")
    print("| figure | parent runs | new runs | parent median (spread) | new median | within the parent's spread |")
    print("|---|---|---|---|---|---|")
    for k in [k for k in runs["parent"][0] if k.endswith("_ms_median")]:
        p, n = [r[k] for r in runs["parent"]], [r[k] for r in runs["new"]]
        pm, nm, spread = statistics.median(p), statistics.median(n), max(p) - min(p)
        verdict = "yes" if abs(nm - pm) <= spread else "faster" if nm < pm else "NO (+%.2f %%)" % (100 * (nm - pm) / pm)
        print(f"| `{k}` | {', '.join('%.3f' % v for v in p)} | {', '.join('%.3f' % v for v in n)} | "
              f"{pm:.3f} ({spread:.3f}) | {nm:.3f} | {verdict} |")
