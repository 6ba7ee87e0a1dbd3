"""Table of the timings in a directory written by speed_runs.sh: per figure
every process of the parent and of the new build, the parent's own
process-to-process spread (min .. max), the new build's median and whether it
lies within that spread.

    python speed_table.py speed > speed_tables.md
"""
import glob
import json
import os
import statistics
import sys

d = sys.argv[1]


def line(path):
    rows = [ln for ln in open(path) if ln.startswith("{")]
    out = json.loads(rows[-1])
    return {**out, **out.get("config", {})}  # bench.py keeps the dna272 figures under "config"


FIGURES = [("dna272", k) for k in ("ms_per_decode_device", "host_api_ms_median", "host_api_ms_min",
                                   "host_api_pinned_ms_median", "host_api_pinned_ms_min", "host_api_llr_ms_median",
                                   "host_api_llr_ms_min")]
FIGURES += [(leg, k) for leg in ("headline", "config5") for k in ("value", "ms_per_step")]

print("| leg | figure | parent, per process | parent min .. max (spread) | new, per process | new median | within |")
print("|---|---|---|---|---|---|---|")
for leg, key in FIGURES:
    v = {who: [line(f)[key] for f in sorted(glob.glob(os.path.join(d, f"{leg}_{who}_*.json")))]
         for who in ("parent", "new")}
    lo, hi, med = min(v["parent"]), max(v["parent"]), statistics.median(v["new"])
    spread = (hi - lo) / statistics.median(v["parent"]) * 100
    inside = "yes" if lo <= med <= hi else f"no ({(med / statistics.median(v['parent']) - 1) * 100:+.2f} % of the parent's median)"
    print(f"| {leg} | `{key}` | {' / '.join(map(str, v['parent']))} | {lo} .. {hi} ({spread:.2f} %) | "
          f"{' / '.join(map(str, v['new']))} | {med:.6g} | {inside} |")
