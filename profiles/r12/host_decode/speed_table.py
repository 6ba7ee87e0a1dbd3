"""Tables of the host-API timings in speed/: per figure the three runs of the
parent and of the new build, the parent's spread (min .. max of its three
runs) and whether each of the new build's runs lies within it.

    python speed_table.py speed > speed_tables.md
"""
import json
import os
import sys

d = sys.argv[1]


def line(path):
    rows = [ln for ln in open(path) if ln.startswith("{")]
    out = json.loads(rows[-1])
    return {**out, **out.get("config", {})}  # bench.py keeps the dna272 figures under "config"


FIGURES = [("dna272", k) for k in ("host_api_ms_median", "host_api_ms_min", "host_api_pinned_ms_median",
                                   "host_api_pinned_ms_min", "host_api_llr_ms_median", "host_api_llr_ms_min",
                                   "ms_per_decode_device")]
FIGURES += [("multi", k) for k in ("codes_ms_median", "codes_ms_min", "llr_ms_median", "llr_ms_min")]

print("| run | figure (ms) | parent 1 / 2 / 3 | new 1 / 2 / 3 | parent's spread | new within |")
print("|---|---|---|---|---|---|")
for run, key in FIGURES:
    v = {who: [line(os.path.join(d, f"{run}_{who}_{i}.json"))[key] for i in (1, 2, 3)] for who in ("parent", "new")}
    lo, hi = min(v["parent"]), max(v["parent"])
    inside = sum(lo <= x <= hi for x in v["new"])
    below = sum(x < lo for x in v["new"])
    note = f"{inside} of 3" + (f", {below} faster" if below else "") + \
        (f", {3 - inside - below} slower (max +{(max(v['new']) / hi - 1) * 100:.1f} %)" if 3 - inside - below else "")
    print(f"| {run} | {key} | {' / '.join(map(str, v['parent']))} | {' / '.join(map(str, v['new']))} | "
          f"{lo} .. {hi} | {note} |")
