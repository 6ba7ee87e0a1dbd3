"""The ordered launch list of a rocprofv3 kernel trace (--kernel-trace
--output-format csv): one line per dispatch in start order, kernel name (its
argument list cut), grid, workgroup and LDS bytes, runs of equal lines folded
to "N x line".

    python trace_list.py run_kernel_trace.csv > launches.txt
"""
import csv
import re
import sys

rows = list(csv.DictReader(open(sys.argv[1])))
cols = rows[0].keys() if rows else []
pick = lambda p: [c for c in cols if c.lower().startswith(p)]
grid, wg, lds = pick("grid_size"), pick("workgroup_size"), pick("lds_block_size")
rows.sort(key=lambda r: (int(r["Start_Timestamp"]), int(r.get("Dispatch_Id", 0))))
out = []
for r in rows:
    name = re.sub(r"\(.*", "", r["Kernel_Name"].replace("(anonymous namespace)::", ""))
    line = "%s grid %s wg %s lds %s" % (name, "x".join(r[c] for c in grid), "x".join(r[c] for c in wg),
                                        "+".join(r[c] for c in lds))
    if out and out[-1][1] == line:
        out[-1][0] += 1
    else:
        out.append([1, line])
for n, line in out:
    print("%d x %s" % (n, line))
print("dispatches", len(rows), file=sys.stderr)
