#!/usr/bin/env python3
"""Read-planner stage timing: one JSON line, also written to --out.

    python tools/plan_bench.py [--reads R] [--device D] [--out FILE]

The input is one trial's raw reads: --reads simulated raw reads of the DNA
code (synth.dna_raw_reads, seed 41, 1 % substitutions, deletions 5e-4 per
base, no insertions -- the channel of the end-to-end test and of profiles/r9).
Three ways from those reads to the decoder's input, in one process:

* python_*: the existing path, dna_llr.split_reads (index decode on the GPU)
  followed by dna_llr.build_llr(align_fn="star") -- the Python planner around
  the GPU distance, aligner and LLR calls;
* native_*: ldpc_dna_reads_llr from the packed raw reads
  (dna_llr.build_llr_native; the packing itself, dna_llr._concat, is done once
  outside the timed calls and reported as pack_ms); native_plan_*: ldpc_dna_plan
  alone on the same reads (the planner without the LLR kernel and its copies);
* host_plan_*: ldpc_dna_plan_host on one CPU thread.

Every figure is wall clock around a synchronous call: --warmup untimed calls,
then --reps timed ones; median, min and max.  Before anything is timed the
native LLRs, masks, codes and kinds are compared with the Python path's and the
device plan with the host plan.  Needs a GPU; there is no fallback.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dna-ldpc-codes_amd"))
import ldpc_amd as L  # noqa: E402
import dna_llr  # noqa: E402
import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=72000)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10", "plan_bench.json"))
    a = ap.parse_args()
    if L.device_count() <= a.device:
        raise SystemExit("plan_bench: no such GPU")
    cw = synth.load_codewords()
    seqs, quals = synth.dna_raw_reads(cw, seed=41, n_reads=a.reads, sub=0.01, ins=0.0, dele=5e-4)
    t0 = time.perf_counter()
    packed = dna_llr._concat(seqs)
    pack_ms = (time.perf_counter() - t0) * 1e3
    q32 = np.ascontiguousarray(quals, np.int32)

    def python_path():
        reads = dna_llr.split_reads(seqs, quals, device=a.device)
        return dna_llr.build_llr(*reads, eps=0.02, align_fn="star", device=a.device)

    def native_path():
        return dna_llr.build_llr_native(None, packed, q32, eps=0.02, device=a.device)[0]

    def native_plan():
        return dna_llr.plan_llr_native(None, packed, q32, device=a.device)

    def host_plan():
        return dna_llr.plan_llr_native(None, packed, q32, host=True)

    old, new, dev, host = python_path(), native_path(), native_plan(), host_plan()
    R = int(host.row_ptr[-1])
    verified = bool(
        np.array_equal(old.llr.view(np.uint64), new.llr.view(np.uint64)) and np.array_equal(old.int_mask, new.int_mask)
        and old.codes is not None and new.codes is not None and np.array_equal(old.codes, new.codes)
        and np.array_equal(old.kind, new.kind) and np.array_equal(dev.kind, host.kind)
        and np.array_equal(dev.row_ptr, host.row_ptr) and np.array_equal(dev.rows[:R], host.rows[:R])
        and np.array_equal(dev.row_q[:R], host.row_q[:R]) and np.array_equal(dev.kind, new.kind))

    def measure(fn):
        for _ in range(max(a.warmup - 1, 0)):  # the checked call above was the first warm-up
            fn()
        ms = []
        for _ in range(a.reps):
            t = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t) * 1e3)
        return {"ms_median": round(statistics.median(ms), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3)}

    out = {"tool": "plan_bench", "reads": len(seqs), "read_bytes": int(packed[2].sum()), "warmup": a.warmup,
           "reps": a.reps, "reads_valid": new.n_reads_valid, "distance_pairs": new.n_pairs,
           "aligned_strands": new.n_aligned_strands, "align_pairs": new.n_align_pairs, "rows": R,
           "erased_strands": int(len(new.erased)), "pack_ms": round(pack_ms, 3)}
    for name, fn in (("python", python_path), ("native", native_path), ("native_plan", native_plan),
                     ("host_plan", host_plan)):
        out.update({f"{name}_{k}": v for k, v in measure(fn).items()})
    out["native_speedup_vs_python"] = round(out["python_ms_median"] / out["native_ms_median"], 2)
    out["verified_identical"] = verified
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not verified:
        raise SystemExit("plan_bench: the native results differ from the Python path's")


if __name__ == "__main__":
    main()
