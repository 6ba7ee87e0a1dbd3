#!/usr/bin/env python3
"""Whole-trial timing, raw reads to decode result: one JSON line, also written
to --out.

    python tools/trial_bench.py [--reads R] [--device D] [--speculate N] [--out FILE]

The input is one trial's raw reads: --reads simulated raw reads of the DNA
code (synth.dna_raw_reads, seed 41, 1 % substitutions, deletions 5e-4 per
base, no insertions -- the channel of the end-to-end test and of
tools/plan_bench.py), packed once outside the timed calls.  Two ways from those
reads to the trial's result, in one process:

* host_*: dna_pipeline.trial_from_raw_reads(native=True) -- ldpc_dna_reads_llr
  (the fp64 LLR matrix, mask and codes to the host), then decode_trial:
  ldpc_decode_codes from the host codes, numpy for the error and re_decode
  counts, fp64 rows through ldpc_decode for every second decode;
* resident_*: dna_pipeline.ResidentTrial.run_raw -- ldpc_trial_run_reads, the
  decoder input never leaving the device.  The handle is created once, outside
  the timed calls (resident_create_ms), as a caller running many trials would.

Every figure is wall clock around a synchronous call: --warmup untimed calls,
then --reps timed ones; median, min and max.  The stage times each path
reports itself (t_llr_s, t_first_s, t_second_s; the resident path's are the
library's own) are given as medians over the same calls.  Before anything is
timed the two results are compared in every field.  --speculate N (DESIGN.md
sec. 8.10) times the resident path with up to N eps2 steps per second decode
(-1: as many as fit; 0, the default: off): the counters of the eps2 loop are
reported, and before anything is timed the resident result is also compared in
every field, hard, iters and valid included, with that of the same handle at
--speculate 0.  Needs a GPU; there is no fallback.
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
import dna_pipeline as P  # noqa: E402
import synth  # noqa: E402

FIELDS = ("n", "first_success", "second_success", "fail_first", "fail_second", "second_iterations", "first_errors",
          "second_errors", "erasure_index", "n_erased_strands", "n_reads_valid", "n_align_pairs", "n_reads_dropped",
          "cnumerr_hist")
STAGES = ("t_llr_s", "t_first_s", "t_second_s")
COUNTERS = ("second_decodes", "second_rows", "second_rows_used", "code_absmax", "steps_per_decode")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=72000)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--speculate", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "trial_bench.json"))
    a = ap.parse_args()
    if L.device_count() <= a.device:
        raise SystemExit("trial_bench: no such GPU")
    cw = synth.load_codewords()
    G = L.graph(L.default_pchk())
    seqs, quals = synth.dna_raw_reads(cw, seed=41, n_reads=a.reads, sub=0.01, ins=0.0, dele=5e-4)
    raw = (dna_llr._concat(seqs), np.ascontiguousarray(quals, np.int32))
    decode_fn = P.gpu_decode_fn(G)
    t0 = time.perf_counter()
    T = P.ResidentTrial(G, cw, device=a.device)
    create_ms = (time.perf_counter() - t0) * 1e3

    def host_path():
        return P.trial_from_raw_reads(raw, cw, eps=0.02, align_fn="star", decode_fn=decode_fn, device=a.device,
                                      native=True)

    def resident_path():
        return T.run_raw(raw, eps=0.02)

    plain = resident_path()  # a new handle speculates nothing
    T.set_speculation(a.speculate)
    old, new = host_path(), resident_path()
    same_as_plain = bool(all(new[k] == plain[k] for k in FIELDS)
                         and all(np.array_equal(new[k], plain[k]) for k in ("hard", "iters", "valid", "kind")))
    del plain  # (as the parent of this option ran: two results alive while timing)
    verified = bool(same_as_plain and all(new[k] == old[k] for k in FIELDS) and np.array_equal(new["hard"], old["hard"])
                    and np.array_equal(new["kind"], old["llr"].kind) and new["resident"]
                    and P.report(new) == P.report(old))

    def measure(fn):
        for _ in range(max(a.warmup - 1, 0)):  # the checked call above was the first warm-up
            fn()
        ms, stages = [], {k: [] for k in STAGES}
        for _ in range(a.reps):
            t = time.perf_counter()
            r = fn()
            ms.append((time.perf_counter() - t) * 1e3)
            for k in STAGES:
                stages[k].append(r[k] * 1e3)
        res = {"ms_median": round(statistics.median(ms), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3)}
        res.update({k[2:-2] + "_ms_median": round(statistics.median(v), 3) for k, v in stages.items()})
        return res

    out = {"tool": "trial_bench", "reads": len(seqs), "read_bytes": int(raw[0][2].sum()), "warmup": a.warmup,
           "reps": a.reps, "first_success": new["first_success"], "second_success": new["second_success"],
           "second_iterations": new["second_iterations"], "erased_strands": new["n_erased_strands"],
           "erasure_index": len(new["erasure_index"]), "resident_create_ms": round(create_ms, 3),
           "speculate": a.speculate, "same_as_speculate_0": same_as_plain}
    out.update({k: new[k] for k in COUNTERS})
    for name, fn in (("host", host_path), ("resident", resident_path)):
        out.update({f"{name}_{k}": v for k, v in measure(fn).items()})
    out["resident_speedup_vs_host"] = round(out["host_ms_median"] / out["resident_ms_median"], 2)
    out["verified_identical"] = verified
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not verified:
        raise SystemExit("trial_bench: the resident trial's result differs from the host path's")


if __name__ == "__main__":
    main()
