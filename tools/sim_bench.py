#!/usr/bin/env python3
"""Strands to trial result, three routes: one JSON line per workload, also
written to --out.

    python tools/sim_bench.py [--reads R] [--device D] [--out FILE]

Workloads: R reads (72 000) of the DNA code's strands with 1 % substitutions;
the same with insertions and deletions at 0.001 each (ragged strands: the
aligner runs, and with run_sim its candidate reads are the only read bytes that
come down); a coverage sweep of 5 read counts between 60 000 and R with 10
trials each.  Routes from the strands to the trial's result, in one process:

* a_*: the route before the channel existed -- synth.dna_raw_reads (numpy
  random matrices, a Python list of str, a Python loop over reads with an
  insertion or deletion), then ResidentTrial.run_raw on that list; generator
  and trial timed separately.  Its reads are another random stream, so its
  result is not compared, only reported;
* b_*: synth.dna_raw_reads_native(device=D) (k_sim_reads, reads copied down),
  then run_raw on them (reads uploaded again); timed separately;
* c_*: ResidentTrial.run_sim, one library call.  Its t_llr_s covers generator +
  planner + code kernel: the library reports no separate generator time.

Every figure is wall clock around synchronous calls: --warmup untimed calls,
then --reps timed ones; median, min and max.  The handle is created once,
outside the timed calls.  Before anything is timed, b's reads are compared with
the numpy replica's (synth.dna_raw_reads_hashed) and b's and c's results in
every field.  The sweep is timed as a whole (median of 3); the same sweep on
route a is not run but given as (a's generator + trial medians) x 50.
Needs a GPU; there is no fallback.
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
import dna_pipeline as P  # noqa: E402
import synth  # noqa: E402

FIELDS = ("n", "first_success", "second_success", "fail_first", "fail_second", "second_iterations", "first_errors",
          "second_errors", "erasure_index", "n_erased_strands", "n_reads_valid", "n_align_pairs", "n_reads_dropped",
          "cnumerr_hist", "resident")
ARRAYS = ("hard", "kind", "stats", "iters", "valid")
SEED = 41


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t) * 1e3)
    return {"ms_median": round(statistics.median(ms), 3), "ms_min": round(min(ms), 3), "ms_max": round(max(ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=72000)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12", "sim_bench.json"))
    a = ap.parse_args()
    if L.device_count() <= a.device:
        raise SystemExit("sim_bench: no such GPU")
    cw = synth.load_codewords()
    G = L.graph(L.default_pchk())
    strands = synth.dna_strands(cw)
    T = P.ResidentTrial(G, cw, device=a.device)
    T.set_strands(strands)
    lines, ok = [], True
    for name, rates in (("sub", (0.01, 0.0, 0.0)), ("sub_indel", (0.01, 0.001, 0.001))):
        gen_a = lambda: synth.dna_raw_reads(cw, SEED, a.reads, *rates)  # noqa: E731
        gen_b = lambda: synth.dna_raw_reads_native(strands, SEED, a.reads, *rates, device=a.device)  # noqa: E731
        raw_a, raw_b = gen_a(), gen_b()
        want = synth.dna_raw_reads_hashed(strands, SEED, a.reads, *rates)
        stride = synth.sim_stride(strands.shape[1])
        live = np.arange(stride)[None, :] < want[0][2][:, None]
        reads_equal = bool(np.array_equal(raw_b[0][2], want[0][2]) and np.array_equal(raw_b[1], want[1]) and
                           np.array_equal(raw_b[0][0].reshape(-1, stride)[live], want[0][0].reshape(-1, stride)[live]))
        res_a, res_b = T.run_raw(raw_a), T.run_raw(raw_b)
        res_c = T.run_sim(SEED, a.reads, *rates)
        same = bool(all(res_c[k] == res_b[k] for k in FIELDS) and all(np.array_equal(res_c[k], res_b[k]) for k in ARRAYS)
                    and P.report(res_c) == P.report(res_b))
        ok = ok and reads_equal and same
        cand = int(res_c["stats"][2] + res_c["stats"][3])  # aligned strands + read-to-centre alignments
        payload = float((want[0][2] - 16).clip(min=0).mean())
        out = {"tool": "sim_bench", "workload": name, "reads": a.reads, "sub": rates[0], "ins": rates[1], "del": rates[2],
               "warmup": a.warmup, "reps": a.reps, "reads_equal_replica": reads_equal, "b_c_identical": same,
               "read_bytes": int(want[0][2].sum()), "candidate_reads": cand,
               "candidate_bytes_est": int(round(cand * payload)),
               "c_first_success": res_c["first_success"], "c_second_success": res_c["second_success"],
               "a_first_success": res_a["first_success"], "a_second_success": res_a["second_success"]}
        for key, fn in (("a_gen", gen_a), ("a_trial", lambda: T.run_raw(raw_a)), ("b_gen", gen_b),
                        ("b_trial", lambda: T.run_raw(raw_b)), ("c_run_sim", lambda: T.run_sim(SEED, a.reads, *rates))):
            slow = key == "a_gen"  # the slowest step by far: fewer repetitions
            m = timed(fn, 1 if slow else a.warmup, 3 if slow else a.reps)
            out.update({f"{key}_{k}": v for k, v in m.items()})
        llr = [T.run_sim(SEED, a.reads, *rates)["t_llr_s"] * 1e3 for _ in range(a.reps)]
        out["c_llr_ms_median"] = round(statistics.median(llr), 3)  # generator + planner + code kernel, not separated
        out["a_total_ms_median"] = round(out["a_gen_ms_median"] + out["a_trial_ms_median"], 3)
        out["b_total_ms_median"] = round(out["b_gen_ms_median"] + out["b_trial_ms_median"], 3)
        out["c_speedup_vs_a"] = round(out["a_total_ms_median"] / out["c_run_sim_ms_median"], 2)
        out["c_speedup_vs_b"] = round(out["b_total_ms_median"] / out["c_run_sim_ms_median"], 2)
        lines.append(out)
    counts = [int(v) for v in np.linspace(60000, a.reads, 5)]
    rows = P.coverage_sweep(T, counts, trials=10, seed=0, sub=0.01)
    m = timed(lambda: P.coverage_sweep(T, counts, trials=10, seed=0, sub=0.01), 0, 3)
    per_a = lines[0]["a_total_ms_median"]
    lines.append({"tool": "sim_bench", "workload": "sweep", "read_counts": counts, "trials": 10, "sub": 0.01,
                  "sweep_ms_median": m["ms_median"], "sweep_ms_min": m["ms_min"], "sweep_ms_max": m["ms_max"],
                  "per_trial_ms": round(m["ms_median"] / len(rows), 3),
                  "route_a_estimate_ms": round(per_a * len(rows), 1),
                  "decoded": {str(n): sum(r["second_success"] == 272 for r in rows if r["n_reads"] == n) for n in counts}})
    text = "\n".join(json.dumps(x) for x in lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if not ok:
        raise SystemExit("sim_bench: the device reads or run_sim's result differ from their comparators")


if __name__ == "__main__":
    main()
