#!/usr/bin/env python3
"""Aligner stage timing: one JSON line, also written to --out.

    python tools/align_bench.py [--reads R] [--device D] [--out FILE]

The input is the candidate groups that plan_llr hands the aligner in one trial:
--reads simulated raw reads of the DNA code (synth.dna_raw_reads, 1 %
substitutions, deletions 5e-4 per base -- the channel of the end-to-end test),
index-decoded, grouped, and filtered by the edit-distance rule.

* align_*: ldpc_dna_star_align on those groups; host buffers in, host buffers
  out, so the time covers the device allocations, the copies both ways,
  k_edit_distance for the centres, k_star_align_pairs, and the merge on the
  host.  Timed with HIP events on the null stream the call uses: --warmup
  untimed calls, then --reps timed ones; median, min and max are reported;
* host_align_ms_median: ldpc_dna_star_align_host on one thread (wall clock,
  median of --host-reps);
* trial: one trial_from_raw_reads(align_fn="star") on the same reads --
  t_align_s (the Python wrapper around the call: string packing + the call +
  unpacking the rows) next to the LLR stage's t_llr_s of the same run.

The device result is compared with the host function's before anything is
timed.  Needs a GPU; there is no fallback.
"""
import argparse
import ctypes as C
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
import dna_pipeline  # noqa: E402
import synth  # noqa: E402


def _hip():
    """The HIP runtime the library itself loaded (for events)."""
    L.lib()
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line:
                return C.CDLL(line.split()[-1])
    raise RuntimeError("the HIP runtime is not loaded")


def _ok(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what}: HIP error {rc}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=72000)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r9", "align_bench.json"))
    a = ap.parse_args()
    if L.device_count() <= a.device:
        raise SystemExit("align_bench: no such GPU")
    mod, lib = dna_llr._lib()
    p = dna_llr._p
    cw = synth.load_codewords()
    raw = synth.dna_raw_reads(cw, seed=41, n_reads=a.reads, sub=0.01, ins=0.0, dele=5e-4)
    reads = dna_llr.split_reads(*raw, device=a.device)
    groups = []

    def record(cand):  # the groups plan_llr would align
        groups.append(list(cand))
        return dna_llr.pad_align(cand)

    dna_llr.plan_llr(*reads, align_fn=record, device=a.device)
    buf, offs, lens = dna_llr._concat([s for g in groups for s in g])
    n, G = len(lens), len(groups)
    gp = np.zeros(G + 1, np.int64)
    gp[1:] = np.cumsum([len(g) for g in groups])
    cap = int(sum(len(g) * (2 * max(map(len, g)) + 16) for g in groups))
    need, stats = C.c_int64(0), np.zeros(3, np.int64)

    class Out:
        def __init__(self):
            self.center, self.width = np.zeros(G, np.int32), np.zeros(G, np.int32)
            self.out_ptr, self.out, self.dist = np.zeros(G + 1, np.int64), np.zeros(cap, np.uint8), np.zeros(n, np.int32)

        def head(self):
            return (p(buf), p(offs), p(lens), n, p(gp), G, p(self.center), p(self.width), p(self.out_ptr), p(self.out),
                    cap, C.byref(need), p(self.dist))

        def same(self, o):
            return all(np.array_equal(x, y) for x, y in ((self.center, o.center), (self.width, o.width),
                                                         (self.out_ptr, o.out_ptr), (self.out, o.out), (self.dist, o.dist)))

    h, d = Out(), Out()

    def host():
        mod._check(lib.ldpc_dna_star_align_host(*h.head()))

    def dev():
        mod._check(lib.ldpc_dna_star_align(*d.head(), a.device, 0, p(stats)))

    hip = _hip()
    _ok(hip.hipSetDevice(a.device), "hipSetDevice")
    ev0, ev1 = C.c_void_p(), C.c_void_p()
    _ok(hip.hipEventCreate(C.byref(ev0)), "hipEventCreate")
    _ok(hip.hipEventCreate(C.byref(ev1)), "hipEventCreate")

    def timed(fn):
        _ok(hip.hipEventRecord(ev0, None), "hipEventRecord")
        fn()
        _ok(hip.hipEventRecord(ev1, None), "hipEventRecord")
        _ok(hip.hipEventSynchronize(ev1), "hipEventSynchronize")
        ms = C.c_float()
        _ok(hip.hipEventElapsedTime(C.byref(ms), ev0, ev1), "hipEventElapsedTime")
        return float(ms.value)

    def wall(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    host()
    timed(dev)  # the first warm-up call, checked
    verified = bool(h.same(d))
    for _ in range(max(a.warmup - 1, 0)):
        timed(dev)
    ms = [timed(dev) for _ in range(a.reps)]
    host_ms = statistics.median([wall(host) for _ in range(a.host_reps)])
    trial = dna_pipeline.trial_from_raw_reads(raw, cw, eps=0.02, align_fn="star", device=a.device)
    out = {
        "tool": "align_bench", "reads": len(raw[0]), "groups": G, "group_reads": n, "read_bytes": int(lens.sum()),
        "pairs": int(stats[2]), "passes": int(stats[1]), "host_groups": int(stats[0]), "row_bytes": int(need.value),
        "width_not_136": int((d.width != 136).sum()), "warmup": a.warmup, "reps": a.reps,
        "align_ms_median": round(statistics.median(ms), 4), "align_ms_min": round(min(ms), 4),
        "align_ms_max": round(max(ms), 4), "host_reps": a.host_reps, "host_align_ms_median": round(host_ms, 4),
        "trial_n_align_pairs": trial["n_align_pairs"], "trial_t_align_s": round(trial["t_align_s"], 6),
        "trial_t_llr_s": round(trial["t_llr_s"], 6), "trial_t_index_s": round(trial["t_index_s"], 6),
        "trial_t_first_s": round(trial["t_first_s"], 6), "trial_first_success": trial["first_success"],
        "trial_second_success": trial["second_success"], "trial_n_erased_strands": trial["n_erased_strands"],
        "verified_against_host": verified,
    }
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not verified:
        raise SystemExit("align_bench: the device result differs from the host function's")


if __name__ == "__main__":
    main()
