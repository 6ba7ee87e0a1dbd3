#!/usr/bin/env python3
"""Strand-index stage timing: one JSON line.

    python tools/index_bench.py [--reads R] [--device D]

* decode_*: ldpc_dna_index_decode on --reads simulated raw reads of the DNA
  code (synth.dna_raw_reads, substitutions 1 %); host buffers in, host buffers
  out, so the time covers the device allocations, the copies both ways and
  k_rs_index_decode;
* strands_*: ldpc_dna_strands on the DNA code (272 x 18432 codeword bytes in,
  18432 x 152 strand bytes out), likewise with its copies.
  Both are timed with HIP events on the null stream the calls use: --warmup
  untimed calls, then --reps timed ones; median, min and max are reported;
* host_*: ldpc_dna_index_decode_host and ldpc_dna_strands_host on one thread
  (wall clock, median of --reps);
* trial: one trial_from_raw_reads on the same reads -- t_index_s (the Python
  wrapper around the decode: string packing + the call + the filter) next to
  the LLR stage's t_llr_s and the first decode's t_first_s of the same run.

The device results are compared with the host functions' before anything is
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
    a = ap.parse_args()
    if L.device_count() <= a.device:
        raise SystemExit("index_bench: no such GPU")
    mod, lib = dna_llr._lib()
    p = dna_llr._p
    cw = synth.load_codewords()
    n_cw, N = cw.shape
    raw = synth.dna_raw_reads(cw, seed=7, n_reads=a.reads, sub=0.01)
    buf, offs, lens = dna_llr._concat(raw[0])
    n = len(lens)
    idx_h, ne_h = np.zeros(n, np.int32), np.zeros(n, np.int32)
    idx_d, ne_d = np.zeros(n, np.int32), np.zeros(n, np.int32)
    sidx = np.ascontiguousarray(dna_llr.strand_indices(), np.int32)
    out_h, out_d = np.zeros((N, 16 + n_cw // 2), np.uint8), np.zeros((N, 16 + n_cw // 2), np.uint8)

    def dec_host():
        mod._check(lib.ldpc_dna_index_decode_host(p(buf), p(offs), p(lens), n, p(idx_h), p(ne_h)))

    def dec_dev():
        mod._check(lib.ldpc_dna_index_decode(p(buf), p(offs), p(lens), n, p(idx_d), p(ne_d), a.device))

    def str_host():
        mod._check(lib.ldpc_dna_strands_host(p(cw), n_cw, N, p(sidx), p(out_h)))

    def str_dev():
        mod._check(lib.ldpc_dna_strands(p(cw), n_cw, N, p(sidx), p(out_d), a.device))

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

    dec_host()
    str_host()
    timed(dec_dev)  # the first warm-up call of each, checked
    timed(str_dev)
    verified = bool(np.array_equal(idx_d, idx_h) and np.array_equal(ne_d, ne_h) and np.array_equal(out_d, out_h))
    res = {}
    for name, fn in (("decode", dec_dev), ("strands", str_dev)):
        for _ in range(max(a.warmup - 1, 0)):
            timed(fn)
        ms = [timed(fn) for _ in range(a.reps)]
        res[name + "_ms_median"] = round(statistics.median(ms), 4)
        res[name + "_ms_min"] = round(min(ms), 4)
        res[name + "_ms_max"] = round(max(ms), 4)
    for name, fn in (("host_decode", dec_host), ("host_strands", str_host)):
        res[name + "_ms_median"] = round(statistics.median([wall(fn) for _ in range(a.reps)]), 4)
    trial = dna_pipeline.trial_from_raw_reads(raw, cw, eps=0.02, align_fn=dna_llr.pad_align, device=a.device)
    out = {
        "tool": "index_bench", "reads": n, "read_bytes": int(len(buf)), "n_cw": n_cw, "N": N,
        "strand_bytes": int(out_d.size), "warmup": a.warmup, "reps": a.reps, **res,
        "cnumerr_hist": {str(k): v for k, v in trial["cnumerr_hist"].items()},
        "trial_t_index_s": round(trial["t_index_s"], 6), "trial_t_llr_s": round(trial["t_llr_s"], 6),
        "trial_t_first_s": round(trial["t_first_s"], 6), "trial_first_success": trial["first_success"],
        "verified_against_host": verified,
    }
    print(json.dumps(out))
    if not verified:
        raise SystemExit("index_bench: device results differ from the host functions'")


if __name__ == "__main__":
    main()
