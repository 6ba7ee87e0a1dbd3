#!/usr/bin/env python3
"""Encoder throughput: one JSON line.

    python tools/encode_bench.py [--pchk FILE] [--batch B] [--device D]

* construct_s: ldpc_encoder_create on the host (GF(2) elimination), median of 3;
* host_cw_per_s: ldpc_encode_host on --host-batch messages (wall clock);
* device_*: ldpc_encoder_encode_device on device-resident messages, timed with
  HIP events on the stream it is given: --warmup untimed calls, then --reps
  timed ones; median, min and max are reported.  device_fraction_of_8TBps is
  the algorithmic traffic (K + N) * B bytes (messages in, codewords out, one
  byte per bit) over the median time, as a share of 8 TB/s.

The first min(B, 512) device codewords are compared with the host encoder's
before anything is timed.  Needs a GPU; there is no fallback.
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
import synth  # noqa: E402

HBM_BYTES_PER_S = 8e12


def _hip():
    """The HIP runtime the library itself loaded (for events and a stream)."""
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
    ap.add_argument("--pchk", default=synth.PCHK)
    ap.add_argument("--batch", type=int, default=100_000)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--host-batch", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9)
    a = ap.parse_args()
    if L.device_count() <= a.device:
        raise SystemExit("encode_bench: no such GPU")
    G = L.Graph(a.pchk)
    tc = []
    for _ in range(3):
        t0 = time.perf_counter()
        enc = L.Encoder(G)
        tc.append(time.perf_counter() - t0)
    B, K, N = a.batch, enc.K, enc.N
    msg = np.random.default_rng(1).integers(0, 2, size=(B, K), dtype=np.uint8)
    hb = min(B, a.host_batch)
    t0 = time.perf_counter()
    host_cw = enc.encode_host(msg[:hb])
    t_host = time.perf_counter() - t0

    hip = _hip()
    _ok(hip.hipSetDevice(a.device), "hipSetDevice")
    stream, ev0, ev1 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    _ok(hip.hipStreamCreate(C.byref(stream)), "hipStreamCreate")
    _ok(hip.hipEventCreate(C.byref(ev0)), "hipEventCreate")
    _ok(hip.hipEventCreate(C.byref(ev1)), "hipEventCreate")
    d_msg, d_cw = L.DeviceBuffer(a.device, B * K), L.DeviceBuffer(a.device, B * N)
    d_msg.upload(msg)

    def once():
        _ok(hip.hipEventRecord(ev0, stream), "hipEventRecord")
        enc.encode_device(d_msg, B, d_cw, device=a.device, stream=stream)
        _ok(hip.hipEventRecord(ev1, stream), "hipEventRecord")
        _ok(hip.hipEventSynchronize(ev1), "hipEventSynchronize")
        ms = C.c_float()
        _ok(hip.hipEventElapsedTime(C.byref(ms), ev0, ev1), "hipEventElapsedTime")
        return float(ms.value)

    once()
    got = d_cw.download(np.empty((hb, N), np.uint8))
    verified = bool(np.array_equal(got, host_cw))
    for _ in range(max(a.warmup - 1, 0)):
        once()
    ms = [once() for _ in range(a.reps)]
    med = statistics.median(ms)
    out = {
        "tool": "encode_bench", "pchk": os.path.basename(a.pchk), "M": G.M, "N": N, "K": K, "rank": enc.rank,
        "batch": B, "construct_s": round(statistics.median(tc), 6),
        "host_batch": hb, "host_cw_per_s": round(hb / t_host, 1),
        "warmup": a.warmup, "reps": a.reps, "device_ms_median": round(med, 4), "device_ms_min": round(min(ms), 4),
        "device_ms_max": round(max(ms), 4), "device_cw_per_s": round(B / (med * 1e-3), 1),
        "bytes_per_cw": K + N, "device_bytes_per_s": round((K + N) * B / (med * 1e-3), 1),
        "device_fraction_of_8TBps": round((K + N) * B / (med * 1e-3) / HBM_BYTES_PER_S, 5),
        "verified_against_host": verified,
    }
    print(json.dumps(out))
    _ok(hip.hipStreamDestroy(stream), "hipStreamDestroy")
    if not verified:
        raise SystemExit("encode_bench: device codewords differ from the host encoder's")


if __name__ == "__main__":
    main()
