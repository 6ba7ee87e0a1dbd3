#!/usr/bin/env python3
"""Error-rate simulation on the DNA code: one JSON line per (algorithm, Eb/N0).

    python tools/ber_bench.py [--pchk FILE] [--ebno 3.5,4,4.5,5,6] [--frames F] [--batch B]
                              [--max-iter I] [--algos bp,msa] [--device D] [--seed S]

Per point, over the quantised AWGN channel of synth.awgn_channel at the code's
rate K / N:

* the counters of ErrorRate.run over --frames frames (after one untimed batch),
  and frames_per_s, wall clock of that run: messages, encoder, channel, decoder
  and error counter, all on the device;
* decode_cw_per_s, the yardstick: the decoder's own rate on the same code and
  schedule -- Engine.decode_codes of pre-generated input, the last batch's
  codes read back from the handle and uploaded once, --reps timed calls;
* other_share: the share of the sampled device time (HIP events on every
  launch, a second, shorter run of its own) in the engine's kernel class
  "other": the three kernels of the simulation (k_sim_messages,
  k_channel_codes, k_frame_errors) and the lane pool's reset, one small launch
  per decode.  The encoder's kernels run on the same stream outside the
  classes, so their time is in neither side of the share.

Not a test and has no threshold.  Needs a GPU; there is no fallback.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "dna-ldpc-codes_amd"))
import ldpc_amd as L  # noqa: E402
import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pchk", default=synth.PCHK)
    ap.add_argument("--ebno", default="3.5,4,4.5,5,6")
    ap.add_argument("--frames", type=int, default=16384)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--max-iter", type=int, default=50)
    ap.add_argument("--algos", default="bp,msa")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    if L.device_count() < 1:
        raise SystemExit("ber_bench: no GPU")
    G = L.Graph(a.pchk)
    t0 = time.perf_counter()
    enc = G.encoder()
    t_enc = time.perf_counter() - t0
    rate = enc.K / enc.N
    d_codes = L.DeviceBuffer(a.device, a.batch * G.N)
    d_hard = L.DeviceBuffer(a.device, a.batch * G.N)
    d_iters = L.DeviceBuffer(a.device, 4 * a.batch)
    d_valid = L.DeviceBuffer(a.device, a.batch)
    for algo in a.algos.split(","):
        er = L.ErrorRate(G, algo=algo, device=a.device, batch=a.batch, encoder=enc)
        eng = L.Engine(G, device=a.device, algo=algo)
        for e in [float(x) for x in a.ebno.split(",")]:
            ch = synth.awgn_channel(e, rate)
            er.run_range(ch, a.max_iter, a.seed, a.frames, a.batch)  # untimed: first-use allocations, the table upload
            t0 = time.perf_counter()
            r = er.run(ch, a.max_iter, a.seed, frames=a.frames)
            dt = time.perf_counter() - t0
            # the yardstick: the last batch's codes, decoded alone
            _, codes, _ = er.read(a.batch)
            d_codes.upload(codes)
            eng.decode_codes(d_codes.at(0), ch[1], L.IN_LLR, a.batch, a.max_iter, d_hard.at(0), None, L.POST_LLR,
                             d_iters.at(0), d_valid.at(0))
            eng.sync()
            t0 = time.perf_counter()
            for _ in range(a.reps):
                eng.decode_codes(d_codes.at(0), ch[1], L.IN_LLR, a.batch, a.max_iter, d_hard.at(0), None, L.POST_LLR,
                                 d_iters.at(0), d_valid.at(0))
            eng.sync()
            dt_dec = (time.perf_counter() - t0) / a.reps
            # the kernel classes, a run of their own: events on every launch
            er.profile(1)
            er.run(ch, a.max_iter, a.seed, frames=min(a.frames, 2 * a.batch))
            st = er.stats()
            er.profile(0)
            total_ms = sum(v["ms"] for v in st.values())
            out = {"code": os.path.basename(a.pchk), "N": G.N, "K": enc.K, "algo": algo, "ebno_db": e,
                   "max_iter": a.max_iter, "batch": a.batch, "seed": a.seed, "encoder_create_s": round(t_enc, 3)}
            out.update({k: v for k, v in r.items() if k != "iter_hist"})
            out["iter_hist"] = r["iter_hist"].tolist()
            out.update(fer=r["frame_err"] / r["frames"], ber=r["bit_err"] / (r["frames"] * G.N),
                       raw_ber=r["raw_bit_err"] / (r["frames"] * G.N), mean_iters=r["iter_sum"] / r["frames"],
                       frames_per_s=round(r["frames"] / dt, 1), decode_cw_per_s=round(a.batch / dt_dec, 1),
                       other_share=round(st["other"]["ms"] / total_ms, 5) if total_ms else None,
                       class_ms={k: round(v["ms"], 3) for k, v in st.items()},
                       other_launches=st["other"]["launches"])
            print(json.dumps(out), flush=True)
        er.close()
        eng.close()


if __name__ == "__main__":
    main()
