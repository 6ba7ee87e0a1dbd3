"""Codes, channels and references of the error-rate simulation's tests
(tests/test_channel_sim.py, tests/test_channel_sim_gpu.py; DESIGN.md sec.
8.11).  Plain numpy and the CPU oracle, no GPU.

Codes, built as the suite already builds them:
  r288   random (8,72)-regular, Q = 4, N = 288
  r96    random (3,6)-regular, Q = 16, N = 96
  rs5    rs_ldpc(5, 16, 4), N = 512
  irr    the 40 x 130 irregular code of refdec_cases (a zero column and
         redundant rows: the information positions are not the first K)
"""
import functools
import os

import numpy as np

import refdec_cases

CODES = ("r288", "r96", "rs5", "irr")
ALGOS = {"bp": 0, "msa": 1, "qmsa": 2}
MAX_ITER = 20
FRAMES = 320


@functools.lru_cache(maxsize=None)
def edges(name):
    from test_random_graphs_gpu import _regular_graph
    if name == "r288":
        return _regular_graph(np.random.default_rng(288), 4)
    if name == "r96":
        return _regular_graph(np.random.default_rng(96), 16, dv=3, dc=6)
    if name == "rs5":
        return refdec_cases.make_edges("rs5")
    if name == "irr":
        return refdec_cases.irregular_edges()
    if name == "q64":  # N = 4608: the error counter's block-per-frame shape
        return _regular_graph(np.random.default_rng(64), 64)
    if name in ("n2048", "n2049"):  # the error counter's last wave-per-frame size; the first block-per-frame one, N % 8 != 0
        N = int(name[1:])
        rows = [j % 64 for j in range(N)] + [(j + 1) % 64 for j in range(0, N, 2)]
        cols = list(range(N)) + list(range(0, N, 2))
        return 64, N, rows, cols
    if name == "n13":  # N = 13: shorter than two words, not a multiple of 8
        rows = [j % 4 for j in range(13)] + [(j + 1) % 4 for j in range(0, 13, 2)]
        cols = list(range(13)) + list(range(0, 13, 2))
        return 4, 13, rows, cols
    raise KeyError(name)


def pchk(tmp, name):
    """The code as a .pchk under tmp (for the oracle; L.Graph loads the same file)."""
    path = os.path.join(str(tmp), name + ".pchk")
    if not os.path.exists(path):
        refdec_cases.write_pchk(path, *edges(name))
    return path


@functools.lru_cache(maxsize=None)
def channels(rate):
    """name -> (thr, table): the three kinds, and a fine AWGN table (step 1/64
    at 1 dB) whose outer levels lie inside the noise, so the +-127 clip is hit."""
    import synth
    return {"awgn4": synth.awgn_channel(4.0, rate), "bsc": synth.bsc_channel(0.02), "bec": synth.bec_channel(0.1),
            "clip": synth.awgn_channel(1.0, rate, step=1 / 64)}


def count(hard, cw, codes, mask, table, iters, valid, kind=0):
    """The records by numpy: the reference of ldpc_frame_errors_host."""
    import ldpc_amd
    B, N = codes.shape
    cw = np.zeros((B, N), np.uint8) if cw is None else (np.asarray(cw) & 1)
    mask = np.ones(N, np.uint8) if mask is None else mask
    d = (np.asarray(hard) & 1) != cw
    val = np.asarray(table)[codes.astype(np.int64) + 128]
    with np.errstate(invalid="ignore"):
        raw = np.where(val >= (1.0 if kind == 1 else 0.0), 0, 1)  # a NaN is not >= 0: it reads as 1
    rec = np.zeros(B, ldpc_amd.BER_RECORD)
    rec["bit_err"] = d.sum(1)
    rec["info_err"] = (d & (mask[None, :] != 0)).sum(1)
    rec["raw_err"] = (raw != cw).sum(1)
    rec["erased"] = (codes == 0).sum(1)
    rec["iters"] = 0 if iters is None else iters
    rec["valid"] = 0 if valid is None else (np.asarray(valid) != 0)
    return rec


def oracle_decode(og, algo, qparams=None, tie_seed=0):
    """decode(codes, table, kind, b0, max_iter) -> (hard, iters, valid) by the CPU oracle."""
    def decode(codes, table, kind, b0, max_iter):
        llr = np.asarray(table)[np.asarray(codes).astype(np.int64) + 128]
        if ALGOS[algo] >= 2:
            q, step, beta = qparams
            h, _, it, v = og.decode_int_batch(llr, max_iter, ALGOS[algo], q, step, beta, seed=tie_seed, threads=4)
        else:
            h, _, it, v = og.decode_batch(llr, max_iter, ALGOS[algo], threads=4, want_post=False)
        return h, it, v
    return decode


def reference_records(og, enc, channel, algo, seed, b0, B, max_iter=MAX_ITER, qparams=None):
    """Frames b0 .. b0 + B - 1 the slow way: random_codewords (or zeros) ->
    the numpy replica of the channel -> the oracle -> the numpy count."""
    import synth
    thr, table = channel[0], channel[1]
    cw = np.zeros((B, og.N), np.uint8) if enc is None else synth.random_codewords(enc, b0, B, seed)
    codes = synth.channel_codes(cw, b0, B, seed, thr)
    h, it, v = oracle_decode(og, algo, qparams)(codes, table, 0, b0, max_iter)
    mask = None
    if enc is not None:
        mask = np.zeros(og.N, np.uint8)
        mask[enc.info_pos] = 1
    return count(h, cw, codes, mask, table, it, v)


def plain_loop(rec, max_iter, frames=None, target=None, max_frames=None):
    """Check_End's rule frame by frame over records of frames 0, 1, ...: the
    result dict ErrorRate.run / ber_run_host must equal."""
    import ldpc_amd
    out = {k: 0 for k in ldpc_amd.BER_COUNTERS}
    hist = np.zeros(max_iter + 1, np.int64)
    limit = frames if frames is not None else max_frames
    for b in range(limit):
        r = rec[b]
        out["frames"] += 1
        out["bit_err"] += int(r["bit_err"])
        out["info_err"] += int(r["info_err"])
        out["frame_err"] += int(r["bit_err"] > 0)
        out["undetected"] += int(r["bit_err"] > 0 and r["valid"] != 0)
        out["detected"] += int(r["valid"] == 0)
        out["raw_bit_err"] += int(r["raw_err"])
        out["raw_frame_err"] += int(r["raw_err"] > 0)
        out["erased"] += int(r["erased"])
        out["iter_sum"] += int(r["iters"])
        hist[r["iters"]] += 1
        if frames is None and out["frame_err"] >= target:
            break
    out["iter_hist"] = hist
    return out


def same_result(got, want, what=""):
    for k in want:
        if k == "iter_hist":
            assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
        else:
            assert got[k] == want[k], (what, k, got[k], want[k])


def planted(rng, B, N, mask):
    """hard / cw / codes / iters / valid with the planted frames: 0 no errors,
    1 errors only in parity positions, 2 every bit wrong; the rest random."""
    cw = rng.integers(0, 2, (B, N)).astype(np.uint8)
    hard = cw ^ (rng.random((B, N)) < 0.1).astype(np.uint8)
    codes = rng.integers(-127, 128, (B, N)).astype(np.int8)
    codes[rng.random((B, N)) < 0.05] = 0
    codes[3, 0], codes[3, N - 1] = 3, -5  # nan_table's NaN entries
    codes[4, N // 2] = -128  # table index 0 (the channel kernel never emits it; a caller's codes may)
    hard[0] = cw[0]
    hard[1] = cw[1] ^ (mask == 0)
    hard[2] = cw[2] ^ 1
    iters = rng.integers(0, MAX_ITER + 1, B).astype(np.int32)
    valid = rng.integers(0, 2, B).astype(np.uint8)
    return hard, cw, codes, iters, valid


def nan_table(table):
    """A copy with NaN entries (the raw rule: not >= 0 -> 1), -0.0 and an infinity."""
    t = np.array(table, copy=True)
    t[128 + 3], t[128 - 5], t[128 + 7], t[128 - 9] = np.nan, np.nan, -0.0, -np.inf
    return t
