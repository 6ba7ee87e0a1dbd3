"""CPU tests of the error-rate simulation: the channel
tables, the numpy replica's statistics, the host forms against the replica and
a numpy count, and the loop (ldpc_ber_run_host with the CPU oracle as decoder)
against a plain Python loop over the same frames.  Every comparison is exact;
the one bound, 6 sigma + 1 on a code's count, is the binomial's own.

Observed here (seed 11, 320 frames, max_iter 20, random codewords, AWGN step
1/16 at the code's rate K / N):
  r96  4 dB  bp   FER 0.025, 3 undetected, 5 detected, counts 0..20 (13 distinct)
  r96  4 dB  msa  FER 0.041, 2 undetected, 11 detected
  irr  4 dB  bp   FER 0.113, 27 undetected, 9 detected
  irr  4 dB  msa  FER 0.109, 30 undetected, 5 detected
  r96  2 dB  bp / msa: frame 0 is in error (the target = 1 case)
"""
import functools
import math

import numpy as np
import pytest

import channel_cases as cc

SEED = 11


# ---------------------------------------------------------------------------
# tables
# ---------------------------------------------------------------------------
def _tables():
    import synth
    t = {f"awgn{db}": synth.awgn_channel(db, 0.875) for db in (1, 4, 7)}
    t.update(bsc=synth.bsc_channel(0.02), bec=synth.bec_channel(0.1), clip=synth.awgn_channel(1.0, 0.875, step=1 / 64))
    return t


def test_tables_are_monotone_and_sum_to_one(L):
    import synth
    for name, (thr, table) in _tables().items():
        assert thr.dtype == np.uint64 and thr.shape == (254,) and table.shape == (256,), name
        assert (np.diff(thr.astype(np.int64)) >= 0).all() and int(thr[-1]) <= synth.SIM_ONE, name
        p = synth.channel_probs(thr)
        assert p.shape == (255,) and (p >= 0).all(), name
        # the probabilities are differences of integers over 2^53: their sum is exactly 1
        assert int(np.diff(np.concatenate([[0], thr.astype(np.int64), [synth.SIM_ONE]])).sum()) == synth.SIM_ONE, name


def test_awgn_table_is_the_quantised_gaussian_and_mirror_symmetric(L):
    """P(code k | x = +1), read from thr, against the Gaussian's own cell
    probabilities for x = -1 at -k: Phi is evaluated at mirrored arguments, so
    the two differ by rounding alone: erfc's result and its argument (a few
    ulp of a value below 2, 2^-52 each) and the floor (2^-53), at both ends of
    a cell on both sides.  16 units of 2^-53 bound that; a wrong cell is off by
    a cell's probability, 1e-3 and more near the mode."""
    import synth
    for db, step in ((1.0, 1 / 16), (4.0, 1 / 16), (7.0, 1 / 16), (1.0, 1 / 64)):
        thr, table = synth.awgn_channel(db, 0.875, step)
        s = synth.std_dev(db, 0.875)
        assert s == 1 / math.sqrt(2 * 0.875 * math.pow(10.0, db * 0.1))
        p = synth.channel_probs(thr)
        k = np.arange(-127, 128)
        assert np.array_equal(table[k + 128], 2.0 * (k * step) / (s * s))
        for kk in range(-126, 127):  # inner cells: x = -1 sends y = -1 + n, code kk <-> cell ((kk - .5) step, (kk + .5) step)
            hi = 0.5 * math.erfc(-(((kk + 0.5) * step + 1) / s) / math.sqrt(2.0))
            lo = 0.5 * math.erfc(-(((kk - 0.5) * step + 1) / s) / math.sqrt(2.0))
            assert abs(p[-kk + 127] - (hi - lo)) <= 16 * 2.0 ** -53, (db, step, kk)
        assert abs(int(p[1:254].argmax()) + 1 - (127 + round(1 / step))) <= 1  # the inner cells' mode: y = +1


def test_bsc_and_bec_code_sets(L):
    import synth
    z = np.zeros((40, 288), np.uint8)
    c = synth.channel_codes(z, 0, 40, SEED, synth.bsc_channel(0.02)[0])
    assert set(np.unique(c).tolist()) == {-1, 1}
    c = synth.channel_codes(z, 0, 40, SEED, synth.bec_channel(0.1)[0])
    assert set(np.unique(c).tolist()) == {0, 1}
    ones = np.ones((40, 288), np.uint8)
    c = synth.channel_codes(ones, 0, 40, SEED, synth.bec_channel(0.1)[0])
    assert set(np.unique(c).tolist()) == {0, -1}
    t = synth.bsc_channel(0.02)[1]
    assert t[129] == math.log(0.98 / 0.02) and t[127] == math.log(0.02 / 0.98)


# ---------------------------------------------------------------------------
# the replica's statistics
# ---------------------------------------------------------------------------
def test_replica_statistics(L):
    """B N = 92 160 draws: every code's count within 6 sqrt(n p (1 - p)) + 1 of n p, p from thr itself."""
    import synth
    B, N = 320, 288
    n = B * N
    z = np.zeros((B, N), np.uint8)
    worst = 0.0
    for name, (thr, _) in _tables().items():
        c = synth.channel_codes(z, 0, B, SEED, thr).astype(np.int64)
        cnt = np.bincount(c.ravel() + 127, minlength=255)
        p = synth.channel_probs(thr)
        bound = 6 * np.sqrt(n * p * (1 - p)) + 1
        ratio = np.abs(cnt - n * p) / bound
        print(name, "worst ratio to the bound", ratio.max())
        assert (ratio <= 1).all(), (name, int(ratio.argmax()) - 127)
        worst = max(worst, ratio.max())
        if name == "bsc":
            print("BSC(0.02) flip rate", (c == -1).mean())
        if name == "bec":
            print("BEC(0.1) erasure rate", (c == 0).mean())
        if name == "clip":  # the clip is hit, from the replica alone: +127 on zeros, -127 on ones
            assert cnt[254] > 0 and p[254] > 0.05
            assert synth.channel_codes(z + 1, 0, B, SEED, thr).min() == -127
    assert worst > 0


# ---------------------------------------------------------------------------
# host form against the replica
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N", [13, 130, 96, 288])
def test_channel_codes_host_equals_replica(L, N):
    import synth
    rng = np.random.default_rng(N)
    B = 70
    for name, (thr, _) in cc.channels(0.875).items():
        for b0 in (0, (1 << 33) + 5):
            for cw in (None, rng.integers(0, 2, (B, N)).astype(np.uint8)):
                want = synth.channel_codes(np.zeros((B, N), np.uint8) if cw is None else cw, b0, B, SEED, thr)
                got = L.channel_codes_host(cw, N, b0, B, SEED, thr)
                assert np.array_equal(got, want), (name, b0, cw is None)
                # split ranges give the same rows
                a = L.channel_codes_host(None if cw is None else cw[:23], N, b0, 23, SEED, thr)
                b = L.channel_codes_host(None if cw is None else cw[23:], N, b0 + 23, B - 23, SEED, thr)
                assert np.array_equal(np.concatenate([a, b]), want), (name, b0, "split")
    thr = cc.channels(0.875)["awgn4"][0]
    assert not np.array_equal(L.channel_codes_host(None, N, 0, 4, SEED, thr), L.channel_codes_host(None, N, 0, 4, SEED + 1, thr))


def test_channel_codes_host_argument_errors(L):
    thr = cc.channels(0.875)["awgn4"][0]
    bad = thr.copy()
    bad[10] = bad[11] + np.uint64(1)
    big = thr.copy()
    big[-1] = np.uint64((1 << 53) + 1)
    for kw in (dict(thr=bad), dict(thr=big), dict(N=1 << 24), dict(N=0), dict(b0=-1), dict(b0=(1 << 40) - 1, B=2)):
        a = dict(cw=None, N=8, b0=0, B=0, seed=1, thr=thr)
        a.update(kw)
        with pytest.raises(L.LdpcError) as e:
            L.channel_codes_host(a["cw"], a["N"], a["b0"], a["B"], a["seed"], a["thr"])
        assert e.value.code == L.LDPC_ERR_ARG, kw


# ---------------------------------------------------------------------------
# the error counter's host form
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("N", [13, 96, 130, 288])
def test_frame_errors_host_equals_numpy_count(L, N):
    rng = np.random.default_rng(1000 + N)
    mask = (rng.random(N) < 0.7).astype(np.uint8)
    mask[0], mask[N - 1] = 1, 0
    B = 37
    hard, cw, codes, iters, valid = cc.planted(rng, B, N, mask)
    table = np.arange(-128, 128) * 0.25
    for t in (table, cc.nan_table(table)):
        got = L.frame_errors_host(hard, cw, codes, mask, t, iters=iters, valid=valid)
        want = cc.count(hard, cw, codes, mask, t, iters, valid)
        assert np.array_equal(got, want)
        assert got["bit_err"][0] == 0 and got["info_err"][1] == 0 < got["bit_err"][1] and got["bit_err"][2] == N
    got = L.frame_errors_host(hard, cw, codes, mask, cc.nan_table(table), iters=iters, valid=valid)
    nan_cols = (codes == 3) | (codes == -5)
    assert nan_cols.any()  # a NaN entry reads as 1: an error exactly where the sent bit is 0
    only = L.frame_errors_host(hard, cw, np.where(nan_cols, codes, 1).astype(np.int8), None, cc.nan_table(np.ones(256)))
    assert np.array_equal(only["raw_err"], ((cw == 0) & nan_cols).sum(1) + ((cw == 1) & ~nan_cols).sum(1))
    # no codeword: zeros; no mask: every position; no iters / valid: 0
    got = L.frame_errors_host(hard, None, codes, None, table)
    assert np.array_equal(got, cc.count(hard, None, codes, None, table, None, None))
    assert np.array_equal(got["info_err"], got["bit_err"])


# ---------------------------------------------------------------------------
# the loop
# ---------------------------------------------------------------------------
class Case:
    """One (code, Eb/N0, algo): the graph, its oracle and encoder, the channel,
    and the reference records of frames 0 .. 319, computed once."""

    def __init__(self, L, oracle_mod, tmp, code, db, algo):
        import synth
        path = cc.pchk(tmp, code)
        self.G = L.Graph(path)
        self.og = oracle_mod.OracleGraph(path)
        self.enc = self.G.encoder()
        self.algo = algo
        self.channel = synth.awgn_channel(db, self.enc.K / self.enc.N)
        self.rec = cc.reference_records(self.og, self.enc, self.channel, algo, SEED, 0, cc.FRAMES)
        self.fe = np.flatnonzero(self.rec["bit_err"] > 0)


@pytest.fixture(scope="module")
def case(L, oracle_mod, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("channel_sim")

    @functools.lru_cache(maxsize=None)
    def get(code, db, algo):
        return Case(L, oracle_mod, tmp, code, db, algo)
    return get


MAIN = [("r96", 4.0, "bp"), ("r96", 4.0, "msa"), ("irr", 4.0, "bp"), ("irr", 4.0, "msa")]


@pytest.mark.parametrize("code,db,algo", MAIN)
def test_conditions_hold_from_the_oracle_alone(case, code, db, algo):
    c = case(code, db, algo)
    r = c.rec
    err = r["bit_err"] > 0
    print(code, db, algo, "FER", err.mean(), "undetected", int((err & (r["valid"] != 0)).sum()), "detected",
          int((r["valid"] == 0).sum()), "counts", sorted(set(r["iters"].tolist())))
    assert (~err).any() and (r["valid"] == 0).any() and (err & (r["valid"] != 0)).any()
    counts = set(r["iters"].tolist())
    assert len(counts) > 3 and 0 in counts
    assert (r["info_err"] <= r["bit_err"]).all() and (r["info_err"] < r["bit_err"]).any()
    assert len(c.fe) >= 3 and c.fe[2] % 64 not in (0, 63) and c.fe[2] % 100 not in (0, 99)  # the cut of target 3


def _stops(c):
    """The four stopping cases of (code, 4 dB)."""
    return [dict(frames=cc.FRAMES), dict(target_frame_errors=3, max_frames=cc.FRAMES),
            dict(target_frame_errors=len(c.fe) + 5, max_frames=200)]


def _loop(L, c, batch, **stop):
    return L.ber_run_host(c.G.N, c.enc, cc.oracle_decode(c.og, c.algo), c.channel, cc.MAX_ITER, SEED, batch, **stop)


@pytest.mark.parametrize("code,db,algo", MAIN)
def test_loop_equals_plain_python_loop(L, case, code, db, algo):
    c = case(code, db, algo)
    for stop in _stops(c):
        want = cc.plain_loop(c.rec, cc.MAX_ITER, frames=stop.get("frames"), target=stop.get("target_frame_errors"),
                             max_frames=stop.get("max_frames"))
        if "frames" not in stop:  # the cut lies strictly inside a batch / the target is never reached
            assert want["frames"] == (c.fe[2] + 1 if stop["target_frame_errors"] == 3 else 200)
        for batch in (1, 64, 100):
            cc.same_result(_loop(L, c, batch, **stop), want, (stop, batch))


@pytest.mark.parametrize("algo", ["bp", "msa"])
def test_loop_target_one_met_by_frame_zero(L, case, algo):
    c = case("r96", 2.0, algo)
    assert c.fe[0] == 0  # from the oracle alone
    want = cc.plain_loop(c.rec, cc.MAX_ITER, target=1, max_frames=cc.FRAMES)
    assert want["frames"] == 1 and want["frame_err"] == 1
    for batch in (1, 64, 100):
        cc.same_result(_loop(L, c, batch, target_frame_errors=1, max_frames=cc.FRAMES), want, batch)


def test_loop_zero_codeword(L, case):
    """No encoder: the zero codeword, info_err counts every position."""
    c = case("r96", 4.0, "bp")
    rec = cc.reference_records(c.og, None, c.channel, "bp", SEED, 0, 100)
    want = cc.plain_loop(rec, cc.MAX_ITER, frames=100)
    assert want["info_err"] == want["bit_err"]
    got = L.ber_run_host(c.G.N, None, cc.oracle_decode(c.og, "bp"), c.channel, cc.MAX_ITER, SEED, 64, frames=100)
    cc.same_result(got, want)


def test_loop_argument_errors(L, case):
    c = case("r96", 4.0, "bp")
    dec = cc.oracle_decode(c.og, "bp")
    with pytest.raises(ValueError):
        L.ber_run_host(c.G.N, c.enc, dec, c.channel, 5, SEED, 64)
    with pytest.raises(ValueError):
        L.ber_run_host(c.G.N, c.enc, dec, c.channel, 5, SEED, 64, target_frame_errors=3)
    for kw in (dict(batch=0), dict(max_iter=-1), dict(target_frame_errors=0, max_frames=5)):
        a = dict(batch=64, max_iter=5)
        a.update({k: v for k, v in kw.items() if k in a})
        stop = {k: v for k, v in kw.items() if k not in a} or dict(frames=4)
        with pytest.raises(L.LdpcError) as e:
            L.ber_run_host(c.G.N, c.enc, dec, c.channel, a["max_iter"], SEED, a["batch"], **stop)
        assert e.value.code == L.LDPC_ERR_ARG, kw
    bad = c.channel[0].copy()
    bad[5] = bad[6] + np.uint64(1)
    with pytest.raises(L.LdpcError):
        L.ber_run_host(c.G.N, c.enc, dec, (bad, c.channel[1]), 5, SEED, 64, frames=4)
    # a decoder that fails ends the run with its code
    with pytest.raises(L.LdpcError):
        L.ber_run_host(c.G.N, c.enc, lambda *a: 1 / 0, c.channel, 5, SEED, 64, frames=4)
