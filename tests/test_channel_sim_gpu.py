"""GPU tests of the error-rate simulation: the three
kernels against the numpy replica and the host forms, ErrorRate.run_range
against replica channel -> CPU oracle -> numpy count, and ErrorRate.run against
the plain Python loop of tests/channel_cases.py.  Small codes only; every
comparison is exact.

The conditions that keep the run / run_range comparisons from passing
vacuously (errors, detected and undetected failures, a spread of iteration
counts including 0) are asserted from the oracle alone in
tests/test_channel_sim.py on the same cases."""
import functools

import numpy as np
import pytest

import channel_cases as cc

pytestmark = pytest.mark.gpu
SEED = 11
FAR = (1 << 33) + 5


class Code:
    def __init__(self, L, oracle_mod, tmp, name):
        self.name = name
        path = cc.pchk(tmp, name)
        self.G = L.Graph(path)
        self.og = oracle_mod.OracleGraph(path)
        self.enc = self.G.encoder()
        self.N, self.rate = self.G.N, self.enc.K / self.G.N
        self.mask = np.zeros(self.N, np.uint8)
        self.mask[self.enc.info_pos] = 1


@pytest.fixture(scope="module")
def code(gpu, oracle_mod, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("channel_sim_gpu")

    @functools.lru_cache(maxsize=None)
    def get(name):
        return Code(gpu, oracle_mod, tmp, name)
    return get


@pytest.fixture(scope="module")
def handle(gpu, code):
    """ErrorRate handles, one per (code, algo, batch, pool_tiles, zero_codeword)."""
    made = {}

    def get(name, algo="bp", batch=320, pool_tiles=None, zero=False):
        key = (name, algo, batch, pool_tiles, zero)
        if key not in made:
            c = code(name)
            made[key] = gpu.ErrorRate(c.G, algo=algo, batch=batch, zero_codeword=zero, encoder=None if zero else c.enc,
                                      pool_tiles=pool_tiles)
        return made[key]
    yield get
    for h in made.values():
        h.close()


# ---------------------------------------------------------------------------
# k_sim_messages + the encoder, k_channel_codes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", cc.CODES)
def test_channel_kernel_equals_replica(gpu, code, handle, name):
    import synth
    c = code(name)
    er = handle(name)
    for b0 in (0, FAR):
        cw_all = synth.random_codewords(c.enc, b0, 320, SEED)
        for chan_name, ch in cc.channels(0.875).items():
            want_all = synth.channel_codes(cw_all, b0, 320, SEED, ch[0])
            for B in (1, 63, 64, 65, 320):
                er.run_range(ch, 0, SEED, b0, B)
                cw, codes, _ = er.read(B)
                assert np.array_equal(cw, cw_all[:B]), (name, chan_name, b0, B, "k_sim_messages + encode_device")
                assert np.array_equal(codes, want_all[:B]), (name, chan_name, b0, B, "k_channel_codes")
    assert len(np.unique(want_all)) > 50 and want_all.max() == 127  # the clipping table came last


@pytest.mark.parametrize("name", ["r96", "irr"])
def test_channel_kernel_range_splits(gpu, code, handle, name):
    """A range through batches of 64 gives the rows of one batch of 320; the
    handle's buffers then hold the last, ragged batch."""
    import synth
    c = code(name)
    ch = cc.channels(0.875)["awgn4"]
    whole = handle(name).run_range(ch, 3, SEED, 7, 150)
    split = handle(name, batch=64).run_range(ch, 3, SEED, 7, 150)
    assert np.array_equal(whole, split)
    cw, codes, _ = handle(name, batch=64).read(22)
    want_cw = synth.random_codewords(c.enc, 7 + 128, 22, SEED)
    assert np.array_equal(cw, want_cw)
    assert np.array_equal(codes, synth.channel_codes(want_cw, 7 + 128, 22, SEED, ch[0]))


def test_zero_codeword_skips_messages_and_encoder(gpu, code, handle):
    import synth
    ch = cc.channels(0.875)["awgn4"]
    er = handle("r96", zero=True)
    er.run_range(ch, 0, SEED, 5, 100)
    cw, codes, _ = er.read(100)
    assert not cw.any()
    assert np.array_equal(codes, synth.channel_codes(cw, 5, 100, SEED, ch[0]))


# ---------------------------------------------------------------------------
# k_frame_errors: one wave per frame up to N = 2048, one block per frame above
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,N", [("n13", 13), ("r96", 96), ("irr", 130), ("r288", 288), ("q64", 4608),
                                    ("n2048", 2048), ("n2049", 2049)])
def test_frame_errors_kernel_equals_host_form(gpu, code, handle, name, N):
    """N = 2048 is the last wave-per-frame size; 2049 the smallest block-per-
    frame one, and not a multiple of 8 (q64's 4608 is)."""
    c = code(name)
    assert c.N == N
    rng = np.random.default_rng(2000 + N)
    B = 70
    er = handle(name, batch=B)
    hard, cw, codes, iters, valid = cc.planted(rng, B, N, c.mask)
    table = np.arange(-128, 128) * 0.25
    for t in (table, cc.nan_table(table)):
        for b in (B, 1, 5):
            got = er.frame_errors(hard[:b], cw[:b], codes[:b], t, iters=iters[:b], valid=valid[:b])
            want = gpu.frame_errors_host(hard[:b], cw[:b], codes[:b], c.mask, t, iters=iters[:b], valid=valid[:b])
            assert np.array_equal(got, want), (name, b)
    assert want["bit_err"][0] == 0 and want["info_err"][1] == 0 < want["bit_err"][1] and want["bit_err"][2] == N
    got = er.frame_errors(hard, None, codes, table)
    assert np.array_equal(got, gpu.frame_errors_host(hard, None, codes, c.mask, table))


# ---------------------------------------------------------------------------
# ErrorRate.run_range against replica -> oracle -> numpy count
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _channel(rate, db=4.0):
    import synth
    return synth.awgn_channel(db, rate)


@pytest.mark.parametrize("algo", ["bp", "msa"])
@pytest.mark.parametrize("name", ["r288", "r96", "irr"])
def test_run_range_equals_oracle(gpu, code, handle, name, algo):
    c = code(name)
    ch = _channel(c.rate)
    for zero in (False, True):
        for max_iter in (0, 1, cc.MAX_ITER):
            want = cc.reference_records(c.og, None if zero else c.enc, ch, algo, SEED, 0, cc.FRAMES, max_iter)
            if max_iter == cc.MAX_ITER:
                assert (want["bit_err"] > 0).any() and (want["bit_err"] == 0).any() and len(set(want["iters"])) > 3
            for pool in (1, 3):  # pools of 64 and 192 lanes: refills happen inside the batch of 320
                got = handle(name, algo, pool_tiles=pool, zero=zero).run_range(ch, max_iter, SEED, 0, cc.FRAMES)
                assert np.array_equal(got, want), (name, algo, zero, max_iter, pool)


def test_run_range_far_frames(gpu, code, handle):
    c = code("r96")
    ch = _channel(c.rate)
    want = cc.reference_records(c.og, c.enc, ch, "bp", SEED, FAR, 100)
    assert np.array_equal(handle("r96", pool_tiles=1).run_range(ch, cc.MAX_ITER, SEED, FAR, 100), want)


def test_run_range_batch_above_1024_takes_the_engines_own_pool(gpu, code, handle):
    """ldpc_ber_create sizes the lane pool for `batch` codewords only up to
    1024; above that the engine chooses its own: 1100 frames in one batch."""
    c = code("r96")
    ch = _channel(c.rate)
    want = cc.reference_records(c.og, c.enc, ch, "bp", SEED, 0, 1100)
    assert (want["bit_err"] > 0).any() and (want["bit_err"] == 0).any() and len(set(want["iters"])) > 3
    assert np.array_equal(handle("r96", batch=1100).run_range(ch, cc.MAX_ITER, SEED, 0, 1100), want)


def test_run_range_quantised_min_sum(gpu, code, handle):
    c = code("r96")
    ch = _channel(c.rate)
    q = (6, 0.5, 0)
    want = cc.reference_records(c.og, c.enc, ch, "qmsa", SEED, 0, cc.FRAMES, 10, qparams=q)
    assert (want["bit_err"] > 0).any() and (want["bit_err"] == 0).any()
    er = handle("r96", "qmsa", pool_tiles=1)
    er.set_params(*q, tie_seed=0)
    assert np.array_equal(er.run_range(ch, 10, SEED, 0, cc.FRAMES), want)


# ---------------------------------------------------------------------------
# ErrorRate.run: the stop rule
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,algo", [("r96", "bp"), ("r96", "msa"), ("irr", "bp")])
def test_run_equals_cpu_loop(gpu, code, handle, name, algo):
    c = code(name)
    ch = _channel(c.rate)
    rec = cc.reference_records(c.og, c.enc, ch, algo, SEED, 0, cc.FRAMES)
    fe = np.flatnonzero(rec["bit_err"] > 0)
    stops = [dict(frames=cc.FRAMES), dict(target_frame_errors=3, max_frames=cc.FRAMES),
             dict(target_frame_errors=len(fe) + 5, max_frames=200)]
    for stop in stops:
        want = cc.plain_loop(rec, cc.MAX_ITER, frames=stop.get("frames"), target=stop.get("target_frame_errors"),
                             max_frames=stop.get("max_frames"))
        for batch in (64, 100, 320):
            er = handle(name, algo, batch=batch)
            got = er.run(ch, cc.MAX_ITER, SEED, **stop)
            cc.same_result(got, want, (stop, batch))
            cc.same_result(er.run(ch, cc.MAX_ITER, SEED, **stop), got, "twice on one handle")
    assert want["frames"] == 200 and cc.plain_loop(rec, cc.MAX_ITER, target=3, max_frames=cc.FRAMES)["frames"] == fe[2] + 1


def test_run_target_one_met_by_frame_zero(gpu, code, handle):
    c = code("r96")
    ch = _channel(c.rate, 2.0)
    rec = cc.reference_records(c.og, c.enc, ch, "bp", SEED, 0, 64)
    assert rec["bit_err"][0] > 0
    want = cc.plain_loop(rec, cc.MAX_ITER, target=1, max_frames=cc.FRAMES)
    assert want["frames"] == 1
    for batch in (64, 100, 320):
        cc.same_result(handle("r96", batch=batch).run(ch, cc.MAX_ITER, SEED, target_frame_errors=1, max_frames=cc.FRAMES),
                       want, batch)


def test_ber_curve_and_argument_errors(gpu, code):
    c = code("r96")
    pts = gpu.ber_curve(c.G, [2.0, 6.0], max_iter=10, seed=SEED, frames=128, batch=64, encoder=c.enc)
    assert [p["ebno_db"] for p in pts] == [2.0, 6.0] and all(p["frames"] == 128 for p in pts)
    assert pts[0]["fer"] > pts[1]["fer"] and pts[0]["raw_bit_err"] > pts[1]["raw_bit_err"] > 0
    er = gpu.ErrorRate(c.G, batch=64, encoder=c.enc)
    ch = _channel(c.rate)
    bad = ch[0].copy()
    bad[9] = bad[10] + np.uint64(1)
    with pytest.raises(gpu.LdpcError):
        er.run_range((bad, ch[1]), 5, SEED, 0, 10)
    with pytest.raises(gpu.LdpcError):
        er.run_range(ch, 5, SEED, (1 << 40) - 5, 10)
    with pytest.raises(ValueError):
        er.run(ch, 5, SEED)
    with pytest.raises(gpu.LdpcError):
        gpu.ErrorRate(c.G, batch=0, encoder=c.enc)
    before = er.stats()["other"]["launches"]
    er.run_range(ch, 5, SEED, 0, 10)
    assert er.stats()["other"]["launches"] >= before + 3  # the three kernels are launches of class "other"
    er.close()
