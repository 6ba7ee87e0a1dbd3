"""Speculated second decodes on the device (ldpc_trial_set_speculation,
k_trial_absmax / k_trial_gather_spec of csrc/dna_trial_kernels.hpp, DESIGN.md
sec. 8.10): a handle with speculation on gives the result of one with it off
in every field, and the counters the rule predicts."""
import numpy as np
import pytest

import dna_pipeline as P
import synth
from test_dna_trial_gpu import EPS, KEYS, SMALL, SMALL_ITERS

pytestmark = pytest.mark.gpu
COUNTERS = ("second_decodes", "second_rows", "second_rows_used", "code_absmax", "steps_per_decode")


def _same(new, old):
    for key in KEYS:
        assert new[key] == old[key], key
    for key in ("hard", "iters", "valid"):
        assert np.array_equal(new[key], old[key]), key
    assert new["second_rows_used"] == old["second_rows_used"] == old["second_rows"]
    assert old["second_decodes"] == old["second_iterations"]


@pytest.fixture(scope="module")
def small(gpu):
    out = {}
    for name, (make, seed) in SMALL.items():
        G = make(gpu)
        enc = G.encoder()
        cw = enc.encode_host(synth.random_messages(enc.K, 0, 65, seed=3))
        y = cw ^ synth.bsc_flips(0, 65, G.N, seed, 0.01).astype(np.uint8)
        out[name] = (G, cw, np.where(y == 1, -1, 1).astype(np.int8))
    return out


@pytest.mark.parametrize("B", [1, 5, 65])
@pytest.mark.parametrize("name", sorted(SMALL))
def test_small_codes(small, name, B):
    """The uint4 paths of both kernels (N = 512) and their byte paths (N =
    1003): one row, a few, and 65 (a second tile of the engine)."""
    G, cw, codes = small[name]
    off = P.ResidentTrial(G, cw[:B])
    for faithful in ((True, False) if B == 65 else (True,)):
        old = off.run_codes(codes[:B], eps=EPS, max_iter=SMALL_ITERS, faithful=faithful)
        assert 1 in old["fail_first"] and old["second_iterations"] >= 1
        for n in (-1, 2, 3):
            T = P.ResidentTrial(G, cw[:B], speculate=n)
            new = T.run_codes(codes[:B], eps=EPS, max_iter=SMALL_ITERS, faithful=faithful)
            _same(new, old)
            assert (new["code_absmax"], new["steps_per_decode"]) == (1, 85)
            if B == 1:  # row 1 fails in every batch: 37 steps, all in one decode when as many as fit
                assert old["second_iterations"] == 37
                want = {-1: (1, 37), 2: (19, 37), 3: (13, 37)}[n]
                assert (new["second_decodes"], new["second_rows"]) == want
            T.close()
    off.close()


@pytest.mark.parametrize("m,P_want", [(42, 3), (127, 1)])
def test_table_space_edges(small, m, P_want):
    """+-42: three steps fit the table; +-127: one, so nothing is speculated.
    At these magnitudes and 3 iterations (checked on the CPU oracle) all 5 rows
    fail every decode: 37 steps of 5 rows, 12 decodes of 3 steps and one of 1."""
    G, cw, codes = small["irregular"]
    k = (codes[:5].astype(np.int32) * m).astype(np.int8)
    old = P.ResidentTrial(G, cw[:5]).run_codes(k, eps=EPS, max_iter=SMALL_ITERS, faithful=False)
    new = P.ResidentTrial(G, cw[:5], speculate=-1).run_codes(k, eps=EPS, max_iter=SMALL_ITERS, faithful=False)
    _same(new, old)
    assert (new["code_absmax"], new["steps_per_decode"]) == (m, P_want)
    assert old["fail_first"] == [1, 2, 3, 4, 5] and old["second_iterations"] == 37
    assert (new["second_decodes"], new["second_rows"]) == ((13, 185) if P_want == 3 else (37, 185))
    assert new["second_decodes"] == new["second_iterations"] or P_want > 1


def test_min_sum(small):
    G, cw, codes = small["rs"]
    old = P.ResidentTrial(G, cw, algo="msa").run_codes(codes, eps=EPS, max_iter=SMALL_ITERS)
    new = P.ResidentTrial(G, cw, algo="msa", speculate=-1).run_codes(codes, eps=EPS, max_iter=SMALL_ITERS)
    _same(new, old)
    assert old["fail_first"] and new["second_decodes"] < old["second_decodes"]


@pytest.fixture(scope="module")
def dna16(codewords):
    return synth.dna_like_codes(codewords, seed=1, reads=57000)[:16], codewords[:16]


def test_dna_16_codewords(G, dna16):
    """N = 18432: the uint4 paths.  One failing row in a handle of 16
    codewords: a batch of 9 rows, then 4, in buffers regrown to 64 rows."""
    k, cw = dna16
    old = P.ResidentTrial(G, cw).run_codes(k, eps=EPS, max_iter=200)
    new = P.ResidentTrial(G, cw, speculate=-1).run_codes(k, eps=EPS, max_iter=200)
    _same(new, old)
    assert new["fail_first"] == [14] and new["second_iterations"] == 13
    assert (new["code_absmax"], new["second_decodes"], new["second_rows"]) == (13, 2, 18)
    assert P.report(new) == P.report(old)


def test_genie_less(G, dna16):
    k, _ = dna16
    old = P.ResidentTrial(G, None, n_cw=16).run_codes(k, eps=EPS, max_iter=200)
    new = P.ResidentTrial(G, None, n_cw=16, speculate=-1).run_codes(k, eps=EPS, max_iter=200)
    _same(new, old)
    assert old["fail_first"] and new["second_decodes"] < old["second_decodes"]


@pytest.fixture(scope="module")
def dna272(G, codewords):
    return synth.dna_like_codes(codewords, seed=1, reads=57000), P.ResidentTrial(G, codewords)


@pytest.mark.parametrize("faithful,want", [(False, (8, 444)), (True, (5, 95))])
def test_dna_272_codewords(dna272, codewords, faithful, want):
    """Lists of 1 to 30 rows, batches of 2 and 3 steps, rows leaving in the middle of a batch."""
    k, T = dna272
    T.set_speculation(0)
    old = T.run_codes(k, eps=EPS, max_iter=200, faithful=faithful)
    assert len(old["fail_first"]) == 30 and old["second_iterations"] == 37
    T.set_speculation(-1)
    new = T.run_codes(k, eps=EPS, max_iter=200, faithful=faithful)
    _same(new, old)
    assert (new["second_decodes"], new["second_rows"]) == want


def test_on_off_on(small, gpu):
    """One handle on -> off -> on with other inputs against fresh handles; the
    counters before any run; the argument error."""
    G, cw, codes = small["irregular"]
    other = np.where((cw ^ synth.bsc_flips(0, 65, G.N, 9, 0.02).astype(np.uint8)) == 1, -1, 1).astype(np.int8)
    T = P.ResidentTrial(G, cw)
    assert T.counters() == dict.fromkeys(COUNTERS, 0)
    with pytest.raises(gpu.LdpcError) as e:
        T.set_speculation(-2)
    assert e.value.code == gpu.LDPC_ERR_ARG and T.speculate == 0
    runs = [(-1, codes, True), (0, other[:5], False), (3, other, False), (-1, codes[:7], True)]
    for n, k, faithful in runs:
        T.set_speculation(n)
        got = T.run_codes(k, eps=EPS, max_iter=SMALL_ITERS, faithful=faithful)
        fresh = P.ResidentTrial(G, cw, speculate=n).run_codes(k, eps=EPS, max_iter=SMALL_ITERS, faithful=faithful)
        plain = P.ResidentTrial(G, cw).run_codes(k, eps=EPS, max_iter=SMALL_ITERS, faithful=faithful)
        _same(got, plain)
        assert {c: got[c] for c in COUNTERS} == {c: fresh[c] for c in COUNTERS} == T.counters()
    assert np.array_equal(T.codes(7), codes[:7])
