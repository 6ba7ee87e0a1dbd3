"""CPU tests of the systematic encoder (include/ldpc_amd.h "Systematic
encoding", csrc/gf2.hpp): positions, rank and host-encoded codewords against
the independent GF(2) reference of gf2_ref.py, the DNA code against its 272
reference codewords, argument errors, and the message generator."""
import ctypes as C

import numpy as np
import pytest

import gf2_ref


def _messages(K, B, seed):
    return (np.random.default_rng(seed).random((B, K)) < 0.5).astype(np.uint8)


@pytest.mark.parametrize("name", gf2_ref.SMALL_CODES + ["tall"])
def test_small_codes_match_reference(L, name):
    G = gf2_ref.small_graph(L, name)
    ref = gf2_ref.RefEncoder(gf2_ref.dense(G))
    enc = G.encoder()
    assert (enc.N, enc.K, enc.rank) == (G.N, ref.K, ref.rank)
    assert np.array_equal(enc.par_pos, ref.par_pos) and np.array_equal(enc.info_pos, ref.info_pos)
    if name == "rs_5_16_4":
        assert (G.M, G.N) == (128, 512) and enc.rank < G.M  # rank-deficient
    if name == "degenerate":  # the zero column and the earlier of the twin columns carry message bits
        assert 2 in enc.info_pos and 4 in enc.info_pos and 7 in enc.par_pos and enc.rank == 4
    m = _messages(enc.K, 70, 3)
    cw = enc.encode_host(m)
    assert cw.dtype == np.uint8 and cw.shape == (70, G.N)
    assert np.array_equal(cw, ref.encode(m))
    for c in cw:
        assert G.syndrome(c)[0] == 0
    assert np.array_equal(enc.extract(cw), m)
    assert np.array_equal(enc.encode_host(m[5]), cw[5])  # a 1-D array is one message
    assert G.encoder() is enc  # cached


@pytest.fixture(scope="module")
def dna(L):
    from conftest import PCHK
    G = L.Graph(PCHK)
    return G, G.encoder()


def test_dna_code_dimensions_and_uniqueness(dna):
    G, enc = dna
    assert (enc.rank, enc.K, enc.N) == (1860, 16572, 18432)
    assert len(enc.par_pos) == 1860 and len(enc.info_pos) == 16572
    assert np.array_equal(np.sort(np.concatenate([enc.par_pos, enc.info_pos])), np.arange(G.N))
    # H[:, par_pos] has full column rank: the codeword of a message is unique
    assert gf2_ref.rank(gf2_ref.dense(G)[:, enc.par_pos]) == 1860


def test_dna_code_reproduces_the_golden_codewords(dna, codewords):
    G, enc = dna
    assert codewords.shape == (272, 18432)
    assert np.array_equal(enc.encode_host(codewords[:, enc.info_pos]), codewords)


def test_dna_code_random_messages_are_codewords(dna):
    G, enc = dna
    cw = enc.encode_host(_messages(enc.K, 64, 9))
    for c in cw:
        assert G.syndrome(c)[0] == 0


def test_errors(L):
    with pytest.raises(L.LdpcError) as e:  # full column rank: K = 0
        L.Graph.from_edges(3, 3, [0, 1, 2], [0, 1, 2]).encoder()
    assert e.value.code == L.LDPC_ERR_UNSUPPORTED
    G = gf2_ref.small_graph(L, "hamming")
    enc = G.encoder()
    assert (enc.K, enc.rank) == (4, 3)
    bad = np.array([[0, 1, 2, 0]])
    for f in (enc.encode_host, enc.encode):  # checked before any device call
        with pytest.raises(ValueError):
            f(bad)
        with pytest.raises(ValueError):
            f(np.zeros((2, 5), np.uint8))  # wrong width
        with pytest.raises(ValueError):
            f(np.zeros((2, 4)))  # not integers
    # the C entry points check the bytes themselves
    b8 = np.ascontiguousarray(bad, np.uint8)
    out = np.zeros((1, 7), np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert L.lib().ldpc_encode_host(enc._h, p(b8), 1, p(out)) == L.LDPC_ERR_ARG
    assert b"neither 0 nor 1" in L.lib().ldpc_last_error()
    assert L.lib().ldpc_encode(enc._h, p(b8), 1, p(out), 0) == L.LDPC_ERR_ARG
    # B = 0: empty results, no device
    assert enc.encode_host(np.zeros((0, 4), np.uint8)).shape == (0, 7)
    assert enc.encode(np.zeros((0, 4), np.uint8)).shape == (0, 7)
    if L.device_count() == 0:
        with pytest.raises(L.LdpcError) as e:
            enc.encode(np.zeros((1, 4), np.uint8))
        assert e.value.code == L.LDPC_ERR_DEVICE
    # the encoder outlives its graph
    G.close()
    cw = enc.encode_host(np.array([[1, 0, 1, 1]]))
    assert np.array_equal(enc.encode_host(np.array([1, 0, 1, 1], bool)), cw[0])  # bool arrays are taken
    H = np.array([[1, 0, 1, 0, 1, 0, 1], [0, 1, 1, 0, 0, 1, 1], [0, 0, 0, 1, 1, 1, 1]])
    assert not ((H @ cw[0]) & 1).any() and np.array_equal(enc.extract(cw), [[1, 0, 1, 1]])
    enc.close()
    enc.close()


def test_random_messages_do_not_depend_on_batching():
    import synth
    whole = synth.random_messages(100, 5, 200, seed=7)
    assert whole.shape == (200, 100) and whole.dtype == np.uint8 and set(np.unique(whole)) == {0, 1}
    parts = np.concatenate([synth.random_messages(100, 5, 1, 7), synth.random_messages(100, 6, 130, 7),
                            synth.random_messages(100, 136, 69, 7)])
    assert np.array_equal(whole, parts)
    assert np.array_equal(synth.random_messages(40, 5, 200, 7), whole[:, :40])  # keyed by (b, k) alone
    assert not np.array_equal(synth.random_messages(100, 5, 200, seed=8), whole)
    # the documented key: low bit of splitmix64(((b << 24) | k) ^ splitmix64(seed))
    def sm(x):
        x = (x + 0x9E3779B97F4A7C15) & (2**64 - 1)
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & (2**64 - 1)
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & (2**64 - 1)
        return x ^ (x >> 31)
    assert whole[3, 17] == sm(((8 << 24) | 17) ^ sm(7)) & 1


def test_random_codewords_on_the_host(L):
    import synth
    G = gf2_ref.small_graph(L, "rs_4_8_3")
    enc = G.encoder()
    cw = synth.random_codewords(enc, 10, 20, seed=1)
    assert np.array_equal(enc.extract(cw), synth.random_messages(enc.K, 10, 20, 1))
    assert all(G.syndrome(c)[0] == 0 for c in cw)
