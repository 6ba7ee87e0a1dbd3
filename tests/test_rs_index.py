"""CPU tests of the strand-index codec (include/ldpc_amd.h "strand index
code", csrc/rs_index.hpp): the encoder against the 18432
reference strands, the host decoder against the independent brute-force
reference of rs_ref.py, the raw-read splitter, the trial-file reader and the
C ABI's argument errors."""
import ctypes as C
import hashlib
import os

import numpy as np
import pytest

import rs_ref
from conftest import GOLDEN


@pytest.fixture(scope="module")
def fx():
    z = np.load(os.path.join(GOLDEN, "index_fixtures.npz"), allow_pickle=False)
    d = np.load(os.path.join(GOLDEN, "dna_fixtures.npz"), allow_pickle=False)
    return {"parity": z["strand_parity"], "sha": str(z["final_dna_sha256"]), "index": d["strand_index"].astype(np.int64)}


@pytest.fixture(scope="module")
def llr_mod(L):
    import dna_llr
    return dna_llr


def strand_sha(strands):
    return hashlib.sha256("\n".join(r.tobytes().decode() for r in strands).encode()).hexdigest()


def test_reference_table_is_the_code(fx):
    """The test reference itself: g(x), linearity over GF(2), minimum distance
    5 from the zero codeword, and the 18432 reference strands as codewords."""
    assert rs_ref.generator() == [1, 13, 12, 8, 7]
    cw = rs_ref.codeword_symbols()
    assert cw.shape == (65536, 8)
    w = rs_ref.pack(cw)
    assert np.array_equal(w >> np.uint32(16), np.arange(65536, dtype=np.uint32))  # systematic, index first
    a, b = np.random.default_rng(1).integers(0, 65536, (2, 5000))
    assert np.array_equal(w[a] ^ w[b], w[a ^ b])
    assert ((cw[1:] != 0).sum(axis=1).min()) == 5
    assert np.array_equal(cw[fx["index"]][:, 4:], fx["parity"])


def test_encoder_matches_the_reference_strands(llr_mod, fx, codewords):
    import synth
    assert np.array_equal(fx["index"], llr_mod.strand_indices())
    pre = llr_mod.encode_indices(fx["index"])
    assert pre.shape == (18432, 16) and pre.dtype == np.uint8
    nt = np.searchsorted(np.frombuffer(b"ACGT", np.uint8), pre)
    sym = 4 * nt[:, 0::2] + nt[:, 1::2]
    assert np.array_equal(sym[:, 4:], fx["parity"])
    assert np.array_equal(rs_ref.pack(sym) >> np.uint32(16), fx["index"].astype(np.uint32))
    # every index, against the polynomial-division table
    allpre = llr_mod.encode_indices(np.arange(65536))
    assert [r.tobytes().decode() for r in allpre] == rs_ref.strings(rs_ref.codeword_symbols())
    strands = synth.dna_strands(codewords)  # host path, default indices
    assert strands.shape == (18432, 152)
    assert np.array_equal(strands[:, :16], pre) and np.array_equal(strands[:, 16:], synth.strand_payloads(codewords))
    assert strand_sha(strands) == fx["sha"]
    with pytest.raises(ValueError):
        llr_mod.encode_indices([65536])
    with pytest.raises(ValueError):
        synth.dna_strands(codewords[:3])


@pytest.mark.parametrize("which", [0, 65535, "fixture"])
def test_exhaustive_single_and_double_errors(llr_mod, fx, which):
    idx = int(fx["index"][1234]) if which == "fixture" else which
    cw = rs_ref.codeword_symbols()[idx]
    i0, n0 = llr_mod.decode_indices_host(rs_ref.strings(cw[None, :]))
    assert (i0.tolist(), n0.tolist()) == ([idx], [0])
    one, two = rs_ref.single_errors(cw), rs_ref.double_errors(cw)
    assert len(one) == 120 and len(two) == 6300
    i1, n1 = llr_mod.decode_indices_host(rs_ref.strings(one))
    assert (i1 == idx).all() and (n1 == 1).all()
    i2, n2 = llr_mod.decode_indices_host(rs_ref.strings(two))
    assert (i2 == idx).all() and (n2 == 2).all()


def test_random_words_match_brute_force(llr_mod):
    words = rs_ref.random_words()
    best, dist = rs_ref.brute_decode(words)
    # the pruned search against the distance to all 65536 codewords
    fb, fd = rs_ref.brute_decode_full(words[:600])
    near = fd <= 2
    assert np.array_equal(dist[:600] <= 2, near) and np.array_equal(best[:600][near], fb[near])
    assert np.array_equal(dist[:600][near], fd[near])
    ok = dist <= 2
    share = ok.mean()
    print("decodable share", share)
    assert 0.05 < share < 0.20  # expected 6421 * 65536 / 2^32 = 0.098
    index, cnumerr = llr_mod.decode_indices_host(rs_ref.strings(words))
    assert index.dtype == np.int32 and cnumerr.dtype == np.int32
    assert np.array_equal(index[ok], best[ok]) and np.array_equal(cnumerr[ok], dist[ok])
    assert (cnumerr[~ok] == -1).all() and (index[~ok] == -1).all()


def test_triple_errors_never_return_the_original(llr_mod, fx):
    rng = np.random.default_rng(5)
    n = 20000
    idx = rng.choice(fx["index"], n)
    words = rs_ref.codeword_symbols()[idx].copy()
    for k in range(n):
        pos = rng.choice(8, 3, replace=False)
        words[k, pos] ^= rng.integers(1, 16, 3).astype(np.uint8)
    index, cnumerr = llr_mod.decode_indices_host(rs_ref.strings(words))
    assert not ((cnumerr >= 0) & (index == idx)).any()
    best, dist = rs_ref.brute_decode(words)  # a miscorrection is the other codeword within distance 2
    ok = dist <= 2
    assert np.array_equal(index[ok], best[ok]) and np.array_equal(cnumerr[ok], dist[ok])
    assert (cnumerr[~ok] == -1).all() and (index[~ok] == -1).all()
    assert 0 < ok.sum() < n and (dist[ok] == 2).all()


def test_edge_case_reads(llr_mod, fx):
    idx = int(fx["index"][77])
    good = rs_ref.strings(rs_ref.codeword_symbols()[idx][None, :])[0]
    reads = ["", good[:15], good, good + "ACGT" * 34, good.lower(), "N" + good[1:], good[:15] + "-",
             good[:7] + "n" + good[8:] + "ACGT", good[:3] + "é" + good[4:], good[:3] + "中" + good[4:]]
    index, cnumerr = llr_mod.decode_indices_host(reads)
    assert index.tolist() == [-1, -1, idx, idx, -1, -1, -1, -1, -1, -1]
    assert cnumerr.tolist() == [-1, -1, 0, 0, -1, -1, -1, -1, -1, -1]
    index, cnumerr = llr_mod.decode_indices_host([])
    assert index.shape == (0,) and cnumerr.shape == (0,)


def test_split_reads_host(llr_mod, codewords):
    import synth
    raw, quals = synth.dna_raw_reads(codewords, seed=3, n_reads=400, sub=0.02, ins=0.004, dele=0.004)
    assert len(raw) == len(quals) == 400 and min(len(s) for s in raw) >= 16
    assert len({len(s) for s in raw}) > 1  # insertions and deletions happened
    got = llr_mod.split_reads(raw, quals, host=True)
    best, dist = rs_ref.brute_decode(np.array([rs_ref.symbols_of(s) for s in raw]))
    keep = np.nonzero(dist <= 2)[0]
    want = (best[keep].tolist(), [raw[i][16:] for i in keep], [quals[i] for i in keep])
    assert got == want
    assert 300 < len(keep) < 400 and (dist[keep] > 0).any()  # both outcomes, and corrections, occur
    reads, hist = llr_mod.split_reads_counted(raw, quals, host=True)
    assert reads == want and hist == {-1: 400 - len(keep), 0: int((dist == 0).sum()), 1: int((dist == 1).sum()),
                                      2: int((dist == 2).sum())}
    with pytest.raises(ValueError):
        llr_mod.split_reads(raw, quals[:-1], host=True)


def test_raw_reads_without_channel_errors_are_the_strands(llr_mod, codewords):
    import synth
    raw, quals = synth.dna_raw_reads(codewords, seed=1, n_reads=300, sub=0.0)
    strands = {r.tobytes().decode() for r in synth.dna_strands(codewords)}
    assert all(s in strands for s in raw)
    index, payloads, q = llr_mod.split_reads(raw, quals, host=True)
    assert len(index) == 300 and q == quals and np.isin(index, llr_mod.strand_indices()).all()
    assert payloads == [s[16:] for s in raw]


def test_read_trial_files(L, tmp_path):
    import dna_pipeline
    seqs = ["ACGT" * 38, "", "ACGTN", "TTTT" * 38 + "A"]
    quals = "C5F,"
    (tmp_path / "72000_RS_3.txt").write_text("\n".join(seqs))  # the last line has no '\n'
    (tmp_path / "72000_RS_Q_3.txt").write_text("\n".join(quals) + "\n")
    got = dna_pipeline.read_trial_files(str(tmp_path), 72000, 3)
    assert got == (seqs, [ord(c) for c in quals])
    (tmp_path / "500_RS_0.txt").write_text("ACGT\nAC\n")
    (tmp_path / "500_RS_Q_0.txt").write_text("C\n")
    with pytest.raises(ValueError):
        dna_pipeline.read_trial_files(str(tmp_path), 500, 0)
    with pytest.raises(FileNotFoundError):
        dna_pipeline.read_trial_files(str(tmp_path), 72000, 4)


def test_c_abi_error_cases(L, llr_mod):
    mod, lib = llr_mod._lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    ARG, OK = L.LDPC_ERR_ARG, L.LDPC_OK
    dev_rc = OK if L.device_count() >= 1 else L.LDPC_ERR_DEVICE

    # ldpc_dna_index_encode
    idx = np.array([0, 65535, 65536], np.int32)
    out = np.zeros((3, 16), np.uint8)
    assert lib.ldpc_dna_index_encode(p(idx), 3, p(out)) == ARG
    assert b"outside 0..65535" in lib.ldpc_last_error()
    assert lib.ldpc_dna_index_encode(p(np.array([-1], np.int32)), 1, p(out)) == ARG
    assert lib.ldpc_dna_index_encode(p(idx), 2, p(out)) == OK
    assert lib.ldpc_dna_index_encode(None, 2, p(out)) == ARG
    assert lib.ldpc_dna_index_encode(p(idx), 2, None) == ARG
    assert lib.ldpc_dna_index_encode(p(idx), -1, p(out)) == ARG
    assert lib.ldpc_dna_index_encode(None, 0, None) == OK

    # the index decoders
    seq = np.frombuffer(b"ACGTACGTACGTACGTAC", np.uint8).copy()
    off, ln = np.array([0, 2], np.int64), np.array([16, 16], np.int32)
    oi, oc = np.zeros(2, np.int32), np.zeros(2, np.int32)
    host = lambda *a: lib.ldpc_dna_index_decode_host(*a)  # noqa: E731
    dev = lambda *a: lib.ldpc_dna_index_decode(*a, 0)  # noqa: E731
    for fn in (host, dev):
        assert fn(None, None, None, 0, None, None) == OK  # n = 0 does nothing
        assert fn(p(seq), p(off), p(ln), -1, p(oi), p(oc)) == ARG
        assert fn(None, p(off), p(ln), 2, p(oi), p(oc)) == ARG
        assert b"null sequences" in lib.ldpc_last_error()
        assert fn(p(seq), None, p(ln), 2, p(oi), p(oc)) == ARG
        assert fn(p(seq), p(off), None, 2, p(oi), p(oc)) == ARG
        assert fn(p(seq), p(off), p(ln), 2, None, p(oc)) == ARG
        assert fn(p(seq), p(off), p(ln), 2, p(oi), None) == ARG
        assert fn(p(seq), p(off), p(np.array([16, -1], np.int32)), 2, p(oi), p(oc)) == ARG
        assert fn(p(seq), p(np.array([0, -2], np.int64)), p(ln), 2, p(oi), p(oc)) == ARG
    assert host(p(seq), p(off), p(ln), 2, p(oi), p(oc)) == OK
    assert dev(p(seq), p(off), p(ln), 2, p(oi), p(oc)) == dev_rc
    assert lib.ldpc_dna_index_decode(p(seq), p(off), p(ln), 2, p(oi), p(oc), 1 << 20) == L.LDPC_ERR_DEVICE
    # all-empty reads need no sequence buffer
    assert host(None, p(off), p(np.zeros(2, np.int32)), 2, p(oi), p(oc)) == OK
    assert oi.tolist() == [-1, -1] and oc.tolist() == [-1, -1]

    # the strand writers
    cw = np.zeros((4, 5), np.uint8)
    sidx = np.arange(5, dtype=np.int32)
    sout = np.zeros((5, 18), np.uint8)
    hosts = lambda *a: lib.ldpc_dna_strands_host(*a)  # noqa: E731
    devs = lambda *a: lib.ldpc_dna_strands(*a, 0)  # noqa: E731
    for fn in (hosts, devs):
        assert fn(p(cw), 3, 5, p(sidx), p(sout)) == ARG  # odd n_cw
        assert b"even" in lib.ldpc_last_error()
        assert fn(p(cw), 0, 5, p(sidx), p(sout)) == ARG
        assert fn(p(cw), -2, 5, p(sidx), p(sout)) == ARG
        assert fn(p(cw), 4, -1, p(sidx), p(sout)) == ARG
        assert fn(None, 4, 5, p(sidx), p(sout)) == ARG
        assert fn(p(cw), 4, 5, None, p(sout)) == ARG
        assert fn(p(cw), 4, 5, p(sidx), None) == ARG
        assert fn(p(cw), 4, 5, p(np.array([0, 1, 2, 3, 65536], np.int32)), p(sout)) == ARG
        assert fn(p(cw), 4, 5, p(np.array([0, 1, -1, 3, 4], np.int32)), p(sout)) == ARG
        assert fn(None, 4, 0, None, None) == OK  # N = 0 does nothing
    assert hosts(p(cw), 4, 5, p(sidx), p(sout)) == OK
    assert sout[:, 16:].tobytes() == b"AA" * 5
    assert devs(p(cw), 4, 5, p(sidx), p(sout)) == dev_rc
    assert lib.ldpc_dna_strands(p(cw), 4, 5, p(sidx), p(sout), -1) == L.LDPC_ERR_DEVICE
    # the Python wrappers turn a code into LdpcError
    if L.device_count() < 1:
        with pytest.raises(L.LdpcError) as e:
            llr_mod.decode_indices(["ACGT" * 4])
        assert e.value.code == L.LDPC_ERR_DEVICE
