"""GPU tests of the strand-index kernels (csrc/dna.hip k_rs_index_decode,
k_strands_write): the device against the host codec word for word and byte
for byte, a raw-read trial against the same trial with the index decoded on
the host, and a write-then-read round trip on a code other than the DNA
code."""
import hashlib
import os

import numpy as np
import pytest

import rs_ref
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

_BASES = np.frombuffer(b"ACGT", np.uint8)


@pytest.fixture(scope="module")
def final_sha():
    return str(np.load(os.path.join(GOLDEN, "index_fixtures.npz"), allow_pickle=False)["final_dna_sha256"])


@pytest.fixture(scope="module")
def prefixes():
    """The 20000 random words and the exhaustive double-error sets of three
    codewords as 16-nt strings, with the host decoder's answer."""
    import dna_llr
    cws = rs_ref.codeword_symbols()
    words = np.concatenate([rs_ref.random_words()] + [rs_ref.double_errors(cws[i]) for i in (0, 65535, 0x1B14)])
    seqs = rs_ref.strings(words)
    index, cnumerr = dna_llr.decode_indices_host(seqs)
    assert len(seqs) == 20000 + 3 * 6300 and (cnumerr[20000:] == 2).all()
    assert 0.05 < (cnumerr[:20000] >= 0).mean() < 0.20
    return seqs, index, cnumerr


def test_device_equals_host_on_batches(gpu, prefixes):
    import dna_llr
    seqs, index, cnumerr = prefixes
    n = len(seqs)
    for B in (1, 63, 64, 65, 255, 256, 257, n):
        a = (7919 * B) % (n - B + 1)  # a different window of the set per size
        gi, gc = dna_llr.decode_indices(seqs[a:a + B])
        assert np.array_equal(gi, index[a:a + B]) and np.array_equal(gc, cnumerr[a:a + B]), B
    gi, gc = dna_llr.decode_indices([])
    assert gi.shape == (0,) and gc.shape == (0,)


def test_device_equals_host_on_ragged_reads(gpu, prefixes):
    """Lengths 0, 15, 16, 17, 152 and 200 interleaved (unaligned offsets);
    the last read is 16 nt and ends exactly at the end of the buffer."""
    import dna_llr
    seqs, _, _ = prefixes
    rng = np.random.default_rng(2)
    tail = "".join(rng.choice(list("ACGT"), 250))
    lens = (0, 15, 16, 17, 152, 200)
    reads = [(s + tail[k % 50:])[:lens[k % 6]] for k, s in enumerate(seqs[:6000:3] + seqs[20000:26300:7])]
    reads += ["ACGTN" * 4, "acgt" * 38, seqs[20001]]
    assert len(reads[-1]) == 16 and {len(r) for r in reads} == set(lens) | {20}
    buf, offs, ln = dna_llr._concat(reads)
    assert offs[-1] + ln[-1] == len(buf) and (offs % 4 != 0).any()
    want_i, want_c = dna_llr.decode_indices_host(reads)
    short = np.array([len(r) < 16 for r in reads])
    assert (want_c[short] == -1).all() and (want_c[~short] >= 0).sum() > 500
    gi, gc = dna_llr.decode_indices(reads)
    assert np.array_equal(gi, want_i) and np.array_equal(gc, want_c)


# partial blocks of 64 strands, one strand, the tail bytes after the dword
# stores (63 * 19, 65 * 19 bytes), and (600, 70): strands longer than the
# 256-byte chunk a block stages (two chunks, the second 60 bytes wide)
@pytest.mark.parametrize("n_cw,N", [(2, 1), (6, 63), (6, 65), (10, 257), (272, 300), (600, 70)])
def test_strand_writer_equals_host(gpu, n_cw, N):
    import synth
    rng = np.random.default_rng(n_cw * 1000 + N)
    cw = rng.integers(0, 2, (n_cw, N), dtype=np.uint8)
    index = rng.integers(0, 1 << 16, N)
    want = synth.dna_strands(cw, index)
    assert want.shape == (N, 16 + n_cw // 2)
    got = synth.dna_strands(cw, index, device=0)
    assert np.array_equal(got, want)


def test_strand_writer_dna_code(gpu, codewords, final_sha):
    import synth
    got = synth.dna_strands(codewords, device=0)
    assert got.shape == (18432, 152)
    assert hashlib.sha256("\n".join(r.tobytes().decode() for r in got).encode()).hexdigest() == final_sha
    assert np.array_equal(got, synth.dna_strands(codewords))


def test_raw_trial_equals_index_given_trial(gpu, codewords):
    """72000 raw reads (substitutions on all 152 positions) through the GPU
    index decode, against the same trial with the index decoded on the host:
    the same reads survive and every field of the result agrees."""
    import dna_llr
    import dna_pipeline
    import synth
    raw = synth.dna_raw_reads(codewords, seed=7, n_reads=72000, sub=0.01)
    res = dna_pipeline.trial_from_raw_reads(raw, codewords, eps=0.02, align_fn=dna_llr.pad_align)
    reads = dna_llr.split_reads(*raw, host=True)
    ref = dna_pipeline.trial_from_reads(reads, codewords, eps=0.02, align_fn=dna_llr.pad_align)
    hist = res["cnumerr_hist"]
    print("cnumerr histogram", hist, "valid reads", res["n_reads_valid"], "first", res["first_success"])
    assert sum(hist.values()) == 72000 and res["n_reads_dropped"] == hist[-1] == 72000 - len(reads[0])
    assert hist[0] > hist[1] > hist[2] > 0 and res["t_index_s"] > 0
    assert np.array_equal(res["hard"], ref["hard"])
    for key in ("first_success", "second_success", "n", "fail_first", "fail_second", "second_iterations",
                "first_errors", "second_errors", "erasure_index", "n_erased_strands", "n_reads_valid"):
        assert res[key] == ref[key], key
    assert np.array_equal(res["llr"].llr.view(np.uint64), ref["llr"].llr.view(np.uint64))
    assert res["first_success"] == 272 and not res["fail_second"]  # the outcome of all ten reference trials


def test_write_then_read_round_trip_rs_7_72_6(gpu):
    """Messages -> Encoder -> strands on the device -> up to two wrong prefix
    symbols per strand -> every index back with the right cnumerr, and the
    payloads map back to the codewords.  The payload length follows n_cw."""
    import dna_llr
    import synth
    R = gpu.Graph.rs_ldpc(7, 72, 6)
    enc = R.encoder()
    n_cw, N = 130, R.N
    cw = enc.encode(synth.random_messages(enc.K, 0, n_cw, seed=11))
    index = np.arange(N)
    strands = synth.dna_strands(cw, index, device=0)
    assert strands.shape == (N, 16 + 65)
    rng = np.random.default_rng(12)
    n_err = np.arange(N) % 3
    rx = strands.copy()
    for j in range(N):
        for p in rng.choice(8, n_err[j], replace=False):
            sym = np.searchsorted(_BASES, rx[j, 2 * p:2 * p + 2])
            v = (4 * sym[0] + sym[1]) ^ int(rng.integers(1, 16))
            rx[j, 2 * p], rx[j, 2 * p + 1] = _BASES[v >> 2], _BASES[v & 3]
    assert ((rx != strands).any(axis=1) == (n_err > 0)).all()
    reads = [r.tobytes().decode() for r in rx]
    gi, gc = dna_llr.decode_indices(reads)
    assert np.array_equal(gi, index) and np.array_equal(gc, n_err)
    sidx, payloads, _ = dna_llr.split_reads(reads, [70] * N)
    assert sidx == index.tolist()
    nt = np.searchsorted(_BASES, np.frombuffer("".join(payloads).encode(), np.uint8).reshape(N, 65))
    back = np.empty((n_cw, N), np.uint8)
    back[0::2] = (nt >> 1).T
    back[1::2] = (nt & 1).T
    assert np.array_equal(back, cw)
    assert np.array_equal(enc.extract(back), synth.random_messages(enc.K, 0, n_cw, seed=11))
