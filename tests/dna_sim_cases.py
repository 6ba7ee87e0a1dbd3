"""Shared cases of the sequencing-channel tests (test_dna_sim.py on the host
form, test_dna_sim_gpu.py on k_sim_reads): shapes, read counts and rates, the
replica computed once per (shape, rates, range) and the byte comparison."""
import functools

import numpy as np

import synth

# (S, L): L below one wave; L + 1 slots = 25; exactly one chunk of bases and a second chunk that holds slot L
# alone; two chunks with a ragged tail; three chunks (the DNA strand); the longest strand, seven chunks
SHAPES = [(5, 1), (7, 24), (64, 64), (100, 86), (33, 152), (3, 399)]
# reads: one; around one wave of reads and around the kernel's 4-read blocks; many blocks
COUNTS = [1, 63, 64, 65, 1000]
# (sub, ins, del): the read is the strand; substitutions only; all three; every base differs; every slot inserts
# (length 2L + 1, every chunk boundary inside the read); every base deleted (length 0)
RATES = [(0.0, 0.0, 0.0), (0.01, 0.0, 0.0), (0.05, 0.05, 0.05), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)]
R0_BIG = 2 ** 33 + 5
SEED = 20260


@functools.lru_cache(maxsize=None)
def strands(S, L):
    s = np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(1000 * S + L).integers(0, 4, (S, L))]
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def replica(S, L, rates, r0, n=max(COUNTS), seed=SEED):
    """dna_raw_reads_hashed once per case: ((buf, offsets, lengths), quals, strand_of), read-only."""
    out = synth.dna_raw_reads_hashed(strands(S, L), seed, n, *rates, r0=r0, with_strands=True)
    for a in (*out[0], out[1], out[2]):
        a.setflags(write=False)
    return out


def assert_same_reads(got, want, n=None):
    """Lengths, quals, strand ids and every byte [0, length) of the first n reads."""
    (gb, go, gl), gq, gs = got
    (wb, wo, wl), wq, ws = want
    n = len(gl) if n is None else n
    assert len(gl) == n and len(wl) >= n
    stride = len(gb) // max(len(gl), 1)
    assert np.array_equal(go, wo[:n]) and (n == 0 or stride == len(wb) // len(wl))
    assert np.array_equal(gl, wl[:n]), "lengths"
    assert np.array_equal(gq, wq[:n]), "quals"
    assert np.array_equal(gs, ws[:n]), "strand ids"
    live = np.arange(stride)[None, :] < gl[:, None]
    assert np.array_equal(gb.reshape(n, stride)[live], wb[:n * stride].reshape(n, stride)[live]), "read bytes"


def check_form(native, S, L, counts=COUNTS, rates=RATES):
    """native(strands, seed, n, sub, ins, dele, r0=..., with_strands=True) against
    the replica on every count and rate, on a far range, and on a split range."""
    s = strands(S, L)
    for rt in rates:
        for n in counts:
            assert_same_reads(native(s, SEED, n, *rt, r0=0, with_strands=True), replica(S, L, rt, 0), n)
    rt = RATES[2]
    want = replica(S, L, rt, R0_BIG, 65)
    whole = native(s, SEED, 65, *rt, r0=R0_BIG, with_strands=True)
    assert_same_reads(whole, want)
    a = native(s, SEED, 23, *rt, r0=R0_BIG, with_strands=True)
    b = native(s, SEED, 42, *rt, r0=R0_BIG + 23, with_strands=True)
    stride = synth.sim_stride(L)
    joined = ((np.concatenate([a[0][0], b[0][0]]), np.arange(65, dtype=np.int64) * stride,
               np.concatenate([a[0][2], b[0][2]])), np.concatenate([a[1], b[1]]), np.concatenate([a[2], b[2]]))
    assert_same_reads(joined, want)
