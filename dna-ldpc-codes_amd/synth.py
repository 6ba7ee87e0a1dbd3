"""Input generators for the decode path (host side, numpy).

* ``dna_like_llrs`` -- SURVEY 8(d) config 2.  The reference's decoder input
  reads (72000_RS_*.txt) are missing blobs (.MISSING_LARGE_BLOBS:6-15), so the
  272-codeword DNA batch is rebuilt from the 272 true codewords with a seeded
  read simulator: strand j carries bit i of codeword i+1 (original
  files/final_DNA.txt payload, A/C/G/T = 00/01/10/11, def_func.DNA2binary
  def_func.py:97-117); per strand Poisson(72000/18432) reads, each nucleotide
  substituted with probability `sub` by a uniformly chosen other base; per-bit
  LLR = (count0 - count1) * ln((1-eps)/eps) exactly as decoder.py:314 computes
  it, and LLR 0 for strands without reads (decoder.py:514-517).
* ``bsc_llrs`` -- host replica of the device BSC generator
  (kernels.hpp k_gen_bsc) used for configs 3-5; tests check the device output
  against it bit for bit.
* ``load_codewords`` -- the 272 true codewords (bit-packed fixture).
* ``dna_raw_reads_hashed`` -- numpy replica of the library's counter-hashed
  sequencing channel (csrc/dna_sim.hpp, k_sim_reads); ``dna_raw_reads_native``
  is the library's host / device form, tests hold the three equal byte for byte.
"""
from __future__ import annotations

import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
PCHK = os.path.join(GOLDEN, "decode_n18432_m2048_final.pchk")
CODEWORDS = os.path.join(GOLDEN, "codewords_272.npz")

EPSILON = 0.02
LLR_UNIT = math.log((1 - EPSILON) / EPSILON)  # 3.8918202981106265 = ln 49 (decoder.py:314)


def load_codewords() -> np.ndarray:
    """[272][18432] uint8 -- codeword_n18432_m1860_{1..272}.txt."""
    z = np.load(CODEWORDS, allow_pickle=False)
    return np.unpackbits(z["bits"], axis=1, count=int(z["n"]))[: int(z["count"])].astype(np.uint8)


def dna_like_llrs(codewords: np.ndarray, seed: int = 0, reads: int = 72000, sub: float = 0.01,
                  eps: float = EPSILON) -> np.ndarray:
    """LLRs [n_cw][N] for the DNA batch (see module doc)."""
    k = dna_like_counts(codewords, seed=seed, reads=reads, sub=sub)
    unit = math.log((1 - eps) / eps)
    llr = k.astype(np.float64) * unit  # int * double, as (count_0-count_1)*math.log(...)
    return np.ascontiguousarray(llr)


def dna_like_codes(codewords: np.ndarray, seed: int = 0, reads: int = 72000, sub: float = 0.01) -> np.ndarray:
    """The count differences of dna_like_llrs as int8 codes (dna_like_llrs ==
    codes * ln((1-eps)/eps)); ValueError if one does not fit."""
    k = dna_like_counts(codewords, seed=seed, reads=reads, sub=sub)
    if k.size and np.abs(k).max() > 127:
        raise ValueError("a count difference exceeds the int8 code range")
    return np.ascontiguousarray(k.astype(np.int8))


def dna_like_counts(codewords: np.ndarray, seed: int = 0, reads: int = 72000, sub: float = 0.01) -> np.ndarray:
    """Count differences count_0 - count_1 [n_cw][N] (int64) of the DNA batch."""
    n_cw, N = codewords.shape
    if n_cw % 2:
        raise ValueError("codewords come in nucleotide pairs (bits 2k, 2k+1 of a strand)")
    rng = np.random.default_rng(seed)
    # strand j: nucleotides k = 0..n_cw/2-1, base = 2*bit(2k) + bit(2k+1)
    bits = codewords.T.astype(np.int64)  # [N][n_cw]
    base = 2 * bits[:, 0::2] + bits[:, 1::2]  # [N][n_nt]
    nreads = rng.poisson(reads / N, size=N)
    strand = np.repeat(np.arange(N), nreads)  # read -> strand
    rb = base[strand]  # [R][n_nt]
    mut = rng.random(rb.shape) < sub
    rb = np.where(mut, (rb + rng.integers(1, 4, size=rb.shape)) % 4, rb)
    rbits = np.empty((rb.shape[0], n_cw), np.int64)
    rbits[:, 0::2] = rb >> 1
    rbits[:, 1::2] = rb & 1
    ones = np.zeros((N, n_cw), np.int64)
    np.add.at(ones, strand, rbits)
    zeros = nreads[:, None] - ones
    return np.ascontiguousarray((zeros - ones).T)  # [n_cw][N] count difference


# --- counter-based BSC generator (bit-identical to kernels.hpp k_gen_bsc) ---
_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _splitmix64(x: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        x = (x + np.uint64(0x9E3779B97F4A7C15)) & _M64
        x = ((x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & _M64
        x = ((x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & _M64
        return x ^ (x >> np.uint64(31))


def bsc_flips(b0: int, B: int, N: int, seed: int, p: float) -> np.ndarray:
    seedmix = _splitmix64(np.array([seed], np.uint64))[0]
    b = np.arange(b0, b0 + B, dtype=np.uint64)[:, None]
    j = np.arange(N, dtype=np.uint64)[None, :]
    u = _splitmix64(((b << np.uint64(24)) | j) ^ seedmix) >> np.uint64(11)
    return (u.astype(np.float64) * 2.0 ** -53) < p


def bsc_llrs(codewords: np.ndarray, b0: int, B: int, seed: int, p: float, mag: float = LLR_UNIT,
             as_lr: bool = False) -> np.ndarray:
    """[B][N] fp64: +-mag (or the host-exp'd LR) for codewords b0..b0+B-1 sent
    over a BSC(p); transmitted word = codewords[b mod n_cw]."""
    n_cw, N = codewords.shape
    idx = (np.arange(b0, b0 + B) % n_cw)
    y = codewords[idx] ^ bsc_flips(b0, B, N, seed, p).astype(np.uint8)
    if as_lr:
        return np.where(y == 1, math.exp(-mag), math.exp(mag))
    return np.where(y == 1, -mag, mag)


# --- random messages and fresh codewords (any code with an encoder) ---------
def random_messages(K: int, b0: int, B: int, seed: int) -> np.ndarray:
    """[B][K] uint8: bit k of message b (b0 <= b < b0 + B) is the low bit of
    splitmix64(((b << 24) | k) ^ splitmix64(seed)) -- the BSC generator's
    keying, so a range gives the same messages however it is split."""
    if not 0 <= K < (1 << 24):
        raise ValueError("K must be below 2^24 (the key holds k in 24 bits)")
    seedmix = _splitmix64(np.array([seed], np.uint64))[0]
    b = np.arange(b0, b0 + B, dtype=np.uint64)[:, None]
    k = np.arange(K, dtype=np.uint64)[None, :]
    return np.ascontiguousarray((_splitmix64(((b << np.uint64(24)) | k) ^ seedmix) & np.uint64(1)).astype(np.uint8))


def random_codewords(enc, b0: int, B: int, seed: int, device=None) -> np.ndarray:
    """[B][N] uint8: the codewords of random_messages(enc.K, b0, B, seed),
    encoded on GPU `device`, or on the host when device is None."""
    m = random_messages(enc.K, b0, B, seed)
    return enc.encode_host(m) if device is None else enc.encode(m, device=device)


# --- the transmission channel of the error-rate simulation --
# A symmetric memoryless channel with at most 255 outputs, as data: thr[254]
# uint64 thresholds (non-decreasing, <= 2^53) and the 256-entry code table of
# decode_codes.  csrc/channel_sim.hpp is the definition; channel_codes below is
# its numpy replica, integer compares only.
CHANNEL_STREAM = 0x4348414E4E454C31  # "CHANNEL1": keeps the channel's draws apart from the messages'
CHANNEL_THR = 254


def std_dev(ebno_db: float, rate: float) -> float:
    """getStd_dev (channel.cpp:9-16), in its operation order."""
    enl = math.pow(10.0, ebno_db * 0.1)
    return 1 / math.sqrt(2 * rate * enl)


def _phi(x: float) -> float:
    return 0.5 * math.erfc(-x / math.sqrt(2.0))


def _thr(p) -> np.ndarray:
    """Cumulative probabilities -> thresholds: floor(2^53 p), made monotone, capped at 2^53."""
    t = [min(SIM_ONE, max(0, int(math.floor(SIM_ONE * float(v))))) for v in p]
    return np.maximum.accumulate(np.array(t, np.uint64))


def awgn_channel(ebno_db: float, rate: float, step: float = 1 / 16):
    """(thr, llr_table): BPSK over AWGN at Eb/N0 `ebno_db` for a code of rate
    `rate`, y = +-1 + n quantised to k = clamp(round(y / step), +-127).
    thr[i] = floor(2^53 Phi(((i - 126.5) step - 1) / sigma)), table[k + 128] =
    2 k step / sigma^2 (channel.cpp:32)."""
    s = std_dev(ebno_db, rate)
    thr = _thr(_phi(((i - 126.5) * step - 1) / s) for i in range(CHANNEL_THR))
    k = np.arange(-128, 128, dtype=np.float64)
    return thr, np.ascontiguousarray(2.0 * (k * step) / (s * s))


def bsc_channel(p: float):
    """(thr, llr_table): codes +-1, a flip with probability p, LLR
    +-ln((1 - p) / p) (channel.cpp:71-84)."""
    thr = _thr([0.0] * 126 + [p, p] + [1.0] * 126)
    table = np.zeros(256)
    table[129], table[127] = math.log((1 - p) / p), math.log(p / (1 - p))
    return thr, table


def bec_channel(eps: float, mag: float = 30.0):
    """(thr, llr_table): code 0 (LLR 0) with probability eps, else +-1 with LLR +-mag."""
    thr = _thr([0.0] * 127 + [eps] + [1.0] * 126)
    table = np.zeros(256)
    table[129], table[127] = mag, -mag
    return thr, table


def channel_probs(thr: np.ndarray) -> np.ndarray:
    """p[k + 127], k = -127 .. 127: the probability of code k on a transmitted 0, read from thr itself."""
    t = np.concatenate([[0], np.asarray(thr, np.uint64).astype(np.float64), [float(SIM_ONE)]])
    return np.diff(t) / float(SIM_ONE)


def channel_codes(cw: np.ndarray, b0: int, B: int, seed: int, thr: np.ndarray) -> np.ndarray:
    """[B][N] int8: the codes of frames b0 .. b0 + B - 1 whose transmitted
    words are cw [B][N] (csrc/channel_sim.hpp):
    u = splitmix64(((b << 24) | j) ^ splitmix64(seed ^ CHANNEL_STREAM)) >> 11,
    k0 = -127 + #{i : u >= thr[i]}, code = -k0 where the bit is 1, else k0."""
    cw = np.asarray(cw)
    thr = np.asarray(thr, np.uint64)
    if cw.shape[0] != B or thr.shape != (CHANNEL_THR,):
        raise ValueError("cw must be [B][N] and thr hold 254 thresholds")
    N = cw.shape[1]
    if not 0 < N < (1 << 24) or b0 < 0 or b0 + B > (1 << 40):
        raise ValueError("N must be below 2^24 and the frames below 2^40")
    key = _splitmix64(np.array([(seed ^ CHANNEL_STREAM) & 0xFFFFFFFFFFFFFFFF], np.uint64))[0]
    b = np.arange(b0, b0 + B, dtype=np.uint64)[:, None]
    j = np.arange(N, dtype=np.uint64)[None, :]
    u = _splitmix64(((b << np.uint64(24)) | j) ^ key) >> np.uint64(11)
    k0 = np.searchsorted(thr, u.ravel(), side="right").reshape(B, N).astype(np.int64) - 127
    return np.ascontiguousarray(np.where((cw & 1) != 0, -k0, k0).astype(np.int8))


# --- sequenced reads for the LLR-construction stage -----
DNA_FIXTURES = os.path.join(GOLDEN, "dna_fixtures.npz")
_BASES = np.frombuffer(b"ACGT", np.uint8)


def quality_hist() -> np.ndarray:
    """Counts of per-read quality characters (ord) from the reference's
    72000_RS_Q_{0..9}.txt (tests/golden/dna_fixtures.npz)."""
    return np.load(DNA_FIXTURES, allow_pickle=False)["quality_hist"]


def strand_payloads(codewords: np.ndarray) -> np.ndarray:
    """[N][n_cw/2] uint8 ASCII: strand j's payload, nucleotide k = bits
    (2k, 2k+1) of codewords (DNA2binary order, def_func.py:97-117)."""
    bits = codewords.T.astype(np.int64)
    return _BASES[2 * bits[:, 0::2] + bits[:, 1::2]]


def dna_reads(codewords: np.ndarray, seed: int = 0, n_reads: int = 72000, sub: float = 0.01,
              ins: float = 0.0, dele: float = 0.0, p_bad_index: float = 0.0,
              quality: np.ndarray = None):
    """Simulated random-sampled reads after index decoding: (index values,
    payload strings, qualities).  Strand uniformly at random (the reference's
    random sampling of `--rs` reads), per-base substitution / insertion /
    deletion, a fraction of reads with a random (mostly invalid) 16-bit
    index, quality = ord(char) drawn from the reference's quality histogram."""
    import dna_llr
    rng = np.random.default_rng(seed)
    pay = strand_payloads(codewords)
    N, nt = pay.shape
    sidx = dna_llr.strand_indices()
    strand = rng.integers(0, N, n_reads)
    idx = sidx[strand].copy()
    bad = rng.random(n_reads) < p_bad_index
    idx[bad] = rng.integers(0, 1 << 16, int(bad.sum()))
    qh = quality_hist() if quality is None else quality
    qvals = np.nonzero(qh)[0]
    quals = rng.choice(qvals, n_reads, p=qh[qvals] / qh[qvals].sum()).astype(np.int64)
    r = pay[strand].copy()
    m = rng.random(r.shape) < sub
    r[m] = _BASES[(np.searchsorted(_BASES, r[m]) + rng.integers(1, 4, int(m.sum()))) % 4]
    seqs = [row.tobytes().decode() for row in r]
    if ins > 0 or dele > 0:
        n_ins = rng.binomial(nt, ins, n_reads)
        n_del = rng.binomial(nt, dele, n_reads)
        for k in np.nonzero((n_ins > 0) | (n_del > 0))[0]:
            s = list(seqs[k])
            for _ in range(int(n_del[k])):
                if s:
                    del s[int(rng.integers(0, len(s)))]
            for _ in range(int(n_ins[k])):
                s.insert(int(rng.integers(0, len(s) + 1)), "ACGT"[int(rng.integers(0, 4))])
            seqs[k] = "".join(s)
    return idx.tolist(), seqs, quals.tolist()


def dna_strands(codewords: np.ndarray, index=None, device=None) -> np.ndarray:
    """[N][16 + n_cw/2] uint8 ASCII: the strands to synthesise -- strand j =
    the 16-nt prefix of index[j] (index + RS(8,4) parity, dna_llr.encode_indices)
    followed by strand_payloads(codewords)[j]; the format of the reference's
    original files/final_DNA.txt.  index defaults to dna_llr.strand_indices();
    written on GPU `device`, or on the host when device is None."""
    import ctypes as C
    import dna_llr
    mod, L = dna_llr._lib()
    cw = np.ascontiguousarray(codewords, np.uint8)
    if cw.ndim != 2 or cw.shape[0] < 2 or cw.shape[0] % 2:
        raise ValueError("codewords come in nucleotide pairs (bits 2k, 2k+1 of a strand)")
    n_cw, N = cw.shape
    idx = np.asarray(dna_llr.strand_indices() if index is None else index)
    if idx.shape != (N,):
        raise ValueError(f"{N} strands need {N} index values")
    if idx.size and (idx.min() < 0 or idx.max() > 0xFFFF):
        raise ValueError("strand indices are 16-bit values (0..65535)")
    idx = np.ascontiguousarray(idx, np.int32)
    out = np.zeros((N, 16 + n_cw // 2), np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    if device is None:
        mod._check(L.ldpc_dna_strands_host(p(cw), n_cw, N, p(idx), p(out)))
    else:
        mod._check(L.ldpc_dna_strands(p(cw), n_cw, N, p(idx), p(out), device))
    return out


def dna_raw_reads(codewords: np.ndarray, seed: int = 0, n_reads: int = 72000, sub: float = 0.01,
                  ins: float = 0.0, dele: float = 0.0, quality: np.ndarray = None):
    """Simulated raw reads, before index decoding: (sequences, qualities) --
    the content of <rs>_RS_<t>.txt / <rs>_RS_Q_<t>.txt.  As dna_reads, but
    whole strands (dna_strands: prefix + payload) are sampled and the channel's
    substitutions / insertions / deletions fall on every position, the index
    prefix included."""
    rng = np.random.default_rng(seed)
    strands = dna_strands(codewords)
    N, nt = strands.shape
    strand = rng.integers(0, N, n_reads)
    qh = quality_hist() if quality is None else quality
    qvals = np.nonzero(qh)[0]
    quals = rng.choice(qvals, n_reads, p=qh[qvals] / qh[qvals].sum()).astype(np.int64)
    r = strands[strand].copy()
    m = rng.random(r.shape) < sub
    r[m] = _BASES[(np.searchsorted(_BASES, r[m]) + rng.integers(1, 4, int(m.sum()))) % 4]
    seqs = [row.tobytes().decode() for row in r]
    if ins > 0 or dele > 0:
        n_ins = rng.binomial(nt, ins, n_reads)
        n_del = rng.binomial(nt, dele, n_reads)
        for k in np.nonzero((n_ins > 0) | (n_del > 0))[0]:
            s = list(seqs[k])
            for _ in range(int(n_del[k])):
                if s:
                    del s[int(rng.integers(0, len(s)))]
            for _ in range(int(n_ins[k])):
                s.insert(int(rng.integers(0, len(s) + 1)), "ACGT"[int(rng.integers(0, 4))])
            seqs[k] = "".join(s)
    return seqs, quals.tolist()


# --- the counter-hashed sequencing channel (csrc/dna_sim.hpp) ---
SIM_ONE = 1 << 53        # probability 1 as a threshold
SIM_MAX_STRAND_NT = 399  # a read of 2L + 1 bytes stays within the planner's 800


def sim_stride(L: int) -> int:
    """Bytes between the starts of two reads: 2L + 1 rounded up to a multiple of 16."""
    return (2 * L + 1 + 15) // 16 * 16


def sim_tables(sub: float, ins: float, dele: float, quality: np.ndarray = None):
    """(t_sub, t_ins, t_del, q_val int32, q_lo uint32): the channel's integer
    thresholds int(p * 2**53) and its quality table -- the characters with a
    nonzero count of the histogram (quality_hist() by default), q_lo[i] =
    (count before i << 32) // total."""
    t = []
    for name, p in (("sub", sub), ("ins", ins), ("dele", dele)):
        if not 0.0 <= p <= 1.0:
            raise ValueError(f"{name} must be a probability")
        t.append(int(p * 2 ** 53))
    if t[0] + t[2] > SIM_ONE:
        raise ValueError("sub + dele must not exceed 1")
    qh = np.asarray(quality_hist() if quality is None else quality).astype(np.int64)
    q_val = np.nonzero(qh)[0]
    if qh.ndim != 1 or (qh < 0).any() or not 1 <= len(q_val) <= 256:
        raise ValueError("the quality histogram needs 1 .. 256 characters with a positive count")
    counts = [int(c) for c in qh[q_val]]
    total, before, q_lo = sum(counts), 0, []
    for c in counts:
        q_lo.append((before << 32) // total)
        before += c
    return t[0], t[1], t[2], np.ascontiguousarray(q_val, np.int32), np.array(q_lo, np.uint32)


def _sim_strands(strands) -> np.ndarray:
    s = np.ascontiguousarray(strands, np.uint8)
    if s.ndim != 2 or s.shape[0] < 1 or not 1 <= s.shape[1] <= SIM_MAX_STRAND_NT:
        raise ValueError(f"strands must be uint8 [S][L] with S >= 1 and 1 <= L <= {SIM_MAX_STRAND_NT}")
    return s


def _sim_return(buf, lens, quals, strand_of, stride, with_strands):
    seqs = (buf.reshape(-1), np.arange(len(lens), dtype=np.int64) * stride, lens)
    return (seqs, quals, strand_of) if with_strands else (seqs, quals)


def dna_raw_reads_hashed(strands: np.ndarray, seed: int, n_reads: int, sub: float = 0.01, ins: float = 0.0,
                         dele: float = 0.0, r0: int = 0, quality: np.ndarray = None, with_strands: bool = False):
    """The reads [r0, r0 + n_reads) of the counter-hashed channel over strands
    [S][L] (ASCII ACGT), in numpy from the definition --
    the replica the library's host and device forms are held equal to; it does
    not call the library.  With h(r, c, p) = splitmix64(((r << 24) | (c << 16)
    | p) ^ splitmix64(seed)), hi = >> 32, u = >> 11: strand (hi(h(r,0,0)) * S)
    >> 32; quality q_val[largest i with q_lo[i] <= hi(h(r,1,0))]; slot p <= L
    inserts "ACGT"[(hi(h(r,3,p)) * 4) >> 32] iff u(h(r,2,p)) < t_ins; base p <
    L, e = u(h(r,4,p)): deleted iff e < t_del, substituted iff e < t_del +
    t_sub by "ACGT"[(b + 1 + ((hi(h(r,5,p)) * 3) >> 32)) & 3], else copied; the
    read is insertion p, base p, ..., insertion L.

    Returns (seqs, quals), what ResidentTrial.run_raw takes: seqs the packed
    triple (buf uint8 [n_reads * stride], offsets int64 = i * stride, lengths
    int32), bytes beyond a read's length 0; quals int32.  with_strands: a third
    entry, the strand of every read (int32)."""
    s = _sim_strands(strands)
    S, L = s.shape
    t_sub, t_ins, t_del, q_val, q_lo = sim_tables(sub, ins, dele, quality)
    if not np.isin(s, _BASES).all():
        raise ValueError("strands hold a byte outside ACGT")
    if r0 < 0 or n_reads < 0 or r0 + n_reads > (1 << 40):
        raise ValueError("the reads must lie in [0, 2^40)")
    u64 = np.uint64
    seedmix = _splitmix64(np.array([seed & 0xFFFFFFFFFFFFFFFF], u64))[0]
    r = np.arange(r0, r0 + n_reads, dtype=u64)

    def h(c, p=None):  # [n] for p None (p = 0), else [n][len(p)]
        key = (r << u64(24)) | u64(c << 16)
        if p is not None:
            key = key[:, None] | p[None, :]
        return _splitmix64(key ^ seedmix)

    hi = lambda x: x >> u64(32)  # noqa: E731
    strand_of = ((hi(h(0)) * u64(S)) >> u64(32)).astype(np.int32)
    quals = q_val[np.searchsorted(q_lo.astype(u64), hi(h(1)), side="right") - 1].astype(np.int32)
    slots, pos = np.arange(L + 1, dtype=u64), np.arange(L, dtype=u64)
    ins_on = (h(2, slots) >> u64(11)) < u64(t_ins)
    ins_base = _BASES[((hi(h(3, slots)) * u64(4)) >> u64(32)).astype(np.int64)]
    e = h(4, pos) >> u64(11)
    kept = e >= u64(t_del)
    subst = kept & (e < u64(t_del + t_sub))
    src = s[strand_of]
    b = np.searchsorted(_BASES, src).astype(np.int64)
    sub_base = _BASES[(b + 1 + ((hi(h(5, pos)) * u64(3)) >> u64(32)).astype(np.int64)) & 3]
    # columns in output order: slot 0, base 0, slot 1, base 1, ..., slot L
    cand = np.zeros((n_reads, 2 * L + 1), np.uint8)
    take = np.zeros((n_reads, 2 * L + 1), bool)
    cand[:, 0::2], take[:, 0::2] = ins_base, ins_on
    cand[:, 1::2], take[:, 1::2] = np.where(subst, sub_base, src), kept
    lens = take.sum(axis=1).astype(np.int32)
    stride = sim_stride(L)
    buf = np.zeros((n_reads, stride), np.uint8)
    rows, cols = np.nonzero(take)
    buf[rows, (np.cumsum(take, axis=1) - 1)[rows, cols]] = cand[rows, cols]
    return _sim_return(buf, lens, quals, strand_of, stride, with_strands)


def dna_raw_reads_native(strands: np.ndarray, seed: int, n_reads: int, sub: float = 0.01, ins: float = 0.0,
                         dele: float = 0.0, r0: int = 0, quality: np.ndarray = None, with_strands: bool = False,
                         device=None):
    """dna_raw_reads_hashed in the library: ldpc_dna_sim_reads_host on one CPU
    thread (device None), or ldpc_dna_sim_reads on GPU `device` (k_sim_reads).
    Same arguments, same return shape, the same bytes up to every read's length."""
    import dna_llr
    mod, L = dna_llr._lib()
    s = _sim_strands(strands)
    t_sub, t_ins, t_del, q_val, q_lo = sim_tables(sub, ins, dele, quality)
    return _sim_native(mod, L, s, seed, r0, n_reads, t_sub, t_ins, t_del, q_val, q_lo, with_strands, device)


def _sim_native(mod, L, s, seed, r0, n_reads, t_sub, t_ins, t_del, q_val, q_lo, with_strands=False, device=None):
    """The library call of dna_raw_reads_native on ready tables (tests pass bad ones)."""
    import ctypes as C
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    S, nt = s.shape
    stride = int(L.ldpc_dna_sim_stride(nt)) or sim_stride(nt)
    n = max(int(n_reads), 0)
    buf = np.zeros((n, stride), np.uint8)
    lens, quals = np.zeros(n, np.int32), np.zeros(n, np.int32)
    strand_of = np.zeros(n, np.int32) if with_strands else None
    args = (p(s), S, nt, C.c_uint64(seed & 0xFFFFFFFFFFFFFFFF), int(r0), int(n_reads), int(t_sub), int(t_ins),
            int(t_del), p(q_val), p(q_lo), 0 if q_val is None else len(q_val), p(buf), p(lens), p(quals), p(strand_of))
    if device is None:
        mod._check(L.ldpc_dna_sim_reads_host(*args))
    else:
        mod._check(L.ldpc_dna_sim_reads(*args, int(device)))
    return _sim_return(buf, lens, quals, strand_of, stride, with_strands)


def dna_reads_edge_cases(codewords: np.ndarray, reads, seed: int = 1):
    """Append reads that put the rarer per-strand shapes of decoder.py's loop
    on fresh strands: single short read (q > 63 and q <= 63), single long
    read, ragged strands with no close pair, ragged strands whose padded
    alignment is not payload length (alignment failure), payload-length
    ragged alignment, non-ACGT characters, and a bit-271 one-vs-one tie."""
    import dna_llr
    idx, seqs, quals = (list(x) for x in reads)
    rng = np.random.default_rng(seed)
    pay = strand_payloads(codewords)
    sidx = dna_llr.strand_indices()
    used = set(idx)
    free = [j for j in rng.permutation(len(sidx)) if int(sidx[j]) not in used]
    it = iter(free)

    def add(j, s, q):
        idx.append(int(sidx[j])); seqs.append(s); quals.append(int(q))

    for q in (70, 60, 67):  # single short read
        j = next(it); add(j, pay[j].tobytes().decode()[:100 + q % 7], q)
    j = next(it); add(j, pay[j].tobytes().decode() + "ACG", 67)  # single long read
    j = next(it)  # ragged, no close pair
    add(j, "".join(rng.choice(list("ACGT"), 136)), 67); add(j, "".join(rng.choice(list("ACGT"), 120)), 67)
    for _ in range(2):  # ragged, padded length 138 != 136 -> alignment failure (kind 3)
        j = next(it); p = pay[j].tobytes().decode()
        add(j, p + "GA", 67); add(j, p[:-1], 70); add(j, p[:-3] + "C", 40)
    for _ in range(2):  # ragged, padded length 136 -> aligned rows counted
        j = next(it); p = pay[j].tobytes().decode()
        add(j, p, 67); add(j, p[:-2], 66); add(j, p[:130], 55)
    j = next(it); p = pay[j].tobytes().decode()  # non-ACGT characters
    add(j, p[:50] + "N" + p[51:], 67); add(j, p[:10] + "-" + p[11:], 67)
    j = next(it); p = pay[j].tobytes().decode()  # tie at bit 271: one 0 vs one 1 among q >= 53
    last = "A" if p[-1] in "CT" else "C"
    add(j, p, 60); add(j, p[:-1] + last, 66); add(j, p, 40)
    return idx, seqs, quals
