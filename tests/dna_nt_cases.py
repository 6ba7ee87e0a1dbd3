"""TEST INFRASTRUCTURE: reads at payload lengths other than the DNA file's 136
nt and their yardstick, shared by test_dna_payload_nt.py (CPU) and
test_dna_payload_nt_gpu.py (GPU).  The yardstick is the plain-Python
restatement of the reference's loop, dna_llr_oracle.build_llr with nbits = 2 *
nt, and the independent aligner star_ref.star_align: no library code.  The raw
reads further down come from the numpy channel synth.dna_raw_reads_hashed over
strands the library's host code writes (synth.dna_strands)."""
import math
from functools import lru_cache

import numpy as np

import dna_llr
import dna_llr_oracle as dorc
import star_ref
import synth
from star_cases import mutate

EPS = 0.02
# (payload_nt, strands): 1 and 4 are one lane of k_plan_rows' byte and dword
# paths, 13 is odd and under one wave, 65 is odd and needs a second trip of the
# byte path (stride 64), 260 a second trip of the dword path (stride 256).  The
# strand counts keep the Python oracle within a few seconds.
NTS = [(1, 120), (4, 120), (13, 200), (65, 300), (260, 40)]


def seed_of(nt):
    return 100 + nt


@lru_cache(maxsize=None)
def reads(nt, n_strands, seed):
    """(index_vals, seqs, quals, strands) in the style of
    dna_plan_cases.dense_input: `strands` are n_strands random sorted 16-bit
    values with 0..6 reads each -- about 10 % unrelated reads of length nt +- 8
    (not below 0), about 40 % star_cases.mutate copies of the strand's payload
    with 0..3 edits, the rest full-length copies with one substitution.
    Qualities 35..74, but at most 63 on an empty read (alone on its strand, an
    empty read of a higher quality is the planner's argument error, as it is
    the reference's IndexError), and at most one empty read per strand (the
    reference indexes the last character of a row the aligner returns, so a
    strand of empty reads alone is outside its domain): a second one is
    replaced by the payload.  The reads are shuffled."""
    rng = np.random.default_rng(seed)
    strands = np.sort(rng.choice(1 << 16, n_strands, replace=False)).astype(np.int64)
    idx, seqs, quals = [], [], []
    for s in strands.tolist():
        parent = "".join(rng.choice(list("ACGT"), nt))
        has_empty = False
        for _ in range(int(rng.integers(0, 7))):
            u = rng.random()
            if u < 0.1:
                r = "".join(rng.choice(list("ACGT"), max(0, nt + int(rng.integers(-8, 9)))))
            elif u < 0.5:
                r = mutate(rng, parent, "ACGT", int(rng.integers(0, 4)))
            else:
                p = int(rng.integers(0, nt))
                r = parent[:p] + "ACGT"[int(rng.integers(0, 4))] + parent[p + 1:]
            if not r and has_empty:
                r = parent
            has_empty |= not r
            idx.append(s), seqs.append(r), quals.append(int(rng.integers(35, 75 if r else 64)))
    order = rng.permutation(len(idx))
    return [idx[i] for i in order], [seqs[i] for i in order], [quals[i] for i in order], strands


def case(nt):
    return reads(nt, dict(NTS)[nt], seed_of(nt))


_ORACLE = {}


def _key(nt, case):
    idx, seqs, quals, strands = case
    return (nt, tuple(idx), tuple(seqs), tuple(quals), tuple(int(v) for v in strands))


def oracle_llr(nt, case):
    """(llr [2nt][S] float64, int_mask [2nt][S] uint8, codes [2nt][S] int8) of
    the oracle at eps = EPS; codes = the count differences llr / unit, saturated
    to int8 as the kernels' are (the CPU test asserts that nothing saturates on
    the committed inputs).  Computed once per input."""
    idx, seqs, quals, strands = case
    key = _key(nt, case)
    if key not in _ORACLE:
        by_strand = dorc.build_llr(idx, seqs, quals, [int(v) for v in strands], EPS, star_ref.star_align, nbits=2 * nt)
        llr = np.array([[float(v[i]) for v in by_strand] for i in range(2 * nt)], np.float64).reshape(2 * nt, -1)
        mask = np.array([[type(v[i]) is int for v in by_strand] for i in range(2 * nt)], np.uint8).reshape(2 * nt, -1)
        diff = np.rint(llr / math.log((1 - EPS) / EPS)).astype(np.int64)
        for a in (llr, mask, diff):
            a.setflags(write=False)
        _ORACLE[key] = (llr, mask, diff)
    llr, mask, diff = _ORACLE[key]
    return llr, mask, np.clip(diff, -127, 127).astype(np.int8)


def count_differences(nt, case):
    """The oracle's count differences before the int8 saturation (int64)."""
    oracle_llr(nt, case)
    return _ORACLE[_key(nt, case)][2]


def reference_kinds(nt, case):
    """(kind [S], widths, groups): every strand's kind by the rules of
    dna_llr's docstring, and of every strand that goes to the aligner the
    aligned width and the candidate reads -- from the reads alone, with
    star_ref's distances and alignment."""
    idx, seqs, quals, strands = case
    pos = {int(v): k for k, v in enumerate(strands)}
    by = {}
    for v, s in zip(idx, seqs):
        if v in pos:
            by.setdefault(pos[v], []).append(s)
    kind, widths, groups = np.zeros(len(strands), np.int32), {}, {}
    for s, rd in by.items():
        if len(rd) == 1:
            kind[s] = 2 if len(rd[0]) < nt else 1
        elif all(len(r) == nt for r in rd):
            kind[s] = 1
        else:
            close = set()
            for a in range(len(rd)):
                for b in range(a + 1, len(rd)):
                    if star_ref.distance(rd[a], rd[b]) < 15:
                        close |= {a, b}
            if close:
                groups[s] = [rd[a] for a in sorted(close)]
                widths[s] = star_ref.star(groups[s])[1]
                kind[s] = 1 if widths[s] == nt else 3
    return kind, widths, groups


def unpacked(seqs):
    """A packed (buf, offsets, lengths) triple as a list of str."""
    buf, offs, lens = seqs
    return [bytes(buf[o:o + n]).decode("latin-1") for o, n in zip(offs.tolist(), lens.tolist())]


def raw_reads(cw, index, seed, n_reads, rates):
    """(strands, (packed raw reads, qualities)): the strands of codewords cw
    [2nt][S] under the index values `index`, and n_reads reads of them through
    the counter-hashed channel at rates = (sub, ins, dele), prefix included."""
    strands = synth.dna_strands(cw, index)
    assert strands.shape == (cw.shape[1], 16 + cw.shape[0] // 2)
    seqs, quals = synth.dna_raw_reads_hashed(strands, seed, n_reads, *rates)
    assert not ((seqs[2] == 16) & (quals > 63)).any()  # (an empty payload with quality > 63 is the planner's error)
    return strands, (seqs, quals)


@lru_cache(maxsize=None)
def raw_case(nt, n_strands=150, n_reads=500, seed=3):
    """(packed raw reads, qualities, strand index values) of random codewords [2nt][n_strands]."""
    rng = np.random.default_rng(seed + nt)
    index = np.sort(rng.choice(1 << 16, n_strands, replace=False)).astype(np.int64)
    cw = rng.integers(0, 2, (2 * nt, n_strands)).astype(np.uint8)
    _, (seqs, quals) = raw_reads(cw, index, seed, n_reads, (0.03, 0.01, 0.01))
    return seqs, quals, index


def trial_case(G, n_cw, seed, n_reads, rates):
    """One resident-trial input of code G with n_cw codewords, so payloads of
    n_cw / 2 nt: codewords from the host encoder, random 16-bit index values,
    raw reads of the strands, and the yardstick's codes -- the host index
    split, then the oracle's count differences."""
    nt = n_cw // 2
    enc = G.encoder()
    cw = enc.encode_host(synth.random_messages(enc.K, 0, n_cw, seed=3))
    index = np.sort(np.random.default_rng(50 + nt).choice(1 << 16, G.N, replace=False)).astype(np.int64)
    strands, raw = raw_reads(cw, index, seed, n_reads, rates)
    reads, hist = dna_llr.split_reads_counted(unpacked(raw[0]), raw[1].tolist(), host=True)
    case = (*reads, index)
    codes = oracle_llr(nt, case)[2]
    assert np.abs(count_differences(nt, case)).max() <= 127
    return dict(nt=nt, cw=cw, index=index, strands=strands, raw=raw, reads=reads, hist=hist, codes=codes)
