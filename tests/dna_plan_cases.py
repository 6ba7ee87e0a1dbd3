"""TEST INFRASTRUCTURE: the inputs and the Python comparator shared by the
read-planner tests (test_dna_plan.py on the CPU, test_dna_plan_gpu.py on the
GPU).  The comparator is dna_llr.plan_llr itself with the built-in aligner on
the host and the numpy Levenshtein below in place of the GPU distances."""
from functools import lru_cache

import numpy as np

import dna_llr
import synth
from star_cases import mutate


def levenshtein_pairs(seqs, pairs):
    """plan_llr's distance_fn without the library: the Levenshtein table of
    every pair at once (numpy across the pairs, Python loops over the cells;
    the recurrence of def_func.edit_dist)."""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    P = len(pairs)
    if P == 0:
        return np.zeros(0, np.int32)
    used = sorted(set(pairs.ravel().tolist()))
    slot = {r: k for k, r in enumerate(used)}
    W = max(len(seqs[r]) for r in used)
    tab = np.zeros((len(used), W + 1), np.int32)  # 0 pads, never equal to a character that counts
    ln = np.zeros(len(used), np.int64)
    for r in used:
        b = np.frombuffer(seqs[r].encode("latin-1"), np.uint8)
        tab[slot[r], :len(b)] = b.astype(np.int32) + 1
        ln[slot[r]] = len(b)
    ia = np.array([slot[r] for r in pairs[:, 0].tolist()])
    ib = np.array([slot[r] for r in pairs[:, 1].tolist()])
    A, B, la, lb = tab[ia], tab[ib], ln[ia], ln[ib]
    row = np.tile(np.arange(W + 1, dtype=np.int32), (P, 1))
    out = row[np.arange(P), lb].copy()  # la == 0
    for i in range(1, int(la.max()) + 1):
        new = np.empty_like(row)
        new[:, 0] = i
        ai = A[:, i - 1]
        for j in range(1, W + 1):
            sub = row[:, j - 1] + (ai != B[:, j - 1])
            new[:, j] = np.minimum(sub, np.minimum(row[:, j], new[:, j - 1]) + 1)
        row = new
        m = la == i
        out[m] = row[m, lb[m]]
    return out.astype(np.int32)


def reference_plan(index_vals, seqs, quals, strands=None):
    """The yardstick: the existing Python planner, off the GPU."""
    return dna_llr.plan_llr(index_vals, seqs, quals, align_fn="star", align_host=True,
                            distance_fn=levenshtein_pairs, strands=strands)


@lru_cache(maxsize=None)
def edge_input():
    """The 3000-read channel of test_build_llr_star_bitexact_vs_oracle with
    synth's edge cases, plus the shape those lack: an empty read of quality
    <= 63 alone on a fresh strand."""
    cw = synth.load_codewords()
    reads = synth.dna_reads(cw, seed=21, n_reads=3000, sub=0.01, ins=0.003, dele=0.003, p_bad_index=0.05)
    idx, seqs, quals = synth.dna_reads_edge_cases(cw, reads, seed=121)
    used = set(idx)
    free = next(int(v) for v in dna_llr.strand_indices() if int(v) not in used)
    return idx + [free], seqs + [""], quals + [60], None


@lru_cache(maxsize=None)
def dense_input(seed=7, n_strands=150):
    """`strands`: n_strands random 16-bit values; 3..8 reads each, mutated
    copies of one 136-nt payload (0..6 edits, so most strands are ragged with
    close pairs) and some unrelated reads; a few reads carry an index that is
    no strand.  The reads are shuffled."""
    rng = np.random.default_rng(seed)
    strands = np.sort(rng.choice(1 << 16, n_strands, replace=False)).astype(np.int64)
    member = set(strands.tolist())
    idx, seqs, quals = [], [], []
    for s in strands.tolist():
        parent = "".join(rng.choice(list("ACGT"), dna_llr.PAYLOAD_NT))
        for _ in range(int(rng.integers(3, 9))):
            if rng.random() < 0.1:
                r = "".join(rng.choice(list("ACGT"), int(rng.integers(120, 150))))
            else:
                r = mutate(rng, parent, "ACGT", int(rng.integers(0, 7)))
            idx.append(s), seqs.append(r), quals.append(int(rng.integers(35, 75)))
    for _ in range(40):
        v = int(rng.integers(0, 1 << 16))
        if v not in member:
            idx.append(v), seqs.append(parent), quals.append(67)
    order = rng.permutation(len(idx))
    return [idx[i] for i in order], [seqs[i] for i in order], [quals[i] for i in order], strands


@lru_cache(maxsize=None)
def reference(name):
    idx, seqs, quals, strands = {"edge": edge_input, "dense": dense_input}[name]()
    return reference_plan(idx, seqs, quals, strands)


def same_plan(got, want, counters=True):
    R = int(want.row_ptr[-1])
    assert np.array_equal(got.kind, want.kind)
    assert np.array_equal(got.row_ptr, want.row_ptr)
    assert got.rows.shape == want.rows.shape and got.row_q.shape == want.row_q.shape
    assert np.array_equal(got.rows[:R], want.rows[:R])
    assert np.array_equal(got.row_q[:R], want.row_q[:R])
    if counters:
        assert (got.n_reads_valid, got.n_pairs, got.n_aligned_strands, got.n_align_pairs) == \
            (want.n_reads_valid, want.n_pairs, want.n_aligned_strands, want.n_align_pairs)
