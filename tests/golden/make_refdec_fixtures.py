"""Regenerate tests/golden/refdec_goldens.npz from the REFERENCE's own decoders,
compiled unmodified by `make -C oracle ref` into oracle/_ref/librefdec.so
(dec.cpp behind oracle/ref_dec_harness.cpp).

Per code (tests/refdec_cases.py: reg4, perm4, rs5, irr and the DNA code) and
algorithm (BP on fp64 likelihood ratios, BP on a 256-entry table of them,
min-sum, Gallager A / B1 / B2, quantised min-sum over q x step x beta) it
stores the reference's hard bits (packed), iteration counts, valid flags and
a 16-byte sha256 digest of every word's posterior bytes (NaNs made one NaN);
for the first words of the small codes the posterior itself; for quantised
min-sum the number of tie draws per word.  Per code: the edge list as written
to the .pchk (the DNA code's file is committed) and the file's sha256; per
input matrix its sha256.  Only data -- no reference source -- is stored.

The inputs come from integers alone (refdec_cases), and their noise figures
were chosen by the reference's outputs alone; this script asserts what they
were chosen for and prints what it measured.

    python tests/golden/make_refdec_fixtures.py [out.npz]
"""
import hashlib
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "dna-ldpc-codes_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import refdec_cases as R  # noqa: E402
import oracle  # noqa: E402


def reference_decode(rd, algo, x, max_iter):
    """(hard, post, iters, valid, ties) from the reference; post None for Gallager."""
    if algo in ("bp", "bpc"):
        return rd.bp(x, max_iter) + (None,)
    if algo == "msa":
        return rd.msa(x, max_iter) + (None,)
    if algo in R.GALLAGER:
        return rd.gallager(R.recv_of(x), R.GALLAGER[algo], max_iter) + (None,)
    q, step, beta = R.QCFG[algo]
    return rd.qmsa(x, max_iter, q, step, beta)


def oracle_decode(og, algo, x, max_iter):
    """The same call on the oracle (tie bits: its own hash, seed 0)."""
    if algo in ("bp", "bpc"):
        out = [og.bp(x[b], max_iter) for b in range(len(x))]
        return (np.array([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out], np.int32),
                np.array([o[3] for o in out], np.uint8))
    if algo == "msa":
        return og.decode_batch(x, max_iter, algo=oracle.ALGO_MSA)
    if algo in R.GALLAGER:
        h, _, it, v = og.decode_int_batch(x, max_iter, 3 + R.GALLAGER[algo])
        return h, None, it, v
    q, step, beta = R.QCFG[algo]
    h, p, it, v = og.decode_int_batch(x, max_iter, oracle.ALGO_QMSA, precision=q, step=step, beta=beta)
    return h, p.astype(np.int32), it, v


def check_spread(code, algo, iters, valid, max_iter, ties):
    """The conditions the noise figures were chosen for."""
    B, u = len(iters), set(int(v) for v in iters)
    between = sorted(k for k in u if 1 < k < max_iter)
    ok, bad = int((valid != 0).sum()), int((valid == 0).sum())
    what = (code, algo, sorted(u), ok, bad)
    assert 0 in u and max_iter in u, what
    assert 4 * ok >= B and 4 * bad >= B, what
    if (code, algo) not in R.CLIFF:
        assert 1 in u and len(between) >= 3, what
    stat = {"iters": {str(k): int((iters == k).sum()) for k in sorted(u)}, "valid": ok, "failed": bad}
    if ties is not None:
        free = ties == 0
        need = 4 if code == "dna" else 32
        assert free.sum() >= need and (valid[free] != 0).any() and (valid[free] == 0).any(), what + (int(free.sum()),)
        stat.update(tie_free=int(free.sum()), tie_free_failed=int((valid[free] == 0).sum()))
    return stat


def select_words(iters, valid, max_iter, ties, n=R.B_DNA):
    """The DNA code's words, chosen from the candidates by the reference's
    outputs alone: the first word that stops at 0, at 1, at each of three
    counts between, two that fail, then the first ones left; among equals a
    word without tie draws first, and a failing one of them at any rate."""
    free = np.ones(len(iters), bool) if ties is None else ties == 0
    order = sorted(range(len(iters)), key=lambda b: (not free[b], b))
    pick = []

    def take(cond, count=1):
        for b in order:
            if count and b not in pick and cond(b):
                pick.append(b)
                count -= 1

    take(lambda b: iters[b] == 0)
    take(lambda b: iters[b] == 1)
    take(lambda b: not valid[b] and free[b])
    take(lambda b: not valid[b], 2 - sum(1 for b in pick if not valid[b]))
    for k in sorted(set(int(v) for v in iters if 1 < v < max_iter))[:4]:
        take(lambda b: iters[b] == k and valid[b])
    take(lambda b: valid[b] and free[b], n - len(pick))
    take(lambda b: True, n - len(pick))
    return np.array(sorted(pick[:n]), np.int16)


def tie_word_agreement(ref, orc):
    """Words with ties: where the oracle's hashed tie bits led to the same
    iteration count, L_Q and the hard bits off zero posteriors must agree.
    Returns (words with ties, of them with equal counts, of those agreeing)."""
    h, p, it, v, ties = ref
    oh, op, oit, _ = orc
    tied = np.flatnonzero(ties > 0)
    same = [b for b in tied if it[b] == oit[b]]
    agree = [b for b in same if np.array_equal(p[b], op[b]) and np.array_equal(h[b][p[b] != 0], oh[b][p[b] != 0])]
    return len(tied), len(same), len(agree)


def build(tmp, log=print, words=None, codes=R.CODES, algos=None, with_oracle=True):
    """words: {'dna/<algo>/': indices} skips the DNA code's candidate decodes
    (a recorded choice); codes / algos(code) narrow what is made;
    with_oracle=False leaves the tie words' comparison with the oracle out."""
    out, stats = {}, {}
    for code in codes:
        if code == "dna":
            path = R.DNA_PCHK
            c0 = R.pchk_row0(path)
        else:
            M, N, rows, cols = R.make_edges(code)
            path = os.path.join(tmp, code + ".pchk")
            R.write_pchk(path, M, N, rows, cols)
            c0 = R.row0_cols(rows, cols)
            out[f"{code}/edges"] = np.array([rows, cols], np.int16)
            out[f"{code}/shape"] = np.array([M, N], np.int32)
        out[f"{code}/pchk_sha256"] = np.array(R.file_sha(path))
        rd = oracle.RefDecoder(path)
        og = oracle.OracleGraph(path) if with_oracle else None
        for algo in (R.ALGOS if algos is None else algos(code)):
            x, max_iter = R.make_input(code, algo, rd.N, c0, R.SEED, R.NOISE)
            k = f"{code}/{algo}/"
            if code == "dna":  # decode the candidates, keep 8 (or the 8 named by `words`)
                w = words[k] if words is not None else None
                if w is None:
                    cand = reference_decode(rd, algo, x, max_iter)
                    w = select_words(cand[2], cand[3], max_iter, cand[4])
                out[k + "words"] = w
                x = np.ascontiguousarray(x[w])
            ref = reference_decode(rd, algo, x, max_iter)
            h, p, it, v, ties = ref
            st = check_spread(code, algo, it, v, max_iter, ties)
            out[k + "in_sha256"] = np.array(hashlib.sha256(x.tobytes()).hexdigest())
            out[k + "max_iter"] = np.int32(max_iter)
            out[k + "hard"] = R.packbits(h)
            out[k + "iters"] = it.astype(np.int16)
            out[k + "valid"] = v.astype(np.uint8)
            if p is not None:
                out[k + "post_sha"] = R.digests(p)
                if code != "dna":
                    out[k + "post_raw"] = R.canon(p[:R.RAW_WORDS])
            if code != "dna":
                for m in R.SHORT.get(algo, ()):  # the same words cut short
                    sh, sp, sit, sv, _ = reference_decode(rd, algo, x, m)
                    assert np.array_equal(sit, np.minimum(it, m))
                    out[k + f"m{m}/hard"], out[k + f"m{m}/valid"] = R.packbits(sh), sv.astype(np.uint8)
                    out[k + f"m{m}/post_sha"] = R.digests(sp, 8)
            if ties is not None:
                out[k + "ties"] = ties.astype(np.int32)
                if with_oracle:
                    n_tied, n_same, n_agree = tie_word_agreement(ref, oracle_decode(og, algo, x, max_iter))
                    st.update(tied=n_tied, tied_same_count=n_same, tied_agree=n_agree)
            stats[f"{code}/{algo}"] = st
            log(f"{code:6s}{algo:10s} max_iter {max_iter:2d} {json.dumps(st)}")
    # the quantiser row: Cal_MSA_Q on values outside the int range (and inside it)
    for q, step in sorted({(q, s) for q, s, _ in R.QMSA_GRID}):
        out[f"quant/q{q}_s{int(step * 10):02d}"] = rd.quantise(R.QUANT_X, q, step)
    out["stats"] = np.array(json.dumps(stats, sort_keys=True))
    return out


def main(argv):
    if not oracle.refdec_available():
        sys.exit("oracle/_ref/librefdec.so is not built: run `make -C oracle ref` where the reference sources are")
    dst = argv[1] if len(argv) > 1 else R.FIXTURE
    with tempfile.TemporaryDirectory() as tmp:
        out = build(tmp)
    np.savez_compressed(dst, **out)
    print(f"{dst}: {os.path.getsize(dst)} bytes")


if __name__ == "__main__":
    main(sys.argv)
