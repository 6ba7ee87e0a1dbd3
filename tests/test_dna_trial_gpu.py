"""The device-resident trial (ldpc_trial_*, dna_pipeline.ResidentTrial; the
kernels of csrc/dna_trial_kernels.hpp) against the
existing Python flow -- dna_pipeline.decode_trial / trial_from_raw_reads with
the GPU decoder through the host API -- field by field."""
import math

import numpy as np
import pytest

import dna_llr
import dna_pipeline as P
import dna_plan_cases as cases
import synth
from test_star_align_gpu import E2E

pytestmark = pytest.mark.gpu
EPS = 0.02
UNIT = math.log((1 - EPS) / EPS)
KEYS = ("n", "first_success", "second_success", "fail_first", "fail_second", "second_iterations", "first_errors",
        "second_errors", "erasure_index")


def _same(new, old, keys=KEYS):
    for key in keys:
        assert new[key] == old[key], key
    assert np.array_equal(new["hard"], old["hard"])


def _python_flow(G, codes, cw, max_iter, faithful=True, algo="bp"):
    llr = P.code_table(UNIT)[codes.astype(np.int64) + 128]
    return P.decode_trial(llr, cw, eps=EPS, max_iter=max_iter, decode_fn=P.gpu_decode_fn(G, algo), faithful=faithful,
                          codes=codes)


def _irregular(L):
    """N = 1003 (no multiple of 4, of 64 or of a block's columns), column degrees 2..4."""
    rng = np.random.default_rng(42)
    M, N = 300, 1003
    rows, cols = [], []
    for j in range(N):
        for i in rng.choice(M, size=int(rng.integers(2, 5)), replace=False):
            rows.append(int(i))
            cols.append(j)
    return L.Graph.from_edges(M, N, rows, cols)


# (graph, BSC seed): 65 codewords through a BSC(0.01) as +-1 codes.  At max_iter 3
# (checked on the CPU oracle) the first decode fails rows 1, 42, 49, 55 of the
# RS-LDPC code, all of which decode by the 25th second decode, and 12 rows of
# the irregular code, rows 1 and 2 among them, one of which decodes later: row
# 1 fails in every batch below, rows succeed next to it from B = 5 on.
SMALL = {"rs": (lambda L: L.Graph.rs_ldpc(5, 16, 4), 3), "irregular": (_irregular, 2)}
SMALL_ITERS = 3


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
def test_run_codes_small_codes(small, name, B):
    """k_trial_stats / gather / scatter: one row, a few, and 65 (a second tile
    of the engine, a ragged last row chunk of the statistics kernel)."""
    G, cw, codes = small[name]
    T = P.ResidentTrial(G, cw[:B])
    for faithful in ((True, False) if B == 65 else (True,)):
        new = T.run_codes(codes[:B], eps=EPS, max_iter=SMALL_ITERS, faithful=faithful)
        old = _python_flow(G, codes[:B], cw[:B], SMALL_ITERS, faithful)
        _same(new, old)
        assert 1 in old["fail_first"] and old["second_iterations"] >= 1
        assert B == 1 or old["first_success"] > 0
    _, _, it, v = G.decode_codes(codes[:B], P.code_table(UNIT), max_iter=SMALL_ITERS, post=None)
    assert np.array_equal(new["iters"], it) and np.array_equal(new["valid"], v)
    T.close()


def test_run_codes_min_sum(small):
    G, cw, codes = small["rs"]
    new = P.ResidentTrial(G, cw, algo="msa").run_codes(codes, eps=EPS, max_iter=SMALL_ITERS)
    old = _python_flow(G, codes, cw, SMALL_ITERS, algo="msa")
    _same(new, old)
    assert old["fail_first"]


def test_handle_reuse_leaves_nothing_behind(small, gpu):
    """The same handle with other inputs, then a fresh one: stale errors /
    re_decode accumulators, batch rows or flags would show."""
    G, cw, codes = small["irregular"]
    other = np.where((cw ^ synth.bsc_flips(0, 65, G.N, 9, 0.02).astype(np.uint8)) == 1, -1, 1).astype(np.int8)
    T = P.ResidentTrial(G, cw, strands=np.arange(G.N))  # (index values: the read call below gets to the library)
    first = T.run_codes(codes, eps=EPS, max_iter=SMALL_ITERS)
    second = T.run_codes(other[:5], eps=EPS, max_iter=SMALL_ITERS, faithful=False)  # fewer rows than the handle holds
    third = T.run_codes(codes, eps=EPS, max_iter=SMALL_ITERS)
    fresh = P.ResidentTrial(G, cw).run_codes(other[:5], eps=EPS, max_iter=SMALL_ITERS, faithful=False)
    _same(second, fresh)
    _same(second, _python_flow(G, other[:5], cw[:5], SMALL_ITERS, faithful=False))
    _same(third, first)
    assert np.array_equal(T.codes(65), codes)
    # the argument errors that need a handle
    with pytest.raises(gpu.LdpcError) as e:
        T.run_codes(np.concatenate([codes, codes[:1]]))
    assert e.value.code == gpu.LDPC_ERR_ARG
    with pytest.raises(gpu.LdpcError) as e:
        T.run_codes(codes[:0])
    assert e.value.code == gpu.LDPC_ERR_ARG
    with pytest.raises(gpu.LdpcError) as e:
        T.run_codes(codes, eps=0.6)
    assert e.value.code == gpu.LDPC_ERR_ARG
    with pytest.raises(gpu.LdpcError, match="2 \\* payload_nt == n_cw") as e:
        T.run_raw((["ACGT" * 40], [60]))
    assert e.value.code == gpu.LDPC_ERR_ARG
    assert _same(T.run_codes(codes, eps=EPS, max_iter=SMALL_ITERS), first) is None  # still usable


@pytest.fixture(scope="module")
def dna16(codewords):
    return synth.dna_like_codes(codewords, seed=1, reads=57000)[:16], codewords[:16]


def test_dna_16_codewords(G, dna16):
    k, cw = dna16
    new = P.ResidentTrial(G, cw).run_codes(k, eps=EPS, max_iter=200)
    old = _python_flow(G, k, cw, 200)
    _same(new, old)
    assert new["fail_first"] == [14] and new["second_iterations"] >= 1
    assert P.report(new) == P.report(old)


def test_genie_less(G, dna16):
    """Without the codewords a row fails iff its valid flag is 0: the lists
    against the valid flags of Graph.decode_codes, replayed stage by stage."""
    k, _ = dna16
    res = P.ResidentTrial(G, None, n_cw=16).run_codes(k, eps=EPS, max_iter=200)
    table = P.code_table(UNIT)
    hard, _, _, v = G.decode_codes(k, table, max_iter=200, post=None)
    fail = (np.nonzero(~v)[0] + 1).tolist()
    assert fail and res["fail_first"] == fail and np.array_equal(res["valid"], v)
    assert res["first_errors"] == {i: -1 for i in fail}
    fail2, eps2, iters = list(fail), EPS - 0.0005, 0
    while fail2 and eps2 > 0.001:
        iters += 1
        h2, _, _, v2 = G.decode_codes(k[np.array(fail2) - 1], P.rescale(table, EPS, eps2), max_iter=200, post=None)
        eps2 = eps2 - 0.0005
        for q, i in enumerate(fail2):
            if v2[q]:
                hard[i - 1] = h2[q]
        fail2 = [] if v2[-1] else [fail2[-1]]  # faithful: the last row's outcome survives
    assert res["fail_second"] == fail2 and res["second_iterations"] == iters
    assert np.array_equal(res["hard"], hard)


def test_code_kernel_equals_llr_kernel(G, codewords):
    """k_dna_codes on the 3000-read edge-case input: the handle's code matrix
    is ldpc_dna_reads_llr's codes byte for byte, with the same codes_exact; the
    trial on it equals the Python flow on those codes."""
    idx, seqs, quals, _ = cases.edge_input()
    built, _ = dna_llr.build_llr_native(idx, seqs, quals, eps=EPS)
    assert built.codes is not None and set(np.unique(built.kind).tolist()) == {0, 1, 2, 3}
    T = P.ResidentTrial(G, codewords)
    # (at max_iter 2 every row fails; eps 0.003 keeps the second decode to three rounds of 272 rows)
    new = T.run_reads((idx, seqs, quals), eps=0.003, max_iter=2)
    assert new["resident"] is True
    assert np.array_equal(T.codes(), built.codes)
    assert np.array_equal(new["kind"], built.kind)
    assert (new["n_reads_valid"], new["n_align_pairs"]) == (built.n_reads_valid, built.n_align_pairs)
    llr = P.code_table(math.log((1 - 0.003) / 0.003))[built.codes.astype(np.int64) + 128]
    old = P.decode_trial(llr, codewords, eps=0.003, max_iter=2, decode_fn=P.gpu_decode_fn(G), codes=built.codes)
    _same(new, old)
    assert old["second_iterations"] == 3 and len(old["fail_first"]) > 200


def test_full_raw_trial(G, codewords):
    raw = synth.dna_raw_reads(codewords, **E2E)
    packed = (dna_llr._concat(raw[0]), raw[1])
    old = P.trial_from_raw_reads(packed, codewords, eps=EPS, align_fn="star", native=True)
    new = P.ResidentTrial(G, codewords).run_raw(packed, eps=EPS)
    print("resident: llr %.4f first %.4f second %.4f s; host path: llr %.4f first %.4f second %.4f s" % (
        new["t_llr_s"], new["t_first_s"], new["t_second_s"], old["t_llr_s"], old["t_first_s"], old["t_second_s"]))
    _same(new, old)
    assert new["second_success"] == 272 and not new["fail_second"] and new["resident"] is True
    assert set(old) <= set(new) and new["llr"] is None
    for key in ("n_erased_strands", "n_reads_valid", "n_align_pairs", "n_reads_dropped", "cnumerr_hist", "t_index_s",
                "t_align_s"):
        assert new[key] == old[key], key
    assert np.array_equal(new["kind"], old["llr"].kind)
    assert new["stats"][0] == old["n_reads_valid"] and new["stats"][3] == old["n_align_pairs"]
    assert P.report(new) == P.report(old)


def test_overflow_falls_back(G, gpu, codewords):
    """300 reads on one strand: count differences beyond int8.  The C call
    says LDPC_ERR_UNSUPPORTED with codes_exact 0; run_raw falls back to the
    host path and gives its result."""
    rng = np.random.default_rng(11)
    v = int(dna_llr.strand_indices()[100])
    prefix = bytes(dna_llr.encode_indices([v])[0]).decode()
    parent = "".join(rng.choice(list("ACGT"), dna_llr.PAYLOAD_NT))
    seqs = [prefix + parent] * 300
    quals = rng.integers(55, 75, 300).tolist()
    T = P.ResidentTrial(G, codewords)
    mod, lib = dna_llr._lib()
    buf, offs, lens, q, _, sidx, n = dna_llr._native_inputs(None, seqs, quals, None)
    out = P._TrialOut(272, G.N, n_strands=len(sidx))
    p = dna_llr._p
    rc = lib.ldpc_trial_run_reads(T._h, p(buf), p(offs), p(lens), p(q), n, None, p(sidx), len(sidx), dna_llr.PAYLOAD_NT,
                                  1, 0, 0.003, 2, 1, out.ref())
    assert rc == gpu.LDPC_ERR_UNSUPPORTED and out.r.codes_exact == 0
    assert b"outside int8" in lib.ldpc_last_error()
    assert int(out.a["stats"][0]) == 300 and (out.a["kind"] == 1).sum() == 1
    new = T.run_raw((seqs, quals), eps=0.003, max_iter=2)
    old = P.trial_from_raw_reads((seqs, quals), codewords, eps=0.003, max_iter=2, align_fn="star", native=True)
    assert new["resident"] is False and old["llr"].codes is None
    _same(new, old)
    assert new["cnumerr_hist"] == old["cnumerr_hist"] and set(new) == set(old) | {"resident"}
