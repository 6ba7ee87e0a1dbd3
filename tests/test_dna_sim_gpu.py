"""The sequencing channel on the GPU (k_sim_reads, the device-source planner,
ldpc_trial_run_sim): the device form against the numpy
replica synth.dna_raw_reads_hashed byte for byte, and ResidentTrial.run_sim
against run_raw on the replica's reads field by field."""
import functools

import numpy as np
import pytest

import dna_llr
import dna_pipeline as P
import dna_sim_cases as cases
import synth

pytestmark = pytest.mark.gpu
# the keys test_dna_trial_gpu.py compares, and those run_raw adds
KEYS = ("n", "first_success", "second_success", "fail_first", "fail_second", "second_iterations", "first_errors",
        "second_errors", "erasure_index")
RAW_KEYS = ("n_erased_strands", "n_reads_valid", "n_align_pairs", "n_reads_dropped", "cnumerr_hist", "t_index_s",
            "t_align_s", "resident")


def _same(new, old):
    for key in KEYS + RAW_KEYS:
        assert new[key] == old[key], key
    for key in ("hard", "kind", "stats", "iters", "valid"):
        assert np.array_equal(new[key], old[key]), key
    assert P.report(new) == P.report(old)
    assert set(new) - set(old) <= {"n_reads", "seed"} and set(old) <= set(new)


@pytest.mark.parametrize("S,nt", cases.SHAPES)
def test_device_form_equals_replica(gpu, S, nt):
    """L below one wave, exactly one chunk of bases, two chunks with a ragged
    tail, three chunks, seven; with every slot inserting the chunk boundaries
    lie inside the read; 1, 63, 64, 65 and 1000 reads are one block of 4 waves
    cut short, 16 blocks less a wave, exactly 16, one more, and 250."""
    cases.check_form(functools.partial(synth.dna_raw_reads_native, device=0), S, nt)


@pytest.fixture(scope="module")
def strands(codewords):
    return synth.dna_strands(codewords)


@pytest.fixture(scope="module")
def trials(G, codewords):
    """(the handle run_sim uses, the handle run_raw uses), shared by the cases below."""
    return P.ResidentTrial(G, codewords), P.ResidentTrial(G, codewords)


# (seed, reads, (sub, ins, del), max_iter)
MOSTLY_ERASED = (5, 3000, (0.01, 0.0, 0.0), 3)
RAGGED = (6, 20000, (0.0, 0.002, 0.002), 3)
DECODES = (7, 72000, (0.01, 0.0, 0.0), 200)


@pytest.mark.parametrize("case", [MOSTLY_ERASED, RAGGED, DECODES], ids=["erased", "ragged", "decodes"])
def test_run_sim_equals_run_raw(trials, strands, case):
    seed, n, rates, max_iter = case
    Ts, Tr = trials
    raw = synth.dna_raw_reads_hashed(strands, seed, n, *rates)
    (_, _, lens), quals = raw
    assert not ((lens == 16) & (quals > 63)).any()  # (an empty payload with quality > 63 is the planner's error)
    if case is RAGGED:  # on the CPU first: the reads do send strands to the aligner
        plan = dna_llr.plan_llr_native(None, raw[0], quals, host=True)
        assert plan.n_aligned_strands > 0 and plan.n_align_pairs > 0
    new = Ts.run_sim(seed, n, *rates, max_iter=max_iter)
    old = Tr.run_raw(raw, max_iter=max_iter)
    print("run_sim: llr %.4f first %.4f second %.4f s; run_raw: llr %.4f first %.4f second %.4f s" % (
        new["t_llr_s"], new["t_first_s"], new["t_second_s"], old["t_llr_s"], old["t_first_s"], old["t_second_s"]))
    _same(new, old)
    assert np.array_equal(Ts.codes(), Tr.codes())
    assert (new["n_reads"], new["seed"], new["resident"]) == (n, seed, True)
    if case is MOSTLY_ERASED:
        assert new["n_erased_strands"] > Ts.N // 2 and new["first_success"] < 272
    if case is RAGGED:
        assert new["stats"][2] > 0 and new["stats"][3] > 0  # aligned strands, read-to-centre alignments
        assert new["stats"][2] == plan.n_aligned_strands and np.array_equal(new["kind"], plan.kind)
    if case is DECODES:
        assert new["first_success"] == 272 and not new["fail_first"] and np.array_equal(new["hard"], Ts.codewords)


def test_handle_reuse(G, codewords, strands):
    """run_sim with two seeds (the second with fewer reads than the buffers
    hold, and ragged strands), then run_raw, on one handle: each equals a fresh
    handle's result."""
    calls = [lambda T: T.run_sim(21, 4000, 0.01, max_iter=3), lambda T: T.run_sim(22, 2500, 0.0, 0.002, 0.002, max_iter=3),
             lambda T: T.run_raw(synth.dna_raw_reads_hashed(strands, 23, 3000, 0.02), max_iter=3)]
    T = P.ResidentTrial(G, codewords)
    for call in calls:
        got, want = call(T), call(P.ResidentTrial(G, codewords))
        _same(got, want)
        assert got["n_reads_valid"] > 0
    assert calls[1](T)["stats"][2] > 0


def test_coverage_sweep(G, codewords, strands):
    T = P.ResidentTrial(G, codewords)
    counts = [2000, 3000]
    rows = P.coverage_sweep(T, counts, trials=2, seed=40, sub=0.01, ins=0.001, dele=0.001, max_iter=3)
    assert [(r["n_reads"], r["trial"], r["seed"]) for r in rows] == [(2000, 0, 40), (2000, 1, 41), (3000, 0, 40),
                                                                     (3000, 1, 41)]
    alone = P.ResidentTrial(G, codewords)
    for r in rows:
        res = alone.run_sim(r["seed"], r["n_reads"], 0.01, 0.001, 0.001, max_iter=3)
        for key in P.SWEEP_KEYS:
            if not key.startswith("t_"):
                assert r[key] == res[key], key
            else:
                assert r[key] >= 0.0
        assert set(r) == {"n_reads", "trial", "seed", *P.SWEEP_KEYS}
    # within a trial the smaller count's reads are the larger count's first ones
    for seed in (40, 41):
        small = synth.dna_raw_reads_native(strands, seed, 2000, 0.01, 0.001, 0.001, with_strands=True, device=0)
        big = synth.dna_raw_reads_native(strands, seed, 3000, 0.01, 0.001, 0.001, with_strands=True, device=0)
        cases.assert_same_reads(small, big, 2000)


def test_errors_leave_the_handle_usable(G, gpu, codewords, strands):
    mod, lib = dna_llr._lib()
    T = P.ResidentTrial(G, None)  # genie-less: no codewords to make the strands from
    with pytest.raises(gpu.LdpcError, match="no strands set") as e:
        T.run_sim(1, 1000, max_iter=3)
    assert e.value.code == gpu.LDPC_ERR_ARG
    for bad in (strands[:-1], strands[:, :-1], np.where(strands == ord("T"), ord("U"), strands)):
        with pytest.raises(gpu.LdpcError) as e:
            T.set_strands(bad)
        assert e.value.code == gpu.LDPC_ERR_ARG and T.strands is None
    first = T.run_sim(1, 3000, strands=strands, max_iter=3)
    assert first["first_errors"] == {i: -1 for i in first["fail_first"]} and first["n_reads_valid"] > 0
    # bad rates, a bad range and a bad table at the C ABI
    _, _, _, q_val, q_lo = synth.sim_tables(0, 0, 0)
    sidx = np.ascontiguousarray(dna_llr.strand_indices(), np.int32)
    p = dna_llr._p
    one = synth.SIM_ONE
    desc = q_lo[::-1].copy()
    for r0, n, ts, ti, td, ql, nq in ((0, 100, one + 1, 0, 0, q_lo, len(q_lo)), (0, 100, 0, -1, 0, q_lo, len(q_lo)),
                                      (0, 100, one, 0, 1, q_lo, len(q_lo)), (-1, 100, 0, 0, 0, q_lo, len(q_lo)),
                                      (2 ** 40 - 50, 100, 0, 0, 0, q_lo, len(q_lo)), (0, -1, 0, 0, 0, q_lo, len(q_lo)),
                                      (0, 100, 0, 0, 0, desc, len(q_lo)), (0, 100, 0, 0, 0, q_lo, 0)):
        out = P._TrialOut(272, G.N, n_strands=len(sidx))
        rc = lib.ldpc_trial_run_sim(T._h, 1, r0, n, ts, ti, td, p(q_val), p(ql), nq, p(sidx), 1, 0, 0.02, 3, 1, out.ref())
        assert rc == gpu.LDPC_ERR_ARG, (r0, n, ts, ti, td, nq)
        assert b"ldpc_trial_run_sim" in lib.ldpc_last_error()
    with pytest.raises(gpu.LdpcError) as e:
        T.run_sim(1, 3000, max_iter=3, eps=0.6)
    assert e.value.code == gpu.LDPC_ERR_ARG
    with pytest.raises(ValueError):
        T.run_sim(1, 3000, sub=1.5)
    again = T.run_sim(1, 3000, max_iter=3)
    _same(again, first)
    _same(again, P.ResidentTrial(G, None).run_raw(synth.dna_raw_reads_hashed(strands, 1, 3000), max_iter=3))
