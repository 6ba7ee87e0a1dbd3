"""The read planner on the GPU (ldpc_dna_plan: the kernels of
csrc/dna_plan_kernels.hpp) against its host form,
ldpc_dna_plan_host, byte for byte; the fused ldpc_dna_reads_llr against the
existing Python path and the oracle; a full raw trial through it."""
import numpy as np
import pytest

import dna_llr
import dna_plan_cases as cases
import star_ref
import synth
from test_star_align_gpu import E2E, _oracle_arrays

pytestmark = pytest.mark.gpu
NT = dna_llr.PAYLOAD_NT


def _both(index_vals, seqs, quals, strands=None, **kw):
    host = dna_llr.plan_llr_native(index_vals, seqs, quals, host=True, strands=strands)
    dev = dna_llr.plan_llr_native(index_vals, seqs, quals, strands=strands, **kw)
    cases.same_plan(dev, host)
    assert dev.cnumerr_hist == host.cnumerr_hist
    return dev, host


@pytest.mark.parametrize("name", ["edge", "dense"])
def test_device_planner_equals_host(gpu, name):
    idx, seqs, quals, strands = {"edge": cases.edge_input, "dense": cases.dense_input}[name]()
    dev, host = _both(idx, seqs, quals, strands)
    assert host.n_aligned_strands > 0 and host.n_pairs > 0
    if name == "dense":  # twice, the same bytes; and several aligner passes
        again = dna_llr.plan_llr_native(idx, seqs, quals, strands=strands)
        cases.same_plan(again, dev)
        assert np.array_equal(again.rows, dev.rows)
        _both(idx, seqs, quals, strands, workspace_bytes=400000)


def test_device_planner_raw_reads(gpu, codewords):
    seqs, quals = synth.dna_raw_reads(codewords, seed=5, n_reads=1037, sub=0.03, ins=0.002, dele=0.002)
    dev, host = _both(None, seqs, quals)
    assert host.cnumerr_hist[-1] > 0 and sum(host.cnumerr_hist.values()) == 1037


def test_one_strand_many_reads(gpu):
    """300 full-length reads on one strand (more than a workgroup's lanes all
    adding to one counter): rows in input order.  S = 1; then 80 of them with
    a ragged read among them: 3160 pairs and one aligner group of one strand."""
    rng = np.random.default_rng(11)
    parent = "".join(rng.choice(list("ACGT"), NT))
    reads = []
    for _ in range(300):
        r = list(parent)
        r[int(rng.integers(0, NT))] = "ACGT"[int(rng.integers(0, 4))]
        reads.append("".join(r))
    quals = rng.integers(35, 75, 300).tolist()
    dev, host = _both([77] * 300, reads, quals, [77])
    assert dev.kind.tolist() == [1] and dev.row_ptr.tolist() == [0, 300]
    assert [bytes(r).decode() for r in dev.rows] == reads and dev.row_q.tolist() == quals
    reads, quals = reads[:80], quals[:80]
    reads[50] = reads[50][:-2]
    dev, host = _both([77] * 80, reads, quals, [77])
    assert dev.n_pairs == 80 * 79 // 2 and dev.n_align_pairs == 79 and dev.row_q.tolist() == quals
    none = dna_llr.plan_llr_native([], [], [], strands=[77])
    assert none.kind.tolist() == [0] and none.row_ptr.tolist() == [0, 0]


def test_reads_llr_equals_existing_path_and_oracle(gpu):
    import dna_llr_oracle as dorc
    idx, seqs, quals, _ = cases.edge_input()
    old = dna_llr.build_llr(idx, seqs, quals, eps=0.02, align_fn="star")
    new = dna_llr.build_llr(idx, seqs, quals, eps=0.02, align_fn="star", native=True)
    assert np.array_equal(new.llr.view(np.uint64), old.llr.view(np.uint64))
    assert np.array_equal(new.int_mask, old.int_mask) and np.array_equal(new.kind, old.kind)
    assert new.codes is not None and np.array_equal(new.codes, old.codes)
    assert (new.n_reads_valid, new.n_pairs, new.n_aligned_strands, new.n_align_pairs) == \
        (old.n_reads_valid, old.n_pairs, old.n_aligned_strands, old.n_align_pairs)
    by_strand = dorc.build_llr(idx, seqs, quals, dna_llr.strand_indices().tolist(), 0.02, star_ref.star_align)
    llr, mask = _oracle_arrays(by_strand)
    assert np.array_equal(new.llr.view(np.uint64), llr.view(np.uint64))
    assert np.array_equal(new.int_mask, mask)
    assert set(np.unique(new.kind).tolist()) == {0, 1, 2, 3}
    # ldpc_dna_plan + ldpc_dna_llr_codes give the fused call's results
    import ctypes as C
    mod, lib = dna_llr._lib()
    plan = dna_llr.plan_llr_native(idx, seqs, quals)
    S, p = len(plan.kind), dna_llr._p
    llr2, mask2 = np.zeros((2 * NT, S)), np.zeros((2 * NT, S), np.uint8)
    codes2, exact = np.zeros((2 * NT, S), np.int8), C.c_int32(0)
    mod._check(lib.ldpc_dna_llr_codes(S, p(plan.kind), p(plan.row_ptr), p(plan.rows), p(plan.row_q), NT, new.unit,
                                      p(llr2), p(mask2), p(codes2), C.byref(exact), 0))
    assert np.array_equal(plan.kind, new.kind) and exact.value == 1
    assert np.array_equal(llr2.view(np.uint64), new.llr.view(np.uint64))
    assert np.array_equal(mask2, new.int_mask) and np.array_equal(codes2, new.codes)


def test_native_raw_trial(gpu, codewords):
    import dna_pipeline
    raw = synth.dna_raw_reads(codewords, **E2E)
    old = dna_pipeline.trial_from_raw_reads(raw, codewords, eps=0.02, align_fn="star")
    packed = (dna_llr._concat(raw[0]), raw[1])
    new = dna_pipeline.trial_from_raw_reads(packed, codewords, eps=0.02, align_fn="star", native=True)
    print("t_llr_s native", new["t_llr_s"], "python", old["t_index_s"] + old["t_llr_s"])
    assert new["second_success"] == 272 and new["first_success"] == old["first_success"] and not new["fail_second"]
    assert np.array_equal(new["hard"], old["hard"]) and np.array_equal(new["llr"].kind, old["llr"].kind)
    assert new["n_reads_dropped"] == old["n_reads_dropped"] and new["cnumerr_hist"] == old["cnumerr_hist"]
    assert new["t_index_s"] == 0.0 and set(new) == set(old)
    assert new["n_align_pairs"] == old["n_align_pairs"] and new["n_reads_valid"] == old["n_reads_valid"]
    assert np.array_equal(new["llr"].codes, old["llr"].codes)


def test_length_limit(gpu, L):
    rng = np.random.default_rng(2)
    long_read = "".join(rng.choice(list("ACGT"), 801))
    args = ([4, 4, 6], [long_read, long_read[:-3], "ACGT"], [60, 61, 62])
    host = dna_llr.plan_llr_native(*args, host=True, strands=[4, 6])
    assert host.kind.tolist() == [3, 2] and host.n_pairs == 1
    with pytest.raises(L.LdpcError, match="read 0 on a ragged strand is longer than 800") as e:
        dna_llr.plan_llr_native(*args, strands=[4, 6])
    assert e.value.code == L.LDPC_ERR_ARG
    # a long read alone on its strand is no ragged strand
    single = ([4, 6], [long_read, "ACGT"], [60, 62])
    _both(*single, [4, 6])
