"""The DNA read path at payload lengths other than 136 nt, on the CPU: what
the shared inputs of dna_nt_cases.py hold (read off the reference's outputs),
the host planner ldpc_dna_plan_host against the Python planner at every
length, raw reads against split-then-plan, and the default length.  No GPU;
the device kernels meet the same inputs in test_dna_payload_nt_gpu.py."""
import math

import numpy as np
import pytest

import dna_llr
import dna_nt_cases as nts
import dna_plan_cases as cases

NT_IDS = [nt for nt, _ in nts.NTS]


@pytest.mark.parametrize("nt", NT_IDS)
def test_inputs_meet_their_conditions(nt):
    """On the oracle's LLRs and star_ref's alignments, never on the library:
    every kind occurs, strands reach the aligner, some come back at the payload
    length and some do not, and every count difference has an int8 code."""
    case = nts.case(nt)
    kind, widths, _ = nts.reference_kinds(nt, case)
    assert set(np.unique(kind).tolist()) == {0, 1, 2, 3}
    assert len(widths) >= 1
    assert any(w == nt for w in widths.values()) and any(w != nt for w in widths.values())
    llr, mask, codes = nts.oracle_llr(nt, case)
    assert llr.shape == mask.shape == codes.shape == (2 * nt, len(case[3]))
    diff = nts.count_differences(nt, case)
    assert np.abs(diff).max() <= 127 and np.array_equal(codes, diff)
    assert np.array_equal(llr, diff * math.log((1 - nts.EPS) / nts.EPS))
    # the oracle's own view of the kinds: strands without reads or candidates are all int 0, kinds 2 and 3
    # touch the last bit alone, kind 1 leaves no int 0
    assert mask[:, kind == 0].all() and not mask[:, kind == 1][:-1].any()
    assert mask[:-1, (kind == 2) | (kind == 3)].all() and not mask[-1, kind == 3].any()
    print("nt %d: %d strands, %d reads, kinds %s, %d aligned strands (%d at width nt)" % (
        nt, len(kind), len(case[0]), np.bincount(kind, minlength=4).tolist(), len(widths),
        sum(w == nt for w in widths.values())))


@pytest.mark.parametrize("nt", NT_IDS)
def test_host_planner_equals_plan_llr(nt):
    idx, seqs, quals, strands = nts.case(nt)
    got = dna_llr.plan_llr_native(idx, seqs, quals, host=True, strands=strands, payload_nt=nt)
    want = dna_llr.plan_llr(idx, seqs, quals, align_fn="star", align_host=True, distance_fn=cases.levenshtein_pairs,
                            strands=strands, payload_nt=nt)
    cases.same_plan(got, want)
    assert got.rows.shape[1] == nt
    kind, widths, _ = nts.reference_kinds(nt, nts.case(nt))
    assert np.array_equal(got.kind, kind) and got.n_aligned_strands == len(widths)


@pytest.mark.parametrize("nt", [13, 65])
def test_raw_reads_equal_split_then_payload_mode(nt):
    seqs, quals, index = nts.raw_case(nt)
    reads, hist = dna_llr.split_reads_counted(nts.unpacked(seqs), quals.tolist(), host=True)
    assert hist[-1] > 0 and hist[1] > 0 and hist[2] > 0
    want = dna_llr.plan_llr_native(*reads, host=True, strands=index, payload_nt=nt)
    got = dna_llr.plan_llr_native(None, seqs, quals, host=True, strands=index, payload_nt=nt)
    cases.same_plan(got, want)
    assert got.cnumerr_hist == hist and sum(want.cnumerr_hist.values()) == 0
    assert want.n_aligned_strands > 0 and set(np.unique(want.kind).tolist()) == {0, 1, 2, 3}


def test_default_length_is_136():
    """payload_nt omitted: the bytes of payload_nt=136, in the library and in the Python planner."""
    idx, seqs, quals, strands = cases.dense_input()
    a = dna_llr.plan_llr_native(idx, seqs, quals, host=True, strands=strands)
    b = dna_llr.plan_llr_native(idx, seqs, quals, host=True, strands=strands, payload_nt=136)
    cases.same_plan(a, b)
    assert a.rows.tobytes() == b.rows.tobytes() and a.row_q.tobytes() == b.row_q.tobytes()
    assert a.rows.shape[1] == dna_llr.PAYLOAD_NT == 136
    c = dna_llr.plan_llr(idx, seqs, quals, align_fn="star", align_host=True, distance_fn=cases.levenshtein_pairs,
                         strands=strands, payload_nt=136)
    want = cases.reference("dense")  # the same call without the keyword
    cases.same_plan(c, want)
    assert c.rows.tobytes() == want.rows.tobytes() and c.row_q.tobytes() == want.row_q.tobytes()
    with pytest.raises(ValueError, match="payload_nt"):
        dna_llr.plan_llr(idx, seqs, quals, strands=strands, payload_nt=0)
