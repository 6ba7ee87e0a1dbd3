"""The DNA read path on the GPU at payload lengths other than 136 nt: the
device planner against its host form, the LLR and code kernels against the
plain-Python oracle bit for bit, and the resident trial on two small codes
(payloads of 65 and 13 nt) against the Python flow on the oracle's codes.  The
inputs and the yardstick are dna_nt_cases.py's; test_dna_payload_nt.py checks
on the CPU that they hold what these tests need.

Length-dependent device code met here and nowhere else: k_plan_rows' byte
path (nt % 4 != 0) with one trip (1, 13) and two (65), its dword path with one
lane (4) and a second trip (260); k_dna_llr / k_dna_codes with grid.y, the row
stride and the last bit of another nt; the planner's width == nt and l < nt
tests; count-rule codes on the byte paths of the trial kernels (N = 1003)."""
import math

import numpy as np
import pytest

import dna_llr
import dna_nt_cases as nts
import dna_pipeline as P
import dna_plan_cases as cases
from test_dna_sim_gpu import _same as same_sim
from test_dna_trial_gpu import KEYS, _irregular, _python_flow, _same as same_trial
from test_dna_trial_spec_gpu import _same as same_spec

pytestmark = pytest.mark.gpu
NT_IDS = [nt for nt, _ in nts.NTS]
UNIT = math.log((1 - nts.EPS) / nts.EPS)


def _both(index_vals, seqs, quals, strands, nt, **kw):
    host = dna_llr.plan_llr_native(index_vals, seqs, quals, host=True, strands=strands, payload_nt=nt)
    dev = dna_llr.plan_llr_native(index_vals, seqs, quals, strands=strands, payload_nt=nt, **kw)
    cases.same_plan(dev, host)  # kind, row_ptr, rows, row_q and the four counters
    assert dev.cnumerr_hist == host.cnumerr_hist
    assert dev.rows.shape[1] == nt
    return dev, host


@pytest.mark.parametrize("nt", NT_IDS)
def test_device_planner_equals_host(gpu, nt):
    idx, seqs, quals, strands = nts.case(nt)
    dev, host = _both(idx, seqs, quals, strands, nt)
    kind, widths, groups = nts.reference_kinds(nt, nts.case(nt))
    assert np.array_equal(dev.kind, kind) and dev.n_aligned_strands == len(widths) > 0
    if nt == 65:
        # a traceback workspace of 100000 bytes holds one block of 64 read-to-centre pairs of these lengths
        # (64 lanes x 73 rows x 5 words at most), so the aligner takes a pass per block: the same groups
        # through the aligner's own entry report how many
        small = 100000
        passes = dna_llr.star_align_batch([groups[s] for s in sorted(groups)], workspace_bytes=small).n_passes
        assert passes >= 3
        again, _ = _both(idx, seqs, quals, strands, nt, workspace_bytes=small)
        assert np.array_equal(again.rows, dev.rows)


def test_device_planner_raw_reads(gpu):
    seqs, quals, index = nts.raw_case(65)
    dev, host = _both(None, seqs, quals, index, 65)
    assert host.cnumerr_hist[-1] > 0 and sum(host.cnumerr_hist.values()) == len(quals)
    assert host.n_aligned_strands > 0 and set(np.unique(host.kind).tolist()) == {0, 1, 2, 3}
    _both(None, seqs, quals, index, 65, workspace_bytes=100000)


@pytest.mark.parametrize("nt", NT_IDS)
def test_llr_equals_oracle(gpu, nt):
    """ldpc_dna_reads_llr (the device planner and k_dna_llr in one call) and
    the Python planner followed by ldpc_dna_llr_codes, both against the oracle:
    the doubles bit for bit, the int-0 mask, the int8 codes and their table."""
    idx, seqs, quals, strands = nts.case(nt)
    llr, mask, codes = nts.oracle_llr(nt, nts.case(nt))
    kind = nts.reference_kinds(nt, nts.case(nt))[0]
    for native in (True, False):
        got = dna_llr.build_llr(idx, seqs, quals, eps=nts.EPS, align_fn="star", strands=strands, native=native,
                                payload_nt=nt)
        assert got.llr.shape == (2 * nt, len(strands)), native
        assert np.array_equal(got.llr.view(np.uint64), llr.view(np.uint64)), native
        assert np.array_equal(got.int_mask, mask), native
        assert got.codes is not None and np.array_equal(got.codes, codes), native
        assert np.array_equal(got.code_table()[got.codes.astype(np.int64) + 128].view(np.uint64), llr.view(np.uint64))
        assert np.array_equal(got.kind, kind), native


def test_one_strand_many_reads(gpu):
    """300 full-length reads of 65 nt on one strand (more than a workgroup's
    lanes all adding to one counter): rows in input order.  Then 80 of them
    with a ragged read among them: 3160 pairs and one aligner group."""
    nt = 65
    rng = np.random.default_rng(12)
    parent = "".join(rng.choice(list("ACGT"), nt))
    reads = []
    for _ in range(300):
        r = list(parent)
        r[int(rng.integers(0, nt))] = "ACGT"[int(rng.integers(0, 4))]
        reads.append("".join(r))
    quals = rng.integers(35, 75, 300).tolist()
    dev, host = _both([77] * 300, reads, quals, [77], nt)
    assert dev.kind.tolist() == [1] and dev.row_ptr.tolist() == [0, 300]
    assert [bytes(r).decode() for r in dev.rows] == reads and dev.row_q.tolist() == quals
    reads, quals = reads[:80], quals[:80]
    reads[50] = reads[50][:-2]
    dev, host = _both([77] * 80, reads, quals, [77], nt)
    assert dev.n_pairs == 80 * 79 // 2 and dev.n_align_pairs == 79 and dev.row_q.tolist() == quals


# (graph, codewords, channel seed, reads, (sub, ins, del)); every decode runs TRIAL_ITERS = 3 iterations.  With
# the CPU oracle decoder on the oracle's codes the first decode fails rows 49, 77, 90, 91 of the 130 of the
# RS-LDPC code (N = 512, payloads of 65 nt) and rows 2, 4, 5, 7, 8, 11, 12, 13, 15, 16, 18, 20, 21, 22, 23, 25 of
# the 26 of the irregular code (N = 1003, payloads of 13 nt); none of them decodes later, so both trials run all
# 37 second decodes.  Insertions are kept rare: one in a candidate widens the strand's alignment, which then
# counts for its last bit alone.
TRIALS = {"rs": (lambda L: L.Graph.rs_ldpc(5, 16, 4), 130, 3, 2000, (0.01, 0.0003, 0.0007)),
          "irregular": (_irregular, 26, 4, 6000, (0.01, 0.001, 0.003))}
TRIAL_ITERS = 3


@pytest.fixture(scope="module", params=sorted(TRIALS))
def trial(gpu, request):
    make, n_cw, seed, n_reads, rates = TRIALS[request.param]
    G = make(gpu)
    c = nts.trial_case(G, n_cw, seed, n_reads, rates)
    c.update(G=G, seed=seed, n_reads=n_reads, rates=rates,
             T=P.ResidentTrial(G, c["cw"], strands=c["index"]),
             flow=_python_flow(G, c["codes"], c["cw"], TRIAL_ITERS))
    return c


def test_trial_run_raw_equals_python_flow_on_oracle_codes(trial):
    c, T, old = trial, trial["T"], trial["flow"]
    # what the input must make the reference flow do
    assert old["fail_first"] and old["first_success"] >= 1 and old["second_iterations"] >= 1
    assert T.payload_nt == c["nt"] and T.n_cw == 2 * c["nt"]
    host = dna_llr.plan_llr_native(None, *c["raw"], host=True, strands=c["index"], payload_nt=c["nt"])
    assert host.n_aligned_strands > 0 and {1, 3} <= set(np.unique(host.kind).tolist())
    new = T.run_raw(c["raw"], eps=nts.EPS, max_iter=TRIAL_ITERS)
    assert new["resident"] is True
    assert np.array_equal(T.codes(), c["codes"])
    assert np.array_equal(new["kind"], host.kind)
    same_trial(new, old, KEYS)
    assert new["cnumerr_hist"] == c["hist"] == host.cnumerr_hist
    assert (new["n_reads_valid"], new["n_align_pairs"]) == (host.n_reads_valid, host.n_align_pairs)
    # reads whose index is decoded already: the same result
    same_trial(T.run_reads(c["reads"], eps=nts.EPS, max_iter=TRIAL_ITERS), old, KEYS)
    assert np.array_equal(T.codes(), c["codes"])


def test_trial_run_sim_equals_run_raw(trial):
    c, T = trial, trial["T"]
    old = T.run_raw(c["raw"], eps=nts.EPS, max_iter=TRIAL_ITERS)
    Ts = P.ResidentTrial(c["G"], c["cw"], strands=c["index"])
    new = Ts.run_sim(c["seed"], c["n_reads"], *c["rates"], eps=nts.EPS, max_iter=TRIAL_ITERS)
    assert np.array_equal(Ts.strands, c["strands"])  # made from the handle's codewords and index values
    same_sim(new, old)
    assert np.array_equal(Ts.codes(), c["codes"])
    assert (new["n_reads"], new["seed"], new["resident"]) == (c["n_reads"], c["seed"], True)


def test_trial_speculation_changes_nothing(trial):
    c, T = trial, trial["T"]
    off = T.run_raw(c["raw"], eps=nts.EPS, max_iter=TRIAL_ITERS)
    Tn = P.ResidentTrial(c["G"], c["cw"], strands=c["index"], speculate=-1)
    on = Tn.run_raw(c["raw"], eps=nts.EPS, max_iter=TRIAL_ITERS)
    same_spec(on, off)
    assert np.array_equal(on["kind"], off["kind"]) and np.array_equal(Tn.codes(), c["codes"])
    assert on["second_decodes"] < off["second_decodes"] and on["steps_per_decode"] > 1


def test_trial_strands_argument_and_fallback(trial, gpu):
    """A handle of another code without index values refuses the read calls; a
    bad index list is refused at construction; a count difference outside int8
    sends run_raw to the host path at the handle's payload length."""
    c, G = trial, trial["G"]
    bare = P.ResidentTrial(G, c["cw"])
    for call in (lambda: bare.run_raw(c["raw"]), lambda: bare.run_reads(c["reads"]), lambda: bare.run_sim(1, 10)):
        with pytest.raises(ValueError, match="index values"):
            call()
    for bad in (c["index"][:-1], c["index"][::-1], c["index"].astype(np.float64),
                np.concatenate([c["index"][:1], c["index"][:-1]])):
        with pytest.raises(ValueError, match="strictly increasing"):
            P.ResidentTrial(G, c["cw"], strands=bad)
    nt = c["nt"]
    rng = np.random.default_rng(11)
    v = int(c["index"][100])
    parent = "".join(rng.choice(list("ACGT"), nt))
    seqs = [bytes(dna_llr.encode_indices([v])[0]).decode() + parent] * 300
    quals = rng.integers(55, 75, 300).tolist()
    new = c["T"].run_raw((seqs, quals), eps=0.003, max_iter=2)
    assert new["resident"] is False and new["n"] == 2 * nt and new["llr"].codes is None
    llr, mask, _ = nts.oracle_llr(nt, ([v] * 300, [parent] * 300, quals, c["index"]))
    diff = np.rint(llr / UNIT)  # the oracle's matrix is at eps = EPS: +-300 units on strand 100, 0 elsewhere
    assert np.array_equal(new["llr"].int_mask, mask) and np.abs(diff).max() == 300
    assert np.array_equal(new["llr"].llr, diff * math.log((1 - 0.003) / 0.003))
    old = P.decode_trial(new["llr"].llr, c["cw"], eps=0.003, max_iter=2, decode_fn=P.gpu_decode_fn(G))
    same_trial(new, old, KEYS)
