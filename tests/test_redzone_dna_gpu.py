"""Red zones around the host arrays of the DNA read path's device entry points
(DESIGN.md sec. 9): every output is a poisoned redzone.HostGuard, every input a
guarded copy compared byte for byte afterwards.  The references are the host
forms and replicas the other DNA tests use; every comparison is exact.  Reads
are packed so that the last one ends at the end of its buffer.
"""
import ctypes as C
import math

import numpy as np
import pytest

import dna_llr
import dna_nt_cases as nts
import dna_pipeline as P
import dna_plan_cases as plan_cases
import dna_sim_cases as sc
import redzone as Z
import star_cases
import synth
from test_dna_payload_nt_gpu import TRIAL_ITERS, TRIALS
from test_dna_trial_gpu import KEYS, _python_flow, _same as same_trial

pytestmark = pytest.mark.gpu
UNIT = math.log((1 - nts.EPS) / nts.EPS)


def gin(a, name, shift=0):
    """A guarded copy of an input array."""
    a = np.ascontiguousarray(a)
    return Z.HostGuard(a.shape, a.dtype, shift, data=a, name=name), a


def unchanged(*pairs):
    for g, a in pairs:
        g.check_unchanged(a)


def ok(L, rc):
    assert rc == L.LDPC_OK, (rc, L.lib().ldpc_last_error())


@pytest.fixture(scope="module")
def lib(gpu):
    return dna_llr._lib()[1]


def _raw_reads_list(n=150):
    seqs, quals, index = nts.raw_case(65)
    return nts.unpacked(seqs)[:n], quals[:n], index


# ---------------------------------------------------------------------------
# Levenshtein distances, the index decoder
# ---------------------------------------------------------------------------
def test_edit_distance_red_zones(gpu, lib):
    seqs, _, _ = _raw_reads_list(120)
    rng = np.random.default_rng(5)
    pairs = rng.integers(0, len(seqs), (300, 2)).astype(np.int32)
    want = plan_cases.levenshtein_pairs(seqs, pairs).astype(np.int32)
    Z.nonconstant(want)
    buf, offs, lens = dna_llr._concat(seqs)
    assert offs[-1] + lens[-1] == len(buf)  # the last read ends with the buffer
    ins = [gin(buf, "seqs", 1), gin(offs, "offsets"), gin(lens, "lengths"), gin(pairs[:, 0], "pair_a"),
           gin(pairs[:, 1], "pair_b")]
    dist = Z.HostGuard(len(pairs), np.int32, name="dist")
    ok(gpu, lib.ldpc_dna_edit_distance(*[g.ptr for g, _ in ins[:3]], len(seqs), ins[3][0].ptr, ins[4][0].ptr, len(pairs),
                                       dist.ptr, 0))
    dist.check_bands()
    unchanged(*ins)
    assert np.array_equal(dist.payload(np.int32), want)


def test_index_decode_red_zones(gpu, lib):
    seqs, _, _ = _raw_reads_list(150)
    seqs[7], seqs[-1] = seqs[7][:9], seqs[-1][:16]  # shorter than a prefix; the last read is a prefix alone
    want_i, want_c = dna_llr.decode_indices_host(seqs)
    assert {-1, 0, 1} <= set(np.unique(want_c).tolist())
    Z.nonconstant(want_i)
    buf, offs, lens = dna_llr._concat(seqs)
    assert offs[-1] + lens[-1] == len(buf)
    ins = [gin(buf, "seqs", 3), gin(offs, "offsets"), gin(lens, "lengths")]
    index, cnumerr = Z.HostGuard(len(seqs), np.int32, name="index"), Z.HostGuard(len(seqs), np.int32, name="cnumerr")
    ok(gpu, lib.ldpc_dna_index_decode(*[g.ptr for g, _ in ins], len(seqs), index.ptr, cnumerr.ptr, 0))
    index.check_bands(), cnumerr.check_bands()
    unchanged(*ins)
    assert np.array_equal(index.payload(np.int32), want_i) and np.array_equal(cnumerr.payload(np.int32), want_c)


# ---------------------------------------------------------------------------
# strands
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n_cw,N", [(6, 63), (6, 65), (2, 1), (600, 70), (6, 2561)])
def test_strands_red_zones(gpu, lib, n_cw, N):
    """N x (16 + n_cw / 2) bytes: 63 x 19 and 65 x 19 leave tails after the
    dword stores; 70 x 316 makes two 256-byte chunks per strand; 2561 strands
    are 41 blocks, so 40 places where one block's range ends and the next
    one's begins (the call copies through a device buffer of its own: a store
    past a block's range shows only as a wrong byte of the next block)."""
    rng = np.random.default_rng(n_cw * 1000 + N)
    cw = rng.integers(0, 2, (n_cw, N)).astype(np.uint8)
    index = np.sort(rng.choice(1 << 16, N, replace=False)).astype(np.int32)
    w = 16 + n_cw // 2
    want = np.zeros((N, w), np.uint8)
    ok(gpu, lib.ldpc_dna_strands_host(dna_llr._p(cw), n_cw, N, dna_llr._p(index), dna_llr._p(want)))
    Z.nonconstant(want)
    for shift in (0, 1):
        ins = [gin(cw, "codewords", shift), gin(index, "index")]
        out = Z.HostGuard((N, w), np.uint8, shift, name="out")
        ok(gpu, lib.ldpc_dna_strands(ins[0][0].ptr, n_cw, N, ins[1][0].ptr, out.ptr, 0))
        out.check_bands()
        unchanged(*ins)
        assert np.array_equal(out.payload(np.uint8, (N, w)), want), shift


# ---------------------------------------------------------------------------
# LLRs and codes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nt", [13, 65])
def test_llr_codes_and_reads_llr_red_zones(gpu, lib, nt):
    idx, seqs, quals, strands = nts.case(nt)
    llr, mask, codes = nts.oracle_llr(nt, nts.case(nt))
    Z.nonconstant(llr), Z.nonconstant(mask), Z.nonconstant(codes)
    S = len(strands)
    kind_ref = nts.reference_kinds(nt, nts.case(nt))[0]

    def outputs():
        return [Z.HostGuard((2 * nt, S), np.float64, name="llr"), Z.HostGuard((2 * nt, S), np.uint8, 1, name="int_mask"),
                Z.HostGuard((2 * nt, S), np.int8, 3, name="codes"), Z.HostGuard(1, np.int32, name="codes_exact")]

    def check(outs):
        for g in outs:
            g.check_bands()
        assert np.array_equal(outs[0].payload(np.uint64, (2 * nt, S)), llr.view(np.uint64))
        assert np.array_equal(outs[1].payload(np.uint8, (2 * nt, S)), mask)
        assert np.array_equal(outs[2].payload(np.int8, (2 * nt, S)), codes)
        assert outs[3].payload(np.int32)[0] == 1

    # the host planner's rows through ldpc_dna_llr_codes
    plan = dna_llr.plan_llr_native(idx, seqs, quals, host=True, strands=strands, payload_nt=nt)
    R = int(plan.row_ptr[-1])
    ins = [gin(plan.kind, "kind"), gin(plan.row_ptr, "row_ptr"), gin(plan.rows[:R], "rows", 1), gin(plan.row_q[:R], "row_q")]
    outs = outputs()
    ok(gpu, lib.ldpc_dna_llr_codes(S, *[g.ptr for g, _ in ins], nt, UNIT, *[g.ptr for g in outs], 0))
    check(outs)
    unchanged(*ins)
    # reads to LLRs in one call
    buf, offs, lens, q, iv, sidx, n = dna_llr._native_inputs(idx, seqs, quals, strands)
    assert offs[-1] + lens[-1] == len(buf) or lens[-1] == 0
    ins = [gin(buf, "seqs", 1), gin(offs, "offsets"), gin(lens, "lengths"), gin(q, "quals"), gin(iv, "index_vals"),
           gin(sidx, "strands")]
    outs = outputs()
    kind, stats = Z.HostGuard(S, np.int32, name="kind"), Z.HostGuard(dna_llr.N_PLAN_STATS, np.int64, name="stats")
    p = [g.ptr for g, _ in ins]
    ok(gpu, lib.ldpc_dna_reads_llr(*p[:4], n, p[4], p[5], S, nt, 1, 0, 0, UNIT, *[g.ptr for g in outs], kind.ptr,
                                   stats.ptr))
    check(outs)
    kind.check_bands(), stats.check_bands()
    unchanged(*ins)
    assert np.array_equal(kind.payload(np.int32), kind_ref)


# ---------------------------------------------------------------------------
# the planner: rows from R on are not touched
# ---------------------------------------------------------------------------
def _plan_inputs(which):
    if which == "edge":
        idx, seqs, quals, strands = plan_cases.edge_input()
        return idx, seqs, quals, strands, dna_llr.PAYLOAD_NT
    return (*nts.case(13), 13)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("which", ["edge", "nt13"])
def test_plan_red_zones(gpu, lib, which):
    idx, seqs, quals, strands, nt = _plan_inputs(which)
    host = dna_llr.plan_llr_native(idx, seqs, quals, host=True, strands=strands, payload_nt=nt)
    buf, offs, lens, q, iv, sidx, n = dna_llr._native_inputs(idx, seqs, quals, strands)
    S, R = len(sidx), int(host.row_ptr[-1])
    assert 0 < R < n  # rows the call must leave alone exist
    Z.nonconstant(host.rows[:R]), Z.nonconstant(host.row_q[:R]), Z.nonconstant(host.kind)
    ins = [gin(buf, "seqs", 1), gin(offs, "offsets"), gin(lens, "lengths"), gin(q, "quals"), gin(iv, "index_vals"),
           gin(sidx, "strands")]
    kind, row_ptr = Z.HostGuard(S, np.int32, name="kind"), Z.HostGuard(S + 1, np.int64, name="row_ptr")
    rows, row_q = Z.HostGuard((n, nt), np.uint8, 1, name="rows"), Z.HostGuard(n, np.int32, name="row_q")
    stats = Z.HostGuard(dna_llr.N_PLAN_STATS, np.int64, name="stats")
    p = [g.ptr for g, _ in ins]
    ok(gpu, lib.ldpc_dna_plan(*p[:4], n, p[4], p[5], S, nt, 1, 0, 0, kind.ptr, row_ptr.ptr, rows.ptr, row_q.ptr,
                              stats.ptr))
    for g in (kind, row_ptr, rows, row_q, stats):
        g.check_bands()
    unchanged(*ins)
    assert np.array_equal(kind.payload(np.int32), host.kind) and np.array_equal(row_ptr.payload(np.int64), host.row_ptr)
    assert np.array_equal(rows.payload(np.uint8, (n, nt))[:R], host.rows[:R])
    assert np.array_equal(row_q.payload(np.int32)[:R], host.row_q[:R])
    rows.check_poison(R * nt)   # "rows from R on are not touched"
    row_q.check_poison(R * 4)
    assert stats.payload(np.int64)[4] == R


# ---------------------------------------------------------------------------
# the aligner: exact capacity, one byte short, several passes
# ---------------------------------------------------------------------------
@pytest.mark.timeout(120)
def test_star_align_red_zones(gpu, lib):
    groups = star_cases.random_groups()
    ref = dna_llr.star_align_batch(groups, host=True)
    needed = len(ref.out)
    Z.nonconstant(ref.out), Z.nonconstant(ref.dist), Z.nonconstant(ref.width)
    reads = [s for g in groups for s in g]
    buf, offs, lens = dna_llr._concat(reads)
    G, n = len(groups), len(reads)
    for capacity, workspace in ((needed, 0), (needed - 1, 0), (needed, 400000)):
        ins = [gin(buf, "seqs", 1), gin(offs, "offsets"), gin(lens, "lengths"), gin(ref.group_ptr, "group_ptr")]
        center, width = Z.HostGuard(G, np.int32, name="center"), Z.HostGuard(G, np.int32, name="width")
        out_ptr, dist = Z.HostGuard(G + 1, np.int64, name="out_ptr"), Z.HostGuard(n, np.int32, name="dist")
        out = Z.HostGuard(capacity, np.uint8, 1, name="out")
        need, stats = Z.HostGuard(1, np.int64, name="out_needed"), Z.HostGuard(3, np.int64, name="stats")
        p = [g.ptr for g, _ in ins]
        rc = lib.ldpc_dna_star_align(*p[:3], n, p[3], G, center.ptr, width.ptr, out_ptr.ptr, out.ptr, capacity, need.ptr,
                                     dist.ptr, 0, workspace, stats.ptr)
        for g in (center, width, out_ptr, dist, out, need, stats):
            g.check_bands()
        unchanged(*ins)
        assert need.payload(np.int64)[0] == needed
        assert np.array_equal(center.payload(np.int32), ref.center) and np.array_equal(width.payload(np.int32), ref.width)
        assert np.array_equal(out_ptr.payload(np.int64), ref.out_ptr) and np.array_equal(dist.payload(np.int32), ref.dist)
        if capacity < needed:
            assert rc == gpu.LDPC_ERR_ARG
            out.check_poison()  # "no row written"
        else:
            ok(gpu, rc)
            assert np.array_equal(out.payload(), ref.out)
            assert (stats.payload(np.int64)[1] > 1) == (workspace != 0)  # the small workspace splits the pairs into passes


# ---------------------------------------------------------------------------
# the sequencing channel
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("S,nt", sc.SHAPES)
def test_sim_reads_red_zones(gpu, lib, S, nt):
    """Every store stays inside the read's slot: with every slot inserting
    (length 2 nt + 1) and with all three error kinds, 65 reads."""
    mod = gpu
    s = sc.strands(S, nt)
    stride = int(lib.ldpc_dna_sim_stride(nt))
    n = 65
    for rates in ((0.05, 0.05, 0.05), (0.0, 1.0, 0.0)):
        want = sc.replica(S, nt, rates, 0)
        Z.nonconstant(want[0][0][:n * stride])
        t_sub, t_ins, t_del, q_val, q_lo = synth.sim_tables(*rates)
        ins = [gin(s, "strands", 1), gin(q_val, "q_val"), gin(q_lo, "q_lo")]
        reads = Z.HostGuard(n * stride, np.uint8, name="reads")
        lengths, quals = Z.HostGuard(n, np.int32, name="lengths"), Z.HostGuard(n, np.int32, name="quals")
        strand_of = Z.HostGuard(n, np.int32, name="strand_of")
        ok(mod, lib.ldpc_dna_sim_reads(ins[0][0].ptr, S, nt, C.c_uint64(sc.SEED), 0, n, t_sub, t_ins, t_del, ins[1][0].ptr,
                                       ins[2][0].ptr, len(q_val), reads.ptr, lengths.ptr, quals.ptr, strand_of.ptr, 0))
        for g in (reads, lengths, quals, strand_of):
            g.check_bands()
        unchanged(*ins)
        got = ((reads.payload(), np.arange(n, dtype=np.int64) * stride, lengths.payload(np.int32)),
               quals.payload(np.int32), strand_of.payload(np.int32))
        sc.assert_same_reads(got, want, n)
        if rates[1] == 1.0:
            assert (got[0][2] == 2 * nt + 1).all()


# ---------------------------------------------------------------------------
# the resident trial: every array of ldpc_trial_result at its documented size
# ---------------------------------------------------------------------------
class GuardedTrialOut(P._TrialOut):
    """dna_pipeline._TrialOut with every array a poisoned HostGuard."""

    def __init__(self, n_cw, N, n_strands=0):
        super().__init__(n_cw, N, n_strands)
        self.guards = {}
        for k, v in list(self.a.items()):
            g = self.guards[k] = Z.HostGuard(v.shape, v.dtype, name=k)
            self.a[k] = g.view
            setattr(self.r, k, g.ptr.value)

    def check_bands(self):
        for g in self.guards.values():
            g.check_bands()


@pytest.fixture(scope="module")
def trial(gpu):
    make, n_cw, seed, n_reads, rates = TRIALS["rs"]
    G = make(gpu)
    c = nts.trial_case(G, n_cw, seed, n_reads, rates)
    c.update(G=G, flow=_python_flow(G, c["codes"], c["cw"], TRIAL_ITERS))
    return c


@pytest.mark.timeout(120)
@pytest.mark.parametrize("speculate", [0, -1])
def test_trial_red_zones(gpu, lib, trial, speculate):
    """RS-LDPC (5,16,4) x 130 codewords (payloads of 65 nt): ldpc_trial_run_codes
    and ldpc_trial_run_reads into guarded result arrays, after a decoy run of
    the handle on the codes shifted by one row."""
    c, old = trial, trial["flow"]
    assert old["fail_first"] and old["first_success"] >= 1 and old["second_iterations"] >= 1
    n_cw, N = c["codes"].shape
    T = P.ResidentTrial(c["G"], c["cw"], strands=c["index"], speculate=speculate)
    decoy = np.ascontiguousarray(np.roll(c["codes"], 1, axis=0))
    try:
        T.run_codes(decoy, eps=nts.EPS, max_iter=TRIAL_ITERS)
        codes, raw = gin(c["codes"], "codes", 1)
        out = GuardedTrialOut(n_cw, N)
        ok(gpu, lib.ldpc_trial_run_codes(T._h, codes.ptr, n_cw, nts.EPS, TRIAL_ITERS, 1, out.ref()))
        out.check_bands()
        codes.check_unchanged(raw)
        same_trial(out.result(), old, KEYS)
        # reads whose index is decoded already, after the decoy again
        T.run_codes(decoy, eps=nts.EPS, max_iter=TRIAL_ITERS)
        buf, offs, lens, q, iv, sidx, n = dna_llr._native_inputs(*c["reads"], c["index"])
        ins = [gin(buf, "seqs", 1), gin(offs, "offsets"), gin(lens, "lengths"), gin(q, "quals"), gin(iv, "index_vals"),
               gin(sidx, "strands")]
        out = GuardedTrialOut(n_cw, N, n_strands=N)
        p = [g.ptr for g, _ in ins]
        ok(gpu, lib.ldpc_trial_run_reads(T._h, *p[:4], n, p[4], p[5], N, c["nt"], 1, 0, nts.EPS, TRIAL_ITERS, 1, out.ref()))
        out.check_bands()
        unchanged(*ins)
        same_trial(out.result(), old, KEYS)
        assert np.array_equal(T.codes(), c["codes"])
        host = dna_llr.plan_llr_native(*c["reads"], host=True, strands=c["index"], payload_nt=c["nt"])
        assert np.array_equal(out.a["kind"], host.kind)
    finally:
        T.close()
