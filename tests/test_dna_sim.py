"""The sequencing channel's host form (ldpc_dna_sim_reads_host,
csrc/dna_sim.hpp) against its numpy replica
synth.dna_raw_reads_hashed, its event rates, and every argument error -- no
GPU.  The replica is written from the definition and does not call the library."""
import ctypes as C
import math

import numpy as np
import pytest

import dna_llr
import dna_sim_cases as cases
import synth


@pytest.mark.parametrize("S,nt", cases.SHAPES)
def test_host_form_equals_replica(S, nt):
    cases.check_form(synth.dna_raw_reads_native, S, nt)


def test_corner_rates_mean_what_they_say():
    S, L = 33, 152
    s = cases.strands(S, L)
    stride = synth.sim_stride(L)
    assert stride == 320 and synth.sim_stride(1) == 16 and synth.sim_stride(399) == 800
    for rt, want_len in zip(cases.RATES, (L, L, None, L, 2 * L + 1, 0)):
        (buf, offs, lens), quals, sof = synth.dna_raw_reads_native(s, 7, 200, *rt, with_strands=True)
        assert np.array_equal(offs, np.arange(200) * stride) and buf.shape == (200 * stride,)
        if want_len is not None:
            assert (lens == want_len).all()
        reads = buf.reshape(200, stride)
        if rt == (0.0, 0.0, 0.0):
            assert np.array_equal(reads[:, :L], s[sof])
        if rt == (1.0, 0.0, 0.0):
            assert (reads[:, :L] != s[sof]).all() and np.isin(reads[:, :L], synth._BASES).all()
        if rt == (0.0, 1.0, 0.0):  # slot p, base p, ..., slot L: the strand sits at the odd positions
            assert np.array_equal(reads[:, 1:2 * L:2], s[sof]) and np.isin(reads[:, :2 * L + 1], synth._BASES).all()


def test_replica_prefix_and_seed():
    S, L = 7, 24
    big = cases.replica(S, L, cases.RATES[2], 0)
    small = synth.dna_raw_reads_hashed(cases.strands(S, L), cases.SEED, 100, *cases.RATES[2], with_strands=True)
    cases.assert_same_reads(small, big, 100)
    other = synth.dna_raw_reads_hashed(cases.strands(S, L), cases.SEED + 1, 100, *cases.RATES[2], with_strands=True)
    assert not np.array_equal(other[2], small[2])


def test_rates():
    """(33, 152), 4000 reads, rates 0.01 / 0.002 / 0.003.  With one rate on at a
    time every event shows: a substituted base always differs from its source
    (mismatches = substitutions), each insertion adds and each deletion removes
    one byte.  An event count is Binomial(m, p), m = 4000 * 152 positions
    (substitution, deletion) or 4000 * 153 slots (insertion): it must lie
    within 6 sigma = 6 * sqrt(m p (1 - p)) of m p.  With all three on, the net
    length change is the difference of two independent such counts.
    Strands: the 4000 strand ids over S = 33 cells give Pearson's chi^2 with 32
    degrees of freedom, mean 32 and variance 2 * 32 = 64; the bound is the mean
    plus 6 standard deviations, 32 + 6 * 8 = 80.  Seeds are fixed."""
    S, L, n = 33, 152, 4000
    s = cases.strands(S, L)
    sub, ins, dele = 0.01, 0.002, 0.003

    def within(count, m, p):
        assert abs(count - m * p) <= 6 * math.sqrt(m * p * (1 - p)), (count, m * p)

    (buf, _, lens), _, sof = synth.dna_raw_reads_native(s, 11, n, sub, 0, 0, with_strands=True)
    assert (lens == L).all()
    within(int((buf.reshape(n, -1)[:, :L] != s[sof]).sum()), n * L, sub)
    (_, _, lens), _ = synth.dna_raw_reads_native(s, 12, n, 0, ins, 0)
    within(int((lens - L).sum()), n * (L + 1), ins)
    assert (lens >= L).all()
    (_, _, lens), _ = synth.dna_raw_reads_native(s, 13, n, 0, 0, dele)
    within(int((L - lens).sum()), n * L, dele)
    assert (lens <= L).all()
    (_, _, lens), quals, sof = synth.dna_raw_reads_native(s, 14, n, sub, ins, dele, with_strands=True)
    net = int((lens - L).sum())
    sigma = math.sqrt(n * (L + 1) * ins * (1 - ins) + n * L * dele * (1 - dele))
    assert abs(net - (n * (L + 1) * ins - n * L * dele)) <= 6 * sigma
    cells = np.bincount(sof, minlength=S)
    assert len(cells) == S
    assert ((cells - n / S) ** 2 / (n / S)).sum() <= 80
    # qualities: every character of the histogram within 6 sigma of its share
    qh = synth.quality_hist()
    for q in np.nonzero(qh)[0]:
        within(int((quals == q).sum()), n, qh[q] / qh.sum())


def test_sim_tables():
    t_sub, t_ins, t_del, q_val, q_lo = synth.sim_tables(0.01, 0.5, 1.0 - 0.01)
    assert (t_sub, t_ins, t_del) == (int(0.01 * 2 ** 53), 2 ** 52, int(0.99 * 2 ** 53))
    qh = synth.quality_hist()
    assert np.array_equal(q_val, np.nonzero(qh)[0]) and q_val.dtype == np.int32 and q_lo.dtype == np.uint32
    assert q_lo[0] == 0 and (np.diff(q_lo.astype(np.int64)) >= 0).all()
    assert synth.sim_tables(0, 0, 0, quality=np.array([0, 3, 0, 1]))[3:][0].tolist() == [1, 3]
    assert synth.sim_tables(0, 0, 0, quality=np.array([0, 3, 0, 1]))[4].tolist() == [0, 3 << 30]
    for bad in ((-0.1, 0, 0), (0, 1.5, 0), (0.6, 0, 0.6)):
        with pytest.raises(ValueError):
            synth.sim_tables(*bad)
    with pytest.raises(ValueError):
        synth.sim_tables(0, 0, 0, quality=np.zeros(5))


def test_argument_errors(L):
    mod, lib = dna_llr._lib()
    s = cases.strands(7, 24).copy()
    _, _, _, q_val, q_lo = synth.sim_tables(0, 0, 0)
    one = synth.SIM_ONE
    good = dict(seed=1, r0=0, n_reads=3, t_sub=0, t_ins=0, t_del=0, q_val=q_val, q_lo=q_lo)

    def call(s=s, **kw):
        a = dict(good, **kw)
        return synth._sim_native(mod, lib, s, a["seed"], a["r0"], a["n_reads"], a["t_sub"], a["t_ins"], a["t_del"],
                                 a["q_val"], a["q_lo"])

    call()
    call(r0=2 ** 40 - 3)  # the last reads the key can hold
    call(t_sub=one - 5, t_del=5, t_ins=one)
    bad_s = s.copy()
    bad_s[6, 23] = ord("N")
    desc = q_lo.copy()
    desc[2] = desc[1] - 1
    first = q_lo.copy()
    first[0] = 1
    for kw in (dict(t_sub=-1), dict(t_ins=-1), dict(t_del=-1), dict(t_sub=one + 1), dict(t_ins=one + 1),
               dict(t_del=one + 1), dict(t_sub=one, t_del=1), dict(n_reads=-1), dict(r0=-1), dict(r0=2 ** 40 - 2),
               dict(r0=2 ** 62), dict(q_val=None), dict(q_lo=None), dict(q_val=q_val[:0], q_lo=q_lo[:0]),
               dict(q_val=np.zeros(257, np.int32), q_lo=np.zeros(257, np.uint32)), dict(q_lo=desc), dict(q_lo=first),
               dict(s=bad_s), dict(s=np.full((3, 400), ord("A"), np.uint8)), dict(s=np.zeros((3, 0), np.uint8))):
        with pytest.raises(mod.LdpcError) as e:
            call(**kw)
        assert e.value.code == mod.LDPC_ERR_ARG, kw
    # null strands and outputs, no strands: straight at the C ABI
    p = dna_llr._p
    buf, lens, quals = np.zeros((3, 64), np.uint8), np.zeros(3, np.int32), np.zeros(3, np.int32)
    head = (7, 24, 1, 0, 3, 0, 0, 0, p(q_val), p(q_lo), len(q_val))
    assert lib.ldpc_dna_sim_reads_host(p(s), *head, p(buf), p(lens), p(quals), None) == mod.LDPC_OK
    for args in ((None, *head, p(buf), p(lens), p(quals), None), (p(s), *head, None, p(lens), p(quals), None),
                 (p(s), *head, p(buf), None, p(quals), None), (p(s), *head, p(buf), p(lens), None, None),
                 (p(s), 0, *head[1:], p(buf), p(lens), p(quals), None)):
        assert lib.ldpc_dna_sim_reads_host(*args) == mod.LDPC_ERR_ARG
        assert b"ldpc_dna_sim_reads_host" in lib.ldpc_last_error()
        # the device form reports the same errors before it looks for a GPU
        assert lib.ldpc_dna_sim_reads(*args, 0) == mod.LDPC_ERR_ARG
    assert [lib.ldpc_dna_sim_stride(v) for v in (0, 1, 152, 399, 400, -3)] == [0, 16, 320, 800, 0, 0]
    # an error leaves the outputs alone
    lens[:] = -7
    assert lib.ldpc_dna_sim_reads_host(p(bad_s), *head, p(buf), p(lens), p(quals), None) == mod.LDPC_ERR_ARG
    assert (lens == -7).all()


def test_trial_entry_points_without_a_handle(L):
    mod, lib = dna_llr._lib()
    s = np.ascontiguousarray(cases.strands(33, 152))
    _, _, _, q_val, q_lo = synth.sim_tables(0, 0, 0)
    p = dna_llr._p
    assert lib.ldpc_trial_set_strands(None, p(s), 33, 152) == mod.LDPC_ERR_ARG
    assert b"ldpc_trial_set_strands" in lib.ldpc_last_error()
    out = dna_llr.TrialResult()
    sidx = np.ascontiguousarray(dna_llr.strand_indices(), np.int32)
    assert lib.ldpc_trial_run_sim(None, 1, 0, 10, 0, 0, 0, p(q_val), p(q_lo), len(q_val), p(sidx), 1, 0, 0.02, 3, 1,
                                  C.byref(out)) == mod.LDPC_ERR_ARG
    assert b"ldpc_trial_run_sim" in lib.ldpc_last_error()
    for bad in (np.zeros(5, np.uint8), np.zeros((2, 3, 4), np.uint8)):
        with pytest.raises(ValueError):
            synth.dna_raw_reads_native(bad, 0, 1)
        with pytest.raises(ValueError):
            synth.dna_raw_reads_hashed(bad, 0, 1)
    with pytest.raises(ValueError):
        synth.dna_raw_reads_hashed(np.full((2, 4), ord("N"), np.uint8), 0, 1)
