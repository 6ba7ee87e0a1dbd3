"""Speculated second decodes on host buffers (ldpc_dna_trial_host_spec,
csrc/dna_trial.hpp): with several eps2 steps per decoder
call the result equals the one-step flow and dna_pipeline.decode_trial in every
field; every callback is handed, bit for bit, the stack of the rescaled rows of
its steps; the number of callbacks and of rows follows the rule, restated here;
the table-space edges (P = 3, 1, 0) and the argument error."""
import hashlib

import numpy as np
import pytest

import dna_pipeline as P
import synth
from test_dna_trial import EPS, KEYS, UNIT, OracleDecoder

SPEC = (-1, 2, 3, 9)


class RowOracle(OracleDecoder):
    """OracleDecoder that remembers per row, not per batch: a speculated batch
    holds rows the one-step flow has decoded already (a codeword's decode does
    not depend on its batch-mates), so each (row, step) is decoded once."""

    def _decode(self, llr, max_iter):
        llr = np.ascontiguousarray(llr)
        keys = [(hashlib.sha1(r.tobytes()).hexdigest(), max_iter) for r in llr]
        todo = sorted({q for q in keys if q not in self.memo}, key=keys.index)
        if todo:
            h, _, _, v = self.og.decode_batch(llr[[keys.index(q) for q in todo]], max_iter, threads=8,
                                              want_post=False)
            for i, q in enumerate(todo):
                self.memo[q] = (h[i].copy(), v[i])
        return (np.stack([self.memo[q][0] for q in keys]),
                np.array([self.memo[q][1] for q in keys], dtype=np.uint8))


@pytest.fixture(scope="module")
def dec(og):
    return RowOracle(og)


@pytest.fixture(scope="module")
def dna16(codewords):
    k = synth.dna_like_codes(codewords, seed=1, reads=57000)[:16]
    return k, codewords[:16]


@pytest.fixture(scope="module")
def hopeless(dna16, codewords):
    """The two hopeless rows of test_dna_trial.py in front of rows 2.. of the 16."""
    k, cw = dna16
    bad = synth.bsc_llrs(codewords, 0, 2, seed=5, p=0.03)
    return np.concatenate([np.where(bad > 0, 1, -1).astype(np.int8), k[2:]]), cw


def eps2_sequence(eps=EPS):
    seq, eps2 = [], eps - 0.0005
    while eps2 > 0.001:
        seq.append(eps2)
        eps2 = eps2 - 0.0005
    return seq


def lanes64(F):
    return 64 * ((F + 63) // 64)


def plan(lists, K, n):
    """The rule over the per-step lists of the one-step run: [(first step, steps, rows)] per decoder call."""
    seq, Pn, out, s = eps2_sequence(), 256 // (2 * K + 1), [], 0
    while s < len(lists):
        F = len(lists[s])
        k = min(len(seq) - s, Pn, lanes64(F) // F)
        if n >= 2:
            k = min(k, n)
        k = max(k, 1)
        out.append((s, k, lists[s]))
        s += k
    return out


def step_lists(k, calls):
    """The rows (0-based) of every second decode of a one-step run, from the codes its callbacks were handed."""
    index = {r.tobytes(): i for i, r in enumerate(k)}
    assert len(index) == len(k)
    return [[index[r.tobytes()] for r in c] for c, _ in calls[1:]]


def run(dec_or_cb, k, cw, n, **kw):
    calls = []
    cb = dec_or_cb.cb if hasattr(dec_or_cb, "cb") else dec_or_cb

    def rec(codes, table, max_iter):
        calls.append((codes, table))
        return cb(codes, table, max_iter)

    return P.decode_trial_host(k, cw, rec, eps=EPS, speculate=n, **kw), calls


def check_speculated(decoder, k, cw, n, base, calls0, **kw):
    """speculate=n against the one-step run (base, calls0): the result, every
    batch's doubles, the counters against the rule.  Returns the result."""
    new, calls = run(decoder, k, cw, n, **kw)
    for key in KEYS:
        assert new[key] == base[key], (n, key)
    assert np.array_equal(new["hard"], base["hard"]) and np.array_equal(new["valid"], base["valid"])
    lists = step_lists(k, calls0)
    assert len(lists) == base["second_iterations"] == base["second_decodes"]
    assert base["second_rows"] == base["second_rows_used"] == sum(len(x) for x in lists)
    K = int(np.abs(k[np.array(base["fail_first"], dtype=np.int64) - 1].astype(np.int32)).max()) if lists else 0
    batches = plan(lists, K, n)
    assert len(calls) - 1 == len(batches) == new["second_decodes"]
    assert new["second_rows"] == sum(kk * len(rows) for _, kk, rows in batches)
    assert new["second_rows_used"] == base["second_rows_used"]
    assert (new["code_absmax"], new["steps_per_decode"]) == ((K, 256 // (2 * K + 1)) if lists else (0, 0))
    seq, t0 = eps2_sequence(), P.code_table(UNIT)
    for (c, t), (s, kk, rows) in zip(calls[1:], batches):
        llr = t0[k[rows].astype(np.int64) + 128]
        want = np.concatenate([P.rescale(llr, EPS, seq[s + j]) for j in range(kk)])
        assert c.shape == want.shape
        assert np.array_equal(t[c.astype(np.int64) + 128].view(np.uint64), want.view(np.uint64)), (n, s, kk)
        if kk == 1:
            assert np.array_equal(t.view(np.uint64), P.rescale(t0, EPS, seq[s]).view(np.uint64))
    return new


def python_flow(dec, k, cw, **kw):
    return P.decode_trial(P.code_table(UNIT)[k.astype(np.int64) + 128], cw, eps=EPS, decode_fn=dec.fn, **kw)


def test_sixteen_codewords(dec, dna16):
    k, cw = dna16
    base, calls0 = run(dec, k, cw, 0)
    old = python_flow(dec, k, cw)
    assert base["fail_first"] == [14] and base["second_iterations"] == 13
    for key in KEYS:
        assert base[key] == old[key], key
    assert np.array_equal(base["hard"], old["hard"])
    for n in SPEC:
        new = check_speculated(dec, k, cw, n, base, calls0)
        if n == -1:
            assert (new["code_absmax"], new["second_decodes"], new["second_rows"]) == (13, 2, 18)
    one, calls1 = run(dec, k, cw, 1)  # 1 is off as 0 is
    assert len(calls1) == len(calls0) and one["second_decodes"] == 13 and one["code_absmax"] == 0


@pytest.mark.parametrize("faithful", [True, False])
def test_two_hopeless_rows(dec, hopeless, faithful):
    k, cw = hopeless
    base, calls0 = run(dec, k, cw, 0, max_iter=20, faithful=faithful)
    old = python_flow(dec, k, cw, max_iter=20, faithful=faithful)
    assert {1, 2} <= set(base["fail_first"]) and base["second_iterations"] == 37
    for key in KEYS:
        assert base[key] == old[key], key
    assert np.array_equal(base["hard"], old["hard"])
    for n in SPEC:
        new = check_speculated(dec, k, cw, n, base, calls0, max_iter=20, faithful=faithful)
        if n == -1:
            assert (new["second_decodes"], new["second_rows"]) == ((5, 73) if faithful else (5, 129))


@pytest.mark.parametrize("faithful", [True, False])
def test_genie_less(dec, dna16, faithful):
    k, _ = dna16
    base, calls0 = run(dec, k, None, 0, faithful=faithful)
    assert base["fail_first"] and base["second_iterations"] >= 1
    for n in SPEC:
        check_speculated(dec, k, None, n, base, calls0, faithful=faithful)


# --- the table-space edges: a tiny matrix and a stub decoder ---------------------------------------------------

def _stub(codes, table, max_iter):
    """hard = the signs of the LLRs; a row whose first two LLRs are negative never decodes."""
    llr = table[codes.astype(np.int64) + 128]
    hard = (llr < 0).astype(np.uint8)
    bad = (llr[:, 0] < 0) & (llr[:, 1] < 0)
    hard[bad, 2] ^= 1
    return hard, (~bad).astype(np.uint8)


def _tiny(m):
    """5 rows of 9 columns of +-m, all different; rows 1 and 3 (0-based) start with two negatives."""
    rng = np.random.default_rng(7)
    s = np.where(rng.integers(0, 2, (5, 9)) == 1, -1, 1)
    s[:, :2] = [[1, 1], [-1, -1], [1, -1], [-1, -1], [-1, 1]]
    s[:, 3] = [1, 1, 1, -1, -1]
    s[:, 4] = [1, -1, 1, 1, -1]
    s[:, 5] = [1, 1, -1, 1, 1]
    k = (s * m).astype(np.int8)
    assert len({r.tobytes() for r in k}) == 5
    return k, (k < 0).astype(np.uint8)


@pytest.mark.parametrize("faithful", [True, False])
@pytest.mark.parametrize("m,P_want", [(42, 3), (127, 1)])
def test_table_space_edges(m, P_want, faithful):
    k, cw = _tiny(m)
    base, calls0 = run(_stub, k, cw, 0, max_iter=5, faithful=faithful)
    assert base["fail_first"] == [2, 4] and base["second_iterations"] == 37
    for n in SPEC:
        new = check_speculated(_stub, k, cw, n, base, calls0, max_iter=5, faithful=faithful)
        assert (new["code_absmax"], new["steps_per_decode"]) == (m, P_want)
        if P_want == 1:
            assert new["second_decodes"] == new["second_iterations"] == 37
    new, _ = run(_stub, k, cw, -1, max_iter=5, faithful=faithful)
    if P_want == 3:  # 12 decodes of 3 steps and one of the last step; faithful drops row 2 after the first step
        assert new["second_decodes"] == 13 and new["second_rows"] == (6 + 34 if faithful else 74)


def test_minus_128_in_a_failing_row():
    k, cw = _tiny(3)
    k[3, 7] = -128 if k[3, 7] < 0 else 127
    k[3, 8] = -128
    cw = (k < 0).astype(np.uint8)
    base, calls0 = run(_stub, k, cw, 0, max_iter=5, faithful=False)
    new = check_speculated(_stub, k, cw, -1, base, calls0, max_iter=5, faithful=False)
    assert (new["code_absmax"], new["steps_per_decode"]) == (128, 0)
    assert new["second_decodes"] == new["second_iterations"] == 37


def test_steps_below_minus_one(L):
    k, cw = _tiny(1)
    with pytest.raises(L.LdpcError) as e:
        P.decode_trial_host(k, cw, _stub, eps=EPS, speculate=-2)
    assert e.value.code == L.LDPC_ERR_ARG
