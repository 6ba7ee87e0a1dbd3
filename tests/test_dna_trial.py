"""The trial loop in the library on host buffers (ldpc_dna_trial_host,
csrc/dna_trial.hpp) against the Python flow, dna_pipeline.decode_trial, both
with the CPU oracle as their decoder; the tables the second decode is handed
against dna_pipeline.rescale bit for bit; genie-less mode; argument errors."""
import ctypes as C
import hashlib
import math

import numpy as np
import pytest

import dna_llr
import dna_pipeline as P
import synth

EPS = 0.02
UNIT = math.log((1 - EPS) / EPS)
KEYS = ("n", "first_success", "second_success", "fail_first", "fail_second", "second_iterations", "first_errors",
        "second_errors", "erasure_index")


class OracleDecoder:
    """The oracle as decode_trial's decode_fn and as the library's callback.
    Both flows ask for the same decodes: each distinct (LLRs, max_iter) is
    decoded once.  calls: the (codes, table) of every callback."""

    def __init__(self, og):
        self.og, self.memo, self.calls = og, {}, []

    def _decode(self, llr, max_iter):
        key = (hashlib.sha1(np.ascontiguousarray(llr).tobytes()).hexdigest(), llr.shape, max_iter)
        if key not in self.memo:
            h, _, _, v = self.og.decode_batch(llr, max_iter, threads=8, want_post=False)
            self.memo[key] = (h, v)
        h, v = self.memo[key]
        return h.copy(), v.copy()

    def fn(self, llr, max_iter):
        return self._decode(llr, max_iter)[0]

    def cb(self, codes, table, max_iter):
        self.calls.append((codes, table))
        return self._decode(table[codes.astype(np.int64) + 128], max_iter)


@pytest.fixture(scope="module")
def dec(og):
    return OracleDecoder(og)


@pytest.fixture(scope="module")
def dna16(codewords):
    llr = synth.dna_like_llrs(codewords, seed=1, reads=57000)[:16]
    k = synth.dna_like_codes(codewords, seed=1, reads=57000)[:16]
    return llr, k, codewords[:16]


def _same(new, old):
    for key in KEYS:
        assert new[key] == old[key], key
    assert np.array_equal(new["hard"], old["hard"])


class Recorder:
    """decode_trial's decode_fn, keeping every batch it is handed."""

    def __init__(self, dec):
        self.dec, self.batches = dec, []

    def __call__(self, llr, max_iter):
        self.batches.append(llr.copy())
        return self.dec.fn(llr, max_iter)


def _check_tables(calls, codes, batches):
    """Call 0 got the codes and k * unit.  Second-decode call q got
    rescale(code_table(unit), eps, eps2_q) bit for bit, and with it
    table[codes + 128] is the Python flow's q-th batch, the stack of
    rescale(llr_row, eps, eps2_q): the same doubles from the same codes."""
    t0 = P.code_table(UNIT)
    assert len(calls) == len(batches)
    assert np.array_equal(calls[0][1].view(np.uint64), t0.view(np.uint64))
    assert np.array_equal(calls[0][0], codes)
    assert np.array_equal(t0[codes.astype(np.int64) + 128].view(np.uint64), batches[0].view(np.uint64))
    eps2 = EPS - 0.0005
    for (c, t), want in zip(calls[1:], batches[1:]):
        assert np.array_equal(t.view(np.uint64), P.rescale(t0, EPS, eps2).view(np.uint64))
        assert np.array_equal(t[c.astype(np.int64) + 128].view(np.uint64), want.view(np.uint64))
        eps2 = eps2 - 0.0005


def test_host_trial_equals_python_flow(dec, dna16):
    llr, k, cw = dna16
    rec = Recorder(dec)
    old = P.decode_trial(llr, cw, eps=EPS, decode_fn=rec)
    assert old["fail_first"] == [14] and old["second_iterations"] >= 1  # the case exercises the second decode
    dec.calls.clear()
    new = P.decode_trial_host(k, cw, dec.cb, eps=EPS)
    _same(new, old)
    assert new["fail_first"] == [14] and new["second_iterations"] >= 1
    assert np.array_equal(new["valid"], dec.cb(k, P.code_table(UNIT), 200)[1].astype(bool))
    _check_tables(dec.calls[:-1], k, rec.batches)
    assert P.report(new) == P.report(old)


@pytest.mark.parametrize("faithful", [True, False])
def test_host_trial_two_hopeless_rows(dec, dna16, codewords, faithful):
    llr, k, cw = dna16
    bad = synth.bsc_llrs(codewords, 0, 2, seed=5, p=0.03)  # hopeless: never decodes
    llr = np.concatenate([bad, llr[2:]])
    k = np.concatenate([np.where(bad > 0, 1, -1).astype(np.int8), k[2:]])
    rec = Recorder(dec)
    old = P.decode_trial(llr, cw, eps=EPS, decode_fn=rec, max_iter=20, faithful=faithful)
    assert {1, 2} <= set(old["fail_first"]) and old["second_iterations"] >= 2
    dec.calls.clear()
    new = P.decode_trial_host(k, cw, dec.cb, eps=EPS, max_iter=20, faithful=faithful)
    _same(new, old)
    _check_tables(dec.calls, k, rec.batches)
    if faithful:
        assert len(new["fail_second"]) <= 1  # the reference's reset keeps only the last re-decoded row
    else:
        assert set(new["fail_second"]) >= {1, 2}


def test_genie_less_fail_lists_are_the_invalid_rows(dec, dna16):
    llr, k, cw = dna16
    dec.calls.clear()
    res = P.decode_trial_host(k, None, dec.cb, eps=EPS)
    _, valid = dec.cb(k, P.code_table(UNIT), 200)
    invalid = (np.nonzero(valid == 0)[0] + 1).tolist()
    assert res["fail_first"] == invalid and invalid  # row 14 ends with a nonzero syndrome
    assert np.array_equal(res["valid"], valid.astype(bool))
    assert res["first_errors"] == {i: -1 for i in invalid}
    assert set(res["second_errors"]) == set(invalid) and set(res["second_errors"].values()) <= {0, -1}
    # every re-decode's own valid flags decide what fails next: replay them
    fail2 = list(invalid)
    for c, t in dec.calls[1:-1]:
        assert len(c) == len(fail2)
        _, v = dec.cb(c, t, 200)
        fail2 = [fail2[-1]] if not v[-1] else []  # faithful: the last row's outcome survives
    assert res["fail_second"] == fail2
    assert res["first_success"] == 16 - len(invalid) and res["second_success"] == 16 - len(fail2)


def test_callback_exception_is_raised(dna16):
    _, k, cw = dna16

    def boom(codes, table, max_iter):
        raise KeyError("decoder")

    with pytest.raises(KeyError):
        P.decode_trial_host(k, cw, boom)


def test_argument_errors(L, dna16):
    _, k, cw = dna16
    mod, lib = dna_llr._lib()
    k4 = np.ascontiguousarray(k[:2, :8])
    cw4 = np.ascontiguousarray(cw[:2, :8])
    out = P._TrialOut(2, 8)
    cb = dna_llr.TRIAL_DECODE_FN(lambda *a: 0)
    p = dna_llr._p

    def host(codes=p(k4), n_cw=2, N=8, fn=cb, eps=0.02, max_iter=5, res=out.ref()):
        return lib.ldpc_dna_trial_host(codes, n_cw, N, p(cw4), fn, None, eps, max_iter, 1, res)

    assert host() == L.LDPC_OK
    for kw in (dict(codes=None), dict(fn=C.cast(None, dna_llr.TRIAL_DECODE_FN)), dict(res=None), dict(n_cw=0),
               dict(n_cw=-2), dict(N=0), dict(eps=0.0015), dict(eps=0.5), dict(eps=float("nan")), dict(eps=-1.0),
               dict(max_iter=-1)):
        assert host(**kw) == L.LDPC_ERR_ARG, kw
        assert b"ldpc_dna_trial_host" in lib.ldpc_last_error()
    with pytest.raises(ValueError):
        P.decode_trial_host(k4.astype(np.int16), cw4, None)
    with pytest.raises(ValueError):
        P.decode_trial_host(k4, cw[:3, :8], None)
    # the handle: argument errors first, then (no GPU here) LDPC_ERR_DEVICE for good arguments
    G = L.Graph(synth.PCHK)
    err = C.c_int(0)
    cwp = p(np.ascontiguousarray(cw))
    assert not lib.ldpc_trial_create(None, 0, 0, 16, cwp, None, C.byref(err)) and err.value == L.LDPC_ERR_ARG
    assert not lib.ldpc_trial_create(G.handle, 0, 0, 0, cwp, None, C.byref(err)) and err.value == L.LDPC_ERR_ARG
    assert not lib.ldpc_trial_create(G.handle, 0, int(L.ALGO_QMSA), 16, cwp, None, C.byref(err))
    assert err.value == L.LDPC_ERR_ARG
    assert lib.ldpc_trial_run_codes(None, p(k4), 2, 0.02, 5, 1, out.ref()) == L.LDPC_ERR_ARG
    assert lib.ldpc_trial_read_codes(None, p(k4), 2) == L.LDPC_ERR_ARG
    if L.device_count() < 1:
        assert not lib.ldpc_trial_create(G.handle, 0, 0, 16, cwp, None, C.byref(err))
        assert err.value == L.LDPC_ERR_DEVICE
        with pytest.raises(L.LdpcError) as e:
            P.ResidentTrial(G, cw)
        assert e.value.code == L.LDPC_ERR_DEVICE
