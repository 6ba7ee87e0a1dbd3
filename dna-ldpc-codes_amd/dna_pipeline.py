"""In-process LDPC stage of the DNA-storage decoder.

Reproduces the decode loop of the reference's ex_decoder/decoder.py without
the 272+ `ldpc.exe` processes and soft/dec text files:

* first decode (decoder.py:553-581): every codeword's LLR vector decoded with
  max_iter 200; the genie check against the true codeword gives `fail_DNA`
  (1-based indices) and the per-strand `re_decode` counts (output bit !=
  input hard decision), from which `erasure_index` = strands with > 140
  (decoder.py:590, def_func.re_index);
* second decode (decoder.py:592-664): while failures remain and eps2 > 0.001,
  rescale the ORIGINAL LLRs of the failed codewords by
  ``(x * ln((1-eps2+0.0005)/(eps2-0.0005))) / ln((1-eps)/eps)`` (zeros kept),
  lower eps2 by 0.0005 and re-decode.  The reference resets ``fail_DNA2 = []``
  inside its per-codeword loop (decoder.py:659-661), so only the LAST re-decoded
  codeword's outcome survives an iteration; this module keeps that behaviour
  (``faithful=True``, the default) or tracks every failure (``faithful=False``).

All decodes of one stage go to the GPU in ONE batched call.  `decode_fn` is
injectable so tests can run the identical flow on the CPU oracle.

The first decode's LLRs are count differences times ln((1-eps)/eps)
(decoder.py:314): when the caller has them as int8 codes (dna_llr's
LlrResult.codes, made by the LLR kernel itself), the GPU decode_fn takes the
codes and the 256-entry table k * unit (Graph.decode_codes) -- the same
doubles, without the host lattice pass over the fp64 matrix that the fp64
entry needs.  The second decode's rescaled LLRs are off that lattice, but each
is still a function of its code alone: the rescaled input of a failed codeword
is its same codes with the 256-entry table rescale(code_table(unit), eps,
eps2).  decode_trial keeps sending them through the fp64 entry; the library's
trial (ResidentTrial, decode_trial_host; csrc/dna_trial.hpp, DESIGN.md sec.
8.8) decodes every stage from the one int8 matrix, which then never leaves the
device.
"""
from __future__ import annotations

import math
import time
from typing import Callable, Dict, List, Optional

import numpy as np

DecodeFn = Callable[[np.ndarray, int], np.ndarray]  # (llr [B][N], max_iter) -> hard [B][N]
# optional attribute `codes` of a DecodeFn: (codes int8 [B][N], table [256], max_iter) -> hard [B][N],
# the decode of llr = table[codes + 128]


def code_table(unit: float) -> np.ndarray:
    """table[k + 128] = k * unit: the doubles (count_0 - count_1) * unit of decoder.py:314."""
    return np.arange(-128, 128, dtype=np.float64) * unit


def gpu_decode_fn(graph=None, algo="bp") -> DecodeFn:
    import ldpc_amd
    g = graph if graph is not None else ldpc_amd.graph(ldpc_amd.default_pchk())

    def fn(llr: np.ndarray, max_iter: int) -> np.ndarray:
        hard, _, _, _ = g.decode(llr, max_iter=max_iter, algo=algo, post=None)
        return hard

    def codes(k: np.ndarray, table: np.ndarray, max_iter: int) -> np.ndarray:
        hard, _, _, _ = g.decode_codes(k, table, max_iter=max_iter, algo=algo, post=None)
        return hard

    fn.codes = codes
    return fn


def rescale(llr: np.ndarray, eps: float, eps2: float) -> np.ndarray:
    """decoder.py:603-609: x -> x * ln((1-eps2+.0005)/(eps2-.0005)) / ln((1-eps)/eps), 0 kept."""
    num = math.log((1 - eps2 + 0.0005) / (eps2 - 0.0005))
    den = math.log((1 - eps) / eps)
    return np.where(llr == 0, llr, (llr * num) / den)


def decode_trial(llr: np.ndarray, codewords: np.ndarray, eps: float = 0.02, max_iter: int = 200,
                 decode_fn: Optional[DecodeFn] = None, faithful: bool = True,
                 codes: Optional[np.ndarray] = None) -> Dict:
    """Run the LDPC part of one decoder.py trial.  llr: [n_cw][N] (row i = soft
    file i+1), codewords: [n_cw][N] true codewords (the genie).  codes
    (optional, int8 [n_cw][N]): the count differences with llr == codes *
    ln((1-eps)/eps) exactly, as the producer guarantees (dna_llr.build_llr);
    a decode_fn with a `codes` attribute then decodes them for the first
    decode."""
    decode_fn = decode_fn or gpu_decode_fn()
    llr = np.ascontiguousarray(llr, dtype=np.float64)
    n_cw, N = llr.shape
    t0 = time.perf_counter()
    if codes is not None and hasattr(decode_fn, "codes"):
        if codes.shape != llr.shape or codes.dtype != np.int8:
            raise ValueError("codes must be int8 with the shape of llr")
        hard = decode_fn.codes(codes, code_table(math.log((1 - eps) / eps)), max_iter)
    else:
        hard = decode_fn(llr, max_iter)
    t_first = time.perf_counter() - t0
    errors = (hard != codewords).sum(axis=1)
    fail = [i + 1 for i in range(n_cw) if errors[i] != 0]
    re_decode = (hard != (llr < 0)).sum(axis=0)  # decoder.py:565-574
    erasure_index = [j for j in range(N) if re_decode[j] > 140]

    fail2: List[int] = list(fail)
    iter_sec = 0
    eps2 = eps - 0.0005
    second_errors = {}
    t1 = time.perf_counter()
    while fail2 and eps2 > 0.001:
        iter_sec += 1
        batch = np.stack([rescale(llr[i - 1], eps, eps2) for i in fail2])
        eps2 = eps2 - 0.0005
        h2 = decode_fn(batch, max_iter)
        new: List[int] = []
        for k, i in enumerate(fail2):
            v = int((h2[k] != codewords[i - 1]).sum())
            second_errors[i] = v
            if faithful:
                new = []  # decoder.py:659-661 resets the list per codeword
            if v != 0:
                new.append(i)
            if v == 0:
                hard[i - 1] = h2[k]
        fail2 = new
    t_second = time.perf_counter() - t1
    return {
        "first_success": n_cw - len(fail), "second_success": n_cw - len(fail2), "n": n_cw,
        "fail_first": fail, "fail_second": fail2, "second_iterations": iter_sec,
        "first_errors": {i: int(errors[i - 1]) for i in fail}, "second_errors": second_errors,
        "erasure_index": erasure_index, "hard": hard, "t_first_s": t_first, "t_second_s": t_second,
    }


def _finish_trial(built, t_llr, codewords, eps, max_iter, decode_fn, faithful) -> Dict:
    res = decode_trial(built.llr, codewords, eps=eps, max_iter=max_iter, decode_fn=decode_fn, faithful=faithful,
                       codes=built.codes)
    res.update(t_llr_s=t_llr, n_erased_strands=int(len(built.erased)), n_reads_valid=built.n_reads_valid,
               n_align_pairs=built.n_align_pairs, t_align_s=built.t_align_s, llr=built)
    return res


def trial_from_reads(reads, codewords: np.ndarray, eps: float = 0.02, max_iter: int = 200, align_fn=None,
                     decode_fn: Optional[DecodeFn] = None, faithful: bool = True, device: int = 0,
                     native: bool = False, strands=None, payload_nt: Optional[int] = None) -> Dict:
    """decoder.py:120-664 for one trial: reads (index values, payloads,
    qualities) -> LLRs on the GPU (dna_llr.build_llr) -> first and second
    decode.  align_fn: "star" (the built-in aligner, on the GPU) or a
    callable.  Adds the LLR stage's time and strand statistics to the result,
    the aligner's share among them (n_align_pairs, t_align_s).  native=True:
    the planner runs in the library as well (build_llr(native=True)).
    strands, payload_nt: the strand index values and the payload length of
    another code than the DNA file's (build_llr's defaults otherwise)."""
    import dna_llr
    nt = dna_llr.PAYLOAD_NT if payload_nt is None else int(payload_nt)
    t0 = time.perf_counter()
    built = dna_llr.build_llr(*reads, eps=eps, align_fn=align_fn, device=device, native=native, strands=strands,
                              payload_nt=nt)
    t_llr = time.perf_counter() - t0
    return _finish_trial(built, t_llr, codewords, eps, max_iter, decode_fn, faithful)


def read_trial_files(directory: str, rs: int, trial: int):
    """(raw_seqs, quals) of one trial's <rs>_RS_<trial>.txt and
    <rs>_RS_Q_<trial>.txt (decoder.py:48-54, :90; def_func.file_read): one
    read per line with the '\\n' stripped, quality = ord of the line's
    character."""
    import os

    def lines(name):
        with open(os.path.join(directory, name), "r") as f:
            return [ln.strip("\n") for ln in f]

    seqs = lines("%d_RS_%d.txt" % (rs, trial))
    qual = lines("%d_RS_Q_%d.txt" % (rs, trial))
    if len(seqs) != len(qual):
        raise ValueError(f"{len(seqs)} reads but {len(qual)} qualities")
    return seqs, [ord(q) for q in qual]  # ord() of a line that is not one character raises, as in the reference


def trial_from_raw_reads(raw_reads, codewords: np.ndarray, eps: float = 0.02, max_iter: int = 200, align_fn=None,
                         decode_fn: Optional[DecodeFn] = None, faithful: bool = True, device: int = 0,
                         host_index: bool = False, native: bool = False, strands=None,
                         payload_nt: Optional[int] = None) -> Dict:
    """decoder.py:59-664 for one trial: raw reads (sequences, qualities) ->
    index decode on the GPU (dna_llr.split_reads; host_index=True: on the CPU)
    -> trial_from_reads.  Adds the index stage's time, the number of reads it
    dropped and the histogram of cnumerr.  native=True: the raw reads (a list
    of str or a packed (buf, offsets, lengths) triple) go straight to
    ldpc_dna_reads_llr -- index decode, planner and LLRs in one library call, so
    t_index_s is 0.0 and its time is part of t_llr_s.  strands, payload_nt: as
    in trial_from_reads."""
    import dna_llr
    nt = dna_llr.PAYLOAD_NT if payload_nt is None else int(payload_nt)
    if native:
        seqs, quals = raw_reads
        t0 = time.perf_counter()
        built, hist = dna_llr.build_llr_native(None, seqs, quals, eps=eps, align=dna_llr._native_align(align_fn),
                                               device=device, strands=strands, payload_nt=nt)
        res = _finish_trial(built, time.perf_counter() - t0, codewords, eps, max_iter, decode_fn, faithful)
        res.update(t_index_s=0.0, n_reads_dropped=hist[-1], cnumerr_hist=hist)
        return res
    t0 = time.perf_counter()
    reads, hist = dna_llr.split_reads_counted(*raw_reads, device=device, host=host_index)
    t_index = time.perf_counter() - t0
    res = trial_from_reads(reads, codewords, eps=eps, max_iter=max_iter, align_fn=align_fn, decode_fn=decode_fn,
                           faithful=faithful, device=device, strands=strands, payload_nt=nt)
    res.update(t_index_s=t_index, n_reads_dropped=hist[-1], cnumerr_hist=hist)
    return res


class _TrialOut:
    """The caller-owned arrays of one ldpc_trial_result and the dict made of them."""

    def __init__(self, n_cw: int, N: int, n_strands: int = 0):
        import ctypes as C

        import dna_llr
        self.n_cw, self.N = n_cw, N
        self.a = {k: np.zeros(n_cw, np.int32) for k in ("fail_first", "fail_second", "first_errors", "second_errors",
                                                        "iters")}
        self.a.update(erasure_index=np.zeros(N, np.int32), hard=np.zeros((n_cw, N), np.uint8),
                      valid=np.zeros(n_cw, np.uint8))
        if n_strands:
            self.a.update(kind=np.zeros(n_strands, np.int32), stats=np.zeros(dna_llr.N_PLAN_STATS, np.int64))
        self.r = dna_llr.TrialResult()
        for k, v in self.a.items():
            setattr(self.r, k, v.ctypes.data_as(C.c_void_p))

    def ref(self):
        import ctypes as C
        return C.byref(self.r)

    def result(self) -> Dict:
        r, a, n = self.r, self.a, self.r.n
        fail = a["fail_first"][:r.n_fail_first].tolist()
        return {
            "first_success": r.first_success, "second_success": r.second_success, "n": n,
            "fail_first": fail, "fail_second": a["fail_second"][:r.n_fail_second].tolist(),
            "second_iterations": r.second_iterations,
            "first_errors": {i: int(a["first_errors"][i - 1]) for i in fail},
            "second_errors": {i + 1: int(v) for i, v in enumerate(a["second_errors"][:n]) if v != -2},
            "erasure_index": a["erasure_index"][:r.n_erasure].tolist(), "hard": a["hard"][:n],
            "t_first_s": r.t_first_s, "t_second_s": r.t_second_s,
            "iters": a["iters"][:n], "valid": a["valid"][:n].astype(bool),
        }


def decode_trial_host(codes: np.ndarray, codewords: Optional[np.ndarray], decode_cb, eps: float = 0.02,
                      max_iter: int = 200, faithful: bool = True, speculate: int = 0) -> Dict:
    """decode_trial in the library on host buffers (ldpc_dna_trial_host,
    csrc/dna_trial.hpp): codes int8 [n_cw][N] are the whole input, every decode
    goes to decode_cb(codes [B][N], table [256], max_iter) -> (hard [B][N],
    valid [B]), the decode of table[codes + 128].  codewords None: genie-less
    (a row fails iff its valid flag is 0; its error count reads -1).  The
    result has decode_trial's keys (plus valid; iters is not reported by a
    callback and reads 0), and the counters second_decodes, second_rows,
    second_rows_used, code_absmax, steps_per_decode.  speculate (DESIGN.md
    sec. 8.10; ldpc_dna_trial_host_spec): 0 or 1 one eps2 step per callback,
    n >= 2 at most n, -1 as many as fit -- the callback then sees the failed
    rows once per step, their codes shifted into that step's slice of the
    packed table; the result is the same in every other key."""
    import ctypes as C

    import dna_llr
    mod, L = dna_llr._lib()
    k = np.ascontiguousarray(codes)
    if k.dtype != np.int8 or k.ndim != 2:
        raise ValueError("codes must be int8 [n_cw][N]")
    n_cw, N = k.shape
    cw = None
    if codewords is not None:
        cw = np.ascontiguousarray(codewords, np.uint8)
        if cw.shape != k.shape:
            raise ValueError("codewords must have the shape of codes")
    raised = []

    def cb(_user, p_codes, p_table, B, it, p_hard, p_valid):
        try:
            c = np.ctypeslib.as_array(p_codes, shape=(B, N))
            t = np.ctypeslib.as_array(p_table, shape=(256,))
            hard, valid = decode_cb(c.copy(), t.copy(), int(it))
            np.ctypeslib.as_array(p_hard, shape=(B, N))[:] = hard
            np.ctypeslib.as_array(p_valid, shape=(B,))[:] = valid
            return 0
        except BaseException as e:  # noqa: BLE001 -- no exception may cross the C frames
            raised.append(e)
            return mod.LDPC_ERR_ARG

    out = _TrialOut(n_cw, N)
    cnt = dna_llr.TrialCounters()
    rc = L.ldpc_dna_trial_host_spec(dna_llr._p(k), n_cw, N, None if cw is None else dna_llr._p(cw),
                                    dna_llr.TRIAL_DECODE_FN(cb), None, float(eps), int(max_iter),
                                    int(bool(faithful)), out.ref(), int(speculate), C.byref(cnt))
    if raised:
        raise raised[0]
    mod._check(rc)
    res = out.result()
    res.update(cnt.as_dict())
    return res


class ResidentTrial:
    """A trial whose decoder input stays on the GPU (ldpc_trial_*, DESIGN.md
    sec. 8.8): one engine, the true codewords, the int8 code matrix and the
    buffers of both decodes live in the handle and are reused by every run.
    codewords None: genie-less (a codeword fails iff its syndrome at exit is
    not zero; error counts read -1).

        T = ResidentTrial(graph, codewords)
        res = T.run_raw((seqs, quals))          # keys of trial_from_raw_reads(native=True)
        res = T.run_codes(codes)                # keys of decode_trial
        print(report(res))

    The times in the result (t_llr_s, t_first_s, t_second_s) are the library's
    own, returned in ldpc_trial_result.

    speculate (set_speculation): 0 or 1 one eps2 step per
    second decode, n >= 2 at most n, -1 as many as fit in the tiles the failed
    rows occupy anyway.  Every run of the handle uses the setting; the result
    differs only in the counters second_decodes, second_rows, second_rows_used,
    code_absmax and steps_per_decode, which every resident result carries.

    The read calls (run_reads, run_raw, run_sim) take the payload length from
    the handle, n_cw // 2 nucleotides, and the strand index values from
    `strands`: N strictly increasing ints, dna_llr.strand_indices() by default
    when N is the DNA file's 18432; a handle of another code needs them."""

    def __init__(self, graph, codewords: Optional[np.ndarray] = None, algo="bp", device: int = 0,
                 n_cw: Optional[int] = None, schedule=None, speculate: int = 0, strands=None):
        import ctypes as C

        import dna_llr
        import ldpc_amd
        self._mod, self._L = dna_llr._lib()
        self.graph, self.device, self.algo = graph, device, ldpc_amd._algo(algo)
        self.codewords = None
        if codewords is not None:
            self.codewords = np.ascontiguousarray(codewords, np.uint8)
            if self.codewords.ndim != 2 or self.codewords.shape[1] != graph.N:
                raise ValueError(f"codewords must have shape [n_cw][{graph.N}]")
            if n_cw is not None and n_cw != len(self.codewords):
                raise ValueError("n_cw differs from the number of codewords")
            n_cw = len(self.codewords)
        self.n_cw = int(2 * dna_llr.PAYLOAD_NT if n_cw is None else n_cw)
        self.N = graph.N
        self.payload_nt = self.n_cw // 2  # an odd n_cw: the library's length check answers the read calls
        self.strand_index = None  # the strand index values of the read calls
        if strands is not None:
            sidx = np.asarray(strands)
            if sidx.ndim != 1 or len(sidx) != self.N or not np.issubdtype(sidx.dtype, np.integer) or \
                    (np.diff(sidx.astype(np.int64)) <= 0).any():
                raise ValueError(f"strands must be {self.N} strictly increasing int index values")
            self.strand_index = sidx.astype(np.int64)
        elif self.N == dna_llr.N_STRANDS:
            self.strand_index = dna_llr.strand_indices()
        self.strands = None  # run_sim's, once set
        sch =ldpc_amd._schedule(schedule)
        err = C.c_int(0)
        self._h = self._L.ldpc_trial_create(graph.handle, device, self.algo, self.n_cw,
                                            None if self.codewords is None else dna_llr._p(self.codewords),
                                            None if sch is None else C.byref(sch), C.byref(err))
        if not self._h:
            raise ldpc_amd.LdpcError(err.value, (self._L.ldpc_last_error() or b"").decode(errors="replace"))
        self.speculate = 0
        if speculate:
            self.set_speculation(speculate)

    def set_speculation(self, n: int) -> None:
        """eps2 steps per second decode for every later run (ldpc_trial_set_speculation)."""
        self._mod._check(self._L.ldpc_trial_set_speculation(self._h, int(n)))
        self.speculate = int(n)

    def counters(self) -> Dict:
        """The counters of the last run (ldpc_trial_get_counters); zeros before the first."""
        import ctypes as C

        import dna_llr
        cnt = dna_llr.TrialCounters()
        self._mod._check(self._L.ldpc_trial_get_counters(self._h, C.byref(cnt)))
        return cnt.as_dict()

    def run_codes(self, codes: np.ndarray, eps: float = 0.02, max_iter: int = 200, faithful: bool = True) -> Dict:
        """The trial of int8 codes [B][N], B <= n_cw, against the first B
        codewords: decode_trial(table[codes + 128], codewords[:B], codes=codes)."""
        import dna_llr
        k = np.ascontiguousarray(codes)
        if k.dtype != np.int8 or k.ndim != 2 or k.shape[1] != self.N:
            raise ValueError(f"codes must be int8 [B][{self.N}]")
        out = _TrialOut(max(len(k), 1), self.N)
        self._mod._check(self._L.ldpc_trial_run_codes(self._h, dna_llr._p(k), len(k), float(eps), int(max_iter),
                                                      int(bool(faithful)), out.ref()))
        res = out.result()
        res.update(self.counters())
        return res

    def _strand_index(self) -> np.ndarray:
        if self.strand_index is None:
            raise ValueError(f"a handle of N = {self.N} strands needs their index values for the read calls: "
                             "ResidentTrial(..., strands=...)")
        return self.strand_index

    def _run_reads(self, index_vals, seqs, quals, eps, max_iter, align_fn, faithful, workspace_bytes):
        """ldpc_trial_run_reads -> the result dict, or None when the codes cannot carry the input."""
        import dna_llr
        mod, L = self._mod, self._L
        buf, offs, lens, q, iv, sidx, n = dna_llr._native_inputs(index_vals, seqs, quals, self._strand_index())
        out = _TrialOut(self.n_cw, self.N, n_strands=len(sidx))
        p = dna_llr._p
        rc = L.ldpc_trial_run_reads(self._h, p(buf), p(offs), p(lens), p(q), n, None if iv is None else p(iv), p(sidx),
                                    len(sidx), self.payload_nt, 1 if dna_llr._native_align(align_fn) else 0,
                                    int(workspace_bytes), float(eps), int(max_iter), int(bool(faithful)), out.ref())
        if rc == mod.LDPC_ERR_UNSUPPORTED and out.r.codes_exact == 0 and self.codewords is not None:
            return None
        dna_llr._native_check(mod, rc)
        return self._resident_result(out)

    def _resident_result(self, out: "_TrialOut") -> Dict:
        """The result dict of a reads-to-result call that stayed on the device."""
        import dna_llr
        res = out.result()
        res.update(self.counters())
        kind, stats = out.a["kind"], out.a["stats"]
        res.update(t_llr_s=out.r.t_llr_s, n_erased_strands=int((kind == dna_llr.KIND_NONE).sum()),
                   n_reads_valid=int(stats[0]), n_align_pairs=int(stats[3]), t_align_s=0.0, llr=None, resident=True,
                   kind=kind, stats=stats)
        return res

    @staticmethod
    def _raw_counts(res: Dict) -> Dict:
        """The index decoder's keys of a raw-reads result, from the planner's stats."""
        hist = {k: int(res["stats"][6 + k]) for k in (-1, 0, 1, 2)}
        res.update(t_index_s=0.0, n_reads_dropped=hist[-1], cnumerr_hist=hist)
        return res

    def _fallback_fn(self):
        return gpu_decode_fn(self.graph, {0: "bp", 1: "msa"}[int(self.algo)])

    def run_reads(self, reads, eps: float = 0.02, max_iter: int = 200, align_fn="star", faithful: bool = True,
                  workspace_bytes: int = 0) -> Dict:
        """run_raw for reads whose index is decoded already: reads = (index
        values, payloads, qualities); the keys of trial_from_reads(native=True)."""
        res = self._run_reads(*reads, eps, max_iter, align_fn, faithful, workspace_bytes)
        if res is None:
            res = trial_from_reads(reads, self.codewords, eps=eps, max_iter=max_iter, align_fn=align_fn,
                                   decode_fn=self._fallback_fn(), faithful=faithful, device=self.device, native=True,
                                   strands=self.strand_index, payload_nt=self.payload_nt)
            res["resident"] = False
        return res

    def run_raw(self, raw_reads, eps: float = 0.02, max_iter: int = 200, align_fn="star", faithful: bool = True,
                workspace_bytes: int = 0) -> Dict:
        """Raw reads (sequences -- a list of str or a packed (buf, offsets,
        lengths) triple -- and qualities) to the trial's result in one library
        call.  The keys are those of trial_from_raw_reads(native=True), with
        llr None (no LLR matrix is made) and resident=True, plus kind, stats,
        iters and valid.  When a count difference is outside int8 the codes
        cannot carry the input (LDPC_ERR_UNSUPPORTED): the call falls back to
        trial_from_raw_reads(native=True) and marks resident=False (that path
        needs the true codewords; without them the error is raised)."""
        seqs, quals = raw_reads
        res = self._run_reads(None, seqs, quals, eps, max_iter, align_fn, faithful, workspace_bytes)
        if res is None:
            res = trial_from_raw_reads(raw_reads, self.codewords, eps=eps, max_iter=max_iter, align_fn=align_fn,
                                       decode_fn=self._fallback_fn(), faithful=faithful, device=self.device,
                                       native=True, strands=self.strand_index, payload_nt=self.payload_nt)
            res["resident"] = False
            return res
        return self._raw_counts(res)

    def set_strands(self, strands: np.ndarray) -> None:
        """The strands run_sim samples, [N][16 + n_cw / 2] uint8 ASCII over ACGT
        (synth.dna_strands): uploaded once (ldpc_trial_set_strands)."""
        import dna_llr
        s = np.ascontiguousarray(strands, np.uint8)
        if s.ndim != 2:
            raise ValueError("strands must be uint8 [N][strand_nt]")
        self._mod._check(self._L.ldpc_trial_set_strands(self._h, dna_llr._p(s), s.shape[0], s.shape[1]))
        self.strands = s

    def run_sim(self, seed: int, n_reads: int, sub: float = 0.01, ins: float = 0.0, dele: float = 0.0,
                strands: Optional[np.ndarray] = None, r0: int = 0, quality: Optional[np.ndarray] = None,
                eps: float = 0.02, max_iter: int = 200, align_fn="star", faithful: bool = True,
                workspace_bytes: int = 0) -> Dict:
        """Strands to the trial's result in one library call (ldpc_trial_run_sim,
        DESIGN.md sec. 8.9): the reads [r0, r0 + n_reads) of the counter-hashed
        channel (synth.dna_raw_reads_hashed: the same reads) are generated on
        the GPU and planned, coded and decoded there; the result is
        run_raw(dna_raw_reads_hashed(...))'s, plus n_reads and seed.  strands:
        set on the first call and kept -- synth.dna_strands(codewords) by
        default, which a genie-less handle cannot make (pass them, or call
        set_strands).  When a count difference is outside int8 the reads are
        made by the library's host form and go through run_raw's fallback."""
        import dna_llr
        import synth
        mod, L = self._mod, self._L
        index = self._strand_index()
        if strands is not None:
            s = np.ascontiguousarray(strands, np.uint8)
            if self.strands is None or s.shape != self.strands.shape or (s != self.strands).any():
                self.set_strands(s)
        elif self.strands is None and self.codewords is not None:
            self.set_strands(synth.dna_strands(self.codewords, index))
        t_sub, t_ins, t_del, q_val, q_lo = synth.sim_tables(sub, ins, dele, quality)
        if index.size and (index.min() < -(1 << 31) or index.max() >= (1 << 31)):
            raise ValueError("strand index values must fit int32")
        sidx = np.ascontiguousarray(index, np.int32)
        out = _TrialOut(self.n_cw, self.N, n_strands=len(sidx))
        p = dna_llr._p
        rc = L.ldpc_trial_run_sim(self._h, int(seed) & 0xFFFFFFFFFFFFFFFF, int(r0), int(n_reads), t_sub, t_ins, t_del,
                                  p(q_val), p(q_lo), len(q_val), p(sidx), 1 if dna_llr._native_align(align_fn) else 0,
                                  int(workspace_bytes), float(eps), int(max_iter), int(bool(faithful)), out.ref())
        if rc == mod.LDPC_ERR_UNSUPPORTED and out.r.codes_exact == 0 and self.codewords is not None:
            raw = synth.dna_raw_reads_native(self.strands, seed, n_reads, sub, ins, dele, r0=r0, quality=quality)
            res = self.run_raw(raw, eps=eps, max_iter=max_iter, align_fn=align_fn, faithful=faithful,
                               workspace_bytes=workspace_bytes)
        else:
            dna_llr._native_check(mod, rc)
            res = self._raw_counts(self._resident_result(out))
        res.update(n_reads=int(n_reads), seed=int(seed))
        return res

    def codes(self, B: Optional[int] = None) -> np.ndarray:
        """The handle's code matrix after a run, rows [0, B) (ldpc_trial_read_codes)."""
        import dna_llr
        B = self.n_cw if B is None else int(B)
        k = np.zeros((B, self.N), np.int8)
        self._mod._check(self._L.ldpc_trial_read_codes(self._h, dna_llr._p(k), B))
        return k

    def close(self):
        if getattr(self, "_h", None):
            self._L.ldpc_trial_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


SWEEP_KEYS = ("first_success", "second_success", "second_iterations", "n_erased_strands", "n_reads_valid",
              "t_llr_s", "t_first_s", "t_second_s")


def coverage_sweep(T: ResidentTrial, n_reads_list, trials: int, seed: int = 0, sub: float = 0.01, ins: float = 0.0,
                   dele: float = 0.0, eps: float = 0.02, max_iter: int = 200, **kw) -> List[Dict]:
    """At which random-sampling number does the archive still decode: one
    T.run_sim per read count n of n_reads_list and trial t < trials.  Trial t
    uses seed `seed + t` and the reads [0, n), so within a trial a smaller
    count's reads are a prefix of a larger count's.  One row per (n, t), in
    that order: n_reads, trial, seed, and SWEEP_KEYS of the run's result (the
    times are the library's own).  Further keywords go to run_sim."""
    rows = []
    for n in n_reads_list:
        for t in range(int(trials)):
            res = T.run_sim(seed + t, int(n), sub=sub, ins=ins, dele=dele, eps=eps, max_iter=max_iter, **kw)
            row = {"n_reads": int(n), "trial": t, "seed": seed + t}
            row.update((k, res[k]) for k in SWEEP_KEYS)
            rows.append(row)
    return rows


def report(res: Dict, rs: int = 72000, total_time: Optional[float] = None, threshold: Optional[int] = None,
           newline: str = "\n") -> str:
    """The o_/x_ result-file body (decoder.py:668-727).  total_time adds the
    'Total time: %f sec' line; threshold adds the 'Re-decoding threshold
    (number): %d' line of the committed o_72000_7_*_result.txt files (written
    by a revision of decoder.py that had it, on Windows: newline='\r\n')."""
    ok = not res["fail_second"]
    fmt = lambda xs: ("None" if not xs else " ".join(str(v) for v in xs) + " ")  # noqa: E731
    n = res["n"]
    lines = ["=" * 78, " " * 31 + "Results" + " " * 40, "=" * 78]
    if total_time is not None:
        lines.append("Total time: %f sec" % total_time)
    lines.append(f"Random Sampling Number: {rs}")
    if threshold is not None:
        lines.append("Re-decoding threshold (number): %d" % threshold)
    if ok:
        lines += ["Decoding success", "", "First decoding result:   %d/%d" % (res["first_success"], n),
                  "Second decoding result:  %d/%d" % (res["second_success"], n),
                  "Second decoding iteration number:  %d" % res["second_iterations"]]
    else:
        lines += ["Decoding failure", "", "First decoding result:\t%d/%d" % (res["first_success"], n),
                  "Second decoding result:\t%d/%d" % (res["second_success"], n)]
    lines += ["First decoding failure index: " + fmt(res["fail_first"]),
              "Second decoding failure index: " + fmt(res["fail_second"])]
    return newline.join(lines) + newline


def result_file_name(res: Dict, rs: int, trial: int, eps: float, threshold: Optional[int] = None) -> str:
    """o_/x_ file name of decoder.py:668-671; with threshold, the
    o_<rs>_<threshold>_<trial>_<eps> form of the committed result files."""
    head = "o" if not res["fail_second"] else "x"
    if threshold is None:
        return head + "_%d_%d_%f_result.txt" % (rs, trial, eps)
    return head + "_%d_%d_%d_%f_result.txt" % (rs, threshold, trial, eps)
