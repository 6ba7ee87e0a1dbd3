"""DNA soft-input construction: sequenced reads -> the 272 x 18432 LLR matrix
(the step before the first decode).

Host mirror of ex_decoder/decoder.py:59-519; the arithmetic runs in HIP
(csrc/dna.hip through the C ABI):

0. raw reads are split into (decoded index, payload, quality): the first 16
   nt are an RS(8,4) word over GF(16), decoded on the GPU; reads with more
   than two symbol errors are dropped (decoder.py:59-92, split_reads);
1. reads whose decoded index is not a strand index are dropped, the rest are
   grouped by strand in read order (decoder.py:103-118, a stable sort);
2. each strand is classified (decoder.py:149-497):
   * no reads                                  -> all LLRs int 0 (:507-510)
   * one read shorter than the payload         -> only the last bit (:240-263)
   * one read, or several all of payload length -> count over the reads
   * several reads of mixed length ("ragged")  -> pairwise edit distance
     (GPU, ldpc_dna_edit_distance) keeps the reads with some partner at
     distance < 15 (:171-178); none -> no LLRs; otherwise the kept reads go
     to the aligner (MUSCLE in the reference, :181-186 -- an injected
     `align_fn` here) and aligned rows of payload length are counted; if
     none survives, only the last bit is set from the failed rows (:266-282);
3. ldpc_dna_llr turns the classified rows into LLRs, bit-major
   ([codeword i][strand j] = soft file i+1, entry j), which is exactly the
   decoder's input layout, plus the int-0 mask the soft-file writer needs.

Differences from the reference (deliberate): when the LAST strand holding
reads is ragged with no close pair, or is a single short read, the reference
keeps looping past the end of decimal_index and raises IndexError; here that
strand simply gets the same LLRs as any other strand of its kind.  MUSCLE is
out of scope: the aligner is either injected (a callable; the
older parity tests hand the same deterministic `pad_align` stand-in to the
product and to the oracle) or the built-in centre-star alignment,
align_fn="star" (star_align / star_align_groups), whose
pairwise tables and tracebacks run on the GPU.

Steps 0-2 also exist in the library: plan_llr_native,
build_llr(native=True) and ldpc_dna_reads_llr run the grouping,
classification, pair enumeration, candidate selection and row layout as GPU
kernels (csrc/dna_plan_kernels.hpp) or on one CPU thread (csrc/dna_plan.hpp),
with plan_llr below as their yardstick.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import time
from dataclasses import dataclass, field
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

PAYLOAD_NT = 136          # decoder.py:156 (len == 136)
N_STRANDS = 18432         # decoder.py:509 (range(18432))
ED_THRESHOLD = 15         # decoder.py:175 (temp < 15)

KIND_NONE, KIND_COUNT, KIND_SHORT, KIND_ALIGN_FAILED = 0, 1, 2, 3

_NO_ALIGNER = "ragged strands need an aligner (align_fn='star' or a callable)"

AlignFn = Callable[[List[str]], List[Tuple[int, str]]]


def strand_indices() -> np.ndarray:
    """The 18432 strand index values in ascending order
    (ex_decoder/pre_processing.py:29-89): every 14-bit value i whose 7
    nucleotides satisfy nt[2] != nt[3] and nt[5] != nt[6] is kept; the r-th
    kept value yields (i << 2) | (j << 1) | ((popcount(r) + j) & 1) for
    j = 0, 1 -- the parity uses the running count r of kept values, as the
    reference's sum(index[i]) does (pre_processing.py:76-78)."""
    i = np.arange(1 << 14, dtype=np.int64)
    nt = [(i >> (12 - 2 * k)) & 3 for k in range(7)]
    kept = i[(nt[2] != nt[3]) & (nt[5] != nt[6])]
    r = np.arange(len(kept), dtype=np.int64)
    pop = np.zeros_like(r)
    x = r.copy()
    while x.any():
        pop += x & 1
        x >>= 1
    out = np.empty(2 * len(kept), np.int64)
    out[0::2] = (kept << 2) | (pop & 1)
    out[1::2] = (kept << 2) | 2 | ((pop + 1) & 1)
    return out


def pad_align(seqs: Sequence[str]) -> List[Tuple[int, str]]:
    """Deterministic stand-in for the MUSCLE call (NOT an aligner): every
    sequence right-padded with '-' to the longest length, records returned
    in reverse input order (MUSCLE also reorders its output records)."""
    n = max((len(s) for s in seqs), default=0)
    return [(k, seqs[k] + "-" * (n - len(seqs[k]))) for k in reversed(range(len(seqs)))]


@dataclass
class LlrResult:
    llr: np.ndarray                # [2*payload_nt][S] float64 (soft file i+1 = row i)
    int_mask: np.ndarray           # same shape, uint8: 1 = int 0 in the reference
    kind: np.ndarray               # [S] int32 strand classification
    n_reads_valid: int = 0
    n_pairs: int = 0               # edit-distance pairs evaluated on the GPU
    n_aligned_strands: int = 0
    erased: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int64))  # strands with no LLRs
    # the count differences: llr == codes * unit exactly (decoder.py:297-314);
    # None when some |count difference| > 127 (no int8 code)
    codes: Optional[np.ndarray] = None  # [2*payload_nt][S] int8
    unit: float = 0.0                   # ln((1-eps)/eps)
    n_align_pairs: int = 0              # read-to-centre alignments of align_fn="star"
    t_align_s: float = 0.0              # time spent in the aligner

    def code_table(self) -> np.ndarray:
        """table[k + 128] = k * unit: with `codes`, the input of
        Graph.decode_codes (the same doubles as llr)."""
        return np.arange(-128, 128, dtype=np.float64) * self.unit

    def write_soft_files(self, directory: str, rs: int):
        """soft<rs>_n18432_m1860_<i>.txt, i = 1..272 (decoder.py:511-516)."""
        import ldpc_amd
        L = ldpc_amd.lib()
        llr = np.ascontiguousarray(self.llr)
        mask = np.ascontiguousarray(self.int_mask)
        ldpc_amd._check(L.ldpc_write_soft_files(os.fsencode(directory), int(rs), llr.ctypes.data_as(C.c_void_p),
                                                mask.ctypes.data_as(C.c_void_p), llr.shape[0], llr.shape[1]))


class TrialResult(C.Structure):
    """ldpc_trial_result (include/ldpc_amd.h): counts, caller-owned arrays
    (any may be null) and the stage times of one trial."""
    _fields_ = [(k, C.c_int32) for k in ("n", "first_success", "second_success", "second_iterations", "n_fail_first",
                                         "n_fail_second", "n_erasure", "codes_exact")] + \
               [(k, C.c_void_p) for k in ("fail_first", "fail_second", "first_errors", "second_errors",
                                          "erasure_index", "hard", "iters", "valid", "kind", "stats")] + \
               [(k, C.c_double) for k in ("t_llr_s", "t_first_s", "t_second_s")]


class TrialCounters(C.Structure):
    """ldpc_trial_counters (include/ldpc_amd.h): what the eps2 loop of the last trial handed its decoder."""
    _fields_ = [(k, C.c_int32) for k in ("second_decodes", "code_absmax", "steps_per_decode", "reserved")] + \
               [(k, C.c_int64) for k in ("second_rows", "second_rows_used")]

    def as_dict(self) -> dict:
        return {k: int(getattr(self, k)) for k in ("second_decodes", "second_rows", "second_rows_used", "code_absmax",
                                                   "steps_per_decode")}


# ldpc_trial_decode_fn: (user, codes, table, B, max_iter, hard, valid) -> int
TRIAL_DECODE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_int8), C.POINTER(C.c_double), C.c_int64, C.c_int32,
                              C.POINTER(C.c_uint8), C.POINTER(C.c_uint8))


def _lib():
    import ldpc_amd
    L = ldpc_amd.lib()
    if not getattr(L, "_dna_bound", False):
        vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
        L.ldpc_dna_llr.argtypes = [i32, vp, vp, vp, vp, i32, C.c_double, vp, vp, i32]
        L.ldpc_dna_llr_codes.argtypes = [i32, vp, vp, vp, vp, i32, C.c_double, vp, vp, vp, vp, i32]
        L.ldpc_dna_edit_distance.argtypes = [vp, vp, vp, i64, vp, vp, i64, vp, i32]
        L.ldpc_write_soft_files.argtypes = [C.c_char_p, i32, vp, vp, i32, i32]
        L.ldpc_py_float_repr.argtypes = [C.c_double, C.c_char_p, i32]
        L.ldpc_dna_index_encode.argtypes = [vp, i64, vp]
        L.ldpc_dna_index_decode_host.argtypes = [vp, vp, vp, i64, vp, vp]
        L.ldpc_dna_index_decode.argtypes = [vp, vp, vp, i64, vp, vp, i32]
        L.ldpc_dna_strands_host.argtypes = [vp, i32, i64, vp, vp]
        L.ldpc_dna_strands.argtypes = [vp, i32, i64, vp, vp, i32]
        L.ldpc_dna_star_align_host.argtypes = [vp, vp, vp, i64, vp, i64, vp, vp, vp, vp, i64, vp, vp]
        L.ldpc_dna_star_align.argtypes = [vp, vp, vp, i64, vp, i64, vp, vp, vp, vp, i64, vp, vp, i32, i64, vp]
        L.ldpc_dna_plan_host.argtypes = [vp, vp, vp, vp, i64, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp]
        L.ldpc_dna_plan.argtypes = [vp, vp, vp, vp, i64, vp, vp, i32, i32, i32, i32, i64, vp, vp, vp, vp, vp]
        L.ldpc_dna_reads_llr.argtypes = [vp, vp, vp, vp, i64, vp, vp, i32, i32, i32, i32, i64, C.c_double, vp, vp,
                                         vp, vp, vp, vp]
        pres = C.POINTER(TrialResult)
        L.ldpc_dna_trial_host.argtypes = [vp, i32, i32, vp, TRIAL_DECODE_FN, vp, C.c_double, i32, i32, pres]
        pcnt = C.POINTER(TrialCounters)
        L.ldpc_dna_trial_host_spec.argtypes = [vp, i32, i32, vp, TRIAL_DECODE_FN, vp, C.c_double, i32, i32, pres, i32,
                                               pcnt]
        L.ldpc_trial_set_speculation.argtypes = [vp, i32]
        L.ldpc_trial_get_counters.argtypes = [vp, pcnt]
        L.ldpc_trial_create.argtypes = [vp, i32, i32, i32, vp, C.POINTER(ldpc_amd.Schedule), C.POINTER(C.c_int)]
        L.ldpc_trial_create.restype = vp
        L.ldpc_trial_free.argtypes = [vp]
        L.ldpc_trial_free.restype = None
        L.ldpc_trial_run_reads.argtypes = [vp, vp, vp, vp, vp, i64, vp, vp, i32, i32, i32, i64, C.c_double, i32, i32,
                                           pres]
        L.ldpc_trial_run_codes.argtypes = [vp, vp, i64, C.c_double, i32, i32, pres]
        L.ldpc_trial_read_codes.argtypes = [vp, vp, i64]
        sim = [vp, i32, i32, C.c_uint64, i64, i64, i64, i64, i64, vp, vp, i32, vp, vp, vp, vp]
        L.ldpc_dna_sim_stride.argtypes = [i32]
        L.ldpc_dna_sim_stride.restype = i64
        L.ldpc_dna_sim_reads_host.argtypes = sim
        L.ldpc_dna_sim_reads.argtypes = sim + [i32]
        L.ldpc_trial_set_strands.argtypes = [vp, vp, i64, i32]
        L.ldpc_trial_run_sim.argtypes = [vp, C.c_uint64, i64, i64, i64, i64, i64, vp, vp, i32, vp, i32, i64,
                                         C.c_double, i32, i32, pres]
        L._dna_bound = True
    return ldpc_amd, L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def edit_distance(seqs: Sequence[str], pairs: np.ndarray, device: int = 0) -> np.ndarray:
    """Levenshtein distance of each (a, b) index pair, on the GPU
    (def_func.edit_dist, def_func.py:10-26)."""
    mod, L = _lib()
    pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    enc = [s.encode("latin-1") for s in seqs]
    lens = np.array([len(b) for b in enc], np.int32)
    offs = np.zeros(len(enc), np.int64)
    if len(enc) > 1:
        offs[1:] = np.cumsum(lens[:-1], dtype=np.int64)
    buf = np.frombuffer(b"".join(enc) or b"\0", np.uint8).copy()
    a = np.ascontiguousarray(pairs[:, 0])
    b = np.ascontiguousarray(pairs[:, 1])
    out = np.zeros(len(pairs), np.int32)
    mod._check(L.ldpc_dna_edit_distance(_p(buf), _p(offs), _p(lens), len(enc), _p(a), _p(b), len(pairs),
                                        _p(out), device))
    return out


def _concat(seqs):
    """Sequences as the C ABI takes them: concatenated bytes, offsets, lengths
    (the packed triple the native planner also accepts in place of a list)."""
    enc = [s.encode("latin-1", "replace") for s in seqs]
    lens = np.array([len(b) for b in enc], np.int32)
    offs = np.zeros(len(enc), np.int64)
    if len(enc) > 1:
        offs[1:] = np.cumsum(lens[:-1], dtype=np.int64)
    buf = np.frombuffer(b"".join(enc) or b"\0", np.uint8).copy()
    return buf, offs, lens


# --- the strand index code: RS(8,4) over GF(16) in the 16-nt prefix ---------
PREFIX_NT = 16            # decoder.py:60 (RS_seq[i][0:16])


def encode_indices(index) -> np.ndarray:
    """[n][16] uint8 ASCII: the prefix (index + RS parity) of each 16-bit
    strand index (host; csrc/rs_index.hpp)."""
    mod, L = _lib()
    idx = np.asarray(index)
    if idx.size and (idx.min() < 0 or idx.max() > 0xFFFF):
        raise ValueError("strand indices are 16-bit values (0..65535)")
    idx = np.ascontiguousarray(idx, np.int32).reshape(-1)
    out = np.zeros((len(idx), PREFIX_NT), np.uint8)
    mod._check(L.ldpc_dna_index_encode(_p(idx), len(idx), _p(out)))
    return out


def _decode_indices(seqs: Sequence[str], device: Optional[int]):
    mod, L = _lib()
    buf, offs, lens = _concat(seqs)
    n = len(lens)
    index = np.full(n, -1, np.int32)
    cnumerr = np.full(n, -1, np.int32)
    if device is None:
        mod._check(L.ldpc_dna_index_decode_host(_p(buf), _p(offs), _p(lens), n, _p(index), _p(cnumerr)))
    else:
        mod._check(L.ldpc_dna_index_decode(_p(buf), _p(offs), _p(lens), n, _p(index), _p(cnumerr), device))
    return index, cnumerr


def decode_indices(seqs: Sequence[str], device: int = 0):
    """(index, cnumerr), int32 [n]: the RS(8,4) decode of every raw read's
    first 16 nt on the GPU (the reference's rs_dec.exe, decoder.py:59-80).
    cnumerr is the number of corrected symbols (0, 1, 2) or -1, index the
    corrected 16-bit value or -1; reads shorter than 16 nt or with a non-ACGT
    character in the prefix give -1."""
    return _decode_indices(seqs, device)


def decode_indices_host(seqs: Sequence[str]):
    """decode_indices on the CPU (one thread)."""
    return _decode_indices(seqs, None)


def split_reads(raw_seqs: Sequence[str], quals: Sequence[int], device: int = 0, host: bool = False):
    """decoder.py:59-92: raw reads -> (index values, payloads, qualities) of
    the reads whose prefix decodes (cnumerr 0, 1 or 2), in input order; the
    payload is seq[16:].  The triple is what plan_llr / build_llr take (the
    valid-index filter of decoder.py:110-115 is applied there)."""
    return split_reads_counted(raw_seqs, quals, device, host)[0]


def split_reads_counted(raw_seqs: Sequence[str], quals: Sequence[int], device: int = 0, host: bool = False):
    """split_reads plus the histogram of cnumerr over all reads:
    (reads, {-1: dropped, 0: .., 1: .., 2: ..})."""
    if len(raw_seqs) != len(quals):
        raise ValueError("raw_seqs and quals must have the same length")
    index, cnumerr = _decode_indices(raw_seqs, None if host else device)
    keep = np.nonzero(cnumerr >= 0)[0]
    hist = {k: int((cnumerr == k).sum()) for k in (-1, 0, 1, 2)}
    reads = (index[keep].astype(np.int64).tolist(), [raw_seqs[i][PREFIX_NT:] for i in keep],
             [int(quals[i]) for i in keep])
    return reads, hist


# --- the built-in aligner: centre-star multiple alignment ----
@dataclass
class StarAlignment:
    """What ldpc_dna_star_align[_host] returns for a batch of groups."""
    center: np.ndarray     # [G] int32: the centre's index inside its group (-1: empty group)
    width: np.ndarray      # [G] int32: the aligned width
    out_ptr: np.ndarray    # [G+1] int64: group g's rows start at out[out_ptr[g]]
    out: np.ndarray        # uint8: the rows, width[g] bytes each, in input order
    dist: np.ndarray       # [n_seqs] int32: Levenshtein distance of every read to its group's centre
    group_ptr: np.ndarray  # [G+1] int64
    n_host_groups: int = 0  # device form: groups of >= 2 reads aligned by the host code inside the call
    n_passes: int = 0       # device form: kernel passes (the workspace budget splits the pairs)
    n_pairs: int = 0        # device form: pairs aligned on the device

    def rows(self, g: int) -> List[bytes]:
        k = int(self.group_ptr[g + 1] - self.group_ptr[g])
        w, o = int(self.width[g]), int(self.out_ptr[g])
        return [self.out[o + r * w:o + (r + 1) * w].tobytes() for r in range(k)]


def star_align_batch(groups: Sequence[Sequence[str]], device: int = 0, host: bool = False,
                     workspace_bytes: int = 0) -> StarAlignment:
    """The centre-star alignment of every group (each a list of reads) in
    one call: on the GPU (`device`; workspace_bytes bounds the
    traceback workspace of one kernel pass, 0 = the library's default), or
    with host=True on one CPU thread.  The two give identical bytes."""
    mod, L = _lib()
    enc = [s for g in groups for s in g]
    buf, offs, lens = _concat(enc)
    gp = np.zeros(len(groups) + 1, np.int64)
    gp[1:] = np.cumsum([len(g) for g in groups], dtype=np.int64)
    G = len(groups)
    center, width = np.zeros(max(G, 1), np.int32), np.zeros(max(G, 1), np.int32)
    out_ptr = np.zeros(G + 1, np.int64)
    dist = np.zeros(max(len(enc), 1), np.int32)
    needed, stats = C.c_int64(0), np.zeros(3, np.int64)
    # a first guess of the output size (twice the longest read per row); the call reports the exact one
    cap = sum(len(g) * (2 * max((len(s) for s in g), default=0) + 16) for g in groups)

    def call(out):
        head = (_p(buf), _p(offs), _p(lens), len(enc), _p(gp), G, _p(center), _p(width), _p(out_ptr), _p(out),
                len(out), C.byref(needed), _p(dist))
        if host:
            return L.ldpc_dna_star_align_host(*head)
        return L.ldpc_dna_star_align(*head, device, int(workspace_bytes), _p(stats))

    out = np.zeros(max(cap, 1), np.uint8)
    rc = call(out)
    if rc == mod.LDPC_ERR_ARG and needed.value > len(out):
        out = np.zeros(needed.value, np.uint8)
        rc = call(out)
    mod._check(rc)
    return StarAlignment(center=center[:G], width=width[:G], out_ptr=out_ptr, out=out[:needed.value],
                         dist=dist[:len(enc)], group_ptr=gp, n_host_groups=int(stats[0]), n_passes=int(stats[1]),
                         n_pairs=int(stats[2]))


def star_align_groups(groups: Sequence[Sequence[str]], device: int = 0, host: bool = False,
                      workspace_bytes: int = 0) -> List[List[Tuple[int, str]]]:
    """star_align for many groups in one call (on GPU `device`, or on the
    CPU with host=True): per group the AlignFn records [(order, row)]."""
    res = star_align_batch(groups, device, host, workspace_bytes)
    return [[(k, r.decode("latin-1")) for k, r in enumerate(res.rows(g))] for g in range(len(groups))]


def star_align(seqs: Sequence[str]) -> List[Tuple[int, str]]:
    """The built-in AlignFn (host only, one group): the deterministic
    centre-star multiple alignment of DESIGN.md sec. 8.6 -- the centre is the
    read with the smallest sum of Levenshtein distances to the others, every
    other read is aligned to it, insertions share '-'-padded columns.
    Records come back in input order as (order, row)."""
    return star_align_groups([list(seqs)], host=True)[0]


def py_float_repr(v: float) -> str:
    """The library's Python-repr formatter (used by the soft-file writer)."""
    mod, L = _lib()
    buf = C.create_string_buffer(40)
    n = L.ldpc_py_float_repr(float(v), buf, 40)
    if n < 0:
        mod._check(n)
    return buf.value.decode()


@dataclass
class LlrPlan:
    """Host classification handed to ldpc_dna_llr."""
    kind: np.ndarray      # [S] int32
    row_ptr: np.ndarray   # [S+1] int64
    rows: np.ndarray      # [max(R,1)][payload_nt] uint8
    row_q: np.ndarray     # [max(R,1)] int32
    n_reads_valid: int
    n_pairs: int
    n_aligned_strands: int
    n_align_pairs: int = 0
    t_align_s: float = 0.0
    cnumerr_hist: dict = field(default_factory=dict)        # plan_llr_native on raw reads


def plan_llr(index_vals: Sequence[int], seqs: Sequence[str], quals: Sequence[int],
             align_fn: Optional[AlignFn] = None, device: int = 0, strands: Optional[np.ndarray] = None,
             distance_fn=None, align_host: Optional[bool] = None, payload_nt: int = PAYLOAD_NT) -> LlrPlan:
    """Group and classify the reads (decoder.py:103-497 control flow).
    Pairwise distances of ragged strands come from the GPU
    (`distance_fn` defaults to edit_distance on `device`).  align_fn is a
    callable, asked once per ragged strand, or "star": the candidate groups
    of all ragged strands then go to the built-in aligner in one batched call
    (star_align_groups on `device`; on the CPU with align_host=True, which is
    also what a caller gets who keeps the distances off the GPU with a
    distance_fn and leaves align_host None).  payload_nt: the payload length
    of a strand in nucleotides (half the number of codewords)."""
    nt = int(payload_nt)
    if nt < 1:
        raise ValueError("payload_nt must be at least 1")
    if isinstance(align_fn, str) and align_fn != "star":
        raise ValueError(f"unknown aligner {align_fn!r} (a callable or 'star')")
    if align_host is None:
        align_host = distance_fn is not None
    distance_fn = distance_fn or (lambda sq, pr: edit_distance(sq, pr, device))
    sidx = strand_indices() if strands is None else np.asarray(strands, np.int64)
    S = len(sidx)
    iv = np.asarray(index_vals, np.int64)
    if not (len(iv) == len(seqs) == len(quals)):
        raise ValueError("index_vals, seqs and quals must have the same length")
    pos = np.searchsorted(sidx, iv)
    ok = pos < S
    ok[ok] = sidx[pos[ok]] == iv[ok]
    read_ids = np.nonzero(ok)[0]
    read_ids = read_ids[np.argsort(pos[read_ids], kind="stable")]  # decoder.py:116
    rpos = pos[read_ids]
    q_all = np.asarray(quals, np.int64)
    lens = np.fromiter((len(seqs[r]) for r in read_ids), np.int64, len(read_ids))
    cnt = np.bincount(rpos, minlength=S)
    start = np.zeros(S + 1, np.int64)
    start[1:] = np.cumsum(cnt)

    kind = np.zeros(S, np.int32)
    all_full = np.ones(S, bool)
    np.logical_and.at(all_full, rpos, lens == nt)
    single = cnt == 1
    first_len = np.zeros(S, np.int64)
    first_len[cnt > 0] = lens[start[:-1][cnt > 0]]
    kind[single & (first_len < nt)] = KIND_SHORT
    kind[single & (first_len >= nt)] = KIND_COUNT
    multi = cnt > 1
    kind[multi & all_full] = KIND_COUNT
    ragged = np.nonzero(multi & ~all_full)[0]

    # ragged strands: all pairs i < k per strand -> one GPU batch
    pair_list, pair_strand = [], []
    for s in ragged:
        n = int(cnt[s])
        ii, kk = np.triu_indices(n, 1)
        pair_list.append(np.stack([start[s] + ii, start[s] + kk], 1))
        pair_strand.append(np.full(len(ii), s))
    rows_of = {}  # strand -> (row strings, qualities) for aligned / failed strands
    n_pairs = 0
    n_aligned = 0
    n_align_pairs = 0
    t_align = 0.0
    if pair_list:
        pairs = np.concatenate(pair_list)
        n_pairs = len(pairs)
        # pair indices refer to positions in the strand-sorted read list
        local = [seqs[r] for r in read_ids]
        d = distance_fn(local, pairs)
        close = d < ED_THRESHOLD
        ps = np.concatenate(pair_strand)
        todo = []  # (strand, candidates, their qualities) of the strands that go to the aligner
        for s in ragged:
            m = close & (ps == s)
            sel = np.unique(pairs[m].ravel())  # decoder.py:176-178 (np.unique: sorted)
            if len(sel) == 0:
                kind[s] = KIND_NONE  # decoder.py:179-188
                continue
            if align_fn is None:
                raise RuntimeError(_NO_ALIGNER)
            todo.append((s, [local[i] for i in sel], q_all[read_ids[sel]]))
        t0 = time.perf_counter()
        if align_fn == "star":  # one batched call for all strands
            records = star_align_groups([cand for _, cand, _ in todo], device=device, host=align_host) if todo else []
            n_align_pairs = sum(len(cand) - 1 for _, cand, _ in todo)
        else:
            records = [align_fn(cand) for _, cand, _ in todo]
        t_align = time.perf_counter() - t0
        for (s, cand, cq), recs in zip(todo, records):
            aligned, aq, err, eq = [], [], [], []
            for order, a in recs:  # decoder.py:195-214
                if len(a) != nt:
                    err.append(a[-1] if a else "")
                    eq.append(int(cq[order]))
                    continue
                aligned.append(a)
                aq.append(int(cq[order]))
            n_aligned += 1
            if aligned:
                kind[s] = KIND_COUNT
                rows_of[s] = (aligned, aq)
            else:
                kind[s] = KIND_ALIGN_FAILED
                rows_of[s] = (err, eq)

    # rows: nt bytes each (kinds 2/3: byte 0 = last base)
    row_count = np.zeros(S, np.int64)
    plain_count = (kind == KIND_COUNT) & ~np.isin(np.arange(S), list(rows_of.keys()))
    row_count[plain_count] = cnt[plain_count]
    row_count[kind == KIND_SHORT] = 1
    for s, (rws, _) in rows_of.items():
        row_count[s] = len(rws)
    row_ptr = np.zeros(S + 1, np.int64)
    row_ptr[1:] = np.cumsum(row_count)
    R = int(row_ptr[-1])
    rows = np.full((max(R, 1), nt), ord("-"), np.uint8)
    row_q = np.zeros(max(R, 1), np.int32)

    # plain count strands: the reads' first nt bases, vectorised
    pc = np.nonzero(plain_count)[0]
    if len(pc):
        sel_reads = np.concatenate([np.arange(start[s], start[s + 1]) for s in pc])
        dst = np.concatenate([np.arange(row_ptr[s], row_ptr[s + 1]) for s in pc])
        blob = np.frombuffer("".join(seqs[read_ids[r]][:nt] for r in sel_reads).encode("latin-1"),
                             np.uint8)
        rows[dst] = blob.reshape(-1, nt)
        row_q[dst] = q_all[read_ids[sel_reads]]
    for s in np.nonzero(kind == KIND_SHORT)[0]:
        r = read_ids[start[s]]
        sq = seqs[r]
        if not sq and q_all[r] > 63:
            raise ValueError(f"empty read on strand {s} with quality > 63 (the reference indexes its last bit)")
        rows[row_ptr[s], 0] = ord(sq[-1]) if sq else ord("-")
        row_q[row_ptr[s]] = q_all[r]
    for s, (rws, qs) in rows_of.items():
        for k, (txt, q) in enumerate(zip(rws, qs)):
            if kind[s] == KIND_COUNT:
                rows[row_ptr[s] + k] = np.frombuffer(txt.encode("latin-1"), np.uint8)
            else:
                rows[row_ptr[s] + k, 0] = ord(txt) if txt else ord("-")
            row_q[row_ptr[s] + k] = q

    return LlrPlan(kind=kind, row_ptr=row_ptr, rows=rows, row_q=row_q, n_reads_valid=len(read_ids),
                   n_pairs=n_pairs, n_aligned_strands=n_aligned, n_align_pairs=n_align_pairs, t_align_s=t_align)


# --- the native planner (csrc/dna_plan.hpp) -------------
N_PLAN_STATS = 9  # include/ldpc_amd.h: valid, pairs, aligned strands, alignments, R, cnumerr -1 / 0 / 1 / 2


def _packed(seqs):
    """(buf, offsets, lengths) of a list of str, or the triple itself."""
    if isinstance(seqs, tuple) and len(seqs) == 3 and isinstance(seqs[0], np.ndarray):
        buf, offs, lens = seqs
        return (np.ascontiguousarray(buf, np.uint8), np.ascontiguousarray(offs, np.int64),
                np.ascontiguousarray(lens, np.int32))
    return _concat(seqs)


def _native_inputs(index_vals, seqs, quals, strands):
    buf, offs, lens = _packed(seqs)
    n = len(lens)
    q = np.ascontiguousarray(quals, np.int32).reshape(-1)
    iv = None
    if index_vals is not None:
        iv64 = np.asarray(index_vals, np.int64).reshape(-1)
        # an index outside int32 is no strand index (strand values are checked below): any invalid value will do
        iv = np.ascontiguousarray(np.where((iv64 < -(1 << 31)) | (iv64 >= (1 << 31)), -1, iv64), np.int32)
    if len(q) != n or (iv is not None and len(iv) != n):
        raise ValueError("index_vals, seqs and quals must have the same length")
    sidx64 = strand_indices() if strands is None else np.asarray(strands, np.int64).reshape(-1)
    if sidx64.size and (sidx64.min() < -(1 << 31) or sidx64.max() >= (1 << 31)):
        raise ValueError("strand index values must fit int32")
    return buf, offs, lens, q, iv, np.ascontiguousarray(sidx64, np.int32), n


def _native_check(mod, rc):
    """The library's error as plan_llr raises it."""
    if rc == mod.LDPC_ERR_ARG:
        msg = mod.lib().ldpc_last_error().decode()
        if "need an aligner" in msg:
            raise RuntimeError(_NO_ALIGNER)
        if "empty read on strand" in msg:
            raise ValueError(msg.split(": ", 1)[-1])
    mod._check(rc)


def plan_llr_native(index_vals, seqs, quals, device: int = 0, host: bool = False,
                    strands: Optional[np.ndarray] = None, align: bool = True, workspace_bytes: int = 0,
                    payload_nt: int = PAYLOAD_NT) -> LlrPlan:
    """plan_llr(..., align_fn="star") in the library: ldpc_dna_plan on GPU
    `device`, or ldpc_dna_plan_host on one CPU thread (host=True); the same
    bytes either way.  index_vals None: `seqs` are raw reads, whose 16-nt
    prefix is decoded and dropped inside the call (split_reads).  seqs is a
    list of str or an already packed (buf, offsets, lengths) triple (_concat).
    align=False is align_fn=None.  The cnumerr histogram of raw reads is
    plan.cnumerr_hist.  payload_nt: the payload length of a strand."""
    mod, L = _lib()
    buf, offs, lens, q, iv, sidx, n = _native_inputs(index_vals, seqs, quals, strands)
    S = len(sidx)
    nt = int(payload_nt)
    kind = np.zeros(S, np.int32)
    row_ptr = np.zeros(S + 1, np.int64)
    rows = np.full((max(n, 1), max(nt, 1)), ord("-"), np.uint8)
    row_q = np.zeros(max(n, 1), np.int32)
    stats = np.zeros(N_PLAN_STATS, np.int64)
    head = (_p(buf), _p(offs), _p(lens), _p(q), n, None if iv is None else _p(iv), _p(sidx), S, nt,
            1 if align else 0)
    tail = (_p(kind), _p(row_ptr), _p(rows), _p(row_q), _p(stats))
    if host:
        rc = L.ldpc_dna_plan_host(*head, *tail)
    else:
        rc = L.ldpc_dna_plan(*head, device, int(workspace_bytes), *tail)
    _native_check(mod, rc)
    R = int(row_ptr[-1])
    plan = LlrPlan(kind=kind, row_ptr=row_ptr, rows=rows[:max(R, 1)], row_q=row_q[:max(R, 1)],
                   n_reads_valid=int(stats[0]), n_pairs=int(stats[1]), n_aligned_strands=int(stats[2]),
                   n_align_pairs=int(stats[3]), t_align_s=0.0)
    plan.cnumerr_hist = {k: int(stats[6 + k]) for k in (-1, 0, 1, 2)}
    return plan


def _native_align(align_fn) -> bool:
    if align_fn is not None and align_fn != "star":
        raise ValueError("native=True takes align_fn None or 'star' (callable aligners run in the Python planner)")
    return align_fn == "star"


def build_llr_native(index_vals, seqs, quals, eps: float = 0.02, align: bool = True, device: int = 0,
                     strands: Optional[np.ndarray] = None, workspace_bytes: int = 0,
                     payload_nt: int = PAYLOAD_NT):
    """ldpc_dna_reads_llr: reads (raw when index_vals is None; a list of str or
    a packed triple) -> (LlrResult, cnumerr histogram) in one library call.
    payload_nt: the payload length of a strand; the matrices have 2 * payload_nt rows."""
    mod, L = _lib()
    buf, offs, lens, q, iv, sidx, n = _native_inputs(index_vals, seqs, quals, strands)
    S = len(sidx)
    nt = int(payload_nt)
    unit = math.log((1 - eps) / eps)  # decoder.py:297
    llr = np.zeros((2 * max(nt, 1), S), np.float64)
    mask = np.zeros((2 * max(nt, 1), S), np.uint8)
    codes = np.zeros((2 * max(nt, 1), S), np.int8)
    kind = np.zeros(S, np.int32)
    stats = np.zeros(N_PLAN_STATS, np.int64)
    exact = C.c_int32(0)
    _native_check(mod, L.ldpc_dna_reads_llr(_p(buf), _p(offs), _p(lens), _p(q), n, None if iv is None else _p(iv),
                                            _p(sidx), S, nt, 1 if align else 0, device, int(workspace_bytes),
                                            unit, _p(llr), _p(mask), _p(codes), C.byref(exact), _p(kind), _p(stats)))
    res = LlrResult(llr=llr, int_mask=mask, kind=kind, n_reads_valid=int(stats[0]), n_pairs=int(stats[1]),
                    n_aligned_strands=int(stats[2]), erased=np.nonzero(kind == KIND_NONE)[0],
                    codes=codes if exact.value else None, unit=unit, n_align_pairs=int(stats[3]), t_align_s=0.0)
    return res, {k: int(stats[6 + k]) for k in (-1, 0, 1, 2)}


def build_llr(index_vals: Sequence[int], seqs: Sequence[str], quals: Sequence[int], eps: float = 0.02,
              align_fn: Optional[AlignFn] = None, device: int = 0,
              strands: Optional[np.ndarray] = None, native: bool = False,
              payload_nt: int = PAYLOAD_NT) -> LlrResult:
    """Reads (decoded index value, payload sequence, quality) -> LlrResult.
    `strands` defaults to strand_indices(); align_fn answers the MUSCLE call
    for ragged strands (required only if such strands have close pairs):
    "star" is the built-in aligner on `device`, a callable is asked per strand.
    native=True: the planner runs in the library too (ldpc_dna_reads_llr, one
    call; align_fn None or "star"; seqs may be a packed triple; t_align_s is
    not measured and reads 0.0).  payload_nt: the payload length of a strand
    in nucleotides; the matrices have 2 * payload_nt rows."""
    if native:
        return build_llr_native(index_vals, seqs, quals, eps, _native_align(align_fn), device, strands,
                                payload_nt=payload_nt)[0]
    mod, L = _lib()
    plan = plan_llr(index_vals, seqs, quals, align_fn, device, strands, payload_nt=payload_nt)
    nt = int(payload_nt)
    S = len(plan.kind)
    unit = math.log((1 - eps) / eps)  # decoder.py:297
    llr = np.zeros((2 * nt, S), np.float64)
    mask = np.zeros((2 * nt, S), np.uint8)
    codes = np.zeros((2 * nt, S), np.int8)
    exact = C.c_int32(0)
    mod._check(L.ldpc_dna_llr_codes(S, _p(plan.kind), _p(plan.row_ptr), _p(plan.rows), _p(plan.row_q), nt,
                                    unit, _p(llr), _p(mask), _p(codes), C.byref(exact), device))
    return LlrResult(llr=llr, int_mask=mask, kind=plan.kind, n_reads_valid=plan.n_reads_valid,
                     n_pairs=plan.n_pairs, n_aligned_strands=plan.n_aligned_strands,
                     erased=np.nonzero(plan.kind == KIND_NONE)[0], codes=codes if exact.value else None, unit=unit,
                     n_align_pairs=plan.n_align_pairs, t_align_s=plan.t_align_s)
