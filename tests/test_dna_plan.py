"""The read planner's host form (csrc/dna_plan.hpp, ldpc_dna_plan_host,
DESIGN.md sec. 8.7) against the Python planner it restates: dna_llr.plan_llr
with the built-in aligner on the host and a numpy Levenshtein
(dna_plan_cases.reference_plan).  No GPU."""
import ctypes as C

import numpy as np
import pytest

import dna_llr
import dna_plan_cases as cases
import synth

NT = dna_llr.PAYLOAD_NT


def _native(name, **kw):
    idx, seqs, quals, strands = {"edge": cases.edge_input, "dense": cases.dense_input}[name]()
    return dna_llr.plan_llr_native(idx, seqs, quals, host=True, strands=strands, **kw)


@pytest.mark.parametrize("name", ["edge", "dense"])
def test_host_planner_equals_plan_llr(name):
    cases.same_plan(_native(name), cases.reference(name))


def test_inputs_cover_every_shape():
    """What the two inputs must hold together, read off the comparator's plans."""
    kinds, with_cand, without_cand = set(), 0, 0
    long_single = short_single = empty_low_q = foreign = False
    for name, make in (("edge", cases.edge_input), ("dense", cases.dense_input)):
        idx, seqs, quals, strands = make()
        ref = cases.reference(name)
        sidx = dna_llr.strand_indices() if strands is None else strands
        kinds |= set(np.unique(ref.kind).tolist())
        pos = {int(v): k for k, v in enumerate(sidx.tolist())}
        by = {}
        for i, v in enumerate(idx):
            if v in pos:
                by.setdefault(pos[v], []).append(i)
            else:
                foreign = True
        for s, rd in by.items():
            ln = [len(seqs[i]) for i in rd]
            if len(rd) == 1:
                long_single |= ln[0] > NT
                short_single |= 0 < ln[0] < NT
                empty_low_q |= ln[0] == 0 and quals[rd[0]] <= 63
            elif any(v != NT for v in ln):  # ragged: with candidates it has rows or kind 3, else kind 0 and no rows
                if ref.row_ptr[s + 1] > ref.row_ptr[s]:
                    with_cand += 1
                else:
                    assert ref.kind[s] == 0
                    without_cand += 1
        assert with_cand >= 1 and ref.n_aligned_strands >= 1
    assert kinds == {0, 1, 2, 3}
    assert with_cand >= 20 and without_cand >= 1
    assert long_single and short_single and empty_low_q and foreign
    assert with_cand == cases.reference("edge").n_aligned_strands + cases.reference("dense").n_aligned_strands


@pytest.fixture(scope="module")
def raw(codewords):
    return synth.dna_raw_reads(codewords, seed=5, n_reads=2500, sub=0.03, ins=0.002, dele=0.002)


def test_raw_reads_equal_split_then_payload_mode(raw):
    seqs, quals = raw
    reads, hist = dna_llr.split_reads_counted(seqs, quals, host=True)
    assert hist[-1] > 0 and hist[1] > 0 and hist[2] > 0
    want = dna_llr.plan_llr_native(*reads, host=True)
    got = dna_llr.plan_llr_native(None, seqs, quals, host=True)
    cases.same_plan(got, want)
    assert got.cnumerr_hist == hist and sum(want.cnumerr_hist.values()) == 0
    assert want.n_aligned_strands > 0
    # a packed triple is taken as the list is
    packed = dna_llr.plan_llr_native(None, dna_llr._concat(seqs), quals, host=True)
    cases.same_plan(packed, got)


def test_input_order_is_row_order():
    """Swapping two full-length reads of one strand swaps exactly their rows."""
    rng = np.random.default_rng(3)
    strands = np.array([5, 9, 12])
    rd = ["".join(rng.choice(list("ACGT"), NT)) for _ in range(6)]
    idx = [9, 5, 9, 12, 9, 5]
    quals = [60, 61, 62, 63, 64, 65]
    a = dna_llr.plan_llr_native(idx, rd, quals, host=True, strands=strands)
    assert a.kind.tolist() == [1, 1, 1] and a.row_ptr.tolist() == [0, 2, 5, 6]
    assert [bytes(r).decode() for r in a.rows] == [rd[1], rd[5], rd[0], rd[2], rd[4], rd[3]]
    assert a.row_q.tolist() == [61, 65, 60, 62, 64, 63]
    rd2, q2 = list(rd), list(quals)
    rd2[0], rd2[4], q2[0], q2[4] = rd[4], rd[0], quals[4], quals[0]
    b = dna_llr.plan_llr_native(idx, rd2, q2, host=True, strands=strands)
    swap = [0, 1, 4, 3, 2, 5]
    assert np.array_equal(b.rows, a.rows[swap]) and np.array_equal(b.row_q, a.row_q[swap])
    assert np.array_equal(b.kind, a.kind) and np.array_equal(b.row_ptr, a.row_ptr)


def test_no_reads_and_no_aligner():
    none = dna_llr.plan_llr_native([], [], [], host=True)
    assert none.kind.shape == (18432,) and not none.kind.any() and not none.row_ptr.any()
    assert none.rows.shape == (1, NT) and none.row_q.shape == (1,) and none.n_reads_valid == 0
    p = "ACGT" * (NT // 4)
    far = "TTGCA" * 24
    # ragged without a close pair: fine without an aligner, kind 0
    ok = dna_llr.plan_llr_native([7, 7, 8], [p, far, p[:50]], [70, 70, 70], host=True, strands=[7, 8], align=False)
    assert ok.kind.tolist() == [0, 2] and ok.row_ptr.tolist() == [0, 0, 1] and ok.n_pairs == 1
    assert ok.rows[0, 0] == ord(p[49]) and (ok.rows[0, 1:] == ord("-")).all()
    with pytest.raises(RuntimeError, match="ragged strands need an aligner"):
        dna_llr.plan_llr_native([7, 7], [p, p[:-1]], [70, 70], host=True, strands=[7, 8], align=False)
    got = dna_llr.plan_llr_native([7, 7], [p, p[:-1]], [70, 66], host=True, strands=[7, 8])
    assert got.kind.tolist() == [1, 0] and got.n_aligned_strands == 1 and got.n_align_pairs == 1
    assert bytes(got.rows[1]).decode() == p[:-1] + "-" and got.row_q.tolist() == [70, 66]
    # the same errors as plan_llr
    with pytest.raises(ValueError, match="empty read on strand 1 with quality > 63"):
        dna_llr.plan_llr_native([8], [""], [64], host=True, strands=[7, 8])
    with pytest.raises(ValueError, match="same length"):
        dna_llr.plan_llr_native([8, 8], [""], [64], host=True, strands=[7, 8])
    assert dna_llr.plan_llr_native([8], [""], [63], host=True, strands=[7, 8]).rows[0, 0] == ord("-")
    with pytest.raises(ValueError, match="align_fn None or 'star'"):
        dna_llr.build_llr([8], [p], [60], align_fn=dna_llr.pad_align, native=True)


def test_abi_argument_errors(L):
    """LDPC_ERR_ARG of ldpc_dna_plan_host and, before any device call, of
    ldpc_dna_plan and ldpc_dna_reads_llr."""
    _, lib = dna_llr._lib()
    buf, offs, lens = dna_llr._concat(["ACGT" * 34, "ACG"])
    q = np.array([60, 64], np.int32)
    iv = np.array([3, 4], np.int32)
    strands = np.array([3, 4, 9], np.int32)
    kind, row_ptr = np.zeros(3, np.int32), np.zeros(4, np.int64)
    rows, row_q, stats = np.zeros((2, NT), np.uint8), np.zeros(2, np.int32), np.zeros(9, np.int64)
    llr, exact = np.zeros((2 * NT, 3)), C.c_int32(0)
    p = dna_llr._p

    def call(form, seqs=buf, off=offs, ln=lens, qq=q, n=2, ix=iv, st=strands, S=3, nt=NT, kd=kind, rp=row_ptr,
             rw=rows, rq=row_q, out=llr):
        ptr = lambda a: None if a is None else p(a)  # noqa: E731
        head = (ptr(seqs), ptr(off), ptr(ln), ptr(qq), n, ptr(ix), ptr(st), S, nt, 1)
        if form == "host":
            return lib.ldpc_dna_plan_host(*head, ptr(kd), ptr(rp), ptr(rw), ptr(rq), p(stats))
        if form == "device":
            return lib.ldpc_dna_plan(*head, 0, 0, ptr(kd), ptr(rp), ptr(rw), ptr(rq), p(stats))
        return lib.ldpc_dna_reads_llr(*head, 0, 0, 3.89, ptr(out), None, None, C.byref(exact), ptr(kd), p(stats))

    who = {"host": "ldpc_dna_plan_host", "device": "ldpc_dna_plan", "fused": "ldpc_dna_reads_llr"}
    assert call("host") == L.LDPC_OK
    assert kind.tolist() == [1, 2, 0] and row_ptr.tolist() == [0, 1, 2, 2] and stats[:5].tolist() == [2, 0, 0, 0, 2]
    for form in ("host", "device", "fused"):
        bad = [dict(st=np.array([3, 9, 4], np.int32)), dict(st=np.array([3, 4, 4], np.int32)), dict(st=None),
               dict(seqs=None), dict(off=None), dict(ln=None), dict(qq=None), dict(n=-1), dict(S=-1), dict(nt=0),
               dict(ln=np.array([136, -1], np.int32)), dict(off=np.array([0, -5], np.int64)),
               dict(off=np.array([0, 2 ** 63 - 2], np.int64)), dict(qq=np.array([60, 64], np.int32), ln=np.array([136, 0], np.int32))]
        if form != "fused":
            bad += [dict(kd=None), dict(rp=None), dict(rw=None), dict(rq=None)]
        else:
            bad += [dict(out=None)]
        for kw in bad:
            if form != "host" and "qq" in kw and "ln" in kw:
                continue  # the empty read of quality 64 is found on the device
            assert call(form, **kw) == L.LDPC_ERR_ARG, (form, kw)
            assert lib.ldpc_last_error().decode().startswith(who[form] + ": "), (form, kw)
    assert call("host", ln=np.array([136, 0], np.int32)) == L.LDPC_ERR_ARG
    assert "empty read on strand 1" in lib.ldpc_last_error().decode()
