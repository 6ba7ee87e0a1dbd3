"""CPU tests of the built-in aligner (include/ldpc_amd.h "The aligner of
ragged strands", csrc/star_align.hpp): the host entry
against the independent reference of star_ref.py byte for byte, the properties
of an alignment checked on the product's output alone, the C ABI's argument
errors, and plan_llr(align_fn="star") on hand-made strands."""
import ctypes as C

import numpy as np
import pytest

import star_cases
import star_ref


@pytest.fixture(scope="module")
def llr_mod(L):
    import dna_llr
    return dna_llr


def _check_against_ref(llr_mod, groups):
    res = llr_mod.star_align_batch(groups, host=True)
    assert len(res.center) == len(res.width) == len(groups) and len(res.out_ptr) == len(groups) + 1
    off = 0
    for g, grp in enumerate(groups):
        centre, width, rows, dist = star_ref.star(grp)
        assert (int(res.center[g]), int(res.width[g])) == (centre, width), (g, grp)
        assert res.rows(g) == rows, (g, grp)
        assert res.dist[off:off + len(grp)].tolist() == dist, (g, grp)
        off += len(grp)
    assert int(res.out_ptr[-1]) == len(res.out) == sum(len(g) * int(w) for g, w in zip(groups, res.width))
    return res


def test_reference_itself():
    """star_ref on cases worked out by hand from the definition."""
    # ACGTT against the centre ACGT: (5,4) diagonal T/T, (4,3): T/G is no diagonal (D[3][2] + 1 = 2 != 1),
    # up fits (D[3][3] + 1 = 1): the first T is an insertion in slot 3, before the centre's T
    assert star_ref.star(["ACGT", "ACT", "AGGT", "ACGTT"]) == (0, 5, [b"ACG-T", b"AC--T", b"AGG-T", b"ACGTT"], [0, 1, 1, 1])
    # homopolymer: the diagonal is preferred from the end, so the gap / the insertion lands at the front
    assert star_ref.star(["AAAA", "AAA"]) == (0, 4, [b"AAAA", b"-AAA"], [0, 1])
    assert star_ref.star(["AAA", "AAAA"]) == (0, 4, [b"-AAA", b"AAAA"], [0, 1])
    assert star_ref.star(["ACGT"]) == (0, 4, [b"ACGT"], [0])
    assert star_ref.star(["", "AC"]) == (0, 2, [b"--", b"AC"], [0, 2])
    assert star_ref.star(["GGGG", "AC", "CA"])[0] == 1  # sums 8, 6, 6: the tie goes to the lower index
    assert star_ref.distance("kitten", "sitting") == 3


def test_random_groups_match_reference(llr_mod):
    groups = list(star_cases.random_groups())
    assert {len(g) for g in groups} == set(range(1, 9))
    res = _check_against_ref(llr_mod, groups)
    assert (res.width[160:] != 136).any() and (res.dist > 0).any()


def test_exhaustive_single_edits(llr_mod):
    groups = star_cases.exhaustive_groups()
    # distinct results of the 30 substitutions, 10 deletions (8 runs) and 44 insertions (4 * 11 - 10)
    assert len(groups) == 2 * (30 + 8 + 34)
    res = _check_against_ref(llr_mod, groups)
    assert (res.center == 0).all() and (res.dist.reshape(-1, 2) == [0, 1]).all()


def test_edge_cases(llr_mod):
    edge = star_cases.edge_groups()
    res = _check_against_ref(llr_mod, edge)
    assert res.rows(0) == [b""] and res.rows(1) == [b"", b""] and res.rows(2) == [b"----", b"ACGT"]
    assert res.rows(5) == [b"ACGTACGT"] * 4 and int(res.center[5]) == 0
    assert res.center[6:9].tolist() == [1, 0, 0]  # ties broken by index
    assert int(res.width[-1]) >= 1000
    # no group, and an empty group between two others
    none = llr_mod.star_align_batch([], host=True)
    assert len(none.center) == 0 and none.out_ptr.tolist() == [0] and len(none.out) == 0
    res = llr_mod.star_align_batch([("AC", "A"), (), ("G",)], host=True)
    assert res.center.tolist() == [0, -1, 0] and res.width.tolist() == [2, 0, 1] and res.out_ptr.tolist() == [0, 4, 4, 5]
    assert res.out.tobytes() == b"ACA-G"
    # the AlignFn forms
    assert llr_mod.star_align(["ACGT", "ACT", "AGGT", "ACGTT"]) == [(0, "ACG-T"), (1, "AC--T"), (2, "AGG-T"), (3, "ACGTT")]
    assert llr_mod.star_align(["ACGT"]) == [(0, "ACGT")]
    assert llr_mod.star_align_groups([["AAAA", "AAA"], ["C"]], host=True) == [[(0, "AAAA"), (1, "-AAA")], [(0, "C")]]


def _levenshtein(a: bytes, b: bytes) -> int:
    """An independent DP (plain Python, two rows)."""
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        cur = [i] + [0] * len(b)
        for j in range(1, len(b) + 1):
            cur[j] = min(prev[j - 1] + (a[i - 1] != b[j - 1]), prev[j] + 1, cur[j - 1] + 1)
        prev = cur
    return prev[-1]


def test_alignment_properties(llr_mod):
    """Checked on the product's output alone: all rows of a group have the
    reported width; a row without '-' is the read; the centre row has '-'
    exactly in the slot columns (every other column is a centre position, in
    order); and the columns of a row that are neither gap/gap in a slot nor
    equal to the centre row's number the Levenshtein distance."""
    groups = list(star_cases.random_groups()) + star_cases.exhaustive_groups()[:40] + star_cases.edge_groups()[:-1]
    res = llr_mod.star_align_batch(groups, host=True)
    off = 0
    for g, grp in enumerate(groups):
        rows, c, w = res.rows(g), int(res.center[g]), int(res.width[g])
        enc = [s.encode("latin-1") for s in grp]
        assert len(rows) == len(grp) and all(len(r) == w for r in rows)
        centre_row = rows[c]
        has_gap_byte = any(b"-" in e for e in enc)
        for r, e in zip(rows, enc):
            assert r.replace(b"-", b"") == e.replace(b"-", b"")
        if not has_gap_byte:
            slot = [ch == ord("-") for ch in centre_row]  # the slot columns
            assert bytes(ch for ch, s in zip(centre_row, slot) if not s) == enc[c]
            for k, (r, e) in enumerate(zip(rows, enc)):
                cost = sum(1 for x, y, s in zip(r, centre_row, slot) if not (x == y))
                assert cost == _levenshtein(e, enc[c]) == int(res.dist[off + k]), (g, k)
                # a slot column holds a '-' in the centre row only
                assert all(y == ord("-") for y, s in zip(centre_row, slot) if s)
        off += len(grp)


def test_c_abi_error_cases(L, llr_mod):
    mod, lib = llr_mod._lib()
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    ARG, OK = L.LDPC_ERR_ARG, L.LDPC_OK
    seq = np.frombuffer(b"ACGTACTAGGT", np.uint8).copy()
    off, ln = np.array([0, 4, 7], np.int64), np.array([4, 3, 4], np.int32)
    gp = np.array([0, 3], np.int64)
    ce, wd, op = np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(2, np.int64)
    out, dist = np.zeros(64, np.uint8), np.zeros(3, np.int32)
    need, stats = C.c_int64(-1), np.zeros(3, np.int64)

    def host(seq_=seq, off_=off, ln_=ln, n=3, gp_=gp, G=1, ce_=ce, wd_=wd, op_=op, out_=out, cap=64, dist_=dist):
        q = lambda a: None if a is None else p(a)  # noqa: E731
        return lib.ldpc_dna_star_align_host(q(seq_), q(off_), q(ln_), n, q(gp_), G, q(ce_), q(wd_), q(op_), q(out_), cap,
                                            C.byref(need), q(dist_))

    def dev(ws=0, device=0, **kw):
        d = dict(seq_=seq, off_=off, ln_=ln, n=3, gp_=gp, G=1, ce_=ce, wd_=wd, op_=op, out_=out, cap=64, dist_=dist)
        d.update(kw)
        q = lambda a: None if a is None else p(a)  # noqa: E731
        return lib.ldpc_dna_star_align(q(d["seq_"]), q(d["off_"]), q(d["ln_"]), d["n"], q(d["gp_"]), d["G"], q(d["ce_"]),
                                       q(d["wd_"]), q(d["op_"]), q(d["out_"]), d["cap"], C.byref(need), q(d["dist_"]),
                                       device, ws, p(stats))

    assert host() == OK
    assert (ce.tolist(), wd.tolist(), op.tolist(), need.value) == ([0], [4], [0, 12], 12)
    assert out[:12].tobytes() == b"ACGTAC-TAGGT" and dist.tolist() == [0, 1, 1]
    assert host(dist_=None) == OK  # dist is optional
    for fn in (host, dev):  # every argument error comes before any device call
        assert fn(off_=None) == ARG and fn(ln_=None) == ARG and fn(gp_=None) == ARG
        assert b"bad arguments" in lib.ldpc_last_error()
        assert fn(ce_=None) == ARG and fn(wd_=None) == ARG and fn(op_=None) == ARG
        assert fn(out_=None) == ARG  # a capacity without a buffer
        assert fn(n=-1) == ARG and fn(G=-1) == ARG and fn(cap=-1) == ARG
        assert fn(seq_=None) == ARG
        assert b"null sequences" in lib.ldpc_last_error()
        assert fn(ln_=np.array([4, -1, 4], np.int32)) == ARG
        assert fn(off_=np.array([0, -4, 7], np.int64)) == ARG
        assert fn(off_=np.array([0, 4, 2**63 - 2], np.int64)) == ARG
        assert b"overflowing" in lib.ldpc_last_error()
        assert fn(gp_=np.array([1, 3], np.int64)) == ARG and fn(gp_=np.array([0, 2], np.int64)) == ARG
        assert fn(gp_=np.array([0, 4], np.int64)) == ARG
        assert b"group_ptr" in lib.ldpc_last_error()
        assert fn(gp_=np.array([0, 5, 3], np.int64), G=2, ce_=np.zeros(2, np.int32), wd_=np.zeros(2, np.int32),
                  op_=np.zeros(3, np.int64)) == ARG
        assert b"monotone" in lib.ldpc_last_error()
        assert fn(G=0, gp_=None) == ARG  # sequences outside every group
        assert fn(n=0, G=0, seq_=None, off_=None, ln_=None, gp_=None, ce_=None, wd_=None, op_=None, out_=None,
                  cap=0, dist_=None) == OK  # nothing to do, no device needed
        assert need.value == 0
    assert dev(ws=-1) == ARG
    assert b"workspace_bytes" in lib.ldpc_last_error()
    # a buffer that is too small: LDPC_ERR_ARG, the needed size and everything but the rows reported
    ce[:], wd[:], op[:], dist[:], out[:] = 9, 9, 9, 9, 0
    need.value = -1
    assert host(cap=11) == ARG
    assert b"the rows need 12" in lib.ldpc_last_error()
    assert (need.value, ce.tolist(), wd.tolist(), op.tolist(), dist.tolist()) == (12, [0], [4], [0, 12], [0, 1, 1])
    assert not out.any()
    assert host(out_=None, cap=0) == ARG and need.value == 12  # the size query
    assert host(cap=12) == OK and out[:12].tobytes() == b"ACGTAC-TAGGT"
    # the device entry: no such device, and without a GPU a clear device error
    assert dev(device=1 << 20) == L.LDPC_ERR_DEVICE and dev(device=-1) == L.LDPC_ERR_DEVICE
    if L.device_count() < 1:
        assert dev() == L.LDPC_ERR_DEVICE
        with pytest.raises(L.LdpcError) as e:
            llr_mod.star_align_groups([["AC", "A"]])
        assert e.value.code == L.LDPC_ERR_DEVICE
    else:
        assert dev() == OK and out[:12].tobytes() == b"ACGTAC-TAGGT"


def _host_distance(seqs, pairs):
    return np.array([star_ref.distance(seqs[a], seqs[b]) for a, b in pairs], np.int32)


def test_plan_llr_with_star_on_hand_made_strands(llr_mod):
    """plan_llr(align_fn="star") with the distances from a host DP: no GPU.  A
    ragged strand whose short reads only miss bases gets 136-wide aligned
    rows, all of them counted; a strand with an insertion against its centre
    is 137 wide and fails the reference's length rule (decoder.py:209-214):
    only the rows' last characters survive."""
    rng = np.random.default_rng(2)
    sidx = llr_mod.strand_indices()
    a, b, c = ("".join(rng.choice(list("ACGT"), 136)) for _ in range(3))
    b = b[:-2] + "CG"  # no homopolymer at the end: a missing last base leaves its gap in the last column
    idx, seqs, quals = [], [], []

    def add(strand, s, q):
        idx.append(int(sidx[strand])); seqs.append(s); quals.append(q)

    add(10, a, 70); add(10, a[:40] + a[41:], 66); add(10, a[:99] + a[101:], 60)      # deletions only
    add(20, b, 70); add(20, b[:50] + "T" + b[50:], 67); add(20, b[:-1], 64)            # one insertion
    add(30, c, 70); add(30, "".join(rng.choice(list("ACGT"), 120)), 70)                # ragged, no close pair
    plan = llr_mod.plan_llr(idx, seqs, quals, align_fn="star", distance_fn=_host_distance)
    assert plan.kind[10] == llr_mod.KIND_COUNT and plan.kind[20] == llr_mod.KIND_ALIGN_FAILED
    assert plan.kind[30] == llr_mod.KIND_NONE and (np.delete(plan.kind, [10, 20, 30]) == llr_mod.KIND_NONE).all()
    assert plan.n_aligned_strands == 2 and plan.n_align_pairs == 4 and plan.t_align_s > 0
    r10 = [plan.rows[r].tobytes().decode() for r in range(plan.row_ptr[10], plan.row_ptr[11])]
    assert r10 == [rec for _, rec in star_ref.star_align(seqs[:3])] and all(len(r) == 136 for r in r10)
    assert r10[0] == a and [r.replace("-", "") for r in r10] == seqs[:3] and [r.count("-") for r in r10] == [0, 1, 2]
    assert plan.row_q[plan.row_ptr[10]:plan.row_ptr[11]].tolist() == [70, 66, 60]
    # strand 20: width 137, every row fails; byte 0 of a failed row is its last character
    rec20 = star_ref.star_align(seqs[3:6])
    assert all(len(r) == 137 for _, r in rec20)
    r20 = [chr(plan.rows[r, 0]) for r in range(plan.row_ptr[20], plan.row_ptr[21])]
    assert r20 == [r[-1] for _, r in rec20] == [b[-1], b[-1], "-"]
    assert plan.row_q[plan.row_ptr[20]:plan.row_ptr[21]].tolist() == [70, 67, 64]
    # the same plan from the reference aligner as a callable; a callable and None behave as before
    ref = llr_mod.plan_llr(idx, seqs, quals, align_fn=star_ref.star_align, distance_fn=_host_distance)
    assert np.array_equal(ref.kind, plan.kind) and np.array_equal(ref.rows, plan.rows)
    assert np.array_equal(ref.row_q, plan.row_q) and np.array_equal(ref.row_ptr, plan.row_ptr)
    assert ref.n_align_pairs == 0
    with pytest.raises(RuntimeError):
        llr_mod.plan_llr(idx, seqs, quals, align_fn=None, distance_fn=_host_distance)
    with pytest.raises(ValueError):
        llr_mod.plan_llr(idx, seqs, quals, align_fn="muscle", distance_fn=_host_distance)
