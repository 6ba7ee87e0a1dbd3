"""Hand-over (LDPC_SCHED_HANDOVER, resident pool on the (8,72)-regular path):
a lane whose codeword enters its max_iter-th update claims its next codeword
in that step, the variable kernel writes the finished outputs and
initialises the new codeword in one launch, and the codeword's last syndrome
(its valid flag) follows in the next check.  A codeword that does not converge
then holds its lane for max_iter steps instead of max_iter + 1.  Nothing a
codeword computes changes: every case equals the oracle and the schedule
without the flag bit for bit (hard bits, iterations, valid flags, posterior)."""
import numpy as np
import pytest

import synth
from test_gpu_parity import _cmp

pytestmark = pytest.mark.gpu

POOL = 192                 # the resident pool's 3 tiles
B_MIX = 2 * POOL + 37      # two pool fills and a partial last tile

# (algorithm, schedule): BP on coded and fp64 input, fp64 min-sum likewise
KINDS = {
    "bp-coded": ("bp", {}),
    "bp-fp64": ("bp", {"lr_table": False}),
    "msa-coded": ("msa", {"msa_compressed": False}),
    "msa-fp64": ("msa", {"msa_compressed": False, "lr_table": False}),
}


@pytest.fixture(scope="module")
def mixed(codewords):
    """Rows alternate between hopeless ones (BSC p = 0.02: no decoder gets
    there in 3 iterations) and noiseless codewords (valid at iteration 0):
    hand-overs into a codeword that finishes at once, hand-overs beside
    early-exiting neighbours in the same 16-lane line, a drain with pending
    syndromes and no claim, a partial last tile."""
    llr = synth.bsc_llrs(codewords, 0, B_MIX, seed=77, p=0.02)
    llr[1::2] = synth.bsc_llrs(codewords, 0, B_MIX, seed=77, p=0.0)[1::2]
    llr = np.ascontiguousarray(llr)
    llr.setflags(write=False)
    return llr


def _both(G, og, llr, max_iter, algo, sch):
    """Flag on and off, posterior on and off: all equal the oracle."""
    out = {}
    for ho in (True, False):
        s = dict(sch, resident=True, handover=ho)
        h, p, it, v = _cmp(G, og, llr, max_iter, algo=algo, chunk=POOL, schedule=s)
        h2, p2, it2, v2 = G.decode(llr, max_iter=max_iter, algo=algo, post=None, chunk=POOL, schedule=s)
        assert p2 is None
        assert np.array_equal(h2, h) and np.array_equal(it2, it) and np.array_equal(v2, v)
        out[ho] = (h, p, it, v)
    for a, b in zip(out[True], out[False]):
        assert np.array_equal(a.view(np.uint64) if a.dtype == np.float64 else a,
                              b.view(np.uint64) if b.dtype == np.float64 else b)
    return out[True]


@pytest.mark.timeout(120)
@pytest.mark.parametrize("max_iter", [1, 3])
@pytest.mark.parametrize("kind", sorted(KINDS))
def test_mixed_handover(G, og, mixed, kind, max_iter):
    algo, sch = KINDS[kind]
    _, _, it, v = _both(G, og, mixed, max_iter, algo, sch)
    assert (it[0::2] == max_iter).all() and not v[0::2].any()  # every hopeless row went through the hand-over
    assert (it[1::2] == 0).all() and v[1::2].all()


@pytest.mark.timeout(120)
@pytest.mark.parametrize("max_iter", [0, 1])
@pytest.mark.parametrize("kind", ["bp-coded", "msa-fp64"])
def test_no_last_stage_and_last_at_first_step(G, og, mixed, kind, max_iter):
    """max_iter = 0: no lane ever has a final update; max_iter = 1: the step
    after a lane's Init is already its last."""
    algo, sch = KINDS[kind]
    _, _, it, _ = _both(G, og, mixed[:70], max_iter, algo, sch)
    assert (it[0::2] == max_iter).all()


def _check_launches(L, G, codes, table, max_iter, handover):
    B, N = codes.shape
    d_in = L.DeviceBuffer(0, B * N)
    d_in.upload(codes)
    d_h, d_i, d_v = L.DeviceBuffer(0, B * N), L.DeviceBuffer(0, B * 4), L.DeviceBuffer(0, B)
    eng = L.Engine(G, 0, "bp", handover=handover)
    try:
        assert eng.resident and eng.handover == handover and eng.cap == POOL
        n0 = eng.stats()["check"]["launches"]
        eng.decode_codes(d_in.at(0), table, L.IN_LLR, B, max_iter, d_h.at(0), None, L.POST_LLR, d_i.at(0), d_v.at(0))
        eng.sync()
        n = eng.stats()["check"]["launches"] - n0
        out = (d_h.download(np.empty((B, N), np.uint8)), d_i.download(np.empty(B, np.int32)),
               d_v.download(np.empty(B, np.uint8)))
    finally:
        eng.close()
        for b in (d_in, d_h, d_i, d_v):
            b.free()
    return n, out


@pytest.mark.timeout(120)
def test_step_count(gpu, G, codewords):
    """G = 4 pool generations of codewords that all run to max_iter = 4: each
    generation takes one step less with the hand-over, but for the first Init
    step and the last pending step; the host's poll lag is the same on both
    sides.  So the check kernel is launched at least G - 2 times less."""
    L = gpu
    gens, max_iter = 4, 4
    B = gens * POOL - 50
    llr = synth.bsc_llrs(codewords, 0, B, seed=2026, p=0.02)
    codes = np.ascontiguousarray(np.where(llr > 0, 1, -1).astype(np.int8))
    table = np.arange(-128, 128, dtype=np.float64) * synth.LLR_UNIT
    n_off, out_off = _check_launches(L, G, codes, table, max_iter, False)
    n_on, out_on = _check_launches(L, G, codes, table, max_iter, True)
    print(f"check launches: hand-over off {n_off}, on {n_on}")
    for a, b in zip(out_on, out_off):
        assert np.array_equal(a, b)
    assert (out_on[1] == max_iter).all() and not out_on[2].any()
    assert n_off - n_on >= gens - 2, (n_off, n_on)


@pytest.mark.timeout(120)
def test_flag_resolution(gpu, G):
    """On only where the kernels that implement it run: the resident pool's
    (8,72)-regular BP / fp64 min-sum."""
    L = gpu

    def resolved(g, algo, **kw):
        eng = L.Engine(g, 0, algo, **kw)
        try:
            assert bool(eng.flags & L.SCHED_FLAGS["handover"]) == eng.handover
            return eng.handover
        finally:
            eng.close()

    assert resolved(G, "bp") is True
    assert resolved(G, "msa", msa_compressed=False) is True
    assert resolved(G, "bp", handover=False) is False
    assert resolved(G, "bp", resident=False) is False
    assert resolved(G, "msa") is False                      # compressed min-sum
    assert resolved(L.Graph.rs_ldpc(6, 32, 4), "bp") is False  # generic resident kernels
