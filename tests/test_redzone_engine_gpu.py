"""Red zones around every device pointer of the engine's entry points
(DESIGN.md sec. 9): ldpc_engine_decode (IN_LLR, IN_LR), ldpc_engine_decode_codes,
ldpc_engine_gen_bsc / _codes and ldpc_encoder_encode_device.

Every buffer is a redzone.DeviceGuard: 4 KiB bands on both sides, outputs
poisoned before each call, inputs compared byte for byte afterwards.  Each
engine first decodes another batch of the same shape (the decoy: what it leaves
in the engine's expanded priors, lane codes and posterior staging is wrong data
for the checked call), then the checked batch, whose outputs must equal the
CPU oracle under the rules of test_real_llr_gpu._same -- so a row a schedule
never stores holds poison or nothing at all, never a stale correct value.
No tolerance anywhere; nothing here can touch memory the test does not own.
"""
import numpy as np
import pytest

import gf2_ref
import redzone as Z
import redzone_cases as RC
import synth
from test_random_graphs_gpu import GEN_SCHEDULES, SCHEDULES

pytestmark = pytest.mark.gpu

CODES = ("reg4", "reg2", "irr", "n13", "bucket")
REGULAR = ("reg4", "reg2")
B = RC.B
SHORT = 37


@pytest.fixture(scope="module")
def cases(gpu, oracle_mod, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("redzone_engine")
    made = {}

    def get(name):
        if name not in made:
            made[name] = RC.Case(name, gpu, oracle_mod, tmp)
        return made[name]
    return get


def schedules(name, algo):
    """(schedule keywords, chunk) of a code and an algorithm."""
    if RC.ALGOS[algo] >= 2:  # the integer decoders run fixed passes whatever the schedule says
        return [({}, 64), ({}, 192), ({"group_tiles": 1}, 64), ({"continuous": False}, 192)]
    out = []
    for s in (SCHEDULES if name in REGULAR else GEN_SCHEDULES):
        s = dict(s)
        chunk = s.pop("_chunk", None)
        out += [(s, c) for c in ((64, 192) if chunk is None else (chunk,))]
    if name == "reg4" and algo == "bp":
        out += [({"handover": h, "fuse_row_block": f}, c) for h in (True, False) for f in (True, False) for c in (64, 192)]
    return out


class Buffers:
    """The guarded device buffers of one decode call of up to nb codewords."""

    def __init__(self, L, N, nb, hard=0, valid=0, codes=0):
        self.N, self.nb = N, nb
        self.fp = Z.DeviceGuard(L, 0, nb * N * 8, name="d_in")
        self.codes = Z.DeviceGuard(L, 0, nb * N, codes, name="d_codes")
        self.hard = Z.DeviceGuard(L, 0, nb * N, hard, name="d_hard")
        self.post = Z.DeviceGuard(L, 0, nb * N * 8, name="d_post")
        self.iters = Z.DeviceGuard(L, 0, nb * 4, name="d_iters")
        self.valid = Z.DeviceGuard(L, 0, nb, valid, name="d_valid")
        self.all = (self.fp, self.codes, self.hard, self.post, self.iters, self.valid)

    def free(self):
        for g in self.all:
            g.free()


def run(L, eng, bufs, case, seed, algo, entry, nb, want_post):
    """One guarded call on rows [0, nb) of the seed's input; returns
    (hard, post or None, iters, valid) of those rows."""
    N, cap = bufs.N, bufs.nb
    bp = algo == "bp"
    post_kind = L.POST_RATIO if bp else L.POST_LLR
    for g in (bufs.hard, bufs.post, bufs.iters, bufs.valid):
        g.fill()
    d_post = bufs.post.ptr if want_post else None
    out = (bufs.hard.ptr, d_post, post_kind, bufs.iters.ptr, bufs.valid.ptr)
    if entry == "codes":
        src, inp = case.codes[seed], bufs.codes
        inp.fill(src)
        eng.decode_codes(inp.ptr, RC.TABLE, L.IN_LLR, nb, case.max_iter, *out)
    else:
        src, inp = (case.lr(seed), bufs.fp) if entry == "lr" else (case.llr[seed], bufs.fp)
        inp.fill(src)
        eng.decode(inp.ptr, L.IN_LR if entry == "lr" else L.IN_LLR, nb, case.max_iter, *out)
    eng.sync()
    inp.check_unchanged(src)
    for g in bufs.all:
        g.check_bands()
    # rows past the batch, and a posterior that was not asked for, were not written
    bufs.hard.check_poison(nb * N)
    bufs.iters.check_poison(nb * 4)
    bufs.valid.check_poison(nb)
    bufs.post.check_poison(nb * N * 8 if want_post else 0)
    return (bufs.hard.payload(np.uint8, (cap, N))[:nb], bufs.post.payload(np.float64, (cap, N))[:nb] if want_post else None,
            bufs.iters.payload(np.int32)[:nb], bufs.valid.payload(np.uint8)[:nb])


def entries(algo, k):
    """(entry form, with posterior) of run k: every form with and without d_post over two runs."""
    if algo == "gallager_b1":  # no posterior
        return [("llr", False), ("codes", False)]
    e = [("llr", True), ("codes", k % 2 == 0)]
    if algo == "bp":
        e.append(("lr", k % 2 == 1))
    return e + ([("llr", False)] if k == 0 else [])


def checked(L, case, bufs, algo, sch, chunk, k, nbs=(B,)):
    """A fresh engine: the decoy batch, then the checked one, per entry form of run k."""
    eng = L.Engine(case.G, 0, algo, chunk=chunk, schedule=sch)
    try:
        if algo == "qmsa":
            eng.set_params(*RC.QPARAMS, tie_seed=RC.TIE_SEED)
        for entry, want_post in entries(algo, k):
            for nb in nbs:
                got = Z.decoy_then(lambda seed: run(L, eng, bufs, case, seed, algo, entry, nb, want_post),
                                   (RC.DECOY,), (RC.REAL,))
                RC.same(got, case.ref(RC.REAL, algo), (case.name, algo, sch, chunk, entry, nb, want_post), rows=nb)
    finally:
        eng.close()


@pytest.mark.timeout(120)
@pytest.mark.parametrize("algo", sorted(RC.ALGOS))
@pytest.mark.parametrize("name", CODES)
def test_decode_every_schedule(gpu, cases, name, algo):
    """B = 165 = 2 x 64 + 37 over pools of 64 and 192 lanes, every schedule
    family, every entry form, with and without d_post, everything at shift 0."""
    case = cases(name)
    case.assert_nonconstant(algo)
    bufs = Buffers(gpu, case.N, B)
    try:
        for k, (sch, chunk) in enumerate(schedules(name, algo)):
            checked(gpu, case, bufs, algo, sch, chunk, k)
    finally:
        bufs.free()


@pytest.mark.timeout(120)
@pytest.mark.parametrize("algo", sorted(RC.ALGOS))
@pytest.mark.parametrize("name", CODES)
def test_decode_short_batches_leave_the_rest_poisoned(gpu, cases, name, algo):
    """One engine decodes 165 words and then 37, and then one, into freshly
    poisoned 165-row buffers: rows from 37 (from 1) on are still poison, and
    the rows written are the checked input's, not the 165-word call's."""
    case = cases(name)
    case.assert_nonconstant(algo)
    bufs = Buffers(gpu, case.N, B)
    try:
        for k, (sch, chunk) in enumerate(schedules(name, algo)[:4]):
            checked(gpu, case, bufs, algo, sch, chunk, k, nbs=(B, SHORT, 1))
    finally:
        bufs.free()


# device pointers the header gives no alignment for, off their natural places
# (fp64 and int32 pointers stay aligned)
PLACEMENTS = [dict(hard=1, valid=1, codes=1), dict(hard=3, codes=5)]


@pytest.mark.timeout(120)
@pytest.mark.parametrize("place", range(len(PLACEMENTS)))
@pytest.mark.parametrize("algo", sorted(RC.ALGOS))
@pytest.mark.parametrize("name", CODES)
def test_decode_misaligned_byte_pointers(gpu, cases, name, algo, place):
    """d_hard at +1 / +3 (the finished lanes' 2/4/8-byte stores fall back to
    bytes), d_valid at +1, d_codes at +1 / +5 (k_lr_table's 8-byte loads fall
    back to bytes; the refills and k_fill_codes read bytes)."""
    case = cases(name)
    bufs = Buffers(gpu, case.N, B, **PLACEMENTS[place])
    try:
        sch = schedules(name, algo)
        some = [sch[0], sch[-1]] + [x for x in sch if x[0] in ({"continuous": False}, {"resident": False})][:2]
        for k, (s, chunk) in enumerate(some):
            checked(gpu, case, bufs, algo, s, chunk, k)
    finally:
        bufs.free()


# ---------------------------------------------------------------------------
# the synthetic channel
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, 1])
def test_gen_bsc_red_zones(gpu, cases, shift):
    """B x N = 7 x 13 (odd), b0 = 12345, 5 codewords (the index wraps): fp64
    of both kinds and int8 codes equal to synth.bsc_llrs; the codewords are
    unchanged (at shift 1 they and the codes sit on odd addresses)."""
    L, case = gpu, cases("n13")
    N, nb, b0, n_cw, seed, p, mag = case.N, 7, 12345, 5, 2026, 0.3, 1.75
    cw = case.G.encoder().encode_host(synth.random_messages(case.G.encoder().K, 0, n_cw, 9))
    Z.nonconstant(cw)
    eng = L.Engine(case.G, 0, "bp", chunk=64)
    d_cw = Z.DeviceGuard(L, 0, cw.size, shift, data=cw, name="d_codewords")
    d_fp = Z.DeviceGuard(L, 0, nb * N * 8, name="d_out fp64")
    d_codes = Z.DeviceGuard(L, 0, nb * N, shift, name="d_out codes")
    try:
        for dseed, rseed in ((seed + 1, seed),) * 2:  # the decoy seed, then the checked one
            for kind, as_lr in ((L.IN_LLR, False), (L.IN_LR, True)):
                want = synth.bsc_llrs(cw, b0, nb, seed=rseed, p=p, mag=mag, as_lr=as_lr)
                Z.nonconstant(want)
                eng.gen_bsc(d_fp.ptr, kind, b0, nb, d_cw.ptr, n_cw, dseed, p, mag)
                eng.sync()
                d_fp.fill()
                eng.gen_bsc(d_fp.ptr, kind, b0, nb, d_cw.ptr, n_cw, rseed, p, mag)
                eng.sync()
                assert np.array_equal(d_fp.payload(np.float64, (nb, N)).view(np.uint64), want.view(np.uint64)), kind
                d_fp.check_bands()
                d_cw.check_unchanged(cw)
            want = np.where(synth.bsc_llrs(cw, b0, nb, seed=rseed, p=p, mag=mag) < 0, -1, 1).astype(np.int8)
            eng.gen_bsc_codes(d_codes.ptr, b0, nb, d_cw.ptr, n_cw, dseed, p)
            eng.sync()
            d_codes.fill()
            eng.gen_bsc_codes(d_codes.ptr, b0, nb, d_cw.ptr, n_cw, rseed, p)
            eng.sync()
            assert np.array_equal(d_codes.payload(np.int8, (nb, N)), want)
            d_codes.check_bands()
            d_cw.check_unchanged(cw)
    finally:
        eng.close()
        for g in (d_cw, d_fp, d_codes):
            g.free()


# ---------------------------------------------------------------------------
# the encoder on device buffers
# ---------------------------------------------------------------------------
ENC_GRAPHS = ("r37x100", "r65x129", "rs_5_16_4")


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("name", ENC_GRAPHS)
def test_encode_device_red_zones(gpu, name, shift):
    """B in 1, 63, 65, 130; messages at shift 0 and 1: k_enc_pack's 4-byte
    loads are on only at shift 0 with K % 4 == 0 (K = 64 of r65x129; r37x100
    has K = 63 and the RS-LDPC code 397, so their rows past the first sit off
    4-byte alignment either way).  The engine's stream and the library's own.
    Codewords equal encode_host, messages unchanged."""
    L = gpu
    G = gf2_ref.small_graph(L, name)
    enc = G.encoder()
    assert (enc.K % 4 == 0) == (name == "r65x129")
    eng = L.Engine(G, 0, "bp", chunk=64)
    try:
        for nb in (1, 63, 65, 130):
            msg = {s: synth.random_messages(enc.K, 0, nb, s) for s in (RC.REAL, RC.DECOY)}
            want = enc.encode_host(msg[RC.REAL])
            Z.nonconstant(want)
            d_msg = Z.DeviceGuard(L, 0, nb * enc.K, shift, name="d_msg")
            d_cw = Z.DeviceGuard(L, 0, nb * enc.N, shift, name="d_cw")
            for stream in (eng.stream, None):
                for s in (RC.DECOY, RC.REAL):  # the decoy leaves its ballots in the encoder's workspace
                    d_msg.fill(msg[s])
                    d_cw.fill()
                    enc.encode_device(d_msg.ptr, nb, d_cw.ptr, device=0, stream=stream)
                    if stream is not None:
                        eng.sync()
                assert np.array_equal(d_cw.payload(np.uint8, (nb, enc.N)), want), (name, nb, stream)
                d_cw.check_bands()
                d_msg.check_unchanged(msg[RC.REAL])
            d_msg.free()
            d_cw.free()
    finally:
        eng.close()
