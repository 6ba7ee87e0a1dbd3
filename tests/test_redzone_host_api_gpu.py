"""Red zones around every host pointer of the host-buffer entry points
(DESIGN.md sec. 9): ldpc_decode, ldpc_decode_codes, ldpc_encode,
ldpc_ber_run_range, ldpc_ber_read and ldpc_ber_frame_errors, called through
ctypes on redzone.HostGuard arrays (the Python wrappers allocate their own
outputs, and np.empty may hand a call the previous call's correct result).

Outputs are poisoned before each call and every call is preceded by a decoy
call on another input of the same shape, so what the slot's pinned staging
halves and device buffers carry from one call into the next is wrong data.
Every comparison is exact.
"""
import ctypes as C

import numpy as np
import pytest

import channel_cases as cc
import gf2_ref
import redzone as Z
import redzone_cases as RC
import synth

pytestmark = pytest.mark.gpu

X = 4096  # codewords per PCIe chunk (test_host_pipeline_gpu)
BATCHES = (1, 65, X + 37)  # the last: two chunks, so a staging half's neighbour is reused
NULLS = (None, "post", "iters", "valid")


@pytest.fixture(scope="module")
def cases(gpu, oracle_mod, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("redzone_host")
    made = {}

    def get(name):
        if name not in made:
            made[name] = RC.Case(name, gpu, oracle_mod, tmp, nb=X + 37)
        return made[name]
    return get


def _opts(L, algo, devices):
    o = L.Opts()
    keep = None
    if devices:
        keep = (C.c_int32 * len(devices))(*devices)
        o.n_devices = len(devices)
        o.devices = C.cast(keep, C.POINTER(C.c_int32))
    o.exp_on_host = 1
    o.post_kind = L.POST_RATIO if algo == "bp" else L.POST_LLR
    if algo == "qmsa":
        o.msa_precision, o.msa_step, o.msa_offset = RC.QPARAMS
        o.tie_seed = RC.TIE_SEED
    return o, keep


def host_decode(L, case, seed, algo, nb, entry, pinned, devices, null):
    """One guarded ldpc_decode / ldpc_decode_codes of rows [0, nb); returns
    (hard, post, iters, valid), None for the output passed as NULL."""
    N = case.N
    src = (case.codes[seed] if entry == "codes" else case.llr[seed])[:nb]
    inp = Z.HostGuard(src.shape, src.dtype, pinned=pinned, data=src, name=entry)
    table = Z.HostGuard(256, np.float64, data=RC.TABLE, name="table")
    out = {"hard": Z.HostGuard((nb, N), np.uint8, name="hard_out"), "post": Z.HostGuard((nb, N), np.float64, name="post_out"),
           "iters": Z.HostGuard(nb, np.int32, name="iters_out"), "valid": Z.HostGuard(nb, np.uint8, name="valid_out")}
    ptr = {k: (None if k == null else g.ptr) for k, g in out.items()}
    o, keep = _opts(L, algo, devices)
    a = int(L.Algo[algo.upper()])
    if entry == "codes":
        rc = L.lib().ldpc_decode_codes(case.G.handle, inp.ptr, table.ptr, L.IN_LLR, nb, case.max_iter, a, ptr["hard"],
                                       ptr["post"], ptr["iters"], ptr["valid"], C.byref(o))
    else:
        rc = L.lib().ldpc_decode(case.G.handle, inp.ptr, nb, case.max_iter, a, ptr["hard"], ptr["post"], ptr["iters"],
                                 ptr["valid"], C.byref(o))
    del keep
    assert rc == L.LDPC_OK, (rc, L.lib().ldpc_last_error())
    inp.check_unchanged(src)
    table.check_unchanged(RC.TABLE)
    for k, g in out.items():
        g.check_bands()
        if k == null:
            g.check_poison()
    return tuple(None if k == null else out[k].payload(out[k].dtype, out[k].shape) for k in ("hard", "post", "iters", "valid"))


def _same(got, ref, what, nb):
    """redzone_cases.same with the outputs that were passed as NULL left out."""
    h, p, it, v = got
    rh, rp, rit, rv = (None if r is None else r[:nb] for r in ref)
    assert np.array_equal(h, rh), (what, "hard")
    if it is not None:
        assert np.array_equal(it, rit), (what, "iters", it, rit)
    if v is not None:
        assert np.array_equal(v, np.asarray(rv, np.uint8)), (what, "valid")
    if p is not None:
        nan = np.isnan(rp)
        assert np.array_equal(np.isnan(p), nan), (what, "posterior NaNs")
        assert np.array_equal(p[~nan].view(np.uint64), rp[~nan].view(np.uint64)), (what, "posterior")


@pytest.mark.timeout(120)
@pytest.mark.parametrize("algo", ["bp", "msa", "qmsa"])
@pytest.mark.parametrize("name", ["n64", "n65"])
def test_host_decode_red_zones(gpu, cases, name, algo):
    """N = 64 (hard bits cross PCIe packed) and 65 (unpacked); B = 1, 65 and
    4096 + 37 (two chunks); one device and two shards on it; pageable and
    pinned input; all outputs, and each optional one NULL in turn."""
    case = cases(name)
    case.assert_nonconstant(algo)
    ref = case.ref(RC.REAL, algo)
    k = 0
    for nb in BATCHES:
        assert len(np.unique(ref[2][:nb])) >= min(nb, 3) and (nb == 1 or 0 < ref[3][:nb].sum() < nb)
        for entry in ("llr", "codes"):
            for devices in (None, [0, 0]):
                for pinned in (False, True):
                    null = NULLS[k % len(NULLS)]
                    k += 1
                    what = (name, algo, nb, entry, devices, pinned, null)
                    got = Z.decoy_then(lambda seed: host_decode(gpu, case, seed, algo, nb, entry, pinned, devices, null),
                                       (RC.DECOY,), (RC.REAL,))
                    _same(got, ref, what, nb)


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("name", ["r37x100", "r65x129", "rs_5_16_4"])
def test_host_encode_red_zones(gpu, name, shift):
    """ldpc_encode at the encoder shapes of test_redzone_engine_gpu, message
    and codeword arrays at shift 0 and 1."""
    L = gpu
    enc = gf2_ref.small_graph(L, name).encoder()
    for nb in (1, 63, 65, 130):
        msg = {s: synth.random_messages(enc.K, 0, nb, s) for s in (RC.REAL, RC.DECOY)}
        want = enc.encode_host(msg[RC.REAL])
        Z.nonconstant(want)
        for s in (RC.DECOY, RC.REAL):
            m = Z.HostGuard((nb, enc.K), np.uint8, shift, data=msg[s], name="msg")
            cw = Z.HostGuard((nb, enc.N), np.uint8, shift, name="cw_out")
            rc = L.lib().ldpc_encode(enc._h, m.ptr, nb, cw.ptr, 0)
            assert rc == L.LDPC_OK, (rc, L.lib().ldpc_last_error())
            m.check_unchanged(msg[s])
            cw.check_bands()
        assert np.array_equal(cw.payload(np.uint8, (nb, enc.N)), want), (name, nb)


@pytest.mark.parametrize("nb", [70, 5])
@pytest.mark.parametrize("name", ["n13", "irr"])
def test_ber_red_zones(gpu, oracle_mod, tmp_path, name, nb):
    """ldpc_ber_run_range's records [B], ldpc_ber_read's three matrices and
    ldpc_ber_frame_errors' inputs and records, on N = 13 and the irregular
    code; a decoy range on another seed first."""
    L = gpu
    path = cc.pchk(tmp_path, name)
    G, og = L.Graph(path), oracle_mod.OracleGraph(path)
    enc = G.encoder()
    N = G.N
    mask = np.zeros(N, np.uint8)
    mask[enc.info_pos] = 1
    thr, table = synth.awgn_channel(2.0, enc.K / N)
    thr = np.ascontiguousarray(thr, np.uint64)
    table = np.ascontiguousarray(table, np.float64)
    er = L.ErrorRate(G, algo="bp", batch=nb, encoder=enc)
    lib = L._ber_lib()
    try:
        b0, seed = 3, 11
        want = cc.reference_records(og, enc, (thr, table), "bp", seed, b0, nb)
        if nb > 8:
            assert (want["bit_err"] > 0).any() and (want["bit_err"] == 0).any() and len(set(want["iters"])) >= 3
        g_thr = Z.HostGuard(254, np.uint64, data=thr, name="thr")
        g_tab = Z.HostGuard(256, np.float64, data=table, name="table")
        for s in (seed + 1, seed):
            rec = Z.HostGuard(nb, L.BER_RECORD, name="records")
            rc = lib.ldpc_ber_run_range(er._h, g_thr.ptr, g_tab.ptr, L.IN_LLR, s, b0, nb, cc.MAX_ITER, rec.ptr)
            assert rc == L.LDPC_OK, (rc, L.lib().ldpc_last_error())
            rec.check_bands()
        g_thr.check_unchanged(thr)
        g_tab.check_unchanged(table)
        assert np.array_equal(rec.payload(L.BER_RECORD), want)
        # the last batch's matrices
        cw_ref = synth.random_codewords(enc, b0, nb, seed)
        codes_ref = synth.channel_codes(cw_ref, b0, nb, seed, thr)
        hard_ref, _, _ = cc.oracle_decode(og, "bp")(codes_ref, table, 0, b0, cc.MAX_ITER)
        Z.nonconstant(cw_ref), Z.nonconstant(hard_ref)
        outs = [Z.HostGuard((nb, N), dt, shift, name=nm) for nm, dt, shift in
                (("cw", np.uint8, 1), ("codes", np.int8, 3), ("hard", np.uint8, 5))]
        rc = lib.ldpc_ber_read(er._h, nb, *[g.ptr for g in outs])
        assert rc == L.LDPC_OK, (rc, L.lib().ldpc_last_error())
        for g, ref in zip(outs, (cw_ref, codes_ref, hard_ref)):
            g.check_bands()
            assert np.array_equal(g.payload(ref.dtype, (nb, N)), ref), g.name
        # the error counter alone, on host arrays
        rng = np.random.default_rng(70 + N)
        hard, cw, codes, iters, valid = cc.planted(rng, max(nb, 5), N, mask)
        ins = [(a, Z.HostGuard(a.shape, a.dtype, shift, data=a, name=nm)) for nm, a, shift in
               (("hard", hard[:nb], 1), ("cw", cw[:nb], 0), ("codes", codes[:nb], 3), ("table", table, 0),
                ("iters", iters[:nb], 0), ("valid", valid[:nb], 1))]
        g = dict((x[1].name, x[1]) for x in ins)
        for decoy in (True, False):
            if decoy:
                g["hard"].fill(1 - hard[:nb])
            else:
                g["hard"].fill(hard[:nb])
            rec = Z.HostGuard(nb, L.BER_RECORD, name="records")
            rc = lib.ldpc_ber_frame_errors(er._h, g["hard"].ptr, g["cw"].ptr, g["codes"].ptr, g["table"].ptr, L.IN_LLR,
                                           g["iters"].ptr, g["valid"].ptr, nb, rec.ptr)
            assert rc == L.LDPC_OK, (rc, L.lib().ldpc_last_error())
            rec.check_bands()
        for a, guard in ins:
            guard.check_unchanged(a)
        want = cc.count(hard[:nb], cw[:nb], codes[:nb], mask, table, iters[:nb], valid[:nb])
        assert len(np.unique(want["bit_err"])) > 2
        assert np.array_equal(rec.payload(L.BER_RECORD), want)
    finally:
        er.close()
