"""The GPU decoders against the REFERENCE's own decoders, without the oracle
in between: tests/golden/refdec_goldens.npz holds what dec.cpp, compiled
unmodified (oracle/ref_dec_harness.cpp), computed for the inputs of
tests/refdec_cases.py.  Hard bits, iteration counts and valid flags are equal,
and so are the posterior bytes (BP's ratio, the min-sum's L, the quantised
min-sum's L_Q; a NaN matches a NaN).  Nothing here needs the reference or
oracle/_ref.

Small codes (reg4: specialised kernels, resident pool, hand-over, fused row
block; perm4: the fused row block resolves off; rs5 = RS-LDPC(5, 16, 4); irr:
generic buckets, a degree-1 row, an empty row, an empty column) at
B = 2 * 64 + 37 over pools of 64 and 192 lanes, and the DNA code once with 8
words.  BP takes fp64 likelihood ratios (IN_LR) on device buffers, and int8
codes with a 256-entry table of likelihood ratios; neither side computes an
exp.  Quantised min-sum is compared in full on the words where the reference
drew no tie bit, and on L_Q and the hard bits off zero posteriors where the
tie hash led to the reference's iteration count."""
import numpy as np
import pytest

import refdec_cases as R

pytestmark = pytest.mark.gpu

CHUNKS = (64, 192)
GALLAGER_NAME = {"ga": "gallager_a", "gb1": "gallager_b1", "gb2": "gallager_b2"}


@pytest.fixture(scope="module")
def fx():
    z = np.load(R.FIXTURE)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def cases(gpu, fx, tmp_path_factory):
    """name -> (Graph, row 0's columns); generated codes come from the fixture's edge lists."""
    tmp = tmp_path_factory.mktemp("refdec_gpu")
    made = {}

    def get(name):
        if name not in made:
            if name == "dna":
                path, c0 = R.DNA_PCHK, R.pchk_row0(R.DNA_PCHK)
            else:
                path = str(tmp / f"{name}.pchk")
                rows, cols = fx[f"{name}/edges"].astype(np.int64)
                M, N = fx[f"{name}/shape"]
                R.write_pchk(path, int(M), int(N), rows, cols)
                c0 = R.row0_cols(rows, cols)
            assert R.file_sha(path) == str(fx[f"{name}/pchk_sha256"])
            made[name] = (gpu.Graph(path), c0)
        return made[name]
    return get


def _engine_bp(L, G, x, max_iter, chunk=0, codes=None, expect=None, **sch):
    """BP on device buffers: fp64 likelihood ratios x, or int8 codes with the
    table x.  Returns (hard, ratio, iters, valid); expect = flags to assert."""
    B = len(x) if codes is None else len(codes)
    src = np.ascontiguousarray(x if codes is None else codes)
    bufs = [L.DeviceBuffer(0, n) for n in (src.nbytes, B * G.N, B * G.N * 8, B * 4, B)]
    d_in, d_h, d_p, d_i, d_v = bufs
    eng = L.Engine(G, 0, "bp", chunk=chunk, **sch)
    try:
        for k, want in (expect or {}).items():
            assert getattr(eng, k) == want, (k, want, sch)
        d_in.upload(src)
        if codes is None:
            eng.decode(d_in.at(0), L.IN_LR, B, max_iter, d_h.at(0), d_p.at(0), L.POST_RATIO, d_i.at(0), d_v.at(0))
        else:
            eng.decode_codes(d_in.at(0), x, L.IN_LR, B, max_iter, d_h.at(0), d_p.at(0), L.POST_RATIO, d_i.at(0),
                             d_v.at(0))
        eng.sync()
        return (d_h.download(np.empty((B, G.N), np.uint8)), d_p.download(np.empty((B, G.N), np.float64)),
                d_i.download(np.empty(B, np.int32)), d_v.download(np.empty(B, np.uint8)))
    finally:
        eng.close()
        for b in bufs:
            b.free()


@pytest.mark.timeout(120)
@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("code", R.SMALL)
def test_bp_likelihood_ratios(gpu, fx, cases, code, chunk):
    """fp64 IN_LR input: the default schedule, the grouped continuous one, fixed
    passes, hand-over on and off, the fused row block on and off; max_iter 0,
    1 and the fixture's own."""
    G, c0 = cases(code)
    x, own = R.recorded_input(fx, code, "bp", G.N, c0)
    ref, _ = R.recorded(fx, code, "bp", G.N)
    fused = code == "reg4"  # perm4: no row block holds every column once; rs5, irr: not (8, 72)-regular
    runs = [({}, {"fused_row_block": fused}), ({"resident": False}, {"resident": False}),
            ({"continuous": False}, {"continuous": False}), ({"handover": True}, {}), ({"handover": False}, {}),
            ({"fuse_row_block": True}, {"fused_row_block": fused}),
            ({"fuse_row_block": False}, {"fused_row_block": False})]
    for sch, expect in runs:
        out = _engine_bp(gpu, G, x, own, chunk, expect=expect, **sch)
        R.compare(out, ref, None, (code, chunk, sch))
        R.compare_raw(fx, code, "bp", out)
    for m in R.SHORT["bp"]:
        for sch in ({}, {"handover": False}, {"resident": False}):
            R.compare(_engine_bp(gpu, G, x, m, chunk, **sch), R.recorded(fx, code, "bp", G.N, m)[0], None,
                     (code, chunk, sch, m))


@pytest.mark.timeout(120)
@pytest.mark.parametrize("code", R.SMALL)
def test_bp_codes_with_a_likelihood_ratio_table(gpu, fx, cases, code):
    """int8 codes and a 256-entry table in LR form (ldpc_decode_codes, IN_LR),
    with the coded variable kernel (lr_table) and without, and the same
    values as fp64."""
    G, c0 = cases(code)
    x, own = R.recorded_input(fx, code, "bpc", G.N, c0)
    codes, table = R.make_codes(code, G.N, c0, R.SEED, R.NOISE), R.lr_table()
    R.same_bits(table[codes.astype(np.int64) + 128], x, "table[codes]")
    ref, _ = R.recorded(fx, code, "bpc", G.N)
    for chunk in CHUNKS:
        for sch in ({}, {"lr_table": True}, {"lr_table": False}, {"resident": False}):
            h, p, it, v = G.decode_codes(codes, table, gpu.IN_LR, max_iter=own, algo="bp", post="ratio", chunk=chunk,
                                         schedule=sch)
            R.compare((h, p, it, v), ref, None, (code, chunk, sch))
            R.compare_raw(fx, code, "bpc", (h, p, it, v))
    R.compare(_engine_bp(gpu, G, x, own, 64), ref, None, (code, "fp64"))


@pytest.mark.timeout(120)
def test_bp_codes_on_device_buffers(gpu, fx, cases):
    """Engine.decode_codes once: reg4, fused row block on and off."""
    G, c0 = cases("reg4")
    _, own = R.recorded_input(fx, "reg4", "bpc", G.N, c0)
    codes, table = R.make_codes("reg4", G.N, c0, R.SEED, R.NOISE), R.lr_table()
    ref, _ = R.recorded(fx, "reg4", "bpc", G.N)
    for fuse in (True, False):
        out = _engine_bp(gpu, G, table, own, 64, codes=codes, expect={"fused_row_block": fuse}, fuse_row_block=fuse)
        R.compare(out, ref, None, ("reg4 device codes", fuse))


@pytest.mark.timeout(120)
@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("code", R.SMALL)
def test_min_sum(fx, cases, code, chunk):
    G, c0 = cases(code)
    x, own = R.recorded_input(fx, code, "msa", G.N, c0)
    ref, _ = R.recorded(fx, code, "msa", G.N)
    for sch in ({}, {"continuous": False}, {"msa_compressed": False}, {"resident": False}):
        out = G.decode(x, max_iter=own, algo="msa", post="llr", chunk=chunk, schedule=sch)
        R.compare(out, ref, None, (code, chunk, sch))
        R.compare_raw(fx, code, "msa", out)
    for m in R.SHORT["msa"]:
        out = G.decode(x, max_iter=m, algo="msa", post="llr", chunk=chunk)
        R.compare(out, R.recorded(fx, code, "msa", G.N, m)[0], None, (code, chunk, m))


def _integer_decoders(fx, G, c0, code, chunk):
    for algo, name in GALLAGER_NAME.items():
        x, own = R.recorded_input(fx, code, algo, G.N, c0)
        h, _, it, v = G.decode(x, max_iter=own, algo=name, post=None, chunk=chunk)
        R.compare((h, None, it, v), R.recorded(fx, code, algo, G.N)[0], None, (code, algo))
    for algo, (q, step, beta) in R.QCFG.items():
        x, own = R.recorded_input(fx, code, algo, G.N, c0)
        ref, ties = R.recorded(fx, code, algo, G.N)
        h, p, it, v = G.decode(x, max_iter=own, algo="qmsa", post="llr", chunk=chunk, msa_precision=q, msa_step=step,
                               msa_offset=beta, tie_seed=5)
        assert np.array_equal(p, np.rint(p))
        out = (h, p.astype(np.int32), it, v)
        R.compare(out, ref, ties, (code, algo))
        R.compare_raw(fx, code, algo, out)


@pytest.mark.timeout(120)
@pytest.mark.parametrize("code", R.SMALL)
def test_integer_decoders(fx, cases, code):
    """Gallager A / B1 / B2 on the signs; quantised min-sum over q x step x
    beta, in full on the words without a tie draw."""
    G, c0 = cases(code)
    _integer_decoders(fx, G, c0, code, 64)


@pytest.mark.timeout(60)
def test_quantiser_row(fx, cases):
    """Cal_MSA_Q on inf, NaN, +-1e300, 2^30 and in-range values: the quantised
    prior is the posterior of a 0-iteration decode."""
    G, _ = cases("irr")
    llr = np.full((3, G.N), 2.0)
    llr[1, :len(R.QUANT_X)] = R.QUANT_X
    for q, step in sorted({(q, s) for q, s, _ in R.QMSA_GRID}):
        _, post, it, _ = G.decode(llr, max_iter=0, algo="qmsa", post="llr", msa_precision=q, msa_step=step)
        want = fx[f"quant/q{q}_s{int(step * 10):02d}"]
        assert (it == 0).all()
        assert np.array_equal(post[1, :len(want)].astype(np.int64), want.astype(np.int64)), (q, step)


@pytest.mark.timeout(300)
def test_dna_code_once(gpu, fx, cases):
    """The DNA code, 8 words per algorithm, through its default pool."""
    G, c0 = cases("dna")
    x, own = R.recorded_input(fx, "dna", "bp", G.N, c0)
    R.compare(_engine_bp(gpu, G, x, own, expect={"resident": True, "fused_row_block": True}),
             R.recorded(fx, "dna", "bp", G.N)[0], None, "dna bp")
    x, own = R.recorded_input(fx, "dna", "bpc", G.N, c0)
    codes = np.ascontiguousarray(R.make_codes("dna", G.N, c0, R.SEED, R.NOISE)[fx["dna/bpc/words"]])
    out = G.decode_codes(codes, R.lr_table(), gpu.IN_LR, max_iter=own, algo="bp", post="ratio")
    R.compare(out, R.recorded(fx, "dna", "bpc", G.N)[0], None, "dna bp codes")
    x, own = R.recorded_input(fx, "dna", "msa", G.N, c0)
    R.compare(G.decode(x, max_iter=own, algo="msa", post="llr"), R.recorded(fx, "dna", "msa", G.N)[0], None, "dna msa")
    _integer_decoders(fx, G, c0, "dna", 0)
