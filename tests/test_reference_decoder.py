"""The oracle against the REFERENCE's own decoders: dec.cpp compiled
unmodified into oracle/_ref/librefdec.so (oracle/ref_dec_harness.cpp), and its
outputs recorded in tests/golden/refdec_goldens.npz by
tests/golden/make_refdec_fixtures.py.

The recorded comparison never skips: for every code, algorithm and word the
oracle gives the reference's hard bits, iteration count, valid flag and
posterior bytes (BP's ratio, the min-sum's L, the quantised min-sum's L_Q; a
NaN matches a NaN).  Quantised min-sum is compared in full on the words where
the reference drew no tie bit (the bits are MKL's); on the others, where the
oracle's hashed bits led to the same iteration count, on L_Q and on the hard
bits off the zero posteriors.  Where librefdec.so is built, the oracle is also
compared with it live on a second, differently seeded batch, at max_iter 0, 1
and the case's own, and the fixture file is made again and compared.

Shown by hand (none of them committed): each of these changes to
oracle/ldpc_oracle.c fails test_oracle_equals_reference_fixture on reg4, rs5
and irr -- the backward pass run forward; `p <= 1` as `p < 1`; the NaN guard
after the decision; Gallager's b off by one (A's b_var, B2's b_dec);
1 - 2/(1+pr) as the single division (pr - 1)/(pr + 1).  Taking 1 - 2/(1+pr)
once, stored in the forward pass and reused in the backward one, is the same
expression on the same operand and gives the same bits: it passes, as it
must."""
import hashlib
import importlib.util
import os

import numpy as np
import pytest

import refdec_cases as R
from conftest import GOLDEN


def _load_maker():
    spec = importlib.util.spec_from_file_location("make_refdec_fixtures",
                                                  os.path.join(GOLDEN, "make_refdec_fixtures.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def maker(oracle_mod):
    return _load_maker()


@pytest.fixture(scope="module")
def fx():
    z = np.load(R.FIXTURE)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def code_files(fx, oracle_mod, tmp_path_factory):
    """name -> (path, row 0's columns, OracleGraph); the generated codes are
    written from the fixture's edge lists and must hash as recorded."""
    tmp = tmp_path_factory.mktemp("refdec")
    made = {}

    def get(name):
        if name not in made:
            if name == "dna":
                path = R.DNA_PCHK
                c0 = R.pchk_row0(path)
            else:
                path = str(tmp / f"{name}.pchk")
                rows, cols = fx[f"{name}/edges"].astype(np.int64)
                M, N = fx[f"{name}/shape"]
                R.write_pchk(path, int(M), int(N), rows, cols)
                c0 = R.row0_cols(rows, cols)
            assert R.file_sha(path) == str(fx[f"{name}/pchk_sha256"])
            made[name] = (path, c0, oracle_mod.OracleGraph(path))
        return made[name]
    return get


@pytest.mark.parametrize("algo", R.ALGOS)
@pytest.mark.parametrize("code", R.CODES)
def test_oracle_equals_reference_fixture(fx, code_files, maker, code, algo):
    path, c0, og = code_files(code)
    x, max_iter = R.recorded_input(fx, code, algo, og.N, c0)
    ref, ties = R.recorded(fx, code, algo, og.N)
    out = maker.oracle_decode(og, algo, x, max_iter)
    R.compare(out, ref, ties, (code, algo))
    R.compare_raw(fx, code, algo, out)
    if ties is not None:
        assert (ties == 0).sum() >= (4 if code == "dna" else 32)
    for m in R.SHORT.get(algo, ()) if code != "dna" else ():
        R.compare(maker.oracle_decode(og, algo, x, m), R.recorded(fx, code, algo, og.N, m)[0], None, (code, algo, m))


def test_oracle_quantiser_equals_reference_fixture(fx, code_files, oracle_mod):
    """Cal_MSA_Q on values outside the int range (tests/test_int_decoders.py)
    and inside it: the oracle's quantised prior, read from a 0-iteration decode."""
    _, _, og = code_files("irr")
    llr = np.full((1, og.N), 2.0)
    llr[0, :len(R.QUANT_X)] = R.QUANT_X
    for q, step in sorted({(q, s) for q, s, _ in R.QMSA_GRID}):
        _, post, _, _ = og.decode_int_batch(llr, 0, oracle_mod.ALGO_QMSA, precision=q, step=step)
        want = fx[f"quant/q{q}_s{int(step * 10):02d}"]
        assert np.array_equal(post[0, :len(want)].astype(np.int64), want.astype(np.int64)), (q, step)
    assert (fx["quant/q6_s05"][:6] == -2 ** 31).all()  # inf, -inf, NaN, +-1e300, 2^30 / step: INT_MIN, as documented


# ---------------------------------------------------------------------------
# live: only where oracle/_ref/librefdec.so is built (the reference sources exist)
# ---------------------------------------------------------------------------
def _need_live(oracle_mod):
    if not oracle_mod.refdec_available():
        pytest.skip("oracle/_ref/librefdec.so not built (reference sources not present)")


@pytest.mark.parametrize("code", R.SMALL)
def test_oracle_equals_reference_live(fx, code_files, maker, oracle_mod, code):
    """A second batch (another seed), at max_iter 0, 1 and the case's own."""
    _need_live(oracle_mod)
    path, c0, og = code_files(code)
    rd = oracle_mod.RefDecoder(path)
    assert (rd.M, rd.N) == (og.M, og.N) and rd.dv == og.regular()[0]
    for algo in R.ALGOS:
        x, own = R.make_input(code, algo, og.N, c0, R.SEED_LIVE, R.NOISE)
        for max_iter in (0, 1, own):
            h, p, it, v, ties = maker.reference_decode(rd, algo, x, max_iter)
            ref = (h, None if p is None else R.digests(p), it, v)
            R.compare(maker.oracle_decode(og, algo, x, max_iter), ref, ties, (code, algo, max_iter))


def test_quantiser_equals_reference_live(code_files, oracle_mod):
    _need_live(oracle_mod)
    path, _, og = code_files("irr")
    rd = oracle_mod.RefDecoder(path)
    llr = np.full((1, og.N), 2.0)
    llr[0, :len(R.QUANT_X)] = R.QUANT_X
    for q, step in [(6, 0.5), (3, 2.0), (4, 1.0), (8, 0.25)]:
        _, post, _, _ = og.decode_int_batch(llr, 0, oracle_mod.ALGO_QMSA, precision=q, step=step)
        assert np.array_equal(post[0].astype(np.int64), rd.quantise(llr[0], q, step).astype(np.int64)), (q, step)


def test_tie_queue_pins_a_tie_word(fx, code_files, maker, oracle_mod):
    """The harness serves a caller's tie bits: fed the bits the oracle's hash
    would draw in the reference's call order -- here all zeros and all ones --
    the reference's decode follows; an exhausted or unread queue is an error."""
    _need_live(oracle_mod)
    path, c0, og = code_files("irr")
    rd = oracle_mod.RefDecoder(path)
    x = np.zeros((1, og.N))  # every prior ties: N draws at the start
    h0 = rd.qmsa(x, 0, 6, 0.5, 0)
    assert h0[4][0] == og.N and not h0[0].any()
    h1 = rd.qmsa(x, 0, 6, 0.5, 0, tie_bits=[np.ones(og.N, np.uint8)])
    assert h1[0].all() and h1[4][0] == og.N
    with pytest.raises(ValueError):
        rd.qmsa(x, 0, 6, 0.5, 0, tie_bits=[np.ones(og.N - 1, np.uint8)])
    with pytest.raises(ValueError):
        rd.qmsa(x, 0, 6, 0.5, 0, tie_bits=[np.ones(og.N + 1, np.uint8)])


def test_fixture_file_is_reproducible(fx, maker, oracle_mod, tmp_path):
    """Made again, the arrays are the recorded ones: the small codes in full,
    the DNA code for three algorithms on the words the file names (its
    candidates' decodes take minutes)."""
    _need_live(oracle_mod)
    words = {k[:-len("words")]: v for k, v in fx.items() if k.endswith("/words")}
    dna = ("bp", "gb1", "q6_s05_b0")
    out = maker.build(str(tmp_path), log=lambda s: None, words=words, with_oracle=False,
                      algos=lambda code: dna if code == "dna" else R.ALGOS)
    assert len(out) > 300
    for k, v in out.items():
        if k == "stats":
            continue
        assert k in fx, k
        v = np.asarray(v)
        if v.dtype.kind == "U":
            assert str(v) == str(fx[k]), k
        else:
            R.same_bits(v, fx[k], k)
