"""The oracle against an independent reference (tests/decoder_ref.py).

GPU == oracle (tests/test_gpu_parity.py and friends) proves sameness, not
correctness: the oracle is this project's own restatement of dec.cpp.  Here
its arithmetic is compared, on trajectories that do not converge as well,
with a reference written from the definition of the algorithms (longdouble
tanh-rule sum-product, min-sum, explicit loops over the other edges): three
small codes, all-zero codeword over a BI-AWGN channel (LLR = 2y / sigma^2),
iteration counts from 0 to max_iter and more than a quarter of the codewords
failing.  What this pins is oracle == definition within FLOAT_TOL, not
oracle == the reference program's binary.

The integer decoders (quantised min-sum, Gallager A / B1 / B2) get a second
plain reference in Python ints; there everything is equal.
"""
import numpy as np
import pytest

import decoder_ref as R
from test_gpu_parity import _write_pchk
from test_random_graphs_gpu import _regular_graph

# ---------------------------------------------------------------------------
# Tolerance.  d = the largest difference, relative to max(1, |L|), between
# decoder_ref run in float64 and in longdouble on exactly the inputs below:
# what an honest fp64 evaluation of the same function on the same inputs can
# be off by.  test_reference_float64_against_longdouble prints it per case and
# asserts it stays below REF_F64_D.  Measured on x86-64 (80-bit longdouble,
# glibc): reg 1.5e-14 / 3.8e-14, rs 2.6e-14 / 6.3e-15, irr 6.93e-11 / 2.2e-15
# (sum-product / min-sum); the irregular code's low-degree rows pass messages
# near 28 through atanh(tanh(.)), which costs the tanh rule digits in fp64.
# REF_F64_D is that maximum rounded up.  The oracle works in the
# likelihood-ratio domain, where 1 - 2 / (1 + pr) cancels for small messages,
# so it is allowed MARGIN times d; one order of magnitude keeps FLOAT_TOL below
# the 1e-9 at which a wrong extrinsic rule (own edge included, an edge
# dropped, a sign: posteriors move by the size of a message, > 1e-3 here)
# could begin to hide.  The negative control shows the comparison failing for
# such a rule.  (The oracle's own distance, printed by
# test_oracle_equals_reference, was at most 4.2e-14 when this was written.)
# ---------------------------------------------------------------------------
REF_F64_D = 7.0e-11
MARGIN = 10.0
FLOAT_TOL = REF_F64_D * MARGIN
MAX_MESSAGE = 30.0  # below it the LR domain neither saturates nor reaches the NaN guards

# (max_iter, sigma range of the pool, pool seed, codewords taken from the pool).
# The pool is 120 all-zero codewords, codeword b at sigma = linspace(lo, hi, 120)[b];
# the indices were chosen on the CPU by decoder_ref alone so that iteration
# counts span 0 .. max_iter, at least a quarter fail, every |message| < 30 and
# every |posterior| >= 1e-3, for sum-product and min-sum alike.
POOL = 120
CASES = {
    "reg": (4, 0.34, 0.60, 11, [1, 8, 28, 39, 37, 30, 78, 52, 67, 38, 44, 45, 47, 49]),
    "rs": (5, 0.34, 0.70, 12, [4, 58, 68, 80, 83, 69, 74, 92, 72, 75, 79, 82, 85, 87]),
    "irr": (5, 0.34, 0.85, 13, [2, 83, 39, 78, 50, 57, 74, 68, 65, 104, 84, 85, 73, 63, 72, 82]),
}
ALGOS = ("bp", "msa")


def _irregular_edges():
    """The recipe of test_irregular_graph_generic_kernels (1 to 4 random
    rows per column, one duplicate entry) with row M-2 of degree 1, row M-1
    empty and column N-1 empty."""
    rng = np.random.default_rng(3)
    M, N = 41, 120
    rows, cols = [], []
    for j in range(N - 1):
        for i in rng.choice(M - 2, size=int(rng.integers(1, 5)), replace=False):
            rows.append(int(i)); cols.append(j)
    rows.append(5); cols.append(7)
    rows.append(M - 2); cols.append(11)
    return M, N, rows, cols


def write_codes(L, tmp):
    """name -> (path of the .pchk, dense H)."""
    out = {}
    M, N, rows, cols = _regular_graph(np.random.default_rng(2), 2)
    _write_pchk(tmp / "reg.pchk", M, N, rows, cols)
    out["reg"] = (str(tmp / "reg.pchk"), R.dense_h(M, N, rows, cols))
    g = L.Graph.rs_ldpc(5, 16, 4)
    g.save_pchk(str(tmp / "rs.pchk"))
    rp, ci, _, _ = g.edges()
    out["rs"] = (str(tmp / "rs.pchk"), R.dense_h(g.M, g.N, np.repeat(np.arange(g.M), np.diff(rp)), ci))
    M, N, rows, cols = _irregular_edges()
    _write_pchk(tmp / "irr.pchk", M, N, rows, cols)
    out["irr"] = (str(tmp / "irr.pchk"), R.dense_h(M, N, rows, cols))
    return out


def awgn_llrs(name, N):
    max_iter, lo, hi, seed, idx = CASES[name]
    sigma = np.linspace(lo, hi, POOL)[:, None]
    y = 1.0 + sigma * np.random.default_rng(seed).normal(size=(POOL, N))
    return np.ascontiguousarray((2.0 * y / sigma ** 2)[idx])


@pytest.fixture(scope="module")
def codes(L, oracle_mod, tmp_path_factory):
    """name -> dict(H, og, llr, max_iter); the oracle's graph must be the H
    the reference decodes on."""
    out = {}
    for name, (path, H) in write_codes(L, tmp_path_factory.mktemp("decoder_ref")).items():
        og = oracle_mod.OracleGraph(path)
        assert (og.M, og.N, og.E) == (H.shape[0], H.shape[1], int(H.sum()))
        Ho = R.dense_h(og.M, og.N, np.repeat(np.arange(og.M), np.diff(og.row_ptr)), og.col_idx)
        assert np.array_equal(Ho, H)
        out[name] = dict(H=H, og=og, llr=awgn_llrs(name, H.shape[1]), max_iter=CASES[name][0])
    H = out["irr"]["H"]
    assert (H.sum(1) == 1).any() and not H[-1].any() and not H[:, -1].any()
    return out


_DECODE = {"bp": R.sum_product, "msa": R.min_sum}


@pytest.fixture(scope="module")
def ref(codes):
    """(code, algo) -> the longdouble reference's Result, computed once."""
    return {(n, a): _DECODE[a](c["H"], c["llr"], c["max_iter"]) for n, c in codes.items() for a in ALGOS}


def _rel(a, b):
    """Largest |a - b| / max(1, |b|); an infinity of b (the column of a
    degree-1 check, see decoder_ref.sum_product) must be met exactly."""
    a = np.asarray(a, np.longdouble)
    b = np.asarray(b, np.longdouble)
    inf = np.isinf(b)
    assert np.array_equal(a[inf], b[inf])
    return float(np.max(np.abs(a[~inf] - b[~inf]) / np.maximum(1, np.abs(b[~inf]))))


def _preconditions(r, max_iter, tol, H, algo):
    """Asserted on the reference alone, before the oracle is looked at."""
    B = len(r.iters)
    assert 12 <= B <= 16
    assert (r.iters == 0).any() and (r.iters == max_iter).any() and ((r.iters > 0) & (r.iters < max_iter)).any()
    assert 4 * int((~r.valid).sum()) >= B
    assert r.max_msg < MAX_MESSAGE, r.max_msg
    assert r.min_post >= 1e6 * tol, r.min_post  # no decision within reach of the tolerance
    # the only infinite posteriors: sum-product's +inf on the bit of a degree-1 check, once an iteration has run
    forced = H[H.sum(1) == 1].any(0) & (algo == "bp")
    assert np.array_equal(np.isposinf(r.post), (r.iters > 0)[:, None] & forced[None, :])
    assert not np.isnan(r.post).any() and not np.isneginf(r.post).any()


def _compare(og, oracle_mod, llr, max_iter, algo, r, tol):
    """The oracle's outputs against a reference Result; raises AssertionError."""
    a = oracle_mod.ALGO_BP if algo == "bp" else oracle_mod.ALGO_MSA
    h, p, it, v = og.decode_batch(llr, max_iter, algo=a, post_mode=oracle_mod.POST_LLR)
    assert np.array_equal(it, r.iters), (it, r.iters)
    assert np.array_equal(v.astype(bool), r.valid)
    assert np.array_equal(h, r.hard)
    err = _rel(p, r.post)
    assert err <= tol, err
    if algo == "bp":
        h2, ratio, it2, v2 = og.decode_batch(llr, max_iter, algo=a, post_mode=oracle_mod.POST_RATIO)
        assert np.array_equal(h2, h) and np.array_equal(it2, it) and np.array_equal(v2, v)
        want = np.exp(r.post)  # longdouble
        bound = tol * np.maximum(1, np.abs(r.post)) * want  # d(exp L) = exp(L) dL
        inf = np.isinf(want)
        assert np.array_equal(ratio[inf], np.asarray(want[inf], np.float64))
        assert (np.abs(np.asarray(ratio, np.longdouble)[~inf] - want[~inf]) <= bound[~inf]).all()
    return err


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("name", list(CASES))
def test_reference_float64_against_longdouble(codes, ref, name, algo):
    """The reference against itself: float64 and longdouble give the same
    decisions, and their posteriors differ by at most REF_F64_D -- the
    figure FLOAT_TOL is derived from."""
    c = codes[name]
    r = ref[name, algo]
    _preconditions(r, c["max_iter"], FLOAT_TOL, c["H"], algo)
    r64 = _DECODE[algo](c["H"], c["llr"], c["max_iter"], dtype=np.float64)
    assert np.array_equal(r64.iters, r.iters) and np.array_equal(r64.hard, r.hard)
    d = _rel(r64.post, r.post)
    print(f"{name} {algo}: float64 vs longdouble reference d = {d:.3e}")
    assert d <= REF_F64_D
    assert FLOAT_TOL < 1e-9


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("name", list(CASES))
def test_oracle_equals_reference(codes, ref, oracle_mod, name, algo):
    """decode_batch (BP with post_mode 0 and 1, min-sum) == the definition:
    hard bits, iteration counts and valid flags equal, posterior LLR within
    FLOAT_TOL relative to max(1, |L|), BP ratio == exp(L) within the same."""
    c = codes[name]
    r = ref[name, algo]
    _preconditions(r, c["max_iter"], FLOAT_TOL, c["H"], algo)
    err = _compare(c["og"], oracle_mod, c["llr"], c["max_iter"], algo, r, FLOAT_TOL)
    print(f"{name} {algo}: oracle vs longdouble reference {err:.3e} (tolerance {FLOAT_TOL:.1e})")


@pytest.mark.parametrize("algo", ALGOS)
def test_negative_control_own_edge_included(codes, ref, oracle_mod, algo):
    """A copy of the reference whose extrinsic loops include the own edge
    must fail the very comparison the oracle passes."""
    c = codes["reg"]
    wrong = _DECODE[algo](c["H"], c["llr"], c["max_iter"], own_edge=True)
    with pytest.raises(AssertionError):
        _compare(c["og"], oracle_mod, c["llr"], c["max_iter"], algo, wrong, FLOAT_TOL)
    # and in the posterior alone, where both ran the same number of iterations
    same = wrong.iters == ref["reg", algo].iters
    same &= ref["reg", algo].iters > 0
    assert same.any()
    assert _rel(wrong.post[same], ref["reg", algo].post[same]) > 1e-3


# ---------------------------------------------------------------------------
# integer decoders
# ---------------------------------------------------------------------------
INT_GRID = [(q, beta, step) for q in (2, 6, 16) for beta in (0, 1) for step in (0.25, 2.0)]
INT_SEED = 20240607
INT_NAMES = {2: "qmsa", 3: "gallager_a", 4: "gallager_b1", 5: "gallager_b2"}


def int_llrs(name, N, B):
    """Noisy BI-AWGN LLRs with erasures: exact zeros quantise to 0 and a
    posterior sum can cancel to 0, which forces the tie bit at Init_MSA and at
    the decisions."""
    rng = np.random.default_rng({"reg": 31, "rs": 32, "irr": 33}[name])
    sigma = np.linspace(0.45, 0.9, B)[:, None]
    x = 2.0 * (1.0 + sigma * rng.normal(size=(B, N))) / sigma ** 2
    x[rng.random((B, N)) < 0.08] = 0.0
    x[rng.random((B, N)) < 0.02] = -0.0
    x[0, : N // 2] = 0.0
    return np.ascontiguousarray(x)


def _int_equal(got, want, what):
    for g, w, part in zip(got, want, ("hard", "post", "iters", "valid")):
        assert np.array_equal(np.asarray(g).astype(np.float64), np.asarray(w).astype(np.float64)), (what, part)


@pytest.mark.parametrize("q,beta,step", INT_GRID)
def test_oracle_quantised_min_sum_equals_reference(codes, q, beta, step):
    """decode_int_batch == the literal Python-int restatement of
    dec.cpp:1174-1764 at q = 2, 6, 16: integers, no tolerance."""
    ties = 0
    for name, c in codes.items():
        llr = int_llrs(name, c["H"].shape[1], 4)
        want = R.int_decode(c["H"], llr, 3, R.QMSA, precision=q, step=step, beta=beta, seed=INT_SEED)
        got = c["og"].decode_int_batch(llr, 3, R.QMSA, precision=q, step=step, beta=beta, seed=INT_SEED)
        _int_equal(got, want, name)
        ties += int((want[1] == 0).sum())
        assert want[2].max() == 3
    assert ties > 0  # posteriors (or quantised priors) of exactly 0: the tie bit decided


@pytest.mark.parametrize("algo", [R.GALLAGER_A, R.GALLAGER_B1, R.GALLAGER_B2])
def test_oracle_gallager_equals_reference(codes, algo):
    for name, c in codes.items():
        llr = int_llrs(name, c["H"].shape[1], 4)
        want = R.int_decode(c["H"], llr, 3, algo)
        got = c["og"].decode_int_batch(llr, 3, algo)
        _int_equal(got, want, name)


def test_tie_bit_and_quantiser_known_values():
    """The reference's own pieces on values worked out by hand: round half
    up, clip to +-(2^(q-1) - 1), sign restored, -0.0 -> 0 (dec.cpp:1708-1743)."""
    x = [0.0, -0.0, 0.49, 0.5, -0.5, 1.49, -2.5, 6.6, 7.5, 100.0, -100.0]
    assert [R.cal_msa_q(v, 1.0, 7, -7) for v in x] == [0, 0, 0, 1, -1, 1, -3, 7, 7, 7, -7]
    assert [R.cal_msa_q(v, 2.0, 1, -1) for v in (0.99, 1.0, -1.0, 50.0)] == [0, 1, -1, 1]
    bits = [R.tie_bit(7, b, s, j) for b in range(4) for s in range(4) for j in range(64)]
    assert 0.35 < np.mean(bits) < 0.65


@pytest.mark.gpu
@pytest.mark.parametrize("q,beta,step", INT_GRID)
def test_gpu_quantised_min_sum_grid(gpu, oracle_mod, tmp_path, q, beta, step):
    """The same q / beta / step grid, GPU == oracle, on the (8, 72)-regular
    code with Q = 2 (the specialised degrees) and the irregular one, B = 70
    (a full tile and a ragged one)."""
    paths = write_codes(gpu, tmp_path)
    for name in ("reg", "irr"):
        path, H = paths[name]
        og = oracle_mod.OracleGraph(path)
        G = gpu.Graph(path)
        llr = int_llrs(name, G.N, 70)
        want = og.decode_int_batch(llr, 12, R.QMSA, precision=q, step=step, beta=beta, seed=INT_SEED, threads=8)
        got = G.decode(llr, max_iter=12, algo="qmsa", post="llr", msa_precision=q, msa_step=step, msa_offset=beta,
                       tie_seed=INT_SEED)
        _int_equal(got, want, name)
        assert (want[1] == 0).any()


# ---------------------------------------------------------------------------
# the host libm on the inputs of the device exp / log checks (test_real_llr_gpu.py)
# ---------------------------------------------------------------------------
def test_host_libm_exp_log_ulps(oracle_mod, tmp_path):
    """For scale: the oracle's exp (zero-iteration posterior ratio) and log
    (posterior LLR of the reg2 BP batch) against longdouble, on the very
    inputs the device's exp and log are measured on.  glibc documents both
    within 1 ulp; observed when this was written: exp 1 ulp, log 1 ulp."""
    import real_llr_cases as C
    M, N, rows, cols = C.regular_rows_permuted(2, 102)
    _write_pchk(tmp_path / "reg2.pchk", M, N, rows, cols)
    og = oracle_mod.OracleGraph(str(tmp_path / "reg2.pchk"))
    x = C.exp_inputs(N, 64)
    _, host, _, _ = og.decode_batch(x, 0, algo=oracle_mod.ALGO_BP, post_mode=oracle_mod.POST_RATIO)
    with np.errstate(over="ignore", under="ignore"):
        want = np.exp(x.astype(np.longdouble)).astype(np.float64)
    nan = np.isnan(x)
    assert (host[nan] == 1.0).all()  # the NaN -> 1 guard (dec.cpp:676-677)
    exp_ulps = C.ulp_distance(host[~nan], want[~nan])
    order = np.argsort(x[~nan], kind="stable")
    sorted_out = host[~nan][order]
    assert (sorted_out[1:] >= sorted_out[:-1]).all()
    sigma, max_iter = C.SIGMA["reg2", "bp"]
    llr = C.gaussian_llrs(N, C.B, sigma, 1)
    C.plant_directed(llr, og.col_idx[og.row_ptr[0]:og.row_ptr[1]])
    _, ratio, _, _ = og.decode_batch(llr, max_iter, algo=oracle_mod.ALGO_BP, post_mode=oracle_mod.POST_RATIO)
    _, post, _, _ = og.decode_batch(llr, max_iter, algo=oracle_mod.ALGO_BP, post_mode=oracle_mod.POST_LLR)
    with np.errstate(divide="ignore"):
        want = np.log(ratio.astype(np.longdouble)).astype(np.float64)
    inf = np.isinf(want)
    assert np.array_equal(post[inf], want[inf])
    log_ulps = C.ulp_distance(post[~inf], want[~inf])
    print(f"host libm: exp max {exp_ulps.max()} ulp, log max {log_ulps.max()} ulp")
    assert exp_ulps.max() <= 1 and log_ulps.max() <= 1
