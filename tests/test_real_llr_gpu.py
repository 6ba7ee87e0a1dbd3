"""The specialised degree-72 / degree-8 kernels on real-valued LLRs.

Every other GPU test feeds k_check_bp<72>, k_check_bp_first<72>, k_var_m<., 8>,
k_check_msa<72>, k_check_msa_c / k_var_msa_c and the hand-over arm lattice
inputs (+-ln 49, k ln 49): in a lane's first check all 72 magnitudes of a row
are then bit-identical, and the "min2 at the min1 edge, min1 elsewhere"
selection, the 7-bit min1 position of the meta word, the first-index rule and
m2 = min(m2, max(m1, a)) never see distinct operands.  Here the channel is
BI-AWGN (all-zero codeword, LLR = 2y / sigma^2), every row's minimum is
unique, and a few codewords carry directed rows (magnitudes one ulp apart,
sign-opposed ties at a row's ends, subnormals, |LLR| = 700 / 745, a NaN at a
row's first / second edge, an all-NaN codeword).  The bar is the one of
test_gpu_parity._cmp / test_random_graphs_gpu._cmp_nan: hard bits, iteration
counts, valid flags and posterior bytes equal to the oracle, a NaN matched by
a NaN -- on every schedule, and every schedule equal to every other.  The
input crosses as fp64 (off the lattice ldpc_decode cannot code it), so the
fp64 prior path of the continuous kernels runs throughout.

The second part measures the device exp and log against longdouble
references (x87 80-bit, rounded to fp64), in ulps.  Observed on one MI355X
(gfx950, the ROCm device library's exp and log), inputs seeded:
  exp  9215 arguments (exp_inputs: Gaussian, +-[1e-300, 745] log-spaced,
       neighbours of ln(DBL_MAX) / ln(DBL_MIN) / ln(denorm_min), 600 and more
       subnormal results): max 1 ulp, 204 results not correctly rounded,
       subnormal results max 1 ulp, monotone, special values exact;
  log  28 799 finite posterior ratios of the reg2 BP batch (4.9e-324 ..
       6.7e+303) and one infinite: max 1 ulp, 44 not correctly rounded.
The host libm on the same inputs is at 1 ulp for both
(tests/test_decoder_reference.py::test_host_libm_exp_log_ulps).
"""
import numpy as np
import pytest

import real_llr_cases as C
from conftest import PCHK
from test_gpu_parity import _write_pchk
from test_random_graphs_gpu import SCHEDULES

pytestmark = pytest.mark.gpu

# Largest distance from the correctly rounded longdouble result, measured on
# the MI355X with these seeded inputs (the tests print the figures before they
# assert); the tests assert observed + 1 ulp.
EXP_ULP_OBSERVED = 1
LOG_ULP_OBSERVED = 1

CODES = ("reg2", "reg16", "rs7")
ALGOS = ("bp", "msa")

# (schedule, chunk, max_iter or None for the case's own)
RUNS = [(s, 64, None) for s in SCHEDULES]
RUNS += [({}, 0, None), ({"resident": False}, 0, None)]  # one fill: the first check reads the prior
RUNS += [({"first_from_prior": False}, 64, None), ({"first_from_prior": False, "resident": False}, 0, None)]
# (fp64 min-sum messages: the compressed min-sum has no resident pool)
RUNS += [({"resident": True, "handover": h, "msa_compressed": False}, 192, mi) for h in (True, False) for mi in (1, 3)]
RUNS += [({"resident": False, "msa_compressed": False, "var_cpw": k}, 64, None) for k in (1, 2, 3, 4, 8)]
# compressed min-sum over 8 pool tiles (4 of them occupied) in groups of 1, 2, 5, 8
RUNS += [({"msa_compressed": True, "group_tiles": g, "var_cpw": k}, 512, None)
         for g, k in ((1, 4), (2, 2), (5, 1), (8, 3))]


class Case:
    """One code: its graph on both sides, one input batch per algorithm, the
    oracle's outputs (computed once per max_iter) and the first GPU result
    per (algorithm, max_iter), which every later schedule must reproduce."""

    def __init__(self, name, gpu, oracle_mod, tmp, nb=C.B, where=C.DIRECTED):
        self.name, self.oracle_mod = name, oracle_mod
        if name == "dna":
            path = PCHK
        else:
            path = str(tmp / f"{name}.pchk")
            if name == "rs7":
                gpu.Graph.rs_ldpc(7, 72, 8).save_pchk(path)  # the smallest RS-LDPC code with rho = 72
            else:
                Q = int(name[3:])
                M, N, rows, cols = C.regular_rows_permuted(Q, 100 + Q)
                _write_pchk(path, M, N, rows, cols)
        self.G = gpu.Graph(path)
        self.og = oracle_mod.OracleGraph(path)
        rp, ci, _, _ = self.G.edges()
        self.llr, self.max_iter = {}, {}
        for algo in ALGOS:
            sigma, self.max_iter[algo] = C.SIGMA[name, algo]
            x = C.gaussian_llrs(self.G.N, nb, sigma, 1)
            self.directed = C.plant_directed(x, ci[rp[0]:rp[1]], where)
            self.llr[algo] = x
        self.plain = np.setdiff1d(np.arange(nb), self.directed)
        self._oracle, self.first = {}, {}

    def oracle(self, algo, max_iter=None):
        mi = self.max_iter[algo] if max_iter is None else max_iter
        if (algo, mi) not in self._oracle:
            a = 0 if algo == "bp" else 1
            h, p, it, v = self.og.decode_batch(self.llr[algo], mi, algo=a, post_mode=1 if a == 0 else 0, threads=16)
            self._oracle[algo, mi] = (h, p, it, v.astype(bool))
        return self._oracle[algo, mi]

    def check(self, algo, got, max_iter=None):
        """got == the oracle, and == the first GPU result of this (algo, max_iter)."""
        mi = self.max_iter[algo] if max_iter is None else max_iter
        _same(got, self.oracle(algo, mi), (self.name, algo, "oracle"))
        _same(got, self.first.setdefault((algo, mi), got), (self.name, algo, "first schedule"))


def _same(got, ref, what):
    h, p, it, v = got
    rh, rp, rit, rv = ref
    assert np.array_equal(it, rit), (what, it, rit)
    assert np.array_equal(np.asarray(v, bool), np.asarray(rv, bool)), what
    assert np.array_equal(h, rh), what
    nan = np.isnan(rp)
    assert np.array_equal(np.isnan(p), nan), what
    assert np.array_equal(p[~nan].view(np.uint64), rp[~nan].view(np.uint64)), what


@pytest.fixture(scope="module")
def cases(gpu, oracle_mod, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("real_llr")
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(name, gpu, oracle_mod, tmp)
        return made[name]
    return get


def _input_properties(c, rb):
    """Everything asserted here comes from the input, the graph and the
    oracle, never from the GPU."""
    G = c.G
    assert (G.dc, G.dv, G.regular_dc, G.regular_dv) == (72, 8, True, True)
    assert C.edge_s_in_row_block_s(G) == rb  # both v2c layouts of the compressed min-sum are covered
    for algo in ALGOS:
        x = c.llr[algo]
        uniq1, uniq2 = C.first_check_positions(x, G)
        assert (uniq1 > 0).all() and (uniq2 > 0).all(), (uniq1.min(), uniq2.min())
        _, _, it, v = c.oracle(algo)
        mi = c.max_iter[algo]
        assert mi <= 25 and 1 < it.mean() < mi, it.mean()
        assert len(np.unique(it)) > 3
        assert not v[c.plain].all()  # a failure among the plain Gaussian codewords
        assert (it[c.directed[:-1]] > 0).all()  # the directed rows reach the check phase


@pytest.mark.parametrize("name,rb", [("reg2", False), ("reg16", False), ("rs7", True)])
def test_inputs_reach_every_min_position(cases, name, rb):
    """(8, 72)-regular, N = 144 (not a multiple of 64), 1152 (the fast
    paths) and 9216 (RS-LDPC, row-block-major v2c); in the first check every
    position 0..71 of a row is the strictly unique min1 and the strictly
    unique min2 somewhere in the batch; the oracle's iteration counts spread
    (1 < mean < max_iter, more than three values, a failure)."""
    _input_properties(cases(name), rb)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("run", range(len(RUNS)))
@pytest.mark.parametrize("name", CODES)
def test_real_llrs_every_schedule_bitexact(cases, name, run):
    """B = 200 through a 64-lane pool (three refills, a ragged last tile), a
    192-lane resident pool with and without the hand-over at max_iter 1 and
    3, one fill, 8-tile groups: equal to the oracle and to every other
    schedule of the same code and algorithm."""
    c = cases(name)
    schedule, chunk, mi = RUNS[run]
    for algo in ALGOS:
        got = c.G.decode(c.llr[algo], max_iter=c.max_iter[algo] if mi is None else mi, algo=algo,
                         post="ratio" if algo == "bp" else "llr", chunk=chunk, schedule=schedule)
        c.check(algo, got, mi)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("name", CODES)
def test_real_llrs_device_resident_engine(gpu, cases, name):
    """The same fp64 batch uploaded to the device: IN_LLR for min-sum, IN_LR
    (the host's exp, as the oracle computes it) for BP; one fill (B <= pool)
    and several."""
    L = gpu
    c = cases(name)
    G = c.G
    nb, N = c.llr["bp"].shape
    # LR = the host libm's exp(LLR): the oracle's 0-iteration posterior ratio, NaN put back (its guard turns NaN to 1)
    _, lr, _, _ = c.og.decode_batch(c.llr["bp"], 0, algo=0, post_mode=1, threads=16)
    lr[np.isnan(c.llr["bp"])] = np.nan
    d_in = L.DeviceBuffer(0, nb * N * 8)
    d_h, d_p, d_i, d_v = L.DeviceBuffer(0, nb * N), L.DeviceBuffer(0, nb * N * 8), L.DeviceBuffer(0, nb * 4), \
        L.DeviceBuffer(0, nb)
    for algo, kind, x, post in (("bp", L.IN_LR, lr, L.POST_RATIO), ("msa", L.IN_LLR, c.llr["msa"], L.POST_LLR)):
        d_in.upload(np.ascontiguousarray(x))
        for chunk in (256, 64):
            eng = L.Engine(G, 0, algo, chunk=chunk)
            assert (eng.cap >= nb) == (chunk == 256)
            eng.decode(d_in.at(0), kind, nb, c.max_iter[algo], d_h.at(0), d_p.at(0), post, d_i.at(0), d_v.at(0))
            eng.sync()
            got = (d_h.download(np.empty((nb, N), np.uint8)), d_p.download(np.empty((nb, N), np.float64)),
                   d_i.download(np.empty(nb, np.int32)), d_v.download(np.empty(nb, np.uint8)).astype(bool))
            c.check(algo, got)
            eng.close()


@pytest.mark.timeout(300)
def test_dna_code_real_llrs(gpu, oracle_mod, tmp_path):
    """The DNA code itself, one case: B = 70, 15 iterations, BP and min-sum."""
    where = {k: 3 + 7 * i for i, k in enumerate(C.DIRECTED)}
    where["all_nan"] = 69
    c = Case("dna", gpu, oracle_mod, tmp_path, nb=70, where=where)
    _input_properties(c, True)
    for algo in ALGOS:
        assert c.max_iter[algo] == 15
        got = c.G.decode(c.llr[algo], max_iter=15, algo=algo, post="ratio" if algo == "bp" else "llr")
        c.check(algo, got)


# ---------------------------------------------------------------------------
# device exp and log, in ulps of the correctly rounded longdouble result
# ---------------------------------------------------------------------------
def test_device_exp_ulps(cases):
    """max_iter = 0, post='ratio', exp_on_host=False returns the device's
    exp(x) (the oracle returns exp(LLR) at zero iterations, its NaN guard
    included).  Specials exact (0, inf, 1.0 at +-0, the guard's 1.0 for NaN),
    monotone over the sorted arguments, elsewhere within EXP_ULP_OBSERVED + 1
    ulp of longdouble exp rounded to fp64."""
    c = cases("reg2")
    x = C.exp_inputs(c.G.N, 64)
    _, got, it, _ = c.G.decode(x, max_iter=0, post="ratio", exp_on_host=False)
    assert (it == 0).all()
    _, host, _, _ = c.og.decode_batch(x, 0, algo=0, post_mode=1)
    with np.errstate(over="ignore", under="ignore"):
        want = np.exp(x.astype(np.longdouble)).astype(np.float64)
    nan = np.isnan(x)
    assert nan.any() and np.array_equal(got[nan], host[nan]) and (got[nan] == 1.0).all()
    assert (got[x == 0] == 1.0).all() and np.signbit(x[x == 0]).any()
    assert (got[np.isposinf(x)] == np.inf).all() and (got[np.isneginf(x)] == 0.0).all()
    assert (want[~nan] == 0).any() and np.isinf(want[~nan & np.isfinite(x)]).any()
    sub = ~nan & (want > 0) & (want < 2.2250738585072014e-308)
    assert sub.sum() > 100
    fin = ~nan  # 0 and inf lie on the ordered line next to denorm_min and DBL_MAX
    ulps = C.ulp_distance(got[fin], want[fin])
    order = np.argsort(x[fin], kind="stable")
    sorted_out = got[fin][order]
    falls = int((sorted_out[1:] < sorted_out[:-1]).sum())
    print(f"device exp: max {ulps.max()} ulp over {fin.sum()} values ({(ulps > 0).sum()} not correctly rounded), "
          f"subnormal results max {C.ulp_distance(got[sub], want[sub]).max()} ulp; "
          f"host libm max {C.ulp_distance(host[fin], want[fin]).max()} ulp; "
          f"decreasing steps {falls}")
    assert falls == 0
    assert ulps.max() <= EXP_ULP_OBSERVED + 1


def test_device_log_ulps(cases):
    """The posterior LLR is the device's log of the posterior ratio: the
    ratio is bit-exact to the oracle, the LLR within LOG_ULP_OBSERVED + 1 ulp
    of longdouble log of that ratio; log(0) = -inf and log(inf) = +inf
    exactly.  (POST_TOL of test_gpu_parity stays: this bound is the tight one.)"""
    c = cases("reg2")
    x, mi = c.llr["bp"], c.max_iter["bp"]
    _, ratio, _, _ = c.G.decode(x, max_iter=mi, post="ratio", chunk=64)
    h, llr, it, v = c.G.decode(x, max_iter=mi, post="llr", chunk=64)
    c.check("bp", (h, ratio, it, v))
    _, host, _, _ = c.og.decode_batch(x, mi, algo=0, post_mode=0, threads=16)
    assert not np.isnan(ratio).any() and (ratio >= 0).all()
    with np.errstate(divide="ignore"):
        want = np.log(ratio.astype(np.longdouble)).astype(np.float64)
    inf = np.isinf(want)
    assert np.array_equal(llr[inf], want[inf])
    ulps = C.ulp_distance(llr[~inf], want[~inf])
    print(f"device log: max {ulps.max()} ulp over {(~inf).sum()} values ({(ulps > 0).sum()} not correctly rounded), "
          f"{inf.sum()} infinite; host libm max {C.ulp_distance(host[~inf], want[~inf]).max()} ulp; "
          f"ratio range {ratio[ratio > 0].min():.3e} .. {ratio[np.isfinite(ratio)].max():.3e}")
    assert not np.isnan(llr).any()
    assert ulps.max() <= LOG_ULP_OBSERVED + 1
