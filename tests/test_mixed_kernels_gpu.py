"""GPU parity where one side of the graph is specialised and the other is not.

The engine picks its check kernel by the rows alone (all of degree 72:
k_check_bp / k_check_msa<72>, k_syndrome_split<72>, k_syndrome<72>) and its
variable kernel by the columns alone (all of degree 8: k_var_m<., 8, ...>), so
a code that is regular on one side only runs a specialised kernel next to a
generic one (k_var_gr_cont / k_var_gr / k_var_*_gen, k_check_gr /
k_check_gr_res / k_check_*_gen).  Each code below is the smallest that reaches
its pairing (CODES: what it reaches); every graph is written as a .pchk and
loaded on both sides, and BP and min-sum decodes must equal the CPU oracle bit
for bit -- hard decisions, iteration counts, valid flags and the posterior (BP
ratio, min-sum L) -- over every schedule family, for fp64 and int8-coded
input.  The channel is +-ln 49 through a BSC plus 1 % erasures at a flip
probability where the exits spread (asserted on the oracle's output), so lanes
finish at different steps and the pools refill.

Pool sizes.  Graph.decode gives a batch of up to 1024 codewords a lane pool
that holds all of them unless the caller names a chunk, so at B = 200 the
`_chunk` 0 and 256 entries decode in a single fill.  The entries with `_chunk`
128 (REFILL_SCHEDULES) are the two-tile pools -- resident and grouped -- whose
lanes are refilled as codewords finish.
"""
import numpy as np
import pytest

from test_gpu_parity import _write_pchk
from test_random_graphs_gpu import GEN_SCHEDULES, SCHEDULES, _cmp_nan, _llr, _regular_graph

pytestmark = pytest.mark.gpu

UNIT = 3.8918202981106265  # ln 49
TABLE = np.arange(-128, 128, dtype=np.float64) * UNIT
B = 200        # three tiles plus 8 lanes
MAX_ITER = 20


def _rows72_graph(rng, M, N):
    """Every row draws 72 distinct columns: regular rows, irregular columns."""
    rows, cols = [], []
    for i in range(M):
        for j in rng.choice(N, size=72, replace=False):
            rows.append(i)
            cols.append(int(j))
    return M, N, rows, cols


def _cols8_graph(rng, M, N):
    """Every column draws 8 distinct rows: regular columns, irregular rows."""
    rows, cols = [], []
    for j in range(N):
        for i in rng.choice(M, size=8, replace=False):
            rows.append(int(i))
            cols.append(j)
    return M, N, rows, cols


# name: (construction, graph seed, (M, N), (dc, regular_dc, dv, regular_dv), p for BP, p for min-sum)
CODES = {
    # rows of degree 72: check<72> kernels next to the generic variable kernels
    "r4x72": (("reg", 4, 4, 72), 1, (16, 288), (72, True, 4, True), 0.003, 0.003),    # var bucket 4; N % 32 == 0
    "r6x72": (("reg", 5, 6, 72), 2, (30, 360), (72, True, 6, True), 0.003, 0.003),    # bucket 8; N % 16 != 0
    "r3x72": (("reg", 8, 3, 72), 3, (24, 576), (72, True, 3, True), 0.003, 0.003),    # N % 64 == 0; below bucket 4
    "r16x72": (("reg", 3, 16, 72), 4, (48, 216), (72, True, 16, True), 0.01, 0.003),  # bucket 16, on its edge
    "r17x72": (("reg", 3, 17, 72), 5, (51, 216), (72, True, 17, True), 0.01, 0.003),  # one past: bucket 24
    "r33x72": (("reg", 2, 33, 72), 6, (66, 144), (72, True, 33, True), 0.01, 0.01),   # no var bucket: fixed passes
    "i72": (("rows72", 24, 300), 1, (24, 300), (72, True, 12, False), 0.003, 0.003),  # irregular columns
    # columns of degree 8: k_var_m<8> next to the generic check kernels
    "r8x16": (("reg", 10, 8, 16), 7, (80, 160), (16, True, 8, True), 0.03, 0.01),     # check bucket 16; 32 | N
    "r8x48": (("reg", 5, 8, 48), 8, (40, 240), (48, True, 8, True), 0.01, 0.003),     # bucket 48; 16 | N, 32 does not
    "r8x96": (("reg", 3, 8, 96), 9, (24, 288), (96, True, 8, True), 0.003, 0.003),    # the last check bucket
    "r8x100": (("reg", 3, 8, 100), 10, (24, 300), (100, True, 8, True), 0.003, 0.003),  # past it: memory-staged check
    "i8": (("cols8", 30, 63), 4, (30, 63), (24, False, 8, True), 0.03, 0.03),         # irregular rows; N % 4 != 0
}
ROWS72 = ["r4x72", "r6x72", "r3x72", "r16x72", "r17x72", "i72"]
COLS8 = ["r8x16", "r8x48", "r8x96", "r8x100", "i8"]
NOT_CONTINUOUS = {"r33x72"}            # no register bucket for its columns
NOT_RESIDENT = {"r33x72", "r8x100"}    # r8x100: continuous, but no register bucket for the in-place check

# two-tile pools under a 200-word batch: every lane is refilled several times
REFILL_SCHEDULES = [
    {"resident": True, "pool_tiles": 2, "_chunk": 128},
    {"resident": False, "group_tiles": 1, "_chunk": 128},
]
ROWS72_SCHEDULES = GEN_SCHEDULES + [{"resident": True, "pool_tiles": 2, "_chunk": 0}] + REFILL_SCHEDULES
COLS8_SCHEDULES = (GEN_SCHEDULES + [s for s in SCHEDULES if {"var_cpw", "nontemporal", "group_tiles"} & set(s)] + [
    {"resident": False, "var_cpw": 2},                         # grouped continuous, every columns-per-wave
    {"resident": False, "nontemporal": False, "var_cpw": 4},
    {"var_cpw": 1}, {"var_cpw": 2}, {"var_cpw": 4}, {"var_cpw": 8},  # the resident pool (in place)
    {"continuous": False, "var_cpw": 8},                       # fixed passes, nontemporal
    {"continuous": False, "nontemporal": False, "var_cpw": 2},
] + REFILL_SCHEDULES + [{"resident": True, "var_cpw": 8, "_chunk": 128}])


class _Mixed:
    """The graphs (one .pchk each, loaded by the oracle and the library), and
    per code and algorithm the channel words with the oracle's decode of them:
    built on first use, then shared by every test and left unchanged."""

    def __init__(self, gpu, oracle_mod, root):
        self.gpu, self.oracle_mod, self.root = gpu, oracle_mod, root
        self._graphs, self._words = {}, {}

    def graph(self, name):
        if name not in self._graphs:
            how, seed, (M, N), degrees, _, _ = CODES[name]
            rng = np.random.default_rng(seed)
            if how[0] == "reg":
                built = _regular_graph(rng, how[1], dv=how[2], dc=how[3])
            else:
                built = (_rows72_graph if how[0] == "rows72" else _cols8_graph)(rng, how[1], how[2])
            assert built[:2] == (M, N)
            path = self.root / f"{name}.pchk"
            _write_pchk(path, *built)
            og = self.oracle_mod.OracleGraph(str(path))
            G = self.gpu.Graph(str(path))
            assert (G.M, G.N, G.E) == (og.M, og.N, og.E) and (G.M, G.N) == (M, N)
            self._graphs[name] = (G, og)
        G, og = self._graphs[name]
        # the pairing the code is here for
        assert (G.dc, G.regular_dc, G.dv, G.regular_dv) == CODES[name][3], name
        return G, og

    def words(self, name, algo):
        """(codes, llr, oracle's (hard, post, iters, valid)) of the code's
        B-word batch for `algo`, the exits spread as the tests need them."""
        G, og = self.graph(name)
        key = (name, algo)
        if key not in self._words:
            seed, p = CODES[name][1], CODES[name][4 if algo == "bp" else 5]
            codes, llr = _channel(np.random.default_rng([seed, 0 if algo == "bp" else 1]), B, G.N, p)
            a = 0 if algo == "bp" else 1
            self._words[key] = (codes, llr, og.decode_batch(llr, MAX_ITER, algo=a, post_mode=1 if a == 0 else 0, threads=8))
        codes, llr, ref = self._words[key]
        _, _, it, v = ref
        # conditions on the input, on the oracle's output: early and late exits, decoded and failed words
        assert 1 < it.mean() < MAX_ITER, (name, algo, it.mean())
        assert v.any() and not v.all(), (name, algo)
        return codes, llr, ref


def _channel(rng, nwords, N, p):
    """+-ln 49 through a BSC of flip probability p, 1 % erasures and a few 3 ln 49,
    as int8 codes and as the fp64 LLRs the table gives them."""
    codes = np.where(rng.random((nwords, N)) < p, -1, 1).astype(np.int8)
    codes[rng.random((nwords, N)) < 0.01] = 0
    codes[rng.random((nwords, N)) < 0.002] = 3
    return codes, np.ascontiguousarray(TABLE[codes.astype(np.int64) + 128])


@pytest.fixture(scope="module")
def mixed(gpu, oracle_mod, tmp_path_factory):
    return _Mixed(gpu, oracle_mod, tmp_path_factory.mktemp("mixed"))


def _bitexact(mixed, name, schedule):
    schedule = dict(schedule)
    chunk = schedule.pop("_chunk", 256)
    G, _ = mixed.graph(name)
    for algo in ("bp", "msa"):
        codes, llr, (rh, rp, rit, rv) = mixed.words(name, algo)
        kw = dict(max_iter=MAX_ITER, algo=algo, post="ratio" if algo == "bp" else "llr", schedule=schedule, chunk=chunk)
        h, p, it, v = G.decode(llr, **kw)
        assert np.array_equal(it, rit), (algo, it, rit)
        assert np.array_equal(v, rv.astype(bool)) and np.array_equal(h, rh), algo
        assert np.array_equal(p.view(np.uint64), rp.view(np.uint64)), algo
        h2, p2, it2, v2 = G.decode_codes(codes, TABLE, **kw)
        assert np.array_equal(h2, h) and np.array_equal(it2, it) and np.array_equal(v2, v), algo
        assert np.array_equal(p2.view(np.uint64), p.view(np.uint64)), algo


@pytest.mark.timeout(120)
@pytest.mark.parametrize("sch", range(len(ROWS72_SCHEDULES)))
@pytest.mark.parametrize("name", ROWS72)
def test_rows72_schedules_bitexact(mixed, name, sch):
    """Rows all of degree 72, columns not all of degree 8: the resident pool
    runs k_check_bp / k_check_msa<72, ., RES> (in place, fused row parity,
    res_arrive) next to k_var_gr_cont<.., INPLACE>, the grouped schedule
    k_syndrome_split<72> next to k_var_gr_cont, fixed passes k_syndrome<72> +
    k_check<72> next to k_var_gr."""
    _bitexact(mixed, name, ROWS72_SCHEDULES[sch])


@pytest.mark.timeout(120)
@pytest.mark.parametrize("sch", range(len(COLS8_SCHEDULES)))
@pytest.mark.parametrize("name", COLS8)
def test_cols8_schedules_bitexact(mixed, name, sch):
    """Columns all of degree 8, rows not all of degree 72: k_var_m<., 8, ...>
    -- every columns-per-wave (falling back to 1 where 4 * cpw does not divide
    N), nontemporal, continuous and in-place forms -- next to k_check_gr,
    k_check_gr_res and, above row degree 96 (r8x100, where `resident` resolves
    to the grouped schedule), the memory-staged k_check_*_gen."""
    _bitexact(mixed, name, COLS8_SCHEDULES[sch])


@pytest.mark.timeout(120)
@pytest.mark.parametrize("name", list(CODES))
def test_mixed_fixed_passes_and_special_values(mixed, name):
    """Fixed passes and the default schedule on a ragged batch with erasures,
    -0.0, +-inf and a NaN; max_iter 0 and 1 (the step after a lane's Init is
    its last) on one code of each family."""
    G, og = mixed.graph(name)
    llr = _llr(np.random.default_rng(CODES[name][1] + 100), 130, G.N, "lattice")
    iters = (MAX_ITER, 0, 1) if name in ("r6x72", "r8x48") else (MAX_ITER,)
    for max_iter in iters:
        for sch in ({"continuous": False}, None):
            _cmp_nan(G, og, llr, max_iter, schedule=sch)
            _cmp_nan(G, og, llr, max_iter, algo="msa", schedule=sch)


@pytest.mark.timeout(120)
def test_mixed_engines_resolve_as_intended(mixed):
    """No decode: the engine each schedule resolves to, per code -- so that a
    pairing that fell back to another kernel family fails here instead of
    passing the decodes above vacuously.  None of the codes is (8, 72)-regular:
    no hand-over, no compressed min-sum, no first check from the prior."""
    gpu = mixed.gpu
    for name in CODES:
        G, _ = mixed.graph(name)
        cont, res = name not in NOT_CONTINUOUS, name not in NOT_RESIDENT
        for algo in ("bp", "msa"):
            # chunk 0: the engine's own pool; 256 and 128: the pools the decodes above name
            for chunk, schedule, want in ((0, {}, (res, cont)), (0, {"resident": True}, (res, cont)),
                                          (0, {"continuous": False}, (False, False)),
                                          (256, {}, (res, cont)), (256, {"resident": False}, (False, cont)),
                                          (128, {"resident": True, "pool_tiles": 2}, (res, cont))):
                eng = gpu.Engine(G, 0, algo, chunk, schedule)
                what = (name, algo, chunk, schedule)
                assert (eng.resident, eng.continuous) == want, what
                assert not (eng.handover or eng.msa_compressed or eng.first_from_prior), what
                assert eng.syndrome_split == (eng.continuous and not eng.resident), what
                if chunk:
                    assert eng.cap == chunk, what
                eng.close()
