"""Inputs of tests/test_real_llr_gpu.py: real-valued (off-lattice) channel
LLRs for the (8, 72)-regular codes, the directed rows planted into them, the
properties asserted on them before anything is decoded, and the argument
sets of the device exp / log checks.  Plain numpy, no GPU: the CPU suite
uses the same inputs to put the host libm on the same scale
(tests/test_decoder_reference.py)."""
import numpy as np

from test_random_graphs_gpu import _regular_graph

B = 200  # with chunk=64: three refills of the lane pool and a ragged tile of 8

# sigma of the BI-AWGN channel (all-zero codeword, LLR = 2y / sigma^2) per code
# and algorithm, chosen on the CPU with the oracle so that the batch mixes early
# exits, late exits and failures (asserted in the tests); max_iter next to it.
SIGMA = {
    ("reg2", "bp"): (0.44, 20), ("reg2", "msa"): (0.40, 20),
    ("reg16", "bp"): (0.44, 25), ("reg16", "msa"): (0.40, 25),
    ("rs7", "bp"): (0.46, 25), ("rs7", "msa"): (0.42, 10),
    ("dna", "bp"): (0.46, 15), ("dna", "msa"): (0.43, 15),
}


def regular_rows_permuted(Q, seed):
    """A random (8, 72)-regular code (M = 8Q, N = 72Q): _regular_graph with
    its rows permuted, so that a column's edges do not lie one per row block
    (DeviceGraph::build then keeps the compressed min-sum's v2c in plain
    column order)."""
    rng = np.random.default_rng(seed)
    M, N, rows, cols = _regular_graph(rng, Q)
    perm = rng.permutation(M)
    return M, N, [int(perm[r]) for r in rows], cols


def edge_s_in_row_block_s(G):
    """Whether edge s of every column lies in row block s (M / dv rows per
    block): the condition under which DeviceGraph::build lays the compressed
    min-sum's v2c out row-block-major."""
    rp, ci, cp, ce = G.edges()
    if G.M % G.dv or not G.regular_dv:
        return False
    edge_row = np.repeat(np.arange(G.M), np.diff(rp))
    blk = edge_row[ce].reshape(G.N, G.dv) // (G.M // G.dv)
    return bool((blk == np.arange(G.dv)[None, :]).all())


def gaussian_llrs(N, nb, sigma, seed):
    y = 1.0 + sigma * np.random.default_rng(seed).normal(size=(nb, N))
    return np.ascontiguousarray(2.0 * y / sigma ** 2)


# codewords that carry a directed row 0 (spread over the fills of a 64-lane
# pool and its last, ragged tile)
DIRECTED = {"ulp_up": 3, "ulp_down": 41, "tie_first": 64, "tie_last": 77, "tiny": 100, "huge": 131,
            "nan_first": 150, "nan_second": 197, "all_nan": 199}


def plant_directed(llr, row_cols, where=DIRECTED):
    """Overwrite entries of row `row_cols` (its 72 columns, ascending) in a
    few codewords; returns the codeword indices touched."""
    c = np.asarray(row_cols)
    assert len(c) == 72

    def below(b, k):
        """A magnitude well below every other one of the row in codeword b."""
        return float(np.abs(np.delete(llr[b, c], k)).min()) / 8.0

    # two magnitudes one ulp apart, in both orders: min1 / min2 differ in the last bit only
    b = where["ulp_up"]; a = below(b, [5, 40]); llr[b, c[5]], llr[b, c[40]] = a, -np.nextafter(a, np.inf)
    b = where["ulp_down"]; a = below(b, [5, 40]); llr[b, c[5]], llr[b, c[40]] = -np.nextafter(a, np.inf), a
    # equal magnitudes, opposite signs, at the first two / last two columns: the first-index rule
    b = where["tie_first"]; a = below(b, [0, 1]); llr[b, c[0]], llr[b, c[1]] = a, -a
    b = where["tie_last"]; a = below(b, [70, 71]); llr[b, c[70]], llr[b, c[71]] = -a, a
    # subnormal and 1e-300 magnitudes
    b = where["tiny"]
    llr[b, c[2]], llr[b, c[17]], llr[b, c[33]], llr[b, c[60]] = 5e-324, -3e-310, 1e-300, -1e-300
    # LR = exp(LLR) at the overflow / underflow edge (exp(700) finite, exp(745) = inf, exp(-745) subnormal)
    b = where["huge"]
    llr[b, c[3]], llr[b, c[9]], llr[b, c[11]], llr[b, c[13]] = 700.0, -700.0, 745.0, -745.0
    # a NaN at the row's first / second edge beside distinct finite magnitudes (the |x0| / |x1| planes)
    llr[where["nan_first"], c[0]] = np.nan
    llr[where["nan_second"], c[1]] = np.nan
    # one negative prior in each of them: the first syndrome is not zero, so the row is checked at least once
    for k, b in where.items():
        llr[b, c[30]] = -abs(llr[b, c[30]])
    llr[where["all_nan"], :] = np.nan
    return sorted(where.values())


def first_check_positions(llr, G):
    """Over rows x codewords of the first check (v2c = the channel LLR):
    counts[0][k] = how often position k of a row holds the strictly unique
    smallest magnitude, counts[1][k] = the strictly unique second smallest.
    Rows with a NaN are left out."""
    rp, ci, _, _ = G.edges()
    dc = G.dc
    mag = np.abs(llr[:, ci.reshape(G.M, dc)])  # [B][M][dc]
    ok = ~np.isnan(mag).any(-1)
    order = np.argsort(mag, axis=-1, kind="stable")
    s = np.take_along_axis(mag, order[..., :3], axis=-1)
    u1 = ok & (s[..., 0] < s[..., 1])
    u2 = u1 & (s[..., 1] < s[..., 2])
    return (np.bincount(order[..., 0][u1], minlength=dc), np.bincount(order[..., 1][u2], minlength=dc))


# ---------------------------------------------------------------------------
# device exp / log
# ---------------------------------------------------------------------------
LOG_DBL_MAX = 709.782712893384  # exp overflows just above it
LOG_DENORM_MIN = -745.1332191019411  # exp reaches 0 just below it


def exp_inputs(N=144, rows=64):
    """One batch [rows][N] of exp arguments: Gaussian values, a log-spaced
    sweep of +-[1e-300, 745], the neighbours of ln(DBL_MAX) and of
    ln(denorm_min), arguments whose result is subnormal, +-0, +-inf, NaN."""
    rng = np.random.default_rng(709)
    sweep = np.geomspace(1e-300, 745.0, 2500)
    near = []
    for v in (LOG_DBL_MAX, LOG_DENORM_MIN, -708.3964185322641):  # the last: ln(DBL_MIN)
        lo = hi = v
        near.append(v)
        for _ in range(40):
            lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
            near += [lo, hi]
    parts = [sweep, -sweep, np.array(near), np.linspace(-745.2, -708.0, 600), rng.normal(0.0, 6.0, 1500),
             rng.normal(0.0, 0.05, 300), np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1.0, -1.0, 709.0, -744.0])]
    x = np.concatenate(parts)
    out = rng.normal(1.5, 2.5, size=rows * N)
    assert x.size <= out.size
    out[: x.size] = x
    return np.ascontiguousarray(out.reshape(rows, N))


def ulp_distance(got, want):
    """Units in the last place between two float64 arrays of finite values or
    equal infinities: the distance between their positions on the ordered
    line of doubles (exact for subnormals; +0 and -0 coincide)."""
    def line(v):
        i = np.ascontiguousarray(v, np.float64).view(np.int64)
        return np.where(i < 0, np.int64(-2 ** 63) - i, i)
    return np.abs(line(got) - line(want))
