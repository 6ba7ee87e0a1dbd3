"""Codes whose fused row block (LDPC_SCHED_FUSE_ROW_BLOCK, engine_plan.hpp's
fuse_row_block_of) is not block 0, shared by the CPU tests of their structure
(tests/test_fused_block_cases.py, tests/test_fuse_plan.py) and the GPU tests
that decode them (tests/test_fused_block_position_gpu.py).  Plain numpy.

With block a > 0 fused, k_var_bp_fused gets row0 = a * Q, k_check_bp_skip
skips rows [a * Q, (a + 1) * Q), and a column's own edge in its fused row is
no longer slot 0 of its 8 edges but the rank of that row among the column's
rows -- any of 0..7, differing between the columns of one wave."""
import numpy as np

import real_llr_cases as C
from test_random_graphs_gpu import _regular_graph

DV, DC = 8, 72

# name -> (Q, a, seed): Q rows per block, a the one block that holds every
# column once.  blk3_12: the fused grid's x dimension is 12 (xcd_block with
# nb > 8, nb % 8 != 0) and the check grid 24 blocks of 4 rows.
CODES = {"blk7_4": (4, 7, 7), "blk3_4": (4, 3, 3), "blk1_4": (4, 1, 1), "blk3_12": (12, 3, 13)}

# The own-edge slot's histogram per code (own_slots), from the graph alone.
SLOT_HIST = {
    "blk7_4": [0, 0, 0, 0, 0, 0, 0, 288],
    "blk3_4": [3, 22, 69, 106, 59, 24, 5, 0],
    "blk1_4": [81, 132, 69, 6, 0, 0, 0, 0],
    "blk3_12": [17, 76, 193, 288, 201, 73, 15, 1],
}


def regular_fused_block_at(Q, a, seed):
    """A random (8, 72)-regular code (M = 8Q, N = 72Q) in which row block a,
    and with near certainty no other, holds every column once (asserted by
    the structure test): _regular_graph's block 0 goes to rows
    [aQ, (a + 1)Q), shuffled within, and its other 7Q rows to a random
    permutation of the remaining positions.  Returns (M, N, rows, cols) for
    _write_pchk."""
    rng = np.random.default_rng(seed)
    M, N, rows, cols = _regular_graph(rng, Q)
    perm = np.empty(M, np.int64)
    perm[:Q] = a * Q + rng.permutation(Q)
    rest = np.concatenate([np.arange(0, a * Q), np.arange((a + 1) * Q, M)])
    perm[Q:] = rng.permutation(rest)
    return M, N, [int(perm[r]) for r in rows], cols


def code(name):
    return regular_fused_block_at(*CODES[name])


def sigma_and_iter(name):
    """The BI-AWGN sigma and max_iter of the code's Gaussian input: those of
    real_llr_cases' codes of the same size."""
    return C.SIGMA["reg2" if CODES[name][0] == 4 else "reg16", "bp"]


def outside_row(G, a):
    """The row outside block a that shares the fewest columns with row a * Q
    (the lowest such row).  None shares no column: the Q rows of every other
    block hold all N columns between them."""
    rp, ci, _, _ = G.edges()
    Q = G.M // DV
    own = set(ci[rp[a * Q]:rp[a * Q + 1]].tolist())
    shared = [len(own & set(ci[rp[r]:rp[r + 1]].tolist())) if r // Q != a else DC + 1 for r in range(G.M)]
    return int(np.argmin(shared))


def directed_where(B, shift):
    """Codeword indices of the directed rows (real_llr_cases.DIRECTED, or a
    compact set for a batch shorter than that), moved up by `shift`."""
    base = C.DIRECTED if B > max(C.DIRECTED.values()) + 1 else {k: 3 + 7 * i for i, k in enumerate(C.DIRECTED)}
    where = {k: b + shift for k, b in base.items()}
    assert max(where.values()) < B
    return where


def gaussian_input(G, name, B):
    """BI-AWGN LLRs of the all-zero codeword with real_llr_cases' directed
    rows (NaN, +-huge, subnormal, one-ulp, ties) planted twice, in disjoint
    sets of codewords: into the columns of row a * Q, the fused block's first
    row, whose d travel through LDS and the in-kernel check, and into the
    columns of a row outside the block, which the check kernel handles."""
    Q, a, _ = CODES[name]
    rp, ci, _, _ = G.edges()
    x = C.gaussian_llrs(G.N, B, sigma_and_iter(name)[0], 1)
    inside, outside = directed_where(B, 0), directed_where(B, 1)
    assert not set(inside.values()) & set(outside.values())
    r = outside_row(G, a)
    assert r // Q != a
    C.plant_directed(x, ci[rp[a * Q]:rp[a * Q + 1]], inside)
    C.plant_directed(x, ci[rp[r]:rp[r + 1]], outside)
    x.setflags(write=False)
    return x


def whole_blocks(M, N, rows, cols):
    """The row blocks of M / 8 rows that hold every column exactly once."""
    blk = np.asarray(rows) // (M // DV)
    c = np.asarray(cols)
    return [b for b in range(DV) if np.array_equal(np.sort(c[blk == b]), np.arange(N))]


def own_slots(M, N, rows, cols, a):
    """slot[j]: the rank of column j's block-a row among its 8 rows -- the
    slot of the column's 8 edges (ascending edge index = ascending row) that
    k_var_bp_fused keeps in LDS."""
    Q = M // DV
    r, c = np.asarray(rows), np.asarray(cols)
    order = np.lexsort((r, c))
    by_col = r[order].reshape(N, DV)  # each column's rows, ascending
    assert np.array_equal(c[order].reshape(N, DV), np.repeat(np.arange(N)[:, None], DV, 1))
    own = by_col // Q == a
    assert (own.sum(1) == 1).all()
    return own.argmax(1)


def wave_slot_counts(M, N, rows, cols, a, waves=8):
    """Per (row of block a, wave): how many distinct own-edge slots the wave's
    DC / waves columns hold; a wave's columns are the row's columns
    ascending, in groups of DC / waves (kFuseWaves = 8: groups of 9)."""
    Q = M // DV
    slot = own_slots(M, N, rows, cols, a)
    r, c = np.asarray(rows), np.asarray(cols)
    out = np.zeros((Q, waves), np.int64)
    for i in range(Q):
        cs = np.sort(c[r == a * Q + i])
        assert len(cs) == DC
        for w in range(waves):
            out[i, w] = len(set(slot[cs[w * (DC // waves):(w + 1) * (DC // waves)]].tolist()))
    return out
