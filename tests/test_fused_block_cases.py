"""The codes of tests/fused_block_cases.py, checked without a GPU: what the
GPU tests of a fused row block that is not block 0
(tests/test_fused_block_position_gpu.py) rely on, from the graph alone, and
that the oracle's decodes of their Gaussian input mix early exits, late exits
and failures."""
import numpy as np
import pytest

import fused_block_cases as F
import real_llr_cases as C
from test_gpu_parity import _write_pchk

NAMES = list(F.CODES)


@pytest.fixture(scope="module")
def graphs(L, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("fused_block_cases")
    out = {}
    for name in NAMES:
        path = str(tmp / f"{name}.pchk")
        _write_pchk(path, *F.code(name))
        out[name] = (L.Graph(path), path)
    return out


@pytest.mark.parametrize("name", NAMES)
def test_one_whole_block_and_its_slots(name):
    Q, a, _ = F.CODES[name]
    M, N, rows, cols = F.code(name)
    assert (M, N, len(rows)) == (8 * Q, 72 * Q, 8 * 72 * Q)
    assert F.whole_blocks(M, N, rows, cols) == [a]
    hist = np.bincount(F.own_slots(M, N, rows, cols, a), minlength=8).tolist()
    assert hist == F.SLOT_HIST[name]


def test_slots_covered():
    hist = {name: np.bincount(F.own_slots(*F.code(name), F.CODES[name][1]), minlength=8) for name in NAMES}
    assert (sum(hist.values()) > 0).all()  # every slot 0..7 over the four codes
    assert (hist["blk3_12"] > 0).all()  # and in blk3_12 alone
    assert hist["blk7_4"][7] == 288  # the last block: always the last slot
    for name in ("blk3_12", "blk3_4"):  # the slot differs between the columns of one wave
        assert F.wave_slot_counts(*F.code(name), F.CODES[name][1]).max() >= 3


@pytest.mark.parametrize("name", NAMES)
def test_loaded_graph_agrees(graphs, name):
    """The library's graph (what the kernels index): its rows hold their
    columns ascending, its col_edge lists a column's edges by ascending row,
    so the own edge's slot is own_slots'; and edge s of a column does not lie
    in row block s, so the compressed min-sum keeps plain column order."""
    Q, a, _ = F.CODES[name]
    G, _ = graphs[name]
    M, N, rows, cols = F.code(name)
    assert (G.M, G.N, G.dv, G.dc, G.regular_dv, G.regular_dc) == (M, N, 8, 72, True, True)
    rp, ci, cp, ce = G.edges()
    assert (np.diff(ci.reshape(M, 72), axis=1) > 0).all()
    by_col = ce.reshape(N, 8)
    assert (np.diff(by_col, axis=1) > 0).all()
    own = by_col // 72 // Q == a  # edge e lies in row e // 72
    assert (own.sum(1) == 1).all()
    assert np.array_equal(own.argmax(1), F.own_slots(M, N, rows, cols, a))
    assert not C.edge_s_in_row_block_s(G)
    r = F.outside_row(G, a)
    assert r // Q != a and 0 <= r < M


@pytest.mark.parametrize("name", NAMES)
def test_oracle_spread(graphs, oracle_mod, name):
    """The Gaussian input of the GPU tests (B = 2 * pool + 37 for pools of 64
    and 192): the directed rows are in place in both rows, and the oracle
    gives more than three distinct iteration counts, valid words and
    failures."""
    Q, a, _ = F.CODES[name]
    G, path = graphs[name]
    og = oracle_mod.OracleGraph(path)
    rp, ci, _, _ = G.edges()
    _, max_iter = F.sigma_and_iter(name)
    for B in (2 * 64 + 37, 2 * 192 + 37):
        x = F.gaussian_input(G, name, B)
        for row, shift in ((a * Q, 0), (F.outside_row(G, a), 1)):
            w = F.directed_where(B, shift)
            c = ci[rp[row]:rp[row + 1]]
            assert np.isnan(x[w["nan_first"], c[0]]) and np.isnan(x[w["nan_second"], c[1]])
            assert np.isnan(x[w["all_nan"]]).all()
            assert x[w["huge"], c[11]] == 745.0 and x[w["tiny"], c[2]] == 5e-324
            assert x[w["tie_first"], c[0]] == -x[w["tie_first"], c[1]]
        _, p, it, v = og.decode_batch(x, max_iter, algo=oracle_mod.ALGO_BP, post_mode=oracle_mod.POST_RATIO, threads=4)
        assert not np.isnan(p).any()  # BP's guard: a NaN product is 1
        print(name, B, "distinct iteration counts", len(np.unique(it)), "failures", int((~v.astype(bool)).sum()))
        assert len(np.unique(it)) > 3 and v.any() and not v.all()
