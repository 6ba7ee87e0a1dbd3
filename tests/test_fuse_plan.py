"""Eligibility of the fused row block (LDPC_SCHED_FUSE_ROW_BLOCK), checked
without a GPU: csrc/engine_plan.hpp's block search (fuse_row_block_of: the
first of the 8 row blocks of M / 8 rows that holds every column exactly once)
and plan_engine's fuse_block, through a stand-alone host program
(tests/fuse_plan/fuse_check.cpp, engine_plan.hpp + graph.cpp, no HIP) built
with g++ into pytest's tmp_path.

The schedule runs only in the resident pool, for BP, on an (8, 72)-regular
code with such a block, with var_cpw at its default and the flag not turned
off; everything else keeps fuse_block = -1.  The codes of
fused_block_cases (the whole block is block 7, 3 or 1) give that block."""
import os
import subprocess

import numpy as np

import fused_block_cases
from conftest import PCHK, ROOT
from real_llr_cases import regular_rows_permuted
from test_gpu_parity import _write_pchk
from test_random_graphs_gpu import _regular_graph


def _line(name, M, N, block, fused):
    """block: the search's answer; fused: what the default BP plan takes
    (and a caller that sets the flag on); every other column is -1."""
    return f"{name}: M={M} N={N} block={block} bp={fused} cpw=-1 msa=-1 grouped=-1 off=-1 on={fused}"


def test_fuse_plan(tmp_path):
    exe = str(tmp_path / "fuse_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-o", exe,
                           os.path.join(ROOT, "tests", "fuse_plan", "fuse_check.cpp"),
                           os.path.join(ROOT, "dna-ldpc-codes_amd", "csrc", "graph.cpp")])
    # Q = 4, unpermuted: every row block is a permutation of the columns
    M, N, rows, cols = _regular_graph(np.random.default_rng(4), 4)
    _write_pchk(tmp_path / "reg4.pchk", M, N, rows, cols)
    # rows 0 and 3 * Q exchanged: blocks 0 and 3 now repeat columns (the rows of two independent random
    # permutations share a column with near certainty; asserted), block 1 is the first whole one
    swap = {0: 3 * 4, 3 * 4: 0}
    rows2 = [swap.get(r, r) for r in rows]
    by_row = {}
    for r, c in zip(rows2, cols):
        by_row.setdefault(r, set()).add(c)
    assert len(set().union(*(by_row[r] for r in range(4)))) < N
    _write_pchk(tmp_path / "swap4.pchk", M, N, rows2, cols)
    # rows permuted over all blocks: no block holds every column once (asserted)
    Mp, Np, rows3, cols3 = regular_rows_permuted(4, 104)
    for a in range(8):
        seen = [c for r, c in zip(rows3, cols3) if r // 4 == a]
        assert len(set(seen)) < len(seen)
    _write_pchk(tmp_path / "perm4.pchk", Mp, Np, rows3, cols3)
    # block a alone holds every column once, a = 7, 3, 1 (Q = 4) and 3 (Q = 12): the codes the GPU decodes
    # (tests/test_fused_block_position_gpu.py), from the same builder and seeds
    placed = []
    for name, (Q, a, _) in fused_block_cases.CODES.items():
        Mb, Nb, rows4, cols4 = fused_block_cases.code(name)
        assert (Mb, Nb) == (8 * Q, 72 * Q)
        _write_pchk(tmp_path / f"{name}.pchk", Mb, Nb, rows4, cols4)
        placed.append((name, Mb, Nb, a))
    assert [(n, a) for n, _, _, a in placed] == [("blk7_4", 7), ("blk3_4", 3), ("blk1_4", 1), ("blk3_12", 3)]
    r = subprocess.run([exe, f"dna={PCHK}", "rs7", f"reg4={tmp_path / 'reg4.pchk'}", f"swap4={tmp_path / 'swap4.pchk'}",
                        f"perm4={tmp_path / 'perm4.pchk'}"] + [f"{n}={tmp_path / (n + '.pchk')}" for n, _, _, _ in placed],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    want = [
        _line("dna", 2048, 18432, 0, 0),
        _line("rs7", 1024, 9216, 0, 0),
        _line("reg4", 32, 288, 0, 0),
        _line("swap4", 32, 288, 1, 1),
        _line("perm4", 32, 288, -1, -1),
        _line("blk7_4", 32, 288, 7, 7),
        _line("blk3_4", 32, 288, 3, 3),
        _line("blk1_4", 32, 288, 1, 1),
        _line("blk3_12", 96, 864, 3, 3),
    ]
    assert r.stdout.splitlines() == want
