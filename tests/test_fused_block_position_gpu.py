"""The fused row block (LDPC_SCHED_FUSE_ROW_BLOCK) where it is not block 0.
Every other code the suite decodes has its whole block first: row0 = 0,
k_check_bp_skip skips rows [0, Q), and a column's own edge in its fused row
is slot 0 of its 8 edges.  The codes of fused_block_cases have block a = 7,
3 and 1 of Q = 4 rows (N = 288) and block 3 of Q = 12 rows (N = 864: a fused
grid of 12 x tiles, xcd_block with nb > 8 and nb % 8 != 0; 24 check blocks),
so k_var_bp_fused gets row0 = a * Q, finds the LDS slot by eid[k][s] == ea
among all eight slots (different slots among the 9 columns of one wave) and
stores lr to edges beyond the first block, and the check skips rows
[a * Q, (a + 1) * Q).  Their structure is asserted from the graph alone in
tests/test_fused_block_cases.py, their plan in tests/test_fuse_plan.py.

Nothing a codeword computes changes: every case equals the oracle and the
schedule without the flag bit for bit -- hard bits, iteration counts, valid
flags and the posterior ratio's bytes.

Inputs: those of test_fused_rowblock_gpu and test_fused_paths_gpu; the
Gaussian input carries real_llr_cases' directed rows (NaN, +-huge, subnormal,
one-ulp, ties) twice, in disjoint codewords: in the columns of row a * Q (the
fused block: LDS and the in-kernel check) and in those of a row outside the
block (the check kernel)."""
import numpy as np
import pytest

import fused_block_cases as F
import synth
from test_fused_paths_gpu import PathCase
from test_fused_paths_gpu import _on_off as _on_off_b
from test_fused_rowblock_gpu import CHUNKS, LN49, MIXED_ITER, _on_off, _resolved, _same
from test_gpu_parity import _write_pchk
from test_real_llr_gpu import _same as _same_msa

pytestmark = pytest.mark.gpu

NAMES = list(F.CODES)
TWO = ["blk3_12", "blk7_4"]


class BlockCase(PathCase):
    """A code of fused_block_cases with Case's inputs and oracle cache."""

    def __init__(self, name, gpu, oracle_mod, tmp):
        self.name = name
        path = str(tmp / f"{name}.pchk")
        _write_pchk(path, *F.code(name))
        self.G = gpu.Graph(path)
        self.og = oracle_mod.OracleGraph(path)
        self.sigma, self.own_iter = F.sigma_and_iter(name)
        self._in, self._oracle = {}, {}

    def gauss(self, B):
        if ("gauss", B) not in self._in:
            self._in["gauss", B] = F.gaussian_input(self.G, self.name, B)
        return self._in["gauss", B]


@pytest.fixture(scope="module")
def cases(gpu, oracle_mod, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("fused_block_position")
    made = {}

    def get(name):
        if name not in made:
            made[name] = BlockCase(name, gpu, oracle_mod, tmp)
        return made[name]
    return get


@pytest.mark.timeout(120)
@pytest.mark.parametrize("name", NAMES)
def test_flag_runs_where_it_says(gpu, cases, name):
    c = cases(name)
    for chunk in CHUNKS:
        assert _resolved(gpu, c.G, chunk) == (True, True)
        assert _resolved(gpu, c.G, chunk, fuse_row_block=False) == (True, False)
        assert _resolved(gpu, c.G, chunk, var_cpw=2) == (True, False)  # an explicit var_cpw keeps k_var_m
        assert _resolved(gpu, c.G, chunk, resident=False) == (False, False)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("name", NAMES)
def test_real_llrs(cases, name, chunk):
    """fp64 priors (off the lattice), hand-over on and off, max_iter 0, 1, 3
    and the case's own; without the posterior at the case's own."""
    c = cases(name)
    for ho in (True, False):
        for mi in (0, 1, 3, c.own_iter):
            _, _, it, v = _on_off(c, "gauss", chunk, mi, {"handover": ho})
        assert len(np.unique(it)) > 3 and not v.all() and v.any()  # early exits, late exits, failures
        _on_off(c, "gauss", chunk, c.own_iter, {"handover": ho}, post=False)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("name", TWO)
def test_lattice_input_coded_and_fp64(cases, name, chunk):
    """The coded variable kernel (lr_table: int8 priors) and the fp64 one on
    the same lattice input."""
    c = cases(name)
    for table in (True, False):
        for ho in (True, False):
            for mi in (0, 1, 3, MIXED_ITER):
                _, _, it, v = _on_off(c, "mixed", chunk, mi, {"handover": ho, "lr_table": table}, post=(mi != 3))
                assert (it[1::2] == 0).all() and v[1::2].all()


@pytest.mark.timeout(120)
@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("name", TWO)
def test_lockstep_tiles(cases, name, chunk):
    """`noisy`: a tile's lanes start together and run the plain path (a
    window of columns in flight per wave) together; also with one fill only
    (B = pool)."""
    c = cases(name)
    for B in (None, chunk):
        for mi in (1, 2, 5):
            for ho in (True, False):
                for table in (True, False):
                    _, _, it, _ = _on_off_b(c, "noisy", chunk, mi, {"handover": ho, "lr_table": table}, B=B)
                    assert (it == mi).mean() > 0.5  # most lanes of a tile in lockstep to the end


@pytest.mark.timeout(120)
@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("name", TWO)
def test_drain_finished_outputs_only(cases, name, chunk):
    """`clean`: every codeword is valid at iteration 0, so every step after
    a refill hands out finished codewords only (the `touched == 0` return
    behind the barrier); also with one fill only (B = pool)."""
    c = cases(name)
    for B in (None, chunk):
        for ho in (True, False):
            for table in (True, False):
                _, _, it, v = _on_off_b(c, "clean", chunk, 5, {"handover": ho, "lr_table": table}, B=B)
                assert (it == 0).all() and v.all()


@pytest.mark.timeout(120)
def test_device_resident_codes(gpu, cases):
    """Engine.decode_codes on device buffers: +-1 codes, the table k * ln 49."""
    L = gpu
    c = cases("blk3_12")
    G, B, mi = c.G, 2 * 192 + 37, 5
    x = c.mixed(B)
    ref = c.oracle("mixed", B, mi)
    codes = np.ascontiguousarray(np.where(x > 0, 1, -1).astype(np.int8))
    table = np.arange(-128, 128, dtype=np.float64) * synth.LLR_UNIT
    assert table[129] == LN49
    d_in = L.DeviceBuffer(0, codes.size)
    d_in.upload(codes)
    d_h, d_p, d_i, d_v = L.DeviceBuffer(0, B * G.N), L.DeviceBuffer(0, B * G.N * 8), L.DeviceBuffer(0, B * 4), \
        L.DeviceBuffer(0, B)
    out = {}
    try:
        for fuse in (True, False):
            eng = L.Engine(G, 0, "bp", fuse_row_block=fuse)
            try:
                assert eng.resident and eng.fused_row_block == fuse and eng.cap == 192
                eng.decode_codes(d_in.at(0), table, L.IN_LLR, B, mi, d_h.at(0), d_p.at(0), L.POST_RATIO, d_i.at(0),
                                 d_v.at(0))
                eng.sync()
                out[fuse] = (d_h.download(np.empty((B, G.N), np.uint8)), d_p.download(np.empty((B, G.N), np.float64)),
                             d_i.download(np.empty(B, np.int32)), d_v.download(np.empty(B, np.uint8)).astype(bool))
            finally:
                eng.close()
    finally:
        for b in (d_in, d_h, d_p, d_i, d_v):
            b.free()
    _same(out[True], ref, "codes on == oracle")
    _same(out[True], out[False], "codes on == off")


@pytest.mark.timeout(120)
def test_neighbours_do_not_fuse(gpu, cases, oracle_mod):
    """Paths that ignore the block: min-sum at its default schedule
    (compressed where the plan takes it) and with fp64 messages, and BP with
    var_cpw = 4, where the flag resolves off.  All equal the oracle."""
    c = cases("blk3_12")
    B = 2 * 64 + 37
    x = c.gauss(B)
    ref = c.og.decode_batch(x, c.own_iter, algo=oracle_mod.ALGO_MSA, post_mode=oracle_mod.POST_LLR, threads=16)
    eng = gpu.Engine(c.G, 0, "msa", chunk=64)
    try:
        assert not eng.fused_row_block
        compressed = eng.msa_compressed
    finally:
        eng.close()
    # (min-sum leaves a NaN prior's posterior NaN: the comparison of test_real_llr_gpu)
    for sch in (None, {"msa_compressed": compressed}, {"msa_compressed": False, "resident": True}):
        got = c.G.decode(x, max_iter=c.own_iter, algo="msa", post="llr", chunk=64, schedule=sch)
        _same_msa(got, ref, ("blk3_12", "msa", sch))
    assert _resolved(gpu, c.G, 64, var_cpw=4) == (True, False)
    got = c.G.decode(x, max_iter=c.own_iter, post="ratio", chunk=64, schedule={"var_cpw": 4})
    _same(got, c.oracle("gauss", B, c.own_iter), ("blk3_12", "bp", "var_cpw=4"))
