"""Fused row block (LDPC_SCHED_FUSE_ROW_BLOCK): in the resident BP pool of an
(8, 72)-regular code with a row block that holds every column once, the
variable kernel runs one workgroup per row of that block, keeps the block's
variable->check messages in LDS and finishes the rows' check update itself
(k_var_bp_fused); the check kernel leaves those rows' messages alone
(k_check_bp_skip).  Nothing a codeword computes changes: every case equals
the oracle and the schedule without the flag bit for bit -- hard bits,
iteration counts, valid flags and the posterior ratio's bytes (BP's NaN guard
leaves no NaN in it).

Codes: the unpermuted random (8, 72)-regular code with Q = 4 rows per block
(N = 288, the smallest with N % 32 == 0: one check block of the fused row
block per tile) and Q = 16 (N = 1152), RS-LDPC(7, 72, 8) (N = 9216), the DNA
code once, and a code with permuted rows, where the flag resolves off.
Inputs: real-valued LLRs with the directed rows of real_llr_cases (NaN,
+-huge, subnormal, one-ulp rows), and +-ln 49 lattice input, noiseless rows
alternating with BSC p = 0.02 rows, which ldpc_decode codes (lr_table) or
passes as fp64.  B = 2 * pool + 37 over pools of 64 and 192 lanes: refills, a
ragged last tile and a drain."""
import numpy as np
import pytest

import real_llr_cases as C
import synth
from conftest import PCHK
from test_gpu_parity import _write_pchk
from test_random_graphs_gpu import _regular_graph

pytestmark = pytest.mark.gpu

LN49 = 3.8918202981106265
CHUNKS = (64, 192)
SIGMA = {"reg4": C.SIGMA["reg2", "bp"], "reg16": C.SIGMA["reg16", "bp"], "rs7": C.SIGMA["rs7", "bp"],
         "perm4": C.SIGMA["reg2", "bp"], "dna": C.SIGMA["dna", "bp"]}
MIXED_ITER = 20


def _bits(a):
    return a.view(np.uint64) if a.dtype == np.float64 else np.asarray(a)


def _same(got, ref, what):
    for g, r in zip(got, ref):
        if g is None or r is None:
            continue
        assert np.array_equal(_bits(np.asarray(g)), _bits(np.asarray(r).astype(np.asarray(g).dtype))), what


class Case:
    """One code: its graph on both sides, the two inputs for a batch of B
    codewords, and the oracle's outputs, computed once per (input, max_iter)."""

    def __init__(self, name, gpu, oracle_mod, tmp):
        self.name = name
        if name == "dna":
            path = PCHK
        else:
            path = str(tmp / f"{name}.pchk")
            if name == "rs7":
                gpu.Graph.rs_ldpc(7, 72, 8).save_pchk(path)
            elif name.startswith("perm"):
                _write_pchk(path, *C.regular_rows_permuted(int(name[4:]), 104))
            else:
                _write_pchk(path, *_regular_graph(np.random.default_rng(int(name[3:])), int(name[3:])))
        self.G = gpu.Graph(path)
        self.og = oracle_mod.OracleGraph(path)
        self.sigma, self.own_iter = SIGMA[name]
        self._in, self._oracle = {}, {}

    def gauss(self, B):
        """BI-AWGN LLRs of the all-zero codeword with the directed rows
        planted into row 0's columns (real_llr_cases)."""
        if ("gauss", B) not in self._in:
            rp, ci, _, _ = self.G.edges()
            x = C.gaussian_llrs(self.G.N, B, self.sigma, 1)
            where = C.DIRECTED if B > max(C.DIRECTED.values()) else {k: 3 + 7 * i for i, k in enumerate(C.DIRECTED)}
            C.plant_directed(x, ci[rp[0]:rp[1]], where)
            x.setflags(write=False)
            self._in["gauss", B] = x
        return self._in["gauss", B]

    def mixed(self, B):
        """+-ln 49: odd rows noiseless (valid at iteration 0), even rows a
        BSC with p = 0.02 on the all-zero codeword."""
        if ("mixed", B) not in self._in:
            rng = np.random.default_rng(77)
            x = np.full((B, self.G.N), LN49)
            flip = rng.random((B, self.G.N)) < 0.02
            flip[1::2] = False
            x[flip] = -LN49
            x.setflags(write=False)
            self._in["mixed", B] = x
        return self._in["mixed", B]

    def oracle(self, kind, B, max_iter):
        k = (kind, B, max_iter)
        if k not in self._oracle:
            x = self.gauss(B) if kind == "gauss" else self.mixed(B)
            h, p, it, v = self.og.decode_batch(x, max_iter, algo=0, post_mode=1, threads=16)
            assert not np.isnan(p).any()  # BP's guard: a NaN product is 1
            self._oracle[k] = (h, p, it, v.astype(bool))
        return self._oracle[k]


@pytest.fixture(scope="module")
def cases(gpu, oracle_mod, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("fused")
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(name, gpu, oracle_mod, tmp)
        return made[name]
    return get


def _resolved(L, G, chunk, **kw):
    eng = L.Engine(G, 0, "bp", chunk=chunk, **kw)
    try:
        assert bool(eng.flags & L.SCHED_FLAGS["fuse_row_block"]) == eng.fused_row_block
        return eng.resident, eng.fused_row_block
    finally:
        eng.close()


def _on_off(c, kind, chunk, max_iter, sch, post=True):
    """Flag on and off: both equal the oracle and each other."""
    B = 2 * chunk + 37
    x = c.gauss(B) if kind == "gauss" else c.mixed(B)
    ref = c.oracle(kind, B, max_iter)
    out = {}
    for fuse in (True, False):
        s = dict(sch, resident=True, fuse_row_block=fuse)
        got = c.G.decode(x, max_iter=max_iter, post="ratio" if post else None, chunk=chunk, schedule=s)
        _same(got, ref, (c.name, kind, chunk, max_iter, sch, fuse, "oracle"))
        out[fuse] = got
    _same(out[True], out[False], (c.name, kind, chunk, max_iter, sch, "on == off"))
    return out[True]


@pytest.mark.timeout(120)
@pytest.mark.parametrize("name", ["reg4", "reg16", "rs7"])
def test_flag_runs_where_it_says(gpu, cases, name):
    c = cases(name)
    for chunk in CHUNKS:
        assert _resolved(gpu, c.G, chunk) == (True, True)
        assert _resolved(gpu, c.G, chunk, fuse_row_block=False) == (True, False)
        assert _resolved(gpu, c.G, chunk, var_cpw=2) == (True, False)  # an explicit var_cpw keeps k_var_m
        assert _resolved(gpu, c.G, chunk, resident=False) == (False, False)


@pytest.mark.timeout(300)
@pytest.mark.parametrize("chunk", CHUNKS)
@pytest.mark.parametrize("name", ["reg4", "reg16", "rs7"])
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
@pytest.mark.parametrize("name", ["reg4", "reg16", "rs7"])
def test_lattice_input_coded_and_fp64(cases, name, chunk):
    """The coded variable kernel (lr_table: int8 priors) and the fp64 one on
    the same lattice input."""
    c = cases(name)
    for table in (True, False):
        for ho in (True, False):
            for mi in (0, 1, 3, MIXED_ITER):
                _, _, it, v = _on_off(c, "mixed", chunk, mi, {"handover": ho, "lr_table": table}, post=(mi != 3))
                assert (it[1::2] == 0).all() and v[1::2].all()


@pytest.mark.timeout(300)
def test_dna_code_once(gpu, cases):
    """The DNA code, 200 codewords through its default 3-tile pool."""
    c = cases("dna")
    assert _resolved(gpu, c.G, 0) == (True, True)
    x = c.gauss(200)
    ref = c.oracle("gauss", 200, c.own_iter)
    on = c.G.decode(x, max_iter=c.own_iter, post="ratio")
    off = c.G.decode(x, max_iter=c.own_iter, post="ratio", schedule={"fuse_row_block": False})
    _same(on, ref, "dna on == oracle")
    _same(on, off, "dna on == off")


@pytest.mark.timeout(120)
def test_permuted_rows_resolve_off(gpu, cases):
    """No row block holds every column once: the flag resolves off, whatever
    the caller sets, and the decode is exact."""
    c = cases("perm4")
    assert _resolved(gpu, c.G, 64) == (True, False)
    assert _resolved(gpu, c.G, 64, fuse_row_block=True) == (True, False)
    _on_off(c, "gauss", 64, c.own_iter, {})
    _on_off(c, "mixed", 64, 3, {})


@pytest.mark.timeout(120)
def test_device_resident_codes(gpu, cases):
    """Engine.decode_codes on device buffers: +-1 codes, the table k * ln 49."""
    L = gpu
    c = cases("rs7")
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
