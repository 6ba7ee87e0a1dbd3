"""One engine used again and again (ldpc_amd.Engine on DeviceBuffers): the
buffers an engine allocates on first use and regrows (the fp64 staging of
coded fixed passes, the prior table, the posterior planes, the lane codes),
the launch sampler behind profile() / stats(), and engines created and closed
in a row.  Two small codes: a random (8, 72)-regular one (N = 144: grouped
continuous BP, compressed min-sum) and an irregular one (the resident pool of
the generic kernels, messages in place).  Every decode must equal the oracle
on table[codes + 128] bit for bit, whatever the engine did before it."""
import math

import numpy as np
import pytest

from test_gpu_parity import _write_pchk
from test_random_graphs_gpu import _random_graph, _regular_graph

pytestmark = pytest.mark.gpu

MAX_ITER = 12
BMAX = 200
SCHEDULES = {"default": {}, "grouped": {"resident": False}, "fixed": {"continuous": False}}


def _tables(unit):
    """(LLR table, BP's LR table by the host libm exp the library and the reference use)"""
    llr = np.arange(-128, 128, dtype=np.float64) * unit
    return llr, np.array([math.exp(x) for x in llr])


class Case:
    def __init__(self, L, oracle_mod, path, seed):
        self.G = L.Graph(str(path))
        self.og = oracle_mod.OracleGraph(str(path))
        rng = np.random.default_rng(seed)
        N = self.G.N
        codes = np.where(rng.random((BMAX, N)) < 0.04, -1, 1).astype(np.int8)
        codes[rng.random((BMAX, N)) < 0.02] = 0
        codes[rng.random((BMAX, N)) < 0.01] = 3
        self.codes = codes
        self.ref = {}  # (unit, algo, B) -> the oracle's (hard, posterior, iterations, valid)

    def expect(self, unit, algo, B):
        key = (unit, algo, B)
        if key not in self.ref:
            llr = np.ascontiguousarray(_tables(unit)[0][self.codes[:B].astype(np.int64) + 128])
            a = 0 if algo == "bp" else 1
            self.ref[key] = self.og.decode_batch(llr, MAX_ITER, algo=a, post_mode=1 if a == 0 else 0, threads=8)
        return self.ref[key]


@pytest.fixture(scope="module")
def cases(gpu, oracle_mod, tmp_path_factory):
    d = tmp_path_factory.mktemp("engine_reuse")
    M, N, rows, cols = _regular_graph(np.random.default_rng(2), 2)
    _write_pchk(d / "reg2.pchk", M, N, rows, cols)
    rows, cols = _random_graph(np.random.default_rng(1004), 24, 64, 3, 12)
    _write_pchk(d / "irr.pchk", 24, 64, rows, cols)
    return {"regular": Case(gpu, oracle_mod, d / "reg2.pchk", 11), "irregular": Case(gpu, oracle_mod, d / "irr.pchk", 12)}


def _run(L, eng, B, N, fn, post=True):
    dh, dit, dv = L.DeviceBuffer(0, B * N), L.DeviceBuffer(0, B * 4), L.DeviceBuffer(0, B)
    dp = L.DeviceBuffer(0, B * N * 8) if post else None
    fn(dh.at(0), dp.at(0) if post else None, dit.at(0), dv.at(0))
    eng.sync()
    return (dh.download(np.empty((B, N), np.uint8)), dp.download(np.empty((B, N), np.float64)) if post else None,
            dit.download(np.empty(B, np.int32)), dv.download(np.empty(B, np.uint8)))


def _check(out, ref, what):
    h, p, it, v = out
    rh, rp, rit, rv = ref
    assert np.array_equal(it, rit) and np.array_equal(v.astype(bool), rv.astype(bool)) and np.array_equal(h, rh), what
    if p is not None:
        assert np.array_equal(p.view(np.uint64), rp.view(np.uint64)), what


def _post_kind(L, algo):
    return L.POST_RATIO if algo == "bp" else L.POST_LLR


@pytest.mark.parametrize("algo", ["bp", "msa"])
@pytest.mark.parametrize("name", ["regular", "irregular"])
def test_staging_regrows_and_tables_alternate(gpu, cases, name, algo):
    """Fixed passes of 128 on codes: batches of 64, 200 (two passes; the
    staging grows once) and 64 again, with table A, table B, then A again."""
    L, c = gpu, cases[name]
    N = c.G.N
    eng = L.Engine(c.G, 0, algo, chunk=128, schedule={"continuous": False})
    assert not eng.continuous and eng.cap == 128
    codes = L.DeviceBuffer(0, BMAX * N)
    codes.upload(c.codes)
    for B, unit in ((64, 1.2), (200, 0.7), (64, 1.2)):
        tab = _tables(unit)[0]
        out = _run(L, eng, B, N, lambda h, p, it, v: eng.decode_codes(codes.at(0), tab, L.IN_LLR, B, MAX_ITER, h, p,
                                                                      _post_kind(L, algo), it, v))
        _check(out, c.expect(unit, algo, B), (name, algo, B, unit))
    eng.close()


@pytest.mark.parametrize("sch", list(SCHEDULES))
@pytest.mark.parametrize("algo", ["bp", "msa"])
@pytest.mark.parametrize("name", ["regular", "irregular"])
def test_posterior_allocated_on_first_use(gpu, cases, name, algo, sch):
    """No posterior, then one, then none: the posterior planes appear with the
    first decode that asks for them and later decodes are not disturbed."""
    L, c = gpu, cases[name]
    N, B, unit = c.G.N, 130, 1.2
    eng = L.Engine(c.G, 0, algo, schedule=SCHEDULES[sch])
    llr, lr = _tables(unit)
    idx = c.codes[:B].astype(np.int64) + 128
    d_in = L.DeviceBuffer(0, B * N * 8)
    d_in.upload(np.ascontiguousarray((lr if algo == "bp" else llr)[idx]))
    kind = L.IN_LR if algo == "bp" else L.IN_LLR
    for post in (False, True, False):
        out = _run(L, eng, B, N, lambda h, p, it, v: eng.decode(d_in.at(0), kind, B, MAX_ITER, h, p,
                                                                _post_kind(L, algo), it, v), post=post)
        _check(out, c.expect(unit, algo, B), (name, algo, sch, post))
    eng.close()


@pytest.mark.parametrize("name,algo,sch", [("regular", "bp", "default"), ("regular", "msa", "default"),
                                           ("irregular", "bp", "default"), ("irregular", "msa", "default"),
                                           ("regular", "bp", "fixed"), ("irregular", "msa", "fixed")])
def test_sampled_launches(gpu, cases, name, algo, sch):
    """profile(stride): every stride-th launch of a class is timed, counted
    from the class's first launch; the launch counts and the results do not
    depend on the stride."""
    L, c = gpu, cases[name]
    N, B, unit = c.G.N, 130, 1.2
    eng = L.Engine(c.G, 0, algo, schedule=SCHEDULES[sch])
    codes = L.DeviceBuffer(0, BMAX * N)
    codes.upload(c.codes)
    tab = _tables(unit)[0]

    def decode():
        out = _run(L, eng, B, N, lambda h, p, it, v: eng.decode_codes(codes.at(0), tab, L.IN_LLR, B, MAX_ITER, h, p,
                                                                      _post_kind(L, algo), it, v))
        return out, eng.stats()

    decode()  # the lane codes, the table and the posterior planes exist from here on
    eng.profile(1)
    out1, s1 = decode()
    assert sum(k["launches"] for k in s1.values()) > 0
    for cls, k in s1.items():
        assert k["sampled"] == k["launches"], (cls, k)
        assert (k["ms"] > 0) == (k["launches"] > 0), (cls, k)
    eng.profile(3)
    out3, s3 = decode()
    for cls, k in s3.items():
        assert k["launches"] == s1[cls]["launches"], (cls, k)
        assert k["sampled"] == -(-k["launches"] // 3), (cls, k)
    eng.profile(0)
    out0, s0 = decode()
    for cls, k in s0.items():
        assert k["launches"] == s1[cls]["launches"] and k["sampled"] == 0 and k["ms"] == 0, (cls, k)
    for out in (out1, out3, out0):
        _check(out, c.expect(unit, algo, B), (name, algo, sch))
    eng.close()


def test_engines_created_and_closed_in_a_row(gpu, cases):
    """Eight engines, one after the other, on one graph: the resident pool
    (messages in place, no scratch), the grouped schedule (both go through the
    placement probe), fixed passes and min-sum; then a ninth."""
    L, c = gpu, cases["irregular"]
    N, B, unit = c.G.N, 130, 0.7
    codes = L.DeviceBuffer(0, BMAX * N)
    codes.upload(c.codes)
    tab = _tables(unit)[0]
    kinds = [("bp", "default"), ("bp", "grouped"), ("bp", "fixed"), ("msa", "default")]
    for i in range(9):
        algo, sch = kinds[i % 4]
        eng = L.Engine(c.G, 0, algo, schedule=SCHEDULES[sch])
        assert eng.resident == (sch == "default") and eng.continuous == (sch != "fixed")
        out = _run(L, eng, B, N, lambda h, p, it, v: eng.decode_codes(codes.at(0), tab, L.IN_LLR, B, MAX_ITER, h, p,
                                                                      _post_kind(L, algo), it, v))
        _check(out, c.expect(unit, algo, B), (i, algo, sch))
        eng.close()
