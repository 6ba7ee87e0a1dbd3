"""The host decode pipeline (ldpc_decode / ldpc_decode_codes) over three and
more PCIe chunks: the only calls in which a staging half is used a second
time, so that the host waits for its earlier H2D copy and the copy stream
waits for the decode that last read its device buffers.

Chunks are 4096 codewords whatever N is, so two small random codes keep the
batches at a few MB: N = 64 (hard bits cross PCIe packed, N % 8 == 0) and
N = 65 (unpacked).  Each graph is written as a .pchk and loaded on both sides;
the oracle decodes every input once and the results are shared.

* fp64 input, five chunks with a ragged last one, whose contents make the
  staging halves change form: chunk 0 on the k * ln 49 lattice (with 0.0 and
  -0.0), 1 and 2 off it (half 0 goes coded -> fp64), 3 on it (half 1 goes
  fp64 -> coded), 4 on it except for one value in its last row (the fallback
  to fp64 after code pieces were enqueued);
* the same rows over two shards on one device (three chunks each);
* int8-coded input from pageable and from pinned memory, one device and two
  shards;
* the quantized min-sum with a tie seed over three chunks (the tie hash takes
  the codeword's index in the call, set per chunk)."""
import numpy as np
import pytest

from test_gpu_parity import _write_pchk
from test_random_graphs_gpu import _random_graph

pytestmark = pytest.mark.gpu

UNIT = 3.8918202981106265  # ln 49
X = 4096                   # codewords per PCIe chunk
B5 = 4 * X + 37            # five chunks; two shards of three chunks each
B3 = 2 * X + 37            # three chunks
MAX_ITER = 5
CODES = {"n64": (24, 64, 3, 12), "n65": (30, 65, 1, 20)}  # M, N, row degrees
ALGOS = [("bp", "ratio"), ("msa", "llr")]


def _lattice(rng, B, N):
    """Multiples of ln 49 near the all-zero codeword, so that codewords leave
    at different iterations, with erasures as 0.0 and -0.0."""
    k = rng.choice(np.array([1.0, -1.0, 2.0, -2.0, 3.0]), p=[0.84, 0.04, 0.06, 0.01, 0.05], size=(B, N))
    x = k * UNIT
    x[rng.random((B, N)) < 0.02] = 0.0
    x[rng.random((B, N)) < 0.01] = -0.0
    return x


def _five_chunks(rng, N):
    x = np.empty((B5, N))
    x[0:X] = _lattice(rng, X, N)
    x[X:3 * X] = rng.normal(3.0, 1.8, size=(2 * X, N))
    x[3 * X:] = _lattice(rng, B5 - 3 * X, N)
    x[B5 - 1, N // 2] = 1.25  # chunk 4: one value off the lattice, in its last row
    return np.ascontiguousarray(x)


class Code:
    pass


@pytest.fixture(scope="module", params=sorted(CODES))
def code(request, gpu, oracle_mod, tmp_path_factory):
    M, N, lo, hi = CODES[request.param]
    rng = np.random.default_rng(4200 + N)
    rows, cols = _random_graph(rng, M, N, lo, hi)
    path = tmp_path_factory.mktemp("pipeline") / f"{request.param}.pchk"
    _write_pchk(path, M, N, rows, cols)
    c = Code()
    c.og = oracle_mod.OracleGraph(str(path))
    c.G = gpu.Graph(str(path))
    assert (c.G.M, c.G.N, c.G.E) == (c.og.M, c.og.N, c.og.E)
    c.llr = _five_chunks(rng, N)
    c.codes = rng.choice(np.array([1, -1, 0, 2, -2, 3], np.int8), p=[0.83, 0.04, 0.03, 0.05, 0.01, 0.04], size=(B5, N))
    c.table = np.arange(-128, 128, dtype=np.float64) * UNIT
    c.ref = {}  # (input, algo) -> the oracle's outputs, computed once

    def ref(which, algo):
        if (which, algo) not in c.ref:
            x = c.llr if which == "llr" else np.ascontiguousarray(c.table[c.codes.astype(np.int64) + 128])
            a = 0 if algo == "bp" else 1
            r = c.og.decode_batch(x, MAX_ITER, algo=a, post_mode=1 if a == 0 else 0, threads=8)
            for arr in r:
                arr.setflags(write=False)
            c.ref[(which, algo)] = r
        return c.ref[(which, algo)]

    c.reference = ref
    return c


def _same(got, ref, what):
    """Hard bits, iterations and valid flags bit for bit; the posterior bit
    for bit except that a NaN only has to be matched by a NaN."""
    h, p, it, v = got
    rh, rp, rit, rv = ref
    assert np.array_equal(it, rit), what
    assert np.array_equal(v, np.asarray(rv).astype(bool)), what
    assert np.array_equal(h, rh), what
    nan = np.isnan(rp)
    assert np.array_equal(np.isnan(p), nan), what
    assert np.array_equal(p[~nan].view(np.uint64), rp[~nan].view(np.uint64)), what


@pytest.mark.parametrize("algo,post", ALGOS)
def test_five_chunks_fp64_one_device_and_two_shards(code, algo, post):
    ref = code.reference("llr", algo)
    one = code.G.decode(code.llr, max_iter=MAX_ITER, algo=algo, post=post)
    _same(one, ref, (algo, "one device"))
    assert 1 < ref[2].mean() < MAX_ITER  # codewords leave at different iterations: lanes are refilled
    two = code.G.decode(code.llr, max_iter=MAX_ITER, algo=algo, post=post, devices=[0, 0])
    _same(two, ref, (algo, "two shards"))
    _same(two, one, (algo, "two shards against one device"))
    # the same slot again: its staging halves start in the form the last call left
    _same(code.G.decode(code.llr, max_iter=MAX_ITER, algo=algo, post=post), ref, (algo, "second call"))


@pytest.mark.parametrize("algo,post", ALGOS)
def test_five_chunks_coded_pageable_pinned_shards(gpu, code, algo, post):
    ref = code.reference("codes", algo)
    llr = np.ascontiguousarray(code.table[code.codes.astype(np.int64) + 128])
    base = code.G.decode(llr, max_iter=MAX_ITER, algo=algo, post=post)
    _same(base, ref, (algo, "decode(table[codes + 128])"))
    pinned = gpu.host_empty(code.codes.shape, np.int8)
    pinned[...] = code.codes
    for name, src in (("pageable", code.codes), ("pinned", pinned)):
        for devs in (None, [0, 0]):
            got = code.G.decode_codes(src, code.table, max_iter=MAX_ITER, algo=algo, post=post, devices=devs)
            _same(got, base, (algo, name, devs))
    del pinned


def test_three_chunks_qmsa_tie_seed(code):
    """Erasures and small LLRs quantize to 0, so the tie hash decides; it is
    keyed by the codeword's index in the call (tie_base per chunk)."""
    x = np.array(code.llr[X - 5:X - 5 + B3])  # lattice, off-lattice and lattice rows
    x[::7, : code.G.N // 2] = 0.0
    x[::5, 3:9] *= 0.05
    rh, rp, rit, rv = code.og.decode_int_batch(x, MAX_ITER, 2, seed=1234, threads=8)
    h, p, it, v = code.G.decode(x, max_iter=MAX_ITER, algo="qmsa", post="llr", tie_seed=1234)
    assert np.array_equal(it, rit) and np.array_equal(v, rv.astype(bool)) and np.array_equal(h, rh)
    assert np.array_equal(p, rp)
    # the seed matters on these inputs: another one gives other hard bits
    rh2 = code.og.decode_int_batch(x, MAX_ITER, 2, seed=99, threads=8)[0]
    assert not np.array_equal(rh2, rh)
