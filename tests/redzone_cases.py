"""Codes, inputs and oracle references of the red-zone tests of the decoders
(tests/test_redzone_engine_gpu.py, tests/test_redzone_host_api_gpu.py).
Plain numpy, the CPU oracle and the library's host-only calls; no GPU.

Codes are the smallest the suite already builds:
  reg4    (8,72)-regular, N = 288 (refdec_cases): the specialised kernels, the
          resident pool, the hand-over, the fused row block, the wide hard stores
  reg2    (8,72)-regular, N = 144 (real_llr_cases): N % 32 != 0
  irr     40 x 130 (refdec_cases): generic buckets, an empty row and column
  n13     N = 13 (channel_cases)
  bucket  row degree 97, column degree 17 (test_random_graphs_gpu._bucket_graph):
          the memory-staged generic kernels
  n64, n65  the host pipeline's codes (test_host_pipeline_gpu): hard bits cross
          PCIe packed and unpacked

An input is int8 codes with the table k * UNIT: a random codeword (so the hard
bits hold both values) sent through a channel whose flip rate grows with the
word's index modulo 8 (so words stop at different iterations and some fail),
a few erasures and stronger values, an infinity and a NaN.  The same values
serve the three entry forms: codes, llr = table[codes + 128], and for BP
lr = the host exp(llr) as the oracle computes it.  Seed REAL is the checked
input, seed DECOY the one a decoy call runs on.
"""
import numpy as np

import channel_cases
import real_llr_cases
import refdec_cases
from redzone import nonconstant

UNIT = 1.25
TABLE = np.arange(-128, 128, dtype=np.float64) * UNIT
TABLE[128 + 100], TABLE[128 - 100], TABLE[128 + 101] = np.inf, -np.inf, np.nan
REAL, DECOY = 31, 32
B = 2 * 64 + 37
MAX_ITER = 12
ALGOS = {"bp": 0, "msa": 1, "qmsa": 2, "gallager_b1": 4}
QPARAMS = (6, 0.5, 0)   # the engine's defaults
TIE_SEED = 1234

# flip probability of the noisiest words
PMAX = {"reg4": 0.012, "reg2": 0.012, "irr": 0.05, "n13": 0.15, "bucket": 0.012, "n64": 0.05, "n65": 0.05}


def edges(name):
    if name == "reg4":
        return refdec_cases.make_edges("reg4")
    if name == "reg2":
        return real_llr_cases.regular_rows_permuted(2, 102)
    if name in ("irr", "n13"):
        return channel_cases.edges(name)
    if name == "bucket":
        from test_random_graphs_gpu import _bucket_graph
        rows, cols = _bucket_graph(np.random.default_rng(511), 20, 300, 97, 17)
        return 20, 300, rows, cols
    if name in ("n64", "n65"):
        from test_host_pipeline_gpu import CODES
        from test_random_graphs_gpu import _random_graph
        M, N, lo, hi = CODES[name]
        rows, cols = _random_graph(np.random.default_rng(4200 + N), M, N, lo, hi)
        return M, N, rows, cols
    raise KeyError(name)


def make_codes(enc, name, seed, nb=B):
    """int8 codes [nb][N] around random codewords of the encoder."""
    import synth
    N = enc.N
    rng = np.random.default_rng(seed * 1000 + N)
    cw = enc.encode_host(synth.random_messages(enc.K, 0, nb, seed)).astype(np.int64)
    p = PMAX[name] * (np.arange(nb) % 8) / 7.0
    flip = rng.random((nb, N)) < p[:, None]
    mag = rng.choice(np.array([1, 2, 3, 5]), p=[0.8, 0.1, 0.07, 0.03], size=(nb, N))
    k = np.where(cw ^ flip, -mag, mag)
    k[rng.random((nb, N)) < 0.01] = 0
    if nb > 4:
        k[1, 0], k[2, N - 1], k[4, N // 2] = 100, -100, 101
    return np.ascontiguousarray(k.astype(np.int8))


class Case:
    """One code on the host side: the .pchk, the oracle graph, the library's
    graph and encoder (host-only calls), the inputs of both seeds and the
    oracle's outputs, computed once per (seed, algo) and never changed."""

    def __init__(self, name, L, oracle_mod, tmp, nb=B, max_iter=MAX_ITER):
        self.name, self.nb, self.max_iter = name, nb, max_iter
        self.path = str(tmp / f"{name}.pchk")
        refdec_cases.write_pchk(self.path, *edges(name))
        self.og = oracle_mod.OracleGraph(self.path)
        self.G = L.Graph(self.path)
        self.N = self.G.N
        assert (self.G.M, self.G.N, self.G.E) == (self.og.M, self.og.N, self.og.E)
        enc = self.G.encoder()
        self.codes = {s: make_codes(enc, name, s, nb) for s in (REAL, DECOY)}
        self.llr = {s: np.ascontiguousarray(TABLE[c.astype(np.int64) + 128]) for s, c in self.codes.items()}
        self._lr, self._ref = {}, {}
        for a in self.codes.values():
            a.setflags(write=False)
        for a in self.llr.values():
            a.setflags(write=False)

    def lr(self, seed):
        """BP's likelihood ratios as the host computes them: the oracle's
        posterior ratio after 0 iterations, with the NaN its guard removes put back."""
        if seed not in self._lr:
            _, lr, _, _ = self.og.decode_batch(self.llr[seed], 0, algo=0, post_mode=1, threads=8)
            lr[np.isnan(self.llr[seed])] = np.nan
            lr.setflags(write=False)
            self._lr[seed] = lr
        return self._lr[seed]

    def ref(self, seed, algo):
        """(hard, post, iters, valid) of the oracle: BP's posterior ratio, the
        min-sum's L, the quantised min-sum's L_Q; Gallager B1 has no posterior."""
        if (seed, algo) not in self._ref:
            a = ALGOS[algo]
            if a < 2:
                r = self.og.decode_batch(self.llr[seed], self.max_iter, algo=a, post_mode=1 if a == 0 else 0, threads=8)
            else:
                q, step, beta = QPARAMS
                r = self.og.decode_int_batch(self.llr[seed], self.max_iter, a, q, step, beta, seed=TIE_SEED, threads=8)
                r = (r[0], r[1].astype(np.float64) if a == 2 else None, r[2], r[3])
            for x in r:
                if x is not None:
                    x.setflags(write=False)
            self._ref[seed, algo] = r
        return self._ref[seed, algo]

    def assert_nonconstant(self, algo):
        """From the reference alone: stale, poisoned or decoy data differs visibly."""
        h, p, it, v = self.ref(REAL, algo)
        what = (self.name, algo)
        nonconstant(h, what)
        nonconstant(v, what)
        # Gallager's decoders fall off a cliff (refdec_cases.CLIFF): a word stops at once or never
        spread = 2 if algo == "gallager_b1" else 3
        assert len(np.unique(it)) >= spread, (what, np.unique(it))
        if p is not None:
            nonconstant(p, what)
        dh, _, dit, dv = self.ref(DECOY, algo)
        differ = (h != dh).any(axis=1)  # (the word with a NaN decodes to one value on both sides)
        assert differ.sum() >= len(h) - 1, (what, "decoy rows equal to real rows", np.flatnonzero(~differ)[:8])
        if self.nb > 8:
            assert not np.array_equal(it, dit) and not np.array_equal(v, dv), what
            assert len(np.unique(it[:37])) >= spread and 0 < v[:37].sum() < 37, what  # the short batch's rows too


def same(got, ref, what, rows=None):
    """test_real_llr_gpu._same over the first `rows` rows of the reference."""
    h, p, it, v = got
    rh, rp, rit, rv = (None if r is None else r[:rows] for r in ref)
    assert np.array_equal(it, rit), (what, "iters", it, rit)
    assert np.array_equal(np.asarray(v, np.uint8), np.asarray(rv, np.uint8)), (what, "valid")
    assert np.array_equal(h, rh), (what, "hard", np.flatnonzero((h != rh).any(axis=1))[:8])
    if p is not None and rp is not None:
        nan = np.isnan(rp)
        assert np.array_equal(np.isnan(p), nan), (what, "posterior NaNs")
        assert np.array_equal(p[~nan].view(np.uint64), rp[~nan].view(np.uint64)), (what, "posterior")
