"""Independent numpy reference of the strand-index code for the tests:
systematic RS(8,4) over GF(16), primitive polynomial 19, generator roots
alpha^1..alpha^4, message symbols first.  Shares nothing with
csrc/rs_index.hpp: field products are carry-less multiplications reduced by
the polynomial (no log tables), the encoder is a polynomial long division
over all 65536 messages, the decoder is a brute-force nearest-codeword search.
"""
import functools
import itertools

import numpy as np

POLY = 19
N_SYM, K_SYM = 8, 4


def gf_mul(a, b):
    a = np.asarray(a, np.int64)
    b = np.asarray(b, np.int64)
    r = np.zeros(np.broadcast(a, b).shape, np.int64)
    for i in range(4):
        r ^= np.where((b >> i) & 1, a << i, 0)
    for bit in (6, 5, 4):
        r ^= np.where((r >> bit) & 1, POLY << (bit - 4), 0)
    return r


def generator():
    """g(x) = (x - a)(x - a^2)(x - a^3)(x - a^4), coefficients from x^4 down."""
    g = [1]
    root = 1
    for _ in range(4):
        root = int(gf_mul(root, 2))
        g = [int(x) ^ int(y) for x, y in zip(g + [0], [0] + [int(gf_mul(c, root)) for c in g])]
    return g


@functools.lru_cache(maxsize=None)
def codeword_symbols() -> np.ndarray:
    """[65536][8] uint8: the codeword of every 16-bit index (symbols 0..3 =
    the index, most significant nibble first; 4..7 = x^4 m(x) mod g(x))."""
    g = generator()
    idx = np.arange(1 << 16, dtype=np.int64)
    reg = np.zeros((1 << 16, N_SYM), np.int64)
    for j in range(K_SYM):
        reg[:, j] = (idx >> (12 - 4 * j)) & 15
    msg = reg[:, :K_SYM].copy()
    for i in range(K_SYM):
        coef = reg[:, i].copy()
        for k in range(5):
            reg[:, i + k] ^= gf_mul(coef, g[k])
    out = np.concatenate([msg, reg[:, K_SYM:]], axis=1).astype(np.uint8)
    out.setflags(write=False)
    return out


def pack(sym) -> np.ndarray:
    """[n][8] symbols -> uint32 words, symbol 0 in the top nibble."""
    s = np.asarray(sym, np.uint32).reshape(-1, N_SYM)
    w = np.zeros(len(s), np.uint32)
    for j in range(N_SYM):
        w |= s[:, j] << np.uint32(28 - 4 * j)
    return w


@functools.lru_cache(maxsize=None)
def _tables():
    v = np.arange(1 << 16)
    nib_weight = sum(((v >> (4 * k)) & 15) != 0 for k in range(4)).astype(np.uint8)
    parity = (pack(codeword_symbols()) & np.uint32(0xFFFF)).astype(np.int64)
    return nib_weight, parity


def brute_decode(sym, chunk: int = 1024):
    """Bounded-distance decode by exhaustive search: (index, distance) of the
    codeword within distance 2 of every word, or (-1, 3) when there is none
    (3 stands for "3 or more").  A codeword that close differs from the word
    in at most two of the four index symbols, so only those 1411 of the 65536
    codewords are compared in full -- the others are at distance >= 3 by
    their index symbols alone (brute_decode_full compares all of them; the
    tests check the two against each other).  The codeword is unique: d = 5."""
    nib_weight, parity = _tables()
    w = pack(sym).astype(np.int64)
    hi, lo = w >> 16, w & 0xFFFF
    delta = np.nonzero(nib_weight <= 2)[0].astype(np.int64)  # index-part differences of weight <= 2
    best = np.empty(len(w), np.int64)
    dist = np.empty(len(w), np.int64)
    for a in range(0, len(w), chunk):
        cand = hi[a:a + chunk, None] ^ delta[None, :]
        d = nib_weight[delta][None, :] + nib_weight[lo[a:a + chunk, None] ^ parity[cand]]
        k = d.argmin(axis=1)
        best[a:a + chunk] = cand[np.arange(len(k)), k]
        dist[a:a + chunk] = d.min(axis=1)
    far = dist > 2
    best[far], dist[far] = -1, 3
    return best, dist


def brute_decode_full(sym, chunk: int = 256):
    """Nearest codeword of every word, by distance to all 65536 codewords:
    (index of the nearest codeword, its Hamming distance in symbols).  The
    nearest codeword is unique when the distance is <= 2 (d = 5)."""
    nib_weight, parity = _tables()
    w = pack(sym).astype(np.int64)
    hi, lo = w >> 16, w & 0xFFFF
    idx = np.arange(1 << 16, dtype=np.int64)
    best = np.empty(len(w), np.int64)
    dist = np.empty(len(w), np.int64)
    for a in range(0, len(w), chunk):
        d = nib_weight[hi[a:a + chunk, None] ^ idx[None, :]] + nib_weight[lo[a:a + chunk, None] ^ parity[None, :]]
        best[a:a + chunk] = d.argmin(axis=1)
        dist[a:a + chunk] = d.min(axis=1)
    return best, dist


def strings(sym):
    """[n][8] symbols as 16-nt strings: symbol j = nt 2j (high pair), 2j+1 (low pair), A/C/G/T = 0..3."""
    s = np.asarray(sym, np.uint8).reshape(-1, N_SYM)
    nt = np.empty((len(s), 2 * N_SYM), np.uint8)
    nt[:, 0::2] = s >> 2
    nt[:, 1::2] = s & 3
    return [row.tobytes().decode() for row in np.frombuffer(b"ACGT", np.uint8)[nt]]


def symbols_of(seq: str) -> np.ndarray:
    v = ["ACGT".index(c) for c in seq[:2 * N_SYM]]
    return np.array([4 * v[2 * j] + v[2 * j + 1] for j in range(N_SYM)], np.uint8)


def single_errors(cw) -> np.ndarray:
    """All 8 * 15 = 120 words at distance 1 from the codeword."""
    out = []
    for p in range(N_SYM):
        for e in range(1, 16):
            w = np.array(cw, np.uint8)
            w[p] ^= e
            out.append(w)
    return np.array(out)


def double_errors(cw) -> np.ndarray:
    """All C(8,2) * 15 * 15 = 6300 words at distance 2 from the codeword."""
    out = []
    for p, q in itertools.combinations(range(N_SYM), 2):
        for e in range(1, 16):
            for f in range(1, 16):
                w = np.array(cw, np.uint8)
                w[p] ^= e
                w[q] ^= f
                out.append(w)
    return np.array(out)


def random_words() -> np.ndarray:
    """The 20000 uniformly random words of the decoder tests."""
    return np.random.default_rng(0).integers(0, 16, (20000, 8)).astype(np.uint8)
