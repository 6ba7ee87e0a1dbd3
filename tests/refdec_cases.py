"""Codes and inputs of the reference-decoder pin (tests/golden/refdec_goldens.npz,
tests/test_reference_decoder.py, tests/test_reference_decoder_gpu.py), shared
by the script that records the fixtures from oracle/_ref/librefdec.so and by
the tests that replay them.  Plain numpy, no GPU.

Every input is derived from integers -- a splitmix64 counter hash mapped to
dyadic values -- so that it regenerates bit for bit on any machine: no libm
function is called on either side.  Belief propagation takes likelihood ratios
(IN_LR) directly, so neither side computes an exp.
"""
import hashlib
import os

import numpy as np

GOLDEN = os.path.dirname(os.path.abspath(__file__)) + "/golden"
FIXTURE = os.path.join(GOLDEN, "refdec_goldens.npz")
DNA_PCHK = os.path.join(GOLDEN, "decode_n18432_m2048_final.pchk")

CODES = ("reg4", "perm4", "rs5", "irr", "dna")
SMALL = CODES[:4]
B_SMALL = 2 * 64 + 37  # a 64-lane pool refills twice and drains through a ragged tile
B_DNA = 8
RAW_WORDS = 2          # words per small code whose posterior is stored raw (all are stored as digests)
SEED, SEED_LIVE = 2024, 977  # the fixture's batch; the live test's second batch

QMSA_GRID = [(q, step, beta) for q in (3, 6) for step in (0.5, 2.0) for beta in (0, 1)]
GALLAGER = {"ga": 0, "gb1": 1, "gb2": 2}


def qname(q, step, beta):
    return f"q{q}_s{int(step * 10):02d}_b{beta}"


ALGOS = ("bp", "bpc", "msa", "ga", "gb1", "gb2") + tuple(qname(*c) for c in QMSA_GRID)
QCFG = {qname(*c): c for c in QMSA_GRID}

# ---------------------------------------------------------------------------
# counter hash
# ---------------------------------------------------------------------------
_M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def _splitmix64(x):
    with np.errstate(over="ignore"):
        x = (x + np.uint64(0x9E3779B97F4A7C15)) & _M64
        x = ((x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & _M64
        x = ((x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & _M64
        return x ^ (x >> np.uint64(31))


def _hash(seed, B, N):
    """[B][N] uint64, a function of (seed, b, j) alone."""
    s = _splitmix64(np.array([seed], np.uint64))[0]
    b = np.arange(B, dtype=np.uint64)[:, None]
    j = np.arange(N, dtype=np.uint64)[None, :]
    return _splitmix64(((b << np.uint64(24)) | j) ^ s)


def _tag(name):
    return int.from_bytes(hashlib.sha256(name.encode()).digest()[:4], "little")


# ---------------------------------------------------------------------------
# codes
# ---------------------------------------------------------------------------
def irregular_edges():
    """The 40 x 130 irregular code: column degrees 1..5 over rows 0..37, row 0
    filled to 12 entries, row 38 of degree 1, row 39 empty, column 129 empty,
    and the first entry written twice (the loaders keep one)."""
    M, N = 40, 130
    h = _hash(40130, N, 8)
    pairs = []
    for j in range(N - 1):
        d = 1 + int(h[j, 0] % np.uint64(5))
        rows = []
        for k in range(1, 8):
            r = int(h[j, k] % np.uint64(38))
            if r not in rows and len(rows) < d:
                rows.append(r)
        pairs += [(r, j) for r in rows]
    have = {j for r, j in pairs if r == 0}
    for j in range(0, N - 1, 9):
        if len(have) < 12 and j not in have:
            pairs.append((0, j))
            have.add(j)
    pairs.append((38, 7))
    pairs.append(pairs[0])
    return M, N, [r for r, _ in pairs], [c for _, c in pairs]


def alist_edges(text):
    """Edges of an alist file as RS_LDPC writes it: "M N", the two largest
    degrees, the degrees, then M row lists padded with zeros to the largest."""
    t = [int(v) for v in text.split()]
    M, N, width = t[0], t[1], t[2]
    rows, cols, at = [], [], 4 + M + N
    for i in range(M):
        for v in t[at:at + width]:
            if v:
                rows.append(i)
                cols.append(v - 1)
        at += width
    return M, N, rows, cols


def make_edges(name):
    """(M, N, rows, cols) of a generated code, as first made (the fixture keeps
    the list, so the tests never call this)."""
    import real_llr_cases
    from test_random_graphs_gpu import _regular_graph
    if name == "reg4":
        return _regular_graph(np.random.default_rng(4), 4)
    if name == "perm4":
        return real_llr_cases.regular_rows_permuted(4, 104)
    if name == "rs5":
        z = np.load(os.path.join(GOLDEN, "code_fixtures.npz"))
        return alist_edges(bytes(z["rs_5_16_4_alist"]).decode())
    if name == "irr":
        return irregular_edges()
    raise KeyError(name)


def write_pchk(path, M, N, rows, cols):
    """The .pchk record stream, entries in the order given (duplicates kept)."""
    by_row = {}
    for r, c in zip(rows, cols):
        by_row.setdefault(int(r), []).append(int(c))
    ints = [(ord("P") << 8) + 0x80, M, N]
    for r in sorted(by_row):
        ints.append(-(r + 1))
        ints.extend(c + 1 for c in by_row[r])
    ints.append(0)
    np.array(ints, dtype="<i4").tofile(str(path))


def file_sha(path):
    with open(path, "rb") as f:
        return hashlib.sha256(f.read()).hexdigest()


def row0_cols(rows, cols):
    return np.array(sorted({int(c) for r, c in zip(rows, cols) if r == 0}), np.int64)


def pchk_row0(path):
    """Columns of row 0 of a .pchk file, ascending."""
    a = np.fromfile(path, dtype="<i4")[3:]
    assert a[0] == -1
    end = int(np.argmax(a[1:] <= 0)) + 1
    return np.unique(a[1:end].astype(np.int64) - 1)


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------
# Per (code, family): max_iter and the noise of the batch.  The all-zero
# codeword is sent.  A position's level is 8, or with falling probability 7..1
# (priors for bit 0: a row of 72 needs strong ones to say anything), except at
# the word's noisy positions, where it is -1 or -2; a position is noisy with
# probability e_b / N, and e_b, the word's expected number of them, is spread
# over 0..emax by the word's hash.  Every ninth word has none (it stops at
# iteration 0).  emax and max_iter were chosen by looking at the REFERENCE's
# outputs alone, so that a batch mixes stops at 0, 1, several counts between
# and max_iter, valid words and failures (make_refdec_fixtures.py asserts it).
def _p(max_iter, emax, **kw):
    return dict(max_iter=max_iter, emax=emax, **kw)


NOISE = {
    ("reg4", "bp"): _p(20, 12), ("reg4", "bpc"): _p(20, 12), ("reg4", "msa"): _p(20, 12), ("reg4", "sign"): _p(10, 8),
    ("reg4", "gb2"): _p(10, 3),
    ("reg4", "q3_s05_b0"): _p(6, 12, unit=0.375), ("reg4", "q3_s05_b1"): _p(6, 12, unit=0.5),
    ("reg4", "q3_s20_b0"): _p(6, 12, unit=1.0), ("reg4", "q3_s20_b1"): _p(6, 24, unit=1.0),
    ("reg4", "q6_s05_b0"): _p(6, 12, unit=1.0), ("reg4", "q6_s05_b1"): _p(6, 12, unit=0.375),
    ("reg4", "q6_s20_b0"): _p(6, 12, unit=1.0), ("reg4", "q6_s20_b1"): _p(6, 12, unit=1.0),
    ("perm4", "bp"): _p(20, 12), ("perm4", "bpc"): _p(20, 12), ("perm4", "msa"): _p(20, 12),
    ("perm4", "sign"): _p(10, 8), ("perm4", "gb2"): _p(10, 3),
    ("perm4", "q3_s05_b0"): _p(6, 12, unit=0.375), ("perm4", "q3_s05_b1"): _p(6, 12, unit=0.5),
    ("perm4", "q3_s20_b0"): _p(6, 12, unit=1.0), ("perm4", "q3_s20_b1"): _p(6, 24, unit=1.0),
    ("perm4", "q6_s05_b0"): _p(6, 12, unit=1.5), ("perm4", "q6_s05_b1"): _p(6, 12, unit=0.375),
    ("perm4", "q6_s20_b0"): _p(6, 8, unit=1.0), ("perm4", "q6_s20_b1"): _p(6, 12, unit=1.5),
    ("rs5", "bp"): _p(20, 48), ("rs5", "bpc"): _p(20, 48), ("rs5", "msa"): _p(6, 70), ("rs5", "sign"): _p(10, 12),
    ("rs5", "q3_s05_b0"): _p(6, 12, unit=1.5), ("rs5", "q3_s05_b1"): _p(6, 12, unit=1.5),
    ("rs5", "q3_s20_b0"): _p(6, 48, unit=1.0), ("rs5", "q3_s20_b1"): _p(6, 96, unit=1.0),
    ("rs5", "q6_s05_b0"): _p(6, 20, unit=1.0, salt=1, bad=7), ("rs5", "q6_s05_b1"): _p(6, 20, unit=1.0, salt=2, bad=7),
    ("rs5", "q6_s20_b0"): _p(6, 20, unit=3.0, bad=5), ("rs5", "q6_s20_b1"): _p(6, 140, unit=1.0),
    ("irr", "bp"): _p(20, 20), ("irr", "bpc"): _p(20, 20), ("irr", "msa"): _p(20, 30), ("irr", "sign"): _p(10, 4),
    ("irr", "q3_s05_b0"): _p(6, 8, unit=1.0), ("irr", "q3_s05_b1"): _p(6, 12, unit=0.5),
    ("irr", "q3_s20_b0"): _p(6, 16, unit=1.5), ("irr", "q3_s20_b1"): _p(6, 24, unit=1.0),
    ("irr", "q6_s05_b0"): _p(6, 24, unit=1.0), ("irr", "q6_s05_b1"): _p(6, 24, unit=0.5),
    ("irr", "q6_s20_b0"): _p(6, 40, unit=2.0), ("irr", "q6_s20_b1"): _p(6, 24, unit=1.0),
    ("dna", "bp"): _p(15, 320, e1=1), ("dna", "bpc"): _p(15, 320, e1=1), ("dna", "msa"): _p(15, 480, e1=1),
    ("dna", "sign"): _p(10, 200, e1=1), ("dna", "q"): _p(10, 160, e1=1, lattice=True),
    ("dna", "ga"): _p(10, 100, e1=1), ("dna", "gb2"): _p(10, 60, e1=1),
    ("dna", "q3_s05_b0"): _p(10, 120, e1=1, lattice=True), ("dna", "q6_s20_b0"): _p(10, 60, e1=1, lattice=True, unit=2.0),
    ("dna", "q3_s20_b1"): _p(10, 160, e1=1, lattice=True, unit=2.0),
    ("dna", "q6_s20_b1"): _p(10, 160, e1=1, lattice=True, unit=2.0),
}

# Gallager's decoders fall off a cliff on these codes: a word is corrected in
# one or two iterations or not at all (on reg4, B2 fails on a single error), so
# the reference yields no three stopping counts between 1 and max_iter here.
# For these the script asserts 0, max_iter and the two quarters only, and
# records the spread it saw.
CLIFF = {("reg4", "ga"), ("reg4", "gb1"), ("reg4", "gb2"), ("perm4", "ga"), ("perm4", "gb1"), ("perm4", "gb2"),
         ("rs5", "gb1"), ("rs5", "gb2"), ("irr", "ga"), ("dna", "gb2")}
CLEAN_EVERY = 9


POOL_DNA = 32  # the DNA code's candidate words: e_b = emax * b / 31 (a few for words 1..5, 2 emax for the last four); 8 of them are kept


def _levels(seed, B, N, emax, e1=3, bad=1, lattice=False):
    h = _hash(seed, B, N)
    hb = _hash(seed ^ 0x5151, B, 1)[:, 0]
    if B == POOL_DNA:
        e = emax * np.arange(B, dtype=np.int64) // (B - 1)
        e[1:6] = (e1, e1, 2, 3, 5)
        e[28:] = 2 * emax
    else:
        e = ((hb >> np.uint64(20)) % np.uint64(emax + 1)).astype(np.int64)
        e[np.arange(B) % CLEAN_EVERY == 4] = 0
    u = ((h >> np.uint64(20)) & np.uint64(0xFFFFF)).astype(np.int64)
    noisy = u < (e[:, None] << 20) // N
    lev = np.full((B, N), 8, np.int64)  # 8 with probability 3/4, 7 with 3/16, ... down to 1
    zero = np.ones((B, N), bool)
    for k in range(7):
        zero &= ((h >> np.uint64(2 * k)) & np.uint64(3)) == 0
        lev -= zero
    lev[noisy] = (-bad - ((h >> np.uint64(14)) & np.uint64(1)).astype(np.int64))[noisy]
    mant = ((h >> np.uint64(40)) & np.uint64(1023)).astype(np.int64)
    if lattice:  # one magnitude, as a BSC gives: the quantised min-sum then meets few zero sums
        return np.where(noisy, -8, 8), np.zeros((B, N), np.int64)
    return lev, mant


def lr_input(seed, B, N, emax, e1=3):
    """Likelihood ratios k * 2^-10 in [2^-6, 2^8], skewed above 1:
    (1024 + mant) * 2^(level - 1 - 10), truncated to a multiple of 2^-10."""
    lev, mant = _levels(seed, B, N, emax, e1)
    t = np.where(lev > 0, lev - 1, lev * 3)  # 2^0..2^7 and 2^-3, 2^-6
    k = ((1024 + mant) << (t + 6)) >> 6
    return np.ascontiguousarray(k.astype(np.float64) * 2.0 ** -10)


def llr_input(seed, B, N, emax, unit=0.5, e1=3, bad=1, lattice=False):
    """Dyadic LLRs: (level * 256 + mant / 4) * 2^-8 * unit, the sign the level's."""
    lev, mant = _levels(seed, B, N, emax, e1, bad, lattice)
    return np.ascontiguousarray((lev * 256 + np.sign(lev) * (mant >> 2)).astype(np.float64) * (2.0 ** -8 * unit))


# The coded form of BP's input: int8 codes into a 256-entry table of likelihood
# ratios (table[code + 128]).  Entries 0..159: the ten levels x 16 mantissas;
# 160..: the directed values; the rest 1.
_LEVELS = (-2, -1, 1, 2, 3, 4, 5, 6, 7, 8)
_SPECIAL = {"zero": 160, "neg_zero": 161, "inf": 162, "nan": 163, "denorm_min": 164, "subnormal": 165,
            "tiny": 166, "huge": 167, "max": 168, "a": 169, "a_up": 170, "eighth": 171, "eight": 172, "quarter": 173}


def lr_table():
    t = np.ones(256)
    for li, lev in enumerate(_LEVELS):
        e = lev - 1 if lev > 0 else 3 * lev
        t[li * 16:li * 16 + 16] = (16 + np.arange(16)) * 2.0 ** (e - 4)
    a = 1.0 + 2.0 ** -7
    for k, v in dict(zero=0.0, neg_zero=-0.0, inf=np.inf, nan=np.nan, denorm_min=5e-324, subnormal=2.0 ** -1060,
                     tiny=2.0 ** -1000, huge=2.0 ** 1000, max=2.0 ** 1023, a=a, a_up=_ulp_up(a), eighth=2.0 ** -3,
                     eight=8.0, quarter=0.25).items():
        t[_SPECIAL[k]] = v
    return t


def lr_codes(seed, B, N, emax, e1, c, where):
    """int8 codes [B][N] with the directed entries planted into row 0's columns c."""
    lev, mant = _levels(seed, B, N, emax, e1)
    li = np.searchsorted(np.array(_LEVELS), lev)
    idx = li * 16 + (mant >> 6)
    S = _SPECIAL
    for kind, b in [kv for w in where for kv in w.items()]:
        if kind == "ulp":
            idx[b, c[0]], idx[b, c[-1]] = S["a"], S["a_up"]
        elif kind == "tie":
            idx[b, c[0]], idx[b, c[1]], idx[b, c[-2]], idx[b, c[-1]] = S["eighth"], S["eight"], S["eight"], S["eighth"]
        elif kind == "tiny":
            idx[b, c[:3]] = (S["denorm_min"], S["subnormal"], S["tiny"])
        elif kind == "huge":
            idx[b, c[:2]] = (S["huge"], S["max"])
        elif kind == "zero_inf":
            idx[b, c[:3]] = (S["zero"], S["neg_zero"], S["inf"])
        elif kind == "nan_first":
            idx[b, c[0]] = S["nan"]
        elif kind == "nan_second":
            idx[b, c[1]] = S["nan"]
        elif kind == "all_nan":
            idx[b, :] = S["nan"]
        if kind != "all_nan":
            idx[b, c[5]] = S["quarter"]
    return np.ascontiguousarray((idx - 128).astype(np.int8))


def _ulp_up(a):
    return np.array([a], np.float64).view(np.int64).__add__(1).view(np.float64)[0]


# codewords that carry directed values in row 0's columns (spread over the
# fills of a 64-lane pool and its ragged last tile); the DNA batch has 8 words
DIRECTED = {"ulp": 3, "tie": 41, "tiny": 64, "huge": 77, "zero_inf": 100, "nan_first": 131, "nan_second": 150,
            "all_nan": 163}
DIRECTED_DNA = ("ulp", "tiny", "huge", "zero_inf", "nan_first")  # candidate word b >= 2 carries kind b % 5


def _where(code, B):
    """A list of {kind: word} plantings."""
    if code != "dna":
        return [DIRECTED]
    return [{DIRECTED_DNA[b % 5]: b} for b in range(2, B)]


def plant(x, c, where, lr):
    """Overwrite entries of row 0 (columns c, ascending, at least 8) in a few
    codewords with the directed values of tests/real_llr_cases.py, in the
    likelihood-ratio domain (lr) or the LLR domain: one-ulp neighbours, a
    sign-opposed tie (a and 1 / a, or a and -a), subnormals, huge values,
    +-0, +-inf and NaN."""
    assert len(c) >= 8
    last = c[-1]
    for kind, b in [kv for w in where for kv in w.items()]:
        if kind == "ulp":
            a = 1.0 + 2.0 ** -7 if lr else 2.0 ** -5
            x[b, c[0]], x[b, last] = (a, _ulp_up(a)) if lr else (a, -_ulp_up(a))
        elif kind == "tie":
            x[b, c[0]], x[b, c[1]] = (2.0 ** -3, 2.0 ** 3) if lr else (2.0 ** -4, -2.0 ** -4)
            x[b, c[-2]], x[b, last] = (2.0 ** 3, 2.0 ** -3) if lr else (-2.0 ** -4, 2.0 ** -4)
        elif kind == "tiny":
            v = (5e-324, 2.0 ** -1060, 2.0 ** -1000, 2.0 ** -1022)
            x[b, c[:4]] = v if lr else (v[0], -v[1], v[2], -v[3])
        elif kind == "huge":
            v = (2.0 ** 1000, 2.0 ** 1023, 2.0 ** 700, 2.0 ** 64)
            x[b, c[:4]] = v if lr else (v[0], -v[1], 745.0, -745.0)
        elif kind == "zero_inf":
            x[b, c[:4]] = (0.0, -0.0, np.inf, np.inf if lr else -np.inf)
        elif kind == "nan_first":
            x[b, c[0]] = np.nan
        elif kind == "nan_second":
            x[b, c[1]] = np.nan
        elif kind == "all_nan":
            x[b, :] = np.nan
        if kind != "all_nan":  # one prior for bit 1: the first syndrome is not zero, the row is checked
            x[b, c[5]] = 2.0 ** -2 if lr else -2.0
    return x


# values of the quantiser row (tests/test_int_decoders.py: out of the int range), and in-range ones
QUANT_X = np.array([np.inf, -np.inf, np.nan, 1e300, -1e300, 2.0 ** 31 * 0.5, 2.0 ** 30 - 0.5, 2.0 ** 30, -2.0 ** 30,
                    0.0, -0.0, 0.24, 0.25, -0.25, 0.75, -1.25, 6.6, 7.75, 100.0, -100.0, 5e-324, -2.0 ** -1030])


def family(algo):
    return "bp" if algo in ("bp", "bpc") else "sign" if algo in GALLAGER else "msa" if algo == "msa" else "q"


def make_input(code, algo, N, c0, seed, noise):
    """The input batch of (code, algo): LR for bp, LLR otherwise (Gallager
    reads its signs).  c0 = row 0's columns.  For the DNA code this is the pool
    of candidate words; the fixture names the 8 it kept."""
    B = POOL_DNA if code == "dna" else B_SMALL
    p = noise[code, algo] if (code, algo) in noise else noise[code, family(algo)]
    s = seed ^ _tag(code + "/" + algo) ^ (p.get("salt", 0) << 8)
    where = _where(code, B)
    if algo == "bpc":  # the same values two ways: x = table[codes + 128]
        x = lr_table()[lr_codes(s, B, N, p["emax"], p.get("e1", 3), c0, where).astype(np.int64) + 128]
    elif algo == "bp":
        x = plant(lr_input(s, B, N, p["emax"], p.get("e1", 3)), c0, where, True)
    else:
        x = llr_input(s, B, N, p["emax"], p.get("unit", 0.5), p.get("e1", 3), p.get("bad", 1), p.get("lattice", False))
        if family(algo) != "q":  # the quantiser's out-of-range inputs have their own row (QUANT_X)
            x = plant(x, c0, where, False)
    x.setflags(write=False)
    return x, p["max_iter"]


def make_codes(code, N, c0, seed, noise):
    """The int8 codes behind make_input(code, "bpc", ...)."""
    B = POOL_DNA if code == "dna" else B_SMALL
    p = noise[code, "bpc"]
    s = seed ^ _tag(code + "/bpc") ^ (p.get("salt", 0) << 8)
    return lr_codes(s, B, N, p["emax"], p.get("e1", 3), c0, _where(code, B))


def recv_of(llr):
    """Gallager's received word: -1 for a negative LLR, else +1 (a NaN is +1)."""
    return np.where(llr < 0, -1, 1).astype(np.int32)


# ---------------------------------------------------------------------------
# comparing
# ---------------------------------------------------------------------------
def canon(post):
    """Posterior bytes with every NaN made the same NaN (a NaN matches a NaN)."""
    p = np.array(post, copy=True)
    if p.dtype == np.float64:
        p[np.isnan(p)] = np.nan
    return np.ascontiguousarray(p)


def digests(post, n=16):
    """[B][n] uint8: the first n bytes of sha256 over each word's canonical posterior bytes."""
    p = canon(post)
    return np.array([np.frombuffer(hashlib.sha256(p[b].tobytes()).digest()[:n], np.uint8) for b in range(len(p))])


SHORT = {"bp": (0, 1), "msa": (0, 1)}  # also recorded at these max_iter (8-byte digests), small codes only


def packbits(h):
    return np.packbits(np.asarray(h, np.uint8), axis=-1)


def same_bits(got, want, what):
    got, want = canon(got), canon(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    view = np.uint64 if got.dtype == np.float64 else got.dtype
    assert np.array_equal(got.view(view), want.view(view)), what


def compare(out, ref, ties, what):
    """out = (hard, post, iters, valid) of the side under test; ref the same
    from the reference with post as [B][16] digests."""
    h, p, it, v = out
    rh, rsha, rit, rv = ref
    free = np.ones(len(it), bool) if ties is None else ties == 0
    assert np.array_equal(it[free], rit[free]), (what, "iterations")
    assert np.array_equal(np.asarray(v, bool)[free], rv.astype(bool)[free]), (what, "valid")
    bad = [b for b in np.flatnonzero(free) if not np.array_equal(h[b], rh[b])]
    assert not bad, (what, "hard bits of words", bad[:8])
    if rsha is not None:
        sha = digests(p, rsha.shape[1])
        bad = [b for b in np.flatnonzero(free) if not np.array_equal(sha[b], rsha[b])]
        assert not bad, (what, "posterior bytes of words", bad[:8])
    if ties is not None:  # words with tie draws: the bits differ, so only where the counts agree
        for b in np.flatnonzero(~free & (it == rit)):
            assert np.array_equal(digests(p[b:b + 1], rsha.shape[1])[0], rsha[b]), (what, "L_Q of tie word", b)
            off = p[b] != 0
            assert np.array_equal(h[b][off], rh[b][off]), (what, "hard bits of tie word", b)


def recorded(fx, code, algo, N, short=None):
    """((hard, digests, iters, valid), ties) as recorded; short = 0 or 1: the record at that max_iter."""
    k = f"{code}/{algo}/"
    it = fx[k + "iters"].astype(np.int32)
    if short is not None:
        it, k = np.minimum(it, short), k + f"m{short}/"
    hard = np.unpackbits(fx[k + "hard"], axis=-1)[:, :N]
    return (hard, fx.get(k + "post_sha"), it, fx[k + "valid"]), fx.get(k + "ties")


def recorded_input(fx, code, algo, N, c0):
    x, max_iter = make_input(code, algo, N, c0, SEED, NOISE)
    if code == "dna":
        x = np.ascontiguousarray(x[fx[f"dna/{algo}/words"]])
    assert hashlib.sha256(x.tobytes()).hexdigest() == str(fx[f"{code}/{algo}/in_sha256"]), (code, algo, "input")
    assert max_iter == int(fx[f"{code}/{algo}/max_iter"])
    return x, max_iter


def compare_raw(fx, code, algo, out):
    """The first words' posteriors themselves, where the fixture holds them
    (the quantised min-sum's: of the words without a tie draw)."""
    k = f"{code}/{algo}/"
    if k + "post_raw" in fx:
        ties = fx.get(k + "ties")
        rows = [b for b in range(RAW_WORDS) if ties is None or ties[b] == 0]
        same_bits(np.asarray(out[1])[rows], fx[k + "post_raw"][rows], (code, algo, "posterior"))
