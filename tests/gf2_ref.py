"""Reference for the systematic encoder (numpy only, test infrastructure).

Row-reduces H with its columns reversed, rows packed 8 bits per byte: the
pivot columns of the reduced row echelon form are the columns independent of
all later columns of H, i.e. the encoder's parity positions (include/ldpc_amd.h
"Systematic encoding"), and every reduced row gives one parity bit as the XOR
of information bits.  The library builds a column basis with tracked
combinations instead (csrc/gf2.hpp); the two share no step.

Also the small codes that tests/test_encoder*.py share.
"""
import numpy as np


def dense(G) -> np.ndarray:
    """H of a Graph as uint8 [M][N]."""
    rp, ci, _, _ = G.edges()
    H = np.zeros((G.M, G.N), np.uint8)
    H[np.repeat(np.arange(G.M), np.diff(rp)), ci] = 1
    return H


def rref_reversed(H):
    """RREF of H[:, ::-1] over GF(2).  Returns (R, piv): R uint8 [rank][N] in
    H's own column order, piv[i] the column of H that row i solves."""
    H = np.asarray(H, np.uint8) & 1
    M, N = H.shape
    R = np.packbits(H[:, ::-1], axis=1)
    piv = []
    r = 0
    for c in range(N):
        if r == M:
            break
        byte, bit = c >> 3, 0x80 >> (c & 7)
        cand = np.nonzero(R[r:, byte] & bit)[0]
        if cand.size == 0:
            continue
        p = r + int(cand[0])
        if p != r:
            R[[r, p]] = R[[p, r]]
        others = np.nonzero(R[:, byte] & bit)[0]
        others = others[others != r]
        R[others] ^= R[r]
        piv.append(N - 1 - c)
        r += 1
    return np.unpackbits(R[:r], axis=1, count=N)[:, ::-1], np.array(piv, np.int64)


def rank(A) -> int:
    return len(rref_reversed(A)[1])


class RefEncoder:
    def __init__(self, H):
        H = np.asarray(H, np.uint8)
        self.N = H.shape[1]
        R, piv = rref_reversed(H)
        self.rank = len(piv)
        self.K = self.N - self.rank
        self.par_pos = np.sort(piv)
        self.info_pos = np.setdiff1d(np.arange(self.N), piv)
        self._piv = piv
        self._P = R[:, self.info_pos].astype(np.int64)  # [rank][K]: parity bit i = P[i] . m

    def encode(self, msg) -> np.ndarray:
        m = np.asarray(msg, np.int64)
        cw = np.zeros((m.shape[0], self.N), np.uint8)
        cw[:, self.info_pos] = m
        cw[:, self._piv] = (m @ self._P.T) & 1
        return cw


# --- the small codes of the encoder tests: (M, N, rows, cols) -------------
def random_edges(seed, M, N, deg=(2, 6)):
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    for i in range(M):
        for j in rng.choice(N, size=int(rng.integers(deg[0], deg[1] + 1)), replace=False):
            rows.append(i)
            cols.append(int(j))
    return M, N, rows, cols


def hamming_edges():
    H = np.array([[1, 0, 1, 0, 1, 0, 1], [0, 1, 1, 0, 0, 1, 1], [0, 0, 0, 1, 1, 1, 1]])
    r, c = np.nonzero(H)
    return 3, 7, r.tolist(), c.tolist()


def degenerate_edges():
    """Column 2 all zero, columns 4 and 7 identical, row 4 a copy of row 1."""
    H = np.array([[1, 1, 0, 0, 1, 0, 0, 1, 0],
                  [0, 1, 0, 1, 0, 1, 0, 0, 1],
                  [1, 0, 0, 1, 1, 0, 1, 1, 0],
                  [0, 0, 0, 0, 1, 1, 1, 1, 1],
                  [0, 1, 0, 1, 0, 1, 0, 0, 1]])
    r, c = np.nonzero(H)
    return H.shape[0], H.shape[1], r.tolist(), c.tolist()


def tall_edges():
    """M = 8200 rows, more than the 8192 whose row parities the dense kernel
    keeps in LDS (it then reads them from global memory): 150 random rows,
    repeated, so the rank stays small and the construction quick."""
    _, N, rows, cols = random_edges(5, 150, 260, deg=(3, 7))
    rows, cols = np.array(rows), np.array(cols)
    M = 8200
    R, Cc = [], []
    for i0 in range(0, M, 150):
        keep = rows + i0 < M
        R.append(rows[keep] + i0)
        Cc.append(cols[keep])
    return M, N, np.concatenate(R).tolist(), np.concatenate(Cc).tolist()


RANDOM_SHAPES = {"r37x100": (11, 37, 100), "r65x129": (12, 65, 129), "r64x70": (13, 64, 70)}


def small_graph(L, name):
    """A Graph of the shared cases, by name."""
    if name == "rs_5_16_4":
        return L.Graph.rs_ldpc(5, 16, 4)
    if name == "rs_4_8_3":
        return L.Graph.rs_ldpc(4, 8, 3)
    if name in RANDOM_SHAPES:
        return L.Graph.from_edges(*random_edges(*RANDOM_SHAPES[name]))
    return L.Graph.from_edges(*{"hamming": hamming_edges, "degenerate": degenerate_edges, "tall": tall_edges}[name]())


SMALL_CODES = ["rs_5_16_4", "rs_4_8_3", "hamming", "r37x100", "r65x129", "r64x70", "degenerate"]
