"""Plain references for the decoders, written from the definitions of the
algorithms -- test infrastructure, independent of oracle/ldpc_oracle.c.

Floating point (sum_product, min_sum): flooding message passing in the LLR
domain on a dense boolean H, in a numpy dtype of the caller's choice
(np.longdouble for checking, np.float64 to measure what an honest fp64
evaluation of the same inputs can be off by).  Only the loop control
(syndrome first, stop at n == max_iter or c == 0, dec.cpp:583-605 and
1216-1250) and the decision rules (dec.cpp:626, 681, 1311-1312, 1675-1676) are
taken from the reference program; the message rules are the textbook ones:

  check    c2v[i][j] = 2 atanh( prod_{j' in row i, j' != j} tanh(v2c[i][j'] / 2) )    (sum-product)
           c2v[i][j] = prod sign(v2c[i][j']) * min |v2c[i][j']|  over j' != j         (min-sum)
  variable v2c[i][j] = prior[j] + sum_{i' in column j, i' != i} c2v[i'][j]
  decision L[j]      = prior[j] + sum_{i' in column j} c2v[i'][j],  bit = 1 when L <= 0

Every "other edges" product, minimum and sum is an explicit loop over an
index list with the own edge deleted: no total divided by the own term, no
prefix / suffix products.

Integer (int_decode): the quantised min-sum and Gallager A / B1 / B2 of
dec.cpp:699-832, 1174-1764 in Python ints with the same O(d^2) loops, for
in-range input (no int wrap-around: the caller keeps |LLR| / step far below
2^31).  The tie bit that stands in for rand_int(2) is the project's own
definition (oracle/ldpc_oracle.c tie_bit) and is taken over as such.
"""
from collections import namedtuple

import numpy as np

Result = namedtuple("Result", "hard post iters valid max_msg min_post")


def dense_h(M, N, rows, cols):
    """Boolean M x N parity-check matrix; a repeated entry counts once
    (mod2sparse_insert finds the existing entry, mod2sparse.cpp:521-524)."""
    H = np.zeros((M, N), bool)
    H[np.asarray(rows, int), np.asarray(cols, int)] = True
    return H


def _lists(H):
    M, N = H.shape
    return [np.flatnonzero(H[i]) for i in range(M)], [np.flatnonzero(H[:, j]) for j in range(N)]


def _syndrome(H, bits):
    return int(((H.astype(np.int64) @ bits.astype(np.int64)) & 1).sum())


def _decode_float(H, llr, max_iter, dtype, check_rule, own_edge):
    """One codeword.  own_edge=True is the deliberately wrong rule of the
    negative control: every extrinsic loop also takes the own edge."""
    M, N = H.shape
    row_cols, col_rows = _lists(H)
    prior = np.asarray(llr, dtype=dtype)
    v2c = np.zeros((M, N), dtype)
    c2v = np.zeros((M, N), dtype)
    for j in range(N):
        v2c[col_rows[j], j] = prior[j]
    post = prior.copy()
    # first guess: BP takes LR < 1 (dec.cpp:626), min-sum "0 when LLR > 0, else 1" (dec.cpp:1311-1312)
    bits = (prior < 0).astype(np.uint8) if check_rule is _tanh_rule else (~(prior > 0)).astype(np.uint8)
    max_msg = float(np.max(np.abs(prior))) if N else 0.0
    min_post = float(np.min(np.abs(prior))) if N else np.inf
    n = 0
    while True:
        c = _syndrome(H, bits)
        if n == max_iter or c == 0:
            break
        for i in range(M):
            cols = row_cols[i]
            x = np.tanh(v2c[i, cols] / dtype(2)) if check_rule is _tanh_rule else v2c[i, cols]
            for k, j in enumerate(cols):
                others = x if own_edge else np.delete(x, k)
                c2v[i, j] = check_rule(others, dtype)
        for j in range(N):
            rows = col_rows[j]
            y = c2v[rows, j]
            for k, i in enumerate(rows):
                others = y if own_edge else np.delete(y, k)
                v2c[i, j] = prior[j] + others.sum(dtype=dtype)
            post[j] = prior[j] + y.sum(dtype=dtype)
        bits = (~(post > 0)).astype(np.uint8)
        msgs = np.abs(np.concatenate([v2c[H], c2v[H]]))
        max_msg = max(max_msg, float(np.max(msgs[np.isfinite(msgs)], initial=0)))
        min_post = min(min_post, float(np.min(np.abs(post))))
        n += 1
    return Result(bits, post, n, c == 0, max_msg, min_post)


def _tanh_rule(others, dtype):
    """others: tanh(v / 2) of the other edges."""
    p = dtype(1)
    for t in others:
        p = p * t
    with np.errstate(divide="ignore"):  # the empty product of a degree-1 check: atanh(1) = inf
        return dtype(2) * np.arctanh(p)


def _min_rule(others, dtype):
    if len(others) == 0:
        return dtype(0)  # a degree-1 row sends 0 (mag_min stays -1 and is clamped, dec.cpp:1427-1428)
    sign = dtype(1)
    for s in others:
        if not s >= 0:
            sign = -sign
    return sign * np.min(np.abs(others))


def _batch(H, llr, max_iter, dtype, rule, own_edge):
    llr = np.atleast_2d(llr)
    res = [_decode_float(H, x, max_iter, dtype, rule, own_edge) for x in llr]
    return Result(np.array([r.hard for r in res], np.uint8), np.array([r.post for r in res], dtype),
                  np.array([r.iters for r in res], np.int32), np.array([r.valid for r in res], bool),
                  max((r.max_msg for r in res), default=0.0), min((r.min_post for r in res), default=np.inf))


def sum_product(H, llr, max_iter, dtype=np.longdouble, own_edge=False):
    """Flooding sum-product on LLRs [B][N]: Result(hard[B][N] u8, post[B][N]
    (the posterior LLR at exit; the prior at 0 iterations), iters[B],
    valid[B], largest finite |message| (priors, v2c and c2v of every
    iteration), smallest |posterior| (priors and every iteration's
    posterior)).  A check of degree 1 states its bit with certainty: the empty
    product is 1 and its message atanh(1) = +inf, exactly, in every iteration;
    such messages (and the v2c and posterior of that column) are the only
    infinite ones and stay out of the largest-message figure."""
    return _batch(H, llr, max_iter, dtype, _tanh_rule, own_edge)


def min_sum(H, llr, max_iter, dtype=np.longdouble, own_edge=False):
    """Float min-sum (decoder_type 20); same outputs as sum_product."""
    return _batch(H, llr, max_iter, dtype, _min_rule, own_edge)


# ---------------------------------------------------------------------------
# integer decoders, dec.cpp:699-832, 1174-1764
# ---------------------------------------------------------------------------
QMSA, GALLAGER_A, GALLAGER_B1, GALLAGER_B2 = 2, 3, 4, 5
_M64 = (1 << 64) - 1


def _smix(x):
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def tie_bit(seed, b, stage, j):
    """The project's stand-in for rand_int(2) (dec.cpp:1273, 1647): stage 0 is
    Init_MSA, stage n + 1 the decision of iteration n; b the codeword's index
    in the call."""
    x = _smix(seed & _M64)
    x = _smix(x ^ (b & _M64))
    x = _smix(x ^ (((stage & 0xFFFFFFFF) << 32) | (j & 0xFFFFFFFF)))
    return x & 1


def cal_msa_q(x, step, max_value, min_value):
    """Cal_MSA_Q(x, 0), dec.cpp:1708-1743, for |x| / step + 0.5 < 2^31."""
    sign = 1 if x >= 0 else -1
    k = int(abs(float(x)) / step + 0.5)  # (int) truncates
    if sign == 1:
        if k > max_value:
            k = max_value
    else:
        if k > -min_value:
            k = -min_value
        k *= sign
    return k


def int_decode(H, llr, max_iter, algo, precision=6, step=0.5, beta=0, seed=0):
    """Batch [B][N] through Run_MSA_Decoder (algo 2) or Run_Gallager_Decoder
    (3 / 4 / 5 = type 0 / 1 / 2).  Returns (hard u8, post f64 (L_Q, or the
    Gallager decision value; the quantised prior at 0 iterations, as the
    project defines it), iters, valid)."""
    M, N = H.shape
    row_cols, col_rows = _lists(H)
    row_cols = [[int(j) for j in r] for r in row_cols]
    col_rows = [[int(i) for i in c] for c in col_rows]
    D_v = max((len(c) for c in col_rows), default=-1)  # CheckRegular dec.cpp:138-169: the largest column degree
    max_value = int(2.0 ** (precision - 1) - 1)  # Set_MSA dec.cpp:1690-1691
    min_value = -max_value
    if algo == GALLAGER_A:
        b_var, b_dec = D_v - 1, D_v  # dec.cpp:777, 811
    elif algo == GALLAGER_B1:
        b_var, b_dec = D_v - 2, D_v - 1
    else:
        b_var, b_dec = D_v // 2 + D_v % 2, D_v // 2 + 1
    llr = np.atleast_2d(np.asarray(llr, np.float64))
    B = llr.shape[0]
    hard = np.zeros((B, N), np.uint8)
    post = np.zeros((B, N), np.float64)
    iters = np.zeros(B, np.int32)
    valid = np.zeros(B, bool)
    for b in range(B):
        v2c = [dict() for _ in range(M)]  # v2c[i][j]
        c2v = [dict() for _ in range(M)]
        dec = [0] * N
        prior = [0] * N
        for j in range(N):
            if algo == QMSA:  # Init_MSA dec.cpp:1256-1277
                m = cal_msa_q(llr[b, j], step, max_value, min_value)
                dec[j] = 0 if m > 0 else 1 if m < 0 else tie_bit(seed, b, 0, j)
            else:  # hard-decision input +-1; Init_Gallager dec.cpp:725-739
                m = -1 if llr[b, j] < 0 else 1
                dec[j] = 0 if m >= 0 else 1
            prior[j] = m
            post[b, j] = m
            for i in col_rows[j]:
                v2c[i][j] = m
        n = 0
        while True:
            c = sum(sum(dec[j] for j in row_cols[i]) & 1 for i in range(M))
            if n == max_iter or c == 0:
                break
            for i in range(M):
                for j in row_cols[i]:
                    if algo == QMSA:  # Check_Update_MSA dec.cpp:1357-1393
                        mag_min, sign = -1, 1
                        for jj in row_cols[i]:
                            if jj != j:
                                x = v2c[i][jj]
                                if mag_min == -1 or mag_min > abs(x):
                                    mag_min = abs(x)
                                sign *= 1 if x >= 0 else -1
                        mag_min -= beta
                        if mag_min < 0:
                            mag_min = 0
                        c2v[i][j] = sign * mag_min
                    else:  # Check_Update_Gallager dec.cpp:748-769
                        temp = 1
                        for jj in row_cols[i]:
                            if jj != j:
                                temp *= v2c[i][jj]
                        c2v[i][j] = temp
            for j in range(N):
                if algo == QMSA:  # Variable_Update_MSA dec.cpp:1465-1482, Cal_MSA_Clip :1748-1764
                    for i in col_rows[j]:
                        s = prior[j]
                        for ii in col_rows[j]:
                            if ii != i:
                                s += c2v[ii][j]
                        v2c[i][j] = max_value if s > max_value else min_value if s < min_value else s
                else:  # Variable_Update_Gallager dec.cpp:771-802
                    message = -prior[j]
                    for i in col_rows[j]:
                        num = 0
                        for ii in col_rows[j]:
                            if ii != i and c2v[ii][j] == message:
                                num += 1
                        v2c[i][j] = message if num >= b_var else prior[j]
            for j in range(N):
                if algo == QMSA:  # Decision_MSA dec.cpp:1624-1654
                    s = prior[j]
                    for i in col_rows[j]:
                        s += c2v[i][j]
                    post[b, j] = s
                    dec[j] = 0 if s > 0 else 1 if s < 0 else tie_bit(seed, b, n + 1, j)
                else:  # Decision_Gallager dec.cpp:804-832
                    message = -prior[j]
                    num = sum(1 for i in col_rows[j] if c2v[i][j] == message)
                    temp = message if num >= b_dec else prior[j]
                    post[b, j] = temp
                    dec[j] = 0 if temp >= 0 else 1
            n += 1
        hard[b] = dec
        iters[b] = n
        valid[b] = c == 0
    return hard, post, iters, valid
