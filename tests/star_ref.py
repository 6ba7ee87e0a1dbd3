"""TEST INFRASTRUCTURE: an independent reference of the centre-star alignment
(DESIGN.md sec. 8.6), written from the definition in numpy / Python.  It keeps
the full Levenshtein table of every pair and walks its own traceback over the
table's values; it shares no code with the product (csrc/star_align.hpp, the
kernels of dna.hip).

Reads are byte strings; the `str` forms encode as latin-1, as dna_llr does.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np

GAP = ord("-")


def _bytes(s) -> bytes:
    return s if isinstance(s, (bytes, bytearray)) else s.encode("latin-1", "replace")


def table(r: bytes, c: bytes) -> np.ndarray:
    """D[i][j] = Levenshtein distance of r[:i] and c[:j], int64 [m+1][n+1].
    Row i from row i-1: x[j] = min(D[i-1][j-1] + (r[i-1] != c[j-1]),
    D[i-1][j] + 1), then D[i][j] = min over k <= j of x[k] + (j - k) with
    x[0] = i (the run of left moves), a running minimum of x[k] - k."""
    m, n = len(r), len(c)
    cv = np.frombuffer(bytes(c), np.uint8)
    D = np.zeros((m + 1, n + 1), np.int64)
    D[0] = np.arange(n + 1)
    ar = np.arange(n + 1)
    for i in range(1, m + 1):
        x = np.empty(n + 1, np.int64)
        x[0] = i
        x[1:] = np.minimum(D[i - 1, :-1] + (cv != r[i - 1]), D[i - 1, 1:] + 1)
        D[i] = np.minimum.accumulate(x - ar) + ar
    return D


def distance(a, b) -> int:
    return int(table(_bytes(a), _bytes(b))[-1, -1])


def pairwise(r: bytes, c: bytes):
    """(at, slots, distance): at[j] = the byte of r on centre position j or
    None, slots[j] = the bytes of r inserted in the gap before position j
    (slot n after the last), in read order."""
    m, n = len(r), len(c)
    D = table(r, c)
    at = [None] * n
    slots = [[] for _ in range(n + 1)]
    i, j = m, n
    while i > 0 or j > 0:
        if i > 0 and j > 0 and D[i, j] == D[i - 1, j - 1] + (r[i - 1] != c[j - 1]):
            at[j - 1] = r[i - 1]
            i, j = i - 1, j - 1
        elif i > 0 and D[i, j] == D[i - 1, j] + 1:
            slots[j].insert(0, r[i - 1])
            i -= 1
        else:
            j -= 1
    return at, slots, int(D[m, n])


def star(seqs: Sequence) -> Tuple[int, int, List[bytes], List[int]]:
    """(centre, width, rows in candidate order, distance of each read to the centre)."""
    bs = [_bytes(s) for s in seqs]
    k = len(bs)
    if k == 1:
        return 0, len(bs[0]), [bytes(bs[0])], [0]
    d = np.zeros((k, k), np.int64)
    for a in range(k):
        for b in range(a + 1, k):
            d[a, b] = d[b, a] = table(bs[a], bs[b])[-1, -1]
    centre = int(np.argmin(d.sum(axis=1)))  # the first minimum: ties to the lowest index
    c = bs[centre]
    n = len(c)
    scripts = []
    for a in range(k):
        if a == centre:
            scripts.append((list(c), [[] for _ in range(n + 1)], 0))
        else:
            scripts.append(pairwise(bs[a], c))
    w = [max(len(s[1][j]) for s in scripts) for j in range(n + 1)]
    rows = []
    for at, slots, _ in scripts:
        row = bytearray()
        for j in range(n + 1):
            row += bytes(slots[j]) + b"-" * (w[j] - len(slots[j]))
            if j < n:
                row.append(GAP if at[j] is None else at[j])
        rows.append(bytes(row))
    return centre, n + sum(w), rows, [s[2] for s in scripts]


def star_align(seqs: Sequence[str]) -> List[Tuple[int, str]]:
    """The AlignFn form: [(order, row)] in candidate order."""
    _, _, rows, _ = star(seqs)
    return [(a, row.decode("latin-1")) for a, row in enumerate(rows)]
