"""TEST INFRASTRUCTURE: the read groups shared by the star-alignment tests
(test_star_align.py on the CPU, test_star_align_gpu.py on the GPU)."""
from functools import lru_cache

import numpy as np


def mutate(rng, parent, alphabet, n_ops):
    s = list(parent)
    for _ in range(n_ops):
        op = int(rng.integers(0, 3))
        if op == 0 and s:
            s[int(rng.integers(0, len(s)))] = alphabet[int(rng.integers(0, len(alphabet)))]
        elif op == 1:
            s.insert(int(rng.integers(0, len(s) + 1)), alphabet[int(rng.integers(0, len(alphabet)))])
        elif s:
            del s[int(rng.integers(0, len(s)))]
    return "".join(s)


@lru_cache(maxsize=None)
def random_groups(seed=17, n_short=160, n_long=48):
    """k = 1..8 reads per group, derived from one parent by random
    substitutions, insertions and deletions, plus some unrelated reads:
    lengths 0..12 over the alphabet AC (many ties), 130..142 over ACGT."""
    rng = np.random.default_rng(seed)
    groups = []
    for t in range(n_short + n_long):
        short = t < n_short
        alphabet = "AC" if short else "ACGT"
        lo, hi = (0, 12) if short else (130, 142)
        parent = "".join(rng.choice(list(alphabet), int(rng.integers(lo, hi + 1))))
        k = 1 + t % 8
        g = []
        for _ in range(k):
            if rng.random() < 0.15:  # an unrelated read
                g.append("".join(rng.choice(list(alphabet), int(rng.integers(lo, hi + 1)))))
            else:
                g.append(mutate(rng, parent, alphabet, int(rng.integers(0, 5 if short else 9)))[:hi])
        groups.append(tuple(g))
    return tuple(groups)


def exhaustive_groups(parent="ACGTTGCAAC"):
    """Every single substitution, insertion and deletion of the parent,
    paired with the parent in both orders."""
    variants = set()
    for p in range(len(parent)):
        variants.add(parent[:p] + parent[p + 1:])
        for c in "ACGT":
            if c != parent[p]:
                variants.add(parent[:p] + c + parent[p + 1:])
    for p in range(len(parent) + 1):
        for c in "ACGT":
            variants.add(parent[:p] + c + parent[p:])
    variants.discard(parent)
    out = []
    for v in sorted(variants):
        out += [(parent, v), (v, parent)]
    return out


def edge_groups():
    rng = np.random.default_rng(5)
    long_read = "".join(rng.choice(list("ACGT"), 1000))
    near = long_read[:400] + long_read[401:700] + "G" + long_read[700:]
    return [
        ("",), ("", ""), ("", "ACGT"), ("ACGT", ""), ("", "", "A"),           # empty reads
        ("ACGTACGT",) * 4,                                                      # all identical
        ("GGGG", "AC", "CA"), ("AC", "CA", "AA", "CC"), ("AT", "TA"),           # centre ties, broken by index
        ("ACNNGT", "AC-GT", "acgt", "AC\xe9GT", "AC\x00GT"),                    # non-ACGT bytes
        (near, long_read, long_read[:990]),                                     # reads of about 1000 nt
    ]
