"""Regenerate tests/golden/index_fixtures.npz from a DATA file of the reference
(read as text; nothing from the reference is imported or executed).

* strand_parity    -- [18432][4] uint8: symbols 4..7 of the 16-nt prefix of
                      every line of original files/final_DNA.txt (two nt per
                      4-bit symbol, A/C/G/T = 0..3, most significant first):
                      the RS(8,4) parity of the strand index in symbols 0..3
                      (dna_fixtures.npz strand_index).  Pins the code's
                      conventions and dna_llr.encode_indices.
* final_dna_sha256 -- sha256 of the 18432 full lines joined by "\\n".  Pins
                      synth.dna_strands (prefix + payload).

    python tests/golden/make_index_fixtures.py <reference checkout>
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "index_fixtures.npz")


def main():
    if len(sys.argv) != 2 or not os.path.isdir(sys.argv[1]):
        sys.exit("usage: make_index_fixtures.py <reference checkout>")
    strands = open(os.path.join(sys.argv[1], "original files", "final_DNA.txt")).read().split()
    assert len(strands) == 18432 and all(len(s) == 152 for s in strands)
    nt = np.array([["ACGT".index(c) for c in s[8:16]] for s in strands], np.uint8)
    parity = (4 * nt[:, 0::2] + nt[:, 1::2]).astype(np.uint8)
    sha = hashlib.sha256("\n".join(strands).encode()).hexdigest()
    np.savez_compressed(OUT, strand_parity=parity, final_dna_sha256=np.array(sha))
    print(f"wrote {OUT}: {len(parity)} parity words, sha256 {sha[:16]}...")


if __name__ == "__main__":
    main()
