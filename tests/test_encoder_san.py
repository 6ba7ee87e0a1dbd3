"""The host encoder under AddressSanitizer + UBSan: a stand-alone host
program (tests/encoder_san/enc_check.cpp: csrc/gf2.hpp + csrc/graph.cpp, its
own main, no HIP) compiled with g++ into pytest's tmp_path and run directly
on the small codes of the encoder tests and the DNA code."""
import os
import subprocess

import gf2_ref
from conftest import PCHK, ROOT


def test_host_encoder_under_asan_ubsan(L, tmp_path):
    exe = str(tmp_path / "enc_check")
    csrc = os.path.join(ROOT, "dna-ldpc-codes_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-static-libasan", "-static-libubsan",  # the runtimes inside the program itself
                           "-o", exe,
                           os.path.join(ROOT, "tests", "encoder_san", "enc_check.cpp"), os.path.join(csrc, "graph.cpp"),
                           "-lpthread"])
    paths = []
    for name in gf2_ref.SMALL_CODES + ["tall"]:
        p = str(tmp_path / (name + ".pchk"))
        gf2_ref.small_graph(L, name).save_pchk(p)
        paths.append(p)
    full = str(tmp_path / "identity.pchk")  # full column rank: K = 0
    L.Graph.from_edges(3, 3, [0, 1, 2], [0, 1, 2]).save_pchk(full)
    r = subprocess.run([exe] + paths + [full, PCHK], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == len(paths) + 2 and all(ln.endswith(" ok") for ln in lines[:-2] + lines[-1:])
    assert lines[-2].endswith("K 0 unsupported")
    assert "rank 1860 K 16572 ok" in lines[-1]
