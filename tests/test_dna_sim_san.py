"""The sequencing channel's host form under AddressSanitizer + UBSan: a
stand-alone host program (tests/dna_sim_san/sim_check.cpp: csrc/dna_sim.hpp
only, its own main, no HIP) compiled with g++ into pytest's tmp_path and run
directly: the corner rates on every shape (nothing happens, every base
substituted, every slot inserts -- the longest read --, every base deleted),
prefix and split ranges, the last reads the key holds, and the argument errors,
every buffer on the heap at exactly its size."""
import os
import re
import subprocess

from conftest import ROOT


def test_dna_sim_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "sim_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-static-libasan", "-static-libubsan",  # the runtimes inside the program itself
                           "-o", exe, os.path.join(ROOT, "tests", "dna_sim_san", "sim_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.fullmatch(r"sim_check ok: \d+ cases", r.stdout.strip())
