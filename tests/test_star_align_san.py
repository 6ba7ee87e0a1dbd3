"""The centre-star aligner's host code under AddressSanitizer + UBSan: a
stand-alone host program (tests/star_align_san/star_check.cpp:
csrc/star_align.hpp only, its own main, no HIP) compiled with g++ into
pytest's tmp_path and run directly on empty reads, k = 1, the exhaustive
single edits of a 10-nt parent in both orders, ties and two long reads, every
read and every output in a heap buffer of exactly its size."""
import os
import subprocess

from conftest import ROOT


def test_star_align_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "star_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-static-libasan", "-static-libubsan",  # the runtimes inside the program itself
                           "-o", exe, os.path.join(ROOT, "tests", "star_align_san", "star_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "star_check ok: 168 single-edit pairs"
