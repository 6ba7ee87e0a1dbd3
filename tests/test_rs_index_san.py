"""The strand-index codec under AddressSanitizer + UBSan: a stand-alone host
program (tests/rs_index_san/rs_check.cpp: csrc/rs_index.hpp only, its own
main, no HIP) compiled with g++ into pytest's tmp_path and run directly on
all codewords, the exhaustive single / double error sets of three codewords
and the edge-case reads."""
import os
import subprocess

from conftest import ROOT


def test_rs_index_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "rs_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-static-libasan", "-static-libubsan",  # the runtimes inside the program itself
                           "-o", exe, os.path.join(ROOT, "tests", "rs_index_san", "rs_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "rs_check ok: 65536 codewords, 360 single and 18900 double errors"
