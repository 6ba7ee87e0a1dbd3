"""The speculating trial loop's host code under AddressSanitizer + UBSan: a
stand-alone host program (tests/dna_trial_spec_san/spec_check.cpp:
csrc/dna_trial.hpp only, its own main, no HIP) compiled with g++ into pytest's
tmp_path and run directly with a stub decoder: K = 0, 1, 42, 127, 128, lists of
1, 5, 64 and 65 rows, steps -1, 2 and 64, faithful both ways, every buffer on the
heap at exactly its size (the packed batch of 64 * ceil(F / 64) rows included)."""
import os
import re
import subprocess

from conftest import ROOT


def test_dna_trial_spec_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "spec_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-D_GLIBCXX_SANITIZE_VECTOR",  # a vector's spare capacity is poisoned too
                           "-static-libasan", "-static-libubsan",  # the runtimes inside the program itself
                           "-o", exe, os.path.join(ROOT, "tests", "dna_trial_spec_san", "spec_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.fullmatch(r"spec_check ok: \d+ cases", r.stdout.strip())
