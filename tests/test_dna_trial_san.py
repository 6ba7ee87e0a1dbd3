"""The trial loop's host code under AddressSanitizer + UBSan: a stand-alone
host program (tests/dna_trial_san/trial_check.cpp: csrc/dna_trial.hpp only, its
own main, no HIP) compiled with g++ into pytest's tmp_path and run directly
with a stub decoder: B = 1, no failures, rows failing until eps2 runs out (the
iteration count against the eps2 sequence), faithful both ways, genie-less, the
erasure index and the argument errors, every buffer on the heap at exactly its
size."""
import os
import re
import subprocess

from conftest import ROOT


def test_dna_trial_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "trial_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-static-libasan", "-static-libubsan",  # the runtimes inside the program itself
                           "-o", exe, os.path.join(ROOT, "tests", "dna_trial_san", "trial_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.fullmatch(r"trial_check ok: \d+ cases", r.stdout.strip())
