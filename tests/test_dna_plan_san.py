"""The read planner's host code under AddressSanitizer + UBSan: a stand-alone
host program (tests/dna_plan_san/plan_check.cpp: csrc/dna_plan.hpp only, its
own main, no HIP) compiled with g++ into pytest's tmp_path and run directly on
the planner's edge cases, raw reads, the argument errors and one dense case,
every input and every output in a heap buffer of exactly its size."""
import os
import re
import subprocess

from conftest import ROOT


def test_dna_plan_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "plan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-static-libasan", "-static-libubsan",  # the runtimes inside the program itself
                           "-o", exe, os.path.join(ROOT, "tests", "dna_plan_san", "plan_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.fullmatch(r"plan_check ok: \d+ cases", r.stdout.strip())
