"""The error-rate simulation's host forms under AddressSanitizer + UBSan: a
stand-alone host program (tests/channel_sim_san/chan_check.cpp:
csrc/channel_sim.hpp and csrc/error_rate.hpp only, its own main, no HIP)
compiled with g++ into pytest's tmp_path and run directly: the corner tables
(all thresholds 0, all 2^53, a single step), N = 1 and N off the word size,
split ranges, the last frames the key holds, the error counter, the loop for
every stop rule and batch size, and the argument errors, every buffer on the
heap at exactly its size."""
import os
import re
import subprocess

from conftest import ROOT


def test_channel_sim_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "chan_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                           "-static-libasan", "-static-libubsan",  # the runtimes inside the program itself
                           "-o", exe, os.path.join(ROOT, "tests", "channel_sim_san", "chan_check.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert re.fullmatch(r"chan_check ok: \d+ cases", r.stdout.strip())
