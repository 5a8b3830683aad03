"""The stopping rule of the s-step GMRES (feddlib_amd/csrc/gmres_stop_rule.hpp) is host arithmetic alone: tests/stop_rule_main.cpp
feeds it scripted event sequences (each of the five claim branches, keep-if-better in both directions, breakdown, a used-up
cycle on both sides of the 0.999 threshold, three stalls, the halving of the block length, the block length a tolerance
allows) and compares every answer and the final its / relres / floor / rec_relres with a table written from the rule as the
solver's documentation states it.  Built with the address and undefined-behaviour sanitizers, run as a child process; no GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stop_rule_table(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "stop_rule")
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(ROOT, "feddlib_amd", "csrc"), os.path.join(ROOT, "tests", "stop_rule_main.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "\n0 mismatches\n" in r.stdout
