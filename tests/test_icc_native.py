"""The ICC planner of upload jobs (csrc/icc_parse.hpp) under AddressSanitizer + UBSan on the CPU (tests/native/icc_fuzz.cpp, a
stand-alone program): valid profiles of every curve form and a JPEG head with a profile in three APP2 chunks, every truncation and
every single-byte mutation (all 255 other values of every byte) of each -- a clean sanitizer run, and a valid kind or a refusal with a reason every time."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "icc_fuzz.cpp")


def test_icc_planner_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "icc_fuzz")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-fsanitize=address,undefined", SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    log = r.stdout[-2000:] + r.stderr[-4000:]
    assert r.returncode == 0 and not r.stderr and "runtime error" not in log and "AddressSanitizer" not in log, log
    assert "icc_fuzz ok" in r.stdout
    print(r.stdout)
