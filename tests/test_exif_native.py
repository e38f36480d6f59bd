"""The EXIF orientation reader of csrc/jpeg_parse.hpp under AddressSanitizer + UBSan on the CPU (tests/native/exif_fuzz.cpp, a
stand-alone program): II and MM blocks, every case that must read as orientation 1, and every truncation and single-byte mutation
of a valid APP1 block -- a clean sanitizer run and an orientation in 1..8 every time."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "exif_fuzz.cpp")


def test_exif_reader_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "exif_fuzz")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-fsanitize=address,undefined", SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    log = r.stdout[-2000:] + r.stderr[-4000:]
    assert r.returncode == 0 and not r.stderr and "runtime error" not in log and "AddressSanitizer" not in log, log
    assert "exif_fuzz ok" in r.stdout
