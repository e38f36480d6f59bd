"""The window-parallel decode of long streams on the CPU (tests/native/jpeg_dec_win_sim.cpp: the three passes of csrc/jpeg_dec.hip's
spec, chain and write kernels with windows and lanes as loops, over csrc/jpeg_dec_core.hpp's own code), built plain and under
ASan + UBSan: its coefficients equal the model's with honest and with deliberately wrong guesses, every window of the test files
synchronises, the window arithmetic holds at the window's byte boundaries, a stream whose last subsequence is exactly full decodes,
and corrupt multi-window files end in a non-zero status with no sanitizer report.  With "--poison BYTE" (tests/native/sim_poison.hpp:
the lane records and window heads, which nothing on the device clears, the staged words and the lanes' state start as that byte) every
line, and the coefficients of every file with status 0, equal the plain run's."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_decode_cases as cases      # noqa: E402
import jpeg_decode_model as model      # noqa: E402
import jpeg_decode_window_cases as wcases      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "jpeg_dec_win_sim.cpp")


def _build(tmp, name, flags):
    exe = str(tmp / name)
    r = subprocess.run(["g++", "-std=c++17", "-g", "-fno-omit-frame-pointer", "-Wall"] + flags + [SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-3000:]
    return exe


def _run(exe, *args):
    r = subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=600)
    log = r.stdout[-2000:] + r.stderr[-4000:]
    assert r.returncode == 0 and not r.stderr and "runtime error" not in log and "AddressSanitizer" not in log, log
    return r.stdout.splitlines()


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("jpeg_dec_win_sim")
    return tmp, _build(tmp, "sim", ["-O2"]), _build(tmp, "sim_san", ["-O1", "-fsanitize=address,undefined"])


def _consts(exe):
    f = _run(exe, "consts")[0].split()
    return dict(zip(f[0::2], (int(v) for v in f[1::2])))


def _dump(tmp, exe, data, poison=False, dirty=None):
    """-> (head fields, status, chain re-decodes per window, coefficients int16 flat); poison: wrong guesses; dirty: --poison BYTE"""
    src, out = str(tmp / "in.jpg"), str(tmp / "out.bin")
    with open(src, "wb") as f:
        f.write(data)
    lines = _run(exe, *(() if dirty is None else ("--poison", str(dirty))), "dump", src, out, *(["poison"] if poison else []))
    assert lines[0].startswith("ok "), lines[0]
    f = lines[1].split()
    again = [] if f[5] == "-" else [int(v) for v in f[5].split(",")]
    assert f[0] == "status" and f[2] == "windows" and int(f[3]) == len(again)
    return [int(v) for v in lines[0].split()[1:]], int(f[1]), again, np.fromfile(out, np.int16)


def _model_coefficients(data):
    p = model.plan(data)
    return p, np.concatenate([g.reshape(-1) for g in model.coefficients(p)])


def _compare(tmp, exe, files, poison):
    for name, data in files.items():
        p, want = _model_coefficients(data)
        head, status, _, got = _dump(tmp, exe, data, poison)
        assert head[:3] == [p.h, p.w, p.sampling], name
        assert status == 0, (name, status)
        assert got.size == want.size and np.array_equal(got.astype(np.int64), want), (name, poison)


@pytest.mark.parametrize("poison", [False, True])
def test_coefficients_equal_the_model_on_the_grid_and_the_encoder_cases(exes, poison):
    tmp, exe, exe_san = exes
    grid = cases.grid_cases()
    _compare(tmp, exe, grid, poison)
    _compare(tmp, exe, cases.encoder_cases(), poison)
    _compare(tmp, exe_san, {k: v for k, v in grid.items() if k.startswith(("33x47", "grey_17x13", "5x3"))}, poison)


@pytest.mark.parametrize("poison", [False, True])
def test_multi_window_files_equal_the_model_and_every_window_synchronises(exes, poison):
    """the files of the GPU test: with honest guesses and with every guess wrong the coefficients are the model's, and the chain pass
    decodes fewer than a window's lanes again in every window (a window that never locked would show `lanes`)"""
    tmp, exe, exe_san = exes
    c = _consts(exe)
    assert c["window_bits"] == c["lanes"] * c["subseq_bits"]
    for name, (data, windows) in wcases.multi_window_files().items():
        p, want = _model_coefficients(data)
        assert len(p.streams) == 1 and -(-8 * len(p.streams[0][0]) // c["window_bits"]) == windows, name
        for e in (exe, exe_san):
            head, status, again, got = _dump(tmp, e, data, poison)
            print(name, "poison" if poison else "honest", "chain re-decodes per window", again)
            assert status == 0 and len(again) == windows and again[0] == 0, (name, again)
            assert all(a < c["lanes"] for a in again), (name, again)
            assert np.array_equal(got.astype(np.int64), want), (name, poison)


@pytest.mark.parametrize("byte", [0x00, 0xFF, 0x5A])
def test_nothing_depends_on_what_lds_and_scratch_held(exes, byte):
    """the grid's sanitizer subset, the encoder's files, the multi-window files (honest and wrong guesses), the full-last-subsequence file
    and the 200 corruptions of the two-window file, under the sanitizers with dirty records, heads, LDS and lane state, against the plain
    program's unpoisoned run"""
    tmp, exe, exe_san = exes
    c = _consts(exe)
    files = {k: v for k, v in cases.grid_cases().items() if k.startswith(("33x47", "grey_17x13", "5x3", "64x48", "40x88"))}
    files.update(cases.encoder_cases())
    files.update({k: v[0] for k, v in wcases.multi_window_files().items()})
    full, _ = wcases.full_last_subsequence_file(c["subseq_bits"] // 8, c["short_max_bytes"])
    files["full_last_subsequence"] = full
    for name, data in files.items():
        for guesses in (False, True):
            a, b = _dump(tmp, exe_san, data, guesses, dirty=byte), _dump(tmp, exe, data, guesses)
            assert a[:3] == b[:3], (name, guesses, a[:3], b[:3])
            if a[1] == 0:
                assert np.array_equal(a[3], b[3]), (name, guesses)
    _, variants = wcases.corrupted_two_window_files()
    pack = str(tmp / "pack_poison.bin")
    with open(pack, "wb") as f:
        for _, data in variants:
            f.write(struct.pack("<I", len(data)) + data)
    lines = _run(exe_san, "--poison", str(byte), "batch", pack)
    assert len(lines) == 200 and lines == _run(exe, "batch", pack)


def test_the_window_table_at_the_windows_byte_boundaries(exes):
    """stream lengths one byte short of, at and one byte past k windows: the window count, every window's first bit and lane count and
    the bit at which its last lane stops"""
    tmp, exe, _ = exes
    c = _consts(exe)
    wbits, s, lanes = c["window_bits"], c["subseq_bits"], c["lanes"]
    wbytes = wbits // 8
    assert wbytes == 32768
    for k in (1, 2, 3, 5):
        for length in (wbytes * k - 1, wbytes * k, wbytes * k + 1):
            lines = _run(exe, "table", str(length))
            bits = 8 * length
            n = -(-bits // wbits)
            assert n == (k if length <= wbytes * k else k + 1)
            assert lines[0] == "windows %d" % n and len(lines) == n + 1
            covered = 0
            for wi, line in enumerate(lines[1:]):
                win0, nl, last = (int(v) for v in line.split())
                assert win0 == wi * wbits == covered
                left = bits - win0
                assert nl == min(lanes, -(-left // s)) and nl >= 1
                assert last == min(bits, win0 + nl * s)
                covered = last
            assert covered == bits, length              # the windows' lanes tile the stream exactly


def test_a_stream_whose_last_subsequence_is_exactly_full(exes):
    tmp, exe, exe_san = exes
    c = _consts(exe)
    data, seed = wcases.full_last_subsequence_file(c["subseq_bits"] // 8, c["short_max_bytes"])
    assert data is not None, "no seed gives a scan of a whole number of subsequences"
    p, want = _model_coefficients(data)
    assert len(p.streams) == 1 and len(p.streams[0][0]) % (c["subseq_bits"] // 8) == 0 and len(p.streams[0][0]) > c["short_max_bytes"]
    print("seed %d: stream of %d bytes" % (seed, len(p.streams[0][0])))
    for poison in (False, True):
        for e in (exe, exe_san):
            head, status, again, got = _dump(tmp, e, data, poison)
            assert status == 0 and np.array_equal(got.astype(np.int64), want), (seed, poison)


def test_corruptions_of_a_two_window_file_under_the_sanitizers(exes):
    """200 seeded single-byte corruptions of the scan of a 2-window file: status 0 exactly where the model decodes the file too, no
    sanitizer report, at least 50 flagged"""
    tmp, _, exe_san = exes
    good, variants = wcases.corrupted_two_window_files()
    assert -(-8 * len(model.plan(good).streams[0][0]) // _consts(exe_san)["window_bits"]) == 2
    pack = str(tmp / "pack.bin")
    with open(pack, "wb") as f:
        for _, data in variants:
            f.write(struct.pack("<I", len(data)) + data)
    lines = _run(exe_san, "batch", pack)
    assert len(lines) == len(variants) == 200
    flagged = 0
    for (name, data), line in zip(variants, lines):
        if line.startswith("refused invalid: "):
            with pytest.raises(model.Refused):
                model.plan(data)
            continue
        status = int(line.split()[1])
        try:
            model.coefficients(model.plan(data))
            model_ok = True
        except (model.Corrupt, model.Refused):
            model_ok = False
        assert (status == 0) == model_ok, (name, line)
        flagged += status != 0
    print("%d of %d corruptions flagged by the decoder" % (flagged, len(variants)))
    assert flagged >= 50
