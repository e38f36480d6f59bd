"""csrc/jpeg_progenc_core.hpp -- the walk the count and emit kernels run, one lane per restart interval -- with the table builder and
the head pieces, compiled into a stand-alone program (tests/native/jpeg_progenc_sim.cpp) under the address and undefined-behaviour
sanitizers: its file of every coefficient case and of pixel images equals the model's, its event counts say the rules fired, and
jpeg_tables.hpp's bound equals the model's.  With "--poison BYTE" (tests/native/sim_poison.hpp: the correction words, the table
builder's work area, the codes and tables and every interval's buffer dirty; the histograms cleared as the launch code clears them)
every line of the same cases equals the plain run's."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_progenc_cases as cases      # noqa: E402
import jpeg_progenc_model as model      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _exe(tmp):
    exe = os.path.join(tmp, "jpeg_progenc_sim")
    src = os.path.join(ROOT, "tests", "native", "jpeg_progenc_sim.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fno-omit-frame-pointer", "-Wall", "-fsanitize=address,undefined", src, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-3000:]
    return exe


def _run(exe, text, *args):
    r = subprocess.run([exe] + list(args), input=text, capture_output=True, text=True, timeout=600)
    log = r.stdout[-2000:] + r.stderr[-4000:]
    assert r.returncode == 0 and not r.stderr and "runtime error" not in log and "AddressSanitizer" not in log, log
    return dict(line.split(": ", 1) for line in r.stdout.splitlines())


def _c_line(name, h, w, q, s, flat):
    return "C %s %d %d %d %d\n%s\n" % (name, h, w, q, s, " ".join(str(int(v)) for v in np.asarray(flat).ravel()))


HWS = [(1, 1), (5, 7), (17, 9), (45, 37), (72, 40), (1024, 1024), (8, 8192), (8192, 8), (8192, 8192)]


@functools.lru_cache(maxsize=None)
def _script():
    """the program's input for every case of this file, and what the model says of each"""
    text = "".join("F %d %d %d %d\n" % (h, w, q, s) for h, w in HWS for q in (1, 50, 85, 100) for s in (0, 2))
    want = {}
    for name in cases.NAMES:
        h, w, q, s, flat = cases.case(name)
        text += _c_line(name, h, w, q, s, flat)
        want[name] = cases.want(name)
    rng = np.random.default_rng(4)
    for i, (h, w) in enumerate([(1, 1), (5, 7), (17, 9), (45, 37), (72, 40)]):
        for q, s in ((1, 0), (85, 2), (100, 0), (100, 2)):
            px = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
            name = "px%d_%d_%d" % (i, q, s)
            text += _c_line(name, h, w, q, s, model.flat_coefs(model.planes_of(px, q, s)))
            want[name] = (model.jpeg_file(px, q, s), None)
    return text, want


@pytest.mark.parametrize("byte", [0x00, 0xFF, 0x5A])
def test_nothing_depends_on_what_lds_and_scratch_held(tmp_path, byte):
    """every case of the test below, under the sanitizers with dirty LDS and scratch: the same lines as the plain run"""
    exe = _exe(str(tmp_path))
    text, want = _script()
    plain = _run(exe, text)
    assert len(plain) == len(HWS) * 8 + len(want) and _run(exe, text, "--poison", str(byte)) == plain


def test_native_against_the_model(tmp_path):
    exe = _exe(str(tmp_path))
    text, want = _script()
    got = _run(exe, text)
    for h, w in HWS:
        for q in (1, 50, 85, 100):
            for s in (0, 2):
                assert got["F %d %d %d %d" % (h, w, q, s)] == "%d %d" % (model.file_bound(h, w, q, s), model.base64_bound(h, w, q, s))
    for name, (f, events) in want.items():
        head, ev = got["C " + name].split(" | ")
        n, hx = head.split()
        assert int(n) == len(f) and bytes.fromhex(hx) == f, name
        if events is None:
            continue
        restart, block, early, zrl_first, zrl_refine, to_zero, dc_neg = (int(v) for v in ev.split())
        assert restart == events.get("eobrun_restart", 0) and block == events.get("eobrun_block", 0) and early == events.get("corr_bits_early_flush", 0), name
        assert zrl_first == events.get("zrl_first", 0) and zrl_refine == events.get("zrl_refine", 0) and to_zero == events.get("ac_shifted_to_zero", 0), name
        assert dc_neg == events.get("dc_negative_shift", 0), name
