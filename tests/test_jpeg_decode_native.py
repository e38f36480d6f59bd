"""csrc/jpeg_parse.hpp and csrc/jpeg_dec_core.hpp on the CPU (tests/native/jpeg_dec_sim.cpp: the lane algorithm of csrc/jpeg_dec.hip
with lanes as a loop, the kernels' own step and loop compiled for the host), built plain and under ASan + UBSan: its coefficients
equal the model's on every case, some case needs more than one round and some stream more than one window, and malformed input
ends in a refusal or a non-zero status with no sanitizer report -- before any of it reaches a GPU.  With "--poison BYTE"
(tests/native/sim_poison.hpp: dirty LDS, lane state and staging; the coefficients cleared as jpeg_dec_launch clears them) every line,
and the coefficients of every file with status 0, equal the plain run's."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_decode_cases as cases      # noqa: E402
import jpeg_decode_model as model      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "jpeg_dec_sim.cpp")


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
    tmp = tmp_path_factory.mktemp("jpeg_dec_sim")
    return tmp, _build(tmp, "sim", ["-O2"]), _build(tmp, "sim_san", ["-O1", "-fsanitize=address,undefined"])


def consts(exe):
    f = _run(exe, "consts")[0].split()
    return dict(zip(f[0::2], (int(v) for v in f[1::2])))


def _dump(tmp, exe, data, poison=None):
    """-> (head fields, {status, rounds, windows, longest}, coefficients int16 flat) or the refusal's reason"""
    src, out = str(tmp / "in.jpg"), str(tmp / "out.bin")
    with open(src, "wb") as f:
        f.write(data)
    lines = _run(exe, *(() if poison is None else ("--poison", str(poison))), "dump", src, out)
    if lines[0].startswith("refused "):
        return lines[0][len("refused "):]
    f = lines[1].split()
    return [int(v) for v in lines[0].split()[1:]], dict(zip(f[0::2], (int(v) for v in f[1::2]))), np.fromfile(out, np.int16)


def _model_coefficients(data):
    p = model.plan(data)
    return p, np.concatenate([g.reshape(-1) for g in model.coefficients(p)])


def _compare(tmp, exe, files):
    for name, data in files.items():
        p, want = _model_coefficients(data)
        head, st, got = _dump(tmp, exe, data)
        assert head[:3] == [p.h, p.w, p.sampling], name
        assert st["status"] == 0, (name, st)
        assert got.size == want.size and np.array_equal(got.astype(np.int64), want), name


def test_coefficients_equal_the_model(exes):
    tmp, exe, exe_san = exes
    grid = cases.grid_cases()
    _compare(tmp, exe, grid)
    _compare(tmp, exe, cases.encoder_cases())
    _compare(tmp, exe, cases.sweep_cases())          # all 589 partial-MCU shapes
    # under the sanitizers: one file of every sampling and table variant
    _compare(tmp, exe_san, {k: v for k, v in grid.items() if k.startswith(("33x47", "grey_17x13", "5x3"))})


def test_long_streams_rounds_and_windows(exes):
    """streams long enough for the lane path: more than one round to settle, and more than one window"""
    tmp, exe, exe_san = exes
    c = consts(exe)
    assert c["window_bits"] == c["lanes"] * c["subseq_bits"]
    side = 16
    while True:                                              # the smallest noise image whose single stream passes 1.25 windows
        data = cases.encode(cases.noise(side, side, 41), 95, 0)
        p = model.plan(data)
        if 8 * len(p.streams[0][0]) >= 1.25 * c["window_bits"]:
            break
        side += 16
    _, want = _model_coefficients(data)
    for e in (exe, exe_san):
        head, st, got = _dump(tmp, e, data)
        print(side, len(p.streams[0][0]), st)
        assert st["status"] == 0 and st["windows"] >= 2 and st["longest"] > 1
        assert np.array_equal(got.astype(np.int64), want)
    # 4:2:0 (the block index in the state makes it slower to lock) and a flat image (hundreds of blocks per subsequence)
    for name, data in (("420", cases.encode(cases.noise(96, 96, 42), 95, 2)), ("flat", cases.encode(np.full((512, 512, 3), 77, np.uint8), 85, 0)),
                       ("smooth422", cases.encode(cases.smooth(160, 200, 43), 95, 1, optimize=True))):
        assert len(model.plan(data).streams[0][0]) > c["short_max_bytes"], name
        _, want = _model_coefficients(data)
        head, st, got = _dump(tmp, exe, data)
        print(name, st)
        assert st["status"] == 0 and st["windows"] >= 1 and np.array_equal(got.astype(np.int64), want), name


def _long_files(c):
    side = 16
    while True:
        data = cases.encode(cases.noise(side, side, 41), 95, 0)
        if 8 * len(model.plan(data).streams[0][0]) >= 1.25 * c["window_bits"]:
            break
        side += 16
    return {"long_noise": data, "long_420": cases.encode(cases.noise(96, 96, 42), 95, 2), "long_flat": cases.encode(np.full((512, 512, 3), 77, np.uint8), 85, 0),
            "long_smooth422": cases.encode(cases.smooth(160, 200, 43), 95, 1, optimize=True)}


@pytest.mark.parametrize("byte", [0x00, 0xFF, 0x5A])
def test_nothing_depends_on_what_lds_and_scratch_held(exes, byte):
    """the grid, the encoder's files, the long streams, the refused files and the malformed pack under the sanitizers with dirty LDS and
    scratch, against the plain program's unpoisoned run: the same lines, and at status 0 the same coefficients"""
    tmp, exe, exe_san = exes
    files = dict(cases.grid_cases())
    files.update(cases.encoder_cases())
    files.update(cases.sweep_cases())
    files.update(_long_files(consts(exe)))
    files.update({"refused_" + k: v[0] for k, v in cases.refused_cases().items()})
    for name, data in files.items():
        a, b = _dump(tmp, exe_san, data, poison=byte), _dump(tmp, exe, data)
        if isinstance(a, str) or isinstance(b, str):
            assert a == b, name
            continue
        assert a[0] == b[0] and a[1] == b[1], (name, a[:2], b[:2])
        if a[1]["status"] == 0:
            assert np.array_equal(a[2], b[2]), name
    _, variants = cases.malformed_pack()
    pack = str(tmp / "pack_poison.bin")
    with open(pack, "wb") as f:
        for _, data in variants:
            f.write(struct.pack("<I", len(data)) + data)
    lines = _run(exe_san, "--poison", str(byte), "batch", pack)
    assert len(lines) == len(variants) and lines == _run(exe, "batch", pack)


def test_plan_reasons_equal_the_models(exes):
    tmp, exe, _ = exes
    for name, (data, word) in cases.refused_cases().items():
        why = _dump(tmp, exe, data)
        with pytest.raises(model.Refused) as e:
            model.plan(data)
        assert why == "invalid: " + e.value.reason and word in why, name


def test_malformed_input_under_the_sanitizers(exes):
    """truncations at every tenth byte, 200 single-byte corruptions of the scan, a DHT whose counts overrun its segment: each ends in
    a refusal or a non-zero status -- or, where a flipped bit still leaves a well-formed stream, in status 0 exactly where the model
    decodes the file too -- and the sanitizers report nothing"""
    tmp, _, exe_san = exes
    good, variants = cases.malformed_pack()
    pack = str(tmp / "pack.bin")
    with open(pack, "wb") as f:
        for _, data in variants:
            f.write(struct.pack("<I", len(data)) + data)
    lines = _run(exe_san, "batch", pack)
    assert len(lines) == len(variants)
    clean = []
    for (name, data), line in zip(variants, lines):
        if name.startswith("cut_") or name == "dht_overrun":
            assert line.startswith("refused invalid: "), (name, line)
            continue
        if line.startswith("refused invalid: "):
            continue
        status = int(line.split()[1])
        try:
            model.coefficients(model.plan(data))
            model_ok = True
        except (model.Corrupt, model.Refused):
            model_ok = False
        assert (status == 0) == model_ok, (name, line)
        clean.append(status == 0)
    print("%d corruptions reached the decoder, %d of them still well-formed streams" % (len(clean), sum(clean)))
    assert clean.count(False) >= 50
    assert "dht_overrun" == variants[-1][0] and "DHT" in lines[-1]
