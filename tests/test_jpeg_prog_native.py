"""csrc/jpeg_parse.hpp's file entry and csrc/jpeg_dec_core.hpp's scan kinds on the CPU (tests/native/jpeg_prog_sim.cpp: a progressive file
decoded the way csrc/jpeg_dec.hip decodes it, with lanes, windows, waves and launches as loops, the steps the kernels' own compiled
for the host), built plain and under ASan + UBSan as a stand-alone program: its coefficients equal the model's on every case, its
refusals carry the model's reasons, and malformed input ends in a refusal or a non-zero status with no sanitizer report -- before
any of it reaches a GPU.  With "--poison BYTE" (tests/native/sim_poison.hpp: the lane records, window heads, masks and walk records,
the walk's LDS, the staged words and the lanes' state dirty; the coefficients cleared as jpeg_dec_launch clears them) every line, and
the coefficients of every file with status 0, equal the plain run's."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_decode_cases as cases      # noqa: E402
import jpeg_decode_model as base       # noqa: E402
import jpeg_prog_cases as prog         # noqa: E402
import jpeg_prog_model as model        # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "jpeg_prog_sim.cpp")


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
    tmp = tmp_path_factory.mktemp("jpeg_prog_sim")
    return tmp, _build(tmp, "sim", ["-O2"]), _build(tmp, "sim_san", ["-O1", "-fsanitize=address,undefined"])


def consts(exe):
    f = _run(exe, "consts")[0].split()
    return dict(zip(f[0::2], (int(v) for v in f[1::2])))


def _dump(tmp, exe, data, poison=False, dirty=None):
    """-> (head fields, the status line's fields, coefficients int16 flat) or the refusal's reason; poison: wrong guesses; dirty: --poison BYTE"""
    src, out = str(tmp / "in.jpg"), str(tmp / "out.bin")
    with open(src, "wb") as f:
        f.write(data)
    lines = _run(exe, *(() if dirty is None else ("--poison", str(dirty))), "dump", src, out, *(["poison"] if poison else []))
    if lines[0].startswith("refused "):
        return lines[0][len("refused "):]
    f = lines[1].split()
    return [int(v) for v in lines[0].split()[1:]], dict(zip(f[0::2], (int(v) for v in f[1::2]))), np.fromfile(out, np.int16)


def _model_coefficients(data):
    p = model.plan(data)
    return p, np.concatenate([g.reshape(-1) for g in model.coefficients(p)])


def _compare(tmp, exe, files, poison=False):
    for name, data in files.items():
        p, want = _model_coefficients(data)
        head, st, got = _dump(tmp, exe, data, poison)
        assert head[:3] == [p.h, p.w, p.sampling] and head[4:] == [len(p.scans), p.nlevels], (name, head)
        assert st["status"] == 0, (name, st)
        assert got.size == want.size and np.array_equal(got.astype(np.int64), want), name
    return len(files)


def test_coefficients_equal_the_model(exes):
    tmp, exe, exe_san = exes
    grid = prog.pillow_grid_cases()
    written = {k: v[0] for k, v in prog.writer_cases().items()}
    assert _compare(tmp, exe, grid) == 109
    assert _compare(tmp, exe, prog.sweep_cases()) == 589
    assert _compare(tmp, exe, written) == 72
    assert _compare(tmp, exe, {"cap": prog.cap_scans_file()[0]}) == 1
    # under the sanitizers, and with the output equal: every file of the writer, and one Pillow file of every sampling
    san = dict(written)
    san.update({k: v for k, v in grid.items() if k.startswith(("33x47", "grey_17x13", "5x3"))})
    assert _compare(tmp, exe_san, san) >= 72 + 15


@pytest.mark.parametrize("byte", [0x00, 0xFF, 0x5A])
def test_nothing_depends_on_what_lds_and_scratch_held(exes, byte):
    """every file of the writer, the Pillow grid, the 64-scan file, a baseline file, the multi-window files (wrong guesses too), the flat
    file, the long-refinement file, the refused files, the malformed pack and the corrupt refinement scans, under the sanitizers with
    dirty scratch and LDS, against the plain program's unpoisoned run"""
    tmp, exe, exe_san = exes
    files = {k: v[0] for k, v in prog.writer_cases().items()}
    files.update(prog.pillow_grid_cases())
    files["cap"] = prog.cap_scans_file()[0]
    files["baseline"] = cases.encode(cases.noise(47, 33, 3), 85, 2)
    files["flat"] = prog.flat_file()
    files["long_refinement"] = prog.long_refinement_file()
    files.update({"refused_" + k: v[0] for k, v in prog.refused_cases().items()})
    many = prog.multi_window_files(consts(exe)["window_bits"])
    for name, data in list(files.items()) + [(k + "_guesses", v) for k, v in many.items()] + list(many.items()):
        guesses = name.endswith("_guesses")
        a, b = _dump(tmp, exe_san, data, guesses, dirty=byte), _dump(tmp, exe, data, guesses)
        if isinstance(a, str) or isinstance(b, str):
            assert a == b, name
            continue
        assert a[0] == b[0] and a[1] == b[1], (name, a[:2], b[:2])
        if a[1]["status"] == 0:
            assert np.array_equal(a[2], b[2]), name
    for which, variants in (("malformed", prog.malformed_pack()[1]), ("refine", prog.corrupt_refinement_candidates()[1])):
        pack = str(tmp / ("poison_%s.bin" % which))
        with open(pack, "wb") as f:
            for _, data in variants:
                f.write(struct.pack("<I", len(data)) + data)
        lines = _run(exe_san, "--poison", str(byte), "batch", pack)
        assert len(lines) == len(variants) and lines == _run(exe, "batch", pack), which


def test_a_baseline_file_takes_the_same_way(exes):
    """plan_file with the progressive bit set still reads a baseline file, and the window path decodes it as before"""
    tmp, exe, _ = exes
    data = cases.encode(cases.noise(47, 33, 3), 85, 2)
    p = base.plan(data)
    want = np.concatenate([g.reshape(-1) for g in base.coefficients(p)])
    head, st, got = _dump(tmp, exe, data)
    assert head == [p.h, p.w, p.sampling, want.size // 64, 1, 1] and st["status"] == 0
    assert np.array_equal(got.astype(np.int64), want)


def test_first_scans_of_several_windows(exes):
    """two files whose largest first scan has 2.5 windows or more, every guessed start state of the window path poisoned"""
    tmp, exe, exe_san = exes
    c = consts(exe)
    assert c["window_bits"] == c["lanes"] * c["subseq_bits"]
    files = prog.multi_window_files(c["window_bits"])
    assert len(files) == 2
    for name, data in files.items():
        nwin = -(-8 * prog.largest_stream(data, (model.DC_FIRST, model.AC_FIRST)) // c["window_bits"])
        assert 8 * prog.largest_stream(data, (model.DC_FIRST, model.AC_FIRST)) >= 2.5 * c["window_bits"], name
        _, want = _model_coefficients(data)
        for e, poison in ((exe, False), (exe, True), (exe_san, True)):
            head, st, got = _dump(tmp, e, data, poison)
            print(name, poison, st)
            assert st["status"] == 0 and st["maxwin"] == nwin >= 3, (name, st)
            assert np.array_equal(got.astype(np.int64), want), (name, poison)


def test_flat_image_eob_runs_only(exes):
    """flat 1024 x 1032 grey: every AC scan is EOB-run symbols only, a run of 16384 blocks and a remainder -- far more blocks than bits,
    and more than any lane's subsequence holds"""
    tmp, exe, exe_san = exes
    data = prog.flat_file()
    p, want = _model_coefficients(data)
    assert p.scans[1].nmcu == 128 * 129 == 16512 and all(len(s.streams[0]) <= 8 for s in p.scans if s.kind in (model.AC_FIRST, model.AC_REFINE))
    for e in (exe, exe_san):
        head, st, got = _dump(tmp, e, data)
        assert st["status"] == 0 and st["maxrun"] == 16512 > 16384, st
        assert np.array_equal(got.astype(np.int64), want)


def test_a_refinement_stream_longer_than_the_walks_staging(exes):
    tmp, exe, exe_san = exes
    c = consts(exe)
    data = prog.long_refinement_file()
    longest = prog.largest_stream(data, (model.AC_REFINE,))
    assert longest > c["short_max_bytes"] and longest > 8 * 4 * c["walk_words"], longest      # the wave kernel's, and many turns of it
    _, want = _model_coefficients(data)
    for e in (exe, exe_san):
        head, st, got = _dump(tmp, e, data)
        print(longest, st)
        # a turn ends with the staged words (4 * walk_words bytes) or with the staged blocks: at least as many as the words need
        assert st["status"] == 0 and st["turns"] >= longest // (4 * c["walk_words"]), st
        assert np.array_equal(got.astype(np.int64), want)


def test_refusal_reasons_equal_the_models(exes):
    tmp, exe, _ = exes
    files = prog.refused_cases()
    assert len(files) == 7
    for name, (data, word) in files.items():
        why = _dump(tmp, exe, data)
        with pytest.raises(model.Refused) as e:
            model.plan(data)
        assert why == "invalid: " + e.value.reason and word in why, (name, why)


def test_accept_zero_is_the_baseline_plan(exes):
    """plan_file with accept == 0: the reasons of plan(), the progressive one among them"""
    tmp, exe, _ = exes
    src = str(tmp / "plan.jpg")
    n = 0
    for name, (data, word) in list(cases.refused_cases().items()) + [("good", (cases.encode(cases.smooth(16, 16, 3)), None))]:
        with open(src, "wb") as f:
            f.write(data)
        line = _run(exe, "plan", src, "0")[0]
        if word is None:
            assert line == "ok 16 16 0 1"
        else:
            with pytest.raises(base.Refused) as e:
                base.plan(data)
            assert line == "refused invalid: " + e.value.reason and word in line, name
        n += 1
    assert n == 5
    with open(src, "wb") as f:
        f.write(cases.refused_cases()["progressive"][0])
    assert _run(exe, "plan", src, "1")[0] == "ok 16 16 0 10"


def test_malformed_input_under_the_sanitizers(exes):
    """a 17 x 13 4:2:0 progressive file cut at every tenth byte and 200 single-byte corruptions spread over its scans: a refusal or a
    non-zero status wherever the model raises, the model's coefficients where it decodes, and no sanitizer report"""
    tmp, _, exe_san = exes
    good, variants = prog.malformed_pack()
    pack = str(tmp / "pack.bin")
    with open(pack, "wb") as f:
        for _, data in variants:
            f.write(struct.pack("<I", len(data)) + data)
    lines = _run(exe_san, "batch", pack)
    assert len(lines) == len(variants) == 200 + (len(good) + 9) // 10
    reached, clean = 0, 0
    for (name, data), line in zip(variants, lines):
        try:
            want = _model_coefficients(data)[1]
            verdict = "ok"
        except model.Refused as e:
            verdict = "refused invalid: " + e.reason
        except model.Corrupt:
            verdict = "corrupt"
        if name.startswith("cut_"):
            assert line.startswith("refused invalid: "), (name, line)
        if line.startswith("refused"):
            assert line == verdict, (name, line, verdict)
            continue
        reached += 1
        status = int(line.split()[1])
        assert (status == 0) == (verdict == "ok"), (name, line, verdict)
        if status == 0:
            clean += 1
            got = _dump(tmp, exe_san, data)[2]
            assert np.array_equal(got.astype(np.int64), want), name
    print("%d corruptions reached the decoder, %d of them still well-formed" % (reached, clean))
    assert reached - clean >= 50


def test_corruptions_of_a_refinement_scan(exes):
    """the candidates from which the GPU tests take their one corrupt file (a byte changed inside the last AC refinement scan): under
    the sanitizers every one ends as the model says, a non-zero status wherever it raises, and several are flagged"""
    tmp, _, exe_san = exes
    good, variants = prog.corrupt_refinement_candidates()
    assert len(variants) == 40
    pack = str(tmp / "refine.bin")
    with open(pack, "wb") as f:
        for _, data in variants:
            f.write(struct.pack("<I", len(data)) + data)
    lines = _run(exe_san, "batch", pack)
    assert len(lines) == 40
    flagged = 0
    for (name, data), line in zip(variants, lines):
        try:
            model.coefficients(model.plan(data))
            ok = True
        except model.Corrupt:
            ok = False
        assert line.startswith("status ") and (int(line.split()[1]) == 0) == ok, (name, line, ok)
        flagged += not ok
    print("%d of 40 flagged" % flagged)
    assert flagged >= 5
