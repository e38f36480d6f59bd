"""The numpy model of the progressive decoder (tests/jpeg_prog_model.py) against Pillow (libjpeg-turbo), and the test-side writer
(tests/jpeg_prog_writer.py) against Pillow: the model's pixels equal Pillow's on Pillow's own progressive files and on every script the
writer stands in for; every file the writer makes decodes, in Pillow, to the pixels of the baseline file its coefficients came from.
The library's host-only plan entry (ire_decode_jpeg_plan_ex: no engine, no GPU) is held to the model on every file on the way: same
size, sampling and scan count, same refusals."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_decode_cases as cases      # noqa: E402
import jpeg_decode_model as base       # noqa: E402
import jpeg_prog_cases as prog         # noqa: E402
import jpeg_prog_model as model        # noqa: E402
import jpeg_prog_writer as writer      # noqa: E402

from image_restoration_platform_amd import _lib      # noqa: E402


def _lib_plan(data):
    """ire_decode_jpeg_plan_ex accepting progressive files -> (h, w, sampling, scans) | the reason without its leading "invalid: " """
    lib = _lib.load()
    h, w, s, k = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    if lib.ire_decode_jpeg_plan_ex(data, len(data), _lib.IRE_DECODE_ACCEPT_PROGRESSIVE, ctypes.byref(h), ctypes.byref(w), ctypes.byref(s), ctypes.byref(k)) != 0:
        why = (lib.ire_last_error() or b"").decode()
        assert why.startswith("invalid: ")
        return why[len("invalid: "):]
    return h.value, w.value, s.value, k.value


def _equal_pillow(files):
    for name, data in files.items():
        assert np.array_equal(model.decode(data), cases.pillow_pixels(data)), name
        p = model.plan(data)
        assert _lib_plan(data) == (p.h, p.w, p.sampling, len(p.scans)), name
    return len(files)


def test_pillow_files_grid():
    # 7 sizes x 3 samplings x (4 qualities + restart), less the two subsampled samplings of width 5 ... none: 5 >= 5; + 4 grey
    assert _equal_pillow(prog.pillow_grid_cases()) == 7 * 3 * 5 + 4


def test_pillow_files_sweep():
    assert _equal_pillow(prog.sweep_cases()) == 19 * 31


def test_pillow_writes_the_simple_progression():
    """what the issue's design rests on: 10 scans in 3 levels for colour, 6 for grey, DRI and RSTn with restart_marker_blocks"""
    p = model.plan(writer.pillow_progressive(cases.noise(13, 17, 5), 85, 2))
    assert [(tuple(s.comps), s.ss, s.se, s.ah, s.al) for s in p.scans] == writer.script_simple()
    assert model.levels(p) == [0, 0, 0, 0, 0, 1, 1, 1, 1, 2] and p.nlevels == 3
    g = model.plan(writer.pillow_progressive(cases.noise(13, 17, 5)[:, :, 0], 85))
    assert [(tuple(s.comps), s.ss, s.se, s.ah, s.al) for s in g.scans] == writer.for_grey(writer.script_simple()) and len(g.scans) == 6
    r = model.plan(writer.pillow_progressive(cases.noise(13, 17, 5), 85, 2, restart_marker_blocks=3))
    assert all(s.restart == 3 for s in r.scans)
    # not interleaved: 3 x 2 REAL luma blocks (the padded grid has 4 x 2) -> 2 streams; interleaved: 2 MCUs -> 1 stream
    assert [s.nstreams for s in r.scans] == [1, 2, 1, 1, 2, 2, 1, 1, 1, 2]
    assert _lib_plan(writer.pillow_progressive(cases.noise(13, 17, 5), 85, 2)) == (13, 17, 2, 10) and _lib_plan(writer.pillow_progressive(cases.noise(13, 17, 5)[:, :, 0], 85)) == (13, 17, 3, 6)


def test_the_writer_against_pillow_and_the_model_on_its_files():
    """every script x 8x8, 17x13, 33x47 x three samplings and grey: Pillow reads the writer's file as the source baseline file, and
    so does the model"""
    files = prog.writer_cases()
    assert len(files) == len(writer.SCRIPTS) * 3 * 4 == 72
    for name, (data, src) in files.items():
        want = cases.pillow_pixels(src)
        assert np.array_equal(cases.pillow_pixels(data), want), name
        assert np.array_equal(model.decode(data), want), name
        assert _lib_plan(data) == want.shape[:2] + (model.plan(data).sampling, len(model.plan(data).scans)), name
    # the simple script reproduces Pillow's structure
    p = model.plan(files["simple_17x13_s2"][0])
    assert [(tuple(s.comps), s.ss, s.se, s.ah, s.al) for s in p.scans] == writer.script_simple()
    # the mozjpeg-style scripts: DC scans of one component each, and two refinement scans of one component in one level
    p = model.plan(files["moz_flat_chroma_33x47_s2"][0])
    assert model.levels(p) == [0] * 7 + [1, 1, 2]
    # restart intervals of the non-interleaved scans count blocks of the real plane
    p = model.plan(files["moz_rst3_17x13_s2"][0])
    assert [s.nstreams for s in p.scans][:3] == [2, 1, 1]


def test_the_cap_of_64_scans():
    data, src = prog.cap_scans_file()
    assert len(model.plan(data).scans) == model.MAX_SCANS == _lib.IRE_DECODE_MAX_SCANS == 64 and _lib_plan(data) == (13, 17, 3, 64)
    assert np.array_equal(model.decode(data), cases.pillow_pixels(src))


def test_refusals():
    files = prog.refused_cases()
    assert len(files) == 7
    for name, (data, word) in files.items():
        with pytest.raises(model.Refused) as e:
            model.plan(data)
        assert word in e.value.reason and e.value.reason.startswith(("progressive JPEG", "JPEG")), (name, e.value.reason)
        assert _lib_plan(data) == e.value.reason, name
    # and the baseline parser's own refusals hold for a progressive frame too
    good = writer.pillow_progressive(cases.smooth(16, 16, 3), 85, 0)
    with pytest.raises(model.Refused) as e:
        model.plan(good[:100])
    assert e.value.reason == "truncated JPEG header" == _lib_plan(good[:100])
    with pytest.raises(model.Refused) as e:
        model.plan(good[:-3])
    assert e.value.reason == "truncated JPEG scan (no EOI)" == _lib_plan(good[:-3])


def test_big_files():
    """the three big files of the native and GPU tests decode to Pillow's pixels in the model"""
    files = dict(prog.multi_window_files(256 * 1024))
    files["flat"] = prog.flat_file()
    files["long_refinement"] = prog.long_refinement_file()
    assert _equal_pillow(files) == 4
