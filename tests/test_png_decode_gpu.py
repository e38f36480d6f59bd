"""The PNG decoder on the device (csrc/png_dec.hip behind csrc/png_parse.hpp) through the C ABI, on an engine created with
IRE_FLAG_DECODE_PNG: its pixels equal Pillow's byte for byte on every shape, colour type, filter and stream of tests/png_cases.py; a
batch of mixed colour types equals the single decodes and touches nothing outside its images; corrupt data gets the status the CPU
form of the decoder gives it, and its neighbours in the batch decode right."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_cases as cases      # noqa: E402

from image_restoration_platform_amd import _lib      # noqa: E402
from image_restoration_platform_amd.engine import Engine, EngineError      # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def png_engine():
    eng = Engine(device_index=0, max_batch=8, num_streams=1, decode_png=True)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def accept():
    files = cases.accept_cases()
    return {name: (data, cases.pil_rgb(data)) for name, data in files.items()}      # the reference, computed once


@pytest.mark.filterwarnings("ignore:Palette images with Transparency")
def test_device_equals_pillow(png_engine, accept):
    """1x1, 1x7, 7x1; 5x7 of every colour type; 63, 64, 65 and 129 rows for the band hand-over; 200x160 RGB; all five filters; zlib's
    levels, windows, strategies and flushes with IDAT cut at one byte; the hand-made streams (258 at 32768, distance 1, 15-bit codes, one
    distance code, literals only, a repeat code across the two sets of lengths)"""
    assert len(accept) >= 50
    for name, (data, want) in accept.items():
        plan = png_engine.decode_png_plan(data)
        assert plan is not None and plan[:2] == want.shape[:2], (name, plan, png_engine.last_plan_reason)
        got = png_engine.decode_png(data)
        bad = int((got != want).sum())
        print("%-16s %6d bytes  plan %s  differing bytes %d" % (name, len(data), plan, bad))
        assert got.shape == want.shape and bad == 0, name


def test_a_batch_of_mixed_colour_types_equals_the_single_decodes(png_engine):
    import torch
    types = [cases.TYPES[i % 5] for i in range(png_engine.max_batch)]
    files = [cases.make(65, 33, ct, filters=(4, 1, 3, 2, 0), seed=20 + i) for i, ct in enumerate(types)]
    singles = [png_engine.decode_png(f) for f in files]
    for f, s in zip(files, singles):
        assert np.array_equal(s, cases.pil_rgb(f))
    out, status = png_engine.decode_png_device(files)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * len(files)
    for i, s in enumerate(singles):
        assert np.array_equal(out[i].cpu().numpy(), s), (i, types[i])


def test_an_image_pitch_larger_than_the_image(png_engine):
    import torch
    files = [cases.make(7, 5, ct, seed=30 + ct) for ct in (2, 3, 6)]
    n, h, w, gap = len(files), 7, 5, 37
    buf = torch.full((n, h * w * 3 + gap), 0xA5, dtype=torch.uint8, device="cuda")
    view = buf[:, :h * w * 3].view(n, h, w, 3)
    out, status = png_engine.decode_png_device(files, out_u8=view)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert status.cpu().tolist() == [0] * n
    for i, f in enumerate(files):
        assert np.array_equal(host[i, :h * w * 3].reshape(h, w, 3), cases.pil_rgb(f)), i
        assert (host[i, h * w * 3:] == 0xA5).all(), i          # the bytes behind each image: untouched


def _cpu_statuses(tmp, files):
    """the statuses csrc/png_inflate_core.hpp gives on the CPU (tests/native/png_dec_sim.cpp, built PLAIN here: no sanitizer runs in a GPU
    test).  That these ten files are safe to send to a device rests on the CPU suite having run first:
    tests/test_png_native.py::test_corrupt_data_gets_ten_distinct_statuses puts the same files through the same text under ASan and UBSan."""
    exe = str(tmp / "png_dec_sim")
    r = subprocess.run(["g++", "-std=c++17", "-O2", os.path.join(ROOT, "tests", "native", "png_dec_sim.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = {}
    for name, data in files.items():
        src = str(tmp / "in.png")
        with open(src, "wb") as f:
            f.write(data)
        lines = subprocess.run([exe, "dump", src, str(tmp / "rgb.bin"), str(tmp / "scan.bin")], capture_output=True, text=True, timeout=60).stdout.splitlines()
        assert lines[1].startswith("status "), (name, lines)
        out[name] = int(lines[1].split()[1])
    return out


def test_corrupt_data_is_flagged_and_its_neighbours_decode(png_engine, tmp_path):
    """the ten corrupt streams of tests/png_cases.py, one distinct status each: first through the decoder's CPU form, then in batches
    between good files of their size"""
    import torch
    corrupt = cases.corrupt_cases()
    want = _cpu_statuses(tmp_path, corrupt)
    assert len(set(want.values())) == 10 and 0 not in want.values()
    good = cases.fuzz_file()
    good_px = cases.pil_rgb(good)
    names = sorted(corrupt)
    for at in range(0, len(names), 4):
        part = names[at:at + 4]
        files, expect = [good], [0]
        for name in part:
            files += [corrupt[name], good]
            expect += [want[name], 0]
        out, status = png_engine.decode_png_device(files[:png_engine.max_batch])
        torch.cuda.synchronize()
        got = status.cpu().tolist()
        print(part, got)
        assert got == expect[:png_engine.max_batch]
        for i, st in enumerate(got):
            if st == 0:
                assert np.array_equal(out[i].cpu().numpy(), good_px), (part, i)
    with pytest.raises(EngineError) as e:
        png_engine.decode_png(corrupt["adler"])
    assert e.value.status == _lib.IRE_ERR_INVALID_INPUT and "corrupt PNG data (decoder status %d)" % want["adler"] in e.value.message
    assert np.array_equal(png_engine.decode_png(good), good_px)          # the engine stays usable


def test_an_engine_without_the_flag_refuses(engine):
    with pytest.raises(EngineError) as e:
        engine.decode_png(cases.fuzz_file())
    assert e.value.status == _lib.IRE_ERR_INVALID_INPUT and "IRE_FLAG_DECODE_PNG" in e.value.message
