"""Long streams of several windows on the device (csrc/jpeg_dec.hip: the spec, chain and write kernels): pixels equal Pillow's and
the status is 0 on files of two and three windows of every sampling, a batch mixes the three stream kernels, the launches that ran
are the window-parallel ones (and the one-workgroup kernel's under IRE_JPEG_DEC_WINDOWS=0, with the same pixels), and a corrupt
multi-window file is flagged alone.  The same files pass through the kernels' code on the CPU in
test_jpeg_decode_windows_native.py."""
import base64
import json
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_decode_cases as cases      # noqa: E402
import jpeg_decode_model as model      # noqa: E402
import jpeg_decode_window_cases as wcases      # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _consts():
    src = open(os.path.join(ROOT, "image_restoration_platform_amd", "csrc", "jpeg_dec_core.hpp")).read()
    lanes = int(re.search(r"constexpr int kLanes = (\d+);", src).group(1))
    bits = int(re.search(r"constexpr int kSubseqBits = (\d+);", src).group(1))
    short = int(re.search(r"constexpr unsigned kShortMaxBytes = (\d+);", src).group(1))
    return lanes * bits, short


def _windows(data):
    p = model.plan(data)
    assert len(p.streams) == 1
    return -(-8 * len(p.streams[0][0]) // _consts()[0])


@pytest.fixture(scope="module")
def files():
    return wcases.multi_window_files()


@pytest.mark.parametrize("name", ["128x128_q95_444", "192x192_q95_444", "160x200_q95_444", "256x256_q90_420", "256x256_q92_422", "grey_256x256_q95"])
def test_multi_window_files_equal_pillow(engine, files, name):
    data, windows = files[name]
    assert _windows(data) == windows and windows >= 2, name
    want = cases.pillow_pixels(data)
    out, status = engine.decode_jpeg_device([data])
    got = out[0].cpu().numpy()
    bad = int((got != want).sum())
    print("%-18s %6d bytes, %d windows, differing bytes %d, status %d" % (name, len(data), windows, bad, int(status[0])))
    assert int(status[0]) == 0 and got.shape == want.shape and bad == 0, name


def test_a_batch_mixes_the_three_stream_kernels(engine):
    """a multi-window stream (spec / chain / write), a single-window long stream (the one-workgroup kernel) and the engine's own
    file of 16-MCU restart intervals (short streams) in one batch"""
    window_bits, short = _consts()
    px = cases.smooth(256, 256, 12)
    many = cases.encode(cases.noise(256, 256, 11), 95, 0)
    one = cases.encode(px, 85, 0)
    own = base64.b64decode(engine.encode_jpeg_base64_fit(px[None])[0])
    assert _windows(many) >= 2
    assert _windows(one) == 1 and len(model.plan(one).streams[0][0]) > short
    assert len(model.plan(own).streams) > 1 and max(len(s[0]) for s in model.plan(own).streams) <= short
    batch = [many, one, own]
    out, status = engine.decode_jpeg_device(batch)
    assert status.cpu().tolist() == [0, 0, 0]
    for i, f in enumerate(batch):
        assert np.array_equal(out[i].cpu().numpy(), cases.pillow_pixels(f)), i


def _timed_engine_decodes(monkeypatch, capfd, windows_env, batch):
    """an engine of its own with IRE_JPEG_DEC_TIMES=1 (both switches are read when an engine is created) -> pixels, status, the
    per-launch sums it prints when it closes"""
    from image_restoration_platform_amd.engine import Engine
    monkeypatch.setenv("IRE_JPEG_DEC_TIMES", "1")
    if windows_env is None:
        monkeypatch.delenv("IRE_JPEG_DEC_WINDOWS", raising=False)
    else:
        monkeypatch.setenv("IRE_JPEG_DEC_WINDOWS", windows_env)
    eng = Engine(device_index=0, max_batch=8, weights_path=None)
    capfd.readouterr()
    try:
        out, status = eng.decode_jpeg_device(batch)
        px, st = out.cpu().numpy(), status.cpu().tolist()
    finally:
        eng.close()
    err = capfd.readouterr().err
    line = next(ln for ln in err.splitlines() if ln.startswith('{"jpeg_dec_kernel_ms"'))
    return px, st, json.loads(line)["jpeg_dec_kernel_ms"]


def test_the_window_kernels_are_the_ones_that_run_and_the_switch_keeps_the_old_one(files, monkeypatch, capfd):
    data = files["192x192_q95_444"][0]
    want = cases.pillow_pixels(data)
    px, st, ms = _timed_engine_decodes(monkeypatch, capfd, None, [data])
    print("default:", ms)
    assert st == [0] and np.array_equal(px[0], want)
    assert ms["calls"] == 1 and ms["spec"] > 0 and ms["chain"] > 0 and ms["write"] > 0
    assert ms["spec"] + ms["chain"] + ms["write"] > ms["long"]              # no one-workgroup launch: two marks in a row
    px0, st0, ms0 = _timed_engine_decodes(monkeypatch, capfd, "0", [data])
    print("IRE_JPEG_DEC_WINDOWS=0:", ms0)
    assert st0 == [0] and np.array_equal(px0[0], want)
    assert ms0["long"] > ms0["spec"] + ms0["chain"] + ms0["write"]           # and here no window launches


def test_a_corrupt_multi_window_file_is_flagged_alone(engine, files):
    """one single-byte corruption of the 2-window file that the model refuses as corrupt, between two good files of its size: run
    once.  Its image is flagged, its neighbours are exact, and the engine decodes a good file afterwards."""
    good, variants = wcases.corrupted_two_window_files(40)

    def corrupt(d):
        try:
            model.coefficients(model.plan(d))
        except model.Corrupt:
            return True
        except model.Refused:
            return False
        return False
    name, bad = next((n, d) for n, d in variants if corrupt(d))
    assert engine.decode_jpeg_plan(bad) is not None, name
    other = cases.encode(cases.noise(128, 128, 31), 95, 0)
    assert _windows(bad) == 2 and _windows(other) == 2
    out, status = engine.decode_jpeg_device([good, bad, other])
    st = status.cpu().tolist()
    print(name, "status", st)
    assert st[0] == 0 and st[1] != 0 and st[2] == 0
    assert np.array_equal(out[0].cpu().numpy(), cases.pillow_pixels(good))
    assert np.array_equal(out[2].cpu().numpy(), cases.pillow_pixels(other))
    assert np.array_equal(engine.decode_jpeg(good), cases.pillow_pixels(good))
