"""Progressive JPEG files on the device (csrc/jpeg_dec.hip behind csrc/jpeg_parse.hpp's file entry) through the C ABI, on an engine
created with IRE_FLAG_DECODE_PROGRESSIVE: the pixels equal Pillow's byte for byte on Pillow's own files and on the scripts the
test-side writer stands in for, at the smallest shapes at which each kernel can go wrong and at the sizes where the code takes
another path (a first scan of several windows, EOB runs longer than a lane's subsequence, a refinement stream longer than the walk's
staging); a mixed batch equals the single calls; corrupt data fails alone; the plan refuses what breaks the progression rules."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_decode_cases as cases      # noqa: E402
import jpeg_prog_cases as prog         # noqa: E402
import jpeg_prog_model as model        # noqa: E402
import jpeg_prog_writer as writer      # noqa: E402

from image_restoration_platform_amd import _lib      # noqa: E402
from image_restoration_platform_amd.engine import Engine, EngineError      # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def peng():
    eng = Engine(device_index=0, max_batch=8, weights_path=None, flags=_lib.IRE_FLAG_DECODE_PROGRESSIVE)
    yield eng
    eng.close()


def _consts():
    src = open(os.path.join(ROOT, "image_restoration_platform_amd", "csrc", "jpeg_dec_core.hpp")).read()
    lanes = int(re.search(r"constexpr int kLanes = (\d+);", src).group(1))
    bits = int(re.search(r"constexpr int kSubseqBits = (\d+);", src).group(1))
    short = int(re.search(r"constexpr unsigned kShortMaxBytes = (\d+);", src).group(1))
    walk_words = int(re.search(r"constexpr unsigned kWalkWords = (\d+);", src).group(1))
    return lanes * bits, short, walk_words


def _small_files():
    """name -> (progressive bytes, the bytes whose Pillow pixels it must give)"""
    d = {}
    for name, px, sub in (("8x8_s0", cases.noise(8, 8, 1), 0), ("17x13_s2", cases.noise(13, 17, 2), 2), ("17x13_s1", cases.noise(13, 17, 3), 1),
                          ("33x47_s2", cases.noise(47, 33, 4), 2), ("33x47_s1", cases.smooth(47, 33, 5), 1), ("5x1_s2", cases.noise(1, 5, 6), 2),
                          ("35x9_s1", cases.noise(9, 35, 7), 1), ("33x47_s2_rst3", cases.noise(47, 33, 8), 2)):
        f = writer.pillow_progressive(px, 85, sub, **({"restart_marker_blocks": 3} if name.endswith("rst3") else {}))
        d["pillow_" + name] = (f, f)
    g = writer.pillow_progressive(cases.noise(13, 17, 9)[:, :, 0], 85)
    d["pillow_17x13_grey"] = (g, g)
    q = writer.pillow_progressive(cases.noise(47, 33, 10), 100, 0)
    d["pillow_33x47_q100"] = (q, q)
    for name, v in prog.writer_cases().items():
        if not name.startswith("simple_"):                 # scripts 2 - 5 (script 1 is Pillow's own, above)
            d["writer_" + name] = v
    return d


def test_device_equals_pillow_on_small_files(peng):
    files = _small_files()
    assert len(files) == 10 + 5 * 12
    for name, (data, src) in files.items():
        want = cases.pillow_pixels(src)
        plan = peng.decode_jpeg_plan(data)
        assert plan is not None and plan[:2] == want.shape[:2], (name, plan, getattr(peng, "last_plan_reason", None))
        got = peng.decode_jpeg(data)
        bad = int((got != want).sum())
        if bad:
            print("%-34s %6d bytes  differing bytes %d" % (name, len(data), bad))
        assert got.shape == want.shape and bad == 0, name


def test_first_scans_of_several_windows(peng, monkeypatch):
    """the largest first scan of each file has at least 2.5 windows (sized from kWindowBits); the same pixels with the window-parallel
    path switched off (IRE_JPEG_DEC_WINDOWS=0, an engine of its own)"""
    window_bits, short, _ = _consts()
    files = prog.multi_window_files(window_bits)
    assert len(files) == 2
    monkeypatch.setenv("IRE_JPEG_DEC_WINDOWS", "0")
    serial = Engine(device_index=0, max_batch=8, weights_path=None, flags=_lib.IRE_FLAG_DECODE_PROGRESSIVE)
    try:
        for name, data in files.items():
            longest = prog.largest_stream(data, (model.DC_FIRST, model.AC_FIRST))
            assert 8 * longest >= 2.5 * window_bits and longest > short, name
            want = cases.pillow_pixels(data)
            print("%s: %d bytes, largest first scan %d bytes = %.2f windows" % (name, len(data), longest, 8 * longest / window_bits))
            assert np.array_equal(peng.decode_jpeg(data), want), name
            assert np.array_equal(serial.decode_jpeg(data), want), name
    finally:
        serial.close()


def test_flat_image_eob_runs_only(peng):
    data = prog.flat_file()
    assert peng.decode_jpeg_plan(data) == (1032, 1024, 3)
    assert np.array_equal(peng.decode_jpeg(data), cases.pillow_pixels(data))


def test_a_refinement_stream_longer_than_the_walks_staging(peng):
    _, short, walk_words = _consts()
    data = prog.long_refinement_file()
    longest = prog.largest_stream(data, (model.AC_REFINE,))
    assert longest > short and longest > 8 * 4 * walk_words
    assert np.array_equal(peng.decode_jpeg(data), cases.pillow_pixels(data))


def test_a_mixed_batch_equals_the_single_calls_and_stays_inside_its_images(peng):
    import torch
    h, w = 47, 33
    src = cases.encode(cases.smooth(h, w, 22), 95, 1)
    files = [writer.pillow_progressive(cases.noise(h, w, 21), 85, 2), writer.from_baseline(src, writer.script_moz()), cases.encode(cases.noise(h, w, 23)[:, :, 0], 85, restart_marker_blocks=2)]
    refs = [files[0], src, files[2]]
    singles = [peng.decode_jpeg(f) for f in files]
    ib, pitch = h * w * 3, h * w * 3 + 52
    buf = torch.full((3 * pitch + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    status = torch.full((3,), -1, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    ptrs = (ctypes.c_char_p * 3)(*files)
    lens = (ctypes.c_size_t * 3)(*[len(f) for f in files])
    rc = peng._lib.ire_decode_jpeg_device(peng._h, ptrs, lens, 3, h, w, ctypes.c_void_p(buf.data_ptr()), pitch, ctypes.c_void_p(status.data_ptr()),
                                          ctypes.c_void_p(s.cuda_stream))
    assert rc == _lib.IRE_OK, peng._lib.ire_last_error()
    s.synchronize()
    out = buf.cpu().numpy()
    assert status.cpu().tolist() == [0, 0, 0]
    for i in range(3):
        assert np.array_equal(out[i * pitch:i * pitch + ib].reshape(h, w, 3), singles[i]), i
        assert np.array_equal(singles[i], cases.pillow_pixels(refs[i])), i
        assert (out[i * pitch + ib:(i + 1) * pitch] == 0xA5).all(), i          # the guard bytes between the images
    assert (out[3 * pitch:] == 0xA5).all()                                      # and behind the last


def test_decoded_pixels_feed_the_classifier_on_the_same_stream(peng):
    import torch
    data = writer.pillow_progressive(cases.smooth(48, 64, 31), 85, 2)
    s = torch.cuda.Stream()
    px, status = peng.decode_jpeg_device([data], stream=s)
    jp = torch.ones(1, dtype=torch.uint8, device="cuda")
    s.wait_stream(torch.cuda.current_stream())
    scores = torch.zeros((1, 7), dtype=torch.float64, device="cuda")
    labels = torch.zeros(1, dtype=torch.int32, device="cuda")
    rc = peng._lib.ire_classify_device(peng._h, ctypes.c_void_p(px.data_ptr()), 1, 48, 64, ctypes.c_void_p(jp.data_ptr()), ctypes.c_void_p(scores.data_ptr()),
                                       ctypes.c_void_p(labels.data_ptr()), ctypes.c_void_p(s.cuda_stream))
    assert rc == _lib.IRE_OK, peng._lib.ire_last_error()
    s.synchronize()
    want, _ = peng.classify(cases.pillow_pixels(data), is_jpeg=True)
    assert int(status[0]) == 0
    assert np.array_equal(scores.cpu().numpy(), want)


def _model_flags(data):
    try:
        model.coefficients(model.plan(data))
    except model.Corrupt:
        return True
    except model.Refused:
        return False
    return False


def test_a_corrupt_refinement_scan_is_refused_and_the_engine_stays_usable(peng):
    """one single-byte corruption inside the last scan (an AC refinement), the first of the seeded candidates that the model flags;
    tests/test_jpeg_prog_native.py runs all candidates through the CPU build of the same code under the sanitizers and finds the same
    verdicts.  Run once."""
    good, variants = prog.corrupt_refinement_candidates()
    name, data = next((n, d) for n, d in variants if _model_flags(d))
    assert peng.decode_jpeg_plan(data) is not None, name
    with pytest.raises(EngineError) as e:
        peng.decode_jpeg(data)
    assert e.value.status == _lib.IRE_ERR_INVALID_INPUT and "invalid: corrupt JPEG data" in e.value.message
    assert np.array_equal(peng.decode_jpeg(good), cases.pillow_pixels(good))


def _plan_ex(lib, data, accept):
    h, w, s, k = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    rc = lib.ire_decode_jpeg_plan_ex(data, len(data), accept, ctypes.byref(h), ctypes.byref(w), ctypes.byref(s), ctypes.byref(k))
    return rc, (h.value, w.value, s.value, k.value), (lib.ire_last_error() or b"").decode()


def test_the_plan_refuses_what_breaks_the_progression(peng):
    lib = peng._lib
    files = prog.refused_cases()
    assert len(files) == 7
    for name, (data, word) in files.items():
        rc, _, why = _plan_ex(lib, data, _lib.IRE_DECODE_ACCEPT_PROGRESSIVE)
        with pytest.raises(model.Refused) as e:
            model.plan(data)
        assert rc == _lib.IRE_ERR_INVALID_INPUT and why == "invalid: " + e.value.reason and word in why, (name, why)
        assert peng.decode_jpeg_plan(data) is None
    # accepted: Pillow's 10 scans, the cap's 64, a baseline file's one
    good = writer.pillow_progressive(cases.noise(13, 17, 5), 85, 2)
    assert _plan_ex(lib, good, 1)[:2] == (_lib.IRE_OK, (13, 17, 2, 10))
    assert _plan_ex(lib, prog.cap_scans_file()[0], 1)[:2] == (_lib.IRE_OK, (13, 17, 3, _lib.IRE_DECODE_MAX_SCANS))
    base = cases.encode(cases.noise(13, 17, 5), 85, 1)
    assert _plan_ex(lib, base, 1)[:2] == (_lib.IRE_OK, (13, 17, 1, 1)) and _plan_ex(lib, base, 0)[:2] == (_lib.IRE_OK, (13, 17, 1, 1))
    # accept == 0 is ire_decode_jpeg_plan: status and text
    n = 0
    for name, (data, word) in list(cases.refused_cases().items()) + [("prog", (good, "progressive JPEG (SOF2)"))]:
        rc0 = lib.ire_decode_jpeg_plan(data, len(data), None, None, None)
        why0 = (lib.ire_last_error() or b"").decode()
        rc, _, why = _plan_ex(lib, data, 0)
        assert rc == rc0 == _lib.IRE_ERR_INVALID_INPUT and why == why0 and word in why, name
        n += 1
    assert n == 5
    assert _plan_ex(lib, good, 2)[0] == _lib.IRE_ERR_INVALID_INPUT          # an unknown accept bit


def test_the_upload_switch_takes_the_device_for_a_progressive_file(peng, monkeypatch):
    from image_restoration_platform_amd import restorator
    data = writer.pillow_progressive(cases.smooth(45, 70, 3), 85, 2)
    monkeypatch.delenv("IRE_UPLOAD_CODEC", raising=False)
    ref, fmt = restorator.decode_image(data, peng)
    monkeypatch.setenv("IRE_UPLOAD_CODEC", "jpeg-device")
    before = dict(restorator.UPLOAD_DECODES)
    got, fmt2 = restorator.decode_image(data, peng)
    assert restorator.UPLOAD_DECODES["device"] == before["device"] + 1 and restorator.UPLOAD_DECODES["host"] == before["host"]
    assert fmt == fmt2 == "jpeg" and got.dtype == ref.dtype and np.array_equal(got, ref)
