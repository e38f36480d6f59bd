"""The JPEG encoder on the device (csrc/jpeg.hip) through the C ABI: its text equals the Python model's (tests/jpeg_model.py, which
equals libjpeg-turbo's file: tests/test_jpeg_model.py) byte for byte, an independent decoder reads it, the bytes do not depend on
batch, position, pitch or stream, nothing is written beyond the bound, and the batcher delivers the text through ire_poll_text."""
import base64
import ctypes
import io
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_cases as cases      # noqa: E402
import jpeg_model as model      # noqa: E402

from image_restoration_platform_amd import _lib      # noqa: E402
from image_restoration_platform_amd.engine import Engine      # noqa: E402

pytestmark = pytest.mark.gpu


def _decode(text):
    from PIL import Image
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        im = Image.open(io.BytesIO(base64.b64decode(text)))
        assert im.format == "JPEG"
        return np.asarray(im.convert("RGB"))


@pytest.fixture(scope="module")
def images():
    return cases.all_cases()


@pytest.fixture(scope="module")
def expected(images):
    """name -> the model's text, computed once"""
    return {k: model.jpeg_base64(px) for k, px in images.items()}


def test_device_text_equals_the_model(engine, images, expected):
    for name, px in images.items():
        got = engine.encode_jpeg_base64_fit(px)
        print("%-14s %7d characters (bound %d)" % (name, len(got), engine.jpeg_base64_bound(*px.shape[:2])))
        assert len(got) == len(expected[name]), name
        assert got == expected[name], name
        assert _decode(got).shape == px.shape, name          # an independent decoder reads the device's own text


def _encode_tensor(engine, t, stride, stream=None, fill=None):
    """raw ire_encode_jpeg_base64_fit_device on a [n][h][w][3] view `t`; -> (texts [n][stride] uint8 on the host, lens)"""
    import torch
    n, h, w, _ = t.shape
    si, sr, _, _ = t.stride()
    out = torch.full((n, stride), 0 if fill is None else fill, dtype=torch.uint8, device="cuda")
    lens = torch.zeros(n, dtype=torch.int64, device="cuda")
    s = stream if stream is not None else torch.cuda.current_stream()
    s.wait_stream(torch.cuda.current_stream())               # the inputs were written on the current stream
    st = engine._lib.ire_encode_jpeg_base64_fit_device(engine._h, ctypes.c_void_p(t.data_ptr()), n, h, w, sr, si, ctypes.c_void_p(out.data_ptr()), stride,
                                                       ctypes.c_void_p(lens.data_ptr()), ctypes.c_void_p(s.cuda_stream))
    assert st == _lib.IRE_OK, engine._lib.ire_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy(), lens.cpu().numpy()


def test_bytes_do_not_depend_on_batch_position_pitch_or_stream(engine):
    import torch
    h, w = 72, 88
    px = np.stack([cases.smooth(h, w, 31), cases.noise(h, w, 32), cases.smooth(h, w, 33)[::-1].copy()])
    want = [model.jpeg_base64(p) for p in px]
    big = torch.full((3, h + 9, w + 13, 3), 255, dtype=torch.uint8, device="cuda")       # row pitch > 3 w (and odd: unaligned rows), image pitch > h * pitch
    big[:, :h, :w] = torch.from_numpy(px).cuda()
    bound = engine.jpeg_base64_bound(h, w)
    stride = (bound + 3) // 4 * 4
    for stream in (None, torch.cuda.Stream()):
        texts, lens = _encode_tensor(engine, big[:, :h, :w], stride, stream)
        for i in range(3):
            dense = torch.from_numpy(px[i:i + 1]).cuda().contiguous()
            t1, l1 = _encode_tensor(engine, dense, stride, stream)
            assert int(lens[i]) == int(l1[0]) == len(want[i])
            assert texts[i, :lens[i]].tobytes() == t1[0, :l1[0]].tobytes() == want[i], (i, stream)
    # the tensor form of the Python host: the same window
    tx, ln = engine.encode_jpeg_base64_fit_tensor(big[:, :h, :w])
    tx, ln = tx.cpu().numpy(), ln.cpu().numpy()
    assert [tx[i, :ln[i]].tobytes() for i in range(3)] == want


def test_nothing_is_written_beyond_the_bound(engine, images, expected):
    import torch
    for name in ("wrap24x136", "mod3_1", "saturated"):
        px = images[name]
        bound = engine.jpeg_base64_bound(*px.shape[:2])
        stride = bound + 517                                  # no multiple of 4 either: the byte-wise text path
        t = torch.from_numpy(np.stack([px, px])).cuda()
        texts, lens = _encode_tensor(engine, t, stride, fill=0xA5)
        for i in range(2):
            assert texts[i, :lens[i]].tobytes() == expected[name]
            assert (texts[i, bound:] == 0xA5).all(), name       # the guard bytes between the bound and the stride
            assert (texts[i, lens[i]:bound] == 0xA5).all()      # (and nothing behind the text's own end)
    # a stride one below the bound is refused
    t = torch.from_numpy(images["7x5"][None]).cuda()
    out = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    lens = torch.zeros(1, dtype=torch.int64, device="cuda")
    st = engine._lib.ire_encode_jpeg_base64_fit_device(engine._h, ctypes.c_void_p(t.data_ptr()), 1, 7, 5, 15, 105, ctypes.c_void_p(out.data_ptr()),
                                                       engine.jpeg_base64_bound(7, 5) - 1, ctypes.c_void_p(lens.data_ptr()), None)
    assert st == _lib.IRE_ERR_INVALID_INPUT and b"invalid" in engine._lib.ire_last_error()


def _poll_text(eng, handle, cap, timeout_ms=-1):
    out = np.full(cap + 16, 0x5A, np.uint8)
    n = ctypes.c_size_t(0)
    sc = np.zeros(7, np.float64)
    st = eng._lib.ire_poll_text(eng._h, handle, timeout_ms, ctypes.c_void_p(out.ctypes.data), cap, ctypes.byref(n), ctypes.c_void_p(sc.ctypes.data), None)
    return st, out, n.value, sc


def test_batcher_delivers_the_jpeg_text(engine):
    eng = Engine(max_batch=4, flags=_lib.IRE_FLAG_RESULT_JPEG)
    try:
        for h, w in ((50, 37), (64, 64)):                       # a ragged job (ire_submit_fit pads on the device) and an aligned one
            px = cases.smooth(h, w, h + w)
            ref = engine.restore_fit(px[None], is_jpeg=False)[0]
            want = model.jpeg_base64(ref)
            bound = eng.jpeg_base64_bound(h, w)
            handle, _, _ = eng.submit_fit(px, is_jpeg=False)
            # ire_poll has nowhere to report a length: invalid, and the job is still there
            buf = np.zeros(bound, np.uint8)
            assert eng._lib.ire_poll(eng._h, handle, -1, ctypes.c_void_p(buf.ctypes.data), None, None) == _lib.IRE_ERR_INVALID_INPUT
            assert b"ire_poll_text" in eng._lib.ire_last_error()
            # a buffer one short of the text: invalid, the length needed is reported, nothing is written or lost
            st, out, n, _ = _poll_text(eng, handle, len(want) - 1)
            assert st == _lib.IRE_ERR_INVALID_INPUT and n == len(want) and (out == 0x5A).all()
            st, out, n, sc = _poll_text(eng, handle, bound)
            assert st == _lib.IRE_OK, eng._lib.ire_last_error()
            assert n == len(want) and out[:n].tobytes() == want and (out[n:] == 0x5A).all()
            assert _decode(out[:n].tobytes()).shape == ref.shape
            # the Python host's poll() goes the same way
            text, _, _ = eng.poll(eng.submit_fit(px, is_jpeg=False))
            assert text == want
    finally:
        eng.close()


def test_restorer_with_the_new_codec_value(engine):
    from PIL import Image
    from image_restoration_platform_amd.restorator import EngineRestorer
    px = cases.smooth(45, 70, 3)
    bio = io.BytesIO()
    Image.fromarray(px, "RGB").save(bio, format="PNG")
    ref = engine.restore_fit(px[None], is_jpeg=False)[0]
    eng = Engine(max_batch=4, flags=_lib.IRE_FLAG_RESULT_JPEG)
    try:
        text = EngineRestorer(eng, result_codec="jpeg-device").restore_image("restore", [bio.getvalue()])["base64Image"]
        assert text.encode("ascii") == model.jpeg_base64(ref)
    finally:
        eng.close()
    # on an unflagged engine the codec value encodes the polled pixels with the same encoder
    text2 = EngineRestorer(engine, result_codec="jpeg-device").restore_image("restore", [bio.getvalue()])["base64Image"]
    assert text2 == text
