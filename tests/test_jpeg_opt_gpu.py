"""The device JPEG encoder (csrc/jpeg.hip) at a chosen quality and chroma sampling, through the C ABI: its text equals the generalised
model's (tests/jpeg_opt_model.py, which equals libjpeg-turbo's file: tests/test_jpeg_opt_model.py) byte for byte, Pillow reads every
file, the bytes do not depend on batch position, pitch or stride, nothing is written beyond ire_jpeg_base64_bound_ex, and a batcher
engine created with its own settings delivers that text through ire_poll_text for an any-size job and for a fusion job."""
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
import jpeg_opt_model as model  # noqa: E402

from image_restoration_platform_amd import _lib      # noqa: E402
from image_restoration_platform_amd.engine import Engine      # noqa: E402

pytestmark = pytest.mark.gpu

SETTINGS = [(85, 2), (50, 0), (100, 2), (1, 2), (95, 0)]
# h x w: one pixel; replication only; a dummy Y block row; a dummy Y block column; both edges ragged; several intervals with a short
# last one at either sampling (tests/test_jpeg_opt_model.py)
SHAPES = [(1, 1), (9, 9), (17, 16), (16, 17), (45, 37), (48, 203)]


def _decode(text, h, w):
    """Pillow reads the file without a warning, to the declared size"""
    from PIL import Image
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        im = Image.open(io.BytesIO(base64.b64decode(text)))
        im.load()
        assert im.format == "JPEG" and im.mode == "RGB" and im.size == (w, h)
        return np.asarray(im)


@pytest.fixture(scope="module")
def images():
    return {hw: (cases.noise if sum(hw) % 2 else cases.smooth)(hw[0], hw[1], 100 * hw[0] + hw[1]) for hw in SHAPES}


@pytest.fixture(scope="module")
def expected(images):
    """(shape, quality, sampling) -> the model's text, computed once"""
    return {(hw, q, s): model.jpeg_base64(px, q, s) for hw, px in images.items() for q, s in SETTINGS}


def test_device_text_equals_the_model(engine, images, expected):
    for q, s in SETTINGS:
        for hw, px in images.items():
            got = engine.encode_jpeg_base64_fit(px, quality=q, sampling=s)
            want = expected[(hw, q, s)]
            print("q %3d s %d %3d x %3d %6d characters (bound %d)" % (q, s, hw[0], hw[1], len(got), engine.jpeg_base64_bound(*hw, q, s)))
            assert len(got) == len(want), (hw, q, s)
            assert got == want, (hw, q, s)
            assert len(got) <= engine.jpeg_base64_bound(*hw, q, s) == model.base64_bound(*hw, q, s)
            assert _decode(got, *hw).shape == px.shape
    # the default of the _ex entries is the first entries' file
    px = images[(45, 37)]
    assert engine.encode_jpeg_base64_fit(px, quality=0, sampling=0) == engine.encode_jpeg_base64_fit(px) == model.jpeg_base64(px, 85, 0)
    for q, s in ((101, 0), (-1, 2), (85, 1), (85, 3)):
        out = np.zeros(1 << 16, np.uint8)
        lens = np.zeros(1, np.uint64)
        st = engine._lib.ire_encode_jpeg_base64_fit_ex(engine._h, ctypes.c_void_p(px.ctypes.data), 1, 45, 37, ctypes.c_void_p(out.ctypes.data), out.size,
                                                       ctypes.c_void_p(lens.ctypes.data), q, s)
        assert st == _lib.IRE_ERR_INVALID_INPUT and b"invalid" in engine._lib.ire_last_error(), (q, s)


def _encode_tensor(engine, t, stride, q, s, fill=0):
    """raw ire_encode_jpeg_base64_fit_device_ex on a [n][h][w][3] view `t`; -> (texts [n][stride] uint8 on the host, lens)"""
    import torch
    n, h, w, _ = t.shape
    si, sr, _, _ = t.stride()
    out = torch.full((n, stride), fill, dtype=torch.uint8, device="cuda")
    lens = torch.zeros(n, dtype=torch.int64, device="cuda")
    st = engine._lib.ire_encode_jpeg_base64_fit_device_ex(engine._h, ctypes.c_void_p(t.data_ptr()), n, h, w, sr, si, ctypes.c_void_p(out.data_ptr()), stride,
                                                          ctypes.c_void_p(lens.data_ptr()), q, s, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == _lib.IRE_OK, engine._lib.ire_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy(), lens.cpu().numpy()


def test_bytes_do_not_depend_on_batch_position_pitch_or_stride(engine):
    import torch
    h, w = 45, 37
    px = np.stack([cases.smooth(h, w, 41), cases.noise(h, w, 42), cases.smooth(h, w, 43)[::-1].copy()])
    big = torch.full((3, h + 9, w + 13, 3), 255, dtype=torch.uint8, device="cuda")       # row pitch > 3 w (and odd: unaligned rows), image pitch > h * pitch
    big[:, :h, :w] = torch.from_numpy(px).cuda()
    for q, s in ((85, 2), (95, 0)):
        want = [model.jpeg_base64(p, q, s) for p in px]
        stride = engine.jpeg_base64_bound(h, w, q, s) + 333                              # larger than needed, and no multiple of 4
        texts, lens = _encode_tensor(engine, big[:, :h, :w], stride, q, s)
        for i in range(3):
            t1, l1 = _encode_tensor(engine, torch.from_numpy(px[i:i + 1]).cuda().contiguous(), stride, q, s)
            assert int(lens[i]) == int(l1[0]) == len(want[i]), (q, s, i)
            assert texts[i, :lens[i]].tobytes() == t1[0, :l1[0]].tobytes() == want[i], (q, s, i)
        # the same image at every position of a batch gives the same bytes
        same = torch.from_numpy(np.stack([px[1]] * 3)).cuda()
        texts, lens = _encode_tensor(engine, same, stride, q, s)
        assert all(texts[i, :lens[i]].tobytes() == want[1] for i in range(3)), (q, s)
        # the tensor form of the Python host: the same window
        tx, ln = engine.encode_jpeg_base64_fit_tensor(big[:, :h, :w], quality=q, sampling=s)
        tx, ln = tx.cpu().numpy(), ln.cpu().numpy()
        assert [tx[i, :ln[i]].tobytes() for i in range(3)] == want


def test_nothing_is_written_beyond_the_bound(engine):
    import torch
    px = cases.noise(24, 136, 16)                             # full-scale noise: the longest texts; wraps intervals across MCU rows
    for q, s in ((100, 2), (100, 0)):
        want = model.jpeg_base64(px, q, s)
        bound = engine.jpeg_base64_bound(24, 136, q, s)
        stride = bound + 517                                  # no multiple of 4 either: the byte-wise text path
        t = torch.from_numpy(np.stack([px, px])).cuda()
        texts, lens = _encode_tensor(engine, t, stride, q, s, fill=0xA5)
        for i in range(2):
            assert texts[i, :lens[i]].tobytes() == want, (q, s)
            assert (texts[i, bound:] == 0xA5).all(), (q, s)       # the guard bytes between the bound and the stride
            assert (texts[i, lens[i]:bound] == 0xA5).all()      # (and nothing behind the text's own end)
        # a stride one below this setting's bound is refused
        out = torch.zeros(2 * stride, dtype=torch.uint8, device="cuda")
        lens = torch.zeros(2, dtype=torch.int64, device="cuda")
        st = engine._lib.ire_encode_jpeg_base64_fit_device_ex(engine._h, ctypes.c_void_p(t.data_ptr()), 2, 24, 136, 3 * 136, 3 * 136 * 24, ctypes.c_void_p(out.data_ptr()),
                                                              bound - 1, ctypes.c_void_p(lens.data_ptr()), q, s, None)
        assert st == _lib.IRE_ERR_INVALID_INPUT and b"invalid" in engine._lib.ire_last_error()


def test_batcher_engine_with_its_own_settings(engine):
    """An engine created with jpeg_quality=60, jpeg_sampling=2 delivers through ire_poll_text the model's text of the restored pixels
    (those from a pixel engine on the same input): one any-size job and one fusion job, at 40 x 56."""
    h, w, q, s = 40, 56, 60, 2
    eng = Engine(max_batch=4, flags=_lib.IRE_FLAG_RESULT_JPEG, jpeg_quality=q, jpeg_sampling=s)
    try:
        assert eng.jpeg_base64_bound(h, w) == model.base64_bound(h, w, q, s) != model.base64_bound(h, w, 85, 0)
        px = cases.smooth(h, w, 51)
        views = [px, cases.smooth(h, w, 52), cases.smooth(h, w, 53)]
        jobs = {"any-size": (lambda e: e.submit_fit(px, is_jpeg=False)), "fusion": (lambda e: e.submit_fuse_fit(views, is_jpeg=False))}
        for name, submit in jobs.items():
            ref = engine.poll(submit(engine))[0]
            assert ref.shape == (h, w, 3), name
            want = model.jpeg_base64(ref, q, s)
            handle, _, _ = submit(eng)
            cap = eng.jpeg_base64_bound(h, w)
            out = np.full(cap + 16, 0x5A, np.uint8)
            n = ctypes.c_size_t(0)
            sc = np.zeros(7, np.float64)
            st = eng._lib.ire_poll_text(eng._h, handle, -1, ctypes.c_void_p(out.ctypes.data), cap, ctypes.byref(n), ctypes.c_void_p(sc.ctypes.data), None)
            assert st == _lib.IRE_OK, eng._lib.ire_last_error()
            assert n.value == len(want) and out[:n.value].tobytes() == want and (out[n.value:] == 0x5A).all(), name
            assert _decode(want, h, w).shape == ref.shape
            assert eng.poll(submit(eng))[0] == want, name       # the Python host's poll() sizes its buffer from the engine's settings
    finally:
        eng.close()
