"""Progressive JPEG results on the device (csrc/jpeg_progenc.hip: coefficient pass, count pass, table kernel, emit pass, gather) against
the model (tests/jpeg_progenc_model.py, which tests/test_jpeg_progenc_model.py holds to libjpeg-turbo's file): pixel images through the
host entry and the windowed device entry; three images in one call; every coefficient case through
ire_debug_jpeg_progressive_from_coefs; the decoded pixels, by Pillow and by the engine's own progressive decoder; the other two JPEG
paths untouched; and every job kind on an engine created with IRE_FLAG_JPEG_PROGRESSIVE."""
import base64
import ctypes
import functools
import io
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_huffopt_model as huffopt    # noqa: E402
import jpeg_opt_model as opt            # noqa: E402
import jpeg_progenc_cases as cases      # noqa: E402
import jpeg_progenc_model as model      # noqa: E402

from image_restoration_platform_amd import _lib      # noqa: E402
from image_restoration_platform_amd.engine import Engine      # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 0xA5
SIZES = [(1, 1), (5, 7), (17, 9), (45, 37), (72, 40), (136, 72), (8, 8192), (8192, 8)]
QUALITIES = [1, 85, 100]


@functools.lru_cache(maxsize=None)
def image(h, w):
    px = cases.noise(h, w, 7 * h + w)
    if h * w > 20000:       # the two long ones: noise on a ramp, so that runs, ZRLs and every category occur along 1024 blocks
        ramp = (np.add.outer(np.arange(h), np.arange(w)) // 3 % 256)[..., None]
        px = ((px.astype(np.int64) % 24) + ramp).astype(np.uint8)
    px.setflags(write=False)
    return px


@functools.lru_cache(maxsize=None)
def want_text(h, w, q, s):
    return model.jpeg_base64(image(h, w), q, s)


def _decode(text, h, w):
    """Pillow reads the file without a warning, to the declared size"""
    from PIL import Image
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        im = Image.open(io.BytesIO(base64.b64decode(text)))
        im.load()
        assert im.format == "JPEG" and im.mode == "RGB" and im.size == (w, h)
        return np.asarray(im)


def _first_difference(a, b):
    return next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))


def _same(got, want, what):
    if got != want:
        try:
            a, b = base64.b64decode(got + b"=" * (-len(got) % 4)), base64.b64decode(want)
        except Exception:
            a, b = got, want
        pytest.fail("%s: %d bytes where the model has %d; first differing byte %s" % (what, len(a), len(b), _first_difference(a, b)))


def _window(px):
    """[n][h][w][3] on the host -> the same pixels as a window of a larger device tensor: rows and images apart"""
    import torch
    n, h, w, _ = px.shape
    big = torch.full((n, h + 5, w + (7 if w % 2 == 0 else 6), 3), 0x3C, dtype=torch.uint8, device="cuda")
    big[:, :h, :w] = torch.from_numpy(np.array(px)).cuda()
    t = big[:, :h, :w]
    assert t.stride(1) % 2 == 1 and t.stride(1) > 3 * w and t.stride(0) > h * t.stride(1)
    return t


def _device_entry(eng, t, q, s, surplus=517):
    """ire_encode_jpeg_progressive_base64_fit_device of the view t into guard-filled texts -> (texts, lens) on the host"""
    import torch
    n, h, w, _ = t.shape
    stride = eng.jpeg_base64_bound(h, w, q, s, progressive=True) + surplus
    out = torch.full((n, stride), GUARD, dtype=torch.uint8, device="cuda")
    lens = torch.zeros(n, dtype=torch.int64, device="cuda")
    st = eng._lib.ire_encode_jpeg_progressive_base64_fit_device(eng._h, ctypes.c_void_p(t.data_ptr()), n, h, w, t.stride(1), t.stride(0), ctypes.c_void_p(out.data_ptr()), stride,
                                                                ctypes.c_void_p(lens.data_ptr()), q, s, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert st == _lib.IRE_OK, eng._lib.ire_last_error()
    torch.cuda.synchronize()
    return out.cpu().numpy(), lens.cpu().numpy()


@pytest.mark.parametrize("s", [0, 2])
@pytest.mark.parametrize("h,w", SIZES)
def test_device_text_equals_the_model(engine, h, w, s):
    """Through the host-pointer entry and the device entry on a window of a larger tensor (row and image pitches): the text is the
    model's, the length exact, the guard bytes behind it intact; Pillow decodes it to the pixels of the device's optimised text."""
    px = image(h, w)
    for q in QUALITIES:
        what = "%d x %d q %d s %d" % (h, w, q, s)
        want = want_text(h, w, q, s)
        assert engine.jpeg_base64_bound(h, w, q, s, progressive=True) == model.base64_bound(h, w, q, s) >= len(want), what
        _same(engine.encode_jpeg_base64_fit(px, q, s, progressive=True), want, what + " (host entry)")
        texts, lens = _device_entry(engine, _window(px[None]), q, s)
        assert int(lens[0]) == len(want), what
        _same(texts[0, :int(lens[0])].tobytes(), want, what + " (device entry, window)")
        assert (texts[0, int(lens[0]):] == GUARD).all(), what
        if h * w <= 20000:
            optimised = engine.encode_jpeg_base64_fit(px, q, s, optimize=True)
            assert np.array_equal(_decode(want, h, w), _decode(optimised, h, w)), what


def test_three_images_in_one_call_equal_three_calls(engine):
    h, w = 45, 37
    imgs = [np.full((h, w, 3), 180, np.uint8), cases.noise(h, w, 21), image(h, w)]
    for q, s in ((85, 0), (60, 2)):
        single = [engine.encode_jpeg_base64_fit(p, q, s, progressive=True) for p in imgs]
        assert single == [model.jpeg_base64(p, q, s) for p in imgs] and len(set(single)) == 3
        for order in ((0, 1, 2), (2, 0, 1)):
            texts, lens = _device_entry(engine, _window(np.stack([imgs[i] for i in order])), q, s)
            for k, i in enumerate(order):
                assert int(lens[k]) == len(single[i]), (q, s, order, k)
                _same(texts[k, :int(lens[k])].tobytes(), single[i], "image %d of %s at q %d s %d" % (k, order, q, s))
                assert (texts[k, int(lens[k]):] == GUARD).all(), (q, s, order, k)


@pytest.mark.parametrize("name", cases.NAMES)
def test_every_coefficient_case(engine, name):
    """ire_debug_jpeg_progressive_from_coefs: the count pass, the table kernel, the emit pass and the gather on exact coefficients --
    whole-interval runs, runs broken in the last block, ZRL chains, the suppressed ZRL, the early flush, the extreme categories, the
    shifts, dummy blocks, a row of 1024 blocks: the file is the model's.  Twice in one call, and behind another case's call."""
    h, w, q, s, flat = cases.case(name)
    want, _ = cases.want(name)
    got = engine.debug_jpeg_progressive_from_coefs(np.stack([flat, flat]), h, w, q, s)
    for k, f in enumerate(got):
        if f != want:
            pytest.fail("%s, image %d: %d bytes where the model has %d; first differing byte %s" % (name, k, len(f), len(want), _first_difference(f, want)))


def test_the_own_decoder_reads_the_file(engine):
    """An engine with IRE_FLAG_DECODE_PROGRESSIVE decodes the device's own progressive file to the pixels Pillow decodes it to."""
    eng = Engine(max_batch=2, flags=_lib.IRE_FLAG_DECODE_PROGRESSIVE)
    try:
        for (h, w), q, s in (((45, 37), 85, 0), ((72, 40), 60, 2), ((17, 9), 100, 2)):
            text = eng.encode_jpeg_base64_fit(image(h, w), q, s, progressive=True)
            assert text == want_text(h, w, q, s) if q in QUALITIES else True
            assert np.array_equal(eng.decode_jpeg(base64.b64decode(text)), _decode(text, h, w)), (h, w, q, s)
    finally:
        eng.close()


def test_the_other_paths_are_unchanged(engine):
    """The fixed-table and the optimised text of one image before and after the progressive path has run: the same, and the models'."""
    px = image(136, 72)
    for q, s in ((85, 0), (60, 2)):
        before = (engine.encode_jpeg_base64_fit(px, q, s, optimize=False), engine.encode_jpeg_base64_fit(px, q, s, optimize=True))
        prog = engine.encode_jpeg_base64_fit(px, q, s, progressive=True)
        after = (engine.encode_jpeg_base64_fit(px, q, s, optimize=False), engine.encode_jpeg_base64_fit(px, q, s, optimize=True))
        assert before == after == (opt.jpeg_base64(px, q, s), huffopt.jpeg_base64(px, q, s))
        assert prog == model.jpeg_base64(px, q, s) and len(prog) < len(before[0])


def _poll_text(eng, handle, cap, timeout_ms=-1):
    out = np.full(cap + 16, 0x5A, np.uint8)
    n = ctypes.c_size_t(0)
    sc = np.zeros(7, np.float64)
    st = eng._lib.ire_poll_text(eng._h, handle, timeout_ms, ctypes.c_void_p(out.ctypes.data), cap, ctypes.byref(n), ctypes.c_void_p(sc.ctypes.data), None)
    return st, out, n.value


@pytest.fixture(scope="module")
def prog_engine():
    eng = Engine(max_batch=4, flags=_lib.IRE_FLAG_RESULT_JPEG | _lib.IRE_FLAG_JPEG_PROGRESSIVE | _lib.IRE_FLAG_JPEG_OPTIMIZE, jpeg_quality=60, jpeg_sampling=2)
    yield eng
    eng.close()


def _submissions():
    import jpeg_decode_cases as dcases
    import upload_cases as uc
    from image_restoration_platform_amd import synth
    file_job = dcases.encode(dcases.smooth(40, 72, 57), 95, 2)
    upload = uc.encode(uc.smooth(97, 131, 7 + 131), 85, 2, 6, False)      # 131 x 97 stored, 4:2:0, orientation 6
    views = np.ascontiguousarray(synth.fusion_views(40, 72)[:2])
    return {"fit": lambda e: e.submit_fit(image(45, 37), is_jpeg=False), "jpeg": lambda e: e.submit_jpeg(file_job),
            "upload": lambda e: e.submit_upload(upload, max_dim=64), "fuse_fit": lambda e: e.submit_fuse_fit(views)}


@pytest.mark.parametrize("kind", ["fit", "jpeg", "upload", "fuse_fit"])
def test_a_job_on_a_progressive_engine(engine, prog_engine, kind):
    """ire_submit_fit / ire_submit_jpeg / ire_submit_upload / ire_submit_fuse_fit on an engine with IRE_FLAG_JPEG_PROGRESSIVE (and
    IRE_FLAG_JPEG_OPTIMIZE beside it, which changes nothing): ire_poll_text gives the direct entry's progressive text of the pixels
    the session's pixel engine returns for the same submission; a too-small cap_bytes reports the length needed and loses nothing."""
    submit = _submissions()[kind]
    eng, q, s = prog_engine, 60, 2
    handle, h, w = submit(eng)
    assert h <= 72 and w <= 72
    ref, ref_scores, _ = engine.poll(submit(engine), timeout_ms=120000)
    assert ref.shape == (h, w, 3)
    want = engine.encode_jpeg_base64_fit(ref, q, s, progressive=True)
    assert want == model.jpeg_base64(ref, q, s)
    bound = eng.jpeg_base64_bound(h, w)
    assert bound == model.base64_bound(h, w, q, s) >= len(want)
    st, out, n = _poll_text(eng, handle, len(want) - 1, timeout_ms=120000)
    assert st == _lib.IRE_ERR_INVALID_INPUT and n == len(want) and (out == 0x5A).all(), eng._lib.ire_last_error()
    st, out, n = _poll_text(eng, handle, bound, timeout_ms=120000)
    assert st == _lib.IRE_OK, eng._lib.ire_last_error()
    _same(out[:n].tobytes(), want, kind + " job")
    assert (out[n:] == 0x5A).all()
    text, scores, _ = eng.poll(submit(eng), timeout_ms=120000)      # the Python host's poll() sizes its buffer by the progressive bound
    assert text == want and np.array_equal(scores, ref_scores)
    assert np.array_equal(_decode(text, h, w), _decode(huffopt.jpeg_base64(ref, q, s), h, w))
