"""The device JPEG encoder (csrc/jpeg.hip) on the cases of tests/jpeg_opt_cases.py: the symbols only quality 100 reaches, chains of ZRL
codes in either table, dummy blocks behind a full DC swing, both sides of the size-class switch, and every job kind on an engine with
its own settings.  Every expected text is the model's (tests/jpeg_opt_model.py, which equals libjpeg-turbo's file on these cases:
tests/test_jpeg_opt_cases.py); every comparison is byte equality.  The conditions the cases exist for are asserted from the model
before the first call (the `ready` fixture)."""
import base64
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_decode_cases as dcases      # noqa: E402
import jpeg_opt_cases as oc             # noqa: E402
import jpeg_opt_model as model          # noqa: E402
from test_jpeg_opt_gpu import _decode   # noqa: E402

from image_restoration_platform_amd import _lib      # noqa: E402
from image_restoration_platform_amd.engine import Engine      # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 0xA5


@pytest.fixture(scope="module")
def ready():
    return oc.assert_conditions()


def _where(name, shape, q, s, got):
    """the first byte in which the text `got` differs from the model's, as (file offset, interval, offset inside the interval); interval
    -1 is the file's head"""
    want = oc.encoded(name, shape, q, s)[0]
    pad = b"=" * (-len(got) % 4)
    try:
        data = base64.b64decode(got + pad)
    except Exception:
        data = b""
    at = next((i for i, (a, b) in enumerate(zip(data, want)) if a != b), min(len(data), len(want)))
    start = model.HEADER_BYTES
    if at < start:
        return at, -1, at
    for k, (_, _, raw, ff, _) in enumerate(oc.encoded(name, shape, q, s)[1]["intervals"]):
        if at < start + raw + ff + 2:
            return at, k, at - start
        start += raw + ff + 2
    return at, None, None


def _window(px):
    """[n][h][w][3] on the host -> the same pixels as a window of a larger device tensor: an odd row pitch, rows and images apart"""
    import torch
    n, h, w, _ = px.shape
    big = torch.full((n, h + 5, w + (7 if w % 2 == 0 else 6), 3), 0x3C, dtype=torch.uint8, device="cuda")
    big[:, :h, :w] = torch.from_numpy(px).cuda()
    t = big[:, :h, :w]
    assert t.stride(1) % 2 == 1 and t.stride(1) > 3 * w and t.stride(0) > h * t.stride(1)
    return t


def _enqueue(eng, t, stride, q, s, stream):
    """ire_encode_jpeg_base64_fit_device_ex of the view `t` into fresh guard-filled texts, on `stream`, without a synchronisation"""
    import torch
    n, h, w, _ = t.shape
    out = torch.full((n, stride), GUARD, dtype=torch.uint8, device="cuda")
    lens = torch.zeros(n, dtype=torch.int64, device="cuda")
    st = eng._lib.ire_encode_jpeg_base64_fit_device_ex(eng._h, ctypes.c_void_p(t.data_ptr()), n, h, w, t.stride(1), t.stride(0), ctypes.c_void_p(out.data_ptr()), stride,
                                                       ctypes.c_void_p(lens.data_ptr()), q, s, ctypes.c_void_p(stream.cuda_stream))
    assert st == _lib.IRE_OK, eng._lib.ire_last_error()
    return out, lens


def _check_batch(shape, names, q, s, texts, lens, what):
    for i, name in enumerate(names):
        want = oc.text(name, shape, q, s)
        n = int(lens[i])
        got = texts[i, :max(n, 0)].tobytes()
        if n != len(want) or got != want:
            pytest.fail("%s: case %s, %d x %d, quality %d, sampling %d, image %d: %d characters where the model has %d; the first differing file byte, its interval and the "
                        "offset in it: %s" % (what, name, shape[0], shape[1], q, s, i, n, len(want), _where(name, shape, q, s, got)))
        assert (texts[i, n:] == GUARD).all(), (what, name, shape, q, s, i)      # nothing between the text's end and the stride


@pytest.mark.parametrize("shape", oc.SHAPES, ids=lambda hw: "%dx%d" % hw)
def test_device_text_equals_the_model_on_every_case_at_every_setting(engine, ready, shape):
    """The shape's cases in one call, the content differing per image, as a window of a larger tensor with an odd row pitch; the stride is
    the bound plus an odd surplus of guard bytes.  Text and length equal the model's per image, nothing is written behind a text, the same
    batch in reverse order gives the same bytes per image, and Pillow reads every file without a warning."""
    import torch
    names = oc.BATCHES[shape]
    px = oc.batch(shape)
    fwd, rev = _window(px), _window(np.ascontiguousarray(px[::-1]))
    for q, s in oc.SETTINGS:
        bound = engine.jpeg_base64_bound(*shape, q, s)
        assert bound == model.base64_bound(*shape, q, s)
        stride = bound + 517
        for what, t, order in (("in order", fwd, names), ("reversed", rev, names[::-1])):
            out, lens = _enqueue(engine, t, stride, q, s, torch.cuda.current_stream())
            torch.cuda.synchronize()
            _check_batch(shape, order, q, s, out.cpu().numpy(), lens.cpu().numpy(), what)
        for name in names:                      # (the device's text is the model's by now)
            assert _decode(oc.text(name, shape, q, s), *shape).shape == (shape[0], shape[1], 3), (name, shape, q, s)
        sizes = [len(oc.text(name, shape, q, s)) for name in names]
        print("%3d x %3d q %3d s %d: %d .. %d characters (bound %d)" % (shape[0], shape[1], q, s, min(sizes), max(sizes), bound))


def test_settings_in_turn_on_one_stream_with_one_synchronisation(ready):
    """A fresh engine and a stream of the test's own: the (41, 139) batch at eight settings in turn into separate outputs, one
    synchronisation at the end.  The first call sizes the engine's scratch for the small class, the second outgrows it, the later ones
    alternate between the classes and the samplings inside the grown buffer."""
    import torch
    shape = (41, 139)
    order = [(1, 0), (100, 2), (86, 0), (87, 0), (85, 2), (86, 2), (100, 0), (1, 0)]
    assert [oc.big_class(q, s) for q, s in order] == [False, True, False, True, False, True, True, False]
    eng = Engine(max_batch=8)
    try:
        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            t = _window(oc.batch(shape))
            runs = [_enqueue(eng, t, eng.jpeg_base64_bound(*shape, q, s) + 517, q, s, stream) for q, s in order]
        stream.synchronize()
        for k, ((q, s), (out, lens)) in enumerate(zip(order, runs)):
            _check_batch(shape, oc.BATCHES[shape], q, s, out.cpu().numpy(), lens.cpu().numpy(), "call %d of the sequence" % k)
    finally:
        eng.close()


def test_every_job_kind_on_an_engine_with_its_own_settings(engine):
    """Engine(flags=IRE_FLAG_RESULT_JPEG, jpeg_quality=92, jpeg_sampling=2), the big class at 4:2:0: a file job, an upload job, three
    uploads of one key submitted before the first poll and an any-size job.  Each polled text is the model's text at (92, 2) of the
    PIXELS the session's pixel engine returns for the same submission -- not another text of the same encoder -- and the scores are equal."""
    from test_submit_upload_gpu import _file
    q, s = 92, 2
    assert oc.big_class(q, s)
    file_job = dcases.encode(dcases.smooth(48, 64, 57), 95, 2)          # 64 x 48, 4:2:0
    upload = _file(131, 97, "420", 6)                                    # turned upright and fitted inside 128: 95 x 70 (h x w)
    px = oc.pixels("cells2", (33, 130))
    eng = Engine(max_batch=4, flags=_lib.IRE_FLAG_RESULT_JPEG, jpeg_quality=q, jpeg_sampling=s)
    try:
        submissions = [("file job", lambda e: e.submit_jpeg(file_job)), ("upload job", lambda e: e.submit_upload(upload, max_dim=128)),
                       ("any-size job", lambda e: e.submit_fit(px, is_jpeg=False))]
        submissions[2:2] = [("upload %d of three of one key" % k, lambda e: e.submit_upload(upload, max_dim=128)) for k in range(3)]
        jobs = [submit(eng) for _, submit in submissions]              # all six before the first poll
        assert (jobs[1][1], jobs[1][2]) == (95, 70) and (jobs[0][1], jobs[0][2]) == (48, 64) and (jobs[-1][1], jobs[-1][2]) == (33, 130)
        got = [eng.poll(j) for j in jobs]
        for (what, submit), job, (text, scores, _) in zip(submissions, jobs, got):
            ref, ref_scores, _ = engine.poll(submit(engine))
            h, w = job[1], job[2]
            assert isinstance(text, bytes) and ref.shape == (h, w, 3), what
            want = model.jpeg_base64(ref, q, s)
            assert len(text) == len(want) <= eng.jpeg_base64_bound(h, w) == model.base64_bound(h, w, q, s), what
            assert text == want, (what, next(i for i in range(len(want)) if text[i] != want[i]))
            assert np.array_equal(scores, ref_scores), what
            assert _decode(text, h, w).shape == ref.shape
    finally:
        eng.close()
