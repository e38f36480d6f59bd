"""The PNG forms of IRE_FLAG_DECODE_PNG_ALL on the device (csrc/png_dec.hip's png_unfilter_any_kernel behind csrc/png_parse.hpp), through
the C ABI: 1, 2, 4 and 16 bits per sample and Adam7 decode to Pillow's pixels byte for byte on every case of tests/png_depth_cases.py
(tests/test_png_depths_native.py puts the same files through the CPU form of the kernel under ASan and UBSan first); a batch that mixes
old and new forms equals the single decodes and touches nothing outside its images; uploads of the new forms equal the same pixels
uploaded as an 8-bit file; a filter byte of 5 on a pass's first row is flagged alone; an engine with IRE_FLAG_DECODE_PNG only refuses
every one of these files with the reason it always gave."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_cases as old_cases      # noqa: E402
import png_depth_cases as cases    # noqa: E402
import png_writer as pw            # noqa: E402

from image_restoration_platform_amd import _lib      # noqa: E402
from image_restoration_platform_amd.engine import Engine, EngineError, upload_plan_reason      # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def all_engine():
    eng = Engine(device_index=0, max_batch=8, num_streams=1, flags=_lib.IRE_FLAG_DECODE_PNG | _lib.IRE_FLAG_DECODE_PNG_ALL)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def png_engine():
    eng = Engine(device_index=0, max_batch=8, num_streams=1, decode_png=True)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def accept():
    return {name: (data, cases.pil_rgb(data)) for name, data in cases.accept_cases().items()}      # the reference, computed once


@pytest.mark.filterwarnings("ignore:Palette images with Transparency")
def test_device_equals_pillow(all_engine, accept):
    """every accepted (colour type, depth) pair with and without interlace at 1x1, 1x2, 3x2, 2x5 and 5x3 (empty passes); widths 9, 17 and
    70 at every sub-8 depth (a partial last byte); 33x70 at 16-bit RGBA (70 units cross the wavefront); 131x9 and 521x9 (more than 64
    rows in one pass); filters 2, 3 and 4 on every pass's first row; Average and Paeth on units whose bytes carry on their own; short and
    long palettes; tRNS"""
    assert len(accept) >= 180
    for name, (data, want) in accept.items():
        plan = all_engine.decode_png_plan(data)
        assert plan is not None and plan[:2] == want.shape[:2], (name, plan, all_engine.last_plan_reason)
        got = all_engine.decode_png(data)
        bad = int((got != want).sum())
        print("%-28s %5d bytes  plan %s  differing bytes %d" % (name, len(data), plan, bad))
        assert got.shape == want.shape and bad == 0, name


def _mixed(h, w):
    """old and new forms of one size: 8-bit without interlace (RGB and palette), Adam7 at 8 bits, a 4-bit palette, 16-bit RGBA with and
    without interlace, 1-bit grey Adam7, 2-bit grey"""
    return [old_cases.make(h, w, 2, seed=40), cases.make(h, w, 2, 8, 1, seed=41), cases.make(h, w, 3, 4, 0, seed=42), cases.make(h, w, 6, 16, 1, seed=43),
            old_cases.make(h, w, 3, seed=44), cases.make(h, w, 0, 1, 1, seed=45), cases.make(h, w, 6, 16, 0, seed=46), cases.make(h, w, 0, 2, 0, seed=47)]


def test_a_batch_of_old_and_new_forms_with_an_image_pitch_larger_than_the_image(all_engine):
    import torch
    h, w, gap = 131, 70, 37          # 131 rows: two bands without interlace, 65 rows in pass 7; 70 units: more than the wavefront
    files = _mixed(h, w)
    n = len(files)
    singles = [all_engine.decode_png(f) for f in files]
    for i, (f, s) in enumerate(zip(files, singles)):
        assert np.array_equal(s, cases.pil_rgb(f)), i
    buf = torch.full((n, h * w * 3 + gap), 0xA5, dtype=torch.uint8, device="cuda")
    view = buf[:, :h * w * 3].view(n, h, w, 3)
    out, status = all_engine.decode_png_device(files, out_u8=view)
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert status.cpu().tolist() == [0] * n
    for i, s in enumerate(singles):
        assert np.array_equal(host[i, :h * w * 3].reshape(h, w, 3), s), i
        assert (host[i, h * w * 3:] == 0xA5).all(), i          # the bytes behind each image: untouched
    # the old forms alone on this engine take the kernel they always took: the same bytes again
    out, status = all_engine.decode_png_device([files[0], files[4]])
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0, 0] and np.array_equal(out[0].cpu().numpy(), singles[0]) and np.array_equal(out[1].cpu().numpy(), singles[4])


@pytest.mark.parametrize("form", [(0, 4, 1), (3, 2, 1), (2, 16, 0), (6, 16, 1)])
def test_an_upload_of_a_new_form_equals_the_same_pixels_as_an_8_bit_file(all_engine, form):
    eng = all_engine
    ct, d, lace = form
    new = cases.make(100, 150, ct, d, lace, smooth=True, seed=11, before_idat=[pw.exif_chunk(6)])
    px = cases.pil_rgb(new)
    old = pw.png(px, 2, (1, 4), before_idat=[pw.exif_chunk(6)])
    assert cases.head_of(old)[3:] == (8, 0) and np.array_equal(cases.pil_rgb(old), px)
    plan = eng.upload_plan(new, 256)          # (256: no shrink, so that the 16-bit files' streams fit the room of their fitted pixels)
    assert plan == eng.upload_plan(old, 256) and plan[:3] == (100, 150, 6)
    jobs = [eng.submit_upload(new, max_dim=256), eng.submit_upload(old, max_dim=256)]
    (out, scores, _), (want, want_scores, _) = [eng.poll(j) for j in jobs]
    assert out.shape == (plan[3], plan[4], 3) and np.array_equal(out, want) and np.array_equal(scores, want_scores)
    # and as a file job
    new_file = cases.make(40, 48, ct, d, lace, smooth=True, seed=12)
    old_file = pw.png(cases.pil_rgb(new_file), 2, (1, 4))
    (out, scores, _), (want, want_scores, _) = [eng.poll(j) for j in [eng.submit_file(new_file), eng.submit_file(old_file)]]
    assert out.shape == (40, 48, 3) and np.array_equal(out, want) and np.array_equal(scores, want_scores)


def test_a_filter_byte_of_5_on_a_pass_first_row_is_flagged_and_its_neighbours_decode(all_engine):
    import torch
    bad, good = cases.bad_filter_adam7()
    other = cases.make(24, 20, 6, 16, 1, seed=5)
    files = [good, bad, other, bad, good]
    out, status = all_engine.decode_png_device(files)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0, 16, 0, 16, 0]
    for i in (0, 2, 4):
        assert np.array_equal(out[i].cpu().numpy(), cases.pil_rgb(files[i])), i
    with pytest.raises(EngineError) as e:
        all_engine.decode_png(bad)
    assert e.value.status == _lib.IRE_ERR_INVALID_INPUT and "corrupt PNG data (decoder status 16)" in e.value.message
    assert np.array_equal(all_engine.decode_png(good), cases.pil_rgb(good))          # the engine stays usable


def test_an_engine_with_the_png_flag_only_refuses_with_the_old_reasons(png_engine):
    files = cases.form_cases()
    for name, data in files.items():
        _, _, ct, d, lace = cases.head_of(data)
        word = cases.old_reason_word(ct, d, lace)
        assert png_engine.decode_png_plan(data) is None and word in png_engine.last_plan_reason, name
        with pytest.raises(EngineError) as e:
            png_engine.decode_png(data)
        assert e.value.status == _lib.IRE_ERR_INVALID_INPUT and e.value.message.startswith("invalid: PNG ") and word in e.value.message, (name, e.value.message)
    # the C entries themselves, not only the Python plan in front of them
    lib = _lib.load()
    out = np.zeros((24, 20, 3), np.uint8)
    for data, word in ((cases.make(24, 20, 2, 8, 1, smooth=True), "Adam7 interlacing"), (cases.make(24, 20, 0, 4, 0, smooth=True), "bit depth other than 8")):
        assert lib.ire_decode_png(png_engine._h, data, len(data), out.ctypes.data, 24, 20) == _lib.IRE_ERR_INVALID_INPUT
        assert word in lib.ire_last_error().decode()
        for submit in (png_engine.submit_file, png_engine.submit_upload):
            with pytest.raises(EngineError) as e:
                submit(data)
            assert e.value.status == _lib.IRE_ERR_INVALID_INPUT and word in e.value.message
        assert upload_plan_reason(data, 2048, png_engine.upload_accept)[0] is None
