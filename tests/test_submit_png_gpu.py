"""PNG files in the batcher, on an engine created with IRE_FLAG_DECODE_PNG: a PNG and a JPEG file of one size share a push and give
the text (here: the pixels) of ire_submit_fit of Pillow's pixels with is_jpeg 0 and 1; a PNG upload with an eXIf orientation equals the
composed calls; a corrupt PNG fails alone at its poll; a noise PNG breaks the room rule at submit; an engine without the flag refuses
a PNG at both entries with the reason it always gave; and the restorer's upload switch."""
import io
import os
import sys

import numpy as np
import pytest
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_cases as cases      # noqa: E402
import png_writer as pw        # noqa: E402

from image_restoration_platform_amd import _lib      # noqa: E402
from image_restoration_platform_amd.engine import Engine, EngineError      # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def png_engine():
    eng = Engine(device_index=0, max_batch=8, num_streams=1, decode_png=True)
    yield eng
    eng.close()


def _jpeg(px):
    bio = io.BytesIO()
    Image.fromarray(px, "RGB").save(bio, format="JPEG", quality=85, subsampling=0)
    return bio.getvalue()


def test_a_png_and_a_jpeg_file_share_a_push(png_engine):
    eng = png_engine
    png = cases.make(80, 96, 6, seed=3)                        # 96 wide, 80 high, RGBA
    jpg = _jpeg(cases.pixels(80, 96, 2, 4))
    # a full slot that alternates the kinds: each kind is decoded in ONE call, every file into its own place of the slot
    files = [png, jpg, cases.make(80, 96, 3, seed=5), jpg, cases.make(80, 96, 0, seed=6), _jpeg(cases.pixels(80, 96, 2, 7)), cases.make(80, 96, 4, seed=8), jpg]
    before = eng.stats()["batches"]
    jobs = [eng.submit_file(f) for f in files]                 # all before the first poll
    got = [eng.poll(j) for j in jobs]
    assert eng.stats()["batches"] == before + 1                # one slot, one batch
    for f, job, (out, scores, _) in zip(files, jobs, got):
        px = np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))
        assert (job[1], job[2]) == (80, 96)
        want, want_scores, _ = eng.poll(eng.submit_fit(px, is_jpeg=f[:2] == b"\xff\xd8"))
        assert np.array_equal(out, want) and np.array_equal(scores, want_scores)
    # is_jpeg matters to the classifier: the PNG's scores are those of is_jpeg = 0, not 1
    px = cases.pil_rgb(png)
    as_jpeg = eng.poll(eng.submit_fit(px, is_jpeg=True))[1]
    assert not np.array_equal(as_jpeg, got[0][1])


def test_a_png_upload_equals_the_composed_calls(png_engine):
    eng = png_engine
    # 300 wide, 200 high, orientation 6; noise on one row in sixteen, so that its data fits the room of its 85 x 57 fitted pixels
    px = cases.pixels(200, 300, 2, 8, noise=0)
    px[::16] = cases.pixels(200, 300, 2, 8)[::16]
    data = pw.png(px, 2, (1, 4), before_idat=[pw.exif_chunk(6)])
    sh, sw, o, oh, ow = eng.upload_plan(data, 128)
    assert (sh, sw, o, oh, ow) == (200, 300, 6, 85, 57)
    job = eng.submit_upload(data, max_dim=128)
    out, scores, _ = eng.poll(job)
    assert (job[1], job[2]) == (oh, ow)
    fitted = eng.preprocess(eng.decode_png(data), 6, 128)
    want, want_scores, _ = eng.poll(eng.submit_fit(fitted, is_jpeg=False))
    assert out.shape == (oh, ow, 3) and np.array_equal(out, want) and np.array_equal(scores, want_scores)
    given = np.linspace(0.1, 0.7, 7)
    out2, scores2, _ = eng.poll(eng.submit_upload(data, max_dim=128, scores=given))
    want2, _, _ = eng.poll(eng.submit_fit(fitted, is_jpeg=False, scores=given))
    assert np.array_equal(out2, want2) and np.array_equal(scores2, given)


def test_a_corrupt_png_fails_alone_at_its_poll(png_engine):
    eng = png_engine
    good = cases.fuzz_file()
    bad = cases.corrupt_cases()["adler"]                       # 24 x 20 like the good file; flagged by the decoder's CPU form first (tests/test_png_native.py)
    jobs = [eng.submit_file(good), eng.submit_file(bad), eng.submit_file(good)]
    want = eng.poll(eng.submit_fit(cases.pil_rgb(good), is_jpeg=False))[0]
    assert np.array_equal(eng.poll(jobs[0])[0], want)
    with pytest.raises(EngineError) as e:
        eng.poll(jobs[1])
    assert e.value.status == _lib.IRE_ERR_INVALID_INPUT and "invalid: corrupt PNG data (decoder status 12)" in e.value.message
    assert np.array_equal(eng.poll(jobs[2])[0], want)


def test_refusals_at_submit(png_engine, engine):
    for submit in (png_engine.submit_file, png_engine.submit_upload):
        with pytest.raises(EngineError) as e:
            submit(cases.noise_rgb())                          # the room rule
        assert e.value.status == _lib.IRE_ERR_INVALID_INPUT and "larger than its" in e.value.message
        with pytest.raises(EngineError) as e:
            submit(cases.refused_cases()["adam7"][0])
        assert "invalid: PNG Adam7" in e.value.message
    # an engine without the flag: today's reason, at both entries
    good = cases.fuzz_file()
    for submit in (engine.submit_jpeg, engine.submit_upload):
        with pytest.raises(EngineError) as e:
            submit(good)
        assert e.value.status == _lib.IRE_ERR_INVALID_INPUT and e.value.message == "invalid: not a JPEG file (no SOI)"


def test_the_upload_switch_of_the_restorer(png_engine, monkeypatch):
    from image_restoration_platform_amd import restorator
    good = cases.make(45, 70, 6, seed=2)
    px = cases.pixels(45, 70, 2, 2)
    interlaced = _interlace(px)                                # the plan refuses it, PIL decodes it
    assert png_engine.decode_png_plan(interlaced) is None and "Adam7" in png_engine.last_plan_reason
    monkeypatch.delenv("IRE_UPLOAD_CODEC", raising=False)
    ref, fmt = restorator.decode_image(good, png_engine)
    for codec in ("png-device", "device"):
        monkeypatch.setenv("IRE_UPLOAD_CODEC", codec)
        before = dict(restorator.UPLOAD_DECODES)
        got, fmt2 = restorator.decode_image(good, png_engine)
        assert restorator.UPLOAD_DECODES["device"] == before["device"] + 1 and restorator.UPLOAD_DECODES["host"] == before["host"]
        assert fmt == fmt2 == "png" and got.dtype == ref.dtype and np.array_equal(got, ref)
        got, _ = restorator.decode_image(interlaced, png_engine)
        assert restorator.UPLOAD_DECODES["host"] == before["host"] + 1 and restorator.UPLOAD_DECODES["device"] == before["device"] + 1
        assert np.array_equal(got, px)
    # jpeg-device keeps its meaning: a PNG goes to the host codec
    monkeypatch.setenv("IRE_UPLOAD_CODEC", "jpeg-device")
    before = dict(restorator.UPLOAD_DECODES)
    restorator.decode_image(good, png_engine)
    assert restorator.UPLOAD_DECODES["host"] == before["host"] + 1 and restorator.UPLOAD_DECODES["device"] == before["device"]


def _interlace(px):
    """px as an Adam7 PNG that Pillow decodes: the seven passes, filter 0, written by hand (Pillow itself writes no interlaced files)"""
    h, w, _ = px.shape
    passes = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))
    raw = b""
    for x0, y0, dx, dy in passes:
        sub = px[y0::dy, x0::dx]
        if sub.size:
            raw += pw.filter_rows(np.ascontiguousarray(sub), (0,))
    return pw.SIG + pw.ihdr(h, w, 2, interlace=1) + pw.chunk(b"IDAT", pw.deflate(raw)) + pw.chunk(b"IEND")
