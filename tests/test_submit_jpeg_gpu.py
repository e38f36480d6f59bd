"""File jobs in the batcher (ire_submit_jpeg): an encoded baseline JPEG upload goes in, is parsed by its submitter, decoded on the
device with its batch and restored -- the result is byte for byte that of ire_submit_fit on the file's PIL pixels, on a pixel
engine and on an IRE_FLAG_RESULT_JPEG engine, the scores too; jobs coalesce; a progressive file is refused at submit; a corrupt
file fails alone; a released job leaves the engine usable; the restorer's upload switch takes the path."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_decode_cases as cases      # noqa: E402
import jpeg_decode_model as model      # noqa: E402
import jpeg_decode_window_cases as wcases      # noqa: E402

from image_restoration_platform_amd import _lib      # noqa: E402
from image_restoration_platform_amd.engine import Engine, EngineError      # noqa: E402

pytestmark = pytest.mark.gpu


def _uploads():
    """five files of 136 x 200 (w x h) and two of 64 x 48: every sampling, grey, optimised tables, a restart interval"""
    big = [cases.encode(cases.noise(200, 136, 51), 90, 0), cases.encode(cases.smooth(200, 136, 52), 85, 2), cases.encode(cases.noise(200, 136, 53), 85, 1, optimize=True),
           cases.encode(cases.smooth(200, 136, 54)[:, :, 0], 85), cases.encode(cases.noise(200, 136, 55), 75, 2, restart_marker_blocks=5)]
    small = [cases.encode(cases.noise(48, 64, 56), 85, 0), cases.encode(cases.smooth(48, 64, 57), 95, 2)]
    return [big[0], small[0], big[1], big[2], small[1], big[3], big[4]]


def _check_equal_to_pixel_jobs(eng):
    files = _uploads()
    before = eng.stats()
    jobs = [eng.submit_jpeg(f) for f in files]              # all seven before the first poll
    got = [eng.poll(j) for j in jobs]
    after = eng.stats()
    print("batches %d, images %d" % (after["batches"] - before["batches"], after["images"] - before["images"]))
    assert after["images"] - before["images"] == len(files)
    assert after["batches"] - before["batches"] < len(files)              # some batch was larger than one
    for f, (out, scores, _) in zip(files, got):
        px = cases.pillow_pixels(f)
        want, want_scores, _ = eng.poll(eng.submit_fit(px, is_jpeg=True))
        if isinstance(want, bytes):
            assert out == want
        else:
            assert out.shape == px.shape and np.array_equal(out, want)
        assert np.array_equal(scores, want_scores)
    # the caller's scores travel with a file job as with a pixel job
    given = np.linspace(0.05, 0.65, 7)
    out, scores, _ = eng.poll(eng.submit_jpeg(files[0], scores=given))
    want, want_scores, _ = eng.poll(eng.submit_fit(cases.pillow_pixels(files[0]), is_jpeg=True, scores=given))
    assert (out == want if isinstance(want, bytes) else np.array_equal(out, want)) and np.array_equal(scores, want_scores)


def test_file_jobs_equal_pixel_jobs_on_a_pixel_engine(engine):
    _check_equal_to_pixel_jobs(engine)


def test_file_jobs_equal_pixel_jobs_on_a_jpeg_result_engine():
    eng = Engine(max_batch=8, flags=_lib.IRE_FLAG_RESULT_JPEG)
    try:
        _check_equal_to_pixel_jobs(eng)
    finally:
        eng.close()


def test_a_progressive_file_is_refused_at_submit(engine):
    prog = cases.encode(cases.smooth(48, 64, 3), 85, 2, progressive=True)
    plan, why = engine.decode_jpeg_plan_reason(prog)
    assert plan is None and "progressive" in why
    job = ctypes.c_void_p()
    rc = engine._lib.ire_submit_jpeg(engine._h, prog, len(prog), None, ctypes.byref(job))
    assert rc == _lib.IRE_ERR_INVALID_INPUT and not job.value
    assert (engine._lib.ire_last_error() or b"").decode() == why
    with pytest.raises(EngineError) as e:
        engine.submit_jpeg(prog)
    assert e.value.status == _lib.IRE_ERR_INVALID_INPUT and e.value.message == why
    assert engine.stats()["queueDepth"] == 0


def test_a_corrupt_file_among_three_fails_alone(engine):
    good, variants = wcases.corrupted_two_window_files(40)

    def corrupt(d):
        try:
            model.coefficients(model.plan(d))
        except model.Corrupt:
            return True
        except model.Refused:
            return False
        return False
    bad = next(d for _, d in variants if corrupt(d))
    other = cases.encode(cases.smooth(128, 128, 61), 85, 2)
    jobs = [engine.submit_jpeg(f) for f in (good, bad, other)]
    first = engine.poll(jobs[0])
    with pytest.raises(EngineError) as e:
        engine.poll(jobs[1])
    assert e.value.status == _lib.IRE_ERR_INVALID_INPUT and "invalid: corrupt JPEG data (decoder status" in e.value.message
    last = engine.poll(jobs[2])
    for f, (out, scores, _) in ((good, first), (other, last)):
        want, want_scores, _ = engine.poll(engine.submit_fit(cases.pillow_pixels(f), is_jpeg=True))
        assert np.array_equal(out, want) and np.array_equal(scores, want_scores)


def test_releasing_a_pending_file_job_leaves_the_engine_usable(engine):
    f = cases.encode(cases.noise(48, 64, 71), 85, 0)
    engine.release(engine.submit_jpeg(f))
    out, _, _ = engine.poll(engine.submit_jpeg(f))
    want, _, _ = engine.poll(engine.submit_fit(cases.pillow_pixels(f), is_jpeg=True))
    assert np.array_equal(out, want)


def test_the_restorer_sends_an_undecoded_upload_as_a_file_job(engine, monkeypatch):
    from image_restoration_platform_amd import restorator
    data = cases.encode(cases.smooth(45, 70, 3), 85, 2)
    prog = cases.encode(cases.smooth(45, 70, 3), 85, 2, progressive=True)
    restorer = restorator.EngineRestorer(engine, result_codec="png")
    monkeypatch.delenv("IRE_UPLOAD_CODEC", raising=False)
    ref = restorer.restore_image("", [data])["base64Image"]
    ref_prog = restorer.restore_image("", [prog])["base64Image"]
    monkeypatch.setenv("IRE_UPLOAD_CODEC", "jpeg-device")
    before = dict(restorator.UPLOAD_DECODES)
    assert restorer.restore_image("", [data])["base64Image"] == ref
    assert restorator.UPLOAD_DECODES["device"] == before["device"] + 1 and restorator.UPLOAD_DECODES["host"] == before["host"]
    assert restorer.restore_image("", [prog])["base64Image"] == ref_prog          # refused at submit: the host codec, as before
    assert restorator.UPLOAD_DECODES["host"] == before["host"] + 1 and restorator.UPLOAD_DECODES["device"] == before["device"] + 1
