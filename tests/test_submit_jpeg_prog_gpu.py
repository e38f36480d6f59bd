"""Progressive files as file jobs of the batcher (ire_submit_jpeg on an engine created with IRE_FLAG_DECODE_PROGRESSIVE): the result
is byte for byte that of ire_submit_fit on the file's PIL pixels, on a pixel engine and on an IRE_FLAG_RESULT_JPEG engine, the scores
too; progressive and baseline files of one size share a batch; a corrupt progressive file fails alone at its poll."""
import os
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


@pytest.fixture(scope="module")
def peng():
    eng = Engine(device_index=0, max_batch=8, flags=_lib.IRE_FLAG_DECODE_PROGRESSIVE)
    yield eng
    eng.close()


def _uploads():
    """four files of 72 x 56 (w x h), progressive and baseline, and one of 64 x 48: -> [(bytes, the bytes whose Pillow pixels it gives)]"""
    src = cases.encode(cases.noise(56, 72, 53), 85, 1)
    a = writer.pillow_progressive(cases.noise(56, 72, 51), 90, 0)
    b = writer.pillow_progressive(cases.smooth(56, 72, 52), 85, 2, restart_marker_blocks=4)
    c = cases.encode(cases.smooth(56, 72, 54), 85, 2)
    d = writer.pillow_progressive(cases.smooth(48, 64, 55)[:, :, 0], 85)
    return [(a, a), (d, d), (b, b), (writer.from_baseline(src, writer.script_moz()), src), (c, c)]


def _check_equal_to_pixel_jobs(eng):
    files = _uploads()
    before = eng.stats()
    jobs = [eng.submit_jpeg(f) for f, _ in files]           # all five before the first poll
    got = [eng.poll(j) for j in jobs]
    after = eng.stats()
    assert after["images"] - before["images"] == len(files) == 5
    assert after["batches"] - before["batches"] < len(files)              # some batch was larger than one
    for (f, ref), (out, scores, _) in zip(files, got):
        px = cases.pillow_pixels(ref)
        want, want_scores, _ = eng.poll(eng.submit_fit(px, is_jpeg=True))
        if isinstance(want, bytes):
            assert out == want
        else:
            assert out.shape == px.shape and np.array_equal(out, want)
        assert np.array_equal(scores, want_scores)


def test_file_jobs_equal_pixel_jobs_on_a_pixel_engine(peng):
    _check_equal_to_pixel_jobs(peng)


def test_file_jobs_equal_pixel_jobs_on_a_jpeg_result_engine():
    eng = Engine(max_batch=8, flags=_lib.IRE_FLAG_RESULT_JPEG | _lib.IRE_FLAG_DECODE_PROGRESSIVE)
    try:
        _check_equal_to_pixel_jobs(eng)
    finally:
        eng.close()


def test_progressive_and_baseline_files_of_one_size_share_a_batch(peng):
    """a first job keeps the device busy; the three behind it (progressive, baseline, progressive: one size) are coalesced meanwhile"""
    h, w = 56, 72
    files = [writer.pillow_progressive(cases.noise(h, w, 61), 85, 2), cases.encode(cases.noise(h, w, 62), 85, 0), writer.pillow_progressive(cases.smooth(h, w, 63), 85, 0)]
    opener = peng.submit_fit(cases.noise(512, 512, 60), is_jpeg=True)
    jobs = [peng.submit_jpeg(f) for f in files]
    peng.poll(opener)
    outs = [peng.poll(j) for j in jobs]
    assert peng.stats()["lastBatch"] == 3
    for f, (out, scores, _) in zip(files, outs):
        want, want_scores, _ = peng.poll(peng.submit_fit(cases.pillow_pixels(f), is_jpeg=True))
        assert np.array_equal(out, want) and np.array_equal(scores, want_scores)


def test_a_corrupt_progressive_file_among_three_fails_alone(peng):
    good, variants = prog.corrupt_refinement_candidates()

    def corrupt(d):
        try:
            model.coefficients(model.plan(d))
        except model.Corrupt:
            return True
        except model.Refused:
            return False
        return False
    bad = next(d for _, d in variants if corrupt(d))
    other = cases.encode(cases.smooth(47, 33, 61), 85, 2)
    jobs = [peng.submit_jpeg(f) for f in (good, bad, other)]
    first = peng.poll(jobs[0])
    with pytest.raises(EngineError) as e:
        peng.poll(jobs[1])
    assert e.value.status == _lib.IRE_ERR_INVALID_INPUT and "invalid: corrupt JPEG data (decoder status" in e.value.message
    last = peng.poll(jobs[2])
    for f, (out, scores, _) in ((good, first), (other, last)):
        want, want_scores, _ = peng.poll(peng.submit_fit(cases.pillow_pixels(f), is_jpeg=True))
        assert np.array_equal(out, want) and np.array_equal(scores, want_scores)
