"""The shapes where 32-bit addresses end (DESIGN.md "Address arithmetic at the largest shapes").

The convolutions address one image's tensor with a 64-bit base and an unsigned 32-bit byte offset, range-checked by a 32-bit buffer
resource.  A level-0 tensor is 64 bytes a pixel: it passes 2^31 bytes at 4096 x 8192 and is 2^32 bytes at 8192 x 8192, the one shape
the engine refuses (csrc/conv_plan.hpp::piece_addressable; tests/test_conv_plan.py holds the rule and every planned launch on the CPU).

The float64 oracle cannot run at 64 Mpx, so the reference is the same network where every offset is small -- two contracts the suite
already keeps bit for bit at small sizes:
  * one large image: the untiled restore equals the row-strip restore (tests/test_tiled_gpu.py); each strip lives in buffers of its own
    and stays below 2^30 bytes.  The issue named 8 strips of 528 and of 1016 rows; the strip planner takes multiples of 128 rows only, so
    4224 rows run as 11 strips of 384 and, at a width of 8192, the last height below 2^32 bytes that strips, 8064 = 63 x 128, as 7 strips
    of 1152.  The largest image the untiled entries take is 2^32 - 2^22 bytes at level 0: 8192 x 8184 strips (8 x 1024, 16 x 512 rows) and
    holds the equality with a ragged last tile column at every level; 8184 x 8192 divides into no such strips and is checked for liveness;
  * many images: a batch of 64 equals the same images eight at a time (test_batch_and_stream_invariance).  Image 32 starts at byte 2^31
    of the level-0 buffers, the batch ends at 2^32.
8192 x 8192 itself: the untiled entries refuse it with the rule's message; in strips it still runs, 16 strips against 8.

Then the byte kernels at their largest window, one image each, against the references the suite uses at small sizes.

Inputs are made on the device from fixed seeds: a colour, two ramps and noise, as tests/test_fit_gpu.py::_images."""
import base64
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def _image(h, w, seed):
    """cuda uint8 [h, w, 3]: smooth structure plus noise; rows, columns and seeds all differ"""
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    x = torch.randn((h, w, 3), generator=g, device="cuda") * 12.0
    x += torch.randint(0, 156, (1, 1, 3), generator=g, device="cuda").float()
    x += torch.linspace(0, 60, w, device="cuda")[None, :, None]
    x += torch.linspace(0, 40, h, device="cuda")[:, None, None]
    return x.clamp_(0, 255).to(torch.uint8)


def _distinct(t, parts):
    """no two of the `parts` equal slices along dim 0 hold the same bytes (their sums differ: sufficient)"""
    import torch
    sums = t.reshape(parts, -1).sum(1, dtype=torch.int64).tolist()
    return len(set(sums)) == parts


def _alive(out, img):
    """not constant, the network did something, and the last 64 rows are not the first 64: a restore that read zeros or dropped its
    stores must not pass by symmetry"""
    assert int(out.min()) != int(out.max())
    assert not bool((out[-64:] == out[:64]).all())
    assert not bool((out == img).all())
    assert int(out[-64:].min()) != int(out[-64:].max()) and int(out[:, -64:].min()) != int(out[:, -64:].max())


def _release(eng):
    """a change of shape frees the workspace, another strip plan the strip session: the large buffers go before the next are made"""
    import torch
    small = torch.zeros((1, 256, 64, 3), dtype=torch.uint8, device="cuda")
    eng.restore_tensor(small)
    eng.restore_tiled_tensor(small[0], 2)
    torch.cuda.synchronize()


def _whole_equals_strips(eng, h, w, nstrips, seed):
    import torch
    assert eng.max_batch_for(h, w) >= 1, "not enough free device memory for one %d x %d image (bytes_per_image)" % (h, w)
    img = _image(h, w, seed)
    assert _distinct(img, nstrips)
    whole = eng.restore_tensor(img[None])[0]
    torch.cuda.synchronize()
    _release(eng)
    tiled = eng.restore_tiled_tensor(img, nstrips)
    torch.cuda.synchronize()
    _release(eng)
    same = torch.equal(tiled, whole)
    if not same:
        bad = (tiled != whole).any(2).any(1).nonzero().flatten()
        pytest.fail("%d x %d: %d rows differ, first %d, last %d" % (h, w, bad.numel(), int(bad[0]), int(bad[-1])))
    _alive(whole, img)


@pytest.fixture(scope="module")
def big_engine():
    from image_restoration_platform_amd.engine import Engine
    eng = Engine(device_index=0, max_batch=1, num_streams=1)
    yield eng
    eng.close()


# ---- one large image ----------------------------------------------------------------------------------------------------------------
def test_4224x8192_past_2_to_the_31_equals_its_11_strips(big_engine):
    """2^31 + 2^26 bytes at level 0: the first of the issue's shapes whose byte offsets leave `int`."""
    _whole_equals_strips(big_engine, 4224, 8192, 11, seed=1)


def test_8192x4224_transposed_equals_its_8_strips(big_engine):
    _whole_equals_strips(big_engine, 8192, 4224, 8, seed=2)


def test_4224x8192_fp8_engine_equals_its_11_strips():
    from image_restoration_platform_amd.engine import Engine
    eng = Engine(device_index=0, max_batch=1, num_streams=1, precision="fp8")
    try:
        _whole_equals_strips(eng, 4224, 8192, 11, seed=3)
    finally:
        eng.close()


def test_8064x8192_the_last_height_below_2_to_the_32_that_strips_equals_its_7_strips(big_engine):
    """2^32 - 2^26 bytes at level 0: the largest image of 8192 columns that both entries take (8184 x 8192 restores untiled -- below -- but
    8184 rows divide into no strips of a multiple of 128 rows)."""
    _whole_equals_strips(big_engine, 8064, 8192, 7, seed=4)


def test_8192x8184_the_largest_accepted_image_equals_its_8_strips(big_engine):
    """2^32 - 2^22 bytes at level 0, the most the rule admits.  8184 columns are no multiple of the 32-pixel tile at any level (8184, 4092,
    2046, 1023): the last tile column overhangs the image while the byte offsets of the last rows sit within 2^22 of 2^32."""
    _whole_equals_strips(big_engine, 8192, 8184, 8, seed=8)


def test_8192x8184_fp8_engine_equals_its_16_strips():
    from image_restoration_platform_amd.engine import Engine
    eng = Engine(device_index=0, max_batch=1, num_streams=1, precision="fp8")
    try:
        _whole_equals_strips(eng, 8192, 8184, 16, seed=9)
    finally:
        eng.close()


def test_8192x8192_is_refused_untiled_and_runs_in_strips(big_engine):
    """2^32 bytes at level 0: a 32-bit resource of that size holds NO bytes, every load would read zero and every store be dropped.  The
    untiled entries refuse the shape and say why, the capacity query answers 0; in strips (each below 2^30 bytes) it runs, and 16 strips of
    512 rows equal 8 of 1024."""
    import torch
    from image_restoration_platform_amd.engine import EngineError
    eng = big_engine
    # the strip runs below hold as much as one untiled image of the largest accepted shape (bytes_per_image); 8192 x 8192 itself answers 0
    assert eng.max_batch_for(8184, 8192) >= 1, "not enough free device memory for the strips of one 8192 x 8192 image (bytes_per_image)"
    img = _image(8192, 8192, seed=5)
    assert _distinct(img, 16)
    assert eng.max_batch_for(8192, 8192) == 0
    for call in (lambda: eng.restore_tensor(img[None]), lambda: eng.restore_fit_tensor(img[None, :8185, :8190].contiguous())):
        with pytest.raises(EngineError) as e:
            call()
        assert e.value.status == 1 and "must stay below 2^32 bytes" in e.value.message and "row strips" in e.value.message, e.value.message
        assert "which 8192 x 8192 (4294967296 bytes) is not" in e.value.message, e.value.message      # the padded size, for the fit entry too
    host = np.zeros((8192, 8192, 3), np.uint8)
    for submit in (eng.submit, eng.submit_fit):       # the batcher queues no job for it
        with pytest.raises(EngineError) as e:
            submit(host)
        assert e.value.status == 1 and "must stay below 2^32 bytes" in e.value.message
    with pytest.raises(EngineError) as e:
        eng.restore_tiled_tensor(img, 1)              # one strip: 8194 rows with its halo
    assert e.value.status == 1 and "below 2^32 bytes" in e.value.message
    s16 = eng.restore_tiled_tensor(img, 16).clone()
    torch.cuda.synchronize()
    s8 = eng.restore_tiled_tensor(img, 8)
    torch.cuda.synchronize()
    _release(eng)
    assert torch.equal(s16, s8)
    _alive(s16, img)


def test_8184x8192_the_largest_image_the_untiled_entry_takes_is_written_to_its_end(big_engine):
    """2^32 - 2^22 bytes at level 0, the transposed largest shape.  8184 rows divide into no strips of a multiple of 128 rows, so the equality
    at this byte count is held by 8192 x 8184 (above); here: the call is accepted and its stores reach the last row and column of an output
    that was zero."""
    import torch
    eng = big_engine
    assert eng.max_batch_for(8184, 8192) >= 1, "not enough free device memory for one 8184 x 8192 image (bytes_per_image)"
    top = _image(8184, 8192, seed=6)
    out = eng.restore_tensor(top[None], out_u8=torch.zeros((1, 8184, 8192, 3), dtype=torch.uint8, device="cuda"))[0]
    torch.cuda.synchronize()
    _release(eng)
    _alive(out, top)
    assert int(out[-1].max()) > 0 and int(out[:, -1].max()) > 0          # the stores reached the last row and column of the zeroed output


# ---- many images --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engine64():
    from image_restoration_platform_amd.engine import Engine
    eng = Engine(device_index=0, max_batch=64, num_streams=1)
    yield eng
    eng.close()


def _batch_equals_eights(eng, h, w, fit, seed):
    import torch
    H, W = (h + 7) // 8 * 8, (w + 7) // 8 * 8
    assert eng.max_batch_for(H, W) >= 64, "not enough free device memory for 64 images of %d x %d (bytes_per_image)" % (H, W)
    imgs = torch.stack([_image(h, w, seed + i) for i in range(64)])
    assert _distinct(imgs, 64)
    run = eng.restore_fit_tensor if fit else eng.restore_tensor
    all64 = run(imgs).clone()
    torch.cuda.synchronize()
    for k in range(0, 64, 8):
        part = run(imgs[k:k + 8].contiguous())
        torch.cuda.synchronize()
        for i in range(8):
            assert torch.equal(all64[k + i], part[i]), (k + i, int((all64[k + i].int() - part[i].int()).abs().max()))
    for i in (0, 31, 32, 63):                # both sides of byte 2^31 of the level-0 buffers, and the batch's two ends
        _alive(all64[i], imgs[i])
    assert not torch.equal(all64[0], all64[32]) and not torch.equal(all64[31], all64[63])


def test_64_images_of_1024x1024_equal_the_same_images_eight_at_a_time(engine64):
    _batch_equals_eights(engine64, 1024, 1024, False, seed=100)


def test_64_images_of_1017x1023_through_restore_fit_equal_eight_at_a_time(engine64):
    """the pad and the crop cross the same marks: the padded batch is 64 x 1024 x 1024"""
    _batch_equals_eights(engine64, 1017, 1023, True, seed=200)


# ---- the byte kernels at the largest window --------------------------------------------------------------------------------------------
BH, BW = 8185, 8191          # the largest window that is a multiple of nothing: both pad paths, every tail


@pytest.fixture(scope="module")
def big():
    """(cuda uint8 [8192, 8192, 3], the same on the host)"""
    import torch
    img = _image(8192, 8192, seed=7)
    torch.cuda.synchronize()
    return img, img.cpu().numpy()


@pytest.mark.parametrize("h,w", [(8192, 8192), (1, 8192)])
def test_classifier_at_the_largest_image_equals_the_c_oracle_bit_for_bit(engine, big, h, w):
    import torch
    from oracle import classifier as oc
    img, host = big
    jp = torch.ones(1, dtype=torch.uint8, device="cuda")
    scores, labels = engine.classify_tensor(img[None, :h, :w].contiguous(), jp)
    torch.cuda.synchronize()
    s, l = oc.classify(np.ascontiguousarray(host[:h, :w]), True)
    got = scores.cpu().numpy()[0]
    assert got.view(np.uint64).tolist() == s.view(np.uint64).tolist(), (got, s)
    assert int(labels[0]) == l


def _decode_png(text):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(base64.b64decode(text))).convert("RGB"))


def test_stored_png_text_at_8185x8191_equals_the_python_encoder(engine, big):
    import torch
    from oracle import encode as oenc
    img, host = big
    px = np.ascontiguousarray(host[:BH, :BW])
    out = engine.encode_png_base64_fit_tensor(img[None, :BH, :BW])          # the window where it lies: its pitches go to the engine
    torch.cuda.synchronize()
    text = out[0].cpu().numpy().tobytes()
    ref = oenc.png_base64(px)
    ref = ref.encode("ascii") if isinstance(ref, str) else bytes(ref)
    assert len(text) == len(ref) == engine.png_base64_bytes_fit(BH, BW)
    assert text == ref, next(i for i in range(0, len(ref), 4096) if text[i:i + 4096] != ref[i:i + 4096])
    assert np.array_equal(_decode_png(text), px)


def test_deflate_png_text_at_8185x8191_decodes_to_the_pixels_within_its_bound(engine, big):
    from test_png_deflate_gpu import _encode_tensor
    img, host = big
    bound = engine.png_deflate_base64_bound(BH, BW)
    texts, lens = _encode_tensor(engine, img[None, :BH, :BW], bound + 517, fill=0xA5)
    n = int(lens[0])
    assert 0 < n <= bound and n % 4 == 0
    assert (texts[0, bound:] == 0xA5).all()             # the guard bytes between the bound and the stride
    assert (texts[0, n:bound] == 0xA5).all()            # and nothing behind the text's own end
    text = texts[0, :n].tobytes()
    assert len(text) == n and 0xA5 not in text
    assert np.array_equal(_decode_png(text), host[:BH, :BW])


def test_jpeg_text_at_8185x8191_equals_libjpeg_turbo(engine, big):
    """Pillow's file with the settings tests/test_jpeg_model.py pins the model to (quality 85, 4:4:4, the model's restart interval)."""
    from test_jpeg_gpu import _encode_tensor
    from test_jpeg_model import pillow_file
    img, host = big
    bound = engine.jpeg_base64_bound(BH, BW)
    texts, lens = _encode_tensor(engine, img[None, :BH, :BW], bound + 517, fill=0xA5)
    n = int(lens[0])
    assert 0 < n <= bound
    assert (texts[0, bound:] == 0xA5).all() and (texts[0, n:bound] == 0xA5).all()
    ref = base64.b64encode(pillow_file(np.ascontiguousarray(host[:BH, :BW])))
    text = texts[0, :n].tobytes()
    assert n == len(ref)
    assert text == ref, next(i for i in range(0, len(ref), 4096) if text[i:i + 4096] != ref[i:i + 4096])


def test_jpeg_text_at_8177x8191_quality_100_420_equals_libjpeg_turbo(engine, big):
    """The other end of the settings at the largest window: quality 100 runs the interval kernel's big size class (18944 bytes of scratch
    per interval against 10112), 4:2:0 has half as many, larger intervals, and 8177 % 16 == 1 gives the last MCU row dummy Y blocks.
    Pillow's file with the settings tests/test_jpeg_opt_model.py pins the model to; the model itself is too slow at this size."""
    from test_jpeg_opt_gpu import _encode_tensor
    from test_jpeg_opt_model import pillow_file
    img, host = big
    h, w, q, s = 8177, BW, 100, 2
    bound = engine.jpeg_base64_bound(h, w, q, s)
    texts, lens = _encode_tensor(engine, img[None, :h, :w], bound + 517, q, s, fill=0xA5)
    n = int(lens[0])
    assert 0 < n <= bound
    assert (texts[0, bound:] == 0xA5).all() and (texts[0, n:bound] == 0xA5).all()
    ref = base64.b64encode(pillow_file(np.ascontiguousarray(host[:h, :w]), q, s))
    text = texts[0, :n].tobytes()
    assert n == len(ref)
    assert text == ref, next(i for i in range(0, len(ref), 4096) if text[i:i + 4096] != ref[i:i + 4096])
