"""Progressive JPEG results, without a GPU: the model (tests/jpeg_progenc_model.py) against libjpeg-turbo's own file (Pillow,
progressive=True, restart_marker_rows=1) byte for byte; the decoder's model (tests/jpeg_prog_model.py) reads the model's file back to
the coefficients it was made of; Pillow decodes it to the very pixels of the optimised baseline file; and the C ABI: the new symbols,
the flag, the bound."""
import ctypes
import functools
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_huffopt_model as huffopt    # noqa: E402
import jpeg_opt_model as opt            # noqa: E402
import jpeg_prog_model as dec           # noqa: E402
import jpeg_progenc_model as model      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from image_restoration_platform_amd import _lib, synth      # noqa: E402

SIZES = [(1, 1), (5, 7), (8, 8), (16, 16), (17, 9), (45, 37), (72, 40), (8, 1032)]
QUALITIES = [1, 50, 85, 95, 100]
KINDS = ["noise", "synth", "flat", "gradient"]


@functools.lru_cache(maxsize=None)
def image(kind, h, w):
    if kind == "noise":
        px = np.random.default_rng(h * 131 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    elif kind == "synth":
        px = np.ascontiguousarray(synth.image(3, max(h, 8), max(w, 8))[:h, :w])
    elif kind == "flat":
        px = np.full((h, w, 3), (200, 30, 90), np.uint8)
    else:
        y, x = np.mgrid[0:h, 0:w]
        px = np.stack([(3 * x + y) % 256, (2 * y + 40) % 256, (x * y // 3 + 7) % 256], -1).astype(np.uint8)
    px.setflags(write=False)
    return px


def pillow_file(px, quality, sampling, **kw):
    from PIL import Image, ImageFile
    bio = io.BytesIO()
    keep = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = 1 << 22      # (a progressive file is written from one buffer)
    try:
        Image.fromarray(px, "RGB").save(bio, format="JPEG", quality=quality, subsampling=sampling, **(kw or dict(progressive=True, restart_marker_rows=1)))
    finally:
        ImageFile.MAXBLOCK = keep
    return bio.getvalue()


@pytest.mark.parametrize("h,w", SIZES)
def test_model_equals_libjpeg_turbo(h, w):
    """Byte equality with Pillow's file for quality=q, subsampling=s, progressive=True, restart_marker_rows=1; and the bound holds."""
    for kind in KINDS:
        px = image(kind, h, w)
        for q in QUALITIES:
            for s in (0, 2):
                f = model.jpeg_file(px, q, s)
                assert f == pillow_file(px, q, s), (kind, h, w, q, s)
                assert len(f) <= model.file_bound(h, w, q, s)


def test_the_scan_script_and_the_restart_intervals():
    """the 72 x 40 image of the issue: SOF2, ten SOS with the script's parameters, the DRI values 5 / 9 alternating at 4:2:0 (wherever the interval changes: six times) and
    written once at 4:4:4, a DHT in front of every scan but the DC refinement"""
    for s, want_dri in ((0, [9]), (2, [5, 9, 5, 9, 5, 9])):
        f = model.jpeg_file(image("noise", 40, 72), 85, s)
        p = dec.plan(f)
        assert [(tuple(sc.comps), sc.ss, sc.se, sc.ah, sc.al) for sc in p.scans] == [tuple(x) for x in model.SCANS]
        segs, i = [], 2
        while i < len(f) - 2:                 # (entropy-coded bytes never hold 0xFF in front of a marker value: stuffing)
            if f[i] == 0xFF and f[i + 1] in (0xC4, 0xDD, 0xDA, 0xC2, 0xDB, 0xE0):
                n = int.from_bytes(f[i + 2:i + 4], "big")
                segs.append((f[i + 1], f[i + 4:i + 2 + n]))
                i += 2 + n
            else:
                i += 1
        assert [int.from_bytes(b, "big") for m, b in segs if m == 0xDD] == want_dri
        assert sum(1 for m, _ in segs if m == 0xC2) == 1 and sum(1 for m, _ in segs if m == 0xC4) == 10
        assert [b[0] for m, b in segs if m == 0xC4] == [t for _, t in model.TABLES]
        assert f[-2:] == b"\xff\xd9"


@pytest.mark.parametrize("h,w", [(17, 9), (45, 37), (72, 40)])
def test_our_decoder_model_reads_the_coefficients_back(h, w):
    for q, s in ((85, 0), (50, 2), (100, 2)):
        px = image("noise", h, w)
        planes = model.planes_of(px, q, s)
        grids = dec.coefficients(dec.plan(model.jpeg_file(px, q, s)))
        for c in range(3):
            assert np.array_equal(grids[c][..., opt.ZIGZAG], planes[c]), (h, w, q, s, c)


@pytest.mark.parametrize("h,w", [(5, 7), (45, 37), (72, 40)])
def test_pillow_decodes_the_pixels_of_the_optimised_baseline_file(h, w):
    from PIL import Image
    for kind in ("noise", "gradient"):
        for q, s in ((85, 0), (60, 2), (100, 0)):
            px = image(kind, h, w)
            a = np.asarray(Image.open(io.BytesIO(model.jpeg_file(px, q, s))).convert("RGB"))
            b = np.asarray(Image.open(io.BytesIO(huffopt.jpeg_file(px, q, s))).convert("RGB"))
            assert np.array_equal(a, b), (kind, h, w, q, s)


def test_abi():
    raw = ctypes.CDLL(_lib.LIB_PATH)
    names = ("ire_jpeg_progressive_base64_bound", "ire_encode_jpeg_progressive_base64_fit_device", "ire_encode_jpeg_progressive_base64_fit",
             "ire_debug_jpeg_progressive_from_coefs")
    ffi = open(os.path.join(ROOT, "image_restoration_platform_amd", "node", "ire_ffi.mjs")).read()
    for name in names:
        assert hasattr(raw, name) and name in _lib.SYMBOLS and name in ffi, name
    assert _lib.IRE_FLAG_JPEG_PROGRESSIVE == 2048
    lib = _lib.load()
    assert ctypes.sizeof(_lib.IreConfig) == 48 and lib.ire_abi_version() == 3
    import torch
    accepted = _lib.IRE_OK if torch.cuda.is_available() else _lib.IRE_ERR_UNAVAILABLE      # as far as the device check

    def init(flags, quality=0, sampling=0):
        h = ctypes.c_void_p()
        cfg = _lib.IreConfig()
        cfg.struct_size, cfg.max_batch, cfg.flags, cfg.jpeg_quality, cfg.jpeg_sampling = ctypes.sizeof(_lib.IreConfig), 2, flags, quality, sampling
        st = lib.ire_init(ctypes.byref(cfg), ctypes.byref(h))
        err = lib.ire_last_error()
        if st == _lib.IRE_OK:
            lib.ire_shutdown(h)
        return st, err

    P = _lib.IRE_FLAG_JPEG_PROGRESSIVE
    assert init(_lib.IRE_FLAG_RESULT_JPEG | P)[0] == accepted
    assert init(_lib.IRE_FLAG_RESULT_JPEG | P | _lib.IRE_FLAG_JPEG_OPTIMIZE, 60, 2)[0] == accepted
    assert init(_lib.IRE_FLAG_RESULT_JPEG | P | _lib.IRE_FLAG_DECODE_PROGRESSIVE)[0] == accepted
    for flags in (P, P | _lib.IRE_FLAG_RESULT_PNG_BASE64, P | _lib.IRE_FLAG_RESULT_PNG_DEFLATE, P | _lib.IRE_FLAG_DECODE_PROGRESSIVE, P | _lib.IRE_FLAG_JPEG_OPTIMIZE):
        st, err = init(flags)
        assert st == _lib.IRE_ERR_INVALID_INPUT and b"invalid" in err and b"IRE_FLAG_RESULT_JPEG" in err, (flags, err)
    for bits in (2, 16, 64, 512, 4096, 8 | P | 512):
        st, err = init(bits)
        assert st == _lib.IRE_ERR_INVALID_INPUT and b"unknown bits" in err, (bits, err)
    # the bound: the model's, at least the optimised one; 0 for what is refused
    for h, w in ((1, 1), (5, 7), (45, 37), (1024, 1024), (8192, 8192), (8, 8192), (8192, 8)):
        for q, s in ((1, 0), (60, 2), (85, 0), (100, 2), (100, 0)):
            assert lib.ire_jpeg_progressive_base64_bound(h, w, q, s) == model.base64_bound(h, w, q, s) >= lib.ire_jpeg_optimized_base64_bound(h, w, q, s) > 0, (h, w, q, s)
        assert lib.ire_jpeg_progressive_base64_bound(h, w, 0, 0) == model.base64_bound(h, w, 85, 0)
    for h, w, q, s in ((0, 8, 85, 0), (8, 8193, 85, 2), (8, 8, 101, 0), (8, 8, -1, 0), (8, 8, 85, 1), (8, 8, 85, 3), (8, 8, 85, -2)):
        assert lib.ire_jpeg_progressive_base64_bound(h, w, q, s) == 0, (h, w, q, s)
    # null handles are refused, not dereferenced
    assert lib.ire_encode_jpeg_progressive_base64_fit(None, None, 1, 5, 7, None, 4096, None, 60, 2) == _lib.IRE_ERR_INVALID_INPUT
    assert lib.ire_encode_jpeg_progressive_base64_fit_device(None, None, 1, 5, 7, 21, 105, None, 4096, None, 60, 2, None) == _lib.IRE_ERR_INVALID_INPUT
    assert lib.ire_debug_jpeg_progressive_from_coefs(None, None, 1, 5, 7, 85, 0, None, 4096, None) == _lib.IRE_ERR_INVALID_INPUT
