"""The files the JPEG decoder is tested on, shared by the CPU tests of the model (test_jpeg_decode_model.py), of the native lane
algorithm (test_jpeg_decode_native.py) and the GPU tests (test_jpeg_decode_gpu.py).  Everything is seeded and made by Pillow (or by
the encoder's own model) when the tests run; nothing is read from disk."""
import io

import numpy as np
from PIL import Image

import jpeg_cases
import jpeg_model
from png_deflate_cases import noise, smooth      # noqa: F401

SIZES = [(8, 8), (16, 16), (17, 13), (33, 47), (64, 48), (5, 3), (40, 88)]          # (w, h)
QUALITIES = [30, 85, 95, 100]


def encode(px, quality=85, subsampling=0, **kw):
    """pixels ([h][w][3] -> RGB, [h][w] -> grey) -> the bytes of Pillow's (libjpeg-turbo's) baseline file"""
    bio = io.BytesIO()
    px = np.ascontiguousarray(px, np.uint8)
    if px.ndim == 2:
        Image.fromarray(px, "L").save(bio, "JPEG", quality=quality, **kw)
    else:
        Image.fromarray(px, "RGB").save(bio, "JPEG", quality=quality, subsampling=subsampling, **kw)
    return bio.getvalue()


def pillow_pixels(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def content(kind, h, w, seed):
    return noise(h, w, seed) if kind == "noise" else smooth(h, w, seed)


def grid_cases():
    """the seven sizes x three samplings x four qualities, smooth and noise alternating; plus optimize and restart variants"""
    d = {}
    seed = 100
    for w, h in SIZES:
        for sub in (0, 1, 2):
            for q in QUALITIES:
                seed += 1
                kind = "noise" if seed % 2 else "smooth"
                d["%dx%d_s%d_q%d_%s" % (w, h, sub, q, kind)] = encode(content(kind, h, w, seed), q, sub)
            d["%dx%d_s%d_opt" % (w, h, sub)] = encode(noise(h, w, seed + 1000), 85, sub, optimize=True)
            d["%dx%d_s%d_rst3" % (w, h, sub)] = encode(smooth(h, w, seed + 2000), 85, sub, restart_marker_blocks=3)
    for w, h in ((8, 8), (17, 13)):
        d["grey_%dx%d" % (w, h)] = encode(noise(h, w, 7)[:, :, 0], 85)
        d["grey_%dx%d_smooth" % (w, h)] = encode(smooth(h, w, 8)[:, :, 1], 95, optimize=True)
    return d


def sweep_cases():
    """heights 1..19 x widths 5..35, the sampling and the content cycling: every partial-MCU shape of every sampling"""
    d = {}
    for h in range(1, 20):
        for w in range(5, 36):
            sub = (h + w) % 3
            kind = "noise" if (h * 31 + w) % 2 else "smooth"
            d["sweep_%dx%d_s%d" % (w, h, sub)] = encode(content(kind, h, w, 1000 + h * 64 + w), 85, sub)
    return d


def encoder_cases():
    """the encoder's own files (tests/jpeg_model.py: 16-MCU intervals, RST numbering wrapping past 7)"""
    return {"enc_" + k: jpeg_model.jpeg_file(px) for k, px in jpeg_cases.all_cases().items()}


def refused_cases():
    """name -> (bytes, a word the reason must contain)"""
    px = smooth(16, 16, 3)
    bio = io.BytesIO()
    Image.fromarray(px, "RGB").convert("CMYK").save(bio, "JPEG")
    good = encode(px)
    return {
        "progressive": (encode(px, progressive=True), "progressive"),
        "cmyk": (bio.getvalue(), "4 components"),
        "420_width4": (encode(smooth(8, 4, 4), 85, 2), "width of at least 5"),
        "cut_in_header": (good[:100], "truncated JPEG header"),
    }


def with_quantisers(data, value):
    """the file with every entry of every quantiser table set to `value`: well-formed, but no encoder writes it"""
    b = bytearray(data)
    i = b.find(b"\xff\xdb")
    while i >= 0:
        n = int.from_bytes(b[i + 2:i + 4], "big")
        for j in range(i + 4, i + 2 + n, 65):
            b[j + 1:j + 65] = bytes([value]) * 64
        i = b.find(b"\xff\xdb", i + 2 + n)
    return bytes(b)


def out_of_range_cases():
    """q100 noise with its quantisers replaced: 4 keeps every sample inside -512..511 before the range limit (Pillow's SIMD code and
    the C formulas still agree), 8 leaves it, 255 also leaves int16 with the dequantised coefficients.  name -> (bytes, in range)"""
    base = encode(noise(24, 40, 9), 100, 0)
    return {"quant4": (with_quantisers(base, 4), True), "quant8": (with_quantisers(base, 8), False), "quant255": (with_quantisers(base, 255), False)}


def malformed_pack():
    """the malformed inputs of the sanitizer run: a 17 x 13 4:2:0 file truncated at every tenth byte position, 200 seeded single-byte
    corruptions of its scan, and a DHT whose counts overrun its segment.  -> [(name, bytes)]"""
    good = encode(noise(13, 17, 5), 85, 2)
    out = [("cut_%d" % n, good[:n]) for n in range(0, len(good), 10)]
    sos = good.index(b"\xff\xda")
    scan0 = sos + 2 + int.from_bytes(good[sos + 2:sos + 4], "big")
    r = np.random.default_rng(99)
    for k in range(200):
        b = bytearray(good)
        at = int(r.integers(scan0, len(good) - 2))
        b[at] ^= int(r.integers(1, 256))
        out.append(("flip_%d_at_%d" % (k, at), bytes(b)))
    dht = good.index(b"\xff\xc4")
    b = bytearray(good)
    for k in range(16):
        b[dht + 5 + k] = 255               # 4080 symbols claimed in a segment of a few dozen bytes
    out.append(("dht_overrun", bytes(b)))
    return good, out
