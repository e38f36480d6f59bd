"""JPEG uploads with EXIF orientations for the upload-job tests: Pillow-written files (Pillow writes a big-endian `MM` block), a
hand-built little-endian `II` block, and the broken blocks that must read as orientation 1.  Test infrastructure."""
import io
import struct

import numpy as np
from PIL import Image


def smooth(h, w, seed):
    """a smooth colour image with some texture: compresses well below its pixels, yet every orientation gives other bytes"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    f = rng.uniform(0.02, 0.09, (3, 2))
    p = rng.uniform(0, 6.28, (3, 2))
    ch = [127 + 70 * np.sin(f[c, 0] * x + p[c, 0]) + 50 * np.cos(f[c, 1] * y + p[c, 1]) + 0.15 * (x - y) for c in range(3)]
    return np.clip(np.stack(ch, -1) + rng.normal(0, 2.0, (h, w, 3)), 0, 255).astype(np.uint8)


def exif_block(orientation=6, le=False, entries=None, ifd_off=8, cut=None):
    """the payload of an APP1 segment: b'Exif\\0\\0' + a TIFF header + IFD0.  entries: [(tag, type, count, value)], default the
    orientation tag alone (SHORT, count 1); ifd_off: what the header claims (the IFD itself always follows the header); cut: keep
    only so many bytes of the block."""
    e = "<" if le else ">"
    if entries is None:
        entries = [(0x0112, 3, 1, orientation)]
    tiff = (b"II" if le else b"MM") + struct.pack(e + "HI", 42, ifd_off) + struct.pack(e + "H", len(entries))
    for tag, typ, count, value in entries:
        tiff += struct.pack(e + "HHI", tag, typ, count) + (struct.pack(e + "HH", value, 0) if typ == 3 else struct.pack(e + "I", value))
    tiff += struct.pack(e + "I", 0)
    blk = b"Exif\0\0" + tiff
    return blk if cut is None else blk[:cut]


def encode(px, quality=85, subsampling=0, orientation=None, progressive=False, app1=None):
    """pixels ([h,w,3], or [h,w] grey) -> a JPEG file.  orientation: written by Pillow through exif= (an `MM` block); app1: the payload
    of an APP1 segment spliced in behind SOI by hand (any bytes)."""
    im = Image.fromarray(px)
    kw = dict(quality=quality, progressive=progressive)
    if px.ndim == 3:
        kw["subsampling"] = subsampling
    if orientation is not None:
        ex = Image.Exif()
        ex[0x0112] = orientation
        kw["exif"] = ex.tobytes()
    b = io.BytesIO()
    im.save(b, "JPEG", **kw)
    data = b.getvalue()
    if app1 is not None:
        data = data[:2] + b"\xff\xe1" + struct.pack(">H", len(app1) + 2) + app1 + data[2:]
    return data


def pillow_pixels(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def pillow_orientation(data):
    return Image.open(io.BytesIO(data)).getexif().get(0x0112, 1)
