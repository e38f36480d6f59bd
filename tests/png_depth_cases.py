"""PNG files of every form beside "8 bits, not interlaced", written by hand for the tests of IRE_FLAG_DECODE_PNG_ALL: samples of 1, 2, 4,
8 and 16 bits packed from the most significant bit down, the seven Adam7 passes cut out of the image, every pass filtered on its own
(all five filter types, the unit of max(1, bits per pixel / 8) bytes, a row of zeros above its first row), the passes' scanlines back
to back in one zlib stream.  Nothing here reads a PNG: Pillow and zlib.decompress are the judges."""
import io
import zlib

import numpy as np

from png_writer import SIG, chunk, deflate, ihdr

CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
# every (colour type, depth) pair the device takes with the accept-all bit
FORMS = [(0, 1), (0, 2), (0, 4), (0, 8), (3, 1), (3, 2), (3, 4), (3, 8), (2, 8), (2, 16), (4, 8), (4, 16), (6, 8), (6, 16)]
ADAM7 = [(0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2)]      # x0, y0, dx, dy
ACCEPT_ALL = 32
FLAG_PNG, FLAG_PNG_ALL = 1024, 8192


def passes(h, w, ctype, depth, interlace):
    """[(x0, y0, dx, dy, pw, ph, row_bytes)] of the passes that have a pixel, in stream order"""
    bits = CHANNELS[ctype] * depth
    out = []
    for x0, y0, dx, dy in (ADAM7 if interlace else [(0, 0, 1, 1)]):
        pw, ph = (w - x0 + dx - 1) // dx if w > x0 else 0, (h - y0 + dy - 1) // dy if h > y0 else 0
        if pw and ph:
            out.append((x0, y0, dx, dy, pw, ph, (pw * bits + 7) // 8))
    return out


def scan_bytes(h, w, ctype, depth, interlace):
    return sum(ph * (1 + rb) for *_, ph, rb in passes(h, w, ctype, depth, interlace))


def filter_offsets(h, w, ctype, depth, interlace):
    """where the filter bytes lie in the stream"""
    out, at = [], 0
    for *_, ph, rb in passes(h, w, ctype, depth, interlace):
        out += [at + r * (1 + rb) for r in range(ph)]
        at += ph * (1 + rb)
    return out


def pack_rows(s, depth):
    """s: (rows, cols, channels) samples below 2^depth -> (rows, row_bytes) uint8, packed from the most significant bit down"""
    rows = s.shape[0]
    flat = s.reshape(rows, -1).astype(np.uint32)
    if depth == 16:
        return np.stack([flat >> 8, flat & 255], axis=-1).reshape(rows, -1).astype(np.uint8)
    if depth == 8:
        return flat.astype(np.uint8)
    bits = ((flat[..., None] >> np.arange(depth - 1, -1, -1)) & 1).reshape(rows, -1).astype(np.uint8)
    return np.packbits(bits, axis=1)          # (zero bits fill the last byte)


def filter_pass(raw, unit, filters, first):
    """raw: (rows, row_bytes) uint8 of ONE pass; row r gets filter type filters[(first + r) % len]; the row above row 0 is zeros"""
    rows, n = raw.shape
    r32 = raw.astype(np.int32)
    out = bytearray()
    zero = np.zeros(n, np.int32)
    for y in range(rows):
        cur, up = r32[y], r32[y - 1] if y else zero
        left, upleft = zero.copy(), zero.copy()
        left[unit:], upleft[unit:] = cur[:n - unit] if n > unit else [], up[:n - unit] if n > unit else []
        ft = int(filters[(first + y) % len(filters)])
        if ft == 0:
            pred = zero
        elif ft == 1:
            pred = left
        elif ft == 2:
            pred = up
        elif ft == 3:
            pred = (left + up) >> 1
        else:
            p = left + up - upleft
            pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - upleft)
            pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, upleft))
        out.append(ft)
        out += ((cur - pred) & 255).astype(np.uint8).tobytes()
    return bytes(out)


def scanlines(s, ctype, depth, interlace, filters):
    """the stream's plain bytes: every pass that has a pixel, filtered on its own; pass k starts its filters at filters[k]"""
    h, w, _ = s.shape
    unit = max(1, CHANNELS[ctype] * depth // 8)
    out = b""
    for k, (x0, y0, dx, dy, pw, ph, rb) in enumerate(passes(h, w, ctype, depth, interlace)):
        raw = pack_rows(s[y0::dy, x0::dx], depth)
        assert raw.shape == (ph, rb)
        out += filter_pass(raw, unit, filters, k)
    return out


def png_any(s, ctype, depth, interlace=0, filters=(0, 1, 2, 3, 4), plte=None, trns=None, before_idat=(), stream=None, **zargs):
    """s: (h, w, channels) samples.  stream: the zlib stream to carry in place of the scanlines' own"""
    h, w, ch = s.shape
    assert ch == CHANNELS[ctype] and int(s.max()) < (1 << depth)
    z = stream if stream is not None else deflate(scanlines(s, ctype, depth, interlace, filters), **zargs)
    out = SIG + ihdr(h, w, ctype, depth=depth, interlace=interlace)
    if plte is not None:
        out += chunk(b"PLTE", bytes(plte))
    if trns is not None:
        out += chunk(b"tRNS", bytes(trns))
    for c in before_idat:
        out += c
    return out + chunk(b"IDAT", z) + chunk(b"IEND")


def samples(h, w, ctype, depth, seed=0, top=None, smooth=False):
    """gradients plus a little noise; a 16-bit sample's LOW byte is noise, so that taking the wrong byte shows (smooth: no noise, and 255 - the
    high byte for the low one, for a file that has to compress below its pixels: the upload jobs' room rule).  top: samples stay below it"""
    rng = np.random.default_rng(1000 * seed + 100 * depth + 10 * h + w + ctype)
    ch = CHANNELS[ctype]
    y, x = np.mgrid[0:h, 0:w]
    s = np.zeros((h, w, ch), np.int64)
    for c in range(ch):
        s[..., c] = 3 * x + 2 * y * (c + 1) + 40 * c
    if not smooth:
        s += rng.integers(-1, 2, s.shape)
    if depth == 16:
        return ((s % 256) << 8 | (255 - s % 256 if smooth else rng.integers(0, 256, s.shape))).astype(np.uint32)
    return (s % (top or (1 << depth))).astype(np.uint32)


def palette(n, seed=5):
    return np.random.default_rng(seed).integers(1, 256, 3 * n, dtype=np.uint8).tobytes()      # (no black entry: an index past the end shows)


def make(h, w, ctype, depth, interlace=0, filters=(0, 1, 2, 3, 4), seed=0, smooth=False, **kw):
    if ctype == 3 and "plte" not in kw:
        kw["plte"] = palette(min(1 << depth, 64))
    return png_any(samples(h, w, ctype, depth, seed, 64 if (ctype == 3 and depth == 8) else None, smooth), ctype, depth, interlace, filters, **kw)


def carry_file(interlace, filters):
    """16-bit RGBA, 9 x 9: every byte of the 8-byte unit one of 0x00, 0x01, 0x7f, 0x80, 0xfe, 0xff on its own, so that Average's halving
    and Paeth's three distances differ from byte to byte of one unit: a carry from one byte into the next would show"""
    rng = np.random.default_rng(77)
    b = rng.choice(np.array([0x00, 0x01, 0x7F, 0x80, 0xFE, 0xFF]), (9, 9, 4, 2))
    b[0, :, :, :] = np.where(np.arange(8).reshape(4, 2) % 2 == 0, 0xFF, 0x01)      # a = 0xff.., b = 0x01.. patterns along the first rows
    b[1, :, :, :] = np.where(np.arange(8).reshape(4, 2) % 2 == 0, 0x01, 0xFF)
    s = (b[..., 0].astype(np.uint32) << 8 | b[..., 1]).astype(np.uint32)
    return png_any(s, 6, 16, interlace, filters)


SMALL = [(1, 1), (1, 2), (3, 2), (2, 5), (5, 3)]          # h x w: in every one of them some Adam7 passes are empty


def form_cases():
    """every accepted form, with and without interlace, at the five small sizes"""
    out = {}
    for ct, d in FORMS:
        for lace in (0, 1):
            for h, w in SMALL:
                if lace == 0 and d == 8:
                    continue          # (the form the decoder always took: tests/png_cases.py)
                out["t%d_d%d_i%d_%dx%d" % (ct, d, lace, h, w)] = make(h, w, ct, d, lace, seed=h + w)
    return out


def edge_cases():
    out = {}
    # a partial last byte at every sub-8 depth
    for ct, d in FORMS:
        if d < 8:
            for w in (9, 17, 70):
                for lace in (0, 1):
                    out["partial_t%d_d%d_i%d_w%d" % (ct, d, lace, w)] = make(5, w, ct, d, lace, seed=w)
    # 70 eight-byte units: more than the 64 lanes of the wavefront
    for lace in (0, 1):
        out["wave_rgba16_i%d_33x70" % lace] = make(33, 70, 6, 16, lace, seed=3)
    # more than 64 rows in one pass: the band hand-off (131 rows: Adam7's pass 7 has 65; 521 rows: its pass 1 has 66)
    for ct, d in ((2, 16), (6, 16), (0, 2), (3, 4), (0, 1)):
        out["band_t%d_d%d_i0_131x9" % (ct, d)] = make(131, 9, ct, d, 0, filters=(4, 3, 1, 2, 0, 4, 4), seed=1)
        out["band_t%d_d%d_i1_131x9" % (ct, d)] = make(131, 9, ct, d, 1, filters=(4, 3, 1, 2, 0, 4, 4), seed=2)
    out["band_t2_d8_i1_131x9"] = make(131, 9, 2, 8, 1, filters=(4, 3, 1, 2, 0, 4, 4), seed=2)
    out["band_t0_d1_i1_521x9"] = make(521, 9, 0, 1, 1, filters=(4, 3, 2), seed=4)
    out["band_t3_d1_i1_521x9"] = make(521, 9, 3, 1, 1, filters=(2, 4, 3), seed=4)
    # filters 2, 3 and 4 on the FIRST row of every pass: its row above is zeros, not the last row of the pass before
    for ft in (2, 3, 4):
        for ct, d in ((6, 16), (3, 4), (2, 8), (0, 1), (4, 16)):
            out["first_f%d_t%d_d%d" % (ft, ct, d)] = make(9, 9, ct, d, 1, filters=(ft,), seed=ft)
    # Average and Paeth on units whose bytes carry on their own
    for ft in (3, 4):
        for lace in (0, 1):
            out["carry_f%d_i%d" % (ft, lace)] = carry_file(lace, (ft,))
    # a palette shorter than 2^depth, with indices past its end; one longer than 2^depth
    for d, n in ((1, 1), (2, 3), (4, 5)):
        for lace in (0, 1):
            out["short_plte_d%d_i%d" % (d, lace)] = png_any(samples(5, 9, 3, d, 8), 3, d, lace, plte=palette(n))
    out["long_plte_d2"] = png_any(samples(5, 9, 3, 2, 8), 3, 2, 1, plte=palette(200))
    # tRNS: read past
    out["trns_plte_d2"] = png_any(samples(5, 9, 3, 2, 9), 3, 2, 1, plte=palette(4), trns=b"\x00\x80\xff")
    out["trns_grey_d1"] = png_any(samples(5, 9, 0, 1, 9), 0, 1, 0, trns=b"\x00\x01")
    out["trns_rgb_d16"] = png_any(samples(5, 9, 2, 16, 9), 2, 16, 1, trns=b"\x12\x34\x00\x10\xff\xff")
    return out


def accept_cases():
    out = form_cases()
    out.update(edge_cases())
    return out


def refused_cases():
    """name -> (file, a word of its reason WITH the accept-all bit, a word of its reason WITHOUT it)"""
    z = deflate(b"\x00" * 400)
    body = lambda head: SIG + head + chunk(b"PLTE", palette(4)) + chunk(b"IDAT", z) + chunk(b"IEND")      # noqa: E731
    out = {"grey16": (body(ihdr(6, 5, 0, depth=16)), "16-bit grey", "bit depth"),
           "grey16_adam7": (body(ihdr(6, 5, 0, depth=16, interlace=1)), "16-bit grey", "bit depth"),
           "palette16": (body(ihdr(6, 5, 3, depth=16)), "16-bit palette", "bit depth"),
           "interlace2": (body(ihdr(6, 5, 2, interlace=2)), "interlace method", "Adam7"),
           "type5": (body(ihdr(6, 5, 5, depth=4)), "colour type", "bit depth")}
    for ct, d in ((2, 1), (2, 2), (2, 4), (4, 1), (4, 2), (4, 4), (6, 1), (6, 2), (6, 4)):
        out["t%d_d%d" % (ct, d)] = (body(ihdr(6, 5, ct, depth=d)), "below 8", "bit depth")
    for d in (0, 3, 5, 7, 12, 32):
        out["depth%d" % d] = (body(ihdr(6, 5, 0, depth=d)), "none of 1, 2, 4, 8 and 16", "bit depth")
    return out


def old_reason_word(ctype, depth, interlace):
    """a word of the reason an engine WITHOUT the accept-all bit gives a file of a new form (csrc/png_parse.hpp checks the depth first)"""
    return "bit depth other than 8" if depth != 8 else "Adam7 interlacing"


def head_of(data):
    """(h, w, colour type, depth, interlace) from the IHDR, read with struct alone"""
    import struct
    w, h, d, ct, _, _, lace = struct.unpack(">IIBBBBB", data[16:29])
    return h, w, ct, d, lace


def idat_stream(data):
    import struct
    i, z = 8, b""
    while i + 8 <= len(data):
        n, kind = struct.unpack(">I4s", data[i:i + 8])
        if kind == b"IDAT":
            z += data[i + 8:i + 8 + n]
        i += 12 + n
    return z


def zlib_says_ok(z, head):
    """the three-part rule of status 0, with stdlib zlib -> (ok, zlib rejects)"""
    h, w, ct, d, lace = head
    try:
        got = zlib.decompress(z)
    except zlib.error:
        return False, True
    return len(got) == scan_bytes(h, w, ct, d, lace) and all(got[o] <= 4 for o in filter_offsets(h, w, ct, d, lace)), False


def pil_rgb(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB")).copy()


def fuzz_files():
    """the two files of the mutation test: Adam7 4-bit palette and 16-bit RGB, 24 x 20, all five filters, ONE IDAT chunk"""
    return {"adam7_plte4": make(24, 20, 3, 4, 1, seed=9, level=6), "rgb16": make(24, 20, 2, 16, 0, seed=9, level=6)}


FUZZ_SEED = 20240917


def bad_filter_adam7():
    """a 24 x 20 Adam7 2-bit grey file whose pass 3 (the third in the stream) starts with filter byte 5: what the parser accepts and the
    unfilter kernel must flag"""
    s = samples(24, 20, 0, 2, 6)
    scan = bytearray(scanlines(s, 0, 2, 1, (0, 1, 2, 3, 4)))
    ps = passes(24, 20, 0, 2, 1)
    at = sum(ph * (1 + rb) for *_, ph, rb in ps[:2])
    assert scan[at] <= 4
    scan[at] = 5
    return png_any(s, 0, 2, 1, stream=deflate(bytes(scan))), png_any(s, 0, 2, 1)
