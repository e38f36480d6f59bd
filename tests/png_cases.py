"""The PNG files of the device decoder's tests, by name.  Accept cases are smooth gradients plus mild noise, so that they compress and
pass the room rule; noise_rgb() is the one file that does not."""
import io
import struct
import zlib

import numpy as np

import png_writer as pw

TYPES = (0, 2, 3, 4, 6)


def pixels(h, w, ctype, seed=0, noise=2):
    """(h, w, bpp) raw samples: gradients plus noise of a few levels (noise = 0: none); a palette image indexes 0..63"""
    rng = np.random.default_rng(1000 * seed + 10 * h + w + ctype)
    bpp = pw.BPP[ctype]
    y, x = np.mgrid[0:h, 0:w]
    px = np.zeros((h, w, bpp), np.int32)
    for c in range(bpp):
        px[..., c] = (3 * x + 2 * y * (c + 1) + 40 * c) % 256
    px += rng.integers(-noise, noise + 1, px.shape)
    if ctype == 3:
        return (px % 64).astype(np.uint8)
    return np.clip(px, 0, 255).astype(np.uint8)


def palette(n=64, seed=5):
    return np.random.default_rng(seed).integers(0, 256, 3 * n, dtype=np.uint8).tobytes()


def make(h, w, ctype, filters=(0, 1, 2, 3, 4), seed=0, noise=2, **kw):
    """a file of gradient pixels; a palette image gets a 64-entry PLTE (and kw may add tRNS)"""
    if ctype == 3 and "plte" not in kw:
        kw["plte"] = palette()
    return pw.png(pixels(h, w, ctype, seed, noise), ctype, filters, **kw)


def pil_rgb(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB")).copy()


def idat_stream(data):
    """the file's zlib stream and (h, w, bytes per pixel), read with struct alone"""
    i, z, head = 8, b"", None
    while i + 8 <= len(data):
        n, kind = struct.unpack(">I4s", data[i:i + 8])
        if kind == b"IHDR":
            w, h, _, ct = struct.unpack(">IIBB", data[i + 8:i + 18])
            head = (h, w, pw.BPP[ct])
        if kind == b"IDAT":
            z += data[i + 8:i + 8 + n]
        i += 12 + n
    return z, head


def noise_rgb(h=48, w=40):
    px = np.random.default_rng(7).integers(0, 256, (h, w, 3), dtype=np.uint8)
    return pw.png(px, 2, (0,), level=6)


def shape_cases():
    """every shape of the issue, across colour types and filters"""
    out = {}
    for ct in TYPES:
        out["1x1_t%d" % ct] = make(1, 1, ct)
        out["5x7_t%d" % ct] = make(5, 7, ct)
    out["1x7_t2"] = make(1, 7, 2, filters=(4,))
    out["7x1_t6"] = make(7, 1, 6)
    out["1x7_t3"] = make(1, 7, 3, filters=(3,))
    out["7x1_t0"] = make(7, 1, 0, filters=(4, 3, 2, 1, 0))
    for rows, ct in ((63, 0), (64, 2), (65, 6), (129, 4), (65, 3)):
        out["%dx33_t%d" % (rows, ct)] = make(rows, 33, ct, filters=(4, 3, 1, 2, 0, 4, 4))
    for ft in range(5):
        out["20x9_f%d" % ft] = make(20, 9, 2, filters=(ft,), seed=ft)
    out["200x160_rgb"] = make(200, 160, 2, level=6)              # 96 KB of scanlines: hundreds of rounds of the queue, back-references of up to 32 KiB
    return out


def zlib_cases():
    """levels, windows, strategies, flushes, IDAT cuts"""
    out = {}
    for level in (0, 1, 6, 9):
        out["level%d" % level] = make(40, 37, 2, level=level, seed=level)
    out["wbits9"] = make(40, 37, 6, level=6, wbits=9)
    for name, st in (("fixed", zlib.Z_FIXED), ("rle", zlib.Z_RLE), ("huffman_only", zlib.Z_HUFFMAN_ONLY)):
        out[name] = make(33, 29, 2, level=6, strategy=st)
    out["mem1"] = make(64, 64, 2, level=6, mem_level=1)
    # one stream of several block types with empty stored blocks between them, IDAT cut at every byte
    px = pixels(30, 31, 2, 3)
    scan = pw.filter_rows(px, (0, 1, 2, 3, 4))
    z = pw.deflate(scan, level=6, pieces=[(500, zlib.Z_SYNC_FLUSH), (0, zlib.Z_FULL_FLUSH), (700, zlib.Z_SYNC_FLUSH), (300, zlib.Z_FULL_FLUSH)])
    out["flushes_cut1"] = pw.png(px, 2, stream=z, idat_cut=1)
    out["cut7"] = make(25, 25, 4, idat_cut=7)
    out["empty_idats"] = _with_empty_idats(px, scan)
    return out


def _with_empty_idats(px, scan):
    z = pw.deflate(scan, level=6)
    h, w, _ = px.shape
    mid = len(z) // 2
    return (pw.SIG + pw.ihdr(h, w, 2) + pw.chunk(b"IDAT", b"") + pw.chunk(b"IDAT", z[:mid]) + pw.chunk(b"IDAT", b"") + pw.chunk(b"IDAT", z[mid:]) +
            pw.chunk(b"IDAT", b"") + pw.chunk(b"IEND"))


def _grey_file(scan, h, w, stream):
    assert len(scan) == h * (1 + w)
    px = np.zeros((h, w, 1), np.uint8)         # (the stream carries the scanlines; px only gives the size)
    return pw.png(px, 0, stream=stream)


def handmade_cases():
    """the streams zlib will not emit, each checked against zlib.decompress where it is built (png_writer.zlib_wrap)"""
    out = {}
    # a match of 258 at distance 32768: grey, 127 wide (scanlines of 128 bytes), 259 rows = 33152 bytes; filter bytes 0
    rng = np.random.default_rng(11)
    first = rng.integers(0, 256, 32768, dtype=np.uint8)
    first[0::128] = 0
    ops = [("lit", int(v)) for v in first] + [("match", 258, 32768)]
    tail = 259 * 128 - 32768 - 258
    ops += [("lit", (7 * k) % 256) for k in range(tail)]       # (none of them at a multiple of 128)
    out["far258"] = _grey_file(pw.expand(ops), 259, 127, pw.stream_fixed(ops))
    # distance 1: 7 rows of 37 bytes, all of them 1 (filter Sub, every difference 1)
    ops = [("lit", 1), ("match", 258, 1)]
    out["dist1"] = _grey_file(pw.expand(ops), 7, 36, pw.stream_fixed(ops))
    # a literal/length code of 15 bits: grey 21 x 20, sixteen values, filter 0
    y, x = np.mgrid[0:20, 0:21]
    g = ((x + 2 * y) % 16).astype(np.uint8)
    scan = pw.filter_rows(g[..., None], (0,))
    out["bits15"] = _grey_file(scan, 20, 21, pw.stream_15bit(scan))
    # rows of 16 bytes (RGB, 5 wide) repeated by matches of 16 at distance 16: one distance symbol
    row = bytes([0] + [(13 * k + 5) % 226 for k in range(15)])
    ops = [("lit", v) for v in row] + [("match", 16, 16)] * 6
    px = np.zeros((7, 5, 3), np.uint8)
    out["one_dist"] = pw.png(px, 2, stream=pw.stream_single_distance(ops))
    out["repeat_across"] = pw.png(px, 2, stream=pw.stream_repeat_across(ops))
    out["literals_only"] = pw.png(px, 2, stream=pw.stream_literals_only(pw.expand(ops)))
    return out


def palette_cases():
    px = pixels(9, 11, 3)
    out = {"plte64": pw.png(px, 3, (0, 4), plte=palette()), "plte_trns": pw.png(px, 3, (1, 2), plte=palette(), trns=bytes(range(0, 128, 2))),
           "plte256": pw.png(px, 3, (3,), plte=palette(256)), "grey_trns": pw.png(pixels(9, 11, 0), 0, (4,), trns=b"\x00\x10"),
           "rgb_trns": pw.png(pixels(9, 11, 2), 2, (4,), trns=b"\x00\x10\x00\x20\x00\x30"),
           "ancillary": pw.png(pixels(9, 11, 2), 2, (2,), before_idat=[pw.chunk(b"gAMA", b"\x00\x00\xb1\x8f"), pw.chunk(b"pHYs", b"\x00\x00\x0b\x13\x00\x00\x0b\x13\x01"),
                                                                      pw.chunk(b"tEXt", b"Comment\x00hello")], after_idat=[pw.chunk(b"tEXt", b"After\x00data")]),
           "no_iend": pw.png(pixels(9, 11, 2), 2, (1,), iend=False)}
    return out


def behind_idat_cases():
    """6 x 5 RGB files with chunks of every kind behind (and, for the CRC rule, in front of) IDAT: tests/test_png_native.py cuts them at
    every byte and holds the parser to being no laxer than Pillow"""
    px = pixels(6, 5, 2)
    text = pw.chunk(b"tEXt", b"After\x00some data here!")
    return {"text": pw.png(px, 2, (1,), after_idat=[text]), "plain": pw.png(px, 2, (1,)),
            "two": pw.png(px, 2, (1,), after_idat=[pw.chunk(b"tEXt", b"A\x00b"), pw.chunk(b"zTXt", b"A\x00\x00" + b"x" * 9)]),
            "critical_behind": pw.png(px, 2, (1,), after_idat=[pw.chunk(b"XXXX", b"abc")]),
            "critical_in_front": pw.png(px, 2, (1,), before_idat=[pw.chunk(b"XXXX", b"abc")]),
            "crc_behind": pw.png(px, 2, (1,), after_idat=[pw.chunk(b"tEXt", b"A\x00b", crc=5)]),
            "crc_in_front": pw.png(px, 2, (1,), before_idat=[pw.chunk(b"tEXt", b"A\x00b", crc=5)]),
            "iend_with_payload": pw.png(px, 2, (1,), iend=False) + pw.chunk(b"IEND", b"zz"),
            "junk_behind_iend": pw.png(px, 2, (1,)) + b"junkjunkjunkjunk",
            "half_a_header": pw.png(px, 2, (1,), iend=False) + b"\x00\x00\x00\x05ab",
            "exif_behind": pw.png(px, 2, (1,), after_idat=[pw.exif_chunk(6)])}


def accept_cases():
    out = {}
    for part in (shape_cases(), zlib_cases(), handmade_cases(), palette_cases()):
        out.update(part)
    return out


def refused_cases():
    """name -> (file, a word of its reason)"""
    px = pixels(6, 5, 2)
    good = pw.png(px, 2)
    z = pw.deflate(pw.filter_rows(px, (0,)))
    body = lambda head, *chunks: pw.SIG + head + b"".join(chunks) + pw.chunk(b"IEND")      # noqa: E731
    idat = pw.chunk(b"IDAT", z)
    out = {
        "depth16": (body(pw.ihdr(6, 5, 2, depth=16), idat), "bit depth"),
        "depth4": (body(pw.ihdr(6, 5, 0, depth=4), idat), "bit depth"),
        "adam7": (body(pw.ihdr(6, 5, 2, interlace=1), idat), "Adam7"),
        "apng": (body(pw.ihdr(6, 5, 2), pw.chunk(b"acTL", b"\x00\x00\x00\x01\x00\x00\x00\x00"), idat), "APNG"),
        "no_plte": (body(pw.ihdr(6, 5, 3), idat), "PLTE"),
        "ihdr_crc": (body(pw.ihdr(6, 5, 2, crc=0x12345678), idat), "CRC"),
        "plte_crc": (body(pw.ihdr(6, 5, 3), pw.chunk(b"PLTE", palette(), crc=1), idat), "CRC"),
        "overrun": (good[:len(good) - 30], "overruns"),
        "split_idat": (body(pw.ihdr(6, 5, 2), pw.chunk(b"IDAT", z[:10]), pw.chunk(b"tEXt", b"a\x00b"), pw.chunk(b"IDAT", z[10:])), "consecutive"),
        "no_idat": (body(pw.ihdr(6, 5, 2)), "no IDAT"),
        "zlib_dict": (body(pw.ihdr(6, 5, 2), pw.chunk(b"IDAT", b"\x78\xbb" + z[2:])), "deflate"),
        "zlib_method": (body(pw.ihdr(6, 5, 2), pw.chunk(b"IDAT", b"\x79\x9c" + z[2:])), "deflate"),
        "zlib_window": (body(pw.ihdr(6, 5, 2), pw.chunk(b"IDAT", b"\x88\x1c" + z[2:])), "deflate"),
        "too_wide": (body(pw.ihdr(6, 8193, 2), idat), "8192"),
        # a chunk behind IDAT whose header is whole and whose payload the file does not hold: Pillow raises "Truncated File Read"
        "cut_in_text_behind_idat": (behind_idat_cases()["text"][:-(12 + 10)], "overruns"),
        "ancillary_crc": (body(pw.ihdr(6, 5, 2), pw.chunk(b"gAMA", b"\x00\x00\xb1\x8f", crc=7), idat), "CRC"),
        "trns_crc": (body(pw.ihdr(6, 5, 2), pw.chunk(b"tRNS", b"\x00\x01\x00\x02\x00\x03", crc=7), idat), "CRC"),
    }
    assert 0x78bb % 31 == 0 and 0x881c % 31 == 0          # (their check bits are right: only the dictionary flag / the window is wrong)
    return out


def fuzz_file():
    """the fixed file of the mutation test: RGB 24 x 20, all five filters, level 6, ONE IDAT chunk"""
    return make(24, 20, 2, level=6, seed=9)


FUZZ_SEED = 20240229


def corrupt_cases():
    """name -> a 24 x 20 RGB file whose DATA is wrong in one way: what the parser accepts and the decoder must flag"""
    px = pixels(24, 20, 2, 9)
    scan = pw.filter_rows(px, (0, 1, 2, 3, 4))
    z = pw.deflate(scan, level=6)
    file_of = lambda stream: pw.png(px, 2, stream=stream)      # noqa: E731
    bad_filter = bytearray(scan)
    bad_filter[61 * 7] = 5
    b = pw.Bits()                       # a dynamic block whose code-length code has no code at all
    for v, n in ((1, 1), (2, 2), (0, 5), (0, 5), (0, 4)) + ((0, 3),) * 4:
        b.put(v, n)
    far = pw.Bits()                     # a fixed block that starts with a match: nothing to copy from
    far.put(1, 1); far.put(1, 2); far.code(0b0000001, 7); far.code(0, 5)       # noqa: E702
    sym286 = pw.Bits()                  # a fixed block with literal/length symbol 286
    sym286.put(1, 1); sym286.put(1, 2); sym286.code(0b11000110, 8)             # noqa: E702
    return {
        "truncated": file_of(z[:len(z) // 2]),
        "block_type3": file_of(b"\x78\x9c\x07" + z[3:]),
        "stored_len": file_of(b"\x78\x9c\x01\x05\x00\x00\x00" + z[7:]),
        "no_codelen_code": file_of(b"\x78\x9c" + b.bytes() + z[8:]),
        "symbol_286": file_of(b"\x78\x9c" + sym286.bytes() + z[8:]),
        "distance_too_far": file_of(b"\x78\x9c" + far.bytes() + z[8:]),
        "too_long": file_of(pw.deflate(scan + b"\x00" * 7)),
        "too_short": file_of(pw.deflate(scan[:-61])),
        "adler": file_of(z[:-1] + bytes([z[-1] ^ 1])),
        "filter_byte_5": file_of(pw.deflate(bytes(bad_filter))),
    }
