"""PNG files written by hand for the device decoder's tests: chunks, a filter type per row (all five, the filtering in numpy), the
zlib stream from zlib.compressobj with any level / window / strategy and flushes between pieces, IDAT cut every k bytes, and a small
deflate bit writer for the streams zlib will not emit.  Nothing here reads a PNG: Pillow and zlib.decompress are the judges."""
import struct
import zlib

import numpy as np

SIG = b"\x89PNG\r\n\x1a\n"
BPP = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}


def chunk(kind, data=b"", crc=None):
    c = zlib.crc32(kind + data) & 0xFFFFFFFF if crc is None else crc
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", c)


def ihdr(h, w, ctype, depth=8, interlace=0, crc=None):
    return chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, interlace), crc)


def exif_chunk(orientation, big_endian=False):
    """an eXIf chunk whose IFD0 holds the orientation tag alone"""
    e = ">" if big_endian else "<"
    tiff = (b"MM" if big_endian else b"II") + struct.pack(e + "HI", 42, 8) + struct.pack(e + "H", 1) + struct.pack(e + "HHIHH", 0x0112, 3, 1, orientation, 0) + struct.pack(e + "I", 0)
    return chunk(b"eXIf", tiff)


def filter_rows(px, filters):
    """px: (h, w, bpp) uint8 raw samples; filters: one type 0..4 per row -> the filtered scanlines, each led by its filter byte"""
    h, w, bpp = px.shape
    raw = px.reshape(h, w * bpp).astype(np.int32)
    out = np.zeros((h, 1 + w * bpp), np.uint8)
    zero = np.zeros(w * bpp, np.int32)
    for y in range(h):
        cur, up = raw[y], raw[y - 1] if y else zero
        left = np.concatenate([np.zeros(bpp, np.int32), cur[:-bpp]]) if w * bpp > bpp else np.zeros(w * bpp, np.int32)
        upleft = np.concatenate([np.zeros(bpp, np.int32), up[:-bpp]]) if w * bpp > bpp else np.zeros(w * bpp, np.int32)
        ft = int(filters[y % len(filters)])
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
        out[y, 0] = ft
        out[y, 1:] = (cur - pred) & 255
    return out.tobytes()


def deflate(data, level=6, wbits=15, mem_level=8, strategy=zlib.Z_DEFAULT_STRATEGY, pieces=None):
    """the zlib stream of data; pieces: [(bytes, flush mode or None), ...] cut points with a flush behind each piece"""
    c = zlib.compressobj(level, zlib.DEFLATED, wbits, mem_level, strategy)
    if pieces is None:
        return c.compress(data) + c.flush()
    out, at = b"", 0
    for n, mode in pieces:
        out += c.compress(data[at:at + n])
        at += n
        if mode is not None:
            out += c.flush(mode)
    return out + c.compress(data[at:]) + c.flush()


def png(px, ctype, filters=(0,), stream=None, idat_cut=None, plte=None, trns=None, before_idat=(), after_idat=(), iend=True, **zargs):
    """px: (h, w, bpp) uint8.  stream: the zlib stream to carry in place of the scanlines' own (the bit writer's)."""
    h, w, bpp = px.shape
    assert bpp == BPP[ctype]
    z = stream if stream is not None else deflate(filter_rows(px, filters), **zargs)
    out = SIG + ihdr(h, w, ctype)
    if plte is not None:
        out += chunk(b"PLTE", bytes(plte))
    if trns is not None:
        out += chunk(b"tRNS", bytes(trns))
    for c in before_idat:
        out += c
    if idat_cut:
        for i in range(0, len(z), idat_cut):
            out += chunk(b"IDAT", z[i:i + idat_cut])
    else:
        out += chunk(b"IDAT", z)
    for c in after_idat:
        out += c
    return out + (chunk(b"IEND") if iend else b"")


# ---- a deflate bit writer for the streams zlib will not emit -------------------------------------------------------------------------
class Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, n):                   # n bits of v, least significant first (header fields, extra bits)
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, n):                  # a Huffman code: most significant bit first
        for k in range(n - 1, -1, -1):
            self.put(c >> k & 1, 1)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def bytes(self):
        self.align()
        return bytes(self.out)


def canonical(lens):
    """code lengths -> {symbol: (code, length)} by RFC 1951 3.2.2"""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    code, nxt = 0, [0] * 16
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = {}
    for s, l in enumerate(lens):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


def len_sym(n):
    i = max(k for k in range(29) if LEN_BASE[k] <= n) if n < 258 else 28
    return 257 + i, n - LEN_BASE[i], LEN_EXTRA[i]


def dist_sym(d):
    i = max(k for k in range(30) if DIST_BASE[k] <= d)
    return i, d - DIST_BASE[i], DIST_EXTRA[i]


ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def dynamic_block(b, ops, lit_lens, dist_lens, final=True, cl_ops=None):
    """One dynamic block.  ops: ('lit', v) | ('match', length, distance); lit_lens (>= 257 entries) and dist_lens (>= 1) are written as
    given, so they may be incomplete where zlib allows it.  cl_ops: the code-length symbols to send, [(symbol, extra value)], in place
    of one symbol per length -- repeat codes that run from the literal lengths into the distance lengths."""
    hlit, hdist = len(lit_lens), len(dist_lens)
    seq = cl_ops if cl_ops is not None else [(l, 0) for l in list(lit_lens) + list(dist_lens)]
    used = sorted({s for s, _ in seq})
    # a complete code over the code-length symbols in use: lengths from a balanced tree
    cl_lens = [0] * 19
    n = len(used)
    if n == 1:
        used.append(0 if used[0] != 0 else 1)
        n = 2
    depth = max(1, (n - 1).bit_length())
    short = (1 << depth) - n                    # symbols that may be one bit shorter
    for k, s in enumerate(used):
        cl_lens[s] = depth - 1 if k < short and depth > 1 else depth
    assert sum(2.0 ** -l for l in cl_lens if l) == 1.0 and max(cl_lens) <= 7
    clc = canonical(cl_lens)
    b.put(1 if final else 0, 1)
    b.put(2, 2)
    b.put(hlit - 257, 5)
    b.put(hdist - 1, 5)
    hclen = max(k for k in range(19) if cl_lens[ORDER[k]]) + 1
    hclen = max(hclen, 4)
    b.put(hclen - 4, 4)
    for k in range(hclen):
        b.put(cl_lens[ORDER[k]], 3)
    for s, extra in seq:
        b.code(*clc[s])
        if s == 16:
            b.put(extra, 2)
        elif s == 17:
            b.put(extra, 3)
        elif s == 18:
            b.put(extra, 7)
    lc, dc = canonical(lit_lens), canonical(dist_lens)
    for op in ops:
        if op[0] == "lit":
            b.code(*lc[op[1]])
        else:
            s, ev, eb = len_sym(op[1])
            b.code(*lc[s])
            b.put(ev, eb)
            d, ev, eb = dist_sym(op[2])
            b.code(*dc[d])
            b.put(ev, eb)
    b.code(*lc[256])


def expand(ops):
    out = bytearray()
    for op in ops:
        if op[0] == "lit":
            out.append(op[1])
        else:
            for _ in range(op[1]):
                out.append(out[-op[2]])
    return bytes(out)


def zlib_wrap(deflate_bytes, data):
    z = b"\x78\x9c" + deflate_bytes + struct.pack(">I", zlib.adler32(data) & 0xFFFFFFFF)
    assert zlib.decompress(z) == data          # every hand-made stream is first checked against zlib on the CPU
    return z


def stream_15bit(data):
    """a dynamic block, literals only, whose literal/length code reaches 15 bits.  The data has 15 or 16 distinct values; they and symbol
    256 get a complete code: a chain of lengths 1, 2, ..., 13 and the last two to four symbols below what the chain leaves"""
    syms = sorted(set(data)) + [256]
    assert 16 <= len(syms) <= 17                # (with fewer the tail would stop at 14 bits)
    lens = [0] * 257
    chain, rest = syms[:13], syms[13:]
    for k, s in enumerate(chain):
        lens[s] = k + 1
    short = 4 - len(rest)                       # the chain leaves 2^-13: four codes of 15 bits, or fewer with 14-bit ones among them
    for k, s in enumerate(rest):
        lens[s] = 14 if k < short else 15
    assert max(lens) == 15 and abs(sum(2.0 ** -l for l in lens if l) - 1.0) < 1e-12
    b = Bits()
    dynamic_block(b, [("lit", v) for v in data], lens, [0])          # HDIST's one code, of length zero
    return zlib_wrap(b.bytes(), bytes(data))


def stream_single_distance(ops):
    """a dynamic block whose distance code is ONE code of one bit (incomplete, allowed by zlib); every match uses that distance symbol"""
    data = expand(ops)
    dsyms = {dist_sym(op[2])[0] for op in ops if op[0] == "match"}
    assert len(dsyms) == 1
    dist_lens = [0] * (max(dsyms) + 1)
    dist_lens[max(dsyms)] = 1
    lit_lens = [8] * 226 + [9] * 60                                  # 226 / 256 + 60 / 512 = 1: complete over all 286 symbols
    b = Bits()
    dynamic_block(b, ops, lit_lens, dist_lens)
    return zlib_wrap(b.bytes(), data)


def stream_literals_only(data):
    """a dynamic block of literals with HDIST = 1 and that one distance length zero"""
    lit_lens = [8] * 255 + [9] * 2                                   # 255 / 256 + 2 / 512 = 1
    b = Bits()
    dynamic_block(b, [("lit", v) for v in data], lit_lens, [0])
    return zlib_wrap(b.bytes(), bytes(data))


def stream_repeat_across(ops):
    """code lengths sent with a repeat code that runs from the literal lengths into the distance lengths: the run that crosses is of
    ZEROS -- length 0 for literal symbols 280..285 and for distance symbols 0..3 -- sent as ONE code 17 of ten."""
    data = expand(ops)
    lit_lens = [8] * 232 + [9] * 48 + [0] * 6                        # 232 / 256 + 48 / 512 = 1; symbols 280..285 unused
    dist_lens = [0] * 4 + [2, 2, 2, 2]                               # distance symbols 4..7 (distances 5..16), complete
    assert all(len_sym(op[1])[0] < 280 and 4 <= dist_sym(op[2])[0] <= 7 for op in ops if op[0] == "match")
    cl = [(8, 0)] * 232 + [(9, 0)] * 48 + [(17, 10 - 3)] + [(2, 0)] * 4     # 17: ten zeros = 6 literal lengths + 4 distance lengths
    b = Bits()
    dynamic_block(b, ops, lit_lens, dist_lens, cl_ops=cl)
    return zlib_wrap(b.bytes(), data)


def stream_fixed(ops, final=True):
    """a fixed block of the ops (any length / distance)"""
    b = Bits()
    b.put(1 if final else 0, 1)
    b.put(1, 2)
    lens = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
    lc = canonical(lens)
    for op in ops:
        if op[0] == "lit":
            b.code(*lc[op[1]])
        else:
            s, ev, eb = len_sym(op[1])
            b.code(*lc[s])
            b.put(ev, eb)
            d, ev, eb = dist_sym(op[2])
            b.code(d, 5)
            b.put(ev, eb)
    b.code(*lc[256])
    return zlib_wrap(b.bytes(), expand(ops))
