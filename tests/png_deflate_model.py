"""The specification of the device's compressing PNG encoder (csrc/deflate.hip) as a Python model: stdlib + numpy, no product code.

    file   = signature | IHDR (8-bit RGB) | ONE IDAT | IEND
    IDAT   = zlib header 78 01 | one deflate block per 32 768 bytes of the filtered stream | Adler-32 of the filtered stream
    filter = type 4 (Paeth) on every scanline, 3 bytes per pixel
    block  = BTYPE 2 (dynamic Huffman), literals + end-of-block only:
             HLIT = 257 codes, HDIST = 2 codes of one bit (what zlib writes for literal-only data), the 259 code lengths sent
             one by one with the code-length alphabet's symbols 0..15 (the run-length symbols 16..18 are NOT used);
             literal codes: optimal under the 15-bit limit (package-merge), code-length codes: optimal under the 7-bit limit;
             every block but the last is followed by an empty stored block (000 + padding, 00 00 FF FF), so that the next block
             starts on a byte boundary; the last block is padded to a byte.

The construction of the code lengths is the device's algorithm step by step, ties included: symbols of non-zero count sorted by
(count, symbol); package-merge over `maxbits` levels in which, among equal weights, a leaf goes before a package; a symbol's length
is the number of levels whose selection holds its leaf.  Adler-32, CRC-32 and base64 come from zlib / base64.

The model is held to the published formats by independent decoders (tests/test_png_deflate_model.py); the device is held to the
model byte for byte (tests/test_png_deflate_gpu.py)."""
import base64
import bisect
import struct
import zlib

import numpy as np

BLOCK = 32768
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
HEADER_BITS_MAX = 3 + 5 + 5 + 4 + 19 * 3 + 259 * 7          # 1887: what a block can spend before its first symbol


# ---- scanline filter ---------------------------------------------------------------------------------------------------------------
def _paeth_predictor(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def paeth_filter(px):
    """[h][w][3] uint8 -> the filtered stream, h * (1 + 3 w) bytes (filter-type bytes included)."""
    px = np.ascontiguousarray(px, np.uint8)
    h, w, _ = px.shape
    cur = px.reshape(h, 3 * w).astype(np.int32)
    a = np.zeros_like(cur); a[:, 3:] = cur[:, :-3]
    b = np.zeros_like(cur); b[1:] = cur[:-1]
    c = np.zeros_like(cur); c[1:, 3:] = cur[:-1, :-3]
    out = np.empty((h, 1 + 3 * w), np.uint8)
    out[:, 0] = 4
    out[:, 1:] = (cur - _paeth_predictor(a, b, c)) & 0xFF
    return out.tobytes()


def paeth_unfilter(stream, h, w):
    """The inverse of paeth_filter (a bijection on the 3 w h residual bytes): any residual stream is some image's."""
    rows = np.frombuffer(stream, np.uint8).reshape(h, 1 + 3 * w)
    assert (rows[:, 0] == 4).all()
    out = np.zeros((h, 3 * w), np.int64)
    for y in range(h):
        for x in range(3 * w):
            a = out[y, x - 3] if x >= 3 else 0
            b = out[y - 1, x] if y else 0
            c = out[y - 1, x - 3] if (y and x >= 3) else 0
            p = a + b - c
            pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
            pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
            out[y, x] = (int(rows[y, 1 + x]) + pred) & 0xFF
    return out.astype(np.uint8).reshape(h, w, 3)


# ---- length-limited optimal codes: package-merge --------------------------------------------------------------------------------------
def limited_lengths(counts, maxbits):
    """counts[s] -> lengths[s] (0 for count 0), every length <= maxbits, minimal sum(count * length).  >= 2 symbols must be used."""
    syms = sorted((s for s, c in enumerate(counts) if c > 0), key=lambda s: (counts[s], s))
    n = len(syms)
    assert n >= 2 and (1 << maxbits) >= n
    leaf = [int(counts[s]) for s in syms]
    cur = leaf[:]                                   # level 0 (the deepest): the leaves alone
    leafpos = [list(range(n))]
    for _ in range(1, maxbits):
        pk = [cur[2 * k] + cur[2 * k + 1] for k in range(len(cur) // 2)]
        pos = [r + bisect.bisect_left(pk, leaf[r]) for r in range(n)]             # packages lighter than the leaf go before it
        nxt = [0] * (n + len(pk))
        for r in range(n):
            nxt[pos[r]] = leaf[r]
        for k, v in enumerate(pk):
            nxt[k + bisect.bisect_right(leaf, v)] = v                             # a leaf of equal weight goes before the package
        cur = nxt
        leafpos.append(pos)
    length = [0] * n
    take = 2 * n - 2
    for j in range(maxbits - 1, -1, -1):
        a = bisect.bisect_left(leafpos[j], take)                                   # leaves among the first `take` items of level j
        for r in range(a):
            length[r] += 1
        take = 2 * (take - a)
    out = [0] * len(counts)
    for r, s in enumerate(syms):
        out[s] = length[r]
    return out


def canonical_codes(lengths):
    """RFC 1951 3.2.2; returned bit-reversed (deflate packs Huffman codes starting at their most significant bit)."""
    maxlen = max(lengths)
    bl = [0] * (maxlen + 2)
    for l in lengths:
        if l:
            bl[l] += 1
    nxt = [0] * (maxlen + 2)
    code = 0
    for b in range(1, maxlen + 1):
        code = (code + bl[b - 1]) << 1
        nxt[b] = code
    out = [0] * len(lengths)
    for s, l in enumerate(lengths):
        if l:
            c = nxt[l]; nxt[l] += 1
            out[s] = int(format(c, "0%db" % l)[::-1], 2)
    return out


# ---- one block ------------------------------------------------------------------------------------------------------------------------
def block_lengths(data):
    """-> (literal/length code lengths [257], code-length code lengths [19]) of one block."""
    hist = np.bincount(np.frombuffer(data, np.uint8), minlength=257).tolist()
    hist[256] = 1
    lit = limited_lengths(hist, 15)
    sent = lit + [1, 1]
    clh = [0] * 19
    for l in sent:
        clh[l] += 1
    return lit, limited_lengths(clh, 7)


def encode_block(data, final):
    """One deflate block (and, unless final, the empty stored block behind it) -> bytes, a whole number of them."""
    lit, cl = block_lengths(data)
    litc, clc = canonical_codes(lit), canonical_codes(cl)
    hclen = max(4, max(i for i, s in enumerate(CL_ORDER) if cl[s]) + 1)
    vals, lens = [1 if final else 0, 2, 0, 1, hclen - 4], [1, 2, 5, 5, 4]
    for s in CL_ORDER[:hclen]:
        vals.append(cl[s]); lens.append(3)
    for l in lit + [1, 1]:
        vals.append(clc[l]); lens.append(cl[l])
    d = np.frombuffer(data, np.uint8)
    vals = np.concatenate([np.array(vals, np.int64), np.array(litc, np.int64)[d], [litc[256]]])
    lens = np.concatenate([np.array(lens, np.int64), np.array(lit, np.int64)[d], [lit[256]]])
    offs = np.concatenate([[0], np.cumsum(lens)])
    total = int(offs[-1])
    nbytes = (total + 3 + 7) // 8 + 4 if not final else (total + 7) // 8
    bits = np.zeros(nbytes * 8, np.uint8)
    for k in range(15):
        m = lens > k
        bits[offs[:-1][m] + k] = (vals[m] >> k) & 1
    out = bytearray(np.packbits(bits, bitorder="little").tobytes())
    if not final:
        out[-4:] = b"\x00\x00\xff\xff"
    return bytes(out)


# ---- the file -------------------------------------------------------------------------------------------------------------------------
def blocks_of(stream):
    return [stream[o:o + BLOCK] for o in range(0, len(stream), BLOCK)]


def idat_payload(px):
    stream = paeth_filter(px)
    blks = blocks_of(stream)
    body = b"".join(encode_block(b, i == len(blks) - 1) for i, b in enumerate(blks))
    return b"\x78\x01" + body + struct.pack(">I", zlib.adler32(stream) & 0xFFFFFFFF)


def _chunk(kind, payload):
    return struct.pack(">I", len(payload)) + kind + payload + struct.pack(">I", zlib.crc32(kind + payload) & 0xFFFFFFFF)


def png_file(px):
    """[h][w][3] uint8 -> the bytes of the PNG file the device writes."""
    px = np.ascontiguousarray(px, np.uint8)
    h, w, _ = px.shape
    return (b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) + _chunk(b"IDAT", idat_payload(px)) +
            _chunk(b"IEND", b""))


def png_base64(px):
    return base64.b64encode(png_file(px))


# ---- the worst case, from the format ---------------------------------------------------------------------------------------------------
def block_bound(nbytes):
    """Bytes of one block of nbytes literals at most: the header, 9 bits per symbol (end-of-block included: an optimal limited code
    costs no more than the flat code of 255 8-bit and 2 9-bit words), the stored block's 3 bits, padding, its 4 length bytes."""
    return (HEADER_BITS_MAX + 9 * (nbytes + 1) + 3 + 7) // 8 + 4


def file_bound(h, w):
    raw = h * (1 + 3 * w)
    full, tail = divmod(raw, BLOCK)
    z = 2 + full * block_bound(BLOCK) + (block_bound(tail) if tail else 0) + 4
    return 8 + 25 + 12 + z + 12


def base64_bound(h, w):
    if not (1 <= h <= 8192 and 1 <= w <= 8192):
        return 0
    return (file_bound(h, w) + 2) // 3 * 4
