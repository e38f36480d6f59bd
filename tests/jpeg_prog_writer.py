"""A test-side writer of progressive JPEG files (pure Python): quantised coefficients (jpeg_decode_model's decode of a Pillow baseline
file), the frame and a SCAN SCRIPT -> file bytes.  It stands in for encoders that are not installed here (mozjpeg's scripts above all):
every scan kind of T.81 Annex G, interleaved and single-component DC scans, any band and successive-approximation schedule, a Huffman
table per scan built from the scan's own symbol counts by the standard's K.2 procedure (so EOBn symbols are coded), an optional
restart interval counted in the scan's own MCUs.  tests/test_jpeg_prog_model.py checks it against Pillow: every file it writes decodes
to exactly the pixels of the baseline file its coefficients came from.

A script is a list of (components, Ss, Se, Ah, Al), components a tuple of frame indices (0 = Y, 1 = Cb, 2 = Cr)."""
import io
import struct

import numpy as np
from PIL import Image, ImageFile

import jpeg_decode_model as base
from jpeg_decode_model import ZIGZAG


def pillow_progressive(px, quality=85, subsampling=0, **kw):
    """pixels ([h][w][3] -> RGB, [h][w] -> grey) -> the bytes of Pillow's (libjpeg-turbo's) progressive file.  MAXBLOCK is raised around
    the save: with the default Pillow fails on large scans ("Suspension not allowed here")."""
    bio = io.BytesIO()
    px = np.ascontiguousarray(px, np.uint8)
    old = ImageFile.MAXBLOCK
    ImageFile.MAXBLOCK = 1 << 24
    try:
        if px.ndim == 2:
            Image.fromarray(px, "L").save(bio, "JPEG", quality=quality, progressive=True, **kw)
        else:
            Image.fromarray(px, "RGB").save(bio, "JPEG", quality=quality, subsampling=subsampling, progressive=True, **kw)
    finally:
        ImageFile.MAXBLOCK = old
    return bio.getvalue()


# ---- the scripts ---------------------------------------------------------------------------------------------------------------------
def script_simple():
    """libjpeg's jpeg_simple_progression for Y Cb Cr: what Pillow writes"""
    return [((0, 1, 2), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((2,), 1, 63, 0, 1), ((1,), 1, 63, 0, 1), ((0,), 6, 63, 0, 2), ((0,), 1, 63, 2, 1),
            ((0, 1, 2), 0, 0, 1, 0), ((2,), 1, 63, 1, 0), ((1,), 1, 63, 1, 0), ((0,), 1, 63, 1, 0)]


def script_moz(chroma_refined=True):
    """mozjpeg-style: DC per component, not interleaved, at full precision; luma 1-8 and 9-63 at Al = 2, refined 2 -> 1 -> 0; chroma
    1-63 at Al = 1 and refined, or (chroma_refined=False) at full precision with the luma bands refined one by one"""
    s = [((0,), 0, 0, 0, 0), ((1,), 0, 0, 0, 0), ((2,), 0, 0, 0, 0), ((0,), 1, 8, 0, 2), ((0,), 9, 63, 0, 2)]
    if chroma_refined:
        return s + [((1,), 1, 63, 0, 1), ((2,), 1, 63, 0, 1), ((0,), 1, 63, 2, 1), ((0,), 1, 63, 1, 0), ((1,), 1, 63, 1, 0), ((2,), 1, 63, 1, 0)]
    return s + [((1,), 1, 63, 0, 0), ((2,), 1, 63, 0, 0), ((0,), 1, 8, 2, 1), ((0,), 9, 63, 2, 1), ((0,), 1, 63, 1, 0)]


def script_spectral():
    """spectral selection only: every Al = 0, bands 1-1 (one coefficient), 2-5, 6-63"""
    return [((0, 1, 2), 0, 0, 0, 0)] + [((c,), a, b, 0, 0) for c in (0, 1, 2) for a, b in ((1, 1), (2, 5), (6, 63))]


def script_dc3():
    """DC at Al = 3 with three refinements; Cb and Cr in ONE interleaved DC scan"""
    return [((0,), 0, 0, 0, 3), ((1, 2), 0, 0, 0, 3), ((0, 1, 2), 0, 0, 3, 2), ((0,), 0, 0, 2, 1), ((1, 2), 0, 0, 2, 1), ((0, 1, 2), 0, 0, 1, 0)] + \
           [((c,), 1, 63, 0, 0) for c in (0, 1, 2)]


def for_grey(script):
    """the script of a one-component frame: what it says about Y"""
    out = []
    for comps, ss, se, ah, al in script:
        if 0 in comps and ((0,), ss, se, ah, al) not in out:
            out.append(((0,), ss, se, ah, al))
    return out


SCRIPTS = {"simple": (script_simple(), 0), "moz": (script_moz(), 0), "moz_flat_chroma": (script_moz(False), 0), "spectral": (script_spectral(), 0),
           "dc3": (script_dc3(), 0), "moz_rst3": (script_moz(), 3)}           # name -> (script, restart interval)


# ---- K.2: a Huffman table from symbol counts (jchuff.c jpeg_gen_optimal_table) ---------------------------------------------------------
def optimal_table(counts):
    """{symbol: count} -> (bits[1..16] as a list of 16, symbols in code order)"""
    freq = [0] * 257
    for s, n in counts.items():
        freq[s] = n
    freq[256] = 1                       # reserves the all-ones code
    codesize, others = [0] * 257, [-1] * 257
    while True:
        c1, v = -1, 1 << 60
        for i in range(257):
            if freq[i] and freq[i] <= v:
                v, c1 = freq[i], i
        c2, v = -1, 1 << 60
        for i in range(257):
            if freq[i] and freq[i] <= v and i != c1:
                v, c2 = freq[i], i
        if c2 < 0:
            break
        freq[c1] += freq[c2]
        freq[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    bits = [0] * 64
    for i in range(257):
        if codesize[i]:
            bits[codesize[i]] += 1
    for i in range(63, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1
    vals = [j for i in range(1, 64) for j in range(256) if codesize[j] == i]
    return bits[1:17], vals


def _codes(bits, vals):
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def _nbits(v):
    return int(v).bit_length()


# ---- one scan -> tokens ("s", symbol) | ("b", value, count) | ("r",) a restart -----------------------------------------------------------
class _Tokens:
    def __init__(self):
        self.t = []
        self.eobrun = 0
        self.be = []                    # correction bits waiting behind the pending EOB run

    def sym(self, s):
        self.t.append(("s", s))

    def bits(self, v, n):
        if n:
            self.t.append(("b", v & ((1 << n) - 1), n))

    def flush_eobrun(self):
        if self.eobrun:
            n = _nbits(self.eobrun) - 1
            self.sym(n << 4)
            self.bits(self.eobrun, n)
            self.eobrun = 0
        for b in self.be:
            self.bits(b, 1)
        self.be = []


def _scan_blocks(p, comps, grids, mcu, rw):
    if len(comps) == 1:
        y, x = divmod(mcu, rw)
        return [(comps[0], grids[comps[0]][y, x])]
    my, mx = divmod(mcu, p.mcus_w)
    return [(c, grids[c][my * p.vs[c] + by, mx * p.hs[c] + bx]) for c in comps for by in range(p.vs[c]) for bx in range(p.hs[c])]


def _scan_tokens(p, grids, scan, restart):
    comps, ss, se, ah, al = scan
    if len(comps) == 1:
        c = comps[0]
        rw, rh = -(-p.plane[c][1] // 8), -(-p.plane[c][0] // 8)
        nmcu = rw * rh
    else:
        rw, nmcu = 0, p.mcus_w * p.mcus_h
    tk = _Tokens()
    pred = {c: 0 for c in comps}
    for mcu in range(nmcu):
        if restart and mcu and mcu % restart == 0:
            tk.flush_eobrun()
            tk.t.append(("r",))
            pred = {c: 0 for c in comps}
        for c, blk in _scan_blocks(p, comps, grids, mcu, rw):
            if ss == 0 and ah == 0:                               # DC first: the difference of the point-transformed values
                v = int(blk[0]) >> al
                d = v - pred[c]
                pred[c] = v
                n = _nbits(abs(d))
                tk.sym(n)
                tk.bits(d if d >= 0 else d - 1, n)
            elif ss == 0:                                         # DC refinement: one bit
                tk.bits((int(blk[0]) >> al) & 1, 1)
            elif ah == 0:                                         # AC first (jcphuff.c encode_mcu_AC_first)
                r = 0
                for k in range(ss, se + 1):
                    v = int(blk[ZIGZAG[k]])
                    a = abs(v) >> al
                    if a == 0:
                        r += 1
                        continue
                    tk.flush_eobrun()
                    while r > 15:
                        tk.sym(0xF0)
                        r -= 16
                    n = _nbits(a)
                    tk.sym((r << 4) | n)
                    tk.bits(a if v >= 0 else ~a, n)
                    r = 0
                if r:
                    tk.eobrun += 1
                    if tk.eobrun == 0x7FFF:
                        tk.flush_eobrun()
            else:                                                 # AC refinement (encode_mcu_AC_refine)
                absv = [abs(int(blk[ZIGZAG[k]])) >> al for k in range(ss, se + 1)]
                eob = max((k for k in range(len(absv)) if absv[k] == 1), default=-1)
                r, br = 0, []
                for k, a in enumerate(absv):
                    if a == 0:
                        r += 1
                        continue
                    while r > 15 and k <= eob:
                        tk.flush_eobrun()
                        tk.sym(0xF0)
                        r -= 16
                        for b in br:
                            tk.bits(b, 1)
                        br = []
                    if a > 1:
                        br.append(a & 1)
                        continue
                    tk.flush_eobrun()
                    tk.sym((r << 4) | 1)
                    tk.bits(0 if int(blk[ZIGZAG[ss + k]]) < 0 else 1, 1)
                    for b in br:
                        tk.bits(b, 1)
                    br = []
                    r = 0
                if r or br:
                    tk.eobrun += 1
                    tk.be += br
                    if tk.eobrun == 0x7FFF or len(tk.be) > 900:
                        tk.flush_eobrun()
    tk.flush_eobrun()
    return tk.t


def _emit(tokens, codes):
    """tokens -> entropy-coded bytes: stuffing, 1-bits to the byte boundary before every restart marker and at the end"""
    out = bytearray()
    acc = n = 0
    rst = 0

    def put(v, c):
        nonlocal acc, n
        acc = (acc << c) | v
        n += c
        while n >= 8:
            b = (acc >> (n - 8)) & 255
            out.append(b)
            if b == 0xFF:
                out.append(0)
            n -= 8
        acc &= (1 << n) - 1

    for t in tokens:
        if t[0] == "s":
            put(*codes[t[1]])
        elif t[0] == "b":
            put(t[1], t[2])
        else:
            if n:
                put((1 << (8 - n)) - 1, 8 - n)
            out += bytes([0xFF, 0xD0 + (rst & 7)])
            rst += 1
    if n:
        put((1 << (8 - n)) - 1, 8 - n)
    return bytes(out)


def _seg(marker, payload):
    return bytes([0xFF, marker]) + struct.pack(">H", len(payload) + 2) + payload


def write(p, grids, script, restart=0, extra_before_scan=None):
    """p: jpeg_decode_model's Plan of the source file (frame, sampling, quantisers), grids: its coefficients -> progressive file bytes.
    extra_before_scan: {scan index: bytes} put in front of that scan's DHT (the refusal cases use it)."""
    out = bytearray(b"\xff\xd8" + _seg(0xE0, b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0"))
    tables = [p.quant[0]] + ([p.quant[1]] if p.ncomp == 3 else [])
    assert p.ncomp == 1 or p.quant[1] == p.quant[2]
    for k, q in enumerate(tables):
        out += _seg(0xDB, bytes([k]) + bytes(int(q[ZIGZAG[z]]) for z in range(64)))
    out += _seg(0xC2, struct.pack(">BHHB", 8, p.h, p.w, p.ncomp) + b"".join(bytes([c + 1, (p.hs[c] << 4) | p.vs[c], min(c, 1)]) for c in range(p.ncomp)))
    if restart:
        out += _seg(0xDD, struct.pack(">H", restart))
    for k, scan in enumerate(script):
        comps, ss, se, ah, al = scan
        tokens = _scan_tokens(p, grids, scan, restart)
        counts = {}
        for t in tokens:
            if t[0] == "s":
                counts[t[1]] = counts.get(t[1], 0) + 1
        out += (extra_before_scan or {}).get(k, b"")
        codes = {}
        if counts:
            bits, vals = optimal_table(counts)
            codes = _codes(bits, vals)
            out += _seg(0xC4, bytes([0x00 if ss == 0 else 0x10]) + bytes(bits) + bytes(vals))
        out += _seg(0xDA, bytes([len(comps)]) + b"".join(bytes([c + 1, 0]) for c in comps) + bytes([ss, se, (ah << 4) | al]))
        out += _emit(tokens, codes)
    return bytes(out + b"\xff\xd9")


def from_baseline(data, script, restart=0, **kw):
    """the bytes of a baseline file (what jpeg_decode_model reads) -> a progressive file with the same coefficients"""
    p = base.plan(data)
    grids = base.coefficients(p)
    return write(p, grids, for_grey(script) if p.ncomp == 1 else script, restart, **kw)
