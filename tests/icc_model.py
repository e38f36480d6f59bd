"""The engine's ICC-to-sRGB transform in numpy integers, its tables built here from a profile's bytes independently of the C++
(icc_parse.hpp): the matrix in exact rationals, the curves with Python floats.  Test infrastructure.

    lin[c][v] = rint(65535 * TRC_c(v / 255))                 clamped to 0..65535
    m         = rint(16384 * inv(M_sRGB) * M_profile)        Q14, M_sRGB's entries rounded to s15Fixed16
    y_c       = clamp((sum_k m[c][k] * lin[k][v_k] + 8192) >> 14, 0, 65535)
    out_c     = enc8(y_c) = rint(255 * sRGB_OETF(y_c / 65535))
    grey:       out = enc8(lin[0][v]) on all three bytes (v: the pixel's first byte)
"""
import math
import struct
from fractions import Fraction

import numpy as np

NONE, IDENTITY, MATRIX, GREY = range(4)
SRGB_D50 = ((0.43607, 0.38515, 0.14307), (0.22249, 0.71687, 0.06061), (0.01392, 0.09708, 0.71410))      # rows X Y Z, columns r g b


class Refused(Exception):
    pass


def _rint(x):
    return int(round(x))      # Python rounds halves to even, as rint does


def _enc8(x):
    l = x / 65535.0
    e = 12.92 * l if l <= 0.0031308 else 1.055 * math.pow(l, 1.0 / 2.4) - 0.055
    return min(255, max(0, _rint(255.0 * e)))


ENC8 = np.array([_enc8(x) for x in range(65536)], np.uint8)
ENC8.setflags(write=False)


def _u16(y):
    if not y > 0.0:
        return 0
    if y >= 1.0:
        return 65535
    return _rint(65535.0 * y)


def _pow(base, g):
    if not base > 0.0:
        return 0.0
    try:
        return math.pow(base, g)
    except OverflowError:
        return math.inf


def _s15(b, o):
    return struct.unpack(">i", b[o:o + 4])[0] / 65536.0


def curve(tag):
    """the bytes of a curve tag -> 256 ints, None for a truncated one; Refused for a kind that is not offered"""
    if len(tag) < 8:
        return None
    kind = tag[:4]
    if kind == b"curv":
        if len(tag) < 12:
            return None
        n = struct.unpack(">I", tag[8:12])[0]
        if n > 4096:
            raise Refused("curve")
        if n == 0:
            return [v * 257 for v in range(256)]
        if n == 1:
            if len(tag) < 14:
                return None
            g = struct.unpack(">H", tag[12:14])[0] / 256.0
            return [_u16(_pow(v / 255.0, g)) for v in range(256)]
        if len(tag) < 12 + 2 * n:
            return None
        t = struct.unpack(">%dH" % n, tag[12:12 + 2 * n])
        out = []
        for v in range(256):
            x = v / 255.0 * (n - 1)
            k = min(int(x), n - 2)
            f = x - k
            out.append(_u16((t[k] + (t[k + 1] - t[k]) * f) / 65535.0))
        return out
    if kind == b"para":
        if len(tag) < 12:
            return None
        fn = struct.unpack(">H", tag[8:10])[0]
        if fn > 4:
            raise Refused("curve")
        np_ = (1, 3, 4, 5, 7)[fn]
        if len(tag) < 12 + 4 * np_:
            return None
        g, a, b, c, d, e, f = [_s15(tag, 12 + 4 * k) for k in range(np_)] + [0.0] * (7 - np_)
        out = []
        for v in range(256):
            x = v / 255.0
            if fn == 0:
                y = _pow(x, g)
            elif fn == 1:
                y = _pow(a * x + b, g) if a != 0.0 and x >= -b / a else 0.0
            elif fn == 2:
                y = _pow(a * x + b, g) + c if a != 0.0 and x >= -b / a else c
            elif fn == 3:
                y = _pow(a * x + b, g) if x >= d else c * x
            else:
                y = _pow(a * x + b, g) + e if x >= d else c * x + f
            out.append(_u16(y))
        return out
    raise Refused("curve")


def _inv3(a):
    det = sum(a[0][i] * (a[1][(i + 1) % 3] * a[2][(i + 2) % 3] - a[1][(i + 2) % 3] * a[2][(i + 1) % 3]) for i in range(3))
    return [[(a[(j + 1) % 3][(i + 1) % 3] * a[(j + 2) % 3][(i + 2) % 3] - a[(j + 1) % 3][(i + 2) % 3] * a[(j + 2) % 3][(i + 1) % 3]) / det
             for j in range(3)] for i in range(3)]


def _round_half_even(q):
    fl = q.numerator // q.denominator
    r = q - fl
    return fl + (1 if r > Fraction(1, 2) or (r == Fraction(1, 2) and fl % 2) else 0)


def plan_profile(p, components=3):
    """the bytes of a profile -> {"kind", "m": [9], "lin": int array [3, 256]}; raises Refused for what the engine refuses"""
    none = {"kind": NONE, "m": [0] * 9, "lin": np.zeros((3, 256), np.int64)}
    if len(p) < 132 or len(p) > 1 << 20:
        return none
    size = struct.unpack(">I", p[:4])[0]
    if size > len(p) or size < 132 or p[36:40] != b"acsp":
        return none
    space, pcs = p[16:20], p[20:24]
    if space not in (b"RGB ", b"GRAY"):
        raise Refused("colour space")
    if pcs != b"XYZ ":
        raise Refused("PCS")
    n = struct.unpack(">I", p[128:132])[0]
    if n > (size - 132) // 12:
        return none
    tags = {}
    for k in range(n):
        sig, off, sz = struct.unpack(">4sII", p[132 + 12 * k:144 + 12 * k])
        if off > size or sz > size - off:
            return none
        tags.setdefault(sig, p[off:off + sz])
    if any(s in tags for s in (b"A2B0", b"A2B1", b"A2B2")):
        raise Refused("A2B")
    lin = np.zeros((3, 256), np.int64)
    if space == b"GRAY":
        if components != 1 or b"kTRC" not in tags:
            return none
        c = curve(tags[b"kTRC"])
        if c is None:
            return none
        lin[0] = c
        same = all(ENC8[lin[0][v]] == v for v in range(256))
        return {"kind": IDENTITY if same else GREY, "m": [0] * 9, "lin": lin}
    if components != 3:
        return none
    cols = []
    for s in (b"rXYZ", b"gXYZ", b"bXYZ"):
        t = tags.get(s)
        if t is None or len(t) < 20 or t[:4] != b"XYZ " or tags.get(s[:1] + b"TRC") is None:
            return none
        cols.append([Fraction(struct.unpack(">i", t[8 + 4 * k:12 + 4 * k])[0], 65536) for k in range(3)])
    for c, s in enumerate((b"rTRC", b"gTRC", b"bTRC")):
        cv = curve(tags[s])
        if cv is None:
            return none
        lin[c] = cv
    srgb = [[Fraction(int(round(v * 65536)), 65536) for v in row] for row in SRGB_D50]
    inv = _inv3(srgb)
    m = []
    for r in range(3):
        for c in range(3):
            v = sum(inv[r][k] * cols[c][k] for k in range(3))
            if not -4 < v < 4:
                raise Refused("matrix")
            m.append(_round_half_even(16384 * v))
    unit = m == [16384, 0, 0, 0, 16384, 0, 0, 0, 16384] and all(ENC8[lin[c][v]] == v for c in range(3) for v in range(256))
    return {"kind": IDENTITY if unit else MATRIX, "m": m, "lin": lin}


def apply(t, rgb):
    """[..., 3] uint8 -> the converted copy"""
    rgb = np.asarray(rgb, np.uint8)
    if t is None or t["kind"] in (NONE, IDENTITY):
        return rgb.copy()
    lin = np.asarray(t["lin"], np.int64)
    if t["kind"] == GREY:
        return np.repeat(ENC8[lin[0][rgb[..., :1]]], 3, axis=-1)
    l = np.stack([lin[k][rgb[..., k]] for k in range(3)], -1)
    m = np.asarray(t["m"], np.int64).reshape(3, 3)
    y = np.clip((l @ m.T + 8192) >> 14, 0, 65535)
    return ENC8[y]
