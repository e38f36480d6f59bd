"""ICC profiles and ICC-tagged JPEG files for the upload-ICC tests, written from the ICC specification (v2: ICC.1:2001-04, v4:
ICC.1:2010): matrix/TRC profiles with every curve form the engine takes, grey kTRC profiles, well-formed profiles it must refuse, and
the APP2 chunking of a profile into a JPEG file (Annex B of the specification).  Test infrastructure."""
import struct

# D50-adapted colorants (columns r, g, b as X, Y, Z), the published values of the three colour spaces
SRGB = ((0.43607, 0.22249, 0.01392), (0.38515, 0.71687, 0.09708), (0.14307, 0.06061, 0.71410))
DISPLAY_P3 = ((0.51512, 0.24120, -0.00105), (0.29198, 0.69225, 0.04189), (0.15710, 0.06657, 0.78407))
ADOBE_RGB = ((0.60974, 0.31111, 0.01947), (0.20528, 0.62567, 0.06087), (0.14919, 0.06322, 0.74457))
SRGB_PARA3 = (2.4, 1 / 1.055, 0.055 / 1.055, 1 / 12.92, 0.04045)      # IEC 61966-2-1 as `para` type 3: g a b c d


def s15f16(v):
    return struct.pack(">i", int(round(v * 65536)))


def xyz_tag(x, y, z):
    return b"XYZ \0\0\0\0" + s15f16(x) + s15f16(y) + s15f16(z)


def curv(values=()):
    """`curv` of count len(values): () the identity, (u8Fixed8,) a gamma, else a u16 table"""
    return b"curv\0\0\0\0" + struct.pack(">I", len(values)) + b"".join(struct.pack(">H", v) for v in values)


def curv_gamma(g):
    return curv((int(round(g * 256)),))


def curv_table(g, n):
    return curv([int(round(65535 * (i / (n - 1)) ** g)) for i in range(n)])


def para(fn, *params):
    assert len(params) == (1, 3, 4, 5, 7)[fn]
    return b"para\0\0\0\0" + struct.pack(">HH", fn, 0) + b"".join(s15f16(p) for p in params)


def _desc(version, text=b"test profile"):
    if version >= 4:
        u = text.decode().encode("utf-16-be")
        return b"mluc\0\0\0\0" + struct.pack(">II", 1, 12) + b"enUS" + struct.pack(">II", len(u), 28) + u
    return b"desc\0\0\0\0" + struct.pack(">I", len(text) + 1) + text + b"\0" + b"\0" * (4 + 4 + 2 + 1 + 67)


def assemble(tags, version=2, space=b"RGB ", pcs=b"XYZ ", device_class=b"mntr"):
    """[(signature, data)] -> the bytes of a profile: header, tag table, 4-aligned tag data"""
    off = 128 + 4 + 12 * len(tags)
    table, body = b"", b""
    for sig, data in tags:
        table += sig + struct.pack(">II", off + len(body), len(data))
        body += data + b"\0" * (-len(data) % 4)
    size = off + len(body)
    hd = struct.pack(">I", size) + b"\0\0\0\0" + (b"\x04\x30\0\0" if version >= 4 else b"\x02\x40\0\0") + device_class + space + pcs
    hd += struct.pack(">6H", 2024, 1, 1, 0, 0, 0) + b"acsp" + b"\0" * 4 + b"\0" * 4 + b"\0" * 4 + b"\0" * 4 + b"\0" * 8 + b"\0" * 4
    hd += s15f16(0.9642) + s15f16(1.0) + s15f16(0.8249) + b"\0" * 4 + b"\0" * 16 + b"\0" * 28
    assert len(hd) == 128
    return hd + struct.pack(">I", len(tags)) + table + body


def _common(version):
    return [(b"desc", _desc(version)), (b"wtpt", xyz_tag(0.9642, 1.0, 0.8249))]


def matrix_profile(colorants, trc, version=2, extra=(), **kw):
    """colorants: ((rX, rY, rZ), (g..), (b..)); trc: one curve's bytes for all three channels, or three"""
    trc = (trc,) * 3 if isinstance(trc, bytes) else tuple(trc)
    tags = _common(version)
    tags += [(s, xyz_tag(*c)) for s, c in zip((b"rXYZ", b"gXYZ", b"bXYZ"), colorants)]
    tags += [(s, t) for s, t in zip((b"rTRC", b"gTRC", b"bTRC"), trc)]
    return assemble(tags + list(extra), version, **kw)


def grey_profile(trc, version=2):
    return assemble(_common(version) + [(b"kTRC", trc)], version, space=b"GRAY")


def display_p3(version=4):
    return matrix_profile(DISPLAY_P3, para(3, *SRGB_PARA3), version)


def adobe_rgb(version=2):
    return matrix_profile(ADOBE_RGB, curv_gamma(563 / 256), version)


def srgb(version=2):
    return matrix_profile(SRGB, para(3, *SRGB_PARA3), version)


def a2b0_profile():
    """well-formed, matrix/TRC tags AND an A2B0 lookup table (an identity lut8 of 2 grid points): littlecms would use the table"""
    lut = b"mft1\0\0\0\0" + bytes((3, 3, 2, 0)) + b"".join(s15f16(v) for v in (1, 0, 0, 0, 1, 0, 0, 0, 1))
    lut += bytes(range(256)) * 3 + bytes(255 * ((i >> (2 - c)) & 1) for i in range(8) for c in range(3)) + bytes(range(256)) * 3
    return matrix_profile(SRGB, para(3, *SRGB_PARA3), 2, extra=[(b"A2B0", lut)])


def cmyk_profile():
    return assemble(_common(2) + [(b"A2B0", b"mft1\0\0\0\0")], 2, space=b"CMYK", pcs=b"Lab ", device_class=b"prtr")


def lab_pcs_profile():
    return matrix_profile(SRGB, curv_gamma(2.2), 2, pcs=b"Lab ")


# ---- a profile inside a JPEG file ----------------------------------------------------------------------------------------------------------
def app2(seq, count, data):
    payload = b"ICC_PROFILE\0" + bytes((seq, count)) + data
    assert len(payload) + 2 <= 65535
    return b"\xff\xe2" + struct.pack(">H", len(payload) + 2) + payload


def chunks(profile, n):
    """the profile cut into n nearly equal parts: [(seq, count, data)] in order"""
    step = -(-len(profile) // n)
    return [(i + 1, n, profile[i * step:(i + 1) * step]) for i in range(n)]


def insert_segments(jpeg, segments):
    """the segments' bytes spliced in behind the file's leading APP0 / APP1 segments (where writers put the profile)"""
    i = 2
    while jpeg[i] == 0xFF and jpeg[i + 1] in (0xE0, 0xE1):
        i += 2 + struct.unpack(">H", jpeg[i + 2:i + 4])[0]
    return jpeg[:i] + b"".join(segments) + jpeg[i:]


def tag(jpeg, profile, n=1, order=None):
    """the file with the profile in n APP2 chunks; order: a permutation of range(n), default in order"""
    ch = chunks(profile, n)
    return insert_segments(jpeg, [app2(*ch[k]) for k in (order if order is not None else range(n))])


def strip_app2(jpeg):
    out, i = jpeg[:2], 2
    while jpeg[i] == 0xFF and jpeg[i + 1] != 0xDA:
        n = 2 + struct.unpack(">H", jpeg[i + 2:i + 4])[0]
        if jpeg[i + 1] != 0xE2:
            out += jpeg[i:i + n]
        i += n
    return out + jpeg[i:]
