"""The progressive files the JPEG decoder is tested on, shared by the CPU tests of the model (test_jpeg_prog_model.py), of the native
code (test_jpeg_prog_native.py) and the GPU tests (test_jpeg_prog_gpu.py, test_submit_jpeg_prog_gpu.py).  Everything is seeded and
made when the tests run, by Pillow (libjpeg's simple progression) or by the test-side writer (jpeg_prog_writer.py: the scripts other
encoders use); nothing is read from disk."""
import functools
import struct

import numpy as np

import jpeg_decode_cases as cases
import jpeg_prog_writer as writer
from jpeg_decode_cases import noise, smooth
from jpeg_prog_writer import pillow_progressive

WRITER_SIZES = [(8, 8), (17, 13), (33, 47)]           # (w, h)


def pillow_grid_cases():
    """the seven sizes x three samplings x four qualities, smooth and noise alternating; grey; a restart interval of 3 blocks"""
    d = {}
    seed = 300
    for w, h in cases.SIZES:
        for sub in (0, 1, 2):
            if sub and w < 5:
                continue
            for q in cases.QUALITIES:
                seed += 1
                kind = "noise" if seed % 2 else "smooth"
                d["%dx%d_s%d_q%d_%s" % (w, h, sub, q, kind)] = pillow_progressive(cases.content(kind, h, w, seed), q, sub)
            d["%dx%d_s%d_rst3" % (w, h, sub)] = pillow_progressive(smooth(h, w, seed + 2000), 85, sub, restart_marker_blocks=3)
    for w, h in ((8, 8), (17, 13)):
        d["grey_%dx%d" % (w, h)] = pillow_progressive(noise(h, w, 7)[:, :, 0], 85)
        d["grey_%dx%d_rst3" % (w, h)] = pillow_progressive(smooth(h, w, 8)[:, :, 1], 95, restart_marker_blocks=3)
    return d


def sweep_cases():
    """heights 1..19 x widths 5..35, the sampling and the content cycling: every partial-MCU shape of every sampling"""
    d = {}
    for h in range(1, 20):
        for w in range(5, 36):
            sub = (h + w) % 3
            kind = "noise" if (h * 31 + w) % 2 else "smooth"
            d["sweep_%dx%d_s%d" % (w, h, sub)] = pillow_progressive(cases.content(kind, h, w, 3000 + h * 64 + w), 85, sub)
    return d


@functools.lru_cache(maxsize=None)
def writer_cases():
    """every script of the writer on 8 x 8, 17 x 13 and 33 x 47 in the three samplings and grey: name -> (progressive bytes, the baseline
    file its coefficients came from).  6 scripts x 3 sizes x 4 = 72 files."""
    d = {}
    for w, h in WRITER_SIZES:
        for sub in (0, 1, 2, 3):
            px = noise(h, w, 500 + 8 * w + sub)
            src = cases.encode(px[:, :, 0] if sub == 3 else px, 85, sub if sub < 3 else 0)
            for name, (script, restart) in writer.SCRIPTS.items():
                d["%s_%dx%d_s%d" % (name, w, h, sub)] = (writer.from_baseline(src, script, restart), src)
    return d


def _dqt():
    return b"\xff\xdb" + struct.pack(">H", 67) + b"\0" + bytes([16] * 64)


def refused_cases():
    """name -> (bytes, a word the reason must contain): what breaks the progression rules, written by the writer from good coefficients"""
    src = cases.encode(noise(13, 17, 9), 85, 2)
    simple = writer.script_simple()
    dc = ((0, 1, 2), 0, 0, 0, 0)
    ac = [((c,), 1, 63, 0, 0) for c in (0, 1, 2)]
    many = [dc] + [((0,), k, k, 0, 0) for k in range(1, 64)] + [((1,), 1, 63, 0, 0), ((2,), 1, 63, 0, 0)]       # 66 scans
    return {
        "incomplete": (writer.from_baseline(src, simple[:-1]), "incomplete"),
        "ah_not_previous_al": (writer.from_baseline(src, [simple[0], ((0,), 1, 5, 0, 2), ((0,), 1, 5, 1, 0)]), "Ah is not the Al"),
        "repeated_first_scan": (writer.from_baseline(src, [dc, ac[0], ac[0]]), "Ah is not the Al"),
        "ac_before_dc": (writer.from_baseline(src, [ac[0], dc, ac[1], ac[2]]), "before the component's DC scan"),
        "ac_two_components": (writer.from_baseline(src, [dc, ac[0], ((1, 2), 1, 63, 0, 0)]), "more than one component"),
        "dqt_between_scans": (writer.from_baseline(src, [dc] + ac, extra_before_scan={2: _dqt()}), "DQT behind the first scan"),
        "too_many_scans": (writer.from_baseline(src, many), "more than 64 scans"),
    }


def cap_scans_file():
    """a grey file of exactly the cap's 64 scans: DC, then 63 bands of one coefficient -- accepted"""
    src = cases.encode(noise(13, 17, 10)[:, :, 0], 85)
    return writer.from_baseline(src, [((0,), 0, 0, 0, 0)] + [((0,), k, k, 0, 0) for k in range(1, 64)]), src


def largest_stream(data, kinds):
    """the longest stream (bytes, stuffing removed) among the file's scans of these kinds (jpeg_prog_model's numbers)"""
    import jpeg_prog_model as model
    return max(len(s) for sc in model.plan(data).scans if sc.kind in kinds for s in sc.streams)


@functools.lru_cache(maxsize=None)
def multi_window_files(window_bits):
    """two files whose largest FIRST scan has at least 2.5 windows: Pillow's q100 noise (its luma 6-63 scan), the side found in steps of
    64; the writer's full-precision luma 1-63 scan of q95 noise, the side found in steps of 32 from 320.  name -> bytes"""
    side = 256
    while True:
        f = pillow_progressive(noise(side, side, 41), 100, 0)
        if 8 * largest_stream(f, (1, 2)) >= 2.5 * window_bits:
            break
        side += 64
    wside = 320
    while True:
        g = writer.from_baseline(cases.encode(noise(wside, wside, 42), 95, 0), writer.script_dc3())
        if 8 * largest_stream(g, (1, 2)) >= 2.5 * window_bits:
            break
        wside += 32
    return {"pillow_q100_%d" % side: f, "writer_dc3_%d" % wside: g}


@functools.lru_cache(maxsize=None)
def flat_file():
    """1024 x 1032 flat grey: 16512 blocks, every AC scan nothing but EOB-run symbols (a run of 16384 and more)"""
    return pillow_progressive(np.full((1032, 1024), 77, np.uint8), 85)


@functools.lru_cache(maxsize=None)
def long_refinement_file():
    """320 x 320 q95 noise by Pillow: its last luma refinement scan is one stream of tens of kilobytes"""
    return pillow_progressive(noise(320, 320, 43), 95, 0)


def corrupt_refinement_candidates(count=40):
    """seeded single-byte corruptions inside the LAST scan (an AC refinement) of a 33 x 47 4:2:0 Pillow file: [(name, bytes)]"""
    good = pillow_progressive(noise(47, 33, 12), 85, 2)
    sos = good.rindex(b"\xff\xda")
    data0 = sos + 2 + int.from_bytes(good[sos + 2:sos + 4], "big")
    r = np.random.default_rng(77)
    out = []
    for k in range(count):
        b = bytearray(good)
        at = int(r.integers(data0, len(good) - 2))
        b[at] ^= int(r.integers(1, 256))
        if b[at] == 0xFF or b[at - 1] == 0xFF:
            b[at] = 0x55 if good[at] != 0x55 else 0x56
        out.append(("refine_flip_%d_at_%d" % (k, at), bytes(b)))
    return good, out


def malformed_pack():
    """a 17 x 13 4:2:0 progressive file cut at every tenth byte, and 200 seeded single-byte corruptions spread over its scans (the
    bytes from its first SOS on: scan headers, the tables between the scans, entropy-coded data).  -> good, [(name, bytes)]"""
    good = pillow_progressive(noise(13, 17, 5), 85, 2)
    out = [("cut_%d" % n, good[:n]) for n in range(0, len(good), 10)]
    first = good.index(b"\xff\xda")
    r = np.random.default_rng(199)
    for k in range(200):
        b = bytearray(good)
        at = first + (k * (len(good) - 2 - first)) // 200 + int(r.integers(0, max(1, (len(good) - 2 - first) // 200)))
        b[at] ^= int(r.integers(1, 256))
        out.append(("flip_%d_at_%d" % (k, at), bytes(b)))
    return good, out
