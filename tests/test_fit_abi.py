"""Any-size entry points of the C ABI (include/ire.h "any-size jobs"): what can be checked without a GPU -- the size arithmetic of
the encoder against oracle/encode.py and the rejection of null engine handles."""
import ctypes

import numpy as np
import pytest

from image_restoration_platform_amd import _lib
from oracle import encode as oenc

HEIGHTS = [1, 2, 3, 9, 16, 40, 771, 772]
WIDTHS = list(range(1, 18)) + [28, 57, 58, 59, 60, 61, 62, 63, 64, 101, 1000, 2048]      # every w mod 8, every 3 w mod 4


@pytest.mark.parametrize("h", HEIGHTS)
def test_png_base64_bytes_fit_is_the_oracles_length(h):
    lib = _lib.load()
    assert {w % 8 for w in WIDTHS} == set(range(8)) and {(3 * w) % 4 for w in WIDTHS} == set(range(4))      # the grid is what it claims to be
    for w in WIDTHS:
        want = len(oenc.png_base64(np.zeros((h, w, 3), np.uint8)))
        assert lib.ire_png_base64_bytes_fit(h, w) == want, (h, w)
        old = lib.ire_png_base64_bytes(h, w)
        if old:
            assert old == want, (h, w)


def test_png_base64_bytes_fit_block_boundary_sizes_and_limits():
    lib = _lib.load()
    for h, w in [(3, 7281), (4, 7281), (1365, 2048), (750, 1000)]:
        assert lib.ire_png_base64_bytes_fit(h, w) == len(oenc.png_base64(np.zeros((h, w, 3), np.uint8)))
    # closed form at the limit (no 200 MB array): file = 57 + 6 + 5 * blocks + h * (1 + 3 w)
    raw = 8192 * (1 + 3 * 8192)
    file = 63 + 5 * ((raw + 65534) // 65535) + raw
    assert lib.ire_png_base64_bytes_fit(8192, 8192) == (file + 2) // 3 * 4 == lib.ire_png_base64_bytes(8192, 8192)
    for h, w in [(0, 8), (8, 0), (-1, 8), (8, -8), (8193, 8), (8, 8193), (0, 0)]:
        assert lib.ire_png_base64_bytes_fit(h, w) == 0, (h, w)


def test_fit_entries_reject_a_null_engine():
    lib = _lib.load()
    px = np.zeros((5, 7, 3), np.uint8)
    out = np.zeros_like(px)
    job = ctypes.c_void_p()
    p = lambda a: ctypes.c_void_p(a.ctypes.data)
    assert lib.ire_submit_fit(None, p(px), 5, 7, 1, None, ctypes.byref(job)) == _lib.IRE_ERR_INVALID_INPUT
    assert b"invalid" in lib.ire_last_error()
    assert lib.ire_restore_fit(None, p(px), 1, 5, 7, None, None, p(out), None) == _lib.IRE_ERR_INVALID_INPUT
    assert b"invalid" in lib.ire_last_error()
    assert lib.ire_restore_fit_device(None, None, 1, 5, 7, None, None, None, None) == _lib.IRE_ERR_INVALID_INPUT
    assert lib.ire_encode_png_base64_fit(None, p(px), 1, 5, 7, p(out), 1024) == _lib.IRE_ERR_INVALID_INPUT
    assert lib.ire_encode_png_base64_fit_device(None, None, 1, 5, 7, 21, 105, None, 1024, None) == _lib.IRE_ERR_INVALID_INPUT


def test_adler_schedule_bounds():
    """The reduction schedule of the encoder's Adler sums (csrc/encode.hip, "The Adler-32 schedule"), redone in Python integers for
    the largest image an entry point accepts, 16384 x 16384, all 255: the largest value every partial reaches before its `mod` (or
    before it is added on) fits the integer it is kept in -- and the schedule gives zlib's Adler-32 on a stream small enough to run."""
    import re
    import os
    import zlib
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "image_restoration_platform_amd", "csrc", "encode.hip")).read()
    consts = {}
    for name, pat in (("kAdlerMod", r"kAdlerMod = (\d+)u"), ("kFrameDwords", r"kFrameDwords = (\d+);"), ("kFrameThreads", r"kFrameThreads = (\d+);")):
        m = re.search(pat, src)
        assert m is not None, "encode.hip no longer defines %s as this test reads it: keep the two in step" % name
        consts[name] = int(m.group(1))
    M, dwords, threads = consts["kAdlerMod"], consts["kFrameDwords"], consts["kFrameThreads"]
    assert M == 65521 and threads == 256
    # the structure the bound rests on is pinned in the kernel itself (static_asserts beside the constants); here: that they are there
    assert src.count("static_assert((unsigned long long)kFrame") >= 3 and "T %= kAdlerMod;" in src
    h = w = 16384
    raw = h * (1 + 3 * w)
    blocks = (raw + 65534) // 65535
    file = 63 + 5 * blocks + raw
    assert raw < 2 ** 32 and file < 2 ** 32                  # raw indices and file offsets are 32-bit in the kernel
    per_byte = (M - 1) * 255                                 # (i mod M) * d
    per_thread = dwords * 4 * per_byte                       # before the thread's `mod`
    assert per_thread < 2 ** 32
    per_wg = 256 * (M - 1)                                   # 256 reduced thread sums, added in 32 bits
    assert per_wg < 2 ** 32
    wgs = (file + 4 * 256 * dwords - 1) // (4 * 256 * dwords)
    assert wgs * per_wg < 2 ** 64                            # the image's T accumulator (64-bit atomic adds), never reduced before the end
    s_thread = dwords * 4 * 255
    assert 256 * s_thread < 2 ** 32                          # S of a workgroup
    assert 255 * raw < 2 ** 64                               # the image's S accumulator
    assert (M - 1) + (M - 1) * (M - 1) + M < 2 ** 64         # the final N + N S - T, in 64 bits
    # the same schedule on a real stream: groups of 16 bytes reduced mod M, then summed
    rng = np.random.default_rng(7)
    d = rng.integers(0, 256, 200000, dtype=np.uint8).astype(object)
    n = len(d)
    S = int(sum(d))
    T = 0
    for g0 in range(0, n, 16):
        T += sum(((g0 + k) % M) * int(d[g0 + k]) for k in range(min(16, n - g0))) % M
    A = (1 + S) % M
    B = (n % M + (n % M) * (S % M) + M - T % M) % M
    assert (B << 16 | A) == zlib.adler32(bytes(int(v) for v in d)) & 0xFFFFFFFF
