"""The files of the window-parallel decode's tests, shared by the CPU tests (test_jpeg_decode_windows_native.py) and the GPU tests
(test_jpeg_decode_windows_gpu.py).  Seeded and made by Pillow when the tests run, as jpeg_decode_cases' are."""
import numpy as np

import jpeg_decode_cases as cases
import jpeg_decode_model as model


def multi_window_files():
    """name -> (bytes, windows of its single stream).  Uniform noise at high quality: one stream without restart markers, two or three
    windows of 256 lanes x 1024 bits long; the tests assert the count, so a change of the encoder cannot make them miss silently.
    The grey file's stream is 6 bytes short of two whole windows: its second window has all its lanes."""
    return {
        "128x128_q95_444": (cases.encode(cases.noise(128, 128, 1), 95, 0), 2),
        "192x192_q95_444": (cases.encode(cases.noise(192, 192, 2), 95, 0), 3),
        "160x200_q95_444": (cases.encode(cases.noise(200, 160, 3), 95, 0), 3),          # ragged: 160 wide, 200 high
        "256x256_q90_420": (cases.encode(cases.noise(256, 256, 4), 90, 2), 2),
        "256x256_q92_422": (cases.encode(cases.noise(256, 256, 5), 92, 1), 3),
        "grey_256x256_q95": (cases.encode(cases.noise(256, 256, 8)[:, :, 0], 95), 2),
    }


def full_last_subsequence_file(subseq_bytes, short_max_bytes, seeds=4000):
    """the first seed whose 40 x 32 noise file has a long stream of a whole number of subsequences -> (bytes, seed) or (None, None)"""
    for seed in range(seeds):
        data = cases.encode(cases.noise(32, 40, seed), 95, 0)
        n = len(model.plan(data).streams[0][0])
        if n % subseq_bytes == 0 and n > short_max_bytes:
            return data, seed
    return None, None


def corrupt_scan_byte(data, rng):
    """one byte of the scan (behind the SOS header, in front of the EOI) xored with a non-zero value"""
    sos = data.index(b"\xff\xda")
    scan0 = sos + 2 + int.from_bytes(data[sos + 2:sos + 4], "big")
    b = bytearray(data)
    at = int(rng.integers(scan0, len(data) - 2))
    b[at] ^= int(rng.integers(1, 256))
    return at, bytes(b)


def corrupted_two_window_files(count=200):
    """-> the good 2-window file, [(name, bytes)]: `count` seeded single-byte corruptions of its scan"""
    good = multi_window_files()["128x128_q95_444"][0]
    r = np.random.default_rng(2024)
    out = []
    for k in range(count):
        at, data = corrupt_scan_byte(good, r)
        out.append(("flip_%d_at_%d" % (k, at), data))
    return good, out
