"""Coefficient arrays for the progressive JPEG encoder (tests/jpeg_progenc_model.py, csrc/jpeg_progenc_core.hpp, csrc/jpeg_progenc.hip),
built so that every rule of jcphuff.c the walk can get wrong fires at least once.  A case is (h, w, quality, sampling, coefficients in
the layout of ire_debug_jpeg_progressive_from_coefs); EXPECT names the model's event counters (jpeg_progenc_model.EVENTS) that the case
must raise.  The same cases go through the model, the CPU program and the device."""
import functools

import numpy as np

import jpeg_opt_model as opt
import jpeg_progenc_model as model


def noise(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def _empty(h, w, s):
    geo, _ = model.geometry(h, w, s)
    return [np.zeros((g[0], g[1], 64), np.int64) for g in geo]


def _eob_whole_interval():
    """DC alone: every AC interval is one end-of-band run over all its blocks, flushed by the restart (or the scan's end)"""
    p = _empty(24, 40, 0)
    for c in range(3):
        p[c][:, :, 0] = np.arange(15).reshape(3, 5) * 7 - 40
    return 24, 40, 85, 0, p


def _run_broken_in_last_block():
    """every block of a row empty but the last, which holds ONE coefficient: the run is sent in front of it"""
    p = _empty(16, 48, 0)
    for c in range(3):
        p[c][:, -1, 9] = 12
        p[c][1, -1, 9] = -5
    return 16, 48, 85, 0, p


def _zrl_chains():
    """runs of 16 and more zeros in front of a coefficient: in the first scans (values that survive the shift) and in the refinement
    scans (values the first scans' shift zeroes: 1 for the Al = 0 scans, 2 and 3 for Y's Ah = 2, Al = 1 scan)"""
    p = _empty(8, 24, 0)
    for c in range(3):
        p[c][0, 0, 1], p[c][0, 0, 40], p[c][0, 0, 63] = 9, -20, 8          # runs of 38 and 22 in the first scans
        p[c][0, 1, 50] = 1                                                    # new at Al = 0 behind 49 zeros
        p[c][0, 2, 20], p[c][0, 2, 58] = -1, 1
    p[0][0, 1, 35] = 3                                                        # new in Y's scan to Al = 1 behind 34 zeros
    p[0][0, 2, 62] = -2
    return 8, 24, 85, 0, p


def _refine_no_trailing_zrl():
    """a new coefficient early, an already-non-zero one far behind it, zeros between and behind: k > EOB, so no ZRL, the correction bit
    joins the run"""
    p = _empty(8, 16, 0)
    for c in range(3):
        p[c][0, 0, 3], p[c][0, 0, 40] = 1, 6
        p[c][0, 1, 2], p[c][0, 1, 30], p[c][0, 1, 60] = -1, -7, 4
    p[0][0, 0, 5], p[0][0, 0, 45] = 2, 9                                      # the same for Y's Ah = 2 scan: 2 >> 1 is 1, 9 >> 1 is 4
    return 8, 16, 85, 0, p


def _early_flush():
    """twenty consecutive blocks full of |c| >= 4 and no newly non-zero coefficient: 63 correction bits per block join the run, which is
    flushed once more than 937 are buffered -- in Y's Ah = 2 scan and in all three Al = 0 scans"""
    p = _empty(8, 160, 0)
    rng = np.random.default_rng(5)
    for c in range(3):
        v = rng.integers(4, 40, (1, 20, 64)) * rng.choice([-1, 1], (1, 20, 64))
        p[c][:] = v
    return 8, 160, 85, 0, p


def _extreme(s):
    """every coefficient at the end of its range at quality 100 (jpeg_opt_model: the DC in -1024..1016, an AC up to 1020), signs
    alternating: the largest category after each shift, and the bound"""
    h, w = 32, 48
    p = _empty(h, w, s)
    for c in range(3):
        q = opt.quant_tables(100)[0 if c == 0 else 1]
        amax = np.array([(opt.coef_bound(opt.ZIGZAG[k]) + 4 * q[opt.ZIGZAG[k]]) // (8 * q[opt.ZIGZAG[k]]) for k in range(64)])
        sign = np.where((np.add.outer(np.arange(p[c].shape[0]), np.arange(p[c].shape[1]))[..., None] + np.arange(64)) % 2 == 0, 1, -1)
        p[c][:] = amax * sign
        dc = np.where((np.add.outer(np.arange(p[c].shape[0]), np.arange(p[c].shape[1]))) % 2 == 0, -1024, 1016)
        p[c][:, :, 0] = dc
    return h, w, 100, s, p


def _negative_dc_and_ones():
    """odd negative DCs (the arithmetic shift rounds down, not towards zero) and AC coefficients of magnitude 1, which the Al = 1
    shift zeroes in the first scans"""
    p = _empty(16, 16, 2)
    rng = np.random.default_rng(9)
    for c in range(3):
        p[c][:, :, 0] = -2 * rng.integers(0, 30, p[c].shape[:2]) - 1
        p[c][:, :, 1:] = rng.integers(-1, 2, p[c][:, :, 1:].shape)
    return 16, 16, 50, 2, p


def _dummy_blocks():
    """pixels through the front end at 4:2:0 on partial MCUs (24 x 8: the right half of an MCU and the lower half are dummy blocks):
    the dummy blocks carry the DC of the block before them"""
    px = noise(24, 8, 3)
    return 24, 8, 95, 2, model.planes_of(px, 95, 2)


def _row_of_1024():
    """8 x 8192: one interval of 1024 blocks per AC scan, sparse coefficients, long end-of-band runs"""
    p = _empty(8, 8192, 0)
    rng = np.random.default_rng(11)
    for c in range(3):
        p[c][0, :, 0] = rng.integers(-200, 200, 1024)
        idx = rng.integers(0, 1024, 60)
        p[c][0, idx, rng.integers(1, 64, 60)] = rng.integers(-9, 10, 60)
    return 8, 8192, 85, 0, p


BUILDERS = {
    "eob_whole_interval": (_eob_whole_interval, ("eobrun_whole_interval",)),
    "run_broken_in_last_block": (_run_broken_in_last_block, ("run_broken_in_last_block",)),
    "zrl_chains": (_zrl_chains, ("zrl_first", "zrl_refine")),
    "refine_no_trailing_zrl": (_refine_no_trailing_zrl, ("refine_zrl_suppressed", "refine_trailing_zeros_no_zrl")),
    "early_flush": (_early_flush, ("corr_bits_early_flush",)),
    "extreme_444": (lambda: _extreme(0), ("ac_size_9_al1", "ac_size_8_al2", "dc_size_10")),
    "extreme_420": (lambda: _extreme(2), ("ac_size_9_al1", "ac_size_8_al2", "dc_size_10")),
    "negative_dc_and_ones": (_negative_dc_and_ones, ("dc_negative_shift", "ac_shifted_to_zero")),
    "dummy_blocks": (_dummy_blocks, ("dc_negative_shift",)),
    "row_of_1024": (_row_of_1024, ("eobrun_block", "eobrun_restart")),
}
NAMES = list(BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (h, w, quality, sampling, flat int16 [blocks][64])"""
    h, w, q, s, planes = BUILDERS[name][0]()
    flat = model.flat_coefs(planes)
    flat.setflags(write=False)
    return h, w, q, s, flat


@functools.lru_cache(maxsize=None)
def want(name):
    """-> (the model's file, the events it counted)"""
    h, w, q, s, flat = case(name)
    model.EVENTS.clear()
    f = model.file_from_planes(model.planes_from_flat(flat, h, w, s), h, w, q, s)
    return f, dict(model.EVENTS)
