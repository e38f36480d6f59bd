"""The batched preprocess (ire_preprocess_batch_device, Engine.preprocess_batch) against oracle.preprocess.preprocess_pixels, image by
image and byte for byte: all eight orientations at every stored size below, batches of 1 and 3 with image pitches larger than the
images (odd pads: the byte-wide stores; multiples of 4: the word-wide ones), the bytes between the output images untouched, a second
call equal to the first (the tap cache) and two size pairs alternating.

Stored sizes (w x h -> max_dim) and what each is there for:
  300 x 257 -> 128   ragged tiles both ways (32 x 32 tiles), scale 2.3
  131 x 97  -> 64    odd sizes, more than one tile
  520 x 40  -> 128   an output of 10 rows or fewer: fewer rows than a tile
  2049 x 16 -> 2048  scale just above 1 (7 taps), wide: 65 tiles along x
  700 x 700 -> 5     scale 140: the tile no longer fits in LDS, the strip form of the horizontal pass
  37 x 1, 1 x 37 -> 16   one row, one column
  64 x 48   -> 64    nothing resized: the orient-only kernels (orientation 1: one strided copy)"""
import functools

import numpy as np
import pytest
import torch

from oracle import preprocess as opp

pytestmark = pytest.mark.gpu

SIZES = [(300, 257, 128), (131, 97, 64), (520, 40, 128), (2049, 16, 2048), (700, 700, 5), (37, 1, 16), (1, 37, 16), (64, 48, 64)]
SENTINEL = 0xA7


@functools.lru_cache(maxsize=None)
def _stored(w, h):
    rng = np.random.default_rng(1000 * w + h)
    a = rng.integers(0, 256, (3, h, w, 3), dtype=np.uint8)
    a[1] = (np.add.outer(np.arange(h) * 3, np.arange(w) * 5)[:, :, None] + np.array([0, 85, 170])).astype(np.uint8)      # ramps: an edge that a misplaced tap moves
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _want(w, h, max_dim, orientation):
    """the oracle's three images of this case: computed once, shared by every test that needs them"""
    out = np.stack([opp.preprocess_pixels(img, orientation, max_dim)[0] for img in _stored(w, h)])
    out.setflags(write=False)
    return out


def _run(engine, stored, orientation, max_dim, pad_in, pad_out):
    """-> (the n output images, the bytes between and behind them) through buffers whose images lie pad bytes further apart than they are long"""
    n, h, w, _ = stored.shape
    ow, oh, _ = engine.preprocess_plan(w, h, orientation, max_dim)
    ib, ob = h * w * 3, oh * ow * 3
    src = torch.full((n, ib + pad_in), 0x11, dtype=torch.uint8, device="cuda")
    src[:, :ib] = torch.from_numpy(np.array(stored).reshape(n, ib)).cuda()      # (a writable copy: the shared inputs stay read-only)
    dst = torch.full((n, ob + pad_out), SENTINEL, dtype=torch.uint8, device="cuda")
    out = engine.preprocess_batch(src[:, :ib].view(n, h, w, 3), orientation, max_dim, out_u8=dst[:, :ob].view(n, oh, ow, 3))
    torch.cuda.synchronize()
    host = dst.cpu().numpy()
    return out.cpu().numpy(), host[:, ob:]


@pytest.mark.parametrize("orientation", range(1, 9))
@pytest.mark.parametrize("w,h,max_dim", SIZES)
def test_batch_equals_the_oracle(engine, w, h, max_dim, orientation):
    stored, want = _stored(w, h), _want(w, h, max_dim, orientation)
    for n, pad_in, pad_out in ((1, 0, 0), (3, 37, 29), (3, 64, 128)):
        got, gaps = _run(engine, np.ascontiguousarray(stored[:n]), orientation, max_dim, pad_in, pad_out)
        assert got.shape == want[:n].shape
        for i in range(n):
            assert np.array_equal(got[i], want[i]), (n, i, pad_in, pad_out, int(np.abs(got[i].astype(int) - want[i]).max()))
        assert np.all(gaps == SENTINEL), (n, pad_in, pad_out)


@pytest.mark.parametrize("orientation", (1, 6))
@pytest.mark.parametrize("side", (2048, 2304))
def test_both_sides_of_the_scale_switch(engine, side, orientation):
    """side x side -> 128.  2048: scale 16, 97 taps, a tile's span is 31 * 16 + 97 = 593 input pixels = 59.3 KB of LDS, the largest tiles
    the tiled kernel is given; 2304: scale 18, 109 taps, 667 pixels = 66.7 KB, above the 64 KB switch: the strip form.  One image each."""
    rng = np.random.default_rng(side + orientation)
    stored = rng.integers(0, 256, (1, side, side, 3), dtype=np.uint8)
    got, gaps = _run(engine, stored, orientation, 128, 0, 17)
    assert np.array_equal(got[0], opp.preprocess_pixels(stored[0], orientation, 128)[0]) and np.all(gaps == SENTINEL)


def test_batch_equals_the_single_image_entry(engine):
    """image i's bytes are those ire_preprocess_device gives for it alone"""
    for w, h, max_dim, o in ((300, 257, 128, 6), (131, 97, 64, 4), (700, 700, 5, 7), (64, 48, 64, 5)):
        stored = np.array(_stored(w, h))      # (a writable copy)
        got, _ = _run(engine, stored, o, max_dim, 5, 3)
        for i in range(3):
            assert np.array_equal(got[i], engine.preprocess_tensor(torch.from_numpy(stored[i]).cuda(), o, max_dim).cpu().numpy())


def test_a_second_call_and_alternating_pairs(engine):
    """the cached tap tables: the same sizes again, then two size pairs in turn, more than once"""
    a, b = (300, 257, 128, 6), (131, 97, 64, 3)
    first = {c: _run(engine, np.ascontiguousarray(_stored(c[0], c[1])), c[3], c[2], 37, 29)[0] for c in (a, b)}
    for c in (a, a, b, a, b, a, b, b):
        got, gaps = _run(engine, np.ascontiguousarray(_stored(c[0], c[1])), c[3], c[2], 37, 29)
        assert np.array_equal(got, first[c]) and np.array_equal(got, _want(c[0], c[1], c[2], c[3])) and np.all(gaps == SENTINEL)


def test_more_pairs_than_the_cache_holds(engine):
    """twenty (in, out) pairs through a cache of sixteen, then the first ones again: a replaced table is rebuilt, not reused"""
    stored = np.ascontiguousarray(_stored(131, 97)[:1])
    dims = list(range(40, 60))
    for max_dim in dims + dims[:3]:
        got, _ = _run(engine, stored, 1, max_dim, 0, 0)
        assert np.array_equal(got[0], opp.preprocess_pixels(stored[0], 1, max_dim)[0]), max_dim


def test_wrong_arguments_are_refused(engine):
    from image_restoration_platform_amd.engine import EngineError
    x = torch.zeros((9, 16, 16, 3), dtype=torch.uint8, device="cuda")
    with pytest.raises(EngineError) as e:
        engine.preprocess_batch(x, 1, 8)                       # n > max_batch (8)
    assert e.value.status == 1 and "batch size" in e.value.message
    y = torch.zeros((2, 16 * 16 * 3 + 8), dtype=torch.uint8, device="cuda")
    lib, out = engine._lib, torch.zeros((2, 8, 8, 3), dtype=torch.uint8, device="cuda")
    import ctypes
    args = lambda ip, op: (engine._h, ctypes.c_void_p(y.data_ptr()), 2, 16, 16, ip, 1, 8, ctypes.c_void_p(out.data_ptr()), 8, 8, op, None)      # noqa: E731
    assert lib.ire_preprocess_batch_device(*args(16 * 16 * 3 - 1, 8 * 8 * 3)) == 1 and b"pitch" in lib.ire_last_error()
    assert lib.ire_preprocess_batch_device(*args(16 * 16 * 3, 8 * 8 * 3 - 1)) == 1 and b"pitch" in lib.ire_last_error()
    assert lib.ire_preprocess_batch_device(*args(16 * 16 * 3 + 8, 8 * 8 * 3)) == 0
    torch.cuda.synchronize()
