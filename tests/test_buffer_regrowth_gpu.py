"""Every scratch buffer the engine owns (csrc/device_buf.hpp) grows, is reused at a smaller size and grows again inside ONE engine; each
result must equal, byte for byte, what a fresh engine returns for that single call.  No tolerance, and no allocation failure here:
that is exercised on the CPU (tests/test_device_buf.py)."""
import numpy as np
import pytest

from image_restoration_platform_amd import synth

pytestmark = pytest.mark.gpu


def _restore(n, h, w):
    x = synth.batch(n, h, w, start=h + w)
    return lambda e: [e.restore(x)]


def _restore_fit(n, h, w):
    x = synth.batch(n, h, w, start=h + w)
    return lambda e: [e.restore_fit(x)]


def _classify(n, h, w):
    x = synth.batch(n, h, w, start=3)
    return lambda e: list(e.classify(x))


def _png_texts(n, h, w):
    x = synth.batch(n, h, w, start=11)
    return lambda e: [np.frombuffer(t, np.uint8) for t in e.encode_png_base64_fit(x) + e.encode_png_deflate_base64_fit(x)]


def _preprocess(h, w, max_dim):
    x = synth.image(5, h, w)
    return lambda e: [e.preprocess(x, max_dim=max_dim)]


def _fuse(k, hw):
    v = np.ascontiguousarray(synth.fusion_views(hw, hw)[:k])
    return lambda e: list(e.fuse(v))


def _tiled(h, w, nstrips):
    x = synth.image(9, h, w)

    def call(e):
        import torch
        out = e.restore_tiled_tensor(torch.from_numpy(x).cuda(), nstrips)
        torch.cuda.synchronize()
        return [out.cpu().numpy()]
    return call


CALLS = [
    ("restore 1x64x64", _restore(1, 64, 64)),
    ("restore 3x128x64", _restore(3, 128, 64)),
    ("restore 1x64x64 again", _restore(1, 64, 64)),
    ("restore_fit 2x50x70", _restore_fit(2, 50, 70)),
    ("restore_fit 1x9x131", _restore_fit(1, 9, 131)),
    ("classify 4x33x17", _classify(4, 33, 17)),
    ("png texts 2x24x40", _png_texts(2, 24, 40)),
    ("png texts 1x8x8", _png_texts(1, 8, 8)),
    ("preprocess 100x60 -> 48", _preprocess(100, 60, 48)),
    ("preprocess 300x200 -> 128", _preprocess(300, 200, 128)),
    ("fuse k=2 64x64", _fuse(2, 64)),
    ("fuse k=2 128x128", _fuse(2, 128)),
    ("fuse k=2 64x64 again", _fuse(2, 64)),
    ("tiled 256x64 in 2", _tiled(256, 64, 2)),
    ("tiled 256x128 in 2", _tiled(256, 128, 2)),
]


def test_results_survive_growth_reuse_and_regrowth():
    from image_restoration_platform_amd.engine import Engine
    one = Engine(device_index=0, max_batch=4)
    try:
        got = [(name, call(one)) for name, call in CALLS]
    finally:
        one.close()
    for (name, call), (_, have) in zip(CALLS, got):
        fresh = Engine(device_index=0, max_batch=4)
        try:
            want = call(fresh)
        finally:
            fresh.close()
        assert len(have) == len(want) and len(want) > 0, name
        for a, b in zip(have, want):
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), name
