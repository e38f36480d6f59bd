"""The scratch buffers the engine owns (csrc/device_buf.hpp) grow, are reused at a smaller size and grow again inside ONE engine; each
result must equal, byte for byte, what a fresh engine returns for that single call, and the call's independent reference where it has
one.  Covered: the network workspace and the staging of the host entries (restore, restore_fit, classify), the stored and deflate PNG
encoders and the three JPEG encoders (TextEncoder's scratch), preprocess and the batch preprocess, fusion, strip sessions, the JPEG
decoder's scratch (baseline, window-parallel: the lane records, progressive: the walk records), the PNG decoder's (the 8-bit form and
16-bit Adam7), the ICC converter's, and the batcher's slots with the decoders' batch halves (an upload job and a fusion job).  What a
fresh engine cannot show -- a kernel that relies on zero, which fresh memory is -- is tests/test_poison_gpu.py's.  No tolerance, and no
allocation failure here: that is exercised on the CPU (tests/test_device_buf.py)."""
import os
import sys

import numpy as np
import pytest

from image_restoration_platform_amd import _lib, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
FLAGS = _lib.IRE_FLAG_DECODE_PNG | _lib.IRE_FLAG_DECODE_PNG_ALL | _lib.IRE_FLAG_DECODE_PROGRESSIVE | _lib.IRE_FLAG_UPLOAD_ICC


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


# ---- the codecs and the jobs: (name, call, the reference or None, whether the call needs the network's weights) -------------------------------
def _jpeg_files():
    import jpeg_decode_cases as jc
    import jpeg_decode_model as jm
    import jpeg_prog_writer as writer
    from test_jpeg_decode_gpu import _consts
    window_bits, short = _consts()
    many, side = [], 64
    while len(many) < 2:                # two streams of several windows, the second the longer
        data = jc.encode(jc.noise(side, side, 77), 95, 0)
        if 8 * len(jm.plan(data).streams[0][0]) >= (2.5 if not many else 3.5) * window_bits:
            many.append(data)
        side += 32
    one = jc.encode(jc.noise(96, 96, 42), 95, 2)
    assert short < len(jm.plan(one).streams[0][0]) <= window_bits // 8
    return [("jpeg decode 33x47 4:2:0", jc.encode(jc.noise(47, 33, 332), 85, 2)), ("jpeg decode 8x8", jc.encode(jc.noise(8, 8, 80), 85, 0)),
            ("jpeg decode 64x48 q100", jc.encode(jc.noise(48, 64, 4), 100, 0)),
            ("jpeg decode several windows", many[0]), ("jpeg decode one window", one), ("jpeg decode more windows", many[1]),
            ("progressive decode 17x13", writer.pillow_progressive(jc.noise(13, 17, 2), 85, 2)), ("progressive decode 8x8", writer.pillow_progressive(jc.noise(8, 8, 1), 85, 0)),
            ("progressive decode 33x47", writer.pillow_progressive(jc.noise(47, 33, 4), 85, 2))]


def _codec_calls():
    import torch
    import icc_cases
    import icc_model
    import jpeg_decode_cases as jc
    import jpeg_huffopt_cases as hc
    import jpeg_huffopt_model as huffopt
    import jpeg_opt_model as opt
    import jpeg_progenc_model as progenc
    import png_cases as pc
    import png_depth_cases as pd
    import upload_cases as uc
    from image_restoration_platform_amd.engine import icc_plan_profile
    from oracle import preprocess as opp
    from test_fusion_jobs_gpu import _reference, _views
    calls = []
    for name, data in _jpeg_files():
        calls.append((name, (lambda d: lambda e: [e.decode_jpeg(d)])(data), [jc.pillow_pixels(data)], False))
    for name, data in [("png decode 24x20 rgb", pc.make(24, 20, 2)), ("png decode 5x7 palette", pc.make(5, 7, 3)), ("png decode 48x40 rgba", pc.make(48, 40, 6)),
                       ("png decode 16-bit Adam7 24x20", pd.make(24, 20, 6, 16, 1, seed=5)), ("png decode 16-bit Adam7 5x3", pd.make(5, 3, 6, 16, 1, seed=8)),
                       ("png decode 16-bit Adam7 33x70", pd.make(33, 70, 6, 16, 1, seed=3))]:
        calls.append((name, (lambda d: lambda e: [e.decode_png(d)])(data), [pd.pil_rgb(data)], False))
    profiles = [icc_cases.rgb_profiles()[n] for n in ("p3_v4", "adobe_v2", "table18", "three_curves")]
    plans = [icc_plan_profile(p, 3)[0] for p in profiles]
    tables = [icc_model.plan_profile(p, 3) for p in profiles]
    for n, h, w in ((2, 33, 31), (1, 5, 7), (4, 64, 64)):
        px = np.random.default_rng(n * h).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
        want = np.stack([icc_model.apply(tables[i], px[i]) for i in range(n)]).astype(np.uint8)
        calls.append(("to_srgb %dx%dx%d" % (n, h, w), (lambda x, k: lambda e: [e.icc_to_srgb(x, plans[:k])])(px, n), [want], False))
    as_bytes = lambda t: np.frombuffer(t if isinstance(t, bytes) else t.encode(), np.uint8)      # noqa: E731
    for label, model, kw in (("jpeg encode", opt, dict(optimize=False, progressive=False)), ("optimised jpeg encode", huffopt, dict(optimize=True, progressive=False)),
                             ("progressive jpeg encode", progenc, dict(progressive=True))):
        for (h, w), q, s in (((45, 37), 85, 0), ((8, 8), 85, 0), ((72, 40), 60, 2)):
            px = hc.noise(h, w, 7 * h + w)
            calls.append(("%s %dx%d" % (label, h, w), (lambda x, q_, s_, kw_: lambda e: [as_bytes(e.encode_jpeg_base64_fit(x, q_, s_, **kw_))])(px, q, s, kw),
                          [as_bytes(model.jpeg_base64(px, q, s))], False))
    for n, h, w, o, m in ((3, 97, 131, 3, 64), (1, 20, 30, 6, 16), (3, 257, 300, 6, 128)):
        stored = np.random.default_rng(h + w).integers(0, 256, (n, h, w, 3), dtype=np.uint8)

        def pp(e, x=stored, o_=o, m_=m):
            out = e.preprocess_batch(torch.from_numpy(x).cuda(), orientation=o_, max_dim=m_)
            torch.cuda.synchronize()
            return [out.cpu().numpy()]
        calls.append(("preprocess batch %dx%dx%d -> %d" % (n, h, w, m), pp, [np.stack([opp.preprocess_pixels(im, o, m)[0] for im in stored])], False))
    # jobs: the reference needs an engine, so it is taken from the fresh one (restore_fit of the oracle's preprocess of Pillow's decode;
    # tests/test_fusion_jobs_gpu.py's composition)
    for w, h, kind, m in ((131, 97, 2, 128), (40, 24, 0, 64), (300, 257, 0, 128)):
        data = uc.encode(uc.smooth(h, w, 7 + w), 85, kind, 6, False)
        fitted = opp.preprocess_pixels(uc.pillow_pixels(data), 6, m)[0]
        calls.append(("upload job %dx%d" % (w, h), (lambda d, m_: lambda e: [e.poll(e.submit_upload(d, max_dim=m_), timeout_ms=120000)[0]])(data, m),
                      (lambda f: lambda e: [e.restore_fit(f)[0]])(fitted), True))
    for h, w, k in ((64, 64, 2), (16, 24, 2), (70, 90, 3)):
        calls.append(("fusion job k=%d %dx%d" % (k, h, w), (lambda h_, w_, k_: lambda e: [e.poll(e.submit_fuse_fit(_views(h_, w_, k_)), timeout_ms=120000)[0]])(h, w, k),
                      (lambda h_, w_, k_: lambda e: [_reference(e, h_, w_, k_)])(h, w, k), True))
    return calls


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


def _same(have, want, name):
    assert len(have) == len(want) and len(want) > 0, name
    for a, b in zip(have, want):
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b), name


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
        _same(have, want, name)


def test_the_codecs_and_the_jobs_survive_growth_reuse_and_regrowth():
    """a grow / smaller / regrow triple of every decoder, the ICC converter, the three JPEG encoders, the batch preprocess, an upload job
    and a fusion job on ONE engine: each result equals a fresh engine's and the call's reference"""
    from image_restoration_platform_amd.engine import Engine
    calls = _codec_calls()
    assert len(calls) == 9 + 6 + 3 + 9 + 3 + 3 + 3
    one = Engine(device_index=0, max_batch=4, flags=FLAGS)
    try:
        got = [call(one) for _, call, _, _ in calls]
    finally:
        one.close()
    for (name, call, ref, weights), have in zip(calls, got):
        fresh = Engine(device_index=0, max_batch=4, flags=FLAGS) if weights else Engine(device_index=0, max_batch=4, flags=FLAGS, weights_path=None)
        try:
            want = call(fresh)
            reference = ref(fresh) if callable(ref) else ref
        finally:
            fresh.close()
        _same(have, want, name)
        _same(have, [np.asarray(r).astype(have[0].dtype) if not isinstance(r, np.ndarray) else r for r in reference], name + " (reference)")
