"""Service level of the any-size path: the Python host's restoreImage seam (restorator.py::EngineRestorer) hands an upload of any
size to the engine as ONE batcher job -- no host pad, no classifier-only call, no PNG decode + crop -- and, on an engine created with
IRE_FLAG_RESULT_PNG_BASE64, returns the device's text as it is."""
import base64
import io

import numpy as np
import pytest

from image_restoration_platform_amd import _lib
from image_restoration_platform_amd.engine import Engine
from image_restoration_platform_amd.restorator import EngineClassifier, EngineRestorer, RestoratorService
from oracle import encode as oenc

pytestmark = pytest.mark.gpu


def _upload(h, w, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    rgb = np.clip(rng.integers(0, 256, (1, 1, 3)) + np.linspace(0, 50, w)[None, :, None] + rng.normal(0, 10, (h, w, 3)), 0, 255).astype(np.uint8)
    bio = io.BytesIO()
    Image.fromarray(rgb, "RGB").save(bio, format="PNG")
    return rgb, bio.getvalue()


def _reference(engine, rgb):
    h, w, _ = rgb.shape
    H, W = max(16, -(-h // 8) * 8), max(16, -(-w // 8) * 8)
    sc, _ = engine.classify(rgb[None], False)
    return engine.restore(np.pad(rgb, ((0, H - h), (0, W - w), (0, 0)), mode="edge")[None], scores=sc)[0, :h, :w]


def _decode(text):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(base64.b64decode(text))).convert("RGB"))


@pytest.mark.parametrize("h,w", [(70, 101), (8, 8)])
def test_restorer_returns_the_device_text_for_any_size(engine, h, w):
    rgb, buf = _upload(h, w, seed=h + w)
    ref = _reference(engine, rgb)
    eng = Engine(max_batch=4, flags=_lib.IRE_FLAG_RESULT_PNG_BASE64)
    try:
        restorer = EngineRestorer(eng, result_codec="png-device")
        before = eng.stats()["batches"]
        res = restorer.restore_image("restore", [buf])
        assert eng.stats()["batches"] - before == 1             # no cached scores: classified inside the same batch, no second call
        text = res["base64Image"]
        assert text.encode("ascii") == oenc.png_base64(ref)     # the device's own file, not a host re-encode
        back = _decode(text)
        assert back.shape == (h, w, 3) and np.array_equal(back, ref)
        # with the scores analyze() cached: the same pixels, again one batch
        before = eng.stats()["batches"]
        EngineClassifier(eng).analyze(buf)
        res2 = restorer.restore_image("restore", [buf])
        assert eng.stats()["batches"] - before == 1
        assert res2["base64Image"] == text
        # the whole service on top of it
        out = RestoratorService(engine=eng).restore(buf)
        assert out["success"] and np.array_equal(_decode(out["restoredImage"]), ref)
    finally:
        eng.close()


def test_restorer_on_an_unflagged_engine_crops_on_the_device(engine):
    rgb, buf = _upload(70, 101, seed=3)
    ref = _reference(engine, rgb)
    for codec in ("png", "png-device"):
        res = EngineRestorer(engine, result_codec=codec).restore_image("restore", [buf])
        back = _decode(res["base64Image"])
        assert back.shape == (70, 101, 3) and np.array_equal(back, ref)
        if codec == "png-device":
            assert res["base64Image"].encode("ascii") == oenc.png_base64(ref)
