"""Any-size jobs through the Node seam (node/engine_adapters.js over node/ire_napi.cc): one ragged image is one batcher job; with
resultCodec 'png-device' the base64Image is the device's own text."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from image_restoration_platform_amd import synth, weights
from oracle import encode as oenc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE_DIR = os.path.join(ROOT, "image_restoration_platform_amd", "node")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(shutil.which("node") is None, reason="node is not installed")]


def test_node_restores_a_ragged_image_as_one_job_and_returns_the_device_text(engine, tmp_path):
    img = np.ascontiguousarray(synth.image(1, 72, 104)[:70, :101])
    f = tmp_path / "a.raw"
    f.write_bytes(b"RAW1" + bytes([101, 0, 70, 0, 1]) + img.tobytes())
    spec = tmp_path / "case.json"
    spec.write_text(json.dumps({"weights": weights.ensure_default(0), "image": str(f), "h": 70, "w": 101}))
    r = subprocess.run(["node", os.path.join(NODE_DIR, "test_fit.js"), str(spec)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:] + r.stdout[-2000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    scores, _ = engine.classify(img, is_jpeg=True)
    ref = np.ascontiguousarray(engine.restore(np.pad(img, ((0, 2), (0, 3), (0, 0)), mode="edge"), scores=scores, is_jpeg=True)[0][:70, :101])
    assert out["pixels"] == {"sha": hashlib.sha256(ref.tobytes()).hexdigest(), "batches": 1}
    want = oenc.png_base64(ref)
    assert out["text"] == {"chars": len(want), "want": len(want), "sha": hashlib.sha256(want).hexdigest(), "head": "PNG", "batches": 1}
    assert out["concurrent"]["allEqual"] is True and out["concurrent"]["batches"] <= 2
    assert out["alignedRule"] == {"bytes": 0}
