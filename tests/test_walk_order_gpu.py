"""The walk direction of the persistent conv kernels (csrc/persist.hpp, ConvArgs::walk_rev) changes WHEN an item runs, never what it
computes: an engine whose launches alternate directions (the default) restores the same bytes as one whose launches all walk forward
(IRE_SNAKE=0).  Items are independent, GroupNorm partials live in per-tile slots and are reduced in a fixed order, and the k-chunks
of an item stay ascending -- so the comparison is for equality.

A workgroup only has an order to reverse when it has several items.  At the device's own grid size the small shapes a test can afford
leave most workgroups 0 or 1 item, so the multi-item cases run with IRE_GRID_CUS=8 (8 workgroups: 3 or more items each at every
level) -- in one fresh child process, because the library reads that switch once per process."""
import os
import subprocess
import sys

import numpy as np
import pytest

from image_restoration_platform_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import os, sys
import numpy as np
from image_restoration_platform_amd import synth
from image_restoration_platform_amd.engine import Engine

def run(imgs, snake, precision):
    if snake is None: os.environ.pop("IRE_SNAKE", None)
    else: os.environ["IRE_SNAKE"] = snake
    eng = Engine(device_index=0, max_batch=8, num_streams=1, precision=precision)      # the switch is read once per engine
    try:
        return eng.restore(imgs)
    finally:
        eng.close()

a = synth.batch(3, 200, 328, start=21)       # workgroups cross image boundaries at C = 128 / 256
b = synth.batch(8, 48, 80, start=5)          # an eighth of the item range is an image
out = {}
for name, imgs, precision in (("a_bf16", a, "bf16"), ("b_bf16", b, "bf16"), ("a_fp8", a, "fp8")):
    out[name + "_fwd"] = run(imgs, "0", precision)
    out[name + "_snake"] = run(imgs, None, precision)
np.savez(sys.argv[1], **out)
"""


def _restore(imgs, snake, monkeypatch):
    from image_restoration_platform_amd.engine import Engine
    if snake is None:
        monkeypatch.delenv("IRE_SNAKE", raising=False)
    else:
        monkeypatch.setenv("IRE_SNAKE", snake)
    eng = Engine(device_index=0, max_batch=8, num_streams=1)
    try:
        return eng.restore(imgs)
    finally:
        eng.close()


def test_alternating_and_forward_walks_restore_equal_bytes_with_many_items_per_workgroup(tmp_path):
    env = dict(os.environ)
    env["IRE_GRID_CUS"] = "8"
    env.pop("IRE_SNAKE", None)
    env["PYTHONPATH"] = ROOT + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
    path = str(tmp_path / "walks.npz")
    r = subprocess.run([sys.executable, "-c", CHILD, path], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-1000:], r.stderr[-3000:])
    z = np.load(path)
    imgs = {"a": synth.batch(3, 200, 328, start=21), "b": synth.batch(8, 48, 80, start=5)}
    for name in ("a_bf16", "b_bf16", "a_fp8"):
        fwd, snake = z[name + "_fwd"], z[name + "_snake"]
        src = imgs[name[0]]
        assert fwd.shape == src.shape and fwd.dtype == np.uint8
        assert np.abs(fwd.astype(np.int32) - src.astype(np.int32)).mean() > 1.0, name       # the network ran
        assert np.array_equal(fwd, snake), (name, int(np.count_nonzero(fwd != snake)))


def test_alternating_and_forward_walks_restore_equal_bytes_at_the_device_grid(monkeypatch):
    imgs = synth.batch(2, 72, 136, start=11)             # most workgroups have 0 or 1 item
    fwd = _restore(imgs, "0", monkeypatch)
    snake = _restore(imgs, None, monkeypatch)
    assert np.abs(fwd.astype(np.int32) - imgs.astype(np.int32)).mean() > 1.0
    assert np.array_equal(fwd, snake), int(np.count_nonzero(fwd != snake))
