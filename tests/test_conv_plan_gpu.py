"""The engine launches what the plan says: one profiled restore per case, and the kernel of every layer group in profile_report() is
the kernel column (kname) of the CPU fixture for that case (tests/golden/conv_plan_9e80c0a.txt, tests/test_conv_plan.py).  Ordinary restores
at the smallest shapes that take every branch of the chain: (1, 72, 136), (1, 512, 512) -- 128-cout items at level 2, the 64-cout
split at level 3 -- and (12, 32, 48), twelve images per launch; every switch set and both fp8 forms on (1, 72, 136)."""
import pytest

from image_restoration_platform_amd import synth
from test_conv_plan import golden_lines, parse
from test_layers_gpu import SWITCHES

pytestmark = pytest.mark.gpu


def _expected(case):
    want = {g: f["kname"] for c, g, f in map(parse, golden_lines()[1:]) if c == case}
    assert want, case
    return want


def _launched(eng, n, h, w):
    eng.profile_enable(1)
    try:
        eng.profile_reset()
        eng.restore(synth.batch(n, h, w, start=3))
        return {r["group"]: r["kernel"] for r in eng.profile_report()}
    finally:
        eng.profile_enable(0)


def _fresh(n, h, w, **kw):
    from image_restoration_platform_amd.engine import Engine
    eng = Engine(device_index=0, **kw)
    try:
        return _launched(eng, n, h, w)
    finally:
        eng.close()


@pytest.mark.parametrize("n,h,w", [(1, 72, 136), (1, 512, 512), (12, 32, 48)])
def test_default_engine_launches_the_planned_kernels(n, h, w):
    assert _fresh(n, h, w, max_batch=32) == _expected("default:bf16:%dx%dx%d" % (n, h, w))


@pytest.mark.parametrize("env", SWITCHES, ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()))
def test_every_switch_set_launches_the_planned_kernels(env, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    assert _fresh(1, 72, 136, max_batch=8) == _expected(",".join("%s=%s" % kv for kv in env.items()) + ":bf16:1x72x136")


@pytest.mark.parametrize("mx", ["1", "0"])
def test_fp8_engine_launches_the_planned_kernels(mx, monkeypatch):
    monkeypatch.setenv("IRE_FP8_MX", mx)
    assert _fresh(1, 72, 136, max_batch=8, precision="fp8") == _expected("IRE_FP8_MX=%s:fp8:1x72x136" % mx)
