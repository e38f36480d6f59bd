"""csrc/gn_fold.hpp's reduction at every pass structure it runs -- full passes of the 8-chain unrolled loop, tail steps, idle lanes and
their mixes -- judged against float64 within the derived bound of oracle/layer_check.py (module docstring: the partials-level check).

Direct: the standalone finalize kernel on given partials (Engine.debug_gn_finalize), over tests/gn_cases.py's sweep of P (partials per
image) and every width; tests/test_gn_cases.py shows on the CPU that these partials put any single dropped, repeated, rotated or
exchanged partial outside the bound at every P.  In the network: the coefficients every activated convolution applied
(NetworkCheck.run_coeffs), at two shapes whose levels reach the unrolled loop -- 3 x 272 x 1000 (P = 544 / 144 / 40 / 12) and the
benchmark's 1024 x 1024 (P = 2048 / 512 / 128 / 32) -- on the default engine (conv_pc / conv_pk prologues), with IRE_PC=0 (conv_rb's
prologue at C = 32 / 64 and in the head), with IRE_GN_FOLD=0 (the standalone kernel) and on the fp8 engine (conv_f8, conv_w4)."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gn_cases as gc      # noqa: E402
from image_restoration_platform_amd import _lib, synth      # noqa: E402
from image_restoration_platform_amd.engine import EngineError      # noqa: E402
from oracle import classifier as oc      # noqa: E402
from oracle import layer_check as lc      # noqa: E402

pytestmark = pytest.mark.gpu


# ---- the standalone kernel on given partials ------------------------------------------------------------------------------
def _judge(label, P, C, ab, ref):
    assert ab.dtype == np.float32 and ab.shape == ref[0].shape + (2,), (label, ab.shape)
    msg = lc.check_coeffs(label, ab.astype(np.float64), ref)
    assert not msg, "P %d C %d, lanes take (full passes, tail steps) %s: %s" % (P, C, gc.regimes(P), msg)
    return lc.coeff_share(ab.astype(np.float64), ref)


def _run_case(engine, c):
    C, off = c["C"], c["film_off"]
    ab = engine.debug_gn_finalize(c["stats"], c["hw"], c["gamma"], c["beta"], c["film"], off)
    return _judge(c["name"], c["stats"].shape[1], C, ab, gc.case_reference(lc, c))


@pytest.mark.parametrize("P", gc.SWEEP)
def test_coded_partials_at_every_pass_structure(engine, P):
    """One call per (P, C) with all images of the code; the sums of the reference are exact (integers)."""
    st = gc.coded_partials(P)
    t0 = time.perf_counter()
    tot, mag = lc.partial_sums(st)
    host, dev, shares = time.perf_counter() - t0, 0.0, []
    for C in gc.WIDTHS:
        g, b = gc.coded_gamma_beta(C)
        t0 = time.perf_counter()
        ab = engine.debug_gn_finalize(st, gc.hw_for(P, C), g, b)
        t1 = time.perf_counter()
        shares.append(_judge("coded partials", P, C, ab, lc.coeffs_from_sums(tot, mag, P, gc.hw_for(P, C), C, g, b)))
        dev, host = dev + t1 - t0, host + time.perf_counter() - t1
    print("GNFOLD direct P %6d | %2d images | regimes %s | share of the bound used per width %s | calls (copies + kernel) %.3f s, reference %.3f s"
          % (P, st.shape[0], gc.regimes(P), " ".join("%.2f" % s for s in shares), dev, host))


@pytest.mark.parametrize("case", gc.float_cases(), ids=lambda c: c["name"].replace(" ", "_"))
def test_float_cases(engine, case):
    print("GNFOLD float | %s | P %d C %d | share of the bound used %.2f" % (case["name"], case["stats"].shape[1], case["C"], _run_case(engine, case)))


def test_64_images_in_one_call(engine):
    c = gc.many_images_case()
    ab = engine.debug_gn_finalize(c["stats"], c["hw"], c["gamma"], c["beta"], c["film"], c["film_off"])
    _judge(c["name"], c["stats"].shape[1], c["C"], ab, gc.case_reference(lc, c))
    # an image's coefficients do not depend on its place in the call, or on the call's size
    one = engine.debug_gn_finalize(c["stats"][37:38], c["hw"], c["gamma"], c["beta"], c["film"][37:38], c["film_off"])
    assert np.array_equal(one[0].view(np.uint32), ab[37].view(np.uint32))


def test_two_calls_of_different_sizes(engine):
    """Nothing of a call outlives it: a large call, a small one, the large one again."""
    big, small = gc.coded_partials(2048), gc.float_cases()[-2]
    g, b = gc.coded_gamma_beta(256)
    first = engine.debug_gn_finalize(big, gc.hw_for(2048, 256), g, b)
    _run_case(engine, small)
    assert np.array_equal(engine.debug_gn_finalize(big, gc.hw_for(2048, 256), g, b).view(np.uint32), first.view(np.uint32))
    _judge("coded partials", 2048, 256, first, lc.coeffs_from_partials(big, gc.hw_for(2048, 256), 256, g, b))


def test_refusals_leave_the_engine_usable(engine):
    st, g, film, out = np.zeros((2, 4, 8, 2), np.float32), np.ones(32, np.float32), np.zeros((2, 70), np.float32), np.zeros((2, 32, 2), np.float32)
    p = lambda a: None if a is None else a.ctypes.data

    def call(stats=st, nimg=2, parts=4, C=32, hw=64, gamma=g, beta=g, fm=None, stride=0, off=0, ab=out):
        rc = engine._lib.ire_debug_gn_finalize(engine._h, p(stats), nimg, parts, C, hw, p(gamma), p(beta), p(fm), stride, off, p(ab))
        return rc, (engine._lib.ire_last_error() or b"").decode()

    assert call()[0] == 0 and call(fm=film, stride=70, off=6)[0] == 0          # the last window that fits: 6 + 64 = 70
    for kw, word in ([dict(C=c), "channels"] for c in (0, 8, 48, 96, 512, -32)):
        assert call(**kw)[0] == _lib.IRE_ERR_INVALID_INPUT and word in call(**kw)[1], kw
    for kw, word in ((dict(nimg=0), "images"), (dict(nimg=65536), "images"), (dict(nimg=-1), "images"), (dict(parts=0), "parts"),
                     (dict(parts=(1 << 20) + 1), "parts"), (dict(hw=0), "hw"), (dict(hw=-5), "hw"), (dict(stats=None), "null"), (dict(gamma=None), "null"),
                     (dict(beta=None), "null"), (dict(ab=None), "null"), (dict(fm=film, stride=70, off=7), "film window"),
                     (dict(fm=film, stride=70, off=-1), "film window"), (dict(fm=film, stride=63, off=0), "film window")):
        rc, msg = call(**kw)
        assert rc == _lib.IRE_ERR_INVALID_INPUT and word in msg and "invalid" in msg, (kw, rc, msg)
    assert engine._lib.ire_debug_gn_finalize(None, p(st), 2, 4, 32, 64, p(g), p(g), None, 0, 0, p(out)) == _lib.IRE_ERR_INVALID_INPUT
    with pytest.raises(EngineError, match="channels"):
        engine.debug_gn_finalize(st, 64, np.ones(40, np.float32), np.ones(40, np.float32))
    _run_case(engine, gc.float_cases()[0])


# ---- in the network: the coefficients every activated convolution applied ------------------------------------------------
SHAPES = {"3x272x1000": (3, 272, 1000, 21), "1x1024x1024": (1, 1024, 1024, 0)}
_default_ab = {}             # shape -> {layer: captured .ab of the default engine} (the IRE_GN_FOLD=0 run compares with them bit for bit)


def _inputs(shape):
    n, h, w, start = SHAPES[shape]
    imgs = synth.batch(n, h, w, start=start)
    # any 7 scores do: those of the images' top-left 64 x 64 (the classifier's oracle is slow on a megapixel)
    return imgs, np.stack([oc.classify(np.ascontiguousarray(im[:64, :64]), True)[0] for im in imgs])


def _parts(shape, level):
    _, h, w, _ = SHAPES[shape]
    return -(-(h >> level) // lc.TILE_H) * -(-(w >> level) // lc.TILE_W)


def _parts_of(shape, nm):
    """Partials per image of the tensor layer `nm` normalises: one per 16 x 32 tile of its level -- but the composed up + fuse convolution
    writes one per tile of its LOW-res input (conv_plan.hpp: stats_level = lin), four at cout = 128 (conv_upq), and dec{l}.rb0.h reads those."""
    l = lc._level(nm)
    if nm.startswith("dec") and nm.endswith(".rb0.h"):
        return _parts(shape, l + 1) * (4 if l == 2 else 1)
    return _parts(shape, l)


def _check_network(eng, weights0, shape, label, fp8=False):
    imgs, sc = _inputs(shape)
    t0 = time.perf_counter()
    eng.debug_capture(True)
    try:
        out = eng.restore(imgs, scores=sc)
        t1 = time.perf_counter()
        nc = lc.NetworkCheck(weights0, imgs, sc, eng.activation, out, fp8=fp8)
        msgs = nc.run_coeffs()
        abs_ = {nm: eng.activation(("head" if nm == "pixels" else nm) + ".ab") for nm in msgs}
    finally:
        eng.debug_capture(False)
    t2 = time.perf_counter()
    assert set(msgs) == {nm for nm in lc.layer_names("fused") if ".rb" in nm} | {"pixels"} and len(msgs) == 33       # no GroupNorm exempt
    bad = ["%s (P = %d: lanes take %s)" % (m, _parts_of(shape, nm), gc.regimes(_parts_of(shape, nm))) for nm, m in msgs.items() if m]
    assert not bad, "%s %s: %d layer(s) with coefficients outside the derived bound:\n  %s" % (label, shape, len(bad), "\n  ".join(bad))
    assert np.array_equal(eng.restore(imgs, scores=sc), out), label + ": the pixels of a run with debug capture differ from an ordinary run's"
    for P in sorted({_parts_of(shape, nm) for nm in msgs}, reverse=True):   # information (pytest -s), not a threshold
        names = [nm for nm in msgs if _parts_of(shape, nm) == P]
        print("GNFOLD network %s %s | P %5d regimes %s | %2d layers | share of the coefficients' bound used %.3f"
              % (label, shape, P, gc.regimes(P), len(names), max(nc.coeff_share[nm] for nm in names)))
    print("GNFOLD network %s %s | run with capture %.2f s, float64 moments and check %.2f s" % (label, shape, t1 - t0, t2 - t1))
    return abs_


def _default(engine, weights0, shape):
    if shape not in _default_ab:
        _default_ab[shape] = _check_network(engine, weights0, shape, "default")
    return _default_ab[shape]


@pytest.mark.parametrize("shape", list(SHAPES))
def test_network_default_engine(engine, weights0, shape):
    """272 x 1000: P = 544 at level 0 (every lane one full pass, half of them one tail step), three images (the images behind a
    workgroup's first take their gamma, beta and FiLM after the reduction).  1024 x 1024: 4 and 1 clean passes, 2 tail steps, idle lanes."""
    assert [_parts(shape, l) for l in range(4)] == {"3x272x1000": [544, 144, 40, 12], "1x1024x1024": [2048, 512, 128, 32]}[shape]
    assert [_parts_of(shape, "dec%d.rb0.h" % l) for l in range(3)] == {"3x272x1000": [144, 40, 48], "1x1024x1024": [512, 128, 128]}[shape]
    _default(engine, weights0, shape)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("env", ["IRE_PC", "IRE_GN_FOLD"])
def test_network_behind_a_switch(engine, weights0, shape, env, monkeypatch):
    """IRE_PC=0: conv_rb's prologue at C = 32 / 64 and in the head.  IRE_GN_FOLD=0: gn_finalize_kernel between the convolutions; its
    coefficients equal the folded prologues' bit for bit."""
    from image_restoration_platform_amd.engine import Engine
    monkeypatch.setenv(env, "0")
    eng = Engine(device_index=0, max_batch=8)
    try:
        abs_ = _check_network(eng, weights0, shape, env + "=0")
    finally:
        eng.close()
    if env == "IRE_GN_FOLD":
        ref = _default(engine, weights0, shape)
        diff = [nm for nm in ref if not np.array_equal(ref[nm].view(np.uint32), abs_[nm].view(np.uint32))]
        assert not diff, "coefficients of the standalone finalize differ from the folded prologue's at %s" % diff


@pytest.mark.parametrize("mx", ["1", "0"])
def test_network_fp8_engine(weights0, mx, monkeypatch):
    """conv_f8.hip's prologue (IRE_FP8_MX=1) and conv_w4.hip's (0) at C >= 128, at P = 40 and 12; level 0 as on the bf16 engine."""
    from image_restoration_platform_amd.engine import Engine
    monkeypatch.setenv("IRE_FP8_MX", mx)
    eng = Engine(device_index=0, max_batch=8, precision="fp8")
    try:
        _check_network(eng, weights0, "3x272x1000", "fp8 mx=" + mx, fp8=True)
    finally:
        eng.close()
