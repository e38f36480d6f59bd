"""GPU parity of the fused classifier scan (through the C ABI) against the CPU oracle: bit-exact
scores, label and integer accumulators (SURVEY.md 8c tolerances)."""
import json
import os
import sys

import numpy as np
import pytest

from image_restoration_platform_amd import synth
from oracle import classifier as oc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import classifier_cases as cc      # noqa: E402

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _check(engine, imgs, is_jpeg, ref=None):
    """ref: the oracle's (scores, label, sums) per image where a caller has them already (classifier_cases.oracle)"""
    scores, labels = engine.classify(imgs, is_jpeg=is_jpeg)
    sums = engine.classifier_sums(len(imgs))
    jp = np.broadcast_to(np.asarray(is_jpeg, dtype=np.uint8), (len(imgs),))
    for i, im in enumerate(imgs):
        s, l, su = ref[i] if ref is not None else oc.classify(im, bool(jp[i]), with_sums=True)
        su = su if isinstance(su, list) else su.as_list()
        assert [int(x) for x in sums[i]] == [int(x) for x in su], (i, im.shape)
        assert np.array_equal(_bits(s), _bits(scores[i])), (i, s, scores[i])   # bit-exact doubles
        assert l == labels[i]


@pytest.mark.parametrize("h,w", [(64, 64), (64, 96), (37, 53), (16, 64), (17, 65), (15, 63), (1, 1), (1, 200),
                                 (130, 1), (3, 5), (256, 256), (200, 120)])
def test_bit_exact_vs_oracle_shapes(engine, h, w):
    imgs = synth.batch(3, max(h, 8), max(w, 8))[:, :h, :w]
    _check(engine, np.ascontiguousarray(imgs), True)


def test_batch8_mixed_jpeg_flags(engine):
    imgs = synth.batch(8, 128, 160)
    _check(engine, imgs, np.array([1, 0, 1, 1, 0, 0, 1, 0], np.uint8))


def test_known_answers_and_golden(engine):
    for c in json.load(open(os.path.join(HERE, "golden", "classifier_kat.json"))):
        h, w = c["size"][1], c["size"][0]
        if "fill" in c:
            img = np.zeros((h, w, 3), np.uint8); img[:] = c["fill"]
        else:
            img = np.random.default_rng(c["rng_seed"]).integers(0, 256, (h, w, 3), dtype=np.uint8)
        s, l = engine.classify(img, is_jpeg=c["is_jpeg"])
        d = dict(zip(oc.KEYS, s[0]))
        for k, v in c.get("expect", {}).items():
            assert d[k] == pytest.approx(v, abs=1e-12), (c["name"], k)
        for k, v in c.get("expect_min", {}).items():       # e.g. noisy_seed1234: noise >= ...
            assert d[k] >= v, (c["name"], k, d[k])
        for k, v in c.get("expect_max", {}).items():
            assert d[k] <= v, (c["name"], k, d[k])
        if "label" in c:
            assert oc.KEYS[l[0]] == c["label"]
    for c in json.load(open(os.path.join(HERE, "golden", "classifier_golden.json"))):
        img = synth.image(c["index"], c["h"], c["w"])
        s, l = engine.classify(img, is_jpeg=bool(c["is_jpeg"]))
        assert [float(x).hex() for x in s[0]] == c["scores_hex"], c["index"]
        assert l[0] == c["label"]


def test_reference_fixtures_through_jpeg_round_trips(engine):
    """classifierService.test.js:19-57 on the GPU: the five fixtures rebuilt through real JPEG round trips
    (tests/ref_fixtures.py <- imageFixtures.js:5-45), the reference's inequalities on the engine's scores, and bit-exact
    agreement with the oracle on those pixels."""
    import sys
    sys.path.insert(0, HERE)
    import ref_fixtures as rf
    imgs = []
    for name, build, check in rf.CASES:
        img = build()
        s, _ = engine.classify(img, is_jpeg=True)
        assert check(dict(zip(oc.KEYS, (float(x) for x in s[0])))), (name, s[0])
        imgs.append(img)
    _check(engine, np.stack(imgs), True)


def test_extreme_pixels(engine):
    rng = np.random.default_rng(7)
    cases = [np.zeros((48, 80, 3), np.uint8), np.full((48, 80, 3), 255, np.uint8),
             (rng.integers(0, 2, (48, 80, 3)) * 255).astype(np.uint8),          # checker-like saturation
             np.tile(np.arange(80, dtype=np.uint8)[None, :, None] * 3, (48, 1, 3))]
    _check(engine, np.stack(cases), True)


def test_full_size_sums_property(engine):
    """At BASELINE sizes the C oracle still finishes in seconds for one image; additionally check the
    size-independent property that the per-channel sums equal numpy's on the whole batch."""
    imgs = synth.batch(2, 1024, 1024)
    _check(engine, imgs[:1], True)
    engine.classify(imgs, is_jpeg=True)
    sums = engine.classifier_sums(2)
    for i in range(2):
        x = imgs[i].astype(np.uint64)
        assert [int(v) for v in sums[i][:3]] == [int(x[..., c].sum()) for c in range(3)]
        assert [int(v) for v in sums[i][3:6]] == [int((x[..., c] ** 2).sum()) for c in range(3)]


def test_row_stride_and_device_path(engine):
    import ctypes
    import torch
    from image_restoration_platform_amd import _lib
    imgs = synth.batch(2, 40, 56)
    # host path with padded rows
    stride = 56 * 3 + 24
    padded = np.zeros((2, 40, stride), np.uint8)
    padded[:, :, :56 * 3] = imgs.reshape(2, 40, -1)
    scores = np.zeros((2, 7)); labels = np.zeros(2, np.int32); jp = np.ones(2, np.uint8)
    rc = _lib.load().ire_classify(engine._h, padded.ctypes.data, 2, 40, 56, stride, jp.ctypes.data, scores.ctypes.data,
                                  labels.ctypes.data)
    assert rc == 0
    ref, _ = engine.classify(imgs, True)
    assert np.array_equal(_bits(scores), _bits(ref))
    # device-pointer path on the torch stream
    x = torch.from_numpy(imgs).cuda()
    s, l = engine.classify_tensor(x, torch.ones(2, dtype=torch.uint8, device="cuda"))
    torch.cuda.synchronize()
    assert np.array_equal(_bits(s.cpu().numpy()), _bits(ref))


def test_invalid_inputs_report_invalid(engine):
    from image_restoration_platform_amd.engine import EngineError
    with pytest.raises(EngineError) as e:
        engine.classify(np.zeros((9, 8, 8, 3), np.uint8))          # n > max_batch
    assert e.value.status == 1 and "invalid" in e.value.message
    with pytest.raises(EngineError):
        engine.classify(np.zeros((1, 0, 8, 3), np.uint8))
    with pytest.raises(EngineError):
        engine.classify(np.zeros((8, 8, 3), np.float32))


# ---- launch geometries beyond one tile per workgroup (classifier_cases.LAUNCHES) ----------------------------

def _launch(engine, name):
    n, h, w, _, want = cc.LAUNCHES[name]
    assert cc.classifier_grid(n, h, w) == want, name
    imgs, jp, ref = cc.launch_batch(name)           # (its input conditions are asserted on the oracle's sums in there)
    _check(engine, imgs, jp, ref)


@pytest.mark.parametrize("name", ["two_rounds_ragged", "benchmark", "second_pass_ragged", "parts_limit", "past_limit",
                                  "second_pass_loop_batch"])
def test_tile_loop_and_row_reduction_vs_oracle(engine, name):
    """The tile loop (prefetch across phases B and C, LDS planes reused), the last workgroup's row reduction beyond 128 rows and the
    `parts` buffer at its limit, each against the oracle: 14 sums, the bits of seven doubles, the label."""
    n, h, w, _, _ = cc.LAUNCHES[name]
    tx, ty, per, rounds, last = cc.classifier_grid(n, h, w)
    ragged = last < rounds                           # the last workgroups walk one tile fewer
    if name == "two_rounds_ragged":
        assert rounds == 2 and ragged and tx * ty == 768 // n + 3
    elif name == "benchmark":
        assert rounds == 3 and ragged and len(range(per - 2, tx * ty, per)) == 2 and len(range(per - 3, tx * ty, per)) == 3
    elif name == "second_pass_ragged":
        assert rounds == 1 and 128 < per < 256 and per % 16 == 3
    elif name == "parts_limit":
        assert rounds == 1 and per == cc.CLS_MAX_WG and tx == 2
    elif name == "past_limit":
        assert rounds == 2 and not ragged and tx * ty == cc.CLS_MAX_WG + 2 and per > 256
    else:
        assert rounds == 2 and n > 1 and 128 < per and n * per <= cc.CLS_MAX_WG
    _launch(engine, name)


@pytest.mark.parametrize("name,max_batch", [("batch32", 32), ("batch64", 64)])
def test_large_batch_engines_vs_oracle(name, max_batch):
    """Engines with max_batch 32 and 64 (at most 24 / 12 workgroups per image; 64 = the ticket array's extent): their own classifier
    in a looped, ragged launch of a whole batch."""
    from image_restoration_platform_amd.engine import Engine
    n, h, w, _, _ = cc.LAUNCHES[name]
    tx, ty, per, rounds, last = cc.classifier_grid(n, h, w)
    assert n == max_batch and per <= cc.CLS_MAX_WG // n < tx * ty and rounds >= 2 and last < rounds
    eng = Engine(device_index=0, max_batch=max_batch, num_streams=1)
    try:
        _launch(eng, name)
    finally:
        eng.close()


@pytest.mark.parametrize("w", [257, 258, 259, 260, 261, 511, 513, 515])
@pytest.mark.parametrize("h", [17, 33])
def test_tile_columns_with_a_ragged_last_column(engine, h, w):
    """More than one tile column: the word-wide load beside the bytewise replicate path of a group that straddles the right edge
    in a second (third) column, a left halo that is the neighbouring tile's pixels, the byte mask of a last group of 1, 2, 3 or 4
    pixels -- and two (three) tile rows, the last of one row."""
    tx, ty, per, rounds, _ = cc.classifier_grid(3, h, w)
    assert tx == -(-w // 256) >= 2 and w % 256 and ty == (h + 15) // 16 >= 2 and h % 16 == 1 and (per, rounds) == (tx * ty, 1)
    imgs = cc.mixed_batch(3, h, w, seed=h * 1000 + w, first=1)
    jp = np.array([1, 0, 1], np.uint8)
    _check(engine, imgs, jp, cc.oracle(("columns", h, w), imgs, jp))


def test_launches_in_sequence_on_one_engine(engine):
    """768 workgroups, then eight, then 8 x 50 looping ones, then 768 again on ONE engine: a row of `parts` left by an earlier
    launch must never be added, and every launch must find the tickets its predecessor reset."""
    for name in ("parts_limit", "one_tile_each", "two_rounds_ragged", "parts_limit"):
        _launch(engine, name)
