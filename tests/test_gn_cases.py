"""The inputs of tests/test_gn_fold_gpu.py can see what they are for -- shown on the CPU with oracle/layer_check.py alone: the sweep of P
holds every pass structure of gn_fold.hpp's reduction, and at every P of it a single partial that is dropped, read in another's place,
rotated among its groups or exchanged, and two images swapped, each put a coefficient outside the derived bound."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gn_cases as gc      # noqa: E402
from oracle import layer_check as lc      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_loop_bounds_are_those_of_the_kernel_source():
    csrc = os.path.join(ROOT, "image_restoration_platform_amd", "csrc")
    fold = open(os.path.join(csrc, "gn_fold.hpp")).read()
    assert "for (; t + 7 * ntl < a.gn_parts; t += 8 * ntl)" in fold and "for (; t < a.gn_parts; t += ntl)" in fold
    assert "tl = tid >> 3, ntl = nthr >> 3" in fold and "int t = act ? tl : a.gn_parts;" in fold
    assert "gn_fold(a, smem, blockIdx.x, blockIdx.x, 512)" in open(os.path.join(csrc, "gn.hip")).read()
    assert gc.NTL == 512 >> 3


def test_regimes_of_the_shapes_the_design_names():
    # (full passes, tail steps) per lane: 200 x 328, 1024^2 and 2048^2 at levels 0..3, 272 x 1000 at level 0
    assert [gc.regimes(p) for p in (143, 42, 12, 4)] == [((0, 0), (2, 3)), ((0, 0), (0, 1)), ((0, 0), (0, 1)), ((0, 0), (0, 1))]
    assert [gc.regimes(p) for p in (2048, 512, 128, 32)] == [((4, 4), (0, 0)), ((1, 1), (0, 0)), ((0, 0), (2, 2)), ((0, 0), (0, 1))]
    assert gc.regimes(8192) == ((16, 16), (0, 0)) and gc.regimes(131072) == ((256, 256), (0, 0))
    assert gc.regimes(544) == ((1, 1), (0, 1)) and sum(t for _, t in gc.lane_regimes(544)) == 32
    assert gc.regimes(448)[0] == (0, 0) and gc.lane_regimes(449)[0] == (1, 0) and gc.lane_regimes(449)[1] == (0, 7)
    for p in gc.SWEEP:                                 # every tile is read exactly once
        assert sum(8 * f + t for f, t in gc.lane_regimes(p)) == p


def test_sweep_holds_every_class():
    lanes = {p: gc.lane_regimes(p) for p in gc.SWEEP}
    for name, pred in gc.CLASSES.items():
        hits = [p for p in gc.SWEEP if pred(lanes[p])]
        print("GNCLASS %-52s P = %s" % (name, hits))
        assert hits, name
    for p in gc.SWEEP:
        assert any(pred(lanes[p]) for pred in gc.CLASSES.values()), p


def _engine_like(tot, mag, P, C):
    """The coefficients a correct float path gives for these sums: the float64 ones rounded to float."""
    g, b = gc.coded_gamma_beta(C)
    A, B, _, _ = lc.coeffs_from_sums(tot, mag, P, gc.hw_for(P, C), C, g, b)
    return np.stack([A, B], -1).astype(np.float32).astype(np.float64)


def _mutations(st, tot, rng):
    """(label, mutated sums): the defect applied to the exact sums `tot` of the coded partials (integers: the arithmetic is exact)."""
    nimg, P = st.shape[:2]
    tiles = sorted({0, P - 1} | {int(v) for v in rng.integers(0, P, 6)})
    at = lambda t: st[:, t].astype(np.float64)
    for t in tiles:
        yield "tile %d dropped" % t, tot - at(t)
        yield "tile %d: its groups rotated by one" % t, tot - at(t) + np.roll(at(t), 1, axis=1)
        yield "tile %d: sum and sumsq exchanged" % t, tot - at(t) + at(t)[:, :, ::-1]
        for t2 in sorted({t ^ 1, int(rng.integers(0, P)), (t + gc.NTL) % P, (t + 8 * gc.NTL) % P} - {t}):
            if t2 < P:
                yield "tile %d read in the place of tile %d" % (t2, t), tot - at(t) + at(t2)
    for i, j in sorted({(0, 1), (0, nimg - 1), (nimg - 2, nimg - 1)}):
        if 0 <= i < j < nimg:
            sw = tot.copy()
            sw[[i, j]] = tot[[j, i]]
            yield "images %d and %d swapped" % (i, j), sw


@pytest.mark.parametrize("P", gc.SWEEP)
def test_every_single_defect_leaves_the_bound(P):
    st = gc.coded_partials(P)
    tot, mag = lc.partial_sums(st)
    assert np.array_equal(mag, tot) and tot.max() < 2.0 ** 53
    for C in (32, 256):
        g, b = gc.coded_gamma_beta(C)
        ref = lc.coeffs_from_sums(tot, mag, P, gc.hw_for(P, C), C, g, b)
        assert lc.check_coeffs("intact", _engine_like(tot, mag, P, C), ref) == ""
        assert lc.coeff_share(_engine_like(tot, mag, P, C), ref) <= 0.5
        worst, n = (np.inf, ""), 0
        for label, mtot in _mutations(st, tot, np.random.default_rng(P)):
            ab = _engine_like(mtot, mag, P, C)
            share = lc.coeff_share(ab, ref)
            assert lc.check_coeffs(label, ab, ref) != "" and share > 1.0, "P %d C %d: %s stays inside the bound (share %.3g)" % (P, C, label, share)
            worst, n = min(worst, (share, label)), n + 1
        print("GNMUTATION P %6d C %3d | %3d defects, all caught | smallest shift / bound %.3g (%s) | regimes %s" % ((P, C, n) + worst + (gc.regimes(P),)))
        assert n >= (3 if P == 1 else 8)


def test_defects_applied_to_the_partials_themselves():
    """The literal form of what _mutations does to the sums: through coeffs_from_partials on a changed copy of the array."""
    P, C = 513, 32
    st = gc.coded_partials(P)
    g, b = gc.coded_gamma_beta(C)
    ref = lc.coeffs_from_partials(st, gc.hw_for(P, C), C, g, b)
    muts = {}
    for name, f in (("drop", lambda m: m.__setitem__((slice(None), 512), 0.0)), ("twice", lambda m: m.__setitem__((slice(None), 511), m[:, 510].copy())),
                    ("rotate", lambda m: m.__setitem__((slice(None), 0), np.roll(m[:, 0], 1, axis=1))), ("swap", lambda m: m.__setitem__(([0, 1],), m[[1, 0]].copy())),
                    ("exchange", lambda m: m.__setitem__((slice(None), 300), m[:, 300, :, ::-1].copy()))):
        m = np.array(st)
        f(m)
        assert not np.array_equal(m, st), name
        A, B, _, _ = lc.coeffs_from_partials(m, gc.hw_for(P, C), C, g, b)
        muts[name] = lc.check_coeffs(name, np.stack([A, B], -1).astype(np.float32).astype(np.float64), ref)
        assert muts[name], name
    assert "image" in muts["drop"] and "channel" in muts["drop"] and "group" in muts["drop"]


def test_run_coeffs_on_the_emulating_oracle():
    """NetworkCheck.run_coeffs (chunked float32 -> float64 moments) judges every GroupNorm as NetworkCheck.coeffs does from the whole
    float64 tensor, passes on the intact oracle's capture, and reports a captured coefficient that is off by a thousandth."""
    import torch
    from image_restoration_platform_amd import synth, weights
    from oracle import classifier as oc
    from oracle import restorenet as onet
    w, imgs = weights.generate(0), synth.batch(2, 72, 136)
    sc = np.stack([oc.classify(im, True)[0] for im in imgs])
    cap = {}
    with torch.no_grad():
        out = onet._Net(w, True, cap, False).forward(imgs, sc.reshape(2, 7))
    nc = lc.NetworkCheck(w, imgs, sc, cap.__getitem__, out, up_mode="plain")
    names = lc.gn_layer_names("plain")
    assert len(names) == 33 and names[-1] == "pixels" and set(names) == {n for n in lc.layer_names("plain") if (n + ".ab") in cap} | {"pixels"}
    nc.chunk = 5000                                         # several chunks per image at every level but the last
    msgs = nc.run_coeffs()
    assert list(msgs) == names and not any(msgs.values()), msgs
    for nm in ("enc0.rb0.h", "dec1.rb1", "pixels"):          # the same moments as the whole-tensor path, to the last bits
        level, src = lc._level(nm), lc.layer_inputs(nm)[0]
        mean, mabs, msq, c = nc._chunked_moments(src, level, chunk=5000)
        for got, want in zip((mean, mabs, msq), lc._gn_moments(nc.get(src))):
            assert np.allclose(got, want, rtol=1e-13, atol=0)
    key = "mid.rb0.h.ab"
    good = cap[key]
    try:
        bad = np.array(good, dtype=np.float32, copy=True).reshape(-1)
        bad[2 * 77] *= np.float32(1.001)
        cap[key] = bad
        msgs = nc.run_coeffs()
    finally:
        cap[key] = good
    assert [nm for nm, m in msgs.items() if m] == ["mid.rb0.h"] and "channel 77" in msgs["mid.rb0.h"]


def test_float_cases_are_what_they_claim():
    cases = {c["name"]: c for c in gc.float_cases()}
    assert len(cases) == 8
    for c in cases.values():
        ref = gc.case_reference(lc, c)
        assert all(np.isfinite(v).all() for v in ref), c["name"]
        ab = np.stack(ref[:2], -1).astype(np.float32).astype(np.float64)
        assert lc.check_coeffs(c["name"], ab, ref) == "", c["name"]            # the reference rounded to float lies inside its own bound
        assert c["film"] is None or c["film_off"] + 2 * c["C"] <= c["film"].shape[1]

    def var(c):
        tot, _ = lc.partial_sums(c["stats"], exact=True)
        cnt = c["hw"] * (c["C"] // 8)
        return tot[:, :, 1] / cnt - (tot[:, :, 0] / cnt) ** 2

    mixed = cases["mixed sign and magnitude"]["stats"]
    assert (mixed[..., 0] < 0).any() and (mixed[..., 0] > 0).any() and np.abs(mixed).min() < 2e-3 and np.abs(mixed).max() > 5e3
    assert (var(cases["mixed sign and magnitude"]) > 0).all()
    assert (var(cases["variance exactly 0"]) == 0).all()
    A = gc.case_reference(lc, cases["variance exactly 0"])[0]
    f = cases["variance exactly 0"]
    assert np.allclose(A, f["gamma"] * (1.0 + f["film"][:, :128].astype(np.float64)) / np.sqrt(1e-5), rtol=1e-12)
    v = var(cases["variance slightly negative"])
    assert (v <= 0).all() and (v < 0).sum() >= 2 * 7 and v.min() > -1e-5
    c = cases["hw G not a power of two"]
    n = c["hw"] * (c["C"] // 8)
    assert n & (n - 1) and n % c["stats"].shape[1]
    g = cases["gamma of both signs with zeros"]["gamma"]
    assert (g == 0).sum() >= 50 and (g > 0).any() and (g < 0).any()
    s = cases["FiLM scale at -1 and below"]["film"][:, :64]
    assert (s == -1).any() and (s < -1).any() and (s > -1).any()
    w = cases["film window off 13 in rows of 2 C + 37"]
    assert w["film_off"] == 13 and w["film"].shape[1] == 2 * 32 + 37
    assert cases["no film"]["film"] is None
    many = gc.many_images_case()
    assert many["stats"].shape[0] == 64 and len({m.tobytes() for m in many["stats"]}) == 64
