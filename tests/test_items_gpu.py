"""Workgroups that walk several items, layer by layer against a reference -- and conv_pk / conv_w4's 128-cout items, which no shape of
tests/test_layers_gpu.py reaches (there plan_conv gives every C >= 128 ResBlock conv the 64-cout items of conv_w4).

At the device's own grid of 256 workgroups a shape small enough for a float64 reference leaves a workgroup 0 to 2 items; the hand-over from
one item's epilogue to the next item's first stage, the (t + 1) & 1 buffers across an item boundary and the per-item offset caches run in
earnest only with IRE_GRID_CUS, which the library reads once per process.  So every case below runs in three fresh child processes, with
grids of 8 workgroups (one per XCD group, stride 1), 16 (two per group, stride 2) and the device's own, each on two shapes:

  (3, 136, 136)  level 2: 34 x 34 in 2 x 3 tiles; level 3: 17 x 17 in 1 x 2 tiles of 2 n-blocks
  (3, 72, 264)   level 2: 18 x 66 in 3 x 2 tiles, the last column 2 pixels wide; level 3: 9 x 33 in 2 x 1 tiles, the last column 1 pixel wide

tests/test_conv_plan.py asserts on the CPU, from plan_conv and the work cursor, the kernel, slab and tile grid of every launch of every case,
that at grids of 8 and 16 every persistent launch has a workgroup with several items, and that conv_pk, conv_w4 and conv_f8 step to the next
n-block, tile column, tile row and image.

What is asserted: (1) the teacher-forced per-layer check (oracle/layer_check.py, its derived bound) on what the grid-8 child captured; (2) every
captured tensor, every (A, B) and the pixels bit-equal between the three grids, so the grids share that one float64 evaluation; (3) the
engine's profile report names the kernel each case exists for; (4) a run without debug capture gives the same pixels.

The children run one after another; when one exits non-zero, by a signal or at its time limit, no further child starts and every test that
needs it or a later one fails with its stderr.  Nothing is retried."""
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_layers_gpu import SWITCHES, _group                       # noqa: E402
from test_strips_layers_gpu import GROUPS_RB, _ab_name, _switched_kernels      # noqa: E402

from image_restoration_platform_amd import synth                  # noqa: E402
from oracle import layer_check as lc                              # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(3, 136, 136), (3, 72, 264)]
GRIDS = ["8", "device", "16"]                 # the order the children run in (IRE_GRID_CUS; "device": unset)
CHILD_TIMEOUT = {"8": 900, "device": 300, "16": 300}
DEEP_NAMES = [nm for nm in lc.layer_names() if ".rb" in nm and lc._level(nm) >= 2]          # the C >= 128 ResBlock convolutions
DEEP = GROUPS_RB((2, 3))


def _sw_id(env):
    return ",".join("%s=%s" % kv for kv in env.items())


def _up_mode(env):
    return "plain" if env.get("IRE_UP_SUBPIX") == "0" else "subpix" if env.get("IRE_UP_FUSE") == "0" else "fused"


def _default_kernels(deep):
    exp = dict.fromkeys(DEEP, deep)
    exp.update(dict.fromkeys(GROUPS_RB((0, 1)) + ["head"], "conv_pc"), stem="conv_stem", down0="conv_down", down1="conv_dnq", down2="conv_dnq",
               up2="conv_upq", up1="conv_up", up0="conv_up")
    return exp


# id -> switches, precision, the layers the teacher-forced check gets (None: the case is held by equal bytes alone), the kernels it exists for
CASES = {
    "default": dict(env={}, precision="bf16", names="all", kernels=_default_kernels("conv_w4")),
    "IRE_W4_SPLIT=0": dict(env={"IRE_W4_SPLIT": "0"}, precision="bf16", names="deep", kernels=_default_kernels("conv_pk")),
    "IRE_W4_SPLIT=0,IRE_PK=0": dict(env={"IRE_W4_SPLIT": "0", "IRE_PK": "0"}, precision="bf16", names="deep", kernels=_default_kernels("conv_w4")),
    "IRE_W4_SPLIT=0,IRE_PK=1": dict(env={"IRE_W4_SPLIT": "0", "IRE_PK": "1"}, precision="bf16", names="deep",
                                   kernels=dict(_default_kernels("conv_pk"), **{g: "conv_w4" for g in DEEP if g.endswith("rb2")})),
    "fp8,IRE_FP8_MX=1": dict(env={"IRE_FP8_MX": "1"}, precision="fp8", names="deep", kernels=_default_kernels("conv_f8")),
    "fp8,IRE_FP8_MX=0": dict(env={"IRE_FP8_MX": "0"}, precision="fp8", names="deep", kernels=_default_kernels("conv_w4")),
}
for _env in SWITCHES:
    CASES["switch " + _sw_id(_env)] = dict(env=_env, precision="bf16", names=None, kernels=_switched_kernels(_env))
CHECKED = [c for c, d in CASES.items() if d["names"]]


def _shape_id(s):
    return "%dx%dx%d" % s


def _images(shape):
    return synth.batch(*shape, start=21)


# ---- the child: python tests/test_items_gpu.py OUT.json CHECK(0|1) -------------------------------------------------------------------------
def _digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _child_case(case, shape, imgs, sc, w, eng, check):
    d = CASES[case]
    up_mode = _up_mode(d["env"])
    rec = {}
    t0 = time.perf_counter()
    eng.debug_capture(True)
    try:
        eng.profile_reset()
        eng.profile_enable(1)
        try:
            out = eng.restore(imgs, scores=sc)
            rec["report"] = {r["group"]: r["kernel"] for r in eng.profile_report()}
        finally:
            eng.profile_enable(0)
        digests = []                                                  # program order: the first name that differs is where two runs part
        for nm in lc.layer_names(up_mode):
            if _ab_name(nm):
                digests.append((_ab_name(nm), _digest(eng.activation(_ab_name(nm)))))
            digests.append((nm, _digest(out if nm == "pixels" else eng.activation(nm))))
        rec["digests"] = digests
        rec["t_gpu"] = time.perf_counter() - t0
        if check and d["names"]:
            names = None if d["names"] == "all" else DEEP_NAMES
            label = "%s %s grid 8" % (case, _shape_id(shape))
            t1 = time.perf_counter()
            try:
                reports = lc.assert_network(w, imgs, sc, eng.activation, out, fp8=d["precision"] == "fp8", up_mode=up_mode, names=names, label=label)
                groups = {}
                for nm, r in reports.items():
                    g = groups.setdefault(_group(nm), [0.0, 0.0, 0.0])
                    g[0], g[1], g[2] = max(g[0], r.headroom), max(g[1], r.median_ulps), max(g[2], r.uncertain)
                rec["check"] = {"message": None, "names": sorted(reports), "lines": [
                    "LAYERCHECK %s | %s | share of the accumulation budget used %.3f | median bound %.2f ulp | uncertain %.1e" % (label, g, hr, med, unc)
                    for g, (hr, med, unc) in sorted(groups.items())]}
            except AssertionError as e:
                rec["check"] = {"message": str(e), "names": [], "lines": []}
            rec["t_ref"] = time.perf_counter() - t1
    finally:
        eng.debug_capture(False)
    t2 = time.perf_counter()
    again = eng.restore(imgs, scores=sc)                              # capture synchronises after every convolution; an ordinary run does not
    rec["t_gpu"] += time.perf_counter() - t2
    rec["nocapture_equal"] = bool(np.array_equal(again, out))
    rec["mean_change"] = float(np.abs(out.astype(np.int32) - imgs.astype(np.int32)).mean())
    return rec


def _child(path, check):
    from image_restoration_platform_amd import weights
    from image_restoration_platform_amd.engine import Engine
    from oracle import classifier as oc
    w = weights.generate(0)
    batches = [(s, _images(s)) for s in SHAPES]
    batches = [(s, im, np.stack([oc.classify(i, True)[0] for i in im])) for s, im in batches]
    switch_vars = sorted({k for d in CASES.values() for k in d["env"]})
    result = {}
    for case, d in CASES.items():
        for k in switch_vars:
            os.environ.pop(k, None)
        os.environ.update(d["env"])
        eng = Engine(device_index=0, max_batch=8, num_streams=1, precision=d["precision"])      # the switches are read once per engine
        try:
            result[case] = {_shape_id(s): _child_case(case, s, im, sc, w, eng, check) for s, im, sc in batches}
        finally:
            eng.close()
    with open(path, "w") as f:
        json.dump(result, f)


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2] == "1")
    sys.exit(0)


# ---- the parent ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """grid -> the child's result, or a string: why there is none."""
    tmp = tmp_path_factory.mktemp("items")
    out, failed = {}, None
    for grid in GRIDS:
        if failed:
            out[grid] = "the child of grid %s was not started: %s" % (grid, failed)
            continue
        env = dict(os.environ)
        env.pop("IRE_GRID_CUS", None)
        if grid != "device":
            env["IRE_GRID_CUS"] = grid
        env["PYTHONPATH"] = ROOT + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
        path = str(tmp / ("grid_%s.json" % grid))
        t0 = time.perf_counter()
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), path, "1" if grid == "8" else "0"], env=env, cwd=ROOT,
                               capture_output=True, text=True, timeout=CHILD_TIMEOUT[grid])
            if r.returncode != 0:
                failed = "the child of grid %s exited with %d:\n%s\n%s" % (grid, r.returncode, r.stdout[-1000:], r.stderr[-3000:])
        except subprocess.TimeoutExpired as e:
            failed = "the child of grid %s was ended at its time limit of %d s:\n%s" % (grid, CHILD_TIMEOUT[grid], str(e.stderr or "")[-3000:])
        if failed:
            out[grid] = failed
            continue
        with open(path) as f:
            out[grid] = json.load(f)
        recs = [rec for c in out[grid].values() for rec in c.values()]
        print("ITEMSTIME grid %s | child %.1f s | restore, capture and digests %.1f s | float64 references %.1f s" % (
            grid, time.perf_counter() - t0, sum(r["t_gpu"] for r in recs), sum(r.get("t_ref", 0.0) for r in recs)))
    return out


def _need(runs, grid):
    if isinstance(runs[grid], str):
        pytest.fail(runs[grid], pytrace=False)
    return runs[grid]


@pytest.mark.parametrize("shape", SHAPES, ids=_shape_id)
@pytest.mark.parametrize("case", CHECKED)
def test_every_element_within_the_derived_bound_with_several_items_per_workgroup(runs, case, shape):
    """Grid 8: `default` gets every layer; the 128-cout item cases and the fp8 engine the sixteen C >= 128 ResBlock convolutions."""
    rec = _need(runs, "8")[case][_shape_id(shape)]
    chk = rec["check"]
    for ln in chk["lines"]:                                               # information (pytest -s), not a threshold
        print(ln)
    print("ITEMSTIME %s %s grid 8 | float64 references %.1f s" % (case, _shape_id(shape), rec["t_ref"]))
    assert chk["message"] is None, chk["message"]
    want = lc.layer_names() if CASES[case]["names"] == "all" else DEEP_NAMES
    assert len(want) == (40 if CASES[case]["names"] == "all" else 16)
    assert set(chk["names"]) == set(want)                                 # no layer of the named set exempt


@pytest.mark.parametrize("case", list(CASES))
def test_every_captured_tensor_has_equal_bytes_at_every_grid(runs, case):
    base = _need(runs, "8")[case]
    for other in ("device", "16"):
        alt = _need(runs, other)[case]
        for shape in map(_shape_id, SHAPES):
            a, b = base[shape]["digests"], alt[shape]["digests"]
            assert [n for n, _ in a] == [n for n, _ in b] and len(a) == len(lc.layer_names(_up_mode(CASES[case]["env"]))) + 33
            diff = [n for (n, x), (_, y) in zip(a, b) if x != y]
            assert not diff, "%s %s: grid 8 and grid %s part at %s (first in program order; %d of %d entries differ: %s)" % (
                case, shape, other, diff[0], len(diff), len(a), " ".join(diff))


@pytest.mark.parametrize("case", list(CASES))
def test_the_kernels_the_case_exists_for_ran(runs, case):
    for grid in GRIDS:
        for shape in map(_shape_id, SHAPES):
            rec = _need(runs, grid)[case][shape]
            for group, kernel in CASES[case]["kernels"].items():
                assert rec["report"].get(group) == kernel, "%s %s grid %s: layer group %s ran on %r, the case exists for %r (report: %r)" % (
                    case, shape, grid, group, rec["report"].get(group), kernel, rec["report"])
            assert rec["mean_change"] > 1.0, (case, shape, grid)          # the network did something


@pytest.mark.parametrize("case", list(CASES))
def test_debug_capture_changes_no_pixel(runs, case):
    for grid in GRIDS:
        for shape in map(_shape_id, SHAPES):
            assert _need(runs, grid)[case][shape]["nocapture_equal"], "%s %s grid %s: the pixels of a run with debug capture differ from an ordinary run's" % (case, shape, grid)
