"""The launch rule book (csrc/conv_plan.hpp) on the CPU box: tests/native/conv_plan_dump.cpp (test infrastructure; libire.so includes
the same header) walks the network's convolutions in schedule order and prints every field of every launch plan, per case and layer
group.  The expected lines (tests/golden/conv_plan_9e80c0a.txt) are a recording of commit 9e80c0a, not of the code under test: that
commit's Engine::build_program and Engine::exec_conv text, and its conv_pc_fits / conv_pk_fits loops, were compiled unchanged into a
scratch harness in which every conv_*_launch, prof_begin / prof_tag and the GroupNorm bookkeeping is a stub that prints what it
received, the ConvW pointers are named sentinels wherever that commit's packer produces the array, a GroupNorm is always pending (so
that the launch shows whether the kernel folds it) and 256 CUs stand for the device.  Four locals no stub sees (tile height,
parts_mul, stats level, ty0) were printed by two lines added to the lifted text.  The recording is kept as it came out.

Cases: default switches on twelve shapes (both sides of the 64-cout split at 512^2 and of both coefficient tables), every switch set
of tests/test_layers_gpu.py and tests/test_restore_gpu.py plus IRE_PK=1 on two shapes, the fp8 engine with IRE_FP8_MX 1 and 0 on
three, (64, 512, 512) for the launch conv_pk's table refuses, and first / middle / last row strips of three strip plans.  The comment-only invariants of the old exec_conv are asserted
separately below, over a wider list (`props`).  A third list (`fp8`) is an fp8 engine under IRE_FP8_MX x IRE_W4 x IRE_PK: the table of
which kernel, slab and bias its C >= 128 ResBlock convolutions really get is asserted at the end.  A fifth list (`items`) is every case
of tests/test_items_gpu.py at its two shapes: kernel, slab, n-blocks and tile grid of every group are asserted against a table written
out here, and the work cursor (tests/test_persist_walk.py's decode) shows that at grids of 8 and 16 workgroups every persistent launch
gives some workgroup several items and that conv_pk, conv_w4 and conv_f8 see every kind of step from one item to the next."""
import glob
import os
import re
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_persist_walk import decode      # noqa: E402    (held equal to csrc/persist.hpp's cursor by that file)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "conv_plan_dump.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden")
SAN_MARKS = ("ERROR: AddressSanitizer", "runtime error", "LeakSanitizer")
CUS = 256                                   # what the dump plans for (MI355X)
COEF_IMGS = {"PK": 4, "PC": None, "PC_HEAD": 64}       # conv_pk.hip PK_IMGS; conv_pc.hip: 64 images at C = 32, 8 at C = 64


def _build(tmp, name, flags):
    exe = str(tmp / name)
    r = subprocess.run(["g++", "-std=c++17", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall"] + flags + [SRC, "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0 and "warning" not in r.stderr, r.stderr[-3000:]
    return exe


def _run(exe, mode):
    r = subprocess.run([exe, mode], capture_output=True, text=True, timeout=600)
    log = r.stdout[-2000:] + r.stderr[-4000:]
    assert r.returncode == 0 and not r.stderr and not any(m in log for m in SAN_MARKS), log
    return r.stdout


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("conv_plan")
    exe, exe_asan = _build(tmp, "cp", ["-O2"]), _build(tmp, "cp_asan", ["-O1", "-fsanitize=address,undefined"])
    return {"fixture": _run(exe, "fixture"), "fixture_asan": _run(exe_asan, "fixture"), "props": _run(exe, "props"), "fp8": _run(exe, "fp8"), "strips": _run(exe, "strips"),
            "items": _run(exe, "items"), "large": _run(exe, "large"), "large_asan": _run(exe_asan, "large"), "rule": _run(exe_asan, "rule")}


FIXTURE = os.path.join(GOLDEN, "conv_plan_9e80c0a.txt")
SCHEDULE = ["stem", "L0.rb1", "L0.rb2", "down0", "L1.rb1", "L1.rb2", "down1", "L2.rb1", "L2.rb2", "down2", "L3.rb1", "L3.rb2",
            "up2", "fuse2", "up1", "fuse1", "up0", "fuse0", "head"]       # the order in which a case's groups first launch


def golden_lines():
    """Every recorded line as the dump prints it, header first.  The file holds a case whole (`case NAME`, then its lines) or as what
    differs from an earlier, whole case (`case NAME like BASE`: the lines that differ, with `.` for a value that is the base's; new
    groups whole; `-GROUP` for a group the case lacks)."""
    text = open(FIXTURE).read().splitlines()
    cases = {}
    for ln in text[1:]:
        if ln.startswith("case "):
            w = ln.split(" ")
            assert len(w) in (2, 4) and w[1] not in cases and (len(w) == 2 or (w[2] == "like" and " like " not in cases[w[3]][0])), ln
            cur = cases[w[1]] = (ln, dict(cases[w[3]][1]) if len(w) == 4 else {})
        elif ln.startswith("-"):
            del cur[1][ln[1:]]
        else:
            g, rest = ln.split(" ", 1)
            assert len(w) == 4 or g not in cur[1], ln
            if "." in rest.split(" "):
                rest = " ".join(b if v == "." else v for v, b in zip(rest.split(" "), cur[1][g].split(" ")))
            cur[1][g] = rest
    out = [text[0]]
    for name, (_, groups) in cases.items():
        assert set(groups) <= set(SCHEDULE), name
        out += ["%s %s %s" % (name, g, groups[g]) for g in SCHEDULE if g in groups]
    return out


def parse(line, fields=open(FIXTURE).readline().split()[3:]):
    case, group, rest = line.split(" ", 2)
    values = rest.split(" ")
    assert len(values) == len(fields), line
    return case, group, dict(zip(fields, values))


def test_every_plan_equals_the_recorded_parent(dumps):
    want = golden_lines()
    assert glob.glob(os.path.join(GOLDEN, "conv_plan_*.txt")) == [FIXTURE]
    assert want[0].startswith("# case group kernel ") and len(want[0].split()) == 3 + 33
    got = dumps["fixture"].splitlines()
    assert got[0] == want[0]
    want, got = want[1:], got[1:]
    assert (len({ln.split(" ", 1)[0] for ln in want}), len(want)) == (63, 1028)          # the fixture is the whole recording
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w
    assert dumps["fixture_asan"] == dumps["fixture"]                                   # under ASan + UBSan: the same lines, no report
    # no two ops of one group plan differently: one line per (case, group)
    keys = [tuple(ln.split(" ", 2)[:2]) for ln in want]
    assert len(set(keys)) == len(keys)
    # the hand-checkable case: at 512^2 level 2 has 8 x 4 tiles x 1 block x 8 = 256 (not < 256: 128-cout items), level 3 has
    # 4 x 2 x 2 x 8 = 128 (< 256: the 64-cout split)
    by = {tuple(ln.split(" ", 2)[:2]): parse(ln)[2] for ln in want}
    assert (by["default:bf16:1x512x512", "L2.rb1"]["w"], by["default:bf16:1x512x512", "L2.rb1"]["kernel"]) == ("w4", "PK")
    assert (by["default:bf16:1x512x512", "L3.rb1"]["w"], by["default:bf16:1x512x512", "L3.rb1"]["w4_nt"]) == ("w4h", "64")
    # both answers of coef_table_fits for conv_pk's table of 4 images: 128-cout items at 512^2 level 2 are 32 per image, an XCD range of a
    # batch of 8 spans one image, of a batch of 64 eight.  (In the recorded parent no launch of the issue's twelve shapes is refused: 5 and
    # 8 images of 1024^2 span 2 and 1 images per range, and small images take the 64-cout items; conv_pc's tables of 64 / 8 images hold
    # every batch up to the engine's limit of 64 images, (12, 32, 48) and (64, 64, 64) included.)
    assert by["default:bf16:8x512x512", "L2.rb1"]["kernel"] == "PK"
    l2 = by["default:bf16:64x512x512", "L2.rb1"]
    assert (l2["kernel"], l2["w"], l2["w4_nt"]) == ("W4", "w4", "0")
    assert by["default:bf16:5x1024x1024", "L3.rb1"]["kernel"] == "PK" and by["default:bf16:8x1024x1024", "L3.rb1"]["kernel"] == "PK"
    assert by["default:bf16:12x32x48", "L1.rb1"]["kernel"] == "PC" and by["default:bf16:64x64x64", "L1.rb1"]["kernel"] == "PC"


def _case(name):
    """(switch set, precision, n, h, w, strip, nstrips) of a case name"""
    env, prec, rest = name.split(":", 2)
    m = re.fullmatch(r"strip(\d+)of(\d+):(\d+)x(\d+)", rest)
    if m:
        s, ns, h, w = map(int, m.groups())
        return env, prec, 1, h, w, s, ns
    n, h, w = map(int, rest.split("x"))
    return env, prec, n, h, w, None, 0


def _fits(cap, items_per_img, nimg):
    """the kernels' rule, restated: the workgroups of XCD group x walk items [items x / X, items (x + 1) / X); none may span more than cap images"""
    items = items_per_img * nimg
    X = min(min(items, CUS), 8)
    return all((hi - 1) // items_per_img - lo // items_per_img + 1 <= cap
               for lo, hi in ((items * x // X, items * (x + 1) // X) for x in range(X)) if hi > lo)


def test_the_comment_only_invariants(dumps):
    lines = [parse(ln) for ln in dumps["props"].splitlines()[1:]]
    cases = {c for c, _, _ in lines}
    assert (len(cases), len(lines)) == (9 * 8 + 1 + 2 + 8 + 4, 87 * 16)
    plans = {}
    for c, g, f in lines + [parse(ln) for ln in dumps["fixture"].splitlines()[1:]]:
        plans.setdefault(_case(c), {})[g] = f
    checked = {"split": 0, "fits": 0, "strips": 0}
    for (env, prec, n, h, w, s, ns), groups in plans.items():
        for g, f in groups.items():
            # 1. 64- or 128-cout items (and the slabs that go with them): a function of the image's shape alone -- the same for every
            #    batch size, and for a strip the same as for its whole image
            if env == "default" and prec == "bf16" and (1, h, w, None, 0) in [k[2:] for k in plans if k[:2] == (env, prec)]:
                one = plans[env, prec, 1, h, w, None, 0][g]
                if s is not None or n <= 8:
                    assert (f["w4_nt"], f["w"] in ("w4", "w4h") and f["w"]) == (one["w4_nt"], one["w"] in ("w4", "w4h") and one["w"]), (env, n, h, w, s, g)
                    checked["split"] += 1
            # 2. conv_pk / conv_pc get only what their coefficient table holds
            if f["kernel"] in COEF_IMGS:
                cap = COEF_IMGS[f["kernel"]] or (64 if f["cout"] == "32" else 8)
                assert _fits(cap, int(f["tiles_x"]) * int(f["tiles_y"]) * int(f["nblocks"]), n), (env, n, h, w, g)
                checked["fits"] += 1
            # 3. a strip's tiles land at their global tile offset, and the finalize is told the whole image's count
            if s is not None and f["stats_level"] != "-1":
                whole = plans[env, prec, 1, h, w, None, 0][g]
                y0 = s * (h // ns)
                assert int(f["ty0"]) == (y0 >> int(f["stats_level"])) // int(f["tile_h"])
                assert int(f["stats_off"]) == int(f["ty0"]) * int(f["tiles_x"]) * 16 * int(f["parts_mul"])
                assert (f["stat_parts"], f["tile_h"], f["tiles_x"], f["parts_mul"]) == (whole["stat_parts"], whole["tile_h"], whole["tiles_x"], whole["parts_mul"])
                assert int(f["tiles_y"]) * ns == int(whole["tiles_y"])
                checked["strips"] += 1
    assert min(checked.values()) > 100, checked


def test_which_kernel_an_fp8_engine_really_runs(dumps):
    """The C >= 128 ResBlock convolutions of an fp8 engine (precision="fp8") under IRE_FP8_MX x IRE_W4 x IRE_PK, read off plan_conv:

      IRE_W4=1 (default)  IRE_FP8_MX=1 (default)  conv_f8.hip, slab w8x, bias8, fp8 = 1
                          IRE_FP8_MX=0            conv_w4.hip on e4m3 operands, slab w8, bias8, fp8 = 1; 128-cout items only
      IRE_W4=0            either                  conv_rb.hip on the bf16 slab wp with the float bias, fp8 = 0

    IRE_PK changes nothing: conv_pk.hip takes no fp8 launch.  IRE_W4=0 makes an fp8 engine run a bf16 kernel SILENTLY -- the rule book
    tests use_w4 before it looks at the precision -- so a per-layer check with fp8=True of such an engine would judge bf16 arithmetic by the
    fp8 rules: that combination is kept out of the fp8 cases of tests/test_layers_gpu.py, and stated in DESIGN.md.  Everything else
    of the network plans exactly as for a bf16 engine (fp8 = 0)."""
    lines = [parse(ln) for ln in dumps["fp8"].splitlines()[1:]]
    deep = ("L2.rb1", "L2.rb2", "L3.rb1", "L3.rb2")
    want = {("1", "1"): ("F8", "conv_f8", "1", "w8x", "bias8"), ("0", "1"): ("W4", "conv_w4", "1", "w8", "bias8"),
            ("1", "0"): ("RB", "conv_rb", "0", "wp", "bias"), ("0", "0"): ("RB", "conv_rb", "0", "wp", "bias")}
    bf16 = {}
    for c, g, f in (parse(ln) for ln in dumps["fixture"].splitlines()[1:]):
        bf16[c, g] = f
    seen = set()
    for c, g, f in lines:
        envs, prec, n, h, w, s, _ = _case(c)
        env = dict(kv.split("=") for kv in envs.split(","))
        assert prec == "fp8" and s is None and set(env) == {"IRE_FP8_MX", "IRE_W4", "IRE_PK"}
        if g in deep:
            assert (f["kernel"], f["kname"], f["fp8"], f["w"], f["bias"]) == want[env["IRE_FP8_MX"], env["IRE_W4"]], (c, g)
            assert f["w4_nt"] == "0" and f["fused_act"] == "1" and f["w1"] == "none"
            assert f["nkc"] == str(int(f["cout"]) // {"F8": 32, "W4": 16, "RB": 32}[f["kernel"]]), (c, g, f["nkc"])
            seen.add((env["IRE_FP8_MX"], env["IRE_W4"], env["IRE_PK"], n, h, w, g))
        else:
            assert f["fp8"] == "0" and f["bias"] != "bias8" and f["w"] not in ("w8x", "w8"), (c, g)
            # the bf16 engine's plan of the same launch, where the recording has the shape under default switches
            same = bf16.get(("default:bf16:%dx%dx%d" % (n, h, w), g))
            if same and (env["IRE_W4"], env["IRE_PK"]) == ("1", "2"):
                assert f == same, (c, g)
    assert len(seen) == 2 * 2 * 2 * 4 * len(deep)                        # every combination, every shape, all four groups
    # IRE_PK is no input of an fp8 engine's plan: the two halves of the table are equal line by line
    by = {(c, g): f for c, g, f in lines}
    for (c, g), f in by.items():
        if "IRE_PK=2" in c and g in deep:
            assert by[c.replace("IRE_PK=2", "IRE_PK=0"), g] == f, (c, g)


def test_the_strip_layer_test_shapes_get_the_kernels_and_items_their_cases_name(dumps):
    """tests/test_strips_layers_gpu.py names a kernel family per shape and reads the kernel off the profile report, which does not carry
    the item width of conv_w4; here the same strips are planned by plan_conv itself: 384x264 in 3 takes the 64-cout items at both deep
    levels, 1024x264 in 8 conv_pk (IRE_PK=0: conv_w4's 128-cout items), an fp8 engine conv_f8 or conv_w4's fp8 form, in every strip."""
    deep = ("L2.rb1", "L2.rb2", "L3.rb1", "L3.rb2")
    want = {("default", "bf16", 384): ("W4", "conv_w4", "w4h", "64", "0"), ("default", "bf16", 1024): ("PK", "conv_pk", "w4", "0", "0"),
            ("default", "bf16", 256): ("W4", "conv_w4", "w4h", "64", "0"), ("default", "bf16", 512): ("W4", "conv_w4", "w4h", "64", "0"),
            ("IRE_PK=0", "bf16", 1024): ("W4", "conv_w4", "w4", "0", "0"),
            ("IRE_FP8_MX=1", "fp8", 384): ("F8", "conv_f8", "w8x", "0", "1"), ("IRE_FP8_MX=1", "fp8", 1024): ("F8", "conv_f8", "w8x", "0", "1"),
            ("IRE_FP8_MX=0", "fp8", 384): ("W4", "conv_w4", "w8", "0", "1"), ("IRE_FP8_MX=0", "fp8", 1024): ("W4", "conv_w4", "w8", "0", "1")}
    seen = set()
    for c, g, f in (parse(ln) for ln in dumps["strips"].splitlines()[1:]):
        env, prec, n, h, w, s, ns = _case(c)
        assert s is not None and (f["iy_lo"], f["in_row_off"]) == ("-1" if s else "0", "1"), (c, g)
        if g in deep:
            assert (f["kernel"], f["kname"], f["w"], f["w4_nt"], f["fp8"]) == want[env, prec, h], (c, g)
            if f["w4_nt"] == "0":
                assert f["nblocks"] == str(int(f["cout"]) // 128), (c, g)
            seen.add((env, prec, h, s, g))
        # ragged beside the boundary: the last tile column of these widths is partial at every level
        if g.startswith("L"):
            assert (w >> int(g[1])) % 32 != 0 and int(f["tiles_x"]) == -(-(w >> int(g[1])) // 32), (c, g)
    assert len(seen) == (3 + 3 + 2 + 3 + 3 + 4 * 3) * len(deep), len(seen)      # (256x72 in 2 has two strips)


# ---- tests/test_items_gpu.py: its cases at its two shapes ---------------------------------------------------------------------------------
ITEM_SHAPES = [(3, 136, 136), (3, 72, 264)]
ITEM_ENVS = ["default", "IRE_W4_SPLIT=0", "IRE_W4_SPLIT=0,IRE_PK=0", "IRE_W4_SPLIT=0,IRE_PK=1", "IRE_PK=0", "IRE_PC=0", "IRE_PC=1", "IRE_W4=0",
             "IRE_UPQ=0", "IRE_DNQ=0", "IRE_UP_FUSE=0", "IRE_UP_SUBPIX=0", "IRE_GN_FOLD=0", "IRE_DOWN_RB=0,IRE_HEAD_RB=0", "IRE_STEM_RB=0"]
ITEM_FP8 = ["IRE_FP8_MX=1", "IRE_FP8_MX=0"]
DEEP = ("L2.rb1", "L2.rb2", "L3.rb1", "L3.rb2")
WIDTHS = (32, 64, 128, 256)


def items_expected(env, prec, h, w):
    """{group: (kernel name, slab, nblocks, w4_nt, tiles_x, tiles_y)} of a case of tests/test_items_gpu.py, written out from the rule book's
    prose (not computed by it): the default schedule first, then what the case's switches move."""
    sw = dict(kv.split("=") for kv in env.split(",")) if env != "default" else {}
    grid = lambda l, th=16: (-(-(w >> l) // 32), -(-(h >> l) // th))
    e = {"stem": ("conv_stem", "wstem", 1, 0) + grid(0), "head": ("conv_pc", "wp", 1, 0) + grid(0),
         "down0": ("conv_down", "wd", 1, 0) + grid(1), "down1": ("conv_dnq", "wdq", 1, 0) + grid(2), "down2": ("conv_dnq", "wdq", 2, 0) + grid(3),
         "up2": ("conv_upq", "wuq", 4, 0) + grid(3), "up1": ("conv_up", "wuf", 2, 0) + grid(2), "up0": ("conv_up", "wuf", 1, 0) + grid(1)}
    for l in range(4):
        for g in ("L%d.rb1" % l, "L%d.rb2" % l):
            # 6 tiles at level 2 and 2 at level 3 per image, at both shapes: tiles * (C / 128) * 8 < 256, the 64-cout items
            e[g] = ("conv_pc", "wp", 1, 0) + grid(l) if l < 2 else ("conv_w4", "w4h", WIDTHS[l] // 64, 64) + grid(l)
    for g in DEEP:
        l, c = int(g[1]), WIDTHS[int(g[1])]
        if prec == "fp8":
            e[g] = (("conv_f8", "w8x") if sw["IRE_FP8_MX"] == "1" else ("conv_w4", "w8")) + (c // 128, 0) + grid(l)
        elif sw.get("IRE_W4") == "0":
            e[g] = ("conv_rb", "wp", c // 64, 0) + grid(l)
        elif sw.get("IRE_W4_SPLIT") == "0":
            pk = int(sw.get("IRE_PK", "2")) >= (2 if g.endswith("rb2") else 1)
            e[g] = ("conv_pk" if pk else "conv_w4", "w4", c // 128, 0) + grid(l)
    pc = int(sw.get("IRE_PC", "3"))
    for l in (0, 1):
        if not pc & (1 << l):
            e["L%d.rb1" % l] = e["L%d.rb2" % l] = ("conv_rb", "wp", 1, 0) + grid(l)
    if not pc & 1:
        e["head"] = ("conv_rb", "wp", 1, 0) + grid(0)
    if sw.get("IRE_UPQ") == "0":
        e["up2"] = ("conv_up", "wuf", 4, 0) + grid(3)
    if sw.get("IRE_DNQ") == "0":
        e["down1"], e["down2"] = ("conv_down", "wd", 2, 0) + grid(2), ("conv_down", "wd", 4, 0) + grid(3)
    if sw.get("IRE_UP_FUSE") == "0" or sw.get("IRE_UP_SUBPIX") == "0":
        for l in range(3):
            e["up%d" % l] = ("conv_up", "wu", WIDTHS[l] // 32, 0) + grid(l + 1) if "IRE_UP_FUSE" in sw else ("conv_rb", "wp", max(1, WIDTHS[l] // 64), 0) + grid(l)
            e["fuse%d" % l] = ("conv_mfma", "w", max(1, WIDTHS[l] // 64), 0) + grid(l, 8)
    if sw.get("IRE_DOWN_RB") == "0":
        for l in range(3):
            e["down%d" % l] = ("conv_mfma", "w", WIDTHS[l + 1] // 64, 0) + grid(l + 1, 4)
    if sw.get("IRE_HEAD_RB") == "0":
        e["head"] = ("conv_mfma", "w", 1, 0) + grid(0, 8)
    if sw.get("IRE_STEM_RB") == "0":
        e["stem"] = ("conv_mfma", "w", 1, 0) + grid(0, 8)
    return e


def _item_plans(dumps):
    plans = {}
    for c, g, f in (parse(ln) for ln in dumps["items"].splitlines()[1:]):
        env, prec, n, h, w, s, _ = _case(c)
        assert s is None and g not in plans.get((env, prec, n, h, w), {}), (c, g)
        plans.setdefault((env, prec, n, h, w), {})[g] = f
    return plans


def test_the_item_test_cases_get_the_kernels_slabs_and_grids_their_table_names(dumps):
    plans = _item_plans(dumps)
    cases = [(e, "bf16") + s for s in ITEM_SHAPES for e in ITEM_ENVS] + [(e, "fp8") + s for s in ITEM_SHAPES for e in ITEM_FP8]
    assert set(cases) <= set(plans) and len(cases) == 34
    for env, prec, n, h, w in cases:
        want = items_expected(env, prec, h, w)
        got = {g: (f["kname"], f["w"], int(f["nblocks"]), int(f["w4_nt"]), int(f["tiles_x"]), int(f["tiles_y"])) for g, f in plans[env, prec, n, h, w].items()}
        assert got == want, (env, prec, h, w, {g: (got.get(g), want.get(g)) for g in set(got) | set(want) if got.get(g) != want.get(g)})
        # the plan of these batches does not depend on the grid size: three images fit every coefficient table outright
        assert n <= min(COEF_IMGS["PK"], 8)
    # the geometry classes the shapes were chosen for
    assert items_expected("default", "bf16", 136, 136)["L2.rb1"][4:] == (2, 3) and items_expected("default", "bf16", 136, 136)["L3.rb1"][4:] == (1, 2)
    assert items_expected("default", "bf16", 72, 264)["L2.rb1"][4:] == (3, 2) and items_expected("default", "bf16", 72, 264)["L3.rb1"][4:] == (2, 1)
    assert ((264 >> 2) % 32, (264 >> 3) % 32, (136 >> 2) % 32, (136 >> 3) % 32) == (2, 1, 2, 17)      # the last tile columns: 2, 1, 2 and 17 pixels wide


def _steps(items):
    """the kinds of step from one item of a workgroup to its next: next n-block of the same tile, next tile column, next tile row, next image"""
    kinds = set()
    for (ia, ya, xa, _, ta), (ib, yb, xb, _, tb) in zip(items, items[1:]):
        kinds.add("n-block" if (ia, ta) == (ib, tb) else "image" if ia != ib else "row" if ya != yb else "column")
    return kinds


@pytest.mark.parametrize("cus", [8, 16])
def test_the_item_test_cases_give_workgroups_several_items_and_every_kind_of_step(dumps, cus):
    """What tests/test_items_gpu.py runs with IRE_GRID_CUS = 8 and 16.  A launch's grid is min(items, cus) workgroups (conv_stem: 2 cus;
    the v1 template conv_mfma is not persistent and has no walk)."""
    plans = _item_plans(dumps)
    steps = {}
    launches = 0
    for (env, prec, n, h, w), groups in plans.items():
        if (n, h, w) not in ITEM_SHAPES:
            continue
        for g, f in groups.items():
            if f["kname"] == "conv_mfma":
                continue
            geo = (int(f["tiles_x"]), int(f["tiles_y"]), n, int(f["nblocks"]), 1)
            items = geo[0] * geo[1] * geo[2] * geo[3]
            G = min(items, cus * (2 if f["kname"] == "conv_stem" else 1))
            walks = [[it for _, it in decode(geo, G, b)] for b in range(G)]
            assert sorted(len(wk) for wk in walks)[-1] >= 2, (env, prec, h, w, g, items, G)
            assert sum(len(wk) for wk in walks) == items
            for wk in walks:
                steps.setdefault(f["kname"], set()).update(_steps(wk))
            launches += 1
    assert launches == 34 * 16 - 2 * (4 + 1)      # 16 persistent launches per case; IRE_DOWN_RB=0,IRE_HEAD_RB=0 and IRE_STEM_RB=0 move 4 and 1 to the v1 template
    for k in ("conv_pk", "conv_w4", "conv_f8"):
        assert steps[k] == {"n-block", "column", "row", "image"}, (k, cus, steps[k])


def test_the_batch_of_the_bit_for_bit_test_plans_conv_w4_64_cout_items_unless_the_split_is_off(dumps):
    """(3, 200, 328): 12 and 4 tiles per image at levels 2 and 3, 12 * 1 * 8 and 4 * 2 * 8 < 256 -- under default switches every value of IRE_PK
    plans conv_w4 on the 64-cout items there, so comparing those engines compares conv_w4 with itself.  With IRE_W4_SPLIT=0 the switch decides:
    that is what tests/test_restore_gpu.py::test_producer_consumer_c128_equals_conv_w4_bit_for_bit runs."""
    plans = _item_plans(dumps)
    want = {"0": ("conv_w4", "conv_w4"), "1": ("conv_pk", "conv_w4"), "2": ("conv_pk", "conv_pk")}
    for pk in "012":
        for g in DEEP:
            f = plans["IRE_PK=" + pk, "bf16", 3, 200, 328][g]
            assert (f["kname"], f["w"], f["w4_nt"]) == ("conv_w4", "w4h", "64"), (pk, g)
            f = plans["IRE_W4_SPLIT=0,IRE_PK=" + pk, "bf16", 3, 200, 328][g]
            assert (f["kname"], f["w"], f["w4_nt"], f["nblocks"]) == (want[pk][g.endswith("rb2")], "w4", "0", str(WIDTHS[int(g[1])] // 128)), (pk, g)


# ---- the largest shapes: csrc/conv_plan.hpp's address rule and conv_extents (DESIGN.md "Address arithmetic at the largest shapes") ----------
U32_END = 1 << 32            # resource sizes and per-lane byte offsets are unsigned 32-bit; 0xffffffff asks for the zero padding
INT_MAX = (1 << 31) - 1      # persist.hpp's cursor and the partials layout count in `int`
LARGE_WHOLE = [(1, 4224, 8192), (1, 8064, 8192), (1, 8128, 8192), (1, 8184, 8192), (1, 8192, 8184), (1, 8192, 8192), (1, 8192, 4224), (64, 1024, 1024)]
LARGE_STRIPS = [(4224, 8192, 11), (8064, 8192, 7), (8192, 8184, 8), (8192, 8184, 16), (8192, 8192, 16), (8192, 4224, 8)]      # tests/test_large_shapes_gpu.py's plans


def test_the_address_rule_has_its_boundary_where_a_level_0_tensor_reaches_2_to_the_32(dumps):
    """piece_addressable(rows, w, halo): every tensor of the piece below 2^32 bytes; level 0 (64 bytes a pixel) is the largest.  Among whole
    images the engine admits otherwise (multiples of 8, 16..8192 a side) that refuses 8192 x 8192 alone, where the byte count is 2^32 exactly
    and wraps to a resource of no bytes; among strips (two halo rows) it refuses from 8190 rows of 8192 pixels."""
    rows = [ln.split() for ln in dumps["rule"].splitlines()]
    assert rows[-1] == ["end", str(U32_END)] and len(rows) == 20
    got = {(int(r), int(w), int(halo)): (int(ok), int(b)) for _, r, w, halo, ok, b in rows[:-1]}
    for (r, w, halo), (ok, b) in got.items():
        assert b == (r + 2 * halo) * w * 64 and ok == (b < U32_END), (r, w, halo, ok, b)
    assert [k for k, v in got.items() if not v[0]] == [(8192, 8192, 0), (8192, 8192, 1), (8190, 8192, 1)]
    assert got[8192, 8192, 0][1] == U32_END and got[8190, 8192, 1][1] == U32_END            # exactly the wrap to zero
    assert got[8184, 8192, 0] == (1, U32_END - 8 * 8192 * 64) and got[8192, 8184, 0][0] == 1 and got[8189, 8192, 1][0] == 1
    assert got[4096, 8192, 0] == (1, 1 << 31) and got[4224, 8192, 0][1] > 1 << 31           # admitted, and past what `int` holds
    # the rule as arithmetic over every admitted whole-image shape: one refusal
    sides = range(16, 8193, 8)
    assert [(h, w) for h in sides[-40:] for w in sides[-40:] if h * w * 64 >= U32_END] == [(8192, 8192)]
    assert all(h * w * 64 < U32_END for h in sides for w in sides if (h, w) != (8192, 8192))


def test_every_launch_of_the_largest_shapes_fits_the_types_the_kernels_index_with(dumps):
    """conv_extents of every launch planned for the large-shape tests: one image's tensors (resource sizes, byte offsets: unsigned 32-bit),
    item, stage and partial counts (`int`).  8192 x 8192 whole is printed too and is the only case with a tensor of 2^32 bytes: what the
    rule refuses.  Strips stay below 2^30 bytes, and the batch of 64 ends at byte 2^32 of its level-0 tensors with image 32 at 2^31."""
    assert dumps["large_asan"] == dumps["large"]
    head, *lines = dumps["large"].splitlines()
    fields = head.split()[3:]
    assert fields == "kernel kname in0_bytes in1_bytes out_bytes batch_bytes items stages stat_floats tiles_x tiles_y nblocks nkc".split()
    cases = {}
    for ln in lines:
        c, g, *v = ln.split(" ")
        assert len(v) == len(fields) and g not in cases.get(c, {}), ln          # one plan per (case, group)
        cases.setdefault(c, {})[g] = dict(zip(fields, v))
    want = ["default:bf16:%dx%dx%d" % s for s in LARGE_WHOLE] + ["default:fp8:1x4224x8192", "default:fp8:1x8192x8184"] + \
           ["default:bf16:strip%dof%d:%dx%d" % (s, n, h, w) for h, w, n in LARGE_STRIPS for s in range(n)]
    assert sorted(cases) == sorted(want)
    over = {}
    for c, groups in cases.items():
        _, _, n, h, w, s, ns = _case(c)
        assert set(groups) == set(SCHEDULE) - {"fuse0", "fuse1", "fuse2"}, c     # default switches: `fuse` rides in `up`
        for g, f in groups.items():
            assert f["kernel"] != "V1", (c, g)                                   # every launch is a persistent kernel: grid = min(items, CUs)
            one = max(int(f["in0_bytes"]), int(f["in1_bytes"]), int(f["out_bytes"]))
            assert int(f["items"]) == int(f["tiles_x"]) * int(f["tiles_y"]) * n * int(f["nblocks"]) > 0
            assert int(f["items"]) <= int(f["stages"]) <= INT_MAX and int(f["stat_floats"]) <= INT_MAX, (c, g)
            assert int(f["batch_bytes"]) == n * one < 1 << 40, (c, g)            # 64-bit bases: far from their type's end
            if one >= U32_END:
                over.setdefault(c, []).append(g)
            if s is not None:
                assert one < 1 << 30, (c, g)
    # the one refused shape, and where it breaks: the level-0 tensors are 2^32 bytes -- a 32-bit resource of NO bytes
    l0 = ["stem", "L0.rb1", "L0.rb2", "down0", "up0", "head"]
    assert over == {"default:bf16:1x8192x8192": l0}
    big = cases["default:bf16:1x8192x8192"]
    assert int(big["stem"]["out_bytes"]) == int(big["L0.rb1"]["in0_bytes"]) == int(big["head"]["in0_bytes"]) == U32_END
    assert int(big["L1.rb1"]["out_bytes"]) == 1 << 31
    # the marks the GPU tests cross
    lv0 = lambda c: int(cases[c]["L0.rb2"]["out_bytes"])
    assert 1 << 31 < lv0("default:bf16:1x4224x8192") == lv0("default:bf16:1x8192x4224") == lv0("default:fp8:1x4224x8192") < U32_END
    assert lv0("default:bf16:1x8064x8192") == U32_END - 128 * 8192 * 64 and lv0("default:bf16:1x8184x8192") == U32_END - 8 * 8192 * 64
    assert lv0("default:bf16:1x8192x8184") == lv0("default:fp8:1x8192x8184") == U32_END - (1 << 22)        # the most the rule admits, strippable
    top = cases["default:bf16:1x8192x8184"]                    # a ragged last tile column at every level: 8184, 4092, 2046, 1023 columns
    assert [int(top[g]["tiles_x"]) for g in ("L0.rb1", "L1.rb1", "L2.rb1", "L3.rb1")] == [256, 128, 64, 32]
    b64 = cases["default:bf16:64x1024x1024"]["L0.rb2"]
    assert int(b64["batch_bytes"]) == U32_END and 32 * int(b64["out_bytes"]) == 1 << 31
    # the 64-image batch stays on the producer / consumer kernel at level 0: its coefficient table holds 64 images
    assert cases["default:bf16:64x1024x1024"]["L0.rb1"]["kname"] == "conv_pc"
