"""Row strips layer by layer: every captured tensor and every (A, B) of a strip run against the untiled run of the same engine, bit for
bit (a strip decomposition changes no bit).  tests/test_tiled_gpu.py holds that at the u8 pixels, at widths that are
multiples of 64 and with sessions of one strip; here the widths are ragged at every level, the strip boundaries lie beside the ragged
tile columns, every A/B switch a strip session accepts runs, and sessions hold several strips and start past strip 0.  Nothing here takes a
tolerance.  A failure names the first differing layer in program order, the strip, the row relative to the strip boundary and the column."""
import os
import sys

import numpy as np
import pytest

from image_restoration_platform_amd import synth
from oracle import classifier as oc
from oracle import layer_check as lc

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_layers_gpu import SWITCHES      # noqa: E402

pytestmark = pytest.mark.gpu

def GROUPS_RB(levels):
    """The profile report's layer groups of the ResBlock convolutions of these levels."""
    return ["L%d.rb%d" % (l, i) for l in levels for i in (1, 2)]


# ---- images ---------------------------------------------------------------------------------------------------------------------------
def _images(h, w, n, seed):
    """One synthetic photograph and one image of uniform random bytes; at every strip boundary the rows on its two sides differ in at least
    half their bytes (checked here, on the CPU): a halo row taken from the wrong side, or left stale, cannot look right."""
    imgs = [synth.image(seed, h, w), np.random.default_rng(1000 + seed).integers(0, 256, (h, w, 3), dtype=np.uint8)]
    hr = h // n
    for im in imgs:
        for y0 in range(hr, h, hr):
            assert (im[y0 - 1] != im[y0]).mean() >= 0.5, "rows %d and %d are too much alike to tell a halo row from its neighbour" % (y0 - 1, y0)
    return imgs


def _ab_name(name):
    """The capture's name of the (A, B) a layer staged its input with, or None where the layer applies no GroupNorm."""
    return "head.ab" if name == "pixels" else name + ".ab" if ".rb" in name else None


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _where(name, whole, strips, h, w, nstrips):
    """The first differing element of a layer as text: strip, row relative to the nearer strip boundary, column, channel."""
    l = lc._level(name)
    rows, cols, hr = h >> l, w >> l, (h // nstrips) >> l
    a, b = _bits(whole).reshape(rows, -1), _bits(strips).reshape(rows, -1)
    c = a.shape[1] // cols
    y = int(np.argmax((a != b).any(axis=1)))
    i = int(np.argmax(a[y] != b[y]))
    s, r = divmod(y, hr)
    edge = "row %d below its upper boundary" % r if r < hr - r else "row %d above its lower boundary" % (hr - 1 - r)
    return "%s: strip %d of %d, %s (level-%d row %d), column %d, channel %d: untiled %r, strips %r; %d of %d elements differ" % (
        name, s, nstrips, edge, l, y, i // c, i % c, whole.reshape(rows, -1)[y, i], strips.reshape(rows, -1)[y, i], int((a != b).sum()), a.size)


# ---- the helper every case goes through ------------------------------------------------------------------------------------------------
def _strip_equals_untiled(eng, img, run_strips, up_mode="fused", label=""):
    """img: [H,W,3] uint8 (numpy).  run_strips(img_cuda, scores_cuda) -> the restored image as a cuda tensor; run_strips.n = strip count.
    Returns the engine's profile report of the captured strip run (layer group -> kernel name)."""
    import torch
    h, w, _ = img.shape
    n = run_strips.n
    sc = torch.from_numpy(np.asarray(oc.classify(img, True)[0], np.float64)).cuda()
    x = torch.from_numpy(img).cuda()
    names = lc.layer_names(up_mode)
    eng.debug_capture(True)
    try:
        whole = eng.restore_tensor(x[None], scores=sc[None])[0].cpu().numpy()
        ref = {}
        for nm in names:
            ref[nm] = whole if nm == "pixels" else eng.activation(nm).copy()
            if _ab_name(nm):
                ref[_ab_name(nm)] = eng.activation(_ab_name(nm)).copy()
        eng.debug_capture(True)                       # (clears what the untiled run left)
        eng.profile_reset()
        eng.profile_enable(1)
        try:
            got = run_strips(x, sc).cpu().numpy()
            report = {r["group"]: r["kernel"] for r in eng.profile_report()}
        finally:
            eng.profile_enable(0)
        for nm in names:                              # program order: the first name reported is where the runs part
            ab = _ab_name(nm)
            if ab:
                a, b = _bits(ref[ab]), _bits(eng.activation(ab))
                assert a.shape == b.shape and np.array_equal(a, b), "%s %s: the (A, B) of the strip run differ at channel %d" % (
                    label, ab, int(np.argmax(a != b)) // 2 if a.shape == b.shape else -1)
            t = got if nm == "pixels" else eng.activation(nm)
            assert t.size == ref[nm].size, (label, nm, t.size, ref[nm].size)
            if nm == "pixels":
                assert np.array_equal(t, ref[nm]), label + " " + _where(nm, ref[nm].astype(np.float32), t.astype(np.float32), h, w, n)
            else:
                assert np.array_equal(_bits(t), _bits(ref[nm])), label + " " + _where(nm, ref[nm], t, h, w, n)
    finally:
        eng.debug_capture(False)
    # capture synchronises the stream after every convolution of every strip; an ordinary run must give the same bytes
    again = run_strips(x, sc).cpu().numpy()
    assert np.array_equal(again, whole), label + " an ordinary strip run differs from the captured one: " + _where(
        "pixels", whole.astype(np.float32), again.astype(np.float32), h, w, n)
    assert np.abs(whole.astype(np.int32) - img.astype(np.int32)).mean() > 1.0      # the network did something
    return report


def _virtual(eng, n):
    """All strips as virtual ranks of one session (Engine.restore_tiled_tensor)."""
    def run(x, sc):
        return eng.restore_tiled_tensor(x, n, scores=sc)
    run.n = n
    return run


# ---- geometry classes: what each shape exists for, asserted so that a changed plan rule fails the case instead of moving it -------------
def _tiles(h, w, l):
    return -(-(h >> l) // 16) * -(-(w >> l) // 32)


def _items_64(h, w, l):
    """conv_plan.hpp's rule for the 64-cout items of conv_w4: a batch of 8 such images would not fill 256 CUs with 128-cout items.  (A
    restatement: tests/test_conv_plan.py plans the strips of these very shapes with plan_conv itself and asserts the item form there.)"""
    return _tiles(h, w, l) * (lc.WIDTHS[l] // 128) * 8 < 256


def _assert_geometry(h, w, n):
    hr = h // n
    assert hr % 128 == 0 and n >= 2
    if (h, w, n) == (384, 264, 3):
        assert [(w >> l) % 32 for l in range(4)] == [8, 4, 2, 1]            # ragged at every level; the last level-3 tile column is 1 wide
        assert hr >> 3 == 16 and -(-(w >> 3) // 32) == 2                       # a level-3 strip: one tile row of two tile columns
        assert _items_64(h, w, 2) and _items_64(h, w, 3)
    elif (h, w, n) == (1024, 264, 8):
        assert _tiles(h, w, 3) == 16 and _tiles(h, w, 2) == 48
        assert not _items_64(h, w, 2) and not _items_64(h, w, 3)
    elif (h, w, n) == (256, 72, 2):
        assert w >> 3 == 9 and -(-w // 32) == 3 and w % 32 == 8
    elif (h, w, n) == (512, 264, 4):
        assert (w >> 3) % 32 == 1
    else:
        raise AssertionError("no geometry class for %r" % ((h, w, n),))


def _assert_kernels(report, expect, label):
    for group, kernel in expect.items():
        assert report.get(group) == kernel, "%s: layer group %s ran on %r, the case exists for %r (report: %r)" % (label, group, report.get(group), kernel, report)


CASES = [(384, 264, 3, "conv_w4"), (1024, 264, 8, "conv_pk"), (256, 72, 2, "conv_w4")]


@pytest.mark.parametrize("h,w,n,deep", CASES, ids=lambda v: str(v))
def test_default_engine_strips_equal_untiled_at_every_layer(engine, h, w, n, deep):
    """(384, 264, 3): ragged at every level, a middle strip, the deep levels on conv_w4's 64-cout items.  (1024, 264, 8): both deep levels on
    conv_pk with ragged columns and first, middle and last strips.  (256, 72, 2): one partial tile at level 3, a last tile column 8 wide."""
    _assert_geometry(h, w, n)
    for i, img in enumerate(_images(h, w, n, seed=h // 64 + n)):
        label = "default %dx%d in %d, image %d:" % (h, w, n, i)
        rep = _strip_equals_untiled(engine, img, _virtual(engine, n), label=label)
        exp = dict.fromkeys(GROUPS_RB((2, 3)), deep)
        exp.update(dict.fromkeys(GROUPS_RB((0, 1)) + ["head"], "conv_pc"), stem="conv_stem", down0="conv_down", down1="conv_dnq", down2="conv_dnq",
                   up2="conv_upq", up1="conv_up", up0="conv_up")
        _assert_kernels(rep, exp, label)


@pytest.mark.parametrize("mx", ["1", "0"])
@pytest.mark.parametrize("h,w,n", [(384, 264, 3), (1024, 264, 8)])
def test_fp8_engine_strips_equal_untiled_at_every_layer(h, w, n, mx, monkeypatch):
    """conv_f8 (IRE_FP8_MX=1) and conv_w4's fp8 form (=0) beside a strip boundary at a ragged edge."""
    from image_restoration_platform_amd.engine import Engine
    _assert_geometry(h, w, n)
    monkeypatch.setenv("IRE_FP8_MX", mx)
    eng = Engine(device_index=0, max_batch=1, precision="fp8")
    try:
        for i, img in enumerate(_images(h, w, n, seed=3 + n)):
            label = "fp8 mx=%s %dx%d in %d, image %d:" % (mx, h, w, n, i)
            rep = _strip_equals_untiled(eng, img, _virtual(eng, n), label=label)
            _assert_kernels(rep, dict.fromkeys(GROUPS_RB((2, 3)), "conv_f8" if mx == "1" else "conv_w4"), label)
    finally:
        eng.close()


# ---- every A/B switch a strip session accepts --------------------------------------------------------------------------------------------
def _switched_kernels(env):
    """Layer groups the switch set moves, and the kernel the profile report must name for them."""
    if env == {"IRE_PK": "0"}:
        return dict.fromkeys(GROUPS_RB((2, 3)), "conv_w4")
    if env == {"IRE_PC": "0"}:
        return dict.fromkeys(GROUPS_RB((0, 1)) + ["head"], "conv_rb")
    if env == {"IRE_PC": "1"}:
        return dict(dict.fromkeys(GROUPS_RB((1,)), "conv_rb"), **dict.fromkeys(GROUPS_RB((0,)) + ["head"], "conv_pc"))
    if env == {"IRE_W4": "0"}:
        return dict.fromkeys(GROUPS_RB((2, 3)), "conv_rb")
    if env == {"IRE_UPQ": "0"}:
        return {"up2": "conv_up"}
    if env == {"IRE_DNQ": "0"}:
        return {"down1": "conv_down", "down2": "conv_down"}
    if env == {"IRE_UP_FUSE": "0"}:
        return dict(dict.fromkeys(["up0", "up1", "up2"], "conv_up"), **dict.fromkeys(["fuse0", "fuse1", "fuse2"], "conv_mfma"))
    if env == {"IRE_UP_SUBPIX": "0"}:
        return dict(dict.fromkeys(["up0", "up1", "up2"], "conv_rb"), **dict.fromkeys(["fuse0", "fuse1", "fuse2"], "conv_mfma"))
    if env == {"IRE_GN_FOLD": "0"}:
        return {}                                     # no convolution moves: the untiled run finalizes in launches of its own (asserted below)
    if env == {"IRE_DOWN_RB": "0", "IRE_HEAD_RB": "0"}:
        return dict.fromkeys(["down0", "down1", "down2", "head"], "conv_mfma")
    if env == {"IRE_STEM_RB": "0"}:
        return {"stem": "conv_mfma"}
    raise AssertionError("no expectation for the switch set %r" % (env,))


@pytest.mark.parametrize("env", SWITCHES, ids=lambda e: ",".join("%s=%s" % kv for kv in e.items()))
def test_strips_equal_untiled_at_every_layer_behind_every_switch(env, monkeypatch):
    """A fresh engine per switch set of test_layers_gpu.SWITCHES; 384x264 in 3 strips (IRE_PK=0: 1024x264 in 8, where conv_w4 gets the
    128-cout items conv_pk takes by default).  The report of the strip run must name the switched kernel for its layers."""
    import torch
    from image_restoration_platform_amd.engine import Engine
    h, w, n = (1024, 264, 8) if env == {"IRE_PK": "0"} else (384, 264, 3)
    _assert_geometry(h, w, n)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    up_mode = "plain" if env.get("IRE_UP_SUBPIX") == "0" else "subpix" if env.get("IRE_UP_FUSE") == "0" else "fused"
    eng = Engine(device_index=0, max_batch=1)
    try:
        for i, img in enumerate(_images(h, w, n, seed=11)):
            label = "%s %dx%d in %d, image %d:" % (" ".join("%s=%s" % kv for kv in env.items()), h, w, n, i)
            rep = _strip_equals_untiled(eng, img, _virtual(eng, n), up_mode=up_mode, label=label)
            _assert_kernels(rep, _switched_kernels(env), label)
        if env == {"IRE_GN_FOLD": "0"}:
            x = torch.from_numpy(img).cuda()
            eng.profile_reset()
            eng.profile_enable(1)
            eng.restore_tensor(x[None])
            launches = eng.profile_query("gn_finalize")["launches"]
            eng.profile_enable(0)
            assert launches >= 33, launches          # one per GroupNorm: the untiled side of this case did not fold them
    finally:
        eng.close()


def test_the_v1_schedule_is_still_refused_by_name(monkeypatch):
    from image_restoration_platform_amd import _lib
    from image_restoration_platform_amd.engine import Engine, EngineError
    monkeypatch.setenv("IRE_CONV_V1", "1")
    eng = Engine(device_index=0, max_batch=1)
    try:
        with pytest.raises(EngineError) as e:
            eng.open_strips(384, 264, 3, 0, 3)
        assert e.value.status == _lib.IRE_ERR_INVALID_INPUT and "IRE_CONV_V1=1" in e.value.message and "invalid" in e.value.message
    finally:
        eng.close()


# ---- split sessions in one process: the layout of a node with fewer GPUs than strips ------------------------------------------------------
def _split(eng, h, w, layout, checks):
    """layout: list of lists of consecutive strip indices, one list per session ("rank").  The driver below is one process playing every
    rank: per op it runs and packs every session, moves the halo rows and the partials slices with torch copies, then unpacks."""
    import torch
    total = sum(len(r) for r in layout)
    hr = h // total
    sessions = [eng.open_strips(h, w, total, r[0], len(r)) for r in layout]

    def run(x, sc):
        for s, r in zip(sessions, layout):
            y0, rows = r[0] * hr, len(r) * hr
            piece = torch.zeros((rows + 2, w, 3), dtype=torch.uint8, device=x.device)
            lo, hi = max(0, y0 - 1), min(h, y0 + rows + 1)
            piece[lo - (y0 - 1):hi - (y0 - 1)] = x[lo:hi]
            s.set_input(piece, sc)
        for k in range(sessions[0].num_ops):
            infos = [s.run_op(k) for s in sessions]
            hb = int(infos[0].halo_bytes)
            assert all(int(i.halo_bytes) == hb for i in infos)
            if hb:
                for s, r, i in zip(sessions, layout, infos):
                    assert (bool(i.has_up), bool(i.has_down)) == (r[0] > 0, r[-1] + 1 < total), (k, r, i.has_up, i.has_down)
                    s.pack_halo(k)
                for a, b in zip(sessions[:-1], sessions[1:]):
                    b.recv_up[:hb].copy_(a.send_down[:hb])
                    a.recv_down[:hb].copy_(b.send_up[:hb])
            tot = int(infos[0].stats_total_bytes)
            if tot:
                per = tot // total
                assert per * total == tot and 0 < tot <= sessions[0].stats.numel()
                end = 0
                for s, r, i in zip(sessions, layout, infos):
                    off, loc = int(i.stats_offset_bytes), int(i.stats_local_bytes)
                    assert (off, loc, int(i.stats_total_bytes)) == (per * r[0], per * len(r), tot), (k, r, off, loc, per)
                    assert off == end                  # disjoint, in rank order, no gap
                    end = off + loc
                    for o in sessions:
                        if o is not s:
                            o.stats[off:off + loc].copy_(s.stats[off:off + loc])
                assert end == tot                      # the slices cover the array
                # every session finalizes from its own copy of the array into its own (A, B), and the sessions of one engine share the
                # capture entry "<layer>.ab" (the last session's stays): equal arrays here are what makes that one entry speak for all
                for o in sessions[1:]:
                    assert torch.equal(o.stats[:tot], sessions[0].stats[:tot]), (k, "the sessions hold different partials")
                checks["stats_ops"] = checks.get("stats_ops", 0) + 1
            else:
                assert all(int(i.stats_local_bytes) == 0 for i in infos)
            if hb:
                for s in sessions:
                    s.unpack_halo(k)
                checks["halo_ops"] = checks.get("halo_ops", 0) + 1
        return torch.cat([s.get_output() for s in sessions], dim=0)
    run.n = total
    run.close = lambda: [s.close() for s in sessions]
    return run


@pytest.mark.parametrize("h,w,layout", [(512, 264, [[0, 1], [2, 3]]), (512, 264, [[0], [1, 2, 3]]), (512, 264, [[0], [1], [2], [3]]),
                                        (512, 264, [[0], [1, 2], [3]]), (384, 264, [[0], [1, 2]])], ids=lambda v: str(v).replace(" ", ""))
def test_split_sessions_equal_untiled_at_every_layer(engine, h, w, layout):
    """Sessions of several strips, sessions that start past strip 0, and a rank with a neighbour on both sides going through pack_halo /
    unpack_halo: strips_.front() against strips_.back(), the partials slice at per_strip * first_strip of per_strip * nlocal bytes.
    Front and back differ only in a session of several strips, and each direction counts only where that session has the neighbour:
    [0,1]+[2,3] has one with a lower and one with an upper neighbour, [0]+[1,2]+[3] one with both; in [0]+[1,2,3] and [0]+[1,2] the session
    of several strips is the last, so only its upper side is exchanged."""
    total = sum(len(r) for r in layout)
    _assert_geometry(h, w, total)
    checks = {}
    run = _split(engine, h, w, layout, checks)
    try:
        for i, img in enumerate(_images(h, w, total, seed=30 + total)):
            _strip_equals_untiled(engine, img, run, label="%dx%d as %r, image %d:" % (h, w, layout, i))
    finally:
        run.close()
    # the driver saw what it is here for: 39 convolutions exchange halo rows and write partials, in each of the 2 x 2 strip runs
    assert checks["halo_ops"] == checks["stats_ops"] == 4 * 39, checks
