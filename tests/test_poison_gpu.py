"""Every entry point on dirty scratch: the result of a call is a function of its inputs alone, whatever the engine's scratch held.

IRE_DEBUG_POISON (csrc/buf_registry.hpp) is read once per process, so the cases run in four fresh child processes started with
IRE_DEBUG_POISON=165: every allocation of either memory policy is born as 0xA5, the weights and tables before their upload included.
A child makes its calls once and compares each with its independent reference (Pillow, tests/*_model.py, oracle/*, oracle/layer_check.py),
then fills every scratch allocation of the process through ire_debug_poison_scratch with 0xFF (bf16 NaN; absurd statuses, counts and
tickets), 0x00 (what fresh memory looks like: the control, and what catches reliance on non-zero) and 0x5A (plausible finite data), and
makes the same calls again after each: all four results must equal the reference byte for byte, and the four results must equal each
other.  Inside a child the calls go large -> small -> large, so a small call runs inside a big dirty buffer.

  A  decoders: baseline, multi-window and progressive JPEG, PNG of every colour type, depth and Adam7, batches of old, new and mixed forms
     with an image pitch and guard bytes, a corrupt file between two good ones (the status the CPU form gives it, its neighbours 0), three
     device-entry calls back to back on one stream
  B  encoders: the five text formats through the window entry on one stream with one synchronise (guard bytes behind every text) and
     through the host entry; the table kernel and the progressive path from coefficients
  C  the network (teacher-forced per-layer check on the first run, every captured tensor equal to it afterwards) on the default engine,
     the fp8 engines, conv_pk and the unfolded GroupNorm; every other kernel switch by its pixels; restore_fit, strips, classify,
     preprocess (single and batch), fuse, to_srgb
  D  jobs: fit, file, upload (JPEG, PNG, 16-bit Adam7 PNG, ICC-tagged), fusion and a corrupt upload on a progressive-JPEG text engine and a
     pixel engine, every round submitted whole before its first poll; a poison call while jobs are unpolled is refused

The children run one after another; when one exits non-zero, by a signal or at its time limit, no further child starts and every test that
needs it or a later one fails with its stderr.  Nothing is retried.  A child reports one record per case and stage; the parent fails on a
record that is missing.  What a flagged (corrupt) image leaves in its pixels is nobody's result and is not compared; its status is."""
import ctypes
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import jpeg_prog_writer as writer      # noqa: E402
import jpeg_progenc_cases as progenc_cases      # noqa: E402
from test_layers_gpu import SWITCHES      # noqa: E402

pytestmark = pytest.mark.gpu

BIRTH = 0xA5                       # IRE_DEBUG_POISON of every child: what an allocation holds when it is handed out
BYTES = (0xFF, 0x00, 0x5A)         # ire_debug_poison_scratch, in this order
STAGES = (None,) + BYTES
GUARD = 0x3C
CHILDREN = ("A", "B", "C", "D")
# seconds: about three times the wall time of each child as measured on an MI355X ("Scratch independence": 4.1, 2.4, 6.0
# and 2.9 s; child A's includes its two g++ runs).  A child that hangs holds the GPU for this long and no longer.
CHILD_TIMEOUT = {"A": 15, "B": 10, "C": 20, "D": 10}

CHECKED = [("default", "bf16", {}), ("fp8 mx=1", "fp8", {"IRE_FP8_MX": "1"}), ("fp8 mx=0", "fp8", {"IRE_FP8_MX": "0"}),
           ("conv_pk", "bf16", {"IRE_W4_SPLIT": "0"}), ("gn unfolded", "bf16", {"IRE_GN_FOLD": "0"})]
OTHERS = [env for env in SWITCHES if env != {"IRE_GN_FOLD": "0"}]


def _sw_id(env):
    return ",".join("%s=%s" % kv for kv in env.items())


NAMES = {
    "A": ["jpeg 1x1", "jpeg 17x13 4:2:0", "jpeg 45x37 4:2:2", "jpeg grey 33x47", "jpeg 40x88 with restart markers",
          "jpeg q95 noise, several windows", "jpeg 96x96 4:2:0, one window", "jpeg q95 noise, several windows, again"] +
         [x for i, s in enumerate(sorted(writer.SCRIPTS)) for x in (["progressive %s 8x8" % s] + (["jpeg baseline between two progressive files"] if i == 0 else []))] +
         ["progressive long refinement 320x320"] +
         ["png colour type %d 5x7" % ct for ct in (0, 2, 3, 4, 6)] +
         ["png 1-bit grey 17x9", "png 4-bit palette Adam7 5x3", "png 16-bit RGBA Adam7 33x70", "png 16-bit RGB Adam7 131x9",
          "png batch, old forms", "png batch, new forms", "png batch, old and new forms with a pitch and guard bytes",
          "corrupt png between two good ones", "corrupt refinement scan between two good files", "filter byte 5 on an Adam7 pass between two good files",
          "three device calls on one stream, small large small"],
    "B": ["window entry cells2 33x130", "window entry flat 16x24", "window entry noise 45x37",
          "host entry cells2 33x130", "host entry flat 16x24", "host entry noise 45x37", "table kernel on fib30", "progressive from coefficients"],
    "C": ["network " + label for label, _, _ in CHECKED] + ["pixels " + _sw_id(env) for env in OTHERS] +
         ["restore_fit 50x70", "restore_fit 9x131", "strips 384x264 in 3", "classify 3x40x515", "preprocess 301x777 orientation 6 -> 256",
          "preprocess batch 131x97 -> 64", "fuse k=3 64x64", "fuse k=3 128x128", "fuse k=3 64x64 again", "to_srgb two profiles"],
    "D": ["text engine: fit 50x70", "text engine: fit 9x131", "text engine: baseline file", "text engine: progressive file",
          "text engine: upload 4:2:0 orientation 6", "text engine: upload 8-bit png", "text engine: upload 16-bit Adam7 png", "text engine: upload icc-tagged",
          "text engine: fusion k=2 70x90", "text engine: corrupt upload", "pixel engine: fit 50x70", "pixel engine: upload 4:2:0 orientation 6",
          "poison call refused while jobs are unpolled",
          "second sizes, text engine: fit 24x40", "second sizes, text engine: fit 130x20", "second sizes, text engine: baseline file 96x80",
          "second sizes, text engine: progressive file 17x13", "second sizes, text engine: upload 4:4:4 300x257", "second sizes, text engine: upload 8-bit rgba png 24x20",
          "second sizes, text engine: upload 16-bit Adam7 png 33x70", "second sizes, text engine: upload icc-tagged 56x32", "second sizes, text engine: fusion k=3 64x64",
          "second sizes, pixel engine: fit 24x40", "second sizes: poison call refused while jobs are unpolled",
          "poison call refused for a delivered, unpolled job"],
}
assert all(len(set(v)) == len(v) for v in NAMES.values())


# ---- the children: python tests/test_poison_gpu.py CHILD OUT.json -------------------------------------------------------------------------------
class Verdict(Exception):
    """a case that ends in a statement instead of a result (a refusal where a result was due, a failed per-layer check)"""


def _u8(x):
    if isinstance(x, (bytes, bytearray)):
        return np.frombuffer(bytes(x), np.uint8)
    if isinstance(x, str):
        return np.frombuffer(x.encode(), np.uint8)
    return np.ascontiguousarray(np.asarray(x)).reshape(-1).view(np.uint8)


def _diff(got, want):
    """None when the two lists hold the same bytes, else (item, first differing offset)"""
    if len(got) != len(want):
        return min(len(got), len(want)), 0
    for i, (g, w) in enumerate(zip(got, want)):
        a, b = _u8(g), _u8(w)
        n = min(a.size, b.size)
        d = np.nonzero(a[:n] != b[:n])[0]
        if d.size:
            return i, int(d[0])
        if a.size != b.size:
            return i, n
    return None


def _digest(items):
    h = hashlib.sha256()
    for x in items:
        a = _u8(x)
        h.update(str(a.size).encode() + b":")
        h.update(a.tobytes())
    return h.hexdigest()


def _record(name, stage, fn):
    from image_restoration_platform_amd import _lib
    from image_restoration_platform_amd.engine import EngineError
    t0 = time.perf_counter()
    rec = {"name": name, "byte": stage, "ok": False, "item": None, "offset": None, "what": None, "digest": None}
    try:
        got, want = fn()
        d = _diff(got, want)
        rec["ok"], rec["digest"] = d is None, _digest(got)
        if d is not None:
            rec["item"], rec["offset"] = d
    except Verdict as e:
        rec["what"] = str(e)[-1500:]
    except EngineError as e:
        if e.status != _lib.IRE_ERR_INVALID_INPUT:          # anything else (a device error among them) ends the child
            raise
        rec["what"] = "refused: " + e.message
    rec["seconds"] = time.perf_counter() - t0
    print("POISONCASE %-70s byte %-4s %s %.2f s" % (name, stage, "ok" if rec["ok"] else "DIFFERS %s %s %s" % (rec["item"], rec["offset"], rec["what"]), rec["seconds"]), flush=True)
    return rec


def _drive(eng, cases, result):
    """the cases once, then again behind each poison call"""
    for stage in STAGES:
        if stage is not None:
            result["filled"].append(int(eng.debug_poison_scratch(stage)))
        for name, fn in cases:
            result["records"].append(_record(name, stage, fn))


def _once(make):
    """a reference computed at its first use and left unchanged"""
    box = []

    def get():
        if not box:
            box.append(make())
        return box[0]
    return get


def _native(src):
    """a simulator of tests/native built plain (no sanitizer runs beside a GPU) -> (the program, its own temporary directory)"""
    tmp = tempfile.mkdtemp(prefix="poison_native_")
    exe = os.path.join(tmp, "sim")
    r = subprocess.run(["g++", "-std=c++17", "-O1", os.path.join(HERE, "native", src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe, tmp


def _consts():
    src = open(os.path.join(ROOT, "image_restoration_platform_amd", "csrc", "jpeg_dec_core.hpp")).read()
    get = lambda pat: int(re.search(pat, src).group(1))      # noqa: E731
    return get(r"constexpr int kLanes = (\d+);") * get(r"constexpr int kSubseqBits = (\d+);"), get(r"constexpr unsigned kShortMaxBytes = (\d+);"), get(r"constexpr int kStBadRange = (\d+);")


def _child_a(result):
    import torch
    import jpeg_decode_cases as jc
    import jpeg_decode_model as jm
    import jpeg_prog_cases as prog
    import jpeg_prog_model as pm
    import png_cases as pc
    import png_depth_cases as pd
    from image_restoration_platform_amd import _lib
    from image_restoration_platform_amd.engine import Engine
    window_bits, short, bad_range = _consts()
    eng = Engine(device_index=0, max_batch=8, num_streams=1, weights_path=None,
                 flags=_lib.IRE_FLAG_DECODE_PNG | _lib.IRE_FLAG_DECODE_PNG_ALL | _lib.IRE_FLAG_DECODE_PROGRESSIVE)
    cases = []

    def host_jpeg(name, data, src=None):
        want = jc.pillow_pixels(src if src is not None else data)
        cases.append((name, lambda: ([eng.decode_jpeg(data)], [want])))

    def host_png(name, data):
        want = pd.pil_rgb(data)
        cases.append((name, lambda: ([eng.decode_png(data)], [want])))

    host_jpeg("jpeg 1x1", jc.encode(jc.noise(1, 1, 1), 85, 0))
    host_jpeg("jpeg 17x13 4:2:0", jc.encode(jc.noise(13, 17, 172), 85, 2))
    host_jpeg("jpeg 45x37 4:2:2", jc.encode(jc.noise(37, 45, 451), 85, 1))
    host_jpeg("jpeg grey 33x47", jc.encode(jc.smooth(47, 33, 33)[:, :, 0], 85))
    host_jpeg("jpeg 40x88 with restart markers", jc.encode(jc.smooth(88, 40, 3), 85, 2, restart_marker_blocks=3))
    side = 64
    while True:                                   # tests/test_jpeg_decode_gpu.py's stream: sized from the kernel's constants to >= 2.5 windows
        many = jc.encode(jc.noise(side, side, 77), 95, 0)
        p = jm.plan(many)
        if 8 * len(p.streams[0][0]) >= 2.5 * window_bits:
            break
        side += 32
    assert len(p.streams) == 1 and len(p.streams[0][0]) > short
    one = jc.encode(jc.noise(96, 96, 42), 95, 2)
    n_one = len(jm.plan(one).streams[0][0])
    assert short < n_one and 8 * n_one <= window_bits          # a long stream of one window: lanes, but no lane records
    host_jpeg("jpeg q95 noise, several windows", many)
    host_jpeg("jpeg 96x96 4:2:0, one window", one)
    host_jpeg("jpeg q95 noise, several windows, again", many)
    written = prog.writer_cases()
    for i, s in enumerate(sorted(writer.SCRIPTS)):
        data, src = written["%s_8x8_s0" % s]
        host_jpeg("progressive %s 8x8" % s, data, src)
        if i == 0:
            host_jpeg("jpeg baseline between two progressive files", jc.encode(jc.noise(47, 33, 3), 85, 2))
    host_jpeg("progressive long refinement 320x320", prog.long_refinement_file())
    for ct in (0, 2, 3, 4, 6):
        host_png("png colour type %d 5x7" % ct, pc.make(5, 7, ct))
    host_png("png 1-bit grey 17x9", pd.make(17, 9, 0, 1, 0, seed=9))
    host_png("png 4-bit palette Adam7 5x3", pd.make(5, 3, 3, 4, 1, seed=8))
    host_png("png 16-bit RGBA Adam7 33x70", pd.make(33, 70, 6, 16, 1, seed=3))
    host_png("png 16-bit RGB Adam7 131x9", pd.make(131, 9, 2, 16, 1, filters=(4, 3, 1, 2, 0, 4, 4), seed=2))

    def png_batch(files, gap):
        """-> [the images, the bytes behind each, the status words] through the device entry"""
        h, w = pd.head_of(files[0])[:2]
        n, ib = len(files), h * w * 3
        buf = torch.full((n, ib + gap), GUARD, dtype=torch.uint8, device="cuda")
        _, status = eng.decode_png_device(files, out_u8=buf[:, :ib].view(n, h, w, 3))
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        return [np.ascontiguousarray(host[:, :ib]), np.ascontiguousarray(host[:, ib:]), status.cpu().numpy()]

    def png_batch_case(name, files, gap):
        h, w = pd.head_of(files[0])[:2]
        want = [np.stack([pd.pil_rgb(f).reshape(-1) for f in files]), np.full((len(files), gap), GUARD, np.uint8), np.zeros(len(files), np.int32)]
        cases.append((name, lambda: (png_batch(files, gap), want)))

    h, w = 70, 33
    old = [pc.make(h, w, 2, seed=40), pc.make(h, w, 3, seed=44), pc.make(h, w, 6, seed=48)]
    new = [pd.make(h, w, 2, 8, 1, seed=41), pd.make(h, w, 3, 4, 0, seed=42), pd.make(h, w, 6, 16, 1, seed=43), pd.make(h, w, 0, 1, 1, seed=45), pd.make(h, w, 0, 2, 0, seed=47)]
    png_batch_case("png batch, old forms", old, 0)
    png_batch_case("png batch, new forms", new, 0)
    png_batch_case("png batch, old and new forms with a pitch and guard bytes", [old[0], new[0], new[1], new[2], old[1], new[3], old[2], new[4]], 37)

    # a corrupt file between two good ones: the status its CPU form gives it (the simulators, built plain), 0 for its neighbours
    any_exe, any_tmp = _native("png_any_sim.cpp")
    prog_exe, prog_tmp = _native("jpeg_prog_sim.cpp")

    def cpu_png_status(data):
        src = os.path.join(any_tmp, "in.png")
        with open(src, "wb") as f:
            f.write(data)
        lines = subprocess.run([any_exe, "dump", src, os.path.join(any_tmp, "rgb.bin"), os.path.join(any_tmp, "scan.bin"), str(pd.ACCEPT_ALL)], capture_output=True, text=True, timeout=60).stdout.splitlines()
        assert lines[1].startswith("status "), lines
        return int(lines[1].split()[1])

    def cpu_jpeg_status(data):
        src = os.path.join(prog_tmp, "in.jpg")
        with open(src, "wb") as f:
            f.write(data)
        lines = subprocess.run([prog_exe, "dump", src, os.path.join(prog_tmp, "out.bin")], capture_output=True, text=True, timeout=60).stdout.splitlines()
        assert lines[1].startswith("status "), lines
        return int(lines[1].split()[1])

    def corrupt_png_case(name, good, bad):
        want_px, st = pd.pil_rgb(good).reshape(-1), cpu_png_status(bad)
        assert st != 0 and cpu_png_status(good) == 0

        def run():
            got = png_batch([good, bad, good], 0)
            return [got[0][0], got[0][2], got[2]], [want_px, want_px, np.array([0, st, 0], np.int32)]
        cases.append((name, run))

    corrupt_png_case("corrupt png between two good ones", pc.fuzz_file(), pc.corrupt_cases()["distance_too_far"])

    def flagged(d):
        try:
            pm.coefficients(pm.plan(d))
        except pm.Corrupt:
            return True
        except pm.Refused:
            return False
        return False
    good_j, variants = prog.corrupt_refinement_candidates()
    bad_j = next(d for _, d in variants if flagged(d))
    st_j = cpu_jpeg_status(bad_j)
    assert st_j != 0 and cpu_jpeg_status(good_j) == 0
    want_j = jc.pillow_pixels(good_j)

    def corrupt_jpeg():
        out, status = eng.decode_jpeg_device([good_j, bad_j, good_j])
        torch.cuda.synchronize()
        st = status.cpu().numpy()
        # (the CPU form has no inverse transform, so it cannot give the out-of-range bit that garbage coefficients may add on the device)
        return [out[0].cpu().numpy(), out[2].cpu().numpy(), st & ~np.int32(bad_range)], [want_j, want_j, np.array([0, st_j & ~bad_range, 0], np.int32)]
    cases.append(("corrupt refinement scan between two good files", corrupt_jpeg))
    bad5, good5 = pd.bad_filter_adam7()
    corrupt_png_case("filter byte 5 on an Adam7 pass between two good files", good5, bad5)

    small_a, small_b = jc.encode(jc.noise(13, 17, 5), 85, 2), jc.encode(jc.noise(5, 7, 2), 85, 0)
    want3 = [jc.pillow_pixels(small_a), jc.pillow_pixels(many), jc.pillow_pixels(small_b), np.zeros(3, np.int32)]

    def three_calls():
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        res = [eng.decode_jpeg_device([f], stream=s) for f in (small_a, many, small_b)]      # both pinned blobs in turn, no wait between
        s.synchronize()
        return [o[0].cpu().numpy() for o, _ in res] + [np.array([int(st[0]) for _, st in res], np.int32)], want3
    cases.append(("three device calls on one stream, small large small", three_calls))

    assert [n for n, _ in cases] == NAMES["A"], [n for n, _ in cases]
    try:
        _drive(eng, cases, result)
    finally:
        eng.close()
        shutil.rmtree(any_tmp, ignore_errors=True)
        shutil.rmtree(prog_tmp, ignore_errors=True)


def _child_b(result):
    import torch
    import jpeg_huffopt_cases as hc
    import jpeg_huffopt_model as huffopt
    import jpeg_opt_cases as oc
    import jpeg_opt_model as opt
    import jpeg_progenc_model as progenc
    import png_deflate_model as deflate
    from image_restoration_platform_amd.engine import TEXT_FORMATS, Engine
    from oracle import encode as oenc
    eng = Engine(device_index=0, max_batch=8, num_streams=1)
    assert oc.big_class(100, 2)
    as_bytes = lambda t: t if isinstance(t, bytes) else t.encode()      # noqa: E731
    # the six calls of one sequence: (format, settings, the model's text)
    SEQ = [("png", None, lambda px: as_bytes(oenc.png_base64(px))), ("png_deflate", None, lambda px: as_bytes(deflate.png_base64(px))),
           ("jpeg", (85, 0), lambda px: as_bytes(opt.jpeg_base64(px, 85, 0))), ("jpeg_opt", (100, 2), lambda px: as_bytes(huffopt.jpeg_base64(px, 100, 2))),
           ("jpeg_prog", (1, 0), lambda px: as_bytes(progenc.jpeg_base64(px, 1, 0)))]
    tiny = hc.noise(8, 8, 3)

    def models(px):
        return [m(px) for _, _, m in SEQ] + [SEQ[0][2](tiny)]

    def window(px):
        n, h, w, _ = px.shape
        big = torch.full((n, h + 5, w + (7 if w % 2 == 0 else 6), 3), GUARD, dtype=torch.uint8, device="cuda")
        big[:, :h, :w] = torch.from_numpy(np.array(px)).cuda()
        return big[:, :h, :w]

    def device_call(fmt, settings, t, stream):
        f = TEXT_FORMATS[fmt]
        ex = () if settings is None else settings
        n, h, w, _ = t.shape
        cb = getattr(eng, f.bound)(h, w, *ex)
        stride = (cb + 517 + 3) // 4 * 4
        out = torch.full((n, stride), GUARD, dtype=torch.uint8, device="cuda")
        lens = torch.zeros(n, dtype=torch.int64, device="cuda") if f.counted else None
        rc = getattr(eng._lib, f.device + (f.ex if ex else ""))(eng._h, ctypes.c_void_p(t.data_ptr()), n, h, w, t.stride(1), t.stride(0), ctypes.c_void_p(out.data_ptr()), stride,
                                                                 *([ctypes.c_void_p(lens.data_ptr())] if f.counted else []), *ex, ctypes.c_void_p(stream.cuda_stream))
        if rc != 0:
            raise Verdict("%s: %s" % (f.device, eng._lib.ire_last_error()))
        return out, lens, cb

    def window_case(px):
        want = _once(lambda: models(px))

        def run():
            tw, tt = window(px[None]), window(tiny[None])
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            calls = [device_call(fmt, st, tw, s) for fmt, st, _ in SEQ] + [device_call("png", None, tt, s)]      # one stream, no wait between
            s.synchronize()
            got, guards = [], []
            for out, lens, cb in calls:
                host = out.cpu().numpy()[0]
                n = int(lens[0]) if lens is not None else cb
                got.append(host[:n].tobytes())
                guards.append(bool((host[n:] == GUARD).all()))
            return got + [guards], want() + [[True] * len(calls)]
        return run

    def host_case(px):
        want = _once(lambda: models(px))

        def run():
            return [eng.encode_png_base64_fit(px), eng.encode_png_deflate_base64_fit(px), eng.encode_jpeg_base64_fit(px, 85, 0, optimize=False, progressive=False),
                    eng.encode_jpeg_base64_fit(px, 100, 2, optimize=True, progressive=False), eng.encode_jpeg_base64_fit(px, 1, 0, progressive=True),
                    eng.encode_png_base64_fit(tiny)], want()
        return run
    images = [("cells2 33x130", np.array(oc.pixels("cells2", (33, 130)))), ("flat 16x24", hc.flat()), ("noise 45x37", hc.noise(45, 37, 13))]
    cases = [("window entry " + n, window_case(px)) for n, px in images] + [("host entry " + n, host_case(px)) for n, px in images]

    fib = hc.synthetic_histograms()["fib30"]
    bits, vals, _ = huffopt.gen_optimal_table(fib)
    want_bv = np.zeros((4, 272), np.uint8)
    want_bv[:, :16], want_bv[:, 16:16 + len(vals)] = bits, vals

    def table_kernel():
        bv, nv = eng.debug_jpeg_huffman(np.stack([fib] * 4).astype(np.uint32)[None])
        return [bv.reshape(4, 272), nv.reshape(4)], [want_bv, np.full(4, len(vals), np.int32)]
    cases.append(("table kernel on fib30", table_kernel))
    name = progenc_cases.NAMES[0]
    h, w, q, s, flat = progenc_cases.case(name)
    want_file = progenc_cases.want(name)[0]
    cases.append(("progressive from coefficients", lambda: (eng.debug_jpeg_progressive_from_coefs(np.stack([flat, flat]), h, w, q, s), [want_file, want_file])))

    assert [n for n, _ in cases] == NAMES["B"], [n for n, _ in cases]
    try:
        _drive(eng, cases, result)
    finally:
        eng.close()


def _child_c(result):
    import torch
    import classifier_cases as cc
    import icc_cases
    import icc_model
    from image_restoration_platform_amd import synth, weights
    from image_restoration_platform_amd.engine import Engine, icc_plan_profile
    from oracle import classifier as ocl
    from oracle import fusion as ofu
    from oracle import layer_check as lc
    from oracle import preprocess as opp
    w0 = weights.generate(0)
    imgs = synth.batch(1, 72, 136, start=11)
    sc = np.stack([ocl.classify(im, True)[0] for im in imgs])
    switch_vars = sorted({k for env in SWITCHES for k in env} | {k for _, _, env in CHECKED for k in env})

    def engine_with(env, precision="bf16", **kw):
        for k in switch_vars:
            os.environ.pop(k, None)
        os.environ.update(env)          # the switches are read once per engine
        return Engine(device_index=0, max_batch=8, num_streams=1, precision=precision, **kw)

    def up_mode(env):
        return "plain" if env.get("IRE_UP_SUBPIX") == "0" else "subpix" if env.get("IRE_UP_FUSE") == "0" else "fused"

    def network_case(eng, label, fp8, mode):
        """the teacher-forced check of every layer on the first run; afterwards the pixels and every captured tensor equal to that run's"""
        first = []

        def run():
            eng.debug_capture(True)
            try:
                out = eng.restore(imgs, scores=sc)
                names = [nm for nm in lc.layer_names(mode) if nm != "pixels"]
                got = [out] + [eng.activation(nm) for nm in names]
                if not first:
                    try:
                        reports = lc.assert_network(w0, imgs, sc, eng.activation, out, fp8=fp8, up_mode=mode, label="poison " + label)
                    except AssertionError as e:
                        raise Verdict(str(e))
                    if set(reports) != set(lc.layer_names(mode)):
                        raise Verdict("a layer was exempt")
                    first.append(got)
            finally:
                eng.debug_capture(False)
            return got, first[0]
        return run

    def pixels_case(eng):
        first = []

        def run():
            out = eng.restore(imgs, scores=sc)
            if not first:
                first.append(out.copy())
            return [out], first
        return run

    # one engine per family, each through all four stages before the next is made
    for label, precision, env in CHECKED[1:]:
        eng = engine_with(env, precision)
        try:
            _drive(eng, [("network " + label, network_case(eng, label, precision == "fp8", up_mode(env)))], result)
        finally:
            eng.close()
    for env in OTHERS:
        eng = engine_with(env)
        try:
            _drive(eng, [("pixels " + _sw_id(env), pixels_case(eng))], result)
        finally:
            eng.close()

    eng = engine_with({}, upload_icc=True)
    cases = [("network default", network_case(eng, "default", False, "fused"))]

    def fit_case(h, w):
        x = synth.image(7, max(h, 8), max(w, 8))[:h, :w][None].copy()
        H, W = max(16, -(-h // 8) * 8), max(16, -(-w // 8) * 8)
        padded = np.pad(x, ((0, 0), (0, H - h), (0, W - w), (0, 0)), mode="edge")
        want = _once(lambda: eng.restore(padded, scores=np.stack([ocl.classify(x[0], True)[0]]))[:, :h, :w].copy())      # (restore: held by the layer check above)
        return lambda: ([eng.restore_fit(x)], [want()])
    cases += [("restore_fit 50x70", fit_case(50, 70)), ("restore_fit 9x131", fit_case(9, 131))]
    big = synth.image(9, 384, 264)
    want_big = _once(lambda: eng.restore(big[None])[0].copy())

    def strips():
        out = eng.restore_tiled_tensor(torch.from_numpy(big).cuda(), 3)
        torch.cuda.synchronize()
        return [out.cpu().numpy()], [want_big()]
    cases.append(("strips 384x264 in 3", strips))
    cimgs = cc.mixed_batch(3, 40, 515, seed=40515, first=1)
    jp = np.array([1, 0, 1], np.uint8)
    ref = cc.oracle(("poison", 40, 515), cimgs, jp)

    def classify():
        scores, labels = eng.classify(cimgs, is_jpeg=jp)
        sums = eng.classifier_sums(3)
        return ([scores, labels.astype(np.int32), sums.astype(np.uint64)],
                [np.stack([np.asarray(s, np.float64) for s, _, _ in ref]), np.array([l for _, l, _ in ref], np.int32), np.array([su for _, _, su in ref], np.uint64)])
    cases.append(("classify 3x40x515", classify))
    rng = np.random.default_rng(301777)
    stored = rng.integers(0, 256, (301, 777, 3), dtype=np.uint8)
    want_pp = opp.preprocess_pixels(stored, 6, 256)[0]
    cases.append(("preprocess 301x777 orientation 6 -> 256", lambda: ([eng.preprocess(stored, orientation=6, max_dim=256)], [want_pp])))
    batch = np.random.default_rng(13197).integers(0, 256, (3, 97, 131, 3), dtype=np.uint8)
    want_b = np.stack([opp.preprocess_pixels(im, 3, 64)[0] for im in batch])

    def pp_batch():
        out = eng.preprocess_batch(torch.from_numpy(batch).cuda(), orientation=3, max_dim=64)
        torch.cuda.synchronize()
        return [out.cpu().numpy()], [want_b]
    cases.append(("preprocess batch 131x97 -> 64", pp_batch))

    def fuse_case(hw):
        views = synth.fusion_views(hw, hw)
        want = _once(lambda: ofu.fuse(views, 0.37))
        return lambda: (list(eng.fuse(views, noise_score=0.37)), [want()[0], np.asarray(want()[1], np.int32)])
    cases += [("fuse k=3 64x64", fuse_case(64)), ("fuse k=3 128x128", fuse_case(128)), ("fuse k=3 64x64 again", fuse_case(64))]
    profiles = [icc_cases.rgb_profiles()[n] for n in ("p3_v4", "adobe_v2")]
    plans = [icc_plan_profile(p, 3) for p in profiles]
    assert all(why is None for _, why in plans)
    px = np.random.default_rng(5).integers(0, 256, (2, 33, 31, 3), dtype=np.uint8)
    want_icc = np.stack([icc_model.apply(icc_model.plan_profile(p, 3), px[i]) for i, p in enumerate(profiles)]).astype(np.uint8)
    cases.append(("to_srgb two profiles", lambda: ([eng.icc_to_srgb(px, [t for t, _ in plans])], [want_icc])))
    try:
        _drive(eng, cases, result)
    finally:
        eng.close()
    order = {n: i for i, n in enumerate(NAMES["C"])}
    assert sorted({r["name"] for r in result["records"]}, key=order.get) == NAMES["C"]


def _child_d(result):
    import icc_cases
    import icc_model
    import icc_writer
    import jpeg_decode_cases as jc
    import jpeg_decode_model as jm
    import jpeg_decode_window_cases as wcases
    import jpeg_progenc_model as progenc
    import png_cases as pc
    import png_depth_cases as pd
    import upload_cases as uc
    from image_restoration_platform_amd import _lib, synth
    from image_restoration_platform_amd.engine import Engine, EngineError
    from oracle import preprocess as opp
    from test_fusion_jobs_gpu import _reference, _views
    decode = _lib.IRE_FLAG_DECODE_PNG | _lib.IRE_FLAG_DECODE_PNG_ALL | _lib.IRE_FLAG_DECODE_PROGRESSIVE | _lib.IRE_FLAG_UPLOAD_ICC
    text = Engine(device_index=0, max_batch=4, flags=_lib.IRE_FLAG_RESULT_JPEG | _lib.IRE_FLAG_JPEG_PROGRESSIVE | decode)
    pix = Engine(device_index=0, max_batch=4, flags=decode)
    try:
        fit_a, fit_b = synth.image(3, 50, 70), synth.image(4, 16, 131)[:9]
        base = jc.encode(jc.smooth(48, 64, 57), 95, 2)
        progf = writer.pillow_progressive(jc.noise(47, 33, 8), 85, 2)
        up_jpeg = uc.encode(uc.smooth(97, 131, 138), 85, 2, 6, False)
        up_png = pc.make(40, 48, 2, seed=21)
        up_png16 = pd.make(100, 150, 6, 16, 1, smooth=True, seed=11)
        p3 = icc_cases.rgb_profiles()["p3_v4"]
        up_icc = icc_writer.tag(icc_cases.stored_file(3), p3)
        views = _views(70, 90, 2)
        good2, variants = wcases.corrupted_two_window_files(40)

        def corrupt(d):
            try:
                jm.coefficients(jm.plan(d))
            except jm.Corrupt:
                return True
            except jm.Refused:
                return False
            return False
        bad = next(d for _, d in variants if corrupt(d))

        def fitted(px, data, max_dim):
            """the oracle's preprocess of decoded pixels, by the orientation the engine's plan read from the file"""
            return opp.preprocess_pixels(px, text.upload_plan(data, max_dim)[2], max_dim)[0]
        # the pixels every job has to deliver: restore_fit, on the pixel engine and before the first poison call, of the independent decode
        restored = lambda px, is_jpeg=True: pix.restore_fit(np.ascontiguousarray(px), is_jpeg=is_jpeg)[0]      # noqa: E731
        ref = {
            "fit 50x70": restored(fit_a), "fit 9x131": restored(fit_b),
            "baseline file": restored(jc.pillow_pixels(base)), "progressive file": restored(jc.pillow_pixels(progf)),
            "upload 4:2:0 orientation 6": restored(fitted(uc.pillow_pixels(up_jpeg), up_jpeg, 128)),
            "upload 8-bit png": restored(fitted(pd.pil_rgb(up_png), up_png, 256), False),
            "upload 16-bit Adam7 png": restored(fitted(pd.pil_rgb(up_png16), up_png16, 256), False),
            "upload icc-tagged": restored(fitted(icc_model.apply(icc_model.plan_profile(p3, 3), uc.pillow_pixels(up_icc)).astype(np.uint8), up_icc, 16)),
            "fusion k=2 70x90": _reference(pix, 70, 90, 2),
        }
        assert text.upload_plan(up_jpeg, 128)[2] == 6
        want_text = {k: progenc.jpeg_base64(v, 85, 0) for k, v in ref.items()}      # the model's text of those pixels, once
        submits = [
            ("text engine: fit 50x70", text, lambda e: e.submit_fit(fit_a), want_text["fit 50x70"]),
            ("text engine: fit 9x131", text, lambda e: e.submit_fit(fit_b), want_text["fit 9x131"]),
            ("text engine: baseline file", text, lambda e: e.submit_jpeg(base), want_text["baseline file"]),
            ("text engine: progressive file", text, lambda e: e.submit_jpeg(progf), want_text["progressive file"]),
            ("text engine: upload 4:2:0 orientation 6", text, lambda e: e.submit_upload(up_jpeg, max_dim=128), want_text["upload 4:2:0 orientation 6"]),
            ("text engine: upload 8-bit png", text, lambda e: e.submit_upload(up_png, max_dim=256), want_text["upload 8-bit png"]),
            ("text engine: upload 16-bit Adam7 png", text, lambda e: e.submit_upload(up_png16, max_dim=256), want_text["upload 16-bit Adam7 png"]),
            ("text engine: upload icc-tagged", text, lambda e: e.submit_upload(up_icc, max_dim=16), want_text["upload icc-tagged"]),
            ("text engine: fusion k=2 70x90", text, lambda e: e.submit_fuse_fit(views), want_text["fusion k=2 70x90"]),
            ("text engine: corrupt upload", text, lambda e: e.submit_upload(bad, max_dim=2048), b"invalid: corrupt JPEG data"),
            ("pixel engine: fit 50x70", pix, lambda e: e.submit_fit(fit_a), ref["fit 50x70"]),
            ("pixel engine: upload 4:2:0 orientation 6", pix, lambda e: e.submit_upload(up_jpeg, max_dim=128), ref["upload 4:2:0 orientation 6"]),
        ]
        # the same kinds of job at other sizes: the rounds alternate between the two sets, so every slot's staging is reused smaller and
        # regrown behind every fill
        fit_c, fit_d = synth.image(5, 24, 40), synth.image(6, 130, 24)[:, :20].copy()
        base2 = jc.encode(jc.smooth(80, 96, 58), 90, 0)
        progf2 = writer.pillow_progressive(jc.noise(13, 17, 9), 85, 2)
        up_jpeg2 = uc.encode(uc.smooth(257, 300, 307), 85, 0, 6, False)
        up_png2 = pc.make(24, 20, 6, seed=22)
        up_png16b = pd.make(33, 70, 6, 16, 1, smooth=True, seed=12)
        adobe = icc_cases.rgb_profiles()["adobe_v2"]
        up_icc2 = icc_writer.tag(icc_cases.stored_file(4, w=56, h=32), adobe)
        views3 = _views(64, 64, 3)
        ref2 = {
            "fit 24x40": restored(fit_c), "fit 130x20": restored(fit_d),
            "baseline file 96x80": restored(jc.pillow_pixels(base2)), "progressive file 17x13": restored(jc.pillow_pixels(progf2)),
            "upload 4:4:4 300x257": restored(fitted(uc.pillow_pixels(up_jpeg2), up_jpeg2, 128)),
            "upload 8-bit rgba png 24x20": restored(fitted(pd.pil_rgb(up_png2), up_png2, 256), False),
            "upload 16-bit Adam7 png 33x70": restored(fitted(pd.pil_rgb(up_png16b), up_png16b, 256), False),
            "upload icc-tagged 56x32": restored(fitted(icc_model.apply(icc_model.plan_profile(adobe, 3), uc.pillow_pixels(up_icc2)).astype(np.uint8), up_icc2, 32)),
            "fusion k=3 64x64": _reference(pix, 64, 64, 3),
        }
        want2 = {k: progenc.jpeg_base64(v, 85, 0) for k, v in ref2.items()}
        second = [
            ("fit 24x40", text, lambda e: e.submit_fit(fit_c)), ("fit 130x20", text, lambda e: e.submit_fit(fit_d)),
            ("baseline file 96x80", text, lambda e: e.submit_jpeg(base2)), ("progressive file 17x13", text, lambda e: e.submit_jpeg(progf2)),
            ("upload 4:4:4 300x257", text, lambda e: e.submit_upload(up_jpeg2, max_dim=128)), ("upload 8-bit rgba png 24x20", text, lambda e: e.submit_upload(up_png2, max_dim=256)),
            ("upload 16-bit Adam7 png 33x70", text, lambda e: e.submit_upload(up_png16b, max_dim=256)), ("upload icc-tagged 56x32", text, lambda e: e.submit_upload(up_icc2, max_dim=32)),
            ("fusion k=3 64x64", text, lambda e: e.submit_fuse_fit(views3)),
        ]
        second = [("second sizes, text engine: " + n, e, f, want2[n]) for n, e, f in second] + [("second sizes, pixel engine: fit 24x40", pix, lambda e: e.submit_fit(fit_c), ref2["fit 24x40"])]
        refused = "poison call refused while jobs are unpolled"
        assert ([s[0] for s in submits] + [refused] + [s[0] for s in second] + ["second sizes: " + refused, "poison call refused for a delivered, unpolled job"]) == NAMES["D"]
        msg = ("%d invalid call: ire_debug_poison_scratch while a job is queued, in flight or not yet polled" % _lib.IRE_ERR_INVALID_INPUT).encode()

        def attempt(e):
            try:
                e.debug_poison_scratch(0x77)
                return b"filled"
            except EngineError as err:
                return ("%d %s" % (err.status, err.message)).encode()

        def round_of(stage, jobs_of, refusal_name):
            """the whole round submitted before its first poll; a poison call on either engine meanwhile; every job polled"""
            order = jobs_of if stage in (None, 0x00) else jobs_of[::-1]          # the same jobs in reverse order behind 0xFF and 0x5A
            jobs = [(name, e, submit(e), want) for name, e, submit, want in order]
            refusals = [attempt(text), attempt(pix)]
            polled = {}
            for name, e, job, want in jobs:
                try:
                    polled[name] = e.poll(job, timeout_ms=120000)[0]
                except EngineError as err:
                    if err.status != _lib.IRE_ERR_INVALID_INPUT:
                        raise
                    polled[name] = b"invalid: corrupt JPEG data" if "invalid: corrupt JPEG data" in err.message else err.message.encode()
            for name, _, _, want in jobs_of:
                result["records"].append(_record(name, stage, lambda: ([polled[name]], [want])))
            result["records"].append(_record(refusal_name, stage, lambda: (refusals, [msg, msg])))

        def delivered_unpolled(stage):
            """one job alone, waited for until it is delivered (a poll with a buffer of one byte says "still pending" only of a finished job,
            and keeps it): its slot is DONE, nothing is queued or in flight.  The poison call must still be refused, and the job intact."""
            job = text.submit_fit(fit_a)
            try:
                text._poll_text(job[0], 120000, 1)
                state = b"polled with one byte"
            except EngineError as err:
                state = b"delivered and kept" if (err.status == _lib.IRE_ERR_INVALID_INPUT and "the job is still pending" in err.message) else err.message.encode()
            got = [state, attempt(text), text.poll(job, timeout_ms=120000)[0]]
            result["records"].append(_record("poison call refused for a delivered, unpolled job", stage, lambda: (got, [b"delivered and kept", msg, want_text["fit 50x70"]])))
        for stage in STAGES:
            if stage is not None:
                result["filled"].append(int(text.debug_poison_scratch(stage)))
            round_of(stage, submits, refused)
            round_of(stage, second, "second sizes: " + refused)
            delivered_unpolled(stage)
    finally:
        text.close()
        pix.close()


if __name__ == "__main__":
    res = {"records": [], "filled": []}
    t_start = time.perf_counter()
    {"A": _child_a, "B": _child_b, "C": _child_c, "D": _child_d}[sys.argv[1]](res)
    res["seconds"] = time.perf_counter() - t_start
    with open(sys.argv[2], "w") as fh:
        json.dump(res, fh)
    sys.exit(0)


# ---- the parent ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """child -> its result, or a string: why there is none"""
    tmp = tmp_path_factory.mktemp("poison")
    out, failed = {}, None
    for child in CHILDREN:
        if failed:
            out[child] = "child %s was not started: %s" % (child, failed)
            continue
        env = dict(os.environ)
        env["IRE_DEBUG_POISON"] = str(BIRTH)
        env["PYTHONPATH"] = ROOT + (os.pathsep + env["PYTHONPATH"] if env.get("PYTHONPATH") else "")
        path = str(tmp / ("child_%s.json" % child))
        t0 = time.perf_counter()
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), child, path], env=env, cwd=ROOT, capture_output=True, text=True, timeout=CHILD_TIMEOUT[child])
            if r.returncode != 0:
                failed = "child %s exited with %d:\n%s\n%s" % (child, r.returncode, r.stdout[-1500:], r.stderr[-3000:])
        except subprocess.TimeoutExpired as e:
            failed = "child %s was ended at its time limit of %d s:\n%s\n%s" % (child, CHILD_TIMEOUT[child], str(e.stdout or "")[-1500:], str(e.stderr or "")[-3000:])
        if failed:
            out[child] = failed
            continue
        with open(path) as f:
            out[child] = json.load(f)
        out[child]["wall"] = time.perf_counter() - t0
        print(r.stdout)                                                          # one POISONCASE line per record (pytest -s)
        print("POISONTIME child %s | wall %.1f s | in the child %.1f s | bytes filled per poison call %s" % (child, out[child]["wall"], out[child]["seconds"], out[child]["filled"]))
    return out


def _need(runs, child):
    if isinstance(runs[child], str):
        pytest.fail(runs[child], pytrace=False)
    return runs[child]


@pytest.mark.parametrize("child,name", [(c, n) for c in CHILDREN for n in NAMES[c]], ids=lambda v: v.replace(" ", "_"))
def test_the_result_is_the_references_whatever_the_scratch_held(runs, child, name):
    """the call on an engine born as 0xA5, then behind a fill with 0xFF, 0x00 and 0x5A: four records, every one equal to the reference,
    and the four results equal to each other"""
    recs = [r for r in _need(runs, child)["records"] if r["name"] == name]
    assert [r["byte"] for r in recs] == list(STAGES), "child %s, %s: records for the stages %s, expected %s" % (child, name, [r["byte"] for r in recs], list(STAGES))
    for r in recs:
        stage = "behind a fill with 0x%02X" % r["byte"] if r["byte"] is not None else "on the engine as it was born"
        assert r["ok"], "child %s, %s, %s: result %s differs from the reference at offset %s%s" % (child, name, stage, r["item"], r["offset"], " (%s)" % r["what"] if r["what"] else "")
    assert len({r["digest"] for r in recs}) == 1, "child %s, %s: the results of the four stages differ from each other" % (child, name)


@pytest.mark.parametrize("child", CHILDREN)
def test_every_poison_call_filled_scratch_and_no_record_is_unknown(runs, child):
    res = _need(runs, child)
    assert res["filled"] and len(res["filled"]) % len(BYTES) == 0 and all(n > 0 for n in res["filled"]), res["filled"]
    assert {r["name"] for r in res["records"]} == set(NAMES[child])
    print("POISONTIME child %s | wall %.1f s | bytes filled %s" % (child, res["wall"], res["filled"]))


def test_the_call_needs_the_variable(engine):
    """without IRE_DEBUG_POISON in the process the call is refused and says which variable it wants (a suite run under the variable by
    hand: it fills instead)"""
    from image_restoration_platform_amd import _lib
    from image_restoration_platform_amd.engine import EngineError
    v = os.environ.get("IRE_DEBUG_POISON", "")
    if v.isascii() and v.isdigit() and len(v) <= 3 and int(v) <= 255:          # csrc/buf_registry.hpp's rule: one to three decimal digits, 0..255
        assert engine.debug_poison_scratch(0) > 0
        return
    with pytest.raises(EngineError) as e:
        engine.debug_poison_scratch(0)
    assert e.value.status == _lib.IRE_ERR_INVALID_INPUT and "IRE_DEBUG_POISON" in e.value.message
    assert engine._lib.ire_debug_poison_scratch(None, 0, None) == _lib.IRE_ERR_INVALID_INPUT
