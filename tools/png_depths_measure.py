"""profiles/png_depths.md: the device PNG decoder (csrc/png_dec.hip) on the forms of IRE_FLAG_DECODE_PNG_ALL, by the method of
tools/png_decode_measure.py: a batch of 8 files of 1024^2 through ire_decode_png_device, 3 warm-up calls, 10 timed, median (min..max),
by HIP events round the call and by wall clock ended at a synchronize; the two kernels' times by the events between the launches
(IRE_PNG_DEC_TIMES=1: the engine prints their sums when it closes; mean per call over the 13 calls).

Forms, all of the same eight photograph-like images (synth.batch), Paeth on every row, zlib level 6:
  rgb8     8-bit RGB, not interlaced (tests/png_writer.py): the form the decoder always took
  adam7    the same pixels, Adam7
  rgba16   16-bit RGBA: every sample the 8-bit one twice (x 257), alpha 65535
  plte4    4-bit palette: the red channel's high four bits as the index of a 16-entry palette
    python tools/png_depths_measure.py [--forms rgb8,adam7,...] [--tree DIR]
--tree: another checkout of this project (built) to take the package from, for an A/B of the rgb8 form against a parent commit; the
files then come from this tree's tests/png_writer.py all the same.  One engine per form, in a process of its own.  Never run by a test.
Prints one JSON object."""
import argparse, io, json, os, pickle, statistics, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS, WARM = 10, 3

CHILD = r"""
import io, json, pickle, statistics, sys, time
sys.path.insert(0, sys.argv[2])
import numpy as np, torch
from PIL import Image
from image_restoration_platform_amd import _lib
from image_restoration_platform_amd.engine import Engine
files = pickle.load(open(sys.argv[1], "rb"))
WARM, REPS = int(sys.argv[3]), int(sys.argv[4])
flags = _lib.IRE_FLAG_DECODE_PNG | getattr(_lib, "IRE_FLAG_DECODE_PNG_ALL", 0)
eng = Engine(max_batch=8, weights_path=None, flags=flags)
out, status = eng.decode_png_device(files)
torch.cuda.synchronize()
assert status.cpu().tolist() == [0] * len(files)
equal = all(np.array_equal(out[i].cpu().numpy(), np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))) for i, f in enumerate(files))
eng.close()
eng = Engine(max_batch=8, weights_path=None, flags=flags)          # (a fresh one: its kernel sums cover the 13 calls below alone)
ev, wall = [], []
for k in range(WARM + REPS):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    eng.decode_png_device(files, out_u8=out)
    b.record()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    if k >= WARM:
        ev.append(a.elapsed_time(b))
        wall.append((t1 - t0) * 1000)
spread = lambda v: {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3), "reps": len(v)}
print(json.dumps({"equal_to_pillow": bool(equal), "events_per_call": spread(ev), "wall_per_call": spread(wall)}))
eng.close()
"""


def make_form(form, px):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import png_writer as pw
    if form == "rgb8":
        return [pw.png(p, 2, (4,), level=6) for p in px]
    import png_depth_cases as dc
    if form == "adam7":
        return [dc.png_any(p.astype(np.uint32), 2, 8, 1, (4,), level=6) for p in px]
    if form == "rgba16":
        out = []
        for p in px:
            s = np.full(p.shape[:2] + (4,), 65535, np.uint32)
            s[..., :3] = p.astype(np.uint32) * 257
            out.append(dc.png_any(s, 6, 16, 0, (4,), level=6))
        return out
    if form == "plte4":
        return [dc.png_any((p[..., :1] >> 4).astype(np.uint32), 3, 4, 0, (4,), plte=dc.palette(16), level=6) for p in px]
    raise SystemExit("unknown form " + form)


def measure(files, tree):
    with tempfile.NamedTemporaryFile(suffix=".pkl", delete=False) as f:
        pickle.dump(files, f)
    r = subprocess.run([sys.executable, "-c", CHILD, f.name, tree, str(WARM), str(REPS)], capture_output=True, text=True, env=dict(os.environ, IRE_PNG_DEC_TIMES="1"), timeout=900)
    os.unlink(f.name)
    if r.returncode != 0:
        return {"error": (r.stderr or r.stdout)[-800:]}
    out = json.loads(r.stdout.strip().splitlines()[-1])
    sums = [json.loads(l)["png_dec_kernel_ms"] for l in r.stderr.splitlines() if l.startswith('{"png_dec_kernel_ms"')]
    if sums:
        d = sums[-1]          # the second engine's
        calls = d["calls"]
        out["kernels"] = {"inflate_ms": round(d["inflate"] / calls, 3), "unfilter_ms": round(d["unfilter"] / calls, 3), "calls": calls,
                          "unfilter_share": round(d["unfilter"] / (d["inflate"] + d["unfilter"]), 4), "walk_share": d["walk_share"], "place_share": d["place_share"]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--forms", default="rgb8,adam7,rgba16,plte4")
    ap.add_argument("--tree", default=ROOT)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    from image_restoration_platform_amd import synth
    px = np.ascontiguousarray(synth.batch(8, 1024, 1024))
    out = {"tree": os.path.relpath(os.path.abspath(a.tree), ROOT), "reps": REPS, "warmup": WARM}
    for form in a.forms.split(","):
        files = make_form(form, px)
        out[form] = {"file_bytes": [len(f) for f in files]} | measure(files, os.path.abspath(a.tree))
        if "error" in out[form]:          # nothing more is started on a device whose last program failed
            print(json.dumps(out))
            sys.exit(1)
    print(json.dumps(out))


main()
