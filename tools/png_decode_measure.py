"""profiles/png_decode.md: the device PNG decoder (csrc/png_dec.hip) against the host decode it would replace, in one job.

Files: eight 1024^2 photograph-like images (synth.batch) as Pillow writes them at compress_level 6, and as tests/png_writer.py writes
them at zlib level 1 (Paeth on every row).  Per set: the device entry's time per batch of 8 and for one file alone, by HIP events round
the call and by wall clock ended at a synchronize (host parse, staging and upload included); the one-file synchronous entry
(ire_decode_png: what restorator.decode_image calls); the two kernels' times by events and lane 0's share of the inflate kernel spent
in the serial walk and in the placement (IRE_PNG_DEC_TIMES=1: a second engine in a child process, its sums printed when it closes);
`Image.open(...).convert("RGB")` of the same files on one core.
`png_decode_measure.py rate`: uploads/s through ire_submit_upload against the route such a file takes without the decoder: PIL decode +
ire_preprocess + ire_submit_fit, both with 16 jobs in flight, alternated round by round.
Warm-up and repeats as printed.  Never run by a test.  Prints one JSON object."""
import io, json, os, pickle, statistics, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
from PIL import Image
from image_restoration_platform_amd import synth
from image_restoration_platform_amd.engine import Engine
import png_writer as pw

REPS, WARM = 10, 3


def pillow(px):
    bio = io.BytesIO()
    Image.fromarray(px, "RGB").save(bio, format="PNG", compress_level=6)
    return bio.getvalue()


def pil(f):
    return np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))


def spread(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "reps": len(v)}


def host_decode(files):
    per = []
    for k in range(1 + 5):
        t0 = time.perf_counter()
        for f in files:
            pil(f)
        if k:
            per.append((time.perf_counter() - t0) * 1000 / len(files))
    return spread(per)


def device_decode(eng, files):
    out, status = eng.decode_png_device(files)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * len(files)
    equal = all(np.array_equal(out[i].cpu().numpy(), pil(f)) for i, f in enumerate(files))
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
    return {"equal_to_pillow": equal, "events_per_call": spread(ev), "wall_per_call": spread(wall), "wall_per_image_ms": round(statistics.median(wall) / len(files), 4)}


def single_entry(eng, files):
    per = []
    for k in range(1 + 4):
        t0 = time.perf_counter()
        for f in files:
            eng.decode_png(f)
        if k:
            per.append((time.perf_counter() - t0) * 1000 / len(files))
    return spread(per)


def kernel_times(files):
    code = ("import sys, pickle; sys.path.insert(0, %r)\n"
            "from image_restoration_platform_amd.engine import Engine\n"
            "import torch\n"
            "files = pickle.load(open(sys.argv[1], 'rb'))\n"
            "e = Engine(max_batch=8, weights_path=None, decode_png=True)\n"
            "for _ in range(%d): e.decode_png_device(files)\n"
            "torch.cuda.synchronize(); e.close()\n") % (ROOT, WARM + REPS)
    with tempfile.NamedTemporaryFile(suffix=".pkl", delete=False) as f:
        pickle.dump(files, f)
    r = subprocess.run([sys.executable, "-c", code, f.name], capture_output=True, text=True, env=dict(os.environ, IRE_PNG_DEC_TIMES="1"), timeout=400)
    os.unlink(f.name)
    for line in r.stderr.splitlines():
        if line.startswith('{"png_dec_kernel_ms"'):
            d = json.loads(line)["png_dec_kernel_ms"]
            calls = d.pop("calls")
            shares = {k: d.pop(k) for k in ("walk_share", "place_share")}
            return {k: round(v / calls, 4) for k, v in d.items()} | shares | {"calls": calls, "unit": "mean ms per call; shares of lane 0's time in the inflate kernel"}
    return {"error": (r.stderr or r.stdout)[-500:]}


def make_sets():
    px = np.ascontiguousarray(synth.batch(8, 1024, 1024))
    return px, {"pillow_level6": [pillow(p) for p in px], "writer_level1_paeth": [pw.png(p, 2, (4,), level=1) for p in px]}


def run_rate():
    eng = Engine(max_batch=8, decode_png=True)
    px, sets = make_sets()
    files = sets["pillow_level6"]
    total, depth = 48, 16

    def drive(submit):
        q = []
        t0 = time.perf_counter()
        for k in range(total):
            if len(q) >= depth:
                eng.poll(q.pop(0))
            q.append(submit(files[k % 8]))
        for j in q:
            eng.poll(j)
        return total / (time.perf_counter() - t0)

    ways = {"submit_upload": lambda: drive(lambda f: eng.submit_upload(f, max_dim=2048)),
            "pil_preprocess_submit_fit": lambda: drive(lambda f: eng.submit_fit(eng.preprocess(pil(f), 1, 2048), is_jpeg=False))}
    same = np.array_equal(eng.poll(eng.submit_upload(files[0], max_dim=2048))[0], eng.poll(eng.submit_fit(eng.preprocess(pil(files[0]), 1, 2048), is_jpeg=False))[0])
    rates = {k: [] for k in ways}
    for rnd in range(1 + 3):
        for k, fn in ways.items():
            v = fn()
            if rnd:
                rates[k].append(v)
    out = {"device": torch.cuda.get_device_name(0), "jobs_in_flight": depth, "jobs_per_round": total, "rounds": 3, "file_bytes": [len(f) for f in files],
           "result_equal_to_the_composed_calls": bool(same)}
    for k, v in rates.items():
        out[k] = {"median_uploads_s": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}
    eng.close()
    print(json.dumps(out))


if len(sys.argv) > 1 and sys.argv[1] == "rate":
    run_rate()
    sys.exit(0)

eng = Engine(max_batch=8, weights_path=None, decode_png=True)
px, sets = make_sets()
out = {"device": torch.cuda.get_device_name(0), "reps": REPS, "warmup": WARM}
for name, files in sets.items():
    out[name] = {"file_bytes": [len(f) for f in files], "host_pil_per_image": host_decode(files), "device_batch_of_8": device_decode(eng, files),
                 "device_one_file": device_decode(eng, files[:1]), "device_single_entry_per_image": single_entry(eng, files), "kernels_batch_of_8": kernel_times(files),
                 "kernels_one_file": kernel_times(files[:1])}
eng.close()
print(json.dumps(out))
