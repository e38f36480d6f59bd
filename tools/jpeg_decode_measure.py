"""profiles/jpeg_decode_device.md: the device JPEG decoder (csrc/jpeg_dec.hip) against the host decode it would replace, in one job.

Files: eight 1024^2 photographs-like images (synth.batch) as Pillow q85 files, 4:4:4 and 4:2:0, no restart markers (one long stream
each: the lane path), and the same eight as the engine's own encoder writes them (16-MCU intervals: 1024 short streams each).
Per set: the one-file entry's wall time per image (ire_decode_jpeg: what restorator.decode_image calls), the device entry's time per batch of 8 by HIP events round the call and by wall clock (host parse, staging and upload
included; the call returns when everything is enqueued, so the wall time ends at a stream synchronize), the time of each launch by
events (IRE_JPEG_DEC_TIMES=1: a second engine, its sums printed when it closes), `Image.open(...).convert("RGB")` of the same files
on one core, and the mean round count per window of the lane algorithm (tests/native/jpeg_dec_sim.cpp, the kernel's own code on the
CPU, built here with g++).  Warm-up 5, 30 repeats, median and min..max.  Never run by a test.  Prints one JSON object.

`jpeg_decode_measure.py windows` (profiles/jpeg_file_jobs.md): the same three sets through two engines of THIS build made side by side,
one with IRE_JPEG_DEC_WINDOWS=0 (every long stream walked by one workgroup: the kernels as they were before the window-parallel
ones) and one with the default, their batches of 8 and their one-file calls ALTERNATED rep by rep; per-launch times of both; the
chain pass's re-decodes per window (tests/native/jpeg_dec_win_sim.cpp); host PIL in the same run.
`jpeg_decode_measure.py rate`: 64 jobs in flight of 1024^2 Pillow q85 4:4:4 files, submit_jpeg img/s against submit_fit fed by PIL
decodes on 1 and on 8 threads, alternated, 5 rounds of 192 jobs each.
`jpeg_decode_measure.py progressive`: the eight images as Pillow's PROGRESSIVE q85 files (4:4:4 and 4:2:0; libjpeg's simple progression,
10 scans -- Pillow writes no mozjpeg script) beside the baseline files of the same coefficients, on one engine created with
IRE_FLAG_DECODE_PROGRESSIVE: batches of 8 and one-file calls, the per-launch times (the `later_scans` key holds everything behind the
first level's lanes), host PIL on the same files."""
import base64, io, json, os, statistics, subprocess, sys, tempfile, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from PIL import Image
from image_restoration_platform_amd import synth
from image_restoration_platform_amd.engine import Engine

REPS, WARM = 30, 5


def pillow(px, sub):
    bio = io.BytesIO()
    Image.fromarray(px, "RGB").save(bio, format="JPEG", quality=85, subsampling=sub)
    return bio.getvalue()


def spread(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "reps": len(v)}


def host_decode(files):
    per = []
    for _ in range(WARM):
        [np.asarray(Image.open(io.BytesIO(f)).convert("RGB")) for f in files]
    for _ in range(REPS):
        t0 = time.perf_counter()
        for f in files:
            np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))
        per.append((time.perf_counter() - t0) * 1000 / len(files))
    return spread(per)


def device_decode(eng, files):
    out, status = eng.decode_jpeg_device(files)
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0] * len(files)
    ref = [np.asarray(Image.open(io.BytesIO(f)).convert("RGB")) for f in files]
    equal = all(np.array_equal(out[i].cpu().numpy(), ref[i]) for i in range(len(files)))
    ev, wall = [], []
    for k in range(WARM + REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        eng.decode_jpeg_device(files, out_u8=out)
        b.record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if k >= WARM:
            ev.append(a.elapsed_time(b))
            wall.append((t1 - t0) * 1000)
    n = len(files)
    return {"equal_to_pillow": equal, "events_per_batch": spread(ev), "wall_per_batch": spread(wall),
            "wall_per_image_ms": round(statistics.median(wall) / n, 4), "file_bytes": [len(f) for f in files]}


def single_entry(eng, files):
    """ire_decode_jpeg, the synchronous one-file entry behind restorator.decode_image: wall time per image, plan and parse included"""
    per = []
    for k in range(2 + 10):
        t0 = time.perf_counter()
        for f in files:
            eng.decode_jpeg(f)
        if k >= 2:
            per.append((time.perf_counter() - t0) * 1000 / len(files))
    return spread(per)


def kernel_times(files, flags=0):
    """a child process with IRE_JPEG_DEC_TIMES=1: the engine prints its per-launch sums when it closes"""
    code = ("import sys, pickle; sys.path.insert(0, %r)\n"
            "from image_restoration_platform_amd.engine import Engine\n"
            "import torch\n"
            "files = pickle.load(open(sys.argv[1], 'rb'))\n"
            "e = Engine(max_batch=8, weights_path=None, flags=%d)\n"
            "for _ in range(%d): e.decode_jpeg_device(files)\n"
            "torch.cuda.synchronize(); e.close()\n") % (ROOT, flags, WARM + REPS)
    import pickle
    with tempfile.NamedTemporaryFile(suffix=".pkl", delete=False) as f:
        pickle.dump(files, f)
    r = subprocess.run([sys.executable, "-c", code, f.name], capture_output=True, text=True, env=dict(os.environ, IRE_JPEG_DEC_TIMES="1"), timeout=300)
    os.unlink(f.name)
    for line in r.stderr.splitlines():
        if line.startswith('{"jpeg_dec_kernel_ms"'):
            d = json.loads(line)["jpeg_dec_kernel_ms"]
            calls = d.pop("calls")
            return {k: round(v / calls, 4) for k, v in d.items()} | {"calls": calls, "unit": "mean ms per batch"}
    return {"error": (r.stderr or r.stdout)[-500:]}


def rounds(files):
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "sim")
        r = subprocess.run(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tests", "native", "jpeg_dec_sim.cpp"), "-o", exe], capture_output=True, text=True)
        if r.returncode:
            return {"error": r.stderr[-300:]}
        tot_r = tot_w = longest = 0
        for f in files:
            p = os.path.join(tmp, "f.jpg")
            open(p, "wb").write(f)
            o = subprocess.run([exe, "dump", p, os.path.join(tmp, "o.bin")], capture_output=True, text=True).stdout.splitlines()[1].split()
            d = dict(zip(o[0::2], map(int, o[1::2])))
            tot_r += d["rounds"]; tot_w += d["windows"]; longest = max(longest, d["longest"])
        return {"windows": tot_w, "mean_rounds_per_window": round(tot_r / tot_w, 2) if tot_w else None, "longest": longest}


def make_sets(eng):
    px = np.ascontiguousarray(synth.batch(8, 1024, 1024))
    return {"pillow_q85_444": [pillow(p, 0) for p in px], "pillow_q85_420": [pillow(p, 2) for p in px],
            "own_encoder_16mcu_intervals": [base64.b64decode(t) for t in eng.encode_jpeg_base64_fit(px)]}


def engine_with(windows):
    if windows is None:
        os.environ.pop("IRE_JPEG_DEC_WINDOWS", None)
    else:
        os.environ["IRE_JPEG_DEC_WINDOWS"] = windows
    e = Engine(max_batch=8, weights_path=None)
    os.environ.pop("IRE_JPEG_DEC_WINDOWS", None)
    return e


def alternated(engines, files):
    """{name: engine}: batches of 8 by wall clock and one-file calls per image, the engines taking turns rep by rep"""
    outs = {k: e.decode_jpeg_device(files)[0] for k, e in engines.items()}
    torch.cuda.synchronize()
    ref = [np.asarray(Image.open(io.BytesIO(f)).convert("RGB")) for f in files]
    res = {k: {"equal_to_pillow": all(np.array_equal(outs[k][i].cpu().numpy(), ref[i]) for i in range(len(files)))} for k in engines}
    wall = {k: [] for k in engines}
    single = {k: [] for k in engines}
    for rep in range(WARM + REPS):
        for k, e in engines.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e.decode_jpeg_device(files, out_u8=outs[k])
            torch.cuda.synchronize()
            if rep >= WARM:
                wall[k].append((time.perf_counter() - t0) * 1000)
    for rep in range(2 + 10):
        for k, e in engines.items():
            t0 = time.perf_counter()
            for f in files:
                e.decode_jpeg(f)
            if rep >= 2:
                single[k].append((time.perf_counter() - t0) * 1000 / len(files))
    for k in engines:
        res[k]["wall_per_batch"] = spread(wall[k])
        res[k]["single_entry_per_image"] = spread(single[k])
    return res


def kernel_times_env(files, windows):
    if windows is not None:
        os.environ["IRE_JPEG_DEC_WINDOWS"] = windows
    try:
        return kernel_times(files)
    finally:
        os.environ.pop("IRE_JPEG_DEC_WINDOWS", None)


def chain_redecodes(files):
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "wsim")
        r = subprocess.run(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tests", "native", "jpeg_dec_win_sim.cpp"), "-o", exe], capture_output=True, text=True)
        if r.returncode:
            return {"error": r.stderr[-300:]}
        per = []
        for f in files:
            p = os.path.join(tmp, "f.jpg")
            open(p, "wb").write(f)
            o = subprocess.run([exe, "dump", p, os.path.join(tmp, "o.bin")], capture_output=True, text=True).stdout.splitlines()[1].split()
            if o[5] != "-":
                per.append([int(v) for v in o[5].split(",")])
        flat = [v for w in per for v in w]
        return {"windows_per_file": [len(w) for w in per], "redecodes_total": sum(flat), "most_in_one_window": max(flat) if flat else 0}


def run_windows():
    engines = {"one_workgroup_per_stream": engine_with("0"), "window_parallel": engine_with(None)}
    sets = make_sets(engines["window_parallel"])
    out = {"device": torch.cuda.get_device_name(0), "reps": REPS, "warmup": WARM}
    for name, files in sets.items():
        out[name] = {"host_pil_per_image": host_decode(files), "alternated": alternated(engines, files),
                     "kernels_one_workgroup_per_stream": kernel_times_env(files, "0"), "kernels_window_parallel": kernel_times_env(files, None),
                     "chain": chain_redecodes(files)}
    # the threshold: the smallest streams the new path takes (2 and 3 windows), one file per call, both engines alternated
    r = np.random.default_rng(7)
    for side in (128, 192, 384):
        bio = io.BytesIO()
        Image.fromarray(r.integers(0, 256, (side, side, 3), dtype=np.uint8), "RGB").save(bio, format="JPEG", quality=95, subsampling=0)
        f = bio.getvalue()
        out["noise_%d_q95_one_file" % side] = {"file_bytes": len(f), "alternated": alternated(engines, [f]), "chain": chain_redecodes([f])}
    for e in engines.values():
        e.close()
    print(json.dumps(out))


def run_rate():
    from concurrent.futures import ThreadPoolExecutor
    eng = Engine(max_batch=8)
    px = np.ascontiguousarray(synth.batch(8, 1024, 1024))
    files = [pillow(p, 0) for p in px]
    total, depth = 192, 64

    def pil(f):
        return np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))

    def drive(submit):
        """`depth` jobs in flight, `total` jobs: img/s"""
        q = []
        t0 = time.perf_counter()
        for k in range(total):
            if len(q) >= depth:
                eng.poll(q.pop(0))
            q.append(submit(files[k % 8]))
        for j in q:
            eng.poll(j)
        return total / (time.perf_counter() - t0)

    def drive_pil(threads):
        with ThreadPoolExecutor(threads) as ex:
            q = []
            t0 = time.perf_counter()
            decoded = ex.map(pil, (files[k % 8] for k in range(total)))
            for rgb in decoded:
                if len(q) >= depth:
                    eng.poll(q.pop(0))
                q.append(eng.submit_fit(rgb, is_jpeg=True))
            for j in q:
                eng.poll(j)
            return total / (time.perf_counter() - t0)

    ways = {"submit_jpeg": lambda: drive(eng.submit_jpeg), "submit_fit_pil_1_thread": lambda: drive_pil(1), "submit_fit_pil_8_threads": lambda: drive_pil(8)}
    same = np.array_equal(eng.poll(eng.submit_jpeg(files[0]))[0], eng.poll(eng.submit_fit(pil(files[0]), is_jpeg=True))[0])
    rates = {k: [] for k in ways}
    for rnd in range(1 + 5):
        for k, fn in ways.items():
            v = fn()
            if rnd:
                rates[k].append(v)
    out = {"device": torch.cuda.get_device_name(0), "jobs_in_flight": depth, "jobs_per_round": total, "rounds": 5, "file_bytes": [len(f) for f in files],
           "result_equal_to_pixel_job": bool(same)}
    for k, v in rates.items():
        out[k] = {"median_img_s": round(statistics.median(v), 1), "min_img_s": round(min(v), 1), "max_img_s": round(max(v), 1)}
    eng.close()
    print(json.dumps(out))


def run_progressive():
    from PIL import ImageFile
    from image_restoration_platform_amd import _lib
    flag = _lib.IRE_FLAG_DECODE_PROGRESSIVE
    eng = Engine(max_batch=8, weights_path=None, flags=flag)
    px = np.ascontiguousarray(synth.batch(8, 1024, 1024))

    def prog(p, sub):
        bio = io.BytesIO()
        old, ImageFile.MAXBLOCK = ImageFile.MAXBLOCK, 1 << 24          # (large scans: "Suspension not allowed here" otherwise)
        try:
            Image.fromarray(p, "RGB").save(bio, format="JPEG", quality=85, subsampling=sub, progressive=True)
        finally:
            ImageFile.MAXBLOCK = old
        return bio.getvalue()
    sets = {"progressive_q85_444": [prog(p, 0) for p in px], "baseline_q85_444": [pillow(p, 0) for p in px],
            "progressive_q85_420": [prog(p, 2) for p in px], "baseline_q85_420": [pillow(p, 2) for p in px]}
    out = {"device": torch.cuda.get_device_name(0), "reps": REPS, "warmup": WARM}
    for name, files in sets.items():
        out[name] = {"host_pil_per_image": host_decode(files), "device": device_decode(eng, files), "device_single_entry_per_image": single_entry(eng, files),
                     "kernels": kernel_times(files, flag)}
    eng.close()
    print(json.dumps(out))


if len(sys.argv) > 1 and sys.argv[1] == "progressive":
    run_progressive()
    sys.exit(0)
if len(sys.argv) > 1 and sys.argv[1] == "windows":
    run_windows()
    sys.exit(0)
if len(sys.argv) > 1 and sys.argv[1] == "rate":
    run_rate()
    sys.exit(0)

eng = Engine(max_batch=8, weights_path=None)
px = np.ascontiguousarray(synth.batch(8, 1024, 1024))
sets = {"pillow_q85_444": [pillow(p, 0) for p in px], "pillow_q85_420": [pillow(p, 2) for p in px],
        "own_encoder_16mcu_intervals": [base64.b64decode(t) for t in eng.encode_jpeg_base64_fit(px)]}
out = {"device": torch.cuda.get_device_name(0), "reps": REPS, "warmup": WARM}
for name, files in sets.items():
    out[name] = {"host_pil_per_image": host_decode(files), "device": device_decode(eng, files), "device_single_entry_per_image": single_entry(eng, files), "kernels": kernel_times(files), "lane_rounds": rounds(files)}
eng.close()
print(json.dumps(out))
