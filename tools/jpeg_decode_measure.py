"""profiles/jpeg_decode_device.md: the device JPEG decoder (csrc/jpeg_dec.hip) against the host decode it would replace, in one job.

Files: eight 1024^2 photographs-like images (synth.batch) as Pillow q85 files, 4:4:4 and 4:2:0, no restart markers (one long stream
each: the lane path), and the same eight as the engine's own encoder writes them (16-MCU intervals: 1024 short streams each).
Per set: the one-file entry's wall time per image (ire_decode_jpeg: what restorator.decode_image calls), the device entry's time per batch of 8 by HIP events round the call and by wall clock (host parse, staging and upload
included; the call returns when everything is enqueued, so the wall time ends at a stream synchronize), the time of each launch by
events (IRE_JPEG_DEC_TIMES=1: a second engine, its sums printed when it closes), `Image.open(...).convert("RGB")` of the same files
on one core, and the mean round count per window of the lane algorithm (tests/native/jpeg_dec_sim.cpp, the kernel's own code on the
CPU, built here with g++).  Warm-up 5, 30 repeats, median and min..max.  Never run by a test.  Prints one JSON object."""
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


def kernel_times(files):
    """a child process with IRE_JPEG_DEC_TIMES=1: the engine prints its per-launch sums when it closes"""
    code = ("import sys, pickle; sys.path.insert(0, %r)\n"
            "from image_restoration_platform_amd.engine import Engine\n"
            "import torch\n"
            "files = pickle.load(open(sys.argv[1], 'rb'))\n"
            "e = Engine(max_batch=8, weights_path=None)\n"
            "for _ in range(%d): e.decode_jpeg_device(files)\n"
            "torch.cuda.synchronize(); e.close()\n") % (ROOT, WARM + REPS)
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


eng = Engine(max_batch=8, weights_path=None)
px = np.ascontiguousarray(synth.batch(8, 1024, 1024))
sets = {"pillow_q85_444": [pillow(p, 0) for p in px], "pillow_q85_420": [pillow(p, 2) for p in px],
        "own_encoder_16mcu_intervals": [base64.b64decode(t) for t in eng.encode_jpeg_base64_fit(px)]}
out = {"device": torch.cuda.get_device_name(0), "reps": REPS, "warmup": WARM}
for name, files in sets.items():
    out[name] = {"host_pil_per_image": host_decode(files), "device": device_decode(eng, files), "device_single_entry_per_image": single_entry(eng, files), "kernels": kernel_times(files), "lane_rounds": rounds(files)}
eng.close()
print(json.dumps(out))
