"""profiles/jpeg_device.md: characters per result of the device JPEG (csrc/jpeg.hip) for synth.batch(8, 1024, 1024) restored by the
engine, against libjpeg-turbo's own q85 4:4:4 file (Pillow, default settings: no restart markers) and the two device PNGs; the GPU
time of the encoder for a batch of 8 and of 1 at 1024^2 (HIP events around repeated calls, median) and the bytes it moves; the size
of a batcher place.  Prints one JSON object."""
import base64, io, json, statistics, sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from PIL import Image
from image_restoration_platform_amd import synth
from image_restoration_platform_amd.engine import Engine
eng = Engine(max_batch=8)
x = synth.batch(8, 1024, 1024)
res = eng.restore_fit(np.ascontiguousarray(x), is_jpeg=False)
texts = eng.encode_jpeg_base64_fit(res)


def pillow(px, **kw):
    bio = io.BytesIO()
    Image.fromarray(px, "RGB").save(bio, format="JPEG", quality=85, subsampling=0, **kw)
    return bio.getvalue()


def psnr(a, b):
    return float(10 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


own = [pillow(r) for r in res]
same = [pillow(r, optimize=False, restart_marker_blocks=16) for r in res]
dec = [np.asarray(Image.open(io.BytesIO(base64.b64decode(t))).convert("RGB")) for t in texts]
out = {"jpeg_chars": [len(t) for t in texts], "bound_chars": eng.jpeg_base64_bound(1024, 1024), "place_bytes": 8 + eng.jpeg_base64_bound(1024, 1024),
       "pillow_q85_chars": [(len(f) + 2) // 3 * 4 for f in own], "equal_to_pillow_with_restart_16": [base64.b64encode(f) == t for f, t in zip(same, texts)],
       "psnr_device_db": [round(psnr(d, r), 2) for d, r in zip(dec, res)],
       "psnr_pillow_db": [round(psnr(np.asarray(Image.open(io.BytesIO(f)).convert("RGB")), r), 2) for f, r in zip(own, res)],
       "stored_png_chars": eng.png_base64_bytes_fit(1024, 1024), "deflate_png_chars": [len(t) for t in eng.encode_png_deflate_base64_fit(res)],
       "verdict_target_chars": 1300000}
t = torch.from_numpy(res).cuda()


def timeit(fn, reps=30):
    for _ in range(5): fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize(); ms.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": reps}


out["jpeg_batch8_1024"] = timeit(lambda: eng.encode_jpeg_base64_fit_tensor(t))
out["deflate_batch8_1024"] = timeit(lambda: eng.encode_png_deflate_base64_fit_tensor(t))
out["stored_batch8_1024"] = timeit(lambda: eng.encode_png_base64_fit_tensor(t))
t1 = t[:1].contiguous()
out["jpeg_batch1_1024"] = timeit(lambda: eng.encode_jpeg_base64_fit_tensor(t1))
# bytes the three kernels move for the batch of 8: pixels in; interval bytes out, in and out again; the file in, the text out
files = sum((len(tx) // 4) * 3 for tx in texts)
out["bytes_moved_batch8"] = 8 * 3 * 1024 * 1024 + 3 * files + sum(len(tx) for tx in texts)
print(json.dumps(out))
