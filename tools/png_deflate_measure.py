"""profiles/png_deflate.md: characters per result, stored against deflate, for synth.batch(8, 1024, 1024) restored by the engine, and the
GPU time of both encoders for a batch of 8 and of 1 at 1024^2 (HIP events around repeated calls, median).  Prints one JSON object."""
import ctypes, json, statistics, sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from image_restoration_platform_amd import synth, _lib
from image_restoration_platform_amd.engine import Engine
eng = Engine(max_batch=8)
x = synth.batch(8, 1024, 1024)
kinds = getattr(synth, "KINDS", None)
res = eng.restore_fit(np.ascontiguousarray(x), is_jpeg=False)
stored = eng.png_base64_bytes_fit(1024, 1024)
texts = eng.encode_png_deflate_base64_fit(res)
out = {"stored_chars": stored, "bound_chars": eng.png_deflate_base64_bound(1024, 1024), "deflate_chars": [len(t) for t in texts],
       "ratio": [round(len(t) / stored, 4) for t in texts], "kinds": list(kinds) if kinds else None}
# inputs too (unrestored), for reference
out["deflate_chars_inputs"] = [len(t) for t in eng.encode_png_deflate_base64_fit(np.ascontiguousarray(x))]
t = torch.from_numpy(res).cuda()
def timeit(fn, reps=30):
    for _ in range(5): fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize(); ms.append(a.elapsed_time(b))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": reps}
out["stored_batch8_1024"] = timeit(lambda: eng.encode_png_base64_fit_tensor(t))
out["deflate_batch8_1024"] = timeit(lambda: eng.encode_png_deflate_base64_fit_tensor(t))
t1 = t[:1].contiguous()
out["stored_batch1_1024"] = timeit(lambda: eng.encode_png_base64_fit_tensor(t1))
out["deflate_batch1_1024"] = timeit(lambda: eng.encode_png_deflate_base64_fit_tensor(t1))
print(json.dumps(out))
