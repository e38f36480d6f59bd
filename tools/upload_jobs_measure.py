"""Measurements behind profiles/upload_jobs.md (run on the MI355X; a run without a GPU fails):

  1. the preprocess of a phone photograph, 4032 x 3024 stored -> fitted inside 2048, orientations 1 and 6, n = 1 and 8 images:
     ire_preprocess_device called n times (the single-image entry, unchanged since it was written) against ONE
     ire_preprocess_batch_device call, per image, device events around `reps` repetitions, the two alternating, three rounds;
  2. 64 such uploads (EXIF orientation 6, 4:2:0, quality 85) through ire_submit_upload against the same 64 through the host: PIL
     decode + ire_preprocess + ire_submit_fit; wall clock from the first submit to the last poll, the two alternating.

    python tools/upload_jobs_measure.py [--out FILE] [--reps 20] [--uploads 64]
"""
import argparse
import ctypes
import io
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--uploads", type=int, default=64)
    args = ap.parse_args()
    import torch
    from PIL import Image
    import upload_cases as uc
    from image_restoration_platform_amd.engine import Engine
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing here can be measured without one")
    eng = Engine(max_batch=8)
    lib, W, H, MAX_DIM = eng._lib, 4032, 3024, 2048
    res = {"stored": [W, H], "max_dim": MAX_DIM, "reps": args.reps, "preprocess": [], "uploads": {}}

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.reps

    stored = torch.randint(0, 256, (8, H, W, 3), dtype=torch.uint8, device="cuda")
    for orientation in (1, 6):
        ow, oh, _ = eng.preprocess_plan(W, H, orientation, MAX_DIM)
        out = torch.empty((8, oh, ow, 3), dtype=torch.uint8, device="cuda")
        for n in (1, 8):
            def single():
                for i in range(n):
                    eng._check(lib.ire_preprocess_device(eng._h, ctypes.c_void_p(stored[i].data_ptr()), H, W, orientation, MAX_DIM, ctypes.c_void_p(out[i].data_ptr()), oh, ow, None))

            def batch():
                eng.preprocess_batch(stored[:n], orientation, MAX_DIM, out_u8=out[:n])
            single(); want = out[:n].clone(); out.zero_(); batch()      # warm both; the bytes are equal at the size that is timed
            torch.cuda.synchronize()
            assert torch.equal(out[:n], want)
            rounds = [(timed(single) / n, timed(batch) / n) for _ in range(3)]
            rec = {"orientation": orientation, "n": n, "single_ms_per_image": [round(a, 4) for a, _ in rounds], "batch_ms_per_image": [round(b, 4) for _, b in rounds]}
            rec["single_median"], rec["batch_median"] = round(statistics.median(rec["single_ms_per_image"]), 4), round(statistics.median(rec["batch_ms_per_image"]), 4)
            res["preprocess"].append(rec)
            print(json.dumps(rec), flush=True)
    del stored, out
    torch.cuda.empty_cache()

    px = uc.smooth(H, W, 3)
    data = uc.encode(px, 85, 2, orientation=6)
    plan = eng.upload_plan(data, MAX_DIM)
    res["uploads"].update({"count": args.uploads, "file_bytes": len(data), "plan": plan, "max_batch_for_fitted": eng.max_batch_for(plan[3], plan[4])})

    def device_path():
        jobs = [eng.submit_upload(data, MAX_DIM) for _ in range(args.uploads)]
        return [eng.poll(j)[0] for j in jobs]

    def host_path():
        jobs = []
        for _ in range(args.uploads):
            stored_px = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
            jobs.append(eng.submit_fit(eng.preprocess(stored_px, 6, MAX_DIM), is_jpeg=True))
        return [eng.poll(j)[0] for j in jobs]
    a, b = device_path()[0], host_path()[0]      # warm both
    res["uploads"]["results_equal"] = bool(np.array_equal(a, b))
    dev_s, host_s = [], []
    for _ in range(3):
        t0 = time.perf_counter(); device_path(); t1 = time.perf_counter(); host_path(); t2 = time.perf_counter()
        dev_s.append(round(t1 - t0, 4)); host_s.append(round(t2 - t1, 4))
    res["uploads"].update({"device_s": dev_s, "host_s": host_s, "device_uploads_per_s": round(args.uploads / statistics.median(dev_s), 2),
                           "host_uploads_per_s": round(args.uploads / statistics.median(host_s), 2)})
    print(json.dumps(res["uploads"]), flush=True)
    eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
