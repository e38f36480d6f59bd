"""Measurements behind profiles/upload_jobs.md (run on the MI355X; a run without a GPU fails):

  1. the preprocess of a phone photograph, 4032 x 3024 stored -> fitted inside 2048, orientations 1 and 6, n = 1 and 8 images:
     ire_preprocess_device called n times (the single-image entry, unchanged since it was written) against ONE
     ire_preprocess_batch_device call, per image, device events around `reps` repetitions, the two alternating, three rounds;
  2. 64 such uploads (EXIF orientation 6, 4:2:0, quality 85) through ire_submit_upload against the same 64 through the host: PIL
     decode + ire_preprocess + ire_submit_fit; wall clock from the first submit to the last poll, the two alternating.

    python tools/upload_jobs_measure.py [--out FILE] [--reps 20] [--uploads 64]

`upload_jobs_measure.py icc` measures what is behind profiles/upload_icc.md instead, on an engine created with IRE_FLAG_UPLOAD_ICC:

  3. the ICC conversion kernel alone: 8 images of 4032 x 3024, all Display P3, one ire_icc_to_srgb_device call, per image, beside the
     batched preprocess (orientation 6, fitted inside 2048) of the same batch, the two alternating, three rounds.  The kernel works in
     place, so its input is copied afresh from an untouched tensor before EVERY call, outside the timed window (device events around
     each single call, summed): a call never sees the output of the one before it.  Two inputs: uniform random bytes and the smooth
     photograph of the upload measurements;
  4. 64 Display-P3-tagged uploads against 64 untagged uploads of the same pixels through ire_submit_upload, alternating;
  5. with --parent ROOT (a built tree of the parent commit): untagged uploads on this tree's flagged engine against the parent's
     engine, one worker process each (`icc-worker`), one repetition at a time in turn.

    python tools/upload_jobs_measure.py icc [--out FILE] [--reps 20] [--uploads 64] [--rounds 7] [--parent ROOT] [--sections kernel,rate]
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


def photo_file():
    """the phone photograph of these measurements: 4032 x 3024 stored, EXIF orientation 6, 4:2:0, quality 85"""
    import upload_cases as uc
    return uc.encode(uc.smooth(3024, 4032, 3), 85, 2, orientation=6)


def icc_worker(args):
    """one engine of the tree at --root (flagged when that tree knows the flag and --flag is given); for every line on stdin, `uploads`
    untagged uploads from the first submit to the last poll, the seconds on stdout"""
    sys.path.insert(0, args.root)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from image_restoration_platform_amd.engine import Engine
    eng = Engine(max_batch=8, **({"upload_icc": True} if args.flag else {}))
    data = photo_file()

    def rep():
        t0 = time.perf_counter()
        jobs = [eng.submit_upload(data, 2048) for _ in range(args.uploads)]
        for j in jobs:
            eng.poll(j)
        return time.perf_counter() - t0
    rep()
    print("ready", flush=True)
    for line in sys.stdin:
        if line.strip() == "quit":
            break
        print("%.6f" % rep(), flush=True)
    eng.close()


def icc_main(args):
    import subprocess
    import torch
    import icc_writer as wr
    from image_restoration_platform_amd.engine import Engine, icc_plan_profile
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing here can be measured without one")
    W, H, MAX_DIM = 4032, 3024, 2048
    res = {"stored": [W, H], "max_dim": MAX_DIM, "reps": args.reps}
    eng = Engine(max_batch=8, upload_icc=True)

    sections = set(args.sections.split(","))
    p3 = wr.display_p3()
    t, why = icc_plan_profile(p3, 3)
    assert why is None

    def kernel_section(name, pristine):
        """`pristine` (8, H, W, 3) stays as it is; `stored` is what the calls work on, refreshed from it before every timed call"""
        stored = pristine.clone()
        flat = stored.view(-1)
        ow, oh, _ = eng.preprocess_plan(W, H, 6, MAX_DIM)
        out = torch.empty((8, oh, ow, 3), dtype=torch.uint8, device="cuda")

        def timed(fn):
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.reps)]
            torch.cuda.synchronize()
            for e0, e1 in ev:
                stored.copy_(pristine)
                e0.record()
                fn()
                e1.record()
            torch.cuda.synchronize()
            return sum(e0.elapsed_time(e1) for e0, e1 in ev) / args.reps

        def convert():
            eng.icc_to_srgb_device(flat, 8, H, W, H * W * 3, [t] * 8)

        def preprocess():
            eng.preprocess_batch(stored, 6, MAX_DIM, out_u8=out)
        stored.copy_(pristine); convert()
        torch.cuda.synchronize()
        changed = int((stored != pristine).sum().item()) / stored.numel()
        stored.copy_(pristine); preprocess()
        rounds = [(timed(convert) / 8, timed(preprocess) / 8) for _ in range(3)]
        k = {"input": name, "n": 8, "bytes_changed_by_one_call": round(changed, 4), "icc_ms_per_image": [round(a, 4) for a, _ in rounds],
             "preprocess_ms_per_image": [round(b, 4) for _, b in rounds]}
        k["icc_median"] = statistics.median(k["icc_ms_per_image"])
        k["traffic_mb_per_image"] = round(2 * H * W * 3 / 1e6, 1)
        k["icc_gb_per_s"] = round(2 * H * W * 3 / 1e9 / (k["icc_median"] / 1e3), 1)
        print(json.dumps(k), flush=True)
        return k

    if "kernel" in sections:
        import upload_cases as uc
        res["kernel"] = [kernel_section("uniform random bytes", torch.randint(0, 256, (8, H, W, 3), dtype=torch.uint8, device="cuda"))]
        torch.cuda.empty_cache()
        smooth = torch.from_numpy(np.ascontiguousarray(uc.smooth(H, W, 3))).cuda()
        res["kernel"].append(kernel_section("smooth photograph", smooth[None].repeat(8, 1, 1, 1)))
        del smooth
        torch.cuda.empty_cache()
    if "rate" not in sections:
        eng.close()
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
        return

    data = photo_file()
    tagged = wr.tag(data, p3)
    assert eng.upload_plan(tagged, MAX_DIM) == eng.upload_plan(data, MAX_DIM)

    def run(f):
        t0 = time.perf_counter()
        jobs = [eng.submit_upload(f, MAX_DIM) for _ in range(args.uploads)]
        outs = [eng.poll(j)[0] for j in jobs]
        return time.perf_counter() - t0, outs[0]
    a, b = run(tagged)[1], run(data)[1]      # warm both
    tag_s, plain_s = [], []
    for _ in range(args.rounds):
        tag_s.append(round(run(tagged)[0], 4)); plain_s.append(round(run(data)[0], 4))
    res["rate"] = {"count": args.uploads, "results_differ": bool(not np.array_equal(a, b)), "tagged_s": tag_s, "untagged_s": plain_s,
                   "tagged_uploads_per_s": round(args.uploads / statistics.median(tag_s), 2), "untagged_uploads_per_s": round(args.uploads / statistics.median(plain_s), 2)}
    print(json.dumps(res["rate"]), flush=True)
    eng.close()
    del eng

    if args.parent:
        me = os.path.abspath(__file__)
        workers = {}
        for name, root, flag in (("this", ROOT, True), ("parent", os.path.abspath(args.parent), False)):
            cmd = [sys.executable, me, "icc-worker", "--root", root, "--uploads", str(args.uploads)] + (["--flag"] if flag else [])
            w = subprocess.Popen(cmd, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True, env={k: v for k, v in os.environ.items() if k != "IRE_LIB"})
            assert w.stdout.readline().strip() == "ready", name
            workers[name] = w
        secs = {"this": [], "parent": []}
        for _ in range(args.rounds):
            for name in ("parent", "this"):
                w = workers[name]
                w.stdin.write("go\n"); w.stdin.flush()
                secs[name].append(float(w.stdout.readline()))
        for w in workers.values():
            w.stdin.write("quit\n"); w.stdin.flush(); w.wait(timeout=60)
        g = {"count": args.uploads, "rounds": args.rounds}
        for name in secs:
            r = sorted(args.uploads / s for s in secs[name])
            g[name] = {"uploads_per_s": [round(v, 2) for v in r], "median": round(statistics.median(r), 2), "spread": round(r[-1] - r[0], 2)}
        g["pass"] = bool(g["this"]["median"] >= g["parent"]["median"] - g["parent"]["spread"])
        res["gate"] = g
        print(json.dumps(g), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", nargs="?", default="", choices=["", "icc", "icc-worker"])
    ap.add_argument("--out", default="")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--uploads", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--parent", default="")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--flag", action="store_true")
    ap.add_argument("--sections", default="kernel,rate", help="icc mode: which of kernel, rate to run (the gate needs rate and --parent)")
    args = ap.parse_args()
    if args.mode == "icc-worker":
        return icc_worker(args)
    if args.mode == "icc":
        return icc_main(args)
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
