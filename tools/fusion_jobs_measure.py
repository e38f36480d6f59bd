"""profiles/fusion_jobs.md: one fusion job of three 1024^2 views end to end -- the caller's three pixel buffers in, the result in the
caller's buffer out -- as the new batcher job (Engine.submit_fuse_fit + poll) and as the composition restore_image used before it
(`legacy` below: only entry points that existed then -- k x submit, k x poll, on a text engine a host decode of every view, ire_fuse,
on a text engine the encode).  On a pixel engine and on an IRE_FLAG_RESULT_JPEG engine; the two ways alternated run by run in one
process; then five concurrent callers (the worker's concurrency), the two ways alternated phase by phase.

  python tools/fusion_jobs_measure.py [--runs 24] [--warmup 3] [--size 1024]          -> one JSON object (times in ms, host clock
                                                                                         around calls that end with the result on the host)
  python tools/fusion_jobs_measure.py --count new|legacy --engine pixel|jpeg --jobs N  -> runs N jobs and exits: for a profiler's
                                                                                         kernel and memory-copy statistics (two values of N:
                                                                                         their difference is the per-job count)
  python tools/fusion_jobs_measure.py --service pixel|jpeg [--tree DIR]                 -> EngineRestorer.restore_image with three PNG uploads
                                                                                         in ONE process lifetime, of the checkout at DIR
                                                                                         (default: this one; a checkout of the parent commit
                                                                                         built beside it gives the other column): one caller,
                                                                                         then five.  `seen`: analyze() ran on every upload
                                                                                         before the clock started, as the service does (no
                                                                                         host decode inside); `cold`: it did not
  python tools/fusion_jobs_measure.py --sum-calls DIR                                   -> total "Calls" of the kernel and memory-copy
                                                                                         statistics CSVs below DIR
"""
import argparse
import base64
import csv
import glob
import io
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sum_calls(root):
    out = {}
    for kind in ("kernel_stats", "memory_copy_stats"):
        n = 0
        for path in glob.glob(os.path.join(root, "**", "*%s.csv" % kind), recursive=True):
            n += sum(int(r["Calls"]) for r in csv.DictReader(open(path)))
        out[kind] = n
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--count", choices=["new", "legacy"])
    ap.add_argument("--engine", choices=["pixel", "jpeg"], default="pixel")
    ap.add_argument("--jobs", type=int, default=1)
    ap.add_argument("--sum-calls")
    ap.add_argument("--service", choices=["pixel", "jpeg"])
    ap.add_argument("--tree", default=ROOT)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    if a.sum_calls:
        print(json.dumps(sum_calls(a.sum_calls)))
        return

    import numpy as np
    from PIL import Image
    from image_restoration_platform_amd import _lib, synth
    from image_restoration_platform_amd.engine import Engine

    views = synth.fusion_views(a.size, a.size)
    for v in views:
        v.setflags(write=False)

    def new_job(eng, text):
        out, _, _ = eng.poll(eng.submit_fuse_fit(views))
        return out

    def legacy_job(eng, text):
        # restore_image's multi-view branch as it was: every view its own batcher job, the fusion a second trip through the host
        jobs = [eng.submit(v) for v in views]
        restored = []
        for j in jobs:
            out, _, _ = eng.poll(j)
            if text:
                out = np.asarray(Image.open(io.BytesIO(base64.b64decode(out))).convert("RGB"))
            restored.append(out)
        fused, _ = eng.fuse(np.stack(restored, axis=0), noise_score=-1.0)
        return eng.encode_jpeg_base64_fit(fused) if text else fused

    ways = {"new": new_job, "legacy": legacy_job}

    def engine_of(kind):
        return Engine(max_batch=8, flags=_lib.IRE_FLAG_RESULT_JPEG if kind == "jpeg" else 0), kind == "jpeg"

    def med(ms):
        return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "runs": len(ms)}

    if a.service:
        import hashlib
        from image_restoration_platform_amd.restorator import EngineClassifier, EngineRestorer
        eng, text = engine_of(a.service)
        rest, cls = EngineRestorer(eng, result_codec="jpeg-device" if text else "jpeg"), EngineClassifier(eng)

        def uploads():      # fresh buffers every job, as a request brings them
            ups = []
            for v in views:
                bio = io.BytesIO()
                Image.fromarray(v, "RGB").save(bio, format="PNG", compress_level=1)
                ups.append(bio.getvalue())
            return ups

        def job(seen, times):
            ups = uploads()
            if seen:
                for u in ups:
                    cls.analyze(u)
            t0 = time.perf_counter()
            res = rest.restore_image("restore", ups)
            times.append((time.perf_counter() - t0) * 1e3)
            return res["base64Image"]

        report = {"tree": os.path.abspath(a.tree), "engine": a.service, "size": a.size, "views": 3,
                  "result_sha1": hashlib.sha1(job(True, []).encode()).hexdigest()}
        for _ in range(a.warmup):
            job(True, []), job(False, [])
        lone = {"seen": [], "cold": []}
        for _ in range(a.runs):
            job(True, lone["seen"]), job(False, lone["cold"])
        conc, per_thread = [], max(4, a.runs // 4)

        def caller():
            for _ in range(per_thread):
                job(True, conc)
        th = [threading.Thread(target=caller) for _ in range(5)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        report["one_caller"] = {w: med(v) for w, v in lone.items()}
        report["five_callers_seen"] = med(conc)       # (latency inside restore_image; the callers' own decode and analyze run outside the clock)
        eng.close()
        print(json.dumps(report))
        return

    if a.count:
        eng, text = engine_of(a.engine)
        for _ in range(a.jobs):
            ways[a.count](eng, text)
        eng.close()
        return

    report = {"size": a.size, "views": 3}
    for kind in ("pixel", "jpeg"):
        eng, text = engine_of(kind)
        res = {w: fn(eng, text) for w, fn in ways.items()}
        same = (res["new"] == res["legacy"]) if text else bool(np.array_equal(res["new"], res["legacy"]))
        for _ in range(a.warmup):
            for fn in ways.values():
                fn(eng, text)
        lone = {w: [] for w in ways}
        for _ in range(a.runs):
            for w, fn in ways.items():           # alternated run by run
                t0 = time.perf_counter()
                fn(eng, text)
                lone[w].append((time.perf_counter() - t0) * 1e3)
        conc = {w: [] for w in ways}
        wall = {w: 0.0 for w in ways}
        per_thread = max(4, a.runs // 4)
        for _ in range(2):                       # alternated phase by phase
            for w, fn in ways.items():
                def caller(fn=fn, w=w):
                    for _ in range(per_thread):
                        t0 = time.perf_counter()
                        fn(eng, text)
                        conc[w].append((time.perf_counter() - t0) * 1e3)      # (list.append is atomic)
                th = [threading.Thread(target=caller) for _ in range(5)]
                t0 = time.perf_counter()
                for t in th:
                    t.start()
                for t in th:
                    t.join()
                wall[w] += time.perf_counter() - t0
        report[kind] = {"results_equal": same,
                        "one_caller": {w: med(v) for w, v in lone.items()},
                        "five_callers": {w: dict(med(v), jobs_per_s=round(len(v) / wall[w], 2)) for w, v in conc.items()}}
        eng.close()
    print(json.dumps(report))


if __name__ == "__main__":
    main()
