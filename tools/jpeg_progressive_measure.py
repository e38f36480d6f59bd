"""profiles/jpeg_progressive.md: the device JPEG encoder's progressive call (csrc/jpeg_progenc.hip) against the optimised call
(csrc/jpeg.hip), in one process and at the same settings.  Input: synth.batch(8, 1024, 1024), already on the device.  Method of
profiles/jpeg_huffopt.md: 20 warm-up calls, then 15 windows of 20 calls between two device events on the calls' stream; a figure is the
median over the windows, in ms per call.  Prints one JSON object.

    python tools/jpeg_progressive_measure.py               optimised and progressive at (85, 4:4:4) and (85, 4:2:0), the text lengths per
                                                           image, the public bound and the coefficient scratch
    python tools/jpeg_progressive_measure.py --base-only   the fixed-table default and the optimised call alone: also runs on a library
                                                           built before the progressive entries existed (IRE_LIB=...), for the A/B of
                                                           the untouched paths
    python tools/jpeg_progressive_measure.py --once        one progressive and one optimised call per setting, for a kernel trace"""
import ctypes, hashlib, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from image_restoration_platform_amd import _lib
NEW = ("ire_jpeg_progressive_base64_bound", "ire_encode_jpeg_progressive_base64_fit_device", "ire_encode_jpeg_progressive_base64_fit", "ire_debug_jpeg_progressive_from_coefs")
base_only, once = "--base-only" in sys.argv, "--once" in sys.argv
if base_only:
    for name in NEW:
        _lib.SYMBOLS.pop(name, None)
import torch
from image_restoration_platform_amd import synth
from image_restoration_platform_amd.engine import Engine

eng = Engine(max_batch=8)
lib = eng._lib
x = torch.from_numpy(synth.batch(8, 1024, 1024)).cuda()
n, h, w, _ = x.shape
stream = torch.cuda.current_stream()


def caller(entry, bound, *settings):
    stride = (bound + 3) // 4 * 4
    out = torch.empty((n, stride), dtype=torch.uint8, device="cuda")
    lens = torch.zeros(n, dtype=torch.int64, device="cuda")

    def call():
        st = entry(eng._h, ctypes.c_void_p(x.data_ptr()), n, h, w, x.stride(1), x.stride(0), ctypes.c_void_p(out.data_ptr()), stride, ctypes.c_void_p(lens.data_ptr()), *settings,
                   ctypes.c_void_p(stream.cuda_stream))
        assert st == 0, lib.ire_last_error()
    return call, out, lens


def measure(call, warm=20, windows=15, per=20):
    for _ in range(warm):
        call()
    torch.cuda.synchronize()
    ms = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        for _ in range(per):
            call()
        b.record(stream)
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / per)
    return {"median_ms": round(statistics.median(ms), 5), "min_ms": round(min(ms), 5), "max_ms": round(max(ms), 5)}


def texts_of(out, lens):
    torch.cuda.synchronize()
    l = lens.cpu().numpy()
    return [out[i, :int(l[i])].cpu().numpy().tobytes() for i in range(n)]


res = {}
for q, s in ((85, 0), (85, 2)):
    key = "%d_%d" % (q, s)
    fixed = caller(lib.ire_encode_jpeg_base64_fit_device_ex, lib.ire_jpeg_base64_bound_ex(h, w, q, s), q, s)
    own = caller(lib.ire_encode_jpeg_optimized_base64_fit_device, lib.ire_jpeg_optimized_base64_bound(h, w, q, s), q, s)
    if base_only:
        res["fixed_" + key] = measure(fixed[0])
        res["optimised_" + key] = measure(own[0])
        res["sha256_" + key] = hashlib.sha256(b"\n".join(texts_of(*fixed[1:]) + texts_of(*own[1:]))).hexdigest()
        continue
    prog = caller(lib.ire_encode_jpeg_progressive_base64_fit_device, lib.ire_jpeg_progressive_base64_bound(h, w, q, s), q, s)
    if once:
        prog[0](); own[0]()
        torch.cuda.synchronize()
        continue
    res["optimised_" + key] = measure(own[0])
    res["progressive_" + key] = measure(prog[0])
    res["optimised_again_" + key] = measure(own[0])
    res["ratio_" + key] = round(res["progressive_" + key]["median_ms"] / res["optimised_" + key]["median_ms"], 4)
    to, tp = texts_of(*own[1:]), texts_of(*prog[1:])
    res["chars_optimised_" + key], res["chars_progressive_" + key] = [len(t) for t in to], [len(t) for t in tp]
    res["chars_ratio_" + key] = round(sum(map(len, tp)) / sum(map(len, to)), 4)
    res["chars_ratio_per_image_" + key] = [round(len(b) / len(a), 4) for a, b in zip(to, tp)]
    res["bound_chars_per_image_" + key] = int(lib.ire_jpeg_progressive_base64_bound(h, w, q, s))
    res["coef_scratch_bytes_per_image_" + key] = (((h + 7) // 8) * ((w + 7) // 8) * 3 if s == 0 else ((h + 15) // 16) * ((w + 15) // 16) * 6) * 128
eng.close()
print(json.dumps(res))
