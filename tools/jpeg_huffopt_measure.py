"""profiles/jpeg_huffopt.md: the device JPEG encoder (csrc/jpeg.hip) with the image's own Huffman tables against the fixed-table call, in
one process and at the same settings.  Input: synth.batch(8, 1024, 1024), already on the device.  Method of profiles/jpeg_options.md:
20 warm-up calls, then 15 windows of 20 calls between two device events on the calls' stream; a figure is the median over the windows,
in ms per call.  Prints one JSON object.

    python tools/jpeg_huffopt_measure.py              fixed and optimised at (85, 4:4:4) and (85, 4:2:0), and the text lengths
    python tools/jpeg_huffopt_measure.py --fixed-only the fixed-table default alone, through ire_encode_jpeg_base64_fit_device: also
                                                      runs on a library built before the optimised entries existed (IRE_LIB=...)
    python tools/jpeg_huffopt_measure.py --once       one optimised and one fixed call per setting, for a kernel trace"""
import ctypes, hashlib, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from image_restoration_platform_amd import _lib
NEW = ("ire_jpeg_optimized_base64_bound", "ire_encode_jpeg_optimized_base64_fit_device", "ire_encode_jpeg_optimized_base64_fit", "ire_debug_jpeg_huffman")
fixed_only, once = "--fixed-only" in sys.argv, "--once" in sys.argv
if fixed_only:
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
    o, l = out.cpu().numpy(), lens.cpu().numpy()
    return [o[i, :int(l[i])].tobytes() for i in range(n)]


res = {}
if fixed_only:
    call, out, lens = caller(lib.ire_encode_jpeg_base64_fit_device, lib.ire_jpeg_base64_bound(h, w))
    res["fixed_85_0"] = measure(call)
    res["fixed_85_0_sha256"] = hashlib.sha256(b"\n".join(texts_of(out, lens))).hexdigest()
else:
    for q, s in ((85, 0), (85, 2)):
        fixed = caller(lib.ire_encode_jpeg_base64_fit_device_ex, lib.ire_jpeg_base64_bound_ex(h, w, q, s), q, s)
        own = caller(lib.ire_encode_jpeg_optimized_base64_fit_device, lib.ire_jpeg_optimized_base64_bound(h, w, q, s), q, s)
        key = "%d_%d" % (q, s)
        if once:
            fixed[0](); own[0]()
            torch.cuda.synchronize()
            continue
        res["fixed_" + key] = measure(fixed[0])
        res["optimised_" + key] = measure(own[0])
        res["fixed_again_" + key] = measure(fixed[0])
        res["ratio_" + key] = round(res["optimised_" + key]["median_ms"] / res["fixed_" + key]["median_ms"], 4)
        tf, to = texts_of(*fixed[1:]), texts_of(*own[1:])
        res["chars_fixed_" + key], res["chars_optimised_" + key] = sum(map(len, tf)), sum(map(len, to))
        res["chars_ratio_" + key] = round(res["chars_optimised_" + key] / res["chars_fixed_" + key], 4)
        res["chars_ratio_per_image_" + key] = [round(len(b) / len(a), 4) for a, b in zip(tf, to)]
        if (q, s) == (85, 0):
            res["fixed_85_0_sha256"] = hashlib.sha256(b"\n".join(tf)).hexdigest()
eng.close()
print(json.dumps(res))
