"""Python host binding of the engine's C ABI (include/ire.h) -- numpy and torch-tensor front ends.

This is the "PyTorch-ROCm extension" side of BASELINE.json's north_star: torch supplies device
memory and streams (tensor.data_ptr(), torch.cuda.current_stream()), the engine does the work.
Nothing here computes pixels on the CPU; if libire.so or the GPU is missing every call raises.
"""
import collections
import ctypes
import os

import numpy as np

from . import _lib, weights as _weights

KEYS = ["blur", "noise", "lowLight", "compression", "scratch", "fade", "colorShift"]  # classifier.js:62-70
FAMILIES = ["classifier", "conv3x3", "conv1x1", "stem", "head", "gn_finalize", "fusion", "all"]


# One row per text format (csrc/codec.hpp TextFormat): the engine flag that selects it for the batcher's results, the ABI's host and
# device entry, the Engine method that gives its bound, the noun of its messages, whether a uint64 count goes with every text, and what
# the entries' names end in where they take the format's settings.  "jpeg_opt" is no result format of its own (flag 0): it is "jpeg"
# with the image's own Huffman tables, chosen by IRE_FLAG_JPEG_OPTIMIZE beside IRE_FLAG_RESULT_JPEG or by optimize=True in a call;
# "jpeg_prog" likewise: "jpeg" as a progressive file, chosen by IRE_FLAG_JPEG_PROGRESSIVE or by progressive=True in a call.
TextFormat = collections.namedtuple("TextFormat", "flag host device bound noun counted ex", defaults=("_ex",))
TEXT_FORMATS = {
    "png": TextFormat(_lib.IRE_FLAG_RESULT_PNG_BASE64, "ire_encode_png_base64_fit", "ire_encode_png_base64_fit_device", "png_base64_bytes_fit", "PNG", False),
    "png_deflate": TextFormat(_lib.IRE_FLAG_RESULT_PNG_DEFLATE, "ire_encode_png_deflate_base64_fit", "ire_encode_png_deflate_base64_fit_device",
                              "png_deflate_base64_bound", "PNG", True),
    "jpeg": TextFormat(_lib.IRE_FLAG_RESULT_JPEG, "ire_encode_jpeg_base64_fit", "ire_encode_jpeg_base64_fit_device", "jpeg_base64_bound", "JPEG", True),
    "jpeg_opt": TextFormat(0, "ire_encode_jpeg_optimized_base64_fit", "ire_encode_jpeg_optimized_base64_fit_device", "_jpeg_optimized_base64_bound", "JPEG", True, ""),
    "jpeg_prog": TextFormat(0, "ire_encode_jpeg_progressive_base64_fit", "ire_encode_jpeg_progressive_base64_fit_device", "_jpeg_progressive_base64_bound", "JPEG", True, ""),
}


def result_format(flags):
    """The TextFormat of the results of an engine created with `flags`, or None: pixels."""
    return next((f for f in TEXT_FORMATS.values() if flags & f.flag), None)


class EngineError(RuntimeError):
    """Raised for a non-zero ire_status; .message feeds RestoratorService._classifyError
    (restorator.js:241-265): it contains 'invalid' / 'timeout' / 'service unavailable'."""

    def __init__(self, status, message):
        super().__init__(message)
        self.status = status
        self.message = message
        self.code = {1: "ENGINE_INVALID_INPUT", 2: "ENGINE_TIMEOUT", 3: "ENGINE_UNAVAILABLE"}.get(status, "ENGINE_INTERNAL")


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


def _jpeg_frame_size(data):
    """(h, w) from the frame header of a JPEG file the engine has just accepted (ire_submit_jpeg parsed it: the segments are
    well-formed and a baseline or progressive frame exists), without walking the file a second time: poll() sizes its buffer from them."""
    i = 2
    while True:
        while data[i] == 0xFF:
            i += 1
        marker, n = data[i], int.from_bytes(data[i + 1:i + 3], "big")
        if marker in (0xC0, 0xC1, 0xC2):
            return int.from_bytes(data[i + 4:i + 6], "big"), int.from_bytes(data[i + 6:i + 8], "big")
        i += 1 + n


def upload_plan_reason(data, max_dim=2048, accept=0):
    """bytes of a JPEG upload -> ((stored_h, stored_w, orientation, out_h, out_w), None): what submit_upload does with it on an engine
    whose decoder accepts `accept` -- or (None, reason) when the file is refused.  ire_upload_plan: pure host, no engine, no GPU."""
    data = bytes(data)
    v = [ctypes.c_int() for _ in range(5)]
    if _lib.load().ire_upload_plan(data, len(data), int(accept), int(max_dim), *[ctypes.byref(x) for x in v]) != 0:
        return None, (_lib.load().ire_last_error() or b"").decode()
    return tuple(x.value for x in v), None


def _icc_result(rc, t):
    if rc != 0:
        return None, (_lib.load().ire_last_error() or b"").decode()
    return t, None


def icc_plan_file(data):
    """bytes of a JPEG file -> (IreIccTransform, None): what an engine created with upload_icc=True does with the file's ICC profile
    (.kind: IRE_ICC_NONE / IDENTITY / MATRIX / GREY) -- or (None, reason) for a profile it refuses.  Pure host, no engine, no GPU."""
    data = bytes(data)
    t = _lib.IreIccTransform()
    return _icc_result(_lib.load().ire_icc_plan_file(data, len(data), ctypes.byref(t)), t)


def icc_plan_profile(profile, components=3):
    """icc_plan_file for the raw bytes of a profile that came with an image of 1 or 3 components (a PNG's iCCP, decoded on the host)."""
    profile = bytes(profile)
    t = _lib.IreIccTransform()
    return _icc_result(_lib.load().ire_icc_plan_profile(profile, len(profile), int(components), ctypes.byref(t)), t)


PNG_SIGNATURE = b"\x89PNG\r\n\x1a\n"


def decode_png_plan_reason(data):
    """bytes of a file -> ((h, w, colour_type), None) when an engine created with decode_png=True decodes it on the device, else (None,
    reason) with the reason the C side gives ("invalid: PNG ...").  ire_decode_png_plan: pure host, no engine, no GPU."""
    data = bytes(data)
    h, w, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    if _lib.load().ire_decode_png_plan(data, len(data), ctypes.byref(h), ctypes.byref(w), ctypes.byref(c)) != 0:
        return None, (_lib.load().ire_last_error() or b"").decode()
    return (h.value, w.value, c.value), None


def decode_png_plan_ex_reason(data, accept=0):
    """decode_png_plan_reason with a choice of what is accepted: accept = 0, or IRE_DECODE_ACCEPT_PNG_ALL for the plan of an engine
    created with IRE_FLAG_DECODE_PNG | IRE_FLAG_DECODE_PNG_ALL.  -> ((h, w, colour_type, depth, interlace), None) or (None, reason).
    ire_decode_png_plan_ex: pure host, no engine, no GPU."""
    data = bytes(data)
    h, w, c, d, lace = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    if _lib.load().ire_decode_png_plan_ex(data, len(data), int(accept), ctypes.byref(h), ctypes.byref(w), ctypes.byref(c), ctypes.byref(d), ctypes.byref(lace)) != 0:
        return None, (_lib.load().ire_last_error() or b"").decode()
    return (h.value, w.value, c.value, d.value, lace.value), None


def decode_png_flags(flags, decode_png=None, environ=None):
    """the flags of an engine: IRE_FLAG_DECODE_PNG is added for decode_png=True and, when decode_png is None, for IRE_DECODE_PNG=1 in
    the environment; nothing is ever taken away"""
    if decode_png is None:
        decode_png = (os.environ if environ is None else environ).get("IRE_DECODE_PNG") == "1"
    return flags | _lib.IRE_FLAG_DECODE_PNG if decode_png else flags


def upload_icc_flags(flags, upload_icc=None, environ=None):
    """the flags of an engine: IRE_FLAG_UPLOAD_ICC is added for upload_icc=True and, when upload_icc is None, for IRE_UPLOAD_ICC=1 in
    the environment (which then holds for EVERY engine of the process that does not say upload_icc=False); nothing is ever taken away"""
    if upload_icc is None:
        upload_icc = (os.environ if environ is None else environ).get("IRE_UPLOAD_ICC") == "1"
    return flags | _lib.IRE_FLAG_UPLOAD_ICC if upload_icc else flags


class Engine:
    def __init__(self, device_index=0, max_batch=8, num_streams=0, weights_path="default", seed=0, flags=0, precision="bf16", jpeg_quality=0,
                 jpeg_sampling=0, upload_icc=None, decode_png=None):
        """jpeg_quality (1..100; 0: 85) and jpeg_sampling (0 = 4:4:4, 2 = 4:2:0): the settings of the results of an engine created with
        flags=IRE_FLAG_RESULT_JPEG; invalid without that flag.  flags=IRE_FLAG_RESULT_JPEG | IRE_FLAG_JPEG_OPTIMIZE: those results
        carry their image's own, optimised Huffman tables (poll sizes its buffer by the larger bound of such a text).
        upload_icc=True (or IRE_FLAG_UPLOAD_ICC in flags; None: the environment's IRE_UPLOAD_ICC=1): submit_upload converts the pixels
        of a file that carries an ICC profile to sRGB on the device, before the resize.
        decode_png=True (or IRE_FLAG_DECODE_PNG in flags; None: the environment's IRE_DECODE_PNG=1): decode_png, and submit_jpeg /
        submit_file / submit_upload take a PNG file beside a JPEG one.  IRE_FLAG_DECODE_PNG_ALL in flags beside it: also 1-, 2-, 4- and
        16-bit files and Adam7 ones (decode_png_plan_ex_reason says which)."""
        flags = decode_png_flags(upload_icc_flags(flags, upload_icc), decode_png)
        self._lib = _lib.load()
        if weights_path == "default":
            weights_path = _weights.ensure_default(seed)
        cfg = _lib.IreConfig()
        cfg.struct_size = ctypes.sizeof(_lib.IreConfig)
        cfg.device_index = device_index
        if precision not in ("bf16", "fp8"):
            raise EngineError(1, "invalid precision: 'bf16' or 'fp8'")
        cfg.precision = 1 if precision == "fp8" else 0          # IRE_PRECISION_*
        cfg.max_batch = max_batch
        cfg.num_streams = num_streams
        cfg.weights_path = weights_path.encode() if weights_path else None
        cfg.flags = flags
        cfg.jpeg_quality = jpeg_quality
        cfg.jpeg_sampling = jpeg_sampling
        self._flags = flags
        self._jpeg_settings = (int(jpeg_quality), int(jpeg_sampling))
        self.last_plan_reason = ""
        h = ctypes.c_void_p()
        self._h = None
        self._check(self._lib.ire_init(ctypes.byref(cfg), ctypes.byref(h)))
        self._h = h
        self.max_batch = max_batch

    def load_weights(self, blob):
        """RestoreNet-v0 weights from memory (the bytes of a weight file): ire_load_weights."""
        b = bytes(blob)
        self._check(self._lib.ire_load_weights(self._h, b, len(b)))

    def _check(self, rc):
        if rc != 0:
            msg = self._lib.ire_last_error()
            raise EngineError(rc, msg.decode() if msg else f"engine error {rc}")

    def close(self):
        if getattr(self, "_h", None):
            for ref in getattr(self, "_sessions", []):     # open strip sessions die with their engine (ire_shutdown would only
                s = ref()                                  # leave them as empty shells): close them first
                if s is not None:
                    s.close()
            self._sessions = []
            self._lib.ire_shutdown(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- host (numpy) -------------------------------------------------------------------------
    @staticmethod
    def _as_batch(rgb):
        rgb = np.asarray(rgb)
        if rgb.dtype != np.uint8:
            raise EngineError(1, "invalid input: image dtype must be uint8")
        if rgb.ndim == 3:
            rgb = rgb[None]
        if rgb.ndim != 4 or rgb.shape[3] != 3:
            raise EngineError(1, "invalid input: expected [N,H,W,3] uint8")
        return np.ascontiguousarray(rgb)

    def classify(self, rgb, is_jpeg=True):
        """-> (scores [N,7] float64, labels [N] int32).  ClassifierService.analyze (classifier.js:40)."""
        rgb = self._as_batch(rgb)
        n, h, w, _ = rgb.shape
        jp = np.ascontiguousarray(np.broadcast_to(np.asarray(is_jpeg, dtype=np.uint8), (n,)))
        scores = np.zeros((n, 7), np.float64)
        labels = np.zeros(n, np.int32)
        self._check(self._lib.ire_classify(self._h, _ptr(rgb), n, h, w, 3 * w, _ptr(jp), _ptr(scores), _ptr(labels)))
        return scores, labels

    def restore(self, rgb, scores=None, is_jpeg=True, return_timings=False):
        """-> restored [N,H,W,3] uint8.  The step behind GeminiClient.restoreImage (geminiClient.js:32)."""
        rgb = self._as_batch(rgb)
        n, h, w, _ = rgb.shape
        jp = np.ascontiguousarray(np.broadcast_to(np.asarray(is_jpeg, dtype=np.uint8), (n,)))
        sc = None
        if scores is not None:
            sc = np.ascontiguousarray(np.asarray(scores, dtype=np.float64).reshape(n, 7))
        out = np.empty_like(rgb)
        t = _lib.IreTimings()
        self._check(self._lib.ire_restore(self._h, _ptr(rgb), n, h, w, _ptr(sc), _ptr(jp), _ptr(out), ctypes.byref(t)))
        if return_timings:
            return out, {"classify_ms": t.classify_ms, "restore_ms": t.restore_ms, "total_ms": t.total_ms}
        return out

    def restore_fit(self, rgb, scores=None, is_jpeg=True, return_timings=False):
        """restore() for an image of ANY size (1..8192 per side): -> restored [N,H,W,3] uint8 of the input's own shape.  The engine
        edge-replicates to the next multiple of 8 (>= 16) on the device, restores and returns the window; scores=None classifies the
        original pixels inside the same call.  Equal, bit for bit, to restore(np.pad(x, edge), scores=classify(x)[0])[:, :H, :W]."""
        rgb = self._as_batch(rgb)
        n, h, w, _ = rgb.shape
        jp = np.ascontiguousarray(np.broadcast_to(np.asarray(is_jpeg, dtype=np.uint8), (n,)))
        sc = None
        if scores is not None:
            sc = np.ascontiguousarray(np.asarray(scores, dtype=np.float64).reshape(n, 7))
        out = np.empty_like(rgb)
        t = _lib.IreTimings()
        self._check(self._lib.ire_restore_fit(self._h, _ptr(rgb), n, h, w, _ptr(sc), _ptr(jp), _ptr(out), ctypes.byref(t)))
        if return_timings:
            return out, {"classify_ms": t.classify_ms, "restore_ms": t.restore_ms, "total_ms": t.total_ms}
        return out

    def fuse(self, views, noise_score=-1.0):
        """views [k,H,W,3] uint8, k in 2..3 -> (fused [H,W,3], shifts [k,2] (dy,dx))."""
        views = self._as_batch(views)
        k, h, w, _ = views.shape
        out = np.empty((h, w, 3), np.uint8)
        shifts = np.zeros((k, 2), np.int32)
        t = _lib.IreTimings()
        self._check(self._lib.ire_fuse(self._h, _ptr(views), k, h, w, float(noise_score), _ptr(out), _ptr(shifts),
                                       ctypes.byref(t)))
        return out, shifts

    def preprocess_plan(self, width, height, orientation=1, max_dim=2048):
        """-> (out_w, out_h, resized): size rule of imagePreprocess.js:12-22,46-55 (host arithmetic, no GPU work)."""
        ow, oh, rs = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        self._check(self._lib.ire_preprocess_plan(int(width), int(height), int(orientation), int(max_dim), ctypes.byref(ow),
                                                  ctypes.byref(oh), ctypes.byref(rs)))
        return ow.value, oh.value, bool(rs.value)

    def preprocess(self, rgb, orientation=1, max_dim=2048):
        """stored pixels [H,W,3] uint8 -> upright pixels fitted inside max_dim (EXIF orient + Lanczos-3), on the GPU."""
        rgb = np.ascontiguousarray(rgb)
        if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3:
            raise EngineError(1, "invalid input: expected [H,W,3] uint8")
        h, w, _ = rgb.shape
        ow, oh, _ = self.preprocess_plan(w, h, orientation, max_dim)
        out = np.empty((oh, ow, 3), np.uint8)
        self._check(self._lib.ire_preprocess(self._h, _ptr(rgb), h, w, int(orientation), int(max_dim), _ptr(out), oh, ow))
        return out

    def preprocess_tensor(self, rgb_u8, orientation=1, max_dim=2048, stream=None):
        import torch
        assert rgb_u8.is_cuda and rgb_u8.dtype == torch.uint8 and rgb_u8.is_contiguous() and rgb_u8.dim() == 3
        h, w, _ = rgb_u8.shape
        ow, oh, _ = self.preprocess_plan(w, h, orientation, max_dim)
        out = torch.empty((oh, ow, 3), dtype=torch.uint8, device=rgb_u8.device)
        self._check(self._lib.ire_preprocess_device(self._h, ctypes.c_void_p(rgb_u8.data_ptr()), h, w, int(orientation), int(max_dim),
                                                    ctypes.c_void_p(out.data_ptr()), oh, ow, self._stream_ptr(stream)))
        return out

    def preprocess_batch(self, rgb_u8, orientation=1, max_dim=2048, out_u8=None, stream=None):
        """cuda uint8 [N,h,w,3] stored images of one size and orientation (N <= max_batch; each image dense, the images any stride
        apart: a view [:, :h*w*3] of a wider [N,pitch] buffer reshaped is fine) -> cuda uint8 [N,out_h,out_w,3] upright fitted images,
        image i byte for byte preprocess_tensor's.  Asynchronous on the torch stream; two launches whatever N.  out_u8: where the
        result goes (same rules: dense images, any stride between them; nothing between them is written)."""
        import torch
        assert rgb_u8.is_cuda and rgb_u8.dtype == torch.uint8 and rgb_u8.dim() == 4 and rgb_u8.shape[3] == 3 and rgb_u8[0].is_contiguous()
        n, h, w, _ = rgb_u8.shape
        ow, oh, _ = self.preprocess_plan(w, h, orientation, max_dim)
        if out_u8 is None:
            out_u8 = torch.empty((n, oh, ow, 3), dtype=torch.uint8, device=rgb_u8.device)
        assert out_u8.is_cuda and out_u8.dtype == torch.uint8 and tuple(out_u8.shape) == (n, oh, ow, 3) and out_u8[0].is_contiguous()
        self._check(self._lib.ire_preprocess_batch_device(self._h, ctypes.c_void_p(rgb_u8.data_ptr()), n, h, w, rgb_u8.stride(0) if n > 1 else h * w * 3,
                                                          int(orientation), int(max_dim), ctypes.c_void_p(out_u8.data_ptr()), oh, ow,
                                                          out_u8.stride(0) if n > 1 else oh * ow * 3, self._stream_ptr(stream)))
        return out_u8

    def upload_plan(self, data, max_dim=2048):
        """(stored_h, stored_w, orientation, out_h, out_w) of a JPEG (with decode_png=True: or PNG) upload as THIS engine's submit_upload takes it; raises EngineError
        (invalid input, the plan's reason) for a file it refuses.  Pure host arithmetic."""
        plan, why = upload_plan_reason(data, max_dim, self.upload_accept)
        if plan is None:
            raise EngineError(_lib.IRE_ERR_INVALID_INPUT, why)
        return plan

    def submit_upload(self, data, max_dim=2048, scores=None):
        """Queue one upload as its bytes -- a JPEG file, or on an engine created with decode_png=True a PNG file (orientation from its eXIf
        chunk; the result is then that of submit_fit(..., is_jpeg=False, ...) of decode_png's pixels): decoded, turned upright by its EXIF orientation, fitted inside max_dim (Lanczos-3) and
        restored, all on the device with its batch.  The result is that of submit_fit(preprocess(decode_jpeg(data), orientation,
        max_dim), is_jpeg=True, scores), of the fitted size upload_plan reports; on an engine created with upload_icc=True the decoded
        pixels first go through icc_to_srgb with the file's own transform (icc_plan_file).  Raises EngineError (invalid input) for a file the plan
        refuses: no job exists then.  A file with corrupt data fails at its poll."""
        data = bytes(data)
        sc = None if scores is None else np.ascontiguousarray(np.asarray(scores, dtype=np.float64).reshape(7))
        job = ctypes.c_void_p()
        self._check(self._lib.ire_submit_upload(self._h, data, len(data), int(max_dim), _ptr(sc), ctypes.byref(job)))
        _, _, _, oh, ow = upload_plan_reason(data, max_dim, self.upload_accept)[0]
        return (job, oh, ow)

    def submit(self, rgb, is_jpeg=True, scores=None):
        """Queue one image with the engine's batcher (in-flight jobs of one shape coalesce into engine batches);
        scores: the 7 scores a previous classify() returned for this image => it is not classified again."""
        rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
        h, w, _ = rgb.shape
        sc = None if scores is None else np.ascontiguousarray(np.asarray(scores, dtype=np.float64).reshape(7))
        job = ctypes.c_void_p()
        self._check(self._lib.ire_submit(self._h, _ptr(rgb), h, w, int(bool(is_jpeg)), _ptr(sc), ctypes.byref(job)))
        return (job, h, w)

    def submit_fit(self, rgb, is_jpeg=True, scores=None):
        """submit() for an image of any size (1..8192 per side); poll() / release() take the job as they take submit()'s."""
        rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
        if rgb.ndim != 3 or rgb.shape[2] != 3:
            raise EngineError(_lib.IRE_ERR_INVALID_INPUT, "invalid input: expected [H,W,3] uint8")
        h, w, _ = rgb.shape
        sc = None if scores is None else np.ascontiguousarray(np.asarray(scores, dtype=np.float64).reshape(7))
        job = ctypes.c_void_p()
        self._check(self._lib.ire_submit_fit(self._h, _ptr(rgb), h, w, int(bool(is_jpeg)), _ptr(sc), ctypes.byref(job)))
        return (job, h, w)

    def submit_jpeg(self, data, scores=None):
        """submit_fit() for an encoded upload: the bytes of a JPEG file that decode_jpeg_plan accepts (baseline; on an engine created with
        IRE_FLAG_DECODE_PROGRESSIVE progressive too), or on an engine created with decode_png=True of a PNG file that decode_png_plan
        accepts (its result is that of submit_fit(decode_png(data), is_jpeg=False, scores)).  The file is parsed in
        this call and decoded on the device with its batch; the result is that of submit_fit(its pixels, is_jpeg=True, scores).
        Raises EngineError (invalid input, the plan's reason) for a file out of scope: no job exists then.  A file with corrupt data
        fails at its poll."""
        data = bytes(data)
        sc = None if scores is None else np.ascontiguousarray(np.asarray(scores, dtype=np.float64).reshape(7))
        job = ctypes.c_void_p()
        self._check(self._lib.ire_submit_jpeg(self._h, data, len(data), _ptr(sc), ctypes.byref(job)))      # the one parse of the file: refuses with the plan's reason
        if data[:8] == PNG_SIGNATURE:          # (accepted, so the engine decodes PNG and IHDR follows the signature)
            w, h = int.from_bytes(data[16:20], "big"), int.from_bytes(data[20:24], "big")
        else:
            h, w = _jpeg_frame_size(data)
        return (job, h, w)

    submit_file = submit_jpeg          # the neutral name: a JPEG file, or on an engine created with decode_png=True a PNG file

    def submit_fuse_fit(self, views, is_jpeg=True, scores=None):
        """Queue ONE fusion job: views [k,H,W,3] uint8 (or a list of k [H,W,3] arrays), k in 2..3, any size 1..8192 per side.  Every
        view is restored as submit_fit() restores it, the restored views are fused on the device (noise score of view 0, as
        fuse(noise_score=-1) takes it) and poll() returns the fused [H,W,3] image -- on a text engine its text.  is_jpeg: one bool or
        k of them; scores: None, or k entries each None or the 7 scores classify() gave for that view.  poll() / release() take the
        job as they take submit()'s; the polled scores are view 0's."""
        vs = [np.ascontiguousarray(v, dtype=np.uint8) for v in views]
        k = len(vs)
        if k and any(v.ndim != 3 or v.shape[2] != 3 or v.shape != vs[0].shape for v in vs):
            raise EngineError(_lib.IRE_ERR_INVALID_INPUT, "invalid input: fusion views must be [H,W,3] uint8 of identical dimensions")
        h, w = (vs[0].shape[0], vs[0].shape[1]) if k else (0, 0)
        jp = np.ascontiguousarray(np.broadcast_to(np.asarray(is_jpeg, dtype=np.uint8), (k,)))
        has = np.zeros(max(k, 1), np.uint8)
        sc = np.zeros((max(k, 1), 7), np.float64)
        if scores is not None and len(scores) != k:
            raise EngineError(_lib.IRE_ERR_INVALID_INPUT, "invalid input: scores must have one entry (7 scores or None) for each fusion view")
        for i, row in enumerate(scores if scores is not None else []):
            if row is not None:
                has[i] = 1
                sc[i] = np.asarray(row, dtype=np.float64).reshape(7)
        ptrs = (ctypes.c_void_p * max(k, 1))(*[v.ctypes.data for v in vs])
        job = ctypes.c_void_p()
        self._check(self._lib.ire_submit_fuse_fit(self._h, ptrs, k, h, w, _ptr(jp), _ptr(has), _ptr(sc), ctypes.byref(job)))
        return (job, h, w)

    def restore_fuse_fit_tensor(self, views_u8, out_u8=None, scores=None, is_jpeg_u8=None, stream=None):
        """The fusion job's computation for tensors, asynchronous on the torch stream: views cuda uint8 [B,k,H,W,3] (B view sets of
        k in 2..3 views, any size 1..8192 per side, B*k <= max_batch) -> fused cuda uint8 [B,H,W,3].  scores: cuda float64 [B*k,7]
        for every view, or None: classified inside."""
        import torch
        assert views_u8.is_cuda and views_u8.dtype == torch.uint8 and views_u8.is_contiguous() and views_u8.dim() == 5
        b, k, h, w, _ = views_u8.shape
        if out_u8 is None:
            out_u8 = torch.empty((b, h, w, 3), dtype=torch.uint8, device=views_u8.device)
        sc = ctypes.c_void_p(scores.data_ptr()) if scores is not None else None
        jp = ctypes.c_void_p(is_jpeg_u8.data_ptr()) if is_jpeg_u8 is not None else None
        self._check(self._lib.ire_restore_fuse_fit_device(self._h, ctypes.c_void_p(views_u8.data_ptr()), b, k, h, w, sc, jp,
                                                          ctypes.c_void_p(out_u8.data_ptr()), self._stream_ptr(stream)))
        return out_u8

    def fusion_wlut(self, noise):
        """noise scores [n] -> blend tables [n,256] uint32, built on the device by the kernel the fusion jobs use (ire_debug_fusion_wlut)."""
        ns = np.ascontiguousarray(np.asarray(noise, dtype=np.float64).reshape(-1))
        out = np.zeros((ns.size, 256), np.uint32)
        self._check(self._lib.ire_debug_fusion_wlut(self._h, _ptr(ns), ns.size, _ptr(out)))
        return out

    def stats(self):
        """Service gauges (f4: getHealthStatus / the /health/ready dependency entry)."""
        st = _lib.IreEngineStats()
        st.struct_size = ctypes.sizeof(_lib.IreEngineStats)
        self._check(self._lib.ire_get_stats(self._h, ctypes.byref(st)))
        return {"queueDepth": st.queue_depth, "batches": st.batches, "images": st.images, "lastBatch": st.last_batch,
                "maxBatch": st.max_batch, "imagesPerSec": st.images_per_sec}

    def max_batch_for(self, h, w):
        return int(self._lib.ire_max_batch_for(self._h, int(h), int(w)))

    def poll(self, job, timeout_ms=-1):
        """-> (restored [H,W,3] uint8 -- or, for an engine created with flags=IRE_FLAG_RESULT_PNG_BASE64 / IRE_FLAG_RESULT_PNG_DEFLATE /
        IRE_FLAG_RESULT_JPEG, the `bytes` of the base64 text of its PNG / JPEG file --, scores[7], timings)"""
        handle, h, w = job
        fmt = result_format(getattr(self, "_flags", 0))
        text = fmt is not None
        if text and fmt.counted:
            return self._poll_text(handle, timeout_ms, getattr(self, fmt.bound)(h, w))
        out = np.empty(getattr(self, fmt.bound)(h, w), np.uint8) if text else np.empty((h, w, 3), np.uint8)     # (the job's own h, w)
        scores = np.zeros(7, np.float64)
        t = _lib.IreTimings()
        self._check(self._lib.ire_poll(self._h, handle, timeout_ms, _ptr(out), _ptr(scores), ctypes.byref(t)))
        if text:
            out = out.tobytes()
        return out, scores, {"classify_ms": t.classify_ms, "restore_ms": t.restore_ms, "total_ms": t.total_ms}

    def _poll_text(self, handle, timeout_ms, cap):
        """ire_poll_text: a result whose length depends on the data (IRE_FLAG_RESULT_PNG_DEFLATE, IRE_FLAG_RESULT_JPEG) -> (`bytes` of its real length, ...)."""
        out = np.empty(cap, np.uint8)
        n = ctypes.c_size_t(0)
        scores = np.zeros(7, np.float64)
        t = _lib.IreTimings()
        self._check(self._lib.ire_poll_text(self._h, handle, timeout_ms, _ptr(out), cap, ctypes.byref(n), _ptr(scores), ctypes.byref(t)))
        return out[:n.value].tobytes(), scores, {"classify_ms": t.classify_ms, "restore_ms": t.restore_ms, "total_ms": t.total_ms}

    def _encode_fit(self, fmt, rgb, settings=None):
        """The host encoder of TEXT_FORMATS[fmt]: [N,H,W,3] (or [H,W,3]) uint8 -> list of N `bytes` (one for a single image).  settings:
        None, or the format's own (JPEG: (quality, sampling)), which go to the entry's _ex form behind its other arguments."""
        f = TEXT_FORMATS[fmt]
        single = np.asarray(rgb).ndim == 3
        x = self._as_batch(rgb)
        n, h, w, _ = x.shape
        ex = () if settings is None else tuple(int(v) for v in settings)
        cb = getattr(self, f.bound)(h, w, *ex)
        if cb == 0:
            raise EngineError(_lib.IRE_ERR_INVALID_INPUT, f"invalid image size or settings for the {f.noun} encoder: height and width must be in 1..8192")
        stride = (cb + 15) // 16 * 16
        out = np.empty((n, stride), np.uint8)
        lens = np.zeros(n, np.uint64) if f.counted else None
        self._check(getattr(self._lib, f.host + (f.ex if ex else ""))(self._h, _ptr(x), n, h, w, _ptr(out), stride, *([_ptr(lens)] if f.counted else []), *ex))
        res = [out[i, :int(lens[i]) if f.counted else cb].tobytes() for i in range(n)]
        return res[0] if single else res

    def _encode_fit_tensor(self, fmt, rgb_u8, stream, settings=None):
        """The device encoder of TEXT_FORMATS[fmt]: -> cuda uint8 [N, bound] ASCII, and for a counted format (that, cuda int64 [N] counts).
        The window is encoded where it lies, its strides go to the engine as pitches.  settings: as for _encode_fit."""
        import torch
        f = TEXT_FORMATS[fmt]
        ex = () if settings is None else tuple(int(v) for v in settings)
        assert rgb_u8.is_cuda and rgb_u8.dtype == torch.uint8 and rgb_u8.dim() == 4 and rgb_u8.shape[3] == 3
        n, h, w, _ = rgb_u8.shape
        si, sr, sp, sc = rgb_u8.stride()
        if sc != 1 or sp != 3 or sr < 3 * w:
            raise EngineError(_lib.IRE_ERR_INVALID_INPUT, f"invalid tensor layout for the {f.noun} encoder: pixels must be dense RGB")
        cb = getattr(self, f.bound)(h, w, *ex)
        if cb == 0:
            raise EngineError(_lib.IRE_ERR_INVALID_INPUT, f"invalid image size or settings for the {f.noun} encoder: height and width must be in 1..8192")
        stride = (cb + 3) // 4 * 4
        out = torch.empty((n, stride), dtype=torch.uint8, device=rgb_u8.device)
        lens = torch.zeros(n, dtype=torch.int64, device=rgb_u8.device) if f.counted else None      # (the counts are uint64 and < 2^63)
        self._check(getattr(self._lib, f.device + (f.ex if ex else ""))(self._h, ctypes.c_void_p(rgb_u8.data_ptr()), n, h, w, sr, si if n > 1 else max(si, sr * h),
                                                                         ctypes.c_void_p(out.data_ptr()), stride,
                                                                         *([ctypes.c_void_p(lens.data_ptr())] if f.counted else []), *ex, self._stream_ptr(stream)))
        return (out[:, :cb], lens) if f.counted else out[:, :cb]

    def png_base64_bytes(self, h, w):
        return int(self._lib.ire_png_base64_bytes(int(h), int(w)))

    def png_deflate_base64_bound(self, h, w):
        """The most characters the compressing encoder can give for an h x w image (0 outside 1..8192): sizes every buffer."""
        return int(self._lib.ire_png_deflate_base64_bound(int(h), int(w)))

    def encode_png_deflate_base64_fit(self, rgb):
        """[N,H,W,3] (or [H,W,3]) uint8, any size 1..8192 per side -> list of N `bytes` (one for a single image): the base64 text of a
        COMPRESSED PNG file of each image (Paeth filter, Huffman-coded deflate blocks), encoded on the device; each of its real length."""
        return self._encode_fit("png_deflate", rgb)

    def encode_png_deflate_base64_fit_tensor(self, rgb_u8, stream=None):
        """cuda uint8 [N,h,w,3], possibly a window of a larger tensor -> (cuda uint8 [N, bound] ASCII, cuda int64 [N] character counts),
        asynchronous on the stream: text i is out[i, :lens[i]]."""
        return self._encode_fit_tensor("png_deflate", rgb_u8, stream)

    def _jpeg_ex(self, quality, sampling):
        """the settings of a direct call: what the call names, else this engine's own (the batcher's results), else 85 and 4:4:4"""
        q0, s0 = getattr(self, "_jpeg_settings", (0, 0))
        return (q0 if quality is None else int(quality), s0 if sampling is None else int(sampling))

    def _jpeg_fmt(self, optimize, progressive=None):
        """"jpeg_prog" | "jpeg_opt" | "jpeg": what the call names, else this engine's own setting (IRE_FLAG_JPEG_PROGRESSIVE,
        IRE_FLAG_JPEG_OPTIMIZE); progressive wins: such a file's tables are always its own"""
        flags = getattr(self, "_flags", 0)
        if bool(flags & _lib.IRE_FLAG_JPEG_PROGRESSIVE) if progressive is None else bool(progressive):
            return "jpeg_prog"
        own = bool(flags & _lib.IRE_FLAG_JPEG_OPTIMIZE)
        return "jpeg_opt" if (own if optimize is None else bool(optimize)) else "jpeg"

    def _jpeg_progressive_base64_bound(self, h, w, quality, sampling):
        return int(self._lib.ire_jpeg_progressive_base64_bound(int(h), int(w), int(quality), int(sampling)))

    def _jpeg_optimized_base64_bound(self, h, w, quality, sampling):
        return int(self._lib.ire_jpeg_optimized_base64_bound(int(h), int(w), int(quality), int(sampling)))

    def jpeg_base64_bound(self, h, w, quality=None, sampling=None, optimize=None, progressive=None):
        """The most characters the JPEG encoder can give for an h x w image at a quality (1..100) and sampling (0 = 4:4:4, 2 = 4:2:0),
        with the fixed Huffman tables, (optimize=True: a larger bound) the image's own, or (progressive=True: larger again) as a
        progressive file; left out: this engine's settings.  0 outside 1..8192 or for settings the encoder refuses.  Sizes every buffer."""
        fmt = self._jpeg_fmt(optimize, progressive)
        if fmt == "jpeg_prog":
            return self._jpeg_progressive_base64_bound(h, w, *self._jpeg_ex(quality, sampling))
        if fmt == "jpeg_opt":
            return self._jpeg_optimized_base64_bound(h, w, *self._jpeg_ex(quality, sampling))
        return int(self._lib.ire_jpeg_base64_bound_ex(int(h), int(w), *self._jpeg_ex(quality, sampling)))

    def encode_jpeg_base64_fit(self, rgb, quality=None, sampling=None, optimize=None, progressive=None):
        """[N,H,W,3] (or [H,W,3]) uint8, any size 1..8192 per side -> list of N `bytes` (one for a single image): the base64 text of a
        baseline JPEG file of each image, encoded on the device; each of its real length.  quality 1..100 and sampling 0 = 4:4:4 |
        2 = 4:2:0; optimize: the file carries the image's own Huffman tables (smaller, the same pixels); progressive: the file is a
        progressive one, ten scans each under its own table (smaller again, the same pixels); left out: this engine's settings
        (quality 85, 4:4:4, the fixed tables unless it was created with others)."""
        return self._encode_fit(self._jpeg_fmt(optimize, progressive), rgb, self._jpeg_ex(quality, sampling))

    def encode_jpeg_base64_fit_tensor(self, rgb_u8, stream=None, quality=None, sampling=None, optimize=None, progressive=None):
        """cuda uint8 [N,h,w,3], possibly a window of a larger tensor -> (cuda uint8 [N, bound] ASCII, cuda int64 [N] character counts),
        asynchronous on the stream: text i is out[i, :lens[i]].  quality, sampling, optimize, progressive: as for encode_jpeg_base64_fit."""
        return self._encode_fit_tensor(self._jpeg_fmt(optimize, progressive), rgb_u8, stream, self._jpeg_ex(quality, sampling))

    def debug_jpeg_huffman(self, counts):
        """[n][4][256] symbol counts -> (bits_vals uint8 [n][4][272], nvals int32 [n][4]): the tables the optimised JPEG path's table
        kernel builds (tests only)"""
        c = np.ascontiguousarray(counts, np.uint32)
        assert c.ndim == 3 and c.shape[1:] == (4, 256)
        bv = np.zeros((c.shape[0], 4, 16 + 256), np.uint8)
        nv = np.zeros((c.shape[0], 4), np.int32)
        self._check(self._lib.ire_debug_jpeg_huffman(self._h, _ptr(c), c.shape[0], _ptr(bv), _ptr(nv)))
        return bv, nv

    def debug_jpeg_progressive_from_coefs(self, coefs, h, w, quality, sampling):
        """[n][blocks][64] int16 coefficients (the layout ire.h gives) -> list of n `bytes`: the progressive files the device makes of
        them, without its coefficient pass (tests only)"""
        c = np.ascontiguousarray(coefs, np.int16)
        assert c.ndim == 3 and c.shape[2] == 64
        n = c.shape[0]
        stride = (self._jpeg_progressive_base64_bound(h, w, quality, sampling) // 4 * 3 + 15) // 16 * 16
        out = np.empty((n, stride), np.uint8)
        lens = np.zeros(n, np.uint64)
        self._check(self._lib.ire_debug_jpeg_progressive_from_coefs(self._h, _ptr(c), n, int(h), int(w), int(quality), int(sampling), _ptr(out), stride, _ptr(lens)))
        return [out[i, :int(lens[i])].tobytes() for i in range(n)]

    # ---- JPEG uploads decoded on the device (csrc/jpeg_parse.hpp, csrc/jpeg_dec.hip) -------------------------------------------
    @property
    def decode_accept(self):
        """what this engine's decoder takes beside baseline files: IRE_DECODE_ACCEPT_PROGRESSIVE when it was created with
        IRE_FLAG_DECODE_PROGRESSIVE, else 0"""
        return _lib.IRE_DECODE_ACCEPT_PROGRESSIVE if getattr(self, "_flags", 0) & _lib.IRE_FLAG_DECODE_PROGRESSIVE else 0

    @property
    def upload_accept(self):
        """decode_accept, and IRE_DECODE_ACCEPT_ICC when the engine was created with IRE_FLAG_UPLOAD_ICC: what upload_plan_reason is asked"""
        f = getattr(self, "_flags", 0)
        return (self.decode_accept | (_lib.IRE_DECODE_ACCEPT_ICC if f & _lib.IRE_FLAG_UPLOAD_ICC else 0) |
                (_lib.IRE_DECODE_ACCEPT_PNG if f & _lib.IRE_FLAG_DECODE_PNG else 0) | self.png_accept)

    @property
    def png_accept(self):
        """IRE_DECODE_ACCEPT_PNG_ALL when the engine was created with IRE_FLAG_DECODE_PNG_ALL, else 0: what this engine's PNG plan is asked"""
        return _lib.IRE_DECODE_ACCEPT_PNG_ALL if getattr(self, "_flags", 0) & _lib.IRE_FLAG_DECODE_PNG_ALL else 0

    def _png_plan(self, data):
        """((h, w, colour_type), None) or (None, reason), as THIS engine's decoder plans the file"""
        plan, why = decode_png_plan_ex_reason(data, self.png_accept)
        return (plan[:3] if plan else None), why

    def icc_to_srgb(self, rgb, transforms):
        """[n,h,w,3] uint8 (or one [h,w,3]) and n IreIccTransform (None: leave the image) -> the converted copy: ire_icc_to_srgb."""
        a = np.array(rgb, dtype=np.uint8, order="C")
        one = a.ndim == 3
        b = a[None] if one else a
        n, h, w, _ = b.shape
        assert len(transforms) == n
        ptrs = (ctypes.c_void_p * n)(*[ctypes.addressof(t) if t is not None else None for t in transforms])
        self._check(self._lib.ire_icc_to_srgb(self._h, _ptr(b), n, h, w, ptrs))
        return b[0] if one else b

    def icc_to_srgb_device(self, buf_u8, n, h, w, pitch, transforms, stream=None):
        """in place over a cuda uint8 tensor that holds n images of h x w x 3 bytes, `pitch` bytes apart: ire_icc_to_srgb_device"""
        assert buf_u8.is_cuda and buf_u8.is_contiguous() and buf_u8.numel() >= pitch * (n - 1) + h * w * 3 and len(transforms) == n
        ptrs = (ctypes.c_void_p * n)(*[ctypes.addressof(t) if t is not None else None for t in transforms])
        self._check(self._lib.ire_icc_to_srgb_device(self._h, ctypes.c_void_p(buf_u8.data_ptr()), n, h, w, int(pitch), ptrs, self._stream_ptr(stream)))
        return buf_u8

    def decode_jpeg_plan_reason(self, data):
        """bytes of a file -> ((h, w, sampling), None) when THIS engine's device decodes it (sampling: 0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0,
        3 = grey), else (None, reason) with the reason the C side gives ("invalid: progressive JPEG ...").  Pure host arithmetic;
        nothing is kept on the engine, so any number of threads may ask (ire_last_error is per thread)."""
        data = bytes(data)
        h, w, s, k = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        if self._lib.ire_decode_jpeg_plan_ex(data, len(data), self.decode_accept, ctypes.byref(h), ctypes.byref(w), ctypes.byref(s), ctypes.byref(k)) != 0:
            return None, (self._lib.ire_last_error() or b"").decode()
        return (h.value, w.value, s.value), None

    def decode_jpeg_plan(self, data):
        """decode_jpeg_plan_reason without the reason: (h, w, sampling) or None.  The reason of the LAST refusal on this engine is kept
        in .last_plan_reason for interactive use; with several threads use decode_jpeg_plan_reason."""
        plan, why = self.decode_jpeg_plan_reason(data)
        if plan is None:
            self.last_plan_reason = why
        return plan

    def decode_jpeg(self, data):
        """bytes of a JPEG file the plan accepts -> [h,w,3] uint8, equal to PIL.Image.open(f).convert("RGB"); raises
        EngineError (invalid input) for a file out of scope or with corrupt data.  The plan runs here (the output's size comes from
        it): a caller need not ask first."""
        data = bytes(data)
        plan, why = self.decode_jpeg_plan_reason(data)
        if plan is None:
            raise EngineError(_lib.IRE_ERR_INVALID_INPUT, why)
        h, w, _ = plan
        out = np.empty((h, w, 3), np.uint8)
        self._check(self._lib.ire_decode_jpeg(self._h, data, len(data), _ptr(out), h, w))
        return out

    # ---- PNG uploads decoded on the device (csrc/png_parse.hpp, csrc/png_dec.hip): an engine created with decode_png=True ----------
    def decode_png_plan(self, data):
        """(h, w, colour_type) or None; the reason of the last refusal is kept in .last_plan_reason (decode_png_plan_reason: no engine)"""
        plan, why = self._png_plan(data)
        if plan is None:
            self.last_plan_reason = why
        return plan

    def decode_png(self, data):
        """bytes of a PNG file the plan accepts -> [h,w,3] uint8, equal to PIL.Image.open(f).convert("RGB"); raises EngineError (invalid
        input) for a file out of scope, for data the device flags, and on an engine created without decode_png=True."""
        data = bytes(data)
        plan, why = self._png_plan(data)
        if plan is None:
            raise EngineError(_lib.IRE_ERR_INVALID_INPUT, why)
        h, w, _ = plan
        out = np.empty((h, w, 3), np.uint8)
        self._check(self._lib.ire_decode_png(self._h, data, len(data), _ptr(out), h, w))
        return out

    def decode_png_device(self, files, out_u8=None, stream=None):
        """decode_jpeg_device for PNG files of one planned size, of any colour types"""
        import torch
        files = [bytes(f) for f in files]
        plans = [self._png_plan(f)[0] for f in files]
        if not files or any(p is None for p in plans) or len({p[:2] for p in plans}) != 1:
            raise EngineError(_lib.IRE_ERR_INVALID_INPUT, "invalid input: decode_png_device takes files of one planned size")
        n, (h, w, _) = len(files), plans[0]
        if out_u8 is None:
            out_u8 = torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda")
        assert out_u8.is_cuda and out_u8.dtype == torch.uint8 and tuple(out_u8.shape) == (n, h, w, 3) and out_u8[0].is_contiguous()
        status = torch.empty(n, dtype=torch.int32, device=out_u8.device)
        ptrs = (ctypes.c_char_p * n)(*files)
        lens = (ctypes.c_size_t * n)(*[len(f) for f in files])
        self._check(self._lib.ire_decode_png_device(self._h, ptrs, lens, n, h, w, ctypes.c_void_p(out_u8.data_ptr()), out_u8.stride(0) if n > 1 else h * w * 3,
                                                    ctypes.c_void_p(status.data_ptr()), self._stream_ptr(stream)))
        return out_u8, status

    def decode_jpeg_device(self, files, out_u8=None, stream=None):
        """list of N <= max_batch files (bytes) of one planned size -> (cuda uint8 [N,h,w,3], cuda int32 [N] status words, 0 = ok),
        asynchronous on the stream.  out_u8: a cuda uint8 [N,h,w,3] tensor or a view of one whose images are dense (h*w*3 bytes)."""
        import torch
        files = [bytes(f) for f in files]
        plans = [self.decode_jpeg_plan_reason(f)[0] for f in files]
        if not files or any(p is None for p in plans) or len({p[:2] for p in plans}) != 1:
            raise EngineError(_lib.IRE_ERR_INVALID_INPUT, "invalid input: decode_jpeg_device takes files of one planned size")
        n, (h, w, _) = len(files), plans[0]
        if out_u8 is None:
            out_u8 = torch.empty((n, h, w, 3), dtype=torch.uint8, device="cuda")
        assert out_u8.is_cuda and out_u8.dtype == torch.uint8 and tuple(out_u8.shape) == (n, h, w, 3) and out_u8[0].is_contiguous()
        status = torch.empty(n, dtype=torch.int32, device=out_u8.device)
        ptrs = (ctypes.c_char_p * n)(*files)
        lens = (ctypes.c_size_t * n)(*[len(f) for f in files])
        self._check(self._lib.ire_decode_jpeg_device(self._h, ptrs, lens, n, h, w, ctypes.c_void_p(out_u8.data_ptr()), out_u8.stride(0) if n > 1 else h * w * 3,
                                                     ctypes.c_void_p(status.data_ptr()), self._stream_ptr(stream)))
        return out_u8, status

    def encode_png_base64(self, rgb):
        """[N,H,W,3] (or [H,W,3]) uint8 -> list of N `bytes` (one for a single image): the base64 text of a PNG file of each image,
        encoded on the device (stored deflate blocks: every PNG decoder reads it)."""
        single = np.asarray(rgb).ndim == 3
        x = self._as_batch(rgb)
        n, h, w, _ = x.shape
        cb = self.png_base64_bytes(h, w)
        if cb == 0:
            raise EngineError(_lib.IRE_ERR_INVALID_INPUT, "invalid image size for the PNG encoder: width must be a multiple of 8")
        stride = (cb + 15) // 16 * 16
        out = np.empty((n, stride), np.uint8)
        self._check(self._lib.ire_encode_png_base64(self._h, _ptr(x), n, h, w, _ptr(out), stride))
        res = [out[i, :cb].tobytes() for i in range(n)]
        return res[0] if single else res

    def encode_png_base64_tensor(self, rgb_u8, stream=None):
        """cuda uint8 [N,H,W,3] -> cuda uint8 [N, chars] ASCII (asynchronous on the stream)."""
        import torch
        n, h, w, _ = rgb_u8.shape
        cb = self.png_base64_bytes(h, w)
        out = torch.empty((n, cb), dtype=torch.uint8, device=rgb_u8.device)
        self._check(self._lib.ire_encode_png_base64_device(self._h, ctypes.c_void_p(rgb_u8.data_ptr()), n, h, w, ctypes.c_void_p(out.data_ptr()), cb,
                                                           self._stream_ptr(stream)))
        return out

    def png_base64_bytes_fit(self, h, w):
        return int(self._lib.ire_png_base64_bytes_fit(int(h), int(w)))

    def encode_png_base64_fit(self, rgb):
        """encode_png_base64() for any size (1..8192 per side)."""
        return self._encode_fit("png", rgb)

    def encode_png_base64_fit_tensor(self, rgb_u8, stream=None):
        """cuda uint8 [N,h,w,3], possibly a window `t[:, :h, :w]` of a larger tensor (only the pixel and channel axes have to be
        dense) -> cuda uint8 [N, chars] ASCII; the window is encoded where it lies, its strides go to the engine as pitches."""
        return self._encode_fit_tensor("png", rgb_u8, stream)

    def restore_fit_tensor(self, rgb_u8, out_u8=None, scores=None, is_jpeg_u8=None, stream=None):
        """restore_tensor() for any size (1..8192 per side), asynchronous on the torch stream."""
        import torch
        assert rgb_u8.is_cuda and rgb_u8.dtype == torch.uint8 and rgb_u8.is_contiguous() and rgb_u8.dim() == 4
        n, h, w, _ = rgb_u8.shape
        if out_u8 is None:
            out_u8 = torch.empty_like(rgb_u8)
        sc = ctypes.c_void_p(scores.data_ptr()) if scores is not None else None
        jp = ctypes.c_void_p(is_jpeg_u8.data_ptr()) if is_jpeg_u8 is not None else None
        self._check(self._lib.ire_restore_fit_device(self._h, ctypes.c_void_p(rgb_u8.data_ptr()), n, h, w, sc, jp,
                                                     ctypes.c_void_p(out_u8.data_ptr()), self._stream_ptr(stream)))
        return out_u8

    def release(self, job):
        """Give a submitted job up without fetching it (after a poll() timeout the caller will not repeat): ire_job_release."""
        handle, _, _ = job
        self._check(self._lib.ire_job_release(self._h, handle))

    def affinity(self):
        """(cpulist, numa_node) the engine's service threads are bound to ("" / -1: no binding)."""
        buf = ctypes.create_string_buffer(4096)
        node = ctypes.c_int32(-1)
        self._check(self._lib.ire_engine_affinity(self._h, buf, len(buf), ctypes.byref(node)))
        return buf.value.decode(), int(node.value)

    # ---- device (torch tensors) ---------------------------------------------------------------
    @staticmethod
    def _stream_ptr(stream):
        import torch
        s = stream if stream is not None else torch.cuda.current_stream()
        return ctypes.c_void_p(s.cuda_stream)

    def classify_tensor(self, rgb_u8, is_jpeg_u8=None, stream=None):
        """rgb_u8: cuda uint8 [N,H,W,3] contiguous -> (scores cuda float64 [N,7], labels cuda int32 [N])."""
        import torch
        assert rgb_u8.is_cuda and rgb_u8.dtype == torch.uint8 and rgb_u8.is_contiguous() and rgb_u8.dim() == 4
        n, h, w, _ = rgb_u8.shape
        scores = torch.empty((n, 7), dtype=torch.float64, device=rgb_u8.device)
        labels = torch.empty((n,), dtype=torch.int32, device=rgb_u8.device)
        jp = ctypes.c_void_p(is_jpeg_u8.data_ptr()) if is_jpeg_u8 is not None else None
        self._check(self._lib.ire_classify_device(self._h, ctypes.c_void_p(rgb_u8.data_ptr()), n, h, w, jp,
                                                  ctypes.c_void_p(scores.data_ptr()), ctypes.c_void_p(labels.data_ptr()),
                                                  self._stream_ptr(stream)))
        return scores, labels

    def restore_tensor(self, rgb_u8, out_u8=None, scores=None, is_jpeg_u8=None, stream=None):
        """Asynchronous on the torch stream: classify (unless scores given) + RestoreNet-v0."""
        import torch
        assert rgb_u8.is_cuda and rgb_u8.dtype == torch.uint8 and rgb_u8.is_contiguous() and rgb_u8.dim() == 4
        n, h, w, _ = rgb_u8.shape
        if out_u8 is None:
            out_u8 = torch.empty_like(rgb_u8)
        sc = ctypes.c_void_p(scores.data_ptr()) if scores is not None else None
        jp = ctypes.c_void_p(is_jpeg_u8.data_ptr()) if is_jpeg_u8 is not None else None
        self._check(self._lib.ire_restore_device(self._h, ctypes.c_void_p(rgb_u8.data_ptr()), n, h, w, sc, jp,
                                                 ctypes.c_void_p(out_u8.data_ptr()), self._stream_ptr(stream)))
        return out_u8

    def fuse_tensor(self, views_u8, noise_score=-1.0, stream=None):
        import torch
        assert views_u8.is_cuda and views_u8.dtype == torch.uint8 and views_u8.is_contiguous() and views_u8.dim() == 4
        k, h, w, _ = views_u8.shape
        out = torch.empty((h, w, 3), dtype=torch.uint8, device=views_u8.device)
        shifts = torch.zeros((k, 2), dtype=torch.int32, device=views_u8.device)
        self._check(self._lib.ire_fuse_device(self._h, ctypes.c_void_p(views_u8.data_ptr()), k, h, w, float(noise_score),
                                              ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(shifts.data_ptr()),
                                              self._stream_ptr(stream)))
        return out, shifts

    def fuse_batch_tensor(self, views_u8, noise_scores=None, stream=None):
        """views [B,k,H,W,3] uint8 on the GPU (B <= 16 view sets of one shape) -> (fused [B,H,W,3], shifts [B,k,2]).
        noise_scores: B floats (host), each < 0 / None => classify view 0 of that set inside.  One pass of the kernel chain."""
        import torch
        assert views_u8.is_cuda and views_u8.dtype == torch.uint8 and views_u8.is_contiguous() and views_u8.dim() == 5
        b, k, h, w, _ = views_u8.shape
        ns = (ctypes.c_double * b)(*([-1.0] * b if noise_scores is None else [float(x) for x in noise_scores]))
        out = torch.empty((b, h, w, 3), dtype=torch.uint8, device=views_u8.device)
        shifts = torch.zeros((b, k, 2), dtype=torch.int32, device=views_u8.device)
        self._check(self._lib.ire_fuse_batch_device(self._h, ctypes.c_void_p(views_u8.data_ptr()), b, k, h, w, ns,
                                                    ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(shifts.data_ptr()),
                                                    self._stream_ptr(stream)))
        return out, shifts

    # ---- cfg 4: row strips ----------------------------------------------------------------------
    def restore_tiled_tensor(self, rgb_u8, nstrips, out_u8=None, scores=None, is_jpeg_u8=None, stream=None):
        """One [H,W,3] image restored as `nstrips` row strips on this GPU (virtual ranks: per-level halo exchange and the
        GroupNorm partials gather are in-device copies).  Bit-identical to restore_tensor on the whole image."""
        import torch
        assert rgb_u8.is_cuda and rgb_u8.dtype == torch.uint8 and rgb_u8.is_contiguous() and rgb_u8.dim() == 3
        h, w, _ = rgb_u8.shape
        if out_u8 is None:
            out_u8 = torch.empty_like(rgb_u8)
        sc = ctypes.c_void_p(scores.data_ptr()) if scores is not None else None
        jp = ctypes.c_void_p(is_jpeg_u8.data_ptr()) if is_jpeg_u8 is not None else None
        self._check(self._lib.ire_restore_tiled_device(self._h, ctypes.c_void_p(rgb_u8.data_ptr()), h, w, int(nstrips), sc, jp,
                                                       ctypes.c_void_p(out_u8.data_ptr()), self._stream_ptr(stream)))
        return out_u8

    def open_strips(self, h, w, nstrips_total, first_strip, nlocal=1):
        import weakref
        s = StripSession(self, h, w, nstrips_total, first_strip, nlocal)
        if not hasattr(self, "_sessions"):
            self._sessions = []
        self._sessions = [r for r in self._sessions if r() is not None] + [weakref.ref(s)]
        return s

    # ---- diagnostics --------------------------------------------------------------------------
    def classifier_sums(self, n):
        sums = np.zeros((n, 14), np.uint64)
        self._check(self._lib.ire_debug_classifier_sums(self._h, n, _ptr(sums)))
        return sums

    def debug_poison_scratch(self, byte):
        """Fill every scratch allocation of the process with `byte` (ire_debug_poison_scratch; only under IRE_DEBUG_POISON) -> bytes filled."""
        n = ctypes.c_uint64(0)
        self._check(self._lib.ire_debug_poison_scratch(self._h, int(byte), ctypes.byref(n)))
        return n.value

    def debug_gn_finalize(self, stats, hw, gamma, beta, film=None, film_off=0):
        """GroupNorm partials [nimg, parts, 8, 2] (sum, sum of squares per tile and group) of tensors of `hw` pixels and C = len(gamma)
        channels -> the (A, B) of y = x A + B as [nimg, C, 2] float32, from the standalone finalize kernel (ire_debug_gn_finalize).
        film: [nimg, film_stride] or None; the scale at film_off + c, the shift at film_off + C + c."""
        st = np.ascontiguousarray(stats, dtype=np.float32)
        assert st.ndim == 4 and st.shape[2:] == (8, 2), st.shape
        g, b = (np.ascontiguousarray(v, dtype=np.float32).reshape(-1) for v in (gamma, beta))
        assert g.size == b.size
        fm = None if film is None else np.ascontiguousarray(film, dtype=np.float32)
        assert fm is None or (fm.ndim == 2 and fm.shape[0] == st.shape[0]), "film: one row per image"
        out = np.zeros((st.shape[0], g.size, 2), np.float32)
        self._check(self._lib.ire_debug_gn_finalize(self._h, _ptr(st), st.shape[0], st.shape[1], g.size, int(hw), _ptr(g), _ptr(b), _ptr(fm),
                                                    0 if fm is None else fm.shape[1], int(film_off), _ptr(out)))
        return out

    def debug_capture(self, on=True):
        self._check(self._lib.ire_debug_capture(self._h, int(on)))

    def activation(self, name):
        cnt = ctypes.c_size_t(0)
        self._check(self._lib.ire_debug_activation(self._h, name.encode(), None, ctypes.byref(cnt)))
        out = np.zeros(cnt.value, np.float32)
        self._check(self._lib.ire_debug_activation(self._h, name.encode(), _ptr(out), ctypes.byref(cnt)))
        return out

    def profile_enable(self, mode=1):
        """Low byte: 0 off, 1 every kernel family, 2 the 3x3 conv family only (fewest HIP events); `mode | (N << 8)`: in mode 2
        bracket the launches of every N-th pass of the network only (an event record is a packet between two kernels)."""
        self._check(self._lib.ire_profile_enable(self._h, int(mode)))

    def profile_reset(self):
        self._check(self._lib.ire_profile_reset(self._h))

    def profile_query(self, family="all"):
        ms, n, fl, by = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double(), ctypes.c_double()
        self._check(self._lib.ire_profile_query(self._h, family.encode(), ctypes.byref(ms), ctypes.byref(n),
                                                ctypes.byref(fl), ctypes.byref(by)))
        return {"ms": ms.value, "launches": n.value, "flops": fl.value, "bytes": by.value}

    def profile_report(self):
        """Per-layer-group rows of the profiled convolution launches since the last reset (ire_profile_report)."""
        import json
        need = ctypes.c_size_t(0)
        self._check(self._lib.ire_profile_report(self._h, None, 0, ctypes.byref(need)))
        buf = ctypes.create_string_buffer(need.value + 64)
        self._check(self._lib.ire_profile_report(self._h, buf, len(buf), ctypes.byref(need)))
        return json.loads(buf.value.decode())


class StripSession:
    """One rank's strips of a tiled restoration (include/ire.h "cfg 4"): the layer program runs one op at a time and the host
    moves halo rows / GroupNorm partials between ranks in between (tiled.py).  All buffers the ranks exchange are torch tensors
    owned here: `stats` (the global partials array, all-gathered in place) and four halo staging rows."""

    def __init__(self, engine, h, w, nstrips_total, first_strip, nlocal=1):
        import torch
        self.eng, self._lib = engine, engine._lib
        self.h, self.w, self.total, self.first, self.nlocal = h, w, nstrips_total, first_strip, nlocal
        self.rows = (h // nstrips_total) * nlocal
        dev = torch.device("cuda", torch.cuda.current_device())
        self.stats = torch.zeros(int(self._lib.ire_strips_stats_bytes(h, w)), dtype=torch.uint8, device=dev)
        row_max = w * 32 * 2                       # W_l * C_l * 2 bytes is the same at every level
        self.send_up, self.send_down, self.recv_up, self.recv_down = (torch.zeros(row_max, dtype=torch.uint8, device=dev) for _ in range(4))
        hnd = ctypes.c_void_p()
        self._s = None
        engine._check(self._lib.ire_strips_open(engine._h, h, w, nstrips_total, first_strip, nlocal, ctypes.c_void_p(self.stats.data_ptr()),
                                                ctypes.byref(hnd)))
        self._s = hnd
        self.num_ops = int(self._lib.ire_strips_num_ops(self._s))

    def close(self):
        if getattr(self, "_s", None):
            self._lib.ire_strips_close(self._s)
            self._s = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_input(self, rows_with_halo_u8, scores_f64, stream=None):
        assert rows_with_halo_u8.is_cuda and rows_with_halo_u8.is_contiguous() and tuple(rows_with_halo_u8.shape) == (self.rows + 2, self.w, 3)
        self.eng._check(self._lib.ire_strips_set_input(self._s, ctypes.c_void_p(rows_with_halo_u8.data_ptr()), ctypes.c_void_p(scores_f64.data_ptr()),
                                                       Engine._stream_ptr(stream)))

    def run_op(self, k, stream=None):
        info = _lib.IreStripXchg()
        self.eng._check(self._lib.ire_strips_run_op(self._s, int(k), Engine._stream_ptr(stream), ctypes.byref(info)))
        return info

    def pack_halo(self, k, stream=None):
        self.eng._check(self._lib.ire_strips_pack_halo(self._s, int(k), ctypes.c_void_p(self.send_up.data_ptr()), ctypes.c_void_p(self.send_down.data_ptr()),
                                                       Engine._stream_ptr(stream)))

    def unpack_halo(self, k, stream=None):
        self.eng._check(self._lib.ire_strips_unpack_halo(self._s, int(k), ctypes.c_void_p(self.recv_up.data_ptr()), ctypes.c_void_p(self.recv_down.data_ptr()),
                                                         Engine._stream_ptr(stream)))

    def get_output(self, stream=None):
        import torch
        out = torch.empty((self.rows, self.w, 3), dtype=torch.uint8, device=self.stats.device)
        self.eng._check(self._lib.ire_strips_get_output(self._s, ctypes.c_void_p(out.data_ptr()), Engine._stream_ptr(stream)))
        return out
