"""Host-side mirror of the reference's service layer for the hot path, wired to the engine.

  RestoratorService        <- server-node/src/services/restorator.js:16-319
  EngineClassifier         -> the duck-typed `classifier` seam  {analyze(buffer) -> {7 scores}}
                              (restorator.js:24, classifier.js:40-99)
  EngineRestorer           -> the duck-typed `geminiClient` seam {restore_image(prompt, images,
                              user_context) -> {base64Image, metadata}} (geminiClient.js:32-97)

Same names, argument meaning and error behaviour as the reference (snake_case methods, the
result dict keeps the reference's camelCase keys because it is the wire envelope):
restore() never raises, the error envelope defaults code 'RESTORATION_FAILED', _classify_error
matches substrings, _determine_failure_stage tests the *truthiness* of integer-ms timings
(Appendix B quirk pinned by tests/restoratorService.test.js:77).
The adapters decode/encode on the host (PIL) and hand decoded RGB to the engine; there is no CPU
pixel path: if the engine is unavailable they raise and restore() returns the error envelope.
"""
import base64
import concurrent.futures
import io
import os
import threading
import time
import uuid
from datetime import datetime, timezone

import numpy as np

from . import _lib
from .engine import result_format
from .prompt_enhancer import KEYS, PromptEnhancerService

BATCH_REQUEST_DELAY_MS = float(os.environ.get("RESTORATION_BATCH_DELAY_MS", "0") or 0)  # restorator.js:13
BATCH_CONCURRENCY = max(1, int(float(os.environ.get("RESTORATION_BATCH_CONCURRENCY", "3") or 3)))  # :14


def _now_ms():
    return int(time.time() * 1000)  # Date.now()


# How an upload becomes pixels (IRE_UPLOAD_CODEC, read at each call):
#   unset        host PIL (libjpeg-turbo, libpng, ...): every format, ~5.6 ms of one core per 1024^2 JPEG -- the default
#   jpeg-device  a JPEG the engine's plan accepts (csrc/jpeg_parse.hpp: baseline; progressive too on an engine created with
#                IRE_FLAG_DECODE_PROGRESSIVE) is decoded on the GPU (csrc/jpeg_dec.hip) to the very bytes PIL gives; every other
#                file -- progressive on an engine without that flag, CMYK, PNG, WebP, one the device flags as corrupt -- goes to
#                PIL exactly as above.  A single upload that reaches restore_image undecoded becomes a file job of the engine's
#                batcher (ire_submit_jpeg): decoded with its batch, eight uploads a time
UPLOAD_DECODES = {"device": 0, "host": 0}      # which way the uploads of this process went


def decode_image(buffer, engine=None):
    """encoded bytes -> (rgb uint8 [H,W,3], format str).  sharp(buf) decodes to 8-bit sRGB
    (Appendix A.1); no EXIF rotation inside the classifier (A.2)."""
    from PIL import Image
    # IRE_UPLOAD_CODEC: jpeg-device | png-device (an engine created with decode_png=True) | device (both)
    codec = os.environ.get("IRE_UPLOAD_CODEC")
    is_jpeg = bytes(buffer[:2]) == b"\xff\xd8" and codec in ("jpeg-device", "device")
    is_png = bytes(buffer[:8]) == b"\x89PNG\r\n\x1a\n" and codec in ("png-device", "device")
    if engine is not None and (is_jpeg or is_png):
        from .engine import EngineError
        try:
            # plans inside: a file out of scope or flagged on the device is "invalid input"
            rgb = engine.decode_jpeg(bytes(buffer)) if is_jpeg else engine.decode_png(bytes(buffer))
            UPLOAD_DECODES["device"] += 1
            return rgb, "jpeg" if is_jpeg else "png"
        except EngineError as e:
            if e.status != _lib.IRE_ERR_INVALID_INPUT:   # only that is the host codec's to judge; unavailable / internal go up
                raise
    UPLOAD_DECODES["host"] += 1
    try:
        im = Image.open(io.BytesIO(bytes(buffer)))
        fmt = (im.format or "").lower()
        im = im.convert("RGB")
    except Exception as e:  # noqa: BLE001
        raise ValueError(f"invalid image buffer: {e}") from e
    return np.ascontiguousarray(np.asarray(im, dtype=np.uint8)), fmt


def encode_png_base64(rgb):
    from PIL import Image
    bio = io.BytesIO()
    Image.fromarray(rgb, "RGB").save(bio, format="PNG")
    return base64.b64encode(bio.getvalue()).decode("ascii")


def encode_jpeg_base64(rgb, quality=85):
    """JPEG q85 4:4:4, the reference's own output settings where it encodes (imagePreprocess.js:57-64)."""
    from PIL import Image
    bio = io.BytesIO()
    Image.fromarray(rgb, "RGB").save(bio, format="JPEG", quality=quality, subsampling=0)
    return base64.b64encode(bio.getvalue()).decode("ascii")


# How the restored image becomes the base64 string of restorator.js:108 (IRE_RESULT_CODEC):
#   png         host PIL PNG (zlib level 6): ~0.2 s of one core per 1024^2 photograph -- the default, what round 3 shipped
#   jpeg        host PIL JPEG q85 4:4:4 (the reference's own settings where it encodes: imagePreprocess.js:57-64): ~15 ms
#   png-device  a PNG of stored deflate blocks + its base64 text written by the GPU (csrc/encode.hip): no host codec work at all;
#               with an engine created with IRE_FLAG_RESULT_PNG_BASE64 the batcher hands the text back instead of pixels
#   png-deflate-device  a COMPRESSED PNG (Paeth filter, Huffman-coded deflate blocks) + its base64 text written by the GPU
#               (csrc/deflate.hip): no host codec work either, and a shorter string; the engine flag is IRE_FLAG_RESULT_PNG_DEFLATE
#   jpeg-device  a baseline JPEG (byte for byte what libjpeg-turbo writes with a restart interval of 48 blocks) + its base64 text
#               written by the GPU (csrc/jpeg.hip): no host codec work, and the shortest string; the engine flag is
#               IRE_FLAG_RESULT_JPEG.  IRE_JPEG_QUALITY (1..100) and IRE_JPEG_SUBSAMPLING (0 = 4:4:4, 2 = 4:2:0) choose the file's
#               settings; unset: quality 85 at 4:4:4, the reference's settings.  IRE_JPEG_OPTIMIZE=1: every file carries its image's
#               own Huffman tables (IRE_FLAG_JPEG_OPTIMIZE), as the reference's mozjpeg encode does: a shorter string, the same pixels.
#               IRE_JPEG_PROGRESSIVE=1: every file is a progressive one (IRE_FLAG_JPEG_PROGRESSIVE), the form mozjpeg writes: ten scans,
#               each under its own table -- shorter again, the same pixels
RESULT_CODEC = os.environ.get("IRE_RESULT_CODEC", "png")
JPEG_SETTINGS = (int(os.environ.get("IRE_JPEG_QUALITY") or 0), int(os.environ.get("IRE_JPEG_SUBSAMPLING") or 0))      # (0: the default)
JPEG_OPTIMIZE = (os.environ.get("IRE_JPEG_OPTIMIZE") or "0") not in ("0", "")
JPEG_PROGRESSIVE = (os.environ.get("IRE_JPEG_PROGRESSIVE") or "0") not in ("0", "")


def jpeg_engine_flags(result_codec=None):
    """IRE_FLAG_JPEG_OPTIMIZE and IRE_FLAG_JPEG_PROGRESSIVE where IRE_JPEG_OPTIMIZE / IRE_JPEG_PROGRESSIVE ask for them and the codec
    value's engine flag allows them, to be or-ed to that flag."""
    if (result_codec or RESULT_CODEC) != "jpeg-device":
        return 0
    return (_lib.IRE_FLAG_JPEG_OPTIMIZE if JPEG_OPTIMIZE else 0) | (_lib.IRE_FLAG_JPEG_PROGRESSIVE if JPEG_PROGRESSIVE else 0)


def jpeg_engine_kwargs(result_codec=None):
    """The Engine(...) arguments of the JPEG settings: given only with the codec value whose engine flag allows them."""
    return {"jpeg_quality": JPEG_SETTINGS[0], "jpeg_sampling": JPEG_SETTINGS[1]} if (result_codec or RESULT_CODEC) == "jpeg-device" else {}


class _Seen:
    """What analyze() learnt about a buffer, for the restoreImage() that follows on the SAME object
    (restorator.js:59-94 hands one Buffer to both seams): decoded pixels + the 7 scores, so a job is
    decoded once and classified once.  Keyed by object identity; the entry holds the buffer, which
    keeps the id valid; a handful of entries (in-flight jobs: 3 per batch, 5 per worker)."""

    def __init__(self, capacity=16):
        self._d = {}
        self._cap = capacity
        self._lock = threading.Lock()

    def put(self, buf, rgb, fmt, scores):
        with self._lock:
            if len(self._d) >= self._cap:
                self._d.pop(next(iter(self._d)))
            self._d[id(buf)] = (buf, rgb, fmt, scores)

    def take(self, buf):
        with self._lock:
            hit = self._d.pop(id(buf), None)
        return None if hit is None or hit[0] is not buf else hit[1:]


def _seen_of(engine):
    if getattr(engine, "_seen", None) is None:
        engine._seen = _Seen()
    return engine._seen


class EngineClassifier:
    """classifier seam: analyze(imageBuffer) -> {blur, noise, lowLight, compression, scratch, fade, colorShift}."""

    def __init__(self, engine, logger=None):
        self.engine = engine
        self.logger = logger

    def analyze(self, image_buffer):
        rgb, fmt = decode_image(image_buffer, self.engine)
        scores, _ = self.engine.classify(rgb, is_jpeg=(fmt == "jpeg"))
        _seen_of(self.engine).put(image_buffer, rgb, fmt, scores[0].copy())
        return {k: float(scores[0, i]) for i, k in enumerate(KEYS)}


class EngineRestorer:
    """geminiClient seam: restore_image(prompt, images, user_context) -> {base64Image, metadata}."""

    def __init__(self, engine, logger=None, result_codec=None):
        self.engine = engine
        self.logger = logger
        self.result_codec = result_codec or RESULT_CODEC

    def _encode(self, result):
        if self.result_codec == "jpeg":
            return encode_jpeg_base64(result)
        if self.result_codec == "png-device":
            return self.engine.encode_png_base64_fit(result).decode("ascii")      # any width: the device encoder
        if self.result_codec == "png-deflate-device":
            return self.engine.encode_png_deflate_base64_fit(result).decode("ascii")
        if self.result_codec == "jpeg-device":      # a JPEG engine's own settings; on any other engine the environment's
            own = getattr(self.engine, "_flags", 0) & _lib.IRE_FLAG_RESULT_JPEG
            return self.engine.encode_jpeg_base64_fit(result, *((None, None, None, None) if own else JPEG_SETTINGS + (JPEG_OPTIMIZE, JPEG_PROGRESSIVE))).decode("ascii")
        return encode_png_base64(result)

    @staticmethod
    def _reply(text):
        return {"base64Image": text,
                "metadata": {"providerRequestId": f"ire-{uuid.uuid4()}", "billedTokens": None, "estimatedCostUsd": 0}}

    def restore_image(self, prompt, images, user_context=None):
        if not images or len(images) > 3:
            raise ValueError("invalid images: expected 1..3 encoded images")  # provider limit: report.md:28
        seen = _seen_of(self.engine)
        text_engine = result_format(getattr(self.engine, "_flags", 0)) is not None      # poll returns the text
        if len(images) == 1 and os.environ.get("IRE_UPLOAD_CODEC") == "jpeg-device" and bytes(images[0][:2]) == b"\xff\xd8":
            # a single upload that analyze() has not decoded goes to the batcher as the FILE it is (ire_submit_jpeg): parsed here,
            # decoded on the device with its batch.  A file the plan refuses (at submit) or the device flags (at poll) is "invalid
            # input": the host codec then judges it, below, exactly as before
            hit = seen.take(images[0])
            if hit is None:
                from .engine import EngineError
                try:
                    out, _, _ = self.engine.poll(self.engine.submit_jpeg(bytes(images[0])))
                    UPLOAD_DECODES["device"] += 1
                    return self._reply(out.decode("ascii") if text_engine else self._encode(out))
                except EngineError as e:
                    if e.status != _lib.IRE_ERR_INVALID_INPUT:
                        raise
                hit = (*decode_image(images[0]), None)          # (no engine: straight to the host codec, which is where the refusal sends it)
            decoded = [hit]
            images = []
        else:
            decoded = []
        for b in images:             # analyze() already decoded and classified this buffer: reuse both
            hit = seen.take(b)
            decoded.append(hit if hit is not None else (*decode_image(b, self.engine), None))
        shapes = {d[0].shape for d in decoded}
        if len(shapes) != 1:
            raise ValueError("invalid images: fusion views must have identical dimensions")
        if len(decoded) == 1:
            # one image of any size is ONE job of the engine's batcher (ire_submit_fit): the engine pads on the device, classifies
            # the image's own pixels in the same batch when analyze() did not, and hands back the h x w window -- on a flagged
            # engine as the text of its PNG, which IS the result for every size
            rgb, fmt, scores = decoded[0]
            out, _, _ = self.engine.poll(self.engine.submit_fit(rgb, is_jpeg=(fmt == "jpeg"), scores=scores))
            return self._reply(out.decode("ascii") if text_engine else self._encode(out))
        # 2..3 views are ONE fusion job of the engine's batcher (ire_submit_fuse_fit): every view restored as a single job would be (its
        # own scores from analyze() where it ran, else classified in the batch), the views fused on the device, the h x w result
        # polled -- on a flagged engine as its text, which IS the reply.  No host pad, decode, crop or second encode.
        job = self.engine.submit_fuse_fit([d[0] for d in decoded], is_jpeg=[d[1] == "jpeg" for d in decoded], scores=[d[2] for d in decoded])
        out, _, _ = self.engine.poll(job)
        return self._reply(out.decode("ascii") if text_engine else self._encode(out))


class RestoratorService:
    """restorator.js:16-319."""

    def __init__(self, gemini_client=None, logger=None, engine=None):
        if gemini_client is None and engine is not None:
            gemini_client = EngineRestorer(engine, logger)
        if not gemini_client:
            raise ValueError("RestoratorService requires a geminiClient")  # restorator.js:18-20
        self.gemini_client = gemini_client
        self.logger = logger
        # public, replaceable by assignment like the reference's (restorator.js:24-25)
        self.classifier = EngineClassifier(engine, logger) if engine is not None else None
        self.prompt_enhancer = PromptEnhancerService(logger)

    # -- restorator.js:37-172 -----------------------------------------------------------------
    def restore(self, image_buffer, user_prompt=None, user_context=None, options=None):
        options = {} if options is None else options
        start = _now_ms()
        timings = {}
        try:
            t0 = _now_ms()
            if self.classifier is None:
                raise RuntimeError("service unavailable: no classifier configured")
            degradation = self.classifier.analyze(image_buffer)
            timings["classify_ms"] = _now_ms() - t0

            t0 = _now_ms()
            enhanced_prompt = self.prompt_enhancer.enhance(degradation=degradation, user_prompt=user_prompt,
                                                           options=options)
            timings["prompt_ms"] = _now_ms() - t0

            t0 = _now_ms()
            result = self.gemini_client.restore_image(prompt=enhanced_prompt, images=[image_buffer],
                                                      user_context=user_context)
            timings["restore_ms"] = _now_ms() - t0
            timings["total_ms"] = _now_ms() - start
            md = result["metadata"]
            return {
                "success": True,
                "restoredImage": result["base64Image"],
                "degradationAnalysis": degradation,
                "enhancedPrompt": enhanced_prompt,
                "timings": timings,
                "metadata": {
                    "providerRequestId": md.get("providerRequestId"),
                    "estimatedCostUsd": md.get("estimatedCostUsd"),
                    "billedTokens": md.get("billedTokens"),
                    "processingTime": timings["total_ms"],
                    "classificationIssues": [{"type": k, "confidence": v} for k, v in degradation.items() if v > 0.3],
                },
            }
        except Exception as error:  # noqa: BLE001 -- restore never raises (restorator.js:141-167)
            timings["total_ms"] = _now_ms() - start
            if self.logger is not None:
                self.logger.error("[restorator] Restoration failed: %s", error)
            return {
                "success": False,
                "error": {"message": str(error), "code": getattr(error, "code", None) or "RESTORATION_FAILED",
                          "type": self._classify_error(error)},
                "timings": timings,
                "metadata": {"processingTime": timings["total_ms"],
                             "failureStage": self._determine_failure_stage(timings)},
            }

    # -- restorator.js:181-236 ----------------------------------------------------------------
    def restore_batch(self, images, user_prompt=None, user_context=None, options=None):
        options = {} if options is None else options

        def task(index, buf):
            if BATCH_REQUEST_DELAY_MS > 0 and index > 0:
                time.sleep(BATCH_REQUEST_DELAY_MS / 1000.0)
            return self.restore(buf, user_prompt, user_context,
                                {**options, "batchIndex": index, "batchSize": len(images)})

        with concurrent.futures.ThreadPoolExecutor(max_workers=BATCH_CONCURRENCY) as ex:
            futs = [ex.submit(task, i, b) for i, b in enumerate(images)]
            return [f.result() for f in futs]  # same order as the input

    # -- restorator.js:241-265 ----------------------------------------------------------------
    @staticmethod
    def _classify_error(error):
        message = str(error).lower()
        if "rate limit" in message or "429" in message:
            return "RATE_LIMIT_EXCEEDED"
        if "timeout" in message or "etimedout" in message:
            return "TIMEOUT"
        if "invalid" in message or "400" in message:
            return "INVALID_INPUT"
        if "unauthorized" in message or "401" in message:
            return "AUTHENTICATION_FAILED"
        if "service unavailable" in message or "503" in message:
            return "SERVICE_UNAVAILABLE"
        return "UNKNOWN_ERROR"

    # -- restorator.js:270-284 (truthiness of ms values, 0 ms counts as "not run") ---------------
    @staticmethod
    def _determine_failure_stage(timings):
        if timings.get("classify_ms") and not timings.get("prompt_ms"):
            return "PROMPT_ENHANCEMENT"
        if timings.get("prompt_ms") and not timings.get("restore_ms"):
            return "AI_RESTORATION"
        if not timings.get("classify_ms"):
            return "CLASSIFICATION"
        return "UNKNOWN"

    # -- restorator.js:289-314 ----------------------------------------------------------------
    def get_health_status(self):
        """The reference probes the classifier with a 100-byte zero buffer, which sharp cannot
        decode, so it reports classifier=False there; kept, plus an explicit
        engine entry so /health/ready can tell "bad probe" from "no GPU"."""
        try:
            try:
                self.classifier.analyze(bytes(100))
                ok = True
            except Exception:  # noqa: BLE001
                ok = False
            engine_ok, metrics = False, None
            try:
                eng = getattr(self.classifier, "engine", None)
                if eng is not None:
                    eng.classify(np.zeros((16, 16, 3), np.uint8))
                    engine_ok = True
                    metrics = eng.stats()            # images/sec gauge + batch counters
            except Exception:  # noqa: BLE001
                engine_ok = False
            out = {"healthy": ok, "services": {"classifier": ok, "promptEnhancer": True, "geminiClient": True,
                                               "engine": engine_ok},
                   "timestamp": datetime.now(timezone.utc).isoformat()}
            if metrics is not None:
                out["metrics"] = {"engine": metrics}
            return out
        except Exception as e:  # noqa: BLE001
            return {"healthy": False, "error": str(e), "timestamp": datetime.now(timezone.utc).isoformat()}


def create_restorator_service(gemini_client=None, logger=None, engine=None):
    return RestoratorService(gemini_client=gemini_client, logger=logger, engine=engine)
