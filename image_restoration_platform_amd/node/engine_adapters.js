// engine_adapters.js -- the two duck-typed seams of the reference's RestoratorService, backed by the
// MI355X engine through the N-API shim (ire_napi.node -> libire.so, include/ire.h).
//
//   createEngineClassifier(opts) -> { analyze(imageBuffer) -> Promise<{blur,noise,lowLight,compression,scratch,fade,colorShift}> }
//       stands in for ClassifierService            server-node/src/services/classifier.js:40-99
//   createEngineRestorer(opts)   -> { restoreImage({prompt, images, userContext}) -> Promise<{base64Image, metadata}> }
//       stands in for GeminiClient.restoreImage     server-node/src/clients/geminiClient.js:32-97
//
// Wiring in the reference (the swap point, server-node/src/context/services.js:56-59):
//     const restorer = createEngineRestorer({ engine });
//     const svc = new RestoratorService({ geminiClient: restorer, logger });
//     svc.classifier = createEngineClassifier({ engine });      // public mutable property, restorator.js:24
//
// The engine consumes decoded RGB; `decode(buffer) -> Promise<{data:Buffer(RGB), width, height, format}>` and
// `encode({data,width,height}) -> Promise<Buffer>` are injected.  In the reference deployment they are two
// lines of sharp (see defaultCodec below); tests inject a raw codec because sharp is not installable offline.
// CommonJS + no optional chaining on purpose: it must also load on the Node 12 that ships in the build image.
'use strict';
const path = require('path');

const KEYS = ['blur', 'noise', 'lowLight', 'compression', 'scratch', 'fade', 'colorShift']; // classifier.js:62-70

function loadAddon() {
  return require(path.join(__dirname, 'ire_napi.node'));
}

function createEngine(opts) {
  opts = opts || {};
  const addon = opts.addon || loadAddon();
  const lib = opts.libPath || path.join(__dirname, '..', 'lib', 'libire.so');
  // throws Error('service unavailable: ...') when there is no gfx950 device: there is no CPU fallback
  // resultCodec 'png-device': the engine's batcher returns every result as the base64 TEXT of a PNG file encoded on the GPU
  // (IRE_FLAG_RESULT_PNG_BASE64; csrc/encode.hip) -- the string restorator.js:108 puts on the wire, with no sharp encode and no
  // Buffer.toString('base64') (1.03 ms of the one JS thread per 1024^2 result) left for this process
  const textResults = opts.resultCodec === 'png-device';
  const handle = addon.init(lib, opts.weightsPath || '', opts.deviceIndex || 0, opts.maxBatch || 8, opts.numStreams || 0, textResults ? 1 : 0);
  // seen: Buffer -> {decoded, scores}: RestoratorService hands the SAME Buffer object first to classifier.analyze and then to
  // geminiClient.restoreImage (restorator.js:59-94); remembering it here means one decode and one classification per job
  return { addon, handle, seen: new WeakMap(), textResults };
}

function defaultCodec() {
  const sharp = require('sharp'); // reference dependency (package.json:37); resolved lazily
  return {
    decode: async (buf) => {
      const img = sharp(buf);
      const meta = await img.metadata();
      const raw = await img.removeAlpha().toColourspace('srgb').raw().toBuffer({ resolveWithObject: true });
      return { data: raw.data, width: raw.info.width, height: raw.info.height, format: meta.format };
    },
    encode: async (o) => sharp(o.data, { raw: { width: o.width, height: o.height, channels: 3 } }).png().toBuffer(),
  };
}

function padToMultipleOf8(img) {
  // RestoreNet has three stride-2 levels: replicate-pad H and W up to multiples of 8 (>= 16), crop afterwards
  const W = Math.max(16, Math.ceil(img.width / 8) * 8), H = Math.max(16, Math.ceil(img.height / 8) * 8);
  if (W === img.width && H === img.height) return { data: img.data, width: W, height: H };
  const out = Buffer.alloc(W * H * 3);
  for (let y = 0; y < H; y++) {
    const sy = Math.min(y, img.height - 1);
    for (let x = 0; x < W; x++) {
      const sx = Math.min(x, img.width - 1);
      img.data.copy(out, (y * W + x) * 3, (sy * img.width + sx) * 3, (sy * img.width + sx) * 3 + 3);
    }
  }
  return { data: out, width: W, height: H };
}

function crop(data, W, w, h) {
  if (W === w) return data.slice(0, w * h * 3);
  const out = Buffer.alloc(w * h * 3);
  for (let y = 0; y < h; y++) data.copy(out, y * w * 3, y * W * 3, y * W * 3 + w * 3);
  return out;
}

function createEngineClassifier(opts) {
  const engine = opts.engine;
  const codec = opts.codec || defaultCodec();
  return {
    async analyze(imageBuffer) {
      const img = await codec.decode(imageBuffer); // rejects on undecodable input -> failureStage CLASSIFICATION
      const flags = Buffer.from([img.format === 'jpeg' ? 1 : 0]); // classifier.js:180 branches on the container
      const r = await engine.addon.classifyAsync(engine.handle, img.data, 1, img.height, img.width, flags);
      if (engine.seen && Buffer.isBuffer(imageBuffer)) engine.seen.set(imageBuffer, { decoded: img, scores: Float64Array.from(r.scores.slice(0, 7)) });
      const out = {};
      KEYS.forEach((k, i) => { out[k] = r.scores[i]; });
      return out;
    },
  };
}

let jobCounter = 0;
function createEngineRestorer(opts) {
  const engine = opts.engine;
  const codec = opts.codec || defaultCodec();
  const timeoutMs = opts.timeoutMs || 120000;     // the reference's provider timeout class (geminiClient.js: a hung call surfaces as TIMEOUT)
  return {
    async restoreImage(args) {
      const images = args.images;
      if (!images || images.length < 1 || images.length > 3) throw new Error('invalid images: expected 1..3 encoded images');
      const decoded = [], known = [];
      for (const b of images) {           // analyze() already decoded and classified this Buffer: reuse both
        const hit = engine.seen && Buffer.isBuffer(b) ? engine.seen.get(b) : undefined;
        known.push(hit ? hit.scores : null);
        decoded.push(hit ? hit.decoded : await codec.decode(b));
      }
      const w = decoded[0].width, h = decoded[0].height;
      if (decoded.some((d) => d.width !== w || d.height !== h)) throw new Error('invalid images: fusion views must have identical dimensions');
      const reply = (base64Image) => {
        jobCounter += 1;
        return { base64Image, metadata: { providerRequestId: 'ire-' + process.pid + '-' + jobCounter, billedTokens: null, estimatedCostUsd: 0 } };
      };
      if (decoded.length === 1) {
        // one image of any size is ONE job of the engine's batcher (ire_submit_fit): the engine pads on the device, classifies the
        // image's own pixels in the same batch when analyze() did not, and hands back the h x w window -- with textResults as the
        // text of its PNG, which IS the result for every size (a one-byte-per-character string: no transcoding)
        const d = decoded[0];
        const flags = Buffer.from([d.format === 'jpeg' ? 1 : 0]);
        const outBytes = engine.textResults ? engine.addon.pngBase64BytesFit(h, w) : 0;
        const r = await engine.addon.restoreFitAsync(engine.handle, d.data, 1, h, w, flags, known[0] || null, timeoutMs, outBytes);
        if (engine.textResults) return reply(r.pixels.latin1Slice(0, r.pixels.length));
        return reply((await codec.encode({ data: r.pixels, width: w, height: h })).toString('base64'));
      }
      // every view is queued with the engine's batcher at once (ire_submit on this thread, ire_poll on the libuv pool): the
      // views of one call and the single-image jobs of the other in-flight calls (3 per batch, 5 per worker) share engine batches
      let W = w, H = h;
      const pending = decoded.map(async (d, i) => {
        const p = padToMultipleOf8(d);
        W = p.width; H = p.height;
        const flags = Buffer.from([d.format === 'jpeg' ? 1 : 0]);
        let scores = known[i];
        if (!scores && (p.width !== d.width || p.height !== d.height)) {
          // the conditioning scores are those of the image itself (what analyze() reports), never of its replicate-padded copy
          scores = Float64Array.from((await engine.addon.classifyAsync(engine.handle, d.data, 1, d.height, d.width, flags)).scores.slice(0, 7));
        }
        // scores known: not classified again; null: classifies inside.  timeoutMs bounds the wait for the engine's batch: a wedged
        // engine rejects with code ENGINE_TIMEOUT ("timeout: ..." -> TIMEOUT in _classifyError) instead of hanging the promise
        const outBytes = engine.textResults ? engine.addon.pngBase64Bytes(p.height, p.width) : 0;
        return engine.addon.restoreAsync(engine.handle, p.data, 1, p.height, p.width, flags, scores || null, timeoutMs, outBytes);
      });
      let restored = (await Promise.all(pending)).map((r) => r.pixels);
      if (engine.textResults) {
        // fusion needs the views' pixels again: the stored-block PNG inflates at memcpy speed
        restored = await Promise.all(restored.map(async (t) => (await codec.decode(Buffer.from(t.latin1Slice(0, t.length), 'base64'))).data));
      }
      if (H < 64 || W < 64) throw new Error('invalid images: fusion needs at least 64x64 pixels');
      const r = await engine.addon.fuseAsync(engine.handle, Buffer.concat(restored), restored.length, H, W, null, -1.0);
      return reply((await codec.encode({ data: crop(r.pixels, W, w, h), width: w, height: h })).toString('base64'));
    },
  };
}

// SURVEY 8(f) row 4.  Two shapes the reference already has:
//  * checkEngine(): a dependency probe in the form healthRouter.js:4-73 uses ({info, ok[, degraded]}), to be listed beside
//    redis / firestore / gcs in GET /health/ready (healthRouter.js:80-117): the deployer adds `engine: engineStatus.info` to
//    `dependencies` and engineStatus to the two `.some(...)` lists (INTEGRATION.md section 1);
//  * metrics(): the images/sec gauge and batch counters, to sit beside `metrics.requests` in the same payload.
// The probe classifies a 16x16 black image on the GPU (~0.1 ms): it tells "no device / library" (unavailable) from "idle".
function createEngineHealth(opts) {
  const engine = opts.engine;
  const probe = Buffer.alloc(16 * 16 * 3);
  function metrics() {
    const s = engine.addon.stats(engine.handle);
    return { imagesPerSec: s.imagesPerSec, images: s.images, batches: s.batches, lastBatch: s.lastBatch, maxBatch: s.maxBatch, queueDepth: s.queueDepth };
  }
  async function checkEngine() {
    const info = { status: 'ok', device: 'gfx950' };
    try {
      await engine.addon.classifyAsync(engine.handle, probe, 1, 16, 16, Buffer.from([0]));
      Object.assign(info, metrics());
      if (info.queueDepth > 4 * info.maxBatch) { info.status = 'degraded'; info.reason = 'engine queue is backing up'; return { info, ok: true, degraded: true }; }
      return { info, ok: true };
    } catch (error) {
      info.status = 'unavailable';
      info.error = error && error.message;
      return { info, ok: false };
    }
  }
  return { checkEngine, metrics };
}

module.exports = { KEYS, createEngine, createEngineClassifier, createEngineRestorer, createEngineHealth, padToMultipleOf8 };
