// Any-size jobs through the Node seam: restoreImage with one ragged image is ONE batcher job of the engine (ire_submit_fit) -- no JS
// padding loop, no classifier-only call, no decode-again of the device's PNG.  Usage: node test_fit.js <case.json>; one JSON line.
// The codec is the raw one of test_adapters.js ("RAW1" + u16 width + u16 height + u8 isJpeg + RGB).
'use strict';
const fs = require('fs');
const crypto = require('crypto');
const ad = require('./engine_adapters.js');

const rawCodec = {
  decode: async (buf) => {
    if (buf.length < 9 || buf.toString('ascii', 0, 4) !== 'RAW1') throw new Error('Input buffer contains unsupported image format');
    const w = buf.readUInt16LE(4), h = buf.readUInt16LE(6);
    return { data: buf.slice(9, 9 + w * h * 3), width: w, height: h, format: buf[8] ? 'jpeg' : 'png' };
  },
  encode: async (o) => Buffer.concat([Buffer.from('RAW1'), Buffer.from([o.width & 255, o.width >> 8, o.height & 255, o.height >> 8, 0]), o.data]),
};
const sha = (b, enc) => crypto.createHash('sha256').update(b, enc).digest('hex');

(async () => {
  const spec = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
  const out = {};
  const img = fs.readFileSync(spec.image);
  // pixels: an unflagged engine returns the cropped window
  const engine = ad.createEngine({ weightsPath: spec.weights, maxBatch: 8 });
  const restorer = ad.createEngineRestorer({ engine, codec: rawCodec });
  const hl = ad.createEngineHealth({ engine });
  let s0 = hl.metrics();
  const r = await restorer.restoreImage({ prompt: 'p', images: [Buffer.from(img)] });
  out.pixels = { sha: sha(Buffer.from(r.base64Image, 'base64').slice(9)), batches: hl.metrics().batches - s0.batches };
  // text: resultCodec 'png-device' -- the device's text is the result for a ragged size too
  const engine2 = ad.createEngine({ weightsPath: spec.weights, maxBatch: 8, resultCodec: 'png-device' });
  const restorer2 = ad.createEngineRestorer({ engine: engine2, codec: rawCodec });
  const hl2 = ad.createEngineHealth({ engine: engine2 });
  s0 = hl2.metrics();
  const tr = await restorer2.restoreImage({ prompt: 'p', images: [Buffer.from(img)] });
  out.text = { chars: tr.base64Image.length, want: engine2.addon.pngBase64BytesFit(spec.h, spec.w), sha: sha(tr.base64Image, 'latin1'),
               head: Buffer.from(tr.base64Image.slice(0, 16), 'base64').toString('latin1').slice(1, 4), batches: hl2.metrics().batches - s0.batches };
  // 8 in flight share engine batches
  s0 = hl2.metrics();
  const rs = await Promise.all(Array.from({ length: 8 }, () => restorer2.restoreImage({ prompt: 'p', images: [Buffer.from(img)] })));
  out.concurrent = { batches: hl2.metrics().batches - s0.batches, allEqual: rs.every((x) => x.base64Image === tr.base64Image) };
  out.alignedRule = { bytes: engine2.addon.pngBase64Bytes(spec.h, spec.w) };     // the aligned entry keeps its rule: 0 for a ragged width
  console.log(JSON.stringify(out));
})().catch((e) => { console.log(JSON.stringify({ fatal: e.message })); process.exit(1); });
