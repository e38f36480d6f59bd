/*
 * ire.h -- C ABI of libire.so, the MI355X-native image-restoration engine.
 *
 * This is the drop-in boundary for the reference's queue-worker hot path
 * (degradation classification -> restoration -> optional <=3-image fusion).
 * The reference has no FFI of its own; its seams are two
 * duck-typed JS objects, and every entry point below names the reference
 * interface it stands behind:
 *
 *   ire_classify*  <- ClassifierService.analyze(Buffer) -> {7 scores}
 *                     server-node/src/services/classifier.js:40-99
 *                     (+ the ranking derived in promptEnhancer.js:121-136)
 *   ire_restore*   <- GeminiClient.restoreImage({prompt, images:[buf], userContext})
 *                     server-node/src/clients/geminiClient.js:32-97, called from
 *                     server-node/src/services/restorator.js:88-94
 *   ire_fuse*      <- the same restoreImage seam with images.length in 2..3
 *                     (geminiClient.js:32,49; docs only: image-restoration-platform.md:787-857)
 *   ire_submit/ire_poll <- restoreBatch's in-flight promises
 *                     server-node/src/services/restorator.js:181-236 (p-limit 3)
 *
 * Conventions: plain pointers and sizes only; the caller owns every buffer; the
 * engine never keeps an input pointer past return (past ire_poll completion for
 * ire_submit); one engine may be used from several threads; no exceptions cross
 * the ABI.  Every call returns an ire_status; ire_last_error() gives the
 * thread-local message.  Messages of IRE_ERR_INVALID_INPUT / _TIMEOUT /
 * _UNAVAILABLE contain "invalid" / "timeout" / "service unavailable", so the
 * reference's RestoratorService._classifyError (restorator.js:241-265) maps
 * them the way it maps provider errors; IRE_ERR_INTERNAL messages start with
 * "internal:" and fall through to UNKNOWN_ERROR there, which is how the
 * reference treats a provider error it does not recognise (restorator.js:262-264).  Images are decoded 8-bit sRGB, NHWC interleaved RGB
 * (what sharp(buf).raw() yields: SURVEY.md Appendix A.1); decode/encode lives
 * in the host adapters.  There is NO CPU fallback: without a gfx950 device
 * ire_init fails with IRE_ERR_UNAVAILABLE.
 */
#ifndef IRE_H
#define IRE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IRE_ABI_VERSION 3   /* 3: ire_job_release, ire_affinity_plan, ire_engine_affinity, ire_profile_report, ire_encode_png_base64*, IRE_FLAG_RESULT_PNG_BASE64; ire_profile_enable mode bits 8..; ire_config.flags checked */

typedef enum ire_status {
    IRE_OK = 0,
    IRE_ERR_INVALID_INPUT = 1, /* message contains "invalid"             -> INVALID_INPUT       */
    IRE_ERR_TIMEOUT = 2,       /* message contains "timeout"             -> TIMEOUT             */
    IRE_ERR_UNAVAILABLE = 3,   /* message contains "service unavailable" -> SERVICE_UNAVAILABLE */
    IRE_ERR_INTERNAL = 4
} ire_status;

/* BF16: bf16 storage and MFMA operands, fp32 accumulate.  FP8 (cfg 4 of BASELINE.json): the C >= 128 ResBlock convolutions
 * take OCP e4m3 MFMA operands -- weights quantised per output channel at load, activations while staging -- everything
 * else as BF16; stated tolerance vs the fp32 oracle: max |d| <= 6/255, PSNR >= 38 dB. */
enum { IRE_PRECISION_BF16 = 0, IRE_PRECISION_FP8 = 1 };

/* Score order = the object-literal order of classifier.js:62-70. */
enum { IRE_SCORE_BLUR = 0, IRE_SCORE_NOISE, IRE_SCORE_LOWLIGHT, IRE_SCORE_COMPRESSION,
       IRE_SCORE_SCRATCH, IRE_SCORE_FADE, IRE_SCORE_COLORSHIFT, IRE_NUM_SCORES };

typedef struct ire_engine ire_engine;

typedef struct ire_config {
    uint32_t struct_size;     /* = sizeof(ire_config); lets the struct grow: a caller built
                                 before the two JPEG fields passes its smaller size, and the
                                 fields it does not have read as 0                        */
    int32_t device_index;     /* HIP device ordinal (one engine = one GPU = one process) */
    int32_t precision;        /* IRE_PRECISION_BF16 | IRE_PRECISION_FP8                  */
    int32_t max_batch;        /* images per call, 1..64 (default 8 when 0)               */
    int32_t num_streams;      /* images restored concurrently on separate HIP streams
                                 (default 0 = engine's choice)                           */
    const char* weights_path; /* RestoreNet-v0 weight file (DESIGN.md "weight file");
                                 NULL: classify/fuse only until ire_load_weights         */
    uint32_t flags;           /* IRE_FLAG_* bits; unknown bits are rejected               */
    int32_t jpeg_quality;     /* with IRE_FLAG_RESULT_JPEG: 1..100, IJG scaling of the Annex K
                                 tables (what libjpeg and Pillow call quality); 0: 85     */
    int32_t jpeg_sampling;    /* with IRE_FLAG_RESULT_JPEG: 0 = 4:4:4, 2 = 4:2:0, numbered as
                                 ire_decode_jpeg_plan numbers it.  Anything else in either
                                 field, or either set without the flag, is invalid        */
} ire_config;
/* The batcher (ire_submit / ire_poll) delivers every result as the base64 TEXT of a PNG file of the restored image, encoded
 * on the device (ire_encode_png_base64_device below), instead of raw pixels: ire_poll's out_rgb then receives
 * ire_png_base64_bytes_fit(h, w) ASCII characters -- the string restorator.js:108 puts on the wire, with no codec or base64 work
 * left for the host. */
#define IRE_FLAG_RESULT_PNG_BASE64 1u
/* The batcher delivers every result as the base64 text of a COMPRESSED PNG file (Paeth-filtered scanlines, Huffman-coded deflate
 * blocks: ire_encode_png_deflate_base64_fit_device below).  The text's length depends on the pixels: such results are fetched with
 * ire_poll_text, into a buffer of ire_png_deflate_base64_bound(h, w) bytes.  Bit value 2 is not a flag; setting both result flags
 * is invalid. */
#define IRE_FLAG_RESULT_PNG_DEFLATE 4u
/* The batcher delivers every result as the base64 text of a baseline JPEG file (ire_encode_jpeg_base64_fit_device_ex below) at
 * ire_config.jpeg_quality and jpeg_sampling; left 0 that is quality 85 at 4:4:4, the reference's own settings
 * (imagePreprocess.js:57-64).  The text's length depends on the pixels: such results are fetched with ire_poll_text, into a buffer
 * of ire_jpeg_base64_bound_ex(h, w, quality, sampling) bytes (ire_jpeg_base64_bound(h, w) for the default).  At most one result
 * flag may be set. */
#define IRE_FLAG_RESULT_JPEG 8u
/* Not a result format, and free to combine with one: ire_decode_jpeg, ire_decode_jpeg_device and ire_submit_jpeg accept PROGRESSIVE
 * JPEG files (ire_decode_jpeg_plan_ex with IRE_DECODE_ACCEPT_PROGRESSIVE) beside baseline ones, in one batch where their planned
 * sizes are equal.  Without it such a file is refused as before and stays with the host codec.  (Bit value 16 stays unknown, as 2
 * does: tests/test_jpeg_model.py holds it to that.) */
#define IRE_FLAG_DECODE_PROGRESSIVE 32u
/* Not a result format: valid only together with IRE_FLAG_RESULT_JPEG (else ire_init fails, "invalid ... IRE_FLAG_RESULT_JPEG").
 * Every JPEG result carries the image's own, optimised Huffman tables (ire_encode_jpeg_optimized_base64_fit_device below) in place
 * of the Annex K ones: a smaller text that decodes to the same pixels.  Such a result is fetched with ire_poll_text into a buffer of
 * ire_jpeg_optimized_base64_bound(h, w, quality, sampling) bytes, which is larger than ire_jpeg_base64_bound_ex's.  (Bit values 2,
 * 16 and 64 stay unknown.) */
#define IRE_FLAG_JPEG_OPTIMIZE 128u
/* Not a result format: valid only together with IRE_FLAG_RESULT_JPEG (else ire_init fails, "invalid ... IRE_FLAG_RESULT_JPEG").
 * Every JPEG result is a PROGRESSIVE file (ire_encode_jpeg_progressive_base64_fit_device below): the same quantised coefficients as
 * libjpeg's ten jpeg_simple_progression scans, each under its own optimal Huffman table -- a text some 4 - 8 % shorter than the
 * optimised baseline one, decoding to the same pixels.  Such a result is fetched with ire_poll_text into a buffer of
 * ire_jpeg_progressive_base64_bound(h, w, quality, sampling) bytes.  IRE_FLAG_JPEG_OPTIMIZE beside it is allowed and changes nothing
 * (a progressive file's tables are always its own).  (Bit values 2, 16, 64 and 512 stay unknown.) */
#define IRE_FLAG_JPEG_PROGRESSIVE 2048u
/* Not a result format, and free to combine with every other flag: UPLOAD jobs (ire_submit_upload) convert the pixels of a file that
 * carries an ICC profile (Display P3, Adobe RGB, ...) to sRGB on the device, between the decode and the preprocess step -- the third
 * operation of the reference's preprocess, .withMetadata({ icc: 'sRGB' }) (imagePreprocess.js:57-66).  See ire_icc_plan_file below for
 * what is converted and what is refused.  Without the flag every upload is treated as sRGB, tagged or not, as before.  File jobs
 * (ire_submit_jpeg) and every other entry are not changed by it. */
#define IRE_FLAG_UPLOAD_ICC 256u
/* Not a result format, and free to combine with every other flag: the engine decodes PNG uploads on the device -- ire_decode_png,
 * ire_decode_png_device, and ire_submit_jpeg / ire_submit_file / ire_submit_upload take a PNG file (they sniff the eight signature
 * bytes) beside a JPEG one.  See ire_decode_png_plan below for what is decoded and what is refused.  Without the flag every entry
 * refuses a PNG with the reason it gave before the flag existed, and nothing else changes.  (Bit value 512 stays unknown, as 2, 16 and
 * 64 do: tests/test_icc_plan.py holds it to that.) */
#define IRE_FLAG_DECODE_PNG 1024u
/* Valid only together with IRE_FLAG_DECODE_PNG (else ire_init fails, "invalid ... IRE_FLAG_DECODE_PNG"): the same entries also take the
 * PNG forms ire_decode_png_plan_ex accepts with IRE_DECODE_ACCEPT_PNG_ALL -- 1, 2 and 4 bits per sample (grey and palette), 16 bits per
 * sample (RGB, grey + alpha, RGB + alpha) and Adam7 interlacing.  16-bit GREY stays with the host codec: Pillow clips it, sharp takes
 * its high byte, so the two hosts disagree.  A batch may mix old and new forms of one size.  Without this bit every entry gives the
 * status, the reason and the bytes it gave before the bit existed.  (Bit values 2, 16, 64, 512 and 4096 stay unknown.) */
#define IRE_FLAG_DECODE_PNG_ALL 8192u



typedef struct ire_timings { /* GPU time measured with HIP events on the engine's stream; mirrors
                                timings.classify_ms / restore_ms of restorator.js:48-98         */
    double classify_ms;
    double restore_ms;
    double total_ms;
} ire_timings;

/* ---- lifecycle ------------------------------------------------------------------------ */
int ire_abi_version(void);
int ire_init(const ire_config* cfg, ire_engine** out);
void ire_shutdown(ire_engine* e);
/* Thread-local message of the last failing call on this thread ("" if none). */
const char* ire_last_error(void);
/* Load RestoreNet-v0 weights from memory (same bytes as the weight file). */
int ire_load_weights(ire_engine* e, const void* blob, size_t bytes);
/* Images of this shape one restore call can take right now: min(max_batch, what the free HBM (hipMemGetInfo) holds
 * at the engine's real per-image footprint: activation workspace + staging); 0 if the shape is unsupported (ire_restore's
 * rules, 8192 x 8192 included) or not
 * even one image fits (a restore call would then fail with IRE_ERR_UNAVAILABLE "out of device memory"). */
int ire_max_batch_for(ire_engine* e, int h, int w);

/* ---- host-buffer entry points (synchronous; copy in, run, copy out) -------------------- */
/* analyze(): n images of h x w, rows row_stride bytes apart (>= 3*w), images n apart by
 * h*row_stride.  is_jpeg[i] != 0 <=> metadata.format === 'jpeg' (classifier.js:180).
 * scores_out: n*7 doubles; label_out: n int32 = first-max argmax in key order (may be NULL). */
int ire_classify(ire_engine* e, const uint8_t* rgb, int n, int h, int w, int row_stride,
                 const uint8_t* is_jpeg, double* scores_out, int32_t* label_out);
/* restoreImage() with one image per job: out_rgb is n*h*w*3 (tightly packed).  scores==NULL
 * => classify inside (is_jpeg then required); else n*7 doubles used as conditioning.
 * h and w must be multiples of 8 (three stride-2 levels), >= 16, at most 8192, and h * w * 64 < 2^32: the network's widest tensor of
 * one image (32 channels of bf16 per pixel) is addressed with 32-bit byte offsets.  Of the sizes up to 8192 a side that excludes
 * 8192 x 8192 alone (IRE_ERR_INVALID_INPUT; ire_max_batch_for answers 0); ire_restore_tiled_device restores it in 2..64 row strips.
 * The batch size is no part of the rule: images lie a 64-bit stride apart. */
int ire_restore(ire_engine* e, const uint8_t* rgb, int n, int h, int w, const double* scores,
                const uint8_t* is_jpeg, uint8_t* out_rgb, ire_timings* t);
/* restoreImage() with k = 2..3 views of one scene: align to view 0 and blend.  out: h*w*3.
 * noise_score: the classifier's noise score of view 0 (sets the blend sigma); <0 => classify inside. */
int ire_fuse(ire_engine* e, const uint8_t* rgb_views, int k, int h, int w, double noise_score,
             uint8_t* out_rgb, int32_t* shifts_out /* k*2 (dy,dx), may be NULL */, ire_timings* t);

/* ---- device-buffer entry points (asynchronous on `stream`, a hipStream_t or NULL) ------ */
/* Same semantics; every pointer is device memory of e's GPU, tightly packed. The FastAPI /
 * PyTorch-ROCm host and bench.py use these with tensor.data_ptr() and the torch stream. */
int ire_classify_device(ire_engine* e, const uint8_t* d_rgb, int n, int h, int w,
                        const uint8_t* d_is_jpeg, double* d_scores, int32_t* d_label, void* stream);
int ire_restore_device(ire_engine* e, const uint8_t* d_rgb, int n, int h, int w,
                       const double* d_scores /* NULL => classify inside */, const uint8_t* d_is_jpeg,
                       uint8_t* d_out_rgb, void* stream);
int ire_fuse_device(ire_engine* e, const uint8_t* d_rgb_views, int k, int h, int w, double noise_score,
                    uint8_t* d_out_rgb, int32_t* d_shifts, void* stream);
/* Several restoreImage() calls with 2..3 images each (geminiClient.js:32,49), coalesced like the batcher coalesces single-image
 * jobs: nsets (1..16) independent view sets of one shape in one call -- d_rgb_views [nsets][k][h][w][3], d_out_rgb
 * [nsets][h][w][3], d_shifts [nsets][k][2] (may be NULL), noise_scores [nsets] doubles in HOST memory (each < 0 => classify
 * view 0 of that set inside).  Results are those of nsets ire_fuse_device calls; the kernel chain runs once. */
int ire_fuse_batch_device(ire_engine* e, const uint8_t* d_rgb_views, int nsets, int k, int h, int w,
                          const double* noise_scores, uint8_t* d_out_rgb, int32_t* d_shifts, void* stream);

/* ---- preprocess step in front of the path (server-node/src/middleware/imagePreprocess.js:24-91) ---- */
/* Pixel part of preprocessImage(): EXIF auto-orient (:43) and fit-inside-max_dim Lanczos-3 resize (:46-55); the JPEG
 * q85 4:4:4 encode (:57-64) stays with the host codec.  width/height are the STORED dimensions (what sharp's
 * metadata() reports, :40,:46), orientation the EXIF tag 1..8, max_dim 2048 in the reference (:4).
 * ire_preprocess_plan is pure host arithmetic (no GPU): it returns the upright, fitted size. */
int ire_preprocess_plan(int width, int height, int orientation, int max_dim, int* out_w, int* out_h, int* resized);
/* rgb: h*w*3 stored pixels; out: out_h*out_w*3 as planned.  Integer two-pass resampler, bit-exact with oracle/preprocess.py. */
int ire_preprocess(ire_engine* e, const uint8_t* rgb, int h, int w, int orientation, int max_dim,
                   uint8_t* out_rgb, int out_h, int out_w);
int ire_preprocess_device(ire_engine* e, const uint8_t* d_rgb, int h, int w, int orientation, int max_dim,
                          uint8_t* d_out_rgb, int out_h, int out_w, void* stream);
/* The batched, asynchronous form: n <= max_batch images of ONE stored size (h x w) and one orientation, image i at d_rgb + i *
 * image_pitch_bytes (>= h*w*3, rows tightly packed), -> n upright fitted images at d_out_rgb + i * out_image_pitch_bytes (>=
 * out_h*out_w*3, rows tightly packed); out_h, out_w as ire_preprocess_plan gives them.  Image i is byte for byte what
 * ire_preprocess_device gives for it alone; nothing between the output images is written.  Two stream operations per call whatever n
 * (one when nothing is resized).  The tap tables of an (input size, output size) pair are built on the host in double precision and
 * kept on the device (the 16 pairs used last): the first call with a new pair uploads them and waits for that upload on `stream`;
 * every later call returns without waiting for the device.  Stored pixels are read along stored rows for every orientation (5..8
 * through a transposing tile in LDS); a resize by more than about 17 (the tile no longer fits in 64 KB of LDS) reads them tap by tap,
 * as ire_preprocess_device does. */
int ire_preprocess_batch_device(ire_engine* e, const uint8_t* d_rgb, int n, int h, int w, size_t image_pitch_bytes,
                                int orientation, int max_dim, uint8_t* d_out_rgb, int out_h, int out_w,
                                size_t out_image_pitch_bytes, void* stream);

/* ---- result side of the seam: restored pixels -> base64 text of a PNG file, on the device (restorator.js:108: `restoredImage` is
 * a base64 string of an ENCODED image; geminiClient.js:75-88) ----
 * The file: signature, IHDR (8-bit RGB), ONE IDAT chunk = a zlib stream of STORED deflate blocks (scanline filter 0) with its
 * Adler-32, its CRC-32, IEND -- every PNG decoder reads it; 0.2 % larger than the pixels.  The text: RFC 4648 base64, '=' padded,
 * no terminator.  Bit-exact against zlib / base64 / a PNG decoder (oracle/encode.py).  w a multiple of 8; n <= max_batch.
 * ire_png_base64_bytes: characters per image (0: unsupported size).  Images / texts are h*w*3 / stride_bytes apart. */
size_t ire_png_base64_bytes(int h, int w);
int ire_encode_png_base64_device(ire_engine* e, const uint8_t* d_rgb, int n, int h, int w, uint8_t* d_chars, size_t stride_bytes,
                                 void* stream);
int ire_encode_png_base64(ire_engine* e, const uint8_t* rgb, int n, int h, int w, uint8_t* chars, size_t stride_bytes);

/* ---- any-size jobs (imagePreprocess.js:46-55 fits an upload inside 2048 px keeping its aspect ratio: a 3000x2000 photograph
 * arrives as 2048x1365, never a multiple of 8) ----
 * h, w in 1..8192.  The engine edge-replicates the image to H = max(16, ceil8(h)), W = max(16, ceil8(w)) on the device
 * (pixel (y, x) = source (min(y, h-1), min(x, w-1))), restores that and returns the top-left h x w window:
 * result == crop(ire_restore(edge_pad(x), scores), h, w).  scores == NULL => the classifier runs on the ORIGINAL h x w pixels
 * (never the padded copy) inside the same call.  A shape ire_restore takes is not padded and gives ire_restore's bytes.
 * ire_restore's size rule holds for the padded image: H * W * 64 < 2^32, i.e. not both h and w above 8184.
 * Device staging: the first batch of a ragged shape allocates the padded staging (and, for text results, the encoder's scratch)
 * for max_batch images of it, so later batches never allocate -- as long as that is <= 256 MB (max_batch * H * W * 3; at
 * max_batch 8 up to about 3300 x 3300).  Above it the staging is sized for the batch at hand, and a later LARGER batch of the
 * same shape grows it: one device synchronisation and reallocation inside that call. */
int ire_restore_fit(ire_engine* e, const uint8_t* rgb, int n, int h, int w, const double* scores,
                    const uint8_t* is_jpeg, uint8_t* out_rgb /* n*h*w*3 */, ire_timings* t);
int ire_restore_fit_device(ire_engine* e, const uint8_t* d_rgb, int n, int h, int w, const double* d_scores,
                           const uint8_t* d_is_jpeg, uint8_t* d_out_rgb, void* stream);
/* The PNG + base64 encoder for any width.  ire_png_base64_bytes_fit: characters per image, pure host arithmetic (0 outside
 * 1..8192); equal to ire_png_base64_bytes wherever that is not 0.  The device entry reads the top-left h x w window of n images
 * whose rows lie row_pitch_bytes (>= 3*w) and whose first pixels lie image_pitch_bytes apart: a window of a larger tensor is
 * encoded where it lies.  The number of stream operations per call does not depend on n. */
size_t ire_png_base64_bytes_fit(int h, int w);
int ire_encode_png_base64_fit_device(ire_engine* e, const uint8_t* d_rgb, int n, int h, int w, size_t row_pitch_bytes,
                                     size_t image_pitch_bytes, uint8_t* d_chars, size_t stride_bytes, void* stream);
int ire_encode_png_base64_fit(ire_engine* e, const uint8_t* rgb, int n, int h, int w, uint8_t* chars, size_t stride_bytes);

/* ---- the same result as a COMPRESSED PNG, on the device ----
 * The file: signature, IHDR, ONE IDAT, IEND.  The IDAT is a zlib stream of the Paeth-filtered scanlines (filter type 4 on every
 * row): one dynamic-Huffman deflate block per 32 768 filtered bytes, literals only, canonical codes of at most 15 bits built on the
 * device from the block's own histogram; every block but the last ends with an empty stored block (00 00 FF FF).  No LZ77 matching.
 * Lossless; every PNG decoder reads it.  The text's length depends on the pixels:
 * ire_png_deflate_base64_bound: the most characters any h x w image can give -- pure host arithmetic, 0 outside 1..8192; per block
 * a 1887-bit header, 9 bits per symbol, the marker; sizes every buffer (stride_bytes >= it; nothing is written beyond it).
 * The encoders read the window as ire_encode_png_base64_fit_device does and write, per image, the text at d_chars + i *
 * stride_bytes and its character count to lens[i] (uint64).  The bytes are a pure function of the pixels: equal for any batch
 * size, position, pitch and stream.  The number of stream operations per call does not depend on n; no host round trip. */
size_t ire_png_deflate_base64_bound(int h, int w);
int ire_encode_png_deflate_base64_fit_device(ire_engine* e, const uint8_t* d_rgb, int n, int h, int w, size_t row_pitch_bytes,
                                             size_t image_pitch_bytes, uint8_t* d_chars, size_t stride_bytes,
                                             uint64_t* d_lens /* n x uint64, device */, void* stream);
int ire_encode_png_deflate_base64_fit(ire_engine* e, const uint8_t* rgb, int n, int h, int w, uint8_t* chars, size_t stride_bytes,
                                      uint64_t* lens /* n x uint64, host */);

/* ---- the same result as a baseline JPEG (quality 85, 4:4:4), on the device ----
 * The file, in the order libjpeg writes it: SOI, JFIF APP0 (1.01, density 1:1), two DQT (the standard's Annex K tables at IJG quality
 * 85), SOF0 (8 bit, Y Cb Cr, each sampled 1 x 1, the real h and w), four DHT (the Annex K tables, fixed), DRI, SOS (one interleaved
 * scan), the entropy-coded data with a restart interval of 16 MCUs, EOI.  Every step is libjpeg's published integer algorithm (16-bit
 * fixed-point colour transform, the "islow" DCT, round-half-up quantiser): the bytes equal libjpeg-turbo's for the same settings.
 * Partial MCUs are completed by edge replication.  Every JPEG decoder reads it.  Lossy, unlike the two PNG forms.
 * ire_jpeg_base64_bound: the most characters any h x w image can give -- pure host arithmetic, 0 outside 1..8192; per MCU 2343 bits
 * (the exact maximum of the fixed Huffman tables over the amplitudes the quantiser can produce), doubled for byte stuffing, 2 bytes of
 * marker per interval; sizes every buffer (stride_bytes >= it; nothing is written beyond it).  A real text is several times shorter.
 * Arguments and guarantees as for ire_encode_png_deflate_base64_fit_device: the window, lens[i] (uint64) characters at d_chars + i *
 * stride_bytes, bytes that are a pure function of the pixels, a number of stream operations independent of n, no host round trip. */
size_t ire_jpeg_base64_bound(int h, int w);
int ire_encode_jpeg_base64_fit_device(ire_engine* e, const uint8_t* d_rgb, int n, int h, int w, size_t row_pitch_bytes,
                                      size_t image_pitch_bytes, uint8_t* d_chars, size_t stride_bytes,
                                      uint64_t* d_lens /* n x uint64, device */, void* stream);
int ire_encode_jpeg_base64_fit(ire_engine* e, const uint8_t* rgb, int n, int h, int w, uint8_t* chars, size_t stride_bytes,
                               uint64_t* lens /* n x uint64, host */);
/* The same with the two settings of the file; the three calls above are their (85, 0) case, byte for byte.
 * quality: 1..100, the IJG scaling of the Annex K tables with the baseline clamp 1..255 (Pillow's quality=); 0: 85.
 * sampling: 0 = 4:4:4 as above; 2 = 4:2:0: Y sampled 2 x 2 (SOF0 0x22), an MCU is 16 x 16 pixels in the order Y00 Y01 Y10 Y11 Cb Cr, a
 * restart interval is 8 MCUs, chroma is libjpeg's h2v2 downsample ((a + b + c + d + bias) >> 2, bias 1 | 2 by output column), and
 * the Y blocks of a partial MCU that lie outside the image are libjpeg's dummy blocks.  The bytes equal libjpeg-turbo's for
 * quality=, subsampling=, optimize=False, restart_marker_blocks = 16 | 8 (tests/test_jpeg_opt_model.py).  4:2:2 and grey are refused
 * ("invalid: ..."), as is a quality outside 0..100; the bound is then 0.  The bound grows with the quality: per MCU 1067 bits at
 * quality 1, 4474 at 100 (4:4:4); 2006 and 9448 at 4:2:0, whose MCU covers four times the pixels. */
size_t ire_jpeg_base64_bound_ex(int h, int w, int quality, int sampling);
int ire_encode_jpeg_base64_fit_device_ex(ire_engine* e, const uint8_t* d_rgb, int n, int h, int w, size_t row_pitch_bytes,
                                         size_t image_pitch_bytes, uint8_t* d_chars, size_t stride_bytes,
                                         uint64_t* d_lens /* n x uint64, device */, int quality, int sampling, void* stream);
int ire_encode_jpeg_base64_fit_ex(ire_engine* e, const uint8_t* rgb, int n, int h, int w, uint8_t* chars, size_t stride_bytes,
                                  uint64_t* lens /* n x uint64, host */, int quality, int sampling);
/* The same three with OPTIMISED Huffman tables, libjpeg's optimize_coding: a first pass over the image counts its symbols (four
 * histograms: DC and AC, for Y and for Cb and Cr together; the DC predictors restart at every restart interval in that pass too), a
 * table per histogram is built as libjpeg's jpeg_gen_optimal_table builds it (code lengths limited to 16), and a second pass codes the
 * image with them.  All on the device, two launches and one small memset more than the fixed-table call, none depending on n, no host
 * round trip.  The file is the one above except that its four DHT segments (0x00, 0x10, 0x01, 0x11) carry the image's own tables, so
 * the head's length varies (at most the fixed head's 629 bytes).  The bytes equal libjpeg-turbo's for quality=, subsampling=,
 * optimize=True, restart_marker_blocks = 16 | 8 (tests/test_jpeg_huffopt_model.py), and decode to the pixels the fixed-table file
 * decodes to.  Arguments, refusals and the asynchronous, windowed device form are those of the _ex entries.  The bound is larger than
 * ire_jpeg_base64_bound_ex's: under an arbitrary table every code can be 16 bits, so a block is priced at 16 bits per position plus its
 * largest categories -- 1665 bits per block at quality 100. */
size_t ire_jpeg_optimized_base64_bound(int h, int w, int quality, int sampling);
int ire_encode_jpeg_optimized_base64_fit_device(ire_engine* e, const uint8_t* d_rgb, int n, int h, int w, size_t row_pitch_bytes,
                                                size_t image_pitch_bytes, uint8_t* d_chars, size_t stride_bytes,
                                                uint64_t* d_lens /* n x uint64, device */, int quality, int sampling, void* stream);
int ire_encode_jpeg_optimized_base64_fit(ire_engine* e, const uint8_t* rgb, int n, int h, int w, uint8_t* chars, size_t stride_bytes,
                                         uint64_t* lens /* n x uint64, host */, int quality, int sampling);
/* The same three as a PROGRESSIVE file (SOF2): the image's quantised coefficients -- those of the entries above, from the same front
 * end, computed once and kept in device scratch (128 bytes per 8 x 8 block) -- sent as the ten scans of libjpeg's
 * jpeg_simple_progression for Y Cb Cr: DC of all three components interleaved at Al = 1; Y 1-5 at Al = 2; Cr 1-63 and Cb 1-63 at
 * Al = 1; Y 6-63 at Al = 2; Y 1-63 refined to Al = 1; the DC refinement to Al = 0; Cr, Cb and Y 1-63 refined to Al = 0.  Every scan
 * that uses Huffman codes is preceded by a DHT with its own optimal table (ten tables per image, built on the device as the optimised
 * entries build theirs), and the restart interval is one MCU row of the scan (a DRI wherever it changes), which is the unit the device
 * codes in parallel: end-of-band runs and buffered correction bits cross blocks but never a restart.  The bytes equal libjpeg-turbo's
 * for Pillow's save(quality=, subsampling=, progressive=True, restart_marker_rows=1) (tests/test_jpeg_progenc_model.py) and decode to
 * the pixels the baseline file decodes to; the engine's own decoder reads them back under IRE_FLAG_DECODE_PROGRESSIVE.  Integer
 * work and fixed-order sums throughout: the text is a pure function of the pixels and the two settings.  Arguments, refusals and the
 * asynchronous, windowed device form are those of the _optimized_ entries.  The bound prices, per scan and block, every code at 16
 * bits, the largest category the quantiser can yield after the scan's shift, one EOBn symbol with 14 extra bits and one correction
 * bit per refined coefficient, doubles that for byte stuffing and adds 2 marker bytes per interval and the largest head per scan
 * (csrc/jpeg_tables.hpp: jpeg_prog_file_bound); nothing is ever written beyond it. */
size_t ire_jpeg_progressive_base64_bound(int h, int w, int quality, int sampling);
int ire_encode_jpeg_progressive_base64_fit_device(ire_engine* e, const uint8_t* d_rgb, int n, int h, int w, size_t row_pitch_bytes,
                                                  size_t image_pitch_bytes, uint8_t* d_chars, size_t stride_bytes,
                                                  uint64_t* d_lens /* n x uint64, device */, int quality, int sampling, void* stream);
int ire_encode_jpeg_progressive_base64_fit(ire_engine* e, const uint8_t* rgb, int n, int h, int w, uint8_t* chars, size_t stride_bytes,
                                           uint64_t* lens /* n x uint64, host */, int quality, int sampling);

/* ---- baseline JPEG uploads decoded on the device ----
 * The RGB bytes equal libjpeg-turbo's (PIL.Image.open(f).convert("RGB")): the file's own Huffman tables, libjpeg's "islow" inverse
 * DCT, its "fancy" chroma upsampling and its 16-bit fixed-point colour transform.
 * ire_decode_jpeg_plan: pure host, no engine.  IRE_OK and the size (sampling: 0 = 4:4:4, 1 = 4:2:2, 2 = 4:2:0, 3 = grey; any
 * output pointer may be NULL) if the device decodes this file: SOF0 / SOF1 with Huffman coding, 8-bit samples, one interleaved
 * scan, 8-bit quantiser tables, up to 4 + 4 Huffman tables of any content, with or without restart markers, 1..8192 per side; Y Cb
 * Cr with luma 1x1 / 2x1 / 2x2 over chroma 1x1 (width >= 5 when subsampled), or one grey component.  Everything else --
 * progressive, arithmetic coding, 12 bit, CMYK, Adobe / RGB colour, several scans, other sampling factors, DNL, a truncated
 * file -- is IRE_ERR_INVALID_INPUT with the reason in ire_last_error ("invalid: ..."): such a file stays with the host codec.
 * ire_decode_jpeg: synchronous; out_rgb receives h*w*3 bytes (h, w as planned).  A stream whose entropy-coded data is corrupt
 * (found on the device) is IRE_ERR_INVALID_INPUT "invalid: corrupt JPEG data"; the engine stays usable.  So is a well-formed stream
 * whose values no picture gives (a dequantised coefficient outside int16, a sample outside -512..511 before the range limit): there
 * libjpeg-turbo's own C and SIMD code give different bytes, and equality with it is promised for every image that is NOT flagged.
 * ire_decode_jpeg_device: n <= max_batch files (host memory) of ONE planned size -> n images on the device, tightly packed rows,
 * image i at d_rgb + i * image_pitch_bytes (>= h*w*3), ready for ire_classify_device / ire_preprocess_device /
 * ire_restore_fit_device on the same stream; d_status: one int32 per image, 0 = ok (the pixels of a flagged image are
 * unspecified, nothing outside them is written).  The host parse runs inside the call; the number of stream operations does not
 * depend on n.  The host waits for one thing only: the upload of the call before last, whose pinned staging (one of two) this call
 * reuses; uploads are ordered behind the kernels of the call before them, so a caller that runs three calls ahead of the device waits
 * for those kernels -- never for the kernels of the call directly before it, nor for its own. */
int ire_decode_jpeg_plan(const uint8_t* file, size_t bytes, int* out_h, int* out_w, int* out_sampling);
/* ire_decode_jpeg_plan with a choice of what is accepted (pure host, no engine).  accept == 0: ire_decode_jpeg_plan itself, status
 * and reason.  IRE_DECODE_ACCEPT_PROGRESSIVE: beside those files a progressive one (SOF2, Huffman-coded, 8-bit; the colour, sampling
 * and size rules above unchanged) with any scan script that T.81 Annex G allows -- DC scans with Ss = Se = 0, interleaved or not; AC
 * scans of one component with 1 <= Ss <= Se <= 63; Ah = 0 in a coefficient's first scan, else Ah = the Al its last scan left and
 * Al = Ah - 1; no AC scan of a component before its first DC scan -- and that is COMPLETE: every coefficient of every component ends
 * at Al = 0 (libjpeg smooths the blocks of an incomplete file; the device does not, so such a file stays with the host codec).
 * Huffman tables and restart intervals may change between scans; a DQT behind the first scan, more than IRE_DECODE_MAX_SCANS scans and
 * everything ire_decode_jpeg_plan refuses are refused ("invalid: progressive JPEG ...").  *out_nscans: the file's scans, 1 for a
 * baseline file.  An engine created with IRE_FLAG_DECODE_PROGRESSIVE decodes what this accepts; in corrupt entropy-coded data it may
 * flag what libjpeg only warns about (a refinement symbol of size > 1, a run that leaves its band, an end-of-band run longer than
 * its stream). */
#define IRE_DECODE_ACCEPT_PROGRESSIVE 1u
#define IRE_DECODE_MAX_SCANS 64
#define IRE_DECODE_ACCEPT_ICC 4u          /* ire_upload_plan only: see there.  (Bit value 2 stays unknown.) */
#define IRE_DECODE_ACCEPT_PNG 16u         /* ire_upload_plan only: the plan of an engine with IRE_FLAG_DECODE_PNG.  (Bit value 8 stays unknown beside 2:
                                             tests/test_icc_plan.py holds both to that.) */
#define IRE_DECODE_ACCEPT_PNG_ALL 32u     /* ire_decode_png_plan_ex, and ire_upload_plan beside IRE_DECODE_ACCEPT_PNG: the plan of an engine with
                                             IRE_FLAG_DECODE_PNG_ALL.  (Bit values 2 and 8 stay unknown.) */
int ire_decode_jpeg_plan_ex(const uint8_t* file, size_t bytes, uint32_t accept, int* out_h, int* out_w, int* out_sampling, int* out_nscans);
int ire_decode_jpeg(ire_engine* e, const uint8_t* file, size_t bytes, uint8_t* out_rgb /* h*w*3 */, int h, int w);
int ire_decode_jpeg_device(ire_engine* e, const uint8_t* const* files, const size_t* bytes, int n, int h, int w, uint8_t* d_rgb,
                           size_t image_pitch_bytes, int32_t* d_status /* n x int32, device */, void* stream);

/* ---- PNG uploads decoded on the device (png_parse.hpp, png_inflate_core.hpp, png_dec.hip) ----
 * The RGB bytes equal PIL.Image.open(f).convert("RGB"): the stream inflated, the scanlines unfiltered, grey replicated, the palette
 * looked up, alpha of any kind dropped.
 * ire_decode_png_plan: pure host, no engine.  IRE_OK and the size and colour type (any output pointer may be NULL) if the device decodes
 * this file: the signature, IHDR first; bit depth 8; colour type 0, 2, 3, 4 or 6; compression 0, filter method 0, no interlace; 1..8192
 * per side; PLTE of 1..256 entries (required for type 3); one or more CONSECUTIVE IDAT chunks, empty ones among them; IEND, or the end
 * of the file, behind the last IDAT; tRNS is read past; gAMA, cHRM, sRGB, pHYs, iCCP, text and every other ancillary chunk are skipped.
 * Everything else -- 16-bit and sub-8-bit depths and Adam7 (but see ire_decode_png_plan_ex and IRE_FLAG_DECODE_PNG_ALL), APNG (acTL in front of IDAT), type 3 without PLTE, an IHDR or PLTE chunk whose
 * CRC-32 is wrong, any other chunk in front of IDAT whose CRC-32 is wrong, a chunk that overruns the file (behind the last IDAT only an
 * empty IEND may lack its CRC, and the file may end inside a chunk's eight header bytes: what Pillow still reads), IDAT chunks that are
 * not consecutive, no IDAT, a zlib header that is not deflate
 * with a window of at most 32 KiB and no preset dictionary -- is IRE_ERR_INVALID_INPUT with the reason in ire_last_error ("invalid: PNG
 * ..."): such a file stays with the host codec.  IDAT CRCs are NOT checked: Pillow does not check them either, and the stream's
 * Adler-32, which the device compares, covers the data.
 * ire_decode_png (engine with IRE_FLAG_DECODE_PNG; else IRE_ERR_INVALID_INPUT): synchronous; out_rgb receives h*w*3 bytes (h, w as
 * planned).  A file whose DATA is FLAGGED on the device is IRE_ERR_INVALID_INPUT "invalid: corrupt PNG data (decoder status N)"; the
 * engine stays usable.  Flagged is everything but this: zlib decompresses the stream without error, it yields exactly
 * h * (1 + w * bytes per pixel) bytes, and every scanline's filter byte is 0..4.  Pillow zero-fills a short stream and ignores a long
 * one; the device flags both, and the host codec then decides.  Equality with Pillow is promised for every image that is NOT flagged.
 * ire_decode_png_device: ire_decode_jpeg_device's contract -- n <= max_batch files (host memory) of ONE planned size, of any colour
 * types, -> n images on the device, image i at d_rgb + i * image_pitch_bytes (>= h*w*3), nothing between them written; d_status: one
 * int32 per image, 0 = ok (the pixels of a flagged image are unspecified); the host parse runs inside the call; two launches whatever
 * n; the host's one wait is for the upload of the call before last.
 * ire_decode_png_plan_ex: ire_decode_png_plan with a choice of what is accepted, and the file's bit depth and interlace method beside
 * its colour type.  accept == 0: ire_decode_png_plan itself, status and reason; any bit but IRE_DECODE_ACCEPT_PNG_ALL is
 * IRE_ERR_INVALID_INPUT "unknown accept bits".  IRE_DECODE_ACCEPT_PNG_ALL: beside those files, bit depth 1, 2 or 4 for colour types 0
 * and 3, bit depth 16 for colour types 2, 4 and 6, and interlace method 1 (Adam7) for every accepted (type, depth) pair; the other
 * rules above are unchanged.  The pixels are still PIL's convert("RGB"): a grey sample of 1, 2 or 4 bits times 255, 85 or 17; a palette
 * index looked up, black where it lies past the last PLTE entry (a PLTE longer than 2^depth entries is read as Pillow reads it);
 * of a 16-bit sample its HIGH byte (0x00ff -> 0, 0x80ff -> 128); tRNS read past, alpha dropped.  Still refused, each with its own
 * reason: the (type, depth) pairs the PNG specification forbids, and 16-bit GREY (colour type 0) -- Pillow opens it as I;16 and
 * convert("RGB") CLIPS (0x0100 -> 255) where sharp takes the high byte, so a device result could equal only one of the two host codecs:
 * "invalid: PNG 16-bit grey: the host codecs disagree on its conversion".  An engine with IRE_FLAG_DECODE_PNG_ALL decodes what this
 * accepts, in ire_decode_png, ire_decode_png_device (old and new forms may share a batch; still two launches) and the submit entries;
 * "flagged" then reads: the stream yields exactly the passes' scanlines -- per pass that has a pixel, rows * (1 + ceil(width * bits per
 * pixel / 8)) bytes -- and every filter byte is 0..4.  The device path is still slower than the host codec (profiles/png_depths.md). */
int ire_decode_png_plan_ex(const uint8_t* file, size_t bytes, uint32_t accept, int* out_h, int* out_w, int* out_colour_type, int* out_depth,
                           int* out_interlace);
int ire_decode_png_plan(const uint8_t* file, size_t bytes, int* out_h, int* out_w, int* out_colour_type);
int ire_decode_png(ire_engine* e, const uint8_t* file, size_t bytes, uint8_t* out_rgb /* h*w*3 */, int h, int w);
int ire_decode_png_device(ire_engine* e, const uint8_t* const* files, const size_t* bytes, int n, int h, int w, uint8_t* d_rgb,
                          size_t image_pitch_bytes, int32_t* d_status /* n x int32, device */, void* stream);

/* ---- async batcher (restoreBatch's in-flight promises) ---------------------------------- */
typedef struct ire_job ire_job;
/* Queue one h x w image for restoration; jobs of equal shape are coalesced into batches of up
 * to max_batch.  The input is copied before return.  scores: the 7 doubles a previous ire_classify
 * of this image returned (the job is then not classified again), or NULL => classify inside. */
int ire_submit(ire_engine* e, const uint8_t* rgb, int h, int w, int is_jpeg, const double* scores, ire_job** job_out);
/* ire_submit without the multiple-of-8 rule (h, w in 1..8192; the result is that of ire_restore_fit); jobs are coalesced by
 * their exact (h, w), polled with ire_poll and released with ire_job_release.  With IRE_FLAG_RESULT_PNG_BASE64 ire_poll
 * delivers ire_png_base64_bytes_fit(h, w) characters: the PNG of the h x w result. */
int ire_submit_fit(ire_engine* e, const uint8_t* rgb, int h, int w, int is_jpeg, const double* scores, ire_job** job_out);
/* ire_submit_fit for an ENCODED upload: `file` is a JPEG file that ire_decode_jpeg_plan accepts (on an engine with
 * IRE_FLAG_DECODE_PROGRESSIVE: that ire_decode_jpeg_plan_ex accepts with IRE_DECODE_ACCEPT_PROGRESSIVE; the room rule below then counts
 * the data of all its scans); the job's result is that
 * of ire_submit_fit(the file's decoded pixels, h, w, is_jpeg = 1, scores) with h, w as the plan reports them (the caller sizes its
 * ire_poll / ire_poll_text buffer from the plan).  The file's head is parsed and its scan is cut in the calling thread, before
 * return (the file may be freed then); the decode runs on the device with the job's batch.  File jobs are coalesced by their planned
 * (h, w), whatever their sampling, and never share a batch with pixel jobs.  A file the plan refuses, or whose entropy-coded data
 * may take more room than its h * w * 3 pixels, is IRE_ERR_INVALID_INPUT with the reason in ire_last_error ("invalid: ...") and
 * creates no job: such a file stays with the host codec.  A file whose DATA the device finds corrupt fails only its own job, at
 * its poll: IRE_ERR_INVALID_INPUT "invalid: corrupt JPEG data (decoder status N)"; the other jobs of its batch complete.  A file job
 * has no preprocess semantics: IRE_FLAG_UPLOAD_ICC does not change it, its pixels are taken as they are decoded. */
int ire_submit_jpeg(ire_engine* e, const uint8_t* file, size_t bytes, const double* scores, ire_job** job_out);
/* The same entry under its neutral name.  On an engine with IRE_FLAG_DECODE_PNG both take a PNG file that ire_decode_png_plan accepts
 * (they sniff the eight signature bytes): the job's result is that of ire_submit_fit(ire_decode_png(file), h, w, is_jpeg = 0, scores).
 * The room rule is the same: a file whose IDAT payload is larger than its h * w * 3 pixels is refused at submit (a noise image
 * compresses to slightly more than its pixels).  PNG and JPEG jobs of one size share a batch, decoded with one call per kind however they interleave.  Corrupt data fails its own job at its
 * poll, "invalid: corrupt PNG data (decoder status N)"; the rest of the batch completes.  ire_submit_upload likewise: its result is
 *   ire_submit_fit(ire_preprocess(ire_decode_png(file), its orientation, max_dim), is_jpeg = 0, scores)
 * with the orientation of an eXIf chunk in front of IDAT (the TIFF walk of a JPEG's Exif block; a broken chunk is orientation 1), and
 * ire_upload_plan says the same with IRE_DECODE_ACCEPT_PNG.  On an engine with IRE_FLAG_UPLOAD_ICC (the plan: IRE_DECODE_ACCEPT_ICC)
 * a PNG that carries iCCP is refused with a reason: reading the chunk is a later change; without that flag the profile is ignored, as
 * a JPEG's is.  Without IRE_FLAG_DECODE_PNG both entries refuse a PNG as they always did ("invalid: not a JPEG file (no SOI)"). */
int ire_submit_file(ire_engine* e, const uint8_t* file, size_t bytes, const double* scores, ire_job** job_out);
/* An UPLOAD job: ire_submit_jpeg with the preprocess step of imagePreprocess.js:40-55 between the decode and the network, all on the
 * device -- no pixel of the upload is ever on the host.  The file is one ire_submit_jpeg takes.  Its orientation is read from the
 * first APP1 segment that is an Exif block (IFD0 tag 0x0112, SHORT, count 1, value 1..8; anything else, a broken block included, is
 * orientation 1 and never a refusal).  The job's result is exactly that of
 *   ire_submit_fit(ire_preprocess(ire_decode_jpeg(file), that orientation, max_dim), is_jpeg = 1, scores)
 * (scores == NULL: the classifier runs on the preprocessed, unpadded pixels); its size is the fitted out_h x out_w.  On an engine created
 * with IRE_FLAG_UPLOAD_ICC the file's ICC profile is honoured, as sharp honours it before it resizes: the result is exactly that of
 *   ire_submit_fit(ire_preprocess(ire_icc_to_srgb(ire_decode_jpeg(file), ire_icc_plan_file(file)), that orientation, max_dim), is_jpeg = 1, scores)
 * and a file whose profile ire_icc_plan_file refuses is refused at submit with that reason and creates no job.  The profile is no part
 * of the batch key: uploads with different profiles, or none, share a batch.  Without the flag nothing changes, for tagged files too.  The reference's
 * q85 re-encode between preprocess and restore (imagePreprocess.js:57-64) is NOT reproduced: it exists to hand an external API a file.
 * ire_upload_plan: pure host, no engine -- what ire_submit_upload will do with this file on an engine whose decoder accepts
 * `accept` (0, or IRE_DECODE_ACCEPT_PROGRESSIVE, IRE_DECODE_ACCEPT_ICC for an engine with IRE_FLAG_UPLOAD_ICC -- the plan then also refuses
 * what ire_icc_plan_file refuses, with the same reason; without the bit the profile is not looked at): the stored size, the orientation, the fitted size (any output pointer may be NULL;
 * the caller sizes its poll buffer from out_h, out_w).  It refuses what ire_decode_jpeg_plan_ex refuses, with the same reason,
 * a max_dim below 1, and a file that breaks the room rule below.
 * Upload jobs are coalesced by (stored h, stored w, orientation, max_dim) and never share a batch with another kind of job.  Known
 * limit, the room rule: the job's cut scan is staged in its input place of out_h * out_w * 3 bytes, so a file whose entropy-coded
 * data may need more (a large file fitted into a small max_dim) is IRE_ERR_INVALID_INPUT ("invalid: ...") at submit and creates no
 * job; the plan refuses it with the same reason.  Corrupt data fails the job alone at its poll, as for ire_submit_jpeg.  The decoded stored
 * images of a batch lie in an engine scratch sized by the any-size staging rule above (max_batch images while that is <= 256 MB). */
int ire_upload_plan(const uint8_t* file, size_t bytes, uint32_t accept, int max_dim, int* stored_h, int* stored_w,
                    int* orientation, int* out_h, int* out_w);
int ire_submit_upload(ire_engine* e, const uint8_t* file, size_t bytes, int max_dim, const double* scores, ire_job** job_out);

/* ---- ICC profiles of uploads: convert to sRGB on the device (icc_parse.hpp, icc.hip) ------------------------------------------------
 * The transform is all-integer and is stated once.  Tables, built on the host in double precision:
 *   lin[c][v] = rint(65535 * TRC_c(v / 255))              u16, clamped (grey: row 0 only)
 *   m         = rint(16384 * inv(M_sRGB) * M_profile)     Q14; M_profile's columns are the profile's rXYZ gXYZ bXYZ, M_sRGB's the D50
 *               sRGB colorants (0.43607, 0.22249, 0.01392), (0.38515, 0.71687, 0.09708), (0.14307, 0.06061, 0.71410) as s15Fixed16
 * Per pixel:
 *   y_c   = clamp((sum_k m[3 c + k] * lin[k][v_k] + 8192) >> 14, 0, 65535)     (arithmetic shift, 64-bit sum)
 *   out_c = enc8(y_c),  enc8(x) = rint(255 * sRGB_OETF(x / 65535)), exact for all 65536 x
 *   IRE_ICC_GREY: out = enc8(lin[0][v]) on all three bytes (v: the pixel's first byte; a decoded grey file has three equal ones)
 * Within one level of littlecms (what sharp runs) on every sample: profiles/upload_icc.md.
 * kind: IRE_ICC_NONE -- nothing to apply: no profile, structurally broken bytes (a size field beyond the bytes, no 'acsp', a tag
 * outside the profile, a missing or truncated rXYZ gXYZ bXYZ rTRC gTRC bTRC / kTRC), or a profile whose colour space is not the
 * image's (RGB for 3 components, GRAY for 1); IRE_ICC_IDENTITY -- the transform above changes no byte (rounded matrix = 16384 I and
 * enc8(lin[c][v]) == v for all v: the common sRGB profiles); IRE_ICC_MATRIX / IRE_ICC_GREY -- a transform to apply.  Accepted: v2 and
 * v4 headers, data colour space RGB or GRAY, PCS XYZ, curves `curv` of count 0 (identity), 1 (a u8Fixed8 gamma), 2..4096 (a u16 table,
 * linearly interpolated) and `para` function types 0..4; `chad` is ignored (the colorants are D50 already).  REFUSED, as
 * IRE_ERR_INVALID_INPUT with the reason in ire_last_error ("invalid: ICC profile ..."): a well-formed profile with an A2B0 / A2B1 /
 * A2B2 tag (littlecms would use the lookup table, not the matrix), any other data colour space (CMYK ...), any other PCS (Lab), a
 * curve of another type or a longer table, a matrix coefficient outside (-4, 4).  Such an upload stays with the host codec.
 * Rendering intents and black-point compensation do not exist here: a matrix profile has one colorimetric transform. */
enum { IRE_ICC_NONE = 0, IRE_ICC_IDENTITY = 1, IRE_ICC_MATRIX = 2, IRE_ICC_GREY = 3 };
typedef struct ire_icc_transform {
    int32_t kind;             /* IRE_ICC_* */
    int32_t m[9];             /* row-major Q14; zeros unless IRE_ICC_MATRIX or an RGB profile's IRE_ICC_IDENTITY */
    uint16_t lin[3][256];
} ire_icc_transform;
/* Pure host, no engine.  ire_icc_plan_profile: the raw bytes of a profile (for callers who decode a PNG's iCCP on the host) that came
 * with an image of `components` (1 or 3) components.  ire_icc_plan_file: the profile of a JPEG file -- the APP2 segments in front of
 * its first scan whose payload starts "ICC_PROFILE\0", a 1-based sequence number and a count, in any order; every chunk must state the
 * same count, every number 1..count must occur exactly once and the assembled profile is at most 1 MiB, else the file has NO profile
 * (IRE_ICC_NONE; never a refusal, like a broken EXIF block) -- and the component count of its frame header. */
int ire_icc_plan_profile(const uint8_t* profile, size_t bytes, int components, ire_icc_transform* out);
int ire_icc_plan_file(const uint8_t* file, size_t bytes, ire_icc_transform* out);
/* The conversion by itself, for pixel callers (PNG / WebP uploads decoded on the host) and for the tests: n <= max_batch tightly
 * packed h x w RGB images (1..8192 per side), converted IN PLACE, image i by t[i] (NULL, IRE_ICC_NONE and IRE_ICC_IDENTITY: left as
 * it is).  One launch whatever n; none when no image needs a transform.  Only pixels are written: with image_pitch_bytes > h*w*3 the
 * bytes between images stay untouched.  ire_icc_to_srgb_device: asynchronous on `stream`, the tables are copied before return.
 * ire_icc_to_srgb: synchronous, host pointers, images h*w*3 apart. */
int ire_icc_to_srgb_device(ire_engine* e, uint8_t* d_rgb, int n, int h, int w, size_t image_pitch_bytes,
                           const ire_icc_transform* const* t /* n entries, NULL = leave */, void* stream);
int ire_icc_to_srgb(ire_engine* e, uint8_t* rgb, int n, int h, int w, const ire_icc_transform* const* t);
/* A FUSION job: k = 2 or 3 views of one scene, all h x w with h, w in 1..8192 (views[v]: h*w*3 bytes, copied before return),
 * submitted once, computed on the device with its batch, polled and released like every other job; its result is the fused h x w
 * image -- pixels, or on a text engine the engine's result text.  Every view is restored as ire_submit_fit restores it (scores of
 * the view's own pixels unless has_scores[v] says that scores + 7*v holds them; is_jpeg NULL: all 1); each restored window is
 * edge-replicated to HF x WF, HF = max(64, ceil8(h)) and WF likewise; the padded set is fused as ire_fuse fuses it with
 * noise_score < 0 (view 0 of the padded set classified, its noise score the blend table's); the fused image is cropped to h x w.
 * For h, w >= 64 on a pixel engine: the bytes of ire_submit_fit per view, edge pad, ire_fuse(noise_score = -1), crop.  scores_out
 * of the poll: view 0's.  Fusion jobs are coalesced by (h, w, k), min(max_batch / k, 16) jobs a batch, never with another kind of job.
 * k outside 2..3, a null view, a size outside 1..8192 or an engine with max_batch < k: IRE_ERR_INVALID_INPUT, no job. */
int ire_submit_fuse_fit(ire_engine* e, const uint8_t* const* views, int k, int h, int w,
                        const uint8_t* is_jpeg /* [k] or NULL */, const uint8_t* has_scores /* [k] or NULL */,
                        const double* scores /* [k][7] */, ire_job** job_out);
/* The same computation for a caller on the device, asynchronous on `stream`: d_views [nsets][k][h][w][3] -> d_out_rgb
 * [nsets][h][w][3]; d_scores [nsets*k][7] (device) for every view, or NULL: classified inside.  nsets <= 16, nsets*k <= max_batch.
 * No host round trip: the blend tables are built on the device. */
int ire_restore_fuse_fit_device(ire_engine* e, const uint8_t* d_views, int nsets, int k, int h, int w,
                                const double* d_scores /* [nsets*k][7] or NULL */, const uint8_t* d_is_jpeg,
                                uint8_t* d_out_rgb, void* stream);
/* Wait up to timeout_ms (<0: forever) for the job; on IRE_OK out_rgb (h*w*3 pixel bytes, or with IRE_FLAG_RESULT_PNG_BASE64
 * ire_png_base64_bytes_fit(h, w) characters -- for an ire_submit job the same number as ire_png_base64_bytes(h, w), which is 0
 * for the ragged widths ire_submit_fit takes: size the buffer with the _fit form), scores_out (7, may
 * be NULL) and t (may be NULL) are filled and the job is released; any other status but
 * IRE_ERR_TIMEOUT releases it too.  IRE_ERR_TIMEOUT leaves the job pending and the handle valid:
 * poll again, or give the job up with ire_job_release.  One thread at a time per handle. */
int ire_poll(ire_engine* e, ire_job* job, int timeout_ms, uint8_t* out_rgb, double* scores_out,
             ire_timings* t);
/* ire_poll with a result length: works on every engine.  On IRE_OK `out` holds *len_out bytes: h*w*3 pixel bytes, the
 * ire_png_base64_bytes_fit(h, w) characters of IRE_FLAG_RESULT_PNG_BASE64, or the real character count of
 * IRE_FLAG_RESULT_PNG_DEFLATE / IRE_FLAG_RESULT_JPEG (at most ire_png_deflate_base64_bound(h, w) / ire_jpeg_base64_bound(h, w)).
 * cap_bytes is the size of `out`: when the result is
 * longer the call returns IRE_ERR_INVALID_INPUT, sets *len_out to the size needed and leaves the job pending.  Otherwise as
 * ire_poll.  On an engine with IRE_FLAG_RESULT_PNG_DEFLATE or IRE_FLAG_RESULT_JPEG ire_poll itself has nowhere to report a length: it returns
 * IRE_ERR_INVALID_INPUT ("invalid: use ire_poll_text") and -- the one exception to its rule -- leaves the job pending. */
int ire_poll_text(ire_engine* e, ire_job* job, int timeout_ms, uint8_t* out, size_t cap_bytes, size_t* len_out,
                  double* scores_out, ire_timings* t);
/* Give up a job without fetching its result -- the caller's promise was rejected on a timeout and
 * the retry policy (server-node/src/utils/retry.js:12-47, 3 attempts) will submit the image anew:
 * frees the handle and whatever only it kept alive (its place among a finished batch's unread
 * results, so the staging slot can cycle; its queued pixels if it never reached a batch).  A job
 * already gathered into a batch is still computed with it.  e == NULL after ire_shutdown: frees
 * the handle only.  job == NULL: no-op. */
int ire_job_release(ire_engine* e, ire_job* job);

/* ---- cfg 4: one large image restored as row strips (imagePreprocess.js:4 caps uploads at 2048 px) ----
 * The image is cut into nstrips equal row strips; every layer runs strip by strip, the boundary rows of every tensor a 3x3
 * convolution reads are exchanged between neighbouring strips after the layer that produced it (per-level halo exchange),
 * and the GroupNorm partial statistics of all strips are combined before each GroupNorm.  The result is bit-identical to
 * ire_restore_device on the whole image.  H must be a multiple of nstrips, rows per strip a multiple of 128, W of 8, and a strip
 * with its two halo rows obeys ire_restore's size rule: (H / nstrips + 2) * W * 64 < 2^32 (8192 x 8192 needs two strips or more). */
/* All strips on this GPU ("virtual ranks": the exchange steps are in-device copies).  d_scores NULL => classify inside. */
int ire_restore_tiled_device(ire_engine* e, const uint8_t* d_rgb, int h, int w, int nstrips, const double* d_scores,
                             const uint8_t* d_is_jpeg, uint8_t* d_out_rgb, void* stream);
/* One rank of the multi-GPU layout: a session owns strips [first_strip, first_strip + nlocal) and runs the layer program one
 * op at a time; between ops the HOST moves halo rows and statistics between ranks (sharding.py: send/recv + all_gather over
 * RCCL).  d_stats_all: device buffer of ire_strips_stats_bytes(h, w) bytes owned by the caller (a torch tensor): the global
 * array of GroupNorm partials, of which this session fills its slice. */
typedef struct ire_strips ire_strips;
typedef struct ire_strip_xchg {   /* what op k left to exchange */
    int32_t halo_bytes;           /* bytes of one boundary row of the op's output (0: nothing to exchange) */
    int32_t has_up, has_down;     /* this session has a remote neighbour above / below */
    int64_t stats_offset_bytes;   /* slice of d_stats_all this session just wrote ... */
    int64_t stats_local_bytes;    /* ... its size (0: the op wrote no statistics) ... */
    int64_t stats_total_bytes;    /* ... and the size of the complete array for this op (equal slices per strip) */
} ire_strip_xchg;
size_t ire_strips_stats_bytes(int h, int w);
int ire_strips_open(ire_engine* e, int h, int w, int nstrips_total, int first_strip, int nlocal, void* d_stats_all, ire_strips** out);
void ire_strips_close(ire_strips* s);
int ire_strips_num_ops(ire_strips* s);
/* d_rows_with_halo: (nlocal*rows_per_strip + 2) x w x 3: the session's rows with one row above and below (rows outside the
 * image are never read); d_scores: the 7 classifier scores of the WHOLE image (the rank that took the job classified it). */
int ire_strips_set_input(ire_strips* s, const uint8_t* d_rows_with_halo, const double* d_scores, void* stream);
int ire_strips_run_op(ire_strips* s, int k, void* stream, ire_strip_xchg* info);
/* copy the first / last real row of op k's output into d_send_up / d_send_down (halo_bytes each; NULL or no neighbour: skipped) */
int ire_strips_pack_halo(ire_strips* s, int k, uint8_t* d_send_up, uint8_t* d_send_down, void* stream);
/* copy the neighbours' rows into the halo rows of op k's output */
int ire_strips_unpack_halo(ire_strips* s, int k, const uint8_t* d_recv_up, const uint8_t* d_recv_down, void* stream);
/* d_out_rows: nlocal*rows_per_strip x w x 3 */
int ire_strips_get_output(ire_strips* s, uint8_t* d_out_rows, void* stream);

/* ---- host feeding at 8 ranks per host (restorator.js:198-211: one independent job per image) ----
 * The engine's service threads (batch launcher, completer) run on the NUMA node of their GPU, on the share of that node's
 * CPUs that falls to this GPU among the node's GPUs (csrc/affinity.hpp); IRE_CPU_AFFINITY=off | <cpulist> overrides.
 * ire_affinity_plan is pure host arithmetic over sysfs (no GPU): sysfs_root NULL = "/sys"; pci_bdf as hipDeviceGetPCIBusId
 * prints it ("0000:c1:00.0"); cpulist_out "" when the node is unknown.  ire_engine_affinity: what engine e applied. */
int ire_affinity_plan(const char* sysfs_root, const char* pci_bdf, char* cpulist_out, size_t cap, int32_t* numa_node_out,
                      int32_t* slot_out, int32_t* nslots_out);
int ire_engine_affinity(ire_engine* e, char* cpulist_out, size_t cap, int32_t* numa_node_out);

/* ---- service gauges (getHealthStatus + /health/ready dependency entry: restorator.js:289-314, healthRouter.js:80-117) ---- */
typedef struct ire_engine_stats {
    uint32_t struct_size;   /* = sizeof(ire_engine_stats) */
    int32_t queue_depth;    /* jobs waiting in the batcher */
    int64_t batches;        /* engine batches (restore calls) since ire_init */
    int64_t images;         /* images restored since ire_init */
    int32_t last_batch;     /* images in the most recent batch: > 1 shows in-flight jobs being coalesced */
    int32_t max_batch;
    double images_per_sec;  /* gauge: images restored over the last 10 s window / its span (0 when idle) */
} ire_engine_stats;
int ire_get_stats(ire_engine* e, ire_engine_stats* out);

/* ---- measurement / diagnostics (used by bench.py and tests; not part of the job path) --- */
/* Raw integer accumulators of the classifier scan for n images (14 u64 each, order documented in
 * csrc/classifier_finalize.hpp) of the last classify / restore call, copied to host. */
int ire_debug_classifier_sums(ire_engine* e, int n, uint64_t* sums_out);
/* The blend tables of n noise scores (host), built on the device by the kernel the fusion jobs use, copied to out (tests only). */
int ire_debug_fusion_wlut(ire_engine* e, const double* noise, int n, uint32_t* out /* [n][256] */);
/* The Huffman tables of n x 4 histograms of 256 symbol counts (host; each count below 10^9, as libjpeg requires), built on the device
 * by the kernel the optimised JPEG results use: per histogram bits[16] then vals[256] (zero behind the nvals symbols that have a
 * code).  n in 1..4096 (tests only). */
int ire_debug_jpeg_huffman(ire_engine* e, const uint32_t* counts /* [n][4][256] */, int n, uint8_t* bits_vals_out /* [n][4][16 + 256] */,
                           int32_t* nvals_out /* [n][4] */);
/* The progressive JPEG path behind its coefficient pass (count pass, table kernel, emit pass, gather) on coefficients given: per
 * image [blocks][64] int16 in zig-zag order, component after component, a component's blocks in raster order -- at 4:4:4 ceil(h/8) x
 * ceil(w/8) blocks per component; at 4:2:0 Y on the MCU grid (2 ceil(h/16) x 2 ceil(w/16), dummy blocks included) and Cb, Cr
 * ceil(h/16) x ceil(w/16).  out_files receives n FILES (not base64) `stride` bytes apart, stride at least
 * ire_jpeg_progressive_base64_bound(h, w, quality, sampling) / 4 * 3, and lens their lengths.  n in 1..max_batch (tests only). */
int ire_debug_jpeg_progressive_from_coefs(ire_engine* e, const int16_t* coefs, int n, int h, int w, int quality, int sampling,
                                          uint8_t* out_files, size_t stride, uint64_t* lens /* n x uint64, host */);
/* Fill every scratch allocation of the process (device and pinned, over its whole capacity, whichever engine owns it) with `byte`, between
 * two waits for the device; *bytes_filled (may be null) = how many bytes that was.  Only in a process started with
 * IRE_DEBUG_POISON=<0..255> (every allocation is then filled with that byte at birth and entered in a registry): IRE_ERR_INVALID_INPUT
 * without it, and while this engine has a job queued, in flight or delivered but not yet polled.  Persistent allocations (weights,
 * tables, tickets that clean themselves: DESIGN.md "Buffer ownership") are left alone.  The caller submits no job while the call runs and keeps
 * every other engine of the process, and every strip session, idle meanwhile (tests only). */
int ire_debug_poison_scratch(ire_engine* e, int byte, uint64_t* bytes_filled);
/* The standalone GroupNorm finalize (csrc/gn.hip: one workgroup per image running csrc/gn_fold.hpp's gn_fold, the function every
 * activated convolution runs in its prologue) on partials given: stats [nimg][parts][8][2] (sum, sum of squares) per tile and group,
 * C in {32, 64, 128, 256} channels, hw pixels per image, gamma / beta [C]; film (may be null) [nimg][film_stride] with the scale at
 * film_off + c and the shift at film_off + C + c.  ab_out receives (A, B) of y = x A + B as [nimg][C][2].  nimg in 1..65535, parts in
 * 1..2^20.  All pointers are host memory; synchronous (tests only). */
int ire_debug_gn_finalize(ire_engine* e, const float* stats, int nimg, int parts, int C, int hw, const float* gamma, const float* beta,
                          const float* film, int film_stride, int film_off, float* ab_out);
/* Turn per-layer capture on/off (slow: synchronises after every layer; tests only). */
int ire_debug_capture(ire_engine* e, int on);
/* Copy one named intermediate activation of the last ire_restore* call to host as float32 NHWC.
 * Returns the element count through *count (call with out==NULL to query).
 * "<layer>.ab" ("head.ab" for the head) names the GroupNorm+FiLM coefficients (A, B) of y = x*A + B that the
 * layer's convolution applied to its input, as [N][C_in][2] float32. */
int ire_debug_activation(ire_engine* e, const char* name, float* out, size_t* count);
/* Accumulated HIP-event time (ms) and launch count per kernel family since the last reset:
 * family in {"classifier","conv3x3","conv1x1","stem","head","gn_finalize","fusion","all"}. */
int ire_profile_enable(ire_engine* e, int mode /* low byte: 0 off, 1 all families, 2 conv3x3 only (least overhead);
                                                   bits 8..: N > 1 = in mode 2 time only every N-th pass of the network */);
int ire_profile_query(ire_engine* e, const char* family, double* ms_out, int64_t* launches_out,
                      double* flops_out, double* bytes_out);
int ire_profile_reset(ire_engine* e);
/* Per-layer-group breakdown of the profiled convolution launches since the last reset, as a JSON array of
 * {"group" ("L0.rb1" .. "L3.rb2", "down0".., "up0".., "stem", "head"), "kernel", "level", "cin", "cout", "launches", "ms",
 *  "flops" (algorithmic), "flops_executed" (what the kernel issues: the sub-pixel `up` form runs 4 of 9 taps), "bytes"
 *  (algorithmic HBM bytes)} written to buf (cap bytes, NUL-terminated).  *needed_out = bytes required; call with
 * buf == NULL to size the buffer.  bench.py's roofline.per_level is computed from this. */
int ire_profile_report(ire_engine* e, char* buf, size_t cap, size_t* needed_out);

#ifdef __cplusplus
}
#endif
#endif /* IRE_H */
