// codec.cpp -- the text encoders' and the JPEG decoder's host side (codec.hpp): argument checks, buffers, uploads, downloads.
#include "codec.hpp"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "deflate.hpp"
#include "encode.hpp"
#include "jpeg.hpp"

namespace ire {

const TextFormat kStoredPng = {"PNG", [](int h, int w, TextSettings) { return png_base64_chars(h, w); }, "ire_png_base64_bytes",
                               [](int n, int h, int w, TextSettings) { return png_scratch_bytes(n, h, w); },
                               [](const uint8_t* d_rgb, int n, int h, int w, size_t row_pitch, size_t image_pitch, uint8_t* d_scratch, uint8_t* d_chars, size_t stride,
                                  uint8_t*, size_t, TextSettings, hipStream_t s) { encode_png_base64_launch(d_rgb, n, h, w, row_pitch, image_pitch, d_scratch, d_chars, stride, s); },
                               false, false, {0, 0, 0, 0}};
const TextFormat kDeflatePng = {"PNG", [](int h, int w, TextSettings) { return png_deflate_base64_bound(h, w); }, "ire_png_deflate_base64_bound",
                                [](int n, int h, int w, TextSettings) { return png_deflate_scratch_bytes(n, h, w); },
                                [](const uint8_t* d_rgb, int n, int h, int w, size_t row_pitch, size_t image_pitch, uint8_t* d_scratch, uint8_t* d_chars, size_t stride,
                                   uint8_t* d_lens, size_t lens_pitch, TextSettings, hipStream_t s) {
                                    encode_png_deflate_base64_launch(d_rgb, n, h, w, row_pitch, image_pitch, d_scratch, d_chars, stride, d_lens, lens_pitch, s);
                                },
                                true, false, {0, 0, 0, 0}};
const TextFormat kJpeg = {"JPEG",
                          [](int h, int w, TextSettings o) {
                              return o.progressive ? jpeg_progressive_base64_bound(h, w, o.quality, o.sampling) : jpeg_base64_bound(h, w, o.quality, o.sampling, o.optimize != 0);
                          },
                          "ire_jpeg_base64_bound",
                          [](int n, int h, int w, TextSettings o) {
                              return o.progressive ? jpeg_progressive_scratch_bytes(n, h, w, o.quality, o.sampling) : jpeg_scratch_bytes(n, h, w, o.quality, o.sampling, o.optimize != 0);
                          },
                          [](const uint8_t* d_rgb, int n, int h, int w, size_t row_pitch, size_t image_pitch, uint8_t* d_scratch, uint8_t* d_chars, size_t stride,
                             uint8_t* d_lens, size_t lens_pitch, TextSettings o, hipStream_t s) {
                              if (o.progressive) return encode_jpeg_progressive_base64_launch(d_rgb, n, h, w, row_pitch, image_pitch, d_scratch, d_chars, stride, d_lens, lens_pitch, o.quality, o.sampling, s);
                              encode_jpeg_base64_launch(d_rgb, n, h, w, row_pitch, image_pitch, d_scratch, d_chars, stride, d_lens, lens_pitch, o.quality, o.sampling, o.optimize != 0, s);
                          },
                          true, true, {kJpegDefaultQuality, kJpegDefaultSampling, 0, 0}};

void check_config_flags(uint32_t flags) {
    constexpr uint32_t kResultBits = IRE_FLAG_RESULT_PNG_BASE64 | IRE_FLAG_RESULT_PNG_DEFLATE | IRE_FLAG_RESULT_JPEG;
    if (flags & ~(kResultBits | IRE_FLAG_DECODE_PROGRESSIVE | IRE_FLAG_JPEG_OPTIMIZE | IRE_FLAG_UPLOAD_ICC | IRE_FLAG_DECODE_PNG | IRE_FLAG_JPEG_PROGRESSIVE | IRE_FLAG_DECODE_PNG_ALL)) fail(IRE_ERR_INVALID_INPUT, "invalid ire_config.flags (unknown bits set)");
    if (((flags & kResultBits) & ((flags & kResultBits) - 1)) != 0) fail(IRE_ERR_INVALID_INPUT, "invalid ire_config.flags (two result formats set)");
    if ((flags & IRE_FLAG_DECODE_PNG_ALL) && !(flags & IRE_FLAG_DECODE_PNG))
        fail(IRE_ERR_INVALID_INPUT, "invalid ire_config.flags: IRE_FLAG_DECODE_PNG_ALL set without IRE_FLAG_DECODE_PNG");
}

const TextFormat* result_format_of(uint32_t flags) {
    return (flags & IRE_FLAG_RESULT_PNG_DEFLATE) ? &kDeflatePng : (flags & IRE_FLAG_RESULT_JPEG) ? &kJpeg : (flags & IRE_FLAG_RESULT_PNG_BASE64) ? &kStoredPng : nullptr;
}

TextSettings jpeg_settings_of(int quality, int sampling, bool optimize, bool progressive) {
    if (quality < 0 || quality > 100) fail(IRE_ERR_INVALID_INPUT, "invalid: JPEG quality must be in 1..100 (0: the default, 85)");
    if (sampling != 0 && sampling != 2) fail(IRE_ERR_INVALID_INPUT, "invalid: JPEG sampling must be 0 (4:4:4) or 2 (4:2:0); 4:2:2 and grey results are not built");
    return {quality ? quality : kJpegDefaultQuality, sampling, optimize ? 1 : 0, progressive ? 1 : 0};
}

TextSettings check_config_jpeg(uint32_t flags, int quality, int sampling) {
    if ((quality || sampling) && !(flags & IRE_FLAG_RESULT_JPEG))
        fail(IRE_ERR_INVALID_INPUT, "invalid ire_config: jpeg_quality or jpeg_sampling set without IRE_FLAG_RESULT_JPEG");
    if ((flags & IRE_FLAG_JPEG_OPTIMIZE) && !(flags & IRE_FLAG_RESULT_JPEG))
        fail(IRE_ERR_INVALID_INPUT, "invalid ire_config.flags: IRE_FLAG_JPEG_OPTIMIZE set without IRE_FLAG_RESULT_JPEG");
    if ((flags & IRE_FLAG_JPEG_PROGRESSIVE) && !(flags & IRE_FLAG_RESULT_JPEG))
        fail(IRE_ERR_INVALID_INPUT, "invalid ire_config.flags: IRE_FLAG_JPEG_PROGRESSIVE set without IRE_FLAG_RESULT_JPEG");
    return jpeg_settings_of(quality, sampling, (flags & IRE_FLAG_JPEG_OPTIMIZE) != 0, (flags & IRE_FLAG_JPEG_PROGRESSIVE) != 0);
}

TextFormat jpeg_format_of(TextSettings o) {
    TextFormat f = kJpeg.with(o);
    if (o.optimize) f.bound_name = "ire_jpeg_optimized_base64_bound";
    if (o.progressive) f.bound_name = "ire_jpeg_progressive_base64_bound";
    return f;
}

namespace {
// every refusal of an encoder entry: "invalid <what> the <PNG | JPEG> encoder<why>"
std::string enc(const TextFormat& f, const char* what, const char* why) { return std::string("invalid ") + what + " the " + f.noun + " encoder" + why; }
void check_stride(const TextFormat& f, size_t stride, size_t bound) {
    if (stride < bound) fail(IRE_ERR_INVALID_INPUT, enc(f, "stride for", ": smaller than ") + f.bound_name + "(h, w)");
}
}  // namespace

// ---- the text encoders: three launches or four and at most one small memset per batch ---------------------------------------------------

void TextEncoder::window(const TextFormat& f, const uint8_t* d_rgb, int n, int h, int w, size_t row_pitch, size_t image_pitch, uint8_t* d_chars, size_t stride,
                         uint8_t* d_lens, size_t lens_pitch, hipStream_t s) {
    check_stride(f, stride, f.bound(h, w));
    if (row_pitch < (size_t)3 * w || (n > 1 && image_pitch < row_pitch * (size_t)(h - 1) + (size_t)3 * w))
        fail(IRE_ERR_INVALID_INPUT, enc(f, "pitch for", ": rows or images overlap"));
    const size_t need = f.scratch_bytes(n, h, w);
    if (need > d_scratch_.bytes()) IRE_HIP(hipDeviceSynchronize());
    d_scratch_.grow(need, batch_room(need, f.scratch_bytes(max_batch_, h, w)));
    f.launch(d_rgb, n, h, w, row_pitch, image_pitch, d_scratch_.get<uint8_t>(), d_chars, stride, d_lens, lens_pitch, s);
}

void TextEncoder::encode_device(const TextFormat& f, const uint8_t* d_rgb, int n, int h, int w, size_t row_pitch, size_t image_pitch, uint8_t* d_chars, size_t stride,
                                uint64_t* d_lens, hipStream_t s) {
    if (!d_rgb || !d_chars || (f.counted && !d_lens) || n < 1 || n > max_batch_) fail(IRE_ERR_INVALID_INPUT, enc(f, "arguments to", " (1..max_batch images)"));
    if (h < 1 || w < 1 || h > 8192 || w > 8192) fail(IRE_ERR_INVALID_INPUT, enc(f, "image size for", ": height and width must be in 1..8192"));
    window(f, d_rgb, n, h, w, row_pitch, image_pitch, d_chars, stride, reinterpret_cast<uint8_t*>(d_lens), sizeof(uint64_t), s);
}

void TextEncoder::encode_png_aligned_device(const uint8_t* d_rgb, int n, int h, int w, uint8_t* d_chars, size_t stride, hipStream_t s) {
    const TextFormat& f = kStoredPng;
    if (!d_rgb || !d_chars || n < 1 || n > max_batch_) fail(IRE_ERR_INVALID_INPUT, enc(f, "arguments to", " (1..max_batch images)"));
    if (h < 1 || w < 8 || w % 8 || h > 16384 || w > 16384) fail(IRE_ERR_INVALID_INPUT, enc(f, "image size for", ": width must be a multiple of 8"));
    window(f, d_rgb, n, h, w, (size_t)3 * w, (size_t)3 * w * h, d_chars, stride, nullptr, 0, s);
}

void TextEncoder::encode_host(const TextFormat& f, const uint8_t* rgb, int n, int h, int w, uint8_t* chars, size_t stride, uint64_t* lens) {
    if (!rgb || !chars || (f.counted && !lens)) fail(IRE_ERR_INVALID_INPUT, enc(f, "arguments to", ": null buffer"));
    if (n < 1 || n > max_batch_ || h < 1 || w < 1 || h > 8192 || w > 8192) fail(IRE_ERR_INVALID_INPUT, enc(f, "arguments to", " (1..max_batch images, 1..8192 per side)"));
    run_host(f, rgb, n, h, w, chars, stride, lens);
}

void TextEncoder::encode_png_aligned_host(const uint8_t* rgb, int n, int h, int w, uint8_t* chars, size_t stride) {
    const TextFormat& f = kStoredPng;
    if (!rgb || !chars) fail(IRE_ERR_INVALID_INPUT, enc(f, "arguments to", ": null buffer"));
    if (n < 1 || n > max_batch_ || h < 1 || w < 8 || w % 8 || h > 16384 || w > 16384) fail(IRE_ERR_INVALID_INPUT, enc(f, "arguments to", " (1..max_batch images, width a multiple of 8)"));
    run_host(f, rgb, n, h, w, chars, stride, nullptr);
}

// pixels up, the result places (256-byte aligned) down as the format's bound asks (TextFormat::counts_first)
void TextEncoder::run_host(const TextFormat& f, const uint8_t* rgb, int n, int h, int w, uint8_t* chars, size_t stride, uint64_t* lens) {
    const size_t ib = (size_t)h * w * 3, cb = f.bound(h, w), head = f.counted ? 8 : 0, cpad = (cb + head + 255) / 256 * 256;
    check_stride(f, stride, cb);
    const size_t in_pad = (ib * n + 255) / 256 * 256, io = in_pad + cpad * (size_t)n;
    if (io > d_io_.bytes()) IRE_HIP(hipDeviceSynchronize());
    d_io_.grow(io);
    hipStream_t s = main_stream_;
    uint8_t* d_px = d_io_.get<uint8_t>();
    IRE_HIP(hipMemcpyAsync(d_px, rgb, ib * n, hipMemcpyHostToDevice, s));
    uint8_t* d_txt = d_px + in_pad;
    places(f, d_px, n, h, w, (size_t)3 * w, ib, d_txt, cpad, s);
    std::vector<uint8_t> stage;
    if (!f.counted) {
        for (int i = 0; i < n; ++i) IRE_HIP(hipMemcpyAsync(chars + stride * i, d_txt + cpad * i, cb, hipMemcpyDeviceToHost, s));
    } else if (f.counts_first) {
        for (int i = 0; i < n; ++i) IRE_HIP(hipMemcpyAsync(&lens[i], d_txt + cpad * i, 8, hipMemcpyDeviceToHost, s));
    } else {         // the host learns the lengths from the D2H that carries the text
        stage.resize(cpad * (size_t)n);
        IRE_HIP(hipMemcpyAsync(stage.data(), d_txt, stage.size(), hipMemcpyDeviceToHost, s));
    }
    IRE_HIP(hipStreamSynchronize(s));
    if (!f.counted) return;
    for (int i = 0; i < n; ++i) {
        uint64_t len = lens[i];
        if (!f.counts_first) std::memcpy(&len, stage.data() + cpad * i, 8);
        if (len > cb) fail(IRE_ERR_INTERNAL, std::string("internal: the ") + f.noun + " encoder reported a length beyond its bound");
        lens[i] = len;
        if (f.counts_first) IRE_HIP(hipMemcpyAsync(chars + stride * i, d_txt + cpad * i + 8, (size_t)len, hipMemcpyDeviceToHost, s));
        else std::memcpy(chars + stride * i, stage.data() + cpad * i + 8, (size_t)len);
    }
    if (f.counts_first) IRE_HIP(hipStreamSynchronize(s));
}

// the optimised JPEG path's table kernel alone, synchronous on the main stream: counts up, tables and symbol counts down
void TextEncoder::debug_jpeg_huffman(const uint32_t* counts, int n, uint8_t* bits_vals_out, int32_t* nvals_out) {
    if (!counts || !bits_vals_out || !nvals_out || n < 1 || n > 4096) fail(IRE_ERR_INVALID_INPUT, "invalid arguments to ire_debug_jpeg_huffman (1..4096 sets of four histograms)");
    const size_t cb = (size_t)n * 4 * 256 * sizeof(uint32_t), tb = (size_t)n * 4 * (16 + 256), tpad = (tb + 255) / 256 * 256, nb = (size_t)n * 4 * sizeof(int32_t);
    if (cb + tpad + nb > d_io_.bytes()) IRE_HIP(hipDeviceSynchronize());
    d_io_.grow(cb + tpad + nb);
    hipStream_t s = main_stream_;
    uint8_t* d = d_io_.get<uint8_t>();
    IRE_HIP(hipMemcpyAsync(d, counts, cb, hipMemcpyHostToDevice, s));
    jpeg_huffman_tables_launch(reinterpret_cast<const unsigned*>(d), n, d + cb, reinterpret_cast<int*>(d + cb + tpad), s);
    IRE_HIP(hipMemcpyAsync(bits_vals_out, d + cb, tb, hipMemcpyDeviceToHost, s));
    IRE_HIP(hipMemcpyAsync(nvals_out, d + cb + tpad, nb, hipMemcpyDeviceToHost, s));
    IRE_HIP(hipStreamSynchronize(s));
}

// the progressive JPEG path behind its coefficient pass, synchronous on the main stream: coefficients up, files and lengths down
void TextEncoder::debug_jpeg_progressive(const int16_t* coefs, int n, int h, int w, int quality, int sampling, uint8_t* files_out, size_t stride, uint64_t* lens_out) {
    if (!coefs || !files_out || !lens_out || n < 1 || n > max_batch_ || h < 1 || w < 1 || h > 8192 || w > 8192)
        fail(IRE_ERR_INVALID_INPUT, "invalid arguments to ire_debug_jpeg_progressive_from_coefs (1..max_batch images, 1..8192 per side)");
    const TextSettings o = jpeg_settings_of(quality, sampling, false, true);
    const size_t bound = jpeg_progressive_file_bound(h, w, o.quality, o.sampling);
    if (stride < bound) fail(IRE_ERR_INVALID_INPUT, "invalid stride for ire_debug_jpeg_progressive_from_coefs: smaller than the file bound");
    const size_t cb = (size_t)n * jpeg_progressive_coef_count(h, w, o.sampling) * sizeof(int16_t), need = jpeg_progressive_scratch_bytes(n, h, w, o.quality, o.sampling);
    if (cb > d_io_.bytes() || need > d_scratch_.bytes()) IRE_HIP(hipDeviceSynchronize());
    d_io_.grow(cb);
    d_scratch_.grow(need);
    hipStream_t s = main_stream_;
    uint8_t* d = d_io_.get<uint8_t>();
    uint8_t* sc = d_scratch_.get<uint8_t>();
    IRE_HIP(hipMemcpyAsync(d, coefs, cb, hipMemcpyHostToDevice, s));
    size_t files_off = 0, file_pitch = 0, flen_off = 0;
    jpeg_progressive_from_coefs_launch(reinterpret_cast<const short*>(d), n, h, w, o.quality, o.sampling, sc, &files_off, &file_pitch, &flen_off, s);
    IRE_HIP(hipMemcpyAsync(lens_out, sc + flen_off, (size_t)n * 8, hipMemcpyDeviceToHost, s));
    IRE_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < n; ++i) {
        if (lens_out[i] > bound) fail(IRE_ERR_INTERNAL, "internal: the JPEG encoder reported a length beyond its bound");
        IRE_HIP(hipMemcpyAsync(files_out + stride * i, sc + files_off + file_pitch * i, (size_t)lens_out[i], hipMemcpyDeviceToHost, s));
    }
    IRE_HIP(hipStreamSynchronize(s));
}

// ---- the JPEG decoder (jpeg_parse.hpp on the host, jpeg_dec.hip on the device) ------------------------------------------------------------

JpegDecoder::JpegDecoder() {
    if (const char* v = std::getenv("IRE_JPEG_DEC_TIMES")) times_ = std::atoi(v) != 0;
    if (const char* v = std::getenv("IRE_JPEG_DEC_WINDOWS")) min_windows_ = (uint32_t)std::max(0, std::atoi(v));
}

JpegDecoder::~JpegDecoder() {
    for (hipEvent_t ev : marks_) if (ev) (void)hipEventDestroy(ev);
}

// two pinned blobs in turn: the one handed out was last uploaded by the call before last, and that upload must have left it
int JpegDecoder::Scratch::next_pin(size_t bytes) {
    const int t = turn;
    turn ^= 1;
    if (up_recorded[t]) IRE_HIP(hipEventSynchronize(up_ev[t]));
    pin[t].grow(bytes, bytes + bytes / 2);
    return t;
}

void JpegDecoder::run(Scratch& S, int turn, const JpegDecLayout& L, size_t pin_bytes, const uint8_t* const* tails, const size_t* tail_bytes, const size_t* tail_off, int n, int h,
                      int w, uint8_t* d_rgb, size_t image_pitch, int32_t* d_status, hipStream_t s, const int* dst) {
    const bool own = &S == &own_, timed = own && times_;
    const size_t coef = jpeg_dec_coef_bytes(n, h, w), planes = jpeg_dec_plane_bytes(n, h, w);
    const size_t lanes = jpeg_dec_lane_bytes(L.nwin), walk = L.walk_blocks ? jpeg_dec_walk_bytes(L.walk_blocks) : 0;
    // before a buffer goes, nothing enqueued may still use it: the whole device, or the one stream that ever uses the batcher's scratch
    if (L.total > S.d_in.bytes() || coef > S.d_coef.bytes() || planes > S.d_planes.bytes() || lanes > S.d_lanes.bytes() || walk > S.d_walk.bytes())
        IRE_HIP(own ? hipDeviceSynchronize() : hipStreamSynchronize(s));
    S.d_in.grow(L.total, L.total + L.total / 2);
    S.d_coef.grow(coef, batch_room(coef, jpeg_dec_coef_bytes(max_batch_, h, w)));
    S.d_planes.grow(planes, batch_room(planes, jpeg_dec_plane_bytes(max_batch_, h, w)));
    if (lanes) S.d_lanes.grow(lanes, lanes + lanes / 2);
    if (walk) S.d_walk.grow(walk, walk + walk / 2);
    uint8_t* d_in = S.d_in.get<uint8_t>();
    IRE_HIP(hipMemcpyAsync(d_in, S.pin[turn].get<uint8_t>(), pin_bytes, hipMemcpyHostToDevice, s));
    if (!S.up_ev[turn]) IRE_HIP(hipEventCreateWithFlags(&S.up_ev[turn], hipEventDisableTiming));
    IRE_HIP(hipEventRecord(S.up_ev[turn], s));
    S.up_recorded[turn] = true;
    for (int i = 0; tails && i < n; ++i)
        if (tail_bytes[i]) IRE_HIP(hipMemcpyAsync(d_in + pin_bytes + tail_off[i], tails[i], tail_bytes[i], hipMemcpyHostToDevice, s));
    if (timed) {
        times_collect();
        for (hipEvent_t& ev : marks_) if (!ev) IRE_HIP(hipEventCreate(&ev));
    }
    jpeg_dec_launch(d_in, L, n, h, w, S.d_coef.get<uint8_t>(), S.d_planes.get<uint8_t>(), lanes ? S.d_lanes.get<uint8_t>() : nullptr, walk ? S.d_walk.get<uint8_t>() : nullptr,
                    d_rgb, image_pitch, d_status, s, timed ? marks_ : nullptr, dst);
    if (own) marks_pending_ = times_;
}

void JpegDecoder::decode_files(const uint8_t* const* files, const size_t* bytes, int n, int h, int w, uint8_t* d_rgb, size_t image_pitch, int32_t* d_status, hipStream_t s) {
    if (!files || !bytes || !d_rgb || !d_status || n < 1 || n > max_batch_) fail(IRE_ERR_INVALID_INPUT, "invalid arguments to the JPEG decoder (1..max_batch files)");
    if (h < 1 || w < 1 || h > 8192 || w > 8192) fail(IRE_ERR_INVALID_INPUT, "invalid image size for the JPEG decoder: height and width must be in 1..8192");
    if (image_pitch < (size_t)3 * w * h) fail(IRE_ERR_INVALID_INPUT, "invalid pitch for the JPEG decoder: images overlap");
    std::vector<jpegparse::File> hd((size_t)n);
    for (int i = 0; i < n; ++i) {
        std::string why;
        if (!files[i] || !jpegparse::head_file(files[i], bytes[i], accept_, hd[i], why))
            fail(IRE_ERR_INVALID_INPUT, files[i] ? why : "invalid arguments to the JPEG decoder: null file");
        if (hd[i].hd.im.h != h || hd[i].hd.im.w != w) fail(IRE_ERR_INVALID_INPUT, "invalid: the JPEG file's size is not the planned h x w");
    }
    const JpegDecLayout L0 = jpeg_dec_layout(hd.data(), bytes, n);
    if (L0.total >= ((size_t)1 << 32)) fail(IRE_ERR_INVALID_INPUT, "invalid: the batch's JPEG files exceed 4 GB");
    const int turn = own_.next_pin(L0.total);
    JpegDecLayout L;
    jpeg_dec_pack(files, bytes, hd.data(), n, L0, own_.pin[turn].get<uint8_t>(), L, min_windows_);
    run(own_, turn, L, L.total, nullptr, nullptr, nullptr, n, h, w, d_rgb, image_pitch, d_status, s);
}

void JpegDecoder::decode_streams(const jpegparse::File* const* hd, const jpegdec::DecStream* const* streams, const uint8_t* const* bytes, const size_t* used, int n, int h,
                                 int w, uint8_t* d_rgb, size_t image_pitch, int32_t* d_status, hipStream_t s, const int* dst) {
    if (!hd || !streams || !bytes || !used || !d_rgb || !d_status || n < 1 || n > max_batch_) fail(IRE_ERR_INTERNAL, "internal: arguments of the batcher's JPEG decode");
    std::vector<uint32_t> ns((size_t)n), nu((size_t)n);
    for (int i = 0; i < n; ++i) {
        if (hd[i]->hd.im.h != h || hd[i]->hd.im.w != w) fail(IRE_ERR_INTERNAL, "internal: a file job in a slot of another size");
        ns[(size_t)i] = hd[i]->nstreams; nu[(size_t)i] = hd[i]->nscans();
    }
    const JpegDecLayout L0 = jpeg_dec_layout_rooms(ns.data(), nu.data(), used, n);
    if (L0.total >= ((size_t)1 << 32)) fail(IRE_ERR_INVALID_INPUT, "invalid: the batch's JPEG files exceed 4 GB");
    const int turn = batch_.next_pin(L0.bytes);
    JpegDecLayout L;
    std::vector<size_t> off((size_t)n);
    jpeg_dec_pack_streams(hd, streams, used, n, L0, batch_.pin[turn].get<uint8_t>(), L, off.data(), min_windows_);
    // the streams go from where their submitters cut them (the slot's pinned input) straight to the blob on the device
    run(batch_, turn, L, L.bytes, bytes, used, off.data(), n, h, w, d_rgb, image_pitch, d_status, s, dst);
}

void JpegDecoder::times_collect() {
    if (!marks_pending_) return;
    marks_pending_ = false;
    if (hipEventSynchronize(marks_[kJpegDecMarks - 1]) != hipSuccess) return;
    for (int k = 0; k < kJpegDecMarks - 1; ++k) { float ms = 0.f; if (hipEventElapsedTime(&ms, marks_[k], marks_[k + 1]) == hipSuccess) ms_[k] += ms; }
    ++calls_;
}

void JpegDecoder::report_times() {
    if (!times_) return;
    times_collect();
    std::fprintf(stderr,
                 "{\"jpeg_dec_kernel_ms\": {\"memset\": %.4f, \"long\": %.4f, \"spec\": %.4f, \"chain\": %.4f, \"write\": %.4f, \"short\": %.4f, \"idct\": %.4f, "
                 "\"colour\": %.4f, \"calls\": %lld, \"later_scans\": %.4f}}\n",
                 ms_[0], ms_[1], ms_[2], ms_[3], ms_[4], ms_[5], ms_[7], ms_[8], (long long)calls_, ms_[6]);
}

void JpegDecoder::decode_host(const uint8_t* file, size_t bytes, uint8_t* out_rgb, int h, int w) {
    if (!file || !out_rgb) fail(IRE_ERR_INVALID_INPUT, "invalid arguments to the JPEG decoder: null buffer");
    if (h < 1 || w < 1 || h > 8192 || w > 8192) fail(IRE_ERR_INVALID_INPUT, "invalid image size for the JPEG decoder: height and width must be in 1..8192");
    const size_t ib = (size_t)h * w * 3, ipad = (ib + 255) / 256 * 256;
    if (ipad + 256 > d_out_.bytes()) IRE_HIP(hipDeviceSynchronize());
    d_out_.grow(ipad + 256);
    hipStream_t s = main_stream_;
    uint8_t* d_px = d_out_.get<uint8_t>();
    int32_t* d_st = reinterpret_cast<int32_t*>(d_px + ipad);
    decode_files(&file, &bytes, 1, h, w, d_px, ib, d_st, s);
    int32_t st = 0;
    IRE_HIP(hipMemcpyAsync(out_rgb, d_px, ib, hipMemcpyDeviceToHost, s));
    IRE_HIP(hipMemcpyAsync(&st, d_st, sizeof(st), hipMemcpyDeviceToHost, s));
    IRE_HIP(hipStreamSynchronize(s));
    // (bits: jpeg_dec_core.hpp kSt*; 16 = values no picture gives, where libjpeg-turbo's C and SIMD code differ)
    if (st != 0) fail(IRE_ERR_INVALID_INPUT, "invalid: corrupt JPEG data (decoder status " + std::to_string(st) + ")");
}

// ---- the PNG decoder (png_parse.hpp on the host, png_dec.hip on the device) ---------------------------------------------------------------

void PngDecoder::setup(int max_batch, bool enabled, bool accept_all, hipStream_t main_stream) {
    max_batch_ = max_batch; enabled_ = enabled; accept_ = accept_all ? pngparse::kAcceptAll : 0u; main_stream_ = main_stream;
    if (const char* v = std::getenv("IRE_PNG_DEC_TIMES")) times_ = std::atoi(v) != 0;
}

PngDecoder::~PngDecoder() {
    if (times_) {
        times_collect();
        std::fprintf(stderr, "{\"png_dec_kernel_ms\": {\"inflate\": %.4f, \"unfilter\": %.4f, \"calls\": %lld, \"walk_share\": %.4f, \"place_share\": %.4f}}\n", ms_[0], ms_[1],
                     (long long)calls_, ticks_[2] > 0 ? ticks_[0] / ticks_[2] : 0.0, ticks_[2] > 0 ? ticks_[1] / ticks_[2] : 0.0);
    }
    for (hipEvent_t ev : marks_) if (ev) (void)hipEventDestroy(ev);
}

void PngDecoder::check_enabled() const {
    if (!enabled_) fail(IRE_ERR_INVALID_INPUT, "invalid: this engine does not decode PNG files (create it with IRE_FLAG_DECODE_PNG)");
}

int PngDecoder::Scratch::next_pin(size_t bytes) {
    const int t = turn;
    turn ^= 1;
    if (up_recorded[t]) IRE_HIP(hipEventSynchronize(up_ev[t]));
    pin[t].grow(bytes, bytes + bytes / 2);
    return t;
}

void PngDecoder::times_collect() {
    if (!marks_pending_) return;
    marks_pending_ = false;
    if (hipEventSynchronize(marks_[2]) != hipSuccess) return;
    for (int k = 0; k < 2; ++k) { float ms = 0.f; if (hipEventElapsedTime(&ms, marks_[k], marks_[k + 1]) == hipSuccess) ms_[k] += ms; }
    ++calls_;
    std::vector<unsigned long long> t(3 * (size_t)ticks_n_);
    if (ticks_n_ && hipMemcpy(t.data(), d_ticks_.get<void>(), t.size() * 8, hipMemcpyDeviceToHost) == hipSuccess)
        for (size_t i = 0; i < t.size(); ++i) ticks_[i % 3] += (double)t[i];
}

void PngDecoder::run(Scratch& S, int turn, const PngDecLayout& L, size_t pin_bytes, const uint8_t* const* tails, const size_t* tail_bytes, const pngdec::Record* rec, int n, int h,
                     int w, uint8_t* d_rgb, size_t image_pitch, int32_t* d_status, hipStream_t s) {
    const bool own = &S == &own_, timed = own && times_;
    // the scanlines of a whole batch of four-byte pixels: the first batch of a shape allocates, later ones of any colour types do not
    // (with kAcceptAll the largest form is interlaced 16-bit RGBA: eight-byte pixels and seven passes' filter bytes)
    const size_t scan_one = accept_ ? (size_t)pngdec::scan_total((uint32_t)h, (uint32_t)w, 6, 16, 1) : (size_t)h * (1 + (size_t)w * 4);
    const size_t scan_full = ((scan_one + 15) & ~(size_t)15) * (size_t)max_batch_;
    if (L.total > S.d_in.bytes() || L.scan_bytes > S.d_scan.bytes()) IRE_HIP(own ? hipDeviceSynchronize() : hipStreamSynchronize(s));
    S.d_in.grow(L.total, L.total + L.total / 2);
    S.d_scan.grow(L.scan_bytes, batch_room(L.scan_bytes, scan_full));
    uint8_t* d_in = S.d_in.get<uint8_t>();
    IRE_HIP(hipMemcpyAsync(d_in, S.pin[turn].get<uint8_t>(), pin_bytes, hipMemcpyHostToDevice, s));
    if (!S.up_ev[turn]) IRE_HIP(hipEventCreateWithFlags(&S.up_ev[turn], hipEventDisableTiming));
    IRE_HIP(hipEventRecord(S.up_ev[turn], s));
    S.up_recorded[turn] = true;
    for (int i = 0; tails && i < n; ++i)
        if (tail_bytes[i]) IRE_HIP(hipMemcpyAsync(d_in + L.bytes + rec[i].in_off, tails[i], tail_bytes[i], hipMemcpyHostToDevice, s));
    if (timed) {
        times_collect();
        for (hipEvent_t& ev : marks_) if (!ev) IRE_HIP(hipEventCreate(&ev));
        d_ticks_.grow(sizeof(unsigned long long) * 3 * (size_t)max_batch_);
        ticks_n_ = n;
    }
    png_dec_launch(d_in, L, n, h, w, S.d_scan.get<uint8_t>(), d_rgb, image_pitch, d_status, s, timed ? marks_ : nullptr, timed ? d_ticks_.get<unsigned long long>() : nullptr);
    if (own) marks_pending_ = timed;
}

void PngDecoder::decode_files(const uint8_t* const* files, const size_t* bytes, int n, int h, int w, uint8_t* d_rgb, size_t image_pitch, int32_t* d_status, hipStream_t s) {
    check_enabled();
    if (!files || !bytes || !d_rgb || !d_status || n < 1 || n > max_batch_) fail(IRE_ERR_INVALID_INPUT, "invalid arguments to the PNG decoder (1..max_batch files)");
    if (h < 1 || w < 1 || h > 8192 || w > 8192) fail(IRE_ERR_INVALID_INPUT, "invalid image size for the PNG decoder: height and width must be in 1..8192");
    if (image_pitch < (size_t)3 * w * h) fail(IRE_ERR_INVALID_INPUT, "invalid pitch for the PNG decoder: images overlap");
    std::vector<pngparse::File> hd((size_t)n);
    std::vector<const pngparse::File*> hp((size_t)n);
    std::vector<size_t> rooms((size_t)n);
    for (int i = 0; i < n; ++i) {
        std::string why;
        if (!files[i] || !pngparse::plan_file(files[i], bytes[i], accept_, hd[(size_t)i], why)) fail(IRE_ERR_INVALID_INPUT, files[i] ? why : "invalid arguments to the PNG decoder: null file");
        if (hd[(size_t)i].h != h || hd[(size_t)i].w != w) fail(IRE_ERR_INVALID_INPUT, "invalid: the PNG file's size is not the planned h x w");
        hp[(size_t)i] = &hd[(size_t)i]; rooms[(size_t)i] = hd[(size_t)i].idat_bytes;
    }
    const PngDecLayout L = png_dec_layout(hp.data(), rooms.data(), nullptr, n, nullptr);
    if (L.total >= ((size_t)1 << 32)) fail(IRE_ERR_INVALID_INPUT, "invalid: the batch's PNG files exceed 4 GB");
    const int turn = own_.next_pin(L.total);
    uint8_t* blob = own_.pin[turn].get<uint8_t>();
    pngdec::Record* rec = reinterpret_cast<pngdec::Record*>(blob);
    (void)png_dec_layout(hp.data(), rooms.data(), nullptr, n, rec);
    for (int i = 0; i < n; ++i) {
        std::string why;
        if (pngparse::stage(hd[(size_t)i], files[i], bytes[i], blob + L.bytes + rec[i].in_off, rooms[(size_t)i], why) != rooms[(size_t)i]) fail(IRE_ERR_INVALID_INPUT, why);
    }
    run(own_, turn, L, L.total, nullptr, nullptr, rec, n, h, w, d_rgb, image_pitch, d_status, s);
}

void PngDecoder::decode_staged(const pngparse::File* const* f, const uint8_t* const* bytes, const size_t* used, const int* dst, int n, int h, int w, uint8_t* d_rgb,
                               size_t image_pitch, int32_t* d_status, hipStream_t s) {
    if (!enabled_ || !f || !bytes || !used || !dst || !d_rgb || !d_status || n < 1 || n > max_batch_) fail(IRE_ERR_INTERNAL, "internal: arguments of the batcher's PNG decode");
    for (int i = 0; i < n; ++i)
        if (f[i]->h != h || f[i]->w != w || used[i] != f[i]->idat_bytes) fail(IRE_ERR_INTERNAL, "internal: a PNG job in a slot of another size");
    const PngDecLayout L = png_dec_layout(f, used, dst, n, nullptr);
    if (L.total >= ((size_t)1 << 32)) fail(IRE_ERR_INVALID_INPUT, "invalid: the batch's PNG files exceed 4 GB");
    const int turn = batch_.next_pin(L.bytes);
    pngdec::Record* rec = reinterpret_cast<pngdec::Record*>(batch_.pin[turn].get<uint8_t>());
    (void)png_dec_layout(f, used, dst, n, rec);
    // the streams go from where their submitters staged them (the slot's pinned input) straight to the blob on the device
    run(batch_, turn, L, L.bytes, bytes, used, rec, n, h, w, d_rgb, image_pitch, d_status, s);
}

void PngDecoder::decode_host(const uint8_t* file, size_t bytes, uint8_t* out_rgb, int h, int w) {
    check_enabled();
    if (!file || !out_rgb) fail(IRE_ERR_INVALID_INPUT, "invalid arguments to the PNG decoder: null buffer");
    if (h < 1 || w < 1 || h > 8192 || w > 8192) fail(IRE_ERR_INVALID_INPUT, "invalid image size for the PNG decoder: height and width must be in 1..8192");
    const size_t ib = (size_t)h * w * 3, ipad = (ib + 255) / 256 * 256;
    if (ipad + 256 > d_out_.bytes()) IRE_HIP(hipDeviceSynchronize());
    d_out_.grow(ipad + 256);
    hipStream_t s = main_stream_;
    uint8_t* d_px = d_out_.get<uint8_t>();
    int32_t* d_st = reinterpret_cast<int32_t*>(d_px + ipad);
    decode_files(&file, &bytes, 1, h, w, d_px, ib, d_st, s);
    int32_t st = 0;
    IRE_HIP(hipMemcpyAsync(out_rgb, d_px, ib, hipMemcpyDeviceToHost, s));
    IRE_HIP(hipMemcpyAsync(&st, d_st, sizeof(st), hipMemcpyDeviceToHost, s));
    IRE_HIP(hipStreamSynchronize(s));
    // (png_inflate_core.hpp Status.  Flagged: whatever zlib would not decompress to exactly the scanlines' bytes (File::scan_bytes) with filter bytes 0..4.
    // Pillow zero-fills a short stream and ignores a long one; the device flags both, and the host codec then decides.)
    if (st != 0) fail(IRE_ERR_INVALID_INPUT, "invalid: corrupt PNG data (decoder status " + std::to_string(st) + ")");
}

}  // namespace ire
