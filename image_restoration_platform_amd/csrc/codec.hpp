// codec.hpp -- the codecs around the network: restored pixels -> the base64 text of a PNG / JPEG file (encode.hip, deflate.hip, jpeg.hip)
// and JPEG uploads -> pixels (jpeg_parse.hpp, jpeg_dec.hip).  One constant description per text format, one path per direction; the
// engine holds one TextEncoder and one JpegDecoder and touches neither's buffers.  Host only.
#pragma once
#include "common.hpp"
#include "device_buf.hpp"
#include "jpeg_dec.hpp"
#include "png_dec.hpp"

namespace ire {

// The format's settings, chosen per engine or per direct call: JPEG's quality (1..100), sampling (0 = 4:4:4, 2 = 4:2:0), optimize
// (0 | 1: the image's own Huffman tables) and progressive (0 | 1: the ten-scan progressive file of jpeg_progenc.hip, whose tables are
// always its own: optimize beside it changes nothing).  The PNG formats have none and ignore them.
struct TextSettings { int quality, sampling, optimize, progressive; };
struct TextFormat {
    const char* noun;                                   // the encoder as its messages name it: "PNG" | "JPEG"
    size_t (*bound_fn)(int h, int w, TextSettings o);   // the most characters an h x w image gives (stored PNG: exactly so many)
    const char* bound_name;                             // ... under its public name (include/ire.h)
    size_t (*scratch_fn)(int n, int h, int w, TextSettings o);      // device scratch of a batch of n
    // the top-left h x w window of n images -> n texts `stride` apart and, for a counted format, their uint64 counts lens_pitch apart
    void (*launch_fn)(const uint8_t* d_rgb, int n, int h, int w, size_t row_pitch, size_t image_pitch, uint8_t* d_scratch, uint8_t* d_chars, size_t stride,
                      uint8_t* d_lens, size_t lens_pitch, TextSettings o, hipStream_t s);
    bool counted;                                       // the text's length depends on the pixels: a result is [uint64 count | text]
    // how the host entry fetches counted results.  false: [count | text] places whole, in ONE copy (the bound is tight: deflate);
    // true: the counts first, then only what they name (the bound is several times a real text: it doubles every byte for stuffing)
    bool counts_first;
    TextSettings settings;                              // a row of the table holds the format's defaults; with() gives a copy with others
    size_t bound(int h, int w) const { return bound_fn(h, w, settings); }
    size_t scratch_bytes(int n, int h, int w) const { return scratch_fn(n, h, w, settings); }
    void launch(const uint8_t* d_rgb, int n, int h, int w, size_t row_pitch, size_t image_pitch, uint8_t* d_scratch, uint8_t* d_chars, size_t stride, uint8_t* d_lens,
                size_t lens_pitch, hipStream_t s) const {
        launch_fn(d_rgb, n, h, w, row_pitch, image_pitch, d_scratch, d_chars, stride, d_lens, lens_pitch, settings, s);
    }
    size_t place_bytes(int h, int w) const { return (counted ? 8 : 0) + bound(h, w); }       // a result's place in a staging buffer
    TextFormat with(TextSettings o) const { TextFormat f = *this; f.settings = o; return f; }
};
extern const TextFormat kStoredPng, kDeflatePng, kJpeg;      // kJpeg: quality 85, 4:4:4
// ire_config.flags: refuses unknown bits and two result formats | the format of the batcher's results, null: pixels
void check_config_flags(uint32_t flags);
const TextFormat* result_format_of(uint32_t flags);
// JPEG settings as the ABI takes them: 0 means the default (85 | 4:4:4); refuses a quality outside 1..100 and a sampling other than 0
// or 2 as "invalid: ..."
TextSettings jpeg_settings_of(int quality, int sampling, bool optimize = false, bool progressive = false);
// ire_config's two JPEG fields, IRE_FLAG_JPEG_OPTIMIZE and IRE_FLAG_JPEG_PROGRESSIVE: jpeg_settings_of, and any of the four set without
// IRE_FLAG_RESULT_JPEG is refused
TextSettings check_config_jpeg(uint32_t flags, int quality, int sampling);
// kJpeg at the settings given; with optimize or progressive its messages name that bound
TextFormat jpeg_format_of(TextSettings o);

// Owns the scratch all formats share and the host entries' staging.  Every call runs under the engine's lock.
class TextEncoder {
public:
    void setup(int max_batch, hipStream_t main_stream) { max_batch_ = max_batch; main_stream_ = main_stream; }
    // the one encoder behind every entry, asynchronous on s.  d_lens: null for a format that is not counted
    void window(const TextFormat& f, const uint8_t* d_rgb, int n, int h, int w, size_t row_pitch, size_t image_pitch, uint8_t* d_chars, size_t stride,
                uint8_t* d_lens, size_t lens_pitch, hipStream_t s);
    // the same into n result places `pitch` apart: [uint64 count | text] for a counted format, else the text
    void places(const TextFormat& f, const uint8_t* d_rgb, int n, int h, int w, size_t row_pitch, size_t image_pitch, uint8_t* d_places, size_t pitch, hipStream_t s) {
        window(f, d_rgb, n, h, w, row_pitch, image_pitch, d_places + (f.counted ? 8 : 0), pitch, f.counted ? d_places : nullptr, pitch, s);
    }
    // the ABI's entries for any size (h, w in 1..8192): device buffers, asynchronous on s | host buffers, synchronous on the main stream
    void encode_device(const TextFormat& f, const uint8_t* d_rgb, int n, int h, int w, size_t row_pitch, size_t image_pitch, uint8_t* d_chars, size_t stride,
                       uint64_t* d_lens, hipStream_t s);
    void encode_host(const TextFormat& f, const uint8_t* rgb, int n, int h, int w, uint8_t* chars, size_t stride, uint64_t* lens);
    // the first entries (stored PNG, w % 8 == 0, up to 16384 per side): their own argument checks in front of the same path
    void encode_png_aligned_device(const uint8_t* d_rgb, int n, int h, int w, uint8_t* d_chars, size_t stride, hipStream_t s);
    void encode_png_aligned_host(const uint8_t* rgb, int n, int h, int w, uint8_t* chars, size_t stride);
    // ire_debug_jpeg_huffman: counts [n][4][256] -> bits_vals_out [n][4][16 + 256], nvals_out [n][4], by jpeg.hip's table kernel alone
    void debug_jpeg_huffman(const uint32_t* counts, int n, uint8_t* bits_vals_out, int32_t* nvals_out);
    // ire_debug_jpeg_progressive_from_coefs: the progressive path behind its coefficient pass on coefficients given (host) -> n files
    // `stride` apart (host) and their lengths
    void debug_jpeg_progressive(const int16_t* coefs, int n, int h, int w, int quality, int sampling, uint8_t* files_out, size_t stride, uint64_t* lens_out);

private:
    void run_host(const TextFormat& f, const uint8_t* rgb, int n, int h, int w, uint8_t* chars, size_t stride, uint64_t* lens);
    int max_batch_ = 8;
    hipStream_t main_stream_ = nullptr;
    Buf<DeviceMem> d_scratch_;            // per batch: the files being assembled and the encoder's state (grows to a whole batch of the shape)
    Buf<DeviceMem> d_io_;                 // host entry: pixels in | result places out
};

// Owns the decoder's buffers.  Two users that never share one: the engine's own entries (decode_files,
// decode_host: under the engine's lock, on the caller's stream) and the batcher's file jobs (decode_streams: ONE thread, the
// batcher's launcher, always on the same stream, without the lock).
class JpegDecoder {
public:
    JpegDecoder();        // reads IRE_JPEG_DEC_WINDOWS and IRE_JPEG_DEC_TIMES
    ~JpegDecoder();
    void setup(int max_batch, uint32_t accept, hipStream_t main_stream) { max_batch_ = max_batch; accept_ = accept; main_stream_ = main_stream; }
    uint32_t accept() const { return accept_; }       // what the parser is asked to take beside baseline files (jpeg_parse.hpp kAccept*)
    // n files of one planned size (jpeg_parse.hpp decides which files) -> n images of h x w x 3 bytes on the device, image_pitch apart,
    // and one status word per image (0: ok).  The host parse runs inside; one upload and a fixed number of launches per batch.  The
    // only wait of the host: for the upload of the call BEFORE LAST, whose pinned staging this call reuses (that upload sits behind
    // the kernels of the call before it, so a caller three calls ahead of the device waits for those).
    void decode_files(const uint8_t* const* files, const size_t* bytes, int n, int h, int w, uint8_t* d_rgb, size_t image_pitch, int32_t* d_status, hipStream_t s);
    // the same for files whose heads were parsed and whose scans were cut by their submitters (streams[i]: hd[i]->nstreams records
    // with offsets inside bytes[i], pinned, used[i] bytes)
    void decode_streams(const jpegparse::File* const* hd, const jpegdec::DecStream* const* streams, const uint8_t* const* bytes, const size_t* used, int n, int h, int w,
                        uint8_t* d_rgb, size_t image_pitch, int32_t* d_status, hipStream_t s, const int* dst = nullptr);
    // dst: null, or which image of d_rgb and which status word file i becomes (a slot that holds other kinds of files between these)
    void decode_host(const uint8_t* file, size_t bytes, uint8_t* out_rgb, int h, int w);      // one file, synchronous on the main stream
    void report_times();      // IRE_JPEG_DEC_TIMES: the summed times as one JSON line on stderr (the engine closes; the device is idle)

private:
    // the batch's upload (records, tables, stream table, stream bytes) pinned and on the device, the coefficient scratch behind the
    // status words, the sample planes
    struct Scratch {
        Buf<PinnedMem> pin[2];            // two, used in turn: call k + 1 is parsed and staged while call k's upload may still run
        Buf<DeviceMem> d_in, d_coef, d_planes;
        Buf<DeviceMem> d_lanes;           // the lane records and window heads of the streams decoded window-parallel
        Buf<DeviceMem> d_walk;            // the masks and walk records of a progressive file's AC refinement scans
        hipEvent_t up_ev[2] = {};         // the last upload out of pin[i]
        bool up_recorded[2] = {};
        int turn = 0;
        Scratch() = default;
        Scratch(const Scratch&) = delete;
        Scratch& operator=(const Scratch&) = delete;
        ~Scratch() { for (hipEvent_t ev : up_ev) if (ev) (void)hipEventDestroy(ev); }
        int next_pin(size_t bytes);       // which blob this call fills: free of its last upload and `bytes` large at least
    };
    // what both entries do once pin[turn] holds the packed batch: grow, upload its first pin_bytes (the batcher's stream bytes follow
    // from where their submitters cut them), record the turn, launch
    void run(Scratch& S, int turn, const JpegDecLayout& L, size_t pin_bytes, const uint8_t* const* tails, const size_t* tail_bytes, const size_t* tail_off, int n, int h, int w,
             uint8_t* d_rgb, size_t image_pitch, int32_t* d_status, hipStream_t s, const int* dst = nullptr);
    void times_collect();

    int max_batch_ = 8;
    uint32_t accept_ = 0;
    hipStream_t main_stream_ = nullptr;
    Scratch own_, batch_;                 // the engine's own entries | the batcher's file jobs
    Buf<DeviceMem> d_out_;                // decode_host: the pixels and the status word
    // IRE_JPEG_DEC_WINDOWS: a long stream of at least so many windows is decoded window-parallel; 0: none, the one-workgroup kernel
    // walks them all (for measurement).  Default, and the least that counts: 2.
    uint32_t min_windows_ = 2;
    // IRE_JPEG_DEC_TIMES=1 (tools/jpeg_decode_measure.py): events between the launches of the engine's own entries, their times summed
    // over the calls.  Collecting waits for the previous call's kernels.
    bool times_ = false, marks_pending_ = false;
    hipEvent_t marks_[kJpegDecMarks] = {};
    double ms_[kJpegDecMarks - 1] = {};
    int64_t calls_ = 0;
};

// The PNG decoder's buffers (png_parse.hpp on the host, png_dec.hip on the device), with the JPEG decoder's two users and its rule for
// the host's one wait.  An engine without IRE_FLAG_DECODE_PNG has the object and refuses every call.
class PngDecoder {
public:
    ~PngDecoder();        // IRE_PNG_DEC_TIMES=1: the two kernels' summed times as one JSON line on stderr (tools/png_decode_measure.py)
    void setup(int max_batch, bool enabled, bool accept_all, hipStream_t main_stream);
    bool enabled() const { return enabled_; }
    // what every plan_file of this engine is asked: pngparse::kAcceptAll on an engine with IRE_FLAG_DECODE_PNG_ALL, else 0
    uint32_t accept() const { return accept_; }
    // n files of one planned size, of any colour types -> n images of h x w x 3 bytes on the device, image_pitch apart, one status word per
    // image (0: ok, else pngdec::Status).  One upload and two launches per batch.
    void decode_files(const uint8_t* const* files, const size_t* bytes, int n, int h, int w, uint8_t* d_rgb, size_t image_pitch, int32_t* d_status, hipStream_t s);
    // the same for files whose submitters planned them and staged their IDAT payloads (bytes[i]: pinned, used[i] bytes); file i becomes image
    // dst[i] and sets status word dst[i]
    void decode_staged(const pngparse::File* const* f, const uint8_t* const* bytes, const size_t* used, const int* dst, int n, int h, int w, uint8_t* d_rgb,
                       size_t image_pitch, int32_t* d_status, hipStream_t s);
    void decode_host(const uint8_t* file, size_t bytes, uint8_t* out_rgb, int h, int w);      // one file, synchronous on the main stream

private:
    struct Scratch {
        Buf<PinnedMem> pin[2];            // two, used in turn (JpegDecoder::Scratch)
        Buf<DeviceMem> d_in, d_scan;      // the batch's upload | the filtered scanlines, n * h * (1 + w * bpp) bytes
        hipEvent_t up_ev[2] = {};
        bool up_recorded[2] = {};
        int turn = 0;
        Scratch() = default;
        Scratch(const Scratch&) = delete;
        Scratch& operator=(const Scratch&) = delete;
        ~Scratch() { for (hipEvent_t ev : up_ev) if (ev) (void)hipEventDestroy(ev); }
        int next_pin(size_t bytes);
    };
    void run(Scratch& S, int turn, const PngDecLayout& L, size_t pin_bytes, const uint8_t* const* tails, const size_t* tail_bytes, const pngdec::Record* rec, int n, int h, int w,
             uint8_t* d_rgb, size_t image_pitch, int32_t* d_status, hipStream_t s);
    void times_collect();
    void check_enabled() const;
    int max_batch_ = 8;
    bool enabled_ = false;
    uint32_t accept_ = 0;
    hipStream_t main_stream_ = nullptr;
    Scratch own_, batch_;
    Buf<DeviceMem> d_out_;                // decode_host: the pixels and the status word
    bool times_ = false, marks_pending_ = false;
    hipEvent_t marks_[3] = {};
    double ms_[2] = {};
    int64_t calls_ = 0;
    Buf<DeviceMem> d_ticks_;              // with times_: lane 0's clock in the inflate kernel's walk | placement | whole, per image
    double ticks_[3] = {};
    int ticks_n_ = 0;
};

}  // namespace ire
