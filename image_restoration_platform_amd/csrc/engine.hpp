// engine.hpp -- the per-GPU engine object behind the C ABI (include/ire.h).
//
// One engine = one process = one MI355X.  It owns: the classifier tables, the RestoreNet-v0
// weights re-laid-out for conv_mfma.hip, per-"lane" activation workspaces (a lane = one HIP
// stream restoring a contiguous slice of the batch, so several images are in flight and the
// per-image working set of the full-resolution levels stays inside the 256 MiB Infinity Cache),
// staging buffers for the host-pointer entry points, the pad and fusion staging of any-size jobs,
// and an event-based per-kernel profiler.  The codecs in front of and behind the network (JPEG
// uploads in, PNG / JPEG text out) are objects of their own (codec.hpp): the engine holds one of
// each, hands them out, and only asks the encoder for the batcher's results as text.
#pragma once
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "classifier.hpp"
#include "codec.hpp"
#include "common.hpp"
#include "conv_mfma.hpp"
#include "conv_plan.hpp"
#include "device_buf.hpp"
#include "icc.hpp"

namespace ire {

struct PackedConv;   // weight_pack.hpp: the host side of ConvW
struct ConvW {
    ConvDesc desc;               // kind, channel counts and which of the arrays below exist (weight_pack.hpp::conv_desc)
    unsigned short* d_w = nullptr;
    unsigned short* d_wp = nullptr;   // slabs with permuted cout rows for conv_rb.hip's direct epilogue
    unsigned short* d_w4 = nullptr;  // second arrangement for conv_w4.hip (C >= 128 ResBlock convs): 16-channel stages, 128-cout blocks
    unsigned short* d_w4h = nullptr; // the same in 64-cout blocks: launches whose 128-cout items number fewer than the CUs (small batches, 512^2 at level 3)
    unsigned short* d_wstem = nullptr;  // CONV_STEM as MFMA A fragments (conv_stem.hip): [ky 3][h 2][32 permuted rows][8], k = 16 ky + 4 kx + c (kx = 3, c = 3: zero)
    unsigned short* d_wd = nullptr;  // CONV_DOWN by pixel phase (conv_down.hip): [nblock64][kc32][phase: 1+2+2+4 taps][tap*4 + c8][64][8]
    unsigned short* d_wu = nullptr;  // CONV_UP as a sub-pixel conv (conv_up.hip): [nblock32][kc32][parity][kk][32][8], taps pre-summed per parity
    // CONV_UP composed with the level's 1x1 `fuse` (weight_pack.hpp::pack_up_fused; conv_up.hip fused form)
    unsigned short* d_wuf = nullptr; // sub-pixel slabs of (Wf_up . Wup), layout of d_wu
    unsigned short* d_wdq = nullptr; // conv_dnq.hip (stride-2 convs with cout % 128 == 0): d_wd's taps as 128-cout slabs
    unsigned short* d_wuq = nullptr; // conv_upq.hip (cout = 128): the same composed weights as [parity][kc32][tap4][c8][128 permuted rows][8]
    unsigned short* d_wsq = nullptr; // conv_upq.hip: skip half of the fuse weights as [ks32][c8][128 permuted rows][8]
    unsigned short* d_wsk = nullptr; // skip half of the fuse weights as MFMA A fragments: [nblock32][ks = C/16][h][32 permuted rows][8]
    float* d_bias_uf = nullptr;      // Wf_up . b_up + b_f
    unsigned char* d_w8x = nullptr;  // IRE_PRECISION_FP8, K = 64 form (conv_f8.hip): [nblock128][kc32][tap][half][128][16] e4m3
    unsigned char* d_w8 = nullptr;   // IRE_PRECISION_FP8: the conv_w4 slabs as OCP e4m3, one scale per output channel
    float* d_oscale = nullptr;       // [cout] weight scale / activation scale (accumulator -> output)
    float* d_bias8 = nullptr;        // [cout] bias / oscale (the accumulators start at it)
    float* d_bias = nullptr;
};
struct GNW {
    int C = 0, level = 0;
    float* d_gamma = nullptr;
    float* d_beta = nullptr;
};
struct RBW {
    GNW gn1, gn2;
    ConvW conv1, conv2;
};
struct Net {
    bool loaded = false;
    ConvW stem, head;
    GNW head_gn;
    RBW enc[4][2], mid[2], dec[3][2];
    ConvW down[3], up[3], fuse[3];
    float* d_film_w = nullptr;
    float* d_film_b = nullptr;
    BufSet<DeviceMem> mem;            // every array the pointers above are views of
};

struct LaneBufs {                     // views into the engine's workspace (device_buf.hpp lane_workspace)
    unsigned short* buf[4][5] = {};   // [level][0..3: activations | 4: the skip tensor (levels 0..2)]
    float *stats = nullptr, *stats2 = nullptr;   // stats2: second partials array: a conv that finalizes its input's GroupNorm itself (gn_fold.hpp) reads one and writes the other
    float2* ab = nullptr;
};
struct Lane {
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
    LaneBufs v;
};

// ---- the layer schedule as a program (engine.cpp::build_program): one list of ops, executed op by op either over a whole
// batch (restore_device) or over the row strips of one image with a halo exchange after every op whose output feeds a
// 3x3 convolution and a gather of the GroupNorm partials before every OP_GN (cfg 4: engine.cpp "strips") ----
constexpr int BUF_NONE = -1;
inline int buf_id(int level, int slot) { return level * 8 + slot; }   // slot 0..3 = act[level][slot], 4 = skip[level]
struct Op {
    enum Kind { GN, CONV } kind = CONV;
    const GNW* gn = nullptr;          // GN: finalize the partials of the tensor produced last -> (A, B) per (image, channel)
    const ConvW* cw = nullptr;        // CONV
    int in0 = BUF_NONE, in1 = BUF_NONE, resid = BUF_NONE, out = BUF_NONE;
    int lin = 0, lout = 0;            // levels of in0 / out
    bool use_ab = false;              // CONV: GroupNorm+FiLM+SiLU applied while staging in0
    bool halo_out = false;            // the output is read by a 3x3 convolution: strips exchange its boundary rows
    bool stats_out = false;           // the conv writes GroupNorm partials of its output
    std::string name;                 // debug-capture name ("" = none)
};
// state shared by everything one network run touches on one stream (a lane, or all strips of a tiled image)
struct Run {
    hipStream_t stream = nullptr;
    float* stats = nullptr;           // [image][tile][8 groups][2] partials of the tensor produced last
    float2* ab = nullptr;             // [image][C] coefficients of the GroupNorm finalized last
    const float* film = nullptr;
    int stat_parts = 0;               // partials per image the last stats-producing conv wrote
    float* stats_alt = nullptr;       // where the NEXT stats-producing conv writes (ping-pong with `stats`); null: in place (strips)
    const GNW* gn_pending = nullptr;  // a GroupNorm whose finalize was deferred to its consumer (exec_op GN -> exec_conv)
    const float* gn_stats = nullptr;  // its partials and their count per image
    int gn_parts = 0;
    bool snake = false;               // whole-batch passes: consecutive convs walk their items in opposite directions (row strips: all forward)
    bool next_rev = false;            // direction of the next cursor-driven conv on this stream
};
// where one executor instance's rows live: a whole batch (halo = 0) or one row strip of one image (halo = 1)
struct Geo {
    int nimg = 1, h = 0, w = 0;       // rows / columns of THIS piece at level 0
    int halo = 0;                     // halo rows above and below in every activation buffer and in img_in
    bool has_up = false, has_down = false;
    int y0 = 0, H = 0;                // first global row of the piece and global image height (level 0)
    unsigned short* buf[4][6] = {};   // buffer starts (halo row included)
    const uint8_t* img_in = nullptr;  // u8 image rows of the piece, halo rows included
    uint8_t* img_out = nullptr;       // u8 output rows of the piece (no halo)
};

// ---- what the batched preprocess (preprocess.hip) keeps between calls ----
// the tap table of one (in_size, out_size) pair on the device: bounds [out][2] (first, count) and behind them taps [out][ksize]
struct TapTable {
    int in = 0, out = 0, ksize = 0;
    int span = 0;                     // the most input pixels the taps of 32 consecutive outputs cover (the tiled kernel's LDS rows)
    uint64_t used = 0;                // LRU stamp; 0: empty
    Buf<DeviceMem> d;
    const int32_t* bounds() const { return d.get<int32_t>(); }
    const int32_t* taps() const { return d.get<int32_t>() + 2 * (size_t)out; }
};
// One user at a time: the engine's own entry (under the engine's lock) and the batcher's upload jobs (its launcher thread, always on
// the copy-in stream) each have their own, as the JPEG decoder's two users do.
struct PreprocessScratch {
    static constexpr int kTables = 16;
    TapTable tab[kTables];
    uint64_t clock = 0;
    Buf<DeviceMem> d_mid;             // the horizontal pass's output, [n][upright h][pitch]
    Buf<DeviceMem> d_stored;          // upload jobs: the decoded stored images of a batch, [n][sh][sw][3]
    // the pair's table, built and uploaded on its first use (the host then waits for the upload on s); later uses touch no stream
    const TapTable& table(int in_size, int out_size, hipStream_t s);
};

struct ProfRec {
    int fam;
    bool own_e0 = true;   // false: e0 is the previous record's e1 (back-to-back profiled launches share the event)
    hipEvent_t e0, e1;
    double flops, bytes;
    double flops_exec = 0;   // flops the kernel really issues (the sub-pixel `up` form runs 4 of 9 taps, its composed skip term C of 2C channels)
    int group = -1;          // index into Engine::prof_groups_ (layer group "L2.rb1", "up0", ...) or -1
};
struct ProfGroup {           // per layer group: what bench.py's roofline.per_level reports
    std::string key, kernel;
    int level = 0, cin = 0, cout = 0;
    double ms = 0, flops = 0, flops_exec = 0, bytes = 0;
    int64_t n = 0;
};

class Engine {
    friend class StripSession;
public:
    explicit Engine(const ire_config& cfg);
    ~Engine();

    void load_weights(const void* blob, size_t bytes);
    void load_weights_file(const char* path);

    // host-pointer paths (synchronous)
    void classify_host(const uint8_t* rgb, int n, int h, int w, int row_stride, const uint8_t* is_jpeg,
                       double* scores, int32_t* label);
    void restore_host(const uint8_t* rgb, int n, int h, int w, const double* scores, const uint8_t* is_jpeg,
                      uint8_t* out, ire_timings* t);
    // device-pointer paths (asynchronous on stream)
    void classify_device(const uint8_t* d_rgb, int n, int h, int w, const uint8_t* d_is_jpeg, double* d_scores,
                         int32_t* d_label, hipStream_t stream);
    void restore_device(const uint8_t* d_rgb, int n, int h, int w, const double* d_scores,
                        const uint8_t* d_is_jpeg, uint8_t* d_out, hipStream_t stream);

    // fusion (fusion.hip)
    void fuse_launch(const uint8_t* d_views, int nsets, int k, int h, int w, const unsigned* host_wluts, uint8_t* d_out,
                     int32_t* d_shifts, hipStream_t s);
    double noise_of_view0(const uint8_t* d_views, int h, int w, hipStream_t s);
    // the chain with its blend tables built on the device from d_noise[i * noise_stride] (fusion_wlut_kernel): no host round trip
    void fuse_launch_device_tables(const uint8_t* d_views, int nsets, int k, int h, int w, const double* d_noise, int noise_stride, uint8_t* d_out,
                                   int32_t* d_shifts, hipStream_t s);
    void debug_fusion_wlut(const double* noise, int n, uint32_t* out);
    // Fusion jobs (k = 2..3 views of one size, h, w in 1..8192), nsets sets laid out [nsets][k][h][w][3]: every view restored as
    // restore_fit_device_mixed restores it, its h x w window edge-replicated to HF x WF = fuse_dim(h) x fuse_dim(w), the sets fused with
    // the noise score of view 0 of the PADDED set (what noise_score < 0 means to ire_fuse), the fused image cropped to h x w.
    // d_txt == null: d_out receives the nsets*h*w*3 fused pixels; else the results leave as text, encoded where the fused padded
    // image lies (txt_stride apart, as restore_fit_device_mixed lays them out).  nsets <= kFuseMaxSets, nsets*k <= max_batch.
    // The view's scores are in scores_device() afterwards, [nsets*k][7].  Nothing in it waits for the stream.
    void restore_fuse_fit_device_mixed(const uint8_t* d_views, int nsets, int k, int h, int w, const double* host_scores, const uint8_t* has_scores,
                                       const uint8_t* d_is_jpeg, uint8_t* d_out, uint8_t* d_txt, size_t txt_stride, hipStream_t stream);
    // the same for a caller on the device: d_scores [nsets*k][7] for every view, or null: classified inside
    void restore_fuse_fit_device(const uint8_t* d_views, int nsets, int k, int h, int w, const double* d_scores, const uint8_t* d_is_jpeg, uint8_t* d_out,
                                 hipStream_t stream);
    static int fuse_dim(int v) { return v <= 64 ? 64 : (v + 7) / 8 * 8; }
    void fuse_host_impl(const uint8_t* rgb_views, int k, int h, int w, double noise_score, uint8_t* out_rgb,
                        int32_t* shifts_out, ire_timings* t);

    // preprocess step in front of the path (preprocess.hip): EXIF orientation + fit-inside Lanczos-3
    void preprocess_device(const uint8_t* d_rgb, int h, int w, int orientation, int max_dim, uint8_t* d_out, int out_h, int out_w,
                           hipStream_t s);
    void preprocess_host(const uint8_t* rgb, int h, int w, int orientation, int max_dim, uint8_t* out, int out_h, int out_w);
    // n <= max_batch images of ONE stored size and orientation, image_pitch apart -> n upright fitted images out_pitch apart: image i
    // is byte for byte preprocess_device's.  Two launches whatever n; no host wait once both tap tables are cached.  P: whose scratch.
    void preprocess_batch_device(PreprocessScratch& P, const uint8_t* d_rgb, int n, int h, int w, size_t image_pitch, int orientation, int max_dim, uint8_t* d_out,
                                 int out_h, int out_w, size_t out_pitch, hipStream_t s);
    PreprocessScratch& preprocess_own() { return pp_own_; }         // the engine's own entries
    PreprocessScratch& preprocess_uploads() { return pp_uploads_; } // the batcher's upload jobs
    // Any-size jobs (h, w in 1..8192): edge-replicate pad to (max(16, ceil8 h), max(16, ceil8 w)) into the engine's padded
    // staging, the network on the padded shape, the top-left h x w window as the result.  The classifier always sees the
    // ORIGINAL pixels.  A shape restore_device takes as it is skips the pad and runs exactly as restore_device does.
    void restore_fit_device(const uint8_t* d_rgb, int n, int h, int w, const double* d_scores, const uint8_t* d_is_jpeg, uint8_t* d_out,
                            hipStream_t stream);
    void restore_fit_host(const uint8_t* rgb, int n, int h, int w, const double* scores, const uint8_t* is_jpeg, uint8_t* out, ire_timings* t);
    // batcher form (restore_device_mixed for any size).  d_txt == null: d_out receives the n*h*w*3 result pixels.  d_txt != null:
    // the results leave as text (png_base64_chars(h, w) characters each, txt_stride apart; with IRE_FLAG_RESULT_PNG_DEFLATE / IRE_FLAG_RESULT_JPEG a uint64
    // character count and then the characters), encoded where the network left them; d_out is then working space of n*h*w*3 bytes.
    void restore_fit_device_mixed(const uint8_t* d_rgb, int n, int h, int w, const double* host_scores, const uint8_t* has_scores,
                                  const uint8_t* d_is_jpeg, uint8_t* d_out, uint8_t* d_txt, size_t txt_stride, hipStream_t stream);
    static bool fit_is_aligned(int h, int w) { return h % 8 == 0 && w % 8 == 0 && h >= 16 && w >= 16; }
    static int fit_dim(int v) { return v <= 16 ? 16 : (v + 7) / 8 * 8; }
    // the codecs (codec.hpp): used inside the same enter / leave bracket as every other call
    TextEncoder& text_encoder() { return enc_; }
    JpegDecoder& jpeg_decoder() { return dec_; }
    PngDecoder& png_decoder() { return pdec_; }             // IRE_FLAG_DECODE_PNG; without the flag it refuses every call
    IccConverter& icc_converter() { return icc_; }          // icc.hpp: ICC-tagged pixels to sRGB
    bool upload_icc() const { return upload_icc_; }         // IRE_FLAG_UPLOAD_ICC: upload jobs honour their file's ICC profile
    const TextFormat* result_format() const { return result_format_; }      // of the batcher's results, with this engine's settings; null: pixels

    void debug_sums(int n, uint64_t* out);
    uint64_t debug_poison_scratch(int byte);      // -> bytes filled
    void debug_gn_finalize(const float* stats, int nimg, int parts, int C, int hw, const float* gamma, const float* beta, const float* film,
                           int film_stride, int film_off, float* ab_out);
    void debug_capture(bool on) { capture_ = on; captured_.clear(); }
    bool debug_activation(const std::string& name, float* out, size_t* count);

    void profile_enable(int mode);   // low byte: 0 off, 1 every kernel family, 2 the 3x3 conv family only; bits 8..: N = time every N-th network pass (mode 2)
    void profile_reset();
    void profile_query(int fam, double* ms, int64_t* launches, double* flops, double* bytes);
    std::string profile_report();    // JSON array, one object per layer group (ire_profile_report)

    int max_batch() const { return max_batch_; }
    // Cross-stream serialisation of the shared GPU scratch (activation workspaces, d_scores_, d_film_, fusion and
    // preprocess scratch): every ABI call brackets its enqueue with enter/leave under the engine mutex.  enter makes the
    // caller's stream wait for the completion event of the previous call (a no-op on the same stream), leave records
    // the new one -- so two threads on two streams interleave whole calls on the GPU, never kernels of two calls.
    void enter(hipStream_t s);
    void leave(hipStream_t s);
    // device bytes one more image of this shape costs (activation workspace + staging), and how many fit right now
    size_t bytes_per_image(int h, int w) const { return workspace_bytes_per_image(h, w); }
    int capacity_for(int h, int w) const;
    // cfg 4: the whole image on this GPU as nstrips "virtual ranks" (strips.cpp); d_scores null => classify inside
    void restore_tiled_device(const uint8_t* d_rgb, int h, int w, int nstrips, const double* d_scores, const uint8_t* d_is_jpeg,
                              uint8_t* d_out, hipStream_t stream);
    void get_stats(ire_engine_stats* out);                            // counters + the images/sec gauge (queue_depth is the ABI layer's)
    // batcher form of restore_device: rows of host_scores (pinned, n*7) flagged in has_scores are used as given, the rest are
    // classified inside (one scan over the batch, skipped when every job brought its scores)
    void restore_device_mixed(const uint8_t* d_rgb, int n, int h, int w, const double* host_scores, const uint8_t* has_scores,
                              const uint8_t* d_is_jpeg, uint8_t* d_out, hipStream_t stream);
    hipStream_t main_stream() const { return main_stream_; }          // the stream of the host entry points and of the batcher's compute
    const double* scores_device() const { return io_.scores; }       // [last n][7], valid after a classify on main_stream()
    std::mutex& mutex() { return mu_; }

private:
    void check_shape(int n, int h, int w, bool for_restore) const;
    void check_fit(int n, int h, int w) const;
    void ensure_pad(int n, int H, int W);      // d_pad_in_ / d_pad_out_, grow-only
    void ensure_fuse_io(int nsets, int k, int HF, int WF, hipStream_t s);      // d_fuse_in_ / d_fuse_out_ / d_fuse_sc_ and the fusion scratch, grow-only
    void check_fuse_fit(int nsets, int k, int h, int w) const;
    void fuse_fit_core(const uint8_t* d_views, int nsets, int k, int h, int w, const double* d_sc, const uint8_t* d_is_jpeg, uint8_t* d_out, uint8_t* d_txt,
                       size_t txt_stride, hipStream_t stream);
    void fuse_reserve(int nsets, size_t px, hipStream_t s);
    void fuse_chain(const uint8_t* d_views, int nsets, int k, int h, int w, const unsigned* host_wluts, uint8_t* d_out, int32_t* d_shifts, hipStream_t s);
    // the scores a batch of jobs runs with: rows flagged in has_scores as given (pinned, n*7), the rest classified; null: restore_device classifies inside
    const double* settle_scores(const uint8_t* d_rgb, int n, int h, int w, const double* host_scores, const uint8_t* has_scores, const uint8_t* d_is_jpeg, hipStream_t stream);
    // d_scores, or for an unaligned shape without them the classifier's of the ORIGINAL pixels (never of the padded copy)
    const double* scores_of_original(const uint8_t* d_rgb, int n, int h, int w, const double* d_scores, const uint8_t* d_is_jpeg, hipStream_t stream);
    double note_restored(int n);               // counters + the 10 s window of the images/sec gauge (n = 0: only prunes it); -> now
    void restore_padded(const uint8_t* d_rgb, int n, int h, int w, const double* d_scores, const uint8_t* d_is_jpeg, hipStream_t stream);
    void restore_host_impl(const uint8_t* rgb, int n, int h, int w, const double* scores, const uint8_t* is_jpeg, uint8_t* out, ire_timings* t);
    void encode_result(const uint8_t* d_rgb, int n, int h, int w, size_t row_pitch, size_t image_pitch, uint8_t* d_txt, size_t txt_stride, hipStream_t s);
    void ensure_io(int n, int h, int w);
    void ensure_workspace(int n, int h, int w);
    void free_workspace();
    void build_program();
    void run_network(Lane& L, int nimg, int h, int w, const uint8_t* d_in, uint8_t* d_out, const float* d_film);
    void exec_op(Run& R, const Op& op, const Geo& g);
    void flush_gn(Run& R, const Geo& g);       // launch the deferred finalize as its own kernel (consumers without the folded prologue)
    void exec_conv(Run& R, const Op& op, const Geo& g);
    static Geo geo_of_lane(const Lane& L, int nimg, int h, int w, const uint8_t* d_in, uint8_t* d_out);
    void prof_begin(int fam, hipStream_t s, double flops, double bytes);
    void prof_tag(const char* key, const char* kernel, int level, int cin, int cout, double flops_exec);   // after prof_begin: the open record's layer group
    void prof_end(hipStream_t s);
    void capture(const char* name, const unsigned short* d, size_t count, hipStream_t s);
    void capture_rows(const char* name, const unsigned short* d, size_t count, size_t total, size_t offset, hipStream_t s);   // a strip's rows into the whole image's entry
    void capture_f32(const char* name, const float* d, size_t count, hipStream_t s);
    template <class T> T* upload(const std::vector<T>& v);     // allocate in net_.mem + copy; null for an empty v
    ConvW upload_conv(const PackedConv& p);                    // weight_pack.hpp's arrays of one convolution -> device

    int device_ = 0;
    int max_batch_ = 8;
    int num_lanes_ = 1;
    const TextFormat* result_format_ = nullptr;
    TextFormat jpeg_format_ = kJpeg;      // kJpeg at ire_config's jpeg_quality and jpeg_sampling: what result_format_ points to on a JPEG engine
    int precision_ = IRE_PRECISION_BF16;
    ConvSwitches sw_;             // the A/B schedule switches, read from the environment once (conv_plan.hpp)
    int cus_ = 256;               // persistent_grid_cus(), read once
    bool snake_ = true;           // IRE_SNAKE (A/B switch, read once): 0 = every conv launch walks its items forward
    std::mutex mu_;
    hipStream_t main_stream_ = nullptr;
    hipEvent_t ev_[4] = {};
    hipEvent_t fork_ev_ = nullptr;
    hipEvent_t busy_ev_ = nullptr;   // completion of the last enqueued call (enter/leave)
    bool busy_recorded_ = false;
    int64_t batches_run_ = 0, images_restored_ = 0;
    int last_batch_ = 0;
    std::deque<std::pair<double, int>> recent_;      // (seconds since init, images) of the last 10 s of restore calls
    double t0_ = 0.0;

    // classifier
    // Every device buffer below is owned through device_buf.hpp: freed with the engine (members die after ~Engine's body: behind its
    // hipDeviceSynchronize, the device still current), grow-only per shape, and empty after a failed grow.
    ClassifierTables tables_{};
    BufSet<DeviceMem> tables_mem_;

    IoBufs<DeviceMem> io_;                // io / classifier buffers (sized by ensure_io)
    int last_n_ = 0;
    FuseBufs<DeviceMem> fuse_;            // fusion scratch
    Buf<DeviceMem> d_zero_{BufUse::Persistent};             // 256 bytes of zeros (conv_upq.hip's zero padding source)
    Buf<DeviceMem> d_pp_tab_, d_pp_mid_, d_pp_in_, d_pp_out_;   // preprocess scratch (tap tables, intermediate of the horizontal pass, host-path staging)
    PreprocessScratch pp_own_, pp_uploads_;
    Buf<DeviceMem> d_pad_in_, d_pad_out_; // any-size jobs: the edge-padded batch in front of the network, and the network's output on the padded shape
    Buf<DeviceMem> d_fuse_in_, d_fuse_out_;   // fusion jobs: the restored windows padded to the fusion shape [n][HF][WF][3], the fused images [sets][HF][WF][3]
    Buf<DeviceMem> d_fuse_sc_;            // ... and the classifier's scores of view 0 of every padded set, [kFuseMaxSets][7] (never io_.scores: those are the jobs')
    TextEncoder enc_;                     // codec.hpp: they own their buffers
    JpegDecoder dec_;
    PngDecoder pdec_;
    IccConverter icc_;
    bool upload_icc_ = false;

    // network
    Net net_;
    std::vector<Op> program_;             // the layer schedule (build_program; rebuilt by load_weights)
    std::unique_ptr<class StripSession> tiled_;   // cached session of restore_tiled_device (one shape at a time)
    int tiled_h_ = 0, tiled_w_ = 0, tiled_n_ = 0;
    std::vector<Lane> lanes_;
    int ws_imgs_cap_ = 0, ws_h_ = 0, ws_w_ = 0;
    BufSet<DeviceMem> ws_;                // what the lanes' LaneBufs point into

    // debug / profile
    // diagnostic stamps (IRE_RB_STAMPS selects the launches; dumped by ~Engine as the workgroup timeline IRE_W4_TL or raw, IRE_STAMPS_RAW)
    Buf<DeviceMem> stamps_dev_{BufUse::Persistent};
    int stamps_cout_ = 0;
    bool stamps_resid_ = false;
    std::string stamps_tl_;
    bool capture_ = false;
    std::map<std::string, std::vector<float>> captured_;
    int prof_on_ = 0;
    int prof_every_ = 1, prof_pass_ = 0;   // mode 2: time every prof_every_-th pass of the network
    bool prof_skip_ = false;
    bool prof_open_ = false;
    bool prof_chain_ = false;          // the stream's last operation is prof_.back()'s end event (prof_chain_stream_): the next record starts there
    hipStream_t prof_chain_stream_ = nullptr;
    bool prof_chainable_ = false;      // true while run_network walks the op list (the only place records may share events)
    std::vector<ProfRec> prof_;
    std::vector<hipEvent_t> ev_pool_;
    double prof_ms_[FAM_COUNT] = {}, prof_flops_[FAM_COUNT] = {}, prof_bytes_[FAM_COUNT] = {};
    int64_t prof_n_[FAM_COUNT] = {};
    double prof_flops_exec_[FAM_COUNT] = {};
    std::vector<ProfGroup> prof_groups_;
    void prof_collect();
};

void preprocess_plan(int width, int height, int orientation, int max_dim, int* out_w, int* out_h, int* resized);

}  // namespace ire
