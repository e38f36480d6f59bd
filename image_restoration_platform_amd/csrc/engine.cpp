// engine.cpp -- engine object: weights, workspaces, layer schedule, lanes, profiler.
// See engine.hpp for the design; the layer schedule follows DESIGN.md "RestoreNet-v0"
// (SURVEY.md Appendix C), which stands behind GeminiClient.restoreImage
// (server-node/src/clients/geminiClient.js:32-97).
#include "engine.hpp"
#include "encode.hpp"
#include "fusion.hpp"

#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>

#include "gn.hpp"
#include "strips.hpp"
#include "weight_pack.hpp"
#include "grey_tables.inc"

namespace ire {

namespace {

inline double now_s() {
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

}  // namespace

Engine::Engine(const ire_config& cfg) {
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        fail(IRE_ERR_UNAVAILABLE, "service unavailable: no HIP device visible (the engine has no CPU fallback)");
    device_ = cfg.device_index;
    if (device_ < 0 || device_ >= ndev) fail(IRE_ERR_INVALID_INPUT, "invalid device_index");
    IRE_HIP(hipSetDevice(device_));
    hipDeviceProp_t prop;
    IRE_HIP(hipGetDeviceProperties(&prop, device_));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        fail(IRE_ERR_UNAVAILABLE, std::string("service unavailable: device is ") + prop.gcnArchName +
                                      ", this engine is built for gfx950 (MI355X) only");
    if (cfg.precision != IRE_PRECISION_BF16 && cfg.precision != IRE_PRECISION_FP8) fail(IRE_ERR_INVALID_INPUT, "invalid precision");
    precision_ = cfg.precision;
    max_batch_ = cfg.max_batch > 0 ? cfg.max_batch : 8;
    if (max_batch_ > 64) fail(IRE_ERR_INVALID_INPUT, "invalid max_batch (1..64)");
    num_lanes_ = cfg.num_streams > 0 ? cfg.num_streams : 1;
    if (num_lanes_ > 16) num_lanes_ = 16;
    check_config_flags(cfg.flags);
    result_format_ = result_format_of(cfg.flags);
    jpeg_format_ = jpeg_format_of(check_config_jpeg(cfg.flags, cfg.jpeg_quality, cfg.jpeg_sampling));
    if (result_format_ == &kJpeg) result_format_ = &jpeg_format_;
    sw_ = ConvSwitches::from_env();
    cus_ = persistent_grid_cus();
    if (const char* v = std::getenv("IRE_SNAKE")) snake_ = std::atoi(v) != 0;
    if (const char* v = std::getenv("IRE_RB_STAMPS")) {   // diagnostic: "<cout>[r]" = stamp the first such ResBlock conv
        stamps_cout_ = std::atoi(v);
        stamps_resid_ = std::strchr(v, 'r') != nullptr;
    }
    if (const char* v = std::getenv("IRE_W4_TL")) stamps_tl_ = v;     // diagnostic (-DIRE_W4_TL builds): CSV path of the workgroup timeline of the LAST stamped launch

    IRE_HIP(hipStreamCreateWithFlags(&main_stream_, hipStreamNonBlocking));
    enc_.setup(max_batch_, main_stream_);
    dec_.setup(max_batch_, (cfg.flags & IRE_FLAG_DECODE_PROGRESSIVE) ? jpegparse::kAcceptProgressive : 0u, main_stream_);
    pdec_.setup(max_batch_, (cfg.flags & IRE_FLAG_DECODE_PNG) != 0, (cfg.flags & IRE_FLAG_DECODE_PNG_ALL) != 0, main_stream_);
    icc_.setup(max_batch_);
    upload_icc_ = (cfg.flags & IRE_FLAG_UPLOAD_ICC) != 0;
    for (auto& ev : ev_) IRE_HIP(hipEventCreate(&ev));
    IRE_HIP(hipEventCreateWithFlags(&fork_ev_, hipEventDisableTiming));
    IRE_HIP(hipEventCreateWithFlags(&busy_ev_, hipEventDisableTiming));
    lanes_.resize(num_lanes_);
    for (auto& L : lanes_) {
        IRE_HIP(hipStreamCreateWithFlags(&L.stream, hipStreamNonBlocking));
        IRE_HIP(hipEventCreateWithFlags(&L.done, hipEventDisableTiming));
    }

    // classifier tables
    unsigned int* d_lin = tables_mem_.alloc<unsigned int>(sizeof(kLin16), BufUse::Persistent);
    unsigned int* d_thr = tables_mem_.alloc<unsigned int>(sizeof(kGreyThr), BufUse::Persistent);
    unsigned char* d_inv = tables_mem_.alloc<unsigned char>(5008, BufUse::Persistent);          // 5001 buckets, padded to whole 16-byte chunks (classifier.hip loads it as uint4)
    IRE_HIP(hipMemset(d_inv, 0, 5008));
    IRE_HIP(hipMemcpy(d_lin, kLin16, sizeof(kLin16), hipMemcpyHostToDevice));
    IRE_HIP(hipMemcpy(d_thr, kGreyThr, sizeof(kGreyThr), hipMemcpyHostToDevice));
    IRE_HIP(hipMemcpy(d_inv, kGreyInv, sizeof(kGreyInv), hipMemcpyHostToDevice));
    tables_ = ClassifierTables{d_lin, d_thr, d_inv};
    if (stamps_cout_ && (!stamps_tl_.empty() || std::getenv("IRE_STAMPS_RAW"))) {      // somebody will dump them
        stamps_dev_.grow(8 * 2 * 64 * 10 * 8);
        IRE_HIP(hipMemset(stamps_dev_.get<void>(), 0, 8 * 2 * 64 * 10 * 8));
    }

    if (cfg.weights_path && cfg.weights_path[0]) load_weights_file(cfg.weights_path);
}

Engine::~Engine() {
    (void)hipSetDevice(device_);
    (void)hipDeviceSynchronize();
    dec_.report_times();
    if (stamps_dev_ && std::getenv("IRE_STAMPS_RAW")) {     // diagnostic builds with their own stamp layout (conv_pk.hip PK_TICKS): the whole buffer, one value per line
        std::vector<unsigned long long> h(8 * 2 * 64 * 10);
        (void)hipMemcpy(h.data(), stamps_dev_.get<void>(), h.size() * 8, hipMemcpyDeviceToHost);
        if (FILE* f = std::fopen(std::getenv("IRE_STAMPS_RAW"), "w")) {
            for (size_t i = 0; i < h.size(); ++i) std::fprintf(f, "%llu\n", h[i]);
            std::fclose(f);
        }
        stamps_dev_.reset();
    }
    if (stamps_dev_ && !stamps_tl_.empty()) {       // workgroup timeline (conv_w4.hip `tl`): raw stamps, one row per workgroup and slot
        std::vector<unsigned long long> h(8 * 2 * 64 * 10);
        (void)hipMemcpy(h.data(), stamps_dev_.get<void>(), h.size() * 8, hipMemcpyDeviceToHost);
        if (FILE* f = std::fopen(stamps_tl_.c_str(), "w")) {
            std::fprintf(f, "wg,slot,realtime_10ns,memtime\n");
            for (int wg = 0; wg < 256; ++wg)
                for (int sl = 0; sl < 16; ++sl)
                    if (h[(size_t)wg * 32 + sl * 2] || h[(size_t)wg * 32 + sl * 2 + 1]) std::fprintf(f, "%d,%d,%llu,%llu\n", wg, sl, h[(size_t)wg * 32 + sl * 2], h[(size_t)wg * 32 + sl * 2 + 1]);
            std::fclose(f);
        }
        stamps_dev_.reset();
    }
    for (auto& L : lanes_) {
        if (L.stream) (void)hipStreamDestroy(L.stream);
        if (L.done) (void)hipEventDestroy(L.done);
    }
    for (auto& ev : ev_) if (ev) (void)hipEventDestroy(ev);
    if (fork_ev_) (void)hipEventDestroy(fork_ev_);
    if (busy_ev_) (void)hipEventDestroy(busy_ev_);
    for (auto& r : prof_) { if (r.own_e0) (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
    for (auto ev : ev_pool_) (void)hipEventDestroy(ev);
    if (main_stream_) (void)hipStreamDestroy(main_stream_);
}

// ------------------------------------------------------------------------------------------------
// weights
// ------------------------------------------------------------------------------------------------
void Engine::load_weights_file(const char* path) {
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) fail(IRE_ERR_INVALID_INPUT, std::string("invalid weights_path: cannot open ") + path);
    std::streamsize sz = f.tellg();
    f.seekg(0);
    std::vector<char> blob((size_t)sz);
    if (!f.read(blob.data(), sz)) fail(IRE_ERR_INVALID_INPUT, std::string("invalid weights_path: short read ") + path);
    load_weights(blob.data(), blob.size());
}

// one packed array -> device (null for an array the packer did not produce: conv_plan.hpp picks kernels by that)
template <class T>
T* Engine::upload(const std::vector<T>& v) {
    if (v.empty()) return nullptr;
    T* d = net_.mem.alloc<T>(v.size() * sizeof(T), BufUse::Persistent);
    IRE_HIP(hipMemcpy(d, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return d;
}

ConvW Engine::upload_conv(const PackedConv& p) {
    ConvW c;
    c.desc = conv_desc(p);
    c.d_w = upload(p.w); c.d_wp = upload(p.wp); c.d_w4 = upload(p.w4); c.d_w4h = upload(p.w4h); c.d_wstem = upload(p.wstem);
    c.d_wd = upload(p.wd); c.d_wu = upload(p.wu); c.d_wuf = upload(p.wuf); c.d_wdq = upload(p.wdq); c.d_wuq = upload(p.wuq);
    c.d_wsq = upload(p.wsq); c.d_wsk = upload(p.wsk); c.d_bias_uf = upload(p.bias_uf); c.d_w8x = upload(p.w8x); c.d_w8 = upload(p.w8);
    c.d_oscale = upload(p.oscale); c.d_bias8 = upload(p.bias8); c.d_bias = upload(p.bias);
    return c;
}

// the weights in weight_pack.hpp's layouts, layer by layer in the order of the schedule
void Engine::load_weights(const void* blob, size_t bytes) {
    const TensorMap tm = parse_weights(blob, bytes);
    IRE_HIP(hipSetDevice(device_));
    IRE_HIP(hipDeviceSynchronize());
    tiled_.reset();
    net_ = Net{};
    if (d_zero_.grow(256)) IRE_HIP(hipMemset(d_zero_.get<void>(), 0, 256));
    const bool fp8 = precision_ == IRE_PRECISION_FP8;
    auto vec = [&](const std::string& nm, size_t n, const std::string& what) -> const std::vector<float>& {
        auto it = tm.find(nm);
        if (it == tm.end() || it->second.data.size() != n) fail(IRE_ERR_INVALID_INPUT, "invalid weight file: " + what);
        return it->second.data;
    };
    auto conv = [&](ConvKind kind, const std::string& nm, int cin, int cout) { return upload_conv(pack_conv(tm, kind, nm + ".w", nm + ".b", cin, cout, fp8)); };
    auto gn = [&](const std::string& nm, int C, int level) {
        GNW g;
        g.C = C; g.level = level;
        g.d_gamma = upload(vec(nm + ".g", C, "missing " + nm + ".g"));
        g.d_beta = upload(vec(nm + ".b", C, "missing " + nm + ".b"));
        return g;
    };
    auto rb = [&](const std::string& p, int C, int level) {
        RBW r;
        r.gn1 = gn(p + ".gn1", C, level);
        r.conv1 = conv(CONV_RB1, p + ".conv1", C, C);
        r.gn2 = gn(p + ".gn2", C, level);
        r.conv2 = conv(CONV_RB2, p + ".conv2", C, C);
        return r;
    };
    net_.stem = conv(CONV_STEM, "stem", 3, 32);
    for (int l = 0; l < 4; ++l) {
        const std::string s = std::to_string(l);
        for (int i = 0; i < 2; ++i) net_.enc[l][i] = rb("enc" + s + ".rb" + std::to_string(i), kWidths[l], l);
        if (l < 3) net_.down[l] = conv(CONV_DOWN, "down" + s, kWidths[l], kWidths[l + 1]);
    }
    for (int i = 0; i < 2; ++i) net_.mid[i] = rb("mid.rb" + std::to_string(i), 256, 3);
    for (int l = 2; l >= 0; --l) {
        const std::string s = std::to_string(l);
        PackedConv up = pack_conv(tm, CONV_UP, "up" + s + ".w", "up" + s + ".b", kWidths[l + 1], kWidths[l], fp8);
        pack_up_fused(tm, up, s);
        net_.up[l] = upload_conv(up);
        net_.fuse[l] = conv(CONV_FUSE, "fuse" + s, 2 * kWidths[l], kWidths[l]);
        for (int i = 0; i < 2; ++i) net_.dec[l][i] = rb("dec" + s + ".rb" + std::to_string(i), kWidths[l], l);
    }
    net_.head_gn = gn("head.gn", 32, 0);
    net_.head = conv(CONV_HEAD, "head", 32, 3);
    net_.d_film_w = upload(vec("film.w", (size_t)kFilmDim * 7, "film"));
    net_.d_film_b = upload(vec("film.b", kFilmDim, "film"));
    net_.loaded = true;
    build_program();
}

// ------------------------------------------------------------------------------------------------
// buffers
// ------------------------------------------------------------------------------------------------
void Engine::check_shape(int n, int h, int w, bool for_restore) const {
    if (n <= 0 || n > max_batch_) fail(IRE_ERR_INVALID_INPUT, "invalid batch size n (1..max_batch)");
    if (h <= 0 || w <= 0 || h > 8192 || w > 8192) fail(IRE_ERR_INVALID_INPUT, "invalid image size");
    if (for_restore && (h % 8 || w % 8 || h < 16 || w < 16))
        fail(IRE_ERR_INVALID_INPUT, "invalid image size for restore: height and width must be multiples of 8, >= 16");
    if (for_restore && !piece_addressable(h, w, 0)) fail(IRE_ERR_INVALID_INPUT, not_addressable(h, w));
}

void Engine::ensure_io(int n, int h, int w) {
    IRE_HIP(hipSetDevice(device_));
    const size_t px = (size_t)h * w;
    if ((size_t)n <= io_.cap_imgs && px <= io_.cap_px) return;
    IRE_HIP(hipDeviceSynchronize());
    // in images: a whole batch of the shape or what was asked for (batch_room), and never less than before on either axis
    const size_t want = batch_room(px * 3 * (size_t)n, px * 3 * (size_t)max_batch_) / (px * 3);
    io_.regrow(std::max({io_.cap_imgs, want, (size_t)n}), std::max(io_.cap_px, px), cls_sums_bytes());
    IRE_HIP(hipMemset(io_.sums, 0, cls_sums_bytes()));
}

void Engine::enter(hipStream_t s) {
    IRE_HIP(hipSetDevice(device_));
    if (busy_recorded_) IRE_HIP(hipStreamWaitEvent(s, busy_ev_, 0));
}
void Engine::leave(hipStream_t s) {
    if (hipEventRecord(busy_ev_, s) == hipSuccess) busy_recorded_ = true;
}

void Engine::check_fit(int n, int h, int w) const {
    if (n <= 0 || n > max_batch_) fail(IRE_ERR_INVALID_INPUT, "invalid batch size n (1..max_batch)");
    if (h < 1 || w < 1 || h > 8192 || w > 8192) fail(IRE_ERR_INVALID_INPUT, "invalid image size: height and width must be in 1..8192");
    if (!piece_addressable(fit_dim(h), fit_dim(w), 0)) fail(IRE_ERR_INVALID_INPUT, not_addressable(fit_dim(h), fit_dim(w)));      // the padded image is what runs
}

void Engine::ensure_pad(int n, int H, int W) {
    const size_t per = (size_t)H * W * 3, need = per * (size_t)n;
    if (need <= d_pad_out_.bytes()) return;      // (the pair has one size, and d_pad_out_ is the one allocated last)
    IRE_HIP(hipSetDevice(device_));
    IRE_HIP(hipDeviceSynchronize());
    d_pad_in_.reset(); d_pad_out_.reset();      // both go before either comes back
    const size_t want = batch_room(need, per * (size_t)max_batch_);
    d_pad_in_.grow(need, want);
    d_pad_out_.grow(need, want);
}

void Engine::free_workspace() {
    ws_.clear();
    for (Lane& L : lanes_) L.v = LaneBufs{};
    ws_imgs_cap_ = ws_h_ = ws_w_ = 0;
}

int Engine::capacity_for(int h, int w) const {
    if (h <= 0 || w <= 0 || h > 8192 || w > 8192 || h % 8 || w % 8 || h < 16 || w < 16) return 0;
    if (!piece_addressable(h, w, 0)) return 0;       // the shape restore refuses (8192 x 8192: conv_plan.hpp)
    size_t free_b = 0, total_b = 0;
    if (hipSetDevice(device_) != hipSuccess || hipMemGetInfo(&free_b, &total_b) != hipSuccess) return 0;
    // what this engine already holds for activations would be released on a change of shape
    const double avail = 0.92 * ((double)free_b + (double)ws_.bytes());
    const double n = avail / (double)bytes_per_image(h, w);
    return n >= (double)max_batch_ ? max_batch_ : (int)n;
}

void Engine::ensure_workspace(int n, int h, int w) {
    // sized by the batch actually asked for (grow-only per shape), not by max_batch: one 8192^2 image must not need 64 slots
    if (h == ws_h_ && w == ws_w_ && n <= ws_imgs_cap_) return;
    const int cap = (h == ws_h_ && w == ws_w_) ? std::max(n, ws_imgs_cap_) : n;
    const int per = ceil_div(cap, num_lanes_);
    IRE_HIP(hipDeviceSynchronize());
    free_workspace();
    // Memory and views are committed together: a throw half way frees `mem` (a partial allocation must not pin HBM: the caller gets
    // "service unavailable" and may retry smaller) and leaves the engine with the empty workspace free_workspace made.
    const std::vector<WsEntry> table = lane_workspace(per, h, w);
    BufSet<DeviceMem> mem;
    std::vector<LaneBufs> views(lanes_.size());
    for (LaneBufs& v : views)
        for (const WsEntry& e : table) {
            void* p = mem.alloc<void>(e.bytes);
            if (e.slot == WS_STATS) v.stats = (float*)p;
            else if (e.slot == WS_STATS2) v.stats2 = (float*)p;
            else if (e.slot == WS_AB) v.ab = (float2*)p;
            else v.buf[e.slot >> 3][e.slot & 7] = (unsigned short*)p;
        }
    ws_ = std::move(mem);
    for (size_t i = 0; i < views.size(); ++i) lanes_[i].v = views[i];
    ws_imgs_cap_ = per * num_lanes_; ws_h_ = h; ws_w_ = w;
}

// ------------------------------------------------------------------------------------------------
// profiler (HIP events on the stream the kernel is launched on)
// ------------------------------------------------------------------------------------------------
void Engine::prof_begin(int fam, hipStream_t s, double flops, double bytes) {
    prof_open_ = prof_on_ == 1 || (prof_on_ == 2 && fam == FAM_CONV3 && !prof_skip_);   // mode 2: dominant family only (fewer events), every prof_every_-th network pass
    if (!prof_open_) { prof_chain_ = false; return; }
    ProfRec r;
    r.fam = fam; r.flops = flops; r.bytes = bytes; r.flops_exec = flops;
    auto get = [&]() {
        hipEvent_t ev;
        if (!ev_pool_.empty()) { ev = ev_pool_.back(); ev_pool_.pop_back(); }
        else IRE_HIP(hipEventCreate(&ev));
        return ev;
    };
    // An event record is a packet of its own on the stream (~4 us between two kernels).  When the previous profiled launch's
    // end event is the stream's last operation, this launch starts its interval there: one event per boundary instead of two.
    if (prof_chainable_ && prof_chain_ && prof_chain_stream_ == s && !prof_.empty()) { r.e0 = prof_.back().e1; r.own_e0 = false; }
    else { r.e0 = get(); IRE_HIP(hipEventRecord(r.e0, s)); }
    r.e1 = get();
    prof_.push_back(r);
}
void Engine::prof_tag(const char* key, const char* kernel, int level, int cin, int cout, double flops_exec) {
    if (!prof_open_) return;
    int gi = -1;
    for (size_t i = 0; i < prof_groups_.size(); ++i) if (prof_groups_[i].key == key) { gi = (int)i; break; }
    if (gi < 0) { ProfGroup g; g.key = key; g.kernel = kernel; g.level = level; g.cin = cin; g.cout = cout; prof_groups_.push_back(g); gi = (int)prof_groups_.size() - 1; }
    prof_.back().group = gi; prof_.back().flops_exec = flops_exec;
}
void Engine::prof_end(hipStream_t s) {
    if (!prof_open_) return;
    IRE_HIP(hipEventRecord(prof_.back().e1, s));
    prof_chain_ = true; prof_chain_stream_ = s;
}
void Engine::prof_collect() {
    prof_chain_ = false;
    if (prof_.empty()) return;
    IRE_HIP(hipDeviceSynchronize());
    for (auto& r : prof_) {
        float ms = 0.f;
        IRE_HIP(hipEventElapsedTime(&ms, r.e0, r.e1));
        prof_ms_[r.fam] += ms; prof_flops_[r.fam] += r.flops; prof_bytes_[r.fam] += r.bytes; prof_n_[r.fam] += 1;
        prof_flops_exec_[r.fam] += r.flops_exec;
        if (r.group >= 0) { ProfGroup& g = prof_groups_[r.group]; g.ms += ms; g.flops += r.flops; g.flops_exec += r.flops_exec; g.bytes += r.bytes; g.n += 1; }
        if (r.own_e0) ev_pool_.push_back(r.e0);
        ev_pool_.push_back(r.e1);
    }
    prof_.clear();
}
// mode: low byte 0 off / 1 every family / 2 the 3x3 conv family only; bits 8.. = N: in mode 2 time only every N-th pass of the network
// (0, 1: every pass).  An event record is a packet of its own between two kernels: 39 per step cost 1.35 % of a 1024^2 bs 8 step.
void Engine::profile_enable(int mode) {
    prof_collect();
    prof_on_ = mode & 0xff;
    prof_every_ = std::max(1, mode >> 8);
    prof_pass_ = 0; prof_skip_ = false;
}
void Engine::profile_reset() {
    prof_collect();
    for (int i = 0; i < FAM_COUNT; ++i) { prof_ms_[i] = prof_flops_[i] = prof_bytes_[i] = prof_flops_exec_[i] = 0; prof_n_[i] = 0; }
    prof_groups_.clear();
}
std::string Engine::profile_report() {
    prof_collect();
    std::string out = "[";
    char buf[512];
    for (size_t i = 0; i < prof_groups_.size(); ++i) {
        const ProfGroup& g = prof_groups_[i];
        std::snprintf(buf, sizeof buf, "%s{\"group\": \"%s\", \"kernel\": \"%s\", \"level\": %d, \"cin\": %d, \"cout\": %d, \"launches\": %lld, "
                      "\"ms\": %.6f, \"flops\": %.6e, \"flops_executed\": %.6e, \"bytes\": %.6e}",
                      i ? ", " : "", g.key.c_str(), g.kernel.c_str(), g.level, g.cin, g.cout, (long long)g.n, g.ms, g.flops, g.flops_exec, g.bytes);
        out += buf;
    }
    return out + "]";
}
void Engine::profile_query(int fam, double* ms, int64_t* launches, double* flops, double* bytes) {
    prof_collect();
    double m = 0, f = 0, b = 0; int64_t n = 0;
    for (int i = 0; i < FAM_COUNT; ++i)
        if (fam < 0 || fam == i) { m += prof_ms_[i]; f += prof_flops_[i]; b += prof_bytes_[i]; n += prof_n_[i]; }
    if (ms) *ms = m;
    if (launches) *launches = n;
    if (flops) *flops = f;
    if (bytes) *bytes = b;
}

// ------------------------------------------------------------------------------------------------
// debug capture
// ------------------------------------------------------------------------------------------------
void Engine::capture(const char* name, const unsigned short* d, size_t count, hipStream_t s) { capture_rows(name, d, count, count, 0, s); }
// `count` bf16 elements at `offset` of an entry of `total` floats (a whole batch: the entry itself; a row strip: its rows of the whole image).
// An entry of the right size is kept and only these rows are replaced: a second strip run under one debug_capture(true) keeps the rows the
// earlier run wrote and this one did not, so a comparison turns capture on (which clears) before every run.
void Engine::capture_rows(const char* name, const unsigned short* d, size_t count, size_t total, size_t offset, hipStream_t s) {
    if (!capture_ || !name) return;
    if (offset + count > total) fail(IRE_ERR_INTERNAL, std::string("internal: debug capture of rows beyond the tensor ") + name);
    IRE_HIP(hipStreamSynchronize(s));
    std::vector<unsigned short> hbuf(count);
    IRE_HIP(hipMemcpy(hbuf.data(), d, count * 2, hipMemcpyDeviceToHost));
    std::vector<float>& f = captured_[name];
    if (f.size() != total) f.assign(total, 0.f);
    for (size_t i = 0; i < count; ++i) {
        uint32_t u = (uint32_t)hbuf[i] << 16;
        std::memcpy(&f[offset + i], &u, 4);
    }
}
void Engine::capture_f32(const char* name, const float* d, size_t count, hipStream_t s) {
    if (!capture_ || !name) return;
    IRE_HIP(hipStreamSynchronize(s));
    std::vector<float> f(count);
    IRE_HIP(hipMemcpy(f.data(), d, count * 4, hipMemcpyDeviceToHost));
    captured_[name] = std::move(f);
}
bool Engine::debug_activation(const std::string& name, float* out, size_t* count) {
    auto it = captured_.find(name);
    if (it == captured_.end()) return false;
    if (count) *count = it->second.size();
    if (out) std::memcpy(out, it->second.data(), it->second.size() * sizeof(float));
    return true;
}
void Engine::debug_sums(int n, uint64_t* out) {
    if (n <= 0 || (size_t)n > io_.cap_imgs) fail(IRE_ERR_INVALID_INPUT, "invalid n for debug sums");
    IRE_HIP(hipDeviceSynchronize());
    IRE_HIP(hipMemcpy(out, io_.sums, sizeof(uint64_t) * 14 * n, hipMemcpyDeviceToHost));
}
// ire_debug_poison_scratch: every scratch allocation of the registry (buf_registry.hpp: the PROCESS's, whichever engine owns it) over
// its whole capacity, between two waits for the device.  Persistent entries were poisoned at birth and keep what their owners put there.
uint64_t Engine::debug_poison_scratch(int byte) {
    if (byte < 0 || byte > 255) fail(IRE_ERR_INVALID_INPUT, "invalid byte for ire_debug_poison_scratch: expected 0..255");
    IRE_HIP(hipSetDevice(device_));
    IRE_HIP(hipDeviceSynchronize());
    uint64_t filled = 0;
    for (const BufRegistry::Entry& e : BufRegistry::get().snapshot()) {
        if (e.persistent) continue;
        if (e.pinned) std::memset(e.p, byte, e.bytes);
        else IRE_HIP(hipMemset(e.p, byte, e.bytes));
        filled += e.bytes;
    }
    IRE_HIP(hipDeviceSynchronize());
    return filled;
}
// ire_debug_gn_finalize: host partials through gn_finalize_kernel (gn.hip: gn_fold with 512 threads, one workgroup per image), the
// coefficients copied back (synchronous; tests only)
void Engine::debug_gn_finalize(const float* stats, int nimg, int parts, int C, int hw, const float* gamma, const float* beta, const float* film,
                               int film_stride, int film_off, float* ab_out) {
    if (!stats || !gamma || !beta || !ab_out) fail(IRE_ERR_INVALID_INPUT, "invalid arguments to ire_debug_gn_finalize: null pointer");
    if (C != 32 && C != 64 && C != 128 && C != 256) fail(IRE_ERR_INVALID_INPUT, "invalid channels for ire_debug_gn_finalize: expected 32, 64, 128 or 256");
    if (nimg < 1 || nimg > 65535) fail(IRE_ERR_INVALID_INPUT, "invalid images for ire_debug_gn_finalize: expected 1..65535");
    if (parts < 1 || parts > (1 << 20)) fail(IRE_ERR_INVALID_INPUT, "invalid parts for ire_debug_gn_finalize: expected 1..2^20");
    if (hw < 1) fail(IRE_ERR_INVALID_INPUT, "invalid hw for ire_debug_gn_finalize: expected >= 1");
    if (film && (film_off < 0 || film_stride < 2 * C || film_off > film_stride - 2 * C))
        fail(IRE_ERR_INVALID_INPUT, "invalid film window for ire_debug_gn_finalize: film_off + 2 C leaves the row of film_stride");
    IRE_HIP(hipSetDevice(device_));
    const size_t nstats = (size_t)nimg * parts * 16, nfilm = film ? (size_t)nimg * film_stride : 0;
    Buf<DeviceMem> d_stats(sizeof(float) * nstats), d_gamma(sizeof(float) * C), d_beta(sizeof(float) * C), d_film(sizeof(float) * std::max<size_t>(nfilm, 1)),
        d_ab(sizeof(float2) * (size_t)nimg * C);
    hipStream_t s = main_stream_;
    IRE_HIP(hipMemcpyAsync(d_stats.get<float>(), stats, sizeof(float) * nstats, hipMemcpyHostToDevice, s));
    IRE_HIP(hipMemcpyAsync(d_gamma.get<float>(), gamma, sizeof(float) * C, hipMemcpyHostToDevice, s));
    IRE_HIP(hipMemcpyAsync(d_beta.get<float>(), beta, sizeof(float) * C, hipMemcpyHostToDevice, s));
    if (film) IRE_HIP(hipMemcpyAsync(d_film.get<float>(), film, sizeof(float) * nfilm, hipMemcpyHostToDevice, s));
    gn_finalize_launch(d_stats.get<float>(), nimg, parts, C, hw, d_gamma.get<float>(), d_beta.get<float>(), film ? d_film.get<float>() : nullptr,
                       film_stride, film_off, d_ab.get<float2>(), s);
    IRE_HIP(hipMemcpyAsync(ab_out, d_ab.get<float2>(), sizeof(float2) * (size_t)nimg * C, hipMemcpyDeviceToHost, s));
    IRE_HIP(hipStreamSynchronize(s));
}

// ------------------------------------------------------------------------------------------------
// RestoreNet-v0 schedule: a program of ops (built once per weight load), executed op by op
// ------------------------------------------------------------------------------------------------
void Engine::build_program() {
    program_.clear();
    auto gn = [&](const GNW& g) { Op o; o.kind = Op::GN; o.gn = &g; program_.push_back(o); };
    auto conv = [&](const ConvW& cw, int in0, int in1, int resid, int out, int lin, int lout, bool use_ab, const std::string& name) {
        Op o; o.kind = Op::CONV; o.cw = &cw; o.in0 = in0; o.in1 = in1; o.resid = resid; o.out = out; o.lin = lin; o.lout = lout;
        o.use_ab = use_ab; o.name = name;
        const bool upf = cw.desc.kind == CONV_UP && in1 != BUF_NONE;      // `up` composed with `fuse`: its output is what fuse's was
        o.halo_out = o.stats_out = conv_feeds_gn(cw.desc.kind, upf);
        program_.push_back(o);
    };
    // ResBlock: out = x + conv2(silu(gn2(conv1(silu(gn1(x)))))); the partials of x were written by x's producer
    auto resblock = [&](const RBW& rb, int x, int tmp, int out, int l, const std::string& name) {
        // GroupNorm+FiLM+SiLU is applied by the consuming conv while it stages its input (a separate activation pass lost every
        // A/B from round 1 to round 3 and was removed in round 4)
        gn(rb.gn1);
        conv(rb.conv1, x, BUF_NONE, BUF_NONE, tmp, l, l, true, name + ".h");
        gn(rb.gn2);
        conv(rb.conv2, tmp, BUF_NONE, x, out, l, l, true, name);
    };
    conv(net_.stem, BUF_NONE, BUF_NONE, BUF_NONE, buf_id(0, 0), 0, 0, false, "stem");
    int x = buf_id(0, 0);
    for (int l = 0; l < 4; ++l) {
        const int rb1_out = (l < 3) ? buf_id(l, 4) : buf_id(l, 3);
        resblock(net_.enc[l][0], x, buf_id(l, 1), buf_id(l, 2), l, "enc" + std::to_string(l) + ".rb0");
        resblock(net_.enc[l][1], buf_id(l, 2), buf_id(l, 1), rb1_out, l, "enc" + std::to_string(l) + ".rb1");
        if (l < 3) {
            conv(net_.down[l], rb1_out, BUF_NONE, BUF_NONE, buf_id(l + 1, 0), l, l + 1, false, "down" + std::to_string(l));
            x = buf_id(l + 1, 0);
        }
    }
    resblock(net_.mid[0], buf_id(3, 3), buf_id(3, 1), buf_id(3, 0), 3, "mid.rb0");
    resblock(net_.mid[1], buf_id(3, 0), buf_id(3, 1), buf_id(3, 2), 3, "mid.rb1");
    int deep = buf_id(3, 2);
    for (int l = 2; l >= 0; --l) {
        const std::string sl = std::to_string(l);
        if (up_is_composed(sw_, net_.up[l].desc)) {
            conv(net_.up[l], deep, buf_id(l, 4), BUF_NONE, buf_id(l, 2), l + 1, l, false, "fuse" + sl);     // one kernel, the `up` tensor never exists
        } else {
            conv(net_.up[l], deep, BUF_NONE, BUF_NONE, buf_id(l, 0), l + 1, l, false, "up" + sl);
            conv(net_.fuse[l], buf_id(l, 0), buf_id(l, 4), BUF_NONE, buf_id(l, 2), l, l, false, "fuse" + sl);
        }
        resblock(net_.dec[l][0], buf_id(l, 2), buf_id(l, 1), buf_id(l, 3), l, "dec" + sl + ".rb0");
        resblock(net_.dec[l][1], buf_id(l, 3), buf_id(l, 1), buf_id(l, 0), l, "dec" + sl + ".rb1");
        deep = buf_id(l, 0);
    }
    gn(net_.head_gn);
    conv(net_.head, deep, BUF_NONE, BUF_NONE, BUF_NONE, 0, 0, true, "");
}

Geo Engine::geo_of_lane(const Lane& L, int nimg, int h, int w, const uint8_t* d_in, uint8_t* d_out) {
    Geo g;
    g.nimg = nimg; g.h = h; g.w = w; g.H = h;
    for (int l = 0; l < 4; ++l)
        for (int b = 0; b < 5; ++b) g.buf[l][b] = L.v.buf[l][b];
    g.img_in = d_in; g.img_out = d_out;
    return g;
}

// One convolution launch: conv_plan.hpp decides everything that can be decided without a device, this binds the pointers the plan
// names and launches.
void Engine::exec_conv(Run& R, const Op& op, const Geo& g) {
    const ConvW& cw = *op.cw;
    const ConvDesc& d = cw.desc;
    ConvSite site;
    site.lin = op.lin; site.lout = op.lout; site.use_ab = op.use_ab; site.has_in1 = op.in1 != BUF_NONE; site.stats_out = op.stats_out;
    site.nimg = g.nimg; site.h = g.h; site.w = g.w; site.H = g.H; site.halo = g.halo; site.has_up = g.has_up; site.has_down = g.has_down;
    site.y0 = g.y0; site.cus = cus_;
    const ConvPlan p = plan_conv(sw_, d, site, precision_ == IRE_PRECISION_FP8);

    // inputs are addressed from the buffer start (halo row included: in_row_off), outputs / residual from the first real row
    auto in_ptr = [&](int id) -> const unsigned short* { return id == BUF_NONE ? nullptr : g.buf[id >> 3][id & 7]; };
    auto out_ptr = [&](int id) -> unsigned short* {
        if (id == BUF_NONE) return nullptr;
        const int l = id >> 3;
        return g.buf[l][id & 7] + (size_t)g.halo * (g.w >> l) * kWidths[l];
    };
    const int Hout = g.h >> op.lout, Wout = g.w >> op.lout;
    ConvArgs a{};
    a.in0 = (d.kind == CONV_STEM) ? (const void*)g.img_in : (const void*)in_ptr(op.in0);
    a.in1 = in_ptr(op.in1);
    if (p.in1_first_row) a.in1 = in_ptr(op.in1) + (size_t)g.halo * Wout * d.cout;
    a.cin0 = d.cin0; a.cin1 = p.cin1; a.kc_split = d.kc_split; a.nkc = p.nkc; a.nblocks = p.nblocks; a.w4_nt = p.w4_nt; a.fp8 = p.fp8;
    const unsigned short* const slabs[] = {nullptr, cw.d_w, cw.d_wp, cw.d_w4, cw.d_w4h, cw.d_wstem, cw.d_wd, cw.d_wu, cw.d_wuf, cw.d_wdq, cw.d_wuq, cw.d_wsq,
                                           cw.d_wsk, reinterpret_cast<const unsigned short*>(cw.d_w8x), reinterpret_cast<const unsigned short*>(cw.d_w8)};   // WeightArr
    const float* const biases[] = {cw.d_bias, cw.d_bias_uf, cw.d_bias8};      // BiasArr
    a.w = slabs[p.w]; a.w1 = slabs[p.w1]; a.bias = biases[p.bias];
    if (p.fp8) a.oscale = cw.d_oscale;
    if (p.zeros) a.zeros = d_zero_.get<void>();
    a.ab = op.use_ab ? R.ab : nullptr; a.resid = out_ptr(op.resid); a.out = out_ptr(op.out);
    a.u8_in = d.kind == CONV_HEAD ? g.img_in + (size_t)g.halo * g.w * 3 : nullptr;
    a.u8_out = d.kind == CONV_HEAD ? g.img_out : nullptr;
    a.Hin = g.h >> op.lin; a.Win = g.w >> op.lin; a.Hout = Hout; a.Wout = Wout;
    a.in_rows = p.in_rows; a.in_row_off = p.in_row_off; a.iy_lo = p.iy_lo; a.iy_span = p.iy_span;
    a.cout = p.cout; a.group_size = p.group_size; a.tiles_x = p.tiles_x; a.tiles_y = p.tiles_y; a.nimg = g.nimg;
    // ping-pong: this conv may still be reading R.stats in its folded finalize
    if (op.stats_out) a.stats = (R.stats_alt ? R.stats_alt : R.stats) + p.stats_offset();
    a.prio_young = sw_.prio_young;
    // walk order (persist.hpp): the first conv of a pass forward, every later one against the conv before it on this stream, so that it
    // starts on the rows the Infinity Cache still holds.  The v1 template has no cursor: it walks forward whatever is asked.
    a.walk_rev = R.snake && R.next_rev && p.kernel != K_V1;
    R.next_rev = !a.walk_rev;
    const bool rb = d.kind == CONV_RB1 || d.kind == CONV_RB2;
    if (stamps_dev_ && rb && d.cout == stamps_cout_ && (d.kind == CONV_RB2) == stamps_resid_) a.stamps = stamps_dev_.get<unsigned long long>();
    if (R.gn_pending) {
        // the deferred GroupNorm finalize of this conv's input: inside the kernel's prologue where it has one (gn_fold.hpp)
        if (p.folds_gn) {
            const GNW& gn = *R.gn_pending;
            a.gn_stats = R.gn_stats; a.gn_parts = R.gn_parts; a.gn_hw = (g.H >> gn.level) * (g.w >> gn.level);
            a.gn_gamma = gn.d_gamma; a.gn_beta = gn.d_beta; a.gn_film = R.film; a.gn_film_stride = kFilmDim; a.gn_film_off = kFilmOff[gn.level];
            a.ab_w = R.ab;
            R.gn_pending = nullptr;
        } else flush_gn(R, g);
    }
    prof_begin(p.fam, R.stream, p.flops, p.bytes);
    switch (p.kernel) {
        case K_V1: conv_launch(d.kind, a, R.stream); break;
        case K_F8: conv_f8_launch(p.resid, a, R.stream); break;
        case K_PK: conv_pk_launch(p.resid, a, R.stream); break;
        case K_W4: conv_w4_launch(p.resid, a, R.stream); break;
        case K_PC: conv_pc_launch(p.resid, false, a, R.stream); break;
        case K_RB: conv_rb_launch(p.resid, p.fused_act, a, R.stream); break;
        case K_PC_HEAD: conv_pc_launch(false, true, a, R.stream); break;
        case K_RB_HEAD: conv_head_launch(a, R.stream); break;
        case K_DNQ: conv_dnq_launch(a, R.stream); break;
        case K_DOWN: conv_down_launch(a, R.stream); break;
        case K_STEM: conv_stem_launch(a, R.stream); break;
        case K_UPQ: conv_upq_launch(a, R.stream); break;
        case K_UP_FUSED:
        case K_UP_SUB: conv_up_subpixel_launch(a, R.stream); break;
        case K_UP_RB: conv_up_launch(a, R.stream); break;
    }
    prof_tag(p.key, p.kname, op.lout, d.cin, d.cout, p.flops_exec);       // layer group of this launch (bench.py roofline.per_level)
    prof_end(R.stream);
    if (op.stats_out) {
        R.stat_parts = p.stat_parts;
        if (R.stats_alt) std::swap(R.stats, R.stats_alt);          // R.stats = the partials produced last
    }
    if (capture_ && !op.name.empty() && a.out && g.halo == 0) capture(op.name.c_str(), a.out, (size_t)g.nimg * Hout * Wout * d.cout, R.stream);
    // a row strip: its real rows (a.out is the first of them) at their place in an entry of the whole image's size, which the first strip
    // to write it creates.  All sessions of one engine fill the same entry; a process that holds only some strips captures only its own
    // rows (the others stay zero).  The (A, B) of a strip run is captured once per op by StripSession::run_op: one finalize serves all strips.
    if (capture_ && !op.name.empty() && a.out && g.halo == 1)
        capture_rows(op.name.c_str(), a.out, (size_t)Hout * Wout * d.cout, (size_t)(g.H >> op.lout) * Wout * d.cout,
                     (size_t)(g.y0 >> op.lout) * Wout * d.cout, R.stream);
    // the (A, B) of y = x A + B this conv applied while staging, [image][cin][2] floats, as "<layer>.ab" ("head.ab" for the head): what a
    // per-layer check needs to recompute the activated operand from the very coefficients the kernel used
    if (capture_ && a.ab != nullptr && g.halo == 0)
        capture_f32(((op.name.empty() ? std::string("head") : op.name) + ".ab").c_str(), reinterpret_cast<const float*>(R.ab), (size_t)g.nimg * d.cin * 2, R.stream);
}

void Engine::flush_gn(Run& R, const Geo& g) {
    const GNW& gn = *R.gn_pending;
    prof_begin(FAM_GN, R.stream, 0, 0);
    gn_finalize_launch(R.gn_stats, g.nimg, R.gn_parts, gn.C, (g.H >> gn.level) * (g.w >> gn.level), gn.d_gamma, gn.d_beta, R.film, kFilmDim,
                       kFilmOff[gn.level], R.ab, R.stream);
    prof_end(R.stream);
    R.gn_pending = nullptr;
}

void Engine::exec_op(Run& R, const Op& op, const Geo& g) {
    switch (op.kind) {
        case Op::GN: {
            // the partials of the tensor produced last; finalized by the consumer itself (exec_conv) unless that is switched off
            // or this is a row strip (one finalize over the gathered array serves all strips)
            R.gn_pending = op.gn; R.gn_stats = R.stats; R.gn_parts = R.stat_parts;
            if (!sw_.gn_fold || g.halo) flush_gn(R, g);
            break;
        }
        case Op::CONV: exec_conv(R, op, g); break;
    }
}

void Engine::run_network(Lane& L, int nimg, int h, int w, const uint8_t* d_in, uint8_t* d_out, const float* d_film) {
    Run R;
    R.stream = L.stream; R.stats = L.v.stats; R.stats_alt = L.v.stats2; R.ab = L.v.ab; R.film = d_film;
    R.snake = snake_;
    const Geo g = geo_of_lane(L, nimg, h, w, d_in, d_out);
    // inside one pass of the op list a profiled launch's end event is the next one's start (prof_begin): nothing but the
    // engine's own wrapped launches goes onto the stream here.  Everywhere else (copies, host syncs between calls) records
    // keep their own start event.
    prof_chain_ = false;
    prof_chainable_ = capture_ == false;
    prof_skip_ = prof_on_ == 2 && prof_every_ > 1 && (prof_pass_ % prof_every_) != 0;
    ++prof_pass_;
    for (const Op& op : program_) exec_op(R, op, g);
    prof_chainable_ = false;
    prof_chain_ = false;
    prof_skip_ = false;
}

// ------------------------------------------------------------------------------------------------
// entry points
// ------------------------------------------------------------------------------------------------
void Engine::classify_device(const uint8_t* d_rgb, int n, int h, int w, const uint8_t* d_is_jpeg, double* d_scores,
                             int32_t* d_label, hipStream_t stream) {
    check_shape(n, h, w, false);
    if (!d_rgb) fail(IRE_ERR_INVALID_INPUT, "invalid input: null image pointer");
    ensure_io(n, 1, 1);
    prof_begin(FAM_CLASSIFIER, stream, 0, (double)n * h * w * 3);
    classifier_launch(tables_, d_rgb, n, h, w, d_is_jpeg, io_.sums, d_scores ? d_scores : io_.scores, d_label ? d_label : io_.label,
                      io_.cond, stream);
    prof_end(stream);
    last_n_ = n;
}

void Engine::restore_device(const uint8_t* d_rgb, int n, int h, int w, const double* d_scores, const uint8_t* d_is_jpeg,
                            uint8_t* d_out, hipStream_t stream) {
    check_shape(n, h, w, true);
    if (!net_.loaded) fail(IRE_ERR_UNAVAILABLE, "service unavailable: RestoreNet weights are not loaded");
    if (!d_rgb || !d_out) fail(IRE_ERR_INVALID_INPUT, "invalid input: null image pointer");
    ensure_io(n, 1, 1);
    ensure_workspace(n, h, w);
    if (d_scores) {
        scores_to_cond_launch(d_scores, n, io_.cond, stream);
    } else {
        // classified inside: the scan's last workgroup per image writes the FiLM vector too (no film launch, no boundary behind the scan)
        prof_begin(FAM_CLASSIFIER, stream, 0, (double)n * h * w * 3);
        classifier_launch(tables_, d_rgb, n, h, w, d_is_jpeg, io_.sums, io_.scores, io_.label, io_.cond, stream, net_.d_film_w, net_.d_film_b, kFilmDim, io_.film);
        prof_end(stream);
    }
    if (d_scores) {
        prof_begin(FAM_GN, stream, 0, 0);
        film_launch(io_.cond, n, net_.d_film_w, net_.d_film_b, kFilmDim, io_.film, stream);
        prof_end(stream);
    }
    last_n_ = n;
    note_restored(n);

    const int lanes_used = std::min(num_lanes_, n);
    const size_t img_bytes = (size_t)h * w * 3;
    if (lanes_used == 1) {
        Lane L = lanes_[0];
        L.stream = stream;  // run inline on the caller's stream
        run_network(L, n, h, w, d_rgb, d_out, io_.film);
        return;
    }
    const int per = ceil_div(n, lanes_used);
    IRE_HIP(hipEventRecord(fork_ev_, stream));
    for (int i = 0; i < lanes_used; ++i) {
        const int i0 = i * per, cnt = std::min(per, n - i0);
        if (cnt <= 0) break;
        Lane& L = lanes_[i];
        IRE_HIP(hipStreamWaitEvent(L.stream, fork_ev_, 0));
        run_network(L, cnt, h, w, d_rgb + (size_t)i0 * img_bytes, d_out + (size_t)i0 * img_bytes,
                    io_.film + (size_t)i0 * kFilmDim);
        IRE_HIP(hipEventRecord(L.done, L.stream));
        IRE_HIP(hipStreamWaitEvent(stream, L.done, 0));
    }
}

void Engine::restore_tiled_device(const uint8_t* d_rgb, int h, int w, int nstrips, const double* d_scores, const uint8_t* d_is_jpeg,
                                  uint8_t* d_out, hipStream_t stream) {
    if (!d_rgb || !d_out) fail(IRE_ERR_INVALID_INPUT, "invalid input: null image pointer");
    if (!tiled_ || tiled_h_ != h || tiled_w_ != w || tiled_n_ != nstrips) {
        IRE_HIP(hipDeviceSynchronize());
        tiled_.reset();
        tiled_.reset(new StripSession(*this, h, w, nstrips, 0, nstrips, nullptr));
        tiled_h_ = h; tiled_w_ = w; tiled_n_ = nstrips;
    }
    ensure_io(1, 1, 1);
    if (!d_scores) {
        prof_begin(FAM_CLASSIFIER, stream, 0, (double)h * w * 3);
        classifier_launch(tables_, d_rgb, 1, h, w, d_is_jpeg, io_.sums, io_.scores, io_.label, io_.cond, stream);
        prof_end(stream);
        d_scores = io_.scores;
    }
    note_restored(1);          // tiled jobs count in the images/sec gauge like whole-batch calls
    tiled_->run_all(d_rgb, d_scores, d_out, stream);
}

void Engine::restore_device_mixed(const uint8_t* d_rgb, int n, int h, int w, const double* host_scores, const uint8_t* has_scores,
                                  const uint8_t* d_is_jpeg, uint8_t* d_out, hipStream_t stream) {
    check_shape(n, h, w, true);
    restore_fit_device_mixed(d_rgb, n, h, w, host_scores, has_scores, d_is_jpeg, d_out, nullptr, 0, stream);
}

// pad into d_pad_in_, the network on the padded shape into d_pad_out_ (d_scores: of the original pixels, never null here)
void Engine::restore_padded(const uint8_t* d_rgb, int n, int h, int w, const double* d_scores, const uint8_t* d_is_jpeg, hipStream_t stream) {
    if (!net_.loaded) fail(IRE_ERR_UNAVAILABLE, "service unavailable: RestoreNet weights are not loaded");
    const int H = fit_dim(h), W = fit_dim(w);
    ensure_pad(n, H, W);
    pad_edge_launch(d_rgb, n, h, w, d_pad_in_.get<uint8_t>(), H, W, stream);
    restore_device(d_pad_in_.get<uint8_t>(), n, H, W, d_scores, d_is_jpeg, d_pad_out_.get<uint8_t>(), stream);
}

void Engine::restore_fit_device(const uint8_t* d_rgb, int n, int h, int w, const double* d_scores, const uint8_t* d_is_jpeg, uint8_t* d_out,
                                hipStream_t stream) {
    check_fit(n, h, w);
    if (fit_is_aligned(h, w)) { restore_device(d_rgb, n, h, w, d_scores, d_is_jpeg, d_out, stream); return; }
    if (!d_rgb || !d_out) fail(IRE_ERR_INVALID_INPUT, "invalid input: null image pointer");
    ensure_io(n, 1, 1);
    restore_padded(d_rgb, n, h, w, scores_of_original(d_rgb, n, h, w, d_scores, d_is_jpeg, stream), d_is_jpeg, stream);
    crop_window_launch(d_pad_out_.get<uint8_t>(), n, fit_dim(h), fit_dim(w), d_out, h, w, stream);
}

// the batcher's results as text: the stored PNG's characters, or with IRE_FLAG_RESULT_PNG_DEFLATE / IRE_FLAG_RESULT_JPEG [uint64 count | characters] per result
void Engine::encode_result(const uint8_t* d_rgb, int n, int h, int w, size_t row_pitch, size_t image_pitch, uint8_t* d_txt, size_t txt_stride, hipStream_t s) {
    enc_.places(result_format_ ? *result_format_ : kStoredPng, d_rgb, n, h, w, row_pitch, image_pitch, d_txt, txt_stride, s);
}

const double* Engine::scores_of_original(const uint8_t* d_rgb, int n, int h, int w, const double* d_scores, const uint8_t* d_is_jpeg, hipStream_t stream) {
    if (d_scores || fit_is_aligned(h, w)) return d_scores;
    classify_device(d_rgb, n, h, w, d_is_jpeg, io_.scores, io_.label, stream);
    return io_.scores;
}

const double* Engine::settle_scores(const uint8_t* d_rgb, int n, int h, int w, const double* host_scores, const uint8_t* has_scores, const uint8_t* d_is_jpeg,
                                    hipStream_t stream) {
    bool any_missing = false, any_given = false;
    for (int i = 0; i < n; ++i) { if (has_scores && has_scores[i]) any_given = true; else any_missing = true; }
    // null: restore_device classifies inside (its scan also writes the FiLM vector); only an aligned shape may
    if (!any_given && fit_is_aligned(h, w)) return nullptr;
    if (any_missing) classify_device(d_rgb, n, h, w, d_is_jpeg, io_.scores, io_.label, stream);      // the ORIGINAL pixels
    for (int i = 0; i < n; ++i)
        if (has_scores && has_scores[i]) IRE_HIP(hipMemcpyAsync(io_.scores + 7 * i, host_scores + 7 * i, sizeof(double) * 7, hipMemcpyHostToDevice, stream));
    return io_.scores;
}

void Engine::restore_fit_device_mixed(const uint8_t* d_rgb, int n, int h, int w, const double* host_scores, const uint8_t* has_scores,
                                      const uint8_t* d_is_jpeg, uint8_t* d_out, uint8_t* d_txt, size_t txt_stride, hipStream_t stream) {
    check_fit(n, h, w);
    ensure_io(n, 1, 1);
    const bool aligned = fit_is_aligned(h, w);
    const double* d_sc = settle_scores(d_rgb, n, h, w, host_scores, has_scores, d_is_jpeg, stream);
    if (aligned) {
        restore_device(d_rgb, n, h, w, d_sc, d_is_jpeg, d_out, stream);
        if (d_txt) encode_result(d_out, n, h, w, (size_t)3 * w, (size_t)3 * w * h, d_txt, txt_stride, stream);
        return;
    }
    const int H = fit_dim(h), W = fit_dim(w);
    restore_padded(d_rgb, n, h, w, d_sc, d_is_jpeg, stream);
    if (d_txt) encode_result(d_pad_out_.get<uint8_t>(), n, h, w, (size_t)3 * W, (size_t)3 * W * H, d_txt, txt_stride, stream);     // the crop costs no pass of its own
    else crop_window_launch(d_pad_out_.get<uint8_t>(), n, H, W, d_out, h, w, stream);
}

// ---- fusion jobs: restore every view, pad the windows to the fusion shape, fuse, crop / encode -- all on the stream ----------------
void Engine::check_fuse_fit(int nsets, int k, int h, int w) const {
    if (k < 2 || k > 3) fail(IRE_ERR_INVALID_INPUT, "invalid view count for fusion: expected 2..3");
    if (h < 1 || w < 1 || h > 8192 || w > 8192) fail(IRE_ERR_INVALID_INPUT, "invalid image size: height and width must be in 1..8192");
    if (!piece_addressable(fit_dim(h), fit_dim(w), 0)) fail(IRE_ERR_INVALID_INPUT, not_addressable(fit_dim(h), fit_dim(w)));      // before anything is allocated for it
    if (nsets < 1 || nsets > kFuseMaxSets || nsets * k > max_batch_) fail(IRE_ERR_INVALID_INPUT, "invalid batch size for fusion: expected 1..16 view sets of at most max_batch images");
}

// Everything a fusion batch of this shape needs beyond the network's own buffers, sized by the grow rule for the largest batch of
// the shape that the batcher can gather WHATEVER its k (a slot of k = 2 holds the most sets, a slot of either k at most max_batch
// views), so that only the FIRST job of a shape allocates and a later job of the other k does not (FuseBufs::regrow synchronises
// the device).
void Engine::ensure_fuse_io(int nsets, int k, int HF, int WF, hipStream_t s) {
    IRE_HIP(hipSetDevice(device_));
    const size_t px = (size_t)HF * WF, per = px * 3;
    const size_t full_sets = (size_t)std::max(nsets, std::min(kFuseMaxSets, max_batch_ / 2));
    const size_t full_views = (size_t)std::max(nsets * k, std::min(kFuseMaxSets * 3, max_batch_));
    const size_t need_in = per * (size_t)nsets * k, need_out = per * (size_t)nsets;
    if (need_in > d_fuse_in_.bytes() || need_out > d_fuse_out_.bytes()) {
        IRE_HIP(hipDeviceSynchronize());
        d_fuse_in_.grow(need_in, batch_room(need_in, per * full_views));
        d_fuse_out_.grow(need_out, batch_room(need_out, per * full_sets));
    }
    if (!d_fuse_sc_) d_fuse_sc_ = Buf<DeviceMem>(sizeof(double) * 7 * kFuseMaxSets);
    // the chain's scratch, about 3.4 bytes per pixel and set (device_buf.hpp FuseBufs), in sets: a whole batch or what was asked for
    const size_t want_sets = batch_room(px * 4 * (size_t)nsets, px * 4 * full_sets) / (px * 4);
    fuse_reserve((int)want_sets, px, s);
}

void Engine::fuse_fit_core(const uint8_t* d_views, int nsets, int k, int h, int w, const double* d_sc, const uint8_t* d_is_jpeg, uint8_t* d_out, uint8_t* d_txt,
                           size_t txt_stride, hipStream_t stream) {
    if (!d_views || !d_out) fail(IRE_ERR_INVALID_INPUT, "invalid input: null image pointer");
    if (!net_.loaded) fail(IRE_ERR_UNAVAILABLE, "service unavailable: RestoreNet weights are not loaded");
    const int n = nsets * k, H = fit_dim(h), W = fit_dim(w), HF = fuse_dim(h), WF = fuse_dim(w);
    const bool aligned = fit_is_aligned(h, w), direct = aligned && h >= 64 && w >= 64;      // direct: the network's output IS the fusion input
    ensure_fuse_io(nsets, k, HF, WF, stream);
    uint8_t* f_in = d_fuse_in_.get<uint8_t>();
    if (direct) restore_device(d_views, n, h, w, d_sc, d_is_jpeg, f_in, stream);
    else {
        if (aligned) { ensure_pad(n, h, w); restore_device(d_views, n, h, w, d_sc, d_is_jpeg, d_pad_out_.get<uint8_t>(), stream); }
        else restore_padded(d_views, n, h, w, d_sc, d_is_jpeg, stream);
        // the restored h x w windows where the network left them -> the fusion input, edge-replicated (never the network's own padding)
        pad_edge_pitched_launch(d_pad_out_.get<uint8_t>(), n, h, w, (size_t)3 * W, (size_t)3 * W * H, f_in, HF, WF, stream);
    }
    // the noise score of view 0 of every PADDED set, into a buffer of its own: io_.scores holds the jobs' scores
    double* f_sc = d_fuse_sc_.get<double>();
    // (ONE launch for all sets: the view 0s lie k images apart; the scan's sums are integers, so its grid does not change a score)
    prof_begin(FAM_CLASSIFIER, stream, 0, (double)nsets * HF * WF * 3);
    classifier_launch(tables_, f_in, nsets, HF, WF, nullptr, io_.sums, f_sc, nullptr, nullptr, stream, nullptr, nullptr, 0, nullptr, (size_t)k * HF * WF * 3);
    prof_end(stream);
    uint8_t* fused = (!d_txt && direct) ? d_out : d_fuse_out_.get<uint8_t>();
    fuse_launch_device_tables(f_in, nsets, k, HF, WF, f_sc + IRE_SCORE_NOISE, 7, fused, nullptr, stream);
    if (d_txt) encode_result(fused, nsets, h, w, (size_t)3 * WF, (size_t)3 * WF * HF, d_txt, txt_stride, stream);     // the crop costs no pass of its own
    else if (!direct) crop_window_launch(fused, nsets, HF, WF, d_out, h, w, stream);
}

void Engine::restore_fuse_fit_device_mixed(const uint8_t* d_views, int nsets, int k, int h, int w, const double* host_scores, const uint8_t* has_scores,
                                           const uint8_t* d_is_jpeg, uint8_t* d_out, uint8_t* d_txt, size_t txt_stride, hipStream_t stream) {
    check_fuse_fit(nsets, k, h, w);
    const int n = nsets * k;
    ensure_io(n, 1, 1);
    // the views' scores exactly as restore_fit_device_mixed settles them for n single jobs
    fuse_fit_core(d_views, nsets, k, h, w, settle_scores(d_views, n, h, w, host_scores, has_scores, d_is_jpeg, stream), d_is_jpeg, d_out, d_txt, txt_stride, stream);
}

void Engine::restore_fuse_fit_device(const uint8_t* d_views, int nsets, int k, int h, int w, const double* d_scores, const uint8_t* d_is_jpeg, uint8_t* d_out,
                                     hipStream_t stream) {
    check_fuse_fit(nsets, k, h, w);
    const int n = nsets * k;
    ensure_io(n, 1, 1);
    fuse_fit_core(d_views, nsets, k, h, w, scores_of_original(d_views, n, h, w, d_scores, d_is_jpeg, stream), d_is_jpeg, d_out, nullptr, 0, stream);
}

double Engine::note_restored(int n) {
    const double t = now_s();
    if (n > 0) {
        batches_run_ += 1; images_restored_ += n; last_batch_ = n;
        recent_.emplace_back(t, n);
    }
    while (!recent_.empty() && recent_.front().first < t - 10.0) recent_.pop_front();
    return t;
}

void Engine::get_stats(ire_engine_stats* out) {
    out->batches = batches_run_;
    out->images = images_restored_;
    out->last_batch = last_batch_;
    out->max_batch = max_batch_;
    const double t = note_restored(0);
    double imgs = 0;
    for (auto& r : recent_) imgs += r.second;
    // span from the first call of the window to now; one lone call reports over >= 1 s so the gauge decays instead of spiking
    const double span = recent_.empty() ? 1.0 : std::max(1.0, t - recent_.front().first);
    out->images_per_sec = recent_.empty() ? 0.0 : imgs / span;
}

void Engine::classify_host(const uint8_t* rgb, int n, int h, int w, int row_stride, const uint8_t* is_jpeg, double* scores,
                           int32_t* label) {
    check_shape(n, h, w, false);
    if (!rgb || !scores) fail(IRE_ERR_INVALID_INPUT, "invalid input: null pointer");
    if (row_stride < 3 * w) fail(IRE_ERR_INVALID_INPUT, "invalid row_stride (< 3*w)");
    ensure_io(n, h, w);
    hipStream_t s = main_stream_;
    IRE_HIP(hipMemcpy2DAsync(io_.in, (size_t)3 * w, rgb, (size_t)row_stride, (size_t)3 * w, (size_t)n * h, hipMemcpyHostToDevice, s));
    std::vector<uint8_t> jp(n, 1);
    if (is_jpeg) std::memcpy(jp.data(), is_jpeg, n);
    IRE_HIP(hipMemcpyAsync(io_.jpeg, jp.data(), n, hipMemcpyHostToDevice, s));
    classify_device(io_.in, n, h, w, io_.jpeg, io_.scores, io_.label, s);
    IRE_HIP(hipMemcpyAsync(scores, io_.scores, sizeof(double) * 7 * n, hipMemcpyDeviceToHost, s));
    if (label) IRE_HIP(hipMemcpyAsync(label, io_.label, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s));
    IRE_HIP(hipStreamSynchronize(s));
}

// the synchronous host entry behind ire_restore and ire_restore_fit: upload, classify (unless scores are given), restore, download
void Engine::restore_host_impl(const uint8_t* rgb, int n, int h, int w, const double* scores, const uint8_t* is_jpeg,
                               uint8_t* out, ire_timings* t) {
    if (!rgb || !out) fail(IRE_ERR_INVALID_INPUT, "invalid input: null pointer");
    ensure_io(n, h, w);
    hipStream_t s = main_stream_;
    const size_t bytes = (size_t)n * h * w * 3;
    IRE_HIP(hipEventRecord(ev_[0], s));
    IRE_HIP(hipMemcpyAsync(io_.in, rgb, bytes, hipMemcpyHostToDevice, s));
    std::vector<uint8_t> jp(n, 1);
    if (is_jpeg) std::memcpy(jp.data(), is_jpeg, n);
    IRE_HIP(hipMemcpyAsync(io_.jpeg, jp.data(), n, hipMemcpyHostToDevice, s));
    const double* d_sc = nullptr;
    IRE_HIP(hipEventRecord(ev_[1], s));
    if (scores) {
        IRE_HIP(hipMemcpyAsync(io_.scores, scores, sizeof(double) * 7 * n, hipMemcpyHostToDevice, s));
        d_sc = io_.scores;
    } else {
        // classify as its own step so classify_ms / restore_ms mirror restorator.js:59-95 (the pixels as uploaded, never a padded copy)
        prof_begin(FAM_CLASSIFIER, s, 0, (double)n * h * w * 3);
        classifier_launch(tables_, io_.in, n, h, w, io_.jpeg, io_.sums, io_.scores, io_.label, io_.cond, s);
        prof_end(s);
        d_sc = io_.scores;
    }
    IRE_HIP(hipEventRecord(ev_[2], s));
    restore_fit_device(io_.in, n, h, w, d_sc, io_.jpeg, io_.out, s);       // (an aligned shape: restore_device as it is)
    IRE_HIP(hipEventRecord(ev_[3], s));
    IRE_HIP(hipMemcpyAsync(out, io_.out, bytes, hipMemcpyDeviceToHost, s));
    IRE_HIP(hipStreamSynchronize(s));
    if (t) {
        float a = 0, b = 0, c = 0;
        IRE_HIP(hipEventElapsedTime(&a, ev_[1], ev_[2]));
        IRE_HIP(hipEventElapsedTime(&b, ev_[2], ev_[3]));
        IRE_HIP(hipEventElapsedTime(&c, ev_[0], ev_[3]));
        t->classify_ms = a; t->restore_ms = b; t->total_ms = c;
    }
}

void Engine::restore_host(const uint8_t* rgb, int n, int h, int w, const double* scores, const uint8_t* is_jpeg, uint8_t* out, ire_timings* t) {
    check_shape(n, h, w, true);
    restore_host_impl(rgb, n, h, w, scores, is_jpeg, out, t);
}

void Engine::restore_fit_host(const uint8_t* rgb, int n, int h, int w, const double* scores, const uint8_t* is_jpeg, uint8_t* out, ire_timings* t) {
    check_fit(n, h, w);
    restore_host_impl(rgb, n, h, w, scores, is_jpeg, out, t);
}

}  // namespace ire
