// api.cpp -- the C ABI of libire.so (include/ire.h): argument checks, exception -> status
// translation, thread-local error text, and the async batcher behind ire_submit/ire_poll.
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <deque>
#include <memory>
#include <thread>

#include <pthread.h>
#include <sched.h>

#include <cstdlib>

#include "affinity.hpp"
#include "batcher.hpp"
#include "engine.hpp"
#include "fusion.hpp"
#include "strips.hpp"

namespace ire {

static thread_local std::string g_last_error;
void set_last_error(int code, const std::string& msg) { (void)code; g_last_error = msg; }

// ---- async batcher (batcher.hpp): the state machine is a template over its backend; this file provides the HIP one -------

// One engine call = one critical section on the host (mutex) AND on the GPU (Engine::enter/leave): the caller's stream first
// waits for the previous call's completion event, so calls from several threads / streams never interleave kernels on
// the shared workspaces.  leave() also runs when f throws: whatever was enqueued before the failure stays fenced.
template <typename F>
static void on_stream(Engine& E, hipStream_t s, F&& f) {
    std::lock_guard<std::mutex> lk(E.mutex());
    E.enter(s);
    try { f(); } catch (...) { E.leave(s); throw; }
    E.leave(s);
}

struct DeviceGuard {       // staging is allocated on first use of a shape, possibly from a caller's thread: leave that thread's current device as it was
    int prev = -1;
    explicit DeviceGuard(int dev) { (void)hipGetDevice(&prev); (void)hipSetDevice(dev); }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

// the five events of a slot: created together, destroyed together
struct SlotEvents {
    hipEvent_t in = nullptr, c0 = nullptr, c1 = nullptr, cw = nullptr, out = nullptr;
    // c1 and cw mark the same point (the batch's compute is done): the launcher QUERIES c1 under the batcher's lock while
    // the completer SLEEPS on cw -- hipEventSynchronize holds the event's own lock for as long as it waits, so a query of the
    // same event from another thread blocks until the batch is done (measured: with one event for both, every submitter stalled
    // behind the launcher for a whole batch and a 16-deep closed loop fell to batches of one, 464 img/s)
    void create() {       // c0 .. c1 is timed
        for (hipEvent_t* e : {&c0, &c1}) IRE_HIP(hipEventCreate(e));
        for (hipEvent_t* e : {&in, &cw, &out}) IRE_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
    }
    ~SlotEvents() { for (hipEvent_t e : {in, c0, c1, cw, out}) if (e) (void)hipEventDestroy(e); }
};
// the backend's side of a slot: its staging (device_buf.hpp; SlotBufs holds views of the pinned half) and its events
struct HipSlot : SlotMem<DeviceMem, PinnedMem> {
    std::unique_ptr<SlotEvents> ev;
    // file jobs: one status word per job from the device's JPEG decoder, and their way back with the batch
    Buf<DeviceMem> d_fstat;
    Buf<PinnedMem> pin_fstat;
    int file_jobs = 0;         // jobs decoded into d_in since the slot opened; 0: a slot of pixel jobs
};

// what a file job keeps of its file between submit and its batch's decode: the head as parsed, the scan's streams as cut
struct FileHead { bool png = false; };
struct JpegFileHead : FileHead {
    jpegparse::File hd;
    std::vector<jpegdec::DecStream> streams;
    std::unique_ptr<icc::Transform> icc;      // an upload on an engine with IRE_FLAG_UPLOAD_ICC whose profile needs a transform; else null
};

// a PNG job's: the plan; the staged input is the IDAT payloads back to back, one zlib stream
struct PngFileHead : FileHead {
    pngparse::File f;
    PngFileHead() { png = true; }
};
static const FileHead& head_of(const void* head) { return *static_cast<const FileHead*>(head); }

// CPU set of this engine's service threads (affinity.hpp): IRE_CPU_AFFINITY = "off" | a cpulist overrides the sysfs plan
static CpuPlan plan_for_device(int device) {
    CpuPlan p;
    const char* env = std::getenv("IRE_CPU_AFFINITY");
    if (env && (!std::strcmp(env, "off") || !std::strcmp(env, "0"))) return p;
    char bdf[64] = {0};
    if (hipDeviceGetPCIBusId(bdf, sizeof(bdf), device) == hipSuccess) p = affinity_plan("/sys", bdf);
    if (env && env[0]) { const auto r = parse_cpulist(env); if (!r.empty()) p.ranges = r; return p; }
    // A container's cpuset (a job that was given 16 of the host's CPUs) outranks the plan: only the planned CPUs this process may
    // run on count, and a share of fewer than four of them (launcher + completer + the host's own waiter threads would queue behind
    // each other) is no plan at all -- the threads then stay wherever the scheduler is allowed to put them.
    cpu_set_t allowed;
    CPU_ZERO(&allowed);
    if (sched_getaffinity(0, sizeof(allowed), &allowed) == 0) {
        std::vector<std::pair<int, int>> keep;
        int n = 0;
        for (int c : p.cpus())
            if (c >= 0 && c < CPU_SETSIZE && CPU_ISSET(c, &allowed)) {
                if (!keep.empty() && keep.back().second == c - 1) keep.back().second = c; else keep.emplace_back(c, c);
                ++n;
            }
        if (n < 4) keep.clear();
        p.ranges = keep;
    }
    return p;
}

static void bind_this_thread(const CpuPlan& p) {
    const auto cpus = p.cpus();
    if (cpus.empty()) return;
    cpu_set_t set;
    CPU_ZERO(&set);
    for (int c : cpus) if (c >= 0 && c < CPU_SETSIZE) CPU_SET(c, &set);
    (void)pthread_setaffinity_np(pthread_self(), sizeof(set), &set);      // (a cpuset that excludes them all: EINVAL, the thread stays where it was)
}

static_assert(kGroupMaxJobs == kFuseMaxSets, "a full fusion slot must be one fused launch");
struct HipBatchBackend {
    Engine& E;
    int device;
    CpuPlan plan;
    hipStream_t cs = nullptr, os = nullptr;      // copy-in | copy-out
    const TextFormat* const fmt;                 // the results' format (codec.hpp); null: pixels
    HipBatchBackend(Engine& e, int dev) : E(e), device(dev), plan(plan_for_device(dev)), fmt(e.result_format()) {}
    ~HipBatchBackend() {
        DeviceGuard g(device);
        if (cs) { (void)hipStreamSynchronize(cs); (void)hipStreamDestroy(cs); }
        if (os) { (void)hipStreamSynchronize(os); (void)hipStreamDestroy(os); }
    }
    int max_batch() const { return E.max_batch(); }
    // a result's place in the staging: the pixels, the stored PNG's text, or [uint64 count | the compressed PNG's or the JPEG's text, bound-sized]
    size_t out_bytes(int h, int w) const { return fmt ? fmt->place_bytes(h, w) : (size_t)h * w * 3; }
    // only a text of data-dependent length is shorter than its place
    const uint8_t* result_view(const uint8_t* place, int h, int w, size_t* len) const {
        if (!fmt || !fmt->counted) { *len = out_bytes(h, w); return place; }
        uint64_t n = 0;
        std::memcpy(&n, place, 8);
        *len = (size_t)std::min<uint64_t>(n, fmt->bound(h, w));
        return place + 8;
    }
    void start() {
        DeviceGuard g(device);
        if (!cs) IRE_HIP(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
        if (!os) IRE_HIP(hipStreamCreateWithFlags(&os, hipStreamNonBlocking));
    }
    void thread_enter(const char*) { (void)hipSetDevice(device); bind_this_thread(plan); }
    // Everything new is complete before the slot is touched: a failure half way (out of pinned memory at the fifth slot) leaves the
    // slot exactly as it was -- usable at its old capacity, or empty.
    void reserve(SlotBufs& b, size_t bytes, int mb) {
        if (b.fixed && bytes <= b.cap) return;
        DeviceGuard g(device);
        std::unique_ptr<HipSlot> fresh(b.impl ? nullptr : new HipSlot());
        HipSlot& hs = b.impl ? *static_cast<HipSlot*>(b.impl) : *fresh;
        std::unique_ptr<SlotEvents> ev(b.fixed ? nullptr : new SlotEvents());
        if (ev) ev->create();
        hs.reserve(bytes, mb, fmt != nullptr);        // the strong guarantee is SlotMem's
        if (ev) hs.ev = std::move(ev);        // (nothing from here on throws)
        if (fresh) b.impl = fresh.release();
        b.pin_in = hs.pin_in.get<uint8_t>(); b.pin_out = hs.pin_out.get<uint8_t>(); b.pin_jp = hs.pin_jp.get<uint8_t>();
        b.pin_sc = hs.pin_sc.get<double>(); b.pin_sc_in = hs.pin_sc_in.get<double>(); b.cap = hs.cap; b.fixed = hs.fixed;
    }
    void release(SlotBufs& b) noexcept {
        DeviceGuard g(device);
        delete static_cast<HipSlot*>(b.impl);
        b = SlotBufs{};
    }
    // ---- file jobs (batcher.hpp: the decoded kinds' hooks).  The parse and the cut run in the submitting thread; the launcher only packs
    // the records of the jobs staged so far and enqueues the decode on the copy-in stream, under the previous batch's compute. ----
    // (every head leaves as a shared_ptr<FileHead>, so the void* the batcher hands back points at the FileHead)
    std::shared_ptr<void> file_plan(const uint8_t* file, size_t bytes, int* h, int* w, size_t* room) { return plan_head(file, bytes, 0, h, w, room); }
    std::shared_ptr<FileHead> plan_head(const uint8_t* file, size_t bytes, uint32_t png_flags, int* h, int* w, size_t* room) {
        std::string why;
        if (E.png_decoder().enabled() && pngparse::is_png(file, bytes)) {      // (an engine without the flag goes on and refuses it as a JPEG parser does)
            auto head = std::make_shared<PngFileHead>();
            if (!pngparse::plan_file(file, bytes, png_flags | E.png_decoder().accept(), head->f, why)) fail(IRE_ERR_INVALID_INPUT, why);
            *h = head->f.h; *w = head->f.w;
            *room = head->f.idat_bytes;
            return head;
        }
        auto head = std::make_shared<JpegFileHead>();
        if (!jpegparse::plan_file(file, bytes, E.jpeg_decoder().accept(), head->hd, why)) fail(IRE_ERR_INVALID_INPUT, why);
        *h = head->hd.hd.im.h; *w = head->hd.hd.im.w;
        *room = jpegparse::file_room(head->hd, bytes);
        return head;
    }
    size_t file_stage(void* head, const uint8_t* file, size_t bytes, uint8_t* dst, size_t room) {
        std::string why;
        if (head_of(head).png) {
            const size_t used = pngparse::stage(static_cast<PngFileHead*>(static_cast<FileHead*>(head))->f, file, bytes, dst, room, why);
            if (!used) fail(IRE_ERR_INVALID_INPUT, why);
            return used;
        }
        JpegFileHead& f = *static_cast<JpegFileHead*>(static_cast<FileHead*>(head));
        f.streams.assign(f.hd.nstreams, jpegdec::DecStream{});
        if (!jpegparse::split_file(f.hd, file, bytes, dst, room, f.streams.data(), why)) fail(IRE_ERR_INVALID_INPUT, why);
        const jpegdec::DecStream& last = f.streams.back();
        return std::max<size_t>((size_t)last.off + last.len, 1);      // (0 would say that nothing was staged: a last scan of no bytes)
    }
    // A file job is decoded straight into the slot's device input.  An upload job is decoded at its STORED size into the engine's scratch,
    // then oriented and fitted into the slot's device input by one batched preprocess.  Either way all on the copy-in stream, under the
    // previous batch's compute.
    void decode(SlotBufs& b, int first, int count, const SlotKey& key, void* const* heads, const size_t* used) {
        HipSlot& hs = *static_cast<HipSlot*>(b.impl);
        const int h = key.h, w = key.w;
        const size_t ib = key.in_bytes();
        if (key.kind != JobKind::Upload) { decode_runs(hs, b, first, count, ib, h, w, hs.d_in.get<uint8_t>(), ib, heads, used); return; }
        const int sh = key.up[0], sw = key.up[1];
        const size_t sb = (size_t)sh * sw * 3;
        PreprocessScratch& P = E.preprocess_uploads();
        // the any-size staging rule (ire.h): for max_batch images while that is <= 256 MB, else for the batch at hand
        P.d_stored.grow(sb * (size_t)(first + count), batch_room(sb * (size_t)(first + count), sb * (size_t)E.max_batch()));
        decode_runs(hs, b, first, count, ib, sh, sw, P.d_stored.get<uint8_t>(), sb, heads, used);
        // the file's ICC profile, as sharp honours it: before the resize.  Every job brings its own tables (the profile is no part of the
        // key); a push in which no job has any enqueues nothing.
        if (E.upload_icc()) {
            const icc::Transform* t[kMaxBatch];
            for (int i = 0; i < count; ++i) t[i] = used[i] && !head_of(heads[i]).png ? static_cast<const JpegFileHead*>(&head_of(heads[i]))->icc.get() : nullptr;
            E.icc_converter().to_srgb_device(true, P.d_stored.get<uint8_t>() + sb * (size_t)first, count, sh, sw, sb, t, cs);
        }
        // (a job with nothing decoded is fitted from whatever the scratch held: it fails alone, its place is never read)
        E.preprocess_batch_device(P, P.d_stored.get<uint8_t>() + sb * (size_t)first, count, sh, sw, sb, key.up[2], key.up[3], hs.d_in.get<uint8_t>() + ib * (size_t)first, h, w, ib, cs);
    }
    // jobs first .. first + count - 1 of the slot, their staged bytes `place` apart in pin_in, decoded to h x w images `pitch` apart in d_rgb
    void decode_runs(HipSlot& hs, SlotBufs& b, int first, int count, size_t place, int h, int w, uint8_t* d_rgb, size_t pitch, void* const* heads, const size_t* used) {
        if (!hs.d_fstat) {                // zeroed once: the word of a job with nothing to decode is never written
            hs.d_fstat = Buf<DeviceMem>(sizeof(int32_t) * kMaxBatch, BufUse::Persistent); hs.pin_fstat = Buf<PinnedMem>(sizeof(int32_t) * kMaxBatch, BufUse::Persistent);
            IRE_HIP(hipMemsetAsync(hs.d_fstat.get<int32_t>(), 0, sizeof(int32_t) * kMaxBatch, cs));
            std::memset(hs.pin_fstat.get<int32_t>(), 0, sizeof(int32_t) * kMaxBatch);
        }
        const jpegparse::File* hd[kMaxBatch];
        const jpegdec::DecStream* streams[kMaxBatch];
        const uint8_t* bytes[kMaxBatch];
        size_t room[kMaxBatch];
        hs.file_jobs = first + count;
        // the PNG jobs of the push, wherever they stand among the others: ONE call, every file to its own image and status word
        {
            const pngparse::File* pf[kMaxBatch];
            int dst[kMaxBatch], n = 0;
            for (int i = 0; i < count; ++i)
                if (used[i] && head_of(heads[i]).png) {
                    pf[n] = &static_cast<const PngFileHead*>(&head_of(heads[i]))->f; bytes[n] = b.pin_in + place * (size_t)(first + i); room[n] = used[i]; dst[n] = first + i;
                    ++n;
                }
            if (n) E.png_decoder().decode_staged(pf, bytes, room, dst, n, h, w, d_rgb, pitch, hs.d_fstat.get<int32_t>(), cs);
        }
        // and the JPEG jobs likewise: one call per kind, whatever the number of jobs and however the kinds interleave.  A job whose staging
        // failed (batcher.hpp) has nothing to decode: its place keeps whatever the slot held, its job fails alone.
        {
            int dst[kMaxBatch], n = 0;
            for (int i = 0; i < count; ++i)
                if (used[i] && !head_of(heads[i]).png) {
                    const JpegFileHead& f = *static_cast<const JpegFileHead*>(&head_of(heads[i]));
                    hd[n] = &f.hd; streams[n] = f.streams.data(); bytes[n] = b.pin_in + place * (size_t)(first + i); room[n] = used[i]; dst[n] = first + i;
                    ++n;
                }
            if (n) E.jpeg_decoder().decode_streams(hd, streams, bytes, room, n, h, w, d_rgb, pitch, hs.d_fstat.get<int32_t>(), cs, dst);
        }
    }
    // file_plan for an upload job: the FITTED size, and the key that says how decode gets there
    std::shared_ptr<void> upload_plan(const uint8_t* file, size_t bytes, int max_dim, int* h, int* w, size_t* room, int key[4]) {
        int sh = 0, sw = 0;
        // (a PNG's iCCP on an engine that honours profiles: refused, reading the chunk is a later change)
        auto head = plan_head(file, bytes, E.upload_icc() ? pngparse::kRefuseIccp : 0u, &sh, &sw, room);
        if (head->png) {
            key[0] = sh; key[1] = sw; key[2] = static_cast<PngFileHead*>(head.get())->f.orientation; key[3] = max_dim;
            preprocess_plan(sw, sh, key[2], max_dim, w, h, nullptr);
            if (!piece_addressable(Engine::fit_dim(*h), Engine::fit_dim(*w), 0)) fail(IRE_ERR_INVALID_INPUT, not_addressable(Engine::fit_dim(*h), Engine::fit_dim(*w)));
            return head;
        }
        if (E.upload_icc()) {
            icc::Transform t;
            std::string why;
            if (!icc::plan_file(file, bytes, t, why)) fail(IRE_ERR_INVALID_INPUT, why);
            if (t.kind == icc::kMatrix || t.kind == icc::kGrey) static_cast<JpegFileHead*>(head.get())->icc.reset(new icc::Transform(t));
        }
        key[0] = sh; key[1] = sw; key[2] = jpegparse::file_orientation(file, bytes); key[3] = max_dim;
        preprocess_plan(sw, sh, key[2], max_dim, w, h, nullptr);
        if (!piece_addressable(Engine::fit_dim(*h), Engine::fit_dim(*w), 0)) fail(IRE_ERR_INVALID_INPUT, not_addressable(Engine::fit_dim(*h), Engine::fit_dim(*w)));
        return head;
    }
    int file_status(SlotBufs& b, int i) { return static_cast<HipSlot*>(b.impl)->pin_fstat.get<int32_t>()[i]; }
    void h2d(SlotBufs& b, size_t off, size_t bytes) {
        HipSlot& hs = *static_cast<HipSlot*>(b.impl);
        hs.file_jobs = 0;
        IRE_HIP(hipMemcpyAsync(hs.d_in.get<uint8_t>() + off, b.pin_in + off, bytes, hipMemcpyHostToDevice, cs));
    }
    // n jobs of one image (key.k == 0) or of k views, one fused result per job: n results, n rows of scores (a fusion job's: its view 0's)
    void launch(SlotBufs& b, int n, const SlotKey& key, const uint8_t* has_sc) {
        HipSlot& hs = *static_cast<HipSlot*>(b.impl);
        const int k = key.k, h = key.h, w = key.w;
        IRE_HIP(hipMemcpyAsync(hs.d_jp.get<uint8_t>(), b.pin_jp, (size_t)n * (size_t)key.images_per_job(), hipMemcpyHostToDevice, cs));
        IRE_HIP(hipEventRecord(hs.ev->in, cs));
        hipStream_t ms = E.main_stream();
        on_stream(E, ms, [&] {
            IRE_HIP(hipStreamWaitEvent(ms, hs.ev->in, 0));
            IRE_HIP(hipEventRecord(hs.ev->c0, ms));
            // classifies the jobs that brought no scores; a shape the network cannot take as it is (ire_submit_fit) is padded into the
            // engine's staging and its window comes back; with a text format the results leave the device as text
            if (k) {
                E.restore_fuse_fit_device_mixed(hs.d_in.get<uint8_t>(), n, k, h, w, b.pin_sc_in, has_sc, hs.d_jp.get<uint8_t>(), hs.d_out.get<uint8_t>(), fmt ? hs.d_txt.get<uint8_t>() : nullptr, (out_bytes(h, w) + 255) / 256 * 256, ms);
                IRE_HIP(hipMemcpy2DAsync(b.pin_sc, sizeof(double) * 7, E.scores_device(), sizeof(double) * 7 * k, sizeof(double) * 7, (size_t)n, hipMemcpyDeviceToHost, ms));      // view 0 of every job
            } else {
                E.restore_fit_device_mixed(hs.d_in.get<uint8_t>(), n, h, w, b.pin_sc_in, has_sc, hs.d_jp.get<uint8_t>(), hs.d_out.get<uint8_t>(), fmt ? hs.d_txt.get<uint8_t>() : nullptr, (out_bytes(h, w) + 255) / 256 * 256, ms);
                IRE_HIP(hipMemcpyAsync(b.pin_sc, E.scores_device(), sizeof(double) * 7 * n, hipMemcpyDeviceToHost, ms));
            }
            if (hs.file_jobs) IRE_HIP(hipMemcpyAsync(hs.pin_fstat.get<int32_t>(), hs.d_fstat.get<int32_t>(), sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, ms));
            hs.file_jobs = 0;
            IRE_HIP(hipEventRecord(hs.ev->c1, ms));
            IRE_HIP(hipEventRecord(hs.ev->cw, ms));
        });
        IRE_HIP(hipStreamWaitEvent(os, hs.ev->c1, 0));
        if (fmt) {
            const size_t ob = out_bytes(h, w), st = (ob + 255) / 256 * 256;
            for (int i = 0; i < n; ++i) IRE_HIP(hipMemcpyAsync(b.pin_out + ob * i, hs.d_txt.get<uint8_t>() + st * i, ob, hipMemcpyDeviceToHost, os));
        } else IRE_HIP(hipMemcpyAsync(b.pin_out, hs.d_out.get<uint8_t>(), out_bytes(h, w) * n, hipMemcpyDeviceToHost, os));
        IRE_HIP(hipEventRecord(hs.ev->out, os));
    }
    bool computing(SlotBufs& b) noexcept { return hipEventQuery(static_cast<HipSlot*>(b.impl)->ev->c1) == hipErrorNotReady; }
    void wait_compute(SlotBufs& b) noexcept { (void)hipEventSynchronize(static_cast<HipSlot*>(b.impl)->ev->cw); }
    void wait_done(SlotBufs& b, ire_timings& t) {
        HipSlot& hs = *static_cast<HipSlot*>(b.impl);
        const hipError_t rc = hipEventSynchronize(hs.ev->out);
        if (rc != hipSuccess) throw Error{IRE_ERR_INTERNAL, std::string("internal: ") + hipGetErrorString(rc)};
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, hs.ev->c0, hs.ev->c1) == hipSuccess) { t.restore_ms = ms; t.total_ms = ms; }
    }
    void drain() noexcept {
        DeviceGuard g(device);
        if (cs) (void)hipStreamSynchronize(cs);
        (void)hipStreamSynchronize(E.main_stream());
        if (os) (void)hipStreamSynchronize(os);
    }
};

}  // namespace ire

struct ire_job { std::shared_ptr<ire::Job> j; };
// A strip session belongs to an engine: ire_shutdown and ire_load_weights must not pull the engine (or its layer program)
// from under an open session.  The engine keeps a registry of its open sessions; shutdown closes their inner objects (the
// caller's handle stays valid as an empty shell: every later call on it returns IRE_ERR_INVALID_INPUT "invalid strip
// session handle" and ire_strips_close only frees the shell), load_weights refuses while sessions are open.
struct ire_strips { std::unique_ptr<ire::StripSession> s; ire_engine* owner = nullptr; };
static std::mutex g_strips_mu;       // guards every ire_engine::sessions list and every ire_strips::s / owner

struct ire_engine {
    std::unique_ptr<ire::Engine> eng;
    std::unique_ptr<ire::HipBatchBackend> backend;                  // (declared before the batcher: destroyed after it)
    std::unique_ptr<ire::Batcher<ire::HipBatchBackend>> batcher;
    int device = 0;
    std::vector<ire_strips*> sessions;     // open strip sessions (g_strips_mu)
    ~ire_engine();
};

ire_engine::~ire_engine() {
    batcher.reset();          // launches what is gathered, completes what is in flight, frees the staging
    backend.reset();
    std::lock_guard<std::mutex> lk(g_strips_mu);
    for (ire_strips* s : sessions) {       // invalidate: the StripSession dies with its engine, the caller's shell survives
        if (eng) { std::lock_guard<std::mutex> lk2(eng->mutex()); s->s.reset(); } else s->s.reset();
        s->owner = nullptr;
    }
    sessions.clear();
}

namespace ire {

template <typename F>
static int guarded(F&& f) {
    try {
        f();
        return IRE_OK;
    } catch (const Error& e) {
        set_last_error(e.code, e.msg);
        return e.code;
    } catch (const std::bad_alloc&) {
        set_last_error(IRE_ERR_UNAVAILABLE, "service unavailable: out of host memory");
        return IRE_ERR_UNAVAILABLE;
    } catch (const std::exception& e) {
        set_last_error(IRE_ERR_INTERNAL, std::string("internal: ") + e.what());
        return IRE_ERR_INTERNAL;
    }
}

static Engine& eng(ire_engine* e) {
    if (!e || !e->eng) fail(IRE_ERR_INVALID_INPUT, "invalid engine handle");
    return *e->eng;
}

static int family_id(const char* f) {
    if (!f) fail(IRE_ERR_INVALID_INPUT, "invalid family");
    const char* names[] = {"classifier", "conv3x3", "conv1x1", "stem", "head", "gn_finalize", "fusion"};
    for (int i = 0; i < 7; ++i) if (!std::strcmp(f, names[i])) return i;
    if (!std::strcmp(f, "all")) return -1;
    fail(IRE_ERR_INVALID_INPUT, "invalid family name");
}

}  // namespace ire

// behind every ire_submit*, after its argument checks: the job that `submit` queues in the batcher, wrapped in a handle
template <typename F>
static void job_handle(ire_job** job_out, F&& submit) {
    *job_out = nullptr;
    std::unique_ptr<ire_job> hnd(new ire_job{});
    hnd->j = submit();
    *job_out = hnd.release();
}

using namespace ire;

extern "C" {

int ire_abi_version(void) { return IRE_ABI_VERSION; }

const char* ire_last_error(void) { return g_last_error.c_str(); }

int ire_init(const ire_config* cfg, ire_engine** out) {
    return guarded([&] {
        if (!cfg || !out) fail(IRE_ERR_INVALID_INPUT, "invalid arguments to ire_init");
        // the struct as it was before jpeg_quality and jpeg_sampling (flags was its last member; 4 bytes of padding behind it, which is
        // where jpeg_quality now lies: the two fields are read only from a caller whose size covers both)
        constexpr size_t kSizeBeforeJpeg = (offsetof(ire_config, flags) + sizeof(uint32_t) + alignof(ire_config) - 1) / alignof(ire_config) * alignof(ire_config);
        static_assert(kSizeBeforeJpeg == 40 && sizeof(ire_config) == 48 && offsetof(ire_config, jpeg_quality) == 36, "ire_config's layout");
        if (cfg->struct_size < kSizeBeforeJpeg) fail(IRE_ERR_INVALID_INPUT, "invalid ire_config.struct_size");
        ire_config c{};
        std::memcpy(&c, cfg, cfg->struct_size < sizeof(ire_config) ? kSizeBeforeJpeg : sizeof(ire_config));
        if (cfg->struct_size < sizeof(ire_config)) c.jpeg_quality = c.jpeg_sampling = 0;
        cfg = &c;
        check_config_flags(cfg->flags);       // (before any device is touched)
        (void)check_config_jpeg(cfg->flags, cfg->jpeg_quality, cfg->jpeg_sampling);
        *out = nullptr;
        std::unique_ptr<ire_engine> E(new ire_engine());
        E->eng.reset(new Engine(*cfg));
        E->device = cfg->device_index;
        E->backend.reset(new HipBatchBackend(*E->eng, E->device));
        E->batcher.reset(new Batcher<HipBatchBackend>(*E->backend));
        *out = E.release();
    });
}

void ire_shutdown(ire_engine* e) { delete e; }

int ire_load_weights(ire_engine* e, const void* blob, size_t bytes) {
    return guarded([&] {
        Engine& E = eng(e);
        if (!blob) fail(IRE_ERR_INVALID_INPUT, "invalid weight blob");
        {
            std::lock_guard<std::mutex> lk(g_strips_mu);     // a session walks the layer program op by op: it must not change under it
            if (!e->sessions.empty()) fail(IRE_ERR_INVALID_INPUT, "invalid call: ire_load_weights while strip sessions are open (close them first)");
        }
        std::lock_guard<std::mutex> lk(E.mutex());
        E.load_weights(blob, bytes);
    });
}

int ire_max_batch_for(ire_engine* e, int h, int w) {
    if (!e || !e->eng) return 0;
    std::lock_guard<std::mutex> lk(e->eng->mutex());
    return e->eng->capacity_for(h, w);
}

int ire_classify(ire_engine* e, const uint8_t* rgb, int n, int h, int w, int row_stride, const uint8_t* is_jpeg,
                 double* scores_out, int32_t* label_out) {
    return guarded([&] {
        Engine& E = eng(e);
        on_stream(E, E.main_stream(), [&] { E.classify_host(rgb, n, h, w, row_stride, is_jpeg, scores_out, label_out); });
    });
}

int ire_restore(ire_engine* e, const uint8_t* rgb, int n, int h, int w, const double* scores, const uint8_t* is_jpeg,
                uint8_t* out_rgb, ire_timings* t) {
    return guarded([&] {
        Engine& E = eng(e);
        on_stream(E, E.main_stream(), [&] { E.restore_host(rgb, n, h, w, scores, is_jpeg, out_rgb, t); });
    });
}

int ire_fuse(ire_engine* e, const uint8_t* rgb_views, int k, int h, int w, double noise_score, uint8_t* out_rgb,
             int32_t* shifts_out, ire_timings* t) {
    return guarded([&] {
        Engine& E = eng(e);
        on_stream(E, E.main_stream(), [&] { fuse_host(E, rgb_views, k, h, w, noise_score, out_rgb, shifts_out, t); });
    });
}

int ire_classify_device(ire_engine* e, const uint8_t* d_rgb, int n, int h, int w, const uint8_t* d_is_jpeg,
                        double* d_scores, int32_t* d_label, void* stream) {
    return guarded([&] {
        Engine& E = eng(e);
        on_stream(E, (hipStream_t)stream, [&] { E.classify_device(d_rgb, n, h, w, d_is_jpeg, d_scores, d_label, (hipStream_t)stream); });
    });
}

int ire_restore_device(ire_engine* e, const uint8_t* d_rgb, int n, int h, int w, const double* d_scores,
                       const uint8_t* d_is_jpeg, uint8_t* d_out_rgb, void* stream) {
    return guarded([&] {
        Engine& E = eng(e);
        on_stream(E, (hipStream_t)stream, [&] { E.restore_device(d_rgb, n, h, w, d_scores, d_is_jpeg, d_out_rgb, (hipStream_t)stream); });
    });
}

int ire_fuse_device(ire_engine* e, const uint8_t* d_rgb_views, int k, int h, int w, double noise_score,
                    uint8_t* d_out_rgb, int32_t* d_shifts, void* stream) {
    return guarded([&] {
        Engine& E = eng(e);
        on_stream(E, (hipStream_t)stream, [&] { fuse_device(E, d_rgb_views, k, h, w, noise_score, d_out_rgb, d_shifts, (hipStream_t)stream); });
    });
}

int ire_fuse_batch_device(ire_engine* e, const uint8_t* d_rgb_views, int nsets, int k, int h, int w, const double* noise_scores,
                          uint8_t* d_out_rgb, int32_t* d_shifts, void* stream) {
    return guarded([&] {
        Engine& E = eng(e);
        on_stream(E, (hipStream_t)stream, [&] { fuse_batch_device(E, d_rgb_views, nsets, k, h, w, noise_scores, d_out_rgb, d_shifts, (hipStream_t)stream); });
    });
}

int ire_preprocess_plan(int width, int height, int orientation, int max_dim, int* out_w, int* out_h, int* resized) {
    return guarded([&] {
        if (!out_w || !out_h) fail(IRE_ERR_INVALID_INPUT, "invalid arguments to ire_preprocess_plan");
        preprocess_plan(width, height, orientation, max_dim, out_w, out_h, resized);
    });
}

int ire_preprocess(ire_engine* e, const uint8_t* rgb, int h, int w, int orientation, int max_dim, uint8_t* out_rgb, int out_h,
                   int out_w) {
    return guarded([&] {
        Engine& E = eng(e);
        on_stream(E, E.main_stream(), [&] { E.preprocess_host(rgb, h, w, orientation, max_dim, out_rgb, out_h, out_w); });
    });
}

int ire_preprocess_device(ire_engine* e, const uint8_t* d_rgb, int h, int w, int orientation, int max_dim, uint8_t* d_out_rgb,
                          int out_h, int out_w, void* stream) {
    return guarded([&] {
        Engine& E = eng(e);
        on_stream(E, (hipStream_t)stream, [&] { E.preprocess_device(d_rgb, h, w, orientation, max_dim, d_out_rgb, out_h, out_w, (hipStream_t)stream); });
    });
}

int ire_preprocess_batch_device(ire_engine* e, const uint8_t* d_rgb, int n, int h, int w, size_t image_pitch_bytes, int orientation, int max_dim, uint8_t* d_out_rgb,
                                int out_h, int out_w, size_t out_image_pitch_bytes, void* stream) {
    return guarded([&] {
        Engine& E = eng(e);
        on_stream(E, (hipStream_t)stream, [&] {
            E.preprocess_batch_device(E.preprocess_own(), d_rgb, n, h, w, image_pitch_bytes, orientation, max_dim, d_out_rgb, out_h, out_w, out_image_pitch_bytes, (hipStream_t)stream);
        });
    });
}

int ire_upload_plan(const uint8_t* file, size_t bytes, uint32_t accept, int max_dim, int* stored_h, int* stored_w, int* orientation, int* out_h, int* out_w) {
    return guarded([&] {
        if (!file) fail(IRE_ERR_INVALID_INPUT, "invalid arguments to ire_upload_plan: null file");
        if (accept & ~(uint32_t)(IRE_DECODE_ACCEPT_PROGRESSIVE | IRE_DECODE_ACCEPT_ICC | IRE_DECODE_ACCEPT_PNG | IRE_DECODE_ACCEPT_PNG_ALL)) fail(IRE_ERR_INVALID_INPUT, "invalid arguments to ire_upload_plan: unknown accept bits");
        if ((accept & IRE_DECODE_ACCEPT_PNG_ALL) && !(accept & IRE_DECODE_ACCEPT_PNG)) fail(IRE_ERR_INVALID_INPUT, "invalid arguments to ire_upload_plan: IRE_DECODE_ACCEPT_PNG_ALL set without IRE_DECODE_ACCEPT_PNG");
        jpegparse::File f;
        std::string why;
        if ((accept & IRE_DECODE_ACCEPT_PNG) && pngparse::is_png(file, bytes)) {
            pngparse::File p;
            if (!pngparse::plan_file(file, bytes, ((accept & IRE_DECODE_ACCEPT_ICC) ? pngparse::kRefuseIccp : 0u) | (accept & IRE_DECODE_ACCEPT_PNG_ALL), p, why)) fail(IRE_ERR_INVALID_INPUT, why);
            int ow = 0, oh = 0;
            preprocess_plan(p.w, p.h, p.orientation, max_dim, &ow, &oh, nullptr);
            if (!piece_addressable(Engine::fit_dim(oh), Engine::fit_dim(ow), 0)) fail(IRE_ERR_INVALID_INPUT, not_addressable(Engine::fit_dim(oh), Engine::fit_dim(ow)));
            if (p.idat_bytes > (size_t)oh * ow * 3) fail(IRE_ERR_INVALID_INPUT, kUploadRoomReason);
            if (stored_h) *stored_h = p.h;
            if (stored_w) *stored_w = p.w;
            if (orientation) *orientation = p.orientation;
            if (out_h) *out_h = oh;
            if (out_w) *out_w = ow;
            return;
        }
        if (!jpegparse::plan_file(file, bytes, accept & IRE_DECODE_ACCEPT_PROGRESSIVE, f, why)) fail(IRE_ERR_INVALID_INPUT, why);
        if (accept & IRE_DECODE_ACCEPT_ICC) {
            icc::Transform t;
            if (!icc::plan_file(file, bytes, t, why)) fail(IRE_ERR_INVALID_INPUT, why);
        }
        const int o = jpegparse::file_orientation(file, bytes);
        int ow = 0, oh = 0;
        preprocess_plan(f.hd.im.w, f.hd.im.h, o, max_dim, &ow, &oh, nullptr);
        if (!piece_addressable(Engine::fit_dim(oh), Engine::fit_dim(ow), 0)) fail(IRE_ERR_INVALID_INPUT, not_addressable(Engine::fit_dim(oh), Engine::fit_dim(ow)));
        if (jpegparse::file_room(f, bytes) > (size_t)oh * ow * 3) fail(IRE_ERR_INVALID_INPUT, kUploadRoomReason);
        if (stored_h) *stored_h = f.hd.im.h;
        if (stored_w) *stored_w = f.hd.im.w;
        if (orientation) *orientation = o;
        if (out_h) *out_h = oh;
        if (out_w) *out_w = ow;
    });
}

static_assert(sizeof(ire_icc_transform) == sizeof(icc::Transform) && offsetof(ire_icc_transform, lin) == offsetof(icc::Transform, lin) &&
              IRE_ICC_NONE == icc::kNone && IRE_ICC_IDENTITY == icc::kIdentity && IRE_ICC_MATRIX == icc::kMatrix && IRE_ICC_GREY == icc::kGrey, "ire.h and icc_parse.hpp");

int ire_icc_plan_profile(const uint8_t* profile, size_t bytes, int components, ire_icc_transform* out) {
    return guarded([&] {
        if (!profile || !out || (components != 1 && components != 3)) fail(IRE_ERR_INVALID_INPUT, "invalid arguments to ire_icc_plan_profile");
        std::string why;
        if (!icc::plan_profile(profile, bytes, components, *reinterpret_cast<icc::Transform*>(out), why)) fail(IRE_ERR_INVALID_INPUT, why);
    });
}

int ire_icc_plan_file(const uint8_t* file, size_t bytes, ire_icc_transform* out) {
    return guarded([&] {
        if (!file || !out) fail(IRE_ERR_INVALID_INPUT, "invalid arguments to ire_icc_plan_file");
        std::string why;
        if (!icc::plan_file(file, bytes, *reinterpret_cast<icc::Transform*>(out), why)) fail(IRE_ERR_INVALID_INPUT, why);
    });
}

int ire_icc_to_srgb_device(ire_engine* e, uint8_t* d_rgb, int n, int h, int w, size_t image_pitch_bytes, const ire_icc_transform* const* t, void* stream) {
    return guarded([&] {
        Engine& E = eng(e);
        on_stream(E, (hipStream_t)stream, [&] {
            E.icc_converter().to_srgb_device(false, d_rgb, n, h, w, image_pitch_bytes, reinterpret_cast<const icc::Transform* const*>(t), (hipStream_t)stream);
        });
    });
}

int ire_icc_to_srgb(ire_engine* e, uint8_t* rgb, int n, int h, int w, const ire_icc_transform* const* t) {
    return guarded([&] {
        Engine& E = eng(e);
        on_stream(E, E.main_stream(), [&] { E.icc_converter().to_srgb_host(rgb, n, h, w, reinterpret_cast<const icc::Transform* const*>(t), E.main_stream()); });
    });
}

size_t ire_png_base64_bytes(int h, int w) { return (h >= 1 && w >= 8 && w % 8 == 0 && h <= 16384 && w <= 16384) ? kStoredPng.bound(h, w) : 0; }

int ire_encode_png_base64_device(ire_engine* e, const uint8_t* d_rgb, int n, int h, int w, uint8_t* d_chars, size_t stride_bytes, void* stream) {
    return guarded([&] {
        Engine& E = eng(e);
        on_stream(E, (hipStream_t)stream, [&] { E.text_encoder().encode_png_aligned_device(d_rgb, n, h, w, d_chars, stride_bytes, (hipStream_t)stream); });
    });
}

int ire_encode_png_base64(ire_engine* e, const uint8_t* rgb, int n, int h, int w, uint8_t* chars, size_t stride_bytes) {
    return guarded([&] {
        Engine& E = eng(e);
        on_stream(E, E.main_stream(), [&] { E.text_encoder().encode_png_aligned_host(rgb, n, h, w, chars, stride_bytes); });
    });
}

size_t ire_png_base64_bytes_fit(int h, int w) { return (h >= 1 && w >= 1 && h <= 8192 && w <= 8192) ? kStoredPng.bound(h, w) : 0; }

int ire_encode_png_base64_fit_device(ire_engine* e, const uint8_t* d_rgb, int n, int h, int w, size_t row_pitch_bytes, size_t image_pitch_bytes,
                                     uint8_t* d_chars, size_t stride_bytes, void* stream) {
    return guarded([&] {
        Engine& E = eng(e);
        on_stream(E, (hipStream_t)stream, [&] { E.text_encoder().encode_device(kStoredPng, d_rgb, n, h, w, row_pitch_bytes, image_pitch_bytes, d_chars, stride_bytes, nullptr, (hipStream_t)stream); });
    });
}

int ire_encode_png_base64_fit(ire_engine* e, const uint8_t* rgb, int n, int h, int w, uint8_t* chars, size_t stride_bytes) {
    return guarded([&] {
        Engine& E = eng(e);
        on_stream(E, E.main_stream(), [&] { E.text_encoder().encode_host(kStoredPng, rgb, n, h, w, chars, stride_bytes, nullptr); });
    });
}

size_t ire_png_deflate_base64_bound(int h, int w) { return (h >= 1 && w >= 1 && h <= 8192 && w <= 8192) ? kDeflatePng.bound(h, w) : 0; }

int ire_encode_png_deflate_base64_fit_device(ire_engine* e, const uint8_t* d_rgb, int n, int h, int w, size_t row_pitch_bytes, size_t image_pitch_bytes,
                                             uint8_t* d_chars, size_t stride_bytes, uint64_t* d_lens, void* stream) {
    return guarded([&] {
        Engine& E = eng(e);
        on_stream(E, (hipStream_t)stream, [&] { E.text_encoder().encode_device(kDeflatePng, d_rgb, n, h, w, row_pitch_bytes, image_pitch_bytes, d_chars, stride_bytes, d_lens, (hipStream_t)stream); });
    });
}

int ire_encode_png_deflate_base64_fit(ire_engine* e, const uint8_t* rgb, int n, int h, int w, uint8_t* chars, size_t stride_bytes, uint64_t* lens) {
    return guarded([&] {
        Engine& E = eng(e);
        on_stream(E, E.main_stream(), [&] { E.text_encoder().encode_host(kDeflatePng, rgb, n, h, w, chars, stride_bytes, lens); });
    });
}

size_t ire_jpeg_base64_bound_ex(int h, int w, int quality, int sampling) {
    if (h < 1 || w < 1 || h > 8192 || w > 8192 || quality < 0 || quality > 100 || (sampling != 0 && sampling != 2)) return 0;
    return kJpeg.with(jpeg_settings_of(quality, sampling)).bound(h, w);
}

int ire_encode_jpeg_base64_fit_device_ex(ire_engine* e, const uint8_t* d_rgb, int n, int h, int w, size_t row_pitch_bytes, size_t image_pitch_bytes, uint8_t* d_chars,
                                         size_t stride_bytes, uint64_t* d_lens, int quality, int sampling, void* stream) {
    return guarded([&] {
        Engine& E = eng(e);
        const TextFormat f = kJpeg.with(jpeg_settings_of(quality, sampling));
        on_stream(E, (hipStream_t)stream, [&] { E.text_encoder().encode_device(f, d_rgb, n, h, w, row_pitch_bytes, image_pitch_bytes, d_chars, stride_bytes, d_lens, (hipStream_t)stream); });
    });
}

int ire_encode_jpeg_base64_fit_ex(ire_engine* e, const uint8_t* rgb, int n, int h, int w, uint8_t* chars, size_t stride_bytes, uint64_t* lens, int quality, int sampling) {
    return guarded([&] {
        Engine& E = eng(e);
        const TextFormat f = kJpeg.with(jpeg_settings_of(quality, sampling));
        on_stream(E, E.main_stream(), [&] { E.text_encoder().encode_host(f, rgb, n, h, w, chars, stride_bytes, lens); });
    });
}

// the same three with the image's own Huffman tables
size_t ire_jpeg_optimized_base64_bound(int h, int w, int quality, int sampling) {
    if (h < 1 || w < 1 || h > 8192 || w > 8192 || quality < 0 || quality > 100 || (sampling != 0 && sampling != 2)) return 0;
    return jpeg_format_of(jpeg_settings_of(quality, sampling, true)).bound(h, w);
}

int ire_encode_jpeg_optimized_base64_fit_device(ire_engine* e, const uint8_t* d_rgb, int n, int h, int w, size_t row_pitch_bytes, size_t image_pitch_bytes, uint8_t* d_chars,
                                                size_t stride_bytes, uint64_t* d_lens, int quality, int sampling, void* stream) {
    return guarded([&] {
        Engine& E = eng(e);
        const TextFormat f = jpeg_format_of(jpeg_settings_of(quality, sampling, true));
        on_stream(E, (hipStream_t)stream, [&] { E.text_encoder().encode_device(f, d_rgb, n, h, w, row_pitch_bytes, image_pitch_bytes, d_chars, stride_bytes, d_lens, (hipStream_t)stream); });
    });
}

int ire_encode_jpeg_optimized_base64_fit(ire_engine* e, const uint8_t* rgb, int n, int h, int w, uint8_t* chars, size_t stride_bytes, uint64_t* lens, int quality, int sampling) {
    return guarded([&] {
        Engine& E = eng(e);
        const TextFormat f = jpeg_format_of(jpeg_settings_of(quality, sampling, true));
        on_stream(E, E.main_stream(), [&] { E.text_encoder().encode_host(f, rgb, n, h, w, chars, stride_bytes, lens); });
    });
}

// the same three as a progressive file
size_t ire_jpeg_progressive_base64_bound(int h, int w, int quality, int sampling) {
    if (h < 1 || w < 1 || h > 8192 || w > 8192 || quality < 0 || quality > 100 || (sampling != 0 && sampling != 2)) return 0;
    return jpeg_format_of(jpeg_settings_of(quality, sampling, false, true)).bound(h, w);
}

int ire_encode_jpeg_progressive_base64_fit_device(ire_engine* e, const uint8_t* d_rgb, int n, int h, int w, size_t row_pitch_bytes, size_t image_pitch_bytes, uint8_t* d_chars,
                                                  size_t stride_bytes, uint64_t* d_lens, int quality, int sampling, void* stream) {
    return guarded([&] {
        Engine& E = eng(e);
        const TextFormat f = jpeg_format_of(jpeg_settings_of(quality, sampling, false, true));
        on_stream(E, (hipStream_t)stream, [&] { E.text_encoder().encode_device(f, d_rgb, n, h, w, row_pitch_bytes, image_pitch_bytes, d_chars, stride_bytes, d_lens, (hipStream_t)stream); });
    });
}

int ire_encode_jpeg_progressive_base64_fit(ire_engine* e, const uint8_t* rgb, int n, int h, int w, uint8_t* chars, size_t stride_bytes, uint64_t* lens, int quality, int sampling) {
    return guarded([&] {
        Engine& E = eng(e);
        const TextFormat f = jpeg_format_of(jpeg_settings_of(quality, sampling, false, true));
        on_stream(E, E.main_stream(), [&] { E.text_encoder().encode_host(f, rgb, n, h, w, chars, stride_bytes, lens); });
    });
}

int ire_debug_jpeg_progressive_from_coefs(ire_engine* e, const int16_t* coefs, int n, int h, int w, int quality, int sampling, uint8_t* out_files, size_t stride, uint64_t* lens) {
    return guarded([&] {
        Engine& E = eng(e);
        on_stream(E, E.main_stream(), [&] { E.text_encoder().debug_jpeg_progressive(coefs, n, h, w, quality, sampling, out_files, stride, lens); });
    });
}

int ire_debug_jpeg_huffman(ire_engine* e, const uint32_t* counts, int n, uint8_t* bits_vals_out, int32_t* nvals_out) {
    return guarded([&] {
        Engine& E = eng(e);
        on_stream(E, E.main_stream(), [&] { E.text_encoder().debug_jpeg_huffman(counts, n, bits_vals_out, nvals_out); });
    });
}

// the first three entries: the default settings of the three above
size_t ire_jpeg_base64_bound(int h, int w) { return ire_jpeg_base64_bound_ex(h, w, 0, 0); }

int ire_encode_jpeg_base64_fit_device(ire_engine* e, const uint8_t* d_rgb, int n, int h, int w, size_t row_pitch_bytes, size_t image_pitch_bytes, uint8_t* d_chars,
                                      size_t stride_bytes, uint64_t* d_lens, void* stream) {
    return ire_encode_jpeg_base64_fit_device_ex(e, d_rgb, n, h, w, row_pitch_bytes, image_pitch_bytes, d_chars, stride_bytes, d_lens, 0, 0, stream);
}

int ire_encode_jpeg_base64_fit(ire_engine* e, const uint8_t* rgb, int n, int h, int w, uint8_t* chars, size_t stride_bytes, uint64_t* lens) {
    return ire_encode_jpeg_base64_fit_ex(e, rgb, n, h, w, chars, stride_bytes, lens, 0, 0);
}

int ire_decode_jpeg_plan(const uint8_t* file, size_t bytes, int* out_h, int* out_w, int* out_sampling) {
    return guarded([&] {
        if (!file) fail(IRE_ERR_INVALID_INPUT, "invalid arguments to ire_decode_jpeg_plan: null file");
        jpegparse::Header hd;
        std::string why;
        if (!jpegparse::plan(file, bytes, hd, why)) fail(IRE_ERR_INVALID_INPUT, why);
        if (out_h) *out_h = hd.im.h;
        if (out_w) *out_w = hd.im.w;
        if (out_sampling) *out_sampling = hd.im.sampling;
    });
}

static_assert(IRE_DECODE_ACCEPT_PROGRESSIVE == jpegparse::kAcceptProgressive && IRE_DECODE_MAX_SCANS == jpegparse::kMaxScans, "ire.h and jpeg_parse.hpp");

int ire_decode_jpeg_plan_ex(const uint8_t* file, size_t bytes, uint32_t accept, int* out_h, int* out_w, int* out_sampling, int* out_nscans) {
    return guarded([&] {
        if (!file) fail(IRE_ERR_INVALID_INPUT, "invalid arguments to ire_decode_jpeg_plan: null file");
        if (accept & ~(uint32_t)IRE_DECODE_ACCEPT_PROGRESSIVE) fail(IRE_ERR_INVALID_INPUT, "invalid arguments to ire_decode_jpeg_plan_ex: unknown accept bits");
        jpegparse::File f;
        std::string why;
        if (!jpegparse::plan_file(file, bytes, accept, f, why)) fail(IRE_ERR_INVALID_INPUT, why);
        if (out_h) *out_h = f.hd.im.h;
        if (out_w) *out_w = f.hd.im.w;
        if (out_sampling) *out_sampling = f.hd.im.sampling;
        if (out_nscans) *out_nscans = (int)f.nscans();
    });
}

int ire_decode_jpeg(ire_engine* e, const uint8_t* file, size_t bytes, uint8_t* out_rgb, int h, int w) {
    return guarded([&] {
        Engine& E = eng(e);
        on_stream(E, E.main_stream(), [&] { E.jpeg_decoder().decode_host(file, bytes, out_rgb, h, w); });
    });
}

int ire_decode_jpeg_device(ire_engine* e, const uint8_t* const* files, const size_t* bytes, int n, int h, int w, uint8_t* d_rgb, size_t image_pitch_bytes,
                           int32_t* d_status, void* stream) {
    return guarded([&] {
        Engine& E = eng(e);
        on_stream(E, (hipStream_t)stream, [&] { E.jpeg_decoder().decode_files(files, bytes, n, h, w, d_rgb, image_pitch_bytes, d_status, (hipStream_t)stream); });
    });
}

static_assert(IRE_DECODE_ACCEPT_ICC == pngparse::kRefuseIccp, "ire.h and png_parse.hpp");
static_assert(IRE_DECODE_ACCEPT_PNG_ALL == pngparse::kAcceptAll, "ire.h and png_parse.hpp");

int ire_decode_png_plan(const uint8_t* file, size_t bytes, int* out_h, int* out_w, int* out_colour_type) {
    return guarded([&] {
        if (!file) fail(IRE_ERR_INVALID_INPUT, "invalid arguments to ire_decode_png_plan: null file");
        pngparse::File f;
        std::string why;
        if (!pngparse::plan_file(file, bytes, 0, f, why)) fail(IRE_ERR_INVALID_INPUT, why);
        if (out_h) *out_h = f.h;
        if (out_w) *out_w = f.w;
        if (out_colour_type) *out_colour_type = f.ctype;
    });
}

int ire_decode_png_plan_ex(const uint8_t* file, size_t bytes, uint32_t accept, int* out_h, int* out_w, int* out_colour_type, int* out_depth, int* out_interlace) {
    return guarded([&] {
        if (!file) fail(IRE_ERR_INVALID_INPUT, "invalid arguments to ire_decode_png_plan_ex: null file");
        if (accept & ~(uint32_t)IRE_DECODE_ACCEPT_PNG_ALL) fail(IRE_ERR_INVALID_INPUT, "invalid arguments to ire_decode_png_plan_ex: unknown accept bits");
        pngparse::File f;
        std::string why;
        if (!pngparse::plan_file(file, bytes, accept, f, why)) fail(IRE_ERR_INVALID_INPUT, why);
        if (out_h) *out_h = f.h;
        if (out_w) *out_w = f.w;
        if (out_colour_type) *out_colour_type = f.ctype;
        if (out_depth) *out_depth = f.depth;
        if (out_interlace) *out_interlace = f.interlace;
    });
}

int ire_decode_png(ire_engine* e, const uint8_t* file, size_t bytes, uint8_t* out_rgb, int h, int w) {
    return guarded([&] {
        Engine& E = eng(e);
        on_stream(E, E.main_stream(), [&] { E.png_decoder().decode_host(file, bytes, out_rgb, h, w); });
    });
}

int ire_decode_png_device(ire_engine* e, const uint8_t* const* files, const size_t* bytes, int n, int h, int w, uint8_t* d_rgb, size_t image_pitch_bytes,
                          int32_t* d_status, void* stream) {
    return guarded([&] {
        Engine& E = eng(e);
        on_stream(E, (hipStream_t)stream, [&] { E.png_decoder().decode_files(files, bytes, n, h, w, d_rgb, image_pitch_bytes, d_status, (hipStream_t)stream); });
    });
}

int ire_restore_fit(ire_engine* e, const uint8_t* rgb, int n, int h, int w, const double* scores, const uint8_t* is_jpeg, uint8_t* out_rgb,
                    ire_timings* t) {
    return guarded([&] {
        Engine& E = eng(e);
        on_stream(E, E.main_stream(), [&] { E.restore_fit_host(rgb, n, h, w, scores, is_jpeg, out_rgb, t); });
    });
}

int ire_restore_fit_device(ire_engine* e, const uint8_t* d_rgb, int n, int h, int w, const double* d_scores, const uint8_t* d_is_jpeg,
                           uint8_t* d_out_rgb, void* stream) {
    return guarded([&] {
        Engine& E = eng(e);
        on_stream(E, (hipStream_t)stream, [&] { E.restore_fit_device(d_rgb, n, h, w, d_scores, d_is_jpeg, d_out_rgb, (hipStream_t)stream); });
    });
}

int ire_restore_tiled_device(ire_engine* e, const uint8_t* d_rgb, int h, int w, int nstrips, const double* d_scores,
                             const uint8_t* d_is_jpeg, uint8_t* d_out_rgb, void* stream) {
    return guarded([&] {
        Engine& E = eng(e);
        on_stream(E, (hipStream_t)stream, [&] { E.restore_tiled_device(d_rgb, h, w, nstrips, d_scores, d_is_jpeg, d_out_rgb, (hipStream_t)stream); });
    });
}

size_t ire_strips_stats_bytes(int h, int w) { return (h > 0 && w > 0) ? StripSession::stats_floats(h, w) * 4 : 0; }

int ire_strips_open(ire_engine* e, int h, int w, int nstrips_total, int first_strip, int nlocal, void* d_stats_all, ire_strips** out) {
    return guarded([&] {
        Engine& E = eng(e);
        if (!out) fail(IRE_ERR_INVALID_INPUT, "invalid arguments to ire_strips_open");
        *out = nullptr;
        std::unique_ptr<ire_strips> S(new ire_strips());
        {
            std::lock_guard<std::mutex> lk(E.mutex());
            S->s.reset(new StripSession(E, h, w, nstrips_total, first_strip, nlocal, (float*)d_stats_all));
        }
        std::lock_guard<std::mutex> lk(g_strips_mu);
        S->owner = e;
        e->sessions.push_back(S.get());
        *out = S.release();
    });
}

void ire_strips_close(ire_strips* s) {
    if (!s) return;
    {
        std::lock_guard<std::mutex> lk(g_strips_mu);
        if (s->owner) {       // the engine is alive: unregister, then free the session under the engine's lock
            auto& v = s->owner->sessions;
            for (size_t i = 0; i < v.size(); ++i) if (v[i] == s) { v.erase(v.begin() + i); break; }
            if (s->s) { std::lock_guard<std::mutex> lk2(s->s->engine().mutex()); s->s.reset(); }
            s->owner = nullptr;
        }
    }
    delete s;
}

static StripSession& strips_of(ire_strips* s) {
    if (!s || !s->s) fail(IRE_ERR_INVALID_INPUT, "invalid strip session handle");
    return *s->s;
}

int ire_strips_num_ops(ire_strips* s) { return (s && s->s) ? s->s->num_ops() : 0; }

int ire_strips_set_input(ire_strips* s, const uint8_t* d_rows_with_halo, const double* d_scores, void* stream) {
    return guarded([&] {
        StripSession& S = strips_of(s);
        on_stream(S.engine(), (hipStream_t)stream, [&] { S.set_input(d_rows_with_halo, d_scores, (hipStream_t)stream); });
    });
}

int ire_strips_run_op(ire_strips* s, int k, void* stream, ire_strip_xchg* info) {
    return guarded([&] {
        StripSession& S = strips_of(s);
        on_stream(S.engine(), (hipStream_t)stream, [&] { S.run_op(k, (hipStream_t)stream, info); });
    });
}

int ire_strips_pack_halo(ire_strips* s, int k, uint8_t* d_send_up, uint8_t* d_send_down, void* stream) {
    return guarded([&] {
        StripSession& S = strips_of(s);
        on_stream(S.engine(), (hipStream_t)stream, [&] { S.pack_halo(k, d_send_up, d_send_down, (hipStream_t)stream); });
    });
}

int ire_strips_unpack_halo(ire_strips* s, int k, const uint8_t* d_recv_up, const uint8_t* d_recv_down, void* stream) {
    return guarded([&] {
        StripSession& S = strips_of(s);
        on_stream(S.engine(), (hipStream_t)stream, [&] { S.unpack_halo(k, d_recv_up, d_recv_down, (hipStream_t)stream); });
    });
}

int ire_strips_get_output(ire_strips* s, uint8_t* d_out_rows, void* stream) {
    return guarded([&] {
        StripSession& S = strips_of(s);
        if (!d_out_rows) fail(IRE_ERR_INVALID_INPUT, "invalid output pointer");
        on_stream(S.engine(), (hipStream_t)stream, [&] { S.get_output(d_out_rows, (hipStream_t)stream); });
    });
}

int ire_get_stats(ire_engine* e, ire_engine_stats* out) {
    return guarded([&] {
        Engine& E = eng(e);
        if (!out || out->struct_size < sizeof(ire_engine_stats)) fail(IRE_ERR_INVALID_INPUT, "invalid ire_engine_stats.struct_size");
        {
            std::lock_guard<std::mutex> lk(E.mutex());
            E.get_stats(out);
        }
        out->queue_depth = e->batcher->queue_depth();
    });
}

int ire_submit(ire_engine* e, const uint8_t* rgb, int h, int w, int is_jpeg, const double* scores, ire_job** job_out) {
    return guarded([&] {
        eng(e);
        if (!rgb || !job_out) fail(IRE_ERR_INVALID_INPUT, "invalid arguments to ire_submit");
        if (h <= 0 || w <= 0 || h % 8 || w % 8 || h < 16 || w < 16 || h > 8192 || w > 8192)
            fail(IRE_ERR_INVALID_INPUT, "invalid image size for restore: height and width must be multiples of 8, >= 16");
        if (!piece_addressable(h, w, 0)) fail(IRE_ERR_INVALID_INPUT, not_addressable(h, w));      // no job is queued for the shape restore refuses
        job_handle(job_out, [&] { return e->batcher->submit(rgb, h, w, is_jpeg, scores); });
    });
}

int ire_submit_fit(ire_engine* e, const uint8_t* rgb, int h, int w, int is_jpeg, const double* scores, ire_job** job_out) {
    return guarded([&] {
        eng(e);
        if (!rgb || !job_out) fail(IRE_ERR_INVALID_INPUT, "invalid arguments to ire_submit_fit");
        if (h < 1 || w < 1 || h > 8192 || w > 8192) fail(IRE_ERR_INVALID_INPUT, "invalid image size: height and width must be in 1..8192");
        if (!piece_addressable(Engine::fit_dim(h), Engine::fit_dim(w), 0)) fail(IRE_ERR_INVALID_INPUT, not_addressable(Engine::fit_dim(h), Engine::fit_dim(w)));
        job_handle(job_out, [&] { return e->batcher->submit(rgb, h, w, is_jpeg, scores); });
    });
}

int ire_submit_jpeg(ire_engine* e, const uint8_t* file, size_t bytes, const double* scores, ire_job** job_out) {
    return guarded([&] {
        eng(e);
        if (!file || !job_out) fail(IRE_ERR_INVALID_INPUT, "invalid arguments to ire_submit_jpeg");
        // (is_jpeg = 0 for a PNG on an engine that decodes it: what ire_submit_fit of its pixels would be told)
        const bool png = eng(e).png_decoder().enabled() && pngparse::is_png(file, bytes);
        job_handle(job_out, [&] { return e->batcher->submit_file(file, bytes, scores, !png); });
    });
}

int ire_submit_file(ire_engine* e, const uint8_t* file, size_t bytes, const double* scores, ire_job** job_out) { return ire_submit_jpeg(e, file, bytes, scores, job_out); }

int ire_submit_upload(ire_engine* e, const uint8_t* file, size_t bytes, int max_dim, const double* scores, ire_job** job_out) {
    return guarded([&] {
        eng(e);
        if (!file || !job_out) fail(IRE_ERR_INVALID_INPUT, "invalid arguments to ire_submit_upload");
        const bool png = eng(e).png_decoder().enabled() && pngparse::is_png(file, bytes);
        job_handle(job_out, [&] { return e->batcher->submit_upload(file, bytes, max_dim, scores, !png); });
    });
}

int ire_submit_fuse_fit(ire_engine* e, const uint8_t* const* views, int k, int h, int w, const uint8_t* is_jpeg, const uint8_t* has_scores, const double* scores,
                        ire_job** job_out) {
    return guarded([&] {
        eng(e);
        if (!views || !job_out) fail(IRE_ERR_INVALID_INPUT, "invalid arguments to ire_submit_fuse_fit");
        *job_out = nullptr;
        if (k < 2 || k > 3) fail(IRE_ERR_INVALID_INPUT, "invalid view count for fusion: expected 2..3");
        for (int v = 0; v < k; ++v) if (!views[v]) fail(IRE_ERR_INVALID_INPUT, "invalid arguments to ire_submit_fuse_fit: null view");
        if (h < 1 || w < 1 || h > 8192 || w > 8192) fail(IRE_ERR_INVALID_INPUT, "invalid image size: height and width must be in 1..8192");
        if (!piece_addressable(Engine::fit_dim(h), Engine::fit_dim(w), 0)) fail(IRE_ERR_INVALID_INPUT, not_addressable(Engine::fit_dim(h), Engine::fit_dim(w)));
        if (has_scores && !scores) for (int v = 0; v < k; ++v) if (has_scores[v]) fail(IRE_ERR_INVALID_INPUT, "invalid arguments to ire_submit_fuse_fit: has_scores without scores");
        job_handle(job_out, [&] { return e->batcher->submit_group(views, k, h, w, is_jpeg, has_scores, scores); });       // (refuses k views on an engine with max_batch < k)
    });
}

int ire_restore_fuse_fit_device(ire_engine* e, const uint8_t* d_views, int nsets, int k, int h, int w, const double* d_scores, const uint8_t* d_is_jpeg,
                                uint8_t* d_out_rgb, void* stream) {
    return guarded([&] {
        Engine& E = eng(e);
        on_stream(E, (hipStream_t)stream, [&] { E.restore_fuse_fit_device(d_views, nsets, k, h, w, d_scores, d_is_jpeg, d_out_rgb, (hipStream_t)stream); });
    });
}

int ire_debug_fusion_wlut(ire_engine* e, const double* noise, int n, uint32_t* out) {
    return guarded([&] {
        Engine& E = eng(e);
        on_stream(E, E.main_stream(), [&] { E.debug_fusion_wlut(noise, n, out); });
    });
}

int ire_poll(ire_engine* e, ire_job* job, int timeout_ms, uint8_t* out_rgb, double* scores_out, ire_timings* t) {
    return guarded([&] {
        eng(e);
        if (!job || !job->j) fail(IRE_ERR_INVALID_INPUT, "invalid job handle");
        // a result of data-dependent length has no way out of this call: refuse it and keep the job (no result is lost to a wrong call)
        if (e->backend->fmt && e->backend->fmt->counted) fail(IRE_ERR_INVALID_INPUT, "invalid: use ire_poll_text (this engine's results have data-dependent lengths)");
        std::string err;
        const int st = e->batcher->poll(job->j, timeout_ms, out_rgb, scores_out, t, &err);
        if (st == IRE_ERR_TIMEOUT) fail(IRE_ERR_TIMEOUT, "timeout: job still pending");       // the handle stays valid: poll again or ire_job_release
        delete job;
        if (st != IRE_OK) fail(st, err);
    });
}

int ire_poll_text(ire_engine* e, ire_job* job, int timeout_ms, uint8_t* out, size_t cap_bytes, size_t* len_out, double* scores_out, ire_timings* t) {
    return guarded([&] {
        eng(e);
        if (!job || !job->j) fail(IRE_ERR_INVALID_INPUT, "invalid job handle");
        if (!len_out) fail(IRE_ERR_INVALID_INPUT, "invalid arguments to ire_poll_text: len_out is null");
        std::string err;
        const int st = e->batcher->poll(job->j, timeout_ms, out, cap_bytes, len_out, scores_out, t, &err);
        if (st == IRE_ERR_TIMEOUT) fail(IRE_ERR_TIMEOUT, "timeout: job still pending");
        if (st == kPollTooSmall) fail(IRE_ERR_INVALID_INPUT, "invalid buffer size for ire_poll_text: the result is longer than cap_bytes (*len_out); the job is still pending");
        delete job;
        if (st != IRE_OK) fail(st, err);
    });
}

int ire_job_release(ire_engine* e, ire_job* job) {
    return guarded([&] {
        if (!job) return;
        // e == NULL: the engine is gone (ire_shutdown with jobs outstanding): only the handle is left to free
        if (e && e->batcher && job->j) e->batcher->release(job->j);
        delete job;
    });
}

int ire_affinity_plan(const char* sysfs_root, const char* pci_bdf, char* cpulist_out, size_t cap, int32_t* numa_node_out,
                      int32_t* slot_out, int32_t* nslots_out) {
    return guarded([&] {
        if (!pci_bdf || !cpulist_out || cap == 0) fail(IRE_ERR_INVALID_INPUT, "invalid arguments to ire_affinity_plan");
        const CpuPlan p = affinity_plan(sysfs_root && sysfs_root[0] ? sysfs_root : "/sys", pci_bdf);
        const std::string l = p.cpulist();
        if (l.size() + 1 > cap) fail(IRE_ERR_INVALID_INPUT, "invalid buffer size for ire_affinity_plan");
        std::memcpy(cpulist_out, l.c_str(), l.size() + 1);
        if (numa_node_out) *numa_node_out = p.numa_node;
        if (slot_out) *slot_out = p.slot;
        if (nslots_out) *nslots_out = p.nslots;
    });
}

int ire_engine_affinity(ire_engine* e, char* cpulist_out, size_t cap, int32_t* numa_node_out) {
    return guarded([&] {
        eng(e);
        if (!cpulist_out || cap == 0) fail(IRE_ERR_INVALID_INPUT, "invalid arguments to ire_engine_affinity");
        const std::string l = e->backend->plan.cpulist();
        if (l.size() + 1 > cap) fail(IRE_ERR_INVALID_INPUT, "invalid buffer size for ire_engine_affinity");
        std::memcpy(cpulist_out, l.c_str(), l.size() + 1);
        if (numa_node_out) *numa_node_out = e->backend->plan.numa_node;
    });
}

int ire_debug_classifier_sums(ire_engine* e, int n, uint64_t* sums_out) {
    return guarded([&] {
        Engine& E = eng(e);
        if (!sums_out) fail(IRE_ERR_INVALID_INPUT, "invalid output pointer");
        std::lock_guard<std::mutex> lk(E.mutex());
        E.debug_sums(n, sums_out);
    });
}

int ire_debug_poison_scratch(ire_engine* e, int byte, uint64_t* bytes_filled) {
    return guarded([&] {
        Engine& E = eng(e);
        if (!BufRegistry::on()) fail(IRE_ERR_INVALID_INPUT, "invalid call: ire_debug_poison_scratch needs IRE_DEBUG_POISON=<0..255> in the environment of the process");
        // The check and the fill under the engine's lock (the batcher's own lock is only ever taken inside it, never the other way round).
        // A queued job's input is already in its slot's staging, a delivered one's result still is: neither survives a fill.  A submit
        // takes the batcher's lock alone, so one that arrives between the check and the fill is not excluded: the caller submits nothing
        // while it poisons (ire.h).
        std::lock_guard<std::mutex> lk(E.mutex());
        if (e->batcher && !e->batcher->idle()) fail(IRE_ERR_INVALID_INPUT, "invalid call: ire_debug_poison_scratch while a job is queued, in flight or not yet polled");
        const uint64_t filled = E.debug_poison_scratch(byte);
        if (bytes_filled) *bytes_filled = filled;
    });
}

int ire_debug_gn_finalize(ire_engine* e, const float* stats, int nimg, int parts, int C, int hw, const float* gamma, const float* beta,
                          const float* film, int film_stride, int film_off, float* ab_out) {
    return guarded([&] {
        Engine& E = eng(e);
        on_stream(E, E.main_stream(), [&] { E.debug_gn_finalize(stats, nimg, parts, C, hw, gamma, beta, film, film_stride, film_off, ab_out); });
    });
}

int ire_debug_capture(ire_engine* e, int on) {
    return guarded([&] {
        Engine& E = eng(e);
        std::lock_guard<std::mutex> lk(E.mutex());
        E.debug_capture(on != 0);
    });
}

int ire_debug_activation(ire_engine* e, const char* name, float* out, size_t* count) {
    return guarded([&] {
        Engine& E = eng(e);
        if (!name) fail(IRE_ERR_INVALID_INPUT, "invalid activation name");
        std::lock_guard<std::mutex> lk(E.mutex());
        if (!E.debug_activation(name, out, count)) fail(IRE_ERR_INVALID_INPUT, std::string("invalid activation name: ") + name);
    });
}

int ire_profile_enable(ire_engine* e, int on) {
    return guarded([&] {
        Engine& E = eng(e);
        std::lock_guard<std::mutex> lk(E.mutex());
        E.profile_enable(on);
    });
}

int ire_profile_query(ire_engine* e, const char* family, double* ms_out, int64_t* launches_out, double* flops_out,
                      double* bytes_out) {
    return guarded([&] {
        Engine& E = eng(e);
        const int fam = family_id(family);
        std::lock_guard<std::mutex> lk(E.mutex());
        E.profile_query(fam, ms_out, launches_out, flops_out, bytes_out);
    });
}

int ire_profile_report(ire_engine* e, char* buf, size_t cap, size_t* needed_out) {
    return guarded([&] {
        Engine& E = eng(e);
        std::string r;
        {
            std::lock_guard<std::mutex> lk(E.mutex());
            r = E.profile_report();
        }
        if (needed_out) *needed_out = r.size() + 1;
        if (buf && cap) {
            if (cap < r.size() + 1) fail(IRE_ERR_INVALID_INPUT, "invalid buffer size for ire_profile_report (query *needed_out first)");
            std::memcpy(buf, r.c_str(), r.size() + 1);
        }
    });
}

int ire_profile_reset(ire_engine* e) {
    return guarded([&] {
        Engine& E = eng(e);
        std::lock_guard<std::mutex> lk(E.mutex());
        E.profile_reset();
    });
}

}  // extern "C"
