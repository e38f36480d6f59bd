// batcher_uploads_stress.cpp -- the batcher's UPLOAD jobs (csrc/batcher.hpp: submit_upload and the optional backend hooks upload_plan
// / decode_upload beside the file hooks) over a host-only STUB backend, built with ThreadSanitizer and with AddressSanitizer + UBSan
// and run by tests/test_batcher_uploads_native.py, in the pattern of tests/native/batcher_files_stress.cpp.  Test infrastructure: the
// stub's "upload" is a seven-byte head (magic, shape, orientation, three switches, upload or plain file) in front of the FITTED pixels
// xored with 0x33; its "decode + preprocess" undoes the xor and adds the key's orientation to every byte, so a job that reached the
// device under another key than its own gives wrong bytes.  A shape's stored size is twice its fitted size whatever the orientation:
// keys that differ only in orientation or max_dim share an output size and must still never share a slot.
//
// What is driven: threads that submit uploads of several keys, plain files and pixels of two output shapes at once (a batch holds
// one kind and, for uploads, one key); a flagged upload in the middle of a batch (it fails alone); uploads the plan refuses and
// uploads that break the room rule (no job); an upload whose staging fails after it got its place; releases while gathering and
// while in flight; more jobs than the slots hold before the first poll (the overflow path); destruction with jobs pending.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <random>

#include "../../image_restoration_platform_amd/csrc/batcher.hpp"

using namespace ire;

static std::atomic<int> g_fail{0};
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "CHECK failed: %s (%s:%d)\n", #c, __FILE__, __LINE__); g_fail++; } } while (0)

static uint8_t f_px(uint8_t v, size_t k) { return (uint8_t)((v ^ 0x5a) + (uint8_t)(k * 7)); }
static void shape_of(int shape, int* h, int* w) { *h = shape ? 24 : 16; *w = shape ? 32 : 16; }      // the FITTED (output) size

constexpr uint8_t kMagic = 0xF2;
constexpr int kHead = 7;             // magic | shape | orientation | flagged by the decode | staging fails | claims more room than its place | upload (else a plain file)
struct StubHead { int shape, orientation; bool flagged, stage_fails; };

enum SlotKind { NONE = 0, K_PIXELS = 1, K_FILES = 2, K_UPLOADS = 4 };
struct StubSlot {
    std::vector<uint8_t> d_in, d_out;
    int fstat[kMaxBatch] = {};
    int kinds = NONE;                // of the batch being gathered (launcher thread only; a batch's first push begins it anew)
    int key[4] = {};                 // ... and the key of its uploads
    std::mutex mu;
    std::condition_variable cv;
    bool compute_done = true, out_done = true;
};

struct StubBackend {
    int mb;
    std::atomic<int> launches{0}, upload_decodes{0}, mixed{0}, key_mixed{0};
    std::mutex qmu;
    std::condition_variable qcv;
    std::deque<std::function<void()>> q;
    bool stop = false;
    std::thread dev;
    explicit StubBackend(int max_batch) : mb(max_batch) {
        dev = std::thread([this] {
            std::unique_lock<std::mutex> lk(qmu);
            for (;;) {
                qcv.wait(lk, [&] { return stop || !q.empty(); });
                if (q.empty()) return;
                auto fn = std::move(q.front()); q.pop_front();
                lk.unlock(); fn(); lk.lock();
            }
        });
    }
    ~StubBackend() { { std::lock_guard<std::mutex> lk(qmu); stop = true; } qcv.notify_all(); dev.join(); }
    int max_batch() const { return mb; }
    size_t out_bytes(int h, int w) const { return (size_t)h * w * 3; }
    void start() {}
    void thread_enter(const char*) {}
    void reserve(SlotBufs& b, size_t bytes, int max_batch) {
        if (b.fixed && bytes <= b.cap) return;
        StubSlot* ss = static_cast<StubSlot*>(b.impl);
        if (!ss) { ss = new StubSlot(); b.impl = ss; }
        if (!b.fixed) { b.pin_jp = new uint8_t[max_batch](); b.pin_sc = new double[7 * max_batch](); b.pin_sc_in = new double[7 * max_batch](); b.fixed = true; }
        if (bytes > b.cap) {
            delete[] b.pin_in; delete[] b.pin_out;
            b.pin_in = new uint8_t[bytes](); b.pin_out = new uint8_t[bytes](); b.cap = bytes;
            ss->d_in.assign(bytes, 0); ss->d_out.assign(bytes, 0);
        }
    }
    void release(SlotBufs& b) noexcept {
        delete[] b.pin_in; delete[] b.pin_out; delete[] b.pin_jp; delete[] b.pin_sc; delete[] b.pin_sc_in;
        delete static_cast<StubSlot*>(b.impl);
        b = SlotBufs{};
    }
    // a push of jobs `first` .. into the slot's batch: what kind it is, and that the batch holds no other
    void note(StubSlot& ss, int first, int kind) {
        if (first == 0) ss.kinds = NONE;
        ss.kinds |= kind;
        if (ss.kinds != kind) ++mixed;
    }
    void h2d(SlotBufs& b, size_t off, size_t bytes) {
        StubSlot& ss = *static_cast<StubSlot*>(b.impl);
        note(ss, off == 0 ? 0 : 1, K_PIXELS);
        std::memcpy(ss.d_in.data() + off, b.pin_in + off, bytes);
    }
    // ---- the file hooks ----
    std::shared_ptr<void> file_plan(const uint8_t* file, size_t bytes, int* h, int* w, size_t* room) {
        if (bytes < (size_t)kHead || file[0] != kMagic) fail(IRE_ERR_INVALID_INPUT, "invalid: not a stub file");
        shape_of(file[1], h, w);
        const size_t ib = (size_t)*h * *w * 3;
        if (bytes != kHead + ib) fail(IRE_ERR_INVALID_INPUT, "invalid: truncated stub file");
        *room = file[5] ? ib + 1 : ib;
        return std::make_shared<StubHead>(StubHead{file[1], file[2], file[3] != 0, file[4] != 0});
    }
    size_t file_stage(void* head, const uint8_t* file, size_t bytes, uint8_t* dst, size_t room) {
        if (static_cast<StubHead*>(head)->stage_fails) fail(IRE_ERR_INVALID_INPUT, "invalid: the stub file changed under the submit");
        CHECK(bytes - kHead <= room);
        std::memcpy(dst, file + kHead, bytes - kHead);
        return bytes - kHead;
    }
    void undo(StubSlot& ss, SlotBufs& b, int first, int count, size_t ib, int add, void* const* heads, const size_t* used) {
        for (int i = 0; i < count; ++i) {
            const StubHead& hd = *static_cast<const StubHead*>(heads[i]);
            CHECK(used[i] == (hd.stage_fails ? 0 : ib));
            for (size_t p = 0; p < used[i]; ++p) ss.d_in[ib * (first + i) + p] = (uint8_t)((b.pin_in[ib * (first + i) + p] ^ 0x33) + add);
            ss.fstat[first + i] = hd.flagged ? 5 : 0;
        }
    }
    void decode(SlotBufs& b, int first, int count, int h, int w, void* const* heads, const size_t* used) {
        StubSlot& ss = *static_cast<StubSlot*>(b.impl);
        note(ss, first, K_FILES);
        undo(ss, b, first, count, (size_t)h * w * 3, 0, heads, used);
    }
    // ---- the upload hooks ----
    std::shared_ptr<void> upload_plan(const uint8_t* file, size_t bytes, int max_dim, int* h, int* w, size_t* room, int key[4]) {
        auto head = file_plan(file, bytes, h, w, room);
        if (max_dim < 1) fail(IRE_ERR_INVALID_INPUT, "invalid arguments to preprocess");
        key[0] = 2 * *h; key[1] = 2 * *w; key[2] = file[2]; key[3] = max_dim;
        return head;
    }
    void decode_upload(SlotBufs& b, int first, int count, int h, int w, const int key[4], void* const* heads, const size_t* used) {
        StubSlot& ss = *static_cast<StubSlot*>(b.impl);
        note(ss, first, K_UPLOADS);
        if (first == 0) std::memcpy(ss.key, key, sizeof(ss.key));
        else if (std::memcmp(ss.key, key, sizeof(ss.key))) ++key_mixed;
        ++upload_decodes;
        CHECK(key[0] == 2 * h && key[1] == 2 * w);
        for (int i = 0; i < count; ++i) if (static_cast<const StubHead*>(heads[i])->orientation != key[2]) ++key_mixed;      // every job under its own key
        undo(ss, b, first, count, (size_t)h * w * 3, key[2] + key[3], heads, used);
    }
    int file_status(SlotBufs& b, int i) { return static_cast<StubSlot*>(b.impl)->fstat[i]; }
    void launch(SlotBufs& b, int n, int h, int w, const uint8_t* has_sc) {
        ++launches;
        StubSlot* ss = static_cast<StubSlot*>(b.impl);
        { std::lock_guard<std::mutex> lk(ss->mu); ss->compute_done = false; ss->out_done = false; }
        std::vector<uint8_t> hs(has_sc, has_sc + n);
        SlotBufs* bp = &b;
        std::lock_guard<std::mutex> lk(qmu);
        q.push_back([=] {
            const size_t ib = (size_t)h * w * 3;
            std::this_thread::sleep_for(std::chrono::microseconds(150));
            for (int i = 0; i < n; ++i) {
                for (size_t p = 0; p < ib; ++p) ss->d_out[ib * i + p] = f_px(ss->d_in[ib * i + p], p);
                for (int s = 0; s < 7; ++s) bp->pin_sc[7 * i + s] = hs[i] ? bp->pin_sc_in[7 * i + s] : (double)ss->d_in[ib * i] + s + (bp->pin_jp[i] ? 0.5 : 0.0);
            }
            { std::lock_guard<std::mutex> l2(ss->mu); ss->compute_done = true; }
            ss->cv.notify_all();
            std::this_thread::sleep_for(std::chrono::microseconds(40));
            std::memcpy(bp->pin_out, ss->d_out.data(), ib * n);
            { std::lock_guard<std::mutex> l2(ss->mu); ss->out_done = true; }
            ss->cv.notify_all();
        });
        qcv.notify_all();
    }
    bool computing(SlotBufs& b) noexcept { StubSlot& ss = *static_cast<StubSlot*>(b.impl); std::lock_guard<std::mutex> lk(ss.mu); return !ss.compute_done; }
    void wait_compute(SlotBufs& b) noexcept { StubSlot& ss = *static_cast<StubSlot*>(b.impl); std::unique_lock<std::mutex> lk(ss.mu); ss.cv.wait(lk, [&] { return ss.compute_done; }); }
    void wait_done(SlotBufs& b, ire_timings& t) { StubSlot& ss = *static_cast<StubSlot*>(b.impl); std::unique_lock<std::mutex> lk(ss.mu); ss.cv.wait(lk, [&] { return ss.out_done; }); t.restore_ms = 0.15; t.total_ms = 0.15; }
    void drain() noexcept {
        std::mutex m; std::condition_variable c; bool done = false;
        { std::lock_guard<std::mutex> lk(qmu); q.push_back([&] { std::lock_guard<std::mutex> l(m); done = true; c.notify_all(); }); }
        qcv.notify_all();
        std::unique_lock<std::mutex> lk(m);
        c.wait(lk, [&] { return done; });
    }
};
static_assert(has_file_jobs<StubBackend>::value && has_upload_jobs<StubBackend>::value, "the stub has the file and the upload hooks");

enum Kind { PIXELS, FILE_OK, UPLOAD_OK, UPLOAD_FLAGGED, UPLOAD_STAGE_FAILS };
struct Img { int h, w, orientation, max_dim; std::vector<uint8_t> px, file; bool with_scores; double sc[7]; int jpeg; Kind kind; };
static Img make_img(std::mt19937& rng, int shape, Kind kind, int orientation = 1, int max_dim = 64) {
    Img im;
    shape_of(shape, &im.h, &im.w);
    im.kind = kind; im.orientation = orientation; im.max_dim = max_dim;
    im.px.resize((size_t)im.h * im.w * 3);
    for (auto& v : im.px) v = (uint8_t)rng();
    im.with_scores = rng() & 1; im.jpeg = kind == PIXELS ? (int)(rng() & 1) : 1;
    for (int s = 0; s < 7; ++s) im.sc[s] = (double)(rng() % 1000) / 1000.0;
    if (kind != PIXELS) {
        im.file = {kMagic, (uint8_t)shape, (uint8_t)orientation, (uint8_t)(kind == UPLOAD_FLAGGED), (uint8_t)(kind == UPLOAD_STAGE_FAILS), 0, (uint8_t)(kind != FILE_OK)};
        for (uint8_t v : im.px) im.file.push_back(v ^ 0x33);
    }
    return im;
}
// what the stub's device makes of the job's pixels before the "network": an upload's bytes carry its key
static uint8_t staged(const Img& im, size_t p) { return (uint8_t)(im.px[p] + (im.kind == PIXELS || im.kind == FILE_OK ? 0 : im.orientation + im.max_dim)); }
static void verify(const Img& im, const std::vector<uint8_t>& out, const double* sc) {
    bool ok = true;
    for (size_t p = 0; p < im.px.size() && ok; ++p) ok = out[p] == f_px(staged(im, p), p);
    CHECK(ok);
    for (int s = 0; s < 7; ++s) CHECK(sc[s] == (im.with_scores ? im.sc[s] : (double)staged(im, 0) + s + (im.jpeg ? 0.5 : 0.0)));
}

using B = Batcher<StubBackend>;
struct Pending { Img im; std::shared_ptr<Job> j; };

static std::shared_ptr<Job> send(B& bt, const Img& im) {
    const double* sc = im.with_scores ? im.sc : nullptr;
    if (im.kind == PIXELS) return bt.submit(im.px.data(), im.h, im.w, im.jpeg, sc);
    if (im.kind == FILE_OK) return bt.submit_file(im.file.data(), im.file.size(), sc);
    return bt.submit_upload(im.file.data(), im.file.size(), im.max_dim, sc);
}
static void finish(const Pending& p, int st, const std::vector<uint8_t>& out, const double* sc, const std::string& err) {
    if (p.im.kind == UPLOAD_FLAGGED) CHECK(st == IRE_ERR_INVALID_INPUT && err == "invalid: corrupt JPEG data (decoder status 5)");
    else if (p.im.kind == UPLOAD_STAGE_FAILS) CHECK(st == IRE_ERR_INVALID_INPUT && err == "invalid: the stub file changed under the submit");
    else { CHECK(st == IRE_OK); if (st == IRE_OK) verify(p.im, out, sc); }
}
static void poll_all(B& bt, std::vector<Pending>& ps) {
    for (auto& p : ps) {
        std::vector<uint8_t> out(p.im.px.size()); double sc[7]; std::string err;
        finish(p, bt.poll(p.j, -1, out.data(), sc, nullptr, &err), out, sc, err);
    }
}

// threads x jobs, every job submitted before the first poll; kinds, keys and shapes mixed; thread `abandoner` gives up every other
// job, some still gathering, some in flight, some done
static void burst(B& bt, int threads, int jobs, int abandoner, unsigned seed, bool uploads_only) {
    std::vector<std::thread> th;
    for (int t = 0; t < threads; ++t)
        th.emplace_back([&, t] {
            std::mt19937 rng(seed + 977 * t);
            std::vector<Pending> pend;
            for (int k = 0; k < jobs; ++k) {
                const unsigned r = rng() % 16;
                const Kind kind = r == 0 ? UPLOAD_FLAGGED : r == 1 ? UPLOAD_STAGE_FAILS : (uploads_only || r < 10) ? UPLOAD_OK : r < 13 ? FILE_OK : PIXELS;
                Pending p{make_img(rng, (k + t) & 1, kind, 1 + (int)(rng() % 3) * 5 % 8, (rng() & 1) ? 64 : 48), nullptr};      // orientations 1, 6, 3; two max_dims
                p.j = send(bt, p.im);
                pend.push_back(std::move(p));
            }
            std::shuffle(pend.begin(), pend.end(), rng);
            size_t released = 0;
            while (!pend.empty()) {
                for (size_t i = 0; i < pend.size();) {
                    Pending& p = pend[i];
                    if (t == abandoner && (released++ & 1)) { bt.release(p.j); pend.erase(pend.begin() + i); continue; }
                    std::vector<uint8_t> out(p.im.px.size());
                    double sc[7]; ire_timings tm{}; std::string err;
                    const int st = bt.poll(p.j, (int)(rng() % 2), out.data(), sc, &tm, &err);
                    if (st == IRE_ERR_TIMEOUT) { ++i; continue; }
                    finish(p, st, out, sc, err);
                    pend.erase(pend.begin() + i);
                }
            }
        });
    for (auto& t : th) t.join();
}

static bool drained(B& bt) {
    for (int i = 0; i < 200 && bt.queue_depth() != 0; ++i) std::this_thread::sleep_for(std::chrono::milliseconds(1));
    return bt.queue_depth() == 0;
}

int main() {
    {   // 1. mixed submitters: uploads of six keys, plain files and pixels of two output shapes, flagged and stage-failing uploads, an abandoner
        StubBackend be(2);
        B bt(be);
        for (unsigned round = 0; round < 6; ++round) {
            burst(bt, 4, 16, (int)(round % 4), 1 + 10 * round, false);
            CHECK(drained(bt));
        }
        const auto c = bt.counters();
        std::printf("mixed: batches %ld overflowed %ld evicted %ld abandoned %ld upload decodes %d mixed %d key_mixed %d\n", c.batches, c.overflowed, c.evicted, c.abandoned,
                    be.upload_decodes.load(), be.mixed.load(), be.key_mixed.load());
        CHECK(c.overflowed > 0 && c.abandoned > 0 && c.failed_batches == 0 && be.upload_decodes.load() > 0);
        CHECK(be.mixed.load() == 0);                     // no batch held two kinds
        CHECK(be.key_mixed.load() == 0);                 // no batch held uploads of two keys
    }
    {   // 2. two keys of ONE output size (orientation 6 and 8; then max_dim 64 and 48), alternating, max_batch 4: each key gathers in
        //    its own slot, and pixel and file jobs of that size in theirs; a flagged upload fails alone
        StubBackend be(4);
        B bt(be);
        std::mt19937 rng(5);
        std::vector<Pending> ps;
        for (int k = 0; k < 8; ++k) ps.push_back(Pending{make_img(rng, 0, k == 2 ? UPLOAD_FLAGGED : UPLOAD_OK, k & 1 ? 8 : 6, 64), nullptr});
        for (int k = 0; k < 4; ++k) ps.push_back(Pending{make_img(rng, 0, UPLOAD_OK, 6, k & 1 ? 48 : 64), nullptr});
        ps.push_back(Pending{make_img(rng, 0, PIXELS), nullptr});
        ps.push_back(Pending{make_img(rng, 0, FILE_OK), nullptr});
        for (auto& p : ps) p.j = send(bt, p.im);
        poll_all(bt, ps);
        const auto c = bt.counters();
        std::printf("keys: batches %ld failed %ld upload decodes %d\n", c.batches, c.failed_batches, be.upload_decodes.load());
        CHECK(c.failed_batches == 0 && be.upload_decodes.load() >= 3 && c.batches >= 5);      // three keys, pixels, files: five slots at least
        CHECK(be.mixed.load() == 0 && be.key_mixed.load() == 0);
    }
    {   // 3. uploads that create no job: refused by the plan, a max_dim the plan refuses, breaking the room rule; then the batcher serves on
        StubBackend be(2);
        B bt(be);
        std::mt19937 rng(6);
        Img im = make_img(rng, 1, UPLOAD_OK, 6);
        std::vector<uint8_t> bad = im.file;
        bad[0] = 0;
        try { bt.submit_upload(bad.data(), bad.size(), 64, nullptr); CHECK(!"refused"); } catch (const Error& e) { CHECK(e.code == IRE_ERR_INVALID_INPUT && e.msg == "invalid: not a stub file"); }
        try { bt.submit_upload(im.file.data(), im.file.size(), 0, nullptr); CHECK(!"refused"); } catch (const Error& e) { CHECK(e.code == IRE_ERR_INVALID_INPUT); }
        bad = im.file; bad[5] = 1;
        try { bt.submit_upload(bad.data(), bad.size(), 64, nullptr); CHECK(!"too large"); }
        catch (const Error& e) { CHECK(e.code == IRE_ERR_INVALID_INPUT && e.msg == kUploadRoomReason); }
        CHECK(bt.queue_depth() == 0 && bt.counters().batches == 0);
        std::vector<Pending> ps{Pending{im, nullptr}};
        ps[0].j = send(bt, im);
        poll_all(bt, ps);
    }
    {   // 4. release while pending and while in flight, uploads only, and the overflow path: 4 x 16 uploads before the first poll over 8 slots of 2
        StubBackend be(2);
        B bt(be);
        std::mt19937 rng(8);
        for (int k = 0; k < 6; ++k) {
            Img im = make_img(rng, k & 1, UPLOAD_OK, 6);
            auto j = send(bt, im);
            if (k & 1) bt.release(j);                                             // still gathering
            else if (k == 2) { std::this_thread::sleep_for(std::chrono::milliseconds(3)); bt.release(j); }      // launched by now: in flight or done
            else { std::vector<uint8_t> o(im.px.size()); double sc[7]; std::string e; CHECK(bt.poll(j, -1, o.data(), sc, nullptr, &e) == IRE_OK); verify(im, o, sc); }
        }
        for (unsigned round = 0; round < 4; ++round) { burst(bt, 4, 16, (int)(round % 4), 500 + round, true); CHECK(drained(bt)); }
        const auto c = bt.counters();
        std::printf("uploads only: batches %ld overflowed %ld evicted %ld abandoned %ld\n", c.batches, c.overflowed, c.evicted, c.abandoned);
        CHECK(c.overflowed > 0 && c.abandoned > 0 && c.failed_batches == 0 && be.mixed.load() == 0 && be.key_mixed.load() == 0);
    }
    {   // 5. destruction with upload jobs pending, gathered, in flight and overflowing
        StubBackend be(2);
        std::vector<Pending> left;
        {
            B bt(be);
            std::mt19937 rng(99);
            for (int k = 0; k < 40; ++k) { Pending p{make_img(rng, k & 1, k % 7 == 3 ? UPLOAD_FLAGGED : UPLOAD_OK, k % 3 ? 6 : 1), nullptr}; p.j = send(bt, p.im); left.push_back(std::move(p)); }
            bt.release(left[5].j);
        }
        left.clear();
    }
    if (g_fail.load()) { std::fprintf(stderr, "batcher_uploads_stress: %d check(s) failed\n", g_fail.load()); return 1; }
    std::puts("batcher_uploads_stress ok");
    return 0;
}
