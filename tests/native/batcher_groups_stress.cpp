// batcher_groups_stress.cpp -- the batcher's FUSION jobs (csrc/batcher.hpp: submit_group and the optional backend hook launch_group)
// over a host-only STUB backend, built with ThreadSanitizer and with AddressSanitizer + UBSan and run by
// tests/test_batcher_groups_native.py, as tests/native/batcher_stress.cpp is for pixel jobs.  Test infrastructure: the stub's
// "fused" result is a checksum of the job's own k staged views, so a job that was handed another job's place, or a view staged in
// the wrong one, shows in its bytes; libire.so instantiates the same template over HIP.
//
// What is driven: threads that submit pixel jobs and k = 2 / k = 3 fusion jobs of two shapes at once (a batch must hold one kind
// and one k: every staged image carries its kind in its first byte and the stub checks each batch it is given), slots that fill
// at max_batch / k jobs and never hold more than kGroupMaxJobs (one fused launch; the stub refuses a larger group as the engine
// does), more jobs than the slots hold before the first poll (overflow: the k views in the job's own vector, copied
// by the launcher; eviction of unread DONE slots), releases while pending / gathered / done, a batch whose launch fails (all its
// jobs fail, nobody else's), destruction with fusion jobs pending.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <random>

#include "../../image_restoration_platform_amd/csrc/batcher.hpp"

using namespace ire;

static std::atomic<int> g_fail{0};
#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "CHECK failed: %s (%s:%d)\n", #c, __FILE__, __LINE__); g_fail++; } } while (0)

static uint8_t f_px(uint8_t v, size_t p) { return (uint8_t)((v ^ 0x5a) + (uint8_t)(p * 7)); }
static uint8_t f_fuse(const uint8_t* const* v, int k, size_t p) {
    unsigned s = (unsigned)(p * 11);
    for (int i = 0; i < k; ++i) s += (unsigned)(v[i][p] ^ (0x21 * (i + 1))) * (unsigned)(2 * i + 3);
    return (uint8_t)s;
}

struct StubSlot {
    std::vector<uint8_t> d_in, d_out;
    std::mutex mu;
    std::condition_variable cv;
    bool compute_done = true, out_done = true;
};

struct StubBackend {
    int mb;
    std::atomic<int> launches{0}, group_launches{0}, mixed{0}, over_capacity{0}, failed_group_jobs{0};
    std::atomic<int> full_groups[4];
    std::atomic<bool> fail_groups{false};
    std::atomic<int> compute_us{150};       // how long a batch "computes"
    std::mutex qmu;
    std::condition_variable qcv;
    std::deque<std::function<void()>> q;
    bool stop = false;
    std::thread dev;
    explicit StubBackend(int max_batch) : mb(max_batch) {
        for (auto& f : full_groups) f = 0;
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
    void h2d(SlotBufs& b, size_t off, size_t bytes) {
        StubSlot& ss = *static_cast<StubSlot*>(b.impl);
        std::memcpy(ss.d_in.data() + off, b.pin_in + off, bytes);
    }
    // njobs jobs of k images each (k = 1: pixel jobs).  Every image of the batch must say `k` in its first byte.
    void enqueue(SlotBufs& b, int njobs, int k, int h, int w, const uint8_t* has_sc) {
        StubSlot* ss = static_cast<StubSlot*>(b.impl);
        const size_t ib = (size_t)h * w * 3;
        if (njobs * k > mb || njobs < 1) ++over_capacity;
        for (int i = 0; i < njobs * k; ++i) if (ss->d_in[ib * i] != (uint8_t)k) ++mixed;
        { std::lock_guard<std::mutex> lk(ss->mu); ss->compute_done = false; ss->out_done = false; }
        std::vector<uint8_t> hs(has_sc, has_sc + njobs * k);
        SlotBufs* bp = &b;
        std::lock_guard<std::mutex> lk(qmu);
        q.push_back([=] {
            std::this_thread::sleep_for(std::chrono::microseconds(compute_us.load()));
            for (int i = 0; i < njobs; ++i) {
                const uint8_t* v[3] = {nullptr, nullptr, nullptr};
                for (int t = 0; t < k; ++t) v[t] = ss->d_in.data() + ib * ((size_t)i * k + t);
                for (size_t p = 0; p < ib; ++p) ss->d_out[ib * i + p] = k == 1 ? f_px(v[0][p], p) : f_fuse(v, k, p);
                const int at = i * k;       // the job's scores are its view 0's
                for (int s = 0; s < 7; ++s) bp->pin_sc[7 * i + s] = hs[at] ? bp->pin_sc_in[7 * at + s] : (double)v[0][1] + s + (bp->pin_jp[at] ? 0.5 : 0.0);
            }
            { std::lock_guard<std::mutex> l2(ss->mu); ss->compute_done = true; }
            ss->cv.notify_all();
            std::this_thread::sleep_for(std::chrono::microseconds(40));
            std::memcpy(bp->pin_out, ss->d_out.data(), ib * njobs);
            { std::lock_guard<std::mutex> l2(ss->mu); ss->out_done = true; }
            ss->cv.notify_all();
        });
        qcv.notify_all();
    }
    void launch(SlotBufs& b, int n, int h, int w, const uint8_t* has_sc) { ++launches; enqueue(b, n, 1, h, w, has_sc); }
    void launch_group(SlotBufs& b, int njobs, int k, int h, int w, const uint8_t* has_sc) {
        ++group_launches;
        if (k < 2 || k > 3 || njobs > mb / k) ++over_capacity;
        else if (njobs == std::min(mb / k, kGroupMaxJobs)) ++full_groups[k];
        // one fused launch takes kGroupMaxJobs view sets (Engine::check_fuse_fit refuses more): a slot must never gather more
        if (njobs > kGroupMaxJobs) { ++over_capacity; throw Error{IRE_ERR_INVALID_INPUT, "invalid batch size for fusion"}; }
        if (fail_groups.load()) { failed_group_jobs += njobs; throw Error{IRE_ERR_INTERNAL, "internal: injected launch failure"}; }
        enqueue(b, njobs, k, h, w, has_sc);
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

// one job: k = 1 a pixel job, else a fusion job of k views
struct Work { int k, h, w; std::vector<uint8_t> px[3]; uint8_t jpeg[3], has[3]; double sc[3][7]; };
static Work make_work(std::mt19937& rng, int k, int shape) {
    Work wk;
    wk.k = k; wk.h = shape ? 24 : 16; wk.w = shape ? 32 : 16;
    for (int v = 0; v < k; ++v) {
        wk.px[v].resize((size_t)wk.h * wk.w * 3);
        for (auto& b : wk.px[v]) b = (uint8_t)rng();
        wk.px[v][0] = (uint8_t)k;           // what kind of batch this image belongs in (the stub checks)
        wk.jpeg[v] = rng() & 1; wk.has[v] = rng() & 1;
        for (int s = 0; s < 7; ++s) wk.sc[v][s] = (double)(rng() % 1000) / 1000.0;
    }
    return wk;
}
using B = Batcher<StubBackend>;
static std::shared_ptr<Job> submit(B& bt, const Work& wk) {
    if (wk.k == 1) return bt.submit(wk.px[0].data(), wk.h, wk.w, wk.jpeg[0], wk.has[0] ? wk.sc[0] : nullptr);
    const uint8_t* v[3] = {wk.px[0].data(), wk.px[1].data(), wk.k == 3 ? wk.px[2].data() : nullptr};
    return bt.submit_group(v, wk.k, wk.h, wk.w, wk.jpeg, wk.has, &wk.sc[0][0]);
}
static void verify(const Work& wk, const std::vector<uint8_t>& out, const double* sc) {
    const uint8_t* v[3] = {wk.px[0].data(), wk.px[1].data(), wk.px[2].data()};
    bool ok = true;
    for (size_t p = 0; p < out.size() && ok; ++p) ok = out[p] == (wk.k == 1 ? f_px(v[0][p], p) : f_fuse(v, wk.k, p));
    CHECK(ok);
    for (int s = 0; s < 7; ++s) CHECK(sc[s] == (wk.has[0] ? wk.sc[0][s] : (double)wk.px[0][1] + s + (wk.jpeg[0] ? 0.5 : 0.0)));
}
struct Pending { Work wk; std::shared_ptr<Job> j; };

// threads x jobs of mixed kinds, every job submitted before the first poll; polls in random order with short timeouts; thread
// `abandoner` gives up every other job.  -> how many polls ended in a failure status
static int burst(B& bt, int threads, int jobs, int abandoner, unsigned seed, bool fail_ok) {
    std::atomic<int> failed{0};
    std::vector<std::thread> th;
    for (int t = 0; t < threads; ++t)
        th.emplace_back([&, t] {
            std::mt19937 rng(seed + 977 * t);
            std::vector<Pending> pend;
            for (int n = 0; n < jobs; ++n) {
                Pending p{make_work(rng, 1 + (int)(rng() % 3), (n + t) & 1), nullptr};
                p.j = submit(bt, p.wk);
                pend.push_back(std::move(p));
            }
            std::shuffle(pend.begin(), pend.end(), rng);
            size_t released = 0;
            while (!pend.empty()) {
                for (size_t i = 0; i < pend.size();) {
                    Pending& p = pend[i];
                    if (t == abandoner && (released++ & 1)) { bt.release(p.j); pend.erase(pend.begin() + i); continue; }
                    std::vector<uint8_t> out(p.wk.px[0].size());
                    double sc[7]; ire_timings tm{}; std::string err;
                    const int st = bt.poll(p.j, (int)(rng() % 2), out.data(), sc, &tm, &err);
                    if (st == IRE_ERR_TIMEOUT) { ++i; continue; }
                    if (st == IRE_OK) verify(p.wk, out, sc);
                    else { CHECK(fail_ok && p.wk.k > 1 && !err.empty()); ++failed; }
                    pend.erase(pend.begin() + i);
                }
            }
        });
    for (auto& t : th) t.join();
    return failed.load();
}

static bool drained(B& bt) {
    for (int i = 0; i < 200 && bt.queue_depth() != 0; ++i) std::this_thread::sleep_for(std::chrono::milliseconds(1));
    return bt.queue_depth() == 0;
}

static int poll_one(B& bt, Pending& p, std::string* err) {
    std::vector<uint8_t> out(p.wk.px[0].size());
    double sc[7];
    const int st = bt.poll(p.j, -1, out.data(), sc, nullptr, err);
    if (st == IRE_OK) verify(p.wk, out, sc);
    return st;
}

int main() {
    {   // 1. bursts past every slot: max_batch 6 (6 pixel jobs, 3 jobs of k = 2, 2 jobs of k = 3 per slot), three kinds x two shapes
        StubBackend be(6);
        B bt(be);
        for (unsigned round = 0; round < 6; ++round) {
            CHECK(burst(bt, 4, 16, (int)(round % 4), 1 + 10 * round, false) == 0);
            CHECK(drained(bt));
        }
        const auto c = bt.counters();
        std::printf("burst: batches %ld overflowed %ld evicted %ld abandoned %ld | group launches %d full k2 %d k3 %d\n", c.batches, c.overflowed, c.evicted, c.abandoned,
                    be.group_launches.load(), be.full_groups[2].load(), be.full_groups[3].load());
        CHECK(c.overflowed > 0 && c.evicted > 0 && c.abandoned > 0 && c.failed_batches == 0);
        CHECK(be.mixed.load() == 0 && be.over_capacity.load() == 0);
        CHECK(be.launches.load() > 0 && be.full_groups[2].load() > 0 && be.full_groups[3].load() > 0);
    }
    {   // 2. max_batch 8: two jobs of k = 3 fill a slot (6 of 8 images; a third job opens the next slot); max_batch 2 refuses k = 3
        StubBackend be(8);
        B bt(be);
        std::mt19937 rng(5);
        std::vector<Pending> p;
        for (int n = 0; n < 3; ++n) { p.push_back(Pending{make_work(rng, 3, 0), nullptr}); p.back().j = submit(bt, p.back().wk); }
        for (auto& x : p) { std::string err; CHECK(poll_one(bt, x, &err) == IRE_OK); }
        CHECK(be.over_capacity.load() == 0 && be.mixed.load() == 0 && be.group_launches.load() >= 2);
        StubBackend small(2);
        B bs(small);
        Work wk = make_work(rng, 3, 0);
        bool refused = false;
        try { (void)submit(bs, wk); } catch (const Error& e) { refused = e.code == IRE_ERR_INVALID_INPUT; }
        CHECK(refused && bs.queue_depth() == 0);
        wk = make_work(rng, 2, 0);
        Pending q{wk, submit(bs, wk)};
        std::string err;
        CHECK(poll_one(bs, q, &err) == IRE_OK);
    }
    {   // 2b. max_batch 64: max_batch / k is 32 and 21, but a slot closes at kGroupMaxJobs = 16 jobs.  The device is kept busy by a
        // pixel batch, so the fusion slots gather until they are full: 34 jobs of k = 2 go as 16 + 16 + 2, 17 of k = 3 as 16 + 1
        StubBackend be(64);
        B bt(be);
        std::mt19937 rng(23);
        for (int k = 2; k <= 3; ++k) {
            be.compute_us = 30000;
            Pending busy{make_work(rng, 1, 1), nullptr};
            busy.j = submit(bt, busy.wk);
            for (int i = 0; i < 2000 && bt.queue_depth() != 0; ++i) std::this_thread::sleep_for(std::chrono::milliseconds(1));      // (its slot has closed: it launches before anything gathered later)
            const int groups = be.group_launches.load(), total = k == 2 ? 34 : 17;
            std::vector<Pending> p;
            for (int n = 0; n < total; ++n) { p.push_back(Pending{make_work(rng, k, 0), nullptr}); p.back().j = submit(bt, p.back().wk); }
            be.compute_us = 150;
            std::string err;
            CHECK(poll_one(bt, busy, &err) == IRE_OK);
            for (auto& x : p) CHECK(poll_one(bt, x, &err) == IRE_OK);
            CHECK(be.full_groups[k].load() == total / kGroupMaxJobs && be.group_launches.load() - groups == total / kGroupMaxJobs + 1);
        }
        CHECK(be.over_capacity.load() == 0 && be.mixed.load() == 0 && bt.counters().failed_batches == 0);
    }
    {   // 3. a pending fusion job is released; later jobs on the same batcher complete
        StubBackend be(6);
        B bt(be);
        std::mt19937 rng(17);
        Pending a{make_work(rng, 3, 1), nullptr};
        a.j = submit(bt, a.wk);
        bt.release(a.j);
        CHECK(bt.counters().abandoned == 1);
        for (int n = 0; n < 4; ++n) {
            Pending b{make_work(rng, 2 + (n & 1), 1), nullptr};
            b.j = submit(bt, b.wk);
            std::string err;
            CHECK(poll_one(bt, b, &err) == IRE_OK);
        }
        CHECK(drained(bt));
    }
    {   // 4. a batch whose launch fails: every job of it fails with the launch's message, pixel jobs beside it complete
        StubBackend be(6);
        B bt(be);
        be.fail_groups = true;
        const int failed = burst(bt, 3, 10, -1, 31, true);
        CHECK(drained(bt));
        const auto c = bt.counters();
        std::printf("failures: batches %ld failed %ld | failed polls %d, jobs in failed launches %d\n", c.batches, c.failed_batches, failed, be.failed_group_jobs.load());
        CHECK(c.failed_batches > 0 && failed > 0 && failed == be.failed_group_jobs.load());      // (nobody abandons here: every job of a failed batch is polled)
        be.fail_groups = false;
        CHECK(burst(bt, 3, 6, -1, 32, false) == 0);
    }
    {   // 5. destruction with fusion jobs pending, gathered, in flight, done-unread and overflowing; the handles are dropped afterwards
        StubBackend be(4);
        std::vector<Pending> left;
        {
            B bt(be);
            std::mt19937 rng(99);
            for (int n = 0; n < 30; ++n) {
                Pending p{make_work(rng, 1 + n % 3, n & 1), nullptr};
                p.j = submit(bt, p.wk);
                left.push_back(std::move(p));
            }
            for (int n = 0; n < 3; ++n) { std::string err; CHECK(poll_one(bt, left[n], &err) == IRE_OK); }
            bt.release(left[5].j);
        }
        left.clear();
    }
    if (g_fail.load()) { std::fprintf(stderr, "batcher_groups_stress: %d check(s) failed\n", g_fail.load()); return 1; }
    std::puts("batcher_groups_stress ok");
    return 0;
}
