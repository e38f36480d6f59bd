// batcher_stress.cpp -- the engine's batcher state machine (image_restoration_platform_amd/csrc/batcher.hpp) over the host-only STUB
// backend of tests/native/batcher_stub.hpp, built with ThreadSanitizer and with AddressSanitizer + UBSan and driven from several
// threads by tests/test_batcher_native.py on the CPU box (sanitizers on the CPU build).
//
// What is driven: concurrent submitters of two shapes staging outside the lock, more jobs than kSlots * max_batch before the
// first poll (overflow queue, launcher-side staging, eviction of unread DONE slots), polls out of order with 0 / 1 ms timeouts
// that are retried, jobs abandoned with release() while pending / in flight / done / overflowing, a closed loop, failing
// allocations (the strong guarantee of reserve) and failing launches, destruction with jobs pending; and, since one stub serves
// every kind, pixel, file, upload and fusion jobs of both shapes submitted at once (no slot holds two keys).  Every delivered
// result is compared with f(input); the process exits non-zero on any mismatch and the sanitizers report the rest.
#include "batcher_stub.hpp"

// threads x jobs, every job submitted before the first poll; polls in random order with short timeouts; thread `abandoner` gives up every other job
static void burst(B& bt, int threads, int jobs, int abandoner, unsigned seed, int expect_fail_ok) {
    std::vector<std::thread> th;
    for (int t = 0; t < threads; ++t)
        th.emplace_back([&, t] {
            std::mt19937 rng(seed + 977 * t);
            std::vector<Pending> pend;
            for (int k = 0; k < jobs; ++k) {
                Pending p{make_img(rng, (k + t) & 1), nullptr};
                try { p.j = bt.submit(p.im.px.data(), p.im.h, p.im.w, p.im.jpeg, p.im.with_scores ? p.im.sc : nullptr); }
                catch (const Error& e) { CHECK(expect_fail_ok && e.code == IRE_ERR_UNAVAILABLE); continue; }
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
                    if (st == IRE_ERR_TIMEOUT) {
                        if (t == abandoner && (rng() % 4) == 0) { bt.release(p.j); pend.erase(pend.begin() + i); continue; }   // a timed-out job given up
                        ++i; continue;
                    }
                    if (st == IRE_OK) verify(p.im, out, sc);
                    else CHECK(expect_fail_ok && !err.empty());
                    pend.erase(pend.begin() + i);
                }
            }
        });
    for (auto& t : th) t.join();
}

static void closed_loop(B& bt, int threads, int inflight, int total) {
    std::vector<std::thread> th;
    for (int t = 0; t < threads; ++t)
        th.emplace_back([&, t] {
            std::mt19937 rng(4242 + t);
            std::deque<Pending> q;
            int sent = 0, got = 0;
            while (got < total) {
                while (sent < total && (int)q.size() < inflight) {
                    Pending p{make_img(rng, t & 1), nullptr};
                    p.j = bt.submit(p.im.px.data(), p.im.h, p.im.w, p.im.jpeg, p.im.with_scores ? p.im.sc : nullptr);
                    q.push_back(std::move(p)); ++sent;
                }
                Pending p = std::move(q.front()); q.pop_front();
                std::vector<uint8_t> out(p.im.px.size());
                double sc[7]; std::string err;
                const int st = bt.poll(p.j, -1, out.data(), sc, nullptr, &err);
                CHECK(st == IRE_OK);
                if (st == IRE_OK) verify(p.im, out, sc);
                ++got;
            }
        });
    for (auto& t : th) t.join();
}

// threads x jobs of all four kinds at once -- pixels, files, uploads of eight keys, fusion jobs of k = 2 and 3 -- at both shapes, every
// job submitted before the first poll and every result verified
static void all_kinds(B& bt, int threads, int jobs, unsigned seed) {
    std::vector<std::thread> th;
    for (int t = 0; t < threads; ++t)
        th.emplace_back([&, t] {
            std::mt19937 rng(seed + 977 * t);
            std::vector<Pending> one;
            std::vector<PendingWork> many;
            for (int n = 0; n < jobs; ++n) {
                const unsigned r = rng() % 5;
                const int shape = (n + t) & 1, orientation = (rng() & 1) ? 6 : 1, max_dim = (rng() & 1) ? 64 : 48;
                if (r < 2) { many.push_back(PendingWork{make_work(rng, 2 + (int)r, shape), nullptr}); many.back().j = send(bt, many.back().wk); }
                else { one.push_back(Pending{make_img(rng, shape, r == 2 ? PIXELS : r == 3 ? FILE_OK : UPLOAD_OK, orientation, max_dim), nullptr}); one.back().j = send(bt, one.back().im); }
            }
            poll_all(bt, one);
            std::string err;
            for (auto& p : many) CHECK(poll_one(bt, p, &err) == IRE_OK);
        });
    for (auto& t : th) t.join();
}

int main() {
    {   // 1. bursts past every slot (max_batch 2: 8 slots hold 16 jobs; 4 x 16 = 64 submitted before the first poll), two shapes, an abandoner
        StubBackend be(2);
        B bt(be);
        for (unsigned round = 0; round < 6; ++round) {
            burst(bt, 4, 16, (int)(round % 4), 1 + 10 * round, 0);
            CHECK(drained(bt));
        }
        closed_loop(bt, 3, 5, 60);
        CHECK(drained(bt));
        const auto c = bt.counters();
        std::printf("burst: batches %ld overflowed %ld evicted %ld abandoned %ld\n", c.batches, c.overflowed, c.evicted, c.abandoned);
        CHECK(c.overflowed > 0 && c.evicted > 0 && c.abandoned > 0 && c.failed_batches == 0);
    }
    {   // 2. allocations and launches that fail: errors reach the jobs, nothing leaks, the service threads live on
        StubBackend be(4);
        be.fail_reserve_every = 5; be.fail_launch_every = 4;
        B* bt = nullptr;
        for (int tries = 0; tries < 8 && !bt; ++tries) {       // the eager reservation of the first submit may be the injected failure
            bt = new B(be);
            std::mt19937 rng(7);
            Img im = make_img(rng, 0);
            try { auto j = bt->submit(im.px.data(), im.h, im.w, 1, nullptr); std::vector<uint8_t> o(im.px.size()); double sc[7]; std::string e; (void)bt->poll(j, -1, o.data(), sc, nullptr, &e); }
            catch (const Error&) { delete bt; bt = nullptr; }
        }
        CHECK(bt != nullptr);
        if (bt) {
            burst(*bt, 4, 12, 1, 3, 1); burst(*bt, 4, 12, 2, 4, 1);
            CHECK(drained(*bt));
            const auto c = bt->counters();
            std::printf("failures: batches %ld failed %ld\n", c.batches, c.failed_batches);
            CHECK(c.failed_batches > 0);
            delete bt;
        }
    }
    {   // 3. destruction with jobs pending, gathered, in flight, done-unread and overflowing; the handles are dropped afterwards
        StubBackend be(2);
        std::vector<Pending> left;
        {
            B bt(be);
            std::mt19937 rng(99);
            for (int k = 0; k < 40; ++k) {
                Pending p{make_img(rng, k & 1), nullptr};
                p.j = bt.submit(p.im.px.data(), p.im.h, p.im.w, p.im.jpeg, nullptr);
                left.push_back(std::move(p));
            }
            for (int k = 0; k < 3; ++k) {
                std::vector<uint8_t> out(left[k].im.px.size()); double sc[7]; std::string err;
                const int st = bt.poll(left[k].j, -1, out.data(), sc, nullptr, &err);
                CHECK(st == IRE_OK);
            }
            bt.release(left[5].j);
        }
        left.clear();
    }
    {   // 4. all four kinds at once, both shapes: every slot holds one key, every delivered result is its own job's
        StubBackend be(6);
        B bt(be);
        for (unsigned round = 0; round < 4; ++round) { all_kinds(bt, 4, 16, 700 + round); CHECK(drained(bt)); }
        const auto c = bt.counters();
        std::printf("all kinds: batches %ld overflowed %ld | launches %d group launches %d decodes %d upload decodes %d\n", c.batches, c.overflowed, be.launches.load(),
                    be.group_launches.load(), be.decodes.load(), be.upload_decodes.load());
        CHECK(c.failed_batches == 0 && be.launches.load() > 0 && be.group_launches.load() > 0 && be.decodes.load() > 0 && be.upload_decodes.load() > 0);
        CHECK(be.mixed.load() == 0 && be.key_mixed.load() == 0 && be.over_capacity.load() == 0);
    }
    return finish_main("batcher_stress");
}
