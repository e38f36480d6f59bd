// batcher_groups_stress.cpp -- the batcher's FUSION jobs (csrc/batcher.hpp: submit_group and the backend's launch under a Group key)
// over the host-only STUB backend of tests/native/batcher_stub.hpp (which says what a stub fusion is), built with ThreadSanitizer and
// with AddressSanitizer + UBSan and run by tests/test_batcher_groups_native.py.
//
// What is driven: threads that submit pixel jobs and k = 2 / k = 3 fusion jobs of two shapes at once (a batch must hold one kind
// and one k: every staged image carries its kind in its first byte and the stub checks each batch it is given), slots that fill
// at max_batch / k jobs and never hold more than kGroupMaxJobs (one fused launch; the stub refuses a larger group as the engine
// does), more jobs than the slots hold before the first poll (overflow: the k views in the job's own vector, copied
// by the launcher; eviction of unread DONE slots), releases while pending / gathered / done, a batch whose launch fails (all its
// jobs fail, nobody else's), destruction with fusion jobs pending.
#include "batcher_stub.hpp"

// threads x jobs of mixed kinds, every job submitted before the first poll; polls in random order with short timeouts; thread
// `abandoner` gives up every other job.  -> how many polls ended in a failure status
static int burst(B& bt, int threads, int jobs, int abandoner, unsigned seed, bool fail_ok) {
    std::atomic<int> failed{0};
    std::vector<std::thread> th;
    for (int t = 0; t < threads; ++t)
        th.emplace_back([&, t] {
            std::mt19937 rng(seed + 977 * t);
            std::vector<PendingWork> pend;
            for (int n = 0; n < jobs; ++n) {
                PendingWork p{make_work(rng, 1 + (int)(rng() % 3), (n + t) & 1), nullptr};
                p.j = send(bt, p.wk);
                pend.push_back(std::move(p));
            }
            std::shuffle(pend.begin(), pend.end(), rng);
            size_t released = 0;
            while (!pend.empty()) {
                for (size_t i = 0; i < pend.size();) {
                    PendingWork& p = pend[i];
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

int main() {
    {   // 1. bursts past every slot: max_batch 6 (6 pixel jobs, 3 jobs of k = 2, 2 jobs of k = 3 per slot), three kinds x two shapes
        StubBackend be(6); be.tagged = true;
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
        StubBackend be(8); be.tagged = true;
        B bt(be);
        std::mt19937 rng(5);
        std::vector<PendingWork> p;
        for (int n = 0; n < 3; ++n) { p.push_back(PendingWork{make_work(rng, 3, 0), nullptr}); p.back().j = send(bt, p.back().wk); }
        for (auto& x : p) { std::string err; CHECK(poll_one(bt, x, &err) == IRE_OK); }
        CHECK(be.over_capacity.load() == 0 && be.mixed.load() == 0 && be.group_launches.load() >= 2);
        StubBackend small(2); small.tagged = true;
        B bs(small);
        Work wk = make_work(rng, 3, 0);
        bool refused = false;
        try { (void)send(bs, wk); } catch (const Error& e) { refused = e.code == IRE_ERR_INVALID_INPUT; }
        CHECK(refused && bs.queue_depth() == 0);
        wk = make_work(rng, 2, 0);
        PendingWork q{wk, send(bs, wk)};
        std::string err;
        CHECK(poll_one(bs, q, &err) == IRE_OK);
    }
    {   // 2b. max_batch 64: max_batch / k is 32 and 21, but a slot closes at kGroupMaxJobs = 16 jobs.  The device is kept busy by a
        // pixel batch, so the fusion slots gather until they are full: 34 jobs of k = 2 go as 16 + 16 + 2, 17 of k = 3 as 16 + 1
        StubBackend be(64); be.tagged = true;
        B bt(be);
        std::mt19937 rng(23);
        for (int k = 2; k <= 3; ++k) {
            be.compute_us = 30000;
            PendingWork busy{make_work(rng, 1, 1), nullptr};
            busy.j = send(bt, busy.wk);
            for (int i = 0; i < 2000 && bt.queue_depth() != 0; ++i) std::this_thread::sleep_for(std::chrono::milliseconds(1));      // (its slot has closed: it launches before anything gathered later)
            const int groups = be.group_launches.load(), total = k == 2 ? 34 : 17;
            std::vector<PendingWork> p;
            for (int n = 0; n < total; ++n) { p.push_back(PendingWork{make_work(rng, k, 0), nullptr}); p.back().j = send(bt, p.back().wk); }
            be.compute_us = 150;
            std::string err;
            CHECK(poll_one(bt, busy, &err) == IRE_OK);
            for (auto& x : p) CHECK(poll_one(bt, x, &err) == IRE_OK);
            CHECK(be.full_groups[k].load() == total / kGroupMaxJobs && be.group_launches.load() - groups == total / kGroupMaxJobs + 1);
        }
        CHECK(be.over_capacity.load() == 0 && be.mixed.load() == 0 && bt.counters().failed_batches == 0);
    }
    {   // 3. a pending fusion job is released; later jobs on the same batcher complete
        StubBackend be(6); be.tagged = true;
        B bt(be);
        std::mt19937 rng(17);
        PendingWork a{make_work(rng, 3, 1), nullptr};
        a.j = send(bt, a.wk);
        bt.release(a.j);
        CHECK(bt.counters().abandoned == 1);
        for (int n = 0; n < 4; ++n) {
            PendingWork b{make_work(rng, 2 + (n & 1), 1), nullptr};
            b.j = send(bt, b.wk);
            std::string err;
            CHECK(poll_one(bt, b, &err) == IRE_OK);
        }
        CHECK(drained(bt));
    }
    {   // 4. a batch whose launch fails: every job of it fails with the launch's message, pixel jobs beside it complete
        StubBackend be(6); be.tagged = true;
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
        StubBackend be(4); be.tagged = true;
        std::vector<PendingWork> left;
        {
            B bt(be);
            std::mt19937 rng(99);
            for (int n = 0; n < 30; ++n) {
                PendingWork p{make_work(rng, 1 + n % 3, n & 1), nullptr};
                p.j = send(bt, p.wk);
                left.push_back(std::move(p));
            }
            for (int n = 0; n < 3; ++n) { std::string err; CHECK(poll_one(bt, left[n], &err) == IRE_OK); }
            bt.release(left[5].j);
        }
        left.clear();
    }
    return finish_main("batcher_groups_stress");
}
