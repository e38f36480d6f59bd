// batcher_files_stress.cpp -- the batcher's FILE jobs (csrc/batcher.hpp: submit_file and the backend hooks file_plan / file_stage /
// decode / file_status) over the host-only STUB backend of tests/native/batcher_stub.hpp (which says what a stub file is), built with
// ThreadSanitizer and with AddressSanitizer + UBSan and run by tests/test_batcher_files_native.py.
//
// What is driven: threads that submit files and pixels of two shapes at once (a batch must never hold both kinds), a flagged file
// in the middle of a batch (it fails alone, with the decoder's status in its message), files the plan refuses and files larger than
// their pixels (no job), a file whose staging fails after it got its place (fails alone), releases while gathering, more file jobs
// than the slots hold before the first poll (the overflow path: staged into the job's own vector, copied by the launcher).
#include "batcher_stub.hpp"

// threads x jobs, every job submitted before the first poll; kinds and shapes mixed; thread `abandoner` gives up every other job
static void burst(B& bt, int threads, int jobs, int abandoner, unsigned seed, bool files_only) {
    std::vector<std::thread> th;
    for (int t = 0; t < threads; ++t)
        th.emplace_back([&, t] {
            std::mt19937 rng(seed + 977 * t);
            std::vector<Pending> pend;
            for (int k = 0; k < jobs; ++k) {
                const unsigned r = rng() % 16;
                const Kind kind = r == 0 ? FILE_FLAGGED : r == 1 ? FILE_STAGE_FAILS : (files_only || (r & 1)) ? FILE_OK : PIXELS;
                Pending p{make_img(rng, (k + t) & 1, kind), nullptr};
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

int main() {
    {   // 1. mixed file / pixel submitters, two shapes, flagged and stage-failing files among them, an abandoner; past every slot
        StubBackend be(2);
        B bt(be);
        for (unsigned round = 0; round < 6; ++round) {
            burst(bt, 4, 16, (int)(round % 4), 1 + 10 * round, false);
            CHECK(drained(bt));
        }
        const auto c = bt.counters();
        std::printf("mixed: batches %ld overflowed %ld evicted %ld abandoned %ld decodes %d mixed %d\n", c.batches, c.overflowed, c.evicted, c.abandoned, be.decodes.load(), be.mixed.load());
        CHECK(c.overflowed > 0 && c.abandoned > 0 && c.failed_batches == 0 && be.decodes.load() > 0);
        CHECK(be.mixed.load() == 0);                     // no batch held files and pixels
    }
    {   // 2. a flagged file in the middle of one batch of four: it fails alone
        StubBackend be(4);
        B bt(be);
        std::mt19937 rng(5);
        std::vector<Pending> ps;
        for (int k = 0; k < 4; ++k) ps.push_back(Pending{make_img(rng, 0, k == 1 ? FILE_FLAGGED : FILE_OK), nullptr});
        for (auto& p : ps) p.j = send(bt, p.im);
        for (auto& p : ps) {
            std::vector<uint8_t> out(p.im.px.size()); double sc[7]; std::string err;
            finish(p, bt.poll(p.j, -1, out.data(), sc, nullptr, &err), out, sc, err);
        }
        const auto c = bt.counters();
        std::printf("flagged: batches %ld failed %ld\n", c.batches, c.failed_batches);
        CHECK(c.batches >= 1 && c.failed_batches == 0);  // (one batch of four unless the submitter was held up for longer than the linger)
    }
    {   // 3. files that create no job: refused by the plan, larger than their pixels; then the batcher serves on
        StubBackend be(2);
        B bt(be);
        std::mt19937 rng(6);
        Img im = make_img(rng, 1, FILE_OK);
        std::vector<uint8_t> bad = im.file;
        bad[F_MAGIC] = 0;
        try { bt.submit_file(bad.data(), bad.size(), nullptr); CHECK(!"refused"); } catch (const Error& e) { CHECK(e.code == IRE_ERR_INVALID_INPUT && e.msg == "invalid: not a stub file"); }
        bad = im.file; bad[F_ROOM] = 1;
        try { bt.submit_file(bad.data(), bad.size(), nullptr); CHECK(!"too large"); }
        catch (const Error& e) { CHECK(e.code == IRE_ERR_INVALID_INPUT && e.msg.find("larger than its pixels") != std::string::npos); }
        CHECK(bt.queue_depth() == 0);
        Pending p{im, nullptr};
        p.j = send(bt, p.im);
        std::vector<uint8_t> out(im.px.size()); double sc[7]; std::string err;
        finish(p, bt.poll(p.j, -1, out.data(), sc, nullptr, &err), out, sc, err);
    }
    {   // 4. release while gathering, files only, and the overflow path: 4 x 16 file jobs before the first poll over 8 slots of 2
        StubBackend be(2);
        B bt(be);
        std::mt19937 rng(8);
        for (int k = 0; k < 6; ++k) { Img im = make_img(rng, k & 1, FILE_OK); auto j = send(bt, im); if (k & 1) bt.release(j); else { std::vector<uint8_t> o(im.px.size()); double sc[7]; std::string e; CHECK(bt.poll(j, -1, o.data(), sc, nullptr, &e) == IRE_OK); verify(im, o, sc); } }
        for (unsigned round = 0; round < 4; ++round) { burst(bt, 4, 16, (int)(round % 4), 500 + round, true); CHECK(drained(bt)); }
        const auto c = bt.counters();
        std::printf("files only: batches %ld overflowed %ld evicted %ld abandoned %ld\n", c.batches, c.overflowed, c.evicted, c.abandoned);
        CHECK(c.overflowed > 0 && c.abandoned > 0 && c.failed_batches == 0);
    }
    {   // 5. destruction with file jobs pending, gathered, in flight and overflowing
        StubBackend be(2);
        std::vector<Pending> left;
        {
            B bt(be);
            std::mt19937 rng(99);
            for (int k = 0; k < 40; ++k) { Pending p{make_img(rng, k & 1, k % 7 == 3 ? FILE_FLAGGED : FILE_OK), nullptr}; p.j = send(bt, p.im); left.push_back(std::move(p)); }
            bt.release(left[5].j);
        }
        left.clear();
    }
    return finish_main("batcher_files_stress");
}
