// batcher_uploads_stress.cpp -- the batcher's UPLOAD jobs (csrc/batcher.hpp: submit_upload, the backend's upload_plan and its decode
// under an upload's key) over the host-only STUB backend of tests/native/batcher_stub.hpp (which says what a stub upload is), built with
// ThreadSanitizer and with AddressSanitizer + UBSan and run by tests/test_batcher_uploads_native.py.
//
// What is driven: threads that submit uploads of several keys, plain files and pixels of two output shapes at once (a batch holds
// one kind and, for uploads, one key); a flagged upload in the middle of a batch (it fails alone); uploads the plan refuses and
// uploads that break the room rule (no job); an upload whose staging fails after it got its place; releases while gathering and
// while in flight; more jobs than the slots hold before the first poll (the overflow path); destruction with jobs pending.
#include "batcher_stub.hpp"

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
        bad[F_MAGIC] = 0;
        try { bt.submit_upload(bad.data(), bad.size(), 64, nullptr); CHECK(!"refused"); } catch (const Error& e) { CHECK(e.code == IRE_ERR_INVALID_INPUT && e.msg == "invalid: not a stub file"); }
        try { bt.submit_upload(im.file.data(), im.file.size(), 0, nullptr); CHECK(!"refused"); } catch (const Error& e) { CHECK(e.code == IRE_ERR_INVALID_INPUT); }
        bad = im.file; bad[F_ROOM] = 1;
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
    return finish_main("batcher_uploads_stress");
}
