// batcher_icc_stress.cpp -- upload jobs whose files carry an ICC profile, in the batcher (csrc/batcher.hpp) over the host-only STUB
// backend of tests/native/batcher_stub.hpp, built with ThreadSanitizer and with AddressSanitizer + UBSan and run by
// tests/test_batcher_icc_native.py.  The profile is NOT part of an upload's slot key: a job's tables travel with its head (what the
// backend's upload_plan returns and its decode is handed back), so uploads of one key with different profiles, or none, share a slot
// and each is converted by its own tables.
//
// The stub of a profile: the first pixel byte of a stub upload is its profile id (0: none), its "tables" are 16 bytes made of that id, and
// the stub's decode adds table[p % 16] to every byte p of the job's image -- a job converted with another job's tables, or with none,
// gives wrong bytes.
#include <type_traits>

#include "batcher_stub.hpp"

struct IccHead : StubHead { int id = 0; uint8_t table[16] = {}; };
static_assert(std::is_standard_layout<StubHead>::value, "the stub's decode reads a head through a StubHead pointer");
static void make_table(int id, uint8_t t[16]) { for (int k = 0; k < 16; ++k) t[k] = id ? (uint8_t)(id * 7 + k * 13 + 1) : 0; }

struct IccStubBackend : StubBackend {
    std::atomic<int> converted{0}, wrong_tables{0}, shared_decodes{0};
    explicit IccStubBackend(int mb) : StubBackend(mb) {}
    std::shared_ptr<void> upload_plan(const uint8_t* file, size_t bytes, int max_dim, int* h, int* w, size_t* room, int key[4]) {
        auto base = StubBackend::upload_plan(file, bytes, max_dim, h, w, room, key);
        auto head = std::make_shared<IccHead>();
        static_cast<StubHead&>(*head) = *static_cast<StubHead*>(base.get());
        head->id = file[kHead] ^ 0x33;
        make_table(head->id, head->table);
        return std::shared_ptr<void>(head, static_cast<StubHead*>(head.get()));      // (what the stub's decode casts back)
    }
    void decode(SlotBufs& b, int first, int count, const SlotKey& key, void* const* heads, const size_t* used) {
        StubBackend::decode(b, first, count, key, heads, used);
        if (key.kind != JobKind::Upload) return;
        StubSlot& ss = *static_cast<StubSlot*>(b.impl);
        const size_t ib = key.in_bytes();
        int ids = 0, last = -1;
        for (int i = 0; i < count; ++i) {
            const IccHead& hd = *static_cast<const IccHead*>(static_cast<const StubHead*>(heads[i]));
            uint8_t want[16];
            make_table(hd.id, want);
            if (std::memcmp(want, hd.table, 16)) ++wrong_tables;      // the head that came back is the one this job's plan made
            if (hd.id != last) { ++ids; last = hd.id; }
            if (!hd.id) continue;
            ++converted;
            for (size_t p = 0; p < used[i]; ++p) ss.d_in[ib * (first + i) + p] = (uint8_t)(ss.d_in[ib * (first + i) + p] + hd.table[p % 16]);
        }
        if (ids > 1) ++shared_decodes;       // one push held jobs of different profiles
    }
};
using IB = Batcher<IccStubBackend>;

static bool all_gone(IB& bt) {       // batcher_stub.hpp's drained, for this backend
    for (int i = 0; i < 200 && bt.queue_depth() != 0; ++i) std::this_thread::sleep_for(std::chrono::milliseconds(1));
    return bt.queue_depth() == 0;
}

struct IccJob { Img im; int id; std::shared_ptr<Job> j; };
static IccJob make_job(std::mt19937& rng, int id, int orientation, int max_dim) {
    IccJob q{make_img(rng, 0, UPLOAD_OK, orientation, max_dim), id, nullptr};
    q.im.px[0] = (uint8_t)id;
    q.im.file[kHead] = (uint8_t)(id ^ 0x33);
    return q;
}
static void check(IB& bt, IccJob& q) {
    std::vector<uint8_t> out(q.im.px.size());
    double sc[7]; std::string err;
    const int st = bt.poll(q.j, -1, out.data(), sc, nullptr, &err);
    CHECK(st == IRE_OK);
    uint8_t t[16];
    make_table(q.id, t);
    bool ok = st == IRE_OK;
    for (size_t p = 0; p < out.size() && ok; ++p) ok = out[p] == f_px((uint8_t)(staged(q.im, p) + t[p % 16]), p);
    CHECK(ok);
}

int main() {
    {   // 1. two uploads of one key with different profiles, submitted while the device computes: ONE slot, one batch, each by its own tables
        IccStubBackend be(4);
        IB bt(be);
        std::mt19937 rng(11);
        for (int round = 0; round < 8; ++round) {
            be.compute_us = 20000;
            Img busy = make_img(rng, 1);
            auto bj = bt.submit(busy.px.data(), busy.h, busy.w, busy.jpeg, nullptr);
            std::this_thread::sleep_for(std::chrono::milliseconds(3));      // (in flight: what follows gathers)
            const int before = be.launches.load(), decodes = be.upload_decodes.load();
            IccJob a = make_job(rng, 1 + round, 6, 64), b = make_job(rng, 101 + round, 6, 64), c = make_job(rng, 0, 6, 64);
            a.j = bt.submit_upload(a.im.file.data(), a.im.file.size(), 64, nullptr);
            b.j = bt.submit_upload(b.im.file.data(), b.im.file.size(), 64, nullptr);
            c.j = bt.submit_upload(c.im.file.data(), c.im.file.size(), 64, nullptr);
            be.compute_us = 150;
            check(bt, a); check(bt, b); check(bt, c);
            CHECK(be.launches.load() - before == 1);            // the three jobs were one batch
            CHECK(be.upload_decodes.load() - decodes >= 1);
            std::vector<uint8_t> out(busy.px.size()); double sc[7]; std::string err;
            CHECK(bt.poll(bj, -1, out.data(), sc, nullptr, &err) == IRE_OK);
        }
        CHECK(be.shared_decodes.load() > 0 && be.wrong_tables.load() == 0 && be.key_mixed.load() == 0 && be.mixed.load() == 0);
        CHECK(all_gone(bt));
    }
    {   // 2. many submitters, profiles and keys at random, every job polled
        IccStubBackend be(4);
        IB bt(be);
        std::vector<std::thread> th;
        for (int t = 0; t < 4; ++t)
            th.emplace_back([&, t] {
                std::mt19937 rng(100 + t);
                for (int round = 0; round < 12; ++round) {
                    std::vector<IccJob> js;
                    for (int k = 0; k < 6; ++k) js.push_back(make_job(rng, (int)(rng() % 3) * (1 + (int)(rng() % 80)), (rng() & 1) ? 6 : 1, 64));
                    for (auto& q : js) q.j = bt.submit_upload(q.im.file.data(), q.im.file.size(), q.im.max_dim, nullptr);
                    for (auto& q : js) check(bt, q);
                }
            });
        for (auto& t : th) t.join();
        std::printf("random: upload decodes %d converted %d shared %d\n", be.upload_decodes.load(), be.converted.load(), be.shared_decodes.load());
        CHECK(be.converted.load() > 0 && be.wrong_tables.load() == 0 && be.key_mixed.load() == 0 && be.mixed.load() == 0);
        CHECK(all_gone(bt));
    }
    return finish_main("batcher_icc_stress");
}
