// device_buf_test.cpp -- csrc/device_buf.hpp on the CPU (tests/test_device_buf.py builds this at -O2 and under ASan + UBSan).  Test
// infrastructure: libire.so includes the same header over hipMalloc / hipHostMalloc; here the memory policy counts.
//   (no argument)  every ownership check below; prints "ok"
//   dump           the workspace table and bytes-per-image lines the Python driver compares with its own restatement of the parent
//   registry       csrc/buf_registry.hpp under IRE_DEBUG_POISON (the driver sets it; also built under ThreadSanitizer): an entry per live
//                  allocation, none after free, reset, a failed grow or for a moved-from buffer, the persistent flag, two threads; prints "ok"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "../../image_restoration_platform_amd/csrc/device_buf.hpp"

using namespace ire;

// The counting policy: the live set, a log of every call, a count of frees of something not live, and an allocation told to throw.
struct Count {
    struct Ev { char what; size_t bytes; };       // 'a' bytes | 'f' 0
    static std::set<void*> live;
    static std::vector<Ev> log;
    static int bad_frees, calls, fail_at;         // fail_at: the calls-th allocation from now throws (0: none)
    static void* alloc(size_t bytes) {
        if (fail_at && ++calls == fail_at) { fail_at = 0; throw std::runtime_error("out of memory"); }
        void* p = std::malloc(bytes);
        live.insert(p);
        log.push_back({'a', bytes});
        return p;
    }
    static void free(void* p) noexcept {
        log.push_back({'f', 0});
        if (!live.erase(p)) { ++bad_frees; return; }
        std::free(p);
    }
    static void fail(int k) { calls = 0; fail_at = k; }
    static void restart() { log.clear(); calls = 0; fail_at = 0; }
};
std::set<void*> Count::live;
std::vector<Count::Ev> Count::log;
int Count::bad_frees = 0, Count::calls = 0, Count::fail_at = 0;

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

template <class F>
static bool throws(F&& f) {
    try { f(); } catch (const std::runtime_error&) { return true; }
    return false;
}
static std::string log_text() {
    std::string s;
    for (const Count::Ev& e : Count::log) s += e.what == 'a' ? "a" + std::to_string(e.bytes) + " " : "f ";
    return s;
}

static void test_buf() {
    Count::restart();
    {
        Buf<Count> z(0);
        CHECK(z.bytes() == 16 && z.get<char>() && log_text() == "a16 ");          // a zero-byte request becomes 16 bytes
        Buf<Count> e;
        CHECK(!e && e.bytes() == 0 && e.get<char>() == nullptr);
        CHECK(e.grow(0) == false && !e);                                           // nothing asked of nothing: still nothing
    }
    CHECK(Count::live.empty());
    Count::restart();
    {
        Buf<Count> b;
        CHECK(b.grow(100, 400) && b.bytes() == 400 && Count::live.size() == 1);
        char* p = b.get<char>();
        CHECK(!b.grow(400, 999) && !b.grow(7, 7) && b.get<char>() == p && b.bytes() == 400);        // below the capacity: no-op, same pointer
        CHECK(log_text() == "a400 ");
        CHECK(b.grow(401, 800) && b.bytes() == 800 && log_text() == "a400 f a800 " && Count::live.size() == 1);      // freed BEFORE the new one is allocated
        Count::fail(1);
        CHECK(throws([&] { b.grow(801, 1600); }));
        CHECK(!b && b.bytes() == 0 && b.get<char>() == nullptr && Count::live.empty());         // empty, not dangling
        CHECK(log_text() == "a400 f a800 f ");
        CHECK(b.grow(801, 1600) && b.bytes() == 1600 && Count::live.size() == 1);               // the retry goes back into the grow
        CHECK(b.grow(2000) && b.bytes() == 2000);
        // exactly one owner after a move
        Buf<Count> c(std::move(b));
        CHECK(!b && b.bytes() == 0 && c.bytes() == 2000 && Count::live.size() == 1);
        Buf<Count> d(32);
        d = std::move(c);
        CHECK(!c && d.bytes() == 2000 && Count::live.size() == 1);      // d's own 32 bytes were freed by the assignment
        d.reset();
        CHECK(!d && Count::live.empty());
        d.reset();
    }
    CHECK(Count::live.empty() && Count::bad_frees == 0);
}

static void test_bufset() {
    Count::restart();
    {
        BufSet<Count> s;
        CHECK(s.bytes() == 0);
        int* a = s.alloc<int>(40);
        char* b = s.alloc<char>(0);
        CHECK(a && b && s.bytes() == 56 && Count::live.size() == 2);
        Count::fail(1);
        CHECK(throws([&] { s.alloc<char>(8); }));
        CHECK(s.bytes() == 56 && Count::live.size() == 2);             // what it held it still holds
        BufSet<Count> t(std::move(s));
        CHECK(s.bytes() == 0 && t.bytes() == 56 && Count::live.size() == 2);
        BufSet<Count> u;
        u.alloc<char>(5);
        u = std::move(t);
        CHECK(u.bytes() == 56 && Count::live.size() == 2);
        u.clear();
        CHECK(u.bytes() == 0 && Count::live.empty());
    }
    {
        BufSet<Count> s;
        s.alloc<char>(1); s.alloc<char>(2);
    }
    CHECK(Count::live.empty() && Count::bad_frees == 0);
}

// every allocation of a regrow from a non-empty state fails in turn: the group is empty afterwards, nothing is live, nothing was freed
// twice, and the next regrow succeeds.  (The parent freed eight buffers, allocated eight and kept the old pointers and capacities on
// a throw: this is the case it fails by construction.)
constexpr size_t kSums = 4096;       // stands for cls_sums_bytes() (classifier.hpp): a fixed size whatever the capacity
static bool io_empty(const IoBufs<Count>& g) {
    return !g.in && !g.out && !g.jpeg && !g.sums && !g.scores && !g.label && !g.cond && !g.film && !g.cap_imgs && !g.cap_px && !g.mem.bytes();
}
static bool fuse_empty(const FuseBufs<Count>& g) { return !g.L && !g.Q && !g.sad && !g.misc && !g.wlut && !g.cap_px && !g.cap_sets && !g.mem.bytes(); }

static void test_groups() {
    {
        Count::restart();
        IoBufs<Count> g;
        CHECK(io_empty(g));
        g.regrow(8, 64 * 64, kSums);
        // the parent's eight requests, in its order (engine.cpp ensure_io): 2 x imgs px 3, imgs, sums, imgs 7 8, imgs 4, imgs 8 4, imgs 960 4
        CHECK(log_text() == "a98304 a98304 a8 a4096 a448 a32 a256 a30720 ");
        CHECK(g.cap_imgs == 8 && g.cap_px == 4096 && g.in && g.film && Count::live.size() == 8);
    }
    CHECK(Count::live.empty());
    for (int k = 1; k <= 9; ++k) {
        Count::restart();
        IoBufs<Count> g;
        g.regrow(2, 64, kSums);
        Count::fail(k);
        const bool threw = throws([&] { g.regrow(4, 256, kSums); });
        CHECK(threw == (k <= 8));                                      // eight allocations: the ninth never comes
        if (!threw) { Count::restart(); continue; }
        CHECK(io_empty(g) && Count::live.empty() && Count::bad_frees == 0);
        g.regrow(4, 256, kSums);
        CHECK(g.cap_imgs == 4 && g.cap_px == 256 && g.in && g.out && g.jpeg && g.sums && g.scores && g.label && g.cond && g.film && Count::live.size() == 8);
    }
    CHECK(Count::live.empty() && Count::bad_frees == 0);
    {
        Count::restart();
        FuseBufs<Count> g;
        g.regrow(2, 64 * 64, 2 * 64 * 81);
        // fusion.hip fuse_launch: sets 3 px | sets 3 (px/16 + px/64 + 16) + 64 | 4 sets sad_words | 4 sets 16 | 4 sets 256
        CHECK(log_text() == "a24576 a2080 a82944 a128 a2048 ");
        CHECK(g.cap_sets == 2 && g.cap_px == 4096);
    }
    for (int k = 1; k <= 6; ++k) {
        Count::restart();
        FuseBufs<Count> g;
        g.regrow(1, 4096, 100);
        Count::fail(k);
        const bool threw = throws([&] { g.regrow(3, 16384, 100); });
        CHECK(threw == (k <= 5));
        if (!threw) { Count::restart(); continue; }
        CHECK(fuse_empty(g) && Count::live.empty() && Count::bad_frees == 0);
        g.regrow(3, 16384, 100);
        CHECK(g.cap_sets == 3 && g.cap_px == 16384 && g.L && g.Q && g.sad && g.misc && g.wlut && Count::live.size() == 5);
    }
    CHECK(Count::live.empty() && Count::bad_frees == 0);
}

static void test_batch_room() {
    // the four parent expressions, `full <= 256 MiB ? full : need` each, as numbers:
    CHECK(batch_room(3145728, 25165824) == 25165824);          // ensure_io in bytes: 1 of 8 images of 1024^2: 8 images
    CHECK(batch_room(100663296, 402653184) == 100663296);      // ensure_pad: 2 of 8 images of 4096^2 (384 MiB a batch): what was asked
    CHECK(batch_room(1, 268435456) == 268435456);              // encode_window / ensure_enc_scratch: 256 MiB itself is still "small"
    CHECK(batch_room(1, 268435457) == 1);                      // one byte more is not
    CHECK(batch_room(268435455, 268435455) == 268435455 && batch_room(300000000, 300000000) == 300000000);
}

using Slot = SlotMem<Count, Count>;
struct SlotView { std::vector<void*> p; size_t cap; bool fixed; };
static SlotView view(const Slot& s) {
    return {{s.d_in.get<void>(), s.d_out.get<void>(), s.d_txt.get<void>(), s.d_jp.get<void>(), s.pin_in.get<void>(), s.pin_out.get<void>(),
             s.pin_jp.get<void>(), s.pin_sc.get<void>(), s.pin_sc_in.get<void>()}, s.cap, s.fixed};
}
static bool same(const SlotView& x, const SlotView& y) { return x.p == y.p && x.cap == y.cap && x.fixed == y.fixed; }

static void test_slot() {
    Count::restart();
    const SlotView empty{std::vector<void*>(9, nullptr), 0, false};
    for (int k = 1; k <= 10; ++k) {          // the first reserve: 4 per-slot arrays + 5 image buffers
        Slot s;
        CHECK(same(view(s), empty));
        Count::restart();
        Count::fail(k);
        const bool threw = throws([&] { s.reserve(1000, 4, true); });
        CHECK(threw == (k <= 9));
        if (threw) {
            CHECK(same(view(s), empty) && Count::live.empty());        // still empty, nothing leaked
            s.reserve(1000, 4, true);
        }
        Count::restart();
        CHECK(s.fixed && s.cap == 1000 && Count::live.size() == 9 && s.d_txt && s.pin_sc_in);
        const SlotView held = view(s);
        s.reserve(1000, 4, true);             // enough already: nothing moves
        CHECK(same(view(s), held) && Count::log.empty());
        for (int j = 1; j <= 5; ++j) {        // a larger shape: the 5 image buffers; every failure leaves the old ones in use
            Count::fail(j);
            CHECK(throws([&] { s.reserve(5000, 4, true); }));
            CHECK(same(view(s), held) && Count::live.size() == 9);
        }
        Count::restart();
        s.reserve(5000, 4, true);
        CHECK(log_text() == "a5000 a5000 a5000 a5000 a6024 f f f f f " && s.cap == 5000 && Count::live.size() == 9);      // new ones complete, THEN the old ones go
    }
    {
        Slot s;
        Count::restart();
        s.reserve(64, 8, false);              // pixels out: no text buffer
        CHECK(log_text() == "a8 a448 a448 a8 a64 a64 a64 a64 " && !s.d_txt && Count::live.size() == 8);
    }
    CHECK(Count::live.empty() && Count::bad_frees == 0);
}

// ---- the registry.  `Pin` is a second policy (pinned, thread-safe, no log) so that both kinds and two threads can be told apart. ----
struct Pin {
    static constexpr bool kPinned = true;
    static void* alloc(size_t bytes) { return std::malloc(bytes); }
    static void free(void* p) noexcept { std::free(p); }
};
static const BufRegistry::Entry* find(const std::vector<BufRegistry::Entry>& v, const void* p) {
    for (const BufRegistry::Entry& e : v) if (e.p == p) return &e;
    return nullptr;
}
// the registry holds exactly these buffers' allocations, with their sizes
template <class... B>
static bool holds(const B&... b) {
    const std::vector<BufRegistry::Entry> v = BufRegistry::get().snapshot();
    size_t n = 0;
    bool ok = true;
    auto one = [&](const void* p, size_t bytes) {
        if (!p) return;
        ++n;
        const BufRegistry::Entry* e = find(v, p);
        ok = ok && e && e->bytes == bytes;
    };
    (one(b.template get<void>(), b.bytes()), ...);
    return ok && v.size() == n;
}

static void test_registry() {
    BufRegistry& R = BufRegistry::get();
    CHECK(BufRegistry::on() && debug_poison_byte() == 90 && R.size() == 0);
    Count::restart();
    {
        Buf<Count> a(100), e;
        Buf<Pin> p(7, BufUse::Persistent);
        CHECK(holds(a, e, p));
        const auto v = R.snapshot();
        CHECK(!find(v, a.get<void>())->pinned && !find(v, a.get<void>())->persistent);           // scratch unless the site says otherwise
        CHECK(find(v, p.get<void>())->pinned && find(v, p.get<void>())->persistent && find(v, p.get<void>())->bytes == 7);
        // grow: the old entry goes, the new one has the new size and the buffer's use; below the capacity nothing changes
        CHECK(p.grow(8, 64) && holds(a, p) && find(R.snapshot(), p.get<void>())->persistent && p.use() == BufUse::Persistent);
        CHECK(!a.grow(50) && holds(a, p));
        CHECK(a.grow(101, 300) && holds(a, p) && find(R.snapshot(), a.get<void>())->bytes == 300);
        // an empty buffer declared persistent stays so through its first grow (Engine: d_zero_)
        Buf<Count> z(BufUse::Persistent);
        CHECK(holds(a, p, z) && z.grow(16) && holds(a, p, z) && find(R.snapshot(), z.get<void>())->persistent);
        // a failed grow: no entry, and none after the retry's predecessor either
        Count::fail(1);
        CHECK(throws([&] { a.grow(301, 600); }));
        CHECK(!a && holds(p, z));
        CHECK(a.grow(301, 600) && holds(a, p, z));
        // a throwing constructor enters nothing
        Count::fail(1);
        CHECK(throws([&] { Buf<Count> t(9); }));
        CHECK(holds(a, p, z));
        // a move: one entry, the same pointer; the moved-from buffer has none; the use travels with the allocation
        void* was = z.get<void>();
        Buf<Count> m(std::move(z));
        CHECK(!z && m.get<void>() == was && holds(a, p, m) && find(R.snapshot(), was)->persistent);
        Buf<Count> n(32);
        n = std::move(m);                       // n's own 32 bytes leave the registry with the assignment
        CHECK(!m && holds(a, p, n) && n.use() == BufUse::Persistent);
        n.reset();
        CHECK(holds(a, p));
        n.reset();
        CHECK(holds(a, p));
    }
    CHECK(R.size() == 0 && Count::live.empty() && Count::bad_frees == 0);
    {
        // sets and groups: an entry per allocation, the persistent ones where device_buf.hpp says
        BufSet<Count> s;
        int* x = s.alloc<int>(40);
        char* y = s.alloc<char>(0, BufUse::Persistent);
        auto v = R.snapshot();
        CHECK(v.size() == 2 && !find(v, x)->persistent && find(v, y)->persistent && find(v, y)->bytes == 16);
        Count::fail(1);
        CHECK(throws([&] { s.alloc<char>(8); }));
        CHECK(R.size() == 2);
        BufSet<Count> t(std::move(s));
        CHECK(R.size() == 2);
        t.clear();
        CHECK(R.size() == 0);
        IoBufs<Count> g;
        g.regrow(2, 64, kSums);
        v = R.snapshot();
        CHECK(v.size() == 8);
        for (const BufRegistry::Entry& e : v) CHECK(e.persistent == (e.p == (void*)g.sums));
        for (int k = 1; k <= 8; ++k) {
            Count::fail(k);
            CHECK(throws([&] { g.regrow(4, 256, kSums); }));
            CHECK(R.size() == 0);
            g.regrow(2, 64, kSums);
            CHECK(R.size() == 8);
        }
        FuseBufs<Count> f;
        f.regrow(1, 4096, 100);
        v = R.snapshot();
        CHECK(v.size() == 13);
        for (const BufRegistry::Entry& e : v) if (e.p != (void*)g.sums) CHECK(e.persistent == (e.p == (void*)f.misc));
        Slot sl;
        sl.reserve(1000, 4, true);
        CHECK(R.size() == 22);
        for (int j = 1; j <= 5; ++j) {          // a failed reserve leaves the slot, and the registry, as they were
            Count::fail(j);
            CHECK(throws([&] { sl.reserve(5000, 4, true); }));
            CHECK(R.size() == 22);
        }
        sl.reserve(5000, 4, true);
        CHECK(R.size() == 22 && find(R.snapshot(), sl.d_txt.get<void>())->bytes == 6024);
    }
    CHECK(R.size() == 0 && Count::live.empty() && Count::bad_frees == 0);
    {
        // two threads allocating, growing, moving and freeing at once while a third reads: every entry accounted for at every join
        std::vector<Buf<Pin>> kept[2];
        auto work = [&](int t) {
            for (int i = 0; i < 2000; ++i) {
                Buf<Pin> b(8 + (size_t)i % 64, (i & 1) ? BufUse::Persistent : BufUse::Scratch);
                b.grow(200);
                Buf<Pin> c(std::move(b));
                if (i % 100 == 0) kept[t].push_back(std::move(c));
            }
        };
        std::thread t0(work, 0), t1(work, 1);
        size_t seen = 0;
        for (int i = 0; i < 200; ++i) seen += R.snapshot().size();
        t0.join(); t1.join();
        (void)seen;
        CHECK(R.size() == 40);
        for (const BufRegistry::Entry& e : R.snapshot()) CHECK(e.pinned && !e.persistent && e.bytes == 200);
        kept[0].clear(); kept[1].clear();
    }
    CHECK(R.size() == 0);
}

static void dump() {
    const int shapes[4][3] = {{1, 16, 16}, {3, 64, 40}, {8, 1024, 1024}, {1, 8192, 8192}};
    for (const auto& s : shapes)
        for (int lanes = 1; lanes <= 3; ++lanes) {
            std::printf("ws %d %d %d %d", s[0], s[1], s[2], lanes);
            for (const WsEntry& e : lane_workspace((s[0] + lanes - 1) / lanes, s[1], s[2])) std::printf(" %d:%zu", e.slot, e.bytes);
            std::printf("\n");
        }
    const int hw[7][2] = {{16, 16}, {64, 40}, {1024, 1024}, {8192, 8192}, {16, 16}, {24, 4096}, {4096, 24}};
    for (const auto& s : hw) std::printf("bpi %d %d %zu\n", s[0], s[1], workspace_bytes_per_image(s[0], s[1]));
    std::printf("partials %zu %zu %zu\n", gn_partials(16, 16), gn_partials(17, 33), gn_partials(8192, 8192));
}

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "dump")) { dump(); return 0; }
    if (argc > 1 && !std::strcmp(argv[1], "registry")) { test_registry(); std::printf("ok\n"); return 0; }
    CHECK(!BufRegistry::on() && debug_poison_byte() == -1);       // the variable is unset: nothing below may enter the registry
    test_buf();
    test_bufset();
    test_groups();
    test_batch_room();
    test_slot();
    CHECK(BufRegistry::get().size() == 0);
    std::printf("ok\n");
    return 0;
}
