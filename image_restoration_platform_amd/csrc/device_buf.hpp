// device_buf.hpp -- who owns device and pinned memory, and how it grows; no HIP, no device code.  libire.so instantiates it over the two
// policies of common.hpp (DeviceMem, PinnedMem), tests/native/device_buf_test.cpp over a counting policy on the CPU.  A policy `Mem` has
// static void* alloc(size_t) (throws on failure) and static void free(void*) noexcept; one of pinned memory also says
// static constexpr bool kPinned = true (a policy without the member counts as device memory).  Under
// IRE_DEBUG_POISON every live allocation of a Buf is entered in buf_registry.hpp's registry, as scratch unless its site says
// BufUse::Persistent; a Buf keeps that use through reset and grow.  Two guarantees (DESIGN.md "Buffer ownership"):
// an engine scratch buffer or group is EMPTY after a failed grow, never dangling (the caller is told "service unavailable", calls again,
// and the capacity check sends it back into the grow); a batcher slot is UNCHANGED after a failed reserve.
#pragma once
#include <cstddef>
#include <cstdint>
#include <type_traits>
#include <utility>
#include <vector>

#include "buf_registry.hpp"
#include "conv_kind.hpp"

namespace ire {

// whether a policy's memory is pinned host memory: its kPinned, false where it has none
template <class Mem, class = void> struct mem_pinned : std::false_type {};
template <class Mem> struct mem_pinned<Mem, std::void_t<decltype(Mem::kPinned)>> : std::bool_constant<Mem::kPinned> {};

// move-only owner of one allocation (a zero-byte request allocates 16 bytes)
template <class Mem>
class Buf {
public:
    Buf() = default;
    explicit Buf(BufUse use) : use_(use) {}      // empty, for a later grow
    explicit Buf(size_t bytes, BufUse use = BufUse::Scratch) : bytes_(bytes ? bytes : 16), use_(use) {
        p_ = Mem::alloc(bytes_);                 // (a throw: nothing allocated, nothing entered)
        if (BufRegistry::on()) BufRegistry::get().add(p_, bytes_, mem_pinned<Mem>::value, use_);
    }
    Buf(Buf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)), use_(o.use_) {}
    Buf& operator=(Buf&& o) noexcept {
        if (this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); bytes_ = std::exchange(o.bytes_, 0); use_ = o.use_; }
        return *this;
    }
    ~Buf() { reset(); }
    template <class T> T* get() const { return static_cast<T*>(p_); }
    size_t bytes() const { return bytes_; }
    BufUse use() const { return use_; }
    explicit operator bool() const { return p_ != nullptr; }
    void reset() noexcept {
        if (p_) {
            if (BufRegistry::on()) BufRegistry::get().remove(p_);      // before the free: the address may be handed out again at once
            Mem::free(p_);
        }
        p_ = nullptr; bytes_ = 0;
    }
    // Room for `need` bytes: nothing when there is, else `want` (>= need) bytes in place of the old ones; true = reallocated.  The old
    // memory goes FIRST (allocating before freeing would double the peak of the largest shapes) and the buffer is empty while the
    // allocation runs, so a throw leaves it empty.
    bool grow(size_t need, size_t want) { if (need <= bytes_) return false; reset(); *this = Buf(want, use_); return true; }
    bool grow(size_t need) { return grow(need, need); }
private:
    void* p_ = nullptr;
    size_t bytes_ = 0;
    BufUse use_ = BufUse::Scratch;
};

// move-only owner of any number of allocations (what it hands out are views)
template <class Mem>
class BufSet {
public:
    template <class T> T* alloc(size_t bytes, BufUse use = BufUse::Scratch) {
        v_.emplace_back();                  // the place first: a throw below leaves an empty entry, not an unowned allocation
        v_.back() = Buf<Mem>(bytes, use);
        return v_.back().template get<T>();
    }
    size_t bytes() const { size_t b = 0; for (const Buf<Mem>& x : v_) b += x.bytes(); return b; }
    void clear() noexcept { v_.clear(); }
private:
    std::vector<Buf<Mem>> v_;
};

// The one grow rule of per-batch scratch: room for a whole batch of the shape when that is small (the first batch of a shape
// allocates, the later ones never do), else what was asked for.
inline size_t batch_room(size_t need, size_t full) { return full <= ((size_t)256 << 20) ? full : need; }

// ---- buffer groups of the engine: several buffers behind one capacity.  regrow empties the group first (memory freed, views null,
// capacities zero), then builds a complete new one aside (a throw frees what that had got) and takes it over. ------------------------
// staging of the host entry points and the classifier's outputs: capacity in images x pixels
template <class Mem>
struct IoBufs {
    BufSet<Mem> mem;
    uint8_t *in = nullptr, *out = nullptr, *jpeg = nullptr;
    unsigned long long* sums = nullptr;       // sums | tickets | workgroup partials (classifier.hpp): `sums_bytes` whatever the capacity
    double* scores = nullptr;
    int32_t* label = nullptr;
    float *cond = nullptr, *film = nullptr;
    size_t cap_imgs = 0, cap_px = 0;
    void regrow(size_t imgs, size_t px, size_t sums_bytes) {
        *this = IoBufs{};
        IoBufs g;
        g.in = g.mem.template alloc<uint8_t>(imgs * px * 3);
        g.out = g.mem.template alloc<uint8_t>(imgs * px * 3);
        g.jpeg = g.mem.template alloc<uint8_t>(imgs);
        g.sums = g.mem.template alloc<unsigned long long>(sums_bytes, BufUse::Persistent);      // cleared once by ensure_io: the tickets clean themselves
        g.scores = g.mem.template alloc<double>(imgs * 7 * 8);
        g.label = g.mem.template alloc<int32_t>(imgs * 4);
        g.cond = g.mem.template alloc<float>(imgs * 8 * 4);
        g.film = g.mem.template alloc<float>(imgs * kFilmDim * 4);
        g.cap_imgs = imgs; g.cap_px = px;
        *this = std::move(g);
    }
};
// fusion scratch (fusion.hip): capacity in view sets x pixels.  Per set: 3 luma planes, 3 quarter-res planes (pitch: a multiple of
// 4), `sad_words` per-workgroup SAD sums (coarse and fine take turns), coarse[3][2] + shifts[3][2] + a ticket, a blend table.
template <class Mem>
struct FuseBufs {
    BufSet<Mem> mem;
    uint8_t *L = nullptr, *Q = nullptr;
    unsigned *sad = nullptr, *wlut = nullptr;
    int* misc = nullptr;                      // [sets][6] coarse | [sets][6] shifts | [sets] tickets
    size_t cap_px = 0;
    int cap_sets = 0;
    void regrow(int sets, size_t px, size_t sad_words) {
        *this = FuseBufs{};
        FuseBufs g;
        const size_t cs = (size_t)sets;
        g.L = g.mem.template alloc<uint8_t>(cs * 3 * px);
        g.Q = g.mem.template alloc<uint8_t>(cs * 3 * (px / 16 + px / 64 + 16) + 64);      // (w >= 64: the pitch adds at most 3 to a row of >= 16)
        g.sad = g.mem.template alloc<unsigned>(sizeof(unsigned) * cs * sad_words);
        g.misc = g.mem.template alloc<int>(sizeof(int) * cs * 16, BufUse::Persistent);      // cleared once by fuse_reserve: the tickets clean themselves
        g.wlut = g.mem.template alloc<unsigned>(sizeof(unsigned) * cs * 256);
        g.cap_px = px; g.cap_sets = sets;
        *this = std::move(g);
    }
};

// ---- the activation workspace of one lane as a table: what Engine::ensure_workspace allocates, in its order.  Slots below 32 are
// level * 8 + b (engine.hpp buf_id): b 0..3 = act[level][b], 4 = skip[level]. -----------------------------------------------------------
constexpr int WS_STATS = 32, WS_STATS2 = 33, WS_AB = 34;
struct WsEntry { int slot; size_t bytes; };
inline std::vector<WsEntry> lane_workspace(int images_per_lane, int h, int w) {
    const size_t per = (size_t)images_per_lane;
    std::vector<WsEntry> t;
    for (int l = 0; l < 4; ++l)
        for (int b = 0; b < (l < 3 ? 5 : 4); ++b) t.push_back({l * 8 + b, per * (h >> l) * (w >> l) * kWidths[l] * 2});
    for (int s : {WS_STATS, WS_STATS2}) t.push_back({s, per * gn_partials(h, w) * 4});
    t.push_back({WS_AB, per * 256 * 2 * sizeof(float)});
    return t;
}
// device bytes one more image of a shape costs (Engine::bytes_per_image): its lane workspace and its two staging images (IoBufs in / out)
inline size_t workspace_bytes_per_image(int h, int w) {
    size_t b = (size_t)h * w * 3 * 2;
    for (const WsEntry& e : lane_workspace(1, h, w)) b += e.bytes;
    return b;
}

// ---- staging of one batcher slot (api.cpp HipBatchBackend; batcher.hpp's SlotBufs holds views of the pinned half).  `fixed`: the
// per-slot arrays sized by max_batch exist; `cap`: bytes of in / out per direction. -----------------------------------------------------
template <class Dev, class Pin>
struct SlotMem {
    Buf<Dev> d_in, d_out, d_txt, d_jp;        // d_txt: the results as text, when the engine delivers text
    Buf<Pin> pin_in, pin_out, pin_jp, pin_sc, pin_sc_in;
    size_t cap = 0;
    bool fixed = false;
    // STRONG guarantee: everything new is complete in `n` before anything old is touched; a throw half way (out of pinned memory at
    // the fifth slot) frees `n` and leaves the slot as it was.
    void reserve(size_t bytes, int max_batch, bool text) {
        const size_t mb = (size_t)max_batch;
        const bool want_fixed = !fixed, want_img = bytes > cap;
        SlotMem n;
        if (want_fixed) { n.pin_jp = Buf<Pin>(mb); n.pin_sc = Buf<Pin>(sizeof(double) * 7 * mb); n.pin_sc_in = Buf<Pin>(sizeof(double) * 7 * mb); n.d_jp = Buf<Dev>(mb); }
        if (want_img) { n.pin_in = Buf<Pin>(bytes); n.pin_out = Buf<Pin>(bytes); n.d_in = Buf<Dev>(bytes); n.d_out = Buf<Dev>(bytes); }
        if (want_img && text) n.d_txt = Buf<Dev>(bytes + 256 * mb);
        if (want_fixed) { pin_jp = std::move(n.pin_jp); pin_sc = std::move(n.pin_sc); pin_sc_in = std::move(n.pin_sc_in); d_jp = std::move(n.d_jp); fixed = true; }
        if (want_img) { pin_in = std::move(n.pin_in); pin_out = std::move(n.pin_out); d_in = std::move(n.d_in); d_out = std::move(n.d_out); d_txt = std::move(n.d_txt); cap = bytes; }
    }
};

}  // namespace ire
