// buf_registry.hpp -- the debug poison switch and the process-wide registry of live allocations behind it; host only, no HIP, so
// tests/native/device_buf_test.cpp runs it on the CPU.  IRE_DEBUG_POISON=<0..255> (read once per process) makes both memory policies
// of common.hpp fill what they allocate with that byte, and makes every Buf of device_buf.hpp enter its allocation here: pointer,
// bytes, device or pinned, persistent or scratch.  ire_debug_poison_scratch walks the scratch entries.  Unset, a Buf tests one static
// flag per allocation and per free and nothing else happens.  (DESIGN.md "Buffer ownership".)
#pragma once
#include <cstddef>
#include <cstdlib>
#include <map>
#include <mutex>
#include <vector>

namespace ire {

// What an allocation is for.  Scratch: written by the call that reads it; any call may find anything there.  Persistent: device-resident
// state that its owner initialises once and later calls rely on.  Scratch is the default on purpose: a buffer nobody declared gets
// poisoned and fails loudly.
enum class BufUse : unsigned char { Scratch = 0, Persistent = 1 };

// the byte of IRE_DEBUG_POISON, or -1 when the variable is unset or anything but one to three decimal digits that say 0..255
// (no sign, no blank, no 0x: what Python's str.isdigit() and int() <= 255 accept, so a test can tell as the library does)
inline int debug_poison_byte() {
    static const int byte = [] {
        const char* v = std::getenv("IRE_DEBUG_POISON");
        if (!v || !v[0]) return -1;
        int b = 0, n = 0;
        for (; v[n]; ++n) {
            if (v[n] < '0' || v[n] > '9' || n >= 3) return -1;
            b = b * 10 + (v[n] - '0');
        }
        return b > 255 ? -1 : b;
    }();
    return byte;
}

class BufRegistry {
public:
    struct Entry { void* p; size_t bytes; bool pinned; bool persistent; };
    static bool on() { return debug_poison_byte() >= 0; }
    static BufRegistry& get() { static BufRegistry r; return r; }
    void add(void* p, size_t bytes, bool pinned, BufUse use) {
        std::lock_guard<std::mutex> lk(mu_);
        live_[p] = Entry{p, bytes, pinned, use == BufUse::Persistent};
    }
    void remove(void* p) {
        std::lock_guard<std::mutex> lk(mu_);
        live_.erase(p);
    }
    std::vector<Entry> snapshot() const {
        std::lock_guard<std::mutex> lk(mu_);
        std::vector<Entry> v;
        v.reserve(live_.size());
        for (const auto& kv : live_) v.push_back(kv.second);
        return v;
    }
    size_t size() const { std::lock_guard<std::mutex> lk(mu_); return live_.size(); }
private:
    mutable std::mutex mu_;
    std::map<void*, Entry> live_;      // by pointer: a moved Buf keeps its entry, the Buf it was moved from has none
};

}  // namespace ire
