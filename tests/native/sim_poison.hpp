// sim_poison.hpp -- "--poison BYTE" of the decoder and encoder simulators.  The simulators stand for LDS and for device scratch with
// std::vector, which starts as zero; the device finds there whatever the last kernel left.  With the option in front of a program's mode,
// everything that stands for LDS or for scratch that the launch code does NOT clear is made by dirty<T>(n) and starts as that byte.
// What the launch code does clear (status words, the coefficient scratch, the histograms) stays a plain zeroed vector of that extent.
// No result may depend on the byte: the tests compare every poisoned run with the plain one, under the sanitizers.
#pragma once
#include <cstdlib>
#include <cstring>
#include <vector>

namespace simpoison {

inline int& poison() { static int byte = -1; return byte; }      // -1: off (everything starts as zero, as before)

// strips a leading "--poison BYTE"
inline void take_poison(int& argc, char**& argv) {
    if (argc >= 3 && !std::strcmp(argv[1], "--poison")) { poison() = std::atoi(argv[2]) & 255; argv[2] = argv[0]; argc -= 2; argv += 2; }
}

template <class T>
inline void soil(T* p, size_t n) { if (poison() >= 0 && n) std::memset(static_cast<void*>(p), poison(), n * sizeof(T)); }

// n objects that stand for uninitialised device memory or LDS
template <class T>
inline std::vector<T> dirty(size_t n) {
    std::vector<T> v(n);
    soil(v.data(), n);
    return v;
}

}  // namespace simpoison
