// icc.hip -- uploads that carry an ICC profile, converted to sRGB on the device: the all-integer transform icc_parse.hpp builds and
// states, applied in place to a batch of tightly packed RGB images.  One kernel, one launch whatever n: blockIdx.y is the image.
//
// The pass moves 2 x 3 bytes per pixel and is HBM-bound by design; what it must not do is lose that to LDS.  A pixel costs nine LDS
// gathers (three lin, three coarse, three last).  lin stays PACKED u16 (128 dwords a row, two a bank) rather than one dword per entry:
// lanes that read the same dword are served by one broadcast, and a packed row has half as many distinct dwords for a wave's 64
// addresses to spread over, which is what the classifier's one-dword-per-entry lin16 table paid for.  The nine matrix coefficients
// are wave-uniform and come through scalar loads, not LDS.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstring>

#include "icc.hpp"

namespace ire {

namespace {

constexpr int kThreads = 256;
constexpr int kIter = 16;               // 4-pixel groups a thread walks: a workgroup stages 6 KB of tables for 48 KB of pixels
constexpr int kGroupsPerBlock = kThreads * kIter;

struct alignas(4) Px4 { uint32_t a, b, c; };      // 4 pixels = 12 bytes = 3 dwords (fusion.hip's blend groups)

__device__ __forceinline__ uint32_t enc8(const uint8_t* coarse, const uint16_t* last, int y) {
    const uint32_t o = coarse[y >> 4];
    return o + ((uint32_t)y > (uint32_t)last[o] ? 1u : 0u);
}

// y_c = clamp((sum_k m[c][k] * lin[k][v_k] + 8192) >> 14, 0, 65535): |m| may reach 2^16 and lin 2^16 - 1, so a product needs 33 bits
// and the sum 35: 64-bit accumulation (DESIGN.md's 32-bit table names this one as NOT 32-bit)
__device__ __forceinline__ int mix(int m0, int m1, int m2, int l0, int l1, int l2) {
    const long long acc = (long long)m0 * l0 + (long long)m1 * l1 + (long long)m2 * l2 + 8192;
    const long long y = acc >> 14;
    return y < 0 ? 0 : y > 65535 ? 65535 : (int)y;
}

template <bool kGrey>
__device__ __forceinline__ void convert(uint32_t& r, uint32_t& g, uint32_t& b, const int* __restrict__ m, const uint16_t* lin, const uint8_t* lut,
                                        const uint8_t* coarse, const uint16_t* last) {
    if (kGrey) { r = g = b = lut[r]; return; }
    const int l0 = lin[r], l1 = lin[256 + g], l2 = lin[512 + b];
    r = enc8(coarse, last, mix(m[0], m[1], m[2], l0, l1, l2));
    g = enc8(coarse, last, mix(m[3], m[4], m[5], l0, l1, l2));
    b = enc8(coarse, last, mix(m[6], m[7], m[8], l0, l1, l2));
}

template <bool kGrey>
__device__ __forceinline__ void run_image(uint8_t* base, size_t npx, const uint8_t* __restrict__ table, const uint8_t* __restrict__ enc, uint32_t* lds) {
    uint16_t* s_lin = reinterpret_cast<uint16_t*>(lds);                  // [3][256] u16 | grey: 256 bytes
    uint8_t* s_lut = reinterpret_cast<uint8_t*>(lds);
    uint8_t* s_coarse = reinterpret_cast<uint8_t*>(lds + 384);           // [4096]
    uint16_t* s_last = reinterpret_cast<uint16_t*>(lds + 384 + 1024);    // [256]
    const int* m = reinterpret_cast<const int*>(table);                  // (wave-uniform: scalar loads)
    if (kGrey) {
        for (int i = threadIdx.x; i < 64; i += kThreads) lds[i] = reinterpret_cast<const uint32_t*>(table)[i];
    } else {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(table + offsetof(IccMatrixTable, lin));
        for (int i = threadIdx.x; i < 384; i += kThreads) lds[i] = src[i];
        const uint32_t* e = reinterpret_cast<const uint32_t*>(enc);
        for (int i = threadIdx.x; i < 1024 + 128; i += kThreads) lds[384 + i] = e[i];
    }
    __syncthreads();
    // pixel k starts at base + 3 k: on a dword when k = base (mod 4).  `head` pixels in front of the first such one and the `tail`
    // pixels behind the last whole group go byte by byte (the first workgroup of the image), the groups between as three dwords
    const size_t mis = (size_t)(reinterpret_cast<uintptr_t>(base) & 3);
    const size_t head = mis < npx ? mis : npx;
    const size_t ngroups = (npx - head) / 4;
    const size_t tail = npx - head - 4 * ngroups;
    if (blockIdx.x == 0 && threadIdx.x < head + tail) {
        const size_t p = threadIdx.x < head ? threadIdx.x : head + 4 * ngroups + (threadIdx.x - head);
        uint8_t* q = base + 3 * p;
        uint32_t r = q[0], g = q[1], b = q[2];
        convert<kGrey>(r, g, b, m, s_lin, s_lut, s_coarse, s_last);
        q[0] = (uint8_t)r; q[1] = (uint8_t)g; q[2] = (uint8_t)b;
    }
    Px4* grp = reinterpret_cast<Px4*>(base + 3 * head);
    const size_t g0 = (size_t)blockIdx.x * kGroupsPerBlock + threadIdx.x;
#pragma unroll 4
    for (int it = 0; it < kIter; ++it) {
        const size_t gi = g0 + (size_t)it * kThreads;
        if (gi >= ngroups) break;
        Px4 v = grp[gi];
        uint32_t c[12] = {v.a & 255, v.a >> 8 & 255, v.a >> 16 & 255, v.a >> 24, v.b & 255, v.b >> 8 & 255, v.b >> 16 & 255, v.b >> 24,
                          v.c & 255, v.c >> 8 & 255, v.c >> 16 & 255, v.c >> 24};
#pragma unroll
        for (int p = 0; p < 4; ++p) convert<kGrey>(c[3 * p], c[3 * p + 1], c[3 * p + 2], m, s_lin, s_lut, s_coarse, s_last);
        v.a = c[0] | c[1] << 8 | c[2] << 16 | c[3] << 24;
        v.b = c[4] | c[5] << 8 | c[6] << 16 | c[7] << 24;
        v.c = c[8] | c[9] << 8 | c[10] << 16 | c[11] << 24;
        grp[gi] = v;
    }
}

// grid (ceil(groups of 4 pixels / kGroupsPerBlock), n).  Image i: npx pixels at rgb + i * pitch, converted in place by blob's record i;
// the workgroups of an image that needs nothing return at once.  Nothing but the image's npx * 3 bytes is written.
__global__ __launch_bounds__(kThreads) void icc_to_srgb_kernel(uint8_t* __restrict__ rgb, size_t pitch, size_t npx, const uint8_t* __restrict__ blob,
                                                                const uint8_t* __restrict__ enc) {
    __shared__ uint32_t lds[384 + 1024 + 128];
    const IccRecord rec = reinterpret_cast<const IccRecord*>(blob)[blockIdx.y];
    uint8_t* base = rgb + pitch * (size_t)blockIdx.y;
    if (rec.kind == icc::kMatrix) run_image<false>(base, npx, blob + rec.off, enc, lds);
    else if (rec.kind == icc::kGrey) run_image<true>(base, npx, blob + rec.off, enc, lds);
}

}  // namespace

IccConverter::~IccConverter() {
    for (Scratch* S : {&own_, &batch_})
        for (hipEvent_t ev : S->up_ev) if (ev) (void)hipEventDestroy(ev);
}

void IccConverter::setup(int max_batch) {
    max_batch_ = max_batch;
    const icc::EncTables& E = icc::enc_tables();
    if (!E.verified) fail(IRE_ERR_INTERNAL, "internal: the sRGB encode tables do not reproduce the exact table");
    uint8_t host[kIccEncBytes];
    std::memcpy(host, E.coarse, 4096);
    std::memcpy(host + 4096, E.last, 512);
    d_enc_ = Buf<DeviceMem>(kIccEncBytes, BufUse::Persistent);
    IRE_HIP(hipMemcpy(d_enc_.get<void>(), host, kIccEncBytes, hipMemcpyHostToDevice));
}

void IccConverter::to_srgb_device(bool batch, uint8_t* d_rgb, int n, int h, int w, size_t image_pitch, const icc::Transform* const* t, hipStream_t s) {
    if (!d_rgb || !t) fail(IRE_ERR_INVALID_INPUT, "invalid arguments to icc_to_srgb: null buffer");
    if (n < 1 || n > max_batch_) fail(IRE_ERR_INVALID_INPUT, "invalid batch size for icc_to_srgb: expected 1..max_batch");
    if (h < 1 || w < 1 || h > 8192 || w > 8192) fail(IRE_ERR_INVALID_INPUT, "invalid image size: height and width must be in 1..8192");
    const size_t npx = (size_t)h * w;
    if (image_pitch < npx * 3) fail(IRE_ERR_INVALID_INPUT, "invalid image pitch for icc_to_srgb: smaller than an image");
    bool any = false;
    for (int i = 0; i < n; ++i) {
        if (!t[i]) continue;
        if (t[i]->kind < icc::kNone || t[i]->kind > icc::kGrey) fail(IRE_ERR_INVALID_INPUT, "invalid ire_icc_transform: unknown kind");
        any = any || t[i]->kind == icc::kMatrix || t[i]->kind == icc::kGrey;
    }
    if (!any) return;
    Scratch& S = batch ? batch_ : own_;
    const size_t cap = (size_t)max_batch_ * (sizeof(IccRecord) + sizeof(IccMatrixTable));
    const int turn = S.turn;
    S.turn ^= 1;
    if (S.up_recorded[turn]) IRE_HIP(hipEventSynchronize(S.up_ev[turn]));
    if (!S.up_ev[turn]) IRE_HIP(hipEventCreateWithFlags(&S.up_ev[turn], hipEventDisableTiming));
    S.pin[turn].grow(cap);
    S.d_blob.grow(cap);               // (allocated once: cap depends on max_batch alone)
    uint8_t* pin = S.pin[turn].get<uint8_t>();
    IccRecord* rec = reinterpret_cast<IccRecord*>(pin);
    size_t off = sizeof(IccRecord) * (size_t)n;
    for (int i = 0; i < n; ++i) {
        const int kind = t[i] ? t[i]->kind : icc::kNone;
        rec[i] = IccRecord{kind, (uint32_t)off};
        if (kind == icc::kMatrix) {
            IccMatrixTable tab{};
            std::memcpy(tab.m, t[i]->m, sizeof(tab.m));
            std::memcpy(tab.lin, t[i]->lin, sizeof(tab.lin));
            std::memcpy(pin + off, &tab, sizeof(tab));
            off += sizeof(tab);
        } else if (kind == icc::kGrey) {
            icc::grey_lut(*t[i], pin + off);
            off += 256;
        }
    }
    IRE_HIP(hipMemcpyAsync(S.d_blob.get<void>(), pin, off, hipMemcpyHostToDevice, s));
    IRE_HIP(hipEventRecord(S.up_ev[turn], s));
    S.up_recorded[turn] = true;
    const size_t groups = (npx + 3) / 4;
    const dim3 grid((unsigned)((groups + kGroupsPerBlock - 1) / kGroupsPerBlock), (unsigned)n);
    hipLaunchKernelGGL(icc_to_srgb_kernel, grid, dim3(kThreads), 0, s, d_rgb, image_pitch, npx, S.d_blob.get<const uint8_t>(), d_enc_.get<const uint8_t>());
    IRE_HIP(hipGetLastError());
}

void IccConverter::to_srgb_host(uint8_t* rgb, int n, int h, int w, const icc::Transform* const* t, hipStream_t s) {
    if (!rgb || !t) fail(IRE_ERR_INVALID_INPUT, "invalid arguments to icc_to_srgb: null buffer");
    if (n < 1 || n > max_batch_) fail(IRE_ERR_INVALID_INPUT, "invalid batch size for icc_to_srgb: expected 1..max_batch");
    if (h < 1 || w < 1 || h > 8192 || w > 8192) fail(IRE_ERR_INVALID_INPUT, "invalid image size: height and width must be in 1..8192");
    const size_t bytes = (size_t)h * w * 3 * (size_t)n;
    d_host_.grow(bytes);
    IRE_HIP(hipMemcpyAsync(d_host_.get<void>(), rgb, bytes, hipMemcpyHostToDevice, s));
    to_srgb_device(false, d_host_.get<uint8_t>(), n, h, w, (size_t)h * w * 3, t, s);
    IRE_HIP(hipMemcpyAsync(rgb, d_host_.get<void>(), bytes, hipMemcpyDeviceToHost, s));
    IRE_HIP(hipStreamSynchronize(s));
}

}  // namespace ire
