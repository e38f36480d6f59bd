// Preprocess step in front of the hot path: the pixel work of
// server-node/src/middleware/imagePreprocess.js:24-91 -- EXIF auto-orient (:43) and fit-inside-2048 Lanczos-3 (:46-55).
// The JPEG q85 4:4:4 encode (:57-64) stays with the host codec (sharp in the Node deployment, Pillow behind FastAPI).
//
// Arithmetic: the published 8-bit resampler of Pillow (two passes, horizontal then vertical; taps normalised and
// rounded to 22-bit integers; one rounding to u8 per pass) -- integer multiply-adds, so the GPU result is bit-exact
// against oracle/preprocess.py, which tests/test_preprocess.py pins bit-exactly against Pillow itself.  libvips' own
// reducer (the reference's dependency) is not in this image: parity with it is unpinned.
//
// Both kernels are HBM-bound byte work (read each stored pixel once, write the intermediate once, read it once, write
// the result): a thread produces one output pixel (3 bytes) from <= ksize taps; the orientation is folded into the
// horizontal pass's reads, so there is no separate transpose pass.  That is the single-image entry (preprocess_device), kept as it was.
//
// The batched entry (preprocess_batch_device, upload jobs) computes the same bytes from tiles staged in LDS -- stored pixels are read along
// stored rows for every orientation -- with the image index as a grid dimension and the tap tables cached on the device: further down.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "engine.hpp"

namespace ire {

namespace {

constexpr int kPrecisionBits = 32 - 8 - 2;

double lanczos3(double x) {
    if (x >= -3.0 && x < 3.0) {
        if (x == 0.0) return 1.0;
        const double px = x * M_PI;
        const double a = std::sin(px) / px;
        const double py = px / 3.0;
        return a * (std::sin(py) / py);
    }
    return 0.0;
}

// bounds[out][2] = (first, count), taps[out][ksize]
int make_taps(int in_size, int out_size, std::vector<int32_t>& bounds, std::vector<int32_t>& taps) {
    const double scale = (double)in_size / out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 3.0 * filterscale;
    const int ksize = (int)std::ceil(support) * 2 + 1;
    bounds.assign((size_t)out_size * 2, 0);
    taps.assign((size_t)out_size * ksize, 0);
    const double ss = 1.0 / filterscale;
    std::vector<double> w(ksize);
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = (xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > in_size) xmax = in_size;
        xmax -= xmin;
        double ww = 0.0;
        for (int x = 0; x < xmax; ++x) { w[x] = lanczos3((x + xmin - center + 0.5) * ss); ww += w[x]; }
        for (int x = 0; x < xmax; ++x) {
            const double k = ww != 0.0 ? w[x] / ww : w[x];
            taps[(size_t)xx * ksize + x] = k < 0 ? (int32_t)(k * (1 << kPrecisionBits) - 0.5) : (int32_t)(k * (1 << kPrecisionBits) + 0.5);
        }
        bounds[(size_t)xx * 2] = xmin;
        bounds[(size_t)xx * 2 + 1] = xmax;
    }
    return ksize;
}

__device__ __forceinline__ int clip8(int v) { v >>= kPrecisionBits; return v < 0 ? 0 : (v > 255 ? 255 : v); }

// upright (y, x) -> stored pixel index, EXIF orientation 1..8; sh, sw = stored height, width
__device__ __forceinline__ size_t stored_index(int orientation, int y, int x, int sh, int sw) {
    int sy, sx;
    switch (orientation) {
        case 2: sy = y; sx = sw - 1 - x; break;
        case 3: sy = sh - 1 - y; sx = sw - 1 - x; break;
        case 4: sy = sh - 1 - y; sx = x; break;
        case 5: sy = x; sx = y; break;
        case 6: sy = sh - 1 - x; sx = y; break;
        case 7: sy = sh - 1 - x; sx = sw - 1 - y; break;
        case 8: sy = x; sx = sw - 1 - y; break;
        default: sy = y; sx = x; break;
    }
    return (size_t)sy * sw + sx;
}

// horizontal pass over the UPRIGHT image (uh x uw) read through the orientation map; out: uh x ow
__global__ __launch_bounds__(256) void resample_h_kernel(const uint8_t* __restrict__ src, int sh, int sw, int orientation, int uh,
                                                         int ow, int ksize, const int32_t* __restrict__ bounds,
                                                         const int32_t* __restrict__ taps, uint8_t* __restrict__ dst) {
    const int xx = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (xx >= ow || y >= uh) return;
    const int x0 = bounds[2 * xx], n = bounds[2 * xx + 1];
    const int32_t* k = taps + (size_t)xx * ksize;
    int r = 1 << (kPrecisionBits - 1), g = r, b = r;
    for (int t = 0; t < n; ++t) {
        const uint8_t* p = src + stored_index(orientation, y, x0 + t, sh, sw) * 3;
        const int kv = k[t];
        r += p[0] * kv; g += p[1] * kv; b += p[2] * kv;
    }
    uint8_t* o = dst + ((size_t)y * ow + xx) * 3;
    o[0] = (uint8_t)clip8(r); o[1] = (uint8_t)clip8(g); o[2] = (uint8_t)clip8(b);
}

// vertical pass: in uh x ow -> out oh x ow; threads run along x (coalesced rows)
__global__ __launch_bounds__(256) void resample_v_kernel(const uint8_t* __restrict__ src, int ow, int oh, int ksize,
                                                         const int32_t* __restrict__ bounds, const int32_t* __restrict__ taps,
                                                         uint8_t* __restrict__ dst) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, yy = blockIdx.y;      // i = byte column in [0, ow*3)
    if (i >= ow * 3 || yy >= oh) return;
    const int y0 = bounds[2 * yy], n = bounds[2 * yy + 1];
    const int32_t* k = taps + (size_t)yy * ksize;
    int acc = 1 << (kPrecisionBits - 1);
    for (int t = 0; t < n; ++t) acc += src[(size_t)(y0 + t) * ow * 3 + i] * k[t];
    dst[(size_t)yy * ow * 3 + i] = (uint8_t)clip8(acc);
}

// orientation only (no size change): one byte-triplet copy per upright pixel
__global__ __launch_bounds__(256) void orient_kernel(const uint8_t* __restrict__ src, int sh, int sw, int orientation, int uh, int uw,
                                                     uint8_t* __restrict__ dst) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= uw || y >= uh) return;
    const uint8_t* p = src + stored_index(orientation, y, x, sh, sw) * 3;
    uint8_t* o = dst + ((size_t)y * uw + x) * 3;
    o[0] = p[0]; o[1] = p[1]; o[2] = p[2];
}

// ---- the batched form (Engine::preprocess_batch_device): blockIdx.z = the image -------------------------------------------------------
// Both tiled kernels work on a tile of the UPRIGHT image, kTY rows high, staged in LDS as lds[x][y][3] with a row pitch of kP bytes
// (25 words, odd: the rows of consecutive x fall on different banks).  The loader is the only code that knows the orientation: it
// always walks the STORED image along its rows -- orientations 1..4 (upright x = stored column) in runs of the tile's width,
// orientations 5..8 (upright x = stored row) in runs of kTY pixels -- and writes LDS transposed where the upright image is.
// flip_a: the stored coordinate that upright x becomes runs backwards; flip_b: the one upright y becomes.
constexpr int kTX = 32, kTY = 32, kP = kTY * 3 + 4;
constexpr size_t kTileLdsMax = 64 * 1024;      // the tiled horizontal pass's LDS per workgroup at most (the scale switch)

template <bool SWAP>
__device__ __forceinline__ void load_tile(uint8_t* lds, const uint8_t* __restrict__ img, int sh, int sw, int flip_a, int flip_b, int xb, int nx, int y0, int uh) {
    const int tid = threadIdx.x;
    if (SWAP) {
        const int ny = min(kTY, uh - y0);
        for (int i = tid; i < nx * (kTY * 3); i += 256) {
            const int xr = i / (kTY * 3), j = i - xr * (kTY * 3), ty = j / 3, c = j - ty * 3;
            if (ty >= ny) continue;
            const int r = flip_a ? sh - 1 - (xb + xr) : xb + xr, col = flip_b ? sw - 1 - (y0 + ty) : y0 + ty;
            lds[xr * kP + j] = img[((size_t)r * sw + col) * 3 + c];
        }
    } else {
        const int wave = tid >> 6, lane = tid & 63;
        for (int ty = wave; ty < kTY && y0 + ty < uh; ty += 4) {
            const int r = flip_b ? sh - 1 - (y0 + ty) : y0 + ty;
            const uint8_t* row = img + (size_t)r * sw * 3;
            for (int j = lane; j < nx * 3; j += 64) {
                const int xr = j / 3, c = j - xr * 3;
                const int col = flip_a ? sw - 1 - (xb + xr) : xb + xr;
                lds[xr * kP + ty * 3 + c] = row[col * 3 + c];
            }
        }
    }
}

// horizontal pass, tiled: a workgroup makes kTY rows x kTX columns of the intermediate.  A thread makes one output column of four
// consecutive rows: their 12 bytes lie side by side in a row of the tile (three word reads per tap, one tap load for all four pixels).
// The results go back through LDS, where the tile was, and leave as whole words along the intermediate's rows (its row pitch mp is a
// multiple of 4; a row's last word may reach into that padding).  span: the LDS rows the launch reserved.
template <bool SWAP>
__global__ __launch_bounds__(256) void resample_h_tiled_kernel(const uint8_t* __restrict__ src, size_t image_pitch, int sh, int sw, int flip_a, int flip_b, int uh,
                                                               int ow, int ksize, const int32_t* __restrict__ bounds, const int32_t* __restrict__ taps,
                                                               uint8_t* __restrict__ mid, int mp, int span) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int xx0 = blockIdx.x * kTX, y0 = blockIdx.y * kTY, xl = min(xx0 + kTX, ow) - 1;
    const int xb = bounds[2 * xx0], nx = min(bounds[2 * xl] + bounds[2 * xl + 1] - xb, span);      // (first and count grow with the output index)
    load_tile<SWAP>(lds, src + blockIdx.z * image_pitch, sh, sw, flip_a, flip_b, xb, nx, y0, uh);
    __syncthreads();
    const int xi = threadIdx.x & 31, xx = xx0 + xi, g = threadIdx.x >> 5;      // rows y0 + 4 g .. + 3 (rows past the image hold whatever LDS held: computed, never stored)
    int acc[12];
    for (int q = 0; q < 12; ++q) acc[q] = 1 << (kPrecisionBits - 1);
    if (xx < ow) {
        const int n = bounds[2 * xx + 1];
        const uint32_t* v = reinterpret_cast<const uint32_t*>(lds + (bounds[2 * xx] - xb) * kP + 12 * g);
        const int32_t* k = taps + (size_t)xx * ksize;
        for (int t = 0; t < n; ++t, v += kP / 4) {
            const int kv = k[t];
            for (int q = 0; q < 3; ++q) {
                const uint32_t w = v[q];
                acc[4 * q] += (int)(w & 255u) * kv; acc[4 * q + 1] += (int)(w >> 8 & 255u) * kv; acc[4 * q + 2] += (int)(w >> 16 & 255u) * kv; acc[4 * q + 3] += (int)(w >> 24) * kv;
            }
        }
    }
    __syncthreads();      // every thread is done with the tile: its place takes the results, as kTY rows of kTX pixels
    if (xx < ow)
        for (int q = 0; q < 12; ++q) lds[(4 * g + q / 3) * (kTX * 3) + xi * 3 + q % 3] = (uint8_t)clip8(acc[q]);
    __syncthreads();
    const int nb = (xl + 1 - xx0) * 3, ny = min(kTY, uh - y0);
    for (int i = threadIdx.x; i < ny * (kTX * 3 / 4); i += 256) {
        const int ty = i / (kTX * 3 / 4), j = (i - ty * (kTX * 3 / 4)) * 4;
        if (j < nb) *reinterpret_cast<uint32_t*>(mid + ((size_t)blockIdx.z * uh + y0 + ty) * mp + (size_t)xx0 * 3 + j) = *reinterpret_cast<const uint32_t*>(lds + ty * (kTX * 3) + j);
    }
}

// horizontal pass for scales whose tile does not fit in LDS: resample_h_kernel per image (a thread gathers its own taps)
__global__ __launch_bounds__(256) void resample_h_strip_kernel(const uint8_t* __restrict__ src, size_t image_pitch, int sh, int sw, int orientation, int uh, int ow,
                                                               int ksize, const int32_t* __restrict__ bounds, const int32_t* __restrict__ taps,
                                                               uint8_t* __restrict__ mid, int mp) {
    const int xx = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (xx >= ow || y >= uh) return;
    const uint8_t* img = src + blockIdx.z * image_pitch;
    const int x0 = bounds[2 * xx], n = bounds[2 * xx + 1];
    const int32_t* k = taps + (size_t)xx * ksize;
    int r = 1 << (kPrecisionBits - 1), g = r, b = r;
    for (int t = 0; t < n; ++t) {
        const uint8_t* p = img + stored_index(orientation, y, x0 + t, sh, sw) * 3;
        const int kv = k[t];
        r += p[0] * kv; g += p[1] * kv; b += p[2] * kv;
    }
    uint8_t* o = mid + ((size_t)blockIdx.z * uh + y) * mp + (size_t)xx * 3;
    o[0] = (uint8_t)clip8(r); o[1] = (uint8_t)clip8(g); o[2] = (uint8_t)clip8(b);
}

// vertical pass: a thread makes four consecutive bytes of an output row from one word per tap (the taps are the row's: uniform loads);
// words: the output rows are word-aligned (3 * ow, the image pitch and the base are multiples of 4), so the four bytes leave as one word
__global__ __launch_bounds__(256) void resample_v_batch_kernel(const uint8_t* __restrict__ mid, int uh, int mp, int ow3, int ksize,
                                                               const int32_t* __restrict__ bounds, const int32_t* __restrict__ taps, uint8_t* __restrict__ dst,
                                                               size_t out_pitch, int words) {
    const int i = (blockIdx.x * blockDim.x + threadIdx.x) * 4, yy = blockIdx.y;
    if (i >= ow3) return;
    const int y0 = bounds[2 * yy], n = bounds[2 * yy + 1];
    const int32_t* k = taps + (size_t)yy * ksize;
    const uint8_t* col = mid + ((size_t)blockIdx.z * uh + y0) * mp + i;
    int a0 = 1 << (kPrecisionBits - 1), a1 = a0, a2 = a0, a3 = a0;
    for (int t = 0; t < n; ++t, col += mp) {
        const uint32_t v = *reinterpret_cast<const uint32_t*>(col);
        const int kv = k[t];
        a0 += (int)(v & 255u) * kv; a1 += (int)(v >> 8 & 255u) * kv; a2 += (int)(v >> 16 & 255u) * kv; a3 += (int)(v >> 24) * kv;
    }
    uint8_t* o = dst + blockIdx.z * out_pitch + (size_t)yy * ow3 + i;
    const uint32_t b0 = (uint32_t)clip8(a0), b1 = (uint32_t)clip8(a1), b2 = (uint32_t)clip8(a2), b3 = (uint32_t)clip8(a3);
    if (words) *reinterpret_cast<uint32_t*>(o) = b0 | b1 << 8 | b2 << 16 | b3 << 24;
    else {
        o[0] = (uint8_t)b0;
        if (i + 1 < ow3) o[1] = (uint8_t)b1;
        if (i + 2 < ow3) o[2] = (uint8_t)b2;
        if (i + 3 < ow3) o[3] = (uint8_t)b3;
    }
}

// orientation only: a kTY x kTX tile of the upright image through LDS -- stored rows in, upright rows out, whole words where `words`
template <bool SWAP>
__global__ __launch_bounds__(256) void orient_tiled_kernel(const uint8_t* __restrict__ src, size_t image_pitch, int sh, int sw, int flip_a, int flip_b, int uh, int uw,
                                                           uint8_t* __restrict__ dst, size_t out_pitch, int words) {
    __shared__ uint8_t lds[kTX * kP];
    const int x0 = blockIdx.x * kTX, y0 = blockIdx.y * kTY, nx = min(kTX, uw - x0), ny = min(kTY, uh - y0);
    load_tile<SWAP>(lds, src + blockIdx.z * image_pitch, sh, sw, flip_a, flip_b, x0, nx, y0, uh);
    __syncthreads();
    uint8_t* out = dst + blockIdx.z * out_pitch + ((size_t)y0 * uw + x0) * 3;
    if (words) {          // 3 * uw is a multiple of 4, so is 3 * x0 = 96 * blockIdx.x, so is 3 * nx
        for (int i = threadIdx.x; i < ny * (kTX * 3 / 4); i += 256) {
            const int ty = i / (kTX * 3 / 4), j = (i - ty * (kTX * 3 / 4)) * 4;
            if (j >= nx * 3) continue;
            uint32_t v = 0;
            for (int q = 0; q < 4; ++q) v |= (uint32_t)lds[(j + q) / 3 * kP + ty * 3 + (j + q) % 3] << (8 * q);
            *reinterpret_cast<uint32_t*>(out + (size_t)ty * uw * 3 + j) = v;
        }
    } else {
        for (int i = threadIdx.x; i < ny * (kTX * 3); i += 256) {
            const int ty = i / (kTX * 3), j = i - ty * (kTX * 3);
            if (j < nx * 3) out[(size_t)ty * uw * 3 + j] = lds[j / 3 * kP + ty * 3 + j % 3];
        }
    }
}

long js_round(double x) { return (long)std::floor(x + 0.5); }

}  // namespace

// imagePreprocess.js:12-22,46-55 -- the box comes from the STORED dimensions (sharp's metadata() ignores EXIF), the upright
// image is then fitted inside it without enlargement.
void preprocess_plan(int width, int height, int orientation, int max_dim, int* out_w, int* out_h, int* resized) {
    if (width <= 0 || height <= 0 || orientation < 1 || orientation > 8 || max_dim < 1)
        fail(IRE_ERR_INVALID_INPUT, "invalid arguments to preprocess: width, height > 0, orientation in 1..8, max_dim >= 1");
    const bool swap = orientation >= 5;
    const int uw = swap ? height : width, uh = swap ? width : height;
    if (width <= max_dim && height <= max_dim) { *out_w = uw; *out_h = uh; if (resized) *resized = 0; return; }
    const double scale = (double)max_dim / (width > height ? width : height);
    const double bw = (double)js_round(width * scale), bh = (double)js_round(height * scale);
    double s2 = bw / uw;
    if (bh / uh < s2) s2 = bh / uh;
    if (s2 > 1.0) s2 = 1.0;
    long ow = js_round(uw * s2), oh = js_round(uh * s2);
    *out_w = ow < 1 ? 1 : (int)ow;
    *out_h = oh < 1 ? 1 : (int)oh;
    if (resized) *resized = 1;
}

void Engine::preprocess_device(const uint8_t* d_rgb, int h, int w, int orientation, int max_dim, uint8_t* d_out, int out_h, int out_w,
                               hipStream_t s) {
    int pw = 0, ph = 0, resized = 0;
    preprocess_plan(w, h, orientation, max_dim, &pw, &ph, &resized);
    if (pw != out_w || ph != out_h) fail(IRE_ERR_INVALID_INPUT, "invalid output size for preprocess: use ire_preprocess_plan");
    if (!d_rgb || !d_out) fail(IRE_ERR_INVALID_INPUT, "invalid arguments to preprocess: null buffer");
    const bool swap = orientation >= 5;
    const int uw = swap ? h : w, uh = swap ? w : h;
    if (!resized) {
        if (orientation == 1) { IRE_HIP(hipMemcpyAsync(d_out, d_rgb, (size_t)h * w * 3, hipMemcpyDeviceToDevice, s)); return; }
        hipLaunchKernelGGL(orient_kernel, dim3((uw + 255) / 256, uh), dim3(256), 0, s, d_rgb, h, w, orientation, uh, uw, d_out);
        IRE_HIP(hipGetLastError());
        return;
    }
    // taps are rebuilt per call (two small tables, <= a few hundred KiB): the step runs once per upload
    std::vector<int32_t> bh_, th_, bv_, tv_;
    const int kh = make_taps(uw, out_w, bh_, th_);
    const int kv = make_taps(uh, out_h, bv_, tv_);
    const size_t need_tab = (bh_.size() + th_.size() + bv_.size() + tv_.size()) * sizeof(int32_t);
    const size_t need_mid = (size_t)uh * out_w * 3;
    d_pp_tab_.grow(need_tab);
    d_pp_mid_.grow(need_mid);
    int32_t* d_bh = d_pp_tab_.get<int32_t>();
    int32_t* d_th = d_bh + bh_.size();
    int32_t* d_bv = d_th + th_.size();
    int32_t* d_tv = d_bv + bv_.size();
    // the tables live in pageable host vectors: copy synchronously with respect to the host (hipMemcpyAsync from
    // pageable memory returns after staging), ordered on `s` before the kernels
    IRE_HIP(hipMemcpyAsync(d_bh, bh_.data(), bh_.size() * 4, hipMemcpyHostToDevice, s));
    IRE_HIP(hipMemcpyAsync(d_th, th_.data(), th_.size() * 4, hipMemcpyHostToDevice, s));
    IRE_HIP(hipMemcpyAsync(d_bv, bv_.data(), bv_.size() * 4, hipMemcpyHostToDevice, s));
    IRE_HIP(hipMemcpyAsync(d_tv, tv_.data(), tv_.size() * 4, hipMemcpyHostToDevice, s));
    IRE_HIP(hipStreamSynchronize(s));      // the vectors die at return
    hipLaunchKernelGGL(resample_h_kernel, dim3((out_w + 255) / 256, uh), dim3(256), 0, s, d_rgb, h, w, orientation, uh, out_w, kh, d_bh,
                       d_th, d_pp_mid_.get<uint8_t>());
    hipLaunchKernelGGL(resample_v_kernel, dim3((out_w * 3 + 255) / 256, out_h), dim3(256), 0, s, d_pp_mid_.get<uint8_t>(), out_w, out_h, kv, d_bv, d_tv,
                       d_out);
    IRE_HIP(hipGetLastError());
}

// The taps are built here, in double precision, by the same make_taps (the device's sin would not round the same).  A miss may
// replace the pair used longest ago: kernels of earlier calls may still read that table, so the device is idle before it is freed.
const TapTable& PreprocessScratch::table(int in_size, int out_size, hipStream_t s) {
    TapTable* lru = &tab[0];
    for (TapTable& t : tab) {
        if (t.used && t.in == in_size && t.out == out_size) { t.used = ++clock; return t; }
        if (t.used < lru->used) lru = &t;
    }
    std::vector<int32_t> bounds, taps;
    const int ksize = make_taps(in_size, out_size, bounds, taps);
    int span = 1;
    for (int x0 = 0; x0 < out_size; x0 += kTX) {
        int lo = in_size, hi = 0;
        for (int x = x0; x < out_size && x < x0 + kTX; ++x) { lo = std::min(lo, bounds[2 * x]); hi = std::max(hi, bounds[2 * x] + bounds[2 * x + 1]); }
        span = std::max(span, hi - lo);
    }
    if (lru->used) { IRE_HIP(hipDeviceSynchronize()); lru->used = 0; lru->d.reset(); }
    lru->d = Buf<DeviceMem>((bounds.size() + taps.size()) * sizeof(int32_t), BufUse::Persistent);      // cached: later calls of the pair read it
    IRE_HIP(hipMemcpyAsync(lru->d.get<int32_t>(), bounds.data(), bounds.size() * 4, hipMemcpyHostToDevice, s));
    IRE_HIP(hipMemcpyAsync(lru->d.get<int32_t>() + bounds.size(), taps.data(), taps.size() * 4, hipMemcpyHostToDevice, s));
    IRE_HIP(hipStreamSynchronize(s));      // the vectors die at return: the one wait of a pair's first use
    lru->in = in_size; lru->out = out_size; lru->ksize = ksize; lru->span = span; lru->used = ++clock;
    return *lru;
}

void Engine::preprocess_batch_device(PreprocessScratch& P, const uint8_t* d_rgb, int n, int h, int w, size_t image_pitch, int orientation, int max_dim,
                                     uint8_t* d_out, int out_h, int out_w, size_t out_pitch, hipStream_t s) {
    int pw = 0, ph = 0, resized = 0;
    preprocess_plan(w, h, orientation, max_dim, &pw, &ph, &resized);
    if (pw != out_w || ph != out_h) fail(IRE_ERR_INVALID_INPUT, "invalid output size for preprocess: use ire_preprocess_plan");
    if (!d_rgb || !d_out) fail(IRE_ERR_INVALID_INPUT, "invalid arguments to preprocess: null buffer");
    if (n < 1 || n > max_batch_) fail(IRE_ERR_INVALID_INPUT, "invalid batch size for preprocess: expected 1..max_batch");
    if (h > 8192 || w > 8192) fail(IRE_ERR_INVALID_INPUT, "invalid image size: height and width must be in 1..8192");
    const size_t in_bytes = (size_t)h * w * 3, out_bytes = (size_t)out_h * out_w * 3;
    if (image_pitch < in_bytes || out_pitch < out_bytes) fail(IRE_ERR_INVALID_INPUT, "invalid image pitch for preprocess: smaller than an image");
    const bool swap = orientation >= 5;
    const int uw = swap ? h : w, uh = swap ? w : h;
    const int flip_a = swap ? (orientation == 6 || orientation == 7) : (orientation == 2 || orientation == 3);
    const int flip_b = swap ? (orientation == 7 || orientation == 8) : (orientation == 3 || orientation == 4);
    const bool aligned = out_pitch % 4 == 0 && (uintptr_t)d_out % 4 == 0 && (size_t)out_w * 3 % 4 == 0;
    if (!resized) {
        if (orientation == 1) { IRE_HIP(hipMemcpy2DAsync(d_out, out_pitch, d_rgb, image_pitch, in_bytes, (size_t)n, hipMemcpyDeviceToDevice, s)); return; }
        const dim3 grid((uw + kTX - 1) / kTX, (uh + kTY - 1) / kTY, n);
        if (swap) hipLaunchKernelGGL(orient_tiled_kernel<true>, grid, dim3(256), 0, s, d_rgb, image_pitch, h, w, flip_a, flip_b, uh, uw, d_out, out_pitch, (int)aligned);
        else hipLaunchKernelGGL(orient_tiled_kernel<false>, grid, dim3(256), 0, s, d_rgb, image_pitch, h, w, flip_a, flip_b, uh, uw, d_out, out_pitch, (int)aligned);
        IRE_HIP(hipGetLastError());
        return;
    }
    const TapTable& H = P.table(uw, out_w, s);
    const TapTable& V = P.table(uh, out_h, s);      // (H was stamped just now: a miss here replaces another pair)
    const int mp = (out_w * 3 + 3) & ~3;
    const size_t per = (size_t)uh * mp;
    P.d_mid.grow(per * n, batch_room(per * n, per * max_batch_));
    uint8_t* mid = P.d_mid.get<uint8_t>();
    const size_t tile = (size_t)H.span * kP, lds = std::max(tile, (size_t)kTY * kTX * 3);      // the tile; the results pass through the same place
    if (tile <= kTileLdsMax) {
        const dim3 grid((out_w + kTX - 1) / kTX, (uh + kTY - 1) / kTY, n);
        if (swap) hipLaunchKernelGGL(resample_h_tiled_kernel<true>, grid, dim3(256), lds, s, d_rgb, image_pitch, h, w, flip_a, flip_b, uh, out_w, H.ksize, H.bounds(), H.taps(), mid, mp, H.span);
        else hipLaunchKernelGGL(resample_h_tiled_kernel<false>, grid, dim3(256), lds, s, d_rgb, image_pitch, h, w, flip_a, flip_b, uh, out_w, H.ksize, H.bounds(), H.taps(), mid, mp, H.span);
    } else
        hipLaunchKernelGGL(resample_h_strip_kernel, dim3((out_w + 255) / 256, uh, n), dim3(256), 0, s, d_rgb, image_pitch, h, w, orientation, uh, out_w, H.ksize, H.bounds(), H.taps(), mid, mp);
    hipLaunchKernelGGL(resample_v_batch_kernel, dim3((mp / 4 + 255) / 256, out_h, n), dim3(256), 0, s, mid, uh, mp, out_w * 3, V.ksize, V.bounds(), V.taps(), d_out, out_pitch,
                       (int)aligned);
    IRE_HIP(hipGetLastError());
}

void Engine::preprocess_host(const uint8_t* rgb, int h, int w, int orientation, int max_dim, uint8_t* out, int out_h, int out_w) {
    int pw = 0, ph = 0;
    preprocess_plan(w, h, orientation, max_dim, &pw, &ph, nullptr);
    if (pw != out_w || ph != out_h) fail(IRE_ERR_INVALID_INPUT, "invalid output size for preprocess: use ire_preprocess_plan");
    if (!rgb || !out) fail(IRE_ERR_INVALID_INPUT, "invalid arguments to preprocess: null buffer");
    const size_t in_bytes = (size_t)h * w * 3, out_bytes = (size_t)out_h * out_w * 3;
    d_pp_in_.grow(in_bytes);
    d_pp_out_.grow(out_bytes);
    uint8_t *const d_in = d_pp_in_.get<uint8_t>(), *const d_res = d_pp_out_.get<uint8_t>();
    hipStream_t s = main_stream_;
    IRE_HIP(hipMemcpyAsync(d_in, rgb, in_bytes, hipMemcpyHostToDevice, s));
    preprocess_device(d_in, h, w, orientation, max_dim, d_res, out_h, out_w, s);
    IRE_HIP(hipMemcpyAsync(out, d_res, out_bytes, hipMemcpyDeviceToHost, s));
    IRE_HIP(hipStreamSynchronize(s));
}

}  // namespace ire
