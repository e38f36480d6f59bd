// png_dec.hip -- PNG uploads decoded on gfx950: two kernels per batch, one wave per image in each.  The arithmetic and the inflate state
// machine are png_inflate_core.hpp's, the text tests/native/png_dec_sim.cpp runs on the CPU; this file adds the barriers between its
// phases, the wavefront of the unfilter and the launch.
//
// K1 png_inflate_kernel: one zlib stream is serial, so the batch is the parallelism.  Lane 0 reads bits from an 8 KiB input window in
//   LDS (all lanes refill it with dword loads) and decodes up to 256 symbols into an LDS queue; then all 64 lanes place the round's
//   bytes, consecutive lanes at consecutive addresses of the filtered-scanline scratch, each byte resolved through the queue (see the
//   core).  There is NO LDS ring of the last 32 KiB: a back-reference that leaves the round reads the scratch itself.  That is safe
//   because the only bytes so read were stored in an EARLIER round by this same workgroup, with a __syncthreads() (a workgroup-scope
//   release / acquire, and the stores' vmcnt wait) between the stores and the loads; one workgroup is one wave on one CU, so store
//   and load pass through the same vector L1, and no other workgroup ever touches this image's scanlines while the kernel runs.
// K2 png_unfilter_kernel: rows as a skewed wavefront, band after band of 64 rows: lane i works on pixel t - i of row 64 b + i at step
//   t and takes `up` and `up left` from lane i - 1 by a cross-lane shift; lane 0 takes them from the last row of the band before,
//   which lane 63 left in LDS.  The store does the colour work: palette lookup, grey replication, alpha drop.
//   Access: each lane reads its own row front to back (1..4 bytes a step, the next step's pixel loaded a step ahead) and writes 3
//   bytes a step; neighbouring lanes are a scanline apart.  Nobody has tuned either kernel: profiles/png_decode.md has the times.
// K2' png_unfilter_any_kernel: takes K2's place for a batch that holds a file of depth 1, 2, 4 or 16 or an Adam7 one (see there);
//   still two launches whatever n.  K1 is the same for every form: only the stream's expected length differs (Record::scan_total).
#include "png_dec.hpp"

namespace ire {
using namespace pngdec;

// ticks: null, or three words per image for lane 0's constant-rate clock: in walk | in place and its barriers | in the whole kernel
// (tools/png_decode_measure.py: which of the two bounds the kernel)
__global__ __launch_bounds__(kLanes) void png_inflate_kernel(const uint8_t* __restrict__ blob, size_t bytes_off, uint8_t* __restrict__ scan, int32_t* __restrict__ status,
                                                             unsigned long long* __restrict__ ticks) {
    __shared__ Inflate S;
    const bool timed = ticks != nullptr && threadIdx.x == 0;
    unsigned long long t_walk = 0, t_place = 0, t0 = 0, t1 = 0;
    const unsigned long long t_begin = timed ? wall_clock64() : 0;
    const Record& R = reinterpret_cast<const Record*>(blob)[blockIdx.x];
    const int lane = (int)threadIdx.x;
    if (lane == 0) begin(S, blob + bytes_off + R.in_off, R.in_len, scan + R.scan_off, R.scan_total);
    __syncthreads();
    for (;;) {
        window_load(S, lane);
        __syncthreads();
        if (lane == 0) { window_commit(S); block_begin(S); }
        __syncthreads();
        const uint32_t done = S.done, kind = S.kind;      // (lane 0 next writes them three barriers on)
        if (done) break;
        if (kind == kKindHuff) fill_fast(S, lane);
        uint32_t end;
        do {
            window_load(S, lane);
            __syncthreads();
            if (timed) t0 = wall_clock64();
            if (lane == 0) { window_commit(S); walk(S); }
            if (timed) { t1 = wall_clock64(); t_walk += t1 - t0; }
            __syncthreads();
            end = S.block_end;
            place(S, lane);
            __syncthreads();
            if (timed) t_place += wall_clock64() - t1;
        } while (!end);
    }
    if (lane == 0) { finish(S); status[R.dst] = S.status; }
    if (timed) { ticks[3 * blockIdx.x] = t_walk; ticks[3 * blockIdx.x + 1] = t_place; ticks[3 * blockIdx.x + 2] = wall_clock64() - t_begin; }
}

__device__ __forceinline__ uint32_t load_px(const uint8_t* p, uint32_t bpp) {
    uint32_t v = 0;
    for (uint32_t k = 0; k < 4; ++k) if (k < bpp) v |= (uint32_t)p[k] << (8 * k);
    return v;
}

// one image of the form "8 bits, not interlaced": the whole workgroup (one wave).  hand: 8192 words of LDS
__device__ __forceinline__ void unfilter_rows8(const Record& R, const uint8_t* __restrict__ scan_all, uint8_t* __restrict__ rgb, uint32_t* hand, int32_t* __restrict__ status) {
    const uint32_t lane = threadIdx.x, h = R.h, w = R.w, bpp = R.bpp, ctype = R.ctype;
    const size_t stride = 1 + (size_t)w * bpp;
    const uint8_t* scan = scan_all + R.scan_off;
    bool bad = false;
    for (uint32_t r0 = 0; r0 < h; r0 += kLanes) {
        const uint32_t r = r0 + lane;
        const bool row = r < h;
        const uint8_t* line = scan + stride * (row ? r : 0);
        uint32_t ft = row ? line[0] : 0;
        if (ft > 4) { bad = true; ft = 0; }
        uint32_t cur = 0, prev = 0;
        uint32_t next = (row && lane == 0) ? load_px(line + 1, bpp) : 0;      // the pixel of the step to come
        for (uint32_t t = 0; t < w + kLanes - 1; ++t) {
            uint32_t up = (uint32_t)__shfl_up((int)cur, 1), upleft = (uint32_t)__shfl_up((int)prev, 1);
            const uint32_t x = t - lane;
            const bool on = row && t >= lane && x < w;
            const uint32_t px = next;
            if (row && t + 1 >= lane && x + 1 < w) next = load_px(line + 1 + (size_t)(x + 1) * bpp, bpp);      // x + 1 in 0 .. w - 1
            if (on) {
                if (lane == 0) { up = hand[x]; upleft = x ? hand[x - 1] : 0; }
                const uint32_t a = x ? cur : 0, b = r ? up : 0, c = (r && x) ? upleft : 0;
                const uint32_t raw = unfilter_px(ft, bpp, px, a, b, c);
                prev = cur; cur = raw;
                const uint32_t v = rgb_of(ctype, raw, R.pal);
                uint8_t* o = rgb + ((size_t)r * w + x) * 3;
                o[0] = (uint8_t)v; o[1] = (uint8_t)(v >> 8); o[2] = (uint8_t)(v >> 16);
                if (lane == kLanes - 1) hand[x] = raw;      // x = t - 63: 63 pixels behind lane 0's reads of this step
            }
        }
        __syncthreads();
    }
    if (bad) status[R.dst] = kStFilter;
}

__global__ __launch_bounds__(kLanes) void png_unfilter_kernel(const uint8_t* __restrict__ blob, const uint8_t* __restrict__ scan_all, uint8_t* __restrict__ rgb_all, size_t image_pitch,
                                                              int32_t* __restrict__ status) {
    __shared__ uint32_t hand[8192];          // the raw pixels of the band's last row, for lane 0 of the next band
    const Record& R = reinterpret_cast<const Record*>(blob)[blockIdx.x];
    if (status[R.dst] != 0) return;      // (the whole workgroup: K1 flagged the stream, its scanlines are not all there)
    unfilter_rows8(R, scan_all, rgb_all + image_pitch * R.dst, hand, status);
}

// ---- every other form: 1, 2, 4 and 16 bits, Adam7 (png_adam7_core.hpp) ------------------------------------------------------------------
__device__ __forceinline__ uint64_t load_unit(const uint8_t* p, uint32_t unit) {
    uint64_t v = 0;
    for (uint32_t k = 0; k < 8; ++k) if (k < unit) v |= (uint64_t)p[k] << (8 * k);
    return v;
}
__device__ __forceinline__ uint64_t shfl_up1(uint64_t v) {
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, 1), hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), 1);
    return (uint64_t)hi << 32 | lo;
}

// One workgroup (one wave) per (image, pass): grid (n, 7) when the batch holds an interlaced file, else (n, 1).  The passes of an image
// share nothing but the output, where each writes its own pixels, so they run side by side; within a pass the scheme is K2's: a skewed
// wavefront over bands of 64 pass rows, lane i on unit t - i of pass row 64 b + i, the band's last row handed on in LDS.  A unit is
// 1..8 bytes in one uint64; the store expands it to its 1..8 pixels and scatters them to (y0 + r dy, x0 + c dx).  A record of the old
// form takes unfilter_rows8 in its workgroup of pass 0, so a mixed batch gives each file the bytes its own form's code gives.
__global__ __launch_bounds__(kLanes) void png_unfilter_any_kernel(const uint8_t* __restrict__ blob, const uint8_t* __restrict__ scan_all, uint8_t* __restrict__ rgb_all,
                                                                  size_t image_pitch, int32_t* __restrict__ status) {
    __shared__ uint64_t hand[8192];          // at most 8192 units a pass row: pw <= 8192, and a sub-8-bit row has <= 4096 bytes
    const Record& R = reinterpret_cast<const Record*>(blob)[blockIdx.x];
    if (status[R.dst] != 0) return;      // (K1's word, or kStFilter from another pass of this image: either way the image is flagged)
    uint8_t* rgb = rgb_all + image_pitch * R.dst;
    const uint32_t p = blockIdx.y;
    if (R.depth == 8 && R.interlace == 0) {
        if (p == 0) unfilter_rows8(R, scan_all, rgb, reinterpret_cast<uint32_t*>(hand), status);
        return;
    }
    if (p >= pass_count(R.interlace)) return;
    const Pass P = pass_of(R.h, R.w, R.ctype, R.depth, R.interlace, p);
    if (P.pw == 0 || P.ph == 0) return;      // (uniform: no barrier is left waiting)
    const uint32_t lane = threadIdx.x, w = R.w, ctype = R.ctype, depth = R.depth;
    const uint32_t unit = filter_unit(ctype, depth), per = unit_pixels(ctype, depth), nu = P.row_bytes / unit;      // row_bytes = nu * unit: whole pixels from 8 bits on
    const size_t stride = 1 + (size_t)P.row_bytes;
    const uint8_t* scan = scan_all + R.scan_off + P.off;
    bool bad = false;
    for (uint32_t r0 = 0; r0 < P.ph; r0 += kLanes) {
        const uint32_t r = r0 + lane;
        const bool row = r < P.ph;
        const uint8_t* line = scan + stride * (row ? r : 0);
        uint32_t ft = row ? line[0] : 0;
        if (ft > 4) { bad = true; ft = 0; }
        uint64_t cur = 0, prev = 0;
        uint64_t next = (row && lane == 0) ? load_unit(line + 1, unit) : 0;
        uint8_t* orow = rgb + ((size_t)(P.y0 + (row ? r : 0) * P.dy) * w + P.x0) * 3;      // y0 + r dy < h where r < ph
        for (uint32_t t = 0; t < nu + kLanes - 1; ++t) {
            uint64_t up = shfl_up1(cur), upleft = shfl_up1(prev);
            const uint32_t x = t - lane;
            const bool on = row && t >= lane && x < nu;
            const uint64_t px = next;
            if (row && t + 1 >= lane && x + 1 < nu) next = load_unit(line + 1 + (size_t)(x + 1) * unit, unit);      // x + 1 in 0 .. nu - 1
            if (on) {
                if (lane == 0) { up = hand[x]; upleft = x ? hand[x - 1] : 0; }
                const uint64_t a = x ? cur : 0, b = r ? up : 0, c = (r && x) ? upleft : 0;      // r: the PASS's row, so its first has no row above
                const uint64_t raw = unfilter_unit(ft, unit, px, a, b, c);
                prev = cur; cur = raw;
                for (uint32_t k = 0; k < per; ++k) {
                    const uint32_t q = x * per + k;                 // the pass's column
                    if (q >= P.pw) break;                           // the row's last byte may hold fewer pixels
                    const uint32_t v = rgb_of_unit(ctype, depth, raw, k, R.pal);
                    uint8_t* o = orow + (size_t)q * P.dx * 3;       // x0 + q dx < w where q < pw
                    o[0] = (uint8_t)v; o[1] = (uint8_t)(v >> 8); o[2] = (uint8_t)(v >> 16);
                }
                if (lane == kLanes - 1) hand[x] = raw;
            }
        }
        __syncthreads();
    }
    if (bad) status[R.dst] = kStFilter;
}

PngDecLayout png_dec_layout(const pngparse::File* const* f, const size_t* rooms, const int* dst, int n, pngdec::Record* rec) {
    PngDecLayout L;
    L.bytes = (sizeof(Record) * (size_t)n + 255) / 256 * 256;
    size_t off = 0, scan = 0;
    for (int i = 0; i < n; ++i) {
        if (rec) {
            Record& r = rec[i];
            r.scan_off = scan; r.in_off = (uint32_t)off; r.in_len = (uint32_t)rooms[i];
            r.dst = (uint32_t)(dst ? dst[i] : i); r.reserved = 0;
            r.h = (uint32_t)f[i]->h; r.w = (uint32_t)f[i]->w; r.ctype = (uint32_t)f[i]->ctype; r.bpp = (uint32_t)f[i]->bpp;
            r.depth = (uint32_t)f[i]->depth; r.interlace = (uint32_t)f[i]->interlace; r.scan_total = (uint32_t)f[i]->scan_bytes(); r.pad = 0;
            std::memcpy(r.pal, f[i]->pal, sizeof(r.pal));
        }
        if (f[i]->depth != 8 || f[i]->interlace) L.any_form = true;
        if (f[i]->interlace) L.passes = (int)kMaxPasses;
        off += (rooms[i] + 3) & ~(size_t)3;
        scan += (f[i]->scan_bytes() + 15) & ~(size_t)15;
    }
    L.total = L.bytes + off;
    L.scan_bytes = scan;
    return L;
}

void png_dec_launch(const uint8_t* d_blob, const PngDecLayout& L, int n, int h, int w, uint8_t* d_scan, uint8_t* d_rgb, size_t image_pitch, int32_t* d_status, hipStream_t s,
                    hipEvent_t* marks, unsigned long long* d_ticks) {
    (void)h; (void)w;
    if (marks) IRE_HIP(hipEventRecord(marks[0], s));
    hipLaunchKernelGGL(png_inflate_kernel, dim3((unsigned)n), dim3(kLanes), 0, s, d_blob, L.bytes, d_scan, d_status, d_ticks);
    IRE_HIP(hipGetLastError());
    if (marks) IRE_HIP(hipEventRecord(marks[1], s));
    // a batch of the old form alone: the kernel it always had; else the one that branches per record, a workgroup per (image, pass)
    if (!L.any_form) hipLaunchKernelGGL(png_unfilter_kernel, dim3((unsigned)n), dim3(kLanes), 0, s, d_blob, d_scan, d_rgb, image_pitch, d_status);
    else hipLaunchKernelGGL(png_unfilter_any_kernel, dim3((unsigned)n, (unsigned)L.passes), dim3(kLanes), 0, s, d_blob, d_scan, d_rgb, image_pitch, d_status);
    IRE_HIP(hipGetLastError());
    if (marks) IRE_HIP(hipEventRecord(marks[2], s));
}

}  // namespace ire
