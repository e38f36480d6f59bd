// jpeg_progenc.hip -- restored RGB pixels -> the base64 text of a PROGRESSIVE JPEG file, on the device: the quantised coefficients of
// jpeg.hip's front end sent as libjpeg's ten jpeg_simple_progression scans, each under its own optimal Huffman table, with a restart
// interval of one MCU row of the scan.  The file is byte for byte Pillow's for progressive=True, restart_marker_rows=1
// (tests/jpeg_progenc_model.py on the CPU; the device equals the model: tests/test_jpeg_progenc_gpu.py).  The coder itself is
// jpeg_progenc_core.hpp, the same code tests/native/jpeg_progenc_sim.cpp runs on the CPU.
//
// A memset of the histograms and seven launches per BATCH, none depending on n or on the image, no host round trip:
//   K0 jpeg.hip's K1 in kCoefs mode   pixels -> colour transform -> (h2v2, dummy blocks) -> islow DCT -> quantiser -> zig-zag, ONCE per
//                                     image, the coefficients as int16 to scratch (128 bytes per block).  Ten scans in two passes each
//                                     would otherwise run the DCT twenty times: the "recompute, not store" choice of
//                                     profiles/jpeg_huffopt.md flips here.
//   K1 prog_walk_kernel<count>        one LANE per restart interval (scan, block row), one workgroup of 64 lanes per 64 rows of one scan:
//                                     the lane walks its interval's blocks in order (walk_interval) and counts the symbols into the
//                                     workgroup's LDS histograms -- a workgroup serves one scan, so one or two tables -- which are added
//                                     to the image's ten in global memory by integer atomics
//   K2 jpeg.hip's jpeg_table_kernel   on a (10, n) grid
//   K3 prog_walk_kernel<emit>         the same walk under the scan's codes (in LDS): MSB-first bits, byte stuffing, the interval's RSTm
//                                     and its byte count to a scratch slot sized by the scan's interval bound
//   K4 prog_prefix_kernel, prog_gather_kernel   one workgroup per image: the prefix sums of its interval sizes; then one workgroup per
//                                     interval: its place from the prefix and the scan heads before it
//                                     (DHT from the device's tables, DRI where the interval changes, SOS); the first interval of a scan
//                                     writes that scan's head, interval 0 the fixed head, the last EOI and the two lengths
//   K5 deflate_base64_kernel          (deflate.hip) base64 over the device-side length
// Everything is integer work, integer atomics and fixed-order sums: the bytes are a pure function of the pixels and the two settings.
//
// The walk is one lane per interval, NOT a wave per interval with lane k = zig-zag position k: the state that crosses blocks (EOBRUN,
// up to 1000 buffered correction bits, the place of every ZRL in a refinement block) makes the ballot form a second algorithm that
// would have to be held to the model separately, and this one is the model's own order of events in the very code the CPU program
// runs.  Its price is measured in profiles/jpeg_progressive.md: the lanes of a wave diverge, a 1024^2 image gives only 18 - 20 waves,
// and the call takes 15 (4:4:4) to 22 (4:2:0) times the optimised call's time -- 0.73 ms per 1024^2 image, 4.3 of the batch's 5.8 ms
// in the emit pass.  That is small beside the host seam the result text is for (14.7 ms per image at 68 img/s) and large beside the
// restore itself (0.9 ms per image); the wave-per-interval walk is what would close it and is not built.  What keeps the lane form
// from being slower still: a block's 128 bytes come to the lane's LDS in eight wide loads, a pass of 63 independent compares turns
// the block into bit masks so that the coders visit the non-zero positions alone, and the emit pass stores its bytes eight at a
// time.  The correction bits of a lane live in LDS (8 KB per workgroup, words 64 apart), not in private memory.
#include "jpeg.hpp"

#include "deflate.hpp"
#include "jpeg_tables.hpp"

namespace ire {

namespace {

using namespace jpegprog;

constexpr int kLanes = 64, kGatherThreads = 256;

struct ProgPlan {
    Geom g;
    unsigned stride[kScans];                  // scratch bytes of one interval of the scan: its bound (jpeg_tables.hpp)
    unsigned long long base[kScans + 1];      // the scan's first slot inside an image's interval scratch; [kScans]: bytes per image
    unsigned groups;                          // workgroups per scan: ceil(the most block rows of any scan / 64)
    unsigned long long file_bound;
};
ProgPlan plan_of(int h, int w, int quality, int sampling) {
    if (!jpegtab::settings_ok(quality, sampling)) fail(IRE_ERR_INVALID_INPUT, "invalid settings for the JPEG encoder (quality 1..100; sampling 0 = 4:4:4 or 2 = 4:2:0)");
    if (h <= 0 || w <= 0 || h > 8192 || w > 8192) fail(IRE_ERR_INVALID_INPUT, "invalid image size for the JPEG encoder (1..8192 per side)");
    ProgPlan p{};
    p.g = geom_of(h, w, sampling);
    unsigned most = 0;
    p.base[0] = 0;
    for (int s = 0; s < kScans; ++s) {
        const size_t b = jpegtab::prog_interval_bound(p.g, quality, s);       // (<= 2 * (3072 * 27 / 8) + 2 at 8192 wide: far below 2^32)
        p.stride[s] = (unsigned)((b + 7) / 8 * 8);                           // (ByteSink stores words of 8 bytes)
        p.base[s + 1] = p.base[s] + (unsigned long long)p.stride[s] * scan_rows(p.g, s);
        if (scan_rows(p.g, s) > most) most = scan_rows(p.g, s);
    }
    p.groups = (most + kLanes - 1) / kLanes;
    p.file_bound = jpegtab::jpeg_prog_file_bound(h, w, quality, sampling);
    return p;
}

struct CountSink {
    unsigned* h;                              // the workgroup's LDS histograms, from table slot0 on
    int slot0;
    __device__ __forceinline__ void sym(int slot, int s) { atomicAdd(&h[(slot - slot0) * 256 + (s & 255)], 1u); }
    __device__ __forceinline__ void bits(uint32_t, unsigned) {}
};

// The AC coders' block, staged: 128 bytes from the coefficient scratch (16-byte aligned: the scratch's parts are 256-byte aligned and a
// block is 128 bytes) to the lane's own 144 bytes of LDS, eight loads in flight at once.  The lane alone writes and reads them.
typedef uint4 __attribute__((may_alias)) Chunk;
constexpr int kBlkChunks = 9;                 // 8 of coefficients and 1 of padding, so that the lanes' copies start in different banks
struct LdsBlocks {
    Chunk* own;
    __device__ __forceinline__ const int16_t* operator()(const int16_t* p) const {
        const Chunk* src = reinterpret_cast<const Chunk*>(p);
        Chunk v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = src[j];
#pragma unroll
        for (int j = 0; j < 8; ++j) own[j] = v[j];
        return reinterpret_cast<const int16_t*>(own);
    }
};

// K1 / K3.  blockIdx.x: scan * groups + the group of 64 block rows; blockIdx.y: the image; the lane: the block row.
template <bool kEmit>
__global__ __launch_bounds__(kLanes) void prog_walk_kernel(ProgPlan p, const short* __restrict__ coefs, unsigned* __restrict__ hist, const unsigned* __restrict__ codes,
                                                           unsigned char* __restrict__ intbuf, unsigned* __restrict__ int_bytes) {
    __shared__ unsigned s_corr[kCorrWords * kLanes];
    __shared__ unsigned s_tab[2 * 256];       // count: the scan's histograms; emit: its codes
    __shared__ uint4 s_blk[kLanes * kBlkChunks];
    const unsigned lane = threadIdx.x, img = blockIdx.y;
    const int scan = (int)(blockIdx.x / p.groups);
    const unsigned row = (blockIdx.x % p.groups) * kLanes + lane, rows = scan_rows(p.g, scan);
    const int t0 = first_table(scan), nt = table_count(scan);
    if ((blockIdx.x % p.groups) * kLanes >= rows) return;                      // (the whole workgroup: no barrier is left behind)
    const unsigned* const own = codes + ((unsigned long long)img * kTables + (unsigned)t0) * 256ull;
    for (int k = (int)lane; k < nt * 256; k += kLanes) s_tab[k] = kEmit ? own[k] : 0u;
    __syncthreads();
    const short* const c = coefs + (unsigned long long)img * p.g.nblocks * 64ull;
    const LdsBlocks stage{reinterpret_cast<Chunk*>(s_blk) + lane * kBlkChunks};
    if (row < rows) {
        if constexpr (kEmit) {
            const unsigned long long slot = (unsigned long long)img * p.g.int0[kScans] + p.g.int0[scan] + row;
            ByteSink bs{intbuf + (unsigned long long)img * p.base[kScans] + p.base[scan] + (unsigned long long)row * p.stride[scan], 0u, p.stride[scan], s_tab, t0, 0ull, 0u, 0ull};
            walk_interval(p.g, scan, row, c, bs, s_corr + lane, (unsigned)kLanes, nullptr, stage);
            bs.finish(row + 1 == rows ? 0 : 0xd0 + (int)(row & 7u));
            int_bytes[slot] = bs.n < p.stride[scan] ? bs.n : p.stride[scan];   // (never beyond: the bound; ByteSink wrote nothing past it either)
        } else {
            CountSink cs{s_tab, t0};
            walk_interval(p.g, scan, row, c, cs, s_corr + lane, (unsigned)kLanes, nullptr, stage);
        }
    }
    if constexpr (!kEmit) {
        __syncthreads();
        unsigned* const dst = hist + ((unsigned long long)img * kTables + (unsigned)t0) * 256ull;
        for (int k = (int)lane; k < nt * 256; k += kLanes) { const unsigned v = s_tab[k]; if (v) atomicAdd(&dst[k], v); }
    }
}

struct FixedHead { unsigned char b[kFixedHead]; };

// K4a.  One workgroup per image: the exclusive prefix sums of its interval sizes, prefix[nint] their total.  A thread sums a run of
// consecutive intervals, one thread adds the 256 run sums up, every thread writes its run's prefixes: one pass, a fixed order.
__global__ __launch_bounds__(kGatherThreads) void prog_prefix_kernel(unsigned nint, const unsigned* __restrict__ int_bytes, unsigned long long* __restrict__ prefix) {
    __shared__ unsigned long long s_run[kGatherThreads];
    const unsigned img = blockIdx.x, t = threadIdx.x;
    const unsigned* sizes = int_bytes + (unsigned long long)img * nint;
    unsigned long long* out = prefix + (unsigned long long)img * (nint + 1ull);
    const unsigned per = (nint + kGatherThreads - 1) / kGatherThreads, k0 = min(t * per, nint), k1 = min(k0 + per, nint);
    unsigned long long sum = 0;
    for (unsigned k = k0; k < k1; ++k) sum += sizes[k];
    s_run[t] = sum;
    __syncthreads();
    if (t == 0) {
        unsigned long long run = 0;
        for (int k = 0; k < kGatherThreads; ++k) { const unsigned long long v = s_run[k]; s_run[k] = run; run += v; }
        out[nint] = run;
    }
    __syncthreads();
    unsigned long long run = s_run[t];
    for (unsigned k = k0; k < k1; ++k) { out[k] = run; run += sizes[k]; }
}

// K4.  blockIdx.x: the interval (all scans' in file order), blockIdx.y: the image.
__global__ __launch_bounds__(kGatherThreads) void prog_gather_kernel(ProgPlan p, FixedHead head, const unsigned char* __restrict__ intbuf, const unsigned* __restrict__ int_bytes,
                                                                     const unsigned long long* __restrict__ prefix, const unsigned char* __restrict__ bits_vals, const int* __restrict__ nvals,
                                                                     unsigned char* __restrict__ files, unsigned long long file_pitch, unsigned long long* __restrict__ flen,
                                                                     unsigned char* __restrict__ lens, unsigned long long lens_pitch) {
    const unsigned iv = blockIdx.x, img = blockIdx.y, t = threadIdx.x, nint = p.g.int0[kScans];
    const unsigned* sizes = int_bytes + (unsigned long long)img * nint;
    const unsigned long long* pre = prefix + (unsigned long long)img * (nint + 1ull);
    const unsigned long long before = pre[iv], all = pre[nint];
    const int scan = scan_of_interval(p.g, iv);
    const int* nv = nvals + (unsigned long long)img * kTables;
    const unsigned char* bv = bits_vals + (unsigned long long)img * kTables * jpeghuff::kBitsVals;
    unsigned long long heads_to = kFixedHead, heads_all = kFixedHead;          // the heads up to and with this scan's | all of them
    unsigned my_head = 0;
    for (int s = 0; s < kScans; ++s) {
        const unsigned hb = scan_head_bytes(p.g, s, nv);
        heads_all += hb;
        if (s <= scan) heads_to += hb;
        if (s == scan) my_head = hb;
    }
    unsigned char* __restrict__ file = files + (unsigned long long)img * file_pitch;
    const unsigned size = sizes[iv];
    const unsigned long long d0 = heads_to + before;
    const unsigned char* __restrict__ srcb = intbuf + (unsigned long long)img * p.base[kScans] + p.base[scan] + (unsigned long long)(iv - p.g.int0[scan]) * p.stride[scan];
    for (unsigned k = t; k < size; k += kGatherThreads) if (d0 + k < p.file_bound) file[d0 + k] = srcb[k];
    if (iv == p.g.int0[scan])
        for (unsigned k = t; k < my_head; k += kGatherThreads) file[d0 - my_head + k] = scan_head_byte(p.g, scan, k, bv, nv);
    if (iv == 0)
        for (unsigned k = t; k < kFixedHead; k += kGatherThreads) file[k] = head.b[k];
    if (iv + 1 == nint) {
        const unsigned long long fl = heads_all + all + 2;
        if (t < 2) file[fl - 2 + t] = t ? 0xd9 : 0xff;
        if (t >= 64 && t < 64 + 48) { const unsigned long long o = fl + (t - 64); if (o < file_pitch) file[o] = 0; }      // what the last base64 thread reads behind the file
        if (t == 128) {
            flen[img] = fl;
            const unsigned long long chars = (fl + 2) / 3 * 4;
            unsigned char* lp = lens + (unsigned long long)img * lens_pitch;
            if ((reinterpret_cast<unsigned long long>(lp) & 7u) == 0) *reinterpret_cast<unsigned long long*>(lp) = chars;
            else for (int k = 0; k < 8; ++k) lp[k] = (unsigned char)(chars >> (8 * k));
        }
    }
}

struct ProgLayout { size_t flen, lens, int_bytes, prefix, hist, codes, bits_vals, nvals, coefs, intbuf, files, file_pitch, total; };
ProgLayout layout_of(int n, const ProgPlan& p) {
    ProgLayout L;
    auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    const size_t nint = p.g.int0[kScans];
    L.flen = 0;                                                      // n x u64
    L.lens = up((size_t)n * 8);                                      // n x u64: the character counts of a call that has no place for them
    L.int_bytes = up(L.lens + (size_t)n * 8);                        // n x nint u32
    L.prefix = up(L.int_bytes + (size_t)n * nint * 4);               // n x (nint + 1) u64
    L.hist = up(L.prefix + (size_t)n * (nint + 1) * 8);               // per image and table: 256 counts | 256 codes | bits and vals | the symbol count
    L.codes = L.hist + (size_t)n * kTables * 256 * 4;
    L.bits_vals = L.codes + (size_t)n * kTables * 256 * 4;
    L.nvals = up(L.bits_vals + (size_t)n * kTables * jpeghuff::kBitsVals);
    L.coefs = up(L.nvals + (size_t)n * kTables * 4);                 // n x nblocks x 64 int16: 128 bytes per block
    L.intbuf = up(L.coefs + (size_t)n * p.g.nblocks * 128);          // n x every interval at its scan's bound
    L.files = up(L.intbuf + (size_t)n * (size_t)p.base[kScans]);
    L.file_pitch = up(((size_t)p.file_bound + 11) / 12 * 12 + 64);   // (the 12-byte groups of the last base64 threads stay inside)
    L.total = L.files + L.file_pitch * (size_t)n;
    return L;
}

// K1 .. K4 on the coefficients at L.coefs
void entropy_launch(const ProgPlan& p, const ProgLayout& L, int n, int h, int w, int quality, int sampling, unsigned char* d_scratch, unsigned char* d_lens, size_t lens_pitch,
                    hipStream_t s) {
    unsigned* hist = reinterpret_cast<unsigned*>(d_scratch + L.hist);
    unsigned* codes = reinterpret_cast<unsigned*>(d_scratch + L.codes);
    unsigned char* bits_vals = d_scratch + L.bits_vals;
    int* nvals = reinterpret_cast<int*>(d_scratch + L.nvals);
    const short* coefs = reinterpret_cast<const short*>(d_scratch + L.coefs);
    unsigned* int_bytes = reinterpret_cast<unsigned*>(d_scratch + L.int_bytes);
    const dim3 walk_grid(kScans * p.groups, n);
    IRE_HIP(hipMemsetAsync(hist, 0, (size_t)n * kTables * 256 * 4, s));
    hipLaunchKernelGGL(prog_walk_kernel<false>, walk_grid, dim3(kLanes), 0, s, p, coefs, hist, (const unsigned*)codes, d_scratch + L.intbuf, int_bytes);
    jpeg_tables_launch(hist, kTables, n, bits_vals, nvals, codes, s);
    hipLaunchKernelGGL(prog_walk_kernel<true>, walk_grid, dim3(kLanes), 0, s, p, coefs, hist, (const unsigned*)codes, d_scratch + L.intbuf, int_bytes);
    unsigned long long* prefix = reinterpret_cast<unsigned long long*>(d_scratch + L.prefix);
    hipLaunchKernelGGL(prog_prefix_kernel, dim3(n), dim3(kGatherThreads), 0, s, p.g.int0[kScans], (const unsigned*)int_bytes, prefix);
    FixedHead head;
    const jpegtab::JpegHeader fixed = jpegtab::jpeg_header(h, w, quality, sampling);
    for (unsigned k = 0; k < kFixedHead; ++k) head.b[k] = fixed.b[k];
    head.b[2 + 18 + 69 + 69 + 1] = 0xc2;                             // SOF2: progressive, Huffman-coded
    hipLaunchKernelGGL(prog_gather_kernel, dim3(p.g.int0[kScans], n), dim3(kGatherThreads), 0, s, p, head, (const unsigned char*)(d_scratch + L.intbuf), (const unsigned*)int_bytes,
                       (const unsigned long long*)prefix, (const unsigned char*)bits_vals, (const int*)nvals, d_scratch + L.files, (unsigned long long)L.file_pitch,
                       reinterpret_cast<unsigned long long*>(d_scratch + L.flen), d_lens, (unsigned long long)lens_pitch);
    IRE_HIP(hipGetLastError());
}

}  // namespace

size_t jpeg_progressive_file_bound(int h, int w, int quality, int sampling) { return (size_t)plan_of(h, w, quality, sampling).file_bound; }
size_t jpeg_progressive_base64_bound(int h, int w, int quality, int sampling) { return ((size_t)plan_of(h, w, quality, sampling).file_bound + 2) / 3 * 4; }
size_t jpeg_progressive_scratch_bytes(int n, int h, int w, int quality, int sampling) { return layout_of(n, plan_of(h, w, quality, sampling)).total; }
size_t jpeg_progressive_coef_count(int h, int w, int sampling) { return (size_t)geom_of(h, w, sampling).nblocks * 64; }

void encode_jpeg_progressive_base64_launch(const unsigned char* d_rgb, int n, int h, int w, size_t row_pitch, size_t image_pitch, unsigned char* d_scratch, unsigned char* d_chars,
                                           size_t text_pitch, unsigned char* d_lens, size_t lens_pitch, int quality, int sampling, hipStream_t s) {
    if (n < 1 || n > 65535) fail(IRE_ERR_INVALID_INPUT, "invalid image count for the JPEG encoder");
    const ProgPlan p = plan_of(h, w, quality, sampling);
    const ProgLayout L = layout_of(n, p);
    jpeg_coefs_launch(d_rgb, n, h, w, row_pitch, image_pitch, quality, sampling, reinterpret_cast<short*>(d_scratch + L.coefs), s);
    entropy_launch(p, L, n, h, w, quality, sampling, d_scratch, d_lens, lens_pitch, s);
    base64_device_length_launch(d_scratch + L.files, L.file_pitch, reinterpret_cast<const unsigned long long*>(d_scratch + L.flen), (size_t)p.file_bound, n, d_chars, text_pitch, s);
    IRE_HIP(hipGetLastError());
}

void jpeg_progressive_from_coefs_launch(const short* d_coefs, int n, int h, int w, int quality, int sampling, unsigned char* d_scratch, size_t* files_off, size_t* file_pitch,
                                        size_t* flen_off, hipStream_t s) {
    if (n < 1 || n > 65535) fail(IRE_ERR_INVALID_INPUT, "invalid image count for the JPEG encoder");
    const ProgPlan p = plan_of(h, w, quality, sampling);
    const ProgLayout L = layout_of(n, p);
    IRE_HIP(hipMemcpyAsync(d_scratch + L.coefs, d_coefs, (size_t)n * p.g.nblocks * 128, hipMemcpyDeviceToDevice, s));
    entropy_launch(p, L, n, h, w, quality, sampling, d_scratch, d_scratch + L.lens, 8, s);
    *files_off = L.files; *file_pitch = L.file_pitch; *flen_off = L.flen;
}

}  // namespace ire
