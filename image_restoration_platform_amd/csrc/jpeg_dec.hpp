// jpeg_dec.hpp -- baseline and progressive JPEG files -> RGB pixels on the device (jpeg_dec.hip), behind the host parser (jpeg_parse.hpp).
#pragma once
#include "common.hpp"
#include "jpeg_parse.hpp"

#include <vector>

namespace ire {
// one dependency level of a batch (jpeg_parse.hpp: Scan::level): its records lie one behind the other, and so do their windows and chains
struct JpegDecLevel {
    uint32_t unit0 = 0, nunits = 0;
    uint32_t max_long = 0, max_short = 0;                          // the widest record's stream counts (the grids of K1 / K2)
    uint32_t win0 = 0, nwin = 0, chain0 = 0, nchain = 0;          // the streams of at least min_windows (>= 2) windows and their windows
    uint32_t dcref_blocks = 0, ac_blocks = 0, ac_streams = 0;     // the widest DC / AC refinement scan (the grids of their kernels)
    uint32_t ac_short = 0, ac_long = 0;                            // has an AC refinement stream of at most / of more than kShortMaxBytes
    uint32_t walk_blocks = 0;                                      // blocks of all its AC refinement scans
};
// where the parts of a batch's upload lie in its blob (bytes), and what the launch needs of the batch
struct JpegDecLayout {
    size_t images = 0, tabs = 0, streams = 0, chains = 0, windows = 0, bytes = 0, total = 0;
    uint32_t nchain = 0, nwin = 0, min_windows = 0, nunits = 0;    // over all levels; nunits: the records (a baseline file: one, a progressive one: its scans)
    size_t walk_blocks = 0;                                        // the most blocks one level's AC refinement scans have
    std::vector<JpegDecLevel> levels;
};
constexpr int kJpegDecMarks = 10;
size_t jpeg_dec_coef_bytes(int n, int h, int w);       // device scratch: status words + coefficients; zeroed by the launch
size_t jpeg_dec_plane_bytes(int n, int h, int w);      // device scratch: the components' sample planes; needs no initialisation
size_t jpeg_dec_lane_bytes(size_t nwin);               // device scratch: 32 bytes per lane and 16 per window of the multi-window streams; needs no initialisation
size_t jpeg_dec_walk_bytes(size_t blocks);             // device scratch: an 8-byte mask and a 4-byte walk record per block of a level's AC refinement scans; needs no initialisation
JpegDecLayout jpeg_dec_layout(const jpegparse::File* f, const size_t* bytes, int n);
// files that were planned (jpegparse::plan_file) -> the blob (L.total bytes of host memory) and `out`.
// Throws Error(IRE_ERR_INVALID_INPUT) with the parser's reason when a scan is refused.  min_windows: a long stream of at least so many
// windows (2 at the least) is decoded window-parallel and entered into the window table; 0: none is.
void jpeg_dec_pack(const uint8_t* const* files, const size_t* bytes, const jpegparse::File* f, int n, const JpegDecLayout& L, uint8_t* blob, JpegDecLayout& out,
                   uint32_t min_windows = 2);
// The same for files whose scans the caller cut before (jpegparse::split_file, each into memory of its own; rooms[i]: the bytes of
// image i's streams): the layout, and the records alone into the first L.bytes bytes of the blob.  byte_off[i]: where image i's
// bytes belong in the blob's byte area (from L.bytes on); the caller copies them there.
JpegDecLayout jpeg_dec_layout_rooms(const uint32_t* nstreams, const uint32_t* nscans, const size_t* rooms, int n);
void jpeg_dec_pack_streams(const jpegparse::File* const* f, const jpegdec::DecStream* const* streams, const size_t* rooms, int n, const JpegDecLayout& L, uint8_t* blob,
                           JpegDecLayout& out, size_t* byte_off, uint32_t min_windows = 2);
// the blob on the device -> n images of h x w x 3 bytes, image_pitch apart, and one status word per image (0: ok)
// d_lanes: jpeg_dec_lane_bytes(L.nwin) bytes, d_walk: jpeg_dec_walk_bytes(L.walk_blocks) bytes (each may be null when it has none)
void jpeg_dec_launch(const uint8_t* d_blob, const JpegDecLayout& L, int n, int h, int w, uint8_t* d_coef, uint8_t* d_planes, uint8_t* d_lanes, uint8_t* d_walk, uint8_t* d_rgb,
                     size_t image_pitch, int32_t* d_status, hipStream_t s, hipEvent_t* marks = nullptr, const int* dst = nullptr);
// dst: null, or n indices 0..63: file i becomes image dst[i] of d_rgb and sets status word dst[i] (null: image i)
// marks: null, or kJpegDecMarks timing events recorded before the memset and behind the memset, level 0's K1, spec, chain and write
// kernels and K2, everything a progressive file runs behind those (later levels, refinement scans), K3, K4 (tools/jpeg_decode_measure.py)
}  // namespace ire
