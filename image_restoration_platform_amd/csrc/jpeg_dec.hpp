// jpeg_dec.hpp -- baseline JPEG files -> RGB pixels on the device (jpeg_dec.hip), behind the host parser (jpeg_parse.hpp).
#pragma once
#include "common.hpp"
#include "jpeg_parse.hpp"

namespace ire {
// where the parts of a batch's upload lie in its blob (bytes), and the widest image's stream counts (the grids of K1 / K2)
struct JpegDecLayout {
    size_t images = 0, tabs = 0, streams = 0, chains = 0, windows = 0, bytes = 0, total = 0;
    uint32_t max_long = 0, max_short = 0;
    // the streams of at least min_windows (>= 2) windows and their windows: the grids of the chain kernel and of the spec / write kernels
    uint32_t nchain = 0, nwin = 0, min_windows = 0;
};
constexpr int kJpegDecMarks = 9;
size_t jpeg_dec_coef_bytes(int n, int h, int w);       // device scratch: status words + coefficients; zeroed by the launch
size_t jpeg_dec_plane_bytes(int n, int h, int w);      // device scratch: the components' sample planes; needs no initialisation
size_t jpeg_dec_lane_bytes(size_t nwin);               // device scratch: 32 bytes per lane and 16 per window of the multi-window streams; needs no initialisation
JpegDecLayout jpeg_dec_layout(const jpegparse::Header* hd, const size_t* bytes, int n);
// files whose heads were accepted -> the blob (L.total bytes of host memory); fills the stream fields of hd[i].im and `out`.
// Throws Error(IRE_ERR_INVALID_INPUT) with the parser's reason when a scan is refused.  min_windows: a long stream of at least so many
// windows (2 at the least) is decoded window-parallel and entered into the window table; 0: none is.
void jpeg_dec_pack(const uint8_t* const* files, const size_t* bytes, jpegparse::Header* hd, int n, const JpegDecLayout& L, uint8_t* blob, JpegDecLayout& out,
                   uint32_t min_windows = 2);
// the blob on the device -> n images of h x w x 3 bytes, image_pitch apart, and one status word per image (0: ok)
// The same for files whose scans the caller cut before (jpegparse::split_scan, each into memory of its own; rooms[i]: the bytes of
// image i's streams): the layout, and the records alone into the first L.bytes bytes of the blob.  byte_off[i]: where image i's
// bytes belong in the blob's byte area (from L.bytes on); the caller copies them there.
JpegDecLayout jpeg_dec_layout_rooms(const uint32_t* nstreams, const size_t* rooms, int n);
void jpeg_dec_pack_streams(const jpegparse::Header* const* hd, const jpegdec::DecStream* const* streams, const size_t* rooms, int n, const JpegDecLayout& L, uint8_t* blob,
                           JpegDecLayout& out, size_t* byte_off, uint32_t min_windows = 2);
// d_lanes: jpeg_dec_lane_bytes(L.nwin) bytes (may be null when L.nwin is 0)
void jpeg_dec_launch(const uint8_t* d_blob, const JpegDecLayout& L, int n, int h, int w, uint8_t* d_coef, uint8_t* d_planes, uint8_t* d_lanes, uint8_t* d_rgb,
                     size_t image_pitch, int32_t* d_status, hipStream_t s, hipEvent_t* marks = nullptr);
// marks: null, or kJpegDecMarks timing events recorded before the memset and behind the memset, K1, the spec, chain and write kernels
// of the multi-window streams, K2, K3, K4 (tools/jpeg_decode_measure.py)
}  // namespace ire
