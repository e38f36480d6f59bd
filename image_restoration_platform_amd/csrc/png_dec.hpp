// png_dec.hpp -- PNG files -> RGB pixels on the device (png_dec.hip), behind the host parser (png_parse.hpp).
#pragma once
#include "common.hpp"
#include "png_inflate_core.hpp"
#include "png_parse.hpp"

namespace ire {
// A batch's upload: n records (pngdec::Record), then the zlib streams, each from a multiple of 4.  bytes: where the streams start.
struct PngDecLayout {
    size_t bytes = 0, total = 0;       // the records' bytes (a multiple of 256) | records and streams
    size_t scan_bytes = 0;             // device scratch: the filtered scanlines of all n images
    bool any_form = false;             // a file of another form than "8 bits, not interlaced" is among them: the second kernel is the per-pass one
    int passes = 1;                    // that kernel's workgroups per image: 7 when a file is interlaced
};
// rooms[i]: the bytes of file i's stream; dst[i]: which image of the output it becomes (null: image i).  Fills rec[i] when rec is not null.
PngDecLayout png_dec_layout(const pngparse::File* const* f, const size_t* rooms, const int* dst, int n, pngdec::Record* rec);
// the blob on the device -> file i to image dst[i] of h x w x 3 bytes, images image_pitch apart, and that image's status word (0: ok;
// pngdec::Status).
// Two launches whatever n.  d_scan: L.scan_bytes bytes, needs no initialisation.
void png_dec_launch(const uint8_t* d_blob, const PngDecLayout& L, int n, int h, int w, uint8_t* d_scan, uint8_t* d_rgb, size_t image_pitch, int32_t* d_status,
                    hipStream_t s, hipEvent_t* marks = nullptr, unsigned long long* d_ticks = nullptr);
// marks: null, or three timing events: before, between and behind the two kernels; d_ticks: null, or 3 * n words (png_dec.hip)
}  // namespace ire
