// jpeg_dec.hpp -- baseline JPEG files -> RGB pixels on the device (jpeg_dec.hip), behind the host parser (jpeg_parse.hpp).
#pragma once
#include "common.hpp"
#include "jpeg_parse.hpp"

namespace ire {
// where the parts of a batch's upload lie in its blob (bytes), and the widest image's stream counts (the grids of K1 / K2)
struct JpegDecLayout {
    size_t images = 0, tabs = 0, streams = 0, bytes = 0, total = 0;
    uint32_t max_long = 0, max_short = 0;
};
size_t jpeg_dec_coef_bytes(int n, int h, int w);       // device scratch: status words + coefficients; zeroed by the launch
size_t jpeg_dec_plane_bytes(int n, int h, int w);      // device scratch: the components' sample planes; needs no initialisation
JpegDecLayout jpeg_dec_layout(const jpegparse::Header* hd, const size_t* bytes, int n);
// files whose heads were accepted -> the blob (L.total bytes of host memory); fills the stream fields of hd[i].im and `out`.
// Throws Error(IRE_ERR_INVALID_INPUT) with the parser's reason when a scan is refused.
void jpeg_dec_pack(const uint8_t* const* files, const size_t* bytes, jpegparse::Header* hd, int n, const JpegDecLayout& L, uint8_t* blob, JpegDecLayout& out);
// the blob on the device -> n images of h x w x 3 bytes, image_pitch apart, and one status word per image (0: ok)
void jpeg_dec_launch(const uint8_t* d_blob, const JpegDecLayout& L, int n, int h, int w, uint8_t* d_coef, uint8_t* d_planes, uint8_t* d_rgb, size_t image_pitch,
                     int32_t* d_status, hipStream_t s, hipEvent_t* marks = nullptr);
// marks: null, or 6 timing events recorded before the memset and behind the memset, K1, K2, K3, K4 (tools/jpeg_decode_measure.py)
}  // namespace ire
