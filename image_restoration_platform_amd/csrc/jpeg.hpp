// jpeg.hpp -- restored RGB pixels -> the base64 text of a baseline JPEG file, on the device (jpeg.hip).  quality: 1..100, the IJG
// scaling of the Annex K tables; sampling: 0 = 4:4:4, 2 = 4:2:0 (as ire_decode_jpeg_plan numbers it).  Anything else is refused.
// optimize: the file carries the image's own Huffman tables (libjpeg's optimize_coding) instead of the Annex K ones; its bound is
// the one under any table (jpeg_tables.hpp), larger than the fixed tables'.
#pragma once
#include "common.hpp"

namespace ire {
constexpr int kJpegDefaultQuality = 85, kJpegDefaultSampling = 0;
size_t jpeg_file_bound(int h, int w, int quality, int sampling, bool optimize = false);      // the largest file any h x w image can give (derivation: jpeg_tables.hpp)
size_t jpeg_base64_bound(int h, int w, int quality, int sampling, bool optimize = false);    // its base64 text
size_t jpeg_scratch_bytes(int n, int h, int w, int quality, int sampling, bool optimize = false);      // device scratch of a batch of n; needs no initialisation
// the top-left h x w window of n images, rows row_pitch and images image_pitch bytes apart -> n texts text_pitch bytes apart (at most
// jpeg_base64_bound(h, w, quality, sampling, optimize) characters each) and their character counts, one uint64 per image, lens_pitch
// bytes apart
void encode_jpeg_base64_launch(const unsigned char* d_rgb, int n, int h, int w, size_t row_pitch, size_t image_pitch, unsigned char* d_scratch,
                               unsigned char* d_chars, size_t text_pitch, unsigned char* d_lens, size_t lens_pitch, int quality, int sampling, bool optimize, hipStream_t s);
// the optimised path's table kernel alone: d_counts [n][4][256] -> d_bits_vals [n][4][16 + 256] and d_nvals [n][4]
void jpeg_huffman_tables_launch(const unsigned* d_counts, int n, unsigned char* d_bits_vals, int* d_nvals, hipStream_t s);
}  // namespace ire
