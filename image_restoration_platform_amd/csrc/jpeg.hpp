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
// what jpeg_progenc.hip takes from jpeg.hip: the front end alone (pixels -> quantised coefficients, int16 in zig-zag order, in the
// layout of jpeg_progenc_core.hpp's Geom, n images of nblocks * 64 apart), and the table kernel on ntab histograms per image
void jpeg_coefs_launch(const unsigned char* d_rgb, int n, int h, int w, size_t row_pitch, size_t image_pitch, int quality, int sampling, short* d_coefs, hipStream_t s);
void jpeg_tables_launch(const unsigned* d_counts, int ntab, int n, unsigned char* d_bits_vals, int* d_nvals, unsigned* d_codes, hipStream_t s);

// jpeg_progenc.hip -- the same pixels as a PROGRESSIVE file: libjpeg's ten jpeg_simple_progression scans, each under its own optimal
// table, a restart interval of one MCU row of the scan (the file of Pillow's progressive=True, restart_marker_rows=1)
size_t jpeg_progressive_file_bound(int h, int w, int quality, int sampling);
size_t jpeg_progressive_base64_bound(int h, int w, int quality, int sampling);
size_t jpeg_progressive_scratch_bytes(int n, int h, int w, int quality, int sampling);
void encode_jpeg_progressive_base64_launch(const unsigned char* d_rgb, int n, int h, int w, size_t row_pitch, size_t image_pitch, unsigned char* d_scratch,
                                           unsigned char* d_chars, size_t text_pitch, unsigned char* d_lens, size_t lens_pitch, int quality, int sampling, hipStream_t s);
// ire_debug_jpeg_progressive_from_coefs: everything behind the coefficient pass on coefficients given (d_coefs: n x nblocks x 64
// int16 on the device) -> n files in d_scratch, at *files_off + i * *file_pitch, their lengths as uint64 at *flen_off
void jpeg_progressive_from_coefs_launch(const short* d_coefs, int n, int h, int w, int quality, int sampling, unsigned char* d_scratch, size_t* files_off,
                                        size_t* file_pitch, size_t* flen_off, hipStream_t s);
size_t jpeg_progressive_coef_count(int h, int w, int sampling);      // int16 values per image
}  // namespace ire
