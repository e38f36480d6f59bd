// encode.hpp -- restored RGB pixels -> the base64 text of a PNG file, on the device, and the pad / crop of any-size jobs (encode.hip).
#pragma once
#include "common.hpp"

namespace ire {
size_t png_file_bytes(int h, int w);        // the PNG file: signature, IHDR, one IDAT of stored deflate blocks, IEND
size_t png_base64_chars(int h, int w);      // its base64 text ('=' padded, no terminator)
size_t png_scratch_bytes(int n, int h, int w);     // device scratch of a batch of n (the files + checksum state); needs no initialisation
// the top-left h x w window of n images, rows row_pitch and images image_pitch bytes apart -> n texts text_pitch bytes apart
void encode_png_base64_launch(const unsigned char* d_rgb, int n, int h, int w, size_t row_pitch, size_t image_pitch, unsigned char* d_scratch,
                              unsigned char* d_chars, size_t text_pitch, hipStream_t s);
// [n][h][w][3] -> [n][H][W][3], pixel (y, x) = source (min(y, h - 1), min(x, w - 1)); W a multiple of 8
void pad_edge_launch(const unsigned char* d_src, int n, int h, int w, unsigned char* d_dst, int H, int W, hipStream_t s);
// the same from the h x w windows of n images whose rows lie row_pitch and whose first pixels lie image_pitch bytes apart
void pad_edge_pitched_launch(const unsigned char* d_src, int n, int h, int w, size_t row_pitch, size_t image_pitch, unsigned char* d_dst, int H, int W, hipStream_t s);
// the top-left h x w window of [n][H][W][3] -> [n][h][w][3]
void crop_window_launch(const unsigned char* d_src, int n, int H, int W, unsigned char* d_dst, int h, int w, hipStream_t s);
}  // namespace ire
