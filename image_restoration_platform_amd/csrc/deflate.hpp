// deflate.hpp -- restored RGB pixels -> the base64 text of a PNG file with Huffman-coded deflate blocks, on the device (deflate.hip).
#pragma once
#include "common.hpp"

namespace ire {
size_t png_deflate_file_bound(int h, int w);        // the largest file any h x w image can give (derivation: deflate.hip, blk_bound)
size_t png_deflate_base64_bound(int h, int w);      // its base64 text
size_t png_deflate_scratch_bytes(int n, int h, int w);     // device scratch of a batch of n; needs no initialisation
// the top-left h x w window of n images, rows row_pitch and images image_pitch bytes apart -> n texts text_pitch bytes apart (at most
// png_deflate_base64_bound(h, w) characters each) and their character counts, one uint64 per image, lens_pitch bytes apart
void encode_png_deflate_base64_launch(const unsigned char* d_rgb, int n, int h, int w, size_t row_pitch, size_t image_pitch, unsigned char* d_scratch,
                                      unsigned char* d_chars, size_t text_pitch, unsigned char* d_lens, size_t lens_pitch, hipStream_t s);
// K4 alone, shared with jpeg.hip: base64 of n files file_pitch bytes apart whose lengths (at most file_bound) lie in device memory.
// Every file must be readable up to the next multiple of 12 behind its length; file_pitch a multiple of 4.
void base64_device_length_launch(const unsigned char* d_files, size_t file_pitch, const unsigned long long* d_flen, size_t file_bound, int n, unsigned char* d_chars,
                                 size_t text_pitch, hipStream_t s);
}  // namespace ire
