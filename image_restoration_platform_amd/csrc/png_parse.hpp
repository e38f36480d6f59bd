// png_parse.hpp -- the host side of the device's PNG decoder (png_dec.hip): reads a file's chunks, decides whether the device decodes
// it and says where its zlib stream lies.  Host-only, header-only, plain C++17, no HIP: libire.so uses it in front of png_dec.hip,
// tests/native/png_dec_sim.cpp and png_fuzz.cpp compile it alone under ASan and UBSan.  No read goes past `bytes`, whatever the file
// says: every access goes through Cursor, and lengths are compared by subtraction, never summed.
//
// Accepted: the signature, IHDR first; bit depth 8; colour type 0, 2, 3, 4 or 6 (1, 3, 1, 2 or 4 bytes per pixel); compression 0,
// filter method 0, interlace 0; 1..8192 per side; PLTE of 1..256 entries (required for type 3); one or more CONSECUTIVE IDAT chunks,
// empty ones among them; behind the last IDAT whole chunks and then IEND (its CRC may be cut off), or the end of the file where a
// chunk would begin or inside a chunk's eight header bytes -- what Pillow still reads; a chunk there whose header is whole and whose
// payload or CRC the file does not hold is refused (Pillow raises on a cut payload).  tRNS is read past: alpha of any kind is dropped, as PIL's
// convert("RGB") drops it.  gAMA, cHRM, sRGB, pHYs, text and every other ancillary chunk are skipped.
// Refused ("invalid: PNG ..."): another bit depth, Adam7, APNG (acTL in front of IDAT), type 3 without PLTE, an IHDR, a PLTE or any
// other chunk in front of IDAT whose CRC-32 is wrong (Pillow checks them all), a chunk that overruns the file, IDAT chunks that are not consecutive, no IDAT, a zlib header that is not deflate
// with a window of at most 32 KiB and no preset dictionary; with kRefuseIccp a file that carries iCCP.
// IDAT CRCs are NOT checked: Pillow does not check them either, and the stream's Adler-32, which the device compares, covers the data.
// A refused file stays with the host codec, so being stricter than Pillow is safe; being laxer is not.
// With kAcceptAll (below) the depth and interlace rules widen to every standard form but 16-bit grey; a PLTE longer than 2^depth entries
// is taken as Pillow takes it (the entries no index reaches are never read), one shorter gives black past its end, as at depth 8.
// The FIRST eXIf chunk in front of IDAT gives the orientation by jpeg_parse.hpp's TIFF walk; a broken chunk is orientation 1, never a refusal.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "jpeg_parse.hpp"
#include "png_adam7_core.hpp"

namespace ire {
namespace pngparse {

constexpr uint32_t kRefuseIccp = 4u;       // ire.h: IRE_DECODE_ACCEPT_ICC -- the caller would have to read the profile; that is a later change
// ire.h: IRE_DECODE_ACCEPT_PNG_ALL -- beside the 8-bit, non-interlaced files: depth 1, 2 and 4 for colour types 0 and 3, depth 16 for colour
// types 2, 4 and 6, and Adam7 for all of them (png_adam7_core.hpp).  Without the bit every answer and every reason is what it was.
// Still refused with it: the (type, depth) pairs the PNG specification forbids (Pillow refuses them too), and 16-bit GREY: Pillow opens
// it as I;16 and convert("RGB") clips (0x0100 -> 255), sharp takes the high byte, so no device result could equal both host codecs.
constexpr uint32_t kAcceptAll = 32u;

struct Span { size_t off, len; };          // an IDAT chunk's payload in the file
struct File {
    int h = 0, w = 0, ctype = 0, bpp = 0;  // bpp: the filter unit's bytes, 1..4 for an 8-bit file, up to 8 for a 16-bit one, 1 below 8 bits
    int depth = 8, interlace = 0;
    uint32_t npal = 0;
    uint8_t pal[768] = {};                 // zeros behind the last entry
    size_t idat_bytes = 0;                 // the zlib stream: what stage() copies, and the job's room
    std::vector<Span> spans;               // the non-empty IDAT payloads, in file order
    int orientation = 1;
    bool iccp = false;
    // the filtered scanlines: the sum over the passes of rows * (1 + row bytes); h * (1 + w * bpp) for an 8-bit file without interlace
    size_t scan_bytes() const { return (size_t)pngdec::scan_total((uint32_t)h, (uint32_t)w, (uint32_t)ctype, (uint32_t)depth, (uint32_t)interlace); }
};

struct Cursor {
    const uint8_t* p;
    size_t n, i = 0;
    bool ok = true;
    Cursor(const uint8_t* p_, size_t n_) : p(p_), n(n_) {}
    size_t left() const { return n - i; }
    unsigned u8() { if (i >= n) { ok = false; return 0; } return p[i++]; }
    uint32_t u32() { uint32_t v = 0; for (int k = 0; k < 4; ++k) v = v << 8 | u8(); return v; }
};

inline bool refuse(std::string& why, const char* reason) { why = std::string("invalid: PNG ") + reason; return false; }

inline bool is_png(const uint8_t* file, size_t bytes) { return file && bytes >= 8 && !std::memcmp(file, "\x89PNG\r\n\x1a\n", 8); }

// CRC-32 of p[0 .. n) (the chunk's type and payload)
inline uint32_t crc32(const uint8_t* p, size_t n) {
    struct Table {
        uint32_t t[256];
        Table() { for (uint32_t v = 0; v < 256; ++v) { uint32_t c = v; for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u))); t[v] = c; } }
    };
    static const Table T;
    uint32_t c = 0xFFFFFFFFu;
    for (size_t i = 0; i < n; ++i) c = T.t[(c ^ p[i]) & 255u] ^ (c >> 8);
    return ~c;
}
constexpr uint32_t tag(char a, char b, char c, char d) { return (uint32_t)(uint8_t)a << 24 | (uint32_t)(uint8_t)b << 16 | (uint32_t)(uint8_t)c << 8 | (uint8_t)d; }

// the whole decision for one file
inline bool plan_file(const uint8_t* file, size_t bytes, uint32_t flags, File& f, std::string& why) {
    f = File{};
    if (!is_png(file, bytes)) return refuse(why, "file without the PNG signature");
    if (bytes >= ((size_t)1 << 31)) return refuse(why, "file of 2 GB or more");
    Cursor c(file, bytes);
    c.i = 8;
    bool have_ihdr = false, have_plte = false, have_exif = false, idat_open = false, idat_closed = false;
    while (c.left() > 0) {
        const uint32_t len = c.u32(), type = c.u32();
        if (!c.ok) { if (idat_open || idat_closed) break; return refuse(why, "chunk that overruns the file"); }
        // payload and CRC: compared by subtraction.  Only an empty IEND behind the data may lack its CRC.
        if (c.left() < 4 || (size_t)len > c.left() - 4) {
            if ((idat_open || idat_closed) && type == tag('I', 'E', 'N', 'D') && len == 0) break;
            return refuse(why, "chunk that overruns the file");
        }
        const size_t pay = c.i;
        c.i += (size_t)len + 4;
        if (!have_ihdr) {
            if (type != tag('I', 'H', 'D', 'R') || len != 13) return refuse(why, "file whose first chunk is not IHDR");
            Cursor s(file + pay, 13 + 4);
            const uint32_t w = s.u32(), h = s.u32();
            const unsigned depth = s.u8(), ctype = s.u8(), comp = s.u8(), filt = s.u8(), lace = s.u8();
            if (s.u32() != crc32(file + pay - 4, 17)) return refuse(why, "IHDR with a wrong CRC");
            const bool all = (flags & kAcceptAll) != 0;
            if (!all && depth != 8) return refuse(why, "bit depth other than 8");
            if (ctype != 0 && ctype != 2 && ctype != 3 && ctype != 4 && ctype != 6) return refuse(why, "unknown colour type");
            if (all) {
                if (depth != 1 && depth != 2 && depth != 4 && depth != 8 && depth != 16) return refuse(why, "bit depth that is none of 1, 2, 4, 8 and 16");
                if (depth == 16 && ctype == 0) return refuse(why, "16-bit grey: the host codecs disagree on its conversion");
                if (depth == 16 && ctype == 3) return refuse(why, "16-bit palette image: no such form");
                if (depth < 8 && ctype != 0 && ctype != 3) return refuse(why, "bit depth below 8 in a colour type that has none");
            }
            if (comp != 0 || filt != 0) return refuse(why, "unknown compression or filter method");
            if (all ? lace > 1 : lace != 0) return refuse(why, all ? "unknown interlace method" : "Adam7 interlacing");
            if (w < 1 || h < 1 || w > 8192 || h > 8192) return refuse(why, "size outside 1..8192");
            f.h = (int)h; f.w = (int)w; f.ctype = (int)ctype; f.depth = (int)depth; f.interlace = (int)lace;
            f.bpp = (int)pngdec::filter_unit(ctype, depth);
            have_ihdr = true;
            continue;
        }
        if (type == tag('I', 'H', 'D', 'R')) return refuse(why, "file with two IHDR chunks");
        if (type == tag('I', 'D', 'A', 'T')) {
            if (idat_closed) return refuse(why, "IDAT chunks that are not consecutive");
            if (!idat_open && f.ctype == 3 && !have_plte) return refuse(why, "palette image without PLTE");
            idat_open = true;
            if (len) { f.spans.push_back(Span{pay, len}); f.idat_bytes += len; }
            continue;
        }
        if (idat_open) { idat_open = false; idat_closed = true; }
        if (type == tag('I', 'E', 'N', 'D')) break;
        if (idat_closed) continue;                               // behind the data only another IDAT matters
        // in front of the data Pillow checks every chunk's CRC, the ancillary ones' too
        if (type != tag('P', 'L', 'T', 'E')) {
            Cursor s(file + pay + len, 4);
            if (s.u32() != crc32(file + pay - 4, (size_t)len + 4)) return refuse(why, "chunk with a wrong CRC in front of the image data");
        }
        if (type == tag('P', 'L', 'T', 'E')) {
            if (have_plte) return refuse(why, "file with two PLTE chunks");
            if (len == 0 || len % 3 || len > 768) return refuse(why, "PLTE of a wrong length");
            Cursor s(file + pay + len, 4);
            if (s.u32() != crc32(file + pay - 4, (size_t)len + 4)) return refuse(why, "PLTE with a wrong CRC");
            std::memcpy(f.pal, file + pay, len);
            f.npal = len / 3;
            have_plte = true;
        } else if (type == tag('a', 'c', 'T', 'L')) return refuse(why, "animation (APNG)");
        else if (type == tag('i', 'C', 'C', 'P')) f.iccp = true;
        else if (type == tag('e', 'X', 'I', 'f') && !have_exif) { have_exif = true; f.orientation = jpegparse::tiff_orientation(file + pay, len); }      // (the first one, as the JPEG walk takes the first Exif block)
        // tRNS and every other chunk: skipped
    }
    if (!have_ihdr) return refuse(why, "file whose first chunk is not IHDR");
    if (f.spans.empty()) return refuse(why, "file without image data (no IDAT)");
    if (f.iccp && (flags & kRefuseIccp)) return refuse(why, "with an iCCP profile: its conversion is not offered on the device");
    // the zlib header: the stream's first two bytes, wherever the chunks cut it
    unsigned hb[2] = {0, 0};
    size_t got = 0;
    for (const Span& s : f.spans)
        for (size_t k = 0; k < s.len && got < 2; ++k) hb[got++] = file[s.off + k];
    if (got < 2 || (hb[0] & 15u) != 8 || (hb[0] >> 4) > 7 || ((hb[0] << 8 | hb[1]) % 31u) != 0 || (hb[1] & 0x20u))
        return refuse(why, "data that is no deflate stream with a window of at most 32 KiB and no preset dictionary");
    return true;
}

// the IDAT payloads back to back into dst (room >= f.idat_bytes): one contiguous zlib stream.  -> bytes written; 0 and a reason when
// the file is not the one that was planned
inline size_t stage(const File& f, const uint8_t* file, size_t bytes, uint8_t* dst, size_t room, std::string& why) {
    if (f.idat_bytes > room) { refuse(why, "internal staging overflow"); return 0; }
    size_t o = 0;
    for (const Span& s : f.spans) {
        if (s.off > bytes || s.len > bytes - s.off) { refuse(why, "file that changed since it was planned"); return 0; }
        std::memcpy(dst + o, file + s.off, s.len);
        o += s.len;
    }
    return o;
}

}  // namespace pngparse
}  // namespace ire
