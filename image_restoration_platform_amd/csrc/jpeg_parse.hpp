// jpeg_parse.hpp -- the host side of the device's JPEG decoder: reads a file's markers, tables and frame, decides whether the device
// decodes it, splits the entropy-coded data at the restart markers into independent streams (byte stuffing removed on the way) and
// builds the decode tables.  Host-only, header-only, plain C++17, no HIP: libire.so uses it in front of jpeg_dec.hip,
// tests/native/jpeg_dec_sim.cpp compiles it alone under ASan and UBSan.  No read goes past `bytes`, whatever the file says: every
// access goes through Cursor or is checked against the end beside it.
//
// Accepted: SOF0 / SOF1 (Huffman), 8-bit samples, ONE interleaved scan (Ss 0, Se 63, Ah = Al = 0), 8-bit quantiser tables, up to
// 4 + 4 Huffman tables of any content, with or without DRI, fill bytes before markers, 1..8192 per side; three components that
// libjpeg reads as Y Cb Cr (a JFIF marker, or ids 1 2 3; no Adobe marker) with luma 1x1, 2x1 or 2x2 and chroma 1x1 (width >= 5 when
// subsampled: below that libjpeg's fancy upsampler switches to replication), or one grey component.  Everything else is refused
// with a reason; the caller then uses the host codec.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "jpeg_dec_core.hpp"

namespace ire {
namespace jpegparse {

using jpegdec::DecImage;
using jpegdec::DecStream;
using jpegdec::DecTable;

struct Header {
    DecImage im{};                  // geometry, sampling, table numbers, quantisers (the stream fields are the caller's)
    DecTable tabs[8]{};             // 0..3: DC tables, 4..7: AC tables
    uint32_t restart = 0;           // MCUs per restart interval, 0: none
    size_t scan_off = 0;            // the first entropy-coded byte
    uint32_t nstreams = 0;          // streams the scan must have
};

// ---- a bounds-checked reader ---------------------------------------------------------------------------------------------------
struct Cursor {
    const uint8_t* p;
    size_t n, i = 0;
    bool ok = true;
    Cursor(const uint8_t* p_, size_t n_) : p(p_), n(n_) {}
    size_t left() const { return n - i; }
    unsigned u8() { if (i >= n) { ok = false; return 0; } return p[i++]; }
    unsigned u16() { const unsigned a = u8(), b = u8(); return a << 8 | b; }
};

// jdhuff.c's jpeg_make_d_derived_tbl: counts[l - 1] codes of length l, their symbols in order.  false: the counts are no prefix code.
inline bool build_table(const uint8_t counts[16], const uint8_t* vals, int nvals, DecTable& t) {
    std::memset(&t, 0, sizeof(t));
    for (int l = 0; l < 18; ++l) t.maxcode[l] = -1;
    std::memcpy(t.vals, vals, (size_t)nvals);
    uint32_t code = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
        const int cnt = counts[l - 1];
        if (code + (uint32_t)cnt > (1u << l)) return false;
        if (cnt) {
            t.valoff[l] = k - (int32_t)code;
            for (int j = 0; j < cnt; ++j, ++k, ++code)
                if (l <= 9)
                    for (uint32_t f = 0; f < (1u << (9 - l)); ++f) t.look[(code << (9 - l)) | f] = (uint16_t)(l << 8 | vals[k]);
            t.maxcode[l] = (int32_t)code - 1;
        }
        code <<= 1;
    }
    return true;
}

inline bool refuse(std::string& why, const char* reason) { why = std::string("invalid: ") + reason; return false; }

// The markers up to and including SOS.  true: `hd` describes a file the device decodes, so far as its head says.
inline bool parse_header(const uint8_t* file, size_t bytes, Header& hd, std::string& why) {
    if (!file || bytes < 4 || file[0] != 0xFF || file[1] != 0xD8) return refuse(why, "not a JPEG file (no SOI)");
    if (bytes >= ((size_t)1 << 28)) return refuse(why, "JPEG file of 256 MB or more");
    Cursor c(file, bytes);
    c.i = 2;
    bool have_q[4] = {}, have_h[8] = {}, jfif = false, adobe = false, have_sof = false;
    uint16_t qt[4][64];
    unsigned cid[4] = {}, ctq[4] = {};
    for (;;) {
        unsigned b = c.u8();
        if (!c.ok) return refuse(why, "truncated JPEG header");
        if (b != 0xFF) return refuse(why, "corrupt JPEG header (no marker where one must be)");
        do b = c.u8(); while (c.ok && b == 0xFF);                // fill bytes
        if (!c.ok) return refuse(why, "truncated JPEG header");
        if (b == 0xD8 || (b >= 0xD0 && b <= 0xD7) || b == 0x01 || b == 0x00) return refuse(why, "corrupt JPEG header (stray marker)");
        if (b == 0xD9) return refuse(why, "JPEG file without a scan");
        const size_t seg0 = c.i;
        const unsigned len = c.u16();
        if (!c.ok || len < 2 || seg0 + len > bytes) return refuse(why, "truncated JPEG header");
        Cursor s(file + seg0 + 2, len - 2);                      // the segment's payload: nothing below reads outside it
        c.i = seg0 + len;
        if (b == 0xC2) return refuse(why, "progressive JPEG (SOF2): not decoded on the device");
        if (b == 0xC9 || b == 0xCA || b == 0xCB || b == 0xCD || b == 0xCE || b == 0xCF || b == 0xCC) return refuse(why, "arithmetic-coded JPEG");
        if (b == 0xC3 || b == 0xC5 || b == 0xC6 || b == 0xC7) return refuse(why, "lossless or hierarchical JPEG");
        if (b == 0xDC) return refuse(why, "JPEG with a DNL marker");
        if (b == 0xC0 || b == 0xC1) {
            if (have_sof) return refuse(why, "JPEG with two frames");
            const unsigned prec = s.u8(), h = s.u16(), w = s.u16(), nc = s.u8();
            if (!s.ok) return refuse(why, "truncated JPEG header");
            if (prec != 8) return refuse(why, "JPEG with 12-bit samples");
            if (h == 0) return refuse(why, "JPEG with a DNL marker");
            if (h > 8192 || w < 1 || w > 8192) return refuse(why, "JPEG size outside 1..8192");
            if (nc == 4) return refuse(why, "JPEG with 4 components (CMYK / YCCK)");
            if (nc != 1 && nc != 3) return refuse(why, "JPEG with an unsupported number of components");
            unsigned hs[4] = {}, vs[4] = {};
            for (unsigned k = 0; k < nc; ++k) { cid[k] = s.u8(); const unsigned hv = s.u8(); hs[k] = hv >> 4; vs[k] = hv & 15u; ctq[k] = s.u8(); }
            if (!s.ok) return refuse(why, "truncated JPEG header");
            for (unsigned k = 0; k < nc; ++k) if (ctq[k] > 3) return refuse(why, "corrupt JPEG header (quantiser table number)");
            DecImage& im = hd.im;
            im.h = (int)h; im.w = (int)w; im.ncomp = (int)nc;
            if (nc == 1) {
                if (hs[0] != 1 || vs[0] != 1) return refuse(why, "unsupported sampling factors");
                im.sampling = 3;
            } else {
                if (hs[1] != 1 || vs[1] != 1 || hs[2] != 1 || vs[2] != 1) return refuse(why, "unsupported sampling factors");
                if (hs[0] == 1 && vs[0] == 1) im.sampling = 0;
                else if (hs[0] == 2 && vs[0] == 1) im.sampling = 1;
                else if (hs[0] == 2 && vs[0] == 2) im.sampling = 2;
                else return refuse(why, "unsupported sampling factors");
                if (im.sampling && w < 5) return refuse(why, "subsampled chroma needs a width of at least 5");
            }
            const uint32_t hmax = hs[0], vmax = vs[0];
            im.mcus_w = (w + 8 * hmax - 1) / (8 * hmax); im.mcus_h = (h + 8 * vmax - 1) / (8 * vmax);
            im.bpm = 0;
            uint32_t off = 0;
            for (unsigned k = 0; k < nc; ++k) {
                im.hs[k] = (uint8_t)hs[k]; im.vs[k] = (uint8_t)vs[k];
                im.gridw[k] = im.mcus_w * hs[k]; im.gridh[k] = im.mcus_h * vs[k];
                im.coef_off[k] = off; off += im.gridw[k] * im.gridh[k];
                im.pw[k] = (w * hs[k] + hmax - 1) / hmax; im.ph[k] = (h * vs[k] + vmax - 1) / vmax;
                for (unsigned y = 0; y < vs[k]; ++y)
                    for (unsigned x = 0; x < hs[k]; ++x) { im.comp_of[im.bpm] = (uint8_t)k; im.bx[im.bpm] = (uint8_t)x; im.by[im.bpm] = (uint8_t)y; ++im.bpm; }
            }
            im.nblocks = im.mcus_w * im.mcus_h * im.bpm;
            have_sof = true;
        } else if (b == 0xDB) {
            while (s.left()) {
                const unsigned pt = s.u8();
                if ((pt >> 4) != 0) return refuse(why, "JPEG with 16-bit quantiser tables");
                if ((pt & 15u) > 3 || s.left() < 64) return refuse(why, "corrupt JPEG header (DQT)");
                for (int k = 0; k < 64; ++k) qt[pt & 15u][jpegdec::natural_of((uint32_t)k)] = (uint16_t)s.u8();
                have_q[pt & 15u] = true;
            }
        } else if (b == 0xC4) {
            while (s.left()) {
                const unsigned tc = s.u8();
                uint8_t counts[16];
                if ((tc >> 4) > 1 || (tc & 15u) > 3 || s.left() < 16) return refuse(why, "corrupt JPEG header (DHT)");
                unsigned total = 0;
                for (int k = 0; k < 16; ++k) { counts[k] = (uint8_t)s.u8(); total += counts[k]; }
                if (total > 256 || total > s.left()) return refuse(why, "corrupt JPEG header (DHT counts overrun the segment)");
                const unsigned slot = (tc >> 4) * 4 + (tc & 15u);
                if (!build_table(counts, s.p + s.i, (int)total, hd.tabs[slot])) return refuse(why, "corrupt JPEG header (DHT is no prefix code)");
                s.i += total;
                have_h[slot] = true;
            }
        } else if (b == 0xDD) {
            if (s.left() < 2) return refuse(why, "truncated JPEG header");
            hd.restart = s.u16();
        } else if (b == 0xE0) {
            if (s.left() >= 5 && !std::memcmp(s.p, "JFIF\0", 5)) jfif = true;
        } else if (b == 0xEE) {
            if (s.left() >= 5 && !std::memcmp(s.p, "Adobe", 5)) adobe = true;
        } else if (b == 0xDA) {
            if (!have_sof) return refuse(why, "corrupt JPEG header (SOS before SOF)");
            DecImage& im = hd.im;
            const unsigned ns = s.u8();
            if (!s.ok) return refuse(why, "truncated JPEG header");
            if ((int)ns != im.ncomp) return refuse(why, "multi-scan JPEG");
            for (unsigned k = 0; k < ns; ++k) {
                const unsigned id = s.u8(), tt = s.u8();
                if (!s.ok) return refuse(why, "truncated JPEG header");
                if (id != cid[k]) return refuse(why, "multi-scan JPEG (components out of frame order)");
                if ((tt >> 4) > 3 || (tt & 15u) > 3) return refuse(why, "corrupt JPEG header (Huffman table number)");
                if (!have_h[tt >> 4] || !have_h[4 + (tt & 15u)]) return refuse(why, "corrupt JPEG header (scan names a missing Huffman table)");
                if (!have_q[ctq[k]]) return refuse(why, "corrupt JPEG header (frame names a missing quantiser table)");
                im.dc_tab[k] = (uint8_t)(tt >> 4); im.ac_tab[k] = (uint8_t)(tt & 15u);
                std::memcpy(im.quant[k], qt[ctq[k]], sizeof(im.quant[k]));
            }
            const unsigned ss = s.u8(), se = s.u8(), ahl = s.u8();
            if (!s.ok) return refuse(why, "truncated JPEG header");
            if (ss != 0 || se != 63 || ahl != 0) return refuse(why, "progressive JPEG scan parameters");
            if (im.ncomp == 3) {
                if (adobe) return refuse(why, "JPEG with an Adobe marker (RGB / YCCK colour)");
                if (!jfif && !(cid[0] == 1 && cid[1] == 2 && cid[2] == 3)) return refuse(why, "JPEG whose colour space is not Y Cb Cr");
            }
            hd.scan_off = c.i;
            const uint32_t nmcu = im.mcus_w * im.mcus_h;
            hd.nstreams = hd.restart ? (nmcu + hd.restart - 1) / hd.restart : 1;
            return true;
        }
        // every other segment (APPn, COM, ...) is skipped
    }
}

// bytes the streams of this file need at most in the staging area (each stream starts on a multiple of 4)
inline size_t scan_room(const Header& hd, size_t bytes) { return bytes - hd.scan_off + 4 * (size_t)hd.nstreams + 8; }

// The scan: cut at RSTn, `FF 00` -> `FF`, each stream's bytes to dst + its off (dst == null: only check).  `room` bytes at dst.
// true: exactly hd.nstreams streams, their markers numbered 0..7 in order, EOI behind the last.
inline bool split_scan(const Header& hd, const uint8_t* file, size_t bytes, uint8_t* dst, size_t room, DecStream* streams, std::string& why) {
    const uint32_t nmcu = hd.im.mcus_w * hd.im.mcus_h;
    const uint8_t *p = file + hd.scan_off, *end = file + bytes;
    size_t o = 0;
    uint32_t ns = 0, len = 0;
    auto begin = [&]() {
        o = (o + 3) & ~(size_t)3;
        len = 0;
    };
    auto finish = [&]() {
        if (streams) {
            const uint32_t m0 = hd.restart ? ns * hd.restart : 0;
            streams[ns] = DecStream{(uint32_t)o, len, m0, hd.restart && nmcu - m0 > hd.restart ? hd.restart : nmcu - m0};
        }
        o += len; ++ns;
    };
    begin();
    for (;;) {
        const uint8_t* q = p < end ? static_cast<const uint8_t*>(std::memchr(p, 0xFF, (size_t)(end - p))) : nullptr;
        const size_t run = (size_t)((q ? q : end) - p);
        if (dst && run) { if (o + len + run > room) return refuse(why, "internal staging overflow"); std::memcpy(dst + o + len, p, run); }
        len += (uint32_t)run;
        if (!q || q + 1 >= end) return refuse(why, "truncated JPEG scan (no EOI)");
        const unsigned m = q[1];
        if (m == 0x00) {
            if (dst) { if (o + len + 1 > room) return refuse(why, "internal staging overflow"); dst[o + len] = 0xFF; }
            ++len; p = q + 2;
        } else if (m == 0xFF) p = q + 1;                                   // a fill byte
        else if (m >= 0xD0 && m <= 0xD7) {
            if (!hd.restart || ns + 1 >= hd.nstreams || m != 0xD0u + (ns & 7u)) return refuse(why, "corrupt JPEG data (restart markers out of order)");
            finish(); begin();
            p = q + 2;
        } else if (m == 0xD9) {
            if (ns + 1 != hd.nstreams) return refuse(why, "corrupt JPEG data (restart markers missing)");
            finish();
            return true;
        } else if (m == 0xDC) return refuse(why, "JPEG with a DNL marker");
        else return refuse(why, "multi-scan JPEG (a marker follows the first scan)");
    }
}

// the whole decision for one file: its head and a dry run over its scan
inline bool plan(const uint8_t* file, size_t bytes, Header& hd, std::string& why) {
    return parse_header(file, bytes, hd, why) && split_scan(hd, file, bytes, nullptr, 0, nullptr, why);
}

}  // namespace jpegparse
}  // namespace ire
