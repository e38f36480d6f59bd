// jpeg_parse.hpp -- the host side of the device's JPEG decoder: reads a file's markers, tables and frame, decides whether the device
// decodes it, splits the entropy-coded data at the restart markers into independent streams (byte stuffing removed on the way) and
// builds the decode tables.  Host-only, header-only, plain C++17, no HIP: libire.so uses it in front of jpeg_dec.hip,
// tests/native/jpeg_dec_sim.cpp compiles it alone under ASan and UBSan.  No read goes past `bytes`, whatever the file says: every
// access goes through Cursor or is checked against the end beside it.
//
// Accepted by parse_header / plan: SOF0 / SOF1 (Huffman), 8-bit samples, ONE interleaved scan (Ss 0, Se 63, Ah = Al = 0), 8-bit quantiser tables, up to
// 4 + 4 Huffman tables of any content, with or without DRI, fill bytes before markers, 1..8192 per side; three components that
// libjpeg reads as Y Cb Cr (a JFIF marker, or ids 1 2 3; no Adobe marker) with luma 1x1, 2x1 or 2x2 and chroma 1x1 (width >= 5 when
// subsampled: below that libjpeg's fancy upsampler switches to replication), or one grey component.  Everything else is refused
// with a reason; the caller then uses the host codec.  head_file / plan_file accept progressive files (SOF2) beside these when asked
// to: see there.  exif_orientation / file_orientation read an upload's EXIF orientation (upload jobs); a broken block is orientation 1, never a refusal.
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

// the frame header's payload -> the image's geometry; the components' ids and quantiser table numbers
inline bool read_frame(Cursor& s, DecImage& im, unsigned cid[4], unsigned ctq[4], std::string& why) {
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
    return true;
}
// a DQT segment's payload -> qt (natural order), have_q
inline bool read_dqt(Cursor& s, uint16_t qt[4][64], bool have_q[4], std::string& why) {
    while (s.left()) {
        const unsigned pt = s.u8();
        if ((pt >> 4) != 0) return refuse(why, "JPEG with 16-bit quantiser tables");
        if ((pt & 15u) > 3 || s.left() < 64) return refuse(why, "corrupt JPEG header (DQT)");
        for (int k = 0; k < 64; ++k) qt[pt & 15u][jpegdec::natural_of((uint32_t)k)] = (uint16_t)s.u8();
        have_q[pt & 15u] = true;
    }
    return true;
}
// the next table of a DHT segment's payload -> t and its slot (0..3: DC, 4..7: AC)
inline bool read_dht(Cursor& s, DecTable& t, unsigned& slot, std::string& why) {
    const unsigned tc = s.u8();
    uint8_t counts[16];
    if ((tc >> 4) > 1 || (tc & 15u) > 3 || s.left() < 16) return refuse(why, "corrupt JPEG header (DHT)");
    unsigned total = 0;
    for (int k = 0; k < 16; ++k) { counts[k] = (uint8_t)s.u8(); total += counts[k]; }
    if (total > 256 || total > s.left()) return refuse(why, "corrupt JPEG header (DHT counts overrun the segment)");
    slot = (tc >> 4) * 4 + (tc & 15u);
    if (!build_table(counts, s.p + s.i, (int)total, t)) return refuse(why, "corrupt JPEG header (DHT is no prefix code)");
    s.i += total;
    return true;
}

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
            if (!read_frame(s, hd.im, cid, ctq, why)) return false;
            have_sof = true;
        } else if (b == 0xDB) {
            if (!read_dqt(s, qt, have_q, why)) return false;
        } else if (b == 0xC4) {
            while (s.left()) {
                DecTable t;
                unsigned slot;
                if (!read_dht(s, t, slot, why)) return false;
                hd.tabs[slot] = t;
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

// One scan's data from file + off: cut at RSTn, `FF 00` -> `FF`, each stream's bytes to dst + its off (dst == null: only check); o: where
// the next stream goes in dst (`room` bytes), carried from scan to scan.  nmcu: the scan's MCUs.  true: exactly nstreams streams, their
// markers numbered 0..7 in order, and behind the last EOI -- or, with `end` (a progressive file), any marker, whose place goes to *end.
inline bool split_data(const uint8_t* file, size_t bytes, size_t off, uint32_t restart, uint32_t nstreams, uint32_t nmcu, uint8_t* dst, size_t room, size_t& o,
                       DecStream* streams, std::string& why, size_t* end_off) {
    const uint8_t *p = file + off, *end = file + bytes;
    uint32_t ns = 0, len = 0;
    auto begin = [&]() {
        o = (o + 3) & ~(size_t)3;
        len = 0;
    };
    auto finish = [&]() {
        if (streams) {
            const uint32_t m0 = restart ? ns * restart : 0;
            streams[ns] = DecStream{(uint32_t)o, len, m0, restart && nmcu - m0 > restart ? restart : nmcu - m0};
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
            if (!restart || ns + 1 >= nstreams || m != 0xD0u + (ns & 7u)) return refuse(why, "corrupt JPEG data (restart markers out of order)");
            finish(); begin();
            p = q + 2;
        } else if (m == 0xDC) return refuse(why, "JPEG with a DNL marker");
        else if (m == 0xD9 || end_off) {
            if (ns + 1 != nstreams) return refuse(why, "corrupt JPEG data (restart markers missing)");
            finish();
            if (end_off) *end_off = (size_t)(q - file);
            return true;
        } else return refuse(why, "multi-scan JPEG (a marker follows the first scan)");
    }
}
// the one scan of a baseline file
inline bool split_scan(const Header& hd, const uint8_t* file, size_t bytes, uint8_t* dst, size_t room, DecStream* streams, std::string& why) {
    size_t o = 0;
    return split_data(file, bytes, hd.scan_off, hd.restart, hd.nstreams, hd.im.mcus_w * hd.im.mcus_h, dst, room, o, streams, why, nullptr);
}

// the whole decision for one file: its head and a dry run over its scan
inline bool plan(const uint8_t* file, size_t bytes, Header& hd, std::string& why) {
    return parse_header(file, bytes, hd, why) && split_scan(hd, file, bytes, nullptr, 0, nullptr, why);
}

// ---- a whole file, baseline or progressive ---------------------------------------------------------------------------------------------
// Progressive (SOF2, Huffman-coded, 8-bit; the frame rules above unchanged): every scan script that T.81 Annex G allows and that is
// COMPLETE -- DC scans (Ss = Se = 0), interleaved or not; AC scans of one component, 1 <= Ss <= Se <= 63; a first scan of a coefficient
// has Ah = 0, a refinement Ah = the Al its last scan left and Al = Ah - 1; no AC scan of a component before its first DC scan; every
// coefficient of every component ends at Al = 0 (else libjpeg smooths the blocks, and nothing here does).  DHT and DRI between the
// scans; no DQT behind the first SOS; kMaxScans scans at most.
constexpr uint32_t kAcceptProgressive = 1u;            // ire.h: IRE_DECODE_ACCEPT_PROGRESSIVE
constexpr uint32_t kMaxScans = 64;                     // ire.h: IRE_DECODE_MAX_SCANS

struct Scan {
    DecImage im{};                  // the frame's record with this scan's MCU, table numbers, kind, band and bit position
    uint16_t tab[8] = {};           // per Huffman slot: its table in the file's pool when this scan began
    uint32_t restart = 0, nstreams = 0, nmcu = 0;       // in the scan's OWN MCUs: one block where it has one component
    uint32_t level = 0;             // 1 + the highest level of an earlier scan that names one of its components and overlaps its band
    size_t data_off = 0, data_end = 0;
};
struct File {
    Header hd;                      // the frame; of a baseline file all of it
    bool progressive = false;
    std::vector<Scan> scans;        // a baseline file: none
    std::vector<DecTable> pool;     // every Huffman table the file defines, in file order (slots are redefined between scans)
    uint32_t nstreams = 0, nlevels = 1;                 // over all scans
    size_t data_bytes = 0;          // the scans' entropy-coded bytes, stuffing and restart markers included
    uint32_t nscans() const { return progressive ? (uint32_t)scans.size() : 1u; }
};

// is the file's frame (the first SOFn in front of any SOS) progressive?  Reads markers only; every doubt is "no".
inline bool frame_is_progressive(const uint8_t* file, size_t bytes) {
    if (!file || bytes < 4 || file[0] != 0xFF || file[1] != 0xD8) return false;
    size_t i = 2;
    while (i + 4 <= bytes) {
        if (file[i] != 0xFF) return false;
        while (i < bytes && file[i] == 0xFF) ++i;
        if (i + 2 >= bytes) return false;
        const unsigned b = file[i++];
        if (b == 0xC2) return true;
        if (b == 0xDA || b == 0xD9 || b == 0xD8 || b == 0x00 || b == 0x01 || (b >= 0xD0 && b <= 0xD7) || (b >= 0xC0 && b <= 0xCF && b != 0xC4 && b != 0xC8)) return false;
        const size_t len = (size_t)file[i] << 8 | file[i + 1];
        if (len < 2) return false;
        i += len;
    }
    return false;
}

inline bool parse_progressive(const uint8_t* file, size_t bytes, File& f, std::string& why) {
    if (bytes >= ((size_t)1 << 28)) return refuse(why, "JPEG file of 256 MB or more");
    Cursor c(file, bytes);
    c.i = 2;
    bool have_q[4] = {}, jfif = false, adobe = false, have_sof = false;
    int slot_tab[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
    uint16_t qt[4][64];
    unsigned cid[4] = {}, ctq[4] = {};
    int coef_bits[4][64];
    uint32_t coef_level[4][64] = {};
    for (auto& cb : coef_bits) for (int& v : cb) v = -1;
    uint32_t restart = 0;
    Header& hd = f.hd;
    f.progressive = true;
    f.scans.clear(); f.pool.clear();
    f.nstreams = 0; f.nlevels = 1; f.data_bytes = 0;
    for (;;) {
        unsigned b = c.u8();
        if (!c.ok) return refuse(why, f.scans.empty() ? "truncated JPEG header" : "truncated JPEG scan (no EOI)");
        if (b != 0xFF) return refuse(why, "corrupt JPEG header (no marker where one must be)");
        do b = c.u8(); while (c.ok && b == 0xFF);                // fill bytes
        if (!c.ok) return refuse(why, f.scans.empty() ? "truncated JPEG header" : "truncated JPEG scan (no EOI)");
        if (b == 0xD8 || (b >= 0xD0 && b <= 0xD7) || b == 0x01 || b == 0x00) return refuse(why, "corrupt JPEG header (stray marker)");
        if (b == 0xD9) {
            if (f.scans.empty()) return refuse(why, "JPEG file without a scan");
            for (int k = 0; k < hd.im.ncomp; ++k)
                for (int z = 0; z < 64; ++z)
                    if (coef_bits[k][z] != 0) return refuse(why, "progressive JPEG with an incomplete scan script (it would be smoothed)");
            return true;
        }
        const size_t seg0 = c.i;
        const unsigned len = c.u16();
        if (!c.ok || len < 2 || seg0 + len > bytes) return refuse(why, "truncated JPEG header");
        Cursor s(file + seg0 + 2, len - 2);                      // the segment's payload: nothing below reads outside it
        c.i = seg0 + len;
        if (b == 0xC9 || b == 0xCA || b == 0xCB || b == 0xCD || b == 0xCE || b == 0xCF || b == 0xCC) return refuse(why, "arithmetic-coded JPEG");
        if (b == 0xC3 || b == 0xC5 || b == 0xC6 || b == 0xC7) return refuse(why, "lossless or hierarchical JPEG");
        if (b == 0xDC) return refuse(why, "JPEG with a DNL marker");
        if (b == 0xC0 || b == 0xC1 || b == 0xC2) {
            if (have_sof || b != 0xC2) return refuse(why, "JPEG with two frames");
            if (!read_frame(s, hd.im, cid, ctq, why)) return false;
            have_sof = true;
        } else if (b == 0xDB) {
            if (!f.scans.empty()) return refuse(why, "progressive JPEG with a DQT behind the first scan");
            if (!read_dqt(s, qt, have_q, why)) return false;
        } else if (b == 0xC4) {
            while (s.left()) {
                DecTable t;
                unsigned slot;
                if (!read_dht(s, t, slot, why)) return false;
                if (f.pool.size() >= 8 * (size_t)kMaxScans + 8) return refuse(why, "progressive JPEG with too many Huffman tables");
                slot_tab[slot] = (int)f.pool.size();
                f.pool.push_back(t);
            }
        } else if (b == 0xDD) {
            if (s.left() < 2) return refuse(why, "truncated JPEG header");
            restart = s.u16();
        } else if (b == 0xE0) {
            if (s.left() >= 5 && !std::memcmp(s.p, "JFIF\0", 5)) jfif = true;
        } else if (b == 0xEE) {
            if (s.left() >= 5 && !std::memcmp(s.p, "Adobe", 5)) adobe = true;
        } else if (b == 0xDA) {
            if (!have_sof) return refuse(why, "corrupt JPEG header (SOS before SOF)");
            if (f.scans.size() >= kMaxScans) return refuse(why, "progressive JPEG with more than 64 scans");
            DecImage& fr = hd.im;
            if (f.scans.empty()) {
                if (fr.ncomp == 3) {
                    if (adobe) return refuse(why, "JPEG with an Adobe marker (RGB / YCCK colour)");
                    if (!jfif && !(cid[0] == 1 && cid[1] == 2 && cid[2] == 3)) return refuse(why, "JPEG whose colour space is not Y Cb Cr");
                }
                for (int k = 0; k < fr.ncomp; ++k) {
                    if (!have_q[ctq[k]]) return refuse(why, "corrupt JPEG header (frame names a missing quantiser table)");
                    std::memcpy(fr.quant[k], qt[ctq[k]], sizeof(fr.quant[k]));
                }
            }
            const unsigned ns = s.u8();
            if (!s.ok) return refuse(why, "truncated JPEG header");
            if (ns < 1 || (int)ns > fr.ncomp) return refuse(why, "progressive JPEG scan with a wrong number of components");
            unsigned comp[4] = {}, tdc[4] = {}, tac[4] = {};
            for (unsigned k = 0; k < ns; ++k) {
                const unsigned id = s.u8(), tt = s.u8();
                if (!s.ok) return refuse(why, "truncated JPEG header");
                unsigned ci = 0;
                while (ci < (unsigned)fr.ncomp && cid[ci] != id) ++ci;
                if (ci == (unsigned)fr.ncomp || (k && ci <= comp[k - 1])) return refuse(why, "progressive JPEG scan (components unknown or out of frame order)");
                if ((tt >> 4) > 3 || (tt & 15u) > 3) return refuse(why, "corrupt JPEG header (Huffman table number)");
                comp[k] = ci; tdc[k] = tt >> 4; tac[k] = tt & 15u;
            }
            const unsigned ss = s.u8(), se = s.u8(), ahl = s.u8(), ah = ahl >> 4, al = ahl & 15u;
            if (!s.ok) return refuse(why, "truncated JPEG header");
            if (ss == 0 ? se != 0 : (se < ss || se > 63)) return refuse(why, "progressive JPEG scan with a wrong band (Ss, Se)");
            if (ss != 0 && ns != 1) return refuse(why, "progressive JPEG with an AC scan of more than one component");
            if (al > 13 || (ah != 0 && al + 1 != ah)) return refuse(why, "progressive JPEG scan with a wrong bit position (Ah, Al)");
            Scan sc;
            sc.im = fr;
            DecImage& im = sc.im;
            im.kind = (uint8_t)(ss == 0 ? (ah ? jpegdec::kScanDcRefine : jpegdec::kScanDcFirst) : (ah ? jpegdec::kScanAcRefine : jpegdec::kScanAcFirst));
            im.ss = (uint8_t)ss; im.se = (uint8_t)se; im.al = (uint8_t)al;
            for (unsigned k = 0; k < ns; ++k) {
                const unsigned ci = comp[k];
                if (ss != 0 && coef_bits[ci][0] < 0) return refuse(why, "progressive JPEG with an AC scan before the component's DC scan");
                for (unsigned z = ss; z <= se; ++z) {
                    const int prev = coef_bits[ci][z];
                    if (prev < 0 ? ah != 0 : (ah == 0 || (unsigned)prev != ah))
                        return refuse(why, "progressive JPEG scan whose Ah is not the Al of the coefficient's last scan");
                    coef_bits[ci][z] = (int)al;
                    if (coef_level[ci][z] + (prev < 0 ? 0u : 1u) > sc.level) sc.level = coef_level[ci][z] + (prev < 0 ? 0u : 1u);
                }
                if (im.kind == jpegdec::kScanDcFirst && slot_tab[tdc[k]] < 0) return refuse(why, "corrupt JPEG header (scan names a missing Huffman table)");
                if (ss != 0 && slot_tab[4 + tac[k]] < 0) return refuse(why, "corrupt JPEG header (scan names a missing Huffman table)");
                im.dc_tab[ci] = (uint8_t)tdc[k]; im.ac_tab[ci] = (uint8_t)tac[k];
            }
            for (unsigned k = 0; k < ns; ++k)
                for (unsigned z = ss; z <= se; ++z) coef_level[comp[k]][z] = sc.level;
            for (int k = 0; k < 8; ++k) sc.tab[k] = (uint16_t)(slot_tab[k] < 0 ? 0 : slot_tab[k]);
            if (ns == 1) {                                       // not interleaved: the blocks of the component's real plane, row by row
                const unsigned ci = comp[0];
                im.raster = 1; im.bpm = 1; im.comp_of[0] = (uint8_t)ci; im.bx[0] = im.by[0] = 0;
                im.rw = (im.pw[ci] + 7) / 8; im.rh = (im.ph[ci] + 7) / 8;
                sc.nmcu = im.rw * im.rh;
            } else {                                             // interleaved: the frame's MCU grid, the scan's components in it
                im.bpm = 0;
                for (unsigned k = 0; k < ns; ++k)
                    for (unsigned y = 0; y < im.vs[comp[k]]; ++y)
                        for (unsigned x = 0; x < im.hs[comp[k]]; ++x) { im.comp_of[im.bpm] = (uint8_t)comp[k]; im.bx[im.bpm] = (uint8_t)x; im.by[im.bpm] = (uint8_t)y; ++im.bpm; }
                sc.nmcu = im.mcus_w * im.mcus_h;
            }
            im.nblocks = sc.nmcu * im.bpm;
            sc.restart = restart;
            sc.nstreams = restart ? (sc.nmcu + restart - 1) / restart : 1;
            sc.data_off = c.i;
            size_t o = 0;
            if (!split_data(file, bytes, sc.data_off, sc.restart, sc.nstreams, sc.nmcu, nullptr, 0, o, nullptr, why, &sc.data_end)) return false;
            c.i = sc.data_end;
            f.nstreams += sc.nstreams;
            f.data_bytes += sc.data_end - sc.data_off;
            if (sc.level + 1 > f.nlevels) f.nlevels = sc.level + 1;
            f.scans.push_back(sc);
        }
        // every other segment (APPn, COM, ...) is skipped
    }
}

// A file's head.  accept == 0: parse_header and its reasons; with kAcceptProgressive a progressive file is walked to its end (its
// scans are checked on the way: nothing is left to plan).
inline bool head_file(const uint8_t* file, size_t bytes, uint32_t accept, File& f, std::string& why) {
    if ((accept & kAcceptProgressive) && frame_is_progressive(file, bytes)) return parse_progressive(file, bytes, f, why);
    f.progressive = false;
    f.scans.clear(); f.pool.clear();
    f.nlevels = 1;
    if (!parse_header(file, bytes, f.hd, why)) return false;
    f.nstreams = f.hd.nstreams;
    f.data_bytes = bytes - f.hd.scan_off;
    return true;
}
// the whole decision for one file: with accept == 0 it is plan()
inline bool plan_file(const uint8_t* file, size_t bytes, uint32_t accept, File& f, std::string& why) {
    return head_file(file, bytes, accept, f, why) && (f.progressive || split_scan(f.hd, file, bytes, nullptr, 0, nullptr, why));
}
// ---- EXIF orientation ----------------------------------------------------------------------------------------------------------------
// The payload of an APP1 segment (behind its length) -> the orientation its IFD0 names: tag 0x0112 of type SHORT, count 1, value 1..8.
// 0: the payload is not an Exif block (the walk goes on to the next APP1).  Everything else that is not exactly that -- a TIFF header
// that is none, an offset or an entry outside the payload, another type or count, a value outside 1..8 -- is 1: an upload with a broken
// EXIF block is an upright upload, never a refused one.  No read leaves p[0 .. n).
// The TIFF walk behind that prefix, shared with a PNG's eXIf chunk (png_parse.hpp), whose payload starts with the TIFF header: t[0 .. m)
// -> 1..8 by the rules above, 1 for everything else.
inline int tiff_orientation(const uint8_t* t, size_t m) {
    if (m < 8) return 1;
    bool le;
    if (t[0] == 'I' && t[1] == 'I') le = true; else if (t[0] == 'M' && t[1] == 'M') le = false; else return 1;
    auto r16 = [&](size_t o) -> uint32_t { return le ? (uint32_t)t[o] | (uint32_t)t[o + 1] << 8 : (uint32_t)t[o] << 8 | t[o + 1]; };      // callers checked o + 2 <= m
    auto r32 = [&](size_t o) -> uint32_t { return le ? r16(o) | r16(o + 2) << 16 : r16(o) << 16 | r16(o + 2); };
    if (r16(2) != 42) return 1;
    const size_t ifd = r32(4);
    if (ifd > m || m - ifd < 2) return 1;
    const uint32_t entries = r16(ifd);
    for (uint32_t k = 0; k < entries; ++k) {
        const size_t e = ifd + 2 + 12 * (size_t)k;
        if (e > m || m - e < 12) return 1;
        if (r16(e) != 0x0112) continue;
        if (r16(e + 2) != 3 || r32(e + 4) != 1) return 1;
        const uint32_t v = r16(e + 8);
        return v >= 1 && v <= 8 ? (int)v : 1;
    }
    return 1;
}
inline int exif_orientation(const uint8_t* p, size_t n) {
    if (n < 6 || std::memcmp(p, "Exif\0\0", 6) != 0) return 0;
    return tiff_orientation(p + 6, n - 6);                         // the TIFF header: offsets count from there
}
// the orientation of a file: that of its first APP1 segment in front of the scan that is an Exif block; 1 when there is none or the
// markers cannot be walked (the planner decides about such a file, not this)
inline int file_orientation(const uint8_t* file, size_t bytes) {
    if (!file || bytes < 4 || file[0] != 0xFF || file[1] != 0xD8) return 1;
    size_t i = 2;
    while (i + 4 <= bytes) {
        if (file[i] != 0xFF) return 1;
        while (i < bytes && file[i] == 0xFF) ++i;
        if (i + 2 >= bytes) return 1;
        const unsigned b = file[i++];
        if (b == 0xDA || b == 0xD9 || b == 0xD8 || b == 0x00 || b == 0x01 || (b >= 0xD0 && b <= 0xD7)) return 1;
        const size_t len = (size_t)file[i] << 8 | file[i + 1];
        if (len < 2 || len > bytes - i) return 1;
        if (b == 0xE1) { const int o = exif_orientation(file + i + 2, len - 2); if (o) return o; }
        i += len;
    }
    return 1;
}

// bytes the streams of this file need at most in the staging area (each stream starts on a multiple of 4)
inline size_t file_room(const File& f, size_t bytes) { return f.progressive ? f.data_bytes + 4 * (size_t)f.nstreams + 8 : scan_room(f.hd, bytes); }
// every scan cut, in file order: the streams' bytes to dst (dst == null: only check), their records to streams[0 .. f.nstreams)
inline bool split_file(const File& f, const uint8_t* file, size_t bytes, uint8_t* dst, size_t room, DecStream* streams, std::string& why) {
    if (!f.progressive) return split_scan(f.hd, file, bytes, dst, room, streams, why);
    size_t o = 0, end = 0;
    uint32_t s0 = 0;
    for (const Scan& sc : f.scans) {
        if (!split_data(file, bytes, sc.data_off, sc.restart, sc.nstreams, sc.nmcu, dst, room, o, streams ? streams + s0 : nullptr, why, &end)) return false;
        if (end != sc.data_end) return refuse(why, "corrupt JPEG data (the file changed since it was planned)");
        s0 += sc.nstreams;
    }
    return true;
}

}  // namespace jpegparse
}  // namespace ire
