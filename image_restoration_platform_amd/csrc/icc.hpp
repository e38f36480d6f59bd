// icc.hpp -- the device side of the ICC conversion of uploads (icc.hip): n tightly packed RGB images converted to sRGB in place by
// the all-integer transform of icc_parse.hpp, one launch whatever n.  The engine holds one IccConverter; like the JPEG decoder it has
// two users that never share scratch: the engine's own entries (under the engine's lock) and the batcher's upload jobs (its launcher
// thread, always on the copy-in stream).
#pragma once
#include "common.hpp"
#include "device_buf.hpp"
#include "icc_parse.hpp"

namespace ire {

// a batch's blob, pinned and on the device: [n] records {int32 kind, uint32 table offset}, then the tables of the images that need
// one -- IccMatrixTable for kMatrix, 256 bytes (enc8(lin[0][v]), composed on the host) for kGrey
struct IccRecord { int32_t kind; uint32_t off; };
struct IccMatrixTable { int32_t m[9]; int32_t pad; uint16_t lin[3][256]; };
static_assert(sizeof(IccMatrixTable) == 1576 && sizeof(IccRecord) == 8, "the blob's layout");
// the encode tables, shared by all images: coarse[4096] bytes, then last[256] u16 (icc_parse.hpp EncTables)
constexpr size_t kIccEncBytes = 4096 + 512;

class IccConverter {
public:
    ~IccConverter();
    void setup(int max_batch);         // uploads the encode tables (the device is current)
    // image i (h x w x 3 bytes at d_rgb + i * image_pitch) by t[i]; a null entry, kNone and kIdentity leave the image as it is.  When
    // no image needs a transform nothing is enqueued.  The tables are copied into pinned staging before return; the only wait of the
    // host is for the upload of the call before last from the same user (two blobs, used in turn).  batch: the batcher's scratch.
    void to_srgb_device(bool batch, uint8_t* d_rgb, int n, int h, int w, size_t image_pitch, const icc::Transform* const* t, hipStream_t s);
    void to_srgb_host(uint8_t* rgb, int n, int h, int w, const icc::Transform* const* t, hipStream_t s);      // synchronous, images h*w*3 apart

private:
    struct Scratch {
        Buf<PinnedMem> pin[2];
        Buf<DeviceMem> d_blob;
        hipEvent_t up_ev[2] = {};
        bool up_recorded[2] = {};
        int turn = 0;
    };
    int max_batch_ = 8;
    Scratch own_, batch_;
    Buf<DeviceMem> d_enc_, d_host_;
};

}  // namespace ire
