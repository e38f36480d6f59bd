// ire_ffi.mjs -- the ffi-napi binding BASELINE.json's north_star names: every entry point of include/ire.h, equivalent to
// the N-API shim (ire_napi.cc).  `ffi-napi` / `ref-napi` cannot be installed in the build image (no network), so this file is
// never LOADED there; tests/test_abi.py parses it and checks every declaration (name, return type, argument count and kinds)
// against include/ire.h, so a deployment that has the two modules can bind libire.so without compiling the shim.
//   const lib = bindIre('/opt/ire/image_restoration_platform_amd/lib/libire.so');
//   lib.ire_classify.async(engine, rgb, 1, h, w, 3 * w, flags, scores /* Float64Array(7) */, labels, cb)   // libuv pool, like sharp
import ffi from 'ffi-napi';
import ref from 'ref-napi';

const P = ref.refType(ref.types.void);       // any pointer (buffers, opaque handles, structs)
const PP = ref.refType(P);                   // pointer to a handle (ire_engine**, ire_job**, ire_strips**)
const IP = ref.refType(ref.types.int);       // int*
export const IRE_ABI_VERSION = 3;
export function bindIre(libPath) {
  return ffi.Library(libPath, {
    ire_abi_version: ['int', []],
    ire_init: ['int', [P, PP]],
    ire_shutdown: ['void', [P]],
    ire_last_error: ['string', []],
    ire_load_weights: ['int', [P, P, 'size_t']],
    ire_max_batch_for: ['int', [P, 'int', 'int']],
    ire_classify: ['int', [P, P, 'int', 'int', 'int', 'int', P, P, P]],
    ire_restore: ['int', [P, P, 'int', 'int', 'int', P, P, P, P]],
    ire_fuse: ['int', [P, P, 'int', 'int', 'int', 'double', P, P, P]],
    ire_classify_device: ['int', [P, P, 'int', 'int', 'int', P, P, P, P]],
    ire_restore_device: ['int', [P, P, 'int', 'int', 'int', P, P, P, P]],
    ire_fuse_device: ['int', [P, P, 'int', 'int', 'int', 'double', P, P, P]],
    ire_fuse_batch_device: ['int', [P, P, 'int', 'int', 'int', 'int', P, P, P, P]],
    ire_preprocess_plan: ['int', ['int', 'int', 'int', 'int', IP, IP, IP]],
    ire_preprocess: ['int', [P, P, 'int', 'int', 'int', 'int', P, 'int', 'int']],
    ire_preprocess_device: ['int', [P, P, 'int', 'int', 'int', 'int', P, 'int', 'int', P]],
    ire_png_base64_bytes: ['size_t', ['int', 'int']],
    ire_encode_png_base64_device: ['int', [P, P, 'int', 'int', 'int', P, 'size_t', P]],
    ire_encode_png_base64: ['int', [P, P, 'int', 'int', 'int', P, 'size_t']],
    ire_restore_fit: ['int', [P, P, 'int', 'int', 'int', P, P, P, P]],
    ire_restore_fit_device: ['int', [P, P, 'int', 'int', 'int', P, P, P, P]],
    ire_png_base64_bytes_fit: ['size_t', ['int', 'int']],
    ire_encode_png_base64_fit_device: ['int', [P, P, 'int', 'int', 'int', 'size_t', 'size_t', P, 'size_t', P]],
    ire_encode_png_base64_fit: ['int', [P, P, 'int', 'int', 'int', P, 'size_t']],
    ire_submit_fit: ['int', [P, P, 'int', 'int', 'int', P, PP]],
    ire_submit_jpeg: ['int', [P, P, 'size_t', P, PP]],
    ire_submit_file: ['int', [P, P, 'size_t', P, PP]],
    ire_submit_upload: ['int', [P, P, 'size_t', 'int', P, PP]],
    ire_upload_plan: ['int', [P, 'size_t', 'int', 'int', P, P, P, P, P]],
    ire_icc_plan_profile: ['int', [P, 'size_t', 'int', P]],
    ire_icc_plan_file: ['int', [P, 'size_t', P]],
    ire_icc_to_srgb_device: ['int', [P, P, 'int', 'int', 'int', 'size_t', P, P]],
    ire_icc_to_srgb: ['int', [P, P, 'int', 'int', 'int', P]],
    ire_preprocess_batch_device: ['int', [P, P, 'int', 'int', 'int', 'size_t', 'int', 'int', P, 'int', 'int', 'size_t', P]],
    ire_submit_fuse_fit: ['int', [P, P, 'int', 'int', 'int', P, P, P, PP]],
    ire_restore_fuse_fit_device: ['int', [P, P, 'int', 'int', 'int', 'int', P, P, P, P]],
    ire_submit: ['int', [P, P, 'int', 'int', 'int', P, PP]],
    ire_poll: ['int', [P, P, 'int', P, P, P]],
    ire_poll_text: ['int', [P, P, 'int', P, 'size_t', P, P, P]],
    ire_png_deflate_base64_bound: ['size_t', ['int', 'int']],
    ire_encode_png_deflate_base64_fit_device: ['int', [P, P, 'int', 'int', 'int', 'size_t', 'size_t', P, 'size_t', P, P]],
    ire_encode_png_deflate_base64_fit: ['int', [P, P, 'int', 'int', 'int', P, 'size_t', P]],
    ire_jpeg_base64_bound: ['size_t', ['int', 'int']],
    ire_encode_jpeg_base64_fit_device: ['int', [P, P, 'int', 'int', 'int', 'size_t', 'size_t', P, 'size_t', P, P]],
    ire_encode_jpeg_base64_fit: ['int', [P, P, 'int', 'int', 'int', P, 'size_t', P]],
    // (quality 1..100 | 0: 85; sampling 0 = 4:4:4, 2 = 4:2:0.  ire_config, passed to ire_init as a buffer, ends with the two as int32)
    ire_jpeg_base64_bound_ex: ['size_t', ['int', 'int', 'int', 'int']],
    ire_encode_jpeg_base64_fit_device_ex: ['int', [P, P, 'int', 'int', 'int', 'size_t', 'size_t', P, 'size_t', P, 'int', 'int', P]],
    ire_encode_jpeg_base64_fit_ex: ['int', [P, P, 'int', 'int', 'int', P, 'size_t', P, 'int', 'int']],
    // (the same with the image's own, optimised Huffman tables)
    ire_jpeg_optimized_base64_bound: ['size_t', ['int', 'int', 'int', 'int']],
    ire_encode_jpeg_optimized_base64_fit_device: ['int', [P, P, 'int', 'int', 'int', 'size_t', 'size_t', P, 'size_t', P, 'int', 'int', P]],
    ire_encode_jpeg_optimized_base64_fit: ['int', [P, P, 'int', 'int', 'int', P, 'size_t', P, 'int', 'int']],
    // (the same as a progressive file: ten scans, each under its own optimal table)
    ire_jpeg_progressive_base64_bound: ['size_t', ['int', 'int', 'int', 'int']],
    ire_encode_jpeg_progressive_base64_fit_device: ['int', [P, P, 'int', 'int', 'int', 'size_t', 'size_t', P, 'size_t', P, 'int', 'int', P]],
    ire_encode_jpeg_progressive_base64_fit: ['int', [P, P, 'int', 'int', 'int', P, 'size_t', P, 'int', 'int']],
    ire_decode_jpeg_plan: ['int', [P, 'size_t', P, P, P]],
    // (accept is a uint32_t of flag bits, 0 or 1 today: passed as an int)
    ire_decode_jpeg_plan_ex: ['int', [P, 'size_t', 'int', P, P, P, P]],
    ire_decode_jpeg: ['int', [P, P, 'size_t', P, 'int', 'int']],
    ire_decode_jpeg_device: ['int', [P, P, P, 'int', 'int', 'int', P, 'size_t', P, P]],
    ire_decode_png_plan: ['int', [P, 'size_t', P, P, P]],
    // (accept: 0 or IRE_DECODE_ACCEPT_PNG_ALL = 32, passed as an int)
    ire_decode_png_plan_ex: ['int', [P, 'size_t', 'int', P, P, P, P, P]],
    ire_decode_png: ['int', [P, P, 'size_t', P, 'int', 'int']],
    ire_decode_png_device: ['int', [P, P, P, 'int', 'int', 'int', P, 'size_t', P, P]],
    ire_job_release: ['int', [P, P]],
    ire_affinity_plan: ['int', ['string', 'string', P, 'size_t', IP, IP, IP]],
    ire_engine_affinity: ['int', [P, P, 'size_t', IP]],
    ire_restore_tiled_device: ['int', [P, P, 'int', 'int', 'int', P, P, P, P]],
    ire_strips_stats_bytes: ['size_t', ['int', 'int']],
    ire_strips_open: ['int', [P, 'int', 'int', 'int', 'int', 'int', P, PP]],
    ire_strips_close: ['void', [P]],
    ire_strips_num_ops: ['int', [P]],
    ire_strips_set_input: ['int', [P, P, P, P]],
    ire_strips_run_op: ['int', [P, 'int', P, P]],
    ire_strips_pack_halo: ['int', [P, 'int', P, P, P]],
    ire_strips_unpack_halo: ['int', [P, 'int', P, P, P]],
    ire_strips_get_output: ['int', [P, P, P]],
    ire_get_stats: ['int', [P, P]],
    ire_debug_classifier_sums: ['int', [P, 'int', P]],
    ire_debug_fusion_wlut: ['int', [P, P, 'int', P]],
    ire_debug_jpeg_huffman: ['int', [P, P, 'int', P, P]],
    ire_debug_jpeg_progressive_from_coefs: ['int', [P, P, 'int', 'int', 'int', 'int', 'int', P, 'size_t', P]],
    ire_debug_poison_scratch: ['int', [P, 'int', P]],
    ire_debug_gn_finalize: ['int', [P, P, 'int', 'int', 'int', 'int', P, P, P, 'int', 'int', P]],
    ire_debug_capture: ['int', [P, 'int']],
    ire_debug_activation: ['int', [P, 'string', P, P]],
    ire_profile_enable: ['int', [P, 'int']],
    ire_profile_query: ['int', [P, 'string', P, P, P, P]],
    ire_profile_reset: ['int', [P]],
    ire_profile_report: ['int', [P, P, 'size_t', P]],
  });
}
