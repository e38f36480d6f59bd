// conv_prims.hpp -- the wave-level vocabulary of the convolution kernels (conv_*.hip): the vector types, the bf16 pack / unpack,
// SiLU, the LDS-DMA load, the cross-lane sums and the stage barriers.  Device code only.  Every conv kernel includes this header;
// a new kernel includes it too and does not copy from it -- a changed wait-state rule or a compiler fix is then made once, here.
// What exists once and serves one kernel stays in that kernel's file (conv_pk's pk_touch, conv_down's dn_wait_vm, ...).
// gn_fold.hpp::gnf_xlane_add is the double-precision relative of the cross-lane sums and keeps its own asm.
#pragma once

namespace ire {

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
typedef float f32x16_t __attribute__((ext_vector_type(16)));
typedef unsigned u32x4_t __attribute__((ext_vector_type(4)));

// two f32 -> one dword of two bf16 (a in the low half), round to nearest even: one v_cvt_pk_bf16_f32
__device__ __forceinline__ unsigned pack_bf16(float a, float b) {
    f32x2_t f = {a, b};
    bf16x2_t v = __builtin_convertvector(f, bf16x2_t);
    return __builtin_bit_cast(unsigned, v);
}
__device__ __forceinline__ float bf16_lo(unsigned u) { return __builtin_bit_cast(float, u << 16); }
__device__ __forceinline__ float bf16_hi(unsigned u) { return __builtin_bit_cast(float, u & 0xffff0000u); }

__device__ __forceinline__ float silu(float y) {
    // y * sigmoid(y); exp2/rcp hardware approximations (rel. err ~1e-6, far below bf16)
    float e = __builtin_amdgcn_exp2f(-1.4426950408889634f * y);
    return y * __builtin_amdgcn_rcpf(1.0f + e);
}

// LDS-DMA, 16 B per lane (1 KB per wave-instruction): LDS destination = wave-uniform byte address (through M0) + lane*16; the
// source is per lane.  M0 is saved and restored around the load: the compiler may hold a value of its own there and is not told
// that the asm writes it (`s_nop 0`: the wait state between the M0 write and the load that reads it).  Not visible to the
// compiler's s_waitcnt bookkeeping: the caller waits (vmcnt) and barriers before anybody reads the destination.
__device__ __forceinline__ void glds16(const void* gsrc, unsigned lds_dst_uniform) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_dst_uniform) : "memory");
}

// Sum over the lanes that share (lane % NCC), NCC in {4, 8}: row rotations (DPP) inside the 16-lane rows, then
// the two permlane swaps across rows / wave halves.  Every lane ends with the total; fixed order => deterministic.
// The swaps are inline asm on purpose: with the builtins hipcc (ROCm 7.2) folds the two results into one register
// when both inputs are the same value (verified in the ISA); the two v_nop are the VALU-write -> permlane wait states.
template <int N> __device__ __forceinline__ float ror_add(float v) {
    const int r = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x120 + N, 0xf, 0xf, false);
    return v + __builtin_bit_cast(float, r);
}
__device__ __forceinline__ float swap16_add(float v) {
    float x = v, y = v;
    asm volatile("v_nop\n\tv_nop\n\tv_permlane16_swap_b32 %0, %1" : "+v"(x), "+v"(y));
    return x + y;
}
__device__ __forceinline__ float swap32_add(float v) {
    float x = v, y = v;
    asm volatile("v_nop\n\tv_nop\n\tv_permlane32_swap_b32 %0, %1" : "+v"(x), "+v"(y));
    return x + y;
}
template <int NCC> __device__ __forceinline__ float group_sum(float v) {
    if constexpr (NCC == 4) v = ror_add<4>(v);
    v = ror_add<8>(v);
    v = swap16_add(v);
    return swap32_add(v);
}

// The per-stage barrier of the producer / consumer kernels, spelled out: only LDS traffic has to be ordered (the tile a producer
// just wrote, the partials a consumer just wrote); global loads, stores and LDS-DMA stay in flight across it.  (hipcc's
// __syncthreads() is the same two instructions on gfx950 -- its workgroup-scope fence waits for lgkmcnt only -- measured equal;
// the asm form states the requirement.)
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// The stage barrier of the all-DMA kernels: this wave's DMA pieces of the next stage have landed, its LDS reads are done; behind
// the barrier everybody's are.  KEEP = 0 waits for every vector-memory operation.  KEEP = 16: the stage that follows an epilogue --
// its successor's pieces were issued IN FRONT of the epilogue's 16 output stores (vector-memory operations retire in issue order:
// "all but the 16 youngest" = exactly those pieces), so the stores drain in the background instead of in front of a barrier (all
// 256 workgroups store 128 KB at the same moment: 30 us per launch when waited for).
template <int KEEP> __device__ __forceinline__ void stage_barrier() {
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" :: "n"(KEEP) : "memory");
}

// Taps of pixel phase p = a*2 + b of a stride-2 3x3 convolution run as four unit-stride ones: offsets dy, dx in {-1, 0}, two
// per axis on the odd phase of that axis, one on the even.
__host__ __device__ constexpr int phase_ntaps(int p) { return ((p >> 1) ? 2 : 1) * ((p & 1) ? 2 : 1); }

}  // namespace ire
