// The exact e2m1 / e8m0 decode and the MFMA step that mxfp4_linear.hip (dense linears) and mxfp4_moe.hip (routed experts) share: both
// read the tile image described at the top of mxfp4_linear.hip.
#pragma once
#include "common.h"
#include <hip/hip_runtime.h>

typedef _Float16 mx4_f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int mx4_u32x4 __attribute__((ext_vector_type(4)));

template <int DT> __device__ __forceinline__ float mx4_h2f(uint16_t h) { return DT == MI355_DTYPE_BF16 ? bf16_to_f32(h) : f16_bits_to_f32(h); }
template <int DT> __device__ __forceinline__ uint16_t mx4_f2h(float f) { return DT == MI355_DTYPE_BF16 ? f32_to_bf16(f) : f32_to_f16_bits(f); }
template <int DT> __device__ __forceinline__ float mx4_rnd(float f) { return mx4_h2f<DT>(mx4_f2h<DT>(f)); }

template <int DT>
__device__ __forceinline__ f32x4_t mx4_mfma(const uint4& a, const uint4& b, const f32x4_t& c) {
    if constexpr (DT == MI355_DTYPE_BF16)
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(mx4_f16x8, a), __builtin_bit_cast(mx4_f16x8, b), c, 0, 0, 0);
}
// group j (0..3) of a lane's scale dword as the f32 number 2^(code - 127): the e8m0 code IS the f32 exponent field
__device__ __forceinline__ float mx4_scale(uint32_t s4, int j) { return __uint_as_float(((s4 >> (8 * j)) & 0xFFu) << 23); }
// does one of the four scale bytes hold 0xFF?  (low seven bits all set AND the top bit set)
__device__ __forceinline__ uint32_t mx4_has_nan(uint32_t s4) { return ((s4 & 0x7F7F7F7Fu) + 0x01010101u) & s4 & 0x80808080u; }
// one dword = 8 e2m1 codes (k ascending, low nibble first) -> one B fragment.  bf16: times `sf` (a power of two; the instruction reads
// its exponent), exact; f16: unscaled, the caller applies sf to the accumulator
template <int DT>
__device__ __forceinline__ uint4 mx4_frag(uint32_t w, float sf) {
    if constexpr (DT == MI355_DTYPE_BF16)
        return make_uint4(__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sf, 0)),
                          __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sf, 1)),
                          __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sf, 2)),
                          __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, sf, 3)));
    else
        return make_uint4(__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, 1.0f, 0)),
                          __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, 1.0f, 1)),
                          __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, 1.0f, 2)),
                          __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, 1.0f, 3)));
}
__device__ __forceinline__ uint32_t mx4_dword(const uint4& v, int j) { return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w; }
// one 32-k MFMA step into the running sum y: bf16 accumulates straight through (the scale sits in the operand), f16 through a fresh
// accumulator and one fma per register
template <int DT>
__device__ __forceinline__ void mx4_step(f32x4_t& y, const uint4& a, const uint4& b, const float sf) {
    if constexpr (DT == MI355_DTYPE_BF16) {
        y = mx4_mfma<DT>(a, b, y);
    } else {
        const f32x4_t acc = mx4_mfma<DT>(a, b, f32x4_t{0.f, 0.f, 0.f, 0.f});
#pragma unroll
        for (int v = 0; v < 4; ++v) y[v] = fmaf(sf, acc[v], y[v]);
    }
}

__device__ __forceinline__ void mx4_dma(const uint8_t* gsrc_lane, uint32_t lds_dst) {
    // 1 KiB per wave: lane l copies 16 B from its own source address to lds_dst + 16 l (inline asm: neither counted nor drained by hipcc)
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc_lane), "s"(lds_dst) : "memory");
}
