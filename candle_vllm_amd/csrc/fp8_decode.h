// The exact e4m3fn decode, the MFMA step and the LDS-DMA idiom that fp8_linear.hip (dense linears) and fp8_moe.hip (routed experts)
// share: both read the tile image described at the top of fp8_linear.hip.
#pragma once
#include "common.h"
#include <hip/hip_runtime.h>

typedef _Float16 fp8l_f16x8 __attribute__((ext_vector_type(8)));
typedef float fp8l_f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int fp8l_u32x4 __attribute__((ext_vector_type(4)));

template <int DT> __device__ __forceinline__ float fp8l_h2f(uint16_t h) { return DT == MI355_DTYPE_BF16 ? bf16_to_f32(h) : f16_bits_to_f32(h); }
template <int DT> __device__ __forceinline__ uint16_t fp8l_f2h(float f) { return DT == MI355_DTYPE_BF16 ? f32_to_bf16(f) : f32_to_f16_bits(f); }
template <int DT> __device__ __forceinline__ float fp8l_rnd(float f) { return fp8l_h2f<DT>(fp8l_f2h<DT>(f)); }

template <int DT>
__device__ __forceinline__ f32x4_t fp8l_mfma(const uint4& a, const uint4& b, const f32x4_t& c) {
    if constexpr (DT == MI355_DTYPE_BF16)
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(fp8l_f16x8, a), __builtin_bit_cast(fp8l_f16x8, b), c, 0, 0, 0);
}
// two e4m3fn bytes (`hi` selects the upper half of w) -> two 16-bit values, exactly: the hardware convert handles the subnormals
// 0x01..0x07 and both zeros; the NaN codes 0x7f / 0xff come out as NaN
template <int DT>
__device__ __forceinline__ uint32_t fp8l_pair(uint32_t w, bool hi) {
    const fp8l_f32x2 f = hi ? __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true) : __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
    if constexpr (DT == MI355_DTYPE_BF16)
        return __builtin_amdgcn_perm(__float_as_uint(f.y), __float_as_uint(f.x), 0x07060302u);      // the upper halves: nothing below them is set
    else
        return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pkrtz(f.x, f.y));                  // |v| in [2^-9, 448], 3 mantissa bits: exact in f16
}
// 8 bytes (k ascending) -> one B fragment
template <int DT>
__device__ __forceinline__ uint4 fp8l_frag(uint32_t lo, uint32_t hi) {
    return make_uint4(fp8l_pair<DT>(lo, false), fp8l_pair<DT>(lo, true), fp8l_pair<DT>(hi, false), fp8l_pair<DT>(hi, true));
}

__device__ __forceinline__ void fp8l_dma(const uint8_t* gsrc_lane, uint32_t lds_dst) {
    // 1 KiB per wave: lane l copies 16 B from its own source address to lds_dst + 16 l (inline asm: neither counted nor drained by hipcc)
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc_lane), "s"(lds_dst) : "memory");
}
