// NVFP4 (e2m1 elements, one e4m3fn scale per 16 k, one f32 scale per tensor) linears for the safetensors path: `LnNvfp4`
// (src/openai/models/linear.rs:1760-1943), the layer the `quant_method: "nvfp4"` exports (ModelOpt / compressed-tensors) load.  The weight is
// [out, in/2] bytes -- MXFP4's coding: byte j of a row holds element 2j in its LOW nibble, a nibble = sign (bit 3) | index into
// {0, 0.5, 1, 1.5, 2, 3, 4, 6} -- with [out, in/16] e4m3fn scale bytes and the f32 multiplier g the reference ends up with
// (1 / weight_global_scale, or weight_scale_2, or 1.0: linear.rs:1829-1853; the caller passes the multiplier):
//     y[t, r] = round_dt( g * sum_c x[t, c] * e2m1(w[r, c]) * e4m3(s[r, c/16]) )          (+ bias, + the fused epilogues of mi355_linear)
// `input_scale` (linear.rs:1855-1879) scales QUANTISED activations; this op is W4A16, quantises nothing and ignores it.
// Accumulation is f32 (v_mfma_f32_16x16x32_{bf16,f16}).  A scale group is HALF an MFMA step, so neither of MXFP4's folds carries over -- but
// in the B-fragment order of the image (lane = 16 * ((k%32)/8) + n%16, 8 consecutive k per lane and step) a lane's 8 operand elements lie
// inside one group, so the scale is folded into the operand per lane, EXACTLY in both dtypes: e2m1 has <= 2 significant bits and e4m3
// <= 4, the product <= 6, |product| in [2^-10, 2688] or 0 -- a normal f16 and a bf16 number.  One f32 accumulator runs through all of K
// for both dtypes; g multiplies the f32 sum in the epilogue, before the first rounding (SILU_MUL: g for the gate half, g_up for up).
// The fold does NOT rest on what v_cvt_scalef32_pk_*_fp4 does with the mantissa of its scale operand (only powers of two go in there):
//   * f16 (10 VALU per MFMA step): the scale byte shifted left by 7 IS the f16 number e4m3(s) * 2^-8 (same exponent position, bias 15 - 7
//     = 8 lower; subnormals map to subnormals, zero to zero), so: decode the nibbles times 2^8 (v_cvt_scalef32_pk_f16_fp4, <= 1536), then
//     one v_pk_mul_f16 per pair by that number -- the 2^8 cancels and the product is exact by the argument above;
//   * bf16 (13 VALU per MFMA step): v_cvt_f32_fp8 decodes the scale byte (subnormals included), v_cvt_scalef32_pk_f32_fp4 the nibbles,
//     v_pk_mul_f32 multiplies a pair (exact) and one v_perm_b32 keeps the two high halves (truncation of a number of <= 6 bits = rounding).
// 40 (f16) / 52 (bf16) VALU per lane, tile and k-block where MXFP4 has 16.
// A NaN scale (0x7F / 0xFF) makes the outputs of its row NaN (the lane that owns the row remembers it and poisons its column before the
// epilogue, independent of the decode); other codes with the sign bit set run clean, value not promised.
//
// Tile image (mi355_nvfp4_tile_repack; nv4_tile_kernel below writes it): 16-row x 128-k tiles,
//     blocks: [tile n/16][k-block k/128][lane = 16 * ((k%32)/8) + n%16][16 B = [(k%128)/32][(k%8)/2]]      (1 KiB: MXFP4's, byte for byte)
//     scales: [tile n/16][k-block k/128][half ((k%32)/16)][row n%16][step (k%128)/32]                      (128 B per tile and k-block)
// -- in MFMA step j of a k-block lane (n%16, kg) multiplies k = 32 j + 8 kg ..+7, i.e. group 2 j + kg/2: the four scales a lane needs in
// a k-block are ONE dword (half kg/2, its row), and 8 k-blocks of a tile's scales are one contiguous KiB (what the GEMM's DMA moves).
//
// Two kernels:
//   nvfp4_small_kernel  1..32 tokens: streaming mat-vec, the weights never touch LDS (register ring, NS_RING k-blocks ahead)
//   nvfp4_gemm_kernel   33.. tokens: 128 x 128 MFMA tile, both operands global -> LDS by DMA, the weight side as packed nibbles
// (33..96 tokens with too few GEMM tiles to fill the chip: 32-token chunks of the first -- nvfp4_run at the end of the file)
#include "common.h"
#include "../../include/mi355_vllm.h"
#include <hip/hip_runtime.h>

typedef _Float16 nv4_f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 nv4_f16x2 __attribute__((ext_vector_type(2)));
typedef unsigned int nv4_u32x4 __attribute__((ext_vector_type(4)));

struct Nv4Args {
    const uint8_t* w;         // tiled blocks
    const uint8_t* s;         // tiled scales
    const void* x;            // 16-bit [T][K]
    void* out;                // 16-bit [T][ldo]
    const void* bias;         // 16-bit [N] or null
    const void* resid;        // 16-bit [T][ldo] (EPI_RESID; may be `out`)
    int32_t T, N, K, ldo, epi;
    int32_t pair_offset;      // SILU_MUL: rows of `up` start here (packed [gate; up], mlp.rs:324-352)
    float g, g_up;            // per-tensor multipliers (g_up: the up half of SILU_MUL)
};

template <int DT> __device__ __forceinline__ float nv4_h2f(uint16_t h) { return DT == MI355_DTYPE_BF16 ? bf16_to_f32(h) : f16_bits_to_f32(h); }
template <int DT> __device__ __forceinline__ uint16_t nv4_f2h(float f) { return DT == MI355_DTYPE_BF16 ? f32_to_bf16(f) : f32_to_f16_bits(f); }
template <int DT> __device__ __forceinline__ float nv4_rnd(float f) { return nv4_h2f<DT>(nv4_f2h<DT>(f)); }

template <int DT>
__device__ __forceinline__ f32x4_t nv4_mfma(const uint4& a, const uint4& b, const f32x4_t& c) {
    if constexpr (DT == MI355_DTYPE_BF16)
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(nv4_f16x8, a), __builtin_bit_cast(nv4_f16x8, b), c, 0, 0, 0);
}
// does one of the four scale bytes hold 0x7F or 0xFF?  (its low seven bits all set: the add carries into bit 7 only then)
__device__ __forceinline__ uint32_t nv4_has_nan(uint32_t s4) { return ((s4 & 0x7F7F7F7Fu) + 0x01010101u) & 0x80808080u; }

// nibble pair SEL (0..3) of dword w times the scale: two exact 16-bit operand elements
template <int DT, int SEL>
__device__ __forceinline__ uint32_t nv4_pair(uint32_t w, float sf32, nv4_f16x2 sf16) {
    if constexpr (DT == MI355_DTYPE_BF16) {
        const f32x2_t p = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, 1.0f, SEL) * sf32;
        return __builtin_amdgcn_perm(__float_as_uint(p.y), __float_as_uint(p.x), 0x07060302u);      // {hi16(p.x), hi16(p.y)}
    } else {
        return __builtin_bit_cast(uint32_t, __builtin_bit_cast(nv4_f16x2, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(w, 256.0f, SEL)) * sf16);
    }
}
// one dword = 8 e2m1 codes (k ascending, low nibble first) times the scale in byte J of the lane's scale dword -> one B fragment
template <int DT, int J>
__device__ __forceinline__ uint4 nv4_frag(uint32_t w, uint32_t s4) {
    float sf32 = 0.f;
    nv4_f16x2 sf16 = {0, 0};
    if constexpr (DT == MI355_DTYPE_BF16) {
        sf32 = __builtin_amdgcn_cvt_f32_fp8((int)s4, J);
    } else {
        const _Float16 h = __builtin_bit_cast(_Float16, (uint16_t)(((s4 >> (8 * J)) & 0xFFu) << 7));    // e4m3(s) * 2^-8
        sf16 = nv4_f16x2{h, h};
    }
    return make_uint4(nv4_pair<DT, 0>(w, sf32, sf16), nv4_pair<DT, 1>(w, sf32, sf16), nv4_pair<DT, 2>(w, sf32, sf16), nv4_pair<DT, 3>(w, sf32, sf16));
}
template <int DT>
__device__ __forceinline__ uint4 nv4_frag_j(uint32_t w, uint32_t s4, int j) {      // j is a constant after unrolling
    return j == 0 ? nv4_frag<DT, 0>(w, s4) : j == 1 ? nv4_frag<DT, 1>(w, s4) : j == 2 ? nv4_frag<DT, 2>(w, s4) : nv4_frag<DT, 3>(w, s4);
}
__device__ __forceinline__ uint32_t nv4_dword(const uint4& v, int j) { return j == 0 ? v.x : j == 1 ? v.y : j == 2 ? v.z : v.w; }

// the rounding chain of one output element, as dense_gemv.hip's: matmul -> dtype, + bias -> dtype (linear.rs:124-172), then
// + residual -> dtype or silu(gate) -> dtype, * up -> dtype (mlp.rs:457); y and up are f32 sums, still without their global scales
template <int DT>
__device__ __forceinline__ void nv4_epilogue(const Nv4Args& a, const int t, const int col, const float y, const float up) {
    const uint16_t* b16 = static_cast<const uint16_t*>(a.bias);
    float o = nv4_rnd<DT>(a.g * y);
    if (b16) o = nv4_rnd<DT>(o + nv4_h2f<DT>(b16[col]));
    if (a.epi == MI355_EPI_SILU_MUL) {
        float u = nv4_rnd<DT>(a.g_up * up);
        if (b16) u = nv4_rnd<DT>(u + nv4_h2f<DT>(b16[a.pair_offset + col]));
        o = nv4_rnd<DT>(nv4_rnd<DT>(o / (1.f + __expf(-o))) * u);
    } else if (a.epi == MI355_EPI_RESID) {
        o = nv4_rnd<DT>(o + nv4_h2f<DT>(static_cast<const uint16_t*>(a.resid)[(size_t)t * a.ldo + col]));
    }
    static_cast<uint16_t*>(a.out)[(size_t)t * a.ldo + col] = nv4_f2h<DT>(o);
}

// ------------------------------------------------------------------------------------------------ 1..32 tokens
// mxfp4_small_kernel's mould.  One workgroup = R row tiles (R = 2: a gate tile and its up tile) x all of K, NS_NW waves; wave w owns the
// k-blocks w, w + NW, ...
//   * weights: global -> registers in image order, a ring of NS_RING k-blocks per wave: one dwordx4 per lane, tile and k-block (a KiB per
//     wave instruction) and the lane's scale dword (the four groups its fragments of the k-block fall into): 40 ring VGPRs, 80 for a
//     pair; 8 waves x 8 k-blocks x 1 KiB keep 64 KiB (R = 2: 128) in flight per workgroup.  A slot beyond the end of K is not fetched
//     (wave-uniform branch);
//   * activations: staged in LDS by all threads, coalesced, G k-blocks per wave at a time (as much of K as fits NS_X_BYTES); rows padded
//     by 16 B so that the 16 rows of an A-fragment read start on different bank quads;
//   * MT = ceil(T / 16) M tiles; four MFMA steps per k-block, each with the in-register fold of the file comment;
//   * cross-wave reduction through LDS (over the staging area), epilogue out of the sums.
constexpr int NS_NW = 8, NS_RING = 8;
constexpr int NS_X_BYTES = 32 * (NS_NW * 256 + 16);        // 66048: 32 tokens x one k-block per wave; two workgroups per CU

template <int DT, int MT, int R>
__global__ void __launch_bounds__(64 * NS_NW) nvfp4_small_kernel(const Nv4Args a, const int G) {
    extern __shared__ __attribute__((aligned(16))) uint8_t ns_lds[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r16 = lane & 15, kg = lane >> 4;
    const int T = a.T, nkb = a.K >> 7;
    const int niter = (nkb + NS_NW - 1) / NS_NW;            // the same for every wave (the barriers below)
    const int ldx = G * NS_NW * 256 + 16;                   // bytes per staged row
    int row0[R];
    row0[0] = (int)blockIdx.x * 16;
    if (R == 2) row0[R - 1] = a.pair_offset + (int)blockIdx.x * 16;
    const uint8_t* wp[R];
    const uint8_t* sp[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        wp[r] = a.w + ((size_t)(row0[r] >> 4) * nkb) * 1024 + lane * 16;
        sp[r] = a.s + ((size_t)(row0[r] >> 4) * nkb) * 128 + (kg >> 1) * 64 + r16 * 4;
    }
    uint4 ring[NS_RING][R];
    uint32_t rs[NS_RING][R];
#define NS_LOAD(SLOT_, I_) do { \
        const int kb_ = wave + (I_) * NS_NW; \
        if (kb_ < nkb) { \
            _Pragma("unroll") for (int r_ = 0; r_ < R; ++r_) { \
                const nv4_u32x4 v_ = __builtin_nontemporal_load(reinterpret_cast<const nv4_u32x4*>(wp[r_] + (size_t)kb_ * 1024)); \
                ring[SLOT_][r_] = make_uint4(v_.x, v_.y, v_.z, v_.w); \
                rs[SLOT_][r_] = *reinterpret_cast<const uint32_t*>(sp[r_] + (size_t)kb_ * 128); \
            } \
        } \
    } while (0)
#pragma unroll
    for (int s = 0; s < NS_RING; ++s) {
#pragma unroll
        for (int r = 0; r < R; ++r) { ring[s][r] = make_uint4(0u, 0u, 0u, 0u); rs[s][r] = 0u; }
        NS_LOAD(s, s);
    }

    f32x4_t y[R][MT];
    uint32_t bad[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        bad[r] = 0u;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) y[r][mt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    }
    const uint8_t* xg = static_cast<const uint8_t*>(a.x);
    const int pass_cols = G * NS_NW * 128;                  // k columns of one staging pass

    for (int i0 = 0; i0 < niter; i0 += NS_RING) {
#pragma unroll
        for (int s = 0; s < NS_RING; ++s) {
            const int i = i0 + s;
            if (i < niter) {                                 // (uniform over the workgroup)
                const int g = i % G;
                if (g == 0) {
                    // ---- the activations of the next G k-blocks of every wave: columns [c0, c0 + pass_cols) of x
                    const int c0 = (i / G) * pass_cols, cols = min(pass_cols, a.K - c0), ppr = cols >> 3;      // 16-byte pieces per row
                    __syncthreads();                         // everyone is done with the previous pass
                    for (int p = threadIdx.x; p < T * ppr; p += 64 * NS_NW) {
                        const int t = p / ppr, c = p - t * ppr;
                        *reinterpret_cast<uint4*>(ns_lds + (size_t)t * ldx + c * 16) =
                            *reinterpret_cast<const uint4*>(xg + ((size_t)t * a.K + c0) * 2 + c * 16);
                    }
                    __syncthreads();
                }
                const int kb = wave + i * NS_NW;
                if (kb < nkb) {
                    const uint8_t* xl = ns_lds + (size_t)(g * NS_NW + wave) * 256 + 16 * kg;                    // this k-block inside the pass
#pragma unroll
                    for (int r = 0; r < R; ++r) bad[r] |= nv4_has_nan(rs[s][r]);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        uint4 af[MT];
#pragma unroll
                        for (int mt = 0; mt < MT; ++mt)
                            af[mt] = *reinterpret_cast<const uint4*>(xl + (size_t)min(mt * 16 + r16, T - 1) * ldx + 64 * j);
#pragma unroll
                        for (int r = 0; r < R; ++r) {
                            const uint4 bf = nv4_frag_j<DT>(nv4_dword(ring[s][r], j), rs[s][r], j);
#pragma unroll
                            for (int mt = 0; mt < MT; ++mt) y[r][mt] = nv4_mfma<DT>(af[mt], bf, y[r][mt]);
                        }
                    }
                }
                NS_LOAD(s, i + NS_RING);
            }
        }
    }
#undef NS_LOAD
    // ---- cross-wave reduction: C layout = lane (column = weight row r16, rows m = 4 kg + v).  A lane saw the scales of its own half
    // (kg / 2) only, and every lane of a column writes its own four rows: lanes kg and kg ^ 2 of a column share what they saw first
    float* red = reinterpret_cast<float*>(ns_lds);          // [NW][R][MT][16 m][16 rows]
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; ++r) {
        bad[r] |= (uint32_t)__shfl_xor((int)bad[r], 32);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int v = 0; v < 4; ++v)
                red[(((wave * R + r) * MT + mt) * 16 + 4 * kg + v) * 16 + r16] = bad[r] ? __builtin_nanf("") : y[r][mt][v];
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < MT * 256; idx += 64 * NS_NW) {
        const int rr = idx & 15, m = idx >> 4;
        if (m >= T) continue;
        float val[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            float s = 0.f;
#pragma unroll
            for (int w = 0; w < NS_NW; ++w) s += red[(((w * R + r) * MT + (m >> 4)) * 16 + (m & 15)) * 16 + rr];
            val[r] = s;
        }
        nv4_epilogue<DT>(a, m, row0[0] + rr, val[0], val[R - 1]);
    }
}

// ------------------------------------------------------------------------------------------------ prompt steps
// mxfp4_gemm_kernel's structure: workgroup tile 128 tokens x 128 weight rows (SILU_MUL: 64 gate rows and the 64 matching up rows), 4 waves
// as 2 x 2, wave tile 64 x 64 (4 x 4 fragments), two workgroups per CU.  K in steps of 64, the DMA of the next step in flight while this one
// is multiplied:
//   * x: 128 rows x 128 B per step, two buffers, 16-byte slot c of row r at slot c ^ (r & 7) (applied to the lane's global source address);
//   * weights: packed nibbles, the image's KiB runs copied verbatim.  A KiB is a whole k-block of a row tile = TWO K steps, so the weight
//     side has two buffers of 8 row tiles x 1 KiB that turn over once per k-block (filled during the first step of the k-block before).
//     A lane's two B fragments of a step are one ds_read_b64 of its own bytes, folded in registers and used by four m-fragments each;
//   * scales: twice as dense as MXFP4's -- 8 k-blocks of a row tile's scale plane are one contiguous KiB, so the two buffers of 8 row
//     tiles x 1 KiB turn over every 8 k-blocks: the buffer of chunk c + 1 is filled during the first step of chunk c (its last reader,
//     k-block 8 c - 1, is a barrier behind), seven k-blocks before its first reader.  A lane past the end of K re-reads the last k-block:
//     nothing is read outside the plane.  No panel and therefore no limit on K; a lane reads the four scales of its half of its row's
//     k-block as one dword per n-fragment.
// Waits: every DMA of a step (4 A + at most 2 B + at most 2 scale instructions per wave, all issued before that step's MFMAs) fills a
// buffer that the NEXT step or a later one reads, and nothing a step reads is still in flight when it starts, so the count that must
// have landed at the end of a step is all of them: s_waitcnt vmcnt(0), then the barrier (the scale stream adds instructions to the
// first step of every eighth k-block, not a second wait; a count above 0 would leave a B or scale buffer of the next step in flight).
// Both dtypes keep one accumulator set through K.
constexpr uint32_t NG_A_BYTES = 128 * 128, NG_B_BYTES = 8 * 1024, NG_S_BYTES = 8 * 1024;
constexpr uint32_t NG_B_OFF = 2 * NG_A_BYTES, NG_S_OFF = NG_B_OFF + 2 * NG_B_BYTES, NG_LDS = NG_S_OFF + 2 * NG_S_BYTES;      // 64 KiB

__device__ __forceinline__ void nv4_dma(const uint8_t* gsrc_lane, uint32_t lds_dst) {
    // 1 KiB per wave: lane l copies 16 B from its own source address to lds_dst + 16 l (inline asm: neither counted nor drained by hipcc)
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc_lane), "s"(lds_dst) : "memory");
}

template <int DT>
__global__ void __launch_bounds__(256, 2) nvfp4_gemm_kernel(const Nv4Args a) {
    extern __shared__ __attribute__((aligned(1024))) uint8_t ng_lds[];   // [A 2 x 16 KiB][B 2 x 8 KiB][scales 2 x 8 KiB]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int m16 = lane & 15, kg = lane >> 4;
    const bool silu = a.epi == MI355_EPI_SILU_MUL;
    const int nkb = a.K >> 7;
    const int t0 = (int)blockIdx.x * 128;                                // token tiles fastest: neighbours share their weight tile through L2
    const int n_cols = silu ? a.pair_offset : a.N;
    const int c0 = (int)blockIdx.y * (silu ? 64 : 128);
    // first weight row of LDS row tile p (clamped: columns beyond the matrix are computed and never stored)
    auto tile_row = [&](int p) {
        if (!silu) return min(c0 + 16 * p, a.N - 16);
        return p < 4 ? min(c0 + 16 * p, a.pair_offset - 16) : min(a.pair_offset + c0 + 16 * (p - 4), a.N - 16);
    };
    const uint32_t lds0 = __builtin_amdgcn_readfirstlane((uint32_t)(size_t)(__attribute__((address_space(3))) void*)ng_lds);
    // staging sources: A round r = rows 32 r + tid / 8 (8 threads = the 8 slots of a row, one wave = 8 rows = 1 KiB); B and scale piece 4 r + wave
    const int srow = tid >> 3, sslot = tid & 7;
    const uint8_t* asrc[4];
    const uint8_t* bsrc[2];
    const uint8_t* ssrc[2];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = 32 * r + srow;
        asrc[r] = static_cast<const uint8_t*>(a.x) + ((size_t)min(t0 + row, a.T - 1) * a.K) * 2 + (size_t)((sslot ^ (row & 7)) * 16);
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const size_t tk = (size_t)(tile_row(4 * r + wave) >> 4) * nkb;
        bsrc[r] = a.w + tk * 1024 + lane * 16;
        ssrc[r] = a.s + tk * 128 + (lane & 7) * 16;                      // + 128 * k-block (lane / 8 of the chunk of 8)
    }
    auto stage_a = [&](int kt, int buf) {
        const uint32_t base = lds0 + (uint32_t)buf * NG_A_BYTES + (uint32_t)wave * 1024u;
#pragma unroll
        for (int r = 0; r < 4; ++r) nv4_dma(asrc[r] + (size_t)kt * 128, base + (uint32_t)r * 4096u);
    };
    auto stage_b = [&](int kb, int buf) {
        const uint32_t base = lds0 + NG_B_OFF + (uint32_t)buf * NG_B_BYTES + (uint32_t)wave * 1024u;
#pragma unroll
        for (int r = 0; r < 2; ++r) nv4_dma(bsrc[r] + (size_t)kb * 1024, base + (uint32_t)r * 4096u);
    };
    auto stage_s = [&](int chunk, int buf) {
        const uint32_t base = lds0 + NG_S_OFF + (uint32_t)buf * NG_S_BYTES + (uint32_t)wave * 1024u;
        const int kb = min(8 * chunk + (lane >> 3), nkb - 1);
#pragma unroll
        for (int r = 0; r < 2; ++r) nv4_dma(ssrc[r] + (size_t)kb * 128, base + (uint32_t)r * 4096u);
    };
    f32x4_t y[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) y[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    // this wave's fragments: A rows, B row tiles (SILU_MUL: fragments 0, 1 = gate columns, 2, 3 = the same columns of up)
    int arow[4], btile[4];
    uint32_t bad[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 4; ++i) arow[i] = wr * 64 + i * 16 + m16;
#pragma unroll
    for (int j = 0; j < 4; ++j) btile[j] = silu ? ((j >> 1) * 4 + wc * 2 + (j & 1)) : (wc * 4 + j);

    stage_a(0, 0);
    stage_b(0, 0);
    stage_s(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int kb = 0; kb < nkb; ++kb) {
        const uint8_t* B = ng_lds + NG_B_OFF + (size_t)(kb & 1) * NG_B_BYTES;
        const uint8_t* S = ng_lds + NG_S_OFF + (size_t)((kb >> 3) & 1) * NG_S_BYTES + (size_t)(kb & 7) * 128 + (kg >> 1) * 64 + m16 * 4;
        uint32_t s4[4];
#pragma unroll
        for (int h = 0; h < 2; ++h) {                                    // K step 2 kb + h: A buffer h
            if (h == 0) {
                stage_a(2 * kb + 1, 1);
                if (kb + 1 < nkb) stage_b(kb + 1, (kb + 1) & 1);
                if ((kb & 7) == 0 && kb + 8 < nkb) stage_s((kb >> 3) + 1, ((kb >> 3) + 1) & 1);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    s4[j] = *reinterpret_cast<const uint32_t*>(S + (size_t)btile[j] * 1024);
                    bad[j] |= nv4_has_nan(s4[j]);
                }
            } else if (kb + 1 < nkb) {
                stage_a(2 * kb + 2, 0);
            }
            const uint8_t* A = ng_lds + (size_t)h * NG_A_BYTES;
            uint2 raw[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) raw[j] = *reinterpret_cast<const uint2*>(B + (size_t)((btile[j] * 64 + lane) * 16 + 8 * h));
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                uint4 af[4], bf[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) af[i] = *reinterpret_cast<const uint4*>(A + (size_t)arow[i] * 128 + (size_t)(((s2 * 4 + kg) ^ (arow[i] & 7)) * 16));
#pragma unroll
                for (int j = 0; j < 4; ++j) bf[j] = nv4_frag_j<DT>(s2 ? raw[j].y : raw[j].x, s4[j], 2 * h + s2);
#pragma unroll
                for (int j = 0; j < 4; ++j)
#pragma unroll
                    for (int i = 0; i < 4; ++i) y[i][j] = nv4_mfma<DT>(af[i], bf[j], y[i][j]);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // the next step has landed (this wave's share of it)
            __syncthreads();                                             // ... everyone's; and everyone is done reading this buffer
        }
    }
    // ---- epilogue: the lane holds tokens 4 kg + v of every m-fragment for column m16 of every n-fragment; it saw the scales of its own
    // half (kg / 2) only, so lanes kg and kg ^ 2 of a column share what they saw
    const float nan = __builtin_nanf("");
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        bad[j] |= (uint32_t)__shfl_xor((int)bad[j], 32);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int t = t0 + wr * 64 + i * 16 + 4 * kg + v;
            if (t >= a.T) continue;
            if (silu) {
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int col = c0 + wc * 32 + j * 16 + m16;
                    if (col < n_cols) nv4_epilogue<DT>(a, t, col, bad[j] ? nan : y[i][j][v], bad[j + 2] ? nan : y[i][j + 2][v]);
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int col = c0 + wc * 64 + j * 16 + m16;
                    if (col < n_cols) nv4_epilogue<DT>(a, t, col, bad[j] ? nan : y[i][j][v], 0.f);
                }
            }
        }
}

// ------------------------------------------------------------------------------------------------ repack
// checkpoint blocks [n][k/2] and scales [n][k/16] -> the two planes of the image: one thread per 16-byte chunk of the block plane (four
// dwords of a row, 32 k apart); the first n * k/64 threads also write one scale dword (one half of a row's eight groups of a k-block)
__global__ void __launch_bounds__(256) nv4_tile_kernel(const uint8_t* __restrict__ in_b, const uint8_t* __restrict__ in_s,
                                                       uint8_t* __restrict__ out_b, uint8_t* __restrict__ out_s, int n, int k) {
    const size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x;                 // chunk index = (tile * nkb + kb) * 64 + lane
    const int nkb = k >> 7;
    if (o >= (size_t)(n >> 4) * nkb * 64) return;
    {
        const int lane = (int)(o & 63);
        const size_t tk = o >> 6;
        const int kb = (int)(tk % nkb), tile = (int)(tk / nkb);
        const uint8_t* src = in_b + (size_t)(tile * 16 + (lane & 15)) * (k >> 1) + kb * 64 + (lane >> 4) * 4;
        uint4 v;
        v.x = *reinterpret_cast<const uint32_t*>(src);
        v.y = *reinterpret_cast<const uint32_t*>(src + 16);
        v.z = *reinterpret_cast<const uint32_t*>(src + 32);
        v.w = *reinterpret_cast<const uint32_t*>(src + 48);
        *reinterpret_cast<uint4*>(out_b + o * 16) = v;
    }
    if (o < (size_t)n * nkb * 2) {                                                  // scale dword index = ((tile * nkb + kb) * 2 + half) * 16 + row
        const int row = (int)(o & 15), half = (int)((o >> 4) & 1);
        const size_t tk = o >> 5;
        const int kb = (int)(tk % nkb), tile = (int)(tk / nkb);
        const uint2 g8 = *reinterpret_cast<const uint2*>(in_s + ((size_t)(tile * 16 + row) * nkb + kb) * 8);      // groups 0..7 of the k-block
        // groups half, half + 2, half + 4, half + 6: the even (odd) bytes of the eight
        *reinterpret_cast<uint32_t*>(out_s + o * 4) = half ? __builtin_amdgcn_perm(g8.y, g8.x, 0x07050301u) : __builtin_amdgcn_perm(g8.y, g8.x, 0x06040200u);
    }
}

#ifndef NVFP4_GEMM_MIN_T
#define NVFP4_GEMM_MIN_T 33            // tokens from which a launch takes the MFMA GEMM (below: two M tiles of the streaming kernel)
#endif
static_assert(NVFP4_GEMM_MIN_T >= 2 && NVFP4_GEMM_MIN_T <= 33, "the streaming kernel has at most two M tiles");

template <int DT>
static int nvfp4_small_launch(const Nv4Args& a, hipStream_t st) {
    const int nkb = a.K >> 7, niter = (nkb + NS_NW - 1) / NS_NW;
    int G = (NS_X_BYTES / a.T - 16) / (NS_NW * 256);                   // k-blocks per wave and staging pass
    G = G < 1 ? 1 : (G > niter ? niter : G);
    const bool pair = a.epi == MI355_EPI_SILU_MUL;
    const int mt = a.T <= 16 ? 1 : 2;
    const size_t xb = (size_t)a.T * (G * NS_NW * 256 + 16), rb = (size_t)NS_NW * (pair ? 2 : 1) * mt * 256 * 4;
    const size_t lds = xb > rb ? xb : rb;
    const dim3 grid((pair ? a.pair_offset : a.N) / 16), block(64 * NS_NW);
#define NS_GO(MT_, R_) do { \
        static Mi355DevOnce attr_; \
        if (!attr_.done()) { (void)hipFuncSetAttribute((const void*)nvfp4_small_kernel<DT, MT_, R_>, hipFuncAttributeMaxDynamicSharedMemorySize, NS_X_BYTES); attr_.set(); } \
        hipLaunchKernelGGL((nvfp4_small_kernel<DT, MT_, R_>), grid, block, lds, st, a, G); \
    } while (0)
    if (mt == 1) { if (pair) NS_GO(1, 2); else NS_GO(1, 1); }
    else { if (pair) NS_GO(2, 2); else NS_GO(2, 1); }
#undef NS_GO
    return (int)hipGetLastError();
}
template <int DT>
static int nvfp4_gemm_launch(const Nv4Args& a, hipStream_t st) {
    static Mi355DevOnce attr;
    if (!attr.done()) {
        (void)hipFuncSetAttribute((const void*)nvfp4_gemm_kernel<DT>, hipFuncAttributeMaxDynamicSharedMemorySize, NG_LDS);
        attr.set();
    }
    const bool pair = a.epi == MI355_EPI_SILU_MUL;
    const int n_cols = pair ? a.pair_offset : a.N, per = pair ? 64 : 128;
    hipLaunchKernelGGL((nvfp4_gemm_kernel<DT>), dim3((a.T + 127) / 128, (n_cols + per - 1) / per), dim3(256), NG_LDS, st, a);
    return (int)hipGetLastError();
}
// Route: the shape of mxfp4_run.  Up to 32 tokens the streaming kernel.  Above, the GEMM -- when its grid has at least NVFP4_GEMM_MIN_WGS
// workgroups or the launch has more than NVFP4_CHUNK_MAX_T tokens; a few-tile launch below that (down: 32 column tiles) runs as 32-token
// chunks of the streaming kernel.  NVFP4_GEMM_MIN_T and NVFP4_GEMM_MIN_WGS are build-time switches for measuring the edges both ways
// (DESIGN.md 5e).
#ifndef NVFP4_GEMM_MIN_WGS
#define NVFP4_GEMM_MIN_WGS 128
#endif
#define NVFP4_CHUNK_MAX_T 96
template <int DT>
static int nvfp4_run(const Nv4Args& a, hipStream_t st) {
    if (a.T < NVFP4_GEMM_MIN_T) return nvfp4_small_launch<DT>(a, st);
    const bool pair = a.epi == MI355_EPI_SILU_MUL;
    const int n_cols = pair ? a.pair_offset : a.N, per = pair ? 64 : 128;
    const int64_t wgs = (int64_t)((a.T + 127) / 128) * ((n_cols + per - 1) / per);
    if (a.T > NVFP4_CHUNK_MAX_T || wgs >= NVFP4_GEMM_MIN_WGS) return nvfp4_gemm_launch<DT>(a, st);
    for (int t0 = 0; t0 < a.T; t0 += NVFP4_GEMM_MIN_T - 1) {
        Nv4Args c = a;
        c.T = a.T - t0 < NVFP4_GEMM_MIN_T - 1 ? a.T - t0 : NVFP4_GEMM_MIN_T - 1;
        c.x = static_cast<const uint16_t*>(a.x) + (size_t)t0 * a.K;
        c.out = static_cast<uint16_t*>(a.out) + (size_t)t0 * a.ldo;
        if (a.resid) c.resid = static_cast<const uint16_t*>(a.resid) + (size_t)t0 * a.ldo;
        const int rc = nvfp4_small_launch<DT>(c, st);
        if (rc) return rc;
    }
    return 0;
}

extern "C" {

int mi355_nvfp4_tile_repack(const void* in_blocks, const void* in_scales, void* out_tiles, void* out_scales, int32_t n, int32_t k, int64_t stream) {
    if (!in_blocks || !in_scales || !out_tiles || !out_scales || in_blocks == out_tiles || in_scales == out_scales) return (int)hipErrorInvalidValue;
    if (n <= 0 || k <= 0 || (n & 15) || (k & 127)) return (int)hipErrorInvalidValue;
    if (((uintptr_t)in_blocks & 3) || ((uintptr_t)in_scales & 7) || ((uintptr_t)out_tiles & 15) || ((uintptr_t)out_scales & 3)) return (int)hipErrorInvalidValue;
    const size_t chunks = (size_t)n * k / 32;
    hipLaunchKernelGGL(nv4_tile_kernel, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const uint8_t*>(in_blocks), static_cast<const uint8_t*>(in_scales), static_cast<uint8_t*>(out_tiles),
                       static_cast<uint8_t*>(out_scales), n, k);
    return (int)hipGetLastError();
}

int mi355_nvfp4_linear_tiled(void* out, const void* x, const void* w_tiled, const void* s_tiled, const void* bias, const void* residual,
                             int32_t num_tokens, int32_t n, int32_t k, int32_t group, float global_scale, float global_scale_up,
                             int32_t dtype, int32_t epilogue, int64_t stream) {
    if (!out || !x || !w_tiled || !s_tiled || num_tokens < 1 || n <= 0 || k <= 0) return (int)hipErrorInvalidValue;
    if (((uintptr_t)x & 15) || ((uintptr_t)w_tiled & 15) || ((uintptr_t)s_tiled & 15)) return (int)hipErrorInvalidValue;
    if (epilogue != MI355_EPI_STORE && epilogue != MI355_EPI_RESID && epilogue != MI355_EPI_SILU_MUL) return (int)hipErrorInvalidValue;
    if (epilogue == MI355_EPI_RESID && !residual) return (int)hipErrorInvalidValue;
    if (group != 16 || (k & 127) || (n & 15)) return (int)hipErrorNotSupported;
    if (epilogue == MI355_EPI_SILU_MUL && (n & 31)) return (int)hipErrorNotSupported;        // gate and up are whole 16-row tiles
    if (dtype != MI355_DTYPE_BF16 && dtype != MI355_DTYPE_F16) return (int)hipErrorNotSupported;
    Nv4Args a{};
    a.w = static_cast<const uint8_t*>(w_tiled); a.s = static_cast<const uint8_t*>(s_tiled); a.x = x; a.out = out; a.bias = bias; a.resid = residual;
    a.T = num_tokens; a.N = n; a.K = k; a.epi = epilogue; a.g = global_scale; a.g_up = global_scale_up;
    if (epilogue == MI355_EPI_SILU_MUL) { a.pair_offset = n / 2; a.ldo = n / 2; } else a.ldo = n;
    return dtype == MI355_DTYPE_BF16 ? nvfp4_run<MI355_DTYPE_BF16>(a, (hipStream_t)stream) : nvfp4_run<MI355_DTYPE_F16>(a, (hipStream_t)stream);
}

}  // extern "C"
