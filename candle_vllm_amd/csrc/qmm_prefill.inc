// Prompt-step quantised GEMM, hand-written (included by qmatmul.hip; shares QmmArgs, the tile layout and the epilogue).
//
// Reference: `QMatMul::forward` serves prompt steps too -- src/openai/models/linear.rs:36-61,765-806, chunks of up to 8192
// tokens (src/openai/pipelines/llm_engine.rs:95).  candle's GPU path dequantises to f16 and calls the vendor GEMM [EXT]; the
// first version here did the same through rocBLAS with a bf16 hi/lo weight image in HBM.  This kernel keeps the weights
// QUANTISED in HBM and unpacks them in registers on the way into the matrix cores:
//   * Q4_K: w = d*sc_j*q - dmin*m_j.  The B operand is the f16 value sc_j*q (an integer <= 63*15 = 945 < 2048: EXACT in
//     f16; built as fma(f16(1024+q), sc_j, -1024*sc_j) from the "0x6400 | q" code trick), so the eight 32-wide sub-blocks of
//     a 256-k super-block chain in ONE accumulator and the f16 super-block scale d is applied once per k-block in f32.
//     The minimum term is one small MFMA per k-block against the staged sub-block sums of the activations.
//   * Q6_K: w = d*sc_s*(q-32), |sc_s*(q-32)| <= 4096 is NOT exact in f16 -> sc = 2*(sc>>1) + (sc&1): two exact operands
//     ((sc>>1)*(q-32) <= 2048 and (sc&1)*(q-32)), two MFMAs per sub-block pair, acc = 2*acc_a + acc_b.
//   * activations stay f32-accurate: x/rs = hi + lo (two f16, 22 bits; rs = per-token power of two that keeps |x/rs| <= 1024,
//     re-applied in the epilogue), hi and lo are separate MFMA passes over the same B fragments: issued flops = 2 x useful.
//   * the repacked tile's lane order (kgroup*16 + row) IS the B-fragment lane order of v_mfma_f32_16x16x32_f16, so weights
//     go HBM -> registers -> MFMA with no LDS round trip; LDS holds only the activation tile (swizzled 16-B slots: the
//     16 rows of an A fragment hit 8 distinct bank quads per half-wave).
//   * workgroup = 8 waves as 4 (M) x 2 (N), tile 128 tokens x 128 rows, wave tile 32 x 64; K walks in chunks of 64.
// Output: f32 C[T][ldp] in the concatenated padded row space, consumed by qmm_epilogue_kernel (bias / residual / SiLU*mul /
// RoPE + cache scatter) with the per-token scale rs.
typedef _Float16 qpg_h2 __attribute__((ext_vector_type(2)));
typedef _Float16 qpg_h4 __attribute__((ext_vector_type(4)));
typedef _Float16 qpg_h8 __attribute__((ext_vector_type(8)));
typedef unsigned int qpg_u32x2 __attribute__((ext_vector_type(2)));

#define QPG_BM 128
#define QPG_BN 128
#define QPG_ROWB 128                 // bytes of one token row of one chunk: 64 k x f16

struct QpgImg {
    uint8_t* xa;                     // [K/64][parts: hi (, lo)][Tpad][128 B] f16, 16-B slot c of row t stored at c ^ (t & 7)
    uint8_t* sfrag;                  // [K/256][Tpad][32 B]: S_hi[8 sub-blocks], S_lo[8] as f16 (sums of hi+lo of the scaled x)
    float* row_scale;                // [Tpad] power of two rs (x = rs * (hi + lo))
    float* row_inv;                  // [Tpad] 1/rms of the token (1 when no norm is fused)
    int Tpad;
    int parts;                       // 1 = one f16 plane (11 bits per activation: ~1e-4 per mat-mul, default), 2 = hi + lo (22 bits, exact mode)
};

// ---- per-token statistics -- 1/rms (fused RMSNorm) and the power-of-two scale that keeps the f16 image in range -- and the image, in ONE
// launch, workgroup = token (rounds 2-4 took two: `qpg_rowstat_kernel` per token, `qpg_prep_kernel` per (k-block, 8 tokens); one box,
// alternated, Llama-3-8B prompt step: T = 512 21.6 k -> 22.6 k tok/s, T = 2048 36.8 k -> 37.3 k, T = 4096 34.2 k -> 34.7 k).
// The statistics pass leaves the token's row (16-57 KB) in L2, the image pass reads it again from there.  Thread i handles the 8 values
// k = 2048 r + 8 i .. + 7 of round r: 32 consecutive threads = one k-block; element order inside an 8-group = {0,2,1,3,4,6,5,7} (what
// "(bytes & 0x000F000F) | 0x64006400" makes of the weights); the sub-block sums (32 k = 4 consecutive 8-groups, as f16 hi + lo, of the
// planes the GEMM multiplies) meet in groups of four lanes.
__global__ void __launch_bounds__(256) qpg_rowprep_kernel(const QmmArgs a, QpgImg im) {
    __shared__ float red[16];
    __shared__ float s_f;
    const int t = blockIdx.x;
    const int El = threadIdx.x & 31;
    const bool live = t < a.B;
    auto load8 = [&](int k, float (&v)[8]) {
        if (a.x_dtype == MI355_DTYPE_BF16) {
            const uint4 w = *reinterpret_cast<const uint4*>(static_cast<const uint16_t*>(a.x) + (size_t)t * a.ldx + k);
            v[0] = bf16lo_to_f32(w.x); v[1] = bf16hi_to_f32(w.x); v[2] = bf16lo_to_f32(w.y); v[3] = bf16hi_to_f32(w.y);
            v[4] = bf16lo_to_f32(w.z); v[5] = bf16hi_to_f32(w.z); v[6] = bf16lo_to_f32(w.w); v[7] = bf16hi_to_f32(w.w);
        } else {
            const float* xp = static_cast<const float*>(a.x) + (size_t)t * a.ldx + k;
            const float4 v0 = *reinterpret_cast<const float4*>(xp), v1 = *reinterpret_cast<const float4*>(xp + 4);
            v[0] = v0.x; v[1] = v0.y; v[2] = v0.z; v[3] = v0.w; v[4] = v1.x; v[5] = v1.y; v[6] = v1.z; v[7] = v1.w;
        }
    };
    // round 6: the row's values (x * norm weight) stay in REGISTERS between the statistics pass and the image pass (K <= 16384: at most 8
    // rounds of 8 values per thread) -- the second pass used to read the row again from L2, one more dependent round trip in a launch
    // whose 2048 small workgroups are nothing but their latency chain
#ifndef QPG_ROWPREP_KEEP
#define QPG_ROWPREP_KEEP 1          // A/B builds: 0 = the image pass re-reads the row (rounds 4-5)
#endif
    constexpr int KEEP_R = QPG_ROWPREP_KEEP ? 8 : 0;
    float keep[KEEP_R ? KEEP_R : 1][8];
    float ss = 0.f, amax = 0.f;
    if (live) {
#pragma unroll
        for (int r = 0; r < KEEP_R; ++r) {
            const int k = (int)threadIdx.x * 8 + r * 2048;
            if (k < a.K) {
                float v[8];
                load8(k, v);
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    ss += v[i] * v[i];
                    const float w = a.norm_w ? v[i] * a.norm_w[k + i] : v[i];
                    amax = fmaxf(amax, fabsf(w));
                    keep[r][i] = w;
                }
            }
        }
        for (int k = (int)threadIdx.x * 8 + KEEP_R * 2048; k < a.K; k += 2048) {       // (rows longer than the register budget: statistics only)
            float v[8];
            load8(k, v);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                ss += v[i] * v[i];
                amax = fmaxf(amax, fabsf(a.norm_w ? v[i] * a.norm_w[k + i] : v[i]));
            }
        }
    }
    ss = block_sum(ss, red);
    __syncthreads();
    amax = wave_max(amax);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = amax;
    __syncthreads();
    if (threadIdx.x == 0) {
        amax = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
        const float inv = a.norm_w ? rsqrtf(ss / (float)a.K + a.eps) : 1.f;
        amax *= inv;
        float rs = 1.f;
        while (amax > 1024.f * rs && rs < 1e30f) rs *= 2.f;          // |x / rs| <= 1024: a sub-block sum stays below 65504
        im.row_scale[t] = rs;
        im.row_inv[t] = inv;
        s_f = inv / rs;
    }
    __syncthreads();
    const float f = s_f;
    constexpr int ORD[8] = {0, 2, 1, 3, 4, 6, 5, 7};
    // (the image holds (x * w) * f -- the kept product times the row factor -- in the register path and in the re-load path alike)
#pragma unroll
    for (int r = 0; r < KEEP_R + 1; ++r) {
      for (int k = (int)threadIdx.x * 8 + r * 2048; k < a.K; k += (r < KEEP_R ? a.K : 2048)) {     // r < KEEP_R: exactly one trip; r == KEEP_R: the tail loop
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = 0.f;
        if (live) {
            if (r < KEEP_R) {
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = keep[r < KEEP_R ? r : 0][i] * f;
            } else {
                load8(k, v);
#pragma unroll
                for (int i = 0; i < 8; ++i) v[i] = (a.norm_w ? v[i] * a.norm_w[k + i] : v[i]) * f;
            }
        }
        qpg_h8 hi, lo;
        float sum = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float x = v[ORD[i]];
            const _Float16 h = (_Float16)x;
            const _Float16 l = (_Float16)(x - (float)h);
            hi[i] = h; lo[i] = l;
            sum += (im.parts == 2) ? (float)h + (float)l : (float)h;
        }
        const int kb = k >> 8, kc = k >> 6, c = (k & 63) >> 3;
        const size_t row = ((size_t)(kc * im.parts) * im.Tpad + t) * QPG_ROWB + (size_t)((c ^ (t & 7)) * 16);
        *reinterpret_cast<qpg_h8*>(im.xa + row) = hi;
        if (im.parts == 2) *reinterpret_cast<qpg_h8*>(im.xa + row + (size_t)im.Tpad * QPG_ROWB) = lo;
        sum += __shfl_xor(sum, 1, 64);
        sum += __shfl_xor(sum, 2, 64);
        if ((El & 3) == 0) {
            const int j = El >> 2;
            const _Float16 sh = (_Float16)sum;
            const _Float16 sl = (_Float16)(sum - (float)sh);
            _Float16* sp = reinterpret_cast<_Float16*>(im.sfrag + ((size_t)kb * im.Tpad + t) * 32);
            sp[j] = sh;
            sp[8 + j] = sl;
        }
      }
    }
}

// ---- B fragment of one 32-wide sub-block of one row tile, straight from the tile's registers.
// `w0,w1` = the lane's 8 bytes of the 64-k group (low nibbles = even sub-block, high nibbles = odd one, `hi` selects);
// M = 0x000F000F and C = 0x64006400 (f16 1024.0 twice) live in VGPRs so that "(w >> s) & M | C" is ONE v_and_or_b32.
__device__ __forceinline__ qpg_h8 qpg_frag_q4k(uint32_t w0, uint32_t w1, const int hi, const uint32_t sc, const uint32_t M, const uint32_t C) {
    // (s, s) as f16 from the 6-bit scale: 1024 + s is 0x6400 | s, minus 1024 in one packed add; offset = -1024 * s
    const qpg_h2 K1024 = {(_Float16)1024.f, (_Float16)1024.f};
    const qpg_h2 S = __builtin_bit_cast(qpg_h2, (sc | (sc << 16)) | C) - K1024;
    const qpg_h2 OFF = S * qpg_h2{(_Float16)(-1024.f), (_Float16)(-1024.f)};
    const int sh = hi ? 4 : 0;
    const qpg_h2 a02 = __builtin_bit_cast(qpg_h2, ((w0 >> sh) & M) | C);          // elements (0,2) of the word's 4 bytes
    const qpg_h2 a13 = __builtin_bit_cast(qpg_h2, ((w0 >> (sh + 8)) & M) | C);    // elements (1,3)
    const qpg_h2 b02 = __builtin_bit_cast(qpg_h2, ((w1 >> sh) & M) | C);
    const qpg_h2 b13 = __builtin_bit_cast(qpg_h2, ((w1 >> (sh + 8)) & M) | C);
    const qpg_h2 r0 = __builtin_elementwise_fma(a02, S, OFF), r1 = __builtin_elementwise_fma(a13, S, OFF);
    const qpg_h2 r2 = __builtin_elementwise_fma(b02, S, OFF), r3 = __builtin_elementwise_fma(b13, S, OFF);
    return qpg_h8{r0[0], r0[1], r1[0], r1[1], r2[0], r2[1], r3[0], r3[1]};
}

// The same B fragment from prepared operands (round 4, the LDS-fed kernel): `sp` / `op` = the sub-block's scale s and offset as f16 pairs
// of TWO sub-blocks (element e is this one's), `w0s, w1s` = the words shifted down by 8 once per chunk, `mk` = 0x000F000F for the low
// nibbles (s, -1024 s) or 0x00F000F0 for the high ones, taken where they stand: 0x6400 | (q << 4) = 1024 + 16 q and
// s q = fma(1024 + 16 q, s / 16, -64 s) -- s / 16 is exact and the fma rounds once: the same bits as the shifted form, two shifts per
// chunk and row tile instead of six, and the scale conversion once per k-block for four sub-blocks at a time.
__device__ __forceinline__ qpg_h8 qpg_frag_q4k_p(uint32_t w0, uint32_t w0s, uint32_t w1, uint32_t w1s, const qpg_h2 sp, const qpg_h2 op, const int e,
                                                 const uint32_t mk, const uint32_t C) {
    const qpg_h2 S = e ? __builtin_shufflevector(sp, sp, 1, 1) : __builtin_shufflevector(sp, sp, 0, 0);
    const qpg_h2 OFF = e ? __builtin_shufflevector(op, op, 1, 1) : __builtin_shufflevector(op, op, 0, 0);
    const qpg_h2 r0 = __builtin_elementwise_fma(__builtin_bit_cast(qpg_h2, (w0 & mk) | C), S, OFF);
    const qpg_h2 r1 = __builtin_elementwise_fma(__builtin_bit_cast(qpg_h2, (w0s & mk) | C), S, OFF);
    const qpg_h2 r2 = __builtin_elementwise_fma(__builtin_bit_cast(qpg_h2, (w1 & mk) | C), S, OFF);
    const qpg_h2 r3 = __builtin_elementwise_fma(__builtin_bit_cast(qpg_h2, (w1s & mk) | C), S, OFF);
    return qpg_h8{r0[0], r0[1], r1[0], r1[1], r2[0], r2[1], r3[0], r3[1]};
}

// ---- Q5_K (tile: mi355_qweight_repack): the Q4_K nibble planes plus the lane's 64 fifth bits, transposed so that the fifth bits of the
// element pair (c, c + 2) of sub-block j sit at bits n and n + 16 of a word, n = 2j + c: ONE shift and ONE AND with `mask` = (1 << pos) twice
// put them at bit `pos` of both 16-bit halves of an operand dword.
__device__ __forceinline__ uint32_t qpg_q5k_hbits(uint32_t h, const int n, const int pos, const uint32_t mask) {
    return (n >= pos ? (h >> (n - pos)) : (h << (pos - n))) & mask;
}

// B fragment of sub-block j of a Q5_K tile for the register-fed kernel, as qpg_frag_q4k: code 0x6400 | nibble | fifth bit << 4 = 1024 + q
// (q <= 31), fma(1024 + q, s, -1024 s) = s q <= 63 * 31 = 1953 < 2048: an exact f16 integer.  `h0, h1` = the lane's fifth-bit words
// (elements 0..3 / 4..7), B = 0x00100010 in a VGPR.
__device__ __forceinline__ qpg_h8 qpg_frag_q5k(uint32_t w0, uint32_t w1, uint32_t h0, uint32_t h1, const int j, const uint32_t sc, const uint32_t M,
                                               const uint32_t B, const uint32_t C) {
    const qpg_h2 K1024 = {(_Float16)1024.f, (_Float16)1024.f};
    const qpg_h2 S = __builtin_bit_cast(qpg_h2, (sc | (sc << 16)) | C) - K1024;
    const qpg_h2 OFF = S * qpg_h2{(_Float16)(-1024.f), (_Float16)(-1024.f)};
    const int sh = (j & 1) ? 4 : 0;
    const qpg_h2 a02 = __builtin_bit_cast(qpg_h2, ((w0 >> sh) & M) | (qpg_q5k_hbits(h0, 2 * j, 4, B) | C));
    const qpg_h2 a13 = __builtin_bit_cast(qpg_h2, ((w0 >> (sh + 8)) & M) | (qpg_q5k_hbits(h0, 2 * j + 1, 4, B) | C));
    const qpg_h2 b02 = __builtin_bit_cast(qpg_h2, ((w1 >> sh) & M) | (qpg_q5k_hbits(h1, 2 * j, 4, B) | C));
    const qpg_h2 b13 = __builtin_bit_cast(qpg_h2, ((w1 >> (sh + 8)) & M) | (qpg_q5k_hbits(h1, 2 * j + 1, 4, B) | C));
    const qpg_h2 r0 = __builtin_elementwise_fma(a02, S, OFF), r1 = __builtin_elementwise_fma(a13, S, OFF);
    const qpg_h2 r2 = __builtin_elementwise_fma(b02, S, OFF), r3 = __builtin_elementwise_fma(b13, S, OFF);
    return qpg_h8{r0[0], r0[1], r1[0], r1[1], r2[0], r2[1], r3[0], r3[1]};
}

// The same for the LDS-fed kernel, nibbles taken where they stand as in qpg_frag_q4k_p.  Low nibbles (j even): 0x6400 | nibble | fifth bit
// << 4 = 1024 + q, offset -1024 s.  High nibbles (j odd): the fifth bit goes to bit 8 of each half and the exponent pattern is 0x5400
// (64.0, whose mantissa ulp is 1/16): 0x5400 | nibble << 4 | bit << 8 = 64 + q, offset -64 s -- the SAME scale operand s serves both, and
// (64 + q) s - 64 s = s q <= 1953 is exact behind the fma's single rounding.  `mk` / `bk` / `C` = 0x000F000F / 0x00100010 / 0x64006400
// (j even) or 0x00F000F0 / 0x01000100 / 0x54005400 (j odd): masks in SGPRs, `C` in a VGPR.  The offset is one packed multiply per fragment: the Q4_K arm keeps
// s, s / 16 and both offsets of every sub-block in 32 registers, which next to the fifth-bit words would cost the fourth wave per SIMD.
__device__ __forceinline__ qpg_h8 qpg_frag_q5k_p(uint32_t w0, uint32_t w0s, uint32_t w1, uint32_t w1s, uint32_t h0, uint32_t h1, const int j,
                                                 const qpg_h2 sp, const int e, const uint32_t mk, const uint32_t bk, const uint32_t C) {
    const qpg_h2 S = e ? __builtin_shufflevector(sp, sp, 1, 1) : __builtin_shufflevector(sp, sp, 0, 0);
    const _Float16 ko = (j & 1) ? (_Float16)(-64.f) : (_Float16)(-1024.f);
    const qpg_h2 OFF = S * qpg_h2{ko, ko};
    const int pos = (j & 1) ? 8 : 4;
    const qpg_h2 r0 = __builtin_elementwise_fma(__builtin_bit_cast(qpg_h2, (w0 & mk) | (qpg_q5k_hbits(h0, 2 * j, pos, bk) | C)), S, OFF);
    const qpg_h2 r1 = __builtin_elementwise_fma(__builtin_bit_cast(qpg_h2, (w0s & mk) | (qpg_q5k_hbits(h0, 2 * j + 1, pos, bk) | C)), S, OFF);
    const qpg_h2 r2 = __builtin_elementwise_fma(__builtin_bit_cast(qpg_h2, (w1 & mk) | (qpg_q5k_hbits(h1, 2 * j, pos, bk) | C)), S, OFF);
    const qpg_h2 r3 = __builtin_elementwise_fma(__builtin_bit_cast(qpg_h2, (w1s & mk) | (qpg_q5k_hbits(h1, 2 * j + 1, pos, bk) | C)), S, OFF);
    return qpg_h8{r0[0], r0[1], r1[0], r1[1], r2[0], r2[1], r3[0], r3[1]};
}

// Workgroup = 4 waves as 2 (M) x 2 (N), one wave per SIMD with the whole 512-register file (the 8-wave version of this
// kernel spilled its activation prefetch at 256 VGPRs and sat at 15 % MFMA-busy): wave tile 64 tokens x 64 rows.
// Register plan: y 64 + acc 64 (per-k-block accumulators), quantised tiles 64 (header, next header, plane 0, plane 1 of
// the four row tiles -- a plane is re-loaded with the NEXT k-block's bytes as soon as its last sub-block is unpacked:
// >= 2 chunks in flight), B fragments 16, A fragments 32 (one 32-k half at a time, all eight reads issued before the first
// MFMA), activation staging 64 (two chunks ahead).  Each row tile is unpacked by the two waves that share it.
// Wave tile = MTW m-tiles x NTW row tiles, WM x WN waves: workgroup tile (16 MTW WM) tokens x (16 NTW WN) rows.  What bounds
// the kernel is the ACTIVATION operand (measured by ablation: without the image loads the step is 36 % shorter, without the
// MFMAs or the unpack it is not shorter at all): a wider workgroup tile in N re-reads the image less often, a wider wave
// tile in N reads each A fragment from LDS less often.
// The register-fed form: since round 4 it runs only for hi + lo activation planes ("exact" activations, PARTS = 2); one plane takes
// qpg_gemm_lds2_kernel below.  WT = MI355_GGML_Q5_K: tile stride Q5K_TILE, the lane's two fifth-bit words travel with the headers (one
// k-block ahead), qpg_frag_q5k builds the fragment (hipcc, gfx950, -O3, <Q5_K, 4, 2, 1, 8, 2>: 218 VGPRs and the Q4_K instantiation's 48 B of scratch).
template <int WT, int MTW, int NTW, int WM, int WN, int PARTS>
__global__ void __launch_bounds__(WM * WN * 64, 1) qpg_gemm_kernel(const QmmArgs a, const QpgImg im, float* __restrict__ C, const int ldc,
                                                          const int n_slots, const int slot_base) {
    static_assert(WT == MI355_GGML_Q4_K || WT == MI355_GGML_Q5_K, "Q6_K goes through qpg_gemm_q6k_kernel");
    constexpr bool Q5 = WT == MI355_GGML_Q5_K;
    constexpr int TILEB = Q5 ? Q5K_TILE : Q4K_TILE;
    extern __shared__ __attribute__((aligned(1024))) uint8_t smem[];  // A tile: [2 buffers][2 parts][128 rows][128 B]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int NTHR = WM * WN * 64, BMk = 16 * MTW * WM, SLOTS = NTW * WN;   // threads, token rows and row tiles per workgroup
    constexpr int PARTB = BMk * QPG_ROWB, BUFB = PARTS * PARTB;       // bytes of one part (hi or lo) / of one LDS buffer of a chunk
    constexpr int XU = (BUFB / 16 + NTHR - 1) / NTHR, WMR = 16 * MTW; // 16-B pieces per thread and chunk (the last round may be partial), token rows per wave
    constexpr bool XFULL = XU * 16 * NTHR == BUFB;
    const int wm = wave / WN, wn = wave % WN;
    const int n16 = lane & 15, kg = lane >> 4;
    const int nkb = a.K >> 8, nchunk = a.K >> 6;
    // grid order (launcher): x = token blocks (fastest), y = row blocks -- the workgroups that run together share their WEIGHT
    // tiles (each XCD's L2 fetches a tile once for its m-blocks) and sweep the activation image, which the Infinity Cache holds
    const int bx = blockIdx.y, by = blockIdx.x;                      // bx: row block, by: token block
    const int t0 = by * BMk;

    // ---- this wave's four row tiles (slots in the concatenated segment space)
    const uint8_t* wbase[NTW];
    bool have[NTW];
#pragma unroll
    for (int i = 0; i < NTW; ++i) {
        int slot = bx * SLOTS + wn * NTW + i;
        have[i] = slot < n_slots;
        if (!have[i]) slot = 0;
        int t = slot, sg = 0;
        while (sg + 1 < a.nseg && t >= a.seg[sg].n_tiles) { t -= a.seg[sg].n_tiles; ++sg; }
        wbase[i] = a.seg[sg].w + (size_t)t * nkb * TILEB;
    }
    uint4 hdr[NTW], hdrn[NTW], p0[NTW], p1[NTW];
    qpg_u32x2 hq[NTW], hqn[NTW];                                      // Q5_K: fifth-bit words of this / the next k-block
    auto ld_hdr = [&](int kb, uint4 (&H)[NTW], qpg_u32x2 (&Q)[NTW]) {
#pragma unroll
        for (int i = 0; i < NTW; ++i) {
            H[i] = ld_nt16(reinterpret_cast<const uint4*>(wbase[i] + (size_t)kb * TILEB) + n16);
            if constexpr (Q5) Q[i] = __builtin_nontemporal_load(reinterpret_cast<const qpg_u32x2*>(wbase[i] + (size_t)kb * TILEB + 2304) + lane);
        }
    };
    auto ld_plane = [&](int kb, int p, uint4 (&P)[NTW]) {
#pragma unroll
        for (int i = 0; i < NTW; ++i) P[i] = ld_nt16(reinterpret_cast<const uint4*>(wbase[i] + (size_t)kb * TILEB) + 16 + 64 * p + lane);
    };
    // ---- activation tile: global image (already in LDS order) -> registers -> LDS; 32 KB per chunk = 4 x 16 B per thread
    const size_t part_stride = (size_t)im.Tpad * QPG_ROWB;
    auto x_load = [&](int kc, uint4 (&r)[XU]) {
        const uint8_t* src = im.xa + ((size_t)(kc * PARTS) * im.Tpad + t0) * QPG_ROWB;
#pragma unroll
        for (int u = 0; u < XU; ++u) {
            const int off = (u * NTHR + threadIdx.x) * 16;            // 0 .. BUFB: part = off / PARTB
            if (XFULL || off < BUFB) r[u] = *reinterpret_cast<const uint4*>(src + (size_t)(off / PARTB) * part_stride + (off % PARTB));
        }
    };
    auto x_store = [&](int buf, const uint4 (&r)[XU]) {
#pragma unroll
        for (int u = 0; u < XU; ++u) {
            const int off = (u * NTHR + threadIdx.x) * 16;
            if (XFULL || off < BUFB) *reinterpret_cast<uint4*>(smem + (size_t)buf * BUFB + (size_t)off) = r[u];
        }
    };

    f32x4_t y[MTW][NTW], acc[MTW][NTW];
#pragma unroll
    for (int mt = 0; mt < MTW; ++mt)
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) { y[mt][nt] = f32x4_t{0.f, 0.f, 0.f, 0.f}; acc[mt][nt] = f32x4_t{0.f, 0.f, 0.f, 0.f}; }
    uint32_t Mk = 0x000F000Fu, Ck = 0x64006400u;
    asm volatile("" : "+v"(Mk), "+v"(Ck));
    uint32_t Bk = 0x00100010u;
    if constexpr (Q5) asm volatile("" : "+v"(Bk));

    uint4 xa_[XU];                                                      // activation chunk kc+1 in flight
    ld_hdr(0, hdr, hq); ld_plane(0, 0, p0); ld_plane(0, 1, p1);
    x_load(0, xa_);
    x_store(0, xa_);
    __syncthreads();

    // LDS buffer of chunk kc = kc & 1.  In chunk kc: chunk kc+1 is requested at the top and goes to the other buffer at the end
    // of kc (that buffer was last read during kc-1).
    for (int kb = 0; kb < nkb; ++kb) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {                                   // compile-time chunk index: every select below is static
        const int kc = 4 * kb + c;
        const int buf = c & 1, buf_next = buf ^ 1;
        const uint8_t* Ab = smem + (size_t)buf * BUFB;
        // (1) this chunk's first-half A fragments leave LDS first: nothing below may delay them
        qpg_h8 af[MTW][PARTS];
        auto a_read = [&](int h) {
#pragma unroll
            for (int mt = 0; mt < MTW; ++mt) {
                const int row = wm * WMR + mt * 16 + n16;
                const int slot = (h * 4 + kg) ^ (row & 7);
#pragma unroll
                for (int p = 0; p < PARTS; ++p)
                    af[mt][p] = *reinterpret_cast<const qpg_h8*>(Ab + (size_t)p * PARTB + (size_t)row * QPG_ROWB + slot * 16);
            }
        };
        a_read(0);
        if (kc + 1 < nchunk) x_load(kc + 1, xa_);                     // one chunk ahead: requested at the top, stored at the bottom
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int j = 2 * c + h;                                  // sub-block of the k-block
            // (2) B fragments of this half for the four row tiles
            qpg_h8 bf[NTW];
#pragma unroll
            for (int nt = 0; nt < NTW; ++nt) {
                const uint4 pl = (c & 2) ? p1[nt] : p0[nt];
                const uint32_t w0 = (c & 1) ? pl.z : pl.x, w1 = (c & 1) ? pl.w : pl.y;
                const uint32_t s0 = hdr[nt].y, s2 = hdr[nt].w;
                const uint32_t scw = (j < 4) ? (s0 & 0x3F3F3F3Fu) : ((s2 & 0x0F0F0F0Fu) | ((s0 >> 2) & 0x30303030u));
                if constexpr (Q5) bf[nt] = qpg_frag_q5k(w0, w1, hq[nt].x, hq[nt].y, j, (scw >> (8 * (j & 3))) & 0xFFu, Mk, Bk, Ck);
                else bf[nt] = qpg_frag_q4k(w0, w1, h, (scw >> (8 * (j & 3))) & 0xFFu, Mk, Ck);
            }
            if (h == 1) {
                // the plane's last sub-block is unpacked: its registers take the NEXT k-block's bytes (>= 2 chunks ahead of use)
                if (c == 1 && kb + 1 < nkb) ld_plane(kb + 1, 0, p0);
                if (c == 3 && kb + 1 < nkb) ld_plane(kb + 1, 1, p1);
                if (c == 2 && kb + 1 < nkb) ld_hdr(kb + 1, hdrn, hqn);
            }
            // (3) MFMAs: the hi (and lo) part of the m-tiles against the four B fragments (independent accumulators per tile pair)
#pragma unroll
            for (int p = 0; p < PARTS; ++p)
#pragma unroll
                for (int mt = 0; mt < MTW; ++mt)
#pragma unroll
                    for (int nt = 0; nt < NTW; ++nt)
                        acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[mt][p], bf[nt], acc[mt][nt], 0, 0, 0);
            if (h == 0) a_read(1);                                    // second half's A fragments: issued behind the first half's MFMAs
        }
        if (c == 3) {
            // ---- end of the k-block: super-block scale d, then the minimum term  - dmin * sum_j m_j S_j
            qpg_h4 sa[MTW];
#pragma unroll
            for (int mt = 0; mt < MTW; ++mt) {
                const int t = t0 + wm * WMR + mt * 16 + n16;
                sa[mt] = *reinterpret_cast<const qpg_h4*>(im.sfrag + ((size_t)kb * im.Tpad + t) * 32 + kg * 8);   // k = 4kg+e: S_hi (kg<2), S_lo
            }
#pragma unroll
            for (int nt = 0; nt < NTW; ++nt) {
                const float d = f16_bits_to_f32((uint16_t)(hdr[nt].x & 0xFFFF));
                const float ndmin = -f16_bits_to_f32((uint16_t)(hdr[nt].x >> 16));
                const uint32_t s1 = hdr[nt].z, s2 = hdr[nt].w;
                const uint32_t mnl = s1 & 0x3F3F3F3Fu, mnh = ((s2 >> 4) & 0x0F0F0F0Fu) | ((s1 >> 2) & 0x30303030u);
                const uint32_t mw = (kg & 1) ? mnh : mnl;             // k = 4kg + e  <->  j = 4(kg & 1) + e
                const qpg_h4 mb = {(_Float16)(float)(mw & 0xFF), (_Float16)(float)((mw >> 8) & 0xFF),
                                   (_Float16)(float)((mw >> 16) & 0xFF), (_Float16)(float)(mw >> 24)};
#pragma unroll
                for (int mt = 0; mt < MTW; ++mt) {
                    const f32x4_t t1 = __builtin_amdgcn_mfma_f32_16x16x16f16(sa[mt], mb, f32x4_t{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        y[mt][nt][v] = fmaf(d, acc[mt][nt][v], fmaf(ndmin, t1[v], y[mt][nt][v]));
                        acc[mt][nt][v] = 0.f;
                    }
                }
            }
#pragma unroll
            for (int nt = 0; nt < NTW; ++nt) { hdr[nt] = hdrn[nt]; hq[nt] = hqn[nt]; }
        }
        if (kc + 1 < nchunk) x_store(buf_next, xa_);
        __syncthreads();                                              // buffer of kc+1 is complete, buffer of kc is free again
      }
    }
    // ---- C[t][slot*16 + n]: lane holds column n16 of its row tiles, rows 4kg+v of its m-tiles
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt) {
        if (!have[nt]) continue;
        const int col = (slot_base + bx * SLOTS + wn * NTW + nt) * 16 + n16;
#pragma unroll
        for (int mt = 0; mt < MTW; ++mt)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int t = t0 + wm * WMR + mt * 16 + 4 * kg + v;
                if (t < a.B) C[(size_t)t * ldc + col] = y[mt][nt][v];
            }
    }
}

// ---- Q6_K.  Tile: sc[16 rows][16 i8] | ql_n0[64 lanes][16 B] | ql_n1 | qh[64][16 B] | d[16 f16]  (see mi355_qweight_repack).
// Lane (kg, row) holds, of every 32-k group G = 4n + tt (n = 128-k half, tt = 0..3), the 4 codes k = 4kg..4kg+3 of its first
// 16-wide sub-block and the 4 codes of its second one: the B fragment of ONE K=32 MFMA if the A operand takes the same 8 k --
// two 8-byte halves of two image slots.  Scale: sc = 2*(sc>>1) + (sc&1), both products with (q-32) exact in f16.
struct Qpg6Tile { uint4 sc, ql0, ql1, qh; uint32_t d; };

__device__ __forceinline__ qpg_h2 qpg_u32_as_h2(uint32_t u) { return __builtin_bit_cast(qpg_h2, u); }

// 8 waves side by side in N, wave tile 32 tokens x 32 rows (two row tiles): workgroup tile 32 x 256 -- like the Q4_K kernel, the
// activation stream is what bounds it, so the workgroup is as wide in N as the registers allow
// MT6 = m-tiles of 16 tokens per wave: 2 = 32 tokens per workgroup (rounds 2-3), 4 = 64 (round 4: every unpacked weight meets 64
// tokens, as the Q4_K kernel's 64 x 256 tile)
template <int PARTS, int MT6 = 2>
__global__ void __launch_bounds__(512, 1) qpg_gemm_q6k_kernel(const QmmArgs a, const QpgImg im, float* __restrict__ C, const int ldc,
                                                              const int n_slots, const int slot_base) {
    extern __shared__ __attribute__((aligned(1024))) uint8_t smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = 0, wn = wave;
    const int n16 = lane & 15, kg = lane >> 4;
    const int nkb = a.K >> 8, nchunk = a.K >> 6;
    constexpr int NT = 2, WGT = 16, BMk = 16 * MT6, PARTB = BMk * QPG_ROWB, BUFB = PARTS * PARTB, XU = (BUFB / 16 + 511) / 512;
    constexpr bool XFULL = XU * 16 * 512 == BUFB;
    const int bx = blockIdx.y, by = blockIdx.x;                      // row block, token block (token blocks fastest: see the Q4_K kernel)
    const int t0 = by * BMk;
    const uint8_t* wbase[NT];
    bool have[NT];
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        int slot = bx * WGT + wn * NT + i;
        have[i] = slot < n_slots;
        if (!have[i]) slot = 0;
        int t = slot, sg = 0;
        while (sg + 1 < a.nseg && t >= a.seg[sg].n_tiles) { t -= a.seg[sg].n_tiles; ++sg; }
        wbase[i] = a.seg[sg].w + (size_t)t * nkb * Q6K_TILE;
    }
    auto load_tiles = [&](int kb, Qpg6Tile (&T)[NT]) {
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const uint8_t* tp = wbase[i] + (size_t)kb * Q6K_TILE;
            const uint4* t4 = reinterpret_cast<const uint4*>(tp);
            T[i].sc = ld_nt16(t4 + n16);
            T[i].ql0 = ld_nt16(t4 + 16 + lane);
            T[i].ql1 = ld_nt16(t4 + 80 + lane);
            T[i].qh = ld_nt16(t4 + 144 + lane);
            T[i].d = __builtin_nontemporal_load(reinterpret_cast<const uint16_t*>(tp + 3328) + n16);
        }
    };
    const size_t part_stride = (size_t)im.Tpad * QPG_ROWB;
    auto x_load = [&](int kc, uint4 (&r)[XU]) {
        const uint8_t* src = im.xa + ((size_t)(kc * PARTS) * im.Tpad + t0) * QPG_ROWB;
#pragma unroll
        for (int u = 0; u < XU; ++u) {
            const int off = (u * 512 + threadIdx.x) * 16;
            if (XFULL || off < BUFB) r[u] = *reinterpret_cast<const uint4*>(src + (size_t)(off / PARTB) * part_stride + (off % PARTB));
        }
    };
    auto x_store = [&](int buf, const uint4 (&r)[XU]) {
#pragma unroll
        for (int u = 0; u < XU; ++u) {
            const int off = (u * 512 + threadIdx.x) * 16;
            if (XFULL || off < BUFB) *reinterpret_cast<uint4*>(smem + (size_t)buf * BUFB + (size_t)off) = r[u];
        }
    };
    f32x4_t y[MT6][NT], acc_a[MT6][NT], acc_b[MT6][NT];
#pragma unroll
    for (int mt = 0; mt < MT6; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            y[mt][nt] = f32x4_t{0.f, 0.f, 0.f, 0.f}; acc_a[mt][nt] = f32x4_t{0.f, 0.f, 0.f, 0.f}; acc_b[mt][nt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        }
    Qpg6Tile cur[NT], nxt[NT];
    uint4 xr[XU];
    load_tiles(0, cur);
    x_load(0, xr);
    x_store(0, xr);
    __syncthreads();
    const qpg_h2 OFF = {(_Float16)(-1056.f), (_Float16)(-1056.f)};   // 0x6400 | code = 1024 + code; code - 32 = that - 1056

    for (int kb = 0; kb < nkb; ++kb) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int kc = 4 * kb + c, buf = c & 1;
        const bool more = kc + 1 < nchunk;
        if (more) x_load(kc + 1, xr);
        if (c == 0 && kb + 1 < nkb) load_tiles(kb + 1, nxt);
        const uint8_t* Ab = smem + (size_t)buf * BUFB;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int G = 2 * c + h, n = G >> 2, tt = G & 3;          // 32-k group of the k-block
            // ---- B fragments (a = (sc>>1)*(q-32), b = (sc&1)*(q-32)) of the two row tiles
            qpg_h8 ba[NT], bb[NT];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const uint4 ql = n ? cur[nt].ql1 : cur[nt].ql0;
                const uint32_t scw[4] = {cur[nt].sc.x, cur[nt].sc.y, cur[nt].sc.z, cur[nt].sc.w};
                qpg_h2 pa[4], pb[4];
#pragma unroll
                for (int is = 0; is < 2; ++is) {
                    const uint32_t qa = is ? ql.z : ql.x, qb = is ? ql.w : ql.y;
                    const uint32_t hq = n ? (is ? cur[nt].qh.w : cur[nt].qh.z) : (is ? cur[nt].qh.y : cur[nt].qh.x);
                    uint32_t t;
                    if (tt == 0) t = (qa & 0x0F0F0F0Fu) | ((hq << 4) & 0x30303030u);
                    else if (tt == 1) t = (qb & 0x0F0F0F0Fu) | ((hq << 2) & 0x30303030u);
                    else if (tt == 2) t = ((qa >> 4) & 0x0F0F0F0Fu) | (hq & 0x30303030u);
                    else t = ((qb >> 4) & 0x0F0F0F0Fu) | ((hq >> 2) & 0x30303030u);
                    const int s = 8 * n + 2 * tt + is;                // 16-wide sub-block
                    const int sc8 = (int)(int8_t)((scw[s >> 2] >> (8 * (s & 3))) & 0xFF);
                    const _Float16 sa = (_Float16)(float)(sc8 >> 1), sb = (_Float16)(float)(sc8 & 1);
                    const qpg_h2 SA = {sa, sa}, SB = {sb, sb};
                    const qpg_h2 c02 = qpg_u32_as_h2((t & 0x00FF00FFu) | 0x64006400u) + OFF;          // codes (0,2) - 32, exact
                    const qpg_h2 c13 = qpg_u32_as_h2(((t >> 8) & 0x00FF00FFu) | 0x64006400u) + OFF;   // codes (1,3)
                    pa[2 * is] = c02 * SA; pa[2 * is + 1] = c13 * SA;
                    pb[2 * is] = c02 * SB; pb[2 * is + 1] = c13 * SB;
                }
                ba[nt] = qpg_h8{pa[0][0], pa[0][1], pa[1][0], pa[1][1], pa[2][0], pa[2][1], pa[3][0], pa[3][1]};
                bb[nt] = qpg_h8{pb[0][0], pb[0][1], pb[1][0], pb[1][1], pb[2][0], pb[2][1], pb[3][0], pb[3][1]};
            }
            // ---- A fragments: elements 0..3 = k 4kg..4kg+3 of the group (image order {0,2,1,3}), 4..7 = k 16+4kg..
#pragma unroll
            for (int mt = 0; mt < MT6; ++mt) {
                const int row = wm * 32 + mt * 16 + n16;
#pragma unroll
                for (int p = 0; p < PARTS; ++p) {
                    const uint8_t* rp = Ab + (size_t)p * PARTB + (size_t)row * QPG_ROWB;
                    const int s0 = (h * 4 + (kg >> 1)) ^ (row & 7), s1 = (h * 4 + 2 + (kg >> 1)) ^ (row & 7);
                    const qpg_h4 lo4 = *reinterpret_cast<const qpg_h4*>(rp + s0 * 16 + (kg & 1) * 8);
                    const qpg_h4 hi4 = *reinterpret_cast<const qpg_h4*>(rp + s1 * 16 + (kg & 1) * 8);
                    const qpg_h8 af = {lo4[0], lo4[1], lo4[2], lo4[3], hi4[0], hi4[1], hi4[2], hi4[3]};
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt) {
                        acc_a[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, ba[nt], acc_a[mt][nt], 0, 0, 0);
                        acc_b[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, bb[nt], acc_b[mt][nt], 0, 0, 0);
                    }
                }
            }
        }
        if (c == 3) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const float d = f16_bits_to_f32((uint16_t)(cur[nt].d & 0xFFFF));
#pragma unroll
                for (int mt = 0; mt < MT6; ++mt)
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        y[mt][nt][v] = fmaf(d, fmaf(2.f, acc_a[mt][nt][v], acc_b[mt][nt][v]), y[mt][nt][v]);
                        acc_a[mt][nt][v] = 0.f; acc_b[mt][nt][v] = 0.f;
                    }
            }
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) cur[nt] = nxt[nt];
        }
        if (more) x_store(buf ^ 1, xr);
        __syncthreads();
      }
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        if (!have[nt]) continue;
        const int col = (slot_base + bx * WGT + wn * NT + nt) * 16 + n16;
#pragma unroll
        for (int mt = 0; mt < MT6; ++mt)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int t = t0 + wm * 32 + mt * 16 + 4 * kg + v;
                if (t < a.B) C[(size_t)t * ldc + col] = y[mt][nt][v];
            }
    }
}

// ---- Q4_K, second form (round 4; the default for one activation plane): image AND weight tiles through LDS by DMA.
// What bounded the kernel above (round 4, read off its ISA): the image chunk went global -> registers -> LDS one chunk ahead, and the
// compiler's s_waitcnt placement drained EVERY outstanding load in front of the chunk's LDS store -- so neither the image nor the weight
// tiles were ever more than one chunk (~0.8 us) ahead of their use, and a chunk lasted one memory latency (MFMA-busy 26 %).  Here no
// register is the destination of a load in flight:
//   * every wave copies its 1 KiB share of an image chunk, the headers, the planes of its two weight tiles and its share of the sub-block
//     sums into LDS with `global_load_lds_dwordx4` issued as asm (tracked, the compiler drains LDS DMAs in front of LDS reads and barriers);
//   * these are the ONLY VMEM instructions of the loop and come in a fixed order (past the end they re-read the last k-block), so the
//     `s_waitcnt vmcnt(N)` in front of a chunk's barrier is an exact count of what was issued after the data the chunk needs;
//   * weights, headers and sums are read from LDS at the point of use (a tile's plane: one conflict-free ds_read_b128 per lane).
// A first attempt kept the weights in registers behind asm loads with counted waits; tools/check_isa_vmcnt.py showed the compiler copying
// and spilling those "available" registers while the loads were in flight.  Arithmetic and its order are the first form's.
// History of the form (profiles/r04_prompt_gemm_lds_ab.txt, Llama-3-8B prompt step at T = 2048): register-fed 28.9 k tok/s -> ONE workgroup of
// 8 waves per CU, 140 KiB of LDS (image ring of 8 chunks 4 ahead, two whole weight stages), 64-token tile 34.6 k, 128-token tile 37.3 k (40.0 k
// with the final prompt attention) -> TWO workgroups per CU, below: 41.1 k (T = 512: 23.8 -> 25.7 k, 1024: 34.2 -> 37.4 k, 4096: 39.2 -> 39.4 k).
// Measured and dropped on the way: the next chunk's first A fragments in flight across a bare s_barrier (-0.3 %).
// ---- TWO workgroups per CU (64 tokens x 256 rows each): 76 KiB of LDS -- image ring of 4 chunks filled 3
// ahead (32 KiB), ONE stage of weight planes per wave, refilled plane by plane (plane 1 of k-block kb in chunk 0 of kb, plane 0 of kb + 1 in
// chunk 2 of kb: two chunks ahead of their first use; 32 KiB), headers and sums double-buffered (8 + 4 KiB, one k-block ahead).
// VMEM order per wave and k-block:  I P1 P1 | I | I H S P0 P0 | I   -> in front of the barrier of an even chunk everything but the ONE
// instruction issued last has to have landed (its image chunk and the plane it starts to use are older), of an odd chunk all but 8;
// the prologue issues  I | I H S P0 P0 | I  (chunks 1..3 of a k-block "-1") so that the counts hold from the first chunk on
// (tests/test_cpu_dma_plan.py).
#define QPG2_LEAD 3
#define QPG2_RING 4
#define QPG2_IMG (QPG2_RING * 8192)
#define QPG2_PLANES (8 * 4096)
#define QPG2_HS (4096 + 2048)                  // one stage of headers (8 waves x 512 B) | sums (64 tokens x 32 B)
#define QPG2_BYTES (QPG2_IMG + QPG2_PLANES + 2 * QPG2_HS)
#define QPG2_NE 1                              // vmcnt in front of the barrier of chunks 0 and 2
#define QPG2_NO 8                              // ... of chunks 1 and 3
// ---- WT = MI355_GGML_Q5_K: the same kernel over Q5_K tiles (2816 B: header and nibble planes at the Q4_K offsets, then 8 B of transposed
// fifth bits per lane).  One more DMA per wave and k-block, Q, brings the fifth-bit words of BOTH tiles (lanes 0..31: the 512 B of tile 0,
// lanes 32..63: of tile 1) into one contiguous KiB; the wave copies them into registers (2 dwords per tile) where it reads the headers, at
// chunk 0.  The fragment is qpg_frag_q5k_p: one shift and one and-or per operand dword on top of the Q4_K unpack; scales, mins, d, dmin,
// the accumulator chain and the minimum term are the Q4_K arm's.
// LDS, 80 KiB = half a CU exactly, so that two workgroups still fit: image ring 32 KiB | planes, one stage, 32 KiB | fifth-bit words, ONE
// stage, 8 KiB | headers, ONE stage, 4 KiB | sums, two stages of 2 KiB.  Headers and fifth-bit words are private to their wave and sit in
// its registers from chunk 0 on: their region takes the next k-block's in chunk 2 of the same k-block (the planes' rule).  The sums are
// read by every wave in chunk 3 and keep two stages.
// VMEM order per wave and k-block:  I P1 P1 | I | I H Q S P0 P0 | I ; prologue  I(0) | I(1) H Q S P0 P0 | I(2) : 7 weight DMAs, all but 1
// landed in front of an even chunk's barrier, all but 9 in front of an odd one's (tests/test_cpu_q5k_dma_plan.py).
// hipcc, gfx950, -O3: 125 VGPRs (FEPI) / 124, no scratch, 4 waves per SIMD (Q4_K: 125); hipOccupancyMaxActiveBlocksPerMultiprocessor: 2.
#define QPG5_Q (8 * 1024)                      // fifth-bit words: 8 waves x 2 tiles x 512 B
#define QPG5_H 4096                            // headers: 8 waves x 2 tiles x 256 B
#define QPG5_S 2048                            // one stage of sums: 64 tokens x 32 B
#define QPG5_BYTES (QPG2_IMG + QPG2_PLANES + QPG5_Q + QPG5_H + 2 * QPG5_S)
#define QPG5_NW 7                              // weight DMA instructions per wave and k-block
#define QPG5_NE 1                              // vmcnt in front of the barrier of chunks 0 and 2
#define QPG5_NO 9                              // ... of chunks 1 and 3
static_assert(QPG5_BYTES == 80 * 1024, "two workgroups per CU: 2 x 80 KiB = the CU's 160 KiB");
// (the Q5_K arm asks for 4 waves per SIMD = 128 VGPRs outright: left at 2, the compiler spent 131..133 and with them the second workgroup)
template <bool FEPI, bool TAB = false, int WT = MI355_GGML_Q4_K>
__global__ void __launch_bounds__(512, WT == MI355_GGML_Q5_K ? 4 : 2) qpg_gemm_lds2_kernel(const QmmArgs a, const QpgImg im, float* __restrict__ C, const int ldc,
                                                              const int n_slots, const int slot_base) {
    static_assert(WT == MI355_GGML_Q4_K || (WT == MI355_GGML_Q5_K && !TAB), "Q6_K: qpg_gemm_q6k_lds_kernel; no block-table launch for Q5_K");
    constexpr bool Q5 = WT == MI355_GGML_Q5_K;
    constexpr int TILEB = Q5 ? Q5K_TILE : Q4K_TILE, NE = Q5 ? QPG5_NE : QPG2_NE, NO = Q5 ? QPG5_NO : QPG2_NO;
    constexpr int MTW = 4, NTW = 2, WN = 8, BMk = 64, SLOTS = NTW * WN, CHB = BMk * QPG_ROWB, LEAD = QPG2_LEAD, RING = QPG2_RING;
    extern __shared__ __attribute__((aligned(1024))) uint8_t smem[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int wn = wave;
    const int n16 = lane & 15, kg = lane >> 4;
    const int nkb = a.K >> 8, nchunk = a.K >> 6;
    int bx = blockIdx.y, by = blockIdx.x;                            // bx: row block, by: token block (token blocks fastest, as above)
    if constexpr (TAB) {
        // 32 token blocks at a time sweep ALL row blocks before the next 32 start (one launch per expert did this by construction: ~33
        // blocks each): the images of the resident workgroups stay 16 MB -- with the plain order, 264 token blocks x 2 row blocks are
        // resident, 135 MB of images that every one of the 112 row-block rounds pulled in again (measured: the grouped GEMMs 5 % slower
        // than the eight launches they replace; with it 1.2 % faster.  The same order for the plain kernel: -0.5 % at 2048 tokens, -1.2 % at 4096,
        // noise at 8192 -- its launches hold one weight matrix and at most 128 token blocks)
        constexpr int GB = 32;
        const int nbx = gridDim.x, ncol = gridDim.y;
        const int L = (int)blockIdx.x + nbx * (int)blockIdx.y;
        const int g = L / (GB * ncol), rem = L - g * GB * ncol;
        const int gl = min(GB, nbx - g * GB);
        bx = rem / gl;
        by = g * GB + (rem - bx * gl);
    }
    const int t0 = by * BMk;
    // grouped launch over a block table (round 6, mi355_qmm_desc.group_block_table: the experts of a mixture-of-experts layer on a prompt
    // step): token block `by` belongs to ONE expert -- its weights start e * moe_stride[s] bytes into the slabs -- and ends at the expert's
    // last row; blocks past the last expert's leave here, before the first DMA and the first barrier
    // (TAB: its own instantiation -- the plain kernel is the Llama prompt step's and stays as it was)
    int t_end = a.B;
    size_t e_grp = 0;
    if constexpr (TAB) {
        const int2 tb = reinterpret_cast<const int2*>(a.blk_tab)[by];
        if (tb.y <= t0) return;
        e_grp = (size_t)tb.x; t_end = tb.y;
    }

    const uint8_t* wbase[NTW];
    bool have[NTW];
    int e_sg[NTW], e_tile[NTW];
    const bool fsilu = FEPI && a.epi == MI355_EPI_SILU_MUL;
#pragma unroll
    for (int i = 0; i < NTW; ++i) {
        int slot = bx * SLOTS + wn * NTW + i;
        if (fsilu) {
            const int pb = (bx * WN + wn) * (NTW / 2) + (i % (NTW / 2));
            slot = (i < NTW / 2) ? pb : a.seg[0].n_tiles + pb;
            have[i] = pb < a.seg[0].n_tiles;
        } else {
            have[i] = slot < n_slots;
        }
        if (!have[i]) slot = 0;
        int t = slot, sg = 0;
        while (sg + 1 < a.nseg && t >= a.seg[sg].n_tiles) { t -= a.seg[sg].n_tiles; ++sg; }
        wbase[i] = a.seg[sg].w + e_grp * (size_t)a.moe_stride[sg] + (size_t)t * nkb * TILEB;
        e_sg[i] = sg; e_tile[i] = t;
    }
    const uint32_t lds0 = __builtin_amdgcn_readfirstlane((uint32_t)(size_t)(qmg_lptr_t)smem);
    const uint8_t* hsrc = ((lane & 16) ? wbase[1] : wbase[0]) + n16 * 16;     // lanes 0..15: header rows of tile 0, 16..31: of tile 1
    auto dma_image = [&](int kc, int slot) {                          // this wave's KiB of chunk kc
        qmg_dma16(im.xa + ((size_t)kc * im.Tpad + t0) * QPG_ROWB + wave * 1024 + lane * 16, lds0 + (uint32_t)(slot * CHB + wave * 1024));
    };
    // weights: ONE stage of planes (a plane is refilled as soon as its two chunks are multiplied), headers and sums double-buffered
    const uint32_t lds_pl = lds0 + QPG2_IMG + (uint32_t)(wave * 4096);                      // [plane][tile][64 lanes][16 B] of this wave
    auto dma_plane = [&](int kb, int pl) {                            // two instructions (tile 0, tile 1)
#pragma unroll
        for (int i = 0; i < NTW; ++i)
            qmg_dma16(wbase[i] + (size_t)kb * TILEB + 256 + pl * 1024 + lane * 16, lds_pl + (uint32_t)((pl * NTW + i) * 1024));
    };
    auto dma_hdr_sums = [&](int kb, int stage) {                      // two instructions: headers of both tiles (32 lanes), this wave's share of the sums (16 lanes)
        if constexpr (Q5) {                                           // three: H, Q (64 lanes, one stage each), S (two stages)
            // the per-lane source addresses are formed here, once per k-block, from a lane number the compiler cannot see through: hoisted
            // out of the loop they are six more VGPRs, which it spilled -- with a full vmcnt(0) behind each reload
            int ln = lane;
            asm volatile("" : "+v"(ln));
            const uint32_t hq = lds0 + QPG2_IMG + QPG2_PLANES;
            const size_t ko = (size_t)kb * TILEB, w10 = (size_t)(wbase[1] - wbase[0]);      // (tile 1 of this lane = tile 0 + w10, modulo 2^64)
            if (ln < 32) qmg_dma16(wbase[0] + ((ln & 16) ? w10 : 0) + ko + (ln & 15) * 16, hq + QPG5_Q + (uint32_t)(wave * 512));
            qmg_dma16(wbase[0] + ((ln & 32) ? w10 : 0) + ko + 2304 + (ln & 31) * 16, hq + (uint32_t)(wave * 1024));   // lanes 0..31: fifth-bit words of tile 0, 32..63: of tile 1
            if (ln < 16) qmg_dma16(im.sfrag + ((size_t)kb * im.Tpad + t0) * 32 + wave * 256 + ln * 16,
                                   hq + QPG5_Q + QPG5_H + (uint32_t)(stage * QPG5_S + wave * 256));
            return;
        }
        const uint32_t hs = lds0 + QPG2_IMG + QPG2_PLANES + (uint32_t)(stage * QPG2_HS);
        if (lane < 32) qmg_dma16(hsrc + (size_t)kb * TILEB, hs + (uint32_t)(wave * 512));
        if (lane < 16) qmg_dma16(im.sfrag + ((size_t)kb * im.Tpad + t0) * 32 + wave * 256 + lane * 16, hs + 4096u + (uint32_t)(wave * 256));
    };

    f32x4_t y[MTW][NTW], acc[MTW][NTW];
#pragma unroll
    for (int mt = 0; mt < MTW; ++mt)
#pragma unroll
        for (int nt = 0; nt < NTW; ++nt) { y[mt][nt] = f32x4_t{0.f, 0.f, 0.f, 0.f}; acc[mt][nt] = f32x4_t{0.f, 0.f, 0.f, 0.f}; }
    uint32_t Mk = 0x000F000Fu, Mh = 0x00F000F0u, Ck = 0x64006400u;
    asm volatile("" : "+v"(Mk), "+v"(Mh), "+v"(Ck));
    // Q5_K: an operand dword is ((h >> n) & B | C) then (w & M | that) -- two v_and_or_b32 with ONE constant each next to a register, so
    // the masks live in SGPRs and only the exponent patterns (Ck, and Ch = f16 64.0 twice for the high nibbles) take VGPRs
    uint32_t M5k = 0x000F000Fu, M5h = 0x00F000F0u, B4 = 0x00100010u, B8 = 0x01000100u, Ch = 0x54005400u;
    if constexpr (Q5) asm volatile("" : "+s"(M5k), "+s"(M5h), "+s"(B4), "+s"(B8), "+v"(Ch));

    // prologue in the steady state's order (chunks 1, 2, 3 of a k-block "-1"): I(0) | I(1) H S P0 P0 | I(2)
    dma_image(0, 0);
    dma_image(min(1, nchunk - 1), 1);
    dma_hdr_sums(0, 0);
    dma_plane(0, 0);
    dma_image(min(2, nchunk - 1), 2);

    int aoff[2][MTW];                                                 // lane offsets of the A fragments inside a chunk slot: [half][m-tile]
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
        for (int mt = 0; mt < MTW; ++mt) {
            const int row = mt * 16 + n16;
            aoff[h][mt] = row * QPG_ROWB + (((h * 4 + kg) ^ (row & 7)) * 16);
        }

    for (int kb = 0; kb < nkb; ++kb) {
        const int kbn = min(kb + 1, nkb - 1);
        const uint8_t* Wpl = smem + QPG2_IMG + wave * 4096;                              // this wave's planes
        const uint8_t* Whs = smem + QPG2_IMG + QPG2_PLANES + (size_t)(kb & 1) * QPG2_HS;  // headers | sums of this k-block
        const uint8_t* Wq5 = smem + QPG2_IMG + QPG2_PLANES;                               // Q5_K: fifth-bit words | headers | sums x 2
        uint4 H[NTW], pl[NTW];
        qpg_u32x2 qh[NTW];                                                 // Q5_K: the lane's fifth-bit words
        qpg_h2 scp[NTW][4], offp[NTW][4], s16p[NTW][4], off16p[NTW][4];    // scale pairs (s0,s2) (s1,s3) (s4,s6) (s5,s7) and what the nibble positions need of them
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int kc = 4 * kb + c;
            if ((c & 1) == 0) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NE) : "memory");     // chunk + the plane (c = 0: and headers, sums) it starts to use
            else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NO) : "memory");
            __syncthreads();                                          // everyone's shares have landed; the previous chunk (and the plane it finished) is read
            dma_image(min(kc + LEAD, nchunk - 1), (kc + LEAD) & (RING - 1));
            if (c == 0) dma_plane(kb, 1);                             // plane 1 of THIS k-block (chunks 2, 3): its region was read last in chunk 3 of kb - 1
            if (c == 2) { dma_hdr_sums(kbn, (kb + 1) & 1); dma_plane(kbn, 0); }   // the next k-block's headers, sums and plane 0 (read last in chunk 1)
            if (c == 0) {
#pragma unroll
                for (int nt = 0; nt < NTW; ++nt) {
                    H[nt] = *reinterpret_cast<const uint4*>((Q5 ? Wq5 + QPG5_Q : Whs) + wave * 512 + nt * 256 + n16 * 16);
                    if constexpr (Q5) qh[nt] = *reinterpret_cast<const qpg_u32x2*>(Wq5 + wave * 1024 + nt * 512 + lane * 8);
                    const uint32_t s0 = H[nt].y, s2 = H[nt].w;
                    const uint32_t scl4 = s0 & 0x3F3F3F3Fu, sch = (s2 & 0x0F0F0F0Fu) | ((s0 >> 2) & 0x30303030u);
                    const qpg_h2 K1024 = {(_Float16)1024.f, (_Float16)1024.f};
                    scp[nt][0] = __builtin_bit_cast(qpg_h2, (scl4 & 0x00FF00FFu) | Ck) - K1024;
                    scp[nt][1] = __builtin_bit_cast(qpg_h2, ((scl4 >> 8) & 0x00FF00FFu) | Ck) - K1024;
                    scp[nt][2] = __builtin_bit_cast(qpg_h2, (sch & 0x00FF00FFu) | Ck) - K1024;
                    scp[nt][3] = __builtin_bit_cast(qpg_h2, ((sch >> 8) & 0x00FF00FFu) | Ck) - K1024;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {                                // (dead code for Q5_K, which needs the scales alone: qpg_frag_q5k_p)
                        offp[nt][i] = scp[nt][i] * qpg_h2{(_Float16)(-1024.f), (_Float16)(-1024.f)};
                        s16p[nt][i] = scp[nt][i] * qpg_h2{(_Float16)0.0625f, (_Float16)0.0625f};
                        off16p[nt][i] = scp[nt][i] * qpg_h2{(_Float16)(-64.f), (_Float16)(-64.f)};
                    }
                }
            }
            if ((c & 1) == 0) {                                       // plane 0 serves chunks 0, 1, plane 1 chunks 2, 3
#pragma unroll
                for (int nt = 0; nt < NTW; ++nt) pl[nt] = *reinterpret_cast<const uint4*>(Wpl + ((c >> 1) * NTW + nt) * 1024 + lane * 16);
            }
            const uint8_t* Ab = smem + (size_t)(kc & (RING - 1)) * CHB;
            qpg_h8 af[MTW];
            auto a_read = [&](int h) {
#pragma unroll
                for (int mt = 0; mt < MTW; ++mt) af[mt] = *reinterpret_cast<const qpg_h8*>(Ab + aoff[h][mt]);
            };
            a_read(0);
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int j = 2 * c + h;
                qpg_h8 bf[NTW];
#pragma unroll
                for (int nt = 0; nt < NTW; ++nt) {
                    const uint32_t w0 = (c & 1) ? pl[nt].z : pl[nt].x, w1 = (c & 1) ? pl[nt].w : pl[nt].y;
                    const int pi = 2 * (j >> 2) + (j & 1), e = (j >> 1) & 1;      // scale pair and element of sub-block j
                    if constexpr (Q5)
                        bf[nt] = qpg_frag_q5k_p(w0, w0 >> 8, w1, w1 >> 8, qh[nt].x, qh[nt].y, j, scp[nt][pi], e, h ? M5h : M5k, h ? B8 : B4, h ? Ch : Ck);
                    else
                        bf[nt] = qpg_frag_q4k_p(w0, w0 >> 8, w1, w1 >> 8, h ? s16p[nt][pi] : scp[nt][pi], h ? off16p[nt][pi] : offp[nt][pi], e, h ? Mh : Mk, Ck);
                }
#pragma unroll
                for (int mt = 0; mt < MTW; ++mt)
#pragma unroll
                    for (int nt = 0; nt < NTW; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[mt], bf[nt], acc[mt][nt], 0, 0, 0);
                if (h == 0) a_read(1);
            }
            if (c == 3) {
                // ---- end of the k-block: super-block scale d, then the minimum term  - dmin * sum_j m_j S_j
                qpg_h4 sa[MTW];
#pragma unroll
                for (int mt = 0; mt < MTW; ++mt) sa[mt] = *reinterpret_cast<const qpg_h4*>((Q5 ? Wq5 + QPG5_Q + QPG5_H - 4096 + (size_t)(kb & 1) * QPG5_S : Whs) + 4096 + (mt * 16 + n16) * 32 + kg * 8);
#pragma unroll
                for (int nt = 0; nt < NTW; ++nt) {
                    const float d = f16_bits_to_f32((uint16_t)(H[nt].x & 0xFFFF));
                    const float ndmin = -f16_bits_to_f32((uint16_t)(H[nt].x >> 16));
                    const uint32_t s1 = H[nt].z, s2 = H[nt].w;
                    const uint32_t mnl = s1 & 0x3F3F3F3Fu, mnh = ((s2 >> 4) & 0x0F0F0F0Fu) | ((s1 >> 2) & 0x30303030u);
                    const uint32_t mw = (kg & 1) ? mnh : mnl;
                    const qpg_h4 mb = {(_Float16)(float)(mw & 0xFF), (_Float16)(float)((mw >> 8) & 0xFF),
                                       (_Float16)(float)((mw >> 16) & 0xFF), (_Float16)(float)(mw >> 24)};
#pragma unroll
                    for (int mt = 0; mt < MTW; ++mt) {
                        const f32x4_t t1 = __builtin_amdgcn_mfma_f32_16x16x16f16(sa[mt], mb, f32x4_t{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
                        for (int v = 0; v < 4; ++v) {
                            y[mt][nt][v] = fmaf(d, acc[mt][nt][v], fmaf(ndmin, t1[v], y[mt][nt][v]));
                            acc[mt][nt][v] = 0.f;
                        }
                    }
                }
            }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                 // the clamped requests of the last k-block

    if constexpr (FEPI) {
        if (a.epi == MI355_EPI_QKV_ROPE_CACHE) {
            // q | k | v of a prompt step (round 6): interleaved RoPE, the cast to bf16 and the q_out / paged-cache scatter in the store loop
            // (QuantizedAttention::forward, attention.rs:920-995) -- no C buffer, no epilogue launch.  A lane holds output row n16 of four
            // tokens; the RoPE partner (row ^ 1) sits in the neighbouring lane: one DPP quad swap.  Segment roles: 0 = q, 1 = k, 2 = v.
            const int hrot = a.rot >> 1;
#pragma unroll
            for (int mt = 0; mt < MTW; ++mt)
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int t = t0 + mt * 16 + 4 * kg + v;
                    const bool tl = t < t_end;                              // (uniform over the lane pair: t does not depend on n16)
                    const float rs = tl ? im.row_scale[t] : 0.f;
                    const int64_t pos = tl ? a.positions[t] : 0;
#pragma unroll
                    for (int nt = 0; nt < NTW; ++nt) {
                        const int sg = e_sg[nt], lrow = e_tile[nt] * 16 + n16;
                        const bool rowok = have[nt] && lrow < a.seg[sg].n_rows;
                        float val = y[mt][nt][v] * rs;
                        if (a.bias && rowok) val += a.bias[a.seg[sg].row0 + lrow];
                        const float partner = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, val), 0xB1, 0xF, 0xF, false));   // quad_perm [1,0,3,2]
                        if (!tl || !rowok) continue;
                        const int d = lrow % a.D;
                        float o = val;
                        if (sg < 2 && d < a.rot) {
                            const float c = a.cos_t[pos * hrot + (d >> 1)], sn = a.sin_t[pos * hrot + (d >> 1)];
                            o = (d & 1) ? (partner * sn + val * c) : (val * c - partner * sn);
                        }
                        qmm_qkv_store(a, sg, lrow, t, o);
                    }
                }
            return;
        }
        float* const aout = a.out;
#pragma unroll
        for (int mt = 0; mt < MTW; ++mt)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int t = t0 + mt * 16 + 4 * kg + v;
                if (t >= t_end) continue;
                const float rs = im.row_scale[t];
                if (fsilu) {
#pragma unroll
                    for (int nt = 0; nt < NTW / 2; ++nt) {
                        const int lrow = e_tile[nt] * 16 + n16;
                        if (!have[nt] || lrow >= a.seg[0].n_rows) continue;
                        float g = y[mt][nt][v] * rs, u = y[mt][nt + NTW / 2][v] * rs;
                        if (a.bias) { g += a.bias[a.seg[0].row0 + lrow]; u += a.bias[a.seg[1].row0 + lrow]; }
                        aout[(size_t)t * a.ldo + lrow] = silu_f(g) * u;
                    }
                } else {
#pragma unroll
                    for (int nt = 0; nt < NTW; ++nt) {
                        const int lrow = e_tile[nt] * 16 + n16;
                        if (!have[nt] || lrow >= a.seg[e_sg[nt]].n_rows) continue;
                        const int orow = a.seg[e_sg[nt]].row0 + lrow;
                        float val = y[mt][nt][v] * rs;
                        if (a.bias) val += a.bias[orow];
                        if (a.epi == MI355_EPI_RESID) val += a.resid[(size_t)t * a.ldo + orow];
                        aout[(size_t)t * a.ldo + orow] = val;
                    }
                }
            }
        return;
    }
#pragma unroll
    for (int nt = 0; nt < NTW; ++nt) {
        if (!have[nt]) continue;
        const int col = (slot_base + bx * SLOTS + wn * NTW + nt) * 16 + n16;
#pragma unroll
        for (int mt = 0; mt < MTW; ++mt)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int t = t0 + mt * 16 + 4 * kg + v;
                if (t < t_end) C[(size_t)t * ldc + col] = y[mt][nt][v];
            }
    }
}

// QPG6_ONE_PLANE (round 6): ONE f16 operand per weight, sc (c - 32) rounded to f16 by the multiply.  |sc (c - 32)| <= 4096 and f16 holds every
// integer to 2048 and every even one to 4096, so the product is inexact only where it is odd and above 2048 (0.7 % of the weights of a
// quantised normal matrix, 2^-12 relative there: 5e-5 on a 14336-deep output next to the 3e-4 of the image's own f16 rounding, which this
// kernel always has -- the hi + lo "exact" image goes through the register-fed qpg_gemm_q6k_kernel and keeps its two exact planes).  Half
// the MFMAs and a third less unpacking: the kernel was running the matrix cores as hard as the Q4_K one, on twice the instructions.
#ifndef QPG6_ONE_PLANE
#define QPG6_ONE_PLANE 1
#endif
// ---- Q6_K, second form: one workgroup per CU (its tiles are larger: 144 KiB) -- image (ring of 4 chunk slots, 3 ahead) and the wave's two weight tiles (two stages,
// one k-block ahead) through LDS by asm DMA; per wave and k-block: I W W W W W W W W | I | I | I (W: scales of both tiles, d of both
// tiles, then ql half 0, ql half 1, qh of tile 0 and 1), so vmcnt = 2 in front of chunk 0's barrier and 2 + 8 in front of the others.
#define QPG6_LDS_WAVE 7168                     // 2 x 256 B scales | 2 x 32 B d | pad to 1 KiB | {ql0, ql1, qh} x 2 tiles x 1 KiB
#define QPG6_LDS_IMG (4 * 8192)
#define QPG6_LDS_WST (8 * QPG6_LDS_WAVE)
#define QPG6_LDS_BYTES (QPG6_LDS_IMG + 2 * QPG6_LDS_WST)
#define QPG6_LEAD 3
#define QPG6_RING 4
#define QPG6_NW 8                              // weight DMA instructions per wave and k-block
#define QPG6_N0 (QPG6_LEAD - 1)                // vmcnt in front of the barrier of chunk 0 ...
#define QPG6_N1 (QPG6_LEAD - 1 + QPG6_NW)      // ... and of chunks 1..3
// FEPI6 (round 6): the epilogue -- store / residual add / the v role of the q|k|v epilogue (bf16 + cache scatter) -- in the store loop,
// as qpg_gemm_lds2_kernel<true> does for Q4_K: no C buffer, no epilogue launch for the Q6_K down projections and values of a Q4_K_M file.
// NT (round 6): row tiles per wave.  2 = 256 rows per workgroup (default); 1 = 128 rows, for launches that would leave half the chip
// empty (the 1024-row value projection at 2048 tokens: 32 token blocks x 4 = 128 workgroups -> 256); the weight DMA is then 5
// instructions per wave and k-block instead of 8, and so is the count in front of chunks 1..3.
// TAB: the block-table launch of qpg_gemm_lds2_kernel<., true> for a Q6_K matrix (the down projections of a Q4_K_M mixture-of-experts file).
template <bool FEPI6, int NT = 2, bool TAB = false>
__global__ void __launch_bounds__(512, 1) qpg_gemm_q6k_lds_kernel(const QmmArgs a, const QpgImg im, float* __restrict__ C, const int ldc,
                                                                  const int n_slots, const int slot_base) {
    extern __shared__ __attribute__((aligned(1024))) uint8_t smem[];
    constexpr int WGT = 8 * NT, MT6 = 4, BMk = 64, CHB = BMk * QPG_ROWB, LEAD = QPG6_LEAD, RING = QPG6_RING;
    constexpr int N1 = QPG6_LEAD - 1 + 2 + 3 * NT;                   // = QPG6_N1 at NT = 2
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int wn = wave;
    const int n16 = lane & 15, kg = lane >> 4;
    const int nkb = a.K >> 8, nchunk = a.K >> 6;
    int bx = blockIdx.y, by = blockIdx.x;
    int t_end = a.B;
    size_t e_grp = 0;
    if constexpr (TAB) {                                             // group-major order + block table: see qpg_gemm_lds2_kernel
        constexpr int GB = 32;
        const int nbx = gridDim.x, ncol = gridDim.y;
        const int L = (int)blockIdx.x + nbx * (int)blockIdx.y;
        const int g = L / (GB * ncol), rem = L - g * GB * ncol;
        const int gl = min(GB, nbx - g * GB);
        bx = rem / gl;
        by = g * GB + (rem - bx * gl);
        const int2 tb = reinterpret_cast<const int2*>(a.blk_tab)[by];
        if (tb.y <= by * BMk) return;
        e_grp = (size_t)tb.x; t_end = tb.y;
    }
    const int t0 = by * BMk;
    const uint8_t* wbase[NT];
    bool have[NT];
    int e_sg[NT], e_tile[NT];                                        // FEPI6: segment and tile of each row tile
#pragma unroll
    for (int i = 0; i < NT; ++i) {
        int slot = bx * WGT + wn * NT + i;
        have[i] = slot < n_slots;
        if (!have[i]) slot = 0;
        int t = slot, sg = 0;
        while (sg + 1 < a.nseg && t >= a.seg[sg].n_tiles) { t -= a.seg[sg].n_tiles; ++sg; }
        wbase[i] = a.seg[sg].w + e_grp * (size_t)a.moe_stride[sg] + (size_t)t * nkb * Q6K_TILE;
        e_sg[i] = sg; e_tile[i] = t;
    }
    const uint32_t lds0 = __builtin_amdgcn_readfirstlane((uint32_t)(size_t)(qmg_lptr_t)smem);
    const uint8_t* scsrc = ((lane & 16) ? wbase[NT - 1] : wbase[0]) + n16 * 16;            // lanes 0..31: the 16 scale rows of tile 0, of tile 1
    const uint8_t* dsrc = ((lane & 2) ? wbase[NT - 1] : wbase[0]) + 3328 + (lane & 1) * 16; // lanes 0..3: the 32 B of d of tile 0, of tile 1
    auto dma_image = [&](int kc, int slot) {
        qmg_dma16(im.xa + ((size_t)kc * im.Tpad + t0) * QPG_ROWB + wave * 1024 + lane * 16, lds0 + (uint32_t)(slot * CHB + wave * 1024));
    };
    auto dma_weights = [&](int kb, int stage) {                       // eight instructions, always in this order
        const uint32_t mine = lds0 + QPG6_LDS_IMG + (uint32_t)(stage * QPG6_LDS_WST + wave * QPG6_LDS_WAVE);
        const size_t ko = (size_t)kb * Q6K_TILE;
        if (lane < 16 * NT) qmg_dma16(scsrc + ko, mine);
        if (lane < 2 * NT) qmg_dma16(dsrc + ko, mine + 512u);
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int q = 0; q < 3; ++q)                               // ql half 0, ql half 1, qh
                qmg_dma16(wbase[i] + ko + 256 + q * 1024 + lane * 16, mine + 1024u + (uint32_t)((i * 3 + q) * 1024));
    };
    f32x4_t y[MT6][NT], acc_a[MT6][NT];
#if !QPG6_ONE_PLANE
    f32x4_t acc_b[MT6][NT];
#endif
#pragma unroll
    for (int mt = 0; mt < MT6; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            y[mt][nt] = f32x4_t{0.f, 0.f, 0.f, 0.f}; acc_a[mt][nt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#if !QPG6_ONE_PLANE
            acc_b[mt][nt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#endif
        }
    dma_weights(0, 0);
#pragma unroll
    for (int c = 0; c < LEAD; ++c) dma_image(min(c, nchunk - 1), c);
    const qpg_h2 OFF = {(_Float16)(-1056.f), (_Float16)(-1056.f)};   // 0x6400 | code = 1024 + code; code - 32 = that - 1056

    for (int kb = 0; kb < nkb; ++kb) {
        const int kbn = min(kb + 1, nkb - 1);
        const uint8_t* Wme = smem + QPG6_LDS_IMG + (size_t)(kb & 1) * QPG6_LDS_WST + wave * QPG6_LDS_WAVE;
        Qpg6Tile cur[NT];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int kc = 4 * kb + c;
        if (c == 0) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(QPG6_N0) : "memory");
        else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N1) : "memory");
        __syncthreads();
        dma_image(min(kc + LEAD, nchunk - 1), (kc + LEAD) & (RING - 1));
        if (c == 0) {
            dma_weights(kbn, (kb + 1) & 1);
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                cur[i].sc = *reinterpret_cast<const uint4*>(Wme + i * 256 + n16 * 16);
                cur[i].d = *reinterpret_cast<const uint16_t*>(Wme + 512 + i * 32 + n16 * 2);
                cur[i].ql0 = *reinterpret_cast<const uint4*>(Wme + 1024 + (i * 3 + 0) * 1024 + lane * 16);
                cur[i].ql1 = *reinterpret_cast<const uint4*>(Wme + 1024 + (i * 3 + 1) * 1024 + lane * 16);
                cur[i].qh = *reinterpret_cast<const uint4*>(Wme + 1024 + (i * 3 + 2) * 1024 + lane * 16);
            }
        }
        const uint8_t* Ab = smem + (size_t)(kc & (RING - 1)) * CHB;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int G = 2 * c + h, n = G >> 2, tt = G & 3;          // 32-k group of the k-block
            qpg_h8 ba[NT];
#if !QPG6_ONE_PLANE
            qpg_h8 bb[NT];
#endif
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const uint4 ql = n ? cur[nt].ql1 : cur[nt].ql0;
                const uint32_t scw[4] = {cur[nt].sc.x, cur[nt].sc.y, cur[nt].sc.z, cur[nt].sc.w};
                qpg_h2 pa[4];
#if !QPG6_ONE_PLANE
                qpg_h2 pb[4];
#endif
#pragma unroll
                for (int is = 0; is < 2; ++is) {
                    const uint32_t qa = is ? ql.z : ql.x, qb = is ? ql.w : ql.y;
                    const uint32_t hq = n ? (is ? cur[nt].qh.w : cur[nt].qh.z) : (is ? cur[nt].qh.y : cur[nt].qh.x);
                    uint32_t t;
                    if (tt == 0) t = (qa & 0x0F0F0F0Fu) | ((hq << 4) & 0x30303030u);
                    else if (tt == 1) t = (qb & 0x0F0F0F0Fu) | ((hq << 2) & 0x30303030u);
                    else if (tt == 2) t = ((qa >> 4) & 0x0F0F0F0Fu) | (hq & 0x30303030u);
                    else t = ((qb >> 4) & 0x0F0F0F0Fu) | ((hq >> 2) & 0x30303030u);
                    const int s = 8 * n + 2 * tt + is;                // 16-wide sub-block
                    const int sc8 = (int)(int8_t)((scw[s >> 2] >> (8 * (s & 3))) & 0xFF);
                    const qpg_h2 c02 = qpg_u32_as_h2((t & 0x00FF00FFu) | 0x64006400u) + OFF;
                    const qpg_h2 c13 = qpg_u32_as_h2(((t >> 8) & 0x00FF00FFu) | 0x64006400u) + OFF;
#if QPG6_ONE_PLANE
                    const _Float16 sa = (_Float16)(float)sc8;
                    const qpg_h2 SA = {sa, sa};
                    pa[2 * is] = c02 * SA; pa[2 * is + 1] = c13 * SA;
#else
                    const _Float16 sa = (_Float16)(float)(sc8 >> 1), sb = (_Float16)(float)(sc8 & 1);
                    const qpg_h2 SA = {sa, sa}, SB = {sb, sb};
                    pa[2 * is] = c02 * SA; pa[2 * is + 1] = c13 * SA;
                    pb[2 * is] = c02 * SB; pb[2 * is + 1] = c13 * SB;
#endif
                }
                ba[nt] = qpg_h8{pa[0][0], pa[0][1], pa[1][0], pa[1][1], pa[2][0], pa[2][1], pa[3][0], pa[3][1]};
#if !QPG6_ONE_PLANE
                bb[nt] = qpg_h8{pb[0][0], pb[0][1], pb[1][0], pb[1][1], pb[2][0], pb[2][1], pb[3][0], pb[3][1]};
#endif
            }
#pragma unroll
            for (int mt = 0; mt < MT6; ++mt) {
                const int row = mt * 16 + n16;
                const uint8_t* rp = Ab + (size_t)row * QPG_ROWB;
                const int s0 = (h * 4 + (kg >> 1)) ^ (row & 7), s1 = (h * 4 + 2 + (kg >> 1)) ^ (row & 7);
                const qpg_h4 lo4 = *reinterpret_cast<const qpg_h4*>(rp + s0 * 16 + (kg & 1) * 8);
                const qpg_h4 hi4 = *reinterpret_cast<const qpg_h4*>(rp + s1 * 16 + (kg & 1) * 8);
                const qpg_h8 af = {lo4[0], lo4[1], lo4[2], lo4[3], hi4[0], hi4[1], hi4[2], hi4[3]};
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    acc_a[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, ba[nt], acc_a[mt][nt], 0, 0, 0);
#if !QPG6_ONE_PLANE
                    acc_b[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, bb[nt], acc_b[mt][nt], 0, 0, 0);
#endif
                }
            }
        }
        if (c == 3) {
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const float d = f16_bits_to_f32((uint16_t)(cur[nt].d & 0xFFFF));
#pragma unroll
                for (int mt = 0; mt < MT6; ++mt)
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
#if QPG6_ONE_PLANE
                        y[mt][nt][v] = fmaf(d, acc_a[mt][nt][v], y[mt][nt][v]);
                        acc_a[mt][nt][v] = 0.f;
#else
                        y[mt][nt][v] = fmaf(d, fmaf(2.f, acc_a[mt][nt][v], acc_b[mt][nt][v]), y[mt][nt][v]);
                        acc_a[mt][nt][v] = 0.f; acc_b[mt][nt][v] = 0.f;
#endif
                    }
            }
        }
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if constexpr (FEPI6) {
        float* const aout = a.out;
#pragma unroll
        for (int mt = 0; mt < MT6; ++mt)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int t = t0 + mt * 16 + 4 * kg + v;
                if (t >= t_end) continue;
                const float rs = im.row_scale[t];
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const int sg = e_sg[nt], lrow = e_tile[nt] * 16 + n16;
                    if (!have[nt] || lrow >= a.seg[sg].n_rows) continue;
                    const int orow = a.seg[sg].row0 + lrow;
                    float val = y[mt][nt][v] * rs;
                    if (a.bias) val += a.bias[orow];
                    if (a.epi == MI355_EPI_QKV_ROPE_CACHE) {          // the launcher sends only the v segment here (role 2: no rotation)
                        qmm_qkv_store(a, sg, lrow, t, val);
                    } else {
                        if (a.epi == MI355_EPI_RESID) val += a.resid[(size_t)t * a.ldo + orow];
                        aout[(size_t)t * a.ldo + orow] = val;
                    }
                }
            }
        return;
    }
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        if (!have[nt]) continue;
        const int col = (slot_base + bx * WGT + wn * NT + nt) * 16 + n16;
#pragma unroll
        for (int mt = 0; mt < MT6; ++mt)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int t = t0 + mt * 16 + 4 * kg + v;
                if (t < t_end) C[(size_t)t * ldc + col] = y[mt][nt][v];
            }
    }
}

// the DMA plan of the LDS-fed prompt kernels for the host-side check of the hand-counted waits (tests/test_cpu_dma_plan.py):
// kind 2 = qpg_gemm_lds2_kernel (its own instruction order; the two counts are those of the even / odd chunks), 5 = the same kernel over
// Q5_K tiles (tests/test_cpu_q5k_dma_plan.py), 6 = qpg_gemm_q6k_lds_kernel
// ->  {LEAD, RING, image DMAs per wave and chunk, weight DMAs per wave and k-block, vmcnt before chunk 0's barrier, vmcnt before the other
// chunks' barriers}
extern "C" int32_t mi355_internal_qpg_dma_plan(int32_t kind, int32_t* out6) {
    if (kind == 6) { const int32_t v[6] = {QPG6_LEAD, QPG6_RING, 1, QPG6_NW, QPG6_N0, QPG6_N1}; for (int i = 0; i < 6; ++i) out6[i] = v[i]; return 0; }
    if (kind == 61) { const int32_t v[6] = {QPG6_LEAD, QPG6_RING, 1, 2 + 3 * 1, QPG6_N0, QPG6_LEAD - 1 + 2 + 3 * 1}; for (int i = 0; i < 6; ++i) out6[i] = v[i]; return 0; }   // NT = 1
    if (kind == 2) { const int32_t v[6] = {QPG2_LEAD, QPG2_RING, 1, 6, QPG2_NE, QPG2_NO}; for (int i = 0; i < 6; ++i) out6[i] = v[i]; return 0; }   // qpg_gemm_lds2_kernel: its own order
    if (kind == 5) { const int32_t v[6] = {QPG2_LEAD, QPG2_RING, 1, QPG5_NW, QPG5_NE, QPG5_NO}; for (int i = 0; i < 6; ++i) out6[i] = v[i]; return 0; }   // ... over Q5_K tiles
    return -1;
}
