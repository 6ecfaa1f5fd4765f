// MXFP4 (OCP MX: e2m1 elements, one e8m0 scale per 32 k) linears for the safetensors path: `LnMxfp4` (src/openai/models/linear.rs:1677-1757),
// the layer the `quant_method: "mxfp4"` exports (`weight_packed` / `weight_scale`) and gpt-oss (`blocks` / `scales`) load.  The weight is
// [out, in/2] bytes -- byte j of a row holds element 2j in its LOW nibble and 2j + 1 in its high nibble, a nibble = sign (bit 3) | index into
// {0, 0.5, 1, 1.5, 2, 3, 4, 6} -- with [out, in/32] e8m0 scale bytes (2^(code - 127); 0xFF is NaN):
//     y[t, r] = round_dt( sum_c x[t, c] * e2m1(w[r, c]) * 2^(s[r, c/32] - 127) )          (+ bias, + the fused epilogues of mi355_linear)
// W4A16: the activations stay 16-bit, accumulation is f32 (v_mfma_f32_16x16x32_{bf16,f16}: a scale group is exactly one MFMA step), and
// the weight operand is decoded EXACTLY by v_cvt_scalef32_pk_{bf16,f16}_fp4 (one instruction per byte = two MFMA operand elements):
//   * bf16: the scale is folded into the operand by that instruction -- 6 * 2^(e-127) and 0.5 * 2^(e-127) are bf16 numbers for every
//     code 2..250 (bf16 has f32's exponent), so one accumulator runs through all of K;
//   * f16: 0.5 * 2^-20 is no f16 number, so the operand is decoded UNSCALED (scale 1.0), every 32-k group gets a fresh accumulator, and one
//     f32 fma per accumulator register folds it in with the scale of the lane's own row (the B-operand lane's row n%16 is the column that
//     lane owns in the 16 x 16 result).
// A 0xFF scale makes the outputs of its row NaN (the lane remembers it and poisons its column before the epilogue).
//
// Tile image (mi355_mxfp4_tile_repack; mx4_tile_kernel below writes it): 16-row x 128-k tiles of 1 KiB,
//     blocks: [tile n/16][k-block k/128][lane = 16 * ((k%32)/8) + n%16][16 B = [(k%128)/32][(k%8)/2]]
//     scales: [tile n/16][k-block k/128][row n%16][group (k%128)/32]                         (64 B per tile and k-block)
// -- a lane's dword j is its B fragment (8 consecutive k of row n%16) of the j-th 32-k MFMA step of the k-block: one dwordx4 per lane and
// (tile, k-block), every wave instruction one contiguous KiB, a tile's k-blocks back to back; the four scales of the lane's row in a
// k-block are one dword, and 16 k-blocks of a tile's scales are one contiguous KiB.
//
// Two kernels:
//   mxfp4_small_kernel  1..32 tokens: streaming mat-vec, the weights never touch LDS (register ring, MS_RING k-blocks ahead)
//   mxfp4_gemm_kernel   33.. tokens: 128 x 128 MFMA tile, both operands global -> LDS by DMA, the weight side as packed nibbles
// (33..96 tokens with too few GEMM tiles to fill the chip: 32-token chunks of the first -- mxfp4_run at the end of the file)
#include "mxfp4_decode.h"            // decode, MFMA step and the LDS DMA, shared with mxfp4_moe.hip
#include "../../include/mi355_vllm.h"
#include <hip/hip_runtime.h>

struct Mx4Args {
    const uint8_t* w;         // tiled blocks
    const uint8_t* s;         // tiled scales
    const void* x;            // 16-bit [T][K]
    void* out;                // 16-bit [T][ldo]
    const void* bias;         // 16-bit [N] or null
    const void* resid;        // 16-bit [T][ldo] (EPI_RESID; may be `out`)
    int32_t T, N, K, ldo, epi;
    int32_t pair_offset;      // SILU_MUL: rows of `up` start here (packed [gate; up], mlp.rs:324-352)
};

// the rounding chain of one output element, as dense_gemv.hip's: matmul -> dtype, + bias -> dtype (linear.rs:124-172), then
// + residual -> dtype or silu(gate) -> dtype, * up -> dtype (mlp.rs:457)
template <int DT>
__device__ __forceinline__ void mx4_epilogue(const Mx4Args& a, const int t, const int col, const float y, const float up) {
    const uint16_t* b16 = static_cast<const uint16_t*>(a.bias);
    float o = mx4_rnd<DT>(y);
    if (b16) o = mx4_rnd<DT>(o + mx4_h2f<DT>(b16[col]));
    if (a.epi == MI355_EPI_SILU_MUL) {
        float u = mx4_rnd<DT>(up);
        if (b16) u = mx4_rnd<DT>(u + mx4_h2f<DT>(b16[a.pair_offset + col]));
        o = mx4_rnd<DT>(mx4_rnd<DT>(o / (1.f + __expf(-o))) * u);
    } else if (a.epi == MI355_EPI_RESID) {
        o = mx4_rnd<DT>(o + mx4_h2f<DT>(static_cast<const uint16_t*>(a.resid)[(size_t)t * a.ldo + col]));
    }
    static_cast<uint16_t*>(a.out)[(size_t)t * a.ldo + col] = mx4_f2h<DT>(o);
}

// ------------------------------------------------------------------------------------------------ 1..32 tokens
// One workgroup = R row tiles (R = 2: a gate tile and its up tile) x all of K, MS_NW waves; wave w owns the k-blocks w, w + NW, ...
//   * weights: global -> registers in image order, a ring of MS_RING k-blocks per wave: ONE dwordx4 per lane, tile and k-block (a KiB per
//     wave instruction) with the lane's scale dword riding along.  A (tile, k-block) is 1 KiB where FP8's is 2, so the ring is 8 deep where
//     FP8's is 4: 8 waves x 8 k-blocks x 1 KiB keep 64 KiB (R = 2: 128) in flight per workgroup, at 32 (64) ring VGPRs.  A slot beyond the
//     end of K is not fetched (wave-uniform branch), so a short K (4096: four k-blocks per wave) issues exactly its own bytes;
//   * activations: staged in LDS by all threads, coalesced, G k-blocks per wave at a time (as much of K as fits MS_X_BYTES: at one
//     token all of K up to 31744 -- once per workgroup; at 32 tokens one k-block per wave and pass); rows padded by 16 B so that the
//     16 rows of an A-fragment read start on different bank quads;
//   * MT = ceil(T / 16) M tiles; four MFMA steps per k-block, the decode one instruction per byte (16 per lane, tile and k-block);
//   * cross-wave reduction through LDS (over the staging area), epilogue out of the sums.
// Llama-3-8B down (256 row tiles x 112 k-blocks) is one workgroup per CU with 14 k-blocks per wave: every CU streams, 64 KiB ahead.
constexpr int MS_NW = 8, MS_RING = 8;
constexpr int MS_X_BYTES = 32 * (MS_NW * 256 + 16);        // 66048: 32 tokens x one k-block per wave; two workgroups per CU

template <int DT, int MT, int R>
__global__ void __launch_bounds__(64 * MS_NW) mxfp4_small_kernel(const Mx4Args a, const int G) {
    extern __shared__ __attribute__((aligned(16))) uint8_t ms_lds[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r16 = lane & 15, kg = lane >> 4;
    const int T = a.T, nkb = a.K >> 7;
    const int niter = (nkb + MS_NW - 1) / MS_NW;            // the same for every wave (the barriers below)
    const int ldx = G * MS_NW * 256 + 16;                   // bytes per staged row
    int row0[R];
    row0[0] = (int)blockIdx.x * 16;
    if (R == 2) row0[R - 1] = a.pair_offset + (int)blockIdx.x * 16;
    const uint8_t* wp[R];
    const uint8_t* sp[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        wp[r] = a.w + ((size_t)(row0[r] >> 4) * nkb) * 1024 + lane * 16;
        sp[r] = a.s + ((size_t)(row0[r] >> 4) * nkb) * 64 + r16 * 4;
    }
    uint4 ring[MS_RING][R];
    uint32_t rs[MS_RING][R];
#define MS_LOAD(SLOT_, I_) do { \
        const int kb_ = wave + (I_) * MS_NW; \
        if (kb_ < nkb) { \
            _Pragma("unroll") for (int r_ = 0; r_ < R; ++r_) { \
                const mx4_u32x4 v_ = __builtin_nontemporal_load(reinterpret_cast<const mx4_u32x4*>(wp[r_] + (size_t)kb_ * 1024)); \
                ring[SLOT_][r_] = make_uint4(v_.x, v_.y, v_.z, v_.w); \
                rs[SLOT_][r_] = *reinterpret_cast<const uint32_t*>(sp[r_] + (size_t)kb_ * 64); \
            } \
        } \
    } while (0)
#pragma unroll
    for (int s = 0; s < MS_RING; ++s) {
#pragma unroll
        for (int r = 0; r < R; ++r) { ring[s][r] = make_uint4(0u, 0u, 0u, 0u); rs[s][r] = 0u; }
        MS_LOAD(s, s);
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
    const int pass_cols = G * MS_NW * 128;                  // k columns of one staging pass

    for (int i0 = 0; i0 < niter; i0 += MS_RING) {
#pragma unroll
        for (int s = 0; s < MS_RING; ++s) {
            const int i = i0 + s;
            if (i < niter) {                                 // (uniform over the workgroup)
                const int g = i % G;
                if (g == 0) {
                    // ---- the activations of the next G k-blocks of every wave: columns [c0, c0 + pass_cols) of x
                    const int c0 = (i / G) * pass_cols, cols = min(pass_cols, a.K - c0), ppr = cols >> 3;      // 16-byte pieces per row
                    __syncthreads();                         // everyone is done with the previous pass
                    for (int p = threadIdx.x; p < T * ppr; p += 64 * MS_NW) {
                        const int t = p / ppr, c = p - t * ppr;
                        *reinterpret_cast<uint4*>(ms_lds + (size_t)t * ldx + c * 16) =
                            *reinterpret_cast<const uint4*>(xg + ((size_t)t * a.K + c0) * 2 + c * 16);
                    }
                    __syncthreads();
                }
                const int kb = wave + i * MS_NW;
                if (kb < nkb) {
                    const uint8_t* xl = ms_lds + (size_t)(g * MS_NW + wave) * 256 + 16 * kg;                    // this k-block inside the pass
#pragma unroll
                    for (int r = 0; r < R; ++r) bad[r] |= mx4_has_nan(rs[s][r]);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        uint4 af[MT];
#pragma unroll
                        for (int mt = 0; mt < MT; ++mt)
                            af[mt] = *reinterpret_cast<const uint4*>(xl + (size_t)min(mt * 16 + r16, T - 1) * ldx + 64 * j);
#pragma unroll
                        for (int r = 0; r < R; ++r) {
                            const float sf = mx4_scale(rs[s][r], j);
                            const uint4 bf = mx4_frag<DT>(mx4_dword(ring[s][r], j), sf);
#pragma unroll
                            for (int mt = 0; mt < MT; ++mt) mx4_step<DT>(y[r][mt], af[mt], bf, sf);
                        }
                    }
                }
                MS_LOAD(s, i + MS_RING);
            }
        }
    }
#undef MS_LOAD
    // ---- cross-wave reduction: C layout = lane (column = weight row r16, rows m = 4 kg + v)
    float* red = reinterpret_cast<float*>(ms_lds);          // [NW][R][MT][16 m][16 rows]
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int v = 0; v < 4; ++v)
                red[(((wave * R + r) * MT + mt) * 16 + 4 * kg + v) * 16 + r16] = bad[r] ? __builtin_nanf("") : y[r][mt][v];
    __syncthreads();
    for (int idx = threadIdx.x; idx < MT * 256; idx += 64 * MS_NW) {
        const int rr = idx & 15, m = idx >> 4;
        if (m >= T) continue;
        float val[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            float s = 0.f;
#pragma unroll
            for (int w = 0; w < MS_NW; ++w) s += red[(((w * R + r) * MT + (m >> 4)) * 16 + (m & 15)) * 16 + rr];
            val[r] = s;
        }
        mx4_epilogue<DT>(a, m, row0[0] + rr, val[0], val[R - 1]);
    }
}

// ------------------------------------------------------------------------------------------------ prompt steps
// Workgroup tile 128 tokens x 128 weight rows (SILU_MUL: 64 gate rows and the 64 matching up rows), 4 waves as 2 x 2, wave tile
// 64 x 64 (4 x 4 fragments), two workgroups per CU.  K in steps of 64, the DMA of the next step in flight while this one is multiplied
// (one counted wait + one barrier per step), as dense_gemm_kernel and fp8_gemm_kernel:
//   * x: 128 rows x 128 B per step, two buffers, 16-byte slot c of row r at slot c ^ (r & 7) (applied to the lane's global source address);
//   * weights: packed nibbles, the image's KiB runs copied verbatim.  A KiB is a whole k-block of a row tile = TWO K steps, so the weight
//     side has two buffers of 8 row tiles x 1 KiB that turn over once per k-block (filled during the first step of the k-block before):
//     4 KiB per 64-k step where FP8 moves 8 and a 16-bit tile 16.  A lane's two B fragments of a step are one ds_read_b64 of its own
//     bytes, decoded in registers (one instruction per byte) and used by four m-fragments each;
//   * scales: 16 k-blocks of a row tile's scale plane are one contiguous KiB, so they ride the same DMA: two buffers of 8 row tiles x
//     1 KiB that turn over every 16 k-blocks (a lane past the end of K re-reads the last k-block: nothing is read outside the plane).  No
//     panel and therefore no limit on K; a lane reads the four scales of its row and k-block as one dword per n-fragment.
// bf16 accumulates straight through K; f16 takes each 32-k step through a fresh accumulator and one fma per register (mx4_step).
constexpr uint32_t MG_A_BYTES = 128 * 128, MG_B_BYTES = 8 * 1024, MG_S_BYTES = 8 * 1024;
constexpr uint32_t MG_B_OFF = 2 * MG_A_BYTES, MG_S_OFF = MG_B_OFF + 2 * MG_B_BYTES, MG_LDS = MG_S_OFF + 2 * MG_S_BYTES;      // 64 KiB

template <int DT>
__global__ void __launch_bounds__(256, 2) mxfp4_gemm_kernel(const Mx4Args a) {
    extern __shared__ __attribute__((aligned(1024))) uint8_t mg_lds[];   // [A 2 x 16 KiB][B 2 x 8 KiB][scales 2 x 8 KiB]
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
    const uint32_t lds0 = __builtin_amdgcn_readfirstlane((uint32_t)(size_t)(__attribute__((address_space(3))) void*)mg_lds);
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
        ssrc[r] = a.s + tk * 64 + (lane & 3) * 16;                       // + 64 * k-block (lane / 4 of the chunk of 16)
    }
    auto stage_a = [&](int kt, int buf) {
        const uint32_t base = lds0 + (uint32_t)buf * MG_A_BYTES + (uint32_t)wave * 1024u;
#pragma unroll
        for (int r = 0; r < 4; ++r) mx4_dma(asrc[r] + (size_t)kt * 128, base + (uint32_t)r * 4096u);
    };
    auto stage_b = [&](int kb, int buf) {
        const uint32_t base = lds0 + MG_B_OFF + (uint32_t)buf * MG_B_BYTES + (uint32_t)wave * 1024u;
#pragma unroll
        for (int r = 0; r < 2; ++r) mx4_dma(bsrc[r] + (size_t)kb * 1024, base + (uint32_t)r * 4096u);
    };
    auto stage_s = [&](int chunk, int buf) {
        const uint32_t base = lds0 + MG_S_OFF + (uint32_t)buf * MG_S_BYTES + (uint32_t)wave * 1024u;
        const int kb = min(16 * chunk + (lane >> 2), nkb - 1);
#pragma unroll
        for (int r = 0; r < 2; ++r) mx4_dma(ssrc[r] + (size_t)kb * 64, base + (uint32_t)r * 4096u);
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
        const uint8_t* B = mg_lds + MG_B_OFF + (size_t)(kb & 1) * MG_B_BYTES;
        const uint8_t* S = mg_lds + MG_S_OFF + (size_t)((kb >> 4) & 1) * MG_S_BYTES + (size_t)(kb & 15) * 64 + m16 * 4;
        uint32_t s4[4];
#pragma unroll
        for (int h = 0; h < 2; ++h) {                                    // K step 2 kb + h: A buffer h
            if (h == 0) {
                stage_a(2 * kb + 1, 1);
                if (kb + 1 < nkb) stage_b(kb + 1, (kb + 1) & 1);
                if ((kb & 15) == 0 && kb + 16 < nkb) stage_s((kb >> 4) + 1, ((kb >> 4) + 1) & 1);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    s4[j] = *reinterpret_cast<const uint32_t*>(S + (size_t)btile[j] * 1024);
                    bad[j] |= mx4_has_nan(s4[j]);
                }
            } else if (kb + 1 < nkb) {
                stage_a(2 * kb + 2, 0);
            }
            const uint8_t* A = mg_lds + (size_t)h * MG_A_BYTES;
            uint2 raw[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) raw[j] = *reinterpret_cast<const uint2*>(B + (size_t)((btile[j] * 64 + lane) * 16 + 8 * h));
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                uint4 af[4], bf[4];
                float sf[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) af[i] = *reinterpret_cast<const uint4*>(A + (size_t)arow[i] * 128 + (size_t)(((s2 * 4 + kg) ^ (arow[i] & 7)) * 16));
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    sf[j] = mx4_scale(s4[j], 2 * h + s2);
                    bf[j] = mx4_frag<DT>(s2 ? raw[j].y : raw[j].x, sf[j]);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {                            // (n-fragment outermost: f16 keeps four fresh accumulators live, not 16)
#pragma unroll
                    for (int i = 0; i < 4; ++i) mx4_step<DT>(y[i][j], af[i], bf[j], sf[j]);
                    // f16: an empty asm that "rewrites" this column's sums and the next column's operand, so that the next four
                    // MFMAs cannot be hoisted above this column's fmas (all 16 fresh accumulators live at once spilled to scratch)
                    if constexpr (DT != MI355_DTYPE_BF16)
                        asm volatile("" : "+v"(y[0][j]), "+v"(y[1][j]), "+v"(y[2][j]), "+v"(y[3][j]), "+v"(bf[(j + 1) & 3].x));
                }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // the next step has landed (this wave's share of it)
            __syncthreads();                                             // ... everyone's; and everyone is done reading this buffer
        }
    }
    // ---- epilogue: the lane holds tokens 4 kg + v of every m-fragment for column m16 of every n-fragment
    const float nan = __builtin_nanf("");
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
                    if (col < n_cols) mx4_epilogue<DT>(a, t, col, bad[j] ? nan : y[i][j][v], bad[j + 2] ? nan : y[i][j + 2][v]);
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int col = c0 + wc * 64 + j * 16 + m16;
                    if (col < n_cols) mx4_epilogue<DT>(a, t, col, bad[j] ? nan : y[i][j][v], 0.f);
                }
            }
        }
}

// ------------------------------------------------------------------------------------------------ repack
// checkpoint blocks [n][k/2] and scales [n][k/32] -> the two planes of the image: one thread per 16-byte chunk of the block plane (four
// dwords of a row, 32 k apart); the first n * k/128 threads also move one scale dword (a row's four groups of a k-block)
__global__ void __launch_bounds__(256) mx4_tile_kernel(const uint8_t* __restrict__ in_b, const uint8_t* __restrict__ in_s,
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
    if (o < (size_t)n * nkb) {                                                      // scale dword index = (tile * nkb + kb) * 16 + row
        const int row = (int)(o & 15);
        const size_t tk = o >> 4;
        const int kb = (int)(tk % nkb), tile = (int)(tk / nkb);
        *reinterpret_cast<uint32_t*>(out_s + o * 4) = *reinterpret_cast<const uint32_t*>(in_s + ((size_t)(tile * 16 + row) * nkb + kb) * 4);
    }
}

#ifndef MXFP4_GEMM_MIN_T
#define MXFP4_GEMM_MIN_T 33            // tokens from which a launch takes the MFMA GEMM (below: two M tiles of the streaming kernel)
#endif
static_assert(MXFP4_GEMM_MIN_T >= 2 && MXFP4_GEMM_MIN_T <= 33, "the streaming kernel has at most two M tiles");

template <int DT>
static int mxfp4_small_launch(const Mx4Args& a, hipStream_t st) {
    const int nkb = a.K >> 7, niter = (nkb + MS_NW - 1) / MS_NW;
    int G = (MS_X_BYTES / a.T - 16) / (MS_NW * 256);                   // k-blocks per wave and staging pass
    G = G < 1 ? 1 : (G > niter ? niter : G);
    const bool pair = a.epi == MI355_EPI_SILU_MUL;
    const int mt = a.T <= 16 ? 1 : 2;
    const size_t xb = (size_t)a.T * (G * MS_NW * 256 + 16), rb = (size_t)MS_NW * (pair ? 2 : 1) * mt * 256 * 4;
    const size_t lds = xb > rb ? xb : rb;
    const dim3 grid((pair ? a.pair_offset : a.N) / 16), block(64 * MS_NW);
#define MS_GO(MT_, R_) do { \
        static Mi355DevOnce attr_; \
        if (!attr_.done()) { (void)hipFuncSetAttribute((const void*)mxfp4_small_kernel<DT, MT_, R_>, hipFuncAttributeMaxDynamicSharedMemorySize, MS_X_BYTES); attr_.set(); } \
        hipLaunchKernelGGL((mxfp4_small_kernel<DT, MT_, R_>), grid, block, lds, st, a, G); \
    } while (0)
    if (mt == 1) { if (pair) MS_GO(1, 2); else MS_GO(1, 1); }
    else { if (pair) MS_GO(2, 2); else MS_GO(2, 1); }
#undef MS_GO
    return (int)hipGetLastError();
}
template <int DT>
static int mxfp4_gemm_launch(const Mx4Args& a, hipStream_t st) {
    static Mi355DevOnce attr;
    if (!attr.done()) {
        (void)hipFuncSetAttribute((const void*)mxfp4_gemm_kernel<DT>, hipFuncAttributeMaxDynamicSharedMemorySize, MG_LDS);
        attr.set();
    }
    const bool pair = a.epi == MI355_EPI_SILU_MUL;
    const int n_cols = pair ? a.pair_offset : a.N, per = pair ? 64 : 128;
    hipLaunchKernelGGL((mxfp4_gemm_kernel<DT>), dim3((a.T + 127) / 128, (n_cols + per - 1) / per), dim3(256), MG_LDS, st, a);
    return (int)hipGetLastError();
}
// Route: the shape of fp8_run.  Up to 32 tokens the streaming kernel.  Above, the GEMM -- when its grid has at least MXFP4_GEMM_MIN_WGS
// workgroups or the launch has more than MXFP4_CHUNK_MAX_T tokens; a few-tile launch below that (down: 32 column tiles) runs as 32-token
// chunks of the streaming kernel.  The three thresholds are FP8's until the measurement of DESIGN.md 5d says otherwise;
// MXFP4_GEMM_MIN_T and MXFP4_GEMM_MIN_WGS are build-time switches for measuring them both ways.
#ifndef MXFP4_GEMM_MIN_WGS
#define MXFP4_GEMM_MIN_WGS 128
#endif
#define MXFP4_CHUNK_MAX_T 96
template <int DT>
static int mxfp4_run(const Mx4Args& a, hipStream_t st) {
    if (a.T < MXFP4_GEMM_MIN_T) return mxfp4_small_launch<DT>(a, st);
    const bool pair = a.epi == MI355_EPI_SILU_MUL;
    const int n_cols = pair ? a.pair_offset : a.N, per = pair ? 64 : 128;
    const int64_t wgs = (int64_t)((a.T + 127) / 128) * ((n_cols + per - 1) / per);
    if (a.T > MXFP4_CHUNK_MAX_T || wgs >= MXFP4_GEMM_MIN_WGS) return mxfp4_gemm_launch<DT>(a, st);
    for (int t0 = 0; t0 < a.T; t0 += MXFP4_GEMM_MIN_T - 1) {
        Mx4Args c = a;
        c.T = a.T - t0 < MXFP4_GEMM_MIN_T - 1 ? a.T - t0 : MXFP4_GEMM_MIN_T - 1;
        c.x = static_cast<const uint16_t*>(a.x) + (size_t)t0 * a.K;
        c.out = static_cast<uint16_t*>(a.out) + (size_t)t0 * a.ldo;
        if (a.resid) c.resid = static_cast<const uint16_t*>(a.resid) + (size_t)t0 * a.ldo;
        const int rc = mxfp4_small_launch<DT>(c, st);
        if (rc) return rc;
    }
    return 0;
}

extern "C" {

int mi355_mxfp4_tile_repack(const void* in_blocks, const void* in_scales, void* out_tiles, void* out_scales, int32_t n, int32_t k, int64_t stream) {
    if (!in_blocks || !in_scales || !out_tiles || !out_scales || in_blocks == out_tiles || in_scales == out_scales) return (int)hipErrorInvalidValue;
    if (n <= 0 || k <= 0 || (n & 15) || (k & 127)) return (int)hipErrorInvalidValue;
    if (((uintptr_t)in_blocks & 3) || ((uintptr_t)in_scales & 3) || ((uintptr_t)out_tiles & 15) || ((uintptr_t)out_scales & 3)) return (int)hipErrorInvalidValue;
    const size_t chunks = (size_t)n * k / 32;
    hipLaunchKernelGGL(mx4_tile_kernel, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const uint8_t*>(in_blocks), static_cast<const uint8_t*>(in_scales), static_cast<uint8_t*>(out_tiles),
                       static_cast<uint8_t*>(out_scales), n, k);
    return (int)hipGetLastError();
}

int mi355_mxfp4_linear_tiled(void* out, const void* x, const void* w_tiled, const void* s_tiled, const void* bias, const void* residual,
                             int32_t num_tokens, int32_t n, int32_t k, int32_t group, int32_t dtype, int32_t epilogue, int64_t stream) {
    if (!out || !x || !w_tiled || !s_tiled || num_tokens < 1 || n <= 0 || k <= 0) return (int)hipErrorInvalidValue;
    if (((uintptr_t)x & 15) || ((uintptr_t)w_tiled & 15) || ((uintptr_t)s_tiled & 15)) return (int)hipErrorInvalidValue;
    if (epilogue != MI355_EPI_STORE && epilogue != MI355_EPI_RESID && epilogue != MI355_EPI_SILU_MUL) return (int)hipErrorInvalidValue;
    if (epilogue == MI355_EPI_RESID && !residual) return (int)hipErrorInvalidValue;
    if (group != 32 || (k & 127) || (n & 15)) return (int)hipErrorNotSupported;
    if (epilogue == MI355_EPI_SILU_MUL && (n & 31)) return (int)hipErrorNotSupported;        // gate and up are whole 16-row tiles
    if (dtype != MI355_DTYPE_BF16 && dtype != MI355_DTYPE_F16) return (int)hipErrorNotSupported;
    Mx4Args a{};
    a.w = static_cast<const uint8_t*>(w_tiled); a.s = static_cast<const uint8_t*>(s_tiled); a.x = x; a.out = out; a.bias = bias; a.resid = residual;
    a.T = num_tokens; a.N = n; a.K = k; a.epi = epilogue;
    if (epilogue == MI355_EPI_SILU_MUL) { a.pair_offset = n / 2; a.ldo = n / 2; } else a.ldo = n;
    return dtype == MI355_DTYPE_BF16 ? mxfp4_run<MI355_DTYPE_BF16>(a, (hipStream_t)stream) : mxfp4_run<MI355_DTYPE_F16>(a, (hipStream_t)stream);
}

}  // extern "C"
