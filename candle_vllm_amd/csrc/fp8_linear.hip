// FP8 (OCP e4m3fn) block-scaled linears for the safetensors path: `LnFp8` (src/openai/models/linear.rs:918-1221), the layer the
// official *-FP8 exports (Qwen3, DeepSeek, ...) load.  The weight is [out, in] e4m3fn bytes with one f32 scale per 128 x 128 block
// (`weight_scale` / `weight_scale_inv`, [ceil(out/128)][in/128]):
//     y[t, r] = round_dt( sum_c x[t, c] * e4m3(w[r, c]) * s[r/128, c/128] )        (+ bias, + the fused epilogues of mi355_linear)
// W8A16: every e4m3 value is exact in bf16 and in f16, so the weight operand is decoded without rounding (one v_cvt_pk_f32_fp8 per
// byte pair, then the upper halves / a round-to-zero pack that cannot round); the activations stay 16-bit; each 128-wide k run is
// accumulated by v_mfma_f32_16x16x32_{bf16,f16} in an accumulator of its own and folded into the running sum with ONE f32 fma per
// accumulator register and the block's scale (a 16-row tile never straddles a scale row: the scale is one scalar per (tile, 128 k)).
//
// Tile image (mi355_fp8_tile_repack; fp8_tile_kernel below writes it): 16-row x 128-k tiles of 2 KiB,
//     [tile n/16][k-block k/128][half (k%128)/64][lane = 16 * ((k%32)/8) + n%16][16 B = [(k%64)/32][k%8]]
// -- a lane's 16 bytes of a half are its two B fragments (8 consecutive k of row n%16) of the two 32-k MFMA steps of that half:
// one dwordx4 per lane and half, every wave instruction one contiguous KiB, a (tile, k-block) 2 contiguous KiB, a tile's k-blocks
// back to back.  The prompt GEMM copies the same KiB runs into LDS verbatim (as bytes) and decodes when it reads a fragment.
//
// Two kernels:
//   fp8_small_kernel  1..32 tokens: streaming mat-vec, the weights never touch LDS (register ring, FS_RING k-blocks ahead)
//   fp8_gemm_kernel   33.. tokens: 128 x 128 MFMA tile, both operands global -> LDS by DMA, the weight side as bytes
// (33..96 tokens with too few GEMM tiles to fill the chip: 32-token chunks of the first -- fp8_run at the end of the file)
#include "fp8_decode.h"
#include "../../include/mi355_vllm.h"
#include <hip/hip_runtime.h>

struct Fp8Args {
    const uint8_t* w;         // tiled image
    const float* scale;       // [ceil(N/128)][K/128]
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
__device__ __forceinline__ void fp8l_epilogue(const Fp8Args& a, const int t, const int col, const float y, const float up) {
    const uint16_t* b16 = static_cast<const uint16_t*>(a.bias);
    float o = fp8l_rnd<DT>(y);
    if (b16) o = fp8l_rnd<DT>(o + fp8l_h2f<DT>(b16[col]));
    if (a.epi == MI355_EPI_SILU_MUL) {
        float u = fp8l_rnd<DT>(up);
        if (b16) u = fp8l_rnd<DT>(u + fp8l_h2f<DT>(b16[a.pair_offset + col]));
        o = fp8l_rnd<DT>(fp8l_rnd<DT>(o / (1.f + __expf(-o))) * u);
    } else if (a.epi == MI355_EPI_RESID) {
        o = fp8l_rnd<DT>(o + fp8l_h2f<DT>(static_cast<const uint16_t*>(a.resid)[(size_t)t * a.ldo + col]));
    }
    static_cast<uint16_t*>(a.out)[(size_t)t * a.ldo + col] = fp8l_f2h<DT>(o);
}

// ------------------------------------------------------------------------------------------------ 1..32 tokens
// One workgroup = R row tiles (R = 2: a gate tile and its up tile) x all of K, FS_NW waves; wave w owns the k-blocks w, w + NW, ...
//   * weights: global -> registers in image order, a ring of FS_RING k-blocks per wave (2 dwordx4 per lane, tile and k-block; the
//     block's scale rides along as a scalar) -- with 8 waves x 4 k-blocks x 2 KiB a workgroup keeps 64 KiB (R = 2: 128) in flight;
//   * activations: staged in LDS by all threads, coalesced, G k-blocks per wave at a time (as much of K as fits FS_X_BYTES: at one
//     token all of K up to 31744 -- once per workgroup; at 32 tokens one k-block per wave and pass); rows padded by 16 B so that the
//     16 rows of an A-fragment read start on different bank quads;
//   * MT = ceil(T / 16) M tiles; the 128-k run goes into a fresh accumulator, then y += s * acc;
//   * cross-wave reduction through LDS (over the staging area), epilogue out of the sums.
constexpr int FS_NW = 8, FS_RING = 4;
constexpr int FS_X_BYTES = 32 * (FS_NW * 256 + 16);        // 66048: 32 tokens x one k-block per wave; two workgroups per CU

template <int DT, int MT, int R>
__global__ void __launch_bounds__(64 * FS_NW) fp8_small_kernel(const Fp8Args a, const int G) {
    extern __shared__ __attribute__((aligned(16))) uint8_t fs_lds[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r16 = lane & 15, kg = lane >> 4;
    const int T = a.T, nkb = a.K >> 7;
    const int niter = (nkb + FS_NW - 1) / FS_NW;            // the same for every wave (the barriers below)
    const int ldx = G * FS_NW * 256 + 16;                   // bytes per staged row
    int row0[R];
    row0[0] = (int)blockIdx.x * 16;
    if (R == 2) row0[R - 1] = a.pair_offset + (int)blockIdx.x * 16;
    const uint8_t* wp[R];
    const float* sp[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        wp[r] = a.w + ((size_t)(row0[r] >> 4) * nkb) * 2048 + lane * 16;
        sp[r] = a.scale + (size_t)(row0[r] >> 7) * nkb;
    }
    uint4 ring[FS_RING][R][2];
    float rs[FS_RING][R];
    // (past the end of K the last k-block is fetched again and not used)
#define FS_LOAD(SLOT_, I_) do { \
        const int kb_ = min(wave + (I_) * FS_NW, nkb - 1); \
        _Pragma("unroll") for (int r_ = 0; r_ < R; ++r_) { \
            const fp8l_u32x4* p_ = reinterpret_cast<const fp8l_u32x4*>(wp[r_] + (size_t)kb_ * 2048); \
            const fp8l_u32x4 v0_ = __builtin_nontemporal_load(p_), v1_ = __builtin_nontemporal_load(p_ + 64); \
            ring[SLOT_][r_][0] = make_uint4(v0_.x, v0_.y, v0_.z, v0_.w); \
            ring[SLOT_][r_][1] = make_uint4(v1_.x, v1_.y, v1_.z, v1_.w); \
            rs[SLOT_][r_] = sp[r_][kb_]; \
        } \
    } while (0)
#pragma unroll
    for (int s = 0; s < FS_RING; ++s) FS_LOAD(s, s);

    f32x4_t y[R][MT];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) y[r][mt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    const f32x4_t zero4 = {0.f, 0.f, 0.f, 0.f};
    const uint8_t* xg = static_cast<const uint8_t*>(a.x);
    const int pass_cols = G * FS_NW * 128;                  // k columns of one staging pass

    for (int i0 = 0; i0 < niter; i0 += FS_RING) {
#pragma unroll
        for (int s = 0; s < FS_RING; ++s) {
            const int i = i0 + s;
            if (i < niter) {                                 // (uniform over the workgroup)
                const int g = i % G;
                if (g == 0) {
                    // ---- the activations of the next G k-blocks of every wave: columns [c0, c0 + pass_cols) of x
                    const int c0 = (i / G) * pass_cols, cols = min(pass_cols, a.K - c0), ppr = cols >> 3;      // 16-byte pieces per row
                    __syncthreads();                         // everyone is done with the previous pass
                    for (int p = threadIdx.x; p < T * ppr; p += 64 * FS_NW) {
                        const int t = p / ppr, c = p - t * ppr;
                        *reinterpret_cast<uint4*>(fs_lds + (size_t)t * ldx + c * 16) =
                            *reinterpret_cast<const uint4*>(xg + ((size_t)t * a.K + c0) * 2 + c * 16);
                    }
                    __syncthreads();
                }
                const int kb = wave + i * FS_NW;
                if (kb < nkb) {
                    const uint8_t* xl = fs_lds + (size_t)(g * FS_NW + wave) * 256 + 16 * kg;                    // this k-block inside the pass
                    f32x4_t acc[R][MT];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        uint4 af[MT], bf[R];
#pragma unroll
                        for (int mt = 0; mt < MT; ++mt)
                            af[mt] = *reinterpret_cast<const uint4*>(xl + (size_t)min(mt * 16 + r16, T - 1) * ldx + 64 * j);
#pragma unroll
                        for (int r = 0; r < R; ++r) {
                            const uint4 v = ring[s][r][j >> 1];
                            bf[r] = (j & 1) ? fp8l_frag<DT>(v.z, v.w) : fp8l_frag<DT>(v.x, v.y);
                        }
#pragma unroll
                        for (int r = 0; r < R; ++r)
#pragma unroll
                            for (int mt = 0; mt < MT; ++mt) acc[r][mt] = fp8l_mfma<DT>(af[mt], bf[r], j == 0 ? zero4 : acc[r][mt]);
                    }
#pragma unroll
                    for (int r = 0; r < R; ++r)
#pragma unroll
                        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                            for (int v = 0; v < 4; ++v) y[r][mt][v] = fmaf(rs[s][r], acc[r][mt][v], y[r][mt][v]);
                }
                FS_LOAD(s, i + FS_RING);
            }
        }
    }
#undef FS_LOAD
    // ---- cross-wave reduction: C layout = lane (column = weight row r16, rows m = 4 kg + v)
    float* red = reinterpret_cast<float*>(fs_lds);          // [NW][R][MT][16 m][16 rows]
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int v = 0; v < 4; ++v) red[(((wave * R + r) * MT + mt) * 16 + 4 * kg + v) * 16 + r16] = y[r][mt][v];
    __syncthreads();
    for (int idx = threadIdx.x; idx < MT * 256; idx += 64 * FS_NW) {
        const int rr = idx & 15, m = idx >> 4;
        if (m >= T) continue;
        float val[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            float s = 0.f;
#pragma unroll
            for (int w = 0; w < FS_NW; ++w) s += red[(((w * R + r) * MT + (m >> 4)) * 16 + (m & 15)) * 16 + rr];
            val[r] = s;
        }
        fp8l_epilogue<DT>(a, m, row0[0] + rr, val[0], val[R - 1]);
    }
}

// ------------------------------------------------------------------------------------------------ prompt steps
// Workgroup tile 128 tokens x 128 weight rows (SILU_MUL: 64 gate rows and the 64 matching up rows), 4 waves as 2 x 2, wave tile
// 64 x 64 (4 x 4 fragments), two workgroups per CU.  K in steps of 64, two LDS buffers, the DMA of step t + 1 in flight while step t is
// multiplied (one counted wait + one barrier per step), as dense_gemm_kernel:
//   * x: 128 rows x 128 B per step, 16-byte slot c of row r at slot c ^ (r & 7) (applied to the lane's global source address);
//   * weights: 8 row tiles x 1 KiB per step, the image's KiB runs copied verbatim -- 8 KiB per step instead of the 16 KiB of a 16-bit
//     tile; a lane's two B fragments of the step are ONE ds_read_b128 of its own 16 bytes, decoded in registers and used by four
//     m-fragments each;
//   * scales: the panel [8 row tiles][K / 128] staged in LDS once per workgroup (no global load the compiler could see inside the K
//     loop); two K steps = one scale block: their products go into `acc`, then y += s * acc per fragment (the scale is
//     wave-uniform per fragment and block: a fragment's 16 rows sit in one scale row).
constexpr uint32_t FG_A_BYTES = 128 * 128, FG_B_BYTES = 8 * 1024, FG_STAGE = FG_A_BYTES + FG_B_BYTES;
constexpr int FG_MAX_NKB = 512;                              // scale panel: 8 x 512 x 4 B = 16 KiB at most (K <= 65536)

template <int DT>
__global__ void __launch_bounds__(256, 2) fp8_gemm_kernel(const Fp8Args a) {
    extern __shared__ __attribute__((aligned(1024))) uint8_t fg_lds[];   // [2 buffers][A 16 KiB | B 8 KiB] [scale panel]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave >> 1, wc = wave & 1;
    const int m16 = lane & 15, kg = lane >> 4;
    const bool silu = a.epi == MI355_EPI_SILU_MUL;
    const int nkb = a.K >> 7, nkt = a.K >> 6;
    const int t0 = (int)blockIdx.x * 128;                                // token tiles fastest: neighbours share their weight tile through L2
    const int n_cols = silu ? a.pair_offset : a.N;
    const int c0 = (int)blockIdx.y * (silu ? 64 : 128);
    // first weight row of LDS row tile p (clamped: columns beyond the matrix are computed and never stored)
    auto tile_row = [&](int p) {
        if (!silu) return min(c0 + 16 * p, a.N - 16);
        return p < 4 ? min(c0 + 16 * p, a.pair_offset - 16) : min(a.pair_offset + c0 + 16 * (p - 4), a.N - 16);
    };
    const uint32_t lds0 = __builtin_amdgcn_readfirstlane((uint32_t)(size_t)(__attribute__((address_space(3))) void*)fg_lds);
    float* const panel = reinterpret_cast<float*>(fg_lds + 2 * FG_STAGE);
    for (int i = tid; i < 8 * nkb; i += 256) {
        const int p = i / nkb, kb = i - p * nkb;
        panel[i] = a.scale[(size_t)(tile_row(p) >> 7) * nkb + kb];
    }
    // staging sources: A round r = rows 32 r + tid / 8 (8 threads = the 8 slots of a row, one wave = 8 rows = 1 KiB); B piece 4 r + wave
    const int srow = tid >> 3, sslot = tid & 7;
    const uint8_t* asrc[4];
    const uint8_t* bsrc[2];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = 32 * r + srow;
        asrc[r] = static_cast<const uint8_t*>(a.x) + ((size_t)min(t0 + row, a.T - 1) * a.K) * 2 + (size_t)((sslot ^ (row & 7)) * 16);
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) bsrc[r] = a.w + ((size_t)(tile_row(4 * r + wave) >> 4) * nkb) * 2048 + lane * 16;
    auto stage = [&](int kt, int buf) {
        const uint32_t base = lds0 + (uint32_t)buf * FG_STAGE + (uint32_t)wave * 1024u;
#pragma unroll
        for (int r = 0; r < 4; ++r) fp8l_dma(asrc[r] + (size_t)kt * 128, base + (uint32_t)r * 4096u);
#pragma unroll
        for (int r = 0; r < 2; ++r) fp8l_dma(bsrc[r] + (size_t)kt * 1024, base + FG_A_BYTES + (uint32_t)r * 4096u);
    };
    const f32x4_t zero4 = {0.f, 0.f, 0.f, 0.f};
    f32x4_t y[4][4], acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) y[i][j] = zero4;
    // this wave's fragments: A rows, B row tiles (SILU_MUL: fragments 0, 1 = gate columns, 2, 3 = the same columns of up)
    int arow[4], btile[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) arow[i] = wr * 64 + i * 16 + m16;
#pragma unroll
    for (int j = 0; j < 4; ++j) btile[j] = silu ? ((j >> 1) * 4 + wc * 2 + (j & 1)) : (wc * 4 + j);

    stage(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int kb = 0; kb < nkb; ++kb) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int kt = 2 * kb + h;                                   // (kt & 1 == h: the buffer index is static)
            if (kt + 1 < nkt) stage(kt + 1, h ^ 1);
            const uint8_t* A = fg_lds + (size_t)h * FG_STAGE;
            const uint8_t* B = A + FG_A_BYTES;
            uint4 raw[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) raw[j] = *reinterpret_cast<const uint4*>(B + (size_t)((btile[j] * 64 + lane) * 16));
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                uint4 af[4], bf[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) af[i] = *reinterpret_cast<const uint4*>(A + (size_t)arow[i] * 128 + (size_t)(((s2 * 4 + kg) ^ (arow[i] & 7)) * 16));
#pragma unroll
                for (int j = 0; j < 4; ++j) bf[j] = s2 ? fp8l_frag<DT>(raw[j].z, raw[j].w) : fp8l_frag<DT>(raw[j].x, raw[j].y);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = fp8l_mfma<DT>(af[i], bf[j], (h == 0 && s2 == 0) ? zero4 : acc[i][j]);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // the next step has landed (this wave's share of it)
            __syncthreads();                                             // ... everyone's; and everyone is done reading this buffer
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float s = panel[btile[j] * nkb + kb];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int v = 0; v < 4; ++v) y[i][j][v] = fmaf(s, acc[i][j][v], y[i][j][v]);
        }
    }
    // ---- epilogue: the lane holds tokens 4 kg + v of every m-fragment for column m16 of every n-fragment
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
                    if (col < n_cols) fp8l_epilogue<DT>(a, t, col, y[i][j][v], y[i][j + 2][v]);
                }
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int col = c0 + wc * 64 + j * 16 + m16;
                    if (col < n_cols) fp8l_epilogue<DT>(a, t, col, y[i][j][v], 0.f);
                }
            }
        }
}

// ------------------------------------------------------------------------------------------------ repack
// checkpoint bytes [n][k] -> the tiled image: one thread per 16-byte chunk of the output (two 8-byte pieces of a row, 32 k apart)
__global__ void __launch_bounds__(256) fp8_tile_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int n, int k) {
    const size_t o = (size_t)blockIdx.x * blockDim.x + threadIdx.x;                 // chunk index = ((tile * nkb + kb) * 2 + half) * 64 + lane
    const int nkb = k >> 7;
    if (o >= (size_t)(n >> 4) * nkb * 128) return;
    const int lane = (int)(o & 63), half = (int)((o >> 6) & 1);
    const size_t tk = o >> 7;
    const int kb = (int)(tk % nkb), tile = (int)(tk / nkb);
    const uint8_t* src = in + (size_t)(tile * 16 + (lane & 15)) * k + kb * 128 + half * 64 + (lane >> 4) * 8;
    const uint2 lo = *reinterpret_cast<const uint2*>(src), hi = *reinterpret_cast<const uint2*>(src + 32);
    *reinterpret_cast<uint4*>(out + o * 16) = make_uint4(lo.x, lo.y, hi.x, hi.y);
}

#ifndef FP8_GEMM_MIN_T
#define FP8_GEMM_MIN_T 33              // tokens from which a launch takes the MFMA GEMM (below: two M tiles of the streaming kernel)
#endif
static_assert(FP8_GEMM_MIN_T >= 2 && FP8_GEMM_MIN_T <= 33, "the streaming kernel has at most two M tiles");

template <int DT>
static int fp8_small_launch(const Fp8Args& a, hipStream_t st) {
    const int nkb = a.K >> 7, niter = (nkb + FS_NW - 1) / FS_NW;
    int G = (FS_X_BYTES / a.T - 16) / (FS_NW * 256);                   // k-blocks per wave and staging pass
    G = G < 1 ? 1 : (G > niter ? niter : G);
    const bool pair = a.epi == MI355_EPI_SILU_MUL;
    const int mt = a.T <= 16 ? 1 : 2;
    const size_t xb = (size_t)a.T * (G * FS_NW * 256 + 16), rb = (size_t)FS_NW * (pair ? 2 : 1) * mt * 256 * 4;
    const size_t lds = xb > rb ? xb : rb;
    const dim3 grid((pair ? a.pair_offset : a.N) / 16), block(64 * FS_NW);
#define FS_GO(MT_, R_) do { \
        static Mi355DevOnce attr_; \
        if (!attr_.done()) { (void)hipFuncSetAttribute((const void*)fp8_small_kernel<DT, MT_, R_>, hipFuncAttributeMaxDynamicSharedMemorySize, FS_X_BYTES); attr_.set(); } \
        hipLaunchKernelGGL((fp8_small_kernel<DT, MT_, R_>), grid, block, lds, st, a, G); \
    } while (0)
    if (mt == 1) { if (pair) FS_GO(1, 2); else FS_GO(1, 1); }
    else { if (pair) FS_GO(2, 2); else FS_GO(2, 1); }
#undef FS_GO
    return (int)hipGetLastError();
}
template <int DT>
static int fp8_gemm_launch(const Fp8Args& a, hipStream_t st) {
    const int nkb = a.K >> 7;
    if (nkb > FG_MAX_NKB) return (int)hipErrorNotSupported;
    const size_t lds = 2 * FG_STAGE + (size_t)8 * nkb * 4;
    static Mi355DevOnce attr;
    if (!attr.done()) {
        (void)hipFuncSetAttribute((const void*)fp8_gemm_kernel<DT>, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * FG_STAGE + 8 * FG_MAX_NKB * 4);
        attr.set();
    }
    const bool pair = a.epi == MI355_EPI_SILU_MUL;
    const int n_cols = pair ? a.pair_offset : a.N, per = pair ? 64 : 128;
    hipLaunchKernelGGL((fp8_gemm_kernel<DT>), dim3((a.T + 127) / 128, (n_cols + per - 1) / per), dim3(256), lds, st, a);
    return (int)hipGetLastError();
}
// Route (measured on Llama-3-8B shapes): up to 32 tokens the streaming kernel.  Above, the GEMM -- when its grid has at
// least FP8_GEMM_MIN_WGS workgroups or the launch has more than FP8_CHUNK_MAX_T tokens.  A few-tile launch with a long K (down: 32 column
// tiles x 14336) keeps 32 CUs busy for 142 us whatever T <= 128 is, where 32-token chunks of the streaming kernel take 37 us each (51 us at 33
// tokens, 76 at 64; 224 at 128, where the GEMM's 155 wins): such launches run in chunks up to 96 tokens (as does, at any T, a K the GEMM's
// scale panel cannot hold).
#ifndef FP8_GEMM_MIN_WGS
#define FP8_GEMM_MIN_WGS 128
#endif
#define FP8_CHUNK_MAX_T 96
template <int DT>
static int fp8_run(const Fp8Args& a, hipStream_t st) {
    if (a.T < FP8_GEMM_MIN_T) return fp8_small_launch<DT>(a, st);
    const bool pair = a.epi == MI355_EPI_SILU_MUL;
    const int n_cols = pair ? a.pair_offset : a.N, per = pair ? 64 : 128;
    const int64_t wgs = (int64_t)((a.T + 127) / 128) * ((n_cols + per - 1) / per);
    if (a.T > FP8_CHUNK_MAX_T || wgs >= FP8_GEMM_MIN_WGS) {
        const int rc = fp8_gemm_launch<DT>(a, st);
        if (rc != (int)hipErrorNotSupported) return rc;                    // K > 65536: nothing was launched, token chunks below
    }
    for (int t0 = 0; t0 < a.T; t0 += FP8_GEMM_MIN_T - 1) {
        Fp8Args c = a;
        c.T = a.T - t0 < FP8_GEMM_MIN_T - 1 ? a.T - t0 : FP8_GEMM_MIN_T - 1;
        c.x = static_cast<const uint16_t*>(a.x) + (size_t)t0 * a.K;
        c.out = static_cast<uint16_t*>(a.out) + (size_t)t0 * a.ldo;
        if (a.resid) c.resid = static_cast<const uint16_t*>(a.resid) + (size_t)t0 * a.ldo;
        const int rc = fp8_small_launch<DT>(c, st);
        if (rc) return rc;
    }
    return 0;
}

extern "C" {

int mi355_fp8_tile_repack(const void* in, void* out, int32_t n, int32_t k, int64_t stream) {
    if (!in || !out || in == out || n <= 0 || k <= 0 || (n & 15) || (k & 127) || ((uintptr_t)in & 7) || ((uintptr_t)out & 15))
        return (int)hipErrorInvalidValue;
    const size_t chunks = (size_t)n * k / 16;
    hipLaunchKernelGGL(fp8_tile_kernel, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       static_cast<const uint8_t*>(in), static_cast<uint8_t*>(out), n, k);
    return (int)hipGetLastError();
}

int mi355_fp8_linear_tiled(void* out, const void* x, const void* w_tiled, const float* w_scale, const void* bias, const void* residual,
                           int32_t num_tokens, int32_t n, int32_t k, int32_t block_n, int32_t block_k, int32_t dtype, int32_t epilogue,
                           int64_t stream) {
    if (!out || !x || !w_tiled || !w_scale || num_tokens < 1 || n <= 0 || k <= 0) return (int)hipErrorInvalidValue;
    if (((uintptr_t)x & 15) || ((uintptr_t)w_tiled & 15)) return (int)hipErrorInvalidValue;
    if (epilogue != MI355_EPI_STORE && epilogue != MI355_EPI_RESID && epilogue != MI355_EPI_SILU_MUL) return (int)hipErrorInvalidValue;
    if (epilogue == MI355_EPI_RESID && !residual) return (int)hipErrorInvalidValue;
    if (block_n != 128 || block_k != 128 || (k & 127) || (n & 15)) return (int)hipErrorNotSupported;
    if (epilogue == MI355_EPI_SILU_MUL && (n & 31)) return (int)hipErrorNotSupported;        // gate and up are whole 16-row tiles
    if (dtype != MI355_DTYPE_BF16 && dtype != MI355_DTYPE_F16) return (int)hipErrorNotSupported;
    Fp8Args a{};
    a.w = static_cast<const uint8_t*>(w_tiled); a.scale = w_scale; a.x = x; a.out = out; a.bias = bias; a.resid = residual;
    a.T = num_tokens; a.N = n; a.K = k; a.epi = epilogue;
    if (epilogue == MI355_EPI_SILU_MUL) { a.pair_offset = n / 2; a.ldo = n / 2; } else a.ldo = n;
    return dtype == MI355_DTYPE_BF16 ? fp8_run<MI355_DTYPE_BF16>(a, (hipStream_t)stream) : fp8_run<MI355_DTYPE_F16>(a, (hipStream_t)stream);
}

}  // extern "C"
