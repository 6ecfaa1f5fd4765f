// MXFP4 fused-MoE expert mat-muls: `moe::moe_gemm_mxfp4` as `FusedMoeMxfp4::forward_with_routing` calls it twice per layer
// (src/openai/models/layers/moe.rs:1782-1835) -- a grouped W4A16 GEMM over the experts' tile images (mxfp4_linear.hip's image, experts
// back to back), routed on the device.  With P = num_tokens * top_k pairs and e_p = topk_ids[p]:
//     out[p, r] = round_dt( w_p * sum_c x[p / x_div, c] * e2m1(B[e_p][r, c]) * 2^(S[e_p][r, c/32] - 127) )
// (w_p = topk_weights[p] or 1; x_div = top_k: one x row per token, the gate|up call; x_div = 1: one per pair, the down call).
// EPI_SILU_MUL takes each expert's image as that of its packed [gate; up] and writes silu(gate) * up with the dense op's rounding points.
//
// Three launches on the caller's stream, no host round trip:
//   mx4moe_plan_kernel   (moe_plan.h) topk_ids -> per-expert counts (LDS), the list of RUNS {expert, first row, rows <= M} and the row list (pair
//                        indices grouped by expert).  Ids outside [0, E) form a pseudo-expert E whose runs are written as zero rows.
//   mx4moe_small_kernel  M = 16: the streaming mould of mxfp4_small_kernel, one run's gathered pairs as one M tile
//   mx4moe_gemm_kernel   M = 64: the LDS-fed mould of mxfp4_gemm_kernel, a run of up to 64 pairs x 128 weight rows per workgroup
// The compute kernels gather x rows and scatter out rows through the row list themselves.  MFMA rows are independent, so a pair's result
// does not depend on where the plan's LDS atomics placed it inside its run: results are bit-identical between launches.
#include "moe_plan.h"
#include "mxfp4_decode.h"
#include "scratch.h"
#include "../../include/mi355_vllm.h"
#include <hip/hip_runtime.h>

struct Mx4MoeArgs {
    const uint8_t* w;         // tiled blocks, experts back to back (N * K / 2 bytes each)
    const uint8_t* s;         // tiled scales (N * K / 32 bytes each)
    const void* x;            // 16-bit [P / x_div][K]
    void* out;                // 16-bit [P][ldo]
    const float* wts;         // [P] or null
    const int32_t* plan;      // [0] = runs; run r = int4 {expert, first row, rows, -} at 4 + 4 r; the row list behind max_runs runs
    int32_t E, N, K, ldo, epi, x_div, max_runs;
    int32_t pair_offset;      // SILU_MUL: rows of `up` start here (packed [gate; up], moe.rs:1739-1741)
};

// the rounding chain of one output element: w_p * sum -> dtype, or gate -> dtype, up -> dtype, silu(gate) -> dtype, * up -> dtype
// (mxfp4_linear.hip's SILU_MUL without a bias)
template <int DT>
__device__ __forceinline__ void mx4moe_store(const Mx4MoeArgs& a, const int p, const int col, const float y, const float up) {
    uint16_t* o = static_cast<uint16_t*>(a.out) + (size_t)p * a.ldo + col;
    if (a.epi == MI355_EPI_SILU_MUL) {
        const float g = mx4_rnd<DT>(y), u = mx4_rnd<DT>(up);
        *o = mx4_f2h<DT>(mx4_rnd<DT>(g / (1.f + __expf(-g))) * u);
    } else {
        *o = mx4_f2h<DT>(a.wts ? a.wts[p] * y : y);
    }
}

// ------------------------------------------------------------------------------------------------ few pairs per expert
// mxfp4_small_kernel's mould: 8 waves own one row tile (R = 2: a gate tile and its up tile) of the RUN's expert over all of K, wave w the
// k-blocks w, w + 8, ... through a register ring of MOS_RING k-blocks (one dwordx4 + one scale dword per lane, tile and k-block); the
// weights never touch LDS, the sums meet there.  Grid (row tiles, runs); a run's pairs (<= 16) are the one M tile: their x rows are
// staged in LDS through the row list (pair / x_div), G k-blocks per wave at a time, and the epilogue scatters to row p with w_p.  An
// expert with <= 16 pairs is read once per launch; at one token there are top_k runs of one pair.
constexpr int MOS_NW = 8, MOS_RING = 8, MOS_M = 16;
constexpr int MOS_X_BYTES = 16 * (2 * MOS_NW * 256 + 16);  // 65792: 16 pairs x two k-blocks per wave; two workgroups per CU

template <int DT, int R>
__global__ void __launch_bounds__(64 * MOS_NW) mx4moe_small_kernel(const Mx4MoeArgs a, const int G) {
    extern __shared__ __attribute__((aligned(16))) uint8_t mos_lds[];
    __shared__ int xrow[MOS_M], prow[MOS_M];
    if ((int)blockIdx.y >= a.plan[0]) return;
    const int4 rd = *reinterpret_cast<const int4*>(a.plan + 4 + 4 * (size_t)blockIdx.y);
    const int e = __builtin_amdgcn_readfirstlane(rd.x), first = __builtin_amdgcn_readfirstlane(rd.y);
    const int T = __builtin_amdgcn_readfirstlane(rd.z);
    const int32_t* rows = a.plan + 4 + 4 * (size_t)a.max_runs + first;
    int row0[R];
    row0[0] = (int)blockIdx.x * 16;
    if (R == 2) row0[R - 1] = a.pair_offset + (int)blockIdx.x * 16;
    if (e >= a.E) {                                          // ids outside [0, E): zero rows, no weight read
        for (int idx = threadIdx.x; idx < T * 16; idx += 64 * MOS_NW)
            static_cast<uint16_t*>(a.out)[(size_t)rows[idx >> 4] * a.ldo + row0[0] + (idx & 15)] = 0;
        return;
    }
    if ((int)threadIdx.x < T) {
        const int p = rows[threadIdx.x];
        prow[threadIdx.x] = p;
        xrow[threadIdx.x] = p / a.x_div;
    }
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int r16 = lane & 15, kg = lane >> 4;
    const int nkb = a.K >> 7;
    const int niter = (nkb + MOS_NW - 1) / MOS_NW;          // the same for every wave (the barriers below)
    const int ldx = G * MOS_NW * 256 + 16;                  // bytes per staged row
    const uint8_t* wp[R];
    const uint8_t* sp[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const size_t tk = ((size_t)e * (a.N >> 4) + (row0[r] >> 4)) * nkb;
        wp[r] = a.w + tk * 1024 + lane * 16;
        sp[r] = a.s + tk * 64 + r16 * 4;
    }
    uint4 ring[MOS_RING][R];
    uint32_t rs[MOS_RING][R];
#define MOS_LOAD(SLOT_, I_) do { \
        const int kb_ = wave + (I_) * MOS_NW; \
        if (kb_ < nkb) { \
            _Pragma("unroll") for (int r_ = 0; r_ < R; ++r_) { \
                const mx4_u32x4 v_ = __builtin_nontemporal_load(reinterpret_cast<const mx4_u32x4*>(wp[r_] + (size_t)kb_ * 1024)); \
                ring[SLOT_][r_] = make_uint4(v_.x, v_.y, v_.z, v_.w); \
                rs[SLOT_][r_] = *reinterpret_cast<const uint32_t*>(sp[r_] + (size_t)kb_ * 64); \
            } \
        } \
    } while (0)
#pragma unroll
    for (int s = 0; s < MOS_RING; ++s) {
#pragma unroll
        for (int r = 0; r < R; ++r) { ring[s][r] = make_uint4(0u, 0u, 0u, 0u); rs[s][r] = 0u; }
        MOS_LOAD(s, s);
    }

    f32x4_t y[R];
    uint32_t bad[R];
#pragma unroll
    for (int r = 0; r < R; ++r) { bad[r] = 0u; y[r] = f32x4_t{0.f, 0.f, 0.f, 0.f}; }
    const uint8_t* xg = static_cast<const uint8_t*>(a.x);
    const int pass_cols = G * MOS_NW * 128;                 // k columns of one staging pass

    for (int i0 = 0; i0 < niter; i0 += MOS_RING) {
#pragma unroll
        for (int s = 0; s < MOS_RING; ++s) {
            const int i = i0 + s;
            if (i < niter) {                                 // (uniform over the workgroup)
                const int g = i % G;
                if (g == 0) {
                    // ---- the gathered activations of the next G k-blocks of every wave: columns [c0, c0 + pass_cols) of the run's x rows
                    const int c0 = (i / G) * pass_cols, cols = min(pass_cols, a.K - c0), ppr = cols >> 3;      // 16-byte pieces per row
                    __syncthreads();                         // everyone is done with the previous pass (first pass: xrow is written)
                    for (int p = threadIdx.x; p < T * ppr; p += 64 * MOS_NW) {
                        const int t = p / ppr, c = p - t * ppr;
                        *reinterpret_cast<uint4*>(mos_lds + (size_t)t * ldx + c * 16) =
                            *reinterpret_cast<const uint4*>(xg + ((size_t)xrow[t] * a.K + c0) * 2 + c * 16);
                    }
                    __syncthreads();
                }
                const int kb = wave + i * MOS_NW;
                if (kb < nkb) {
                    const uint8_t* xl = mos_lds + (size_t)(g * MOS_NW + wave) * 256 + 16 * kg;                  // this k-block inside the pass
#pragma unroll
                    for (int r = 0; r < R; ++r) bad[r] |= mx4_has_nan(rs[s][r]);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const uint4 af = *reinterpret_cast<const uint4*>(xl + (size_t)min(r16, T - 1) * ldx + 64 * j);
#pragma unroll
                        for (int r = 0; r < R; ++r) {
                            const float sf = mx4_scale(rs[s][r], j);
                            mx4_step<DT>(y[r], af, mx4_frag<DT>(mx4_dword(ring[s][r], j), sf), sf);
                        }
                    }
                }
                MOS_LOAD(s, i + MOS_RING);
            }
        }
    }
#undef MOS_LOAD
    // ---- cross-wave reduction: C layout = lane (column = weight row r16, rows m = 4 kg + v)
    float* red = reinterpret_cast<float*>(mos_lds);         // [NW][R][16 m][16 rows]
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int v = 0; v < 4; ++v) red[((wave * R + r) * 16 + 4 * kg + v) * 16 + r16] = bad[r] ? __builtin_nanf("") : y[r][v];
    __syncthreads();
    if (threadIdx.x < 256) {
        const int rr = threadIdx.x & 15, m = threadIdx.x >> 4;
        if (m >= T) return;
        float val[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            float s = 0.f;
#pragma unroll
            for (int w = 0; w < MOS_NW; ++w) s += red[((w * R + r) * 16 + m) * 16 + rr];
            val[r] = s;
        }
        mx4moe_store<DT>(a, prow[m], row0[0] + rr, val[0], val[R - 1]);
    }
}

// ------------------------------------------------------------------------------------------------ many pairs per expert
// mxfp4_gemm_kernel's mould (global_load_lds_dwordx4 one 64-k step ahead, the weight side as packed nibbles in two buffers that turn
// over once per k-block, 16 k-blocks of scales riding the same DMA, the activation side swizzled), re-cut for experts: an expert owns
// about P / E rows, so the workgroup tile is one run of up to 64 pairs x 128 weight rows (SILU_MUL: 64 gate rows and the 64 matching up
// rows).  4 waves side by side along N: a wave owns all 64 pairs x 2 row tiles (4 x 2 fragments, 32 accumulator registers), so every
// packed B fragment is decoded by exactly one wave (2 x 2 waves would decode each twice) and with SILU_MUL a wave holds a gate tile and
// its own up tile.  LDS: A 2 x 8 KiB + B 2 x 8 KiB + scales 2 x 8 KiB + the run's 64 row-list entries = 48.25 KiB.
//   * A: the lane's global source address of row r comes from the row list in LDS (pair / x_div), so the gather is the DMA itself; rows
//     beyond the run re-read its last row and are masked at the store;
//   * the epilogue scatters row t of the tile to out row p = row list[t] with w_p.
constexpr uint32_t MOG_M = 64;
constexpr uint32_t MOG_A_BYTES = MOG_M * 128, MOG_B_BYTES = 8 * 1024, MOG_S_BYTES = 8 * 1024;
constexpr uint32_t MOG_B_OFF = 2 * MOG_A_BYTES, MOG_S_OFF = MOG_B_OFF + 2 * MOG_B_BYTES, MOG_ROW_OFF = MOG_S_OFF + 2 * MOG_S_BYTES;
constexpr uint32_t MOG_LDS = MOG_ROW_OFF + MOG_M * 4;

template <int DT>
__global__ void __launch_bounds__(256, 2) mx4moe_gemm_kernel(const Mx4MoeArgs a) {
    extern __shared__ __attribute__((aligned(1024))) uint8_t mog_lds[];  // [A 2 x 8 KiB][B 2 x 8 KiB][scales 2 x 8 KiB][row list]
    if ((int)blockIdx.y >= a.plan[0]) return;
    const int4 rd = *reinterpret_cast<const int4*>(a.plan + 4 + 4 * (size_t)blockIdx.y);
    const int e = __builtin_amdgcn_readfirstlane(rd.x), first = __builtin_amdgcn_readfirstlane(rd.y);
    const int T = __builtin_amdgcn_readfirstlane(rd.z);
    const int32_t* rows = a.plan + 4 + 4 * (size_t)a.max_runs + first;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m16 = lane & 15, kg = lane >> 4;
    const bool silu = a.epi == MI355_EPI_SILU_MUL;
    const int nkb = a.K >> 7;
    const int n_cols = silu ? a.pair_offset : a.N, per = silu ? 64 : 128;
    const int c0 = (int)blockIdx.x * per;                                // row tiles fastest: neighbours share their run's x rows through L2
    if (e >= a.E) {                                                      // ids outside [0, E): zero rows, no weight read
        for (int idx = tid; idx < T * per; idx += 256) {
            const int col = c0 + idx % per;
            if (col < n_cols) static_cast<uint16_t*>(a.out)[(size_t)rows[idx / per] * a.ldo + col] = 0;
        }
        return;
    }
    int* lrow = reinterpret_cast<int*>(mog_lds + MOG_ROW_OFF);
    if (tid < (int)MOG_M) lrow[tid] = rows[min(tid, T - 1)];
    __syncthreads();
    // first weight row of LDS row tile p (clamped: columns beyond the matrix are computed and never stored)
    auto tile_row = [&](int p) {
        if (!silu) return min(c0 + 16 * p, a.N - 16);
        return p < 4 ? min(c0 + 16 * p, a.pair_offset - 16) : min(a.pair_offset + c0 + 16 * (p - 4), a.N - 16);
    };
    const uint32_t lds0 = __builtin_amdgcn_readfirstlane((uint32_t)(size_t)(__attribute__((address_space(3))) void*)mog_lds);
    // staging sources: A round r = rows 32 r + tid / 8 (8 threads = the 8 slots of a row, one wave = 8 rows = 1 KiB); B and scale piece 4 r + wave
    const int srow = tid >> 3, sslot = tid & 7;
    const uint8_t* asrc[2];
    const uint8_t* bsrc[2];
    const uint8_t* ssrc[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int row = 32 * r + srow;
        asrc[r] = static_cast<const uint8_t*>(a.x) + ((size_t)(lrow[row] / a.x_div) * a.K) * 2 + (size_t)((sslot ^ (row & 7)) * 16);
        const size_t tk = ((size_t)e * (a.N >> 4) + (tile_row(4 * r + wave) >> 4)) * nkb;
        bsrc[r] = a.w + tk * 1024 + lane * 16;
        ssrc[r] = a.s + tk * 64 + (lane & 3) * 16;                       // + 64 * k-block (lane / 4 of the chunk of 16)
    }
    auto stage_a = [&](int kt, int buf) {
        const uint32_t base = lds0 + (uint32_t)buf * MOG_A_BYTES + (uint32_t)wave * 1024u;
#pragma unroll
        for (int r = 0; r < 2; ++r) mx4_dma(asrc[r] + (size_t)kt * 128, base + (uint32_t)r * 4096u);
    };
    auto stage_b = [&](int kb, int buf) {
        const uint32_t base = lds0 + MOG_B_OFF + (uint32_t)buf * MOG_B_BYTES + (uint32_t)wave * 1024u;
#pragma unroll
        for (int r = 0; r < 2; ++r) mx4_dma(bsrc[r] + (size_t)kb * 1024, base + (uint32_t)r * 4096u);
    };
    auto stage_s = [&](int chunk, int buf) {
        const uint32_t base = lds0 + MOG_S_OFF + (uint32_t)buf * MOG_S_BYTES + (uint32_t)wave * 1024u;
        const int kb = min(16 * chunk + (lane >> 2), nkb - 1);
#pragma unroll
        for (int r = 0; r < 2; ++r) mx4_dma(ssrc[r] + (size_t)kb * 64, base + (uint32_t)r * 4096u);
    };
    f32x4_t y[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) y[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    // this wave's fragments: A rows 16 i + m16; B row tiles (SILU_MUL: fragment 0 = a gate tile, 1 = the same columns of up)
    int arow[4], btile[2];
    uint32_t bad[2] = {0u, 0u};
#pragma unroll
    for (int i = 0; i < 4; ++i) arow[i] = i * 16 + m16;
    btile[0] = silu ? wave : 2 * wave;
    btile[1] = silu ? 4 + wave : 2 * wave + 1;

    stage_a(0, 0);
    stage_b(0, 0);
    stage_s(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int kb = 0; kb < nkb; ++kb) {
        const uint8_t* B = mog_lds + MOG_B_OFF + (size_t)(kb & 1) * MOG_B_BYTES;
        const uint8_t* S = mog_lds + MOG_S_OFF + (size_t)((kb >> 4) & 1) * MOG_S_BYTES + (size_t)(kb & 15) * 64 + m16 * 4;
        uint32_t s4[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {                                    // K step 2 kb + h: A buffer h
            if (h == 0) {
                stage_a(2 * kb + 1, 1);
                if (kb + 1 < nkb) stage_b(kb + 1, (kb + 1) & 1);
                if ((kb & 15) == 0 && kb + 16 < nkb) stage_s((kb >> 4) + 1, ((kb >> 4) + 1) & 1);
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    s4[j] = *reinterpret_cast<const uint32_t*>(S + (size_t)btile[j] * 1024);
                    bad[j] |= mx4_has_nan(s4[j]);
                }
            } else if (kb + 1 < nkb) {
                stage_a(2 * kb + 2, 0);
            }
            const uint8_t* A = mog_lds + (size_t)h * MOG_A_BYTES;
            uint2 raw[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) raw[j] = *reinterpret_cast<const uint2*>(B + (size_t)((btile[j] * 64 + lane) * 16 + 8 * h));
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                uint4 af[4], bf[2];
                float sf[2];
#pragma unroll
                for (int i = 0; i < 4; ++i) af[i] = *reinterpret_cast<const uint4*>(A + (size_t)arow[i] * 128 + (size_t)(((s2 * 4 + kg) ^ (arow[i] & 7)) * 16));
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    sf[j] = mx4_scale(s4[j], 2 * h + s2);
                    bf[j] = mx4_frag<DT>(s2 ? raw[j].y : raw[j].x, sf[j]);
                }
#pragma unroll
                for (int j = 0; j < 2; ++j) {                            // (n-fragment outermost: f16 keeps four fresh accumulators live, not eight)
#pragma unroll
                    for (int i = 0; i < 4; ++i) mx4_step<DT>(y[i][j], af[i], bf[j], sf[j]);
                    // f16: as in mxfp4_gemm_kernel, keep the next column's MFMAs below this column's fmas
                    if constexpr (DT != MI355_DTYPE_BF16)
                        asm volatile("" : "+v"(y[0][j]), "+v"(y[1][j]), "+v"(y[2][j]), "+v"(y[3][j]), "+v"(bf[(j + 1) & 1].x));
                }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // the next step has landed (this wave's share of it)
            __syncthreads();                                             // ... everyone's; and everyone is done reading this buffer
        }
    }
    // ---- epilogue: the lane holds pairs 4 kg + v of every m-fragment for column m16 of its two n-fragments
    const float nan = __builtin_nanf("");
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int t = i * 16 + 4 * kg + v;
            if (t >= T) continue;
            const int p = lrow[t];
            if (silu) {
                const int col = c0 + wave * 16 + m16;
                if (col < n_cols) mx4moe_store<DT>(a, p, col, bad[0] ? nan : y[i][0][v], bad[1] ? nan : y[i][1][v]);
            } else {
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int col = c0 + btile[j] * 16 + m16;
                    if (col < n_cols) mx4moe_store<DT>(a, p, col, bad[j] ? nan : y[i][j][v], 0.f);
                }
            }
        }
}

// Route, from what the host knows (the counts are on the device): pairs per expert on average.  Below MX4MOE_GEMM_MIN_AVG the streaming
// kernel, from it on the GEMM.  Measured both ways with this build-time switch: from one pair per expert the GEMM is ahead
// on a layer's two calls together.
#ifndef MX4MOE_GEMM_MIN_AVG
#define MX4MOE_GEMM_MIN_AVG 1
#endif

template <int DT>
static int mx4moe_run(Mx4MoeArgs a, const int32_t* ids, const int32_t P, hipStream_t st) {
    const bool gemm = (int64_t)P >= (int64_t)MX4MOE_GEMM_MIN_AVG * a.E, pair = a.epi == MI355_EPI_SILU_MUL;
    const int M = gemm ? (int)MOG_M : MOS_M;
    const int64_t max_runs = mx4moe_max_runs(P, a.E, M);
    if (max_runs > 65535) return (int)hipErrorNotSupported;              // (the runs are the grid's y extent)
    void* plan = nullptr;
    int rc = mi355_scratch_get(&plan, MI355_SCR_MX4MOE_PLAN, (size_t)(4 + 4 * max_runs + P) * 4, st, false);
    if (rc) return rc;
    a.plan = static_cast<const int32_t*>(plan);
    a.max_runs = (int32_t)max_runs;
    hipLaunchKernelGGL(mx4moe_plan_kernel, dim3(1), dim3(1024), 0, st, static_cast<int32_t*>(plan), ids, P, a.E, M, a.max_runs);
    if ((rc = (int)hipGetLastError())) return rc;
    const int n_cols = pair ? a.pair_offset : a.N;
    if (gemm) {
        static Mi355DevOnce attr;
        if (!attr.done()) {
            (void)hipFuncSetAttribute((const void*)mx4moe_gemm_kernel<DT>, hipFuncAttributeMaxDynamicSharedMemorySize, MOG_LDS);
            attr.set();
        }
        const int per = pair ? 64 : 128;
        hipLaunchKernelGGL((mx4moe_gemm_kernel<DT>), dim3((n_cols + per - 1) / per, a.max_runs), dim3(256), MOG_LDS, st, a);
        return (int)hipGetLastError();
    }
    // a run has at most min(P, 16) pairs: as much of K per staging pass as fits beside them (at one token: top_k rows)
    const int nkb = a.K >> 7, niter = (nkb + MOS_NW - 1) / MOS_NW, tmax = P < MOS_M ? P : MOS_M;
    int G = (MOS_X_BYTES / tmax - 16) / (MOS_NW * 256);                  // k-blocks per wave and staging pass
    G = G > niter ? niter : G;
    const size_t xb = (size_t)tmax * (G * MOS_NW * 256 + 16), rb = (size_t)MOS_NW * (pair ? 2 : 1) * 256 * 4;
    const size_t lds = xb > rb ? xb : rb;
    const dim3 grid(n_cols / 16, a.max_runs), block(64 * MOS_NW);
#define MOS_GO(R_) do { \
        static Mi355DevOnce attr_; \
        if (!attr_.done()) { (void)hipFuncSetAttribute((const void*)mx4moe_small_kernel<DT, R_>, hipFuncAttributeMaxDynamicSharedMemorySize, MOS_X_BYTES); attr_.set(); } \
        hipLaunchKernelGGL((mx4moe_small_kernel<DT, R_>), grid, block, lds, st, a, G); \
    } while (0)
    if (pair) MOS_GO(2); else MOS_GO(1);
#undef MOS_GO
    return (int)hipGetLastError();
}

extern "C" {

int mi355_moe_mxfp4_tile_repack(const void* in_blocks, const void* in_scales, void* out_tiles, void* out_scales, int32_t n_expert, int32_t n,
                                int32_t k, int64_t stream) {
    if (n_expert < 1 || n <= 0 || (n & 15) || (int64_t)n_expert * n > INT32_MAX) return (int)hipErrorInvalidValue;
    // experts lie back to back and own whole 16-row tiles: the image of the stacked [E * n, k] matrix IS the E images back to back
    return mi355_mxfp4_tile_repack(in_blocks, in_scales, out_tiles, out_scales, n_expert * n, k, stream);
}

int mi355_moe_gemm_mxfp4(void* out, const void* x, const void* w_tiled, const void* s_tiled, const int32_t* topk_ids, const float* topk_weights,
                         int32_t num_tokens, int32_t top_k, int32_t n_expert, int32_t x_div, int32_t n, int32_t k, int32_t group,
                         int32_t dtype, int32_t epilogue, int64_t stream) {
    if (num_tokens == 0) return 0;
    if (!out || !x || !w_tiled || !s_tiled || !topk_ids || num_tokens < 0 || n <= 0 || k <= 0) return (int)hipErrorInvalidValue;
    if (top_k < 1 || n_expert < 1 || (x_div != 1 && x_div != top_k) || (int64_t)num_tokens * top_k > INT32_MAX) return (int)hipErrorInvalidValue;
    if (((uintptr_t)x & 15) || ((uintptr_t)w_tiled & 15) || ((uintptr_t)s_tiled & 15) || ((uintptr_t)topk_ids & 3) || ((uintptr_t)topk_weights & 3))
        return (int)hipErrorInvalidValue;
    if (epilogue != MI355_EPI_STORE && epilogue != MI355_EPI_SILU_MUL) return (int)hipErrorInvalidValue;
    if (epilogue == MI355_EPI_SILU_MUL && topk_weights) return (int)hipErrorInvalidValue;
    if (group != 32 || (k & 127) || (n & 15) || n_expert > MP_MAX_E) return (int)hipErrorNotSupported;
    if (epilogue == MI355_EPI_SILU_MUL && (n & 31)) return (int)hipErrorNotSupported;        // gate and up are whole 16-row tiles
    if (dtype != MI355_DTYPE_BF16 && dtype != MI355_DTYPE_F16) return (int)hipErrorNotSupported;
    Mx4MoeArgs a{};
    a.w = static_cast<const uint8_t*>(w_tiled); a.s = static_cast<const uint8_t*>(s_tiled); a.x = x; a.out = out; a.wts = topk_weights;
    a.E = n_expert; a.N = n; a.K = k; a.epi = epilogue; a.x_div = x_div;
    if (epilogue == MI355_EPI_SILU_MUL) { a.pair_offset = n / 2; a.ldo = n / 2; } else a.ldo = n;
    const int32_t P = num_tokens * top_k;
    return dtype == MI355_DTYPE_BF16 ? mx4moe_run<MI355_DTYPE_BF16>(a, topk_ids, P, (hipStream_t)stream)
                                     : mx4moe_run<MI355_DTYPE_F16>(a, topk_ids, P, (hipStream_t)stream);
}

}  // extern "C"
