// FP8 (e4m3fn, 128 x 128 block scales) fused-MoE expert mat-muls: `moe_gemm_fp8` as `FusedMoeFp8::forward_with_routing` calls it twice per
// layer (src/openai/models/layers/moe.rs:1429-1481) -- a grouped W8A16 GEMM over the experts' tile images (fp8_linear.hip's image, experts
// back to back), routed on the device.  With P = num_tokens * top_k pairs and e_p = topk_ids[p]:
//     out[p, r] = round_dt( w_p * sum_kb s[e_p][srow(r)][kb] * sum_{c in kb} x[p / x_div, c] * e4m3(W[e_p][r, c]) )
// (w_p = topk_weights[p] or 1; x_div = top_k: one x row per token, the gate|up call; x_div = 1: one per pair, the down call).
// Scale rows: the reference packs gate|up scales as cat(gate_scale, up_scale) (moe.rs:1230-1231, 1385-1386), so each half has
// ceil(n_half / 128) scale rows of its own: srow(r) = (r / n_half) * ceil(n_half / 128) + (r % n_half) / 128; n_half == 0 (down): r / 128.
// EPI_SILU_MUL takes each expert's image as that of its packed [gate; up] and writes silu(gate) * up with the dense op's rounding points.
//
// Three launches on the caller's stream, no host round trip:
//   mx4moe_plan_kernel   (moe_plan.h, shared with mxfp4_moe.hip) topk_ids -> runs {expert, first row, rows <= M} and the row list
//   fp8moe_small_kernel  M = 16: the streaming mould of fp8_small_kernel, one run's gathered pairs as one M tile
//   fp8moe_gemm_kernel   M = 64: the LDS-fed mould of fp8_gemm_kernel, a run of up to 64 pairs x 128 weight rows per workgroup
// Numerics are the dense FP8 op's: the weight bytes decode exactly, each 128-k run goes into an accumulator of its own and is folded into
// the running sum with one f32 fma per register and the (row tile, k-block) scale.  MFMA rows are independent, so a pair's result does not
// depend on where the plan's LDS atomics placed it inside its run: results are bit-identical between launches.
#include "fp8_decode.h"
#include "moe_plan.h"
#include "scratch.h"
#include "../../include/mi355_vllm.h"
#include <hip/hip_runtime.h>

struct Fp8MoeArgs {
    const uint8_t* w;         // tiled image, experts back to back (N * K bytes each)
    const float* scale;       // [E][SR][K / 128]
    const void* x;            // 16-bit [P / x_div][K]
    void* out;                // 16-bit [P][ldo]
    const float* wts;         // [P] or null
    const int32_t* plan;      // [0] = runs; run r = int4 {expert, first row, rows, -} at 4 + 4 r; the row list behind max_runs runs
    int32_t E, N, K, ldo, epi, x_div, max_runs;
    int32_t pair_offset;      // SILU_MUL: rows of `up` start here (packed [gate; up], moe.rs:1230, 1385)
    int32_t n_half, sr_half, SR;  // scale rows: n_half == 0: SR = ceil(N / 128); else sr_half = ceil(n_half / 128) per half, SR = 2 sr_half
};

// scale row of weight row `row` (a 16-row tile never straddles one: n_half % 16 == 0)
__device__ __forceinline__ int fp8moe_srow(const Fp8MoeArgs& a, const int row) {
    if (a.n_half == 0) return row >> 7;
    return row >= a.n_half ? a.sr_half + ((row - a.n_half) >> 7) : row >> 7;
}

// the rounding chain of one output element: w_p * sum -> dtype, or gate -> dtype, up -> dtype, silu(gate) -> dtype, * up -> dtype
// (fp8_linear.hip's SILU_MUL without a bias)
template <int DT>
__device__ __forceinline__ void fp8moe_store(const Fp8MoeArgs& a, const int p, const int col, const float y, const float up) {
    uint16_t* o = static_cast<uint16_t*>(a.out) + (size_t)p * a.ldo + col;
    if (a.epi == MI355_EPI_SILU_MUL) {
        const float g = fp8l_rnd<DT>(y), u = fp8l_rnd<DT>(up);
        *o = fp8l_f2h<DT>(fp8l_rnd<DT>(g / (1.f + __expf(-g))) * u);
    } else {
        *o = fp8l_f2h<DT>(a.wts ? a.wts[p] * y : y);
    }
}

// ------------------------------------------------------------------------------------------------ few pairs per expert
// fp8_small_kernel's mould: 8 waves own one row tile (R = 2: a gate tile and its up tile) of the RUN's expert over all of K, wave w the
// k-blocks w, w + 8, ... through a register ring of FMS_RING k-blocks (two dwordx4 per lane, tile and k-block; the (tile, k-block) scale
// rides along as a wave-uniform value); the weights never touch LDS, the sums meet there.  Grid (row tiles, runs); a run's pairs (<= 16)
// are the one M tile: their x rows are staged in LDS through the row list (pair / x_div), G k-blocks per wave at a time; each 128-k run
// goes into a fresh accumulator, then y += s * acc; the epilogue scatters to row p with w_p.  An expert with <= 16 pairs is read once per
// launch; at one token there are top_k runs of one pair.
constexpr int FMS_NW = 8, FMS_RING = 4, FMS_M = 16;
constexpr int FMS_X_BYTES = 16 * (2 * FMS_NW * 256 + 16);  // 65792: 16 pairs x two k-blocks per wave; two workgroups per CU

template <int DT, int R>
__global__ void __launch_bounds__(64 * FMS_NW) fp8moe_small_kernel(const Fp8MoeArgs a, const int G) {
    extern __shared__ __attribute__((aligned(16))) uint8_t fms_lds[];
    __shared__ int xrow[FMS_M], prow[FMS_M];
    if ((int)blockIdx.y >= a.plan[0]) return;
    const int4 rd = *reinterpret_cast<const int4*>(a.plan + 4 + 4 * (size_t)blockIdx.y);
    const int e = __builtin_amdgcn_readfirstlane(rd.x), first = __builtin_amdgcn_readfirstlane(rd.y);
    const int T = __builtin_amdgcn_readfirstlane(rd.z);
    const int32_t* rows = a.plan + 4 + 4 * (size_t)a.max_runs + first;
    int row0[R];
    row0[0] = (int)blockIdx.x * 16;
    if (R == 2) row0[R - 1] = a.pair_offset + (int)blockIdx.x * 16;
    if (e >= a.E) {                                          // ids outside [0, E): zero rows, no weight read
        for (int idx = threadIdx.x; idx < T * 16; idx += 64 * FMS_NW)
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
    const int niter = (nkb + FMS_NW - 1) / FMS_NW;          // the same for every wave (the barriers below)
    const int ldx = G * FMS_NW * 256 + 16;                  // bytes per staged row
    const uint8_t* wp[R];
    const float* sp[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        wp[r] = a.w + (((size_t)e * (a.N >> 4) + (row0[r] >> 4)) * nkb) * 2048 + lane * 16;
        sp[r] = a.scale + ((size_t)e * a.SR + fp8moe_srow(a, row0[r])) * nkb;
    }
    uint4 ring[FMS_RING][R][2];
    float rs[FMS_RING][R];
    // (past the end of K the last k-block is fetched again and not used)
#define FMS_LOAD(SLOT_, I_) do { \
        const int kb_ = min(wave + (I_) * FMS_NW, nkb - 1); \
        _Pragma("unroll") for (int r_ = 0; r_ < R; ++r_) { \
            const fp8l_u32x4* p_ = reinterpret_cast<const fp8l_u32x4*>(wp[r_] + (size_t)kb_ * 2048); \
            const fp8l_u32x4 v0_ = __builtin_nontemporal_load(p_), v1_ = __builtin_nontemporal_load(p_ + 64); \
            ring[SLOT_][r_][0] = make_uint4(v0_.x, v0_.y, v0_.z, v0_.w); \
            ring[SLOT_][r_][1] = make_uint4(v1_.x, v1_.y, v1_.z, v1_.w); \
            rs[SLOT_][r_] = sp[r_][kb_]; \
        } \
    } while (0)
#pragma unroll
    for (int s = 0; s < FMS_RING; ++s) FMS_LOAD(s, s);

    const f32x4_t zero4 = {0.f, 0.f, 0.f, 0.f};
    f32x4_t y[R];
#pragma unroll
    for (int r = 0; r < R; ++r) y[r] = zero4;
    const uint8_t* xg = static_cast<const uint8_t*>(a.x);
    const int pass_cols = G * FMS_NW * 128;                 // k columns of one staging pass

    for (int i0 = 0; i0 < niter; i0 += FMS_RING) {
#pragma unroll
        for (int s = 0; s < FMS_RING; ++s) {
            const int i = i0 + s;
            if (i < niter) {                                 // (uniform over the workgroup)
                const int g = i % G;
                if (g == 0) {
                    // ---- the gathered activations of the next G k-blocks of every wave: columns [c0, c0 + pass_cols) of the run's x rows
                    const int c0 = (i / G) * pass_cols, cols = min(pass_cols, a.K - c0), ppr = cols >> 3;      // 16-byte pieces per row
                    __syncthreads();                         // everyone is done with the previous pass (first pass: xrow is written)
                    for (int p = threadIdx.x; p < T * ppr; p += 64 * FMS_NW) {
                        const int t = p / ppr, c = p - t * ppr;
                        *reinterpret_cast<uint4*>(fms_lds + (size_t)t * ldx + c * 16) =
                            *reinterpret_cast<const uint4*>(xg + ((size_t)xrow[t] * a.K + c0) * 2 + c * 16);
                    }
                    __syncthreads();
                }
                const int kb = wave + i * FMS_NW;
                if (kb < nkb) {
                    const uint8_t* xl = fms_lds + (size_t)(g * FMS_NW + wave) * 256 + 16 * kg;                  // this k-block inside the pass
                    f32x4_t acc[R];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const uint4 af = *reinterpret_cast<const uint4*>(xl + (size_t)min(r16, T - 1) * ldx + 64 * j);
#pragma unroll
                        for (int r = 0; r < R; ++r) {
                            const uint4 v = ring[s][r][j >> 1];
                            const uint4 bf = (j & 1) ? fp8l_frag<DT>(v.z, v.w) : fp8l_frag<DT>(v.x, v.y);
                            acc[r] = fp8l_mfma<DT>(af, bf, j == 0 ? zero4 : acc[r]);
                        }
                    }
#pragma unroll
                    for (int r = 0; r < R; ++r)
#pragma unroll
                        for (int v = 0; v < 4; ++v) y[r][v] = fmaf(rs[s][r], acc[r][v], y[r][v]);
                }
                FMS_LOAD(s, i + FMS_RING);
            }
        }
    }
#undef FMS_LOAD
    // ---- cross-wave reduction: C layout = lane (column = weight row r16, rows m = 4 kg + v)
    float* red = reinterpret_cast<float*>(fms_lds);         // [NW][R][16 m][16 rows]
    __syncthreads();
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int v = 0; v < 4; ++v) red[((wave * R + r) * 16 + 4 * kg + v) * 16 + r16] = y[r][v];
    __syncthreads();
    if (threadIdx.x < 256) {
        const int rr = threadIdx.x & 15, m = threadIdx.x >> 4;
        if (m >= T) return;
        float val[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            float s = 0.f;
#pragma unroll
            for (int w = 0; w < FMS_NW; ++w) s += red[((w * R + r) * 16 + m) * 16 + rr];
            val[r] = s;
        }
        fp8moe_store<DT>(a, prow[m], row0[0] + rr, val[0], val[R - 1]);
    }
}

// ------------------------------------------------------------------------------------------------ many pairs per expert
// fp8_gemm_kernel's mould (global_load_lds_dwordx4 one 64-k step ahead, two buffers, the weight side as the image's KiB runs copied
// verbatim as bytes, the activation side swizzled, the scales as a panel in LDS), re-cut for experts: an expert owns about P / E rows, so
// the workgroup tile is one run of up to 64 pairs x 128 weight rows (SILU_MUL: 64 gate rows and the 64 matching up rows).  4 waves side
// by side along N: a wave owns all 64 pairs x 2 row tiles (4 x 2 fragments), so every byte fragment is decoded by exactly one wave
// (2 x 2 waves would decode each twice) and with SILU_MUL a wave holds a gate tile and its own up tile.  The 128-k run accumulator and
// the running sum are both live: 64 accumulator registers.  LDS: 2 x (A 8 KiB + B 8 KiB) + the run's 64 row-list entries + the scale
// panel [8 row tiles][K / 128] f32 (<= 16 KiB: K <= 65536; a longer K takes the streaming kernel) = 48.25 KiB at most.
//   * A: the lane's global source address of row r comes from the row list in LDS (pair / x_div), so the gather is the DMA itself; rows
//     beyond the run re-read its last row and are masked at the store;
//   * scales: one panel entry per (row tile, k-block) -- a 128-row workgroup tile may straddle a scale row, a 16-row tile never does --
//     staged once per workgroup: no global load inside the K loop;
//   * the epilogue scatters row t of the tile to out row p = row list[t] with w_p.
constexpr uint32_t FMG_M = 64;
constexpr uint32_t FMG_A_BYTES = FMG_M * 128, FMG_B_BYTES = 8 * 1024, FMG_STAGE = FMG_A_BYTES + FMG_B_BYTES;
constexpr uint32_t FMG_ROW_OFF = 2 * FMG_STAGE, FMG_PANEL_OFF = FMG_ROW_OFF + FMG_M * 4;
constexpr int FMG_MAX_NKB = 512;                             // scale panel: 8 x 512 x 4 B = 16 KiB at most (K <= 65536)

template <int DT>
__global__ void __launch_bounds__(256, 2) fp8moe_gemm_kernel(const Fp8MoeArgs a) {
    extern __shared__ __attribute__((aligned(1024))) uint8_t fmg_lds[];  // [2 buffers][A 8 KiB | B 8 KiB][row list][scale panel]
    if ((int)blockIdx.y >= a.plan[0]) return;
    const int4 rd = *reinterpret_cast<const int4*>(a.plan + 4 + 4 * (size_t)blockIdx.y);
    const int e = __builtin_amdgcn_readfirstlane(rd.x), first = __builtin_amdgcn_readfirstlane(rd.y);
    const int T = __builtin_amdgcn_readfirstlane(rd.z);
    const int32_t* rows = a.plan + 4 + 4 * (size_t)a.max_runs + first;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m16 = lane & 15, kg = lane >> 4;
    const bool silu = a.epi == MI355_EPI_SILU_MUL;
    const int nkb = a.K >> 7, nkt = a.K >> 6;
    const int n_cols = silu ? a.pair_offset : a.N, per = silu ? 64 : 128;
    const int c0 = (int)blockIdx.x * per;                                // row tiles fastest: neighbours share their run's x rows through L2
    if (e >= a.E) {                                                      // ids outside [0, E): zero rows, no weight read
        for (int idx = tid; idx < T * per; idx += 256) {
            const int col = c0 + idx % per;
            if (col < n_cols) static_cast<uint16_t*>(a.out)[(size_t)rows[idx / per] * a.ldo + col] = 0;
        }
        return;
    }
    int* lrow = reinterpret_cast<int*>(fmg_lds + FMG_ROW_OFF);
    if (tid < (int)FMG_M) lrow[tid] = rows[min(tid, T - 1)];
    // first weight row of LDS row tile p (clamped: columns beyond the matrix are computed and never stored)
    auto tile_row = [&](int p) {
        if (!silu) return min(c0 + 16 * p, a.N - 16);
        return p < 4 ? min(c0 + 16 * p, a.pair_offset - 16) : min(a.pair_offset + c0 + 16 * (p - 4), a.N - 16);
    };
    float* const panel = reinterpret_cast<float*>(fmg_lds + FMG_PANEL_OFF);
    const float* se = a.scale + (size_t)e * a.SR * nkb;
    for (int i = tid; i < 8 * nkb; i += 256) {
        const int p = i / nkb, kb = i - p * nkb;
        panel[i] = se[(size_t)fp8moe_srow(a, tile_row(p)) * nkb + kb];
    }
    __syncthreads();
    const uint32_t lds0 = __builtin_amdgcn_readfirstlane((uint32_t)(size_t)(__attribute__((address_space(3))) void*)fmg_lds);
    // staging sources: A round r = rows 32 r + tid / 8 (8 threads = the 8 slots of a row, one wave = 8 rows = 1 KiB); B piece 4 r + wave
    const int srow = tid >> 3, sslot = tid & 7;
    const uint8_t* asrc[2];
    const uint8_t* bsrc[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int row = 32 * r + srow;
        asrc[r] = static_cast<const uint8_t*>(a.x) + ((size_t)(lrow[row] / a.x_div) * a.K) * 2 + (size_t)((sslot ^ (row & 7)) * 16);
        bsrc[r] = a.w + (((size_t)e * (a.N >> 4) + (tile_row(4 * r + wave) >> 4)) * nkb) * 2048 + lane * 16;
    }
    auto stage = [&](int kt, int buf) {
        const uint32_t base = lds0 + (uint32_t)buf * FMG_STAGE + (uint32_t)wave * 1024u;
#pragma unroll
        for (int r = 0; r < 2; ++r) fp8l_dma(asrc[r] + (size_t)kt * 128, base + (uint32_t)r * 4096u);
#pragma unroll
        for (int r = 0; r < 2; ++r) fp8l_dma(bsrc[r] + (size_t)kt * 1024, base + FMG_A_BYTES + (uint32_t)r * 4096u);
    };
    const f32x4_t zero4 = {0.f, 0.f, 0.f, 0.f};
    f32x4_t y[4][2], acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) y[i][j] = zero4;
    // this wave's fragments: A rows 16 i + m16; B row tiles (SILU_MUL: fragment 0 = a gate tile, 1 = the same columns of up)
    int arow[4], btile[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) arow[i] = i * 16 + m16;
    btile[0] = silu ? wave : 2 * wave;
    btile[1] = silu ? 4 + wave : 2 * wave + 1;

    stage(0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int kb = 0; kb < nkb; ++kb) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int kt = 2 * kb + h;                                   // (kt & 1 == h: the buffer index is static)
            if (kt + 1 < nkt) stage(kt + 1, h ^ 1);
            const uint8_t* A = fmg_lds + (size_t)h * FMG_STAGE;
            const uint8_t* B = A + FMG_A_BYTES;
            uint4 raw[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) raw[j] = *reinterpret_cast<const uint4*>(B + (size_t)((btile[j] * 64 + lane) * 16));
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                uint4 af[4], bf[2];
#pragma unroll
                for (int i = 0; i < 4; ++i) af[i] = *reinterpret_cast<const uint4*>(A + (size_t)arow[i] * 128 + (size_t)(((s2 * 4 + kg) ^ (arow[i] & 7)) * 16));
#pragma unroll
                for (int j = 0; j < 2; ++j) bf[j] = s2 ? fp8l_frag<DT>(raw[j].z, raw[j].w) : fp8l_frag<DT>(raw[j].x, raw[j].y);
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = fp8l_mfma<DT>(af[i], bf[j], (h == 0 && s2 == 0) ? zero4 : acc[i][j]);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // the next step has landed (this wave's share of it)
            __syncthreads();                                             // ... everyone's; and everyone is done reading this buffer
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float s = panel[btile[j] * nkb + kb];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int v = 0; v < 4; ++v) y[i][j][v] = fmaf(s, acc[i][j][v], y[i][j][v]);
        }
    }
    // ---- epilogue: the lane holds pairs 4 kg + v of every m-fragment for column m16 of its two n-fragments
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int t = i * 16 + 4 * kg + v;
            if (t >= T) continue;
            const int p = lrow[t];
            if (silu) {
                const int col = c0 + wave * 16 + m16;
                if (col < n_cols) fp8moe_store<DT>(a, p, col, y[i][0][v], y[i][1][v]);
            } else {
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int col = c0 + btile[j] * 16 + m16;
                    if (col < n_cols) fp8moe_store<DT>(a, p, col, y[i][j][v], 0.f);
                }
            }
        }
}

// Route, from what the host knows (the counts are on the device): pairs per expert on average.  Below FP8MOE_GEMM_MIN_AVG the streaming
// kernel, from it on the GEMM (measured both ways with this build-time switch: DESIGN.md 5g).  A K beyond the GEMM's scale panel
// (> 65536) takes the streaming kernel at any count: the op itself has no K limit.
#ifndef FP8MOE_GEMM_MIN_AVG
#define FP8MOE_GEMM_MIN_AVG 1
#endif

template <int DT>
static int fp8moe_run(Fp8MoeArgs a, const int32_t* ids, const int32_t P, hipStream_t st) {
    const int nkb = a.K >> 7;
    const bool gemm = (int64_t)P >= (int64_t)FP8MOE_GEMM_MIN_AVG * a.E && nkb <= FMG_MAX_NKB, pair = a.epi == MI355_EPI_SILU_MUL;
    const int M = gemm ? (int)FMG_M : FMS_M;
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
            (void)hipFuncSetAttribute((const void*)fp8moe_gemm_kernel<DT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      FMG_PANEL_OFF + 8 * FMG_MAX_NKB * 4);
            attr.set();
        }
        const int per = pair ? 64 : 128;
        hipLaunchKernelGGL((fp8moe_gemm_kernel<DT>), dim3((n_cols + per - 1) / per, a.max_runs), dim3(256),
                           FMG_PANEL_OFF + (size_t)8 * nkb * 4, st, a);
        return (int)hipGetLastError();
    }
    // a run has at most min(P, 16) pairs: as much of K per staging pass as fits beside them (at one token: top_k rows)
    const int niter = (nkb + FMS_NW - 1) / FMS_NW, tmax = P < FMS_M ? P : FMS_M;
    int G = (FMS_X_BYTES / tmax - 16) / (FMS_NW * 256);                  // k-blocks per wave and staging pass
    G = G > niter ? niter : G;
    const size_t xb = (size_t)tmax * (G * FMS_NW * 256 + 16), rb = (size_t)FMS_NW * (pair ? 2 : 1) * 256 * 4;
    const size_t lds = xb > rb ? xb : rb;
    const dim3 grid(n_cols / 16, a.max_runs), block(64 * FMS_NW);
#define FMS_GO(R_) do { \
        static Mi355DevOnce attr_; \
        if (!attr_.done()) { (void)hipFuncSetAttribute((const void*)fp8moe_small_kernel<DT, R_>, hipFuncAttributeMaxDynamicSharedMemorySize, FMS_X_BYTES); attr_.set(); } \
        hipLaunchKernelGGL((fp8moe_small_kernel<DT, R_>), grid, block, lds, st, a, G); \
    } while (0)
    if (pair) FMS_GO(2); else FMS_GO(1);
#undef FMS_GO
    return (int)hipGetLastError();
}

extern "C" {

int mi355_moe_fp8_tile_repack(const void* in, void* out, int32_t n_expert, int32_t n, int32_t k, int64_t stream) {
    if (n_expert < 1 || n <= 0 || (n & 15) || (int64_t)n_expert * n > INT32_MAX) return (int)hipErrorInvalidValue;
    // experts lie back to back and own whole 16-row tiles: the image of the stacked [E * n, k] matrix IS the E images back to back
    return mi355_fp8_tile_repack(in, out, n_expert * n, k, stream);
}

int mi355_moe_gemm_fp8(void* out, const void* x, const void* w_tiled, const float* w_scale, const int32_t* topk_ids,
                       const float* topk_weights, int32_t num_tokens, int32_t top_k, int32_t n_expert, int32_t x_div, int32_t n, int32_t k,
                       int32_t n_half, int32_t block_n, int32_t block_k, int32_t dtype, int32_t epilogue, int64_t stream) {
    if (num_tokens == 0) return 0;
    if (!out || !x || !w_tiled || !w_scale || !topk_ids || num_tokens < 0 || n <= 0 || k <= 0) return (int)hipErrorInvalidValue;
    if (top_k < 1 || n_expert < 1 || (x_div != 1 && x_div != top_k) || (int64_t)num_tokens * top_k > INT32_MAX) return (int)hipErrorInvalidValue;
    if (((uintptr_t)x & 15) || ((uintptr_t)w_tiled & 15) || ((uintptr_t)w_scale & 3) || ((uintptr_t)topk_ids & 3) || ((uintptr_t)topk_weights & 3))
        return (int)hipErrorInvalidValue;
    if (epilogue != MI355_EPI_STORE && epilogue != MI355_EPI_SILU_MUL) return (int)hipErrorInvalidValue;
    if (epilogue == MI355_EPI_SILU_MUL && topk_weights) return (int)hipErrorInvalidValue;
    if (block_n != 128 || block_k != 128 || (k & 127) || (n & 15) || n_expert > MP_MAX_E) return (int)hipErrorNotSupported;
    if ((n_half != 0 && n_half != n / 2) || (n_half & 15)) return (int)hipErrorInvalidValue;   // a 16-row tile stays inside one scale row
    if (epilogue == MI355_EPI_SILU_MUL && ((n & 31) || n_half != n / 2)) return (int)hipErrorNotSupported;   // gate and up are whole 16-row tiles
    if (dtype != MI355_DTYPE_BF16 && dtype != MI355_DTYPE_F16) return (int)hipErrorNotSupported;
    Fp8MoeArgs a{};
    a.w = static_cast<const uint8_t*>(w_tiled); a.scale = w_scale; a.x = x; a.out = out; a.wts = topk_weights;
    a.E = n_expert; a.N = n; a.K = k; a.epi = epilogue; a.x_div = x_div;
    a.n_half = n_half; a.sr_half = (n_half + 127) / 128; a.SR = n_half ? 2 * a.sr_half : (n + 127) / 128;
    if (epilogue == MI355_EPI_SILU_MUL) { a.pair_offset = n / 2; a.ldo = n / 2; } else a.ldo = n;
    const int32_t P = num_tokens * top_k;
    return dtype == MI355_DTYPE_BF16 ? fp8moe_run<MI355_DTYPE_BF16>(a, topk_ids, P, (hipStream_t)stream)
                                     : fp8moe_run<MI355_DTYPE_F16>(a, topk_ids, P, (hipStream_t)stream);
}

}  // extern "C"
