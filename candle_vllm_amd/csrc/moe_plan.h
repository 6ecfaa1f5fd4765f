// The routing plan that the fused-MoE expert mat-muls share (mxfp4_moe.hip, fp8_moe.hip): topk_ids -> per-expert counts (LDS), the list
// of RUNS {expert, first row, rows <= M} and the row list (pair indices grouped by expert).  Ids outside [0, E) form a pseudo-expert E whose
// runs the compute kernels write as zero rows.  The plan lives in MI355_SCR_MX4MOE_PLAN and is rewritten by every call on its stream.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// One workgroup.  Counts by LDS atomics, the two prefix sums (rows, runs) by wave 0 in chunks of 64 experts, the runs by a binary search
// per run, then the placement: pair p goes to row off[e] + (tickets of e so far).
constexpr int MP_MAX_E = 4096;

static __global__ void __launch_bounds__(1024) mx4moe_plan_kernel(int32_t* __restrict__ plan, const int32_t* __restrict__ ids, const int P,
                                                                  const int E, const int M, const int max_runs) {
    __shared__ int cnt[MP_MAX_E + 1], off[MP_MAX_E + 1], roff[MP_MAX_E + 2];
    const int tid = threadIdx.x;
    for (int e = tid; e <= E; e += 1024) cnt[e] = 0;
    __syncthreads();
    for (int p = tid; p < P; p += 1024) {
        const int e = ids[p];
        atomicAdd(&cnt[(unsigned)e < (unsigned)E ? e : E], 1);
    }
    __syncthreads();
    if (tid < 64) {
        int crow = 0, crun = 0;
        for (int b = 0; b <= E; b += 64) {
            const int e = b + tid;
            const int c = e <= E ? cnt[e] : 0, r = (c + M - 1) / M;
            int ic = c, ir = r;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int tc = __shfl_up(ic, d), tr = __shfl_up(ir, d);
                if (tid >= d) { ic += tc; ir += tr; }
            }
            if (e <= E) { off[e] = crow + ic - c; roff[e] = crun + ir - r; }
            crow += __shfl(ic, 63);
            crun += __shfl(ir, 63);
        }
        if (tid == 0) { roff[E + 1] = crun; plan[0] = min(crun, max_runs); }     // (crun <= max_runs: see mx4moe_max_runs)
    }
    __syncthreads();
    const int nruns = min(roff[E + 1], max_runs);
    for (int r = tid; r < nruns; r += 1024) {
        int lo = 0, hi = E + 1;                                                  // roff[lo] <= r < roff[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (roff[mid] <= r) lo = mid; else hi = mid;
        }
        const int i = r - roff[lo];
        *reinterpret_cast<int4*>(plan + 4 + 4 * r) = make_int4(lo, off[lo] + i * M, min(M, cnt[lo] - i * M), 0);
    }
    __syncthreads();
    for (int e = tid; e <= E; e += 1024) cnt[e] = 0;
    __syncthreads();
    int32_t* rows = plan + 4 + 4 * (size_t)max_runs;
    for (int p = tid; p < P; p += 1024) {
        const int e0 = ids[p], e = (unsigned)e0 < (unsigned)E ? e0 : E;
        rows[off[e] + atomicAdd(&cnt[e], 1)] = p;
    }
}
// every non-empty expert (the pseudo-expert of the out-of-range ids included) ends on at most one partial run
static int64_t mx4moe_max_runs(int64_t P, int64_t E, int64_t M) { return (P < E + 1 ? P : E + 1) + P / M; }
