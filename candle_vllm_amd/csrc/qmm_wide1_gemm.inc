// The GEMM kernels of the 9..32-token path (single-plane generation): split-K partial sums, finished by qmm_epilogue_kernel in its own launch.
// (Running that epilogue inside the GEMM launch, per 256-column block or per row tile, was measured in round 4 and lost: DESIGN_HISTORY.md.)
// Included by qmatmul.hip after QmgChainOut.

// The kernels below read none of this: the argument keeps its place so that their kernel-argument layout stays as it was validated.
struct QwFuse {
    unsigned* ticket;
    const float* ssp;
    QmgChainOut ch;
    unsigned* tile_ticket;
    int ks, n_runs;
    int run_lo[3], run_hi[3];
};

// QW1_LEAD: k-blocks of the activation image in flight ahead of the one the consumers work on (ring of QW1_LEAD + 1 LDS stages).
// 2 since round 4: the skeleton of the gate/up launch (tools/probe_wide_stream.hip: weights + 18 KB image DMA + stores + LDS reads, no
// arithmetic) takes 17.8 us with a double buffer and 15.0 with three stages; the ragged batch-32 step gains 0.5 % (6304 -> 6333 tok/s,
// three alternations on one box, profiles/r04_b32_wide_lead2_ab.txt).  The loader's barrier is then the bare instruction: the release
// fence of __syncthreads() makes the compiler drain every DMA (`s_waitcnt vmcnt(0)`) in front of the s_barrier, so no ring deeper than
// two was ever in flight before; what has to have landed is waited for by count.
// Measured and NOT kept: the seven weight tiles of a k-block through the same stages as well (2 header + 14 plane DMAs by the loader, three
// ds_read_b128 per consumer, no VMEM instruction in the consumers' loop): 6365 -> 6339 tok/s; two-deep weight prefetch in registers with
// asm loads and counted waits: the compiler copies / spills the "available" registers while the loads are in flight (tools/check_isa_vmcnt.py).
#ifndef QW1_LEAD
#define QW1_LEAD 2
#endif
#define QW1_NB (QW1_LEAD + 1)
template <int MT, int WT, int NC = QMG_NC, bool GRP = false>
__device__ __forceinline__ void qw1_gemm_body(const QmmArgs& a, const uint8_t* __restrict__ img, float* __restrict__ part, const int ldp,
                                              const int s0, const int s1, const int n_slots, const int slot_base, const int bx,
                                              const int nb = MT * 16) {
    // (nb, grouped launches: the group's live token rows -- the partial sums of the rows past them are never read)
    extern __shared__ __attribute__((aligned(1024))) uint8_t smem[];
    constexpr int BP = MT * 16;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nkb = a.K >> 8;
    const size_t kbb = (((size_t)MT * (16 * 32 * 16 + 512 + 64)) + 1023) / 1024 * 1024;
    const int kb_per = (nkb + gridDim.y - 1) / gridDim.y;
    const int kb_lo = blockIdx.y * kb_per, kb_hi = min(nkb, kb_lo + kb_per);         // never empty: the launcher normalises the split
    const size_t stb = kbb;                                                          // one stage = the image of one k-block
    if (wave == NC) {
        // loader wave: the images of the next QW1_LEAD k-blocks are in flight while the consumers work on kb
        constexpr int nchunk = (int)(((size_t)MT * (16 * 32 * 16 + 512 + 64) + 1023) / 1024);      // 1 KiB = one wave-wide 16-B DMA
        constexpr int NI = nchunk;                                        // DMA instructions of one stage
        auto dma_kb = [&](int kb, int buf) {
            const uint8_t* src = img + (size_t)kb * kbb;
            uint8_t* dst = smem + (size_t)buf * stb;
#pragma unroll
            for (int c = 0; c < nchunk; ++c)
                __builtin_amdgcn_global_load_lds((qmg_gptr_t)(src + (size_t)c * 1024 + lane * 16), (qmg_lptr_t)(dst + (size_t)c * 1024), 16, 0, 0);
        };
        // the loader's barrier: with QW1_LEAD == 2 the bare instruction -- the release fence of __syncthreads() makes the compiler drain
        // every DMA (`s_waitcnt vmcnt(0)`) in front of the s_barrier; what has to have landed is waited for by count just before
        auto loader_barrier = [&]() {
            if constexpr (QW1_LEAD >= 2) __builtin_amdgcn_s_barrier();
            else __syncthreads();
        };
        // "everything but the k-block requested last has landed": DMAs complete in order, one request = NI instructions
        // "everything but the `ahead` stages requested last has landed": DMAs complete in order, one stage = NI instructions
        auto wait_landed = [&](int ahead) {
            if (QW1_LEAD >= 3 && ahead >= 2) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NI) : "memory");
            else if (QW1_LEAD >= 2 && ahead >= 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NI) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        };
        static_assert(QW1_LEAD >= 1 && QW1_LEAD <= 3 && 2 * NI < 64, "vmcnt is six bits");
        const int len = kb_hi - kb_lo;
#pragma unroll
        for (int i = 0; i < QW1_LEAD; ++i)
            if (i < len) dma_kb(kb_lo + i, i);
        wait_landed(min(QW1_LEAD, len) - 1);                             // the first stage
        loader_barrier();
        int bufn = QW1_LEAD % QW1_NB;                                     // ring stage of k-block kb + QW1_LEAD
        for (int kb = kb_lo; kb < kb_hi; ++kb) {
            if (kb + QW1_LEAD < kb_hi) dma_kb(kb + QW1_LEAD, bufn);
            bufn = bufn + 1 == QW1_NB ? 0 : bufn + 1;
            wait_landed(min(kb + QW1_LEAD, kb_hi - 1) - (kb + 1));        // k-block kb + 1 is complete behind this barrier; the later ones may be in flight
            loader_barrier();
        }
    } else {
        int slot = bx * NC + wave;
        const bool have = slot < n_slots;
        if (!have) slot = 0;
        int t = slot, sg = s0;
        while (sg + 1 < s1 && t >= a.seg[sg].n_tiles) { t -= a.seg[sg].n_tiles; ++sg; }
        const int wtype = WT ? WT : a.seg[sg].type;
        const int wtb = (wtype == MI355_GGML_Q4_K) ? Q4K_TILE : Q6K_TILE;
        const uint8_t* wbase = a.seg[sg].w + (size_t)t * nkb * wtb;
        if constexpr (GRP) wbase += (size_t)blockIdx.z * a.moe_stride[sg];          // grouped launch: this group's expert
        float y[MT][4];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int v = 0; v < 4; ++v) y[mt][v] = 0.f;
        // (one weight tile ahead; TWO ahead measured neutral-to-worse in round 4: gate/up 21.2 -> 22.1 us at 85 instead of 74 VGPRs)
        {
            // (the loop unrolled by two with two register sets in turn -- no `cur = nxt` copies, 16 -> 5 v_mov per k-block -- measured 0.5 % SLOWER
            // on the ragged batch-32 step, round 4: profiles/r04_b32_unpack_ab.txt)
            // (weight tiles TWO ahead in three register sets, the loop unrolled by three so that no tile in flight is copied -- counted waits
            // verified in the ISA, 120 VGPRs -- on top of the three-stage image ring: 6295 -> 5920 tok/s on the ragged batch-32 step, round 4)
            TileRegs cur = load_tile<WT>(wtype, wbase + (size_t)kb_lo * wtb, lane);
            __syncthreads();                                              // first image landed
            int buf = 0;                                                  // ring stages count from the split's first k-block
            for (int kb = kb_lo; kb < kb_hi; ++kb) {
                const uint8_t* Lc = smem + (size_t)buf * stb;
                buf = buf + 1 == QW1_NB ? 0 : buf + 1;
                const bool more = kb + 1 < kb_hi;
                TileRegs nxt = load_tile<WT>(wtype, more ? wbase + (size_t)(kb + 1) * wtb : wbase, more ? lane : 0);
                if (wtype == MI355_GGML_Q4_K) wide1_q4k<MT>(cur, Lc, lane, y);
                else wide1_q6k<MT>(cur, Lc, lane, y);
                cur = nxt;
                __syncthreads();
            }
        }
        // the lane holds tokens 4kg + v of every m-tile for weight row rr: the partial sums of this k-split
        const int kg = lane >> 4, rr = lane & 15;
        if (have) {
            float* pp = part + (size_t)blockIdx.y * BP * ldp + (size_t)(slot_base + slot) * 16 + rr;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int v = 0; v < 4; ++v)
                    if (!GRP || 16 * mt + 4 * kg + v < nb) pp[(size_t)(16 * mt + 4 * kg + v) * ldp] = y[mt][v];
        }
    }
}
template <int MT, int WT>
__global__ void __launch_bounds__(512, 4) qw1_gemm_kernel(const QmmArgs a, const uint8_t* __restrict__ img, float* __restrict__ part,
                                                          const int ldp, const int n_slots, const int slot_base, const QwFuse fz) {
    qmm_kernarg_burst_all(a);
    QMM_BURST_CHAIN(fz.ch);
    QMM_BURST_VALS(img, part, ldp, fz.ticket, fz.ssp, fz.ks);
    QMM_BURST_VALS(n_slots, slot_base);
    if (a.rows_dev && *a.rows_dev <= a.rows_min) return;
    qw1_gemm_body<MT, WT>(a, img, part, ldp, 0, a.nseg, n_slots, slot_base, (int)blockIdx.x);
}
// q, k (Q4_K) + v (Q6_K) in one launch: a uniform branch between two specialised bodies (generation three's rule)
template <int MT, int WTA, int WTB>
__global__ void __launch_bounds__(512, 2) qw1_gemm2_kernel(const QmmArgs a, const uint8_t* __restrict__ img, float* __restrict__ part,
                                                           const int ldp, const int s_split, const int slots0, const int slots1, const QwFuse fz) {
    qmm_kernarg_burst_all(a);
    QMM_BURST_CHAIN(fz.ch);
    QMM_BURST_VALS(img, part, ldp, fz.ticket, fz.ssp, fz.ks);
    QMM_BURST_VALS(s_split, slots0, slots1);
    if (a.rows_dev && *a.rows_dev <= a.rows_min) return;
    const int nwg0 = (slots0 + QMG_NC - 1) / QMG_NC;
    if ((int)blockIdx.x < nwg0) qw1_gemm_body<MT, WTA>(a, img, part, ldp, 0, s_split, slots0, 0, (int)blockIdx.x);
    else qw1_gemm_body<MT, WTB>(a, img, part, ldp, s_split, a.nseg, slots1, slots0, (int)blockIdx.x - nwg0);
}
// grouped launches (QwGroup, qmm_wide1.inc): blockIdx.z = the group; image and partial sums of the group, its own row gate
template <int MT, int WT>
__global__ void __launch_bounds__(512, 4) qw1_gemm_grp_kernel(const QmmArgs a, const uint8_t* __restrict__ img, float* __restrict__ part,
                                                              const int ldp, const int n_slots, const int slot_base, const QwFuse fz,
                                                              const QwGroup g) {
    qmm_kernarg_burst_all(a);
    QMM_BURST_CHAIN(fz.ch);
    QMM_BURST_VALS(img, part, ldp, fz.ticket, fz.ssp, fz.ks);
    QMM_BURST_VALS(n_slots, slot_base, g.img, g.part);
    const int e = blockIdx.z;
    const int nb = a.rows_dev ? min(a.B, a.rows_dev[e] - a.rows_min) : a.B;
    if (nb <= 0) return;
    qw1_gemm_body<MT, WT, QMG_NC, true>(a, img + (size_t)e * g.img, part + (size_t)e * g.part, ldp, 0, a.nseg, n_slots, slot_base,
                                               (int)blockIdx.x, nb);
}
template <int MT, int WTA, int WTB>
__global__ void __launch_bounds__(512, 2) qw1_gemm2_grp_kernel(const QmmArgs a, const uint8_t* __restrict__ img, float* __restrict__ part,
                                                               const int ldp, const int s_split, const int slots0, const int slots1,
                                                               const QwFuse fz, const QwGroup g) {
    qmm_kernarg_burst_all(a);
    QMM_BURST_CHAIN(fz.ch);
    QMM_BURST_VALS(img, part, ldp, fz.ticket, fz.ssp, fz.ks);
    QMM_BURST_VALS(s_split, slots0, slots1, g.img, g.part);
    const int e = blockIdx.z;
    const int nb = a.rows_dev ? min(a.B, a.rows_dev[e] - a.rows_min) : a.B;
    if (nb <= 0) return;
    const int nwg0 = (slots0 + QMG_NC - 1) / QMG_NC;
    img += (size_t)e * g.img; part += (size_t)e * g.part;
    if ((int)blockIdx.x < nwg0) qw1_gemm_body<MT, WTA, QMG_NC, true>(a, img, part, ldp, 0, s_split, slots0, 0, (int)blockIdx.x, nb);
    else qw1_gemm_body<MT, WTB, QMG_NC, true>(a, img, part, ldp, s_split, a.nseg, slots1, slots0, (int)blockIdx.x - nwg0, nb);
}
