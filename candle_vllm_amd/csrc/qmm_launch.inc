// Host side of the quantised mat-mul path: everything that chooses and launches the kernels of qmatmul.hip and its qmm_*.inc files.
// Included once by qmatmul.hip after the last kernel.  Top to bottom: per-stream state and the tuning switches; one helper per launch
// decision (token window, k-split, scratch, chain request, runs of same-type segments, waves per workgroup, LDS attribute, the
// x_dtype x norm ladder); one launcher per kernel family; the router mi355_qmm_launch, which every entry point goes through.
//
// Scratch of the wide / prompt paths (activation images, split-K partials, the prompt-step workspace) belongs to the
// (device, stream) that launches: two models on two streams never share an image, growing a buffer never frees memory a
// captured graph still replays from (scratch.cpp; ADVICE r1).  The chain hint is per (device, stream) too.
// image staged by the last chained epilogue: valid for exactly the next wide launch if it consumes the same activations
struct QmgChainState { bool valid; const void* x; int B, K, MT, buf; const float* norm_w; hipStream_t st; int sp; int x_dtype = MI355_DTYPE_F32;
                       int grp = 1; int64_t grp_stride = 0;                       // grouped launch: groups and elements between their activations
                       // the images were built WITHOUT their activations ever being written to `x` (mi355_internal_moe_stage_grouped: `x` is
                       // only the key the consumer will present).  A launch that presents this key and cannot take the images must fail, it
                       // must never stage from `x` (stale rows, silently wrong results -- ADVICE r5)
                       bool prestaged = false; };
struct QmgStream { int cur = 0; QmgChainState chain = {false, nullptr, 0, 0, 0, 0, nullptr, nullptr, 0}; };
static std::mutex g_qmg_mu;
static std::map<std::pair<int, hipStream_t>, QmgStream> g_qmg_streams;
static QmgStream& qmg_stream(hipStream_t st) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lock(g_qmg_mu);
    return g_qmg_streams[std::make_pair(dev, st)];              // std::map: the reference stays valid across later inserts
}
// ---- tuning switches (set through mi355_set_tuning in qmatmul.hip) and the token thresholds of the routes
static int g_tune_exact_act = 0;                             // mi355_set_tuning(24, 1): "exact" activations on the 9..32-token and prompt paths: f16 hi + lo planes (22 bits) instead of one f16 plane
static int g_tune_chain = 1;                                  // mi355_set_tuning(9, 0): never chain (A/B experiments)
// k-split of the 9..32-token launches: split K until a launch has QMG_KS_TARGET (row tile, k-split) slots = 4 consumer waves per CU,
// keeping >= QMG_KS_MINKB k-blocks per workgroup.  (Measured at batch 32: targets 512 / 768 / 1024 / 1280 / 1536 / 2048 / 4096 ->
// 4081 / 4634 / 4835-4900 / 4737 / 4742 / 4686 / 4607 tok/s: less splitting = fewer partial sums for the epilogue and longer pipelines.)
#define QMG_KS_TARGET 1024
#define QMG_KS_MINKB 2
#define QMG_GRP_KS_TARGET 4096                                // the same for grouped launches (slots of all groups)
#define QMP_MIN_TOKENS 96                                  // fewest tokens that take the prompt-step GEMM (launches with a Q5_K segment: Q5P_MIN_TOKENS)
static int g_tune_qpg_fepi = 1;                           // mi355_set_tuning(48, 0): A/B, separate epilogue launch.  Default: the prompt-step GEMM applies the epilogue itself (Q4_K launches; store / residual / SiLU * up; round 4: +7 % on the prompt step)
static int g_tune_prefill_gemm = 1;                        // mi355_set_tuning(6, v): 1 = prompt steps take the prompt-step GEMM, 0 = always stream the quantised weights (A/B)
static int g_qmm_exact = 0;                               // parity mode 2 (tests only; kernel in qmm_exact.inc, switch: mi355_internal_qmm_set_exact)
// Fewest tokens of a launch with a Q5_K segment that take the prompt-step GEMM.  Above QMP_MIN_TOKENS (96) because the 32-token chunks split K and the
// prompt GEMM does not: the Llama-3-8B down projection (4096 x 14336: 16 row blocks, 56 k-blocks in a row) takes 184..186 us from 96 to 256
// tokens on the GEMM against 35.5 us per 32-token chunk (107 us at 96, 142 us at 128 tokens) -- it wins from the sixth chunk on, gate|up
// (67 against 132 us at 96 tokens) from the start.  DESIGN.md section 5b has the table.
#define Q5P_MIN_TOKENS 192
// ONE statement of "a grouped mat-mul of B token rows runs as the z extent of the 9..32-token launches" (mi355_qmm_launch takes that path,
// mi355_internal_moe_stage_grouped builds images only for it, mi355_internal_moe_scatter_combine_to_image stages only for it): three hand
// copies of this condition had to agree for the fused MoE staging to be correct (ADVICE r5).
static bool qmg_wide_one_launch(int B) {
    return B > 8 && B <= 8 * QMW_MAXMT && !g_tune_exact_act && !g_qmm_exact && !(B >= QMP_MIN_TOKENS && g_tune_prefill_gemm);
}

// ================================================================================================ one helper per decision
// the descriptor restricted to tokens [b0, b0 + bn): every per-token pointer moves, nothing else changes
static QmmArgs qmm_token_window(const QmmArgs& a, int b0, int bn) {
    QmmArgs w = a;
    const size_t xes = (a.x_dtype == MI355_DTYPE_BF16) ? 2 : 4;
    w.B = bn;
    w.x = static_cast<const uint8_t*>(a.x) + (size_t)b0 * a.ldx * xes;
    w.out = a.out ? a.out + (size_t)b0 * a.ldo : nullptr;
    w.resid = a.resid ? a.resid + (size_t)b0 * a.ldo : nullptr;
    w.q_out = a.q_out ? a.q_out + (size_t)b0 * a.Hq * a.D : nullptr;
    w.positions = a.positions ? a.positions + b0 : nullptr;
    w.slot_mapping = a.slot_mapping ? a.slot_mapping + b0 : nullptr;
    return w;
}

static int qmm_total_tiles(const QmmArgs& a) {
    int n = 0;
    for (int s = 0; s < a.nseg; ++s) n += a.seg[s].n_tiles;
    return n;
}

// no empty split: the kernels walk ceil(nkb / ks) k-blocks per split, and every split's partial sums are added up
static int qmm_no_empty_split(int nkb, int ks) {
    const int kb_per = (nkb + ks - 1) / ks;
    return (nkb + kb_per - 1) / kb_per;
}
// k-split of a 9..32-token launch: double until the launch has `target` (row tile, k-split) slots, keeping >= QMG_KS_MINKB k-blocks per
// split.  qmg_launch's kernels take the power of two as it is (normalise = false); nkb = 9, few slots: 4 there, 3 normalised
static int qmm_split_k(int64_t n_slots, int nkb, int target, bool normalise) {
    int ks = 1;
    while (n_slots * ks < target && nkb / (ks * 2) >= QMG_KS_MINKB) ks *= 2;
    return normalise ? qmm_no_empty_split(nkb, ks) : ks;
}

static inline int qmg_buf(void** p, int key, size_t need, hipStream_t st) { return mi355_scratch_get(p, key, need, st, false); }
// Activation image of a 9..32-token launch in image buffer `buf` (0 / 1): [nkb][kbb] image bytes, then the sum-of-squares partials
// [nkb][rows] (ssp).  G > 1: one image per group, each rounded to the 1-KiB DMA granule, group e's `stride` bytes after group e - 1's.
struct QmgImage { uint8_t* img; float* ssp; size_t stride; };
static int qmg_image(QmgImage& o, int buf, size_t kbb, int nkb, int rows, int G, hipStream_t st) {
    const size_t one = kbb * nkb + (size_t)nkb * rows * sizeof(float);
    o.stride = (one + 1023) / 1024 * 1024;
    void* p = nullptr;
    const int rc = qmg_buf(&p, buf ? MI355_SCR_QMM_IMG1 : MI355_SCR_QMM_IMG0, G > 1 ? G * o.stride : one, st);
    o.img = static_cast<uint8_t*>(p);
    o.ssp = reinterpret_cast<float*>(o.img + kbb * nkb);
    return rc;
}
// ... and with it the split-K partial sums [G][ks][rows][ldp]
static int qmg_scratch(QmgImage& im, float** part, int buf, size_t kbb, int nkb, int rows, int G, int ks, int ldp, hipStream_t st) {
    int rc = qmg_image(im, buf, kbb, nkb, rows, G, st);
    if (rc) return rc;
    void* p = nullptr;
    rc = qmg_buf(&p, MI355_SCR_QMM_PART, (size_t)G * ks * rows * ldp * sizeof(float), st);
    *part = static_cast<float*>(p);
    return rc;
}

// chain request honoured: the epilogue of this launch also stages the image of the next wide mat-mul (x = our out, k = next_k)
static bool qmm_chain_wanted(const QmmArgs& a) {
    return g_tune_chain && a.chain_next && a.next_k > 0 && (a.next_k % 256) == 0 && a.ldo == a.next_k &&
           (a.epi == MI355_EPI_RESID || a.epi == MI355_EPI_SILU_MUL || a.epi == MI355_EPI_STORE) &&
           (a.epi == MI355_EPI_SILU_MUL ? a.seg[0].n_rows == a.next_k : (a.nseg == 1 && a.seg[0].n_rows == a.next_k));
}

// One GEMM launch per run of same-type segments: the type-specialised builds need no schedule pinning and do not spill (the mixed build
// did); each run writes its own columns of the partial-sum buffer.  f(r, run_slots, slot_base): r = the descriptor cut to the run.
// (moe_stride travels with its segment: only the grouped kernels of qw1_launch read it; qmm_gemm_kernel never does, the prompt kernels
// multiply it by the block table's expert, which is 0 without a block table -- and no block-table launch comes here)
template <typename F>
static void qmm_for_each_run(const QmmArgs& a, F&& f) {
    for (int s0 = 0, slot_base = 0; s0 < a.nseg;) {
        int s1 = s0 + 1;
        while (s1 < a.nseg && a.seg[s1].type == a.seg[s0].type) ++s1;
        QmmArgs r = a;
        r.nseg = s1 - s0;
        int run_slots = 0;
        for (int q = 0; q < r.nseg; ++q) { r.seg[q] = a.seg[s0 + q]; r.moe_stride[q] = a.moe_stride[s0 + q]; run_slots += r.seg[q].n_tiles; }
        f(r, run_slots, slot_base);
        slot_base += run_slots;
        s0 = s1;
    }
}
// exactly one Q4_K run followed by one Q6_K run (one launch of the two-type kernels): the index of the first Q6_K segment and the
// tiles of the Q4_K run; 0 otherwise
static int qmm_q4_then_q6(const QmmArgs& a, int* slots0) {
    int s_split = 0;
    *slots0 = 0;
    while (s_split < a.nseg && a.seg[s_split].type == MI355_GGML_Q4_K) *slots0 += a.seg[s_split++].n_tiles;
    if (s_split == 0 || s_split == a.nseg) return 0;
    for (int q = s_split; q < a.nseg; ++q) if (a.seg[q].type != MI355_GGML_Q6_K) return 0;
    return s_split;
}

// once per device: let `kernels` use `bytes` of dynamic LDS
template <typename... Kernels>
static void qmm_allow_lds(Mi355DevOnce& once, int bytes, Kernels... kernels) {
    if (once.done()) return;
    ((void)hipFuncSetAttribute((const void*)kernels, hipFuncAttributeMaxDynamicSharedMemorySize, bytes), ...);
    once.set();
}

// The decode kernels are built per activation type and per "an RMSNorm weight is fused" (XB, NRM of qmm_body): f(XB, NRM) with the two
// as std::integral_constant, so that the caller names its kernel once
template <typename F>
static void qmm_by_x_and_norm(const QmmArgs& a, F&& f) {
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    const bool xb = a.x_dtype == MI355_DTYPE_BF16, nrm = a.norm_w != nullptr;
    if (xb && nrm) f(I1{}, I1{});
    else if (xb) f(I1{}, I0{});
    else if (nrm) f(I0{}, I1{});
    else f(I0{}, I0{});
}

static size_t qmm_lds_bytes(int BT, int R, int NW) {
    const size_t xw = (size_t)32 * 2 * BT * 16;
    return (size_t)NW * xw + (size_t)NW * R * BT * 16 * 4 + (size_t)NW * BT * 4 + 64;
}
// Waves per workgroup of a decode launch: the largest NW in {8,4,2} for which every workgroup of the launch is resident at
// once (no second dispatch round => no tail), judged by the occupancy the runtime reports for `kernel`; blocks_per_cu is the
// caller's cache of that answer (one per kernel instantiation, -1 = not asked yet).
static int qmm_pick_nw(const void* kernel, int (&blocks_per_cu)[3], int BT, int R, int n_wg, int nkb) {
    const int cus = mi355_num_cus();                      // per device (common.h)
    int pick = 1;
    for (int i = 0; i < 3; ++i) {                         // never below 2 waves: one wave per tile serialises K
        const int nw = 8 >> i;
        if (nw > nkb) continue;
        if (blocks_per_cu[i] < 0) {
            int nb = 0;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, 64 * nw, qmm_lds_bytes(BT, R, nw)) != hipSuccess || nb < 1) nb = 1;
            blocks_per_cu[i] = nb;
        }
        pick = nw;
        if ((long)n_wg <= (long)blocks_per_cu[i] * cus) return nw;
    }
    // more workgroups than the chip holds even at 2 waves each: several rounds anyway -> 4 waves
    return nkb >= 4 ? 4 : pick;
}

// ================================================================================================ 9..32 tokens
// hi + lo f16 planes ("exact" activations, mi355_set_tuning(24, 1)): MT = m-tiles of 8 tokens
template <int MT>
static int qmg_launch(const QmmArgs& a0, hipStream_t st) {
    QmmArgs a = a0;
    if (a.paired) a.paired = 0;                 // slots are plain (segment, tile) order; the epilogue pairs gate/up rows
    const int nkb = a.K / 256, n_slots = qmm_total_tiles(a), ldp = n_slots * 16;
    const size_t kbb = qmg_kb_bytes(MT);
    const int ks = qmm_split_k(n_slots, nkb, QMG_KS_TARGET, false);
    // activation image: staged by the previous launch's epilogue (chain) or by the prep kernel now
    QmgStream& qs = qmg_stream(st);
    const bool chained = qs.chain.valid && qs.chain.x == a.x && qs.chain.B == a.B && qs.chain.K == a.K &&
                         qs.chain.MT == MT && qs.chain.sp == 0 && qs.chain.norm_w == a.norm_w && qs.chain.st == st &&
                         a.x_dtype == MI355_DTYPE_F32 && a.ldx == a.K;
    qs.chain.valid = false;
    const int cur = chained ? qs.chain.buf : qs.cur;
    // (a chained image was sized by the epilogue that staged it: the same request returns the same buffer)
    QmgImage im;
    float* part = nullptr;
    int rc = qmg_scratch(im, &part, cur, kbb, nkb, MT * 8, 1, ks, ldp, st);
    if (rc) return rc;
    static Mi355DevOnce attr_done;
    qmm_allow_lds(attr_done, 160 * 1024, qmm_gemm_kernel<MT, MI355_GGML_Q4_K>, qmm_gemm_kernel<MT, MI355_GGML_Q6_K>,
                  qmm_gemm2_kernel<MT, MI355_GGML_Q4_K, MI355_GGML_Q6_K>);
    if (!chained) hipLaunchKernelGGL((qmm_prep2_kernel<MT>), dim3(nkb, MT), dim3(256), 0, st, im.img, im.ssp, a, kbb);
    int slots0 = 0;
    const int s_split = qmm_q4_then_q6(a, &slots0);
    if (s_split) {
        const int slots1 = n_slots - slots0;
        const dim3 ggrid((slots0 + QMG_NC - 1) / QMG_NC + (slots1 + QMG_NC - 1) / QMG_NC, ks);
        hipLaunchKernelGGL((qmm_gemm2_kernel<MT, MI355_GGML_Q4_K, MI355_GGML_Q6_K>), ggrid, dim3(512), 2 * kbb, st, a, im.img, part, ldp, s_split, slots0, slots1);
    } else {
        qmm_for_each_run(a, [&](const QmmArgs& r, int run_slots, int slot_base) {
            const dim3 ggrid((run_slots + QMG_NC - 1) / QMG_NC, ks);
            if (r.seg[0].type == MI355_GGML_Q4_K)
                hipLaunchKernelGGL((qmm_gemm_kernel<MT, MI355_GGML_Q4_K>), ggrid, dim3(512), 2 * kbb, st, r, im.img, part, ldp, run_slots, slot_base);
            else
                hipLaunchKernelGGL((qmm_gemm_kernel<MT, MI355_GGML_Q6_K>), ggrid, dim3(512), 2 * kbb, st, r, im.img, part, ldp, run_slots, slot_base);
        });
    }
    // chain: this epilogue also stages the image of the next wide mat-mul (x = our out) into the other buffer
    QmgChainOut ch{nullptr, nullptr, nullptr, 0, 0, 0, 0};
    const bool want = qmm_chain_wanted(a);
    if (want) {
        QmgImage nx;
        rc = qmg_image(nx, cur ^ 1, kbb, a.next_k / 256, MT * 8, 1, st);
        if (rc) return rc;
        ch = QmgChainOut{nx.img, nx.ssp, a.next_norm_w, a.next_k, MT, kbb, 0};
        qs.chain = QmgChainState{true, a.out, a.B, a.next_k, MT, cur ^ 1, a.next_norm_w, st, 0};
    }
    qs.cur = cur;
    hipLaunchKernelGGL(qmm_epilogue_kernel, dim3((ldp + 255) / 256, want ? MT * 8 : a.B), dim3(256), 0, st, a, part, ldp, ks,
                       MT * 8, im.ssp, ch);
    return (int)hipGetLastError();
}

// single-plane launcher (qmm_wide1.inc, qmm_wide1_gemm.inc): MT = m-tiles of 16 tokens (1: 9..16 tokens, 2: 17..32)
template <int MT>
static int qw1_launch(const QmmArgs& a0, hipStream_t st) {
    QmmArgs a = a0;
    if (a.paired) a.paired = 0;
    const int nkb = a.K / 256, n_slots = qmm_total_tiles(a), ldp = n_slots * 16, BP = MT * 16;
    const size_t kbb = qw1_kb_bytes(MT);
    // grouped launch: G mat-muls of these shapes in the z extent of every launch (the experts of a mixture-of-experts layer)
    const int G = a.grp_n > 1 ? a.grp_n : 1;
    int ks = qmm_split_k((int64_t)n_slots * G, nkb, G > 1 ? QMG_GRP_KS_TARGET : QMG_KS_TARGET, false);
#ifndef QW1_Q6K_LONGK_WGS
#define QW1_Q6K_LONGK_WGS 0
#endif
    if (QW1_Q6K_LONGK_WGS > 0 && G == 1 && a.nseg == 1 && nkb >= 32 && a.seg[0].type == MI355_GGML_Q6_K) {
        // Rounds 4-5 (two MFMA chains per Q6_K weight, 411 VALU per tile and k-block: profiles/r03_pmc_sq_b32_set1.json): the long-K Q6_K
        // launch (the down projection: 256 tiles x 56 k-blocks) was bound by its unpack arithmetic, and 37 x 14 = 518 workgroups -- two per
        // CU, the second one's waves in the first's stalls -- beat the power-of-two split (37 x 4): 27.6 -> 23.8 us.  With ONE operand per
        // weight (round 6, QW1_Q6K_ONE_PLANE) the arithmetic is no longer the bound and the 14 partial sums per output are pure cost:
        // same box, ragged batch-32 step: 14 splits 6515 / 6529 tok/s, 7 splits 6699 / 6667, the general rule's 4 splits 6749 / 6729
        // (profiles/r06_b32_q6k_ab.txt) -- the special case is off (-DQW1_Q6K_LONGK_WGS=512 builds it back for A/B).
        const int n_wg = (n_slots + QMG_NC - 1) / QMG_NC;
        const int cus = QW1_Q6K_LONGK_WGS;
        if (n_wg * ks < cus) {
            int want = (cus + n_wg - 1) / n_wg;
            while (want > 1 && nkb / want < 4) --want;
            if (want > ks) ks = want;
        }
    }
    // (gate/up, 256 workgroups of 16 k-blocks: a split into 2 x 8 for two workgroups per CU measured +-0.1 % on the batch-32 step, round 4)
    ks = qmm_no_empty_split(nkb, ks);
    QmgStream& qs = qmg_stream(st);
    const bool chained = qs.chain.valid && qs.chain.x == a.x && qs.chain.B == a.B && qs.chain.K == a.K &&
                         qs.chain.MT == MT && qs.chain.sp == 1 && qs.chain.norm_w == a.norm_w && qs.chain.st == st &&
                         a.x_dtype == qs.chain.x_dtype && a.ldx == a.K && qs.chain.grp == G &&
                         (G == 1 || qs.chain.grp_stride == a.grp_x);
    const bool orphan = qs.chain.valid && qs.chain.prestaged && qs.chain.x == a.x && !chained;
    qs.chain.valid = false;
    if (orphan) {                                                       // the images behind this key were staged for another launch shape,
        mi355_note_error((int)hipErrorInvalidValue);                     // and `x` itself was never written: refuse instead of staging stale rows
        return (int)hipErrorInvalidValue;
    }
    const int cur = chained ? qs.chain.buf : qs.cur;
    QmgImage im;
    float* part = nullptr;
    int rc = qmg_scratch(im, &part, cur, kbb, nkb, BP, G, ks, ldp, st);
    if (rc) return rc;
    static Mi355DevOnce attr_done;
    qmm_allow_lds(attr_done, 160 * 1024, qw1_gemm_kernel<MT, MI355_GGML_Q4_K>, qw1_gemm_kernel<MT, MI355_GGML_Q6_K>,
                  qw1_gemm2_kernel<MT, MI355_GGML_Q4_K, MI355_GGML_Q6_K>, qw1_gemm_grp_kernel<MT, MI355_GGML_Q4_K>,
                  qw1_gemm_grp_kernel<MT, MI355_GGML_Q6_K>, qw1_gemm2_grp_kernel<MT, MI355_GGML_Q4_K, MI355_GGML_Q6_K>);
    uint8_t* const img = im.img;
    float* const ssp = im.ssp;
    // chain: the epilogue also stages the image of the next wide mat-mul (x = our out) into the other buffer
    QmgChainOut ch{nullptr, nullptr, nullptr, 0, 0, 0, 0};
    size_t imgb2 = 0;
    const bool want = qmm_chain_wanted(a);
    if (want) {
        QmgImage nx;
        rc = qmg_image(nx, cur ^ 1, kbb, a.next_k / 256, BP, G, st);
        if (rc) return rc;
        imgb2 = nx.stride;
        ch = QmgChainOut{nx.img, nx.ssp, a.next_norm_w, a.next_k, MT, kbb, 1};
    }
    const QwGroup grp{a.grp_x, a.grp_out, (int64_t)im.stride, (int64_t)ks * BP * ldp, (int64_t)imgb2};
    const QwFuse fz{};                                                // unread kernel argument (qmm_wide1_gemm.inc)
    if (!chained && G > 1) hipLaunchKernelGGL((qw1_prep_grp_kernel<MT>), dim3(nkb, MT * 2, G), dim3(256), 0, st, img, ssp, a, kbb, grp);
    else if (!chained) hipLaunchKernelGGL((qw1_prep_kernel<MT>), dim3(nkb, MT * 2), dim3(256), 0, st, img, ssp, a, kbb);
    int slots0 = 0;
    const int s_split = qmm_q4_then_q6(a, &slots0);
    if (s_split) {
        const int slots1 = n_slots - slots0;
        const dim3 ggrid((slots0 + QMG_NC - 1) / QMG_NC + (slots1 + QMG_NC - 1) / QMG_NC, ks, G);
        if (G > 1) hipLaunchKernelGGL((qw1_gemm2_grp_kernel<MT, MI355_GGML_Q4_K, MI355_GGML_Q6_K>), ggrid, dim3(512), QW1_NB * kbb, st, a, img, part, ldp, s_split, slots0, slots1, fz, grp);
        else hipLaunchKernelGGL((qw1_gemm2_kernel<MT, MI355_GGML_Q4_K, MI355_GGML_Q6_K>), ggrid, dim3(512), QW1_NB * kbb, st, a, img, part, ldp, s_split, slots0, slots1, fz);
    } else {
        qmm_for_each_run(a, [&](const QmmArgs& r, int run_slots, int slot_base) {
            const dim3 ggrid((run_slots + QMG_NC - 1) / QMG_NC, ks, G);
            if (G > 1) {
                if (r.seg[0].type == MI355_GGML_Q4_K)
                    hipLaunchKernelGGL((qw1_gemm_grp_kernel<MT, MI355_GGML_Q4_K>), ggrid, dim3(512), QW1_NB * kbb, st, r, img, part, ldp, run_slots, slot_base, fz, grp);
                else
                    hipLaunchKernelGGL((qw1_gemm_grp_kernel<MT, MI355_GGML_Q6_K>), ggrid, dim3(512), QW1_NB * kbb, st, r, img, part, ldp, run_slots, slot_base, fz, grp);
            } else if (r.seg[0].type == MI355_GGML_Q4_K)
                hipLaunchKernelGGL((qw1_gemm_kernel<MT, MI355_GGML_Q4_K>), ggrid, dim3(512), QW1_NB * kbb, st, r, img, part, ldp, run_slots, slot_base, fz);
            else
                hipLaunchKernelGGL((qw1_gemm_kernel<MT, MI355_GGML_Q6_K>), ggrid, dim3(512), QW1_NB * kbb, st, r, img, part, ldp, run_slots, slot_base, fz);
        });
    }
    if (want) { qs.chain = QmgChainState{true, a.out, a.B, a.next_k, MT, cur ^ 1, a.next_norm_w, st, 1}; qs.chain.grp = G; qs.chain.grp_stride = a.grp_out; }
    qs.cur = cur;
    if (G > 1)
        hipLaunchKernelGGL(qmm_epilogue_grp_kernel, dim3((ldp + 255) / 256, want ? BP : a.B, G), dim3(256), 0, st, a, part, ldp, ks, BP, ssp, ch, grp);
    else
        hipLaunchKernelGGL(qmm_epilogue_kernel, dim3((ldp + 255) / 256, want ? BP : a.B), dim3(256), 0, st, a, part, ldp, ks, BP, ssp, ch);
    return (int)hipGetLastError();
}

// Q5_K (qmm_q5k.inc: q5g_gemm_kernel), every segment Q5_K: MT = m-tiles of 16 tokens (1: 9..16 tokens, 2: 17..32); the image of
// qw1_prep_kernel, never chained
template <int MT>
static int q5g_launch(const QmmArgs& a0, hipStream_t st) {
    QmmArgs a = a0;
    a.paired = 0;                                   // slots are plain (segment, tile) order; the epilogue pairs gate / up rows
    a.chain_next = 0;
    const int nkb = a.K / 256, BP = MT * 16, n_slots = qmm_total_tiles(a), ldp = n_slots * 16;
    const size_t kbb = qw1_kb_bytes(MT);
    const int ks = qmm_split_k(n_slots, nkb, QMG_KS_TARGET, true);
    QmgImage im;
    float* part = nullptr;
    const int rc = qmg_scratch(im, &part, qmg_stream(st).cur, kbb, nkb, BP, 1, ks, ldp, st);
    if (rc) return rc;
    hipLaunchKernelGGL((qw1_prep_kernel<MT>), dim3(nkb, MT * 2), dim3(256), 0, st, im.img, im.ssp, a, kbb);
    hipLaunchKernelGGL((q5g_gemm_kernel<MT>), dim3((n_slots + Q5G_NC - 1) / Q5G_NC, ks), dim3(64 * Q5G_NC), 2 * kbb, st, a, im.img, part, ldp, n_slots);
    hipLaunchKernelGGL(qmm_epilogue_kernel, dim3((ldp + 255) / 256, a.B), dim3(256), 0, st, a, part, ldp, ks, BP, im.ssp,
                       QmgChainOut{nullptr, nullptr, nullptr, 0, 0, 0, 0}, (const float*)nullptr);
    return (int)hipGetLastError();
}

// ================================================================================================ prompt step
// Prompt-step path (num_tokens >= QMP_MIN_TOKENS): the matmul is compute-bound, so it is run as a GEMM on the matrix cores
// (qmm_prefill.inc) instead of streaming the quantised weights once per 32 tokens.

// hand-written prompt-step GEMM (qmm_prefill.inc); returns hipErrorNotSupported for launches it does not cover (then the
// caller streams the weights 32 tokens at a time)
static int qpg_launch(const QmmArgs& a0, hipStream_t st) {
    QmmArgs a = a0;
    a.paired = 0;
    for (int s = 0; s < a.nseg; ++s)
        if (!is_kquant(a.seg[s].type) || (a.seg[s].type == MI355_GGML_Q5_K && a.blk_tab)) return (int)hipErrorNotSupported;
    if (a.moe_expert || (a.K & 255)) return (int)hipErrorNotSupported;
    const int n_slots = qmm_total_tiles(a);
    const int T = a.B, K = a.K, ldp = n_slots * 16, nkb = K >> 8;
    const int Tpad = (T + QPG_BM - 1) / QPG_BM * QPG_BM;
    const int parts = g_tune_exact_act ? 2 : 1;             // activation planes of the f16 image (mi355_set_tuning(24, 1) = hi + lo)
    // (a block-table launch only exists with the epilogue in the store loop: no C buffer -- it would be 1.9 GB for a Mixtral chunk)
    const size_t xa_b = (size_t)K * Tpad * 2 * parts, sf_b = (size_t)nkb * Tpad * 32, rs_b = (size_t)Tpad * 4, c_b = a.blk_tab ? 0 : (size_t)T * ldp * 4;
    void* ws = nullptr;
    int rc = qmg_buf(&ws, MI355_SCR_QMP_WS, xa_b + sf_b + 2 * rs_b + c_b + 4096, st);
    if (rc) return rc;
    uint8_t* base = static_cast<uint8_t*>(ws);
    QpgImg im;
    im.xa = base; im.sfrag = base + xa_b;
    im.row_scale = reinterpret_cast<float*>(base + xa_b + sf_b);
    im.row_inv = im.row_scale + Tpad;
    im.Tpad = Tpad;
    im.parts = parts;
    float* C = reinterpret_cast<float*>(base + xa_b + sf_b + 2 * rs_b);
    static Mi355DevOnce attr64, attr80, attr160;
    qmm_allow_lds(attr64, 64 * 1024, qpg_gemm_kernel<MI355_GGML_Q4_K, 4, 2, 1, 8, 2>, qpg_gemm_kernel<MI355_GGML_Q5_K, 4, 2, 1, 8, 2>, qpg_gemm_q6k_kernel<2, 2>);
    qmm_allow_lds(attr80, 80 * 1024, qpg_gemm_lds2_kernel<true>, qpg_gemm_lds2_kernel<false>, qpg_gemm_lds2_kernel<true, true>,
                  qpg_gemm_lds2_kernel<true, false, MI355_GGML_Q5_K>, qpg_gemm_lds2_kernel<false, false, MI355_GGML_Q5_K>);
    qmm_allow_lds(attr160, 160 * 1024, qpg_gemm_q6k_lds_kernel<false>, qpg_gemm_q6k_lds_kernel<true>, qpg_gemm_q6k_lds_kernel<true, 1>,
                  qpg_gemm_q6k_lds_kernel<true, 2, true>);
    hipLaunchKernelGGL(qpg_rowprep_kernel, dim3(Tpad), dim3(256), 0, st, a, im);          // row statistics + image, one launch (workgroup = token)
    // mi355_set_tuning(48, 1), the default: all segments Q4_K (or all Q5_K), one activation plane, and an epilogue that is a store /
    // residual add / SiLU * up over two equal segments -> the GEMM writes the outputs itself, no C buffer, no epilogue launch
    {
        bool all_q4 = true, all_q5 = true;
        for (int s = 0; s < a.nseg; ++s) { all_q4 = all_q4 && a.seg[s].type == MI355_GGML_Q4_K; all_q5 = all_q5 && a.seg[s].type == MI355_GGML_Q5_K; }
        const bool epi_ok = a.epi == MI355_EPI_STORE || a.epi == MI355_EPI_RESID ||
                            (a.epi == MI355_EPI_SILU_MUL && a.nseg == 2 && a.seg[0].n_tiles == a.seg[1].n_tiles && a.seg[0].n_rows == a.seg[1].n_rows);
        if (g_tune_qpg_fepi && (all_q4 || all_q5) && epi_ok && parts == 1) {
            QmmArgs r = a;
            r.norm_w = nullptr;                                 // applied while the image was built
            // 64 tokens x 256 rows per workgroup (waves 64 x 32), two workgroups per CU
            const dim3 g_(Tpad / 64, (n_slots + 15) / 16), b_(512);
            if (all_q5) hipLaunchKernelGGL((qpg_gemm_lds2_kernel<true, false, MI355_GGML_Q5_K>), g_, b_, (size_t)QPG5_BYTES, st, r, im, C, ldp, n_slots, 0);
            else if (a.blk_tab) hipLaunchKernelGGL((qpg_gemm_lds2_kernel<true, true>), g_, b_, (size_t)QPG2_BYTES, st, r, im, C, ldp, n_slots, 0);
            else hipLaunchKernelGGL((qpg_gemm_lds2_kernel<true>), g_, b_, (size_t)QPG2_BYTES, st, r, im, C, ldp, n_slots, 0);
            return (int)hipGetLastError();
        }
        if (a.blk_tab) {
            // block-table launches: Q4_K above; one Q6_K matrix with a store / residual epilogue here (the down projections of a Q4_K_M file)
            if (a.nseg == 1 && a.seg[0].type == MI355_GGML_Q6_K && (a.epi == MI355_EPI_STORE || a.epi == MI355_EPI_RESID) && parts == 1 &&
                g_tune_qpg_fepi) {
                QmmArgs r = a;
                r.norm_w = nullptr;
                hipLaunchKernelGGL((qpg_gemm_q6k_lds_kernel<true, 2, true>), dim3(Tpad / 64, (n_slots + 15) / 16), dim3(512), (size_t)QPG6_LDS_BYTES, st, r, im, C,
                                   ldp, n_slots, 0);
                return (int)hipGetLastError();
            }
            return (int)hipErrorNotSupported;
        }
    }
    // q | k | v of a prompt step (EPI_QKV_ROPE_CACHE, round 6): q and k (both Q4_K or both Q5_K) -- and v where it has their type -- go through the fused store loop
    // (RoPE + bf16 + cache scatter in the GEMM); a Q6_K v (half the layers of a Q4_K_M file) keeps its own GEMM + the epilogue launch, which
    // then sees q and k as empty segments (n_rows = 0: their columns of C were never written)
#ifndef QPG_FUSE_Q6K
#define QPG_FUSE_Q6K 1          // A/B builds: 0 = Q6_K prompt GEMMs write the C buffer and an epilogue launch follows (rounds 2-5)
#endif
#ifndef QPG6_SPLIT_SMALL
#define QPG6_SPLIT_SMALL 1      // A/B builds: 0 = the Q6_K value projection always in 256-row workgroups
#endif
#ifndef QPG_FUSE_QKV
#define QPG_FUSE_QKV 1          // A/B builds: 0 = q | k | v through the C buffer and the epilogue launch (rounds 2-5)
#endif
    // (from 1024 tokens: measured +0.7 % at 2048 and +1.2 % at 4096 tokens, -1.9 % at 512 -- profiles/r06_prompt_qkv_fused_ab.txt)
    if (QPG_FUSE_QKV && T >= 1024 && g_tune_qpg_fepi && parts == 1 && a.epi == MI355_EPI_QKV_ROPE_CACHE && a.nseg == 3 &&
        a.seg[0].type != MI355_GGML_Q6_K && a.seg[1].type == a.seg[0].type &&
        (a.seg[2].type == a.seg[0].type || (QPG_FUSE_Q6K && a.seg[2].type == MI355_GGML_Q6_K))) {
        const bool v4 = a.seg[2].type == a.seg[0].type;                 // v goes with q and k
        const bool q5 = a.seg[0].type == MI355_GGML_Q5_K;
        QmmArgs r = a;
        r.norm_w = nullptr;                                         // applied while the image was built
        if (!v4) r.nseg = 2;
        const int f_slots = qmm_total_tiles(r);
        const dim3 gf(Tpad / 64, (f_slots + 15) / 16);
        if (q5) hipLaunchKernelGGL((qpg_gemm_lds2_kernel<true, false, MI355_GGML_Q5_K>), gf, dim3(512), (size_t)QPG5_BYTES, st, r, im, C, ldp, f_slots, 0);
        else hipLaunchKernelGGL((qpg_gemm_lds2_kernel<true>), gf, dim3(512), (size_t)QPG2_BYTES, st, r, im, C, ldp, f_slots, 0);
        if (v4) return (int)hipGetLastError();
        // v (Q6_K): its own GEMM with the fused store loop; q and k stay in the descriptor as EMPTY segments (no tiles) so that the value
        // segment keeps its role (2 = v: bf16 + cache scatter, no rotation) and its row offsets
        QmmArgs rv = a;
        rv.norm_w = nullptr;
        rv.seg[0].n_tiles = 0; rv.seg[1].n_tiles = 0;
        // (one row tile per wave where two would leave CUs empty: 1024 rows x 2048 tokens = 128 workgroups of 256 rows)
        const int vt = a.seg[2].n_tiles;
        if (QPG6_SPLIT_SMALL && (Tpad / 64) * ((vt + 15) / 16) < mi355_num_cus())
            hipLaunchKernelGGL((qpg_gemm_q6k_lds_kernel<true, 1>), dim3(Tpad / 64, (vt + 7) / 8), dim3(512), (size_t)QPG6_LDS_BYTES, st, rv, im, C, ldp, vt, 0);
        else
            hipLaunchKernelGGL((qpg_gemm_q6k_lds_kernel<true>), dim3(Tpad / 64, (vt + 15) / 16), dim3(512), (size_t)QPG6_LDS_BYTES, st, rv, im, C, ldp, vt, 0);
        return (int)hipGetLastError();
    }
    // the whole mat-mul is one Q6_K run and its epilogue is a store / residual add: fused store loop, no C buffer, no epilogue launch
    // (from 4096 tokens -- measured: +1.2 % at 4096, -0.2 % at 2048: profiles/r06_prompt_q6k_fused_ab.txt)
    bool all_q6 = true;
    for (int s = 0; s < a.nseg; ++s) all_q6 = all_q6 && a.seg[s].type == MI355_GGML_Q6_K;
    if (QPG_FUSE_Q6K && g_tune_qpg_fepi && parts == 1 && T >= 4096 && all_q6 && (a.epi == MI355_EPI_STORE || a.epi == MI355_EPI_RESID)) {
        QmmArgs r = a;
        r.norm_w = nullptr;
        hipLaunchKernelGGL((qpg_gemm_q6k_lds_kernel<true>), dim3(Tpad / 64, (n_slots + 15) / 16), dim3(512), (size_t)QPG6_LDS_BYTES, st, r, im, C, ldp, n_slots, 0);
        return (int)hipGetLastError();
    }
    qmm_for_each_run(a, [&](const QmmArgs& r, int run_slots, int slot_base) {
        if (r.seg[0].type == MI355_GGML_Q4_K) {
            // 64 x 256, waves 64 x 32, two workgroups per CU
            const dim3 g4(Tpad / 64, (run_slots + 15) / 16), b_(512);
            if (parts == 1)                                             // one activation plane: image and weights through LDS by DMA
                hipLaunchKernelGGL((qpg_gemm_lds2_kernel<false>), g4, b_, (size_t)QPG2_BYTES, st, r, im, C, ldp, run_slots, slot_base);
            else                                                        // hi + lo planes ("exact" activations): the register-fed form
                hipLaunchKernelGGL((qpg_gemm_kernel<MI355_GGML_Q4_K, 4, 2, 1, 8, 2>), g4, b_, (size_t)2 * 2 * 64 * QPG_ROWB, st, r, im, C, ldp, run_slots, slot_base);
        } else if (r.seg[0].type == MI355_GGML_Q5_K) {                  // the same two kernels over Q5_K tiles
            const dim3 g5(Tpad / 64, (run_slots + 15) / 16), b_(512);
            if (parts == 1)
                hipLaunchKernelGGL((qpg_gemm_lds2_kernel<false, false, MI355_GGML_Q5_K>), g5, b_, (size_t)QPG5_BYTES, st, r, im, C, ldp, run_slots, slot_base);
            else
                hipLaunchKernelGGL((qpg_gemm_kernel<MI355_GGML_Q5_K, 4, 2, 1, 8, 2>), g5, b_, (size_t)2 * 2 * 64 * QPG_ROWB, st, r, im, C, ldp, run_slots, slot_base);
        } else {
            if (parts == 1) {                      // Q6_K: 64 tokens x 256 rows per workgroup; token blocks fastest
                const dim3 grid(Tpad / 64, (run_slots + 15) / 16);
                hipLaunchKernelGGL((qpg_gemm_q6k_lds_kernel<false>), grid, dim3(512), (size_t)QPG6_LDS_BYTES, st, r, im, C, ldp, run_slots, slot_base);
            } else {
                const dim3 grid(Tpad / 32, (run_slots + 15) / 16);     // 32 tokens x 256 rows, register-fed: hi + lo planes ("exact" activations)
                hipLaunchKernelGGL((qpg_gemm_q6k_kernel<2, 2>), grid, dim3(512), 16 * 1024, st, r, im, C, ldp, run_slots, slot_base);
            }
        }
    });
    a.norm_w = nullptr;                                     // applied while the image was built
    hipLaunchKernelGGL(qmm_epilogue_kernel, dim3((ldp + 255) / 256, T), dim3(256), 0, st, a, C, ldp, 1, T, (const float*)nullptr,
                       QmgChainOut{nullptr, nullptr, nullptr, 0, 0, 0, 0}, (const float*)im.row_scale);
    return (int)hipGetLastError();
}

// ================================================================================================ 1..8 tokens
// Q4_K / Q6_K (WT = the launch's uniform tile type, 0 = mixed): qmm_kernel, or qmm_moe_kernel for (token, slot) pairs of expert mat-vecs
template <int BT, int R, int WT>
static int qmm_launch_btrw(QmmArgs& a, int n_wg, hipStream_t st) {
    a.kch = 0;
    static Mi355DevOnce attr_done;
    qmm_allow_lds(attr_done, 160 * 1024, qmm_kernel<BT, R, WT, 0, 0>, qmm_kernel<BT, R, WT, 0, 1>, qmm_kernel<BT, R, WT, 1, 0>, qmm_kernel<BT, R, WT, 1, 1>);
    // (token, slot) pairs of a mixture-of-experts launch are workgroups too: all of them should be resident at once
    // the paired (gate / up) single-token launch runs TWO waves per workgroup: measured on the product build, alternated on one box
    // (profiles/r06_b1_gateup_waves_ab.txt): 2 waves 1.841 ms per step, 4 waves 1.862, 8 waves 1.875.  The occupancy rule below picked 2 while
    // the kernel needed 134 VGPRs and flipped to 4 when a register-allocation change brought it to 127 -- a choice that depends on the
    // allocator's mood is not a choice (QMM_NW_PAIRED: A/B builds)
#ifndef QMM_NW_PAIRED
#define QMM_NW_PAIRED 2
#endif
    static int blocks_per_cu[3] = {-1, -1, -1};
    const int NW = (QMM_NW_PAIRED > 0 && a.paired && BT == 1 && !a.moe_expert && a.K / 256 >= QMM_NW_PAIRED)
                       ? QMM_NW_PAIRED
                       : qmm_pick_nw((const void*)qmm_kernel<BT, R, WT, 0, 1>, blocks_per_cu, BT, R, n_wg * (a.moe_expert ? a.moe_pairs : 1), a.K / 256);
    const size_t shm = qmm_lds_bytes(BT, R, NW);
    if (shm > 160 * 1024) return (int)hipErrorInvalidValue;
    if (a.moe_expert) {
        if constexpr (BT == 1) {
            static Mi355DevOnce moe_attr_done;
            qmm_allow_lds(moe_attr_done, 160 * 1024, qmm_moe_kernel<R, WT, 0, 0>, qmm_moe_kernel<R, WT, 0, 1>, qmm_moe_kernel<R, WT, 1, 0>, qmm_moe_kernel<R, WT, 1, 1>);
            qmm_by_x_and_norm(a, [&](auto XB, auto NRM) {
                hipLaunchKernelGGL((qmm_moe_kernel<R, WT, decltype(XB)::value, decltype(NRM)::value>), dim3(n_wg, a.moe_pairs), dim3(64 * NW), shm, st, a);
            });
        } else {
            return (int)hipErrorInvalidValue;
        }
    } else {
        qmm_by_x_and_norm(a, [&](auto XB, auto NRM) {
            hipLaunchKernelGGL((qmm_kernel<BT, R, WT, decltype(XB)::value, decltype(NRM)::value>), dim3(n_wg), dim3(64 * NW), shm, st, a);
        });
    }
    return (int)hipGetLastError();
}

template <int BT, int R>
static int qmm_launch_btr(QmmArgs& a, int wt, int n_wg, hipStream_t st) {
    if (wt == MI355_GGML_Q4_K) return qmm_launch_btrw<BT, R, MI355_GGML_Q4_K>(a, n_wg, st);
    if (wt == MI355_GGML_Q6_K) return qmm_launch_btrw<BT, R, MI355_GGML_Q6_K>(a, n_wg, st);
    return qmm_launch_btrw<BT, R, 0>(a, n_wg, st);
}

// any Q5_K segment (qmm_q5k.inc: q5k_kernel; MIXED = other k-quant types next to it)
template <int BT, int R, bool MIXED>
static int q5k_launch_btrm(QmmArgs& a, int n_wg, hipStream_t st) {
    static Mi355DevOnce attr_done;
    static int blocks_per_cu[3] = {-1, -1, -1};
    qmm_allow_lds(attr_done, 160 * 1024, q5k_kernel<BT, R, MIXED>);
    const int NW = qmm_pick_nw((const void*)q5k_kernel<BT, R, MIXED>, blocks_per_cu, BT, R, n_wg, a.K / 256);
    const size_t shm = qmm_lds_bytes(BT, R, NW);
    if (shm > 160 * 1024) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL((q5k_kernel<BT, R, MIXED>), dim3(n_wg), dim3(64 * NW), shm, st, a);
    return (int)hipGetLastError();
}

// BT = tokens staged per workgroup; R = tiles per workgroup, wt = uniform tile type of the launch (0: mixed), q5 = a Q5_K segment is among them
template <int BT>
static int qmm_launch_bt(QmmArgs& a, int R, int wt, bool q5, int n_wg, hipStream_t st) {
    if (q5) {
        if (R == 2) return wt == 0 ? q5k_launch_btrm<BT, 2, true>(a, n_wg, st) : q5k_launch_btrm<BT, 2, false>(a, n_wg, st);
        return wt == 0 ? q5k_launch_btrm<BT, 1, true>(a, n_wg, st) : q5k_launch_btrm<BT, 1, false>(a, n_wg, st);
    }
    if (R == 4) return qmm_launch_btr<BT, 4>(a, wt, n_wg, st);
    if (R == 2) return qmm_launch_btr<BT, 2>(a, wt, n_wg, st);
    return qmm_launch_btr<BT, 1>(a, wt, n_wg, st);
}
// 1..8 tokens -> the build for 1 / 2 / 4 / 8 staged tokens
static int qmm_launch_decode(QmmArgs& a, int R, int wt, bool q5, int n_wg, hipStream_t st) {
    if (a.B == 1) return qmm_launch_bt<1>(a, R, wt, q5, n_wg, st);
    if (a.B == 2) return qmm_launch_bt<2>(a, R, wt, q5, n_wg, st);
    if (a.B <= 4) return qmm_launch_bt<4>(a, R, wt, q5, n_wg, st);
    return qmm_launch_bt<8>(a, R, wt, q5, n_wg, st);
}

// Q8_0 (q8_0_matmul_kernel): one launch whatever the token count

static int q8_0_launch(const QmmArgs& a, hipStream_t st) {
    if (a.nseg != 1 || a.norm_w || a.moe_expert || (a.epi != MI355_EPI_STORE && a.epi != MI355_EPI_RESID) || (a.K % 32) || a.K <= 0)
        return (int)hipErrorInvalidValue;
    if (a.B == 0) return 0;
    hipLaunchKernelGGL(q8_0_matmul_kernel, dim3(a.seg[0].n_rows, (a.B + 7) / 8), dim3(64), 0, st, a);
    return (int)hipGetLastError();
}

// parity mode 2 (qmm_exact.inc): one launch per token
static int qmm_exact_launch(const QmmArgs& a, hipStream_t st) {
    const int total_tiles = qmm_total_tiles(a);
    for (int b = 0; b < a.B; ++b) {
        const QmmArgs w = qmm_token_window(a, b, 1);
        if (a.paired) hipLaunchKernelGGL((qmm_exact_kernel<2>), dim3(a.seg[0].n_tiles), dim3(256), 0, st, w);
        else hipLaunchKernelGGL((qmm_exact_kernel<1>), dim3(total_tiles), dim3(256), 0, st, w);
    }
    return (int)hipGetLastError();
}

// ================================================================================================ the router
// A launch below the prompt threshold is cut into windows of tokens.  Which launcher serves the next window and how many tokens it
// takes, from the types of the launch (q5 = a Q5_K segment, pure_q5 = nothing else), the tokens left and mi355_set_tuning(24, .):
//   Q4_K / Q6_K      32, then 9..32 tokens: qw1_launch (one f16 plane), with "exact" activations qmg_launch (hi + lo planes)
//   every tile Q5_K  32, then 9..32 tokens: q5g_launch
//   Q5_K mixed with other types: 8-token windows on q5k_kernel<., ., true> (the 9..32-token kernels take one tile type per run)
//   <= 8 tokens left: the streaming mat-vec kernels, built for 1 / 2 / 4 / 8 staged tokens
enum QmmRoute { QMM_DECODE, QMM_WIDE1, QMM_WIDE_EXACT, QMM_WIDE_Q5 };
struct QmmChunk { QmmRoute route; int bn; };
static QmmChunk qmm_next_chunk(bool q5, bool pure_q5, int left, bool exact_act) {
    if (left <= 8 || (q5 && !pure_q5)) return {QMM_DECODE, left < 8 ? left : 8};
    const int bn = left < 8 * QMW_MAXMT ? left : 8 * QMW_MAXMT;
    return {pure_q5 ? QMM_WIDE_Q5 : (exact_act ? QMM_WIDE_EXACT : QMM_WIDE1), bn};
}

// Run one fused quantised mat-mul over token rows [0, B).  The order of the checks is part of the interface (which error a bad call gets)
int mi355_qmm_launch(QmmArgs a, int64_t stream) {
    hipStream_t st = to_stream(stream);
    {   // images staged WITHOUT backing activations (fused MoE staging) may only be consumed by the grouped 9..32-token launch they were
        // built for; any other route would read rows nobody wrote.  qw1_launch checks the remaining fields (tile height, k, norm, groups)
        QmgStream& qs0 = qmg_stream(st);
        if (qs0.chain.valid && qs0.chain.prestaged && qs0.chain.x == a.x && qs0.chain.st == st &&
            !(a.grp_n > 1 && qmg_wide_one_launch(a.B) && a.nseg >= 1 && a.seg[0].type != MI355_GGML_Q8_0)) {
            qs0.chain.valid = false;
            mi355_note_error((int)hipErrorInvalidValue);
            return (int)hipErrorInvalidValue;
        }
    }
    if (a.nseg >= 1 && a.seg[0].type == MI355_GGML_Q8_0) return q8_0_launch(a, st);
    if (a.K <= 0 || (a.K % 256) || a.B < 0 || a.nseg < 1 || a.nseg > 3) return (int)hipErrorInvalidValue;
    if (a.B == 0) return 0;
    // ---- validation, and what the choices below need to know about the segments
    int total_tiles = 0, wt = a.seg[0].type;                  // wt: uniform tile type of the launch, else 0 (mixed)
    bool div4 = true, div2 = true, q5 = false, any_q6 = false;
    for (int s = 0; s < a.nseg; ++s) {
        if (!is_kquant(a.seg[s].type)) return (int)hipErrorInvalidValue;
        q5 = q5 || a.seg[s].type == MI355_GGML_Q5_K;
        any_q6 = any_q6 || a.seg[s].type == MI355_GGML_Q6_K;
        if (a.seg[s].type != wt) wt = 0;
        total_tiles += a.seg[s].n_tiles;
        if (a.seg[s].n_tiles % 4) div4 = false;
        if (a.seg[s].n_tiles % 2) div2 = false;
    }
    // the expert, grouped and block-table kernels and the parity-mode kernel decode Q4_K / Q6_K only: refuse Q5_K, never mis-decode it
    if (q5 && (a.moe_expert || a.grp_n > 1 || a.blk_tab || g_qmm_exact)) return (int)hipErrorNotSupported;
    if (a.paired && (a.nseg != 2 || a.seg[0].n_tiles != a.seg[1].n_tiles)) return (int)hipErrorInvalidValue;
    if (q5) qmg_stream(st).chain.valid = false;               // no Q5_K launch consumes or stages an activation image for a successor
    if (a.grp_n > 1) {
        // grouped launch: grp_n mat-muls of these shapes.  The 9..32-token path runs them as the z extent of its launches; everything
        // else (other token counts, the exact modes) runs them one after the other -- same results, the descriptor's meaning is the loop
        if (a.moe_expert || a.bias || (a.epi != MI355_EPI_STORE && a.epi != MI355_EPI_SILU_MUL)) return (int)hipErrorInvalidValue;
        if (!qmg_wide_one_launch(a.B)) {
            const size_t xes = (a.x_dtype == MI355_DTYPE_BF16) ? 2 : 4;
            for (int e = 0; e < a.grp_n; ++e) {
                QmmArgs r = a;
                r.grp_n = 0; r.chain_next = 0;
                for (int s = 0; s < a.nseg; ++s) r.seg[s].w = a.seg[s].w + (size_t)e * a.moe_stride[s];
                r.x = static_cast<const uint8_t*>(a.x) + (size_t)e * a.grp_x * xes;
                r.out = a.out + (size_t)e * a.grp_out;
                if (a.rows_dev) r.rows_dev = a.rows_dev + e;
                const int rc = mi355_qmm_launch(r, stream);
                if (rc) return rc;
            }
            return 0;
        }
    }
    if (g_qmm_exact && !a.moe_expert && !a.rows_dev) return qmm_exact_launch(a, st);   // parity mode 2 (tests only)
    // ---- tiles per workgroup: amortise the activation staging but keep >= ~1024 workgroups (4 per CU).  Q5_K stops at 2 (its ring of
    // units and the fifth-bit words: qmm_q5k.inc); gate / up pairs are two by construction
    int R;
    if (a.paired) {
        R = (!q5 && a.seg[0].n_tiles % 2 == 0 && a.seg[0].n_tiles / 2 >= 1024) ? 4 : 2;
    } else {
        R = 1;
        if (div2 && total_tiles / 2 >= 1024) R = 2;
        // four Q6_K tiles per workgroup need more than the register file (256 VGPRs + spills once the body is branch-free):
        // lm_head of Llama-3-8B 108 us with R = 4, 74 us with R = 2
        if (div4 && total_tiles / 4 >= 1024 && !any_q6 && !q5) R = 4;
    }
    const int n_wg = a.paired ? a.seg[0].n_tiles / (R / 2) : total_tiles / R;
    if (a.moe_expert) {                                       // every (token, slot) pair is a 1-token mat-vec of its own expert
        if (a.moe_pairs < 1 || a.moe_xdiv < 1 || a.epi == MI355_EPI_QKV_ROPE_CACHE || a.epi == MI355_EPI_RESID) return (int)hipErrorInvalidValue;
        a.B = 1;
        return qmm_launch_bt<1>(a, R, wt, false, n_wg, st);
    }
    // ---- prompt step: the hand-written quantised GEMM (qmm_prefill.inc); mi355_set_tuning(6, 0) = the chunks below (A/B)
    const bool prompt = a.B >= (q5 ? Q5P_MIN_TOKENS : QMP_MIN_TOKENS);
    if (a.blk_tab && !(prompt && g_tune_prefill_gemm == 1)) return (int)hipErrorNotSupported;   // only the prompt GEMM reads a block table
    if (prompt && g_tune_prefill_gemm) {
        const int rcq = qpg_launch(a, st);
        if (rcq != (int)hipErrorNotSupported || a.blk_tab) return rcq;
    }
    // ---- everything else: windows of tokens, the weights streamed once per window
    for (int b0 = 0; b0 < a.B;) {
        const QmmChunk c = qmm_next_chunk(q5, wt == MI355_GGML_Q5_K, a.B - b0, g_tune_exact_act != 0);
        QmmArgs w = qmm_token_window(a, b0, c.bn);
        int rc;
        if (c.route == QMM_WIDE1) rc = c.bn <= 16 ? qw1_launch<1>(w, st) : qw1_launch<2>(w, st);
        else if (c.route == QMM_WIDE_EXACT) rc = c.bn <= 16 ? qmg_launch<2>(w, st) : (c.bn <= 24 ? qmg_launch<3>(w, st) : qmg_launch<4>(w, st));
        else if (c.route == QMM_WIDE_Q5) rc = c.bn <= 16 ? q5g_launch<1>(w, st) : q5g_launch<2>(w, st);
        else rc = qmm_launch_decode(w, R, wt, q5, n_wg, st);
        if (rc) return rc;
        b0 += c.bn;
    }
    return 0;
}
