// Q5_K (GGML type 13, the Q5_K_M mix) on the quantised mat-mul path: device code only.  Included by qmatmul.hip after the shared device
// helpers; the launchers (q5k_launch_btrm, q5g_launch) and the routing are in qmm_launch.inc.
//
// Reference boundary: candle `QMatMul::forward` over a Q5K tensor (SURVEY App. C), same call sites as Q4_K / Q6_K.
// block_q5_K = f16 d, dmin | scales[12] (6-bit sc_j, m_j as Q4_K) | qh[32] | qs[128];  w = d sc_j q - dmin m_j with
// q = nibble | fifth bit << 4, the fifth bit of element l of sub-block j being bit j of qh[l].
//
// Tile (mi355_qweight_repack, 2816 B per 16 rows x 256 k): header and nibble planes as the Q4_K tile, then the lane's 64
// fifth bits transposed into consumption order (layout note next to the repack), so that a code is three bit operations:
//     (qs >> sh) & 0x000F000F  |  (qh >> (2j + c - 4)) & 0x00100010  |  exponent pattern
// Prompt steps (>= Q5P_MIN_TOKENS = 192 tokens) take the Q5_K arms of the prompt-step GEMM in qmm_prefill.inc (qpg_gemm_lds2_kernel<., false,
// MI355_GGML_Q5_K>; hi + lo activation planes: qpg_gemm_kernel<MI355_GGML_Q5_K, ...>) through qpg_launch.  Two kernels here:
//   * q5k_kernel (1..8 tokens): the streaming mat-vec of the path -- per-wave LDS image of hi + lo bf16 activation rows,
//     codes 128 + q exact in bf16, the -128 MFMA that cancels the offset and yields the sub-block sums of the minimum
//     term, d / dmin once per tile, register ring of (k-block, tile) units with a compile-time load count (4 per unit,
//     5 in launches that mix in Q4_K / Q6_K tiles: those tiles go through compute3_q4k / compute3_q6k), the common epilogue;
//   * q5g_gemm_kernel (9..32 tokens per launch; 33..191 tokens, and prompts with mi355_set_tuning(6, 0), in 32-token chunks): one f16 activation plane with a
//     power-of-two scale per (token, k-block) -- the image of qw1_prep_kernel -- B operand sc_j q exact in f16
//     (63 * 31 = 1953 < 2048), the eight sub-block MFMAs of a k-block chained in one accumulator, the minimum term as one
//     K = 16 MFMA per m-tile against the staged sub-block sums, d / dmin / 2^e applied per (row, k-block).  Eight waves =
//     eight row tiles per workgroup and ALL of them compute: the next k-block's image travels global -> registers -> LDS
//     (each wave copies its 1-KiB chunks while it multiplies; two LDS stages, one barrier per k-block), split K,
//     partial sums [ks][token][row] finished by qmm_epilogue_kernel (every epilogue of the path).
// Not served (mi355_qmm_launch: hipErrorNotSupported, nothing computed): MoE expert ids, grouped launches, block tables, parity mode 2.

typedef unsigned int q5k_u32x2_t __attribute__((ext_vector_type(2)));

// MIXED = false: every tile of the launch is Q5_K, four loads per unit.  MIXED = true: five loads whatever the tile's type
// (Q4_K adds two same-line dummies, Q5_K one; its fifth-bit words arrive as the 16-B line shared by a lane pair), so that the
// number of outstanding loads stays a compile-time constant and the vmcnt waits stay counted.
template <bool MIXED>
__device__ __forceinline__ TileRegs q5k_load_tile(int type, const uint8_t* __restrict__ t, int lane) {
    TileRegs r;
    const int row = lane & 15;
    const uint4* t4 = reinterpret_cast<const uint4*>(t);
    r.a = ld_nt16(t4 + row);                    // d, dmin, scales[12]   (Q6_K: 16 x i8 scales)
    r.b = ld_nt16(t4 + 16 + lane);              // nibble plane 0        (Q6_K: ql half 0)
    r.c = ld_nt16(t4 + 80 + lane);              // nibble plane 1        (Q6_K: ql half 1)
    if constexpr (!MIXED) {
        const q5k_u32x2_t h = __builtin_nontemporal_load(reinterpret_cast<const q5k_u32x2_t*>(t + 2304) + lane);
        r.d = make_uint4(h.x, h.y, 0, 0);
        r.e = 0;
    } else {
        const bool q6 = type == MI355_GGML_Q6_K, q5 = type == MI355_GGML_Q5_K;
        const uint4 h = ld_nt16(t4 + (q6 ? 144 + lane : (q5 ? 144 + (lane >> 1) : 0)));
        r.d = (q5 && (lane & 1)) ? make_uint4(h.z, h.w, 0, 0) : h;
        r.e = __builtin_nontemporal_load(reinterpret_cast<const uint16_t*>(t + (q6 ? 3328 : 0)) + (q6 ? row : 0));
    }
    return r;
}

// fifth bits of the element pair (c, c + 2) of sub-block j, at bit 4 of both halves (n = 2j + c; the tile format's order)
__device__ __forceinline__ uint32_t q5k_hbits(uint32_t h, int n, uint32_t bit) {
    return (n >= 4 ? (h >> (n - 4)) : (h << (4 - n))) & bit;
}

// RR Q5_K tiles x one k-block x up to 8 tokens (hi rows 0..7, lo rows 8..15 of the same MFMA)
template <int BT, int NV, int RR>
__device__ __forceinline__ void compute_q5k(const TileRegs* w, const uint8_t* ximg, int lane, float (*y)[NV]) {
    const int m = lane & 15, kg = lane >> 4;
    const uint8_t* abase = ximg + ((size_t)kg * (2 * BT) + a_row_of<BT>(m)) * 16;
    uint4 aw[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) aw[j] = *reinterpret_cast<const uint4*>(abase + (size_t)j * 4 * (2 * BT) * 16);
    float d[RR], dm[RR];
    uint32_t scl[RR], sch[RR], mnl[RR], mnh[RR];
#pragma unroll
    for (int r = 0; r < RR; ++r) {
        d[r] = f16_bits_to_f32((uint16_t)(w[r].a.x & 0xFFFF));
        dm[r] = f16_bits_to_f32((uint16_t)(w[r].a.x >> 16)) * (1.f / 128.f);
        const uint32_t s0 = w[r].a.y, s1 = w[r].a.z, s2 = w[r].a.w;
        scl[r] = s0 & 0x3F3F3F3Fu;
        mnl[r] = s1 & 0x3F3F3F3Fu;
        sch[r] = (s2 & 0x0F0F0F0Fu) | ((s0 >> 2) & 0x30303030u);
        mnh[r] = ((s2 >> 4) & 0x0F0F0F0Fu) | ((s1 >> 2) & 0x30303030u);
        asm volatile("" : "+v"(scl[r]), "+v"(sch[r]), "+v"(mnl[r]), "+v"(mnh[r]));   // one v_cvt_f32_ubyteN per value below
    }
    uint32_t nib = 0x000F000Fu, bit5 = 0x00100010u, n128 = 0xC300C300u;   // bf16 -128.0 twice
    asm volatile("" : "+v"(nib), "+v"(bit5), "+v"(n128));
    const uint4 negw = make_uint4(n128, n128, n128, n128);
    float sP[RR][NV], sM[RR][NV];
#pragma unroll
    for (int r = 0; r < RR; ++r)
#pragma unroll
        for (int v = 0; v < NV; ++v) { sP[r][v] = 0.f; sM[r][v] = 0.f; }
    const f32x4_t zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const bf16x8_t af = __builtin_bit_cast(bf16x8_t, aw[j]);
        // -128 * sum(x) of the sub-block in accumulator layout: cancels the code offset AND is the sum of the minimum term
        const f32x4_t cin = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, __builtin_bit_cast(bf16x8_t, negw), zero, 0, 0, 0);
        const int p = j >> 2, pr = (j >> 1) & 1, sh = (j & 1) * 4;
#pragma unroll
        for (int r = 0; r < RR; ++r) {
            const uint4 qs = p ? w[r].c : w[r].b;
            const uint32_t w0 = pr ? qs.z : qs.x, w1 = pr ? qs.w : qs.y;
            const uint32_t h0 = w[r].d.x, h1 = w[r].d.y;
            uint4 bw;                                                // codes 128 + q (q < 32): exact bf16
            bw.x = ((w0 >> sh) & nib) | (q5k_hbits(h0, 2 * j, bit5) | BF16_128);            // elements (b0, b2)
            bw.y = ((w0 >> (sh + 8)) & nib) | (q5k_hbits(h0, 2 * j + 1, bit5) | BF16_128);  // elements (b1, b3)
            bw.z = ((w1 >> sh) & nib) | (q5k_hbits(h1, 2 * j, bit5) | BF16_128);            // elements (b4, b6)
            bw.w = ((w1 >> (sh + 8)) & nib) | (q5k_hbits(h1, 2 * j + 1, bit5) | BF16_128);  // elements (b5, b7)
            const f32x4_t acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, __builtin_bit_cast(bf16x8_t, bw), cin, 0, 0, 0);
            const float sc = (float)((((j < 4) ? scl[r] : sch[r]) >> (8 * (j & 3))) & 0xFF);
            const float mn = (float)((((j < 4) ? mnl[r] : mnh[r]) >> (8 * (j & 3))) & 0xFF);
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                sP[r][v] = fmaf(sc, acc[v], sP[r][v]);
                sM[r][v] = fmaf(mn, cin[v], sM[r][v]);               // sign folded: cin = -128 sum(x), dm = dmin / 128
            }
        }
    }
#pragma unroll
    for (int r = 0; r < RR; ++r)
#pragma unroll
        for (int v = 0; v < NV; ++v) y[r][v] = fmaf(d[r], sP[r][v], fmaf(dm[r], sM[r][v], y[r][v]));
}

// One workgroup = R row tiles x all of K; its waves split the k-blocks and walk their (k-block, tile) units through a register
// ring.  A Q5_K unit is 4 + 4 + 4 + 2 dwords per lane against Q4_K's 12, and its unpack keeps the fifth-bit words live next
// to the nibble words: the ring is max(R, 2) units deep (one k-block ahead at R = 2, two at R = 1), and R stops at 2.
// hipcc for gfx950, -O3, no spills: VGPRs at R = 1 / R = 2 -- 1 token 109 / 126 (4 waves per SIMD), 2 tokens 135 / 139 (3),
// 4 tokens 181 / 205 (2), 8 tokens 213 / 223 (2); launches that mix types: 125 / 112, 153 / 135, 205 / 181, 237 / 203.
template <int BT, int R, bool MIXED>
__global__ void __launch_bounds__(512) q5k_kernel(const QmmArgs a) {
    qmm_kernarg_burst(a);
    constexpr int NV = BT < 4 ? BT : 4;
    constexpr int PF = R > 2 ? R : 2;
    constexpr int PFK = PF / R;                                    // ring depth in k-blocks
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), NW = blockDim.x >> 6;
    const int nkb = a.K >> 8;

    int segi[R], tile[R];
    if (a.paired) {
#pragma unroll
        for (int r = 0; r < R; ++r) { segi[r] = r & 1; tile[r] = blockIdx.x * (R / 2 > 0 ? R / 2 : 1) + (r >> 1); }
    } else {
        int t = blockIdx.x * R, s = 0;
        const int nt0 = a.seg[0].n_tiles, nt1 = a.seg[1].n_tiles;
        if (a.nseg > 1 && t >= nt0) {
            t -= nt0; s = 1;
            if (a.nseg > 2 && t >= nt1) { t -= nt1; s = 2; }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) { segi[r] = s; tile[r] = t + r; }      // launcher: n_tiles % R == 0 in every segment
    }
    const uint8_t* wbase[R];
    int wtype[R], wtb[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        wtype[r] = MIXED ? seg_pick(a.seg[0].type, a.seg[1].type, a.seg[2].type, segi[r]) : MI355_GGML_Q5_K;   // wave-uniform
        wtb[r] = wtype[r] == MI355_GGML_Q5_K ? Q5K_TILE : (wtype[r] == MI355_GGML_Q4_K ? Q4K_TILE : Q6K_TILE);
        const uint8_t* wp = a.seg[0].w;
        if (segi[r] == 1) wp = a.seg[1].w;
        else if (segi[r] == 2) wp = a.seg[2].w;
        wbase[r] = wp + (size_t)tile[r] * nkb * wtb[r];
    }
    const float* nwp = a.norm_w ? a.norm_w : reinterpret_cast<const float*>(a.seg[0].w);   // any readable K floats: static load count

    constexpr int XW = 32 * 2 * BT * 16;                          // per-wave hi / lo fragment image of one k-block
    uint8_t* ximg = smem + (size_t)wave * XW;
    float* red = reinterpret_cast<float*>(smem + (size_t)NW * XW);   // [NW][R][BT][16]
    float* red_ss = red + (size_t)NW * R * BT * 16;               // [NW][BT]

    float y[R][NV];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int v = 0; v < NV; ++v) y[r][v] = 0.f;
    float ss[BT];
#pragma unroll
    for (int b = 0; b < BT; ++b) ss[b] = 0.f;

    EpiPre ep;
    epi_pre_early<BT, R>(a, segi, tile, ep);

    // this wave's k-blocks: kb = wave + NW kbi; ring slot s <-> (kbi0 + s / R, tile s % R)
    const int n_my_kb = (nkb > wave) ? (nkb - wave + NW - 1) / NW : 0;
    const int kb_last = n_my_kb > 0 ? wave + NW * (n_my_kb - 1) : 0;
    XRegs<BT> xr[PFK];
    TileRegs buf[PF];
#pragma unroll
    for (int q = 0; q < PFK; ++q) {
        const int kb = wave + NW * q;
        xr[q] = load_x<BT>(a, kb <= kb_last ? kb : kb_last, lane, nwp);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const bool ok = q < n_my_kb;
            buf[q * R + r] = q5k_load_tile<MIXED>(wtype[r], ok ? wbase[r] + (size_t)kb * wtb[r] : wbase[r], ok ? lane : 0);
        }
    }
    for (int kbi0 = 0; kbi0 < n_my_kb; kbi0 += PFK) {
#pragma unroll
        for (int q = 0; q < PFK; ++q) {
            const int kbi = kbi0 + q;
            const bool active = kbi < n_my_kb;                    // wave-uniform
            if (active) stage_kblock3<BT>(a, xr[q], ximg, lane, ss);
            const int kbn = wave + NW * (kbi + PFK);
            xr[q] = load_x<BT>(a, kbn <= kb_last ? kbn : kb_last, lane, nwp);
            const bool ok = kbi + PFK < n_my_kb;
            if constexpr (!MIXED) {
                if (active) compute_q5k<BT, NV, R>(&buf[q * R], ximg, lane, y);   // the R tiles share C_in and the A fragments
            } else {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    if (!active) continue;
                    if (wtype[r] == MI355_GGML_Q5_K) compute_q5k<BT, NV, 1>(&buf[q * R + r], ximg, lane, &y[r]);
                    else if (wtype[r] == MI355_GGML_Q4_K) compute3_q4k<BT, NV, 1>(&buf[q * R + r], ximg, lane, &y[r]);
                    else compute3_q6k<BT, NV, 1>(&buf[q * R + r], ximg, lane, &y[r]);
                }
            }
            // unconditional refill (past the end: the tile's first line): a guarded load costs the counted waits
#pragma unroll
            for (int r = 0; r < R; ++r)
                buf[q * R + r] = q5k_load_tile<MIXED>(wtype[r], ok ? wbase[r] + (size_t)kbn * wtb[r] : wbase[r], ok ? lane : 0);
        }
    }
    epi_pre_late<BT>(a, ep);
    // hi + lo, then the cross-wave reduction in LDS: after the xor-32 add, lanes 0..31 hold batch 4 kg + v
    const int kg = lane >> 4, row = lane & 15;
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            y[r][v] += __shfl_xor(y[r][v], 32, 64);
            const int b = 4 * kg + v;
            if (kg < 2 && b < BT) red[(((size_t)wave * R + r) * BT + b) * 16 + row] = y[r][v];
        }
    if (a.norm_w) {
#pragma unroll
        for (int b = 0; b < BT; ++b) {
            const float t = wave_sum(ss[b]);
            if (lane == 0) red_ss[wave * BT + b] = t;
        }
    }
    __syncthreads();
    qmm_epilogue<BT, R>(a, red, red_ss, NW, segi, tile, ep);
}

// ================================================================================================ 9..32 tokens
// one Q5_K tile x one k-block x MT m-tiles of 16 tokens (image layout: qmm_wide1.inc).  Lane (m, kg): A fragment = token m,
// elements 8 kg .. 8 kg + 7 of the sub-block; the lane receives D[token 4 kg + v][weight row m].
template <int MT>
__device__ __forceinline__ void q5g_unit(const TileRegs& w, const uint8_t* __restrict__ L, int lane, float (&y)[MT][4]) {
    const int m = lane & 15, kg = lane >> 4;
    const uint8_t* sfrag = L + (size_t)32 * MT * 16 * 16;
    const float* tsc = reinterpret_cast<const float*>(sfrag + (size_t)MT * 512);
    const float d = f16_bits_to_f32((uint16_t)(w.a.x & 0xFFFF));
    const float ndmin = -f16_bits_to_f32((uint16_t)(w.a.x >> 16));
    const uint32_t s0 = w.a.y, s1 = w.a.z, s2 = w.a.w;
    const uint32_t scl = s0 & 0x3F3F3F3Fu, mnl = s1 & 0x3F3F3F3Fu;
    const uint32_t sch = (s2 & 0x0F0F0F0Fu) | ((s0 >> 2) & 0x30303030u);
    const uint32_t mnh = ((s2 >> 4) & 0x0F0F0F0Fu) | ((s1 >> 2) & 0x30303030u);
    const uint2 mb = bytes4_to_bf16x4((kg & 1) ? mnh : mnl);           // B fragment of the minimum term: k = 4 kg + e <-> j = 4 (kg & 1) + e
    uint32_t nib = 0x000F000Fu, bit5 = 0x00100010u, c1024 = 0x64006400u;
    asm volatile("" : "+v"(nib), "+v"(bit5), "+v"(c1024));
    const qmg_h2 k1024 = {(_Float16)1024.f, (_Float16)1024.f}, kneg = {(_Float16)(-1024.f), (_Float16)(-1024.f)};
    // scale pairs (sc0, sc2) (sc1, sc3) (sc4, sc6) (sc5, sc7) as f16: 1024 + sc is 0x6400 | sc, minus 1024 in one packed add
    qmg_h2 scp[4];
    scp[0] = __builtin_bit_cast(qmg_h2, (scl & 0x00FF00FFu) | c1024) - k1024;
    scp[1] = __builtin_bit_cast(qmg_h2, ((scl >> 8) & 0x00FF00FFu) | c1024) - k1024;
    scp[2] = __builtin_bit_cast(qmg_h2, (sch & 0x00FF00FFu) | c1024) - k1024;
    scp[3] = __builtin_bit_cast(qmg_h2, ((sch >> 8) & 0x00FF00FFu) | c1024) - k1024;
    f32x4_t acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    const uint32_t h0 = w.d.x, h1 = w.d.y;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const qmg_h2 sp = scp[2 * (j >> 2) + (j & 1)];               // holds sc_j in half (j >> 1) & 1
        const qmg_h2 S = ((j >> 1) & 1) ? __builtin_shufflevector(sp, sp, 1, 1) : __builtin_shufflevector(sp, sp, 0, 0);
        const qmg_h2 OFF = S * kneg;
        const int p = j >> 2, pr = (j >> 1) & 1, sh = (j & 1) * 4;
        const uint4 qs = p ? w.c : w.b;
        const uint32_t w0 = pr ? qs.z : qs.x, w1 = pr ? qs.w : qs.y;
        // f16 code 1024 + q ("0x6400 | q", q < 32), then fma(1024 + q, sc, -1024 sc) = sc q <= 1953: an exact f16 integer
        const qmg_h2 r0 = __builtin_elementwise_fma(__builtin_bit_cast(qmg_h2, ((w0 >> sh) & nib) | (q5k_hbits(h0, 2 * j, bit5) | c1024)), S, OFF);
        const qmg_h2 r1 = __builtin_elementwise_fma(__builtin_bit_cast(qmg_h2, ((w0 >> (sh + 8)) & nib) | (q5k_hbits(h0, 2 * j + 1, bit5) | c1024)), S, OFF);
        const qmg_h2 r2 = __builtin_elementwise_fma(__builtin_bit_cast(qmg_h2, ((w1 >> sh) & nib) | (q5k_hbits(h1, 2 * j, bit5) | c1024)), S, OFF);
        const qmg_h2 r3 = __builtin_elementwise_fma(__builtin_bit_cast(qmg_h2, ((w1 >> (sh + 8)) & nib) | (q5k_hbits(h1, 2 * j + 1, bit5) | c1024)), S, OFF);
        const qmg_h8 bw = {r0[0], r0[1], r1[0], r1[1], r2[0], r2[1], r3[0], r3[1]};
        const uint8_t* abase = L + ((size_t)(4 * j + kg) * (MT * 16) + m) * 16;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const uint4 aw = *reinterpret_cast<const uint4*>(abase + (size_t)mt * 16 * 16);
            acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(qmg_h8, aw), bw, acc[mt], 0, 0, 0);
        }
    }
    const f32x4_t zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        // sum_j m_j S_j[token]: the sub-block sums were formed once when the image was staged (bf16 hi / lo pieces, K = 16)
        const uint2 sa = *reinterpret_cast<const uint2*>(sfrag + ((size_t)(mt * 4 + kg) * 16 + m) * 8);
        const f32x4_t t1 = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(__builtin_bit_cast(s16x4_t, sa), __builtin_bit_cast(s16x4_t, mb), zero, 0, 0, 0);
        const float4 s4 = *reinterpret_cast<const float4*>(tsc + mt * 16 + 4 * kg);       // 2^e of tokens 4 kg .. 4 kg + 3 for this k-block
        const float sv[4] = {s4.x, s4.y, s4.z, s4.w};
#pragma unroll
        for (int v = 0; v < 4; ++v) y[mt][v] = fmaf(sv[v], fmaf(d, acc[mt][v], ndmin * t1[v]), y[mt][v]);
    }
}

#define Q5G_NC 8        // waves = row tiles per workgroup
// the image of one k-block is NCH 1-KiB chunks; wave w copies chunks w, w + 8, ... (a wave past the last chunk re-reads it: the
// load count stays static, only the store is guarded)
template <int NCH, int NI>
__device__ __forceinline__ void q5g_img_fetch(uint4 (&st)[NI], const uint8_t* __restrict__ src, int wave, int lane) {
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int c = wave + Q5G_NC * i;
        st[i] = *reinterpret_cast<const uint4*>(src + (size_t)(c < NCH ? c : NCH - 1) * 1024 + lane * 16);
    }
}
template <int NCH, int NI>
__device__ __forceinline__ void q5g_img_put(const uint4 (&st)[NI], uint8_t* dst, int wave, int lane) {
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int c = wave + Q5G_NC * i;
        if (c < NCH) *reinterpret_cast<uint4*>(dst + (size_t)c * 1024 + lane * 16) = st[i];
    }
}
// hipcc for gfx950, -O3: MT = 1: 72 VGPRs (7 waves per SIMD), MT = 2: 85 VGPRs (5), no scratch; LDS 18 / 36 KiB (two stages of
// 9 / 18 KiB): two 8-wave workgroups per CU at the least.
template <int MT>
__global__ void __launch_bounds__(512) q5g_gemm_kernel(const QmmArgs a, const uint8_t* __restrict__ img, float* __restrict__ part,
                                                       const int ldp, const int n_slots) {
    extern __shared__ __attribute__((aligned(1024))) uint8_t smem[];
    if (a.rows_dev && *a.rows_dev <= a.rows_min) return;
    constexpr int BP = MT * 16;
    constexpr size_t KBB = (((size_t)MT * (16 * 32 * 16 + 512 + 64)) + 1023) / 1024 * 1024;   // = qw1_kb_bytes(MT)
    constexpr int NCH = (int)(KBB / 1024), NI = (NCH + Q5G_NC - 1) / Q5G_NC;                  // 1-KiB chunks of a stage; per wave
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nkb = a.K >> 8;
    const int kb_per = (nkb + gridDim.y - 1) / gridDim.y;
    const int kb_lo = blockIdx.y * kb_per, kb_hi = min(nkb, kb_lo + kb_per);                  // never empty: the launcher normalises the split
    int slot = blockIdx.x * Q5G_NC + wave;
    const bool have = slot < n_slots;
    if (!have) slot = 0;                                               // a wave without a tile still copies its share of the image
    int t = slot, sg = 0;
    while (sg + 1 < a.nseg && t >= a.seg[sg].n_tiles) { t -= a.seg[sg].n_tiles; ++sg; }
    const uint8_t* wbase = a.seg[sg].w + (size_t)t * nkb * Q5K_TILE;
    uint4 st[NI];
    float y[MT][4];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int v = 0; v < 4; ++v) y[mt][v] = 0.f;
    q5g_img_fetch<NCH, NI>(st, img + (size_t)kb_lo * KBB, wave, lane);
    TileRegs cur = q5k_load_tile<false>(MI355_GGML_Q5_K, wbase + (size_t)kb_lo * Q5K_TILE, lane);
    q5g_img_put<NCH, NI>(st, smem, wave, lane);
    __syncthreads();
    for (int kb = kb_lo; kb < kb_hi; ++kb) {
        const int buf = (kb - kb_lo) & 1;
        const bool more = kb + 1 < kb_hi;
        q5g_img_fetch<NCH, NI>(st, img + (size_t)(more ? kb + 1 : kb) * KBB, wave, lane);   // lands in registers under the MFMAs below
        const TileRegs nxt = q5k_load_tile<false>(MI355_GGML_Q5_K, more ? wbase + (size_t)(kb + 1) * Q5K_TILE : wbase, more ? lane : 0);
        q5g_unit<MT>(cur, smem + (size_t)buf * KBB, lane, y);
        if (more) q5g_img_put<NCH, NI>(st, smem + (size_t)(buf ^ 1) * KBB, wave, lane);   // the stage every wave left at the previous barrier
        cur = nxt;
        __syncthreads();
    }
    const int kg = lane >> 4, rr = lane & 15;
    if (have) {
        float* pp = part + (size_t)blockIdx.y * BP * ldp + (size_t)slot * 16 + rr;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int v = 0; v < 4; ++v) pp[(size_t)(16 * mt + 4 * kg + v) * ldp] = y[mt][v];
    }
}
