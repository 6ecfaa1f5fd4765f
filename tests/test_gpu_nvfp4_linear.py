"""NVFP4 (e2m1 elements, e4m3 scale per 16 k, f32 scale per tensor) linears (`LnNvfp4`, linear.rs:1760-1943) through `Nvfp4Linear` /
`DenseLlama.set_nvfp4`: the op against an f64 product of the exactly decoded weights, the fused epilogues, NaN scales, the refusals, and a
tiny all-NVFP4 Llama through prompt, decode and the captured greedy loop.  Route edges of csrc/nvfp4_linear.hip: 16 | 17 tokens (one / two
M tiles of the streaming kernel); from 33 tokens the GEMM when its grid has 128 workgroups or T > 96, else 32-token chunks."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import dense_llama as DL                                            # noqa: E402
from oracle import gptq as G                                                    # noqa: E402
from oracle import ops as O                                                     # noqa: E402
from tests.test_gpu_linear import check_ulp, cv, dev16, host16                  # noqa: E402,F401

MAG = np.array([0, 0.5, 1, 1.5, 2, 3, 4, 6], np.float64)
E2M1 = np.concatenate([MAG, -MAG])                                              # code = sign << 3 | magnitude index
_c = np.arange(127)                                                             # e4m3fn codes 0x00 .. 0x7E: subnormals m/8 * 2^-6, then (1 + m/8) * 2^(e-7)
E4M3 = np.where(_c < 8, (_c & 7) / 8.0 * 2.0 ** -6, (1 + (_c & 7) / 8.0) * 2.0 ** ((_c >> 3) - 7.0))
GS, GS_UP = 0.0123, 0.0123 * 0.7                                                # global scales: no powers of two, nor is their ratio


def pack(codes):
    return (codes[:, 0::2] | (codes[:, 1::2] << 4)).astype(np.uint8)            # element 2j in the low nibble of byte j


def case(N, K):
    """codes cycling through all 16 (-0 included, a different phase per row), scale bytes cycling through all 127 codes 0x00 .. 0x7E (zero
    and the subnormals included, a different phase per row and group), and the dequantised f64 matrix without the global scale"""
    codes = ((np.arange(N * K) + 7 * (np.arange(N * K) // K)) % 16).reshape(N, K).astype(np.uint8)
    s = ((np.arange(N * K // 16) + 11 * (np.arange(N * K // 16) // (K // 16))) % 127).reshape(N, K // 16).astype(np.uint8)
    return pack(codes), s, E2M1[codes] * np.repeat(E4M3[s], 16, 1)


def nv4(cv, b, s, g=GS, bias=None, g_up=None):
    return cv.Nvfp4Linear(torch.from_numpy(b).cuda(), torch.from_numpy(s).cuda(), g, bias, g_up)


# one tile and one k-block; N = 144 / 272: a ragged GEMM tile behind one / two full ones; K = 384: an odd k-block count; T on both sides of
# every route edge -- 16 | 17, 32 | 33 (a second chunk of one token), 96 | 97 (three chunks | the GEMM), and at 33 tokens 127 | 128 GEMM
# workgroups (N = 16256 | 16384: chunks | the GEMM); (130, 272, 384): ragged GEMM tiles; (300, 272, 1024): three token tiles, steady K loop;
# (130, 144, 2176): 17 k-blocks = the GEMM's LDS scale buffers (8 k-blocks each) turn over twice, the last chunk ragged.
# The streaming kernel's 8 waves split the k-blocks and keep a ring of 8, so only a long K leaves its prologue (one tile keeps these small):
# (1, 16, 10368): 81 k-blocks = 10 per wave with a ragged tail, the ring refilled and wrapped, one staging pass;
# (16, 16, 8448): 66 k-blocks, 2 per wave and pass, five passes, the last ragged; (32, 16, 8320): 65, 1 per wave and pass, nine passes, ragged
SHAPES = [(1, 16, 128), (1, 144, 384), (4, 272, 1024), (16, 272, 384), (17, 144, 384), (32, 272, 1024), (33, 272, 384), (96, 144, 384),
          (97, 144, 384), (33, 16256, 128), (33, 16384, 128), (130, 272, 384), (300, 272, 1024), (130, 144, 2176), (1, 16, 10368),
          (16, 16, 8448), (32, 16, 8320)]


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("T,N,K", SHAPES)
def test_nvfp4_linear_matches_f64_product(cv, dt, T, N, K):
    b, s, deq = case(N, K)
    x = G.round_dt(np.random.default_rng(T * 1000 + N).normal(0, 1, (T, K)), dt)
    y = host16(nv4(cv, b, s).forward(dev16(x, dt)), dt)
    ref = G.round_dt(GS * (x.astype(np.float64) @ deq.T), dt)
    assert np.abs(ref).max() < 65504                                            # (GS was chosen for this on the CPU: at most 972)
    print(f"T={T} N={N} K={K} {dt}: max |err| / max |ref| = {np.abs(y - ref).max() / np.abs(ref).max():.3e}")
    # both operands exact, f32 accumulation, one f32 multiply by the global scale (2^-24 relative): the dense op's own bound
    check_ulp(y, ref, dt, ulps=1.01, what="nvfp4 linear")


# one T per route with a packed [gate; up] of 144 rows each: the halves of a column sit in different tiles with different global scales
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("T,N,K", [(3, 288, 384), (20, 288, 384), (70, 288, 384), (100, 288, 384)])
def test_nvfp4_linear_fused_epilogues(cv, dt, T, N, K):
    b, s, deq = case(N, K)
    rng = np.random.default_rng(T)
    x = G.round_dt(rng.normal(0, 1, (T, K)), dt)
    bias = G.round_dt(rng.normal(0, 0.2, N), dt)
    res = G.round_dt(rng.normal(0, 1, (T, N)), dt)
    acc = x.astype(np.float64) @ deq.T
    mm = G.round_dt(GS * acc, dt)
    xd, rd = dev16(x, dt), dev16(res, dt)
    y = host16(nv4(cv, b, s, bias=dev16(bias, dt)).forward(xd, epilogue=cv.EPI_RESID, residual=rd, out=rd), dt)      # out aliases residual
    check_ulp(y, G.round_dt(G.round_dt(mm + bias, dt) + res, dt), dt, ulps=2.01, what="bias + resid", mag=mm)
    up = G.round_dt(GS_UP * acc[:, N // 2:], dt)
    y2 = host16(nv4(cv, b, s, g_up=GS_UP).forward(xd, epilogue=cv.EPI_SILU_MUL), dt)
    assert y2.shape == (T, N // 2)
    check_ulp(y2, G.silu_mul16(mm[:, :N // 2], up, dt), dt, ulps=2.01, what="silu(gate) * up", mag=up)


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("T", [1, 100])                                         # both kernels
def test_nvfp4_nan_scale_poisons_its_row_alone(cv, dt, T):
    b, s, deq = case(32, 256)
    s[21, 5], s[9, 2] = 0x7F, 0xFF                                              # an odd and an even group: both halves of the scale plane
    x = G.round_dt(np.random.default_rng(T).normal(0, 1, (T, 256)), dt)
    y = host16(nv4(cv, b, s).forward(dev16(x, dt)), dt)
    assert np.isnan(y[:, [9, 21]]).all()
    keep = ~np.isin(np.arange(32), [9, 21])
    check_ulp(y[:, keep], G.round_dt(GS * (x.astype(np.float64) @ deq[keep].T), dt), dt, ulps=1.01, what="rows beside the NaN rows")


@pytest.mark.parametrize("what,N,K,group,tdt", [("group 32", 128, 128, 32, torch.bfloat16), ("k = 192", 128, 192, 16, torch.bfloat16),
                                                ("n = 24", 24, 128, 16, torch.bfloat16), ("f32", 128, 128, 16, torch.float32)])
def test_nvfp4_linear_refuses_before_any_launch(cv, what, N, K, group, tdt):
    from candle_vllm_amd import lib
    w = torch.zeros((N, K // 2), dtype=torch.uint8, device="cuda")
    s = torch.full((N, K // 16), 0x38, dtype=torch.uint8, device="cuda")
    x = torch.ones((2, K), dtype=tdt, device="cuda")
    out = torch.full((2, N), 7.0, dtype=tdt, device="cuda")
    rc = lib.mi355_nvfp4_linear_tiled(out.data_ptr(), x.data_ptr(), w.data_ptr(), s.data_ptr(), None, None, 2, N, K, group, 1.0, 1.0,
                                      {torch.bfloat16: 2, torch.float16: 1, torch.float32: 0}[tdt], cv.EPI_STORE, 0)
    torch.cuda.synchronize()
    assert rc != 0 and bool((out == 7.0).all()), (what, rc)


def quantise(w, two_bits):
    """nearest e2m1 under the nearest e4m3 group scale; the global scale maps the tensor's largest group scale to at most 448 and has one
    (2^e) or two (1.5 * 2^e) significant bits, so that the dequantised weights (<= 6 bits * <= 2 bits) are exact in bf16"""
    n, k = w.shape
    g = w.reshape(n, k // 16, 16).astype(np.float64)
    gs = (1.5 if two_bits else 1.0) * 2.0 ** np.ceil(np.log2(np.abs(g).max() / (6 * 448)))
    s = np.maximum(np.abs(np.abs(g).max(-1)[..., None] / (6 * gs) - E4M3).argmin(-1), 1).astype(np.uint8)
    idx = np.abs(np.abs(g / (E4M3[s] * gs)[..., None])[..., None] - MAG).argmin(-1)
    codes = (idx | ((g < 0) << 3)).astype(np.uint8).reshape(n, k)
    return pack(codes), s, float(gs), (E2M1[codes].reshape(g.shape) * (E4M3[s] * gs)[..., None]).reshape(n, k).astype(np.float32)


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def test_nvfp4_llama_prompt_decode_and_greedy_graph(lib):
    """all seven projections of a tiny Llama in NVFP4, each with its own global scale (gate's 2^e, up's 1.5 * 2^e'): the dequantised
    weights are exact in bf16, so oracle.dense_llama on them is the reference; prompt (132 tokens: GEMM) and decode steps (3 tokens) at
    the bound of test_dense_llama_prompt_then_decode, then the greedy loop: graph == eager == oracle tokens"""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    from candle_vllm_amd import dense_model as M
    cfg = DL.DenseConfig.tiny()
    W = DL.make_weights(cfg)
    q4 = []
    for lw in W["layers"]:
        q4.append({})
        for name in ("wq", "wk", "wv", "wo", "w1", "w2", "w3"):
            b, s, gs, lw[name] = quantise(lw[name], name in ("wk", "wo", "w3"))
            q4[-1][name] = (b, s, gs)
    assert q4[0]["w1"][2] != q4[0]["w3"][2]
    orc = DL.OracleDenseLlama(cfg, W, flash_layout=False)
    gm = M.DenseLlama(cfg, max_batch=4, kv_layout=M.KV_PAGED)
    gm.load_oracle_weights({"tok_embd": W["tok_embd"], "output_norm": W["output_norm"], "output": W["output"],
                            "layers": [{n: v for n, v in lw.items() if n not in q4[0]} for lw in W["layers"]]})
    for l, d in enumerate(q4):
        for name, (b, s, gs) in d.items():
            gm.set_nvfp4(l, name, b, s, gs)
    with pytest.raises(RuntimeError):                                           # one format per slot
        gm.set_weight(0, "wq", W["layers"][0]["wq"])
    gm.alloc_kv_cache(16)
    # the prompt seed was chosen on the oracle alone: under these weights its top two logits tie at some step of seeds 1 - 5 and come within
    # 0.5 % of max |logit| with 11 (the MXFP4 test's); with 53 they stay at least 1.7 % apart at each of the ten steps below
    rng = np.random.default_rng(53)
    seqs = [{"tokens": [int(t) for t in rng.integers(0, cfg.vocab, 37)], "block_table": [3, 7, 2]},
            {"tokens": [int(t) for t in rng.integers(0, cfg.vocab, 5)], "block_table": [1]},
            {"tokens": [int(t) for t in rng.integers(0, cfg.vocab, 90)], "block_table": [9, 4, 5, 6, 8, 10, 11]}]
    cache = orc.new_cache(16)
    meta = O.prepare_prompt(seqs, cfg.block_size)
    ref = orc.forward(meta, cache, is_prefill=True)
    got = gm.forward(meta, is_prefill=True).cpu().numpy()
    assert _rel(got, ref) < 2e-2, _rel(got, ref)
    assert [int(r.argmax()) for r in got] == [int(r.argmax()) for r in ref]
    for step in range(2):
        for s, row in zip(seqs, ref):
            s["tokens"].append(int(row.argmax()))
        dmeta = O.prepare_decode(seqs, cfg.block_size)
        ref = orc.forward(dmeta, cache)
        got = gm.forward(dmeta).cpu().numpy()
        assert _rel(got, ref) < 2e-2, (step, _rel(got, ref))
        assert [int(r.argmax()) for r in got] == [int(r.argmax()) for r in ref]
    with pytest.raises(RuntimeError):                                           # the first step froze the weights
        gm.set_nvfp4(0, "wq", *q4[0]["wq"])
    # ---- greedy loop from the oracle's cache: 6 steps, eager then graph
    for s, row in zip(seqs, ref):
        s["tokens"].append(int(row.argmax()))
    steps, want = 6, []
    bt = np.zeros((3, 7), np.uint32)
    for i, s in enumerate(seqs):
        bt[i, :len(s["block_table"])] = s["block_table"]
    toks0, lens0 = [s["tokens"][-1] for s in seqs], [len(s["tokens"]) for s in seqs]
    o_cache = [(k.copy(), v.copy()) for k, v in cache]
    for _ in range(steps):
        lg = orc.forward(O.prepare_decode(seqs, cfg.block_size), o_cache)
        want.append([int(r.argmax()) for r in lg])
        for s, t in zip(seqs, want[-1]):
            s["tokens"].append(t)
    stream = torch.cuda.Stream()
    for use_graph in (False, True):
        for l, (kc, vc) in enumerate(cache):
            gm.kv_upload(l, kc, vc)
        gm.set_graph(use_graph)
        gm.decode_begin(toks0, lens0, bt, ctx_cap=max(lens0) + steps, stream=stream.cuda_stream)
        got = []
        for _ in range(steps):
            gm.decode_step(stream.cuda_stream)
            got.append([int(t) for t in gm.read_tokens(stream.cuda_stream)])
        assert got == want, (use_graph, got, want)
    assert gm.graph_stats()[0] >= 1

