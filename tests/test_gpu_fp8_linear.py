"""FP8 (e4m3fn) block-scaled linears (`LnFp8`, linear.rs:918-1221) through `Fp8Linear` / `DenseLlama.set_fp8`: the op against an f64
product of the exactly decoded weights, the fused epilogues, the refusals, and a tiny all-fp8 Llama through prompt, decode and the
captured greedy loop.  Route edges of csrc/fp8_linear.hip: 16 | 17 tokens (one / two M tiles of the streaming kernel); from 33 tokens the
GEMM when its grid has 128 workgroups or T > 96, else 32-token chunks of the streaming kernel."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import dense_llama as DL                                            # noqa: E402
from oracle import gptq as G                                                    # noqa: E402
from oracle import ops as O                                                     # noqa: E402
from tests.test_gpu_linear import check_ulp, cv, dev16, host16                  # noqa: E402,F401

FINITE = np.array([c for c in range(256) if c & 0x7F != 0x7F], np.uint8)        # all 254 finite codes: subnormals and both zeros included
TINY = np.array(list(range(0x00, 0x08)) + list(range(0x80, 0x88)), np.uint8)    # only the zeros and the subnormals


def case(N, K, seed, codes=FINITE):
    """weight bytes cycling through `codes` (a different phase per row), f32 scales that are no powers of two, and the dequantised
    f64 matrix"""
    rng = np.random.default_rng(seed)
    w = codes[(np.arange(N * K) + 37 * (np.arange(N * K) // K)) % len(codes)].reshape(N, K)
    s = rng.uniform(0.5, 1.5, (-(-N // 128), K // 128)).astype(np.float32) * 2.0 ** -9
    deq = O.e4m3fn_to_f32(w).astype(np.float64) * np.repeat(np.repeat(s.astype(np.float64), 128, 0)[:N], 128, 1)
    return w, s, deq


def fp8(cv, w, s, bias=None):
    return cv.Fp8Linear(torch.from_numpy(w).cuda(), torch.from_numpy(s).cuda(), bias)


# one tile and one k-block; N = 144 / 272: a ragged last scale row behind one / two full ones; K = 384: an odd k-block count; T on both
# sides of every route edge -- 16 | 17, 32 | 33 (a second chunk of one token), 96 | 97 (three chunks | the GEMM), and at 33 tokens 127 | 128
# GEMM workgroups (N = 16256 | 16384: chunks | the GEMM); (130, 272, 384): ragged GEMM tiles; (300, 272, 1024): three token tiles, steady K loop.
# The streaming kernel's 8 waves split the k-blocks, so only a long K leaves its prologue (one tile keeps these small):
# (1, 16, 5248): 41 k-blocks = 6 per wave with a ragged tail, the 4-deep ring refilled and wrapped, one staging pass of 6 k-blocks per wave;
# (16, 16, 4224): 2 k-blocks per wave and pass, three passes, the last ragged; (32, 16, 2176): 1 per wave and pass, three passes, ragged
SHAPES = [(1, 16, 128), (1, 144, 384), (4, 272, 1024), (16, 272, 384), (17, 144, 384), (31, 272, 384), (32, 272, 1024), (33, 272, 384),
          (34, 144, 384), (96, 144, 384), (97, 144, 384), (33, 16256, 128), (33, 16384, 128), (130, 272, 384), (300, 272, 1024),
          (1, 16, 5248), (16, 16, 4224), (32, 16, 2176)]


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("T,N,K", SHAPES)
def test_fp8_linear_matches_f64_product(cv, dt, T, N, K):
    w, s, deq = case(N, K, N + K)
    x = G.round_dt(np.random.default_rng(T * 1000 + N).normal(0, 1, (T, K)), dt)
    y = host16(fp8(cv, w, s).forward(dev16(x, dt)), dt)
    ref = G.round_dt(x.astype(np.float64) @ deq.T, dt)
    print(f"T={T} N={N} K={K} {dt}: max |err| / max |ref| = {np.abs(y - ref).max() / np.abs(ref).max():.3e}")
    # both operands exact, f32 accumulation: the dense op's own bound
    check_ulp(y, ref, dt, ulps=1.01, what="fp8 linear")


@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("T", [1, 40])                                          # both kernels
def test_fp8_linear_subnormal_codes_alone(cv, dt, T):
    """weights of nothing but +-0 and the subnormals: next to +-448 a subnormal decoded as 0 would hide under the bound"""
    w, s, deq = case(16, 128, 9, TINY)
    x = G.round_dt(np.random.default_rng(T).normal(0, 1, (T, 128)), dt)
    y = host16(fp8(cv, w, s).forward(dev16(x, dt)), dt)
    check_ulp(y, G.round_dt(x.astype(np.float64) @ deq.T, dt), dt, ulps=1.01, what="subnormal codes")


# one T per route with a packed [gate; up] of 144 rows each (whole 16-row tiles): one / two M tiles, three chunks, the GEMM by T; (70, 16384,
# 128): the GEMM by its grid (128 tiles of 64 pairs); (17, 32, 2176): a pair in the streaming kernel's steady state (three staging passes)
@pytest.mark.parametrize("dt", ["bf16", "f16"])
@pytest.mark.parametrize("T,N,K", [(3, 288, 384), (20, 288, 384), (70, 288, 384), (100, 288, 384), (70, 16384, 128), (17, 32, 2176)])
def test_fp8_linear_fused_epilogues(cv, dt, T, N, K):
    w, s, deq = case(N, K, 5)
    rng = np.random.default_rng(T)
    x = G.round_dt(rng.normal(0, 1, (T, K)), dt)
    b = G.round_dt(rng.normal(0, 0.2, N), dt)
    res = G.round_dt(rng.normal(0, 1, (T, N)), dt)
    mm = G.round_dt(x.astype(np.float64) @ deq.T, dt)
    xd, rd = dev16(x, dt), dev16(res, dt)
    y = host16(fp8(cv, w, s, dev16(b, dt)).forward(xd, epilogue=cv.EPI_RESID, residual=rd, out=rd), dt)      # out aliases residual
    check_ulp(y, G.round_dt(G.round_dt(mm + b, dt) + res, dt), dt, ulps=2.01, what="bias + resid", mag=mm)
    # N = 288: gate = rows 0..143 (scale rows 0, 1), up = rows 144..287 (scale rows 1, 2): the halves of a column see different scales
    y2 = host16(fp8(cv, w, s).forward(xd, epilogue=cv.EPI_SILU_MUL), dt)
    assert y2.shape == (T, N // 2)
    check_ulp(y2, G.silu_mul16(mm[:, :N // 2], mm[:, N // 2:], dt), dt, ulps=2.01, what="silu(gate) * up", mag=mm[:, N // 2:])


@pytest.mark.parametrize("what,N,K,block,tdt", [("block 64", 128, 128, 64, torch.bfloat16), ("k = 192", 128, 192, 128, torch.bfloat16),
                                                ("n = 24", 24, 128, 128, torch.bfloat16), ("f32", 128, 128, 128, torch.float32)])
def test_fp8_linear_refuses_before_any_launch(cv, what, N, K, block, tdt):
    from candle_vllm_amd import lib
    w = torch.zeros((N, K), dtype=torch.uint8, device="cuda")
    s = torch.ones((4, 4), dtype=torch.float32, device="cuda")
    x = torch.ones((2, K), dtype=tdt, device="cuda")
    out = torch.full((2, N), 7.0, dtype=tdt, device="cuda")
    rc = lib.mi355_fp8_linear_tiled(out.data_ptr(), x.data_ptr(), w.data_ptr(), s.data_ptr(), None, None, 2, N, K, block, block,
                                    {torch.bfloat16: 2, torch.float16: 1, torch.float32: 0}[tdt], cv.EPI_STORE, 0)
    torch.cuda.synchronize()
    assert rc != 0 and bool((out == 7.0).all()), (what, rc)


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def test_fp8_llama_prompt_decode_and_greedy_graph(lib):
    """all seven projections of a tiny Llama in fp8 with power-of-two block scales: the dequantised weights are exact in bf16, so
    oracle.dense_llama on them is the reference; prompt (132 tokens: GEMM) and decode steps (3 tokens) at the bound of
    test_dense_llama_prompt_then_decode, then the greedy loop: graph == eager == oracle tokens"""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X")
    from candle_vllm_amd import dense_model as M
    cfg = DL.DenseConfig.tiny()
    W = DL.make_weights(cfg)
    q8 = []
    for lw in W["layers"]:
        q8.append({})
        for name in ("wq", "wk", "wv", "wo", "w1", "w2", "w3"):
            n, k = lw[name].shape
            br, bk = np.meshgrid(np.arange(-(-n // 128)), np.arange(k // 128), indexing="ij")
            s = (2.0 ** (-10 + (br + 2 * bk) % 3)).astype(np.float32)
            full = np.repeat(np.repeat(s, 128, 0)[:n], 128, 1)
            b = O.f32_to_e4m3fn(lw[name] / full)
            q8[-1][name] = (b, s)
            lw[name] = O.e4m3fn_to_f32(b) * full
    orc = DL.OracleDenseLlama(cfg, W, flash_layout=False)
    gm = M.DenseLlama(cfg, max_batch=4, kv_layout=M.KV_PAGED)
    gm.load_oracle_weights({"tok_embd": W["tok_embd"], "output_norm": W["output_norm"], "output": W["output"],
                            "layers": [{n: v for n, v in lw.items() if n not in q8[0]} for lw in W["layers"]]})
    for l, d in enumerate(q8):
        for name, (b, s) in d.items():
            gm.set_fp8(l, name, b, s)
    with pytest.raises(RuntimeError):                                           # one format per slot
        gm.set_weight(0, "wq", W["layers"][0]["wq"])
    gm.alloc_kv_cache(16)
    rng = np.random.default_rng(3)
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
        gm.set_fp8(0, "wq", *q8[0]["wq"])
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
