"""Q5_K on the GPU: both kernels, the refusals and a Q5_K_M-shaped file against an f64 dequantisation by the ggml formula written out here."""
import ctypes
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import kquants as kq          # noqa: E402
from oracle import llama                  # noqa: E402
from oracle import ops as O               # noqa: E402

Q5 = 13
NARROW_TOL, WIDE_TOL = 1e-4, 5e-4         # <= 8 tokens: hi + lo bf16 activations ; >= 9: one f16 plane (tests/test_gpu_ops.py:47)


@pytest.fixture(scope="module")
def cv(lib):
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    import candle_vllm_amd.ops as ops
    return ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rel_err(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / max(1e-30, np.abs(ref).max()))


def rms_norm64(x, nw, eps=1e-5):
    x = x.astype(np.float64)
    return x / np.sqrt((x * x).mean(-1, keepdims=True) + eps) * nw


def q4k_as_q5k(raw):
    """Q4_K blocks -> the same weights as Q5_K blocks: 32 zero fifth-bit bytes after d, dmin, scales[12]"""
    b = np.asarray(raw, np.uint8).reshape(-1, 144)
    return np.concatenate([b[:, :16], np.zeros((len(b), 32), np.uint8), b[:, 16:]], 1).reshape(-1)


def dequant_q5k(blocks):
    """uint8 [N, K/256, 176] = f16 d, dmin | scales[12] | qh[32] | qs[128]  ->  f64 [N, K]"""
    d = blocks[..., 0:2].copy().view(np.float16)[..., 0].astype(np.float64)
    dmin = blocks[..., 2:4].copy().view(np.float16)[..., 0].astype(np.float64)
    s, qh, qs = (blocks[..., a:b].astype(np.int64) for a, b in ((4, 16), (16, 48), (48, 176)))
    sc = np.concatenate([s[..., 0:4] & 63, (s[..., 8:12] & 15) | ((s[..., 0:4] >> 6) << 4)], -1)
    m = np.concatenate([s[..., 4:8] & 63, (s[..., 8:12] >> 4) | ((s[..., 4:8] >> 6) << 4)], -1)
    g = qs.reshape(qs.shape[:-1] + (4, 1, 32))
    nib = np.concatenate([g & 15, g >> 4], -2).reshape(qs.shape[:-1] + (8, 32))          # sub-block j = 2 (group) + (nibble)
    q = nib | (((qh[..., None, :] >> np.arange(8)[:, None]) & 1) << 4)
    w = d[..., None, None] * sc[..., None] * q - dmin[..., None, None] * m[..., None]
    return w.reshape(blocks.shape[0], -1)


@functools.lru_cache(maxsize=None)
def case(n, k, payload="random", salt=0):
    """random bytes hit every code point, scale pattern and fifth-bit pattern; "ff": sc = m = 63, q = 31 (63 * 31 = 1953)"""
    rng = np.random.default_rng(n * 7919 + k + salt)
    b = rng.integers(0, 256, (n, k // 256, 176), dtype=np.uint8)
    if payload == "ff":
        b[..., 4:] = 0xFF
    b[..., 0:4] = (rng.uniform(0.5, 2, (n, k // 256, 2)) * 1e-3).astype(np.float16).view(np.uint8).reshape(n, k // 256, 4)
    return b, dequant_q5k(b)


def test_dequantize_and_native_reference_kernel(cv):
    b, w = case(40, 1024)
    m = cv.QMatMul(b, Q5, "cuda")
    assert rel_err(m.dequantize().cpu().numpy(), w) < 1e-6
    x = np.random.default_rng(2).normal(size=(3, 1024)).astype(np.float32)
    assert rel_err(m.forward_ref(dev(x)).cpu().numpy(), x.astype(np.float64) @ w.T) < 1e-5


# (1, 32768, 256): two tiles per workgroup without a pair ; (1, 64, 16 / 57 k-blocks): the ring depths of an earlier NaN defect
SHAPES = [(1, 64, 256), (1, 40, 512), (1, 4096, 4096), (1, 32768, 256), (1, 64, 4096), (1, 64, 14592), (3, 128, 4096),
          (5, 32, 14336), (8, 256, 2048), (9, 64, 512), (33, 96, 4096), (130, 40, 512), (300, 272, 256)]


@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("T,N,K,payload", [s + ("random",) for s in SHAPES] + [(2, 64, 256, "ff"), (17, 64, 512, "ff")])
def test_forward(cv, T, N, K, payload, bias):
    b, w = case(N, K, payload)
    m = cv.QMatMul(b, Q5, "cuda")
    rng = np.random.default_rng(T)
    x = rng.normal(size=(T, K)).astype(np.float32)
    bv = rng.normal(size=N).astype(np.float32) if bias else None
    got = m.forward(dev(x), dev(bv) if bias else None).cpu().numpy()
    ref = x.astype(np.float64) @ w.T
    tol = NARROW_TOL if T <= 8 else WIDE_TOL
    err = rel_err(got, ref + (bv if bias else 0))
    err_ref = rel_err(got - (bv if bias else 0), m.forward_ref(dev(x)).cpu().numpy().astype(np.float64))
    print(f"T={T} N={N} K={K} {payload}: rel_err {err:.3e}, against the native kernel {err_ref:.3e}")
    assert np.isfinite(got).all() and err < tol and err_ref < tol + 1e-5


@pytest.mark.parametrize("T", [1, 5, 12])
def test_fused_norm_qkv_rope_cache(cv, T):
    """RMSNorm + [Q5_K q, Q5_K k, Q6_K v] + interleaved RoPE + cache write (the q | k | v launch of a Q5_K_M layer)"""
    rng = np.random.default_rng(14)
    hid, H, Hkv, D, bs, NB = 1024, 8, 2, 128, 64, 6
    (bq, wq), (bk, wk) = case(H * D, hid), case(Hkv * D, hid)
    bv = kq.quantize(rng.normal(0, 0.05, (Hkv * D, hid)).astype(np.float32), kq.GGML_Q6_K)
    wv = np.asarray(kq.dequantize_q6_k(bv), np.float64).reshape(Hkv * D, hid)
    mats = [cv.QMatMul(w, t, "cuda") for w, t in ((bq, Q5), (bk, Q5), (bv, kq.GGML_Q6_K))]
    x = rng.normal(size=(T, hid)).astype(np.float32)
    nw = (1 + rng.normal(0, 0.1, hid)).astype(np.float32)
    pos = rng.integers(0, 500, T).astype(np.int64)
    slots = rng.permutation(NB * bs)[:T].astype(np.int64)
    cos, sin = O.rope_tables(500000.0, D, 512)
    xn = rms_norm64(x, nw)
    q = O.rope_apply((xn @ wq.T).reshape(T, H, D), cos, sin, pos, True)
    k = O.rope_apply((xn @ wk.T).reshape(T, Hkv, D), cos, sin, pos, True)
    v = (xn @ wv.T).reshape(T, Hkv, D)
    for flash in (True, False):
        ks, vs = O.kv_cache_shapes(NB, bs, Hkv, D, 2, flash)
        kc, vc = rng.integers(0, 65536, ks).astype(np.uint16), rng.integers(0, 65536, vs).astype(np.uint16)
        kcd, vcd = (dev(c.view(np.int16)).view(torch.bfloat16) for c in (kc, vc))
        q_out = torch.zeros((T, H * D), dtype=torch.bfloat16, device="cuda")
        cv.qmatmul_fused(mats, dev(x), epilogue=cv.EPI_QKV_ROPE_CACHE, norm_weight=dev(nw), norm_eps=1e-5,
                         rope=dict(cos=dev(cos), sin=dev(sin), positions=dev(pos), slot_mapping=dev(slots), q_out=q_out,
                                   key_cache=kcd, value_cache=vcd, num_heads=H, num_kv_heads=Hkv, head_dim=D))
        assert np.abs(q_out.float().cpu().numpy().reshape(T, H, D) - O.round_bf16(q)).max() <= 2 ** -7 * np.abs(q).max()
        kref, vref = kc.copy(), vc.copy()
        O.reshape_and_cache(O.f32_to_bf16_bits(k.astype(np.float32)), O.f32_to_bf16_bits(v.astype(np.float32)), kref, vref, slots, flash)
        gk, gv = (t.view(torch.int16).cpu().numpy().view(np.uint16) for t in (kcd, vcd))
        wk_, wv_ = kref != kc, vref != vc
        assert np.array_equal(gk[~wk_], kc[~wk_]) and np.array_equal(gv[~wv_], vc[~wv_])       # untouched slots: bit-identical
        assert np.abs(O.bf16_bits_to_f32(gk[wk_]) - O.bf16_bits_to_f32(kref[wk_])).max() <= 2 ** -7 * np.abs(k).max()
        assert np.abs(O.bf16_bits_to_f32(gv[wv_]) - O.bf16_bits_to_f32(vref[wv_])).max() <= 2 ** -7 * np.abs(v).max()


@pytest.mark.parametrize("T", [1, 5, 12])
def test_fused_silu_pair_and_bf16_residual(cv, T):
    rng = np.random.default_rng(15)
    hid, I = 1024, 512
    (bg, wg), (bu, wu), (bd, wd) = case(I, hid), case(I, hid, salt=1), case(hid, I)
    mg, mu, md = (cv.QMatMul(b, Q5, "cuda") for b in (bg, bu, bd))
    x = rng.normal(size=(T, hid)).astype(np.float32)
    nw = (1 + rng.normal(0, 0.1, hid)).astype(np.float32)
    h = torch.empty((T, I), dtype=torch.float32, device="cuda")
    cv.qmatmul_fused([mg, mu], dev(x), epilogue=cv.EPI_SILU_MUL, out=h, norm_weight=dev(nw), norm_eps=1e-5)
    g, u = rms_norm64(x, nw) @ wg.T, rms_norm64(x, nw) @ wu.T
    tol = NARROW_TOL if T <= 8 else 2 * WIDE_TOL                      # silu(g) * u multiplies two single-plane products
    assert rel_err(h.cpu().numpy(), g / (1 + np.exp(-g)) * u) < tol
    hb = h.to(torch.bfloat16)                                         # down projection: bf16 activations, out aliases the residual
    res = dev(x.copy())
    cv.qmatmul_fused([md], hb, epilogue=cv.EPI_RESID, out=res, residual=res)
    assert rel_err(res.cpu().numpy(), x + hb.float().cpu().numpy().astype(np.float64) @ wd.T) < (NARROW_TOL if T <= 8 else WIDE_TOL)


@pytest.mark.parametrize("what", ["moe_expert_ids", "group_count", "parity_mode_2"])
def test_refusals_compute_nothing(cv, lib, what):
    from candle_vllm_amd.ops import QmmDesc, _dev, _stream
    m = cv.QMatMul(case(64, 256)[0], Q5, "cuda")
    x, ids = dev(np.ones((2, 256), np.float32)), dev(np.zeros(2, np.int32))
    out = torch.full((2, 64), -7.0, dtype=torch.float32, device="cuda")
    d = QmmDesc()
    d.nseg, d.x, d.x_dtype, d.ldx, d.k, d.num_tokens = 1, _dev(x), cv.DT_F32, 256, 256, 2
    d.w_tiles[0], d.ggml_type[0], d.n_rows[0] = _dev(m.tiles), Q5, 64
    d.epilogue, d.out, d.ldo = cv.EPI_STORE, _dev(out), 64
    if what == "moe_expert_ids":
        d.moe_expert_ids, d.moe_pairs, d.moe_x_div = _dev(ids), 2, 1
    elif what == "group_count":
        d.group_count = 2
    else:
        lib.mi355_internal_qmm_set_exact(1)
    try:
        rc = lib.mi355_qmatmul_fused(ctypes.byref(d), _stream())
    finally:
        lib.mi355_internal_qmm_set_exact(0)
    torch.cuda.synchronize()
    assert rc == 801 and bool((out == -7.0).all())


@pytest.mark.parametrize("what,B,windows", [("q4k_resid", 41, (32, 9)), ("q5k_silu_pair", 41, (32, 9)), ("mixed_qkv_rope_cache", 19, (8, 8, 3))])
def test_one_call_equals_calls_on_its_token_windows(cv, what, B, windows):
    """One mi355_qmatmul_fused call of B tokens is cut into windows of tokens: 32, then 9..32 for Q4_K / Q6_K and for pure Q5_K launches,
    8-token windows where Q5_K is mixed with other types.  Tiles per workgroup, waves and the k-split do not depend on B, so the
    sub-launches are the same launches as separate calls on those windows: every output must be BIT-identical.  Distinct positions and
    slots: a window whose positions / slot_mapping / q_out offset is off writes other cache slots or rotates by another angle.
    (ops.qmatmul_fused never requests a chain: chain_next = 0 throughout.)"""
    assert sum(windows) == B
    rng = np.random.default_rng(41)
    K, N = 512, 64
    q4 = lambda: cv.QMatMul(kq.quantize(rng.normal(0, 0.05, (N, K)).astype(np.float32), kq.GGML_Q4_K), kq.GGML_Q4_K, "cuda")
    q6 = lambda: cv.QMatMul(kq.quantize(rng.normal(0, 0.05, (N, K)).astype(np.float32), kq.GGML_Q6_K), kq.GGML_Q6_K, "cuda")
    q5 = lambda salt: cv.QMatMul(case(N, K, salt=salt)[0], Q5, "cuda")
    x = dev(rng.normal(size=(B, K)).astype(np.float32))
    starts = np.concatenate([[0], np.cumsum(windows)[:-1]])

    if what != "mixed_qkv_rope_cache":
        mats = [q4()] if what == "q4k_resid" else [q5(0), q5(1)]
        epi = cv.EPI_RESID if what == "q4k_resid" else cv.EPI_SILU_MUL
        res = dev(rng.normal(size=(B, N)).astype(np.float32))

        def run(lo, hi, out):
            cv.qmatmul_fused(mats, x[lo:hi], epilogue=epi, out=out[lo:hi], residual=res[lo:hi] if epi == cv.EPI_RESID else None)
        whole, parts = (torch.full((B, N), -7.0, dtype=torch.float32, device="cuda") for _ in range(2))
        run(0, B, whole)
        for b0, bn in zip(starts, windows):
            run(int(b0), int(b0 + bn), parts)
        torch.cuda.synchronize()
        assert np.isfinite(whole.cpu().numpy()).all() and not bool((whole == -7.0).any())
        assert torch.equal(whole, parts)
        return

    mats = [q5(0), q4(), q6()]                                          # q (Q5_K) | k (Q4_K) | v (Q6_K): the 8-token mixed kernel
    H, Hkv, D, bs, NB = 1, 1, 64, 64, 2
    nw = dev((1 + rng.normal(0, 0.1, K)).astype(np.float32))
    pos = dev(rng.permutation(500)[:B].astype(np.int64))
    slots = dev(rng.permutation(NB * bs)[:B].astype(np.int64))
    cos, sin = (dev(t) for t in O.rope_tables(500000.0, D, 512))
    ks, vs = O.kv_cache_shapes(NB, bs, Hkv, D, 2, True)
    kc0, vc0 = rng.integers(0, 65536, ks).astype(np.uint16), rng.integers(0, 65536, vs).astype(np.uint16)
    got = []
    for cuts in ([(0, B)], [(int(b0), int(b0 + bn)) for b0, bn in zip(starts, windows)]):
        kcd, vcd = (dev(c.view(np.int16)).view(torch.bfloat16) for c in (kc0, vc0))
        q_out = torch.zeros((B, H * D), dtype=torch.bfloat16, device="cuda")
        for lo, hi in cuts:
            cv.qmatmul_fused(mats, x[lo:hi], epilogue=cv.EPI_QKV_ROPE_CACHE, norm_weight=nw, norm_eps=1e-5,
                             rope=dict(cos=cos, sin=sin, positions=pos[lo:hi], slot_mapping=slots[lo:hi], q_out=q_out[lo:hi],
                                       key_cache=kcd, value_cache=vcd, num_heads=H, num_kv_heads=Hkv, head_dim=D))
        torch.cuda.synchronize()
        got.append([t.view(torch.int16).cpu().numpy() for t in (q_out, kcd, vcd)])
    assert (got[0][1] != kc0.view(np.int16)).sum() > B * Hkv * D // 2 and bool(got[0][0].any())   # the call did write the cache and q
    for a, b in zip(*got):
        assert np.array_equal(a, b)


def test_q5km_model_file(lib, tmp_path):
    """the tiny Q4_K_M Llama with every Q4_K tensor re-encoded as Q5_K (zero fifth bits: bit-identical weights, so the oracle
    on the original weights is exact): a 24-token prompt step, then 8 greedy steps, eager and as a replayed graph"""
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    from candle_vllm_amd import model as M
    from oracle import gguf_writer as GW
    cfg = llama.LlamaConfig.tiny()
    W = dict(llama.make_weights(cfg, seed=1234, recipe="q4_k_m"))
    W["tok_embd"] = kq.dequantize_q6_k(kq.quantize(W["tok_embd"], kq.GGML_Q6_K)).reshape(cfg.vocab, cfg.hidden).astype(np.float32)
    path = os.path.join(tmp_path, "q5km.gguf")
    md, ts = GW.llama_to_gguf(path, cfg, W)
    t5 = [(name, Q5, q4k_as_q5k(raw), dims) if t == 12 else (name, t, raw, dims) for name, t, raw, dims in ts]
    assert sum(t == Q5 for _, t, _, _ in t5) >= 4 * cfg.n_layers
    GW.write_gguf(path, md, t5)
    gm = M.GGUFLLaMa.from_gguf(path, max_batch=4, max_blocks_per_seq=16, block_size=cfg.block_size, kv_layout=M.KV_FLASH)
    gm.alloc_kv_cache(16)
    orc = llama.OracleLlama(cfg, W)
    rng = np.random.default_rng(5)
    steps, blocks = 8, [3, 7, 2, 9][: -(-(24 + 9) // cfg.block_size)]
    seq = {"tokens": [int(t) for t in rng.integers(0, cfg.vocab, 24)], "block_table": blocks}
    cache, meta = orc.new_cache(16), O.prepare_prompt([seq], cfg.block_size)
    ref = orc.forward(meta, cache, is_prefill=True)
    got = gm.forward_prefill(meta).cpu().numpy()
    rel = float(np.abs(got - ref).max() / np.abs(ref).max())
    print(f"prompt logits rel_err {rel:.3e}")
    assert rel < 3e-3 and int(got[0].argmax()) == int(ref[0].argmax())       # tests/test_gpu_model.py: the Q4_K_M file's bound
    seq["tokens"].append(int(ref[0].argmax()))
    tok0, len0 = [seq["tokens"][-1]], [len(seq["tokens"])]
    want = []
    for _ in range(steps):
        want.append([int(orc.forward(O.prepare_decode([seq], cfg.block_size), cache)[0].argmax())])
        seq["tokens"].append(want[-1][0])
    bt, stream = np.asarray([blocks], np.uint32), torch.cuda.Stream()
    for use_graph in (False, True):
        gm.forward_prefill(meta)                                             # the prompt's K/V again: both runs start alike
        gm.set_graph(use_graph)
        gm.decode_begin(tok0, len0, bt, ctx_cap=len0[0] + steps, stream=stream.cuda_stream)
        run = []
        for _ in range(steps):
            gm.decode_step(stream.cuda_stream)
            run.append([int(t) for t in gm.read_tokens(stream.cuda_stream)])
        assert run == want, (use_graph, run, want)
