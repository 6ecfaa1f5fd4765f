"""Q5_K prompt steps (>= 192 tokens): the Q5_K arms of the prompt-step GEMM behind `QMatMul.forward` / `qmatmul_fused`, against the f64
dequantisation by the ggml formula (helpers and bounds of tests/test_gpu_q5k.py)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import candle_vllm_amd                                                # noqa: E402
from oracle import kquants as kq                                      # noqa: E402
from oracle import ops as O                                           # noqa: E402
from tests import test_gpu_q5k as small                               # noqa: E402
from tests.test_gpu_q5k import NARROW_TOL, Q5, WIDE_TOL, case, cv, dev, rel_err, rms_norm64   # noqa: E402,F401

# Q5P_MIN_TOKENS (csrc/qmm_q5k.inc): the fewest tokens of a Q5_K launch routed to the prompt GEMM.  Not the 96 of the other types: the
# Llama-3-8B down projection loses to the 32-token chunks at 96 and 128 tokens (184 against 107 / 142 us) and wins from 192 on.
T_MIN = 192
T_ODD = T_MIN + 2       # a fourth 64-token block with 2 live tokens (T_MIN itself: three full blocks)
# N = 40: the last tile is partly padding; 272 = 17 tiles: the second row block has one live tile.  K = 256: one k-block, every prefetch
# clamped; 768: both sum stages and the image ring wrap; 2048: steady state.
CASES = [(T_MIN, 40, 256), (T_MIN, 272, 768), (T_MIN, 40, 2048), (T_MIN, 272, 2048), (T_ODD, 272, 256), (T_ODD, 40, 768),
         (T_ODD, 272, 768), (T_ODD, 40, 2048)]


@pytest.mark.parametrize("T,N,K,payload,bias", [c + ("random", i % 2 == 1) for i, c in enumerate(CASES)] +
                         [(T_ODD, 40, 768, "ff", False), (T_ODD, 40, 768, "ff", True)])   # ff: sc = m = 63, q = 31 (63 * 31 = 1953)
def test_forward(cv, T, N, K, payload, bias):
    b, w = case(N, K, payload)
    rng = np.random.default_rng(T)
    x = rng.normal(size=(T, K)).astype(np.float32)
    bv = rng.normal(size=N).astype(np.float32) if bias else None
    got = cv.QMatMul(b, Q5, "cuda").forward(dev(x), dev(bv) if bias else None).cpu().numpy()
    err = rel_err(got, x.astype(np.float64) @ w.T + (bv if bias else 0))
    print(f"T={T} N={N} K={K} {payload} bias={bias}: rel_err {err:.3e}")
    assert np.isfinite(got).all() and err < WIDE_TOL


def test_forward_exact_activations(cv):
    """key 24 = 1: hi + lo activation planes through the register-fed kernel, the bound of two planes"""
    b, w = case(272, 2048)
    x = np.random.default_rng(130).normal(size=(T_ODD, 2048)).astype(np.float32)
    with candle_vllm_amd.tuning(24, 1):
        got = cv.QMatMul(b, Q5, "cuda").forward(dev(x)).cpu().numpy()
    err = rel_err(got, x.astype(np.float64) @ w.T)
    print(f"exact activations: rel_err {err:.3e}")
    assert err < NARROW_TOL


@pytest.mark.parametrize("T", [T_ODD, 1024])                          # type runs + epilogue launch ; fused store loop, Q6_K v in its own launch
def test_fused_norm_qkv_rope_cache(cv, T):
    rng = np.random.default_rng(14)
    hid, H, Hkv, D, bs, NB = 1024, 8, 2, 128, 64, 17
    (bq, wq), (bk, wk) = case(H * D, hid), case(Hkv * D, hid)
    bv = kq.quantize(rng.normal(0, 0.05, (Hkv * D, hid)).astype(np.float32), kq.GGML_Q6_K)
    wv = np.asarray(kq.dequantize_q6_k(bv), np.float64).reshape(Hkv * D, hid)
    mats = [cv.QMatMul(w, t, "cuda") for w, t in ((bq, Q5), (bk, Q5), (bv, kq.GGML_Q6_K))]
    x = rng.normal(size=(T, hid)).astype(np.float32)
    nw = (1 + rng.normal(0, 0.1, hid)).astype(np.float32)
    pos, slots = rng.integers(0, 500, T).astype(np.int64), rng.permutation(NB * bs)[:T].astype(np.int64)
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
        # written positions from the slots alone: with 1024 tokens a few new values equal the random old ones, so "kref != kc" misses them
        wk_, wv_ = np.zeros(ks, np.uint16), np.zeros(vs, np.uint16)
        O.reshape_and_cache(np.full(k.shape, 1, np.uint16), np.full(v.shape, 1, np.uint16), wk_, wv_, slots, flash)
        wk_, wv_ = wk_ != 0, wv_ != 0
        assert np.array_equal(gk[~wk_], kc[~wk_]) and np.array_equal(gv[~wv_], vc[~wv_])       # untouched slots: bit-identical
        assert np.abs(O.bf16_bits_to_f32(gk[wk_]) - O.bf16_bits_to_f32(kref[wk_])).max() <= 2 ** -7 * np.abs(k).max()
        assert np.abs(O.bf16_bits_to_f32(gv[wv_]) - O.bf16_bits_to_f32(vref[wv_])).max() <= 2 ** -7 * np.abs(v).max()


def test_fused_silu_pair_and_bf16_residual(cv):
    """the SiLU gate|up pair and the bf16-input residual down projection: body and bounds (2 WIDE_TOL, WIDE_TOL) of the decode-size test"""
    small.test_fused_silu_pair_and_bf16_residual(cv, T_ODD)


def test_block_table_is_still_refused(cv, lib):
    from candle_vllm_amd.ops import QmmDesc, _dev, _stream
    m = cv.QMatMul(case(64, 256)[0], Q5, "cuda")
    x, tab = dev(np.ones((T_MIN, 256), np.float32)), dev(np.array([[0, 64], [0, 128], [0, 192]], np.int32))
    out = torch.full((T_MIN, 64), -7.0, dtype=torch.float32, device="cuda")
    d = QmmDesc()
    d.nseg, d.x, d.x_dtype, d.ldx, d.k, d.num_tokens = 1, _dev(x), cv.DT_F32, 256, 256, T_MIN
    d.w_tiles[0], d.ggml_type[0], d.n_rows[0] = _dev(m.tiles), Q5, 64
    d.epilogue, d.out, d.ldo, d.group_block_table = cv.EPI_STORE, _dev(out), 64, _dev(tab)
    rc = lib.mi355_qmatmul_fused(ctypes.byref(d), _stream())
    torch.cuda.synchronize()
    assert rc == 801 and bool((out == -7.0).all())
