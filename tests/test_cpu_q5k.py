"""Q5_K on the host: the load-time tile size and the GGUF dry run of a Q5_K_M-shaped file (no GPU needed)."""
import ctypes
import os

import numpy as np
import pytest

from oracle import gguf_writer as GW
from oracle import llama

Q5K_TILE = 16 * 16 + 2 * 64 * 16 + 64 * 8          # header | two nibble planes | transposed fifth bits = 2816


@pytest.mark.parametrize("n,k,want", [(64, 256, 4 * Q5K_TILE), (40, 512, 3 * 2 * Q5K_TILE), (1, 14336, 56 * Q5K_TILE),
                                      (64, 384, -1), (64, 0, -1)])
def test_repacked_size_of_q5k(lib, n, k, want):
    assert lib.mi355_qweight_repacked_size(13, n, k) == want


def test_check_gguf_accepts_q5k_tensors(lib, tmp_path):
    """every Q4_K tensor of the tiny Llama file re-typed to Q5_K (32 zero fifth-bit bytes after d, dmin, scales): served;
    a Q8_0 tensor in the same place: still 801"""
    from candle_vllm_amd._lib import LlamaConfig
    cfg = llama.LlamaConfig.tiny(hidden=512, n_heads=4, n_kv_heads=2, head_dim=128, intermediate=768, vocab=512)
    p = os.path.join(tmp_path, "q5.gguf")
    md, ts = GW.llama_to_gguf(p, cfg, llama.make_weights(cfg, seed=6))

    def check(retype8=None):
        t2 = []
        for name, t, raw, dims in ts:
            if name == retype8:
                t, raw = 8, np.zeros((dims[0] * dims[1] // 32) * 34, np.uint8)
            elif t == 12:
                b = np.asarray(raw, np.uint8).reshape(-1, 144)
                t, raw = 13, np.concatenate([b[:, :16], np.zeros((len(b), 32), np.uint8), b[:, 16:]], 1).reshape(-1)
            t2.append((name, t, raw, dims))
        GW.write_gguf(p, md, t2)
        c = LlamaConfig()
        return lib.mi355_llama_check_gguf(p.encode(), 0, 1, ctypes.addressof(c))
    assert any(t == 12 for _, t, _, _ in ts)
    assert check() == 0
    assert check(retype8="blk.0.attn_v.weight") == 801
